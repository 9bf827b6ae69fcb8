"""RxPlan.papr_study (ofdm_papr_study): the PAPR / CCDF study of `Task 2/Main_model_Task_2.m:69-97` as one device-resident call,
against the oracle.

Samples: `tx` equals the oracle's composition payload -> [Scrambler per frame] -> mapping -> OFDM_map_carriers -> OFDM_modulator
(oracle.tx_frame without channel and noise, composed as tests/test_gpu_txgen.py composes `want`), to that file's tolerances for
the generator's noise-free TX (1e-13 relative l2 in double, 2e-6 in single).

Counts: v = oracle.calculate_window_PAPR(signal, window) on the returned samples in double.  For every edge e the device's
exceedance count (`above` plus the bins at and above e) must lie between #(v > e + TOL_DB) and #(v > e - TOL_DB): TOL_DB = 1e-9 dB is
this algorithm's tolerance (tests/test_gpu_papr.py), and a window whose value lies that close to an edge may fall on either
side.  No case is left out of the bracket.  peak is compared exactly with max(re^2 + im^2) of the returned samples, power_sum to
1e-12 relative, PAPR_dB with oracle.calculatePAPR to TOL_DB."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_l2
import papr_cases as pc
import published

pytestmark = pytest.mark.gpu

TOL_DB = 1e-9
REG = (1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0)          # T2/Main_model_Task_2.m:36
BINS = dict(n=600, lo=0.0, hi=30.0)


def _cfg(kind):
    from ofdm_course_amd import frames as fr
    if kind == "small":
        return fr.config_small()                                                      # Nfft 256, 5 symbols
    if kind == "mid":
        return fr.config_small(nfft=1024, n_carrier=400, const="8PSK", n_symb=3)
    return fr.config_small(nfft=2048, n_carrier=512, const="64QAM", n_symb=5)         # "wide": 11520 samples per frame


_PLANS = {}


def _plan(ofdm, kind, precision="fp64"):
    from ofdm_course_amd import frames as fr
    if (kind, precision) not in _PLANS:
        cfg = _cfg(kind)
        _PLANS[kind, precision] = (cfg, fr.make_plan(cfg, ofdm, precision=precision))
    return _PLANS[kind, precision]


def _oracle_tx(ofdm, oracle, cfg, bits, Register):
    """[frame_samples] of one frame carrying `bits`: the composition of tests/test_gpu_txgen.py without channel and noise."""
    from ofdm_course_amd import frames as fr
    pv = np.repeat(fr.pilot_column(cfg, ofdm)[:, None], cfg.N_symb, axis=1)
    return oracle.tx_frame(bits, cfg.Nfft, cfg.T_guard, cfg.N_symb, cfg.dataCarriers, cfg.pilotCarriers, pv, cfg.Constellation,
                           h=None, SNR=None, Register=Register)[0]


def _power(x):
    x = np.asarray(x).astype(np.complex128)
    return x.real * x.real + x.imag * x.imag


def _exceed(out):
    hist = np.asarray(out["hist"]).astype(np.int64)
    return np.concatenate([np.cumsum(hist[::-1])[::-1], [0]]) + int(out["above"])


def _check_values(out, v, edges):
    """The bracket rule on the window values v (NaN: dropped), the conservation identity and the CCDF."""
    v = np.asarray(v, dtype=np.float64)
    nan = int(np.count_nonzero(np.isnan(v)))
    sv = np.sort(v[~np.isnan(v)])
    more = lambda x: sv.size - np.searchsorted(sv, x, side="right")                   # noqa: E731  #(v > x)
    got = _exceed(out)
    lo_cnt, hi_cnt = more(edges + TOL_DB), more(edges - TOL_DB)
    assert np.all(lo_cnt <= got) and np.all(got <= hi_cnt), (got - lo_cnt, hi_cnt - got)
    assert int(out["dropped"]) == nan
    assert int(out["windows"]) == v.size == int(np.sum(out["hist"])) + int(out["below"]) + int(out["above"]) + int(out["dropped"])
    valid = v.size - nan
    assert np.array_equal(np.asarray(out["CCDF"]), got / np.float64(valid))
    assert np.array_equal(np.asarray(out["edges"]), edges)


def _check_study(oracle, out, window, bins, n_signals):
    tx = np.asarray(out["tx"])
    assert tx.shape[1] == n_signals
    sig = [tx[:, s].astype(np.complex128) for s in range(n_signals)]
    v = np.concatenate([oracle.calculate_window_PAPR(x, window) for x in sig])
    assert v.size == n_signals * (tx.shape[0] - window + 1)
    _check_values(out, v, np.linspace(bins["lo"], bins["hi"], bins["n"] + 1))
    assert int(out["dropped"]) == 0
    for s, x in enumerate(sig):
        p = _power(x)
        assert float(out["peak"][s]) == float(np.max(p))                              # exactly
        assert abs(float(out["power_sum"][s]) - float(np.sum(p))) <= 1e-12 * float(np.sum(p))
        assert abs(float(out["PAPR_dB"][s]) - oracle.calculatePAPR(x)) <= TOL_DB


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("register", [None, REG])
@pytest.mark.parametrize("payload", ["philox", "caller"])
@pytest.mark.parametrize("kind", ["small", "mid"])
def test_samples_equal_the_oracle_composition_and_counts_follow(ofdm, oracle, kind, payload, register, precision):
    cfg, plan = _plan(ofdm, kind, precision)
    _, bps = oracle.constellation_func(cfg.Constellation)
    nsig, fps, seed, f0 = 2, 3, 0x1234ABCD5, 7
    if payload == "philox":
        bits = np.stack([oracle.payload_bits_philox(len(cfg.dataCarriers) * cfg.N_symb, bps, seed, f0 + g) for g in range(nsig * fps)])
        given = None
    else:
        bits = np.random.default_rng(11).integers(0, 2, (nsig * fps, plan.frame_bits), dtype=np.uint8)
        bits[1] = 0                                                                   # a structured frame: all zeros
        given = bits
    out = plan.papr_study(nsig, fps, seed=seed, frame0=f0, Register=register, payload_bits=given, bins=BINS, want_tx=True)
    tx = np.asarray(out["tx"])
    assert tx.shape == (fps * cfg.frame_samples, nsig) and tx.dtype == (np.complex128 if precision == "fp64" else np.complex64)
    for g in range(nsig * fps):
        want = _oracle_tx(ofdm, oracle, cfg, bits[g], register)
        got = tx[(g % fps) * cfg.frame_samples:(g % fps + 1) * cfg.frame_samples, g // fps]
        assert rel_l2(got, want) < (1e-13 if precision == "fp64" else 2e-6), (g, rel_l2(got, want))
    _check_study(oracle, out, cfg.Nfft, BINS, nsig)                                   # window defaults to Nfft


@pytest.mark.parametrize("kind,window,fps,precision", [
    ("small", 256, 1, "fp64"), ("small", 256, 3, "fp32"), ("small", 512, 3, "fp64"), ("small", 1024, 1, "fp64"),
    ("small", 1024, 3, "fp64"), ("mid", 2048, 1, "fp64"), ("wide", 2048, 1, "fp64"), ("wide", 4096, 1, "fp64"),
    ("wide", 8192, 1, "fp64"), ("wide", 8192, 2, "fp32"), ("wide", 4096, 3, "fp64")])
def test_every_kernel_form(ofdm, oracle, kind, window, fps, precision):
    """Each C of papr_hist_kernel (4: window 256; 8: 512 .. 4096) and the two-phase form (8192); windows spanning several
    symbols and their CPs (1024 on the Nfft-256 plan); a last workgroup that is partial (no window count here is a multiple of
    its window)."""
    cfg, plan = _plan(ofdm, kind, precision)
    nsig = 2 if window < 4096 else 1                          # (the oracle recomputes every window from scratch)
    assert (fps * cfg.frame_samples - window + 1) % window != 0
    out = plan.papr_study(nsig, fps, seed=5, frame0=1, Register=REG, window=window, bins=BINS, want_tx=True)
    _check_study(oracle, out, window, BINS, nsig)


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k      # bitwise


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_outputs_do_not_depend_on_the_chunking(ofdm, oracle, precision):
    cfg, plan = _plan(ofdm, "small", precision)
    kw = dict(seed=9, Register=REG, bins=BINS, want_tx=True)
    ref = plan.papr_study(5, 3, frame0=4, max_frames_per_chunk=0, **kw)
    _check_study(oracle, ref, cfg.Nfft, BINS, 5)
    for cap in (3, 6, 7):                                                             # 1, 2, 2 signals per chunk
        _same(ref, plan.papr_study(5, 3, frame0=4, max_frames_per_chunk=cap, **kw))
    # two calls over disjoint stream ranges add up to the one call over both
    a = plan.papr_study(2, 3, frame0=4, **kw)
    b = plan.papr_study(3, 3, frame0=4 + 6, **kw)
    assert np.array_equal(a["hist"] + b["hist"], ref["hist"])
    for k in ("below", "above", "dropped", "windows"):
        assert a[k] + b[k] == ref[k]
    for k in ("peak", "power_sum", "PAPR_dB"):
        assert np.array_equal(np.concatenate([a[k], b[k]]), ref[k])
    assert np.array_equal(np.concatenate([a["tx"], b["tx"]], axis=1), ref["tx"])
    # overwritten, not accumulated: an empty call gives an empty table
    z = plan.papr_study(0, 3, **kw)
    assert z["windows"] == 0 and not np.any(z["hist"]) and z["peak"].shape == (0,)


@pytest.mark.parametrize("n_bins", [7, 1])
def test_a_grid_inside_the_distribution_fills_both_tails(ofdm, oracle, n_bins):
    """The grid spans the quartiles of the oracle's own window values of these signals (composed by the oracle from the payload
    draw, nothing from the library): a quarter of the windows falls below it and a quarter at or above it."""
    cfg, plan = _plan(ofdm, "small")
    _, bps = oracle.constellation_func(cfg.Constellation)
    nsig, fps, seed = 3, 3, 2
    v = []
    for s in range(nsig):
        frames = [_oracle_tx(ofdm, oracle, cfg, oracle.payload_bits_philox(len(cfg.dataCarriers) * cfg.N_symb, bps, seed, s * fps + g), None)
                  for g in range(fps)]
        v.append(oracle.calculate_window_PAPR(np.concatenate(frames), cfg.Nfft))
    lo, hi = (float(q) for q in np.quantile(np.concatenate(v), [0.25, 0.75]))
    bins = dict(n=n_bins, lo=lo, hi=hi)
    out = plan.papr_study(nsig, fps, seed=seed, bins=bins, want_tx=True)
    _check_study(oracle, out, cfg.Nfft, bins, nsig)
    assert out["below"] > 0 and out["above"] > 0 and int(np.sum(out["hist"])) > 0


@pytest.mark.parametrize("bins", [dict(n=4096, lo=0.0, hi=32.0), dict(n=1, lo=0.0, hi=30.0)])
def test_extreme_bin_counts(ofdm, oracle, bins):
    cfg, plan = _plan(ofdm, "small")
    out = plan.papr_study(3, 3, seed=2, bins=bins, want_tx=True)
    _check_study(oracle, out, cfg.Nfft, bins, 3)
    assert out["below"] == 0 and out["above"] == 0 and int(np.sum(out["hist"])) == out["windows"]   # a PAPR lies in [0, 10 log10 W]


def _broken(plan, **brk):
    kw = dict(n_signals=2, frames_per_signal=3, Register=REG, window=256, bins=dict(BINS))
    for k, v in brk.items():
        if k in ("n", "lo", "hi"):
            kw["bins"][k] = v
        else:
            kw[k] = v
    return plan.papr_study(**kw)


@pytest.mark.parametrize("brk,msg", [
    (dict(window=768), "papr_study: window must be a power of two, 256 .. 8192 (768)"),
    (dict(window=8192), "papr_study: window 8192 exceeds the signal of 4320 samples"),
    (dict(n=0), "papr_study: n_bins must be 1 .. 4096 (0)"),
    (dict(n=4097), "papr_study: n_bins must be 1 .. 4096 (4097)"),
    (dict(lo=3.0, hi=3.0), "papr_study: lo_db and hi_db must be finite with lo_db < hi_db"),
    (dict(Register=(1, 0, 0, 2, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0)), "papr_study: register entries must be 0 or 1"),
    (dict(payload_bits=np.zeros(100, np.uint8)), "papr_study: payload_bits must hold n_signals * frames_per_signal * frame_bits = 5760 bits"),
])
def test_refusals(ofdm, brk, msg):
    _, plan = _plan(ofdm, "small")
    assert "payload_bits" in msg or msg in [m for _, _, m in pc.order(1)] + [m for _, m in pc.SINGLE]   # the host test's texts
    with pytest.raises(ofdm.OfdmError) as e:
        _broken(plan, **brk)
    assert msg in str(e.value)


def test_refusal_of_a_precision_mismatch(ofdm):
    from ofdm_course_amd import _lib as L
    _, plan = _plan(ofdm, "small")                           # a double plan called with the single-precision flag
    hist, tails = np.zeros(600, np.uint64), np.zeros(3, np.uint64)
    rc = plan.lib.ofdm_papr_study(plan.handle, 1, 0, 1, 1, None, None, 256, 600, 0.0, 30.0, 0, hist.ctypes.data_as(C.c_void_p),
                                  tails.ctypes.data_as(C.c_void_p), None, None, L.OFDM_F32)
    assert rc < 0
    assert plan.lib.ofdm_last_error_string().decode() == "papr_study: precision flag differs from the plan's"
    assert not hist.any() and not tails.any()


def test_device_flavour_gives_the_same_tables(ofdm):
    import torch
    cfg, plan = _plan(ofdm, "small", "fp32")
    kw = dict(seed=3, frame0=2, Register=REG, bins=BINS, want_tx=True)
    host = plan.papr_study(4, 3, **kw)
    dev = plan.papr_study(4, 3, device=torch.device("cuda:0"), **kw)
    for k in host:
        assert dev[k].is_cuda, k
        if k == "PAPR_dB":                                    # log10 of the device against the host's: a rounding apart
            assert np.max(np.abs(dev[k].cpu().numpy() - host[k])) < 1e-12
        else:
            assert np.array_equal(dev[k].cpu().numpy(), np.asarray(host[k])), k


def test_reference_payload_pins_the_published_figures(ofdm, oracle):
    """T2 geometry, one signal of 10 frames carrying the reference's image bits: the curves pass tests/published.py:check_papr
    (Task 2/README.md:54,:70-71) and the histogram is, under the bracket rule, the one of drivers.task2's window values."""
    from ofdm_course_amd.drivers import task2, task2_ccdf
    bits = published.eagle_bits()
    plan = task2_ccdf.make_plan(ofdm)
    need = 10 * plan.frame_bits
    rep = task2.run(ofdm, input_bits=bits)
    papr = {}
    for tag, reg in task2_ccdf.CURVES:
        out = plan.papr_study(1, 10, Register=reg, payload_bits=bits[:need].reshape(10, plan.frame_bits), window=1024, bins=BINS)
        papr[tag] = {"PAPR_dB": float(out["PAPR_dB"][0]), "PAPR_ccdf": out["edges"], "CCDF": out["CCDF"]}
        _check_values(out, rep["papr"][tag]["_PAPRs"], np.linspace(0.0, 30.0, 601))
        assert abs(papr[tag]["PAPR_dB"] - rep["papr"][tag]["PAPR_dB"]) <= TOL_DB
    published.check_papr(papr)


def test_driver_equals_the_direct_call(ofdm):
    from ofdm_course_amd.drivers import task2_ccdf
    bins = dict(n=300, lo=2.0, hi=14.0)
    res = task2_ccdf.run(signals=8, frames_per_signal=2, bins=bins, seed=6, signals_per_tile=3)
    plan = task2_ccdf.make_plan(ofdm)
    for tag, reg in task2_ccdf.CURVES:
        want = plan.papr_study(8, 2, seed=6, Register=reg, bins=bins)
        for k in want:
            assert np.array_equal(np.asarray(res[tag][k]), np.asarray(want[k])), (tag, k)
    assert res["plain"]["windows"] == 8 * (2 * 5760 - 1024 + 1)
    assert not np.array_equal(res["plain"]["hist"], res["scrambled"]["hist"])         # two curves, not one twice
