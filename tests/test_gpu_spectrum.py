"""The received-spectrum capture: rx_spectrum (ofdm_rx_spectrum) and RxPlan.spectrum_study (ofdm_spectrum_study).

Against numpy: np.fft.fft in double of the very samples handed to rx_spectrum, every transform size 64 .. 8192 in both precisions,
the tolerances of SURVEY 8(c): amp rows rel. l2 <= 1e-13 log2(Nfft) (fp64) / 1e-6 log2(Nfft) (fp32), power rows twice that.
The study against the per-frame call: bitwise.  Known answers from the oracle's own functions on noise-free frames composed as
tests/test_gpu_txgen.py composes them (oracle.tx_frame).  The refusals of tests/spectrum_cases.py, each followed by a good call."""
import numpy as np
import pytest

import spectrum_cases as sc
from conftest import rel_l2

pytestmark = pytest.mark.gpu

REG = (1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0)          # T5/Main_model_Task_5.m:55
TAPS3 = np.array([[0, 1.0], [4, 0.6], [10, 0.3]])              # T4/Main_model_Task_4.m:257-261, T3/Main_model_Task_3.m:122-126

SHAPES = {
    "n256": dict(),                                                                   # frames.config_small()
    "n1024": dict(nfft=1024, n_carrier=400, const="8PSK", n_symb=3),
    "n64": dict(nfft=64, n_carrier=32, const="QPSK", n_symb=3),
    "n128": dict(nfft=128, n_carrier=64, const="QPSK", n_symb=3),
    "n512": dict(nfft=512, n_carrier=100, const="8PSK", n_symb=2),
    "n2048": dict(nfft=2048, n_carrier=512, const="64QAM", n_symb=2),
    "n4096": dict(nfft=4096, n_carrier=1024, const="256QAM", n_symb=2),
    "n8192": dict(nfft=8192, n_carrier=600, comb=8, const="16QAM", n_symb=3),
}


def _cfg(name):
    from ofdm_course_amd import frames as fr
    return fr.config_small(**SHAPES[name])


def _tol(nfft, precision):
    return (1e-13 if precision == "fp64" else 1e-6) * np.log2(nfft)


def _reference(rx, cfg, first, nw):
    """|fft| and the summed |fft|^2 of the windows of rx [frame_samples, n_frames], numpy in double."""
    stride = cfg.Nfft + cfg.T_guard
    x = np.asarray(rx).astype(np.complex128)
    seg = np.stack([x[first + w * stride: first + w * stride + cfg.Nfft, :].T for w in range(nw)], axis=1)   # [f, w, Nfft]
    S = np.fft.fft(seg, axis=2)
    return np.abs(S), (S.real ** 2 + S.imag ** 2).sum(axis=1), seg


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_amp_and_power_against_numpy(ofdm, oracle, name, precision):
    from ofdm_course_amd import frames as fr
    cfg = _cfg(name)
    plan = fr.make_plan(cfg, ofdm, precision=precision)
    h, _ = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    per_wg = max(1, 256 // (cfg.Nfft // 8))                       # frames per workgroup: more than two workgroups, the last partial
    nfr = 2 * per_wg + 1
    rx = np.asarray(plan.tx_frames_fused(nfr, h=h, SNR=20.0, seed=5, frame0=2)["rx"])
    stride, fs, tg, ns = cfg.Nfft + cfg.T_guard, cfg.frame_samples, cfg.T_guard, cfg.N_symb
    firsts = [0, 1, tg, tg + stride, fs - cfg.Nfft, stride - cfg.Nfft // 2]     # the last: over a symbol boundary and its CP
    tol, worst_a, worst_p, calls = _tol(cfg.Nfft, precision), 0.0, 0.0, 0
    for first in firsts:
        for nw in sorted({1, 2, ns}):
            if not sc.end_ok(cfg.Nfft, tg, ns, first, nw):
                continue
            out = ofdm.rx_spectrum(plan, rx, first=first, n_windows=nw, want_power=True)
            amp, power, _ = _reference(rx, cfg, first, nw)
            assert out["amp"].shape == (nfr, nw, cfg.Nfft) and out["amp"].dtype == (np.float64 if precision == "fp64" else np.float32)
            assert out["power"].shape == (nfr, cfg.Nfft) and out["power"].dtype == np.float64
            ea = max(rel_l2(out["amp"][f, w], amp[f, w]) for f in range(nfr) for w in range(nw))
            ep = max(rel_l2(out["power"][f], power[f]) for f in range(nfr))
            worst_a, worst_p, calls = max(worst_a, ea), max(worst_p, ep), calls + 1
            print(f"{name} {precision} first={first} n_windows={nw}: amp {ea:.3e} power {ep:.3e} (tol {tol:.1e} / {2 * tol:.1e})")
            assert ea <= tol and ep <= 2 * tol, (first, nw, ea, ep)
    assert calls >= 8                                             # every first, every window count somewhere
    # first=None is T_guard (T3/Main_model_Task_3.m:138); without want_power no power row
    dflt = ofdm.rx_spectrum(plan, rx)
    assert dflt["power"] is None and np.array_equal(dflt["amp"], ofdm.rx_spectrum(plan, rx, first=tg)["amp"])
    plan.close()


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_device_flavour_and_nonfinite_samples(ofdm, precision):
    import torch
    from ofdm_course_amd import frames as fr
    cfg = _cfg("n256")
    plan = fr.make_plan(cfg, ofdm, precision=precision, device=0)
    rx = np.asarray(plan.tx_frames_fused(4, SNR=15.0, seed=8)["rx"]).copy()
    host = ofdm.rx_spectrum(plan, rx, first=33, n_windows=3, want_power=True)
    dev = ofdm.rx_spectrum(plan, torch.from_numpy(rx).cuda(), first=33, n_windows=3, want_power=True)
    assert np.array_equal(dev["amp"].cpu().numpy(), host["amp"]) and np.array_equal(dev["power"].cpu().numpy(), host["power"])
    # a NaN in window 1 of frame 2, an Inf in window 0 of frame 3: those amp rows, and the frames' power rows, are not finite
    stride = cfg.Nfft + cfg.T_guard
    rx[33 + stride + 100, 2] = np.nan
    rx[33 + 7, 3] = np.inf
    bad = ofdm.rx_spectrum(plan, rx, first=33, n_windows=3, want_power=True)
    fin = np.isfinite(bad["amp"]).all(axis=2)
    assert not np.isfinite(bad["amp"][2, 1]).any() and not np.isfinite(bad["amp"][3, 0]).any()
    assert fin[:2].all() and fin[2, 0] and fin[2, 2] and fin[3, 1] and fin[3, 2]
    assert not np.isfinite(bad["power"][2]).any() and not np.isfinite(bad["power"][3]).any()
    assert np.array_equal(bad["power"][:2], host["power"][:2]) and np.array_equal(bad["amp"][:2], host["amp"][:2])
    plan.close()


def _study_args(plan, cfg, oracle, kind):
    h, _ = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    return {"h": dict(h=h), "clean": dict(), "fading": dict(fading=([0, 3, 9], [1.0, 0.5, 0.25])),
            "random": dict(h=h, Time_Delay="random", Freq_Shift="random"), "register": dict(h=h, Register=REG),
            "all": dict(fading=([0, 5], [1.0, 0.3]), Time_Delay=7, Freq_Shift="random", Register=REG)}[kind]


def _rebuild(plan, ofdm, cfg, first, nw, snr, seed, fpp, f0, kw):
    """One point of the study from the per-frame call: the power rows, their left-to-right float64 sum from 0, and the np.fmax
    (from 0) over the frames and windows of the single-window power rows."""
    rx = np.asarray(plan.tx_frames_fused(fpp, SNR=snr, seed=seed, frame0=f0, **kw)["rx"])
    rows = ofdm.rx_spectrum(plan, rx, first=first, n_windows=nw, want_power=True)["power"]
    acc = np.zeros(cfg.Nfft, np.float64)
    for f in range(fpp):
        acc = acc + rows[f]
    pk = np.zeros(cfg.Nfft, np.float64)
    for w in range(nw):
        one = ofdm.rx_spectrum(plan, rx, first=first + w * (cfg.Nfft + cfg.T_guard), n_windows=1, want_power=True)["power"]
        pk = np.fmax(pk, np.fmax.reduce(one, axis=0))
    return dict(frame_power=rows, power_sums=acc, peak=pk)


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("kind", ["h", "clean", "fading", "random", "register", "all"])
def test_study_equals_the_per_frame_call_bitwise(ofdm, oracle, kind, precision):
    """frame_power[p] = rx_spectrum(tx_frames_fused(point p's arguments))["power"]; power_sums[p] = the left-to-right float64 sum
    of those rows, starting from 0; peak[p] = the maximum over frames f and windows w of the single-window power row
    rx_spectrum(first + w (Nfft + T_guard), n_windows=1, want_power=True)["power"][f], which is re^2 + im^2 of that one window as
    the kernel forms it (0 + it), with np.fmax."""
    from ofdm_course_amd import frames as fr
    cfg = _cfg("n1024" if kind in ("fading", "register") else "n256")
    plan = fr.make_plan(cfg, ofdm, precision=precision)
    kw = _study_args(plan, cfg, oracle, kind)
    snrs, seeds, fpp, f0, first, nw = [8.0, 25.0], [3, 0x1234ABCD5], 4, 6, cfg.T_guard + 1, 2
    st = plan.spectrum_study(snrs, fpp, seeds=seeds, frame0=f0, first=first, n_windows=nw, want_peak=True, want_frame_power=True,
                             **kw)
    assert st["power_sums"].shape == (2, cfg.Nfft) and st["frame_power"].shape == (2, fpp, cfg.Nfft)
    for p in range(2):
        want = _rebuild(plan, ofdm, cfg, first, nw, snrs[p], seeds[p], fpp, f0, kw)
        assert np.array_equal(st["frame_power"][p], want["frame_power"])
        assert np.array_equal(st["power_sums"][p], want["power_sums"])
        assert np.array_equal(st["peak"][p], want["peak"])
        assert np.array_equal(st["mean_power"][p], st["power_sums"][p] / (fpp * nw))
        assert np.array_equal(st["amp_rms"][p], np.sqrt(st["mean_power"][p]))
    assert not np.array_equal(st["power_sums"][0], st["power_sums"][1])
    # without the optional outputs the sums are the same
    plain = plan.spectrum_study(snrs, fpp, seeds=seeds, frame0=f0, first=first, n_windows=nw, **kw)
    assert set(plain) == {"power_sums", "mean_power", "amp_rms"} and np.array_equal(plain["power_sums"], st["power_sums"])
    plan.close()


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_no_output_depends_on_the_chunking_or_the_flavour(ofdm, oracle, precision):
    import torch
    from ofdm_course_amd import frames as fr
    cfg = _cfg("n256")
    plan = fr.make_plan(cfg, ofdm, precision=precision, device=0)
    kw = dict(_study_args(plan, cfg, oracle, "random"), seeds=[1, 2, 3], frame0=1, n_windows=cfg.N_symb, want_peak=True)
    snrs = [5.0, 15.0, 30.0]
    base = plan.spectrum_study(snrs, 5, want_frame_power=True, **kw)
    for chunk in (1, 3):
        for wfp in (True, False):                                 # the rows in the caller's buffer, or in the call's scratch
            got = plan.spectrum_study(snrs, 5, max_frames_per_chunk=chunk, want_frame_power=wfp, **kw)
            for key in got:
                assert np.array_equal(got[key], base[key]), (chunk, wfp, key)
    dev = plan.spectrum_study(snrs, 5, device="cuda:0", max_frames_per_chunk=3, want_frame_power=True, **kw)
    torch.cuda.synchronize()
    for key in base:
        assert dev[key].is_cuda and np.array_equal(dev[key].cpu().numpy(), base[key]), key
    # no frames, no points: zero sums, nothing else touched
    none = plan.spectrum_study(snrs, 0, want_peak=True)
    assert none["power_sums"].shape == (3, 256) and not none["power_sums"].any() and not none["peak"].any()
    assert plan.spectrum_study([], 5)["power_sums"].shape == (0, 256)
    # a NaN SNR makes every sample of its point NaN: NaN sums, and fmax leaves the peak at 0; the next point is untouched
    bad = plan.spectrum_study([float("nan"), 15.0], 5, seeds=[1, 2], frame0=1, n_windows=cfg.N_symb, want_peak=True, h=kw["h"],
                              Time_Delay="random", Freq_Shift="random")
    assert np.isnan(bad["power_sums"][0]).all() and not bad["peak"][0].any()
    assert np.array_equal(bad["power_sums"][1], base["power_sums"][1]) and np.array_equal(bad["peak"][1], base["peak"][1])
    plan.close()


def _oracle_frames(oracle, ofdm, cfg, nfr, seed, **kw):
    """Noise-free frames from the oracle's own TX functions, and their carrier matrices X [Nfft, N_symb] per frame."""
    from ofdm_course_amd import frames as fr
    _, bps = oracle.constellation_func(cfg.Constellation)
    pv = np.repeat(fr.pilot_column(cfg, ofdm)[:, None], cfg.N_symb, axis=1)
    nd = len(cfg.dataCarriers)
    rx, X = [], []
    for f in range(nfr):
        bits = oracle.payload_bits_philox(nd * cfg.N_symb, bps, seed, f)
        rx.append(oracle.tx_frame(bits, cfg.Nfft, cfg.T_guard, cfg.N_symb, cfg.dataCarriers, cfg.pilotCarriers, pv,
                                  cfg.Constellation, **kw)[0])
        iq, _ = oracle.mapping(bits, cfg.Constellation)
        X.append(oracle.OFDM_map_carriers(iq, cfg.N_symb, cfg.Nfft, cfg.dataCarriers, cfg.pilotCarriers, pv))
    return np.stack(rx, axis=1), X, fr.pilot_column(cfg, ofdm)


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_known_answers_from_the_oracles_functions(ofdm, oracle, precision):
    from ofdm_course_amd import frames as fr
    cfg = _cfg("n256")
    plan = fr.make_plan(cfg, ofdm, precision=precision)
    cdt = np.complex128 if precision == "fp64" else np.complex64
    N, tg, ns, nc = cfg.Nfft, cfg.T_guard, cfg.N_symb, cfg.N_carrier
    tol = _tol(N, precision)
    pc0 = np.rint(cfg.pilotCarriers).astype(int) - 1
    h, H = oracle.get_MP_channel_resp(TAPS3, N)
    clean, X, pil = _oracle_frames(oracle, ofdm, cfg, 2, 31)
    multi, _, _ = _oracle_frames(oracle, ofdm, cfg, 2, 31, h=h)
    shifted, _, _ = _oracle_frames(oracle, ofdm, cfg, 2, 31, Freq_Shift=5)
    a_clean = ofdm.rx_spectrum(plan, clean.astype(cdt), first=tg, n_windows=ns, want_power=True)
    a_multi = ofdm.rx_spectrum(plan, multi.astype(cdt), first=tg, n_windows=ns)["amp"]
    a_shift = ofdm.rx_spectrum(plan, shifted.astype(cdt), first=tg, n_windows=ns)["amp"]
    for f in range(2):
        for s in range(ns):
            want = np.abs(X[f][:, s])                             # |OFDM_map_carriers(...)(:, s)|: T1/Main_model.m:77 on a clean stream
            assert np.allclose(want[pc0], np.abs(pil)) and not want[nc:].any() and want[:nc].all()
            # first = T_guard + s (Nfft + T_guard) through its own call, and as window s of the frame
            one = ofdm.rx_spectrum(plan, clean.astype(cdt), first=tg + s * (N + tg))["amp"][f, 0]
            assert np.array_equal(one, a_clean["amp"][f, s])
            e = rel_l2(one, want)
            em = rel_l2(a_multi[f, s], want * np.abs(H))          # the CP holds the 3-tap channel: |X(k)| |H_freq(k)|
            es = rel_l2(a_shift[f, s], np.roll(want, 5))          # add_CFO(5): bin k moves to k + 5, circularly
            print(f"{precision} frame {f} symbol {s}: clean {e:.3e} multipath {em:.3e} cfo {es:.3e} (tol {tol:.1e})")
            assert e <= tol and em <= tol and es <= tol
            assert np.max(one[nc:]) <= tol * np.linalg.norm(want)              # the null carriers
            assert np.max(np.abs(one[pc0] - np.abs(pil))) <= tol * np.linalg.norm(want)
    if precision == "fp64":                                       # Parseval: sum_k power = Nfft sum |segment|^2
        _, _, seg = _reference(clean, cfg, tg, ns)
        lhs, rhs = a_clean["power"].sum(axis=1), N * (np.abs(seg) ** 2).sum(axis=(1, 2))
        print("Parseval rel. error", np.abs(lhs - rhs) / rhs)
        assert np.all(np.abs(lhs - rhs) <= 1e-12 * rhs)
    plan.close()


def _refused(ofdm, fn, msg):
    with pytest.raises(ofdm.OfdmError) as e:
        fn()
    assert msg in str(e.value), (msg, str(e.value))


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_refusals_leave_the_plan_usable(ofdm, oracle, precision):
    from ofdm_course_amd import frames as fr
    cfg = _cfg("n256")
    plan = fr.make_plan(cfg, ofdm, precision=precision)
    h, _ = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    rx = np.asarray(plan.tx_frames_fused(2, h=h, seed=4)["rx"])
    good_rx = ofdm.rx_spectrum(plan, rx, want_power=True)
    good_st = plan.spectrum_study([20.0], 3, h=h, want_peak=True, want_frame_power=True)
    end = "{} windows from sample {} on end behind the frame of 1440 samples"
    capture = [(dict(first=-1), "first must be >= 0 (-1)"), (dict(n_windows=0), "n_windows must be >= 1 (0)"),
               (dict(n_windows=-3), "n_windows must be >= 1 (-3)"), (dict(first=1185), end.format(1, 1185)),
               (dict(first=33, n_windows=5), end.format(5, 33)), (dict(n_windows=6), end.format(6, 32)),
               (dict(first=(1 << 63) - 1), end.format(1, (1 << 63) - 1)),
               (dict(first=0, n_windows=(1 << 63) - 1), end.format((1 << 63) - 1, 0)),
               (dict(first=-1, n_windows=0), "first must be >= 0 (-1)")]                   # the first refusal wins
    for brk, msg in capture:
        _refused(ofdm, lambda: ofdm.rx_spectrum(plan, rx, want_power=True, **brk), "rx_spectrum: " + msg)
        again = ofdm.rx_spectrum(plan, rx, want_power=True)
        assert np.array_equal(again["amp"], good_rx["amp"]) and np.array_equal(again["power"], good_rx["power"])
        _refused(ofdm, lambda: plan.spectrum_study([20.0], 3, h=h, **brk), "spectrum_study: " + msg)
        assert np.array_equal(plan.spectrum_study([20.0], 3, h=h)["power_sums"], good_st["power_sums"])
    study = [(dict(max_frames_per_chunk=-1), "spectrum_study: bad arguments"),
             (dict(frames_per_point=-1), "spectrum_study: bad arguments"),
             (dict(frame0=(1 << 32) - 3), "spectrum_study: frame index outside the 32-bit stream range"),
             (dict(Register=(1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 2)), "spectrum_study: register entries must be 0 or 1"),
             (dict(fading=([0, 3], [1.0, 0.5])), "spectrum_study: give h (one channel for every frame) or taps (a channel per frame), not both"),
             (dict(h=None, fading=([0, 3, 3], [1.0, 0.5, 0.5])), "spectrum_study: tap delay 3 given twice"),
             (dict(h=None, fading=([0, 4097], [1.0, 0.5]), first=-1), "spectrum_study: tap delay 4097 outside 0 .. 4096"),
             (dict(h=np.ones(65)), "tx_frames_fused: 65 nonzero channel taps (at most 64)")]
    for brk, msg in study:
        args = dict(dict(SNRs=[20.0], frames_per_point=3, h=h), **brk)
        _refused(ofdm, lambda: plan.spectrum_study(**args), msg)
        again = plan.spectrum_study([20.0], 3, h=h, want_peak=True, want_frame_power=True)
        for key in good_st:
            assert np.array_equal(again[key], good_st[key]), key
    # through the C entry: no output at all, the precision flag of the other precision, no plan
    import ctypes as C
    from ofdm_course_amd import _lib as L
    flags = L.OFDM_F64 if precision == "fp64" else L.OFDM_F32
    buf = np.ascontiguousarray(rx.T)
    amp = np.full((2, 1, 256), -1.0, np.float64 if precision == "fp64" else np.float32)
    p_rx, p_amp = buf.ctypes.data_as(C.c_void_p), amp.ctypes.data_as(C.c_void_p)
    lib = plan.lib
    for args, msg in [((plan.handle, p_rx, 2, 32, 1, None, None, flags), "rx_spectrum: no output is given"),
                      ((plan.handle, p_rx, 2, 32, 1, p_amp, None, flags ^ L.OFDM_F64), "rx_spectrum: precision flag differs from the plan's"),
                      ((plan.handle, None, 2, 32, 1, p_amp, None, flags), "rx_spectrum: bad arguments"),
                      ((None, p_rx, 2, 32, 1, p_amp, None, flags), "rx_spectrum: bad arguments"),
                      ((plan.handle, p_rx, -1, 32, 1, p_amp, None, flags), "rx_spectrum: n_frames must be 0 .. 2^31 - 1 (-1)")]:
        rc = lib.ofdm_rx_spectrum(*args)
        assert rc < 0 and msg in lib.ofdm_last_error_string().decode(), (msg, lib.ofdm_last_error_string())
        assert (amp == -1.0).all()                                # nothing was written
    L.check(lib.ofdm_rx_spectrum(plan.handle, p_rx, 2, 32, 1, p_amp, None, flags), "rx_spectrum")
    assert np.array_equal(amp, good_rx["amp"])                    # amp alone: the power row is optional
    snr, sd = np.array([20.0]), np.array([1], np.uint64)
    rc = lib.ofdm_spectrum_study(plan.handle, None, 0, None, None, 0, 0, 0, 0, 0.0, None, snr.ctypes.data_as(C.c_void_p),
                                 sd.ctypes.data_as(C.c_void_p), 1, 3, 0, 0, 32, 1, None, None, None, flags)
    assert rc < 0 and "spectrum_study: no output is given" in lib.ofdm_last_error_string().decode()
    assert np.array_equal(plan.spectrum_study([20.0], 3, h=h)["power_sums"], good_st["power_sums"])
    plan.close()


def test_task3_spectrum_driver_replays_the_report_figures(ofdm, tmp_path):
    """python -m ofdm_course_amd.drivers.task3_spectrum on three frames per figure: the clean spectrum has the pilots above the
    data and nothing beyond N_carrier, AWGN puts power there (T3/Main_model_Task_3.m:155), CFO = 5 moves every line by five
    bins, CFO = 100 by a hundred, and the multipath figure is the clean one times |H_freq|."""
    import json
    from ofdm_course_amd.drivers import task3_spectrum as t3s
    out = tmp_path / "out.json"
    t3s.main(["--json", str(out), "--frames", "3"])
    res = json.loads(out.read_text())
    assert res["frames"] == 3 and res["clean_SNR_dB"] == 3000.0 and res["first"] == 128
    sc_ = {n: {k: np.asarray(v) if isinstance(v, list) else v for k, v in s.items()} for n, s in res["scenarios"].items()}
    assert [sc_[n]["figure"] for n, _, _ in t3s.SCENARIOS] == [2, 4, 9, 12, 14, 16, 18, 24]
    clean = sc_["clean"]["amp_rms"]
    assert clean.shape == (1024,) and np.max(clean[400:]) <= 1e-12 * np.max(clean) and sc_["clean"]["null_power_share"] < 1e-24
    assert 1e-4 < sc_["awgn_25dB"]["null_power_share"] < 1e-2            # 624 of 1024 bins at -25 dB of the frame's power
    assert rel_l2(sc_["cfo_5"]["amp_rms"], np.roll(clean, 5)) < 1e-10
    assert rel_l2(sc_["cfo_100"]["amp_rms"], np.roll(clean, 100)) < 1e-10
    H = np.abs(np.fft.fft(np.array([1.0, 0, 0.4, 0, 0.01]), 1024))
    assert rel_l2(sc_["multipath"]["amp_rms"], clean * H) < 1e-10
    for n in ("cfo_0.01", "cfo_0.1", "sto_37"):                          # leakage / ISI: power beyond N_carrier
        assert sc_[n]["null_power_share"] > 1e-6
    assert all(np.all(s["peak"] * 3 >= s["power_sums"] * (1 - 1e-12)) for s in sc_.values())
