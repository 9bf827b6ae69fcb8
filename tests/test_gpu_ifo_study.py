"""The integer-CFO capture: rx_ifo (ofdm_rx_ifo) and RxPlan.ifo_study (ofdm_ifo_study).

rx_ifo against the oracle's composition for the stage -- raw: abs(fft(x(Nfft+1 : 2 Nfft))); receiver: AutoCorrFunction(x, T_guard,
Nfft), add_STO(TgPosition), add_STO(-(Nfft + T_guard)), add_CFO(-FreqOffset), then the same -- with the relative l2 bound of
tests/test_gpu_spectrum.py (1e-13 log2 Nfft in fp64, 1e-6 log2 Nfft in fp32); the picks exactly in fp64, and in fp32 on every frame
whose oracle spectrum has no bin, at or below the larger of the two picks, within a relative 1e-4 of 0.77 (at most 2 % of a case's
frames may be set aside so).  Against the existing entries on the same frames.  Which comparisons share the arithmetic: at Nfft 256
the receiver takes its staged form -- t4_align_kernel's rotation is t4_rotate's expression, and its transform is the wg_fft of
fft_core.hpp in the layout the capture uses -- and ofdm_remove_IFO transforms with the same kernel, so there IFO and status are
required to be equal on every frame in both precisions.  At Nfft 512 and 2048 the receiver's spectrum comes from the wave-local
transforms (and at 2048 / fp32 from t4_ifo_wave_kernel with a float rotor): the near-tie rule applies.  The study against the
per-frame call: bitwise, rebuilt with the twins of tests/ifo_cases.py."""
import warnings

import numpy as np
import pytest

import ifo_cases as ic

pytestmark = pytest.mark.gpu

REG = (1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0)          # T5/Main_model_Task_5.m:55
THR = 0.77                                                    # remove_IFO.m:6
STAGE = {"raw": 0, "receiver": 1}
# (shape of frames.config_small, precision, frames per kind, the receiver shares the capture's arithmetic)
CASES = {
    "n256-fp64": (dict(), "fp64", 3, True),
    "n256-fp32": (dict(), "fp32", 3, True),
    "n512-fp64": (dict(nfft=512, n_carrier=128), "fp64", 2, False),
    "n2048-fp32": (dict(nfft=2048, n_carrier=512, const="8PSK", n_symb=3), "fp32", 1, False),     # 4 frames: t4_ifo_wave_kernel
}


def _cfg(**kw):
    from ofdm_course_amd import frames as fr
    return fr.config_small(**kw)


def _tol(nfft, precision):
    return (1e-13 if precision == "fp64" else 1e-6) * np.log2(nfft)


def _frames(plan, oracle, cfg, per, seed=11):
    """`per` frames of each kind: clean, the 3-tap h, Time_Delay 7, and h with both draws."""
    h, _ = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    kinds = [dict(SNR=300.0), dict(h=h, SNR=25.0), dict(SNR=25.0, Time_Delay=7),
             dict(h=h, SNR=25.0, Time_Delay="random", Freq_Shift="random")]
    return np.concatenate([np.asarray(plan.tx_frames_fused(per, seed=seed, frame0=4 * i, **kw)["rx"]) for i, kw in enumerate(kinds)],
                          axis=1)


def _oracle_stage(oracle, x, cfg, stage, time_desync):
    """(|S|, IFO or 0, status, TgPosition, FreqOffset) of the oracle's composition for the stage on one frame."""
    N, Tg = cfg.Nfft, cfg.T_guard
    x = np.asarray(x, np.complex128)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, pos, fo, ok = oracle.AutoCorrFunction(x, Tg, N)
    y = x
    if stage == "receiver":
        if time_desync:
            y = oracle.add_STO(oracle.add_STO(y, pos), -(N + Tg))
        y = oracle.add_CFO(y, -fo, N)
    amp = np.abs(np.fft.fft(y[N:2 * N]))
    inds = np.nonzero(amp > THR)[0]
    status = 0 if ok else 1
    return amp, (int(inds[0]) if inds.size else 0), (status if inds.size else -1), pos, fo


def _near_tie(amp_w, upto):
    """The oracle's spectrum has a bin at or below `upto` within a relative 1e-4 of 0.77."""
    return bool(np.any(np.abs(amp_w[:upto + 1] - THR) <= 1e-4 * THR))


@pytest.mark.parametrize("stage,time_desync", [("raw", 1), ("receiver", 1), ("receiver", 0)])
@pytest.mark.parametrize("case", list(CASES))
def test_rx_ifo_against_the_oracle(ofdm, oracle, case, stage, time_desync):
    import torch
    from ofdm_course_amd import frames as fr
    shape, precision, per, _ = CASES[case]
    cfg = _cfg(**shape)
    plan = fr.make_plan(cfg, ofdm, precision=precision, device=0)
    rx = _frames(plan, oracle, cfg, per)
    rx = np.concatenate([rx, rx[:, 1:2] * np.asarray(1e-3, rx.dtype)], axis=1)        # one frame scaled by 1e-3: no line
    nfr, N = rx.shape[1], cfg.Nfft
    got = ofdm.rx_ifo(plan, rx, stage=stage, time_desync=time_desync)
    assert got["amp"].shape == (nfr, N) and got["amp"].dtype == (np.float64 if precision == "fp64" else np.float32)
    assert got["ifo"].dtype == np.int32 and got["status"].dtype == np.int32 and got["n_above"].dtype == np.int32
    assert got["tg_position"].dtype == np.int64 and got["freq_offset"].dtype == np.float64
    dev = ofdm.rx_ifo(plan, torch.from_numpy(rx).cuda(), stage=stage, time_desync=time_desync)
    torch.cuda.synchronize()
    for key in got:                                               # the device flavour: the same bits
        assert np.array_equal(dev[key].cpu().numpy(), got[key], equal_nan=True), key
    assert ofdm.rx_ifo(plan, rx, stage=stage, time_desync=time_desync, want_amp=False)["amp"] is None
    excluded = 0
    for f in range(nfr):
        amp_w, ifo_w, st_w, pos_w, fo_w = _oracle_stage(oracle, rx[:, f], cfg, stage, time_desync)
        a = got["amp"][f].astype(np.float64)
        rel = np.linalg.norm(a - amp_w) / np.linalg.norm(amp_w)
        print(f"{case} {stage} td={time_desync} frame {f}: rel l2 {rel:.3g} (bound {_tol(N, precision):.3g}), IFO {got['ifo'][f]} "
              f"(oracle {ifo_w}), status {got['status'][f]} ({st_w}), n_above {got['n_above'][f]} ({int((amp_w > THR).sum())}), "
              f"TgPosition {got['tg_position'][f]} ({pos_w})")
        assert np.all(np.isfinite(a)) and rel < _tol(N, precision)
        assert got["tg_position"][f] == pos_w
        if precision == "fp32" and _near_tie(amp_w, max(int(got["ifo"][f]), ifo_w)):
            excluded += 1
            continue
        assert got["ifo"][f] == ifo_w and got["status"][f] == st_w, (case, stage, f)
    print(f"{case} {stage}: {excluded} of {nfr} frames set aside by the near-tie rule")
    assert excluded <= 0.02 * nfr
    # the scaled frame: no line, IFO 0, nothing above, a finite row
    assert got["status"][-1] == -1 and got["ifo"][-1] == 0 and got["n_above"][-1] == 0 and np.all(np.isfinite(got["amp"][-1]))
    # n_above counts the bins of the returned row above the threshold (fp32: the row is rounded after the comparison)
    rows_above = (got["amp"].astype(np.float64) > THR).sum(axis=1)
    assert np.array_equal(got["n_above"], rows_above)
    plan.close()


@pytest.mark.parametrize("time_desync", [1, 0])
@pytest.mark.parametrize("case", list(CASES))
def test_rx_ifo_against_the_existing_entries(ofdm, oracle, case, time_desync):
    from ofdm_course_amd import frames as fr
    shape, precision, per, shared = CASES[case]
    cfg = _cfg(**shape)
    plan = fr.make_plan(cfg, ofdm, precision=precision)
    rx = _frames(plan, oracle, cfg, per, seed=23)
    nfr = rx.shape[1]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        chain = ofdm.rx_chain_task4(plan, rx, time_desync=time_desync, freq_desync=1, mp_desync=0)
    rcv = ofdm.rx_ifo(plan, rx, stage="receiver", time_desync=time_desync)
    raw = ofdm.rx_ifo(plan, rx, stage="raw", time_desync=time_desync)
    for out in (rcv, raw):                                        # the AutoCorrFunction stage in front is the receiver's own
        assert np.array_equal(out["tg_position"], np.asarray(chain["TgPosition"]))
        assert np.array_equal(out["freq_offset"].view(np.uint64), np.asarray(chain["FreqOffset"]).view(np.uint64))
    # the receiver reports -1 for a frame without a line and decodes it with an IFO of 0
    c_st, c_ifo = np.asarray(chain["status"]), np.asarray(chain["IFO"])
    c_ifo = np.where(c_st == -1, 0, c_ifo)
    raw_entry = []
    for f in range(nfr):
        try:
            raw_entry.append(int(ofdm.remove_IFO(rx[:, f], cfg.Nfft)[1]))
        except ofdm.OfdmError:
            raw_entry.append(None)
    print(f"{case} td={time_desync}: receiver IFO {rcv['ifo'].tolist()} chain {c_ifo.tolist()}; raw IFO {raw['ifo'].tolist()} "
          f"entry {raw_entry}; status {rcv['status'].tolist()} chain {c_st.tolist()}")
    excluded = 0
    for f in range(nfr):
        pairs = [(rcv["ifo"][f], c_ifo[f], rcv["status"][f], c_st[f], "receiver"),
                 (raw["ifo"][f], raw_entry[f] if raw_entry[f] is not None else 0, raw["status"][f] == -1, raw_entry[f] is None, "raw")]
        for mine, theirs, st_mine, st_theirs, stage in pairs:
            if not shared:
                amp_w = _oracle_stage(oracle, rx[:, f], cfg, stage, time_desync)[0]
                if _near_tie(amp_w, max(int(mine), int(theirs))):
                    excluded += 1
                    continue
            assert mine == theirs and st_mine == st_theirs, (case, stage, f, mine, theirs, st_mine, st_theirs)
    assert excluded <= 0.02 * 2 * nfr
    plan.close()


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_known_answer_an_integer_shift_rolls_the_row(ofdm, precision):
    """Freq_Shift = 3, no delay, no noise (300 dB): x(n) e^{2 pi i 3 n / Nfft} over a window of Nfft samples that starts at Nfft has
    the clean window's spectrum moved up by three bins."""
    from ofdm_course_amd import frames as fr
    cfg = _cfg()
    plan = fr.make_plan(cfg, ofdm, precision=precision)
    clean = np.asarray(plan.tx_frames_fused(3, SNR=300.0, seed=5)["rx"])
    shifted = np.asarray(plan.tx_frames_fused(3, SNR=300.0, seed=5, Freq_Shift=3.0)["rx"])
    a0 = ofdm.rx_ifo(plan, clean, stage="raw")
    a3 = ofdm.rx_ifo(plan, shifted, stage="raw")
    r3 = ofdm.rx_ifo(plan, shifted, stage="receiver")
    want = np.roll(a0["amp"].astype(np.float64), 3, axis=1)
    rel = np.linalg.norm(a3["amp"] - want, axis=1) / np.linalg.norm(want, axis=1)
    print(f"{precision}: rel l2 of the rolled row {rel.tolist()}, IFO clean {a0['ifo'].tolist()} shifted {a3['ifo'].tolist()} "
          f"receiver {r3['ifo'].tolist()}")
    # two spectra of two roundings of the frame (the generator rounds the rotated samples): twice the bound of one
    assert np.all(rel < 2 * _tol(cfg.Nfft, precision))
    assert np.all(a0["status"] == 0) and np.array_equal(a3["ifo"] - 3, a0["ifo"]) and np.array_equal(r3["ifo"], a3["ifo"])
    plan.close()


def _study_args(cfg, oracle, kind):
    h, _ = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    return {"clean": dict(), "h": dict(h=h), "fading": dict(fading=([0, 3, 9], [1.0, 0.5, 0.25])),
            "delay7": dict(Time_Delay=7), "random": dict(h=h, Time_Delay="random", Freq_Shift="random"),
            "register": dict(h=h, Register=REG, Freq_Shift=0.24)}[kind]


def _rebuild(plan, ofdm, cfg, stage, td, span, snr, seed, fpp, f0, kw):
    """One point of the study from the per-frame call, the generator's draws and the twins of ifo_cases.py."""
    fr = plan.tx_frames_fused(fpp, SNR=snr, seed=seed, frame0=f0, want_draws=True, **kw)
    per = ofdm.rx_ifo(plan, np.asarray(fr["rx"]), stage=stage, time_desync=td)
    cfo = np.asarray(fr["Freq_Shift"]) if "Freq_Shift" in kw else np.zeros(fpp, np.float64)
    a = per["amp"].astype(np.float64)
    N = a.shape[1]
    fin = np.isfinite(a)
    acc = np.zeros(N, np.float64)
    for f in range(fpp):                                          # left to right, from 0; x + 0.0 = x for x >= +0
        acc = acc + np.where(fin[f], a[f], 0.0)
    line = per["status"] != -1
    hist, below, above, hit = np.zeros(2 * span + 1, np.int64), 0, 0, 0
    s1, s2 = np.float64(0.0), np.float64(0.0)
    for f in np.nonzero(line)[0]:
        b = ic.err_bin(per["ifo"][f], cfo[f], span)
        if b == ic.ERR_BELOW:
            below += 1
        elif b == ic.ERR_ABOVE:
            above += 1
        else:
            hist[b] += 1
            hit += int(b == span)
        e = ic.cfo_total_err(per["freq_offset"][f], per["ifo"][f], cfo[f])
        if np.isfinite(e):
            s1 = s1 + np.abs(e)
            s2 = s2 + e * e
    return dict(spec_sums=acc, spec_dropped=(~fin).sum(axis=0), above_counts=(a > THR).sum(axis=0),
                ifo_hist=np.bincount(per["ifo"][line], minlength=N), no_line=int((~line).sum()), err_hist=hist, err_below=below,
                err_above=above, hit=hit, cfo_err=np.array([s1, s2]), fallback=int((per["status"] == 1).sum()), ifo=per["ifo"],
                status=per["status"], n_above=per["n_above"], tg_position=per["tg_position"], freq_offset=per["freq_offset"])


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("stage", ["raw", "receiver"])
@pytest.mark.parametrize("kind", ["clean", "h", "fading", "delay7", "random", "register"])
def test_study_equals_the_per_frame_call_bitwise(ofdm, oracle, kind, stage, precision):
    """Every output of a point is rebuilt from rx_ifo(tx_frames_fused(the point's arguments)) and the generator's draws: spec_sums the
    left-to-right float64 sum from 0 of the amp rows, above_counts the rows above 0.77 (in fp32 the row is rounded after the
    library's comparison; a bin that the rounding moves across 0.77 would show here and in rx_ifo's n_above test), the histograms
    and cfo_err through the twins of ifo_cases.py.  The last point is noise alone (-40 dB)."""
    from ofdm_course_amd import frames as fr
    cfg = _cfg()
    plan = fr.make_plan(cfg, ofdm, precision=precision)
    kw = _study_args(cfg, oracle, kind)
    span = 2 if kind == "random" else 32                          # a narrow span: the tails are used
    snrs, seeds, fpp, f0 = [8.0, 25.0, -40.0], [3, 0x1234ABCD5, 9], 4, 6
    st = plan.ifo_study(snrs, fpp, seeds=seeds, frame0=f0, stage=stage, time_desync=1, err_span=span, want_frames=True, **kw)
    N = cfg.Nfft
    assert st["spec_sums"].shape == (3, N) and st["err_hist"].shape == (3, 2 * span + 1) and st["ifo"].shape == (3, fpp)
    assert st["above_counts"].dtype == np.int64 and st["ifo_hist"].dtype == np.int64 and st["status"].dtype == np.int32
    for p in range(3):
        want = _rebuild(plan, ofdm, cfg, stage, 1, span, snrs[p], seeds[p], fpp, f0, kw)
        for key, val in want.items():
            val = np.asarray(val)
            got = np.asarray(st[key][p])
            assert np.array_equal(got.view(np.uint64) if val.dtype.kind == "f" else got,
                                  val.view(np.uint64) if val.dtype.kind == "f" else val), (kind, stage, p, key, got, val)
        # the identities
        assert st["ifo_hist"][p].sum() + st["no_line"][p] == fpp
        assert st["err_hist"][p].sum() + st["err_below"][p] + st["err_above"][p] == fpp - st["no_line"][p]
        assert np.all(st["above_counts"][p] <= fpp) and not st["spec_dropped"][p].any()
    with np.errstate(divide="ignore", invalid="ignore"):
        assert np.array_equal(st["mean_spec"], st["spec_sums"] / (fpp - st["spec_dropped"]), equal_nan=True)
        assert np.array_equal(st["hit_rate"], st["hit"] / np.float64(fpp)) and np.array_equal(st["no_line_rate"], st["no_line"] / np.float64(fpp))
        assert np.array_equal(st["mean_abs_cfo_err"], st["cfo_err"][:, 0] / (fpp - st["no_line"]), equal_nan=True)
    plain = plan.ifo_study(snrs, fpp, seeds=seeds, frame0=f0, stage=stage, time_desync=1, err_span=span, **kw)
    assert set(plain) == set(st) - {"ifo", "status", "n_above", "tg_position", "freq_offset"}
    for key in plain:
        assert np.array_equal(plain[key], st[key], equal_nan=True), key
    plan.close()


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_no_output_depends_on_the_chunking_or_the_flavour(ofdm, oracle, precision):
    import torch
    from ofdm_course_amd import frames as fr
    cfg = _cfg()
    plan = fr.make_plan(cfg, ofdm, precision=precision, device=0)
    h, _ = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    kw = dict(h=h, Time_Delay="random", Freq_Shift="random", seeds=[1, 2, 3], frame0=1, want_frames=True, err_span=3)
    snrs = [-40.0, 15.0, 30.0]
    for stage in ("raw", "receiver"):
        base = plan.ifo_study(snrs, 5, stage=stage, **kw)
        assert base["ifo_hist"].sum() + base["no_line"].sum() == 15
        for chunk in (1, 3):
            got = plan.ifo_study(snrs, 5, stage=stage, max_frames_per_chunk=chunk, **kw)
            assert set(got) == set(base)
            for key in got:
                assert np.array_equal(got[key], base[key], equal_nan=True), (stage, chunk, key)
        nofr = plan.ifo_study(snrs, 5, stage=stage, max_frames_per_chunk=3, **dict(kw, want_frames=False))
        for key in nofr:
            assert np.array_equal(nofr[key], base[key], equal_nan=True), key
        dev = plan.ifo_study(snrs, 5, stage=stage, device="cuda:0", max_frames_per_chunk=3, **kw)
        torch.cuda.synchronize()
        for key in base:
            assert dev[key].is_cuda and np.array_equal(dev[key].cpu().numpy(), base[key], equal_nan=True), (stage, key)
    none = plan.ifo_study(snrs, 0)
    assert none["spec_sums"].shape == (3, 256) and not none["spec_sums"].any() and not none["ifo_hist"].any() and not none["no_line"].any()
    assert plan.ifo_study([], 5)["spec_sums"].shape == (0, 256)
    plan.close()


def _refused(ofdm, fn, msg):
    with pytest.raises(ofdm.OfdmError) as e:
        fn()
    assert msg in str(e.value), (msg, str(e.value))


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_refusals_leave_the_plan_usable(ofdm, oracle, precision):
    import ctypes as C
    from ofdm_course_amd import _lib as L
    from ofdm_course_amd import frames as fr
    cfg = _cfg()
    plan = fr.make_plan(cfg, ofdm, precision=precision)
    h, _ = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    rx = np.asarray(plan.tx_frames_fused(2, h=h, seed=4)["rx"])
    good_rx = ofdm.rx_ifo(plan, rx)
    good_st = plan.ifo_study([20.0], 3, h=h, want_frames=True)

    def same_rx():
        again = ofdm.rx_ifo(plan, rx)
        return all(np.array_equal(again[k], good_rx[k], equal_nan=True) for k in good_rx)

    def same_st():
        again = plan.ifo_study([20.0], 3, h=h, want_frames=True)
        return all(np.array_equal(again[k], good_st[k], equal_nan=True) for k in good_st)

    # the capture refusals of ifo_cases.py a caller reaches through the Python layer with this plan, through both entries
    reach = {"stage": dict(stage=2), "time_desync": dict(time_desync=2), "span": dict(err_span=0)}
    for rid, _, msg in ic.capture_order(True):
        if rid not in reach:
            continue
        if rid != "span":
            _refused(ofdm, lambda: ofdm.rx_ifo(plan, rx, **reach[rid]), "rx_ifo: " + msg)
            assert same_rx()
        _refused(ofdm, lambda: plan.ifo_study([20.0], 3, h=h, **reach[rid]), "ifo_study: " + msg)
        assert same_st()
    _refused(ofdm, lambda: plan.ifo_study([20.0], 3, h=h, err_span=4097), "ifo_study: err_span must be 1 .. 4096 (4097)")
    # "short": a plan of one symbol (288 samples < 2 Nfft); "route": a plan with one pilot carrier
    short = fr.make_plan(_cfg(n_symb=1), ofdm, precision=precision)
    msg = dict((rid, m) for rid, _, m in ic.capture_order(True))
    _refused(ofdm, lambda: ofdm.rx_ifo(short, rx[:288]), "rx_ifo: " + msg["short"])
    _refused(ofdm, lambda: short.ifo_study([20.0], 3), "ifo_study: " + msg["short"])
    short.close()
    one_cfg = _cfg()
    one = ofdm.RxPlan(one_cfg.Nfft, one_cfg.T_guard, one_cfg.N_symb, one_cfg.N_carrier, one_cfg.pilotCarriers[:1],
                      np.setdiff1d(np.arange(1, one_cfg.N_carrier + 1), one_cfg.pilotCarriers[:1]).astype(np.float64),
                      fr.pilot_column(one_cfg, ofdm)[:1], 1, 1, one_cfg.Constellation, precision=precision)
    _refused(ofdm, lambda: ofdm.rx_ifo(one, rx), "rx_ifo: " + msg["route"])
    _refused(ofdm, lambda: one.ifo_study([20.0], 3), "ifo_study: " + msg["route"])
    one.close()
    assert same_rx() and same_st()
    study = [(dict(max_frames_per_chunk=-1), "ifo_study: bad arguments"),
             (dict(frames_per_point=-1), "ifo_study: bad arguments"),
             (dict(frame0=(1 << 32) - 3), "ifo_study: frame index outside the 32-bit stream range"),
             (dict(Register=(1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 2)), "ifo_study: register entries must be 0 or 1"),
             (dict(fading=([0, 3], [1.0, 0.5])), "ifo_study: give h (one channel for every frame) or taps (a channel per frame), not both"),
             (dict(h=None, fading=([0, 3, 3], [1.0, 0.5, 0.5])), "ifo_study: tap delay 3 given twice"),
             (dict(h=None, fading=([0, 4097], [1.0, 0.5]), stage=2), "ifo_study: tap delay 4097 outside 0 .. 4096"),
             (dict(h=np.ones(65)), "tx_frames_fused: 65 nonzero channel taps (at most 64)")]
    for brk, text in study:
        args = dict(dict(SNRs=[20.0], frames_per_point=3, h=h), **brk)
        _refused(ofdm, lambda: plan.ifo_study(**args), text)
        assert same_st()
    # through the C entry: no output at all, the other precision's flag, no plan, no frames pointer, a bad count
    flags = L.OFDM_F64 if precision == "fp64" else L.OFDM_F32
    buf = np.ascontiguousarray(rx.T)
    amp = np.full((2, 256), -1.0, np.float64 if precision == "fp64" else np.float32)
    p_rx, p_amp = buf.ctypes.data_as(C.c_void_p), amp.ctypes.data_as(C.c_void_p)
    lib = plan.lib
    for args, text in [((plan.handle, p_rx, 2, 1, 1, None, None, None, None, None, None, flags), "rx_ifo: no output is given"),
                       ((plan.handle, p_rx, 2, 1, 1, p_amp, None, None, None, None, None, flags ^ L.OFDM_F64),
                        "rx_ifo: precision flag differs from the plan's"),
                       ((plan.handle, None, 2, 1, 1, p_amp, None, None, None, None, None, flags), "rx_ifo: bad arguments"),
                       ((None, p_rx, 2, 1, 1, p_amp, None, None, None, None, None, flags), "rx_ifo: bad arguments"),
                       ((plan.handle, p_rx, -1, 1, 1, p_amp, None, None, None, None, None, flags),
                        "rx_ifo: n_frames must be 0 .. 2^31 - 1 (-1)")]:
        rc = lib.ofdm_rx_ifo(*args)
        assert rc < 0 and text in lib.ofdm_last_error_string().decode(), (text, lib.ofdm_last_error_string())
        assert (amp == -1.0).all()                                # nothing was written
    L.check(lib.ofdm_rx_ifo(plan.handle, p_rx, 2, 1, 1, p_amp, None, None, None, None, None, flags), "rx_ifo")
    assert np.array_equal(amp, good_rx["amp"])                    # amp alone: every other output is optional
    snr, sd = np.array([20.0]), np.array([1], np.uint64)
    head = (plan.handle, None, 0, None, None, 0, 0, 0, 0, 0.0, 1, 1, None, snr.ctypes.data_as(C.c_void_p), sd.ctypes.data_as(C.c_void_p),
            1, 3, 0, 0, 32)
    rc = lib.ofdm_ifo_study(*head, *([None] * 16), flags)
    assert rc < 0 and "ifo_study: no output is given" in lib.ofdm_last_error_string().decode()
    hit = np.full(1, 99, np.uint64)
    L.check(lib.ofdm_ifo_study(*head, *([None] * 8), hit.ctypes.data_as(C.c_void_p), *([None] * 7), flags), "ifo_study")
    assert hit[0] == plan.ifo_study([20.0], 3, seeds=[1])["hit"][0]   # one table alone: every output is optional
    assert same_st()
    plan.close()


def test_task4_ifo_driver_smoke(ofdm, tmp_path, monkeypatch):
    """python -m ofdm_course_amd.drivers.task4_ifo at a few frames and three SNR points: both studies in the JSON, and at 60 dB the
    error of figure 13b is below 0.5 -- well under one carrier."""
    import json
    from ofdm_course_amd.drivers import task4_ifo as t4i
    monkeypatch.setattr(t4i, "FIG_SNRS", (0.0, 30.0, 60.0))
    out = tmp_path / "out.json"
    t4i.main(["--json", str(out), "--frames", "4", "--frames-per-tile", "3"])
    res = json.loads(out.read_text())
    fig = res["figure_13b"]
    assert res["frames"] == 4 and fig["figure"] == "13b" and fig["SNR_dB"] == [0.0, 30.0, 60.0]
    assert (fig["Time_Delay"], fig["Freq_Shift"]) == (150, 0.24)
    print("figure 13b mean |e|:", fig["mean_abs_err"], "no_line:", fig["no_line"])
    assert fig["no_line"][2] == 0 and fig["mean_abs_err"][2] < 0.5
    assert np.asarray(fig["ifo_hist"]).shape == (3, 1024) and np.asarray(fig["ifo_hist"])[2].sum() == 4
    assert set(res["c3"]) == {"raw", "receiver"}
    for stage, tab in res["c3"].items():
        assert 0.0 <= tab["hit_rate"] <= 1.0 and len(tab["err_hist"]) == 2 * t4i.ERR_SPAN + 1 == len(tab["err_offsets"])
        assert sum(tab["err_hist"]) + tab["err_below"] + tab["err_above"] == 4 - round(tab["no_line_rate"] * 4)
        assert len(tab["above_rel"]) == len(tab["ifo_rel"]) == len(tab["rel_bins"]) == 2 * t4i.REL_SPAN + 1
        assert max(tab["above_rel"]) <= 4
        print(stage, "hit rate", tab["hit_rate"], "err_hist", tab["err_hist"], "above_rel", tab["above_rel"], "ifo_rel", tab["ifo_rel"])
