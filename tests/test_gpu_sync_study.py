"""The coarse-sync capture: rx_acf (ofdm_rx_acf) and RxPlan.sync_study (ofdm_sync_study).

rx_acf against the entry that exists, AutoCorrFunction on each frame: rho, TgPosition and FreqOffset bit for bit.  amp has no
counterpart there; it is sqrt(re^2 + im^2) formed in double from that rho and rounded to the plan's precision.  From complex64 the
squares and their sum's operands are exact in double, so a fused or an unfused sum rounds alike and amp is bit for bit
float32(sqrt(float64(re)^2 + float64(im)^2)); from complex128 the sum may be fused, one rounding fewer, so amp is held to one
unit in the last place of that expression.  Against the oracle: the bounds of tests/test_gpu_sync_sizes.py, restated -- rho
1e-11 (fp64) / 1e-4 (fp32), FreqOffset 1e-9 / 1e-6 -- with equal positions and catch-branch flags.  The study against the
per-frame call: bitwise, rebuilt with the twins of tests/sync_cases.py.  The refusals of tests/sync_cases.py, each followed by a
good call."""
import warnings

import numpy as np
import pytest

import sync_cases as sc

pytestmark = pytest.mark.gpu

REG = (1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0)          # T5/Main_model_Task_5.m:55
RHO_TOL = {"fp64": 1e-11, "fp32": 1e-4}                       # tests/test_gpu_sync_sizes.py: rho
FO_TOL = {"fp64": 1e-9, "fp32": 1e-6}                         # tests/test_gpu_sync_sizes.py: FreqOffset
THR = 0.77                                                    # AutoCorrFunction.m:10

# (shape of frames.config_small, WidthWindow): n256 has n_out = 1440 - W - 256 > 1024, the curve crosses an acf_tile boundary;
# n1024 with W = 1024 is the LDS maximum (n_out = 1408)
CASES = {
    "n256-w1": (dict(), 1),
    "n256-w16": (dict(), 16),
    "n256-w32": (dict(), 32),
    "n1024-w1024": (dict(nfft=1024, n_carrier=400, const="8PSK", n_symb=3), 1024),
}


def _cfg(**kw):
    from ofdm_course_amd import frames as fr
    return fr.config_small(**kw)


def _bits(a):
    """The bit patterns of a float or complex array: NaN compares equal to the same NaN."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 16: np.uint64}[a.dtype.itemsize])


def _amp_of(rho, precision):
    """sqrt(re^2 + im^2) in double from rho, then the plan's precision."""
    re, im = rho.real.astype(np.float64), rho.imag.astype(np.float64)
    with np.errstate(invalid="ignore"):
        a = np.sqrt(re * re + im * im)
    return a if precision == "fp64" else a.astype(np.float32)


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("case", list(CASES))
def test_rx_acf_against_the_existing_entry_and_the_oracle(ofdm, oracle, case, precision):
    import torch
    from ofdm_course_amd import frames as fr
    shape, W = CASES[case]
    cfg = _cfg(**shape)
    plan = fr.make_plan(cfg, ofdm, precision=precision, device=0)
    h, _ = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    nfr = 5                                                       # one workgroup per frame
    # frames 0 .. 2 through the channel; 3 and 4 without one, so the zero tail add_STO leaves stays zero: 0 / 0 = NaN lags
    kw = dict(SNR=25.0, seed=11, Time_Delay="random", Freq_Shift="random")
    rx = np.concatenate([np.asarray(plan.tx_frames_fused(3, h=h, frame0=3, **kw)["rx"]),
                         np.asarray(plan.tx_frames_fused(2, frame0=6, **kw)["rx"])], axis=1)
    n_out = cfg.frame_samples - W - cfg.Nfft
    got = ofdm.rx_acf(plan, rx, width=W, want_rho=True)
    assert got["amp"].shape == (nfr, n_out) and got["rho"].shape == (nfr, n_out)
    assert got["amp"].dtype == (np.float64 if precision == "fp64" else np.float32)
    assert got["tg_position"].dtype == np.int64 and got["status"].dtype == np.int32 and got["freq_offset"].dtype == np.float64
    dev = ofdm.rx_acf(plan, torch.from_numpy(rx).cuda(), width=W, want_rho=True)
    torch.cuda.synchronize()
    for key in got:                                               # the device flavour: the same bits
        assert np.array_equal(_bits(dev[key].cpu().numpy()), _bits(got[key])), key
    assert ofdm.rx_acf(plan, rx, width=W)["rho"] is None
    if W == cfg.T_guard:                                          # width=None is T_guard (T4/Main_model_Task_4.m:278)
        dflt = ofdm.rx_acf(plan, rx)
        assert np.array_equal(_bits(dflt["amp"]), _bits(got["amp"])) and np.array_equal(dflt["tg_position"], got["tg_position"])
    for f in range(nfr):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            rho, pos, fo = ofdm.AutoCorrFunction(rx[:, f], W, cfg.Nfft)
            rho_w, pos_w, fo_w, ok = oracle.AutoCorrFunction(rx[:, f].astype(np.complex128), W, cfg.Nfft)
        rho = np.asarray(rho)
        # the existing entry, bit for bit
        assert np.array_equal(_bits(got["rho"][f]), _bits(rho)), (case, f)
        assert got["tg_position"][f] == pos
        print(f"{case} {precision} frame {f}: pos {pos} (oracle {pos_w}, ok {ok}), FreqOffset {got['freq_offset'][f]!r} entry {fo!r} "
              f"oracle {fo_w!r}, NaN lags {int(np.isnan(rho_w).sum())}")
        want = _amp_of(rho, precision)
        if precision == "fp32":
            assert np.array_equal(_bits(got["amp"][f]), _bits(want)), (case, f)
        else:
            fin = ~np.isnan(want)
            assert np.array_equal(np.isnan(got["amp"][f]), ~fin)
            assert np.all(np.abs(got["amp"][f][fin] - want[fin]) <= np.spacing(want[fin])), (case, f)
        # the oracle
        nan_w = np.isnan(rho_w)
        amp_w = np.abs(rho_w)
        err = float(np.max(np.abs(got["amp"][f].astype(np.float64) - amp_w)[~nan_w])) if (~nan_w).any() else 0.0
        margin = float(np.nanmin(np.abs(amp_w[W:] - THR))) if (~nan_w[W:]).any() else float("inf")
        print(f"  max|amp - |rho_w|| {err:.3g} (bound {RHO_TOL[precision]:.0e}), |fo - fo_w| {abs(got['freq_offset'][f] - fo_w):.3g} "
              f"(bound {FO_TOL[precision]:.0e}), smallest ||rho_w| - 0.77| {margin:.3g}")
        assert np.array_equal(np.isnan(got["amp"][f]), nan_w)     # 0 / 0 stays NaN
        assert err < RHO_TOL[precision]
        assert got["tg_position"][f] == pos_w and got["status"][f] == (0 if ok else 1)
        assert abs(got["freq_offset"][f] - fo_w) < FO_TOL[precision]
    plan.close()


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_known_answer_on_a_clean_frame(ofdm, precision):
    """No noise (3000 dB: sigma is 1e-150 of the signal), no channel: the cyclic prefix repeats the symbol's tail, so every window
    that lies inside a guard interval has rho = 1 -- lags s (Nfft + T_guard) .. s (Nfft + T_guard) + T_guard - W of every symbol s --
    and half a symbol further the window holds independent samples: below the threshold."""
    from ofdm_course_amd import frames as fr
    cfg = _cfg()
    plan = fr.make_plan(cfg, ofdm, precision=precision)
    rx = np.asarray(plan.tx_frames_fused(3, SNR=3000.0, seed=2)["rx"])
    stride, tg = cfg.Nfft + cfg.T_guard, cfg.T_guard
    for W in (tg // 2, tg):
        out = ofdm.rx_acf(plan, rx, width=W)
        amp, n_out = out["amp"].astype(np.float64), out["amp"].shape[1]
        on = np.array([s * stride + d for s in range(cfg.N_symb) for d in range(tg - W + 1) if s * stride + d < n_out])
        mid = np.array([s * stride + stride // 2 for s in range(cfg.N_symb) if s * stride + stride // 2 < n_out])
        assert on.size >= (cfg.N_symb - 1) * (tg - W + 1) and mid.size >= cfg.N_symb - 1
        print(f"{precision} W={W}: max |amp - 1| on the plateaus {np.max(np.abs(amp[:, on] - 1)):.3g}, largest mid-symbol {np.max(amp[:, mid]):.3g}")
        assert np.max(np.abs(amp[:, on] - 1.0)) < RHO_TOL[precision]
        assert np.max(amp[:, mid]) < THR
        assert np.all(out["status"] == 0)                         # two runs above the threshold exist: no catch branch
    plan.close()


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("case", list(CASES))
def test_rx_acf_freq_offset_equals_the_existing_entry_bitwise(ofdm, oracle, case, precision):
    """FreqOffset of rx_acf against AutoCorrFunction's on the same frame, bit for bit.  rho(TgPosition) is the same number on both
    sides (test_rx_acf_against_the_existing_entry_and_the_oracle) and every entry takes -atan2(im, re) / (2 pi) of it on the
    device.  (While AutoCorrFunction took it on the host these frames differed in the last place: n256-w1 frame 2
    -0.2182402018166256 against the host's -0.21824020181662562, n256-w32 frame 4 0.15606475841342438 / 0.1560647584134244.)"""
    from ofdm_course_amd import frames as fr
    shape, W = CASES[case]
    cfg = _cfg(**shape)
    plan = fr.make_plan(cfg, ofdm, precision=precision)
    h, _ = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    kw = dict(SNR=25.0, seed=11, Time_Delay="random", Freq_Shift="random")
    rx = np.concatenate([np.asarray(plan.tx_frames_fused(3, h=h, frame0=3, **kw)["rx"]),
                         np.asarray(plan.tx_frames_fused(2, frame0=6, **kw)["rx"])], axis=1)
    got = ofdm.rx_acf(plan, rx, width=W)["freq_offset"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = np.array([ofdm.AutoCorrFunction(rx[:, f], W, cfg.Nfft)[2] for f in range(rx.shape[1])])
    print(f"{case} {precision}: rx_acf {got.tolist()} entry {want.tolist()}")
    assert np.array_equal(_bits(got), _bits(want)), (case, got.tolist(), want.tolist())
    plan.close()


def _study_args(cfg, oracle, kind):
    h, _ = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    return {"clean": dict(), "h": dict(h=h), "fading": dict(fading=([0, 3, 9], [1.0, 0.5, 0.25])),
            "delay7": dict(Time_Delay=7), "random": dict(h=h, Time_Delay="random", Freq_Shift="random"),
            "register": dict(h=h, Register=REG, Freq_Shift=0.24)}[kind]


def _rebuild(plan, ofdm, cfg, W, snr, seed, fpp, f0, kw):
    """One point of the study from the per-frame call, the generator's draws and the twins of sync_cases.py."""
    fr = plan.tx_frames_fused(fpp, SNR=snr, seed=seed, frame0=f0, want_draws=True, **kw)
    per = ofdm.rx_acf(plan, np.asarray(fr["rx"]), width=W)
    sto = np.asarray(fr["Time_Delay"]) if "Time_Delay" in kw else np.zeros(fpp, np.int64)
    cfo = np.asarray(fr["Freq_Shift"]) if "Freq_Shift" in kw else np.zeros(fpp, np.float64)
    a = per["amp"].astype(np.float64)
    n_out, stride = a.shape[1], cfg.Nfft + cfg.T_guard
    fin = np.isfinite(a)
    acc = np.zeros(n_out, np.float64)
    for f in range(fpp):                                          # left to right, from 0; x + 0.0 = x for x >= +0
        acc = acc + np.where(fin[f], a[f], 0.0)
    s1, s2 = np.float64(0.0), np.float64(0.0)
    for f in range(fpp):
        e = sc.ffo_err(per["freq_offset"][f], cfo[f])
        s1 = s1 + np.abs(e)
        s2 = s2 + e * e
    tg = per["tg_position"]
    return dict(acf_sums=acc, acf_dropped=(~fin).sum(axis=0), acf_peak=np.fmax(0.0, np.fmax.reduce(a, axis=0)),
                tg_hist=np.bincount(tg[tg - 1 < n_out] - 1, minlength=n_out), fallback=int((per["status"] == 1).sum()),
                phase_hist=np.bincount([sc.phase_bin(t, s, stride) for t, s in zip(tg, sto)], minlength=stride),
                ffo_err=np.array([s1, s2]), tg_position=tg, status=per["status"], freq_offset=per["freq_offset"]), sto


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("kind", ["clean", "h", "fading", "delay7", "random", "register"])
def test_study_equals_the_per_frame_call_bitwise(ofdm, oracle, kind, precision):
    """Every output of a point is rebuilt from rx_acf(tx_frames_fused(the point's arguments)) and the generator's draws: acf_sums the
    left-to-right float64 sum from 0 of the amp rows with the values that are not finite skipped, acf_dropped their count, acf_peak
    np.fmax over the frames (from 0), the histograms and ffo_err through the twins of sync_cases.py.  The last point is noise alone
    (-40 dB: a window of 32 independent products exceeds 0.77 with probability exp(-0.77^2 32) = 6e-9 per lag), where the oracle
    too finds no plateau in any frame: the catch branch is taken (asserted for the kinds that run at W = T_guard = 32).  Time_Delay = 7
    without a channel leaves seven zero samples behind the frame; at W = 4 the windows of the last three lags are all zero."""
    from ofdm_course_amd import frames as fr
    cfg = _cfg()
    plan = fr.make_plan(cfg, ofdm, precision=precision)
    kw = _study_args(cfg, oracle, kind)
    W = {"clean": 16, "fading": 1, "delay7": 4}.get(kind, cfg.T_guard)
    snrs, seeds, fpp, f0 = [8.0, 25.0, -40.0], [3, 0x1234ABCD5, 9], 4, 6
    st = plan.sync_study(snrs, fpp, seeds=seeds, frame0=f0, width=W, want_peak=True, want_frames=True, **kw)
    n_out, stride = cfg.frame_samples - W - cfg.Nfft, cfg.Nfft + cfg.T_guard
    assert st["acf_sums"].shape == (3, n_out) and st["phase_hist"].shape == (3, stride) and st["tg_position"].shape == (3, fpp)
    assert st["acf_dropped"].dtype == np.int64 and st["tg_hist"].dtype == np.int64 and st["status"].dtype == np.int32
    for p in range(3):
        want, sto = _rebuild(plan, ofdm, cfg, W, snrs[p], seeds[p], fpp, f0, kw)
        for key, val in want.items():
            assert np.array_equal(_bits(st[key][p]) if np.asarray(val).dtype.kind == "f" else st[key][p],
                                  _bits(val) if np.asarray(val).dtype.kind == "f" else val), (kind, p, key)
        assert np.all(st["acf_dropped"][p] <= fpp)                # frames added + dropped = frames_per_point, per lag
        with np.errstate(divide="ignore", invalid="ignore"):
            assert np.array_equal(st["mean_acf"][p], st["acf_sums"][p] / (fpp - st["acf_dropped"][p]), equal_nan=True)
        assert st["tg_hist"][p].sum() == fpp and st["phase_hist"][p].sum() == fpp          # n_out > 64: 65 has a bin
        assert st["tg_hist"][p][64] >= st["fallback"][p]
        if kind == "delay7":                                      # the zero tail add_STO leaves: 0 / 0 at the last 7 - W lags, every frame
            assert np.all(sto == 7) and np.all(st["acf_dropped"][p][-3:] == fpp) and not st["acf_dropped"][p][:-3].any()
            assert not st["acf_sums"][p][-3:].any() and np.all(np.isnan(st["mean_acf"][p][-3:]))
        if kind in ("clean", "h", "fading", "register"):
            assert not st["acf_dropped"][p].any()
    assert np.all(st["tg_position"][st["status"] == 1] == 65)
    if W == cfg.T_guard:                                          # the noise point: the oracle finds no plateau, nor does the study
        noise = np.asarray(plan.tx_frames_fused(fpp, SNR=snrs[2], seed=seeds[2], frame0=f0, **kw)["rx"]).astype(np.complex128)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            oks = [oracle.AutoCorrFunction(noise[:, f], W, cfg.Nfft)[3] for f in range(fpp)]
        assert not all(oks)
        assert st["fallback"][2] >= 1 and st["fallback"][2] == fpp - sum(oks)
    if kind == "register":
        # a fixed shift of 0.24 at 25 dB.  e is wrapped into [-0.5, 0.5]: an estimate that knew nothing of the shift would be
        # uniform there, mean |e| = 0.25; one that does is below it.  (mean |e|)^2 <= mean e^2 is Cauchy-Schwarz.
        m1, m2 = st["ffo_err"][1] / fpp
        print(f"{precision}: Freq_Shift 0.24 at 25 dB, mean |e| {m1:.3g}, rms {np.sqrt(m2):.3g}")
        assert 0 < m1 < 0.25 and m1 * m1 <= m2 * (1 + 1e-12)
        assert np.array_equal(st["mean_abs_ffo_err"], st["ffo_err"][:, 0] / fpp)
    # without the optional outputs the rest is the same
    plain = plan.sync_study(snrs, fpp, seeds=seeds, frame0=f0, width=W, **kw)
    assert set(plain) == {"acf_sums", "acf_dropped", "mean_acf", "tg_hist", "fallback", "phase_hist", "ffo_err", "mean_abs_ffo_err"}
    for key in plain:
        assert np.array_equal(plain[key], st[key], equal_nan=True), key
    plan.close()


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_no_output_depends_on_the_chunking_or_the_flavour(ofdm, oracle, precision):
    import torch
    from ofdm_course_amd import frames as fr
    cfg = _cfg()
    plan = fr.make_plan(cfg, ofdm, precision=precision, device=0)
    kw = dict(Time_Delay="random", Freq_Shift="random", seeds=[1, 2, 3], frame0=1, want_peak=True, want_frames=True)   # no channel: zero tails
    snrs = [-40.0, 15.0, 30.0]
    base = plan.sync_study(snrs, 5, **kw)
    assert base["fallback"][0] >= 1 and base["acf_dropped"].any()
    for chunk in (1, 3):
        got = plan.sync_study(snrs, 5, max_frames_per_chunk=chunk, **kw)
        assert set(got) == set(base)
        for key in got:
            assert np.array_equal(got[key], base[key], equal_nan=True), (chunk, key)
    nofr = plan.sync_study(snrs, 5, max_frames_per_chunk=3, **dict(kw, want_frames=False))   # the scalars in the call's scratch
    for key in nofr:
        assert np.array_equal(nofr[key], base[key], equal_nan=True), key
    dev = plan.sync_study(snrs, 5, device="cuda:0", max_frames_per_chunk=3, **kw)
    torch.cuda.synchronize()
    for key in base:
        assert dev[key].is_cuda and np.array_equal(dev[key].cpu().numpy(), base[key], equal_nan=True), key
    # no frames, no points: zero tables, nothing else touched
    none = plan.sync_study(snrs, 0, want_peak=True)
    assert none["acf_sums"].shape == (3, 1152) and not none["acf_sums"].any() and not none["tg_hist"].any()
    assert not none["phase_hist"].any() and not none["ffo_err"].any() and not none["fallback"].any() and not none["acf_peak"].any()
    assert plan.sync_study([], 5)["acf_sums"].shape == (0, 1152)
    plan.close()


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_agreement_with_the_task4_receiver(ofdm, oracle, precision):
    """width=None is the receiver's own window (T4/Main_model_Task_4.m:278): the same TgPosition, catch-branch flag and FreqOffset as
    rx_chain_task4 reports.  Its statuses -1 (no IFO line) and -2 (index error) belong to later stages: 0 here."""
    from ofdm_course_amd import frames as fr
    cfg = _cfg()
    plan = fr.make_plan(cfg, ofdm, precision=precision)
    h, _ = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    rx = np.asarray(plan.tx_frames_fused(6, h=h, SNR=20.0, seed=21, Time_Delay="random", Freq_Shift="random")["rx"])
    noise = np.asarray(plan.tx_frames_fused(2, SNR=-40.0, seed=22)["rx"])
    rx = np.concatenate([rx, noise], axis=1)
    got = ofdm.rx_acf(plan, rx)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        chain = ofdm.rx_chain_task4(plan, rx, time_desync=1, freq_desync=1, mp_desync=0)
    status = np.where(np.asarray(chain["status"]) < 0, 0, np.asarray(chain["status"]))
    print(f"{precision}: TgPosition {got['tg_position'].tolist()}, status {got['status'].tolist()} (receiver {np.asarray(chain['status']).tolist()})")
    assert np.array_equal(got["tg_position"], chain["TgPosition"])
    assert np.array_equal(got["status"], status)
    assert np.array_equal(_bits(got["freq_offset"]), _bits(np.asarray(chain["FreqOffset"])))
    assert (got["status"] == 0).any() and (got["status"] == 1).any()
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
    good_rx = ofdm.rx_acf(plan, rx, want_rho=True)
    good_st = plan.sync_study([20.0], 3, h=h, want_peak=True, want_frames=True)

    def same_rx():
        again = ofdm.rx_acf(plan, rx, want_rho=True)
        return all(np.array_equal(_bits(again[k]) if again[k].dtype.kind in "fc" else again[k],
                                  _bits(good_rx[k]) if again[k].dtype.kind in "fc" else good_rx[k]) for k in good_rx)

    def same_st():
        again = plan.sync_study([20.0], 3, h=h, want_peak=True, want_frames=True)
        return all(np.array_equal(again[k], good_st[k], equal_nan=True) for k in good_st)

    capture = [(dict(width=0), "WidthWindow must be 1 .. 1024 (0)"), (dict(width=-5), "WidthWindow must be 1 .. 1024 (-5)"),
               (dict(width=1025), "WidthWindow must be 1 .. 1024 (1025)"),
               (dict(width=1024), None)]                               # 1440 - 1024 - 256 = 160 lags: accepted
    for brk, msg in capture:
        if msg is None:
            assert ofdm.rx_acf(plan, rx, **brk)["amp"].shape == (2, 160)
            assert plan.sync_study([20.0], 3, h=h, **brk)["acf_sums"].shape == (1, 160)
            continue
        _refused(ofdm, lambda: ofdm.rx_acf(plan, rx, **brk), "rx_acf: " + msg)
        assert same_rx()
        _refused(ofdm, lambda: plan.sync_study([20.0], 3, h=h, **brk), "sync_study: " + msg)
        assert same_st()
    # a frame shorter than WidthWindow + Nfft + 1: a plan of one symbol (288 samples) at the receiver's window
    short_cfg = _cfg(n_symb=1)
    short = fr.make_plan(short_cfg, ofdm, precision=precision)
    msg = "a frame of 288 samples is shorter than WidthWindow + Nfft + 1 (32 + 256 + 1)"
    _refused(ofdm, lambda: ofdm.rx_acf(short, rx[:288]), "rx_acf: " + msg)
    _refused(ofdm, lambda: short.sync_study([20.0], 3), "sync_study: " + msg)
    assert ofdm.rx_acf(short, rx[:288], width=31)["amp"].shape == (2, 1)       # n_out = 1: the catch branch, no lag 65
    one = ofdm.rx_acf(short, rx[:288], width=31)
    assert np.all(one["status"] == 1) and np.all(one["tg_position"] == 65) and np.all(np.isnan(one["freq_offset"]))
    st1 = short.sync_study([20.0], 3, width=31)                          # n_out <= 64: fallback frames are counted in fallback alone
    assert st1["fallback"][0] == 3 and st1["tg_hist"].sum() == 0 and st1["phase_hist"].sum() == 3 and np.isnan(st1["ffo_err"]).all()
    short.close()
    study = [(dict(max_frames_per_chunk=-1), "sync_study: bad arguments"),
             (dict(frames_per_point=-1), "sync_study: bad arguments"),
             (dict(frame0=(1 << 32) - 3), "sync_study: frame index outside the 32-bit stream range"),
             (dict(Register=(1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 2)), "sync_study: register entries must be 0 or 1"),
             (dict(fading=([0, 3], [1.0, 0.5])), "sync_study: give h (one channel for every frame) or taps (a channel per frame), not both"),
             (dict(h=None, fading=([0, 3, 3], [1.0, 0.5, 0.5])), "sync_study: tap delay 3 given twice"),
             (dict(h=None, fading=([0, 4097], [1.0, 0.5]), width=0), "sync_study: tap delay 4097 outside 0 .. 4096"),
             (dict(h=np.ones(65)), "tx_frames_fused: 65 nonzero channel taps (at most 64)"),
             (dict(Time_Delay="random", width=0), "sync_study: WidthWindow must be 1 .. 1024 (0)")]
    for brk, msg in study:
        args = dict(dict(SNRs=[20.0], frames_per_point=3, h=h), **brk)
        _refused(ofdm, lambda: plan.sync_study(**args), msg)
        assert same_st()
    # the table of sync_cases.py: every refusal of both entries that a caller can reach through the Python layer
    assert {rid for rid, _, _ in sc.capture_order()} == {"width", "short", "output"}
    # through the C entry: no output at all, the precision flag of the other precision, no plan, no frames pointer, a bad count
    flags = L.OFDM_F64 if precision == "fp64" else L.OFDM_F32
    buf = np.ascontiguousarray(rx.T)
    amp = np.full((2, 1152), -1.0, np.float64 if precision == "fp64" else np.float32)
    p_rx, p_amp = buf.ctypes.data_as(C.c_void_p), amp.ctypes.data_as(C.c_void_p)
    lib = plan.lib
    for args, msg in [((plan.handle, p_rx, 2, 32, None, None, None, None, None, flags), "rx_acf: no output is given"),
                      ((plan.handle, p_rx, 2, 32, p_amp, None, None, None, None, flags ^ L.OFDM_F64), "rx_acf: precision flag differs from the plan's"),
                      ((plan.handle, None, 2, 32, p_amp, None, None, None, None, flags), "rx_acf: bad arguments"),
                      ((None, p_rx, 2, 32, p_amp, None, None, None, None, flags), "rx_acf: bad arguments"),
                      ((plan.handle, p_rx, -1, 32, p_amp, None, None, None, None, flags), "rx_acf: n_frames must be 0 .. 2^31 - 1 (-1)")]:
        rc = lib.ofdm_rx_acf(*args)
        assert rc < 0 and msg in lib.ofdm_last_error_string().decode(), (msg, lib.ofdm_last_error_string())
        assert (amp == -1.0).all()                                # nothing was written
    L.check(lib.ofdm_rx_acf(plan.handle, p_rx, 2, 32, p_amp, None, None, None, None, flags), "rx_acf")
    assert np.array_equal(_bits(amp), _bits(good_rx["amp"]))      # amp alone: every other output is optional
    snr, sd = np.array([20.0]), np.array([1], np.uint64)
    rc = lib.ofdm_sync_study(plan.handle, None, 0, None, None, 0, 0, 0, 0, 0.0, None, snr.ctypes.data_as(C.c_void_p),
                             sd.ctypes.data_as(C.c_void_p), 1, 3, 0, 0, 32, None, None, None, None, None, None, None, None, None, None,
                             flags)
    assert rc < 0 and "sync_study: no output is given" in lib.ofdm_last_error_string().decode()
    sums = np.full((1, 1152), -1.0)
    L.check(lib.ofdm_sync_study(plan.handle, None, 0, None, None, 0, 0, 0, 0, 0.0, None, snr.ctypes.data_as(C.c_void_p),
                                sd.ctypes.data_as(C.c_void_p), 1, 3, 0, 0, 32, sums.ctypes.data_as(C.c_void_p), None, None, None, None,
                                None, None, None, None, None, flags), "sync_study")
    assert np.array_equal(sums, plan.sync_study([20.0], 3, seeds=[1])["acf_sums"])      # the sums alone: every table is optional
    assert same_st()
    plan.close()


def test_task4_acf_driver_replays_the_report_figures(ofdm, tmp_path):
    """python -m ofdm_course_amd.drivers.task4_acf on three frames per point: on the clean channel W = 1 gives |rho| = 1 at every lag
    (no plateau edge: the catch branch), W = T_guard / 2 and T_guard put a plateau of T_guard - W + 1 lags at one at every symbol
    start, and the fractional error of figure 13a falls with the SNR."""
    import json
    from ofdm_course_amd.drivers import task4_acf as t4a
    out = tmp_path / "out.json"
    t4a.main(["--json", str(out), "--frames", "3"])
    res = json.loads(out.read_text())
    assert res["frames"] == 3 and res["T_guard"] == 128 and list(res["acf"]) == [n for n, _, _ in t4a.ACF_FIGURES]
    acf = {n: {k: np.asarray(v) if isinstance(v, list) else v for k, v in s.items()} for n, s in res["acf"].items()}
    assert np.max(np.abs(acf["W_1"]["mean_acf"] - 1.0)) < 1e-11 and acf["W_1"]["fallback"] == 3
    for name, w in (("W_half_guard", 64), ("W_guard", 128)):
        m = acf[name]["mean_acf"]
        assert acf[name]["n_out"] == 5760 - w - 1024 and acf[name]["fallback"] == 0 and not acf[name]["acf_dropped"].any()
        for s in range(4):
            assert np.max(np.abs(m[s * 1152: s * 1152 + 128 - w + 1] - 1.0)) < 1e-11
            assert m[s * 1152 + 576] < 0.77
        assert acf[name]["phase_hist"].sum() == 3 and acf[name]["tg_hist"].sum() == 3
    assert acf["W_nfft"]["n_out"] == 5760 - 2048 and np.all(acf["W_nfft"]["mean_acf"] <= 1.0 + 1e-11)
    ffo = res["ffo"]
    err = np.asarray(ffo["mean_abs_err"])
    # below about 5 dB the plateau stays under 0.77 (|rho| = SNR / (1 + SNR)) and the catch branch reads lag 65: an error of order
    # 0.25; above, it falls to the floor the run's middle leaves, a few lags off the one-lag plateau of W = T_guard
    assert err.shape == (61,) and np.all(np.isfinite(err)) and np.mean(err[-10:]) < np.mean(err[:10]) and err[-1] < 0.01
