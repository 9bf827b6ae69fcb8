"""The accumulate stage of the spectrum, sync, fine and IFO studies past the first iteration of its two loops.

The study suites run at most 32 frames per point: one 64-row tile of the column loop, one 256-frame block of the scalar loop.
Here every study runs 260 frames per point, once in one chunk (four full tiles and a tail of 4; one full scalar block and a tail
of 4) and once capped at 70 frames per chunk (70, 70, 70, 50: a tile boundary inside a chunk, a chunk shorter than a tile, every
chunk resuming on the accumulators the one before left).  That one uncapped chunk holds all 260 frames is asserted with the chunk
models of tests/*_cases.py (the twins of the plans' *_chunk, held to the headers by the host tests).

The reference is the host rebuild of the study's own suite -- _rebuild of test_gpu_spectrum.py, test_gpu_sync_study.py and
test_gpu_ifo_study.py: the per-frame entry on tx_frames_fused output, summed left to right in float64 from 0, the values that are
not finite skipped and counted, np.fmax from 0, the scalar sums through the twins of tests/*_cases.py.  The fine study has no
per-frame entry on received frames (rx_fine takes the demodulator's output, which no entry returns), so its rows are the study's own
at one frame per call -- one row, the first of one tile: 0 + t, or a dropped count of 1 -- summed the same way, and its scalar sums are
rebuilt from the per-frame outputs of the 260-frame call through the twin of fine_cases.py; in fp64 the call is also held to
_reference_study / _check_study of test_gpu_fine_study.py, the oracle's composition, at that suite's own bounds.

Every comparison is bit for bit: equal bit patterns on every number, NaN in the same places (a NaN has no value to compare)."""
import numpy as np
import pytest

import fine_cases as fc
import ifo_cases as ic
import spectrum_cases as spc
import sync_cases as sc
import test_gpu_fine_study as fine_suite
import test_gpu_ifo_study as ifo_suite
import test_gpu_spectrum as spectrum_suite
import test_gpu_sync_study as sync_suite

pytestmark = pytest.mark.gpu

FPP, CAP = 260, 70                                            # 4 x 64 + 4 = 256 + 4; 70 = 64 + 6, 260 = 3 x 70 + 50
SEEDS, F0 = [3, 0x1234ABCD5, 9], 6                            # the study suites' own


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if want.dtype.kind != "f":
        return got.shape == want.shape and np.array_equal(got, want)
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan])


def _both_chunkings(study, **kw):
    """The study in one chunk and capped at CAP frames per chunk: every output the same bytes."""
    whole, capped = study(max_frames_per_chunk=0, **kw), study(max_frames_per_chunk=CAP, **kw)
    assert set(whole) == set(capped)
    for key in whole:
        assert _same(capped[key], whole[key]), ("capped at %d" % CAP, key)
    return whole


def _cfg(**kw):
    from ofdm_course_amd import frames as fr
    return fr.config_small(**kw)


def test_one_chunk_holds_every_frame():
    """The chunk rule at the shapes below, both precisions, with every region the generator can ask for: 260 frames are one chunk."""
    short = dict(sc.SHAPE, n_symb=1, frame_words=6)
    fine = dict(sc.SHAPE, n_symb=6, n_carrier=100, np=18, nd=82, frame_words=62)           # fc.geometry
    for f64 in (0, 1):
        assert spc.chunk_model(sc.SHAPE, f64, 1, 1, 64, FPP, 0, 1) == FPP
        assert sc.chunk_model(sc.SHAPE, f64, 1, 1, 64, FPP, 0, 4) == FPP and sc.chunk_model(short, f64, 1, 1, 64, FPP, 0, 31) == FPP
        assert fc.chunk_model(fine, f64, 1, 1, 64, FPP, 0, "T4") == FPP
        assert ic.chunk_model(sc.SHAPE, f64, 1, 1, 64, FPP, 0) == FPP
        assert sc.chunk_model(sc.SHAPE, f64, 1, 1, 64, FPP, CAP, 4) == CAP


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_spectrum_study(ofdm, oracle, precision):
    """Nfft 256: four column workgroups, no tail workgroup; the peak folds a second array (the single-window rows)."""
    from ofdm_course_amd import frames as fr
    cfg = _cfg()
    plan = fr.make_plan(cfg, ofdm, precision=precision)
    h, _ = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    kw = dict(h=h, Time_Delay="random", Freq_Shift="random")
    snrs, first, nw = [8.0, 25.0], cfg.T_guard + 1, 2
    st = _both_chunkings(plan.spectrum_study, SNRs=snrs, frames_per_point=FPP, seeds=SEEDS[:2], frame0=F0, first=first,
                         n_windows=nw, want_peak=True, want_frame_power=True, **kw)
    for p in range(2):
        want = spectrum_suite._rebuild(plan, ofdm, cfg, first, nw, snrs[p], SEEDS[p], FPP, F0, kw)
        for key, val in want.items():
            assert _same(st[key][p], val), (p, key)
    plan.close()


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_sync_study(ofdm, oracle, precision):
    """Time_Delay = 7 without a channel at W = 4: n_out = 1180 = 18 x 64 + 28, the last column workgroup has idle lanes, and the
    last three lags are 0 / 0 in every frame -- dropped 260 times each; the -40 dB point is noise alone.  Then a frame of one symbol
    at W = 31: n_out = 1, the catch branch finds no lag 65, FreqOffset is NaN, and the wrapped error, NaN, is added like any other:
    sync adds whatever the frame left, so ffo_err is NaN from the first frame on (line `s1 += fabs(e)` of the scalar tail with the
    skip switched off)."""
    from ofdm_course_amd import frames as fr
    cfg = _cfg()
    plan = fr.make_plan(cfg, ofdm, precision=precision)
    kw, W, snrs = dict(Time_Delay=7), 4, [25.0, -40.0]
    st = _both_chunkings(plan.sync_study, SNRs=snrs, frames_per_point=FPP, seeds=SEEDS[:2], frame0=F0, width=W, want_peak=True,
                         want_frames=True, **kw)
    assert st["acf_sums"].shape == (2, 1180)
    for p in range(2):
        want, sto = sync_suite._rebuild(plan, ofdm, cfg, W, snrs[p], SEEDS[p], FPP, F0, kw)
        for key, val in want.items():
            assert _same(st[key][p], val), (p, key)
        assert np.all(sto == 7) and np.all(st["acf_dropped"][p][-3:] == FPP) and not st["acf_dropped"][p][:-3].any()
        assert not st["acf_sums"][p][-3:].any()
    print(f"{precision}: fallback {st['fallback'].tolist()}, ffo_err {st['ffo_err'].tolist()}")
    plan.close()
    short_cfg = _cfg(n_symb=1)
    short = fr.make_plan(short_cfg, ofdm, precision=precision)
    kw = dict(Freq_Shift="random")
    st = _both_chunkings(short.sync_study, SNRs=[20.0], frames_per_point=FPP, seeds=SEEDS[:1], frame0=F0, width=31, want_peak=True,
                         want_frames=True, **kw)
    want, _ = sync_suite._rebuild(short, ofdm, short_cfg, 31, 20.0, SEEDS[0], FPP, F0, kw)
    for key, val in want.items():
        assert _same(st[key][0], val), ("one symbol", key)
    assert st["fallback"][0] == FPP and np.isnan(st["freq_offset"]).all() and np.isnan(st["ffo_err"]).all()
    short.close()


def _fine_scalars(st, p, g):
    """tau_err and phase_sums of point p from the call's per-frame outputs: left to right from 0, the values that are not finite
    skipped (and counted)."""
    N, stride = g["Nfft"], g["Nfft"] + g["T_guard"]
    e1 = e2 = p1 = p2 = np.float64(0.0)
    e_nan = p_nan = 0
    for f in range(st["frame_tau"].shape[1]):
        e = fc.tau_err(st["frame_tau"][p, f], st["frame_tg_position"][p, f], st["frame_time_delay"][p, f], N, stride)
        ph = np.float64(st["frame_phase"][p, f])
        if np.isfinite(e):
            e1, e2 = e1 + np.abs(e), e2 + e * e
        else:
            e_nan += 1
        if np.isfinite(ph):
            p1, p2 = p1 + ph, p2 + ph * ph
        else:
            p_nan += 1
    return dict(tau_err=np.array([e1, e2]), phase_sums=np.array([p1, p2]), tau_nan=e_nan, phase_nan=p_nan)


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_fine_study(ofdm, oracle, precision):
    """L = 107 = 64 + 43: two column workgroups, the second with idle lanes, and the tail workgroup with two columns.  The 16 dB
    point has frames whose tau = mean([]) is NaN (test_fine_study_histogram_identity_with_nan_frames): their timing error is NaN and
    is left out of tau_err, and so is their phase, NaN too, out of phase_sums.  The second point is 30 dB, not a clean one: on clean
    frames most differences of neighbouring taus are ties at 0, where the mask of the oracle's composition and the device's differ
    by a rounding (the fine suite compares with the oracle at 16 .. 30 dB only)."""
    g = fc.geometry(oracle)
    plan = fine_suite._plan(ofdm, g, precision)
    snrs, kw, bins = [16.0, 30.0], dict(Time_Delay=5, seed=5), fine_suite.BINS
    st = _both_chunkings(plan.fine_study, SNRs=snrs, frames_per_point=FPP, bins=bins, want_frames=True, **kw)
    L = fc.fine_len(len(g["pc"]), g["N_symb"], "T4")
    assert L == 107 and st["tau_curve_sums"].shape == (2, L)
    for p in range(2):
        acc, dropped, keep = np.zeros(L, np.float64), np.zeros(L, np.int64), np.zeros(L, np.int64)
        for f in range(FPP):                                  # the frame's row: the study at this one frame
            one = plan.fine_study([snrs[p]], 1, bins=bins, frame0=f, **kw)
            assert np.all(one["curve_dropped"][0] <= 1) and not one["tau_curve_sums"][0][one["curve_dropped"][0] == 1].any()
            acc = acc + one["tau_curve_sums"][0]
            dropped += one["curve_dropped"][0]
            keep += one["keep_counts"][0]
        assert _same(st["tau_curve_sums"][p], acc) and _same(st["curve_dropped"][p], dropped) and _same(st["keep_counts"][p], keep), p
        for key, val in _fine_scalars(st, p, g).items():
            assert _same(st[key][p], val), (p, key)
    print(f"{precision}: tau_nan {st['tau_nan'].tolist()}, phase_nan {st['phase_nan'].tolist()}, tau_err {st['tau_err'].tolist()}")
    assert 0 < st["tau_nan"][0] < FPP and 0 < st["phase_nan"][0] < FPP and np.all(np.isfinite(st["tau_err"]))
    assert np.all(np.isfinite(st["phase_sums"]))
    if precision == "fp64":                                   # the oracle's composition, at the fine suite's bounds
        ref = fine_suite._reference_study(ofdm, oracle, plan, g, snrs, FPP, "T4", 1, 0, bins, **kw)
        fine_suite._check_study(st, ref, 2, FPP)
    plan.close()


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_ifo_study(ofdm, oracle, precision):
    """The receiver's stage on the drawn impairments, with the noise point; then the raw stage behind Time_Delay = -512 without a
    channel: samples 0 .. 511 of the frame are add_STO's zeros with the noise on them, the window Nfft .. 2 Nfft - 1 holds noise
    alone, and a frame whose noise has no bin above 0.77 has no line: its total error is NaN and is left out of cfo_err (at 3000 dB
    every frame, and cfo_err stays 0)."""
    from ofdm_course_amd import frames as fr
    cfg = _cfg()
    plan = fr.make_plan(cfg, ofdm, precision=precision)
    h, _ = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    runs = [("receiver", dict(h=h, Time_Delay="random", Freq_Shift="random"), [25.0, -40.0], 2),
            ("raw", dict(Time_Delay=-512, Freq_Shift="random"), [3000.0, 6.0, 3.0], 32)]
    for stage, kw, snrs, span in runs:
        n = len(snrs)
        st = _both_chunkings(plan.ifo_study, SNRs=snrs, frames_per_point=FPP, seeds=SEEDS[:n], frame0=F0, stage=stage,
                             time_desync=1, err_span=span, want_frames=True, **kw)
        for p in range(n):
            want = ifo_suite._rebuild(plan, ofdm, cfg, stage, 1, span, snrs[p], SEEDS[p], FPP, F0, kw)
            for key, val in want.items():
                assert _same(st[key][p], val), (stage, p, key)
        print(f"{precision} {stage}: no_line {st['no_line'].tolist()}, cfo_err {st['cfo_err'].tolist()}")
        assert np.all(np.isfinite(st["cfo_err"]))
        if stage == "raw":
            assert st["no_line"][0] == FPP and not st["cfo_err"][0].any()
    plan.close()
