"""The fine-sync capture on the GPU: rx_fine (ofdm_rx_fine) against the restatement of the oracle's expressions (tests/fine_cases.py)
and against fine_sync bit for bit, and RxPlan.fine_study (ofdm_fine_study) call by call against tx_frames_fused -> the oracle's
front end -> the restatement, under every chunking, with its histogram identity and its refusals."""
import numpy as np
import pytest

import fine_cases as fc
from conftest import crandn

pytestmark = pytest.mark.gpu


def _plan(ofdm, g, precision="fp64"):
    return ofdm.RxPlan(g["Nfft"], g["T_guard"], g["N_symb"], g["N_carrier"], g["pc"], g["dc"], g["col"], min(8, len(g["pc"])), 1,
                       "16QAM", precision=precision)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _pilot_frames(rng, g, n, tau=2e-4, noise=1e-6, dt=np.complex128):
    """Frames whose pilot rows carry a residual delay tau inside the 1e-3 mask and a little noise: most pairs are kept."""
    N, S = g["Nfft"], g["N_symb"]
    X = crandn(rng, N, S, n)
    X[np.rint(g["pc"]).astype(int) - 1, :, :] = g["pv"][:, :, None]
    X = X * np.exp(-2j * np.pi * tau * np.arange(N))[:, None, None] + noise * crandn(rng, N, S, n)
    return X.astype(dt)


@pytest.mark.parametrize("variant", ["T4", "T5"])
def test_rx_fine_matches_the_restatement_of_the_oracle(ofdm, oracle, variant):
    """Noisy frames through the oracle's front end; taus to the tolerance test_fine_sync holds tau to in double, keep and n_used exact.
    The seeds are chosen so that no |diff| of the oracle sits within 1e-9 of the mask's 1e-3 (asserted)."""
    g = fc.geometry(oracle)
    plan = _plan(ofdm, g)
    Xs = [fc.oracle_front_end(oracle, g, fc.oracle_frame(oracle, g, seed=1000 + s, snr=snr, Time_Delay=5))[0]
          for s, snr in enumerate([30.0, 25.0, 20.0, 16.0, 10.0])]
    got = ofdm.rx_fine(plan, np.stack(Xs, axis=2), variant=variant, time_desync=1, want_taus=True, want_keep=True)
    for f, X in enumerate(Xs):
        r = fc.restate(X, g["pc"], g["pv"], variant)
        Np = len(g["pc"])                                                # symbol 1 is blanked by the add_STO pair: its Np entries
        assert not np.any(r["taus"][:Np]) and not np.any(r["diffs"][Np - 1:] == 0)       # are exact zeros, no other diff is 0
        assert not np.any(np.abs(np.abs(r["diffs"]) - 1e-3) < 1e-9)
        assert got["taus"].shape == (len(Xs), r["taus"].size)
        assert np.max(np.abs(got["taus"][f] - r["taus"])) < 1e-12
        assert np.array_equal(got["keep"][f].astype(bool), r["keep"]) and got["n_used"][f] == r["n_used"]
        assert got["n_phase"][f] == r["n_phase"]
        if np.isnan(r["tau"]):
            assert np.isnan(got["tau"][f]) and np.isnan(got["phase"][f])
        else:
            assert abs(got["tau"][f] - r["tau"]) < 1e-12 and abs(got["phase"][f] - r["phase"]) < 1e-10
    plan.close()


def test_rx_fine_second_trip_carries_the_kept_rank(ofdm, oracle):
    """The T4 geometry with 16 symbols: M = 68 * 16 = 1088 > 256 threads x 4 entries, so the last 63 entries are a second trip whose
    rank among the kept entries starts where the first trip's ended."""
    g = fc.geometry(oracle, Nfft=1024, T_guard=128, N_symb=16, N_carrier=400)
    assert len(g["pc"]) == 68
    plan = _plan(ofdm, g)
    X = _pilot_frames(np.random.default_rng(3), g, 3)
    for variant in ("T4", "T5"):
        got = ofdm.rx_fine(plan, X, variant=variant, want_taus=True, want_keep=True)
        for f in range(3):
            r = fc.restate(X[:, :, f], g["pc"], g["pv"], variant)
            assert r["taus"].size == (1087 if variant == "T4" else 1088) and r["keep"][1024:].sum() > 30 and r["n_used"] > 900
            assert not np.any(np.abs(np.abs(r["diffs"]) - 1e-3) < 1e-9)
            assert np.array_equal(got["keep"][f].astype(bool), r["keep"]) and got["n_used"][f] == r["n_used"]
            assert np.max(np.abs(got["taus"][f] - r["taus"])) < 1e-12 and abs(got["tau"][f] - r["tau"]) < 1e-12
    plan.close()


def test_rx_fine_one_symbol_and_clean_frame(ofdm, oracle):
    """One symbol: M - 1 < Np gives the T5 length rule for both variants, a trailing 0, n_used = 0 and tau NaN.  A clean frame: every
    |qks| <= 1e-3, phase NaN with n_phase = 0."""
    g1 = fc.geometry(oracle, N_symb=1)
    plan = _plan(ofdm, g1)
    X = _pilot_frames(np.random.default_rng(4), g1, 2)
    for variant in ("T4", "T5"):
        got = ofdm.rx_fine(plan, X, variant=variant, want_taus=True, want_keep=True)
        assert got["taus"].shape == (2, len(g1["pc"])) and np.all(got["taus"][:, -1] == 0.0)
        assert np.all(got["n_used"] == 0) and np.all(np.isnan(got["tau"])) and np.all(np.isnan(got["phase"]))
        r = fc.restate(X[:, :, 0], g1["pc"], g1["pv"], variant)
        assert np.array_equal(got["keep"][0].astype(bool), r["keep"]) and np.max(np.abs(got["taus"][0] - r["taus"])) < 1e-12
    plan.close()
    g = fc.geometry(oracle)
    plan = _plan(ofdm, g)
    Xc, _, _ = fc.oracle_front_end(oracle, g, fc.oracle_frame(oracle, g, seed=45, snr=None, Time_Delay=5))
    got = ofdm.rx_fine(plan, Xc)
    assert got["n_phase"][0] == 0 and np.isnan(got["phase"][0]) and np.isfinite(got["tau"][0]) and got["n_used"][0] > 0
    plan.close()


@pytest.mark.parametrize("precision,dt", [("fp32", np.complex64), ("fp64", np.complex128)])
@pytest.mark.parametrize("variant", ["T4", "T5"])
@pytest.mark.parametrize("td", [0, 1])
def test_rx_fine_estimates_are_fine_syncs_bit_for_bit(ofdm, oracle, precision, dt, variant, td):
    g = fc.geometry(oracle)
    plan = _plan(ofdm, g, precision)
    rng = np.random.default_rng(17)
    X = np.concatenate([_pilot_frames(rng, g, 2, dt=dt), _pilot_frames(rng, g, 2, tau=3e-3, noise=3e-2, dt=dt)], axis=2)
    got = ofdm.rx_fine(plan, X, variant=variant, time_desync=td)
    finite = 0
    for f in range(X.shape[2]):
        _, tau, ph = ofdm.fine_sync(np.ascontiguousarray(X[:, :, f]), g["pc"], g["pv"].astype(dt), td, 0, variant=variant,
                                    return_estimates=True)
        assert _bits(got["tau"][f]) == _bits(tau) and _bits(got["phase"][f]) == _bits(ph), (f, got["tau"][f], tau, got["phase"][f], ph)
        finite += np.isfinite(tau)
    assert finite >= 2
    plan.close()


def _reference_study(ofdm, oracle, plan, g, snrs, fpp, variant, td, fd, bins, **gen):
    """fine_study call by call: tx_frames_fused -> the oracle's front end -> the restatement, summed in frame order."""
    N, stride, Np = g["Nfft"], g["Nfft"] + g["T_guard"], len(g["pc"])
    L = fc.fine_len(Np, g["N_symb"], variant)
    out = dict(sums=np.zeros((len(snrs), L)), dropped=np.zeros((len(snrs), L), np.int64), keep=np.zeros((len(snrs), L), np.int64),
               hist=[], err=np.zeros((len(snrs), 2)), ph=np.zeros((len(snrs), 2)), ph_nan=np.zeros(len(snrs), np.int64),
               used=np.zeros(len(snrs), np.int64), tgh=np.zeros((len(snrs), stride), np.int64), tg=[], tau=[], td=[])
    for p, snr in enumerate(snrs):
        fr = plan.tx_frames_fused(fpp, SNR=snr, seed=gen.get("seed", 1), want_draws=True,
                                  **{k: v for k, v in gen.items() if k != "seed"})
        errs = []
        for f in range(fpp):
            X, tg, _ = fc.oracle_front_end(oracle, g, fr["rx"][:, f], freq_desync=fd)
            r = fc.restate(X, g["pc"], g["pv"], variant, time_desync=td)
            sto = int(fr["Time_Delay"][f])
            fin = np.isfinite(r["taus"])
            out["sums"][p][fin] += r["taus"][fin]
            out["dropped"][p] += ~fin
            out["keep"][p] += r["keep"]
            e = fc.tau_err(r["tau"], tg, sto, N, stride)
            errs.append(e)
            if np.isfinite(e):
                out["err"][p, 0] += abs(e)
                out["err"][p, 1] += e * e
            if np.isfinite(r["phase"]):
                out["ph"][p, 0] += r["phase"]
                out["ph"][p, 1] += r["phase"] * r["phase"]
            else:
                out["ph_nan"][p] += 1
            out["used"][p] += r["n_used"]
            out["tgh"][p, fc.sc.phase_bin(tg, sto, stride)] += 1
            out["tg"].append(tg); out["tau"].append(r["tau"]); out["td"].append(sto)
        out["hist"].append(fc.histogram(errs, bins["n"], bins["lo"], bins["hi"]))
    return out


def _check_study(got, ref, n, fpp):
    scale = np.maximum(np.abs(ref["sums"]), 1e-3)                       # taus are ~1e-2: a floor for the entries that sum to ~0
    assert np.max(np.abs(got["tau_curve_sums"] - ref["sums"]) / scale) < 1e-12
    assert np.array_equal(got["curve_dropped"], ref["dropped"]) and np.array_equal(got["keep_counts"], ref["keep"])
    for p in range(n):
        hist, below, above, nan = ref["hist"][p]
        assert np.array_equal(got["tau_hist"][p], hist) and (got["tau_below"][p], got["tau_above"][p], got["tau_nan"][p]) == (below, above, nan)
        assert got["tau_hist"][p].sum() + got["tau_below"][p] + got["tau_above"][p] + got["tau_nan"][p] == fpp
    assert np.allclose(got["tau_err"], ref["err"], rtol=1e-9, atol=1e-12) and np.allclose(got["phase_sums"], ref["ph"], rtol=1e-9, atol=1e-12)
    assert np.array_equal(got["phase_nan"], ref["ph_nan"]) and np.array_equal(got["used_sums"], ref["used"])
    assert np.array_equal(got["tg_hist"], ref["tgh"])
    assert np.array_equal(got["frame_tg_position"].ravel(), ref["tg"]) and np.array_equal(got["frame_time_delay"].ravel(), ref["td"])
    assert np.allclose(got["frame_tau"].ravel(), ref["tau"], rtol=0, atol=1e-12, equal_nan=True)


BINS = dict(n=64, lo=-4.0, hi=4.0)
H3 = np.array([1.0, 0, 0, 0.5 + 0.2j, 0, 0, 0, -0.25j])


@pytest.fixture(scope="module")
def study_case(ofdm, oracle):
    g = fc.geometry(oracle)
    return g, _plan(ofdm, g)


@pytest.mark.parametrize("delay", [5, "random"])
def test_fine_study_call_by_call(ofdm, oracle, study_case, delay):
    """3 points x 8 frames, fixed and drawn Time_Delay, against the composition; and bitwise the same under every chunking."""
    g, plan = study_case
    snrs, fpp = [30.0, 22.0, 16.0], 8
    kw = dict(Time_Delay=delay, Register=[int(c) for c in fc.REGISTER], seed=5)
    got = plan.fine_study(snrs, fpp, bins=BINS, want_frames=True, **kw)
    ref = _reference_study(ofdm, oracle, plan, g, snrs, fpp, "T4", 1, 0, BINS, **kw)
    _check_study(got, ref, len(snrs), fpp)
    for cap in (1, 3):
        other = plan.fine_study(snrs, fpp, bins=BINS, want_frames=True, max_frames_per_chunk=cap, **kw)
        for k, v in got.items():
            a, b = np.asarray(v), np.asarray(other[k])
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), (cap, k)


def test_fine_study_histogram_identity_with_nan_frames(ofdm, oracle, study_case):
    """16 dB (chosen with the oracle: 6 of 16 of its frames have tau = mean([])): finite and NaN frames in one point."""
    g, plan = study_case
    got = plan.fine_study([16.0, 3000.0], 32, Time_Delay=5, want_frames=True)
    for p in range(2):
        assert got["tau_hist"][p].sum() + got["tau_below"][p] + got["tau_above"][p] + got["tau_nan"][p] == 32
        assert got["tau_nan"][p] == np.isnan(got["frame_tau"][p]).sum() and got["used_sums"][p] == got["frame_n_used"][p].sum()
        assert np.all((got["frame_n_used"][p] == 0) == np.isnan(got["frame_tau"][p]))
    assert 0 < got["tau_nan"][0] < 32
    assert got["tau_nan"][1] == 0 and got["tau_hist"][1].sum() == 32 and got["mean_abs_err"][1] < 0.05   # clean: e is ~0
    assert got["phase_nan"][1] + np.isfinite(got["frame_phase"][1]).sum() == 32
    assert np.all(got["keep_rate"] >= 0) and np.all(got["keep_rate"] <= 1) and got["keep_counts"][0].sum() < got["keep_counts"][1].sum()


def test_fine_study_with_fading_and_with_frequency_sync(ofdm, oracle, study_case):
    g, plan = study_case
    snrs, fpp = [28.0, 18.0], 6
    fading = ([0, 3, 7], [1.0, 0.3, 0.1])
    got = plan.fine_study(snrs, fpp, bins=BINS, want_frames=True, fading=fading, Time_Delay=12, seed=9)
    ref = _reference_study(ofdm, oracle, plan, g, snrs, fpp, "T4", 1, 0, BINS, fading=fading, Time_Delay=12, seed=9)
    _check_study(got, ref, 2, fpp)
    kw = dict(Time_Delay=7, Freq_Shift=1.24, seed=3, h=H3)
    for variant in ("T4", "T5"):
        got = plan.fine_study(snrs, fpp, bins=BINS, want_frames=True, time_desync=1, freq_desync=1, variant=variant, **kw)
        ref = _reference_study(ofdm, oracle, plan, g, snrs, fpp, variant, 1, 1, BINS, **kw)
        _check_study(got, ref, 2, fpp)


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_fine_study_front_end_is_the_receivers(ofdm, oracle, precision):
    """The direct form (Nfft 1024: compact pilot rows, t4_fine_est_kernel in the receiver): the study's TgPosition and status are
    rx_chain_task4's on the same frames, and its tau / phase are rx_fine's on the demodulator's output."""
    g = fc.geometry(oracle, Nfft=1024, T_guard=128, N_symb=5, N_carrier=400)
    plan = _plan(ofdm, g, precision)
    got = plan.fine_study([25.0], 6, Time_Delay=12, want_frames=True, seed=2)
    fr = plan.tx_frames_fused(6, SNR=25.0, seed=2, Time_Delay=12)
    rx = ofdm.rx_chain_task4(plan, fr["rx"], 1, 0, 0)
    assert np.array_equal(got["frame_tg_position"][0], rx["TgPosition"]) and np.array_equal(got["frame_status"][0], rx["status"])
    X = []
    for f in range(6):
        y = ofdm.add_STO(ofdm.add_STO(np.ascontiguousarray(fr["rx"][:, f]), int(rx["TgPosition"][f])), -(1024 + 128))
        X.append(np.asarray(ofdm.OFDM_demodulator(np.asarray(y).reshape((1024 + 128, 5), order="F"), 128)))
    one = ofdm.rx_fine(plan, np.stack(X, axis=2))
    tol = 1e-12 if precision == "fp64" else 2e-5                          # another transform in front: not the same bits
    assert np.allclose(got["frame_tau"][0], one["tau"], rtol=0, atol=tol, equal_nan=True)
    assert np.isfinite(got["frame_tau"][0]).sum() >= 3
    plan.close()


def test_refusals_reach_the_caller_in_the_plans_words(ofdm, oracle, study_case):
    g, plan = study_case
    E = ofdm.OfdmError
    X = np.zeros((g["Nfft"], g["N_symb"], 1), np.complex128)
    with pytest.raises(E, match="variant must be 'T4' or 'T5'"):
        ofdm.rx_fine(plan, X, variant="T3")
    with pytest.raises(E, match=r"rx_fine: X must be \[Nfft, N_symb, n_frames\]"):
        ofdm.rx_fine(plan, X[:-1])
    cases = [(dict(time_desync=0, freq_desync=0), "time_desync and freq_desync are both off"),
             (dict(bins=dict(n=0, lo=-4.0, hi=4.0)), r"bins must have n >= 1 and finite lo < hi \(0, -4, 4\)"),
             (dict(bins=dict(n=8, lo=1.0, hi=1.0)), "bins must have n >= 1"),
             (dict(bins=dict(n=8, lo=float("nan"), hi=1.0)), "bins must have n >= 1"),
             (dict(h=H3, fading=([0, 3], [1.0, 0.5])), "give h .* or taps .*, not both"),
             (dict(max_frames_per_chunk=65536), "fine_study: bad arguments"),
             (dict(Time_Delay="random", Register=[2] * 15), "register entries must be 0 or 1")]
    for kw, msg in cases:
        with pytest.raises(E, match=msg):
            plan.fine_study([20.0], 4, **kw)
    assert plan.fine_study([], 4)["tau_hist"].shape == (0, 64) and plan.fine_study([20.0], 0)["tau_nan"][0] == 0
