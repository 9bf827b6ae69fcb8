"""The restatement of fine_sync's curve (tests/fine_cases.py: taus, keep, n_used from the oracle's own expressions) against the oracle
on the CPU: the mean of taus[keep] behind the first Np kept entries is oracle.fine_sync's tau bit for bit, for both variants, on
noisy and clean frames; and the timing-error formula e = tau Nfft + phi_s + 1 holds on the oracle for a window forced into the
guard interval.  Nothing here touches a GPU."""
import numpy as np
import pytest

import fine_cases as fc


def _same(a, b):
    return (np.isnan(a) and np.isnan(b)) or np.float64(a).tobytes() == np.float64(b).tobytes()


@pytest.mark.parametrize("variant", ["T4", "T5"])
@pytest.mark.parametrize("snr", [None, 30.0, 10.0])
def test_mean_of_the_kept_entries_is_the_oracles_tau_bit_for_bit(oracle, variant, snr):
    g = fc.geometry(oracle)
    Np = len(g["pc"])
    for D in (0, 5, 40):
        y = fc.oracle_frame(oracle, g, seed=7 + D, snr=snr, Time_Delay=D)
        X, _, _ = fc.oracle_front_end(oracle, g, y)
        for td in (0, 1):
            _, tau, ph = oracle.fine_sync(X, g["pc"], g["pv"], td, 0, variant=variant)
            r = fc.restate(X, g["pc"], g["pv"], variant, time_desync=td)
            assert r["taus"].shape == r["keep"].shape == (fc.fine_len(Np, g["N_symb"], variant),) and not r["keep"][0]
            sel = r["taus"][r["keep"]][Np:]
            assert r["n_used"] == sel.size
            assert _same(np.mean(sel) if sel.size else np.nan, tau) and _same(r["tau"], tau) and _same(r["phase"], ph)
            if variant == "T5":
                assert r["taus"][-1] == 0.0                              # the trailing 0 of T5/fine_sync.m:8
    # one symbol: the T4 variant keeps the Np allocated entries (the T5 length), nothing is left behind the first Np
    g1 = fc.geometry(oracle, N_symb=1)
    X = np.fft.fft(fc.oracle_frame(oracle, g1, seed=3, snr=snr).reshape((-1, 1), order="F")[g1["T_guard"]:], axis=0)
    r = fc.restate(X, g1["pc"], g1["pv"], variant)
    assert r["taus"].size == Np and r["taus"][-1] == 0.0 and r["n_used"] == 0 and np.isnan(r["tau"])
    assert np.isnan(oracle.fine_sync(X, g1["pc"], g1["pv"], 1, 0, variant=variant)[1])


def test_a_clean_frame_has_no_phase_and_low_snr_has_no_tau(oracle):
    """The issue's probe: on a clean frame every |qks| <= 1e-3 (phase = mean([]) = NaN), and at 10 dB the 1e-3 mask of the T4
    variant leaves nothing behind the first Np kept entries."""
    g = fc.geometry(oracle)
    X, _, _ = fc.oracle_front_end(oracle, g, fc.oracle_frame(oracle, g, seed=45, snr=None, Time_Delay=5))
    r = fc.restate(X, g["pc"], g["pv"], "T4")
    assert r["n_phase"] == 0 and np.isnan(r["phase"]) and np.isfinite(r["tau"])
    nan = 0
    for s in range(4):
        X, _, _ = fc.oracle_front_end(oracle, g, fc.oracle_frame(oracle, g, seed=60 + s, snr=10.0, Time_Delay=5))
        nan += np.isnan(fc.restate(X, g["pc"], g["pv"], "T4")["tau"])
    assert nan == 4


def test_timing_error_formula_on_the_oracle_for_a_window_inside_the_guard_interval(oracle):
    """Clean frames, TgPosition forced so that phi_s + 1 = -T_guard + 2 .. 0.  Asserted: |e| <= 10 x the largest the oracle itself
    shows (fine_cases.ORACLE_E_MAX_IN_RANGE, printed here) on the windows inside the unambiguous range of the angle, less than
    Nfft / (2 deltak) samples early; outside it the estimate is aliased by Nfft / deltak and e + Nfft / deltak is held to 10 x
    what the oracle shows for it.  Recorded, not bounded: the windows where the oracle's own tau is mean([]) = NaN (the T4 mask
    drops equal neighbours), and the late windows phi_s + 1 > 0, which take samples of the next symbol."""
    g = fc.geometry(oracle)
    N, Tg = g["Nfft"], g["T_guard"]
    stride = N + Tg
    period = N / (g["pc"][1] - g["pc"][0])
    worst_in = worst_alias = 0.0
    late, empty = [], []
    for D in (0, 5, 40, 200):
        y = fc.oracle_frame(oracle, g, seed=100 + D, snr=None, Time_Delay=D)
        for variant in ("T4", "T5"):
            for k in range(-Tg + 2, 4):                                  # k = phi_s + 1
                tg = (k - 1 - D) % stride + 1
                assert fc.phase_wrapped(tg, D, stride) == k - 1
                X, _, _ = fc.oracle_front_end(oracle, g, y, tg_position=tg)
                tau = oracle.fine_sync(X, g["pc"], g["pv"], 1, 0, variant=variant)[1]
                e = fc.tau_err(tau, tg, D, N, stride)
                if k > 0:
                    late.append((D, variant, k, float(e)))
                    continue
                if np.isnan(tau):                                        # mean([]): the T4 mask drops equal neighbours (:33) -- no
                    empty.append((D, variant, k))                        # estimate, nothing for the formula to say
                    continue
                if -k < period / 2:
                    assert abs(e) <= fc.E_BOUND, (D, variant, k, e)
                    worst_in = max(worst_in, abs(e))
                else:
                    assert abs(e + period) <= fc.E_BOUND_ALIASED, (D, variant, k, e)
                    worst_alias = max(worst_alias, abs(e + period))
    print(f"largest |e| inside the unambiguous range {worst_in!r}, of e + Nfft / deltak outside it {worst_alias!r}; late windows: "
          f"{late}; no estimate: {empty}")
    assert worst_in <= fc.ORACLE_E_MAX_IN_RANGE and worst_alias <= fc.ORACLE_E_MAX_ALIASED     # the recorded figures still hold
    assert len(late) == 4 * 2 * 3 and all(v == "T4" for _, v, _ in empty) and len(empty) < 4 * (Tg - 1) // 2
