"""Cases of the fine-sync capture's call plan (csrc/fine_plan.hpp), shared by tests/test_fine_plan_host.py (the header, on the CPU,
through tests/host/fine_plan_main.cpp), tests/test_fine_restatement_host.py (the restatement below against the oracle) and
tests/test_gpu_fine_study.py (rx_fine and RxPlan.fine_study against the restatement, and the same refusals through the library).
TEST INFRASTRUCTURE: a hand-written model of the header, nothing here is read from it."""
import numpy as np

import sync_cases as sc

REGISTER = sc.REGISTER
SHAPE = sc.SHAPE                                                # Nfft 256, T_guard 32, 5 symbols, 64 carriers, 16 pilots
BUDGET = 2 * (2 << 30)                                          # the Task-4 sweep's: the workspace and the arena together
LDS_LIMIT = 150 << 10
THREADS, U = 256, 4
VARIANTS = {"T5": 0, "T4": 1}


# ---- the length of `taus`
def fine_len(n_pilots, n_symb, variant):
    """T5/fine_sync.m:8 allocates Np * N_symb entries (the loop leaves the last 0); T4/fine_sync.m:8 allocates Np and the loop of
    :25-30 grows it to Np * N_symb - 1, unless that is below Np.  variant: 0 / 1 or "T5" / "T4"."""
    t4 = variant in (1, "T4")
    M = n_pilots * n_symb
    return M - 1 if t4 and M - 1 >= n_pilots else M


# ---- the two frame functions
def phase_wrapped(tg_position, time_delay, stride):
    """phi = (TgPosition - 1 + Time_Delay) mod stride wrapped into (-stride / 2, stride / 2]."""
    phi = sc.phase_bin(tg_position, time_delay, stride)
    return phi - stride if 2 * phi > stride else phi


def tau_err(tau, tg_position, time_delay, nfft, stride):
    """e = tau * Nfft + phi_s + 1 in float64 (the product is exact: Nfft is a power of two)."""
    return np.float64(tau) * np.float64(nfft) + np.float64(phase_wrapped(tg_position, time_delay, stride) + 1)


BELOW, ABOVE, NAN = -1, -2, -3


def fine_bin(e, n, lo, hi):
    """NAN for a value that is not finite, BELOW for e < lo, ABOVE for e >= hi, else floor((e - lo) * n / (hi - lo)) held to n - 1."""
    e, lo, hi = np.float64(e), np.float64(lo), np.float64(hi)
    if not np.isfinite(e):
        return NAN
    if e < lo:
        return BELOW
    if not e < hi:
        return ABOVE
    return min(int((e - lo) * np.float64(n) / (hi - lo)), n - 1)


def histogram(errs, n, lo, hi):
    """(hist [n], below, above, nan) of a point's timing errors."""
    hist, tails = np.zeros(n, np.int64), {BELOW: 0, ABOVE: 0, NAN: 0}
    for e in errs:
        b = fine_bin(e, n, lo, hi)
        if b >= 0:
            hist[b] += 1
        else:
            tails[b] += 1
    return hist, tails[BELOW], tails[ABOVE], tails[NAN]


# ---- the restatement of fine_sync's curve from the oracle's own expressions (oracle/ofdm_oracle.py:389-418)
def _angle0(z):
    z = np.asarray(z)
    return np.where(z == 0, 0.0, np.angle(z))


def restate(X, pilotCarriers, pilotValues, variant, time_desync=1):
    """-> dict(taus [L], keep [L] bool, diffs [L - 1], n_used, tau, n_phase, phase) of one demodulated frame X [Nfft, N_symb]."""
    X = np.array(X, dtype=np.complex128)
    pc1 = np.asarray(pilotCarriers, dtype=np.float64).ravel()
    pc = np.rint(pc1).astype(np.int64) - 1
    tx = np.asarray(pilotValues)
    if tx.ndim == 1:
        tx = tx[:, None]
    txf = tx.ravel(order="F")
    rxf = X[pc, :].ravel(order="F")
    deltak = pc1[1] - pc1[0]
    q = txf * np.conj(rxf)
    taus = np.zeros(txf.size)
    taus[:-1] = _angle0(q[1:] * np.conj(q[:-1])) / (2 * np.pi * deltak)
    if variant == "T4" and txf.size - 1 >= pc.size:
        taus = taus[:-1]
    diffs = np.diff(taus)
    if variant == "T4":
        mask = np.concatenate([[False], (np.abs(diffs) < 1e-3) & (diffs != 0)])
    else:
        mask = np.concatenate([[False], np.abs(diffs) < 1e-3])
    sel = taus[mask][pc.size:]
    tau = np.mean(sel) if sel.size else np.nan
    if time_desync:
        nn = np.arange(X.shape[0], dtype=np.float64)
        X = X * np.conj(np.exp(-2j * np.pi * tau * nn))[:, None]
    qks = _angle0(txf * np.conj(X[pc, :].ravel(order="F")))
    selq = qks[np.abs(qks) > 1e-3]
    return dict(taus=taus, keep=mask, diffs=diffs, n_used=int(sel.size), tau=float(tau), n_phase=int(selq.size),
                phase=float(np.mean(selq)) if selq.size else float("nan"))


# ---- the geometry of the parity tests (the issue's): Nfft 256, T_guard 32, 6 symbols, 100 carriers, 15 % pilots, 16QAM
def geometry(o, Nfft=256, T_guard=32, N_symb=6, N_carrier=100, percent=15):
    pc, dc = o.pilot_layout_percent(Nfft, N_carrier, percent, 2)
    d = o.constellation_func("16QAM")[0]
    amp = 4 / 3 * np.max(np.abs(d))
    col = np.where(np.arange(len(pc)) % 2 == 0, amp, -amp).astype(np.complex128)
    return dict(Nfft=Nfft, T_guard=T_guard, N_symb=N_symb, N_carrier=N_carrier, pc=pc, dc=dc, col=col,
                pv=np.repeat(col[:, None], N_symb, axis=1))


def oracle_frame(o, g, seed, snr=None, Time_Delay=None, Freq_Shift=None):
    """One frame of the geometry through the oracle's TX and channel (PCG64 payload and noise draws keyed by `seed`)."""
    rng = np.random.default_rng(seed)
    n = (g["Nfft"] + g["T_guard"]) * g["N_symb"]
    bits = rng.integers(0, 2, len(g["dc"]) * g["N_symb"] * 4).astype(np.uint8)
    noise = (rng.standard_normal(n), rng.standard_normal(n)) if snr is not None else None
    y, _ = o.tx_frame(bits, g["Nfft"], g["T_guard"], g["N_symb"], g["dc"], g["pc"], g["pv"], "16QAM", SNR=snr, noise=noise,
                      Time_Delay=Time_Delay, Freq_Shift=Freq_Shift)
    return y


def oracle_front_end(o, g, y, tg_position=None, freq_desync=0):
    """The front end of T4/Main_model_Task_4.m:278-310 on the oracle: AutoCorrFunction(Rx, T_guard, Nfft) (or a forced
    TgPosition), add_STO x 2, with freq_desync add_CFO(-FreqOffset) and remove_IFO, OFDM_demodulator.  -> (X, TgPosition, ok)"""
    import warnings
    N, Tg, S = g["Nfft"], g["T_guard"], g["N_symb"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, tg, fo, ok = o.AutoCorrFunction(y, Tg, N)
    if tg_position is not None:
        tg = int(tg_position)
    y2 = o.add_STO(o.add_STO(y, tg), -(N + Tg))
    if freq_desync:
        y2 = o.add_CFO(y2, -fo, N)
        y2, _ = o.remove_IFO(y2, N)
    return o.OFDM_demodulator(y2.reshape((N + Tg, S), order="F"), Tg), int(tg), ok


# The error formula on the oracle: clean frames of the geometry above at Time_Delay 0, 5, 40, 200 with TgPosition forced so that
# phi_s + 1 runs over -T_guard + 2 .. 0 (the window inside the guard interval, no sample of the next symbol).  The largest |e| the
# oracle itself shows, measured by tests/test_fine_restatement_host.py (which prints it), and the bound the test holds the formula
# to: 10 x that.  The bound is asserted where the formula can hold: the angle of fine_sync.m:14 is unambiguous for |tau Nfft| <
# Nfft / (2 deltak) = 21.33 samples (deltak 6), so the asserted windows are those less than 21.33 samples early (3.6e-15 there:
# the rounding of a mean of exact angles).  An earlier window of 22 .. 30 samples reads Nfft / deltak = 42.67 samples late -- over
# the whole set the largest |e| is that alias, 42.67, and 10 x it would bound nothing --: there the test holds e + Nfft / deltak
# to 10 x what the oracle shows for it (7.1e-15).  Windows where the T4 mask leaves tau = mean([]) = NaN are recorded only.
ORACLE_E_MAX_IN_RANGE, ORACLE_E_MAX_ALIASED = 3.6e-15, 7.2e-15
E_BOUND, E_BOUND_ALIASED = 10 * ORACLE_E_MAX_IN_RANGE, 10 * ORACLE_E_MAX_ALIASED


# ---- the check orders: (refusal id, what breaks a good call for it, message)
def good_rx(f64):
    return dict(SHAPE, plan=1, x=1, f64=f64, f64_flag=f64, n_frames=3, variant=1, out=1)


def good_study(f64):
    return dict(SHAPE, plan=1, f64=f64, f64_flag=f64, frame0=0, n_points=1, fpp=5, max_chunk=0, points=1, sto_mode=2, cfo_mode=0,
                reg=REGISTER, h=3, taps="none", power=1.0, variant=1, td=1, fd=0, bins_n=64, bins_lo=-4.0, bins_hi=4.0, out=1)


def capture_order(what):
    return [
        ("variant", dict(variant=2), f"{what}: variant must be 0 (T5/fine_sync.m) or 1 (T4/fine_sync.m) (2)"),
        ("few_pilots", dict(np=1), f"{what}: fine_sync needs at least two pilot carriers (1)"),
        ("long", dict(np=1 << 16, n_symb=1 << 15), f"{what}: Np * N_symb must be below 2^31 (2147483648)"),
    ]


def rx_order(f64):
    what = "rx_fine"
    return ([("args", dict(x=0), f"{what}: bad arguments")] + sc.plan_order(what, f64) +
            [("frames", dict(n_frames=1 << 31), f"{what}: n_frames must be 0 .. 2^31 - 1 (2147483648)")] + capture_order(what) +
            [("output", dict(out=0), f"{what}: no output is given")])


def study_order(f64):
    what = "fine_study"
    return ([("args", dict(max_chunk=65536), f"{what}: bad arguments"),
             ("points_missing", dict(points=0), f"{what}: snr_db / seeds missing"),
             ("points_many", dict(n_points=1 << 31), f"{what}: too many points")] + sc.plan_order(what, f64) +
            [("stream", dict(frame0=(1 << 32) - 5), f"{what}: frame index outside the 32-bit stream range"),
             ("modes", dict(sto_mode=3), f"{what}: sto_mode / cfo_mode must be 0, 1 or 2"),
             ("register", dict(reg="100101010000002"), f"{what}: register entries must be 0 or 1"),
             ("both", dict(taps="0,3"), f"{what}: give h (one channel for every frame) or taps (a channel per frame), not both")] +
            capture_order(what)[:2] +
            [("sync", dict(td=0, fd=0), f"{what}: time_desync and freq_desync are both off: the receiver runs no fine_sync, there is "
                                        "nothing to study"),
             ("route", dict(n_symb=1),f"{what}: rx_chain_task4: frame shorter than T_guard + Nfft, or T_guard outside 1..1024"),
             ("bins", dict(bins_n=0), f"{what}: bins must have n >= 1 and finite lo < hi (0, -4, 4)"),
             ("output", dict(out=0), f"{what}: no output is given")])


def broken_from(good, order, i):
    return sc.broken_from(good, order, i)


# ---- the chunk rule and the launch shape
def t4_frame_bytes(shape, f64):
    """The receiver's arena per frame as the Task-4 sweep budgets it (t4_route.hpp)."""
    cs = 16 if f64 else 8
    n, s = shape["nfft"], shape["n_symb"]
    ln = (n + shape["t_guard"]) * s
    return cs * (ln + n * s + shape["np"] * s + 2 * n + shape["np"] + shape["n_carrier"]) + 128 + 4 * shape["frame_words"]


def row_bytes(shape, variant):
    """One row of L doubles, L bytes of mask and 64 bytes of scalars."""
    return 9 * fine_len(shape["np"], shape["n_symb"], variant) + 64


def chunk_model(shape, f64, scr, imp, fade_taps, fpp, cap, variant):
    per = sc.frame_bytes(shape, f64, scr, imp, fade_taps) + t4_frame_bytes(shape, f64) + row_bytes(shape, variant)
    ch = cap if cap > 0 else max(1, BUDGET // per)
    return max(1, min(ch, fpp, 65535))


def pass_model(shape, variant, frames):
    """(threads, grid, lds, trips, acc_threads, acc_grid, acc_lds)"""
    L = fine_len(shape["np"], shape["n_symb"], variant)
    return (256, frames, 88, -(-L // (THREADS * U)), 256, -(-L // 64) + 1, 64 * 64 * 8)
