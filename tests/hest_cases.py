"""Cases of the channel-estimate capture's call plan (csrc/hest_plan.hpp), shared by tests/test_hest_plan_host.py (the header, on the
CPU, through tests/host/hest_plan_main.cpp) and tests/test_gpu_hest_study.py (the same refusals through rx_hest and
RxPlan.channel_study, and the numpy twins of the study's sums).  TEST INFRASTRUCTURE: a hand-written model of the header, nothing
here is read from it."""
import numpy as np

from fine_cases import t4_frame_bytes
from sync_cases import CHANNEL as _SYNC_CHANNEL, LDS_LIMIT, REGISTER, SHAPE, broken_from, frame_bytes  # noqa: F401

BUDGET = 2 * (2 << 30)                                          # the Task-4 sweep's: the workspace and the arena together
MAX_BINS = 4096
BIN_BELOW, BIN_ABOVE, BIN_NAN = -1, -2, -3


def good_rx(f64):
    """An ofdm_rx_hest call every check accepts: 3 frames, both synchroniser flags on."""
    return dict(SHAPE, plan=1, rx=1, f64=f64, f64_flag=f64, n_frames=3, time_desync=1, freq_desync=1, out=1)


def good_study(f64):
    """An ofdm_hest_study call every check accepts: 1 point of 5 frames, a 3-tap h, both impairments drawn, scrambled."""
    return dict(SHAPE, plan=1, f64=f64, f64_flag=f64, frame0=0, n_points=1, fpp=5, max_chunk=0, points=1, sto_mode=2, cfo_mode=2,
                reg=REGISTER, h=3, taps="none", power=1.0, time_desync=1, freq_desync=1, bins_n=60, bins_lo=-50.0, bins_hi=10.0, out=1)


# the capture checks, the last of both entries, in their order: (refusal id, what breaks a good call for it, message behind "what: ")
def capture_order(study):
    return ([("time_desync", dict(time_desync=2), "time_desync must be 0 or 1 (2)"),
             ("freq_desync", dict(freq_desync=2), "freq_desync must be 0 or 1 (2)"),
             ("pilots", dict(np=1), "estimate_channel needs at least two pilot carriers (1)"),
             ("route", dict(n_symb=1), "rx_chain_task4: frame shorter than T_guard + Nfft, or T_guard outside 1..1024")] +
            ([("bins", dict(bins_n=0), "bins must have n 1 .. 4096 and finite lo < hi (0, -50, 10)")] if study else []) +
            [("output", dict(out=0), "no output is given")])


def plan_order(what, f64):
    return [
        ("device", dict(ctx_device=1), "RX plan belongs to device 0, the context is on device 1"),
        ("precision", dict(f64_flag=1 - f64), f"{what}: precision flag differs from the plan's"),
        ("no_data", dict(nd=0), f"{what}: the plan has no data carriers"),
        ("pilots", dict(pilots_in_band=0), f"{what}: pilots outside 1..N_carrier are not supported"),
        ("nfft", dict(nfft=100), f"{what}: unsupported Nfft 100 / T_guard 32"),
    ]


def rx_order(f64):
    what = "rx_hest"
    return ([("args", dict(rx=0), f"{what}: bad arguments")] + plan_order(what, f64) +
            [("frames", dict(n_frames=1 << 31), f"{what}: n_frames must be 0 .. 2^31 - 1 (2147483648)")] +
            [(rid, brk, f"{what}: {msg}") for rid, brk, msg in capture_order(False)])


def study_order(f64):
    what = "hest_study"
    return ([("args", dict(max_chunk=-1), f"{what}: bad arguments"),
             ("points_missing", dict(points=0), f"{what}: snr_db / seeds missing"),
             ("points_many", dict(n_points=1 << 31), f"{what}: too many points")] + plan_order(what, f64) +
            [("stream", dict(frame0=(1 << 32) - 5), f"{what}: frame index outside the 32-bit stream range"),
             ("modes", dict(sto_mode=3), f"{what}: sto_mode / cfo_mode must be 0, 1 or 2"),
             ("register", dict(reg="100101010000002"), f"{what}: register entries must be 0 or 1"),
             ("both", dict(taps="0,3"), f"{what}: give h (one channel for every frame) or taps (a channel per frame), not both")] +
            [(rid, brk, f"{what}: {msg}") for rid, brk, msg in capture_order(True)])


# the channel refusals of the study, behind "both" and in front of the capture
CHANNEL = [(brk, rid, msg.replace("sync_study", "hest_study")) for brk, rid, msg in _SYNC_CHANNEL]


def row_bytes(shape):
    """Per carrier four doubles and a byte, per pilot two doubles and a byte, and the frame's scalars (four of 8 bytes, two of 4)."""
    return 33 * shape["n_carrier"] + 17 * shape["np"] + 40


def chunk_model(shape, f64, scr, imp, fade_taps, fpp, cap):
    per = frame_bytes(shape, f64, scr, imp, fade_taps) + t4_frame_bytes(shape, f64) + row_bytes(shape)
    ch = cap if cap > 0 else max(1, BUDGET // per)
    return max(1, min(ch, fpp, 65535))


def lanes(n_carrier):
    """The lanes of a frame: the next power of two of N_carrier, at least 16 and at most 256."""
    l = 16
    while l < 256 and l < n_carrier:
        l *= 2
    return l


def pass_model(shape, frames):
    """(threads, lanes, frames_per_wg, lds, grid, acc_threads, acc_grid, acc_grid_pilots, acc_lds): 256 threads over whole frames; the
    taps of at most 16 frames, 64 complex doubles each, in LDS; 64 columns per accumulating workgroup with a tile of 64 rows of a
    double and a byte."""
    l = lanes(shape["n_carrier"])
    per = 256 // l
    return (256, l, per, 16 * 16 * 64, -(-frames // per), 256, -(-shape["n_carrier"] // 64), -(-shape["np"] // 64), 9 * 64 * 64)


# ---- the twins of the header's functions
def thresholds(n, lo, hi, n_carrier):
    """The dB edges lo + i (hi - lo) / n (the last one hi) -- only their order and ends are modelled here; the table itself is the
    stand-alone program's (and the library's): pow is not required to round the same way everywhere."""
    return [lo + (hi - lo) * i / n if i < n else hi for i in range(n + 1)]


def hist_bin(v, thr):
    """The bin of v on the table thr[0 .. n]: NaN, below thr[0], at or above thr[n], else the last b with thr[b] <= v."""
    n = len(thr) - 1
    if v != v:
        return BIN_NAN
    if v < thr[0]:
        return BIN_BELOW
    if not v < thr[n]:
        return BIN_ABOVE
    return int(np.searchsorted(np.asarray(thr, np.float64), np.float64(v), side="right")) - 1


def cabs(z):
    """sqrt(re re + im im) in float64: two rounded products, a rounded sum, a root."""
    z = np.asarray(z)
    re, im = z.real.astype(np.float64), z.imag.astype(np.float64)
    return np.sqrt(re * re + im * im)


def true_channel(delays, amps, n_carrier, nfft):
    """H_f(k) = sum_t a_{f,t} e^{-2 pi i d_t k / Nfft} on k = 0 .. n_carrier - 1, float64; amps [frames, taps]."""
    k = np.arange(n_carrier, dtype=np.float64)
    amps = np.atleast_2d(np.asarray(amps, np.complex128))
    ph = np.exp(-2j * np.pi * np.outer(np.asarray(delays, np.float64), k) / nfft)
    return amps @ ph


def ordered_sum(rows, bad):
    """((0 + v_0) + v_1) + .. per column in frame order, the rows whose `bad` is set left out; (sums, dropped)."""
    rows, bad = np.asarray(rows, np.float64), np.asarray(bad, bool)
    acc = np.zeros(rows.shape[1], np.float64)
    for f in range(rows.shape[0]):
        acc = np.where(bad[f], acc, acc + np.where(bad[f], 0.0, rows[f]))
    return acc, bad.sum(axis=0).astype(np.int64)
