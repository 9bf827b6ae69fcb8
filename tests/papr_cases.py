"""Cases of the PAPR study's call plan (csrc/papr_plan.hpp), shared by tests/test_papr_plan_host.py (the header, on the CPU,
through tests/host/papr_plan_main.cpp) and tests/test_gpu_papr_study.py (the same refusals through RxPlan.papr_study).  TEST
INFRASTRUCTURE: a hand-written model of the header, nothing here is read from it."""

REGISTER = "100101010000000"                                   # T2/Main_model_Task_2.m:36

# frames.config_small(): Nfft 256, T_guard 32, 5 symbols, 64 carriers, comb 4, 16QAM
SHAPE = dict(nfft=256, t_guard=32, n_symb=5, n_carrier=64, np=16, nd=48, bps=4, frame_words=30, pilots_in_band=1, device=0,
             ctx_device=0)
FRAME_SAMPLES = (256 + 32) * 5


def good_call(f64):
    """A call every check accepts: 2 signals of 3 frames (4320 samples each), window 256, the default grid."""
    return dict(SHAPE, plan=1, f64=f64, out=1, f64_flag=f64, frame0=0, n_signals=2, fps=3, reg=REGISTER, window=256, n_bins=600,
                lo=0, hi=30, max_chunk=0)


# the checks in the order papr_prelude makes them: (refusal id, what breaks the good call for it, its message)
def order(f64):
    return [
        ("args", dict(out=0), "papr_study: bad arguments"),
        ("device", dict(ctx_device=1), "RX plan belongs to device 0, the context is on device 1"),
        ("precision", dict(f64_flag=1 - f64), "papr_study: precision flag differs from the plan's"),
        ("no_data", dict(nd=0), "papr_study: the plan has no data carriers"),
        ("pilots", dict(pilots_in_band=0), "papr_study: pilots outside 1..N_carrier are not supported"),
        ("nfft", dict(nfft=100), "papr_study: unsupported Nfft 100 / T_guard 32"),
        ("stream", dict(frame0=1 << 32), "papr_study: frame index outside the 32-bit stream range"),
        ("signals", dict(n_signals=-1), "papr_study: n_signals must be >= 0 (-1)"),
        ("frames", dict(fps=0), "papr_study: frames_per_signal must be >= 1 (0)"),
        ("stream", dict(n_signals=1 << 31), "papr_study: frame index outside the 32-bit stream range"),
        ("bins", dict(n_bins=4097), "papr_study: n_bins must be 1 .. 4096 (4097)"),
        ("range", dict(lo=30, hi=30), "papr_study: lo_db and hi_db must be finite with lo_db < hi_db"),
        ("window", dict(window=768), "papr_study: window must be a power of two, 256 .. 8192 (768)"),
        ("window_long", dict(window=8192), "papr_study: window 8192 exceeds the signal of 4320 samples"),
        ("register", dict(reg="100101010000002"), "papr_study: register entries must be 0 or 1"),
        ("chunk_cap", dict(max_chunk=-1), "papr_study: max_frames_per_chunk must be >= 0"),
    ]


def broken_from(f64, i):
    """The good call broken for every check from position i on (where two breaks set one key, the earlier check's wins)."""
    call = good_call(f64)
    for _, brk, _ in reversed(order(f64)[i:]):
        call.update(brk)
    return call


# single breaks, each with the message the library must give: (what is broken, message)
SINGLE = [
    (dict(n_bins=0), "papr_study: n_bins must be 1 .. 4096 (0)"),
    (dict(n_bins=4097), "papr_study: n_bins must be 1 .. 4096 (4097)"),
    (dict(lo=3, hi=3), "papr_study: lo_db and hi_db must be finite with lo_db < hi_db"),
    (dict(lo=5, hi=-5), "papr_study: lo_db and hi_db must be finite with lo_db < hi_db"),
    (dict(lo="-inf", hi=5), "papr_study: lo_db and hi_db must be finite with lo_db < hi_db"),
    (dict(lo=0, hi="nan"), "papr_study: lo_db and hi_db must be finite with lo_db < hi_db"),
    (dict(window=768), "papr_study: window must be a power of two, 256 .. 8192 (768)"),
    (dict(window=128), "papr_study: window must be a power of two, 256 .. 8192 (128)"),
    (dict(window=16384), "papr_study: window must be a power of two, 256 .. 8192 (16384)"),
    (dict(window=0), "papr_study: window must be a power of two, 256 .. 8192 (0)"),
    (dict(window=8192), "papr_study: window 8192 exceeds the signal of 4320 samples"),
    (dict(frame0=(1 << 32) - 6), "papr_study: frame index outside the 32-bit stream range"),
    (dict(n_signals=1 << 62, fps=1 << 30), "papr_study: frame index outside the 32-bit stream range"),
]

WINDOWS = (256, 512, 1024, 2048, 4096, 8192)
LDS_LIMIT = 160 << 10
STATIC_LDS = 256


def pass_model(window, n_bins, samples, signals):
    """(threads, per_thread, two_phase, scan_bytes, lds, windows, grid_x, grid_y) of the histogram pass."""
    threads = {256: 128, 512: 256, 1024: 256, 2048: 512, 4096: 1024, 8192: 1024}[window]
    two = int(window == 8192)
    scan = 8 * (window + window // 32 + 1) * (2 if two else 4)
    windows = samples - window + 1
    return (threads, 2 * window // threads, two, scan, scan + 4 * (n_bins + 3), windows, -(-windows // window), signals)


def bin_model(v, lo, hi, n):
    """The bin of v in exact arithmetic where it is unambiguous (the cases of the host test avoid bin edges that are not
    representable): 0 .. n - 1, n = below, n + 1 = at or above hi, n + 2 = NaN."""
    import math
    from fractions import Fraction
    if math.isnan(v):
        return n + 2
    if v < lo:
        return n
    if v >= hi:
        return n + 1
    return min(n - 1, int((Fraction(v) - Fraction(lo)) * n // (Fraction(hi) - Fraction(lo))))
