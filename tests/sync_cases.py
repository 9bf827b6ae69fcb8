"""Cases of the coarse-sync capture's call plan (csrc/sync_plan.hpp), shared by tests/test_sync_plan_host.py (the header, on the
CPU, through tests/host/sync_plan_main.cpp) and tests/test_gpu_sync_study.py (the same refusals through rx_acf and
RxPlan.sync_study, and the twins of the header's two frame functions).  TEST INFRASTRUCTURE: a hand-written model of the header,
nothing here is read from it."""
import numpy as np

REGISTER = "100101010000000"                                   # T5/Main_model_Task_5.m:55

# frames.config_small(): Nfft 256, T_guard 32, 5 symbols, 64 carriers, comb 4, 16QAM
SHAPE = dict(nfft=256, t_guard=32, n_symb=5, n_carrier=64, np=16, nd=48, bps=4, frame_words=30, pilots_in_band=1, device=0,
             ctx_device=0)
STRIDE = 256 + 32
FRAME_SAMPLES = STRIDE * 5
BUDGET = 2 << 30
MAXW = 1024
LDS_LIMIT = 150 << 10


def n_out(shape, width):
    """numel(AutoCorr) = length(RxSignal) - WidthWindow - Nfft (AutoCorrFunction.m:3)."""
    return (shape["nfft"] + shape["t_guard"]) * shape["n_symb"] - width - shape["nfft"]


def good_rx(f64):
    """An ofdm_rx_acf call every check accepts: 3 frames, the window of T4/Main_model_Task_4.m:278."""
    return dict(SHAPE, plan=1, rx=1, f64=f64, f64_flag=f64, n_frames=3, width=32, out=1)


def good_study(f64):
    """An ofdm_sync_study call every check accepts: 1 point of 5 frames, a 3-tap h, both impairments drawn, scrambled."""
    return dict(SHAPE, plan=1, f64=f64, f64_flag=f64, frame0=0, n_points=1, fpp=5, max_chunk=0, points=1, sto_mode=2, cfo_mode=2,
                reg=REGISTER, h=3, taps="none", power=1.0, width=32, out=1)


# the capture checks, the last of both entries, in their order: (refusal id, what breaks a good call for it, message behind "what: ")
def capture_order():
    return [
        ("width", dict(width=0), "WidthWindow must be 1 .. 1024 (0)"),
        ("short", dict(n_symb=1), "a frame of 288 samples is shorter than WidthWindow + Nfft + 1 (32 + 256 + 1)"),
        ("output", dict(out=0), "no output is given"),
    ]


def plan_order(what, f64):
    return [
        ("device", dict(ctx_device=1), "RX plan belongs to device 0, the context is on device 1"),
        ("precision", dict(f64_flag=1 - f64), f"{what}: precision flag differs from the plan's"),
        ("no_data", dict(nd=0), f"{what}: the plan has no data carriers"),
        ("pilots", dict(pilots_in_band=0), f"{what}: pilots outside 1..N_carrier are not supported"),
        ("nfft", dict(nfft=100), f"{what}: unsupported Nfft 100 / T_guard 32"),
    ]


def rx_order(f64):
    what = "rx_acf"
    return ([("args", dict(rx=0), f"{what}: bad arguments")] + plan_order(what, f64) +
            [("frames", dict(n_frames=1 << 31), f"{what}: n_frames must be 0 .. 2^31 - 1 (2147483648)")] +
            [(rid, brk, f"{what}: {msg}") for rid, brk, msg in capture_order()])


def study_order(f64):
    what = "sync_study"
    return ([("args", dict(max_chunk=-1), f"{what}: bad arguments"),
             ("points_missing", dict(points=0), f"{what}: snr_db / seeds missing"),
             ("points_many", dict(n_points=1 << 31), f"{what}: too many points")] + plan_order(what, f64) +
            [("stream", dict(frame0=(1 << 32) - 5), f"{what}: frame index outside the 32-bit stream range"),
             ("modes", dict(sto_mode=3), f"{what}: sto_mode / cfo_mode must be 0, 1 or 2"),
             ("register", dict(reg="100101010000002"), f"{what}: register entries must be 0 or 1"),
             ("both", dict(taps="0,3"), f"{what}: give h (one channel for every frame) or taps (a channel per frame), not both")] +
            [(rid, brk, f"{what}: {msg}") for rid, brk, msg in capture_order()])


def broken_from(good, order, i):
    """The good call broken for every check from position i on (where two breaks set one key, the earlier check's wins)."""
    call = dict(good)
    for _, brk, _ in reversed(order[i:]):
        call.update(brk)
    return call


# the channel refusals of the study, behind "both" and in front of the capture: (what is broken, id, message)
CHANNEL = [
    (dict(h="bad"), "channel", "tx_frames_fused: bad channel"),
    (dict(h=65), "tap_count", "tx_frames_fused: 65 nonzero channel taps (at most 64)"),
    (dict(h="none", taps="0,4097"), "fade_delay", "sync_study: tap delay 4097 outside 0 .. 4096"),
    (dict(h="none", taps="0,3,3"), "fade_twice", "sync_study: tap delay 3 given twice"),
    (dict(h="none", taps="0,3", power=0.0), "fade_power", "sync_study: tap powers must be positive and finite"),
]


def frame_bytes(shape, f64, scr, imp, fade_taps):
    """The generator's workspace per frame with the RX region: TX, partials, (two bit regions), RX, reference words, (two draws),
    (the amplitudes)."""
    cs = 16 if f64 else 8
    fs = (shape["nfft"] + shape["t_guard"]) * shape["n_symb"]
    bits = shape["nd"] * shape["n_symb"] * shape["bps"]
    return cs * fs + 8 * shape["n_symb"] + (2 * bits if scr else 0) + cs * fs + 4 * shape["frame_words"] + (16 if imp else 0) + \
        16 * fade_taps


def row_bytes(shape, width):
    """One row of n_out doubles and the frame's scalars (three of 8 bytes, the status padded to 8)."""
    return 8 * n_out(shape, width) + 32


def chunk_model(shape, f64, scr, imp, fade_taps, fpp, cap, width):
    ch = cap if cap > 0 else max(1, BUDGET // (frame_bytes(shape, f64, scr, imp, fade_taps) + row_bytes(shape, width)))
    return max(1, min(ch, fpp, 65535))


def pass_model(shape, f64, width, frames):
    """(threads, grid, lds, acc_threads, acc_grid): the prefix table of 1024 + width + 1 entries of four sums and a tile of 1024
    complex values, both in the plan's precision; 64 lags per accumulating workgroup and one more for the wrapped errors."""
    lds = (32 if f64 else 16) * (1024 + width + 1) + (16 if f64 else 8) * 1024
    return (256, frames, lds, 256, -(-n_out(shape, width) // 64) + 1)


# ---- the twins of the header's two frame functions
def phase_bin(tg_position, sto, stride):
    """(TgPosition - 1 + sto) mod (Nfft + T_guard), in 0 .. stride - 1 for either sign of sto (Python's % is already that)."""
    return (int(tg_position) - 1 + int(sto)) % int(stride)


def ffo_err(freq_offset, cfo):
    """ffo_true = cfo - rint(cfo); d = FreqOffset - ffo_true; e = d - rint(d): float64, ties to even (np.rint)."""
    fo, cfo = np.float64(freq_offset), np.float64(cfo)
    ffo_true = cfo - np.rint(cfo)
    d = fo - ffo_true
    return d - np.rint(d)
