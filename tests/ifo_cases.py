"""Cases of the integer-CFO capture's call plan (csrc/ifo_plan.hpp), shared by tests/test_ifo_plan_host.py (the header, on the CPU,
through tests/host/ifo_plan_main.cpp) and tests/test_gpu_ifo_study.py (the same refusals through rx_ifo and RxPlan.ifo_study, and
the twins of the header's two frame functions).  TEST INFRASTRUCTURE: a hand-written model of the header, nothing here is read
from it."""
import numpy as np

from sync_cases import BUDGET, CHANNEL as _SYNC_CHANNEL, LDS_LIMIT, REGISTER, SHAPE, broken_from, frame_bytes  # noqa: F401

MAX_SPAN = 4096
ERR_BELOW, ERR_ABOVE = -1, -2


def good_rx(f64):
    """An ofdm_rx_ifo call every check accepts: 3 frames, the receiver's stage."""
    return dict(SHAPE, plan=1, rx=1, f64=f64, f64_flag=f64, n_frames=3, stage=1, time_desync=1, out=1)


def good_study(f64):
    """An ofdm_ifo_study call every check accepts: 1 point of 5 frames, a 3-tap h, both impairments drawn, scrambled."""
    return dict(SHAPE, plan=1, f64=f64, f64_flag=f64, frame0=0, n_points=1, fpp=5, max_chunk=0, points=1, sto_mode=2, cfo_mode=2,
                reg=REGISTER, h=3, taps="none", power=1.0, stage=1, time_desync=1, err_span=32, out=1)


# the capture checks, the last of both entries, in their order: (refusal id, what breaks a good call for it, message behind "what: ")
def capture_order(study):
    return ([("stage", dict(stage=2), "stage must be 0 (the received frame) or 1 (the receiver's stream) (2)"),
             ("time_desync", dict(time_desync=2), "time_desync must be 0 or 1 (2)"),
             ("short", dict(n_symb=1), "rx_signal(Nfft+1:2*Nfft) exceeds the frame"),
             ("route", dict(np=1), "rx_chain_task4: fine_sync needs at least two pilot carriers")] +
            ([("span", dict(err_span=0), "err_span must be 1 .. 4096 (0)")] if study else []) +
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
    what = "rx_ifo"
    return ([("args", dict(rx=0), f"{what}: bad arguments")] + plan_order(what, f64) +
            [("frames", dict(n_frames=1 << 31), f"{what}: n_frames must be 0 .. 2^31 - 1 (2147483648)")] +
            [(rid, brk, f"{what}: {msg}") for rid, brk, msg in capture_order(False)])


def study_order(f64):
    what = "ifo_study"
    return ([("args", dict(max_chunk=-1), f"{what}: bad arguments"),
             ("points_missing", dict(points=0), f"{what}: snr_db / seeds missing"),
             ("points_many", dict(n_points=1 << 31), f"{what}: too many points")] + plan_order(what, f64) +
            [("stream", dict(frame0=(1 << 32) - 5), f"{what}: frame index outside the 32-bit stream range"),
             ("modes", dict(sto_mode=3), f"{what}: sto_mode / cfo_mode must be 0, 1 or 2"),
             ("register", dict(reg="100101010000002"), f"{what}: register entries must be 0 or 1"),
             ("both", dict(taps="0,3"), f"{what}: give h (one channel for every frame) or taps (a channel per frame), not both")] +
            [(rid, brk, f"{what}: {msg}") for rid, brk, msg in capture_order(True)])


# the channel refusals of the study, behind "both" and in front of the capture
CHANNEL = [(brk, rid, msg.replace("sync_study", "ifo_study")) for brk, rid, msg in _SYNC_CHANNEL]


def row_bytes(shape):
    """One row of Nfft doubles, Nfft bytes for the bins above the threshold, and the frame's scalars (three of 8 bytes, three of
    4, padded to 40)."""
    return 9 * shape["nfft"] + 40


def chunk_model(shape, f64, scr, imp, fade_taps, fpp, cap):
    ch = cap if cap > 0 else max(1, BUDGET // (frame_bytes(shape, f64, scr, imp, fade_taps) + row_bytes(shape)))
    return max(1, min(ch, fpp, 65535))


def pass_model(shape, f64, frames):
    """(threads, frames_per_wg, lds, grid, acc_threads, acc_grid, acc_lds): a transform of Nfft / 8 threads per frame in workgroups
    of at least 256; per transform Nfft + Nfft / 8 + 8 padded complex elements of LDS, and two 32-bit words for each of 16
    wavefronts; 64 bins per accumulating workgroup with a tile of 64 rows of doubles, and one more workgroup for the errors."""
    n = shape["nfft"]
    threads = max(256, n // 8)
    per = threads // (n // 8)
    lds = (16 if f64 else 8) * per * (n + n // 8 + 8) + 2 * 4 * 16
    return (threads, per, lds, -(-frames // per), 256, n // 64 + 1, 8 * 64 * 64)


# ---- the twins of the header's two frame functions
def err_bin(ifo, cfo, span):
    """IFO - rint(Freq_Shift) (float64, ties to even) as a bin 0 .. 2 span, or below / above."""
    d = np.float64(int(ifo)) - np.rint(np.float64(cfo))
    if d < -span:
        return ERR_BELOW
    if not d <= span:
        return ERR_ABOVE
    return int(d + span)


def cfo_total_err(freq_offset, ifo, cfo):
    """(FreqOffset + IFO) - Freq_Shift: two float64 additions in this order."""
    return (np.float64(freq_offset) + np.float64(int(ifo))) - np.float64(cfo)
