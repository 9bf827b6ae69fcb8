"""Cases of the payload transport's call plan (csrc/payload_plan.hpp), shared by tests/test_payload_plan_host.py (the header, on the
CPU, through tests/host/payload_plan_main.cpp) and tests/test_gpu_payload.py (the numpy twin of the cut and the join, and the same
refusals through RxPlan.transport).  TEST INFRASTRUCTURE: a hand-written model of the header, nothing here is read from it."""
import numpy as np

from error_cases import DESCR, SHAPE, unpack  # noqa: F401
from fine_cases import t4_frame_bytes
from sync_cases import REGISTER, broken_from, frame_bytes  # noqa: F401

BUDGET = 2 << 30
STREAMS = 1 << 32
THREADS, MAX_GRID = 256, 4096


# ---- the numpy twin of the cut and the join
def n_frames(n_bits, frame_bits):
    return -(-n_bits // frame_bits)


def position(n_bits, frame_bits, first_frame, period, g):
    """Frame g of a call -> (payload frame, repeat, first stream bit or -1, how many of its bits are payload)."""
    repeat, k = (0, g) if period is None else divmod(g, period)
    frame = first_frame + k
    bit0 = frame * frame_bits
    if bit0 >= n_bits:
        return frame, repeat, -1, 0
    return frame, repeat, bit0, min(frame_bits, n_bits - bit0)


def cut(bits, frame_bits, first_frame, count):
    """A 0 / 1 stream -> [count, frame_bits]: frame f holds the stream bits (first_frame + f) frame_bits .., zeros beyond its end."""
    bits = np.asarray(bits, np.uint8).ravel()
    out = np.zeros((count, frame_bits), np.uint8)
    for f in range(count):
        part = bits[(first_frame + f) * frame_bits:(first_frame + f + 1) * frame_bits]
        out[f, :part.size] = part
    return out


def join(frames, n_bits):
    """[F, frame_bits] decisions -> the stream of n_bits, and its packed bytes with the spare bits of the last byte 0."""
    stream = np.asarray(frames, np.uint8).reshape(-1)[:n_bits]
    return stream, np.packbits(stream)


def frame_bytes_payload(shape, f64, scr, imp, fade_taps):
    """The generator's workspace per frame with the RX region and the payload's byte-per-bit region, present without a Scrambler too."""
    bits = shape["nd"] * shape["n_symb"] * shape["bps"]
    return frame_bytes(shape, f64, scr, imp, fade_taps) + (0 if scr else bits)


def chunk_model(shape, f64, receiver, scr, fade_taps, frames, cap):
    """As the matching sweep budgets its chunk, with the chunk's decisions beside it; receiver 4 always has the draw regions."""
    per = frame_bytes_payload(shape, f64, scr, receiver == 4, fade_taps) + 4 * shape["frame_words"]
    budget = BUDGET
    if receiver == 4:
        per += t4_frame_bytes(shape, f64)
        budget = 2 * BUDGET
    ch = cap if cap > 0 else max(1, budget // per)
    return max(1, min(ch, frames, 65535))


def grid(items):
    return max(1, min(-(-items // THREADS), MAX_GRID))


# ---- the refusals, in their order: (refusal id, what breaks a good call for it, message)
def good_transport(receiver, f64):
    """An ofdm_payload_transport call every check accepts: 1 point, 2 repeats of 2 * 960 + 13 bits, a 3-tap h, scrambled, the plan
    descrambling; receiver 4 with both impairments drawn and every flag on."""
    t4 = receiver == 4
    return dict(SHAPE, descr=DESCR, plan=1, f64=f64, f64_flag=f64, receiver=receiver, payload=1, n_bits=2 * 960 + 13, repeats=2,
                frame0=0, n_points=1, max_chunk=0, points=1, sto_mode=2 if t4 else 0, cfo_mode=2 if t4 else 0,
                time_desync=int(t4), freq_desync=int(t4), mp_desync=1, reg=REGISTER, h=3, taps="none", power=1.0, out=1)


def _plan_order(what, f64):
    # (the stream range of the sweep's plan check cannot fail behind the transport's own frames check)
    return [("device", dict(ctx_device=1), "RX plan belongs to device 0, the context is on device 1"),
            ("precision", dict(f64_flag=1 - f64), f"{what}: precision flag differs from the plan's"),
            ("pilots", dict(pilots_in_band=0), f"{what}: pilots outside 1..N_carrier are not supported"),
            ("nfft", dict(nfft=100), f"{what}: unsupported Nfft 100 / T_guard 32")]


_DESCR_ORDER = [("register", dict(reg="100101010000020"), "register entries must be 0 or 1"),
                ("descr_needed", dict(descr=0), "with the Scrambler on the plan needs a DeScrambler with the same register "
                                                "(ofdm_rx_plan_set_descrambler)")]


def transport_order(receiver, f64):
    t = "transport"
    own = [("receiver", dict(receiver=3), f"{t}: receiver must be 4 (rx_chain_task4) or 5 (rx_chain_task5) (3)"),
           ("args", dict(payload=0), f"{t}: bad arguments"),
           ("no_data", dict(nd=0), f"{t}: the plan has no data carriers"),
           ("bits", dict(n_bits=0), f"{t}: the payload must have at least one bit (0)"),
           ("repeats", dict(repeats=0), f"{t}: repeats must be at least 1 (0)"),
           # (asked with every later check broken too: the frame of 2^31 + 64 bits holds the whole payload, F = 1)
           ("frames", dict(frame0=STREAMS - 2), f"{t}: 1 frames x 2 repeats from frame {STREAMS - 2} leave the 32-bit stream range"),
           ("channel", dict(taps="0,3"), f"{t}: give h (one channel for every frame) or taps (a channel per frame), not both")]
    if receiver == 5:
        sweep = ([("task5_imp", dict(sto_mode=1), f"{t}: receiver 5 runs as ber_sweep_task5 does: no sto_mode / cfo_mode, "
                                                  "time_desync and freq_desync 0, mp_desync 1"),
                  ("args", dict(max_chunk=-1), f"{t}: bad arguments"),
                  ("points_missing", dict(points=0), f"{t}: snr_db / seeds missing"),
                  ("points_many", dict(n_points=1 << 31), f"{t}: too many points")] + _plan_order(t, f64) +
                 [("mmse_points", dict(mmse=1, n_points=2), f"{t}: an MMSE-mode plan is built for one SNR (n_points must be 1)")] +
                 [(rid, brk, f"{t}: {msg}") for rid, brk, msg in _DESCR_ORDER] +
                 [("channel", dict(h="bad"), "tx_frames_fused: bad channel")])
    else:
        t4 = "ber_sweep_task4"                                       # the Task-4 sweep names itself behind its channel check
        sweep = ([("args", dict(n_points=-1), f"{t}: bad arguments"),
                  ("channel", dict(h="bad"), "tx_frames_fused: bad channel"),
                  ("chunk_cap", dict(max_chunk=65536), f"{t4}: max_frames_per_chunk must be 0..65535 (the limit of rx_chain_task4)"),
                  ("points_missing", dict(points=0), f"{t4}: snr_db / seeds missing"),
                  ("points_many", dict(n_points=1 << 31), f"{t4}: too many points")] + _plan_order(t4, f64) +
                 [("modes", dict(sto_mode=3), f"{t4}: sto_mode / cfo_mode must be 0, 1 or 2")] +
                 [(rid, brk, f"{t4}: {msg}") for rid, brk, msg in _DESCR_ORDER])
    last = [("frame_bits", dict(n_symb=11184811), f"{t}: a frame must have 1 .. 2^31 - 1 bits (2147483712)"),
            ("output", dict(out=0), f"{t}: no output is wanted")]
    return own + sweep + last


def good_generator(f64):
    return dict(SHAPE, plan=1, f64=f64, f64_flag=f64, payload=1, n_bits=2 * 960 + 13, first_frame=0, frame0=0, n_frames=3, rx=1,
                sto_mode=0, cfo_mode=0, sc_ref=1, reg=REGISTER, h=3, taps="none", power=1.0)


def generator_order(f64):
    t = "tx_frames_payload"
    return ([("bits", dict(n_bits=0), f"{t}: the payload must have at least one bit (0)"),
             ("first_frame", dict(first_frame=STREAMS), f"{t}: first_frame must be 0 .. 2^32 - 1 ({STREAMS})"),
             ("channel", dict(taps="0,3"), f"{t}: give h (one channel for every frame) or taps (a channel per frame), not both"),
             ("args", dict(rx=0), f"{t}: bad arguments")] +
            [("device", dict(ctx_device=1), "RX plan belongs to device 0, the context is on device 1"),
             ("precision", dict(f64_flag=1 - f64), f"{t}: precision flag differs from the plan's"),
             ("no_data", dict(nd=0), f"{t}: the plan has no data carriers"),
             ("pilots", dict(pilots_in_band=0), f"{t}: pilots outside 1..N_carrier are not supported"),
             ("nfft", dict(nfft=100), f"{t}: unsupported Nfft 100 / T_guard 32"),
             ("stream", dict(frame0=STREAMS - 3), f"{t}: frame index outside the 32-bit stream range"),
             ("modes", dict(cfo_mode=3), f"{t}: sto_mode / cfo_mode must be 0, 1 or 2"),
             ("sc_ref", dict(reg="none"), f"{t}: sc_ref_bits_out needs the Scrambler register"),
             ("channel", dict(h="bad"), "tx_frames_fused: bad channel"),
             ("frame_bits", dict(n_symb=11184811), f"{t}: a frame must have 1 .. 2^31 - 1 bits (2147483712)")])
