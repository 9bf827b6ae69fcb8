"""Cases of the error anatomy's call plan (csrc/error_plan.hpp), shared by tests/test_error_plan_host.py (the header, on the CPU,
through tests/host/error_plan_main.cpp), tests/test_gpu_error_profile.py and tests/test_gpu_error_study.py (the numpy twin of the
profile and the same refusals through bit_error_profile and RxPlan.error_study).  TEST INFRASTRUCTURE: a hand-written model of the
header, nothing here is read from it."""
import numpy as np

from fine_cases import t4_frame_bytes
from sync_cases import REGISTER, SHAPE as _SHAPE, broken_from, frame_bytes  # noqa: F401

SHAPE = dict(_SHAPE, mmse=0, descr=0)
DESCR = 0x80000000 | 0xA9                                       # the plan's DeScrambler for REGISTER: bit m - 1 = Register(m), m <= 14
BUDGET = 2 << 30
MAX_GAP_BINS = 1024
COUNTER_MAX = (1 << 32) - 1
THREADS, MAX_GRID, SCRATCH_WORDS, LDS_LIMIT = 256, 1024, 20, 64 << 10
BPS = (1, 2, 3, 4, 6, 8)                                        # BPSK, QPSK, 8PSK, 16QAM, 64QAM, 256QAM


# ---- the numpy twin of the profile
def unpack(packed, frame_bits):
    """[frames, frame_bytes] uint8, MSB first inside each byte -> [frames, frame_bits] 0 / 1."""
    return np.unpackbits(np.asarray(packed, np.uint8), axis=1)[:, :frame_bits]


def pack(bits, frame_bytes):
    """[frames, frame_bits] 0 / 1 -> [frames, frame_bytes] uint8, the padding zero."""
    out = np.zeros((bits.shape[0], frame_bytes), np.uint8)
    p = np.packbits(np.asarray(bits, np.uint8), axis=1)
    out[:, :p.shape[1]] = p
    return out


def profile(bits, ref, nd, n_symb, bps, gap_bins):
    """The tables of bit_error_profile from packed decisions and packed reference bits, [frames, frame_bytes] uint8 each."""
    frame_bits = nd * n_symb * bps
    wrong = unpack(bits, frame_bits) ^ unpack(ref, frame_bits)
    grid = wrong.reshape(-1, n_symb, nd, bps).astype(np.int64)
    frame_errors = wrong.sum(axis=1).astype(np.int64)
    gap_hist, above = np.zeros(gap_bins, np.int64), 0
    for row in wrong:
        gaps = np.diff(np.flatnonzero(row))
        gap_hist += np.bincount(gaps[gaps <= gap_bins] - 1, minlength=gap_bins)
        above += int((gaps > gap_bins).sum())
    return dict(errors=int(frame_errors.sum()), frames_in_error=int((frame_errors > 0).sum()), carrier_errors=grid.sum(axis=(0, 1, 3)),
                symbol_errors=grid.sum(axis=(0, 2, 3)), label_errors=grid.sum(axis=(0, 1, 2)), gap_hist=gap_hist, gap_above=above,
                frame_errors=frame_errors, map=grid.sum(axis=(0, 3)))


TABLES = ("errors", "frames_in_error", "carrier_errors", "symbol_errors", "label_errors", "gap_hist", "gap_above")


def assert_profile(got, want, point=None, frames=True, emap=True):
    """Every table of `got` (a result of bit_error_profile, or point `point` of a study's) equals the twin's, and the identities."""
    pick = (lambda a: np.asarray(a)) if point is None else (lambda a: np.asarray(a)[point])
    names = TABLES + (("frame_errors",) if frames else ()) + (("map",) if emap else ())
    for name in names:
        assert np.array_equal(pick(got[name]), np.asarray(want[name])), name
    errors, fie = int(pick(got["errors"])), int(pick(got["frames_in_error"]))
    for name in ("carrier_errors", "symbol_errors", "label_errors"):
        assert int(pick(got[name]).sum()) == errors, name
    assert int(pick(got["gap_hist"]).sum()) + int(pick(got["gap_above"])) == errors - fie
    if emap:
        m = pick(got["map"])
        assert np.array_equal(m.sum(axis=0), pick(got["carrier_errors"])) and np.array_equal(m.sum(axis=1), pick(got["symbol_errors"]))


# ---- the twins of the header's functions
def position(i, nd, bps):
    """Stream bit i of a frame -> (OFDM symbol, data index, label bit): q = i // bps = s nd + d, r = i % bps."""
    q, r = divmod(i, bps)
    s, d = divmod(q, nd)
    return s, d, r


def recip(bps):
    return (65536 + bps - 1) // bps


def small_div(n, rc):
    return (n * rc) >> 16


def frame_bits(shape):
    return shape["nd"] * shape["n_symb"] * shape["bps"]


def bit_bytes(shape):
    """The two bit buffers of a chunk: the decisions and the scrambled reference, frame_words words each."""
    return 8 * shape["frame_words"]


def chunk_model(shape, f64, receiver, scr, fade_taps, fpp, cap):
    """As the matching sweep budgets its chunk, with the bit buffers beside it; receiver 4 always has the draw regions."""
    per = frame_bytes(shape, f64, scr, receiver == 4, fade_taps) + bit_bytes(shape)
    budget = BUDGET
    if receiver == 4:
        per += t4_frame_bytes(shape, f64)
        budget = 2 * BUDGET
    ch = cap if cap > 0 else max(1, budget // per)
    return max(1, min(ch, fpp, 65535))


def pass_model(shape, gap_bins, frames):
    """(threads, symbols_in_lds, lds, flush_frames, launch_frames, grid): uint32 counters carrier[nd], symbol[N_symb], label[bps],
    gap[gap_bins + 1] and 20 words of scratch within 64 KiB, the symbol table left out where it does not fit; a workgroup may add
    frame_bits per frame to a counter, so it takes at most (2^32 - 1) // frame_bits frames."""
    words = shape["nd"] + shape["bps"] + gap_bins + 1 + SCRATCH_WORDS
    sym = 4 * (words + shape["n_symb"]) <= LDS_LIMIT
    lds = 4 * (words + (shape["n_symb"] if sym else 0))
    flush = max(1, COUNTER_MAX // max(1, frame_bits(shape)))
    launch = max(1, min(frames, min(flush * MAX_GRID, 1 << 31)))
    return (THREADS, int(sym), lds, flush, launch, min(launch, MAX_GRID))


# ---- the refusals, in their order: (refusal id, what breaks a good call for it, message)
def table_order(what):
    return [("frame_bits", dict(n_symb=22369622), f"{what}: a frame must have at most 2^32 - 1 bits of 1 .. 8 per symbol (4294967424, 4)"),
            ("gap_bins", dict(gap_bins=0), f"{what}: gap_bins must be 1 .. 1024 (0)"),
            ("output", dict(out=0), f"{what}: no output is given")]


def good_profile():
    return dict(SHAPE, plan=1, bits=1, ref=1, n_frames=3, gap_bins=64, out=1)


def profile_order():
    what = "bit_error_profile"
    return ([("args", dict(ref=0), f"{what}: bad arguments"),
             ("device", dict(ctx_device=1), "RX plan belongs to device 0, the context is on device 1"),
             ("no_data", dict(nd=0), f"{what}: the plan has no data carriers"),
             ("frames", dict(n_frames=1 << 31), f"{what}: n_frames must be 0 .. 2^31 - 1 (2147483648)")] + table_order(what))


def good_study(receiver, f64):
    """An ofdm_error_study call every check accepts: 1 point of 5 frames, a 3-tap h, scrambled, the plan descrambling; receiver 4
    with both impairments drawn and every flag on."""
    t4 = receiver == 4
    return dict(SHAPE, descr=DESCR, plan=1, f64=f64, f64_flag=f64, receiver=receiver, side=1, frame0=0, n_points=1, fpp=5, max_chunk=0,
                points=1, sto_mode=2 if t4 else 0, cfo_mode=2 if t4 else 0, time_desync=int(t4), freq_desync=int(t4), mp_desync=1,
                reg=REGISTER, h=3, taps="none", power=1.0, gap_bins=64, out=1)


def _plan_order(what, f64):
    return [("device", dict(ctx_device=1), "RX plan belongs to device 0, the context is on device 1"),
            ("precision", dict(f64_flag=1 - f64), f"{what}: precision flag differs from the plan's"),
            ("no_data", dict(nd=0), f"{what}: the plan has no data carriers"),
            ("pilots", dict(pilots_in_band=0), f"{what}: pilots outside 1..N_carrier are not supported"),
            ("nfft", dict(nfft=100), f"{what}: unsupported Nfft 100 / T_guard 32"),
            ("stream", dict(frame0=(1 << 32) - 5), f"{what}: frame index outside the 32-bit stream range")]


_DESCR_ORDER = [("register", dict(reg="100101010000020"), "register entries must be 0 or 1"),
                ("descr_needed", dict(descr=0), "with the Scrambler on the plan needs a DeScrambler with the same register "
                                                "(ofdm_rx_plan_set_descrambler)")]


def study_order(receiver, f64):
    own = [("receiver", dict(receiver=3), "error_study: receiver must be 4 (rx_chain_task4) or 5 (rx_chain_task5) (3)"),
           ("side", dict(side=2), "error_study: side must be 0 (payload) or 1 (channel) (2)"),
           ("channel", dict(taps="0,3"), "error_study: give h (one channel for every frame) or taps (a channel per frame), not both")]
    if receiver == 5:
        what = "ber_sweep_task5"
        sweep = ([("task5_imp", dict(sto_mode=1), "error_study: receiver 5 runs as ber_sweep_task5 does: no sto_mode / cfo_mode, "
                                                  "time_desync and freq_desync 0, mp_desync 1"),
                  ("args", dict(max_chunk=-1), f"{what}: bad arguments"),
                  ("points_missing", dict(points=0), f"{what}: snr_db / seeds missing"),
                  ("points_many", dict(n_points=1 << 31), f"{what}: too many points")] + _plan_order(what, f64) +
                 [("mmse_points", dict(mmse=1, n_points=2), f"{what}: an MMSE-mode plan is built for one SNR (n_points must be 1)")] +
                 [(rid, brk, f"{what}: {msg}") for rid, brk, msg in _DESCR_ORDER] +
                 [("channel", dict(h="bad"), "tx_frames_fused: bad channel")])
    else:
        what = "ber_sweep_task4"
        sweep = ([("args", dict(fpp=-1), f"{what}: bad arguments"),
                  ("channel", dict(h="bad"), "tx_frames_fused: bad channel"),
                  ("chunk_cap", dict(max_chunk=65536), f"{what}: max_frames_per_chunk must be 0..65535 (the limit of rx_chain_task4)"),
                  ("points_missing", dict(points=0), f"{what}: snr_db / seeds missing"),
                  ("points_many", dict(n_points=1 << 31), f"{what}: too many points")] + _plan_order(what, f64) +
                 [("modes", dict(sto_mode=3), f"{what}: sto_mode / cfo_mode must be 0, 1 or 2")] +
                 [(rid, brk, f"{what}: {msg}") for rid, brk, msg in _DESCR_ORDER])
    return own + sweep + table_order("error_study")
