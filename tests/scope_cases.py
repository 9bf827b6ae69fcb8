"""Hand-written model of csrc/scope_plan.hpp (constellation capture of the Task-4 receiver and sweep): the refusals of
ofdm_rx_chain_task4_iq and ofdm_ber_sweep_task4_scope in the order they are made, the LDS the density grid adds to the
equalise / demap stage, and the bin of a value.  TEST INFRASTRUCTURE: a helper module (no tests here), imported by
test_scope_plan_host.py (against the header, on the CPU) and test_gpu_scope_task4.py (against the library).  Nothing here
calls into the product.

The binning, as the header of the library states it:
    scale = bins / (2 * half_width)                       (double)
    col   = clamp(floor((re + half_width) * scale), 0, bins - 1),   row the same from im   (double arithmetic)
    a point with a non-finite re or im is not binned, it is counted as dropped."""
import math

import numpy as np

STAGE_LDS_LIMIT = 150 * 1024
BINS_ALLOWED = (8, 16, 32, 64, 128)

# the messages, as printf formats (%lld / %d / %zu: integers)
MSG_IQ_FIRST = "rx_chain_task4_iq: iq_first must be >= 0 (%lld)"
MSG_IQ_COUNT = "rx_chain_task4_iq: iq_count must be >= 1 (%lld)"
MSG_IQ_END = "rx_chain_task4_iq: iq_first + iq_count must not exceed nd * N_symb = %lld"
MSG_DENSITY_OUT = "ber_sweep_task4_scope: density_out missing (ofdm_ber_sweep_task4_nmse is the call without it)"
MSG_BINS = "ber_sweep_task4_scope: bins must be 8, 16, 32, 64 or 128 (%d)"
MSG_HALF_WIDTH = "ber_sweep_task4_scope: half_width must be finite and > 0"
MSG_SKIP = "ber_sweep_task4_scope: scope_skip must be 0 .. nd * N_symb - 1 (%lld)"
MSG_LDS = "ber_sweep_task4_scope: the equalise / demap stage with a %d x %d grid needs %zu bytes of LDS (at most %zu)"
MESSAGES = dict(iq_first=MSG_IQ_FIRST, iq_count=MSG_IQ_COUNT, iq_end=MSG_IQ_END, density_out=MSG_DENSITY_OUT, bins=MSG_BINS,
                half_width=MSG_HALF_WIDTH, skip=MSG_SKIP, lds=MSG_LDS)
IQ_ORDER = ("iq_first", "iq_count", "iq_end")
DENSITY_ORDER = ("density_out", "bins", "half_width", "skip", "lds")


def fmt(msg, *args):
    return msg.replace("%lld", "%d").replace("%zu", "%d") % args


def iq_refusal(first, count, decisions):
    """None, or (id, message) of the first check of ofdm_rx_chain_task4_iq's window that fails."""
    if first < 0:
        return "iq_first", fmt(MSG_IQ_FIRST, first)
    if count < 1:
        return "iq_count", fmt(MSG_IQ_COUNT, count)
    if first + count > decisions:
        return "iq_end", fmt(MSG_IQ_END, decisions)
    return None


def stage_lds(f64, n_carrier, decisions):
    """eq_demap_kernel's dynamic LDS without a grid: 1 ./ H per carrier, a byte per decision padded to 32, 16 spare bytes."""
    return (16 if f64 else 8) * n_carrier + ((decisions + 31) & ~31) + 16


def grid_layout(f64, n_carrier, decisions, bins):
    """(offset of the grid, bytes the grid adds, bytes of the stage with it): the grid starts on the next 16-byte boundary."""
    base = stage_lds(f64, n_carrier, decisions)
    off = (base + 15) & ~15
    total = off + 4 * bins * bins
    return off, total - base, total


def density_refusal(out, bins, half_width, skip, f64, n_carrier, decisions):
    """None, or (id, message) of the first check of ofdm_ber_sweep_task4_scope's own arguments that fails."""
    if not out:
        return "density_out", MSG_DENSITY_OUT
    if bins not in BINS_ALLOWED:
        return "bins", fmt(MSG_BINS, bins)
    if not (math.isfinite(half_width) and half_width > 0):
        return "half_width", MSG_HALF_WIDTH
    if not 0 <= skip < decisions:
        return "skip", fmt(MSG_SKIP, skip)
    total = grid_layout(f64, n_carrier, decisions, bins)[2]
    if total > STAGE_LDS_LIMIT:
        return "lds", fmt(MSG_LDS, bins, bins, total, STAGE_LDS_LIMIT)
    return None


# ---- the questions of test_scope_plan_host.py
# every refusal of the window, in order: each line fails the named check and passes the ones in front of it; a line that fails
# two names the first
IQ_CASES = [
    # (first, count, decisions)
    (0, 1, 1), (0, 120, 120), (119, 1, 120), (60, 60, 120), (37, 50, 120),            # accepted: whole, last, to the end, middle
    (-1, 1, 120), (-5, 0, 120), (-(2 ** 62), 2 ** 62, 120),                            # iq_first (also with a bad count)
    (0, 0, 120), (3, -2, 120), (500, 0, 120),                                          # iq_count (also behind the end)
    (0, 121, 120), (120, 1, 120), (119, 2, 120), (500, 1, 120), (1, 2 ** 63 - 1, 120),  # iq_end; the sum does not fit 64 bits
]

DENSITY_CASES = [
    # (out, bins, half_width, skip, f64, n_carrier, decisions)
    (1, 8, 1.0, 0, 0, 48, 120), (1, 16, 0.5, 119, 1, 48, 120), (1, 32, 1e-300, 0, 0, 201, 513), (1, 64, 1e300, 5, 1, 800, 34000),
    (1, 128, 1.5, 0, 0, 800, 34000),
    (0, 8, 1.0, 0, 0, 48, 120), (0, 7, -1.0, -1, 0, 48, 120),                          # density_out first, whatever else is wrong
    (1, 0, 1.0, 0, 0, 48, 120), (1, 7, 1.0, 0, 0, 48, 120), (1, 24, 1.0, 0, 0, 48, 120), (1, 256, 1.0, 0, 0, 48, 120),
    (1, -8, float("nan"), 0, 0, 48, 120), (1, 4, 1.0, 500, 0, 48, 120),                # bins before half_width and skip
    (1, 8, 0.0, 0, 0, 48, 120), (1, 8, -1.0, 0, 0, 48, 120), (1, 8, float("inf"), 0, 0, 48, 120),
    (1, 8, float("nan"), 0, 0, 48, 120), (1, 8, float("-inf"), 120, 0, 48, 120),       # half_width before skip
    (1, 8, 1.0, -1, 0, 48, 120), (1, 8, 1.0, 120, 0, 48, 120), (1, 8, 1.0, 2 ** 40, 0, 48, 120),
    (1, 128, 1.0, 0, 1, 4096, 27000), (1, 128, 1.0, 120, 1, 4096, 27000),              # skip before the LDS
    # the LDS: 16 * 4096 + 27008 + 16 = 92560 bytes without a grid; 64 x 64 fits (108944), 128 x 128 does not (158096)
    (1, 64, 1.0, 0, 1, 4096, 27000), (1, 128, 1.0, 0, 1, 4096, 27000),
    # exactly at the limit: 8 * 10000 + 8064 + 16 = 88080 (a multiple of 16) + 65536 = 153616 > 153600; 48 bytes less fits
    (1, 128, 1.0, 0, 0, 10000, 8050), (1, 128, 1.0, 0, 0, 9994, 8050),
]

# (v, half_width, bins, the bin written down by hand).  scale = bins / (2 half_width).
BIN_CASES = [
    ("0", 1.0, 8, 4), ("-0.0", 1.0, 8, 4),                            # zero of either sign: the first bin of the upper half
    ("-1", 1.0, 8, 0), ("1", 1.0, 8, 7),                              # -half_width: bin 0; +half_width: floor = bins, clamped
    ("-0.75", 1.0, 8, 1), ("-0.5", 1.0, 8, 2), ("0.25", 1.0, 8, 5), ("0.75", 1.0, 8, 7),      # exactly on an edge: the upper bin
    ("-0.7500000000000001", 1.0, 8, 0), ("0.2499999999999997", 1.0, 8, 4),                   # just below an edge: the lower bin
    ("0.24999999999999997", 1.0, 8, 5),                              # one ulp of v below 0.25 vanishes in v + half_width = 1.25
    ("-1.0000001", 1.0, 8, 0), ("-7", 1.0, 8, 0), ("-1e300", 1.0, 8, 0), ("-1.7976931348623157e308", 1.0, 8, 0),   # beyond -half_width
    ("1.0000001", 1.0, 8, 7), ("7", 1.0, 8, 7), ("1e300", 1.0, 8, 7), ("1.7976931348623157e308", 1.0, 8, 7),       # beyond +half_width
    ("1e300", 1e-300, 128, 127), ("-1e300", 1e-300, 128, 0),          # the product overflows to +-inf: still an edge bin
    ("inf", 1.0, 8, -1), ("-inf", 1.0, 8, -1), ("nan", 1.0, 8, -1), ("-nan", 1.0, 8, -1),        # not binned
    ("0", 1.5, 64, 32), ("-1.5", 1.5, 64, 0), ("1.5", 1.5, 64, 63), ("1.453125", 1.5, 64, 63), ("1.40625", 1.5, 64, 62),
    ("-0.046875", 1.5, 64, 31), ("3", 1.5, 64, 63),
    ("0.3", 0.25, 16, 15), ("-0.3", 0.25, 16, 0), ("0.1", 0.25, 16, 11), ("0.125", 0.25, 16, 12),
    ("5e-324", 1.0, 128, 64), ("-5e-324", 1.0, 128, 64),              # a denormal vanishes in v + half_width
]


def bin_of(v, half_width, bins):
    """The model's own arithmetic (python floats are doubles): checked against the hand-written BIN_CASES and used for the
    numpy histogram below."""
    if not math.isfinite(v):
        return -1
    t = (v + half_width) * (bins / (2.0 * half_width))
    if not t >= 0:
        return 0
    if t >= bins:
        return bins - 1
    return int(math.floor(t))


def histogram(iq, bins, half_width, skip=0):
    """([bins, bins] int64 grid at [row of im, column of re], dropped) of the points iq[skip:] of one frame, or of every row of
    a [frames, points] array, in double."""
    iq = np.atleast_2d(np.asarray(iq))[:, skip:].astype(np.complex128).ravel()
    scale = bins / (2.0 * half_width)
    fin = np.isfinite(iq.real) & np.isfinite(iq.imag)
    z = iq[fin]
    with np.errstate(over="ignore"):
        col = np.clip(np.floor((z.real + half_width) * scale), 0, bins - 1).astype(np.int64)
        row = np.clip(np.floor((z.imag + half_width) * scale), 0, bins - 1).astype(np.int64)
    grid = np.zeros((bins, bins), dtype=np.int64)
    np.add.at(grid, (row, col), 1)
    return grid, int(iq.size - z.size)
