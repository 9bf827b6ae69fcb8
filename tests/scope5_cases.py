"""Hand-written model of the Task-5 part of csrc/scope_plan.hpp (constellation capture of the Task-5 receiver and sweeps): the
refusals of ofdm_rx_chain_task5_iq and ofdm_ber_sweep_task5_scope in the order they are made, and where the density grid lies
behind the LDS of the symbol stage a route names.  TEST INFRASTRUCTURE: a helper module (no tests here), imported by
test_scope5_plan_host.py (against the header, on the CPU) and test_gpu_scope_task5.py (against the library).  Nothing here calls
into the product.  The binning and the histogram are those of scope_cases.py: one bin function serves both receivers."""
import math

import routes

BINS_ALLOWED = (8, 16, 32, 64, 128)
STAGES = ("generic", "rx_symbols", "wave", "coop4", "r2", "eq_demap")          # SYM_* of chain_route.hpp, in order
GENERIC_LDS_LIMIT = 158 * 1024
STAGE_LDS_LIMIT = 150 * 1024

MSG_IQ_FIRST = "rx_chain_task5_iq: iq_first must be >= 0 (%lld)"
MSG_IQ_COUNT = "rx_chain_task5_iq: iq_count must be >= 1 (%lld)"
MSG_IQ_END = "rx_chain_task5_iq: iq_first + iq_count must not exceed nd * N_symb = %lld"
MSG_DENSITY_OUT = "ber_sweep_task5_scope: density_out missing (ofdm_ber_sweep_task5_fading / _ex are the calls without it)"
MSG_BINS = "ber_sweep_task5_scope: bins must be 8, 16, 32, 64 or 128 (%d)"
MSG_HALF_WIDTH = "ber_sweep_task5_scope: half_width must be finite and > 0"
MSG_SKIP = "ber_sweep_task5_scope: scope_skip must be 0 .. nd * N_symb - 1 (%lld)"
MSG_LDS = "ber_sweep_task5_scope: the %s symbol stage with a %d x %d grid needs %zu bytes of LDS (at most %zu)"
MESSAGES = dict(iq_first=MSG_IQ_FIRST, iq_count=MSG_IQ_COUNT, iq_end=MSG_IQ_END, density_out=MSG_DENSITY_OUT, bins=MSG_BINS,
                half_width=MSG_HALF_WIDTH, skip=MSG_SKIP, lds=MSG_LDS)
IQ_ORDER = ("iq_first", "iq_count", "iq_end")
DENSITY_ORDER = ("density_out", "bins", "half_width", "skip", "lds")


def fmt(msg, *args):
    return msg.replace("%lld", "%d").replace("%zu", "%d") % args


def iq_refusal(first, count, decisions):
    """None, or (id, message) of the first check of ofdm_rx_chain_task5_iq's window that fails."""
    if first < 0:
        return "iq_first", fmt(MSG_IQ_FIRST, first)
    if count < 1:
        return "iq_count", fmt(MSG_IQ_COUNT, count)
    if first + count > decisions:
        return "iq_end", fmt(MSG_IQ_END, decisions)
    return None


def lds_limit(stage):
    return GENERIC_LDS_LIMIT if stage == 0 else STAGE_LDS_LIMIT


def grid_layout(lds, bins):
    """(offset of the grid, bytes of the stage with it): the grid starts on the next 16-byte boundary behind the stage's bytes."""
    off = (lds + 15) & ~15
    return off, off + 4 * bins * bins


def density_refusal(stage, lds, out, bins, half_width, skip, decisions):
    """None, or (id, message) of the first check of ofdm_ber_sweep_task5_scope's own arguments that fails."""
    if not out:
        return "density_out", MSG_DENSITY_OUT
    if bins not in BINS_ALLOWED:
        return "bins", fmt(MSG_BINS, bins)
    if not (math.isfinite(half_width) and half_width > 0):
        return "half_width", MSG_HALF_WIDTH
    if not 0 <= skip < decisions:
        return "skip", fmt(MSG_SKIP, skip)
    total = grid_layout(lds, bins)[1]
    if total > lds_limit(stage):
        return "lds", fmt(MSG_LDS, STAGES[stage], bins, bins, total, lds_limit(stage))
    return None


def wave_lds(nd, n_symb, wpb=4):
    """wave_layout (chain_route.hpp): the wave stage's dynamic LDS at four wavefronts per workgroup."""
    cb = 1
    while (cb * nd) % 32 != 0:
        cb += 1
    unit = cb
    while cb * nd < 1920 and cb < n_symb:
        cb += unit
    if cb >= n_symb:
        cb = n_symb
    codes_bytes = (cb * nd + 31 + 32) & ~31
    wave_bytes = (routes.WV_CODES_OFF + codes_bytes + 15) & ~15
    return routes.WV_OFF_WAVE + wpb * wave_bytes


def stage_of_case(case):
    """(stage index, the stage's dynamic LDS without a grid) of a routes.Case on the route with the MER sums wanted -- the
    formulas of routes.py, stage by stage."""
    r = routes.expected_route(case, case.precision, case.mode, case.descr, True, case.env)
    f = routes._plan_fields(case)
    f64 = case.precision == "fp64"
    decisions = f["nd"] * case.n_symb
    fam = routes.symbols_family(r.symbols)
    if fam == "chain_generic":
        return 0, routes.generic_lds_bytes(case, f, f64)
    if fam == "rx_symbols":
        nw = case.nfft // 512
        return 1, (16 if f64 else 8) * (nw * routes.WAVE_LDS_ELEMS + routes.WAVE_TW_ELEMS) + ((decisions + 31) & ~31)
    if fam == "wave":
        return 2, wave_lds(f["nd"], case.n_symb)
    if fam == "coop4":
        return 3, routes.CP_OFF_CODES + 2 * ((f["nd"] + 63) & ~31)
    if fam == "r2":
        return 4, 8 * (8 * routes.WAVE_LDS_ELEMS + routes.WAVE_TW_ELEMS) + ((decisions + 31) & ~31)
    assert fam == "eq_demap", r.symbols
    return 5, (16 if f64 else 8) * case.nc + ((decisions + 31) & ~31) + 16


# ---- the questions of test_scope5_plan_host.py
IQ_CASES = [
    # (first, count, decisions)
    (0, 1, 1), (0, 288, 288), (287, 1, 288), (96, 100, 288), (48, 192, 288),           # accepted: whole, last, across symbols
    (-1, 1, 288), (-5, 0, 288), (-(2 ** 62), 2 ** 62, 288),                            # iq_first (also with a bad count)
    (0, 0, 288), (3, -2, 288), (500, 0, 288),                                          # iq_count (also behind the end)
    (0, 289, 288), (288, 1, 288), (287, 2, 288), (500, 1, 288), (1, 2 ** 63 - 1, 288),  # iq_end; the sum does not fit 64 bits
]

DENSITY_CASES = [
    # (stage, lds, out, bins, half_width, skip, decisions)
    (0, 9000, 1, 8, 1.0, 0, 144), (1, 13000, 1, 16, 0.5, 143, 144), (2, 50944, 1, 32, 1e-300, 0, 1152),
    (3, 77952, 1, 64, 1e300, 5, 1536), (4, 45056, 1, 128, 1.5, 0, 1050), (5, 9616, 1, 128, 1.5, 0, 1050),
    (2, 50944, 0, 8, 1.0, 0, 1152), (0, 9000, 0, 7, -1.0, -1, 144),                    # density_out first, whatever else is wrong
    (1, 13000, 1, 0, 1.0, 0, 144), (1, 13000, 1, 7, 1.0, 0, 144), (1, 13000, 1, 24, 1.0, 0, 144), (1, 13000, 1, 256, 1.0, 0, 144),
    (1, 13000, 1, -8, float("nan"), 0, 144), (1, 13000, 1, 4, 1.0, 500, 144),          # bins before half_width and skip
    (2, 50944, 1, 8, 0.0, 0, 1152), (2, 50944, 1, 8, -1.0, 0, 1152), (2, 50944, 1, 8, float("inf"), 0, 1152),
    (2, 50944, 1, 8, float("nan"), 0, 1152), (2, 50944, 1, 8, float("-inf"), 1152, 1152),   # half_width before skip
    (3, 77952, 1, 8, 1.0, -1, 1536), (3, 77952, 1, 8, 1.0, 1536, 1536), (3, 77952, 1, 8, 1.0, 2 ** 40, 1536),
    (1, 100000, 1, 128, 1.0, 144, 144),                                                # skip before the LDS
    # the LDS: 100000 bytes of an rx_symbols stage; 64 x 64 fits (100000 + 16384 = 116384), 128 x 128 does not (165536)
    (1, 100000, 1, 64, 1.0, 0, 144), (1, 100000, 1, 128, 1.0, 0, 144),
    # exactly at each limit: 150 KiB = 153600 for every stage but the generic kernel, 158 KiB = 161792 for that one
    (4, 88064, 1, 128, 1.0, 0, 144), (4, 88065, 1, 128, 1.0, 0, 144),                  # 88064 + 65536 = 153600 fits; one byte more pads to + 16
    (0, 96256, 1, 128, 1.0, 0, 144), (0, 96257, 1, 128, 1.0, 0, 144),                  # 96256 + 65536 = 161792 fits
    (0, 90000, 1, 128, 1.0, 0, 144), (5, 90000, 1, 128, 1.0, 0, 144),                  # the same bytes: within the generic limit, beyond the stage limit
]
