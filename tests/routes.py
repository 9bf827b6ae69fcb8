"""Route model and case table of the Task-5 receiver's dispatcher (ofdm_rx_chain_task5_ex).  TEST INFRASTRUCTURE.

`expected_route` restates, in Python, chain_route_choose (ofdm-course_amd/csrc/chain_route.hpp), the host decision by which one
plan and one batch choose their kernels; every predicate names the function or clause it restates.  The model stays hand-written:
tests/test_route_model_host.py compares it with the chooser itself, on the CPU.  `ROUTES` is the hand-written list of
routes that must stay covered, `CASES` the concrete configurations that cover them (tests/test_route_table.py keeps the two
and the env switches of the dispatch sources in step; tests/test_gpu_chain_routes.py runs every case against the oracle).

`python tests/routes.py` prints, for every fp32 OMP case, the smallest top-2 score gap of the ORACLE's own pursuit on the
case's Philox frames (oracle.tx_frame on awgn_philox / payload_bits_philox, CPU only): the evidence that no case has a
near-tied pick (threshold 1e-4 of the maximum, pick_audit.py), recorded in GAPS below the table.
"""
from __future__ import annotations

import os
import re
from collections import namedtuple
from dataclasses import dataclass, field

import numpy as np

Route = namedtuple("Route", "entry front estimator omp_state c0 symbols ba descr mer")


class Refused(Exception):
    """The host check that refuses the configuration: `where` = the refusal id of chain_route_choose (chain_route.hpp, REFUSE_*
    in lower case), `fragment` = a piece of the message."""

    def __init__(self, where, fragment):
        super().__init__(f"{where}: {fragment}")
        self.where, self.fragment = where, fragment


# ---------------------------------------------------------------------------------------------------------------------
# constants of the dispatch sources
# ---------------------------------------------------------------------------------------------------------------------
CH_MAXT = 32                    # ofdm_chain.hip
FAST_MAXT = 32                  # chain_fast_core.hpp
WAVE_LDS_ELEMS = 512 + 64       # chain_fast_core.hpp
WAVE_TW_ELEMS = 2 * 7 * 64      # chain_fast_core.hpp
OMP_RT = 8                      # chain_fast_core.hpp
FAST_MAX_DECISIONS = 48 * 1024  # ofdm_chain_fast.hip
GENERIC_LDS_LIMIT = 158 * 1024  # ofdm_chain.hip
STAGE_LDS_LIMIT = 150 * 1024    # ofdm_chain_fast.hip, ofdm_chain_split.hip
SPLIT_LDS_LIMIT = 120 * 1024    # ofdm_chain_split.hip
WV_N = 2048                     # ofdm_chain_wave.hip
WV_TR_ELEMS, WV_TW_ROWS = 576, 31                                   # ofdm_chain_wave.hip
WV_OFF_WAVE = 8 * 64 * WV_TW_ROWS + 8 * 64 * 7 + 8 * 64 * 4 + 256   # ofdm_chain_wave.hip
WV_CODES_OFF = 8 * WV_TR_ELEMS + 8 * 64 + 16                        # ofdm_chain_wave.hip
CP_N = 8192                     # ofdm_chain_coop.hip
CP_OFF_CODES = 2 * (8 * 64 * 7) + 4 * 8 * 576 + 3 * 2048 * 8        # ofdm_chain_coop.hip

DISPATCH_FILES = ("chain_route.hpp", "ofdm_chain.hip", "ofdm_chain_fast.hip", "ofdm_chain_split.hip", "ofdm_chain_wave.hip",
                  "ofdm_chain_coop.hip", "ofdm_chain_mmse.hip")
# chain switches read outside the dispatch files: none since the chooser (chain_route.hpp) reads OFDM_PILOT_FPW, the frames per
# wavefront of the fused symbol-1 + OMP launch, for the route it reports
EXTRA_SWITCHES = ()

BITS_PER_AXIS = {"BPSK": 0, "QPSK": 0, "8PSK": 0, "16QAM": 2, "64QAM": 3, "256QAM": 4}   # ofdm_core.hip (kind 1 only)
BPS = {"BPSK": 1, "QPSK": 2, "8PSK": 3, "16QAM": 4, "64QAM": 6, "256QAM": 8}


def _align16(n):
    return (n + 15) & ~15


def fft_lds_elems(n):           # fft_core.hpp
    return n + (n >> 3) + 8


def fft_xforms_per_wg(n):       # fft_core.hpp
    threads = n // 8 if n // 8 >= 256 else 256
    return threads // (n // 8)


# ---------------------------------------------------------------------------------------------------------------------
# a case
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    nfft: int
    nc: int
    comb: int                    # comb 1:comb:N_carrier, unless `pilots` is given
    const: str
    n_symb: int
    delays: tuple                # channel tap delays (amplitudes: linspace(1, 0.35) with a phase ramp); dominant_taps = len
    precision: str = "fp32"
    mode: str = "omp"            # omp | mmse
    descr: bool = False
    mer: bool = False
    env: dict = field(default_factory=dict)
    base_env: dict | None = None  # switch-only cases: the route the result is also compared with (None: no such comparison)
    h_tol64: float | None = None  # fp64 switch cases whose switch changes the arithmetic: rel_l2 bound on H against the base route
                                  # (None: H must be bit-identical)
    pilots: tuple | None = None  # ("percent", pct, tail) | ("extra", carrier, ...) = the comb plus these carriers
    k_atoms: int | None = None
    n_frames: int = 5
    seed: int = 1
    snr: float = 30.0
    set_aside: int = 0           # frames the case may set aside for a near-tied pick (0: tie-free by construction)
    covers: str = ""             # which gap of the issue / which switch the case is there for

    # -- geometry ------------------------------------------------------------------------------------------------
    def pilot_carriers(self):
        comb = np.arange(1, self.nc + 1, self.comb)
        if self.pilots is None:
            return comb
        if self.pilots[0] == "percent":                      # oracle.pilot_layout_percent (T4/Main_model_Task_4.m:14-24)
            _, pct, tail = self.pilots
            amount = int(np.floor(pct / 100 * self.nc + 0.5))
            step = self.nc // amount
            return np.array(list(range(1, self.nc - tail + 1, step)) + [self.nc])
        assert self.pilots[0] == "extra"
        return np.concatenate([comb, np.array(self.pilots[1:], dtype=comb.dtype)])

    def data_carriers(self):
        allc = np.arange(1, self.nc + 1)
        return allc[~np.isin(allc, self.pilot_carriers())]

    @property
    def K(self):
        return int(self.k_atoms) if self.k_atoms is not None else int(np.ceil(self.nc / self.comb))

    @property
    def taps(self):
        n = len(self.delays)
        amp = np.linspace(1.0, 0.35, n) * np.exp(1j * 0.9 * np.arange(n))
        return np.stack([np.asarray(self.delays, dtype=complex), amp], axis=1)

    def cfg(self):
        """The FrameConfig of the case (imports the package)."""
        from ofdm_course_amd import frames as fr
        return fr.FrameConfig(self.name, self.nfft, self.nc, self.comb, self.const, N_symb=self.n_symb, taps=self.taps,
                              SNR_dB=self.snr, dominant_taps=len(self.delays),
                              pilots=None if self.pilots is None else self.pilot_carriers().astype(np.float64),
                              K_atoms=self.k_atoms)

    def route(self):
        return expected_route(self, self.precision, self.mode, self.descr, self.mer, self.env)


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
def _plan_fields(c):
    """What ofdm_rx_plan_create derives from the carriers (ofdm_chain.hip)."""
    pc0 = np.asarray(c.pilot_carriers(), dtype=np.int64) - 1
    dc0 = np.asarray(c.data_carriers(), dtype=np.int64) - 1
    mod4 = 0
    for r in np.unique(dc0 & 3):
        mod4 |= 1 << int(r)
    in_band = bool(np.all(pc0 + 1 <= c.nc))
    comb_m, lg_up = 0, -1
    if pc0.size >= 2 and pc0[0] == 0:
        comb = int(pc0[1] - pc0[0])
        is_comb = comb >= 1 and c.nfft % comb == 0 and bool(np.all(pc0 == comb * np.arange(pc0.size)))
        m = c.nfft // comb if is_comb else 0
        if is_comb and pc0.size <= m:
            comb_m = m
        if is_comb and m <= 512 and 512 % m == 0 and pc0.size <= m:
            lg_up = 0
            while (m << lg_up) < 512:
                lg_up += 1
    return dict(np=int(pc0.size), nd=int(dc0.size), mod4=mod4, in_band=in_band, comb_m=comb_m, lg_up=lg_up)


def generic_lds_bytes(c, f, f64):
    """ofdm_chain.hip (mirrors chain_layout + launch_chain)."""
    cs = 16 if f64 else 8
    taps = len(c.delays)
    b = _align16(cs * fft_lds_elems(c.nfft)) + _align16(cs * f["np"]) + _align16(cs * c.K) + _align16(16 * CH_MAXT * 2)
    b += _align16(4 * (CH_MAXT + 4)) + _align16(16 * taps * taps) + _align16(f["nd"] * c.n_symb)
    return b * fft_xforms_per_wg(c.nfft)


def wave_layout_ok(nd, n_symb, wpb):
    """ofdm_chain_wave.hip."""
    cb = 1
    while (cb * nd) % 32 != 0:
        cb += 1
    unit = cb
    while cb * nd < 1920 and cb < n_symb:
        cb += unit
    if cb >= n_symb:
        cb = n_symb
    codes_bytes = (cb * nd + 31 + 32) & ~31
    if codes_bytes > 6144:
        return False
    wave_bytes = (WV_CODES_OFF + codes_bytes + 15) & ~15
    return WV_OFF_WAVE + wpb * wave_bytes <= (78 if wpb == 8 else 52) * 1024


def omp_layout(np_, k, taps, f64, fft_elems, env):
    """ofdm_chain_fast.hip -> (fpw, reg_c0, total bytes)."""
    cs = 16 if f64 else 8
    wave = taps > OMP_RT
    state = ((cs * taps * (taps | 1) + 15) & ~15) if wave else 16        # (omp_wave_rs: omp_wave_core.hpp)
    gram_elems = ((k + 511) & ~511) + k if wave else k
    per_frame = cs * (np_ + 1) + cs * k + state
    fpw = 1 if wave else 4
    v = int(env.get("OFDM_OMP_FPW", 0) or 0)
    if not wave and v in (1, 2, 4, 8):
        fpw = v
    while fpw > 1 and 4 * fpw * per_frame + cs * gram_elems > 96 * 1024:
        fpw >>= 1
    fb = 4 * fpw
    reg_c0 = wave and fft_elems > 0 and k <= 512 and k <= np_ + 1 and "OFDM_OMP_C0_LDS" not in env
    fft_bytes = _align16(cs * fft_elems)
    if reg_c0:
        total = _align16(cs * gram_elems) + max(fb * state, _align16(cs * fb * (np_ + 1)) + fft_bytes)
    else:
        total = _align16(cs * fb * (np_ + 1)) + _align16(cs * fb * k) + _align16(cs * gram_elems) + max(fb * state, fft_bytes)
    return fpw, bool(reg_c0), total


OMP_ROUTES = ("auto", "batch", "wide")


def wide_serves(nfft, k, taps):
    """omp_wide_refusal (omp_wide_host.hpp)."""
    return nfft in (512, 1024, 2048, 4096) and 1 <= k <= nfft and 1 <= taps <= 32 and taps <= k


def omp_kernel(c, f, f64, env, omp_route):
    """omp_route_choose (omp_wide_host.hpp) on omp_batch_kernel's LDS need: 'batch' or 'wide', or Refused."""
    by_fft = f["comb_m"] == 2048 and f["np"] <= 2048 and c.K <= 2048 and "OFDM_OMP_NO_FFT" not in env
    total = omp_layout(f["np"], c.K, len(c.delays), f64, fft_lds_elems(2048) if by_fft else 0, env)[2]
    if omp_route == "batch":
        return "batch"                                                   # (its own refusal comes later: omp_lds)
    if omp_route == "auto" and total <= STAGE_LDS_LIMIT:
        return "batch"
    if not wide_serves(c.nfft, c.K, len(c.delays)):
        raise Refused("omp_route", "wide OMP route")
    return "wide"


def _omp_estimator(c, f, f64, env, kernel="batch"):
    """The OMP stage of the chooser: omp_batch_kernel's form, or the wide kernel."""
    if kernel == "wide":
        return "omp_wide", "-", "-"
    taps = len(c.delays)
    by_fft = f["comb_m"] == 2048 and f["np"] <= 2048 and c.K <= 2048 and "OFDM_OMP_NO_FFT" not in env
    fpw, reg_c0, total = omp_layout(f["np"], c.K, taps, f64, fft_lds_elems(2048) if by_fft else 0, env)
    if total > STAGE_LDS_LIMIT:
        raise Refused("omp_lds", "OMP stage needs")
    mfma = (not f64) and c.K % 16 == 0 and f["np"] % 4 == 0 and "OFDM_OMP_NO_MFMA" not in env
    est = "omp_fft" if by_fft else "omp_mfma" if mfma else "omp_scalar"
    # frames per wavefront of the register-resident pursuit: a launch geometry the kernel's lane groups follow 
    return est, "wave" if taps > OMP_RT else f"regs<fpw={fpw}>", "reg" if reg_c0 else "lds"


def _mmse_estimator(f, f64, env):
    """mmse_stage_run (chain_fast_core.hpp), ofdm_chain_mmse.hip; the factors exist on fp32 plans only
    (ofdm_chain.hip)."""
    np_pad = (f["np"] + 15) & ~15                                        # ofdm_chain.hip
    factored = (not f64) and f["np"] % 4 == 0 and np_pad % 16 == 0 and "OFDM_MMSE_NO_MFMA" not in env \
        and "OFDM_MMSE_DENSE" not in env                                 # ofdm_chain_mmse.hip
    if factored:
        if np_pad <= 256 and "OFDM_MMSE_TWO_LAUNCHES" not in env:        # (h_out of the stage is the plan's workspace)
            return "mmse_fused"
        g = int(env.get("OFDM_MMSE_G", 4))                               # mmse_apply_mfma_kernel<G>
        return f"mmse_factored<G={8 if g >= 8 else 4 if g >= 4 else 2 if g >= 2 else 1}>"
    if (not f64) and f["np"] % 4 == 0 and "OFDM_MMSE_NO_MFMA" not in env:   # (m_pad is a multiple of 16 by construction)
        return "mmse_dense_mfma"
    return "mmse_dense_scalar"
def expected_route(c, precision, mode, descr, mer, env, omp_route="batch"):
    """The route ofdm_rx_chain_task5_ex takes for case geometry `c` on a plan in `omp_route`, or raises Refused."""
    f64 = precision == "fp64"
    mmse = mode == "mmse"
    f = _plan_fields(c)
    taps, bps, ba = len(c.delays), BPS[c.const], BITS_PER_AXIS[c.const]
    decisions = f["nd"] * c.n_symb
    forced_generic = "OFDM_CHAIN_GENERIC" in env
    # chain_route_choose, the fast clause
    fast_ok = (not forced_generic) and c.nfft in (512, 1024, 2048, 4096) and taps <= FAST_MAXT and bps <= 8 \
        and decisions <= FAST_MAX_DECISIONS
    fast = f["in_band"] and fast_ok                                      # ofdm_chain.hip
    split = False
    if not fast and f["in_band"]:                                        # ofdm_chain.hip
        # chain_split_fits (chain_route.hpp)
        split_ok = (not forced_generic) and taps <= FAST_MAXT and bps <= 8 and \
            (16 if f64 else 8) * c.nc + ((decisions + 31) & ~31) <= SPLIT_LDS_LIMIT
        split = split_ok and (c.nfft > 4096 or mmse or generic_lds_bytes(c, f, f64) > GENERIC_LDS_LIMIT)

    if not fast and not split:                                           # ofdm_chain.hip
        if mmse:
            raise Refused("mmse_entry", "the MMSE mode of a plan needs pilots inside 1..N_carrier")
        if omp_route == "wide":
            raise Refused("wide_generic", "generic single-kernel entry")
        if generic_lds_bytes(c, f, f64) > GENERIC_LDS_LIMIT:
            raise Refused("generic_lds", "bytes of LDS (limit 158 KiB")
        # one kernel: transform, in-kernel correlation and pursuit, equalise, demap, pack
        return Route("generic", "fused", "omp_scalar", "-", "-", "chain_generic", ba, "pass" if descr else "none", mer)

    kernel = None
    if mmse:
        est, state, c0 = _mmse_estimator(f, f64, env), "-", "-"
    else:
        kernel = omp_kernel(c, f, f64, env, omp_route)                   # refused before anything else of the fast / split forms

    if fast:
        nw = c.nfft // 512                                               # ofdm_chain_fast.hip
        prune = c.nc <= 128 * nw
        fused = (not mmse) and f["lg_up"] >= 0 and taps <= OMP_RT and c.K <= 512 and omp_route != "wide" \
            and "OFDM_FAST_UNFUSED" not in env
        if fused:
            # rx_pilot_omp_kernel: c0 by a wave-local inverse transform, register-resident pursuit (ofdm_chain_pilot.hip)
            cs, ystride, pf = (16 if f64 else 8), max(f["np"], c.K), 4                     # ofdm_chain_pilot.hip
            v = int(env.get("OFDM_PILOT_FPW", 0) or 0)
            if v in (1, 2, 4, 8):
                pf = v
            while pf > 1 and cs * nw * pf * ystride > 8 * 1024:
                pf >>= 1
            front, est, state, c0 = "fused", "omp_fft", f"regs<fpw={pf}>", "lds"
        else:
            front = "pilot+omp"
            if not mmse:
                est, state, c0 = _omp_estimator(c, f, f64, env, kernel)
        # chain_route_choose, the wave clause: the wave stage whenever its conditions hold, DeScrambler or not (a descrambling MMSE
        # or MER plan takes it too and hands its decisions to descr_pass_kernel; seen in the kernel trace, profiles/routes/README.md)
        wave = (not f64) and nw == 4 and prune and "OFDM_FAST_NO_WAVE" not in env \
            and taps <= FAST_MAXT and wave_layout_ok(f["nd"], c.n_symb, 4) and wave_layout_ok(f["nd"], c.n_symb, 8) \
            and not (mer and "OFDM_WAVE_EXACT_SLICER" in env)
        if wave:
            no_skip = "OFDM_WAVE_NO_SKIP" in env
            if "OFDM_WAVE_EXACT_SLICER" in env:                          # ofdm_chain_wave.hip
                form = "exact"
            elif f["mod4"] == 14 and not no_skip:
                form = "skip0"
            elif f["mod4"] == 10 and not no_skip:
                form = "skip02"
            else:
                form = "none"
            symbols = f"wave<{form}>"
        else:
            dyn = (16 if f64 else 8) * (nw * WAVE_LDS_ELEMS + WAVE_TW_ELEMS) + ((decisions + 31) & ~31)
            if dyn > STAGE_LDS_LIMIT:
                raise Refused("symbol_lds", "symbol stage needs")
            symbols = f"rx_symbols<{nw},{'true' if prune else 'false'}>"
        # ofdm_chain.hip: in the pack stage of the wave kernel, except with MER; every other stage hands over raw decisions
        d = "none" if not descr else "in_kernel" if (wave and not mer and not mmse) else "pass"
        return Route("fast", front, est, state, c0, symbols, ba, d, mer)

    # split form, ofdm_chain_split.hip
    if not mmse:
        est, state, c0 = _omp_estimator(c, f, f64, env, kernel)
    d = "pass" if descr else "none"
    if not f64:
        # chain_route_choose, the coop4 clause
        coop = "OFDM_SPLIT_NO_COOP" not in env and c.nfft == CP_N and c.nc <= CP_N // 4 and c.K <= 512 and taps <= FAST_MAXT \
            and (f["mod4"] & 1) == 0 and (f["nd"] & 31) == 0 \
            and CP_OFF_CODES + 2 * ((f["nd"] + 63) & ~31) <= 78 * 1024
        # chain_route_choose, the r2 clause
        r2 = (not coop) and "OFDM_SPLIT_NO_R2" not in env and c.nfft == 8192 and c.nc <= 2048 and taps <= FAST_MAXT and \
            8 * (8 * WAVE_LDS_ELEMS + WAVE_TW_ELEMS) + ((decisions + 31) & ~31) <= 78 * 1024
        if coop or r2:
            return Route("split", "demod8192", est, state, c0, "coop4" if coop else "r2", ba, d, mer)
    if c.nfft == 8192 and "OFDM_SPLIT_GENERIC_FFT" not in env:
        # without the fused pilot LS values, or under OFDM_SPLIT_ALL_ROWS, the rows of pilot-only sub-transforms are
        # computed on data symbols too
        front = "demod8192+pls" if "OFDM_SPLIT_NO_PLS_FUSE" in env else \
            "demod8192<all_rows>" if "OFDM_SPLIT_ALL_ROWS" in env else "demod8192"
    else:
        front = "demod_generic+pls"
    vec = (not f64) and c.nc % 2 == 0 and c.nc <= 2048 and "OFDM_EQD_SCALAR" not in env   # (x_stride = N_carrier)
    if (16 if f64 else 8) * c.nc + ((decisions + 31) & ~31) + 16 > STAGE_LDS_LIMIT:
        raise Refused("eq_demap_lds", "equalise / demap stage needs")
    return Route("split", front, est, state, c0, f"eq_demap<{'vec' if vec else 'scalar'}>", ba, d, mer)


# ofdm_chain_fast.hip cannot fire: the fast path is entered with at most 48 Ki decisions , so the symbol stage asks
# for at most 16 * (8 * 576 + 896) + 49152 = 137216 bytes (fp64, Nfft 4096), below its 150 KiB limit.  test_route_table.py
# recomputes this bound; there is therefore no refusal case for that line.
FAST_SYMBOL_LDS_MAX = 16 * (8 * WAVE_LDS_ELEMS + WAVE_TW_ELEMS) + FAST_MAX_DECISIONS


def symbols_family(symbols):
    return symbols.split("<")[0]


def estimator_family(estimator):
    return estimator.split("_")[0]


def strip_knob(value):
    """A field value without its launch-geometry knob: 'regs<fpw=2>' -> 'regs', 'mmse_factored<G=8>' -> 'mmse_factored'."""
    return value.split("<")[0] if isinstance(value, str) and not value.startswith(("rx_symbols", "wave", "eq_demap")) else value


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
T3 = (0, 3, 7)
T12 = (0, 2, 5, 9, 14, 20, 27, 35, 44, 54, 65, 77)
NO8192 = {"OFDM_SPLIT_NO_COOP": "1", "OFDM_SPLIT_NO_R2": "1"}




def _both(name, *a, **kw):
    """The same case in fp32 and fp64."""
    return [Case(f"{name}-fp32", *a, precision="fp32", **kw), Case(f"{name}-fp64", *a, precision="fp64", **kw)]


PCT = ("percent", 15, 2)                      # the Task-4 layout rule: comb_m = 0, comb_lg_up = -1, every residue class holds data

CASES: list[Case] = [
    # ---- the generic kernel: Nfft below 512 has no fast path (ofdm_chain_fast.hip); every slicer order
    *_both("generic-64-qpsk-descr", 64, 32, 4, "QPSK", 3, (0, 2, 5), descr=True, covers="descr pass after the generic kernel"),
    *_both("generic-128-16qam-mer", 128, 64, 4, "16QAM", 3, T3, mer=True, snr=24.0),
    *_both("generic-256-64qam", 256, 100, 4, "64QAM", 3, T3),
    *_both("generic-256-256qam", 256, 64, 4, "256QAM", 2, T3, snr=36.0),
    # gap 2: a pilot outside 1..N_carrier forces the generic kernel at every Nfft (ofdm_chain.hip)
    *_both("generic-oob-256-descr", 256, 64, 4, "16QAM", 3, T3, pilots=("extra", 80), descr=True, covers="gap 2"),
    Case("generic-oob-2048-mer", 2048, 512, 4, "64QAM", 2, T3, pilots=("extra", 600), mer=True, snr=24.0, seed=7, covers="gap 2"),
    # ---- fast path, fused symbol-1 + OMP launch (comb whose Nfft/comb divides 512), rx_symbols_kernel<NW, PRUNE2>
    *_both("fast-512-pruned", 512, 128, 4, "QPSK", 3, T3),
    *_both("fast-512-unpruned-mer", 512, 200, 4, "16QAM", 3, T3, mer=True, snr=24.0),
    *_both("fast-1024-pruned", 1024, 256, 4, "64QAM", 3, T3),
    *_both("fast-1024-unpruned-descr", 1024, 400, 8, "256QAM", 2, T3, descr=True, snr=36.0, covers="gap 7 (rx_symbols + pass)"),
    Case("fast-2048-pruned-fp64", 2048, 512, 4, "64QAM", 3, T3, precision="fp64"),
    Case("fast-2048-pruned-nowave", 2048, 512, 4, "64QAM", 3, T3, env={"OFDM_FAST_NO_WAVE": "1"}, base_env={}),
    Case("fast-512-pilot-fpw", 512, 128, 4, "16QAM", 2, T3, env={"OFDM_PILOT_FPW": "1"}, base_env={}, n_frames=7),
    # gap 3: PRUNE2 = false at NW = 4 and NW = 8
    *_both("fast-2048-unpruned", 2048, 800, 8, "16QAM", 2, T3, covers="gap 3"),
    *_both("fast-4096-unpruned-mer", 4096, 1400, 8, "64QAM", 2, T3, mer=True, snr=24.0, covers="gap 3"),
    *_both("fast-4096-pruned", 4096, 1024, 8, "8PSK", 2, T3),
    # ---- wave-per-frame symbol stage (Nfft 2048, fp32, N_carrier <= 512): the three skip forms, the exact slicer, every order
    Case("wave-skip0-64qam", 2048, 512, 4, "64QAM", 3, T3),
    Case("wave-skip0-qpsk-descr", 2048, 448, 4, "QPSK", 3, T3, descr=True),
    Case("wave-skip02-16qam-mer", 2048, 200, 2, "16QAM", 3, T3, mer=True, snr=24.0),
    Case("wave-none-256qam", 2048, 384, 8, "256QAM", 2, T3, snr=36.0),
    Case("wave-exact-64qam", 2048, 512, 4, "64QAM", 3, T3, env={"OFDM_WAVE_EXACT_SLICER": "1"}, base_env={}),
    Case("wave-noskip-16qam", 2048, 512, 4, "16QAM", 3, T3, env={"OFDM_WAVE_NO_SKIP": "1"}, base_env={}, covers="gap 6"),
    Case("wave-descr-mer-pass", 2048, 512, 4, "16QAM", 3, T3, descr=True, mer=True, snr=24.0, covers="descr pass after the wave MER variant"),
    # gap 8: a percent layout and K != Np -- the three-launch front end as the natural route, no wave skip, nd % 32 != 0
    Case("wave-percent-k-scalar", 2048, 500, 6, "64QAM", 3, T3, pilots=PCT, k_atoms=70, covers="gap 8: K < Np, K % 16 != 0"),
    *_both("fast-percent-2048", 2048, 800, 6, "64QAM", 2, T3, pilots=PCT, k_atoms=144, covers="gap 8: the Task-4 layout"),
    *_both("fast-percent-1024-k-gt-np", 1024, 300, 6, "16QAM", 3, T3, pilots=PCT, k_atoms=64, covers="gap 8: K > Np + 1"),
    *_both("fast-percent-512", 512, 200, 6, "8PSK", 3, T3, pilots=PCT, k_atoms=40, covers="gap 8: rx_pilot_kernel at NW = 1"),
    # ---- gap 4: the OMP correlation forms and their knobs (three-launch front end)
    *_both("omp-12taps-mfma", 2048, 512, 4, "16QAM", 2, T12, covers="gap 4: LDS-state pursuit, MFMA correlation (fp32)"),
    *_both("omp-fft-4096-regs", 4096, 1024, 2, "16QAM", 2, T3, covers="gap 4: comb_m = 2048, the by-transform form"),
    *_both("omp-fft-4096-12taps-regc0", 4096, 1024, 2, "QPSK", 2, T12, covers="gap 4: reg_c0"),
    Case("omp-fft-4096-12taps-k-gt-np", 4096, 1024, 2, "16QAM", 2, T12, k_atoms=520, covers="gap 4/8: K > Np + 1 turns reg_c0 off"),
    Case("omp-c0-lds", 4096, 1024, 2, "QPSK", 2, T12, env={"OFDM_OMP_C0_LDS": "1"}, base_env={}),
    Case("omp-no-fft", 4096, 1024, 2, "16QAM", 2, T3, env={"OFDM_OMP_NO_FFT": "1"}, base_env={}),
    # the switch replaces c0 by a 2048-point inverse transform with the direct dictionary sums: other summation order.  Bound: one
    # ulp (2.2e-16) per stage of the transform it replaces or per level of the pairwise sum (<= 13), times the gain of the 3-tap
    # refit (< 4) = 52 ulp = 1.2e-14; observed 9.99e-16
    Case("omp-no-fft-fp64", 4096, 1024, 2, "16QAM", 2, T3, precision="fp64", env={"OFDM_OMP_NO_FFT": "1"}, base_env={},
         h_tol64=1.2e-14),
    Case("omp-no-mfma", 2048, 512, 4, "16QAM", 2, T12, env={"OFDM_OMP_NO_MFMA": "1"}, base_env={}),
    Case("omp-unfused-fpw1", 1024, 256, 4, "16QAM", 2, T3, env={"OFDM_FAST_UNFUSED": "1", "OFDM_OMP_FPW": "1"},
         base_env={"OFDM_FAST_UNFUSED": "1"}, n_frames=11),
    Case("omp-unfused-fpw2", 1024, 256, 4, "16QAM", 2, T3, env={"OFDM_FAST_UNFUSED": "1", "OFDM_OMP_FPW": "2"},
         base_env={"OFDM_FAST_UNFUSED": "1"}, n_frames=11),
    Case("omp-unfused-fpw8-fp64", 1024, 256, 4, "16QAM", 2, T3, precision="fp64",
         env={"OFDM_FAST_UNFUSED": "1", "OFDM_OMP_FPW": "8"}, base_env={"OFDM_FAST_UNFUSED": "1"}, n_frames=11),
    Case("generic-forced-1024", 1024, 256, 4, "16QAM", 2, T3, env={"OFDM_CHAIN_GENERIC": "1"}, base_env={}),
    # ---- gap 5: the MMSE stage forms and their knobs
    Case("mmse-fused-wave", 2048, 512, 4, "64QAM", 3, T3, mode="mmse", mer=True, snr=24.0, covers="gap 5: one launch, np_pad <= 256"),
    Case("mmse-fused-wave-8psk", 2048, 256, 4, "8PSK", 3, T3, mode="mmse"),
    Case("mmse-two-launches", 2048, 512, 4, "64QAM", 3, T3, mode="mmse", env={"OFDM_MMSE_TWO_LAUNCHES": "1"}, base_env={}),
    Case("mmse-factored-natural", 4096, 1024, 2, "16QAM", 2, T3, mode="mmse", n_frames=9, covers="gap 5: np_pad 512 > 256"),
    Case("mmse-g1", 4096, 1024, 2, "16QAM", 2, T3, mode="mmse", n_frames=9, env={"OFDM_MMSE_G": "1"}, base_env={}),
    Case("mmse-g2", 4096, 1024, 2, "16QAM", 2, T3, mode="mmse", n_frames=9, env={"OFDM_MMSE_G": "2"}, base_env={}),
    Case("mmse-g8", 4096, 1024, 2, "16QAM", 2, T3, mode="mmse", n_frames=9, env={"OFDM_MMSE_G": "8"}, base_env={}),
    Case("mmse-dense-mfma", 2048, 512, 4, "64QAM", 3, T3, mode="mmse", env={"OFDM_MMSE_DENSE": "1"}, base_env={}),
    Case("mmse-no-mfma", 2048, 512, 4, "64QAM", 3, T3, mode="mmse", env={"OFDM_MMSE_NO_MFMA": "1"}, base_env={}),
    *_both("mmse-dense-scalar-np50", 1024, 400, 8, "16QAM", 3, T3, mode="mmse", covers="gap 5: Np % 4 != 0"),
    *_both("mmse-2048-unpruned-256qam", 2048, 1022, 8, "256QAM", 2, T3, mode="mmse", snr=36.0, covers="gap 3 in MMSE mode"),
    Case("mmse-descr-wave-pass", 2048, 512, 4, "QPSK", 3, T3, mode="mmse", descr=True,
         covers="DeScrambler + MMSE: the wave stage's HEXT build, then descr_pass_kernel"),
    Case("mmse-descr-four-wave", 2048, 512, 4, "QPSK", 3, T3, mode="mmse", descr=True, env={"OFDM_FAST_NO_WAVE": "1"},
         base_env={}, covers="DeScrambler + MMSE on rx_symbols_kernel's HEXT build"),
    # ---- gap 1(a): MMSE mode at Nfft 64 / 128 / 256 = the split form with the generic transform and pilot_ls_kernel
    *_both("split-mmse-64", 64, 32, 4, "QPSK", 3, (0, 2), mode="mmse", covers="gap 1a"),
    *_both("split-mmse-128-mer", 128, 64, 4, "16QAM", 3, T3, mode="mmse", mer=True, snr=24.0, covers="gap 1a"),
    *_both("split-mmse-256-descr", 256, 100, 4, "64QAM", 3, T3, mode="mmse", descr=True, covers="gap 1a, gap 7"),
    Case("split-mmse-256-odd-nc", 256, 63, 4, "256QAM", 2, T3, mode="mmse", snr=36.0, covers="gap 6: odd N_carrier -> scalar eq_demap"),
    # ---- gap 1(b): more than 48 Ki decisions per frame leaves the fast path; the generic kernel's LDS need sends it to split
    *_both("split-512-49k-decisions", 512, 384, 4, "QPSK", 171, T3, n_frames=3, covers="gap 1b"),
    # ---- Nfft 8192
    Case("coop4-64qam-mer", 8192, 1024, 4, "64QAM", 2, T3, mer=True, snr=24.0),
    Case("coop4-12taps-regc0", 8192, 1024, 4, "16QAM", 2, T12, covers="reg_c0 on the 8192 front end"),
    Case("coop4-mmse-qpsk", 8192, 512, 4, "QPSK", 2, T3, mode="mmse"),
    Case("coop4-256qam", 8192, 512, 4, "256QAM", 2, T3, snr=36.0),
    Case("r2-comb8-16qam", 8192, 600, 8, "16QAM", 2, T3),
    Case("r2-comb8-descr-16qam", 8192, 600, 8, "16QAM", 2, T3, descr=True, covers="gap 7: r2 + descr_pass_kernel"),
    Case("r2-descr-64qam", 8192, 1024, 4, "64QAM", 2, T3, descr=True, covers="gap 7: coop4 + descr_pass_kernel (the case keeps its name: the golden files key on it)"),
    Case("r2-percent-qpsk-mer", 8192, 600, 6, "QPSK", 2, T3, pilots=PCT, k_atoms=96, mer=True, snr=24.0, seed=8, covers="gap 8 at 8192"),
    Case("r2-mmse-256qam", 8192, 600, 8, "256QAM", 2, T3, mode="mmse", snr=36.0),
    Case("split-8192-wide", 8192, 2560, 8, "16QAM", 2, T3, n_frames=3, covers="gap 6: N_carrier > 2048 -> scalar eq_demap"),
    Case("split-8192-fp64-descr", 8192, 600, 8, "64QAM", 2, T3, precision="fp64", descr=True, covers="gap 7"),
    Case("split-8192-fp64-mmse-mer", 8192, 600, 8, "16QAM", 2, T3, precision="fp64", mode="mmse", mer=True, snr=24.0),
    Case("split-8192-fp64-16qam", 8192, 600, 8, "16QAM", 2, T3, precision="fp64"),
    Case("split-8192-fp64-qpsk", 8192, 600, 4, "QPSK", 2, T3, precision="fp64"),
    Case("split-8192-fp64-256qam", 8192, 300, 4, "256QAM", 2, T3, precision="fp64", snr=36.0),
    # ---- gap 6: switches without a natural route, each against the oracle and against the route without the switch
    Case("split-8192-vec-8psk-mer", 8192, 600, 8, "8PSK", 2, T3, env=NO8192, mer=True, snr=24.0),
    Case("split-8192-vec-64qam", 8192, 600, 8, "64QAM", 2, T3, env=NO8192),
    Case("split-8192-vec-256qam", 8192, 600, 8, "256QAM", 2, T3, env=NO8192, snr=36.0),
    Case("sw-no-coop", 8192, 1024, 4, "64QAM", 2, T3, env={"OFDM_SPLIT_NO_COOP": "1"}, base_env={}),
    Case("sw-no-r2", 8192, 600, 8, "16QAM", 2, T3, env={"OFDM_SPLIT_NO_R2": "1"}, base_env={}),
    Case("sw-eqd-scalar", 8192, 600, 8, "16QAM", 2, T3, env={**NO8192, "OFDM_EQD_SCALAR": "1"}, base_env=NO8192, covers="gap 6"),
    Case("sw-generic-fft", 8192, 600, 8, "16QAM", 2, T3, env={**NO8192, "OFDM_SPLIT_GENERIC_FFT": "1"}, base_env=NO8192, covers="gap 6"),
    Case("sw-no-pls-fuse", 8192, 600, 8, "16QAM", 2, T3, env={**NO8192, "OFDM_SPLIT_NO_PLS_FUSE": "1"}, base_env=NO8192, covers="gap 6"),
    Case("sw-all-rows", 8192, 600, 8, "16QAM", 2, T3, env={**NO8192, "OFDM_SPLIT_ALL_ROWS": "1"}, base_env=NO8192, covers="gap 6"),
    # another 8192-point transform algorithm (13 stages): the same 52 ulp = 1.2e-14 bound; observed 1.46e-16
    Case("sw-generic-fft-fp64", 8192, 600, 8, "16QAM", 2, T3, precision="fp64", env={"OFDM_SPLIT_GENERIC_FFT": "1"}, base_env={},
         h_tol64=1.2e-14),
    Case("sw-no-pls-fuse-fp64", 8192, 600, 8, "16QAM", 2, T3, precision="fp64", env={"OFDM_SPLIT_NO_PLS_FUSE": "1"}, base_env={}),
    Case("sw-all-rows-fp64", 8192, 600, 8, "16QAM", 2, T3, precision="fp64", env={"OFDM_SPLIT_ALL_ROWS": "1"}, base_env={}),
]

# The routes that must stay covered, one line each: (route, how it is reached -- "natural" = no switch set -- at which
# Nfft / N_carrier, and why it exists).  Left out because the predicates exclude them:
#   * fused front end with omp_state wave / c0 reg / omp_mfma / omp_scalar: rx_pilot_omp_kernel takes at most OMP_RT taps and
#     always correlates by its wave-local inverse transform (ofdm_chain_fast.hip, ofdm_chain_pilot.hip)
#   * c0 reg outside {omp_fft, wave}: reg_c0 needs both (ofdm_chain_fast.hip)
#   * wave / coop4 / r2 and eq_demap<vec> in fp64, omp_mfma and the three MFMA MMSE forms in fp64: fp32-only code
#   * descr in_kernel outside wave, and with MER (ofdm_chain.hip); coop4 and r2 never descramble themselves (descr pass)
#   * wave<exact> with MER (ofdm_chain_fast.hip sends it to rx_symbols<4,true>)
#   * generic with an MMSE estimator (refused, ofdm_chain.hip); generic has no separate estimator launch at all
#   * demod8192+pls and demod_generic+pls with coop4 / r2 (their front end is always demod8192, ofdm_chain_split.hip)
def _G(ba, descr, mer):
    return Route("generic", "fused", "omp_scalar", "-", "-", "chain_generic", ba, descr, mer)


def _FU(fpw, symbols, ba, descr="none", mer=False):
    return Route("fast", "fused", "omp_fft", f"regs<fpw={fpw}>", "lds", symbols, ba, descr, mer)


def _FO(est, state, c0, symbols, ba, descr="none", mer=False):
    return Route("fast", "pilot+omp", est, state, c0, symbols, ba, descr, mer)


def _S(front, est, state, c0, symbols, ba, descr="none", mer=False):
    return Route("split", front, est, state, c0, symbols, ba, descr, mer)


def _rg(n):
    return f"regs<fpw={n}>"


_SV, _SS, _GEN, _D8 = "eq_demap<vec>", "eq_demap<scalar>", "demod_generic+pls", "demod8192"

# Knowingly left out of the list (the table test asserts these pairs per kernel FAMILY only): the slicer order BA and the
# estimator are template / launch parameters independent of NW, PRUNE2 and the wave skip form, so not every
# (rx_symbols<NW,PRUNE2>, ba), (wave<form>, ba) and (instantiation, estimator) pair is listed -- each NW x PRUNE2 and each
# wave form appears with at least one BA, each BA with at least one of them.  Nothing but reading the templates supports
# that independence.
# (route, why it exists, the precisions in which it exists and must be covered)
ROUTES = [
    # ---- entry generic: rx_chain_kernel does everything (ofdm_chain.hip).  Taken when neither fast nor split applies
    (_G(0, "pass", False), "Nfft < 512 is below the fast path (ofdm_chain_fast.hip); a DeScrambler plan hands raw decisions to descr_pass_kernel (ofdm_chain.hip); table-search slicer", "both"),
    (_G(2, "none", True), "Nfft < 512, MER instantiation rx_chain_kernel<T, N, MerSums> (ofdm_chain.hip); 2 bits per axis", "both"),
    (_G(3, "none", False), "Nfft < 512, 3 bits per axis, nd % 32 != 0", "both"),
    (_G(4, "none", False), "Nfft < 512, 4 bits per axis", "both"),
    (_G(2, "pass", False), "a pilot outside 1..N_carrier clears pilots_in_band (ofdm_chain.hip) and bars fast and split ; DeScrambler plan", "both"),
    (_G(2, "none", False), "OFDM_CHAIN_GENERIC at a fast-path size (ofdm_chain_fast.hip, ofdm_chain_split.hip)", "fp32"),
    (_G(3, "none", True), "out-of-band pilot at a fast-path Nfft (2048) with MER", "fp32"),
    # ---- entry fast, fused front end: comb pilots with Nfft/comb | 512, <= OMP_RT taps, K <= 512 (ofdm_chain_fast.hip);
    #      the pursuit's frames per wavefront follow from max(Np, K) (ofdm_chain_pilot.hip); symbol stage
    #      rx_symbols_kernel<NW = Nfft/512, PRUNE2 = N_carrier <= 128 NW> 
    (_FU(4, "rx_symbols<1,true>", 0), "Nfft 512, N_carrier <= 128", "both"),
    (_FU(1, "rx_symbols<1,true>", 2), "OFDM_PILOT_FPW = 1 (ofdm_chain_pilot.hip): one frame per wavefront in the fused launch", "fp32"),
    (_FU(4, "rx_symbols<1,false>", 2, mer=True), "Nfft 512, N_carrier > 128: un-pruned 512-point transform; MER variant", "both"),
    (_FU(4, "rx_symbols<2,true>", 3), "Nfft 1024, N_carrier <= 256", "both"),
    (_FU(4, "rx_symbols<2,false>", 4, "pass"), "Nfft 1024, N_carrier > 256; DeScrambler outside the wave stage = descr_pass_kernel (ofdm_chain.hip)", "both"),
    (_FU(1, "rx_symbols<4,true>", 3), "Nfft 2048, N_carrier <= 512 in fp64: the wave stage is fp32 only (ofdm_chain_wave.hip)", "fp64"),
    (_FU(2, "rx_symbols<4,true>", 3), "the same geometry in fp32 under OFDM_FAST_NO_WAVE (ofdm_chain_wave.hip)", "fp32"),
    (_FU(2, "rx_symbols<4,false>", 2), "Nfft 2048, N_carrier > 512 (PRUNE2 = false at NW = 4), fp32", "fp32"),
    (_FU(1, "rx_symbols<4,false>", 2), "the same in fp64 (the Y buffer of a group halves the frames per wavefront)", "fp64"),
    (_FU(1, "rx_symbols<8,false>", 3, mer=True), "Nfft 4096, N_carrier > 1024 (PRUNE2 = false at NW = 8); MER variant", "both"),
    (_FU(1, "rx_symbols<8,true>", 0), "Nfft 4096, N_carrier <= 1024", "both"),
    # wave-per-frame symbol stage: Nfft 2048, fp32, N_carrier <= 512, frame fits wave_layout (ofdm_chain_wave.hip)
    (_FU(2, "wave<skip0>", 3), "comb 4: no data carrier = 0 mod 4, one of four rounds skipped (ofdm_chain_wave.hip); the benchmark route", "fp32"),
    (_FU(2, "wave<skip0>", 0, "in_kernel"), "DeScrambler in the wave kernel's pack stage (the DeScrambler builds of chain_wave_symbols_run, ofdm_chain_wave.hip)", "fp32"),
    (_FU(2, "wave<skip0>", 2, "pass", True), "DeScrambler + MER: the wave MER variants do not descramble (ofdm_chain.hip, ofdm_chain_wave.hip)", "fp32"),
    (_FU(4, "wave<none>", 4), "comb 8: data on every residue class, no round skipped", "fp32"),
    (_FU(2, "wave<none>", 2), "OFDM_WAVE_NO_SKIP on a comb-4 plan (ofdm_chain_wave.hip)", "fp32"),
    (_FU(2, "wave<exact>", 3), "OFDM_WAVE_EXACT_SLICER: the threshold-count slicer build (ofdm_chain_wave.hip)", "fp32"),
    # ---- entry fast, three-launch front end (rx_pilot_kernel, then omp_batch_kernel or the MMSE stage): any other layout,
    #      more than OMP_RT taps, K > 512, MMSE mode, or OFDM_FAST_UNFUSED
    (_FO("omp_scalar", _rg(4), "lds", "wave<skip02>", 2, mer=True), "comb 2 at Nfft 2048: Nfft/comb = 1024 > 512 is not a fused layout; data on odd residues only -> two rounds skipped (ofdm_chain_wave.hip); K = Np = 100 is no multiple of 16 -> scalar correlation", "fp32"),
    (_FO("omp_scalar", _rg(4), "lds", "wave<none>", 3), "percent layout (comb_m = 0) with K < Np, K % 16 != 0", "fp32"),
    (_FO("omp_scalar", _rg(4), "lds", "rx_symbols<4,false>", 3), "the Task-4 percent layout at its own size (2048 / 800)", "both"),
    (_FO("omp_scalar", _rg(4), "lds", "rx_symbols<2,false>", 2), "percent layout with K > Np + 1", "both"),
    (_FO("omp_scalar", _rg(4), "lds", "rx_symbols<1,false>", 0), "percent layout at Nfft 512: rx_pilot_kernel at NW = 1", "both"),
    (_FO("omp_mfma", "wave", "lds", "wave<skip0>", 2), "more than OMP_RT taps: one frame per wavefront, R state in LDS (ofdm_chain_fast.hip); fp32, K % 16 == 0, Np % 4 == 0 -> MFMA correlation ", "fp32"),
    (_FO("omp_scalar", "wave", "lds", "rx_symbols<4,true>", 2), "the same plan in fp64: no MFMA form , no wave stage", "fp64"),
    (_FO("omp_scalar", "wave", "lds", "wave<skip0>", 2), "OFDM_OMP_NO_MFMA on the fp32 plan", "fp32"),
    (_FO("omp_fft", _rg(2), "lds", "rx_symbols<8,true>", 2), "comb 2 at Nfft 4096: comb_m = 2048 -> c0 by a 2048-point inverse transform (ofdm_chain_fast.hip); fp32", "fp32"),
    (_FO("omp_fft", _rg(1), "lds", "rx_symbols<8,true>", 2), "the same in fp64 (96 KiB rule halves the frames per wavefront)", "fp64"),
    (_FO("omp_fft", "wave", "reg", "rx_symbols<8,true>", 0), "by-transform + more than OMP_RT taps + K <= 512, K <= Np + 1: c0 in registers (ofdm_chain_fast.hip)", "both"),
    (_FO("omp_fft", "wave", "lds", "rx_symbols<8,true>", 2), "K > Np + 1: c0 stays in LDS ", "fp32"),
    (_FO("omp_fft", "wave", "lds", "rx_symbols<8,true>", 0), "OFDM_OMP_C0_LDS on a reg_c0 plan ", "fp32"),
    (_FO("omp_mfma", _rg(2), "lds", "rx_symbols<8,true>", 2), "OFDM_OMP_NO_FFT on the comb_m = 2048 plan, fp32: MFMA correlation", "fp32"),
    (_FO("omp_scalar", _rg(1), "lds", "rx_symbols<8,true>", 2), "OFDM_OMP_NO_FFT in fp64: scalar correlation", "fp64"),
    (_FO("omp_mfma", _rg(1), "lds", "rx_symbols<2,true>", 2), "OFDM_OMP_FPW = 1 (ofdm_chain_fast.hip) on the forced three-launch form", "fp32"),
    (_FO("omp_mfma", _rg(2), "lds", "rx_symbols<2,true>", 2), "OFDM_OMP_FPW = 2", "fp32"),
    (_FO("omp_scalar", _rg(8), "lds", "rx_symbols<2,true>", 2), "OFDM_OMP_FPW = 8 (fp64)", "fp64"),
    # MMSE mode on the fast path (always three launches): ofdm_chain_mmse.hip
    (_FO("mmse_fused", "-", "-", "wave<skip0>", 3, mer=True), "fp32, Np % 4 == 0, np_pad <= 256: both factors in one launch ; HEXT build of the wave kernel, MER", "fp32"),
    (_FO("mmse_fused", "-", "-", "wave<skip0>", 0), "the same with the table-search slicer", "fp32"),
    (_FO("mmse_fused", "-", "-", "wave<skip0>", 0, "pass"), "DeScrambler + MMSE: ofdm_chain.hip clears the view's DeScrambler, so launch_fast still takes the wave stage (the kernel trace shows it; the comment at ofdm_chain_wave.hip says otherwise)", "fp32"),
    (_FO("mmse_fused", "-", "-", "rx_symbols<4,true>", 0, "pass"), "the same under OFDM_FAST_NO_WAVE: rx_symbols_kernel's HEXT build with descr_pass_kernel", "fp32"),
    (_FO("mmse_fused", "-", "-", "rx_symbols<4,false>", 4), "MMSE at PRUNE2 = false, NW = 4", "fp32"),
    (_FO("mmse_factored<G=4>", "-", "-", "wave<skip0>", 3), "OFDM_MMSE_TWO_LAUNCHES ", "fp32"),
    (_FO("mmse_factored<G=4>", "-", "-", "rx_symbols<8,true>", 2), "np_pad = 512 > 256: two launches are the natural form, default tile G = 4 ", "fp32"),
    (_FO("mmse_factored<G=1>", "-", "-", "rx_symbols<8,true>", 2), "OFDM_MMSE_G = 1 : mmse_apply_mfma_kernel<1>", "fp32"),
    (_FO("mmse_factored<G=2>", "-", "-", "rx_symbols<8,true>", 2), "OFDM_MMSE_G = 2", "fp32"),
    (_FO("mmse_factored<G=8>", "-", "-", "rx_symbols<8,true>", 2), "OFDM_MMSE_G = 8", "fp32"),
    (_FO("mmse_dense_mfma", "-", "-", "wave<skip0>", 3), "OFDM_MMSE_DENSE : the dense operator on the matrix cores ", "fp32"),
    (_FO("mmse_dense_scalar", "-", "-", "wave<skip0>", 3), "OFDM_MMSE_NO_MFMA ", "fp32"),
    (_FO("mmse_dense_scalar", "-", "-", "rx_symbols<2,false>", 2), "Np % 4 != 0 (fp32), and every fp64 plan: mmse_apply_valu_kernel ", "both"),
    (_FO("mmse_dense_scalar", "-", "-", "rx_symbols<4,false>", 4), "fp64 MMSE at PRUNE2 = false, NW = 4", "fp64"),
    # ---- entry split (ofdm_chain.hip): MMSE mode outside the fast path, > 48 Ki decisions + generic LDS need > 158 KiB, Nfft 8192
    (_S(_GEN, "mmse_fused", "-", "-", _SV, 0), "MMSE at Nfft 64 (fp32): demod_keep_device + pilot_ls_kernel (ofdm_chain_split.hip), vector eq_demap (even N_carrier)", "fp32"),
    (_S(_GEN, "mmse_dense_scalar", "-", "-", _SS, 0), "the same in fp64: scalar eq_demap is the only fp64 form", "fp64"),
    (_S(_GEN, "mmse_fused", "-", "-", _SV, 2, mer=True), "MMSE at Nfft 128 with MER (eq_demap_kernel<.., MerOut>)", "fp32"),
    (_S(_GEN, "mmse_dense_scalar", "-", "-", _SS, 2, mer=True), "the same in fp64", "fp64"),
    (_S(_GEN, "mmse_dense_scalar", "-", "-", _SV, 3, "pass"), "MMSE at Nfft 256 with Np = 25 (not a multiple of 4) and a DeScrambler plan", "fp32"),
    (_S(_GEN, "mmse_dense_scalar", "-", "-", _SS, 3, "pass"), "the same in fp64", "fp64"),
    (_S(_GEN, "mmse_fused", "-", "-", _SS, 4), "odd N_carrier: the natural route of the fp32 scalar eq_demap ", "fp32"),
    (_S(_GEN, "omp_mfma", _rg(4), "lds", _SV, 0), "Nfft 512 with more than 48 Ki decisions (ofdm_chain_fast.hip) whose generic LDS need exceeds 158 KiB (ofdm_chain.hip); fp32", "fp32"),
    (_S(_GEN, "omp_scalar", _rg(4), "lds", _SS, 0), "the same in fp64", "fp64"),
    (_S(_D8, "omp_fft", _rg(4), "lds", "coop4", 3, mer=True), "Nfft 8192 fp32, comb 4 (no data = 0 mod 4), nd % 32 == 0, K <= 512 (ofdm_chain_coop.hip); comb_m = 2048 -> by-transform OMP; MER", "fp32"),
    (_S(_D8, "omp_fft", "wave", "reg", "coop4", 2), "the same front end with more than OMP_RT taps: reg_c0 at 8192 (the C5 benchmark's form)", "fp32"),
    (_S(_D8, "mmse_fused", "-", "-", "coop4", 0), "coop4 in MMSE mode (HEXT), table-search slicer", "fp32"),
    (_S(_D8, "omp_fft", _rg(4), "lds", "coop4", 4), "coop4 with 4 bits per axis", "fp32"),
    (_S(_D8, "omp_scalar", _rg(4), "lds", "r2", 2, "pass"), "the same plan with a DeScrambler: r2 hands raw decisions to descr_pass_kernel", "fp32"),
    (_S(_D8, "omp_scalar", _rg(4), "lds", "r2", 2), "comb 8 at 8192: data = 0 mod 4 exists, coop4 refuses, rx_symbols_r2_kernel takes it (ofdm_chain_split.hip)", "fp32"),
    (_S(_D8, "omp_fft", _rg(4), "lds", "coop4", 3, "pass"), "a DeScrambler plan on coop4: the stage hands raw decisions to descr_pass_kernel (the receiver clears the view's DeScrambler before the split form runs, so coop4 never saw one: the parent's outputs, tests/golden/chain_routes_parent.json)", "fp32"),
    (_S(_D8, "omp_fft", _rg(4), "lds", "r2", 3), "OFDM_SPLIT_NO_COOP on a coop4 plan", "fp32"),
    (_S(_D8, "omp_scalar", _rg(4), "lds", "r2", 0, mer=True), "percent layout at 8192 with MER", "fp32"),
    (_S(_D8, "mmse_dense_scalar", "-", "-", "r2", 4), "r2 in MMSE mode, Np = 75", "fp32"),
    (_S(_D8, "omp_mfma", _rg(4), "lds", _SS, 2), "Nfft 8192 fp32 with N_carrier > 2048: neither coop4 nor r2, and no vector eq_demap (ofdm_chain_split.hip)", "fp32"),
    (_S(_D8, "omp_scalar", _rg(4), "lds", _SS, 3, "pass"), "every fp64 plan at 8192: demod_keep8192 with fused pilot LS (ofdm_chain_split.hip); DeScrambler", "fp64"),
    (_S(_D8, "mmse_dense_scalar", "-", "-", _SS, 2, mer=True), "fp64 MMSE at 8192 with MER", "fp64"),
    (_S(_D8, "omp_fft", _rg(4), "lds", _SS, 0), "fp64 comb 4 at 8192: by-transform OMP in double", "fp64"),
    (_S(_D8, "omp_fft", _rg(4), "lds", _SS, 4), "the same with 4 bits per axis (demap_square_lut, ofdm_chain_split.hip)", "fp64"),
    (_S(_D8, "omp_scalar", _rg(4), "lds", _SV, 2), "OFDM_SPLIT_NO_R2 (and NO_COOP): the fp32 split form at 8192 with the vector eq_demap", "fp32"),
    (_S(_D8, "omp_scalar", _rg(4), "lds", _SV, 0, mer=True), "the same, table-search slicer, MER", "fp32"),
    (_S(_D8, "omp_scalar", _rg(4), "lds", _SV, 3), "the same, 3 bits per axis", "fp32"),
    (_S(_D8, "omp_scalar", _rg(4), "lds", _SV, 4), "the same, 4 bits per axis", "fp32"),
    (_S(_D8, "omp_scalar", _rg(4), "lds", _SS, 2), "OFDM_EQD_SCALAR (ofdm_chain_split.hip), fp32; also the fp64 base route of the split switches", "both"),
    (_S(_GEN, "omp_scalar", _rg(4), "lds", _SV, 2), "OFDM_SPLIT_GENERIC_FFT : demod_keep_device + pilot_ls_kernel at 8192, fp32", "fp32"),
    (_S(_GEN, "omp_scalar", _rg(4), "lds", _SS, 2), "the same in fp64", "fp64"),
    (_S("demod8192+pls", "omp_scalar", _rg(4), "lds", _SV, 2), "OFDM_SPLIT_NO_PLS_FUSE : demod_keep8192 without pilot LS, then pilot_ls_kernel; fp32", "fp32"),
    (_S("demod8192+pls", "omp_scalar", _rg(4), "lds", _SS, 2), "the same in fp64", "fp64"),
    (_S("demod8192<all_rows>", "omp_scalar", _rg(4), "lds", _SV, 2), "OFDM_SPLIT_ALL_ROWS : pilot-only sub-transform rows are computed on data symbols too; fp32", "fp32"),
    (_S("demod8192<all_rows>", "omp_scalar", _rg(4), "lds", _SS, 2), "the same in fp64", "fp64"),
]

# Excluded from the table by name:
#   *_WG_PER_CU   resident-workgroup overrides: they change the grid size of a persistent kernel, not which code runs
#   OFDM_T4_*     switches of the Task-4 receiver (read in t4_route.hpp; tests/t4_routes.py and test_t4_route_host.py audit them), not of this dispatcher
#   OFDM_WAVE_ABL read only under #ifdef OFDM_DIAG (ofdm_chain_wave.hip): the shipped library does not contain it
EXCLUDED_SWITCHES = (re.compile(r"_WG_PER_CU$"), re.compile(r"^OFDM_T4_"), re.compile(r"^OFDM_WAVE_ABL$"))


def dispatch_switches(csrc=None, excluded=False):
    """Every OFDM_* name that getenv reads in the six dispatch files, minus the exclusions (excluded=True: with them)."""
    csrc = csrc or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ofdm-course_amd", "csrc")
    names = set()
    for fn in DISPATCH_FILES:
        with open(os.path.join(csrc, fn)) as fh:
            names.update(re.findall(r'getenv\("(OFDM_[A-Z0-9_]+)"\)', fh.read()))
    return {n for n in names if excluded or not any(p.search(n) for p in EXCLUDED_SWITCHES)}


def table_switches():
    return {k for c in CASES for k in c.env} - set(EXTRA_SWITCHES)


# Host-side refusals: (case, refusal id).  The case is never launched; see test_gpu_chain_routes.py.
REFUSALS: list[Case] = [
    Case("refuse-mmse-oob", 256, 64, 4, "16QAM", 3, T3, pilots=("extra", 80), mode="mmse", n_frames=2),           # ofdm_chain.hip
    # the generic kernel forced onto a frame whose decisions do not fit its LDS (the natural route of this frame is split)
    Case("refuse-generic-lds", 512, 384, 4, "QPSK", 171, T3, env={"OFDM_CHAIN_GENERIC": "1"}, n_frames=2),          # ofdm_chain.hip
    # fp64, Np = 1024, K = 1500: 4 frames of Y + c0 = 161.6 KB in the OMP stage (MMSE mode of the same plan does not use it)
    Case("refuse-omp-lds", 4096, 4096, 4, "QPSK", 1, T3, precision="fp64", k_atoms=1500, n_frames=2),               # ofdm_chain_fast.hip
]
# what test_route_refusals changes before it calls the same plan again
REFUSAL_FOLLOW_UP = {"refuse-mmse-oob": dict(mode="omp"), "refuse-generic-lds": dict(env={}),
                     "refuse-omp-lds": dict(env={"OFDM_CHAIN_GENERIC": "1"})}
REFUSAL_IDS = {"refuse-mmse-oob": "mmse_entry", "refuse-generic-lds": "generic_lds", "refuse-omp-lds": "omp_lds"}


# ---------------------------------------------------------------------------------------------------------------------
# tie-free inputs: the oracle's own pursuit on the Philox frames of a case (CPU)
# ---------------------------------------------------------------------------------------------------------------------
REG = (1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0)          # T5/Main_model_Task_5.m:55


def oracle_frames(case, oracle):
    """The case's frames from the oracle alone: (rx [frame_samples, n_frames] complex128, bits [n_frames, frame_bits])."""
    D, bps = oracle.constellation_func(case.const)
    pc, dc = case.pilot_carriers().astype(np.float64), case.data_carriers().astype(np.float64)
    amp = 2.0 * np.max(np.abs(D))                                         # frames.pilot_column
    pv_col = np.where(np.arange(pc.size) % 2 == 0, amp, -amp).astype(np.complex128)
    pv = np.repeat(pv_col[:, None], case.n_symb, axis=1)
    h, _ = oracle.get_MP_channel_resp(case.taps, case.nfft)
    tg = case.nfft // 8
    rx, bits = [], []
    for f in range(case.n_frames):
        b = oracle.payload_bits_philox(dc.size * case.n_symb, bps, case.seed, f)
        noise = oracle.awgn_philox((case.nfft + tg) * case.n_symb, case.seed, f)
        y, _ = oracle.tx_frame(b, case.nfft, tg, case.n_symb, dc, pc, pv, case.const, h=h, SNR=case.snr, noise=noise,
                               Register=REG if case.descr else None, noise_first=True)
        rx.append(y)
        bits.append(b)
    return np.stack(rx, axis=1), np.stack(bits), pv_col


def oracle_min_gap(case, oracle):
    """Smallest (best - second) / best over every pick of every frame of OMP_estimate.m:7-23 on the case's frames."""
    rx, _, pv_col = oracle_frames(case, oracle)
    S = oracle.sensing_matrix(case.pilot_carriers().astype(np.float64), case.nfft, case.K)
    pc0 = case.pilot_carriers() - 1
    L = case.nfft + case.nfft // 8
    worst = 1.0
    for f in range(case.n_frames):
        X1 = oracle.OFDM_demodulator(rx[:L, f][:, None], case.nfft // 8)
        y = X1[pc0, 0] / pv_col
        idx, r = [], y.copy()
        for it in range(len(case.delays)):
            sc = np.sort(np.abs(S.conj().T @ r))
            worst = min(worst, float((sc[-1] - sc[-2]) / sc[-1]))
            idx.append(int(np.argmax(np.abs(S.conj().T @ r))))
            A = S[:, idx]
            r_new = y - A @ (oracle._pinv_matlab(A) @ y)
            stop = it > 0 and np.linalg.norm(r_new - r) / np.linalg.norm(r) < 1e-2      # OMP_estimate.m:20
            r = r_new
            if stop:
                break
        # the replay above is the oracle's own pursuit: same picks, same stop
        assert [k + 1 for k in idx] == list(oracle.OMP_estimate(y, S, case.nfft, len(case.delays))[2]), (case.name, f)
    return worst


# Smallest top-2 gap of the oracle's pursuit per fp32 OMP case, as printed by `python tests/routes.py` (seed = the case's
# `seed`).  Every one is far above the 1e-4 near-tie threshold, and above the 2e-6 by which the fp32 frames differ from the
# oracle's (test_gpu_txgen.py): no case sets a frame aside.  test_route_table.py checks that the list is complete.
GAPS: dict[str, float] = {
    "fast-percent-512-fp32": 0.202,
    "generic-64-qpsk-descr-fp32": 0.254,
    "generic-128-16qam-mer-fp32": 0.231,
    "generic-256-64qam-fp32": 0.189,
    "generic-256-256qam-fp32": 0.0283,
    "generic-oob-256-descr-fp32": 0.0647,
    "generic-oob-2048-mer": 0.00137,
    "fast-512-pruned-fp32": 0.035,
    "fast-512-unpruned-mer-fp32": 0.185,
    "fast-1024-pruned-fp32": 0.0312,
    "fast-1024-unpruned-descr-fp32": 0.198,
    "fast-2048-pruned-nowave": 0.0288,
    "fast-512-pilot-fpw": 0.0351,
    "fast-2048-unpruned-fp32": 0.199,
    "fast-4096-unpruned-mer-fp32": 0.135,
    "fast-4096-pruned-fp32": 0.0288,
    "wave-skip0-64qam": 0.0288,
    "wave-skip0-qpsk-descr": 0.0386,
    "wave-skip02-16qam-mer": 0.00129,
    "wave-none-256qam": 0.00818,
    "wave-exact-64qam": 0.0288,
    "wave-noskip-16qam": 0.0288,
    "wave-descr-mer-pass": 0.0285,
    "wave-percent-k-scalar": 0.0334,
    "fast-percent-2048-fp32": 0.201,
    "fast-percent-1024-k-gt-np-fp32": 0.0892,
    "omp-12taps-mfma-fp32": 0.0045,
    "omp-fft-4096-regs-fp32": 0.0268,
    "omp-fft-4096-12taps-regc0-fp32": 0.00161,
    "omp-fft-4096-12taps-k-gt-np": 0.00176,
    "omp-c0-lds": 0.00161,
    "omp-no-fft": 0.0268,
    "omp-no-mfma": 0.0045,
    "omp-unfused-fpw1": 0.0309,
    "omp-unfused-fpw2": 0.0309,
    "generic-forced-1024": 0.0312,
    "split-512-49k-decisions-fp32": 0.278,
    "coop4-64qam-mer": 0.00373,
    "coop4-12taps-regc0": 0.00149,
    "coop4-256qam": 0.00184,
    "r2-comb8-16qam": 0.00133,
    "r2-comb8-descr-16qam": 0.00133,
    "r2-descr-64qam": 0.00427,
    "r2-percent-qpsk-mer": 0.00147,
    "split-8192-wide": 0.0968,
    "split-8192-vec-8psk-mer": 0.00158,
    "split-8192-vec-64qam": 0.00132,
    "split-8192-vec-256qam": 0.00123,
    "sw-no-coop": 0.00427,
    "sw-no-r2": 0.00133,
    "sw-eqd-scalar": 0.00133,
    "sw-generic-fft": 0.00133,
    "sw-no-pls-fuse": 0.00133,
    "sw-all-rows": 0.00133,
}


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import ofdm_oracle
    for c in CASES:
        if c.precision == "fp32" and c.mode == "omp":
            print(f'    "{c.name}": {oracle_min_gap(c, ofdm_oracle):.3g},', flush=True)
