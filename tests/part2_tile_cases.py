"""Cases of the per-realisation tests of the two Task-5 study tiles (csrc/ofdm_part2.hip: ofdm_task5_part2_tile, ofdm_task5_mse_tile)
and their replay on the oracle, made on the CPU alone.  TEST INFRASTRUCTURE: no GPU, no HIP.

The drivers add a tile's results over its realisations before anything is compared; here every realisation keeps its own slot:
oracle_tile returns nmse[4, F] and errors[4, F] (rows LS, MMSE, MP, OMP) of drivers/task5_part2.py:102-124 call by call on
OracleLib, oracle_mse_tile the four errors per SNR point of drivers/task5.py:102-109.  Every realisation has its own channel
(fading_taps with a distinct seed), so a result in the wrong slot, or one evaluated against a neighbour's channel, shows.

Every case is the smallest frame that reaches its kernel variant (N_symb = 2, T_guard = Nfft / 8, 16QAM, SNR 20 dB), and its first
F puts a full workgroup in front of a ragged one for every split of the tile:
    P2_FT = 8 realisations per workgroup (p2_apply_operator_kernel), FB = 4 fpw in {16, 8, 4} (mp_batch_kernel), 4 / 2 / 1
    wavefronts per workgroup (mmse_wave_kernel), 8-realisation column groups (corr_mfma_f32), one workgroup per realisation
    (fir_multi_kernel, p2_nmse_kernel).

  case  Nfft / N_carrier / pilots / K           F      what it reaches
  A     256 / 128 / comb 4 (Np 32) / 64         37, 1  fpw 4 in both precisions, MFMA MP with 2 tiles and two column groups;
                                                       37 = 2 16 + 5 = 4 8 + 5 = 9 4 + 1.  ETU: 9 paths, the OMP stage is omp_frame_wave
  A7    the same with EPA (7 paths)             37     the register-resident OMP under the same F
  AV    A's shape, ETU at 20 / 22 / 24 MHz      21     the nine delays differ from one realisation to the next (a delay profile
                                                       fixes them at one sampling rate): p2_nmse_kernel and fir_multi_kernel
                                                       must read every realisation's own delays
  B     256 / 192 / comb 4 (Np 48) / 64         21     odd tile count (3): `two == false` in corr_mfma_f32; N_carrier = 128 + 64
  C     256 / 100 / random mask Np 18 / 256     19     np % 4 != 0: fp32 takes the scalar MP; Np no multiple of 8 (operator tail);
                                                       N_carrier < 128; all Nfft delays; ETU's last path (delay 100) is not inside
                                                       1..N_carrier: the tile's delay-spread rule skips it
  D     1024 / 640 / comb 4 (Np 160) / 256      21     fp64 fpw 2 (FB 8); fp32 fpw 4 with 10 tiles
  E     1024 / 640 / random mask Np 320 / 1024  13     fp64 fpw 1 (FB 4); fp32 fpw 2: MFMA with FB 8, one column group
  F     1024 / 640 / random mask Np 576 / 1024  9      fp32 only: fpw 1, MFMA with FB 4 (half a column group), 36 tiles
A-C use ETU at 20 MHz (9 distinct paths), A7 and D-F EPA at 100 MHz (7 distinct paths); every case keeps Np >= paths (below that
OMP_estimate.m:17 is a rank-deficient pinv, test_gpu_part2_tile.py).  No shape had to move: the library serves all of them
(tests/test_part2_tile_cases_host.py works that out from mp_layout, omp_layout and chain_split_fits).

  M1    A's layout, constant pilots, fp64 + fp32   37 SNRs 0..30 dB   every per-point stage across workgroup bounds, inv_snr_v[f]
  M2    2048 / 1280 / comb 1 (Np 1280) / 2048, fp32   5 points        wpw = 1 in mmse_wave_kernel (Np > 1200), MFMA MP with FB 4 and
                                                                      80 tiles, mse_tau_kernel at an N_carrier that is no power of two
  M3    M1's layout, fp64, 5 points    channel_taps with two rows at delay 10 (the later wins, get_MP_channel_resp.m:12-14) and one
                                       at delay 150 >= N_carrier

Margins.  The exact fp64 assertions hold where the oracle's own decisions are not within rounding of a tie: per realisation the
smallest relative gap between the best and the second-best score over the MP and the OMP iterations, and the smallest distance
of an equalised data point to a 16QAM decision boundary in units of the grid step.  The seeds below were chosen on the oracle
alone such that every realisation clears 1e-6 in both; a realisation whose smallest pick gap is below 1e-3 (the fp32 NMSE
tolerance of the project) is `fp32_loose`: at most 10 % of a case, never a workgroup's first or last slot.
`python tests/part2_tile_cases.py` prints all of them."""
from __future__ import annotations

import dataclasses
import math

import numpy as np

from omp_wide_cases import pursuit_min_gap
from oracle_lib import OracleLib

N_SYMB = 2
CONSTELLATION = "16QAM"
SNR_DB = 20.0
PROFILE_RATE = {"ETU": 2e7, "EPA": 1e8}          # sampling rates at which the table delays round to distinct samples
PROFILE_PATHS = {"ETU": 9, "EPA": 7}
FP64_GAP = 1e-6
FP32_GAP = 1e-3
P2_FT = 8                                        # ofdm_part2.hip
OMP_RT = 8                                       # chain_fast_core.hpp


def mp_fpw(np_, taps, f64):
    """mp_layout (ofdm_part2.hip): realisations per wavefront of mp_batch_kernel; kc = Np."""
    cs = 16 if f64 else 8
    fpw = 4
    while fpw > 1 and cs * 4 * fpw * (np_ + 1 + np_) + 4 * 4 * fpw * taps > 72 * 1024:
        fpw >>= 1
    return fpw


def mp_lds_bytes(np_, taps, f64):
    cs = 16 if f64 else 8
    fb = 4 * mp_fpw(np_, taps, f64)
    a16 = lambda v: (v + 15) & ~15                                                  # noqa: E731
    return a16(cs * fb * (np_ + 1)) + a16(cs * fb * np_) + a16(4 * fb * taps)


def mp_mfma(np_, f64):
    """part2_tile_run: the matrix-core MP (kc = Np columns in 16-atom tiles, 4 pilots per k-step)."""
    return (not f64) and np_ % 16 == 0 and np_ % 4 == 0


def mmse_wpw(np_, sweep):
    """Wavefronts per workgroup of mmse_wave_kernel: 4 in the part-2 tile, as many as fit in the MSE tile."""
    wpw = 4
    while sweep and wpw > 1 and 16 * 4 * np_ * wpw > 150 * 1024:
        wpw >>= 1
    return wpw


@dataclasses.dataclass(frozen=True)
class TileCase:
    name: str
    nfft: int
    n_carrier: int
    pilots: tuple          # ("comb", step) or ("mask", Np): sort(randperm(N_carrier, Np)) of drivers.task5_part2
    K: int
    F: tuple               # realisations per tile call; F[0] is the replayed tile, the others are its prefixes
    profile: str
    seed: int
    precisions: tuple = ("fp64", "fp32")
    fpw: tuple = (4, 4)    # (fp64, fp32) of mp_batch_kernel, as the table above claims
    tiles: int = 0         # 16-atom tiles of the fp32 matrix-core MP, 0 = the scalar MP
    omp: str = "wave"      # omp_batch_kernel's form: "wave" (more than OMP_RT paths) or "regs"
    rates: tuple = ()      # sampling rates dealt round-robin over the realisations; () = PROFILE_RATE of the profile

    @property
    def t_guard(self):
        return self.nfft // 8

    @property
    def paths(self):
        return PROFILE_PATHS[self.profile]

    def layout(self):
        """(pilotCarriers, dataCarriers), 1-based float64."""
        from ofdm_course_amd.drivers import common as c
        from ofdm_course_amd.drivers import task5_part2 as p2
        if self.pilots[0] == "comb":
            _, pc, dc = c.layout_comb(self.nfft, self.n_carrier, self.pilots[1])
        else:
            _, pc, dc, step = p2.random_pilot_layout(self.nfft, self.n_carrier, self.pilots[1], [self.seed, 7])
            assert step != 1, "the mask's second and third pilot are neighbours: the driver would switch to the 100 % rule"
        return pc, dc

    @property
    def n_pilots(self):
        return self.n_carrier // self.pilots[1] if self.pilots[0] == "comb" else self.pilots[1]

    def taps_list(self):
        """F[0] channel draws, every one from its own seed."""
        from ofdm_course_amd.drivers import common as c
        rng = np.random.Generator(np.random.PCG64([self.seed, 3]))
        seeds = rng.choice(2 ** 16, size=self.F[0], replace=False) + 1
        rates = self.rates or (PROFILE_RATE[self.profile],)
        return [c.fading_taps(self.profile, rates[f % len(rates)], s) for f, s in enumerate(seeds)]


TILE_CASES = [
    TileCase("A", 256, 128, ("comb", 4), 64, (37, 1), "ETU", seed=15, fpw=(4, 4), tiles=2),
    TileCase("A7", 256, 128, ("comb", 4), 64, (37,), "EPA", seed=11, fpw=(4, 4), tiles=2, omp="regs"),
    TileCase("AV", 256, 128, ("comb", 4), 64, (21,), "ETU", seed=6, fpw=(4, 4), tiles=2, rates=(2e7, 2.2e7, 2.4e7)),
    TileCase("B", 256, 192, ("comb", 4), 64, (21,), "ETU", seed=12, fpw=(4, 4), tiles=3),
    TileCase("C", 256, 100, ("mask", 18), 256, (19,), "ETU", seed=11, fpw=(4, 4), tiles=0),
    TileCase("D", 1024, 640, ("comb", 4), 256, (21,), "EPA", seed=1, fpw=(2, 4), tiles=10, omp="regs"),
    TileCase("E", 1024, 640, ("mask", 320), 1024, (13,), "EPA", seed=5, fpw=(1, 2), tiles=20, omp="regs"),
    TileCase("F", 1024, 640, ("mask", 576), 1024, (9,), "EPA", seed=12, precisions=("fp32",), fpw=(1, 1), tiles=36, omp="regs"),
]
TILE = {c.name: c for c in TILE_CASES}

# the pilot bound of the part-2 tile's MMSE stage ("at most 585 pilots"): the last served count and the first refused one
BOUND_SERVED = TileCase("P585", 1024, 640, ("mask", 585), 1024, (2,), "EPA", seed=12, precisions=("fp32",), fpw=(1, 1))
BOUND_REFUSED = TileCase("P586", 1024, 640, ("mask", 586), 1024, (2,), "EPA", seed=12, precisions=("fp32",), fpw=(1, 1))


class MarginLib(OracleLib):
    """OracleLib that also records, per MP_estimate / OMP_estimate call, the smallest top-two gap of the pursuit's scores."""

    def __init__(self, oracle):
        super().__init__(oracle)
        self.mp_gaps, self.omp_gaps = [], []

        def omp(Y, S, Nfft, taps, SNR_dB=0.0):
            self.omp_gaps.append(pursuit_min_gap(oracle, Y, np.asarray(S), taps))
            return oracle.OMP_estimate(Y, S, Nfft, taps, SNR_dB)
        self.OMP_estimate = omp

    def MP_estimate(self, Y, S, Nfft, dominant_taps):
        self.mp_gaps.append(mp_min_gap(self._o, Y, np.asarray(S), dominant_taps))
        return super().MP_estimate(Y, S, Nfft, dominant_taps)


def mp_min_gap(oracle, y, S, taps):
    """Smallest (best - second) / best over the projections of MP_estimate.m:10-18 (|S(:, 1:Np)' r|^2 / Np, picked columns at
    -100); the replay is checked against the oracle's own picks."""
    S = np.asarray(S)
    n = S.shape[0]
    r = np.asarray(y, dtype=np.complex128).ravel().copy()
    picks, worst = [], 1.0
    for _ in range(int(taps)):
        proj = np.abs(S[:, :n].conj().T @ r) ** 2 / n
        proj[picks] = -100.0
        top = np.sort(proj)
        worst = min(worst, float((top[-1] - top[-2]) / top[-1]))
        k = int(np.argmax(proj))
        picks.append(k)
        a = S[:, k]
        r = r - a * ((a.conj() @ r) / n)
    assert [k + 1 for k in picks] == list(oracle.MP_estimate(y, S, S.shape[1], taps)[2])
    return worst


def decision_margin(iq):
    """Smallest distance of a 16QAM point to a decision boundary (0, +-2 / sqrt(10) per axis) in units of the grid step."""
    step = 2.0 / math.sqrt(10.0)
    a = np.abs(np.concatenate([np.real(iq).ravel(), np.imag(iq).ravel()]))
    return float(np.min(np.minimum(a, np.abs(a - step))) / step)


def build_tile(oracle, case):
    """The inputs of one tile call: the scenario's frame as drivers/task5_part2.py:74-80 makes it, and the channel draws."""
    from ofdm_course_amd.drivers import common as c
    lib = OracleLib(oracle)
    pc, dc = case.layout()
    dict_, bps = lib.constellation_func(CONSTELLATION)
    pilotValues = c.alternating_pilots(2 * np.max(np.abs(dict_)), len(pc), N_SYMB)
    bits = c.synthetic_bits(N_SYMB * len(dc) * bps, [case.seed, 1])
    TX_IQ, pad = lib.mapping(bits, CONSTELLATION)
    X = lib.OFDM_map_carriers(TX_IQ, N_SYMB, case.nfft, dc, pc, pilotValues)
    Tx = np.asarray(lib.OFDM_modulator(X, case.t_guard)).ravel(order="F")
    Tx_noised, _ = lib.Noise(SNR_DB, Tx, seed=case.seed, stream=0)
    return dict(pc=pc, dc=dc, pilotValues=pilotValues, bits=bits, pad=pad, Tx=Tx, Tx_noised=np.asarray(Tx_noised),
                taps_list=case.taps_list())


_TILE_CACHE = {}


def oracle_tile_full(oracle, case):
    """drivers/task5_part2.py:102-124 for every realisation of case.F[0], nothing summed.  Returns dict(nmse [4, F], errors
    [4, F], mp_gap [F], omp_gap [F], margin [4, F], bits); computed once per case."""
    if case.name in _TILE_CACHE:
        return _TILE_CACHE[case.name]
    from ofdm_course_amd.drivers import common as c
    lib = MarginLib(oracle)
    b = build_tile(oracle, case)
    pc, dc, pilotValues, bits, pad = b["pc"], b["dc"], b["pilotValues"], b["bits"], b["pad"]
    Nfft, N_carrier, T_Guard, F = case.nfft, case.n_carrier, case.t_guard, case.F[0]
    S = lib.sensing_matrix(pc, Nfft, case.K)                                        # :102
    nmse, errors, margin = np.zeros((4, F)), np.zeros((4, F), dtype=np.int64), np.zeros((4, F))
    for f, taps in enumerate(b["taps_list"]):
        h_t, H_f = lib.get_MP_channel_resp(taps, Nfft)                              # :107
        rx = c.conv_truncate(lib, b["Tx_noised"], h_t).reshape((Nfft + T_Guard, N_SYMB), order="F")   # :108-109
        Xr = lib.OFDM_demodulator(rx, T_Guard)                                      # :110
        h_full = np.zeros(N_carrier, dtype=np.complex128)
        h_full[:min(len(h_t), N_carrier)] = np.asarray(h_t)[:N_carrier]             # :111-112
        H = [lib.LS_CE(Xr, pilotValues, pc, N_carrier),                             # :113
             lib.MMSE_CE(Xr, pilotValues, pc, Nfft, N_carrier, h_full, SNR_DB)]     # :114
        Y = np.asarray(lib.get_payload(np.asarray(Xr)[:, :1], pc)).ravel() / pilotValues[:, 0]   # :115
        H.append(lib.MP_estimate(Y, S, Nfft, taps.shape[0])[0])                     # :117
        H.append(lib.OMP_estimate(Y, S, Nfft, taps.shape[0], SNR_DB)[0])            # :118
        for e in range(4):
            nmse[e, f] = c.mse_row(H_f, H[e], N_carrier)                            # :120
            eq = lib.equalize_signal(Xr, H[e], N_carrier)                           # :121
            RX_IQ = np.asarray(lib.get_payload(eq, dc)).ravel(order="F")            # :122
            out_bits = lib.demapping(pad, RX_IQ, CONSTELLATION)                     # :123
            errors[e, f] = lib.BER_func(bits, np.asarray(out_bits).ravel(), return_count=True)   # :124
            margin[e, f] = decision_margin(RX_IQ)
    res = dict(nmse=nmse, errors=errors, mp_gap=np.array(lib.mp_gaps), omp_gap=np.array(lib.omp_gaps), margin=margin,
               bits=int(bits.size))
    _TILE_CACHE[case.name] = res
    return res


def oracle_tile(oracle, case, F=None):
    """(nmse [4, F], errors [4, F]) per realisation; F defaults to case.F[0], a smaller F is its prefix (the realisations are
    independent of one another in the script)."""
    full = oracle_tile_full(oracle, case)
    F = case.F[0] if F is None else F
    return full["nmse"][:, :F].copy(), full["errors"][:, :F].copy()


def fp32_loose(full):
    """Realisations whose smallest MP / OMP pick gap is below the fp32 tolerance."""
    return np.minimum(full["mp_gap"], full["omp_gap"]) < FP32_GAP


def boundary_slots(F):
    """First and last slots of every workgroup of every split: groups of 4 (mmse_wave_kernel, FB = 4) cover those of 8 and 16;
    the last realisation of the tile closes the ragged group."""
    return np.array([f % 4 in (0, 3) or f == F - 1 for f in range(F)])


# ---- the MSE(SNR) tile -------------------------------------------------------------------------------------------------------
CHANNEL_TAPS = ((0, 1.0), (4, .8), (10, .6), (15, .4), (21, .2), (25, .1))             # Main_model_Task_5.m:112-119
M3_TAPS = CHANNEL_TAPS[:3] + ((10, -.3 + .25j),) + CHANNEL_TAPS[3:] + ((150, .2 - .1j),)   # delay 10 twice; 150 >= N_carrier


@dataclasses.dataclass(frozen=True)
class MseCase:
    name: str
    nfft: int
    n_carrier: int
    comb: int
    K: int
    snrs: tuple
    channel_taps: tuple
    seed: int
    precisions: tuple
    stream0: int = 1
    fpw32: int = 4         # mp_batch_kernel in fp32
    wpw: int = 4           # wavefronts per workgroup of mmse_wave_kernel

    @property
    def t_guard(self):
        return self.nfft // 8

    @property
    def n_pilots(self):
        return self.n_carrier // self.comb

    def taps(self):
        return np.array(self.channel_taps)


MSE_CASES = [
    MseCase("M1", 256, 128, 4, 64, tuple(np.linspace(0.0, 30.0, 37)), CHANNEL_TAPS, seed=2, precisions=("fp64", "fp32")),
    MseCase("M2", 2048, 1280, 1, 2048, (0.0, 7.5, 15.0, 22.5, 30.0), CHANNEL_TAPS, seed=1, precisions=("fp32",), fpw32=1, wpw=1),
    MseCase("M3", 256, 128, 4, 64, (0.0, 7.5, 15.0, 22.5, 30.0), M3_TAPS, seed=2, precisions=("fp64",)),
]
MSE = {c.name: c for c in MSE_CASES}


def build_mse(oracle, case):
    """The clean TX stream of drivers/task5.py:43-58 (constant pilots of 4/3 of the largest symbol, a scrambled payload when the
    comb leaves data carriers) and the plan's arguments."""
    from ofdm_course_amd.drivers import common as c
    lib = OracleLib(oracle)
    _, pc, dc = c.layout_comb(case.nfft, case.n_carrier, case.comb)
    dict_, bps = lib.constellation_func(CONSTELLATION)
    amp = 4 / 3 * np.max(np.abs(dict_))
    pilotValues = np.full((len(pc), N_SYMB), amp, dtype=np.complex128)
    if case.comb != 1:
        bits = c.synthetic_bits(N_SYMB * len(dc) * bps, case.seed)
        TX_IQ, _ = lib.mapping(c.scramble_per_frame(lib, "Scrambler", bits, 1), CONSTELLATION)
        X = lib.OFDM_map_carriers(TX_IQ, N_SYMB, case.nfft, dc, pc, pilotValues)
    else:
        X = np.zeros((case.nfft, N_SYMB), dtype=np.complex128)
        X[pc.astype(int) - 1, :] = pilotValues
    Tx = np.asarray(lib.OFDM_modulator(X, case.t_guard)).ravel(order="F")
    return dict(pc=pc, dc=dc, pilotValues=pilotValues, amp=amp, Tx=Tx)


_MSE_CACHE = {}


def oracle_mse_tile_full(oracle, case):
    """drivers/task5.py:102-109 (Main_model_Task_5.m:305-345) for every SNR point: Noise from Philox stream stream0 + i, the dense
    impulse response of get_MP_channel_resp (a later row at the same delay wins), MMSE with h = ifft(H_LS).  Returns dict(mse
    [4, n], mp_gap [n], omp_gap [n]); computed once per case."""
    if case.name in _MSE_CACHE:
        return _MSE_CACHE[case.name]
    from ofdm_course_amd.drivers import common as c
    from ofdm_course_amd.drivers import task5
    lib = MarginLib(oracle)
    b = build_mse(oracle, case)
    taps = case.taps()
    H_tau, H_freq = lib.get_MP_channel_resp(taps, case.nfft)
    S = lib.sensing_matrix(b["pc"], case.nfft, case.K)
    mse = np.zeros((4, len(case.snrs)))
    for i, snr in enumerate(case.snrs):
        Rx_i, _ = lib.Noise(float(snr), b["Tx"], seed=case.seed, stream=case.stream0 + i)
        Rx_i = c.conv_truncate(lib, Rx_i, H_tau)
        Xi = lib.OFDM_demodulator(np.asarray(Rx_i).reshape((case.nfft + case.t_guard, N_SYMB), order="F"), case.t_guard)
        _, m, _ = task5._estimates(lib, Xi, b["pilotValues"], b["pc"], case.nfft, case.n_carrier, b["amp"], S, taps.shape[0],
                                   float(snr), H_freq)
        mse[:, i] = [m["LS"], m["MMSE"], m["MP"], m["OMP"]]
    res = dict(mse=mse, mp_gap=np.array(lib.mp_gaps), omp_gap=np.array(lib.omp_gaps))
    _MSE_CACHE[case.name] = res
    return res


def oracle_mse_tile(oracle, case):
    """MSEs [4, n] per SNR point, rows LS, MMSE, MP, OMP."""
    return oracle_mse_tile_full(oracle, case)["mse"].copy()


def report(oracle):
    """One line per case: the smallest pick gaps, the smallest decision margin and the share of fp32_loose realisations."""
    lines = []
    for case in TILE_CASES:
        full = oracle_tile_full(oracle, case)
        loose = fp32_loose(full)
        lines.append(f"{case.name:3s} seed {case.seed}  MP gap {full['mp_gap'].min():.3g}  OMP gap {full['omp_gap'].min():.3g}  "
                     f"decision margin {full['margin'].min():.3g}  fp32_loose {int(loose.sum())}/{loose.size} "
                     f"{np.flatnonzero(loose).tolist()}")
    for case in MSE_CASES:
        full = oracle_mse_tile_full(oracle, case)
        lines.append(f"{case.name:3s} seed {case.seed}  MP gap {full['mp_gap'].min():.3g}  OMP gap {full['omp_gap'].min():.3g}")
    return lines


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import ofdm_oracle
    print("\n".join(report(ofdm_oracle)))
