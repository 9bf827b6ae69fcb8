"""The zero-delay-spread corner of the MMSE estimators (csrc/mmse_tau.hpp): cases, the host-arithmetic prediction, the exact
reference and its sensitivity floor, made on the CPU alone.  TEST INFRASTRUCTURE: no GPU, no HIP.

h = a delta[k - d] has tau_rms = 0 exactly; r2 - r^2 of MMSE_CE.m:22-24 is then rounding noise of either sign.
  * host_diff: that difference in the order of the library's host code (ofdm_chain_mmse.hip, ofdm_part2.hip), in plain doubles.
  * exact: oracle.MMSE_CE with h0 = a delta[k], the same amplitude moved to bin 0, where r = r2 = 0 without rounding and rf, rf2
    are the tau = 0 matrices (MMSE_CE.m uses h for nothing else).  The oracle is not modified.
  * floor: oracle.MMSE_CE with the two-tap h = [sqrt(1 - q), sqrt(q)], q = (d sqrt(8 eps))^2 -- tau = the square root of the
    largest rounding error r2 - r^2 can carry at delay d -- against exact, as rel_l2: what the reference itself can not resolve.
`python tests/mmse_degenerate_cases.py` prints the floors of every case of tests/test_gpu_mmse_degenerate.py (the chain cases on
the oracle's own frames of the same geometry; the test measures them again on the frames it runs)."""
from __future__ import annotations

import dataclasses

import numpy as np

import part2_tile_cases as tc

A = 0.7 - 0.2j
EPS = float(np.finfo(np.float64).eps)
CAP = 1e-3                       # a derived fp64 bound above this means a badly conditioned case, not a wider bound


def host_diff(taps):
    """r2 - r * r of [(amplitude, delay), ...] as the host code forms it: p = re^2 + im^2; s0 += p; s1 += p d; s2 += p d d."""
    s0 = s1 = s2 = 0.0
    for a, d in taps:
        a, d = complex(a), float(d)
        p = a.real * a.real + a.imag * a.imag
        s0 += p
        s1 += p * d
        s2 += p * d * d
    r, r2 = s1 / s0, s2 / s0
    return r2 - r * r


def tau_delta(d):
    return d * np.sqrt(8 * EPS)


def two_tap(d):
    q = tau_delta(d) ** 2
    return np.array([np.sqrt(1 - q), np.sqrt(q)], dtype=np.complex128)


def rel_l2(a, b):
    return float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b)))


def exact(oracle, Y, Xp, pilots, nfft, nc, a, snr):
    return oracle.MMSE_CE(Y, Xp, pilots, nfft, nc, np.array([a], dtype=np.complex128), snr)[0]


def floor(oracle, Y, Xp, pilots, nfft, nc, a, d, snr):
    return rel_l2(oracle.MMSE_CE(Y, Xp, pilots, nfft, nc, two_tap(d), snr)[0], exact(oracle, Y, Xp, pilots, nfft, nc, a, snr))


# ---- (a) ofdm.MMSE_CE: (nfft, nc, comb, a, d, h_len or None = N_carrier) ------------------------------------------------------
CE_SNR = 20.0
CE_CASES = [(512, 128, 4, A, d, None) for d in range(1, 64)] + [(1024, 400, 8, 0.8 + 0j, 27, None), (512, 128, 4, A, 10, 11)]


def ce_inputs(oracle, nfft, nc, comb, a, d, precision):
    """Y = a exp(-2 pi i d k / Nfft) + noise at CE_SNR on unit pilots; fp32: the amplitude, then Y, rounded to float.  Returns
    (Y, Xp, pilots, a).  The noise keeps the case conditioned: at tau = 0 the estimate is the mean of the pilot LS values
    (rf, rf2 are all ones), and the noiseless pilot phasors of a comb-4 layout sum to exactly zero when d is a multiple of 4 --
    a zero reference has no relative error."""
    pc, _ = oracle.pilot_layout_comb(nc, comb)
    if precision == "fp32":
        a = complex(np.complex64(a))
    rng = np.random.default_rng([nfft, d])
    w = (rng.standard_normal(nfft) + 1j * rng.standard_normal(nfft)) * (abs(a) * 10 ** (-CE_SNR / 20) / np.sqrt(2))
    Y = (a * np.exp(-2j * np.pi * d * np.arange(nfft) / nfft) + w)[:, None]
    Xp = np.ones((len(pc), 1), dtype=np.complex128)
    if precision == "fp32":
        Y, Xp = Y.astype(np.complex64), Xp.astype(np.complex64)
    return Y, Xp, pc, a


def ce_floors(oracle, precision="fp64"):
    out = []
    for nfft, nc, comb, a, d, _ in CE_CASES:
        Y, Xp, pc, a_ = ce_inputs(oracle, nfft, nc, comb, a, d, precision)
        out.append(floor(oracle, Y.astype(np.complex128), Xp.astype(np.complex128), pc, nfft, nc, a_, d, CE_SNR))
    return np.array(out)


# ---- (b) plan.set_mmse: (precision, nfft, nc, comb, const) x delays ----------------------------------------------------------
CHAIN_CASES = [("fp64", 512, 128, 4, "QPSK"), ("fp32", 512, 128, 4, "QPSK"), ("fp32", 1024, 400, 8, "16QAM")]
CHAIN_DELAYS = (5, 10, 15)
CHAIN_SNR = 22.0
CHAIN_FRAMES = 5


# ---- (c) ofdm_task5_part2_tile: case A's shape, one path per realisation ---------------------------------------------------
@dataclasses.dataclass(frozen=True)
class OnePathTile(tc.TileCase):
    n_paths: int = 1

    @property
    def paths(self):
        return self.n_paths

    def taps_list(self):
        if self.n_paths == 1:                                    # delays 1..21, the amplitude of the issue's sweep
            return [np.array([[d, A]], dtype=np.complex128) for d in range(1, self.F[0] + 1)]
        # a second path at a delay >= N_carrier: the tile's delay-spread rule (h_t(1:N_carrier)) skips it, one path is left
        return [np.array([[d, A], [late, amp]], dtype=np.complex128)
                for d, late, amp in ((5, self.n_carrier + 2, 0.05 + 0.02j), (10, self.n_carrier + 9, -0.03 + 0.04j))][:self.F[0]]


TILE_ONE = OnePathTile("DG1", 256, 128, ("comb", 4), 64, (21,), "ETU", seed=15, n_paths=1)
TILE_TWO = OnePathTile("DG2", 256, 128, ("comb", 4), 64, (2,), "ETU", seed=15, n_paths=2)
TILE_NONE = [np.array([[130, A], [140, 0.3 + 0j]], dtype=np.complex128)]      # every path outside 1..N_carrier: refused


def tile_kept(case, taps):
    """The (amplitude, delay) pairs the tile's delay-spread rule keeps."""
    return [(complex(a), int(np.real(d))) for d, a in taps if int(np.real(d)) < case.n_carrier]


class TauOracle:
    """The oracle with MMSE_CE's h replaced: mode "exact" moves the one kept path to bin 0, mode "floor" hands the two-tap h of
    tau_delta(d).  Every other attribute is the oracle's own; MMSE_CE itself is the oracle's function."""

    def __init__(self, oracle, mode):
        self._o, self._mode = oracle, mode

    def __getattr__(self, name):
        return getattr(self._o, name)

    def MMSE_CE(self, Y, Xp, pilot_loc, Nfft, N_carrier, h, SNR):
        h = np.asarray(h).ravel()
        (d,) = np.flatnonzero(h)                                  # one path inside 1..N_carrier
        hh = np.array([h[d]], dtype=np.complex128) if self._mode == "exact" else two_tap(int(d))
        return self._o.MMSE_CE(Y, Xp, pilot_loc, Nfft, N_carrier, hh, SNR)


def tile_reference(oracle, case):
    """oracle_tile_full with the exact-tau MMSE_CE, and the relative move of the MMSE NMSE under tau_delta (the carried floor)."""
    ex = tc.oracle_tile_full(TauOracle(oracle, "exact"), dataclasses.replace(case, name=case.name + "-exact"))
    fl = tc.oracle_tile_full(TauOracle(oracle, "floor"), dataclasses.replace(case, name=case.name + "-floor"))
    return ex, np.abs(fl["nmse"][1] - ex["nmse"][1]) / ex["nmse"][1]


def report(oracle):
    import routes
    lines = []
    fl = ce_floors(oracle)
    lines.append("(a) MMSE_CE d = 1..63: " + " ".join(f"{v:.2e}" for v in fl[:63]))
    lines.append(f"(a) (1024, 400, 8, 0.8, 27): {fl[63]:.3g}   h_len = d + 1 (d = 10): {fl[64]:.3g}   largest {fl.max():.3g}, "
                 f"fp64 bound {4 * fl.max():.3g}")
    worst = 0.0
    for prec, nfft, nc, comb, const in CHAIN_CASES:
        case = routes.Case("deg", nfft, nc, comb, const, 3, (0, 3, 7), precision=prec, snr=CHAIN_SNR, n_frames=CHAIN_FRAMES, seed=6)
        rx, _, pv_col = routes.oracle_frames(case, oracle)
        pv = np.repeat(pv_col[:, None], 3, axis=1)
        pc = case.pilot_carriers().astype(np.float64)
        per = []
        for d in CHAIN_DELAYS:
            for f in range(CHAIN_FRAMES):
                X = oracle.OFDM_demodulator(rx[:, f].reshape((nfft + nfft // 8, 3), order="F"), nfft // 8)
                per.append(floor(oracle, X, pv, pc, nfft, nc, A, d, CHAIN_SNR))
        worst = max(worst, max(per))
        lines.append(f"(b) {prec} ({nfft}, {nc}, {comb}) d = {CHAIN_DELAYS}: largest over {len(per)} frames {max(per):.3g}")
    lines.append(f"(b) largest {worst:.3g}, fp64 bound {4 * worst:.3g}")
    for case in (TILE_ONE, TILE_TWO):
        ex, fl = tile_reference(oracle, case)
        lines.append(f"(c) {case.name}: NMSE floors " + " ".join(f"{v:.2e}" for v in fl) + f"   largest {fl.max():.3g}; MP gap "
                     f"{ex['mp_gap'].min():.3g} OMP gap {ex['omp_gap'].min():.3g} decision margin {ex['margin'].min():.3g}")
    neg = [d for d in range(1, 64) if host_diff([(A, d)]) < 0]
    lines.append(f"host arithmetic, a = {A}: r2 - r^2 < 0 at d = {neg} ({len(neg)} of 63)")
    return lines


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import ofdm_oracle
    print("\n".join(report(ofdm_oracle)))
