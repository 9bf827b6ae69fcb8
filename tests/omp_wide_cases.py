"""Inputs of the wide OMP route's tests (tests/test_gpu_omp_wide.py), made on the CPU with the oracle alone.  TEST INFRASTRUCTURE.

With Np << K neighbouring atoms of the dictionary are coherent, and a device pick may differ from the oracle's only where the
oracle's OWN two best scores are within rounding of each other.  So every seed below was chosen with the oracle alone such
that every iteration of every realisation has a top-two gap (best - second) / best above 1e-6 (fp64 cases) or 1e-3 (cases that
also run in fp32; the near-tie threshold of tests/pick_audit.py is 1e-4), with Np >= taps (no rank-deficient pinv).
No realisation is set aside.  The smallest gap found stands next to each seed; tests/test_omp_wide_inputs_host.py recomputes
every one and fails on a drift above 1 % (`python tests/omp_wide_cases.py` prints them)."""
from __future__ import annotations

import dataclasses

import numpy as np

from oracle_lib import OracleLib


def pursuit_min_gap(oracle, y, S, taps):
    """Smallest (best - second) / best over every pick of OMP_estimate.m:7-23 on (y, S); the replay is checked against the
    oracle's own picks."""
    y = np.asarray(y, dtype=np.complex128).ravel()
    idx, r, worst = [], y.copy(), 1.0
    for it in range(int(taps)):
        sc = np.abs(S.conj().T @ r)
        top = np.sort(sc)
        worst = min(worst, float((top[-1] - top[-2]) / top[-1]))
        idx.append(int(np.argmax(sc)))
        A = S[:, idx]
        r_new = y - A @ (oracle._pinv_matlab(A) @ y)
        stop = it > 0 and np.linalg.norm(r_new - r) / np.linalg.norm(r) < 1e-2      # OMP_estimate.m:20
        r = r_new
        if stop:
            break
    assert [k + 1 for k in idx] == list(oracle.OMP_estimate(y, S, S.shape[1], taps)[2])
    return worst


@dataclasses.dataclass(frozen=True)
class YCase:
    """n pilot LS vectors Y = H(pilots) + noise of a `delays`-tap channel with PCG64(seed) amplitudes."""
    name: str
    nfft: int
    n_carrier: int
    pilots: tuple          # ("mask", Np) = sort(randperm(N_carrier, Np)) drawn from `seed`, or ("comb", step)
    K: int
    delays: tuple
    seed: int
    gap: float             # smallest top-two gap of the oracle's pursuit over the n realisations
    n: int = 5
    snr_db: float = 30.0

    @property
    def taps(self):
        return len(self.delays)

    def pilot_carriers(self):
        if self.pilots[0] == "comb":
            return np.arange(1, self.n_carrier + 1, self.pilots[1])
        rng = np.random.Generator(np.random.PCG64([self.seed, 11]))
        return np.sort(rng.permutation(self.n_carrier)[:self.pilots[1]] + 1)

    def data_carriers(self):
        pc = self.pilot_carriers()
        a = np.arange(1, self.n_carrier + 1)
        d = a[~np.isin(a, pc)]
        return d if d.size else a[:0]

    def Y(self):
        """[Np, n] complex128."""
        rng = np.random.Generator(np.random.PCG64([self.seed, 13]))
        pc0 = self.pilot_carriers() - 1
        d = np.asarray(self.delays)
        out = np.empty((pc0.size, self.n), dtype=np.complex128)
        for j in range(self.n):
            a = (rng.standard_normal(d.size) + 1j * rng.standard_normal(d.size)) * np.exp(-0.15 * np.arange(d.size))
            H = np.exp(-2j * np.pi * np.outer(pc0, d) / self.nfft) @ a
            w = (rng.standard_normal(pc0.size) + 1j * rng.standard_normal(pc0.size)) / np.sqrt(2)
            out[:, j] = H + w * np.sqrt(np.mean(np.abs(H) ** 2) * 10 ** (-self.snr_db / 10))
        return out

    def min_gap(self, oracle):
        S = oracle.sensing_matrix(self.pilot_carriers().astype(np.float64), self.nfft, self.K)
        Y = self.Y()
        return min(pursuit_min_gap(oracle, Y[:, j], S, self.taps) for j in range(self.n))


OMP_RT = 8                                       # chain_fast_core.hpp
EPA7 = (0, 1, 2, 3, 5, 8, 17)                    # seven paths, EPA-like spacing at the sample rate of a 512-point frame
ETU9 = (0, 1, 2, 4, 6, 9, 15, 27, 50)            # nine paths: more than OMP_RT = 8, the refit state in LDS

Y_CASES = [
    YCase("mask24-512-taps7", 512, 512, ("mask", 24), 512, EPA7, seed=1, gap=0.02238),
    YCase("mask24-512-taps9", 512, 512, ("mask", 24), 512, ETU9, seed=1, gap=0.003937),
    YCase("comb4-1024-k256", 1024, 1024, ("comb", 4), 256, EPA7, seed=2, gap=0.003638),
]


# the two small plans of the refusal test (Nfft the wide kernel is not built for): their batch-route picks are compared too
REFUSAL_CASES = [
    YCase("comb4-256-refused", 256, 256, ("comb", 4), 64, (0, 2, 5), seed=1, gap=0.002779, n=2),
    YCase("comb4-8192-refused", 8192, 256, ("comb", 4), 64, (0, 2, 5), seed=1, gap=0.0001746, n=2),
]


# ---- omp_batch_kernel with more than OMP_RT taps (omp_frame_wave), whose refit is now the function it shares with the wide
# kernel: the two shapes whose receiver outputs are stored from the commit before the split (tests/golden/omp_wave_parent.npz,
# written by wave_parent_outputs below on that commit's library) and must come out bit for bit.
#   (Nfft, N_carrier, comb, K, delays): a: dictionary correlation (MFMA in fp32, scalar in fp64), c0 in LDS;
#   b: comb_m = 2048, c0 by transform and in registers (reg_c0), 12 taps
WAVE_PARENT = {
    "a": (512, 512, 4, 128, ETU9),
    "b": (4096, 1024, 2, 512, (0, 1, 2, 4, 6, 9, 15, 27, 50, 81, 130, 200)),
}


def wave_parent_frames(key, n=3):
    """rx [(Nfft + Nfft/8) * 2, n] complex64 (the fp64 run takes the same samples), pilot and data carriers, pilot column."""
    nfft, nc, comb, K, delays = WAVE_PARENT[key]
    rng = np.random.Generator(np.random.PCG64([17, len(delays)]))
    pc = np.arange(1, nc + 1, comb)
    dc = np.setdiff1d(np.arange(1, nc + 1), pc)
    tg, ns = nfft // 8, 2
    rx = np.empty(((nfft + tg) * ns, n), dtype=np.complex64)
    for f in range(n):
        X = np.zeros((nfft, ns), dtype=np.complex128)
        X[pc - 1] = 2.0
        X[dc - 1] = ((2 * rng.integers(0, 2, (dc.size, ns)) - 1) + 1j * (2 * rng.integers(0, 2, (dc.size, ns)) - 1)) / np.sqrt(2)
        x = np.fft.ifft(X, axis=0)
        tx = np.concatenate([x[-tg:], x], axis=0).ravel(order="F")
        h = np.zeros(max(delays) + 1, dtype=np.complex128)
        h[list(delays)] = (rng.standard_normal(len(delays)) + 1j * rng.standard_normal(len(delays))) * np.exp(-0.1 * np.arange(len(delays)))
        y = np.convolve(tx, h)[:tx.size]
        y = y + (rng.standard_normal(y.size) + 1j * rng.standard_normal(y.size)) * np.sqrt(np.mean(np.abs(y) ** 2) * 1e-3 / 2)
        rx[:, f] = y
    return rx, pc, dc, np.full(pc.size, 2.0)


def wave_parent_outputs(ofdm, key, precision):
    """(index [taps, n] int32, H [N_carrier, n]) of rx_chain_task5 on the frames above."""
    nfft, nc, comb, K, delays = WAVE_PARENT[key]
    rx, pc, dc, pv = wave_parent_frames(key)
    plan = ofdm.RxPlan(nfft, nfft // 8, 2, nc, pc, dc, pv, K, len(delays), "QPSK", precision=precision)
    out = ofdm.rx_chain_task5(plan, rx.astype(np.complex128) if precision == "fp64" else rx, want_h=True, want_index=True)
    plan.close()
    return np.asarray(out["index"]).copy(), np.asarray(out["H"]).copy()


class GapLib(OracleLib):
    """OracleLib that also records the smallest top-two gap of every OMP_estimate call of a driver replay."""

    def __init__(self, oracle):
        super().__init__(oracle)
        self.worst = 1.0
        self.calls = 0

        def omp(Y, S, Nfft, taps, SNR_dB=0.0):
            self.worst = min(self.worst, pursuit_min_gap(oracle, Y, np.asarray(S), taps))
            self.calls += 1
            return oracle.OMP_estimate(Y, S, Nfft, taps, SNR_dB)
        self.OMP_estimate = omp


# ---- the driver replays (tests 3 and 4): keyword sets of drivers.task5_part2.run / drivers.task5.run, the seed inside
# reg_pilot = 0 at the reference's own size: Nfft 4096, dictionary = all 4096 delays, random mask of 64 pilots, EPA (7 paths);
# runs in fp64 and fp32, so the gap bound is 1e-3
PART2_KW = dict(Nfft=4096, N_carrier=1024, reg_pilot=0, Nps=[64], monteCarloRuns=3, seed=2)
PART2_GAP = 0.003698
# Main_model_Task_5.m as committed: Nfft 4096, comb 1 (Np = K = 1024), three SNR points
MSE_KW = dict(Nfft=4096, N_carrier=1024, comb=1, seed=1)
MSE_SNRS = (5.0, 17.5, 30.0)
MSE_GAP = 0.00566
# the same frame through a nine-path channel: more than OMP_RT taps, where omp_batch_kernel keeps a two-sided Gram table and
# its state exceeds the LDS bound (test_omp_wide_inputs_host.py computes both figures)
MSE9_TAPS = ((0, 1.0), (4, .8), (10, .6), (15, .4), (21, .3), (25, .25), (31, .2), (38, .15), (47, .1))
MSE9_GAP = 0.01344


def part2_gap(oracle):
    from ofdm_course_amd.drivers import task5_part2
    lib = GapLib(oracle)
    task5_part2.run(lib, **PART2_KW)
    assert lib.calls == 3
    return lib.worst


def mse_gap(oracle, nine=False):
    from ofdm_course_amd.drivers import task5
    lib = GapLib(oracle)
    kw = dict(MSE_KW, channel_taps=np.array(MSE9_TAPS)) if nine else MSE_KW
    task5.run(lib, SNRs=np.array(MSE_SNRS), **kw)
    # (the single-frame part of the driver makes one more OMP_estimate call, at SNR_dB = 20: it counts too)
    assert lib.calls == 4
    return lib.worst


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import ofdm_oracle
    for c in Y_CASES + REFUSAL_CASES:
        print(c.name, c.seed, f"{c.min_gap(ofdm_oracle):.4g}")
    print("part2", f"{part2_gap(ofdm_oracle):.4g}")
    print("mse", f"{mse_gap(ofdm_oracle):.4g}", "mse9", f"{mse_gap(ofdm_oracle, True):.4g}")
