"""Cases of the plan's OMP route (RxPlan.set_omp_route; tests/test_gpu_omp_route.py), made on the CPU with the oracle alone.
TEST INFRASTRUCTURE.

Every case is a routes.Case whose pilots may be a random mask (drivers.task5_part2.random_pilot_layout, the layout of
T5/Task5_part2.m:58-64) and whose dictionary holds all Nfft delays, so the frames, the oracle's pursuit and the gap method are
those of tests/routes.py (oracle_frames, oracle_min_gap).  With Np << K = Nfft neighbouring atoms are coherent: the mask seeds
below were chosen with the oracle alone so that every pick of every frame has a top-two gap (best - second) / best above 1e-3
(the near-tie threshold of tests/pick_audit.py is 1e-4).  No frame is set aside.  GAPS records the figure of every fp32 case
(`python tests/omp_route_cases.py` prints them); tests/test_omp_route_host.py recomputes each one."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import routes


@dataclass
class RouteCase(routes.Case):
    mask: tuple | None = None    # (Np, mask seed): sort(randperm(N_carrier, Np)) instead of the comb
    omp_route: str = "auto"      # what the plan is set to

    def pilot_carriers(self):
        if self.mask is None:
            return super().pilot_carriers()
        from ofdm_course_amd.drivers.task5_part2 import random_pilot_layout
        pc = random_pilot_layout(self.nfft, self.nc, self.mask[0], self.mask[1])[1]
        assert pc.size == self.mask[0], "the mask seed gave pilot_step 1 (the 100 % rule)"
        return pc.astype(np.int64)

    def cfg(self):
        from ofdm_course_amd import frames as fr
        return fr.FrameConfig(self.name, self.nfft, self.nc, self.comb, self.const, N_symb=self.n_symb, taps=self.taps,
                              SNR_dB=self.snr, dominant_taps=len(self.delays),
                              pilots=self.pilot_carriers().astype(np.float64), K_atoms=self.k_atoms)


T4 = (0, 2, 5, 9)

# 1. shapes omp_batch_kernel refuses ("OMP stage needs"): `auto` takes the wide kernel
AUTO_4096 = [RouteCase(f"auto-4096-mask48-{p}", 4096, 256, 1, "16QAM", 2, T4, precision=p, k_atoms=4096, mask=(48, 2), n_frames=4)
             for p in ("fp32", "fp64")]
AUTO_2048 = [RouteCase("auto-2048-mask40-fp64", 2048, 200, 1, "QPSK", 2, T4, precision="fp64", k_atoms=2048, mask=(40, 2),
                       n_frames=4)]
# 2. `wide` forced where `batch` also serves (NE = 8; Nfft 512: lg_up = 2, Nfft 1024: lg_up = 1).
#    A comb-4 plan that would take the fused front end: on pilots 1 : 4 : N_carrier the atoms k and k + Nfft / 4 are the SAME
#    column, so a dictionary beyond K = Nfft / comb = 128 has exact ties in every pick (oracle gap 0) and no tie-free frame
#    exists; the comb plan therefore carries the largest tie-free dictionary, K = 128, and K = Nfft = 512 runs on a random mask.
WIDE_512 = [RouteCase(f"wide-512-comb4-k128-{p}", 512, 256, 4, "16QAM", 2, routes.T3, precision=p, k_atoms=128, omp_route="wide",
                      n_frames=4) for p in ("fp32", "fp64")]
WIDE_512_MASK = [RouteCase(f"wide-512-mask48-{p}", 512, 256, 1, "16QAM", 2, T4, precision=p, k_atoms=512, mask=(48, 2),
                           omp_route="wide", n_frames=4) for p in ("fp32", "fp64")]
WIDE_1024 = [RouteCase(f"wide-1024-mask48-{p}", 1024, 256, 1, "64QAM", 2, T4, precision=p, k_atoms=1024, mask=(48, 3),
                       omp_route="wide", n_frames=4) for p in ("fp32", "fp64")]
# 4. the split call sites: more than 48 Ki decisions per frame at Nfft 512 (Nfft, N_carrier and N_symb of routes'
#    split-512-49k-decisions; a random mask instead of its comb, for the reason above: K = 512)
SPLIT_512 = [RouteCase(f"wide-split-512-49k-{p}", 512, 384, 1, "QPSK", 171, routes.T3, precision=p, k_atoms=512, mask=(48, 2),
                       omp_route="wide", n_frames=3) for p in ("fp32", "fp64")]

CASES = AUTO_4096 + AUTO_2048 + WIDE_512 + WIDE_512_MASK + WIDE_1024 + SPLIT_512

# 5. `wide` on plans the wide route cannot serve: (case, fragment of the reason)
REFUSED = [
    (RouteCase("wide-refused-8192", 8192, 256, 4, "QPSK", 2, routes.T3, omp_route="wide", n_frames=2), "not built for Nfft 8192"),
    (RouteCase("wide-refused-256", 256, 64, 4, "QPSK", 2, routes.T3, omp_route="wide", n_frames=2), "generic single-kernel entry"),
    (RouteCase("wide-refused-oob", 512, 128, 4, "QPSK", 2, routes.T3, pilots=("extra", 200), omp_route="wide", n_frames=2),
     "a pilot outside 1..N_carrier"),
]

# smallest top-two gap of the oracle's own pursuit on the Philox frames of every fp32 case (routes.oracle_min_gap)
GAPS: dict[str, float] = {
    "auto-4096-mask48-fp32": 0.002189,
    "wide-512-comb4-k128-fp32": 0.2527,
    "wide-512-mask48-fp32": 0.1643,
    "wide-1024-mask48-fp32": 0.009029,
    "wide-split-512-49k-fp32": 0.2353,
}


@functools.lru_cache(maxsize=None)
def _frames(name):
    from oracle import ofdm_oracle
    case = {c.name: c for c in CASES + [r[0] for r in REFUSED]}[name]
    rx, bits, pv_col = routes.oracle_frames(case, ofdm_oracle)
    for a in (rx, bits, pv_col):
        a.setflags(write=False)
    return rx, bits, pv_col


def frames(case):
    """(rx [frame_samples, n_frames] complex128, bits [n_frames, frame_bits], pilot column) from oracle.tx_frame: made once per
    case and shared (read-only)."""
    return _frames(case.name)


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import ofdm_oracle
    for c in CASES:
        if c.precision == "fp32":
            print(f'    "{c.name}": {routes.oracle_min_gap(c, ofdm_oracle):.4g},', flush=True)
