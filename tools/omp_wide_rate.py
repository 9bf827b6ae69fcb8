"""Rates of the wide OMP route (omp_wide_kernel, csrc/ofdm_omp_wide.hip), one JSON line.

1. The reg_pilot = 0 study of Task5_part2.m at the reference's size (Nfft 4096, dictionary = all 4096 delays, random pilot
   masks) as device tiles against the same scenarios call by call (batched=False), wall clock of drivers.task5_part2.run.
2. ofdm_OMP_estimate_batch on one set of pilot vectors with route="wide" against route="batch" at a shape both kernels can run
   (Nfft 2048, K = 1024, random mask of 64 pilots, 7 taps, fp32 and fp64), event-timed in alternating rounds.

    python tools/omp_wide_rate.py [runs per scenario] [realisations of part 2]
"""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ofdm_course_amd as ofdm  # noqa: E402
from ofdm_course_amd.drivers import task5_part2  # noqa: E402
from sweep_rate import ab_rounds  # noqa: E402


def study(runs, precision):
    kw = dict(reg_pilot=0, Nps=[16, 32, 64, 128, 256], monteCarloRuns=runs, seed=2)       # Nfft 4096, N_carrier 1024, EPA
    out = {}
    for name, batched in (("tiled", True), ("call_by_call", False)):
        task5_part2.run(ofdm, batched=batched, precision=precision, **dict(kw, monteCarloRuns=2))      # both forms warm: first plans, workspaces, launches
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = task5_part2.run(ofdm, batched=batched, precision=precision, **kw)
        torch.cuda.synchronize()
        out[name + "_s"] = time.perf_counter() - t0
        out[name + "_BER_OMP"] = [float(v) for v in r["BERs"][3]]
    out["realisations"] = runs * len(kw["Nps"])
    return out


def kernels(n, precision):
    rng = np.random.Generator(np.random.PCG64(4))
    nfft, nc, n_p, K, taps = 2048, 1024, 64, 1024, 7
    pc = np.sort(rng.permutation(nc)[:n_p] + 1)
    dc = np.setdiff1d(np.arange(1, nc + 1), pc)
    plan = ofdm.RxPlan(nfft, nfft // 8, 2, nc, pc, dc, np.ones(n_p), K, taps, "QPSK", precision=precision)
    d = np.array([0, 1, 2, 3, 5, 8, 17])
    a = rng.standard_normal((taps, n)) + 1j * rng.standard_normal((taps, n))
    Y = np.exp(-2j * np.pi * np.outer(pc - 1, d) / nfft) @ a
    Y = Y + 0.03 * (rng.standard_normal(Y.shape) + 1j * rng.standard_normal(Y.shape))
    Yd = torch.as_tensor(Y.astype(np.complex128 if precision == "fp64" else np.complex64)).cuda()
    wide, batch = ab_rounds(lambda: ofdm.OMP_estimate_batch(plan, Yd, route="wide"), lambda: ofdm.OMP_estimate_batch(plan, Yd, route="batch"))
    iw = ofdm.OMP_estimate_batch(plan, Yd, route="wide")[0]
    ib = ofdm.OMP_estimate_batch(plan, Yd, route="batch")[0]
    plan.close()
    return {"realisations": n, "wide_ms": wide, "batch_ms": batch, "realisations_with_equal_picks": int((iw == ib).all(dim=0).sum().item())}


def main():
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    ofdm.init(0)
    print(json.dumps({"tool": "omp_wide_rate",
                      "study_nfft4096_k4096": {p: study(runs, p) for p in ("fp32", "fp64")},
                      "kernels_nfft2048_k1024_np64_taps7": {p: kernels(n, p) for p in ("fp32", "fp64")}}), flush=True)


if __name__ == "__main__":
    main()
