"""Frames/s of the estimator study, one JSON line: RxPlan.estimator_study (ofdm_estimator_study) at config M's geometry (Nfft 2048,
512 carriers, comb 4 = 128 pilots, which the MMSE stage accepts, K 128, 64QAM, 14 symbols) on the EPA tap-delay line at 30.72 MHz,
a channel per frame, everything device-resident.

The yardstick is the sum of two existing calls with the same points and frames in the same run on the same card: ber_sweep(fading=)
on an OMP plan plus ber_sweep(fading=) on a set_mmse_ls plan.  Those two run two of the four estimators, each through the
receiver's faster symbol stages, so the ratio says what the four-estimator picture costs against the two halves that existed, not
how far the study is from a bound.  The three are timed in alternation, the median of --reps calls each after one warm-up, with the
spread (max - min); the study's OMP row is compared with the OMP sweep's errors.

    python tools/estimator_study_rate.py [--frames 4096] [--points 20] [--precision fp32] [--mmse ls] [--reps 5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ofdm_course_amd as ofdm  # noqa: E402
from ofdm_course_amd import frames as fr  # noqa: E402
from ofdm_course_amd.drivers import common as c  # noqa: E402


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternating(routes, reps):
    """{tag: (median ms, spread ms)} of the routes timed in turn, round after round, after one warm-up each."""
    for fn in routes.values():
        fn()
    torch.cuda.synchronize()
    ms = {tag: [] for tag in routes}
    for _ in range(reps):
        for tag, fn in routes.items():
            ms[tag].append(once(fn))
    return {tag: (float(np.median(v)), float(max(v) - min(v))) for tag, v in ms.items()}


def measure(frames, snrs, precision, mmse, reps):
    dev = torch.device("cuda:0")
    cfg = fr.config_M()
    fading = c.fading_profile("EPA", 30.72e6)
    study_plan = fr.make_plan(cfg, ofdm, precision=precision, device=0)
    omp_plan = fr.make_plan(cfg, ofdm, precision=precision, device=0)
    ls_plan = fr.make_plan(cfg, ofdm, precision=precision, device=0)
    ls_plan.set_mmse_ls(snrs[0])
    kw = dict(fading=fading, seed=3, device=dev)
    routes = {"sweep_omp": lambda: omp_plan.ber_sweep(snrs, frames, **kw),
              "sweep_mmse_ls": lambda: ls_plan.ber_sweep(snrs, frames, **kw),
              "study": lambda: study_plan.estimator_study(snrs, frames, mmse=mmse, **kw)}
    a, b = routes["sweep_omp"](), routes["study"]()
    torch.cuda.synchronize()
    res = {"config": "M", "frames_per_point": frames, "points": len(snrs), "dtype": "f32" if precision == "fp32" else "f64", "mmse": mmse,
           "reps": reps, "n_pilots": study_plan.n_pilots, "taps": len(fading[0]),
           "omp_row_errors_equal_sweep": bool(torch.equal(a["errors"].to(torch.int64), b["errors"][:, 3].to(torch.int64))),
           "BER": [float(x) for x in b["BER"][len(snrs) // 2].tolist()]}
    total = frames * len(snrs)
    for tag, (ms, spread) in alternating(routes, reps).items():
        res[tag] = {"ms": ms, "spread_ms": spread, "frames_per_s": total / (ms * 1e-3)}
    res["study_over_two_sweeps"] = res["study"]["ms"] / (res["sweep_omp"]["ms"] + res["sweep_mmse_ls"]["ms"])
    for p in (study_plan, omp_plan, ls_plan):
        p.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=4096, help="frames per point")
    ap.add_argument("--points", type=int, default=20, help="SNR points, spread over 0 .. 30 dB")
    ap.add_argument("--precision", choices=["fp32", "fp64"], default="fp32")
    ap.add_argument("--mmse", choices=["ls", "genie"], default="ls")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ofdm.init(0)
    snrs = [float(s) for s in np.linspace(0.0, 30.0, a.points)]
    print(json.dumps({"tool": "estimator_study_rate", "result": measure(a.frames, snrs, a.precision, a.mmse, a.reps)}), flush=True)


if __name__ == "__main__":
    main()
