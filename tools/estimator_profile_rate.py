"""What the estimator profile costs on top of the estimator study, one JSON line: RxPlan.estimator_profile (ofdm_estimator_profile)
against RxPlan.estimator_study (ofdm_estimator_study) with identical arguments on the shapes of tools/estimator_study_rate.py --
config M's geometry (Nfft 2048, 512 carriers, comb 4 = 128 pilots, K 128, 64QAM, 14 symbols) on the EPA tap-delay line at
30.72 MHz, a channel per frame, everything device-resident.

The profile is the study's call with three kernels behind each chunk (the per-carrier sums read the four H buffers once more), so
the ratio is the cost of the pictures.  The two are timed in alternation in the same run on the same card, the median of --reps
calls each after one warm-up, with the spread (max - min); the study's tables of both are compared bit for bit.

    python tools/estimator_profile_rate.py [--frames 4096] [--points 20] [--precision fp32] [--mmse ls] [--reps 5]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ofdm_course_amd as ofdm  # noqa: E402
from ofdm_course_amd import frames as fr  # noqa: E402
from ofdm_course_amd.drivers import common as c  # noqa: E402
from estimator_study_rate import alternating  # noqa: E402


def measure(frames, snrs, precision, mmse, reps):
    dev = torch.device("cuda:0")
    cfg = fr.config_M()
    fading = c.fading_profile("EPA", 30.72e6)
    study_plan = fr.make_plan(cfg, ofdm, precision=precision, device=0)
    profile_plan = fr.make_plan(cfg, ofdm, precision=precision, device=0)
    kw = dict(fading=fading, seed=3, device=dev, mmse=mmse)
    routes = {"study": lambda: study_plan.estimator_study(snrs, frames, **kw),
              "profile": lambda: profile_plan.estimator_profile(snrs, frames, **kw)}
    a, b = routes["study"](), routes["profile"]()
    torch.cuda.synchronize()
    res = {"config": "M", "frames_per_point": frames, "points": len(snrs), "dtype": "f32" if precision == "fp32" else "f64", "mmse": mmse,
           "reps": reps, "n_pilots": study_plan.n_pilots, "taps": len(fading[0]),
           "study_tables_equal": bool(all(torch.equal(a[k], b[k]) for k in ("errors", "nmse_sums", "nmse_dropped")))}
    total = frames * len(snrs)
    for tag, (ms, spread) in alternating(routes, reps).items():
        res[tag] = {"ms": ms, "spread_ms": spread, "frames_per_s": total / (ms * 1e-3)}
    res["profile_over_study"] = res["profile"]["ms"] / res["study"]["ms"]
    for p in (study_plan, profile_plan):
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
    print(json.dumps({"tool": "estimator_profile_rate", "result": measure(a.frames, snrs, a.precision, a.mmse, a.reps)}), flush=True)


if __name__ == "__main__":
    main()
