"""Frames/s of the received-spectrum study, one JSON line: the one-call study (RxPlan.spectrum_study, ofdm_spectrum_study) against
the generator alone and against the per-function route on the same tree, on the T3 geometry (T3/Main_model_Task_3.m:6-24: Nfft
1024, 400 carriers, 15 % pilots, 16QAM, 5 symbols per frame), AWGN at 25 dB, one point, everything device-resident.

  study          spectrum_study(first = T_guard, n_windows) for all frames: power per bin summed over the frames
  generator      tx_frames_fused for the same frames to a device buffer, nothing else
  per-function   tx_frames_fused -> torch.fft.fft of the n_windows slices of every frame -> abs()^2 -> sum over windows and frames

Median of --reps calls after one warm-up, with the spread (max - min).

    python tools/spectrum_study_rate.py [--frames 16384] [--windows 1] [--precision fp64] [--reps 3]
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
from ofdm_course_amd.drivers import task3_spectrum as t3s  # noqa: E402


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(max(ms) - min(ms))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=16384)
    ap.add_argument("--windows", type=int, default=1)
    ap.add_argument("--precision", choices=["fp32", "fp64"], default="fp64")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    ofdm.init(0)
    dev = torch.device("cuda:0")
    plan = t3s.make_plan(ofdm, precision=a.precision, device_index=0)
    N, tg, nw, stride = plan.Nfft, plan.T_guard, a.windows, plan.Nfft + plan.T_guard
    res = {"geometry": "T3:6-24", "frames": a.frames, "windows": nw, "SNR_dB": 25.0, "dtype": "f32" if a.precision == "fp32" else "f64",
           "reps": a.reps}

    def study():
        return plan.spectrum_study([25.0], a.frames, first=tg, n_windows=nw, device=dev)["power_sums"]

    def generator():
        return plan.tx_frames_fused(a.frames, SNR=25.0, device=dev)["rx"]

    def per_function():
        rx = generator().t()                                             # [frames, frame_samples], contiguous
        seg = torch.stack([rx[:, tg + w * stride: tg + w * stride + N] for w in range(nw)], dim=1)
        S = torch.fft.fft(seg, dim=2)
        return (S.real.double() ** 2 + S.imag.double() ** 2).sum(dim=(0, 1))

    want, got = per_function(), study()[0]
    res["study_vs_per_function_rel_l2"] = float(torch.linalg.norm(got - want) / torch.linalg.norm(want))
    for tag, fn in (("study", study), ("generator", generator), ("per_function", per_function)):
        ms, spread = timed(fn, a.reps)
        res[tag] = {"ms": ms, "spread_ms": spread, "frames_per_s": a.frames / (ms * 1e-3)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
