"""Windows/s of the Task-2 PAPR / CCDF study, one JSON line: the one-call study (RxPlan.papr_study, ofdm_papr_study) against the
per-function route on the same geometry (T2/Main_model_Task_2.m:6-24: Nfft 1024, 400 carriers, 1 % pilots, 16QAM, 5 symbols per
frame, 10 frames per signal), everything device-resident, fp64.

  per-function   tx_frames(noise off) for all signals -> calculate_window_PAPR per signal (one double per window to HBM) ->
                 calculateCCDF over all window values (hipCUB sort + run-length pass); runs on any commit that has those three
  study          papr_study for all signals, plain curve (Register=None); also with the Scrambler on

    python tools/papr_study_rate.py [--signals 2048] [--route per-function|study|both] [--reps 3]
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
from ofdm_course_amd.drivers import common as c  # noqa: E402


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


def t2_plan(Nfft=1024, N_carrier=400, spf=5):
    _, pil, dat = c.layout_percent(Nfft, N_carrier, 1, tail=2)
    d, _ = ofdm.constellation_func("16QAM")
    return ofdm.RxPlan(Nfft, Nfft // 8, spf, N_carrier, pil, dat, np.full(len(pil), 2 * np.max(np.abs(d)), complex), 8, 1, "16QAM",
                       precision="fp64", device=0)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--signals", type=int, default=2048)
    ap.add_argument("--frames-per-signal", type=int, default=10)
    ap.add_argument("--route", choices=["per-function", "study", "both"], default="both")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    ofdm.init(0)
    dev = torch.device("cuda:0")
    plan = t2_plan()
    n_sig = a.frames_per_signal * plan.frame_samples
    windows = a.signals * (n_sig - plan.Nfft + 1)
    res = {"geometry": "T2:6-24", "signals": a.signals, "frames_per_signal": a.frames_per_signal, "window": plan.Nfft,
           "windows": windows, "dtype": "f64", "reps": a.reps}

    def per_function():
        tx = plan.tx_frames(a.signals * a.frames_per_signal, h=None, SNR=None, seed=1, device=dev)["rx"]   # [frame_samples, frames]
        sig = tx.t().contiguous().view(a.signals, n_sig)
        vals = torch.cat([ofdm.calculate_window_PAPR(sig[s], plan.Nfft) for s in range(a.signals)])
        return ofdm.calculateCCDF(vals)

    if a.route in ("per-function", "both"):
        ms, spread = timed(per_function, a.reps)
        res["per_function"] = {"ms": ms, "spread_ms": spread, "windows_per_s": windows / (ms * 1e-3)}
    if a.route in ("study", "both"):
        for tag, reg in (("study", None), ("study_scrambled", c.REGISTER)):
            ms, spread = timed(lambda: plan.papr_study(a.signals, a.frames_per_signal, seed=1, Register=reg, device=dev), a.reps)
            res[tag] = {"ms": ms, "spread_ms": spread, "windows_per_s": windows / (ms * 1e-3)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
