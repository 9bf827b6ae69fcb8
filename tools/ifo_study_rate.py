"""Frames/s of the integer-CFO study, one JSON line: the one-call study (RxPlan.ifo_study, ofdm_ifo_study) against the generator
alone and against the nearest composition a tree without the study has, on the T4 geometry (T4/Main_model_Task_4.m:6-36: Nfft
1024, 400 carriers, T_Guard 128, 15 % pilots, 16QAM, 5 symbols per frame), Time_Delay 150, Freq_Shift 0.24 (T4:119-121), one
point at 25 dB, everything device-resident.

  study_raw       ifo_study(stage="raw") for all frames: the summed spectrum, the counts above 0.77, the histograms, the error sums
  study_receiver  the same with stage="receiver": the segment through the STO fix and the rotation by -FreqOffset
  generator       tx_frames_fused for the same frames to a device buffer, nothing else
  composition     tx_frames_fused -> rx_chain_task4(time_desync=1, freq_desync=1, mp_desync=0): IFO and status per frame with the
                  rest of the receiver behind them, and no spectrum.  Other outputs: a yardstick only.

A tree without RxPlan.ifo_study reports the generator and the composition only (the figure to put beside the study's).
Median of --reps calls after one warm-up, with the spread (max - min).

    python tools/ifo_study_rate.py [--frames 16384] [--precision fp64] [--reps 3]
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


def make_plan(precision):
    """The plan of one T4 frame, as drivers/task4_acf.py builds it (restated: the tool also runs on trees without that driver)."""
    _, pilotCarriers, dataCarriers = c.layout_percent(1024, 400, 15, tail=2)
    dict_, _ = ofdm.constellation_func("16QAM")
    amp = 4 / 3 * np.max(np.abs(dict_))
    pv = np.where(np.arange(len(pilotCarriers)) % 2 == 0, amp, -amp).astype(np.complex128)
    return ofdm.RxPlan(1024, 128, 5, 400, pilotCarriers, dataCarriers, pv, 8, 1, "16QAM", precision=precision, device=0)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=16384)
    ap.add_argument("--precision", choices=["fp32", "fp64"], default="fp64")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    ofdm.init(0)
    dev = torch.device("cuda:0")
    plan = make_plan(a.precision)
    imp = dict(Time_Delay=150, Freq_Shift=0.24)
    res = {"geometry": "T4:6-36", "frames": a.frames, "SNR_dB": 25.0, "Time_Delay": 150, "Freq_Shift": 0.24, "dtype": "f32" if a.precision == "fp32" else "f64", "reps": a.reps}

    def generator():
        return plan.tx_frames_fused(a.frames, SNR=25.0, device=dev, **imp)["rx"]

    def composition():
        return ofdm.rx_chain_task4(plan, generator(), time_desync=1, freq_desync=1, mp_desync=0)

    routes = [("generator", generator), ("composition", composition)]
    if hasattr(plan, "ifo_study"):
        def study_raw():
            return plan.ifo_study([25.0], a.frames, stage="raw", device=dev, **imp)

        def study_receiver():
            return plan.ifo_study([25.0], a.frames, stage="receiver", device=dev, **imp)

        st, ch = study_receiver(), composition()
        line = ch["status"] != -1
        res["study_vs_composition_ifo_hist_equal"] = bool(torch.equal(
            st["ifo_hist"][0], torch.bincount(ch["IFO"][line].long(), minlength=plan.Nfft)))
        routes = [("study_raw", study_raw), ("study_receiver", study_receiver)] + routes
    for tag, fn in routes:
        ms, spread = timed(fn, a.reps)
        res[tag] = {"ms": ms, "spread_ms": spread, "frames_per_s": a.frames / (ms * 1e-3)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
