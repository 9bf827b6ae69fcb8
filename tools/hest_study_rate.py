"""Frames/s of the channel study, one JSON line: the one-call study (RxPlan.channel_study, ofdm_hest_study) against the generator
alone and against the nearest composition a tree without the study has, on the T4 geometry (T4/Main_model_Task_4.m:6-36: Nfft
1024, 400 carriers, T_Guard 128, 15 % pilots, 16QAM, 5 symbols per frame) with the 3-tap channel of T4:252-256, one point at 25 dB,
everything device-resident.

  study_off / study_on   channel_study for all frames with the synchroniser off (no STO / CFO) / on (both drawn per frame): the
                         per-carrier and per-pilot sums, both NMSE figures, the histogram
  generator              tx_frames_fused for the same frames to a device buffer, nothing else
  composition            tx_frames_fused -> rx_chain_task4(mp_desync=1, want_h=True), the synchroniser as in study_on: H_est per
                         frame with the equaliser and the demapper behind it, and no curve.  Other outputs: a yardstick only.
  rows_pass_ms           one device-to-device copy of as many bytes as the study's rows hold for these frames: the cost of one
                         pass over the rows, the allowance of "a study below the composition plus one pass over the rows"

A tree without RxPlan.channel_study reports the generator and the composition only (the figure to put beside the study's).
Median of --reps calls after one warm-up, with the spread (max - min).

    python tools/hest_study_rate.py [--frames 16384] [--precision fp64] [--reps 3]
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

CHANNEL_TAPS = np.array([[0, 1.0], [4, 0.6], [10, 0.3]])          # T4/Main_model_Task_4.m:252-256


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
    h, _ = ofdm.get_MP_channel_resp(CHANNEL_TAPS, 1024)
    imp = dict(Time_Delay="random", Freq_Shift="random")
    res = {"geometry": "T4:6-36", "channel": "T4:252-256", "frames": a.frames, "SNR_dB": 25.0,
           "dtype": "f32" if a.precision == "fp32" else "f64", "reps": a.reps}

    def generator():
        return plan.tx_frames_fused(a.frames, h=h, SNR=25.0, device=dev, **imp)["rx"]

    def composition():
        return ofdm.rx_chain_task4(plan, generator(), time_desync=1, freq_desync=1, mp_desync=1, want_h=True)

    routes = [("generator", generator), ("composition", composition)]
    if hasattr(plan, "channel_study"):
        def study_off():
            return plan.channel_study([25.0], a.frames, h=h, device=dev)

        def study_on():
            return plan.channel_study([25.0], a.frames, h=h, time_desync=1, freq_desync=1, device=dev, **imp)

        st, ch = study_on(), composition()
        He = ch["H"].T
        fin = torch.isfinite(He.real) & torch.isfinite(He.imag)
        res["study_vs_composition_dropped_equal"] = bool(torch.equal(st["dropped"][0], (~fin).sum(dim=0)))
        row_bytes = (33 * plan.N_carrier + 17 * plan.n_pilots) * a.frames
        src = torch.empty(row_bytes, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        ms, spread = timed(lambda: dst.copy_(src), a.reps)
        res["rows_pass_ms"] = {"ms": ms, "spread_ms": spread, "bytes": row_bytes}
        routes = [("study_off", study_off), ("study_on", study_on)] + routes
    for tag, fn in routes:
        ms, spread = timed(fn, a.reps)
        res[tag] = {"ms": ms, "spread_ms": spread, "frames_per_s": a.frames / (ms * 1e-3)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
