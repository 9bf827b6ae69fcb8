"""Frames/s of the error study, one JSON line: RxPlan.error_study (ofdm_error_study) against the existing sweep call with identical
arguments, in the same run on the same card, everything device-resident, one point.

  M    frames.config_M() (Nfft 2048, 512 carriers, comb 4, 64QAM, OMP with 6 taps, 14 symbols), 20480 frames, its 6-tap channel at its
       SNR: ber_sweep against error_study(receiver="task5")
  C3   frames.config_C3() (Nfft 2048, T_guard 256, 800 carriers, 64QAM, 50 symbols), 4096 frames, both impairments drawn per frame
       and every synchroniser flag on: ber_sweep_task4 against error_study(receiver="task4")

The yardstick is the sweep, never the study itself: the two are timed in alternation (sweep, study, sweep, study, ..), the median
of --reps calls each after one warm-up, with the spread (max - min), and the study's errors are compared with the sweep's.  What the
study adds per chunk is one kernel that reads the decisions and the reference bits once.  --map also times the study with the
time-frequency map; --register the scrambled forms, with the study on both sides.

    python tools/error_study_rate.py [--config M C3] [--reps 5] [--map] [--register]
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

REGISTER = (1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0)       # T5/Main_model_Task_5.m:55


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


def measure(name, reps, want_map, register):
    dev = torch.device("cuda:0")
    if name == "M":
        cfg, F = fr.config_M(), 20480
        sweep_name, study = "ber_sweep", dict(receiver="task5")
        imp = {}
    else:
        cfg, F = fr.config_C3(), 4096
        sweep_name, study = "ber_sweep_task4", dict(receiver="task4", time_desync=1, freq_desync=1, mp_desync=1)
        imp = dict(Time_Delay="random", Freq_Shift="random")
    plan = fr.make_plan(cfg, ofdm, precision="fp32", device=0)
    h, _ = ofdm.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    snr = cfg.SNR_dB
    reg = REGISTER if register else None
    if register:
        plan.set_descrambler(REGISTER)
    kw = dict(h=h, seed=3, device=dev, Register=reg, **imp)
    sweep_kw = dict(kw, **{k: v for k, v in study.items() if k != "receiver"}) if name == "C3" else kw
    sweep = lambda: getattr(plan, sweep_name)([snr], F, **sweep_kw)                                   # noqa: E731
    routes = {"sweep": sweep, "study": lambda: plan.error_study([snr], F, **study, **kw)}
    if want_map:
        routes["study_map"] = lambda: plan.error_study([snr], F, want_map=True, **study, **kw)
    if register:
        routes["study_channel"] = lambda: plan.error_study([snr], F, side="channel", **study, **kw)
    a, b = sweep(), routes["study"]()
    torch.cuda.synchronize()
    res = {"config": name, "frames": F, "SNR_dB": snr, "dtype": "f32", "reps": reps, "register": bool(register),
           "errors": int(a["errors"][0].item()), "study_errors_equal_sweep": bool(torch.equal(a["errors"].to(torch.int64), b["errors"].to(torch.int64))),
           "frame_words": plan.frame_bytes // 4, "study_extra_read_bytes": 2 * plan.frame_bytes * F}
    for tag, (ms, spread) in alternating(routes, reps).items():
        res[tag] = {"ms": ms, "spread_ms": spread, "frames_per_s": F / (ms * 1e-3)}
    res["study_over_sweep"] = res["study"]["ms"] / res["sweep"]["ms"]
    plan.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", nargs="+", choices=["M", "C3"], default=["M", "C3"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--map", action="store_true", help="also the study with want_map")
    ap.add_argument("--register", action="store_true", help="scrambled frames, the plan descrambling; the study on both sides")
    a = ap.parse_args()
    ofdm.init(0)
    print(json.dumps({"tool": "error_study_rate", "results": [measure(n, a.reps, a.map, a.register) for n in a.config]}), flush=True)


if __name__ == "__main__":
    main()
