"""The integer frequency offset of the `Task 4/README.md` report, replayed on the device over many frames.

Figure 13b is "Влияние шума на оценку целочисленного частотного сдвига", the twin of figure 13a out of the same loop
(`Task 4/Main_model_Task_4.m:113-135`): `|FreqOffset + e_IFO - Freq_Shift|` over SNR 0:1:60 at Time_Delay 150 and Freq_Shift 0.24,
`remove_IFO` run on the received frame with `AutoCorrFunction` beside it (T4:124-125).  Here it is `RxPlan.ifo_study`
(ofdm_ifo_study) with stage="raw" over 61 points on the T4 geometry of drivers/task4_acf.py: the mean of that error over the frames
that have a line above 0.77, and where the pick falls (ifo_hist).

The second study asks why the receiver's remove_IFO (T4:278-303) misses on frames with a drawn offset: both stages at 30 dB with
Time_Delay and Freq_Shift drawn per frame as T4:101-108 draws them.  Per stage it reports the hit rate and the histogram of IFO -
rint(Freq_Shift) (err_hist over -ERR_SPAN .. ERR_SPAN) and, from a second call with the offset held at REL_FREQ_SHIFT (the delay
still drawn), above_rel: how many frames have a bin above 0.77 at each of the bins rint(REL_FREQ_SHIFT) - REL_SPAN .. + REL_SPAN,
beside ifo_rel, the picks in the same bins -- which bins below the line take the pick.

Under `python -m torch.distributed.run` every process takes one GPU and the tiles of `--frames-per-tile` frames dealt to its rank,
as drivers/task4_tau.py deals them; one SUM all-reduce of the int64 tables and one of the float64 sums end each call.

    python -m ofdm_course_amd.drivers.task4_ifo --json out.json --frames 1000
"""
from __future__ import annotations

import argparse
import json
import os

import numpy as np

from .. import sweep
from . import common as c
from .task4_acf import make_plan
from .task4_tau import check_args, reduce_over_ranks, tiles

FIGURE = "13b"
FIG_SNRS = tuple(float(s) for s in range(0, 61))                                  # T4:114 SNRs=(0:1:60)
FIG_TIME_DELAY, FIG_FREQ_SHIFT = 150, 0.24                                        # T4:119,:121
C3_SNR_DB = 30.0
ERR_SPAN = 8
REL_SPAN = 8
REL_FREQ_SHIFT = 12.24
STAGES = ("raw", "receiver")


def figure_args():
    """The ifo_study arguments of figure 13b."""
    return dict(SNRs=list(FIG_SNRS), Time_Delay=FIG_TIME_DELAY, Freq_Shift=FIG_FREQ_SHIFT, stage="raw", time_desync=1, err_span=ERR_SPAN)


def c3_args(stage):
    """The ifo_study arguments of the drawn-offset study of one stage: one point, both draws per frame (T4:101-108)."""
    return dict(SNRs=[C3_SNR_DB], Time_Delay="random", Freq_Shift="random", stage=stage, time_desync=1, err_span=ERR_SPAN)


def rel_args(stage):
    """The same with the offset held at REL_FREQ_SHIFT: every frame's line is expected at one bin."""
    return dict(c3_args(stage), Freq_Shift=REL_FREQ_SHIFT)


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


INT_KEYS = ("spec_dropped", "above_counts", "ifo_hist", "err_hist", "no_line", "err_below", "err_above", "hit", "fallback")
SUM_KEYS = ("spec_sums", "cfo_err")


def study_call(plan, my_tiles, n_points, reduce, **kw):
    """ifo_study over this rank's tiles, its tables added up and reduced over the ranks.  -> dict of numpy arrays over all frames of
    all ranks: the int64 tables of INT_KEYS and the float64 sums of SUM_KEYS."""
    N, ne = plan.Nfft, 2 * kw["err_span"] + 1
    widths = dict(spec_dropped=N, above_counts=N, ifo_hist=N, err_hist=ne, no_line=1, err_below=1, err_above=1, hit=1, fallback=1,
                  spec_sums=N, cfo_err=2)
    counts = np.zeros((n_points, sum(widths[k] for k in INT_KEYS)), dtype=np.int64)
    sums = np.zeros((n_points, sum(widths[k] for k in SUM_KEYS)), dtype=np.float64)
    for frame0, nf in my_tiles:
        out = plan.ifo_study(frames_per_point=nf, frame0=frame0, **kw)
        counts += np.concatenate([_np(out[k]).reshape(n_points, -1) for k in INT_KEYS], axis=1).astype(np.int64)
        sums += np.concatenate([_np(out[k]).reshape(n_points, -1) for k in SUM_KEYS], axis=1)
    counts, sums = reduce(counts, sums)
    res, at = {}, 0
    for k in INT_KEYS:
        res[k] = counts[:, at:at + widths[k]] if widths[k] > 1 else counts[:, at]
        at += widths[k]
    at = 0
    for k in SUM_KEYS:
        res[k] = sums[:, at:at + widths[k]]
        at += widths[k]
    return res


def around(row, centre, span):
    """row[centre - span .. centre + span], zero where that leaves the row."""
    out = np.zeros(2 * span + 1, dtype=row.dtype)
    for i, k in enumerate(range(centre - span, centre + span + 1)):
        if 0 <= k < row.size:
            out[i] = row[k]
    return out


def run(frames=100, seed=1, precision="fp64", Nfft=1024, N_carrier=400, Percent_pilot=15, Constellation="16QAM", Amount_ODFM_SpF=5,
        device_index=0, max_frames_per_chunk=0, lib=None, frames_per_tile=4096, rank=0, world=1, reduce=reduce_over_ranks):
    """Returns (on every rank) {"figure_13b": {figure, SNR_dB, Time_Delay, Freq_Shift, mean_abs_err, rms_err, no_line, fallback,
    ifo_hist}, "c3": {stage: {SNR_dB, hit_rate, no_line_rate, mean_abs_cfo_err, err_hist, err_below, err_above, err_offsets,
    rel_Freq_Shift, rel_bins, above_rel, ifo_rel, rel_hit_rate}}, ...}: one ifo_study call per tile of this rank for the figure and for each stage,
    every point on the same payload (key `seed`, frames 0 ..), reduced over the ranks by `reduce`.  lib: the library module
    (default: ofdm_course_amd)."""
    bad = check_args(frames, frames_per_tile)
    if bad:
        raise ValueError(bad)
    if lib is None:
        import ofdm_course_amd as lib

    lib.init(device_index)
    dev = f"cuda:{device_index}"
    plan = make_plan(lib, Nfft, N_carrier, Percent_pilot, Constellation, Amount_ODFM_SpF, precision, device_index)
    common = dict(seed=seed, Register=c.REGISTER, device=dev, max_frames_per_chunk=max_frames_per_chunk)
    mine = tiles(frames, frames_per_tile, rank, world)
    res = {"driver": "Task 4/remove_IFO.m:5-8, Task 4/Main_model_Task_4.m:113-135,:278-303", "frames": frames, "seed": seed,
           "Nfft": Nfft, "N_carrier": N_carrier, "T_guard": plan.T_guard, "dtype": "f32" if precision == "fp32" else "f64",
           "n_gpus": world, "frames_per_tile": frames_per_tile, "tiles_this_rank": len(mine)}
    kw = figure_args()
    out = study_call(plan, mine, len(FIG_SNRS), reduce, **common, **kw)
    with_line = (frames - out["no_line"]).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        res["figure_13b"] = {"figure": FIGURE, "SNR_dB": kw["SNRs"], "Time_Delay": kw["Time_Delay"], "Freq_Shift": kw["Freq_Shift"],
                             "mean_abs_err": out["cfo_err"][:, 0] / with_line, "rms_err": np.sqrt(out["cfo_err"][:, 1] / with_line),
                             "no_line": out["no_line"], "fallback": out["fallback"], "ifo_hist": out["ifo_hist"]}
    res["c3"] = {}
    for stage in STAGES:
        kw = c3_args(stage)
        out = study_call(plan, mine, 1, reduce, **common, **kw)
        with_line = np.float64(frames - out["no_line"][0])
        with np.errstate(divide="ignore", invalid="ignore"):
            res["c3"][stage] = {"SNR_dB": C3_SNR_DB, "hit_rate": out["hit"][0] / np.float64(frames),
                                "no_line_rate": out["no_line"][0] / np.float64(frames),
                                "mean_abs_cfo_err": out["cfo_err"][0, 0] / with_line, "fallback": int(out["fallback"][0]),
                                "err_hist": out["err_hist"][0], "err_below": int(out["err_below"][0]),
                                "err_above": int(out["err_above"][0]), "err_offsets": list(range(-ERR_SPAN, ERR_SPAN + 1)),
                                }
        rel = study_call(plan, mine, 1, reduce, **common, **rel_args(stage))
        centre = int(np.rint(REL_FREQ_SHIFT))
        res["c3"][stage].update(rel_Freq_Shift=REL_FREQ_SHIFT, rel_bins=list(range(centre - REL_SPAN, centre + REL_SPAN + 1)),
                                above_rel=around(rel["above_counts"][0], centre, REL_SPAN),
                                ifo_rel=around(rel["ifo_hist"][0], centre, REL_SPAN), rel_hit_rate=rel["hit"][0] / np.float64(frames))
    plan.close()
    return res


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=100, metavar="N", help="frames of 5 symbols per point")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--precision", choices=["fp32", "fp64"], default="fp64")
    ap.add_argument("--frames-per-tile", type=int, default=4096, help="frames of one ifo_study call: the unit dealt to the ranks")
    ap.add_argument("--backend", default="nccl", help="nccl = RCCL over xGMI; gloo for rehearsals")
    ap.add_argument("--device", type=int, default=None, help="the GPU of this process (default: its local rank)")
    ap.add_argument("--json", default=None)
    return ap


def parse_args(argv=None):
    """The command line; arguments the replay cannot run with are a usage error."""
    ap = parser()
    a = ap.parse_args(argv)
    bad = check_args(a.frames, a.frames_per_tile)
    if bad:
        ap.error(bad)
    return a


def main(argv=None, lib=None):
    """One process per GPU (RANK / LOCAL_RANK / WORLD_SIZE of torch.distributed.run); rank 0 writes the result.  lib: a stand-in
    for the library (tests): one rank, no process group."""
    a = parse_args(argv)
    rank, local_rank, world = (0, 0, 1) if lib is not None else sweep.dist_env()
    dev_index = local_rank if a.device is None else a.device
    reduce = reduce_over_ranks
    if world > 1:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(dev_index)
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if a.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index))
            reduce = lambda counts, sums: reduce_over_ranks(counts, sums, device=torch.device("cuda", dev_index))  # noqa: E731
        else:
            dist.init_process_group(a.backend)
    res = run(a.frames, a.seed, a.precision, device_index=dev_index, lib=lib, frames_per_tile=a.frames_per_tile, rank=rank,
              world=world, reduce=reduce)
    if rank == 0:
        text = json.dumps(c.to_jsonable(res))
        if a.json:
            with open(a.json, "w") as f:
                f.write(text)
        else:
            print(text, flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
