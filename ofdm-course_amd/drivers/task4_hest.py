"""The channel estimate of the `Task 4/README.md` report, replayed on the device over many frames.

Figure 21 ("Эквализация", `Task 4/Main_model_Task_4.m:318-332`) plots `|H_freq|`, the stems `|Hest_at_pilots|` and the dashed
`|H_est|` over the carrier index for one frame through the 3-tap channel of T4:252-256.  Here it is `RxPlan.channel_study`
(ofdm_hest_study) on the T4 geometry of drivers/task4_acf.py with that channel, one point at 3000 dB (the script's "no noise") and one
at 25 dB: the means of the three curves over the frames.

The profile study runs SNR 0:1:30 with Percent_pilot 15 and 25 and reports, per point, where in the band the error of the estimate
sits -- nmse_profile = sum_f |H - H_est|^2 / frames per carrier, and pilot_err = the same at the pilots before interpolation -- with
both figures of the whole band: NMSE, the plain difference of T4:205-239, and amp_NMSE of (|H_est| - |H|)^2, what figure 21 shows.
It runs once with the synchroniser off (no STO / CFO) and once with it on and both impairments drawn per frame (T4:101-108): there
the plain difference contains the ramp fine_sync removes and does not fall to the noise floor, while amp_NMSE does.

Under `python -m torch.distributed.run` every process takes one GPU and the tiles of `--frames-per-tile` frames dealt to its rank,
as drivers/task4_ifo.py deals them; one SUM all-reduce of the int64 tables and one of the float64 sums end each call.

    python -m ofdm_course_amd.drivers.task4_hest --json out.json --frames 1000
"""
from __future__ import annotations

import argparse
import json
import os

import numpy as np

from .. import sweep
from . import common as c
from .task4 import CHANNEL_TAPS
from .task4_acf import make_plan
from .task4_tau import check_args, reduce_over_ranks, tiles

FIGURE = "21"
FIG_SNRS = (3000.0, 25.0)                                                         # "no noise" and T4:84 SNR_dB = 25
STUDY_SNRS = tuple(float(s) for s in range(0, 31))
STUDY_PERCENT_PILOT = (15, 25)
NFFT, N_CARRIER = 1024, 400
BINS = dict(n=60, lo=-50.0, hi=10.0)


def figure_args(h):
    """The channel_study arguments of figure 21: the 3-tap channel, no STO / CFO, the synchroniser off."""
    return dict(SNRs=list(FIG_SNRS), h=h, time_desync=0, freq_desync=0, bins=BINS)


def study_args(h, sync):
    """The channel_study arguments of the profile study; sync: both impairments drawn per frame and both synchroniser flags on."""
    kw = dict(SNRs=list(STUDY_SNRS), h=h, time_desync=int(sync), freq_desync=int(sync), bins=BINS)
    if sync:
        kw.update(Time_Delay="random", Freq_Shift="random")
    return kw


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


INT_KEYS = ("dropped", "pilot_dropped", "nmse_hist", "nmse_below", "nmse_above", "nmse_nan", "status_counts")
SUM_KEYS = ("est_amp_sums", "true_amp_sums", "err_sums", "amp_err_sums", "pilot_amp_sums", "pilot_err_sums", "nmse_sums", "amp_nmse_sums")


def study_call(plan, my_tiles, n_points, reduce, **kw):
    """channel_study over this rank's tiles, its tables added up and reduced over the ranks.  -> dict of numpy arrays over all frames
    of all ranks: the int64 tables of INT_KEYS and the float64 sums of SUM_KEYS."""
    nc, npil, nb = plan.N_carrier, plan.n_pilots, kw["bins"]["n"]
    widths = dict(dropped=nc, pilot_dropped=npil, nmse_hist=nb, nmse_below=1, nmse_above=1, nmse_nan=1, status_counts=4,
                  est_amp_sums=nc, true_amp_sums=nc, err_sums=nc, amp_err_sums=nc, pilot_amp_sums=npil, pilot_err_sums=npil,
                  nmse_sums=1, amp_nmse_sums=1)
    counts = np.zeros((n_points, sum(widths[k] for k in INT_KEYS)), dtype=np.int64)
    sums = np.zeros((n_points, sum(widths[k] for k in SUM_KEYS)), dtype=np.float64)
    for frame0, nf in my_tiles:
        out = plan.channel_study(frames_per_point=nf, frame0=frame0, **kw)
        counts += np.concatenate([_np(out[k]).reshape(n_points, -1) for k in INT_KEYS], axis=1).astype(np.int64)
        sums += np.concatenate([_np(out[k]).reshape(n_points, -1) for k in SUM_KEYS], axis=1)
    counts, sums = reduce(counts, sums)
    res = {}
    for keys, table in ((INT_KEYS, counts), (SUM_KEYS, sums)):
        at = 0
        for k in keys:
            res[k] = table[:, at:at + widths[k]] if widths[k] > 1 else table[:, at]
            at += widths[k]
    return res


def curves(out, frames):
    """The means of a call over the frames that were kept, carrier by carrier / pilot by pilot."""
    with np.errstate(divide="ignore", invalid="ignore"):
        kept = (frames - out["dropped"]).astype(np.float64)
        pkept = (frames - out["pilot_dropped"]).astype(np.float64)
        return dict(mean_est_amp=out["est_amp_sums"] / kept, mean_true_amp=out["true_amp_sums"] / kept,
                    nmse_profile=out["err_sums"] / kept, amp_profile=out["amp_err_sums"] / kept,
                    pilot_stems=out["pilot_amp_sums"] / pkept, pilot_err=out["pilot_err_sums"] / pkept, frames_kept=kept.min(axis=1))


def run(frames=100, seed=1, precision="fp64", Nfft=NFFT, N_carrier=N_CARRIER, Constellation="16QAM", Amount_ODFM_SpF=5,
        device_index=0, max_frames_per_chunk=0, lib=None, frames_per_tile=4096, rank=0, world=1, reduce=reduce_over_ranks):
    """Returns (on every rank) {"figure_21": {figure, SNR_dB, pilotCarriers, mean_est_amp, mean_true_amp, pilot_stems},
    "study": {Percent_pilot: {"sync_off" / "sync_on": {SNR_dB, NMSE, amp_NMSE, nmse_profile, pilot_err, frames_kept, nmse_nan,
    status_counts}}}, ...}: one channel_study call per tile of this rank for the figure and for each study, every point on the same
    payload (key `seed`, frames 0 ..), reduced over the ranks by `reduce`.  NMSE and amp_NMSE are the means over the frames whose
    estimate is finite, rebuilt from the per-carrier sums (a frame that is not finite would make the per-point sums NaN).  lib: the
    library module (default: ofdm_course_amd)."""
    bad = check_args(frames, frames_per_tile)
    if bad:
        raise ValueError(bad)
    if lib is None:
        import ofdm_course_amd as lib

    lib.init(device_index)
    dev = f"cuda:{device_index}"
    h, _ = lib.get_MP_channel_resp(CHANNEL_TAPS, Nfft)                                # T4:252-260
    common = dict(seed=seed, Register=c.REGISTER, device=dev, max_frames_per_chunk=max_frames_per_chunk)
    mine = tiles(frames, frames_per_tile, rank, world)
    res = {"driver": "Task 4/estimate_channel.m:6-8, Task 4/Main_model_Task_4.m:252-260,:318-332", "frames": frames, "seed": seed,
           "Nfft": Nfft, "N_carrier": N_carrier, "dtype": "f32" if precision == "fp32" else "f64", "n_gpus": world,
           "frames_per_tile": frames_per_tile, "tiles_this_rank": len(mine), "study": {}}
    for pct in STUDY_PERCENT_PILOT:
        plan = make_plan(lib, Nfft, N_carrier, pct, Constellation, Amount_ODFM_SpF, precision, device_index)
        if pct == STUDY_PERCENT_PILOT[0]:
            kw = figure_args(h)
            cv = curves(study_call(plan, mine, len(FIG_SNRS), reduce, **common, **kw), frames)
            res["figure_21"] = {"figure": FIGURE, "SNR_dB": kw["SNRs"], "pilotCarriers": np.asarray(c.layout_percent(Nfft, N_carrier, pct, tail=2)[1], np.int64),
                                "mean_est_amp": cv["mean_est_amp"], "mean_true_amp": cv["mean_true_amp"],
                                "pilot_stems": cv["pilot_stems"]}
        tab = {}
        for mode, sync in (("sync_off", False), ("sync_on", True)):
            kw = study_args(h, sync)
            out = study_call(plan, mine, len(STUDY_SNRS), reduce, **common, **kw)
            cv = curves(out, frames)
            tab[mode] = {"SNR_dB": kw["SNRs"], "NMSE": cv["nmse_profile"].mean(axis=1), "amp_NMSE": cv["amp_profile"].mean(axis=1),
                         "nmse_profile": cv["nmse_profile"], "pilot_err": cv["pilot_err"], "frames_kept": cv["frames_kept"],
                         "nmse_nan": out["nmse_nan"], "status_counts": out["status_counts"]}
        res["study"][str(pct)] = tab
        plan.close()
    return res


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=100, metavar="N", help="frames of 5 symbols per point")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--precision", choices=["fp32", "fp64"], default="fp64")
    ap.add_argument("--frames-per-tile", type=int, default=4096, help="frames of one channel_study call: the unit dealt to the ranks")
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
