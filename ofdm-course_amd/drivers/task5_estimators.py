"""The estimator comparison of Task 5, replayed on the device over many channel realisations.

`Task 5/Task5_part2.m:148-205, :269-304` runs LS_CE, MMSE_CE, MP_estimate and OMP_estimate on the same received frame of every
channel realisation and reports four NMSE and four BER figures per pilot scenario (`Task 5/README.md:68-71, :99-102`);
`Task 5/Main_model_Task_5.m:303-346` does the same over SNR.  Here both are `RxPlan.estimator_study` (ofdm_estimator_study): every
estimator sees the same noise and the same channel, a realisation per frame.  Two replays:

  curves   four BER(SNR) and four NMSE(SNR) curves at one pilot layout (comb `--comb`), SNR 0:0.5:30;
  pilots   four BER and NMSE values per pilot count at 20 dB -- regular combs N_carrier // count, or random masks of `count` pilots
           (`--pilots random`, Task5_part2.m:58-64) -- and, per estimator, the smallest count whose BER is below 5 %: the table of
           `Task 5/README.md:68-71`.

The channel is the tap-delay-line stand-in of drivers/common.py (fading_profile: table delays rounded to samples, a uniform phase
per tap and frame, no Doppler), not lteFadingChannel, whose fractional-delay filter is closed source.  The counts this driver
reports below the 5 % threshold are therefore the driver's own: they need not be the report's 16 / 16 / 8 / 8.

With `--curves` the first replay goes through `RxPlan.estimator_profile` (ofdm_estimator_profile), the same call with the pictures
of `Task 5/Main_model_Task_5.m:207-231, :238-242`: for the SNR points `--curve-snrs` (default 0,10,20,30; points of the 0:0.5:30
grid) the JSON adds, under curves.pictures, |H| and the four |H_est| over the carriers as means over the frames, the error per
carrier, the histogram of the frames' error, and OMP's picks and the channel's taps per delay with the support counts.  Without
`--curves` the output is what it was.

Under `python -m torch.distributed.run` every process takes one GPU and the tiles of `--frames-per-tile` frames dealt to its rank
through `frame0`, as drivers/task4_hest.py deals them; one SUM all-reduce of the int64 tables and one of the float64 sums end each
call.

    python -m ofdm_course_amd.drivers.task5_estimators --profile EPA --json out.json --frames 1000
"""
from __future__ import annotations

import argparse
import json
import os

import numpy as np

from .. import sweep
from . import common as c
from .task4_tau import check_args, reduce_over_ranks, tiles
from .task5_part2 import ESTIMATORS, random_pilot_layout

CURVE_SNRS = tuple(0.5 * i for i in range(61))                                    # 0:0.5:30
TABLE_SNR = 20.0                                                                   # Task5_part2.m:20
BER_THRESHOLD = 0.05                                                               # Task 5/README.md:68-71
NFFT, N_CARRIER, N_SYMB, SAMPLING_RATE = 1024, 640, 7, 4e7                         # (SamplingRate: Task5_part2.m:27-34)
DEFAULT_COUNTS = (8, 16, 32, 64, 128)
MAX_PILOTS = 585                                                                   # the MMSE stage of the estimator body
MMSE_MODES = ("ls", "genie")
PICTURE_SNRS = (0.0, 10.0, 20.0, 30.0)                                             # --curve-snrs
PICTURE_BINS = dict(n=60, lo=-50.0, hi=10.0)


def check_layout(pilots, counts, comb, n_carrier=N_CARRIER, n_paths=1):
    """What the replays need of the pilot arguments; the text of the refusal, or None."""
    if pilots not in ("regular", "random"):
        return "--pilots must be regular or random"
    if not (2 <= comb <= n_carrier // 2):
        return f"--comb must be 2 .. {n_carrier // 2}"
    if n_carrier // comb > MAX_PILOTS:
        return f"--comb {comb} gives {n_carrier // comb} pilots (the MMSE stage takes at most {MAX_PILOTS})"
    if not counts:
        return "--counts needs at least one pilot count"
    for n in counts:
        if not (max(2, n_paths) <= n <= min(MAX_PILOTS, n_carrier // 2)):
            return f"--counts: {n} outside {max(2, n_paths)} .. {min(MAX_PILOTS, n_carrier // 2)} (at least the profile's paths)"
    if list(counts) != sorted(set(counts)):
        return "--counts must be ascending and distinct"
    return None


def layout(pilots, count, nfft=NFFT, n_carrier=N_CARRIER, seed=1):
    """(pilotCarriers, dataCarriers, K) of one scenario: the comb N_carrier // count (its own pilot count may exceed `count`:
    Task5_part2.m:13-17 keeps the first comb of each count) or a random mask of `count` pilots, and the dictionary size: all delays
    a comb can tell apart (Nfft // comb, at most 256) but at least Np columns for MP_estimate.m:10; all Nfft delays for a mask."""
    if pilots == "regular":
        comb = n_carrier // count
        _, pc, dc = c.layout_comb(nfft, n_carrier, comb)
        return pc, dc, max(min(nfft // comb, 256), len(pc))
    _, pc, dc, _ = random_pilot_layout(nfft, n_carrier, count, [seed, 7])
    return pc, dc, nfft


def smallest_count_below(counts, ber, threshold=BER_THRESHOLD):
    """Per estimator the smallest pilot count whose BER is below `threshold` (None: no count is).  ber: [len(counts), 4]."""
    ber = np.asarray(ber, dtype=np.float64)
    out = {}
    for e, name in enumerate(ESTIMATORS):
        hit = [int(n) for n, b in sorted(zip(counts, ber[:, e])) if b < threshold]
        out[name] = hit[0] if hit else None
    return out


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def study_call(plan, my_tiles, n_points, reduce, **kw):
    """estimator_study over this rank's tiles, its tables added up and reduced over the ranks: one int64 table (errors, nmse_dropped)
    and one float64 table (nmse_sums).  -> dict(errors, nmse_dropped [n, 4] int64, nmse_sums [n, 4]) over all frames of all ranks."""
    counts = np.zeros((n_points, 8), dtype=np.int64)
    sums = np.zeros((n_points, 4), dtype=np.float64)
    for frame0, nf in my_tiles:
        out = plan.estimator_study(frames_per_point=nf, frame0=frame0, **kw)
        counts += np.concatenate([_np(out["errors"]), _np(out["nmse_dropped"])], axis=1).astype(np.int64)
        sums += _np(out["nmse_sums"])
    counts, sums = reduce(counts, sums)
    return dict(errors=counts[:, :4], nmse_dropped=counts[:, 4:], nmse_sums=sums)


def check_curve_snrs(snrs):
    """The points of --curve-snrs are points of the curves' grid; the text of the refusal, or None."""
    if not snrs:
        return "--curve-snrs needs at least one SNR"
    for v in snrs:
        if v not in CURVE_SNRS:
            return f"--curve-snrs: {v:g} is not a point of the grid {CURVE_SNRS[0]:g}:{CURVE_SNRS[1] - CURVE_SNRS[0]:g}:{CURVE_SNRS[-1]:g}"
    return None


# the tables of estimator_profile the driver adds up: (key, trailing shape per point as a function of nc, K, T, bins)
_PROFILE_COUNTS = (("errors", lambda nc, K, T, nb: (4,)), ("nmse_dropped", lambda nc, K, T, nb: (4,)),
                   ("nmse_hist", lambda nc, K, T, nb: (4, nb)), ("nmse_below", lambda nc, K, T, nb: (4,)),
                   ("nmse_above", lambda nc, K, T, nb: (4,)), ("nmse_nan", lambda nc, K, T, nb: (4,)),
                   ("pick_hist", lambda nc, K, T, nb: (K,)), ("n_picks_hist", lambda nc, K, T, nb: (T + 1,)),
                   ("true_outside", lambda nc, K, T, nb: ()), ("support_hits", lambda nc, K, T, nb: ()),
                   ("support_misses", lambda nc, K, T, nb: ()), ("support_false", lambda nc, K, T, nb: ()))
_PROFILE_SUMS = (("nmse_sums", lambda nc, K, T, nb: (4,)), ("true_amp_sums", lambda nc, K, T, nb: (nc,)),
                 ("est_amp_sums", lambda nc, K, T, nb: (4, nc)), ("err_sums", lambda nc, K, T, nb: (4, nc)),
                 ("tap_amp_sums", lambda nc, K, T, nb: (K,)), ("true_tap_amp_sums", lambda nc, K, T, nb: (K,)))


def profile_call(plan, my_tiles, n_points, reduce, nc, K, T, bins=PICTURE_BINS, **kw):
    """estimator_profile over this rank's tiles, its tables added up and reduced over the ranks: the new int64 tables join the one
    int64 table of study_call, the new float64 sums its one float64 table.  -> dict of numpy arrays over all frames of all ranks:
    what study_call returns and the tables of _PROFILE_COUNTS / _PROFILE_SUMS, each [n_points, ...]."""
    nb = bins["n"]
    cshape = [(k, f(nc, K, T, nb)) for k, f in _PROFILE_COUNTS]
    sshape = [(k, f(nc, K, T, nb)) for k, f in _PROFILE_SUMS]
    width = lambda shapes: sum(int(np.prod(sh)) for _, sh in shapes)                  # noqa: E731
    flat = lambda out, shapes: np.concatenate([_np(out[k]).reshape(n_points, -1) for k, _ in shapes], axis=1)   # noqa: E731
    counts = np.zeros((n_points, width(cshape)), dtype=np.int64)
    sums = np.zeros((n_points, width(sshape)), dtype=np.float64)
    for frame0, nf in my_tiles:
        out = plan.estimator_profile(frames_per_point=nf, frame0=frame0, bins=bins, **kw)
        counts += flat(out, cshape).astype(np.int64)
        sums += flat(out, sshape)
    counts, sums = reduce(counts, sums)
    res = {}
    for table, shapes in ((counts, cshape), (sums, sshape)):
        at = 0
        for k, sh in shapes:
            n = int(np.prod(sh))
            res[k] = table[:, at:at + n].reshape((n_points,) + sh)
            at += n
    return res


def pictures(out, frames, snrs, bins=PICTURE_BINS):
    """The pictures of the points `snrs` of the curves' grid from profile_call's tables: means over the frames, a dropped frame out
    of its estimator's denominator."""
    at = [CURVE_SNRS.index(v) for v in snrs]
    kept = (frames - out["nmse_dropped"][at]).astype(np.float64)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        res = dict(SNR_dB=list(snrs), mean_true_amp=out["true_amp_sums"][at] / float(frames), mean_est_amp=out["est_amp_sums"][at] / kept,
                   nmse_profile=out["err_sums"][at] / kept, edges_dB=np.linspace(bins["lo"], bins["hi"], bins["n"] + 1),
                   mean_tap_amp=out["tap_amp_sums"][at] / float(frames), mean_true_tap_amp=out["true_tap_amp_sums"][at] / float(frames))
    for k in ("nmse_hist", "nmse_below", "nmse_above", "nmse_nan", "pick_hist", "n_picks_hist", "true_outside", "support_hits",
              "support_misses", "support_false"):
        res[k] = out[k][at]
    return res


def figures(out, frames, frame_bits, n_carrier):
    """BER and NMSE [n, 4] of a call: NMSE as RxPlan.estimator_study forms it, the dropped frames out of the denominator."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return dict(BER=out["errors"] / float(frames * frame_bits),
                    NMSE=out["nmse_sums"] / ((frames - out["nmse_dropped"]).astype(np.float64) * float(n_carrier)),
                    nmse_dropped=out["nmse_dropped"])


def make_plan(lib, pc, dc, K, n_paths, Constellation, n_symb, precision, nfft=NFFT, n_carrier=N_CARRIER):
    dict_, _ = lib.constellation_func(Constellation)
    pilots = c.alternating_pilots(2 * np.max(np.abs(np.asarray(dict_))), len(pc), 1)[:, 0]       # Task5_part2.m:86-91
    return lib.RxPlan(nfft, nfft // 8, n_symb, n_carrier, pc, dc, pilots, K, n_paths, Constellation, precision=precision)


def run(profile="EPA", frames=100, mmse="ls", pilots="regular", counts=DEFAULT_COUNTS, comb=4, seed=1, precision="fp64",
        Constellation="16QAM", device_index=0, max_frames_per_chunk=0, lib=None, frames_per_tile=4096, rank=0, world=1,
        reduce=reduce_over_ranks, curves=False, curve_snrs=PICTURE_SNRS):
    """Returns (on every rank) {"curves": {SNR_dB, comb, n_pilots, BER, NMSE, nmse_dropped} with BER / NMSE [61, 4] in the order of
    `rows`, "pilots": {SNR_dB, layout, counts, n_pilots, BER, NMSE [len(counts), 4], nmse_dropped, smallest_count_below_5_percent},
    ...}: one estimator_study call per tile of this rank and scenario, reduced over the ranks by `reduce`.  lib: the library module
    (default: ofdm_course_amd).  curves: the first replay through estimator_profile, and "curves" gains "pictures" (the dict of
    `pictures`) for the points curve_snrs."""
    delays, powers = c.fading_profile(profile, SAMPLING_RATE)
    bad = check_args(frames, frames_per_tile) or check_layout(pilots, list(counts), comb, N_CARRIER, len(delays)) or \
        (check_curve_snrs(list(curve_snrs)) if curves else None)
    if bad:
        raise ValueError(bad)
    if mmse not in MMSE_MODES:
        raise ValueError("--mmse must be ls or genie")
    if lib is None:
        import ofdm_course_amd as lib
    lib.init(device_index)
    common = dict(fading=(delays, powers), mmse=mmse, seed=seed, device=f"cuda:{device_index}", max_frames_per_chunk=max_frames_per_chunk)
    mine = tiles(frames, frames_per_tile, rank, world)
    res = {"driver": "Task 5/Task5_part2.m:148-205,:269-304, Task 5/Main_model_Task_5.m:303-346", "rows": list(ESTIMATORS),
           "profile": profile, "channel": "tap-delay line of drivers/common.py:fading_profile, not lteFadingChannel", "mmse": mmse,
           "frames": frames, "seed": seed, "Nfft": NFFT, "N_carrier": N_CARRIER, "dtype": "f32" if precision == "fp32" else "f64",
           "n_gpus": world, "frames_per_tile": frames_per_tile, "tiles_this_rank": len(mine)}
    # the curves over SNR at one layout
    _, pc, dc = c.layout_comb(NFFT, N_CARRIER, comb)
    K = max(min(NFFT // comb, 256), len(pc))
    plan = make_plan(lib, pc, dc, K, len(delays), Constellation, N_SYMB, precision)
    if curves:
        out = profile_call(plan, mine, len(CURVE_SNRS), reduce, N_CARRIER, K, len(delays), SNRs=list(CURVE_SNRS), **common)
    else:
        out = study_call(plan, mine, len(CURVE_SNRS), reduce, SNRs=list(CURVE_SNRS), **common)
    fig = figures(out, frames, plan.frame_bits, N_CARRIER)
    plan.close()
    res["curves"] = dict(SNR_dB=list(CURVE_SNRS), comb=comb, n_pilots=len(pc), **fig)
    if curves:
        res["curves"]["pictures"] = dict(K=K, dominant_taps=len(delays), **pictures(out, frames, list(curve_snrs)))
    # the pilot-count table at 20 dB
    ber, nmse, drop, n_pilots = [], [], [], []
    for n in counts:
        pc, dc, K = layout(pilots, n, seed=seed)
        plan = make_plan(lib, pc, dc, K, len(delays), Constellation, N_SYMB, precision)
        fig = figures(study_call(plan, mine, 1, reduce, SNRs=[TABLE_SNR], **common), frames, plan.frame_bits, N_CARRIER)
        plan.close()
        ber.append(fig["BER"][0]); nmse.append(fig["NMSE"][0]); drop.append(fig["nmse_dropped"][0]); n_pilots.append(len(pc))
    res["pilots"] = dict(SNR_dB=TABLE_SNR, layout=pilots, counts=list(counts), n_pilots=n_pilots, BER=np.array(ber), NMSE=np.array(nmse),
                         nmse_dropped=np.array(drop), threshold=BER_THRESHOLD,
                         smallest_count_below_5_percent=smallest_count_below(counts, np.array(ber)))
    return res


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--profile", choices=sorted(c.DELAY_PROFILES), required=True)
    ap.add_argument("--frames", type=int, default=100, metavar="N", help="channel realisations (frames of 7 symbols) per point")
    ap.add_argument("--mmse", choices=MMSE_MODES, default="ls", help="MMSE_CE's h: ifft(H_LS) per frame, or the frame's true taps")
    ap.add_argument("--pilots", choices=["regular", "random"], default="regular", help="the layouts of the pilot-count table")
    ap.add_argument("--counts", type=int, nargs="+", default=list(DEFAULT_COUNTS), help="pilot counts of the table, ascending")
    ap.add_argument("--comb", type=int, default=4, help="the comb of the curves over SNR")
    ap.add_argument("--curves", action="store_true", help="the curves over SNR through estimator_profile, with the per-carrier and "
                    "per-delay pictures of --curve-snrs in the JSON")
    ap.add_argument("--curve-snrs", type=lambda t: [float(v) for v in t.split(",") if v], default=list(PICTURE_SNRS), metavar="A,B,..",
                    help="the SNR points of the pictures, points of the grid 0:0.5:30 (default 0,10,20,30)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--precision", choices=["fp32", "fp64"], default="fp64")
    ap.add_argument("--frames-per-tile", type=int, default=4096, help="frames of one estimator_study call: the unit dealt to the ranks")
    ap.add_argument("--backend", default="nccl", help="nccl = RCCL over xGMI; gloo for rehearsals")
    ap.add_argument("--device", type=int, default=None, help="the GPU of this process (default: its local rank)")
    ap.add_argument("--json", default=None)
    return ap


def parse_args(argv=None):
    """The command line; arguments the replays cannot run with are a usage error."""
    ap = parser()
    a = ap.parse_args(argv)
    bad = check_args(a.frames, a.frames_per_tile) or check_layout(a.pilots, a.counts, a.comb, N_CARRIER,
                                                                  len(c.fading_profile(a.profile, SAMPLING_RATE)[0])) or \
        (check_curve_snrs(a.curve_snrs) if a.curves else None)
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
    res = run(a.profile, a.frames, a.mmse, a.pilots, tuple(a.counts), a.comb, a.seed, a.precision, device_index=dev_index, lib=lib,
              frames_per_tile=a.frames_per_tile, rank=rank, world=world, reduce=reduce, curves=a.curves, curve_snrs=tuple(a.curve_snrs))
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
