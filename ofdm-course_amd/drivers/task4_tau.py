"""The fine synchroniser's pictures of the `Task 4/README.md` report, replayed on the device over many frames.

Figures 18a and 18b of the report plot `taus`, the residual-delay estimate every pair of adjacent pilots gives
(`Task 4/fine_sync.m:10-30`; the commented lines :10-18 are the plot), against the carrier number: 18a on the clean channel with a
time offset, 18b the same at 25 dB -- the report's argument for averaging tau over all pilots and masking the jumps out
(`fine_sync.m:32-35`).  Here each figure is one `RxPlan.fine_study` call (ofdm_fine_study) of one point on the T4 geometry -- Nfft
1024, 400 carriers, T_Guard 128, 15 % pilots at 4/3 max|dict|, 16QAM, frames of 5 symbols with the Scrambler register of T4:43 reset
per frame --, Time_Delay 12, time sync only (fine_sync(., 1, 0), T4:160): `--frames` frames are generated, synchronised and
demodulated on the GPUs and only the sums come back.  The curve is the mean of taus over the pilots of symbol 2, entries Np ..
2 Np - 2 of `taus` (symbol 1 is blanked by the add_STO pair of T4:292-294), with the share of frames that kept each pair.  The study
is the tau(SNR) companion of drivers/task4_mer.py at the points of T4:137-203, SNR 0:1:40 at Time_Delay 12: per point the mean
|e| of the timing error e = tau Nfft + phi_s + 1 in samples, the share of frames where tau = mean([]) = NaN (and the whole frame
with it), the mean share of pilot pairs the 1e-3 mask keeps, and the histogram of e.

The script's Noise stage is off for figure 18a; the generator always runs Noise, so it runs at CLEAN_SNR_DB = 3000 dB, the convention
of drivers/task3_spectrum.py and drivers/task4_acf.py: the frames are the noise-free ones to rounding.

One process per GPU, as drivers/task2_ccdf.py: the frames of a point are dealt to the ranks in tiles of `--frames-per-tile`
(`sweep.tiles_for_rank`); tile b is the frames b * frames_per_tile .. of every point (fine_study's frame0), so a frame is the same
frame whichever rank draws it.  One SUM all-reduce of the int64 tables (curve_dropped, keep_counts, the histogram and its tails)
and one of the float64 sums (tau_curve_sums, tau_err) end each call; the counts do not depend on the number of GPUs, the sums
only in the order of their last additions (inside a tile they are added in frame order).

    python -m ofdm_course_amd.drivers.task4_tau --json out.json --frames 1000
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \\
        -m ofdm_course_amd.drivers.task4_tau --json out.json --frames 100000
"""
from __future__ import annotations

import argparse
import json
import os

import numpy as np

from .. import sweep
from . import common as c
from .task4_acf import make_plan

CLEAN_SNR_DB = 3000.0
TIME_DELAY = 12                                                                   # T4:148
FIGURES = (("clean", "18a", CLEAN_SNR_DB), ("snr_25dB", "18b", 25.0))
STUDY_SNRS = tuple(float(s) for s in range(0, 41))                                # T4:140 SNRs=(0:1:40)
BINS = dict(n=64, lo=-4.0, hi=4.0)


def check_args(frames, frames_per_tile=4096):
    """What the replay needs of its arguments; the text of the refusal, or None."""
    if frames < 1:
        return "--frames must be >= 1"
    if frames_per_tile < 1:
        return "--frames-per-tile must be >= 1"
    return None


def tiles(frames, frames_per_tile, rank, world):
    """(frame0, frames) of the tiles dealt to this rank: a partition of 0 .. frames - 1 over the ranks."""
    n_tiles = -(-frames // frames_per_tile)
    return [(b * frames_per_tile, min(frames_per_tile, frames - b * frames_per_tile))
            for _, b in sweep.tiles_for_rank(1, n_tiles, rank, world)]


def reduce_over_ranks(counts, sums, device=None):
    """The two collectives of a call: the int64 tables through sweep.all_reduce_counters, the float64 sums through
    sweep.all_reduce_sums (both no-ops on one rank)."""
    box = sweep.Counters(*counts.shape)
    box.errors += counts
    return sweep.all_reduce_counters(box, device=device).errors, sweep.all_reduce_sums(sums, device=device)


def study_call(plan, my_tiles, n_points, L, n_bins, reduce, **kw):
    """fine_study over this rank's tiles, its tables added up and reduced over the ranks.  -> dict of numpy arrays: the int64 tables
    curve_dropped, keep_counts [n, L], tau_hist [n, n_bins], tau_below, tau_above, tau_nan [n] and the float64 tau_curve_sums [n, L],
    tau_err [n, 2], over all frames of all ranks."""
    counts = np.zeros((n_points, 2 * L + n_bins + 3), dtype=np.int64)
    sums = np.zeros((n_points, L + 2), dtype=np.float64)
    for frame0, nf in my_tiles:
        out = plan.fine_study(frames_per_point=nf, frame0=frame0, **kw)
        counts += np.concatenate([_np(out["curve_dropped"]), _np(out["keep_counts"]), _np(out["tau_hist"])] +
                                 [_np(out[k])[:, None] for k in ("tau_below", "tau_above", "tau_nan")], axis=1).astype(np.int64)
        sums += np.concatenate([_np(out["tau_curve_sums"]), _np(out["tau_err"])], axis=1)
    counts, sums = reduce(counts, sums)
    return dict(curve_dropped=counts[:, :L], keep_counts=counts[:, L:2 * L], tau_hist=counts[:, 2 * L:2 * L + n_bins],
                tau_below=counts[:, -3], tau_above=counts[:, -2], tau_nan=counts[:, -1], tau_curve_sums=sums[:, :L],
                tau_err=sums[:, L:])


def figure_args(snr_db):
    """The fine_study arguments of figure 18a / 18b: one point, the time offset, time sync only."""
    return dict(SNRs=[float(snr_db)], Time_Delay=TIME_DELAY, time_desync=1, freq_desync=0, variant="T4")


def study_args():
    """The fine_study arguments of the tau(SNR) study."""
    return dict(SNRs=list(STUDY_SNRS), Time_Delay=TIME_DELAY, time_desync=1, freq_desync=0, variant="T4", bins=dict(BINS))


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def symbol2(n_pilots):
    """Entries Np .. 2 Np - 2 of taus: the pairs of adjacent pilots inside symbol 2."""
    return slice(n_pilots, 2 * n_pilots - 1)


def run(frames=100, seed=1, precision="fp64", Nfft=1024, N_carrier=400, Percent_pilot=15, Constellation="16QAM", Amount_ODFM_SpF=5,
        device_index=0, max_frames_per_chunk=0, lib=None, frames_per_tile=4096, rank=0, world=1, reduce=reduce_over_ranks):
    """Returns (on every rank) {"figures": {name: {figure, SNR_dB, pilot_carriers, tau_curve, tau_curve_samples, keep_rate, tau_nan}},
    "study": {SNR_dB, mean_abs_err, rms_err, nan_share, keep_share, tau_hist, tau_below, tau_above, tau_nan, edges}, ...}: one
    fine_study call per tile of this rank for each figure and for the study, every point on the same payload (key `seed`, frames
    0 ..), reduced over the ranks by `reduce`.  lib: the library module (default: ofdm_course_amd)."""
    bad = check_args(frames, frames_per_tile)
    if bad:
        raise ValueError(bad)
    if lib is None:
        import ofdm_course_amd as lib

    lib.init(device_index)
    dev = f"cuda:{device_index}"
    plan = make_plan(lib, Nfft, N_carrier, Percent_pilot, Constellation, Amount_ODFM_SpF, precision, device_index)
    _, pilotCarriers, _ = c.layout_percent(Nfft, N_carrier, Percent_pilot, tail=2)
    n_pil = len(pilotCarriers)
    common = dict(seed=seed, Register=c.REGISTER, device=dev, max_frames_per_chunk=max_frames_per_chunk)
    mine = tiles(frames, frames_per_tile, rank, world)
    L = n_pil * Amount_ODFM_SpF - 1                                               # numel(taus) of T4/fine_sync.m
    res = {"driver": "Task 4/fine_sync.m:10-35, Task 4/Main_model_Task_4.m:137-203", "frames": frames, "seed": seed,
           "clean_SNR_dB": CLEAN_SNR_DB, "Time_Delay": TIME_DELAY, "Nfft": Nfft, "N_carrier": N_carrier, "T_guard": plan.T_guard,
           "n_pilots": n_pil, "dtype": "f32" if precision == "fp32" else "f64", "n_gpus": world, "frames_per_tile": frames_per_tile,
           "tiles_this_rank": len(mine), "figures": {}}
    sel = symbol2(n_pil)
    for name, figure, snr in FIGURES:
        out = study_call(plan, mine, 1, L, BINS["n"], reduce, bins=dict(BINS), **common, **figure_args(snr))
        sums, drop = out["tau_curve_sums"][0][sel], out["curve_dropped"][0][sel]
        with np.errstate(divide="ignore", invalid="ignore"):
            curve = sums / (frames - drop)
        res["figures"][name] = {"figure": figure, "SNR_dB": float(snr), "pilot_carriers": np.asarray(pilotCarriers)[:-1],
                                "tau_curve": curve, "tau_curve_samples": curve * Nfft,
                                "keep_rate": out["keep_counts"][0][sel] / np.float64(frames), "tau_nan": int(out["tau_nan"][0])}
    out = study_call(plan, mine, len(STUDY_SNRS), L, BINS["n"], reduce, **common, **study_args())
    err, nan = out["tau_err"], out["tau_nan"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        res["study"] = {"SNR_dB": list(STUDY_SNRS), "mean_abs_err": err[:, 0] / (frames - nan), "rms_err": np.sqrt(err[:, 1] / (frames - nan)),
                        "nan_share": nan / frames, "keep_share": out["keep_counts"].sum(axis=1) / float(frames * L),
                        "tau_hist": out["tau_hist"], "tau_below": out["tau_below"], "tau_above": out["tau_above"],
                        "tau_nan": out["tau_nan"], "edges": np.linspace(BINS["lo"], BINS["hi"], BINS["n"] + 1)}
    plan.close()
    return res


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=100, metavar="N", help="frames of 5 symbols per point")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--precision", choices=["fp32", "fp64"], default="fp64")
    ap.add_argument("--frames-per-tile", type=int, default=4096, help="frames of one fine_study call: the unit dealt to the ranks")
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
