"""Where the bit errors of the reference's BER figures sit, replayed on the device over many frames.

Every BER the reports show is one number per SNR point (`Task 3/Main_model_Task_3.m:237-266`, `Task 4/Main_model_Task_4.m:354-366`).
`RxPlan.error_study` (ofdm_error_study) keeps the integer tables behind it; three replays:

  t4_carriers     the T4 geometry (T4:6-36) with the 3-tap channel of T4:252-256, 16QAM, scrambled, the channel side: carrier_BER over
                  dataCarriers beside nmse_profile and mean_true_amp of `RxPlan.channel_study` at a few SNRs -- the fades of H and the
                  band edges where the spline of estimate_channel.m:8 extrapolates --, with the synchroniser off and on; with it on
                  symbol_errors shows the first symbol, which the receiver zeroes (T4:292-294).
  t3_labels       the T3 geometry, AWGN, no synchroniser: label_errors per constellation (bit 0 = the MSB of the label): Gray-mapped
                  16QAM and 64QAM protect their label bits unequally.
  t3_descrambler  the T3 geometry with the Register of T3:36 at a high SNR, both sides: DeScrambler.m:8-13 is self-synchronising (the
                  register is fed by the received bit, taps on Register(13) and Register(14)), so one channel error is payload errors
                  at i, i + 13 and i + 14: errors_payload / errors_channel near 3, and peaks of the gap histogram at 1 and 13 on the
                  payload side only.

Under `python -m torch.distributed.run` every process takes one GPU and the tiles of `--frames-per-tile` frames dealt to its rank
through frame0, as drivers/task4_hest.py deals them; one SUM all-reduce of the int64 tables ends each error_study call.

    python -m ofdm_course_amd.drivers.error_anatomy --json out.json --frames 1000
"""
from __future__ import annotations

import argparse
import json
import os

import numpy as np

from .. import sweep
from . import common as c
from . import task4_hest as t4h
from .task4 import CHANNEL_TAPS
from .task4_acf import make_plan
from .task4_tau import check_args, tiles

T4_SNRS = (10.0, 20.0, 30.0)
LABEL_CONSTELLATIONS = ("QPSK", "16QAM", "64QAM")
LABEL_SNRS = (5.0, 10.0, 15.0, 20.0)
DESCR_SNRS = (16.0, 18.0)                                                          # 16QAM in AWGN: one error in a few frames, far apart
GAP_BINS = 64
NFFT, N_CARRIER, PERCENT_PILOT = 1024, 400, 15
INT_KEYS = ("errors", "frames_in_error", "carrier_errors", "symbol_errors", "label_errors", "gap_hist", "gap_above")


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


# ---- the pure table shaping (no GPU, no library)
def widths(nd, n_symb, bps, gap_bins):
    """The columns each table of INT_KEYS takes in the one int64 block a call reduces."""
    return dict(errors=1, frames_in_error=1, carrier_errors=nd, symbol_errors=n_symb, label_errors=bps, gap_hist=gap_bins, gap_above=1)


def join_tables(out, n_points):
    """The tables of one error_study result as one int64 block [n_points, sum(widths)]."""
    return np.concatenate([_np(out[k]).reshape(n_points, -1) for k in INT_KEYS], axis=1).astype(np.int64)


def split_tables(block, w):
    """The inverse of join_tables: dict of [n_points] / [n_points, width] int64 arrays."""
    if block.shape[1] != sum(w[k] for k in INT_KEYS):
        raise ValueError(f"error_anatomy: a block of {block.shape[1]} columns for tables of {sum(w[k] for k in INT_KEYS)}")
    res, at = {}, 0
    for k in INT_KEYS:
        res[k] = block[:, at] if k in ("errors", "frames_in_error", "gap_above") else block[:, at:at + w[k]]
        at += w[k]
    return res


def check_identities(t):
    """The identities of the tables, per point; the text of the first that fails, or None."""
    for k in ("carrier_errors", "symbol_errors", "label_errors"):
        if not np.array_equal(t[k].sum(axis=1), t["errors"]):
            return f"sum({k}) differs from errors"
    if not np.array_equal(t["gap_hist"].sum(axis=1) + t["gap_above"], t["errors"] - t["frames_in_error"]):
        return "sum(gap_hist) + gap_above differs from errors - frames_in_error"
    return None


def rates(t, frames, n_symb, bps):
    """BER, FER and carrier_BER (divided by frames N_symb bps) of the tables of `frames` frames per point."""
    nd = t["carrier_errors"].shape[1]
    return dict(BER=t["errors"] / float(frames * nd * n_symb * bps), FER=t["frames_in_error"] / float(frames),
                carrier_BER=t["carrier_errors"] / float(frames * n_symb * bps))


def carrier_table(t, frames, n_symb, bps, dataCarriers, curves):
    """The first replay's table: carrier_BER over dataCarriers beside the channel study's nmse_profile and mean_true_amp at those
    carriers (curves: task4_hest.curves of the same points, over carriers 1 .. N_carrier)."""
    dc = np.asarray(dataCarriers, np.int64)
    r = rates(t, frames, n_symb, bps)
    return {"dataCarriers": dc, "carrier_BER": r["carrier_BER"], "nmse_profile": curves["nmse_profile"][:, dc - 1],
            "mean_true_amp": curves["mean_true_amp"][:, dc - 1], "symbol_errors": t["symbol_errors"], "BER": r["BER"], "FER": r["FER"]}


def label_table(t, frames, nd, n_symb):
    """label_errors with the BER of each label bit (a label bit is sent frames nd N_symb times per point)."""
    return {"label_errors": t["label_errors"], "label_BER": t["label_errors"] / float(frames * nd * n_symb), "errors": t["errors"]}


def descrambler_table(payload, channel):
    """Both sides of the third replay: the ratio of the error counts (NaN without a channel error) and the gap histograms."""
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = payload["errors"].astype(np.float64) / channel["errors"].astype(np.float64)
    side = lambda t: {"errors": t["errors"], "frames_in_error": t["frames_in_error"], "gap_hist": t["gap_hist"], "gap_above": t["gap_above"],
                      "gap_1": t["gap_hist"][:, 0], "gap_13": t["gap_hist"][:, 12], "gap_14": t["gap_hist"][:, 13]}
    return {"ratio_payload_over_channel": ratio, "payload": side(payload), "channel": side(channel)}


# ---- the calls
def reduce_counts(counts, device=None):
    """The one collective of a call: the int64 block through sweep.all_reduce_counters (a no-op on one rank)."""
    box = sweep.Counters(*counts.shape)
    box.errors += counts
    return sweep.all_reduce_counters(box, device=device).errors


def study_call(plan, my_tiles, n_points, reduce, gap_bins=GAP_BINS, **kw):
    """error_study over this rank's tiles through frame0, the tables added up and reduced over the ranks: one int64 all-reduce."""
    w = widths(plan.n_data, plan.N_symb, plan.bps, gap_bins)
    counts = np.zeros((n_points, sum(w.values())), dtype=np.int64)
    for frame0, nf in my_tiles:
        counts += join_tables(plan.error_study(frames_per_point=nf, frame0=frame0, gap_bins=gap_bins, **kw), n_points)
    t = split_tables(reduce(counts), w)
    bad = check_identities(t)
    if bad:
        raise RuntimeError(f"error_anatomy: {bad}")
    return t


def t4_args(h, sync):
    """The arguments error_study and channel_study share in the first replay; sync: both impairments drawn, both flags on."""
    kw = dict(SNRs=list(T4_SNRS), h=h, time_desync=int(sync), freq_desync=int(sync))
    if sync:
        kw.update(Time_Delay="random", Freq_Shift="random")
    return kw


def run(frames=100, seed=1, precision="fp64", device_index=0, max_frames_per_chunk=0, lib=None, frames_per_tile=4096, rank=0, world=1,
        reduce=reduce_counts, reduce_hest=t4h.reduce_over_ranks):
    """Returns (on every rank) {"t4_carriers": {"sync_off" / "sync_on": carrier_table}, "t3_labels": {constellation: label_table},
    "t3_descrambler": descrambler_table, ...}.  lib: the library module (default: ofdm_course_amd)."""
    bad = check_args(frames, frames_per_tile)
    if bad:
        raise ValueError(bad)
    if lib is None:
        import ofdm_course_amd as lib

    lib.init(device_index)
    dev = f"cuda:{device_index}"
    mine = tiles(frames, frames_per_tile, rank, world)
    common = dict(seed=seed, device=dev, max_frames_per_chunk=max_frames_per_chunk)
    res = {"driver": "Task 3/Main_model_Task_3.m:36,:237-266, Task 4/Main_model_Task_4.m:252-256,:292-294,:354-366, DeScrambler.m:8-13",
           "frames": frames, "seed": seed, "Nfft": NFFT, "N_carrier": N_CARRIER, "dtype": "f32" if precision == "fp32" else "f64",
           "n_gpus": world, "frames_per_tile": frames_per_tile, "tiles_this_rank": len(mine), "gap_bins": GAP_BINS}
    # 1: the T4 geometry behind the 3-tap channel
    plan = make_plan(lib, NFFT, N_CARRIER, PERCENT_PILOT, "16QAM", 5, precision, device_index)
    plan.set_descrambler(c.REGISTER)
    h, _ = lib.get_MP_channel_resp(CHANNEL_TAPS, NFFT)
    res["t4_carriers"] = {"SNR_dB": list(T4_SNRS)}
    for mode, sync in (("sync_off", False), ("sync_on", True)):
        kw = t4_args(h, sync)
        t = study_call(plan, mine, len(T4_SNRS), reduce, receiver="task4", mp_desync=1, side="channel", Register=c.REGISTER, **common, **kw)
        cv = t4h.curves(t4h.study_call(plan, mine, len(T4_SNRS), reduce_hest, bins=t4h.BINS, Register=c.REGISTER, **common, **kw), frames)
        res["t4_carriers"][mode] = carrier_table(t, frames, plan.N_symb, plan.bps, plan.dataCarriers, cv)
    plan.close()
    # 2: the T3 geometry in AWGN, every flag off
    awgn = dict(receiver="task4", time_desync=0, freq_desync=0, mp_desync=0)
    res["t3_labels"] = {"SNR_dB": list(LABEL_SNRS)}
    for const in LABEL_CONSTELLATIONS:
        plan = make_plan(lib, NFFT, N_CARRIER, PERCENT_PILOT, const, 5, precision, device_index)
        t = study_call(plan, mine, len(LABEL_SNRS), reduce, SNRs=list(LABEL_SNRS), **awgn, **common)
        res["t3_labels"][const] = label_table(t, frames, plan.n_data, plan.N_symb)
        plan.close()
    # 3: the Register of T3:36, both sides
    plan = make_plan(lib, NFFT, N_CARRIER, PERCENT_PILOT, "16QAM", 5, precision, device_index)
    plan.set_descrambler(c.REGISTER)
    sides = {side: study_call(plan, mine, len(DESCR_SNRS), reduce, SNRs=list(DESCR_SNRS), side=side, Register=c.REGISTER, **awgn, **common)
             for side in ("payload", "channel")}
    res["t3_descrambler"] = dict(descrambler_table(sides["payload"], sides["channel"]), SNR_dB=list(DESCR_SNRS))
    plan.close()
    return res


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=100, metavar="N", help="frames of 5 symbols per point")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--precision", choices=["fp32", "fp64"], default="fp64")
    ap.add_argument("--frames-per-tile", type=int, default=4096, help="frames of one error_study call: the unit dealt to the ranks")
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
    reduce, reduce_hest = reduce_counts, t4h.reduce_over_ranks
    if world > 1:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(dev_index)
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if a.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index))
            reduce = lambda counts: reduce_counts(counts, device=torch.device("cuda", dev_index))  # noqa: E731
            reduce_hest = lambda counts, sums: t4h.reduce_over_ranks(counts, sums, device=torch.device("cuda", dev_index))  # noqa: E731
        else:
            dist.init_process_group(a.backend)
    res = run(a.frames, a.seed, a.precision, device_index=dev_index, lib=lib, frames_per_tile=a.frames_per_tile, rank=rank, world=world,
              reduce=reduce, reduce_hest=reduce_hest)
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
