"""The pilot-mask study of `Task 5/Task5_part2.m` on the device: BER and channel-estimate NMSE of OMP equalisation against the
number of pilots, for the regular combs (reg_pilot = 1, :12) or for random masks with the dictionary of all Nfft delays
(reg_pilot = 0, :58-64, :181-184), at SNR 20 dB (:20), and the smallest pilot count whose BER is below 5 % (the figure the
reference's report quotes per delay profile).

Per pilot count ONE `RxPlan.ber_sweep(fading=, want_nmse=True)` call: the fused generator draws a channel realisation per
frame (the Monte-Carlo runs of :148-155), the Task-5 receiver decodes, the bit errors and the NMSE sums are reduced on the
device.  The plan's OMP stage is in "auto" (`RxPlan.set_omp_route`): omp_batch_kernel while its state fits the LDS, else
omp_wide_kernel -- at Nfft 4096 every random-mask count takes the wide kernel.  The counts are dealt round-robin over the ranks
(as `sweep.tiles_for_rank` deals tiles); the bit counts travel in the int64 all-reduce of `sweep`, the NMSE sums in its float64
one.  The Philox key of a count depends on the count only, so the table does not depend on the number of GPUs.

The fading stand-in is NOT `lteFadingChannel` (closed source): `common.fading_profile` takes the public 3GPP delay table, rounds
the delays to samples and draws one random phase per tap and frame.  The thresholds found here are
therefore those of this stand-in and are not expected to equal the report's.

    python -m ofdm_course_amd.drivers.task5_masks --profile ETU --pilots random --json out.json
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \\
        -m ofdm_course_amd.drivers.task5_masks --profile EPA --pilots regular
"""
from __future__ import annotations

import argparse
import json
import os

import numpy as np

from . import common as c
from .task5_part2 import random_pilot_layout, scenario_combs

ROUTE_CODES = {None: 0, "batch": 1, "wide": 2}
ROUTE_NAMES = {v: k for k, v in ROUTE_CODES.items()}


def default_counts(N_carrier=1024):
    """:13-21 -- the distinct pilot counts floor(N_carrier / comb) of the combs 4..256 (`Nps` of the random study too)."""
    return scenario_combs(N_carrier)[1]


def counts_for_rank(n_counts, rank, world):
    """Round-robin deal of the pilot counts (sweep.tiles_for_rank with one batch)."""
    if not (0 <= rank < world):
        raise ValueError("rank outside world")
    return list(range(n_counts))[rank::world]


def threshold(counts, ber, level=0.05):
    """The smallest pilot count whose BER is below `level`; None when no count gets there."""
    ok = [int(n) for n, b in zip(counts, ber) if np.isfinite(b) and b < level]
    return min(ok) if ok else None


def layout(Nfft, N_carrier, n_pilots, pilots, mask_seed):
    """(pilotCarriers, dataCarriers, K) of one pilot count: the first comb with that count and K = ceil(Nfft / comb) (:48-79,
    :183), or a random mask with all Nfft delays (:58-64, :181)."""
    if pilots == "random":
        _, pc, dc, _ = random_pilot_layout(Nfft, N_carrier, n_pilots, mask_seed)
        return pc, dc, Nfft
    combs, amounts = scenario_combs(N_carrier, lo=2, hi=N_carrier)
    hit = np.nonzero(amounts == n_pilots)[0]
    if hit.size == 0:
        raise ValueError(f"no comb gives {n_pilots} pilots in {N_carrier} carriers")
    comb = int(combs[hit[0]])
    _, pc, dc = c.layout_comb(Nfft, N_carrier, comb)
    return pc, dc, int(np.ceil(Nfft / comb))


def run(lib=None, profile="ETU", pilots="random", counts=None, frames=100, Nfft=4096, N_carrier=1024, N_symb=14,
        Constellation="16QAM", SNR_dB=20.0, SamplingRate=4e7, seed=5, precision="fp32", rank=0, world=1, device=None):
    """This rank's share of the study: {"counts", "errors" [n] int64, "bits" [n] int64, "nmse_sums" [n] float64, "routes" [n]
    int64 (ROUTE_CODES of the kernel the OMP stage ran, 0 where another rank holds the count)}; `finish` turns the reduced
    sums into the table."""
    lib = lib or c.default_lib()
    if pilots not in ("regular", "random"):
        raise ValueError("pilots must be 'regular' or 'random'")
    counts = np.asarray(default_counts(N_carrier) if counts is None else counts, dtype=int)
    delays, powers = c.fading_profile(profile, SamplingRate)
    dict_, _ = lib.constellation_func(Constellation)
    amp = 2 * np.max(np.abs(dict_))                                                 # :84-85
    n = len(counts)
    errors, bits, routes = (np.zeros(n, dtype=np.int64) for _ in range(3))
    nmse = np.zeros(n, dtype=np.float64)
    for kk in counts_for_rank(n, rank, world):
        pc, dc, K = layout(Nfft, N_carrier, int(counts[kk]), pilots, [seed, 7, kk])
        if len(dc) == 0:                  # the 100 % rule (a mask whose pilot_step is 1, :67-75) leaves no payload: BER is NaN
            continue
        pv = c.alternating_pilots(amp, len(pc), 1)[:, 0]                            # :86-91
        plan = lib.RxPlan(Nfft, Nfft // 8, N_symb, N_carrier, pc, dc, pv, K, len(delays), Constellation, precision=precision)
        plan.set_omp_route("auto")
        out = plan.ber_sweep([float(SNR_dB)], int(frames), fading=(delays, powers), seeds=[int(seed) + 1000003 * kk],
                             want_nmse=True, device=device)
        errors[kk] = int(np.asarray(_host(out["errors"]))[0])
        bits[kk] = int(out["bits"])
        nmse[kk] = float(np.asarray(_host(out["nmse_sums"]))[0])
        routes[kk] = ROUTE_CODES[plan.last_omp_route]
        plan.close()
    return {"counts": counts, "errors": errors, "bits": bits, "nmse_sums": nmse, "routes": routes,
            "_meta": dict(profile=profile, pilots=pilots, frames=int(frames), Nfft=Nfft, N_carrier=N_carrier, N_symb=N_symb,
                          Constellation=Constellation, SNR_dB=float(SNR_dB), SamplingRate=SamplingRate, seed=seed,
                          precision=precision, delays=np.asarray(delays).tolist(), powers=np.asarray(powers).tolist())}


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def finish(part, world=1):
    """The table from the (reduced) sums of `run`."""
    m = part["_meta"]
    counts = np.asarray(part["counts"])
    ran = np.asarray(part["bits"]) > 0
    ber = np.where(ran, part["errors"] / np.maximum(part["bits"], 1), np.nan)
    nmse = np.where(ran, part["nmse_sums"] / float(max(m["frames"], 1) * m["N_carrier"]), np.nan)   # :202-205, :318
    return {"driver": "Task 5/Task5_part2.m", **m, "n_gpus": int(world), "amounts_pilots": counts.tolist(),
            "errors": part["errors"].tolist(), "bits": part["bits"].tolist(), "BER": ber.tolist(), "NMSE": nmse.tolist(),
            "omp_route": [ROUTE_NAMES[int(r)] for r in part["routes"]], "threshold_level": 0.05,
            "pilots_for_ber_below_5_percent": threshold(counts, ber)}


def reduce_parts(part, device=None):
    """One int64 all-reduce (errors, bits, route codes) and one float64 all-reduce (NMSE sums) over the default process group."""
    from ofdm_course_amd import sweep
    n = len(part["counts"])
    cnt = sweep.Counters(n, 2)
    cnt.errors[:, 0], cnt.errors[:, 1], cnt.bits[:, 0] = part["errors"], part["routes"], part["bits"]
    tot = sweep.all_reduce_counters(cnt, device=device)
    sums = sweep.all_reduce_sums(np.asarray(part["nmse_sums"], dtype=np.float64), device=device)
    return dict(part, errors=tot.errors[:, 0].copy(), routes=tot.errors[:, 1].copy(), bits=tot.bits[:, 0].copy(), nmse_sums=sums)


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--profile", choices=["EPA", "EVA", "ETU"], default="ETU")
    ap.add_argument("--pilots", choices=["regular", "random"], default="random")
    ap.add_argument("--counts", type=int, nargs="*", default=None, help="pilot counts (default: the reference's Nps)")
    ap.add_argument("--frames", type=int, default=100, help="channel realisations per pilot count (monteCarloRuns)")
    ap.add_argument("--nfft", type=int, default=4096)
    ap.add_argument("--n-carrier", type=int, default=1024)
    ap.add_argument("--n-symb", type=int, default=14)
    ap.add_argument("--constellation", default="16QAM")
    ap.add_argument("--snr", type=float, default=20.0)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--precision", choices=["fp32", "fp64"], default="fp32")
    ap.add_argument("--backend", default="nccl", help="nccl = RCCL over xGMI; gloo for rehearsals")
    ap.add_argument("--force-device", type=int, default=None, help="rehearsal only: every rank on this GPU")
    ap.add_argument("--json", default=None)
    return ap


def main(argv=None):
    a = parser().parse_args(argv)
    import torch
    import torch.distributed as dist
    import ofdm_course_amd as ofdm
    from ofdm_course_amd import sweep
    rank, local_rank, world = sweep.dist_env()
    dev_index = local_rank if a.force_device is None else a.force_device
    torch.cuda.set_device(dev_index)
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if a.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index))
        else:
            dist.init_process_group(a.backend)
    ofdm.init(dev_index)
    dev = torch.device("cuda", dev_index)
    part = run(ofdm, a.profile, a.pilots, a.counts, a.frames, a.nfft, a.n_carrier, a.n_symb, a.constellation, a.snr,
               seed=a.seed, precision=a.precision, rank=rank, world=world, device=dev)
    torch.cuda.synchronize()
    res = finish(reduce_parts(part, device=dev if a.backend == "nccl" else None), world)
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
