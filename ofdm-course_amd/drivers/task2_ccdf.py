"""The PAPR / CCDF study of `Task 2/Main_model_Task_2.m:69-97` over many signals, sharded over the GPUs of one node.

The script draws its CCDF from ONE signal of 50 symbols: 56 577 strongly correlated windows, a curve that ends near 1e-3
(`drivers/task2.py` replays exactly that).  Here a signal is still the script's -- `--frames-per-signal` frames of 5 symbols,
Nfft 1024, 400 carriers, 1 % pilots at 2 max|dict|, 16QAM (T2:6-24) -- but there are `--signals` of them, generated and counted on
the device by `RxPlan.papr_study` (ofdm_papr_study): no sample and no window value leaves the GPU, only the count table of the
grid `--bins N,LO,HI` (dB), the NaN / out-of-grid counts and each signal's peak and power.  Both curves of T2:78-82 come from one
invocation: `plain` (Register=None) and `scrambled` (the register of T2:36, reset per frame, T2:40-50).

Signals are dealt to the ranks in tiles of `--signals-per-tile` (`sweep.tiles_for_rank`); signal i uses the Philox streams
i * frames_per_signal .. of key `--seed`, so the tables do not depend on the GPU count.  One SUM all-reduce of the int64 count
tables and one of the float64 peaks / powers (a signal's entries are zero on every rank but its owner's) end the study.

With `--payload random` (the Philox draw) the two curves coincide up to their statistical spread: scrambling a uniform random
payload gives a uniform random payload.  The Scrambler only matters for a structured payload such as the image bits of the
reference (`--payload FILE.npz`: `packed` + `n_bits` as tests/golden/eagle_bits.npz holds them, or `bits`; read cyclically, signal
i takes the next frames_per_signal * frame_bits bits), where the plain signal's runs of equal bits pile up into peaks (T2
README: 22-23 dB against about 10 dB).

    python -m ofdm_course_amd.drivers.task2_ccdf --signals 4096
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \\
        -m ofdm_course_amd.drivers.task2_ccdf --signals 65536 --bins 1200,0,30
"""
from __future__ import annotations

import argparse
import json
import math
import os
import time

import numpy as np

from . import common as c

CURVES = (("plain", None), ("scrambled", c.REGISTER))                            # T2:36,:78-82


def parse_bins(text):
    """'N,LO,HI' -> dict(n=, lo=, hi=); ValueError with the reason otherwise."""
    parts = str(text).split(",")
    if len(parts) != 3:
        raise ValueError("--bins must be N,LO,HI")
    try:
        n, lo, hi = int(parts[0]), float(parts[1]), float(parts[2])
    except ValueError:
        raise ValueError("--bins must be N,LO,HI (an integer and two numbers)") from None
    return dict(n=n, lo=lo, hi=hi)


def check_args(signals, frames_per_signal, payload, bins, signals_per_tile=1024):
    """What the study needs of its arguments; the text of the refusal, or None."""
    if signals < 1:
        return "--signals must be >= 1"
    if frames_per_signal < 1:
        return "--frames-per-signal must be >= 1"
    if signals_per_tile < 1:
        return "--signals-per-tile must be >= 1"
    if not (1 <= bins["n"] <= 4096):
        return "--bins: N must be 1 .. 4096"
    if not (math.isfinite(bins["lo"]) and math.isfinite(bins["hi"]) and bins["lo"] < bins["hi"]):
        return "--bins: LO and HI must be finite with LO < HI"
    if payload != "random":
        if not str(payload).endswith(".npz"):
            return "--payload must be 'random' or a .npz file"
        if not os.path.exists(payload):
            return f"--payload: {payload} not found"
    return None


def load_payload(path):
    """The bits of a payload file: `packed` (+ `n_bits`) or `bits`."""
    g = np.load(path)
    if "packed" in g:
        bits = np.unpackbits(g["packed"])
        return bits[: int(g["n_bits"])] if "n_bits" in g else bits
    if "bits" in g:
        return (np.asarray(g["bits"]).ravel() != 0).astype(np.uint8)
    raise ValueError(f"{path}: neither `packed` nor `bits`")


def signal_bits(bits, first_signal, n_signals, per_signal):
    """Signals first_signal .. of a payload read cyclically -> [n_signals, per_signal]."""
    idx = (np.arange(n_signals * per_signal, dtype=np.int64) + int(first_signal) * per_signal) % bits.size
    return bits[idx].reshape(n_signals, per_signal)


def make_plan(lib, Nfft=1024, N_carrier=400, Percent_pilot=1, Constellation="16QAM", Amount_ODFM_SpF=5, precision="fp64",
              device_index=None):
    """The plan of one T2 frame (T2:6-24,:57-58): T_Guard = Nfft / 8, the percent pilot rule, every pilot at 2 max|dict|.  (The
    plan's estimator settings are not used by the study.)"""
    _, pilotCarriers, dataCarriers = c.layout_percent(Nfft, N_carrier, Percent_pilot, tail=2)
    dict_, _ = lib.constellation_func(Constellation)
    amp = 2 * np.max(np.abs(dict_))
    return lib.RxPlan(Nfft, Nfft // 8, Amount_ODFM_SpF, N_carrier, pilotCarriers, dataCarriers,
                      np.full(len(pilotCarriers), amp, dtype=np.complex128), min(8, Nfft), 1, Constellation,
                      precision=precision, device=device_index)


def run(signals=1024, frames_per_signal=10, payload="random", bins=None, seed=1, precision="fp64", signals_per_tile=1024,
        Nfft=1024, N_carrier=400, Percent_pilot=1, Constellation="16QAM", Amount_ODFM_SpF=5, rank=0, world=1, device_index=0,
        backend="nccl"):
    """Returns (on every rank) {"plain": curve, "scrambled": curve, ...}; a curve holds hist [n], below, above, dropped, windows,
    edges [n + 1], CCDF [n + 1], peak / power_sum / PAPR_dB [signals] -- the outputs of RxPlan.papr_study over all signals."""
    import torch
    import ofdm_course_amd as ofdm
    from ofdm_course_amd import sweep

    bins = dict(n=600, lo=0.0, hi=30.0) if bins is None else dict(bins)
    bad = check_args(signals, frames_per_signal, payload, bins, signals_per_tile)
    if bad:
        raise ValueError(bad)
    ofdm.init(device_index)
    dev = torch.device("cuda", device_index)
    plan = make_plan(ofdm, Nfft, N_carrier, Percent_pilot, Constellation, Amount_ODFM_SpF, precision, device_index)
    file_bits = None if payload == "random" else load_payload(payload)
    per_signal = frames_per_signal * plan.frame_bits
    nb = bins["n"]
    n_tiles = -(-signals // signals_per_tile)
    cnt = torch.zeros((len(CURVES), nb + 3), dtype=torch.int64, device=dev)      # bins, then below / above / dropped
    sig = torch.zeros((len(CURVES), signals, 2), dtype=torch.float64, device=dev)
    t0 = time.perf_counter()
    mine = [b for _, b in sweep.tiles_for_rank(1, n_tiles, rank, world)]
    for b in mine:
        s0 = b * signals_per_tile
        ns = min(signals_per_tile, signals - s0)
        pb = None if file_bits is None else signal_bits(file_bits, s0, ns, per_signal)
        for ci, (_, reg) in enumerate(CURVES):
            out = plan.papr_study(ns, frames_per_signal, seed=seed, frame0=s0 * frames_per_signal, Register=reg,
                                  payload_bits=pb, window=Nfft, bins=bins, device=dev)
            cnt[ci, :nb] += out["hist"]
            cnt[ci, nb] += out["below"]
            cnt[ci, nb + 1] += out["above"]
            cnt[ci, nb + 2] += out["dropped"]
            sig[ci, s0:s0 + ns, 0] = out["peak"]
            sig[ci, s0:s0 + ns, 1] = out["power_sum"]
    counters = sweep.Counters(len(CURVES), nb + 3)
    counters.errors += cnt.cpu().numpy()
    sums = sig.cpu().numpy()
    torch.cuda.synchronize()
    local_s = time.perf_counter() - t0
    on = dev if backend == "nccl" else None
    total = sweep.all_reduce_counters(counters, device=on).errors
    sums = sweep.all_reduce_sums(sums, device=on)
    n_sig = frames_per_signal * plan.frame_samples
    res = {"driver": "Task 2/Main_model_Task_2.m:69-97", "signals": signals, "frames_per_signal": frames_per_signal,
           "payload": payload, "bins": bins, "window": Nfft, "seed": seed, "n_gpus": world, "tiles_this_rank": len(mine),
           "seconds_this_rank": local_s, "dtype": "f32" if precision == "fp32" else "f64"}
    edges = np.linspace(bins["lo"], bins["hi"], nb + 1)
    for ci, (tag, _) in enumerate(CURVES):
        hist, below, above, dropped = total[ci, :nb], int(total[ci, nb]), int(total[ci, nb + 1]), int(total[ci, nb + 2])
        valid = int(hist.sum()) + below + above
        exceed = (np.concatenate([np.cumsum(hist[::-1])[::-1], [0]]) + above).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            res[tag] = {"hist": hist, "below": below, "above": above, "dropped": dropped, "windows": valid + dropped,
                        "edges": edges, "CCDF": exceed / np.float64(valid), "peak": sums[ci, :, 0], "power_sum": sums[ci, :, 1],
                        "PAPR_dB": 10.0 * np.log10(sums[ci, :, 0] / (sums[ci, :, 1] / n_sig))}
    return res


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--signals", type=int, default=1024, metavar="N", help="signals per curve")
    ap.add_argument("--frames-per-signal", type=int, default=10, help="frames of 5 symbols per signal (T2:9: 10)")
    ap.add_argument("--payload", default="random", metavar="random|FILE.npz", help="the Philox draw, or a payload file read cyclically")
    ap.add_argument("--bins", default="600,0,30", metavar="N,LO,HI", help="the grid of the count table, dB")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--precision", choices=["fp32", "fp64"], default="fp64")
    ap.add_argument("--signals-per-tile", type=int, default=1024, help="signals of one papr_study call")
    ap.add_argument("--backend", default="nccl", help="nccl = RCCL over xGMI; gloo for rehearsals")
    ap.add_argument("--force-device", type=int, default=None, help="rehearsal only: every rank on this GPU")
    ap.add_argument("--json", default=None)
    return ap


def parse_args(argv=None):
    """The command line; arguments the study cannot run with are a usage error."""
    ap = parser()
    a = ap.parse_args(argv)
    try:
        a.bins = parse_bins(a.bins)
    except ValueError as e:
        ap.error(str(e))
    bad = check_args(a.signals, a.frames_per_signal, a.payload, a.bins, a.signals_per_tile)
    if bad:
        ap.error(bad)
    return a


def main():
    a = parse_args()
    import torch
    import torch.distributed as dist
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
    res = run(a.signals, a.frames_per_signal, a.payload, a.bins, a.seed, a.precision, a.signals_per_tile, rank=rank, world=world,
              device_index=dev_index, backend=a.backend)
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
