"""Monte-Carlo BER(SNR) sweep of the fused Task-5 RX chain, sharded over the GPUs of one node (SURVEY.md 8e;
BASELINE config 5: Nfft 8192, 256-QAM, sparse 32-tap channel, OMP_estimate, 20 SNR points over 8 GPUs).

The reference's sweeps are loops over independent SNR points (T5/Main_model_Task_5.m:303-346,
T3/Main_model_Task_3.m:237-268).  Here every (snr_idx, batch_idx) tile is one unit: tiles are dealt round-robin
to the ranks (`sweep.tiles_for_rank`), each tile generates its frames on its own GPU (`ofdm_tx_frames`: payload -> TX ->
multipath -> Noise, Philox streams keyed by the tile, so the table does not depend on the GPU count; nothing is drawn
or packed on the host), runs `rx_chain_task5`, and adds
its error / bit counts to a device table that is read once.  One SUM all-reduce of the int64 counters (and one of the
float64 sums, when there are any) ends the sweep -- no samples are exchanged.

--fused (opt-in): the reference's order, Noise -> conv(h) (T5/Task5_part2.m:134,:152), through `RxPlan.ber_sweep`
(ofdm_ber_sweep_task5: the three-pass generator + the chain + a device reduction, one call for the points a rank holds of a
batch, the same tile keys).

--config C3: the Task-4 receiver (coarse sync, IFO, fine sync, spline equaliser; T4/Main_model_Task_4.m:99-134,:278-347) on
frames with a random STO / CFO per frame, through `RxPlan.ber_sweep_task4` (ofdm_ber_sweep_task4), with the same tile keys
and dealing as --fused.  Per point the JSON adds `status_counts` (frames with receiver status 0, 1, -1, -2) and
`cfo_abs_err` (the sum of |FreqOffset + IFO - Freq_Shift| over the point's frames).  The integer counters travel in the int64
all-reduce; the CFO sums in a second, float64 one.  --mer adds per point `mer_sums` and `MER_dB`, the MER of the point's
frames: at C3 MER_func of RX_IQ(Nfft+T_Guard+1:end) per frame, concatenated (ofdm_ber_sweep_task4_ex), beside the CFO sums;
at C5 / M MER_func of each frame's whole RX_IQ (T5/Main_model_Task_5.m:282; ofdm_ber_sweep_task5_ex with --fused,
rx_chain_task5(want_mer) per tile otherwise).  The two MER_func sums travel in a float64 all-reduce.

--fused --fading {EPA,EVA,ETU} (C5 / M): a channel realisation per frame instead of the one channel cfg.taps -- the Monte-Carlo
runs of T5/Task5_part2.m:148-155 at sweep rate, through `RxPlan.ber_sweep(fading=common.fading_profile(...))`
(ofdm_ber_sweep_task5_fading), with the same tile keys and dealing.  The profile's delays are taken at FADING_SAMPLING_RATE; the
OMP estimator sees a delay only below the plan's K dictionary columns (ETU's last taps lie beyond M's 128: an error floor, as
for any echo the dictionary cannot hold).  --nmse adds per point `nmse_sums` and `NMSE`, the channel-estimate error against
fft(h_f) on carriers 1..N_carrier averaged over the point's frames (T5/Task5_part2.m:202-205,:318); the sums are doubles and
travel in the float64 all-reduce.  The JSON line names the profile under "fading".

--estimator mmse-ls (C5 / M): MMSE_CE with h = ifft(H_est_LS) per frame, the call of T5/Main_model_Task_5.m:178-180 and
:317-319 (`RxPlan.set_mmse_ls`): no channel is handed to the receiver, every point is estimated at its own SNR, and the plan
decodes all points of a batch in one call with --fused, with --fading, --mer and --nmse as for omp.  (--estimator mmse is the
fixed-h form of T5/Task5_part2.m:176-177: one point per call, no --fading.)  The JSON line names the estimator.

--fused --random-pilots NP [--mask-seed S] [--dictionary full] (M): the random-mask study of T5/Task5_part2.m:58-64 at sweep
rate.  The plan's pilots are a sorted random mask of NP carriers in 1..N_carrier (`task5_part2.random_pilot_layout`, seeded by
--mask-seed); --dictionary full gives the estimator all Nfft delays (K = Nfft, :181-184) and puts the plan's OMP stage in "auto"
(`RxPlan.set_omp_route`): omp_batch_kernel while its state fits the LDS, else omp_wide_kernel.  The JSON line carries "pilots":
"random", "n_pilots", "mask_seed", "K" and "omp_route", the kernel the OMP stage ran.

--fused --density BINS [--half-width L] (C5 / M): per point the constellation of the receiver as a density, a BINS x BINS grid
on [-L, L)^2 of every equalised point RX_IQ of the point's frames (rows: im, columns: re; the scatter of
T5/Main_model_Task_5.m:248-251 over the points MER_func sums at :282), accumulated on the device by the symbol stage
(`RxPlan.ber_sweep(density=...)`, ofdm_ber_sweep_task5_scope).  L defaults to 1.5 max|dict|.  The JSON line adds `density`
(one grid per point), `density_dropped` (points with a non-finite coordinate, not binned), `density_points` (the points counted
per SNR), `density_bins` and `half_width`; the grids are integers and travel in the int64 all-reduce.  With --fading,
--estimator mmse-ls and --random-pilots as without it.  (The Task-4 receiver's density is `task4_mer --density`.)

    python -m ofdm_course_amd.drivers.sweep_ber --config C5 --batches 4 --frames-per-tile 64
    python -m ofdm_course_amd.drivers.sweep_ber --config C3 --batches 4 --frames-per-tile 256
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \\
        -m ofdm_course_amd.drivers.sweep_ber --config C5 --batches 16
"""
from __future__ import annotations

import argparse
import json
import os
import time

import numpy as np

FADING_SAMPLING_RATE = 30.72e6          # samples/s the delay profiles are rounded at: LTE 20 MHz, the rate of Nfft 2048


def check_fading(config, estimator, fused, fading, nmse):
    """What --fading / --nmse need; the text of the refusal, or None."""
    if nmse and fading is None:
        return "--nmse needs --fading"
    if fading is None:
        return None
    if not fused:
        return "--fading needs --fused"
    if config not in ("C5", "M"):
        return "--fading is for the Task-5 receiver (configs C5 and M)"
    if estimator not in ("omp", "mmse-ls"):
        return "--fading needs the OMP or the mmse-ls estimator (a fixed-h MMSE plan is built for one channel)"
    return None


def check_pilots(config, estimator, fused, random_pilots, dictionary):
    """What --random-pilots / --dictionary full need; the text of the refusal, or None."""
    if random_pilots is None and dictionary != "full":
        return None
    if not fused:
        return "--random-pilots / --dictionary full need --fused"
    if config != "M":
        return "--random-pilots / --dictionary full are for config M (the wide OMP route is not built for Nfft 8192)"
    if estimator != "omp":
        return "--random-pilots / --dictionary full need the OMP estimator"
    if random_pilots is not None and random_pilots < 3:
        return "--random-pilots needs at least 3 pilots"
    return None


def check_density(config, fused, density, half_width):
    """What --density / --half-width need; the text of the refusal, or None."""
    if half_width is not None and density is None:
        return "--half-width needs --density"
    if density is None:
        return None
    if config == "C3" or not fused:
        return ("--density needs --fused at config C5 or M (the Task-5 receiver's sweep); the Task-4 receiver's density is "
                "`python -m ofdm_course_amd.drivers.task4_mer --density`")
    return None


def apply_pilots(cfg, random_pilots, mask_seed, dictionary):
    """The frame configuration with the random mask (T5/Task5_part2.m:58-64) and / or the dictionary of all Nfft delays."""
    from ofdm_course_amd.drivers.task5_part2 import random_pilot_layout
    if random_pilots is not None:
        cfg.pilots = random_pilot_layout(cfg.Nfft, cfg.N_carrier, random_pilots, mask_seed)[1]
        if cfg.K_atoms is None:
            cfg.K_atoms = int(np.ceil(cfg.N_carrier / cfg.comb))       # the comb's dictionary, unless --dictionary full
    if dictionary == "full":
        cfg.K_atoms = cfg.Nfft                                         # :181 F = dftmtx(Nfft), all columns
    return cfg


def make_sweep_plan(cfg, lib, precision, device_index, dictionary="comb"):
    """The plan of the sweep; with the dictionary of all Nfft delays its OMP stage may take the wide kernel ("auto")."""
    from ofdm_course_amd import frames as fr
    plan = fr.make_plan(cfg, lib, precision=precision, device=device_index)
    if dictionary == "full":
        plan.set_omp_route("auto")
    return plan


def run(config="C5", snrs=None, batches=2, frames_per_tile=32, precision="fp32", seed=7, estimator="omp",
        rank=0, world=1, device_index=0, backend="nccl", fused=False, mer=False, fading=None, nmse=False,
        random_pilots=None, mask_seed=1, dictionary="comb", density=None, half_width=None):
    """Returns (on every rank) the reduced table {"SNRs", "errors", "bits", "BER", ...}; with density=BINS also density
    [n, BINS, BINS] (rows: im, columns: re), density_dropped [n], density_points, density_bins and half_width.
    Per batch of the tiles this rank holds, one call decodes one tile (rx_chain_task5 on make_frames_device frames, or
    ber_sweep for an MMSE plan, which is built for one SNR) or all of the batch's points (ber_sweep with --fused,
    ber_sweep_task4 at C3)."""
    import torch
    import ofdm_course_amd as ofdm
    from ofdm_course_amd import frames as fr
    from ofdm_course_amd import sweep
    from ofdm_course_amd.drivers.common import fading_profile

    bad = check_fading(config, estimator, fused, fading, nmse) or check_pilots(config, estimator, fused, random_pilots, dictionary) or \
        check_density(config, fused, density, half_width)
    if bad:
        raise ValueError(bad)
    ofdm.init(device_index)
    dev = torch.device("cuda", device_index)
    cfg = {"C5": fr.config_C5, "M": fr.config_M, "C3": fr.config_C3}[config]()
    snrs = np.arange(0.0, 30.0, 1.5) if snrs is None else np.asarray(snrs, dtype=float)      # 20 points
    cfg = apply_pilots(cfg, random_pilots, mask_seed, dictionary)
    plan = make_sweep_plan(cfg, ofdm, precision, device_index, dictionary)
    task4 = config == "C3"
    h, _ = ofdm.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    if estimator == "mmse":
        hh = np.zeros(cfg.N_carrier, dtype=np.complex128)
        hh[: len(h)] = h
    n = len(snrs)
    # int64 columns: bit errors (+ C3: frames with receiver status 0, 1, -1, -2); float64 columns: (C3: the sum of
    # |FreqOffset + IFO - Freq_Shift|) (+ mer: the MER_func sums s1, s2) (+ nmse: the channel-estimate error sums) -- one
    # device table each, read once
    # (+ density: the bins x bins grid of the point and its dropped points, behind them)
    c_dens = 5 if task4 else 1
    n_dens = 0
    if density is not None:
        density = int(density)
        n_dens = max(density, 0) ** 2
        half_width = 1.5 * float(np.max(np.abs(ofdm.constellation_func(cfg.Constellation)[0]))) if half_width is None else float(half_width)
    cnt = torch.zeros((n, c_dens + (n_dens + 1 if density is not None else 0)), dtype=torch.int64, device=dev)
    c_mer = int(task4)
    c_nmse = c_mer + (2 if mer else 0)
    flt = torch.zeros((n, c_nmse + int(nmse)), dtype=torch.float64, device=dev)
    profile = fading_profile(fading, FADING_SAMPLING_RATE) if fading else None
    counters = sweep.Counters(n, cnt.shape[1])
    t0 = time.perf_counter()
    n_tiles = 0
    by_batch = {}
    for si, bi in sweep.tiles_for_rank(n, batches, rank, world):
        by_batch.setdefault(bi, []).append(si)
    for bi, sis in by_batch.items():
        keys = [sweep.tile_seed_stream(seed, si, bi, frames_per_tile) for si in sis]
        whole = task4 or (fused and estimator != "mmse")
        if estimator == "mmse-ls" and not task4 and whole:
            plan.set_mmse_ls(cfg.SNR_dB)                       # (the sweep estimates every point at the point's own SNR)
        for g in [list(range(len(sis)))] if whole else [[i] for i in range(len(sis))]:
            pts = [sis[i] for i in g]
            seeds, stream0 = [keys[i][0] for i in g], keys[g[0]][1]
            if task4:                                          # random STO / CFO, all three desync stages on
                out = plan.ber_sweep_task4(snrs[pts], frames_per_tile, h=h, Time_Delay="random", Freq_Shift="random",
                                           seeds=seeds, frame0=stream0, device=dev, want_mer=mer,
                                           mer_skip=cfg.Nfft + cfg.T_guard)
                cnt[pts, 1:] += out["status_counts"]
                flt[pts, 0] += out["cfo_abs_err"]
                errors, mer_sums = out["errors"], out.get("mer_sums")
            elif fused:
                if estimator == "mmse":
                    plan.set_mmse(hh, float(snrs[pts[0]]))
                chan = dict(fading=profile, want_nmse=nmse) if fading else dict(h=h)
                if density is not None:
                    chan["density"] = dict(bins=density, half_width=half_width, skip=0)
                out = plan.ber_sweep(snrs[pts], frames_per_tile, seeds=seeds, frame0=stream0, device=dev, want_mer=mer, **chan)
                errors, mer_sums = out["errors"], out.get("mer_sums")
                if density is not None:
                    cnt[pts, c_dens:c_dens + n_dens] += out["density"].view(torch.int64).reshape(len(pts), n_dens)
                    cnt[pts, c_dens + n_dens] += out["density_dropped"].view(torch.int64)
                if nmse:
                    flt[pts, c_nmse] += out["nmse_sums"]
            else:
                cfg.SNR_dB = float(snrs[pts[0]])
                data = fr.make_frames_device(cfg, ofdm, plan, frames_per_tile, seed=seeds[0], device=dev, frame0=stream0)
                if estimator == "mmse":
                    plan.set_mmse(hh, cfg.SNR_dB)
                elif estimator == "mmse-ls":
                    plan.set_mmse_ls(cfg.SNR_dB)
                out = ofdm.rx_chain_task5(plan, data["rx"], ref_bits_packed=data["packed"], want_mer=mer)
                errors, mer_sums = out["errors"].sum(), out["mer_sums"].sum(dim=0) if mer else None
            cnt[pts, 0] += errors
            if mer:
                flt[pts, c_mer:c_mer + 2] += mer_sums
        n_tiles += len(sis)
        for si in sis:
            counters.add(si, 0, 0, frames_per_tile * plan.frame_bits)
    counters.errors += cnt.cpu().numpy()
    sums = flt.cpu().numpy()
    torch.cuda.synchronize()
    local_s = time.perf_counter() - t0
    on = dev if backend == "nccl" else None
    total = sweep.all_reduce_counters(counters, device=on)
    sums = sweep.all_reduce_sums(sums, device=on)
    errors, bits = total.errors[:, 0], total.bits[:, 0]
    res = {"config": config, "estimator": "task4" if task4 else estimator, "SNRs": snrs.tolist(), "errors": errors.tolist(),
           "bits": bits.tolist(), "BER": (errors / np.maximum(bits, 1)).tolist()}
    if task4:
        res.update(status_counts=total.errors[:, 1:].tolist(), cfo_abs_err=sums[:, 0].tolist())
    res.update(batches=batches, frames_per_tile=frames_per_tile, n_gpus=world, tiles_this_rank=n_tiles,
               seconds_this_rank=local_s, dtype="f32" if precision == "fp32" else "f64")
    if task4:
        res.update(order="noise_first", impairments={"Time_Delay": "random", "Freq_Shift": "random"})
    elif fused:
        res.update(order="noise_first", fused=True)
    if random_pilots is not None:
        res.update(pilots="random", n_pilots=int(random_pilots), mask_seed=int(mask_seed))
    if random_pilots is not None or dictionary == "full":
        res.update(K=int(cfg.K), omp_route=plan.last_omp_route)
    if fading:
        res["fading"] = {"profile": fading, "sampling_rate": FADING_SAMPLING_RATE, "delays": profile[0].tolist(),
                         "powers": profile[1].tolist()}
    if nmse:
        res["nmse_sums"] = sums[:, c_nmse].tolist()
        res["NMSE"] = (sums[:, c_nmse] / (batches * frames_per_tile * cfg.N_carrier)).tolist()
    if mer:
        m = sums[:, c_mer:c_mer + 2]
        res["mer_sums"] = m.tolist()
        res["MER_dB"] = (10.0 * np.log10(m[:, 0] / m[:, 1])).tolist()
    if density is not None:
        res.update(density=total.errors[:, c_dens:c_dens + n_dens].reshape(n, density, density).tolist(),
                   density_dropped=total.errors[:, c_dens + n_dens].tolist(),
                   density_points=batches * frames_per_tile * plan.frame_bits // plan.bps, density_bins=density,
                   half_width=half_width)
    return res


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=["C5", "M", "C3"], default="C5")
    ap.add_argument("--batches", type=int, default=2, help="tiles per SNR point")
    ap.add_argument("--frames-per-tile", type=int, default=32)
    ap.add_argument("--snrs", type=float, nargs="*", default=None)
    ap.add_argument("--precision", choices=["fp32", "fp64"], default="fp32")
    ap.add_argument("--estimator", choices=["omp", "mmse", "mmse-ls"], default="omp",
                    help="mmse: MMSE_CE with the true channel (one point per call); mmse-ls: MMSE_CE with h = ifft(H_LS) per frame")
    ap.add_argument("--backend", default="nccl", help="nccl = RCCL over xGMI; gloo for rehearsals")
    ap.add_argument("--force-device", type=int, default=None, help="rehearsal only: every rank on this GPU")
    ap.add_argument("--fused", action="store_true", help="reference order (Noise -> conv) through RxPlan.ber_sweep")
    ap.add_argument("--mer", action="store_true", help="per-point MER_dB (MER_func sums of the receiver)")
    ap.add_argument("--fading", choices=["EPA", "EVA", "ETU"], default=None,
                    help="with --fused at C5 / M: a channel realisation of this delay profile per frame")
    ap.add_argument("--nmse", action="store_true", help="with --fading: per-point NMSE of the channel estimate")
    ap.add_argument("--random-pilots", type=int, default=None, metavar="NP",
                    help="with --fused at M: a sorted random mask of NP pilot carriers in 1..N_carrier (Task5_part2.m:58-64)")
    ap.add_argument("--mask-seed", type=int, default=1, help="seed of the random pilot mask")
    ap.add_argument("--dictionary", choices=["comb", "full"], default="comb",
                    help="full: K = Nfft, all delays (Task5_part2.m:181-184); the plan's OMP route is then 'auto'")
    ap.add_argument("--density", type=int, default=None, metavar="BINS",
                    help="with --fused at C5 / M: per point a BINS x BINS density of the equalised points (8, 16, 32, 64 or 128)")
    ap.add_argument("--half-width", type=float, default=None, metavar="L", help="with --density: the grid spans [-L, L)^2 (default 1.5 max|dict|)")
    ap.add_argument("--json", default=None)
    return ap


def parse_args(argv=None):
    """The command line; a --fading / --nmse combination the sweep cannot run is a usage error."""
    ap = parser()
    a = ap.parse_args(argv)
    bad = check_fading(a.config, a.estimator, a.fused, a.fading, a.nmse) or \
        check_pilots(a.config, a.estimator, a.fused, a.random_pilots, a.dictionary) or \
        check_density(a.config, a.fused, a.density, a.half_width)
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
    res = run(a.config, a.snrs, a.batches, a.frames_per_tile, a.precision, estimator=a.estimator, rank=rank, world=world,
              device_index=dev_index, backend=a.backend, fused=a.fused, mer=a.mer, fading=a.fading, nmse=a.nmse,
              random_pilots=a.random_pilots, mask_seed=a.mask_seed, dictionary=a.dictionary, density=a.density,
              half_width=a.half_width)
    if rank == 0:
        text = json.dumps(res)
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
