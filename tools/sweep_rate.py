"""BER(SNR) sweep rate: the frame generators against each other and the end-to-end sweep tile, one JSON line.

Per config (fp32, the benchmark tiles): generation ms of tx_frames(noise_first=True) (the staged ofdm_tx_frames_ex) and of
tx_frames_fused on the same frames, the RX ms of rx_chain_task5 on that tile, and one-point ber_sweep calls of the same
size (generation + RX + reduction) as sym/s.  The roofline of the fused generator counts its bytes as 3 sample passes (TX
write, TX read, RX write) + the packed reference bits, against 8 TB/s.

C3 (the Task-4 receiver, 4096 frames of 50 symbols, random STO / CFO per frame, 30 dB): the staged
tx_frames(noise_first=True, Time_Delay="random", Freq_Shift="random") against tx_frames_fused with the same draws (and
without the CFO stage, the cost of the per-sample double sincos), rx_chain_task4 on the tile, and a one-point
ber_sweep_task4 call of the same size.  With --mer the C3 entry adds the same sweep with the MER sums on
(ber_sweep_task4(want_mer=True, mer_skip=Nfft+T_guard), ofdm_ber_sweep_task4_ex) and rx_chain_task4 with want_mer, each timed
in alternation with its MER-off form (rounds of `reps` calls each) so that the two medians see the same clocks.

--fading (M, C5): the cost of a channel per frame.  The generator with the config's static channel (tx_frames_fused(h=...),
the yardstick) against the generator drawing a channel per frame on the same delays with the taps' powers
(tx_frames_fused(fading=...), ofdm_tx_frames_fading), three rounds of `reps` calls each in alternation, every round's median
and the spread (max - min) of each side; then the one-point fading sweep without and with the NMSE outputs in the same
alternation (their difference is t5_frame_nmse_kernel + the stored estimates) beside the RX time of the tile.

--fading C3: the Task-4 tile over channel realisations with the NMSE outputs (ber_sweep_task4(fading=, want_nmse=True),
ofdm_ber_sweep_task4_fading) against the static-channel tile (ber_sweep_task4(h=), the parent's code) on the same delays, both
with random STO / CFO, 4096 frames, one point, in the same alternation; and the static tile with the NMSE outputs on
(ofdm_ber_sweep_task4_nmse).

    python tools/sweep_rate.py [--mer] [--fading] [M C4 C5 C3]
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ofdm_course_amd as ofdm  # noqa: E402
from ofdm_course_amd import frames as fr  # noqa: E402

PEAK_TBS = 8.0


def timed(fn, reps=5, warm=1):
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
    return float(np.median(ms))


def config(name):
    if name == "M":
        return fr.config_M(), 20480, False
    if name == "C4":
        return fr.FrameConfig("C4", 4096, 1024, 4, "64QAM"), 8192, True
    return fr.config_C5(), 3072, False


def measure(name, reps=5):
    cfg, F, mmse = config(name)
    dev = torch.device("cuda:0")
    plan = fr.make_plan(cfg, ofdm, precision="fp32", device=0)
    h, _ = ofdm.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    if mmse:
        hh = np.zeros(cfg.N_carrier, dtype=np.complex64)
        hh[: len(h)] = h
        plan.set_mmse(hh, cfg.SNR_dB)
    snr = cfg.SNR_dB
    ms_ex = timed(lambda: plan.tx_frames(F, h=h, SNR=snr, seed=3, device=dev, noise_first=True), reps)
    torch.cuda.empty_cache()
    ms_fused = timed(lambda: plan.tx_frames_fused(F, h=h, SNR=snr, seed=3, device=dev), reps)
    gen = plan.tx_frames_fused(F, h=h, SNR=snr, seed=3, device=dev)
    ms_rx = timed(lambda: ofdm.rx_chain_task5(plan, gen["rx"], ref_bits_packed=gen["packed"]), reps)
    ber_rx = float(ofdm.rx_chain_task5(plan, gen["rx"], ref_bits_packed=gen["packed"])["errors"].to(torch.int64).sum().item())
    del gen
    torch.cuda.empty_cache()
    ms_sweep = timed(lambda: plan.ber_sweep([snr], F, h=h, seed=3, device=dev), reps)
    res = plan.ber_sweep([snr], F, h=h, seed=3, device=dev)
    err = int(res["errors"][0].item())
    sample_bytes = 8 * cfg.frame_samples * F
    counted = 3 * sample_bytes + plan.frame_bytes * F
    plan.close()
    torch.cuda.empty_cache()
    nsym = F * cfg.N_symb
    return {"config": name, "frames": F, "estimator": "mmse" if mmse else "omp", "snr_db": snr,
            "gen_ex_ms": ms_ex, "gen_fused_ms": ms_fused, "gen_speedup": ms_ex / ms_fused, "rx_ms": ms_rx,
            "sweep_ms": ms_sweep, "sweep_sym_per_s": nsym / ms_sweep * 1e3, "rx_sym_per_s": nsym / ms_rx * 1e3,
            "ber": err / (F * plan.frame_bits), "sweep_errors_equal_composed": err == int(ber_rx),
            "roofline": {"sample_pass_bytes": sample_bytes, "counted_bytes": counted,
                         "gen_fused_tbs": counted / (ms_fused * 1e-3) / 1e12,
                         "gen_fused_frac": counted / (ms_fused * 1e-3) / 1e12 / PEAK_TBS,
                         "floor_ms": counted / (PEAK_TBS * 1e12) * 1e3}}


def ab_timed(fa, fb, reps=5, rounds=3):
    """medians of fa and fb timed in alternating rounds (a drift of the clocks hits both)"""
    a, b = [], []
    for _ in range(rounds):
        a.append(timed(fa, reps))
        b.append(timed(fb, reps))
    return float(np.median(a)), float(np.median(b))


def ab_rounds(fa, fb, reps=5, rounds=3):
    """every round's median of fa and fb, timed in alternating rounds"""
    a, b = [], []
    for _ in range(rounds):
        a.append(timed(fa, reps))
        b.append(timed(fb, reps))
    return a, b


def measure_fading(name, reps=5):
    cfg, F, _ = config(name)
    dev = torch.device("cuda:0")
    plan = fr.make_plan(cfg, ofdm, precision="fp32", device=0)
    h, _ = ofdm.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    snr = cfg.SNR_dB
    nz = np.flatnonzero(h)                                   # the same delay line for both: equal tap count and halo
    fad = (nz, np.abs(h[nz]) ** 2)
    st, fa = ab_rounds(lambda: plan.tx_frames_fused(F, h=h, SNR=snr, seed=3, device=dev),
                       lambda: plan.tx_frames_fused(F, fading=fad, SNR=snr, seed=3, device=dev), reps)
    torch.cuda.empty_cache()
    gen = plan.tx_frames_fused(F, fading=fad, SNR=snr, seed=3, device=dev)
    ms_rx = timed(lambda: ofdm.rx_chain_task5(plan, gen["rx"], ref_bits_packed=gen["packed"]), reps)
    del gen
    torch.cuda.empty_cache()
    off, on = ab_rounds(lambda: plan.ber_sweep([snr], F, fading=fad, seed=3, device=dev),
                        lambda: plan.ber_sweep([snr], F, fading=fad, seed=3, device=dev, want_nmse=True), reps)
    res = plan.ber_sweep([snr], F, fading=fad, seed=3, device=dev, want_nmse=True)
    r = {"config": name, "mode": "fading", "frames": F, "snr_db": snr, "n_taps": int(nz.size), "halo": int(nz[-1]),
         "gen_static_ms": st, "gen_fading_ms": fa, "gen_static_spread_ms": max(st) - min(st),
         "gen_fading_spread_ms": max(fa) - min(fa), "gen_fading_over_static": float(np.median(fa) / np.median(st)),
         "rx_ms": ms_rx, "sweep_fading_ms": off, "sweep_fading_nmse_ms": on,
         "nmse_ms_per_tile": float(np.median(on) - np.median(off)),
         "ber": int(res["errors"][0].item()) / (F * plan.frame_bits), "NMSE": float(res["NMSE"][0].item())}
    plan.close()
    torch.cuda.empty_cache()
    return r


def measure_c3_fading(reps=5):
    cfg, F = fr.config_C3(), 4096
    dev = torch.device("cuda:0")
    plan = fr.make_plan(cfg, ofdm, precision="fp32", device=0)
    h, _ = ofdm.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    snr = cfg.SNR_dB
    imp = dict(Time_Delay="random", Freq_Shift="random")
    nz = np.flatnonzero(h)                                   # the same delay line for both: equal tap count and halo
    fad = (nz, np.abs(h[nz]) ** 2)
    static = lambda **kw: plan.ber_sweep_task4([snr], F, h=h, seed=3, device=dev, **imp, **kw)
    fading = lambda **kw: plan.ber_sweep_task4([snr], F, fading=fad, seed=3, device=dev, **imp, **kw)
    st, fn = ab_rounds(static, lambda: fading(want_nmse=True), reps)
    st2, sn = ab_rounds(static, lambda: static(want_nmse=True), reps)
    rs, rf = static(want_nmse=True), fading(want_nmse=True)
    r = {"config": "C3", "mode": "fading", "frames": F, "snr_db": snr, "impairments": "random STO / CFO",
         "n_taps": int(nz.size), "halo": int(nz[-1]), "sweep_static_ms": st, "sweep_fading_nmse_ms": fn,
         "fading_nmse_over_static": float(np.median(fn) / np.median(st)), "sweep_static_again_ms": st2,
         "sweep_static_nmse_ms": sn, "static_nmse_over_static": float(np.median(sn) / np.median(st2)),
         "static": {"ber": int(rs["errors"][0].item()) / (F * plan.frame_bits), "NMSE": float(rs["NMSE"][0].item()),
                    "status_counts": rs["status_counts"][0].cpu().tolist()},
         "fading": {"ber": int(rf["errors"][0].item()) / (F * plan.frame_bits), "NMSE": float(rf["NMSE"][0].item()),
                    "status_counts": rf["status_counts"][0].cpu().tolist()}}
    plan.close()
    torch.cuda.empty_cache()
    return r


def measure_c3(reps=5, mer=False):
    cfg, F = fr.config_C3(), 4096
    dev = torch.device("cuda:0")
    plan = fr.make_plan(cfg, ofdm, precision="fp32", device=0)
    h, _ = ofdm.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    snr = cfg.SNR_dB
    imp = dict(Time_Delay="random", Freq_Shift="random")
    ms_ex = timed(lambda: plan.tx_frames(F, h=h, SNR=snr, seed=3, device=dev, noise_first=True, **imp), reps)
    ex = plan.tx_frames(F, h=h, SNR=snr, seed=3, device=dev, noise_first=True, want_draws=True, **imp)
    draws = (ex["Time_Delay"].clone(), ex["Freq_Shift"].clone())
    del ex
    torch.cuda.empty_cache()
    ms_fused = timed(lambda: plan.tx_frames_fused(F, h=h, SNR=snr, seed=3, device=dev, **imp), reps)
    ms_no_cfo = timed(lambda: plan.tx_frames_fused(F, h=h, SNR=snr, seed=3, device=dev, Time_Delay="random"), reps)
    gen = plan.tx_frames_fused(F, h=h, SNR=snr, seed=3, device=dev, want_draws=True, **imp)
    same_draws = bool(torch.equal(gen["Time_Delay"], draws[0]) and torch.equal(gen["Freq_Shift"], draws[1]))
    ms_rx = timed(lambda: ofdm.rx_chain_task4(plan, gen["rx"], 1, 1, 1, ref_bits_packed=gen["packed"]), reps)
    out = ofdm.rx_chain_task4(plan, gen["rx"], 1, 1, 1, ref_bits_packed=gen["packed"])
    err_rx = int(out["errors"].to(torch.int64).sum().item())
    del gen, out
    torch.cuda.empty_cache()
    ms_sweep = timed(lambda: plan.ber_sweep_task4([snr], F, h=h, seed=3, device=dev, **imp), reps)
    res = plan.ber_sweep_task4([snr], F, h=h, seed=3, device=dev, **imp)
    err = int(res["errors"][0].item())
    sample_bytes = 8 * cfg.frame_samples * F
    counted = 3 * sample_bytes + plan.frame_bytes * F
    nsym = F * cfg.N_symb
    r = {"config": "C3", "frames": F, "estimator": "task4", "snr_db": snr, "impairments": "random STO / CFO",
         "gen_ex_ms": ms_ex, "gen_fused_ms": ms_fused, "gen_speedup": ms_ex / ms_fused, "gen_fused_no_cfo_ms": ms_no_cfo,
         "draws_equal_ex": same_draws, "rx_ms": ms_rx, "sweep_ms": ms_sweep, "sweep_sym_per_s": nsym / ms_sweep * 1e3,
         "rx_sym_per_s": nsym / ms_rx * 1e3, "ber": err / (F * plan.frame_bits),
         "status_counts": res["status_counts"][0].cpu().tolist(),
         "cfo_abs_err_mean": float(res["cfo_abs_err"][0].item()) / F, "sweep_errors_equal_composed": err == err_rx,
         "roofline": {"sample_pass_bytes": sample_bytes, "counted_bytes": counted,
                      "gen_fused_tbs": counted / (ms_fused * 1e-3) / 1e12,
                      "gen_fused_frac": counted / (ms_fused * 1e-3) / 1e12 / PEAK_TBS,
                      "floor_ms": counted / (PEAK_TBS * 1e12) * 1e3}}
    if mer:
        skip = cfg.Nfft + cfg.T_guard
        off, on = ab_timed(lambda: plan.ber_sweep_task4([snr], F, h=h, seed=3, device=dev, **imp),
                           lambda: plan.ber_sweep_task4([snr], F, h=h, seed=3, device=dev, want_mer=True, mer_skip=skip, **imp),
                           reps)
        rm = plan.ber_sweep_task4([snr], F, h=h, seed=3, device=dev, want_mer=True, mer_skip=skip, **imp)
        gen = plan.tx_frames_fused(F, h=h, SNR=snr, seed=3, device=dev, **imp)
        rx_off, rx_on = ab_timed(lambda: ofdm.rx_chain_task4(plan, gen["rx"], 1, 1, 1, ref_bits_packed=gen["packed"]),
                                 lambda: ofdm.rx_chain_task4(plan, gen["rx"], 1, 1, 1, ref_bits_packed=gen["packed"],
                                                             want_mer=True, mer_skip=skip), reps)
        del gen
        torch.cuda.empty_cache()
        r["mer"] = {"mer_skip": skip, "sweep_off_ms": off, "sweep_on_ms": on, "sweep_on_over_off": on / off,
                    "sweep_on_sym_per_s": nsym / on * 1e3, "rx_off_ms": rx_off, "rx_on_ms": rx_on,
                    "rx_on_over_off": rx_on / rx_off, "MER_dB": float(rm["MER_dB"][0].item()),
                    "errors_equal_off": int(rm["errors"][0].item()) == err}
    plan.close()
    torch.cuda.empty_cache()
    return r


def main():
    args = sys.argv[1:]
    mer = "--mer" in args
    fading = "--fading" in args
    names = [a for a in args if a not in ("--mer", "--fading")] or (["M", "C5"] if fading else ["M", "C4", "C5"])
    ofdm.init(0)
    if fading:
        configs = [measure_c3_fading() if n == "C3" else measure_fading(n) for n in names]
    else:
        configs = [measure_c3(mer=mer) if n == "C3" else measure(n) for n in names]
    out = {"tool": "sweep_rate", "dtype": "f32", "configs": configs}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
