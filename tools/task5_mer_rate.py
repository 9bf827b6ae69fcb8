"""MER off / on times (ms per call, medians of four alternating rounds) of rx_chain_task5 and RxPlan.ber_sweep at M, C4
(Nfft 4096, MMSE mode, one point) and C5; one JSON line per config.  usage: python tools/task5_mer_rate.py [out.json]"""
import json, sys, time
import numpy as np
import torch
import ofdm_course_amd as ofdm
from ofdm_course_amd import frames as fr

ofdm.init(0)
dev = torch.device("cuda", 0)
res = {}
def timed(fn, reps):
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize(); return (time.perf_counter() - t) / reps * 1e3
for name, nfr, fpp in (("M", 8192, 2048), ("C4", 4096, 1024), ("C5", 1024, 256)):
    if name == "C4":                                  # Nfft 4096, MMSE_CE (tools/bench_configs.py c4)
        cfg = fr.FrameConfig("C4", 4096, 1024, 4, "64QAM")
    else:
        cfg = fr.config_M() if name == "M" else fr.config_C5()
    plan = fr.make_plan(cfg, ofdm, precision="fp32", device=0)
    pts = [10.0, 20.0]
    if name == "C4":
        hh = np.zeros(cfg.N_carrier, dtype=np.complex128)
        h0, _ = ofdm.get_MP_channel_resp(cfg.taps, cfg.Nfft)
        hh[: len(h0)] = h0
        plan.set_mmse(hh, cfg.SNR_dB)
        pts = [20.0]
    data = fr.make_frames_device(cfg, ofdm, plan, nfr, seed=3, device=dev)
    rx = data["rx"]
    h, _ = ofdm.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    f_off = lambda: ofdm.rx_chain_task5(plan, rx)
    f_on = lambda: ofdm.rx_chain_task5(plan, rx, want_mer=True)
    s_off = lambda: plan.ber_sweep(pts, fpp, h=h, device=dev)
    s_on = lambda: plan.ber_sweep(pts, fpp, h=h, device=dev, want_mer=True)
    for f in (f_off, f_on, s_off, s_on):
        f()
    r = {"rx_off": [], "rx_on": [], "sweep_off": [], "sweep_on": []}
    for _ in range(4):
        r["rx_off"].append(timed(f_off, 10)); r["rx_on"].append(timed(f_on, 10))
        r["sweep_off"].append(timed(s_off, 2)); r["sweep_on"].append(timed(s_on, 2))
    med = {k: float(np.median(v)) for k, v in r.items()}
    med["rx_cost_pct"] = 100 * (med["rx_on"] / med["rx_off"] - 1)
    med["sweep_cost_pct"] = 100 * (med["sweep_on"] / med["sweep_off"] - 1)
    med["frames"], med["frames_per_point"] = nfr, fpp
    res[name] = med
    plan.close()
    print(name, json.dumps(med), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(res, f)
