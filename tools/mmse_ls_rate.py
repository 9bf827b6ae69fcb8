"""Cost of the MMSE mode with h = ifft(H_LS) per frame (RxPlan.set_mmse_ls) at config M, one JSON line.

The one-point fused BER sweep of 20480 frames (tools/sweep_rate.py's tile) in OMP mode and in the new mode, timed in alternating
rounds so that both see the same clocks, and the three stage times of one rx_chain_task5 call per mode from
ofdm_rx_plan_set_timing (front end, estimator stage, symbol stage; OMP at M runs front end and pursuit as one launch).

    python tools/mmse_ls_rate.py [frames]
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
from sweep_rate import ab_rounds  # noqa: E402


def main():
    F = int(sys.argv[1]) if len(sys.argv) > 1 else 20480
    ofdm.init(0)
    cfg = fr.config_M()
    dev = torch.device("cuda:0")
    h, _ = ofdm.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    snr = cfg.SNR_dB
    # a plan per mode: no mode switch (a host synchronisation) inside a timed call
    plans = {"omp": fr.make_plan(cfg, ofdm, precision="fp32", device=0), "mmse-ls": fr.make_plan(cfg, ofdm, precision="fp32", device=0)}
    plans["mmse-ls"].set_mmse_ls(snr)
    plan = plans["omp"]

    def sweep(k):
        return plans[k].ber_sweep([snr], F, h=h, seed=3, device=dev)

    omp, ls = ab_rounds(lambda: sweep("omp"), lambda: sweep("mmse-ls"))
    ber = {k: int(sweep(k)["errors"][0].item()) / (F * plan.frame_bits) for k in plans}
    gen = plan.tx_frames_fused(F, h=h, SNR=snr, seed=3, device=dev)
    stages = {}
    for k, pk in plans.items():
        pk.set_timing(True)
        runs = []
        for _ in range(6):
            ofdm.rx_chain_task5(pk, gen["rx"], ref_bits_packed=gen["packed"])
            runs.append([float(x) for x in pk.last_kernel_ms()])
        stages[k] = np.median(np.asarray(runs[1:]), axis=0).tolist()
    for pk in plans.values():
        pk.close()
    nsym = F * cfg.N_symb
    print(json.dumps({"tool": "mmse_ls_rate", "config": "M", "frames": F, "snr_db": snr, "dtype": "f32",
                      "sweep_omp_ms": omp, "sweep_mmse_ls_ms": ls,
                      "sweep_omp_sym_per_s": nsym / float(np.median(omp)) * 1e3,
                      "sweep_mmse_ls_sym_per_s": nsym / float(np.median(ls)) * 1e3, "ber": ber,
                      "stage_ms_front_estimator_symbols": stages}), flush=True)


if __name__ == "__main__":
    main()
