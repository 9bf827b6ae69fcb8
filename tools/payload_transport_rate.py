"""Payload transport rate at config M (fp32, one point): RxPlan.transport on the test card repeated to a few thousand frames against
the same work done with the entries the parent commit has -- tx_frames_fused (Philox payload, the same frame count and channel)
followed by rx_chain_task5 with the reference bits -- one JSON line.

The two sides are timed in alternation, three rounds of `reps` calls each, every round's median and the spread (max - min) of each
side: the difference between them means something only where it exceeds both spreads.  The composition does not join the frames
nor count per stream bit; transport does (payload_frames_kernel in place of tx_bits_kernel, payload_join_kernel,
payload_tally_kernel with the ones columns), so the figure is the cost of the way in and the way out on top of generator + receiver.

    python tools/payload_transport_rate.py [--repeats 600] [--reps 5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ofdm_course_amd as ofdm  # noqa: E402
from ofdm_course_amd import frames as fr  # noqa: E402
from ofdm_course_amd.drivers import send_picture as sp  # noqa: E402


def timed(fn, reps):
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=600, help="the card is 5 frames of config M (32256 bits each): 600 repeats "
                                                             "are 3000 frames; see `frames` in the output")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    cfg = fr.config_M()
    dev = torch.device("cuda:0")
    plan = fr.make_plan(cfg, ofdm, precision="fp32", device=0)
    h, _ = ofdm.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    bits = torch.from_numpy(sp.image_bits(sp.test_card())).to(dev)
    F = -(-bits.numel() // plan.frame_bits)
    n_frames = F * a.repeats
    snr = cfg.SNR_dB

    def transport(**kw):
        return plan.transport(bits, [snr], repeats=a.repeats, h=h, seed=3, device=dev, **kw)

    def composed():
        gen = plan.tx_frames_fused(n_frames, h=h, SNR=snr, seed=3, device=dev)
        return ofdm.rx_chain_task5(plan, gen["rx"], ref_bits_packed=gen["packed"])

    sides = {"transport": lambda: transport(want_ones=True, want_frames=True), "transport_errors_only": lambda: transport(want_decoded=False),
             "composed": composed}
    for fn in sides.values():                                        # warm-up: workspaces, first-call growth
        fn()
    rounds = {k: [] for k in sides}
    for _ in range(3):
        for k, fn in sides.items():
            rounds[k].append(timed(fn, a.reps))
    out = transport()
    torch.cuda.synchronize()
    res = {"config": "M", "dtype": "f32", "n_bits": int(bits.numel()), "frame_bits": int(plan.frame_bits), "frames_per_repeat": int(F),
           "repeats": a.repeats, "frames": int(n_frames), "SNR_dB": snr, "BER": float(out["BER"].mean().item()), "reps": a.reps}
    for k, ms in rounds.items():
        med = float(np.median(ms))
        res[k] = {"ms_rounds": ms, "ms": med, "spread_ms": max(ms) - min(ms), "frames_per_s": n_frames / (med * 1e-3),
                  "symbols_per_s": n_frames * cfg.N_symb / (med * 1e-3)}
    res["transport_over_composed"] = res["transport"]["ms"] / res["composed"]["ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
