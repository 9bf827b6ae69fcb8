"""Profiling target of the fused generator and the BER(SNR) sweep tile (for rocprofv3 --kernel-trace --stats and the
FETCH_SIZE / WRITE_SIZE passes, profiles/sweep/): per config one tx_frames_fused call and one two-point ber_sweep call of
the benchmark tile, fp32, nothing else on the GPU but the plan set-up.  C3: tx_frames_fused with random STO / CFO and a
two-point ber_sweep_task4 call (the Task-4 receiver, all desync stages on).

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/sweep_profile.py M C5
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/sweep_profile.py C3
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ofdm_course_amd as ofdm  # noqa: E402
from ofdm_course_amd import frames as fr  # noqa: E402

TILES = {"M": (fr.config_M, 20480), "C5": (fr.config_C5, 3072), "C3": (fr.config_C3, 4096)}
IMP = dict(Time_Delay="random", Freq_Shift="random")

ofdm.init(0)
dev = torch.device("cuda:0")
for name in sys.argv[1:] or ["M", "C5"]:
    make, F = TILES[name]
    cfg = make()
    plan = fr.make_plan(cfg, ofdm, precision="fp32", device=0)
    h, _ = ofdm.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    t4 = name == "C3"
    gen = plan.tx_frames_fused(F, h=h, SNR=cfg.SNR_dB, seed=3, device=dev, **(IMP if t4 else {}))
    del gen
    torch.cuda.empty_cache()
    if t4:
        res = plan.ber_sweep_task4(np.array([20.0, 30.0]), F // 2, h=h, seed=3, device=dev, **IMP)
    else:
        res = plan.ber_sweep(np.array([10.0, 20.0]), F // 2, h=h, seed=3, device=dev)
    torch.cuda.synchronize()
    print(name, F, "frames; errors per point", res["errors"].cpu().tolist(), flush=True)
    plan.close()
    torch.cuda.empty_cache()
