"""Replay of the NMSE(SNR) study of `Task 4/Main_model_Task_4.m:205-239` ("the effect of noise on the channel estimate", graph
`Task 4/graphs/nmse(snr).png`) on the Task-4 geometry of drivers/task4.py (Nfft 1024, 400 carriers, 16QAM, 10 frames x 5
symbols = N_symb 50).

Per SNR point (T4:209-236): Noise(SNR) -> conv with the taps 0 / 4 / 10 (amplitudes 1 / 0.6 / 0.3), truncated ->
OFDM_demodulator -> estimate_channel -> MSEs(i) = (H_freq - H_est)(H_freq - H_est)' / N_carrier over carriers 1..N_carrier.
Every point is part of one ofdm_ber_sweep_task4_nmse call (RxPlan.ber_sweep_task4 with want_nmse): the fused generator
(Noise -> conv) and the batched Task-4 receiver with the flags (time_desync, freq_desync, mp_desync) = (0, 0, 1).  The script
draws one realisation per point; here a point is the mean over `frames_per_point` realisations (frames of N_symb symbols,
Philox payload and noise keyed by `seed`).  Percent_pilot = 15 is the committed value (T4:14); 25 gives pilot_step 4, the
setting of the published graph.

fading="EPA" | "EVA" | "ETU" replaces the fixed taps by a channel drawn per frame on that 3GPP delay line
(ofdm_ber_sweep_task4_fading, drivers.common.fading_profile at the sampling rate of drivers/sweep_ber.py), the error then
taken against each frame's own channel.  sync=True adds Time_Delay = Freq_Shift = "random" (T4:101-110) with time_desync and
freq_desync on: the whole synchroniser in front of the estimator -- the NMSE then contains the delay / phase ramp fine_sync
removes.
"""
from __future__ import annotations

import numpy as np

from . import common as c

TAPS = np.array([[0, 1.0], [4, 0.6], [10, 0.3]])                                  # T4:213-217


def run(lib=None, SNRs=None, frames_per_point=8, seed=1, Nfft=1024, N_carrier=400, Amount_OFDM_Frames=10,
        Amount_ODFM_SpF=5, Percent_pilot=15, Constellation="16QAM", fading=None, sync=False, precision="fp64", device=None):
    """T4/Main_model_Task_4.m:205-239.  SNRs default to the script's 0:0.5:30.  Returns SNRs, NMSE, nmse_sums, errors, bits,
    BER and status_counts."""
    lib = lib or c.default_lib()
    SNRs = np.arange(0.0, 30.5, 0.5) if SNRs is None else np.asarray(SNRs, dtype=np.float64).ravel()
    T_Guard = Nfft // 8
    N_symb = Amount_OFDM_Frames * Amount_ODFM_SpF
    _, pilotCarriers, dataCarriers = c.layout_percent(Nfft, N_carrier, Percent_pilot, tail=2)   # T4:14-21
    dict_, _ = lib.constellation_func(Constellation)
    col = c.alternating_pilots(4 / 3 * np.max(np.abs(dict_)), len(pilotCarriers), 1)[:, 0]      # T4:26-31
    kw = {}
    if fading is not None:
        from .sweep_ber import FADING_SAMPLING_RATE
        delays, powers = c.fading_profile(str(fading), FADING_SAMPLING_RATE)
        kw["fading"] = (delays, powers)
    else:
        kw["h"], _ = lib.get_MP_channel_resp(TAPS, Nfft)                                        # T4:221
    if sync:
        kw.update(Time_Delay="random", Freq_Shift="random")
    plan = lib.RxPlan(Nfft, T_Guard, N_symb, N_carrier, pilotCarriers, dataCarriers, col, len(pilotCarriers), 3,
                      Constellation, precision=precision, device=device)
    try:
        out = plan.ber_sweep_task4(SNRs, int(frames_per_point), time_desync=int(bool(sync)), freq_desync=int(bool(sync)),
                                   mp_desync=1, seed=int(seed), want_nmse=True, **kw)
    finally:
        plan.close()
    errors = np.asarray(out["errors"])
    res = {"driver": "Task 4/Main_model_Task_4.m:205-239", "SNRs": SNRs, "NMSE": np.asarray(out["NMSE"], dtype=np.float64),
           "nmse_sums": np.asarray(out["nmse_sums"]), "errors": errors, "bits": int(out["bits"]),
           "BER": errors / max(int(out["bits"]), 1), "status_counts": np.asarray(out["status_counts"]),
           "frames_per_point": int(frames_per_point), "Percent_pilot": Percent_pilot, "sync": bool(sync)}
    if fading is not None:
        res["fading"] = {"profile": str(fading), "sampling_rate": FADING_SAMPLING_RATE, "delays": delays.tolist(),
                         "powers": powers.tolist()}
    return res


if __name__ == "__main__":
    c.cli(run, __doc__)
