"""Replay of the MER(SNR) study of `Task 4/Main_model_Task_4.m:136-200` ("the effect of noise on fine timing sync") on the
Task-4 geometry of drivers/task4.py (Nfft 1024, 400 carriers, 15 % pilots, 16QAM, 10 frames x 5 symbols = N_symb 50).

Per SNR point (T4:144-163): Noise(SNR) -> add_STO(Time_Delay = 12) -> AutoCorrFunction -> add_STO(TgPosition) ->
add_STO(-(Nfft+T_Guard)) -> OFDM_demodulator -> fine_sync(., 1, freq_desync = 0) -> get_payload -> MER_func(RX_IQ(Nfft+T_Guard+1:end)),
and the script plots abs(MERs - SNRs) (T4:196-199).  Every point is one ofdm_ber_sweep_task4_ex call (RxPlan.ber_sweep_task4 with
want_mer): the fused generator (Noise -> add_STO) and the batched Task-4 receiver with time_desync = 1, freq_desync = 0 (the
committed flag of T4:85, the second flag of fine_sync in the study), mp_desync = 0.  The script draws one realisation per
point; here a point is the MER of `frames_per_point` realisations concatenated (frames of N_symb symbols, Philox payload and
noise keyed by `seed`).
"""
from __future__ import annotations

import numpy as np

from . import common as c


def run(lib=None, SNRs=None, frames_per_point=8, seed=1, Nfft=1024, N_carrier=400, Amount_OFDM_Frames=10,
        Amount_ODFM_SpF=5, Percent_pilot=15, Constellation="16QAM", Time_Delay=12, precision="fp64", device=None):
    """T4/Main_model_Task_4.m:136-200.  SNRs default to the script's 0:1:40.  Returns SNRs, MER_dB and
    MER_minus_SNR = abs(MER_dB - SNRs)."""
    lib = lib or c.default_lib()
    SNRs = np.arange(0.0, 41.0, 1.0) if SNRs is None else np.asarray(SNRs, dtype=np.float64).ravel()
    T_Guard = Nfft // 8
    N_symb = Amount_OFDM_Frames * Amount_ODFM_SpF
    _, pilotCarriers, dataCarriers = c.layout_percent(Nfft, N_carrier, Percent_pilot, tail=2)   # T4:14-21
    dict_, _ = lib.constellation_func(Constellation)
    col = c.alternating_pilots(4 / 3 * np.max(np.abs(dict_)), len(pilotCarriers), 1)[:, 0]      # T4:26-31
    plan = lib.RxPlan(Nfft, T_Guard, N_symb, N_carrier, pilotCarriers, dataCarriers, col, len(pilotCarriers), 3,
                      Constellation, precision=precision, device=device)
    try:
        out = plan.ber_sweep_task4(SNRs, int(frames_per_point), Time_Delay=int(Time_Delay), time_desync=1, freq_desync=0,
                                   mp_desync=0, seed=int(seed), want_mer=True, mer_skip=Nfft + T_Guard)
    finally:
        plan.close()
    mer = np.asarray(out["MER_dB"], dtype=np.float64)
    return {"driver": "Task 4/Main_model_Task_4.m:136-200", "SNRs": SNRs, "MER_dB": mer,
            "MER_minus_SNR": np.abs(mer - SNRs), "frames_per_point": int(frames_per_point), "Time_Delay": int(Time_Delay),
            "mer_sums": np.asarray(out["mer_sums"]), "errors": np.asarray(out["errors"]), "bits": int(out["bits"]),
            "status_counts": np.asarray(out["status_counts"])}


if __name__ == "__main__":
    c.cli(run, __doc__)
