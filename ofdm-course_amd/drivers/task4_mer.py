"""Replay of the MER(SNR) study of `Task 4/Main_model_Task_4.m:136-200` ("the effect of noise on fine timing sync") on the
Task-4 geometry of drivers/task4.py (Nfft 1024, 400 carriers, 15 % pilots, 16QAM, 10 frames x 5 symbols = N_symb 50).

Per SNR point (T4:144-163): Noise(SNR) -> add_STO(Time_Delay = 12) -> AutoCorrFunction -> add_STO(TgPosition) ->
add_STO(-(Nfft+T_Guard)) -> OFDM_demodulator -> fine_sync(., 1, freq_desync = 0) -> get_payload -> MER_func(RX_IQ(Nfft+T_Guard+1:end)),
and the script plots abs(MERs - SNRs) (T4:196-199).  Every point is one ofdm_ber_sweep_task4_ex call (RxPlan.ber_sweep_task4 with
want_mer): the fused generator (Noise -> add_STO) and the batched Task-4 receiver with time_desync = 1, freq_desync = 0 (the
committed flag of T4:85, the second flag of fine_sync in the study), mp_desync = 0.  The script draws one realisation per
point; here a point is the MER of `frames_per_point` realisations concatenated (frames of N_symb symbols, Philox payload and
noise keyed by `seed`).

`--density BINS [--half-width L]` (run(density=BINS, half_width=L)) adds what the script shows beside the curve, one scatter per
SNR point (T4:165, the frames of its GIF): per point the constellation density of RX_IQ(Nfft+T_Guard+1:end) -- the span of
its MER -- over all realisations, a BINS x BINS grid on [-L, L)^2 (ofdm_ber_sweep_task4_scope), and the scatter
RX_IQ(length(dataCarriers)+1 : 2*length(dataCarriers)) of the point's first frame (tx_frames_fused + rx_chain_task4 with
iq_window).  L defaults to 1.5 max|dict|.  Without the option the output is unchanged.
"""
from __future__ import annotations

import numpy as np

from . import common as c


def run(lib=None, SNRs=None, frames_per_point=8, seed=1, Nfft=1024, N_carrier=400, Amount_OFDM_Frames=10,
        Amount_ODFM_SpF=5, Percent_pilot=15, Constellation="16QAM", Time_Delay=12, precision="fp64", device=None,
        density=None, half_width=None):
    """T4/Main_model_Task_4.m:136-200.  SNRs default to the script's 0:1:40.  Returns SNRs, MER_dB and
    MER_minus_SNR = abs(MER_dB - SNRs); with density=BINS also density [n, BINS, BINS] (rows: im, columns: re),
    density_dropped [n], density_points (the points counted per SNR), half_width and scatter [n, nd] (T4:165)."""
    lib = lib or c.default_lib()
    SNRs = np.arange(0.0, 41.0, 1.0) if SNRs is None else np.asarray(SNRs, dtype=np.float64).ravel()
    T_Guard = Nfft // 8
    N_symb = Amount_OFDM_Frames * Amount_ODFM_SpF
    _, pilotCarriers, dataCarriers = c.layout_percent(Nfft, N_carrier, Percent_pilot, tail=2)   # T4:14-21
    dict_, _ = lib.constellation_func(Constellation)
    col = c.alternating_pilots(4 / 3 * np.max(np.abs(dict_)), len(pilotCarriers), 1)[:, 0]      # T4:26-31
    plan = lib.RxPlan(Nfft, T_Guard, N_symb, N_carrier, pilotCarriers, dataCarriers, col, len(pilotCarriers), 3,
                      Constellation, precision=precision, device=device)
    kw, scatter = {}, None
    nd = len(dataCarriers)
    if density is not None:
        half_width = 1.5 * float(np.max(np.abs(dict_))) if half_width is None else float(half_width)
        kw["density"] = dict(bins=int(density), half_width=half_width, skip=Nfft + T_Guard)     # the span of the MER (T4:163)
    try:
        out = plan.ber_sweep_task4(SNRs, int(frames_per_point), Time_Delay=int(Time_Delay), time_desync=1, freq_desync=0,
                                   mp_desync=0, seed=int(seed), want_mer=True, mer_skip=Nfft + T_Guard, **kw)
        if density is not None and int(frames_per_point) > 0:
            rows = []
            for snr in SNRs:                                                                    # the point's first frame
                gen = plan.tx_frames_fused(1, SNR=float(snr), seed=int(seed), frame0=0, Time_Delay=int(Time_Delay),
                                           device=device)
                rx = gen["rx"] if device is None else gen["rx"].contiguous()
                one = lib.rx_chain_task4(plan, rx, 1, 0, 0, iq_window=(nd, nd))                 # T4:165
                iq = one["RX_IQ"]
                rows.append(np.asarray(iq.cpu() if hasattr(iq, "cpu") else iq)[0])
            scatter = np.stack(rows) if rows else np.zeros((0, nd), dtype=np.complex128)
    finally:
        plan.close()
    mer = np.asarray(out["MER_dB"].cpu() if hasattr(out["MER_dB"], "cpu") else out["MER_dB"], dtype=np.float64)
    host = lambda v: np.asarray(v.cpu() if hasattr(v, "cpu") else v)
    res = {"driver": "Task 4/Main_model_Task_4.m:136-200", "SNRs": SNRs, "MER_dB": mer,
           "MER_minus_SNR": np.abs(mer - SNRs), "frames_per_point": int(frames_per_point), "Time_Delay": int(Time_Delay),
           "mer_sums": host(out["mer_sums"]), "errors": host(out["errors"]), "bits": int(out["bits"]),
           "status_counts": host(out["status_counts"])}
    if density is not None:
        res.update(density=host(out["density"]), density_dropped=host(out["density_dropped"]),
                   density_points=int(frames_per_point) * (nd * N_symb - (Nfft + T_Guard)), half_width=half_width,
                   density_bins=int(density))
        if scatter is not None:
            res["scatter"] = scatter
    return res


def _main():
    """The common command line plus `--density BINS [--half-width L]`."""
    import argparse
    import sys
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--density", type=int, default=None)
    ap.add_argument("--half-width", type=float, default=None)
    a, rest = ap.parse_known_args()
    if a.half_width is not None and a.density is None:
        raise SystemExit("--half-width needs --density")
    sys.argv = [sys.argv[0], *rest]
    if a.density is not None:
        sys.argv.append(f"density={a.density}")
        if a.half_width is not None:
            sys.argv.append(f"half_width={a.half_width!r}")
    c.cli(run, __doc__)


if __name__ == "__main__":
    _main()
