"""The amplitude spectra ("АЧХ") of the `Task 3/README.md` report, replayed on the device over many frames.

The report shows, for every impairment of `Task 3/Main_model_Task_3.m:85-135`, the line of :138,
`abs(fft(Rx_OFDM_Signal(T_Guard+1 : Nfft+T_Guard)))`: the spectrum of the useful part of the first OFDM symbol.  Here every such
figure is one point of `RxPlan.spectrum_study` (ofdm_spectrum_study) on the T3 geometry -- Nfft 1024, 400 carriers, 15 % pilots at
4/3 max|dict|, 16QAM, frames of 5 symbols with the Scrambler register of T3:36 reset per frame (T3:6-59) --: `--frames` frames are
generated and transformed on one GPU and only the power per bin, summed over the frames, comes back.  `amp_rms` = sqrt(mean power)
is the report's curve averaged over the frames (over the payload, and over the noise where there is any); with `--frames 1` it is the
report's single line for the Philox payload.

SCENARIOS holds the settings with the figure numbers of `Task 3/README.md`.  The script switches its Noise stage off for every
figure but the AWGN one; the generator always runs Noise, so those scenarios run at CLEAN_SNR_DB = 3000 dB, the largest round
value whose linear form 10^(SNR/10) = 1e300 is still a finite double: the per-component sigma is about 1e-150 of the signal's RMS,
far below half an ulp of any sample, and the frames are the noise-free ones to rounding.  The generator's Noise stage is not
touched.  The remark of T3:155, that the null carriers take part of the AWGN power (the reason MER differs from SNR), is the
`null_power_share` of the AWGN figure against the clean one.

    python -m ofdm_course_amd.drivers.task3_spectrum --json out.json --frames 1000
"""
from __future__ import annotations

import argparse
import json

import numpy as np

from . import common as c

CLEAN_SNR_DB = 3000.0
CHANNEL_TAPS = np.array([[0, 1.0], [2, 0.4], [4, 0.01]])                          # T3/Main_model_Task_3.m:122-126

# (name, figure of Task 3/README.md, settings): SNR (T3:99), Time_Delay (:107), Freq_Shift (:115), multipath (:121-135)
SCENARIOS = (
    ("clean", 2, dict()),
    ("awgn_25dB", 4, dict(SNR=25.0)),
    ("sto_37", 9, dict(Time_Delay=37)),
    ("cfo_5", 12, dict(Freq_Shift=5.0)),
    ("cfo_0.01", 14, dict(Freq_Shift=0.01)),
    ("cfo_0.1", 16, dict(Freq_Shift=0.1)),
    ("cfo_100", 18, dict(Freq_Shift=100.0)),
    ("multipath", 24, dict(multipath=True)),
)


def check_args(frames, windows, n_symb=5):
    """What the replay needs of its arguments; the text of the refusal, or None."""
    if frames < 1:
        return "--frames must be >= 1"
    if not (1 <= windows <= n_symb):
        return f"--windows must be 1 .. {n_symb}"
    return None


def make_plan(lib, Nfft=1024, N_carrier=400, Percent_pilot=15, Constellation="16QAM", Amount_ODFM_SpF=5, precision="fp64",
              device_index=None):
    """The plan of one T3 frame (T3:6-24,:56-59): T_Guard = Nfft / 8, the percent pilot rule, every pilot at 4/3 max|dict|.  (The
    plan's estimator settings are not used by the study.)"""
    _, pilotCarriers, dataCarriers = c.layout_percent(Nfft, N_carrier, Percent_pilot, tail=2)
    dict_, _ = lib.constellation_func(Constellation)
    amp = 4 / 3 * np.max(np.abs(dict_))
    return lib.RxPlan(Nfft, Nfft // 8, Amount_ODFM_SpF, N_carrier, pilotCarriers, dataCarriers,
                      np.full(len(pilotCarriers), amp, dtype=np.complex128), min(8, Nfft), 1, Constellation,
                      precision=precision, device=device_index)


def study_args(settings, lib, Nfft):
    """The spectrum_study arguments of one scenario."""
    kw = dict(SNRs=[float(settings.get("SNR", CLEAN_SNR_DB))], Time_Delay=settings.get("Time_Delay"),
              Freq_Shift=settings.get("Freq_Shift"))
    if settings.get("multipath"):
        kw["h"], _ = lib.get_MP_channel_resp(CHANNEL_TAPS, Nfft)                  # T3:130
    return kw


def run(frames=100, windows=1, seed=1, precision="fp64", Nfft=1024, N_carrier=400, Percent_pilot=15, Constellation="16QAM",
        Amount_ODFM_SpF=5, device_index=0, max_frames_per_chunk=0):
    """Returns {"scenarios": {name: {figure, settings, SNR_dB, power_sums [Nfft], mean_power, amp_rms, peak,
    null_power_share}}, ...}: one spectrum_study point per figure, every point on the same payload (key `seed`, frames 0 ..)."""
    bad = check_args(frames, windows, Amount_ODFM_SpF)
    if bad:
        raise ValueError(bad)
    import torch
    import ofdm_course_amd as ofdm

    ofdm.init(device_index)
    dev = torch.device("cuda", device_index)
    plan = make_plan(ofdm, Nfft, N_carrier, Percent_pilot, Constellation, Amount_ODFM_SpF, precision, device_index)
    res = {"driver": "Task 3/Main_model_Task_3.m:85-143", "frames": frames, "windows": windows, "seed": seed,
           "clean_SNR_dB": CLEAN_SNR_DB, "first": plan.T_guard, "Nfft": Nfft, "N_carrier": N_carrier,
           "dtype": "f32" if precision == "fp32" else "f64", "scenarios": {}}
    for name, figure, settings in SCENARIOS:
        kw = study_args(settings, ofdm, Nfft)
        out = plan.spectrum_study(frames_per_point=frames, seed=seed, Register=c.REGISTER, first=plan.T_guard, n_windows=windows,
                                  device=dev, want_peak=True, max_frames_per_chunk=max_frames_per_chunk, **kw)
        mean = out["mean_power"][0].cpu().numpy()
        res["scenarios"][name] = {"figure": figure, "settings": {k: v for k, v in settings.items()}, "SNR_dB": kw["SNRs"][0],
                                  "power_sums": out["power_sums"][0].cpu().numpy(), "mean_power": mean,
                                  "amp_rms": out["amp_rms"][0].cpu().numpy(), "peak": out["peak"][0].cpu().numpy(),
                                  "null_power_share": float(mean[N_carrier:].sum() / mean.sum())}    # T3:155
    plan.close()
    return res


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=100, metavar="N", help="frames of 5 symbols per figure")
    ap.add_argument("--windows", type=int, default=1, help="symbols of each frame that are transformed (T3:138: the first)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--precision", choices=["fp32", "fp64"], default="fp64")
    ap.add_argument("--device", type=int, default=0, help="the one GPU the replay runs on")
    ap.add_argument("--json", default=None)
    return ap


def parse_args(argv=None):
    """The command line; arguments the replay cannot run with are a usage error."""
    ap = parser()
    a = ap.parse_args(argv)
    bad = check_args(a.frames, a.windows)
    if bad:
        ap.error(bad)
    return a


def main(argv=None):
    a = parse_args(argv)
    res = run(a.frames, a.windows, a.seed, a.precision, device_index=a.device)
    text = json.dumps(c.to_jsonable(res))
    if a.json:
        with open(a.json, "w") as f:
            f.write(text)
    else:
        print(text, flush=True)


if __name__ == "__main__":
    main()
