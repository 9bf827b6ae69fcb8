"""The coarse synchroniser's pictures of the `Task 4/README.md` report, replayed on the device over many frames.

Figures 6-9 of the report are `plot(abs(AutoCorr))` of `Task 4/Main_model_Task_4.m:282-287` for four window widths of
`AutoCorrFunction(Rx_OFDM_Signal, W, Nfft)`: W = 1, T_Guard / 2, T_Guard and Nfft -- the report's argument for W = T_Guard / 2.
Figure 13a is "Влияние шума на оценку частотного сдвига" (T4:113-135): the error of the estimated frequency offset over SNR 0:1:60
at Time_Delay 150 and Freq_Shift 0.24, W = T_Guard.  Here every ACF figure is one `RxPlan.sync_study` call (ofdm_sync_study) of one
point, and figure 13a one call of 61 points, on the T4 geometry -- Nfft 1024, 400 carriers, T_Guard 128, 15 % pilots at 4/3
max|dict|, 16QAM, frames of 5 symbols with the Scrambler register of T4:43 reset per frame --: `--frames` frames per point are
generated and correlated on one GPU and only the sums come back.  `mean_acf` is the report's curve averaged over the frames; with
`--frames 1` it is the report's single line for the Philox payload.  Figure 13a reports the mean |e| of the fractional offset alone,
e the wrapped error of FreqOffset against Freq_Shift: the integer part that remove_IFO adds in the script is not estimated here
(the Task-4 sweep's cfo_abs_err covers the total).

The script's Noise stage is off for the ACF figures; the generator always runs Noise, so those run at CLEAN_SNR_DB = 3000 dB, the
convention of drivers/task3_spectrum.py: the frames are the noise-free ones to rounding.

    python -m ofdm_course_amd.drivers.task4_acf --json out.json --frames 1000
"""
from __future__ import annotations

import argparse
import json

import numpy as np

from . import common as c

CLEAN_SNR_DB = 3000.0

# (name, figure of Task 4/README.md, WidthWindow as a function of (Nfft, T_Guard))
ACF_FIGURES = (
    ("W_1", 6, lambda nfft, tg: 1),
    ("W_half_guard", 7, lambda nfft, tg: tg // 2),
    ("W_guard", 8, lambda nfft, tg: tg),
    ("W_nfft", 9, lambda nfft, tg: nfft),
)
FFO_FIGURE = 13                                                                   # 13a
FFO_SNRS = tuple(float(s) for s in range(0, 61))                                  # T4:114
FFO_TIME_DELAY, FFO_FREQ_SHIFT = 150, 0.24                                        # T4:119,:121


def check_args(frames):
    """What the replay needs of its arguments; the text of the refusal, or None."""
    if frames < 1:
        return "--frames must be >= 1"
    return None


def make_plan(lib, Nfft=1024, N_carrier=400, Percent_pilot=15, Constellation="16QAM", Amount_ODFM_SpF=5, precision="fp64",
              device_index=None):
    """The plan of one T4 frame (T4:6-36): T_Guard = Nfft / 8, the percent pilot rule, pilots at 4/3 max|dict| with alternating
    sign.  (The plan's estimator settings are not used by the study.)"""
    _, pilotCarriers, dataCarriers = c.layout_percent(Nfft, N_carrier, Percent_pilot, tail=2)
    dict_, _ = lib.constellation_func(Constellation)
    amp = 4 / 3 * np.max(np.abs(dict_))
    pv = np.where(np.arange(len(pilotCarriers)) % 2 == 0, amp, -amp).astype(np.complex128)
    return lib.RxPlan(Nfft, Nfft // 8, Amount_ODFM_SpF, N_carrier, pilotCarriers, dataCarriers, pv, min(8, Nfft), 1, Constellation,
                      precision=precision, device=device_index)


def acf_args(width):
    """The sync_study arguments of one ACF figure: the clean channel, one point."""
    return dict(SNRs=[CLEAN_SNR_DB], width=int(width))


def ffo_args(T_guard):
    """The sync_study arguments of figure 13a."""
    return dict(SNRs=list(FFO_SNRS), Time_Delay=FFO_TIME_DELAY, Freq_Shift=FFO_FREQ_SHIFT, width=int(T_guard))


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def run(frames=100, seed=1, precision="fp64", Nfft=1024, N_carrier=400, Percent_pilot=15, Constellation="16QAM", Amount_ODFM_SpF=5,
        device_index=0, max_frames_per_chunk=0, lib=None):
    """Returns {"acf": {name: {figure, width, n_out, acf_sums, acf_dropped, mean_acf, acf_peak, tg_hist, fallback, phase_hist}},
    "ffo": {figure, SNR_dB, Time_Delay, Freq_Shift, width, mean_abs_err, rms_err, fallback, phase_hist}, ...}: one sync_study call
    per ACF figure and one for figure 13a, every point on the same payload (key `seed`, frames 0 ..).  lib: the library module
    (default: ofdm_course_amd)."""
    bad = check_args(frames)
    if bad:
        raise ValueError(bad)
    if lib is None:
        import ofdm_course_amd as lib

    lib.init(device_index)
    dev = f"cuda:{device_index}"
    plan = make_plan(lib, Nfft, N_carrier, Percent_pilot, Constellation, Amount_ODFM_SpF, precision, device_index)
    common = dict(frames_per_point=frames, seed=seed, Register=c.REGISTER, device=dev, max_frames_per_chunk=max_frames_per_chunk)
    res = {"driver": "Task 4/Main_model_Task_4.m:113-135,:278-287", "frames": frames, "seed": seed, "clean_SNR_dB": CLEAN_SNR_DB,
           "Nfft": Nfft, "N_carrier": N_carrier, "T_guard": plan.T_guard, "dtype": "f32" if precision == "fp32" else "f64",
           "acf": {}}
    for name, figure, width_of in ACF_FIGURES:
        kw = acf_args(width_of(Nfft, plan.T_guard))
        out = plan.sync_study(want_peak=True, **common, **kw)
        res["acf"][name] = {"figure": figure, "width": kw["width"], "n_out": int(out["acf_sums"].shape[1]),
                            "acf_sums": _np(out["acf_sums"][0]), "acf_dropped": _np(out["acf_dropped"][0]),
                            "mean_acf": _np(out["mean_acf"][0]), "acf_peak": _np(out["acf_peak"][0]),
                            "tg_hist": _np(out["tg_hist"][0]), "fallback": int(_np(out["fallback"])[0]),
                            "phase_hist": _np(out["phase_hist"][0])}
    kw = ffo_args(plan.T_guard)
    out = plan.sync_study(**common, **kw)
    ffo = _np(out["ffo_err"])
    res["ffo"] = {"figure": FFO_FIGURE, "SNR_dB": kw["SNRs"], "Time_Delay": kw["Time_Delay"], "Freq_Shift": kw["Freq_Shift"],
                  "width": kw["width"], "mean_abs_err": ffo[:, 0] / frames, "rms_err": np.sqrt(ffo[:, 1] / frames),
                  "fallback": _np(out["fallback"]), "phase_hist": _np(out["phase_hist"])}
    plan.close()
    return res


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=100, metavar="N", help="frames of 5 symbols per point")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--precision", choices=["fp32", "fp64"], default="fp64")
    ap.add_argument("--device", type=int, default=0, help="the one GPU the replay runs on")
    ap.add_argument("--json", default=None)
    return ap


def parse_args(argv=None):
    """The command line; arguments the replay cannot run with are a usage error."""
    ap = parser()
    a = ap.parse_args(argv)
    bad = check_args(a.frames)
    if bad:
        ap.error(bad)
    return a


def main(argv=None, lib=None):
    a = parse_args(argv)
    res = run(a.frames, a.seed, a.precision, device_index=a.device, lib=lib)
    text = json.dumps(c.to_jsonable(res))
    if a.json:
        with open(a.json, "w") as f:
            f.write(text)
    else:
        print(text, flush=True)


if __name__ == "__main__":
    main()
