"""drivers/task4_acf.py on the CPU: the figure table against the report's figure numbers and the script's settings, the argument
checks, the command line, and the JSON layout with the library stubbed (a plan whose sync_study records its arguments and returns
arrays of the documented shapes).  Nothing here touches a GPU."""
import json

import numpy as np
import pytest

from ofdm_course_amd.drivers import task4_acf as t4a


def test_figures_are_the_acf_and_offset_pictures_of_the_report():
    assert [(n, f, w(1024, 128)) for n, f, w in t4a.ACF_FIGURES] == [("W_1", 6, 1), ("W_half_guard", 7, 64), ("W_guard", 8, 128),
                                                                     ("W_nfft", 9, 1024)]
    assert t4a.FFO_FIGURE == 13 and t4a.FFO_SNRS == tuple(float(s) for s in range(61))            # T4:114 SNRs=(0:1:60)
    assert (t4a.FFO_TIME_DELAY, t4a.FFO_FREQ_SHIFT) == (150, 0.24)                                # T4:119,:121
    assert t4a.acf_args(64) == dict(SNRs=[3000.0], width=64)
    assert t4a.ffo_args(128) == dict(SNRs=list(t4a.FFO_SNRS), Time_Delay=150, Freq_Shift=0.24, width=128)
    assert np.isfinite(10.0 ** (t4a.CLEAN_SNR_DB / 10.0))
    assert "CLEAN_SNR_DB = 3000 dB" in t4a.__doc__ and "T4:113-135" in t4a.__doc__ and "remove_IFO" in t4a.__doc__


class _Plan:
    def __init__(self, lib, *args, **kw):
        self.lib, self.args, self.kw = lib, args, kw
        self.Nfft, self.T_guard, self.N_symb = args[0], args[1], args[2]
        self.closed = False

    def sync_study(self, SNRs, frames_per_point, width=None, want_peak=False, **kw):
        self.lib.calls.append(dict(kw, SNRs=SNRs, frames_per_point=frames_per_point, width=width, want_peak=want_peak))
        n, n_out, stride = len(SNRs), (self.Nfft + self.T_guard) * self.N_symb - width - self.Nfft, self.Nfft + self.T_guard
        out = dict(acf_sums=np.full((n, n_out), 2.0 * frames_per_point), acf_dropped=np.zeros((n, n_out), np.int64),
                   mean_acf=np.full((n, n_out), 2.0), tg_hist=np.zeros((n, n_out), np.int64), fallback=np.arange(n, dtype=np.int64),
                   phase_hist=np.zeros((n, stride), np.int64),
                   ffo_err=np.stack([np.full(n, 0.5 * frames_per_point), np.full(n, 0.25 * frames_per_point)], axis=1))
        if want_peak:
            out["acf_peak"] = np.full((n, n_out), 3.0)
        return out

    def close(self):
        self.closed = True


class _Lib:
    def __init__(self):
        self.calls, self.plans, self.inits = [], [], []

    def init(self, device):
        self.inits.append(device)

    @staticmethod
    def constellation_func(name):
        assert name == "16QAM"
        return np.array([3 + 3j, 1 - 1j]) / np.sqrt(10), 4

    def RxPlan(self, *args, **kw):
        self.plans.append(_Plan(self, *args, **kw))
        return self.plans[-1]


def test_json_layout_with_the_library_stubbed(tmp_path):
    lib = _Lib()
    out = tmp_path / "out.json"
    t4a.main(["--json", str(out), "--frames", "7", "--seed", "3"], lib=lib)
    res = json.loads(out.read_text())
    # one plan of the T4 geometry, closed at the end
    (plan,) = lib.plans
    assert plan.closed and lib.inits == [0]
    assert plan.args[:4] == (1024, 128, 5, 400) and plan.args[9] == "16QAM" and plan.kw == dict(precision="fp64", device=0)
    pc, dc, pv = plan.args[4], plan.args[5], plan.args[6]
    assert len(pc) == len(pv) == 68 and len(dc) == 400 - 68 and pc[0] == 1 and pc[-1] == 400          # T4:16-24
    amp = 4 / 3 * np.sqrt(18 / 10)
    assert np.allclose(pv[0::2], amp) and np.allclose(pv[1::2], -amp)                                   # T4:31-35
    # four ACF calls of one clean point each, then figure 13a as one call of 61 points
    assert [c["width"] for c in lib.calls] == [1, 64, 128, 1024, 128]
    for call in lib.calls:
        assert call["frames_per_point"] == 7 and call["seed"] == 3 and call["device"] == "cuda:0"
        assert list(call["Register"]) == [1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0] and call["max_frames_per_chunk"] == 0
    for call in lib.calls[:4]:
        assert call["SNRs"] == [3000.0] and call["want_peak"] and "Time_Delay" not in call and "Freq_Shift" not in call
    last = lib.calls[4]
    assert last["SNRs"] == [float(s) for s in range(61)] and last["Time_Delay"] == 150 and last["Freq_Shift"] == 0.24
    assert not last["want_peak"]
    # the layout
    assert res["frames"] == 7 and res["seed"] == 3 and res["clean_SNR_dB"] == 3000.0 and res["T_guard"] == 128
    assert res["Nfft"] == 1024 and res["N_carrier"] == 400 and res["dtype"] == "f64"
    assert list(res["acf"]) == ["W_1", "W_half_guard", "W_guard", "W_nfft"]
    for name, figure, width_of in t4a.ACF_FIGURES:
        fig = res["acf"][name]
        w = width_of(1024, 128)
        n_out = 5760 - w - 1024
        assert fig["figure"] == figure and fig["width"] == w and fig["n_out"] == n_out and fig["fallback"] == 0
        assert set(fig) == {"figure", "width", "n_out", "acf_sums", "acf_dropped", "mean_acf", "acf_peak", "tg_hist", "fallback",
                            "phase_hist"}
        assert len(fig["acf_sums"]) == len(fig["mean_acf"]) == len(fig["acf_peak"]) == len(fig["tg_hist"]) == n_out
        assert len(fig["phase_hist"]) == 1152 and fig["mean_acf"][0] == 2.0 and fig["acf_sums"][0] == 14.0
    ffo = res["ffo"]
    assert set(ffo) == {"figure", "SNR_dB", "Time_Delay", "Freq_Shift", "width", "mean_abs_err", "rms_err", "fallback", "phase_hist"}
    assert ffo["figure"] == 13 and ffo["SNR_dB"] == [float(s) for s in range(61)] and ffo["width"] == 128
    assert ffo["mean_abs_err"] == [0.5] * 61 and ffo["rms_err"] == [0.5] * 61 and ffo["fallback"] == list(range(61))
    assert len(ffo["phase_hist"]) == 61 and len(ffo["phase_hist"][0]) == 1152


def test_argument_checks_and_command_line(capsys):
    assert t4a.check_args(1) is None and t4a.check_args(10 ** 6) is None
    assert t4a.check_args(0) == "--frames must be >= 1" and t4a.check_args(-3) == "--frames must be >= 1"
    a = t4a.parse_args(["--json", "out.json", "--frames", "7"])
    assert (a.json, a.frames, a.seed, a.precision, a.device) == ("out.json", 7, 1, "fp64", 0)
    assert t4a.parse_args([]).frames == 100
    with pytest.raises(SystemExit):
        t4a.parse_args(["--frames", "0"])
    assert "--frames must be >= 1" in capsys.readouterr().err
    lib = _Lib()
    with pytest.raises(ValueError, match="--frames"):
        t4a.run(frames=0, lib=lib)                                       # refused before the library is touched
    assert not lib.inits and not lib.plans
