"""drivers/task4_ifo.py on the CPU: the study settings against the script's, the argument checks, the tiles dealt to the ranks with
the two reductions of a call, and the JSON layout with the library stubbed (a plan whose ifo_study records its arguments and
returns arrays of the documented shapes).  Nothing here touches a GPU."""
import json

import numpy as np
import pytest

from ofdm_course_amd.drivers import task4_ifo as t4i


def test_settings_are_the_scripts():
    assert t4i.FIGURE == "13b" and t4i.FIG_SNRS == tuple(float(s) for s in range(61))             # T4:114 SNRs=(0:1:60)
    assert (t4i.FIG_TIME_DELAY, t4i.FIG_FREQ_SHIFT) == (150, 0.24)                                # T4:119,:121
    assert t4i.figure_args() == dict(SNRs=list(t4i.FIG_SNRS), Time_Delay=150, Freq_Shift=0.24, stage="raw", time_desync=1, err_span=8)
    assert t4i.c3_args("receiver") == dict(SNRs=[30.0], Time_Delay="random", Freq_Shift="random", stage="receiver", time_desync=1,
                                           err_span=8)
    assert t4i.rel_args("raw") == dict(t4i.c3_args("raw"), Freq_Shift=12.24)
    assert "T4:124-125" in t4i.__doc__ and "T4:278-303" in t4i.__doc__ and "13b" in t4i.__doc__
    assert list(t4i.around(np.arange(10), 1, 2)) == [0, 0, 1, 2, 3] and list(t4i.around(np.arange(10), 9, 1)) == [8, 9, 0]


class _Plan:
    def __init__(self, lib, *args, **kw):
        self.lib, self.args, self.kw = lib, args, kw
        self.Nfft, self.T_guard, self.N_symb = args[0], args[1], args[2]
        self.closed = False

    def ifo_study(self, SNRs, frames_per_point, err_span=32, **kw):
        self.lib.calls.append(dict(kw, SNRs=SNRs, frames_per_point=frames_per_point, err_span=err_span))
        n, N, fpp = len(SNRs), self.Nfft, frames_per_point
        hist = np.zeros((n, N), np.int64)
        hist[:, 12] = fpp - 1                                          # one frame of every call without a line
        ehist = np.zeros((n, 2 * err_span + 1), np.int64)
        ehist[:, err_span] = fpp - 1
        return dict(spec_sums=np.full((n, N), 2.0 * fpp), spec_dropped=np.zeros((n, N), np.int64),
                    above_counts=np.tile(np.arange(N, dtype=np.int64) % 2 * fpp, (n, 1)), ifo_hist=hist,
                    no_line=np.ones(n, np.int64), err_hist=ehist, err_below=np.zeros(n, np.int64), err_above=np.zeros(n, np.int64),
                    hit=np.full(n, fpp - 1, np.int64), cfo_err=np.stack([np.full(n, 0.5 * (fpp - 1)), np.full(n, 0.25 * (fpp - 1))], axis=1),
                    fallback=np.arange(n, dtype=np.int64))

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
    t4i.main(["--json", str(out), "--frames", "7", "--seed", "3", "--frames-per-tile", "4"], lib=lib)
    res = json.loads(out.read_text())
    (plan,) = lib.plans
    assert plan.closed and lib.inits == [0]
    assert plan.args[:4] == (1024, 128, 5, 400) and plan.args[9] == "16QAM" and plan.kw == dict(precision="fp64", device=0)
    # two tiles (4 + 3 frames) for the figure and for each of the two calls of each stage
    assert [(c["frame0"], c["frames_per_point"]) for c in lib.calls] == [(0, 4), (4, 3)] * 5
    assert [c["stage"] for c in lib.calls] == ["raw"] * 6 + ["receiver"] * 4
    assert [c["Freq_Shift"] for c in lib.calls] == [0.24] * 2 + ["random"] * 2 + [12.24] * 2 + ["random"] * 2 + [12.24] * 2
    for call in lib.calls:
        assert call["seed"] == 3 and call["device"] == "cuda:0" and call["err_span"] == 8 and call["time_desync"] == 1
        assert list(call["Register"]) == [1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0] and call["max_frames_per_chunk"] == 0
    assert lib.calls[0]["SNRs"] == [float(s) for s in range(61)] and lib.calls[0]["Time_Delay"] == 150
    assert res["frames"] == 7 and res["seed"] == 3 and res["n_gpus"] == 1 and res["frames_per_tile"] == 4 and res["tiles_this_rank"] == 2
    fig = res["figure_13b"]
    assert set(fig) == {"figure", "SNR_dB", "Time_Delay", "Freq_Shift", "mean_abs_err", "rms_err", "no_line", "fallback", "ifo_hist"}
    # 7 frames in two tiles, one of each tile without a line: 5 with one; sum |e| = 0.5 * 5, sum e^2 = 0.25 * 5
    assert fig["no_line"] == [2] * 61 and fig["mean_abs_err"] == [0.5] * 61 and fig["rms_err"] == [0.5] * 61
    assert fig["fallback"] == [2 * p for p in range(61)] and np.asarray(fig["ifo_hist"]).shape == (61, 1024)
    assert set(res["c3"]) == {"raw", "receiver"}
    for tab in res["c3"].values():
        assert set(tab) == {"SNR_dB", "hit_rate", "no_line_rate", "mean_abs_cfo_err", "fallback", "err_hist", "err_below", "err_above",
                            "err_offsets", "rel_Freq_Shift", "rel_bins", "above_rel", "ifo_rel", "rel_hit_rate"}
        assert tab["hit_rate"] == 5 / 7 and tab["no_line_rate"] == 2 / 7 and tab["mean_abs_cfo_err"] == 0.5
        assert tab["err_offsets"] == list(range(-8, 9)) and tab["err_hist"][8] == 5 and sum(tab["err_hist"]) == 5
        assert tab["rel_bins"] == list(range(4, 21)) and tab["ifo_rel"][8] == 5 and sum(tab["ifo_rel"]) == 5
        assert tab["above_rel"] == [7 * (k % 2) for k in range(4, 21)]


def test_tiles_and_reductions():
    counts = np.arange(6, dtype=np.int64).reshape(2, 3)
    sums = np.arange(4, dtype=np.float64).reshape(2, 2)
    got_c, got_s = t4i.reduce_over_ranks(counts, sums)                 # one rank: both collectives are no-ops
    assert np.array_equal(got_c, counts) and np.array_equal(got_s, sums)
    seen = []
    for rank in range(3):
        seen += t4i.tiles(10, 4, rank, 3)
    assert sorted(seen) == [(0, 4), (4, 4), (8, 2)]
    calls = []

    def reduce(c, s):
        calls.append((c.dtype, s.dtype, c.shape, s.shape))
        return 2 * c, 2.0 * s                                          # a second rank that saw the same

    lib = _Lib()
    plan = lib.RxPlan(1024, 128, 5, 400)
    out = t4i.study_call(plan, [(0, 3)], 2, reduce, SNRs=[1.0, 2.0], err_span=8)
    assert calls == [(np.dtype(np.int64), np.dtype(np.float64), (2, 3 * 1024 + 17 + 5), (2, 1024 + 2))]   # one of each per call
    assert out["hit"].tolist() == [4, 4] and out["no_line"].tolist() == [2, 2] and out["cfo_err"][0].tolist() == [2.0, 1.0]
    assert out["ifo_hist"].shape == (2, 1024) and out["err_hist"].shape == (2, 17) and out["spec_sums"][0, 0] == 12.0


def test_argument_checks_and_command_line(capsys):
    a = t4i.parse_args(["--json", "out.json", "--frames", "7"])
    assert (a.json, a.frames, a.seed, a.precision, a.device, a.frames_per_tile) == ("out.json", 7, 1, "fp64", None, 4096)
    with pytest.raises(SystemExit):
        t4i.parse_args(["--frames", "0"])
    assert "--frames must be >= 1" in capsys.readouterr().err
    lib = _Lib()
    with pytest.raises(ValueError, match="--frames"):
        t4i.run(frames=0, lib=lib)                                       # refused before the library is touched
    assert not lib.inits and not lib.plans
