"""drivers/task4_tau.py on the CPU: the figure table against the report's figure numbers and the script's settings, the argument
checks, the command line, the dealing of the frames to the ranks, and -- with the library stubbed by a plan whose fine_study records
its arguments and returns tables that depend on which frames it was given -- the JSON layout, the frame0 split and the two
reductions: two simulated ranks reduce to what one rank computes.  Nothing here touches a GPU."""
import json

import numpy as np
import pytest

from ofdm_course_amd.drivers import task4_tau as t4t


def test_figures_and_study_are_the_reports():
    assert t4t.FIGURES == (("clean", "18a", 3000.0), ("snr_25dB", "18b", 25.0))
    assert t4t.TIME_DELAY == 12 and t4t.STUDY_SNRS == tuple(float(s) for s in range(41))          # T4:140,:148
    assert t4t.figure_args(25.0) == dict(SNRs=[25.0], Time_Delay=12, time_desync=1, freq_desync=0, variant="T4")
    assert t4t.study_args() == dict(SNRs=list(t4t.STUDY_SNRS), Time_Delay=12, time_desync=1, freq_desync=0, variant="T4",
                                    bins=dict(n=64, lo=-4.0, hi=4.0))
    assert t4t.symbol2(68) == slice(68, 135) and np.isfinite(10.0 ** (t4t.CLEAN_SNR_DB / 10.0))
    assert "CLEAN_SNR_DB = 3000 dB" in t4t.__doc__ and "T4:137-203" in t4t.__doc__ and "fine_sync.m:10-30" in t4t.__doc__


class _Plan:
    """fine_study over the frames frame0 .. frame0 + frames_per_point - 1: frame g is kept at every entry when g is even, falls
    into bin g mod n, has tau = NaN when g is a multiple of 5 and the error (g + 1) / 4; every entry of taus is 0.5."""

    def __init__(self, lib, *args, **kw):
        self.lib, self.args, self.kw = lib, args, kw
        self.Nfft, self.T_guard, self.N_symb = args[0], args[1], args[2]
        self.n_pilots = len(args[4])
        self.closed = False

    def fine_study(self, SNRs, frames_per_point, frame0=0, bins=None, **kw):
        self.lib.calls.append(dict(kw, SNRs=SNRs, frames_per_point=frames_per_point, frame0=frame0, bins=bins))
        n, L, fpp = len(SNRs), self.n_pilots * self.N_symb - 1, frames_per_point
        nb = 64 if bins is None else bins["n"]
        g = np.arange(frame0, frame0 + fpp)
        hist = np.zeros((n, nb), np.int64)
        np.add.at(hist, (slice(None), g % nb), 1)
        err = (g + 1) / 4.0
        return dict(tau_curve_sums=np.full((n, L), 0.5 * fpp), curve_dropped=np.zeros((n, L), np.int64),
                    keep_counts=np.full((n, L), int(np.sum(g % 2 == 0)), np.int64), tau_hist=hist, tau_below=np.zeros(n, np.int64),
                    tau_above=np.full(n, int(np.sum(g % 3 == 0)), np.int64), tau_nan=np.full(n, int(np.sum(g % 5 == 0)), np.int64),
                    tau_err=np.stack([np.full(n, err.sum()), np.full(n, (err * err).sum())], axis=1))

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
    t4t.main(["--json", str(out), "--frames", "9", "--seed", "3"], lib=lib)
    res = json.loads(out.read_text())
    (plan,) = lib.plans
    assert plan.closed and lib.inits == [0]
    assert plan.args[:4] == (1024, 128, 5, 400) and plan.args[9] == "16QAM" and plan.kw == dict(precision="fp64", device=0)
    assert len(plan.args[4]) == 68
    # one tile: one call per figure, then the study as one call of 41 points
    assert [c["SNRs"] for c in lib.calls] == [[3000.0], [25.0], [float(s) for s in range(41)]]
    for call in lib.calls:
        assert call["frames_per_point"] == 9 and call["frame0"] == 0 and call["seed"] == 3 and call["device"] == "cuda:0"
        assert (call["time_desync"], call["freq_desync"], call["variant"]) == (1, 0, "T4") and call["max_frames_per_chunk"] == 0
        assert call["Time_Delay"] == 12 and call["bins"] == dict(n=64, lo=-4.0, hi=4.0)
        assert list(call["Register"]) == [1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0]
    assert res["frames"] == 9 and res["seed"] == 3 and res["Time_Delay"] == 12 and res["n_pilots"] == 68 and res["dtype"] == "f64"
    assert (res["n_gpus"], res["frames_per_tile"], res["tiles_this_rank"]) == (1, 4096, 1)
    assert list(res["figures"]) == ["clean", "snr_25dB"]
    for name, figure, snr in t4t.FIGURES:
        fig = res["figures"][name]
        assert set(fig) == {"figure", "SNR_dB", "pilot_carriers", "tau_curve", "tau_curve_samples", "keep_rate", "tau_nan"}
        assert fig["figure"] == figure and fig["SNR_dB"] == snr and fig["tau_nan"] == 2                # frames 0 and 5
        assert len(fig["pilot_carriers"]) == len(fig["tau_curve"]) == len(fig["keep_rate"]) == 67 and fig["pilot_carriers"][0] == 1
        assert fig["tau_curve"][0] == 0.5 and fig["tau_curve_samples"][0] == 512.0       # sums / (frames - dropped), x Nfft
        assert fig["keep_rate"][0] == 5 / 9                                              # frames 0, 2, 4, 6, 8
    st = res["study"]
    assert set(st) == {"SNR_dB", "mean_abs_err", "rms_err", "nan_share", "keep_share", "tau_hist", "tau_below", "tau_above", "tau_nan",
                       "edges"}
    err = np.arange(1, 10) / 4.0
    assert st["SNR_dB"] == [float(s) for s in range(41)] and np.allclose(st["mean_abs_err"], err.sum() / 7)
    assert np.allclose(st["rms_err"], np.sqrt((err * err).sum() / 7)) and st["nan_share"] == [2 / 9] * 41
    assert np.allclose(st["keep_share"], 5 / 9) and len(st["edges"]) == 65 and st["tau_above"] == [3] * 41
    assert len(st["tau_hist"]) == 41 and st["tau_hist"][0] == [1] * 9 + [0] * 55


def test_frames_are_dealt_as_a_partition():
    for frames, per_tile in ((9, 2), (37, 5), (4096, 4096), (4097, 4096), (3, 10)):
        for world in (1, 2, 3, 8):
            seen = []
            for rank in range(world):
                for frame0, nf in t4t.tiles(frames, per_tile, rank, world):
                    assert 1 <= nf <= per_tile and frame0 % per_tile == 0
                    seen += list(range(frame0, frame0 + nf))
            assert sorted(seen) == list(range(frames))
    assert t4t.tiles(9, 2, 0, 2) == [(0, 2), (4, 2), (8, 1)] and t4t.tiles(9, 2, 1, 2) == [(2, 2), (6, 2)]
    assert t4t.tiles(3, 10, 1, 2) == []                                   # a rank without a tile still joins the reductions


def test_two_ranks_reduce_to_what_one_rank_computes():
    """The frame0 split and the two reductions against the recording library: rank 1's tables are captured at its reductions and
    added at rank 0's, as the int64 and the float64 all-reduce would."""
    whole = t4t.run(frames=9, seed=3, lib=_Lib(), frames_per_tile=2)
    assert whole["tiles_this_rank"] == 5
    sent, seen = [], []

    def capture(counts, sums):
        sent.append((counts.copy(), sums.copy()))
        return counts, sums

    def add_other(counts, sums):
        other_counts, other_sums = sent[len(seen)]
        seen.append((counts.dtype, sums.dtype, counts.shape, sums.shape))
        return counts + other_counts, sums + other_sums

    lib1, lib0 = _Lib(), _Lib()
    t4t.run(frames=9, seed=3, lib=lib1, frames_per_tile=2, rank=1, world=2, reduce=capture)
    both = t4t.run(frames=9, seed=3, lib=lib0, frames_per_tile=2, rank=0, world=2, reduce=add_other)
    assert len(sent) == len(seen) == 3                                   # one pair of reductions per figure and one for the study
    L = 68 * 5 - 1
    assert seen == [(np.int64, np.float64, (n, 2 * L + 64 + 3), (n, L + 2)) for n in (1, 1, 41)]
    # every call of a rank is one of its tiles, each of the three studies over all of them
    assert [(c["frame0"], c["frames_per_point"]) for c in lib0.calls] == [(0, 2), (4, 2), (8, 1)] * 3
    assert [(c["frame0"], c["frames_per_point"]) for c in lib1.calls] == [(2, 2), (6, 2)] * 3
    assert (both["n_gpus"], both["tiles_this_rank"]) == (2, 3)
    for key in ("figures", "study"):
        a, b = json.dumps(t4t.c.to_jsonable(whole[key])), json.dumps(t4t.c.to_jsonable(both[key]))
        assert a == b, key
    # the default reduction is the identity on one rank, on the dtypes the collectives take
    counts, sums = np.arange(6, dtype=np.int64).reshape(2, 3), np.ones((2, 2))
    rc, rs = t4t.reduce_over_ranks(counts, sums)
    assert np.array_equal(rc, counts) and rc.dtype == np.int64 and np.array_equal(rs, sums) and rs.dtype == np.float64


def test_argument_checks_and_command_line(capsys):
    assert t4t.check_args(1) is None and t4t.check_args(0) == "--frames must be >= 1"
    assert t4t.check_args(5, 0) == "--frames-per-tile must be >= 1" and t4t.check_args(5, 1) is None
    a = t4t.parse_args(["--json", "out.json", "--frames", "7", "--frames-per-tile", "3"])
    assert (a.json, a.frames, a.seed, a.precision, a.device, a.frames_per_tile, a.backend) == ("out.json", 7, 1, "fp64", None, 3, "nccl")
    assert t4t.parse_args([]).frames == 100 and t4t.parse_args([]).frames_per_tile == 4096
    for argv, text in ((["--frames", "0"], "--frames must be >= 1"), (["--frames-per-tile", "0"], "--frames-per-tile must be >= 1")):
        with pytest.raises(SystemExit):
            t4t.parse_args(argv)
        assert text in capsys.readouterr().err
    lib = _Lib()
    with pytest.raises(ValueError, match="--frames"):
        t4t.run(frames=0, lib=lib)                                       # refused before the library is touched
    assert not lib.inits and not lib.plans
