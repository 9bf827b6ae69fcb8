"""drivers/task4_hest.py on the CPU: the study settings against the script's, the argument checks, the tiles dealt to the ranks with
the two reductions of a call, and the JSON layout with the library stubbed (a plan whose channel_study records its arguments and
returns arrays of the documented shapes).  Nothing here touches a GPU."""
import json

import numpy as np
import pytest

from ofdm_course_amd.drivers import task4_hest as t4h


def test_settings_are_the_scripts():
    assert t4h.FIGURE == "21" and t4h.FIG_SNRS == (3000.0, 25.0)
    assert t4h.STUDY_SNRS == tuple(float(s) for s in range(31)) and t4h.STUDY_PERCENT_PILOT == (15, 25)
    assert np.array_equal(t4h.CHANNEL_TAPS, [[0, 1.0], [4, 0.6], [10, 0.3]])                          # the 3-tap channel
    h = np.ones(3)
    assert t4h.figure_args(h) == dict(SNRs=[3000.0, 25.0], h=h, time_desync=0, freq_desync=0, bins=dict(n=60, lo=-50.0, hi=10.0))
    off, on = t4h.study_args(h, False), t4h.study_args(h, True)
    assert (off["time_desync"], off["freq_desync"]) == (0, 0) and "Time_Delay" not in off and "Freq_Shift" not in off
    assert (on["time_desync"], on["freq_desync"], on["Time_Delay"], on["Freq_Shift"]) == (1, 1, "random", "random")
    assert "T4:252-256" in t4h.__doc__ and ":318-332" in t4h.__doc__ and "Figure 21" in t4h.__doc__


class _Plan:
    def __init__(self, lib, *args, **kw):
        self.lib, self.args, self.kw = lib, args, kw
        self.Nfft, self.N_carrier, self.n_pilots = args[0], args[3], len(args[4])
        self.closed = False

    def channel_study(self, SNRs, frames_per_point, bins, **kw):
        self.lib.calls.append(dict(kw, SNRs=SNRs, frames_per_point=frames_per_point, bins=bins, n_pilots=self.n_pilots))
        n, nc, npil, fpp = len(SNRs), self.N_carrier, self.n_pilots, frames_per_point
        drop = np.zeros((n, nc), np.int64)
        sync = kw["time_desync"]
        if sync:
            drop[:] = 1                                               # one frame of every call without a finite estimate
        kept = fpp - (1 if sync else 0)
        hist = np.zeros((n, bins["n"]), np.int64)
        hist[:, 3] = kept
        return dict(est_amp_sums=np.full((n, nc), 2.0 * kept), true_amp_sums=np.full((n, nc), 1.5 * kept),
                    err_sums=np.full((n, nc), 0.5 * kept), amp_err_sums=np.full((n, nc), 0.25 * kept), dropped=drop,
                    pilot_amp_sums=np.full((n, npil), 3.0 * kept), pilot_err_sums=np.full((n, npil), 0.125 * kept),
                    pilot_dropped=drop[:, :npil], nmse_sums=np.full(n, 0.5 * kept * nc), amp_nmse_sums=np.full(n, 0.25 * kept * nc),
                    nmse_hist=hist, nmse_below=np.zeros(n, np.int64), nmse_above=np.zeros(n, np.int64),
                    nmse_nan=np.full(n, fpp - kept, np.int64), status_counts=np.tile(np.array([fpp, 0, 0, 0], np.int64), (n, 1)))

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

    @staticmethod
    def get_MP_channel_resp(taps, nfft):
        h = np.zeros(11, np.complex128)
        for d, a in np.asarray(taps):
            h[int(d)] = a
        return h, np.fft.fft(h, nfft)

    def RxPlan(self, *args, **kw):
        self.plans.append(_Plan(self, *args, **kw))
        return self.plans[-1]


def test_json_layout_with_the_library_stubbed(tmp_path):
    lib = _Lib()
    out = tmp_path / "out.json"
    t4h.main(["--json", str(out), "--frames", "7", "--seed", "3", "--frames-per-tile", "4"], lib=lib)
    res = json.loads(out.read_text())
    p15, p25 = lib.plans
    assert p15.closed and p25.closed and lib.inits == [0] and p15.n_pilots < p25.n_pilots
    assert p15.args[:4] == (1024, 128, 5, 400) and p15.args[9] == "16QAM" and p15.kw == dict(precision="fp64", device=0)
    # two tiles (4 + 3 frames) for the figure and for each mode of each pilot share
    assert [(c["frame0"], c["frames_per_point"]) for c in lib.calls] == [(0, 4), (4, 3)] * 5
    assert [c["time_desync"] for c in lib.calls] == [0] * 4 + [1] * 2 + [0] * 2 + [1] * 2
    assert [c["n_pilots"] for c in lib.calls] == [p15.n_pilots] * 6 + [p25.n_pilots] * 4
    for call in lib.calls:
        assert call["seed"] == 3 and call["device"] == "cuda:0" and call["bins"] == dict(n=60, lo=-50.0, hi=10.0)
        assert list(call["Register"]) == [1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0] and call["max_frames_per_chunk"] == 0
        assert np.array_equal(np.nonzero(call["h"])[0], [0, 4, 10])
        assert call["freq_desync"] == call["time_desync"] and (call.get("Time_Delay") == "random") == bool(call["time_desync"])
    assert lib.calls[0]["SNRs"] == [3000.0, 25.0] and lib.calls[2]["SNRs"] == [float(s) for s in range(31)]
    assert res["frames"] == 7 and res["seed"] == 3 and res["n_gpus"] == 1 and res["frames_per_tile"] == 4 and res["tiles_this_rank"] == 2
    fig = res["figure_21"]
    assert set(fig) == {"figure", "SNR_dB", "pilotCarriers", "mean_est_amp", "mean_true_amp", "pilot_stems"}
    assert np.asarray(fig["mean_est_amp"]).shape == (2, 400) and len(fig["pilotCarriers"]) == p15.n_pilots
    assert fig["mean_est_amp"][0][0] == 2.0 and fig["mean_true_amp"][1][399] == 1.5 and fig["pilot_stems"][0][0] == 3.0
    assert set(res["study"]) == {"15", "25"}
    for tab in res["study"].values():
        assert set(tab) == {"sync_off", "sync_on"}
        for mode, t in tab.items():
            assert set(t) == {"SNR_dB", "NMSE", "amp_NMSE", "nmse_profile", "pilot_err", "frames_kept", "nmse_nan", "status_counts"}
            # the means over the frames kept: 7, or 5 where one frame of each of the two tiles was dropped
            assert t["NMSE"] == [0.5] * 31 and t["amp_NMSE"] == [0.25] * 31 and t["pilot_err"][0][0] == 0.125
            assert t["frames_kept"] == [5.0 if mode == "sync_on" else 7.0] * 31 and t["nmse_nan"] == [2 if mode == "sync_on" else 0] * 31
            assert t["status_counts"][0] == [7, 0, 0, 0]


def test_tiles_and_reductions():
    seen = []
    for rank in range(3):
        seen += t4h.tiles(10, 4, rank, 3)
    assert sorted(seen) == [(0, 4), (4, 4), (8, 2)]
    calls = []

    def reduce(c, s):
        calls.append((c.dtype, s.dtype, c.shape, s.shape))
        return 2 * c, 2.0 * s                                          # a second rank that saw the same

    lib = _Lib()
    plan = lib.RxPlan(1024, 128, 5, 400, list(range(1, 61)))
    out = t4h.study_call(plan, [(0, 3)], 2, reduce, SNRs=[1.0, 2.0], bins=dict(n=60, lo=-50.0, hi=10.0), time_desync=0)
    # one int64 and one float64 reduction per call
    assert calls == [(np.dtype(np.int64), np.dtype(np.float64), (2, 400 + 60 + 60 + 3 + 4), (2, 4 * 400 + 2 * 60 + 2))]
    assert out["status_counts"].tolist() == [[6, 0, 0, 0]] * 2 and out["nmse_hist"][0, 3] == 6 and out["est_amp_sums"][0, 0] == 12.0
    assert out["nmse_sums"].tolist() == [0.5 * 3 * 400 * 2] * 2 and out["pilot_err_sums"].shape == (2, 60)
    cv = t4h.curves(out, 6)
    assert cv["mean_est_amp"][0, 0] == 2.0 and cv["pilot_stems"][1, 59] == 3.0 and cv["frames_kept"].tolist() == [6.0, 6.0]


def test_argument_checks_and_command_line(capsys):
    a = t4h.parse_args(["--json", "out.json", "--frames", "7"])
    assert (a.json, a.frames, a.seed, a.precision, a.device, a.frames_per_tile) == ("out.json", 7, 1, "fp64", None, 4096)
    with pytest.raises(SystemExit):
        t4h.parse_args(["--frames", "0"])
    assert "--frames must be >= 1" in capsys.readouterr().err
    lib = _Lib()
    with pytest.raises(ValueError, match="--frames"):
        t4h.run(frames=0, lib=lib)                                       # refused before the library is touched
    assert not lib.inits and not lib.plans
