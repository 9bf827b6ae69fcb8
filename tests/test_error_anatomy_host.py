"""drivers/error_anatomy.py on the CPU: the pure table shaping on synthetic tables (the block a call reduces and its inverse, the
identities, the rates, the three replays' tables), the tiles dealt to the ranks with the one int64 reduction of a call, and the JSON
layout with the library stubbed (a plan whose error_study and channel_study record their arguments and return arrays of the
documented shapes).  Nothing here touches a GPU."""
import json

import numpy as np
import pytest

from ofdm_course_amd.drivers import error_anatomy as ea


def _tables(n, nd, ns, bps, gb, frames, rng):
    """Synthetic tables that satisfy the identities: `frames` frames per point, each with errors at random stream positions."""
    t = {k: np.zeros((n,) if k in ("errors", "frames_in_error", "gap_above") else
                     (n, dict(carrier_errors=nd, symbol_errors=ns, label_errors=bps, gap_hist=gb)[k]), np.int64) for k in ea.INT_KEYS}
    for p in range(n):
        for _ in range(frames):
            pos = np.flatnonzero(rng.random(nd * ns * bps) < 0.02 * (p + 1))
            if not pos.size:
                continue
            q, r = np.divmod(pos, bps)
            s, d = np.divmod(q, nd)
            t["errors"][p] += pos.size
            t["frames_in_error"][p] += 1
            np.add.at(t["carrier_errors"][p], d, 1)
            np.add.at(t["symbol_errors"][p], s, 1)
            np.add.at(t["label_errors"][p], r, 1)
            g = np.diff(pos)
            np.add.at(t["gap_hist"][p], g[g <= gb] - 1, 1)
            t["gap_above"][p] += int((g > gb).sum())
    return t


def test_settings_are_the_scripts():
    assert ea.T4_SNRS == (10.0, 20.0, 30.0) and ea.LABEL_CONSTELLATIONS == ("QPSK", "16QAM", "64QAM") and ea.GAP_BINS == 64
    assert np.array_equal(ea.CHANNEL_TAPS, [[0, 1.0], [4, 0.6], [10, 0.3]])                           # T4:252-256
    h = np.ones(3)
    off, on = ea.t4_args(h, False), ea.t4_args(h, True)
    assert (off["time_desync"], off["freq_desync"]) == (0, 0) and "Time_Delay" not in off and "Freq_Shift" not in off
    assert (on["time_desync"], on["freq_desync"], on["Time_Delay"], on["Freq_Shift"]) == (1, 1, "random", "random")
    for cite in ("T4:252-256", "T4:292-294", "DeScrambler.m:8-13", "T3:36", "estimate_channel.m:8"):
        assert cite in ea.__doc__, cite


def test_block_of_a_call_and_its_inverse_and_the_identities():
    rng = np.random.default_rng(1)
    t = _tables(3, 7, 4, 6, 16, 5, rng)
    w = ea.widths(7, 4, 6, 16)
    assert w == dict(errors=1, frames_in_error=1, carrier_errors=7, symbol_errors=4, label_errors=6, gap_hist=16, gap_above=1)
    block = ea.join_tables(t, 3)
    assert block.dtype == np.int64 and block.shape == (3, 36)
    back = ea.split_tables(block, w)
    assert all(np.array_equal(back[k], t[k]) and back[k].shape == t[k].shape for k in ea.INT_KEYS)
    assert ea.check_identities(back) is None
    one = ea.split_tables(ea.join_tables(_tables(2, 1, 1, 1, 1, 3, rng), 2), ea.widths(1, 1, 1, 1))   # width-1 tables stay 2-D
    assert one["carrier_errors"].shape == (2, 1) and one["gap_hist"].shape == (2, 1) and one["errors"].shape == (2,)
    for key, msg in (("carrier_errors", "sum(carrier_errors) differs from errors"), ("label_errors", "sum(label_errors) differs from errors"),
                     ("gap_hist", "sum(gap_hist) + gap_above differs from errors - frames_in_error")):
        broken = {k: v.copy() for k, v in back.items()}
        broken[key][1, 0] += 1
        assert ea.check_identities(broken) == msg
    with pytest.raises(ValueError, match="a block of 35 columns for tables of 36"):
        ea.split_tables(block[:, :-1], w)


def test_rates_and_the_three_tables():
    rng = np.random.default_rng(2)
    nd, ns, bps, frames = 5, 3, 4, 6
    t = _tables(2, nd, ns, bps, 64, frames, rng)
    r = ea.rates(t, frames, ns, bps)
    assert np.array_equal(r["BER"], t["errors"] / (frames * nd * ns * bps)) and np.array_equal(r["FER"], t["frames_in_error"] / frames)
    assert np.array_equal(r["carrier_BER"], t["carrier_errors"] / (frames * ns * bps))
    assert np.allclose(r["carrier_BER"].mean(axis=1), r["BER"])
    dc = np.array([2, 3, 5, 6, 8])
    curves = dict(nmse_profile=np.arange(16.0).reshape(2, 8), mean_true_amp=10.0 + np.arange(16.0).reshape(2, 8))
    ct = ea.carrier_table(t, frames, ns, bps, dc, curves)
    assert set(ct) == {"dataCarriers", "carrier_BER", "nmse_profile", "mean_true_amp", "symbol_errors", "BER", "FER"}
    assert np.array_equal(ct["nmse_profile"], [[1, 2, 4, 5, 7], [9, 10, 12, 13, 15]]) and ct["mean_true_amp"][0, 0] == 11.0
    assert ct["carrier_BER"].shape == ct["nmse_profile"].shape == (2, 5)
    lt = ea.label_table(t, frames, nd, ns)
    assert np.array_equal(lt["label_BER"], t["label_errors"] / (frames * nd * ns)) and np.allclose(lt["label_BER"].mean(axis=1), r["BER"])
    pay = {k: 3 * v for k, v in t.items()}
    pay["errors"] = pay["errors"].copy()
    pay["errors"][1], t["errors"][1] = 5, 0                                    # no channel error: the ratio of nothing
    dt = ea.descrambler_table(pay, t)
    assert dt["ratio_payload_over_channel"][0] == 3.0 and not np.isfinite(dt["ratio_payload_over_channel"][1])
    assert np.array_equal(dt["payload"]["gap_13"], pay["gap_hist"][:, 12]) and np.array_equal(dt["channel"]["gap_1"], t["gap_hist"][:, 0])
    assert set(dt["payload"]) == {"errors", "frames_in_error", "gap_hist", "gap_above", "gap_1", "gap_13", "gap_14"}


class _Plan:
    def __init__(self, lib, *args, **kw):
        self.lib, self.args, self.kw = lib, args, kw
        self.Nfft, self.N_symb, self.N_carrier, self.n_pilots, self.n_data = args[0], args[2], args[3], len(args[4]), len(args[5])
        self.dataCarriers = np.asarray(args[5], np.int32)
        self.bps = {"QPSK": 2, "16QAM": 4, "64QAM": 6}[args[9]]
        self.descr, self.closed = None, False

    def set_descrambler(self, reg):
        self.descr = None if reg is None else list(reg)

    def error_study(self, SNRs, frames_per_point, gap_bins, **kw):
        self.lib.calls.append(dict(kw, what="error", SNRs=SNRs, frames_per_point=frames_per_point, gap_bins=gap_bins, const=self.args[9],
                                   descr=self.descr))
        n, fpp = len(SNRs), frames_per_point
        mult = 3 if kw.get("side", "payload") == "payload" and kw.get("Register") is not None else 1
        z = lambda w: np.zeros((n, w), np.int64)
        car, sym, lab, gap = z(self.n_data), z(self.N_symb), z(self.bps), z(gap_bins)
        car[:, 0] = sym[:, 0] = lab[:, -1] = mult * fpp                         # `mult` errors in every frame, all in one place
        gap[:, 0] = gap[:, 12] = (fpp if mult == 3 else 0)
        return dict(errors=np.full(n, mult * fpp, np.int64), frames_in_error=np.full(n, fpp, np.int64), carrier_errors=car,
                    symbol_errors=sym, label_errors=lab, gap_hist=gap, gap_above=np.zeros(n, np.int64))

    def channel_study(self, SNRs, frames_per_point, bins, **kw):
        self.lib.calls.append(dict(kw, what="hest", SNRs=SNRs, frames_per_point=frames_per_point))
        n, nc, npil, fpp = len(SNRs), self.N_carrier, self.n_pilots, frames_per_point
        hist = np.zeros((n, bins["n"]), np.int64)
        return dict(est_amp_sums=np.full((n, nc), 2.0 * fpp), true_amp_sums=np.full((n, nc), 1.5 * fpp), err_sums=np.full((n, nc), 0.5 * fpp),
                    amp_err_sums=np.full((n, nc), 0.25 * fpp), dropped=np.zeros((n, nc), np.int64), pilot_amp_sums=np.full((n, npil), 3.0 * fpp),
                    pilot_err_sums=np.full((n, npil), 0.125 * fpp), pilot_dropped=np.zeros((n, npil), np.int64),
                    nmse_sums=np.full(n, 0.5 * fpp * nc), amp_nmse_sums=np.full(n, 0.25 * fpp * nc), nmse_hist=hist,
                    nmse_below=np.zeros(n, np.int64), nmse_above=np.zeros(n, np.int64), nmse_nan=np.zeros(n, np.int64),
                    status_counts=np.tile(np.array([fpp, 0, 0, 0], np.int64), (n, 1)))

    def close(self):
        self.closed = True


class _Lib:
    def __init__(self):
        self.calls, self.plans, self.inits = [], [], []

    def init(self, device):
        self.inits.append(device)

    @staticmethod
    def constellation_func(name):
        return np.array([3 + 3j, 1 - 1j]) / np.sqrt(10), {"QPSK": 2, "16QAM": 4, "64QAM": 6}[name]

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
    ea.main(["--json", str(out), "--frames", "7", "--seed", "3", "--frames-per-tile", "4"], lib=lib)
    res = json.loads(out.read_text())
    assert len(lib.plans) == 5 and all(p.closed for p in lib.plans) and lib.inits == [0]
    assert [p.args[9] for p in lib.plans] == ["16QAM", "QPSK", "16QAM", "64QAM", "16QAM"]
    assert lib.plans[0].args[:4] == (1024, 128, 5, 400) and lib.plans[0].kw == dict(precision="fp64", device=0)
    # two tiles (4 + 3 frames) per call: sync off / on with error_study then channel_study, three constellations, two sides
    assert [(c["frame0"], c["frames_per_point"]) for c in lib.calls] == [(0, 4), (4, 3)] * 9
    assert [c["what"] for c in lib.calls] == (["error"] * 2 + ["hest"] * 2) * 2 + ["error"] * 10
    errs = [c for c in lib.calls if c["what"] == "error"]
    for call in lib.calls:
        assert call["seed"] == 3 and call["device"] == "cuda:0" and call["max_frames_per_chunk"] == 0
    for call in errs:
        assert call["receiver"] == "task4" and call["gap_bins"] == 64
    t4 = errs[:4]
    assert [c["time_desync"] for c in t4] == [0, 0, 1, 1] and all(c["side"] == "channel" and c["mp_desync"] == 1 for c in t4)
    assert all(np.array_equal(np.nonzero(c["h"])[0], [0, 4, 10]) and c["descr"] == list(ea.c.REGISTER) for c in t4)
    assert all((c.get("Time_Delay") == "random") == bool(c["time_desync"]) for c in t4)
    labels = errs[4:10]
    assert [c["const"] for c in labels] == ["QPSK"] * 2 + ["16QAM"] * 2 + ["64QAM"] * 2
    assert all(c.get("h") is None and c.get("Register") is None and c["descr"] is None and (c["time_desync"], c["freq_desync"],
               c["mp_desync"]) == (0, 0, 0) and c["SNRs"] == [5.0, 10.0, 15.0, 20.0] for c in labels)
    assert [c["side"] for c in errs[10:]] == ["payload", "payload", "channel", "channel"]
    assert all(list(c["Register"]) == list(ea.c.REGISTER) and c["descr"] == list(ea.c.REGISTER) for c in errs[10:])
    assert res["frames"] == 7 and res["seed"] == 3 and res["n_gpus"] == 1 and res["frames_per_tile"] == 4 and res["tiles_this_rank"] == 2
    assert set(res) >= {"driver", "t4_carriers", "t3_labels", "t3_descrambler", "gap_bins", "dtype"}
    t4c = res["t4_carriers"]
    assert set(t4c) == {"SNR_dB", "sync_off", "sync_on"} and t4c["SNR_dB"] == [10.0, 20.0, 30.0]
    nd = lib.plans[0].n_data
    for mode in ("sync_off", "sync_on"):
        tab = t4c[mode]
        assert set(tab) == {"dataCarriers", "carrier_BER", "nmse_profile", "mean_true_amp", "symbol_errors", "BER", "FER"}
        assert np.asarray(tab["carrier_BER"]).shape == np.asarray(tab["nmse_profile"]).shape == (3, nd) and len(tab["dataCarriers"]) == nd
        assert tab["carrier_BER"][0][0] == 7 / (7 * 5 * 4) and tab["carrier_BER"][0][1] == 0.0 and tab["FER"] == [1.0] * 3
        assert tab["nmse_profile"][0][0] == 0.5 and tab["mean_true_amp"][2][nd - 1] == 1.5 and tab["symbol_errors"][0] == [7, 0, 0, 0, 0]
    lab = res["t3_labels"]
    assert set(lab) == {"SNR_dB", "QPSK", "16QAM", "64QAM"}
    assert [len(lab[k]["label_errors"][0]) for k in ("QPSK", "16QAM", "64QAM")] == [2, 4, 6] and lab["64QAM"]["label_errors"][3] == [0] * 5 + [7]
    d = res["t3_descrambler"]
    assert set(d) == {"SNR_dB", "ratio_payload_over_channel", "payload", "channel"} and d["ratio_payload_over_channel"] == [3.0, 3.0]
    assert d["payload"]["gap_1"] == [7, 7] and d["payload"]["gap_13"] == [7, 7] and d["channel"]["gap_13"] == [0, 0]
    assert len(d["payload"]["gap_hist"][0]) == 64


def test_tiles_and_the_one_int64_reduction():
    seen = []
    for rank in range(3):
        seen += ea.tiles(10, 4, rank, 3)
    assert sorted(seen) == [(0, 4), (4, 4), (8, 2)]
    calls = []

    def reduce(counts):
        calls.append((counts.dtype, counts.shape))
        return 2 * counts                                                # a second rank that saw the same

    lib = _Lib()
    plan = lib.RxPlan(1024, 128, 5, 400, list(range(1, 61)), list(range(61, 401)), None, 8, 1, "16QAM")
    t = ea.study_call(plan, [(0, 3), (3, 2)], 2, reduce, SNRs=[1.0, 2.0], receiver="task4")
    assert calls == [(np.dtype(np.int64), (2, 1 + 1 + 340 + 5 + 4 + 64 + 1))]      # one reduction for both tiles
    assert t["errors"].tolist() == [10, 10] and t["carrier_errors"][0, 0] == 10 and t["frames_in_error"].tolist() == [10, 10]
    assert [(c["frame0"], c["frames_per_point"]) for c in lib.calls] == [(0, 3), (3, 2)]
    with pytest.raises(RuntimeError, match="error_anatomy: sum"):
        ea.study_call(plan, [(0, 3)], 2, lambda counts: counts + 1, SNRs=[1.0, 2.0], receiver="task4")
    assert np.array_equal(ea.reduce_counts(np.arange(6, dtype=np.int64).reshape(2, 3)), np.arange(6).reshape(2, 3))   # one rank: a no-op


def test_argument_checks_and_command_line(capsys):
    a = ea.parse_args(["--json", "out.json", "--frames", "7"])
    assert (a.json, a.frames, a.seed, a.precision, a.device, a.frames_per_tile) == ("out.json", 7, 1, "fp64", None, 4096)
    with pytest.raises(SystemExit):
        ea.parse_args(["--frames", "0"])
    assert "--frames must be >= 1" in capsys.readouterr().err
    lib = _Lib()
    with pytest.raises(ValueError, match="--frames"):
        ea.run(frames=0, lib=lib)                                        # refused before the library is touched
    assert not lib.inits and not lib.plans
