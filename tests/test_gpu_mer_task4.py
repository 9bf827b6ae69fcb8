"""MER of the Task-4 receiver (ofdm_rx_chain_task4_ex, the MER variant of eq_demap_kernel) and of its one-call sweep
(ofdm_ber_sweep_task4_ex): the per-frame MER_func sums {sum |ideal|^2, sum |ideal - RX_IQ|^2} (T5/MER_func.m:3-25) against
the oracle replay of each frame's equalised RX_IQ (T4/Main_model_Task_4.m:278-340) and against the per-function path; the
other outputs bit-identical to the entries without MER; the sweep's per-point sums against the receiver's per-frame sums,
chunk invariance, the Task-3 trend, refusals and the drivers (the MER(SNR) study of T4:136-200, sweep_ber --mer)."""
import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_task4_batch import _frames

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG = (1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0)          # T3/Main_model_Task_3.m:46


def _plan(ofdm, d, cfg_kw, precision):
    N, nc, S = cfg_kw["Nfft"], cfg_kw["N_carrier"], cfg_kw["N_symb"]
    return ofdm.RxPlan(N, d["Tg"], S, nc, d["pil"], d["dat"], d["col"], int(np.ceil(nc / 6)), 3, cfg_kw["const"],
                       precision=precision)


def _oracle_rx_iq(oracle, y, d, cfg_kw, flags):
    """The oracle replay of T4/Main_model_Task_4.m:278-341 for one frame -> RX_IQ = get_payload(.)(:).  A frame for which
    remove_IFO finds no line (the script's index error, status -1) is decoded with IFO = 0, as the batch decodes it."""
    import warnings
    N, nc, S = cfg_kw["Nfft"], cfg_kw["N_carrier"], cfg_kw["N_symb"]
    Tg = d["Tg"]
    td, fd, mp = flags
    y = np.asarray(y, dtype=np.complex128)
    if td or fd:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _, pos, fo, _ = oracle.AutoCorrFunction(y, Tg, N)
        if td:
            y = oracle.add_STO(oracle.add_STO(y, pos), -(N + Tg))
        if fd:
            y = oracle.add_CFO(y, -fo, N)
            try:
                y, _ = oracle.remove_IFO(y, N)
            except IndexError:
                pass
    X = oracle.OFDM_demodulator(y.reshape((N + Tg, S), order="F"), Tg)
    if td or fd:
        X = oracle.fine_sync(X, d["pil"], d["pv"], td, fd, variant="T4")
        X = X[0] if isinstance(X, tuple) else X
    if mp:
        H, _ = oracle.estimate_channel(X, d["allc"], d["pil"], d["pv"])
        X = oracle.equalize_signal(X, H, nc)
    return oracle.get_payload(X, d["dat"]).ravel(order="F")


def _oracle_sums(oracle, iq, const):
    """sum1, sum2 of MER_func.m:19-23 with the nearest-point rule of oracle.MER_func."""
    D, _ = oracle.constellation_func(const)
    ideal = D[np.argmin(np.abs(iq[None, :] - D[:, None]), axis=0)]
    return np.sum(ideal.real ** 2 + ideal.imag ** 2), np.sum((ideal - iq).real ** 2 + (ideal - iq).imag ** 2)


GEOMS = {"n1024": dict(Nfft=1024, N_carrier=400, N_symb=10, const="16QAM"),         # fp32: the VEC (carrier pair) path
         "n512": dict(Nfft=512, N_carrier=201, N_symb=8, const="QPSK")}             # odd N_carrier: the scalar path


@pytest.mark.parametrize("flags", [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)])
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_mer_sums_equal_the_oracle_replay(ofdm, oracle, geom, precision, flags):
    cfg_kw = GEOMS[geom]
    nfr = 5
    d = _frames(ofdm, cfg_kw, nfr, precision, seed=21)
    d["rx"][:, 3] *= 1e-3                                  # no spectral line reaches 0.77: status -1 with freq_desync
    plan = _plan(ofdm, d, cfg_kw, precision)
    N, Tg = cfg_kw["Nfft"], d["Tg"]
    n_iq = len(d["dat"]) * cfg_kw["N_symb"]
    iqs = [_oracle_rx_iq(oracle, d["rx"][:, f], d, cfg_kw, flags) for f in range(nfr)]
    saw_status_m1 = False
    for skip in (0, N + Tg):
        out = ofdm.rx_chain_task4(plan, d["rx"], *flags, want_mer=True, mer_skip=skip)
        got = np.asarray(out["mer_sums"])
        assert got.shape == (nfr, 2)
        st = np.asarray(out["status"])
        saw_status_m1 |= bool((st == -1).any())
        for f in range(nfr):
            iq = iqs[f][skip:]
            if not np.all(np.isfinite(iq)):              # the blanked first symbol can make estimate_channel NaN
                assert np.isnan(got[f, 1]), (f, got[f])
                continue
            w1, w2 = _oracle_sums(oracle, iq, cfg_kw["const"])
            if precision == "fp64":
                assert abs(got[f, 0] - w1) <= 1e-9 * w1 and abs(got[f, 1] - w2) <= 1e-9 * w2, (skip, f, got[f], w1, w2)
            else:
                n = n_iq - skip
                assert abs(got[f, 0] - w1) <= 1e-4 * w1 + 1e-6 * n, (skip, f, got[f, 0], w1)
                assert abs(got[f, 1] - w2) <= 1e-4 * w2 + 1e-6 * n, (skip, f, got[f, 1], w2)
        np.testing.assert_array_equal(np.asarray(out["MER_dB"]), 10 * np.log10(got[:, 0] / got[:, 1]))
    if flags[1]:
        assert saw_status_m1
    plan.close()


@pytest.mark.parametrize("const", ["16QAM", "64QAM", "8PSK"])
def test_mer_equals_the_per_function_path(ofdm, const):
    """flags (0,0,0), no channel: 10 log10(s1 / s2) == MER_func(get_payload(OFDM_demodulator(rx))) of the library, per frame."""
    from ofdm_course_amd.drivers import common as dc
    N, nc, S = 1024, 400, 5
    _, pil, dat = dc.layout_percent(N, nc, 15, tail=2)
    dct, _ = ofdm.constellation_func(const)
    col = dc.alternating_pilots(4 / 3 * float(np.max(np.abs(dct))), len(pil), 1)[:, 0]
    plan = ofdm.RxPlan(N, N // 8, S, nc, pil, dat, col, len(pil), 3, const, precision="fp64")
    gen = plan.tx_frames_fused(6, SNR=18.0, seed=9, frame0=4)
    rx = np.asarray(gen["rx"])
    for skip in (0, N + N // 8):
        out = ofdm.rx_chain_task4(plan, rx, 0, 0, 0, want_mer=True, mer_skip=skip)
        for f in range(rx.shape[1]):
            X = ofdm.OFDM_demodulator(rx[:, f].reshape((N + N // 8, S), order="F"), N // 8)
            iq = np.ascontiguousarray(np.asarray(ofdm.get_payload(X, dat)).ravel(order="F")[skip:])
            want = ofdm.MER_func(iq, const)
            assert abs(float(out["MER_dB"][f]) - want) <= 1e-9, (skip, f, float(out["MER_dB"][f]), want)
    plan.close()


def _mid(ofdm, precision, device=None):
    from ofdm_course_amd import frames as fr
    cfg = fr.config_small(nfft=512, n_carrier=200, comb=5, const="16QAM", n_symb=6, dominant_taps=3)
    return cfg, fr.make_plan(cfg, ofdm, precision=precision, device=device)


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_mer_changes_no_other_output(ofdm, oracle, precision):
    """rx_chain_task4_ex with MER on == rx_chain_task4, every output bit for bit (with the DeScrambler as well);
    ber_sweep_task4_ex == ber_sweep_task4 on errors, status counts, cfo_abs_err and frame errors."""
    cfg, plan = _mid(ofdm, precision)
    h, _ = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    for reg in (None, REG):
        plan.set_descrambler(reg)
        gen = plan.tx_frames_fused(12, h=h, SNR=15.0, seed=4, frame0=3, Register=reg, Time_Delay="random",
                                   Freq_Shift="random")
        for flags in [(1, 1, 1), (1, 0, 0), (0, 0, 0)]:
            a = ofdm.rx_chain_task4(plan, gen["rx"], *flags, ref_bits_packed=gen["packed"], want_h=True)
            b = ofdm.rx_chain_task4(plan, gen["rx"], *flags, ref_bits_packed=gen["packed"], want_h=True, want_mer=True,
                                    mer_skip=cfg.Nfft + cfg.T_guard)
            for k in ("bits", "errors", "TgPosition", "FreqOffset", "IFO", "status", "H"):
                assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (reg is None, flags, k)
        kw = dict(h=h, Time_Delay="random", Freq_Shift="random", seeds=[5, 6], frame0=2, Register=reg,
                  want_frame_errors=True)
        a = plan.ber_sweep_task4([8.0, 20.0], 10, **kw)
        b = plan.ber_sweep_task4([8.0, 20.0], 10, want_mer=True, mer_skip=7, want_frame_mer=True, **kw)
        for k in ("errors", "status_counts", "cfo_abs_err", "frame_errors"):
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (reg is None, k)
        assert a["bits"] == b["bits"]
    plan.close()


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_sweep_mer_equals_the_receiver_and_is_chunk_invariant(ofdm, oracle, precision):
    import torch
    cfg, plan = _mid(ofdm, precision, device=0)
    h, _ = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    snrs, seeds, fpp, f0, skip = [5.0, 15.0, 30.0], [11, 12, 13], 20, 40, cfg.Nfft + cfg.T_guard
    kw = dict(h=h, Time_Delay="random", Freq_Shift="random", seeds=seeds, frame0=f0, want_mer=True, mer_skip=skip,
              want_frame_mer=True)
    base = plan.ber_sweep_task4(snrs, fpp, **kw)
    ms, fm = np.asarray(base["mer_sums"]), np.asarray(base["frame_mer_sums"])
    assert ms.shape == (3, 2) and fm.shape == (3, fpp, 2)
    for p in range(3):
        gen = plan.tx_frames_fused(fpp, h=h, SNR=snrs[p], seed=seeds[p], frame0=f0, Time_Delay="random",
                                   Freq_Shift="random")
        out = ofdm.rx_chain_task4(plan, gen["rx"], 1, 1, 1, want_mer=True, mer_skip=skip)
        per = np.asarray(out["mer_sums"])
        assert per.tobytes() == fm[p].tobytes(), p                       # the per-frame sums, bit for bit
        want = per.sum(axis=0)                                          # NaN where a frame's equaliser is NaN, as MER_func
        assert np.array_equal(np.isnan(ms[p]), np.isnan(want)), (p, ms[p], want)
        ok = ~np.isnan(want)
        assert np.all(np.abs(ms[p][ok] - want[ok]) <= 1e-12 * np.abs(want[ok])), (p, ms[p], want)
    for ch in (1, 7, 0):
        other = plan.ber_sweep_task4(snrs, fpp, max_frames_per_chunk=ch, **kw)
        assert np.asarray(other["mer_sums"]).tobytes() == ms.tobytes(), ch
        assert np.asarray(other["frame_mer_sums"]).tobytes() == fm.tobytes(), ch
        assert np.array_equal(np.asarray(other["errors"]), np.asarray(base["errors"])), ch
    dev = plan.ber_sweep_task4(snrs, fpp, device="cuda:0", **kw)
    assert isinstance(dev["mer_sums"], torch.Tensor) and dev["mer_sums"].is_cuda and dev["MER_dB"].is_cuda
    assert dev["mer_sums"].cpu().numpy().tobytes() == ms.tobytes()
    assert dev["frame_mer_sums"].cpu().numpy().tobytes() == fm.tobytes()
    assert np.allclose(dev["MER_dB"].cpu().numpy(), np.asarray(base["MER_dB"]), rtol=0, atol=1e-12, equal_nan=True)
    plan.close()


def test_sweep_task3_mode_mer_rises_with_snr(ofdm):
    """T3/Main_model_Task_3.m:237-268 with the MER of :186: 16QAM, flags (0,0,0), Scrambler + DeScrambler; MER(SNR) on 0:5:30
    dB rises strictly."""
    from ofdm_course_amd.drivers import common as dc
    _, pil, dat = dc.layout_percent(1024, 400, 15, tail=2)
    d, _ = ofdm.constellation_func("16QAM")
    amp = 4 / 3 * float(np.max(np.abs(d)))
    plan = ofdm.RxPlan(1024, 128, 5, 400, pil, dat, np.full(len(pil), amp, dtype=np.complex128), len(pil), 3, "16QAM",
                       precision="fp32", device=0)
    plan.set_descrambler(REG)
    snrs = np.arange(0.0, 31.0, 5.0)
    res = plan.ber_sweep_task4(snrs, 16, seed=31, Register=REG, want_mer=True)
    mer = np.asarray(res["MER_dB"])
    assert np.all(np.isfinite(mer)) and np.all(np.diff(mer) > 0), mer
    assert abs(mer[-1] - snrs[-1]) < 3.0, mer                     # the noise is set on the signal with its CP
    plan.close()


def test_mer_refusals(ofdm, oracle):
    from ofdm_course_amd import _lib as L
    cfg, plan = _mid(ofdm, "fp32")
    n_iq = len(cfg.dataCarriers) * cfg.N_symb
    gen = plan.tx_frames_fused(2, SNR=20.0, seed=1)
    for bad in (-1, n_iq, n_iq + 5):
        with pytest.raises(ofdm.OfdmError):
            ofdm.rx_chain_task4(plan, gen["rx"], 1, 1, 1, want_mer=True, mer_skip=bad)
        with pytest.raises(ofdm.OfdmError):
            plan.ber_sweep_task4([20.0], 4, want_mer=True, mer_skip=bad)
    ofdm.rx_chain_task4(plan, gen["rx"], 1, 1, 1, want_mer=True, mer_skip=n_iq - 1)       # the last index is allowed
    # at the C ABI, with and without the MER outputs
    rx = np.ascontiguousarray(np.asarray(gen["rx"]))
    ms = np.zeros(4, dtype=np.float64)
    snr, seeds, err = np.array([20.0]), np.array([1], dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def rxc(skip, out):
        return plan.lib.ofdm_rx_chain_task4_ex(plan.handle, p(rx), 2, 1, 1, 1, None, None, None, None, None, None, None,
                                               None, skip, out, L.OFDM_F32)

    def sweep(skip, out):
        return plan.lib.ofdm_ber_sweep_task4_ex(plan.handle, None, 0, 0, 0, 0, 0.0, 0, 0, 0, p(snr), p(seeds), 1, 4, 0, None,
                                                0, p(err), None, None, None, skip, out, None, L.OFDM_F32)
    for out in (p(ms), None):
        assert rxc(-1, out) != 0 and rxc(n_iq, out) != 0 and rxc(0, out) == 0
        assert sweep(-1, out) != 0 and sweep(n_iq, out) != 0 and sweep(0, out) == 0
    plan.close()


def test_task4_mer_driver_equals_direct_calls(ofdm):
    """drivers/task4_mer.py (T4/Main_model_Task_4.m:136-200) on a short grid == ber_sweep_task4 called directly."""
    from ofdm_course_amd.drivers import common as dc
    from ofdm_course_amd.drivers import task4_mer
    snrs = [0.0, 10.0, 25.0]
    r = task4_mer.run(ofdm, SNRs=snrs, frames_per_point=3, seed=5)
    N, nc, S = 1024, 400, 50
    _, pil, dat = dc.layout_percent(N, nc, 15, tail=2)
    d, _ = ofdm.constellation_func("16QAM")
    col = dc.alternating_pilots(4 / 3 * np.max(np.abs(d)), len(pil), 1)[:, 0]
    plan = ofdm.RxPlan(N, N // 8, S, nc, pil, dat, col, len(pil), 3, "16QAM", precision="fp64")
    want = plan.ber_sweep_task4(snrs, 3, Time_Delay=12, time_desync=1, freq_desync=0, mp_desync=0, seed=5, want_mer=True,
                                mer_skip=N + N // 8)
    assert np.asarray(r["mer_sums"]).tobytes() == np.asarray(want["mer_sums"]).tobytes()
    assert np.array_equal(r["MER_dB"], np.asarray(want["MER_dB"]))
    assert np.array_equal(r["MER_minus_SNR"], np.abs(np.asarray(want["MER_dB"]) - np.asarray(snrs)))
    assert np.all(np.diff(r["MER_dB"]) > 0)
    plan.close()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(cmd, out):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(out) as f:
        return json.load(f)


def test_sweep_driver_c3_mer(ofdm, tmp_path):
    """sweep_ber --config C3 --mer: two gloo ranks on one GPU give the per-point MER of a single direct call per tile;
    without --mer the output has no MER keys and the same counters."""
    from ofdm_course_amd import frames as fr
    from ofdm_course_amd import sweep
    snrs, batches, fpt, seed = [12.0, 24.0], 2, 4, 7
    common = ["--config", "C3", "--batches", str(batches), "--frames-per-tile", str(fpt), "--snrs", *map(str, snrs)]
    dist = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
            "127.0.0.1", "--master-port", str(_free_port()), "-m", "ofdm_course_amd.drivers.sweep_ber", *common,
            "--backend", "gloo", "--force-device", "0"]
    two = _run([*dist, "--mer", "--json", str(tmp_path / "two.json")], tmp_path / "two.json")
    assert two["n_gpus"] == 2
    cfg = fr.config_C3()
    plan = fr.make_plan(cfg, ofdm, precision="fp32")
    h, _ = ofdm.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    s = np.zeros((len(snrs), 2))
    err = np.zeros(len(snrs), dtype=np.int64)
    for si, bi in sweep.tiles_for_rank(len(snrs), batches, 0, 1):
        key, stream0 = sweep.tile_seed_stream(seed, si, bi, fpt)
        r = plan.ber_sweep_task4([snrs[si]], fpt, h=h, Time_Delay="random", Freq_Shift="random", seeds=[key], frame0=stream0,
                                 want_mer=True, mer_skip=cfg.Nfft + cfg.T_guard)
        s[si] += np.asarray(r["mer_sums"])[0]
        err[si] += r["errors"][0]
    assert two["errors"] == err.tolist()
    assert np.allclose(np.asarray(two["mer_sums"]), s, rtol=1e-12, atol=0, equal_nan=True)
    assert np.allclose(two["MER_dB"], 10 * np.log10(s[:, 0] / s[:, 1]), rtol=1e-12, atol=0, equal_nan=True)
    off = _run([*dist, "--json", str(tmp_path / "off.json")], tmp_path / "off.json")
    assert "MER_dB" not in off and "mer_sums" not in off
    assert off["errors"] == two["errors"] and off["status_counts"] == two["status_counts"]
    assert off["cfo_abs_err"] == two["cfo_abs_err"]
    plan.close()
