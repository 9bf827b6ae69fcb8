"""ofdm_tx_frames_fused_ex (the three-pass generator with the Task-4 impairments, Noise -> add_STO -> add_CFO -> conv) and
ofdm_ber_sweep_task4 (one device-resident BER(SNR) tile of the Task-4 receiver): the generator against the oracle's
composition (oracle.tx_frame(noise_first=True, Time_Delay=, Freq_Shift=) on the Philox draws) and against
ofdm_tx_frames_ex(noise_first=1); the sweep's counts against rx_chain_task4 on the generator's frames, call by call."""
import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REG = (1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0)          # T3/Main_model_Task_3.m:46, T5/Main_model_Task_5.m:55
STATUS = (0, 1, -1, -2)

# (Time_Delay, Freq_Shift): drawn; a negative STO (the delay branch of add_STO.m); an STO beyond the largest channel delay
# (25 for M, 7 for small) without CFO; a CFO with STO 0
IMPAIRMENTS = [("random", "random"), (-37, 3.3), (40, None), (0, 2.7)]


def _cfg(name):
    from ofdm_course_amd import frames as fr
    if name == "M":
        return fr.config_M()
    if name == "small":
        return fr.config_small()
    return fr.config_small(nfft=512, n_carrier=200, comb=5, const="16QAM", n_symb=6, dominant_taps=3)


@pytest.mark.parametrize("imp", IMPAIRMENTS, ids=["random", "sto-neg", "sto-long", "cfo-only"])
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("name", ["small", "M"])
def test_fused_ex_generator_equals_the_oracle_composition(ofdm, oracle, name, precision, imp):
    from ofdm_course_amd import frames as fr
    cfg = _cfg(name)
    plan = fr.make_plan(cfg, ofdm, precision=precision)
    sto, cfo = imp
    nfr, seed, f0 = (4 if name == "M" else 5), 0x51D0C0FE3, 11
    h, _ = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    kw = dict(h=h, SNR=cfg.SNR_dB, seed=seed, Time_Delay=sto, Freq_Shift=cfo)
    gen = plan.tx_frames_fused(nfr, frame0=f0, want_draws=True, **kw)
    ex = plan.tx_frames(nfr, frame0=f0, noise_first=True, want_draws=True, **kw)
    # the per-frame draws are ofdm_tx_frames_ex's, exactly
    assert np.array_equal(np.asarray(gen["Time_Delay"]), np.asarray(ex["Time_Delay"]))
    assert np.array_equal(np.asarray(gen["Freq_Shift"]), np.asarray(ex["Freq_Shift"]))
    _, bps = oracle.constellation_func(cfg.Constellation)
    nd = len(cfg.dataCarriers)
    pv = np.repeat(fr.pilot_column(cfg, ofdm)[:, None], cfg.N_symb, axis=1)
    rx = np.asarray(gen["rx"])
    span = cfg.Nfft + cfg.T_guard + 1
    for f in range(nfr):
        d_sto, d_cfo = oracle.sto_cfo_draw_philox(span, seed, f0 + f)
        want_sto = d_sto if sto == "random" else (0 if sto is None else sto)
        want_cfo = d_cfo if cfo == "random" else (0.0 if cfo is None else cfo)
        assert int(np.asarray(gen["Time_Delay"])[f]) == want_sto
        assert float(np.asarray(gen["Freq_Shift"])[f]) == want_cfo
        bits = oracle.payload_bits_philox(nd * cfg.N_symb, bps, seed, f0 + f)
        assert np.array_equal(np.asarray(gen["packed"])[f], fr.pack_bits(bits[None, :])[0])      # bit-exact
        noise = oracle.awgn_philox(cfg.frame_samples, seed, f0 + f)
        want, _ = oracle.tx_frame(bits, cfg.Nfft, cfg.T_guard, cfg.N_symb, cfg.dataCarriers, cfg.pilotCarriers, pv,
                                  cfg.Constellation, h=h, SNR=cfg.SNR_dB, noise=noise, noise_first=True,
                                  Time_Delay=None if sto is None else want_sto,
                                  Freq_Shift=None if cfo is None else want_cfo)
        assert rel_l2(rx[:, f], want) < (1e-13 if precision == "fp64" else 2e-6), f
    if precision == "fp64":                              # the staged generator in the same order: rounding apart, equal
        assert np.array_equal(np.asarray(ex["packed"]), np.asarray(gen["packed"]))
        for f in range(nfr):
            assert rel_l2(rx[:, f], np.asarray(ex["rx"])[:, f]) < 1e-13
    # batching independence: frames 1..2 generated alone are the same arrays, bit for bit
    sub = plan.tx_frames_fused(2, frame0=f0 + 1, want_draws=True, **kw)
    assert np.array_equal(np.asarray(sub["rx"]), rx[:, 1:3])
    assert np.array_equal(np.asarray(sub["packed"]), np.asarray(gen["packed"])[1:3])
    assert np.array_equal(np.asarray(sub["Freq_Shift"]), np.asarray(gen["Freq_Shift"])[1:3])


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("name", ["small", "M"])
def test_fused_without_impairments_is_the_unchanged_path(ofdm, oracle, name, precision):
    """tx_frames_fused without the new keywords (ofdm_tx_frames_fused) == the _ex entry with both modes 0, bit for bit,
    with and without the Scrambler; the device flavour returns the host flavour's arrays."""
    import torch
    from ofdm_course_amd import frames as fr
    cfg = _cfg(name)
    plan = fr.make_plan(cfg, ofdm, precision=precision, device=0)
    h, _ = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    for reg in (None, REG):
        old = plan.tx_frames_fused(3, h=h, SNR=15.0, seed=5, frame0=2, Register=reg)
        new = plan.tx_frames_fused(3, h=h, SNR=15.0, seed=5, frame0=2, Register=reg, want_draws=True)   # modes 0
        assert np.array_equal(np.asarray(new["rx"]), np.asarray(old["rx"]))
        assert np.array_equal(np.asarray(new["packed"]), np.asarray(old["packed"]))
        if reg is not None:
            assert np.array_equal(np.asarray(new["sc_packed"]), np.asarray(old["sc_packed"]))
        assert not np.asarray(new["Time_Delay"]).any() and not np.asarray(new["Freq_Shift"]).any()
    host = plan.tx_frames_fused(3, h=h, SNR=15.0, seed=5, frame0=2, Time_Delay="random", Freq_Shift="random",
                                want_draws=True)
    dev = plan.tx_frames_fused(3, h=h, SNR=15.0, seed=5, frame0=2, Time_Delay="random", Freq_Shift="random",
                               want_draws=True, device="cuda:0")
    torch.cuda.synchronize()
    assert np.array_equal(dev["rx"].cpu().numpy(), np.asarray(host["rx"]))
    assert np.array_equal(dev["Time_Delay"].cpu().numpy(), np.asarray(host["Time_Delay"]))


def _composed(ofdm, plan, gen, flags):
    """rx_chain_task4 on a generator call's frames -> (frame errors, status counts, sum |FreqOffset + IFO - Freq_Shift|)."""
    out = ofdm.rx_chain_task4(plan, gen["rx"], *flags, ref_bits_packed=gen["packed"])
    fe = np.asarray(out["errors"]).astype(np.int64)
    st = np.asarray(out["status"])
    counts = np.array([(st == s).sum() for s in STATUS], dtype=np.int64)
    err = np.abs(np.asarray(out["FreqOffset"]) + np.asarray(out["IFO"]).astype(np.float64) - np.asarray(gen["Freq_Shift"]))
    return fe, counts, float(err.sum()) if flags[1] else 0.0


def _check_sweep_equals_composed(ofdm, plan, res, snrs, seeds, fpp, f0, h, imp, flags, reg=None):
    fe = np.asarray(res["frame_errors"]).astype(np.int64)
    assert res["bits"] == fpp * plan.frame_bits
    assert np.array_equal(np.asarray(res["errors"]), fe.sum(axis=1))
    for p, (snr, sd) in enumerate(zip(snrs, seeds)):
        gen = plan.tx_frames_fused(fpp, h=h, SNR=snr, seed=sd, frame0=f0, Register=reg, want_draws=True,
                                   Time_Delay=imp[0], Freq_Shift=imp[1])
        want_fe, want_counts, want_cfo = _composed(ofdm, plan, gen, flags)
        assert np.array_equal(fe[p], want_fe), p
        assert np.array_equal(np.asarray(res["status_counts"])[p], want_counts), p
        got_cfo = float(np.asarray(res["cfo_abs_err"])[p])
        if flags[1]:
            assert np.isfinite(got_cfo) and abs(got_cfo - want_cfo) <= 1e-12 * max(abs(want_cfo), 1e-300), (got_cfo, want_cfo)
        else:
            assert got_cfo == 0.0


@pytest.mark.parametrize("flags", [(1, 1, 1), (1, 1, 0)])
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_sweep_task4_equals_the_composed_path(ofdm, oracle, precision, flags):
    from ofdm_course_amd import frames as fr
    cfg = _cfg("mid")
    plan = fr.make_plan(cfg, ofdm, precision=precision)
    h, _ = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    imp = ("random", "random")
    snrs, seeds, fpp, f0 = [5.0, 15.0, 30.0], [11, 12, 13], 24, 40
    res = plan.ber_sweep_task4(snrs, fpp, h=h, Time_Delay=imp[0], Freq_Shift=imp[1], time_desync=flags[0],
                               freq_desync=flags[1], mp_desync=flags[2], seeds=seeds, frame0=f0, want_frame_errors=True)
    _check_sweep_equals_composed(ofdm, plan, res, snrs, seeds, fpp, f0, h, imp, flags)
    assert int(np.asarray(res["status_counts"]).sum()) == len(snrs) * fpp


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_sweep_task4_scrambler_and_metric_geometry(ofdm, oracle, precision):
    """Scrambler + DeScrambler (errors against the payload) on the small geometry; flags (1,1,1) at config M."""
    from ofdm_course_amd import frames as fr
    cfg = _cfg("small")
    plan = fr.make_plan(cfg, ofdm, precision=precision)
    h, _ = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    imp, flags = (25, 4.2), (1, 1, 1)
    plan.set_descrambler(REG)
    res = plan.ber_sweep_task4([10.0, 25.0], 16, h=h, Time_Delay=imp[0], Freq_Shift=imp[1], seeds=[3, 4], frame0=5,
                               Register=REG, want_frame_errors=True)
    _check_sweep_equals_composed(ofdm, plan, res, [10.0, 25.0], [3, 4], 16, 5, h, imp, flags, reg=REG)
    cfg = _cfg("M")
    plan = fr.make_plan(cfg, ofdm, precision=precision)
    h, _ = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    imp = ("random", "random")
    res = plan.ber_sweep_task4([20.0], 12, h=h, Time_Delay="random", Freq_Shift="random", seed=8, frame0=3,
                               want_frame_errors=True)
    _check_sweep_equals_composed(ofdm, plan, res, [20.0], [8], 12, 3, h, imp, flags)


def test_sweep_task4_chunk_invariance(ofdm, oracle):
    """max_frames_per_chunk 1, 7 and the default give bitwise equal outputs, the double CFO sum included; the device
    flavour equals the host flavour."""
    import torch
    from ofdm_course_amd import frames as fr
    cfg = _cfg("mid")
    plan = fr.make_plan(cfg, ofdm, precision="fp32", device=0)
    h, _ = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    kw = dict(h=h, Time_Delay="random", Freq_Shift="random", seeds=[21, 22], frame0=17, want_frame_errors=True)
    snrs, fpp = [8.0, 20.0], 20
    base = plan.ber_sweep_task4(snrs, fpp, **kw)
    for ch in (1, 7):
        other = plan.ber_sweep_task4(snrs, fpp, max_frames_per_chunk=ch, **kw)
        for k in ("errors", "status_counts", "frame_errors"):
            assert np.array_equal(np.asarray(other[k]), np.asarray(base[k])), (ch, k)
        assert np.asarray(other["cfo_abs_err"]).tobytes() == np.asarray(base["cfo_abs_err"]).tobytes(), ch
    dev = plan.ber_sweep_task4(snrs, fpp, device="cuda:0", **kw)
    assert isinstance(dev["errors"], torch.Tensor) and dev["errors"].is_cuda
    assert np.array_equal(dev["errors"].cpu().numpy(), base["errors"])
    assert np.array_equal(dev["status_counts"].cpu().numpy(), base["status_counts"])
    assert dev["cfo_abs_err"].cpu().numpy().tobytes() == np.asarray(base["cfo_abs_err"]).tobytes()


@pytest.mark.parametrize("const", ["BPSK", "QPSK", "8PSK", "16QAM"])
def test_sweep_task4_task3_mode(ofdm, const):
    """T3/Main_model_Task_3.m:237-268: no STO / CFO / channel, flags (0,0,0), Scrambler + per-frame DeScrambler, on the
    Task-3 geometry (Nfft 1024, 400 carriers, 15 % pilots at 4/3 max|dict|, frames of 5 symbols)."""
    from ofdm_course_amd.drivers import common as dc
    _, pil, dat = dc.layout_percent(1024, 400, 15, tail=2)
    d, _ = ofdm.constellation_func(const)
    amp = 4 / 3 * float(np.max(np.abs(d)))
    plan = ofdm.RxPlan(1024, 128, 5, 400, pil, dat, np.full(len(pil), amp, dtype=np.complex128), len(pil), 3, const,
                       precision="fp32", device=0)
    plan.set_descrambler(REG)
    snrs, fpp = [0.0, 10.0, 20.0, 30.0], 32
    res = plan.ber_sweep_task4(snrs, fpp, seed=31, frame0=0, Register=REG, want_frame_errors=True)
    assert not np.asarray(res["cfo_abs_err"]).any()
    assert np.array_equal(np.asarray(res["status_counts"])[:, 0], [fpp] * 4)
    for p, snr in enumerate(snrs):
        gen = plan.tx_frames_fused(fpp, SNR=snr, seed=31, frame0=0, Register=REG, want_draws=True)
        fe, counts, _ = _composed(ofdm, plan, gen, (0, 0, 0))
        assert np.array_equal(np.asarray(res["frame_errors"])[p].astype(np.int64), fe)
        assert np.array_equal(np.asarray(res["status_counts"])[p], counts)
    ber = np.asarray(res["errors"]) / res["bits"]
    if const in ("BPSK", "QPSK"):
        assert ber[3] == 0.0, ber
    if const == "16QAM":                                 # strictly falling until it reaches zero
        assert ber[0] > ber[1] > 0.0, ber
        for a, b in zip(ber[1:], ber[2:]):
            assert a > b or a == b == 0.0, ber


def test_sweep_task4_c3_tile(ofdm):
    """config_C3 (the Task-4 benchmark geometry), fp32, 2 points x 256 frames, random STO / CFO, all desync stages on."""
    import torch
    from ofdm_course_amd import frames as fr
    cfg = fr.config_C3()
    plan = fr.make_plan(cfg, ofdm, precision="fp32", device=0)
    h, _ = ofdm.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    dev = torch.device("cuda:0")
    snrs, seeds, F = [20.0, 30.0], [5, 6], 256
    res = plan.ber_sweep_task4(snrs, F, h=h, Time_Delay="random", Freq_Shift="random", seeds=seeds, device=dev,
                               want_frame_errors=True)
    for p in range(2):
        gen = plan.tx_frames_fused(F, h=h, SNR=snrs[p], seed=seeds[p], device=dev, Time_Delay="random",
                                   Freq_Shift="random", want_draws=True)
        out = ofdm.rx_chain_task4(plan, gen["rx"], 1, 1, 1, ref_bits_packed=gen["packed"])
        assert torch.equal(res["frame_errors"][p], out["errors"])
        counts = [int((out["status"] == s).sum().item()) for s in STATUS]
        assert res["status_counts"][p].cpu().tolist() == counts
        want = (out["FreqOffset"] + out["IFO"].to(torch.float64) - gen["Freq_Shift"]).abs().sum().item()
        got = float(res["cfo_abs_err"][p].item())
        assert np.isfinite(got) and abs(got - want) <= 1e-12 * abs(want)


def test_sweep_task4_refusals(ofdm, oracle):
    from ofdm_course_amd import _lib as L
    from ofdm_course_amd import frames as fr
    cfg = _cfg("small")
    plan = fr.make_plan(cfg, ofdm, precision="fp32")
    h, _ = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    with pytest.raises(ofdm.OfdmError):                  # scrambled frames, plan without a DeScrambler
        plan.ber_sweep_task4([20.0], 4, h=h, Register=REG)
    plan.set_descrambler(REG)
    with pytest.raises(ofdm.OfdmError):                  # a descrambling plan, unscrambled frames
        plan.ber_sweep_task4([20.0], 4, h=h)
    plan.set_descrambler(None)
    with pytest.raises(ofdm.OfdmError):                  # a chunk beyond rx_chain_task4's 65535 frames
        plan.ber_sweep_task4([20.0], 4, h=h, max_frames_per_chunk=65536)
    with pytest.raises(ofdm.OfdmError):
        plan.tx_frames_fused(2, h=h, Time_Delay="sometimes")
    # bad modes and a precision flag that differs from the plan's, at the C ABI
    snr = np.array([20.0])
    seeds = np.array([1], dtype=np.uint64)
    err = np.zeros(1, dtype=np.uint64)
    rx = np.zeros(2 * cfg.frame_samples, dtype=np.complex64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def sweep(sto_mode, cfo_mode, flags):
        return plan.lib.ofdm_ber_sweep_task4(plan.handle, None, 0, sto_mode, 0, cfo_mode, 0.0, 1, 1, 0, p(snr), p(seeds), 1,
                                             4, 0, None, 0, p(err), None, None, None, flags)

    def gen(sto_mode, cfo_mode, flags):
        return plan.lib.ofdm_tx_frames_fused_ex(plan.handle, None, 0, 20.0, 1, 0, 2, None, sto_mode, 0, cfo_mode, 0.0, p(rx),
                                                None, None, None, None, flags)
    assert sweep(3, 0, L.OFDM_F32) != 0 and sweep(0, -1, L.OFDM_F32) != 0
    assert gen(0, 3, L.OFDM_F32) != 0 and gen(-1, 0, L.OFDM_F32) != 0
    assert sweep(2, 2, L.OFDM_F64) != 0 and gen(2, 2, L.OFDM_F64) != 0
    assert sweep(2, 2, L.OFDM_F32) == 0 and gen(2, 2, L.OFDM_F32) == 0      # the same calls, well formed


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


def test_sweep_driver_c3_equals_direct_calls(ofdm, tmp_path):
    """sweep_ber --config C3: world 1 == ber_sweep_task4 per tile with the same keys; two gloo ranks == one process."""
    from ofdm_course_amd import frames as fr
    from ofdm_course_amd import sweep
    from ofdm_course_amd.drivers import sweep_ber
    snrs, batches, fpt, seed = [10.0, 20.0, 30.0], 2, 8, 7
    got = sweep_ber.run("C3", snrs, batches, fpt, "fp32", seed=seed, backend="gloo")
    cfg = fr.config_C3()
    plan = fr.make_plan(cfg, ofdm, precision="fp32")
    h, _ = ofdm.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    err = np.zeros(len(snrs), dtype=np.int64)
    st = np.zeros((len(snrs), 4), dtype=np.int64)
    cae = np.zeros(len(snrs))
    for si, bi in sweep.tiles_for_rank(len(snrs), batches, 0, 1):
        key, stream0 = sweep.tile_seed_stream(seed, si, bi, fpt)
        r = plan.ber_sweep_task4([snrs[si]], fpt, h=h, Time_Delay="random", Freq_Shift="random", seeds=[key], frame0=stream0)
        err[si] += r["errors"][0]
        st[si] += r["status_counts"][0]
        cae[si] += r["cfo_abs_err"][0]
    assert got["errors"] == err.tolist()
    assert got["status_counts"] == st.tolist()
    assert got["bits"] == [batches * fpt * plan.frame_bits] * len(snrs)
    assert np.allclose(got["cfo_abs_err"], cae, rtol=1e-12, atol=0)
    common = ["--config", "C3", "--batches", "2", "--frames-per-tile", "4", "--snrs", "12", "24"]
    one = _run([sys.executable, "-m", "ofdm_course_amd.drivers.sweep_ber", *common, "--json", str(tmp_path / "one.json")],
               tmp_path / "one.json")
    two = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                "127.0.0.1", "--master-port", str(_free_port()), "-m", "ofdm_course_amd.drivers.sweep_ber", *common,
                "--backend", "gloo", "--force-device", "0", "--json", str(tmp_path / "two.json")], tmp_path / "two.json")
    assert two["n_gpus"] == 2 and one["n_gpus"] == 1
    assert one["errors"] == two["errors"] and one["bits"] == two["bits"]
    assert one["status_counts"] == two["status_counts"]
    assert np.allclose(one["cfo_abs_err"], two["cfo_abs_err"], rtol=1e-12, atol=0)
