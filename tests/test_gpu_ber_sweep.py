"""ofdm_tx_frames_fused (the reference-order generator in three sample passes) and ofdm_ber_sweep_task5 (one device-resident
tile of a BER(SNR) sweep): the generator against the oracle's composition of the TX + channel sections
(oracle.tx_frame(noise_first=True) on the Philox draws) and against ofdm_tx_frames_ex(noise_first=1); the sweep's counts
against rx_chain_task5 on the same frames, call by call."""
import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu

REG = (1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0)          # T5/Main_model_Task_5.m:55


def _cfg(name):
    from ofdm_course_amd import frames as fr
    if name == "M":
        return fr.config_M()
    if name == "C5":
        return fr.config_C5()
    if name == "small":
        return fr.config_small()
    nfft, nc, comb, const = {"qpsk256": (256, 64, 4, "QPSK"), "8psk1024": (1024, 400, 8, "8PSK")}[name]
    return fr.config_small(nfft=nfft, n_carrier=nc, comb=comb, const=const, n_symb=3, dominant_taps=3)


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("name", ["qpsk256", "M", "8psk1024", "C5"])
def test_fused_generator_equals_the_oracle_composition(ofdm, oracle, precision, name):
    from ofdm_course_amd import frames as fr
    cfg = _cfg(name)
    plan = fr.make_plan(cfg, ofdm, precision=precision)
    nfr = 4 if name == "C5" else 5
    n_oracle = 2 if name == "C5" else nfr              # Nfft 8192 with 32 taps: two frames through the oracle
    seed, f0 = 0x1234ABCD5, 7
    h, _ = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    gen = plan.tx_frames_fused(nfr, h=h, SNR=cfg.SNR_dB, seed=seed, frame0=f0)
    _, bps = oracle.constellation_func(cfg.Constellation)
    nd = len(cfg.dataCarriers)
    pv = np.repeat(fr.pilot_column(cfg, ofdm)[:, None], cfg.N_symb, axis=1)
    rx = np.asarray(gen["rx"])
    for f in range(n_oracle):
        bits = oracle.payload_bits_philox(nd * cfg.N_symb, bps, seed, f0 + f)
        assert np.array_equal(np.asarray(gen["packed"])[f], fr.pack_bits(bits[None, :])[0])      # bit-exact
        noise = oracle.awgn_philox(cfg.frame_samples, seed, f0 + f)
        want, _ = oracle.tx_frame(bits, cfg.Nfft, cfg.T_guard, cfg.N_symb, cfg.dataCarriers, cfg.pilotCarriers, pv,
                                  cfg.Constellation, h=h, SNR=cfg.SNR_dB, noise=noise, noise_first=True)
        assert rel_l2(rx[:, f], want) < (1e-13 if precision == "fp64" else 2e-6)
    if precision == "fp64":                              # the staged generator in the same order: rounding apart, equal
        ex = plan.tx_frames(nfr, h=h, SNR=cfg.SNR_dB, seed=seed, frame0=f0, noise_first=True)
        assert np.array_equal(np.asarray(ex["packed"]), np.asarray(gen["packed"]))
        for f in range(nfr):
            assert rel_l2(rx[:, f], np.asarray(ex["rx"])[:, f]) < 1e-13
    # batching independence: frames 2..3 generated alone are the same arrays, bit for bit
    sub = plan.tx_frames_fused(2, h=h, SNR=cfg.SNR_dB, seed=seed, frame0=f0 + 2)
    assert np.array_equal(np.asarray(sub["rx"]), rx[:, 2:4])
    assert np.array_equal(np.asarray(sub["packed"]), np.asarray(gen["packed"])[2:4])


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_fused_generator_scrambler_and_device_flavour(ofdm, oracle, precision):
    """Scrambler per frame (register reset): packed payload and scrambled bits bit-equal to tx_frames_ex's, waveform ==
    the oracle's composition; the device flavour returns the host flavour's arrays; no channel = Noise only."""
    import torch
    from ofdm_course_amd import frames as fr
    cfg = fr.config_small(nfft=512, n_carrier=200, comb=5, const="16QAM", n_symb=4, dominant_taps=3)
    plan = fr.make_plan(cfg, ofdm, precision=precision, device=0)
    nfr, seed, f0 = 6, 77, 1000
    h, _ = oracle.get_MP_channel_resp(np.array([[0, 1.0], [4, 0.6], [10, 0.3]]), cfg.Nfft)
    gen = plan.tx_frames_fused(nfr, h=h, SNR=25.0, seed=seed, frame0=f0, Register=REG)
    ex = plan.tx_frames(nfr, h=h, SNR=25.0, seed=seed, frame0=f0, Register=REG, noise_first=True, want_bits=True)
    assert np.array_equal(np.asarray(gen["packed"]), np.asarray(ex["packed"]))
    assert np.array_equal(np.asarray(gen["sc_packed"]), np.asarray(ex["sc_packed"]))
    pv = np.repeat(fr.pilot_column(cfg, ofdm)[:, None], cfg.N_symb, axis=1)
    for f in range(nfr):
        bits = np.asarray(ex["bits"])[f]
        noise = oracle.awgn_philox(cfg.frame_samples, seed, f0 + f)
        want, sc = oracle.tx_frame(bits, cfg.Nfft, cfg.T_guard, cfg.N_symb, cfg.dataCarriers, cfg.pilotCarriers, pv,
                                   cfg.Constellation, h=h, SNR=25.0, noise=noise, Register=REG, noise_first=True)
        assert np.array_equal(np.asarray(gen["sc_packed"])[f], fr.pack_bits(sc[None, :])[0])
        assert rel_l2(np.asarray(gen["rx"])[:, f], want) < (1e-13 if precision == "fp64" else 2e-6)
    dgen = plan.tx_frames_fused(nfr, h=h, SNR=25.0, seed=seed, frame0=f0, Register=REG, device="cuda:0")
    torch.cuda.synchronize()
    assert np.array_equal(dgen["rx"].cpu().numpy(), np.asarray(gen["rx"]))
    assert np.array_equal(dgen["sc_packed"].cpu().numpy(), np.asarray(gen["sc_packed"]))
    flat = plan.tx_frames_fused(2, h=None, SNR=25.0, seed=seed, frame0=f0)
    flat_ex = plan.tx_frames(2, h=None, SNR=25.0, seed=seed, frame0=f0, noise_first=True)
    assert rel_l2(np.asarray(flat["rx"]), np.asarray(flat_ex["rx"])) < (1e-13 if precision == "fp64" else 2e-6)


def _composed(ofdm, plan, gen):
    return np.asarray(ofdm.rx_chain_task5(plan, gen["rx"], ref_bits_packed=gen["packed"])["errors"]).astype(np.int64)


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("name", ["small", "M"])
def test_sweep_equals_the_composed_path(ofdm, oracle, precision, name):
    from ofdm_course_amd import frames as fr
    cfg = _cfg(name)
    plan = fr.make_plan(cfg, ofdm, precision=precision)
    h, _ = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    snrs, seeds, fpp, f0 = [0.0, 10.0, 20.0], [11, 12, 13], 24, 40
    res = plan.ber_sweep(snrs, fpp, h=h, seeds=seeds, frame0=f0, want_frame_errors=True)
    fe = np.asarray(res["frame_errors"]).astype(np.int64)
    assert res["bits"] == fpp * plan.frame_bits
    assert np.array_equal(np.asarray(res["errors"]), fe.sum(axis=1))
    for p, (snr, sd) in enumerate(zip(snrs, seeds)):
        fused = _composed(ofdm, plan, plan.tx_frames_fused(fpp, h=h, SNR=snr, seed=sd, frame0=f0))
        assert np.array_equal(fe[p], fused)
        staged = _composed(ofdm, plan, plan.tx_frames(fpp, h=h, SNR=snr, seed=sd, frame0=f0, noise_first=True))
        if precision == "fp64":
            assert np.array_equal(fe[p], staged)
        else:
            assert abs(int(fe[p].sum()) - int(staged.sum())) <= 1e-5 * res["bits"]
    assert fe[0].sum() > fe[2].sum()


def test_sweep_invariance(ofdm, oracle):
    """Chunking, point grouping, repetition and the device flavour leave every count unchanged."""
    import torch
    from ofdm_course_amd import frames as fr
    cfg = fr.config_M()
    plan = fr.make_plan(cfg, ofdm, precision="fp32", device=0)
    h, _ = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    snrs, seeds, fpp = [5.0, 12.0, 20.0], [3, 4, 5], 24
    base = plan.ber_sweep(snrs, fpp, h=h, seeds=seeds, frame0=9, want_frame_errors=True)
    small = plan.ber_sweep(snrs, fpp, h=h, seeds=seeds, frame0=9, want_frame_errors=True, max_frames_per_chunk=7)
    assert np.array_equal(np.asarray(small["frame_errors"]), np.asarray(base["frame_errors"]))
    assert np.array_equal(small["errors"], base["errors"])
    for p in range(3):
        one = plan.ber_sweep([snrs[p]], fpp, h=h, seeds=[seeds[p]], frame0=9, want_frame_errors=True)
        assert np.array_equal(np.asarray(one["frame_errors"])[0], np.asarray(base["frame_errors"])[p])
    again = plan.ber_sweep(snrs, fpp, h=h, seeds=seeds, frame0=9, want_frame_errors=True)
    assert np.array_equal(np.asarray(again["frame_errors"]), np.asarray(base["frame_errors"]))
    dev = plan.ber_sweep(snrs, fpp, h=h, seeds=seeds, frame0=9, want_frame_errors=True, device="cuda:0")
    assert isinstance(dev["errors"], torch.Tensor) and dev["errors"].is_cuda
    assert np.array_equal(dev["errors"].cpu().numpy(), base["errors"])
    assert np.array_equal(dev["frame_errors"].cpu().numpy().astype(np.uint32), np.asarray(base["frame_errors"]))
    # one seed for every point (the default) == that seed repeated
    same = plan.ber_sweep(snrs, 8, h=h, seed=21, frame0=0)
    assert np.array_equal(same["errors"], plan.ber_sweep(snrs, 8, h=h, seeds=[21, 21, 21], frame0=0)["errors"])


def test_sweep_modes(ofdm, oracle):
    """Scrambler + DeScrambler plan, MMSE plan (one point), and the refused combinations."""
    from ofdm_course_amd import frames as fr
    cfg = fr.config_M()
    plan = fr.make_plan(cfg, ofdm, precision="fp32")
    h, _ = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    fpp = 16
    with pytest.raises(ofdm.OfdmError):                  # scrambled frames, plan without a DeScrambler
        plan.ber_sweep([20.0], fpp, h=h, seed=2, Register=REG)
    plan.set_descrambler(REG)
    with pytest.raises(ofdm.OfdmError):                  # a descrambling plan, unscrambled frames
        plan.ber_sweep([20.0], fpp, h=h, seed=2)
    res = plan.ber_sweep([10.0, 20.0], fpp, h=h, seeds=[2, 3], Register=REG, want_frame_errors=True)
    for p, (snr, sd) in enumerate(((10.0, 2), (20.0, 3))):
        gen = plan.tx_frames_fused(fpp, h=h, SNR=snr, seed=sd, Register=REG)
        assert np.array_equal(np.asarray(res["frame_errors"])[p].astype(np.int64), _composed(ofdm, plan, gen))
    other = list(REG)
    other[3] = 0
    with pytest.raises(ofdm.OfdmError):                  # a different register on the plan
        plan.ber_sweep([20.0], fpp, h=h, seed=2, Register=other)
    plan.set_descrambler(None)
    hh = np.zeros(cfg.N_carrier, dtype=np.complex128)
    hh[: len(h)] = h
    plan.set_mmse(hh, 20.0)
    res = plan.ber_sweep([20.0], fpp, h=h, seed=5, want_frame_errors=True)
    gen = plan.tx_frames_fused(fpp, h=h, SNR=20.0, seed=5)
    assert np.array_equal(np.asarray(res["frame_errors"])[0].astype(np.int64), _composed(ofdm, plan, gen))
    with pytest.raises(ofdm.OfdmError):
        plan.ber_sweep([10.0, 20.0], fpp, h=h, seed=5)
    plan.set_mmse(None)
    bad = np.zeros(5000, dtype=np.complex128)
    bad[4500] = 1.0
    with pytest.raises(ofdm.OfdmError):                  # a tap beyond the 4096-sample halo
        plan.tx_frames_fused(1, h=bad)


def test_sweep_c5_tile(ofdm):
    """768 C5 frames at 20 dB (the 511-sample halo of the 32-tap channel): per-frame counts == the composed path."""
    import torch
    from ofdm_course_amd import frames as fr
    cfg = fr.config_C5()
    plan = fr.make_plan(cfg, ofdm, precision="fp32", device=0)
    h, _ = ofdm.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    dev = torch.device("cuda:0")
    F = 768
    res = plan.ber_sweep([20.0], F, h=h, seed=5, device=dev, want_frame_errors=True)
    gen = plan.tx_frames_fused(F, h=h, SNR=20.0, seed=5, device=dev)
    out = ofdm.rx_chain_task5(plan, gen["rx"], ref_bits_packed=gen["packed"])
    assert torch.equal(res["frame_errors"][0], out["errors"])
    assert int(res["errors"][0].item()) == int(out["errors"].to(torch.int64).sum().item())


def test_sweep_ber_falls_with_snr(ofdm, oracle):
    from ofdm_course_amd import frames as fr
    cfg = fr.config_M()
    plan = fr.make_plan(cfg, ofdm, precision="fp32", device=0)
    h, _ = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    snrs = np.arange(0.0, 31.0, 5.0)
    res = plan.ber_sweep(snrs, 64, h=h, seed=9, device="cuda:0")
    ber = res["errors"].cpu().numpy() / res["bits"]
    assert np.all(np.diff(ber) <= 0), ber
    assert ber[-1] < 0.1 * ber[1], ber


def test_sweep_driver_fused_equals_per_tile_calls(ofdm):
    from ofdm_course_amd import frames as fr
    from ofdm_course_amd import sweep
    from ofdm_course_amd.drivers import sweep_ber
    snrs, batches, fpt, seed = [0.0, 10.0, 20.0], 2, 8, 7
    got = sweep_ber.run("M", snrs, batches, fpt, "fp32", seed=seed, fused=True, backend="gloo")
    assert got["fused"] is True and got["order"] == "noise_first"
    cfg = fr.config_M()
    plan = fr.make_plan(cfg, ofdm, precision="fp32")
    h, _ = ofdm.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    want = np.zeros(len(snrs), dtype=np.int64)
    for si, bi in sweep.tiles_for_rank(len(snrs), batches, 0, 1):
        key, stream0 = sweep.tile_seed_stream(seed, si, bi, fpt)
        want[si] += plan.ber_sweep([snrs[si]], fpt, h=h, seeds=[key], frame0=stream0)["errors"][0]
    assert got["errors"] == want.tolist()
    assert got["bits"] == [batches * fpt * plan.frame_bits] * len(snrs)
