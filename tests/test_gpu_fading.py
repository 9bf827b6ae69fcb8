"""ofdm_tx_frames_fading (the fused generator with a channel drawn per frame) and ofdm_ber_sweep_task5_fading (the Task-5
BER(SNR) sweep over those realisations, with the channel-estimate error): the draw against its restatement on the oracle's
Philox, the generator against the oracle's composition with each frame's own h, the sweep's counts and NMSE sums against
rx_chain_task5 on the same frames, call by call."""
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

REG = (1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0)          # T5/Main_model_Task_5.m:55
EPA = ((0, 1, 2, 3, 6, 13),                                   # fading_profile("EPA", 30.72e6): inside M's K = 128 atoms
       (0.32130224, 0.25521944, 0.20272801, 0.21195555, 0.00612229, 0.00267248))


def _cfg(name):
    from ofdm_course_amd import frames as fr
    if name == "M":
        return fr.config_M()
    if name == "small":
        return fr.config_small()
    return fr.config_small(nfft=256, n_carrier=64, comb=4, const="QPSK", n_symb=3, dominant_taps=3)      # qpsk256


def _fading(name):
    if name == "M":
        return EPA
    return (0, 3, 7), (1.0, 0.36, 0.09)                       # inside the small plans' K = 16 atoms, dominant_taps = 3


def draw_taps(oracle, delays, powers, seed, frame0, n_frames):
    """The draw convention of ofdm_tx_frames_fading restated: tap t of frame f from Philox4x32-10 counter
    (t, 0, frame0 + f, 3), key = seed; u = (word0 + 0.5) 2^-32; a = sqrt(power_t / sum power) e^{2 pi i u}.  [n_frames, n_taps]"""
    n = len(delays)
    pw = np.asarray(powers, dtype=np.float64)
    g = np.sqrt(pw / np.sum(pw))
    ctr = np.array([[t, 0, frame0 + f, 3] for f in range(n_frames) for t in range(n)], dtype=np.uint64)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    u = (oracle.philox4x32_10(ctr, key)[:, 0].astype(np.float64) + 0.5) * 2.0 ** -32
    return g[None, :] * np.exp(2j * np.pi * u.reshape(n_frames, n))


def dense_h(delays, amps):
    h = np.zeros(max(delays) + 1, dtype=np.complex128)
    h[list(delays)] = amps
    return h


def point_sum(v):
    """The documented order of the per-point sums: thread i of 256 adds frames i, i + 256, ...; a butterfly (xor 32 .. 1) over
    each wavefront of 64; the four partials as (p0 + p1) + (p2 + p3)."""
    lanes = np.zeros(256)
    for i, x in enumerate(np.asarray(v, dtype=np.float64)):
        lanes[i % 256] += x
    w = lanes.reshape(4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[:, np.arange(64) ^ off]
    return (w[0, 0] + w[1, 0]) + (w[2, 0] + w[3, 0])


def true_nmse(delays, amps, H_est, nfft, nc):
    """sum_k |fft(h_f, Nfft)(k) - H_est(k, f)|^2 over carriers 1..N_carrier, per frame, in double"""
    out = np.empty(amps.shape[0])
    for f in range(amps.shape[0]):
        d = np.fft.fft(dense_h(delays, amps[f]), nfft)[:nc] - np.asarray(H_est)[:, f].astype(np.complex128)
        out[f] = np.sum(d.real ** 2 + d.imag ** 2)
    return out


def test_taps_follow_the_draw_convention(ofdm, oracle):
    from ofdm_course_amd import frames as fr
    plan = fr.make_plan(_cfg("small"), ofdm, precision="fp64")
    delays, powers = (0, 2, 5, 9, 17, 30), (1.0, 0.5, 0.3, 0.2, 0.05, 0.01)
    seed, f0 = 0x1234ABCD5, 7
    gen = plan.tx_frames_fused(5, fading=(delays, powers), SNR=20.0, seed=seed, frame0=f0, want_taps=True)
    taps = np.asarray(gen["taps"])
    assert taps.shape == (5, 6) and taps.dtype == np.complex128
    assert np.max(np.abs(taps - draw_taps(oracle, delays, powers, seed, f0, 5))) <= 1e-13
    assert np.max(np.abs(np.sum(np.abs(taps) ** 2, axis=1) - 1.0)) <= 1e-13
    sub = plan.tx_frames_fused(2, fading=(delays, powers), SNR=20.0, seed=seed, frame0=f0 + 2, want_taps=True)
    assert np.array_equal(np.asarray(sub["taps"]), taps[2:4])                   # (seed, frame0 + f, t) only
    assert np.array_equal(np.asarray(sub["rx"]), np.asarray(gen["rx"])[:, 2:4])
    other = plan.tx_frames_fused(5, fading=(delays, powers), SNR=20.0, seed=seed, frame0=f0 + 100, want_taps=True)
    assert np.min(np.abs(np.asarray(other["taps"]) - taps)) > 0                 # another frame0: other realisations


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("name", ["qpsk256", "M"])
def test_fading_generator_equals_the_oracle_composition(ofdm, oracle, precision, name):
    """M: 32 256 samples = 8 segments of 4096 with a 300-sample halo across their boundaries."""
    import torch
    from ofdm_course_amd import frames as fr
    cfg = _cfg(name)
    plan = fr.make_plan(cfg, ofdm, precision=precision, device=0)
    tol = 1e-13 if precision == "fp64" else 2e-6
    delays, powers = ((0, 5, 40, 300), (1.0, 0.5, 0.25, 0.1)) if name == "M" else ((0, 3, 7), (1.0, 0.36, 0.09))
    nfr, seed, f0 = 5, 0x1234ABCD5, 7
    gen = plan.tx_frames_fused(nfr, fading=(delays, powers), SNR=cfg.SNR_dB, seed=seed, frame0=f0, want_taps=True)
    amps = draw_taps(oracle, delays, powers, seed, f0, nfr)
    assert np.max(np.abs(np.asarray(gen["taps"]) - amps)) <= 1e-13
    _, bps = oracle.constellation_func(cfg.Constellation)
    nd = len(cfg.dataCarriers)
    pv = np.repeat(fr.pilot_column(cfg, ofdm)[:, None], cfg.N_symb, axis=1)
    rx = np.asarray(gen["rx"])
    for f in range(nfr):
        bits = oracle.payload_bits_philox(nd * cfg.N_symb, bps, seed, f0 + f)
        assert np.array_equal(np.asarray(gen["packed"])[f], fr.pack_bits(bits[None, :])[0])      # bit-exact
        noise = oracle.awgn_philox(cfg.frame_samples, seed, f0 + f)
        want, _ = oracle.tx_frame(bits, cfg.Nfft, cfg.T_guard, cfg.N_symb, cfg.dataCarriers, cfg.pilotCarriers, pv,
                                  cfg.Constellation, h=dense_h(delays, amps[f]), SNR=cfg.SNR_dB, noise=noise,
                                  noise_first=True)
        assert rel_l2(rx[:, f], want) < tol
    # one tap at delay 0 with power 1: frame f is the static generator's frame with h = [a_f0]
    one = plan.tx_frames_fused(nfr, fading=((0,), (1.0,)), SNR=cfg.SNR_dB, seed=seed, frame0=f0, want_taps=True)
    a0 = draw_taps(oracle, (0,), (1.0,), seed, f0, nfr)
    for f in range(nfr):
        static = plan.tx_frames_fused(1, h=a0[f], SNR=cfg.SNR_dB, seed=seed, frame0=f0 + f)
        assert rel_l2(np.asarray(one["rx"])[:, f], np.asarray(static["rx"])[:, 0]) < tol
        assert np.array_equal(np.asarray(one["packed"])[f], np.asarray(static["packed"])[0])
    # the device flavour returns the host flavour's arrays
    dgen = plan.tx_frames_fused(nfr, fading=(delays, powers), SNR=cfg.SNR_dB, seed=seed, frame0=f0, want_taps=True,
                                device="cuda:0")
    torch.cuda.synchronize()
    assert np.array_equal(dgen["rx"].cpu().numpy(), rx)
    assert np.array_equal(dgen["taps"].cpu().numpy(), np.asarray(gen["taps"]))
    assert np.array_equal(dgen["packed"].cpu().numpy(), np.asarray(gen["packed"]))


def test_fading_generator_with_the_scrambler(ofdm, oracle):
    """The Scrambler stage is ofdm_tx_frames_fused's: the packed payload and scrambled bits are those of the static call."""
    from ofdm_course_amd import frames as fr
    plan = fr.make_plan(_cfg("small"), ofdm, precision="fp32")
    fad = _fading("small")
    gen = plan.tx_frames_fused(4, fading=fad, SNR=25.0, seed=77, frame0=1000, Register=REG)
    ref = plan.tx_frames_fused(4, h=None, SNR=25.0, seed=77, frame0=1000, Register=REG)
    assert np.array_equal(np.asarray(gen["packed"]), np.asarray(ref["packed"]))
    assert np.array_equal(np.asarray(gen["sc_packed"]), np.asarray(ref["sc_packed"]))


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("name", ["small", "M"])
def test_fading_sweep_equals_the_composed_path(ofdm, oracle, precision, name):
    from ofdm_course_amd import frames as fr
    cfg = _cfg(name)
    plan = fr.make_plan(cfg, ofdm, precision=precision)
    delays, powers = fad = _fading(name)
    snrs, seeds, fpp, f0 = [0.0, 10.0, 20.0], [11, 12, 13], 24, 40
    res = plan.ber_sweep(snrs, fpp, fading=fad, seeds=seeds, frame0=f0, want_frame_errors=True, want_nmse=True,
                         want_frame_nmse=True)
    fe = np.asarray(res["frame_errors"]).astype(np.int64)
    fn = np.asarray(res["frame_nmse"])
    assert res["bits"] == fpp * plan.frame_bits
    assert np.array_equal(np.asarray(res["errors"]), fe.sum(axis=1))
    for p, (snr, sd) in enumerate(zip(snrs, seeds)):
        gen = plan.tx_frames_fused(fpp, fading=fad, SNR=snr, seed=sd, frame0=f0)
        out = ofdm.rx_chain_task5(plan, gen["rx"], ref_bits_packed=gen["packed"], want_h=True)
        assert np.array_equal(fe[p], np.asarray(out["errors"]).astype(np.int64))
        amps = draw_taps(oracle, delays, powers, sd, f0, fpp)
        want = true_nmse(delays, amps, out["H"], cfg.Nfft, cfg.N_carrier)
        print(name, precision, snr, "frame_nmse rel", np.max(np.abs(fn[p] - want) / want))
        assert np.all(np.abs(fn[p] - want) <= 1e-9 * want)
        if precision == "fp64" and name == "small":     # against the oracle's receiver on the same frames
            ow = oracle.rx_chain_task5(np.asarray(gen["rx"]), cfg.Nfft, cfg.T_guard, cfg.N_carrier, cfg.pilotCarriers,
                                       cfg.dataCarriers, fr.pilot_column(cfg, ofdm), cfg.K, cfg.dominant_taps,
                                       cfg.Constellation)
            wo = true_nmse(delays, amps, ow["H"].T, cfg.Nfft, cfg.N_carrier)
            print(name, precision, snr, "frame_nmse rel (oracle)", np.max(np.abs(fn[p] - wo) / wo))
            assert np.all(np.abs(fn[p] - wo) <= 1e-8 * wo)
        assert np.asarray(res["nmse_sums"])[p] == point_sum(fn[p])                  # one call's outputs: bitwise
    assert np.array_equal(np.asarray(res["NMSE"]), np.asarray(res["nmse_sums"]) / (fpp * cfg.N_carrier))


def test_fading_sweep_invariance(ofdm):
    """Chunking, point grouping, repetition and the device flavour leave every count and every NMSE sum unchanged, bitwise."""
    import torch
    from ofdm_course_amd import frames as fr
    plan = fr.make_plan(_cfg("M"), ofdm, precision="fp32", device=0)
    snrs, seeds, fpp = [5.0, 12.0, 20.0], [3, 4, 5], 24
    kw = dict(fading=EPA, frame0=9, want_frame_errors=True, want_nmse=True)
    base = plan.ber_sweep(snrs, fpp, seeds=seeds, **kw)
    for chunk in (0, 7, 24):
        got = plan.ber_sweep(snrs, fpp, seeds=seeds, max_frames_per_chunk=chunk, **kw)
        assert np.array_equal(np.asarray(got["frame_errors"]), np.asarray(base["frame_errors"]))
        assert np.array_equal(got["errors"], base["errors"])
        assert np.array_equal(np.asarray(got["nmse_sums"]), np.asarray(base["nmse_sums"]))
    for p in range(3):
        one = plan.ber_sweep([snrs[p]], fpp, seeds=[seeds[p]], **kw)
        assert one["errors"][0] == base["errors"][p]
        assert np.asarray(one["nmse_sums"])[0] == np.asarray(base["nmse_sums"])[p]
    again = plan.ber_sweep(snrs, fpp, seeds=seeds, **kw)                           # a repeated call
    assert np.array_equal(again["errors"], base["errors"])
    assert np.array_equal(np.asarray(again["nmse_sums"]), np.asarray(base["nmse_sums"]))
    dev = plan.ber_sweep(snrs, fpp, seeds=seeds, device="cuda:0", **kw)
    assert isinstance(dev["nmse_sums"], torch.Tensor) and dev["nmse_sums"].is_cuda
    assert np.array_equal(dev["errors"].cpu().numpy(), base["errors"])
    assert np.array_equal(dev["nmse_sums"].cpu().numpy(), np.asarray(base["nmse_sums"]))
    # the NMSE outputs change nothing else, and another frame0 is another set of realisations
    plain = plan.ber_sweep(snrs, fpp, seeds=seeds, fading=EPA, frame0=9)
    assert np.array_equal(plain["errors"], base["errors"])
    a = plan.tx_frames_fused(4, fading=EPA, seed=3, frame0=9, want_taps=True)["taps"]
    b = plan.tx_frames_fused(4, fading=EPA, seed=3, frame0=10, want_taps=True)["taps"]
    assert not np.array_equal(np.asarray(a), np.asarray(b)) and np.array_equal(np.asarray(a)[1:], np.asarray(b)[:3])


def test_fading_sweep_nmse_and_ber_fall_with_snr(ofdm):
    from ofdm_course_amd import frames as fr
    plan = fr.make_plan(_cfg("M"), ofdm, precision="fp32", device=0)
    res = plan.ber_sweep([5.0, 15.0, 25.0], 64, fading=EPA, seed=9, device="cuda:0", want_nmse=True)
    nmse = res["NMSE"].cpu().numpy()
    ber = res["errors"].cpu().numpy() / res["bits"]
    assert np.all(np.isfinite(nmse)) and np.all(np.diff(nmse) < 0), nmse
    assert ber[2] < ber[0], ber


def test_fading_refusals_leave_the_plan_usable(ofdm):
    from ofdm_course_amd import frames as fr
    cfg = _cfg("M")
    plan = fr.make_plan(cfg, ofdm, precision="fp32")
    h, _ = ofdm.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    ok = plan.ber_sweep([20.0], 8, fading=EPA, seed=5, want_nmse=True)
    bad = [((), ()),                                                    # n_taps 0
           (tuple(range(65)), (1.0,) * 65),                             # n_taps 65
           ((0, 3, 3), (1.0, 0.5, 0.2)),                                # a repeated delay
           ((0, 4097), (1.0, 0.5)),                                     # a delay beyond the 4096-sample halo
           ((0, -1), (1.0, 0.5)),
           ((0, 3), (1.0, 0.0)),                                        # non-positive powers
           ((0, 3), (1.0, -0.5))]
    for fad in bad:
        with pytest.raises(ofdm.OfdmError):
            plan.ber_sweep([20.0], 8, fading=fad, seed=5)
        with pytest.raises(ofdm.OfdmError):
            plan.tx_frames_fused(2, fading=fad, seed=5)
    with pytest.raises(ofdm.OfdmError):                                 # one channel or a channel per frame, not both
        plan.ber_sweep([20.0], 8, h=h, fading=EPA, seed=5)
    with pytest.raises(ofdm.OfdmError):
        plan.tx_frames_fused(2, h=h, fading=EPA, seed=5)
    with pytest.raises(ofdm.OfdmError):                                 # NMSE is against a drawn channel
        plan.ber_sweep([20.0], 8, h=h, seed=5, want_nmse=True)
    hh = np.zeros(cfg.N_carrier, dtype=np.complex128)
    hh[: len(h)] = h
    plan.set_mmse(hh, 20.0)
    with pytest.raises(ofdm.OfdmError):                                 # an MMSE operator is built for one h
        plan.ber_sweep([20.0], 8, fading=EPA, seed=5)
    plan.set_mmse(None)
    again = plan.ber_sweep([20.0], 8, fading=EPA, seed=5, want_nmse=True)
    assert np.array_equal(again["errors"], ok["errors"]) and np.array_equal(again["nmse_sums"], ok["nmse_sums"])


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


def test_two_rank_fading_sweep_equals_single_process(tmp_path):
    """The driver with --fused --fading EPA --nmse: two gloo ranks on one GPU against one process -- the integer counters
    equal, the NMSE sums to the association of the float64 all-reduce."""
    common = ["--config", "M", "--batches", "2", "--frames-per-tile", "3", "--snrs", "4", "16", "28", "--fused", "--fading",
              "EPA", "--nmse"]
    one = _run([sys.executable, "-m", "ofdm_course_amd.drivers.sweep_ber", *common, "--json", str(tmp_path / "one.json")],
               tmp_path / "one.json")
    two = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                "127.0.0.1", "--master-port", str(_free_port()), "-m", "ofdm_course_amd.drivers.sweep_ber", *common,
                "--backend", "gloo", "--force-device", "0", "--json", str(tmp_path / "two.json")], tmp_path / "two.json")
    assert two["n_gpus"] == 2 and one["n_gpus"] == 1
    assert one["errors"] == two["errors"] and one["bits"] == two["bits"]
    assert one["fading"]["profile"] == "EPA" and one["fading"]["delays"] == [0, 1, 2, 3, 6, 13]
    a, b = np.asarray(one["NMSE"]), np.asarray(two["NMSE"])
    assert np.all(a > 0) and np.all(np.abs(a - b) <= 1e-12 * a)
    assert np.all(np.abs(np.asarray(one["nmse_sums"]) - a * (2 * 3 * 512)) <= 1e-12 * np.asarray(one["nmse_sums"]))
