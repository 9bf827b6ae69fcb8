"""The payload transport on the GPU: tx_frames_fused(payload_bits=) (ofdm_tx_frames_payload) against the oracle's composition and
against the existing generator entries, and RxPlan.transport (ofdm_payload_transport) against its own composition from the public
pieces -- tx_frames_fused(payload_bits=) per repeat, rx_chain_task5 / rx_chain_task4, unpacking and joining in numpy
(tests/payload_cases.py) -- every integer compared exactly.

Configurations, both frames.config_small: "small" (Nfft 256, 16QAM, 5 symbols: frame_bits = 960, a multiple of 32) and "8psk"
(Nfft 1024, 400 carriers, 8PSK, 3 symbols, the variant of tests/test_gpu_papr_study.py: frame_bits = 2700, 2700 % 8 = 4 and
2700 % 32 = 12, so every frame but the first starts inside a byte and two frames meet inside an output word).  The SNRs of the
composition tests were chosen on the CPU with the oracle (tx_frame -> rx_chain_task5 over six frames): "small" 6 dB -> BER 0.110,
8 dB -> 0.069; "8psk" 4 dB -> 0.104, 6 dB -> 0.065: far from 0 and from one half.  The Task-4 receiver with time_desync on zeroes
the first OFDM symbol (T4/Main_model_Task_4.m:292-294): on "8psk" that is a third of the frame, BER near 1 / 6 once its
synchroniser locks.  On these short frames it locks at 30 and 35 dB, the points of that case (measured: 934 of 5413 bits wrong in
every repeat at both: the zeroed symbol, the rest decoded), and not at 20 dB (all-zero decisions, 2731 wrong)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import payload_cases as pc
from conftest import rel_l2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG = (1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0)          # T3/Main_model_Task_3.m:36
T3_TAPS = np.array([[0, 1.0], [2, 0.4], [4, 0.01]])           # T3/Main_model_Task_3.m:122-126
LINE = ([0, 3, 9], [1.0, 0.5, 0.25])
SNRS = {"small": [6.0, 8.0], "8psk": [4.0, 6.0], "task4": [30.0, 35.0]}


def _cfg(kind):
    from ofdm_course_amd import frames as fr
    if kind == "small":
        return fr.config_small()
    return fr.config_small(nfft=1024, n_carrier=400, const="8PSK", n_symb=3)


def _plan(ofdm, kind, precision):
    from ofdm_course_amd import frames as fr
    cfg = _cfg(kind)
    return cfg, fr.make_plan(cfg, ofdm, precision=precision, device=0)


def _payload(n_bits, seed=7):
    return np.random.default_rng(seed).integers(0, 2, n_bits, dtype=np.uint8)


def _same(a, b, keys=None):
    for k in (a.keys() if keys is None else keys):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert keys is not None or set(a) == set(b)


# ---- 1. the generator against the oracle
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("register", [None, REG], ids=["plain", "scrambled"])
@pytest.mark.parametrize("channel", ["h", "none"])
def test_generator_with_a_payload_equals_the_oracle_composition(ofdm, oracle, precision, register, channel):
    """"8psk" (frame_bits % 8 = 4): a payload of 2 frame_bits + 13 bits whose second frame is all zeros; frame 2 carries zeros beyond
    bit 13; ref_bits and sc_ref_bits exactly, rx to the tolerances of tests/test_gpu_txgen.py."""
    from ofdm_course_amd import frames as fr
    cfg, plan = _plan(ofdm, "8psk", precision)
    fb = plan.frame_bits
    assert fb == 2700 and fb % 8 == 4
    bits = _payload(2 * fb + 13)
    bits[fb:2 * fb] = 0
    seed, f0, snr = 0x1234ABCD5, 5, 20.0
    h = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)[0] if channel == "h" else None
    gen = plan.tx_frames_fused(3, h=h, SNR=snr, seed=seed, frame0=f0, Register=register, payload_bits=bits)
    frames = pc.cut(bits, fb, 0, 3)
    assert not frames[1].any() and not frames[2][13:].any() and frames[2][:13].tolist() == bits[2 * fb:].tolist()
    pv = np.repeat(fr.pilot_column(cfg, ofdm)[:, None], cfg.N_symb, axis=1)
    tol = ((1e-12 if register else 1e-13) if precision == "fp64" else (3e-6 if register else 2e-6))
    for f in range(3):
        noise = oracle.awgn_philox(cfg.frame_samples, seed, f0 + f)
        want, sc = oracle.tx_frame(frames[f], cfg.Nfft, cfg.T_guard, cfg.N_symb, cfg.dataCarriers, cfg.pilotCarriers, pv,
                                   cfg.Constellation, h=h, SNR=snr, noise=noise, Register=register, noise_first=True)
        assert np.array_equal(np.asarray(gen["packed"])[f], fr.pack_bits(frames[f][None, :])[0])
        if register:
            assert np.array_equal(np.asarray(gen["sc_packed"])[f], fr.pack_bits(sc[None, :])[0])
        err = rel_l2(np.asarray(gen["rx"])[:, f], want)
        print(f"frame {f}: rel l2 {err:.3e} (bound {tol:.0e})")
        assert err < tol
    assert not fr.unpack_bits(np.asarray(gen["packed"])[2], plan.frame_bytes * 8)[0, 13:].any()
    # the packed form of the same stream, and the device flavour
    packed = plan.tx_frames_fused(3, h=h, SNR=snr, seed=seed, frame0=f0, Register=register, payload_packed=(np.packbits(bits), bits.size))
    _same(packed, gen)
    import torch
    dev = plan.tx_frames_fused(3, h=h, SNR=snr, seed=seed, frame0=f0, Register=register, payload_bits=torch.from_numpy(bits).cuda(),
                               device="cuda:0")
    torch.cuda.synchronize()
    _same({k: v.cpu().numpy() for k, v in dev.items()}, gen)
    plan.close()


# ---- 2. only the bit source changes
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("variant", ["static", "fading", "imp", "fading-imp"])
def test_only_the_bit_source_changes(ofdm, oracle, precision, variant):
    """With the Philox bits of (seed, frame0 + f) as the payload every output equals the existing call's, bitwise."""
    from ofdm_course_amd import frames as fr
    cfg, plan = _plan(ofdm, "8psk", precision)
    seed, f0, n = 91, 11, 4
    kw = dict(SNR=12.0, seed=seed, frame0=f0)
    if variant == "static":
        kw.update(h=oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)[0], Register=REG)
    elif variant == "fading":
        kw.update(fading=LINE, want_taps=True)
    elif variant == "imp":
        kw.update(h=oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)[0], Time_Delay=12, Freq_Shift="random", want_draws=True)
    else:
        kw.update(fading=LINE, want_taps=True, Time_Delay="random", Freq_Shift=3.25, want_draws=True, Register=REG)
    old = plan.tx_frames_fused(n, **kw)
    bits = np.concatenate([oracle.payload_bits_philox(plan.n_data * cfg.N_symb, plan.bps, seed, f0 + f) for f in range(n)])
    new = plan.tx_frames_fused(n, payload_bits=bits, **kw)
    _same(new, old)
    # other bits: other samples and reference bits, the same draws
    other = plan.tx_frames_fused(n, payload_bits=bits ^ 1, **kw)
    assert not np.array_equal(np.asarray(other["rx"]), np.asarray(old["rx"]))
    assert np.array_equal(np.asarray(other["packed"]) ^ np.asarray(old["packed"]), fr.pack_bits(np.ones((n, plan.frame_bits), np.uint8)))
    _same(other, old, keys=[k for k in old if k in ("taps", "Time_Delay", "Freq_Shift")])
    plan.close()


# ---- 3. payload_frame0
@pytest.mark.parametrize("kind", ["small", "8psk"])
def test_payload_frame0_shifts_the_stream_not_the_draws(ofdm, oracle, kind):
    cfg, plan = _plan(ofdm, kind, "fp32")
    bits = _payload(2 * plan.frame_bits + 13, seed=3)
    kw = dict(h=oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)[0], SNR=15.0, seed=5, Register=REG)
    whole = plan.tx_frames_fused(4, frame0=20, payload_bits=bits, **kw)          # frame 3 lies beyond the payload: all zeros
    part = plan.tx_frames_fused(2, frame0=21, payload_bits=bits, payload_frame0=1, **kw)
    for k in ("rx", "packed", "sc_packed"):
        a = np.asarray(whole[k])
        assert np.array_equal(a[:, 1:3] if k == "rx" else a[1:3], np.asarray(part[k])), k
    assert not np.asarray(whole["packed"])[3].any() and np.asarray(whole["sc_packed"])[3].any()
    plan.close()


# ---- 4 .. 7. transport against its composition
def _compose(ofdm, plan, bits, snrs, repeats, receiver, gen_kw, seeds, frame0, flags=None, mmse_ls=False):
    """tx_frames_fused(payload_bits=) per repeat -> the receiver (ref_bits_packed=) -> unpack, join and count in numpy."""
    n_bits, fb = bits.size, plan.frame_bits
    F = pc.n_frames(n_bits, fb)
    share = np.array([pc.position(n_bits, fb, 0, F, g)[3] for g in range(F)])
    nb8 = (n_bits + 7) // 8
    out = dict(decoded=np.zeros((len(snrs), repeats, nb8), np.uint8), errors=np.zeros((len(snrs), repeats), np.int64),
               frame_errors=np.zeros((len(snrs), repeats, F), np.int64), ones=np.zeros((len(snrs), n_bits), np.int64),
               rx_errors=np.zeros((len(snrs), repeats), np.int64))
    for p, snr in enumerate(snrs):
        if mmse_ls:
            plan.set_mmse_ls(snr)
        for r in range(repeats):
            gen = plan.tx_frames_fused(F, SNR=snr, seed=seeds[p], frame0=frame0 + r * F, payload_bits=bits, **gen_kw)
            if receiver == "task4":
                got = ofdm.rx_chain_task4(plan, np.asarray(gen["rx"]), time_desync=flags[0], freq_desync=flags[1], mp_desync=flags[2],
                                          ref_bits_packed=np.asarray(gen["packed"]))
            else:
                got = ofdm.rx_chain_task5(plan, np.asarray(gen["rx"]), ref_bits_packed=np.asarray(gen["packed"]))
            frames = pc.unpack(np.asarray(got["bits"]), fb)
            stream, packed = pc.join(frames, n_bits)
            wrong = stream != bits
            out["decoded"][p, r] = packed
            out["errors"][p, r] = wrong.sum()
            out["frame_errors"][p, r] = [wrong[g * fb:g * fb + share[g]].sum() for g in range(F)]
            out["ones"][p] += stream
            out["rx_errors"][p, r] = np.asarray(got["errors"]).astype(np.int64).sum()
    return out


def _assert_transport(got, want, n_bits):
    for k in ("decoded", "errors", "frame_errors", "ones"):
        assert np.array_equal(np.asarray(got[k]), want[k]), k
    assert np.array_equal(np.asarray(got["decoded_bits"]), np.unpackbits(want["decoded"], axis=2)[:, :, :n_bits])
    assert np.array_equal(np.asarray(got["BER"]), want["errors"] / np.float64(n_bits))
    assert np.array_equal(np.asarray(got["loopback"]), want["errors"] == 0)
    assert np.array_equal(np.asarray(got["frame_errors"]).sum(axis=2), np.asarray(got["errors"]))
    if n_bits % 8:                                                # the spare bits of the last byte are zero
        assert not (np.asarray(got["decoded"])[:, :, -1] & ((1 << (8 - n_bits % 8)) - 1)).any()


CASES = {  # kind, precision, receiver, what is set on the plan, generator arguments
    "task5-omp": ("8psk", "fp32", "task5", None),
    "task5-mmse-ls": ("8psk", "fp64", "task5", "mmse-ls"),
    "task5-register": ("8psk", "fp32", "task5", "register"),
    "task4-sto": ("8psk", "fp64", "task4", "task4"),
    "task5-fading": ("small", "fp32", "task5", "fading"),
}


def _case(ofdm, oracle, name):
    kind, precision, receiver, what = CASES[name]
    cfg, plan = _plan(ofdm, kind, precision)
    h = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)[0]
    gen_kw, t_kw, flags = dict(h=h), {}, None
    if what == "register":
        plan.set_descrambler(REG)
        gen_kw["Register"] = REG
    elif what == "task4":
        gen_kw["Time_Delay"] = 12
        t_kw, flags = dict(time_desync=1, freq_desync=0, mp_desync=1), (1, 0, 1)
    elif what == "fading":
        gen_kw = dict(fading=LINE)
    return ("task4" if what == "task4" else kind), plan, receiver, gen_kw, t_kw, flags, what == "mmse-ls"


@pytest.mark.parametrize("name", list(CASES))
def test_transport_is_its_composition(ofdm, oracle, name):
    """repeats = 3, two points, a payload of 2 frame_bits + 13 bits: decoded, errors, frame_errors and ones exactly."""
    kind, plan, receiver, gen_kw, t_kw, flags, mmse_ls = _case(ofdm, oracle, name)
    bits = _payload(2 * plan.frame_bits + 13, seed=len(name))
    snrs, seeds, frame0, repeats = SNRS[kind], [17, 23], 3, 3
    want = _compose(ofdm, plan, bits, snrs, repeats, receiver, gen_kw, seeds, frame0, flags, mmse_ls)
    if mmse_ls:
        plan.set_mmse_ls(0.0)                                     # (the transport uses each point's own SNR)
    got = plan.transport(bits, snrs, repeats=repeats, receiver=receiver, seeds=seeds, frame0=frame0, want_ones=True, want_frames=True,
                         **gen_kw, **t_kw)
    ber = want["errors"].sum() / (bits.size * repeats * len(snrs))
    print(f"{name}: errors {want['errors'].tolist()} BER {ber:.3f}")
    _assert_transport(got, want, bits.size)
    assert got["n_bits"] == bits.size and got["frames"] == 3
    assert 0.01 < ber < 0.4                                       # something to count, far from one half
    plan.close()


@pytest.mark.parametrize("kind", ["small", "8psk"])
def test_errors_are_the_receivers_own_counts_on_whole_frames(ofdm, oracle, kind):
    """With n_bits a multiple of frame_bits nothing is masked: errors is the sum of the receiver's own per-frame counts."""
    cfg, plan = _plan(ofdm, kind, "fp32")
    gen_kw = dict(h=oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)[0])
    bits = _payload(2 * plan.frame_bits, seed=2)
    want = _compose(ofdm, plan, bits, SNRS[kind], 3, "task5", gen_kw, [5, 6], 0)
    got = plan.transport(bits, SNRS[kind], repeats=3, seeds=[5, 6], want_frames=True, want_ones=True, **gen_kw)
    _assert_transport(got, want, bits.size)
    assert np.array_equal(np.asarray(got["errors"]), want["rx_errors"]) and want["rx_errors"].sum() > 0
    plan.close()


# ---- 5. loop-back
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("kind", ["small", "8psk"])
def test_loopback_on_the_clean_channel(ofdm, oracle, precision, kind):
    """3000 dB through the 3-tap channel of T3/Main_model_Task_3.m:122-126 with the Register of :36: the reference's own check."""
    cfg, plan = _plan(ofdm, kind, precision)
    plan.set_descrambler(REG)
    bits = _payload(3 * plan.frame_bits + 5, seed=9)
    h = oracle.get_MP_channel_resp(T3_TAPS, cfg.Nfft)[0]
    got = plan.transport(bits, [3000.0], repeats=2, h=h, Register=REG, want_ones=True)
    assert np.array_equal(np.asarray(got["decoded_bits"]), np.broadcast_to(bits, (1, 2, bits.size)))
    assert np.array_equal(np.asarray(got["decoded"])[0, 1], np.packbits(bits))
    assert np.asarray(got["loopback"]).all() and not np.asarray(got["errors"]).any() and not np.asarray(got["BER"]).any()
    assert np.array_equal(np.asarray(got["ones"])[0], 2 * bits.astype(np.int64))
    plan.close()


# ---- 6. chunking
@pytest.mark.parametrize("name", ["task5-register", "task4-sto"])
def test_no_output_depends_on_the_chunking(ofdm, oracle, name):
    """F = 3, repeats = 3: chunks of 1, 2 and 8 frames.  With 2 frames a chunk ends inside a repeat, and on "8psk" (frame_bits %
    32 = 12) inside an output word of the joined stream."""
    kind, plan, receiver, gen_kw, t_kw, flags, _ = _case(ofdm, oracle, name)
    bits = _payload(2 * plan.frame_bits + 13, seed=4)
    kw = dict(repeats=3, receiver=receiver, seeds=[3, 4], frame0=9, want_ones=True, want_frames=True, **gen_kw, **t_kw)
    runs = [plan.transport(bits, SNRS[kind], max_frames_per_chunk=ch, **kw) for ch in (0, 1, 2, 3 * 3 - 1)]
    assert np.asarray(runs[0]["errors"]).sum() > 0
    for other in runs[1:]:
        _same(other, runs[0])
    plan.close()


# ---- 7. edges
@pytest.mark.parametrize("kind", ["small", "8psk"])
def test_edges_of_the_stream(ofdm, oracle, kind):
    cfg, plan = _plan(ofdm, kind, "fp32")
    fb = plan.frame_bits
    gen_kw = dict(h=oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)[0])
    sizes = [1, fb, fb + 1, fb + 8 - fb % 8, fb + 9 - fb % 8, fb + 15 - fb % 8]
    assert {n % 8 for n in sizes} >= {0, 1, 7}
    for n_bits in sizes:
        bits = np.ones(n_bits, np.uint8) if n_bits == 1 else _payload(n_bits, seed=n_bits)
        want = _compose(ofdm, plan, bits, SNRS[kind][:1], 2, "task5", gen_kw, [8], 1)
        got = plan.transport(bits, SNRS[kind][:1], repeats=2, seeds=[8], frame0=1, want_frames=True, want_ones=True, **gen_kw)
        _assert_transport(got, want, n_bits)
        assert got["frames"] == pc.n_frames(n_bits, fb) and np.asarray(got["decoded"]).shape == (1, 2, (n_bits + 7) // 8)
    plan.close()


# ---- 8. refusals
def test_refusals_by_message(ofdm, oracle):
    cfg, plan = _plan(ofdm, "small", "fp32")
    h = oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)[0]
    bits = _payload(1000)

    def refused(msg, *a, **kw):
        with pytest.raises(ofdm.OfdmError) as e:
            plan.transport(*a, **kw)
        assert msg in str(e.value), str(e.value)

    refused("transport: the payload must have at least one bit (0)", np.zeros(0, np.uint8), [10.0])
    refused("transport: repeats must be at least 1 (0)", bits, [10.0], repeats=0)
    refused("leave the 32-bit stream range", bits, [10.0], repeats=2, frame0=(1 << 32) - 4)
    refused("transport: give h (one channel for every frame) or taps (a channel per frame), not both", bits, [10.0], h=h, fading=LINE)
    refused("transport: receiver 5 runs as ber_sweep_task5 does", bits, [10.0], Time_Delay=12)
    refused("transport: with the Scrambler on the plan needs a DeScrambler with the same register", bits, [10.0], Register=REG)
    refused("ber_sweep_task4: max_frames_per_chunk must be 0..65535", bits, [10.0], receiver="task4", max_frames_per_chunk=65536)
    refused('transport: receiver must be "task5" or "task4"', bits, [10.0], receiver="task3")
    refused("give payload_bits or payload_packed", None, [10.0])
    refused("payload_packed holds fewer than n_bits", None, [10.0], payload_packed=(b"\x00", 9))
    plan.set_descrambler(REG)
    refused("transport: the plan descrambles but the frames are not scrambled", bits, [10.0])
    plan.set_descrambler(None)
    plan.set_mmse(h, 10.0)
    refused("transport: an MMSE-mode plan is built for one SNR (n_points must be 1)", bits, [10.0, 12.0], h=h)
    refused("transport: an MMSE-mode plan is built for one channel h", bits, [10.0], fading=LINE)
    plan.set_mmse(None)
    with pytest.raises(ofdm.OfdmError, match="tx_frames_payload: first_frame must be 0"):
        plan.tx_frames_fused(1, payload_bits=bits, payload_frame0=-1)
    with pytest.raises(ofdm.OfdmError, match="tx_frames_payload: the payload must have at least one bit"):
        plan.tx_frames_fused(1, payload_bits=np.zeros(0, np.uint8))
    with pytest.raises(ofdm.OfdmError, match="not both"):
        plan.tx_frames_fused(1, payload_bits=bits, h=h, fading=LINE)
    # nothing was written or left behind: the next call is the usual one
    assert np.asarray(plan.transport(bits, [3000.0], h=h)["loopback"]).all()
    plan.close()


# ---- 9. the device flavour
def test_device_flavour_returns_the_same_tables(ofdm, oracle):
    import torch
    cfg, plan = _plan(ofdm, "8psk", "fp32")
    plan.set_descrambler(REG)
    bits = _payload(2 * plan.frame_bits + 13, seed=12)
    kw = dict(repeats=3, h=oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)[0], Register=REG, seeds=[1, 2], want_ones=True, want_frames=True)
    host = plan.transport(bits, SNRS["8psk"], **kw)
    for payload in (dict(payload_bits=torch.from_numpy(bits).cuda()), dict(payload_packed=(torch.from_numpy(np.packbits(bits)).cuda(), bits.size)),
                    dict(payload_bits=bits)):
        dev = plan.transport(SNRs=SNRS["8psk"], device="cuda:0", **payload, **kw)
        torch.cuda.synchronize()
        assert all(v.is_cuda for k, v in dev.items() if k not in ("n_bits", "frames"))
        _same({k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in dev.items()}, host)
    assert np.asarray(host["errors"]).sum() > 0
    plan.close()


# ---- 10. the driver
def _read_pgm(path):
    with open(path, "rb") as f:
        magic, dims, maxval = f.readline().split(), f.readline().split(), f.readline().split()
        assert magic == [b"P5"] and maxval == [b"255"]
        w, hgt = int(dims[0]), int(dims[1])
        return np.frombuffer(f.read(), np.uint8).reshape(hgt, w)


def test_send_picture_driver_equals_the_direct_call(ofdm, oracle, tmp_path):
    from ofdm_course_amd.drivers import send_picture as sp
    out, pgm = tmp_path / "out.json", tmp_path / "pgm"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "ofdm_course_amd.drivers.send_picture", "--json", str(out), "--card", "--config", "small",
                        "--snr", "8,3000", "--repeats", "2", "--pgm-dir", str(pgm)], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    res = json.loads(out.read_text())
    card = sp.test_card()
    bits = sp.image_bits(card)
    assert bits.size == 360 * 360 and res["n_bits"] == bits.size
    cfg, taps, reg = sp.link("small")
    h = oracle.get_MP_channel_resp(taps, cfg.Nfft)[0]
    from ofdm_course_amd import frames as fr
    plan = fr.make_plan(cfg, ofdm, precision="fp32", device=0)
    plan.set_descrambler(reg)
    want = plan.transport(bits, [8.0, 3000.0], repeats=2, h=h, Register=reg, seed=res["seed"], want_ones=True)
    assert res["errors"] == np.asarray(want["errors"]).tolist() and res["loopback"] == np.asarray(want["loopback"]).tolist()
    assert res["BER"] == np.asarray(want["BER"]).tolist() and res["loopback"][1] == [True, True] and res["errors"][0][0] > 0
    first, mean = _read_pgm(pgm / "snr_3000_first.pgm"), _read_pgm(pgm / "snr_3000_mean.pgm")
    assert np.array_equal(first, card * 255) and np.array_equal(mean, card * 255)            # the card, byte for byte
    noisy = _read_pgm(pgm / "snr_8_first.pgm")
    assert np.array_equal(noisy, sp.picture(np.asarray(want["decoded_bits"])[0, 0]))
    assert np.array_equal(_read_pgm(pgm / "snr_8_mean.pgm"), sp.mean_picture(np.asarray(want["ones"])[0], 2))
    plan.close()
