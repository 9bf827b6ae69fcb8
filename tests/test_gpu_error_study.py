"""RxPlan.error_study (ofdm_error_study) against the public pieces: for each point tx_frames_fused with the same arguments (the
payload and the scrambled reference bits), rx_chain_task5 / rx_chain_task4 with bits out, and the numpy twin of
tests/error_cases.py.  `errors` of side="payload" equals the matching sweep's exactly; every table is the same for
max_frames_per_chunk 0, 1 and a value that does not divide frames_per_point; with a Register, side="channel" equals the twin on the
receiver's raw decisions and side="payload" the twin on DeScrambler_frames of those decisions; the plan descrambles as before after
a side="channel" call; the refusals come in the sweeps' own words.

Cases: receiver 5 on wave-skip0-64qam and wave-skip0-qpsk-descr of tests/routes.py (fp32) and on generic-64-qpsk-descr in both
precisions; receiver 4 on n64, the smallest case of tests/t4_routes.py, with the synchroniser on, in both precisions; a fading case
on frames.config_small in fp64."""
import warnings

import numpy as np
import pytest

import error_cases as ec
import routes
import t4_cases as tc

pytestmark = pytest.mark.gpu

REG = (1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0)          # T5/Main_model_Task_5.m:55 = T3/Main_model_Task_3.m:36
FPP, CHUNKS, GAP = 5, (0, 1, 2), 16
LINE = ([0, 3, 9], [1.0, 0.5, 0.25])


def _route_plan(ofdm, oracle, name):
    from ofdm_course_amd import frames as fr
    case = next(c for c in routes.CASES if c.name == name)
    cfg = case.cfg()
    plan = fr.make_plan(cfg, ofdm, precision=case.precision, device=0)
    return plan, oracle.get_MP_channel_resp(cfg.taps, cfg.Nfft)[0], case.descr


def _t4_plan(ofdm, oracle, precision):
    case = tc.BY_NAME["n64"]
    lay = tc.layout(oracle, case)
    plan = ofdm.RxPlan(case.Nfft, case.T_guard, case.N_symb, case.N_carrier, lay["pc"], lay["dc"], lay["col"], len(lay["pc"]), 3,
                       case.const, precision=precision, device=0)
    return plan, oracle.get_MP_channel_resp(tc.channel_taps(case), case.Nfft)[0]


def _decode(ofdm, plan, receiver, rx, flags):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if receiver == "task4":
            return np.asarray(ofdm.rx_chain_task4(plan, rx, time_desync=flags[0], freq_desync=flags[1], mp_desync=flags[2])["bits"])
        return np.asarray(ofdm.rx_chain_task5(plan, rx)["bits"])


def _expected(ofdm, plan, receiver, snr, gen_kw, flags, register, side):
    """The twin's tables of one point from tx_frames_fused + the receiver + numpy; with a Register the receiver runs with the
    DeScrambler off (its raw decisions), the payload side through DeScrambler_frames."""
    gen = plan.tx_frames_fused(FPP, SNR=snr, Register=register, **gen_kw)
    rx, payload = np.asarray(gen["rx"]), np.asarray(gen["packed"])
    if register is None:
        return ec.profile(_decode(ofdm, plan, receiver, rx, flags), payload, plan.n_data, plan.N_symb, plan.bps, GAP)
    plan.set_descrambler(None)
    raw = _decode(ofdm, plan, receiver, rx, flags)
    plan.set_descrambler(register)
    if side == "channel":
        return ec.profile(raw, np.asarray(gen["sc_packed"]), plan.n_data, plan.N_symb, plan.bps, GAP)
    des = np.asarray(ofdm.DeScrambler_frames(register, ec.unpack(raw, plan.frame_bits).T)).T
    return ec.profile(ec.pack(des, plan.frame_bytes), payload, plan.n_data, plan.N_symb, plan.bps, GAP)


def _study_equals_the_pieces(ofdm, plan, receiver, snrs, study_kw, gen_kw, flags, register, sweep_errors):
    sides = ("payload", "channel") if register is not None else ("payload",)
    for side in sides:
        runs = [plan.error_study(snrs, FPP, receiver=receiver, side=side, gap_bins=GAP, want_map=True, want_frames=True,
                                 Register=register, max_frames_per_chunk=ch, **study_kw) for ch in CHUNKS]
        for other in runs[1:]:                                    # no table depends on the chunking
            for key in ec.TABLES + ("frame_errors", "map"):
                assert np.array_equal(np.asarray(other[key]), np.asarray(runs[0][key])), (side, key)
        for p, snr in enumerate(snrs):
            want = _expected(ofdm, plan, receiver, snr, gen_kw, flags, register, side)
            ec.assert_profile(runs[0], want, point=p)
        if side == "payload":
            assert np.array_equal(np.asarray(runs[0]["errors"]), np.asarray(sweep_errors))
        assert np.asarray(runs[0]["errors"]).sum() > 0             # the SNRs leave something to locate
    if register is None:                                          # without a Register both sides are the same bits
        a = plan.error_study(snrs, FPP, receiver=receiver, side="channel", gap_bins=GAP, **study_kw)
        assert all(np.array_equal(np.asarray(a[k]), np.asarray(runs[0][k])) for k in ec.TABLES)


@pytest.mark.parametrize("name", ["wave-skip0-64qam", "wave-skip0-qpsk-descr", "generic-64-qpsk-descr-fp32", "generic-64-qpsk-descr-fp64"])
def test_receiver5_against_the_pieces(ofdm, oracle, name):
    plan, h, descr = _route_plan(ofdm, oracle, name)
    register = REG if descr else None
    if descr:
        plan.set_descrambler(REG)
    snrs = [2.0, 8.0] if "qpsk" in name else [14.0, 20.0]
    kw = dict(h=h, seed=17, frame0=3)
    sweep = plan.ber_sweep(snrs, FPP, Register=register, **kw)
    _study_equals_the_pieces(ofdm, plan, "task5", snrs, kw, kw, None, register, sweep["errors"])
    if descr:                                                     # the plan descrambles as it did: the sweep's usual result
        again = plan.ber_sweep(snrs, FPP, Register=register, **kw)
        assert np.array_equal(np.asarray(again["errors"]), np.asarray(sweep["errors"]))
    plan.close()


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_receiver4_synchroniser_on_against_the_pieces(ofdm, oracle, precision):
    plan, h = _t4_plan(ofdm, oracle, precision)
    plan.set_descrambler(REG)
    snrs, flags = [6.0, 12.0], (1, 1, 1)
    gen_kw = dict(h=h, seed=29, frame0=1, Time_Delay="random", Freq_Shift="random")
    study_kw = dict(gen_kw, time_desync=1, freq_desync=1, mp_desync=1)
    sweep = plan.ber_sweep_task4(snrs, FPP, Register=REG, **study_kw)
    _study_equals_the_pieces(ofdm, plan, "task4", snrs, study_kw, gen_kw, flags, REG, sweep["errors"])
    again = plan.ber_sweep_task4(snrs, FPP, Register=REG, **study_kw)
    assert np.array_equal(np.asarray(again["errors"]), np.asarray(sweep["errors"]))
    plan.close()


def test_fading_against_the_pieces(ofdm):
    from ofdm_course_amd import frames as fr
    plan = fr.make_plan(fr.config_small(), ofdm, precision="fp64", device=0)
    snrs = [10.0, 16.0]
    kw = dict(fading=LINE, seed=41, frame0=2)
    sweep = plan.ber_sweep(snrs, FPP, **kw)
    _study_equals_the_pieces(ofdm, plan, "task5", snrs, kw, kw, None, None, sweep["errors"])
    dev = plan.error_study(snrs, FPP, gap_bins=GAP, want_map=True, want_frames=True, device=0, **kw)
    host = plan.error_study(snrs, FPP, gap_bins=GAP, want_map=True, want_frames=True, **kw)
    import torch
    torch.cuda.synchronize()
    for key in ec.TABLES + ("frame_errors", "map"):               # the device flavour: the same integers
        assert np.array_equal(dev[key].cpu().numpy().astype(np.int64), np.asarray(host[key]).astype(np.int64)), key
    plan.close()


def test_isolated_channel_errors_become_three_payload_errors(ofdm, oracle):
    """A Register and an SNR at which the channel side has isolated errors: the study's two sides against the twin on the receiver's
    raw decisions and on DeScrambler_frames of them -- taken from the per-function DeScrambler, not from the study -- with at least
    one frame whose channel error lies more than 14 bits from the frame's end, so that it spreads to i, i + 13 and i + 14.
    The SNR comes from the oracle's channel, on the CPU: Noise(SNR) scales the noise to the frame's mean power, so data carrier k
    (unit power beside Np pilots of power pilot_amp^2) sees gamma_k = |H(k)|^2 Nfft SNR / (nd + Np pilot_amp^2), a QPSK bit is wrong
    with Q(sqrt(gamma_k)), and the first SNR on a grid of 0.5 dB that expects at most two wrong bits in a frame of 2016 (8.0 dB:
    1.9) leaves them about a thousand bits apart."""
    from math import erfc, sqrt
    plan, h, _ = _route_plan(ofdm, oracle, "wave-skip0-qpsk-descr")
    plan.set_descrambler(REG)
    cfg = next(c for c in routes.CASES if c.name == "wave-skip0-qpsk-descr").cfg()
    gain = np.abs(np.fft.fft(np.asarray(h).ravel(), cfg.Nfft)[np.asarray(cfg.dataCarriers, int) - 1]) ** 2 * cfg.Nfft / \
        (len(cfg.dataCarriers) + len(cfg.pilotCarriers) * cfg.pilot_amp ** 2)
    expect = lambda s: cfg.N_symb * 2 * sum(0.5 * erfc(sqrt(g * 10 ** (s / 10) / 2)) for g in gain)
    snr = float(next(s for s in np.arange(0.0, 30.0, 0.5) if expect(s) <= 2.0))
    assert snr == 8.0
    kw = dict(h=h, seed=17, frame0=3)
    ch = plan.error_study([snr], FPP, side="channel", gap_bins=GAP, want_frames=True, Register=REG, **kw)
    pay = plan.error_study([snr], FPP, side="payload", gap_bins=GAP, want_frames=True, Register=REG, **kw)
    want_ch = _expected(ofdm, plan, "task5", snr, kw, None, REG, "channel")
    want_pay = _expected(ofdm, plan, "task5", snr, kw, None, REG, "payload")
    ec.assert_profile(ch, want_ch, point=0, emap=False)
    ec.assert_profile(pay, want_pay, point=0, emap=False)
    gen = plan.tx_frames_fused(FPP, SNR=snr, Register=REG, **kw)
    plan.set_descrambler(None)
    raw = _decode(ofdm, plan, "task5", np.asarray(gen["rx"]), None)
    plan.set_descrambler(REG)
    wrong = ec.unpack(raw, plan.frame_bits) ^ ec.unpack(np.asarray(gen["sc_packed"]), plan.frame_bits)
    spread = [f for f in range(FPP) if wrong[f].any() and np.flatnonzero(wrong[f]).max() < plan.frame_bits - 14]
    assert spread, ("no frame with a channel error more than 14 bits from its end", snr, want_ch["frame_errors"])
    assert int(np.asarray(pay["errors"])[0]) > int(np.asarray(ch["errors"])[0]) > 0, (want_pay["frame_errors"], want_ch["frame_errors"])
    plan.close()


def test_refusals_in_the_sweeps_own_words(ofdm, oracle):
    plan, h, _ = _route_plan(ofdm, oracle, "generic-64-qpsk-descr-fp32")
    needs = "with the Scrambler on the plan needs a DeScrambler with the same register"
    for receiver, what in (("task5", "ber_sweep_task5"), ("task4", "ber_sweep_task4")):
        with pytest.raises(ofdm.OfdmError, match=f"{what}: {needs}"):
            plan.error_study([10.0], 2, receiver=receiver, h=h, Register=REG)
    plan.set_descrambler(REG)
    with pytest.raises(ofdm.OfdmError, match="ber_sweep_task5: the plan descrambles but the frames are not scrambled"):
        plan.error_study([10.0], 2, h=h)
    with pytest.raises(ofdm.OfdmError, match="ber_sweep_task5: the plan descrambles but the frames are not scrambled"):
        plan.ber_sweep([10.0], 2, h=h)
    for kw in (dict(Time_Delay=3), dict(Freq_Shift=0.25), dict(time_desync=1), dict(freq_desync=1), dict(mp_desync=0)):
        with pytest.raises(ofdm.OfdmError, match="error_study: receiver 5 runs as ber_sweep_task5 does"):
            plan.error_study([10.0], 2, h=h, Register=REG, **kw)
    with pytest.raises(ofdm.OfdmError, match=r"error_study: gap_bins must be 1 \.\. 1024 \(0\)"):
        plan.error_study([10.0], 2, h=h, Register=REG, gap_bins=0)
    with pytest.raises(ofdm.OfdmError, match="ber_sweep_task4: max_frames_per_chunk must be 0..65535"):
        plan.error_study([10.0], 2, receiver="task4", h=h, Register=REG, max_frames_per_chunk=65536)
    with pytest.raises(ofdm.OfdmError, match="give h .one channel for every frame. or taps"):
        plan.error_study([10.0], 2, h=h, fading=LINE, Register=REG)
    with pytest.raises(ofdm.OfdmError, match='receiver must be "task5" or "task4"'):
        plan.error_study([10.0], 2, receiver="task3", h=h, Register=REG)
    ok = plan.error_study([10.0], 2, h=h, Register=REG)           # and the plan still descrambles after every refusal
    assert np.array_equal(np.asarray(ok["errors"]), np.asarray(plan.ber_sweep([10.0], 2, h=h, Register=REG)["errors"]))
    plan.close()
