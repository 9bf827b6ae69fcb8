"""The MMSE mode without a supplied channel (ofdm_rx_plan_set_mmse_ls) of the Task-5 receiver and its sweeps against the oracle.

Expected values, frame by frame, from the oracle's existing functions only (T5/Main_model_Task_5.m:178-180):
    H_LS = LS_CE(X, Xp, pilots, Nc);  H = MMSE_CE(X, Xp, pilots, Nfft, Nc, ifft(H_LS), snr)
then equalize_signal -> get_payload -> demapping [-> DeScrambler], as oracle.rx_chain_task5 does with OMP.  The frames are
oracle.tx_frame on Philox draws (routes.oracle_frames), the geometries the smallest at which each path of the stage can go wrong.

Rules.  fp64: rel_l2(H) < 1e-9 (the fixed-h MMSE chain test's bound), bits and error counts equal.  fp32: every
differing decision within 1e-4 level spacings of a decision boundary in the oracle's arithmetic (flip_audit.py, the distance the
fp32 MMSE chain tests use), and rel_l2(H) < H_BOUND_F32.

H_BOUND_F32 comes from the oracle alone (`python tests/test_gpu_mmse_ls.py` prints it, CPU only): the composition in double
against the same composition with the pilot LS values rounded to float32 is the input-rounding floor of a case; the bound is
8 x the largest floor over the fp32 cases.  Measured floors: fast-512 2.36e-08, wave-2048 2.20e-08, np50 2.21e-08,
front-8192 2.22e-08, one-tap 1.02e-08, fast-512-descr 2.32e-08, wave-2048-mer 2.20e-08 -> largest 2.36e-08, bound 1.89e-07.
"""
import numpy as np
import pytest

import routes
from conftest import rel_l2
from flip_audit import decision_flip_audit
from routes import REG, T3, Case

pytestmark = pytest.mark.gpu

H_BOUND_F64 = 1e-9
FLOOR_F32 = 2.36e-8             # the largest input-rounding floor over the fp32 cases (header)
H_BOUND_F32 = 8 * FLOOR_F32

CASES = [
    # frame count no multiple of the frames per workgroup (4)
    Case("fast-512", 512, 128, 4, "16QAM", 3, T3, precision="fp32", n_frames=5),
    Case("fast-512", 512, 128, 4, "16QAM", 3, T3, precision="fp64", n_frames=5),
    # the benchmark geometry's route: one wavefront per frame in the symbol stage
    Case("wave-2048", 2048, 512, 4, "64QAM", 3, T3, precision="fp32", n_frames=7),
    # Np = 50: no multiple of 4 (scalar forms, band tail), fewer pilots than lanes
    Case("np50", 1024, 400, 8, "16QAM", 3, T3, precision="fp32"),
    Case("np50", 1024, 400, 8, "16QAM", 3, T3, precision="fp64"),
    # Nfft below the fast path: the split form
    Case("split-256", 256, 100, 4, "16QAM", 3, T3, precision="fp64"),
    # the large-Nfft front end
    Case("front-8192", 8192, 600, 8, "16QAM", 2, T3, precision="fp32", n_frames=3),
    # interpolate operator with an appended end pilot and an uneven last knot spacing
    Case("percent", 2048, 800, 4, "16QAM", 3, T3, precision="fp64", pilots=("percent", 15, 2), n_frames=3),
    # degenerate delay spread: one tap, 60 dB -- r2 - r^2 is the noise's alone
    Case("one-tap", 512, 128, 4, "16QAM", 3, (0,), precision="fp32", snr=60.0, n_frames=3),
    Case("one-tap", 512, 128, 4, "16QAM", 3, (0,), precision="fp64", snr=60.0, n_frames=3),
    # DeScrambler (the pass over the packed decisions) and MER (the variadic MER variants)
    Case("fast-512-descr", 512, 128, 4, "16QAM", 3, T3, precision="fp32", descr=True, n_frames=5),
    Case("fast-512-descr", 512, 128, 4, "16QAM", 3, T3, precision="fp64", descr=True, n_frames=5),
    Case("wave-2048-mer", 2048, 512, 4, "64QAM", 3, T3, precision="fp32", mer=True, n_frames=7),
    Case("fast-512-mer", 512, 128, 4, "16QAM", 3, T3, precision="fp64", mer=True, n_frames=5),
]

_REF = {}


def compose(oracle, X, pv, pilots, nfft, nc, snr, round32=False):
    """Main_model_Task_5.m:178-180 on one demodulated frame; round32: the pilot LS values rounded to float32 first."""
    if round32:
        pc0 = np.asarray(pilots, int) - 1
        y = (X[pc0, 0] / pv[:, 0]).astype(np.complex64).astype(np.complex128)
        X = X.copy()
        X[pc0, 0] = y
        pv = np.ones_like(pv)
    H_LS = oracle.LS_CE(X, pv, pilots, nc)
    return oracle.MMSE_CE(X, pv, pilots, nfft, nc, np.fft.ifft(H_LS), snr)[0]


def reference(oracle, case, snr=None, rx=None, key=None):
    """The oracle's side of a case (computed once): frames, H, the equalised payload, the decisions."""
    key = key or (case.name, case.precision)
    if key in _REF:
        return _REF[key]
    from ofdm_course_amd import frames as fr
    tx_bits = None
    if rx is None:
        rx, tx_bits, _ = routes.oracle_frames(case, oracle)
        rx = rx.astype(np.complex128 if case.precision == "fp64" else np.complex64)
    snr = case.snr if snr is None else snr
    pc, dc = case.pilot_carriers().astype(np.float64), case.data_carriers().astype(np.float64)
    D, _ = oracle.constellation_func(case.const)
    amp = 2.0 * np.max(np.abs(D))                                          # frames.pilot_column
    pv = np.repeat(np.where(np.arange(pc.size) % 2 == 0, amp, -amp).astype(np.complex128)[:, None], case.n_symb, axis=1)
    tg, nfr = case.nfft // 8, rx.shape[1]
    rx64 = rx.astype(np.complex128)
    H = np.zeros((nfr, case.nc), dtype=np.complex128)
    iq = np.zeros((nfr, dc.size * case.n_symb), dtype=np.complex128)
    raw, floor_num, floor_den = [], 0.0, 0.0
    for f in range(nfr):
        X = oracle.OFDM_demodulator(rx64[:, f].reshape((case.nfft + tg, case.n_symb), order="F"), tg)
        H[f] = compose(oracle, X, pv, pc, case.nfft, case.nc, snr)
        if case.precision == "fp32":
            d = compose(oracle, X, pv, pc, case.nfft, case.nc, snr, round32=True) - H[f]
            floor_num += np.sum(np.abs(d) ** 2)
            floor_den += np.sum(np.abs(H[f]) ** 2)
        iq[f] = oracle.get_payload(oracle.equalize_signal(X, H[f], case.nc), dc).ravel(order="F")
        raw.append(np.asarray(oracle.demapping(0, iq[f], case.const)).ravel())
    raw = np.stack(raw)
    bits = np.stack([oracle.DeScrambler_fast(REG, raw[f])[0] for f in range(nfr)]) if case.descr else raw
    ref = dict(rx=rx, tx_bits=tx_bits, packed=None if tx_bits is None else fr.pack_bits(tx_bits), H=H, iq=iq, raw=raw, bits=bits,
               floor=float(np.sqrt(floor_num / floor_den)) if floor_den else None)
    _REF[key] = ref
    return ref


def _plan(ofdm, case, snr=None):
    from ofdm_course_amd import frames as fr
    plan = fr.make_plan(case.cfg(), ofdm, precision=case.precision)
    plan.set_mmse_ls(case.snr if snr is None else snr)
    if case.descr:
        plan.set_descrambler(REG)
    return plan


def _mer_sums(oracle, iq, raw_bits01, const):
    D, bps = oracle.constellation_func(const)
    b = np.asarray(raw_bits01, dtype=np.int64)[: iq.size * bps].reshape(iq.size, bps)
    ideal = D[b @ (1 << np.arange(bps - 1, -1, -1))]
    return np.array([np.sum(ideal.real ** 2 + ideal.imag ** 2), np.sum((ideal - iq).real ** 2 + (ideal - iq).imag ** 2)])


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c.name}-{c.precision}")
def test_chain_matches_the_oracle_composition(ofdm, oracle, case):
    from ofdm_course_amd import frames as fr
    ref = reference(oracle, case)
    f64, nfr = case.precision == "fp64", case.n_frames
    plan = _plan(ofdm, case)
    kw = dict(ref_bits_packed=ref["packed"], want_h=True, want_mer=case.mer)
    out = ofdm.rx_chain_task5(plan, ref["rx"], **kw)
    again = ofdm.rx_chain_task5(plan, ref["rx"], **kw)
    H = np.asarray(out["H"]).T
    bits = fr.unpack_bits(np.asarray(out["bits"]), plan.frame_bits)
    errors = np.asarray(out["errors"]).astype(np.int64)
    # determinism: the same call twice, bitwise
    assert np.asarray(again["H"]).tobytes() == np.asarray(out["H"]).tobytes()
    assert np.asarray(again["bits"]).tobytes() == np.asarray(out["bits"]).tobytes()
    assert np.array_equal(np.asarray(again["errors"]), np.asarray(out["errors"]))
    if case.mer:
        assert np.asarray(again["mer_sums"]).tobytes() == np.asarray(out["mer_sums"]).tobytes()
    # always: H finite, the counter is the popcount of the call's own bits
    assert np.isfinite(H.view(np.float64 if f64 else np.float32)).all()
    assert np.array_equal(errors, np.count_nonzero(bits != ref["tx_bits"], axis=1))
    err_H = rel_l2(H, ref["H"])
    print(f"{case.name} {case.precision}: rel_l2(H) {err_H:.3g} (floor {ref['floor']}, bound {H_BOUND_F64 if f64 else H_BOUND_F32:.3g})")
    raw_got = np.stack([oracle.Scrambler_fast(REG, bits[f])[0] for f in range(nfr)]) if case.descr else bits
    if f64:
        assert err_H < H_BOUND_F64
        assert np.array_equal(bits, ref["bits"])
        assert np.array_equal(errors, np.count_nonzero(ref["bits"] != ref["tx_bits"], axis=1))
    else:
        assert ref["floor"] <= FLOOR_F32 * 1.005, (case.name, ref["floor"])      # the header's figure is this case's
        flips, worst = 0, 0.0
        for f in range(nfr):
            n, w = decision_flip_audit(oracle, raw_got[f], ref["raw"][f], ref["iq"][f], case.const, what=f"{case.name} frame {f}")
            flips, worst = flips + n, max(worst, w)
        print(f"{case.name}: {flips} boundary decisions differ from the oracle's (largest distance {worst:.3g})")
        assert err_H < H_BOUND_F32
    if case.mer:
        n_iq = ref["iq"].shape[1]
        dc = case.data_carriers().astype(np.float64)
        tg = case.nfft // 8
        for f in range(nfr):
            if f64:
                z = ref["iq"][f]
            else:               # RX_IQ of the estimate the call returned (test_gpu_mer_task5.py), itself checked above
                X = oracle.OFDM_demodulator(ref["rx"][:, f].astype(np.complex128).reshape((case.nfft + tg, case.n_symb), order="F"), tg)
                z = oracle.get_payload(oracle.equalize_signal(X, H[f].astype(np.complex128), case.nc), dc).ravel(order="F")
            got, want = np.asarray(out["mer_sums"])[f].astype(np.float64), _mer_sums(oracle, z, raw_got[f], case.const)
            print(f"{case.name} frame {f}: MER sums {got} (oracle {want})")
            if f64:
                assert np.allclose(got, want, rtol=1e-9, atol=0)
            else:
                assert np.all(np.abs(got - want) <= 1e-4 * np.abs(want) + 1e-6 * n_iq)
    plan.close()


def test_modes_exclude_each_other_and_the_generic_entry_refuses(ofdm, oracle, monkeypatch):
    from ofdm_course_amd import frames as fr
    case = CASES[1]                                                        # fast-512 fp64
    ref = reference(oracle, case)
    cfg = case.cfg()
    plan = fr.make_plan(cfg, ofdm, precision="fp64")
    omp = ofdm.rx_chain_task5(plan, ref["rx"], ref_bits_packed=ref["packed"], want_h=True, want_index=True)
    h, _ = ofdm.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    hh = np.zeros(cfg.N_carrier, dtype=np.complex128)
    hh[: len(h)] = h
    plan.set_mmse(hh, case.snr)
    fixed = np.asarray(ofdm.rx_chain_task5(plan, ref["rx"], want_h=True)["H"]).copy()
    plan.set_mmse_ls(case.snr)                                             # clears the fixed-h operator
    ls = np.asarray(ofdm.rx_chain_task5(plan, ref["rx"], want_h=True)["H"]).copy()
    assert rel_l2(ls.T, ref["H"]) < H_BOUND_F64 and rel_l2(ls, fixed) > 1e-6
    out = plan.ber_sweep([10.0, 20.0], 4, h=h, seed=3)                     # more than one point: not the fixed-h mode
    assert len(out["errors"]) == 2
    plan.set_mmse(hh, case.snr)                                            # clears the LS mode
    assert np.asarray(ofdm.rx_chain_task5(plan, ref["rx"], want_h=True)["H"]).tobytes() == fixed.tobytes()
    with pytest.raises(ofdm.OfdmError, match="built for one SNR"):
        plan.ber_sweep([10.0, 20.0], 4, h=h, seed=3)
    with pytest.raises(ofdm.OfdmError, match="built for one channel h"):
        plan.ber_sweep([20.0], 4, fading=((0, 3, 7), (1.0, 0.36, 0.09)), seed=3)
    plan.set_mmse_ls(case.snr)
    plan.set_mmse(None)                                                    # h = NULL: OMP mode, whichever MMSE mode was on
    back = ofdm.rx_chain_task5(plan, ref["rx"], ref_bits_packed=ref["packed"], want_h=True, want_index=True)
    assert np.asarray(back["H"]).tobytes() == np.asarray(omp["H"]).tobytes()
    assert np.array_equal(np.asarray(back["index"]), np.asarray(omp["index"]))
    plan.set_mmse_ls(case.snr)
    plan.set_mmse_ls(None)                                                 # enable = 0: OMP mode
    back = ofdm.rx_chain_task5(plan, ref["rx"], ref_bits_packed=ref["packed"], want_h=True)
    assert np.asarray(back["H"]).tobytes() == np.asarray(omp["H"]).tobytes()
    # the generic single-kernel entry refuses the mode with the wording of the fixed-h refusal
    plan.set_mmse_ls(case.snr)
    monkeypatch.setenv("OFDM_CHAIN_GENERIC", "1")
    with pytest.raises(ofdm.OfdmError, match="the MMSE mode of a plan needs pilots inside"):
        ofdm.rx_chain_task5(plan, ref["rx"], want_h=True)
    monkeypatch.delenv("OFDM_CHAIN_GENERIC")
    assert np.asarray(ofdm.rx_chain_task5(plan, ref["rx"], want_h=True)["H"]).tobytes() == ls.tobytes()
    plan.close()


SWEEP_SNRS, SWEEP_SEEDS, SWEEP_FPP = [10.0, 20.0, 30.0], [21, 22, 23], 6


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_sweep_points_use_their_own_snr(ofdm, oracle, precision):
    """A 3-point sweep = three 1-point sweeps bit for bit = the same sweep in chunks of 4; fp64: its errors are those of the
    oracle composition on tx_frames_fused's frames, each point at its own SNR."""
    from ofdm_course_amd import frames as fr
    case = Case("fast-512", 512, 128, 4, "16QAM", 3, T3, precision=precision)
    cfg = case.cfg()
    plan = _plan(ofdm, case, snr=-5.0)                                     # the plan's own SNR is not what a sweep uses
    h, _ = ofdm.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    kw = dict(h=h, frame0=5, want_frame_errors=True, want_mer=True, want_frame_mer=True)
    base = plan.ber_sweep(SWEEP_SNRS, SWEEP_FPP, seeds=SWEEP_SEEDS, **kw)
    keys = ("errors", "frame_errors", "mer_sums", "frame_mer_sums")
    for variant in (dict(max_frames_per_chunk=4), dict(max_frames_per_chunk=0), dict()):
        got = plan.ber_sweep(SWEEP_SNRS, SWEEP_FPP, seeds=SWEEP_SEEDS, **kw, **variant)
        for k in keys:
            assert np.asarray(got[k]).tobytes() == np.asarray(base[k]).tobytes(), (variant, k)
    for p in range(3):
        one = plan.ber_sweep([SWEEP_SNRS[p]], SWEEP_FPP, seeds=[SWEEP_SEEDS[p]], **kw)
        for k in keys:
            assert np.asarray(one[k])[0].tobytes() == np.asarray(base[k])[p].tobytes(), (p, k)
    assert len(set(np.asarray(base["errors"]).tolist())) > 1               # the points differ
    for p in range(3):
        gen = plan.tx_frames_fused(SWEEP_FPP, h=h, SNR=SWEEP_SNRS[p], seed=SWEEP_SEEDS[p], frame0=5)
        # the chain at the point's SNR: what the sweep ran
        plan.set_mmse_ls(SWEEP_SNRS[p])
        out = ofdm.rx_chain_task5(plan, gen["rx"], ref_bits_packed=gen["packed"], want_mer=True)
        assert np.array_equal(np.asarray(out["errors"]).astype(np.int64), np.asarray(base["frame_errors"])[p].astype(np.int64))
        # the MER sums move with every change of H, hence of 1 / snr: bitwise those of the chain at the point's SNR, and not
        # those of the chain at a neighbouring point's
        fm = np.asarray(base["frame_mer_sums"])[p]
        assert np.ascontiguousarray(np.asarray(out["mer_sums"])).tobytes() == np.ascontiguousarray(fm).tobytes()
        plan.set_mmse_ls(SWEEP_SNRS[(p + 1) % 3])
        other = ofdm.rx_chain_task5(plan, gen["rx"], ref_bits_packed=gen["packed"], want_mer=True)
        assert not np.array_equal(np.asarray(other["mer_sums"]), fm)
        if precision == "fp64":
            ref = reference(oracle, case, snr=SWEEP_SNRS[p], rx=np.asarray(gen["rx"]), key=("sweep", p))
            tx = fr.unpack_bits(np.asarray(gen["packed"]), plan.frame_bits)
            want = np.count_nonzero(ref["bits"] != tx, axis=1)
            print("point", p, "errors", np.asarray(base["frame_errors"])[p], "oracle", want)
            assert np.array_equal(np.asarray(base["frame_errors"])[p].astype(np.int64), want)
    plan.close()


def test_fading_sweep_nmse(ofdm, oracle):
    """EPA (drivers/common.py:fading_profile at 30.72e6 samples/s), 2 points, 5 frames: frame_nmse against fft(h_f) - H_oracle from
    taps_out (test_gpu_fading.py's check and tolerance), nmse_sums = the fixed-order sum."""
    from ofdm_course_amd.drivers.common import fading_profile
    from test_gpu_fading import draw_taps, point_sum, true_nmse
    prof = fading_profile("EPA", 30.72e6)
    EPA = (tuple(int(d) for d in prof[0]), tuple(float(x) for x in prof[1]))
    case = Case("fading-512", 512, 128, 4, "16QAM", 3, T3, precision="fp64")
    cfg = case.cfg()
    plan = _plan(ofdm, case)
    snrs, seeds, fpp, f0 = [15.0, 25.0], [31, 32], 5, 2
    res = plan.ber_sweep(snrs, fpp, fading=EPA, seeds=seeds, frame0=f0, want_frame_errors=True, want_nmse=True, want_frame_nmse=True)
    fn = np.asarray(res["frame_nmse"])
    for chunk in (4, 0):
        got = plan.ber_sweep(snrs, fpp, fading=EPA, seeds=seeds, frame0=f0, want_frame_errors=True, want_nmse=True,
                             want_frame_nmse=True, max_frames_per_chunk=chunk)
        for k in ("errors", "frame_errors", "nmse_sums", "frame_nmse"):
            assert np.asarray(got[k]).tobytes() == np.asarray(res[k]).tobytes(), (chunk, k)
    for p, (snr, sd) in enumerate(zip(snrs, seeds)):
        gen = plan.tx_frames_fused(fpp, fading=EPA, SNR=snr, seed=sd, frame0=f0, want_taps=True)
        amps = np.asarray(gen["taps"])
        assert np.max(np.abs(amps - draw_taps(oracle, EPA[0], EPA[1], sd, f0, fpp))) <= 1e-13
        ref = reference(oracle, case, snr=snr, rx=np.asarray(gen["rx"]), key=("fading", p))
        want = true_nmse(EPA[0], amps, ref["H"].T, cfg.Nfft, cfg.N_carrier)
        print("fading point", p, "frame_nmse rel", np.max(np.abs(fn[p] - want) / want))
        assert np.all(np.abs(fn[p] - want) <= 1e-8 * want)                 # (test_gpu_fading.py: against the oracle's receiver)
        assert np.asarray(res["nmse_sums"])[p] == point_sum(fn[p])
    plan.close()


if __name__ == "__main__":                                                  # the input-rounding floors of the header (CPU only)
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import ofdm_oracle
    floors = {c.name: reference(ofdm_oracle, c)["floor"] for c in CASES if c.precision == "fp32"}
    for k, v in floors.items():
        print(f"{k} {v:.3g}")
    print(f"largest {max(floors.values()):.3g}, bound {8 * max(floors.values()):.3g}")
