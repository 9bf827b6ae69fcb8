"""The OMP route of an RX plan (ofdm_rx_plan_set_omp_route, RxPlan.set_omp_route): rx_chain_task5 and both Task-5 sweeps with
omp_wide_kernel as their OMP stage -- the dictionary of all Nfft delays on a random pilot mask (T5/Task5_part2.m:58-64,
:181-184), which a plan left in the default refuses ("OMP stage needs").  Cases and frames: tests/omp_route_cases.py
(oracle.tx_frame frames, tie-free by the oracle's own pursuit: tests/test_omp_route_host.py).

Rules (those of tests/test_gpu_chain_routes.py): fp64 -- picks, bits and error counts equal to the oracle's, rel_l2(H) < 1e-9;
fp32 -- rel_l2(H) < 2e-4, every pick the arg-max or a near-tie (pick_audit.py) with NO frame set aside, every differing decision
a boundary point (flip_audit.py), at most 2 * n_frames of them; MER sums with the tolerances of test_gpu_mer_task5.py.

The comb-4 case of the forced route carries K = 128, not K = Nfft: on comb pilots the atoms k and k + Nfft / comb are one and
the same column, so every pick of a larger dictionary is an exact tie and no tie-free frame exists (omp_route_cases.py)."""
import dataclasses
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import omp_route_cases as oc
from conftest import rel_l2
from flip_audit import decision_flip_audit
from pick_audit import omp_pick_audit

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _call(ofdm, case, route, mer=True):
    """One rx_chain_task5 call of the case's frames on a fresh plan set to `route` (None: left as created)."""
    from ofdm_course_amd import frames as fr
    cfg = case.cfg()
    rx, tx_bits, _ = oc.frames(case)
    plan = fr.make_plan(cfg, ofdm, precision=case.precision)
    assert plan.omp_route == "batch" and plan.last_omp_route is None
    if route is not None:
        plan.set_omp_route(route)
        assert plan.omp_route == route
    try:
        out = ofdm.rx_chain_task5(plan, rx.astype(np.complex128 if case.precision == "fp64" else np.complex64),
                                  ref_bits_packed=fr.pack_bits(tx_bits), want_h=True, want_index=True, want_mer=mer)
        res = dict(bits=fr.unpack_bits(np.asarray(out["bits"]), plan.frame_bits), packed=np.asarray(out["bits"]).copy(),
                   errors=np.asarray(out["errors"]).astype(np.int64), H=np.asarray(out["H"]).T.copy(),
                   index=np.asarray(out["index"]).T.copy(), mer=np.asarray(out["mer_sums"]).copy() if mer else None,
                   taken=plan.last_omp_route)
    finally:
        plan.close()
    return res


def _mer_sums(oracle, iq, bits01, const):
    D, bps = oracle.constellation_func(const)
    b = np.asarray(bits01, dtype=np.int64)[: iq.size * bps].reshape(iq.size, bps)
    ideal = D[b @ (1 << np.arange(bps - 1, -1, -1))]
    return np.array([np.sum(ideal.real ** 2 + ideal.imag ** 2), np.sum((ideal - iq).real ** 2 + (ideal - iq).imag ** 2)])


def _check_against_oracle(oracle, case, got):
    cfg = case.cfg()
    rx64, tx_bits, pv_col = oc.frames(case)
    nfr, f64 = case.n_frames, case.precision == "fp64"
    ref = oracle.rx_chain_task5(rx64, cfg.Nfft, cfg.T_guard, cfg.N_carrier, cfg.pilotCarriers, cfg.dataCarriers, pv_col, cfg.K,
                                cfg.dominant_taps, case.const, want_iq=True)
    assert np.array_equal(got["errors"], np.count_nonzero(got["bits"] != tx_bits, axis=1))
    idx = got["index"]
    assert idx.max() <= cfg.K and idx.min() >= 0
    if f64:
        for f in range(nfr):
            want = list(ref["index"][f])
            assert list(idx[f][: len(want)]) == want and not idx[f][len(want):].any(), (f, idx[f], want)
    else:
        Smat = oracle.sensing_matrix(cfg.pilotCarriers, cfg.Nfft, cfg.K)
        pc = np.asarray(cfg.pilotCarriers, int) - 1
        L = cfg.Nfft + cfg.T_guard
        for f in range(nfr):
            picks = [int(k) for k in idx[f] if k > 0]
            X1 = oracle.OFDM_demodulator(rx64[:L, f][:, None], cfg.T_guard)
            near, H_refit = omp_pick_audit(oracle, X1[pc, 0] / pv_col, Smat, picks, cfg.Nfft)
            assert rel_l2(got["H"][f], H_refit[:cfg.N_carrier]) < 2e-4, f
            want = list(ref["index"][f])
            assert near == 0 and picks == want and not idx[f][len(want):].any(), (f, near, picks, want)   # no frame set aside
    err_H = rel_l2(got["H"], ref["H"])
    print(f"{case.name}: rel_l2(H) {err_H:.3g}")
    assert err_H < (1e-9 if f64 else 2e-4)
    if f64:
        assert np.array_equal(got["bits"], ref["bits"])
        assert np.array_equal(got["errors"], np.count_nonzero(ref["bits"] != tx_bits, axis=1))
    else:
        flips = sum(decision_flip_audit(oracle, got["bits"][f], ref["bits"][f], ref["iq"][f], case.const,
                                        what=f"{case.name} frame {f}")[0] for f in range(nfr))
        print(f"{case.name}: {flips} boundary decisions differ from the oracle's")
        assert flips <= 2 * nfr
    n_iq = len(cfg.dataCarriers) * cfg.N_symb
    for f in range(nfr):
        want = _mer_sums(oracle, ref["iq"][f], got["bits"][f], case.const)
        g = np.asarray(got["mer"][f], dtype=np.float64)
        if f64:
            assert np.allclose(g, want, rtol=1e-9, atol=0), (f, g, want)
        else:
            assert np.all(np.abs(g - want) <= 1e-4 * np.abs(want) + 1e-6 * n_iq), (f, g, want)


# ---- 1. shapes that take the wide route by themselves
@pytest.mark.parametrize("case", oc.AUTO_4096 + oc.AUTO_2048, ids=lambda c: c.name)
def test_auto_decodes_what_the_batch_kernel_refuses(ofdm, oracle, case):
    """Fails on a library without the plan route: there these calls end with "OMP stage needs"."""
    got = _call(ofdm, case, "auto")
    assert got["taken"] == "wide"
    _check_against_oracle(oracle, case, got)


@pytest.mark.parametrize("case", oc.AUTO_4096 + oc.AUTO_2048, ids=lambda c: c.name)
def test_default_plan_still_refuses(ofdm, case):
    for route in (None, "batch"):
        with pytest.raises(ofdm.OfdmError) as e:
            _call(ofdm, case, route)
        assert "OMP stage needs" in str(e.value)


# ---- 2. the wide route forced where omp_batch_kernel also serves; 4. the split call sites
@pytest.mark.parametrize("case", oc.WIDE_512 + oc.WIDE_512_MASK + oc.WIDE_1024 + oc.SPLIT_512, ids=lambda c: c.name)
def test_forced_wide_route(ofdm, oracle, case):
    got = _call(ofdm, case, "wide")
    assert got["taken"] == "wide"
    if case.precision == "fp64":
        base = _call(ofdm, case, "batch")
        assert base["taken"] == "batch"
        assert np.array_equal(got["index"], base["index"])
        assert got["packed"].tobytes() == base["packed"].tobytes() and np.array_equal(got["errors"], base["errors"])
        d = rel_l2(got["H"], base["H"])
        print(f"{case.name}: against the batch route rel_l2(H) {d:.3g}")
        assert d < 1e-12
    _check_against_oracle(oracle, case, got)


def test_split_case_takes_the_split_entry():
    import routes
    for c in oc.SPLIT_512:
        assert routes.expected_route(c, c.precision, "omp", False, True, {}).entry == "split"
    for c in oc.WIDE_512:                                         # would take the fused front end
        assert routes.expected_route(c, c.precision, "omp", False, True, {}).front == "fused"


# ---- 3. `auto` on a plan omp_batch_kernel serves: the route it always took, bit for bit
@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_auto_is_bit_identical_where_batch_fits(ofdm, precision):
    from ofdm_course_amd import frames as fr
    cfg = fr.config_M()
    data = fr.make_frames(cfg, ofdm, 5, seed=3, precision=precision)
    outs = []
    for route in (None, "auto"):
        plan = fr.make_plan(cfg, ofdm, precision=precision)
        if route:
            plan.set_omp_route(route)
        out = ofdm.rx_chain_task5(plan, data["rx"], ref_bits_packed=data["packed"], want_h=True, want_index=True)
        assert plan.last_omp_route == "batch"
        outs.append({k: np.asarray(out[k]).copy() for k in ("bits", "errors", "H", "index")})
        plan.close()
    for k in ("bits", "errors", "H", "index"):
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k
    got = fr.unpack_bits(outs[0]["bits"], data["bits"].shape[1])
    assert np.array_equal(outs[0]["errors"].astype(np.int64), np.count_nonzero(got != data["bits"], axis=1))


# ---- 5. refusals: an argument error that names the reason, before any launch; the plan works again in `batch`
@pytest.mark.parametrize("case,fragment", oc.REFUSED, ids=lambda x: x.name if hasattr(x, "name") else None)
def test_wide_refusals_name_the_reason(ofdm, oracle, case, fragment):
    from ofdm_course_amd import frames as fr
    cfg = case.cfg()
    rx, tx_bits, _ = oc.frames(case)
    rx = rx.astype(np.complex64)
    packed = fr.pack_bits(tx_bits)
    plan = fr.make_plan(cfg, ofdm, precision="fp32")
    plan.set_omp_route("wide")
    for _ in range(2):
        with pytest.raises(ofdm.OfdmError) as e:
            ofdm.rx_chain_task5(plan, rx, ref_bits_packed=packed, want_h=True)
        assert fragment in str(e.value), str(e.value)
    with pytest.raises(ofdm.OfdmError):
        plan.set_omp_route("widest")
    plan.set_omp_route("batch")
    out = ofdm.rx_chain_task5(plan, rx, ref_bits_packed=packed, want_h=True)
    bits = fr.unpack_bits(np.asarray(out["bits"]), plan.frame_bits)
    errs = np.asarray(out["errors"]).astype(np.int64)
    assert np.array_equal(errs, np.count_nonzero(bits != tx_bits, axis=1))
    assert errs.sum() < 0.05 * tx_bits.size and np.isfinite(np.asarray(out["H"])).all()
    plan.close()


def test_mmse_modes_ignore_the_route(ofdm):
    from ofdm_course_amd import frames as fr
    case = oc.WIDE_1024[0]
    cfg = case.cfg()
    rx, tx_bits, _ = oc.frames(case)
    outs = []
    for route in ("batch", "wide"):
        plan = fr.make_plan(cfg, ofdm, precision="fp32")
        plan.set_omp_route(route)
        plan.set_mmse_ls(case.snr)
        out = ofdm.rx_chain_task5(plan, rx.astype(np.complex64), ref_bits_packed=fr.pack_bits(tx_bits), want_h=True)
        assert plan.last_omp_route is None
        outs.append((np.asarray(out["bits"]).tobytes(), np.asarray(out["H"]).tobytes()))
        plan.close()
    assert outs[0] == outs[1]


# ---- 6. the sweeps on the Nfft 4096 plan of test 1
FADING = ((0, 2, 5, 9), (1.0, 0.5, 0.25, 0.1))
SNRS, SEEDS, FPP, F0 = [24.0, 30.0], [21, 22], 4, 5


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("channel", ["static", "fading"])
def test_sweeps_equal_the_chain_call_by_call(ofdm, oracle, precision, channel):
    from ofdm_course_amd import frames as fr
    from test_gpu_fading import draw_taps, point_sum, true_nmse
    case = [c for c in oc.AUTO_4096 if c.precision == precision][0]
    cfg = case.cfg()
    plan = fr.make_plan(cfg, ofdm, precision=precision)
    plan.set_omp_route("auto")
    fad = channel == "fading"
    h, _ = ofdm.get_MP_channel_resp(cfg.taps, cfg.Nfft)
    chan = dict(fading=FADING, want_nmse=True, want_frame_nmse=True) if fad else dict(h=h)
    kw = dict(seeds=SEEDS, frame0=F0, want_frame_errors=True, want_mer=True, want_frame_mer=True, **chan)
    res = plan.ber_sweep(SNRS, FPP, **kw)
    assert plan.last_omp_route == "wide"
    fe = np.asarray(res["frame_errors"]).astype(np.int64)
    assert res["bits"] == FPP * plan.frame_bits and np.array_equal(np.asarray(res["errors"]), fe.sum(axis=1))
    for p, (snr, sd) in enumerate(zip(SNRS, SEEDS)):
        gen = plan.tx_frames_fused(FPP, SNR=snr, seed=sd, frame0=F0, **(dict(fading=FADING) if fad else dict(h=h)))
        out = ofdm.rx_chain_task5(plan, gen["rx"], ref_bits_packed=gen["packed"], want_h=True, want_mer=True)
        assert np.array_equal(fe[p], np.asarray(out["errors"]).astype(np.int64))
        assert np.array_equal(np.asarray(res["frame_mer_sums"])[p], np.asarray(out["mer_sums"]))
        assert fe[p].sum() < 0.05 * res["bits"]
        if fad:
            fn = np.asarray(res["frame_nmse"])
            amps = draw_taps(oracle, FADING[0], FADING[1], sd, F0, FPP)
            want = true_nmse(FADING[0], amps, out["H"], cfg.Nfft, cfg.N_carrier)
            print(case.name, snr, "frame_nmse rel", np.max(np.abs(fn[p] - want) / want))
            assert np.all(np.abs(fn[p] - want) <= 1e-9 * want)       # (the sum is formed in double in both precisions)
            assert np.asarray(res["nmse_sums"])[p] == point_sum(fn[p])
    # chunk invariance, bitwise
    for chunk in (1, 3):
        got = plan.ber_sweep(SNRS, FPP, max_frames_per_chunk=chunk, **kw)
        for k in ("frame_errors", "errors", "mer_sums", "frame_mer_sums") + (("nmse_sums", "frame_nmse") if fad else ()):
            assert np.asarray(got[k]).tobytes() == np.asarray(res[k]).tobytes(), (chunk, k)
    plan.close()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(cmd, out):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(out) as f:
        return json.load(f)


def test_two_rank_mask_study_equals_single_process(tmp_path):
    """drivers/task5_masks.py on two pilot counts: two gloo ranks on the one GPU against one process (fresh child processes)."""
    common = ["--profile", "EPA", "--pilots", "random", "--counts", "48", "64", "--frames", "4", "--nfft", "4096",
              "--n-carrier", "256", "--n-symb", "2", "--snr", "24", "--seed", "2"]
    mod = "ofdm_course_amd.drivers.task5_masks"
    one = _run([sys.executable, "-m", mod, *common, "--json", str(tmp_path / "one.json")], tmp_path / "one.json")
    two = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                "127.0.0.1", "--master-port", str(_free_port()), "-m", mod, *common, "--backend", "gloo", "--force-device", "0",
                "--json", str(tmp_path / "two.json")], tmp_path / "two.json")
    assert one["n_gpus"] == 1 and two["n_gpus"] == 2
    assert one["errors"] == two["errors"] and one["bits"] == two["bits"] and min(one["bits"]) > 0
    assert one["NMSE"] == two["NMSE"]                     # one addend per count: the float64 all-reduce adds zeros
    assert one["omp_route"] == two["omp_route"] == ["wide", "wide"]
    assert one["amounts_pilots"] == [48, 64] and all(np.isfinite(one["NMSE"]))
