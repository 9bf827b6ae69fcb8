"""ofdm_task5_part2_tile and ofdm_task5_mse_tile (csrc/ofdm_part2.hip) per realisation and across workgroup bounds: every slot of
nmse[4, F] / errors[4, F] against the oracle's replay of the same realisation (tests/part2_tile_cases.py; the drivers compare
sums only), at tile sizes that put a full workgroup in front of a ragged one for every split of the realisations, and at the
shapes that reach each kernel variant.  The tolerances are those of tests/test_gpu_part2_tile.py and
test_task5_sweep_tile_equals_oracle_and_call_by_call, applied per realisation / per point.  What makes them meaningful (the
realisations can be told apart, the oracle's decisions are clear of ties): tests/test_part2_tile_cases_host.py."""
import ctypes as C

import numpy as np
import pytest

import part2_tile_cases as tc

pytestmark = pytest.mark.gpu

FP64_TOL = dict(rtol=1e-9, atol=1e-12)
FP32_TOL = dict(rtol=2e-3, atol=1e-6)


def _cdt(precision):
    return np.complex128 if precision == "fp64" else np.complex64


def _inputs(oracle, case):
    from ofdm_course_amd import frames as fr
    b = tc.build_tile(oracle, case)
    b["ref"] = fr.pack_bits(np.asarray(b["bits"])[None, :])[0]
    return b


def _plan(ofdm, case, b, precision):
    return ofdm.RxPlan(case.nfft, case.t_guard, tc.N_SYMB, case.n_carrier, b["pc"], b["dc"], b["pilotValues"][:, 0], case.K,
                       case.paths, tc.CONSTELLATION, precision=precision)


def _tile(ofdm, plan, b, taps_list):
    out = ofdm.task5_part2_tile(plan, b["Tx_noised"].astype(_cdt("fp64" if plan.f64 else "fp32")), taps_list, tc.SNR_DB, b["ref"])
    return np.asarray(out["nmse"]).copy(), np.asarray(out["errors"]).astype(np.int64)


def _fresh(ofdm, case, b, precision, taps_list):
    plan = _plan(ofdm, case, b, precision)
    r = _tile(ofdm, plan, b, taps_list)
    plan.close()
    return r


@pytest.fixture(scope="module")
def inputs(oracle):
    cache = {}

    def get(case):
        if case.name not in cache:
            cache[case.name] = _inputs(oracle, case)
        return cache[case.name]
    return get


@pytest.fixture(scope="module")
def runs(ofdm, inputs):
    """(nmse [4, F], errors [4, F]) of the full tile of a case on a fresh plan, computed once per (case, precision)."""
    cache = {}

    def get(case, precision):
        if (case.name, precision) not in cache:
            b = inputs(case)
            cache[case.name, precision] = _fresh(ofdm, case, b, precision, b["taps_list"])
        return cache[case.name, precision]
    return get


def _same(a, b):
    return np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1], b[1])


FP64_RUNS = [(c, F) for c in tc.TILE_CASES if "fp64" in c.precisions for F in c.F]


@pytest.mark.parametrize("case,F", FP64_RUNS, ids=[f"{c.name}-F{F}" for c, F in FP64_RUNS])
def test_every_realisation_equals_the_oracle_fp64(ofdm, oracle, inputs, runs, case, F):
    """Bit errors of every realisation and estimator identical to the oracle's, NMSE to 1e-9."""
    b = inputs(case)
    nmse, errors = runs(case, "fp64") if F == case.F[0] else _fresh(ofdm, case, b, "fp64", b["taps_list"][:F])
    want_nmse, want_errors = tc.oracle_tile(oracle, case, F)
    assert nmse.shape == errors.shape == (4, F)
    print(case.name, F, "largest relative NMSE deviation per estimator", np.max(np.abs(nmse - want_nmse) / want_nmse, axis=1),
          "realisations with other bit errors", np.flatnonzero(np.any(errors != want_errors, axis=0)).tolist())
    assert np.array_equal(errors, want_errors), (errors - want_errors)
    assert np.allclose(nmse, want_nmse, **FP64_TOL)


def _check_fp32(name, got, full, F):
    nmse, errors = got
    want_nmse, want_errors, bits = full["nmse"][:, :F], full["errors"][:, :F], full["bits"]
    ok = ~tc.fp32_loose(full)[:F]
    print(name, "fp32: largest relative NMSE deviation per estimator", np.max(np.abs(nmse - want_nmse) / want_nmse, axis=1),
          "largest bit-error difference", np.max(np.abs(errors - want_errors), axis=1), "of", bits, "loose", np.flatnonzero(~ok).tolist())
    assert nmse.shape == errors.shape == (4, F)
    assert np.all(np.isfinite(nmse)) and np.all((errors >= 0) & (errors <= bits))
    assert np.allclose(nmse[:, ok], want_nmse[:, ok], **FP32_TOL)
    assert np.all(np.abs(errors[:, ok] - want_errors[:, ok]) <= 0.005 * bits + 8)


FP32_CASES = [c for c in tc.TILE_CASES if "fp32" in c.precisions]


@pytest.mark.parametrize("case", FP32_CASES, ids=[c.name for c in FP32_CASES])
def test_every_realisation_equals_the_oracle_fp32(oracle, runs, case):
    _check_fp32(case.name, runs(case, "fp32"), tc.oracle_tile_full(oracle, case), case.F[0])


MFMA_CASES = [tc.TILE[n] for n in ("A", "B", "D", "E", "F")]


@pytest.mark.parametrize("case", MFMA_CASES, ids=[c.name for c in MFMA_CASES])
def test_matrix_core_mp_equals_scalar_mp_fp32(ofdm, oracle, inputs, runs, case, monkeypatch):
    """OFDM_MP_NO_MFMA=1: the MP row of every realisation agrees with the matrix-core run (NMSE 1e-3 relative + 1e-6, bit errors
    within 8) -- 2, 3, 10, 20 and 36 tiles, FB 16, 8 and 4."""
    assert case.tiles > 0
    nmse, errors = runs(case, "fp32")
    monkeypatch.setenv("OFDM_MP_NO_MFMA", "1")
    b = inputs(case)
    s_nmse, s_errors = _fresh(ofdm, case, b, "fp32", b["taps_list"])
    ok = ~tc.fp32_loose(tc.oracle_tile_full(oracle, case))
    print(case.name, "MP row, scalar against MFMA: NMSE", np.max(np.abs(s_nmse[2] - nmse[2]) / nmse[2]), "bit errors",
          np.max(np.abs(s_errors[2] - errors[2])))
    assert np.allclose(s_nmse[2][ok], nmse[2][ok], rtol=1e-3, atol=1e-6)
    assert np.all(np.abs(s_errors[2][ok] - errors[2][ok]) <= 8)
    assert np.all(np.isfinite(s_nmse))


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_a_realisation_does_not_depend_on_its_slot(ofdm, inputs, runs, precision):
    """Case A: the first 5 realisations of the 37-tile are bit-identical to a tile of those 5 alone, realisations 16..36 to a
    tile of that slice (there they sit in slots 0..20 instead of behind a full MP workgroup)."""
    case = tc.TILE["A"]
    b = inputs(case)
    nmse, errors = runs(case, precision)
    for sl in (slice(0, 5), slice(16, 37)):
        part = _fresh(ofdm, case, b, precision, b["taps_list"][sl])
        assert _same(part, (nmse[:, sl], errors[:, sl])), sl


@pytest.fixture(scope="module")
def mse_inputs(oracle):
    return {c.name: tc.build_mse(oracle, c) for c in tc.MSE_CASES}


def _mse_plan(ofdm, case, b, precision):
    return ofdm.RxPlan(case.nfft, case.t_guard, tc.N_SYMB, case.n_carrier, b["pc"], b["dc"], b["pilotValues"][:, 0], case.K,
                       len(case.channel_taps), tc.CONSTELLATION, precision=precision)


def _mse(ofdm, plan, case, Tx, lo=0, hi=None):
    snrs = np.array(case.snrs)[lo:hi]
    return np.asarray(ofdm.task5_mse_tile(plan, Tx.astype(_cdt("fp64" if plan.f64 else "fp32")), case.taps(), snrs, seed=case.seed,
                                          stream0=case.stream0 + lo)).copy()


MSE_RUNS = [(c, p) for c in tc.MSE_CASES for p in c.precisions]


@pytest.mark.parametrize("case,precision", MSE_RUNS, ids=[f"{c.name}-{p}" for c, p in MSE_RUNS])
def test_every_point_of_the_mse_tile_equals_the_oracle(ofdm, oracle, mse_inputs, case, precision):
    """Per SNR point and estimator: fp64 to 1e-9, fp32 to 2e-3 (M1: 37 points across every workgroup bound, each at its own
    SNR; M2: one wavefront per workgroup in the MMSE stage, 80 tiles, N_carrier 1280; M3: a repeated delay and one beyond
    N_carrier)."""
    b = mse_inputs[case.name]
    plan = _mse_plan(ofdm, case, b, precision)
    got = _mse(ofdm, plan, case, b["Tx"])
    want = tc.oracle_mse_tile(oracle, case)
    print(case.name, precision, "largest relative deviation per estimator", np.max(np.abs(got - want) / want, axis=1))
    assert got.shape == want.shape == (4, len(case.snrs))
    np.testing.assert_allclose(got, want, rtol=1e-9 if precision == "fp64" else 2e-3)
    if case.name == "M1":
        parts = np.concatenate([_mse(ofdm, plan, case, b["Tx"], 0, 20), _mse(ofdm, plan, case, b["Tx"], 20, 37)], axis=1)
        assert np.array_equal(parts.view(np.uint64), got.view(np.uint64))
    plan.close()


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_results_survive_the_growth_of_the_shared_arena(ofdm, inputs, runs, precision):
    """One plan: A with F = 1, F = 37, F = 1, the MSE tile of M1's points on A's clean frame, F = 37 again -- the arena the two
    tiles share with the Task-4 receiver grows twice on the way.  Every result is bit-identical to the same call on a fresh
    plan."""
    case, m1 = tc.TILE["A"], tc.MSE["M1"]
    b = inputs(case)
    full = runs(case, precision)
    one = _fresh(ofdm, case, b, precision, b["taps_list"][:1])
    fresh = _plan(ofdm, case, b, precision)
    mse = _mse(ofdm, fresh, m1, b["Tx"])
    fresh.close()
    plan = _plan(ofdm, case, b, precision)
    assert _same(_tile(ofdm, plan, b, b["taps_list"][:1]), one)
    assert _same(_tile(ofdm, plan, b, b["taps_list"]), full)
    assert _same(_tile(ofdm, plan, b, b["taps_list"][:1]), one)
    assert np.array_equal(_mse(ofdm, plan, m1, b["Tx"]).view(np.uint64), mse.view(np.uint64))
    assert _same(_tile(ofdm, plan, b, b["taps_list"]), full)
    plan.close()
    assert np.all(np.isfinite(mse)) and np.all(mse > 0)


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_device_flavour_on_a_side_stream(ofdm, inputs, runs, mse_inputs, precision):
    """torch.cuda inputs on a stream that is not the default one: device tensors come back, equal to the host flavour's."""
    import torch
    case, m1 = tc.TILE["A"], tc.MSE["M1"]
    b, mb = inputs(case), mse_inputs["M1"]
    plan, mplan = _plan(ofdm, case, b, precision), _mse_plan(ofdm, m1, mb, precision)
    want_mse = _mse(ofdm, mplan, m1, mb["Tx"])
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        tx = torch.from_numpy(b["Tx_noised"].astype(_cdt(precision))).cuda()
        out = ofdm.task5_part2_tile(plan, tx, b["taps_list"], tc.SNR_DB, torch.from_numpy(b["ref"].copy()).cuda())
        assert out["nmse"].is_cuda and out["errors"].is_cuda and tuple(out["nmse"].shape) == tuple(out["errors"].shape) == (4, 37)
        got = out["nmse"].cpu().numpy().copy(), out["errors"].cpu().numpy().astype(np.int64)
        ms = ofdm.task5_mse_tile(mplan, torch.from_numpy(mb["Tx"].astype(_cdt(precision))).cuda(), m1.taps(), np.array(m1.snrs),
                                 seed=m1.seed, stream0=m1.stream0)
        assert ms.is_cuda and tuple(ms.shape) == (4, 37)
        got_mse = ms.cpu().numpy().copy()
    plan.close()
    mplan.close()
    assert _same(got, runs(case, precision))
    assert np.array_equal(got_mse.view(np.uint64), want_mse.view(np.uint64))


def test_pilot_bound_of_the_mmse_stage(ofdm, oracle):
    """586 pilots are refused with the entry's message, 585 are served (fp32, the scalar MP: 585 is odd) and equal the oracle."""
    case = tc.BOUND_REFUSED
    b = _inputs(oracle, case)
    plan = _plan(ofdm, case, b, "fp32")
    with pytest.raises(ofdm.OfdmError, match="at most 585 pilots"):
        _tile(ofdm, plan, b, b["taps_list"])
    plan.close()
    case = tc.BOUND_SERVED
    b = _inputs(oracle, case)
    _check_fp32(case.name, _fresh(ofdm, case, b, "fp32", b["taps_list"]), tc.oracle_tile_full(oracle, case), 2)


def test_refusals_leave_the_plan_usable(ofdm, inputs, runs):
    """Every refusal carries the entry's own message, and the plan serves the next valid call with unchanged results."""
    from ofdm_course_amd import _lib as L
    case = tc.TILE["A"]
    b = inputs(case)
    taps = b["taps_list"][:5]
    full = runs(case, "fp64")
    want = full[0][:, :5], full[1][:, :5]                    # (a realisation does not depend on its slot: tested above)
    plan = _plan(ofdm, case, b, "fp64")
    assert _same(_tile(ofdm, plan, b, taps), want)

    plan.set_descrambler(tc_register())
    with pytest.raises(ofdm.OfdmError, match="DeScrambler"):
        _tile(ofdm, plan, b, taps)
    plan.set_descrambler(None)
    assert _same(_tile(ofdm, plan, b, taps), want)

    with pytest.raises(ofdm.OfdmError, match="same number of channel taps"):
        _tile(ofdm, plan, b, taps[:4] + [taps[4][:-1]])
    assert _same(_tile(ofdm, plan, b, taps), want)

    # a precision flag opposite to the plan's: only the C entry can be handed one
    tx = np.ascontiguousarray(b["Tx_noised"].astype(np.complex64))
    delay = np.ascontiguousarray(np.array([np.real(t[:, 0]) for t in taps]).astype(np.int32))
    amp = np.ascontiguousarray(np.array([t[:, 1] for t in taps]).astype(np.complex128))
    ref = np.ascontiguousarray(b["ref"])
    nm, er = np.zeros((4, 5)), np.zeros((4, 5), dtype=np.uint32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)                                        # noqa: E731
    rc = L.load().ofdm_task5_part2_tile(plan.handle, ptr(tx), ptr(delay), ptr(amp), delay.shape[1], 5, tc.SNR_DB, ptr(ref), ptr(nm),
                                        ptr(er), L.OFDM_F32 | L.OFDM_HOST)
    with pytest.raises(ofdm.OfdmError, match="precision flag differs from the plan's"):
        L.check(rc, "task5_part2_tile")
    assert not nm.any() and not er.any()
    assert _same(_tile(ofdm, plan, b, taps), want)

    late = taps[2].copy()
    late[-1, 0] = case.nfft
    with pytest.raises(ofdm.OfdmError, match="tap delay outside"):
        _tile(ofdm, plan, b, taps[:2] + [late] + taps[3:])
    assert _same(_tile(ofdm, plan, b, taps), want)

    nmse, errors = _tile(ofdm, plan, b, [])
    assert nmse.shape == errors.shape == (4, 0)
    assert _same(_tile(ofdm, plan, b, taps), want)
    plan.close()


def tc_register():
    from ofdm_course_amd.drivers import common
    return common.REGISTER
