"""The refusals of ofdm_rx_chain_task4 (t4_route_choose, the rows of t4_routes.REFUSALS on the n64 geometry): the call raises
OfdmError with the message the receiver's source has always had for it, and the plan is left as it was -- a valid call on it
afterwards equals, bit for bit, the same call on a fresh plan.

The one-pilot plan has no valid call: the spline operator of estimate_channel.m:8 needs two knots, and its build (t4_plan_tables)
fails on every call of such a plan, with or without a sync flag.  Before the route was chosen up front that build came before
the check of fine_sync's two pilots, so "fine_sync needs at least two pilot carriers" was never seen; now the route's refusal
comes first when a sync flag is set.  For that row the call afterwards is compared as the error it raises."""
import numpy as np
import pytest

import t4_cases as tc
import t4_routes as tr

pytestmark = pytest.mark.gpu

# the flags of the call afterwards: no sync flag, so the changed guard / frame length / pilot count is accepted
AFTER_FLAGS = (0, 0, 1)
NO_SPLINE = "spline: needs at least two knots"


def _plan(ofdm, oracle, precision, changed):
    c = tc.BY_NAME["n64"]
    lay = tc.layout(oracle, c)
    pc, dc, col = lay["pc"], lay["dc"], lay["col"]
    if changed.get("np") == 1:
        pc, col = pc[:1], col[:1]
        dc = np.arange(2, c.N_carrier + 1, dtype=np.float64)
    tg, ns = changed.get("t_guard", c.T_guard), changed.get("n_symb", c.N_symb)
    plan = ofdm.RxPlan(c.Nfft, tg, ns, c.N_carrier, pc, dc, col, int(np.ceil(c.N_carrier / 6)), 3, c.const, precision=precision)
    return plan, (c.Nfft + tg) * ns


def _call(ofdm, plan, rx, flags):
    """The outputs as bytes, or the text of the error the call raises."""
    from ofdm_course_amd._lib import OfdmError
    try:
        out = ofdm.rx_chain_task4(plan, rx, *flags, want_h=True)
    except OfdmError as e:
        return str(e)
    return {k: np.ascontiguousarray(np.asarray(v)).tobytes() for k, v in out.items() if v is not None}


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("name", sorted(tr.REFUSALS))
def test_refused_call_raises_and_leaves_the_plan_as_it_was(ofdm, oracle, monkeypatch, name, precision):
    from ofdm_course_amd._lib import OfdmError
    for v in ("OFDM_T4_STAGED", "OFDM_T4_NO_WAVE", "OFDM_T4_FULL_ACF", "OFDM_T4_UNFUSED_SYNC", "OFDM_T4_DENSE_SPLINE"):
        monkeypatch.delenv(v, raising=False)
    changed, flags, _, msg = tr.REFUSALS[name]
    plan, rows = _plan(ofdm, oracle, precision, changed)
    rng = np.random.default_rng([64, len(name)])
    rx = ((rng.standard_normal((rows, 3)) + 1j * rng.standard_normal((rows, 3))) / np.sqrt(2)).astype(
        np.complex128 if precision == "fp64" else np.complex64)
    with pytest.raises(OfdmError) as e:
        ofdm.rx_chain_task4(plan, rx, *flags, want_h=True)
    assert msg in str(e.value)
    after = _call(ofdm, plan, rx, AFTER_FLAGS)
    assert _call(ofdm, plan, rx, AFTER_FLAGS) == after          # (a failed build of the plan's tables leaves none behind)
    plan.close()
    fresh_plan, _ = _plan(ofdm, oracle, precision, changed)
    fresh = _call(ofdm, fresh_plan, rx, AFTER_FLAGS)
    fresh_plan.close()
    if name == "one_pilot":
        assert NO_SPLINE in fresh and after == fresh
        return
    assert sorted(after) == sorted(fresh) == ["FreqOffset", "H", "IFO", "TgPosition", "bits", "status"]
    for k in fresh:
        assert after[k] == fresh[k], k
