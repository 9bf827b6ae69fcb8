"""ofdm_rx_chain_task4 against the outputs of the commit before its route decision moved into t4_route.hpp
(tests/golden/t4_routes_parent.json, written by `python tests/golden/make_golden.py --t4-routes-parent` on that commit): every
case of t4_cases.CASES in both precisions with the flags (1, 1, 1) and (0, 0, 1), and the seven switch runs of t4_routes.py
(test_gpu_task4_sizes.SWITCH_RUNS + OFDM_T4_DENSE_SPLINE), bit for bit.  TgPosition, IFO, status and the bit pattern of
FreqOffset are compared on every frame; the error counts, the packed bits and H on the frames with status >= 0 (remove_IFO's
index error leaves the others undefined).  The file lists the fields it keeps: those that agreed between two runs of the parent."""
import hashlib
import json
import os

import numpy as np
import pytest

import t4_cases as tc
from t4_routes import SWITCH_ROWS
from test_gpu_task4_sizes import _run

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "t4_routes_parent.json")
FIELDS = ("TgPosition", "IFO", "status", "FreqOffset", "errors", "packed", "H")

RUNS = [(c.name, p, fl, ()) for c in tc.CASES for p in ("fp64", "fp32") for fl in tc.TWO_FLAGS]
RUNS += [(name, p, (1, 1, 1), (switch,)) for switch, name in SWITCH_ROWS for p in ("fp64", "fp32")]


def run_id(run):
    name, precision, flags, env = run
    return "-".join([name, precision, "".join(map(str, flags)), *env])


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def route_record(ofdm, oracle, monkeypatch, run):
    """One call of the run through test_gpu_task4_sizes._run, reduced to what the golden file stores."""
    name, precision, flags, env = run
    got = _run(ofdm, oracle, monkeypatch, tc.BY_NAME[name], precision, flags, env=env)
    live = got["status"] >= 0
    return dict(TgPosition=[int(v) for v in got["TgPosition"]], IFO=[int(v) for v in got["IFO"]],
                status=[int(v) for v in got["status"]],
                FreqOffset=[f"{int(v):016x}" for v in np.asarray(got["FreqOffset"], np.float64).view(np.uint64)],
                errors=[int(e) if ok else -1 for e, ok in zip(got["errors"], live)],
                packed=_sha(got["packed"][live]), H=_sha(got["H"][:, live]))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_golden_lists_every_run(golden):
    assert sorted(golden["runs"]) == sorted(run_id(r) for r in RUNS)
    assert tuple(golden["fields"]) == FIELDS


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_run_matches_parent(ofdm, oracle, monkeypatch, golden, run):
    got = route_record(ofdm, oracle, monkeypatch, run)
    want = golden["runs"][run_id(run)]
    for field in golden["fields"]:
        assert got[field] == want[field], (run_id(run), field)
