"""Every case of routes.CASES against the outputs of the commit before the route decision moved into chain_route.hpp
(tests/golden/chain_routes_parent.json, written by `python tests/golden/make_golden.py --chain-routes-parent` on that commit):
the packed bits, the error counts, the pick indices and the bytes of H, bit for bit.  The file lists the fields it keeps: those
whose hashes agreed between two runs of the parent (the MER sums are accumulated with floating-point atomics and stay under the
tolerance checks of test_gpu_chain_routes.py)."""
import hashlib
import json
import os

import numpy as np
import pytest

from routes import CASES
from test_gpu_chain_routes import _call, _frames, _set_env

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_routes_parent.json")


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def route_hashes(ofdm, oracle, monkeypatch, case):
    """One call of the case through test_gpu_chain_routes._call, reduced to what the golden file stores."""
    cfg = case.cfg()
    _set_env(monkeypatch, {})
    rx, _, packed = _frames(ofdm, oracle, case, cfg)
    got = _call(ofdm, monkeypatch, case, cfg, case.env, rx, packed)
    rec = dict(packed=_sha(got["packed"]), errors=[int(e) for e in got["errors"]], H=_sha(got["H"]))
    if got["index"] is not None:
        rec["index"] = _sha(got["index"])
    return rec


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_golden_lists_every_case(golden):
    assert sorted(golden["cases"]) == sorted(c.name for c in CASES)
    assert set(golden["fields"]) <= {"packed", "errors", "index", "H"} and "packed" in golden["fields"]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_route_matches_parent(ofdm, oracle, monkeypatch, golden, case):
    got = route_hashes(ofdm, oracle, monkeypatch, case)
    want = golden["cases"][case.name]
    for field in golden["fields"]:
        if field == "index" and case.mode != "omp":
            continue
        assert got[field] == want[field], (case.name, field)
