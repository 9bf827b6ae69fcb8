"""rx_chain_task4 and ber_sweep_task4 against what they returned on the commit before task4_run was split into t4_call_prepare,
t4_front_end and the stages behind (tests/golden/t4_split_parent.json, written by tests/golden/make_t4_split_golden.py on that
commit through the public calls): one small batch per route of t4_routes.py -- every case of t4_cases.CASES in both precisions
with the flags (1, 1, 1) and (0, 0, 1), and the seven switch runs --, bit for bit: TgPosition, IFO, status, the error counts, the
packed bits and the MER sums of the receiver call; the errors, status counts, per-frame errors and the MER sums (per point and per
frame) of a sweep of 2 points x 3 frames.  The file lists the fields it keeps: those that agreed between two runs of the parent."""
import json
import os

import pytest

import t4_split_cases as ts

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "t4_split_parent.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_golden_lists_every_run_and_both_entries(golden):
    assert sorted(golden["runs"]) == sorted(ts.run_id(r) for r in ts.RUNS)
    assert set(golden["fields"]) <= set(ts.FIELDS)
    # bits, errors and MER sums of both entries are among the fields that were repeatable on the parent
    assert {"errors", "packed", "mer_sums", "sweep_errors", "sweep_frame_errors", "sweep_mer_sums"} <= set(golden["fields"])


@pytest.mark.parametrize("run", ts.RUNS, ids=ts.run_id)
def test_run_matches_parent(ofdm, oracle, golden, run):
    got = ts.record(ofdm, oracle, run)
    want = golden["runs"][ts.run_id(run)]
    for field in golden["fields"]:
        assert got[field] == want[field], (ts.run_id(run), field)
