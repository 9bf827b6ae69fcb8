"""What makes the assertions of tests/test_gpu_estimator_study.py meaningful, worked out on the oracle alone (no GPU): the frames of
the study's cases restated on the oracle's Philox (estimator_cases.host_frames; the GPU test ties it to tx_frames_fused: the same bits
and taps, the samples to rounding) and replayed call by call.  The seeds the cases name were chosen for this:
  * every frame of every fp64 run (estimator_cases.FP64_RUNS: case, fading or static channel, mmse ls or genie) clears the 1e-6
    margins of the exact assertions -- pick gaps of MP and OMP, distance of every row's equalised points to a decision boundary;
  * of cases A and C (the fp32 runs) at most 10 % of a point's frames are fp32_loose (a pick gap below 1e-3), none of them in a
    workgroup's first or last slot.
Case A's runs and case C are replayed here in full.  Case D's 2 x 111 frames were replayed once and their margins are kept in
tests/golden/estimator_margins.json (every run's, per frame); here every kept value is checked against the bound and, per run and
point, the frame with the smallest kept margin is replayed again and must reproduce it."""
import json
import os

import numpy as np
import pytest

import estimator_cases as ec
import part2_tile_cases as tc

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "estimator_margins.json")))["runs"]


def _points(oracle, name, channel):
    return [ec.host_frames(oracle, ec.CASES[name], snr, seed, ec.FRAMES, channel=channel) for snr, seed in zip(ec.POINTS, ec.seeds(name))]


@pytest.fixture(scope="module")
def frames(oracle):
    cache = {}

    def get(name, channel):
        if (name, channel) not in cache:
            cache[name, channel] = _points(oracle, name, channel)
        return cache[name, channel]
    return get


def _kept(run):
    g = GOLDEN["-".join(run)]
    return (np.array([g[str(p)]["gap"] for p in range(len(ec.POINTS))]), np.array([g[str(p)]["margin"] for p in range(len(ec.POINTS))]))


RUNS_A = [r for r in ec.FP64_RUNS if r[0] == "A"]


@pytest.mark.parametrize("run", RUNS_A, ids=["-".join(r) for r in RUNS_A])
def test_every_frame_of_case_a_clears_the_fp64_margins(oracle, frames, run):
    name, channel, mmse = run
    r = ec.replay(oracle, ec.CASES[name], frames(name, channel), ec.POINTS, mmse)
    print(run, "smallest pick gap", r["gap"].min(), "smallest decision margin", r["margin"].min())
    assert r["clear"].all() and r["gap"].min() >= tc.FP64_GAP and r["margin"].min() >= tc.FP64_GAP
    assert np.all(np.isfinite(r["nmse"])) and np.all(r["nmse"] > 0)
    if "-".join(run) in GOLDEN:
        gap, margin = _kept(run)
        assert np.allclose(r["gap"], gap, rtol=1e-6) and np.allclose(r["margin"], margin, rtol=1e-6)


RUNS_D = [r for r in ec.FP64_RUNS if r[0] == "D"]


@pytest.mark.parametrize("run", RUNS_D, ids=["-".join(r) for r in RUNS_D])
def test_every_frame_of_case_d_clears_the_fp64_margins(oracle, frames, run):
    name, channel, mmse = run
    gap, margin = _kept(run)
    assert gap.shape == margin.shape == (len(ec.POINTS), ec.FRAMES)
    assert gap.min() >= tc.FP64_GAP and margin.min() >= tc.FP64_GAP
    worst = sorted({int(np.argmin(margin[p])) for p in range(len(ec.POINTS))})
    r = ec.replay(oracle, ec.CASES[name], frames(name, channel), ec.POINTS, mmse, frames=worst)
    print(run, "kept smallest gap", gap.min(), "margin", margin.min(), "replayed frames", worst)
    assert np.allclose(r["gap"][:, worst], gap[:, worst], rtol=1e-6) and np.allclose(r["margin"][:, worst], margin[:, worst], rtol=1e-6)
    assert r["clear"][:, worst].all()


@pytest.mark.parametrize("name", ["A", "C"])
def test_the_fp32_cases_are_loose_in_few_frames_and_never_at_a_workgroup_bound(oracle, frames, name):
    pts = frames(name, "fading")
    r = ec.replay(oracle, ec.CASES[name], pts, ec.POINTS, "ls")
    bnd = tc.boundary_slots(ec.FRAMES)
    print(name, "fp32_loose per point", [np.flatnonzero(l).tolist() for l in r["loose"]])
    assert r["clear"].all()
    for p in range(len(ec.POINTS)):
        assert r["loose"][p].mean() <= 0.1 and not (r["loose"][p] & bnd).any(), p
    # the realisations can be told apart: no two frames of a point share a channel or an error sum
    for g, n in zip(pts, r["nmse"]):
        assert len({a.tobytes() for a in g["taps"]}) == ec.FRAMES and len(set(n[:, 3])) == ec.FRAMES


def test_case_geometry_reaches_the_kernel_variants():
    a, c, d = ec.CASES["A"], ec.CASES["C"], ec.CASES["D"]
    assert (a.nfft, a.n_carrier, a.n_pilots, a.K) == (256, 128, 32, 64) and tc.mp_mfma(a.n_pilots, False)
    assert (c.nfft, c.n_carrier, c.n_pilots, c.K) == (256, 100, 18, 256) and not tc.mp_mfma(c.n_pilots, False) and c.n_pilots % 4
    assert (d.nfft, d.n_carrier, d.n_pilots, d.K) == (1024, 640, 160, 256) and tc.mp_fpw(d.n_pilots, d.paths, True) == 2
    assert max(ec.fading(c)[0]) >= c.n_carrier                    # ETU's last path is outside 1..N_carrier
    for case in (a, c, d):
        assert len(ec.fading(case)[0]) == case.paths
    # 37 frames: ragged for every split (16, 8 and 4 per workgroup) and for the chunks of 5 and 16 the GPU test asks for
    assert ec.FRAMES == 2 * 16 + 5 == 4 * 8 + 5 == 9 * 4 + 1 and ec.FRAMES % 5 and ec.FRAMES % 16
