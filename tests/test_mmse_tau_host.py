"""The clamped rms delay spread of the MMSE estimators (csrc/mmse_tau.hpp), CPU only.

Every MMSE entry takes tau_rms = sqrt(max(r2 - r^2, 0)) of MMSE_CE.m:19-24 from that header.  For h = a delta[k - d] the exact
value is 0 and the computed difference is rounding noise of either sign; without the clamp a negative one turns every carrier of
the estimate into NaN.  The header is compiled here into a stand-alone program (tests/mmse_tau_main.cpp) with the address and
undefined-behaviour sanitizers and run as a program on (amplitude, delay) pairs; numpy forms the same difference in the same
order, so the test knows which pairs are negative and keeps covering the corner."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import mmse_degenerate_cases as dg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DF, NPS = 1.0 / 128, 4.0


@pytest.fixture(scope="module")
def tau_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no C++ compiler for the stand-alone program"
    exe = str(tmp_path_factory.mktemp("mmse_tau") / "mmse_tau_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "mmse_tau_main.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, responses, df=DF, nps=NPS):
    """responses: [[(amplitude, delay), ...], ...] -> (tau [n], c [n])."""
    text = "".join(f"{len(r)} " + " ".join(f"{complex(a).real.hex()} {complex(a).imag.hex()} {float(d).hex()}" for a, d in r) + "\n"
                   for r in responses)
    r = subprocess.run([exe, float(df).hex(), float(nps).hex()], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr        # a sanitizer report is a failure
    v = np.array([[float.fromhex(x) for x in line.split()] for line in r.stdout.splitlines()])
    assert v.shape == (len(responses), 2)
    return v[:, 0], v[:, 1]


def test_one_tap_sweep_is_finite_and_within_the_rounding_bound(tau_program):
    """a = 0.7 - 0.2j, d = 1..63: c finite, >= 0, at most 2 pi d sqrt(8 eps) df Nps; exactly 0 where numpy finds the difference
    negative, and at least 8 of the 63 pairs are (14 here)."""
    d = np.arange(1, 64)
    diff = np.array([dg.host_diff([(dg.A, k)]) for k in d])
    neg = d[diff < 0]
    print("negative pairs:", neg.tolist(), "smallest difference", diff.min())
    assert len(neg) >= 8
    tau, c = _run(tau_program, [[(dg.A, k)] for k in d])
    assert np.all(np.isfinite(c)) and np.all(c >= 0) and np.all(np.isfinite(tau)) and np.all(tau >= 0)
    assert np.all(c <= 2 * np.pi * dg.tau_delta(d) * DF * NPS)
    assert np.all(c[diff <= 0] == 0)
    want = 2.0 * np.pi * np.sqrt(np.maximum(diff, 0.0)) * DF * NPS              # the same operations in the same order
    assert np.array_equal(c, want)


def test_the_cases_of_the_gpu_tests_are_negative_in_host_arithmetic(tau_program):
    """plan.set_mmse at d = 5, 10, 15 and the study tile's realisations (d = 1..21, one path; two paths with the second outside
    1..N_carrier): the host code's difference is negative for the three chain delays and for some of the tile's, and the helper
    returns c = 0 there -- without the clamp these are the NaN operators of ofdm_rx_plan_set_mmse and ofdm_task5_part2_tile."""
    chain = [[(dg.A, d)] for d in dg.CHAIN_DELAYS]
    assert all(dg.host_diff(r) < 0 for r in chain)
    tiles = [dg.tile_kept(case, t) for case in (dg.TILE_ONE, dg.TILE_TWO) for t in case.taps_list()]
    assert all(len(r) == 1 for r in tiles)                                       # one path left inside 1..N_carrier
    neg = [r[0][1] for r in tiles if dg.host_diff(r) < 0]
    print("tile delays with a negative difference:", neg)
    assert len(neg) >= 3
    for nc, nps, rs in ((128, 4.0, chain), (400, 8.0, chain), (128, 4.0, tiles)):
        tau, c = _run(tau_program, rs, df=1.0 / nc, nps=nps)
        assert np.all(np.isfinite(c)) and np.all(c >= 0)
        assert np.all(c[[dg.host_diff(r) <= 0 for r in rs]] == 0)


def test_ordinary_profile_is_unchanged(tau_program, oracle):
    """The 6-tap profile of tests/test_gpu_chanest.py: tau_rms of oracle.MMSE_CE to 1e-12 relative, c = 2 pi tau df Nps."""
    taps = np.array([[0, 1], [4, .8], [10, .6], [15, .4], [21, .2], [25, .1]])
    h, _ = oracle.get_MP_channel_resp(taps, 512)
    pc, _ = oracle.pilot_layout_comb(128, 4)
    Y = np.ones((512, 1), dtype=np.complex128)
    _, want = oracle.MMSE_CE(Y, np.ones((len(pc), 1)), pc, 512, 128, h, 20.0)
    tau, c = _run(tau_program, [[(a, d) for d, a in enumerate(np.asarray(h).ravel())]])
    print("tau_rms", tau[0], "oracle", want)
    assert want > 1 and abs(tau[0] - want) <= 1e-12 * want
    assert abs(c[0] - 2 * np.pi * want * DF * NPS) <= 1e-12 * c[0]
