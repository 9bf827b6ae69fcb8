"""The call plan of the estimator profile (csrc/est_profile_plan.hpp) on the CPU: tests/host/est_profile_plan_main.cpp is compiled
with the host compiler and the address and undefined-behaviour sanitizers into a stand-alone program and asked about every refusal
of the entry in its order, the chunk rule at a small and at a budget-limited shape, the launch shapes, and the bin function the
histogram takes from hest_plan.hpp at the edges of the grid, against numpy."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ofdm-course_amd", "csrc")
HEADER = os.path.join(CSRC, "est_profile_plan.hpp")

BUDGET = 2 << 30
SHAPE = dict(nfft=256, t_guard=32, n_symb=2, n_carrier=100, np=25, nd=75, bps=2, frame_words=10, pilots_in_band=1, device=0,
             ctx_device=0)
W = "estimator_profile"


def good(f64):
    return dict(SHAPE, plan=1, f64=f64, f64_flag=f64, frame0=0, n_points=1, fpp=5, max_chunk=0, points=1, h="none", taps="0,3,7",
                power=1.0, mmse_mode=0, out=1, descr=0, bins_n=60, bins_lo=-50.0, bins_hi=10.0)


# the checks in their order: (id, what breaks the good call there, the message)
ORDER = [
    ("args", dict(max_chunk=65536), f"{W}: bad arguments"),
    ("points_missing", dict(points=0), f"{W}: snr_db / seeds missing"),
    ("points_many", dict(n_points=1 << 31), f"{W}: too many points"),
    ("device", dict(ctx_device=1), "RX plan belongs to device 0, the context is on device 1"),
    ("precision", None, f"{W}: precision flag differs from the plan's"),
    ("no_data", dict(nd=0), f"{W}: the plan has no data carriers"),
    ("pilots", dict(pilots_in_band=0), f"{W}: pilots outside 1..N_carrier are not supported"),
    ("nfft", dict(nfft=200), f"{W}: unsupported Nfft 200 / T_guard 32"),
    ("stream", dict(frame0=(1 << 32) - 5), f"{W}: frame index outside the 32-bit stream range"),
    ("both", dict(h=4), f"{W}: give h (one channel for every frame) or taps (a channel per frame), not both"),
    ("fade_twice", dict(taps="0,3,3"), f"{W}: tap delay 3 given twice"),
    ("descr", dict(descr=1),
     f"{W}: the study runs unscrambled (Task5_part2.m:104-114,:285-299 are commented out); clear the plan's DeScrambler"),
    ("mmse_mode", dict(mmse_mode=2), f"{W}: mmse_mode must be 0 (h = ifft(H_LS)) or 1 (the frame's true taps) (2)"),
    ("bins", dict(bins_n=0), f"{W}: bins must have n 1 .. 4096 and finite lo < hi (0, -50, 10)"),
    ("output", dict(out=0), f"{W}: no output is given"),
]


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no C++ compiler for the stand-alone program"
    exe = str(tmp_path_factory.mktemp("est_profile_plan") / "est_profile_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "est_profile_plan_main.cpp"), "-o", exe], check=True)
    return exe


def _ask(host_program, lines):
    r = subprocess.run([host_program], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr              # a sanitizer report is a failure
    got = r.stdout.splitlines()
    assert len(got) == len(lines)
    return got


def _line(cmd, *dicts, **kv):
    merged = {}
    for d in dicts:
        merged.update(d)
    merged.update(kv)
    return cmd + " " + " ".join(f"{k}={v}" for k, v in merged.items())


@pytest.mark.parametrize("f64", [0, 1])
def test_every_refusal_in_the_documented_order(host_program, f64):
    checks = [(rid, dict(f64_flag=1 - f64) if rid == "precision" else brk, msg) for rid, brk, msg in ORDER]
    base = good(f64)
    lines = []
    for i in range(len(checks) + 1):                                 # every check from i on broken: check i is the first that fails
        d = dict(base)
        for _, brk, _ in reversed(checks[i:]):
            d.update(brk)
        lines.append(_line("profile", d))
    got = _ask(host_program, lines)
    for i, (rid, _, msg) in enumerate(checks):
        assert got[i] == f"refused {rid} {msg}", (i, rid, got[i])
    assert got[-1] == "ok"
    assert _ask(host_program, [_line("profile", base, plan=0)])[0] == f"refused args {W}: bad arguments"


def test_bins_refusals_in_the_channel_study_wording(host_program):
    base = good(1)
    bad = [(dict(bins_n=0), "(0, -50, 10)"), (dict(bins_n=4097), "(4097, -50, 10)"), (dict(bins_n=-3), "(-3, -50, 10)"),
           (dict(bins_lo=10.0), "(60, 10, 10)"), (dict(bins_lo=11.0), "(60, 11, 10)"), (dict(bins_hi="inf"), "(60, -50, inf)"),
           (dict(bins_lo="-inf"), "(60, -inf, 10)"), (dict(bins_lo="nan"), None), (dict(bins_hi="nan"), None)]
    got = _ask(host_program, [_line("profile", base, **b) for b, _ in bad])
    for (b, tail), g in zip(bad, got):
        assert g.startswith(f"refused bins {W}: bins must have n 1 .. 4096 and finite lo < hi ("), (b, g)
        if tail:
            assert g.endswith(tail), (b, g)
    ok = [dict(bins_n=1), dict(bins_n=4096), dict(bins_lo=9.999), dict(bins_lo=-1e300, bins_hi=1e300)]
    assert _ask(host_program, [_line("profile", base, **o) for o in ok]) == ["ok"] * len(ok)
    # the wording is the channel study's: one text in hest_plan.hpp, none in the profile's header
    hest = open(os.path.join(CSRC, "hest_plan.hpp")).read()
    assert hest.count("bins must have n 1 .. %d and finite lo < hi") == 1
    assert "bins must have" not in open(HEADER).read()


def frame_bytes(s, f64, fade_taps):
    cs = 16 if f64 else 8
    fs = (s["nfft"] + s["t_guard"]) * s["n_symb"]
    return 2 * cs * fs + 8 * s["n_symb"] + 4 * s["frame_words"] + 16 * fade_taps


def study_bytes(s, f64, taps):
    cs = 16 if f64 else 8
    body = cs * (s["n_carrier"] * s["n_symb"] + s["np"] + 4 * s["n_carrier"]) + 8
    rows = cs * (s["n_carrier"] + s["np"]) + 20 * taps + 16 * s["n_carrier"] + 4 * 12
    return body + rows


def chunk_model(s, f64, fade_taps, taps, fpp, cap, budget=2 * BUDGET):
    """The profile adds no bytes per frame: it reads what the study's budget holds already."""
    ch = cap if cap > 0 else max(1, budget // (frame_bytes(s, f64, fade_taps) + study_bytes(s, f64, taps)))
    return max(1, min(ch, fpp, 65535))


def test_chunk_rule_small_and_budget_limited(host_program):
    combos = [(f64, ft, fpp, cap) for f64 in (0, 1) for ft in (0, 4) for fpp in (1, 5, 65536) for cap in (0, 1, 2, 65535)]
    got = _ask(host_program, [_line("chunk", SHAPE, f64=f, fade_taps=t, taps=3, fpp=p, cap=c) for f, t, p, c in combos])
    for (f64, ft, fpp, cap), g in zip(combos, got):
        chunk, study, extra = map(int, g.split())
        assert extra == 0 and chunk == study == chunk_model(SHAPE, f64, ft, 3, fpp, cap), (f64, ft, fpp, cap, g)
    big = dict(SHAPE, nfft=8192, t_guard=1024, n_symb=64, n_carrier=6000, np=585, frame_words=10 ** 5)   # the budget is the limit
    chunk, study, _ = map(int, _ask(host_program, [_line("chunk", big, f64=1, taps=9, fpp=10 ** 6, cap=0)])[0].split())
    assert chunk == study == chunk_model(big, 1, 0, 9, 10 ** 6, 0) and 1 <= chunk < 65535
    small_budget = 10 * (frame_bytes(SHAPE, 1, 4) + study_bytes(SHAPE, 1, 3)) + 7                       # ten frames and a rest
    chunk, study, _ = map(int, _ask(host_program, [_line("chunk", SHAPE, f64=1, fade_taps=4, taps=3, fpp=37, cap=0,
                                                         budget=small_budget)])[0].split())
    assert chunk == study == 10


def test_launch_shapes(host_program):
    cases = [(100, 25, 5), (64, 256, 1), (65, 257, 64), (1200, 2048, 4096)]
    got = _ask(host_program, [_line("pass", SHAPE, n_carrier=nc, k_atoms=k, frames=m) for nc, k, m in cases])
    for (nc, k, m), g in zip(cases, got):
        # 13 quantities x ceil(nc / 64) workgroups of 256 threads on a 64 x 64 tile of doubles; a thread per delay, tiles of 32
        # frames x (32 picks of 4 + 8 bytes, 64 taps of 8 bytes); a thread per frame and estimator
        assert tuple(map(int, g.split())) == (256, -(-nc // 64), 13, 32768, 256, -(-k // 256), 32 * (12 * 32 + 8 * 64), 256,
                                              -(-4 * m // 256))


def test_bin_function_at_the_grid_edges_against_numpy(host_program):
    for n, lo, hi, nc in ((60, -50.0, 10.0, 100), (1, -3.0, 0.5, 200), (7, -10.0, 11.0, 1)):
        edges = np.array([hi if i == n else lo + (hi - lo) * i / n for i in range(n + 1)])
        want_thr = nc * 10.0 ** (edges / 10.0)
        vals = []
        for t in want_thr:
            vals += [np.nextafter(t, 0.0), t, np.nextafter(t, np.inf)]
        vals += [0.0, 1e-300, 1e300, float("inf"), float("nan"), -1.0]
        g = _ask(host_program, [_line("bins", n=n, lo=lo, hi=hi, n_carrier=nc, v=",".join(float(v).hex() if np.isfinite(v) else str(v)
                                                                                      for v in vals))])[0]
        thr_txt, bins_txt = g.split("|")
        thr = np.array([float.fromhex(t) for t in thr_txt.split()])
        assert thr.shape == (n + 1,) and np.all(np.diff(thr) > 0)
        np.testing.assert_allclose(thr, want_thr, rtol=4 * 2.0 ** -52, atol=0)      # pow against numpy's: an ulp or two
        got = [int(b) for b in bins_txt.split()]
        v = np.array(vals)
        with np.errstate(invalid="ignore"):
            want = np.searchsorted(thr, v, side="right") - 1           # the last b with thr[b] <= v
            want = np.where(np.isnan(v), -3, np.where(v < thr[0], -1, np.where(v >= thr[n], -2, want)))
        # asked with the program's own table, so the edges are hit exactly where the tables agree; elsewhere a neighbour of an
        # edge is still classified by the same comparisons
        exact = np.array([float.fromhex(float(x).hex()) if np.isfinite(x) else x for x in vals])
        assert np.array_equal(exact, v, equal_nan=True)
        assert got == list(want), (n, lo, hi)


def test_the_header_is_free_of_the_device_runtime():
    src = open(HEADER).read()
    assert "hip/" not in src and "__global__" not in src and "hipLaunch" not in src
    assert set(re.findall(r'#include [<"]([^>"]+)[>"]', src)) <= {"cstddef", "cstdint", "chain_route.hpp", "est_plan.hpp", "hest_plan.hpp"}
