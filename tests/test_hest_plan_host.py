"""The call plan of the channel-estimate capture (csrc/hest_plan.hpp) on the CPU: tests/host/hest_plan_main.cpp is compiled with the
host compiler and the address and undefined-behaviour sanitizers into a stand-alone program and asked about the refusals of both
entries in their order, the chunk rule at its edges, the launch shapes with their LDS budget, and the bin function -- at and beside
every edge of the table, for NaN and for both infinities -- against the Python twins of tests/hest_cases.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hest_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ofdm-course_amd", "csrc")
HEADER = os.path.join(CSRC, "hest_plan.hpp")


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no C++ compiler for the stand-alone program"
    exe = str(tmp_path_factory.mktemp("hest_plan") / "hest_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "hest_plan_main.cpp"), "-o", exe], check=True)
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
def test_rx_hest_first_refusal_wins_in_the_documented_order(host_program, f64):
    order, good = hc.rx_order(f64), hc.good_rx(f64)
    got = _ask(host_program, [_line("rx", hc.broken_from(good, order, i)) for i in range(len(order) + 1)])
    for i, (rid, _, msg) in enumerate(order):
        assert got[i] == f"refused {rid} {msg}", (i, rid, got[i])
    assert got[-1] == "ok"
    assert _ask(host_program, [_line("rx", good, plan=0)])[0] == "refused args rx_hest: bad arguments"
    # every flag pair; without a synchroniser flag the route has nothing to refuse: one symbol, no guard
    ok = [dict(n_frames=0), dict(n_frames=(1 << 31) - 1), dict(time_desync=0), dict(freq_desync=0), dict(time_desync=0, freq_desync=0),
          dict(time_desync=0, freq_desync=0, n_symb=1), dict(time_desync=0, freq_desync=0, t_guard=0), dict(np=2), dict(bins_n=0)]
    assert _ask(host_program, [_line("rx", good, **o) for o in ok]) == ["ok"] * len(ok)
    bad = [(dict(time_desync=-1), "time_desync", "time_desync must be 0 or 1 (-1)"),
           (dict(freq_desync=-1), "freq_desync", "freq_desync must be 0 or 1 (-1)"),
           (dict(np=0), "pilots", "estimate_channel needs at least two pilot carriers (0)"),
           (dict(time_desync=0, freq_desync=0, np=1), "pilots", "estimate_channel needs at least two pilot carriers (1)"),
           (dict(t_guard=0), "route", "rx_chain_task4: frame shorter than T_guard + Nfft, or T_guard outside 1..1024"),
           (dict(time_desync=0, n_symb=1, nfft=512, t_guard=64), "route", "rx_chain_task4: frame shorter than T_guard + Nfft, or T_guard outside 1..1024")]
    got = _ask(host_program, [_line("rx", good, **b) for b, _, _ in bad])
    for (b, rid, msg), g in zip(bad, got):
        assert g == f"refused {rid} rx_hest: {msg}", (b, g)


@pytest.mark.parametrize("f64", [0, 1])
def test_hest_study_first_refusal_wins_in_the_documented_order(host_program, f64):
    order, good = hc.study_order(f64), hc.good_study(f64)
    got = _ask(host_program, [_line("study", hc.broken_from(good, order, i)) for i in range(len(order) + 1)])
    for i, (rid, _, msg) in enumerate(order):
        assert got[i] == f"refused {rid} {msg}", (i, rid, got[i])
    assert got[-1] == "ok"
    assert _ask(host_program, [_line("study", good, plan=0)])[0] == "refused args hest_study: bad arguments"
    for brk in (dict(n_points=-1), dict(fpp=-1), dict(max_chunk=65536)):
        assert _ask(host_program, [_line("study", good, **brk)])[0] == "refused args hest_study: bad arguments"
    ok = [dict(n_points=0, points=0), dict(fpp=0), dict(reg="none"), dict(h="none"), dict(h="none", taps="0,3,7"), dict(h=64),
          dict(sto_mode=0, cfo_mode=0), dict(max_chunk=1), dict(max_chunk=65535), dict(frame0=(1 << 32) - 6), dict(bins_n=1),
          dict(bins_n=4096), dict(time_desync=0, freq_desync=0), dict(bins_lo=-1e300, bins_hi=1e300)]
    assert _ask(host_program, [_line("study", good, **o) for o in ok]) == ["ok"] * len(ok)
    bad = [(dict(bins_n=-1), "(-1, -50, 10)"), (dict(bins_n=4097), "(4097, -50, 10)"), (dict(bins_lo=10.0), "(60, 10, 10)"),
           (dict(bins_lo=11.0), "(60, 11, 10)"), (dict(bins_hi="nan"), "(60, -50, nan)"), (dict(bins_hi="inf"), "(60, -50, inf)"),
           (dict(bins_lo="-inf"), "(60, -inf, 10)")]
    got = _ask(host_program, [_line("study", good, **b) for b, _ in bad])
    assert got == [f"refused bins hest_study: bins must have n 1 .. 4096 and finite lo < hi {tail}" for _, tail in bad]


def test_channel_refusals_sit_between_the_two_channels_check_and_the_capture(host_program):
    good = hc.good_study(1)
    got = _ask(host_program, [_line("study", good, **brk) for brk, _, _ in hc.CHANNEL])
    for (brk, rid, msg), g in zip(hc.CHANNEL, got):
        assert g == f"refused {rid} {msg}", (brk, g)
    got = _ask(host_program, [_line("study", good, **dict(brk, time_desync=2)) for brk, _, _ in hc.CHANNEL])
    assert [g.split()[1] for g in got] == [rid for _, rid, _ in hc.CHANNEL]
    assert _ask(host_program, [_line("study", good, h=65, taps="0,3")])[0].split()[1] == "both"


def test_chunk_rule_at_its_edges(host_program):
    """max(1, min(cap or 2 BUDGET // (generator frame bytes with the RX region + the receiver's arena + the rows), frames_per_point,
    65535)); the rows: 33 bytes per carrier, 17 per pilot, 40 of scalars."""
    combos = [(f64, scr, imp, ft, fpp, cap) for f64 in (0, 1) for scr in (0, 1) for imp in (0, 1) for ft in (0, 3)
              for fpp in (1, 5, 65535, 65536, 10 ** 7) for cap in (0, 1, 3, 65535)]
    got = _ask(host_program, [_line("chunk", hc.SHAPE, f64=f, scr=s, imp=i, fade_taps=t, fpp=p, cap=c) for f, s, i, t, p, c in combos])
    for (f64, scr, imp, ft, fpp, cap), g in zip(combos, got):
        chunk, fb, rows = map(int, g.split())
        assert fb == hc.frame_bytes(hc.SHAPE, f64, scr, imp, ft) and rows == 33 * 64 + 17 * 16 + 40 == hc.row_bytes(hc.SHAPE)
        assert chunk == hc.chunk_model(hc.SHAPE, f64, scr, imp, ft, fpp, cap), (f64, scr, imp, ft, fpp, cap)
        assert 1 <= chunk <= min(fpp, 65535)
    big = dict(hc.SHAPE, nfft=8192, t_guard=1024, n_symb=64, n_carrier=6000, np=1500)   # the budget, not the grid, is the limit
    a = int(_ask(host_program, [_line("chunk", big, f64=1, fpp=10 ** 6, cap=0)])[0].split()[0])
    assert a == hc.chunk_model(big, 1, 0, 0, 0, 10 ** 6, 0) and 1 <= a < 65535
    huge = dict(big, n_symb=4096)                                     # a frame beyond the whole budget: one frame per chunk
    assert int(_ask(host_program, [_line("chunk", huge, f64=1, fpp=10, cap=0)])[0].split()[0]) == 1


def test_launch_shapes_and_lds_budget(host_program):
    combos = [(nc, npil, frames) for nc in (1, 15, 16, 17, 64, 65, 100, 128, 255, 256, 257, 400, 4096) for npil in (2, 64, 65, 1024)
              for frames in (1, 3, 33, 65535)]
    got = _ask(host_program, [_line("pass", hc.SHAPE, n_carrier=c, np=p, frames=m) for c, p, m in combos])
    for (nc, npil, frames), g in zip(combos, got):
        assert tuple(map(int, g.split())) == hc.pass_model(dict(hc.SHAPE, n_carrier=nc, np=npil), frames), (nc, npil, frames)
        threads, lanes, per, lds, grid, acc_threads, acc_grid, acc_pil, acc_lds = map(int, g.split())
        assert threads == 256 and lanes * per == 256 and per <= 16       # whole wavefronts, every frame slot of the LDS used
        assert (lanes >= nc or lanes == 256) and (lanes // 2 < nc or lanes == 16)
        assert (grid - 1) * per < frames <= grid * per
        assert lds == 16384 <= hc.LDS_LIMIT and acc_lds == 36864 <= hc.LDS_LIMIT
        assert (acc_grid - 1) * 64 < nc <= acc_grid * 64 and (acc_pil - 1) * 64 < npil <= acc_pil * 64
        assert (per == 1) == (nc > 128)                                   # one frame per workgroup from 129 carriers on


def test_bin_function_at_and_beside_every_edge(host_program):
    """On three grids: the value at threshold b falls in bin b (the last in `above`), the value just below it in bin b - 1 (the first in
    `below`), the value just above it in bin b; NaN, both infinities, 0 and a negative value; and arbitrary values against the twin's
    search on the program's own table."""
    for n, lo, hi, nc in [(60, -50.0, 10.0, 64), (1, -3.0, 0.0, 400), (7, -20.5, 3.25, 1), (4096, -100.0, 100.0, 8192)]:
        grid = dict(n=n, lo=lo, hi=hi, n_carrier=nc)
        thr = [float.fromhex(t) for t in _ask(host_program, [_line("table", grid)])[0].split()]
        assert len(thr) == n + 1 and all(a < b for a, b in zip(thr, thr[1:]))
        # the table against the formula, to the rounding of pow: N_carrier 10^(edge / 10)
        edges = np.asarray(hc.thresholds(n, lo, hi, nc))
        assert np.allclose(thr, nc * 10.0 ** (edges / 10.0), rtol=1e-13, atol=0.0)
        assert thr[-1] == nc * 10.0 ** (hi / 10.0) or abs(thr[-1] / (nc * 10.0 ** (hi / 10.0)) - 1) < 1e-15
        picks = list(range(n + 1)) if n <= 60 else [0, 1, 2, n // 2, n - 1, n]
        qs = [_line("binat", grid, edge=b, side=s) for b in picks for s in (-1, 0, 1)]
        got = list(map(int, _ask(host_program, qs)))
        for i, b in enumerate(picks):
            below, at, above = got[3 * i:3 * i + 3]
            assert below == (b - 1 if b > 0 else hc.BIN_BELOW), (n, b, below)
            assert at == above == (b if b < n else hc.BIN_ABOVE), (n, b, at, above)
        special = [("nan", hc.BIN_NAN), ("-nan", hc.BIN_NAN), ("inf", hc.BIN_ABOVE), ("-inf", hc.BIN_BELOW), ("0", hc.BIN_BELOW),
                   ("-1.5", hc.BIN_BELOW), ("0x1p-1074", hc.BIN_BELOW), ("0x1.fffffffffffffp1023", hc.BIN_ABOVE)]
        got = list(map(int, _ask(host_program, [_line("bin", grid, v=v) for v, _ in special])))
        assert got == [w for _, w in special], (n, got)
        rng = np.random.default_rng(n)
        vals = np.concatenate([nc * 10.0 ** (rng.uniform(lo - 5, hi + 5, 200) / 10.0), np.asarray(thr)])
        got = list(map(int, _ask(host_program, [_line("bin", grid, v=float(v).hex()) for v in vals])))
        assert got == [hc.hist_bin(float(v), thr) for v in vals]
        assert all(g in (hc.BIN_BELOW, hc.BIN_ABOVE) or 0 <= g < n for g in got)


def test_every_refusal_text_is_in_the_header_and_the_header_is_free_of_the_device_runtime():
    src = open(HEADER).read()
    for fmt in ("%s: time_desync must be 0 or 1 (%d)", "%s: freq_desync must be 0 or 1 (%d)",
                "%s: estimate_channel needs at least two pilot carriers (%d)",
                "%s: bins must have n 1 .. %d and finite lo < hi (%d, %g, %g)", "%s: no output is given",
                "%s: n_frames must be 0 .. 2^31 - 1 (%lld)"):
        assert f'"{fmt}"' in src, fmt
    main = open(os.path.join(ROOT, "tests", "host", "hest_plan_main.cpp")).read()
    names = re.findall(r'"(\w+)"', re.search(r"IDS\[HEST_REFUSALS\] = \{(.*?)\};", main, re.S).group(1))
    txf = open(os.path.join(CSRC, "txf_plan.hpp")).read()
    txf_enum = re.search(r"TXF_OK = 0,(.*?)TXF_REFUSALS", txf, re.S).group(1)
    # the front every study shares: its texts live in txf_plan.hpp, and the header calls it
    for fmt in ("%s: register entries must be 0 or 1",
                "%s: give h (one channel for every frame) or taps (a channel per frame), not both"):
        assert f'"{fmt}"' in txf and f'"{fmt}"' not in src, fmt
    assert "txf_study_prelude(" in src and "inline int txf_study_prelude(" in txf
    own = re.search(r"enum \{ HEST_REFUSE_FRAMES = TXF_REFUSALS,(.*?)HEST_REFUSALS \}", src, re.S).group(1)
    assert [n.upper() for n in names[1:]] == re.findall(r"TXF_REFUSE_(\w+)", txf_enum) + ["FRAMES"] + re.findall(r"HEST_REFUSE_(\w+)", own)
    assert "hip/" not in src and "__global__" not in src and "hipLaunch" not in src
    assert set(re.findall(r'#include [<"]([^>"]+)[>"]', src)) <= {"algorithm", "cmath", "cstddef", "cstdint", "sync_plan.hpp"}
    hip = open(os.path.join(CSRC, "ofdm_hest_study.hip")).read()
    assert '#include "hest_plan.hpp"' in hip and "hest_rx_prelude(" in hip and "hest_study_prelude(" in hip
    assert "hest_chunk(" in hip and "hest_pass(" in hip and "TXF_WS_BUDGET" not in hip
    assert "hest_bin(" in hip and "hest_thresholds(" in hip and "log10" not in hip      # the device never takes a logarithm
    assert "txf_frame_nmse(" in hip and "txf_point_sums1(" in hip and "t5_frame_nmse_kernel<" not in hip   # called, not rewritten
    sweep = open(os.path.join(CSRC, "ofdm_ber_sweep.hip")).read()
    assert "channel_resp(a, dl, k, nfft, inv, hr, hi)" in sweep and "channel_resp(" in hip                 # one H_f(k) for both
    assert "sincospi" not in sweep and "sincospi" not in hip
    assert "hipfft" not in hip.lower() and "rocblas" not in hip.lower()
