"""The call plan of the coarse-sync capture (csrc/sync_plan.hpp) on the CPU: tests/host/sync_plan_main.cpp is compiled with the
host compiler and the address and undefined-behaviour sanitizers into a stand-alone program and asked about the refusals of both
entries in their order, the chunk rule, the launch shape with its LDS budget, and the two frame functions -- the guard-phase bin
at the extremes of int64 and the wrapped fractional error at its ties -- against the Python twins of tests/sync_cases.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sync_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ofdm-course_amd", "csrc")
HEADER = os.path.join(CSRC, "sync_plan.hpp")
I64_MAX = (1 << 63) - 1


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no C++ compiler for the stand-alone program"
    exe = str(tmp_path_factory.mktemp("sync_plan") / "sync_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "sync_plan_main.cpp"), "-o", exe], check=True)
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
def test_rx_acf_first_refusal_wins_in_the_documented_order(host_program, f64):
    order, good = sc.rx_order(f64), sc.good_rx(f64)
    got = _ask(host_program, [_line("rx", sc.broken_from(good, order, i)) for i in range(len(order) + 1)])
    for i, (rid, _, msg) in enumerate(order):
        assert got[i] == f"refused {rid} {msg}", (i, rid, got[i])
    assert got[-1] == "ok"
    assert _ask(host_program, [_line("rx", good, plan=0)])[0] == "refused args rx_acf: bad arguments"
    ok = [dict(n_frames=0), dict(n_frames=(1 << 31) - 1), dict(width=1), dict(width=16), dict(width=1024),
          dict(n_symb=1, width=31)]                               # the last: n_out = 288 - 31 - 256 = 1
    assert _ask(host_program, [_line("rx", good, **o) for o in ok]) == ["ok"] * len(ok)
    bad = [(dict(width=-1), "width", "WidthWindow must be 1 .. 1024 (-1)"), (dict(width=1025), "width", "WidthWindow must be 1 .. 1024 (1025)"),
           (dict(n_symb=1, width=32), "short", "a frame of 288 samples is shorter than WidthWindow + Nfft + 1 (32 + 256 + 1)"),
           (dict(n_symb=2, nfft=1024, t_guard=0, n_carrier=64, width=1024), "short",
            "a frame of 2048 samples is shorter than WidthWindow + Nfft + 1 (1024 + 1024 + 1)"),
           (dict(width=I64_MAX), "width", f"WidthWindow must be 1 .. 1024 ({I64_MAX})")]
    got = _ask(host_program, [_line("rx", good, **b) for b, _, _ in bad])
    for (b, rid, msg), g in zip(bad, got):
        assert g == f"refused {rid} rx_acf: {msg}", (b, g)


@pytest.mark.parametrize("f64", [0, 1])
def test_sync_study_first_refusal_wins_in_the_documented_order(host_program, f64):
    order, good = sc.study_order(f64), sc.good_study(f64)
    got = _ask(host_program, [_line("study", sc.broken_from(good, order, i)) for i in range(len(order) + 1)])
    for i, (rid, _, msg) in enumerate(order):
        assert got[i] == f"refused {rid} {msg}", (i, rid, got[i])
    assert got[-1] == "ok"
    assert _ask(host_program, [_line("study", good, plan=0)])[0] == "refused args sync_study: bad arguments"
    for brk in (dict(n_points=-1), dict(fpp=-1)):
        assert _ask(host_program, [_line("study", good, **brk)])[0] == "refused args sync_study: bad arguments"
    ok = [dict(n_points=0, points=0), dict(fpp=0), dict(reg="none"), dict(h="none"), dict(h="none", taps="0,3,7"), dict(h=64),
          dict(sto_mode=0, cfo_mode=0), dict(max_chunk=1), dict(frame0=(1 << 32) - 6), dict(width=1), dict(width=1024)]
    assert _ask(host_program, [_line("study", good, **o) for o in ok]) == ["ok"] * len(ok)


def test_channel_refusals_sit_between_the_two_channels_check_and_the_capture(host_program):
    good = sc.good_study(1)
    got = _ask(host_program, [_line("study", good, **brk) for brk, _, _ in sc.CHANNEL])
    for (brk, rid, msg), g in zip(sc.CHANNEL, got):
        assert g == f"refused {rid} {msg}", (brk, g)
    # behind "h and taps together", in front of the capture
    got = _ask(host_program, [_line("study", good, **dict(brk, width=0)) for brk, _, _ in sc.CHANNEL])
    assert [g.split()[1] for g in got] == [rid for _, rid, _ in sc.CHANNEL]
    assert _ask(host_program, [_line("study", good, h=65, taps="0,3")])[0].split()[1] == "both"


def test_chunk_rule(host_program):
    """max(1, min(cap or BUDGET // (generator frame bytes with the RX region + the row and the scalars), frames_per_point, 65535))."""
    combos = [(f64, scr, imp, ft, fpp, cap, w) for f64 in (0, 1) for scr in (0, 1) for imp in (0, 1) for ft in (0, 3)
              for fpp in (1, 5, 10 ** 7) for cap in (0, 1, 3, 65535, 10 ** 7) for w in (1, 32, 1024)]
    got = _ask(host_program, [_line("chunk", sc.SHAPE, f64=f, scr=s, imp=i, fade_taps=t, fpp=p, cap=c, width=w)
                              for f, s, i, t, p, c, w in combos])
    for (f64, scr, imp, ft, fpp, cap, w), g in zip(combos, got):
        chunk, fb, rows = map(int, g.split())
        assert fb == sc.frame_bytes(sc.SHAPE, f64, scr, imp, ft) and rows == 8 * (1440 - w - 256) + 32
        assert chunk == sc.chunk_model(sc.SHAPE, f64, scr, imp, ft, fpp, cap, w), (f64, scr, imp, ft, fpp, cap, w)
    big = dict(sc.SHAPE, nfft=8192, t_guard=1024, n_symb=64)         # a frame of 9 MB: the budget, not the grid, is the limit
    a = int(_ask(host_program, [_line("chunk", big, f64=1, fpp=10 ** 6, cap=0, width=1024)])[0].split()[0])
    assert a == sc.chunk_model(big, 1, 0, 0, 0, 10 ** 6, 0, 1024) and 1 <= a < 65535


def test_launch_shape_and_lds_budget(host_program):
    t4 = dict(sc.SHAPE, nfft=1024, t_guard=128, n_symb=5)
    combos = [(shape, f64, w, frames) for shape in (sc.SHAPE, t4) for f64 in (0, 1) for w in (1, 16, 32, 128, 1024)
              for frames in (1, 3, 65535)]
    got = _ask(host_program, [_line("pass", sh, f64=f, width=w, frames=m) for sh, f, w, m in combos])
    for (shape, f64, w, frames), g in zip(combos, got):
        assert tuple(map(int, g.split())) == sc.pass_model(shape, f64, w, frames), (f64, w, frames)
        threads, grid, lds, acc_threads, acc_grid = map(int, g.split())
        assert threads == 256 and grid == frames and lds <= sc.LDS_LIMIT
        assert (acc_grid - 2) * 64 < sc.n_out(shape, w) <= (acc_grid - 1) * 64      # the lags' workgroups, and one for the errors
    # the largest case, double at the widest window: 32 * 2049 + 16 * 1024 bytes, one workgroup per CU of 160 KiB
    lds = int(_ask(host_program, [_line("pass", t4, f64=1, width=sc.MAXW, frames=1)])[0].split()[2])
    assert lds == 81952 and lds <= sc.LDS_LIMIT and (160 << 10) // lds == 1
    assert (160 << 10) // sc.pass_model(t4, 0, sc.MAXW, 1)[2] == 3 and (160 << 10) // sc.pass_model(t4, 1, 128, 1)[2] == 3


def test_guard_phase_bin_against_unbounded_integers(host_program):
    """(TgPosition - 1 + sto) mod stride in 0 .. stride - 1, also where TgPosition - 1 + sto does not fit 64 bits."""
    strides = [1, 2, 72, 288, 1152, 9216, 1 << 62]                  # the header's sum of two remainders fits up to 2^62
    tgs = [1, 2, 65, 288, 289, 1152, 1153, I64_MAX]
    stos = [0, 1, -1, 7, -7, 287, 288, -288, -289, 150, 1 << 40, -(1 << 40), I64_MAX, -I64_MAX, -I64_MAX - 1]
    cases = [(t, s, m) for m in strides for t in tgs for s in stos]
    got = _ask(host_program, [_line("phase", tg=t, sto=s, stride=m) for t, s, m in cases])
    for (t, s, m), g in zip(cases, got):
        assert int(g) == sc.phase_bin(t, s, m) and 0 <= int(g) < m, (t, s, m, g)
    # a delay of sto samples moves the guard interval by -sto: the bin stays
    assert len({sc.phase_bin(17 - s, s, 288) for s in (-300, -1, 0, 5, 16)}) == 1


def test_wrapped_fractional_error_against_the_twin(host_program):
    """e = d - rint(d), d = FreqOffset - (cfo - rint(cfo)), bit for bit, at the ties (rint to even), across the wrap and for NaN."""
    rng = np.random.default_rng(7)
    fos = [0.0, 0.24, -0.24, 0.5, -0.5, 0.4999999999999999, 0.26, -0.26, 1e-17, float("nan")] + list(rng.uniform(-0.5, 0.5, 20))
    cfos = [0.0, 0.24, 0.5, 1.5, 2.5, -0.5, -1.5, 0.74, -0.74, 100.24, 0.49999999999999994, float("nan")] + list(rng.uniform(-3, 3, 20))
    cases = [(f, c) for f in fos for c in cfos]
    got = _ask(host_program, [_line("ffo", fo=float(f).hex(), cfo=float(c).hex()) for f, c in cases])
    for (f, c), g in zip(cases, got):
        want = sc.ffo_err(f, c)
        if np.isnan(want):
            assert "nan" in g, (f, c, g)
        else:
            assert float.fromhex(g) == want and np.signbit(float.fromhex(g)) == np.signbit(want), (f, c, g, want)
            assert abs(want) <= 0.5
    # ties to even: cfo 0.5 and 2.5 round down, 1.5 up
    assert sc.ffo_err(0.0, 0.5) == -0.5 and sc.ffo_err(0.0, 1.5) == 0.5 and sc.ffo_err(0.0, 2.5) == -0.5
    assert sc.ffo_err(0.24, 0.24) == 0.0 and sc.ffo_err(-0.25, 3.75) == 0.0
    assert abs(sc.ffo_err(0.49, -0.49) - (-0.02)) < 1e-15            # across the wrap: 0.98 is an error of -0.02


def test_every_refusal_text_is_in_the_header_and_the_header_is_free_of_the_device_runtime():
    src = open(HEADER).read()
    for fmt in ("%s: WidthWindow must be 1 .. %d (%lld)", "%s: a frame of %lld samples is shorter than WidthWindow + Nfft + 1 (%lld + %d + 1)",
                "%s: no output is given", "%s: n_frames must be 0 .. 2^31 - 1 (%lld)"):
        assert f'"{fmt}"' in src, fmt
    main = open(os.path.join(ROOT, "tests", "host", "sync_plan_main.cpp")).read()
    names = re.findall(r'"(\w+)"', re.search(r"IDS\[SYNC_REFUSALS\] = \{(.*?)\};", main, re.S).group(1))
    txf = open(os.path.join(CSRC, "txf_plan.hpp")).read()
    txf_enum = re.search(r"TXF_OK = 0,(.*?)TXF_REFUSALS", txf, re.S).group(1)
    # the front every study shares: its texts live in txf_plan.hpp, and the header calls it
    for fmt in ("%s: register entries must be 0 or 1",
                "%s: give h (one channel for every frame) or taps (a channel per frame), not both"):
        assert f'"{fmt}"' in txf and f'"{fmt}"' not in src, fmt
    assert "txf_study_prelude(" in src and "inline int txf_study_prelude(" in txf
    own = re.search(r"enum \{ SYNC_REFUSE_FRAMES = TXF_REFUSALS,(.*?)SYNC_REFUSALS \}", src, re.S).group(1)
    assert [n.upper() for n in names[1:]] == re.findall(r"TXF_REFUSE_(\w+)", txf_enum) + ["FRAMES"] + re.findall(r"SYNC_REFUSE_(\w+)", own)
    assert "hip/" not in src and "__global__" not in src and "hipLaunch" not in src
    assert set(re.findall(r'#include [<"]([^>"]+)[>"]', src)) <= {"cmath", "cstddef", "cstdint", "txf_plan.hpp"}
    hip = open(os.path.join(CSRC, "ofdm_sync_study.hip")).read()
    assert '#include "sync_plan.hpp"' in hip and "sync_rx_prelude(" in hip and "sync_study_prelude(" in hip
    assert "sync_chunk(" in hip and "sync_pass(" in hip and "TXF_WS_BUDGET" not in hip
    assert "sync_phase_bin(" in hip and "sync_ffo_err(" in hip      # the device code uses the header's definitions
    assert "hipfft" not in hip.lower() and "rocblas" not in hip.lower()
