"""The call plan of the integer-CFO capture (csrc/ifo_plan.hpp) on the CPU: tests/host/ifo_plan_main.cpp is compiled with the host
compiler and the address and undefined-behaviour sanitizers into a stand-alone program and asked about the refusals of both entries
in their order, the chunk rule, the launch shape with its LDS budget, and the two frame functions -- the bin of IFO -
rint(Freq_Shift) at its ties and edges and the total error -- against the Python twins of tests/ifo_cases.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ifo_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ofdm-course_amd", "csrc")
HEADER = os.path.join(CSRC, "ifo_plan.hpp")


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no C++ compiler for the stand-alone program"
    exe = str(tmp_path_factory.mktemp("ifo_plan") / "ifo_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "ifo_plan_main.cpp"), "-o", exe], check=True)
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
def test_rx_ifo_first_refusal_wins_in_the_documented_order(host_program, f64):
    order, good = ic.rx_order(f64), ic.good_rx(f64)
    got = _ask(host_program, [_line("rx", ic.broken_from(good, order, i)) for i in range(len(order) + 1)])
    for i, (rid, _, msg) in enumerate(order):
        assert got[i] == f"refused {rid} {msg}", (i, rid, got[i])
    assert got[-1] == "ok"
    assert _ask(host_program, [_line("rx", good, plan=0)])[0] == "refused args rx_ifo: bad arguments"
    ok = [dict(n_frames=0), dict(n_frames=(1 << 31) - 1), dict(stage=0), dict(time_desync=0), dict(stage=0, time_desync=0),
          dict(n_symb=2), dict(err_span=0), dict(np=2)]             # 2 symbols of 288 hold 512 samples; the span is the study's
    assert _ask(host_program, [_line("rx", good, **o) for o in ok]) == ["ok"] * len(ok)
    bad = [(dict(stage=-1), "stage", "stage must be 0 (the received frame) or 1 (the receiver's stream) (-1)"),
           (dict(time_desync=-1), "time_desync", "time_desync must be 0 or 1 (-1)"),
           (dict(n_symb=1), "short", "rx_signal(Nfft+1:2*Nfft) exceeds the frame"),
           (dict(n_symb=2, t_guard=0, nfft=256), "route", "rx_chain_task4: frame shorter than T_guard + Nfft, or T_guard outside 1..1024"),
           (dict(nfft=4096, t_guard=2048, n_symb=2), "route",
            "rx_chain_task4: frame shorter than T_guard + Nfft, or T_guard outside 1..1024")]
    got = _ask(host_program, [_line("rx", good, **b) for b, _, _ in bad])
    for (b, rid, msg), g in zip(bad, got):
        assert g == f"refused {rid} rx_ifo: {msg}", (b, g)


@pytest.mark.parametrize("f64", [0, 1])
def test_ifo_study_first_refusal_wins_in_the_documented_order(host_program, f64):
    order, good = ic.study_order(f64), ic.good_study(f64)
    got = _ask(host_program, [_line("study", ic.broken_from(good, order, i)) for i in range(len(order) + 1)])
    for i, (rid, _, msg) in enumerate(order):
        assert got[i] == f"refused {rid} {msg}", (i, rid, got[i])
    assert got[-1] == "ok"
    assert _ask(host_program, [_line("study", good, plan=0)])[0] == "refused args ifo_study: bad arguments"
    for brk in (dict(n_points=-1), dict(fpp=-1)):
        assert _ask(host_program, [_line("study", good, **brk)])[0] == "refused args ifo_study: bad arguments"
    ok = [dict(n_points=0, points=0), dict(fpp=0), dict(reg="none"), dict(h="none"), dict(h="none", taps="0,3,7"), dict(h=64),
          dict(sto_mode=0, cfo_mode=0), dict(max_chunk=1), dict(frame0=(1 << 32) - 6), dict(err_span=1), dict(err_span=4096),
          dict(stage=0), dict(time_desync=0)]
    assert _ask(host_program, [_line("study", good, **o) for o in ok]) == ["ok"] * len(ok)
    bad = [(dict(err_span=-1), "err_span must be 1 .. 4096 (-1)"), (dict(err_span=4097), "err_span must be 1 .. 4096 (4097)")]
    got = _ask(host_program, [_line("study", good, **b) for b, _ in bad])
    assert got == [f"refused span ifo_study: {msg}" for _, msg in bad]


def test_channel_refusals_sit_between_the_two_channels_check_and_the_capture(host_program):
    good = ic.good_study(1)
    got = _ask(host_program, [_line("study", good, **brk) for brk, _, _ in ic.CHANNEL])
    for (brk, rid, msg), g in zip(ic.CHANNEL, got):
        assert g == f"refused {rid} {msg}", (brk, g)
    got = _ask(host_program, [_line("study", good, **dict(brk, stage=2)) for brk, _, _ in ic.CHANNEL])
    assert [g.split()[1] for g in got] == [rid for _, rid, _ in ic.CHANNEL]
    assert _ask(host_program, [_line("study", good, h=65, taps="0,3")])[0].split()[1] == "both"


def test_chunk_rule(host_program):
    """max(1, min(cap or BUDGET // (generator frame bytes with the RX region + the row, the mask and the scalars), frames_per_point,
    65535))."""
    combos = [(f64, scr, imp, ft, fpp, cap) for f64 in (0, 1) for scr in (0, 1) for imp in (0, 1) for ft in (0, 3)
              for fpp in (1, 5, 10 ** 7) for cap in (0, 1, 3, 65535, 10 ** 7)]
    got = _ask(host_program, [_line("chunk", ic.SHAPE, f64=f, scr=s, imp=i, fade_taps=t, fpp=p, cap=c) for f, s, i, t, p, c in combos])
    for (f64, scr, imp, ft, fpp, cap), g in zip(combos, got):
        chunk, fb, rows = map(int, g.split())
        assert fb == ic.frame_bytes(ic.SHAPE, f64, scr, imp, ft) and rows == 9 * 256 + 40
        assert chunk == ic.chunk_model(ic.SHAPE, f64, scr, imp, ft, fpp, cap), (f64, scr, imp, ft, fpp, cap)
    big = dict(ic.SHAPE, nfft=8192, t_guard=1024, n_symb=64)         # a frame of 9 MB: the budget, not the grid, is the limit
    a = int(_ask(host_program, [_line("chunk", big, f64=1, fpp=10 ** 6, cap=0)])[0].split()[0])
    assert a == ic.chunk_model(big, 1, 0, 0, 0, 10 ** 6, 0) and 1 <= a < 65535


def test_launch_shape_and_lds_budget(host_program):
    combos = [(n, f64, frames) for n in (64, 128, 256, 512, 1024, 2048, 4096, 8192) for f64 in (0, 1) for frames in (1, 3, 33, 65535)]
    got = _ask(host_program, [_line("pass", ic.SHAPE, nfft=n, f64=f, frames=m) for n, f, m in combos])
    for (n, f64, frames), g in zip(combos, got):
        assert tuple(map(int, g.split())) == ic.pass_model(dict(ic.SHAPE, nfft=n), f64, frames), (n, f64, frames)
        threads, per, lds, grid, acc_threads, acc_grid, acc_lds = map(int, g.split())
        assert threads % 64 == 0 and threads <= 1024 and per * (n // 8) == threads     # whole wavefronts, all of them busy
        assert (grid - 1) * per < frames <= grid * per and lds <= ic.LDS_LIMIT and acc_lds <= ic.LDS_LIMIT
        assert (acc_grid - 1) * 64 == n
        assert (per == 1) == (n >= 2048)                              # one workgroup per frame from Nfft 2048 on
    lds = int(_ask(host_program, [_line("pass", ic.SHAPE, nfft=8192, f64=1, frames=1)])[0].split()[2])
    assert lds == 16 * (8192 + 1024 + 8) + 128 == 147712 and lds <= ic.LDS_LIMIT


def test_error_bin_against_the_twin(host_program):
    """IFO - rint(Freq_Shift) with ties to even, at the edges of the span and for a draw that is not a number."""
    cfos = [0.0, 0.24, 0.5, 1.5, 2.5, -0.5, 3.49999, 3.5, 30.5, 29.5, 12.76, -2.5, 1e9, float("nan"), float("inf")]
    cases = [(i, c, s) for i in (0, 1, 2, 3, 4, 29, 30, 31, 255, 4095, 8191) for c in cfos for s in (1, 2, 32, 4096)]
    got = _ask(host_program, [_line("errbin", ifo=i, cfo=float(c).hex(), span=s) for i, c, s in cases])
    for (i, c, s), g in zip(cases, got):
        assert int(g) == ic.err_bin(i, c, s), (i, c, s, g)
        assert int(g) in (ic.ERR_BELOW, ic.ERR_ABOVE) or 0 <= int(g) <= 2 * s
    # ties to even: 0.5 and 2.5 round down, 1.5 and 3.5 up; the middle bin is a hit; the edges are inside
    assert ic.err_bin(0, 0.5, 4) == 4 and ic.err_bin(2, 1.5, 4) == 4 and ic.err_bin(2, 2.5, 4) == 4 and ic.err_bin(4, 3.5, 4) == 4
    assert ic.err_bin(0, 4.0, 4) == 0 and ic.err_bin(0, 5.0, 4) == ic.ERR_BELOW
    assert ic.err_bin(8, 4.0, 4) == 8 and ic.err_bin(9, 4.0, 4) == ic.ERR_ABOVE and ic.err_bin(3, float("nan"), 4) == ic.ERR_ABOVE


def test_total_error_against_the_twin(host_program):
    rng = np.random.default_rng(11)
    fos = [0.0, 0.24, -0.26, 0.5, 1e-17, float("nan")] + list(rng.uniform(-0.5, 0.5, 12))
    cfos = [0.0, 0.24, 25.24, 30.5, -0.5] + list(rng.uniform(-0.5, 30.5, 12))
    cases = [(f, i, c) for f in fos for i in (0, 1, 25, 30, 255) for c in cfos]
    got = _ask(host_program, [_line("total", fo=float(f).hex(), ifo=i, cfo=float(c).hex()) for f, i, c in cases])
    for (f, i, c), g in zip(cases, got):
        want = ic.cfo_total_err(f, i, c)
        if np.isnan(want):
            assert "nan" in g
        else:
            assert float.fromhex(g) == want and np.signbit(float.fromhex(g)) == np.signbit(want), (f, i, c, g, want)
    assert abs(ic.cfo_total_err(0.24, 25, 25.24)) < 1e-14


def test_every_refusal_text_is_in_the_header_and_the_header_is_free_of_the_device_runtime():
    src = open(HEADER).read()
    for fmt in ("%s: stage must be 0 (the received frame) or 1 (the receiver's stream) (%d)", "%s: time_desync must be 0 or 1 (%d)",
                "%s: rx_signal(Nfft+1:2*Nfft) exceeds the frame", "%s: err_span must be 1 .. %lld (%lld)", "%s: no output is given",
                "%s: n_frames must be 0 .. 2^31 - 1 (%lld)"):
        assert f'"{fmt}"' in src, fmt
    route = open(os.path.join(CSRC, "t4_route.hpp")).read()
    assert '"rx_chain_task4: rx_signal(Nfft+1:2*Nfft) exceeds the frame"' in route      # the wording the short frame borrows
    main = open(os.path.join(ROOT, "tests", "host", "ifo_plan_main.cpp")).read()
    names = re.findall(r'"(\w+)"', re.search(r"IDS\[IFO_REFUSALS\] = \{(.*?)\};", main, re.S).group(1))
    txf = open(os.path.join(CSRC, "txf_plan.hpp")).read()
    txf_enum = re.search(r"TXF_OK = 0,(.*?)TXF_REFUSALS", txf, re.S).group(1)
    # the front every study shares: its texts live in txf_plan.hpp, and the header calls it
    for fmt in ("%s: register entries must be 0 or 1",
                "%s: give h (one channel for every frame) or taps (a channel per frame), not both"):
        assert f'"{fmt}"' in txf and f'"{fmt}"' not in src, fmt
    assert "txf_study_prelude(" in src and "inline int txf_study_prelude(" in txf
    own = re.search(r"enum \{ IFO_REFUSE_FRAMES = TXF_REFUSALS,(.*?)IFO_REFUSALS \}", src, re.S).group(1)
    assert [n.upper() for n in names[1:]] == re.findall(r"TXF_REFUSE_(\w+)", txf_enum) + ["FRAMES"] + re.findall(r"IFO_REFUSE_(\w+)", own)
    assert "hip/" not in src and "__global__" not in src and "hipLaunch" not in src
    assert set(re.findall(r'#include [<"]([^>"]+)[>"]', src)) <= {"algorithm", "cmath", "cstddef", "cstdint", "sync_plan.hpp"}
    hip = open(os.path.join(CSRC, "ofdm_ifo_study.hip")).read()
    assert '#include "ifo_plan.hpp"' in hip and "ifo_rx_prelude(" in hip and "ifo_study_prelude(" in hip
    assert "ifo_chunk(" in hip and "ifo_pass(" in hip and "TXF_WS_BUDGET" not in hip
    assert "ifo_err_bin(" in hip and "cfo_total_err(" in hip       # the device code uses the header's definitions
    assert "t4_rotate<T>(t4_raw<T>(" in hip and "wg_fft<T, N, false>" in hip
    t4 = open(os.path.join(CSRC, "ofdm_chain_t4.hip")).read()
    assert '#include "t4_stream.hpp"' in t4 and "cx<T> t4_raw(" not in t4 and "cx<T> t4_rotate(" not in t4   # shared, not restated
    assert "hipfft" not in hip.lower() and "rocblas" not in hip.lower()
