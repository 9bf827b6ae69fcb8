"""The call plan of the spectrum capture (csrc/spectrum_plan.hpp) on the CPU: tests/host/spectrum_plan_main.cpp is compiled with the
host compiler and the address and undefined-behaviour sanitizers into a stand-alone program and asked about the refusals of both
entries in their order, the end-of-window comparison at the extremes of int64, the chunk rule and the launch shape
(tests/spectrum_cases.py)."""
import os
import re
import shutil
import subprocess

import pytest

import spectrum_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ofdm-course_amd", "csrc")
HEADER = os.path.join(CSRC, "spectrum_plan.hpp")
I64_MAX = (1 << 63) - 1


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no C++ compiler for the stand-alone program"
    exe = str(tmp_path_factory.mktemp("spectrum_plan") / "spectrum_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "spectrum_plan_main.cpp"), "-o", exe], check=True)
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
def test_rx_spectrum_first_refusal_wins_in_the_documented_order(host_program, f64):
    order, good = sc.rx_order(f64), sc.good_rx(f64)
    got = _ask(host_program, [_line("rx", sc.broken_from(good, order, i)) for i in range(len(order) + 1)])
    for i, (rid, _, msg) in enumerate(order):
        assert got[i] == f"refused {rid} {msg}", (i, rid, got[i])
    assert got[-1] == "ok"
    assert _ask(host_program, [_line("rx", good, plan=0)])[0] == "refused args rx_spectrum: bad arguments"
    ok = [dict(n_frames=0), dict(n_frames=(1 << 31) - 1), dict(first=0), dict(first=1), dict(first=sc.FRAME_SAMPLES - 256),
          dict(first=0, n_windows=5), dict(first=32, n_windows=5), dict(first=300, n_windows=4)]
    assert _ask(host_program, [_line("rx", good, **o) for o in ok]) == ["ok"] * len(ok)


@pytest.mark.parametrize("f64", [0, 1])
def test_spectrum_study_first_refusal_wins_in_the_documented_order(host_program, f64):
    order, good = sc.study_order(f64), sc.good_study(f64)
    got = _ask(host_program, [_line("study", sc.broken_from(good, order, i)) for i in range(len(order) + 1)])
    for i, (rid, _, msg) in enumerate(order):
        assert got[i] == f"refused {rid} {msg}", (i, rid, got[i])
    assert got[-1] == "ok"
    assert _ask(host_program, [_line("study", good, plan=0)])[0] == "refused args spectrum_study: bad arguments"
    for brk in (dict(n_points=-1), dict(fpp=-1)):
        assert _ask(host_program, [_line("study", good, **brk)])[0] == "refused args spectrum_study: bad arguments"
    ok = [dict(n_points=0, points=0), dict(fpp=0), dict(reg="none"), dict(h="none"), dict(h="none", taps="0,3,7"), dict(h=64),
          dict(sto_mode=0, cfo_mode=0), dict(max_chunk=1), dict(frame0=(1 << 32) - 6), dict(first=0), dict(n_windows=1)]
    assert _ask(host_program, [_line("study", good, **o) for o in ok]) == ["ok"] * len(ok)


def test_channel_refusals_sit_between_the_two_channels_check_and_the_capture(host_program):
    good = sc.good_study(1)
    got = _ask(host_program, [_line("study", good, **brk) for brk, _, _ in sc.CHANNEL])
    for (brk, rid, msg), g in zip(sc.CHANNEL, got):
        assert g == f"refused {rid} {msg}", (brk, g)
    # behind "h and taps together", in front of the capture
    got = _ask(host_program, [_line("study", good, **dict(brk, first=-1)) for brk, _, _ in sc.CHANNEL])
    assert [g.split()[1] for g in got] == [rid for _, rid, _ in sc.CHANNEL]
    assert _ask(host_program, [_line("study", good, h=65, taps="0,3")])[0].split()[1] == "both"


def test_end_of_window_comparison_against_unbounded_integers(host_program):
    """first + (n_windows - 1) (Nfft + T_guard) + Nfft <= frame_samples, also where the left side does not fit 64 bits."""
    geoms = [(256, 32, 5), (64, 0, 1), (64, 64, 2), (8192, 8192, 3), (1024, 80, 3)]
    cases = []
    for nfft, tg, ns in geoms:
        stride, fs = nfft + tg, (nfft + tg) * ns
        firsts = [0, 1, tg, tg + stride, fs - nfft, fs - nfft + 1, fs - nfft - 1, stride - 1, fs, I64_MAX, I64_MAX - 1, I64_MAX - nfft,
                  I64_MAX // stride, 1 << 62]
        counts = [1, 2, ns, ns + 1, ns - 1, I64_MAX, I64_MAX - 1, I64_MAX // stride, I64_MAX // stride + 1, I64_MAX // stride + 2,
                  1 << 62, (1 << 62) // stride]
        cases += [(nfft, tg, ns, f, w) for f in firsts for w in counts if f >= 0 and w >= 1]
    got = _ask(host_program, [_line("capture", sc.SHAPE, nfft=n, t_guard=t, n_symb=s, first=f, n_windows=w, out=1)
                              for n, t, s, f, w in cases])
    accepted = 0
    for (n, t, s, f, w), g in zip(cases, got):
        want = sc.end_ok(n, t, s, f, w)
        assert (g == "ok") == want, (n, t, s, f, w, g)
        if not want:
            assert g == f"refused end rx_spectrum: {w} windows from sample {f} on end behind the frame of {(n + t) * s} samples"
        accepted += want
    assert accepted >= 5 * len(geoms)                                # both answers are exercised
    # the last start that fits, and one more window than fit
    assert _ask(host_program, [_line("capture", sc.SHAPE, first=sc.FRAME_SAMPLES - 256, n_windows=1, out=1),
                               _line("capture", sc.SHAPE, first=sc.FRAME_SAMPLES - 255, n_windows=1, out=1),
                               _line("capture", sc.SHAPE, first=32, n_windows=5, out=1),
                               _line("capture", sc.SHAPE, first=33, n_windows=5, out=1)]) == \
        ["ok", "refused end rx_spectrum: 1 windows from sample 1185 on end behind the frame of 1440 samples", "ok",
         "refused end rx_spectrum: 5 windows from sample 33 on end behind the frame of 1440 samples"]


def test_chunk_rule(host_program):
    """max(1, min(cap or BUDGET // (generator frame bytes with the RX region + the power rows), frames_per_point, 65535))."""
    combos = [(f64, scr, imp, ft, fpp, cap, peak) for f64 in (0, 1) for scr in (0, 1) for imp in (0, 1) for ft in (0, 3)
              for fpp in (1, 5, 10 ** 7) for cap in (0, 1, 3, 65535, 10 ** 7) for peak in (0, 1)]
    got = _ask(host_program, [_line("chunk", sc.SHAPE, f64=f, scr=s, imp=i, fade_taps=t, fpp=p, cap=c, peak=k)
                              for f, s, i, t, p, c, k in combos])
    for (f64, scr, imp, ft, fpp, cap, peak), g in zip(combos, got):
        chunk, fb, rows = map(int, g.split())
        assert fb == sc.frame_bytes(sc.SHAPE, f64, scr, imp, ft) and rows == 8 * 256 * (2 if peak else 1)
        assert chunk == sc.chunk_model(sc.SHAPE, f64, scr, imp, ft, fpp, cap, peak), (f64, scr, imp, ft, fpp, cap, peak)
    big = dict(sc.SHAPE, nfft=8192, t_guard=8192, n_symb=64)         # a frame of 16 MB: the budget, not the grid, is the limit
    a, b = (int(_ask(host_program, [_line("chunk", big, f64=1, fpp=10 ** 6, cap=0, peak=k)])[0].split()[0]) for k in (0, 1))
    assert a == sc.chunk_model(big, 1, 0, 0, 0, 10 ** 6, 0, 0) and b == sc.chunk_model(big, 1, 0, 0, 0, 10 ** 6, 0, 1)
    assert 1 <= b <= a < 65535


def test_launch_shape_of_every_transform_size(host_program):
    combos = [(nfft, f64, frames) for nfft in (64, 128, 256, 512, 1024, 2048, 4096, 8192) for f64 in (0, 1)
              for frames in (1, 3, 31, 32, 33, 65535, (1 << 31) - 1)]
    got = _ask(host_program, [_line("pass", sc.SHAPE, nfft=n, f64=f, frames=m) for n, f, m in combos])
    for (nfft, f64, frames), g in zip(combos, got):
        assert tuple(map(int, g.split())) == sc.pass_model(nfft, f64, frames), (nfft, f64, frames)
        threads, per_wg, lds, grid, _, acc_grid = map(int, g.split())
        assert threads <= 1024 and threads == per_wg * nfft // 8 and lds <= 160 << 10
        assert (grid - 1) * per_wg < frames <= grid * per_wg         # the last workgroup may be partial, never empty
        assert acc_grid * 64 == nfft                                 # 64 bins per workgroup of the accumulate kernel


def test_every_refusal_text_is_in_the_header_and_the_header_is_free_of_the_device_runtime():
    src = open(HEADER).read()
    for fmt in ("%s: first must be >= 0 (%lld)", "%s: n_windows must be >= 1 (%lld)",
                "%s: %lld windows from sample %lld on end behind the frame of %lld samples", "%s: no output is given",
                "%s: n_frames must be 0 .. 2^31 - 1 (%lld)"):
        assert f'"{fmt}"' in src, fmt
    main = open(os.path.join(ROOT, "tests", "host", "spectrum_plan_main.cpp")).read()
    names = re.findall(r'"(\w+)"', re.search(r"IDS\[SPEC_REFUSALS\] = \{(.*?)\};", main, re.S).group(1))
    txf = open(os.path.join(CSRC, "txf_plan.hpp")).read()
    txf_enum = re.search(r"TXF_OK = 0,(.*?)TXF_REFUSALS", txf, re.S).group(1)
    # the front every study shares: its texts live in txf_plan.hpp, and the header calls it
    for fmt in ("%s: register entries must be 0 or 1",
                "%s: give h (one channel for every frame) or taps (a channel per frame), not both"):
        assert f'"{fmt}"' in txf and f'"{fmt}"' not in src, fmt
    assert "txf_study_prelude(" in src and "inline int txf_study_prelude(" in txf
    own = re.search(r"enum \{ SPEC_REFUSE_FRAMES = TXF_REFUSALS,(.*?)SPEC_REFUSALS \}", src, re.S).group(1)
    assert [n.upper() for n in names[1:]] == re.findall(r"TXF_REFUSE_(\w+)", txf_enum) + ["FRAMES"] + re.findall(r"SPEC_REFUSE_(\w+)", own)
    assert "hip/" not in src and "__global__" not in src and "hipLaunch" not in src and "__device__" not in src
    assert set(re.findall(r'#include [<"]([^>"]+)[>"]', src)) <= {"algorithm", "cstddef", "cstdint", "txf_plan.hpp"}
    hip = open(os.path.join(CSRC, "ofdm_spectrum.hip")).read()
    assert '#include "spectrum_plan.hpp"' in hip and "spectrum_rx_prelude(" in hip and "spectrum_study_prelude(" in hip
    assert "spectrum_chunk(" in hip and "spectrum_pass(" in hip and "TXF_WS_BUDGET" not in hip
    assert "hipfft" not in hip.lower() and "atomic" not in hip.split('#include "txf_study.hpp"')[1]
