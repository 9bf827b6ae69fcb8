"""The call plan of the fine-sync capture (csrc/fine_plan.hpp) on the CPU: tests/host/fine_plan_main.cpp is compiled with the host
compiler and the address and undefined-behaviour sanitizers into a stand-alone program and asked about the refusals of both entries
in their order, the length of `taus`, the chunk rule, the launch shape with its LDS budget, and the two frame functions -- the
timing error at the wrap and at the extremes of int64, the bin of the histogram with its tails and its NaN rule -- against the
Python twins of tests/fine_cases.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fine_cases as fc
import sync_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ofdm-course_amd", "csrc")
HEADER = os.path.join(CSRC, "fine_plan.hpp")
I64_MAX = (1 << 63) - 1


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no C++ compiler for the stand-alone program"
    exe = str(tmp_path_factory.mktemp("fine_plan") / "fine_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "fine_plan_main.cpp"), "-o", exe], check=True)
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
def test_rx_fine_first_refusal_wins_in_the_documented_order(host_program, f64):
    order, good = fc.rx_order(f64), fc.good_rx(f64)
    got = _ask(host_program, [_line("rx", fc.broken_from(good, order, i)) for i in range(len(order) + 1)])
    for i, (rid, _, msg) in enumerate(order):
        assert got[i] == f"refused {rid} {msg}", (i, rid, got[i])
    assert got[-1] == "ok"
    assert _ask(host_program, [_line("rx", good, plan=0)])[0] == "refused args rx_fine: bad arguments"
    ok = [dict(n_frames=0), dict(n_frames=(1 << 31) - 1), dict(variant=0), dict(np=2), dict(n_symb=1),
          dict(np=1 << 15, n_symb=(1 << 16) - 1)]
    assert _ask(host_program, [_line("rx", good, **o) for o in ok]) == ["ok"] * len(ok)
    bad = [(dict(variant=-1), "variant", "variant must be 0 (T5/fine_sync.m) or 1 (T4/fine_sync.m) (-1)"),
           (dict(np=0), "few_pilots", "fine_sync needs at least two pilot carriers (0)"),
           (dict(np=46341, n_symb=46341), "long", "Np * N_symb must be below 2^31 (2147488281)")]
    got = _ask(host_program, [_line("rx", good, **b) for b, _, _ in bad])
    for (b, rid, msg), g in zip(bad, got):
        assert g == f"refused {rid} rx_fine: {msg}", (b, g)


@pytest.mark.parametrize("f64", [0, 1])
def test_fine_study_first_refusal_wins_in_the_documented_order(host_program, f64):
    order, good = fc.study_order(f64), fc.good_study(f64)
    got = _ask(host_program, [_line("study", fc.broken_from(good, order, i)) for i in range(len(order) + 1)])
    for i, (rid, _, msg) in enumerate(order):
        assert got[i] == f"refused {rid} {msg}", (i, rid, got[i])
    assert got[-1] == "ok"
    assert _ask(host_program, [_line("study", good, plan=0)])[0] == "refused args fine_study: bad arguments"
    for brk in (dict(n_points=-1), dict(fpp=-1), dict(max_chunk=-1)):
        assert _ask(host_program, [_line("study", good, **brk)])[0] == "refused args fine_study: bad arguments"
    ok = [dict(n_points=0, points=0), dict(fpp=0), dict(reg="none"), dict(h="none"), dict(h="none", taps="0,3,7"), dict(h=64),
          dict(sto_mode=0, cfo_mode=0), dict(max_chunk=1), dict(max_chunk=65535), dict(td=0, fd=1), dict(td=1, fd=1), dict(variant=0),
          dict(bins_n=1, bins_lo=0.0, bins_hi=1e-300)]
    assert _ask(host_program, [_line("study", good, **o) for o in ok]) == ["ok"] * len(ok)
    bins = [dict(bins_n=-1), dict(bins_lo=4.0), dict(bins_lo=5.0), dict(bins_lo="nan"), dict(bins_hi="nan"), dict(bins_hi="inf"),
            dict(bins_lo="-inf")]
    assert [g.split()[1] for g in _ask(host_program, [_line("study", good, **b) for b in bins])] == ["bins"] * len(bins)
    got = _ask(host_program, [_line("study", good, np=1 << 16, n_symb=1 << 15)])[0]
    assert got == "refused long fine_study: Np * N_symb must be below 2^31 (2147483648)"


def test_channel_refusals_sit_between_the_two_channels_check_and_the_capture(host_program):
    good = fc.good_study(1)
    channel = [(brk, rid, msg.replace("sync_study", "fine_study")) for brk, rid, msg in sc.CHANNEL]
    got = _ask(host_program, [_line("study", good, **brk) for brk, _, _ in channel])
    for (brk, rid, msg), g in zip(channel, got):
        assert g == f"refused {rid} {msg}", (brk, g)
    got = _ask(host_program, [_line("study", good, **dict(brk, variant=2)) for brk, _, _ in channel])
    assert [g.split()[1] for g in got] == [rid for _, rid, _ in channel]
    assert _ask(host_program, [_line("study", good, h=65, taps="0,3")])[0].split()[1] == "both"


def test_length_of_taus(host_program):
    cases = [(np_, s, v) for np_ in (2, 3, 16, 68) for s in (1, 2, 5, 16) for v in (0, 1)]
    got = _ask(host_program, [_line("len", np=p, n_symb=s, variant=v) for p, s, v in cases])
    for (p, s, v), g in zip(cases, got):
        assert int(g) == fc.fine_len(p, s, v), (p, s, v, g)
    assert fc.fine_len(16, 1, 1) == 16 and fc.fine_len(16, 2, 1) == 31 and fc.fine_len(16, 2, 0) == 32     # one symbol: the T5 rule
    assert fc.fine_len(68, 16, "T4") == 1087 and fc.fine_len(68, 16, "T5") == 1088


def test_chunk_rule(host_program):
    """max(1, min(cap or BUDGET // (generator frame bytes with the RX region + the receiver's arena + the row, the mask and the
    scalars), frames_per_point, 65535)) on the Task-4 sweep's budget."""
    combos = [(f64, scr, imp, ft, fpp, cap, v) for f64 in (0, 1) for scr in (0, 1) for imp in (0, 1) for ft in (0, 3)
              for fpp in (1, 5, 10 ** 7) for cap in (0, 1, 3, 65535) for v in (0, 1)]
    got = _ask(host_program, [_line("chunk", fc.SHAPE, f64=f, scr=s, imp=i, fade_taps=t, fpp=p, cap=c, variant=v)
                              for f, s, i, t, p, c, v in combos])
    for (f64, scr, imp, ft, fpp, cap, v), g in zip(combos, got):
        chunk, rows = map(int, g.split())
        assert rows == 9 * (80 - v) + 64
        assert chunk == fc.chunk_model(fc.SHAPE, f64, scr, imp, ft, fpp, cap, v), (f64, scr, imp, ft, fpp, cap, v)
    big = dict(fc.SHAPE, nfft=8192, t_guard=1024, n_symb=64, n_carrier=4096, np=615)     # 9 MB frames: the budget is the limit
    a = int(_ask(host_program, [_line("chunk", big, f64=1, fpp=10 ** 6, cap=0, variant=1)])[0].split()[0])
    assert a == fc.chunk_model(big, 1, 0, 0, 0, 10 ** 6, 0, 1) and 1 <= a < 65535


def test_launch_shape_and_lds_budget(host_program):
    t4 = dict(fc.SHAPE, nfft=1024, t_guard=128, n_symb=16, n_carrier=400, np=68)
    combos = [(shape, v, frames) for shape in (fc.SHAPE, t4, dict(t4, n_symb=1)) for v in (0, 1) for frames in (1, 3, 65535)]
    got = _ask(host_program, [_line("pass", sh, variant=v, frames=m) for sh, v, m in combos])
    for (shape, v, frames), g in zip(combos, got):
        assert tuple(map(int, g.split())) == fc.pass_model(shape, v, frames), (v, frames)
        threads, grid, lds, trips, acc_threads, acc_grid, acc_lds = map(int, g.split())
        L = fc.fine_len(shape["np"], shape["n_symb"], v)
        assert threads == 256 and grid == frames and lds <= fc.LDS_LIMIT and acc_lds == 32768 <= fc.LDS_LIMIT
        assert (trips - 1) * 1024 < L <= trips * 1024 and (acc_grid - 2) * 64 < L <= (acc_grid - 1) * 64
    # the T4 geometry with 16 symbols: 1087 entries, a second trip of the 256 threads x 4 entries
    assert fc.pass_model(t4, 1, 1)[3] == 2 and fc.pass_model(fc.SHAPE, 1, 1)[3] == 1


def test_timing_error_at_the_wrap_and_at_the_extremes(host_program):
    """e = tau Nfft + phi_s + 1, phi_s in (-stride / 2, stride / 2]: phi = 0, stride / 2, stride - 1; negative Time_Delay; int64."""
    rng = np.random.default_rng(11)
    taus = [0.0, -1.0 / 1024, 8.0 / 1024, 3.0 / 256, 1e-17, float("nan")] + list(rng.uniform(-0.05, 0.05, 6))
    geo = [(1024, 1152), (256, 288), (64, 72), (64, 73)]                           # (an odd stride: no tie at the half)
    cases = []
    for nfft, stride in geo:
        for phi in (0, 1, stride // 2 - 1, stride // 2, stride // 2 + 1, stride - 2, stride - 1):
            for sto in (0, 12, -12, 150, -700, stride, -stride, 1 << 40, -(1 << 40), I64_MAX, -I64_MAX - 1):
                tg = (phi - sto) % stride + 1
                cases += [(t, tg, sto, nfft, stride, phi) for t in taus[:3]]
        cases += [(t, tg, 5, nfft, stride, None) for t in taus for tg in (1, 65, stride, I64_MAX)]
    got = _ask(host_program, [_line("err", tau=float(t).hex(), tg=tg, sto=s, nfft=n, stride=m) for t, tg, s, n, m, _ in cases])
    for (t, tg, s, n, m, phi), g in zip(cases, got):
        want = fc.tau_err(t, tg, s, n, m)
        if phi is not None:
            assert sc.phase_bin(tg, s, m) == phi
            phis = phi - m if 2 * phi > m else phi
            assert -m / 2 < phis <= m / 2 and want == np.float64(t) * n + (phis + 1)
        if np.isnan(want):
            assert "nan" in g
        else:
            assert float.fromhex(g) == want, (t, tg, s, n, m, g, want)
    # the oracle's clean frames (the issue): phi_s = 0 with tau Nfft = -0.9926 is e = 0.0074; phi_s = -4 with +3.0 is e = 0
    assert abs(fc.tau_err(-0.9926 / 1024, 1, 0, 1024, 1152) - 0.0074) < 1e-12
    assert fc.tau_err(3.0 / 256, 285, 0, 256, 288) == 0.0 and fc.phase_wrapped(285, 0, 288) == -4
    assert fc.phase_wrapped(145, 0, 288) == 144 and fc.phase_wrapped(146, 0, 288) == -143         # the half stays, the next wraps


def test_histogram_bin_with_tails_and_nan(host_program):
    rng = np.random.default_rng(5)
    grids = [(64, -4.0, 4.0), (1, 0.0, 1.0), (7, -1.0, 2.5), (1000, -1e-3, 1e-3)]
    cases = []
    for n, lo, hi in grids:
        w = (hi - lo) / n
        es = [lo, hi, np.nextafter(lo, -np.inf), np.nextafter(hi, -np.inf), np.nextafter(hi, np.inf), lo + w, lo + 3 * w,
              np.nextafter(lo + w, -np.inf), 0.0, -0.0, float("nan"), float("inf"), float("-inf"), 1e300, -1e300]
        cases += [(e, n, lo, hi) for e in es + list(rng.uniform(lo - w, hi + w, 40))]
    got = _ask(host_program, [_line("bin", e=float(e).hex() if np.isfinite(e) else e, n=n, lo=float(lo).hex(), hi=float(hi).hex())
                              for e, n, lo, hi in cases])
    for (e, n, lo, hi), g in zip(cases, got):
        assert int(g) == fc.fine_bin(e, n, lo, hi), (e, n, lo, hi, g)
        assert -3 <= int(g) < n
    assert fc.fine_bin(float("nan"), 64, -4, 4) == fc.NAN and fc.fine_bin(float("inf"), 64, -4, 4) == fc.NAN
    assert fc.fine_bin(-4.0, 64, -4, 4) == 0 and fc.fine_bin(4.0, 64, -4, 4) == fc.ABOVE and fc.fine_bin(-4.1, 64, -4, 4) == fc.BELOW
    assert fc.fine_bin(0.0, 64, -4, 4) == 32 and fc.fine_bin(np.nextafter(4.0, 0), 64, -4, 4) == 63
    hist, below, above, nan = fc.histogram([0.0, 0.01, -5, 9, float("nan"), 3.99], 64, -4.0, 4.0)
    assert hist.sum() + below + above + nan == 6 and (below, above, nan) == (1, 1, 1) and hist[32] == 2 and hist[63] == 1


def test_every_refusal_text_is_in_the_header_and_the_header_is_free_of_the_device_runtime():
    src = open(HEADER).read()
    for fmt in ("%s: variant must be 0 (T5/fine_sync.m) or 1 (T4/fine_sync.m) (%d)", "%s: fine_sync needs at least two pilot carriers (%d)",
                "%s: Np * N_symb must be below 2^31 (%lld)", "%s: no output is given", "%s: n_frames must be 0 .. 2^31 - 1 (%lld)",
                "%s: bins must have n >= 1 and finite lo < hi (%d, %g, %g)"):
        assert f'"{fmt}"' in src, fmt
    main = open(os.path.join(ROOT, "tests", "host", "fine_plan_main.cpp")).read()
    names = re.findall(r'"(\w+)"', re.search(r"IDS\[FINE_REFUSALS\] = \{(.*?)\};", main, re.S).group(1))
    txf = open(os.path.join(CSRC, "txf_plan.hpp")).read()
    txf_enum = re.search(r"TXF_OK = 0,(.*?)TXF_REFUSALS", txf, re.S).group(1)
    # the front every study shares: its texts live in txf_plan.hpp, and the header calls it
    for fmt in ("%s: register entries must be 0 or 1",
                "%s: give h (one channel for every frame) or taps (a channel per frame), not both"):
        assert f'"{fmt}"' in txf and f'"{fmt}"' not in src, fmt
    assert "txf_study_prelude(" in src and "inline int txf_study_prelude(" in txf
    own = re.search(r"enum \{ FINE_REFUSE_FRAMES = TXF_REFUSALS,(.*?)FINE_REFUSALS \}", src, re.S).group(1)
    mine = [n.replace("PILOTS", "FEW_PILOTS") for n in re.findall(r"FINE_REFUSE_(\w+)", own)]
    assert [n.upper() for n in names[1:]] == re.findall(r"TXF_REFUSE_(\w+)", txf_enum) + ["FRAMES"] + mine
    assert "hip/" not in src and "__global__" not in src and "hipLaunch" not in src
    assert set(re.findall(r'#include [<"]([^>"]+)[>"]', src)) <= {"cmath", "cstddef", "cstdint", "sync_plan.hpp"}
