"""The call plan of the fused frame generator and the BER sweeps (csrc/txf_plan.hpp) on the CPU: tests/host/txf_plan_main.cpp is
compiled with the host compiler and the address and undefined-behaviour sanitizers into a stand-alone program and asked about
the workspace (bytes per frame, the layout of a chunk, the chunk rule), the channel of a call, the channel pass and the
refusals of every entry family (tests/txf_cases.py).  The sizes are restated here from the formulas of the commit before the
header: a region added to one of them and not the other fails here, without a GPU."""
import itertools
import math
import os
import re
import shutil
import struct
import subprocess

import pytest

import txf_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ofdm-course_amd", "csrc")
BPS = {"QPSK": 2, "8PSK": 3, "16QAM": 4, "64QAM": 6, "256QAM": 8}
BUDGET = 2 << 30
REGIONS = ("tx", "partial", "b0", "b1", "rx", "ref", "sto", "cfo", "amp", "hest")       # the parent's order
CHUNKS = (1, 7, 65535)


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no C++ compiler for the stand-alone program"
    exe = str(tmp_path_factory.mktemp("txf_plan") / "txf_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "txf_plan_main.cpp"), "-o", exe], check=True)
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


def _geometries():
    from ofdm_course_amd import frames as fr
    cfgs = [fr.config_M(), fr.config_C3(), fr.config_C5(), fr.config_small(),
            fr.config_small(nfft=256, n_carrier=64, comb=4, const="QPSK", n_symb=3, dominant_taps=3),
            fr.config_small(nfft=1024, n_carrier=400, comb=8, const="8PSK", n_symb=3, dominant_taps=3)]
    out = []
    for c in cfgs:
        nd, bps = len(c.dataCarriers), BPS[c.Constellation]
        out.append(dict(nfft=c.Nfft, t_guard=c.T_guard, n_symb=c.N_symb, n_carrier=c.N_carrier, np=len(c.pilotCarriers), nd=nd,
                        bps=bps, frame_words=(nd * c.N_symb * bps + 31) // 32))
    assert [(g["nfft"], g["bps"]) for g in out] == [(2048, 6), (2048, 6), (8192, 8), (256, 4), (256, 2), (1024, 3)]
    return out


def _uses():
    return [dict(scr=s, sweep=w, imp=i, fade_taps=t, hest=h)
            for s, w, i, t, h in itertools.product((0, 1), (0, 1), (0, 1), (0, 1, 9, 64), (0, 1))]


def _shapes():
    return [dict(g, f64=f) for g in _geometries() for f in (0, 1)]


def _per_frame(s, u):
    """The bytes per frame of each region, as txf_frame_bytes and txf_workspace of the parent wrote them (twice)."""
    cs = 16 if s["f64"] else 8
    fs = (s["nfft"] + s["t_guard"]) * s["n_symb"]
    frame_bits = s["nd"] * s["n_symb"] * s["bps"]
    return [cs * fs, 8 * s["n_symb"], frame_bits * u["scr"], frame_bits * u["scr"], cs * fs * u["sweep"],
            4 * s["frame_words"] * u["sweep"], 8 * u["imp"], 8 * u["imp"], 16 * u["fade_taps"], cs * s["n_carrier"] * u["hest"]]


def _frame_bytes(s, u):
    cs = 16 if s["f64"] else 8
    fs = (s["nfft"] + s["t_guard"]) * s["n_symb"]
    frame_bits = s["nd"] * s["n_symb"] * s["bps"]
    return (cs * fs * (2 if u["sweep"] else 1) + 8 * s["n_symb"] + (2 * frame_bits if u["scr"] else 0) +
            (4 * s["frame_words"] if u["sweep"] else 0) + (16 if u["imp"] else 0) + 16 * u["fade_taps"] +
            (cs * s["n_carrier"] if u["hest"] else 0))


def _a256(b):
    return (b + 255) & ~255


def test_frame_bytes_and_layout_are_the_parents(host_program):
    combos = [(s, u, ch) for s in _shapes() for u in _uses() for ch in CHUNKS]
    got = _ask(host_program, [_line("layout", s, u, ch=ch) for s, u, ch in combos])
    assert len(combos) == 6 * 2 * 64 * 3                    # geometries, precisions, uses, chunk sizes
    for (s, u, ch), g in zip(combos, got):
        w = g.split()
        frame_bytes, total = int(w[0]), int(w[1])
        regions = [tuple(map(int, x.split(":"))) for x in w[2:]]
        assert len(regions) == len(REGIONS)
        assert frame_bytes == _frame_bytes(s, u) == sum(_per_frame(s, u)), (s, u)
        # the parent's need: every region of ch frames padded to 256 bytes, carved in the parent's order
        sizes = [_a256(b * ch) for b in _per_frame(s, u)]
        assert [b for _, b in regions] == sizes, (s, u, ch)
        off = 0
        for (o, b), pf in zip(regions, _per_frame(s, u)):
            assert o == off and o % 256 == 0 and (b == 0) == (pf == 0)          # in order, aligned, disjoint, absent = empty
            off += b
        assert total == off == sum(sizes)
        assert ch * frame_bytes + 256 * len(REGIONS) >= total                   # what a chunk is budgeted with holds it


def test_chunk_rule(host_program):
    """Generator and Task-5 sweep: max(1, min(cap or BUDGET // frame_bytes, frames, 65535)); the Task-4 sweep: twice the budget
    over frame_bytes + t4_frame_bytes (+ 16 with the per-frame MER sums)."""
    combos = [(s, u, fr_, cap, t4, mer) for s in _shapes() for u in _uses() for fr_ in (0, 1, 5, 10 ** 6) for cap in (0, 2, 65535)
              for t4, mer in ((0, 0), (1, 0), (1, 1)) if not t4 or (u["sweep"] and u["imp"])]
    got = _ask(host_program, [_line("chunk", s, u, frames=f, cap=c, t4=t4, mer=mer) for s, u, f, c, t4, mer in combos])
    for (s, u, frames, cap, t4, mer), g in zip(combos, got):
        fb = _frame_bytes(s, u)
        if t4:
            cs = 16 if s["f64"] else 8
            ln = (s["nfft"] + s["t_guard"]) * s["n_symb"]
            t4b = cs * (ln + s["nfft"] * s["n_symb"] + s["np"] * s["n_symb"] + 2 * s["nfft"] + s["np"] + s["n_carrier"]) + 128 + 4 * s["frame_words"]
            default = max(1, 2 * BUDGET // (fb + t4b + (16 if mer else 0)))
        else:
            default = max(1, BUDGET // fb)
        assert int(g) == max(1, min(cap or default, frames, 65535)), (s, u, frames, cap, t4, mer)


def _dbits(v):
    return f"{struct.unpack('<Q', struct.pack('<d', v))[0]:016x}"


def test_static_channel(host_program):
    taps = "0:1:0,1:0:0,3:0.5:-0.25,7:0:0.125"
    lines = [_line("channel", f64=f, h_len=8, h_taps=taps) for f in (0, 1)]
    lines += [_line("channel", f64=1, h="null", h_len=0), _line("channel", f64=0, h="x", h_len=0),
              _line("channel", f64=1, h_len=6), _line("channel", f64=1, h="null", h_len=3), _line("channel", f64=1, h_len=-1),
              _line("channel", f64=0, h_len=4097, h_taps="4096:1:0"), _line("channel", f64=0, h_len=4098, h_taps="4097:1:0"),
              _line("channel", f64=1, h_len=64, h_taps=",".join(f"{i}:1:0" for i in range(64))),
              _line("channel", f64=1, h_len=65, h_taps=",".join(f"{i}:1:0" for i in range(65)))]
    got = _ask(host_program, lines)
    kept = " ".join(f"{d}:{_dbits(re_)}:{_dbits(im)}" for d, re_, im in ((0, 1.0, 0.0), (3, 0.5, -0.25), (7, 0.0, 0.125)))
    assert got[0] == got[1] == f"ok 7 3 {kept}"                       # exact zeros skipped, halo = the largest delay
    unit = f"ok 0 1 0:{_dbits(1.0)}:{_dbits(0.0)}"
    assert got[2] == got[3] == unit                                   # null or empty h: one unit tap
    assert got[4] == "ok 0 0"                                         # an all-zero h: no taps
    assert got[5] == got[6] == "refused channel " + tc.message("channel", None)
    assert got[7].startswith("ok 4096 1 4096:")
    assert got[8] == "refused tap_delay " + tc.message("tap_delay", None, (4097, 4096))
    assert got[9].startswith("ok 63 64 ")
    assert got[10] == "refused tap_count " + tc.message("tap_count", None, (65, 64))


def test_fading_line(host_program):
    delays, powers = [7, 0, 300, 12], [0.3, 1.0, 1e-3, 0.25]
    ok = _line("fading", what="w", n_taps=4, delays=",".join(map(str, delays)), powers=",".join(map(repr, powers)))
    many = lambda n: _line("fading", what="w", n_taps=n, delays=",".join(map(str, range(n))), powers=",".join(["1"] * n))   # noqa: E731
    bad = [("fade_twice", "3,9,3", "1,1,1", (3,)), ("fade_delay", "3,-1", "1,1", (-1, 4096)), ("fade_delay", "4097", "1", (4097, 4096)),
           ("fade_power", "0,4", "1,0", ()), ("fade_power", "0,4", "1,-2", ()), ("fade_power", "0,4", "inf,1", ()),
           ("fade_power", "0,4", "1,nan", ()), ("fade_power", "0,4", "1e308,1e308", ())]
    lines = [ok, many(64), many(65), many(0), _line("fading", what="w", n_taps=1, delays="null", powers="1"),
             _line("fading", what="w", n_taps=1, delays="4096", powers="2")]
    lines += [_line("fading", what="w", n_taps=len(d.split(",")), delays=d, powers=p) for _, d, p, _ in bad]
    got = _ask(host_program, lines)
    s = 0.0
    for p in powers:
        s += p                                                          # in index order
    want = " ".join(f"{d}:{_dbits(math.sqrt(p / s))}" for d, p in zip(delays, powers))
    assert got[0] == f"ok 300 4 {want}"
    assert got[1].startswith("ok 63 64 ")
    assert got[2] == got[3] == "refused fade_count " + tc.message("fade_count", "w", (64,))
    assert got[4] == "refused fade_missing " + tc.message("fade_missing", "w")
    assert got[5] == f"ok 4096 1 4096:{_dbits(1.0)}"
    for (rid, _, _, values), g in zip(bad, got[6:]):
        assert g == f"refused {rid} " + tc.message(rid, "w", values)


def test_channel_pass(host_program):
    """Kernel, dynamic LDS = cs * (TXF_SEG + halo + (fade ? n_taps : 0)) and grid = (ceil(len / TXF_SEG), nf)."""
    names = {(0, 0): "tx_channel_fused_kernel", (1, 0): "tx_channel_imp_kernel", (0, 1): "tx_channel_fade_kernel",
             (1, 1): "tx_channel_imp_fade_kernel"}
    two = dict(_geometries()[5], n_symb=5)                              # Nfft 1024 x 5 symbols: 5760 samples, two segments
    shapes = _shapes() + [dict(two, f64=0), dict(two, f64=1)]
    combos = [(s, imp, fade, halo, nt, nf) for s in shapes for imp in (0, 1) for fade in (0, 1)
              for halo, nt, nf in ((0, 1, 1), (10, 3, 5), (4096, 64, 65535))]
    got = _ask(host_program, [_line("pass", s, imp=i, fade=f, halo=h, n_taps=nt, nf=nf) for s, i, f, h, nt, nf in combos])
    segments = set()
    for (s, imp, fade, halo, nt, nf), g in zip(combos, got):
        ln = (s["nfft"] + s["t_guard"]) * s["n_symb"]
        w = g.split()
        assert w[1] == names[imp, fade] and w[0] == {(0, 0): "plain", (1, 0): "imp", (0, 1): "fade", (1, 1): "imp_fade"}[imp, fade]
        assert int(w[2]) == (16 if s["f64"] else 8) * (4096 + halo + (nt if fade else 0))
        assert (int(w[3]), int(w[4]), int(w[5])) == (-(-ln // 4096), nf, ln)
        segments.add(int(w[3]))
    assert {1, 2, 8} <= segments                                       # one segment, two (a frame of > 4096 samples), config M's
    src = open(os.path.join(CSRC, "ofdm_txfused.hip")).read()
    for n in names.values():
        assert f"void {n}(" in src


@pytest.mark.parametrize("family", sorted(tc.ORDER))
def test_first_refusal_wins_in_the_parents_order(host_program, family):
    """A call broken for every check from position i on is refused by check i, with the parent's message; broken for none, it
    is accepted.  Both precisions."""
    order = tc.ORDER[family]
    for f64 in (0, 1):
        shape = dict(_geometries()[4], f64=f64)
        lines = [_line("prelude", tc.broken_from(family, shape, i)) for i in range(len(order) + 1)]
        got = _ask(host_program, lines)
        for i, (rid, what) in enumerate(order):
            assert got[i] == f"refused {rid} " + tc.message(rid, what, tc.BREAK[rid][1]), (family, i, rid)
        assert got[-1].startswith("ok ")


def test_every_refusal_is_in_an_order_and_its_text_in_the_header():
    src = open(os.path.join(CSRC, "txf_plan.hpp")).read()
    for rid, text in tc.MSG.items():
        assert f'"{text}"' in src, rid
    assert {rid for o in tc.ORDER.values() for rid, _ in o} == set(tc.MSG) == set(tc.BREAK)
    ids = re.search(r"IDS\[TXF_REFUSALS\] = \{(.*?)\};", open(os.path.join(ROOT, "tests", "host", "txf_plan_main.cpp")).read(), re.S)
    assert set(re.findall(r'"(\w+)"', ids.group(1))) == set(tc.MSG) | {"ok"}
    for case in tc.API:
        assert case[4] in tc.MSG and case[1] in ("tx_frames_fused", "ber_sweep", "ber_sweep_task4")


def test_the_header_is_free_of_the_device_runtime():
    src = open(os.path.join(CSRC, "txf_plan.hpp")).read()
    assert "hip/" not in src and "__global__" not in src and "__device__" not in src
    assert set(re.findall(r'#include [<"]([^>"]+)[>"]', src)) <= {"algorithm", "cmath", "cstdarg", "cstddef", "cstdint", "cstdio",
                                                                 "vector", "t4_route.hpp"}
    # the .hip side keeps no second copy of a size or of the chunk rule
    for name in ("ofdm_txfused.hip", "ofdm_ber_sweep.hip"):
        hip = open(os.path.join(CSRC, name)).read()
        assert "a256" not in hip and "TXF_WS_BUDGET" not in hip
