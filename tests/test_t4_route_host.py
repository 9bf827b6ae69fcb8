"""The route decision of the Task-4 receiver (csrc/t4_route.hpp: t4_route_choose, t4_arena_layout, t4_frame_bytes) against the
hand-written table of tests/t4_routes.py, on the CPU: tests/host/t4_route_main.cpp is compiled with the host compiler and the
address and undefined-behaviour sanitizers into a stand-alone program, which answers every case of t4_cases.CASES with each of
its flag sets in both precisions, the seven switch runs, frames.config_C3() (the benchmark's Task-4 workload) and the refusals.
A disagreement between the table and the dispatcher fails here, without a GPU."""
import glob
import os
import re
import shutil
import subprocess

import pytest

import t4_cases as tc
import t4_routes as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ofdm-course_amd", "csrc")
BPS = {"QPSK": 2, "16QAM": 4, "64QAM": 6}
ARENA_REGIONS = 12                  # the reserve(...) list of t4_arena_layout, each region padded to 256 bytes


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no C++ compiler for the stand-alone program"
    exe = str(tmp_path_factory.mktemp("t4_route") / "t4_route_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "t4_route_main.cpp"), "-o", exe], check=True)
    return exe


def _geometries():
    """name -> dict(nfft, t_guard, n_symb, n_carrier, np, frames, frame_words) of the table's cases and of config C3."""
    from oracle import ofdm_oracle as oracle
    from ofdm_course_amd import frames as fr
    out = {}
    for c in tc.CASES:
        pc, dc = oracle.pilot_layout_percent(c.Nfft, c.N_carrier, c.pct, 2)
        out[c.name] = dict(nfft=c.Nfft, t_guard=c.T_guard, n_symb=c.N_symb, n_carrier=c.N_carrier, np=len(pc),
                           frames=tc.total_frames(c), frame_words=(len(dc) * c.N_symb * BPS[c.const] + 31) // 32)
    cfg = fr.config_C3()
    assert (cfg.Nfft, cfg.T_guard, cfg.N_carrier, cfg.N_symb) == (2048, 256, 800, 50)
    out["C3"] = dict(nfft=cfg.Nfft, t_guard=cfg.T_guard, n_symb=cfg.N_symb, n_carrier=cfg.N_carrier, np=len(cfg.pilotCarriers),
                     frames=4096, frame_words=(len(cfg.dataCarriers) * cfg.N_symb * BPS[cfg.Constellation] + 31) // 32)
    return out


def _rows():
    """(id, geometry name, precision, flags, env, expected words) of every accepted row of the table."""
    rows = []
    for name, precision in tr.STATIC:
        for flags in tr.flag_sets(name):
            rows.append((f"{name}-{precision}-{''.join(map(str, flags))}", name, precision, flags, (), tr.expected_words(name, precision, flags)))
    for switch, name in tr.SWITCH_ROWS:
        for precision in ("fp64", "fp32"):
            rows.append((f"{name}-{precision}-111-{switch}", name, precision, (1, 1, 1), (switch,), tr.SWITCH_WORDS[switch, name, precision]))
    return rows


def _line(geo, precision, flags, env, **changed):
    kv = dict(geo, f64=int(precision == "fp64"), time_desync=flags[0], freq_desync=flags[1], mp_desync=flags[2],
              band_tables=int(precision == "fp32"))           # t4_plan_tables builds the band on every fp32 plan
    kv.update(changed)
    return " ".join([f"{k}={v}" for k, v in kv.items()] + [f"{k}=1" for k in env])


def _ask(host_program, lines):
    r = subprocess.run([host_program], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr              # a sanitizer report is a failure
    got = r.stdout.splitlines()
    assert len(got) == len(lines)
    return got


def _header_switches():
    return set(re.findall(r'getenv\("(OFDM_T4_\w+)"\)', open(os.path.join(CSRC, "t4_route.hpp")).read()))


@pytest.fixture(scope="module")
def answers(host_program):
    for v in _header_switches() | {"OFDM_EQD_SCALAR"}:
        os.environ.pop(v, None)
    geo = _geometries()
    rows = _rows()
    got = _ask(host_program, [_line(geo[name], precision, flags, env) for _, name, precision, flags, env, _ in rows])
    return geo, rows, [g.split(" ") for g in got]


def test_table_covers_what_it_should():
    assert {n for n, _ in tr.STATIC} == {c.name for c in tc.CASES} | {"C3"}
    assert len(_rows()) == 2 * sum(len(tc.flag_sets(c)) for c in tc.CASES) + 2 * 5 + 2 * 7
    from test_gpu_task4_sizes import SWITCH_RUNS
    assert tr.SWITCH_ROWS[:6] == [(s, n) for s, n, _ in SWITCH_RUNS] and tr.SWITCH_ROWS[6][0] == "OFDM_T4_DENSE_SPLINE"


def test_chooser_answers_what_the_table_expects(answers):
    geo, rows, got = answers
    bad = []
    for (rid, name, _, _, _, want), g in zip(rows, got):
        words, fstride = " ".join(g[:11]), int(g[11])
        g_ = geo[name]
        want_stride = g_["np"] * g_["n_symb"] if g[7] == "compact" else g_["nfft"] * g_["n_symb"]
        if words != want or fstride != want_stride:
            bad.append((rid, words, want, fstride, want_stride))
    for b in bad:
        print(*b, sep="\n    ")
    assert not bad


def test_refusals_come_before_anything_else_with_the_parent_messages(host_program):
    geo = _geometries()["n64"]
    names = sorted(tr.REFUSALS)
    lines = [_line(geo, p, tr.REFUSALS[n][1], (), **tr.REFUSALS[n][0]) for n in names for p in ("fp64", "fp32")]
    got = _ask(host_program, lines)
    for i, n in enumerate(names):
        _, _, rid, msg = tr.REFUSALS[n]
        assert got[2 * i] == got[2 * i + 1] == f"refused {rid} {msg}", (n, got[2 * i])
    assert {r[2] for r in tr.REFUSALS.values()} == {"guard", "pilots"}
    # the three message texts of the parent, verbatim (the second is unreachable behind the first: t4_routes.REFUSALS)
    src = open(os.path.join(CSRC, "t4_route.hpp")).read()
    for msg in (tr.MSG_GUARD, tr.MSG_IFO_SEGMENT, tr.MSG_PILOTS):
        assert f'"{msg}"' in src, msg


def test_the_header_is_free_of_the_device_runtime():
    src = open(os.path.join(CSRC, "t4_route.hpp")).read()
    assert "hip/" not in src and "__global__" not in src and "__device__" not in src
    assert set(re.findall(r'#include [<"]([^>"]+)[>"]', src)) <= {"cstddef", "cstdint", "cstdlib", "chain_route.hpp"}


def test_every_route_switch_is_read_in_the_header_and_covered_by_a_row():
    elsewhere = {}
    for path in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")):
        if os.path.basename(path) != "t4_route.hpp":
            for v in re.findall(r'getenv\("(OFDM_T4_\w+)"\)', open(path).read()):
                elsewhere.setdefault(v, []).append(os.path.basename(path))
    assert elsewhere == {"OFDM_T4_WAVE_SPC": ["ofdm_t4_wave.hip"]}            # a grid-shape tuning value, not a route switch
    switches = _header_switches()
    assert switches == {"OFDM_T4_FULL_ACF", "OFDM_T4_STAGED", "OFDM_T4_UNFUSED_SYNC", "OFDM_T4_DENSE_SPLINE", "OFDM_T4_NO_WAVE"}
    assert switches == {s for s, _ in tr.SWITCH_ROWS}


def test_frame_bytes_is_the_parents_formula_and_bounds_the_arena(answers):
    """t4_frame_bytes sizes the chunks of the BER sweep: its value must stay what it was,
        cs * (len + Nfft * S + np * S + 2 * Nfft + np + N_carrier) + 128 + 4 * frame_words,   len = (Nfft + T_guard) * S,
    and F of it (+ the alignment padding of the arena's regions) must hold the arena of a call over F frames, at 1 frame, at the
    case's count and at the 65535 of the entry's limit.  OFDM_T4_FULL_ACF adds the curve, which the sweep does not budget."""
    geo, rows, got = answers
    checked = 0
    for (rid, name, precision, _, env, _), g in zip(rows, got):
        q = geo[name]
        cs = 16 if precision == "fp64" else 8
        ln = (q["nfft"] + q["t_guard"]) * q["n_symb"]
        want = cs * (ln + q["nfft"] * q["n_symb"] + q["np"] * q["n_symb"] + 2 * q["nfft"] + q["np"] + q["n_carrier"]) + 128 + 4 * q["frame_words"]
        assert int(g[15]) == want, rid
        if "OFDM_T4_FULL_ACF" in env:
            continue
        for total, F in zip(map(int, g[12:15]), (1, q["frames"], 65535)):
            assert total <= F * want + ARENA_REGIONS * 256, (rid, F, total)
        checked += 1
    assert checked == len(rows) - 4
