"""The Task-5 part of the constellation-capture plan (csrc/scope_plan.hpp: scope5_iq_check, scope5_density_check, the grid's
place behind a symbol stage's LDS) against the hand-written model of tests/scope5_cases.py, on the CPU:
tests/host/scope5_plan_main.cpp is compiled with the host compiler and the address and undefined-behaviour sanitizers into a
stand-alone program, which answers every refusal in order and the LDS bytes of the accepted calls.  A disagreement between the
model and the header fails here, without a GPU."""
import dataclasses
import os
import re
import shutil
import subprocess

import pytest

import routes
import scope5_cases as s5
import scope_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ofdm-course_amd", "csrc")
HEADER = os.path.join(CSRC, "scope_plan.hpp")


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no C++ compiler for the stand-alone program"
    exe = str(tmp_path_factory.mktemp("scope5_plan") / "scope5_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "scope5_plan_main.cpp"), "-o", exe], check=True)
    return exe


def _ask(host_program, lines):
    r = subprocess.run([host_program], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr              # a sanitizer report is a failure
    got = r.stdout.splitlines()
    assert len(got) == len(lines)
    return got


def _num(v):
    return repr(float(v)) if isinstance(v, float) else str(v)


def test_window_refusals_in_order(host_program):
    got = _ask(host_program, [f"iq first={f} count={c} decisions={d}" for f, c, d in s5.IQ_CASES])
    seen = set()
    for case, g in zip(s5.IQ_CASES, got):
        want = s5.iq_refusal(*case)
        assert g == ("ok" if want is None else f"refused {want[0]} {want[1]}"), (case, g)
        seen.add(None if want is None else want[0])
    assert seen == {None, *s5.IQ_ORDER}
    # the order itself, written down: a window wrong in every way is refused for its start, then its count, then its end
    assert s5.iq_refusal(-1, 0, 10)[0] == "iq_first" and s5.iq_refusal(11, 0, 10)[0] == "iq_count"
    assert s5.iq_refusal(11, 1, 10)[0] == "iq_end"
    # the three refusals are the Task-4 entry's, under the Task-5 entry's name
    for case in s5.IQ_CASES:
        a, b = s5.iq_refusal(*case), sc.iq_refusal(*case)
        assert (a is None) == (b is None) and (a is None or (a[0] == b[0] and a[1] == b[1].replace("task4", "task5")))


def test_density_refusals_in_order_and_lds_bytes(host_program):
    lines = [f"density stage={st} lds={lds} out={o} bins={b} half_width={_num(hw)} skip={s} decisions={d}"
             for st, lds, o, b, hw, s, d in s5.DENSITY_CASES]
    got = _ask(host_program, lines)
    seen, fits = set(), set()
    for case, g in zip(s5.DENSITY_CASES, got):
        want = s5.density_refusal(*case)
        if want is None:
            st, lds, _, bins = case[:4]
            off, total = s5.grid_layout(lds, bins)
            assert g == f"ok {off} {total}", (case, g)
            assert off % 16 == 0 and 0 <= off - lds < 16 and total == off + 4 * bins * bins and total <= s5.lds_limit(st)
            fits.add(st)
        else:
            assert g == f"refused {want[0]} {want[1]}", (case, g)
        seen.add(None if want is None else want[0])
    assert seen == {None, *s5.DENSITY_ORDER} and fits == set(range(6))
    # the order itself, written down
    bad = dict(stage=1, lds=100000, out=0, bins=9, half_width=0.0, skip=-1, decisions=144)
    for fix, name in (({}, "density_out"), (dict(out=1), "bins"), (dict(bins=128), "half_width"), (dict(half_width=2.0), "skip"),
                      (dict(skip=0), "lds")):
        bad.update(fix)
        assert s5.density_refusal(**bad)[0] == name
    bad.update(bins=64)
    assert s5.density_refusal(**bad) is None
    # the limits, written down: the generic kernel's 158 KiB, 150 KiB for every other stage
    assert s5.density_refusal(4, 88064, 1, 128, 1.0, 0, 144) is None and s5.density_refusal(4, 88065, 1, 128, 1.0, 0, 144)[0] == "lds"
    assert s5.density_refusal(0, 96256, 1, 128, 1.0, 0, 144) is None and s5.density_refusal(0, 96257, 1, 128, 1.0, 0, 144)[0] == "lds"
    assert s5.density_refusal(0, 90000, 1, 128, 1.0, 0, 144) is None and "eq_demap" in s5.density_refusal(5, 90000, 1, 128, 1.0, 0, 144)[1]


def test_the_wave_stage_bytes_are_its_layouts(host_program):
    """The wave stage's LDS is not in the route: scope5_stage_lds takes it from wave_layout at four wavefronts per workgroup."""
    shapes = [(384, 3), (100, 3), (336, 2), (384, 1), (96, 40), (77, 5)]
    got = _ask(host_program, [f"wave nd={nd} n_symb={ns}" for nd, ns in shapes])
    for (nd, ns), g in zip(shapes, got):
        assert routes.wave_layout_ok(nd, ns, 4)
        assert int(g) == s5.wave_lds(nd, ns) <= 52 * 1024, (nd, ns, g)


def test_the_limits_and_the_stage_bytes_are_the_receivers():
    route = open(os.path.join(CSRC, "chain_route.hpp")).read()
    assert "GENERIC_LDS_LIMIT = 158 * 1024" in route and "STAGE_LDS_LIMIT = OMP_STAGE_LDS_LIMIT" in route
    assert re.search(r"enum \{ SYM_GENERIC, SYM_RX_SYMBOLS, SYM_WAVE, SYM_COOP4, SYM_R2, SYM_EQ_DEMAP \}", route)
    src = open(HEADER).read()
    assert "GENERIC_LDS_LIMIT" in src and "158" not in src and "150" not in src
    for msg in s5.MESSAGES.values():
        assert f'"{msg}"' in src, msg
    # every stage of the table of the issue has a natural case whose stage the model names
    want = {"generic-128-16qam-mer-fp32": 0, "fast-512-pruned-fp64": 1, "wave-skip0-64qam": 2, "coop4-64qam-mer": 3,
            "r2-comb8-16qam": 4, "split-8192-vec-8psk-mer": 5}
    by_name = {c.name: c for c in routes.CASES}
    for name, st in want.items():
        got, lds = s5.stage_of_case(dataclasses.replace(by_name[name], mer=True))
        assert got == st and 0 < lds <= s5.lds_limit(st), (name, got, lds)


def test_the_task5_stages_bin_through_the_one_function():
    """The Scope variants of the Task-5 symbol stages call scope_bin, through the one per-point function of chain_fast_core.hpp;
    each symbol-stage source calls that function at its MER sites and adds no environment switch."""
    core = open(os.path.join(CSRC, "chain_fast_core.hpp")).read()
    assert core.count("scope_bin((double)ye.") == 2 and "inline int scope_bin(" not in core
    sites = {"ofdm_chain.hip": 1, "ofdm_chain_fast.hip": 2, "ofdm_chain_wave.hip": 1, "ofdm_chain_coop.hip": 2}
    for name, n in sites.items():
        src = open(os.path.join(CSRC, name)).read()
        assert src.count("scope5_point<T>(") == n, name
    split = open(os.path.join(CSRC, "ofdm_chain_split.hip")).read()
    assert split.count("scope5_point<T>(") == 3
