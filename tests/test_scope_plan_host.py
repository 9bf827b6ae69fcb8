"""The constellation-capture plan (csrc/scope_plan.hpp: scope_iq_check, scope_density_check, the grid's place in the equalise /
demap stage's LDS, scope_bin) against the hand-written model of tests/scope_cases.py, on the CPU: tests/host/scope_plan_main.cpp
is compiled with the host compiler and the address and undefined-behaviour sanitizers into a stand-alone program, which answers
every refusal in order, the LDS bytes of the accepted calls and the bin of every edge value.  A disagreement between the model
and the header fails here, without a GPU."""
import os
import re
import shutil
import subprocess

import pytest

import scope_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ofdm-course_amd", "csrc")
HEADER = os.path.join(CSRC, "scope_plan.hpp")


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no C++ compiler for the stand-alone program"
    exe = str(tmp_path_factory.mktemp("scope_plan") / "scope_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "scope_plan_main.cpp"), "-o", exe], check=True)
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
    lines = [f"iq first={f} count={c} decisions={d}" for f, c, d in sc.IQ_CASES]
    got = _ask(host_program, lines)
    seen = set()
    for case, g in zip(sc.IQ_CASES, got):
        want = sc.iq_refusal(*case)
        assert g == ("ok" if want is None else f"refused {want[0]} {want[1]}"), (case, g)
        seen.add(None if want is None else want[0])
    assert seen == {None, *sc.IQ_ORDER}
    # the order itself, written down: a window wrong in every way is refused for its start, then its count, then its end
    assert sc.iq_refusal(-1, 0, 10)[0] == "iq_first" and sc.iq_refusal(11, 0, 10)[0] == "iq_count"
    assert sc.iq_refusal(11, 1, 10)[0] == "iq_end"


def test_density_refusals_in_order_and_lds_bytes(host_program):
    lines = [f"density out={o} bins={b} half_width={_num(hw)} skip={s} f64={f} n_carrier={nc} decisions={d}"
             for o, b, hw, s, f, nc, d in sc.DENSITY_CASES]
    got = _ask(host_program, lines)
    seen = set()
    for case, g in zip(sc.DENSITY_CASES, got):
        want = sc.density_refusal(*case)
        if want is None:
            _, bins, _, _, f64, nc, d = case
            off, extra, total = sc.grid_layout(f64, nc, d, bins)
            assert g == f"ok {off} {extra} {total}", (case, g)
            assert off % 16 == 0 and 4 * bins * bins <= extra < 4 * bins * bins + 16 and total <= sc.STAGE_LDS_LIMIT
        else:
            assert g == f"refused {want[0]} {want[1]}", (case, g)
        seen.add(None if want is None else want[0])
    assert seen == {None, *sc.DENSITY_ORDER}
    # the order itself, written down
    bad = dict(out=0, bins=9, half_width=0.0, skip=-1, f64=1, n_carrier=4096, decisions=27000)
    for fix, name in (({}, "density_out"), (dict(out=1), "bins"), (dict(bins=128), "half_width"), (dict(half_width=2.0), "skip"),
                      (dict(skip=0), "lds")):
        bad.update(fix)
        assert sc.density_refusal(**bad)[0] == name
    bad.update(bins=64)
    assert sc.density_refusal(**bad) is None
    # the two figures quoted in scope_cases.DENSITY_CASES
    assert sc.stage_lds(1, 4096, 27000) == 92560 and sc.grid_layout(1, 4096, 27000, 64)[2] == 108944
    assert sc.grid_layout(1, 4096, 27000, 128)[2] == 158096 > sc.STAGE_LDS_LIMIT


def test_bin_of_every_edge_value(host_program):
    got = _ask(host_program, [f"bin v={v} half_width={_num(hw)} bins={b}" for v, hw, b, _ in sc.BIN_CASES])
    for (v, hw, b, want), g in zip(sc.BIN_CASES, got):
        assert int(g) == want, (v, hw, b, g, want)
        assert sc.bin_of(float(v), hw, b) == want, (v, hw, b)                # the model used for the GPU histograms agrees
    vals = {v for v, hw, b, _ in sc.BIN_CASES if (hw, b) == (1.0, 8)}
    assert {"-0.0", "-1", "1", "inf", "-inf", "nan", "-0.75", "-7", "7"} <= vals


def test_the_limit_and_the_stage_bytes_are_the_receivers():
    """The model's constants are the ones the receiver uses (chain_route.hpp), and the header takes them from there."""
    route = open(os.path.join(CSRC, "chain_route.hpp")).read()
    wide = open(os.path.join(CSRC, "omp_wide_host.hpp")).read()
    assert "STAGE_LDS_LIMIT = OMP_STAGE_LDS_LIMIT" in route and "OMP_STAGE_LDS_LIMIT = 150 * 1024" in wide
    assert "(size_t)(f64 ? 16 : 8) * n_carrier + (((size_t)decisions + 31) & ~size_t(31)) + 16" in route
    src = open(HEADER).read()
    assert "STAGE_LDS_LIMIT" in src and "eq_demap_lds_bytes" in src and "150" not in src


def test_the_header_holds_the_messages_and_is_free_of_the_device_runtime():
    src = open(HEADER).read()
    for msg in sc.MESSAGES.values():
        assert f'"{msg}"' in src, msg
    assert "hip/" not in src and "__global__" not in src and "hipLaunch" not in src
    # the device qualifier comes through a macro that is empty for a host compiler
    assert re.search(r"#if defined\(__HIPCC__\)\s*\n#define OFDM_SCOPE_HD __host__ __device__\s*\n#else\s*\n#define OFDM_SCOPE_HD\s*\n#endif", src)
    assert src.count("__device__") == 1
    assert set(re.findall(r'#include [<"]([^>"]+)[>"]', src)) <= {"cmath", "cstdarg", "cstddef", "cstdint", "cstdio",
                                                                  "chain_route.hpp"}


def test_the_kernel_and_the_host_bin_through_the_one_function():
    """scope_bin is defined once, in the header, and eq_demap_kernel's capture calls it for both coordinates."""
    defs = 0
    for name in os.listdir(CSRC):
        if name.endswith((".hip", ".hpp")):
            defs += len(re.findall(r"inline int scope_bin\(", open(os.path.join(CSRC, name)).read()))
    assert defs == 1
    split = open(os.path.join(CSRC, "ofdm_chain_split.hip")).read()
    assert '#include "scope_plan.hpp"' in split and split.count("scope_bin((double)ye.") == 2
