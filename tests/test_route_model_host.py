"""The route decision of the Task-5 receiver (csrc/chain_route.hpp: chain_route_choose) against the hand-written model of
tests/routes.py, on the CPU: tests/host/chain_route_main.cpp is compiled with the host compiler and the address and
undefined-behaviour sanitizers into a stand-alone program, which answers every case of routes.CASES and routes.REFUSALS, every
case of omp_route_cases.CASES under each of the three OMP routes, and the five baseline configurations of frames.py (bench.py's
workload) in both precisions.  A disagreement between the model and the dispatcher fails here, without a GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import omp_route_cases as oc
import routes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OMP_ROUTE_IDS = {"auto": 0, "batch": 1, "wide": 2}


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no C++ compiler for the stand-alone program"
    exe = str(tmp_path_factory.mktemp("chain_route") / "chain_route_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "chain_route_main.cpp"), "-o", exe], check=True)
    return exe


def _shape_line(c, precision, mode, descr, mer, env, omp_route, ls=False):
    """The ChainShape ofdm_rx_plan_create / set_mmse / set_descrambler / set_omp_route leave for the case, as the program reads it."""
    f = routes._plan_fields(c)
    f64 = precision == "fp64"
    np_pad = (f["np"] + 15) & ~15
    # ofdm_rx_plan_set_mmse builds the factors of an fp32 plan when mmse_factored_usable says so (the switches as they are then)
    # (ls: ofdm_rx_plan_set_mmse_ls -- no operator and no factors, estimator EST_MMSE_LS)
    factors = mode == "mmse" and not ls and not f64 and f["np"] % 4 == 0 and "OFDM_MMSE_NO_MFMA" not in env and "OFDM_MMSE_DENSE" not in env
    kv = dict(nfft=c.nfft, n_symb=c.n_symb, n_carrier=c.nc, np=f["np"], nd=f["nd"], k_atoms=c.K, taps=len(c.delays),
              bps=routes.BPS[c.const], bits_per_axis=routes.BITS_PER_AXIS[c.const], f64=int(f64), pilots_in_band=int(f["in_band"]),
              comb_m=f["comb_m"], comb_lg_up=f["lg_up"], data_mod4=f["mod4"], estimator=(2 if ls else 1) if mode == "mmse" else 0,
              mmse_factors=int(factors), np_pad=np_pad if factors else 0, m_pad=(c.nc + 15) & ~15 if mode == "mmse" and not ls else 0,
              descr_on=int(descr), omp_route=OMP_ROUTE_IDS[omp_route], want_mer=int(mer))
    return " ".join([f"{k}={v}" for k, v in kv.items()] + [f"{k}={v}" for k, v in env.items()])


def _want(c, precision, mode, descr, mer, env, omp_route):
    try:
        r = routes.expected_route(c, precision, mode, descr, mer, env, omp_route)
    except routes.Refused as e:
        return f"refused {e.where}"
    return " ".join([r.entry, r.front, r.estimator, r.omp_state, r.c0, r.symbols, str(r.ba), r.descr, str(int(r.mer))])


def _baseline_cases():
    """The five baseline configurations as routes.Case geometry (name, Case)."""
    from ofdm_course_amd import frames as fr
    out = []
    for cfg in (fr.config_M(), fr.config_C5(), fr.config_C3(), fr.config_small(), fr.config_small(nfft=512, n_carrier=128)):
        pc = np.asarray(cfg.pilotCarriers, dtype=np.int64)
        c = routes.Case(f"baseline-{cfg.name}-{cfg.Nfft}", cfg.Nfft, cfg.N_carrier, 1, cfg.Constellation, cfg.N_symb,
                        tuple(range(cfg.dominant_taps)), k_atoms=cfg.K)
        c.pilot_carriers = lambda pc=pc: pc
        assert np.array_equal(c.data_carriers(), np.asarray(cfg.dataCarriers, dtype=np.int64))
        out.append(c)
    return out


def _all_calls():
    calls = []
    for c in routes.CASES + routes.REFUSALS:
        calls.append((c.name, (c, c.precision, c.mode, c.descr, c.mer, c.env, "batch")))
    for c in oc.CASES:
        for r in routes.OMP_ROUTES:
            calls.append((f"{c.name}/{r}", (c, c.precision, c.mode, c.descr, c.mer, c.env, r)))
    for c in _baseline_cases():
        for p in ("fp32", "fp64"):
            calls.append((f"{c.name}/{p}", (c, p, "omp", False, False, {}, "batch")))
    return calls


def test_chooser_answers_what_the_model_expects(host_program, monkeypatch):
    for v in sorted(routes.dispatch_switches(excluded=True) | set(routes.EXTRA_SWITCHES)):
        monkeypatch.delenv(v, raising=False)
    calls = _all_calls()
    assert len(calls) == len(routes.CASES) + len(routes.REFUSALS) + 3 * len(oc.CASES) + 10
    text = "\n".join(_shape_line(*a) for _, a in calls) + "\n"
    r = subprocess.run([host_program], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr              # a sanitizer report is a failure
    got = r.stdout.splitlines()
    assert len(got) == len(calls)
    bad = [(name, g, _want(*a)) for (name, a), g in zip(calls, got) if g != _want(*a)]
    for b in bad:
        print(*b, sep="\n    ")
    assert not bad
    # the refusals of the table are refused by the chooser with the id the table records
    for c in routes.REFUSALS:
        assert got[[n for n, _ in calls].index(c.name)] == f"refused {routes.REFUSAL_IDS[c.name]}"


def test_mmse_ls_plans_take_the_mmse_route_with_their_own_stage(host_program, monkeypatch):
    """A plan in the h = ifft(H_LS) mode: every MMSE case of the table again with estimator EST_MMSE_LS.  The route is the MMSE
    route of the case (entry, front end, symbol stage with its HEXT build, DeScrambler pass) with mmse_ls_stage_run as the
    estimator, whatever the MMSE switches say."""
    for v in sorted(routes.dispatch_switches(excluded=True) | set(routes.EXTRA_SWITCHES)):
        monkeypatch.delenv(v, raising=False)
    cases = [c for c in routes.CASES + routes.REFUSALS if c.mode == "mmse"]
    assert len(cases) >= 20
    text = "\n".join(_shape_line(c, c.precision, c.mode, c.descr, c.mer, c.env, "batch", ls=True) for c in cases) + "\n"
    r = subprocess.run([host_program], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    got = r.stdout.splitlines()
    assert len(got) == len(cases)
    for c, g in zip(cases, got):
        want = _want(c, c.precision, c.mode, c.descr, c.mer, c.env, "batch").split(" ")
        if want[0] != "refused":
            want[2] = "mmse_ls"
        assert g == " ".join(want), (c.name, g, want)


def test_the_header_is_free_of_the_device_runtime():
    src = open(os.path.join(ROOT, "ofdm-course_amd", "csrc", "chain_route.hpp")).read()
    assert "hip/" not in src and "__global__" not in src and "__device__" not in src
    assert set(__import__("re").findall(r'#include [<"]([^>"]+)[>"]', src)) <= {"cstddef", "cstdint", "cstdlib", "omp_wide_host.hpp"}
