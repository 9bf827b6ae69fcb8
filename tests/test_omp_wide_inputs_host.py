"""CPU checks of the wide OMP route (csrc/ofdm_omp_wide.hip, ofdm_OMP_estimate_batch):

* the inputs of tests/test_gpu_omp_wide.py are tie-free by construction: the recorded top-two gaps of the oracle's own pursuit
  (tests/omp_wide_cases.py) are recomputed here and may not drift by more than 1 %;
* the host code of the route (LDS layout, supported shapes, route choice: csrc/omp_wide_host.hpp) is compiled into a stand-alone
  program with the address and undefined-behaviour sanitizers and run over every required (Nfft, K, taps, precision);
* the LDS bounds of omp_batch_kernel that send a shape to the wide route, from the model of its layout (routes.omp_layout);
* the kernel compiles for gfx950 without scratch in both precisions; the entry is declared, exported and bound."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import omp_wide_cases as wc
import routes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ofdm-course_amd", "csrc")
LIMIT = 150 * 1024


@pytest.mark.parametrize("case", wc.Y_CASES + wc.REFUSAL_CASES, ids=[c.name for c in wc.Y_CASES + wc.REFUSAL_CASES])
def test_recorded_gaps_of_the_pilot_vectors(oracle, case):
    assert len(case.pilot_carriers()) >= case.taps and case.n == (5 if case in wc.Y_CASES else 2)
    g = case.min_gap(oracle)
    print(case.name, "seed", case.seed, "smallest top-two gap", g)
    assert g > 1e-6
    assert abs(g - case.gap) <= 0.01 * g, (g, case.gap)


def test_recorded_gap_of_the_part2_replay(oracle):
    g = wc.part2_gap(oracle)
    print("part2 replay, seed", wc.PART2_KW["seed"], "smallest top-two gap", g)
    assert g > 1e-3                                            # the replay also runs in fp32
    assert abs(g - wc.PART2_GAP) <= 0.01 * g, (g, wc.PART2_GAP)


@pytest.mark.parametrize("nine", [False, True], ids=["committed-6-taps", "9-taps"])
def test_recorded_gap_of_the_mse_replay(oracle, nine):
    g = wc.mse_gap(oracle, nine)
    want = wc.MSE9_GAP if nine else wc.MSE_GAP
    print("MSE replay, nine paths" if nine else "MSE replay", "smallest top-two gap", g)
    assert g > 1e-6
    assert abs(g - want) <= 0.01 * g, (g, want)


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no C++ compiler for the stand-alone program"
    exe = str(tmp_path_factory.mktemp("omp_wide") / "omp_wide_host_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "omp_wide_host_main.cpp"), "-o", exe], check=True)
    return exe


def _wide_total(taps, f64):
    cs = 16 if f64 else 8
    state = (cs * taps * (taps | 1) + 15) & ~15                # omp_wave_rs: omp_wave_core.hpp
    fft = (cs * routes.fft_lds_elems(2048) + 15) & ~15
    return state, max(4 * state, fft)


def test_host_code_under_the_sanitizers(host_program):
    r = subprocess.run([host_program, "sweep"], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr          # a sanitizer report is a failure
    lines = r.stdout.strip().splitlines()
    lay = [tuple(int(v) for v in re.findall(r"\d+", ln)) for ln in lines if ln.startswith("layout")]
    assert len(lay) == 64
    for _, f64, taps, state, total in lay:                       # (the first number is the "64" of the label)
        assert (state, total) == _wide_total(taps, bool(f64)), (f64, taps)
        assert total <= LIMIT
    # every K from taps to Nfft at the four sizes, 32 tap counts, two precisions
    want = 2 * sum(nfft - taps + 1 for taps in range(1, 33) for nfft in (512, 1024, 2048, 4096))
    assert lines[-1] == f"visited {want}"


# (shape, batch layout refused?) -- the bounds of omp_batch_kernel from its own layout (omp_layout, chain_route.hpp)
def _batch_total(np_, k, taps, f64, comb_m=0):
    by_fft = comb_m == 2048 and np_ <= 2048 and k <= 2048
    return routes.omp_layout(np_, k, taps, f64, routes.fft_lds_elems(2048) if by_fft else 0, {})[2]


def test_batch_bounds_and_route_choice(host_program):
    """Where omp_layout(...).total crosses 150 KB, i.e. where the tiles change kernel.  K = 4096 is refused in both precisions
    whatever Np; the driver's fp64 default at K = 2048 with 64 pilots is refused too; Main_model_Task_5.m as committed
    (Np = K = 1024, six paths, fp64) still fits by 6 016 bytes, and stops fitting with more than OMP_RT = 8 paths."""
    figures = {
        "K 4096, Np 64, 7 taps, fp32": _batch_total(64, 4096, 7, False),
        "K 4096, Np 64, 7 taps, fp64": _batch_total(64, 4096, 7, True),
        "K 2048, Np 64, 7 taps, fp64": _batch_total(64, 2048, 7, True),
        "K 2048, Np 64, 7 taps, fp32": _batch_total(64, 2048, 7, False),
        "K 1024, Np 1024, 6 taps, fp64": _batch_total(1024, 1024, 6, True),
        "K 1024, Np 1024, 9 taps, fp64": _batch_total(1024, 1024, 9, True),
    }
    print(figures)
    assert figures["K 4096, Np 64, 7 taps, fp32"] > LIMIT and figures["K 4096, Np 64, 7 taps, fp64"] > LIMIT
    assert figures["K 2048, Np 64, 7 taps, fp64"] > LIMIT >= figures["K 2048, Np 64, 7 taps, fp32"]
    assert figures["K 1024, Np 1024, 6 taps, fp64"] == 147584 <= LIMIT < figures["K 1024, Np 1024, 9 taps, fp64"]
    # smallest K the fp64 batch kernel refuses with 64 pilots and 7 taps, from the same formula
    k_first = next(k for k in range(7, 4097) if _batch_total(64, k, 7, True) > LIMIT)
    print("fp64, Np 64, 7 taps: omp_batch_kernel refuses from K =", k_first)
    assert k_first == 1868 and _batch_total(64, k_first - 1, 7, True) <= LIMIT        # DESIGN.md section 3 quotes the figure

    def choose(route, lds, nfft, k, taps):
        r = subprocess.run([host_program, "choose", str(route), str(lds), str(nfft), str(k), str(taps)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr
        code, why = r.stdout.strip().split(" ", 1)
        return int(code), why

    assert choose(0, figures["K 4096, Np 64, 7 taps, fp64"], 4096, 4096, 7) == (2, "-")
    assert choose(0, figures["K 1024, Np 1024, 6 taps, fp64"], 4096, 1024, 6) == (1, "-")
    assert choose(0, figures["K 1024, Np 1024, 9 taps, fp64"], 4096, 1024, 9) == (2, "-")
    assert choose(1, figures["K 4096, Np 64, 7 taps, fp32"], 4096, 4096, 7)[0] == 0
    code, why = choose(2, 1024, 8192, 4096, 7)
    assert code == 0 and "8192" in why
    code, why = choose(0, LIMIT + 1, 8192, 8192, 7)
    assert code == 0 and "8192" in why


def test_kernel_compiles_without_scratch():
    """hipcc --offload-arch=gfx950 on the new file, device side only: four instantiations (float / double, 8 / 16 atoms per
    thread), none with scratch or spilled registers."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.path.exists(hipcc), "hipcc is what builds the library"
    from ofdm_course_amd import build
    r = subprocess.run([hipcc, *build.CFLAGS, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(CSRC, "ofdm_omp_wide.hip"), "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S*omp_wide_kernel\S*)", r.stderr)
    assert len(names) == 4, names
    for key in ("ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill"):
        vals = [int(v) for v in re.findall(re.escape(key) + r": (\d+)", r.stderr)]
        assert len(vals) == 4 and not any(vals), (key, vals)
    print([(n[:40], v) for n, v in zip(names, re.findall(r" VGPRs: (\d+)", r.stderr))], re.findall(r"AGPRs: (\d+)", r.stderr))


def test_binding_and_python_surface():
    import ctypes as C
    from ofdm_course_amd import _lib as L
    from ofdm_course_amd import api
    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "ofdm_mi355x.h")).read()
    assert "int ofdm_OMP_estimate_batch(ofdm_rx_plan* plan, const void* y, int64_t n, int route, int32_t* index_out, void* x_out," in hdr
    assert list(lib.ofdm_OMP_estimate_batch.argtypes) == [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                                                          C.c_void_p, C.c_int]
    assert callable(api.OMP_estimate_batch) and "OMP_estimate_batch" in api.__all__


def test_the_wide_route_never_reads_the_dictionary():
    src = open(os.path.join(CSRC, "ofdm_omp_wide.hip")).read()
    code = "\n".join(ln.split("//")[0] for ln in src.splitlines())
    assert "sct" not in code


class _TileSpy(wc.OracleLib):
    """The oracle adapter plus a tile entry that only records the plans it is given."""

    def __init__(self, oracle):
        super().__init__(oracle)
        self.tiles = []

    def RxPlan(self, Nfft, T_guard, N_symb, N_carrier, pilotCarriers, dataCarriers, pv, K, taps, Constellation, precision="fp32"):

        class Plan:
            shape = (Nfft, K, len(pilotCarriers), precision)

            def close(self):
                pass
        return Plan()

    def task5_part2_tile(self, plan, tx, taps_list, snr, ref):
        self.tiles.append(plan.shape + (len(taps_list),))
        return dict(nmse=np.zeros((4, len(taps_list))), errors=np.zeros((4, len(taps_list)), dtype=np.uint32))


def test_driver_tiles_what_the_library_serves(oracle):
    """drivers/task5_part2.py with batched=True: the random-mask study at the driver's default sizes (K = Nfft = 4096) runs as
    tiles; at Nfft 8192 the comb scenarios with K <= 2048 are tiled as they always were, and only a dictionary the wide kernel
    would be needed for (K = 8192) runs call by call."""
    from ofdm_course_amd.drivers import task5_part2
    lib = _TileSpy(oracle)
    task5_part2.run(lib, reg_pilot=0, Nps=[64, 128], monteCarloRuns=2, batched=True)
    assert lib.tiles == [(4096, 4096, 64, "fp64", 2), (4096, 4096, 128, "fp64", 2)]
    lib = _TileSpy(oracle)
    r = task5_part2.run(lib, Nfft=8192, N_carrier=256, combs=[4, 8], monteCarloRuns=1, batched=True, precision="fp32")
    assert lib.tiles == [(8192, 2048, 64, "fp32", 1), (8192, 1024, 32, "fp32", 1)] and np.all(r["_sums"]["runs"] == 1)
    lib = _TileSpy(oracle)
    r = task5_part2.run(lib, Nfft=8192, N_carrier=256, reg_pilot=0, Nps=[16], monteCarloRuns=1, batched=True)
    assert lib.tiles == [] and np.all(r["_sums"]["runs"] == 1) and r["_sums"]["bits"][0] > 0
