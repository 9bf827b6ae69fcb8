"""Host parts of the MMSE mode with h = ifft(H_LS) per frame (ofdm_rx_plan_set_mmse_ls), CPU only.

The rms delay spread of MMSE_CE.m:19-24 is formed from three Hermitian forms y^H A_q y on the pilot LS values y
(csrc/mmse_ls_forms.hpp).  The builder of the A_q is compiled here as a stand-alone program with the address and
undefined-behaviour sanitizers and run as a program; its output is checked against numpy's direct moments of
ifft(oracle.LS_CE(...)) to 1e-12 relative, for a percent layout (appended end pilot, uneven last knot spacing), a comb layout
whose last pilot is not the last carrier, and a prime N_carrier (the transform's odd-radix branch)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import routes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def forms_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no C++ compiler for the stand-alone program"
    exe = str(tmp_path_factory.mktemp("mmse_ls") / "mmse_ls_forms_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "mmse_ls_forms_main.cpp"), "-o", exe], check=True)
    return exe


def _forms(exe, tmp_path, oracle, pilots, nc):
    n_p = len(pilots)
    W = np.zeros((nc, n_p))                                  # interpolate.m as a real operator: its action on unit vectors
    for j in range(n_p):
        e = np.zeros(n_p, dtype=np.complex128)
        e[j] = 1.0
        W[:, j] = oracle.interpolate(e, pilots, nc, "spline").real
    wf, af = str(tmp_path / "W.bin"), str(tmp_path / "A.bin")
    W.ravel(order="F").tofile(wf)
    r = subprocess.run([exe, str(nc), str(n_p), wf, af], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr        # a sanitizer report is a failure
    A = np.fromfile(af, dtype=np.complex128).reshape(3, n_p, n_p)       # [q][j][i]
    return np.transpose(A, (0, 2, 1))                          # [q][i][j]


CASES = [("percent", routes.Case("percent", 2048, 800, 4, "16QAM", 3, (0, 3), pilots=("percent", 15, 2)).pilot_carriers(), 800),
         ("comb", np.arange(1, 401, 8), 400),
         ("prime", np.arange(1, 212, 3), 211)]


@pytest.mark.parametrize("name,pilots,nc", CASES, ids=[c[0] for c in CASES])
def test_forms_equal_the_direct_ifft_moments(forms_program, tmp_path, oracle, name, pilots, nc):
    A = _forms(forms_program, tmp_path, oracle, pilots, nc)
    n_p = len(pilots)
    assert np.allclose(A, np.conj(np.transpose(A, (0, 2, 1))), rtol=0, atol=1e-13 * np.abs(A).max())      # Hermitian
    rng = np.random.default_rng(5)
    k = np.arange(nc, dtype=np.float64)
    for trial in range(4):
        y = rng.standard_normal(n_p) + 1j * rng.standard_normal(n_p)
        if trial == 3:
            y = np.full(n_p, 0.7 - 0.2j)                       # a one-tap channel: all the energy at k = 0
        X = np.zeros((nc, 1), dtype=np.complex128)
        X[np.asarray(pilots) - 1, 0] = y
        h = np.fft.ifft(oracle.LS_CE(X, np.ones((n_p, 1)), pilots, nc))                   # Main_model_Task_5.m:178-179
        p = (h * np.conj(h)).real
        want = np.array([np.sum(p), np.sum(p * k), np.sum(p * k * k)])                     # MMSE_CE.m:20-23
        got = np.array([np.vdot(y, A[q] @ y) for q in range(3)])
        scale = np.array([want[0], want[0] * nc, want[0] * nc * nc])                       # a one-tap channel has want[1:] ~ 0
        print(name, trial, "relative", np.abs(got.real - want) / scale, "imag", np.abs(got.imag) / scale)
        assert np.all(np.abs(got.imag) <= 1e-12 * scale)
        if trial < 3:
            assert np.all(np.abs(got.real - want) <= 1e-12 * np.abs(want)), (got, want)
        else:
            assert np.all(np.abs(got.real - want) <= 1e-12 * scale), (got, want)


def test_binding_and_python_surface():
    """The entry is declared in the header, exported, bound with its three arguments, and RxPlan carries the switch.  (That
    set_mmse and set_mmse_ls clear each other is plan state, and a plan needs a device: tests/test_gpu_mmse_ls.py.)"""
    import ctypes as C
    from ofdm_course_amd import _lib as L
    from ofdm_course_amd import api
    lib = L.load()
    assert "int ofdm_rx_plan_set_mmse_ls(ofdm_rx_plan* plan, int enable, double snr_db);" in \
        open(os.path.join(ROOT, "include", "ofdm_mi355x.h")).read()
    assert list(lib.ofdm_rx_plan_set_mmse_ls.argtypes) == [C.c_void_p, C.c_int, C.c_double]
    assert callable(api.RxPlan.set_mmse_ls)


def test_driver_accepts_the_estimator():
    from ofdm_course_amd.drivers import sweep_ber
    a = sweep_ber.parse_args(["--config", "M", "--fused", "--fading", "EPA", "--nmse", "--mer", "--estimator", "mmse-ls"])
    assert a.estimator == "mmse-ls"
    assert sweep_ber.check_fading("M", "mmse-ls", True, "EPA", True) is None
    assert sweep_ber.check_fading("M", "mmse", True, "EPA", False) is not None           # the fixed-h mode stays refused
    assert sweep_ber.parse_args([]).estimator == "omp"
