"""AutoCorrFunction, remove_IFO and fine_sync (variant T4) against the oracle at the sizes of t4_cases.py, both dtypes: the
per-function entries are what test_gpu_task4_batch.py and test_gpu_task4_sizes.py compare the batched receiver with, and
test_gpu_channel_sync.py pins them at Nfft 1024 only.  Inputs: the first frame of each case (t4_cases.build_frames), streams cut
from it, and its clean TX stream for remove_IFO.  The fp32 runs get the frame cast to complex64; the oracle always gets the
complex128 frame (fine_sync: the same cast matrix on both sides, as test_fine_sync does).

Bounds: rho 1e-11 (fp64) / 1e-4 (fp32, the bound stated at acf4 in sync_core.hpp), FreqOffset 1e-9 / 1e-6, remove_IFO and fine_sync
the bounds of test_remove_ifo / test_fine_sync (1024-point tests).  None was measured: all are inherited."""
import warnings

import numpy as np
import pytest

import t4_cases as tc
from conftest import rel_l2

pytestmark = pytest.mark.gpu

DTYPES = [(np.complex128, "fp64"), (np.complex64, "fp32")]


def _streams():
    """(id, case name, how the stream is cut from frame 0): every row of the issue's list."""
    out = [(c.name, c.name, None) for c in tc.CASES]                   # n8192: W = 1024; n2048tg255: W = 255; n64: n_out = 792 < 1024
    out.append(("n1024tg100-cut", "n1024tg100", "cut"))                # a stream cut short, n_out = 2 * 1024 + 333
    out.append(("n256-short", "n256", "short"))                        # n_out = 777 < 1024
    out.append(("n512odd-zero-tail", "n512odd", "zero-tail"))          # zeros after the first plateau: NaN to the end, catch branch
    return out


def _acf_input(oracle, name, how):
    case = tc.BY_NAME[name]
    fr = tc.build_frames(oracle, case)
    x = fr["rx"][:, 0].copy()
    W, N = case.T_guard, case.Nfft
    if how == "cut":
        x = x[: W + N + 2 * 1024 + 333]
    elif how == "short":
        x = x[: W + N + 777]
    elif how == "zero-tail":
        f, g, h = tc.acf_of(oracle, case, fr)[0]["runs"]
        assert 0 <= g < h
        x[g + W + N + 1:] = 0                                           # x[m + Nfft] = 0 in every window from g + W + 1 on: 0 / 0
    return case, x


@pytest.mark.parametrize("dt,prec", DTYPES, ids=[p for _, p in DTYPES])
@pytest.mark.parametrize("sid,name,how", _streams(), ids=[s[0] for s in _streams()])
def test_autocorr_function_sizes(ofdm, oracle, sid, name, how, dt, prec):
    """rho, TgPosition and FreqOffset of one stream; where a whole window is zero (the tail add_STO leaves behind the frame) the
    reference's rho is 0 / 0 = NaN and so must the kernel's be: NaN is "not above" the threshold (AutoCorrFunction.m:6, :12)."""
    case, x = _acf_input(oracle, name, how)
    W, N = case.T_guard, case.Nfft
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        rho, pos, fo = ofdm.AutoCorrFunction(x.astype(dt), W, N)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rho_w, pos_w, fo_w, ok = oracle.AutoCorrFunction(x, W, N)
    rho = np.asarray(rho)
    f, g, h = tc.search_runs(np.abs(rho_w), W)
    upto = h if h >= 0 else rho_w.size - 1
    margin = float(np.nanmin(np.abs(np.abs(rho_w[W: upto + 1]) - tc.THR)))
    nan_w = np.isnan(rho_w)
    err = float(np.max(np.abs(rho - rho_w)[~nan_w])) if (~nan_w).any() else 0.0
    print(f"{sid} {prec}: n_out {rho_w.size}, NaN entries {int(nan_w.sum())}, max|rho - rho_w| {err:.3g}, |fo - fo_w| {abs(fo - fo_w):.3g}, "
          f"pos {pos} (oracle {pos_w}, ok {ok}), threshold margin {margin:.3g}")
    print(f"  entries finite here but NaN in the reference: {int(np.count_nonzero(~np.isnan(rho) & nan_w))}, NaN here but finite there: "
          f"{int(np.count_nonzero(np.isnan(rho) & ~nan_w))}")
    assert margin >= tc.M_ACF                                           # the position is decided firmly (t4_cases host conditions)
    assert rho.shape == rho_w.shape
    assert err < (1e-11 if prec == "fp64" else 1e-4)                    # over the entries the reference defines (not 0 / 0)
    assert np.array_equal(np.isnan(rho), nan_w)                         # 0 / 0 stays NaN = "not above" (AutoCorrFunction.m:6, :12)
    assert pos == pos_w
    assert abs(fo - fo_w) < (1e-9 if prec == "fp64" else 1e-6)
    if how == "zero-tail":
        assert not ok and pos == 65 and nan_w[-1] and any("guard" in str(m.message) for m in w)


def _clean_tx(oracle, name):
    case = tc.BY_NAME[name]
    return case, tc.build_frames(oracle, case)["tx0"]


@pytest.mark.parametrize("ifo", [0, 1, 30])
@pytest.mark.parametrize("name", ["n64", "n512odd", "n4096", "n8192"])
def test_remove_ifo_sizes(ofdm, oracle, name, ifo):
    case, tx = _clean_tx(oracle, name)
    rx = oracle.add_CFO(tx, ifo, case.Nfft)
    fixed_w, want = oracle.remove_IFO(rx, case.Nfft)
    fixed, got = ofdm.remove_IFO(rx, case.Nfft)
    f32, got32 = ofdm.remove_IFO(rx.astype(np.complex64), case.Nfft)
    print(f"{name} IFO {ifo}: oracle {want}, fp64 {got} rel_l2 {rel_l2(fixed, fixed_w):.3g}, fp32 {got32} rel_l2 {rel_l2(f32, fixed_w):.3g}")
    assert got == want and got32 == want
    assert rel_l2(fixed, fixed_w) < 1e-12
    assert rel_l2(f32, fixed_w) < 5e-7


@pytest.mark.parametrize("dt,tol", [(np.complex128, 1e-10), (np.complex64, 2e-5)], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", ["n64", "n512odd", "n4096", "n8192"])
def test_fine_sync_t4_sizes(ofdm, oracle, name, dt, tol):
    """The demodulator output of the case's first frame with a finite tau (oracle chain up to T4:310: a residual timing ramp of
    TgPosition's few samples, a common phase, the blanked first symbol, noise and the channel) through fine_sync, variant T4."""
    case = tc.BY_NAME[name]
    fr = tc.build_frames(oracle, case)
    rep = tc.replay(oracle, case, fr, (1, 1, 1))
    f0 = next(f for f, r in enumerate(rep) if r["H"] is not None and np.all(np.isfinite(r["H"])))
    X = rep[f0]["X0"].astype(dt)
    got, tau, ph = ofdm.fine_sync(X, fr["pc"], fr["pv"].astype(dt), 1, 1, variant="T4", return_estimates=True)
    want, tau_w, ph_w = oracle.fine_sync(X.astype(np.complex128), fr["pc"], fr["pv"], 1, 1, variant="T4")
    print(f"{name}: tau {tau:.6g} (oracle {tau_w:.6g}), phase {ph:.6g} ({ph_w:.6g}), rel_l2 {rel_l2(got, want):.3g}")
    assert np.isfinite(tau_w) and np.isfinite(ph_w)
    assert abs(tau - tau_w) < tol and abs(ph - ph_w) < 100 * tol
    assert rel_l2(got, want) < 200 * tol
    same = ofdm.fine_sync(X, fr["pc"], fr["pv"].astype(dt), 0, 0, variant="T4")
    assert np.array_equal(same, X)
