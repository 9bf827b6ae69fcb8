"""CPU checks that make the assertions of tests/test_gpu_part2_tile_frames.py meaningful (cases: tests/part2_tile_cases.py):

* every case reaches the kernel variant its table line claims: realisations per wavefront of mp_batch_kernel from a restatement of
  mp_layout, 16-atom tiles and their parity, column groups of corr_mfma_f32, the OMP kernel and its form, and that the library
  serves the shape (LDS bounds of the MP, OMP, MMSE and equalise stages);
* every F puts a full workgroup in front of a ragged one for every split of the realisations;
* the oracle's per-realisation results can be told apart: a result in the wrong slot cannot pass;
* the oracle's own decisions are clear of ties: pick gaps of MP / OMP and decision margins of the equalised points per realisation."""
import itertools

import numpy as np
import pytest

import part2_tile_cases as tc
import routes

LIMIT = 150 * 1024
FP64_TOL = dict(rtol=1e-9, atol=1e-12)          # tests/test_gpu_part2_tile.py
FP32_TOL = dict(rtol=2e-3, atol=1e-6)


def _omp(np_, k, taps, f64):
    fpw, _, total = routes.omp_layout(np_, k, taps, f64, 0, {})
    return ("batch" if total <= LIMIT else "wide"), ("wave" if taps > tc.OMP_RT else "regs"), total


@pytest.mark.parametrize("case", tc.TILE_CASES, ids=[c.name for c in tc.TILE_CASES])
def test_tile_case_reaches_its_variant(case):
    pc, dc = case.layout()
    n_p, taps = len(pc), case.paths
    assert n_p == case.n_pilots and len(dc) == case.n_carrier - n_p > 0 and case.K >= n_p >= taps
    assert n_p <= 585                                                   # the MMSE stage of the part-2 tile
    chans = case.taps_list()
    assert all(t.shape[0] == taps for t in chans)
    assert all(0 <= np.real(t[:, 0]).max() < case.nfft for t in chans)
    keys = {t.tobytes() for t in chans}
    assert len(keys) == case.F[0]                                       # no two realisations share a channel
    line = [case.name, f"Np {n_p}"]
    for prec, want in zip(("fp64", "fp32"), case.fpw):
        f64 = prec == "fp64"
        fpw = tc.mp_fpw(n_p, taps, f64)
        assert fpw == want, (case.name, prec, fpw)
        assert tc.mp_lds_bytes(n_p, taps, f64) <= LIMIT
        route, form, total = _omp(n_p, case.K, taps, f64)
        assert (route, form) == ("batch", case.omp), (case.name, prec, route, form, total)
        # chain_split_fits (chain_route.hpp): the equalise stage holds the frame
        assert (16 if f64 else 8) * case.n_carrier + ((len(dc) * tc.N_SYMB + 31) & ~31) <= routes.SPLIT_LDS_LIMIT
        line.append(f"{prec}: fpw {fpw} (FB {4 * fpw}), OMP {route}/{form} {total} B")
        if prec in case.precisions:
            # a full workgroup in front of a ragged one: MP (FB), the spline operator (P2_FT), MMSE (4 wavefronts)
            for g in (4 * fpw, tc.P2_FT, 4):
                assert case.F[0] > g and case.F[0] % g != 0, (case.name, prec, g)
    mfma = tc.mp_mfma(n_p, False)
    assert (n_p // 16 if mfma else 0) == case.tiles
    if mfma:
        fb = 4 * case.fpw[1]
        line.append(f"MFMA MP: {case.tiles} tiles ({'even' if case.tiles % 2 == 0 else 'odd: two == false'}), "
                    f"{(fb + 7) // 8} column group(s) of {min(fb, 8)}")
    else:
        line.append("scalar MP in fp32")
        assert n_p % 4 != 0 and n_p % 8 != 0
    print("  ".join(line))


def test_table_claims():
    """The properties the table lists, each on the case that is there for it."""
    T = tc.TILE
    assert T["A"].tiles == 2 and T["A"].fpw == (4, 4) and T["A"].F == (37, 1) and T["A7"].F[0] == 37
    assert T["B"].tiles % 2 == 1 and T["B"].n_carrier % 128 == 64 and T["B"].n_carrier % 256 != 0
    assert T["C"].n_pilots % 4 != 0 and T["C"].n_carrier < 128 and T["C"].K == T["C"].nfft
    assert any(np.real(t[:, 0]).max() >= T["C"].n_carrier for t in T["C"].taps_list())    # the skipped tap of cvals
    assert T["D"].fpw == (2, 4) and tc.mp_fpw(142, 7, True) == 4 and tc.mp_fpw(144, 7, True) == 2   # (143 with the 7 picks)
    assert T["E"].fpw == (1, 2) and tc.mp_fpw(286, 7, True) == 2 and tc.mp_fpw(288, 7, True) == 1
    assert T["F"].fpw[1] == 1 and T["F"].precisions == ("fp32",) and T["F"].tiles == 36
    d = [tuple(np.real(t[:, 0]).astype(int)) for t in T["AV"].taps_list()]
    assert len(set(d)) == 3 and all(d[f] != d[f + 1] for f in range(len(d) - 1)) and len(set(d[0])) == 9
    assert len({tuple(np.real(t[:, 0]).astype(int)) for t in T["A"].taps_list()}) == 1   # (one rate: one set of delays)
    assert {c.profile for c in (T["A"], T["B"], T["C"])} == {"ETU"} and {T[n].profile for n in ("A7", "D", "E", "F")} == {"EPA"}
    M = tc.MSE
    assert (M["M1"].nfft, M["M1"].n_carrier, M["M1"].comb, M["M1"].K) == (T["A"].nfft, T["A"].n_carrier, 4, T["A"].K)
    assert len(M["M1"].snrs) == 37 and M["M1"].snrs[0] == 0 and M["M1"].snrs[-1] == 30
    d = [int(np.real(r[0])) for r in M["M3"].channel_taps]
    assert d.count(10) == 2 and sum(M["M3"].n_carrier <= v < M["M3"].nfft for v in d) == 1


@pytest.mark.parametrize("case", tc.MSE_CASES, ids=[c.name for c in tc.MSE_CASES])
def test_mse_case_reaches_its_variant(case):
    n_p, taps = case.n_pilots, len(case.channel_taps)
    assert tc.mp_fpw(n_p, taps, False) == case.fpw32 and tc.mmse_wpw(n_p, True) == case.wpw
    for prec in case.precisions:
        f64 = prec == "fp64"
        assert tc.mp_lds_bytes(n_p, taps, f64) <= LIMIT and 16 * 2 * case.n_carrier <= LIMIT and 16 * 4 * n_p * case.wpw <= LIMIT
        route, form, total = _omp(n_p, case.K, taps, f64)
        assert (route, form) == ("batch", "regs")
        print(case.name, prec, f"Np {n_p}: MP fpw {tc.mp_fpw(n_p, taps, f64)}, mmse wpw {case.wpw}, OMP {route}/{form} {total} B,",
              f"MFMA tiles {n_p // 16 if tc.mp_mfma(n_p, f64) else 0}")
    if case.name == "M2":
        assert n_p > 1200 and n_p // 16 == 80 and case.n_carrier & (case.n_carrier - 1) and case.K == case.nfft


def _pairs_apart(v, rtol, atol):
    d = [abs(a - b) > rtol * max(abs(a), abs(b)) + atol for a, b in itertools.combinations(v, 2)]
    return np.array(d)


@pytest.mark.parametrize("case", tc.TILE_CASES, ids=[c.name for c in tc.TILE_CASES])
def test_realisations_can_be_told_apart(oracle, case):
    """Per estimator the NMSE values of any two realisations differ by more than 100 times the fp64 tolerance, 90 % of the pairs
    by more than the fp32 tolerance, and the error counts are not all equal: a slot mix-up cannot pass."""
    full = tc.oracle_tile_full(oracle, case)
    for e in range(4):
        v = full["nmse"][e]
        assert np.all(_pairs_apart(v, 100 * FP64_TOL["rtol"], 100 * FP64_TOL["atol"])), (case.name, e)
        share = np.mean(_pairs_apart(v, FP32_TOL["rtol"], FP32_TOL["atol"]))
        assert share >= 0.9, (case.name, e, share)
        assert len(set(full["errors"][e].tolist())) > 1, (case.name, e)
    assert np.all(full["errors"] <= full["bits"])


@pytest.mark.parametrize("case", tc.MSE_CASES, ids=[c.name for c in tc.MSE_CASES])
def test_points_can_be_told_apart(oracle, case):
    full = tc.oracle_mse_tile_full(oracle, case)
    for e in range(4):
        assert np.all(_pairs_apart(full["mse"][e], 100 * FP64_TOL["rtol"], 100 * FP64_TOL["atol"])), (case.name, e)
        assert np.mean(_pairs_apart(full["mse"][e], FP32_TOL["rtol"], 0.0)) >= 0.9, (case.name, e)


@pytest.mark.parametrize("case", tc.TILE_CASES, ids=[c.name for c in tc.TILE_CASES])
def test_decision_margins_of_the_oracle(oracle, case):
    full = tc.oracle_tile_full(oracle, case)
    F = case.F[0]
    loose = tc.fp32_loose(full)
    print(case.name, "seed", case.seed, "smallest MP pick gap", full["mp_gap"].min(), "OMP pick gap", full["omp_gap"].min(),
          "decision margin", full["margin"].min(), "fp32_loose", f"{int(loose.sum())}/{F}", np.flatnonzero(loose).tolist())
    assert full["mp_gap"].shape == full["omp_gap"].shape == (F,)
    assert np.all(full["mp_gap"] > tc.FP64_GAP) and np.all(full["omp_gap"] > tc.FP64_GAP) and np.all(full["margin"] > tc.FP64_GAP)
    assert loose.sum() <= 0.1 * F
    assert not np.any(loose & tc.boundary_slots(F))


@pytest.mark.parametrize("case", tc.MSE_CASES, ids=[c.name for c in tc.MSE_CASES])
def test_pick_gaps_of_the_mse_points(oracle, case):
    full = tc.oracle_mse_tile_full(oracle, case)
    n = len(case.snrs)
    loose = np.minimum(full["mp_gap"], full["omp_gap"]) < tc.FP32_GAP
    print(case.name, "seed", case.seed, "smallest MP pick gap", full["mp_gap"].min(), "OMP pick gap", full["omp_gap"].min(),
          "fp32_loose", f"{int(loose.sum())}/{n}")
    assert full["mp_gap"].shape == full["omp_gap"].shape == (n,)
    assert np.all(full["mp_gap"] > tc.FP64_GAP) and np.all(full["omp_gap"] > tc.FP64_GAP)
    if "fp32" in case.precisions:
        assert not loose.any()                                          # the fp32 comparison sets no point aside


def test_the_two_host_rules_of_the_mse_tile_on_the_oracle(oracle):
    """M3: the oracle convolves with the dense vector get_MP_channel_resp builds -- the later row at delay 10 wins -- and the
    error is measured against its transform, the tap at delay 150 >= N_carrier included."""
    case = tc.MSE["M3"]
    h, H = oracle.get_MP_channel_resp(case.taps(), case.nfft)
    assert h[10] == case.channel_taps[3][1] != case.channel_taps[2][1] and len(h) == 151 and h[150] == case.channel_taps[-1][1]
    assert np.allclose(H, np.fft.fft(h, case.nfft))
