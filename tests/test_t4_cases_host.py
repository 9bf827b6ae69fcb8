"""The case table of t4_cases.py against the conditions the GPU tests (test_gpu_sync_sizes.py, test_gpu_task4_sizes.py) rely on,
with the oracle alone: every frame firm under every flag set the GPU tests use (so they set no frame aside), the index error
exactly on the attenuated frame, enough decodable frames, and draws that take the search kernel's state machine through its
tile-border branches.  The seeds of the table were chosen so that this passes; the conditions are not negotiable."""
import numpy as np
import pytest

import t4_cases as tc


@pytest.mark.parametrize("case", tc.CASES, ids=lambda c: c.name)
def test_every_frame_is_firm_under_every_flag_set(oracle, case):
    fr = tc.build_frames(oracle, case)
    assert fr["rx"].dtype == np.complex128 and fr["rx"].shape == ((case.Nfft + case.T_guard) * case.N_symb, tc.total_frames(case))
    for flags in tc.flag_sets(case):
        rep = tc.replay(oracle, case, fr, flags)
        soft = [(f, r["m_acf"], r["m_ifo"]) for f, r in enumerate(rep) if not r["firm"]]
        assert not soft, (case.name, flags, soft)


@pytest.mark.parametrize("case", tc.CASES, ids=lambda c: c.name)
def test_full_sync_draws(oracle, case):
    fr = tc.build_frames(oracle, case)
    rep = tc.replay(oracle, case, fr, (1, 1, 1))
    nb = fr["bits"].shape[1]
    failed = [f for f, r in enumerate(rep) if r["IFO"] == "index error"]
    assert failed == [tc.weak_frame(case)], failed                      # exactly the attenuated frame
    decoded = [f for f, r in enumerate(rep) if r["bits"] is not None and f not in fr["noise"]
               and np.count_nonzero(r["bits"] != fr["bits"][f]) < 0.2 * nb]              # the reference's own gate, T4:367
    assert len(decoded) >= 2, decoded
    assert any(r["H"] is not None and np.all(np.isfinite(r["H"])) for r in rep)
    n_out = fr["rx"].shape[0] - case.T_guard - case.Nfft
    for f, r in enumerate(rep):
        assert 1 <= r["TgPosition"] <= n_out, (f, r["TgPosition"])      # no status -2 anywhere
        assert r["ok"] == (f not in fr["noise"]), f                     # the catch branch on the noise frames and nowhere else


@pytest.mark.parametrize("name", ["n64late", "n256", "n512odd"])
def test_first_run_straddles_a_tile_border(oracle, name):
    """f in one 1024-tile, g in the next: the 1-based first run [first, last] contains a multiple of 1024."""
    case = tc.BY_NAME[name]
    fr = tc.build_frames(oracle, case)
    hits = []
    for f, a in enumerate(tc.acf_of(oracle, case, fr)):
        fi, g, h = a["runs"]
        if h >= 0 and (fi + 1 - 1) // 1024 != g // 1024:               # first = fi + 1, last = g: some 1024 k in [first, last]
            hits.append(f)
    assert hits and fr["late"] in hits, hits


@pytest.mark.parametrize("name", [c.name for c in tc.CASES if c.Nfft >= 1024])
def test_tg_position_and_second_run_in_different_tiles(oracle, name):
    """The reload branch of t4_acf_search_kernel: the tile in LDS when the search ends is not TgPosition's."""
    case = tc.BY_NAME[name]
    fr = tc.build_frames(oracle, case)
    for f, a in enumerate(tc.acf_of(oracle, case, fr)):
        assert a["ok"] and (a["pos"] - 1) // 1024 != a["runs"][2] // 1024, (f, a["pos"], a["runs"])


def test_n64_noise_frame_takes_the_catch_branch(oracle):
    case = tc.BY_NAME["n64"]
    fr = tc.build_frames(oracle, case)
    assert len(fr["noise"]) == 1
    r = tc.replay(oracle, case, fr, (1, 1, 1))[fr["noise"][0]]
    n_out = fr["rx"].shape[0] - case.T_guard - case.Nfft
    assert not r["ok"] and r["TgPosition"] == 65 and 65 <= n_out and 65 < case.Nfft + case.T_guard
    assert tc.expected_status(r) == 1


def test_n8192_early_frame_has_a_plateau_below_w(oracle):
    """AutoCorrFunction.m:13 (`th > WidthWindow`) is only visible on a frame that is above the threshold before index W."""
    case = tc.BY_NAME["n8192"]
    fr = tc.build_frames(oracle, case)
    a = tc.acf_of(oracle, case, fr)[0]
    amp = np.abs(a["rho"][: case.T_guard])
    lo = np.flatnonzero(amp > tc.THR)
    assert lo.size and lo[-1] + 1 < case.T_guard and a["runs"][0] > case.T_guard + 1024, (lo[[0, -1]] if lo.size else lo, a["runs"])
    assert float(np.min(np.abs(amp - tc.THR))) >= tc.M_ACF
