"""bit_error_profile (ofdm_bit_error_profile) alone, on planted errors: no receiver runs.  Every output against the numpy twin of
tests/error_cases.py, exactly, with the identities between the tables; host and device arrays, with and without the map and the
per-frame counts.

Geometries: `one` -- the smallest plan the constructor accepts (one data carrier, one symbol, BPSK: a frame of one bit); `small` --
108 bits of 8PSK, no multiple of 32, one tile; `big` -- the wave-skip0-64qam case of tests/routes.py with 4 symbols, 9216 bits =
288 words, so the gap carry crosses the tile of 256 words at bit 8192; `long` -- one data carrier on 17000 symbols: no multiple of
32, three tiles, and a symbol table that does not fit in LDS (the counts go to the global table); `long6` -- the same with six bits
per symbol, so that a word's errors fall into runs within one symbol (one global atomic per run)."""
import dataclasses

import numpy as np
import pytest

import error_cases as ec
import routes

pytestmark = pytest.mark.gpu

TILE_BITS = 256 * 32


def _plan(ofdm, name):
    from ofdm_course_amd import frames as fr
    if name == "big":
        case = dataclasses.replace(next(c for c in routes.CASES if c.name == "wave-skip0-64qam"), n_symb=4)
        return fr.make_plan(case.cfg(), ofdm, precision="fp32")
    nfft, nc, pil, dat, const, ns = {"one": (64, 2, [1], [2], "BPSK", 1),
                                     "small": (64, 16, [1, 5, 9, 13], [2, 3, 4, 6, 7, 8, 10, 11, 12, 14, 15, 16], "8PSK", 3),
                                     "long": (64, 2, [1], [2], "BPSK", 17000),
                                     "long6": (64, 4, [1], [2, 3, 4], "QPSK", 17000)}[name]
    return ofdm.RxPlan(nfft, 0, ns, nc, pil, dat, np.ones(len(pil), np.complex128), len(pil), 1, const, precision="fp64")


def _planted(plan, gap_bins, seed):
    """Seven frames: no error; one error; errors at bits 0, 31, 32, the bit in front of the tile boundary, the boundary and the last
    bit; two errors further apart than gap_bins (where the frame is that long); every bit wrong; a sparse random frame; a dense one."""
    fb, rng = plan.frame_bits, np.random.default_rng(seed)
    wrong = np.zeros((7, fb), np.uint8)
    wrong[1, fb // 2] = 1
    for i in (0, 31, 32, TILE_BITS - 1, TILE_BITS, fb - 1):
        if i < fb:
            wrong[2, i] = 1
    wrong[3, [min(3, fb - 1), min(3 + gap_bins + 1, fb - 1)]] = 1
    wrong[4, :] = 1
    wrong[5] = rng.random(fb) < min(1.0, 6.0 / fb)
    wrong[6] = rng.random(fb) < 0.5
    ref = rng.integers(0, 2, (7, fb), dtype=np.uint8)
    ref_p, bits_p = ec.pack(ref, plan.frame_bytes), ec.pack(ref ^ wrong, plan.frame_bytes)
    pad = 8 * plan.frame_bytes - fb
    if pad:                                                       # the padding differs: it must be masked
        bits_p[:, -1] |= np.uint8((1 << min(pad, 8)) - 1)
    return bits_p, ref_p, wrong


@pytest.mark.parametrize("gap_bins", [1, 64, 1024])
@pytest.mark.parametrize("name", ["one", "small", "big", "long", "long6"])
def test_planted_errors_equal_the_twin(ofdm, name, gap_bins):
    import torch
    plan = _plan(ofdm, name)
    bits, ref, wrong = _planted(plan, gap_bins, seed=len(name) + gap_bins)
    want = ec.profile(bits, ref, plan.n_data, plan.N_symb, plan.bps, gap_bins)
    assert np.array_equal(want["frame_errors"], wrong.sum(axis=1)) and want["frame_errors"][4] == plan.frame_bits
    if plan.frame_bits > gap_bins + 4:
        assert want["gap_above"] >= 1
    got = ofdm.bit_error_profile(plan, bits, ref, gap_bins=gap_bins, want_map=True, want_frames=True)
    ec.assert_profile(got, want)
    assert got["bits"] == 7 * plan.frame_bits and np.array_equal(got["dataCarriers"], plan.dataCarriers)
    assert float(got["FER"]) == want["frames_in_error"] / 7 and 4 <= want["frames_in_error"] <= 6
    assert np.array_equal(got["carrier_BER"], want["carrier_errors"] / float(7 * plan.N_symb * plan.bps))
    lean = ofdm.bit_error_profile(plan, bits, ref, gap_bins=gap_bins)
    assert "map" not in lean and "frame_errors" not in lean
    ec.assert_profile(lean, want, frames=False, emap=False)
    dev = ofdm.bit_error_profile(plan, torch.from_numpy(bits).cuda(), torch.from_numpy(ref).cuda(), gap_bins=gap_bins, want_map=True,
                                 want_frames=True)
    torch.cuda.synchronize()
    ec.assert_profile({k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in dev.items()}, want)
    plan.close()


def test_more_frames_than_workgroups_and_no_frames(ofdm):
    """1029 frames on at most 1024 workgroups: the frame stride and a last round of five workgroups; no frame at all: zeros."""
    plan = _plan(ofdm, "small")
    rng = np.random.default_rng(5)
    fb = plan.frame_bits
    wrong = (rng.random((1029, fb)) < rng.random((1029, 1)) * 0.2).astype(np.uint8)
    ref = rng.integers(0, 2, (1029, fb), dtype=np.uint8)
    bits, refp = ec.pack(ref ^ wrong, plan.frame_bytes), ec.pack(ref, plan.frame_bytes)
    got = ofdm.bit_error_profile(plan, bits, refp, gap_bins=16, want_map=True, want_frames=True)
    ec.assert_profile(got, ec.profile(bits, refp, plan.n_data, plan.N_symb, plan.bps, 16))
    none = ofdm.bit_error_profile(plan, bits[:0], refp[:0], gap_bins=16, want_map=True, want_frames=True)
    assert int(none["errors"]) == 0 and not none["carrier_errors"].any() and not none["map"].any() and none["frame_errors"].shape == (0,)
    plan.close()


def test_refusals(ofdm):
    plan = _plan(ofdm, "small")
    z = np.zeros((2, plan.frame_bytes), np.uint8)
    for gb in (0, 1025):
        with pytest.raises(ofdm.OfdmError, match=rf"bit_error_profile: gap_bins must be 1 \.\. 1024 \({gb}\)"):
            ofdm.bit_error_profile(plan, z, z, gap_bins=gb)
    with pytest.raises(ofdm.OfdmError, match=r"must be \[n_frames, frame_bytes\]"):
        ofdm.bit_error_profile(plan, z[:, :-1], z[:, :-1])
    plan.close()
