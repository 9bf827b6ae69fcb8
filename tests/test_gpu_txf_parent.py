"""The fused frame generator and the BER sweeps against the outputs of the commit before their call plan moved into txf_plan.hpp
and the sweeps into ofdm_ber_sweep.hip (tests/golden/txf_parent.json, written by `python tests/golden/make_golden.py
--txf-parent` from this tree against the library of that commit), bit for bit: SHA-256 of the bytes of every returned array,
the per-point doubles as hexadecimal bit patterns.  The four generator entries with and without the Scrambler register, the
Task-5 sweep (static and fading, MER and NMSE) and the Task-4 sweep (plain, _ex, _nmse, fading; flags (1, 1, 1) and (0, 0, 1);
mer_skip 0 and one symbol) at max_frames_per_chunk 0 and 2 -- 5 frames per point, so the cap leaves an uneven last chunk --
in both precisions, and every refused call of txf_cases.API with the text of its OfdmError.  A Task-4 point with a frame of
status < 0 keeps only its status counts (remove_IFO's index error leaves the frame's other outputs undefined).  The file lists
the fields it keeps: those that agreed between two runs of the parent."""
import hashlib
import json
import os

import numpy as np
import pytest

import txf_cases as tc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "txf_parent.json")
FIELDS = ("rx", "packed", "sc_packed", "taps", "Time_Delay", "Freq_Shift", "errors", "bits", "frame_errors", "mer_sums", "MER_dB",
          "frame_mer_sums", "nmse_sums", "NMSE", "frame_nmse", "status_counts", "cfo_abs_err", "error")
FRAMES, SNRS, SEEDS, FRAME0 = 5, (14.0, 26.0), (0x1234ABCD5, 77), 3
# Nfft 1024 x 5 symbols: 5760 samples, two channel segments, and the taps' halo crosses their boundary
SHAPES = {"q256": dict(nfft=256, n_carrier=64, comb=4, const="QPSK", n_symb=3),
          "a512": dict(nfft=512, n_carrier=128, comb=4, const="16QAM", n_symb=4),
          "p1024": dict(nfft=1024, n_carrier=400, comb=8, const="8PSK", n_symb=5)}
H = np.array([1.0, 0, 0, 0.5 - 0.25j, 0, 0, 0, 0.125j])
LINE = ([0, 3, 7], [1.0, 0.5, 0.25])
GEN = {"fused": dict(h=H), "fused_ex_fixed": dict(h=H, Time_Delay=5, Freq_Shift=0.3, want_draws=True),
       "fused_ex_drawn": dict(h=H, Time_Delay="random", Freq_Shift="random", want_draws=True),
       "fading": dict(fading=LINE, want_taps=True),
       "fading_ex": dict(fading=LINE, want_taps=True, Time_Delay="random", Freq_Shift="random", want_draws=True)}
T5 = {"static": dict(h=H), "fading": dict(fading=LINE, want_nmse=True, want_frame_nmse=True)}
T4 = {"plain": dict(h=H), "ex": dict(h=H, want_mer=True, want_frame_mer=True),
      "nmse": dict(h=H, want_mer=True, want_nmse=True, want_frame_nmse=True),
      "fading": dict(fading=LINE, want_mer=True, want_frame_mer=True, want_nmse=True, want_frame_nmse=True)}

RUNS = [("gen", s, p, e, scr) for s in SHAPES for p in ("fp32", "fp64") for e in GEN for scr in (0, 1)]
RUNS += [("t5", s, p, e, scr, ch) for s in SHAPES for p in ("fp32", "fp64") for e in T5 for scr, ch in ((0, 0), (1, 2))]
RUNS += [("t4", s, p, e, fl, ch) for s in SHAPES for p in ("fp32", "fp64") for e in T4 for fl in ("111", "001") for ch in (0, 2)]
RUNS += [("refused", c[0]) for c in tc.API]


def run_id(run):
    return "-".join(map(str, run))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _hex(a):
    return [f"{int(v):016x}" for v in np.ascontiguousarray(a, np.float64).ravel().view(np.uint64)]


_PLANS = {}


def _plan(ofdm, shape, precision, setup=""):
    """One plan per (shape, precision, set-up), kept for the module: "descr" descrambles with tc.REG, "mmse" has an MMSE operator."""
    key = (shape, precision, setup)
    if key not in _PLANS:
        from ofdm_course_amd import frames as fr
        plan = fr.make_plan(fr.config_small(dominant_taps=3, **SHAPES[shape]), ofdm, precision=precision)
        if setup == "descr":
            plan.set_descrambler(tc.REG)
        if setup == "mmse":
            plan.set_mmse(H, 20.0)
        _PLANS[key] = plan
    return _PLANS[key]


def _reduced(out, live=None):
    """The returned dictionary as the golden file stores it; live: the points of a Task-4 sweep whose other outputs are defined."""
    rec = {}
    for k, v in out.items():
        if k == "bits":
            rec[k] = int(v)
            continue
        v = np.asarray(v)
        if live is not None and k != "status_counts":
            v = v[live]
        if k in ("errors", "status_counts"):
            rec[k] = [int(x) for x in v.ravel()]
        elif k in ("mer_sums", "MER_dB", "nmse_sums", "NMSE", "cfo_abs_err"):
            rec[k] = _hex(v)
        else:
            rec[k] = _sha(v)
    return rec


def record(ofdm, run):
    """One run reduced to what the golden file stores: field -> value."""
    kind = run[0]
    if kind == "refused":
        _, method, setup, kw, rid, what, values = next(c for c in tc.API if c[0] == run[1])
        plan = _plan(ofdm, "q256", "fp32", setup)
        kw = {k: (v() if callable(v) else plan.n_data * plan.N_symb if v == "ND_NSYMB" else v) for k, v in kw.items()}
        args = (FRAMES,) if method == "tx_frames_fused" else (SNRS, FRAMES)
        with pytest.raises(ofdm.OfdmError) as e:
            getattr(plan, method)(*args, **kw)
        return dict(error=str(e.value))
    _, shape, precision, entry = run[:4]
    if kind == "gen":
        plan = _plan(ofdm, shape, precision)
        return _reduced(plan.tx_frames_fused(FRAMES, SNR=SNRS[0], seed=SEEDS[0], frame0=FRAME0,
                                             Register=tc.REG if run[4] else None, **GEN[entry]))
    if kind == "t5":
        scr, chunk = run[4:]
        plan = _plan(ofdm, shape, precision, "descr" if scr else "")
        return _reduced(plan.ber_sweep(SNRS, FRAMES, seeds=SEEDS, frame0=FRAME0, Register=tc.REG if scr else None,
                                       want_frame_errors=True, want_mer=True, want_frame_mer=True, max_frames_per_chunk=chunk,
                                       **T5[entry]))
    flags, chunk = run[4:]
    plan = _plan(ofdm, shape, precision)
    kw = dict(T4[entry])
    if kw.get("want_mer"):
        kw["mer_skip"] = plan.n_data if chunk else 0                  # one symbol's payload, or none
    imp = dict(Time_Delay="random", Freq_Shift="random") if flags == "111" else {}
    out = plan.ber_sweep_task4(SNRS, FRAMES, seeds=SEEDS, frame0=FRAME0, time_desync=int(flags[0]), freq_desync=int(flags[1]),
                               mp_desync=int(flags[2]), want_frame_errors=True, max_frames_per_chunk=chunk, **imp, **kw)
    sc = np.asarray(out["status_counts"])
    return _reduced(out, live=(sc[:, 2] == 0) & (sc[:, 3] == 0))


def refusal_of(run):
    c = next(c for c in tc.API if c[0] == run[1])
    return c[4], c[5], c[6]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_golden_lists_every_run(golden):
    assert sorted(golden["runs"]) == sorted(run_id(r) for r in RUNS)
    assert tuple(golden["fields"]) == FIELDS


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_run_matches_parent(ofdm, golden, run):
    got = record(ofdm, run)
    want = golden["runs"][run_id(run)]
    assert set(got) & set(golden["fields"]) == set(want)
    for field in want:
        assert got[field] == want[field], (run_id(run), field)
    if run[0] == "refused":
        rid, what, values = refusal_of(run)
        plan = _plan(ofdm, "q256", "fp32")
        values = (plan.n_data * plan.N_symb,) if values == "ND_NSYMB" else values
        assert ": " + tc.message(rid, what, values) + " (rc=" in got["error"]
