"""ofdm_rx_chain_task4 at every Nfft, guard and fallback path of its dispatch (t4_route_choose, t4_route.hpp; the stages of
ofdm_chain_t4.hip): the fixed cases of t4_cases.py (frames from the oracle alone, every frame firm: test_t4_cases_host.py)
against the per-function chain at the same precision and against the oracle replay of T4/Main_model_Task_4.m:278-347; no frame
is set aside.

What each row reaches (kernels, and the T4Route fields that select them; tests/t4_routes.py holds the whole route of every row):
  n64         form = staged natively: t4_align_kernel, ifo = segment_staged (t4_segment_kernel, first_above_kernel,
              t4_ifo_kernel), demod = demod_device, est = tau_phase_apply (fine_tau_kernel / fine_phase_kernel on the full grid,
              pilots_compact = 0, then fine_apply_kernel), means = kernel (t4_mean_pilots_kernel, compact = 0);
              acf = search (t4_acf_search_kernel) with n_out = 792 < one tile; the catch branch (TgPosition 65, status 1) on
              the noise frame, 65 < one symbol (72 samples);
              OFDM_T4_FULL_ACF -> acf = full: acf_kernel + acf_plateau_kernel + t4_scalars_kernel
  n64late     the same kernels on a stream longer than one tile: the first run starts in tile 0 and ends in tile 1 (the search's
              state machine carried across tiles), TgPosition's tile reloaded
  n256        staged form natively; the late frame as above
  n512odd     form = direct: demod = demod<1> (t4_demod_kernel<T, 1>, its slot_m and the 64-sample rotor chain) with sync on,
              ifo = segment_direct (t4_segment_direct_kernel, t4_ifo_finalize_kernel), est = means = fused (t4_fine_est_kernel);
              odd N_carrier: eq_vec = 0, the scalar equaliser path; the late frame
  n1024tg100  demod<2> with T_guard = 100 (stream indices sy * (N + Tg) + Tg + m);
              OFDM_T4_UNFUSED_SYNC -> est = tau_phase (fine_tau_kernel / fine_phase_kernel with pilots_compact = 1) and
              means = kernel with the lazy rotation (lazy_rot = 1)
  n2048odd    fp32: t4_demod_wave_supported refuses the odd carrier count -> demod<4> (t4_demod_kernel<float, 4>) and
              ifo = segment_direct with no switch set; fp64: t4_demod_kernel<double, 4>
  n2048tg255  fp32: ifo = wave (t4_ifo_wave_kernel) and demod = wave (t4_demod_wave_kernel) with an odd guard;
              OFDM_T4_NO_WAVE -> demod<4>
  n4096       demod<8>; 5 frames < T4_FT = 8 (t4_apply_operator_kernel, channel = dense, fp64);
              OFDM_T4_UNFUSED_SYNC; OFDM_T4_STAGED -> form = staged at 4096
  n8192       staged form natively; T_guard = ACF_MAXW = 1024: t4_acf_search_kernel with 81952 (fp64) bytes of dynamic LDS
              (acf_search_lds_bytes), E = EMAX = 8 entries per thread in acf_tile, the search starting in the second tile
              (from = W) past frame 0's plateau below W; OFDM_T4_FULL_ACF -> acf_kernel with 65568 bytes (fp64)

Deviations of the table from the issue's, both forced by the reference itself (details in t4_cases.py): n4096 and n8192 carry
5 symbols instead of 4 / 3 (and n8192 4 frames instead of 3, frame 0 with its first plateau below index W) -- estimate_channel.m:6 averages the blanked first symbol into the pilot means, H comes out (S - 1) / S
too small, and a 64-QAM frame of 4 or 3 symbols cannot pass the reference's BER < 0.2 gate whatever the draw (measured on the
oracle: 0.216 .. 0.221 at S = 4); and the frame whose first run crosses a tile border is a delayed ("late") frame, in n64late
for Nfft 64.

Tolerances: all inherited, none measured -- per-function chain: test_batch_equals_per_function_chain; oracle:
test_batch_against_oracle_replay_nfft2048_many_draws (FreqOffset 1e-9 / 1e-6, rel_l2(H) 1e-8 / 2e-4, 2 bits per frame in fp64,
decision_flip_audit with band 2e-3 in fp32); switch-only runs: test_gpu_chain_routes.py (fp64 bit for bit, H bit for bit where
the switch keeps the arithmetic -- OFDM_T4_FULL_ACF, OFDM_T4_UNFUSED_SYNC, OFDM_T4_NO_WAVE -- else rel_l2 < 1e-12 -- OFDM_T4_STAGED,
another transform; fp32 rel_l2(H) < 2e-5 and at most 2 * n_frames differing bits)."""
import numpy as np
import pytest

import t4_cases as tc
from conftest import rel_l2
from flip_audit import decision_flip_audit
from test_gpu_task4_batch import _per_function

pytestmark = pytest.mark.gpu

T4_SWITCHES = ("OFDM_T4_STAGED", "OFDM_T4_NO_WAVE", "OFDM_T4_WAVE_SPC", "OFDM_T4_FULL_ACF", "OFDM_T4_UNFUSED_SYNC",
               "OFDM_T4_DENSE_SPLINE")


def _run(ofdm, oracle, monkeypatch, case, precision, flags, env=()):
    """One rx_chain_task4 call on a plan of its own with only the switches of `env` set."""
    from ofdm_course_amd import frames as fr
    for v in T4_SWITCHES:
        monkeypatch.delenv(v, raising=False)
    for v in env:
        monkeypatch.setenv(v, "1")
    d = tc.build_frames(oracle, case)
    rx = d["rx"] if precision == "fp64" else d["rx"].astype(np.complex64)
    plan = ofdm.RxPlan(case.Nfft, case.T_guard, case.N_symb, case.N_carrier, d["pc"], d["dc"], d["col"],
                       int(np.ceil(case.N_carrier / 6)), 3, case.const, precision=precision)
    out = ofdm.rx_chain_task4(plan, rx, *flags, ref_bits_packed=fr.pack_bits(d["bits"]), want_h=True)
    nb, nbytes = plan.frame_bits, plan.frame_bytes
    assert nb == d["bits"].shape[1]
    packed = np.asarray(out["bits"]).copy()
    res = dict(packed=packed, bits=fr.unpack_bits(packed, nb), pad=fr.unpack_bits(packed, nbytes * 8)[:, nb:],
               errors=np.asarray(out["errors"]).astype(np.int64), H=np.asarray(out["H"]).copy(),
               TgPosition=np.asarray(out["TgPosition"]).copy(), FreqOffset=np.asarray(out["FreqOffset"]).copy(),
               IFO=np.asarray(out["IFO"]).copy(), status=np.asarray(out["status"]).copy(), rx=rx)
    plan.close()
    for v in env:
        monkeypatch.delenv(v, raising=False)
    return res


def _same_or_both_nan(a, b, tol):
    return abs(a - b) < tol or (np.isnan(a) and np.isnan(b))


def _params():
    for case in tc.CASES:
        for precision in ("fp64", "fp32"):
            for flags in tc.flag_sets(case):
                yield pytest.param(case, precision, flags, id=f"{case.name}-{precision}-{''.join(map(str, flags))}")


@pytest.mark.parametrize("case,precision,flags", list(_params()))
def test_case_matches_per_function_chain_and_oracle(ofdm, oracle, monkeypatch, case, precision, flags):
    f64 = precision == "fp64"
    d = tc.build_frames(oracle, case)
    nfr = tc.total_frames(case)
    got = _run(ofdm, oracle, monkeypatch, case, precision, flags)
    rep = tc.replay(oracle, case, d, flags)
    assert all(r["firm"] for r in rep)                                   # nothing to set aside (test_t4_cases_host.py)
    sync, mp = bool(flags[0] or flags[1]), bool(flags[2])

    # ---- always
    assert np.array_equal(got["errors"], np.count_nonzero(got["bits"] != d["bits"], axis=1))
    assert not got["pad"].any()
    want_status = [tc.expected_status(r) for r in rep]
    assert [int(s) for s in got["status"]] == want_status
    assert [f for f, r in enumerate(rep) if not r["ok"]] == (d["noise"] if sync else [])        # the catch-branch frames

    # ---- the per-function chain at the same precision
    dd = dict(Tg=case.T_guard, pil=d["pc"], dat=d["dc"], allc=d["allc"], pv=d["pv"])
    cfg_kw = dict(Nfft=case.Nfft, N_carrier=case.N_carrier, N_symb=case.N_symb, const=case.const)
    import warnings
    for f in range(nfr):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref = _per_function(ofdm, got["rx"][:, f].copy(), dd, cfg_kw, flags)
        assert int(got["TgPosition"][f]) == ref["TgPosition"], f
        assert _same_or_both_nan(float(got["FreqOffset"][f]), ref["FreqOffset"], 1e-12), f
        assert int(got["status"][f]) == ref["status"], f
        if ref["status"] >= 0:
            assert int(got["IFO"][f]) == ref["IFO"], f
            nbad = np.count_nonzero(got["bits"][f] != ref["bits"])
            assert nbad <= (0 if f64 else 4), (f, nbad)
            if mp:
                hg = got["H"][:, f]
                if np.all(np.isfinite(ref["H"])):
                    e = rel_l2(hg, ref["H"])
                    assert e < (1e-10 if f64 else 1e-4), (f, e)
                else:
                    assert np.array_equal(np.isnan(hg), np.isnan(ref["H"])), f

    # ---- the oracle replay
    compared = 0
    worst_h = worst_fo = 0.0
    for f, r in enumerate(rep):
        assert int(got["TgPosition"][f]) == r["TgPosition"], f
        assert _same_or_both_nan(float(got["FreqOffset"][f]), r["FreqOffset"], 1e-9 if f64 else 1e-6), f
        if sync and np.isfinite(r["FreqOffset"]):
            worst_fo = max(worst_fo, abs(float(got["FreqOffset"][f]) - r["FreqOffset"]))
        if r["IFO"] == "index error":
            continue
        assert int(got["IFO"][f]) == r["IFO"], f
        if mp:
            hg = got["H"][:, f]
            if not np.all(np.isfinite(r["H"])):     # the reference's blanked first symbol / an empty fine_sync mean makes it NaN
                assert np.array_equal(np.isnan(hg), np.isnan(r["H"])), f
                continue
            e = rel_l2(hg, r["H"])
            worst_h = max(worst_h, e)
            assert e < (1e-8 if f64 else 2e-4), (f, e)
        elif not np.all(np.isfinite(r["iq"])):
            continue
        if f64:
            nbad = np.count_nonzero(got["bits"][f] != r["bits"])
            assert nbad <= 2, (f, nbad)
        else:
            decision_flip_audit(oracle, got["bits"][f], r["bits"], r["iq"], case.const, band=2e-3,
                                what=f"{case.name} {precision} {flags} frame {f}")
        compared += 1
    print(f"{case.name} {precision} {flags}: {compared} frames compared with the oracle's decisions, worst rel_l2(H) {worst_h:.3g}, "
          f"worst |FreqOffset - oracle| {worst_fo:.3g}")
    if flags == (1, 1, 1):                           # the other flag sets leave the CFO or the STO in: fine_sync's tau is mostly NaN there
        assert compared >= 2, compared


SWITCH_RUNS = [("OFDM_T4_UNFUSED_SYNC", "n1024tg100", True), ("OFDM_T4_UNFUSED_SYNC", "n4096", True),
               ("OFDM_T4_FULL_ACF", "n64", True), ("OFDM_T4_FULL_ACF", "n8192", True),
               ("OFDM_T4_STAGED", "n4096", False), ("OFDM_T4_NO_WAVE", "n2048tg255", True)]


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("switch,name,same_arithmetic", SWITCH_RUNS, ids=[f"{s[0]}-{s[1]}" for s in SWITCH_RUNS])
def test_switch_only_run_equals_the_run_without_it(ofdm, oracle, monkeypatch, switch, name, same_arithmetic, precision):
    case = tc.BY_NAME[name]
    nfr = tc.total_frames(case)
    a = _run(ofdm, oracle, monkeypatch, case, precision, (1, 1, 1))
    b = _run(ofdm, oracle, monkeypatch, case, precision, (1, 1, 1), env=(switch,))
    for k in ("TgPosition", "IFO", "status"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["FreqOffset"], b["FreqOffset"], equal_nan=True)
    live = a["status"] >= 0
    ha, hb = a["H"][:, live], b["H"][:, live]
    assert np.array_equal(np.isnan(ha), np.isnan(hb))
    fin = np.isfinite(ha) & np.isfinite(hb)
    e = rel_l2(hb[fin], ha[fin])
    nbad = int(np.count_nonzero(a["bits"][live] != b["bits"][live]))
    print(f"{switch} {name} {precision}: rel_l2(H) {e:.3g}, {nbad} differing bits")
    if precision == "fp64":
        assert np.array_equal(a["packed"][live], b["packed"][live]) and np.array_equal(a["errors"][live], b["errors"][live])
        if same_arithmetic:
            assert np.array_equal(ha, hb, equal_nan=True)
        else:
            assert e < 1e-12
    else:
        assert e < 2e-5 and nbad <= 2 * nfr
