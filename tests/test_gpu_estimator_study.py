"""ofdm_estimator_study (csrc/ofdm_est_study.hip, RxPlan.estimator_study): LS, MMSE, MP and OMP on the same generated frames, per
frame against the oracle's replay of that frame (tests/estimator_cases.py) on the frames tx_frames_fused returns for the same
arguments, bitwise independence of the chunking and of a split by frame0, the identities between its outputs, the cross-checks
against ber_sweep and task5_part2_tile, and its refusals.  3 points x 37 frames: ragged for every split into workgroups."""
import ctypes as C

import numpy as np
import pytest

import estimator_cases as ec
import part2_tile_cases as tc

pytestmark = pytest.mark.gpu

FP64_TOL = dict(rtol=1e-9, atol=1e-12)
FP32_TOL = dict(rtol=2e-3, atol=1e-6)
STATIC_TAPS = ec.STATIC_TAPS


def _static_h(precision):
    return ec.static_h().astype(np.complex128 if precision == "fp64" else np.complex64)


def _chan(case, channel, precision):
    return dict(h=_static_h(precision)) if channel == "static" else dict(fading=ec.fading(case))


@pytest.fixture(scope="module")
def plans(ofdm, oracle):
    cache = {}

    def get(name, precision, channel="fading"):
        key = (name, precision, channel)
        if key not in cache:
            case = ec.CASES[name]
            cache[key] = ec.make_plan(ofdm, oracle, case, precision, len(STATIC_TAPS) if channel == "static" else None)
        return cache[key]
    yield get
    for p in cache.values():
        p.close()


@pytest.fixture(scope="module")
def studies(plans):
    """RxPlan.estimator_study(POINTS, FRAMES, want_frames=True) once per (case, precision, channel, mmse)."""
    cache = {}

    def get(name, precision, channel, mmse):
        key = (name, precision, channel, mmse)
        if key not in cache:
            cache[key] = plans(name, precision, channel).estimator_study(
                ec.POINTS, ec.FRAMES, mmse=mmse, seeds=ec.seeds(name), want_frames=True, **_chan(ec.CASES[name], channel, precision))
        return cache[key]
    return get


@pytest.fixture(scope="module")
def replays(oracle, plans):
    """The oracle's replay of the generator's own frames, once per (case, precision, channel, mmse)."""
    cache = {}

    def get(name, precision, channel, mmse):
        key = (name, precision, channel, mmse)
        if key in cache:
            return cache[key]
        case, plan = ec.CASES[name], plans(name, precision, channel)
        pts = []
        for snr, seed in zip(ec.POINTS, ec.seeds(name)):
            g = plan.tx_frames_fused(ec.FRAMES, SNR=snr, seed=seed, frame0=0, want_taps=channel == "fading",
                                     **_chan(case, channel, precision))
            bits = np.unpackbits(np.asarray(g["packed"]), axis=1)[:, :plan.frame_bits]
            if channel == "fading":
                delays, taps = ec.fading(case)[0], np.asarray(g["taps"])
            else:
                delays = [d for d, _ in STATIC_TAPS]
                taps = np.tile(np.array([a for _, a in STATIC_TAPS], dtype=np.complex128), (ec.FRAMES, 1))
            pts.append(dict(rx=np.asarray(g["rx"]).astype(np.complex128), taps=taps, bits=bits, delays=delays))
        cache[key] = ec.replay(oracle, case, pts, ec.POINTS, mmse)
        return cache[key]
    return get


FP64_RUNS = ec.FP64_RUNS


@pytest.mark.parametrize("name,channel", [("A", "fading"), ("A", "static"), ("D", "fading")])
def test_the_host_restatement_is_the_generators_frames(oracle, plans, name, channel):
    """estimator_cases.host_frames, on which the seeds were chosen and the margins are asserted without a GPU
    (tests/test_estimator_cases_host.py), against tx_frames_fused for the same arguments in fp64: the same bits and taps, the
    samples to rounding -- so what the oracle alone clears, the frames compared here clear."""
    case, plan = ec.CASES[name], plans(name, "fp64", channel)
    for snr, seed in zip(ec.POINTS, ec.seeds(name)):
        g = plan.tx_frames_fused(ec.FRAMES, SNR=snr, seed=seed, frame0=0, want_taps=channel == "fading", **_chan(case, channel, "fp64"))
        want = ec.host_frames(oracle, case, snr, seed, ec.FRAMES, channel=channel)
        assert np.array_equal(np.unpackbits(np.asarray(g["packed"]), axis=1)[:, :plan.frame_bits], want["bits"])
        if channel == "fading":
            assert np.max(np.abs(np.asarray(g["taps"]) - want["taps"])) <= 1e-13
        rx = np.asarray(g["rx"])
        assert rx.shape == want["rx"].shape
        assert np.max(np.abs(rx - want["rx"])) <= 1e-12 * np.max(np.abs(want["rx"]))


@pytest.mark.parametrize("name,channel,mmse", FP64_RUNS, ids=["-".join(r) for r in FP64_RUNS])
def test_every_frame_equals_the_oracle_fp64(studies, replays, name, channel, mmse):
    """frame_errors equal to the oracle's on every frame -- every frame of every run clears the 1e-6 margins, which
    tests/test_estimator_cases_host.py asserts on the oracle alone and this test again on the frames it compares --, frame_nmse to
    the tile's fp64 tolerance."""
    got, want = studies(name, "fp64", channel, mmse), replays(name, "fp64", channel, mmse)
    fe, fn = np.asarray(got["frame_errors"]).astype(np.int64), np.asarray(got["frame_nmse"])
    assert fe.shape == fn.shape == (len(ec.POINTS), ec.FRAMES, 4)
    clear = want["clear"]
    print(name, channel, mmse, "frames clear of the margins", int(clear.sum()), "of", clear.size, "largest relative NMSE deviation",
          np.max(np.abs(fn - want["nmse"]) / want["nmse"], axis=(0, 1)), "frames with other bit errors",
          np.argwhere(np.any(fe != want["errors"], axis=2)).tolist())
    assert clear.all()
    assert np.array_equal(fe, want["errors"])
    assert np.allclose(fn, want["nmse"], **FP64_TOL)


@pytest.mark.parametrize("name,mmse", [("A", "ls"), ("A", "genie"), ("C", "ls"), ("C", "genie")])
def test_every_frame_equals_the_oracle_fp32(studies, replays, name, mmse):
    """fp32 (A: the matrix-core MP; C: the scalar MP, np % 4 != 0, a path outside 1..N_carrier): frame_nmse to the project's fp32
    NMSE tolerance and the bit errors exact, on the frames that are not fp32_loose (at most 10 % of the case are)."""
    got, want = studies(name, "fp32", "fading", mmse), replays(name, "fp32", "fading", mmse)
    fe, fn = np.asarray(got["frame_errors"]).astype(np.int64), np.asarray(got["frame_nmse"])
    ok = ~want["loose"]
    print(name, mmse, "fp32_loose", np.argwhere(~ok).tolist(), "largest relative NMSE deviation",
          np.max(np.abs(fn[ok] - want["nmse"][ok]) / want["nmse"][ok], axis=0), "largest bit-error difference",
          np.max(np.abs(fe[ok] - want["errors"][ok]), axis=0))
    assert ok.mean() >= 0.9
    assert np.all(np.isfinite(fn))
    assert np.allclose(fn[ok], want["nmse"][ok], **FP32_TOL)
    assert np.array_equal(fe[ok], want["errors"][ok])


def _bits_of(out):
    return [np.asarray(out[k]).copy() for k in ("errors", "nmse_sums", "nmse_dropped", "frame_errors", "frame_nmse")]


def _same(a, b):
    return all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("mmse", ["ls", "genie"])
def test_no_output_depends_on_the_chunking_or_on_a_split_by_frame0(plans, studies, precision, mmse):
    case, plan = ec.CASES["A"], plans("A", precision)
    full = _bits_of(studies("A", precision, "fading", mmse))
    kw = dict(fading=ec.fading(case), mmse=mmse, seeds=ec.seeds("A"), want_frames=True)
    for cap in (5, 16):
        assert _same(_bits_of(plan.estimator_study(ec.POINTS, ec.FRAMES, max_frames_per_chunk=cap, **kw)), full), cap
    a = _bits_of(plan.estimator_study(ec.POINTS, 21, **kw))
    b = _bits_of(plan.estimator_study(ec.POINTS, ec.FRAMES - 21, frame0=21, **kw))
    assert np.array_equal(a[0] + b[0], full[0]) and np.array_equal(a[2] + b[2], full[2])
    assert np.concatenate([a[3], b[3]], axis=1).tobytes() == full[3].tobytes()
    assert np.concatenate([a[4], b[4]], axis=1).tobytes() == full[4].tobytes()
    # the device flavour: the same bits, tensors on the device
    dev = plan.estimator_study(ec.POINTS, ec.FRAMES, device="cuda:0", **kw)
    assert dev["errors"].is_cuda and dev["frame_nmse"].is_cuda
    assert _same([dev[k].cpu().numpy() for k in ("errors", "nmse_sums", "nmse_dropped", "frame_errors", "frame_nmse")], full)


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_identities_between_the_outputs(plans, studies, precision):
    out = studies("A", precision, "fading", "ls")
    fe, fn = np.asarray(out["frame_errors"]).astype(np.int64), np.asarray(out["frame_nmse"])
    assert np.array_equal(np.asarray(out["errors"]), fe.sum(axis=1))
    assert out["rows"] == ec.ROWS and out["bits"] == ec.FRAMES * plans("A", precision).frame_bits
    for p in range(len(ec.POINTS)):
        for e in range(4):
            s, d = ec.in_order_sum(fn[p, :, e])
            assert np.asarray(out["nmse_sums"])[p, e] == s and np.asarray(out["nmse_dropped"])[p, e] == d == 0
    nc = ec.CASES["A"].n_carrier
    assert np.array_equal(np.asarray(out["NMSE"]), np.asarray(out["nmse_sums"]) / (float(ec.FRAMES) * nc))
    assert np.array_equal(np.asarray(out["BER"]), np.asarray(out["errors"]) / float(out["bits"]))
    # only the sums asked for: the same values; without error outputs no equaliser runs and H of MP / OMP is the taps' transform
    plan = plans("A", precision)
    kw = dict(fading=ec.fading(ec.CASES["A"]), seeds=ec.seeds("A"))
    lean = plan.estimator_study(ec.POINTS, ec.FRAMES, **kw)
    assert all(np.asarray(lean[k]).tobytes() == np.asarray(out[k]).tobytes() for k in ("errors", "nmse_sums", "nmse_dropped"))
    assert "frame_errors" not in lean and "frame_nmse" not in lean


@pytest.mark.parametrize("mmse", ["ls", "genie"])
def test_without_error_outputs_no_equaliser_runs(plans, studies, mmse):
    """Only nmse_sums asked for, which the C entry alone can be told (the Python method always takes errors): no reference bits are
    made, no equaliser runs and H of MP and OMP is the transform of their taps (the MSE tile's tail of the estimator body), where
    the full call takes it from the equalise stage: the same sums to the fp64 tolerance, LS and MMSE bit for bit."""
    from ofdm_course_amd import _lib as L
    case, plan = ec.CASES["A"], plans("A", "fp64")
    full = np.asarray(studies("A", "fp64", "fading", mmse)["nmse_sums"])
    fd = ec.fading(case)
    dl = np.ascontiguousarray(np.asarray(fd[0], dtype=np.int32))
    pw = np.ascontiguousarray(np.asarray(fd[1], dtype=np.float64))
    snr, seeds = np.array(ec.POINTS, dtype=np.float64), np.array(ec.seeds("A"), dtype=np.uint64)
    ptr = lambda a: C.c_void_p(a.ctypes.data)                                        # noqa: E731
    for cap in (0, 5):
        ns = np.full((3, 4), np.nan)
        L.check(L.load().ofdm_estimator_study(plan.handle, None, 0, ptr(dl), ptr(pw), dl.size, ptr(snr), ptr(seeds), 3, ec.FRAMES, 0,
                                              {"ls": 0, "genie": 1}[mmse], cap, None, ptr(ns), None, None, None,
                                              L.OFDM_F64 | L.OFDM_HOST), "estimator_study")
        print(mmse, cap, "largest relative deviation of nmse_sums per row", np.max(np.abs(ns / full - 1), axis=0))
        assert ns[:, :2].tobytes() == full[:, :2].tobytes()
        assert np.allclose(ns, full, **FP64_TOL)


def test_a_genie_frame_without_a_tap_inside_the_band_is_dropped(ofdm, oracle, plans, studies):
    """One tap at delay 130 >= N_carrier = 128: tau_rms has no energy to measure, every frame's MMSE row is dropped; LS, MP and OMP
    are what they are in the ls mode, where all four rows are served."""
    case = ec.CASES["A"]
    plan = ec.make_plan(ofdm, oracle, case, "fp64", n_taps=1)
    kw = dict(fading=([130], [1.0]), seeds=ec.seeds("A"), want_frames=True)
    genie = plan.estimator_study(ec.POINTS, ec.FRAMES, mmse="genie", **kw)
    ls = plan.estimator_study(ec.POINTS, ec.FRAMES, mmse="ls", **kw)
    plan.close()
    drop = np.asarray(genie["nmse_dropped"])
    assert np.array_equal(drop[:, 1], np.full(len(ec.POINTS), ec.FRAMES)) and not drop[:, [0, 2, 3]].any()
    assert np.all(np.isnan(np.asarray(genie["frame_nmse"])[:, :, 1])) and np.all(np.asarray(genie["nmse_sums"])[:, 1] == 0)
    assert np.all(np.isnan(np.asarray(genie["NMSE"])[:, 1]))
    for k in ("nmse_sums", "frame_nmse", "frame_errors", "errors"):
        assert np.asarray(genie[k])[..., [0, 2, 3]].tobytes() == np.asarray(ls[k])[..., [0, 2, 3]].tobytes(), k
    assert not np.asarray(ls["nmse_dropped"]).any() and np.all(np.isfinite(np.asarray(ls["frame_nmse"])))


def test_omp_and_mmse_ls_rows_equal_the_sweeps(ofdm, oracle, plans, studies, replays):
    """fp64, case A, on the frames that clear the margins: the OMP row's frame errors are those of ber_sweep(fading=) for the same
    arguments, the mmse = "ls" MMSE row's those of the same sweep on a set_mmse_ls plan; the NMSE of both to the fp64 tolerance."""
    case = ec.CASES["A"]
    out, clear = studies("A", "fp64", "fading", "ls"), replays("A", "fp64", "fading", "ls")["clear"]
    fe, fn = np.asarray(out["frame_errors"]).astype(np.int64), np.asarray(out["frame_nmse"])
    kw = dict(fading=ec.fading(case), seeds=ec.seeds("A"), want_frame_errors=True, want_nmse=True, want_frame_nmse=True)
    for row, ls in ((3, False), (1, True)):
        plan = ec.make_plan(ofdm, oracle, case, "fp64")
        if ls:
            plan.set_mmse_ls(ec.POINTS[0])                          # (the sweep estimates every point at the point's own SNR)
        sw = plan.ber_sweep(ec.POINTS, ec.FRAMES, **kw)
        plan.close()
        sfe = np.asarray(sw["frame_errors"]).astype(np.int64)
        assert np.array_equal(fe[:, :, row][clear], sfe[clear]), row
        # OMP: the same taps through two transforms.  MMSE: the receiver solves with the moment forms of mmse_ls_forms.hpp, the
        # study with the Levinson recursion of the tiles: two fp64 solutions of a system whose condition number is at most about
        # snr * Np (1e3 * 32 here), so they agree to about 1e5 eps = 1e-11 in H and twice that in the error sum; 1e-8 is asked
        tol = dict(rtol=1e-8, atol=1e-12) if ls else FP64_TOL
        print("row", row, "largest relative deviation of frame_nmse", np.max(np.abs(fn[:, :, row] / np.asarray(sw["frame_nmse"]) - 1)))
        assert np.allclose(fn[:, :, row], np.asarray(sw["frame_nmse"]), **tol), row
        assert np.allclose(np.asarray(out["NMSE"])[:, row], np.asarray(sw["NMSE"]), rtol=tol["rtol"]), row
        if clear.all():
            assert np.array_equal(np.asarray(out["errors"])[:, row], np.asarray(sw["errors"]))


def test_static_channel_rows_equal_the_part2_tile(ofdm, oracle, plans, studies):
    """fp64, case A, a static channel, one point: the tile takes the generator's frames one by one (its TX stream is the frame in
    front of the channel: the generator without h at the same seed, noise first) with the channel's taps and the frame's payload;
    its four rows equal the study's genie rows: bit errors exactly, NMSE = frame_nmse / N_carrier to the fp64 tolerance."""
    from ofdm_course_amd import frames as fr
    case, plan = ec.CASES["A"], plans("A", "fp64", "static")
    snr, seed, nf = ec.POINTS[1], ec.seeds("A")[1], 8
    out = plan.estimator_study([snr], nf, h=_static_h("fp64"), mmse="genie", seeds=[seed], want_frames=True)
    g = plan.tx_frames_fused(nf, SNR=snr, seed=seed, frame0=0)
    taps = np.array([[d, a] for d, a in STATIC_TAPS], dtype=np.complex128)
    for f in range(nf):
        t = ofdm.task5_part2_tile(plan, np.ascontiguousarray(np.asarray(g["rx"])[:, f]), [taps], snr, np.asarray(g["packed"])[f])
        assert np.array_equal(np.asarray(t["errors"]).astype(np.int64)[:, 0], np.asarray(out["frame_errors"]).astype(np.int64)[0, f]), f
        assert np.allclose(np.asarray(t["nmse"])[:, 0] * case.n_carrier, np.asarray(out["frame_nmse"])[0, f], **FP64_TOL), f


def test_refusals_come_before_any_output_is_written(ofdm, oracle, plans):
    from ofdm_course_amd import _lib as L
    case = ec.CASES["A"]
    plan = ec.make_plan(ofdm, oracle, case, "fp64")
    fd = ec.fading(case)
    with pytest.raises(ofdm.OfdmError, match='mmse must be "ls" or "genie"'):
        plan.estimator_study(ec.POINTS, 5, fading=fd, mmse="lmmse")
    with pytest.raises(ofdm.OfdmError, match="give h .one channel for every frame. or taps"):
        plan.estimator_study(ec.POINTS, 5, fading=fd, h=_static_h("fp64"))
    with pytest.raises(ofdm.OfdmError, match="bad arguments"):
        plan.estimator_study(ec.POINTS, 5, fading=fd, max_frames_per_chunk=65536)
    plan.set_descrambler(tc_register())
    with pytest.raises(ofdm.OfdmError, match="estimator_study: the study runs unscrambled"):
        plan.estimator_study(ec.POINTS, 5, fading=fd)
    plan.set_descrambler(None)

    # through the C entry: mmse_mode outside 0 / 1, no output, the other precision -- and nothing is written
    dl = np.ascontiguousarray(np.asarray(fd[0], dtype=np.int32))
    pw = np.ascontiguousarray(np.asarray(fd[1], dtype=np.float64))
    snr, seeds = np.array(ec.POINTS, dtype=np.float64), np.array(ec.seeds("A"), dtype=np.uint64)
    err = np.full((3, 4), 77, dtype=np.uint64)
    ptr = lambda a: C.c_void_p(a.ctypes.data)                                        # noqa: E731

    def call(mode, errors, flags):
        return L.load().ofdm_estimator_study(plan.handle, None, 0, ptr(dl), ptr(pw), dl.size, ptr(snr), ptr(seeds), 3, 5, 0, mode, 0,
                                             errors, None, None, None, None, flags)
    for mode, errors, flags, msg in ((2, ptr(err), L.OFDM_F64 | L.OFDM_HOST, "mmse_mode must be 0"),
                                     (0, None, L.OFDM_F64 | L.OFDM_HOST, "estimator_study: no output is given"),
                                     (0, ptr(err), L.OFDM_F32 | L.OFDM_HOST, "precision flag differs from the plan's")):
        with pytest.raises(ofdm.OfdmError, match=msg):
            L.check(call(mode, errors, flags), "estimator_study")
        assert np.all(err == 77)
    plan.close()

    # what the part-2 tile refuses of a plan, in its words: K < Np for MP_estimate
    pc, dc, pv = ec.layout(oracle, case)
    small = ofdm.RxPlan(case.nfft, case.t_guard, tc.N_SYMB, case.n_carrier, pc, dc, pv[:, 0], 16, 3, tc.CONSTELLATION, precision="fp64")
    with pytest.raises(ofdm.OfdmError, match="MP_estimate: the loop bound is Np columns"):
        small.estimator_study(ec.POINTS, 5, fading=([0, 3, 7], [1.0, 0.36, 0.09]))
    small.close()
    b = tc.BOUND_REFUSED
    lay = ec.layout(oracle, b)
    many = ofdm.RxPlan(b.nfft, b.t_guard, tc.N_SYMB, b.n_carrier, lay[0], lay[1], lay[2][:, 0], b.K, b.paths, tc.CONSTELLATION,
                       precision="fp32")
    with pytest.raises(ofdm.OfdmError, match="task5_part2_tile: MMSE stage supports at most 585 pilots"):
        many.estimator_study(ec.POINTS, 5, fading=ec.fading(b))
    many.close()


def tc_register():
    from ofdm_course_amd.drivers import common
    return common.REGISTER
