"""ofdm_estimator_profile (csrc/ofdm_est_profile.hip, RxPlan.estimator_profile): the estimator study's outputs bit for bit, the
per-carrier sums of the four estimates, the histogram of the frames' error and the per-delay tables of OMP_estimate's picks -- against
estimator_study for the same arguments, across chunkings and a split by frame0, through the identities between the outputs, per
frame against the oracle's LS_CE, MMSE_CE, MP_estimate and OMP_estimate on the frames tx_frames_fused returns for the same
arguments, and its refusals.

Shape A: Nfft 256, T_guard 32, N_carrier 100 (no multiple of 64), comb 4 -> 25 pilots, K = 25, QPSK, N_symb 2, dominant_taps 3, a
3-tap channel, static and drawn per frame; 3 points x 5 frames.  Shape B: Nfft 512, T_guard 64, N_carrier 200, comb 8 -> 25 pilots,
K = 25, a 4-tap line whose last delay 30 is outside the dictionary, dominant_taps 4.

The pick count.  The relative-change stop of OMP_estimate.m:20 ends a frame early when the atom just added moves the residual by
less than 1 % of its norm, that is, explains less than 1e-4 of its energy.  MP_estimate needs K >= Np, so the dictionary has at
least as many columns as the residual has entries (25 x 25 here, of full rank): the best of them always explains about 1 / Np = 4 %
of a noise-like residual, far above the stop's 1e-4, and the oracle makes all 4 picks on 15 of the 15 frames of shape B.  By the
same argument raising dominant_taps does not produce a frame with fewer picks before the residual is exhausted at Np picks, where
the next pick is an arg-max over rounding noise and no longer comparable between two implementations.  So
n_picks_hist is asserted equal to the oracle's pick counts frame by frame and through its identities, and no second non-empty bin
is demanded of shape B.  Said plainly: on every plan the entry accepts, bins 0 .. dominant_taps - 1 of n_picks_hist are zero, and no
test here runs est_delay_kernel on a slot that was not made (tap_idx = -1: the slot skipped by the owner of every delay, picks = 0
through idx + 1, made < dominant_taps); that path is covered by reading the kernel only.

The split by frame0.  The per-carrier sums keep no per-frame rows, so a 2 + 3 split cannot be re-summed on the host; what two
calls can be held to exactly is the one-frame split (0 + v_0) + v_1 = sums(frame 0) + sums(frame 1), and the order inside one call
is covered by max_frames_per_chunk in {0, 1, 2}."""
import numpy as np
import pytest

from oracle_lib import OracleLib
from pick_audit import omp_pick_audit

pytestmark = pytest.mark.gpu

ROWS = ("LS", "MMSE", "MP", "OMP")
POINTS = (5.0, 15.0, 30.0)
SEEDS = (101, 202, 303)
FRAMES = 5
N_SYMB = 2
CONSTELLATION = "QPSK"
SHAPES = {"A": dict(nfft=256, t_guard=32, n_carrier=100, comb=4, K=25, T=3, fading=([0, 3, 7], [1.0, 0.36, 0.09])),
          "B": dict(nfft=512, t_guard=64, n_carrier=200, comb=8, K=25, T=4, fading=([0, 4, 9, 30], [1.0, 0.5, 0.25, 0.2]))}
STATIC_TAPS = ((0, 1.0), (2, -0.5 + 0.3j), (5, 0.25j))
# the tolerance of frame_nmse (and so of nmse_sums) against the oracle in tests/test_gpu_estimator_study.py:15, used at :117
FP64_TOL = dict(rtol=1e-9, atol=1e-12)

STUDY_KEYS = ("errors", "nmse_sums", "nmse_dropped", "frame_errors", "frame_nmse")
INT_TABLES = ("errors", "nmse_dropped", "nmse_hist", "nmse_below", "nmse_above", "nmse_nan", "pick_hist", "n_picks_hist", "true_outside",
              "support_hits", "support_misses", "support_false")
SUMS = ("nmse_sums", "true_amp_sums", "est_amp_sums", "err_sums", "amp_err_sums", "tap_amp_sums", "true_tap_amp_sums")
FRAME_ROWS = ("frame_errors", "frame_nmse", "picks", "tap_x")
DERIVED = ("BER", "NMSE", "mean_true_amp", "mean_est_amp", "nmse_profile", "edges", "thresholds")


def _layout(oracle, s):
    from ofdm_course_amd.drivers import common as c
    _, pc, dc = c.layout_comb(s["nfft"], s["n_carrier"], s["comb"])
    d, _ = OracleLib(oracle).constellation_func(CONSTELLATION)
    return pc, dc, c.alternating_pilots(2 * np.max(np.abs(d)), len(pc), N_SYMB)


def _static_h(precision):
    h = np.zeros(6, dtype=np.complex128)
    for d, a in STATIC_TAPS:
        h[d] = a
    return h.astype(np.complex128 if precision == "fp64" else np.complex64)


def _chan(shape, channel, precision):
    return dict(h=_static_h(precision)) if channel == "static" else dict(fading=SHAPES[shape]["fading"])


@pytest.fixture(scope="module")
def plans(ofdm, oracle):
    cache = {}

    def get(shape, precision):
        if (shape, precision) not in cache:
            s = SHAPES[shape]
            pc, dc, pv = _layout(oracle, s)
            cache[(shape, precision)] = ofdm.RxPlan(s["nfft"], s["t_guard"], N_SYMB, s["n_carrier"], pc, dc, pv[:, 0], s["K"], s["T"],
                                                    CONSTELLATION, precision=precision)
        return cache[(shape, precision)]
    yield get
    for p in cache.values():
        p.close()


@pytest.fixture(scope="module")
def profiles(plans):
    """RxPlan.estimator_profile(POINTS, FRAMES, want_frames=True) once per (shape, precision, channel, mmse); left unchanged."""
    cache = {}

    def get(shape, precision, channel, mmse):
        key = (shape, precision, channel, mmse)
        if key not in cache:
            cache[key] = plans(shape, precision).estimator_profile(POINTS, FRAMES, mmse=mmse, seeds=SEEDS, want_frames=True,
                                                                   **_chan(shape, channel, precision))
        return cache[key]
    return get


def _abs(z):
    """|z| as the kernels form it: two rounded products, a rounded sum, a root (numpy's abs is hypot)."""
    z = np.asarray(z, dtype=np.complex128)
    return np.sqrt(z.real * z.real + z.imag * z.imag)


def _in_order(rows):
    """((0 + v_0) + v_1) + .. along axis 0."""
    s = np.zeros(np.asarray(rows).shape[1:])
    for v in rows:
        s = s + v
    return s


def _bytes_equal(a, b, keys):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), k


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("mmse", ["ls", "genie"])
@pytest.mark.parametrize("channel", ["fading", "static"])
def test_the_studys_outputs_bit_for_bit(plans, profiles, precision, mmse, channel):
    plan = plans("A", precision)
    got = profiles("A", precision, channel, mmse)
    want = plan.estimator_study(POINTS, FRAMES, mmse=mmse, seeds=SEEDS, want_frames=True, **_chan("A", channel, precision))
    _bytes_equal(got, want, STUDY_KEYS + ("BER", "NMSE"))
    assert got["rows"] == want["rows"] == ROWS and got["bits"] == want["bits"]
    lean, lean_want = (f(POINTS, FRAMES, mmse=mmse, seeds=SEEDS, **_chan("A", channel, precision))
                       for f in (plan.estimator_profile, plan.estimator_study))
    _bytes_equal(lean, lean_want, ("errors", "nmse_sums", "nmse_dropped"))
    assert "picks" not in lean and "frame_nmse" not in lean
    _bytes_equal(lean, got, INT_TABLES + SUMS)


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("shape,channel,mmse", [("A", "fading", "ls"), ("A", "static", "genie"), ("B", "fading", "ls")])
def test_no_output_depends_on_the_chunking_or_on_a_split_by_frame0(plans, profiles, precision, shape, channel, mmse):
    plan, full = plans(shape, precision), profiles(shape, precision, channel, mmse)
    kw = dict(mmse=mmse, seeds=SEEDS, want_frames=True, **_chan(shape, channel, precision))
    for cap in (0, 1, 2):
        _bytes_equal(plan.estimator_profile(POINTS, FRAMES, max_frames_per_chunk=cap, **kw), full,
                     INT_TABLES + SUMS + FRAME_ROWS + DERIVED)
    a = plan.estimator_profile(POINTS, 2, **kw)
    b = plan.estimator_profile(POINTS, FRAMES - 2, frame0=2, **kw)
    for k in INT_TABLES:
        assert np.array_equal(np.asarray(a[k]) + np.asarray(b[k]), np.asarray(full[k])), k
    for k in FRAME_ROWS:
        assert np.concatenate([np.asarray(a[k]), np.asarray(b[k])], axis=1).tobytes() == np.asarray(full[k]).tobytes(), k
    # the double sums: re-summed in frame order from the per-frame rows of the two parts
    fn = np.concatenate([np.asarray(a["frame_nmse"]), np.asarray(b["frame_nmse"])], axis=1)
    picks = np.concatenate([np.asarray(a["picks"]), np.asarray(b["picks"])], axis=1)
    tx = np.concatenate([np.asarray(a["tap_x"]), np.asarray(b["tap_x"])], axis=1)
    for p in range(len(POINTS)):
        for e in range(4):
            s = 0.0
            for v in fn[p, :, e]:
                s = s + v if np.isfinite(v) else s
            assert s == np.asarray(full["nmse_sums"])[p, e]
        assert _tap_sums(picks[p], tx[p], SHAPES[shape]["K"])[1].tobytes() == np.asarray(full["tap_amp_sums"])[p].tobytes()
    # the per-carrier sums have no per-frame rows to re-sum; what a split can be compared with exactly is the one-frame split,
    # (0 + v_0) + v_1 = sums(frame 0) + sums(frame 1)
    one = [plan.estimator_profile(POINTS, 1, frame0=f, **kw) for f in (0, 1)]
    two = plan.estimator_profile(POINTS, 2, **kw)
    for k in ("true_amp_sums", "est_amp_sums", "err_sums", "amp_err_sums", "true_tap_amp_sums"):
        assert (np.asarray(one[0][k]) + np.asarray(one[1][k])).tobytes() == np.asarray(two[k]).tobytes(), k
    # the device flavour: the same bits, tensors on the device
    dev = plan.estimator_profile(POINTS, FRAMES, device="cuda:0", **kw)
    assert dev["err_sums"].is_cuda and dev["pick_hist"].is_cuda and dev["nmse_profile"].is_cuda
    _bytes_equal({k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in dev.items()}, full,
                 INT_TABLES + SUMS + ("frame_nmse", "picks", "tap_x", "mean_true_amp", "mean_est_amp", "nmse_profile"))


def _tap_sums(picks, tap_x, K):
    """pick_hist and tap_amp_sums of one point from its frames' slots, in frame order and slot order."""
    hist, amp = np.zeros(K, dtype=np.int64), np.zeros(K)
    for f in range(picks.shape[0]):
        for q in range(picks.shape[1]):
            if picks[f, q] > 0:
                hist[picks[f, q] - 1] += 1
                amp[picks[f, q] - 1] = amp[picks[f, q] - 1] + _abs(tap_x[f, q])
    return hist, amp


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("shape,channel", [("A", "fading"), ("A", "static"), ("B", "fading")])
def test_identities_between_the_outputs(profiles, precision, shape, channel):
    s, out = SHAPES[shape], profiles(shape, precision, channel, "ls")
    nc, K, T = s["n_carrier"], s["K"], s["T"]
    g = {k: np.asarray(v) for k, v in out.items() if k != "rows"}
    assert g["true_amp_sums"].shape == (3, nc) and g["err_sums"].shape == (3, 4, nc) and g["nmse_hist"].shape == (3, 4, 60)
    assert g["pick_hist"].shape == g["tap_amp_sums"].shape == (3, K) and g["n_picks_hist"].shape == (3, T + 1)
    assert g["picks"].shape == g["tap_x"].shape == (3, FRAMES, T) and g["picks"].dtype == np.int32 and g["tap_x"].dtype == np.complex128
    assert np.array_equal(g["nmse_hist"].sum(axis=2) + g["nmse_below"] + g["nmse_above"] + g["nmse_nan"], np.full((3, 4), FRAMES))
    assert np.array_equal(g["nmse_nan"], g["nmse_dropped"])
    # the histogram is the frames on the thresholds: numpy's search on the same table
    thr = g["thresholds"]
    assert np.allclose(thr, nc * 10.0 ** (g["edges"] / 10.0), rtol=1e-14)
    for p in range(3):
        for e in range(4):
            b = np.searchsorted(thr, g["frame_nmse"][p, :, e], side="right") - 1
            assert np.array_equal(np.bincount(b[(b >= 0) & (b < 60)], minlength=60), g["nmse_hist"][p, e])
    assert np.array_equal(g["pick_hist"].sum(axis=1), (g["n_picks_hist"] * np.arange(T + 1)).sum(axis=1))
    assert np.array_equal(g["n_picks_hist"].sum(axis=1), np.full(3, FRAMES))
    delays = s["fading"][0] if channel == "fading" else [d for d, _ in STATIC_TAPS]
    inside = [d for d in delays if d < K]
    assert np.array_equal(g["support_hits"] + g["support_misses"], np.full(3, FRAMES * len(inside)))
    assert np.array_equal(g["true_outside"], np.full(3, FRAMES * (len(delays) - len(inside))))
    distinct = np.array([sum(len(set(int(k) for k in g["picks"][p, f] if k > 0)) for f in range(FRAMES)) for p in range(3)])
    assert np.array_equal(g["support_hits"] + g["support_false"], distinct)
    hits = np.array([sum(len(set(int(k) - 1 for k in g["picks"][p, f] if k > 0) & set(inside)) for f in range(FRAMES))
                     for p in range(3)])
    assert np.array_equal(g["support_hits"], hits)
    # re-ordering frames_per_point * nc non-negative doubles: a relative frames_per_point * nc * 2^-52
    assert np.allclose(g["err_sums"].sum(axis=2), g["nmse_sums"], rtol=FRAMES * nc * 2.0 ** -52, atol=0)
    for p in range(3):
        hist, amp = _tap_sums(g["picks"][p], g["tap_x"][p], K)
        assert np.array_equal(hist, g["pick_hist"][p]) and amp.tobytes() == g["tap_amp_sums"][p].tobytes()
        made = (g["picks"][p] > 0).sum(axis=1)
        assert np.array_equal(np.bincount(made, minlength=T + 1), g["n_picks_hist"][p])
    assert np.array_equal(g["mean_true_amp"], g["true_amp_sums"] / float(FRAMES))
    assert np.array_equal(g["nmse_profile"], g["err_sums"] / (FRAMES - g["nmse_dropped"]).astype(np.float64)[..., None])
    assert np.array_equal(g["mean_est_amp"], g["est_amp_sums"] / (FRAMES - g["nmse_dropped"]).astype(np.float64)[..., None])
    if shape == "B":                                                  # the tap at delay 30 is outside the dictionary of 25 columns
        assert np.all(g["true_outside"] == FRAMES) and np.all(g["support_misses"] >= 0)
        assert np.all(g["true_tap_amp_sums"][:, [1, 2, 3, 5, 6, 7, 8] + list(range(10, K))] == 0)


@pytest.fixture(scope="module")
def replays(oracle, plans):
    """The oracle's four estimates of the generator's own frames (fp64), once per (shape, channel, mmse): per point and frame the
    true H, the four H on carriers 1..N_carrier, OMP's picks and the pilot LS values Y."""
    cache = {}

    def get(shape, channel, mmse):
        key = (shape, channel, mmse)
        if key in cache:
            return cache[key]
        s, plan, lib = SHAPES[shape], plans(shape, "fp64"), OracleLib(oracle)
        pc, dc, pv = _layout(oracle, s)
        S = lib.sensing_matrix(pc, s["nfft"], s["K"])
        nc = s["n_carrier"]
        Ht, He, picks, Ys = (np.zeros((3, FRAMES, nc), complex), np.zeros((3, FRAMES, 4, nc), complex),
                             np.zeros((3, FRAMES, s["T"]), np.int32), np.zeros((3, FRAMES, len(pc)), complex))
        all_taps = []
        for p, (snr, seed) in enumerate(zip(POINTS, SEEDS)):
            g = plan.tx_frames_fused(FRAMES, SNR=snr, seed=seed, frame0=0, want_taps=channel == "fading", **_chan(shape, channel, "fp64"))
            if channel == "fading":
                delays, amps = s["fading"][0], np.asarray(g["taps"])
            else:
                delays = [d for d, _ in STATIC_TAPS]
                amps = np.tile(np.array([a for _, a in STATIC_TAPS], dtype=np.complex128), (FRAMES, 1))
            all_taps.append(amps)
            rx = np.asarray(g["rx"]).astype(np.complex128)
            for f in range(FRAMES):
                taps = np.stack([np.asarray(delays).astype(complex), amps[f]], axis=1)
                h_t, H_f = lib.get_MP_channel_resp(taps, s["nfft"])
                Xr = lib.OFDM_demodulator(rx[:, f].reshape((s["nfft"] + s["t_guard"], N_SYMB), order="F"), s["t_guard"])
                H_LS = lib.LS_CE(Xr, pv, pc, nc)
                if mmse == "genie":
                    h = np.zeros(nc, dtype=np.complex128)
                    h[:min(len(h_t), nc)] = np.asarray(h_t)[:nc]
                else:
                    h = np.asarray(lib.OFDM_modulator(np.asarray(H_LS).ravel().reshape(-1, 1), 0)).ravel()
                Y = np.asarray(lib.get_payload(np.asarray(Xr)[:, :1], pc)).ravel() / pv[:, 0]
                omp = oracle.OMP_estimate(Y, S, s["nfft"], s["T"], float(snr))
                H = [H_LS, lib.MMSE_CE(Xr, pv, pc, s["nfft"], nc, h, float(snr)), lib.MP_estimate(Y, S, s["nfft"], s["T"])[0], omp[0]]
                Ht[p, f] = np.asarray(H_f).ravel()[:nc]
                for e in range(4):
                    He[p, f, e] = np.asarray(H[e]).ravel()[:nc]
                idx = np.asarray(omp[2]).ravel().astype(np.int32)
                picks[p, f, :len(idx)] = idx
                Ys[p, f] = Y
        cache[key] = dict(H=Ht, He=He, picks=picks, Y=Ys, S=S, taps=all_taps)
        return cache[key]
    return get


def _carrier_sums(Ht, He):
    """true_amp_sums [P, nc], est_amp_sums, err_sums, amp_err_sums [P, 4, nc] of H [P, F, nc] and H_e [P, F, 4, nc] in frame order."""
    ta, ea = _abs(Ht), _abs(He)
    d = Ht[:, :, None, :] - He
    err = d.real * d.real + d.imag * d.imag
    aerr = (ea - ta[:, :, None, :]) ** 2
    sw = lambda a: _in_order(np.swapaxes(a, 0, 1))                                   # noqa: E731
    return dict(true_amp_sums=sw(ta), est_amp_sums=sw(ea), err_sums=sw(err), amp_err_sums=sw(aerr))


@pytest.mark.parametrize("shape,channel,mmse", [("A", "fading", "ls"), ("A", "fading", "genie"), ("A", "static", "ls"),
                                                ("A", "static", "genie"), ("B", "fading", "ls")])
def test_per_carrier_sums_and_picks_equal_the_oracle_fp64(profiles, replays, shape, channel, mmse):
    """The per-carrier sums against numpy's frame-order sums of the oracle's four estimates, to the tolerance frame_nmse is held to
    against the oracle (tests/test_gpu_estimator_study.py:15,:117: rtol 1e-9, atol 1e-12); OMP's picks identical, and
    n_picks_hist the oracle's pick counts (the module's docstring: every frame makes all its picks)."""
    got, want = profiles(shape, "fp64", channel, mmse), replays(shape, channel, mmse)
    assert np.array_equal(np.asarray(got["picks"]), want["picks"])
    sums = _carrier_sums(want["H"], want["He"])
    for k, w in sums.items():
        g = np.asarray(got[k])
        print(shape, channel, mmse, k, "largest deviation relative to the largest entry", np.max(np.abs(g - w)) / np.max(np.abs(w)))
        assert np.allclose(g, w, **FP64_TOL), k
    made = (want["picks"] > 0).sum(axis=2)
    T = SHAPES[shape]["T"]
    for p in range(3):
        assert np.array_equal(np.asarray(got["n_picks_hist"])[p], np.bincount(made[p], minlength=T + 1))
    # the truth's delay-domain curve: the frame's own amplitudes at the delays inside the dictionary
    delays = SHAPES[shape]["fading"][0] if channel == "fading" else [d for d, _ in STATIC_TAPS]
    for p in range(3):
        w = np.zeros(SHAPES[shape]["K"])
        for t, d in enumerate(delays):
            if d < SHAPES[shape]["K"]:
                w[d] = _in_order(_abs(want["taps"][p][:, t])[:, None])[0]
        assert np.allclose(np.asarray(got["true_tap_amp_sums"])[p], w, rtol=1e-13, atol=0)


# fp32 against the fp64 run of the same call: the largest deviation of est_amp_sums, err_sums and amp_err_sums, relative to the
# largest entry of the table, measured per case on an MI355X (the method of tests/test_gpu_mmse_ls.py: measure, record, bound at a
# stated multiple).  The bound of every case is FP32_BOUND_FACTOR times the largest figure recorded here.
FP32_MEASURED = {("A", "fading", "ls"): 2.45e-7, ("A", "fading", "genie"): 2.45e-7, ("A", "static", "ls"): 2.85e-7,
                 ("A", "static", "genie"): 2.85e-7, ("B", "fading", "ls"): 2.78e-7}
FP32_BOUND_FACTOR = 8.0
FP32_BOUND = FP32_BOUND_FACTOR * max(FP32_MEASURED.values())


@pytest.mark.parametrize("shape,channel,mmse", [("A", "fading", "ls"), ("A", "fading", "genie"), ("A", "static", "ls"),
                                                ("A", "static", "genie"), ("B", "fading", "ls")])
def test_fp32_against_the_fp64_run_of_the_same_call(oracle, profiles, replays, shape, channel, mmse):
    """Picks under the near-tie rule of tests/pick_audit.py: a frame whose fp32 picks differ from the fp64 run's must pass the audit
    along its own picks, and at most one frame per case may differ.  The per-carrier sums of
    the estimates within FP32_BOUND = 8 x 2.85e-7 of the table's largest entry; measured per case, the largest of the three
    tables: A fading ls 2.45e-7, A fading genie 2.45e-7, A static ls 2.85e-7, A static genie 2.85e-7, B fading ls 2.78e-7; no frame's picks differed.  The
    truth's sums are double in both runs: equal with a channel per frame, whose amplitudes are drawn in double; with a static
    channel h comes in the plan's precision, each tap rounded to float, so they agree to 2^-23 (measured 6.7e-9)."""
    lo, hi, want = profiles(shape, "fp32", channel, mmse), profiles(shape, "fp64", channel, mmse), replays(shape, channel, mmse)
    p32, p64 = np.asarray(lo["picks"]), np.asarray(hi["picks"])
    differ = np.argwhere(np.any(p32 != p64, axis=2))
    for p, f in differ:
        omp_pick_audit(oracle, want["Y"][p, f], want["S"], [k for k in p32[p, f] if k > 0], SHAPES[shape]["nfft"])
    print(shape, channel, mmse, "frames whose fp32 picks differ", differ.tolist())
    assert len(differ) <= 1, differ.tolist()
    devs = {}
    for k in ("true_amp_sums", "est_amp_sums", "err_sums", "amp_err_sums"):
        a, b = np.asarray(lo[k]), np.asarray(hi[k])
        if k != "true_amp_sums" and len(differ):                      # an excused frame's point is compared without that frame's table
            keep = [p for p in range(3) if p not in set(differ[:, 0].tolist())]
            a, b = a[keep], b[keep]
        devs[k] = np.max(np.abs(a - b)) / np.max(np.abs(b))
        print(shape, channel, mmse, k, "fp32 against fp64, largest deviation relative to the largest entry", devs[k])
    assert devs["true_amp_sums"] <= (2.0 ** -23 if channel == "static" else 0.0)
    for k in ("est_amp_sums", "err_sums", "amp_err_sums"):
        assert devs[k] <= FP32_BOUND, (k, devs[k])


def test_frames_dropped_for_one_estimator_leave_the_others_alone(ofdm, oracle, plans):
    """mmse = "genie" with a line whose every delay is >= N_carrier: tau_rms has no energy to measure, every frame's MMSE row is
    dropped -- nmse_dropped = frames, its per-carrier sums stay zero -- and LS, MP and OMP are what they are in the ls mode."""
    s = SHAPES["A"]
    pc, dc, pv = _layout(oracle, s)
    plan = ofdm.RxPlan(s["nfft"], s["t_guard"], N_SYMB, s["n_carrier"], pc, dc, pv[:, 0], s["K"], 2, CONSTELLATION, precision="fp64")
    kw = dict(fading=([100, 104], [1.0, 0.5]), seeds=SEEDS, want_frames=True)
    genie = plan.estimator_profile(POINTS, FRAMES, mmse="genie", **kw)
    ls = plan.estimator_profile(POINTS, FRAMES, mmse="ls", **kw)
    plan.close()
    drop = np.asarray(genie["nmse_dropped"])
    assert np.array_equal(drop[:, 1], np.full(3, FRAMES)) and not drop[:, [0, 2, 3]].any()
    assert np.array_equal(np.asarray(genie["nmse_nan"]), drop) and not np.asarray(genie["nmse_hist"])[:, 1].any()
    for k in ("est_amp_sums", "err_sums", "amp_err_sums"):
        assert not np.asarray(genie[k])[:, 1].any(), k
        assert np.asarray(genie[k])[:, [0, 2, 3]].tobytes() == np.asarray(ls[k])[:, [0, 2, 3]].tobytes(), k
        assert np.all(np.isfinite(np.asarray(ls[k])))
    assert np.all(np.isnan(np.asarray(genie["nmse_profile"])[:, 1])) and np.all(np.isnan(np.asarray(genie["mean_est_amp"])[:, 1]))
    for k in ("true_amp_sums", "pick_hist", "tap_amp_sums", "n_picks_hist", "picks", "tap_x", "true_tap_amp_sums"):
        assert np.asarray(genie[k]).tobytes() == np.asarray(ls[k]).tobytes(), k
    assert np.all(np.asarray(genie["true_outside"]) == 2 * FRAMES) and not np.asarray(genie["true_tap_amp_sums"]).any()
    assert not np.asarray(genie["support_hits"]).any() and not np.asarray(genie["support_misses"]).any()


def test_refusals(ofdm, oracle, plans):
    from ofdm_course_amd.drivers import common
    s = SHAPES["A"]
    pc, dc, pv = _layout(oracle, s)
    plan = ofdm.RxPlan(s["nfft"], s["t_guard"], N_SYMB, s["n_carrier"], pc, dc, pv[:, 0], s["K"], s["T"], CONSTELLATION, precision="fp64")
    fd = s["fading"]
    for bins in (dict(n=0, lo=-50.0, hi=10.0), dict(n=4097, lo=-50.0, hi=10.0), dict(n=60, lo=10.0, hi=10.0),
                 dict(n=60, lo=-50.0, hi=float("inf")), dict(n=60, lo=float("nan"), hi=10.0)):
        with pytest.raises(ofdm.OfdmError, match=r"estimator_profile: bins must have n 1 \.\. 4096 and finite lo < hi \("):
            plan.estimator_profile(POINTS, FRAMES, fading=fd, bins=bins)
    with pytest.raises(ofdm.OfdmError, match="estimator_profile: bins must be dict"):
        plan.estimator_profile(POINTS, FRAMES, fading=fd, bins=dict(n=60))
    with pytest.raises(ofdm.OfdmError, match="estimator_profile: unknown bins keys"):
        plan.estimator_profile(POINTS, FRAMES, fading=fd, bins=dict(n=60, lo=-50.0, hi=10.0, width=1.0))
    with pytest.raises(ofdm.OfdmError, match='estimator_profile: mmse must be "ls" or "genie"'):
        plan.estimator_profile(POINTS, FRAMES, fading=fd, mmse="lmmse")
    plan.set_descrambler(common.REGISTER)
    with pytest.raises(ofdm.OfdmError, match="estimator_profile: the study runs unscrambled"):
        plan.estimator_profile(POINTS, FRAMES, fading=fd)
    plan.set_descrambler(None)
    out = plan.estimator_profile(POINTS, FRAMES, fading=fd, bins=dict(n=1, lo=-60.0, hi=40.0))
    assert np.asarray(out["nmse_hist"]).shape == (3, 4, 1) and np.all(np.asarray(out["nmse_hist"]) == FRAMES)
    plan.close()


def test_task5_estimators_driver_with_and_without_curves(ofdm, tmp_path, monkeypatch):
    """python -m ofdm_course_amd.drivers.task5_estimators at two frames, three SNR points and one pilot count: with --curves the JSON
    gains curves.pictures with the per-carrier, histogram and per-delay tables of the points asked for; everything else, and the
    whole JSON without --curves, is what estimator_study gives (the profile returns its tables bit for bit)."""
    import json
    from ofdm_course_amd.drivers import task5_estimators as te
    monkeypatch.setattr(te, "CURVE_SNRS", (0.0, 10.0, 30.0))
    base = ["--profile", "EPA", "--frames", "2", "--counts", "16", "--precision", "fp64"]
    plain, curves = tmp_path / "plain.json", tmp_path / "curves.json"
    te.main(base + ["--json", str(plain)])
    te.main(base + ["--json", str(curves), "--curves", "--curve-snrs", "0,30"])
    a, b = json.loads(plain.read_text()), json.loads(curves.read_text())
    assert "pictures" not in a["curves"] and set(a["curves"]) == {"SNR_dB", "comb", "n_pilots", "BER", "NMSE", "nmse_dropped"}
    pic = b["curves"].pop("pictures")
    assert a == b
    nc, K, T = te.N_CARRIER, pic["K"], pic["dominant_taps"]
    assert pic["SNR_dB"] == [0.0, 30.0] and (K, T) == (256, 6)
    for k, shape in (("mean_true_amp", (2, nc)), ("mean_est_amp", (2, 4, nc)), ("nmse_profile", (2, 4, nc)), ("nmse_hist", (2, 4, 60)),
                     ("pick_hist", (2, K)), ("mean_tap_amp", (2, K)), ("mean_true_tap_amp", (2, K)), ("n_picks_hist", (2, T + 1)),
                     ("support_hits", (2,)), ("support_misses", (2,)), ("support_false", (2,)), ("true_outside", (2,))):
        assert np.asarray(pic[k]).shape == shape, k
    hist = np.asarray(pic["nmse_hist"]).sum(axis=2) + np.asarray(pic["nmse_below"]) + np.asarray(pic["nmse_above"]) + np.asarray(pic["nmse_nan"])
    assert np.array_equal(hist, np.full((2, 4), 2)) and np.array_equal(np.asarray(pic["n_picks_hist"]).sum(axis=1), [2, 2])
    # the mean of the profile over the carriers is the curve's NMSE at that point
    at = [0, 2]
    assert np.allclose(np.asarray(pic["nmse_profile"]).mean(axis=2), np.asarray(b["curves"]["NMSE"])[at], rtol=1e-12)
