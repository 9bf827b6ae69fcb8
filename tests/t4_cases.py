"""Fixed table of small Task-4 receiver cases, their frames and their oracle replay.  TEST INFRASTRUCTURE: a helper module (no
tests here), imported by test_t4_cases_host.py, test_gpu_sync_sizes.py and test_gpu_task4_sizes.py.  Everything in this file
uses the oracle only -- no call into the product.

Case = (name, Nfft, T_guard, N_carrier, N_symb, const, n_frames, seed, pilot percent, late, noise_seed):

  name         Nfft  T_guard  N_carrier  N_symb  const  frames  pilots %  what it reaches
  n64            64        8         48      12  QPSK     9 + 1       15  staged form natively; fallback position 65 < one symbol
  n64late        64        8         48      18  QPSK     4 + 1       15  n64 with a stream that reaches past 1024 (see "late" below)
  n256          256       32        100       8  16QAM    9 + 1       15  staged form natively
  n512odd       512       64        201       6  16QAM    9 + 1       15  NW = 1, scalar equaliser path
  n1024tg100   1024      100        400       6  16QAM    6           15  guard not Nfft / 8, NW = 2
  n2048odd     2048      256        801       5  64QAM    5           15  fp32 falls off the wave path with no switch
  n2048tg255   2048      255        800       5  64QAM    5           15  wave path with an odd guard
  n4096        4096      512       1024       5  64QAM    5           15  NW = 8; fewer than T4_FT = 8 frames
  n8192        8192     1024       1600       5  64QAM    4           15  staged natively; W = ACF_MAXW; LDS above 64 KB

n4096 and n8192 carry 5 symbols, not 4 and 3: estimate_channel.m:6 averages the blanked first symbol (T4:292-294) into the pilot
means, so H is (S - 1) / S too small and the equalised points S / (S - 1) too large -- with 64-QAM and S = 4 the reference's own
BER lies at 0.216 .. 0.221 for every draw (0.125 from the blanked symbol alone), above its 0.2 gate (T4:367); S = 5 passes as the
two 2048-point rows do.

The seeds (231, 6, 1, 1, 3, 1, 1, 11, 26) are the first ones under which test_t4_cases_host.py passes.
Every layout pilot_layout_percent(Nfft, N_carrier, 15, 2) has at least 9 pilots, so no percentage had to be raised.

Frames (build_frames): mapping -> OFDM_map_carriers -> OFDM_modulator -> Noise(30 dB) -> add_STO(random 0..Nfft+Tg) ->
add_CFO(random integer 0..30 + a fraction in +-0.5) -> apply_channel (3 taps, longest delay below T_guard / 2), complex128.
Frame `n_frames - 2` is multiplied by 1e-3: no spectral line reaches 0.77, remove_IFO's index error (status -1).

Extra frames, appended after the n_frames of the table ("+ 1" above):
  * noise (n64: noise_seed is not None): one frame of pure unit-variance noise -> the catch branch of AutoCorrFunction.m:21-24,
    TgPosition 65, ok false.
  * late (n64late, n256, n512odd): one frame delayed by add_STO(., -1023) instead of being advanced, i.e. 1023 zeros in front
    (rho is NaN there = "not above"), so that its first guard-interval plateau sits on index 1024: the search kernel finds the
    start of the first run in one 1024-tile and its end in the next.  A frame made by the chain above always has its first
    plateau inside the first T_guard + Nfft + T_guard samples, so at Nfft <= 512 no draw of it can ever reach a tile border;
    n64's stream (864 samples) does not even contain index 1024, hence the longer twin n64late.

  * early (n8192, frame 0 -- not an extra frame): STO = Nfft + T_guard - 256, so the first guard-interval plateau lies wholly below
    index W = 1024, where AutoCorrFunction.m:13 does not look: a search that started at 0 instead of W would lock onto it.
    TgPosition is then the second symbol's plateau and the frame decodes one symbol off, so n8192 has a fourth frame to keep two
    decodable ones.

replay(): the function-by-function chain of T4/Main_model_Task_4.m:278-347 on the oracle, per frame, with two firmness margins
taken from the oracle's own curves (how far the two 0.77 decisions of the reference are from flipping):
  m_acf = min | |rho_i| - 0.77 | over 0-based i from W to the start of the second run (to the end when the search fails)
  m_ifo = min | |spec_k| - 0.77 | / max|spec| over the bins up to and including the first one above 0.77 (all bins when none is)
A frame is firm when m_acf >= 1e-4 (the fp32 bound on rho stated at acf4 in sync_core.hpp) and m_ifo >= 1e-5 (about ten times
the suite's fp32 FFT bound per bin)."""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name Nfft T_guard N_carrier N_symb const n_frames seed pct late noise_seed")

CASES = [
    Case("n64", 64, 8, 48, 12, "QPSK", 9, 231, 15, False, 1),
    Case("n64late", 64, 8, 48, 18, "QPSK", 4, 6, 15, True, None),
    Case("n256", 256, 32, 100, 8, "16QAM", 9, 1, 15, True, None),
    Case("n512odd", 512, 64, 201, 6, "16QAM", 9, 1, 15, True, None),
    Case("n1024tg100", 1024, 100, 400, 6, "16QAM", 6, 3, 15, False, None),
    Case("n2048odd", 2048, 256, 801, 5, "64QAM", 5, 1, 15, False, None),
    Case("n2048tg255", 2048, 255, 800, 5, "64QAM", 5, 1, 15, False, None),
    Case("n4096", 4096, 512, 1024, 5, "64QAM", 5, 11, 15, False, None),
    Case("n8192", 8192, 1024, 1600, 5, "64QAM", 4, 26, 15, False, None),
]
BY_NAME = {c.name: c for c in CASES}

ALL_FLAGS = [(1, 1, 1), (1, 0, 1), (0, 1, 0), (0, 0, 1), (0, 0, 0)]          # test_batch_equals_per_function_chain's
TWO_FLAGS = [(1, 1, 1), (0, 0, 1)]
FIVE_FLAG_CASES = ("n64", "n512odd", "n4096", "n8192")

THR = 0.77
M_ACF, M_IFO = 1e-4, 1e-5
EARLY = {"n8192": 256}          # frame 0 of these cases: STO = Nfft + T_guard - this, its first plateau lies below index W
LATE = 1023                     # zeros in front of the late frame: its first plateau sits on 1-based index 1024


def flag_sets(case):
    return ALL_FLAGS if case.name in FIVE_FLAG_CASES else TWO_FLAGS


def total_frames(case):
    return case.n_frames + (1 if case.late else 0) + (1 if case.noise_seed is not None else 0)


def weak_frame(case):
    return case.n_frames - 2


def layout(oracle, case):
    """pilotCarriers, dataCarriers, allCarriers (1-based), the pilot column (+-4/3 max|dict| alternating) and its [np x N_symb]
    matrix (T4/Main_model_Task_4.m:14-31)."""
    pc, dc = oracle.pilot_layout_percent(case.Nfft, case.N_carrier, case.pct, 2)
    assert len(pc) >= 4, (case.name, len(pc))
    allc = np.arange(1, case.N_carrier + 1, dtype=np.float64)
    D, bps = oracle.constellation_func(case.const)
    amp = 4 / 3 * float(np.max(np.abs(D)))
    col = np.where(np.arange(len(pc)) % 2 == 0, amp, -amp).astype(np.complex128)
    return dict(pc=pc, dc=dc, allc=allc, col=col, pv=np.repeat(col[:, None], case.N_symb, axis=1), bps=bps)


def channel_taps(case):
    """Three taps (1, 0.6, 0.3), the longest delay below T_guard / 2: the [0, 4, 10] of the existing Task-4 tests, scaled with Nfft
    below 1024 -- T4/fine_sync.m:33 keeps a pilot pair only where the slope of the channel's phase changes by less than 1e-3
    per pair, and a ten-sample echo on a 256-point symbol leaves fewer kept pairs than pilots: tau = mean([]) = NaN in every frame."""
    d2 = min(10, max(2, int(round(10 * case.Nfft / 1024))), (case.T_guard + 1) // 2 - 1)
    d1 = max(1, int(round(0.4 * d2)))
    assert 0 < d1 < d2 < case.T_guard / 2
    return np.array([[0, 1.0], [d1, 0.6], [d2, 0.3]])


_FRAMES = {}


def build_frames(oracle, case):
    """dict(rx = [(Nfft + Tg) * N_symb, total_frames] complex128, bits = [total_frames, frame bits] uint8 (zeros for a noise frame),
    sto, cfo, noise = indices of pure-noise frames, late = index of the late frame or None, tx0 = the clean TX stream of frame 0)
    + layout()."""
    if case.name in _FRAMES:
        return _FRAMES[case.name]
    N, Tg, S = case.Nfft, case.T_guard, case.N_symb
    lay = layout(oracle, case)
    h, _ = oracle.get_MP_channel_resp(channel_taps(case), N)
    rng = np.random.default_rng([case.seed, N, Tg, case.N_carrier])
    L = (N + Tg) * S
    nb = S * len(lay["dc"]) * lay["bps"]
    nfr = total_frames(case)
    rx = np.zeros((L, nfr), dtype=np.complex128)
    bits_all = np.zeros((nfr, nb), dtype=np.uint8)
    sto, cfo = [], []
    n_sig = case.n_frames + (1 if case.late else 0)
    for f in range(n_sig):
        bits = rng.integers(0, 2, nb).astype(np.uint8)
        iq, _ = oracle.mapping(bits, case.const)
        X = oracle.OFDM_map_carriers(iq, S, N, lay["dc"], lay["pc"], lay["pv"])
        tx = oracle.OFDM_modulator(X, Tg).ravel(order="F")
        if f == 0:
            tx0 = tx
        y, _ = oracle.Noise(30.0, tx, rng=rng)
        s_ = int(rng.integers(0, N + Tg + 1))
        c_ = float(rng.integers(0, 31)) + (rng.random() - 0.5)
        if case.late and f == n_sig - 1:
            s_ = -LATE
        if f == 0 and case.name in EARLY:
            s_ = N + Tg - EARLY[case.name]
        y = oracle.add_CFO(oracle.add_STO(y, s_), c_, N)
        y = oracle.apply_channel(y, h)
        if f == weak_frame(case):
            y = y * 1e-3
        rx[:, f] = y
        bits_all[f] = bits
        sto.append(s_); cfo.append(c_)
    noise = []
    if case.noise_seed is not None:
        r2 = np.random.default_rng([case.noise_seed, 77])
        rx[:, nfr - 1] = (r2.standard_normal(L) + 1j * r2.standard_normal(L)) / np.sqrt(2)
        noise.append(nfr - 1)
    out = dict(lay, rx=rx, bits=bits_all, sto=sto, cfo=cfo, noise=noise, late=(n_sig - 1) if case.late else None, h=h, tx0=tx0)
    _FRAMES[case.name] = out
    return out


def search_runs(amp, W):
    """AutoCorrFunction.m:10-20 as the three indices of the kernels' search (0-based, -1 = not found): f = first i >= W above the
    threshold, g = first i > f not above it (the first run is [f, g - 1]), h = first i > g above it (a second run exists)."""
    with np.errstate(invalid="ignore"):
        above = np.asarray(amp) > THR                     # NaN counts as "not above"
    def first(lo, want):
        idx = np.flatnonzero(above[lo:] == want)
        return int(lo + idx[0]) if idx.size else -1
    f = first(W, True)
    g = first(f + 1, False) if f >= 0 else -1
    h = first(g + 1, True) if g >= 0 else -1
    return f, g, h


_ACF = {}


def acf_of(oracle, case, frames):
    """Per frame (rho, TgPosition, FreqOffset, ok, (f, g, h), m_acf): computed once per case, whatever the flags."""
    if case.name in _ACF:
        return _ACF[case.name]
    import warnings
    res = []
    for fr in range(frames["rx"].shape[1]):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            rho, pos, fo, ok = oracle.AutoCorrFunction(frames["rx"][:, fr], case.T_guard, case.Nfft)
        amp = np.abs(rho)
        f, g, h = search_runs(amp, case.T_guard)
        assert ok == (h >= 0) and (not ok or pos == ((f + 1) + g) // 2), (case.name, fr, pos, f, g, h)
        upto = h if h >= 0 else amp.size - 1
        m_acf = float(np.nanmin(np.abs(amp[case.T_guard: upto + 1] - THR)))
        res.append(dict(rho=rho, pos=int(pos), fo=float(fo), ok=bool(ok), runs=(f, g, h), m_acf=m_acf))
    _ACF[case.name] = res
    return res


_REPLAY = {}


def replay(oracle, case, frames, flags):
    """T4/Main_model_Task_4.m:278-347 frame by frame.  Per frame a dict: TgPosition, FreqOffset, ok (0 / 0.0 / True when neither
    sync flag is set), IFO (an int, or "index error": remove_IFO.m:8 -- H, iq and bits are None then), H(1..N_carrier) (None
    without mp_desync), X0 (the demodulator's output), iq (equalised payload), bits, m_acf, m_ifo, firm."""
    key = (case.name, tuple(flags))
    if key in _REPLAY:
        return _REPLAY[key]
    td, fd, mp = flags
    N, Tg, S, nc = case.Nfft, case.T_guard, case.N_symb, case.N_carrier
    acf = acf_of(oracle, case, frames) if (td or fd) else None
    out = []
    for fr in range(frames["rx"].shape[1]):
        y = frames["rx"][:, fr]
        r = dict(TgPosition=0, FreqOffset=0.0, ok=True, IFO=0, H=None, iq=None, bits=None, m_acf=np.inf, m_ifo=np.inf)
        if td or fd:
            a = acf[fr]
            r.update(TgPosition=a["pos"], FreqOffset=a["fo"], ok=a["ok"], m_acf=a["m_acf"])
            if td:
                y = oracle.add_STO(oracle.add_STO(y, a["pos"]), -(N + Tg))                  # T4:292-294
        if fd:
            y = oracle.add_CFO(y, -r["FreqOffset"], N)                                      # T4:301
            spec = np.abs(np.fft.fft(y[N: 2 * N]))                                          # remove_IFO.m:5
            top = float(np.max(spec))
            with np.errstate(invalid="ignore"):
                ab = np.flatnonzero(spec > THR)
            upto = int(ab[0]) if ab.size else N - 1
            r["m_ifo"] = float(np.min(np.abs(spec[: upto + 1] - THR)) / top) if top > 0 and np.isfinite(top) else 0.0
            try:
                y, ifo = oracle.remove_IFO(y, N)                                            # T4:303
                r["IFO"] = int(ifo)
            except IndexError:
                r["IFO"] = "index error"
        r["firm"] = bool(r["m_acf"] >= M_ACF and r["m_ifo"] >= M_IFO)
        if r["IFO"] != "index error":
            X = oracle.OFDM_demodulator(y.reshape((N + Tg, S), order="F"), Tg)              # T4:308-310
            r["X0"] = X                                                                     # what fine_sync is given
            if td or fd:
                X = oracle.fine_sync(X, frames["pc"], frames["pv"], td, fd, variant="T4")[0]        # T4:314
            if mp:
                H, _ = oracle.estimate_channel(X, frames["allc"], frames["pc"], frames["pv"])       # T4:318
                r["H"] = np.asarray(H)[:nc]
                with np.errstate(divide="ignore", invalid="ignore"):
                    X = oracle.equalize_signal(X, H, nc)                                    # T4:334
            r["iq"] = oracle.get_payload(X, frames["dc"]).ravel(order="F")                  # T4:340-341
            r["bits"] = np.asarray(oracle.demapping(-1, r["iq"], case.const)).ravel()      # T4:347
        out.append(r)
    _REPLAY[key] = out
    return out


def expected_status(r):
    """status of ofdm_rx_chain_task4 for a replayed frame: -1 = remove_IFO's index error, 1 = the catch branch, else 0."""
    if r["IFO"] == "index error":
        return -1
    return 0 if r["ok"] else 1
