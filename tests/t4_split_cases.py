"""What rx_chain_task4 and ber_sweep_task4 returned on the commit before task4_run was split into prepare / front end / the stages
behind (tests/golden/t4_split_parent.json, written by `python tests/golden/make_t4_split_golden.py` on that commit through these
public calls only).  TEST INFRASTRUCTURE: a helper module (no tests here), imported by that script and by
test_gpu_task4_split_parent.py.  One small batch per route of t4_routes.py: every case of t4_cases.CASES in both precisions with
the flags (1, 1, 1) and (0, 0, 1), and the seven switch runs."""
import hashlib
import os

import numpy as np

import t4_cases as tc
from t4_routes import SWITCH_ROWS

T4_SWITCHES = ("OFDM_T4_UNFUSED_SYNC", "OFDM_T4_FULL_ACF", "OFDM_T4_STAGED", "OFDM_T4_NO_WAVE", "OFDM_T4_DENSE_SPLINE")
RUNS = [(c.name, p, fl, ()) for c in tc.CASES for p in ("fp64", "fp32") for fl in tc.TWO_FLAGS]
RUNS += [(name, p, (1, 1, 1), (switch,)) for switch, name in SWITCH_ROWS for p in ("fp64", "fp32")]
FIELDS = ("TgPosition", "IFO", "status", "errors", "packed", "mer_sums", "sweep_errors", "sweep_status_counts", "sweep_frame_errors",
          "sweep_mer_sums", "sweep_frame_mer_sums")
SWEEP_SNRS, SWEEP_FRAMES = [30.0, 15.0], 3


def run_id(run):
    name, precision, flags, env = run
    return "-".join([name, precision, "".join(map(str, flags)), *env])


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _hex(a):
    return [f"{int(v):016x}" for v in np.ascontiguousarray(np.asarray(a, np.float64)).ravel().view(np.uint64)]


def record(ofdm, oracle, run):
    """One rx_chain_task4 call with the MER sums on the case's frames and one ber_sweep_task4 call of 2 points x 3 frames with the
    case's channel on a plan of their own, with only the switches of the run set; reduced to what the golden file stores.  Error
    counts, bits and MER sums of the receiver call on the frames with status >= 0 (remove_IFO's index error leaves the others
    undefined)."""
    from ofdm_course_amd import frames as fr
    name, precision, flags, env = run
    case = tc.BY_NAME[name]
    saved = {v: os.environ.pop(v, None) for v in T4_SWITCHES}
    for v in env:
        os.environ[v] = "1"
    try:
        d = tc.build_frames(oracle, case)
        rx = d["rx"] if precision == "fp64" else d["rx"].astype(np.complex64)
        plan = ofdm.RxPlan(case.Nfft, case.T_guard, case.N_symb, case.N_carrier, d["pc"], d["dc"], d["col"],
                           int(np.ceil(case.N_carrier / 6)), 3, case.const, precision=precision)
        out = ofdm.rx_chain_task4(plan, rx, *flags, ref_bits_packed=fr.pack_bits(d["bits"]), want_mer=True)
        status = np.asarray(out["status"])
        live = status >= 0
        rec = dict(TgPosition=[int(v) for v in out["TgPosition"]], IFO=[int(v) for v in out["IFO"]], status=[int(v) for v in status],
                   errors=[int(e) if ok else -1 for e, ok in zip(np.asarray(out["errors"]), live)],
                   packed=_sha(np.asarray(out["bits"])[live]), mer_sums=_hex(np.asarray(out["mer_sums"])[live]))
        sw = plan.ber_sweep_task4(SWEEP_SNRS, SWEEP_FRAMES, h=d["h"], Time_Delay="random" if flags[0] else None,
                                  Freq_Shift="random" if flags[1] else None, time_desync=flags[0], freq_desync=flags[1],
                                  mp_desync=flags[2], seed=case.seed, want_frame_errors=True, want_mer=True, want_frame_mer=True)
        rec.update(sweep_errors=[int(v) for v in np.asarray(sw["errors"])],
                   sweep_status_counts=[int(v) for v in np.asarray(sw["status_counts"]).ravel()],
                   sweep_frame_errors=[int(v) for v in np.asarray(sw["frame_errors"]).ravel()],
                   sweep_mer_sums=_hex(sw["mer_sums"]), sweep_frame_mer_sums=_hex(sw["frame_mer_sums"]))
        plan.close()
    finally:
        for v in T4_SWITCHES:
            os.environ.pop(v, None)
            if saved[v] is not None:
                os.environ[v] = saved[v]
    return rec
