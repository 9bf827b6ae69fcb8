"""The refusals of the fused frame generator and the BER sweeps (csrc/txf_plan.hpp), shared by tests/test_txf_plan_host.py (the
header alone, on the CPU) and tests/test_gpu_txf_parent.py (the library through api.py, against the recorded parent).

MSG: refusal id -> the message as the source of the commit before txf_plan.hpp has it, a C format, verbatim.
ORDER: entry family -> its checks in the order the entry makes them, each (id, the `what` its message names).
BREAK: refusal id -> (the key=value tokens of tests/host/txf_plan_main.cpp's `prelude` command that make this check fail,
the values of the message's formats behind `what`).  A call broken for every check from position i of ORDER on must be refused
by check i: the first refusal wins.
API: the refused calls that can be made through api.py, each (name, family, RxPlan method, plan set-up, keyword arguments,
id of the refusal expected, `what`, format values); several are wrong in two ways."""
import numpy as np

REG = (1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0)          # T5/Main_model_Task_5.m:55
REG_STR = "".join(map(str, REG))
DESCR_ON = 0x80000000
DESCR_REG = DESCR_ON | sum(b << i for i, b in enumerate(REG[:14]))

MSG = {
    "args": "%s: bad arguments",
    "device": "RX plan belongs to device %d, the context is on device %d",
    "precision": "%s: precision flag differs from the plan's",
    "no_data": "%s: the plan has no data carriers",
    "pilots": "%s: pilots outside 1..N_carrier are not supported",
    "nfft": "%s: unsupported Nfft %d / T_guard %d",
    "stream": "%s: frame index outside the 32-bit stream range",
    "modes": "%s: sto_mode / cfo_mode must be 0, 1 or 2",
    "sc_ref": "%s: sc_ref_bits_out needs the Scrambler register",
    "channel": "tx_frames_fused: bad channel",
    "tap_delay": "tx_frames_fused: channel tap at delay %d (at most %d)",
    "tap_count": "tx_frames_fused: %d nonzero channel taps (at most %d)",
    "fade_count": "%s: n_taps must be 1 .. %d",
    "fade_missing": "%s: tap_delay / tap_power missing",
    "fade_delay": "%s: tap delay %d outside 0 .. %d",
    "fade_twice": "%s: tap delay %d given twice",
    "fade_power": "%s: tap powers must be positive and finite",
    "register": "%s: register entries must be 0 or 1",
    "descr_needed": "%s: with the Scrambler on the plan needs a DeScrambler with the same register (ofdm_rx_plan_set_descrambler)",
    "descr_unwanted": "%s: the plan descrambles but the frames are not scrambled",
    "points_missing": "%s: snr_db / seeds missing",
    "points_many": "%s: too many points",
    "mmse_points": "%s: an MMSE-mode plan is built for one SNR (n_points must be 1)",
    "mmse_fading": "%s: an MMSE-mode plan is built for one channel h (ofdm_rx_plan_set_mmse)",
    "chunk_cap": "ber_sweep_task4: max_frames_per_chunk must be 0..65535 (the limit of rx_chain_task4)",
    "mer_skip": "ber_sweep_task4_ex: mer_skip must be 0 .. nd * N_symb - 1 (%lld)",
    "nmse_mp": "ber_sweep_task4: the NMSE outputs need mp_desync (without estimate_channel there is no estimate)",
}


def message(rid, what, values=()):
    fmt = MSG[rid].replace("%lld", "%d")
    return fmt % ((what,) * fmt.startswith("%s") + tuple(values))


_PLAN = ["device", "precision", "no_data", "pilots", "nfft", "stream"]
_STATIC = ["channel", "tap_delay", "tap_count"]
_FADING = ["fade_count", "fade_missing", "fade_delay", "fade_twice", "fade_power"]
_DESCR = ["register", "descr_needed", "descr_unwanted"]


def _order(what, ids, later=None, later_ids=()):
    return [(i, what) for i in ids] + [(i, later) for i in later_ids]


ORDER = {
    "gen": _order("tx_frames_fused_ex", ["args"] + _PLAN + ["modes", "sc_ref"] + _STATIC),
    "gen_fading": _order("tx_frames_fading_ex", ["args"] + _PLAN + ["modes", "sc_ref"] + _FADING),
    "t5": _order("ber_sweep_task5", ["args", "points_missing", "points_many"] + _PLAN + ["mmse_points"] + _DESCR + _STATIC),
    "t5_fading": _order("ber_sweep_task5_fading", ["args", "points_missing", "points_many"] + _PLAN + ["mmse_fading"] + _DESCR + _FADING),
    "t4": _order("ber_sweep_task4", ["args"] + _STATIC + ["chunk_cap", "points_missing", "points_many"] + _PLAN +
                 ["modes"] + _DESCR + ["mer_skip", "nmse_mp"]),
    "t4_fading": _order("ber_sweep_task4_fading", ["args"] + _FADING, "ber_sweep_task4",
                        ["chunk_cap", "points_missing", "points_many"] + _PLAN + ["modes"] + _DESCR + ["mer_skip", "nmse_mp"]),
}

_H65 = ",".join(f"{i}:1:0" for i in range(65))
BREAK = {
    "args": (dict(plan=0), ()),
    "device": (dict(device=1, ctx_device=0), (1, 0)),
    "precision": (dict(f64_flag="FLIP"), ()),
    "no_data": (dict(nd=0), ()),
    "pilots": (dict(pilots_in_band=0), ()),
    "nfft": (dict(nfft=100, t_guard=12), (100, 12)),
    "stream": (dict(frame0=2 ** 32 - 3), ()),
    "modes": (dict(sto_mode=3), ()),
    "sc_ref": (dict(sc_ref_out=1, reg="none"), ()),
    "channel": (dict(h="null", h_len=3), ()),
    "tap_delay": (dict(h="x", h_len=4098, h_taps=_H65 + ",4097:0:1"), (4097, 4096)),
    "tap_count": (dict(h="x", h_len=70, h_taps=_H65), (65, 64)),
    "fade_count": (dict(n_taps=65, delays="0", powers="1"), (64,)),
    "fade_missing": (dict(n_taps=2, delays="null", powers="1,1"), ()),
    "fade_delay": (dict(n_taps=2, delays="3,5000", powers="1,0"), (5000, 4096)),
    "fade_twice": (dict(n_taps=2, delays="3,3", powers="1,0"), (3,)),
    "fade_power": (dict(n_taps=2, delays="0,3", powers="1,0"), ()),
    "register": (dict(reg="2" + REG_STR[1:]), ()),
    "descr_needed": (dict(reg=REG_STR, descr=0), ()),
    "descr_unwanted": (dict(reg="none", descr=DESCR_ON), ()),
    "points_missing": (dict(snr=0), ()),
    "points_many": (dict(n_points=2 ** 31), ()),
    "mmse_points": (dict(mmse=1), ()),
    "mmse_fading": (dict(mmse=1), ()),
    "chunk_cap": (dict(max_chunk=65536), ()),
    "mer_skip": (dict(mer_skip=-1), (-1,)),
    "nmse_mp": (dict(nmse_out=1, mp_desync=0), ()),
}


def base_call(family, shape):
    """The key=value tokens of an accepted `prelude` call of the family on `shape` (a dict of the shape keys)."""
    kv = dict(shape, family=family.split("_")[0], what=ORDER[family][0][1], plan=1, out=1, f64_flag=shape["f64"], frame0=0,
              n_frames=5, reg="none", device=0, ctx_device=0, pilots_in_band=1, descr=0, mmse=0)
    if family.endswith("fading"):
        kv.update(fading=1, n_taps=3, delays="0,3,7", powers="1,0.5,0.25")
    else:
        kv.update(h="x", h_len=8, h_taps="0:1:0,3:0.5:0.25")
    if family[:2] in ("t5", "t4"):
        kv.update(snr=1, seeds=1, n_points=2, max_chunk=0)
    if family[:2] == "t4" or family.startswith("gen"):
        kv.update(imp=1, sto_mode=2, cfo_mode=1)
    return kv


def broken_from(family, shape, i):
    """base_call broken for every check of ORDER[family] from position i on (an earlier check's tokens override a later one's;
    of checks that exclude each other the earliest stays)."""
    kv = base_call(family, shape)
    for rid, _ in reversed(ORDER[family][i:]):
        for k, v in BREAK[rid][0].items():
            kv[k] = (1 - shape["f64"]) if v == "FLIP" else v
    return kv


# ---- the refused calls that api.py can make.  h / fading values are built by the functions below when the call is made.
def h_taps(n, at):
    h = np.zeros(n, np.complex128)
    h[list(at)] = 1.0
    return h


H_LATE = lambda: h_taps(4098, [0, 4097])                        # noqa: E731
H_MANY = lambda: h_taps(70, range(65))                          # noqa: E731
FAR = 2 ** 32 - 3                                               # frame0 + 5 frames leaves the 32-bit stream range
LINE = ([0, 3, 7], [1.0, 0.5, 0.25])
# (name, RxPlan method, plan set-up ("" | "mmse" | "descr"), kwargs, refusal id, what, format values)
API = [
    ("gen-stream", "tx_frames_fused", "", dict(frame0=FAR), "stream", "tx_frames_fused", ()),
    ("gen-ex-stream", "tx_frames_fused", "", dict(frame0=FAR, Time_Delay=3), "stream", "tx_frames_fused_ex", ()),
    ("gen-fading-stream", "tx_frames_fused", "", dict(frame0=FAR, fading=LINE), "stream", "tx_frames_fading", ()),
    ("gen-fading-ex-stream", "tx_frames_fused", "", dict(frame0=FAR, fading=LINE, Freq_Shift=0.1), "stream", "tx_frames_fading_ex", ()),
    ("gen-tap-delay", "tx_frames_fused", "", dict(h=H_LATE), "tap_delay", None, (4097, 4096)),
    ("gen-tap-count", "tx_frames_fused", "", dict(h=H_MANY), "tap_count", None, (65, 64)),
    ("gen-stream-before-tap-delay", "tx_frames_fused", "", dict(frame0=FAR, h=H_LATE), "stream", "tx_frames_fused", ()),
    ("gen-fade-count-0", "tx_frames_fused", "", dict(fading=([], [])), "fade_count", "tx_frames_fading", (64,)),
    ("gen-fade-count-65", "tx_frames_fused", "", dict(fading=(list(range(65)), [1.0] * 65)), "fade_count", "tx_frames_fading", (64,)),
    ("gen-fade-delay", "tx_frames_fused", "", dict(fading=([0, -2], [1.0, 1.0])), "fade_delay", "tx_frames_fading", (-2, 4096)),
    ("gen-fade-twice", "tx_frames_fused", "", dict(fading=([4, 4], [1.0, 1.0]), Time_Delay="random"), "fade_twice", "tx_frames_fading_ex", (4,)),
    ("gen-fade-power-0", "tx_frames_fused", "", dict(fading=([0, 4], [1.0, 0.0])), "fade_power", "tx_frames_fading", ()),
    ("gen-fade-power-nan", "tx_frames_fused", "", dict(fading=([0, 4], [1.0, float("nan")])), "fade_power", "tx_frames_fading", ()),
    ("gen-fade-delay-before-power", "tx_frames_fused", "", dict(fading=([0, 5000], [1.0, -1.0])), "fade_delay", "tx_frames_fading", (5000, 4096)),
    ("t5-args", "ber_sweep", "", dict(max_frames_per_chunk=-1), "args", "ber_sweep_task5", ()),
    ("t5-stream", "ber_sweep", "", dict(frame0=FAR), "stream", "ber_sweep_task5", ()),
    ("t5-mmse-points", "ber_sweep", "mmse", dict(), "mmse_points", "ber_sweep_task5", ()),
    ("t5-mmse-fading", "ber_sweep", "mmse", dict(fading=LINE), "mmse_fading", "ber_sweep_task5_fading", ()),
    ("t5-register", "ber_sweep", "descr", dict(Register=(2,) + REG[1:]), "register", "ber_sweep_task5", ()),
    ("t5-descr-needed", "ber_sweep", "", dict(Register=REG), "descr_needed", "ber_sweep_task5", ()),
    ("t5-descr-unwanted", "ber_sweep", "descr", dict(), "descr_unwanted", "ber_sweep_task5", ()),
    ("t5-tap-delay", "ber_sweep", "", dict(h=H_LATE), "tap_delay", None, (4097, 4096)),
    ("t5-fade-twice", "ber_sweep", "", dict(fading=([4, 4], [1.0, 1.0])), "fade_twice", "ber_sweep_task5_fading", (4,)),
    ("t5-stream-before-mmse", "ber_sweep", "mmse", dict(frame0=FAR), "stream", "ber_sweep_task5", ()),
    ("t5-mmse-before-descr", "ber_sweep", "mmse", dict(Register=REG), "mmse_points", "ber_sweep_task5", ()),
    ("t5-descr-before-tap-count", "ber_sweep", "descr", dict(h=H_MANY), "descr_unwanted", "ber_sweep_task5", ()),
    ("t4-chunk-cap", "ber_sweep_task4", "", dict(max_frames_per_chunk=65536), "chunk_cap", None, ()),
    ("t4-chunk-cap-negative", "ber_sweep_task4", "", dict(max_frames_per_chunk=-1), "chunk_cap", None, ()),
    ("t4-tap-delay-before-chunk-cap", "ber_sweep_task4", "", dict(h=H_LATE, max_frames_per_chunk=65536), "tap_delay", None, (4097, 4096)),
    ("t4-fade-power-before-stream", "ber_sweep_task4", "", dict(fading=([0, 4], [1.0, float("inf")]), frame0=FAR), "fade_power", "ber_sweep_task4_fading", ()),
    ("t4-stream", "ber_sweep_task4", "", dict(frame0=FAR), "stream", "ber_sweep_task4", ()),
    ("t4-fading-stream", "ber_sweep_task4", "", dict(frame0=FAR, fading=LINE), "stream", "ber_sweep_task4", ()),
    ("t4-descr-needed", "ber_sweep_task4", "", dict(Register=REG), "descr_needed", "ber_sweep_task4", ()),
    ("t4-descr-unwanted", "ber_sweep_task4", "descr", dict(), "descr_unwanted", "ber_sweep_task4", ()),
    ("t4-mer-skip", "ber_sweep_task4", "", dict(want_mer=True, mer_skip="ND_NSYMB"), "mer_skip", None, "ND_NSYMB"),
    ("t4-nmse-mp", "ber_sweep_task4", "", dict(want_nmse=True, mp_desync=0), "nmse_mp", None, ()),
    ("t4-mer-skip-before-nmse-mp", "ber_sweep_task4", "", dict(want_mer=True, mer_skip=-1, want_nmse=True, mp_desync=0), "mer_skip", None, (-1,)),
    ("t4-descr-before-mer-skip", "ber_sweep_task4", "descr", dict(want_mer=True, mer_skip=-1), "descr_unwanted", "ber_sweep_task4", ()),
]
