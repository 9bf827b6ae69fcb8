"""CPU checks of the plan's OMP route (ofdm_rx_plan_set_omp_route) and of the drivers that use it: the cases of
tests/test_gpu_omp_route.py are tie-free by the oracle's own pursuit, the ABI and the Python surface are bound, the dispatch
sources call the one stage function, and drivers/sweep_ber.py (--random-pilots, --mask-seed, --dictionary full) and
drivers/task5_masks.py do what they say against a library that only records."""
import os
import re

import numpy as np
import pytest

import omp_route_cases as oc
import routes
from oracle_lib import OracleLib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ofdm-course_amd", "csrc")


def test_cases_are_oracle_sized_and_tie_free(oracle):
    """Every fp32 case: the smallest top-two gap of the oracle's pursuit on the case's frames is above 1e-3 and is the recorded
    one; no frame is set aside (the cap is zero).  The fp64 cases need distinct picks only: above 1e-6."""
    need = [c for c in oc.CASES if c.precision == "fp32"]
    assert {c.name for c in need} == set(oc.GAPS)
    for c in oc.CASES:
        assert 3 <= c.n_frames <= 8 and c.snr >= 24.0 and 3 <= len(c.delays) <= 6 <= c.pilot_carriers().size, c.name
        assert c.set_aside == 0
        if c not in oc.SPLIT_512:                                  # (the split entry needs > 48 Ki decisions per frame)
            assert c.n_symb == 2 and c.nc <= 256, c.name
    for c in need:
        g = routes.oracle_min_gap(c, oracle)
        print(c.name, g)
        assert g > 1e-3, (c.name, g)
        assert abs(g - oc.GAPS[c.name]) <= 0.01 * g, (c.name, g, oc.GAPS[c.name])
    for c in oc.AUTO_2048:
        assert routes.oracle_min_gap(c, oracle) > 1e-6


def test_comb_pilots_alias_the_full_dictionary(oracle):
    """Why the comb-4 case stops at K = Nfft / comb: beyond it two atoms are the same column on the comb's carriers."""
    c = oc.WIDE_512[0]
    S = oracle.sensing_matrix(c.pilot_carriers().astype(np.float64), c.nfft, c.nfft)
    assert np.allclose(S[:, 5], S[:, 5 + c.nfft // c.comb], atol=1e-12) and c.K == c.nfft // c.comb


def test_case_routes_are_the_ones_meant():
    lim = routes.STAGE_LDS_LIMIT
    for c in oc.AUTO_4096 + oc.AUTO_2048:                           # a default plan refuses them: omp_lds
        with pytest.raises(routes.Refused) as e:
            routes.expected_route(c, c.precision, "omp", False, True, {})
        assert e.value.where == "omp_lds"
    for c in oc.WIDE_512:
        assert routes.expected_route(c, c.precision, "omp", False, True, {}).front == "fused"
    for c in oc.WIDE_512_MASK + oc.WIDE_1024:
        r = routes.expected_route(c, c.precision, "omp", False, True, {})
        assert (r.entry, r.front) == ("fast", "pilot+omp")
    for c in oc.SPLIT_512:
        assert routes.expected_route(c, c.precision, "omp", False, True, {}).entry == "split"
    assert lim == 150 * 1024


def test_binding_and_python_surface():
    import ctypes as C
    from ofdm_course_amd import _lib as L
    from ofdm_course_amd import api
    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "ofdm_mi355x.h")).read()
    assert "int ofdm_rx_plan_set_omp_route(ofdm_rx_plan* plan, int route);" in hdr
    assert list(lib.ofdm_rx_plan_set_omp_route.argtypes) == [C.c_void_p, C.c_int]
    assert list(lib.ofdm_rx_plan_get_omp_route.argtypes) == [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    assert callable(api.RxPlan.set_omp_route) and isinstance(api.RxPlan.omp_route, property)
    assert api._OMP_ROUTES == {"auto": 0, "batch": 1, "wide": 2}      # the words of OMP_estimate_batch(route=)


def test_receiver_call_sites_go_through_the_stage_function():
    """The three OMP call sites of the receiver run the kernel the route chose (ChainRoute::omp_taken) and report it;
    omp_batch_run and omp_wide_run are each called from the one stage function only, which ofdm_chain_fast.hip,
    ofdm_chain_split.hip and ofdm_part2.hip reach and nothing calls around."""
    code = {}
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith((".hip", ".hpp")):
            src = open(os.path.join(CSRC, fn)).read()
            code[fn] = "\n".join(ln.split("//")[0] for ln in src.splitlines())
    site = r"OFDM_TRY\(omp_stage_run<T>\(P, pv\.nfft, n_frames, route\.omp_taken, pv\.omp_out\)\)"
    assert len(re.findall(site, code["ofdm_chain_fast.hip"])) == 1
    assert len(re.findall(site, code["ofdm_chain_split.hip"])) == 2
    assert len(re.findall(r"omp_stage_run<T>\(", code["ofdm_chain_fast.hip"])) == 1
    assert len(re.findall(r"omp_stage_run<T>\(", code["ofdm_chain_split.hip"])) == 2
    assert len(re.findall(r"OFDM_TRY\(omp_stage_run<T>\(", code["ofdm_part2.hip"])) == 3
    for fn in ("ofdm_chain_split.hip", "ofdm_part2.hip"):
        assert "omp_batch_run" not in code[fn] and "omp_wide_run" not in code[fn], fn
    assert "OFDM_TRY(omp_batch_run" not in code["ofdm_chain_fast.hip"]
    # calls (a name followed by its template argument and a parenthesis, outside a declaration or definition): one each, in the
    # stage function of chain_fast_core.hpp
    calls = {k: [(fn, m.group(0)) for fn, c in code.items() for m in re.finditer(r"(?<!int )\b" + k + r"<T>\(", c)]
             for k in ("omp_batch_run", "omp_wide_run")}
    for k, v in calls.items():
        assert [fn for fn, _ in v] == ["chain_fast_core.hpp"], (k, v)
    stage = code["chain_fast_core.hpp"]
    body = stage[stage.index("inline int omp_stage_run("):]
    body = body[: body.index("\n}\n")]
    assert "omp_batch_run<T>(" in body and "omp_wide_run<T>(" in body and stage.count("inline int omp_stage_run(") == 1


# ---- the drivers against a library that records
class _Plan:
    def __init__(self, log, args, kw):
        self.log, self.args, self.kw, self.route = log, args, kw, "batch"
        self.frame_bits = 1000
        log.append(("RxPlan", args, kw))

    def set_omp_route(self, route):
        self.route = route
        self.log.append(("set_omp_route", route))

    @property
    def last_omp_route(self):
        return "wide" if self.args[7] == self.args[0] else "batch"         # K == Nfft

    def ber_sweep(self, SNRs, frames_per_point, **kw):
        self.log.append(("ber_sweep", list(SNRs), frames_per_point, kw, self.route, self.args))
        n_p = len(self.args[4])
        return dict(errors=np.array([1000 // n_p], dtype=np.int64), bits=frames_per_point * self.frame_bits,
                    nmse_sums=np.array([1.0 / n_p]))

    def close(self):
        self.log.append(("close",))


class _Recorder(OracleLib):
    def __init__(self, oracle):
        super().__init__(oracle)
        self.log = []

    def RxPlan(self, *args, **kw):
        return _Plan(self.log, args, kw)


def test_sweep_ber_flags(oracle, capsys):
    from ofdm_course_amd import frames as fr
    from ofdm_course_amd.drivers import sweep_ber
    from ofdm_course_amd.drivers.task5_part2 import random_pilot_layout
    a = sweep_ber.parse_args(["--config", "M", "--fused", "--random-pilots", "64", "--mask-seed", "9", "--dictionary", "full"])
    assert (a.random_pilots, a.mask_seed, a.dictionary) == (64, 9, "full")
    for argv in (["--config", "M", "--random-pilots", "64"], ["--config", "C5", "--fused", "--dictionary", "full"],
                 ["--config", "M", "--fused", "--estimator", "mmse-ls", "--random-pilots", "64"],
                 ["--config", "M", "--fused", "--random-pilots", "2"]):
        with pytest.raises(SystemExit):
            sweep_ber.parse_args(argv)
    capsys.readouterr()
    assert sweep_ber.check_pilots("C5", "omp", False, None, "comb") is None          # nothing asked: nothing refused
    cfg = sweep_ber.apply_pilots(fr.config_M(), 64, 9, "full")
    want = random_pilot_layout(2048, 512, 64, 9)[1]
    assert np.array_equal(cfg.pilotCarriers, want) and want.size == 64 and np.all(np.diff(want) > 0)
    assert want.min() >= 1 and want.max() <= 512 and cfg.K == 2048
    assert not np.isin(cfg.dataCarriers, want).any() and cfg.dataCarriers.size == 512 - 64
    assert not np.array_equal(want, random_pilot_layout(2048, 512, 64, 10)[1])
    assert sweep_ber.apply_pilots(fr.config_M(), 64, 9, "comb").K == 128               # the mask alone keeps the comb's dictionary
    assert sweep_ber.apply_pilots(fr.config_M(), None, 1, "full").K == 2048
    lib = _Recorder(oracle)
    sweep_ber.make_sweep_plan(cfg, lib, "fp32", 0, "full")
    (_, args, kw), route = lib.log
    assert args[:4] == (2048, 256, 14, 512) and np.array_equal(args[4], want) and args[7] == 2048 and kw["precision"] == "fp32"
    assert route == ("set_omp_route", "auto")
    lib = _Recorder(oracle)
    sweep_ber.make_sweep_plan(fr.config_M(), lib, "fp32", 0)
    assert [e[0] for e in lib.log] == ["RxPlan"]                                      # the default plan: no route set


def test_mask_study_driver(oracle):
    from ofdm_course_amd.drivers import common, task5_masks as tm
    from ofdm_course_amd.drivers.task5_part2 import random_pilot_layout, scenario_combs
    assert np.array_equal(tm.default_counts(1024), scenario_combs(1024)[1])
    assert tm.counts_for_rank(5, 0, 1) == [0, 1, 2, 3, 4]
    assert tm.counts_for_rank(5, 0, 2) == [0, 2, 4] and tm.counts_for_rank(5, 1, 2) == [1, 3]
    with pytest.raises(ValueError):
        tm.counts_for_rank(5, 2, 2)
    # the threshold on a synthetic table
    assert tm.threshold([128, 64, 32, 16], [0.001, 0.02, 0.049, 0.3]) == 32
    assert tm.threshold([16, 32], [0.05, 0.2]) is None and tm.threshold([16, 32], [float("nan"), 0.01]) == 32
    counts = [16, 32, 64]
    parts = []
    for world in (1, 2):
        for rank in range(world):
            lib = _Recorder(oracle)
            p = tm.run(lib, profile="EPA", pilots="random", counts=counts, frames=7, Nfft=4096, N_carrier=256, N_symb=2,
                       seed=2, rank=rank, world=world)
            calls = [e for e in lib.log if e[0] == "ber_sweep"]
            mine = tm.counts_for_rank(3, rank, world)
            assert len(calls) == len(mine)                                            # one call per pilot count
            assert [e[0] for e in lib.log] == ["RxPlan", "set_omp_route", "ber_sweep", "close"] * len(mine)
            for kk, (_, snrs, fpp, kw, route, args) in zip(mine, calls):
                assert snrs == [20.0] and fpp == 7 and route == "auto" and kw["want_nmse"] is True
                assert np.array_equal(args[4], random_pilot_layout(4096, 256, counts[kk], [2, 7, kk])[1])
                assert args[7] == 4096 and args[8] == len(kw["fading"][0])              # K = Nfft, taps = the profile's paths
                d, pw = common.fading_profile("EPA", 4e7)
                assert np.array_equal(kw["fading"][0], d) and np.array_equal(kw["fading"][1], pw)
                assert kw["seeds"] == [2 + 1000003 * kk]                              # keyed by the count, not by the rank
            assert [i for i in range(3) if p["bits"][i]] == mine
            parts.append(p)
    one, (a, b) = parts[0], parts[1:]
    for k in ("errors", "bits", "nmse_sums", "routes"):
        assert np.array_equal(one[k], a[k] + b[k]), k                                 # what the two all-reduces add up
    res = tm.finish(one)
    assert res["amounts_pilots"] == counts and res["omp_route"] == ["wide"] * 3
    assert np.allclose(res["BER"], [1000 // n / 7000 for n in counts]) and res["pilots_for_ber_below_5_percent"] == 16
    assert np.allclose(res["NMSE"], [1.0 / n / (7 * 256) for n in counts])
    # a mask whose pilot_step is 1 falls under the 100 % rule (Task5_part2.m:67-75) and has no payload: no call, BER NaN
    lib = _Recorder(oracle)
    res = tm.finish(tm.run(lib, profile="EPA", pilots="random", counts=counts, frames=7, Nfft=4096, N_carrier=256, N_symb=2, seed=1))
    assert len([e for e in lib.log if e[0] == "ber_sweep"]) == 2 and np.isnan(res["BER"][2]) and res["omp_route"][2] is None
    assert res["pilots_for_ber_below_5_percent"] == 16
    # the regular combs: the first comb of each count, K = ceil(Nfft / comb)
    lib = _Recorder(oracle)
    tm.run(lib, profile="EVA", pilots="regular", counts=[64, 32], frames=3, Nfft=4096, N_carrier=256, N_symb=2)
    plans = [e for e in lib.log if e[0] == "RxPlan"]
    assert [(len(e[1][4]), e[1][7]) for e in plans] == [(64, 1024), (32, 512)]
    assert np.array_equal(plans[0][1][4], np.arange(1, 257, 4))
    assert "lteFadingChannel" in tm.__doc__ and "NOT" in tm.__doc__
