"""The route table of the Task-5 dispatcher stays in step with the dispatch sources (CPU only): routes.CASES covers
routes.ROUTES and nothing else, the switches of the table are the switches the sources read, the field values and pairs the
table promises occur in both precisions, the recorded pick gaps are the oracle's, and the refusals are where the model says."""
import dataclasses

import pytest

import routes
from routes import CASES, GAPS, REFUSALS, ROUTES


def _routes_of(cases):
    return {c.name: c.route() for c in cases}


def test_every_case_is_a_listed_route_and_every_route_has_a_case():
    """ROUTES is written from the dispatch code, not from CASES: a route listed there without a case, in a precision it is
    listed for, fails here, and so does a case on a route nobody listed."""
    listed = {}
    for r, why, prec in ROUTES:
        assert r not in listed, f"listed twice: {r}"
        assert why and prec in ("fp32", "fp64", "both"), r
        listed[r] = ("fp32", "fp64") if prec == "both" else (prec,)
    hit = {(c.route(), c.precision) for c in CASES}
    stray = {c.name: c.route() for c in CASES if c.precision not in listed.get(c.route(), ())}
    assert not stray, f"cases on routes that ROUTES does not list: {stray}"
    missing = [(r, p) for r, ps in listed.items() for p in ps if (r, p) not in hit]
    assert not missing, f"routes without a case: {missing}"
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)


def test_every_case_is_necessary():
    """No case can be removed without losing a (route, precision) or a (switch setting, precision): together with the test
    above and the switch test below, removing any one case fails this module."""
    for c in CASES:
        rest = [x for x in CASES if x is not c]
        only_route = (c.route(), c.precision) not in {(x.route(), x.precision) for x in rest}
        only_env = bool(c.env) and (frozenset(c.env.items()), c.precision) not in {(frozenset(x.env.items()), x.precision) for x in rest}
        assert only_route or only_env, f"{c.name} duplicates another case"


# every switch setting that must be exercised, per precision: removing the case that carries one fails here
SWITCH_SETTINGS = {
    "fp32": [{"OFDM_FAST_NO_WAVE": "1"}, {"OFDM_PILOT_FPW": "1"}, {"OFDM_WAVE_EXACT_SLICER": "1"}, {"OFDM_WAVE_NO_SKIP": "1"},
             {"OFDM_OMP_C0_LDS": "1"}, {"OFDM_OMP_NO_FFT": "1"}, {"OFDM_OMP_NO_MFMA": "1"},
             {"OFDM_FAST_UNFUSED": "1", "OFDM_OMP_FPW": "1"}, {"OFDM_FAST_UNFUSED": "1", "OFDM_OMP_FPW": "2"},
             {"OFDM_CHAIN_GENERIC": "1"}, {"OFDM_MMSE_TWO_LAUNCHES": "1"}, {"OFDM_MMSE_G": "1"}, {"OFDM_MMSE_G": "2"},
             {"OFDM_MMSE_G": "8"}, {"OFDM_MMSE_DENSE": "1"}, {"OFDM_MMSE_NO_MFMA": "1"}, routes.NO8192,
             {"OFDM_SPLIT_NO_COOP": "1"}, {"OFDM_SPLIT_NO_R2": "1"}, {**routes.NO8192, "OFDM_EQD_SCALAR": "1"},
             {**routes.NO8192, "OFDM_SPLIT_GENERIC_FFT": "1"}, {**routes.NO8192, "OFDM_SPLIT_NO_PLS_FUSE": "1"},
             {**routes.NO8192, "OFDM_SPLIT_ALL_ROWS": "1"}],
    "fp64": [{"OFDM_OMP_NO_FFT": "1"}, {"OFDM_FAST_UNFUSED": "1", "OFDM_OMP_FPW": "8"}, {"OFDM_SPLIT_GENERIC_FFT": "1"},
             {"OFDM_SPLIT_NO_PLS_FUSE": "1"}, {"OFDM_SPLIT_ALL_ROWS": "1"}],
}


def test_every_switch_setting_has_its_case():
    for prec, settings in SWITCH_SETTINGS.items():
        have = [c.env for c in CASES if c.precision == prec and c.env]
        for e in settings:
            assert e in have, (prec, e)
        for e in have:
            assert e in settings, (prec, e)


def test_cases_are_oracle_sized():
    for c in CASES + REFUSALS:
        assert 1 <= c.n_frames <= 11, c.name
        assert c.snr >= 24.0, c.name


def test_table_switches_are_the_switches_of_the_dispatch_sources():
    """A getenv("OFDM_...") added to a dispatch file fails here until a case sets it; a switch removed from the sources fails
    until its case goes.  (Excluded by name, with the reason, in routes.EXCLUDED_SWITCHES.)"""
    src, tab = routes.dispatch_switches(), routes.table_switches()
    assert src == tab, f"in the sources only: {sorted(src - tab)}; in the table only: {sorted(tab - src)}"
    assert len(src) >= 19


def test_switch_cases_name_their_base_route():
    for c in CASES:
        if c.base_env is not None:
            assert set(c.base_env.items()) < set(c.env.items()), c.name


FIELDS_F32 = dict(
    entry={"generic", "fast", "split"},
    front={"fused", "pilot+omp", "demod8192", "demod8192+pls", "demod_generic+pls"},
    estimator={"omp_fft", "omp_mfma", "omp_scalar", "mmse_fused", "mmse_factored", "mmse_dense_mfma", "mmse_dense_scalar"},
    omp_state={"regs", "wave", "-"}, c0={"reg", "lds", "-"},
    symbols={"chain_generic", "wave<skip0>", "wave<skip02>", "wave<none>", "wave<exact>", "coop4", "r2", "eq_demap<vec>",
             "eq_demap<scalar>"} | {f"rx_symbols<{nw},{p}>" for nw in (1, 2, 4, 8) for p in ("true", "false")},
    ba={0, 2, 3, 4}, descr={"none", "in_kernel", "pass"}, mer={False, True})
# fp64 has no MFMA form, no wave / coop4 / r2 stage, no vector eq_demap and therefore no in-kernel DeScrambler
FIELDS_F64 = dict(
    entry=FIELDS_F32["entry"], front=FIELDS_F32["front"], estimator={"omp_fft", "omp_scalar", "mmse_dense_scalar"},
    omp_state=FIELDS_F32["omp_state"], c0=FIELDS_F32["c0"],
    symbols={"chain_generic", "eq_demap<scalar>"} | {f"rx_symbols<{nw},{p}>" for nw in (1, 2, 4, 8) for p in ("true", "false")},
    ba={0, 2, 3, 4}, descr={"none", "pass"}, mer={False, True})


@pytest.mark.parametrize("precision,fields", [("fp32", FIELDS_F32), ("fp64", FIELDS_F64)])
def test_every_field_value_and_pair_occurs(precision, fields):
    rs = [c.route() for c in CASES if c.precision == precision]
    for name, want in fields.items():
        got = {routes.strip_knob(getattr(r, name)) for r in rs}
        assert got == want, f"{precision} {name}: missing {want - got}, unexpected {got - want}"
    # pairs, by kernel family (the template parameters NW / PRUNE2 / skip form do not enter the slicer or the estimator)
    fam = {routes.symbols_family(s) for s in fields["symbols"]}
    pairs = {(routes.symbols_family(r.symbols), r.ba) for r in rs}
    assert pairs == {(s, b) for s in fam for b in (0, 2, 3, 4)}, {(s, b) for s in fam for b in (0, 2, 3, 4)} - pairs
    # (by family: ROUTES says which (instantiation, ba) pairs are knowingly left out)
    est = {(routes.symbols_family(r.symbols), routes.estimator_family(r.estimator)) for r in rs}
    want = {(s, e) for s in fam for e in ("omp", "mmse")} - {("chain_generic", "mmse")}          # refused: mmse_entry
    assert est == want, want - est


def test_each_gap_of_the_issue_has_a_named_case():
    text = " | ".join(c.covers for c in CASES)
    for g in ("gap 1a", "gap 1b", "gap 2", "gap 3", "gap 4", "gap 5", "gap 6", "gap 7", "gap 8"):
        assert g in text, g


def test_refusals_are_where_the_model_says():
    for c in REFUSALS:
        with pytest.raises(routes.Refused) as e:
            c.route()
        assert e.value.where == routes.REFUSAL_IDS[c.name], c.name
    # the symbol_lds refusal of the fast form cannot fire (routes.FAST_SYMBOL_LDS_MAX): no case for it
    assert routes.FAST_SYMBOL_LDS_MAX <= routes.STAGE_LDS_LIMIT
    # the refused frames really are oracle-sized and the refusing geometry is reachable without the refusing condition
    base = dataclasses.replace([c for c in REFUSALS if c.name == "refuse-generic-lds"][0], env={})
    assert base.route().entry == "split"


def test_recorded_pick_gaps_are_the_oracles():
    """Every fp32 OMP case is tie-free by construction: the oracle's own pursuit on the case's Philox frames never has a top-2
    score gap below 1e-3 of the maximum (the near-tie threshold is 1e-4, pick_audit.py), and the table records the figure."""
    from oracle import ofdm_oracle
    need = [c for c in CASES if c.precision == "fp32" and c.mode == "omp"]
    assert {c.name for c in need} == set(GAPS), set(GAPS) ^ {c.name for c in need}
    for c in need:
        assert c.set_aside == 0
        g = routes.oracle_min_gap(c, ofdm_oracle)
        assert g > 1e-3, (c.name, g)
        assert abs(g - GAPS[c.name]) <= 0.01 * g, (c.name, g, GAPS[c.name])
