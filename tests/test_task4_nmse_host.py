"""CPU: the entries of the Task-4 fading / NMSE sweep (ofdm_tx_frames_fading_ex, ofdm_ber_sweep_task4_nmse,
ofdm_ber_sweep_task4_fading) are declared, exported and bound with the header's argument counts, and the Python layer and the
driver carry the new keywords.  No compute: nothing here needs a GPU."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofdm_tx_frames_fading_ex", "ofdm_ber_sweep_task4_nmse", "ofdm_ber_sweep_task4_fading")


def _declarations():
    """name -> argument count of every prototype of include/ofdm_mi355x.h (comments stripped, as test_abi_and_host.py
    strips them)."""
    txt = open(os.path.join(ROOT, "include", "ofdm_mi355x.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(ofdm_[A-Za-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_new_entries_are_declared_exported_and_bound():
    from ofdm_course_amd import _lib
    decl = _declarations()
    lib = _lib.load()
    for name in NEW:
        assert name in decl, f"{name} is not declared in include/ofdm_mi355x.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.py"
    # every binding has the header's argument count (the new entries included)
    for name, argtypes in _lib.SIGNATURES.items():
        assert len(argtypes) == decl[name], (name, len(argtypes), decl[name])
    # the new entries are their siblings plus what the issue adds: STO / CFO modes, values and draws; two NMSE outputs;
    # (tap_delay, tap_power, n_taps) in place of (h, h_len)
    assert decl["ofdm_tx_frames_fading_ex"] == decl["ofdm_tx_frames_fading"] + 6 == 20
    assert decl["ofdm_ber_sweep_task4_nmse"] == decl["ofdm_ber_sweep_task4_ex"] + 2 == 27
    assert decl["ofdm_ber_sweep_task4_fading"] == decl["ofdm_ber_sweep_task4_nmse"] + 1 == 28


def test_python_layer_has_the_new_keywords():
    from ofdm_course_amd import api
    p = inspect.signature(api.RxPlan.ber_sweep_task4).parameters
    assert p["fading"].default is None and p["want_nmse"].default is False and p["want_frame_nmse"].default is False
    src = inspect.getsource(api.RxPlan.tx_frames_fused)
    assert "does not combine with Time_Delay" not in src
    assert "ofdm_tx_frames_fading_ex" in inspect.getsource(api.RxPlan)


def test_driver_imports_and_has_the_options():
    from ofdm_course_amd.drivers import task4_mer, task4_nmse
    p = inspect.signature(task4_nmse.run).parameters
    assert p["fading"].default is None and p["sync"].default is False
    assert p["Percent_pilot"].default == 15 and p["frames_per_point"].default == 8
    q = inspect.signature(task4_mer.run).parameters                       # the sibling's geometry defaults
    for k in ("Nfft", "N_carrier", "Amount_OFDM_Frames", "Amount_ODFM_SpF", "Constellation", "precision"):
        assert p[k].default == q[k].default, k
