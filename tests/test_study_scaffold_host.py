"""The studies' scaffold, read as source text (no compiler, no GPU): every study entry generates its frames through the one
point x chunk loop of csrc/txf_study.hpp, and every study's plan header makes the shared front of its checks through
txf_study_prelude of csrc/txf_plan.hpp -- none carries a copy of either."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ofdm-course_amd", "csrc")

STUDIES = ["ofdm_spectrum.hip", "ofdm_sync_study.hip", "ofdm_fine_study.hip", "ofdm_ifo_study.hip", "ofdm_hest_study.hip",
           "ofdm_error_study.hip"]
HEADERS = ["spectrum_plan.hpp", "sync_plan.hpp", "fine_plan.hpp", "ifo_plan.hpp", "hest_plan.hpp"]
# the format strings of the shared front (txf_check_args, txf_check_sweep, txf_check_modes, the register, h and taps together)
SHARED = ["%s: bad arguments", "%s: snr_db / seeds missing", "%s: too many points", "%s: sto_mode / cfo_mode must be 0, 1 or 2",
          "%s: register entries must be 0 or 1", "%s: give h (one channel for every frame) or taps (a channel per frame), not both"]


def _read(name):
    return open(os.path.join(CSRC, name)).read()


def _code(text):
    """The text without its // comments."""
    return re.sub(r"//[^\n]*", "", text)


def test_the_studies_share_one_scaffold():
    for name in STUDIES:                                                   # a study entry generates through the shared loop
        code = _code(_read(name))
        assert '#include "txf_study.hpp"' in code, name
        assert "txf_sweep_points(" in code and "TxfStudyArgs" in code, name
        assert "txf_generate(" not in code and "txf_workspace(" not in code and "tx_dict_device(" not in code, name
        assert not re.search(r"c0\s*\+=\s*CH", code), name
        assert "tabs[]" not in code and "auto table = " not in code, name  # the tables: txf_table
    for name in HEADERS:                                                   # a plan header makes the shared front through one call
        src = _read(name)
        assert "txf_study_prelude(" in _code(src), name
        for fmt in SHARED:
            assert f'"{fmt}"' not in src, (name, fmt)
        for fn in ("txf_check_sweep(", "txf_check_modes(", "txf_call_channel("):
            assert fn not in _code(src), (name, fn)
    study = _code(_read("txf_study.hpp"))                                  # the scaffold holds the one loop ...
    assert study.count("txf_generate(") == 1 and len(re.findall(r"c0\s*\+=\s*CH", study)) == 1
    assert "__global__" not in study and "__device__" not in study        # (host code only)
    plan = _read("txf_plan.hpp")                                           # ... and txf_plan.hpp the shared texts
    for fmt in SHARED:
        assert f'"{fmt}"' in plan, fmt
    assert "inline int txf_study_prelude(" in plan and "inline TxfUse txf_study_use(" in plan
    sweep = _code(_read("ofdm_ber_sweep.hip"))                             # the BER sweeps: the same loop, no copy of it
    assert '#include "txf_study.hpp"' in sweep and "txf_sweep_points(" in sweep and "txf_generate(" not in sweep
    # ... and one density accumulator for both: the plan's buffer grows in one place, a receiver call's capture is made in one
    for once in ("pl->ws_scope_bytes <", "hipMalloc(&pl->ws_scope", "scope_scale("):
        assert sweep.count(once) == 1, once
