#!/usr/bin/env python3
"""Which chain kernels did tests/test_gpu_chain_routes.py really launch?

    rocprofv3 --kernel-trace --stats -d DIR -o routes --output-format csv -- \\
        python -m pytest tests/test_gpu_chain_routes.py -m gpu
    python tools/route_coverage.py DIR/**/routes_kernel_stats.csv -o profiles/routes/coverage.json

Reads the kernel names of the stats (or trace) CSV, demangles them, and compares them with
  * the symbol-stage instantiation that tests/routes.py predicts for every case (a predicted kernel that was not launched,
    or a launched symbol-stage kernel that no case predicts, is a bug in the model or in the dispatcher), and
  * the chain kernel instantiations present in libofdm_mi355x.so (the host stubs of the library's symbol table).
The trace carries no test boundaries, so kernels are attributed to the module as a whole, not to single cases.
Exit status 1 when a predicted kernel is missing or a template parameter value of a chain kernel was never launched.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

CHAIN_FAMILIES = ("rx_chain_kernel", "rx_pilot_kernel", "rx_pilot_omp_kernel", "omp_batch_kernel", "rx_symbols_kernel",
                  "rx_symbols_wave_kernel", "rx_symbols_coop4_kernel", "rx_symbols_r2_kernel", "eq_demap_kernel",
                  "pilot_ls_kernel", "descr_pass_kernel", "mmse_fused_kernel", "mmse_apply_mfma_kernel",
                  "mmse_apply_valu_kernel", "spline_band_kernel", "demod_keep8192_kernel", "demod_keep_kernel")

# Template parameter values that this module does not launch, with the reason
REASONS = [
    # (family, position, values, reason)
    ("rx_symbols_wave_kernel", 3, {"1"}, "ABL = 1 is built only with -DOFDM_DIAG (ofdm_chain_wave.hip:499-501)"),
    ("demod_keep_kernel", 1, {"64", "128", "256", "512", "1024", "2048", "4096", "8192"},
     "one instantiation per Nfft; the split form reaches it at Nfft 64 / 128 / 256 / 512 (MMSE mode, 48 Ki decisions) and at "
     "8192 under OFDM_SPLIT_GENERIC_FFT; Nfft 1024 / 2048 / 4096 need > 48 Ki decisions per frame, not oracle-sized"),
    ("rx_chain_kernel", 1, {"512", "1024", "4096"},
     "one instantiation per Nfft; the generic kernel is the natural route below 512 and with out-of-band pilots (256, 2048 "
     "here) and forced at 1024; these sizes run in tests/test_gpu_chain.py::test_chain_matches_oracle[generic]"),
    ("rx_chain_kernel", 1, {"8192"},
     "reachable only with an out-of-band pilot or OFDM_CHAIN_GENERIC at Nfft 8192; no test launches it (open)"),
    ("rx_pilot_omp_kernel", 3, {"2", "6", "8"},
     "RT = register-resident picks (2 / 4 / 6 / 8): tests/test_gpu_chain.py::test_chain_comb_pilot_stage covers every bucket"),
]


def normalise(name: str) -> str:
    n = name.strip().strip('"')
    n = re.sub(r"\s*\[clone .*\]$", "", n)
    n = re.sub(r"\.kd$", "", n)
    n = re.sub(r"^void ", "", n)
    depth, cut = 0, len(n)
    for i, ch in enumerate(n):                       # cut the parameter list: the first '(' outside <>
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            cut = i
            break
    n = n[:cut]
    return n.replace("ofdm::__device_stub__", "").replace("ofdm::", "").replace(" ", "")


def demangle(names):
    mangled = [n for n in names if n.startswith("_Z")]
    if not mangled:
        return list(names)
    out = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.split("\n")
    table = dict(zip(mangled, out))
    return [table.get(n, n) for n in names]


def launched_kernels(paths):
    calls = {}
    for p in paths:
        with open(p, newline="") as fh:
            rd = csv.DictReader(fh)
            col = "Name" if "Name" in rd.fieldnames else "Kernel_Name"
            rows = list(rd)
        names = demangle([r[col] for r in rows])
        for r, n in zip(rows, names):
            k = normalise(n)
            calls[k] = calls.get(k, 0) + int(r.get("Calls", 1) or 1)
    return calls


def library_kernels(lib):
    out = subprocess.run(["nm", "-C", lib], capture_output=True, text=True, check=True).stdout
    ks = set()
    for line in out.splitlines():
        if "__device_stub__" in line:
            ks.add(normalise(line.split(" ", 2)[2]))
    return ks


def family(k):
    return k.split("<")[0]


def targs(k):
    if "<" not in k:
        return []
    body, depth, cur, out = k[k.index("<") + 1:-1], 0, "", []
    for ch in body:
        if ch == "," and depth == 0:
            out.append(cur)
            cur = ""
            continue
        depth += ch == "<"
        depth -= ch == ">"
        cur += ch
    return out + [cur]


def predicted_symbol_kernel(case):
    """The symbol-stage instantiation of a case, from its modelled route."""
    r = case.route()
    T = "double" if case.precision == "fp64" else "float"
    b = lambda v: "true" if v else "false"
    hx = case.mode == "mmse"
    s = r.symbols
    if s == "chain_generic":
        return f"rx_chain_kernel<{T},{case.nfft}" + (",MerSums>" if r.mer else ">")
    if s.startswith("rx_symbols<"):
        nw, pr = s[len("rx_symbols<"):-1].split(",")
        return f"rx_symbols_kernel<{T},{nw},{pr},{r.ba},{b(hx)}" + (",MerSums>" if r.mer else ">")
    if s.startswith("wave<"):
        form = {"exact": "0,0", "skip0": "2,1", "skip02": "2,5", "none": "2,0"}[s[5:-1]]
        return f"rx_symbols_wave_kernel<{r.ba},{b(hx)},4,0,true,{form},{b(r.descr == 'in_kernel')}" + (",MerSums>" if r.mer else ">")
    if s in ("coop4", "r2"):
        return f"rx_symbols_{s}_kernel<{r.ba},{b(hx)}" + (",MerSums>" if r.mer else ">")
    vec = s == "eq_demap<vec>"
    return f"eq_demap_kernel<{T},{r.ba},{b(hx)},{b(vec)}" + (",MerOut>" if r.mer else ">")


SYMBOL_FAMILIES = ("rx_chain_kernel", "rx_symbols_kernel", "rx_symbols_wave_kernel", "rx_symbols_coop4_kernel",
                   "rx_symbols_r2_kernel", "eq_demap_kernel")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("csv", nargs="+", help="rocprofv3 kernel stats / kernel trace CSV of the routes module")
    ap.add_argument("--lib", default=os.path.join(ROOT, "ofdm-course_amd", "libofdm_mi355x.so"))
    ap.add_argument("-o", "--out", default=None)
    a = ap.parse_args()
    import routes

    calls = {k: v for k, v in launched_kernels(a.csv).items() if family(k) in CHAIN_FAMILIES}
    lib = {k for k in library_kernels(a.lib) if family(k) in CHAIN_FAMILIES}
    launched = set(calls)
    predicted = {}
    import dataclasses
    for c in routes.CASES:
        predicted.setdefault(predicted_symbol_kernel(c), []).append(c.name)
        if c.base_env is not None:                   # the route the switch case is compared with
            predicted.setdefault(predicted_symbol_kernel(dataclasses.replace(c, env=c.base_env)), []).append(c.name + " (base)")
    for c, env in ((c, e) for c in routes.REFUSALS for e in [routes.REFUSAL_FOLLOW_UP[c.name]]):   # the call after the refusal
        predicted.setdefault(predicted_symbol_kernel(dataclasses.replace(c, **env)), []).append(c.name + " (afterwards)")
    missing = sorted(k for k in predicted if k not in launched)
    unpredicted = sorted(k for k in launched if family(k) in SYMBOL_FAMILIES and k not in predicted)
    not_in_lib = sorted(launched - lib)

    never = sorted(lib - launched)
    # per family and template parameter position: the values the library holds that were never launched
    uncovered, explained = [], []
    for fam in CHAIN_FAMILIES:
        have = [targs(k) for k in lib if family(k) == fam]
        got = [targs(k) for k in launched if family(k) == fam]
        if not have:
            continue
        for pos in range(max(len(t) for t in have)):
            hv = {t[pos] if pos < len(t) else "-" for t in have}
            gv = {t[pos] if pos < len(t) else "-" for t in got}
            for v in sorted(hv - gv):
                why = next((r for f, p, vals, r in REASONS if f == fam and p == pos and v in vals), None)
                (explained if why else uncovered).append(dict(family=fam, position=pos, value=v, reason=why))
    by_family = {}
    for k in never:
        by_family.setdefault(family(k), []).append(k)
    report = dict(
        launched={k: calls[k] for k in sorted(calls)},
        predicted_symbol_kernels={k: v for k, v in sorted(predicted.items())},
        predicted_but_not_launched=missing,
        launched_symbol_kernels_no_case_predicts=unpredicted,
        launched_but_not_in_library=not_in_lib,
        library_chain_instantiations=len(lib),
        never_launched_count={f: len(v) for f, v in sorted(by_family.items())},
        never_launched=by_family,
        never_launched_reason=("cross product of template parameters: every value of every template parameter of the family was "
                               "launched at least once by this module, except the values listed under "
                               "parameter_values_never_launched with their reason"),
        parameter_values_never_launched=explained,
        parameter_values_never_launched_without_reason=uncovered)
    text = json.dumps(report, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(f"{len(launched)} of {len(lib)} chain kernel instantiations launched; {len(missing)} predicted but not launched, "
          f"{len(unpredicted)} launched symbol kernels no case predicts, {len(uncovered)} template parameter values never launched "
          f"without a written reason")
    for k in missing:
        print("  predicted, not launched:", k, predicted[k])
    for k in unpredicted:
        print("  launched, not predicted:", k)
    for u in uncovered:
        print("  never launched:", u)
    return 1 if (missing or uncovered) else 0


if __name__ == "__main__":
    sys.exit(main())
