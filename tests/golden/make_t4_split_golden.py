"""Writes tests/golden/t4_split_parent.json: what rx_chain_task4 and ber_sweep_task4 return for the runs of tests/t4_split_cases.py,
through the public calls only.  Run on the commit BEFORE task4_run was split (needs a GPU); every run is made twice and the file
lists the fields that agreed between the two on every run -- the ones tests/test_gpu_task4_split_parent.py compares bit for bit.

    python tests/golden/make_t4_split_golden.py [--out tests/golden/t4_split_parent.json]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import t4_split_cases as ts  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(HERE, "t4_split_parent.json"))
    a = ap.parse_args()
    import ofdm_course_amd as ofdm
    from oracle import ofdm_oracle as oracle
    ofdm.init()
    runs, stable = {}, set(ts.FIELDS)
    for run in ts.RUNS:
        first, second = ts.record(ofdm, oracle, run), ts.record(ofdm, oracle, run)
        stable -= {f for f in ts.FIELDS if first[f] != second[f]}
        runs[ts.run_id(run)] = first
    fields = [f for f in ts.FIELDS if f in stable]
    with open(a.out, "w") as fh:
        json.dump({"fields": fields, "runs": {k: {f: v[f] for f in fields} for k, v in runs.items()}}, fh, indent=0, sort_keys=True)
    print(f"{len(runs)} runs, fields kept: {fields}; not repeatable: {sorted(set(ts.FIELDS) - stable)}", flush=True)


if __name__ == "__main__":
    main()
