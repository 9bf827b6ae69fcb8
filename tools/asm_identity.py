"""Instruction and descriptor identity of the kernels two source trees have in common (CPU only).

usage: python tools/asm_identity.py <old csrc dir> <new csrc dir> [file.hip | old1.hip,old2.hip=new1.hip,new2.hip ...]

Each .hip file is compiled device-only to gfx950 assembly (hipcc -S, the library's flags) from both trees.  Every kernel
of the old tree must have a twin in the new one with the same demangled name (an empty trailing template pack adds
nothing to it) whose instructions and `.amdhsa_kernel` descriptor are identical; label numbers, comments and the mangled
names are ignored.  Kernels only the new tree has are listed.  Each tree's csrc must sit two levels below its include/
(as in the repository: <tree>/ofdm-course_amd/csrc, <tree>/include).  Exit status 1 on any difference."""
import concurrent.futures as cf
import os
import re
import subprocess
import sys
import tempfile

FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=fast", "-fno-slp-vectorize",
         "-Wno-pass-failed", "-Wno-logical-op-parentheses", "--cuda-device-only", "-S"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
DEFAULT = ["ofdm_chain.hip", "ofdm_chain_fast.hip", "ofdm_chain_wave.hip", "ofdm_chain_coop.hip", "ofdm_chain_split.hip",
           "ofdm_txfused.hip", "ofdm_ber_sweep.hip"]


def _asm(csrc, name, out):
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(csrc))), "include")
    r = subprocess.run([HIPCC, *FLAGS, "-I" + inc, os.path.join(csrc, name), "-o", out], capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"hipcc failed for {csrc}/{name}:\n{r.stderr}")
    return open(out).read()


def _demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, r.stdout.splitlines()))


def _kernels(text):
    """mangled name -> (normalised body, normalised descriptor)"""
    bodies, descs = {}, {}
    for m in re.finditer(r"^(_Z\S+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        bodies[m.group(1)] = m.group(2)
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M):
        descs[m.group(1)] = m.group(2)
    out = {}
    for name, desc in descs.items():
        if name not in bodies:
            continue
        norm = lambda s: "\n".join(l for l in (re.sub(r";.*", "", x).rstrip() for x in
                                               re.sub(r"\.L\w+?\d+(_\d+)?", ".L", s.replace(name, "K")).splitlines()) if l)
        out[name] = (norm(bodies[name]), norm(desc))
    return out


def _pool(jobs, tree, names):
    """The kernels of several files as one table; a kernel instantiated in two of them must be the same in both."""
    pool = {}
    for f in names:
        for k, v in _kernels(jobs[tree, f].result()).items():
            if pool.setdefault(k, v) != v:
                sys.exit(f"{tree} {f}: {_demangle([k])[k]} differs from its instance in another file of the pool")
    return pool


def main():
    old, new, files = sys.argv[1], sys.argv[2], sys.argv[3:] or DEFAULT
    # `a.hip,b.hip=a.hip,c.hip`: the kernels of the old files (left) pooled against those of the new files (right)
    pairs = [tuple(side.split(",") for side in (f.split("=") if "=" in f else (f, f))) for f in files]
    bad = 0
    with tempfile.TemporaryDirectory() as td, cf.ThreadPoolExecutor(max_workers=8) as ex:
        jobs = {(t, f): ex.submit(_asm, d, f, os.path.join(td, f"{t}_{f}.s"))
                for t, d, i in (("old", old, 0), ("new", new, 1)) for p in pairs for f in p[i]}
        for fo, fn in pairs:
            f = ",".join(fn)
            ko, kn = _pool(jobs, "old", fo), _pool(jobs, "new", fn)
            do, dn = _demangle(list(ko)), _demangle(list(kn))
            by_name = {dn[k]: k for k in kn}
            same = 0
            for k, (body, desc) in ko.items():
                twin = by_name.pop(do[k], None)
                if twin is None:
                    print(f"{f}: MISSING {do[k]}")
                    bad += 1
                elif kn[twin] != (body, desc):
                    print(f"{f}: DIFFERS {do[k]} ({'instructions' if kn[twin][0] != body else 'descriptor'})")
                    bad += 1
                else:
                    same += 1
            print(f"{f}: {same} of {len(ko)} kernels identical; new: {len(by_name)}", flush=True)
            for name in sorted(by_name):
                print(f"    + {name}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
