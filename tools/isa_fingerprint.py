#!/usr/bin/env python3
"""Per-kernel fingerprint of the decoder translation units' device code, for refactors that must not change it.

Each unit is compiled to device-only assembly with the shipped flags (-S --cuda-device-only plus build_native's FLAGS and
TU_FLAGS: the build's own lists, so the tool cannot drift from it).  Every kernel (.amdhsa_kernel NAME) is cut from its label to its last
s_endpgm and hashed.  Two compiles of the same source differ only in the __hip_cuid_* symbol at the end of the file, so the
cut text is reproducible.  Comments are dropped, and so is the function number the compiler puts into local labels
(.LBB<f>_<b>): both only say where in the file the function stands.

  tools/isa_fingerprint.py --out after.json                 # compile the tree this script lives in, write the table
  tools/isa_fingerprint.py --csrc OTHER/alignsdf_amd/csrc --out before.json
  tools/isa_fingerprint.py --compare before.json after.json # exit status 1 unless every kernel is on both sides, identical
"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from alignsdf_amd.build_native import FLAGS, HIPCC, TU_FLAGS     # noqa: E402

# the sweep units and every unit that carries the fp32 chain (gradient, projection, tracing, reverse mode and its batched loss form)
UNITS = ["decoder.hip", "k1_kernels.hip", "k1pa_kernels.hip", "k1_cls_kernels.hip", "k1h_kernels.hip", "k1hw_kernels.hip",
         "k1h_nerf_kernels.hip", "k1s_kernels.hip", "k1s_nerf_kernels.hip",
         "k1g_kernels.hip", "k1p_kernels.hip", "k1t_kernels.hip", "k1v_kernels.hip", "k1vb_kernels.hip"]


def cut_kernels(isa):
    """{kernel name: text from its label to its last s_endpgm}"""
    out = {}
    lines = isa.splitlines()
    at = {m.group(1): i for i, m in ((i, re.match(r"([A-Za-z_]\w*):", l)) for i, l in enumerate(lines)) if m}
    for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", isa, flags=re.M):
        first = at[name]
        end = next(i for i in range(first, len(lines)) if lines[i].startswith(".Lfunc_end"))
        last = max(i for i in range(first, end) if lines[i].split(";")[0].strip() == "s_endpgm")
        body = [l.split(";")[0].rstrip() for l in lines[first:last + 1]]
        out[name] = re.sub(r"\.LBB\d+_", ".LBB_", "\n".join(l for l in body if l))
    return out


def fingerprint(csrc, asm_dir=None):
    table = {}
    with tempfile.TemporaryDirectory() as tmp:
        tmp = asm_dir or tmp
        procs = [(u, subprocess.Popen([HIPCC, *FLAGS, *TU_FLAGS.get(u, []), "-S", "--cuda-device-only", u, "-o", os.path.join(tmp, u + ".s")], cwd=csrc, stderr=subprocess.PIPE, text=True))
                 for u in UNITS]
        for u, proc in procs:
            _, err = proc.communicate()
            if proc.returncode != 0:
                sys.exit("%s: %s" % (u, err[-2000:]))
            with open(os.path.join(tmp, u + ".s")) as f:
                for name, body in cut_kernels(f.read()).items():
                    table[u + ":" + name] = {"sha256": hashlib.sha256(body.encode()).hexdigest(), "lines": body.count("\n") + 1}
    return table


def compare(a, b):
    bad = 0
    for k in sorted(set(a) | set(b)):
        state = "missing before" if k not in a else "missing after" if k not in b else "same" if a[k] == b[k] else "DIFFERENT"
        bad += state != "same"
        print("%-9s %s %s" % (state, (a.get(k) or b[k])["sha256"][:12], k))
    print("%d kernels, %d not identical" % (len(set(a) | set(b)), bad))
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--csrc", default=os.path.join(ROOT, "alignsdf_amd", "csrc"))
    ap.add_argument("--out")
    ap.add_argument("--asm-dir", help="keep the assembly files here")
    ap.add_argument("--compare", nargs=2, metavar=("BEFORE", "AFTER"))
    args = ap.parse_args()
    if args.compare:
        with open(args.compare[0]) as fa, open(args.compare[1]) as fb:
            sys.exit(1 if compare(json.load(fa), json.load(fb)) else 0)
    table = fingerprint(args.csrc, args.asm_dir)
    for k in sorted(table):
        print(table[k]["sha256"][:12], "%6d" % table[k]["lines"], k)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
