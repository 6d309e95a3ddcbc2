#!/usr/bin/env python
"""The LDS read forms of every kernel in libagp_hip.so, from the device assembly.

    python tools/lds_read_forms.py [--out profiles/r15_lds_read_forms.txt] [--asm FILE]
    python tools/lds_read_forms.py --asm RESULT.s --against PARENT.s --compare-out FILE

Compiles csrc/agp_capi.hip as tools/kernel_resources.py does, with --cuda-device-only -S (cross-compiles for gfx950 without a GPU,
~2 min; `--asm FILE` reads an assembly produced earlier) and writes one row per kernel: the number of ds_read_b64, ds_read_b128,
ds_read2st64_b64, and of ds_read2_b64 by the distance |offset1 - offset0| of its two offsets (in 8-byte units).  Why the form matters
(DESIGN.md section 5 "round 14" and "round 15"): a ds_read2_b64 serves 16 lanes per LDS cycle and banks modulo 32; with the MFMA
operand layout of the Cholesky kernels (row stride LDP = 66 doubles, two neighbouring k-steps 4 doubles apart) a pair of distance 4
costs 16 LDS cycles where two ds_read_b64 cost 4.  tests/test_lds_read_forms.py reads the committed table and fails when a fp64
Cholesky kernel has such a pair again.

`--against` compares two assemblies kernel by kernel (instruction sequences with the labels renamed) and writes the kernels named
by --compare-filter (a regular expression on the short kernel name) plus every kernel that differs.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

DIST_COLS = (1, 2, 4, 8)  # ds_read2_b64 distances with a column of their own; every other distance is counted under "other"


def compile_asm():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "agp.s")
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", out, KR.SRC]
        print("[lds_read_forms]", " ".join(cmd), file=sys.stderr, flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit(r.returncode)
        return open(out).read()


def kernels(text):
    """device assembly -> {mangled kernel name: [instruction lines, labels renamed]} (functions that are no kernels are left out)"""
    funcs, cur, is_kernel = {}, None, set()
    for line in text.splitlines():
        m = re.match(r"^([A-Za-z_][\w$.]*):\s*; @\1\s*$", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
            continue
        s = line.strip()
        if s.startswith(".amdhsa_kernel "):
            is_kernel.add(s.split()[1])
        if s.startswith(".Lfunc_end"):
            cur = None
        if cur is None or not s or s[0] in ".;" or s.endswith(":") or not re.match(r"^[a-z]", s):
            continue
        s = s.split(";", 1)[0].strip()
        cur.append(re.sub(r"\.LBB\d+_\d+", ".LBB", re.sub(r"\s+", " ", s)))
    return {k: v for k, v in funcs.items() if k in is_kernel}


def read_forms(instrs):
    """-> dict(b64, b128, st64, and d<distance> for the ds_read2_b64)"""
    c = {"b64": 0, "b128": 0, "st64": 0}
    for s in instrs:
        op = s.split(" ", 1)[0]
        if op == "ds_read_b64":
            c["b64"] += 1
        elif op == "ds_read_b128":
            c["b128"] += 1
        elif op == "ds_read2st64_b64":
            c["st64"] += 1
        elif op == "ds_read2_b64":
            o0 = re.search(r"offset0:(\d+)", s)
            o1 = re.search(r"offset1:(\d+)", s)
            d = abs((int(o1.group(1)) if o1 else 0) - (int(o0.group(1)) if o0 else 0))
            key = f"d{d}" if d in DIST_COLS else "other"
            c[key] = c.get(key, 0) + 1
    return c


def short_names(mangled):
    return [KR.short(n) for n in KR.demangle(list(mangled))]


def table(asm):
    ks = kernels(asm)
    names = dict(zip(ks, short_names(ks)))
    rows = sorted(((names[k], read_forms(v)) for k, v in ks.items()), key=lambda r: r[0])
    w = max(len(n) for n, _ in rows)
    cols = [("b64", "b64"), ("b128", "b128"), ("st64", "2st64")] + [(f"d{d}", f"2@{d}") for d in DIST_COLS] + [("other", "2@oth")]
    head = f"{'kernel':<{w}}  " + " ".join(f"{t:>6}" for _, t in cols)
    lines = [head, "-" * len(head)]
    for n, c in rows:
        lines.append(f"{n:<{w}}  " + " ".join(f"{c.get(k, 0):>6}" for k, _ in cols))
    lines += ["", f"{len(rows)} kernels, {sum(1 for _, c in rows if c.get('d4', 0))} with a ds_read2_b64 of distance 4"]
    return "\n".join(lines) + "\n"


def read_table(path):
    """the committed table -> {kernel: dict(b64, b128, st64, d1, d2, d4, d8, other)} (+ key "_sha256": the sources' hash)"""
    out = {}
    keys = ["b64", "b128", "st64"] + [f"d{d}" for d in DIST_COLS] + ["other"]
    with open(path) as fh:
        for line in fh:
            if line.startswith("# sources sha256:"):
                out["_sha256"] = line.split(":", 1)[1].strip()
            m = re.match(r"^(k_\S.*?)\s{2,}(\d+(?:\s+\d+){%d})\s*$" % (len(keys) - 1), line)
            if m:
                out[m.group(1)] = dict(zip(keys, map(int, m.group(2).split())))
    return out


def compare(asm_parent, asm_result, pattern):
    """parent against result, kernel by kernel -> text"""
    kp, kr = kernels(asm_parent), kernels(asm_result)
    names = dict(zip(list(kp) + [k for k in kr if k not in kp], short_names(list(kp) + [k for k in kr if k not in kp])))
    allk = sorted(names, key=lambda k: names[k])
    differ = [k for k in allk if kp.get(k) != kr.get(k)]
    w = max(len(names[k]) for k in allk)
    lines = [f"{len(allk)} kernels, {len(differ)} with a changed instruction sequence"]

    def counts(ins):
        c = read_forms(ins)
        pre = lambda p: sum(1 for s in ins if s.startswith(p))
        return (f"ds_read_b64={c['b64']} ds_read2_b64@4={c.get('d4', 0)} ds_read2_b64@8={c.get('d8', 0)} ds_read(all)={pre('ds_read')} "
                f"ds_write={pre('ds_write')} v_mfma={pre('v_mfma')} s_barrier={pre('s_barrier')} global_load={pre('global_load')} "
                f"global_store={pre('global_store')}")

    for k in allk:
        if not (k in differ or re.search(pattern, names[k])):
            continue
        a, b = kp.get(k), kr.get(k)
        same = "identical sequence" if a == b else "differs"
        lines.append(f"{names[k]:<{w}}  parent {len(a or []):>6}  result {len(b or []):>6} instructions  {same}")
        if a != b:
            lines.append("    parent  " + (counts(a) if a is not None else "absent"))
            lines.append("    result  " + (counts(b) if b is not None else "absent"))
    fl = [k for k in allk if "float" in names[k]]
    lines.append(f"{len(fl)} kernels with float in their name, {sum(1 for k in fl if k in differ)} of them differ")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_lds_read_forms.txt"))
    ap.add_argument("--asm", default=None)
    ap.add_argument("--against", default=None, help="the parent's assembly: compare instead of writing the table")
    ap.add_argument("--compare-out", default=None)
    ap.add_argument("--compare-filter", default=r"^k_chol_|^k_diag_bench|^k_safe_")
    a = ap.parse_args()
    asm = open(a.asm).read() if a.asm else compile_asm()
    if a.against:
        text = compare(open(a.against).read(), asm, a.compare_filter)
        if a.compare_out:
            with open(a.compare_out, "w") as fh:
                fh.write(text)
        print(text.splitlines()[0])
        return
    tab = table(asm)
    hdr = ("# LDS read forms of every kernel of libagp_hip.so: hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S\n"
           "# (tools/lds_read_forms.py; b64 = ds_read_b64, b128 = ds_read_b128, 2st64 = ds_read2st64_b64, 2@d = ds_read2_b64 whose two\n"
           "# offsets are d 8-byte units apart, 2@oth = every other distance)\n"
           f"# sources sha256: {KR.source_hash()}\n")
    with open(a.out, "w") as fh:
        fh.write(hdr + tab)
    print(tab.splitlines()[-1], "->", a.out)


if __name__ == "__main__":
    main()
