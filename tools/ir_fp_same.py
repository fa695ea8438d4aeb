#!/usr/bin/env python3
"""Same rounding?  Compares the floating-point dataflow of kernels in two optimised IR files, operand order included where it
decides a contraction: equal instruction counts (tools/isa_counts.py) do not tell which of two products the backend fuses into
an fma -- it takes the FIRST fmul operand of an fadd, and that order is set by the passes (Reassociate's ranks, SLP) in whatever
function the expression lived in when they ran (profiles/lpl_steps_isa.txt).
Every value gets a hash of its opcode and its operands' hashes.  Leaves: loads, extractelement, phi, arguments.  Operands of
fadd / fmul are sorted (commuting them is exact) EXCEPT for an fadd of two fmuls, the contraction-sensitive case.

usage: hipcc --offload-arch=gfx950 <CXXFLAGS> --cuda-device-only -S -emit-llvm -o old.ll unit.hip   (on both trees), then
       ir_fp_same.py old.ll new.ll [kernel name pattern] [examples to print]      exit status 1 if a kernel differs"""
import collections
import hashlib
import re
import sys

sys.setrecursionlimit(100000)
FP = re.compile(r"^(fmul|fadd|fsub|fdiv|fneg|.*call.*@llvm\.(fma|sqrt|fabs|amdgcn\.(rcp|rsq|div|fmed|trig|frexp|ldexp)))")


def kernels(path):
    s, out = open(path).read(), {}
    for m in re.finditer(r"define protected amdgpu_kernel void @(\w+)\(", s):
        out[m.group(1)] = s[m.start():s.index("\n}\n", m.start())]
    return out


def analyse(text):
    defs, order, memo = {}, [], {}
    for line in text.split("\n"):
        m = re.match(r"(%[\w.]+) = (.*)", line.strip())
        if m:
            defs[m.group(1)] = re.sub(r", align \d+", "", re.sub(r", ![\w.]+ ![\w.]+", "", m.group(2)))
            order.append(m.group(1))

    def h(v):
        if v in memo:
            return memo[v]
        if v not in defs:
            return v
        rhs = defs[v]
        if rhs.startswith(("phi", "extractelement")):
            memo[v] = "LEAF"
        elif rhs.startswith("load"):
            memo[v] = "LOAD " + rhs.split(",")[0]
        else:
            memo[v] = "CYCLE"
            ops = re.findall(r"%[\w.]+", rhs)
            if re.match(r"(fadd|fmul) ", rhs) and len(ops) == 2:
                ordered = rhs.startswith("fadd") and all(o in defs and defs[o].startswith("fmul") for o in ops)
                hs = [h(o) for o in ops]
                txt = rhs.split("%")[0] + " ".join(hs if ordered else sorted(hs)) + (" ORDERED" if ordered else "")
            else:
                txt = re.sub(r"%[\w.]+", lambda m: h(m.group(0)), rhs)
            memo[v] = hashlib.md5(txt.encode()).hexdigest()[:10]
        return memo[v]

    return defs, [(v, h(v)) for v in order if FP.match(defs[v])]


def show(defs, v, depth):
    if v not in defs or depth == 0:
        return v
    rhs = defs[v]
    if rhs.startswith(("phi", "load")):
        return rhs.split()[0]
    rhs = re.sub(r"\b(contract|double|noundef|tail call)\b ?", "", rhs)
    return "(" + re.sub(r"%[\w.]+", lambda m: show(defs, m.group(0), depth - 1), rhs) + ")"


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    pat = sys.argv[3] if len(sys.argv) > 3 else "."
    examples = int(sys.argv[4]) if len(sys.argv) > 4 else 0
    bad = 0
    for n in sorted(set(a) & set(b)):
        if not re.search(pat, n):
            continue
        (da, fa), (db, fb) = analyse(a[n]), analyse(b[n])
        ca, cb = collections.Counter(x for _, x in fa), collections.Counter(x for _, x in fb)
        only_a, only_b = ca - cb, cb - ca
        bad += bool(only_a or only_b)
        print(f"{n:46s} fp values {len(fa)} / {len(fb)}  only old {sum(only_a.values())}  only new {sum(only_b.values())}")
        for side, d, f, only in (("old", da, fa, only_a), ("new", db, fb, only_b)):
            for v, x in [t for t in f if t[1] in only][:examples]:
                print("   ", side, v, show(d, v, 3)[:220])
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
