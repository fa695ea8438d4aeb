#!/usr/bin/env python3
"""Same rounding?  Compares the floating-point dataflow of kernels in two optimised IR files, operand order included where it
decides a contraction: equal instruction counts (tools/isa_counts.py) do not tell which of two products the backend fuses into
an fma -- it takes the FIRST fmul operand of an fadd, and that order is set by the passes (Reassociate's ranks, SLP) in whatever
function the expression lived in when they ran (profiles/lpl_steps_isa.txt).
Every value gets a hash of its opcode and its operands' hashes.  Leaves: loads, extractelement, phi, arguments.  Operands of
fadd / fmul are sorted (commuting them is exact) EXCEPT for an fadd of two fmuls, the contraction-sensitive case.

Kernels of any linkage are listed (the POVAR_KERNEL ones are static: plain `define amdgpu_kernel`), and an MFMA call is a
floating-point value like any other call: its operands (A, B, accumulator) hash in their order.
A kernel that was renamed is paired through --map OLD=NEW, substrings that single out its old and its new (mangled) name, e.g.
--map lm_covILi12E=lm_covINS_7ScdPoseE; a kernel left without a partner on either side is reported and counts as different.

usage: hipcc --offload-arch=gfx950 <CXXFLAGS> --cuda-device-only -S -emit-llvm -o old.ll unit.hip   (on both trees), then
       ir_fp_same.py [--map OLD=NEW]... old.ll new.ll [kernel name pattern] [examples to print]
exit status 1 if a kernel differs"""
import collections
import hashlib
import re
import sys

sys.setrecursionlimit(100000)
FP = re.compile(r"^(fmul|fadd|fsub|fdiv|fneg|.*call.*@llvm\.(fma|sqrt|fabs|amdgcn\.(rcp|rsq|div|fmed|trig|frexp|ldexp|mfma)))")


def kernels(path):
    s, out = open(path).read(), {}
    for m in re.finditer(r"define (?:[\w()]+ )*amdgpu_kernel void @(\w+)\(", s):
        out[m.group(1)] = s[m.start():s.index("\n}\n", m.start())]
    return out


def analyse(text):
    defs, order, memo = {}, [], {}
    for line in text.split("\n"):
        m = re.match(r"(%[\w.]+) = (.*)", line.strip())
        if m:
            # (metadata, alignment and the module-wide numbers of attribute groups are not dataflow)
            defs[m.group(1)] = re.sub(r", align \d+| #\d+", "", re.sub(r", ![\w.]+ ![\w.]+", "", m.group(2)))
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
    argv, renames = sys.argv[1:], []
    while argv and argv[0] == "--map":
        renames.append(argv[1].split("=", 1))
        argv = argv[2:]
    a, b = kernels(argv[0]), kernels(argv[1])
    pat = argv[2] if len(argv) > 2 else "."
    examples = int(argv[3]) if len(argv) > 3 else 0

    for old, new in renames:  # the one old kernel whose name contains OLD takes the name of the one new kernel that contains NEW
        was, now = [n for n in a if old in n], [n for n in b if new in n]
        if len(was) != 1 or len(now) != 1:
            sys.exit(f"--map {old}={new}: matches {len(was)} old and {len(now)} new kernels, need one of each")
        a[now[0]] = a.pop(was[0])
    bad = 0
    for n in sorted(set(a) ^ set(b)):
        if re.search(pat, n):
            bad += 1
            print(f"{n:46s} only in the {'old' if n in a else 'new'} file")
    for n in sorted(set(a) & set(b)):
        if not re.search(pat, n):
            continue
        (da, fa), (db, fb) = analyse(a[n]), analyse(b[n])
        mfma = sum("amdgcn.mfma" in da[v] for v, _ in fa), sum("amdgcn.mfma" in db[v] for v, _ in fb)
        ca, cb = collections.Counter(x for _, x in fa), collections.Counter(x for _, x in fb)
        only_a, only_b = ca - cb, cb - ca
        bad += bool(only_a or only_b)
        print(f"{n:46s} fp values {len(fa)} / {len(fb)}  only old {sum(only_a.values())}  only new {sum(only_b.values())}"
              + (f"  mfma {mfma[0]} / {mfma[1]}" if any(mfma) else ""))
        for side, d, f, only in (("old", da, fa, only_a), ("new", db, fb, only_b)):
            for v, x in [t for t in f if t[1] in only][:examples]:
                print("   ", side, v, show(d, v, 3)[:220])
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
