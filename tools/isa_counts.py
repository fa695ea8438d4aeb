#!/usr/bin/env python3
"""Same vector and memory work, same registers?  For two builds of a translation unit (assembly as for tools/isa_same.py) and
the kernels whose name matches a pattern: per kernel the counts of fp64 / fp32 vector instructions, ds_*, buffer_* / global_* /
flat_*, s_load*, s_barrier and s_waitcnt, .amdhsa_next_free_vgpr, occupancy and scratch size, and whether the s_waitcnt
instructions come in the same order.  Every other device function must be identical (isa_same.py's comparison).
Scalar bookkeeping and register numbering may differ: they are not counted.

usage: isa_counts.py old.s new.s [name pattern, default e0_ck]     exit status 1 if a count, a register figure or another
function differs"""
import re
import subprocess
import sys

from isa_same import body, funcs

CLASSES = (("fp64", r"v_\w+_f64"), ("fp32", r"v_\w+_f32"), ("ds", r"ds_\w+"), ("vmem", r"(buffer|global|flat|scratch)_\w+"),
           ("s_load", r"s_(buffer_)?load\w+"), ("s_barrier", r"s_barrier"), ("s_waitcnt", r"s_waitcnt\w*"))


def kernel_info(path):
    """{name: {next_free_vgpr, Occupancy, ScratchSize}} from the .amdhsa_kernel blocks and the compiler's comments"""
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z[^:]*):", line)
        if m:
            cur = m.group(1)
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.match(r"\s*\.amdhsa_next_free_vgpr (\d+)", line)
        if m and cur:
            out.setdefault(cur, {})["next_free_vgpr"] = int(m.group(1))
        m = re.match(r"; (Occupancy|ScratchSize): (\d+)", line)
        if m and cur:
            out.setdefault(cur, {})[m.group(1)] = int(m.group(2))
    return out


def counts(lines):
    c = {name: 0 for name, _ in CLASSES}
    for x in lines:
        op = x.split()[0]
        for name, pat in CLASSES:
            if re.fullmatch(pat, op):
                c[name] += 1
    return c


def main():
    old, new = sys.argv[1], sys.argv[2]
    pat = sys.argv[3] if len(sys.argv) > 3 else "e0_ck"
    a, b = funcs(old), funcs(new)
    ia, ib = kernel_info(old), kernel_info(new)
    names = sorted(set(a) | set(b))
    dem = [d.split("(")[0] for d in subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n")]
    bad = 0
    other_same = other = 0
    for n, d in zip(names, dem):
        sa, sb = body(a.get(n, [])), body(b.get(n, []))
        if not re.search(pat, d):
            other += 1
            other_same += sa == sb
            if sa != sb:
                bad += 1
                print(f"  OTHER FUNCTION DIFFERS: {d}   {len(sa)} -> {len(sb)} instructions")
            continue
        ca, cb = counts(sa), counts(sb)
        fa, fb = ia.get(n, {}), ib.get(n, {})
        notes = []
        for key in ca:
            if ca[key] != cb[key]:
                notes.append(f"{key} {ca[key]} -> {cb[key]}")
        for key in ("next_free_vgpr", "Occupancy"):
            if fa.get(key) != fb.get(key):
                notes.append(f"{key} {fa.get(key)} -> {fb.get(key)}")
        if fb.get("ScratchSize", 0) > fa.get("ScratchSize", 0):
            notes.append(f"ScratchSize {fa.get('ScratchSize')} -> {fb.get('ScratchSize')}")
        bad += bool(notes)
        wa = [x for x in sa if x.startswith("s_waitcnt")]
        wb = [x for x in sb if x.startswith("s_waitcnt")]
        state = "identical" if sa == sb else f"{len(sa)} -> {len(sb)} instructions"
        print(f"  {d}: {state}; fp64 {cb['fp64']} fp32 {cb['fp32']} ds {cb['ds']} vmem {cb['vmem']} s_load {cb['s_load']} "
              f"s_barrier {cb['s_barrier']} s_waitcnt {cb['s_waitcnt']} vgpr {fb.get('next_free_vgpr')} occupancy {fb.get('Occupancy')} "
              f"scratch {fa.get('ScratchSize')} -> {fb.get('ScratchSize')}; s_waitcnt order {'same' if wa == wb else 'DIFFERS'}"
              + ("; MISMATCH: " + ", ".join(notes) if notes else ""))
    print(f"{other_same} of {other} other device functions identical instruction by instruction; {bad} mismatches")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
