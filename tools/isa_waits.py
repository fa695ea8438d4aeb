#!/usr/bin/env python3
"""Where do the camera-chunk kernels wait for vector memory between their barriers?  For two builds of a translation unit
(assembly as for tools/isa_same.py) and every e0_ck / e0_ck_h instantiation: each `s_waitcnt vmcnt(N)` -- with the instruction
it guards -- in three stretches of the kernel's text, the ones in which a wavefront walks no row:
  entry    kernel entry -> the first record gather (the first 16-byte load with a per-lane offset)
  fwd-end  the landmark-record requests behind a wavefront's last forward row (G: lmrec + 3 entries, step 2: + 4) -> the
           barrier that ends the way forward
  lm-step  that barrier -> the barrier behind the landmark step (g = G u)
A "barrier" is s_barrier or, in the instantiations with two groups of wavefronts, the s_sleep of the group barrier.  The
stretches are found in the TEXT of the function (block placement keeps them contiguous in these kernels: checked by eye on
the default instantiation); the loop over landmark tiles beyond the ones requested ahead lies inside lm-step and is marked.
Behind each kernel: VGPRs, scratch, occupancy and the instruction counts of tools/isa_counts.py.  The guarded instructions are
printed for the kernels whose name contains the optional third argument (default: the two headline instantiations); for the
others the counts N alone, in text order.

usage: isa_waits.py old.s new.s [substring of the kernels to print in full | all]"""
import re
import subprocess
import sys

from isa_counts import counts, kernel_info
from isa_same import funcs

PAT = r"e0_ck(_h)?<"
FULL = ("e0_ck<16, 2, false, 1, false, true>", "e0_ck_h<16, 2, false, 2048>")


def lines_of(buf):
    return [re.sub(r";.*", "", x).strip() for x in buf if x.strip() and not x.strip().startswith(";")]


def is_barrier(x):
    return x.startswith("s_barrier") or x.startswith("s_sleep")


def waits(seg):
    out = []
    for i, x in enumerate(seg):
        m = re.match(r"s_waitcnt .*vmcnt\((\d+)\)", x)
        if m:
            nxt = next((y for y in seg[i + 1:] if not y.startswith("s_waitcnt") and not y.startswith(".L")), "(end of the stretch)")
            out.append((m.group(1), nxt))
    return out


def stretches(ls, step2):
    first_gather = next(i for i, x in enumerate(ls) if re.match(r"(buffer_load_dwordx4 .* offen|global_load_dwordx4 )", x))
    rec_off = "offset:2048" if step2 else "offset:1536"
    g = next(i for i, x in enumerate(ls) if x.startswith("global_load_dwordx2") and x.endswith(rec_off))
    b2 = next(i for i in range(g, len(ls)) if is_barrier(ls[i]))
    b3 = next(i for i in range(b2 + 1, len(ls)) if is_barrier(ls[i]))
    return {"entry": ls[:first_gather], "fwd-end": ls[g:b2], "lm-step": ls[b2 + 1:b3]}


def main():
    old, new = sys.argv[1], sys.argv[2]
    full = (sys.argv[3],) if len(sys.argv) > 3 else FULL
    fa, fb = funcs(old), funcs(new)
    ia, ib = kernel_info(old), kernel_info(new)
    names = sorted(set(fa) & set(fb))
    dem = [d.split("(")[0] for d in subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n")]
    for n, d in zip(names, dem):
        if not re.search(PAT, d):
            continue
        print(d.replace("void povar::", ""))
        for tag, f, info in (("parent", fa, ia), ("head", fb, ib)):
            ls = lines_of(f[n])
            c = counts([x for x in ls if not x.startswith(".L")])
            i = info.get(n, {})
            print(f"  {tag}: vgpr {i.get('next_free_vgpr')} scratch {i.get('ScratchSize')} occupancy {i.get('Occupancy')}; fp64 {c['fp64']} "
                  f"ds {c['ds']} vmem {c['vmem']} s_load {c['s_load']} s_waitcnt {c['s_waitcnt']}")
            in_full = full == ("all",) or any(x in d for x in full)
            brief = []
            for name, seg in stretches(ls, "e0_ck_h<" in d).items():
                w = waits(seg)
                if in_full:
                    print(f"    {name:8s}" + ("none" if not w else ("\n" + " " * 12).join(f"vmcnt({n}) -> {x}" for n, x in w)))
                else:
                    brief.append(f"{name}: " + (" ".join(n for n, _ in w) or "none"))
            if brief:
                print("    " + "   ".join(brief))
    return 0


if __name__ == "__main__":
    sys.exit(main())
