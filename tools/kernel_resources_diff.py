#!/usr/bin/env python3
"""Compare the kernel resources of two builds of the same translation units, per instantiation.

    for u in UNIT...; do                   (the translation units under comparison, e.g. k_cubic_grad k_points_grad)
      hipcc <the Makefile's CXXFLAGS> -Rpass-analysis=kernel-resource-usage --cuda-device-only -S $u.hip -o DIR/$u.s 2> DIR/$u.remarks
    done                                   (once in each tree: DIR = before/, after/)
    python tools/kernel_resources_diff.py before after UNIT... > table.csv

Writes one CSV row per kernel and, to stderr, a summary per unit.  Exit status 1 if an instantiation gained scratch or
AGPRs, changed its LDS size, or sits on a lower occupancy step than before (512 VGPRs per SIMD, allocated in granules of 8,
at most 8 waves: the rule of tests/test_points_grad_cpu.py).  With both .s files present it also says whether the device
assembly is the same text (the `__hip_cuid_<hash>` symbol, which the compiler derives from the source file, set aside).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import parse  # noqa: E402


def step(vgprs):
    return min(8, 512 // (-(-vgprs // 8) * 8))


def asm_text(path):
    return [l for l in open(path) if "__hip_cuid_" not in l]


def main():
    before, after, units = sys.argv[1], sys.argv[2], sys.argv[3:]
    failed = False
    print("unit,kernel,vgpr_before,vgpr_after,waves_before,waves_after,sgpr_before,sgpr_after,lds_before,lds_after,"
          "scratch_before,scratch_after,agpr_before,agpr_after")
    for u in units:
        a = {r["demangled"]: r for r in parse(os.path.join(before, u + ".remarks"))}
        b = {r["demangled"]: r for r in parse(os.path.join(after, u + ".remarks"))}
        assert a.keys() == b.keys(), (u, sorted(set(a) ^ set(b))[:4])
        changed = lower = worse = 0
        for k in a:
            x, y = a[k], b[k]
            print(f'{u},"{k}",{x["vgpr"]},{y["vgpr"]},{step(x["vgpr"])},{step(y["vgpr"])},{x["sgpr"]},{y["sgpr"]},'
                  f'{x["lds"]},{y["lds"]},{x["scratch"]},{y["scratch"]},{x["agpr"]},{y["agpr"]}')
            changed += x["vgpr"] != y["vgpr"]
            lower += step(y["vgpr"]) < step(x["vgpr"])
            worse += y["scratch"] > x["scratch"] or y["agpr"] > x["agpr"] or y["lds"] != x["lds"]
        same = ""
        sa, sb = os.path.join(before, u + ".s"), os.path.join(after, u + ".s")
        if os.path.exists(sa) and os.path.exists(sb):
            same = "; device assembly " + ("identical" if asm_text(sa) == asm_text(sb) else "DIFFERS")
        print(f"{u}: {len(a)} kernels, VGPR count changed in {changed}, lower occupancy step in {lower}, "
              f"scratch / AGPRs / LDS worse in {worse}{same}", file=sys.stderr)
        failed = failed or lower or worse
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
