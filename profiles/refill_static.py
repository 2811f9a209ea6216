#!/usr/bin/env python3
"""Static counts of k_bnb_bound_refill's instantiations in a device assembly listing.

    hipcc <the Makefile's HIPFLAGS> -Icsrc -I../include -DHVP_N=<N> -S --cuda-device-only \
        -o lane_<N>.s csrc/hvp_lane_inst.hip
    profiles/refill_static.py lane_<N>.s [...]

Method (profiles/r09a_scan_static.txt): an instruction is a line of the function's text that is
neither a label nor a directive; the trip section is the longest stretch without a global access.
Registers, scratch, LDS and waves per SIMD are read from the kernel's .amdhsa_ directives and the
occupancy comment the compiler writes behind the function.
"""
import re
import sys

PH = {"0": "ANY", "1": "LEAF", "2": "UPPER"}


def functions(text):
    """name -> (body lines, trailer lines up to the next function)"""
    out = {}
    cur = None
    for line in text.splitlines():
        m = re.match(r"^(_ZN\w*k_bnb_bound_refill\w*):", line)
        if m:
            cur = m.group(1)
            out[cur] = ([], [])
            part = 0
            continue
        if cur is None:
            continue
        if re.match(r"^\.Lfunc_end", line):
            part = 1
        if part == 1 and re.match(r"^\s*\.(globl|protected)\s", line) and out[cur][1]:
            cur = None
            continue
        out[cur][part].append(line)
    return out


def is_instr(line):
    s = line.split(";")[0].strip()
    return bool(s) and not s.endswith(":") and not s.startswith(".")


def counts(lines):
    ins = [l.split(";")[0].strip() for l in lines if is_instr(l)]
    return {
        "instr": len(ins),
        "scratch": sum(i.startswith("scratch_") for i in ins),
        "readlane": sum(i.startswith("v_readlane") for i in ins),
        "ds": sum(i.startswith("ds_") for i in ins),
    }


def trip(lines):
    ins = [l.split(";")[0].strip() for l in lines if is_instr(l)]
    best, start = (0, 0), 0
    for i, s in enumerate(ins + ["global_end"]):
        if s.startswith("global_") or s.startswith("flat_"):
            if i - start > best[1] - best[0]:
                best = (start, i)
            start = i + 1
    return ins[best[0]:best[1]]


def field(trailer, key):
    for l in trailer:
        m = re.search(key + r"[:\s]+(\d+)", l)
        if m:
            return int(m.group(1))
    return -1


def main():
    print("# kernel                     instr scratchB vgpr waves  ldsB | trip: instr scratch readlane  ds")
    for path in sys.argv[1:]:
        fns = functions(open(path).read())
        for name in sorted(fns):
            m = re.search(r"k_bnb_bound_refillILi(\d+)ELb([01])E(?:Li(\d)E)?E", name)  # (PH absent: the kernel before)
            if not m:
                continue
            body, trailer = fns[name]
            c = counts(body)
            t = counts(trip(body))
            tag = "<%s,%s,%s>" % (m.group(1), m.group(2), PH[m.group(3) or "0"])
            print("%-28s %5d %8d %4d %5d %5d | %11d %7d %8d %3d" % (
                tag, c["instr"], field(trailer, r"; ScratchSize"), field(trailer, r"; NumVgprs"),
                field(trailer, r"; Occupancy"), field(trailer, r"; LDSByteSize"),
                t["instr"], t["scratch"], t["readlane"], t["ds"]))


if __name__ == "__main__":
    main()
