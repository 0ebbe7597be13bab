#!/usr/bin/env python3
"""Static instruction counts of one kernel's main loop, from the assembly of a single-kernel compile (nothing is run).

usage: isa_loop_counts.py kernel.s [loop.txt]

kernel.s: what
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -Isybil_amd/csrc -Iinclude --offload-device-only -S one.hip -o kernel.s
writes for a .hip file that includes scan_packed.h and explicitly instantiates ONE kernel (profiles/key_word_isa.txt).
The loop is the largest span from a label to a backward branch to it among the spans that hold the fewest (but some) buffer
loads -- the late-materialisation loop with the block that enters a piece, not the kernel-wide spans around it.  Prints the
kernel's register metadata, the counts of the whole kernel and of the loop, and the loop's vector opcodes by frequency;
writes the loop's instructions to loop.txt when asked.  The counting of profiles/key_word_isa.txt and valu_diet_isa.txt.
"""
import re
import sys

META = (".vgpr_count", ".sgpr_count", ".sgpr_spill_count", ".vgpr_spill_count", ".private_segment_fixed_size")


def analyse(path):
    ins, labels, meta = [], {}, {}
    for line in open(path).read().splitlines():
        m = re.match(r"^(\.LBB\d+_\d+):", line)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        s = line.strip()
        for key in META:
            if s.startswith(key + ":"):
                meta[key] = int(s.split(":")[1])
        if line.startswith("\t") and s and s[0] not in ".;":
            ins.append(s.split(";")[0].strip())
    spans = []
    for j, t in enumerate(ins):
        m = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", t)
        k = labels.get(m.group(1)) if m else None
        if k is not None and k <= j:
            loads = sum(x.startswith("buffer_load") for x in ins[k:j + 1])
            if loads:
                spans.append((loads, ins[k:j + 1]))
    fewest = min(n for n, _ in spans)
    loop = max((sp for n, sp in spans if n == fewest), key=len)
    return meta, ins, loop


def counts(span):
    c = dict(instructions=len(span), valu=0, salu=0, ds=0, buffer_loads=0, branches=0, f64=0, v_mov=0, v_bfe=0, mul24=0, lane_moves=0, s_nop=0)
    for t in span:
        op = t.split()[0]
        if op.startswith("v_"):
            c["valu"] += 1
            c["f64"] += "f64" in op
            c["v_mov"] += op.startswith("v_mov")
            c["v_bfe"] += op.startswith("v_bfe")
            c["mul24"] += "u24" in op
            c["lane_moves"] += "readlane" in op or "writelane" in op
        elif op.startswith("s_cbranch") or op == "s_branch":
            c["branches"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
            c["s_nop"] += op == "s_nop"
        elif op.startswith("ds_"):
            c["ds"] += 1
        elif op.startswith("buffer_load"):
            c["buffer_loads"] += 1
    return c


if __name__ == "__main__":
    meta, ins, loop = analyse(sys.argv[1])
    print("metadata", meta)
    print("whole   ", counts(ins))
    print("loop    ", counts(loop))
    ops = {}
    for t in loop:
        if t.startswith("v_"):
            ops[t.split()[0]] = ops.get(t.split()[0], 0) + 1
    print("loop VALU", sorted(ops.items(), key=lambda kv: -kv[1]))
    if len(sys.argv) > 2:
        open(sys.argv[2], "w").write("\n".join(loop) + "\n")
