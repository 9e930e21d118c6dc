#!/usr/bin/env python3
"""Static instruction mix of the wave kernel between its phase marks (the `; MARK p` comments STAMP() leaves in a
non-diagnostic build).  The sweeps are fully unrolled, so the static count of a phase is what one interior-point iteration
issues.  Usage: asm_phase_mix.py kernel.s [first_mark last_mark]

Every vector opcode whose name carries `f64` counts as FP64 arithmetic, whatever its encoding suffix (`v_fmac_f64_e32`,
`v_fmac_f64_dpp`, `v_mul_f64_e64`, `v_cmp_gt_f64_e32`, `v_cvt_f64_i32_e32`), and so does an FP64 MFMA; the second table splits the
vector instructions of every phase into that arithmetic and the rest (selects, integer compares, moves, lane reads, swaps,
address arithmetic)."""
import collections
import re
import sys

VECTOR = ("fp64", "mfma", "readlane", "writelane", "v_mov", "v_mov_dpp", "v_cndmask", "v_cmp", "v_swap", "valu_other")
ARITHMETIC = ("fp64", "mfma")


def classify(op):
    if op.startswith("v_mfma"): return "mfma"
    if op.startswith("v_") and "f64" in op: return "fp64"
    if op.startswith("v_readlane") or op.startswith("v_readfirstlane"): return "readlane"
    if op.startswith("v_writelane"): return "writelane"
    if op.startswith("ds_read") or op.startswith("ds_load"): return "ds_read"
    if op.startswith("ds_write") or op.startswith("ds_store"): return "ds_write"
    if op.startswith("ds_"): return "ds_other"
    if op.startswith("global_") or op.startswith("buffer_") or op.startswith("flat_") or op.startswith("scratch_"): return "vmem"
    if op == "s_waitcnt": return "s_waitcnt"
    if op == "s_nop": return "s_nop"
    if op.startswith("s_load") or op.startswith("s_buffer"): return "smem"
    if op.startswith("s_cbranch") or op == "s_branch": return "branch"
    if op.startswith("s_"): return "salu"
    if op.startswith("v_mov") and op.endswith("_dpp"): return "v_mov_dpp"
    if op.startswith("v_mov") or op.startswith("v_accvgpr"): return "v_mov"
    if op.startswith("v_cndmask"): return "v_cndmask"
    if op.startswith("v_cmp"): return "v_cmp"
    if op.startswith("v_swap") or op.startswith("v_permlane"): return "v_swap"
    if op.startswith("v_"): return "valu_other"
    return "other"


def opcode(line):
    """the mnemonic of a line of compiler assembly, or None for a comment, a directive, a label or a blank line"""
    t = line.strip()
    if not t or t.startswith(";") or t.startswith(".") or t.split(";")[0].strip().endswith(":"):
        return None
    return t.split()[0]


def phase_mix(lines):
    """-> [(first mark, next mark, Counter of classes, DPP instructions)] for every pair of successive marks"""
    marks = [(i, int(m.group(1))) for i, l in enumerate(lines) if (m := re.search(r"; MARK (\d+)", l))]
    rows = []
    for (i0, p0), (i1, p1) in zip(marks, marks[1:]):
        mix = collections.Counter()
        dpp = 0
        for l in lines[i0:i1]:
            op = opcode(l)
            if op is None:
                continue
            mix[classify(op)] += 1
            t = l.strip()
            if "dpp" in t or "quad_perm" in t or "row_" in t: dpp += 1
        rows.append((p0, p1, mix, dpp))
    return rows


def split(mix):
    """(vector instructions, arithmetic among them, the rest)"""
    vec = sum(mix[k] for k in VECTOR)
    ari = sum(mix[k] for k in ARITHMETIC)
    return vec, ari, vec - ari


def main():
    path = sys.argv[1]
    rows = phase_mix(open(path).read().split("\n"))
    keys = ["fp64", "mfma", "readlane", "v_mov", "v_mov_dpp", "v_cndmask", "v_cmp", "v_swap", "valu_other", "ds_read", "ds_write", "vmem", "salu",
            "s_nop", "s_waitcnt", "branch"]
    print("%-9s %6s " % ("phase", "total") + " ".join("%9s" % k for k in keys) + "   dpp")
    for p0, p1, mix, dpp in rows:
        print("%3d->%-3d  %6d " % (p0, p1, sum(mix.values())) + " ".join("%9d" % mix[k] for k in keys) + "  %4d" % dpp)
    print()
    print("%-9s %8s %11s %15s" % ("phase", "vector", "arithmetic", "non-arithmetic"))
    for p0, p1, mix, _ in rows:
        print("%3d->%-3d  %8d %11d %15d" % ((p0, p1) + split(mix)))


if __name__ == "__main__":
    main()
