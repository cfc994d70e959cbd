#!/usr/bin/env python3
"""Instruction counts per basic block of one kernel in hipcc's assembly output.

    hipcc -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize --offload-arch=gfx950 --cuda-device-only -S \
        -o fw_kernels.s firework_amd/csrc/fw_kernels.hip
    python tools/isa_blocks.py fw_kernels.s 'k_extend_linear_deferILb1E' [--grep v_rcp_f32]

A block starts at a label (.LBB*, or the `; %bb.N` comment of a fall-through block).  Columns: vector ALU instructions (every v_*
that is not a memory instruction), of those the quarter-rate transcendentals (v_rcp / v_rsq / v_sqrt / v_exp / v_log / v_sin / v_cos),
scalar instructions, LDS and vector-memory instructions.  --grep marks the blocks that hold the given mnemonic.  The kernel's register
and scratch figures are printed from its metadata.  This is how profiles/defer_pretest_isa.txt was made."""
import argparse
import re

TRANS = ("v_rcp_", "v_rsq_", "v_sqrt_", "v_exp_", "v_log_", "v_sin_", "v_cos_")
VMEM = ("global_", "buffer_", "flat_", "scratch_")


def kernel_lines(path, needle):
    out, inside, name = [], False, None
    with open(path) as f:
        for line in f:
            if not inside:
                m = re.match(r"^(\S*%s\S*):" % re.escape(needle), line)
                if m:
                    inside, name = True, m.group(1)
                continue
            if line.startswith(".Lfunc_end") or ".amdhsa_kernel" in line:
                break
            out.append(line.rstrip("\n"))
    if name is None:
        raise SystemExit(f"no function matching {needle!r} in {path}")
    return name, out


def metadata(path, name):
    keys = ("num_vgpr", "num_agpr", "numbered_sgpr", "private_seg_size")
    found = {}
    pat = re.compile(r"^\s*\.set %s\.(\w+), (.+)$" % re.escape(name))
    with open(path) as f:
        for line in f:
            m = pat.match(line)
            if m and m.group(1) in keys:
                found[m.group(1)] = m.group(2).strip()
    return found


def blocks(lines):
    cur = ["entry", dict(valu=0, trans=0, salu=0, lds=0, vmem=0, ops=[])]
    out = [cur]
    for line in lines:
        m = re.match(r"^(\.LBB\w+):", line) or re.match(r"^; %(bb\.\d+):", line)
        if m:
            cur = [m.group(1), dict(valu=0, trans=0, salu=0, lds=0, vmem=0, ops=[])]
            out.append(cur)
            continue
        m = re.match(r"^\s+([a-z_0-9]+)", line)
        if not m:
            continue
        op = m.group(1)
        c = cur[1]
        c["ops"].append(op)
        if op.startswith(VMEM):
            c["vmem"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
            c["trans"] += op.startswith(TRANS)
        elif op.startswith("s_"):
            c["salu"] += 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("kernel", help="substring of the mangled kernel name")
    ap.add_argument("--grep", default=None, help="mark blocks holding this mnemonic (prefix)")
    a = ap.parse_args()
    name, lines = kernel_lines(a.asm, a.kernel)
    print(name)
    print("  " + ", ".join(f"{k} = {v}" for k, v in sorted(metadata(a.asm, name).items())))
    print(f"  {'block':<12}{'VALU':>6}{'trans':>7}{'SALU':>6}{'LDS':>5}{'VMEM':>6}")
    tot = dict(valu=0, trans=0, salu=0, lds=0, vmem=0)
    for label, c in blocks(lines):
        for k in tot:
            tot[k] += c[k]
        if not c["ops"]:
            continue
        mark = "  <-- " + a.grep if a.grep and any(o.startswith(a.grep) for o in c["ops"]) else ""
        print(f"  {label:<12}{c['valu']:>6}{c['trans']:>7}{c['salu']:>6}{c['lds']:>5}{c['vmem']:>6}{mark}")
    print(f"  {'total':<12}{tot['valu']:>6}{tot['trans']:>7}{tot['salu']:>6}{tot['lds']:>5}{tot['vmem']:>6}")


if __name__ == "__main__":
    main()
