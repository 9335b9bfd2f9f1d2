#!/usr/bin/env python3
"""Per-basic-block instruction counts of one kernel in a hipcc -S listing.

    hipcc --offload-arch=gfx950 <the Makefile's CXXFLAGS> --cuda-device-only -S \
        csrc/ldt_resize4.hip -o resize4.s
    python tools/isa_blocks.py resize4.s _ZN3ldt9k_resize4ILi5ELi5ELb0ELb0EEE

prints, for every basic block of the first kernel whose symbol starts with the
given prefix: its label, the v_* instructions in it, and how many of them are
multiplies in _e32 form, SDWA multiplies, v_mad_u32_u24, v_mad_u64_u32,
v_min_u32*, v_add3, plain v_add, byte extractions (v_and / v_bfe / v_lshrrev),
then its LDS reads and writes, global loads and stores, and the block's
branch targets. profiles/trim/resize4_isa.txt was put together from it.
"""
import re
import sys


def blocks(path, prefix):
    out, cur, inside = [], None, False
    for line in open(path):
        s = line.strip()
        if not inside:
            if s.startswith(prefix) and s.split(";")[0].strip().endswith(":"):
                inside = True
                cur = ["entry", []]
                out.append(cur)
            continue
        if s.startswith(".Lfunc_end") or s.startswith("s_endpgm"):
            if s.startswith("s_endpgm"):
                cur[1].append(s)
            if s.startswith(".Lfunc_end"):
                break
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", s)
        if m:
            cur = [m.group(1), []]
            out.append(cur)
            continue
        if not s or s.startswith(";") or s.startswith("."):
            continue
        cur[1].append(s.split(";")[0].strip())
        if s.startswith("s_cbranch") or s.startswith("s_branch"):
            # what follows a branch is a block of its own (a fall-through one has no label)
            base = cur[0].split("+")[0]
            cur = ["%s+%d" % (base, sum(1 for b in out if b[0].split("+")[0] == base)), []]
            out.append(cur)
    return out


def main():
    path, prefix = sys.argv[1], sys.argv[2]
    cols = ["v_*", "mul_e32", "mul_sdwa", "mad24", "mad64", "min", "add3", "add", "extract", "ds_r", "ds_w", "g_ld", "g_st"]
    print("%-12s " % "block" + " ".join("%8s" % c for c in cols) + "  branches")
    tot = [0] * len(cols)
    for label, ins in blocks(path, prefix):
        ops = [i.split()[0] for i in ins]
        c = [
            sum(o.startswith("v_") for o in ops),
            sum(o in ("v_mul_u32_u24_e32", "v_mul_i32_i24_e32") for o in ops),
            sum(o in ("v_mul_u32_u24_sdwa", "v_mul_i32_i24_sdwa") for o in ops),
            sum(o.startswith("v_mad_u32_u24") or o.startswith("v_mad_i32_i24") for o in ops),
            sum(o.startswith("v_mad_u64_u32") or o.startswith("v_mad_i64_i32") for o in ops),
            sum(o.startswith("v_min_u32") for o in ops),
            sum(o.startswith("v_add3_u32") for o in ops),
            sum(o.startswith("v_add_u32") or o.startswith("v_add_co") or o.startswith("v_addc") for o in ops),
            sum(o.startswith("v_and_b32") or o.startswith("v_bfe_u32") or o.startswith("v_lshrrev_b32") for o in ops),
            sum(o.startswith("ds_read") for o in ops),
            sum(o.startswith("ds_write") for o in ops),
            sum(o.startswith("global_load") or o.startswith("s_load") or o.startswith("s_buffer_load") for o in ops),
            sum(o.startswith("global_store") or o.startswith("flat_store") for o in ops),
        ]
        br = [i.split()[-1] for i in ins if i.startswith("s_cbranch") or i.startswith("s_branch")]
        if not ins:
            continue
        tot = [a + b for a, b in zip(tot, c)]
        print("%-12s " % label + " ".join("%8d" % x for x in c) + "  " + " ".join(br))
    print("%-12s " % "total" + " ".join("%8d" % x for x in tot))


if __name__ == "__main__":
    main()
