"""Instruction mix of the C = 128 7x6 trunk's conv layers, from the compiler's assembly of tower.hip
(hipcc -O3 --offload-arch=gfx950 --cuda-device-only -S tower.hip, with the Makefile's flags).

  python scripts/asm_layer_counts.py tower.s [fp16|bf16]

Prints one row per basic block of k_tower_dyn<Cfg<128,256,7,6,...>> that holds a whole layer's MFMAs (960 per wave:
the main loop's blocks, one layer each), and one for the whole kernel.  A record for profiles/, not a test."""
import collections
import re
import sys

COLS = ("v_mfma", "ds_read_b128", "buffer_load", "v_add_u32", "v_mad_u32_u24", "v_and_b32", "v_add3_u32", "v_mul_u32_u24",
        "v_cvt_f32_f16", "v_fma_mix_f32", "v_lshlrev_b32", "v_pk_add_f32", "v_add_f32", "v_accvgpr_read")


def blocks(path, tag):
    name = re.compile(r"^_ZN5tower11k_tower_dynINS_3CfgILi128ELi256ELi7ELi6E\w*" + tag + r"Lb0ELb1E\w*:")
    inside, cur, label = False, [], "entry"
    for line in open(path):
        if not inside:
            inside = bool(name.match(line))
            continue
        s = line.strip()
        if s.startswith(".Lfunc_end"):
            break
        m = re.match(r"^(\.LBB\w+):", s)
        if m:
            yield label, cur
            label, cur = m.group(1), []
        elif s and not s.startswith((";", ".")):
            cur.append(s.split()[0])
    yield label, cur


def row(label, ins):
    c = collections.Counter()
    for i in ins:
        for col in COLS:
            if i.startswith(col):
                c[col] += 1
    return f"{label:>10} all {len(ins):5d}  " + "  ".join(f"{col} {c[col]}" for col in COLS)


if __name__ == "__main__":
    tag = {"fp16": "DF16_", "bf16": "DF16b"}[sys.argv[2] if len(sys.argv) > 2 else "fp16"]
    whole = []
    for label, ins in blocks(sys.argv[1], tag):
        whole += ins
        if sum(i.startswith("v_mfma") for i in ins) >= 960:
            print(row(label, ins))
    print(row("kernel", whole))
