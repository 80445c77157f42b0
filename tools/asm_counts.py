#!/usr/bin/env python3
"""Static instruction counts of the packet-traversal kernels in a gfx950 assembly listing.

    hipcc <product flags> -S --cuda-device-only knn_wave.hip -o knn_wave.s
    python tools/asm_counts.py knn_wave.s [substring of the mangled kernel name ...]

Per kernel: the resource metadata (VGPRs, SGPRs, spills, LDS), the instruction mix, the lane-spill
reloads (v_readlane_b32 from the spill VGPRs is not told apart from data readlanes: both counted),
and every run of >= 6 consecutive VGPR-to-VGPR v_mov_b32 (the list copies of profiles/r07_knn_issue).
"""
import re
import sys

DEFAULT = ["k_knn_wave_bILi22E", "10k_knn_waveILi22E"]


def body(lines, name):
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and name in l.split(":")[0] and ":" in l)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start].split(":")[0], lines[start + 1:end]


def meta(lines, sym):
    out = {}
    i = next((k for k, l in enumerate(lines) if l.strip() == f".name:           {sym}"), None)
    j = next((k for k, l in enumerate(lines) if l.strip() == f".symbol:         {sym}.kd"), None)
    if i is None or j is None:
        return out
    lo = max(0, min(i, j) - 40)
    for l in lines[lo:max(i, j) + 40]:
        m = re.match(r"\s+\.(vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|group_segment_fixed_size|agpr_count):\s+(\d+)", l)
        if m:
            out[m.group(1)] = int(m.group(2))
    return out


def main():
    path = sys.argv[1]
    names = sys.argv[2:] or DEFAULT
    lines = open(path).read().splitlines()
    vv = re.compile(r"\s*v_mov_b32(_e32)?\s+v\d+,\s*v\d+\s*$")
    for name in names:
        sym, b = body(lines, name)
        ins = [l.strip() for l in b if l.startswith("\t") and not l.strip().startswith((".", ";"))]
        cnt = {}
        for l in ins:
            op = l.split()[0]
            cnt[op] = cnt.get(op, 0) + 1
        valu = sum(v for k, v in cnt.items() if k.startswith("v_"))
        salu = sum(v for k, v in cnt.items() if k.startswith("s_") and not k.startswith(("s_load", "s_waitcnt", "s_nop", "s_branch", "s_cbranch", "s_barrier", "s_endpgm")))
        runs, r = [], 0
        for l in ins:
            if vv.match(l):
                r += 1
            else:
                if r >= 6:
                    runs.append(r)
                r = 0
        print(sym)
        print("  meta:", meta(lines, sym))
        print(f"  instructions {len(ins)}  v_* {valu}  s_* (alu) {salu}  ds_* {sum(v for k, v in cnt.items() if k.startswith('ds_'))}")
        print(f"  v_mov_b32 {cnt.get('v_mov_b32_e32', 0) + cnt.get('v_mov_b32', 0)}  v_readlane_b32 {cnt.get('v_readlane_b32', 0)}"
              f"  v_writelane_b32 {cnt.get('v_writelane_b32', 0)}  s_nop {cnt.get('s_nop', 0)}  s_set_gpr_idx_on {cnt.get('s_set_gpr_idx_on', 0)}")
        print(f"  runs of >=6 VGPR-to-VGPR v_mov_b32: {runs} (sum {sum(runs)})")


if __name__ == "__main__":
    main()
