#!/usr/bin/env python3
"""Resources of the kernels of a gfx950 code object, read from the metadata of its assembly -- no GPU needed:

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S -o pfbwt.s pfbwt-f_amd/csrc/pfbwt_hip.hip
    tools/kernel_resources.py pfbwt.s k_emit_groups_large k_seg_scatter

One line per kernel whose demangled name holds one of the patterns: workgroup size, VGPRs (requested and as allocated in granules of
8), LDS bytes, scratch bytes, spilled VGPRs (to scratch) and SGPRs (to lanes of a VGPR, no memory), and the waves resident per CU that follow from them: by registers 512 / allocation per
SIMD (at most 8), by LDS 160 KiB / footprint workgroups, and the cap of 32 waves per CU, in whole workgroups."""
import re
import subprocess
import sys


def kernels(path):
    txt = open(path).read()
    i = txt.index("amdhsa.kernels:")
    out = []
    for blk in re.split(r"\n  - \.agpr_count:", txt[i:])[1:]:
        f = {}
        for key in ("name", "vgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "max_flat_workgroup_size"):
            m = re.search(r"\.%s:\s+(\S+)" % key, ".agpr_count:" + blk)
            f[key] = m.group(1) if m else "0"
        out.append(f)
    return out


def main():
    path, pats = sys.argv[1], sys.argv[2:]
    ks = [k for k in kernels(path) if not k["name"].endswith(".kd")]
    names = subprocess.run(["c++filt"] + [k["name"] for k in ks], capture_output=True, text=True).stdout.splitlines()
    print("| kernel | threads | VGPRs (allocated) | LDS B | scratch B | VGPR spills | SGPR spills | waves per CU |")
    print("|---|---|---|---|---|---|---|---|")
    for k, dn in zip(ks, names):
        if pats and not any(p in dn for p in pats):
            continue
        thr, vg, lds = int(k["max_flat_workgroup_size"]), int(k["vgpr_count"]) + int(k["agpr_count"]), int(k["group_segment_fixed_size"])
        alloc = max(8, (vg + 7) // 8 * 8)
        wg_waves = (thr + 63) // 64
        by_reg = min(8, 512 // alloc) * 4 // wg_waves
        by_lds = (160 * 1024) // lds if lds else 1 << 20
        wgs = min(by_reg, by_lds, 32 // wg_waves)
        short = re.sub(r"\(.*", "", dn).replace("void pfp::", "").replace("unsigned long", "u64").replace("unsigned int", "u32")
        print("| `%s` | %d | %d (%d) | %d | %s | %d | %d | %d workgroups = %d |" % (short, thr, vg, alloc, lds, k["private_segment_fixed_size"], int(k["vgpr_spill_count"]), int(k["sgpr_spill_count"]), wgs, wgs * wg_waves))


if __name__ == "__main__":
    main()
