#!/usr/bin/env python3
"""Time count and locate queries (pfp_ri_index / pfp_ri_count / pfp_ri_locate, csrc/runindex.h) on a bench.py workload shape, on the card.

  --workload S-chr22                 (bench.py's generators and shapes, not changed; not repetitive: counts near 1)
  --workload S-20x32M                (a repetitive panel: a read of 150 bases occurs about once per haplotype)
Both are built with -s -r, so that the phi route and the SA route of locate run on the same build.

On the resident state of one build:
  * ri_index:   pfp_ri_index, `--reps` times (min and median of the wall times; the per-kernel split from the engine's HIP-event
                profile of one more call);
  * ri_count:   pfp_ri_count over `--reads` reads of `--read-len` bases sampled from the text with `--subs` substitutions per base
                (default 150 bases, none; reads that hold an N are dropped), the same way: wall times of the whole call (upload of the reads and the sort of their
                lengths on the host included, the copy of the results back to the host not) and kernels_ms;
  * ri_locate_phi / ri_locate_sa: pfp_ri_locate with ri_route = 1 / 2, `--max-occ` positions per read at most (0: all).
patterns_per_s and positions_per_s are given for the wall minimum and for the sum of the kernel times; info holds pieces, max_piece
and phi_steps.  The two locate routes must return the same arrays; the tool checks it.
Writes one JSON line to profiles/ri_time_<workload>.json (or --out) and prints it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pfbwt-f_amd", "python"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pfbwt_hip
from ms_time import timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="S-chr22", choices=["S-chr22", "S-5M", "S-50M", "S-20x32M"])
    ap.add_argument("--reads", type=int, default=1 << 18)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--subs", type=float, default=0.0, help="substitutions per base")
    ap.add_argument("--max-occ", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ri-dir-log2", type=int, default=-1, help="text positions per block of the phi directory (-1: from n / r)")
    ap.add_argument("--out", default="", help="file for the JSON line (default: profiles/ri_time_<workload>.json)")
    a = ap.parse_args()
    import numpy as np
    import torch
    from bench import WORKLOADS, synth_to_device
    L, H, seed, nruns, w, p, u64 = WORKLOADS[a.workload]
    d = torch.empty((H, L), dtype=torch.uint8, device="cuda")
    synth_to_device(d, L, H, seed, nruns)
    torch.cuda.synchronize()
    # the reads: pieces of the records, with substitutions when asked for, made on the device, kept on the host
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    rl = min(a.read_len, L)
    draw = 2 * a.reads                                     # reads with an N are dropped: a read inside a run of N occurs once per position of the run
    rows = torch.randint(0, H, (draw,), device="cuda", generator=g)
    cols = torch.randint(0, L - rl + 1, (draw,), device="cuda", generator=g)
    reads = d[rows[:, None], cols[:, None] + torch.arange(rl, device="cuda")[None, :]]
    reads = reads[(reads != ord("N")).all(dim=1)][:a.reads]
    a.reads = int(reads.shape[0])
    if a.subs > 0:
        hit = torch.rand((a.reads, rl), device="cuda", generator=g) < a.subs
        letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
        reads = torch.where(hit, letters[torch.randint(0, 4, (a.reads, rl), device="cuda", generator=g)], reads)
    bases = reads.cpu().numpy().reshape(-1)
    offsets = (np.arange(a.reads + 1, dtype=np.uint64) * np.uint64(rl))
    del reads, rows, cols
    ctx = pfbwt_hip.PfpContext(w=w, p=p, u64=u64, sai=True)          # the default workspace: index and results must fit it
    ctx.feed_device_view(d.data_ptr(), H, L, d.stride(0))
    ctx.finalize(); ctx.parse_bwt(); b = ctx.bwt_build(sa=True, rssa=True)
    del d; torch.cuda.empty_cache()
    out = dict(workload=a.workload, n=int(b.nout - 1), r=int(b.r), u_bytes=8 if u64 else 4, reps=a.reps, build_ms=round(ctx.stage_ms()["bwt_build"], 1),
               reads=a.reads, read_len=rl, subs=a.subs, max_occ=a.max_occ, ri_dir_log2=a.ri_dir_log2)
    if a.ri_dir_log2 >= 0:
        ctx.debug_set(ri_dir_log2=a.ri_dir_log2)
    C = pfbwt_hip.C
    out["ri_index"] = timed(ctx, lambda: ctx._check(ctx.L.pfp_ri_index(ctx.h)), a.reps)
    bp, op = bases.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p)
    arrays = {}
    for key, route in (("ri_count", 0), ("ri_locate_phi", 1), ("ri_locate_sa", 2)):
        info = pfbwt_hip.RiInfo()
        if route:
            ctx.debug_set(ri_route=route)
            call = lambda: ctx._check(ctx.L.pfp_ri_locate(ctx.h, bp, op, a.reads, a.max_occ, C.byref(info)))
        else:
            call = lambda: ctx._check(ctx.L.pfp_ri_count(ctx.h, bp, op, a.reads, C.byref(info)))
        q = timed(ctx, call, a.reps)
        q["info"] = {k: int(getattr(info, k)) for k, _ in pfbwt_hip.RiInfo._fields_}
        for name, ms in (("wall", q["min_ms"]), ("kernels", q["kernels_sum_ms"])):
            q["patterns_per_s_" + name] = round(a.reads / (ms * 1e-3))
            if route:
                q["positions_per_s_" + name] = round(q["info"]["reported"] / (ms * 1e-3))
        if route:
            q["mean_piece"] = round(q["info"]["reported"] / max(q["info"]["pieces"], 1), 3)
            cnt, pos = np.empty(a.reads, ctx.udt), np.empty(q["info"]["reported"], ctx.udt)
            ctx._check(ctx.L.pfp_ri_get(ctx.h, cnt.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p) if pos.size else None))
            arrays[route] = (cnt, pos)
        out[key] = q
    out["routes_equal"] = bool(np.array_equal(arrays[1][0], arrays[2][0]) and np.array_equal(arrays[1][1], arrays[2][1]))
    free, total = torch.cuda.mem_get_info()
    out["device_bytes_committed"] = int(total - free)
    ctx.close()
    line = json.dumps(out)
    path = a.out or os.path.join(ROOT, "profiles", "ri_time_%s.json" % a.workload.replace("S-", "").lower())
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    if not out["routes_equal"]:
        sys.exit("the phi route and the SA route returned different arrays")


if __name__ == "__main__":
    main()
