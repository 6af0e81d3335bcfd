#!/usr/bin/env python3
"""Time maximal-exact-match queries (pfp_mem_find, csrc/mems.h) on a bench.py workload shape, on the card.

  --workload S-chr22                 (bench.py's generators and shapes, not changed; not repetitive: a MEM occurs about once)
  --workload S-20x32M                (a repetitive panel: a MEM of a read occurs about once per haplotype)
Both are built with -s -r, so that the phi route and the SA route of locate run on the same build; thresholds by pfp_thresholds.

On the resident state of one build, after pfp_ms_index, pfp_ri_index and ONE pfp_ms_query over `--reads` reads of `--read-len` bases
sampled from the text with `--subs` substitutions per base (default 2^18 reads of 150 bases, 1 %; the query is timed too, as in
tools/ms_time.py, for the scale):
  * mem_find:            pfp_mem_find(min_len, locate = 0), `--reps` times -- min and median of the wall times of the whole call (the
                         upload of the reads + 1 offsets and the one round trip for the number of MEMs included, the copy of the
                         results back to the host not) and kernels_ms, the per-kernel split from the engine's HIP-event profile of
                         one more call;
  * mem_locate_phi / mem_locate_sa: the same with locate = 1 and ri_route = 1 / 2, `--max-occ` positions per MEM at most (0: all).
Every entry holds info (mems, sum_len, occurrences, ...); mems_per_s and positions_per_s are given for the wall minimum and for the
sum of the kernel times.  The two locate routes must return the same arrays; the tool checks it.
Writes one JSON line to profiles/mem_time_<workload>.json (or --out) and prints it."""
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
    ap.add_argument("--subs", type=float, default=0.01, help="substitutions per base")
    ap.add_argument("--min-len", type=int, default=20)
    ap.add_argument("--max-occ", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="", help="file for the JSON line (default: profiles/mem_time_<workload>.json)")
    a = ap.parse_args()
    import numpy as np
    import torch
    from bench import WORKLOADS, synth_to_device
    L, H, seed, nruns, w, p, u64 = WORKLOADS[a.workload]
    d = torch.empty((H, L), dtype=torch.uint8, device="cuda")
    synth_to_device(d, L, H, seed, nruns)
    torch.cuda.synchronize()
    # the reads: pieces of the records with substitutions, made on the device, kept on the host (reads with an N are dropped)
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    rl = min(a.read_len, L)
    draw = 2 * a.reads
    rows = torch.randint(0, H, (draw,), device="cuda", generator=g)
    cols = torch.randint(0, L - rl + 1, (draw,), device="cuda", generator=g)
    reads = d[rows[:, None], cols[:, None] + torch.arange(rl, device="cuda")[None, :]]
    reads = reads[(reads != ord("N")).all(dim=1)][:a.reads]
    a.reads = int(reads.shape[0])
    hit = torch.rand((a.reads, rl), device="cuda", generator=g) < a.subs
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    reads = torch.where(hit, letters[torch.randint(0, 4, (a.reads, rl), device="cuda", generator=g)], reads)
    bases = reads.cpu().numpy().reshape(-1)
    offsets = (np.arange(a.reads + 1, dtype=np.uint64) * np.uint64(rl))
    del reads, hit, rows, cols
    U = 8 if u64 else 4
    want = 96 * H * (L + w) + (64 << 20) + a.reads * rl * (6 * U + 2)          # (the default workspace is sized by the text alone)
    ctx = pfbwt_hip.PfpContext(w=w, p=p, u64=u64, sai=True, workspace_bytes=want if want < 0.8 * torch.cuda.mem_get_info()[1] else 0)
    ctx.feed_device_view(d.data_ptr(), H, L, d.stride(0))
    ctx.finalize(); ctx.parse_bwt(); b = ctx.bwt_build(sa=True, rssa=True)
    del d; torch.cuda.empty_cache()
    out = dict(workload=a.workload, n=int(b.nout - 1), r=int(b.r), u_bytes=U, reps=a.reps, build_ms=round(ctx.stage_ms()["bwt_build"], 1),
               reads=a.reads, read_len=rl, subs=a.subs, min_len=a.min_len, max_occ=a.max_occ)
    C = pfbwt_hip.C
    ctx._check(ctx.L.pfp_thresholds(ctx.h, None))
    ctx.ms_index(); ctx.ri_index()
    msinfo = pfbwt_hip.MsInfo()
    bp, op = bases.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p)
    out["ms_query"] = timed(ctx, lambda: ctx._check(ctx.L.pfp_ms_query(ctx.h, bp, op, a.reads, C.byref(msinfo))), a.reps)
    arrays = {}
    for key, route in (("mem_find", 0), ("mem_locate_phi", 1), ("mem_locate_sa", 2)):
        info = pfbwt_hip.MemInfo()
        if route:
            ctx.debug_set(ri_route=route)
        q = timed(ctx, lambda: ctx._check(ctx.L.pfp_mem_find(ctx.h, a.min_len, 1 if route else 0, a.max_occ, C.byref(info))), a.reps)
        q["info"] = {k: int(getattr(info, k)) for k, _ in pfbwt_hip.MemInfo._fields_}
        for name, ms in (("wall", q["min_ms"]), ("kernels", q["kernels_sum_ms"])):
            q["mems_per_s_" + name] = round(q["info"]["mems"] / (ms * 1e-3))
            if route:
                q["positions_per_s_" + name] = round(q["info"]["reported"] / (ms * 1e-3))
        if route:
            cnt, pos = np.empty(q["info"]["mems"], ctx.udt), np.empty(q["info"]["reported"], ctx.udt)
            ctx._check(ctx.L.pfp_mem_get(ctx.h, None, None, None, cnt.ctypes.data_as(C.c_void_p) if cnt.size else None, pos.ctypes.data_as(C.c_void_p) if pos.size else None))
            arrays[route] = (cnt, pos)
        out[key] = q
    out["mems"], out["sum_len"], out["occurrences"] = (out["mem_locate_phi"]["info"][k] for k in ("mems", "sum_len", "occurrences"))
    out["routes_equal"] = bool(np.array_equal(arrays[1][0], arrays[2][0]) and np.array_equal(arrays[1][1], arrays[2][1]))
    free, total = torch.cuda.mem_get_info()
    out["device_bytes_committed"] = int(total - free)
    ctx.close()
    line = json.dumps(out)
    path = a.out or os.path.join(ROOT, "profiles", "mem_time_%s.json" % a.workload.replace("S-", "").lower())
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    if not out["routes_equal"]:
        sys.exit("the phi route and the SA route returned different arrays")


if __name__ == "__main__":
    main()
