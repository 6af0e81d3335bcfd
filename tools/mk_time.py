#!/usr/bin/env python3
"""Time marker queries (pfp_mk_query, csrc/markerquery.h) against pfp_ri_count of the same batch in the same process, on a bench.py
workload shape, on the card.

  --workload S-50M                   (bench.py's generators and shapes, not changed)
The reads are `--reads` pieces of `--read-len` bases of the records (reads with an N dropped).  The marker array is made on the
device (pfp_marker_array, fused with a -s -r build) from a seeded marker-positions stream: an interval of 1 .. 24 positions about
every `--gap` positions, one to three markers per list out of a pool of `--pool` lists; pfp_mk_index takes it from there.

On the resident state of one build, `--reps` times each (min and median of the wall times with the copy of the results to the host;
the per-kernel split from the engine's HIP-event profile of one more call):
  * count:        pfp_ri_count + pfp_ri_get -- the yardstick: it does the same search;
  * whole:        pfp_mk_query(min_len = 0);
  * suffixes:     pfp_mk_query(min_len = --min-len, max_rows = --max-rows);
  * with --routes also `whole` and `suffixes` with mk_wave_max = 0 (every pattern through the sort).
cnt must equal pfp_ri_count's; the tool checks it.  Writes one JSON line to profiles/mk_time_<workload>.json (or --out) and prints it."""
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


def seeded_mps(np, n, gap, pool, seed):
    rng = np.random.default_rng(seed)
    lists = [[int(x) for x in rng.integers(1, 1 << 44, int(rng.integers(1, 4)))] for _ in range(pool)]
    out, p = [], int(rng.integers(0, gap))
    lens, gaps, which = rng.integers(1, 25, 2 * n // gap + 16).tolist(), rng.integers(0, 2 * gap, 2 * n // gap + 16).tolist(), rng.integers(0, pool, 2 * n // gap + 16).tolist()
    k = 0
    while p < n - 30:
        out += [p, p + lens[k] - 1] + lists[which[k]] + [0xFFFFFFFFFFFFFFFF]
        p += lens[k] + gaps[k]; k += 1
    return np.array(out, np.uint64), k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="S-50M", choices=["S-chr22", "S-5M", "S-50M", "S-20x32M"])
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--min-len", type=int, default=20)
    ap.add_argument("--max-rows", type=int, default=100)
    ap.add_argument("--gap", type=int, default=150)
    ap.add_argument("--pool", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--routes", action="store_true", help="also with mk_wave_max = 0")
    ap.add_argument("--out", default="", help="file for the JSON line (default: profiles/mk_time_<workload>.json)")
    a = ap.parse_args()
    import numpy as np
    import torch
    from bench import WORKLOADS, synth_to_device
    L, H, seed, nruns, w, p, u64 = WORKLOADS[a.workload]
    d = torch.empty((H, L), dtype=torch.uint8, device="cuda")
    synth_to_device(d, L, H, seed, nruns)
    torch.cuda.synchronize()
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    rl = min(a.read_len, L)
    draw = 2 * a.reads
    rows = torch.randint(0, H, (draw,), device="cuda", generator=g)
    cols = torch.randint(0, L - rl + 1, (draw,), device="cuda", generator=g)
    reads = d[rows[:, None], cols[:, None] + torch.arange(rl, device="cuda")[None, :]]
    reads = reads[(reads != ord("N")).all(dim=1)][:a.reads]
    a.reads = int(reads.shape[0])
    bases = reads.cpu().numpy().reshape(-1)
    offsets = (np.arange(a.reads + 1, dtype=np.uint64) * np.uint64(rl))
    del reads, rows, cols
    ctx = pfbwt_hip.PfpContext(w=w, p=p, u64=u64, sai=True)
    ctx.feed_device_view(d.data_ptr(), H, L, d.stride(0))
    ctx.finalize(); ctx.parse_bwt(); b = ctx.bwt_build(sa=True, rssa=True)
    del d; torch.cuda.empty_cache()
    n = int(b.nout - 1)
    mps, intervals = seeded_mps(np, n, a.gap, a.pool, 7)
    ma = ctx.marker_array(mps)
    out = dict(workload=a.workload, n=n, r=int(b.r), u_bytes=8 if u64 else 4, reps=a.reps, reads=a.reads, read_len=rl, min_len=a.min_len, max_rows=a.max_rows, mps_intervals=intervals, ma_words=int(ma.size))
    del ma
    ctx.ri_index()
    C = pfbwt_hip.C
    vp = lambda x: x.ctypes.data_as(C.c_void_p) if x.size else None
    bp, op = vp(bases), vp(offsets)
    out["index"] = timed(ctx, lambda: out.__setitem__("index_info", ctx.mk_index()), a.reps)
    got = {}

    def count():
        info = pfbwt_hip.RiInfo()

        def call():
            ctx._check(ctx.L.pfp_ri_count(ctx.h, bp, op, a.reads, C.byref(info)))
            cnt = np.empty(a.reads, ctx.udt)
            ctx._check(ctx.L.pfp_ri_get(ctx.h, vp(cnt), None))
            got["count"] = cnt
        out["count"] = timed(ctx, call, a.reps)
        out["count"]["info"] = {k: int(getattr(info, k)) for k, _ in pfbwt_hip.RiInfo._fields_}

    def query(key, min_len, max_rows):
        info = pfbwt_hip.MkInfo()

        def call():
            ctx._check(ctx.L.pfp_mk_query(ctx.h, bp, op, a.reads, min_len, max_rows, C.byref(info)))
            cnt, probes, moff = np.empty(a.reads, ctx.udt), np.empty(a.reads, ctx.udt), np.empty(a.reads + 1, np.uint64)
            marker, freq = np.empty(int(info.entries), np.uint64), np.empty(int(info.entries), np.uint64)
            ctx._check(ctx.L.pfp_mk_offsets_get(ctx.h, vp(moff), None))
            ctx._check(ctx.L.pfp_mk_get(ctx.h, vp(cnt), vp(probes), vp(marker), vp(freq)))
            got[key] = (cnt, probes, moff, marker, freq)
        q = timed(ctx, call, a.reps)
        q["info"] = {k: int(getattr(info, k)) for k, _ in pfbwt_hip.MkInfo._fields_}
        q["patterns_per_s_wall"] = round(a.reads / (q["min_ms"] * 1e-3))
        q["over_count"] = round(q["min_ms"] / out["count"]["min_ms"], 3)
        q["bytes_to_host"] = int(sum(x.nbytes for x in got[key]))
        out[key] = q

    count()
    query("whole", 0, 0)
    query("suffixes", a.min_len, a.max_rows)
    equal = np.array_equal(got["whole"][0], got["count"]) and np.array_equal(got["suffixes"][0], got["count"])
    if a.routes:
        ctx.debug_set(mk_wave_max=0)
        query("whole_sort", 0, 0)
        query("suffixes_sort", a.min_len, a.max_rows)
        ctx.debug_set(mk_wave_max=64)
        equal = equal and all(np.array_equal(x, y) for x, y in zip(got["whole"] + got["suffixes"], got["whole_sort"] + got["suffixes_sort"]))
    out["results_equal"] = bool(equal)
    free, total = torch.cuda.mem_get_info()
    out["device_bytes_committed"] = int(total - free)
    ctx.close()
    line = json.dumps(out)
    path = a.out or os.path.join(ROOT, "profiles", "mk_time_%s.json" % a.workload.replace("S-", "").lower())
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    if not equal:
        sys.exit("the counts differ from pfp_ri_count, or the two reductions from one another")


if __name__ == "__main__":
    main()
