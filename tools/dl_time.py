#!/usr/bin/env python3
"""Time document listing (pfp_ri_docs, csrc/doclist.h) against what a caller had before it, on a bench.py workload shape, on the card.

  --workload S-chr22                 (bench.py's generators and shapes, not changed; not repetitive: counts near 1)
  --workload S-20x32M                (a repetitive panel: a read of 150 bases occurs about once per haplotype)
The reads are those of tools/ri_time.py (`--reads` pieces of `--read-len` bases of the records, reads with an N dropped); the documents are
the records of the workload.  Built with -s -r, so that both locate routes run on the same build.

On the resident state of one build, per locate route (ri_route 1 = phi, 2 = the SA):
  * docs_<route>:  pfp_ri_docs + the copy of cnt, doc, freq and the offsets to the host, `--reps` times (min and median of the wall
                   times; the per-kernel split from the engine's HIP-event profile of one more call);
  * host_<route>:  pfp_ri_locate + pfp_ri_get of all positions + numpy.searchsorted on the record starts + numpy.unique over
                   (read, document) keys on the host, the same way; get_ms, searchsorted_ms and unique_ms split the last call.
Both must give the same lists; the tool checks it.  With --crossover (S-20x32M in DESIGN.md) the listing also runs with each reduction
route forced: dl_wave_max = 0 (table), dl_table_max = 0 (wave + sort), both 0 (sort), and with PFP_DL_INSIDE.
Writes one JSON line to profiles/dl_time_<workload>.json (or --out) and prints it."""
import argparse
import json
import os
import sys
import time

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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--crossover", action="store_true", help="also every reduction route forced, and PFP_DL_INSIDE")
    ap.add_argument("--out", default="", help="file for the JSON line (default: profiles/dl_time_<workload>.json)")
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
    starts = pfbwt_hip.doc_starts([L] * H, w)
    ndocs = int(starts.size)
    out = dict(workload=a.workload, n=int(b.nout - 1), r=int(b.r), u_bytes=8 if u64 else 4, reps=a.reps, reads=a.reads, read_len=rl, ndocs=ndocs)
    ctx.ri_index()
    C = pfbwt_hip.C
    vp = lambda x: x.ctypes.data_as(C.c_void_p) if x.size else None
    bp, op, sp = vp(bases), vp(offsets), vp(starts)
    got = {}

    def listing(key, inside=False):
        info = pfbwt_hip.DlInfo()

        def call():
            ctx._check(ctx.L.pfp_ri_docs(ctx.h, bp, op, a.reads, sp, ndocs, 1 if inside else 0, 0, C.byref(info)))
            cnt, doff = np.empty(a.reads, ctx.udt), np.empty(a.reads + 1, np.uint64)
            doc, freq = np.empty(int(info.entries), ctx.udt), np.empty(int(info.entries), ctx.udt)
            ctx._check(ctx.L.pfp_ri_docs_offsets_get(ctx.h, vp(doff), None))
            ctx._check(ctx.L.pfp_ri_docs_get(ctx.h, vp(cnt), vp(doc), vp(freq)))
            got[key] = (cnt, doff, doc, freq)
        q = timed(ctx, call, a.reps)
        q["info"] = {k: int(getattr(info, k)) for k, _ in pfbwt_hip.DlInfo._fields_}
        q["patterns_per_s_wall"] = round(a.reads / (q["min_ms"] * 1e-3))
        q["bytes_to_host"] = int(sum(x.nbytes for x in got[key]))
        out[key] = q

    def host(key):
        info = pfbwt_hip.RiInfo()
        split = {}

        def call():
            ctx._check(ctx.L.pfp_ri_locate(ctx.h, bp, op, a.reads, 0, C.byref(info)))
            t0 = time.perf_counter()
            cnt, pos, ooff = np.empty(a.reads, ctx.udt), np.empty(int(info.reported), ctx.udt), np.empty(a.reads + 1, np.uint64)
            ctx._check(ctx.L.pfp_ri_offsets_get(ctx.h, vp(ooff), None))
            ctx._check(ctx.L.pfp_ri_get(ctx.h, vp(cnt), vp(pos)))
            t1 = time.perf_counter()
            doc = np.searchsorted(starts, pos, side="right").astype(np.uint64) - np.uint64(1)
            t2 = time.perf_counter()
            owner = np.repeat(np.arange(a.reads, dtype=np.uint64), np.diff(ooff).astype(np.int64))
            keys, freq = np.unique(owner * np.uint64(ndocs) + doc, return_counts=True)
            doff = np.zeros(a.reads + 1, np.uint64)
            np.cumsum(np.bincount((keys // np.uint64(ndocs)).astype(np.int64), minlength=a.reads), out=doff[1:])
            t3 = time.perf_counter()
            split.update(get_ms=round((t1 - t0) * 1e3, 3), searchsorted_ms=round((t2 - t1) * 1e3, 3), unique_ms=round((t3 - t2) * 1e3, 3))
            got[key] = (cnt, doff, (keys % np.uint64(ndocs)).astype(ctx.udt), freq.astype(ctx.udt))
        q = timed(ctx, call, a.reps)
        q.update(split)
        q["positions"] = int(info.reported)
        q["bytes_to_host"] = int(a.reads * (8 if u64 else 4) + 8 * (a.reads + 1) + int(info.reported) * (8 if u64 else 4))
        out[key] = q

    equal = True
    for route, name in ((1, "phi"), (2, "sa")):
        ctx.debug_set(ri_route=route, dl_wave_max=64, dl_table_max=16384)
        listing("docs_" + name)
        host("host_" + name)
        equal = equal and all(np.array_equal(x, y) for x, y in zip(got["docs_" + name], got["host_" + name]))
    if a.crossover:
        ctx.debug_set(ri_route=2)
        for key, tun in (("forced_table", dict(dl_wave_max=0, dl_table_max=16384)), ("forced_wave_sort", dict(dl_wave_max=64, dl_table_max=0)), ("forced_sort", dict(dl_wave_max=0, dl_table_max=0))):
            ctx.debug_set(**tun)
            listing(key)
            equal = equal and all(np.array_equal(x, y) for x, y in zip(got[key], got["docs_sa"]))
        ctx.debug_set(dl_wave_max=64, dl_table_max=16384)
        listing("inside", inside=True)
    out["lists_equal"] = bool(equal)
    free, total = torch.cuda.mem_get_info()
    out["device_bytes_committed"] = int(total - free)
    ctx.close()
    line = json.dumps(out)
    path = a.out or os.path.join(ROOT, "profiles", "dl_time_%s.json" % a.workload.replace("S-", "").lower())
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    if not equal:
        sys.exit("the listing and the host reduction returned different lists")


if __name__ == "__main__":
    main()
