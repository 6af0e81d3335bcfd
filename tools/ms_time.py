#!/usr/bin/env python3
"""Time matching-statistics queries (pfp_ms_index / pfp_ms_query, csrc/matchstats.h) on a bench.py workload shape, on the card.

  --workload S-chr22 | S-3G          (bench.py's generators and shapes, not changed; built with -s -r, thresholds by pfp_thresholds)
  --workload S-32G                   (built with -r only, thresholds by pfp_thresholds_windowed)

On the resident state of one build:
  * ms_index:  pfp_ms_index, `--reps` times (min and median of the wall times; the per-kernel split from the engine's HIP-event
               profile of one more call);
  * ms_query:  pfp_ms_query over `--reads` reads of `--read-len` bases sampled from the text with `--subs` substitutions per base
               (default 150 bases, 1 %), the same way: wall times of the whole call (upload of the reads and the sort of their
               lengths on the host included, the copy of the results back to the host not), and kernels_ms, the HIP-event times
               of its kernels, whose sum is the time the device was busy.  reads_per_s and gbases_per_s are given for both.
The context is created with a workspace that has room for the batch (the default is sized by the text alone).
Writes one JSON line to profiles/ms_time_<workload>.json (or --out) and prints it."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pfbwt-f_amd", "python"))
sys.path.insert(0, ROOT)
import pfbwt_hip


def wall(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(1e3 * (time.perf_counter() - t0))
    return {"min_ms": round(min(ts), 3), "median_ms": round(statistics.median(ts), 3), "all_ms": [round(t, 3) for t in ts]}


def timed(ctx, call, reps):
    res = wall(call, reps)
    ctx.profile_enable(True); ctx.profile_reset()          # one more call for the split (events around every launch)
    call()
    res["kernels_ms"] = {r["kernel"]: round(r["ms"], 3) for r in ctx.profile()}
    res["kernels_sum_ms"] = round(sum(res["kernels_ms"].values()), 3)
    ctx.profile_enable(False)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="S-chr22", choices=["S-chr22", "S-3G", "S-5M", "S-50M", "S-20x32M", "S-100x32M", "S-32G"])
    ap.add_argument("--reads", type=int, default=1 << 20)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--subs", type=float, default=0.01, help="substitutions per base")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ms-dir-log2", type=int, default=-1, help="rows per block of the run directory (-1: from n / r)")
    ap.add_argument("--out", default="", help="file for the JSON line (default: profiles/ms_time_<workload>.json)")
    a = ap.parse_args()
    import numpy as np
    import torch
    from bench import WORKLOADS, synth_to_device
    L, H, seed, nruns, w, p, u64 = WORKLOADS[a.workload]
    d = torch.empty((H, L), dtype=torch.uint8, device="cuda")
    synth_to_device(d, L, H, seed, nruns)
    torch.cuda.synchronize()
    # the reads: pieces of the records with substitutions, made on the device, kept on the host
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    rl = min(a.read_len, L)
    rows = torch.randint(0, H, (a.reads,), device="cuda", generator=g)
    cols = torch.randint(0, L - rl + 1, (a.reads,), device="cuda", generator=g)
    idx = cols[:, None] + torch.arange(rl, device="cuda")[None, :]
    reads = d[rows[:, None], idx]
    hit = torch.rand((a.reads, rl), device="cuda", generator=g) < a.subs
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    reads = torch.where(hit, letters[torch.randint(0, 4, (a.reads, rl), device="cuda", generator=g)], reads)
    bases = reads.cpu().numpy().reshape(-1)
    offsets = (np.arange(a.reads + 1, dtype=np.uint64) * np.uint64(rl))
    del reads, hit, idx, rows, cols
    # the default workspace is sized by the text (96 bytes per base of it); a batch of reads this large gets room of its own
    U = 8 if u64 else 4
    want = 96 * H * (L + w) + (64 << 20) + a.reads * rl * (6 * U + 2)
    ctx = pfbwt_hip.PfpContext(w=w, p=p, u64=u64, sai=True, workspace_bytes=want if want < 0.8 * torch.cuda.mem_get_info()[1] else 0)
    ctx.feed_device_view(d.data_ptr(), H, L, d.stride(0))
    big = a.workload in ("S-32G", "S-100x32M")                 # no room for a full SA: -r only, windowed thresholds
    ctx.finalize(); ctx.parse_bwt(); b = ctx.bwt_build(sa=not big, rssa=True)
    del d; torch.cuda.empty_cache()
    out = dict(workload=a.workload, n=int(b.nout - 1), r=int(b.r), u_bytes=8 if u64 else 4, reps=a.reps, build_ms=round(ctx.stage_ms()["bwt_build"], 1),
               reads=a.reads, read_len=rl, subs=a.subs)
    C = pfbwt_hip.C
    t0 = time.perf_counter()
    ctx._check(ctx.L.pfp_thresholds_windowed(ctx.h, 0, None, None) if big else ctx.L.pfp_thresholds(ctx.h, None))
    out["thresholds_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    if a.ms_dir_log2 >= 0:
        ctx.debug_set(ms_dir_log2=a.ms_dir_log2)
    out["ms_dir_log2"] = a.ms_dir_log2
    out["ms_index"] = timed(ctx, lambda: ctx._check(ctx.L.pfp_ms_index(ctx.h)), a.reps)
    info = pfbwt_hip.MsInfo()
    bp, op = bases.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p)
    q = timed(ctx, lambda: ctx._check(ctx.L.pfp_ms_query(ctx.h, bp, op, a.reads, C.byref(info))), a.reps)
    out["ms_query"] = q
    out["info"] = {k: int(getattr(info, k)) for k, _ in pfbwt_hip.MsInfo._fields_}
    nb = a.reads * rl
    for key, ms in (("wall", q["min_ms"]), ("kernels", q["kernels_sum_ms"])):
        out["reads_per_s_" + key] = round(a.reads / (ms * 1e-3))
        out["gbases_per_s_" + key] = round(nb / (ms * 1e-3) / 1e9, 4)
    free, total = torch.cuda.mem_get_info()
    out["device_bytes_committed"] = int(total - free)
    ctx.close()
    line = json.dumps(out)
    path = a.out or os.path.join(ROOT, "profiles", "ms_time_%s.json" % a.workload.replace("S-", "").lower())
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
