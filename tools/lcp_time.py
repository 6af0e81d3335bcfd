#!/usr/bin/env python3
"""Time the LCP-array post-pass (pfp_lcp_array, csrc/lcparray.h) on a bench.py workload shape, on the card.

  --workload S-chr22 (-s)   S-3G (-s -r)   S-32G (-r)        (bench.py's generators and shapes, not changed)

On the resident state of one build, `--reps` times each (min and median of the wall times; the per-kernel split from the
engine's HIP-event profile of the fastest repeat):
  * runs:  pfp_lcp_array(PFP_LCP_RUNS) against pfp_debug_check_sample_order -- the same r - 1 comparisons, one lane per pair,
    eight bytes per step (the baseline; where the build has run samples);
  * rows:  pfp_lcp_array(PFP_LCP_ROWS) against pfp_doc_array(PFP_DA_ROWS) -- the same SA streamed in, the same bytes streamed
    out (the floor; where the build has the full SA); split: lcp_pairs / lcp_long / memset + scan / lcp_gather.
--lcp-long-min N repeats the LCP passes with another single-lane limit (A/B of the long route).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pfbwt-f_amd", "python"))
sys.path.insert(0, ROOT)
import pfbwt_hip


def wall(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(1e3 * (time.perf_counter() - t0))
    return {"min_ms": round(min(ts), 3), "median_ms": round(statistics.median(ts), 3), "all_ms": [round(t, 3) for t in ts]}


def lcp_pass(ctx, what, reps):
    info = pfbwt_hip.LcpInfo()
    res = wall(lambda: ctx._check(ctx.L.pfp_lcp_array(ctx.h, what, pfbwt_hip.C.byref(info))), reps)
    ctx.profile_enable(True); ctx.profile_reset()          # one more call for the split (events around every launch)
    ctx._check(ctx.L.pfp_lcp_array(ctx.h, what, pfbwt_hip.C.byref(info)))
    res["kernels_ms"] = {r["kernel"]: round(r["ms"], 3) for r in ctx.profile()}
    ctx.profile_enable(False)
    res["info"] = {k: int(getattr(info, k)) for k, _ in pfbwt_hip.LcpInfo._fields_}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="S-chr22", choices=["S-chr22", "S-3G", "S-32G", "S-5M", "S-50M"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lcp-long-min", type=int, default=0, help="also time with this single-lane limit (e.g. 1073741824: no long route)")
    ap.add_argument("--rssa", action="store_true", help="build the run samples too where the shape has -s only (S-chr22: the runs comparison)")
    a = ap.parse_args()
    import torch
    from bench import WORKLOADS, outputs_of, synth_to_device
    L, H, seed, nruns, w, p, u64 = WORKLOADS[a.workload]
    want_sa, want_rssa = outputs_of(a.workload)
    want_rssa = want_rssa or a.rssa
    d = torch.empty((H, L), dtype=torch.uint8, device="cuda")
    synth_to_device(d, L, H, seed, nruns)
    torch.cuda.synchronize()
    ctx = pfbwt_hip.PfpContext(w=w, p=p, u64=u64, sai=True)
    ctx.feed_device_view(d.data_ptr(), H, L, d.stride(0))
    ctx.finalize(); ctx.parse_bwt(); b = ctx.bwt_build(sa=want_sa, rssa=want_rssa)
    del d; torch.cuda.empty_cache()
    out = dict(workload=a.workload, n=int(b.nout - 1), r=int(b.r), u_bytes=8 if u64 else 4, sa=want_sa, rssa=want_rssa, reps=a.reps, build_ms=round(ctx.stage_ms()["bwt_build"], 1))
    if want_rssa:
        order = {}
        out["check_sample_order"] = wall(lambda: order.update(ctx.check_sample_order()), a.reps)
        out["check_sample_order"]["max_lcp"] = order["max_lcp"]
        out["lcp_runs"] = lcp_pass(ctx, pfbwt_hip.LCP_RUNS, a.reps)
        out["runs_max_lcp_agrees"] = out["lcp_runs"]["info"]["max_lcp"] == order["max_lcp"]
    if want_sa:
        docs = np.ascontiguousarray(pfbwt_hip.doc_starts([L] * H, w), np.uint64)
        out["doc_array_rows"] = wall(lambda: ctx._check(ctx.L.pfp_doc_array(ctx.h, pfbwt_hip._ptr(docs), docs.size, pfbwt_hip.DA_ROWS)), a.reps)
        out["lcp_rows"] = lcp_pass(ctx, pfbwt_hip.LCP_ROWS, a.reps)
        out["rows_over_doc_array"] = round(out["lcp_rows"]["min_ms"] / out["doc_array_rows"]["min_ms"], 2)
    if a.lcp_long_min:
        ctx.debug_set(lcp_long_min=a.lcp_long_min)
        key = "lcp_long_min_%d" % a.lcp_long_min
        out[key] = lcp_pass(ctx, pfbwt_hip.LCP_RUNS if want_rssa else pfbwt_hip.LCP_ROWS, min(a.reps, 2))
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
