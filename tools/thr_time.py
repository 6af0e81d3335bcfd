#!/usr/bin/env python3
"""Time the thresholds post-pass (pfp_thresholds, csrc/thresholds.h) on a bench.py workload shape, on the card.

  --workload S-chr22 (-s, run samples added)   S-3G (-s -r)        (bench.py's generators and shapes, not changed)

On the resident state of one build with the full SA and the run samples, `--reps` times each (min and median of the wall times;
the per-kernel split from the engine's HIP-event profile of one more call):
  * lcp_rows:       pfp_lcp_array(PFP_LCP_ROWS) -- the yardstick: the threshold pass reads the same rows once more plus r-sized work;
  * thr_cached:     pfp_thresholds on the rows that call left;
  * thr_scratch:    pfp_thresholds without them (the rows are made into scratch first: about lcp_rows + thr_cached).
--thr-long-min N / --thr-tile N repeat the cached pass with other tunables (A/B of the long route).  Writes one JSON line to
profiles/thr_time_<workload>.json (or --out) and prints it.

--windowed: the route without a resident SA (pfp_thresholds_windowed) instead.  S-chr22 / S-3G keep their -s -r build, so that the
full route on the same build is the yardstick (thr_scratch) and the two results are compared on the device (wordsum); S-32G is
built with -r only, where no full route exists: lcp_runs (pfp_lcp_array(PFP_LCP_RUNS), the irreducible values) stands next to the
build time instead.  thr_windowed is timed with those values cached (thr_windowed_cold: without them); its kernels_ms split names
plcp_build (pairs + directory), the emission kernels of the windows, lcp_sparse, thr_tiles and thr_queries / thr_long;
device_bytes_committed is what the device had in use afterwards (text and build included; the workspace keeps what it committed).  --window-rows R: rows per window (0: the default).
The JSON line goes to profiles/thr_time_<workload>_windowed.json."""
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
    ctx.profile_enable(False)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="S-chr22", choices=["S-chr22", "S-3G", "S-5M", "S-50M", "S-20x32M", "S-100x32M", "S-32G"])
    ap.add_argument("--windowed", action="store_true", help="time pfp_thresholds_windowed (S-32G: a build with -r only)")
    ap.add_argument("--window-rows", type=int, default=0, help="rows per window of the windowed route (0: the default)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--thr-long-min", type=int, nargs="*", default=[], help="also time the cached pass with these single-lane limits")
    ap.add_argument("--thr-tile", type=int, nargs="*", default=[], help="also time the cached pass with these tile sizes")
    ap.add_argument("--out", default="", help="file for the JSON line (default: profiles/thr_time_<workload>.json)")
    a = ap.parse_args()
    import torch
    from bench import WORKLOADS, synth_to_device
    L, H, seed, nruns, w, p, u64 = WORKLOADS[a.workload]
    d = torch.empty((H, L), dtype=torch.uint8, device="cuda")
    synth_to_device(d, L, H, seed, nruns)
    torch.cuda.synchronize()
    ctx = pfbwt_hip.PfpContext(w=w, p=p, u64=u64, sai=True)
    ctx.feed_device_view(d.data_ptr(), H, L, d.stride(0))
    big = a.workload in ("S-32G", "S-100x32M")                 # no room for a full SA: -r only
    if big and not a.windowed:
        sys.exit("%s is built with -r only: the full route needs the SA on the device (use --windowed)" % a.workload)
    ctx.finalize(); ctx.parse_bwt(); b = ctx.bwt_build(sa=not big, rssa=True)
    del d; torch.cuda.empty_cache()
    out = dict(workload=a.workload, n=int(b.nout - 1), r=int(b.r), u_bytes=8 if u64 else 4, reps=a.reps, build_ms=round(ctx.stage_ms()["bwt_build"], 1))
    C = pfbwt_hip.C
    linfo, tinfo = pfbwt_hip.LcpInfo(), pfbwt_hip.ThrInfo()
    if a.windowed:
        nwin = C.c_uint64(0)
        win = lambda: ctx._check(ctx.L.pfp_thresholds_windowed(ctx.h, a.window_rows, C.byref(tinfo), C.byref(nwin)))
        def sums():
            res = []
            for ptr in ctx.thresholds_device_ptrs():
                o = (C.c_uint64 * 2)()
                ctx._check(ctx.L.pfp_debug_wordsum(ctx.h, ptr, 2 * int(b.r) * (8 if u64 else 4), o))
                res.append((int(o[0]), int(o[1])))
            return res
        out["windowed"] = True
        if not big:                                           # the yardstick, and the arrays to compare with
            out["thr_scratch"] = timed(ctx, lambda: ctx._check(ctx.L.pfp_thresholds(ctx.h, C.byref(tinfo))), a.reps)
            full_sums, full_info = sums(), {k: int(getattr(tinfo, k)) for k, _ in pfbwt_hip.ThrInfo._fields_}
        out["thr_windowed_cold"] = wall(win, 1)
        out["lcp_runs"] = timed(ctx, lambda: ctx._check(ctx.L.pfp_lcp_array(ctx.h, pfbwt_hip.LCP_RUNS, C.byref(linfo))), a.reps)
        out["thr_windowed"] = timed(ctx, win, a.reps)
        out["windows"], out["window_rows"] = int(nwin.value), a.window_rows
        out["info"] = {k: int(getattr(tinfo, k)) for k, _ in pfbwt_hip.ThrInfo._fields_}
        if not big:
            out["equal_to_full_route"] = bool(sums() == full_sums and out["info"] == full_info)
            out["windowed_over_full"] = round(out["thr_windowed"]["min_ms"] / out["thr_scratch"]["min_ms"], 2)
        free, total = torch.cuda.mem_get_info()                # the workspace never gives committed memory back: the high-water mark
        out["device_bytes_committed"] = int(total - free)
        ctx.close()
        line = json.dumps(out)
        path = a.out or os.path.join(ROOT, "profiles", "thr_time_%s_windowed.json" % a.workload.replace("S-", "").lower())
        with open(path, "w") as f:
            f.write(line + "\n")
        print(line, flush=True)
        return
    thr = lambda: ctx._check(ctx.L.pfp_thresholds(ctx.h, C.byref(tinfo)))
    out["thr_scratch"] = timed(ctx, thr, a.reps)
    out["lcp_rows"] = timed(ctx, lambda: ctx._check(ctx.L.pfp_lcp_array(ctx.h, pfbwt_hip.LCP_ROWS, C.byref(linfo))), a.reps)
    out["thr_cached"] = timed(ctx, thr, a.reps)
    out["info"] = {k: int(getattr(tinfo, k)) for k, _ in pfbwt_hip.ThrInfo._fields_}
    out["cached_over_lcp_rows"] = round(out["thr_cached"]["min_ms"] / out["lcp_rows"]["min_ms"], 2)
    for key, vals, dflt in (("thr_long_min", a.thr_long_min, 128), ("thr_tile", a.thr_tile, 1024)):
        for v in vals:
            ctx.debug_set(**{key: v})
            res = timed(ctx, thr, min(a.reps, 3))
            res["long_queries"] = int(tinfo.long_queries)
            out["%s_%d" % (key, v)] = res
        ctx.debug_set(**{key: dflt})
    ctx.close()
    line = json.dumps(out)
    path = a.out or os.path.join(ROOT, "profiles", "thr_time_%s.json" % a.workload.replace("S-", "").lower())
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
