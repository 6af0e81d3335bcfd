#!/usr/bin/env python3
"""Measurement of the variant-panel feed (pfp_parse_feed_panel; DESIGN.md section 4 "Panel feed").

A seeded S-32G-shaped panel: a reference of --ref bases (32 000 000), --haplotypes haplotypes (1000; the expanded text has to fit into
page-locked host memory AND twice into HBM for the comparison, so smaller boxes take 100 and say so), a site every --site-every bases
(100), a tenth of the sites short indels.  In one process, after a warm-up of each, --reps (3) alternations of
  (a) pfp_parse_feed_panel from host arrays, through to the device synchronise the call ends with;
  (b) the path it replaces: the same text from page-locked host memory through pfp_parse_feed per record;
  (c) the floor: the same text already in HBM through pfp_parse_feed_device per record, a plain device copy.
Then finalize + parse_bwt + bwt_build(rssa) on (a) and (b) with the word sums of .bwt / .ssa / .esa compared, and one more (a) under the
library's own per-kernel event profile for the kernels of the feed.  Prints one JSON line (--out FILE: also written there)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "pfbwt-f_amd", "python"))
import pfbwt_hip


def make_panel(ref_len, nhap, every, seed):
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, ref_len, dtype=np.uint8)
    ref = np.frombuffer(b"ACGT", np.uint8)[ref]
    pos = np.arange(every // 2, ref_len - every - 16, every, dtype=np.uint64)
    pos = pos + rng.integers(0, max(every // 4, 1), pos.size).astype(np.uint64)      # ascending, further apart than any span
    ns = pos.size
    kind = rng.integers(0, 20, ns)                      # 0: insertion, 1: deletion, else SNP
    span = np.where(kind == 1, rng.integers(2, 7, ns), 1).astype(np.uint32)
    alen = np.where(kind == 0, rng.integers(2, 7, ns), 1).astype(np.uint64)
    alt_off = np.concatenate([[0], np.cumsum(alen)]).astype(np.uint64)
    alt = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(alt_off[-1]), dtype=np.uint8)]
    first = alt_off[:-1].astype(np.int64)
    snp = kind > 1
    alt[first[snp]] = np.frombuffer(b"CGTA", np.uint8)[np.searchsorted(np.frombuffer(b"ACGT", np.uint8), ref[pos[snp].astype(np.int64)])]      # a base that differs
    alt[first[~snp]] = ref[pos[~snp].astype(np.int64)]                                                                                          # indels keep the anchor base
    freq = rng.integers(1, 50, ns).astype(np.uint8)     # allele frequency of the site in percent
    gt = (rng.integers(0, 100, (ns, nhap), dtype=np.uint8) < freq[:, None]).astype(np.uint8)
    return dict(ref=ref, ref_off=np.array([0, ref_len], np.uint64), site_first=np.array([0, ns], np.uint64), pos=pos, span=span,
                allele_first=np.arange(ns + 1, dtype=np.uint64), alt_off=alt_off, alt_bytes=alt, gt=gt, nhap=nhap)


def wordsums(ctx):
    b = ctx.bsizes; U = 8 if ctx.u64 else 4
    ptrs = ctx.bwt_device_ptrs()
    out = {}
    for name, p, nbytes in (("bwt", ptrs[0], b.nout), ("ssa", ptrs[2], 2 * b.r * U), ("esa", ptrs[3], 2 * b.r * U)):
        s = C.c_uint64(0)
        ctx._check(ctx.L.pfp_debug_wordsum(ctx.h, C.c_void_p(p), int(nbytes), C.byref(s)))
        out[name] = int(s.value)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--haplotypes", type=int, default=1000); ap.add_argument("--ref", type=int, default=32_000_000); ap.add_argument("--site-every", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3); ap.add_argument("--seed", type=int, default=1); ap.add_argument("--no-build", action="store_true"); ap.add_argument("--out")
    a = ap.parse_args()
    w = 10
    t0 = time.time()
    P = make_panel(a.ref, a.haplotypes, a.site_every, a.seed)
    pcie_a = sum(int(np.asarray(v).nbytes) for k, v in P.items() if k != "nhap")
    print("panel: %d sites, %d haplotypes, %.1f MB of arrays (%.1f s to make)" % (P["pos"].size, a.haplotypes, pcie_a / 1e6, time.time() - t0), file=sys.stderr, flush=True)
    A = pfbwt_hip.PfpContext(w=w, p=100, u64=True, sai=True)
    info = A.feed_panel(ref_first=True, records=True, **P)      # warm-up of (a); its text is what (b) and (c) feed
    n = A.text_length()
    starts = np.array([s for _, s in A.docs()] + [n], np.int64)
    host = torch.empty(n, dtype=torch.uint8, pin_memory=True)
    A._check(A.L.pfp_text_get(A.h, 0, n, C.c_void_p(host.data_ptr())))
    dev = host.to("cuda"); torch.cuda.synchronize()
    lens = (np.diff(starts) - w).tolist(); offs = starts[:-1].tolist()
    Bc = pfbwt_hip.PfpContext(w=w, p=100, u64=True, sai=True); Cc = pfbwt_hip.PfpContext(w=w, p=100, u64=True, sai=True)
    for ctx in (Bc, Cc):
        ctx.reserve(n)

    def run_a():
        A.reset(); t = time.perf_counter(); A.feed_panel(ref_first=True, **P); return (time.perf_counter() - t) * 1e3

    def run_b():
        Bc.reset(); t = time.perf_counter()
        for o, l in zip(offs, lens):
            Bc._check(Bc.L.pfp_parse_feed(Bc.h, C.c_void_p(host.data_ptr() + o), l, 1))
        return (time.perf_counter() - t) * 1e3

    def run_c():
        Cc.reset(); t = time.perf_counter()
        for o, l in zip(offs, lens):
            Cc._check(Cc.L.pfp_parse_feed_device(Cc.h, C.c_void_p(dev.data_ptr() + o), l, 1))
        return (time.perf_counter() - t) * 1e3
    run_b(); run_c()                                             # warm-up of (b) and (c)
    ms = {"a": [], "b": [], "c": []}
    for _ in range(max(a.reps, 3)):
        ms["a"].append(run_a()); ms["b"].append(run_b()); ms["c"].append(run_c())
    res = {"tool": "panel_bench", "haplotypes": a.haplotypes, "ref": a.ref, "sites": int(P["pos"].size), "n": int(n), "records": info["records"], "alt_applied": info["alt_applied"],
           "pcie_bytes": {"a": pcie_a, "b": int(sum(lens))}}
    for k, v in ms.items():
        res[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}
    A.reset(); A.profile_enable(True); A.profile_reset(); A.feed_panel(ref_first=True, **P)
    prof = {r["kernel"]: r for r in A.profile() if r["kernel"].startswith("panel_") or r["kernel"].startswith("scan_")}
    A.profile_enable(False)
    res["kernels_ms"] = {k: r["ms"] for k, r in prof.items()}
    if "panel_fill" in prof and prof["panel_fill"]["ms"] > 0:
        res["fill_write_GBps"] = n / prof["panel_fill"]["ms"] / 1e6
    assert A.text_length() == Bc.text_length() == Cc.text_length() == n
    if not a.no_build:
        sums = {}
        for name, ctx in (("a", A), ("b", Bc)):
            t = time.perf_counter(); ctx.finalize(); ctx.parse_bwt(); ctx.bwt_build(sa=False, rssa=True); sums[name] = wordsums(ctx)
            res["build_%s_ms" % name] = (time.perf_counter() - t) * 1e3; res["r"] = int(ctx.bsizes.r)
        res["wordsums"] = sums; res["wordsums_equal"] = sums["a"] == sums["b"]
        assert sums["a"] == sums["b"], sums
    line = json.dumps(res)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")
    for ctx in (A, Bc, Cc):
        ctx.close()


if __name__ == "__main__":
    main()
