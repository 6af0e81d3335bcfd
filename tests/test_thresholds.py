"""Matching-statistics thresholds post-pass (include/pfbwt_hip.h: pfp_thresholds; csrc/thresholds.h; pfbwt-f --thr).

Run k starts at row s = ssa[2k] with the symbol c = bwt[s]; e = the largest row < s with bwt[e] == c.  No such e: thr = tlcp = 0.
Otherwise tlcp = min lcp[e+1 .. s] and thr = the LEFTMOST row in (e, s] that holds it.  The expected values never come from the
engine: text, bwt, sa and ssa are the pinned oracle's, lcp is computed from them by direct suffix comparison (lcp_numpy), and the
thresholds by two checkers:
* thresholds_brute: per run, np.argmin over lcp[e+1 : s+1] (argmin is leftmost); exact, every run; small and medium texts;
* check_properties: vectorised (np.minimum.reduceat over the gaps), for arrays of any size: e < j <= s, lcp[j] == min of the gap,
  and min lcp[e+1 .. j-1] > lcp[j] when j > e + 1 -- together they determine j uniquely.
Every case runs with the default tunables and with thr_long_min = 1, thr_tile = 16 (every gap of more than one row takes the
wave-per-run route, gaps of more than 32 rows read tile minima)."""
import hashlib
import os
import subprocess
import sys
import numpy as np
import pytest
from pfp_testlib import EMU_SO, GOLDEN, ROOT, golden_case, oracle_run

import pfbwt_hip

EMUB = os.path.join(ROOT, "tests", "emu", "build")
BIN = os.path.join(ROOT, "pfbwt-f_amd", "bin")
FIXTURES = ["edge", "w4p7", "mult_chroms_fa", "single_chrom", "mult_chroms", "panel8"]
FORCED = {"thr_long_min": 1, "thr_tile": 16}
DEFAULTS = {"thr_long_min": 128, "thr_tile": 1024}


# ---- the checkers ------------------------------------------------------------------------------------------------------------
def lcp_numpy(text, sa):
    """LCP array of T$ by direct comparison: all rows at once, one byte position per step (as in test_lcp_array.py)"""
    n = len(text)
    t = np.empty(n + 1, np.int16); t[:n] = np.frombuffer(bytes(text), np.uint8); t[n] = -1      # the terminator: unique, smallest
    sa = np.asarray(sa, np.int64)
    assert sa.size == n + 1 and sa[0] == n
    lcp = np.zeros(n + 1, np.int64)
    rows = np.arange(1, n + 1)
    a, b = sa[:-1].copy(), sa[1:].copy()
    while rows.size:
        eq = t[a] == t[b]
        rows, a, b = rows[eq], a[eq] + 1, b[eq] + 1
        lcp[rows] += 1
    return lcp.astype(np.uint64)


def previous_rows(bwt, starts):
    """for every run start s: (has, e) with e = the largest row < s that holds bwt[s] (has = False: there is none)"""
    bwt = np.asarray(bwt, np.uint8)
    starts = np.asarray(starts, np.int64)
    has = np.zeros(starts.size, bool); e = np.zeros(starts.size, np.int64)
    heads = bwt[starts]
    for c in np.unique(heads):
        rows_c = np.flatnonzero(bwt == c)
        sel = np.flatnonzero(heads == c)
        idx = np.searchsorted(rows_c, starts[sel])              # rows_c[idx] == s
        assert np.array_equal(rows_c[idx], starts[sel])
        has[sel] = idx > 0
        e[sel] = np.where(idx > 0, rows_c[np.maximum(idx, 1) - 1], 0)
    return has, e


def thresholds_brute(bwt, lcp, ssa):
    """(thr, tlcp, span) per run: np.argmin over the gap, run by run; span = s - e (0: no threshold)"""
    starts = np.asarray(ssa, np.uint64)[0::2].astype(np.int64)
    lcp = np.asarray(lcp, np.uint64)
    has, e = previous_rows(bwt, starts)
    r = starts.size
    thr, tl, span = np.zeros(r, np.uint64), np.zeros(r, np.uint64), np.zeros(r, np.int64)
    for k in range(r):
        if has[k]:
            s, ee = int(starts[k]), int(e[k])
            j = ee + 1 + int(np.argmin(lcp[ee + 1:s + 1]))
            thr[k], tl[k], span[k] = j, lcp[j], s - ee
    return thr, tl, span


def pairs(rows, vals):
    out = np.empty(2 * len(rows), np.uint64)
    out[0::2] = rows; out[1::2] = vals
    return out


def check_properties(bwt, lcp, ssa, thr, tlcp):
    """the three properties, for every run, vectorised; raises AssertionError with the first offending run; returns (none, max_span)"""
    starts = np.asarray(ssa, np.uint64)[0::2].astype(np.int64)
    thr, tlcp = np.asarray(thr, np.uint64), np.asarray(tlcp, np.uint64)
    r = starts.size
    assert thr.size == 2 * r and tlcp.size == 2 * r
    assert np.array_equal(thr[0::2].astype(np.int64), starts) and np.array_equal(tlcp[0::2].astype(np.int64), starts), "rows of the pairs"
    has, e = previous_rows(bwt, starts)
    j, v = thr[1::2].astype(np.int64), tlcp[1::2]
    bad = np.flatnonzero(~has & ((j != 0) | (v != 0)))
    assert bad.size == 0, "run %d has no threshold, got (%d, %d)" % (bad[0], j[bad[0]], v[bad[0]])
    q = np.flatnonzero(has)
    if q.size == 0:
        return int(r), 0
    big = np.iinfo(np.uint64).max
    ext = np.concatenate([np.asarray(lcp, np.uint64), np.array([big], np.uint64)])      # (so that s + 1 = n + 1 is an index)
    eq, sq, jq, vq = e[q], starts[q], j[q], v[q]
    bad = np.flatnonzero((jq <= eq) | (jq > sq))                                         # 1. e < j <= s
    assert bad.size == 0, "run %d: row %d outside (%d, %d]" % (q[bad[0]], jq[bad[0]], eq[bad[0]], sq[bad[0]])
    idx = np.empty(2 * q.size, np.int64); idx[0::2] = eq + 1; idx[1::2] = sq + 1
    gap_min = np.minimum.reduceat(ext, idx)[0::2]                                        # min lcp[e+1 .. s]
    bad = np.flatnonzero((ext[jq] != gap_min) | (vq != gap_min))                         # 2. lcp[j] == the minimum (and tlcp holds it)
    assert bad.size == 0, "run %d: lcp[%d] = %d, tlcp %d, minimum of the gap %d" % (q[bad[0]], jq[bad[0]], ext[jq[bad[0]]], vq[bad[0]], gap_min[bad[0]])
    left = np.flatnonzero(jq > eq + 1)                                                   # 3. strictly larger values in front of j
    if left.size:
        idx = np.empty(2 * left.size, np.int64); idx[0::2] = eq[left] + 1; idx[1::2] = jq[left]
        front_min = np.minimum.reduceat(ext, idx)[0::2]
        bad = np.flatnonzero(front_min <= ext[jq[left]])
        assert bad.size == 0, "run %d: row %d is not the leftmost minimum" % (q[left[bad[0]]], jq[left[bad[0]]])
    return int(r - q.size), int((sq - eq).max())


def same(a, b):
    return a is not None and b is not None and np.array_equal(np.asarray(a, np.uint64), np.asarray(b, np.uint64))


class Expected:
    def __init__(self, ref, lcp):
        self.ref, self.lcp = ref, lcp
        self.starts = np.asarray(ref["ssa"], np.uint64)[0::2]
        j, v, self.span = thresholds_brute(ref["bwt"], lcp, ref["ssa"])
        self.thr, self.tlcp = pairs(self.starts, j), pairs(self.starts, v)
        self.r = self.starts.size
        self.none = int((self.span == 0).sum())
        # queries whose minimum occurs more than once in the gap
        self.tied = 0
        has, e = previous_rows(ref["bwt"], self.starts.astype(np.int64))
        for k in np.flatnonzero(has):
            self.tied += int((lcp[int(e[k]) + 1:int(self.starts[k]) + 1] == v[k]).sum() > 1)

    def info(self, long_min):
        return {"runs": self.r, "none": self.none, "long_queries": int((self.span > long_min).sum()), "max_span": int(self.span.max())}


def build(factory, seqs, w, p, U, sa=True, rssa=True, non_acgt_to_a=False, **switches):
    ctx = factory(w=w, p=p, u64=(U == 8), sai=True, non_acgt_to_a=non_acgt_to_a)
    if switches:
        ctx.debug_set(**switches)
    for s in seqs:
        ctx.feed(s, True)
    ctx.finalize(); ctx.parse_bwt(); ctx.bwt_build(sa=sa, rssa=rssa)
    return ctx


def check_against(ctx, exp, tag):
    """one build against the expected arrays: default tunables, then nearly every query down the long route with 16-row tiles"""
    for tun in (DEFAULTS, FORCED):
        ctx.debug_set(**tun)
        thr, tlcp, info = ctx.thresholds()
        assert same(thr, exp.thr), (tag, tun, "thr", int(np.flatnonzero(np.asarray(thr, np.uint64) != exp.thr)[0]))
        assert same(tlcp, exp.tlcp), (tag, tun, "tlcp")
        assert info == exp.info(tun["thr_long_min"]), (tag, tun, info, exp.info(tun["thr_long_min"]))
        check_properties(exp.ref["bwt"], exp.lcp, exp.ref["ssa"], thr, tlcp)


def assert_routes_covered(exps, what):
    """from the expected arrays: the forced settings sent queries down the long route, some across more than two tiles, some
    minimum was tied, and some run beside the terminator's has no threshold"""
    assert sum(e.info(FORCED["thr_long_min"])["long_queries"] for e in exps) > 0, what
    assert max(int(e.span.max()) for e in exps) > 2 * FORCED["thr_tile"], what
    assert sum(e.tied for e in exps) > 0, what
    assert all(e.none >= 2 for e in exps), what            # the terminator's run and the first run of at least one base


_fixture_cache = {}


def fixture_expected(case):
    if case not in _fixture_cache:
        man, recs = golden_case(case)
        seqs = [s for _, s in recs]
        ref = oracle_run(seqs, w=man["w"], p=man["p"], U=8)
        _fixture_cache[case] = (man, seqs, Expected(ref, lcp_numpy(ref["text"], ref["sa"])))
    return _fixture_cache[case]


def check_fixtures(factory, cases=FIXTURES):
    exps = []
    for case in cases:
        man, seqs, exp = fixture_expected(case)
        exps.append(exp)
        for U in (4, 8):
            ctx = build(factory, seqs, man["w"], man["p"], U)
            check_against(ctx, exp, (case, U))
            ctx.close()
    assert_routes_covered(exps, "fixtures")
    for e in exps:                                           # every fixture on its own reaches the long route when forced
        assert e.info(1)["long_queries"] > 0


def seeded_collections(seed):
    rng = np.random.default_rng(seed)
    rnd = lambda n: bytes(rng.choice(list(b"ACGT"), int(n)).astype(np.uint8))
    base = rnd(1500)
    mut = lambda: bytes(np.where(rng.random(len(base)) < 0.01, rng.choice(list(b"ACGT"), len(base)), np.frombuffer(base, np.uint8)).astype(np.uint8))
    return {
        "n_runs": [mut() + b"N" * 200, mut()[:700] + b"N" * 30 + mut()[700:], rnd(300) + b"N" * 500],      # gaps across the N bucket
        "gaps_and_n": [mut()[:500] + b"-" * 40 + mut()[500:], b"-" * 7 + mut() + b"N" * 60, rnd(200) + b"-" + rnd(100)],
        "single_record": [mut()],
        "panel": [mut() for _ in range(12)],
    }


def check_collection(factory, seqs, w, p, U, tag, non_acgt_to_a=False):
    ref = oracle_run(seqs, w=w, p=p, U=U, non_acgt_to_a=non_acgt_to_a)
    assert ref.get("err") is None, (tag, ref.get("err"))          # a collection the oracle rejects is a test error
    exp = Expected(ref, lcp_numpy(ref["text"], ref["sa"]))
    ctx = build(factory, seqs, w, p, U, non_acgt_to_a=non_acgt_to_a)
    check_against(ctx, exp, tag)
    ctx.close()
    return exp


def check_seeded(factory):
    exps = []
    for seed in (1, 2):
        for name, seqs in seeded_collections(seed).items():
            for w, p in ((10, 100), (4, 7)):
                exps.append(check_collection(factory, seqs, w, p, 4 if seed == 1 else 8, (seed, name, w, p)))
    assert_routes_covered(exps, "seeded")
    # a gap that crosses two first-symbol bucket borders holds two zeros: with N and '-' in the text such gaps exist
    zero_tied = 0
    for e in exps:
        v = e.tlcp[1::2]
        zero_tied += int(((v == 0) & (e.span > 0)).sum())
    assert zero_tied > 0
    rng = np.random.default_rng(9)
    base = bytes(rng.choice(list(b"ACGT"), 1200).astype(np.uint8))
    iupac = bytearray(base + base[:700])
    for k in rng.integers(0, len(iupac), 40):
        iupac[int(k)] = int(rng.choice(list(b"RYKMSWn")))
    for U, (w, p) in ((4, (4, 7)), (8, (10, 100))):
        e = check_collection(factory, [bytes(iupac), base[200:]], w, p, U, ("non_acgt_to_a", U), non_acgt_to_a=True)
        assert set(bytes(e.ref["text"])) <= set(b"ACGT")
    n_only = [base[:600] + b"N" * 90 + base[600:], base[100:900]]          # the same text with and without the folding of N
    check_collection(factory, n_only, 10, 100, 8, "n_kept")
    check_collection(factory, n_only, 10, 100, 8, "n_folded", non_acgt_to_a=True)


def check_cached_and_scratch(factory):
    """equal results with and without a preceding lcp_array(rows=True); lcp_array results fetched after thresholds() unchanged"""
    man, seqs, exp = fixture_expected("mult_chroms_fa")
    C = pfbwt_hip.C
    for U in (4, 8):
        dt = np.uint64 if U == 8 else np.uint32
        ctx = build(factory, seqs, man["w"], man["p"], U)
        assert ctx.lcp_array_device_ptrs() == [None, None]
        a = ctx.thresholds()                                      # rows into scratch
        assert ctx.lcp_array_device_ptrs() == [None, None]        # ... which left no LCP result behind
        lcp, slcp, linfo = ctx.lcp_array()
        assert same(lcp, exp.lcp)
        b = ctx.thresholds()                                      # on the cached rows
        assert same(a[0], b[0]) and same(a[1], b[1]) and a[2] == b[2] and same(a[0], exp.thr) and same(a[1], exp.tlcp)
        lcp2, slcp2 = np.empty(lcp.size, dt), np.empty(slcp.size, dt)
        assert ctx.L.pfp_lcp_array_get(ctx.h, lcp2.ctypes.data_as(C.c_void_p), slcp2.ctypes.data_as(C.c_void_p)) == 0
        assert same(lcp2, lcp) and same(slcp2, slcp)
        _, s3, _ = ctx.lcp_array(rows=False)                      # the rows are gone: scratch again
        assert ctx.lcp_array_device_ptrs()[0] is None
        c = ctx.thresholds()
        assert same(c[0], exp.thr) and same(c[1], exp.tlcp) and same(s3, slcp)
        assert same(ctx.lcp_array(rows=False)[1], slcp)
        p = ctx.thresholds_device_ptrs()
        assert p[0] and p[1] and p[0] != p[1]
        ctx.close()


def check_errors(factory):
    E_STATE = pfbwt_hip.E_STATE
    man, seqs, exp = fixture_expected("mult_chroms_fa")
    ref = exp.ref
    w, p = man["w"], man["p"]
    C = pfbwt_hip.C
    buf = np.empty(2 * exp.r, np.uint64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def status(ctx):
        with pytest.raises(pfbwt_hip.PfpError) as e:
            ctx.thresholds()
        return e.value.status

    ctx = factory(w=w, p=p, u64=True, sai=True)
    assert ctx.L.pfp_thresholds(ctx.h, None) == E_STATE                          # no build at all
    assert ctx.L.pfp_thresholds(None, None) == pfbwt_hip.E_ARG
    for s in seqs:
        ctx.feed(s, True)
    ctx.finalize(); ctx.parse_bwt()
    assert ctx.L.pfp_thresholds(ctx.h, None) == E_STATE                          # parsed, not built
    ctx.bwt_build(sa=True, rssa=True)
    assert ctx.L.pfp_thresholds_get(ctx.h, vp(buf), vp(buf)) == E_STATE          # nothing made yet
    assert ctx.L.pfp_thresholds_write(ctx.h, -1, -1) == E_STATE
    assert ctx.thresholds_device_ptrs() == [None, None]
    assert ctx.L.pfp_thresholds(ctx.h, None) == 0                                # info is nullable
    thr, tlcp, _ = ctx.thresholds()                                              # a second call replaces the first
    assert same(thr, exp.thr) and same(tlcp, exp.tlcp)
    assert ctx.L.pfp_thresholds_get(ctx.h, None, vp(buf)) == 0 and same(buf, exp.tlcp)      # NULL skips one
    ctx.bwt_build(sa=False, rssa=True)                                           # a new build drops the arrays; no SA
    assert ctx.thresholds_device_ptrs() == [None, None]
    assert status(ctx) == E_STATE and ctx.L.pfp_thresholds_get(ctx.h, vp(buf), vp(buf)) == E_STATE
    ctx.bwt_build(sa=True, rssa=False)                                           # no run samples
    assert status(ctx) == E_STATE
    ctx.bwt_build(sa=False, rssa=False)                                          # BWT only
    assert status(ctx) == E_STATE
    for sl in range(2):                                                          # a slice, even with SA and samples
        ctx.bwt_build_slice(sl, 2, sa=True, rssa=True)
        assert status(ctx) == E_STATE
    ctx.bwt_build(sa=True, rssa=True)                                            # the context is still usable
    assert same(ctx.thresholds()[0], exp.thr)
    ctx.close()
    ctx = factory(w=w, p=p, u64=True, sai=True)                                  # a loaded parse: no text in the context
    ctx.bwt_load(ref["dict"], ref["occ"], ref["bwlast"], ref["ilist"], ref["bwsai"], n_hint=ref["n"])
    ctx.bwt_build(sa=True, rssa=True)
    assert status(ctx) == E_STATE
    assert np.array_equal(ctx.bwt_get()["sa"].astype(np.uint64), ref["sa"])
    ctx.close()
    half = len(seqs) // 2 or 1                                                   # a merge of two shards: no text either
    ctxs, views = [], []
    for r, grp in enumerate((seqs[:half], seqs[half:])):
        c = factory(w=w, p=p, u64=True, sai=True)
        if r:
            c.feed_left_context(w)
        for s in grp:
            c.feed(s, True)
        c.finalize(shard=True)
        ctxs.append(c); views.append(c.shard_view())
    g = factory(w=w, p=p, u64=True, sai=True)
    g.merge_shards(views); g.parse_bwt(); g.bwt_build(sa=True, rssa=True)
    assert status(g) == E_STATE
    assert np.array_equal(g.bwt_get()["sa"].astype(np.uint64), ref["sa"])
    for c in ctxs + [g]:
        c.close()
    ctx = factory(w=w, p=p, u64=True, sai=True)                                  # unknown values of the tunables are clamped, unknown keys refused
    ctx.debug_set(thr_long_min=0, thr_tile=3)
    with pytest.raises(pfbwt_hip.PfpError):
        ctx.debug_set(thr_tiles=16)
    ctx.close()


def check_coexistence(factory):
    """document, LCP, marker arrays and thresholds of one build in several call orders: every array still fetchable and unchanged"""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import marker_oracle as mo
    from test_markers import seeded_mps
    man, seqs, exp = fixture_expected("mult_chroms_fa")
    ref = exp.ref
    b = pfbwt_hip.doc_starts([len(s) for s in seqs], man["w"])
    mps = seeded_mps(ref["sa"].size, 5)
    ma_exp = mo.marker_array(mps, ref["sa"])
    C = pfbwt_hip.C
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for U in (8, 4):
        dt = np.uint64 if U == 8 else np.uint32
        for order in ("da_lcp_ma_thr", "thr_ma_lcp_da", "thr_lcp_thr_da_thr", "lcp_thr_lcp_ma_da_thr_lcp", "ma_thr_da_thr_lcp"):
            ctx = build(factory, seqs, man["w"], man["p"], U)
            das = ma = None
            for step in order.split("_"):
                if step == "da":
                    das = ctx.doc_array(b)
                elif step == "lcp":
                    ctx.lcp_array()
                elif step == "ma":
                    ma = ctx.marker_array(mps)
                else:
                    ctx.thresholds()
            r, ep, rows = ctx.bsizes.r, ctx.esa_pairs, ctx._rows
            da, sda, eda = np.empty(rows, dt), np.empty(2 * r, dt), np.empty(2 * ep, dt)
            lcp, slcp, thr, tlcp = np.empty(rows, dt), np.empty(2 * r, dt), np.empty(2 * r, dt), np.empty(2 * r, dt)
            assert ctx.L.pfp_doc_array_get(ctx.h, p(da), p(sda), p(eda)) == 0
            assert ctx.L.pfp_lcp_array_get(ctx.h, p(lcp), p(slcp)) == 0
            assert ctx.L.pfp_thresholds_get(ctx.h, p(thr), p(tlcp)) == 0
            for k, got in enumerate((da, sda, eda)):
                assert same(got, das[k]), (U, order, k)
            assert same(lcp, exp.lcp) and same(thr, exp.thr) and same(tlcp, exp.tlcp), (U, order)
            if ma is not None:
                assert np.array_equal(ma, ma_exp), (U, order)
                ma2 = np.empty(ma.size, np.uint64)
                assert ctx.L.pfp_marker_array_get(ctx.h, p(ma2)) == 0 and np.array_equal(ma2, ma_exp), (U, order)
            out = ctx.bwt_get()
            assert same(out["sa"], ref["sa"]) and same(out["ssa"], ref["ssa"]) and same(out["esa"], ref["esa"]) and same(out["bwt"], ref["bwt"]), (U, order)
            ctx.close()


# ---- command line ------------------------------------------------------------------------------------------------------------
def sha_f(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def run(cmd, check=True):
    pr = subprocess.run(cmd, capture_output=True, text=True)
    assert pr.returncode == 0 or not check, pr.stderr[-2000:]
    return pr


def read_u(path, U):
    return np.fromfile(path, "<u4" if U == 4 else "<u8").astype(np.uint64)


def check_cli(exe, tmp):
    """exe: {'pfbwt-f': path, 'pfbwt-f64': path}"""
    others = ("bwt", "sa", "ssa", "esa", "dict", "occ", "parse", "bwlast", "ilist", "bwsai", "n", "lcp", "slcp", "da", "sda", "eda")
    for case in ("mult_chroms_fa", "edge"):
        man, seqs, exp = fixture_expected(case)
        fa = os.path.join(GOLDEN, case, "input.fa")
        wp = ["-w", str(man["w"]), "-p", str(man["p"])]
        for name, U in (("pfbwt-f64", 8), ("pfbwt-f", 4)):
            pref = os.path.join(tmp, "%s_%d" % (case, U))
            pr = run([exe[name], "-r", "--thr"] + wp + ["-o", pref, fa])                 # -r alone: the SA stays on the device
            assert "TASK\tthresholds\t" in pr.stderr
            assert same(read_u(pref + ".thr", U), exp.thr), (case, U)
            assert same(read_u(pref + ".tlcp", U), exp.tlcp), (case, U)
            assert not os.path.exists(pref + ".sa") and not os.path.exists(pref + ".lcp")
            mf = man["files"]["u%d" % (U * 8)]
            for e in ("bwt", "ssa", "esa", "dict", "occ", "parse", "bwlast", "ilist", "bwsai", "n"):
                assert sha_f(pref + "." + e) == mf[e]["sha256"], (case, U, e)
            with_thr, without = pref + "_all", pref + "_base"                            # everything in one run
            run([exe[name], "-s", "-r", "--thr", "--lcp", "--da"] + wp + ["-o", with_thr, fa])
            run([exe[name], "-s", "-r", "--lcp", "--da"] + wp + ["-o", without, fa])
            for e in others:
                assert sha_f(with_thr + "." + e) == sha_f(without + "." + e), (case, U, e)
            assert sha_f(with_thr + ".sa") == mf["sa"]["sha256"]
            assert same(read_u(with_thr + ".thr", U), exp.thr) and same(read_u(with_thr + ".tlcp", U), exp.tlcp), (case, U)
            assert same(read_u(with_thr + ".lcp", U), exp.lcp), (case, U)
            assert not os.path.exists(without + ".thr") and not os.path.exists(without + ".tlcp")
    fa = os.path.join(GOLDEN, "edge", "input.fa")
    wp = ["-w", "10", "-p", "20"]

    def refused(args, word, prefix):
        pr = run([exe["pfbwt-f64"]] + args + wp + ["-o", prefix] + ([fa] if "--pfbwt-only" not in args else []), check=False)
        assert pr.returncode != 0 and "--thr" in pr.stderr and word in pr.stderr, pr.stderr[-500:]
        for e in ("bwt", "thr", "tlcp", "sa", "dict"):
            assert not os.path.exists(prefix + "." + e), (args, e)

    refused(["--thr"], "-r", os.path.join(tmp, "no_r"))
    refused(["--thr", "-s"], "-r", os.path.join(tmp, "s_only"))
    refused(["--thr", "-r", "--parse-only"], "--parse-only", os.path.join(tmp, "po"))
    refused(["--thr", "-r", "--gpus", "2"], "--gpus", os.path.join(tmp, "gp"))
    refused(["--thr", "-r", "--pfbwt-only"], "--pfbwt-only", os.path.join(tmp, "pb"))
    assert "--thr" in run([exe["pfbwt-f"], "-h"]).stderr


def test_checkers_agree():
    """brute force and the property checker on a hand-made text with tied minima: they accept the same answer, and the property
    checker refuses every other row of every gap"""
    assert [f for f, _ in pfbwt_hip.ThrInfo._fields_] == ["runs", "none", "long_queries", "max_span"]
    rng = np.random.default_rng(4)
    for t in (b"ACGTACGAACGTNNACGT-ACGTTTTTACG", bytes(rng.choice(list(b"ACGT"), 300).astype(np.uint8)) * 2 + b"NNNN" + bytes(rng.choice(list(b"AC"), 200).astype(np.uint8))):
        n = len(t)
        sa = np.array(sorted(range(n + 1), key=lambda i: t[i:] + b"\x00"), np.int64)
        bwt = np.array([t[i - 1] if i else 0 for i in sa], np.uint8)
        lcp = lcp_numpy(t, sa)
        starts = np.flatnonzero(np.concatenate([[True], bwt[1:] != bwt[:-1]]))
        ssa = pairs(starts, sa[starts])
        j, v, span = thresholds_brute(bwt, lcp, ssa)
        thr, tlcp = pairs(starts, j), pairs(starts, v)
        none, max_span = check_properties(bwt, lcp, ssa, thr, tlcp)
        assert none == int((span == 0).sum()) >= 2 and max_span == int(span.max())
        # the definition, restated with plain loops
        tied = 0
        for k, s in enumerate(starts):
            prev = [i for i in range(s) if bwt[i] == bwt[s]]
            if not prev:
                assert j[k] == 0 and v[k] == 0 and span[k] == 0
                continue
            e = prev[-1]
            gap = [int(x) for x in lcp[e + 1:s + 1]]
            assert v[k] == min(gap) and j[k] == e + 1 + gap.index(min(gap)) and span[k] == s - e
            tied += gap.count(min(gap)) > 1
            for other in range(e, s + 2):                     # every other row, the borders included: refused
                if other == j[k]:
                    continue
                wrong = thr.copy(); wrong[2 * k + 1] = other
                wl = tlcp.copy(); wl[2 * k + 1] = lcp[other] if 0 <= other <= n else 0
                with pytest.raises(AssertionError):
                    check_properties(bwt, lcp, ssa, wrong, wl)
            wl = tlcp.copy(); wl[2 * k + 1] += 1              # the right row with a wrong value: refused
            with pytest.raises(AssertionError):
                check_properties(bwt, lcp, ssa, thr, wl)
        assert tied > 0


# ---- CPU: the emulated library -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pfbwt-f_amd"), "emu", "emu-host"], check=True, stdout=subprocess.DEVNULL)
    return lambda **kw: pfbwt_hip.PfpContext(lib=EMU_SO, **kw)


def test_thresholds_fixtures_emu(emu):
    check_fixtures(emu)


def test_thresholds_seeded_emu(emu):
    check_seeded(emu)


def test_thresholds_cached_and_scratch_rows_emu(emu):
    check_cached_and_scratch(emu)


def test_thresholds_errors_emu(emu):
    check_errors(emu)


def test_thresholds_coexistence_emu(emu):
    check_coexistence(emu)


def test_thresholds_cli_emu(emu, tmp_path):
    check_cli({"pfbwt-f": os.path.join(EMUB, "pfbwt-f-emu"), "pfbwt-f64": os.path.join(EMUB, "pfbwt-f64-emu")}, str(tmp_path))


# ---- GPU: the product library --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_thresholds_fixtures_seeded_gpu(gpu_ctx_factory):
    check_fixtures(gpu_ctx_factory)
    check_seeded(gpu_ctx_factory)


@pytest.mark.gpu
def test_thresholds_routes_errors_gpu(gpu_ctx_factory):
    check_cached_and_scratch(gpu_ctx_factory)
    check_errors(gpu_ctx_factory)
    check_coexistence(gpu_ctx_factory)


@pytest.mark.gpu
def test_thresholds_cli_gpu(gpu_ctx_factory, tmp_path):
    check_cli({"pfbwt-f": os.path.join(BIN, "pfbwt-f"), "pfbwt-f64": os.path.join(BIN, "pfbwt-f64")}, str(tmp_path))


@pytest.mark.gpu
def test_thresholds_medium_panel_gpu(gpu_ctx_factory):
    """64 synthetic haplotypes of 1 Mbase (the panel of test_lcp_array_medium_panel_gpu), -s -r, U = 8 (cached LCP rows) and U = 4
    (rows into scratch, the LCP array fetched afterwards), after check_sa() and check_samples().  EVERY run is checked by
    check_properties at full size, with the default tunables and with thr_long_min = 1 / thr_tile = 16, which must give the same
    arrays.  The lcp the properties are checked against is the engine's own, vouched for here by (a) the structure of the whole array
    (K = lcp + sa in text order, test_lcp_array.check_structure), which with the run-start values determines it, (b) the values of a
    seeded SAMPLE of run starts against direct suffix comparison -- 20 000 of them plus the 1 000 largest; the share is printed and
    asserted to be that sample, not more -- and (c) 20 000 seeded random rows; test_lcp_array_medium_panel_gpu checks the same
    array of the same build at all its run starts."""
    from test_sharded import synth
    from test_lcp_array import check_structure, run_start_values
    seqs = synth(31, 1 << 20, 64)
    w = 10
    text = b"".join(s + b"A" * w for s in seqs)
    n = len(text)
    rng = np.random.default_rng(23)
    for U in (8, 4):
        ctx = build(gpu_ctx_factory, seqs, w, 100, U)
        o = ctx.check_sa()
        assert o["rows"] == n + 1 and o["out_of_range"] == o["duplicates"] == o["bwt_mismatches"] == 0 and o["eos_bytes"] == 1, o
        o = ctx.check_samples()
        assert o["runs"] == ctx.bsizes.r and o["row_errors"] == o["value_errors"] == 0, o
        out = ctx.bwt_get()
        bwt, sa, ssa = out["bwt"], out["sa"].astype(np.int64), out["ssa"].astype(np.uint64)
        if U == 8:
            lcp = ctx.lcp_array()[0]
            thr, tlcp, info = ctx.thresholds()
        else:
            thr, tlcp, info = ctx.thresholds()
            lcp = ctx.lcp_array()[0]
        ctx.debug_set(**FORCED)
        thr2, tlcp2, info2 = ctx.thresholds()
        ctx.close()
        r = ssa.size // 2
        rows = ssa[0::2].astype(np.int64)
        # the lcp: (a) structure, (b) a sample of the run starts, (c) random rows
        check_structure(lcp, sa, ssa[1::2])
        sample = min(20000, r - 1)
        idx = np.unique(np.concatenate([rng.choice(np.arange(1, r), sample, replace=False), 1 + np.argsort(lcp[rows[1:]])[-1000:]]))
        share = idx.size / r
        print("U = %d: r = %d, lcp vouched for at %d run starts (%.2f %% of them), the structure of all rows and 20 000 random rows" % (U, r, idx.size, 100 * share))
        assert sample <= idx.size <= sample + 1000 and share == idx.size / r
        assert same(lcp[rows[idx]], run_start_values(text, sa[rows[idx] - 1], sa[rows[idx]])), U
        pick = rng.integers(1, n + 1, 20000)
        assert same(lcp[pick], run_start_values(text, sa[pick - 1], sa[pick])) and lcp[0] == 0, U
        # the thresholds: every run
        none, max_span = check_properties(bwt, lcp, ssa, thr, tlcp)
        assert same(thr, thr2) and same(tlcp, tlcp2)
        has, e = previous_rows(bwt, rows)
        span = np.where(has, rows - e, 0)
        for inf, lm in ((info, DEFAULTS["thr_long_min"]), (info2, FORCED["thr_long_min"])):
            assert inf == {"runs": r, "none": none, "long_queries": int((span > lm).sum()), "max_span": max_span}, (U, inf)
        assert info2["long_queries"] > 0 and max_span > 2 * DEFAULTS["thr_tile"] and info["long_queries"] > 0, (info, info2)
        print("U = %d: info %s; forced %s" % (U, info, info2))
