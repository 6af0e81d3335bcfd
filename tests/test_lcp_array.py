"""LCP-array post-pass (include/pfbwt_hip.h: pfp_lcp_array; csrc/lcparray.h; pfbwt-f --lcp).

LCP[0] = 0, LCP[i] = longest common prefix of T[SA[i-1] .. n) and T[SA[i] .. n) over the normalised text T with a terminator
smaller than every byte at n.  The expected values never come from the engine: they are computed from the pinned oracle's text
and arrays (on the large GPU inputs: from the text that was fed and the arrays check_sa() / check_samples() vouch for) by
comparing suffixes directly, with two checkers:
* lcp_numpy: an active-set loop over all rows, one byte position per step (exact for every row; small texts);
* pair_lcp: one pair, Python bytes slices, doubling then bisection (run starts and sampled rows of large texts), together with
  the structure check of the whole array: K = lcp + sa scattered to text order is non-decreasing and changes only at the text
  positions of run-start rows (Karkkainen, Manzini, Puglisi, CPM 2009) -- run-start values + that structure determine the array.
Every case runs with the default lcp_long_min and with 16 (most pairs take the wave-per-pair route)."""
import hashlib
import json
import os
import subprocess
import time
import numpy as np
import pytest
from pfp_testlib import EMU_SO, GOLDEN, ROOT, golden_case, oracle_run

import pfbwt_hip

EMUB = os.path.join(ROOT, "tests", "emu", "build")
BIN = os.path.join(ROOT, "pfbwt-f_amd", "bin")
FIXTURES = ["edge", "w4p7", "mult_chroms_fa", "single_chrom", "mult_chroms", "panel8"]


# ---- the checkers ------------------------------------------------------------------------------------------------------------
def lcp_numpy(text, sa):
    """LCP array of T$ by direct comparison: all rows at once, one byte position per step"""
    n = len(text)
    t = np.empty(n + 1, np.int16); t[:n] = np.frombuffer(bytes(text), np.uint8); t[n] = -1      # the terminator: unique, smallest
    sa = np.asarray(sa, np.int64)
    assert sa.size == n + 1 and sa[0] == n
    lcp = np.zeros(n + 1, np.int64)
    rows = np.arange(1, n + 1)
    a, b = sa[:-1].copy(), sa[1:].copy()
    while rows.size:
        eq = t[a] == t[b]                 # (the terminator equals nothing else, so a + h and b + h never pass n)
        rows, a, b = rows[eq], a[eq] + 1, b[eq] + 1
        lcp[rows] += 1
    return lcp.astype(np.uint64)


def pair_lcp(t, a, b):
    """common prefix of t[a:] and t[b:] (bytes; the terminator behind t differs from everything): doubling, then bisection"""
    lim = len(t) - max(a, b)
    lo, k = 0, 1
    while lo < lim:
        k = min(k, lim - lo)
        if t[a + lo:a + lo + k] != t[b + lo:b + lo + k]:
            break
        lo += k; k *= 2
    else:
        return lim
    hi = lo + k                           # t[a + lo : a + hi] != t[b + lo : b + hi], equal in front of lo
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if t[a + lo:a + mid] == t[b + lo:b + mid]:
            lo = mid
        else:
            hi = mid
    return lo


def run_start_values(t, sa_prev, sa_at):
    return np.array([pair_lcp(t, int(a), int(b)) for a, b in zip(sa_prev, sa_at)], np.uint64)


def check_structure(lcp, sa, start_pos):
    """K = lcp + sa in text order: non-decreasing, constant between the text positions of run-start rows"""
    sa = np.asarray(sa, np.int64)
    K = np.empty(sa.size, np.int64); K[sa] = np.asarray(lcp, np.int64) + sa
    d = np.diff(K)
    assert (d >= 0).all(), "K decreases at %d" % int(np.flatnonzero(d < 0)[0])
    irr = np.zeros(sa.size, bool); irr[np.asarray(start_pos, np.int64)] = True
    bad = np.flatnonzero((d != 0) & ~irr[1:])
    assert bad.size == 0, "K changes at the reducible position %d" % int(bad[0] + 1)


def same(a, b):
    return a is not None and b is not None and np.array_equal(np.asarray(a, np.uint64), np.asarray(b, np.uint64))


def expected_slcp(lcp, ssa):
    s = np.asarray(ssa, np.uint64).copy()
    s[1::2] = lcp[s[0::2].astype(np.int64)]
    return s


def info_of(slcp):
    v = np.asarray(slcp[1::2], np.uint64)
    return {"pairs": int(v.size), "max_lcp": int(v.max()) if v.size else 0, "sum_lcp": int(v.sum())}


def build(factory, seqs, w, p, U, sa=True, rssa=True, non_acgt_to_a=False, workspace_bytes=0, **switches):
    ctx = factory(w=w, p=p, u64=(U == 8), sai=True, non_acgt_to_a=non_acgt_to_a, workspace_bytes=workspace_bytes)
    if switches:
        ctx.debug_set(**switches)
    for s in seqs:
        ctx.feed(s, True)
    ctx.finalize(); ctx.parse_bwt(); ctx.bwt_build(sa=sa, rssa=rssa)
    return ctx


def check_against(ctx, lcp_exp, ssa, tag, long_mins=(None, 16)):
    """rows + runs of one build against the expected arrays, with the default single-lane limit and with a small one"""
    slcp_exp = expected_slcp(lcp_exp, ssa)
    want = info_of(slcp_exp)
    for lm in long_mins:
        if lm is not None:
            ctx.debug_set(lcp_long_min=lm)
        lcp, slcp, info = ctx.lcp_array()
        assert same(lcp, lcp_exp), (tag, lm, "lcp")
        assert same(slcp, slcp_exp), (tag, lm, "slcp")
        assert same(slcp[0::2], np.asarray(ssa)[0::2]), (tag, lm, "slcp rows")
        assert {k: info[k] for k in want} == want, (tag, lm, info, want)
        cap = lm or 512       # a value above the limit was finished by a wave, one below it was not (a value equal to it may be either)
        assert int((slcp_exp[1::2] > cap).sum()) <= info["long_pairs"] <= int((slcp_exp[1::2] >= cap).sum()), (tag, lm, info)


_fixture_cache = {}


def fixture_expected(case):
    if case not in _fixture_cache:
        man, recs = golden_case(case)
        seqs = [s for _, s in recs]
        ref = oracle_run(seqs, w=man["w"], p=man["p"], U=8)
        _fixture_cache[case] = (man, seqs, ref, lcp_numpy(ref["text"], ref["sa"]))
    return _fixture_cache[case]


def check_fixtures(factory, cases=FIXTURES):
    for case in cases:
        man, seqs, ref, lcp_exp = fixture_expected(case)
        for U in (4, 8):
            ctx = build(factory, seqs, man["w"], man["p"], U)
            check_against(ctx, lcp_exp, ref["ssa"], (case, U))
            ctx.close()


def seeded_collections(seed):
    """the shapes of test_doc_array.seeded_collections"""
    rng = np.random.default_rng(seed)
    rnd = lambda n: bytes(rng.choice(list(b"ACGT"), int(n)).astype(np.uint8))
    base = rnd(1500)
    mut = lambda: bytes(np.where(rng.random(len(base)) < 0.01, rng.choice(list(b"ACGT"), len(base)), np.frombuffer(base, np.uint8)).astype(np.uint8))
    return {
        "empty_records": [b"", rnd(400), b"", b"", mut(), b""],
        "shorter_than_w": [rnd(1), rnd(3), mut(), rnd(9), rnd(2), rnd(11), mut()],
        "n_run_ends": [mut() + b"N" * 200, mut() + b"N" * 30, rnd(300) + b"N" * 500],
        "single_record": [mut()],
        "panel": [mut() for _ in range(12)],
    }


def check_collection(factory, seqs, w, p, U, tag, non_acgt_to_a=False):
    ref = oracle_run(seqs, w=w, p=p, U=U, non_acgt_to_a=non_acgt_to_a)
    assert ref.get("err") is None, (tag, ref.get("err"))          # a collection the oracle rejects is a test error
    lcp_exp = lcp_numpy(ref["text"], ref["sa"])
    ctx = build(factory, seqs, w, p, U, non_acgt_to_a=non_acgt_to_a)
    check_against(ctx, lcp_exp, ref["ssa"], tag)
    ctx.close()
    return ref, lcp_exp


def check_seeded(factory):
    for seed in (1, 2):
        for name, seqs in seeded_collections(seed).items():
            for w, p in ((10, 100), (4, 7)):
                check_collection(factory, seqs, w, p, 4 if seed == 1 else 8, (seed, name, w, p))
    rng = np.random.default_rng(9)
    base = bytes(rng.choice(list(b"ACGT"), 1200).astype(np.uint8))
    # lower-case input is folded, letters outside ACGT become A: the LCP is that of the NORMALISED text
    lower = [base[:600] + base[600:].lower(), base.lower()[100:900], base[300:]]
    ref, _ = check_collection(factory, lower, 10, 100, 8, "lower_case")
    assert bytes(ref["text"][:1200]) == base
    iupac = bytearray(base + base[:700])
    for k in rng.integers(0, len(iupac), 40):
        iupac[int(k)] = int(rng.choice(list(b"RYKMSWn")))
    ref, _ = check_collection(factory, [bytes(iupac), base[200:]], 4, 7, 4, "non_acgt_to_a", non_acgt_to_a=True)
    assert set(bytes(ref["text"])) <= set(b"ACGT")


def long_pair_records(L, seed=21):
    rng = np.random.default_rng(seed)
    rnd = lambda n: bytes(rng.choice(list(b"ACGT"), int(n)).astype(np.uint8))
    return [rnd(3000) + b"C" + b"N" * L, rnd(2500) + b"G" + b"N" * L, rnd(2000)]


def check_long_pair(factory, L, U, arrays_from_engine):
    """records R1 + N^L, R2 + N^L: the rows N^L A^w ... of the two records are adjacent and start different runs (C / G in front),
    so one run-start value is L + w -- reached by the wave-per-pair route WITHOUT forcing it"""
    w, p = 10, 100
    seqs = long_pair_records(L)
    # (nearly all of this text is two dictionary words: the suffix sort of a dictionary as long as the text asks for more than the
    # default workspace of 96 bytes per base, so the large case names its workspace -- an address range, committed on demand)
    ctx = build(factory, seqs, w, p, U, workspace_bytes=(4 << 30) if L > 1000000 else 0)
    if arrays_from_engine:
        o = ctx.check_sa()
        assert o["out_of_range"] == o["duplicates"] == o["bwt_mismatches"] == 0 and o["eos_bytes"] == 1, o
        o = ctx.check_samples()
        assert o["runs"] == ctx.bsizes.r and o["row_errors"] == o["value_errors"] == 0, o
        out = ctx.bwt_get()
        text = b"".join(s + b"A" * w for s in seqs)
        sa, ssa, esa = out["sa"].astype(np.uint64), out["ssa"].astype(np.uint64), out["esa"].astype(np.uint64)
    else:
        ref = oracle_run(seqs, w=w, p=p, U=U)
        text, sa, ssa, esa = bytes(ref["text"]), ref["sa"], ref["ssa"], ref["esa"]
    lcp, slcp, info = ctx.lcp_array()
    ctx.close()
    assert info["max_lcp"] >= L + w and info["long_pairs"] >= 1, info
    assert same(slcp[0::2], ssa[0::2])
    rows = ssa[0::2].astype(np.int64)
    exp = np.zeros(rows.size, np.uint64)
    exp[1:] = run_start_values(text, sa[rows[1:] - 1], sa[rows[1:]])           # (a) every run-start value
    assert same(slcp[1::2], exp), int(np.flatnonzero(slcp[1::2] != exp)[0])
    assert same(lcp[rows], exp)
    check_structure(lcp, sa, ssa[1::2])                                        # (b) the rest of the array
    assert {k: info[k] for k in ("pairs", "max_lcp", "sum_lcp")} == info_of(slcp)
    assert int(exp.max()) >= L + w
    return info


def check_routes(factory):
    """run starts from bwt / sa (no samples) and runs without a full SA"""
    man, seqs, ref, lcp_exp = fixture_expected("mult_chroms_fa")
    slcp_exp = expected_slcp(lcp_exp, ref["ssa"])
    for U in (4, 8):
        for lm in (512, 16):
            ctx = build(factory, seqs, man["w"], man["p"], U, sa=True, rssa=False, lcp_long_min=lm)
            lcp, slcp, info = ctx.lcp_array(runs=False)
            assert same(lcp, lcp_exp) and slcp is None, (U, lm)
            assert {k: info[k] for k in ("pairs", "max_lcp", "sum_lcp")} == info_of(slcp_exp), info
            with pytest.raises(pfbwt_hip.PfpError) as e:
                ctx.lcp_array(rows=False, runs=True)
            assert e.value.status == pfbwt_hip.E_STATE
            ctx.close()
            ctx = build(factory, seqs, man["w"], man["p"], U, sa=False, rssa=True, lcp_long_min=lm)
            lcp, slcp, info = ctx.lcp_array(rows=False)
            assert same(slcp, slcp_exp) and lcp is None, (U, lm)
            with pytest.raises(pfbwt_hip.PfpError) as e:
                ctx.lcp_array(rows=True, runs=False)
            assert e.value.status == pfbwt_hip.E_STATE
            assert same(ctx.lcp_array(rows=False)[1], slcp_exp)              # still usable
            ctx.close()


def check_slices(factory):
    rng = np.random.default_rng(3)
    seqs = [bytes(rng.choice(list(b"ACGT"), int(n)).astype(np.uint8)) for n in rng.integers(200, 900, 9)]
    seqs[4] = seqs[1][:150] + seqs[4]; seqs[7] = seqs[1]                       # some long common prefixes
    w, p = 4, 7
    ref = oracle_run(seqs, w=w, p=p, U=8)
    slcp_exp = expected_slcp(lcp_numpy(ref["text"], ref["sa"]), ref["ssa"])
    for U in (4, 8):
        for lm in (512, 16):
            ctx = build(factory, seqs, w, p, U, lcp_long_min=lm)
            assert same(ctx.lcp_array(rows=False)[1], slcp_exp)
            for ns in (1, 3, 7):
                parts, pairs = [], 0
                for sl in range(ns):
                    ctx.bwt_build_slice(sl, ns, sa=True, rssa=True)
                    if ns > 1:
                        with pytest.raises(pfbwt_hip.PfpError) as e:
                            ctx.lcp_array(rows=True, runs=False)
                        assert e.value.status == pfbwt_hip.E_STATE
                    _, s, info = ctx.lcp_array(rows=False, runs=True)
                    assert s.size == 2 * ctx.bsizes.r
                    parts.append(s); pairs += info["pairs"]
                assert same(np.concatenate(parts), slcp_exp), (U, lm, ns)
                assert pairs == slcp_exp.size // 2
            ctx.close()


def check_errors(factory):
    E_ARG, E_STATE = pfbwt_hip.E_ARG, pfbwt_hip.E_STATE
    man, seqs, ref, lcp_exp = fixture_expected("mult_chroms_fa")
    w, p = man["w"], man["p"]

    def status(ctx, **kw):
        with pytest.raises(pfbwt_hip.PfpError) as e:
            ctx.lcp_array(**kw)
        return e.value.status

    ctx = factory(w=w, p=p, u64=True, sai=True)                       # no build at all
    assert ctx.L.pfp_lcp_array(ctx.h, pfbwt_hip.LCP_ROWS, None) == E_STATE
    for s in seqs:
        ctx.feed(s, True)
    ctx.finalize(); ctx.parse_bwt()
    assert ctx.L.pfp_lcp_array(ctx.h, pfbwt_hip.LCP_RUNS, None) == E_STATE      # parsed, not built
    ctx.bwt_build(sa=True, rssa=True)
    assert status(ctx, rows=False, runs=False) == E_ARG               # what = 0
    assert ctx.L.pfp_lcp_array(ctx.h, 4, None) == E_ARG and ctx.L.pfp_lcp_array(ctx.h, 7, None) == E_ARG
    assert ctx.L.pfp_lcp_array_get(ctx.h, lcp_exp.ctypes.data_as(pfbwt_hip.C.c_void_p), None) == E_STATE      # nothing made yet
    lcp, slcp, _ = ctx.lcp_array()                                    # the context is still usable
    assert same(lcp, lcp_exp)
    _, s2, _ = ctx.lcp_array(rows=False)                              # a second call replaces the first: no .lcp any more
    assert same(s2, slcp)
    assert ctx.L.pfp_lcp_array_get(ctx.h, lcp_exp.ctypes.data_as(pfbwt_hip.C.c_void_p), None) == E_STATE
    assert ctx.lcp_array_device_ptrs()[0] is None and ctx.lcp_array_device_ptrs()[1]
    ctx.bwt_build(sa=False, rssa=False)                               # a new build drops the arrays; BWT only: nothing to work from
    assert ctx.lcp_array_device_ptrs() == [None, None]
    assert status(ctx) == E_STATE and status(ctx, runs=False) == E_STATE and status(ctx, rows=False) == E_STATE
    ctx.close()
    ctx = factory(w=w, p=p, u64=True, sai=True)                       # a loaded parse: no text in the context
    ctx.bwt_load(ref["dict"], ref["occ"], ref["bwlast"], ref["ilist"], ref["bwsai"], n_hint=ref["n"])
    ctx.bwt_build(sa=True, rssa=True)
    assert status(ctx) == E_STATE and status(ctx, rows=False) == E_STATE
    assert np.array_equal(ctx.bwt_get()["sa"].astype(np.uint64), ref["sa"])
    ctx.close()
    half = len(seqs) // 2 or 1                                       # a merge of two shards: no text either
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
    assert status(g) == E_STATE and status(g, rows=False) == E_STATE
    assert np.array_equal(g.bwt_get()["sa"].astype(np.uint64), ref["sa"])
    for c in ctxs + [g]:
        c.close()


def check_coexistence(factory):
    """doc_array then lcp_array and the reverse, and repeated calls: all five arrays still fetchable and unchanged"""
    man, seqs, ref, lcp_exp = fixture_expected("mult_chroms_fa")
    b = pfbwt_hip.doc_starts([len(s) for s in seqs], man["w"])
    slcp_exp = expected_slcp(lcp_exp, ref["ssa"])
    C = pfbwt_hip.C

    def fetch(ctx, U):
        dt = np.uint64 if U == 8 else np.uint32
        r, ep, rows = ctx.bsizes.r, ctx.esa_pairs, ctx._rows
        da, sda, eda = np.empty(rows, dt), np.empty(2 * r, dt), np.empty(2 * ep, dt)
        lcp, slcp = np.empty(rows, dt), np.empty(2 * r, dt)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert ctx.L.pfp_doc_array_get(ctx.h, p(da), p(sda), p(eda)) == 0
        assert ctx.L.pfp_lcp_array_get(ctx.h, p(lcp), p(slcp)) == 0
        return da, sda, eda, lcp, slcp

    for U in (8, 4):
        for order in ("da_lcp", "lcp_da", "da_lcp_da_lcp", "lcp_da_lcp_lcp_da"):
            ctx = build(factory, seqs, man["w"], man["p"], U)
            das = None
            for step in order.split("_"):
                if step == "da":
                    das = ctx.doc_array(b)
                else:
                    ctx.lcp_array()
            got = fetch(ctx, U)
            for k in range(3):
                assert same(got[k], das[k]), (U, order, k)
            assert same(got[3], lcp_exp) and same(got[4], slcp_exp), (U, order)
            out = ctx.bwt_get()
            assert same(out["sa"], ref["sa"]) and same(out["ssa"], ref["ssa"]) and same(out["bwt"], ref["bwt"]), (U, order)
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
    for case in ("mult_chroms_fa", "edge"):
        man, seqs, ref, lcp_exp = fixture_expected(case)
        slcp_exp = expected_slcp(lcp_exp, ref["ssa"])
        fa = os.path.join(GOLDEN, case, "input.fa")
        wp = ["-w", str(man["w"]), "-p", str(man["p"])]
        for name, U in (("pfbwt-f64", 8), ("pfbwt-f", 4)):
            pref = os.path.join(tmp, "%s_%d" % (case, U))
            pr = run([exe[name], "-s", "-r", "--lcp"] + wp + ["-o", pref, fa])
            assert "TASK\tLCP array\t" in pr.stderr
            mf = man["files"]["u%d" % (U * 8)]
            for e in ("bwt", "sa", "ssa", "esa", "dict", "occ", "parse", "bwlast", "ilist", "bwsai", "n"):
                assert sha_f(pref + "." + e) == mf[e]["sha256"], (case, U, e)     # every other file as without --lcp
            assert os.path.getsize(pref + ".lcp") == os.path.getsize(pref + ".sa")
            assert same(read_u(pref + ".lcp", U), lcp_exp), (case, U)
            assert same(read_u(pref + ".slcp", U), slcp_exp), (case, U)
            p2 = pref + "_r"                                                       # -r alone: .slcp only
            run([exe[name], "-r", "--lcp"] + wp + ["-o", p2, fa])
            assert same(read_u(p2 + ".slcp", U), slcp_exp) and not os.path.exists(p2 + ".lcp") and not os.path.exists(p2 + ".sa")
            assert sha_f(p2 + ".ssa") == mf["ssa"]["sha256"] and sha_f(p2 + ".bwt") == mf["bwt"]["sha256"]
    # refusals: a message that names the cause, no output files
    fa = os.path.join(GOLDEN, "edge", "input.fa")
    wp = ["-w", "10", "-p", "20"]

    def refused(args, word, prefix):
        pr = run([exe["pfbwt-f64"]] + args + wp + ["-o", prefix] + ([fa] if "--pfbwt-only" not in args else []), check=False)
        assert pr.returncode != 0 and "--lcp" in pr.stderr and word in pr.stderr, pr.stderr[-500:]
        for e in ("bwt", "lcp", "slcp", "sa", "dict"):
            assert not os.path.exists(prefix + "." + e), (args, e)

    refused(["--lcp"], "-s", os.path.join(tmp, "no_s"))
    refused(["--lcp", "-s", "--parse-only"], "--parse-only", os.path.join(tmp, "po"))
    refused(["--lcp", "-s", "--gpus", "2"], "--gpus", os.path.join(tmp, "gp"))
    refused(["--lcp", "-s", "--pfbwt-only"], "--pfbwt-only", os.path.join(tmp, "pb"))
    assert "--lcp" in run([exe["pfbwt-f"], "-h"]).stderr


def test_checkers_agree():
    """the two checkers against each other and against a hand-made case"""
    t = b"ACGTACGAACGT"
    n = len(t)
    sa = sorted(range(n + 1), key=lambda i: t[i:] + b"\x00")      # (0x00 < every base)
    lcp = lcp_numpy(t, sa)
    for i in range(1, n + 1):
        a, b = t[sa[i - 1]:], t[sa[i]:]
        k = 0
        while k < min(len(a), len(b)) and a[k] == b[k]:
            k += 1
        assert lcp[i] == k == pair_lcp(t, sa[i - 1], sa[i])
    assert lcp[0] == 0 and pair_lcp(b"AAAAAAAAAA", 0, 3) == 7 and pair_lcp(b"AAAAACAAAAAT", 0, 6) == 5


# ---- CPU: the emulated library -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pfbwt-f_amd"), "emu", "emu-host"], check=True, stdout=subprocess.DEVNULL)
    return lambda **kw: pfbwt_hip.PfpContext(lib=EMU_SO, **kw)


def test_lcp_array_fixtures_emu(emu):
    check_fixtures(emu)


def test_lcp_array_seeded_emu(emu):
    check_seeded(emu)


def test_lcp_array_long_pair_emu(emu):
    """L = 40 000 (oracle run: 5 524 runs, largest run-start value 40 011): the default lcp_long_min lies below it"""
    check_long_pair(emu, 40000, 8, arrays_from_engine=False)
    check_long_pair(emu, 40000, 4, arrays_from_engine=False)


def test_lcp_array_routes_emu(emu):
    check_routes(emu)


def test_lcp_array_slices_emu(emu):
    check_slices(emu)


def test_lcp_array_errors_coexistence_emu(emu):
    check_errors(emu)
    check_coexistence(emu)


def test_lcp_array_cli_emu(emu, tmp_path):
    check_cli({"pfbwt-f": os.path.join(EMUB, "pfbwt-f-emu"), "pfbwt-f64": os.path.join(EMUB, "pfbwt-f64-emu")}, str(tmp_path))


# ---- GPU: the product library --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lcp_array_fixtures_seeded_gpu(gpu_ctx_factory):
    check_fixtures(gpu_ctx_factory)
    check_seeded(gpu_ctx_factory)


@pytest.mark.gpu
def test_lcp_array_long_pair_gpu(gpu_ctx_factory):
    """L = 3 000 000: run-start values by pair_lcp on the arrays check_sa / check_samples vouch for, the rest by structure"""
    check_long_pair(gpu_ctx_factory, 40000, 8, arrays_from_engine=False)
    info = check_long_pair(gpu_ctx_factory, 3000000, 8, arrays_from_engine=True)
    print("long pair, L = 3 000 000, U = 8:", info)
    check_long_pair(gpu_ctx_factory, 3000000, 4, arrays_from_engine=True)


@pytest.mark.gpu
def test_lcp_array_routes_slices_errors_gpu(gpu_ctx_factory):
    check_routes(gpu_ctx_factory)
    check_slices(gpu_ctx_factory)
    check_errors(gpu_ctx_factory)
    check_coexistence(gpu_ctx_factory)


@pytest.mark.gpu
def test_lcp_array_medium_panel_gpu(gpu_ctx_factory):
    """64 synthetic haplotypes of 1 Mbase, -s -r, U = 8 and 4, after check_sa() and check_samples(): (a) the value of every run
    start against pair_lcp -- ALL r run starts unless that is projected to take more than five minutes, then a seeded sample of
    200 000 run starts plus the 1 000 largest values (the test prints which was used, and r); (b) the structure of the whole array;
    (c) 20 000 seeded random rows by direct comparison; (d) info.max_lcp == max(slcp values) == check_sample_order()["max_lcp"]."""
    from test_sharded import synth
    seqs = synth(31, 1 << 20, 64)
    w = 10
    text = b"".join(s + b"A" * w for s in seqs)
    n = len(text)
    rng = np.random.default_rng(17)
    for U in (8, 4):
        ctx = build(gpu_ctx_factory, seqs, w, 100, U)
        o = ctx.check_sa()
        assert o["rows"] == n + 1 and o["out_of_range"] == o["duplicates"] == o["bwt_mismatches"] == 0 and o["eos_bytes"] == 1, o
        o = ctx.check_samples()
        assert o["runs"] == ctx.bsizes.r and o["row_errors"] == o["value_errors"] == 0, o
        order = ctx.check_sample_order()
        out = ctx.bwt_get()
        sa, ssa = out["sa"].astype(np.int64), out["ssa"].astype(np.int64)
        lcp, slcp, info = ctx.lcp_array()
        ctx.close()
        r = ssa.size // 2
        rows, vals = ssa[0::2], slcp[1::2].astype(np.uint64)
        assert same(slcp[0::2], rows) and same(lcp[rows], vals) and vals[0] == 0 and rows[0] == 0
        # (a)
        t0 = time.time()
        probe = min(r - 1, 50000)
        idx = np.arange(1, r)
        exp = run_start_values(text, sa[rows[1:probe + 1] - 1], sa[rows[1:probe + 1]])
        per_pair = (time.time() - t0) / max(probe, 1)
        if per_pair * r <= 300:
            exp = np.concatenate([exp, run_start_values(text, sa[rows[probe + 1:] - 1], sa[rows[probe + 1:]])])
            used = "all %d run starts" % r
        else:
            idx = np.unique(np.concatenate([rng.choice(np.arange(1, r), 200000, replace=False), 1 + np.argsort(vals[1:])[-1000:]]))
            exp = run_start_values(text, sa[rows[idx] - 1], sa[rows[idx]])
            used = "a seeded sample of %d of the %d run starts (with the 1 000 largest values)" % (idx.size, r)
        print("U = %d: r = %d, run-start values checked on %s in %.1f s; info %s" % (U, r, used, time.time() - t0, info))
        bad = np.flatnonzero(vals[idx] != exp)
        assert bad.size == 0, (U, int(idx[bad[0]]), int(vals[idx[bad[0]]]), int(exp[bad[0]]))
        # (b)
        check_structure(lcp, sa, ssa[1::2])
        # (c)
        pick = rng.integers(1, n + 1, 20000)
        assert same(lcp[pick], run_start_values(text, sa[pick - 1], sa[pick])), U
        assert lcp[0] == 0
        # (d)
        assert info["max_lcp"] == int(vals.max()) == order["max_lcp"], (info, order)
        assert info["pairs"] == r and info["sum_lcp"] == int(vals.sum())


@pytest.mark.gpu
def test_lcp_array_cli_gpu(gpu_ctx_factory, tmp_path):
    check_cli({"pfbwt-f": os.path.join(BIN, "pfbwt-f"), "pfbwt-f64": os.path.join(BIN, "pfbwt-f64")}, str(tmp_path))
