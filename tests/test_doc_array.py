"""Document-array post-pass (include/pfbwt_hip.h: pfp_doc_array; csrc/docarray.h; pfbwt-f --da).

doc(s) = max{k : b_k <= s} over the record starts b_k (the values of .docs).  The checker is numpy over the pinned oracle's arrays:
np.searchsorted(b, sa, side="right") - 1 on the SA and on the value half of the .ssa / .esa pairs.
* fixtures (3, 8, 2 and 1 records) and seeded collections (empty records, records shorter than w, records ending in N runs, one
  record), U = 4 and 8, the LDS route and the two-level route (forced through doc_lds_max, and reached with > 8192 records);
* slices 1, 3, 7 of pfp_bwt_build_slice, a merge of two shards, pfp_sharded_* with three ranks: equal to the single-context result;
* error codes; the command line (--da; --pfbwt-only from .docs, also a merge_pfp --docs merge; the refusals)."""
import hashlib
import os
import subprocess
import numpy as np
import pytest
from pfp_testlib import EMU_SO, GOLDEN, ROOT, golden_case, oracle_run

import pfbwt_hip

EMUB = os.path.join(ROOT, "tests", "emu", "build")
BIN = os.path.join(ROOT, "pfbwt-f_amd", "bin")


def doc_of(b, v):
    return (np.searchsorted(np.asarray(b, np.uint64), np.asarray(v, np.uint64), side="right") - 1).astype(np.uint64)


def expected(b, sa, ssa, esa):
    """numpy over SA values: (da, sda, eda)"""
    sda = np.asarray(ssa, np.uint64).copy(); eda = np.asarray(esa, np.uint64).copy()
    sda[1::2] = doc_of(b, sda[1::2]); eda[1::2] = doc_of(b, eda[1::2])
    return (doc_of(b, sa) if sa is not None else None), sda, eda


def same(a, b):
    return a is not None and b is not None and np.array_equal(np.asarray(a, np.uint64), np.asarray(b, np.uint64))


def build(factory, seqs, w, p, U, sa=True, rssa=True, **switches):
    ctx = factory(w=w, p=p, u64=(U == 8), sai=True)
    if switches:
        ctx.debug_set(**switches)
    for s in seqs:
        ctx.feed(s, True)
    ctx.finalize(); ctx.parse_bwt(); ctx.bwt_build(sa=sa, rssa=rssa)
    return ctx


def check_collection(factory, seqs, w, p, U, tag, lds=(8192, 2)):
    ref = oracle_run(seqs, w=w, p=p, U=U)
    if ref.get("err") == "one_word":
        return False
    b = pfbwt_hip.doc_starts([len(s) for s in seqs], w)
    exp = expected(b, ref["sa"], ref["ssa"], ref["esa"])
    ctx = build(factory, seqs, w, p, U)
    for m in lds:      # the route is chosen per call: one build, both routes
        ctx.debug_set(doc_lds_max=m)
        got = ctx.doc_array(b)
        for name, g, e in zip(("da", "sda", "eda"), got, exp):
            assert same(g, e), (tag, U, m, name)
    ctx.close()
    return True


FIXTURES = ["mult_chroms_fa", "panel8", "edge", "single_chrom", "mult_chroms"]


def check_fixtures(factory):
    for case in FIXTURES:
        man, recs = golden_case(case)
        seqs = [s for _, s in recs]
        b = pfbwt_hip.doc_starts([len(s) for s in seqs], man["w"])
        docs = os.path.join(GOLDEN, case, "u64.docs")
        if os.path.exists(docs):      # the reference's .docs holds b_k
            assert [int(l.split()[1]) for l in open(docs)] == b.tolist(), case
        for U in (4, 8):
            assert check_collection(factory, seqs, man["w"], man["p"], U, case)
        if len(seqs) == 1:
            ctx = build(factory, seqs, man["w"], man["p"], 8)
            da, sda, eda = ctx.doc_array(b)
            assert not da.any() and not sda[1::2].any() and not eda[1::2].any()
            ctx.close()


def seeded_collections(seed):
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


def check_seeded(factory):
    for seed in (1, 2):
        for name, seqs in seeded_collections(seed).items():
            for w, p in ((10, 100), (4, 7)):
                assert check_collection(factory, seqs, w, p, 4 if seed == 1 else 8, (seed, name, w, p), lds=(8192, 3)), (name, "one word")


def check_many_records(factory):
    """> 8192 records: the two-level route without forcing it (and row 0 in the last record)"""
    rng = np.random.default_rng(7)
    seqs = [bytes(rng.choice(list(b"ACGT"), int(n)).astype(np.uint8)) for n in rng.integers(0, 6, 9000)]
    assert check_collection(factory, seqs, 2, 5, 8, "many", lds=(8192,))


def check_slices(factory):
    rng = np.random.default_rng(3)
    seqs = [bytes(rng.choice(list(b"ACGT"), int(n)).astype(np.uint8)) for n in rng.integers(200, 900, 9)]
    w, p = 4, 7
    b = pfbwt_hip.doc_starts([len(s) for s in seqs], w)
    for U in (4, 8):
        ctx = build(factory, seqs, w, p, U)
        whole = ctx.doc_array(b)
        assert same(whole[0], expected(b, ctx.bwt_get()["sa"], [], [])[0])
        for ns in (1, 3, 7):
            parts = [[], [], []]
            for sl in range(ns):
                ctx.bwt_build_slice(sl, ns, sa=True, rssa=True)
                got = ctx.doc_array(b, rows=True, runs=True)
                assert got[2].size == 2 * ctx.esa_pairs
                for k in range(3):
                    parts[k].append(got[k])
            for k in range(3):
                assert same(np.concatenate(parts[k]), whole[k]), (U, ns, k)
        ctx.close()


def check_merge(factory, seqs, w, p, U):
    ref = oracle_run(seqs, w=w, p=p, U=U)
    b = pfbwt_hip.doc_starts([len(s) for s in seqs], w)
    exp = expected(b, ref["sa"], ref["ssa"], ref["esa"])
    half = len(seqs) // 2
    ctxs, views = [], []
    for r, grp in enumerate((seqs[:half], seqs[half:])):
        c = factory(w=w, p=p, u64=(U == 8), sai=True)
        if r:
            c.feed_left_context(w)
        for s in grp:
            c.feed(s, True)
        c.finalize(shard=True)
        ctxs.append(c); views.append(c.shard_view())
    g = factory(w=w, p=p, u64=(U == 8), sai=True)
    g.merge_shards(views); g.parse_bwt(); g.bwt_build(sa=True, rssa=True)
    got = g.doc_array(b)
    for k in range(3):
        assert same(got[k], exp[k]), ("merge", k)
    for c in ctxs + [g]:
        c.close()
    return exp


def check_sharded(lib, seqs, w, p, U, exp):
    b = pfbwt_hip.doc_starts([len(s) for s in seqs], w)
    shards = [[0], [1, 2], list(range(3, len(seqs)))]
    sb = pfbwt_hip.ShardedBuild(3, devices=[0, 0, 0], w=w, p=p, u64=(U == 8), lib=lib)
    for r, grp in enumerate(shards):
        for i in grp:
            sb.rank(r).feed(seqs[i], True)
    sb.build(sa=True, rssa=True)
    parts = [[], [], []]
    for r in range(3):
        got = sb.rank(r).doc_array(b)      # every rank: the whole collection's table
        for k in range(3):
            parts[k].append(got[k])
    for k in range(3):
        assert same(np.concatenate(parts[k]), exp[k]), ("sharded", k)
    sb.close()


def check_errors(factory):
    E_ARG, E_STATE = pfbwt_hip.E_ARG, pfbwt_hip.E_STATE
    rng = np.random.default_rng(5)
    seqs = [bytes(rng.choice(list(b"ACGT"), 700).astype(np.uint8)) for _ in range(3)]
    b = pfbwt_hip.doc_starts([700] * 3, 10)
    n = 3 * 710

    def status(ctx, starts, rows=True, runs=True):
        with pytest.raises(pfbwt_hip.PfpError) as e:
            ctx.doc_array(np.asarray(starts, np.uint64), rows=rows, runs=runs)
        return e.value.status

    ctx = build(factory, seqs, 10, 100, 8)
    assert status(ctx, [0, 900, 800]) == E_ARG           # not ascending
    assert status(ctx, [0, 710, 710]) == E_ARG           # not strictly ascending
    assert status(ctx, [5, 710, 1420]) == E_ARG          # does not start at 0
    assert status(ctx, [0, 710, n]) == E_ARG             # a start >= n
    assert ctx.doc_array(b)[0].size == n + 1             # the context is still usable
    ctx.close()
    ctx = build(factory, seqs, 10, 100, 8, sa=False, rssa=False)      # BWT only
    assert status(ctx, b) == E_STATE and status(ctx, b, runs=False) == E_STATE and status(ctx, b, rows=False) == E_STATE
    ctx.close()
    ctx = build(factory, seqs, 10, 100, 8, sa=False, rssa=True)       # rows without SA
    assert status(ctx, b, rows=True, runs=False) == E_STATE
    assert ctx.doc_array(b, rows=False)[1].size == 2 * ctx.bsizes.r
    ctx.close()
    ctx = build(factory, seqs, 10, 100, 4, sa=True, rssa=False)       # runs without samples
    assert status(ctx, b, rows=False, runs=True) == E_STATE
    assert ctx.doc_array(b, runs=False)[0].size == n + 1
    ctx.close()
    ctx = factory(w=10, p=100, u64=True, sai=True)                    # no build at all
    assert status(ctx, b) == E_STATE
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


def check_cli(exe, merge, tmp):
    """exe: {'pfbwt-f': path, 'pfbwt-f64': path}"""
    import json
    for case in ("mult_chroms_fa", "edge"):
        man = json.load(open(os.path.join(GOLDEN, case, "manifest.json")))
        fa = os.path.join(GOLDEN, case, "input.fa")
        b = [int(l.split()[1]) for l in open(os.path.join(GOLDEN, case, "u64.docs"))]
        ref = None
        for name, U in (("pfbwt-f64", 8), ("pfbwt-f", 4)):
            pref = os.path.join(tmp, "%s_%d" % (case, U))
            wp = ["-w", str(man["w"]), "-p", str(man["p"])]
            run([exe[name], "-s", "-r", "--da"] + wp + ["-o", pref, fa])
            mf = man["files"]["u%d" % (U * 8)]
            for e in ("bwt", "sa", "ssa", "esa", "dict", "occ", "parse", "bwlast", "ilist", "bwsai", "n"):
                assert sha_f(pref + "." + e) == mf[e]["sha256"], (case, U, e)     # every other file as without --da
            assert not os.path.exists(pref + ".docs")                              # .docs only with --print-docs
            exp = expected(b, read_u(pref + ".sa", U), read_u(pref + ".ssa", U), read_u(pref + ".esa", U))
            for e, x in zip(("da", "sda", "eda"), exp):
                assert same(read_u(pref + "." + e, U), x), (case, U, e)
            if U == 8:
                ref = {e: open(pref + "." + e, "rb").read() for e in ("da", "sda", "eda")}
            # the two-stage form: --parse-only --print-docs, then --pfbwt-only --da from .docs
            p2 = pref + "_2"
            run([exe[name], "--parse-only", "--print-docs", "-s"] + wp + ["-o", p2, fa])
            run([exe[name], "--pfbwt-only", "-s", "-r", "--da"] + wp + ["-o", p2])
            for e in ("da", "sda", "eda"):
                assert open(p2 + "." + e, "rb").read() == open(pref + "." + e, "rb").read(), (case, U, e)
        # three parts parsed on their own with --print-docs, merged with merge_pfp --docs, --pfbwt-only --da on the merge
        if case == "edge":
            continue
        recs = golden_case(case)[1]
        parts = []
        for i, (nm, s) in enumerate(recs):
            q = os.path.join(tmp, "part%d.fa" % i)
            open(q, "wb").write(b">" + nm.encode() + b"\n" + s + b"\n")
            run([exe["pfbwt-f64"], "--parse-only", "--print-docs", "-s", "-w", str(man["w"]), "-p", str(man["p"]), "-o", q, q])
            parts.append(q)
        mg = os.path.join(tmp, "merged")
        run([merge, "-w", str(man["w"]), "-p", str(man["p"]), "-s", "--parse-bwt", "--docs", "-o", mg] + parts)
        assert [int(l.split()[1]) for l in open(mg + ".docs")] == b                  # a merged .docs holds b_k too
        run([exe["pfbwt-f64"], "--pfbwt-only", "-s", "-r", "--da", "-w", str(man["w"]), "-p", str(man["p"]), "-o", mg])
        for e in ("da", "sda", "eda"):
            assert open(mg + "." + e, "rb").read() == ref[e], ("merge", e)
    # refusals
    fa = os.path.join(GOLDEN, "edge", "input.fa")
    p3 = os.path.join(tmp, "nodocs2")
    run([exe["pfbwt-f64"], "--parse-only", "-s", "-w", "10", "-p", "20", "-o", p3, fa])     # a parse without .docs
    pr = run([exe["pfbwt-f64"], "--pfbwt-only", "-s", "--da", "-w", "10", "-p", "20", "-o", p3], check=False)
    assert pr.returncode != 0 and ".docs" in pr.stderr and not os.path.exists(p3 + ".da")
    pr = run([exe["pfbwt-f64"], "--da", "-w", "10", "-p", "20", "-o", os.path.join(tmp, "nos"), fa], check=False)
    assert pr.returncode != 0 and "-s" in pr.stderr and not os.path.exists(os.path.join(tmp, "nos.bwt"))
    pr = run([exe["pfbwt-f"], "--da", "-s", "--gpus", "2", "-o", os.path.join(tmp, "g"), fa], check=False)
    assert pr.returncode != 0 and "--gpus" in pr.stderr
    assert "--da" in run([exe["pfbwt-f"], "-h"]).stderr


def test_doc_starts_helper():
    assert pfbwt_hip.doc_starts([5, 0, 3, 7], 10).tolist() == [0, 15, 25, 38]
    assert pfbwt_hip.doc_starts([100] * 4, 4).tolist() == [0, 104, 208, 312]      # a device batch: k * (len + w)
    assert pfbwt_hip.doc_starts([9], 10).tolist() == [0]


# ---- CPU: the emulated library -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pfbwt-f_amd"), "emu", "emu-host"], check=True, stdout=subprocess.DEVNULL)
    return lambda **kw: pfbwt_hip.PfpContext(lib=EMU_SO, **kw)


def test_doc_array_fixtures_emu(emu):
    check_fixtures(emu)


def test_doc_array_seeded_emu(emu):
    check_seeded(emu)


def test_doc_array_two_level_many_records_emu(emu):
    check_many_records(emu)


def test_doc_array_slices_emu(emu):
    check_slices(emu)


def test_doc_array_merge_and_sharded_emu(emu):
    from test_sharded import synth
    seqs = synth(5, 3000, 5)
    exp = check_merge(emu, seqs, 10, 100, 8)
    check_sharded(EMU_SO, seqs, 10, 100, 8, exp)


def test_doc_array_errors_emu(emu):
    check_errors(emu)


def test_doc_array_cli_emu(emu, tmp_path):
    check_cli({"pfbwt-f": os.path.join(EMUB, "pfbwt-f-emu"), "pfbwt-f64": os.path.join(EMUB, "pfbwt-f64-emu")}, os.path.join(EMUB, "merge_pfp-emu"), str(tmp_path))


# ---- GPU: the product library --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_doc_array_fixtures_routes_gpu(gpu_ctx_factory):
    check_fixtures(gpu_ctx_factory)
    check_seeded(gpu_ctx_factory)
    check_many_records(gpu_ctx_factory)


@pytest.mark.gpu
def test_doc_array_slices_errors_gpu(gpu_ctx_factory):
    check_slices(gpu_ctx_factory)
    check_errors(gpu_ctx_factory)


@pytest.mark.gpu
def test_doc_array_medium_panel_gpu(gpu_ctx_factory):
    """64 synthetic haplotypes of 1 Mbase, -s -r: the device's own SA and samples (checked by check_sa / check_samples) against
    the document arrays fetched from the device"""
    from test_sharded import synth
    seqs = synth(31, 1 << 20, 64)
    b = pfbwt_hip.doc_starts([len(s) for s in seqs], 10)
    for U in (8, 4):
        ctx = build(gpu_ctx_factory, seqs, 10, 100, U)
        o = ctx.check_sa()
        assert o["rows"] == 64 * ((1 << 20) + 10) + 1 and o["out_of_range"] == o["duplicates"] == o["bwt_mismatches"] == 0 and o["eos_bytes"] == 1, o
        o = ctx.check_samples()
        assert o["runs"] == ctx.bsizes.r and o["row_errors"] == o["value_errors"] == 0, o
        out = ctx.bwt_get()
        exp = expected(b, out["sa"], out["ssa"], out["esa"])
        got = ctx.doc_array(b)
        for k in range(3):
            assert same(got[k], exp[k]), (U, k)
        assert np.array_equal(np.bincount(got[0].astype(np.int64)), np.array([len(s) + 10 for s in seqs[:-1]] + [len(seqs[-1]) + 11]))
        ctx.close()


@pytest.mark.gpu
def test_doc_array_merge_sharded_cli_gpu(gpu_ctx_factory, tmp_path):
    from test_sharded import synth
    seqs = synth(6, 20000, 5)
    exp = check_merge(gpu_ctx_factory, seqs, 10, 100, 8)
    check_sharded(None, seqs, 10, 100, 8, exp)
    check_cli({"pfbwt-f": os.path.join(BIN, "pfbwt-f"), "pfbwt-f64": os.path.join(BIN, "pfbwt-f64")}, os.path.join(BIN, "merge_pfp"), str(tmp_path))
