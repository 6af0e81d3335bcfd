"""Thresholds without a resident SA (include/pfbwt_hip.h: pfp_thresholds_windowed; include/pfbwt_hip_dev.h: pfp_debug_rows_windowed;
csrc/lcparray.h: sparse PLCP; csrc/thresholds.h: the windowed route; pfbwt-f --thr-window).

The build keeps run samples only (sa=False, rssa=True).  The SA is visited window by window (the emission run again into scratch),
the LCP rows of a window come from r sorted (text position, LCP + position) pairs and a block directory, and the gap of a run is
answered piecewise: a head piece and a tail piece inside single tiles of the windows that hold them, whole tiles from tile minima
kept for the whole output.  Expected arrays never come from the engine: text, bwt, sa and ssa are the pinned oracle's, lcp is
lcp_numpy, thresholds are thresholds_brute (test_thresholds.py); the one exception is the medium panel of the GPU, which compares
the windowed route with pfp_thresholds on the same build (vouched for by test_thresholds_medium_panel_gpu).
* rows: pfp_debug_rows_windowed == (oracle SA, lcp_numpy) for windows of 16 and 48 rows, one window, five windows, and directory
  blocks of 1, 8 and 2^40 text positions and the default -- thresholds only look at minima, a wrong non-minimal LCP would pass them;
* thresholds: == exp.thr / exp.tlcp / exp.info, check_properties, for windows of 16 and 48 rows with thr_long_min = 1 and
  thr_tile = 16 (every piece of more than one row by a wave; gaps over many windows) and the default window with the defaults;
  the cases are asserted -- from the expected arrays -- to hold gaps with lo and s in different windows, gaps over three windows
  and more, gaps that begin on a window's first row and gaps that end on a window's last row."""
import os
import numpy as np
import pytest
from pfp_testlib import EMU_SO, GOLDEN, ROOT, golden_case, oracle_run
from test_lcp_array import lcp_numpy
from test_thresholds import (BIN, DEFAULTS, EMUB, FORCED, Expected, build, check_properties, fixture_expected, previous_rows, read_u, run, same,
                             seeded_collections, sha_f)

import pfbwt_hip

ROW_FIXTURES = ["edge", "w4p7", "mult_chroms_fa"]
BLOCK_LOG2 = (0, 3, 40, -1)             # one text position per block, eight, one block for the whole text, the default (from n / r)
LONG_N = 3000
WIN = 2000                              # rows per window where the window size is not the point (16 windows on mult_chroms_fa; a multiple of 16)


def five(nout, tile=1):
    """rows per window that give five windows (a multiple of `tile`)"""
    w = -(-nout // 5)
    w = -(-w // tile) * tile
    assert -(-nout // w) == 5, (nout, tile)
    return w


# ---- rows ------------------------------------------------------------------------------------------------------------------------
def check_rows_of(ctx, sa_exp, lcp_exp, pairs, tag):
    for W, B in pairs:
        ctx.debug_set(plcp_block_log2=B)
        sa, lcp = ctx.debug_rows_windowed(W)
        assert same(sa, sa_exp), (tag, W, B, "sa", int(np.flatnonzero(np.asarray(sa, np.uint64) != sa_exp)[0]))
        assert same(lcp, lcp_exp), (tag, W, B, "lcp", int(np.flatnonzero(np.asarray(lcp, np.uint64) != lcp_exp)[0]))
    ctx.debug_set(plcp_block_log2=-1)


def check_rows(factory):
    for case in ROW_FIXTURES:
        man, seqs, exp = fixture_expected(case)
        sa_exp = np.asarray(exp.ref["sa"], np.uint64)
        nout = sa_exp.size
        windows = (16, 48, nout + 7, five(nout))
        # every window with every block size on the smallest fixture; on the others every window and every block size once
        pairs = [(W, B) for W in windows for B in BLOCK_LOG2] if case == "edge" else list(zip(windows, BLOCK_LOG2)) + [(48, -1)]
        for U in (4, 8):
            ctx = build(factory, seqs, man["w"], man["p"], U, sa=False, rssa=True)
            check_rows_of(ctx, sa_exp, exp.lcp, pairs, (case, U))
            one_sided = ctx.debug_rows_windowed(48, sa=False)          # either pointer may be NULL
            assert one_sided[0] is None and same(one_sided[1], exp.lcp)
            one_sided = ctx.debug_rows_windowed(48, lcp=False)
            assert one_sided[1] is None and same(one_sided[0], sa_exp)
            ctx.close()


_long_cache = {}


def long_chain_expected():
    """R1 N^L R2 N^L: reducible chains of L rows, and thousands of text positions in a row without a run start"""
    if not _long_cache:
        rng = np.random.default_rng(77)
        rnd = lambda n: bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))
        seqs = [rnd(400) + b"N" * LONG_N + rnd(300) + b"N" * LONG_N]
        ref = oracle_run(seqs, w=10, p=100, U=8)
        assert ref.get("err") is None, ref.get("err")
        _long_cache["v"] = (seqs, ref, lcp_numpy(ref["text"], ref["sa"]))
    return _long_cache["v"]


def check_rows_long_chain(factory):
    seqs, ref, lcp = long_chain_expected()
    assert int(lcp.max()) >= LONG_N
    sa_exp = np.asarray(ref["sa"], np.uint64)
    pos = np.sort(np.asarray(ref["ssa"], np.uint64)[1::2].astype(np.int64))          # text positions of the run starts
    assert int(np.diff(pos).max()) > 2000                                              # blocks that are empty over thousands of positions
    nout = sa_exp.size
    for U in (4, 8):
        ctx = build(factory, seqs, 10, 100, U, sa=False, rssa=True)
        check_rows_of(ctx, sa_exp, lcp, [(48, 0), (five(nout), 3), (nout, 40), (1000, -1)], ("long_chain", U))
        ctx.close()


# ---- thresholds --------------------------------------------------------------------------------------------------------------------
def gap_kinds(exp, W):
    """from the expected arrays, for windows of W rows: gaps with lo and s in different windows, gaps over three windows or more,
    gaps with lo on a window's first row, gaps with s on a window's last row"""
    starts = exp.starts.astype(np.int64)
    has, e = previous_rows(exp.ref["bwt"], starts)
    lo, s = e[has] + 1, starts[has]
    nout = int(np.asarray(exp.ref["sa"]).size)
    last = ((s + 1) % W == 0) | (s == nout - 1)
    return int((lo // W != s // W).sum()), int((s // W - lo // W >= 2).sum()), int((lo % W == 0).sum()), int(last.sum())


def check_windowed(ctx, exp, windows, tun, tag):
    ctx.debug_set(**tun)
    for W in windows:
        thr, tlcp, info, nwin = ctx.thresholds_windowed(W)
        assert same(thr, exp.thr), (tag, W, tun, "thr", int(np.flatnonzero(np.asarray(thr, np.uint64) != exp.thr)[0]))
        assert same(tlcp, exp.tlcp), (tag, W, tun, "tlcp")
        assert info == exp.info(tun["thr_long_min"]), (tag, W, tun, info, exp.info(tun["thr_long_min"]))
        check_properties(exp.ref["bwt"], exp.lcp, exp.ref["ssa"], thr, tlcp)
        nout = int(np.asarray(exp.ref["sa"]).size)
        tile = tun["thr_tile"]
        rows = min(-(-(W or (1 << 30)) // tile) * tile, -(-nout // tile) * tile)
        assert nwin == -(-nout // rows), (tag, W, nwin)


def check_small(ctx, exp, tag):
    check_windowed(ctx, exp, (16, 48), FORCED, tag)
    check_windowed(ctx, exp, (0,), DEFAULTS, tag)


_seeded_cache = {}


def seeded_expected():
    """the collections of test_thresholds.check_seeded, their oracle runs and expected arrays: once per process"""
    if not _seeded_cache:
        out = []
        for seed in (1, 2):
            for name, seqs in seeded_collections(seed).items():
                for w, p in ((10, 100), (4, 7)):
                    U = 4 if seed == 1 else 8
                    ref = oracle_run(seqs, w=w, p=p, U=U)
                    assert ref.get("err") is None, (seed, name, ref.get("err"))
                    out.append(((seed, name, w, p), seqs, w, p, U, Expected(ref, lcp_numpy(ref["text"], ref["sa"]))))
        _seeded_cache["v"] = out
    return _seeded_cache["v"]


def check_fixtures_small(factory):
    kinds = {16: np.zeros(4, np.int64), 48: np.zeros(4, np.int64)}
    for case in ("edge", "w4p7"):
        man, seqs, exp = fixture_expected(case)
        for W in kinds:
            kinds[W] += gap_kinds(exp, W)
        for U in (4, 8):
            ctx = build(factory, seqs, man["w"], man["p"], U, sa=False, rssa=True)
            check_small(ctx, exp, (case, U))
            ctx.close()
    exp = fixture_expected("edge")[2]
    assert gap_kinds(exp, 16) == (636, 13, 165, 155) and gap_kinds(exp, 48) == (219, 2, 56, 49)
    for W in kinds:
        assert (kinds[W] > 0).all(), (W, kinds[W])


def check_seeded_small(factory):
    kinds = {16: np.zeros(4, np.int64), 48: np.zeros(4, np.int64)}
    for tag, seqs, w, p, U, exp in seeded_expected():
        for W in kinds:
            kinds[W] += gap_kinds(exp, W)
        ctx = build(factory, seqs, w, p, U, sa=False, rssa=True)
        check_small(ctx, exp, tag)
        ctx.close()
    for W in kinds:
        assert (kinds[W] > 0).all(), (W, kinds[W])


FIVE = (("mult_chroms_fa", 5, (4, 8), (DEFAULTS, FORCED)), ("single_chrom", 5, (4, 8), (DEFAULTS, FORCED)), ("mult_chroms", 5, (4, 8), (DEFAULTS, FORCED)))
PANEL8 = (("panel8", 8, (8,), (DEFAULTS,)),)          # 2 M rows: 64-bit values, eight windows, the default tunables only


def check_fixtures_five(factory, cases=FIVE):
    """the larger fixtures with five windows (panel8: eight), default tunables and forced routes"""
    for case, nwin, widths, tuns in cases:
        man, seqs, exp = fixture_expected(case)
        nout = int(np.asarray(exp.ref["sa"]).size)
        for U in widths:
            ctx = build(factory, seqs, man["w"], man["p"], U, sa=False, rssa=True)
            for tun in tuns:
                W = -(-(-(-nout // nwin)) // tun["thr_tile"]) * tun["thr_tile"]
                assert -(-nout // W) == nwin, (case, W)
                assert gap_kinds(exp, W)[0] > 0, (case, W)                     # gaps with lo and s in different windows
                check_windowed(ctx, exp, (W,), tun, (case, U))
            ctx.close()


def check_published_state(factory):
    """the call changes nothing of the build: arrays, sizes, the absence (or presence) of the SA"""
    man, seqs, exp = fixture_expected("mult_chroms_fa")
    ref = exp.ref
    C = pfbwt_hip.C
    for U in (4, 8):
        dt = np.uint64 if U == 8 else np.uint32
        ctx = build(factory, seqs, man["w"], man["p"], U, sa=False, rssa=True)
        before = ctx.bwt_get()
        sizes = (ctx.bsizes.nout, ctx.bsizes.r, ctx.bsizes.easy_cases, ctx.bsizes.hard_cases, ctx.stage_ms()["bwt_build"])
        ptrs = ctx.bwt_device_ptrs()
        assert ptrs[1] is None
        ctx.debug_set(**FORCED)
        thr, tlcp, info, nwin = ctx.thresholds_windowed(48)
        assert same(thr, exp.thr) and same(tlcp, exp.tlcp) and nwin == -(-ref["sa"].size // 48) and info == exp.info(1)
        after = ctx.bwt_get()
        for k in ("bwt", "ssa", "esa"):
            assert np.array_equal(before[k], after[k]) and same(after[k], ref[k]), (U, k)
        assert after["sa"] is None and ctx.bwt_device_ptrs() == ptrs
        buf = np.empty(ref["sa"].size, dt)
        assert ctx.L.pfp_bwt_get(ctx.h, None, buf.ctypes.data_as(C.c_void_p), None, None) == pfbwt_hip.E_STATE      # still no SA
        with pytest.raises(pfbwt_hip.PfpError):
            ctx.thresholds()                                                                                      # the full route still needs one
        assert (ctx.bsizes.nout, ctx.bsizes.r, ctx.bsizes.easy_cases, ctx.bsizes.hard_cases, ctx.stage_ms()["bwt_build"]) == sizes
        ctx.bwt_build(sa=True, rssa=True)                           # with a resident SA: ignored and left alone
        full = ctx.thresholds()
        ptrs = ctx.bwt_device_ptrs()
        win = ctx.thresholds_windowed(WIN)
        assert same(win[0], full[0]) and same(win[1], full[1]) and win[2] == full[2] and same(win[0], exp.thr)
        out = ctx.bwt_get()
        assert same(out["sa"], ref["sa"]) and same(out["bwt"], ref["bwt"]) and same(out["ssa"], ref["ssa"]) and same(out["esa"], ref["esa"])
        assert ctx.bwt_device_ptrs() == ptrs
        ctx.close()


def check_coexistence(factory):
    man, seqs, exp = fixture_expected("mult_chroms_fa")
    ref = exp.ref
    starts = pfbwt_hip.doc_starts([len(s) for s in seqs], man["w"])
    C = pfbwt_hip.C
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for U in (8, 4):
        dt = np.uint64 if U == 8 else np.uint32
        for order in ("slcp_thrw", "thrw_slcp_da_thrw"):
            ctx = build(factory, seqs, man["w"], man["p"], U, sa=False, rssa=True, **FORCED)
            slcp_exp = das = None
            for step in order.split("_"):
                if step == "slcp":
                    slcp_exp = ctx.lcp_array(rows=False)[1]
                    assert same(slcp_exp[1::2], exp.lcp[np.asarray(ref["ssa"], np.uint64)[0::2].astype(np.int64)])
                elif step == "da":
                    das = ctx.doc_array(starts, rows=False)
                else:
                    first = ctx.thresholds_windowed(WIN)
                    assert same(first[0], exp.thr) and same(first[1], exp.tlcp), (U, order)
            r, ep = ctx.bsizes.r, ctx.esa_pairs
            slcp, thr, tlcp = np.empty(2 * r, dt), np.empty(2 * r, dt), np.empty(2 * r, dt)
            assert ctx.L.pfp_lcp_array_get(ctx.h, None, p(slcp)) == 0 and same(slcp, slcp_exp), (U, order)
            assert ctx.L.pfp_thresholds_get(ctx.h, p(thr), p(tlcp)) == 0 and same(thr, exp.thr) and same(tlcp, exp.tlcp), (U, order)
            if das is not None:
                sda, eda = np.empty(2 * r, dt), np.empty(2 * ep, dt)
                assert ctx.L.pfp_doc_array_get(ctx.h, None, p(sda), p(eda)) == 0 and same(sda, das[1]) and same(eda, das[2]), (U, order)
            out = ctx.bwt_get()
            assert same(out["ssa"], ref["ssa"]) and same(out["esa"], ref["esa"]) and same(out["bwt"], ref["bwt"]), (U, order)
            second = ctx.thresholds_windowed(0)                     # a second call replaces the first
            assert same(second[0], exp.thr) and second[3] == 1
            assert ctx.L.pfp_thresholds_get(ctx.h, p(thr), None) == 0 and same(thr, exp.thr)
            ctx.bwt_build(sa=False, rssa=True)                      # a new build drops the arrays
            assert ctx.thresholds_device_ptrs() == [None, None]
            assert ctx.L.pfp_thresholds_get(ctx.h, p(thr), p(tlcp)) == pfbwt_hip.E_STATE
            assert same(ctx.thresholds_windowed(WIN)[0], exp.thr)
            ctx.close()


def check_errors(factory):
    E_STATE = pfbwt_hip.E_STATE
    man, seqs, exp = fixture_expected("mult_chroms_fa")
    ref = exp.ref
    w, p = man["w"], man["p"]
    nout = ref["sa"].size
    buf = np.empty(nout, np.uint64)
    vp = lambda a: a.ctypes.data_as(pfbwt_hip.C.c_void_p)

    def both(ctx, status):
        assert ctx.L.pfp_thresholds_windowed(ctx.h, WIN, None, None) == status
        assert ctx.L.pfp_debug_rows_windowed(ctx.h, WIN, vp(buf), None) == status

    ctx = factory(w=w, p=p, u64=True, sai=True)
    both(ctx, E_STATE)                                                           # no build at all
    assert ctx.L.pfp_thresholds_windowed(None, 48, None, None) == pfbwt_hip.E_ARG
    assert ctx.L.pfp_debug_rows_windowed(None, 48, None, None) == pfbwt_hip.E_ARG
    for s in seqs:
        ctx.feed(s, True)
    ctx.finalize(); ctx.parse_bwt()
    both(ctx, E_STATE)                                                           # parsed, not built
    ctx.bwt_build(sa=True, rssa=False)                                           # no run samples
    both(ctx, E_STATE)
    ctx.bwt_build(sa=False, rssa=False)                                          # BWT only
    both(ctx, E_STATE)
    for sl in range(2):                                                          # a slice, even with samples
        ctx.bwt_build_slice(sl, 2, sa=False, rssa=True)
        both(ctx, E_STATE)
    ctx.bwt_build(sa=False, rssa=True)                                           # the context is still usable
    assert ctx.L.pfp_debug_rows_windowed(ctx.h, 0, vp(buf), None) == pfbwt_hip.E_ARG
    assert ctx.thresholds_device_ptrs() == [None, None]
    assert ctx.L.pfp_thresholds_windowed(ctx.h, 0, None, None) == 0              # info and windows are nullable
    assert same(ctx.thresholds_windowed(WIN)[0], exp.thr)
    ctx.debug_set(thr_window_rows=0, plcp_block_log2=1000)                       # values out of range are clamped, unknown keys refused
    assert same(ctx.thresholds_windowed()[1], exp.tlcp)
    ctx.debug_set(thr_window_rows=64, plcp_block_log2=-5)
    assert ctx.thresholds_windowed()[3] == -(-nout // 1024)                      # rounded up to a multiple of thr_tile
    for key in ("thr_window", "plcp_block", "thr_windows_rows"):
        with pytest.raises(pfbwt_hip.PfpError):
            ctx.debug_set(**{key: 16})
    ctx.close()
    ctx = factory(w=w, p=p, u64=True, sai=True)                                  # a loaded parse: no text in the context
    ctx.bwt_load(ref["dict"], ref["occ"], ref["bwlast"], ref["ilist"], ref["bwsai"], n_hint=ref["n"])
    ctx.bwt_build(sa=False, rssa=True)
    both(ctx, E_STATE)
    assert same(ctx.bwt_get()["ssa"], ref["ssa"])
    ctx.close()


# ---- command line ------------------------------------------------------------------------------------------------------------------
def check_cli(exe, tmp):
    for case in ("edge", "mult_chroms_fa"):
        man, seqs, exp = fixture_expected(case)
        fa = os.path.join(GOLDEN, case, "input.fa")
        wp = ["-w", str(man["w"]), "-p", str(man["p"])]
        for name, U in (("pfbwt-f64", 8), ("pfbwt-f", 4)):
            for win in ("48", "0"):
                pref = os.path.join(tmp, "%s_%d_%s" % (case, U, win))
                pr = run([exe[name], "-r", "--thr", "--thr-window", win] + wp + ["-o", pref, fa])
                assert "TASK\tthresholds\t" in pr.stderr
                assert same(read_u(pref + ".thr", U), exp.thr), (case, U, win)
                assert same(read_u(pref + ".tlcp", U), exp.tlcp), (case, U, win)
                assert not os.path.exists(pref + ".sa") and not os.path.exists(pref + ".lcp")
                mf = man["files"]["u%d" % (U * 8)]
                for e in ("bwt", "ssa", "esa", "dict", "occ", "parse", "bwlast", "ilist", "bwsai", "n"):
                    assert sha_f(pref + "." + e) == mf[e]["sha256"], (case, U, win, e)
    fa = os.path.join(GOLDEN, "edge", "input.fa")
    prefix = os.path.join(tmp, "no_thr")
    pr = run([exe["pfbwt-f64"], "-r", "--thr-window", "48", "-w", "10", "-p", "20", "-o", prefix, fa], check=False)
    assert pr.returncode != 0 and "--thr-window" in pr.stderr and "--thr" in pr.stderr, pr.stderr[-500:]
    for e in ("bwt", "thr", "tlcp", "ssa", "dict"):
        assert not os.path.exists(prefix + "." + e), e
    assert "--thr-window" in run([exe["pfbwt-f"], "-h"]).stderr


# ---- CPU: the emulated library -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    import subprocess
    subprocess.run(["make", "-C", os.path.join(ROOT, "pfbwt-f_amd"), "emu", "emu-host"], check=True, stdout=subprocess.DEVNULL)
    return lambda **kw: pfbwt_hip.PfpContext(lib=EMU_SO, **kw)


def test_windowed_rows_emu(emu):
    check_rows(emu)
    check_rows_long_chain(emu)


def test_windowed_thresholds_fixtures_emu(emu):
    check_fixtures_small(emu)
    check_fixtures_five(emu)


def test_windowed_thresholds_panel8_emu(emu):
    check_fixtures_five(emu, PANEL8)


def test_windowed_thresholds_seeded_emu(emu):
    check_seeded_small(emu)


def test_windowed_thresholds_state_coexistence_errors_emu(emu):
    check_published_state(emu)
    check_coexistence(emu)
    check_errors(emu)


def test_windowed_thresholds_cli_emu(emu, tmp_path):
    check_cli({"pfbwt-f": os.path.join(EMUB, "pfbwt-f-emu"), "pfbwt-f64": os.path.join(EMUB, "pfbwt-f64-emu")}, str(tmp_path))


# ---- GPU: the product library --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_windowed_rows_gpu(gpu_ctx_factory):
    check_rows(gpu_ctx_factory)
    check_rows_long_chain(gpu_ctx_factory)


@pytest.mark.gpu
def test_windowed_thresholds_fixtures_gpu(gpu_ctx_factory):
    check_fixtures_small(gpu_ctx_factory)
    check_fixtures_five(gpu_ctx_factory)
    check_fixtures_five(gpu_ctx_factory, PANEL8)


@pytest.mark.gpu
def test_windowed_thresholds_seeded_gpu(gpu_ctx_factory):
    check_seeded_small(gpu_ctx_factory)


@pytest.mark.gpu
def test_windowed_thresholds_state_coexistence_errors_gpu(gpu_ctx_factory):
    check_published_state(gpu_ctx_factory)
    check_coexistence(gpu_ctx_factory)
    check_errors(gpu_ctx_factory)


@pytest.mark.gpu
def test_windowed_thresholds_cli_gpu(gpu_ctx_factory, tmp_path):
    check_cli({"pfbwt-f": os.path.join(BIN, "pfbwt-f"), "pfbwt-f64": os.path.join(BIN, "pfbwt-f64")}, str(tmp_path))


@pytest.mark.gpu
def test_windowed_thresholds_medium_panel_gpu(gpu_ctx_factory):
    """64 synthetic haplotypes of 1 Mbase (the panel of test_thresholds_medium_panel_gpu), U = 8 and U = 4, -s -r: the windowed route
    with windows of 2^23 and of 2^20 + 1024 rows must give the arrays and the info of pfp_thresholds on the same build bit for bit
    (that route is checked at every run by test_thresholds_medium_panel_gpu), and pfp_debug_rows_windowed the rows of pfp_lcp_array
    and the resident SA.  No numpy brute force at this size."""
    from test_sharded import synth
    seqs = synth(31, 1 << 20, 64)
    for U in (8, 4):
        ctx = build(gpu_ctx_factory, seqs, 10, 100, U)
        full = ctx.thresholds()
        assert full[2]["long_queries"] > 0
        nout = int(ctx.bsizes.nout)
        for W in (1 << 23, (1 << 20) + 1024):
            win = ctx.thresholds_windowed(W)
            assert win[3] == -(-nout // W) and win[3] > 1, (U, W, win[3])
            assert same(win[0], full[0]) and same(win[1], full[1]) and win[2] == full[2], (U, W, win[2], full[2])
        sa_w, lcp_w = ctx.debug_rows_windowed((1 << 20) + 1024)
        assert same(lcp_w, ctx.lcp_array(runs=False)[0]), U
        assert same(sa_w, ctx.bwt_get()["sa"]), U
        ctx.close()
