"""The table trigger scan with waves that own contiguous text (parse.h, k_trigger_scan_tab): a workgroup takes a contiguous share of
groups (4 chunks of 1 KiB each), a wave one run of consecutive groups of that share, the grid is sized by the CU count; the word in
front of a thread comes from the lane in front, from the wave's previous chunk, or -- first chunk of a run -- from memory; group counts
are plain stores.  Every case runs
twice, with the table scan and with the hash-per-window scan (no_trigger_table=1, the independent route), and both must give the
oracle's images.  The cases sit on the seams: text lengths around a thread's 16 bases, a chunk, a run and a workgroup's share; planted
triggers in the last base of a chunk, the first of the next, the first base of a run and of a share, and below w; rows of the row view
and of the device batch whose pads straddle those seams; invalid bytes on them; with and without the packed shadow.  On the CPU through
tests/emu (two CUs there; scan_waves=2 makes two waves walk a share, runs of several groups), on the card with the product library."""
import os
import subprocess
import numpy as np
import pytest
from pfp_testlib import EMU_SO, ROOT, compare, engine_run, oracle_run

NAMES = ("dict", "occ", "parse", "last", "sai", "bwt", "ssa", "esa")
CHUNK, RUN = 1024, 4096            # bases per chunk (one load instruction of a wave) and per group of 256 mask words (the shortest run of a wave)
SMALL_SHARE = 4 * RUN              # a workgroup's share while there are fewer groups than 4 x the most workgroups
M64 = (1 << 64) - 1


def with_switches(base, **sw):
    def f(**kw):
        c = base(**kw)
        c.debug_set(**sw)
        return c
    return f


def rnd(rng, n, alphabet=b"ACGT"):
    return rng.choice(np.frombuffer(alphabet, np.uint8), n).astype(np.uint8).tobytes()


def wang_hash(key):
    key = (~key + (key << 21)) & M64
    key ^= key >> 24
    key = (key + (key << 3) + (key << 8)) & M64
    key ^= key >> 14
    key = (key + (key << 2) + (key << 4)) & M64
    key ^= key >> 28
    return (key + (key << 31)) & M64


def is_trigger(kmer, p):
    v = 0
    for c in kmer:
        v = (v << 2) | b"ACGT".index(c)
    return wang_hash(v) % p == 0


def double_trigger(rng, w, p):
    """w + 1 bases whose two windows of w both trigger; None where the few k-mers of a small w have no such pair"""
    import itertools
    if w <= 5:
        for t in itertools.product(b"ACGT", repeat=w + 1):
            s = bytes(t)
            if is_trigger(s[:w], p) and is_trigger(s[1:], p):
                return s
        return None
    for _ in range(200000):
        s = rnd(rng, w + 1)
        if is_trigger(s[:w], p) and is_trigger(s[1:], p):
            return s
    raise AssertionError("no double trigger for w=%d p=%d" % (w, p))


def plant(text, s, end):
    """s so that its last base is text[end]"""
    a = bytearray(text)
    a[end + 1 - len(s):end + 1] = s
    return bytes(a)


def both_routes(factory, seqs, w, p, ntoa=False, **sw):
    """[] when the table scan and the hash-per-window scan both give the oracle's images (a text that is one phrase: the oracle's refusal)"""
    import pfbwt_hip
    ref = oracle_run(seqs, w=w, p=p, U=8, non_acgt_to_a=ntoa)
    bad = []
    for nt in (0, 1):
        try:
            res = engine_run(with_switches(factory, no_trigger_table=nt, **sw), seqs, w, p, 8, non_acgt_to_a=ntoa)
        except pfbwt_hip.PfpError as e:
            if not (ref.get("err") == "one_word" and e.status == pfbwt_hip.E_ONE_WORD):
                bad.append((nt, "status %d" % e.status))
            continue
        d = compare(res, ref, 8, NAMES) if "err" not in ref else ["accepted what the oracle refuses: %s" % ref["err"]]
        if d:
            bad.append((nt, d))
    return bad, ref


def finish(c):
    sz = c.finalize()
    res = {"n": sz.n, "m": sz.m, "dwords": sz.dwords, "dsize": sz.dsize}
    res.update(c.parse_get())
    c.parse_bwt()
    res.update(c.parse_bwt_get())
    b = c.bwt_build(sa=True, rssa=True)
    res.update(c.bwt_get())
    res["r"] = b.r
    return res


def run_lengths(factory, big, **sw):
    """lengths around every unit: a thread's 16 bases, a chunk, a run, a share of the small-input geometry, and (card) of the large one --
    as the bases of one record (the text is w longer) and as the length of the whole text, pads included"""
    rng = np.random.default_rng(31)
    w, p = 3, 7
    lens = [1, 15, 16, 17, CHUNK - 1, CHUNK, CHUNK + 1, RUN - 1, RUN, RUN + 1, SMALL_SHARE - 1, SMALL_SHARE, SMALL_SHARE + 1, 3 * SMALL_SHARE - 1, 3 * SMALL_SHARE + 1] + big
    base = rnd(rng, max(lens))
    bad = []
    for n in lens:
        cases = [[base[:n]]]
        if n > 40 + 2 * w:
            cases.append([base[:40], base[40:n - 2 * w]])
        for seqs in cases:
            d, _ = both_routes(factory, seqs, w, p, **sw)
            if d:
                bad.append((n, len(seqs), d))
    return bad


def run_dense(factory, n, share, ws=range(1, 11), **sw):
    """w = 1 .. 10, p = 3 and 7: triggers every few bases, and planted ones on every seam: in the last base of a chunk and the first of the
    next, in the first base of a run and of a workgroup's share (the oracle's phrase ends say that they did trigger), and below w"""
    rng = np.random.default_rng(77)
    bad = []
    for w in ws:
        for p in (3, 7):
            t = rnd(rng, n)
            dt = double_trigger(rng, w, p)
            seams = [CHUNK, 5 * CHUNK, RUN, 2 * RUN, 3 * RUN, share // 2, share, share + share // 2, 2 * share] if dt else []
            for s in seams:
                t = plant(t, dt, s)                    # triggers at s - 1 (last base of a chunk) and s (first base of the next chunk / run / share)
            if dt:
                t = plant(t, dt, w)                    # a trigger window that ends at w - 1 (must not count) and one that ends at w (the first that may)
            pk = (w + (p == 7)) & 1                    # with and without the packed shadow (the Xp == nullptr path), in turn
            d, ref = both_routes(factory, [t], w, p, dedup_packed=pk, **sw)
            if d:
                bad.append((w, p, pk, d))
            ends = set(int(e) - 1 for e in ref["sai"][:-1])          # sai = position of a phrase's last byte in the text with one Dollar in front
            want = [s - 1 for s in seams] + seams + ([w] if dt else [])
            miss = [e for e in want if e not in ends]
            if miss or any(e < w for e in ends):
                bad.append((w, p, "planted triggers", miss))
    return bad


def view_geometries(share):
    # (rows, length, stride, w): w bases of pad behind every row
    return [(9, 1003, 1024, 10),                    # no multiple of 16, shorter than a chunk
            (300, 7, 9, 4),                         # rows shorter than a thread's 16 bases
            (40, 1020, 1100, 10),                   # the first pad straddles a chunk seam, the later ones move through the chunks
            (7, RUN - 6, RUN + 64, 10),             # pads straddle the run seams
            (3, share - 3, share + 16, 8),          # a pad straddles a workgroup's share; rows longer than a run
            (5, 5000, 5003, 3)]


def run_views(factory, share, to_dev=None, routes=((0, 1), (0, 0), (1, 1)), **sw):
    """the row view and the device batch against feeding record by record"""
    rng = np.random.default_rng(9)
    bad = []
    for count, length, stride, w in view_geometries(share):
        p = 7 if w < 10 else 100
        base = np.frombuffer(rnd(rng, length, b"ACGTacgtN"), np.uint8)
        rows = np.full((count, stride), ord("G"), np.uint8)       # what lies between the rows must never be read as text
        for h in range(count):
            rows[h, :length] = base
            k = min(5, length)
            rows[h, rng.integers(0, length, k)] = rng.choice(np.frombuffer(b"ACGT-", np.uint8), k)
        seqs = [rows[h, :length].tobytes() for h in range(count)]
        ref = oracle_run(seqs, w=w, p=p, U=8)
        keep = None
        if to_dev is None:
            dptr, dstride = rows.ctypes.data, stride
        else:
            dptr, dstride, keep = to_dev(rows, length)
        for how in ("view", "device_batch"):
            for nt, pk in routes:                      # (no_trigger_table, dedup_packed)
                c = with_switches(factory, no_trigger_table=nt, dedup_packed=pk, **sw)(w=w, p=p, u64=True, sai=True)
                try:
                    if how == "view":
                        c.feed_device_view(dptr, count, length, dstride)
                    else:
                        c.feed_device_batch(dptr, count, length, dstride)
                    res = finish(c)
                finally:
                    c.close()
                d = compare(res, ref, 8, NAMES)
                if d:
                    bad.append((count, length, how, nt, pk, d))
        if keep is not None:
            keep.close()
    return bad


def run_symbols(factory, n, share, **sw):
    """lower case, IUPAC with and without non-ACGT -> A; an invalid byte at a chunk's first and last base and at the base in front of a
    run and of a share: PFP_E_INVALID_CHAR with the smallest bad position and its byte, on both routes"""
    import pfbwt_hip
    rng = np.random.default_rng(5)
    bad = []
    low = rnd(rng, n, b"ACGTacgtNn-")
    d, _ = both_routes(factory, [low, low[:n // 2]], 6, 13, **sw)
    if d:
        bad.append(("lower", d))
    iu = rnd(rng, n, b"ACGTRYKMSWNacgtn-")
    for w, p in ((10, 100), (4, 7)):
        d, _ = both_routes(factory, [iu, rnd(rng, n // 2), iu[:n // 3]], w, p, ntoa=True, **sw)
        if d:
            bad.append(("iupac_ntoa", w, d))
    clean = rnd(rng, n, b"ACGTacgtN")
    for positions in ([CHUNK], [CHUNK - 1], [RUN - 1], [share - 1], [share], [0], [n - 1], [2 * RUN, RUN - 1, share], [3 * CHUNK + 17, 3 * CHUNK + 16]):
        a = bytearray(clean)
        for k, q in enumerate(positions):
            a[q] = b"RxY"[k % 3]
        ref = oracle_run([bytes(a)], w=4, p=7, U=8)
        if ref.get("err") != "invalid_char":
            bad.append((positions, "oracle accepted", ref.get("err")))
            continue
        for nt in (0, 1):
            try:
                engine_run(with_switches(factory, no_trigger_table=nt, **sw), [bytes(a)], 4, 7, 8)
                bad.append((positions, nt, "accepted"))
            except pfbwt_hip.PfpError as e:
                if (e.pos, e.ch) != (ref["err_pos"], ref["err_char"]) or e.pos != min(positions):
                    bad.append((positions, nt, e.pos, e.ch, ref["err_pos"], ref["err_char"]))
    return bad


@pytest.fixture(scope="module")
def emu_factory():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pfbwt-f_amd"), "emu"], check=True, stdout=subprocess.DEVNULL)
    import pfbwt_hip
    assert pfbwt_hip.load_library(EMU_SO).pfp_backend().decode() == "cpu-emu-TEST-ONLY"
    return lambda **kw: pfbwt_hip.PfpContext(lib=EMU_SO, **kw)


# The interpreter has two CUs: at most 8 workgroups.  With all 16 waves a share of 4 groups keeps 4 waves busy with one group each; with
# scan_waves=2 two waves walk it, two groups each, and texts beyond 32 groups give longer shares.
def test_scan_lengths_emu(emu_factory):
    assert run_lengths(emu_factory, []) == []
    assert run_lengths(emu_factory, [], scan_waves=2) == []


def test_scan_dense_triggers_emu(emu_factory):
    assert run_dense(emu_factory, 2 * SMALL_SHARE + 100, SMALL_SHARE, scan_waves=2) == []


def test_scan_long_shares_emu(emu_factory):
    """48 groups on 8 workgroups: shares of 6 groups, runs of three groups with two waves, of two with five (the last two waves idle), of
    one with 16"""
    n = 48 * RUN - 5
    assert run_dense(emu_factory, n, 6 * RUN, ws=(10,), scan_waves=2) == []
    rng = np.random.default_rng(3)
    t = rnd(rng, n)
    for sw in ({}, {"scan_waves": 5}):
        d, _ = both_routes(emu_factory, [t], 4, 7, **sw)
        assert d == [], sw


def test_scan_views_emu(emu_factory):
    assert run_views(emu_factory, SMALL_SHARE, scan_waves=2) == []
    assert run_views(emu_factory, SMALL_SHARE, routes=((0, 1),)) == []


def test_scan_symbols_emu(emu_factory):
    assert run_symbols(emu_factory, 2 * SMALL_SHARE + 77, SMALL_SHARE, scan_waves=2) == []
    assert run_symbols(emu_factory, 2 * SMALL_SHARE + 77, SMALL_SHARE) == []


# ---- the same on the card.  256 CUs: up to 1024 workgroups; a text of fewer than 4096 groups (16 Mbase) has shares of 4 groups.
@pytest.mark.gpu
def test_scan_lengths_gpu(gpu_ctx_factory):
    assert run_lengths(gpu_ctx_factory, [40 * SMALL_SHARE + 1]) == []


@pytest.mark.gpu
def test_scan_dense_triggers_gpu(gpu_ctx_factory):
    assert run_dense(gpu_ctx_factory, 3 * SMALL_SHARE + 100, SMALL_SHARE) == []
    assert run_dense(gpu_ctx_factory, 2 * SMALL_SHARE + 100, SMALL_SHARE, scan_waves=2) == []


def device_rows(factory):
    """device memory without another runtime in the process: the (never finalized) text of a second context"""
    import ctypes as C

    def to_dev(rows, length):
        owner = factory(w=3, p=100)
        for h in range(rows.shape[0]):
            owner.feed(bytes(rows[h, :length]), True)
        ptr, n = C.c_void_p(), C.c_uint64()
        owner._check(owner.L.pfp_text_view(owner.h, C.byref(ptr), C.byref(n)))
        assert n.value == rows.shape[0] * (length + 3)
        return ptr.value, length + 3, owner
    return to_dev


@pytest.mark.gpu
def test_scan_views_gpu(gpu_ctx_factory):
    assert run_views(gpu_ctx_factory, SMALL_SHARE, device_rows(gpu_ctx_factory)) == []


@pytest.mark.gpu
def test_scan_symbols_gpu(gpu_ctx_factory):
    assert run_symbols(gpu_ctx_factory, 2 * SMALL_SHARE + 77, SMALL_SHARE) == []


@pytest.mark.gpu
def test_scan_large_geometry_gpu(gpu_ctx_factory):
    """the geometry of large inputs, every feed path: 9 records of 8 Mbase = 17 600 groups on 1024 workgroups -- shares of 18 groups, runs
    of two groups for nine of a workgroup's waves, none for the others, a cut share for the last workgroup.  (Contexts that earlier tests dropped without
    closing are collected first: the workspace of a context is sized by the memory that is free.)"""
    import gc
    import pfbwt_hip
    gc.collect()
    rng = np.random.default_rng(12)
    count, length, w, p = 9, 8_000_003, 10, 100
    base = np.frombuffer(rnd(rng, length), np.uint8)
    rows = np.empty((count, length), np.uint8)
    for h in range(count):
        rows[h] = base
        at = rng.integers(0, length, 3000)
        rows[h, at] = rng.choice(np.frombuffer(b"ACGTNacgt", np.uint8), at.size)
    seqs = [rows[h].tobytes() for h in range(count)]
    ref = oracle_run(seqs, w=w, p=p, U=8)
    dptr, dstride, owner = device_rows(gpu_ctx_factory)(rows, length)
    bad = []
    try:
        for how in ("feed", "view", "device_batch"):
            for nt in (0, 1):
                c = with_switches(gpu_ctx_factory, no_trigger_table=nt)(w=w, p=p, u64=True, sai=True)
                try:
                    if how == "feed":
                        for s in seqs:
                            c.feed(s, True)
                    elif how == "view":
                        c.feed_device_view(dptr, count, length, dstride)
                    else:
                        c.feed_device_batch(dptr, count, length, dstride)
                    res = finish(c)
                    d = compare(res, ref, 8, NAMES)
                except pfbwt_hip.PfpError as e:
                    d = [str(e), "workspace needed %d" % c.L.pfp_workspace_needed(c.h)]
                finally:
                    c.close()
                if d:
                    bad.append((how, nt, d))
    finally:
        owner.close()
    assert bad == []
