"""What the feeding entries (pfbwt-f_amd/csrc/feed_host.h) refuse and what they append: every rejected call leaves the text as it was,
and every way of feeding the same records -- one by one, as a host or device batch, as a view, in parts, after a finalize, after a
reopen, behind a left context, past the reserved range -- gives the same text (pfp_text_get) and the oracle's parse.
(w, p) = (4, 7), records of 1 to 40 bases; every case on the emulator and, marked gpu, on the card."""
import ctypes as C
import hashlib
import numpy as np
import pytest
from pfp_testlib import compare, oracle_run
from test_sharded import emu_factory  # noqa: F401  (a fixture)
import pfbwt_hip

W, P = 4, 7
PAD = b"A" * W
PARSE_NAMES = ("dict", "occ", "parse", "last", "sai", "bwlast", "ilist", "bwsai")
E = pfbwt_hip


def rnd(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def ctx(factory, U):
    return factory(w=W, p=P, u64=(U == 8), sai=True)


def emu_rows(factory):
    """rows in "device" memory: on the emulator host memory is device memory"""
    keep = []
    def dev(rows, length):
        keep.append(rows)
        return rows.ctypes.data, rows.shape[1]
    return dev


def gpu_rows(factory):
    """rows in device memory without another runtime in the process: the raw text of a second context whose pad is stride - length"""
    keep = []
    def dev(rows, length):
        owner = factory(w=rows.shape[1] - length, p=100)
        for r in rows:
            owner.feed(bytes(r[:length]), True)
        ptr, n = C.c_void_p(), C.c_uint64()
        owner._check(owner.L.pfp_text_view(owner.h, C.byref(ptr), C.byref(n)))
        assert n.value == rows.size
        keep.append(owner)
        return ptr.value, rows.shape[1]
    return dev


def row_array(rng, count, length, stride):
    rows = np.full((count, stride), ord("N"), np.uint8)
    for r in rows:
        r[:length] = np.frombuffer(rnd(rng, length), np.uint8)
    return rows


def row_text(rows, length):
    return b"".join(bytes(r[:length]) + PAD for r in rows)


def snapshot(c):
    """text_length() and text_get() of a context (a context without text answers text_get with a status)"""
    n = c.text_length()
    try:
        return n, c.text_get()
    except E.PfpError as e:
        return n, e.status


def reopen(c):
    c.L.pfp_parse_reopen.argtypes = [C.c_void_p]
    return c.L.pfp_parse_reopen(c.h)


def parse_arrays(c):
    sz = c.finalize()
    res = {"n": sz.n, "m": sz.m, "dwords": sz.dwords, "dsize": sz.dsize}
    res.update(c.parse_get()); c.parse_bwt(); res.update(c.parse_bwt_get())
    return res


def registered(c, a):
    """page-locks the array for the length of a with block (the emulator knows no page-locked memory: a no-op there)"""
    class Reg:
        def __enter__(self): assert c.L.pfp_host_register(a.ctypes.data, a.size) == 0
        def __exit__(self, *exc): assert c.L.pfp_host_unregister(a.ctypes.data) == 0
    return Reg()


# ---- rejections: the status, and the text is what it was ---------------------------------------------------------------------------
def case_rejections(factory, dev, U):
    rng = np.random.default_rng(5)
    c = ctx(factory, U)
    for n in (1, 17, 40):
        c.feed(rnd(rng, n), True)
    L, h = c.L, c.h
    rows = row_array(rng, 5, 33, 40)
    hp = rows.ctypes.data
    dp, ds = dev(rows, 33)
    buf = np.zeros(64, np.uint8)
    before = snapshot(c)
    n = before[0]
    assert n == 1 + 17 + 40 + 3 * W and len(before[1]) == n
    calls = [
        (lambda: L.pfp_parse_feed(h, None, 5, 1), E.E_ARG),
        (lambda: L.pfp_parse_feed_batch(h, hp, 2, 33, 32), E.E_ARG),
        (lambda: L.pfp_parse_feed_device_batch(h, dp, 2, 33, 32), E.E_ARG),
        (lambda: L.pfp_parse_feed_batch(h, None, 2, 33, 40), E.E_ARG),
        (lambda: L.pfp_parse_feed_device_batch(h, None, 2, 33, 40), E.E_ARG),
        (lambda: L.pfp_parse_feed_batch(h, hp, 0, 33, 40), E.PFP_OK),
        (lambda: L.pfp_parse_feed_device_batch(h, dp, 0, 33, ds), E.PFP_OK),
        (lambda: L.pfp_parse_feed_device_view(h, dp, 0, 33, ds), E.E_ARG),
        (lambda: L.pfp_parse_feed_device_view(h, dp, 2, 0, ds), E.E_ARG),
        (lambda: L.pfp_parse_feed_device_view(h, dp, 2, 33, 32), E.E_ARG),
        (lambda: L.pfp_parse_feed_device_view(h, None, 2, 33, ds), E.E_ARG),
        (lambda: L.pfp_parse_feed_device_view(h, dp, 2, 33, ds), E.E_STATE),
        (lambda: L.pfp_parse_feed_left_context(h), E.E_STATE),
        (lambda: L.pfp_text_get(h, n + 1, 0, buf.ctypes.data), E.E_ARG),
        (lambda: L.pfp_text_get(h, 0, n + 1, buf.ctypes.data), E.E_ARG),
        (lambda: L.pfp_text_get(h, n, 1, buf.ctypes.data), E.E_ARG),
        (lambda: L.pfp_debug_set(h, b"no_such_switch", 1), E.E_ARG),
        (lambda: L.pfp_debug_set(h, None, 1), E.E_ARG),
        (lambda: reopen(c), E.PFP_OK),                                       # a feeding context: nothing to reopen
    ]
    for i, (call, want) in enumerate(calls):
        assert call() == want, i
        assert snapshot(c) == before, i
    c.close()


def case_too_large(factory, dev, U):
    """a record of 2^32 (32-bit positions) resp. 2^40 bases: refused before anything is reserved or read, so a small buffer serves"""
    rng = np.random.default_rng(6)
    big = 1 << (32 if U == 4 else 40)
    rows = row_array(rng, 1, 33, 40)
    hp = rows.ctypes.data
    dp, _ = dev(rows, 33)
    for filled in (False, True):
        c = ctx(factory, U)
        if filled: c.feed(rnd(rng, 23), True)
        L, h = c.L, c.h
        before = snapshot(c)
        calls = [lambda: L.pfp_parse_feed(h, hp, big, 1), lambda: L.pfp_parse_feed_device(h, dp, big, 1),
                 lambda: L.pfp_parse_feed_batch(h, hp, 1, big, big), lambda: L.pfp_parse_feed_device_batch(h, dp, 1, big, big)]
        if not filled: calls.append(lambda: L.pfp_parse_feed_device_view(h, dp, 1, big, big))      # (a view on a context with text is E_STATE)
        for i, call in enumerate(calls):
            assert call() == E.E_TOO_LARGE, (filled, i)
            assert snapshot(c) == before, (filled, i)
        with registered(c, rows):                                            # the page-locked route of the host batch
            assert L.pfp_parse_feed_batch(h, hp, 1, big, big) == E.E_TOO_LARGE
        assert snapshot(c) == before
        c.close()


def case_reopen_states(factory, dev, U):
    """a context filled by pfp_merge_shards or pfp_bwt_load holds no text: nothing to reopen"""
    rng = np.random.default_rng(7)
    seqs = [rnd(rng, 40), rnd(rng, 37)]
    ref = oracle_run(seqs, w=W, p=P, U=U)
    assert "err" not in ref
    parts = []
    for s in seqs:
        c = ctx(factory, U); c.feed(s, True); c.finalize(shard=True); parts.append(c)
    g = ctx(factory, U)
    g.merge_shards([c.shard_view() for c in parts])
    before = snapshot(g)
    assert reopen(g) == E.E_STATE and snapshot(g) == before
    ld = ctx(factory, U)
    ld.bwt_load(ref["dict"], ref["occ"], ref["bwlast"], ref["ilist"], ref["bwsai"], n_hint=ref["n"])
    before = snapshot(ld)
    assert reopen(ld) == E.E_STATE and snapshot(ld) == before
    for c in parts + [g, ld]: c.close()


# ---- equalities --------------------------------------------------------------------------------------------------------------------
def case_batch_vs_single(factory, dev, U):
    rng = np.random.default_rng(8)
    first = rnd(rng, 9)                                                      # the batches append behind a record
    rows = row_array(rng, 5, 33, 40)
    dp, ds = dev(rows, 33)
    want = first + PAD + row_text(rows, 33)
    texts = []
    for mode in ("single", "host", "host_registered", "device"):
        c = ctx(factory, U); c.feed(first, True)
        if mode == "single":
            for r in rows: c.feed(bytes(r[:33]), True)
        elif mode == "host": c.feed_host_batch(rows.ctypes.data, 5, 33, 40)
        elif mode == "host_registered":
            with registered(c, rows): c.feed_host_batch(rows.ctypes.data, 5, 33, 40)
        else: c.feed_device_batch(dp, 5, 33, ds)
        assert c.text_length() == len(want)
        texts.append(c.text_get()); c.close()
    assert texts == [want] * 4


def case_batch_empty_records(factory, dev, U):
    for mode in ("host", "device"):
        c = ctx(factory, U)
        (c.feed_host_batch if mode == "host" else c.feed_device_batch)(0, 3, 0, 0)
        assert c.text_length() == 3 * W and c.text_get() == b"A" * (3 * W)
        c.close()


def case_partial_records(factory, dev, U):
    rng = np.random.default_rng(9)
    x, y = rnd(rng, 13), rnd(rng, 27)
    a, b = ctx(factory, U), ctx(factory, U)
    a.feed(x, False); a.feed(y, True)
    b.feed(x + y, True)
    assert a.text_get() == b.text_get() == x + y + PAD
    a.close(); b.close()


def case_view_then_feed(factory, dev, U):
    rng = np.random.default_rng(10)
    rows = row_array(rng, 2, 21, 32)
    dp, ds = dev(rows, 21)
    z = rnd(rng, 15)
    c = ctx(factory, U)
    c.feed_device_view(dp, 2, 21, ds); c.feed(z, True)
    assert c.text_get() == row_text(rows, 21) + z + PAD
    c.close()


def case_view_then_text(factory, dev, U):
    rng = np.random.default_rng(11)
    rows = row_array(rng, 2, 21, 32)
    dp, ds = dev(rows, 21)
    a, b = ctx(factory, U), ctx(factory, U)
    a.feed_device_view(dp, 2, 21, ds)
    b.feed_device_batch(dp, 2, 21, ds)
    assert a.text_length() == b.text_length() == 2 * (21 + W)
    assert a.text_get() == b.text_get() == row_text(rows, 21)
    a.close(); b.close()


def case_feed_after_finalize(factory, dev, U):
    rng = np.random.default_rng(12)
    A, B = rnd(rng, 40), rnd(rng, 31)
    c = ctx(factory, U)
    c.feed(A, True); c.finalize(); c.feed(B, True)                           # no reopen: a new text
    assert c.text_length() == len(B) + W and c.text_get() == B + PAD
    c.close()


def case_reopen(factory, dev, U):
    """feed, finalize (resp. a whole build), reopen, feed: the parse of both records"""
    rng = np.random.default_rng(13)
    A, B = rnd(rng, 40), rnd(rng, 38)
    ref = oracle_run([A, B], w=W, p=P, U=U)
    assert "err" not in ref and "err" not in oracle_run([A], w=W, p=P, U=U)
    for built in (False, True):
        c = ctx(factory, U)
        c.feed(A, True); c.finalize()
        if built: c.parse_bwt(); c.bwt_build(sa=True, rssa=True)
        assert reopen(c) == E.PFP_OK
        c.feed(B, True)
        assert c.text_get() == A + PAD + B + PAD
        assert compare(parse_arrays(c), ref, U, names=PARSE_NAMES) == [], built
        c.close()


def case_left_context(factory, dev, U):
    rng = np.random.default_rng(14)
    r = rnd(rng, 40)
    c = ctx(factory, U)
    c.feed_left_context(); c.feed(r, True)
    assert c.text_get() == PAD + r + PAD
    c.finalize(shard=True)
    assert c.shard_view().left_context == W
    c.close()


def case_outgrow_reserved(factory, dev, U):
    """the one path that copies text: pfp_parse_reserve announced 1 byte, so the range is hint + hint / 8 + 64 MiB, rounded up to its
    2 MiB pieces; a record of that many bases does not fit behind the first one.  No finalize: this is copy time only."""
    hint = 1
    reserved = hint + hint // 8 + (64 << 20)
    piece = 2 << 20
    big_len = (reserved + piece - 1) // piece * piece
    rng = np.random.default_rng(15)
    block = rnd(rng, 1000003)                                               # (a period that is no multiple of a piece, a page or a staging buffer)
    head, big = rnd(rng, 1000), (block * (big_len // len(block) + 1))[:big_len]
    c = ctx(factory, U)
    c.reserve(hint)
    c.feed(head, True); c.feed(big, True)
    assert c.text_length() == 1000 + W + big_len + W
    assert c.text_get(0, 1000 + W) == head + PAD
    assert hashlib.sha256(c.text_get(1000 + W)).digest() == hashlib.sha256(big + PAD).digest()
    c.close()


CASES = {"rejections": case_rejections, "too_large": case_too_large, "reopen_states": case_reopen_states, "batch_vs_single": case_batch_vs_single,
         "batch_empty_records": case_batch_empty_records, "partial_records": case_partial_records, "view_then_feed": case_view_then_feed,
         "view_then_text": case_view_then_text, "feed_after_finalize": case_feed_after_finalize, "reopen": case_reopen, "left_context": case_left_context}


@pytest.mark.parametrize("U", [4, 8])
@pytest.mark.parametrize("case", sorted(CASES))
def test_feed_emu(emu_factory, case, U):
    CASES[case](emu_factory, emu_rows(emu_factory), U)


@pytest.mark.gpu
@pytest.mark.parametrize("U", [4, 8])
@pytest.mark.parametrize("case", sorted(CASES))
def test_feed_gpu(gpu_ctx_factory, case, U):
    CASES[case](gpu_ctx_factory, gpu_rows(gpu_ctx_factory), U)


# (one width: the text buffer and its move do not depend on the width of the indices)
def test_outgrow_reserved_emu(emu_factory):
    case_outgrow_reserved(emu_factory, None, 8)


@pytest.mark.gpu
def test_outgrow_reserved_gpu(gpu_ctx_factory):
    case_outgrow_reserved(gpu_ctx_factory, None, 8)
