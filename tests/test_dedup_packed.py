"""De-duplication against the 2-bit packed shadow of the text (parse.h, DedupText): the trigger scan writes the codes of every 16
bases and a clean bit per 16 bases, k_dedup_insert hashes and compares phrases covered by clean words in 2-bit form.  Every case runs
with dedup_packed=1 and =0 and must give the oracle's images either way: strings with equal codes but different bytes (N/A, '-'/T) in
both orders, lower case, IUPAC with non-ACGT->A, phrases at every offset against the 16-base words, the Dollars of the first and the
last phrase, long phrases, windows that do not fit, an abandoned first table, the hash-per-window scan (no shadow), the feed paths,
a two-shard merge and both dedup variants.  On the CPU through tests/emu, on the card with the product library."""
import os
import subprocess
import numpy as np
import pytest
from pfp_testlib import EMU_SO, ROOT, compare, engine_run, oracle_run

NAMES = ("dict", "occ", "parse", "last", "sai", "bwt", "ssa", "esa")


def with_switches(base, **sw):
    def f(**kw):
        c = base(**kw)
        c.debug_set(**sw)
        return c
    return f


def rnd(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(list(alphabet), n).astype(np.uint8))


def mutate(rng, s, k, alphabet=b"ACGT"):
    a = bytearray(s)
    for i in rng.integers(0, len(a), k):
        a[i] = alphabet[rng.integers(0, len(alphabet))]
    return bytes(a)


def swap_codes(s, frm, to, every):
    """every `every`-th occurrence of byte frm replaced by `to` (same 2-bit code, different byte)"""
    a = bytearray(s)
    idx = [i for i, c in enumerate(a) if c == frm][::every]
    for i in idx:
        a[i] = to
    return bytes(a)


def cases(scale):
    rng = np.random.default_rng(2024)
    L = 1500 * scale
    base = rnd(rng, L)
    out = []
    # N against A and '-' against T: equal codes, different bytes; the clean copy first, and the unclean copy first
    # (short phrases: many workgroups, most of them clean; the swaps in a stretch of their own, and everywhere)
    na = swap_codes(swap_codes(base, ord("A"), ord("N"), 7), ord("T"), ord("-"), 11)
    na_part = base[:L // 3] + na[L // 3:L // 3 + 200] + base[L // 3 + 200:]
    out.append(("n_vs_a", [base, na_part, base, na_part, base, na_part, base, na_part, base], 4, 7, False))
    out.append(("a_vs_n", [na_part, base, na_part, base, na_part, base, na_part, base, na_part], 4, 7, False))
    out.append(("n_vs_a_long", [base, na, base, na, base, na, base, na, base], 10, 100, False))
    out.append(("n_vs_a_short", [base[:600], na[:600]] * 5, 4, 7, False))
    # lower case (clean after normalisation), IUPAC with non-ACGT -> A, lower case + N without it
    low = bytes(c + 32 if i % 3 == 0 else c for i, c in enumerate(base))
    out.append(("lower", [base, low, mutate(rng, low, 5), base, low, low, base, low], 4, 7, False))
    iu = rnd(rng, L, b"ACGTRYKMSWNacgtn-")
    for w, p in ((10, 100), (4, 7)):
        out.append(("iupac_ntoa", [iu, mutate(rng, iu, 4, b"ACGTRYN"), iu, base, iu, mutate(rng, base, 3, b"ACGTRY"), iu, iu], w, p, True))
    out.append(("lower_n", [rnd(rng, L, b"ACGTacgtNn")] * 4 + [base] * 4, 6, 13, False))
    # every offset against the 16-base words, n no multiple of 16, the Dollars of phrase 0 and of the last phrase
    out.append(("offsets", [rnd(rng, k) + base[:800 * scale] for k in range(16)] + [base[:5]], 4, 7, False))
    out.append(("tail", [base[:777], base[:777], base[:777] + b"ACG"], 4, 7, False))
    # long phrases: runs of N longer than LONG_PHRASE, the same run twice
    out.append(("long", [base[:900] + b"N" * 3000 + base[900:1500], base[:900] + b"N" * 3000 + base[900:1500], mutate(rng, base, 9)] * 3, 10, 100, False))
    return out


def run_all(factory, scale, variants=(0, 1)):
    bad = []
    for name, seqs, w, p, ntoa in cases(scale):
        ref = oracle_run(seqs, w=w, p=p, U=8, non_acgt_to_a=ntoa)
        for pk in (1, 0):
            for v in variants:
                res = engine_run(with_switches(factory, dedup_packed=pk, dedup_variant=v), seqs, w, p, 8, non_acgt_to_a=ntoa)
                d = compare(res, ref, 8, NAMES)
                if d:
                    bad.append((name, pk, v, d))
    return bad


def run_fallbacks(factory, scale):
    """a workgroup window that exceeds the LDS tile (phrases just below LONG_PHRASE), a first table that is abandoned, the
    hash-per-window scan (no packed shadow)"""
    rng = np.random.default_rng(7)
    bad = []
    base = rnd(rng, 1200 * scale)
    # phrases of ~2000 bases (runs of 'N' just below LONG_PHRASE, N never triggers at p = 100) side by side: windows beyond the tile
    big = [base[:300] + b"N" * 1900 + base[300:600] + b"N" * 1890 + base[600:], ] * 6
    runs = [("big_window", big, 10, 100, {}),
            ("abandon", [mutate(rng, base, 40) for _ in range(8)], 6, 13, {"dedup_table_log2": 10}),
            ("w12_no_table", [base, mutate(rng, base, 6)] * 4, 12, 50, {"no_trigger_table": 1}),
            ("no_table", [base, mutate(rng, base, 6)] * 4, 10, 100, {"no_trigger_table": 1})]
    for name, seqs, w, p, sw in runs:
        ref = oracle_run(seqs, w=w, p=p, U=8)
        for pk in (1, 0):
            for v in (0, 1):
                res = engine_run(with_switches(factory, dedup_packed=pk, dedup_variant=v, **sw), seqs, w, p, 8)
                d = compare(res, ref, 8, NAMES)
                if d:
                    bad.append((name, pk, v, d))
    return bad


def run_feeds(factory, to_dev=None):
    """device view, host batch, device batch, FASTA: the same parse as feeding record by record, with and without the shadow"""
    rng = np.random.default_rng(9)
    count, length, stride, w, p = 9, 1003, 1024, 10, 100
    base = np.frombuffer(rnd(rng, length, b"ACGTacgt"), np.uint8)
    rows = np.zeros((count, stride), np.uint8)
    for h in range(count):
        rows[h, :length] = base
        rows[h, rng.integers(0, length, 5)] = rng.choice(list(b"ACGTN"), 5)
    seqs = [rows[h, :length].tobytes() for h in range(count)]
    ref = oracle_run(seqs, w=w, p=p, U=8)
    bad = []
    keep = []
    if to_dev is None:
        dptr, dstride = rows.ctypes.data, stride
    else:
        dptr, dstride, owner = to_dev(rows, length); keep.append(owner)
    fasta = b"".join(b">r%d\n" % h + s[:500] + b"\n" + s[500:] + b"\n" for h, s in enumerate(seqs))
    for pk in (1, 0):
        for how in ("view", "host_batch", "device_batch", "fasta"):
            c = with_switches(factory, dedup_packed=pk)(w=w, p=p, u64=True, sai=True)
            try:
                if how == "view":
                    c.feed_device_view(dptr, count, length, dstride)
                elif how == "host_batch":
                    c.feed_host_batch(rows.ctypes.data, count, length, stride)
                elif how == "device_batch":
                    c.feed_device_batch(dptr, count, length, dstride)
                else:
                    c.feed_fasta(fasta)
                sz = c.finalize()
                res = {"n": sz.n, "m": sz.m, "dwords": sz.dwords, "dsize": sz.dsize}
                res.update(c.parse_get())
            finally:
                c.close()
            d = compare(res, ref, 8, ("dict", "occ", "parse", "last"))
            if d:
                bad.append((how, pk, d))
    for o in keep:
        o.close()
    return bad


def run_merge(factory):
    from test_sharded import sharded_single_process
    rng = np.random.default_rng(5)
    base = rnd(rng, 2500)
    seqs = [mutate(rng, base, 8) for _ in range(4)]
    ref = oracle_run(seqs, w=10, p=100, U=4)
    bad = []
    for pk in (1, 0):
        res = sharded_single_process(with_switches(factory, dedup_packed=pk), seqs, [[0, 1], [2, 3]], 10, 100, 4)
        d = compare(res, ref, 4)
        if d:
            bad.append((pk, d))
    return bad


@pytest.fixture(scope="module")
def emu_factory():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pfbwt-f_amd"), "emu"], check=True, stdout=subprocess.DEVNULL)
    import pfbwt_hip
    assert pfbwt_hip.load_library(EMU_SO).pfp_backend().decode() == "cpu-emu-TEST-ONLY"
    return lambda **kw: pfbwt_hip.PfpContext(lib=EMU_SO, **kw)


def test_dedup_packed_cases_emu(emu_factory):
    assert run_all(emu_factory, 1) == []


def test_dedup_packed_fallbacks_emu(emu_factory):
    assert run_fallbacks(emu_factory, 1) == []


def test_dedup_packed_feeds_emu(emu_factory):
    assert run_feeds(emu_factory) == []


def test_dedup_packed_merge_emu(emu_factory):
    assert run_merge(emu_factory) == []


def gpu_factory():
    import pfbwt_hip
    assert pfbwt_hip.load_library().pfp_backend().decode() == "hip-gfx950"
    return lambda **kw: pfbwt_hip.PfpContext(device=0, **kw)


@pytest.mark.gpu
def test_dedup_packed_cases_gpu():
    assert run_all(gpu_factory(), 8) == []


@pytest.mark.gpu
def test_dedup_packed_fallbacks_gpu():
    assert run_fallbacks(gpu_factory(), 8) == []


@pytest.mark.gpu
def test_dedup_packed_feeds_gpu():
    import ctypes as C
    F = gpu_factory()

    def to_dev(rows, length):      # device memory without another runtime in the process: the (never finalized) text of a second context
        owner = F(w=3, p=100)
        for h in range(rows.shape[0]):
            owner.feed(bytes(rows[h, :length]), True)
        ptr, n = C.c_void_p(), C.c_uint64()
        owner._check(owner.L.pfp_text_view(owner.h, C.byref(ptr), C.byref(n)))
        assert n.value == rows.shape[0] * (length + 3)
        return ptr.value, length + 3, owner
    assert run_feeds(F, to_dev) == []


@pytest.mark.gpu
def test_dedup_packed_merge_gpu():
    assert run_merge(gpu_factory()) == []
