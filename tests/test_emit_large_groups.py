"""k_emit_groups_large (emit.h): the groups of special rows that are too long for a batch of k_emit_groups are sorted in LDS, one
group per workgroup turn, by 512 threads (groups of at most 8192 rows) or 1024 threads (at most 16384 rows).  .bwt, .ssa, .esa and r
must equal the oracle at both widths of the text positions, with 32- and 64-bit row counters (force_wide_rows), in one build and in
three slices; pfp_debug_emit_large_groups tells which of the two instantiations a build reached.

Panels reach the kernels at their real geometry: H copies of one random base sequence (w = 6, p = 13) in which three sites carry
another base in a fixed half of the copies -- site 9 and site 22 in the copies of the first half, site 25 in the even copies.  The
base has 40 bases, the shortest for which the sites fall as follows (the emulator's time goes with H x bases; with 120 bases and
other sites the same counts come out).  The suffix behind a site is shared by the dictionary words that differ at the site: a
group of special rows with one member per variant.  Sites 22 and 25 lie in one word, site 9 in another, so a panel holds
  - three groups of H rows: behind site 9 (2 members), behind site 25 (4 members: the variants of sites 22 x 25), and the suffixes
    at the start of a copy (2 members: the first copy follows the start of the text, every other copy a copy),
  - two groups of ceil(H / 2) and floor(H / 2) rows: the suffixes behind site 22 hold site 25, one group per variant of it.
A group of at most 4096 rows fits a batch of k_emit_groups, one of at most 8192 rows goes on the first list, one of at most 16384
rows on the second, a longer one is left to the sort route.  Hence the groups taken per list, (first, second):
  H =  8192: (3, 0)  full buffer of the 8 K kernel; the halves (4096 rows) stay in the batches
  H =  8193: (1, 3)  the smallest group of the 16 K kernel; the half of 4097 rows is the smallest of the 8 K kernel
  H = 16384: (2, 3)  full buffer of the 16 K kernel, and both halves fill the buffer of the 8 K kernel
  H = 16385: (1, 1)  the three groups of H rows are NOT taken; the halves have 8193 and 8192 rows
A build that emits its windows twice (a pass for the bytes, a pass for the samples) counts every group twice.

On the emulator the emission starts from the oracle's parse (pfp_bwt_load): fibers need seconds to parse a panel and a fraction of a
second to emit it, and the parse is not what this file is about; on the card the whole pipeline runs.  The small end -- one item per
thread, fewer than 64 rows, row counts that are no multiple of the wave or the workgroup, groups of several hundred members -- comes
from the wide_groups and haplotypes cases of test_group_reduce.py with batches of 8 / 12 / 40 rows, through the whole pipeline on
both.  The emulator tests run once more in a process with PFP_EMU_POISON=1 (fresh workspace memory holds 0xA5, not zeros)."""
import functools
import os
import subprocess
import sys
import numpy as np
import pytest
from pfp_testlib import EMU_SO, ROOT, compare, oracle_run
from test_group_reduce import cases

NAMES = ("bwt", "ssa", "esa")
W, P, BASES, SEED = 6, 13, 40, 13
SITES = ((9, "half"), (22, "half"), (25, "even"))
EXPECT = {8192: (3, 0), 8193: (1, 3), 16384: (2, 3), 16385: (1, 1)}


@functools.lru_cache(maxsize=None)
def panel(H):
    rng = np.random.default_rng(SEED)
    base = rng.choice(list(b"ACGT"), BASES).astype(np.uint8)
    rows = np.tile(base, (H, 1))
    h = np.arange(H)
    for pos, which in SITES:
        rows[(h < H // 2) if which == "half" else (h % 2 == 0), pos] = b"ACGT"[(b"ACGT".index(bytes([base[pos]])) + 1) % 4]
    return tuple(bytes(r) for r in rows)


@functools.lru_cache(maxsize=None)
def panel_ref(H, U):
    return oracle_run(list(panel(H)), w=W, p=P, U=U)


@functools.lru_cache(maxsize=None)
def small_case(name, copies, U):
    seqs, w, p = next((s, w, p) for n, s, w, p, _ in cases(copies) if n == name)
    return seqs, w, p, oracle_run(seqs, w=w, p=p, U=U)


def parsed(factory, seqs, w, p, U, ref, load):
    c = factory(w=w, p=p, u64=(U == 8), sai=True)
    try:
        if load:
            c.bwt_load(ref["dict"], ref["occ"], ref["bwlast"], ref["ilist"], ref["bwsai"])
        else:
            for s in seqs:
                c.feed(s, True)
            c.finalize(); c.parse_bwt()
    except Exception:
        c.close()
        raise
    return c


def taken(c):
    g = c.emit_large_groups()
    assert (g["rows_8k"], g["rows_16k"]) == (8192, 16384), g
    return g["groups_8k"], g["groups_16k"]


def builds_equal_oracle(c, ref, U, tag, nslices=3):
    """the BWT alone (every window is emitted once), BWT + run samples, and the slices of a sliced emission, from one parse;
    returns the groups taken by the first two"""
    c.bwt_build(sa=False, rssa=False)
    assert compare(c.bwt_get(), ref, U, ("bwt",)) == [], tag
    once = taken(c)
    b = c.bwt_build(sa=False, rssa=True)
    res = c.bwt_get(); res["r"] = b.r
    assert compare(res, ref, U, NAMES) == [], tag
    sampled = taken(c)
    parts = {k: [] for k in NAMES}; r = 0
    for sl in range(nslices):
        b, _, _ = c.bwt_build_slice(sl, nslices, sa=False, rssa=True)
        o = c.bwt_get()
        for k in NAMES:
            parts[k].append(o[k])
        r += b.r
    res = {k: np.concatenate(v) for k, v in parts.items()}; res["r"] = r
    assert compare(res, ref, U, NAMES) == [], tag + ("sliced",)
    return once, sampled


def check_panel(factory, H, load):
    for U in (4, 8):
        ref = panel_ref(H, U)
        c = parsed(factory, panel(H), W, P, U, ref, load)
        try:
            for fw in (0, 1):
                c.debug_set(force_wide_rows=fw)
                once, sampled = builds_equal_oracle(c, ref, U, (H, U, fw))
                want = EXPECT[H]
                assert once == want, (H, U, fw, once)
                assert sampled in (want, (2 * want[0], 2 * want[1])), (H, U, fw, sampled)
        finally:
            c.close()


def check_small(factory, name, copies, U):
    """batches of 8 / 12 / 40 rows: a longer group of at most four members and at most four batches of rows goes to the 8 K kernel,
    the others (wide_groups: up to `copies` members) take the sort route.  With 8 rows both cases have such groups: behind a changed
    base of haplotypes lie the 12 rows of the 12 copies, and the suffixes that start two or three bases in front of the shared
    stretch of wide_groups occur in copies / 16 or copies / 64 of the copies."""
    seqs, w, p, ref = small_case(name, copies, U)
    c = parsed(factory, seqs, w, p, U, ref, False)
    try:
        for rows in (8, 12, 40):
            for fw in (0, 1):
                c.debug_set(emit_group_rows=rows, big_group_members=4, force_wide_rows=fw)
                once, sampled = builds_equal_oracle(c, ref, U, (name, U, rows, fw))
                assert once[1] == 0 and sampled[1] == 0 and sampled[0] in (once[0], 2 * once[0]), (name, U, rows, fw, once, sampled)
                if rows == 8:
                    assert once[0] > 0, (name, U, rows, fw, once)
    finally:
        c.close()


@pytest.fixture(scope="module")
def emu_factory():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pfbwt-f_amd"), "emu"], check=True, stdout=subprocess.DEVNULL)
    import pfbwt_hip
    assert pfbwt_hip.load_library(EMU_SO).pfp_backend().decode() == "cpu-emu-TEST-ONLY"
    return lambda **kw: pfbwt_hip.PfpContext(lib=EMU_SO, **kw)


@pytest.mark.parametrize("H", sorted(EXPECT))
def test_large_groups_panel_emu(emu_factory, H):
    check_panel(emu_factory, H, load=True)


SMALL = [(n, U) for n in ("wide_groups", "haplotypes") for U in (4, 8)]


@pytest.mark.parametrize("name,U", SMALL)
def test_large_groups_small_end_emu(emu_factory, name, U):
    check_small(emu_factory, name, 160, U)


def test_large_groups_poisoned_workspace_emu(emu_factory):
    if os.environ.get("PFP_EMU_POISON"):
        return      # this IS the poisoned run
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "emu and not poisoned"],
                       env=dict(os.environ, PFP_EMU_POISON="1"), cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]


def gpu_factory():
    import pfbwt_hip
    assert pfbwt_hip.load_library().pfp_backend().decode() == "hip-gfx950"
    return lambda **kw: pfbwt_hip.PfpContext(device=0, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("H", sorted(EXPECT))
def test_large_groups_panel_gpu(H):
    check_panel(gpu_factory(), H, load=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name,U", SMALL)
def test_large_groups_small_end_gpu(name, U):
    check_small(gpu_factory(), name, 500, U)
