"""The device-wide primitives of pfbwt-f_amd/csrc/prims.h on their own -- device_scan, radix_sort_pairs, device_compact --
through the hooks of include/pfbwt_hip_dev.h (pfp_debug_sort_pairs, pfp_debug_scan, pfp_debug_compact), against plain numpy, at
the sizes where their kernels change route.  Every edge size is computed from pfp_debug_prims_geometry, so a retune of the tile
sizes moves the edges with it.

Sort: the values are the original indices and the reference is a stable argsort of the keys masked to the digits the passes
cover, so ONE comparison of the returned values checks the order, the stability and that no pair is lost, doubled or parted
from its key.  Every hook call asserts that the guard words around its device buffers are intact.

Every group of cases runs in a child process of its own (this file, run as a script), once on the emulated library (tests/emu,
PFP_EMU_POISON=1: fresh device memory holds garbage) and once, marked gpu, on the product library."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest
from pfp_testlib import EMU_SO, ROOT, compare, engine_run, oracle_run

U32, U64, VP = C.c_uint32, C.c_uint64, C.c_void_p
WORKSPACE = 256 << 20     # the largest case (S * S + S + 3 u32 elements in, out and partials) needs 34 MiB; committed as touched
FILL = 0xEEEEEEEE          # what a hook leaves in output elements that the primitive did not write


def ptr(a):
    return None if a is None else a.ctypes.data_as(VP)


class Prims:
    """one context of the library under test and the prototypes of the hooks"""

    def __init__(self, kind):
        import pfbwt_hip
        self.lib = EMU_SO if kind == "emu" else None
        # A workspace of a fixed size: left to itself the context sizes it by n and reserves a larger one whenever n grows,
        # dozens of times in a group -- and on the MI355X the first stores into a range that was unmapped and mapped again
        # were seen to be lost (the section on device memory): guard bytes written right after it read back as zero.
        self.ctx = pfbwt_hip.PfpContext(lib=self.lib, workspace_bytes=WORKSPACE)
        assert self.ctx.backend() == ("cpu-emu-TEST-ONLY" if kind == "emu" else "hip-gfx950")
        L = self.L = self.ctx.L
        L.pfp_debug_prims_geometry.argtypes = [C.POINTER(U32)]
        L.pfp_debug_sort_pairs.argtypes = [VP, VP, C.c_int, VP, U64, C.POINTER(C.c_int), C.c_int, VP, VP, C.POINTER(U32)]
        L.pfp_debug_scan.argtypes = [VP, VP, C.c_int, C.c_int, C.c_int, U64, VP, VP, C.POINTER(U32)]
        L.pfp_debug_compact.argtypes = [VP, VP, VP, U64, VP, C.POINTER(U32), C.POINTER(U32)]
        g = (U32 * 4)()
        assert L.pfp_debug_prims_geometry(g) == 0
        self.T, self.S, self.SMALL_MAX, self.GRID = (int(x) for x in g)
        assert self.T % 256 == 0 and self.S % 256 == 0 and self.SMALL_MAX >= 2 and self.GRID > 256, list(g)

    def route(self, seg_grid=None, seg_stage=1):
        self.ctx.debug_set(seg_grid=self.GRID if seg_grid is None else seg_grid, seg_stage=seg_stage)

    def sort_status(self, keys, ranges):
        """(status, sorted keys, values) of radix_sort_pairs on (keys, their indices); the guards are asserted"""
        n = len(keys)
        vals = np.arange(n, dtype=np.uint32)
        ko = np.full(n, 0x11, keys.dtype); vo = np.full(n, 0x11, np.uint32)
        flat = (C.c_int * (2 * len(ranges)))(*[x for r in ranges for x in r])
        bad = U32(7)
        rc = self.L.pfp_debug_sort_pairs(self.ctx.h, ptr(keys), keys.itemsize, ptr(vals), n, flat, len(ranges), ptr(ko), ptr(vo), C.byref(bad))
        assert rc != 0 or bad.value == 0, ("guard words changed", bad.value, n, ranges)
        return rc, ko, vo

    def scan(self, a, op, mode, want_total=True):
        """(output, total | None) of pfp_debug_scan; mode 0 out of place, 1 in place, 2 k_scan_spine alone"""
        out = np.full(len(a), 0x11, a.dtype); tot = np.full(1, 0x11, a.dtype); bad = U32(7)
        rc = self.L.pfp_debug_scan(self.ctx.h, ptr(a), a.itemsize, op, mode, len(a), ptr(out), ptr(tot) if want_total else None, C.byref(bad))
        assert rc == 0 and bad.value == 0, (rc, bad.value, len(a), a.dtype, op, mode)
        return out, (tot[0] if want_total else None)

    def compact(self, src, flag):
        n = len(flag)
        out = np.full(n, 0x11, np.uint32); cnt = U32(0x11111111); bad = U32(7)
        rc = self.L.pfp_debug_compact(self.ctx.h, ptr(src), ptr(flag), n, ptr(out), C.byref(cnt), C.byref(bad))
        assert rc == 0 and bad.value == 0, (rc, bad.value, n)
        return out, cnt.value


# ---- sort ------------------------------------------------------------------------------------------------------------------
K32_8, K32_21, K32_32 = (np.uint32, ((0, 8),)), (np.uint32, ((0, 21),)), (np.uint32, ((0, 32),))
K64_64, K64_SPLIT, K64_8 = (np.uint64, ((0, 64),)), (np.uint64, ((0, 12), (32, 44))), (np.uint64, ((0, 8),))
DISTS = ("uniform", "outside", "equal", "two", "sorted", "reverse", "ninety")


def digit_mask(ranges, bits):
    """the key bits the passes look at: a FULL 8-bit digit at lo, lo + 8, ... below hi, for every range; the shifts must ascend"""
    m, last = 0, -8
    for lo, hi in ranges:
        for s in range(lo, hi, 8):
            assert s >= last + 8, ranges      # (the reference below orders by the masked key as one integer)
            m |= 0xFF << s; last = s
    return m & ((1 << bits) - 1)


def spread(rng, n, mask, dt):
    """n random keys with all their bits inside mask"""
    return rng.integers(0, 1 << 63, n, dtype=np.uint64).astype(dt) & dt(mask)


def make_keys(rng, n, dt, ranges, dist):
    bits = 8 * np.dtype(dt).itemsize
    mask = digit_mask(ranges, bits); full = (1 << bits) - 1
    if dist == "uniform":
        k = spread(rng, n, mask, dt)
    elif dist == "outside":      # few values in the covered digits (many ties), random bits everywhere else: they must not move a pair
        k = spread(rng, 5, mask, dt)[rng.integers(0, 5, n)] | spread(rng, n, full & ~mask, dt)
    elif dist == "equal":
        k = np.full(n, spread(rng, 1, full, dt)[0], dt)
    elif dist == "two":          # every covered digit is 0x00 or 0xFF
        k = np.where(rng.random(n) < 0.5, dt(mask), dt(0)).astype(dt) | spread(rng, n, full & ~mask, dt)
    elif dist in ("sorted", "reverse"):
        k = np.sort(spread(rng, n, mask, dt))
        if dist == "reverse": k = k[::-1].copy()
    else:                        # ninety: 90 % one key
        k = spread(rng, n, mask, dt); k[rng.random(n) < 0.9] = spread(rng, 1, mask, dt)[0]
    return np.ascontiguousarray(k, dt)


def check_sort(P, keys, ranges, tag):
    rc, ko, vo = P.sort_status(keys, ranges)
    assert rc == 0, (tag, rc)
    perm = np.argsort(keys & keys.dtype.type(digit_mask(ranges, 8 * keys.itemsize)), kind="stable").astype(np.uint32)
    if not np.array_equal(vo, perm):
        i = int(np.flatnonzero(vo != perm)[0])
        raise AssertionError("%s: values differ from the stable permutation at %d of %d: got %d want %d (%d differ)" % (tag, i, len(keys), vo[i], perm[i], int((vo != perm).sum())))
    assert np.array_equal(ko, keys[perm]), (tag, "keys")


LAYOUTS = (K32_8, K64_64, K32_21, K64_SPLIT, K32_32)      # the widths alternate: any two neighbours hold both


def run_sorts(P, cases, seed):
    """cases: (size, its routes).  A cross-section of size x route x key layout x distribution: every size runs under every one
    of its routes, layouts (5) and distributions (7) rotate against the routes (4 or 8 per size, the scatter kernels alternating),
    so every size meets both scatter kernels and both key widths, and every route every layout"""
    rng = np.random.default_rng(seed)
    i = 0
    for n, routes in cases:
        seen = set()
        for grid, stage in routes:
            P.route(grid, stage)
            dt, ranges = LAYOUTS[i % len(LAYOUTS)]; dist = DISTS[i % len(DISTS)]; i += 1
            seen |= {("stage", stage), np.dtype(dt).itemsize}
            check_sort(P, make_keys(rng, n, dt, ranges, dist), ranges, "n=%d grid=%s stage=%d %s %s %s" % (n, grid, stage, np.dtype(dt).name, ranges, dist))
        assert seen == {("stage", 0), ("stage", 1), 4, 8}, (n, seen)


def group_sort_small(P):
    """one tile or less: k_small_sort (the route switches do not apply).  Every size with every layout, three of the seven
    distributions each, rotating: over the sizes every layout meets every distribution"""
    T = P.T
    rng = np.random.default_rng(1)
    i = 0
    for n in (2, 63, 64, 65, T - 1, T):
        for dt, ranges in LAYOUTS:
            for j in range(3):
                dist = DISTS[i % len(DISTS)]; i += 1
                check_sort(P, make_keys(rng, n, dt, ranges, dist), ranges, "n=%d %s %s %s" % (n, np.dtype(dt).name, ranges, dist))


def group_sort_tiles(P):
    """a second tile of one pair, last waves of 31 / 32 / 33 and 63 / 64 / 65 pairs (the leader of a digit comes from the high
    half of the vote when the low half is empty), whole tiles: as ONE segment of several tiles (seg_grid 1) and as one tile per
    segment, staged and unstaged"""
    T = P.T
    sizes = [T + 1] + [T + d for d in (31, 32, 33, 63, 64, 65)] + [2 * T, 2 * T + 1]
    run_sorts(P, [(n, [(1, 1), (1, 0), (None, 1), (None, 0)]) for n in sizes], 2)


def group_sort_five_tiles(P):
    """Five tiles, the last one short by a pair (5T - 1) or holding one pair (4T + 1), and six with one pair in the last (5T + 1).
    seg_grid 1: one segment walks all tiles; 2: three tiles per segment, on five tiles 3 + 2 -- the walk of the last segment ends at
    tbase >= n; 3: two per segment, on five tiles 2 + 2 + 1; the default: one tile per segment.  In a segment of several tiles the
    pairs of tile t + 1 are fetched while tile t is ranked and the per-digit cursors are carried from tile to tile."""
    T = P.T
    run_sorts(P, [(5 * T - 1, [(g, s) for g in (1, 2, 3, None) for s in (1, 0)]), (5 * T + 1, [(g, s) for g in (1, 2, 3, None) for s in (0, 1)]),
                  (4 * T + 1, [(2, 1), (3, 0), (2, 0), (3, 1)])], 3)


def sort_segments(P, G, cases):
    """G segments of one tile under the default seg_grid, one 8-bit pass"""
    assert G <= P.GRID
    n = (G - 1) * P.T + 1 if G > P.SMALL_MAX else G * P.T
    rng = np.random.default_rng(G)
    for (dt, ranges), stage, dist in cases:
        P.route(None, stage)
        check_sort(P, make_keys(rng, n, dt, ranges, dist), ranges, "G=%d n=%d stage=%d %s %s" % (G, n, stage, np.dtype(dt).name, dist))


def group_sort_g_small_max(P):
    """SEG_SMALL_MAX whole tiles: the most segments k_seg_small takes"""
    sort_segments(P, P.SMALL_MAX, [(K32_8, 1, "uniform"), (K64_8, 0, "outside"), (K32_8, 0, "ninety"), (K64_8, 1, "uniform")])


def group_sort_g_small_max_plus_one(P):
    """one pair more: the first size of the k_seg_colscan / k_seg_dbase pair"""
    sort_segments(P, P.SMALL_MAX + 1, [(K32_8, 0, "uniform"), (K64_8, 1, "outside"), (K32_8, 1, "two"), (K64_8, 0, "uniform")])


def group_sort_g257(P):
    """256 tiles and a pair: k_seg_colscan walks its column in two trips with a carry"""
    sort_segments(P, 257, [(K32_8, 1, "outside"), (K64_8, 0, "uniform")])


def group_sort_ranges_contract(P):
    """What `ranges` means (the comment above radix_sort_pairs): whole 8-bit digits from lo.  The bits between hi and the end of
    the last digit of a range take part in the order, the bits above do not; and more passes than the one-workgroup sort holds
    (SMALL_MAX_PASSES = 8) are sorted by the segmented route at any n."""
    T = P.T
    rng = np.random.default_rng(5)
    for n in (T, T + 1):
        for stage in (1, 0):
            P.route(None, stage)
            # {0, 21}: bits 21 .. 23 are in the third digit, bits 24 .. 31 in none
            low = rng.integers(0, 4, n).astype(np.uint32); spill = rng.integers(0, 8, n).astype(np.uint32); above = rng.integers(0, 256, n).astype(np.uint32)
            keys = low | (spill << np.uint32(21)) | (above << np.uint32(24))
            rc, ko, vo = P.sort_status(keys, ((0, 21),))
            assert rc == 0
            assert np.array_equal(vo, np.argsort(keys & np.uint32(0xFFFFFF), kind="stable").astype(np.uint32)), (n, stage)
            assert not np.array_equal(vo, np.argsort(keys & np.uint32(0x1FFFFF), kind="stable").astype(np.uint32))      # (the spill bits did count)
            # nine passes over a u64 key: three ranges whose digits overlap nowhere but sum to more than eight passes cannot be
            # had from 64 bits, so one range is given twice -- sorting again by a digit that is already sorted changes nothing
            k64 = make_keys(rng, n, np.uint64, ((0, 64),), "uniform")
            rc, ko, vo = P.sort_status(k64, ((0, 8), (0, 64)))
            assert rc == 0, (n, stage, rc)
            perm = np.argsort(k64, kind="stable").astype(np.uint32)
            assert np.array_equal(vo, perm) and np.array_equal(ko, k64[perm]), (n, stage)
    # n <= 1 and an empty range list: the input comes back as it is
    for keys, ranges in ((np.array([9], np.uint32), ((0, 32),)), (np.zeros(0, np.uint64), ((0, 64),)), (np.array([3, 1, 2], np.uint32), ())):
        rc, ko, vo = P.sort_status(keys, ranges)
        assert rc == 0 and np.array_equal(ko, keys) and np.array_equal(vo, np.arange(len(keys), dtype=np.uint32))


# ---- scan ------------------------------------------------------------------------------------------------------------------
def scan_ref(a, op, exclusive):
    """(output, total) in a's own dtype: sums wrap as the device's do"""
    if len(a) == 0:
        return a.copy(), a.dtype.type(0)
    inc = np.cumsum(a, dtype=a.dtype) if op == 0 else np.maximum.accumulate(a)
    if not exclusive:
        return inc, inc[-1]
    ex = np.zeros(len(a), a.dtype); ex[1:] = inc[:-1]
    return ex, inc[-1]


def scan_inputs(rng, n, dt, S):
    """(name, op, array): sums that wrap / pass 2^53, maxima over mostly-zero input with the large values where a wave or a tile hands over"""
    out = []
    if dt == np.uint32:
        out.append(("wrap", 0, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)))      # prefixes wrap past 2^32 after a few elements
        out.append(("flags", 0, (rng.random(n) < 0.3).astype(np.uint32)))
        big = lambda k: rng.integers(1 << 20, 1 << 32, k, dtype=np.uint64).astype(np.uint32)
    else:
        out.append(("2^45", 0, (np.uint64(1 << 45) + rng.integers(0, 1 << 20, n, dtype=np.uint64))))   # prefixes pass 2^53 after 256 elements
        big = lambda k: rng.integers(1 << 33, 1 << 63, k, dtype=np.uint64)
    rare = np.zeros(n, dt); hit = rng.random(n) < 0.01; rare[hit] = big(int(hit.sum()))
    out.append(("rare", 1, rare))
    for name, at in (("first", [0]), ("last", [n - 1]), ("waves", [t * S + 8 * 64 * w for t in (0, 1, 2) for w in (1, 2, 3)])):
        a = np.zeros(n, dt); at = [x for x in at if 0 <= x < n]
        if not at: continue
        if name == "waves": a[rng.random(n) < 0.02] = 7
        a[at] = np.sort(big(len(at)))     # rising: each one becomes the running maximum exactly at thread 0 of its wave
        out.append((name, 1, a))
    out.append(("uniform", 1, big(n) if n else np.zeros(0, dt)))
    return out


def check_scan(P, a, op, mode, want_total, tag):
    got, tot = P.scan(a, op, mode, want_total)
    want, wtot = scan_ref(a, op, exclusive=(op == 0 or mode == 2))
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got != want)[0])
        raise AssertionError("%s: first difference at %d of %d: got %d want %d (%d differ)" % (tag, i, len(a), got[i], want[i], int((got != want).sum())))
    assert not want_total or tot == wtot, (tag, "total", tot, wtot)


def group_scan(P):
    """device_scan, both ops and widths, out of place and in place, with and without the total, around one and several tiles"""
    S = P.S
    rng = np.random.default_rng(11)
    for n in (0, 1, 7, 8, 9, S - 1, S, S + 1, 3 * S + 5):
        for dt in (np.uint32, np.uint64):
            for name, op, a in scan_inputs(rng, n, dt, S):
                for mode in (0, 1):
                    for want_total in (True, False):
                        check_scan(P, a, op, mode, want_total, "n=%d %s %s op=%d mode=%d total=%d" % (n, np.dtype(dt).name, name, op, mode, want_total))


def group_scan_spine(P):
    """k_scan_spine alone: a one-workgroup exclusive scan whose carry crosses its iterations from S + 1 elements on"""
    S = P.S
    rng = np.random.default_rng(12)
    for n in (1, S, S + 1, 2 * S + 5):
        for dt in (np.uint32, np.uint64):
            for name, op, a in scan_inputs(rng, n, dt, S):
                for want_total in (True, False):
                    check_scan(P, a, op, 2, want_total, "spine n=%d %s %s op=%d total=%d" % (n, np.dtype(dt).name, name, op, want_total))


def group_scan_two_tile_spine(P):
    """S * S + S + 3 u32 elements (16 MiB): more than S partials, so the spine of a real device_scan takes two iterations and
    the carry of the first reaches the tiles behind it"""
    S = P.S
    n = S * S + S + 3
    rng = np.random.default_rng(13)
    check_scan(P, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), 0, 0, True, "two-tile spine, wrapping sum")
    a = np.zeros(n, np.uint32); a[[5, S * S - 1, S * S + 1]] = [9, 1 << 30, 5]; a[rng.random(n) < 0.001] = 3
    check_scan(P, a, 1, 1, True, "two-tile spine, max in place")


# ---- compaction ----------------------------------------------------------------------------------------------------------
def group_compact(P):
    S = P.S
    rng = np.random.default_rng(21)
    for n in (0, 1, 255, 256, 257, S + 1, 3 * S + 5):
        pats = {"none": np.zeros(n, np.uint32), "all": np.ones(n, np.uint32), "alternating": (np.arange(n) & 1).astype(np.uint32),
                "1%": (rng.random(n) < 0.01).astype(np.uint32)}
        for name, flag in pats.items():
            for src in (None, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)):
                out, cnt = P.compact(src, flag)
                keep = flag != 0
                assert cnt == int(keep.sum()), (n, name, cnt, int(keep.sum()))
                want = (np.arange(n, dtype=np.uint32) if src is None else src)[keep]
                assert np.array_equal(out[:cnt], want), (n, name, src is None)
                assert np.all(out[cnt:] == FILL), (n, name, "stores behind the count")


# ---- the segmented sort inside a whole build ---------------------------------------------------------------------------
def pipeline(P, stage):
    """engine == oracle on every array with every sort of more than a tile cut into two segments of several tiles"""
    from test_gpu_parity import synth
    import pfbwt_hip
    seqs = synth(5, 40000, 1)
    launches = {}
    def factory(**kw):
        ctx = pfbwt_hip.PfpContext(lib=P.lib, **kw)
        ctx.debug_set(seg_grid=2, seg_stage=stage)
        ctx.profile_enable(True)
        close = ctx.close
        def close_and_count():
            for r in ctx.profile(): launches[r["kernel"]] = launches.get(r["kernel"], 0) + r["launches"]
            close()
        ctx.close = close_and_count
        return ctx
    for U in (4, 8):
        launches.clear()
        ref = oracle_run(seqs, w=4, p=11, U=U)
        res = engine_run(factory, seqs, 4, 11, U)
        assert compare(res, ref, U) == [], U
        # a build that stayed on the one-workgroup sort proves nothing about the route
        assert launches.get("radix_hist", 0) > 0, launches
        print("U=%d radix_hist launches %d, radix_scatter %d" % (U, launches["radix_hist"], launches["radix_scatter"]))


def group_pipeline_staged(P):
    pipeline(P, 1)


def group_pipeline_unstaged(P):
    pipeline(P, 0)


def group_debug_sort(P):
    """pfp_debug_sort (tools/sort_bench.py): its own check finds no neighbours out of order and every value next to the key its
    index was given, on the one-workgroup route and on the segmented one"""
    P.L.pfp_debug_sort.argtypes = [VP, U64, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(U32), C.POINTER(U32)]
    P.route(2, 1)
    for n, bits in ((P.T - 1, 64), (2 * P.T + 1, 40), (5 * P.T + 1, 17)):
        ms, bad, wrong = C.c_double(-1), U32(7), U32(7)
        assert P.L.pfp_debug_sort(P.ctx.h, n, bits, 2, C.byref(ms), C.byref(bad), C.byref(wrong)) == 0
        assert bad.value == 0 and wrong.value == 0 and ms.value >= 0, (n, bits, bad.value, wrong.value, ms.value)


GROUPS = [k[len("group_"):] for k in list(globals()) if k.startswith("group_")]


def run_group(kind, group):
    e = dict(os.environ)
    if kind == "emu":
        subprocess.run(["make", "-C", os.path.join(ROOT, "pfbwt-f_amd"), "emu"], check=True, stdout=subprocess.DEVNULL)
        e["PFP_EMU_POISON"] = "1"
    pr = subprocess.run([sys.executable, os.path.abspath(__file__), kind, group], env=e, capture_output=True, text=True, timeout=600)
    assert pr.returncode == 0 and ("prims ok %s" % group) in pr.stdout, pr.stdout[-1500:] + pr.stderr[-3000:]


@pytest.mark.parametrize("group", GROUPS)
def test_prims_emu(group):
    run_group("emu", group)


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
def test_prims_gpu(group):
    run_group("gpu", group)


if __name__ == "__main__":
    kind, group = sys.argv[1], sys.argv[2]
    globals()["group_" + group](Prims(kind))
    print("prims ok %s" % group)
