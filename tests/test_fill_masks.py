"""Run masks of the one-pass run sampling (BWT + run samples, no full SA).  With fill_masks=1 k_fill stores the 16-bit run mask of every
full piece of 16 rows it writes, k_run_masks_fix recomputes the masks that the final bytes of the special rows change (and those
k_fill cannot know: the first row of a slot list, the window's first and last piece) and k_mask_tile_count counts the run starts per
tile from the masks; with fill_masks=0, and whenever a window starts off a multiple of 16, k_run_tile_count reads the window's bytes
back.  With fill_skip=1 k_fill's slot compaction bisects over the slots without rows instead of walking them.  Every combination
must give the oracle's .bwt, .ssa, .esa and r: 32- and 64-bit row counters, small group batches with the sort route, a sample
overflow (the exact route follows), windows of 4096, 16400 (a multiple of 16 but not of 4096) and 777 rows (unaligned: falls back),
and a sliced emission (slices behind the first start unaligned).  The profile's launch counts tell which route ran, so that a
silent fallback cannot pass for the new route.  On the CPU through tests/emu (PFP_EMU_POISON=1 in the environment fills fresh memory
with garbage: a mask nobody wrote shows), on the card with the product library."""
import os
import subprocess
import numpy as np
import pytest
from pfp_testlib import EMU_SO, ROOT, compare, oracle_run

NAMES = ("bwt", "ssa", "esa")
U_ALL = (4, 8)

# switch settings of the issue; True: the windows start at multiples of 16, so fill_masks=1 must take the new route
SETTINGS = (
    ({}, True),
    ({"force_wide_rows": 1}, True),
    ({"emit_group_rows": 8, "big_group_members": 4}, True),
    ({"sample_cap": 40}, True),
    ({"emit_chunk_rows": 4096}, True),
    ({"emit_chunk_rows": 16400}, True),
    ({"emit_chunk_rows": 777}, False),
    ({"emit_group_rows": 0, "emit_chunk_rows": 4096}, True),      # no packed records of the special slots: the fix-up reads the per-slot ones
)
MODES = ((1, 1), (1, 0), (0, 1), (0, 0))      # (fill_masks, fill_skip)


def rnd(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(list(alphabet), n).astype(np.uint8))


def mutate(rng, s, k, alphabet=b"ACGT"):
    a = bytearray(s)
    for i in rng.integers(0, len(a), k):
        a[i] = alphabet[rng.integers(0, len(alphabet))]
    return bytes(a)


def cases(copies):
    rng = np.random.default_rng(77)
    out = []
    # test_group_reduce's wide_groups: `copies` random heads in front of one shared stretch -- clusters of thousands of slots
    # without rows (suffixes of length <= w) and uniform groups that span workgroups
    shared = rnd(rng, 60)
    wide = b"".join(rnd(rng, 30) + shared for _ in range(copies))
    out.append(("wide_groups", [wide], 4, 7, False))
    # mutated haplotypes: special groups of a few members, whole words, stretches that end at every residue modulo 16
    base = rnd(rng, 10000)
    out.append(("haplotypes", [mutate(rng, base, 14) for _ in range(14)], 6, 13, False))
    # more than 40 000 rows: k_fill starts several slot lists at multiples of 4096, window edges fall inside special groups
    b2 = rnd(rng, 4200)
    out.append(("rows_40k", [mutate(rng, b2, 9) for _ in range(10)], 5, 11, False))
    # lower case, N and '-'
    low = bytes(c + 32 if i % 5 == 0 else c for i, c in enumerate(base[:3000]))
    ln = rnd(rng, 1500, b"ACGTNacgtn-")
    out.append(("lower_n", [low, base[:3000], ln, mutate(rng, ln, 6, b"ACGTN"), low], 4, 7, False))
    return out


DEFAULTS = {"force_wide_rows": 0, "emit_group_rows": 4096, "big_group_members": -2, "sample_cap": -1, "emit_chunk_rows": 0}


class Parsed:
    """A context that holds the parse and the parse BWT of a collection: every emission (the switches are read per build) runs on it.
    Its workspace has room for the one-pass sample arrays: with the default of a small text the samples always take the exact route."""

    def __init__(self, factory, seqs, w, p, U, ntoa):
        self.c = factory(w=w, p=p, u64=(U == 8), non_acgt_to_a=ntoa, sai=True, workspace_bytes=1 << 30)
        try:
            for s in seqs:
                self.c.feed(s, True)
            self.c.finalize(); self.c.parse_bwt()
            self.c.profile_enable(True)
        except Exception:
            self.c.close()
            raise

    def close(self):
        self.c.close()

    def build(self, sw, slices=None):
        """-r build(s): (arrays and r, launches of `run_masks` and of `runs` per build, first row of every build)"""
        c = self.c
        c.debug_set(**dict(DEFAULTS, **sw))
        parts = {k: [] for k in NAMES}
        r = 0; launches = []; begins = []
        for sl in range(slices or 1):
            c.profile_reset()
            if slices:
                b, beg, _ = c.bwt_build_slice(sl, slices, sa=False, rssa=True)
            else:
                b, beg = c.bwt_build(sa=False, rssa=True), 0
            o = c.bwt_get()
            prof = {row["kernel"]: row["launches"] for row in c.profile()}
            for k in NAMES:
                parts[k].append(o[k])
            r += b.r; begins.append(beg)
            launches.append((prof.get("run_masks", 0), prof.get("runs", 0)))
        res = {k: np.concatenate(v) for k, v in parts.items()}
        res["r"] = r
        return res, launches, begins


def route_errors(launches, new_route, overflow):
    """new route: two `run_masks` launches per window and no `runs` launch (none but the exact route's after an overflow);
    old route: no `run_masks` launch at all"""
    bad = []
    for nm, nr in launches:
        if new_route:
            if nm == 0 or nm % 2 or (nr != 0 and not overflow) or (overflow and nr * 2 != nm):
                bad.append("new route expected: run_masks %d, runs %d" % (nm, nr))
        elif nm != 0 or nr == 0:
            bad.append("old route expected: run_masks %d, runs %d" % (nm, nr))
    return bad


def run_all(factory, copies, settings=SETTINGS, modes=MODES, us=U_ALL):
    bad = []
    for name, seqs, w, p, ntoa in cases(copies):
        for U in us:
            ref = oracle_run(seqs, w=w, p=p, U=U, non_acgt_to_a=ntoa)
            if name == "rows_40k":
                assert ref["n"] + 1 >= 40000
            ctx = Parsed(factory, seqs, w, p, U, ntoa)
            try:
                for sw, aligned in settings:
                    for fm, fs in modes:
                        res, launches, _ = ctx.build(dict(sw, fill_masks=fm, fill_skip=fs))
                        d = compare(res, ref, U, NAMES) + route_errors(launches, fm == 1 and aligned, "sample_cap" in sw)
                        if d:
                            bad.append((name, U, sw, fm, fs, d))
            finally:
                ctx.close()
    return bad


def run_sliced(factory, copies, nslices=3):
    """pfp_bwt_build_slice: the slices concatenated == the oracle; a slice that starts off a multiple of 16 takes the old route
    (slice 0 starts at row 0 and takes the new one)"""
    bad = []
    name, seqs, w, p, ntoa = cases(copies)[0]
    for U in U_ALL:
        ref = oracle_run(seqs, w=w, p=p, U=U, non_acgt_to_a=ntoa)
        ctx = Parsed(factory, seqs, w, p, U, ntoa)
        try:
            for fm, fs in MODES:
                res, launches, begins = ctx.build({"fill_masks": fm, "fill_skip": fs}, slices=nslices)
                assert all(b % 16 for b in begins[1:]), begins      # the case is what it claims to be
                d = compare(res, ref, U, NAMES)
                for la, beg in zip(launches, begins):
                    d += route_errors([la], fm == 1 and beg % 16 == 0, False)
                if d:
                    bad.append((name, U, fm, fs, d))
        finally:
            ctx.close()
    return bad


@pytest.fixture(scope="module")
def emu_factory():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pfbwt-f_amd"), "emu"], check=True, stdout=subprocess.DEVNULL)
    import pfbwt_hip
    assert pfbwt_hip.load_library(EMU_SO).pfp_backend().decode() == "cpu-emu-TEST-ONLY"
    return lambda **kw: pfbwt_hip.PfpContext(lib=EMU_SO, **kw)


def test_fill_masks_emu(emu_factory):
    assert run_all(emu_factory, 700) == []


def test_fill_masks_sliced_emu(emu_factory):
    assert run_sliced(emu_factory, 700) == []


def gpu_factory():
    import pfbwt_hip
    assert pfbwt_hip.load_library().pfp_backend().decode() == "hip-gfx950"
    return lambda **kw: pfbwt_hip.PfpContext(device=0, **kw)


@pytest.mark.gpu
def test_fill_masks_gpu():
    assert run_all(gpu_factory(), 3000) == []


@pytest.mark.gpu
def test_fill_masks_sliced_gpu():
    assert run_sliced(gpu_factory(), 3000) == []
