"""First / last parse row of the groups of a run-aware emission (BWT + run samples, no full SA): with group_reduce=1 k_emit_slots
reduces them per group from the per-word table k_pack_wpq writes (emit.h), with group_reduce=0 k_big_mark reads ilist and takes
atomics per member.  Both must give the oracle's BWT and run samples, in one build and in a sliced emission, and the BWT alone.  The cases hold uniform groups of many hundreds of members
(a shared stretch behind distinct random heads: groups that span several waves and workgroups), groups of a few members, whole-word
members, lower case, N runs and IUPAC bytes (mapped to A); they run with 32- and 64-bit row counters, through both per-slot record routes (prec and the
two-gather route), with small group batches, and at both widths of the text positions.  On the CPU through tests/emu, on the card
with the product library."""
import os
import subprocess
import numpy as np
import pytest
from pfp_testlib import EMU_SO, ROOT, compare, engine_run, oracle_run

NAMES = ("bwt", "ssa", "esa")


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


def cases(copies):
    rng = np.random.default_rng(31)
    shared = rnd(rng, 60)
    out = []
    # `copies` distinct random heads in front of one shared stretch: the words that end inside the stretch share suffixes whose
    # preceding bytes lie in the stretch too -- uniform groups of about `copies` members (several workgroups of slots)
    wide = b"".join(rnd(rng, 30) + shared for _ in range(copies))
    out.append(("wide_groups", [wide], 4, 7, False))
    out.append(("wide_groups_w10", [wide, mutate(rng, wide, 40)], 10, 100, False))
    # a haplotype collection: groups of a few members, whole words, runs
    base = rnd(rng, 3000)
    out.append(("haplotypes", [mutate(rng, base, 12) for _ in range(12)], 6, 13, False))
    # lower case and IUPAC bytes, and a word that starts the text (the Dollar in front of its first byte)
    low = bytes(c + 32 if i % 5 == 0 else c for i, c in enumerate(base))
    ln = rnd(rng, 1500, b"ACGTNacgtn-")
    out.append(("lower_n", [low, base, ln, mutate(rng, ln, 6, b"ACGTN"), low, base], 4, 7, False))
    iu = rnd(rng, 1500, b"ACGTRYKMSWNacgtn")
    out.append(("iupac_ntoa", [iu, base, mutate(rng, iu, 6, b"ACGTRY"), iu], 4, 7, True))
    return out


def run_all(factory, copies, switches):
    bad = []
    for name, seqs, w, p, ntoa in cases(copies):
        for U in (4, 8):
            ref = oracle_run(seqs, w=w, p=p, U=U, non_acgt_to_a=ntoa)
            for sw in switches:
                for gr in (1, 0):
                    for rssa in (True, False):      # run samples, and the BWT alone
                        res = engine_run(with_switches(factory, group_reduce=gr, **sw), seqs, w, p, U, non_acgt_to_a=ntoa, sa=False, rssa=rssa)
                        d = compare(res, ref, U, NAMES if rssa else ("bwt",))
                        if d:
                            bad.append((name, U, sw, gr, rssa, d))
    return bad


def run_sliced(factory, copies, nslices=3):
    """pfp_bwt_build_slice: every slice runs the per-slot pass (and the reduction) again; the slices concatenated == the oracle"""
    bad = []
    name, seqs, w, p, ntoa = cases(copies)[0]
    for U in (4, 8):
        ref = oracle_run(seqs, w=w, p=p, U=U, non_acgt_to_a=ntoa)
        for gr in (1, 0):
            parts = {"bwt": [], "ssa": [], "esa": []}; r = 0
            for sl in range(nslices):
                c = with_switches(factory, group_reduce=gr)(w=w, p=p, u64=(U == 8), sai=True)
                try:
                    for s in seqs:
                        c.feed(s, True)
                    c.finalize(); c.parse_bwt()
                    b, beg, rows = c.bwt_build_slice(sl, nslices, sa=False, rssa=True)
                    o = c.bwt_get()
                finally:
                    c.close()
                for k in parts:
                    if o.get(k) is not None:
                        parts[k].append(o[k])
                r += b.r
            res = {k: np.concatenate(v) for k, v in parts.items() if v}; res["r"] = r
            d = compare(res, ref, U, NAMES)
            if d:
                bad.append((name, U, gr, d))
    return bad


SWITCHES = ({}, {"force_wide_rows": 1}, {"no_slot_records": 1}, {"emit_group_rows": 8, "big_group_members": 4})


@pytest.fixture(scope="module")
def emu_factory():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pfbwt-f_amd"), "emu"], check=True, stdout=subprocess.DEVNULL)
    import pfbwt_hip
    assert pfbwt_hip.load_library(EMU_SO).pfp_backend().decode() == "cpu-emu-TEST-ONLY"
    return lambda **kw: pfbwt_hip.PfpContext(lib=EMU_SO, **kw)


def test_group_reduce_emu(emu_factory):
    assert run_all(emu_factory, 700, SWITCHES[:2]) == []


def test_group_reduce_routes_emu(emu_factory):
    assert run_all(emu_factory, 300, SWITCHES[2:]) == []


def test_group_reduce_sliced_emu(emu_factory):
    assert run_sliced(emu_factory, 300) == []


def gpu_factory():
    import pfbwt_hip
    assert pfbwt_hip.load_library().pfp_backend().decode() == "hip-gfx950"
    return lambda **kw: pfbwt_hip.PfpContext(device=0, **kw)


@pytest.mark.gpu
def test_group_reduce_gpu():
    assert run_all(gpu_factory(), 3000, SWITCHES) == []


@pytest.mark.gpu
def test_group_reduce_sliced_gpu():
    assert run_sliced(gpu_factory(), 3000) == []
