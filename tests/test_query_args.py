"""What the pattern queries refuse and accept of a batch (csrc/queries.h: pattern_args_check, PatternBatch): pfp_ms_query, pfp_ri_count,
pfp_ri_locate and pfp_ri_docs take the same (bases, offsets, npatterns) and must treat it alike, at both widths.

The expectations are the behaviour of the entries before they shared that code; where the entries differ (pfp_ri_offsets_get after a
count: there are no positions, so PFP_E_STATE) the difference is asserted per entry.  The arrays themselves are pinned against brute
force by test_matchstats / test_runindex / test_doclist; here equal batches in different dress must give equal answers.
The text: the first 600 bases of the w4p7 fixture as two records."""
import subprocess
import os
import numpy as np
import pytest
from pfp_testlib import EMU_SO, ROOT, golden_case
from test_thresholds import build

import pfbwt_hip

E_ARG, E_STATE = pfbwt_hip.E_ARG, pfbwt_hip.E_STATE
ENTRIES = ["ms_query_flat", "ri_count_flat", "ri_locate_flat", "ri_docs_flat"]
WIDTHS = [4, 8]
_cache = {}


def text_case():
    if "text" not in _cache:
        man, recs = golden_case("w4p7")
        s = recs[0][1][:600]
        seqs = [s[:333], s[333:]]                                           # (odd lengths)
        _cache["text"] = (man["w"], man["p"], seqs, pfbwt_hip.doc_starts([len(x) for x in seqs], man["w"]))
    return _cache["text"]


def context(kind, factory, U, state):
    """state: 'ready' = every index, 'flag' = the same with non_acgt_to_a, 'bare' = a build without an index"""
    key = (kind, U, state)
    if key not in _cache:
        w, p, seqs, _ = text_case()
        ctx = build(factory, seqs, w, p, U, sa=True, rssa=True, non_acgt_to_a=(state == "flag"))
        if state != "bare":
            ctx.thresholds(); ctx.ms_index(); ctx.ri_index()
        _cache[key] = ctx
    return _cache[key]


def call(ctx, entry, bases, offsets):
    """the arrays and the info of one entry, as a list"""
    f = getattr(ctx, entry)
    return list(f(bases, offsets, text_case()[3]) if entry == "ri_docs_flat" else f(bases, offsets))


def status(ctx, entry, bases, offsets):
    with pytest.raises(pfbwt_hip.PfpError) as e:
        call(ctx, entry, bases, offsets)
    return e.value.status


def equal(a, b):
    return len(a) == len(b) and all(x == y if isinstance(x, dict) else np.array_equal(x, y) for x, y in zip(a, b))


def offsets_now(ctx, entry, count):
    """(status, offsets) of the entry's pfp_*_offsets_get"""
    fn = {"ms_query_flat": ctx.L.pfp_ms_offsets_get, "ri_docs_flat": ctx.L.pfp_ri_docs_offsets_get}.get(entry, ctx.L.pfp_ri_offsets_get)
    out, n = np.full(count + 1, 77, np.uint64), pfbwt_hip.C.c_uint64(77)
    st = fn(ctx.h, out.ctypes.data_as(pfbwt_hip.C.c_void_p), pfbwt_hip.C.byref(n))
    return st, out, n.value


def patterns():
    """a batch with a pattern that occurs, an empty one, one that does not occur, an upper / lower case mix"""
    _, _, seqs, _ = text_case()
    t = seqs[0]
    return [t[10:40], b"", t[100:117] + b"TTTTTTTTTTTT", t[200:260].lower(), t[5:6], seqs[1][-20:]]


def flat(pats):
    return pfbwt_hip.PfpContext._flat_patterns(pats)


def check_descending(ctx, entry):
    assert status(ctx, entry, b"ACGTACGT", [0, 5, 3]) == E_ARG
    assert status(ctx, entry, b"ACGTACGT", [4, 2]) == E_ARG                # (also when the last offset lies below the first)
    assert status(ctx, entry, b"ACGTACGT", [0, 5, 3, 8]) == E_ARG


def check_zero_byte(ctx, entry):
    assert status(ctx, entry, b"ACG\x00T", [0, 5]) == E_ARG
    assert status(ctx, entry, b"ACGT\x00", [0, 2, 5]) == E_ARG             # in the last byte
    assert status(ctx, entry, b"\x00ACGT", [0, 0, 5]) == E_ARG             # behind an empty pattern
    bases, off = flat(patterns())
    assert equal(call(ctx, entry, b"\x00" + bases + b"\x00", off + np.uint64(1)), call(ctx, entry, bases, off))      # (outside the batch: not looked at)


def check_zero_byte_with_flag(ctx, entry):
    pats = patterns()
    bases, off = flat(pats)
    zero = bytearray(bases)
    at = [int(off[0]) + 3, int(off[3]) + 7, int(off[6]) - 1]               # inside the first and the fourth pattern, the last byte
    want = bytearray(bases)
    for x in at:
        zero[x] = 0; want[x] = ord("A")
    got = call(ctx, entry, bytes(zero), off)
    assert equal(got, call(ctx, entry, bytes(want), off))
    assert got[-1]["patterns"] == len(pats) and got[-1]["bases"] == len(bases)


def check_no_patterns(ctx, entry):
    got = call(ctx, entry, b"", [0])
    assert all(a.size == (1 if k in OFFSET_ARRAYS[entry] else 0) for k, a in enumerate(got[:-1])), got
    assert got[-1]["patterns"] == 0 and got[-1]["bases"] == 0
    for k in OFFSET_ARRAYS[entry]:
        assert got[k].tolist() == [0]
    st, out, n = offsets_now(ctx, entry, 0)
    if entry == "ri_count_flat":
        assert st == E_STATE                                                # a count has no positions and no offsets
    else:
        assert st == 0 and out.tolist() == [0] and n == 0
    assert equal(got, call(ctx, entry, b"ACGT", [2]))                       # (bases given, none of them used)


# which of the returned arrays are offsets (one more value than there are patterns)
OFFSET_ARRAYS = {"ms_query_flat": (), "ri_count_flat": (), "ri_locate_flat": (1,), "ri_docs_flat": (1,)}


def check_all_empty(ctx, entry):
    got = call(ctx, entry, b"", [0, 0, 0, 0])
    info = got[-1]
    assert info["patterns"] == 3 and info["bases"] == 0
    if entry == "ms_query_flat":
        assert got[0].size == 0 and got[1].size == 0 and info["breaks"] == 0
    else:
        cnt = got[0] if entry != "ri_locate_flat" else got[2]
        assert cnt.tolist() == [0, 0, 0] and info["found"] == 0 and info["occurrences"] == 0      # (include/pfbwt_hip.h: an empty pattern has cnt = 0 and no values)
        assert all(a.size == 0 for k, a in enumerate(got[:-1]) if a is not cnt and k not in OFFSET_ARRAYS[entry])
    for k in OFFSET_ARRAYS[entry]:
        assert got[k].tolist() == [0, 0, 0, 0]
    if entry != "ri_count_flat":
        st, out, n = offsets_now(ctx, entry, 3)
        assert st == 0 and out.tolist() == [0, 0, 0, 0] and n == 3
    assert equal(got, call(ctx, entry, b"ACGT", [3, 3, 3, 3]))


def check_rebased(ctx, entry):
    bases, off = flat(patterns())
    want = call(ctx, entry, bases, off)
    assert want[-1]["patterns"] == 6 and want[-1]["bases"] == len(bases)
    for front in (1, 7, 4096):
        got = call(ctx, entry, b"G" * front + bases + b"TT", off + np.uint64(front))
        assert equal(got, want), front
    if entry == "ms_query_flat":
        st, out, n = offsets_now(ctx, entry, 6)
        assert st == 0 and out.tolist() == off.tolist() and n == 6          # the offsets of the result start at 0


def check_before_index(ctx, entry):
    bases, off = flat(patterns())
    assert status(ctx, entry, bases, off) == E_STATE
    assert status(ctx, entry, b"ACGTACGT", [0, 5, 3]) == E_STATE            # the state wins over descending offsets
    assert status(ctx, entry, b"ACG\x00T", [0, 5]) == E_STATE               # and over a 0 byte
    assert status(ctx, entry, b"", [0]) == E_STATE


CASES = {"descending": ("ready", check_descending), "zero_byte": ("ready", check_zero_byte), "zero_byte_with_flag": ("flag", check_zero_byte_with_flag),
         "no_patterns": ("ready", check_no_patterns), "all_empty": ("ready", check_all_empty), "rebased": ("ready", check_rebased),
         "before_index": ("bare", check_before_index)}


def check(kind, factory, entry, U, case):
    state, f = CASES[case]
    f(context(kind, factory, U, state), entry)


@pytest.fixture(scope="module", autouse=True)
def close_contexts():
    yield
    for key in [k for k in _cache if isinstance(k, tuple)]:
        _cache.pop(key).close()


# ---- CPU: the emulated library -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pfbwt-f_amd"), "emu"], check=True, stdout=subprocess.DEVNULL)
    return lambda **kw: pfbwt_hip.PfpContext(lib=EMU_SO, **kw)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("U", WIDTHS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_query_args_emu(emu, entry, U, case):
    check("emu", emu, entry, U, case)


# ---- GPU: the product library --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("U", WIDTHS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_query_args_gpu(gpu_ctx_factory, entry, U, case):
    check("gpu", gpu_ctx_factory, entry, U, case)
