"""What pfp_shard_load and pfp_merge_shards refuse, and what they leave behind: every case is rejected by a host check or by the
kernels' own `bad` counters (nothing reads out of bounds), the context that refused is empty afterwards, the shard contexts are
untouched, and the same inputs, repaired, give the oracle's single parse."""
import numpy as np
import pytest
from pfp_testlib import compare, oracle_run
from test_sharded import emu_factory, one_phrase_cases, synth  # noqa: F401  (emu_factory is a fixture)
import pfbwt_hip

W, P = 4, 7
PARSE_NAMES = ("dict", "occ", "parse", "last", "sai", "bwlast", "ilist", "bwsai")


def status_of(call, *args):
    with pytest.raises(pfbwt_hip.PfpError) as e:
        call(*args)
    return e.value.status


def merged_parse(g, views):
    sz = g.merge_shards(views)
    res = {"n": sz.n, "m": sz.m, "dwords": sz.dwords, "dsize": sz.dsize}
    res.update(g.parse_get()); g.parse_bwt(); res.update(g.parse_bwt_get())
    return res


def view_fields(v):
    return [getattr(v, k) for k, _ in v._fields_]


# ---- pfp_shard_load ---------------------------------------------------------------------------------------------------------
def bad_image(case, d, p):
    """(dictionary image, parse, status) of a damaged copy of the valid image (d, p); the dictionary image is in rank order:
    words that end in EndOfWord = 1, then EndOfDict = 0"""
    dwords = int((d == 1).sum())
    if case == "no_tail": return d[:-2], p, pfbwt_hip.E_CORRUPT
    if case == "end_of_word_only": return d[:-1], p, pfbwt_hip.E_CORRUPT
    if case == "tiny_dict": return d[-2:], p, pfbwt_hip.E_ARG                 # dsize < 3 (with a good tail: the size is what is refused)
    if case == "empty_parse": return d, p[:0], pfbwt_hip.E_ARG
    q = p.copy()
    if case == "rank_zero": q[len(q) // 2] = 0; return d, q, pfbwt_hip.E_CORRUPT
    if case == "rank_past_end": q[len(q) // 3] = dwords + 1; return d, q, pfbwt_hip.E_CORRUPT
    if case == "short_word":      # a word of w bytes in front (rank 1), every other rank moves up by one; one phrase refers to it
        d2 = np.concatenate([np.frombuffer(b"ACGT"[:W] + b"\x01", np.uint8), d])
        q = q + 1; q[len(q) // 2] = 1
        return d2, q, pfbwt_hip.E_CORRUPT
    raise KeyError(case)


LOAD_CASES = ("no_tail", "end_of_word_only", "tiny_dict", "empty_parse", "rank_zero", "rank_past_end", "short_word")
_load_ref = {}


def load_inputs(U):
    if U not in _load_ref:
        seqs = synth(3, 3000, 2)
        _load_ref[U] = (oracle_run(seqs, w=W, p=P, U=U, want_sa=False), [oracle_run([s], w=W, p=P, U=U, want_sa=False) for s in seqs])
    return _load_ref[U]


def check_shard_load_rejects(factory, case, U):
    ref, parts = load_inputs(U)
    a, b, g = (factory(w=W, p=P, u64=(U == 8), sai=True) for _ in range(3))
    d, p, want = bad_image(case, parts[0]["dict"], parts[0]["parse"])
    assert status_of(a.shard_load, d, p) == want
    assert status_of(a.shard_view) == pfbwt_hip.E_STATE
    a.shard_load(parts[0]["dict"], parts[0]["parse"])                     # the same context takes a valid image
    b.shard_load(parts[1]["dict"], parts[1]["parse"])
    assert compare(merged_parse(g, [a.shard_view(), b.shard_view()]), ref, U, names=PARSE_NAMES) == []
    for c in (a, b, g): c.close()


@pytest.mark.parametrize("U", [4, 8])
@pytest.mark.parametrize("case", LOAD_CASES)
def test_shard_load_rejects_emu(emu_factory, case, U):
    check_shard_load_rejects(emu_factory, case, U)


@pytest.mark.gpu
@pytest.mark.parametrize("U", [4, 8])
@pytest.mark.parametrize("case", LOAD_CASES)
def test_shard_load_rejects_gpu(gpu_ctx_factory, case, U):
    check_shard_load_rejects(gpu_ctx_factory, case, U)


# ---- pfp_merge_shards -------------------------------------------------------------------------------------------------------
def damage_view(case, views):
    """damages views in place; returns (status, compact)"""
    if case == "context_on_view0": views[0].left_context = W; return pfbwt_hip.E_ARG, False
    if case == "context_not_w": views[2].left_context = W - 1; return pfbwt_hip.E_ARG, False
    if case == "ye_without_last": views[1].d_last = None; return pfbwt_hip.E_ARG, False
    if case == "last_without_ye": views[2].d_ye = None; return pfbwt_hip.E_ARG, False
    if case == "no_pid": views[2].d_pid = None; return pfbwt_hip.E_ARG, False
    if case == "no_phrases": views[1].m = 0; return pfbwt_hip.E_ARG, False
    if case == "compact_n_plus_1": views[0].n += 1; return pfbwt_hip.E_CORRUPT, True
    raise KeyError(case)


MERGE_CASES = ("context_on_view0", "context_not_w", "ye_without_last", "last_without_ye", "no_pid", "no_phrases", "compact_n_plus_1")
_merge_ref = {}


def merge_inputs(U):
    """two haplotypes with a record of ONE phrase between them (the one-base record of one_phrase_cases())"""
    if U not in _merge_ref:
        hap = synth(3, 3000, 2)
        tiny = one_phrase_cases()[3][0][3]
        seqs = [hap[0], tiny, hap[1]]
        _merge_ref[U] = (seqs, oracle_run(seqs, w=W, p=P, U=U, want_sa=False))
    return _merge_ref[U]


def check_merge_rejects(factory, case, U):
    seqs, ref = merge_inputs(U)
    ctxs = []
    for s in seqs:
        c = factory(w=W, p=P, u64=(U == 8), sai=True)                     # every shard parsed on its own: the merge re-tests the seams
        c.feed(s, True); c.finalize(shard=True)
        ctxs.append(c)
    before = [view_fields(c.shard_view()) for c in ctxs]
    assert before[1][1] == 1                                              # the middle shard is a single phrase
    g = factory(w=W, p=P, u64=(U == 8), sai=True)
    views = [c.shard_view() for c in ctxs]
    want, compact = damage_view(case, views)
    if compact:
        for v in views: v.d_ye = v.d_last = None
    assert status_of(g.merge_shards, views) == want
    assert g.L.pfp_parse_get(g.h, None, None, None, None, None) == pfbwt_hip.E_STATE      # the merging context is empty
    assert [view_fields(c.shard_view()) for c in ctxs] == before                           # the shards are untouched
    views = [c.shard_view() for c in ctxs]                                                 # the same views, repaired
    if compact:
        for v in views: v.d_ye = v.d_last = None
    assert compare(merged_parse(g, views), ref, U, names=PARSE_NAMES) == []
    for c in ctxs + [g]: c.close()


@pytest.mark.parametrize("U", [4, 8])
@pytest.mark.parametrize("case", MERGE_CASES)
def test_merge_shards_rejects_emu(emu_factory, case, U):
    check_merge_rejects(emu_factory, case, U)


@pytest.mark.gpu
@pytest.mark.parametrize("U", [4, 8])
@pytest.mark.parametrize("case", MERGE_CASES)
def test_merge_shards_rejects_gpu(gpu_ctx_factory, case, U):
    check_merge_rejects(gpu_ctx_factory, case, U)
