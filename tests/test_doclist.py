"""Document listing with frequencies on the device (include/pfbwt_hip.h: pfp_ri_docs; csrc/doclist.h; pfbwt-f --doclist / --doclist-inside /
--doclist-max).

The expected values never come from the engine: for every pattern all bytes.find occurrences of the normalised pattern in the oracle's
text, numpy.searchsorted on the record starts, the INSIDE rule as the header writes it (s + m <= b_{doc(s)+1} - w) and a Counter.
test_checkers_agree shows, without any engine, that this agrees with test_runindex.brute_locate + doc_starts on every fixture, that the
sum of the frequencies plus the outside occurrences is the count, and that the checker refuses a dropped document, a swapped pair and
a frequency off by one.
Every check runs with each reduction route forced (dl_wave_max / dl_table_max 0 in turn, both 0, the defaults) and with chunks of 1 and
7 rows and the default budget; all arrays must be equal to brute force in every variant.  The fixtures have a handful of records, so a
panel of 300 short records is seeded and built here (many_docs); its record table is also merged down to 1, 2, 64, 65 and 257
documents -- across one wave and one tile of counters -- refined to a document every 4, 2 and 1 bytes (above 1024, 4096 and 8192
documents: the larger tables of counters, the large LDS table of starts, the two-level bisection) and run with doc_lds_max forced
small; a fixture with a document every 4 bytes has more documents than the table route takes.
The fixture cases take text and SA from the oracle alone (the models of test_runindex / test_matchstats cost half a minute on the large
fixtures, which this file's GPU tests would pay for first)."""
import os
import subprocess
from collections import Counter
import numpy as np
import pytest
from pfp_testlib import EMU_SO, GOLDEN, ROOT, golden_case, oracle_run
from test_thresholds import build, read_u, run, same
from test_matchstats import FIXTURES, normalise
from test_runindex import brute_locate, brute_occurrences, inverse_sa, seeded_case, seeded_texts, text_patterns

import pfbwt_hip

EMUB = os.path.join(ROOT, "tests", "emu", "build")
BIN = os.path.join(ROOT, "pfbwt-f_amd", "bin")
INFO_KEYS = ["patterns", "bases", "found", "occurrences", "listed", "skipped", "outside", "entries", "max_docs", "chunks", "by_wave", "by_table", "by_sort", "route"]
DEFAULTS = {"dl_chunk_values": 0, "dl_wave_max": 64, "dl_table_max": 16384, "ri_route": 0}
# every reduction route forced, then chunks of 1 and 7 rows (the default budget is far above every batch here: one chunk)
VARIANTS = [{}, {"dl_wave_max": 0}, {"dl_table_max": 0}, {"dl_wave_max": 0, "dl_table_max": 0}, {"dl_chunk_values": 1}, {"dl_chunk_values": 7},
            {"dl_chunk_values": 7, "dl_wave_max": 0, "dl_table_max": 0}, {"dl_chunk_values": 1, "dl_wave_max": 0}]
BLOCK = 256                  # lanes per workgroup of the kernels (csrc/common.h)
MAX_COUNT = 2000             # a pattern that occurs more often is not asked for on the fixtures (brute force lists its occurrences)
INSIDE_CLASSES = ["ends_at_limit", "one_past_limit", "inside_pad", "across_border", "last_record", "all_dropped"]


# ---- the checkers ------------------------------------------------------------------------------------------------------------
def brute_docs(text, starts, w, P, inside):
    """(cnt, documents ascending, frequencies, outside) of the normalised pattern P"""
    occ = np.array(brute_occurrences(text, P), np.int64)
    if not occ.size:
        return 0, [], [], 0
    b = np.asarray(starts, np.int64)
    d = np.searchsorted(b, occ, side="right") - 1
    end = np.append(b[1:], len(text))[d]
    keep = (occ + len(P) <= end - w) if inside else np.ones(occ.size, bool)
    c = Counter(d[keep].tolist())
    docs = sorted(c)
    return int(occ.size), docs, [c[k] for k in docs], int((~keep).sum())


class Expected:
    """the patterns of one text and one record table, and what brute force says about them"""

    def __init__(self, text, starts, w, pats, non_acgt_to_a=False):
        self.text, self.starts, self.w = text, np.asarray(starts, np.uint64), w
        self.pats = [bytes(p) for p in pats]
        self.norm = [normalise(p, non_acgt_to_a) for p in self.pats]
        self.bases = sum(len(p) for p in self.pats)
        self._got = {}

    def with_table(self, starts):
        return Expected(self.text, starts, self.w, self.pats)

    def lists(self, inside):
        if inside not in self._got:
            self._got[inside] = [brute_docs(self.text, self.starts, self.w, P, inside) for P in self.norm]
        return self._got[inside]

    def cnt(self):
        return np.array([g[0] for g in self.lists(False)], np.uint64)

    def info(self, inside, max_count, route, tun):
        """tun: the switches of the call (missing: the defaults)"""
        t = dict(DEFAULTS); t.update(tun)
        ls, nd = self.lists(inside), int(self.starts.size)
        skip = [bool(max_count) and g[0] > max_count for g in ls]
        rows = [0 if s else g[0] for g, s in zip(ls, skip)]
        lens = [0 if s else len(g[1]) for g, s in zip(ls, skip)]
        wave = sum(1 for c in rows if 0 < c <= t["dl_wave_max"])
        table = sum(1 for c in rows if c > t["dl_wave_max"] and nd <= t["dl_table_max"])
        chunks, j = 0, 0
        budget = t["dl_chunk_values"] or (1 << 62)
        while j < len(rows):                                               # patterns in order while their rows fit the budget, one at least
            total, k = rows[j], j + 1
            while k < len(rows) and total + rows[k] <= budget:
                total += rows[k]; k += 1
            chunks += 1; j = k
        return dict(patterns=len(self.pats), bases=self.bases, found=sum(g[0] > 0 for g in ls), occurrences=sum(g[0] for g in ls), listed=sum(n > 0 for n in lens), skipped=sum(skip),
                    outside=sum(0 if s else g[3] for g, s in zip(ls, skip)), entries=sum(lens), max_docs=max(lens or [0]), chunks=chunks, by_wave=wave, by_table=table,
                    by_sort=sum(c > 0 for c in rows) - wave - table, route=route)

    def check(self, got, inside, max_count, route, tun, tag):
        """got: what PfpContext.ri_docs returned"""
        cnt, docs, freqs, info = got
        ls = self.lists(inside)
        assert same(cnt, self.cnt()), (tag, "cnt")
        assert len(docs) == len(freqs) == len(ls), tag
        for j, g in enumerate(ls):
            skip = bool(max_count) and g[0] > max_count
            want_d, want_f = ([], []) if skip else (g[1], g[2])
            assert docs[j].tolist() == want_d, (tag, "documents of pattern", j, self.pats[j][:40], docs[j].tolist()[:20], want_d[:20])
            assert freqs[j].tolist() == want_f, (tag, "frequencies of pattern", j, self.pats[j][:40], freqs[j].tolist()[:20], want_f[:20])
            if not skip and want_d:
                assert sum(want_f) == g[0] - g[3], (tag, j)
        want = self.info(inside, max_count, route, tun)
        assert info == want, (tag, info, want)

    def inside_classes(self):
        """how many occurrences / patterns fall into every class of INSIDE_CLASSES"""
        have = {c: 0 for c in INSIDE_CLASSES}
        b = self.starts.astype(np.int64)
        n, w = len(self.text), self.w
        ends = np.append(b[1:], n)
        for P, g in zip(self.norm, self.lists(True)):
            m = len(P)
            for s in brute_occurrences(self.text, P):
                d = int(np.searchsorted(b, s, side="right")) - 1
                lim = int(ends[d]) - w
                have["ends_at_limit"] += s + m == lim
                have["one_past_limit"] += s + m == lim + 1
                have["inside_pad"] += s >= lim and s + m <= int(ends[d])
                have["across_border"] += s < lim and s + m > int(ends[d])
                have["last_record"] += d == b.size - 1 and s + m == n - w
            have["all_dropped"] += g[0] > 0 and not g[1]
        return have


def inside_patterns(text, starts, w):
    """patterns around the end of a record in the middle, and of the last one"""
    b = [int(x) for x in starts] + [len(text)]
    k = (len(b) - 1) // 2
    e = b[k + 1] - w                                                       # the first pad byte behind record k
    out = [text[max(e - 10, b[k]):e], text[max(e - 9, b[k]):e + 1], b"A" * w, b"A" * (w - 1), text[len(text) - w - 10:len(text) - w]]
    if k + 1 < len(b) - 1:
        out.append(text[max(e - 5, b[k]):e + w + 5])                       # across the border into record k + 1
    return [p for p in out if p]


def equal_results(a, b):
    return same(a[0], b[0]) and len(a[1]) == len(b[1]) and all(np.array_equal(x, y) for x, y in zip(a[1] + a[2], b[1] + b[2]))


def run_variants(ctx, exp, has_sa, tag, variants=VARIANTS, max_counts=(0,)):
    """every variant, with and without PFP_DL_INSIDE, against brute force; the locate routes on the first variant"""
    for inside in (False, True):
        first = None
        for vi, tun in enumerate(variants):
            ctx.debug_set(**dict(DEFAULTS, **tun))
            routes = ([1, 2] if has_sa else [1]) if vi == 0 else [0]
            for r in routes:
                ctx.debug_set(ri_route=r)
                used = r if r else (2 if has_sa else 1)
                for mc in max_counts:
                    got = ctx.ri_docs(exp.pats, exp.starts, inside=inside, max_count=mc)
                    exp.check(got, inside, mc, used, tun, (tag, "inside", inside, tun, "ri_route", r, "max_count", mc))
                    if mc == 0:
                        assert first is None or equal_results(first, got), (tag, "variants differ", tun)
                        first = first or got
    ctx.debug_set(**DEFAULTS)


_cache = {}


def fixture_case(case):
    if case not in _cache:
        man, recs = golden_case(case)                                       # (the oracle alone: the models of the other query tests cost half a minute on the large fixtures)
        seqs = [s for _, s in recs]
        ref = oracle_run(seqs, w=man["w"], p=man["p"], U=8)
        text, w = bytes(ref["text"]), man["w"]
        starts = pfbwt_hip.doc_starts([len(s) for s in seqs], w)
        rng = np.random.default_rng(FIXTURES.index(case) + 170)
        pats = text_patterns(rng, text, 64, 300)
        pats = [p for p in pats if text.count(normalise(p, False)[:4] or b"#") <= 4 * MAX_COUNT]
        pats = [p for p in pats if len(brute_occurrences(text, normalise(p, False))) <= MAX_COUNT]
        pats += inside_patterns(text, starts, w)
        pats.insert(5, b"")
        _cache[case] = (man, seqs, Expected(text, starts, w, pats), ref)
    return _cache[case]


def seeded_dl_case(ci, c):
    """None: the oracle or the index refuses the text"""
    key = ("seeded", ci)
    if key not in _cache:
        got = seeded_case(ci, c)
        if got is None or got[2] is None:
            _cache[key] = None
        else:
            ref, model, riexp, _ = got
            starts = pfbwt_hip.doc_starts([len(s) for s in c["seqs"]], c["w"])
            pats = riexp.pats[:50] + inside_patterns(model.text, starts, c["w"])
            _cache[key] = Expected(model.text, starts, c["w"], pats, c["non_acgt_to_a"])
    return _cache[key]


# ---- the many-document panel -----------------------------------------------------------------------------------------------------
MOTIF = b"GTCCGATAGCTT"
TAG = b"TGGCATTC"
PANEL_W, PANEL_P, PANEL_RECORDS, PANEL_SEED = 4, 5, 300, 4260      # (the seed: a text whose .bwt holds no EndOfWord byte, which pfp_ri_index refuses for such tiny w / p)
PLANTED = {12: 1, 10: 63, 9: 64, 8: 65, 7: 256, 6: 257}                    # prefix of MOTIF -> the records that hold it


def many_docs():
    """(seqs, patterns by name): 300 records of 24 .. 40 bases -- record 0 has a tandem repeat on top -- each with TAG once and at most
    one prefix of MOTIF planted, so that MOTIF[:k] occurs in exactly PLANTED[k] records, once in each; records 7 and 299 are equal"""
    if "panel" in _cache:
        return _cache["panel"]
    rng = np.random.default_rng(PANEL_SEED)
    ks = sorted(PLANTED, reverse=True)
    klass = []                                                             # the longest prefix a record holds (0: none)
    for k in ks:
        klass += [k] * (PLANTED[k] - len(klass))
    klass += [0] * (PANEL_RECORDS - 2 - len(klass))
    klass = [klass[i] for i in rng.permutation(len(klass))]
    klass.insert(7, 0)                                                     # (record 7, the one with a twin, holds no prefix)
    seqs = []
    for i, k in enumerate(klass):
        while True:
            plant = b"" if not k else MOTIF[:k] + (b"" if k == 12 else bytes(rng.choice([x for x in b"ACGT" if x != MOTIF[k]], 1).astype(np.uint8)))
            L = int(rng.integers(24, 41))
            free = L - len(TAG) - len(plant)
            fill = bytes(rng.choice(list(b"ACGT"), free).astype(np.uint8))
            cut = int(rng.integers(0, free + 1))
            s = TAG + fill[:cut] + plant + fill[cut:]
            if s.count(TAG) == 1 and s.count(MOTIF[:6]) == (1 if k else 0) and b"AAAA" not in s:
                break
        seqs.append(s)
    seqs[0] = seqs[0] + b"AC" * 80                                          # the tandem repeat: one document with 79 occurrences of ACAC
    seqs.append(seqs[7])                                                    # two equal records
    named = {"c0": MOTIF[:11] + (b"A" if MOTIF[11:] != b"A" else b"C"), "c1": MOTIF, "c63": MOTIF[:10], "c64": MOTIF[:9], "c65": MOTIF[:8], "c256": MOTIF[:7], "c257": MOTIF[:6],
             "every_record": TAG, "tandem": b"ACAC", "twin": seqs[7]}
    _cache["panel"] = (seqs, named)
    return _cache["panel"]


def panel_case():
    if "panel_exp" not in _cache:
        seqs, named = many_docs()
        ref = oracle_run(seqs, w=PANEL_W, p=PANEL_P, U=8)
        assert ref.get("err") is None and not (np.asarray(ref["bwt"]) == 1).any(), "the oracle or pfp_ri_index would refuse the panel"
        text = ref["text"].tobytes() if hasattr(ref["text"], "tobytes") else bytes(ref["text"])
        starts = pfbwt_hip.doc_starts([len(s) for s in seqs], PANEL_W)
        rng = np.random.default_rng(PANEL_SEED + 1)
        pats = list(named.values()) + text_patterns(rng, text, 16, 30) + inside_patterns(text, starts, PANEL_W) + [b"", b"X"]
        _cache["panel_exp"] = (seqs, named, Expected(text, starts, PANEL_W, pats))
    return _cache["panel_exp"]


def assert_panel_classes(exp, named):
    """the counts the panel was built for really occur"""
    names = list(named)
    got = {k: exp.lists(False)[names.index(k)] for k in names}
    assert [got[k][0] for k in ("c0", "c1", "c63", "c64", "c65", "c256", "c257")] == [0, 1, 63, 64, 65, 256, 257]
    assert all(len(got[k][1]) == got[k][0] for k in ("c1", "c63", "c64", "c65", "c256", "c257"))      # once per record
    assert got["every_record"][1] == list(range(PANEL_RECORDS)) and set(got["every_record"][2]) == {1}
    assert max(got["tandem"][2]) >= 70 and got["tandem"][1][0] == 0 and len(got["tandem"][1]) > 1
    assert got["twin"][1] == [7, PANEL_RECORDS - 1] and got["twin"][2] == [1, 1]
    missing = [c for c, v in exp.inside_classes().items() if not v]
    assert not missing, missing


def merged(starts, k):
    """the table cut down to k documents by merging neighbouring records"""
    s = np.asarray(starts, np.uint64)
    return s[np.arange(k) * s.size // k]


# a document every `step` bytes of the panel: (1024, 4096] documents take k_dl_table<4096> and the large LDS table of starts, (4096, 8192]
# k_dl_table<16384>, above 8192 the starts are bisected in two levels
FINE_TABLES = [(4, (1024, 4096)), (2, (4096, 8192)), (1, (8192, 16384))]


def fine_case(step):
    key = ("fine", step)
    if key not in _cache:
        exp = panel_case()[2]
        _cache[key] = exp.with_table(np.arange(0, len(exp.text) - 1, step, dtype=np.uint64))
    return _cache[key]


def check_panel(factory):
    seqs, named, exp = panel_case()
    assert_panel_classes(exp, named)
    for U, sa in ((4, False), (8, True)):
        ctx = build(factory, seqs, PANEL_W, PANEL_P, U, sa=sa, rssa=True)
        ctx.ri_index()                                                     # the index accepts the text
        run_variants(ctx, exp, sa, ("panel", U))
        for k in (1, 2, 64, 65, 257):
            sub = exp.with_table(merged(exp.starts, k))
            assert sub.starts.size == k and sub.starts[0] == 0
            run_variants(ctx, sub, sa, ("panel", U, "documents", k), variants=VARIANTS[:4] + VARIANTS[5:6])
        for lds in (2, 3, 7, 64):                                          # the two-level bisection: every 2^shift-th start in LDS, the rest in global memory
            ctx.debug_set(doc_lds_max=lds)
            run_variants(ctx, exp, sa, ("panel", U, "doc_lds_max", lds), variants=VARIANTS[:1] + VARIANTS[3:4])
        ctx.debug_set(doc_lds_max=8192)
        for step, tabs in FINE_TABLES:                                     # a document every `step` bytes: the larger tables of counters and of starts
            sub = fine_case(step)
            assert tabs[0] < sub.starts.size <= tabs[1] and sub.info(False, 0, 1, {})["by_table"] > 0, sub.starts.size
            run_variants(ctx, sub, sa, ("panel", U, "a document every", step), variants=VARIANTS[:4] + VARIANTS[6:7])
        ctx.close()
    # more documents than the table route takes: the sort route by default, the start table in two levels
    man, seqs, exp, _ = fixture_case("single_chrom")
    sub = Expected(exp.text, np.arange(0, len(exp.text) - 1, 4, dtype=np.uint64), man["w"], exp.pats[:24] + [exp.text[:2], exp.text[7:10]])
    want = sub.info(False, 0, 1, {})
    assert sub.starts.size > 16384 and want["by_sort"] > 0 and want["by_table"] == 0 and want["by_wave"] > 0, (sub.starts.size, want)
    ctx = build(factory, seqs, man["w"], man["p"], 4, sa=False, rssa=True)
    ctx.ri_index()
    run_variants(ctx, sub, False, ("single_chrom", "a document every 4"), variants=VARIANTS[:2] + [{"dl_chunk_values": 100}])
    ctx.close()


def check_fixtures(factory, cases=FIXTURES, light=()):
    have = {c: 0 for c in INSIDE_CLASSES}
    for case in cases:
        for c, v in fixture_case(case)[2].inside_classes().items():
            have[c] += v
    assert all(have.values()), have
    for ci, case in enumerate(cases):
        man, seqs, exp, _ = fixture_case(case)
        for U, sa in ([(8, True)] if case in light else [(4, bool(ci % 2)), (8, not ci % 2)]):
            ctx = build(factory, seqs, man["w"], man["p"], U, sa=sa, rssa=True)
            ctx.ri_index()
            run_variants(ctx, exp, sa, (case, U), variants=VARIANTS[:2] + VARIANTS[3:4] + VARIANTS[5:6] if case in light else VARIANTS)
            ctx.close()


def check_seeded(factory):
    reached = 0
    for ci, c in enumerate(seeded_texts()):
        exp = seeded_dl_case(ci, c)
        if exp is None:
            continue
        for U in (4, 8):
            sa = c["sa"] if U == c["U"] else not c["sa"]
            ctx = build(factory, c["seqs"], c["w"], c["p"], U, sa=sa, rssa=True, non_acgt_to_a=c["non_acgt_to_a"])
            ctx.ri_index()
            run_variants(ctx, exp, sa, ("seeded", ci, U))
            ctx.close()
        reached += 1
    assert reached >= 5, reached


def check_batch_shapes(factory):
    """max_count around a count K; 0 patterns, only empty or absent patterns, BLOCK and BLOCK + 1 patterns, a chunk border on an empty
    pattern, one pattern larger than the chunk budget"""
    seqs, named, exp = panel_case()
    text, rng = exp.text, np.random.default_rng(11)
    pieces = [text[a:a + 9] for a in rng.integers(0, len(text) - 9, BLOCK + 1).tolist()]
    shapes = [[], [b"", b"X", b"", b"XX"], pieces[:BLOCK], pieces, [named["c64"], b"", named["c65"], b"", b"", named["c1"]], [named["c1"], named["every_record"], named["c1"]]]
    ctx = build(factory, seqs, PANEL_W, PANEL_P, 4, sa=False, rssa=True)
    ctx.ri_index()
    for q, pats in enumerate(shapes):
        sub = Expected(text, exp.starts, PANEL_W, pats)
        tuns = [{}, {"dl_chunk_values": 64}, {"dl_chunk_values": 65}, {"dl_chunk_values": 7, "dl_table_max": 0}] if q >= 4 else [{}, {"dl_chunk_values": 1}]
        run_variants(ctx, sub, False, ("shape", q), variants=tuns)
    got = ctx.ri_docs([], exp.starts)
    assert got[0].size == 0 and got[1] == [] and got[3]["chunks"] == 0 and got[3]["entries"] == 0
    # max_count: K is listed, K + 1 is skipped
    sub = Expected(text, exp.starts, PANEL_W, [named["c64"], named["c65"], named["c1"], named["c257"]])
    for K in (64, 65, 1, 256, 257):
        for tun in ({}, {"dl_chunk_values": 7}):
            ctx.debug_set(**dict(DEFAULTS, **tun))
            for inside in (False, True):
                got = ctx.ri_docs(sub.pats, sub.starts, inside=inside, max_count=K)
                sub.check(got, inside, K, 1, tun, ("max_count", K, tun, inside))
                assert got[3]["skipped"] == sum(c > K for c in (64, 65, 1, 257)) and same(got[0], [64, 65, 1, 257])
    ctx.debug_set(**DEFAULTS)
    ctx.close()


def check_state_and_errors(factory):
    E_STATE, E_ARG, E_NOMEM, E_TOO_LARGE = pfbwt_hip.E_STATE, pfbwt_hip.E_ARG, pfbwt_hip.E_NOMEM, pfbwt_hip.E_TOO_LARGE
    man, seqs, exp, ref = fixture_case("mult_chroms_fa")
    w, p = man["w"], man["p"]
    C = pfbwt_hip.C
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    small = Expected(exp.text, exp.starts, w, exp.pats[:30])
    other = Expected(exp.text, exp.starts, w, exp.pats[30:45])
    pats, starts = small.pats, small.starts
    buf = np.empty(1 << 16, np.uint64)
    bases = np.frombuffer(b"ACGTACGT", np.uint8)
    off = np.array([0, 4], np.uint64)

    def status(f, *a, **kw):
        with pytest.raises(pfbwt_hip.PfpError) as e:
            f(*a, **kw)
        return e.value.status

    def nothing_made(ctx):
        L = ctx.L
        return (L.pfp_ri_docs_get(ctx.h, vp(buf), None, None) == E_STATE and L.pfp_ri_docs_get(ctx.h, None, None, None) == E_STATE and L.pfp_ri_docs_write(ctx.h, -1, -1, -1, -1) == E_STATE
                and L.pfp_ri_docs_offsets_get(ctx.h, vp(buf), None) == E_STATE and ctx.ri_docs_device_ptrs() == [None] * 3)

    def raw(ctx, b=bases, o=off, np_=1, st=starts, nd=None, flags=0):
        return ctx.L.pfp_ri_docs(ctx.h, None if b is None else vp(b), None if o is None else vp(o), np_, None if st is None else vp(st), st.size if nd is None and st is not None else (nd or 0), flags, 0, None)

    ctx = factory(w=w, p=p, u64=True, sai=True)
    L = ctx.L
    assert L.pfp_ri_docs(None, vp(bases), vp(off), 1, vp(starts), starts.size, 0, 0, None) == E_ARG and L.pfp_ri_docs_get(None, None, None, None) == E_ARG
    assert L.pfp_ri_docs_write(None, -1, -1, -1, -1) == E_ARG and L.pfp_ri_docs_offsets_get(None, None, None) == E_ARG and L.pfp_ri_docs_device_ptrs(None, None, None, None) == E_ARG
    assert L.pfp_ri_docs_file(None, b"x", vp(starts), starts.size, 0, 0, None) == E_ARG
    assert raw(ctx) == E_STATE and nothing_made(ctx)                                                       # no build at all
    for s in seqs:
        ctx.feed(s, True)
    ctx.finalize(); ctx.parse_bwt(); ctx.bwt_build(sa=True, rssa=True)
    assert status(ctx.ri_docs, pats, starts) == E_STATE and nothing_made(ctx)                             # no index
    assert L.pfp_ri_docs_file(ctx.h, b"/nonexistent", vp(starts), starts.size, 0, 0, None) == E_STATE
    ctx.ri_index()                                                                                        # needs nothing else
    assert nothing_made(ctx)
    assert L.pfp_ri_docs_file(ctx.h, b"/nonexistent", vp(starts), starts.size, 0, 0, None) == -9          # PFP_E_IO
    assert L.pfp_ri_docs_file(ctx.h, None, vp(starts), starts.size, 0, 0, None) == E_ARG
    before = ctx.bwt_get()
    loc_before = ctx.ri_locate(pats)
    # arguments
    assert raw(ctx, b=None) == E_ARG and raw(ctx, o=None) == E_ARG and raw(ctx, st=None) == E_ARG and raw(ctx, nd=0) == E_ARG and nothing_made(ctx)
    assert raw(ctx, flags=2) == E_ARG and raw(ctx, flags=1 << 31) == E_ARG                                # unknown flag bits
    assert status(ctx.ri_docs_flat, bases, [0, 5, 3], starts) == E_ARG                                     # descending offsets
    assert status(ctx.ri_docs, [b"ACG", b"AC\x00T"], starts) == E_ARG                                      # a 0 byte
    n = len(exp.text)
    for bad in ([1, 5], [0, 5, 5], [0, 9, 5], [0, n], [0, 5, n + 3]):                                      # a bad table
        assert status(ctx.ri_docs, pats, np.array(bad, np.uint64)) == E_ARG, bad
    assert raw(ctx, np_=1 << 32) == E_TOO_LARGE and raw(ctx, nd=1 << 32) == E_TOO_LARGE and nothing_made(ctx)
    assert raw(ctx) == 0                                                                                  # info is nullable
    n1 = C.c_uint64(7)
    assert L.pfp_ri_docs_offsets_get(ctx.h, None, C.byref(n1)) == 0 and n1.value == 1
    a = ctx.ri_docs_flat(bases, [2, 6, 8], starts)                                                         # offsets need not start at 0
    b = ctx.ri_docs([b"GTAC", b"GT"], starts)
    assert same(a[0], b[0]) and same(a[2], np.concatenate(b[1])) and same(a[3], np.concatenate(b[2])) and a[4] == b[3]
    # the results: their own slot, beside count / locate
    first = ctx.ri_docs(pats, starts)
    small.check(first, False, 0, 2, {}, "state")
    d = ctx.ri_docs_device_ptrs()
    assert all(d) and len(set(d)) == 3
    cnt_now, pos_now = np.empty(len(pats), np.uint64), np.empty(int(loc_before[1].sum()), np.uint64)
    assert L.pfp_ri_get(ctx.h, vp(cnt_now), vp(pos_now)) == 0 and same(cnt_now, loc_before[1]) and same(pos_now, np.concatenate(loc_before[0]))      # pfp_ri_get unchanged by a listing
    flat = ctx.ri_docs_flat(*ctx._flat_patterns(pats), starts)

    def still_there(tag):
        cnt, doc, freq, doff = np.empty(len(pats), np.uint64), np.empty(flat[2].size, np.uint64), np.empty(flat[3].size, np.uint64), np.empty(len(pats) + 1, np.uint64)
        assert L.pfp_ri_docs_get(ctx.h, vp(cnt), vp(doc), vp(freq)) == 0 and L.pfp_ri_docs_offsets_get(ctx.h, vp(doff), None) == 0, tag
        assert same(cnt, flat[0]) and same(doff, flat[1]) and same(doc, flat[2]) and same(freq, flat[3]), tag

    still_there("at once")
    ctx.thresholds(); ctx.ms_index(); ctx.ri_index(); ctx.lcp_array(); ctx.doc_array(starts); ctx.ms_query(pats); ctx.mem_find(1, locate=True)
    still_there("after the other passes")
    ctx.mem_find(2); ctx.ms_query(pats[:3]); ctx.doc_array(starts); ctx.lcp_array(); ctx.ri_index(); ctx.ms_index(); ctx.thresholds()
    still_there("after the other passes, other order")
    ctx.ri_count(other.pats); still_there("after a count")
    ctx.ri_locate(other.pats); still_there("after a locate")
    assert ctx.ri_docs_device_ptrs() == d
    ctx.debug_set(ri_route=1)
    small.check(ctx.ri_docs(pats, starts, inside=True), True, 0, 1, {}, "phi beside the SA")
    ctx.debug_set(ri_route=0)
    other.check(ctx.ri_docs(other.pats, starts), False, 0, 2, {}, "a second call replaces the first")
    n1 = C.c_uint64(0)
    assert L.pfp_ri_docs_offsets_get(ctx.h, None, C.byref(n1)) == 0 and n1.value == len(other.pats)
    after = ctx.bwt_get()                                                                                 # the published build is unchanged
    for k in ("bwt", "sa", "ssa", "esa"):
        assert np.array_equal(before[k], after[k]), k
    assert same(after["ssa"], ref["ssa"]) and same(after["bwt"], ref["bwt"]) and same(after["esa"], ref["esa"])
    # a new build drops them; without an SA route 2 is refused
    ctx.bwt_build(sa=False, rssa=True)
    assert nothing_made(ctx) and status(ctx.ri_docs, pats, starts) == E_STATE
    ctx.ri_index()
    small.check(ctx.ri_docs(pats, starts), False, 0, 1, {}, "rssa only")
    ctx.debug_set(ri_route=2)
    assert status(ctx.ri_docs, pats, starts) == E_STATE                                                   # the SA route without an SA
    ctx.debug_set(ri_route=0)
    ctx.bwt_build_slice(0, 2, sa=True, rssa=True)                                                         # a slice
    assert status(ctx.ri_docs, pats, starts) == E_STATE
    ctx.close()
    # a context filled by pfp_bwt_load answers the same arrays
    for sa in (True, False):
        ctx = factory(w=w, p=p, u64=True, sai=True)
        ctx.bwt_load(ref["dict"], ref["occ"], ref["bwlast"], ref["ilist"], ref["bwsai"], n_hint=ref["n"])
        ctx.bwt_build(sa=sa, rssa=True)
        ctx.ri_index()
        for inside in (False, True):
            small.check(ctx.ri_docs(pats, starts, inside=inside), inside, 0, 2 if sa else 1, {}, ("loaded", sa, inside))
        ctx.close()
    # PFP_E_NOMEM from a small workspace leaves a following call with max_count working
    ctx = None
    for mib in (24, 32, 48, 64, 96):
        try:
            ctx = build(lambda **kw: factory(workspace_bytes=mib << 20, **kw), seqs, w, p, 8, sa=False, rssa=True)
            ctx.ri_index()
            break
        except pfbwt_hip.PfpError as e:
            assert e.status == E_NOMEM
            ctx = None
    assert ctx is not None
    t = exp.text
    singles = [t[a:a + 1] for a in range(4)]
    fine = np.arange(0, len(t) - 1, 2, dtype=np.uint64)                                                   # a document every two bytes: the upper bound of the pairs is the counts
    loc = ctx.ri_locate(pats)
    assert status(ctx.ri_docs, singles * 4000, fine) == E_NOMEM and nothing_made(ctx)
    assert ctx.L.pfp_workspace_needed(ctx.h) > (mib << 20)
    cnt_now, pos_now = np.empty(len(pats), np.uint64), np.empty(int(loc[1].sum()), np.uint64)
    assert L.pfp_ri_get(ctx.h, vp(cnt_now), vp(pos_now)) == 0 and same(cnt_now, loc[1]) and same(pos_now, np.concatenate(loc[0]))      # every other result as it was
    cnt, docs, freqs, info = ctx.ri_docs(singles * 4000, fine, max_count=1000)
    assert info["skipped"] == 16000 and info["entries"] == 0 and info["listed"] == 0 and all(x.size == 0 for x in docs)
    for q, S in enumerate(singles):
        assert same(cnt[q::4], np.full(4000, t.count(normalise(S, False))))
    small.check(ctx.ri_docs(pats, starts), False, 0, 1, {}, "after NOMEM")
    ctx.debug_set(dl_wave_max=1000, dl_table_max=1 << 20, dl_chunk_values=-5)                             # values out of range are clamped
    small.check(ctx.ri_docs(pats, starts), False, 0, 1, {}, "clamped")
    with pytest.raises(pfbwt_hip.PfpError):
        ctx.debug_set(dl_wave=3)
    ctx.close()


# ---- command line ------------------------------------------------------------------------------------------------------------
def check_cli(exe, factory, tmp):
    """exe: {'pfbwt-f': path, 'pfbwt-f64': path}"""
    man, seqs, exp, _ = fixture_case("mult_chroms_fa")
    fa = os.path.join(GOLDEN, "mult_chroms_fa", "input.fa")
    wp = ["-w", str(man["w"]), "-p", str(man["p"])]
    reads = [p for p in exp.pats[:50] if p]
    sub = Expected(exp.text, exp.starts, man["w"], reads)
    K = sorted(int(c) for c in sub.cnt() if c > 1)[0]
    fasta, fastq = os.path.join(tmp, "reads.fa"), os.path.join(tmp, "reads.fq")
    with open(fasta, "wb") as f:
        for j, r in enumerate(reads):
            f.write(b">r%d some words\n" % j + b"\n".join(r[k:k + 60] for k in range(0, len(r), 60)) + b"\n")
    with open(fastq, "wb") as f:
        for j, r in enumerate(reads):
            f.write(b"@r%d\n" % j + r + b"\n+\n" + b"@" * len(r) + b"\n")
    EXT = ("dl.cnt", "dl.off", "dl.doc", "dl.freq")

    def files(pref):
        return {e: open(pref + "." + e, "rb").read() for e in ("bwt", "sa", "ssa", "esa", "cnt", "dict", "occ", "parse", "bwlast", "ilist", "n", "da", "sda") if os.path.exists(pref + "." + e)}

    def same_files(pref, f, U):
        assert same(read_u(pref + ".dl.cnt", U), f[0]) and same(read_u(pref + ".dl.doc", U), f[2]) and same(read_u(pref + ".dl.freq", U), f[3]), pref
        assert same(read_u(pref + ".dl.off", 8), f[1]) and os.path.getsize(pref + ".dl.off") == 8 * (len(reads) + 1), pref

    for name, U in (("pfbwt-f64", 8), ("pfbwt-f", 4)):
        ctx = build(factory, seqs, man["w"], man["p"], U, sa=True, rssa=True)
        ctx.ri_index()
        bases, off = ctx._flat_patterns(reads)
        plain_dl, inside_dl, capped_dl = ctx.ri_docs_flat(bases, off, sub.starts), ctx.ri_docs_flat(bases, off, sub.starts, inside=True), ctx.ri_docs_flat(bases, off, sub.starts, inside=True, max_count=K)
        sub.check(ctx.ri_docs(reads, sub.starts), False, 0, 2, {}, name)
        ctx.close()
        # FASTA reads and -r alone on one program, FASTQ reads beside -s --count on the other; every other output file: byte-identical
        rd, extra = (fasta, ["-r"]) if U == 8 else (fastq, ["-r", "-s", "--count", fasta])
        pref, plain = os.path.join(tmp, "dl_%d" % U), os.path.join(tmp, "plain_%d" % U)
        pr = run([exe[name]] + extra + wp + ["--doclist", rd, "-o", pref, fa])
        assert "TASK\tdoclist\t" in pr.stderr and "doclist: %d reads, %d found, %d occurrences, %d listed, %d pairs" % (len(reads), plain_dl[4]["found"], plain_dl[4]["occurrences"], plain_dl[4]["listed"], plain_dl[4]["entries"]) in pr.stderr
        same_files(pref, plain_dl, U)
        run([exe[name]] + extra + wp + ["-o", plain, fa])
        a, b = files(pref), files(plain)
        assert a == b and "bwt" in a and "ssa" in a and not any(os.path.exists(plain + "." + e) for e in EXT), (name, rd, sorted(a), sorted(b))
        pref = os.path.join(tmp, "capped_%d" % U)
        pr = run([exe[name], "-r", "--doclist", fastq if U == 8 else fasta, "--doclist-inside", "--doclist-max", str(K)] + wp + ["-o", pref, fa])
        same_files(pref, capped_dl, U)
        assert "%d skipped" % capped_dl[4]["skipped"] in pr.stderr and capped_dl[4]["skipped"] > 0
        if U == 8:
            pref = os.path.join(tmp, "inside_%d" % U)
            run([exe[name], "-r", "--doclist", fastq, "--doclist-inside"] + wp + ["-o", pref, fa])
            same_files(pref, inside_dl, U)
            nodocs = os.path.join(tmp, "no_docs_%d" % U)                                               # --pfbwt-only without <prefix>.docs
            run([exe[name], "--parse-only", "-r"] + wp + ["-o", nodocs, fa])
            pr = run([exe[name], "--pfbwt-only", "-r", "--doclist", fasta] + wp + ["-o", nodocs], check=False)
            assert pr.returncode != 0 and "--doclist with --pfbwt-only needs %s.docs (write it with --parse-only --print-docs)" % nodocs in pr.stderr
        else:
            pref = os.path.join(tmp, "two_steps_%d" % U)                                               # --pfbwt-only: the records come from <prefix>.docs
            run([exe[name], "--parse-only", "-r", "--print-docs"] + wp + ["-o", pref, fa])
            run([exe[name], "--pfbwt-only", "-r", "--doclist", fasta] + wp + ["-o", pref])
            same_files(pref, plain_dl, U)
    efa = os.path.join(GOLDEN, "edge", "input.fa")

    def refused(args, opt, word, prefix):
        pr = run([exe["pfbwt-f64"]] + args + ["-w", "10", "-p", "20", "-o", prefix, efa], check=False)
        assert pr.returncode != 0 and opt in pr.stderr and word in pr.stderr.split("Command line")[-1].split("\n", 1)[1], pr.stderr[-500:]
        for e in ("bwt", "dict") + EXT:
            assert not os.path.exists(prefix + "." + e), (args, e)

    refused(["--doclist", fasta], "--doclist", "-r", os.path.join(tmp, "no_r"))
    refused(["--doclist", fasta, "-r", "--gpus", "2"], "--doclist", "--gpus", os.path.join(tmp, "gpus"))
    refused(["--doclist", fasta, "-r", "--parse-only"], "--doclist", "--parse-only", os.path.join(tmp, "parse_only"))
    refused(["--doclist-inside", "-r"], "--doclist-inside", "--doclist ", os.path.join(tmp, "no_doclist"))
    refused(["--doclist-max", "3", "-r"], "--doclist-max", "--doclist ", os.path.join(tmp, "no_doclist2"))
    h = run([exe["pfbwt-f"], "-h"]).stderr
    assert "--doclist <reads>" in h and "--doclist-inside" in h and "--doclist-max <K>" in h


def test_checkers_agree():
    """brute force against brute_locate + doc_starts on every fixture, without any engine; the sum of the frequencies and the outside
    occurrences is the count; the panel's classes occur; the checker refuses a dropped document, a swapped pair and a frequency off by one"""
    assert [f for f, _ in pfbwt_hip.DlInfo._fields_] == INFO_KEYS
    for case in FIXTURES:
        man, seqs, exp, ref = fixture_case(case)
        isa = inverse_sa(ref["sa"])
        assert same(exp.starts, pfbwt_hip.doc_starts([len(s) for s in seqs], man["w"]))
        b = exp.starts.astype(np.int64)
        for inside in (False, True):
            for P, g in zip(exp.norm, exp.lists(inside)):
                c, pos = brute_locate(exp.text, isa, P, 0)
                d = np.searchsorted(b, np.array(pos, np.int64), side="right") - 1 if pos else np.zeros(0, np.int64)
                assert c == g[0] and sum(g[2]) + g[3] == c and all(f >= 1 for f in g[2]) and g[1] == sorted(set(g[1]))
                if not inside:
                    assert g[3] == 0 and g[1] == sorted(set(d.tolist())) and g[2] == [int((d == k).sum()) for k in g[1]]
                else:
                    assert set(g[1]) <= set(d.tolist())
        assert exp.info(True, 0, 1, {})["outside"] > 0
    assert max(fixture_case(case)[2].info(False, 0, 1, {})["max_docs"] for case in FIXTURES) >= 2
    seqs, named, pexp = panel_case()
    assert_panel_classes(pexp, named)
    assert 9000 <= len(pexp.text) <= 13000 and len(seqs) == PANEL_RECORDS
    for k in (1, 2, 64, 65, 257):
        assert merged(pexp.starts, k).size == k
    i0 = pexp.info(False, 0, 1, {})
    assert i0["by_wave"] > 0 and i0["by_table"] > 0 and pexp.info(False, 0, 1, {"dl_table_max": 0})["by_sort"] == i0["by_table"] and pexp.info(False, 0, 1, {"dl_chunk_values": 7})["chunks"] > 10
    # the checker refuses wrong answers
    ls = pexp.lists(False)
    arr = lambda k: [np.array(g[k], np.uint64) for g in ls]
    good = (pexp.cnt(), arr(1), arr(2), pexp.info(False, 0, 1, {}))
    pexp.check(good, False, 0, 1, {}, "good")
    j = list(named).index("c64")
    for what in ("dropped", "swapped", "off_by_one"):
        docs, freqs = list(good[1]), list(good[2])
        if what == "dropped":
            docs[j], freqs[j] = docs[j][1:], freqs[j][1:]
        elif what == "swapped":
            docs[j] = np.concatenate([docs[j][1:2], docs[j][0:1], docs[j][2:]])
        else:
            freqs[j] = np.concatenate([freqs[j][:1] + 1, freqs[j][1:]])
        with pytest.raises(AssertionError):
            pexp.check((good[0], docs, freqs, good[3]), False, 0, 1, {}, what)


# ---- CPU: the emulated library -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pfbwt-f_amd"), "emu", "emu-host"], check=True, stdout=subprocess.DEVNULL)
    return lambda **kw: pfbwt_hip.PfpContext(lib=EMU_SO, **kw)


def test_doclist_fixtures_emu(emu):
    check_fixtures(emu, light=("panel8",))


def test_doclist_seeded_emu(emu):
    check_seeded(emu)


def test_doclist_panel_emu(emu):
    check_panel(emu)


def test_doclist_batch_shapes_emu(emu):
    check_batch_shapes(emu)


def test_doclist_state_and_errors_emu(emu):
    check_state_and_errors(emu)


def test_doclist_cli_emu(emu, tmp_path):
    check_cli({"pfbwt-f": os.path.join(EMUB, "pfbwt-f-emu"), "pfbwt-f64": os.path.join(EMUB, "pfbwt-f64-emu")}, emu, str(tmp_path))


# ---- GPU: the product library --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_doclist_fixtures_gpu(gpu_ctx_factory):
    check_fixtures(gpu_ctx_factory)


@pytest.mark.gpu
def test_doclist_seeded_gpu(gpu_ctx_factory):
    check_seeded(gpu_ctx_factory)


@pytest.mark.gpu
def test_doclist_panel_gpu(gpu_ctx_factory):
    check_panel(gpu_ctx_factory)


@pytest.mark.gpu
def test_doclist_batch_shapes_gpu(gpu_ctx_factory):
    check_batch_shapes(gpu_ctx_factory)


@pytest.mark.gpu
def test_doclist_state_and_errors_gpu(gpu_ctx_factory):
    check_state_and_errors(gpu_ctx_factory)


@pytest.mark.gpu
def test_doclist_cli_gpu(gpu_ctx_factory, tmp_path):
    check_cli({"pfbwt-f": os.path.join(BIN, "pfbwt-f"), "pfbwt-f64": os.path.join(BIN, "pfbwt-f64")}, gpu_ctx_factory, str(tmp_path))
