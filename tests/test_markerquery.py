"""Marker queries on the device (include/pfbwt_hip.h: pfp_mk_index / pfp_mk_query; csrc/markerquery.h; pfbwt-f --mps / --ma / --markers).

The expected values never come from the engine.  For every probed suffix of a pattern all bytes.find occurrences in the oracle's text
are listed; with the .mps stream the array was made from, an occurrence at s carries the list of the mps interval that holds s (the
text-space form of the header), and freq(X) counts the occurrences whose list holds X.  The counters of `info` that speak about
records (records, raw, the routes, the chunks) need the record structure of the .ma stream: that is oracle/marker_oracle.py's
marker_array on the oracle's SA, never the engine's.  test_checkers_agree shows without any engine that the text-space form agrees
with the row-space definition (rows of the interval against the records of the oracle's .ma stream), that the classes the kernels
branch on occur, and that the checker refuses a dropped pair, a swapped pair and a frequency off by one.
Hand-made .ma streams (check_lists) have no .mps stream: there an occurrence at s carries the list of the record that holds row
ISA[s], which is the definition itself."""
import os
import subprocess
import sys
from collections import Counter
import numpy as np
import pytest
from pfp_testlib import EMU_SO, GOLDEN, ROOT, golden_case, oracle_run
from test_thresholds import build, read_u, run, same
from test_matchstats import normalise
from test_runindex import inverse_sa, seeded_texts, text_patterns
from test_markers import fixture as marker_fixture, seeded_mps

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import marker_oracle as mo

import pfbwt_hip

EMUB = os.path.join(ROOT, "tests", "emu", "build")
BIN = os.path.join(ROOT, "pfbwt-f_amd", "bin")
INDEX_KEYS = ["records", "entries", "distinct", "max_list", "rows"]
INFO_KEYS = ["patterns", "bases", "found", "occurrences", "steps", "probes", "capped", "rows", "records", "raw", "listed", "entries", "max_markers", "chunks", "by_wave", "by_sort"]
DEFAULTS = {"mk_chunk_entries": 0, "mk_wave_max": 64}
VARIANTS = [{}, {"mk_wave_max": 0}, {"mk_chunk_entries": 1}, {"mk_chunk_entries": 7}, {"mk_chunk_entries": 7, "mk_wave_max": 0}]
MODES = [(0, 0), (8, 0), (8, 4), (1, 50)]                                  # (min_len, max_rows)
CASES = ["single_chrom", "mult_chroms"]
DELIM = int(mo.DELIM)


# ---- the checkers ------------------------------------------------------------------------------------------------------------
class Model:
    """one text with its SA and one marker array: `mps` (then the array is the oracle's, and frequencies are counted in text space)
    or a .ma stream `ma` (frequencies by the row of every occurrence)"""

    def __init__(self, text, sa, mps=None, ma=None):
        self.text, self.n = bytes(text), len(text)
        self.isa = inverse_sa(sa)
        self.ma = np.asarray(mo.marker_array(mps, sa) if ma is None else ma, np.uint64)
        f, l, lists = mo.mps_parse(self.ma)
        self.first, self.last = np.array(f, np.int64), np.array(l, np.int64)
        self.sets = [sorted(set(x)) for x in lists]
        self.cum = np.concatenate([[0], np.cumsum([len(x) for x in self.sets], dtype=np.int64)]).astype(np.int64)
        self.text_space = mps is not None
        if self.text_space:
            s, e, ls = mo.mps_parse(mps)
            keep = [k for k in range(len(s)) if ls[k]]
            self.ps, self.pe, self.psets = np.array([s[k] for k in keep], np.int64), np.array([e[k] for k in keep], np.int64), [sorted(set(ls[k])) for k in keep]
        self._occ, self._probe = {}, {}

    def index_info(self):
        return dict(records=len(self.sets), entries=int(self.cum[-1]), distinct=len({x for s in self.sets for x in s}), max_list=max([len(s) for s in self.sets] or [0]),
                    rows=int((self.last - self.first + 1).sum()))

    def occ(self, S, limit=0):
        """the occurrences of S in the text; limit > 0: None as soon as there are more than `limit`"""
        if S in self._occ:
            o = self._occ[S]
            return None if limit and o.size > limit else o
        out, i = [], self.text.find(S)
        while i >= 0:
            out.append(i)
            if limit and len(out) > limit:
                return None
            i = self.text.find(S, i + 1)
        self._occ[S] = np.array(out, np.int64)
        return self._occ[S]

    def probe(self, S):
        """(cnt, text-space or by-row frequencies, row-space frequencies, record overlaps, raw entries) of one probed string"""
        if S not in self._probe:
            o = self.occ(S)
            rows = self.isa[o]
            lo, hi = int(rows.min()), int(rows.min()) + o.size
            assert int(rows.max()) == hi - 1, "the occurrences of a string are an interval of rows"
            ka, kb = int(np.searchsorted(self.last, lo, side="left")), int(np.searchsorted(self.first, hi, side="left"))
            rf = Counter()
            for k in range(ka, kb):
                wgt = min(hi, int(self.last[k]) + 1) - max(lo, int(self.first[k]))
                assert wgt >= 1
                for X in self.sets[k]:
                    rf[X] += wgt
            tf = Counter()
            if self.text_space:
                k = np.searchsorted(self.ps, o, side="right") - 1
                ok = (k >= 0) & (o <= self.pe[np.maximum(k, 0)]) if self.ps.size else np.zeros(o.size, bool)
                for kk, c in zip(*np.unique(k[ok], return_counts=True)):
                    for X in self.psets[int(kk)]:
                        tf[X] += int(c)
            else:
                k = np.searchsorted(self.first, rows, side="right") - 1
                ok = (k >= 0) & (rows <= self.last[np.maximum(k, 0)]) if self.first.size else np.zeros(o.size, bool)
                for kk, c in zip(*np.unique(k[ok], return_counts=True)):
                    for X in self.sets[int(kk)]:
                        tf[X] += int(c)
            self._probe[S] = (int(o.size), tf, rf, kb - ka, int(self.cum[kb] - self.cum[ka]), (lo, hi, ka, kb))
        return self._probe[S]

    def query(self, P, min_len, max_rows):
        """P: a normalised pattern"""
        m = len(P)
        out = dict(cnt=0, probes=0, capped=0, rows=0, records=0, raw=0, steps=0, freq=Counter(), rfreq=Counter(), spans=[])
        if not m:
            return out
        fail = -1                                                          # the longest suffix start whose suffix does not occur
        for i in range(m - 1, -1, -1):
            if self.text.find(P[i:]) < 0:
                fail = i
                break
        out["steps"] = m - fail if fail >= 0 else m
        out["cnt"] = int(self.occ(P).size) if fail < 0 else 0
        for i in ([0] if not min_len else range(0, m - min_len + 1)):
            if i <= fail:
                continue
            S = P[i:]
            if max_rows and self.occ(S, max_rows) is None:
                out["capped"] += 1
                continue
            c, tf, rf, recs, raw, span = self.probe(S)
            out["probes"] += 1; out["rows"] += c; out["records"] += recs; out["raw"] += raw
            out["freq"].update(tf); out["rfreq"].update(rf); out["spans"].append(span)
        return out


class Expected:
    """the patterns of one model and what brute force says about them"""

    def __init__(self, model, pats, non_acgt_to_a=False):
        self.model, self.pats = model, [bytes(p) for p in pats]
        self.norm = [normalise(p, non_acgt_to_a) for p in self.pats]
        self.bases = sum(len(p) for p in self.pats)
        self._got = {}

    def answers(self, min_len, max_rows):
        key = (min_len, max_rows)
        if key not in self._got:
            self._got[key] = [self.model.query(P, min_len, max_rows) for P in self.norm]
        return self._got[key]

    def info(self, min_len, max_rows, tun):
        t = dict(DEFAULTS); t.update(tun)
        qs = self.answers(min_len, max_rows)
        raws, lens = [q["raw"] for q in qs], [len(q["freq"]) for q in qs]
        chunks, j, budget = 0, 0, t["mk_chunk_entries"] or (1 << 62)
        while j < len(raws):                                               # patterns in order while their raw entries fit the budget, one at least
            total, k = raws[j], j + 1
            while k < len(raws) and total + raws[k] <= budget:
                total += raws[k]; k += 1
            chunks += 1; j = k
        wave = sum(1 for r in raws if 0 < r <= t["mk_wave_max"])
        return dict(patterns=len(qs), bases=self.bases, found=sum(q["cnt"] > 0 for q in qs), occurrences=sum(q["cnt"] for q in qs), steps=sum(q["steps"] for q in qs), probes=sum(q["probes"] for q in qs),
                    capped=sum(q["capped"] for q in qs), rows=sum(q["rows"] for q in qs), records=sum(q["records"] for q in qs), raw=sum(raws), listed=sum(n > 0 for n in lens), entries=sum(lens),
                    max_markers=max(lens or [0]), chunks=chunks, by_wave=wave, by_sort=sum(r > 0 for r in raws) - wave)

    def check(self, got, min_len, max_rows, tun, tag):
        """got: what PfpContext.mk_query returned"""
        cnt, probes, markers, freqs, info = got
        qs = self.answers(min_len, max_rows)
        assert same(cnt, [q["cnt"] for q in qs]), (tag, "cnt")
        assert same(probes, [q["probes"] for q in qs]), (tag, "probes")
        assert len(markers) == len(freqs) == len(qs), tag
        for j, q in enumerate(qs):
            want_m = sorted(q["freq"])
            want_f = [q["freq"][X] for X in want_m]
            assert markers[j].dtype == np.uint64 and freqs[j].dtype == np.uint64, tag
            assert markers[j].tolist() == want_m, (tag, "markers of pattern", j, self.pats[j][:40], markers[j].tolist()[:8], want_m[:8])
            assert freqs[j].tolist() == want_f, (tag, "frequencies of pattern", j, self.pats[j][:40], freqs[j].tolist()[:8], want_f[:8])
        want = self.info(min_len, max_rows, tun)
        assert info == want, (tag, info, want)


def equal_results(a, b):
    return same(a[0], b[0]) and same(a[1], b[1]) and len(a[2]) == len(b[2]) and all(np.array_equal(x, y) for x, y in zip(a[2] + a[3], b[2] + b[3]))


def run_variants(ctx, exp, tag, variants=VARIANTS, modes=MODES):
    """every mode in every variant against brute force; the variants of a mode give equal arrays.  Returns the default variant's results"""
    out = {}
    for mode in modes:
        first = None
        for tun in variants:
            ctx.debug_set(**dict(DEFAULTS, **tun))
            got = ctx.mk_query(exp.pats, *mode)
            exp.check(got, mode[0], mode[1], tun, (tag, mode, tun))
            assert first is None or equal_results(first, got), (tag, mode, "variants differ", tun)
            first = first or got
        out[mode] = first
    ctx.debug_set(**DEFAULTS)
    return out


_cache = {}


def fixture_case(case):
    """(manifest, records, text, sa, {"golden": mps, "seeded": mps}, patterns)"""
    if case not in _cache:
        man, recs = golden_case(case)
        seqs = [s for _, s in recs]
        sa, _, mps, _ = marker_fixture(case)
        ref = oracle_run(seqs, w=man["w"], p=man["p"], U=8)
        text = bytes(ref["text"])
        assert same(ref["sa"], sa) and sa.size == len(text) + 1 <= 330331
        rng = np.random.default_rng(CASES.index(case) + 520)
        pats = text_patterns(rng, text, 68, 59) + [b"", b"#"]
        pats.insert(3, text[:1])                                           # one base: a fourth of the rows, every record on them
        _cache[case] = (man, seqs, text, sa, {"golden": mps, "seeded": seeded_mps(sa.size, 5)}, pats)
    return _cache[case]


def fixture_expected(case, stream):
    key = (case, stream)
    if key not in _cache:
        man, seqs, text, sa, streams, pats = fixture_case(case)
        _cache[key] = Expected(Model(text, sa, mps=streams[stream]), pats)
    return _cache[key]


def check_fixtures(factory):
    for case in CASES:
        man, seqs, text, sa, streams, pats = fixture_case(case)
        for U in (4, 8):
            results = []
            for fused in (True, False):
                ctx = build(factory, seqs, man["w"], man["p"], U, sa=fused, rssa=True)
                ctx.ri_index()
                for stream in ("seeded", "golden"):
                    exp = fixture_expected(case, stream)
                    if fused:
                        ma = ctx.marker_array(streams[stream])
                        assert np.array_equal(ma, exp.model.ma), (case, U, stream)
                        inf = ctx.mk_index()
                    else:
                        inf = ctx.mk_index(exp.model.ma)
                    assert inf == exp.model.index_info(), (case, U, stream, inf, exp.model.index_info())
                    results.append(run_variants(ctx, exp, (case, U, "fused" if fused else "host", stream), variants=VARIANTS if stream == "seeded" else VARIANTS[:1]))
                ctx.close()
            for a, b in zip(results[:2], results[2:]):                     # fused and host stream: equal arrays
                for mode in MODES:
                    assert equal_results(a[mode], b[mode]) and a[mode][4] == b[mode][4], (case, U, mode)


# ---- hand-made marker arrays ---------------------------------------------------------------------------------------------------
LIST_CLASSES = ["starts_on_border", "ends_on_border", "one_row_inside", "three_records", "no_record", "reaches_row_n"]
BIG = 1 << 63


def seeded_lists_case(ci, c):
    """(text, sa, patterns, .ma stream) or None when the oracle or the index would refuse the text.  The records are laid around the
    rows of one two-byte string; their lists hold what can go wrong: a repeated value, 1 / 64 / 65 / 257 markers, bit 63, two
    values that differ only above bit 32"""
    key = ("lists", ci)
    if key not in _cache:
        ref = oracle_run(c["seqs"], w=c["w"], p=c["p"], U=8)
        if ref.get("err") is not None or (np.asarray(ref["bwt"]) == 1).any():
            _cache[key] = None
            return None
        text, sa = bytes(ref["text"]), np.asarray(ref["sa"], np.uint64)
        n, isa = len(text), inverse_sa(sa)
        grams = sorted({text[a:a + L] for L in (1, 2, 3, 4) for a in range(n - L + 1)})
        rng = np.random.default_rng(70 + ci)
        span = lambda g: (lambda rows: (int(rows.min()), int(rows.max()) + 1))(isa[np.array([a for a in range(n - len(g) + 1) if text[a:a + len(g)] == g], np.int64)])
        fits = [g for g in grams if len(g) == 2 and span(g)[1] - span(g)[0] >= 12 and span(g)[0] >= 3 and span(g)[1] + 4 < n - 2]
        base = max(fits, key=lambda g: span(g)[1] - span(g)[0])         # the two-byte string with the most rows that leaves room around them
        lo, hi = span(base)
        pats = [bytes([b]) for b in sorted(set(text)) if b in b"ACGT"] + [base] + grams[:200] + text_patterns(rng, text, 40, 30) + [b"", b"#"]
        pats += [text[int(sa[r]):int(sa[r]) + 12] for r in (lo - 2, lo - 1, lo, lo + 1, lo + 5, hi - 2, hi, n - 1, n) if int(sa[r]) < n]      # single rows in and between the records
        many = lambda k, salt: [BIG + salt + 3 * q for q in range(k)]
        recs = [(lo - 2, lo - 1, [5, 5, 9, 5]),                             # ends in front of the interval; a repeated value
                (lo, lo, [7, 7 + (1 << 32), 7 + (1 << 40)]),                # starts with it; values that differ only above bit 32
                (lo + 1, lo + 2, many(64, 0)),                              # adjacent
                (lo + 3, lo + 4, many(65, 1)),
                (lo + 6, hi - 3, many(257, 2)),                             # one row free on either side of the neighbours
                (hi - 1, hi + 1, [BIG, 5, (1 << 64) - 2]),                  # across the interval's end
                (n - 1, n, [11])]                                           # one marker; ends at row n
        ma = mo.mps_build([r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs])
        _cache[key] = (text, sa, pats, ma)
    return _cache[key]


def list_classes(exp, modes):
    have = {c: 0 for c in LIST_CLASSES}
    m = exp.model
    for mode in modes:
        for q in exp.answers(*mode):
            for lo, hi, ka, kb in q["spans"]:
                have["starts_on_border"] += any(int(m.first[k]) == lo for k in range(ka, kb))
                have["ends_on_border"] += any(int(m.last[k]) == hi - 1 for k in range(ka, kb))
                have["one_row_inside"] += any(int(m.first[k]) == lo - 1 or int(m.last[k]) == hi for k in range(ka, kb))
                have["three_records"] += kb - ka >= 3
                have["no_record"] += kb == ka
                have["reaches_row_n"] += kb > ka and int(m.last[kb - 1]) == m.n and hi == m.n + 1
    return have


LIST_MODES = [(0, 0), (1, 0), (2, 3)]


def lists_cases():
    out = []
    for ci, c in enumerate(seeded_texts()):
        if len(out) < 2 and sum(len(s) for s in c["seqs"]) >= 300:
            got = seeded_lists_case(ci, c)
            if got is not None:
                out.append((ci, c, got))
    assert len(out) == 2
    return out


def check_lists(factory):
    have = {c: 0 for c in LIST_CLASSES}
    for ci, c, (text, sa, pats, ma) in lists_cases():
        exp = Expected(Model(text, sa, ma=ma), pats)
        for k, v in list_classes(exp, LIST_MODES).items():
            have[k] += v
        assert exp.model.index_info() == dict(records=7, entries=2 + 3 + 64 + 65 + 257 + 3 + 1, distinct=len({x for s in exp.model.sets for x in s}), max_list=257, rows=int((exp.model.last - exp.model.first + 1).sum()))
        for U in (4, 8):
            ctx = build(factory, c["seqs"], c["w"], c["p"], U, sa=False, rssa=True)
            ctx.ri_index()
            assert ctx.mk_index(ma) == exp.model.index_info(), (ci, U)
            run_variants(ctx, exp, ("lists", ci, U), modes=LIST_MODES)
            ctx.close()
    missing = [k for k, v in have.items() if not v]
    assert not missing, (missing, have)


def check_batch_shapes(factory):
    """0 patterns, only empty / absent patterns, 256 and 257 patterns, a chunk border on an empty pattern, one pattern larger than the
    budget, an empty index"""
    ci, c, (text, sa, pats, ma) = lists_cases()[1]
    model = Model(text, sa, ma=ma)
    rng = np.random.default_rng(12)
    pieces = [text[a:a + 5] for a in rng.integers(0, len(text) - 5, 257).tolist()]
    heavy = max(pats, key=lambda P: model.query(P, 0, 0)["raw"])
    light = sorted({P for P in pats if model.query(P, 0, 0)["raw"] > 0}, key=lambda P: (model.query(P, 0, 0)["raw"], P))[:2]      # the two with the fewest raw entries
    small = max(model.query(P, 0, 0)["raw"] for P in light)
    assert model.query(heavy, 0, 0)["raw"] > 300 and small <= 5 and len(light) == 2
    shapes = [[], [b"", b"#", b"", b"##"], pieces[:256], pieces, [light[0], b"", light[1], b"", b"", heavy], [light[0], heavy, light[1]]]
    ctx = build(factory, c["seqs"], c["w"], c["p"], 4, sa=False, rssa=True)
    ctx.ri_index()
    ctx.mk_index(ma)
    for q, ps in enumerate(shapes):
        exp = Expected(model, ps)
        tuns = [{}, {"mk_chunk_entries": 1}] if q < 4 else [{}, {"mk_chunk_entries": small}, {"mk_chunk_entries": 64}, {"mk_chunk_entries": 2, "mk_wave_max": 0}]
        run_variants(ctx, exp, ("shape", q), variants=tuns, modes=[(0, 0), (2, 0)])
    got = ctx.mk_query([])
    assert got[0].size == 0 and got[2] == [] and got[4]["chunks"] == 0 and got[4]["entries"] == 0
    assert Expected(model, shapes[5]).info(0, 0, {"mk_chunk_entries": small})["chunks"] == 3
    # an empty index: every count as before, no pairs
    empty = Model(text, sa, ma=np.zeros(0, np.uint64))
    assert ctx.mk_index(np.zeros(0, np.uint64)) == dict(records=0, entries=0, distinct=0, max_list=0, rows=0)
    exp = Expected(empty, pats[:60])
    got = run_variants(ctx, exp, "empty index", variants=VARIANTS[:2], modes=[(0, 0), (1, 0)])
    assert got[(1, 0)][4]["entries"] == 0 and got[(1, 0)][4]["probes"] > 0 and same(got[(0, 0)][0], ctx.ri_count(exp.pats)[0])
    ctx.close()


def check_state_and_errors(factory):
    E_STATE, E_ARG, E_NOMEM, E_TOO_LARGE, E_CORRUPT = pfbwt_hip.E_STATE, pfbwt_hip.E_ARG, pfbwt_hip.E_NOMEM, pfbwt_hip.E_TOO_LARGE, pfbwt_hip.E_CORRUPT
    case = "single_chrom"
    man, seqs, text, sa, streams, allpats = fixture_case(case)
    w, p = man["w"], man["p"]
    full = fixture_expected(case, "seeded")
    small, other = Expected(full.model, allpats[:30]), Expected(full.model, allpats[30:45])
    pats, ma, n = small.pats, full.model.ma, len(text)
    C = pfbwt_hip.C
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    buf = np.empty(1 << 16, np.uint64)
    bases = np.frombuffer(b"ACGTACGT", np.uint8)
    off = np.array([0, 4], np.uint64)

    def status(f, *a, **kw):
        with pytest.raises(pfbwt_hip.PfpError) as e:
            f(*a, **kw)
        return e.value.status

    def nothing_made(ctx):
        L = ctx.L
        return (L.pfp_mk_get(ctx.h, vp(buf), None, None, None) == E_STATE and L.pfp_mk_get(ctx.h, None, None, None, None) == E_STATE and L.pfp_mk_write(ctx.h, -1, -1, -1, -1, -1) == E_STATE
                and L.pfp_mk_offsets_get(ctx.h, vp(buf), None) == E_STATE and ctx.mk_device_ptrs() == [None] * 4)

    def raw(ctx, b=bases, o=off, np_=1):
        return ctx.L.pfp_mk_query(ctx.h, None if b is None else vp(b), None if o is None else vp(o), np_, 0, 0, None)

    ctx = factory(w=w, p=p, u64=True, sai=True)
    L = ctx.L
    assert L.pfp_mk_index(None, None, 0, None) == E_ARG and L.pfp_mk_query(None, vp(bases), vp(off), 1, 0, 0, None) == E_ARG and L.pfp_mk_get(None, None, None, None, None) == E_ARG
    assert L.pfp_mk_write(None, -1, -1, -1, -1, -1) == E_ARG and L.pfp_mk_offsets_get(None, None, None) == E_ARG and L.pfp_mk_device_ptrs(None, None, None, None, None) == E_ARG
    assert L.pfp_mk_query_file(None, b"x", 0, 0, None) == E_ARG
    assert status(ctx.mk_index, ma) == E_STATE and raw(ctx) == E_STATE and nothing_made(ctx)               # no build at all
    for s in seqs:
        ctx.feed(s, True)
    ctx.finalize(); ctx.parse_bwt(); ctx.bwt_build(sa=True, rssa=True)
    assert status(ctx.mk_index) == E_STATE                                                                 # ma=None without a marker array
    assert L.pfp_mk_index(ctx.h, None, 5, None) == E_ARG                                                   # NULL with words
    assert ctx.marker_array(np.zeros(0, np.uint64)).size == 0 and status(ctx.mk_index) == E_STATE          # an empty one is none
    assert np.array_equal(ctx.marker_array(streams["seeded"]), ma)
    assert L.pfp_mk_index(ctx.h, None, 0, None) == 0                                                       # info is nullable
    assert status(ctx.mk_query, pats) == E_STATE and nothing_made(ctx)                                    # no pfp_ri_index
    assert L.pfp_mk_query_file(ctx.h, b"/nonexistent", 0, 0, None) == E_STATE
    ctx.ri_index()
    assert nothing_made(ctx)
    assert L.pfp_mk_query_file(ctx.h, b"/nonexistent", 0, 0, None) == -9 and L.pfp_mk_query_file(ctx.h, None, 0, 0, None) == E_ARG      # PFP_E_IO
    before = ctx.bwt_get()
    # a stream that is no marker array: one per class; the index is gone after each, everything else as it was
    rec = lambda f, l, ms: [f, l] + list(ms) + [DELIM]
    corrupt = {"no delimiter at the end": rec(3, 5, [7]) + [9, 12, 8], "no delimiter behind two markers": rec(3, 5, [7]) + [9, 12, 8, 8], "no delimiter at all": [3, 5, 7], "cut inside the keys": rec(3, 5, [7]) + [9], "no marker": rec(3, 5, [7]) + rec(9, 12, []), "an empty record": rec(3, 5, [7]) + [DELIM],
               "first > last": rec(6, 5, [7]), "last > n": rec(3, n + 1, [7]), "first == previous last": rec(3, 5, [7]) + rec(5, 8, [7]), "out of order": rec(30, 50, [7]) + rec(9, 12, [8])}
    for why, words in corrupt.items():
        ctx.mk_index(ma)
        assert status(ctx.mk_index, np.array(words, np.uint64)) == E_CORRUPT, why
        assert status(ctx.mk_query, pats) == E_STATE, why                                                  # a failing call leaves no marker index
    assert ctx.mk_index(np.array(rec(0, 0, [1]) + rec(n, n, [1, 1]), np.uint64)) == dict(records=2, entries=2, distinct=1, max_list=1, rows=2)      # the limits themselves
    assert np.array_equal(ctx.marker_array(streams["seeded"]), ma)                                        # (and the marker array still works)
    assert ctx.mk_index() == full.model.index_info()
    # arguments
    assert raw(ctx, b=None) == E_ARG and raw(ctx, o=None) == E_ARG and nothing_made(ctx)
    assert status(ctx.mk_query_flat, bases, [0, 5, 3]) == E_ARG and status(ctx.mk_query, [b"ACG", b"AC\x00T"]) == E_ARG      # descending offsets, a 0 byte
    assert raw(ctx, np_=1 << 32) == E_TOO_LARGE and nothing_made(ctx)
    assert raw(ctx) == 0                                                                                  # info is nullable
    n1 = C.c_uint64(7)
    assert L.pfp_mk_offsets_get(ctx.h, None, C.byref(n1)) == 0 and n1.value == 1
    a = ctx.mk_query_flat(bases, [2, 6, 8])                                                                # offsets need not start at 0
    b = ctx.mk_query([b"GTAC", b"GT"])
    assert same(a[0], b[0]) and same(a[3], np.concatenate(b[2])) and same(a[4], np.concatenate(b[3])) and a[5] == b[4]
    # the results: slots of their own, beside everything else
    first = ctx.mk_query(pats, 8, 4)
    small.check(first, 8, 4, {}, "state")
    d = ctx.mk_device_ptrs()
    assert all(d[:2]) and len(set(d)) == 4
    flat = ctx.mk_query_flat(*ctx._flat_patterns(pats), 8, 4)
    cnt_exp = ctx.ri_count(pats)[0]
    assert same(flat[0], cnt_exp)                                                                         # cnt is pfp_ri_count's whatever min_len and max_rows say
    starts = pfbwt_hip.doc_starts([len(s) for s in seqs], w)

    def still_there(tag):
        cnt, probes, moff = np.empty(len(pats), np.uint64), np.empty(len(pats), np.uint64), np.empty(len(pats) + 1, np.uint64)
        marker, freq = np.empty(flat[3].size, np.uint64), np.empty(flat[4].size, np.uint64)
        assert L.pfp_mk_get(ctx.h, vp(cnt), vp(probes), vp(marker), vp(freq)) == 0 and L.pfp_mk_offsets_get(ctx.h, vp(moff), None) == 0, tag
        assert same(cnt, flat[0]) and same(probes, flat[1]) and same(moff, flat[2]) and same(marker, flat[3]) and same(freq, flat[4]), tag

    still_there("at once")
    ctx.thresholds(); ctx.ms_index(); ctx.ri_index(); ctx.lcp_array(); ctx.doc_array(starts); ctx.ms_query(pats); ctx.mem_find(1, locate=True); ctx.ri_docs(other.pats, starts); ctx.marker_array(streams["golden"])
    still_there("after the other passes")
    ctx.marker_array(streams["seeded"]); ctx.ri_docs(pats[:3], starts); ctx.mem_find(2); ctx.ms_query(pats[:3]); ctx.doc_array(starts); ctx.lcp_array(); ctx.ri_index(); ctx.ms_index(); ctx.thresholds()
    still_there("after the other passes, other order")
    ctx.ri_count(other.pats); still_there("after a count")
    ctx.ri_locate(other.pats); still_there("after a locate")
    ctx.mk_index(); still_there("after a second marker index")
    assert ctx.mk_device_ptrs() == d
    other.check(ctx.mk_query(other.pats, 1, 50), 1, 50, {}, "a second call replaces the first")
    n1 = C.c_uint64(0)
    assert L.pfp_mk_offsets_get(ctx.h, None, C.byref(n1)) == 0 and n1.value == len(other.pats)
    ctx.marker_array(streams["golden"])                                                                   # the index is its own copy
    small.check(ctx.mk_query(pats), 0, 0, {}, "after another marker array")
    after = ctx.bwt_get()                                                                                 # the published build is unchanged
    for k in ("bwt", "sa", "ssa", "esa"):
        assert np.array_equal(before[k], after[k]), k
    # a new build drops index and results
    ctx.bwt_build(sa=False, rssa=True)
    assert nothing_made(ctx) and status(ctx.mk_query, pats) == E_STATE and status(ctx.mk_index) == E_STATE
    ctx.ri_index()
    assert status(ctx.mk_query, pats) == E_STATE
    ctx.mk_index(ma)
    small.check(ctx.mk_query(pats, 8, 0), 8, 0, {}, "rssa only")
    ctx.bwt_build_slice(0, 2, sa=True, rssa=True)                                                         # a slice
    assert status(ctx.mk_index, ma) == E_STATE and status(ctx.mk_query, pats) == E_STATE
    ctx.close()
    # a context filled by pfp_bwt_load answers the same arrays from the host stream
    ref = oracle_run(seqs, w=w, p=p, U=8)
    ctx = factory(w=w, p=p, u64=True, sai=True)
    ctx.bwt_load(ref["dict"], ref["occ"], ref["bwlast"], ref["ilist"], ref["bwsai"], n_hint=ref["n"])
    ctx.bwt_build(sa=False, rssa=True)
    ctx.ri_index()
    assert ctx.mk_index(ma) == full.model.index_info()
    for mode in MODES:
        small.check(ctx.mk_query(pats, *mode), mode[0], mode[1], {}, ("loaded", mode))
    ctx.close()
    # PFP_E_NOMEM from a small workspace leaves a following call with max_rows working
    ctx = None
    for mib in (24, 32, 48, 64, 96):
        try:
            ctx = build(lambda **kw: factory(workspace_bytes=mib << 20, **kw), seqs, w, p, 8, sa=False, rssa=True)
            ctx.ri_index()
            ctx.mk_index(ma)
            break
        except pfbwt_hip.PfpError as e:
            assert e.status == E_NOMEM
            ctx = None
    assert ctx is not None
    L = ctx.L
    singles = [text[a:a + 1] for a in range(4)]
    loc = ctx.ri_locate(pats)
    assert status(ctx.mk_query, singles * 30000) == E_NOMEM and nothing_made(ctx)                         # (16 bytes per slot of the upper bound: distinct markers per pattern)
    assert L.pfp_workspace_needed(ctx.h) > (mib << 20)
    cnt_now, pos_now = np.empty(len(pats), np.uint64), np.empty(int(loc[1].sum()), np.uint64)
    assert L.pfp_ri_get(ctx.h, vp(cnt_now), vp(pos_now)) == 0 and same(cnt_now, loc[1]) and same(pos_now, np.concatenate(loc[0]))      # every other result as it was
    cnt, probes, markers, freqs, info = ctx.mk_query(singles * 30000, 0, 1000)
    assert info["capped"] == 120000 and info["entries"] == 0 and info["probes"] == 0 and all(x.size == 0 for x in markers)
    for q, S in enumerate(singles):
        assert same(cnt[q::4], np.full(30000, text.count(normalise(S, False))))
    small.check(ctx.mk_query(pats, 8, 4), 8, 4, {}, "after NOMEM")
    ctx.debug_set(mk_wave_max=1000, mk_chunk_entries=-5)                                                  # values out of range are clamped
    small.check(ctx.mk_query(pats), 0, 0, {}, "clamped")
    ctx.debug_set(mk_wave_max=-3)
    small.check(ctx.mk_query(pats), 0, 0, {}, "clamped")
    with pytest.raises(pfbwt_hip.PfpError):
        ctx.debug_set(mk_wave=3)
    ctx.close()


# ---- command line ------------------------------------------------------------------------------------------------------------
def check_cli(exe, factory, tmp):
    """exe: {'pfbwt-f': path, 'pfbwt-f64': path}"""
    case = "mult_chroms"
    man, seqs, text, sa, streams, allpats = fixture_case(case)
    exp = Expected(fixture_expected(case, "seeded").model, [p for p in allpats[:50] if p])
    reads, ma = exp.pats, exp.model.ma
    fa = os.path.join(tmp, "input.fa")
    with open(fa, "wb") as f:
        for j, s in enumerate(seqs):
            f.write(b">s%d\n" % j + s + b"\n")
    wp = ["-w", str(man["w"]), "-p", str(man["p"])]
    fasta, fastq, mpsf, maf = os.path.join(tmp, "reads.fa"), os.path.join(tmp, "reads.fq"), os.path.join(tmp, "in.mps"), os.path.join(tmp, "in.ma")
    with open(fasta, "wb") as f:
        for j, r in enumerate(reads):
            f.write(b">r%d some words\n" % j + b"\n".join(r[k:k + 60] for k in range(0, len(r), 60)) + b"\n")
    with open(fastq, "wb") as f:
        for j, r in enumerate(reads):
            f.write(b"@r%d\n" % j + r + b"\n+\n" + b"@" * len(r) + b"\n")
    streams["seeded"].astype("<u8").tofile(mpsf); ma.astype("<u8").tofile(maf)
    EXT = ("mk.cnt", "mk.probes", "mk.off", "mk.marker", "mk.freq")

    def files(pref):
        return {e: open(pref + "." + e, "rb").read() for e in ("bwt", "sa", "ssa", "esa", "cnt", "dict", "occ", "parse", "bwlast", "ilist", "bwsai", "n") if os.path.exists(pref + "." + e)}

    def same_files(pref, f, U):
        assert same(read_u(pref + ".mk.cnt", U), f[0]) and same(read_u(pref + ".mk.probes", U), f[1]) and same(read_u(pref + ".mk.marker", 8), f[3]) and same(read_u(pref + ".mk.freq", 8), f[4]), pref
        assert same(read_u(pref + ".mk.off", 8), f[2]) and os.path.getsize(pref + ".mk.off") == 8 * (len(reads) + 1) and os.path.getsize(pref + ".mk.marker") == 8 * f[3].size, pref

    for name, U in (("pfbwt-f64", 8), ("pfbwt-f", 4)):
        ctx = build(factory, seqs, man["w"], man["p"], U, sa=False, rssa=True)
        ctx.ri_index(); ctx.mk_index(ma)
        bases, off = ctx._flat_patterns(reads)
        whole, sub = ctx.mk_query_flat(bases, off), ctx.mk_query_flat(bases, off, 8, 4)
        exp.check(ctx.mk_query(reads, 8, 4), 8, 4, {}, name)
        ctx.close()
        # --mps: FASTA reads with -r alone on one program, FASTQ reads beside -s --count on the other; every other file: byte-identical
        rd, extra = (fasta, ["-r"]) if U == 8 else (fastq, ["-r", "-s", "--count", fasta])
        pref, plain = os.path.join(tmp, "mk_%d" % U), os.path.join(tmp, "plain_%d" % U)
        pr = run([exe[name]] + extra + wp + ["--mps", mpsf, "--markers", rd, "-o", pref, fa])
        assert "TASK\tmarkers\t" in pr.stderr and "markers: %d reads, %d found, %d probes, %d capped, %d listed, %d pairs" % (len(reads), whole[5]["found"], whole[5]["probes"], whole[5]["capped"], whole[5]["listed"], whole[5]["entries"]) in pr.stderr
        assert np.array_equal(np.fromfile(pref + ".ma", "<u8"), ma), name                                 # the oracle's stream
        same_files(pref, whole, U)
        run([exe[name]] + extra + wp + ["-o", plain, fa])
        a, b = files(pref), files(plain)
        assert a == b and "bwt" in a and "ssa" in a and ("sa" in a) == (U == 4) and not any(os.path.exists(plain + "." + e) for e in EXT + ("ma",)), (name, sorted(a), sorted(b))
        # --ma with -r alone, the sub-options
        pref = os.path.join(tmp, "ma_%d" % U)
        pr = run([exe[name], "-r", "--ma", maf, "--markers", fastq if U == 8 else fasta, "--markers-min-len", "8", "--markers-max-rows", "4"] + wp + ["-o", pref, fa])
        same_files(pref, sub, U)
        assert "%d capped" % sub[5]["capped"] in pr.stderr and sub[5]["capped"] > 0 and not os.path.exists(pref + ".ma") and not os.path.exists(pref + ".sa")
        if U == 8:                                                                                        # --mps alone writes the array; --pfbwt-only with --ma
            pref = os.path.join(tmp, "only_mps")
            run([exe[name], "--mps", mpsf] + wp + ["-o", pref, fa])
            assert np.array_equal(np.fromfile(pref + ".ma", "<u8"), ma) and not os.path.exists(pref + ".sa") and not os.path.exists(pref + ".mk.cnt")
            pref = os.path.join(tmp, "two_steps")
            run([exe[name], "--parse-only", "-r"] + wp + ["-o", pref, fa])
            run([exe[name], "--pfbwt-only", "-r", "--ma", maf, "--markers", fasta] + wp + ["-o", pref])
            same_files(pref, whole, U)
    efa = os.path.join(GOLDEN, "edge", "input.fa")

    def refused(args, opt, word, prefix):
        pr = run([exe["pfbwt-f64"]] + args + ["-w", "10", "-p", "20", "-o", prefix, efa], check=False)
        assert pr.returncode != 0 and opt in pr.stderr and word in pr.stderr.split("Command line")[-1].split("\n", 1)[1], pr.stderr[-500:]
        for e in ("bwt", "dict", "ma") + EXT:
            assert not os.path.exists(prefix + "." + e), (args, e)

    refused(["--markers", fasta, "--ma", maf], "--markers", "-r", os.path.join(tmp, "no_r"))
    refused(["--markers", fasta, "--ma", maf, "-r", "--gpus", "2"], "--markers", "--gpus", os.path.join(tmp, "gpus"))
    refused(["--markers", fasta, "--ma", maf, "-r", "--parse-only"], "--markers", "--parse-only", os.path.join(tmp, "parse_only"))
    refused(["--markers", fasta, "-r"], "--markers", "--mps", os.path.join(tmp, "no_array"))
    refused(["--markers", fasta, "-r", "--mps", mpsf, "--ma", maf], "--mps", "--ma", os.path.join(tmp, "both"))
    refused(["--markers-min-len", "3", "-r"], "--markers-min-len", "--markers ", os.path.join(tmp, "no_markers"))
    refused(["--markers-max-rows", "3", "-r"], "--markers-max-rows", "--markers ", os.path.join(tmp, "no_markers2"))
    h = run([exe["pfbwt-f"], "-h"]).stderr
    assert "--mps <file>" in h and "--ma <file>" in h and "--markers <reads>" in h and "--markers-min-len <L>" in h and "--markers-max-rows <K>" in h


def test_checkers_agree():
    """the text-space brute force against the row-space definition on both marker fixtures and both streams, without any engine; the
    classes the kernels branch on occur; the checker refuses a dropped pair, a swapped pair and a frequency off by one"""
    assert [f for f, _ in pfbwt_hip.MkInfo._fields_] == INFO_KEYS and [f for f, _ in pfbwt_hip.MkIndexInfo._fields_] == INDEX_KEYS
    for case in CASES:
        for stream in ("golden", "seeded"):
            exp = fixture_expected(case, stream)
            assert exp.model.text_space and exp.model.index_info()["records"] > 0
            for mode in MODES + [(1, 0)]:
                for q in exp.answers(*mode):
                    assert q["freq"] == q["rfreq"], (case, stream, mode)
                    assert all(f >= 1 for f in q["freq"].values()) and q["probes"] == len(q["spans"])
        exp = fixture_expected(case, "seeded")
        for mode in ((0, 0), (8, 0)):                                       # both reductions
            i = exp.info(mode[0], mode[1], {})
            assert i["by_wave"] > 0 and i["by_sort"] > 0, (case, mode, i)
        for mode in ((8, 4), (1, 50)):
            assert exp.info(mode[0], mode[1], {})["capped"] > 0, (case, mode)
        assert exp.info(8, 0, {"mk_chunk_entries": 7})["chunks"] > 10 and exp.info(0, 0, {"mk_wave_max": 0})["by_wave"] == 0
        cnts = [q["cnt"] for q in exp.answers(0, 0)]
        assert cnts == [q["cnt"] for q in exp.answers(8, 4)] and max(cnts) > 1000 and 0 in cnts
    for ci, c, (text, sa, pats, ma) in lists_cases():                      # the hand-made arrays: by row
        exp = Expected(Model(text, sa, ma=ma), pats)
        for mode in LIST_MODES:
            for q in exp.answers(*mode):
                assert q["freq"] == q["rfreq"], (ci, mode)
    # the checker refuses wrong answers
    exp = fixture_expected("single_chrom", "seeded")
    qs = exp.answers(8, 0)
    good = (np.array([q["cnt"] for q in qs], np.uint64), np.array([q["probes"] for q in qs], np.uint64), [np.array(sorted(q["freq"]), np.uint64) for q in qs],
            [np.array([q["freq"][X] for X in sorted(q["freq"])], np.uint64) for q in qs], exp.info(8, 0, {}))
    exp.check(good, 8, 0, {}, "good")
    j = max(range(len(qs)), key=lambda k: len(qs[k]["freq"]))
    assert len(qs[j]["freq"]) >= 2
    for what in ("dropped", "swapped", "off_by_one"):
        ms, fs = list(good[2]), list(good[3])
        if what == "dropped":
            ms[j], fs[j] = ms[j][1:], fs[j][1:]
        elif what == "swapped":
            ms[j] = np.concatenate([ms[j][1:2], ms[j][0:1], ms[j][2:]])
        else:
            fs[j] = np.concatenate([fs[j][:1] + np.uint64(1), fs[j][1:]])
        with pytest.raises(AssertionError):
            exp.check((good[0], good[1], ms, fs, good[4]), 8, 0, {}, what)


# ---- CPU: the emulated library -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pfbwt-f_amd"), "emu", "emu-host"], check=True, stdout=subprocess.DEVNULL)
    return lambda **kw: pfbwt_hip.PfpContext(lib=EMU_SO, **kw)


def test_markerquery_fixtures_emu(emu):
    check_fixtures(emu)


def test_markerquery_lists_emu(emu):
    check_lists(emu)


def test_markerquery_batch_shapes_emu(emu):
    check_batch_shapes(emu)


def test_markerquery_state_and_errors_emu(emu):
    check_state_and_errors(emu)


def test_markerquery_cli_emu(emu, tmp_path):
    check_cli({"pfbwt-f": os.path.join(EMUB, "pfbwt-f-emu"), "pfbwt-f64": os.path.join(EMUB, "pfbwt-f64-emu")}, emu, str(tmp_path))


# ---- GPU: the product library --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_markerquery_fixtures_gpu(gpu_ctx_factory):
    check_fixtures(gpu_ctx_factory)


@pytest.mark.gpu
def test_markerquery_lists_gpu(gpu_ctx_factory):
    check_lists(gpu_ctx_factory)


@pytest.mark.gpu
def test_markerquery_batch_shapes_gpu(gpu_ctx_factory):
    check_batch_shapes(gpu_ctx_factory)


@pytest.mark.gpu
def test_markerquery_state_and_errors_gpu(gpu_ctx_factory):
    check_state_and_errors(gpu_ctx_factory)


@pytest.mark.gpu
def test_markerquery_cli_gpu(gpu_ctx_factory, tmp_path):
    check_cli({"pfbwt-f": os.path.join(BIN, "pfbwt-f"), "pfbwt-f64": os.path.join(BIN, "pfbwt-f64")}, gpu_ctx_factory, str(tmp_path))
