"""Maximal exact matches on the device (include/pfbwt_hip.h: pfp_mem_find; csrc/mems.h; pfbwt-f --mems / --mems-locate / --mems-max).

The expected values never come from the engine.  From the pinned oracle (text, bwt, sa, ssa, esa) there are:
* brute force, by the definition and independent of any matching statistic: for every pattern all (i, l) with P[i:i+l] in the text
  (bytes.find) that cannot be extended to the left or to the right (bytes.find again) -- the set of (pattern, start, len); min_len
  only filters that set;
* the models: ptr must be test_matchstats.Model.pointers at the MEM's first base, cnt / pos must be test_runindex.brute_locate of
  the MEM's bytes, and pieces / max_piece / phi_steps of info on the phi route come from test_runindex.Model.locate.
test_checkers_agree shows, without any engine, brute force == the rule of the header over test_matchstats.brute_ms on every fixture
and seeded case, that every class of CLASSES occurs, and that the checker refuses a MEM that is dropped, shifted or shortened.
Brute force costs one text scan per (start, length) pair that occurs, so the patterns are short: up to 120 bases on texts of up to
SMALL_ROWS rows, up to 32 bases on the larger fixtures.  On the emulated library panel8 (100 s per build there) runs with U = 8 on
one build with the SA; on the card it runs like the others."""
import os
import subprocess
import numpy as np
import pytest
from pfp_testlib import EMU_SO, GOLDEN, ROOT
from test_thresholds import build, fixture_expected, lcp_numpy, read_u, run, same, thresholds_brute
from test_matchstats import FIXTURES, SMALL_ROWS, Model as MsModel, brute_ms, fixture_case as ms_fixture_case, mutated, normalise, window_for
from test_runindex import Model as RiModel, brute_locate, capped, fixture_case as ri_fixture_case, seeded_case, seeded_texts, text_patterns

import pfbwt_hip

EMUB = os.path.join(ROOT, "tests", "emu", "build")
BIN = os.path.join(ROOT, "pfbwt-f_amd", "bin")
DEFAULTS = {"ri_dir_log2": -1, "ms_dir_log2": -1, "ri_route": 0}
INFO_KEYS = ["patterns", "bases", "mems", "max_len", "sum_len", "occurrences", "reported", "pieces", "max_count", "max_piece", "phi_steps", "route"]
BLOCK = 256                  # lanes per workgroup of the kernels (csrc/common.h)
SCAN_TILE = BLOCK * 16       # bases per tile of the flag sum (csrc/prims.h)
MAX_COUNT = 3000             # a MEM that occurs more often is not asked for (brute force sorts its occurrences)
CLASSES = ["no_mem_absent_byte", "no_mem_below_min", "one_base", "empty_between", "whole_pattern", "border", "border_len0", "several_mems", "len_eq_min", "len_below_min",
           "text_suffix", "pads", "count_one", "count_three", "three_runs"]


# ---- the checkers ------------------------------------------------------------------------------------------------------------
def brute_mems(text, P):
    """all (i, l), l >= 1, that satisfy the definition: P[i:i+l] occurs, P[i-1:i+l] and P[i:i+l+1] do not (or do not exist)"""
    m, out, known = len(P), [], {}

    def occurs(a, b):
        if (a, b) not in known:
            known[(a, b)] = text.find(P[a:b]) >= 0
        return known[(a, b)]

    for i in range(m):
        l = 1
        while i + l <= m and occurs(i, i + l):                  # (a string that does not occur has no extension that does)
            if (i == 0 or not occurs(i - 1, i + l)) and (i + l == m or not occurs(i, i + l + 1)):
                out.append((i, l))
            l += 1
    return out


def rule_mems(ln, min_len):
    """the rule of the header over the lengths of ONE pattern"""
    L = max(min_len, 1)
    return [(i, int(ln[i])) for i in range(len(ln)) if ln[i] >= L and (i == 0 or ln[i - 1] <= ln[i])]


class Expected:
    """the patterns of one build and what the checkers say about their MEMs"""

    def __init__(self, ms_model, ri_model, isa, pats, non_acgt_to_a, pads):
        self.ms, self.ri, self.isa, self.pads = ms_model, ri_model, isa, pads
        self.text = ri_model.text
        self.pats = [bytes(p) for p in pats]
        self.norm = [normalise(p, non_acgt_to_a) for p in self.pats]
        self.bases = sum(len(p) for p in self.pats)
        self.all = [brute_mems(self.text, P) for P in self.norm]          # min_len = 1
        self.ptr = [ms_model.pointers(P)[0] for P in self.norm]
        self._loc, self._search = {}, {}
        for j, ms in enumerate(self.all):                                 # by ascending start, and their ends ascend too
            assert all(a[0] < b[0] and a[0] + a[1] < b[0] + b[1] for a, b in zip(ms, ms[1:])), j
        self.lens = sorted({l for ms in self.all for _, l in ms})
        self.max_len = self.lens[-1] if self.lens else 0

    def mems(self, min_len):
        L = max(min_len, 1)
        return [[(i, l) for i, l in ms if l >= L] for ms in self.all]

    def string(self, j, i, l):
        return self.norm[j][i:i + l]

    def located(self, S, max_occ):
        if (S, max_occ) not in self._loc:
            self._loc[(S, max_occ)] = brute_locate(self.text, self.isa, S, max_occ)
        return self._loc[(S, max_occ)]

    def pieces(self, S, max_occ):
        if S not in self._search:
            self._search[S] = self.ri.search(S)
        lo, cnt, top, why = self._search[S]
        assert why is None
        return self.ri.locate(lo, cnt, top, max_occ)[1]

    def count(self, S):
        return self.located(S, 1)[0]

    def min_lens(self):
        """min_len values of the issue: 1, an L* that occurs (one with L* - 1 occurring too where there is one), L* + 1, max_len + 1"""
        both = [l for l in self.lens if l >= 2 and l - 1 in self.lens]
        star = both[0] if both else (self.lens[0] if self.lens else 1)
        return sorted({1, star, star + 1, self.max_len + 1}), star

    def info(self, min_len, route, max_occ=0):
        ms = self.mems(min_len)
        flat = [self.string(j, i, l) for j in range(len(ms)) for i, l in ms[j]]
        want = dict(patterns=len(self.pats), bases=self.bases, mems=len(flat), max_len=max([len(s) for s in flat] or [0]), sum_len=sum(len(s) for s in flat),
                    occurrences=0, reported=0, pieces=0, max_count=0, max_piece=0, phi_steps=0, route=route)
        if route:
            loc = [self.located(s, max_occ) for s in flat]
            want.update(occurrences=sum(c for c, _ in loc), reported=sum(len(p) for _, p in loc), max_count=max([c for c, _ in loc] or [0]))
            pcs = [self.pieces(s, max_occ) for s in flat]
            want.update(pieces=sum(p[0] for p in pcs))
            if route == 1:
                want.update(max_piece=max([p[1] for p in pcs] or [0]), phi_steps=sum(p[2] for p in pcs))
        return want

    def check(self, got, min_len, route, max_occ, tag):
        """got: what PfpContext.mem_find returned (route 0: without locate)"""
        start, ln, ptr = got[0], got[1], got[2]
        want, n = self.mems(min_len), len(self.text)
        assert len(start) == len(ln) == len(ptr) == len(self.pats), tag
        k = 0
        for j, P in enumerate(self.norm):
            have = list(zip(start[j].tolist(), ln[j].tolist()))
            assert have == want[j], (tag, "MEMs of pattern", j, self.pats[j][:40], have, want[j])
            for q, (i, l) in enumerate(want[j]):
                p = int(ptr[j][q])
                assert p == self.ptr[j][i], (tag, "ptr", j, i)
                assert p + l <= n and self.text[p:p + l] == P[i:i + l], (tag, "text at ptr", j, i)
                if route:
                    c, pos = self.located(P[i:i + l], max_occ)
                    assert int(got[3][j][q]) == c and c >= 1, (tag, "cnt", j, i, int(got[3][j][q]), c)
                    assert got[4][k].tolist() == pos, (tag, "pos", j, i, max_occ)
                    assert max_occ or p in pos, (tag, "ptr is an occurrence", j, i)
                k += 1
        if route:
            assert len(got[3]) == len(self.pats) and len(got[4]) == k, tag
        assert got[-1] == self.info(min_len, route, max_occ), (tag, got[-1], self.info(min_len, route, max_occ))

    def classes(self, min_len, star):
        """how many patterns / MEMs fall into every class (min_len: a value > 1 of min_lens())"""
        have = {c: 0 for c in CLASSES}
        n, t = len(self.text), self.text
        cut = self.mems(min_len)
        for j, P in enumerate(self.norm):
            ms = self.all[j]
            have["no_mem_absent_byte"] += bool(P) and not ms and all(c not in self.ri.runs_of for c in P)
            have["no_mem_below_min"] += bool(ms) and not cut[j]
            have["one_base"] += len(P) == 1
            have["empty_between"] += not P and 0 < j < len(self.norm) - 1 and bool(self.norm[j - 1]) and bool(self.norm[j + 1])
            have["whole_pattern"] += ms == [(0, len(P))] and bool(P)
            prev = self.norm[j - 1] if j else b""
            if prev and ms and ms[0][0] == 0:                               # behind a pattern whose last base has len 1 / 0
                have["border"] += prev[-1] in self.ri.runs_of
                have["border_len0"] += prev[-1] not in self.ri.runs_of
            have["several_mems"] += len(ms) >= 2
            for i, l in ms:
                S = P[i:i + l]
                have["len_eq_min"] += l == star
                have["len_below_min"] += l == star - 1
                have["text_suffix"] += S == t[n - l:]
                have["pads"] += S == b"A" * l and any(a <= p and p + l <= b for p in self.located(S, 0)[1] for a, b in self.pads)
                c = self.count(S)
                have["count_one"] += c == 1
                have["count_three"] += c >= 3
                if S not in self._search:
                    self._search[S] = self.ri.search(S)
                lo, cnt, top, _ = self._search[S]
                have["three_runs"] += self.ri.run_of(lo + cnt - 1) - self.ri.run_of(lo) >= 2
        return have


def make_patterns(rng, ri_model, w, pads):
    """patterns for one text: record pieces with 0 .. 3 substitutions, and one or more for every class of CLASSES by name"""
    t, n = ri_model.text, ri_model.n
    small = n + 1 <= SMALL_ROWS
    pats = text_patterns(rng, t, 36 if small else 8, 120 if small else 32)
    pats += [mutated(rng, p, 2) for p in text_patterns(rng, t, 12 if small else 4, 120 if small else 32)]
    a = n // 3
    pats.insert(3, b"")                                                  # an empty pattern between two others
    pats += [b"X", b"XX"]                                                # no MEM: bytes that head no run
    pats += [t[n // 2:n // 2 + 1], b"", t[a:a + 1]]                      # one base
    pats += [t[a:a + 25], t[a + 7:a + 30].lower()]                       # the whole pattern (the second one behind a last base of len 1: the border)
    pats += [t[a:a + 9] + b"X", t[a + 40:a + 52]]                        # ... behind a last base of len 0
    pats += [t[n - min(n, 30):], b"X" + t[n - min(n, 9):]]               # a text suffix
    pats += [b"X" + b"A" * w + b"X", b"X" + b"A" * (w - 1) + b"X"]       # pad 'A's, maximal between bytes that do not occur
    if pads:
        e0 = pads[0][0]
        pats.append(t[max(e0 - 8, 0):e0 + w + 8])                        # across a record border
    for L in (1, 2, 3, 4, 6, 9, 12):                                     # short strings between bytes that do not occur: many occurrences
        for b in rng.integers(0, n - L + 1, 3).tolist():
            S = t[b:b + L]
            if 0 < len(S) and t.count(S) <= MAX_COUNT:
                pats.append(b"X" + S + b"X")
    return pats


def usable(text, pats, non_acgt_to_a):
    """drops the patterns with a MEM that occurs more than MAX_COUNT times (overlapping occurrences counted by a cheap upper bound)"""
    out = []
    for P in pats:
        N = normalise(P, non_acgt_to_a)
        runs = [s for s in N.replace(b"X", b" ").split() if len(s) <= 3]
        if all(text.count(s) * len(s) <= MAX_COUNT for s in runs):
            out.append(P)
    return out


def pad_ranges(seqs, w):
    starts = [int(x) for x in pfbwt_hip.doc_starts([len(s) for s in seqs], w)]
    return [(starts[k] + len(seqs[k]), starts[k] + len(seqs[k]) + w) for k in range(len(seqs))]


_cache = {}


def fixture_case(case):
    if case not in _cache:
        man, seqs, msexp = ms_fixture_case(case)
        riexp = ri_fixture_case(case)[2]
        rng = np.random.default_rng(FIXTURES.index(case) + 510)
        pads = pad_ranges(seqs, man["w"])
        pats = usable(riexp.model.text, make_patterns(rng, riexp.model, man["w"], pads), False)
        _cache[case] = (man, seqs, Expected(msexp.model, riexp.model, riexp.isa, pats, False, pads))
    return _cache[case]


def seeded_mem_case(ci, c):
    """None: the oracle or the index refuses the text (a one-word parse, EndOfWord bytes in .bwt)"""
    key = ("seeded", ci)
    if key not in _cache:
        got = seeded_case(ci, c)
        if got is None or got[2] is None:
            _cache[key] = None
        else:
            ref, ri_model, riexp, _ = got
            ms_model = MsModel(ref, thresholds_brute(ref["bwt"], lcp_numpy(ref["text"], ref["sa"]), ref["ssa"])[0])
            rng = np.random.default_rng(610 + ci)
            pads = pad_ranges(c["seqs"], c["w"])
            pats = usable(ri_model.text, make_patterns(rng, ri_model, c["w"], pads), c["non_acgt_to_a"])
            _cache[key] = Expected(ms_model, ri_model, riexp.isa, pats, c["non_acgt_to_a"], pads)
    return _cache[key]


def covered(exps, tag):
    total = {c: 0 for c in CLASSES}
    for exp in exps:
        lens, star = exp.min_lens()
        have = exp.classes(star + 1, star)
        for k in total:
            total[k] += have[k]
    missing = [c for c in CLASSES if not total[c]]
    assert not missing, (tag, missing)


# ---- one build through every route ---------------------------------------------------------------------------------------------
def prepare(ctx, has_sa, exp):
    """thresholds, both indexes and the matching statistics of the patterns"""
    if has_sa:
        ctx.thresholds()
    else:
        ctx.thresholds_windowed(window_for(int(ctx.bsizes.nout), 1024))
    ctx.ms_index(); ctx.ri_index()
    return ctx.ms_query(exp.pats)


def equal_results(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all(np.array_equal(u, v) for u, v in zip(x, y)) for x, y in zip(a[:-1], b[:-1]))


def run_build(ctx, exp, has_sa, tag):
    prepare(ctx, has_sa, exp)
    lens, star = exp.min_lens()
    routes = [1, 2] if has_sa else [1]
    first = {}
    for r in routes:
        ctx.debug_set(ri_route=r)
        for L in lens:
            got = ctx.mem_find(L, locate=True)
            exp.check(got, L, r, 0, (tag, "route", r, "min_len", L))
            if L in first:
                assert equal_results(first[L], got), (tag, "routes differ", L)
            first.setdefault(L, got)
    empty = first[exp.max_len + 1]                                       # no MEM at all: valid empty results
    assert empty[-1]["mems"] == 0 and all(x.size == 0 for x in empty[0]) and empty[4] == [] and ctx.mem_device_ptrs()[0]
    ctx.debug_set(ri_route=0)
    exp.check(ctx.mem_find(0, locate=True), 1, 2 if has_sa else 1, 0, (tag, "min_len 0 means 1"))
    got = ctx.mem_find(star)
    exp.check(got, star, 0, 0, (tag, "no locate"))
    assert equal_results(first[star][:3] + (None,), got), (tag, "no locate")
    cnts = type("Counts", (), {"cnt": [exp.count(exp.string(j, i, l)) for j, ms in enumerate(exp.all) for i, l in ms]})
    for r in routes:
        ctx.debug_set(ri_route=r)
        for mo in capped(cnts):
            exp.check(ctx.mem_find(1, locate=True, max_occ=mo), 1, r, mo, (tag, "max_occ", mo, r))
    for d in (0, 40):                                                    # the directories at one row / position and one block for everything
        ctx.debug_set(ms_dir_log2=d, ri_dir_log2=d, ri_route=1)
        ctx.ms_index(); ctx.ri_index(); ctx.ms_query(exp.pats)
        got = ctx.mem_find(1, locate=True)
        assert equal_results(first[1], got) and got[-1] == exp.info(1, 1), (tag, "dir_log2", d)
    ctx.debug_set(**DEFAULTS)


def check_fixtures(factory, cases=FIXTURES, light=()):
    exps = [fixture_case(case)[2] for case in cases]
    covered(exps, "fixtures")
    for ci, case in enumerate(cases):
        man, seqs, exp = fixture_case(case)
        for U, sa in ([(8, True)] if case in light else [(4, bool(ci % 2)), (8, not ci % 2)]):
            ctx = build(factory, seqs, man["w"], man["p"], U, sa=sa, rssa=True)
            run_build(ctx, exp, sa, (case, U))
            ctx.close()


def check_seeded(factory):
    reached, exps = 0, []
    for ci, c in enumerate(seeded_texts()):
        exp = seeded_mem_case(ci, c)
        if exp is None:
            continue
        exps.append(exp)
        for U in (4, 8):
            sa = c["sa"] if U == c["U"] else not c["sa"]
            ctx = build(factory, c["seqs"], c["w"], c["p"], U, sa=sa, rssa=True, non_acgt_to_a=c["non_acgt_to_a"])
            run_build(ctx, exp, sa, ("seeded", ci, U))
            ctx.close()
        reached += 1
    assert reached >= 5, reached
    covered(exps, "seeded")


def one_mem_patterns(text, k, rng):
    """k patterns with exactly one MEM each: eight text bytes between two bytes that do not occur"""
    return [b"X" + text[a:a + 8] + b"X" for a in rng.integers(0, len(text) - 8, k).tolist()]


def check_batch_shapes(factory):
    """0, 1, BLOCK and BLOCK + 1 MEMs (one lane in a second workgroup of the search), and one base past a tile of the flag sum"""
    man, seqs, exp = fixture_case("mult_chroms_fa")
    rng = np.random.default_rng(77)
    shapes = [[b"X", b"", b"XX"]] + [one_mem_patterns(exp.text, k, rng) for k in (1, BLOCK, BLOCK + 1)]
    shapes.append(one_mem_patterns(exp.text, SCAN_TILE // 10, rng) + [b"X" + exp.text[50:55] + b"X"])
    subs = [Expected(exp.ms, exp.ri, exp.isa, pats, False, exp.pads) for pats in shapes]
    assert [s.info(1, 0)["mems"] for s in subs[:4]] == [0, 1, BLOCK, BLOCK + 1] and subs[4].bases == SCAN_TILE + 1
    for U, sa in ((4, False), (8, True)):
        ctx = build(factory, seqs, man["w"], man["p"], U, sa=sa, rssa=True)
        for q, sub in enumerate(subs):
            prepare(ctx, sa, sub) if q == 0 else ctx.ms_query(sub.pats)
            sub.check(ctx.mem_find(1, locate=True), 1, 2 if sa else 1, 0, ("shape", q, U))
            sub.check(ctx.mem_find(1), 1, 0, 0, ("shape", q, U, "no locate"))
        ctx.close()


def check_state_and_errors(factory):
    E_STATE, E_ARG, E_NOMEM = pfbwt_hip.E_STATE, pfbwt_hip.E_ARG, pfbwt_hip.E_NOMEM
    man, seqs, exp = fixture_case("mult_chroms_fa")
    ref, w, p = fixture_expected("mult_chroms_fa")[2].ref, man["w"], man["p"]
    C = pfbwt_hip.C
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    small = Expected(exp.ms, exp.ri, exp.isa, exp.pats[:30], False, exp.pads)
    other = Expected(exp.ms, exp.ri, exp.isa, exp.pats[30:50], False, exp.pads)
    buf = np.empty(1 << 16, np.uint64)

    def status(f, *a, **kw):
        with pytest.raises(pfbwt_hip.PfpError) as e:
            f(*a, **kw)
        return e.value.status

    def nothing_made(ctx):
        L = ctx.L
        return (L.pfp_mem_get(ctx.h, vp(buf), None, None, None, None) == E_STATE and L.pfp_mem_get(ctx.h, None, None, None, None, None) == E_STATE and L.pfp_mem_write(ctx.h, -1, -1, -1, -1, -1) == E_STATE
                and L.pfp_mem_offsets_get(ctx.h, vp(buf), None, None, None) == E_STATE and ctx.mem_device_ptrs() == [None] * 5)

    ctx = factory(w=w, p=p, u64=True, sai=True)
    L = ctx.L
    assert L.pfp_mem_find(None, 1, 0, 0, None) == E_ARG and L.pfp_mem_get(None, None, None, None, None, None) == E_ARG and L.pfp_mem_write(None, -1, -1, -1, -1, -1) == E_ARG
    assert L.pfp_mem_offsets_get(None, None, None, None, None) == E_ARG and L.pfp_mem_device_ptrs(None, None, None, None, None, None) == E_ARG
    assert L.pfp_mem_find(ctx.h, 1, 0, 0, None) == E_STATE and nothing_made(ctx)                           # no build at all
    for s in seqs:
        ctx.feed(s, True)
    ctx.finalize(); ctx.parse_bwt(); ctx.bwt_build(sa=True, rssa=True)
    ctx.thresholds(); ctx.ms_index()
    assert status(ctx.mem_find) == E_STATE and nothing_made(ctx)                                          # no matching statistics yet
    ctx.ms_query(small.pats)
    assert status(ctx.mem_find, 1, locate=True) == E_STATE and nothing_made(ctx)                          # locate without a count / locate index
    before = ctx.bwt_get()
    ms_before = ctx.ms_query(small.pats)
    assert L.pfp_mem_find(ctx.h, 1, 0, 0, None) == 0                                                      # info is nullable
    small.check(ctx.mem_find(1), 1, 0, 0, "without an index")
    n1, n2 = C.c_uint64(0), C.c_uint64(0)
    assert L.pfp_mem_offsets_get(ctx.h, None, C.byref(n1), None, C.byref(n2)) == 0 and n1.value == len(small.pats) and n2.value == small.info(1, 0)["mems"]
    # after a find without locate there is no cnt / pos
    assert L.pfp_mem_get(ctx.h, None, None, None, vp(buf), None) == E_STATE and L.pfp_mem_get(ctx.h, None, None, None, None, vp(buf)) == E_STATE
    assert L.pfp_mem_offsets_get(ctx.h, None, None, vp(buf), None) == E_STATE and L.pfp_mem_write(ctx.h, -1, -1, -1, 1, -1) == E_STATE and L.pfp_mem_write(ctx.h, -1, -1, -1, -1, 1) == E_STATE
    d = ctx.mem_device_ptrs()
    assert d[0] and d[1] and d[2] and d[3] is None and d[4] is None
    ctx.ri_index()
    first = ctx.mem_find(1, locate=True)
    small.check(first, 1, 2, 0, "state")
    d = ctx.mem_device_ptrs()
    assert all(d) and len(set(d)) == 5
    ctx.debug_set(ri_route=1)
    small.check(ctx.mem_find(1, locate=True), 1, 1, 0, "phi beside the SA")
    ctx.debug_set(ri_route=0)
    assert ctx.mem_device_ptrs() == d                                                                     # a second find gives both slots back: the same MEMs lie where they lay
    for _ in range(2):
        ctx.mem_find(1, locate=True, max_occ=1)
        assert ctx.mem_device_ptrs()[:4] == d[:4]
    small.check(ctx.mem_find(3), 3, 0, 0, "a second find replaces the first")
    assert L.pfp_mem_get(ctx.h, None, None, None, vp(buf), None) == E_STATE
    assert ctx.mem_device_ptrs()[0] == d[0]                                                               # ... and so behind a find with locate
    ctx.mem_find(1, locate=True)
    assert ctx.mem_device_ptrs() == d
    # results survive the other post-passes in both orders, and a later query of other patterns
    first = ctx.mem_find_flat(1, locate=True)
    starts = pfbwt_hip.doc_starts([len(s) for s in seqs], w)

    def still_there(tag):
        now = {k: np.empty(first[k].size, np.uint64) for k in ("start", "len", "ptr", "cnt", "pos")}
        moff, poff = np.empty(first["mem_off"].size, np.uint64), np.empty(first["pos_off"].size, np.uint64)
        assert L.pfp_mem_get(ctx.h, *[vp(now[k]) for k in ("start", "len", "ptr", "cnt", "pos")]) == 0 and L.pfp_mem_offsets_get(ctx.h, vp(moff), None, vp(poff), None) == 0, tag
        assert all(same(now[k], first[k]) for k in now) and same(moff, first["mem_off"]) and same(poff, first["pos_off"]), tag

    ctx.thresholds(); ctx.ms_index(); ctx.ri_index(); ctx.lcp_array(); ctx.doc_array(starts)
    still_there("after the other passes")
    ctx.doc_array(starts); ctx.lcp_array(); ctx.ri_index(); ctx.ms_index(); ctx.thresholds()
    still_there("after the other passes, other order")
    ctx.ri_count(small.pats); ctx.ri_locate(small.pats[:5])
    ctx.ms_query(other.pats)                                                                              # a later query of other patterns
    still_there("after another ms_query")
    other.check(ctx.mem_find(1, locate=True), 1, 2, 0, "the MEMs of the other patterns")
    ms_again = ctx.ms_query(small.pats)                                                                   # matching statistics beside them: unchanged
    assert all(np.array_equal(x, y) for x, y in zip(ms_before[0] + ms_before[1], ms_again[0] + ms_again[1]))
    ctx.ms_query([])                                                                                      # npatterns = 0
    got = ctx.mem_find(1, locate=True)
    assert got[:5] == ([], [], [], [], []) and got[-1]["mems"] == 0 and got[-1]["patterns"] == 0
    f = ctx.mem_find_flat(1, locate=True)
    assert f["mem_off"].tolist() == [0] and f["pos_off"].tolist() == [0]
    after = ctx.bwt_get()                                                                                 # the published build is unchanged
    for k in ("bwt", "sa", "ssa", "esa"):
        assert np.array_equal(before[k], after[k]), k
    assert same(after["ssa"], ref["ssa"]) and same(after["bwt"], ref["bwt"])
    # a new build drops them; without an SA route 2 is refused
    ctx.ms_query(small.pats); ctx.mem_find(1, locate=True)
    ctx.bwt_build(sa=False, rssa=True)
    assert nothing_made(ctx) and status(ctx.mem_find) == E_STATE
    ctx.thresholds_windowed(0); ctx.ms_index(); ctx.ri_index(); ctx.ms_query(small.pats)
    small.check(ctx.mem_find(1, locate=True), 1, 1, 0, "rssa only")
    ctx.debug_set(ri_route=2)
    assert status(ctx.mem_find, 1, locate=True) == E_STATE                                                # the SA route without an SA
    small.check(ctx.mem_find(1), 1, 0, 0, "without locate the route does not matter")
    ctx.debug_set(ri_route=0)
    ctx.close()
    # PFP_E_NOMEM from a small workspace leaves a following capped call working
    ctx = None
    for mib in (24, 32, 48, 64, 96):
        try:
            ctx = build(lambda **kw: factory(workspace_bytes=mib << 20, **kw), seqs, w, p, 8, sa=False, rssa=True)
            ctx.thresholds_windowed(0); ctx.ms_index(); ctx.ri_index()
            break
        except pfbwt_hip.PfpError as e:
            assert e.status == E_NOMEM
            ctx = None
    assert ctx is not None
    t = exp.text
    singles = [t[a:a + 1] for a in range(4)]
    ms_big = ctx.ms_query(singles * 4000)                                                                # single bases: every one is a MEM that occurs in a quarter of the text
    assert status(ctx.mem_find, 1, locate=True) == E_NOMEM and nothing_made(ctx)
    assert ctx.L.pfp_workspace_needed(ctx.h) > (mib << 20)
    f = ctx.mem_find_flat(1, locate=True, max_occ=2)
    assert f["info"]["mems"] == 16000 and f["info"]["reported"] == 32000 and same(f["start"], np.zeros(16000)) and same(f["len"], np.ones(16000))
    for q, S in enumerate(singles):
        c, pos = brute_locate(t, exp.isa, S, 2)
        assert same(f["cnt"][q::4], np.full(4000, c)) and same(f["pos"].reshape(-1, 2)[q::4], np.tile(pos, (4000, 1))), S
    ptr, ln, _ = ctx.ms_query(singles * 4000)                                                            # the matching statistics were left as they were
    assert np.array_equal(np.concatenate(ptr), np.concatenate(ms_big[0])) and same(f["ptr"], np.concatenate(ptr))
    ctx.ms_query(small.pats)
    small.check(ctx.mem_find(1, locate=True), 1, 1, 0, "after NOMEM")
    ctx.close()


# ---- command line ------------------------------------------------------------------------------------------------------------
def check_cli(exe, factory, tmp):
    """exe: {'pfbwt-f': path, 'pfbwt-f64': path}"""
    man, seqs, exp = fixture_case("mult_chroms_fa")
    fa = os.path.join(GOLDEN, "mult_chroms_fa", "input.fa")
    wp = ["-w", str(man["w"]), "-p", str(man["p"])]
    reads = [p for p in exp.pats[:50] if p]
    sub = Expected(exp.ms, exp.ri, exp.isa, reads, False, exp.pads)
    fasta, fastq = os.path.join(tmp, "reads.fa"), os.path.join(tmp, "reads.fq")
    with open(fasta, "wb") as f:
        for j, r in enumerate(reads):
            f.write(b">r%d some words\n" % j + b"\n".join(r[k:k + 60] for k in range(0, len(r), 60)) + b"\n")
    with open(fastq, "wb") as f:
        for j, r in enumerate(reads):
            f.write(b"@r%d\n" % j + r + b"\n+\n" + b"@" * len(r) + b"\n")
    Lm, K = sub.min_lens()[1], 2
    EXT = ("mem.start", "mem.len", "mem.ptr", "mem.off", "mem.cnt", "mem.pos", "mem.poff")

    def files(pref):
        return {e: open(pref + "." + e, "rb").read() for e in ("bwt", "sa", "ssa", "esa", "thr", "tlcp", "ms.ptr", "ms.len", "ms.off", "cnt", "dict", "occ") if os.path.exists(pref + "." + e)}

    def same_files(pref, f, U, locate):
        for k, e in (("start", "mem.start"), ("len", "mem.len"), ("ptr", "mem.ptr")) + ((("cnt", "mem.cnt"), ("pos", "mem.pos")) if locate else ()):
            assert same(read_u(pref + "." + e, U), f[k]), (pref, e)
        assert same(read_u(pref + ".mem.off", 8), f["mem_off"]) and os.path.getsize(pref + ".mem.off") == 8 * (len(reads) + 1), pref
        if locate:
            assert same(read_u(pref + ".mem.poff", 8), f["pos_off"]) and os.path.getsize(pref + ".mem.poff") == 8 * (f["info"]["mems"] + 1), pref
        else:
            assert not any(os.path.exists(pref + "." + e) for e in EXT[4:]), pref

    for name, U in (("pfbwt-f64", 8), ("pfbwt-f", 4)):
        ctx = build(factory, seqs, man["w"], man["p"], U, sa=True, rssa=True)
        prepare(ctx, True, sub)
        plain_mems, located, capped_mems = ctx.mem_find_flat(Lm), ctx.mem_find_flat(1, locate=True), ctx.mem_find_flat(1, locate=True, max_occ=K)
        sub.check(ctx.mem_find(1, locate=True), 1, 2, 0, name)
        ctx.close()
        for rd, extra in ((fasta, ["-r"]), (fastq, ["-r", "-s", "--count", fasta])):
            base = "%s_%d" % (os.path.basename(rd), U)
            pref, plain = os.path.join(tmp, base), os.path.join(tmp, "plain_" + base)
            args = [exe[name]] + extra + ["--thr", "--ms", rd] + wp
            pr = run(args + ["--mems", "1", "--mems-locate", "-o", pref, fa])
            assert "TASK\tmems\t" in pr.stderr and "mems: %d reads, %d matches" % (len(reads), located["info"]["mems"]) in pr.stderr
            same_files(pref, located, U, True)
            run(args + ["-o", plain, fa])                                                              # every other output file: byte-identical
            a, b = files(pref), files(plain)
            assert a == b and "bwt" in a and "ms.ptr" in a and not any(os.path.exists(plain + "." + e) for e in EXT), (name, rd, sorted(a), sorted(b))
        pref = os.path.join(tmp, "nolocate_%d" % U)
        run([exe[name], "-r", "--thr", "--ms", fasta, "--mems", str(Lm)] + wp + ["-o", pref, fa])
        same_files(pref, plain_mems, U, False)
        pref = os.path.join(tmp, "capped_%d" % U)
        run([exe[name], "-r", "--thr", "--thr-window", "0", "--ms", fastq, "--mems", "0", "--mems-locate", "--mems-max", str(K)] + wp + ["-o", pref, fa])
        same_files(pref, capped_mems, U, True)
    efa = os.path.join(GOLDEN, "edge", "input.fa")

    def refused(args, opt, word, prefix):
        pr = run([exe["pfbwt-f64"]] + args + ["-w", "10", "-p", "20", "-o", prefix, efa], check=False)
        assert pr.returncode != 0 and opt in pr.stderr and word in pr.stderr.split("Command line")[-1].split("\n", 1)[1], pr.stderr[-500:]
        for e in ("bwt", "dict", "ms.ptr") + EXT:
            assert not os.path.exists(prefix + "." + e), (args, e)

    refused(["--mems", "3", "-r", "--thr"], "--mems", "--ms", os.path.join(tmp, "no_ms"))
    refused(["--mems-locate", "-r", "--thr", "--ms", fasta], "--mems-locate", "--mems ", os.path.join(tmp, "no_mems"))
    refused(["--mems-max", "3", "-r", "--thr", "--ms", fasta], "--mems-max", "--mems ", os.path.join(tmp, "no_mems2"))
    refused(["--mems-max", "3", "--mems", "2", "-r", "--thr", "--ms", fasta], "--mems-max", "--mems-locate", os.path.join(tmp, "no_locate"))
    h = run([exe["pfbwt-f"], "-h"]).stderr
    assert "--mems <L>" in h and "--mems-locate" in h and "--mems-max <K>" in h


def test_checkers_agree():
    """brute force against the rule of the header over brute-force matching statistics, without any engine, on every fixture and
    seeded case; every class occurs; the checker refuses a MEM that is dropped, shifted by one or shortened by one"""
    assert [f for f, _ in pfbwt_hip.MemInfo._fields_] == INFO_KEYS
    fix = [fixture_case(c)[2] for c in FIXTURES]
    seeded = [e for e in (seeded_mem_case(ci, c) for ci, c in enumerate(seeded_texts())) if e is not None]
    assert len(seeded) >= 5
    covered(fix, "fixtures")
    covered(seeded, "seeded")
    for exp in fix + seeded:
        lens, star = exp.min_lens()
        assert exp.max_len >= 2 and len(lens) >= 3
        for j, P in enumerate(exp.norm):
            ln = brute_ms(exp.text, P)
            for L in lens + [0]:
                assert rule_mems(ln, L) == exp.mems(L)[j], (P[:40], L)
            for i, l in exp.all[j]:                              # the model's pointer is an occurrence of the MEM
                p = exp.ptr[j][i]
                assert exp.text[p:p + l] == P[i:i + l] and p in exp.located(P[i:i + l], 0)[1]
        assert exp.info(exp.max_len + 1, 1)["mems"] == 0 and exp.info(star, 0)["mems"] > exp.info(star + 1, 0)["mems"]
    # the checker refuses wrong answers
    exp = fix[0]
    ms = exp.mems(1)
    j = next(j for j in range(len(ms)) if len(ms[j]) >= 2 and ms[j][0][1] >= 2)
    arr = lambda f: [np.array([f(j2, i, l) for i, l in ms[j2]], np.uint64) for j2 in range(len(ms))]
    good = (arr(lambda j2, i, l: i), arr(lambda j2, i, l: l), arr(lambda j2, i, l: exp.ptr[j2][i]), exp.info(1, 0))
    exp.check(good, 1, 0, 0, "good")
    for what in ("dropped", "shifted", "shortened"):
        start, ln, ptr = [list(x) for x in good[:3]]
        if what == "dropped":
            start[j], ln[j], ptr[j] = start[j][1:], ln[j][1:], ptr[j][1:]
        elif what == "shifted":
            start[j] = np.concatenate([start[j][:1] + 1, start[j][1:]]); ptr[j] = np.concatenate([ptr[j][:1] + 1, ptr[j][1:]])
        else:
            ln[j] = np.concatenate([ln[j][:1] - 1, ln[j][1:]])
        with pytest.raises(AssertionError):
            exp.check((start, ln, ptr, good[3]), 1, 0, 0, what)


# ---- CPU: the emulated library -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pfbwt-f_amd"), "emu", "emu-host"], check=True, stdout=subprocess.DEVNULL)
    return lambda **kw: pfbwt_hip.PfpContext(lib=EMU_SO, **kw)


def test_mems_fixtures_emu(emu):
    check_fixtures(emu, light=("panel8",))


def test_mems_seeded_emu(emu):
    check_seeded(emu)


def test_mems_batch_shapes_emu(emu):
    check_batch_shapes(emu)


def test_mems_state_and_errors_emu(emu):
    check_state_and_errors(emu)


def test_mems_cli_emu(emu, tmp_path):
    check_cli({"pfbwt-f": os.path.join(EMUB, "pfbwt-f-emu"), "pfbwt-f64": os.path.join(EMUB, "pfbwt-f64-emu")}, emu, str(tmp_path))


# ---- GPU: the product library --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_mems_fixtures_gpu(gpu_ctx_factory):
    check_fixtures(gpu_ctx_factory)


@pytest.mark.gpu
def test_mems_seeded_gpu(gpu_ctx_factory):
    check_seeded(gpu_ctx_factory)


@pytest.mark.gpu
def test_mems_batch_shapes_gpu(gpu_ctx_factory):
    check_batch_shapes(gpu_ctx_factory)


@pytest.mark.gpu
def test_mems_state_and_errors_gpu(gpu_ctx_factory):
    check_state_and_errors(gpu_ctx_factory)


@pytest.mark.gpu
def test_mems_cli_gpu(gpu_ctx_factory, tmp_path):
    check_cli({"pfbwt-f": os.path.join(BIN, "pfbwt-f"), "pfbwt-f64": os.path.join(BIN, "pfbwt-f64")}, gpu_ctx_factory, str(tmp_path))
