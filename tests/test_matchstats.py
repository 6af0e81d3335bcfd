"""Matching-statistics queries on the device (include/pfbwt_hip.h: pfp_ms_index / pfp_ms_query; csrc/matchstats.h; pfbwt-f --ms).

For every position i of a pattern P the engine returns a text position ptr[i] and the length len[i] of the longest prefix of
P[i:] that occurs in the text.  The expected values never come from the engine: text, bwt, ssa and esa are the pinned oracle's, the
thresholds are thresholds_brute over lcp_numpy (test_thresholds.py), and there are two checkers:
* Model: the five pointer steps of the header in plain Python over those arrays -- exact ptr, exact match / up / down / absent /
  breaks counts (thresholds are pinned to the leftmost minimiser, so ptr is fully determined);
* check_properties, independent of the model, for every position: T[ptr : ptr + len] == P[i : i + len], and P[i : i + len + 1]
  does not occur in T (bytes.find) unless i + len == m -- the search is made for the rightmost position of every distinct end
  i + len: a string that holds a string that does not occur does not occur either; on small texts len == brute_ms, which grows
  every length byte by byte with bytes.find.
Every build runs with the default tunables and again with the run directory at one row, two rows and one block for everything
(ms_dir_log2 = 0, 1, 40) and with ms_long_min = 1 (every break of more than one matching byte goes to the wave route), on
thresholds made with the defaults and with thr_long_min = 1 / thr_tile = 16, and on windowed thresholds of a build without SA --
windows of 16 rows on the small builds, five windows on the fixtures of 100 kbase and more, as in test_thresholds_windowed.py (every
window runs the emission again: 16-row windows over 2 M rows are hours on the emulated library, and on the card 7 000 to 130 000
emissions per build, each with its launches and a host round trip, where a case may take a few seconds).  This departs from the
issue, which names windows of 16 rows for every build; windows of 16 rows on the larger fixtures are what
test_thresholds_windowed.py's rows test covers.  All of them must give the arrays A second departure, on the emulated library only: panel8 (2 M rows, 100 s per build there) runs with U = 8 and its windowed
thresholds on the same build, not with both widths and a second build with run samples only; on the card it runs like the others."""
import bisect
import os
import subprocess
import numpy as np
import pytest
from pfp_testlib import EMU_SO, GOLDEN, ROOT, oracle_run, random_cases
from test_thresholds import DEFAULTS as THR_DEFAULTS, FORCED as THR_FORCED, build, fixture_expected, lcp_numpy, read_u, run, same, thresholds_brute

import pfbwt_hip

EMUB = os.path.join(ROOT, "tests", "emu", "build")
BIN = os.path.join(ROOT, "pfbwt-f_amd", "bin")
FIXTURES = ["edge", "w4p7", "mult_chroms_fa", "single_chrom", "mult_chroms", "panel8"]
MS_DEFAULTS = {"ms_dir_log2": -1, "ms_long_min": 512}
ROUTES = [{}, {"ms_dir_log2": 0}, {"ms_dir_log2": 1}, {"ms_dir_log2": 40}, {"ms_long_min": 1}]
SMALL_ROWS = 20000           # builds up to this size: windows of 16 rows, brute-force lengths
INFO_KEYS = ["patterns", "bases", "match", "up", "down", "absent", "breaks", "long_breaks", "max_len"]


# ---- the checkers ------------------------------------------------------------------------------------------------------------
def normalise(p, non_acgt_to_a):
    p = bytes(p).upper()
    return bytes(c if c in b"ACGT" else 65 for c in p) if non_acgt_to_a else p


class Model:
    """the pointer steps of include/pfbwt_hip.h over the oracle's arrays and brute-force threshold rows (one per run)"""

    def __init__(self, ref, thr_rows):
        self.text = bytes(ref["text"]); self.n = len(self.text)
        bwt = np.asarray(ref["bwt"], np.uint8)
        ssa = np.asarray(ref["ssa"], np.uint64).astype(np.int64); esa = np.asarray(ref["esa"], np.uint64).astype(np.int64)
        self.start, self.sval, self.end, self.eval = ssa[0::2].tolist(), ssa[1::2].tolist(), esa[0::2].tolist(), esa[1::2].tolist()
        self.head = bwt[ssa[0::2]].tolist()
        self.thr = [int(x) for x in thr_rows]
        r = len(self.start)
        assert len(self.thr) == r and len(self.end) == r
        self.lfhead, acc = [0] * r, 0
        for k in sorted(range(r), key=lambda k: self.head[k]):          # (sorted is stable)
            self.lfhead[k] = acc; acc += self.end[k] - self.start[k] + 1
        assert acc == self.n + 1
        self.runs_of = {}
        for k in range(r):
            self.runs_of.setdefault(self.head[k], []).append(k)
        self.refused = 1 in self.runs_of

    def pointers(self, P):
        """P normalised; returns (ptr, counts) -- counts also of the two jump edge cases"""
        n, ptr = self.n, [0] * len(P)
        cnt = dict(match=0, up=0, down=0, absent=0, up_no_kn=0, down_no_kp=0)
        row, pos = 0, n
        for i in range(len(P) - 1, -1, -1):
            c = P[i]; runs = self.runs_of.get(c)
            if not runs:
                ptr[i] = n; row, pos = 0, n; cnt["absent"] += 1
                continue
            k = bisect.bisect_right(self.start, row) - 1
            if self.head[k] == c:
                cnt["match"] += 1
            else:
                j = bisect.bisect_right(runs, k)
                kn = runs[j] if j < len(runs) else None
                kp = runs[j - 1] if j > 0 else None
                if kn is not None and (kp is None or row >= self.thr[kn]):
                    cnt["down"] += 1; cnt["down_no_kp"] += kp is None
                    k = kn; row, pos = self.start[k], self.sval[k]
                else:
                    cnt["up"] += 1; cnt["up_no_kn"] += kn is None
                    k = kp; row, pos = self.end[k], self.eval[k]
            row = self.lfhead[k] + (row - self.start[k]); pos -= 1; ptr[i] = pos
        return ptr, cnt


def count_breaks(ptr):
    return sum(1 for i in range(len(ptr)) if i == 0 or ptr[i] != ptr[i - 1] + 1)


def brute_ms(text, P):
    """len[i] = the longest prefix of P[i:] that occurs in text, grown byte by byte; the growth starts at the length of the position
    in front minus one, which is known to occur (a part of a string that occurs)"""
    out, L = [], 0
    for i in range(len(P)):
        L = max(L - 1, 0)
        while i + L < len(P) and text.find(P[i:i + L + 1]) >= 0:
            L += 1
        out.append(L)
    return out


def check_properties(text, P, ptr, ln, tag=None):
    """raises AssertionError at the first position whose (ptr, len) is not an occurrence of a longest match"""
    n, m, seen_end = len(text), len(P), set()
    assert len(ptr) == m and len(ln) == m, tag
    for i in range(m - 1, -1, -1):
        p, L = int(ptr[i]), int(ln[i])
        assert p + L <= n and i + L <= m, (tag, i, p, L)
        assert text[p:p + L] == P[i:i + L], (tag, i, p, L)
        e = i + L
        if e < m and e not in seen_end:                       # (a larger i with this end: this string holds that one)
            assert text.find(P[i:e + 1]) < 0, (tag, i, p, L)
            seen_end.add(e)


class Expected:
    """the patterns of one build and what the checkers say about them"""

    def __init__(self, model, pats, non_acgt_to_a, brute):
        self.model, self.pats = model, [bytes(p) for p in pats]
        self.norm = [normalise(p, non_acgt_to_a) for p in self.pats]
        self.ptr, self.counts = [], dict(match=0, up=0, down=0, absent=0, up_no_kn=0, down_no_kp=0)
        self.breaks = 0
        for P in self.norm:
            ptr, cnt = model.pointers(P)
            self.ptr.append(np.array(ptr, np.uint64))
            self.breaks += count_breaks(ptr)
            for k in cnt:
                self.counts[k] += cnt[k]
        self.bases = sum(len(p) for p in self.pats)
        self.brute = [np.array(brute_ms(model.text, P), np.uint64) for P in self.norm] if brute else None

    def lens_info(self, ln, long_min):
        brk_lens = [int(l[i]) for p, l in zip(self.ptr, ln) for i in range(len(p)) if i == 0 or int(p[i]) != int(p[i - 1]) + 1]
        return dict(long_breaks=sum(1 for x in brk_lens if x > long_min), max_len=max([int(l.max()) for l in ln if l.size] or [0]))

    def check(self, got, long_min, tag):
        ptr, ln, info = got
        assert len(ptr) == len(self.pats) and len(ln) == len(self.pats), tag
        for j, P in enumerate(self.norm):
            assert ptr[j].size == len(P) and same(ptr[j], self.ptr[j]), (tag, "ptr of pattern", j, self.pats[j][:40])
            check_properties(self.model.text, P, ptr[j], ln[j], (tag, j))
            if self.brute is not None:
                assert same(ln[j], self.brute[j]), (tag, "len of pattern", j)
        self.check_info(info, ln, long_min, tag)

    def check_info(self, info, ln, long_min, tag):
        want = dict(patterns=len(self.pats), bases=self.bases, breaks=self.breaks, **{k: self.counts[k] for k in ("match", "up", "down", "absent")})
        want.update(self.lens_info(ln, long_min))
        assert info == want, (tag, info, want)

    def check_same(self, first, got, long_min, tag):
        """another route: the arrays of the first run, bit for bit"""
        for a, b in ((first[0], got[0]), (first[1], got[1])):
            assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)), tag
        self.check_info(got[2], got[1], long_min, tag)


# ---- patterns ------------------------------------------------------------------------------------------------------------------
def mutated(rng, s, subs):
    b = bytearray(s)
    for _ in range(subs):
        if b:
            b[int(rng.integers(0, len(b)))] = int(rng.choice(list(b"ACGT")))
    return bytes(b)


def text_patterns(rng, text, count, long_every=8, short_max=100, long_max=500):
    """substrings of the text with 0 .. 4 substitutions: most of 1 .. short_max bytes, every long_every-th of up to long_max"""
    n, out = len(text), []
    for q in range(count):
        L = int(rng.integers(1, min(long_max if q % long_every == 0 else short_max, n) + 1))
        a = int(rng.integers(0, n - L + 1))
        out.append(mutated(rng, text[a:a + L], int(rng.integers(0, 5))))
    return out


def jump_edge_patterns(model, sa):
    """one pattern whose walk goes UP because no run of its first symbol lies behind its row, one that goes DOWN because none lies in
    front: a symbol (the rarest first) in front of the first bytes of one of the last / first suffixes of the SA"""
    n, out = model.n, []
    syms = [c for c in sorted(model.runs_of, key=lambda c: len(model.runs_of[c])) if c != 0]
    for key, rows in (("up_no_kn", (n, n - 1, n - 2, n - 4, n - 8)), ("down_no_kp", (1, 2, 3, 5, 9))):
        found = None
        for L in (30, 12, 6, 3, 1):
            for row in rows:
                s = int(sa[row]); S = model.text[s:s + L]
                for c in syms:
                    P = bytes([c]) + S
                    if found is None and S and model.pointers(P)[1][key]:
                        found = P
        assert found is not None, key
        out.append(found)
    return out


def fixture_patterns(case, seqs, w, model, sa):
    rng = np.random.default_rng(FIXTURES.index(case) + 40)
    text, n = model.text, model.n
    pats = text_patterns(rng, text, 200)
    pats += [bytes(rng.choice(list(b"ACGT"), int(rng.integers(1, 80))).astype(np.uint8)) for _ in range(10)]        # pure random
    pats.append(text[n // 2:n // 2 + 1])                                                  # length 1
    pats.insert(3, b"")                                                                   # an empty one between two others
    starts = [int(x) for x in pfbwt_hip.doc_starts([len(s) for s in seqs], w)]
    lens = [len(s) for s in seqs]
    e0 = starts[0] + lens[0]                                                              # the end of record 0, its w pad 'A's behind it
    assert text[e0:e0 + w] == b"A" * w
    pats.append(text[max(e0 - 20, 0):e0 + w + 20])                                        # across a record border, the pad inside
    k = min((k for k in range(len(seqs)) if lens[k]), key=lambda k: lens[k])
    pats.append(text[starts[k]:starts[k] + min(lens[k], 1500)])                           # a whole short record (the first 1500 bytes of a long one)
    pats.append(b"X" + text[0:30])                                                        # pos reaches 0: the terminator's row is stepped over
    pats.append(text[n - 30:n])
    pats.append(text[n // 3:n // 3 + 60].lower())                                         # lower case
    pats.append(b"X"); pats.append(b"AC" + b"X" + text[10:40])                            # a byte that does not occur
    pats.append(bytes(text[n // 2:n // 2 + 1]) * 600)                                     # one base 600 times
    for c in b"N-":                                                                       # N / '-' where the text has them (edge)
        i = text.find(bytes([c]))
        if i >= 0:
            pats.append(text[max(i - 10, 0):i + 12]); pats.append(b"ACG" + bytes([c]) * 3 + b"T")
    rare = min((c for c in model.runs_of if c), key=lambda c: len(model.runs_of[c]))       # begin / end with the rarest symbol
    for a in (n // 5, n // 2):
        pats.append(bytes([rare]) + text[a:a + 25]); pats.append(text[a:a + 25] + bytes([rare]))
    pats += jump_edge_patterns(model, sa)
    return pats


def assert_steps_covered(exp, tag):
    c = exp.counts
    assert min(c["match"], c["up"], c["down"], c["absent"]) > 0, (tag, c)
    assert c["up_no_kn"] > 0 and c["down_no_kp"] > 0, (tag, c)


# ---- one build through every route ---------------------------------------------------------------------------------------------
def window_for(nout, tile):
    if nout <= SMALL_ROWS:
        return 16
    return -(-(-(-nout // 5)) // tile) * tile          # five windows


def run_routes(factory, seqs, w, p, U, non_acgt_to_a, exp, tag, one_build=False):
    """one_build: the windowed thresholds on the build with the SA (which they ignore) instead of a second build with run samples only"""
    ctx = build(factory, seqs, w, p, U, non_acgt_to_a=non_acgt_to_a)
    first = None
    for thr_tun in (THR_DEFAULTS, THR_FORCED):
        ctx.debug_set(**thr_tun)
        ctx.thresholds()
        for route in ROUTES:
            tun = dict(MS_DEFAULTS); tun.update(route)
            ctx.debug_set(**tun)
            ctx.ms_index()
            got = ctx.ms_query(exp.pats)
            if first is None:
                exp.check(got, tun["ms_long_min"], (tag, U))
                first = got
            else:
                exp.check_same(first, got, tun["ms_long_min"], (tag, U, thr_tun, route))
    nout = int(ctx.bsizes.nout)
    if not one_build:
        ctx.close()
        ctx = build(factory, seqs, w, p, U, sa=False, rssa=True, non_acgt_to_a=non_acgt_to_a)      # windowed thresholds, no SA
    ctx.debug_set(**THR_DEFAULTS); ctx.debug_set(**MS_DEFAULTS)
    ctx.thresholds_windowed(window_for(nout, THR_DEFAULTS["thr_tile"]))
    ctx.ms_index()
    exp.check_same(first, ctx.ms_query(exp.pats), MS_DEFAULTS["ms_long_min"], (tag, U, "windowed"))
    ctx.close()
    return first


_expected_cache = {}


def fixture_case(case):
    if case not in _expected_cache:
        man, seqs, texp = fixture_expected(case)
        model = Model(texp.ref, texp.thr[1::2])
        pats = fixture_patterns(case, seqs, man["w"], model, texp.ref["sa"])
        _expected_cache[case] = (man, seqs, Expected(model, pats, False, brute=model.n + 1 <= SMALL_ROWS))
    return _expected_cache[case]


def check_fixtures(factory, cases=FIXTURES, light=()):
    """light: fixtures that run with U = 8 and one build only (a build of panel8 takes 100 s on the emulated library)"""
    for case in cases:
        man, seqs, exp = fixture_case(case)
        assert not exp.model.refused, case
        assert len(exp.pats) >= 200 and exp.bases < 20000, (case, len(exp.pats), exp.bases)
        assert_steps_covered(exp, case)
        for U in ((8,) if case in light else (4, 8)):
            first = run_routes(factory, seqs, man["w"], man["p"], U, False, exp, case, one_build=case in light)
            assert exp.lens_info(first[1], 1)["long_breaks"] > 0, case          # the forced route did send breaks to the waves


def check_seeded(factory):
    refused = reached = 0
    total = dict(match=0, up=0, down=0, absent=0)
    for ci, c in enumerate(random_cases(3, 60)):
        ref = oracle_run(c["seqs"], w=c["w"], p=c["p"], U=c["U"], non_acgt_to_a=c["non_acgt_to_a"])
        if ref.get("err") is not None:          # a one-word parse
            continue
        tag = ("seeded", ci)
        if 1 in set(np.asarray(ref["bwt"], np.uint8).tolist()):          # EndOfWord bytes in .bwt: not the BWT of the text
            ctx = build(factory, c["seqs"], c["w"], c["p"], c["U"], non_acgt_to_a=c["non_acgt_to_a"])
            ctx.thresholds()
            with pytest.raises(pfbwt_hip.PfpError) as e:
                ctx.ms_index()
            assert e.value.status == pfbwt_hip.E_STATE, tag
            assert ctx.ms_device_ptrs() == [None, None]
            ctx.close()
            refused += 1
            continue
        thr_rows = thresholds_brute(ref["bwt"], lcp_numpy(ref["text"], ref["sa"]), ref["ssa"])[0]
        model = Model(ref, thr_rows)
        assert not model.refused
        rng = np.random.default_rng(100 + ci)
        pats = text_patterns(rng, model.text, 36, short_max=60, long_max=200)
        pats += [bytes(rng.choice(list(b"ACGTN"), int(rng.integers(1, 40))).astype(np.uint8)) for _ in range(4)]
        pats += [b"", b"acgtn" + model.text[:20].lower(), b"X" + model.text[:12], model.text[-12:] + b"-"]
        exp = Expected(model, pats, c["non_acgt_to_a"], brute=True)
        run_routes(factory, c["seqs"], c["w"], c["p"], c["U"], c["non_acgt_to_a"], exp, tag)
        for k in total:
            total[k] += exp.counts[k]
        reached += 1
    assert refused >= 5 and reached >= 30, (refused, reached)
    assert min(total.values()) > 0, total


def check_state_and_errors(factory):
    E_STATE, E_ARG, E_NOMEM = pfbwt_hip.E_STATE, pfbwt_hip.E_ARG, pfbwt_hip.E_NOMEM
    man, seqs, exp = fixture_case("mult_chroms_fa")
    texp = fixture_expected("mult_chroms_fa")[2]
    ref, w, p = texp.ref, man["w"], man["p"]
    C = pfbwt_hip.C
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    pats = exp.pats[:40]
    small = Expected(exp.model, pats, False, brute=False)
    buf = np.empty(exp.bases + 8, np.uint64)

    def status(f, *a):
        with pytest.raises(pfbwt_hip.PfpError) as e:
            f(*a)
        return e.value.status

    ctx = factory(w=w, p=p, u64=True, sai=True)
    assert ctx.L.pfp_ms_index(None) == E_ARG and ctx.L.pfp_ms_index(ctx.h) == E_STATE                    # no build at all
    for s in seqs:
        ctx.feed(s, True)
    ctx.finalize(); ctx.parse_bwt(); ctx.bwt_build(sa=True, rssa=True)
    assert status(ctx.ms_query, pats) == E_STATE                                                          # query before index
    assert status(ctx.ms_index) == E_STATE                                                                # index without thresholds
    assert ctx.L.pfp_ms_get(ctx.h, vp(buf), vp(buf)) == E_STATE and ctx.L.pfp_ms_write(ctx.h, -1, -1) == E_STATE
    assert ctx.ms_device_ptrs() == [None, None]
    ctx.thresholds(); ctx.ms_index()
    assert ctx.L.pfp_ms_get(ctx.h, vp(buf), vp(buf)) == E_STATE                                           # an index, no query yet
    before = ctx.bwt_get(); thr_before = ctx.thresholds()[:2]
    small.check(ctx.ms_query(pats), 512, "state")
    ptr, ln, info = ctx.ms_query([])                                                                      # npatterns = 0
    assert ptr == [] and ln == [] and info["patterns"] == info["bases"] == info["breaks"] == 0
    ptr, ln, info = ctx.ms_query([b"", b""])
    assert [x.size for x in ptr] == [0, 0] and info["patterns"] == 2 and info["bases"] == 0
    assert status(ctx.ms_query, [b"ACG", b"AC\x00T"]) == E_ARG                                            # a 0 byte
    bases = np.frombuffer(b"ACGTACGT", np.uint8)
    assert status(ctx.ms_query_flat, bases, [0, 5, 3]) == E_ARG                                           # descending offsets
    off = np.array([0, 4], np.uint64)
    assert ctx.L.pfp_ms_query(ctx.h, None, vp(off), 1, None) == E_ARG and ctx.L.pfp_ms_query(ctx.h, vp(bases), None, 1, None) == E_ARG
    assert ctx.L.pfp_ms_query(ctx.h, vp(bases), vp(off), 1, None) == 0                                    # info is nullable
    a = ctx.ms_query_flat(bases, [2, 6, 8])                                                               # offsets need not start at 0
    b = ctx.ms_query([b"GTAC", b"GT"])
    assert same(a[0], np.concatenate(b[0])) and same(a[1], np.concatenate(b[1])) and a[2] == b[2]
    # the index survives a second thresholds call and LCP / document-array calls made after it; a second index replaces the first
    first = ctx.ms_query(pats)
    ctx.debug_set(**THR_FORCED); ctx.thresholds(); ctx.debug_set(**THR_DEFAULTS)
    ctx.lcp_array(); ctx.doc_array(pfbwt_hip.doc_starts([len(s) for s in seqs], w))
    small.check_same(first, ctx.ms_query(pats), 512, "after other passes")
    ctx.ms_index()
    small.check_same(first, ctx.ms_query(pats), 512, "second index")
    d = ctx.ms_device_ptrs()
    assert d[0] and d[1] and d[0] != d[1]
    # the published build is unchanged by index and query
    after = ctx.bwt_get(); thr_after = ctx.thresholds()[:2]
    for k in ("bwt", "sa", "ssa", "esa"):
        assert np.array_equal(before[k], after[k]), k
    assert same(thr_before[0], thr_after[0]) and same(thr_before[1], thr_after[1]) and same(after["ssa"], ref["ssa"]) and same(after["bwt"], ref["bwt"])
    # a new build drops both slots
    ctx.bwt_build(sa=False, rssa=True)
    assert ctx.L.pfp_ms_get(ctx.h, vp(buf), vp(buf)) == E_STATE and ctx.ms_device_ptrs() == [None, None]
    assert status(ctx.ms_query, pats) == E_STATE and status(ctx.ms_index) == E_STATE                      # (no thresholds either)
    ctx.thresholds_windowed(2000); ctx.ms_index()                                                         # rssa only: windowed thresholds will do
    small.check_same(first, ctx.ms_query(pats), 512, "rssa only")
    ctx.bwt_build(sa=True, rssa=False)                                                                    # no run samples
    assert status(ctx.ms_index) == E_STATE
    ctx.bwt_build_slice(0, 2, sa=True, rssa=True)                                                         # a slice
    assert status(ctx.ms_index) == E_STATE
    ctx.close()
    ctx = factory(w=w, p=p, u64=True, sai=True)                                                           # a loaded parse: no text
    ctx.bwt_load(ref["dict"], ref["occ"], ref["bwlast"], ref["ilist"], ref["bwsai"], n_hint=ref["n"])
    ctx.bwt_build(sa=True, rssa=True)
    assert status(ctx.ms_index) == E_STATE
    ctx.close()
    # PFP_E_NOMEM from a tiny workspace leaves a following smaller query working
    ctx = None
    for mib in (24, 32, 48, 64, 96):
        try:
            ctx = build(lambda **kw: factory(workspace_bytes=mib << 20, **kw), seqs, w, p, 8)
            ctx.thresholds(); ctx.ms_index()
            break
        except pfbwt_hip.PfpError as e:
            assert e.status == E_NOMEM
            ctx = None
    assert ctx is not None
    big = [exp.model.text[:60000]] * 40
    assert status(ctx.ms_query, big) == E_NOMEM
    small.check_same(first, ctx.ms_query(pats), 512, "after NOMEM")
    ctx.debug_set(ms_dir_log2=1000, ms_long_min=0)                                                        # values out of range are clamped, unknown keys refused
    ctx.ms_index(); small.check_same(first, ctx.ms_query(pats), 1, "clamped")
    with pytest.raises(pfbwt_hip.PfpError):
        ctx.debug_set(ms_dir=3)
    ctx.close()


# ---- command line ------------------------------------------------------------------------------------------------------------
def check_cli(exe, factory, tmp):
    """exe: {'pfbwt-f': path, 'pfbwt-f64': path}"""
    man, seqs, exp = fixture_case("mult_chroms_fa")
    fa = os.path.join(GOLDEN, "mult_chroms_fa", "input.fa")
    wp = ["-w", str(man["w"]), "-p", str(man["p"])]
    reads = [p for p in exp.pats[:60] if p] + [exp.pats[-1]]
    fasta, fastq = os.path.join(tmp, "reads.fa"), os.path.join(tmp, "reads.fq")
    with open(fasta, "wb") as f:
        for j, r in enumerate(reads):
            f.write(b">r%d some words\n" % j + b"\n".join(r[k:k + 60] for k in range(0, len(r), 60)) + b"\n")
    with open(fastq, "wb") as f:
        for j, r in enumerate(reads):
            f.write(b"@r%d\n" % j + r + b"\n+\n" + b"@" * len(r) + b"\n")
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    for name, U in (("pfbwt-f64", 8), ("pfbwt-f", 4)):
        ctx = build(factory, seqs, man["w"], man["p"], U)
        ctx.thresholds(); ctx.ms_index()
        ptr, ln, _ = ctx.ms_query(reads)
        ctx.close()
        for rd, extra in ((fasta, []), (fastq, ["--thr-window", "2000"])):
            pref = os.path.join(tmp, "%s_%d" % (os.path.basename(rd), U))
            pr = run([exe[name], "-r", "--thr", "--ms", rd] + extra + wp + ["-o", pref, fa])
            assert "TASK\tmatching statistics\t" in pr.stderr
            assert same(read_u(pref + ".ms.ptr", U), np.concatenate(ptr)), (name, rd)
            assert same(read_u(pref + ".ms.len", U), np.concatenate(ln)), (name, rd)
            assert same(read_u(pref + ".ms.off", U), off), (name, rd)
            assert os.path.getsize(pref + ".ms.off") == U * off.size
            assert os.path.exists(pref + ".thr") and os.path.exists(pref + ".bwt")
    efa = os.path.join(GOLDEN, "edge", "input.fa")

    def refused(args, word, prefix):
        pr = run([exe["pfbwt-f64"]] + args + ["-w", "10", "-p", "20", "-o", prefix] + ([efa] if "--pfbwt-only" not in args else []), check=False)
        assert pr.returncode != 0 and "--ms" in pr.stderr and word in pr.stderr, pr.stderr[-500:]
        for e in ("bwt", "ms.ptr", "ms.len", "ms.off", "dict"):
            assert not os.path.exists(prefix + "." + e), (args, e)

    refused(["--ms", fasta], "-r", os.path.join(tmp, "no_r"))
    refused(["--ms", fasta, "-r"], "--thr", os.path.join(tmp, "no_thr"))
    refused(["--ms", fasta, "-r", "--thr", "--parse-only"], "--parse-only", os.path.join(tmp, "po"))
    refused(["--ms", fasta, "-r", "--thr", "--gpus", "2"], "--gpus", os.path.join(tmp, "gp"))
    refused(["--ms", fasta, "-r", "--thr", "--pfbwt-only"], "--pfbwt-only", os.path.join(tmp, "pb"))
    assert "--ms" in run([exe["pfbwt-f"], "-h"]).stderr


def test_checkers_agree():
    """the model against brute force and the property checker, without any engine: on hand-made texts every length of the model's
    pointers is the brute-force one, every step kind and both jump edge cases occur, and the property checker refuses a length that is
    one too short, one too long, and a pointer that is moved"""
    assert [f for f, _ in pfbwt_hip.MsInfo._fields_] == INFO_KEYS
    rng = np.random.default_rng(6)
    rnd = lambda k, ab=b"ACGT": bytes(rng.choice(list(ab), k).astype(np.uint8))
    base = rnd(400)
    total = dict(match=0, up=0, down=0, absent=0, up_no_kn=0, down_no_kp=0)
    for t in (b"ACGTACGAACGTNNACGT-ACGTTTTTACG", base + mutated(rng, base, 9) + b"NNNN" + rnd(150, b"AC") + mutated(rng, base, 5)[:200]):
        n = len(t)
        sa = np.array(sorted(range(n + 1), key=lambda i: t[i:] + b"\x00"), np.int64)
        bwt = np.array([t[i - 1] if i else 0 for i in sa], np.uint8)
        lcp = lcp_numpy(t, sa)
        starts = np.flatnonzero(np.concatenate([[True], bwt[1:] != bwt[:-1]]))
        ends = np.concatenate([starts[1:] - 1, [n]])
        pair = lambda rows: np.stack([rows, sa[rows]], 1).reshape(-1).astype(np.uint64)
        ref = dict(text=np.frombuffer(t, np.uint8), bwt=bwt, ssa=pair(starts), esa=pair(ends), n=n)
        model = Model(ref, thresholds_brute(bwt, lcp, ref["ssa"])[0])
        pats = text_patterns(rng, t, 60, short_max=40, long_max=120) + [rnd(20), b"X" + t[:9], t[-9:], b"G" + t[:5], b"NN", b"TTTTTTTTTT", b"X"]
        pats += jump_edge_patterns(model, sa)
        for P in pats:
            ptr, cnt = model.pointers(P)
            for k in cnt:
                total[k] += cnt[k]
            ln = [0] * len(P)
            for i in range(len(P)):                      # the definition of len, restated with a plain loop
                while i + ln[i] < len(P) and ptr[i] + ln[i] < n and P[i + ln[i]] == t[ptr[i] + ln[i]]:
                    ln[i] += 1
            assert ln == brute_ms(t, P), P
            b = 0
            for i in range(len(P)):                      # lengths from the last break, as the engine fills them in
                if i == 0 or ptr[i] != ptr[i - 1] + 1:
                    b = i
                assert ln[i] == ln[b] - (i - b) and (ln[i] >= 1 or ptr[i] == n or t.find(P[i:i + 1]) < 0), (P, i)
            check_properties(t, P, ptr, ln)
            for i in range(len(P)):
                for dl, dp in ((-1, 0), (1, 0), (0, 1)):
                    if ln[i] + dl < 0 or (dp and ln[i] == 0):
                        continue
                    wl, wp = list(ln), list(ptr)
                    wl[i] += dl; wp[i] += dp
                    if dp and wp[i] + wl[i] <= n and t[wp[i]:wp[i] + wl[i]] == P[i:i + wl[i]]:
                        continue                           # (another occurrence of the same match: also right)
                    with pytest.raises(AssertionError):
                        check_properties(t, P, wp, wl)
    assert min(total.values()) > 0, total


# ---- CPU: the emulated library -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pfbwt-f_amd"), "emu", "emu-host"], check=True, stdout=subprocess.DEVNULL)
    return lambda **kw: pfbwt_hip.PfpContext(lib=EMU_SO, **kw)


def test_matchstats_fixtures_emu(emu):
    check_fixtures(emu, light=("panel8",))


def test_matchstats_seeded_emu(emu):
    check_seeded(emu)


def test_matchstats_state_and_errors_emu(emu):
    check_state_and_errors(emu)


def test_matchstats_cli_emu(emu, tmp_path):
    check_cli({"pfbwt-f": os.path.join(EMUB, "pfbwt-f-emu"), "pfbwt-f64": os.path.join(EMUB, "pfbwt-f64-emu")}, emu, str(tmp_path))


# ---- GPU: the product library --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_matchstats_fixtures_gpu(gpu_ctx_factory):
    check_fixtures(gpu_ctx_factory)


@pytest.mark.gpu
def test_matchstats_seeded_gpu(gpu_ctx_factory):
    check_seeded(gpu_ctx_factory)


@pytest.mark.gpu
def test_matchstats_state_and_errors_gpu(gpu_ctx_factory):
    check_state_and_errors(gpu_ctx_factory)


@pytest.mark.gpu
def test_matchstats_cli_gpu(gpu_ctx_factory, tmp_path):
    check_cli({"pfbwt-f": os.path.join(BIN, "pfbwt-f"), "pfbwt-f64": os.path.join(BIN, "pfbwt-f64")}, gpu_ctx_factory, str(tmp_path))


@pytest.mark.gpu
def test_matchstats_reads_gpu(gpu_ctx_factory):
    """mult_chroms (330 kbase) with 1024 reads of at most 150 bases sampled from the text with about 1 % substitutions, in both
    widths: several workgroups of k_ms_pointers, lengths sorted across waves, the results scattered back to the reads' own places.
    Every position is property-checked; the pointers and counts are the model's."""
    man, seqs, _ = fixture_case("mult_chroms")
    texp = fixture_expected("mult_chroms")[2]
    model = Model(texp.ref, texp.thr[1::2])
    rng = np.random.default_rng(77)
    text, n = model.text, model.n
    reads = []
    for q in range(1024):
        L = int(rng.integers(1, 151)) if q % 3 else 150
        a = int(rng.integers(0, n - L + 1))
        reads.append(mutated(rng, text[a:a + L], int(rng.binomial(L, 0.01))))
    exp = Expected(model, reads, False, brute=False)
    assert exp.counts["up"] + exp.counts["down"] > 0 and exp.breaks > 1024
    for U in (4, 8):
        ctx = build(gpu_ctx_factory, seqs, man["w"], man["p"], U, sa=True, rssa=True)
        ctx.thresholds(); ctx.ms_index()
        exp.check(ctx.ms_query(reads), 512, ("reads", U))
        ctx.close()
