"""Count and locate queries on the device (include/pfbwt_hip.h: pfp_ri_index / pfp_ri_count / pfp_ri_locate; csrc/runindex.h;
pfbwt-f --count / --locate).

The expected values never come from the engine.  From the pinned oracle (text, bwt, sa, ssa, esa) there are two checkers:
* Model: the interval and toehold steps of the header and phi in plain Python over the oracle's .ssa / .esa and bwt -- exact lo, cnt,
  top, and the exact found / occurrences / reported / pieces / max_count / max_piece / phi_steps of info;
* brute force, independent of the model: all occurrences by bytes.find on the text, ordered by the oracle's inverse SA, the last
  min(cnt, max_occ) of them when capped.
test_checkers_agree shows model == brute force on every fixture and seeded case without any engine.
Every build (U = 4 and 8) is reused for every route: the default tunables, the phi directory at one position, two positions and one
block for everything (ri_dir_log2 = 0, 1, 40), the run directory at one row and one block (ms_dir_log2 = 0, 40), ri_route = 1, and on
builds with the SA ri_route = 2, which must equal the phi route bit for bit.
Reading of two cases the issue names: (1) "an interval emptied at the first step" -- the first step maps the full interval [0, n + 1)
to the whole segment of its symbol, so only a byte that heads no run can empty it; the class `empty_first` therefore holds patterns
whose LAST byte is such a byte, and `empty_second` the earliest step at which an interval of present bytes can become empty.  (2)
"phi through the last sorted sample" -- the largest sval is n, the sample of row 0, and no walk steps down from row 0; the class
`phi_last` asserts the last sample a walk can use, the one in front of it in text order.  (3) "a phi step that lands exactly on a
sample (p == sval[j])" -- phi is applied to the value of a row that is not the first of its piece, so never to the value of a run
start; what does happen, and what `phi_on_sample` asserts, is a step whose RESULT is a sample: a piece of at least two rows whose
first row starts its run."""
import bisect
import os
import subprocess
import numpy as np
import pytest
from pfp_testlib import EMU_SO, GOLDEN, ROOT, oracle_run, random_cases
from test_thresholds import build, fixture_expected, read_u, run, same
from test_matchstats import FIXTURES, mutated, normalise

import pfbwt_hip

EMUB = os.path.join(ROOT, "tests", "emu", "build")
BIN = os.path.join(ROOT, "pfbwt-f_amd", "bin")
RI_DEFAULTS = {"ri_dir_log2": -1, "ms_dir_log2": -1, "ri_route": 0}
ROUTES = [{"ri_route": 1}, {}, {"ri_dir_log2": 0, "ri_route": 1}, {"ri_dir_log2": 1, "ri_route": 1}, {"ri_dir_log2": 40, "ri_route": 1}, {"ms_dir_log2": 0, "ri_route": 1},
          {"ms_dir_log2": 40, "ri_route": 1}, {"ri_route": 2}]          # (the first one is checked against the checkers, the others against it)
INFO_KEYS = ["patterns", "bases", "found", "occurrences", "reported", "pieces", "max_count", "max_piece", "phi_steps", "route"]
BLOCK = 256                  # lanes per workgroup of the kernels (csrc/common.h)
CLASSES = ["absent_byte", "empty_first", "empty_second", "empty_middle", "empty_last", "count_one", "inside_run", "run_to_run", "three_runs", "phi_on_sample", "phi_first", "phi_last",
           "text_prefix", "text_prefix_plus", "text_suffix", "whole_record", "pads", "empty_pattern"]


# ---- the checkers ------------------------------------------------------------------------------------------------------------
class Model:
    """the steps of include/pfbwt_hip.h over the oracle's run samples and bwt"""

    def __init__(self, ref):
        self.text = bytes(ref["text"]); self.n = n = len(self.text)
        bwt = np.asarray(ref["bwt"], np.uint8)
        ssa = np.asarray(ref["ssa"], np.uint64).astype(np.int64); esa = np.asarray(ref["esa"], np.uint64).astype(np.int64)
        self.start, self.sval, self.end, self.eval = ssa[0::2].tolist(), ssa[1::2].tolist(), esa[0::2].tolist(), esa[1::2].tolist()
        self.head = bwt[ssa[0::2]].tolist()
        self.r = r = len(self.start)
        assert len(self.end) == r and self.start[0] == 0 and self.end[-1] == n
        self.lfhead, acc = [0] * r, 0
        for k in sorted(range(r), key=lambda k: self.head[k]):          # (sorted is stable)
            self.lfhead[k] = acc; acc += self.end[k] - self.start[k] + 1
        assert acc == n + 1
        self.runs_of = {}
        for k in range(r):
            self.runs_of.setdefault(self.head[k], []).append(k)
        self.seg_end = {}                                               # the end of every symbol's segment
        syms = sorted(self.runs_of)
        for a, c in enumerate(syms):
            self.seg_end[c] = self.lfhead[self.runs_of[syms[a + 1]][0]] if a + 1 < len(syms) else n + 1
        self.refused = 1 in self.runs_of
        order = sorted(range(r), key=lambda k: self.sval[k])
        self.pq = [self.sval[k] for k in order]; self.prun = order

    def run_of(self, row):
        return bisect.bisect_right(self.start, row) - 1

    def lfc(self, c, row):
        """(LFc(row), head of its run == c, the last run of c in front of its run or None)"""
        k = self.run_of(row)
        if self.head[k] == c:
            return self.lfhead[k] + (row - self.start[k]), True, None
        runs = self.runs_of[c]
        j = bisect.bisect_right(runs, k)
        return (self.lfhead[runs[j]] if j < len(runs) else self.seg_end[c]), False, (runs[j - 1] if j else None)

    def search(self, P):
        """P normalised; returns (lo, cnt, top, why) -- why: None found, 'empty', or ('absent' | 'emptied', steps taken before, m)"""
        n, m = self.n, len(P)
        if not m:
            return 0, 0, None, "empty"
        lo, hi, top = 0, n + 1, self.eval[-1]
        for i in range(m - 1, -1, -1):
            c = P[i]
            if c not in self.runs_of:
                return 0, 0, None, ("absent", m - 1 - i, m)
            lo2 = self.lfc(c, lo)[0]
            hi2, hit, kp = self.lfc(c, hi - 1)
            if hit:
                hi2 += 1; top -= 1
            elif kp is not None:
                top = self.eval[kp] - 1
                assert (self.end[kp] >= lo) == (lo2 < hi2)
            if lo2 >= hi2:
                return 0, 0, None, ("emptied", m - 1 - i, m)
            lo, hi = lo2, hi2
        return lo, hi - lo, top, None

    def phi(self, p, flags=None):
        i = bisect.bisect_right(self.pq, p) - 1
        j = self.prun[i]
        assert j > 0
        if flags is not None:
            flags["phi_first"] |= i == 0; flags["phi_last"] |= i == self.r - 2
        return self.eval[j - 1] + (p - self.pq[i])

    def locate(self, lo, cnt, top, max_occ, flags=None):
        """the reported values in row order and (pieces, longest piece, phi steps)"""
        if not cnt:
            return [], (0, 0, 0)
        hi = lo + cnt
        rep = min(cnt, max_occ) if max_occ else cnt
        first = hi - rep
        out, pieces, longest, steps = [0] * rep, 0, 0, 0
        for k in range(self.run_of(first), self.run_of(hi - 1) + 1):
            a, b = max(first, self.start[k]), min(hi - 1, self.end[k])
            p = top if b == hi - 1 else self.eval[k]
            pieces += 1; longest = max(longest, b - a + 1)
            if flags is not None and b > a and a == self.start[k]:
                flags["phi_on_sample"] = True
            for row in range(b, a - 1, -1):
                out[row - first] = p
                if row > a:
                    p = self.phi(p, flags); steps += 1
        return out, (pieces, longest, steps)


def brute_occurrences(text, P):
    out, i = [], text.find(P) if P else -1
    while i >= 0:
        out.append(i); i = text.find(P, i + 1)
    return out


def brute_locate(text, isa, P, max_occ):
    """(cnt, the reported positions): the occurrences in suffix order, the last min(cnt, max_occ) of them when capped"""
    occ = sorted(brute_occurrences(text, P), key=lambda p: isa[p])
    return len(occ), (occ[len(occ) - min(len(occ), max_occ):] if max_occ else occ)


class Expected:
    """the patterns of one build and what both checkers say about them"""

    def __init__(self, model, isa, pats, non_acgt_to_a):
        self.model, self.isa, self.pats = model, isa, [bytes(p) for p in pats]
        self.norm = [normalise(p, non_acgt_to_a) for p in self.pats]
        self.found = [model.search(P) for P in self.norm]
        self.cnt = np.array([f[1] for f in self.found], np.uint64)
        self.bases = sum(len(p) for p in self.pats)
        self._loc = {}

    def located(self, max_occ):
        if max_occ not in self._loc:
            pos, pieces, longest, steps = [], 0, 0, 0
            for P, (lo, cnt, top, _) in zip(self.norm, self.found):
                got, (a, b, c) = self.model.locate(lo, cnt, top, max_occ)
                bc, bpos = brute_locate(self.model.text, self.isa, P, max_occ)
                assert bc == cnt and bpos == got, ("model != brute force", P[:40], max_occ)
                pos.append(np.array(got, np.uint64)); pieces += a; longest = max(longest, b); steps += c
            self._loc[max_occ] = (pos, pieces, longest, steps)
        return self._loc[max_occ]

    def info(self, route, max_occ=0):
        want = dict(patterns=len(self.pats), bases=self.bases, found=int((self.cnt > 0).sum()), occurrences=int(self.cnt.sum()), max_count=int(self.cnt.max()) if self.cnt.size else 0,
                    reported=0, pieces=0, max_piece=0, phi_steps=0, route=route)
        if route:
            pos, pieces, longest, steps = self.located(max_occ)
            want.update(reported=sum(p.size for p in pos), pieces=pieces)
            if route == 1:
                want.update(max_piece=longest, phi_steps=steps)
        return want

    def check_count(self, got, tag):
        cnt, info = got
        assert same(cnt, self.cnt), (tag, "cnt")
        assert info == self.info(0), (tag, info, self.info(0))

    def check_locate(self, got, route, max_occ, tag):
        pos, cnt, info = got
        want = self.located(max_occ)[0]
        assert same(cnt, self.cnt), (tag, "cnt")
        assert len(pos) == len(want), tag
        for j in range(len(want)):
            assert same(pos[j], want[j]), (tag, "pos of pattern", j, self.pats[j][:40])
        assert info == self.info(route, max_occ), (tag, info, self.info(route, max_occ))


def inverse_sa(sa):
    sa = np.asarray(sa, np.uint64).astype(np.int64)
    isa = np.empty(sa.size, np.int64); isa[sa] = np.arange(sa.size)
    return isa


# ---- patterns ------------------------------------------------------------------------------------------------------------------
def classify(model, P, seqs_norm, w):
    """the classes of CLASSES a normalised pattern belongs to (by the model alone)"""
    out = set()
    lo, cnt, top, why = model.search(P)
    t, n = model.text, model.n
    if why == "empty":
        return {"empty_pattern"}
    if why is not None:
        kind, before, m = why
        if kind == "absent":
            out.add("absent_byte")
            if before == 0:
                out.add("empty_first")
        elif before == 1:
            out.add("empty_second")
        elif before == m - 1 and m >= 3:
            out.add("empty_last")
        elif 1 < before < m - 1:
            out.add("empty_middle")
        if len(P) > 1 and P[1:] == t[:len(P) - 1]:
            out.add("text_prefix_plus")
        return out
    hi = lo + cnt
    k0, k1 = model.run_of(lo), model.run_of(hi - 1)
    if cnt == 1:
        out.add("count_one")
    if cnt >= 2 and k0 == k1:
        out.add("inside_run")
    if cnt >= 2 and model.start[k0] == lo and model.end[k1] == hi - 1:
        out.add("run_to_run")
    if k1 - k0 >= 2:
        out.add("three_runs")
    if cnt <= 4000:
        flags = dict(phi_on_sample=False, phi_first=False, phi_last=False)
        model.locate(lo, cnt, top, 0, flags)
        out |= {k for k in flags if flags[k]}
    if P == t[:len(P)]:
        out.add("text_prefix")
    if P == t[n - len(P):]:
        out.add("text_suffix")
    if P in seqs_norm:
        out.add("whole_record")
    if P == b"A" * len(P) and len(P) >= w:
        out.add("pads")
    return out


def edge_patterns(model, seqs, w, non_acgt_to_a, rng, per_class=2):
    """patterns chosen from the model so that every class is hit; returns (patterns, {class: how many})"""
    t, n = model.text, model.n
    seqs_norm = {normalise(s, non_acgt_to_a) for s in seqs if s}
    cand = [b"", b"A" * w, b"A" * (w + 1), b"A" * (w // 2 + 1), t[:1], t[:7], t[:min(n, 40)], b"X" + t[:6], t[n - 1:], t[n - 9:], t[n - min(n, 33):], b"X", t[:5] + b"X", b"X" + t[3:9] + b"X"]
    cand += [s for s in sorted(seqs_norm, key=len)[:2]]
    absent = [c for c in b"ACGT" if c not in model.runs_of]
    cand += [t[:1] + bytes([c]) for c in absent]
    if n <= 400:
        cand += sorted({t[a:a + L] for L in range(1, 13) for a in range(n - L + 1)})
    else:
        for a in rng.integers(0, n - 12, 260).tolist():
            cand += [t[a:a + L] for L in (1, 2, 3, 4, 6, 9, 12)]
    # strings that occur nowhere, made from strings that do: the interval empties at the step of the changed byte
    for a in rng.integers(0, max(n - 14, 1), 60).tolist():
        s = t[a:a + int(rng.integers(3, 14))]
        for i in (0, 1, len(s) // 2, len(s) - 2):
            if 0 <= i < len(s):
                for c in b"ACGT":
                    cand.append(s[:i] + bytes([c]) + s[i + 1:])
    # samples: a suffix that starts at a run-start sample sits at a run start; its short prefixes walk through that sample
    for k in range(0, model.r, max(model.r // 40, 1)):
        for L in (1, 2, 3, 5):
            if model.sval[k] + L <= n:
                cand.append(t[model.sval[k]:model.sval[k] + L])
    present = [c for c in sorted(model.runs_of) if c]
    cand += [bytes([a, b]) for a in present for b in present]           # a pair of bytes that both occur, but not side by side: empty at the second step
    for i in (0, 1, model.r - 2):
        if 0 <= i < model.r:
            for L in (1, 2, 3, 4, 6):
                for d in range(0, 7):
                    p = model.pq[i] + d
                    if p + L <= n:
                        cand.append(t[p:p + L])
    seen, pats, have = set(), [], {c: 0 for c in CLASSES}
    for P in cand:
        if P in seen or len(P) > 2100:
            continue
        seen.add(P)
        cl = classify(model, P, seqs_norm, w)
        if any(have[c] < per_class for c in cl) and (model.search(P)[1] <= 3000):
            pats.append(P)
            for c in cl:
                have[c] += 1
    return pats, have


def classes_of(model, pats, seqs, w, non_acgt_to_a):
    """how many of the patterns fall into every class"""
    seqs_norm = {normalise(s, non_acgt_to_a) for s in seqs if s}
    have = {c: 0 for c in CLASSES}
    for P in pats:
        for c in classify(model, normalise(P, non_acgt_to_a), seqs_norm, w):
            have[c] += 1
    return have


def text_patterns(rng, text, count, max_len):
    """record pieces of 1 .. max_len bytes, with and without one substitution"""
    n, out = len(text), []
    for q in range(count):
        L = int(rng.integers(1, min(max_len, n) + 1)) if q % 4 else int(rng.integers(1, min(12, n) + 1))
        a = int(rng.integers(0, n - L + 1))
        out.append(mutated(rng, text[a:a + L], q % 2))
    return out


def capped(exp):
    """the max_occ values of the issue around a pattern that occurs at least three times (the smallest such count)"""
    c = [int(x) for x in exp.cnt if x >= 3]
    assert c, "no pattern occurs three times"
    c = min(c)
    return sorted({1, 2, c - 1, c, c + 1})


# ---- one build through every route ---------------------------------------------------------------------------------------------
def run_routes(ctx, exp, has_sa, tag, caps=True):
    first = None
    for route in ROUTES:
        tun = dict(RI_DEFAULTS); tun.update(route)
        if tun["ri_route"] == 2 and not has_sa:
            continue
        ctx.debug_set(**tun)
        ctx.ri_index()
        used = 2 if tun["ri_route"] == 2 or (tun["ri_route"] == 0 and has_sa) else 1
        got = ctx.ri_locate(exp.pats)
        if first is None:
            exp.check_count(ctx.ri_count(exp.pats), (tag, route))
            exp.check_locate(got, used, 0, (tag, route))
            first = got
        else:
            assert len(got[0]) == len(first[0]) and all(np.array_equal(a, b) for a, b in zip(got[0], first[0])) and np.array_equal(got[1], first[1]), (tag, route)
            assert got[2] == exp.info(used), (tag, route, got[2], exp.info(used))
    if caps:
        for r in ([1, 2] if has_sa else [1]):
            ctx.debug_set(**dict(RI_DEFAULTS, ri_route=r))
            for mo in capped(exp):
                exp.check_locate(ctx.ri_locate(exp.pats, max_occ=mo), r, mo, (tag, "max_occ", mo, r))
    ctx.debug_set(**RI_DEFAULTS)
    return first


_cache = {}


def fixture_case(case):
    if case not in _cache:
        man, seqs, texp = fixture_expected(case)
        model = Model(texp.ref)
        rng = np.random.default_rng(FIXTURES.index(case) + 70)
        pats = edge_patterns(model, seqs, man["w"], False, rng)[0]
        pats += text_patterns(rng, model.text, 90, 300)
        pats.insert(3, b""); pats.append(model.text[model.n // 3:model.n // 3 + 50].lower())
        have = classes_of(model, pats, seqs, man["w"], False)
        _cache[case] = (man, seqs, Expected(model, inverse_sa(texp.ref["sa"]), pats, False), have)
    return _cache[case]


def seeded_texts():
    """texts over AC and ACGT, 30 .. 2000 bases, 1 .. 6 records, two of them with two equal records"""
    out = []
    for ci, (ab, nrec, total, wp, twin) in enumerate([(b"AC", 1, 30, (3, 2), False), (b"ACGT", 2, 60, (6, 3), True), (b"AC", 3, 300, (4, 5), True), (b"ACGT", 4, 400, (4, 5), False),
                                                      (b"ACGT", 6, 2000, (6, 11), True), (b"AC", 5, 1200, (10, 20), False), (b"ACGT", 1, 900, (5, 7), False), (b"AC", 6, 700, (8, 11), True)]):
        rng = np.random.default_rng(900 + ci)
        lens = np.maximum(rng.multinomial(total, np.ones(nrec) / nrec), 1)
        seqs = [bytes(rng.choice(list(ab), int(L)).astype(np.uint8)) for L in lens]
        if twin:
            seqs[-1] = seqs[0]
        out.append(dict(seqs=seqs, w=wp[0], p=wp[1], U=8 if ci % 2 else 4, non_acgt_to_a=False, sa=ci % 3 != 2))
    return out


def seeded_case(ci, c):
    key = ("seeded", ci)
    if key not in _cache:
        ref = oracle_run(c["seqs"], w=c["w"], p=c["p"], U=8, non_acgt_to_a=c["non_acgt_to_a"])
        if ref.get("err") is not None:
            _cache[key] = None
        else:
            model = Model(ref)
            if model.refused:
                _cache[key] = (ref, model, None, None)
            else:
                rng = np.random.default_rng(300 + ci)
                pats = edge_patterns(model, c["seqs"], c["w"], c["non_acgt_to_a"], rng)[0]
                pats += text_patterns(rng, model.text, 24, 300)
                have = classes_of(model, pats, c["seqs"], c["w"], c["non_acgt_to_a"])
                _cache[key] = (ref, model, Expected(model, inverse_sa(ref["sa"]), pats, c["non_acgt_to_a"]), have)
    return _cache[key]


def all_seeded():
    return seeded_texts() + [dict(c, sa=bool(i % 2)) for i, c in enumerate(random_cases(5, 14))]


def assert_classes_covered(have, tag, skip=()):
    missing = [c for c in CLASSES if not have[c] and c not in skip]
    assert not missing, (tag, missing)


def check_fixtures(factory, cases=FIXTURES, light=()):
    total = {c: 0 for c in CLASSES}
    for case in cases:
        man, seqs, exp, have = fixture_case(case)
        assert not exp.model.refused, case
        for k in total:
            total[k] += have[k]
    # (a whole record of a fixture is longer than the patterns used here; the seeded texts have them)
    assert_classes_covered(total, "fixtures", skip=("whole_record",))
    for case in cases:
        man, seqs, exp, have = fixture_case(case)
        for U in ((8,) if case in light else (4, 8)):
            ctx = build(factory, seqs, man["w"], man["p"], U)
            run_routes(ctx, exp, True, (case, U))
            ctx.close()


def check_seeded(factory):
    refused = reached = 0
    total = {c: 0 for c in CLASSES}
    for ci, c in enumerate(all_seeded()):
        got = seeded_case(ci, c)
        if got is None:          # a one-word parse
            continue
        ref, model, exp, have = got
        tag = ("seeded", ci)
        if exp is None:          # EndOfWord bytes in .bwt: not the BWT of the text
            ctx = build(factory, c["seqs"], c["w"], c["p"], c["U"], non_acgt_to_a=c["non_acgt_to_a"])
            with pytest.raises(pfbwt_hip.PfpError) as e:
                ctx.ri_index()
            assert e.value.status == pfbwt_hip.E_STATE, tag
            with pytest.raises(pfbwt_hip.PfpError) as e:
                ctx.ri_count([b"A"])
            assert e.value.status == pfbwt_hip.E_STATE and ctx.ri_device_ptrs() == [None, None], tag
            ctx.close()
            refused += 1
            continue
        for k in total:
            total[k] += have[k]
        for U in (4, 8):
            ctx = build(factory, c["seqs"], c["w"], c["p"], U, sa=c["sa"], rssa=True, non_acgt_to_a=c["non_acgt_to_a"])
            run_routes(ctx, exp, c["sa"], tag + (U,))
            ctx.close()
        reached += 1
    assert refused >= 1 and reached >= 12, (refused, reached)
    assert_classes_covered(total, "seeded batch")


def batch_with_pieces(exp, want):
    """patterns of exp whose pieces (uncapped) number exactly `want`: greedy, the rest filled with one-piece patterns"""
    pieces = [exp.model.locate(lo, cnt, top, 0)[1][0] for lo, cnt, top, _ in exp.found]
    pick, total = [], 0
    for j in sorted(range(len(pieces)), key=lambda j: -pieces[j]):
        if pieces[j] > 1 and total + pieces[j] <= want - 8:
            pick.append(j); total += pieces[j]
    ones = [j for j in range(len(pieces)) if pieces[j] == 1]
    while total < want:
        pick.append(ones[(want - total) % len(ones)]); total += 1
    return [exp.pats[j] for j in pick]


def check_batch_shapes(factory):
    """64 and 65 patterns (the border of a wave) and a batch whose pieces number BLOCK + 1 (one lane in a second workgroup)"""
    man, seqs, exp, _ = fixture_case("mult_chroms_fa")
    isa = exp.isa
    for U in (4, 8):
        ctx = build(factory, seqs, man["w"], man["p"], U, sa=False, rssa=True)
        ctx.ri_index()
        for k in (64, 65):
            sub = Expected(exp.model, isa, exp.pats[:k], False)
            sub.check_count(ctx.ri_count(sub.pats), ("batch", k, U))
            sub.check_locate(ctx.ri_locate(sub.pats), 1, 0, ("batch", k, U))
        sub = Expected(exp.model, isa, batch_with_pieces(exp, BLOCK + 1), False)
        assert sub.info(1)["pieces"] == BLOCK + 1
        sub.check_locate(ctx.ri_locate(sub.pats), 1, 0, ("pieces", U))
        ctx.close()


def check_state_and_errors(factory):
    E_STATE, E_ARG, E_NOMEM, E_TOO_LARGE = pfbwt_hip.E_STATE, pfbwt_hip.E_ARG, pfbwt_hip.E_NOMEM, pfbwt_hip.E_TOO_LARGE
    man, seqs, exp, _ = fixture_case("mult_chroms_fa")
    ref, w, p = fixture_expected("mult_chroms_fa")[2].ref, man["w"], man["p"]
    C = pfbwt_hip.C
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    small = Expected(exp.model, exp.isa, exp.pats[:40], False)
    pats = small.pats
    buf = np.empty(int(exp.cnt.sum()) + 8, np.uint64)

    def status(f, *a, **kw):
        with pytest.raises(pfbwt_hip.PfpError) as e:
            f(*a, **kw)
        return e.value.status

    ctx = factory(w=w, p=p, u64=True, sai=True)
    L = ctx.L
    assert L.pfp_ri_index(None) == E_ARG and L.pfp_ri_index(ctx.h) == E_STATE                             # no build at all
    for s in seqs:
        ctx.feed(s, True)
    ctx.finalize(); ctx.parse_bwt(); ctx.bwt_build(sa=True, rssa=True)
    assert status(ctx.ri_count, pats) == E_STATE and status(ctx.ri_locate, pats) == E_STATE               # query before index
    assert L.pfp_ri_get(ctx.h, vp(buf), None) == E_STATE and L.pfp_ri_write(ctx.h, -1, -1, -1) == E_STATE and L.pfp_ri_offsets_get(ctx.h, vp(buf), None) == E_STATE
    assert L.pfp_ri_query_file(ctx.h, b"/nonexistent", 0, 0, None) == E_STATE and L.pfp_ri_query_file(ctx.h, None, 0, 0, None) == E_ARG
    assert ctx.ri_device_ptrs() == [None, None]
    ctx.ri_index()                                                                                        # needs no thresholds
    assert L.pfp_ri_get(ctx.h, vp(buf), None) == E_STATE                                                  # an index, no query yet
    assert L.pfp_ri_query_file(ctx.h, b"/nonexistent", 0, 0, None) == -9                                                          # PFP_E_IO
    before = ctx.bwt_get()
    small.check_count(ctx.ri_count(pats), "state")
    assert L.pfp_ri_get(ctx.h, vp(buf), vp(buf)) == E_STATE and L.pfp_ri_offsets_get(ctx.h, vp(buf), None) == E_STATE      # pos after a count
    assert L.pfp_ri_write(ctx.h, -1, -1, 1) == E_STATE and L.pfp_ri_write(ctx.h, -1, 1, -1) == E_STATE
    d = ctx.ri_device_ptrs()
    assert d[0] and d[1] is None
    small.check_locate(ctx.ri_locate(pats), 2, 0, "state")
    d = ctx.ri_device_ptrs()
    assert d[0] and d[1] and d[0] != d[1]
    cnt, info = ctx.ri_count([])                                                                          # npatterns = 0
    assert cnt.size == 0 and info["patterns"] == info["bases"] == info["found"] == 0
    pos, cnt, info = ctx.ri_locate([])
    assert pos == [] and cnt.size == 0 and info["reported"] == 0
    pos, cnt, info = ctx.ri_locate([b"", b""])
    assert [x.size for x in pos] == [0, 0] and cnt.tolist() == [0, 0] and info["patterns"] == 2 and info["bases"] == 0
    assert status(ctx.ri_count, [b"ACG", b"AC\x00T"]) == E_ARG and status(ctx.ri_locate, [b"\x00"]) == E_ARG       # a 0 byte
    bases = np.frombuffer(b"ACGTACGT", np.uint8)
    assert status(ctx.ri_count_flat, bases, [0, 5, 3]) == E_ARG and status(ctx.ri_locate_flat, bases, [0, 5, 3]) == E_ARG      # descending offsets
    off = np.array([0, 4], np.uint64)
    assert L.pfp_ri_count(ctx.h, None, vp(off), 1, None) == E_ARG and L.pfp_ri_count(ctx.h, vp(bases), None, 1, None) == E_ARG
    assert L.pfp_ri_locate(ctx.h, None, vp(off), 1, 0, None) == E_ARG and L.pfp_ri_locate(ctx.h, vp(bases), None, 1, 0, None) == E_ARG
    assert L.pfp_ri_count(ctx.h, vp(bases), vp(off), 1 << 32, None) == E_TOO_LARGE and L.pfp_ri_locate(ctx.h, vp(bases), vp(off), 1 << 32, 0, None) == E_TOO_LARGE
    assert L.pfp_ri_count(ctx.h, vp(bases), vp(off), 1, None) == 0                                        # info is nullable
    a = ctx.ri_locate_flat(bases, [2, 6, 8])                                                              # offsets need not start at 0
    b = ctx.ri_locate([b"GTAC", b"GT"])
    assert same(a[0], np.concatenate(b[0])) and same(a[2], b[1]) and a[3] == b[2] and a[1].tolist() == [0, b[0][0].size, b[0][0].size + b[0][1].size]
    # index and results survive thresholds, a matching-statistics index, LCP and document arrays, in this order and the other
    first = ctx.ri_locate(pats)
    starts = pfbwt_hip.doc_starts([len(s) for s in seqs], w)
    ctx.thresholds(); ctx.ms_index()
    ms_first = ctx.ms_query(pats)
    ctx.lcp_array(); ctx.doc_array(starts)
    cnt_now = np.empty(len(pats), np.uint64); pos_now = np.empty(int(first[1].sum()), np.uint64)
    assert L.pfp_ri_get(ctx.h, vp(cnt_now), vp(pos_now)) == 0 and same(cnt_now, first[1]) and same(pos_now, np.concatenate(first[0]))      # the results
    small.check_locate(ctx.ri_locate(pats), 2, 0, "after other passes")                                   # the index
    ctx.doc_array(starts); ctx.lcp_array(); ctx.ri_index(); ctx.ms_index(); ctx.thresholds()
    small.check_locate(ctx.ri_locate(pats), 2, 0, "second index, other order")
    ms_again = ctx.ms_query(pats)                                                                         # matching statistics beside it: unchanged
    assert all(np.array_equal(x, y) for x, y in zip(ms_first[0] + ms_first[1], ms_again[0] + ms_again[1])) and ms_first[2] == ms_again[2]
    ctx.debug_set(ri_route=1)
    small.check_locate(ctx.ri_locate(pats), 1, 0, "phi beside the SA")
    ctx.debug_set(ri_route=0)
    # the published build is unchanged by index and query
    after = ctx.bwt_get()
    for k in ("bwt", "sa", "ssa", "esa"):
        assert np.array_equal(before[k], after[k]), k
    assert same(after["ssa"], ref["ssa"]) and same(after["bwt"], ref["bwt"])
    # a new build drops index and results
    ctx.bwt_build(sa=False, rssa=True)
    assert L.pfp_ri_get(ctx.h, vp(buf), None) == E_STATE and ctx.ri_device_ptrs() == [None, None] and status(ctx.ri_count, pats) == E_STATE
    ctx.ri_index()                                                                                        # rssa only: phi
    small.check_locate(ctx.ri_locate(pats), 1, 0, "rssa only")
    ctx.debug_set(ri_route=2)
    assert status(ctx.ri_locate, pats) == E_STATE                                                         # the SA route without an SA
    small.check_count(ctx.ri_count(pats), "count does not care")
    ctx.debug_set(ri_route=0)
    ctx.bwt_build(sa=True, rssa=False)                                                                    # no run samples
    assert status(ctx.ri_index) == E_STATE
    ctx.bwt_build_slice(0, 2, sa=True, rssa=True)                                                         # a slice
    assert status(ctx.ri_index) == E_STATE
    ctx.close()
    # a context filled by pfp_bwt_load answers the same arrays as the one that parsed the text
    for sa in (True, False):
        ctx = factory(w=w, p=p, u64=True, sai=True)
        ctx.bwt_load(ref["dict"], ref["occ"], ref["bwlast"], ref["ilist"], ref["bwsai"], n_hint=ref["n"])
        ctx.bwt_build(sa=sa, rssa=True)
        ctx.ri_index()
        small.check_count(ctx.ri_count(pats), ("loaded", sa))
        got = ctx.ri_locate(pats)
        small.check_locate(got, 2 if sa else 1, 0, ("loaded", sa))
        assert all(np.array_equal(x, y) for x, y in zip(got[0], first[0]))
        ctx.close()
    # PFP_E_NOMEM from a tiny workspace leaves a following smaller query working
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
    t = exp.model.text
    big = [t[a:a + 1] for a in range(4)] * 40000                                                          # single bases: every one reports a quarter of the text
    assert status(ctx.ri_locate, big) == E_NOMEM
    assert ctx.L.pfp_workspace_needed(ctx.h) > (mib << 20)
    assert status(ctx.ri_count, [t[:60000]] * ((200 << 20) // min(len(t), 60000) + 1)) == E_NOMEM                  # 200 MiB of patterns
    small.check_locate(ctx.ri_locate(pats), 1, 0, "after NOMEM")
    small.check_locate(ctx.ri_locate(pats, max_occ=2), 1, 2, "after NOMEM, capped")
    ctx.debug_set(ri_dir_log2=1000, ms_dir_log2=1000, ri_route=7)                                         # values out of range are clamped, unknown keys refused
    ctx.ri_index()
    assert status(ctx.ri_locate, pats) == E_STATE                                                         # (route 2)
    ctx.debug_set(ri_route=-3)
    small.check_locate(ctx.ri_locate(pats), 1, 0, "clamped")
    with pytest.raises(pfbwt_hip.PfpError):
        ctx.debug_set(ri_dir=3)
    ctx.close()


# ---- command line ------------------------------------------------------------------------------------------------------------
def check_cli(exe, factory, tmp):
    """exe: {'pfbwt-f': path, 'pfbwt-f64': path}"""
    man, seqs, exp, _ = fixture_case("mult_chroms_fa")
    fa = os.path.join(GOLDEN, "mult_chroms_fa", "input.fa")
    wp = ["-w", str(man["w"]), "-p", str(man["p"])]
    reads = [p for p in exp.pats[:60] if p] + [exp.pats[-1]]
    sub = Expected(exp.model, exp.isa, reads, False)
    fasta, fastq = os.path.join(tmp, "reads.fa"), os.path.join(tmp, "reads.fq")
    with open(fasta, "wb") as f:
        for j, r in enumerate(reads):
            f.write(b">r%d some words\n" % j + b"\n".join(r[k:k + 60] for k in range(0, len(r), 60)) + b"\n")
    with open(fastq, "wb") as f:
        for j, r in enumerate(reads):
            f.write(b"@r%d\n" % j + r + b"\n+\n" + b"@" * len(r) + b"\n")
    K = capped(sub)[-2]

    def files(pref):
        return {e: open(pref + "." + e, "rb").read() for e in ("bwt", "sa", "ssa", "esa", "thr", "tlcp", "ms.ptr", "ms.len", "ms.off", "dict", "occ") if os.path.exists(pref + "." + e)}

    for name, U in (("pfbwt-f64", 8), ("pfbwt-f", 4)):
        ctx = build(factory, seqs, man["w"], man["p"], U, sa=False, rssa=True)
        ctx.ri_index()
        cnt = ctx.ri_count(reads)[0]
        pos, ooff, _, _ = ctx.ri_locate_flat(*ctx._flat_patterns(reads))
        posk, ooffk, _, _ = ctx.ri_locate_flat(*ctx._flat_patterns(reads), max_occ=K)
        ctx.close()
        sub.check_count((cnt, sub.info(0)), name)
        for rd, extra, other in ((fasta, ["-r"], []), (fastq, ["-r", "-s"], ["--thr", "--ms", fasta])):
            pref, plain = os.path.join(tmp, "%s_%d" % (os.path.basename(rd), U)), os.path.join(tmp, "plain_%s_%d" % (os.path.basename(rd), U))
            pr = run([exe[name], "--count", rd, "--locate", rd] + extra + other + wp + ["-o", pref, fa])
            assert "TASK\tcount\t" in pr.stderr and "TASK\tlocate\t" in pr.stderr
            assert same(read_u(pref + ".cnt", U), cnt) and same(read_u(pref + ".loc.cnt", U), cnt), (name, rd)
            assert same(read_u(pref + ".loc.pos", U), pos) and same(read_u(pref + ".loc.off", 8), ooff), (name, rd)
            assert os.path.getsize(pref + ".loc.off") == 8 * (len(reads) + 1)
            run([exe[name]] + extra + other + wp + ["-o", plain, fa])                                      # every other output file: byte-identical
            a, b = files(pref), files(plain)
            assert a == b and "bwt" in a and "ssa" in a and ("ms.ptr" in a) == bool(other), (name, rd, sorted(a), sorted(b))
        # capped, and from the files of a parse alone
        pref = os.path.join(tmp, "po_%d" % U)
        run([exe[name], "--parse-only", "-r"] + wp + ["-o", pref, fa])
        pr = run([exe[name], "--pfbwt-only", "-r", "--locate", fasta, "--locate-max", str(K)] + wp + ["-o", pref])
        assert same(read_u(pref + ".loc.cnt", U), cnt) and same(read_u(pref + ".loc.pos", U), posk) and same(read_u(pref + ".loc.off", 8), ooffk), name
        assert not os.path.exists(pref + ".cnt")
    efa = os.path.join(GOLDEN, "edge", "input.fa")

    def refused(args, opt, word, prefix):
        pr = run([exe["pfbwt-f64"]] + args + ["-w", "10", "-p", "20", "-o", prefix, efa], check=False)
        assert pr.returncode != 0 and opt in pr.stderr and word in pr.stderr, pr.stderr[-500:]
        for e in ("bwt", "cnt", "loc.cnt", "loc.pos", "loc.off", "dict"):
            assert not os.path.exists(prefix + "." + e), (args, e)

    for opt in ("--count", "--locate"):
        refused([opt, fasta], opt, "-r", os.path.join(tmp, "no_r" + opt))
        refused([opt, fasta, "-r", "--parse-only"], opt, "--parse-only", os.path.join(tmp, "po" + opt))
        refused([opt, fasta, "-r", "--gpus", "2"], opt, "--gpus", os.path.join(tmp, "gp" + opt))
    refused(["--locate-max", "3", "-r"], "--locate-max", "--locate", os.path.join(tmp, "lm"))
    h = run([exe["pfbwt-f"], "-h"]).stderr
    assert "--count" in h and "--locate" in h and "--locate-max" in h


def test_checkers_agree():
    """the model against brute force, without any engine: on every fixture and seeded case lo / cnt / top of the model are the rows of the
    oracle's SA whose suffix starts with the pattern, the model's located values are the brute-force occurrences in suffix order for
    every cap, every class of patterns occurs, and brute force refuses a value that is moved, dropped or out of order"""
    assert [f for f, _ in pfbwt_hip.RiInfo._fields_] == INFO_KEYS
    exps = [fixture_case(c)[2] for c in FIXTURES]
    total = {c: 0 for c in CLASSES}
    for ci, c in enumerate(all_seeded()):
        got = seeded_case(ci, c)
        if got is not None and got[2] is not None:
            exps.append(got[2])
            for k in total:
                total[k] += got[3][k]
    assert_classes_covered(total, "seeded batch")
    assert len(exps) >= 18
    for exp in exps:
        m, sa = exp.model, np.argsort(exp.isa)
        for mo in [0] + capped(exp):
            exp.located(mo)                                  # asserts model == brute force per pattern
        for P, (lo, cnt, top, why) in zip(exp.norm, exp.found):
            assert cnt == len(brute_occurrences(m.text, P))
            if cnt:
                assert top == sa[lo + cnt - 1] and all(m.text[int(s):int(s) + len(P)] == P for s in sa[lo:lo + cnt])
                assert (lo == 0 or m.text[int(sa[lo - 1]):int(sa[lo - 1]) + len(P)] != P) and (lo + cnt == m.n + 1 or m.text[int(sa[lo + cnt]):int(sa[lo + cnt]) + len(P)] != P)
        for p in range(0, m.n, max(m.n // 300, 1)):          # phi against the SA itself
            assert m.phi(p) == sa[exp.isa[p] - 1]
    # small texts: every substring of up to 12 bytes, and every such string with its last byte changed
    for ci, c in enumerate(seeded_texts()[:4]):
        ref, m, exp, _ = seeded_case(ci, c)
        subs = {m.text[a:a + L] for L in range(1, 13) for a in range(m.n - L + 1)}
        subs |= {s[:-1] + bytes([x]) for s in list(subs)[::7] for x in b"ACGT"}
        for P in subs:
            lo, cnt, top, _ = m.search(P)
            for mo in (0, 2):
                assert brute_locate(m.text, exp.isa, P, mo) == (cnt, m.locate(lo, cnt, top, mo)[0]), P
    # the brute-force checker refuses wrong answers
    exp = exps[0]
    j = next(j for j in range(len(exp.pats)) if exp.cnt[j] >= 3)
    good = exp.located(0)[0]
    for wrong in (np.concatenate([good[j][:1] + 1, good[j][1:]]), good[j][:-1], good[j][::-1]):
        bad = list(good); bad[j] = wrong
        with pytest.raises(AssertionError):
            exp.check_locate((bad, exp.cnt, exp.info(1)), 1, 0, "wrong")


# ---- CPU: the emulated library -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pfbwt-f_amd"), "emu", "emu-host"], check=True, stdout=subprocess.DEVNULL)
    return lambda **kw: pfbwt_hip.PfpContext(lib=EMU_SO, **kw)


def test_runindex_fixtures_emu(emu):
    check_fixtures(emu, light=("panel8",))


def test_runindex_seeded_emu(emu):
    check_seeded(emu)


def test_runindex_batch_shapes_emu(emu):
    check_batch_shapes(emu)


def test_runindex_state_and_errors_emu(emu):
    check_state_and_errors(emu)


def test_runindex_cli_emu(emu, tmp_path):
    check_cli({"pfbwt-f": os.path.join(EMUB, "pfbwt-f-emu"), "pfbwt-f64": os.path.join(EMUB, "pfbwt-f64-emu")}, emu, str(tmp_path))


# ---- GPU: the product library --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_runindex_fixtures_gpu(gpu_ctx_factory):
    check_fixtures(gpu_ctx_factory)


@pytest.mark.gpu
def test_runindex_seeded_gpu(gpu_ctx_factory):
    check_seeded(gpu_ctx_factory)


@pytest.mark.gpu
def test_runindex_batch_shapes_gpu(gpu_ctx_factory):
    check_batch_shapes(gpu_ctx_factory)


@pytest.mark.gpu
def test_runindex_state_and_errors_gpu(gpu_ctx_factory):
    check_state_and_errors(gpu_ctx_factory)


@pytest.mark.gpu
def test_runindex_cli_gpu(gpu_ctx_factory, tmp_path):
    check_cli({"pfbwt-f": os.path.join(BIN, "pfbwt-f"), "pfbwt-f64": os.path.join(BIN, "pfbwt-f64")}, gpu_ctx_factory, str(tmp_path))
