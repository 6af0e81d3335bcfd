"""Both recursive suffix sorts at their length limits, on both sides of each.  csrc/dictrec.h sorts the dictionary through a level-2
parse of it (4-byte windows, p2 = 16): byte-identical dictionary suffixes stay ONE tie class however many level-2 phrases they share
(k_dr_p2_heads + k_dr_p2_double), a longest level-2 phrase of DR_MAX_PHRASE = 1024 bytes takes the route and one of 1025 gives it up.
csrc/recsort.h sorts an integer string the same way: REC_MAX_PHRASE = 1024 symbols taken, 1025 given up.  Every case runs in a
subprocess with PFP_TEST_HOOKS=1, PFP_VERBOSE=1 and the forcing switches, compares every array bit-exact with the oracle, and asserts
from the verbose lines which route ran.  CPU: tests/emu with poisoned memory; GPU: the product library, plus one collection that takes
the dictionary route with the default switches."""
import hashlib
import itertools
import os
import subprocess
import sys
import numpy as np
import pytest
from pfp_testlib import ROOT


def mix32(v):
    """the 32-bit hash of dr_trigger (dictrec.h) and rs_trigger (recsort.h)"""
    h = (v * 0x9E3779B1) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0x85EBCA77) & 0xFFFFFFFF
    h ^= h >> 13
    return h


def dr_window_triggers(win, p2=16):
    """dr_trigger for a 4-byte window inside a word: the window ends a level-2 phrase"""
    return min(win) > 1 and mix32(int.from_bytes(bytes(win), "big")) % p2 == 0


def level2_phrase_lengths(D, p2=16):
    """lengths of the level-2 phrases of a dictionary image (k_dr_trig_write + k_dr_starts): a phrase ends at a triggering window and
    at every EndOfWord, the next one starts 3 bytes in front of that end (behind an EndOfWord: at the next word)"""
    D = bytes(D)
    lens, prev = [], None
    for x in range(len(D)):
        if D[x] == 1 or (D[x] != 0 and x >= 3 and dr_window_triggers(D[x - 3:x + 1], p2)):
            s = 0 if prev is None else (prev + 1 if D[prev] == 1 else prev - 3)
            lens.append(x - s + 1)
            prev = x
    return lens


def text_trigger(kmer_bytes, p):
    """the text-level trigger of the parse (w = len(kmer_bytes)): the oracle's Wang hash of the 2-bit k-mer, mod p"""
    from pfp_testlib import oracle
    v = 0
    for b in kmer_bytes:
        v = (v << 2) | b"ACGT".index(b)
    return oracle().orc_wang_hash(v) % p == 0


def rnd(rng, n):
    return bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))


def flanked(stretch, order=b"TGC", seed=1):
    """one record per byte of `order`: a shared left flank, that byte, the stretch, a shared right flank.  The byte in front makes the
    stretch's group of identical dictionary suffixes "hard" (different preceding bytes); in this order the records' suffixes sort in
    the parse otherwise than the words that follow their words in the dictionary, so a tie class split in two changes .bwt and .sa"""
    rng = np.random.default_rng(seed)
    left, right = rnd(rng, 400), rnd(rng, 400)
    return [left[:-1] + bytes([b]) + stretch + right for b in order]


def periodic_unit(p2):
    """the first repeat unit (2 or 3 bases, not a run of one base) inside which every 4-byte window ends a level-2 phrase at p2 (or, at
    p2 = 16 where no such unit exists, at least one window per period) and no 10-mer triggers the text-level parse (w = 10, p = 100)"""
    for need_all in (True, False):
        for L in (2, 3):
            for u in itertools.product(b"ACGT", repeat=L):
                u = bytes(u)
                if len(set(u)) == 1:
                    continue
                s = u * 8
                hits = [dr_window_triggers(s[i:i + 4], p2) for i in range(L)]
                if (all(hits) if need_all else any(hits)) and not any(text_trigger(s[i:i + 10], 100) for i in range(L)):
                    return u
    raise AssertionError("no repeat unit triggers at p2=%d" % p2)


def homopolymer_base():
    """a base whose runs neither end a level-2 phrase nor trigger the text-level parse: a run of it is ONE long level-2 phrase"""
    for b in b"CGT":
        if not dr_window_triggers(bytes([b]) * 4) and not text_trigger(bytes([b]) * 10, 100):
            return b
    raise AssertionError("every base triggers")


def long_phrase_records(target):
    """records whose dictionary has a longest level-2 phrase of exactly `target` bytes (a homopolymer run, its length found by search)"""
    from pfp_testlib import oracle_run
    b = homopolymer_base()
    for L in range(target - 60, target + 20):
        seqs = flanked(bytes([b]) * L)
        if max(level2_phrase_lengths(oracle_run(seqs, w=10, p=100, U=8, want_sa=False)["dict"])) == target:
            return seqs
    raise AssertionError("no run length gives a level-2 phrase of %d bytes" % target)


def dict_case(name):
    """(seqs, w, p, non_acgt_to_a) of a named dictionary case"""
    if name.startswith("arun"):               # (a) an A run: every byte of it ends a level-2 phrase (dr_trigger("AAAA") % 16 == 0)
        return flanked(b"A" * int(name[4:])), 10, 100, False
    if name.startswith("ngap"):               # (a) the same run as an N gap through --non-acgt-to-a
        return flanked(b"N" * int(name[4:])), 10, 100, True
    if name.startswith("unit"):               # (b) a periodic stretch of 3000 bases whose windows trigger at p2
        p2 = int(name[4:])
        return flanked(periodic_unit(p2) * (3000 // len(periodic_unit(p2)))), 10, 100, False
    if name.startswith("long"):               # (c) longest level-2 phrase of exactly 1024 / 1025 bytes
        return long_phrase_records(int(name[4:])), 10, 100, False
    raise KeyError(name)


DICT_CODE = r'''
import sys
sys.path.insert(0, sys.argv[1] + "/tests")
from pfp_testlib import EMU_SO, compare, engine_run, oracle_run
from test_level2_limits import dict_case
import pfbwt_hip
lib = EMU_SO if sys.argv[2] == "emu" else None
if lib is None: assert pfbwt_hip.load_library().pfp_backend().decode() == "hip-gfx950"
seqs, w, p, ntoa = dict_case(sys.argv[3])
ref = oracle_run(seqs, w=w, p=p, U=8, non_acgt_to_a=ntoa)
res = engine_run(lambda **kw: pfbwt_hip.PfpContext(lib=lib, **kw), seqs, w, p, 8, non_acgt_to_a=ntoa)
bad = compare(res, ref, 8)
assert not bad, bad
print("case ok")
'''


def run_case(code, kind, arg, env):
    e = dict(os.environ); e.update(env); e["PFP_TEST_HOOKS"] = "1"; e["PFP_VERBOSE"] = "1"
    if kind == "emu":
        subprocess.run(["make", "-C", os.path.join(ROOT, "pfbwt-f_amd"), "emu"], check=True, stdout=subprocess.DEVNULL)
        e["PFP_EMU_POISON"] = "1"      # fresh device memory holds garbage, as on the card
    pr = subprocess.run([sys.executable, "-c", code, ROOT, kind, arg], env=e, capture_output=True, text=True, timeout=1500)
    assert pr.returncode == 0 and "case ok" in pr.stdout, pr.stdout[-1500:] + pr.stderr[-3000:]
    return pr.stderr


def assert_dict_route(log, route, longest=None):
    """route: "taken" (assembled; `longest` = its longest level-2 phrase), "long ties" (taken, and neighbour pairs of P2 equal beyond
    the first pass were resolved by doubling), "given up" (a level-2 phrase of `longest` bytes), "old" (the route was never tried)"""
    started = [l for l in log.splitlines() if "recursive dictionary sort:" in l]
    assembled = "dictionary assembled" in log
    if route == "old":
        assert "recursive dictionary sort" not in log, log[-2000:]
    elif route == "given up":
        assert "recursive dictionary sort given up: a level-2 phrase of %d bytes" % longest in log and not assembled, log[-2000:]
    else:
        assert len(started) == 1 and assembled, log[-2000:]
        if longest is not None:
            assert "(longest %d)" % longest in started[0], started[0]
        ties = [l for l in log.splitlines() if "P2 tie classes:" in l]
        assert bool(ties) == (route == "long ties"), ties or log[-2000:]


# (name, switches, route, longest level-2 phrase)
DICT_CASES = [
    ("arun70000", {"PFP_DICT_REC": "1"}, "long ties", None),      # shared by three words: more than 65 536 level-2 phrases
    ("arun65540", {"PFP_DICT_REC": "1"}, "long ties", None),
    ("arun65530", {"PFP_DICT_REC": "1"}, "long ties", None),
    ("arun70000", {"PFP_DICT_REC": "0"}, "old", None),            # the control: the old dictionary sorter
    ("ngap70000", {"PFP_DICT_REC": "1"}, "long ties", None),
    ("unit16", {"PFP_DICT_REC": "1"}, "long ties", None),
    ("unit5", {"PFP_DICT_REC": "1", "PFP_DICT_REC_P2": "5"}, "long ties", None),
    ("long1024", {"PFP_DICT_REC": "1"}, "taken", 1024),
    ("long1025", {"PFP_DICT_REC": "1"}, "given up", 1025),
]
EMU_DICT_CASES = [c for c in DICT_CASES if c[0] not in ("arun65530", "ngap70000")]
CASE_ID = lambda c: "%s,%s" % (c[0], ",".join("%s=%s" % (k.replace("PFP_", ""), v) for k, v in c[1].items()))


@pytest.mark.parametrize("case", EMU_DICT_CASES, ids=CASE_ID)
def test_dictionary_sort_limits_emu(case):
    name, env, route, longest = case
    assert_dict_route(run_case(DICT_CODE, "emu", name, env), route, longest)


@pytest.mark.gpu
@pytest.mark.parametrize("case", DICT_CASES, ids=CASE_ID)
def test_dictionary_sort_limits_gpu(case):
    name, env, route, longest = case
    assert_dict_route(run_case(DICT_CODE, "gpu", name, env), route, longest)


AUTO_CODE = r'''
import hashlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import bench
import pfbwt_hip
from test_level2_limits import flanked
assert pfbwt_hip.load_library().pfp_backend().decode() == "hip-gfx950"
panel = bench.synth_seqs(1_500_000, 30, 1000, (0, 0, 0, 0))
gaps = flanked(b"N" * 70000)
# the oracle reads each gap as the A run --non-acgt-to-a makes of it
_, dig = bench.cpu_baseline(panel + [np.frombuffer(s.replace(b"N", b"A"), np.uint8) for s in gaps], 10, 100, True, mode=("-s", "-r"))
c = pfbwt_hip.PfpContext(w=10, p=100, u64=True, sai=True, non_acgt_to_a=True)
for s in panel + gaps:
    c.feed(s, True)
sz = c.finalize(); c.parse_bwt(); c.bwt_build(sa=True, rssa=True)
assert sz.dsize >= (1 << 22) and sz.dsize * 8 <= sz.n, (sz.dsize, sz.n)      # the window of the automatic choice
o = c.bwt_get()
for k in ("bwt", "sa", "ssa", "esa"):
    assert hashlib.sha256(o[k].tobytes()).hexdigest() == dig[k], k
c.close()
print("case ok")
'''


@pytest.mark.gpu
def test_dictionary_sort_default_route_gpu():
    """(e) a collection whose dictionary takes the recursive sort with the DEFAULT switches (at least 4 MiB, at most n / 8): 30 x 1.5
    Mbase of the synthetic panel and the three records of case (a) with 70 kbp N gaps through --non-acgt-to-a.  .bwt .sa .ssa .esa ==
    oracle/pfbwt_oracle by sha256; the log shows the route, taken by itself, and the long ties it resolved"""
    e = dict(os.environ); e["PFP_VERBOSE"] = "1"; e.pop("PFP_TEST_HOOKS", None)
    pr = subprocess.run([sys.executable, "-c", AUTO_CODE, ROOT], env=e, capture_output=True, text=True, timeout=1500)
    assert pr.returncode == 0 and "case ok" in pr.stdout, pr.stdout[-1500:] + pr.stderr[-3000:]
    assert_dict_route(pr.stderr, "long ties")


def test_level2_restatements():
    """the restated triggers pick what the cases need: AAAA ends a level-2 phrase at p2 = 16 and an A run stays inside one word of the
    text-level parse, the periodic units trigger, the homopolymer base does not"""
    assert dr_window_triggers(b"AAAA") and not text_trigger(b"A" * 10, 100)
    assert dr_window_triggers(b"GAGA", 5)
    for p2 in (16, 5):
        u = periodic_unit(p2)
        assert any(dr_window_triggers((u * 4)[i:i + 4], p2) for i in range(len(u)))
    b = homopolymer_base()
    assert not dr_window_triggers(bytes([b]) * 4)


def rec_case(plen, seed=9):
    """an integer string (alphabet 400, p2 = 4) whose longest level-2 phrase has exactly `plen` symbols: two triggers with plen - 2
    symbols between them that do not trigger, in six copies with random context in front and one shared tail behind, so that equal
    suffixes share more than plen + 1 symbols; one copy differs in the symbol before its last trigger"""
    k = 400
    trig = [v for v in range(1, k) if mix32(v) % 4 == 0]
    non = [v for v in range(1, k) if mix32(v) % 4 != 0]
    rng = np.random.default_rng(seed)
    body = np.array([trig[0]] + list(rng.choice(non, plen - 2)) + [trig[1]], np.uint32)
    other = body.copy(); other[-2] = non[0] if body[-2] != non[0] else non[1]
    tail = rng.integers(1, k, 40).astype(np.uint32)
    parts = []
    for c in range(6):
        parts += [rng.integers(1, k, 50).astype(np.uint32), other if c == 3 else body, tail]
    return np.concatenate(parts + [np.zeros(1, np.uint32)]), k


REC_CODE = r'''
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[1] + "/tests")
from pfp_testlib import oracle, EMU_SO
from test_level2_limits import rec_case
import pfbwt_hip
lib = EMU_SO if sys.argv[2] == "emu" else None
if lib is None: assert pfbwt_hip.load_library().pfp_backend().decode() == "hip-gfx950"
s, k = rec_case(int(sys.argv[3]))
SA, rounds = pfbwt_hip.sacak_int(s, k, lib=lib)
want = np.zeros(len(s), np.uint64)
assert oracle().orc_sais_int(s.ctypes.data_as(C.c_void_p), want.ctypes.data_as(C.c_void_p), len(s), k) == 0
assert np.array_equal(SA.astype(np.uint64), want)
print("case ok")
'''


def assert_rec_route(log, plen):
    if plen <= 1024:
        assert any("recursive parse sort (depth 0):" in l and "(longest %d)" % plen in l for l in log.splitlines()), log[-2000:]
        assert "assembled:" in log, log[-2000:]
    else:
        assert "recursive parse sort given up: a level-2 phrase of %d symbols" % plen in log, log[-2000:]
        assert "recursive parse sort (depth 0)" not in log, log[-2000:]


@pytest.mark.parametrize("plen", [1024, 1025])
def test_parse_sort_phrase_limit_emu(plen):
    """(d) REC_MAX_PHRASE through the sacak_int drop-in: route taken at 1024 symbols, given up at 1025; SA == SA-IS either way"""
    assert_rec_route(run_case(REC_CODE, "emu", str(plen), {"PFP_PARSE_REC": "1"}), plen)


@pytest.mark.gpu
@pytest.mark.parametrize("plen", [1024, 1025])
def test_parse_sort_phrase_limit_gpu(plen):
    assert_rec_route(run_case(REC_CODE, "gpu", str(plen), {"PFP_PARSE_REC": "1"}), plen)
