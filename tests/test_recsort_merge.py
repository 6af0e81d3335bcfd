"""The assembly of the recursive parse sort with its inverted lists read off SA(P2) and the rows of a class merged
(pfbwt-f_amd/csrc/recsort.h: k_rs_slice_payload, k_rs_merge; PFP_PARSE_REC_MERGE=1, the default) against the route it replaces
(PFP_PARSE_REC_MERGE=0: lists by a sort by word, rows by the LDS sort of k_rs_assemble), the new lists under the old sort
(PFP_PARSE_REC_MERGE=2) and the oracle's SA-IS.  The
keys of a class are distinct, so both routes must give the same array, element by element.  Through the sacak_int drop-in and
through the whole pipeline; CPU: tests/emu with poisoned memory, GPU: the product library.  Every run says on stderr
(PFP_VERBOSE) which route assembled it: a run that asked for the merge and silently took the old route fails."""
import os
import re
import subprocess
import sys
import pytest
from pfp_testlib import ROOT
from test_recsort import PIPE_CODE

CODE = r'''
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1] + "/tests")
from pfp_testlib import oracle, EMU_SO
import pfbwt_hip
lib = EMU_SO if sys.argv[2] == "emu" else None
if lib is None: assert pfbwt_hip.load_library().pfp_backend().decode() == "hip-gfx950"
def check(s, k, tag):
    want = np.zeros(len(s), np.uint64)
    assert oracle().orc_sais_int(s.ctypes.data_as(C.c_void_p), want.ctypes.data_as(C.c_void_p), len(s), k) == 0
    got = {}
    for merge in ("0", "1", "2"):
        os.environ["PFP_PARSE_REC_MERGE"] = merge          # read by the context that sacak_int creates
        sys.stderr.write("\n@case %s merge=%s\n" % (tag, merge)); sys.stderr.flush()
        got[merge], rounds = pfbwt_hip.sacak_int(s, k, lib=lib)
        assert np.array_equal(got[merge].astype(np.uint64), want), (tag, merge, len(s), k)
    assert np.array_equal(got["0"], got["1"]) and np.array_equal(got["0"], got["2"]), tag
rng = np.random.default_rng(int(sys.argv[3]))
def panel(L, H, sigma, mut):
    base = rng.integers(1, sigma, L).astype(np.uint32); rows = []
    for h in range(H):
        r = base.copy(); m = rng.random(L) < mut; r[m] = rng.integers(1, sigma, int(m.sum())); rows.append(r)
    return np.concatenate(rows + [np.zeros(1, np.uint32)])
for (L, H, sigma, mut) in ((40, 100, 9, 0.03), (300, 20, 50, 0.02), (2000, 8, 5, 0.01), (50, 4, 20, 0.05)):
    check(panel(L, H, sigma, mut), sigma, "panel-%d-%d-%d" % (L, H, sigma))
for n, k in ((1000, 5), (3000, 2)):
    s = rng.integers(1, k, n).astype(np.uint32); s[-1] = 0; check(s, k, "random-%d-%d" % (n, k))
check(np.concatenate([np.tile(np.array([3, 1, 2], np.uint32), 500), [0]]).astype(np.uint32), 4, "periodic")
check(np.concatenate([np.full(900, 7, np.uint32), rng.integers(1, 9, 300).astype(np.uint32), np.full(1500, 7, np.uint32), [0]]).astype(np.uint32), 9, "runs")
print("merge ok")
'''

# on top of PFP_PARSE_REC=1; what the log of the merged runs must show at least once: "merged" = k_rs_merge assembled a level,
# "global" = a class with more rows than a batch went through the global sort, "sorted" = k_rs_merge handed a batch to the LDS sort
ENVS = [
    ({}, ("merged",)),
    ({"PFP_PARSE_REC_P2": "2"}, ("merged",)),
    ({"PFP_PARSE_REC_P2": "7"}, ("merged",)),
    ({"PFP_PARSE_REC_TILE_ROWS": "5"}, ("merged", "global")),
    ({"PFP_PARSE_REC_TILE_ROWS": "40"}, ("merged", "global")),
    ({"PFP_PARSE_REC_MERGE_MEMBERS": "2"}, ("merged", "sorted")),
    ({"PFP_PARSE_REC_DEPTH": "3"}, ("merged",)),
]
IDS = [",".join("%s=%s" % (k.replace("PFP_PARSE_REC_", ""), v) for k, v in e.items()) or "default" for e, _ in ENVS]
ROUTE = {"0": "lists sorted by word, rows sorted in LDS", "1": "lists from SA(P2) slices, rows merged", "2": "lists from SA(P2) slices, rows sorted in LDS"}


def routes_of(stderr):
    """[(case tag, merge flag, log of that sort)]"""
    parts = re.split(r"^@case (\S+) merge=([012])$", stderr, flags=re.M)
    return [(parts[i], parts[i + 1], parts[i + 2]) for i in range(1, len(parts) - 2, 3)]


def run_cases(kind, env, must, seed=7):
    e = dict(os.environ); e.update(env); e["PFP_PARSE_REC"] = "1"; e["PFP_TEST_HOOKS"] = "1"; e["PFP_VERBOSE"] = "1"
    if kind == "emu":
        e["PFP_EMU_POISON"] = "1"      # fresh device memory holds garbage, as on the card
    pr = subprocess.run([sys.executable, "-c", CODE, ROOT, kind, str(seed)], env=e, capture_output=True, text=True, timeout=1500)
    assert pr.returncode == 0 and "merge ok" in pr.stdout, pr.stdout[-1500:] + pr.stderr[-3000:]
    seen, levels = set(), {}
    for tag, merge, log in routes_of(pr.stderr):
        lines = [l for l in log.splitlines() if "assembled:" in l]
        for l in lines:      # every level of the recursion assembles by the route that was asked for
            assert ROUTE[merge] in l, (tag, merge, l)
        if merge == "1" and lines:
            seen.add("merged")
            if "through the global sort" in log: seen.add("global")
            if any(int(re.search(r"(\d+) batches with a class of more than", l).group(1)) > 0 for l in lines): seen.add("sorted")
        levels.setdefault(tag, set()).add(len(lines))
    assert all(len(v) == 1 for v in levels.values()), levels      # a string that takes the route takes it, as deep, whichever way it is assembled
    assert seen >= set(must), (seen, must)


@pytest.mark.parametrize("env,must", ENVS, ids=IDS)
def test_merge_assembly_emu(env, must):
    subprocess.run(["make", "-C", os.path.join(ROOT, "pfbwt-f_amd"), "emu"], check=True, stdout=subprocess.DEVNULL)
    run_cases("emu", env, must)


@pytest.mark.gpu
@pytest.mark.parametrize("env,must", ENVS, ids=IDS)
def test_merge_assembly_gpu(env, must):
    run_cases("gpu", env, must)


def run_pipeline(kind, merge, names):
    e = dict(os.environ); e.update({"PFP_PARSE_REC": "1", "PFP_PARSE_REC_MERGE": merge, "PFP_TEST_HOOKS": "1", "PFP_VERBOSE": "1"})
    if kind == "emu":
        e["PFP_EMU_POISON"] = "1"
    pr = subprocess.run([sys.executable, "-c", PIPE_CODE, ROOT, kind] + names, env=e, capture_output=True, text=True, timeout=1500)
    assert pr.returncode == 0 and "pipeline ok" in pr.stdout, pr.stdout[-1500:] + pr.stderr[-3000:]
    lines = [l for l in pr.stderr.splitlines() if "assembled:" in l]
    assert lines and all(ROUTE[merge] in l for l in lines), lines[:3]


@pytest.mark.parametrize("merge", ["0", "1"])
def test_pipeline_with_merge_assembly_emu(merge):
    """whole build (parse -> parse BWT through the recursive sort -> BWT + SA + samples), U = 8 and 4 == oracle == the reference's file digests"""
    run_pipeline("emu", merge, ["w4p7", "mult_chroms_fa", "edge"])


@pytest.mark.gpu
@pytest.mark.parametrize("merge", ["0", "1"])
def test_pipeline_with_merge_assembly_gpu(merge):
    run_pipeline("gpu", merge, ["w4p7", "mult_chroms_fa", "edge", "panel8"])
