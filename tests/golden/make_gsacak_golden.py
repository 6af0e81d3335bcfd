#!/usr/bin/env python3
"""Fixture of the dictionary suffix-sort stage, made in the build container from the reference's own gsacak():
for the cases edge, w4p7, mult_chroms_fa and single_chrom, the dictionary the oracle builds (U = 8) is sorted by
oracle/_ref/libgsacak64.so (compiled from gsa/gsacak.c by `make -C oracle ref`) and its gSA and gLCP are kept, with the
sha256 of the dictionary they belong to, in tests/golden/gsacak_dict_u64.npz.  tests/test_oracle_golden.py compares the
oracle's orc_gsa_lcp with these arrays on every machine, and with the library itself where oracle/_ref is built.
usage: python3 tests/golden/make_gsacak_golden.py   (needs oracle/_ref/libgsacak64.so)"""
import ctypes as C
import hashlib
import os
import sys
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from pfp_testlib import ROOT, golden_case, oracle_run

CASES = ("edge", "w4p7", "mult_chroms_fa", "single_chrom")
g = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libgsacak64.so"))
g.gsacak.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
out = {}
for name in CASES:
    man, recs = golden_case(name)
    d = oracle_run([s for _, s in recs], w=man["w"], p=man["p"], U=8)["dict"].copy()
    SA, LCP = np.zeros(d.size, np.uint64), np.zeros(d.size, np.int64)
    g.gsacak(d.ctypes.data_as(C.c_void_p), SA.ctypes.data_as(C.c_void_p), LCP.ctypes.data_as(C.c_void_p), None, d.size)
    out[name + "_dict_sha256"] = np.frombuffer(hashlib.sha256(d.tobytes()).digest(), np.uint8)
    out[name + "_gsa"] = SA.astype("<u8")
    out[name + "_glcp"] = LCP.astype("<i8")
    print(name, "dictionary bytes", d.size)
np.savez_compressed(os.path.join(HERE, "gsacak_dict_u64.npz"), **out)
