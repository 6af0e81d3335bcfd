"""Variant-panel feed (include/pfbwt_hip.h: pfp_parse_feed_panel; csrc/panel.h, csrc/panel_host.h).

Expected values never come from the engine: model_panel() restates "kept sites" and "record" of the header in plain Python on
bytes.  test_model_reproduces_reference_goldens pins that model to texts the reference wrote from VCFs.
* text parity: the bytes of the text after feed_panel == the model's; parse and BWT == those of a context fed the model's records;
* the smallest shapes that can break the kernels, each with the defaults, panel_tile 1 / 2 / 64 and the smallest output tile;
* info counters, document names and starts, doc_array of a panel build; every error code, with the context intact afterwards.
Every check runs on the emulated library (_emu) and, grouped, on the card (@pytest.mark.gpu)."""
import ctypes as C
import gzip
import hashlib
import os
import subprocess
import numpy as np
import pytest
from pfp_testlib import EMU_SO, GOLDEN, ROOT, fasta_records

import pfbwt_hip

VCFPRE = os.path.join(GOLDEN, "vcf_")      # tests/golden/vcf_<name>: plain files, because every directory there is a fixture case
SWITCHES = ({}, {"panel_tile": 1}, {"panel_tile": 2}, {"panel_tile": 64}, {"panel_out_bytes": 256}, {"panel_swizzle": 0, "panel_tile": 2, "panel_out_bytes": 256})


# ---- the model ---------------------------------------------------------------------------------------------------------------
class Panel:
    """contigs: list of bytes; sites: per contig a list of (pos, span, [alt bytes, ...]); gt: (nsites, nhap) uint8"""

    def __init__(self, contigs, sites, gt, nhap, contig_names=None, hap_names=None):
        self.contigs, self.sites, self.nhap = contigs, sites, nhap
        self.nsites = sum(len(s) for s in sites)
        self.gt = np.asarray(gt, np.uint8).reshape(self.nsites, nhap)
        self.contig_names, self.hap_names = contig_names, hap_names

    def arrays(self):
        flat = [s for ss in self.sites for s in ss]
        alts = [a for s in flat for a in s[2]]
        return dict(ref=b"".join(self.contigs), ref_off=np.cumsum([0] + [len(c) for c in self.contigs]), site_first=np.cumsum([0] + [len(s) for s in self.sites]),
                    pos=np.array([s[0] for s in flat], np.uint64), span=np.array([s[1] for s in flat], np.uint32),
                    allele_first=np.cumsum([0] + [len(s[2]) for s in flat]), alt_off=np.cumsum([0] + [len(a) for a in alts]), alt_bytes=b"".join(alts),
                    gt=self.gt, nhap=self.nhap, contig_names=self.contig_names, hap_names=self.hap_names)


def model_panel(p, ref_first):
    """records (bytes, without their pads) in output order, their names, and the counters of pfp_panel_info that do not depend on w"""
    keep, v, skipped = [], 0, 0
    for ss in p.sites:
        end, k = 0, []
        for pos, span, alts in ss:
            if pos >= end:
                k.append((v, pos, span, alts)); end = pos + span
            else:
                skipped += 1
            v += 1
        keep.append(k)
    applied = 0

    def record(c, h):
        nonlocal applied
        ref, out, cur = p.contigs[c], [], 0
        for v, pos, span, alts in keep[c]:
            g = 0 if h is None else int(p.gt[v, h])
            out.append(ref[cur:pos]); out.append(ref[pos:pos + span] if g == 0 else alts[g - 1]); cur = pos + span
            applied += g > 0
        out.append(ref[cur:])
        return b"".join(out)
    cname = lambda c: p.contig_names[c] if p.contig_names else "c%d" % c
    hname = lambda h: p.hap_names[h] if p.hap_names else "h%d" % h
    recs, names = [], []
    for h in ([None] if ref_first else []) + list(range(p.nhap)):
        for c in range(len(p.contigs)):
            recs.append(record(c, h)); names.append(cname(c) if h is None else hname(h) + "." + cname(c))
    info = dict(contigs=len(p.contigs), haplotypes=p.nhap, records=len(recs), sites=p.nsites, kept=sum(len(k) for k in keep), skipped_overlap=skipped, alt_applied=applied,
                min_record=min((len(r) for r in recs), default=0), max_record=max((len(r) for r in recs), default=0))
    return recs, names, info


def text_of(recs, w):
    return b"".join(r + b"A" * w for r in recs)


def read_vcf(fa, vcf):
    """the reader's rules restated for the fixtures: diploid samples, s.0 / s.1, '.' = 0, a haploid call serves both"""
    recs = fasta_records(fa)
    idx = {n: i for i, (n, _) in enumerate(recs)}
    sites = [[] for _ in recs]; rows = [[] for _ in recs]; samples = []
    for line in gzip.open(vcf, "rt") if vcf.endswith(".gz") else open(vcf):
        f = line.rstrip("\n").split("\t")
        if line.startswith("##"):
            continue
        if line.startswith("#"):
            samples = f[9:]; continue
        c = idx[f[0]]; pos = int(f[1]) - 1; alts = [a.encode() for a in f[4].split(",")]
        assert recs[c][1][pos:pos + len(f[3])].upper() == f[3].upper().encode()
        row = []
        for s in f[9:]:
            g = [0 if x in (".", "") else int(x) for x in s.split(":")[0].replace("/", "|").split("|")]
            row += g * 2 if len(g) == 1 else g
        sites[c].append((pos, len(f[3]), alts)); rows[c].append(row)
    gt = np.array([r for rr in rows for r in rr], np.uint8).reshape(-1, 2 * len(samples))
    return Panel([s for _, s in recs], sites, gt, 2 * len(samples), [n for n, _ in recs], ["%s.%d" % (s, k) for s in samples for k in (0, 1)])


def test_model_reproduces_reference_goldens():
    """needs no engine: the model on the reference's own VCF inputs == the texts whose .bwt / .sa the reference wrote"""
    for case, n in (("single_chrom", 110110), ("mult_chroms", 330330)):
        p = read_vcf(VCFPRE + case + ".fa", VCFPRE + case + ".vcf.gz")
        text = text_of(model_panel(p, True)[0], 10)
        gold = fasta_records(os.path.join(GOLDEN, case, "input.fa"))
        assert len(gold) == 1 and len(text) == n and text == gold[0][1] + b"A" * 10, case
    p = read_vcf(VCFPRE + "mult_chroms_indels.fa", VCFPRE + "mult_chroms_indels.vcf.gz")
    recs, names, info = model_panel(p, True)
    assert len(text_of(recs, 10)) == 90120 and info["skipped_overlap"] == 0 and names[:2] == ["seq1", "seq2"] and names[3] == "sample0.0.seq1"


# ---- panels ------------------------------------------------------------------------------------------------------------------
def rnd(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(list(alphabet), int(n)).astype(np.uint8))


def seeded_panel(seed, lens, nhap, nsites, max_alt=3, indel=0.3, maxlen=12, alphabet=b"ACGT", overlap=0.1):
    """positions ascend inside a contig; some sites overlap or repeat a position (skipped), some are pure insertions or deletions"""
    rng = np.random.default_rng(seed)
    contigs = [rnd(rng, n, alphabet) for n in lens]
    sites = []
    for c, ref in enumerate(contigs):
        k = int(nsites[c]); ss = []
        pos = np.sort(rng.integers(0, len(ref) + 1, k)) if len(ref) or k == 0 else np.zeros(k, np.int64)
        for q in pos:
            q = int(q)
            if ss and rng.random() < overlap:
                q = ss[-1][0]
            span = 0 if q == len(ref) or rng.random() < indel / 3 else min(len(ref) - q, 1 if rng.random() > indel else int(rng.integers(1, maxlen)))
            alts = [rnd(rng, 0 if rng.random() < indel / 3 else (max(span, 1) if rng.random() > indel else int(rng.integers(0, maxlen))), alphabet) for _ in range(int(rng.integers(1, max_alt + 1)))]
            ss.append((q, span, alts))
        sites.append(ss)
    flat = [s for ss in sites for s in ss]
    gt = np.array([[int(rng.integers(0, len(s[2]) + 1)) if rng.random() < 0.4 else 0 for _ in range(nhap)] for s in flat], np.uint8).reshape(len(flat), nhap)
    return Panel(contigs, sites, gt, nhap)


def named_panels():
    rng = np.random.default_rng(77)
    r200 = rnd(rng, 200); r40 = rnd(rng, 40)
    every = [(i, 1, [bytes([b"ACGT"[(b"ACGT".index(bytes([r200[i]])) + 1) % 4]])]) for i in range(200)]
    multi = [(10 * i, 1, [bytes([65 + (a % 26)]) * (1 + a % 3) for a in range(255)]) for i in range(4)]
    out = {
        "no_sites": Panel([r200, r40], [[], []], np.zeros((0, 3)), 3),
        "one_contig_without_sites": Panel([r40, r200], [[], [(5, 1, [b"T"]), (100, 2, [b"", b"GGG"])]], [[1, 0, 1], [2, 1, 0]], 3),
        "empty_contig": Panel([b"", r40, b""], [[], [(3, 1, [b"C"])], [(0, 0, [b"ACGT"])]], [[1, 0], [0, 1]], 2),
        "short_contig": Panel([b"ACGTA", r40[:15]], [[(4, 1, [b"TT"])], [(0, 15, [b"G"])]], [[1, 0, 1, 1], [0, 1, 0, 1]], 4),
        "first_and_last_byte": Panel([r200], [[(0, 1, [b"N"]), (197, 3, [b"ac"])]], [[1, 0, 1], [1, 1, 0]], 3),
        "pure_insertions": Panel([r40], [[(0, 0, [b"TTT"]), (7, 0, [b"A"]), (7, 0, [b"CC", b"G"]), (40, 0, [b"GATTACA"])]], [[1, 0], [1, 1], [2, 1], [1, 0]], 2),
        "adjacent": Panel([r200], [[(10, 5, [b"A"]), (15, 5, [b""]), (20, 1, [b"TTTTTTTT"]), (21, 0, [b"C"])]], np.ones((4, 5)), 5),
        "overlaps_and_duplicates": Panel([r200], [[(10, 5, [b"A"]), (12, 1, [b"C"]), (14, 3, [b"G"]), (15, 1, [b"T"]), (15, 1, [b"A"]), (15, 0, [b"GG"]), (16, 2, [b"A"])]], np.ones((7, 3)), 3),
        "snp_at_every_base": Panel([r200], [every], (np.arange(200 * 6).reshape(200, 6) % 3 == 0), 6),
        "multi_allelic_255": Panel([r40], [multi], [[255, 0, 1, 128], [254, 255, 2, 0], [0, 0, 0, 0], [7, 77, 177, 255]], 4),
        "deletion_empties_contig": Panel([r40, r200], [[(0, 40, [b""])], [(0, 200, [b"", b"AC"])]], [[1, 0, 1], [1, 2, 0]], 3),
        "insertion_5000": Panel([r200], [[(50, 1, [rnd(rng, 5000)]), (120, 2, [rnd(rng, 700)])]], [[1, 0, 1], [0, 1, 1]], 3),
        "no_haplotypes": Panel([r200, r40], [[(5, 1, [b"T"])], []], np.zeros((1, 0)), 0),
    }
    # alleles that straddle 16-byte and tile borders of the output: insertions of 1 .. 40 bytes every 13 bases
    out["straddle"] = Panel([rnd(rng, 700)], [[(13 * i, i % 3, [rnd(rng, 1 + (i * 7) % 40)]) for i in range(50)]], (np.arange(50 * 9).reshape(50, 9) % 2), 9)
    return out


def seeded_panels():
    return {
        "long_contig": seeded_panel(1, [40000], 3, [300]),
        "many_haplotypes": seeded_panel(2, [2000, 5, 900], 70, [150, 2, 60]),
        "many_sites": seeded_panel(3, [3000], 4, [3000], indel=0.1),
        "three_contigs": seeded_panel(4, [1200, 17, 333], 7, [90, 5, 200], max_alt=5, alphabet=b"ACGTNacgt"),
    }


# ---- checks ------------------------------------------------------------------------------------------------------------------
def feed_and_compare(ctx, p, w, ref_first, tag, base=b"", docs_before=()):
    recs, names, minfo = model_panel(p, ref_first)
    info = ctx.feed_panel(ref_first=ref_first, records=True, **p.arrays())
    want = base + text_of(recs, w)
    assert ctx.text_length() == len(want), tag
    got = ctx.text_get()
    assert got == want, (tag, next(i for i in range(len(want)) if got[i] != want[i]))
    minfo["bases"] = len(want) - len(base)
    assert info == minfo, (tag, info, minfo)
    starts = np.cumsum([len(base)] + [len(r) + w for r in recs])[:-1].tolist()
    assert ctx.docs() == list(docs_before) + list(zip(names, starts)), tag
    return recs, starts


def check_shapes(factory, panels, switches=SWITCHES):
    residues = set()
    for name, p in panels.items():
        for sw in switches:
            for ref_first in (True, False):
                ctx = factory(w=10 if ref_first else 3, p=50, u64=True)
                ctx.debug_set(**sw)
                _, starts = feed_and_compare(ctx, p, 10 if ref_first else 3, ref_first, (name, sw, ref_first))
                residues |= {s % 16 for s in starts}
                ctx.close()
    return residues


def check_appended(factory):
    """a feed record in front, one behind; two panels in a row; a panel after a pending device view"""
    ps = named_panels()
    a, b = ps["straddle"], ps["pure_insertions"]
    for w, sw in ((7, {}), (4, {"panel_tile": 2, "panel_out_bytes": 256})):
        ctx = factory(w=w, p=50, u64=True); ctx.debug_set(**sw)
        ctx.feed(b"ACGTTGCA" * 5 + b"C", True)
        base = b"ACGTTGCA" * 5 + b"C" + b"A" * w
        recs_a, starts_a = feed_and_compare(ctx, a, w, True, "after a record", base=base)
        base += text_of(recs_a, w)
        names_a = model_panel(a, True)[1]
        recs_b, _ = feed_and_compare(ctx, b, w, False, "second panel", base=base, docs_before=list(zip(names_a, starts_a)))
        base += text_of(recs_b, w)
        ctx.feed(b"GGGTTT", True)
        assert ctx.text_get() == base + b"GGGTTT" + b"A" * w
        ctx.close()
    # the view: rows of a second context's text (device memory), pending until the panel flushes it
    owner = factory(w=2, p=50, u64=True)
    rows = [rnd(np.random.default_rng(k), 30) for k in range(4)]
    for r in rows:
        owner.feed(r, True)
    ptr, n = C.c_void_p(), C.c_uint64()
    owner._check(owner.L.pfp_text_view(owner.h, C.byref(ptr), C.byref(n)))
    ctx = factory(w=5, p=50, u64=True)
    ctx.feed_device_view(ptr.value, 4, 30, 32)
    feed_and_compare(ctx, a, 5, True, "after a view", base=text_of(rows, 5))
    ctx.close(); owner.close()


def pipeline(ctx):
    sz = ctx.finalize(); out = {"n": sz.n, "m": sz.m}
    out.update(ctx.parse_get()); ctx.parse_bwt(); b = ctx.bwt_build(sa=True, rssa=True); out.update(ctx.bwt_get()); out["r"] = b.r
    return out


def check_pipeline_parity(factory):
    """finalize + parse_bwt + bwt_build on a panel feed == the same on the model's records through pfp_parse_feed; doc_array of the
    panel build == the model's record of every SA value"""
    p = seeded_panel(9, [1500, 400], 6, [120, 40], alphabet=b"ACGTNacgtn", max_alt=4)
    q = seeded_panel(10, [1500, 400], 6, [120, 40], alphabet=b"ACGTRYacgtNn", max_alt=4)
    for U in (4, 8):
        for w in (4, 10):
            for ntoa, pan in ((False, p), (True, q)):
                recs, _, _ = model_panel(pan, True)
                a = factory(w=w, p=11, u64=(U == 8), non_acgt_to_a=ntoa, sai=True)
                a.feed_panel(ref_first=True, records=True, **pan.arrays())
                b = factory(w=w, p=11, u64=(U == 8), non_acgt_to_a=ntoa, sai=True)
                for r in recs:
                    b.feed(r, True)
                ra, rb = pipeline(a), pipeline(b)
                for k in rb:
                    assert np.array_equal(np.asarray(ra[k]), np.asarray(rb[k])), (U, w, ntoa, k)
                starts = np.array([s for _, s in a.docs()], np.uint64)
                assert starts.tolist() == pfbwt_hip.doc_starts([len(r) for r in recs], w).tolist()
                da = a.doc_array(starts, rows=True, runs=False)[0]
                assert np.array_equal(np.asarray(da, np.uint64), (np.searchsorted(starts, np.asarray(rb["sa"], np.uint64), side="right") - 1).astype(np.uint64))
                a.close(); b.close()


def check_errors(factory):
    E_ARG, E_BIG, E_NOMEM = pfbwt_hip.E_ARG, pfbwt_hip.E_TOO_LARGE, pfbwt_hip.E_NOMEM
    good = named_panels()["adjacent"]
    w = 6

    def fresh():
        ctx = factory(w=w, p=50, u64=False)
        ctx.feed(b"ACGTACGTAC", True)
        ctx.feed_panel(ref_first=False, records=True, **named_panels()["short_contig"].arrays())
        return ctx, ctx.text_get(), ctx.docs()

    def intact(ctx, text, docs, tag):
        """text, documents and a following feed + finalize as without the failed call"""
        assert ctx.text_length() == len(text) and ctx.text_get() == text and ctx.docs() == docs, tag
        ctx.feed(b"TTGACCA", True)
        other = factory(w=w, p=50, u64=False)
        other.feed(text, False); other.feed(b"TTGACCA", True)
        assert other.text_get() == ctx.text_get(), tag
        sa, sb = ctx.finalize(), other.finalize()
        assert (sa.n, sa.m, sa.dwords, sa.dsize) == (sb.n, sb.m, sb.dwords, sb.dsize), tag
        ga, gb = ctx.parse_get(), other.parse_get()
        assert all(np.array_equal(ga[k], gb[k]) for k in ("dict", "parse", "last")), tag
        other.close()

    def fails(ctx, arr, flags=None, **kw):
        with pytest.raises(pfbwt_hip.PfpError) as e:
            ctx.feed_panel(flags=flags, **dict(arr, **kw))
        return e.value

    base = good.arrays()
    bad_args = {
        "ref NULL": dict(ref=b""), "ref_off NULL": dict(ref_off=None), "site_first NULL": dict(site_first=None), "pos NULL": dict(pos=None), "span NULL": dict(span=None),
        "allele_first NULL": dict(allele_first=None), "alt_off NULL": dict(alt_off=None), "alt_bytes NULL": dict(alt_bytes=b""), "gt NULL": dict(gt=None),
        "ref_off descends": dict(ref_off=[200, 0]), "site_first descends": dict(site_first=[4, 0]), "site_first short": dict(site_first=[0, 3]),
        "pos descends": dict(pos=[10, 15, 14, 21]), "pos + span beyond": dict(pos=[10, 15, 20, 199], span=[5, 5, 1, 2]), "pos beyond": dict(pos=[10, 15, 20, 201]),
        "allele_first descends": dict(allele_first=[0, 2, 1, 3, 4]), "allele_first beyond nalt": dict(allele_first=[0, 1, 2, 3, 9]), "alt_off descends": dict(alt_off=[0, 1, 0, 9, 10]),
    }
    for tag, kw in bad_args.items():
        ctx, text, docs = fresh()
        assert fails(ctx, base, **kw).status == E_ARG, tag
        intact(ctx, text, docs, tag); ctx.close()
    ctx, text, docs = fresh()
    assert fails(ctx, base, flags=4).status == E_ARG and fails(ctx, base, flags=1 | 8).status == E_ARG
    # a genotype beyond the site's ALT list: found on the device, the smallest index is reported
    gt = good.gt.copy(); gt[2, 3] = 2; gt[3, 0] = 9
    e = fails(ctx, base, gt=gt)
    assert (e.status, e.pos, e.ch) == (E_ARG, 2 * 5 + 3, 2)
    intact(ctx, text, docs, "genotype"); ctx.close()
    # 2^32 or more sites / records: refused before any array is read
    ctx, text, docs = fresh()
    one = np.zeros(3, np.uint64)
    P = pfbwt_hip.Panel(); P.ncontigs = 2; P.ref_off = one.ctypes.data; P.site_first = one.ctypes.data; P.nsites = 1 << 32; P.nhap = 1
    assert ctx.L.pfp_parse_feed_panel(ctx.h, C.byref(P), 0, None) == E_BIG
    P.nsites = 0; P.nhap = 1 << 31
    assert ctx.L.pfp_parse_feed_panel(ctx.h, C.byref(P), 1, None) == E_BIG
    # the text would pass the limit of the 32-bit width: known once the lengths are (1100 haplotypes of 2^22 bases)
    big = np.full(1 << 22, 67, np.uint8)
    e = fails(ctx, dict(ref=big, ref_off=[0, big.size], site_first=[0, 0], pos=[], span=[], allele_first=[0], alt_off=[0], alt_bytes=b"", gt=None, nhap=1100))
    assert e.status == E_BIG
    intact(ctx, text, docs, "too large"); ctx.close()
    # a workspace that holds the small panels but not 48 MB of reference
    ctx = factory(w=w, p=50, u64=False, workspace_bytes=32 << 20)
    ctx.feed(b"ACGTACGTAC", True)
    ctx.feed_panel(ref_first=False, records=True, **named_panels()["short_contig"].arrays())
    text, docs = ctx.text_get(), ctx.docs()
    big = np.full(48 << 20, 71, np.uint8)
    e = fails(ctx, dict(ref=big, ref_off=[0, big.size], site_first=[0, 0], pos=[], span=[], allele_first=[0], alt_off=[0], alt_bytes=b"", gt=None, nhap=1))
    assert e.status == E_NOMEM and ctx.L.pfp_workspace_needed(ctx.h) > (48 << 20)
    intact(ctx, text, docs, "nomem"); ctx.close()
    # valid and empty: nothing is appended
    for kw, rf in ((dict(nhap=0, gt=None), False), (dict(ref=b"", ref_off=[0], site_first=[0], pos=[], span=[], allele_first=[0], alt_off=[0], alt_bytes=b"", gt=None), True)):
        ctx, text, docs = fresh()
        info = ctx.feed_panel(ref_first=rf, records=True, **dict(base, **kw))
        assert info["records"] == 0 and info["bases"] == 0
        intact(ctx, text, docs, "empty"); ctx.close()


def check_reset_after_stage(factory):
    """a context in a later stage is reset like the other feeds do"""
    p = named_panels()["straddle"]
    ctx = factory(w=4, p=7, u64=True)
    ctx.feed(rnd(np.random.default_rng(1), 500), True); ctx.finalize()
    feed_and_compare(ctx, p, 4, True, "after finalize")
    ctx.finalize(); ctx.close()


# ---- CPU: the emulated library -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pfbwt-f_amd"), "emu", "emu-host"], check=True, stdout=subprocess.DEVNULL)
    return lambda **kw: pfbwt_hip.PfpContext(lib=EMU_SO, **kw)


def test_panel_named_shapes_emu(emu):
    assert check_shapes(emu, named_panels()) == set(range(16))      # record starts at every residue mod 16


def test_panel_seeded_shapes_emu(emu):
    check_shapes(emu, seeded_panels(), switches=SWITCHES[:1] + SWITCHES[3:5])
    small = {k: v for k, v in seeded_panels().items() if k != "long_contig"}
    check_shapes(emu, small, switches=SWITCHES[1:3] + SWITCHES[5:])


def test_panel_appended_emu(emu):
    check_appended(emu)
    check_reset_after_stage(emu)


def test_panel_pipeline_parity_emu(emu):
    check_pipeline_parity(emu)


def test_panel_errors_emu(emu):
    check_errors(emu)


# ---- GPU: the product library --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_panel_shapes_gpu(gpu_ctx_factory):
    assert check_shapes(gpu_ctx_factory, named_panels()) == set(range(16))
    check_shapes(gpu_ctx_factory, seeded_panels())


@pytest.mark.gpu
def test_panel_appended_parity_errors_gpu(gpu_ctx_factory):
    check_appended(gpu_ctx_factory)
    check_reset_after_stage(gpu_ctx_factory)
    check_pipeline_parity(gpu_ctx_factory)
    check_errors(gpu_ctx_factory)


@pytest.mark.gpu
def test_panel_medium_gpu(gpu_ctx_factory):
    """64 haplotypes x 2 Mbase, a site every 50 bases: sha256 of the text and of .bwt against the model's records through pfp_parse_feed"""
    rng = np.random.default_rng(5)
    L, nhap, step = 1 << 21, 64, 50
    ref = rnd(rng, L)
    pos = np.arange(7, L - 20, step)
    kinds = rng.integers(0, 10, pos.size)
    sites = [(int(q), 1 if k else int(rng.integers(0, 4)), [rnd(rng, 1 if k else int(rng.integers(0, 6)))]) for q, k in zip(pos, kinds)]
    gt = (rng.random((pos.size, nhap)) < 0.2).astype(np.uint8)
    p = Panel([ref], [sites], gt, nhap)
    recs, _, minfo = model_panel(p, True)
    a = gpu_ctx_factory(w=10, p=100, u64=True)
    info = a.feed_panel(ref_first=True, **p.arrays())
    assert info["alt_applied"] == minfo["alt_applied"] and info["max_record"] == minfo["max_record"]
    want = text_of(recs, 10)
    assert a.text_length() == len(want) and hashlib.sha256(a.text_get()).digest() == hashlib.sha256(want).digest()
    b = gpu_ctx_factory(w=10, p=100, u64=True)
    for r in recs:
        b.feed(r, True)
    for c in (a, b):
        c.finalize(); c.parse_bwt(); c.bwt_build(sa=False, rssa=True)
    assert a.bsizes.r == b.bsizes.r and hashlib.sha256(a.bwt_get()["bwt"]).digest() == hashlib.sha256(b.bwt_get()["bwt"]).digest()
    a.close(); b.close()
