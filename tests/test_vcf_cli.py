"""VCF reader and command line of the variant-panel feed (pfp_parse_feed_vcf_file, csrc/vcfread.h; pfbwt-f --vcf).

* `--vcf` builds of the reference's own tests/data VCFs (copied to tests/golden/vcf_*) == the .bwt / .sa the reference wrote from them
  (tests/golden/<case>/reference_golden.*), .ssa / .esa and the n: / r: lines of that case's manifest;
* mult_chroms_indels, sample subsets and orders, --vcf-no-ref, plain-text VCF: == a build fed the records of test_panel.model_panel;
* every PFP_E_CORRUPT rule from a hand-written VCF with the line number asserted; symbolic ALT lines and '.' genotypes counted;
* the refused flag combinations.
Emulator binaries (make emu-host) on the CPU, product binaries on the card."""
import gzip
import hashlib
import json
import os
import subprocess
import numpy as np
import pytest
from pfp_testlib import EMU_SO, GOLDEN, ROOT
from test_panel import Panel, VCFPRE, model_panel, read_vcf, text_of

import pfbwt_hip

EMUB = os.path.join(ROOT, "tests", "emu", "build")
BIN = os.path.join(ROOT, "pfbwt-f_amd", "bin")
E_IO = -9


def sha_f(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def run(cmd, check=True):
    pr = subprocess.run(cmd, capture_output=True, text=True)
    assert pr.returncode == 0 or not check, pr.stderr[-2000:]
    return pr


def fixture(case):
    return VCFPRE + case + ".fa", VCFPRE + case + ".vcf.gz"


def model_files(factory, recs, w, p, U):
    """.bwt / .sa / .ssa / .esa images of a build fed the model's records through pfp_parse_feed"""
    ctx = factory(w=w, p=p, u64=(U == 8), sai=True)
    for r in recs:
        ctx.feed(r, True)
    ctx.finalize(); ctx.parse_bwt(); ctx.bwt_build(sa=True, rssa=True)
    out = ctx.bwt_get(); ctx.close()
    dt = "<u8" if U == 8 else "<u4"
    return {"bwt": np.asarray(out["bwt"], np.uint8).tobytes(), "sa": np.asarray(out["sa"]).astype(dt).tobytes(), "ssa": np.asarray(out["ssa"]).astype(dt).tobytes(), "esa": np.asarray(out["esa"]).astype(dt).tobytes()}


def same_files(pref, want, tag):
    for e, img in want.items():
        assert open(pref + "." + e, "rb").read() == img, (tag, e)


def select(p, haps):
    return Panel(p.contigs, p.sites, p.gt[:, haps], len(haps), p.contig_names, [p.hap_names[h] for h in haps])


def check_reference_goldens(exe, tmp):
    for case in ("single_chrom", "mult_chroms"):
        man = json.load(open(os.path.join(GOLDEN, case, "manifest.json")))
        fa, vcf = fixture(case)
        for name, U in (("pfbwt-f64", 8), ("pfbwt-f", 4)):
            pref = os.path.join(tmp, "%s_%d" % (case, U))
            pr = run([exe[name], "-s", "-r", "--vcf", vcf, "-o", pref, fa])
            assert open(pref + ".bwt", "rb").read() == gzip.open(os.path.join(GOLDEN, case, "reference_golden.bwt.gz")).read(), (case, U)
            if U == 8:
                assert open(pref + ".sa", "rb").read() == gzip.open(os.path.join(GOLDEN, case, "reference_golden.sa.u64.gz")).read(), case
            mf = man["files"]["u%d" % (U * 8)]
            for e in ("bwt", "sa", "ssa", "esa", "n"):
                assert sha_f(pref + "." + e) == mf[e]["sha256"], (case, U, e)
            assert "n: %d\n" % man["n"] in pr.stderr and "r: %d\n" % man["r"] in pr.stderr, pr.stderr[-500:]


def check_indels_samples_plain(exe, factory, tmp):
    # indels: against the model-fed build, with the names of vcf_scan.cpp:166-170 in .docs
    fa, vcf = fixture("mult_chroms_indels")
    p = read_vcf(fa, vcf)
    recs, names, _ = model_panel(p, True)
    pref = os.path.join(tmp, "indels")
    run([exe["pfbwt-f64"], "-s", "-r", "--print-docs", "--vcf", vcf, "-o", pref, fa])
    same_files(pref, model_files(factory, recs, 10, 100, 8), "indels")
    docs = [l.split() for l in open(pref + ".docs")]
    assert [d[0] for d in docs] == names and names[:4] == ["seq1", "seq2", "seq3", "sample0.0.seq1"]
    assert [int(d[1]) for d in docs] == pfbwt_hip.doc_starts([len(r) for r in recs], 10).tolist()
    assert open(pref + ".n").read() == "90120\n"
    # --parse-only writes the parse of the same text
    run([exe["pfbwt-f64"], "--parse-only", "--vcf", vcf, "-o", pref + "_p", fa])
    for e in ("dict", "occ", "parse", "n"):
        assert sha_f(pref + "_p." + e) == sha_f(pref + "." + e), e
    # a subset of the samples in another order; without the reference; -w / -p / the 32-bit program
    fa, vcf = fixture("single_chrom")
    p = read_vcf(fa, vcf)
    samples = [h[:-2] for h in p.hap_names[::2]]
    assert len(samples) == 5
    pick = [3, 1]
    sub = select(p, [2 * s + k for s in pick for k in (0, 1)])
    pref = os.path.join(tmp, "subset")
    run([exe["pfbwt-f"], "-s", "-r", "-w", "6", "-p", "30", "--print-docs", "--vcf", vcf, "--vcf-samples", ",".join(samples[s] for s in pick), "-o", pref, fa])
    recs, names, _ = model_panel(sub, True)
    same_files(pref, model_files(factory, recs, 6, 30, 4), "subset")
    assert [l.split()[0] for l in open(pref + ".docs")] == names and names[1] == samples[3] + ".0." + p.contig_names[0]
    pref = os.path.join(tmp, "noref")
    run([exe["pfbwt-f64"], "-s", "-r", "--vcf-no-ref", "--vcf", vcf, "-o", pref, fa])
    same_files(pref, model_files(factory, model_panel(p, False)[0], 10, 100, 8), "no ref")
    # a plain-text VCF gives what the gzip one gives
    plain = os.path.join(tmp, "single_chrom.vcf")
    open(plain, "wb").write(gzip.open(vcf).read())
    pref2 = os.path.join(tmp, "noref_plain")
    run([exe["pfbwt-f64"], "-s", "-r", "--vcf-no-ref", "--vcf", plain, "-o", pref2, fa])
    for e in ("bwt", "sa", "ssa", "esa"):
        assert sha_f(pref2 + "." + e) == sha_f(pref + "." + e), e


# ---- hand-written inputs ---------------------------------------------------------------------------------------------------------
REF = ">c1 first\nACGTACGTAC\nGGTTAACC\n>c2\nTTTTCCCCGGGGAAAA\n>c3\n\n"      # c1 = ACGTACGTACGGTTAACC (18), c2 (16), c3 empty
HDR = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1\ts2\n"


def vline(chrom, pos, ref, alt, *gts, fmt="GT"):
    return "\t".join([chrom, str(pos), ".", ref, alt, ".", ".", ".", fmt] + list(gts)) + "\n"


# name -> (VCF text, 1-based line of the refusal)
MALFORMED = {
    "unknown contig": (HDR + vline("c1", 1, "A", "C", "0|1", "1|1") + vline("c9", 2, "T", "C", "0|1", "1|1"), 4),
    "contig not contiguous": (HDR + vline("c1", 1, "A", "C", "0|1", "1|1") + vline("c2", 1, "T", "C", "0|0", "0|0") + vline("c1", 5, "A", "C", "0|0", "0|0"), 5),
    "positions descend": (HDR + vline("c1", 5, "A", "C", "0|1", "1|1") + vline("c1", 4, "T", "C", "0|1", "1|1"), 4),
    "REF differs": (HDR + vline("c1", 2, "G", "C", "0|1", "1|1"), 3),
    "REF past the contig": (HDR + vline("c2", 15, "AAA", "C", "0|1", "1|1"), 3),
    "genotype beyond ALT": (HDR + vline("c1", 1, "A", "C,G", "0|2", "3|1"), 3),
    "ploidy 3": (HDR + vline("c1", 1, "A", "C", "0|1|1", "1|1"), 3),
    "256 ALTs": (HDR + vline("c1", 1, "A", ",".join(["C", "G", "T", "AA"] * 64), "0|1", "1|1"), 3),
    "short line": (HDR + vline("c1", 1, "A", "C", "0|1", "1|1") + vline("c1", 3, "G", "C", "0|1"), 4),
    "GT not first": (HDR + vline("c1", 1, "A", "C", "9:0|1", "9:1|1", fmt="DP:GT"), 3),
    "data before #CHROM": ("##fileformat=VCFv4.2\n" + vline("c1", 1, "A", "C", "0|1", "1|1"), 2),
}
# accepted: lower-case REF, '/' and haploid calls, '.' genotypes, symbolic ALT lines (dropped), an overlap (skipped), contigs in another order
GOOD = (HDR + vline("c2", 1, "tttt", "T,TTTTTT", "1/2", "2") + vline("c2", 3, "T", "<DEL>", "0|1", "1|1") + vline("c2", 4, "T", "G", "1|1", "1|1") + vline("c2", 9, "G", "*", "0|1", "0|0")
        + vline("c2", 10, "G", "C", ".|1", ".") + vline("c2", 16, "A", "AGG]c1:5]", "1|1", "1|1") + vline("c1", 18, "C", "CAT", "0|1", "./.", fmt="GT:DP") + vline("c1", 18, "C", "G", "1|1", "1|1"))


def write_inputs(tmp, name, text):
    fa = os.path.join(tmp, "ref.fa"); open(fa, "w").write(REF)
    vcf = os.path.join(tmp, name.replace(" ", "_") + ".vcf"); open(vcf, "w").write(text)
    return fa, vcf


def check_reader_rules(factory, exe, tmp):
    for name, (text, line) in MALFORMED.items():
        fa, vcf = write_inputs(tmp, name, text)
        ctx = factory(w=4, p=7, u64=True)
        ctx.feed(b"ACGT", True)
        with pytest.raises(pfbwt_hip.PfpError) as e:
            ctx.feed_vcf_file(fa, vcf)
        assert (e.value.status, e.value.pos) == (pfbwt_hip.E_CORRUPT, line), name
        assert ctx.text_get() == b"ACGTAAAA", name
        ctx.close()
    fa, vcf = write_inputs(tmp, "unknown contig", MALFORMED["unknown contig"][0])
    pr = run([exe["pfbwt-f64"], "--vcf", vcf, "-o", os.path.join(tmp, "bad"), fa], check=False)
    assert pr.returncode != 0 and "line 4" in pr.stderr and not os.path.exists(os.path.join(tmp, "bad.bwt"))
    ctx = factory(w=4, p=7, u64=True)
    for a, b in ((fa, os.path.join(tmp, "nope.vcf")), (os.path.join(tmp, "nope.fa"), vcf)):
        with pytest.raises(pfbwt_hip.PfpError) as e:
            ctx.feed_vcf_file(a, b)
        assert e.value.status == E_IO
    with pytest.raises(pfbwt_hip.PfpError) as e:      # a sample the file lacks: the line of #CHROM
        ctx.feed_vcf_file(*write_inputs(tmp, "good", GOOD), samples="s2,s7")
    assert (e.value.status, e.value.pos) == (pfbwt_hip.E_CORRUPT, 2)
    # the accepted input, gzip-compressed: counters, names and text against the model
    fa, vcf = write_inputs(tmp, "good", GOOD)
    gz = vcf + ".gz"; gzip.open(gz, "wb").write(GOOD.encode())
    c1, c2 = b"ACGTACGTACGGTTAACC", b"TTTTCCCCGGGGAAAA"
    p = Panel([c1, c2, b""], [[(17, 1, [b"CAT"]), (17, 1, [b"G"])], [(0, 4, [b"T", b"TTTTTT"]), (3, 1, [b"G"]), (9, 1, [b"C"])], []],
              [[0, 1, 0, 0], [1, 1, 1, 1], [1, 2, 2, 2], [1, 1, 1, 1], [0, 1, 0, 0]], 4, ["c1", "c2", "c3"], ["s1.0", "s1.1", "s2.0", "s2.1"])
    recs, names, minfo = model_panel(p, True)
    info = ctx.feed_vcf_file(fa, gz, records=True)
    assert (info["lines"], info["samples"], info["skipped_symbolic"], info["missing_gt"]) == (8, 2, 3, 4), info
    assert info["panel"]["skipped_overlap"] == 2 and info["panel"]["kept"] == 3 and info["panel"]["alt_applied"] == minfo["alt_applied"] and info["panel"]["records"] == 15
    assert ctx.text_get() == text_of(recs, 4) and [n for n, _ in ctx.docs()] == names
    ctx.close()
    # a subset in another order through the API
    ctx = factory(w=4, p=7, u64=True)
    ctx.feed_vcf_file(fa, vcf, samples=["s2"], ref_first=False)
    assert ctx.text_get() == text_of(model_panel(select(p, [2, 3]), False)[0], 4)
    ctx.close()


def check_refusals(exe, tmp):
    fa, vcf = fixture("single_chrom")
    out = os.path.join(tmp, "refused")
    for extra, word in ((["--gpus", "2"], "--gpus"), (["--pfbwt-only"], "--pfbwt-only")):
        pr = run([exe["pfbwt-f64"], "--vcf", vcf, "-o", out] + extra + [fa], check=False)
        assert pr.returncode != 0 and "--vcf" in pr.stderr and word in pr.stderr, extra
    pr = run([exe["pfbwt-f64"], "--vcf", vcf, "-o", out], check=False)      # no FASTA argument: stdin
    assert pr.returncode != 0 and "--vcf" in pr.stderr and "stdin" in pr.stderr
    for extra in (["--vcf-samples", "a"], ["--vcf-no-ref"]):
        pr = run([exe["pfbwt-f64"], "-o", out] + extra + [fa], check=False)
        assert pr.returncode != 0 and "--vcf" in pr.stderr
    assert not os.path.exists(out + ".bwt") and not os.path.exists(out + ".dict")
    assert "--vcf" in run([exe["pfbwt-f"], "-h"]).stderr


# ---- CPU: the emulated library and binaries ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pfbwt-f_amd"), "emu", "emu-host"], check=True, stdout=subprocess.DEVNULL)
    return lambda **kw: pfbwt_hip.PfpContext(lib=EMU_SO, **kw)


EMU_EXE = {"pfbwt-f": os.path.join(EMUB, "pfbwt-f-emu"), "pfbwt-f64": os.path.join(EMUB, "pfbwt-f64-emu")}
GPU_EXE = {"pfbwt-f": os.path.join(BIN, "pfbwt-f"), "pfbwt-f64": os.path.join(BIN, "pfbwt-f64")}


def test_vcf_reference_goldens_emu(emu, tmp_path):
    check_reference_goldens(EMU_EXE, str(tmp_path))


def test_vcf_indels_samples_plain_emu(emu, tmp_path):
    check_indels_samples_plain(EMU_EXE, emu, str(tmp_path))


def test_vcf_reader_rules_emu(emu, tmp_path):
    check_reader_rules(emu, EMU_EXE, str(tmp_path))


def test_vcf_refusals_emu(emu, tmp_path):
    check_refusals(EMU_EXE, str(tmp_path))


# ---- GPU: the product library and binaries -------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_vcf_reference_goldens_gpu(gpu_ctx_factory, tmp_path):
    check_reference_goldens(GPU_EXE, str(tmp_path))


@pytest.mark.gpu
def test_vcf_builds_rules_refusals_gpu(gpu_ctx_factory, tmp_path):
    check_indels_samples_plain(GPU_EXE, gpu_ctx_factory, str(tmp_path))
    check_reader_rules(gpu_ctx_factory, GPU_EXE, str(tmp_path))
    check_refusals(GPU_EXE, str(tmp_path))
