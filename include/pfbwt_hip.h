/*
 * include/pfbwt_hip.h -- C ABI of libpfbwt_hip.so, the MI355X (gfx950) engine for the hot path of
 * alshai/pfbwt-f: prefix-free parse, BWT of the parse, dictionary suffix sort and BWT/SA emission.
 *
 * Plain pointers and sizes only (no C++/torch types), so the reference's host code can bind it:
 * INTEGRATION.md shows the replacement bodies for include/pfparser.hpp and include/pfbwt.hpp.
 * Every entry point names the reference interface it stands in for (file:line under the
 * reference tree).  All entry points return PFP_OK (0) or a negative pfp_status; none calls exit().
 *
 * uint_t width: the reference fixes `uint_t` at compile time (-DM64, gsa/gsacak.h:44-58).  Here it
 * is a per-context flag: arrays documented as "U-wide" hold uint32_t without PFP_FLAG_U64 and
 * uint64_t with it.
 *
 * Threading: one pfp_ctx per host thread (the reference gives each std::thread its own PfParser,
 * src/merge_pfp.cpp:97-104).  A context owns one HIP stream and one device workspace.
 */
#ifndef PFBWT_HIP_H
#define PFBWT_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pfp_ctx pfp_ctx;

typedef enum pfp_status {
    PFP_OK = 0,
    PFP_E_ARG = -1,          /* bad argument (w > 32: pfparser.hpp:371-376; p == 0; NULL) */
    PFP_E_INVALID_CHAR = -2, /* hash.hpp:31 "error, invalid character"; see pfp_error_detail */
    PFP_E_TOO_LARGE = -3,    /* input needs 64-bit device indices (pfparser.hpp:326-331, 393-404) */
    PFP_E_NOMEM = -4,        /* device workspace exhausted; pfp_workspace_needed() says how much */
    PFP_E_HIP = -5,          /* HIP runtime error; pfp_error_detail gives the hipError_t */
    PFP_E_ONE_WORD = -6,     /* pfparser.hpp:390-392 "only one dict word total" */
    PFP_E_STATE = -7,        /* call order violated (e.g. pfp_parse_bwt before pfp_parse_finalize) */
    PFP_E_CORRUPT = -8,      /* loaded parse files are inconsistent (pfbwt.hpp:139 "something went wrong!") */
    PFP_E_IO = -9            /* pfp_parse_feed_fasta_file: the file cannot be opened or read (pfparser.hpp:302-304 "failed to open file!") */
} pfp_status;

/* pfp_create flags */
#define PFP_FLAG_U64           1u /* uint_t = uint64_t (pfbwt-f64), else uint32_t (pfbwt-f) */
#define PFP_FLAG_NON_ACGT_TO_A 2u /* PfParserParams::non_acgt_to_a, pfparser.hpp:342-344 */
#define PFP_FLAG_SAI           4u /* PfParserParams::get_sai: keep sai/bwsai (needed for -s / -r) */

/* sizes reported after the parse; names as in SURVEY.md section 8 */
typedef struct pfp_parse_sizes {
    uint64_t n;      /* PfParser::get_n(): text length incl. the w 'A's after each sequence */
    uint64_t m;      /* get_parse_size(): phrases in the parse */
    uint64_t dwords; /* distinct phrases */
    uint64_t dsize;  /* bytes of the .dict image */
} pfp_parse_sizes;

typedef struct pfp_bwt_sizes {
    uint64_t nout;   /* n + 1 outputs */
    uint64_t r;      /* number of BWT runs (src/pfbwt-f.cpp:304-305) */
    uint64_t easy_cases, hard_cases; /* pfbwt.hpp:188 statistics (single-word / multi-word groups) */
} pfp_bwt_sizes;

/* ---- context --------------------------------------------------------------------------------- */
/* PfParser(PfParserParams) pfparser.hpp:82-84 + PrefixFreeBWT ctor pfbwt.hpp:64-81 (w only).
 * device = HIP device ordinal; workspace_bytes = device arena size, 0 = sized on demand. */
pfp_ctx *pfp_create(int w, uint64_t p, unsigned flags, int device, uint64_t workspace_bytes, int *status);
void pfp_destroy(pfp_ctx *ctx);
const char *pfp_strerror(int status);
/* for PFP_E_INVALID_CHAR: text position and byte; for PFP_E_HIP: *ch = hipError_t */
int pfp_error_detail(pfp_ctx *ctx, uint64_t *pos, int *ch);
/* bytes of device workspace the last PFP_E_NOMEM call would have needed (estimate) */
uint64_t pfp_workspace_needed(pfp_ctx *ctx);
/* drop the fed text and every result, keep the context and its workspace.  A stage that fails leaves the
 * context as it was before the call (workspace marks restored): after a failed pfp_parse_finalize the fed text
 * is still there -- retry, append more, or pfp_reset; after PFP_E_NOMEM from pfp_bwt_build(want_sa = 1) a retry
 * with want_sa = 0 or pfp_bwt_build_slice starts from the same state. */
int pfp_reset(pfp_ctx *ctx);

/* ---- stage 1: parse -------------------------------------------------------------------------- */
/* PfParser::add_fasta inner loop, pfparser.hpp:335-352: append raw sequence bytes (host memory).
 * end_of_seq != 0 closes the record: the w 'A's of :335-337 are appended.  Case folding, the
 * optional non-ACGT->A mapping and the validity check of hash.hpp:30-31 happen on the device. */
int pfp_parse_feed(pfp_ctx *ctx, const uint8_t *bases, uint64_t len, int end_of_seq);
/* `count` records of `len` bytes each, record k at bases + k*stride (host memory): the same as `count` calls of
 * pfp_parse_feed(.., len, 1).  Ingest (include/kseq.h:228 reads 16 KiB at a time): page-locked
 * (hipHostMalloc / hipHostRegister) memory is moved by one strided DMA transfer; pageable memory goes through the
 * context's two 32 MiB pinned staging buffers, the host copy into one overlapping the transfer of the other.
 * Both feed calls return when the caller's buffer may be reused. */
int pfp_parse_feed_batch(pfp_ctx *ctx, const uint8_t *bases, uint64_t count, uint64_t len, uint64_t stride);
/* same, but the bytes are already in device memory (one record, pad appended by the library) */
int pfp_parse_feed_device(pfp_ctx *ctx, const void *d_bases, uint64_t len, int end_of_seq);
/* `count` records of `len` bytes each, record k at d_bases + k*stride (device memory): the same as `count` calls of
 * pfp_parse_feed_device(.., len, 1), done as one strided copy (a collection of equal-length haplotypes) */
int pfp_parse_feed_device_batch(pfp_ctx *ctx, const void *d_bases, uint64_t count, uint64_t len, uint64_t stride);
/* The same rows WITHOUT the copy: the caller's buffer becomes the text of this parse -- it must be the first and only feed, and the
 * rows must stay valid and unchanged until pfp_parse_finalize returns.  The trigger scan of pfp_parse_finalize reads the rows where
 * they are and writes the normalised text (with the w 'A's behind every row) into the context's own buffer, which the later stages
 * use: one pass over the input instead of a copy pass and a scan pass (S-32G: 11 ms of 300).  Any other call that appends to or hands
 * out the text first materialises the rows like pfp_parse_feed_device_batch would have.  PFP_E_STATE: the context already holds text. */
int pfp_parse_feed_device_view(pfp_ctx *ctx, const void *d_bases, uint64_t count, uint64_t len, uint64_t stride);
/* FASTA ingest on the device: RAW file bytes -- header lines, newlines and all -- in any chunking (host memory;
 * page-locked memory is read by DMA in place).  Stands in for kseq_read as PfParser::add_fasta drives it, include/kseq.h:178-228,
 * include/pfparser.hpp:300-337: bytes in front of the first '>' / '@' are skipped, a line that starts with '>' or '@' is a header
 * line, the other lines are concatenated without their line ends ('\r' dropped), every record -- empty ones too -- is followed
 * by the w 'A's.  flags: PFP_FASTA_FINAL closes the stream (the last record's pad; the next call starts a new file),
 * PFP_FASTA_RECORDS collects, for the records that START in this call, the offset of their header's first byte in `raw` and the
 * text position (get_n() coordinates) of their first base -- the (name, start) pairs of --print-docs, pfparser.hpp:321-325 -- to be
 * fetched with pfp_parse_fasta_records; *nrec (nullable) = their number.  The raw bytes cross PCIe in chunks of up to 256 MiB;
 * stripping chunk k overlaps the upload of chunk k + 1; returns when the caller's buffer may be reused.
 * PFP_E_ARG with pfp_error_detail ch == '+': a line starts with '+' (a FASTQ quality section, kseq.h:209-221) -- not handled on
 * the device, the context must be reset and the input read by a host-side reader (pfp_parse_feed per record). */
#define PFP_FASTA_FINAL   1u
#define PFP_FASTA_RECORDS 2u
int pfp_parse_feed_fasta(pfp_ctx *ctx, const uint8_t *raw, uint64_t len, unsigned flags, uint64_t *nrec);
int pfp_parse_fasta_records(pfp_ctx *ctx, uint64_t *raw_off, uint64_t *text_pos);
/* The reading side of PfParser::add_fasta, pfparser.hpp:300-307 (gzopen + kseq_init + the kseq_read loop, include/kseq.h:178-228):
 * `path` ("-" = stdin; gzip or plain, detected by content) is read in 64 MiB blocks into page-locked buffers -- a plain regular
 * file by several threads at independent offsets, a gzip stream or a pipe by one -- and the blocks go through
 * pfp_parse_feed_fasta while the next ones are being read.  FASTQ (the first record starts with '@') is read record by record
 * on the host with kseq's rules (quality lines skipped).  flags: PFP_FASTA_RECORDS collects (name, start) of every record for
 * pfp_parse_docs / pfp_parse_doc_get (--print-docs); the stream is always closed (PFP_FASTA_FINAL implied).  info (nullable):
 * raw bytes read, records, text length behind the file, time the consumer waited for the readers, wall time, and which
 * reader ran (1 parallel pread, 2 single zlib / pipe reader, 3 host record reader). */
typedef struct pfp_ingest_info { uint64_t raw_bytes, records, n; double read_wait_ms, total_ms; int mode; } pfp_ingest_info;
int pfp_parse_feed_fasta_file(pfp_ctx *ctx, const char *path, unsigned flags, pfp_ingest_info *info);
/* ---- variant-panel feed: the haplotypes of a reference + variants, expanded on the device ------------------------------------------
 * Stands in for the reference's VCF front end: src/vcf_scan.cpp writes the consensus of ONE haplotype, vcf_to_bwt.py:191-242 runs it
 * once per haplotype, pipes every output through `pfbwt-f64 --parse-only` and merges the parses with merge_pfp.  Here the panel itself
 * crosses PCIe -- ref_len + nsites * nhap bytes instead of nhap * ref_len -- and kernels write every record into the text buffer
 * (csrc/panel.h).  Nothing downstream changes.
 * Panel.  ncontigs reference contigs, contig c = ref[ref_off[c] .. ref_off[c+1]) (empty contigs are allowed).  nsites sites grouped by
 * contig: contig c owns the sites [site_first[c], site_first[c+1]).  Site v has a 0-based position pos[v] in its contig, span[v] = the
 * number of reference bytes it replaces (0: a pure insertion in front of pos; pos + span <= the contig's length) and ALT alleles 1, 2,
 * ...: ALT allele a is the byte string number allele_first[v] + a - 1 of (alt_off, alt_bytes); an empty string is a deletion.  Allele 0
 * is the reference's own bytes ref[pos .. pos + span): no REF string is passed.  Inside a contig the positions ascend, not necessarily
 * strictly.  gt[v * nhap + h] (site-major, as a VCF delivers it) = the allele of haplotype h at site v.
 * Kept sites (src/vcf_scan.cpp:175-213).  Within a contig end = 0 at the start; site v is kept iff pos[v] >= end, and then end = pos[v]
 * + span[v].  Every other site is skipped for every haplotype: the rule looks at geometry only, never at genotypes.
 * Record of (h, c).  For the kept sites v1 < v2 < ... of c: ref[0 .. pos[v1]) + allele(gt[v1, h]) + ref[pos[v1] + span[v1] .. pos[v2])
 * + ... + ref[end_last .. len_c), followed by the w 'A's of pfparser.hpp:335-337.
 * Order.  With PFP_PANEL_REF_FIRST the ncontigs records of the reference itself come first (allele 0 everywhere); then for h = 0 ..
 * nhap-1 the contigs 0 .. ncontigs-1 (haplotype-major: the order vcf_to_bwt.py:191-192, 218, 242 gives its files).  The nrec = (nhap +
 * ref_first) * ncontigs records are appended to the text like pfp_parse_feed_device_batch appends rows.  Bytes are written raw: case
 * folding, PFP_FLAG_NON_ACGT_TO_A and the validity check stay in pfp_parse_finalize.
 * The call is one of the feeds: a pending row view is flushed first, a context in a later stage is reset, the text may already hold
 * records and more may follow; it returns when the caller's arrays may be reused.  PFP_PANEL_RECORDS: (name, start) of every record
 * for pfp_parse_docs / pfp_parse_doc_get (appended to those of a text that is not empty): a reference record is named <contig>, a
 * haplotype record <hap_names[h]>.<contig>; missing names are generated as h<k> / c<k>.
 * PFP_E_ARG: NULL arrays, descending offsets, positions that descend inside a contig, pos + span beyond its contig, allele_first /
 * alt_off inconsistent, unknown flag bits, a genotype >= 1 + the site's ALT count -- pfp_error_detail then reports pos = the index into
 * gt and ch = the value; the genotypes are checked on the device before anything is written.  PFP_E_TOO_LARGE: the text would pass the
 * width's limit (as for pfp_parse_feed), 2^32 or more sites or records.  PFP_E_NOMEM: pfp_workspace_needed reports the demand (the
 * uploaded arrays + 8 bytes per (tile of panel_tile kept sites, haplotype) + 8 per record; all of it is given back before returning).
 * Every failure leaves text, n, the view and the document names as they were.  nhap == 0 without REF_FIRST and ncontigs == 0 append
 * nothing.  pfp_debug_set: panel_tile, panel_out_bytes, panel_swizzle (include/pfbwt_hip_dev.h).
 * Out of scope: the marker-positions stream (.mps) of a panel, bit-packed genotypes, pfp_sharded_* with a panel. */
#define PFP_PANEL_REF_FIRST 1u
#define PFP_PANEL_RECORDS   2u   /* collect (name, start) of every record for pfp_parse_docs / pfp_parse_doc_get */
typedef struct pfp_panel {       /* all host memory */
    uint64_t ncontigs; const uint8_t *ref; const uint64_t *ref_off;          /* ncontigs + 1 */
    const char *const *contig_names;                                         /* nullable; used with PFP_PANEL_RECORDS */
    uint64_t nsites; const uint64_t *site_first;                             /* ncontigs + 1 */
    const uint64_t *pos; const uint32_t *span; const uint64_t *allele_first; /* nsites, nsites, nsites + 1 */
    uint64_t nalt; const uint64_t *alt_off; const uint8_t *alt_bytes;        /* nalt + 1 offsets */
    uint64_t nhap; const uint8_t *gt; const char *const *hap_names;          /* nsites * nhap; names nullable */
} pfp_panel;
typedef struct pfp_panel_info { uint64_t contigs, haplotypes, records, sites, kept, skipped_overlap,
    alt_applied /* (record, kept site) pairs with gt > 0 */, bases /* text bytes added, pads included */, min_record, max_record; } pfp_panel_info;
int pfp_parse_feed_panel(pfp_ctx *ctx, const pfp_panel *panel, unsigned flags, pfp_panel_info *info /* nullable */);
/* The same from files: a reference FASTA and a text VCF (plain or gzip / bgzip), read on the host by a reader of this project (csrc/
 * vcfread.h: zlib and the standard library, no htslib); one pfp_panel is built and fed with one pfp_parse_feed_panel call.
 * Contigs = the FASTA's records in FASTA order (a contig without VCF lines yields the reference sequence for every haplotype).  Samples
 * = the columns of the #CHROM line, or the comma list `samples` (a subset, in the order given).  Every sample is two haplotypes, s.0 and
 * s.1 (include/vcf_scanner.hpp:217-219).  GT must be the first FORMAT key; '|' and '/' both separate; a haploid call serves both
 * haplotypes (:32-38); '.' is allele 0 and counted in missing_gt (:185-188).  A site whose ALT list holds a symbolic allele (<...>, *,
 * a breakend, .) is dropped before the overlap rule and counted in skipped_symbolic.
 * PFP_E_CORRUPT with the 1-based line number in pfp_error_detail pos: a contig name the FASTA lacks, lines of one contig that are not
 * contiguous or descend, REF that differs from the FASTA (case-insensitive) or runs past the contig, a genotype beyond the ALT list,
 * ploidy above 2, more than 255 ALTs, a short line, a sample of `samples` that the file lacks (line of #CHROM).  PFP_E_IO: unreadable files.
 * Out of scope: BCF, indexed / region reads, ploidy other than 2. */
typedef struct pfp_vcf_info { uint64_t lines, samples, skipped_symbolic, missing_gt; pfp_panel_info panel; } pfp_vcf_info;
int pfp_parse_feed_vcf_file(pfp_ctx *ctx, const char *ref_fasta, const char *vcf, const char *samples /* nullable: comma list, subset and order */,
                            unsigned flags, pfp_vcf_info *info /* nullable */);
int pfp_parse_docs(pfp_ctx *ctx, uint64_t *count);
int pfp_parse_doc_get(pfp_ctx *ctx, uint64_t i, const char **name, uint64_t *start);   /* valid until the next pfp_parse_feed_fasta_file */
/* Announce the size of the text that is going to be fed (e.g. the size of the FASTA file): sizes the ADDRESS range of the text
 * buffer -- HBM itself is committed as the text grows.  Optional; without it the range is four times what the first feed needs
 * (at least 64 MiB) and doubles when the text outgrows it (the text is then moved once: a device-to-device copy). */
int pfp_parse_reserve(pfp_ctx *ctx, uint64_t text_bytes);
/* Back to feeding with the text kept: after pfp_parse_finalize the (normalised) text is still on the device, more
 * records can be appended and pfp_parse_finalize run again -- what PfParser::operator+= (pfparser.hpp:194-263) needs
 * when the right-hand parse is appended as text (pfp_text_view of its context + pfp_parse_feed_device) instead of being
 * merged phrase by phrase.  PFP_E_STATE for a context whose state came from pfp_merge_shards or pfp_bwt_load. */
int pfp_parse_reopen(pfp_ctx *ctx);
/* device pointer and length of the text fed so far (NULL / 0 when the context holds none) */
int pfp_text_view(pfp_ctx *ctx, const uint8_t **d_text, uint64_t *n);
/* bytes [off, off + len) of that text copied to host memory (PFP_E_ARG: the range is not inside the text) */
int pfp_text_get(pfp_ctx *ctx, uint64_t off, uint64_t len, uint8_t *host);
/* PfParser::finalize pfparser.hpp:484-517 (+ process_phrase :595-601 for every phrase): trigger scan,
 * phrase de-duplication, dictionary sort, ranks, occ, last, sai.  Results stay on the device. */
int pfp_parse_finalize(pfp_ctx *ctx, pfp_parse_sizes *out);
/* The same for a shard that is only going to be merged (pfp_shard_view_get + pfp_merge_shards): phrases, dictionary words
 * and phrase ids, but no dictionary sort, ranks, .parse or .occ -- the merge produces those for the united dictionary.  The
 * context then answers pfp_shard_view_get only (pfp_parse_get / pfp_parse_bwt: PFP_E_STATE), like one filled by
 * pfp_shard_load. */
int pfp_parse_finalize_shard(pfp_ctx *ctx, pfp_parse_sizes *out);
/* save_parser pfbwt_io.hpp:234-249 getters: copy results to caller-owned host buffers (NULL skips).
 * dict: dsize bytes (.dict image); occ: dwords U-wide; parse: m uint32 (1-based ranks);
 * last: m bytes; sai: m U-wide (only with PFP_FLAG_SAI). */
int pfp_parse_get(pfp_ctx *ctx, uint8_t *dict, void *occ, uint32_t *parse, uint8_t *last, void *sai);
/* PfParser::bwt_of_parse pfparser.hpp:379-467 (sacak_int :425 included) */
int pfp_parse_bwt(pfp_ctx *ctx);
/* the three vectors handed to OutFn at pfparser.hpp:466: bwlast m+1 bytes, ilist / bwsai m+1 U-wide */
int pfp_parse_bwt_get(pfp_ctx *ctx, uint8_t *bwlast, void *ilist, void *bwsai);

/* ---- multi-GPU: sharded parse (semantics of PfParser::operator+=, pfparser.hpp:194-263) ---- */
/* A shard is a run of whole sequences.  Shard r > 0 is fed the w 'A's that end shard r-1 first (pfp_parse_feed(ctx,
 * "AAAA...", w, 0) or pfp_parse_feed_left_context) as left context, then its sequences; every shard is parsed with pfp_parse_finalize on its own GPU.
 * pfp_shard_view_get exposes the device arrays of a finished local parse (to be copied into send buffers with
 * pfp_device_copy and exchanged with one RCCL all-gather); pfp_merge_shards takes the N views -- device pointers on
 * the calling context's GPU -- and leaves that context in the state pfp_parse_finalize would have produced on the
 * concatenated text (then pfp_parse_get / pfp_parse_bwt / pfp_bwt_build as usual). */
typedef struct pfp_shard_view {
    uint64_t n, m, dwords, dsize;   /* n counts the w context bytes of a shard r > 0 */
    const uint8_t *d_dict;          /* dsize bytes: distinct phrases, each + 0x01, then 0x00 (any order) */
    const uint32_t *d_ws;           /* dwords+1 word starts in d_dict */
    const uint32_t *d_pid;          /* m: word id of every phrase */
    const uint64_t *d_ye;           /* m: 1-based end position of every phrase in the shard's text (= sai) */
    const uint8_t *d_last;          /* m.  d_ye and d_last may BOTH be NULL: pfp_merge_shards then derives them from d_dict / d_ws / d_pid
                                       (a phrase ends where its predecessor ended + its word's length - w), so that only the dictionary
                                       and 4 bytes per phrase have to travel between GPUs */
    uint64_t left_context;          /* bytes of left context in front of the shard's own text: w (pfp_parse_feed_left_context: the
                                       shard was parsed knowing that w 'A's precede it) or 0 (a stand-alone parse, e.g. one made by
                                       `pfbwt-f --parse-only` and loaded with pfp_shard_load: the merge then re-tests the first w
                                       windows of the shard like PfParser::operator+=, pfparser.hpp:226-245) */
} pfp_shard_view;
/* the w 'A's that end the previous shard, fed as left context of a shard r > 0 (must be the first feed of the shard) */
int pfp_parse_feed_left_context(pfp_ctx *ctx);
/* A parse that was saved to <prefix>.dict / <prefix>.parse (pfbwt_io.hpp:234-249; load_parser :211-222 + init_from_dict_ranks,
 * pfparser.hpp:549-567) becomes a shard on the device: dict = the .dict image (dsize bytes), parse = m 1-based ranks.
 * The context then answers pfp_shard_view_get (left_context = 0) -- nothing else; it holds no text. */
int pfp_shard_load(pfp_ctx *ctx, const uint8_t *dict, uint64_t dsize, const uint32_t *parse, uint64_t m);
int pfp_shard_view_get(pfp_ctx *ctx, pfp_shard_view *view);
int pfp_device_copy(pfp_ctx *ctx, void *d_dst, const void *d_src, uint64_t bytes);
int pfp_merge_shards(pfp_ctx *ctx, int nshards, const pfp_shard_view *views, pfp_parse_sizes *out);

/* ---- multi-GPU from ONE process: N devices, N host threads, RCCL called directly ------------------------------------------------
 * The reference's only parallelism has this shape: src/merge_pfp.cpp:131-152 gives every std::thread its own PfParser over a
 * contiguous slice of the inputs and folds the per-thread parsers with PfParser::operator+= (include/pfparser.hpp:194-263).  Here
 * rank r owns device devices[r] (NULL: 0 .. ndev-1): the caller feeds rank r's run of whole sequences into pfp_sharded_ctx(s, r) with
 * any pfp_parse_feed* call (the w 'A's that end the previous run are already in front of it, pfparser.hpp:335-337; ranks may be fed
 * from different threads), then ONE call builds everything: every rank finalizes its shard (pfp_parse_finalize_shard), the ranks
 * exchange {dictionary, word starts, phrase ids} in one ncclAllGather over xGMI (ncclCommInitAll at creation; librccl.so is loaded
 * at run time, only when distinct devices have to talk -- ranks that share a device, a rehearsal of the protocol on one card,
 * copy device to device), every rank merges (pfp_merge_shards), sorts dictionary and parse, and emits slice r of the output rows
 * (pfp_bwt_build_slice).  Afterwards pfp_bwt_get / pfp_bwt_device_ptrs / pfp_bwt_write of rank r's context deliver slice r; the
 * slices in rank order are the reference's .bwt / .sa / .ssa / .esa.  psz: sizes of the whole collection's parse; bsz / slice_begin /
 * slice_rows / esa_pairs: ndev entries each (NULL skips).  A failing rank (an invalid character in its shard, ...) makes every rank
 * give up before the collective; pfp_sharded_error names it (every rank needs at least one sequence: PFP_E_ARG otherwise).
 * pfp_sharded_reset: all ranks ready for the next collection. */
typedef struct pfp_sharded pfp_sharded;
pfp_sharded *pfp_sharded_create(int w, uint64_t p, unsigned flags, int ndev, const int *devices, uint64_t workspace_bytes, int *status);
void pfp_sharded_destroy(pfp_sharded *s);
int pfp_sharded_ranks(pfp_sharded *s);
pfp_ctx *pfp_sharded_ctx(pfp_sharded *s, int rank);
int pfp_sharded_build(pfp_sharded *s, int want_sa, int want_rssa, pfp_parse_sizes *psz, pfp_bwt_sizes *bsz,
                      uint64_t *slice_begin, uint64_t *slice_rows, uint64_t *esa_pairs);
int pfp_sharded_reset(pfp_sharded *s);
const char *pfp_sharded_error(pfp_sharded *s);

/* ---- stage 2: BWT / SA ------------------------------------------------------------------------- */
/* PrefixFreeBWT ctor pfbwt.hpp:64-81, for --pfbwt-only: upload .dict .occ .bwlast .ilist [.bwsai]
 * images (host memory).  Not needed when pfp_parse_finalize + pfp_parse_bwt ran in this context.
 * ilist and bwsai must hold nrows elements each, like bwlast (the caller compares the file sizes).
 * n_hint: the value of the .n file (src/pfbwt-f.cpp:282-285), sizes the workspace and arms the
 * "exactly n + 1 rows" check of the emission; 0 = unknown.  PFP_E_CORRUPT: the images are inconsistent
 * (dictionary not terminated, word count != entries of occ, sum(occ) + 1 != nrows, an ilist entry >= nrows). */
int pfp_bwt_load(pfp_ctx *ctx, const uint8_t *dict, uint64_t dsize, const void *occ, uint64_t dwords,
                 const uint8_t *bwlast, const void *ilist, const void *bwsai, uint64_t nrows, uint64_t n_hint);
/* PrefixFreeBWT::generate_bwt_lcp pfbwt.hpp:96-194 (sort_dict_suffixes :206-223 = gsacak included)
 * fused with the CLI's out_fn src/pfbwt-f.cpp:298-328: BWT bytes, SA (row 0 := n), run samples. */
int pfp_bwt_build(pfp_ctx *ctx, int want_sa, int want_rssa, pfp_bwt_sizes *out);
/* The same, with the rows on their way to host memory while the emission is still running: host_bwt (n + 1 bytes, n from
 * pfp_parse_sizes / pfp_text_length) and, with want_sa, host_sa (n + 1 U-wide values) are filled window by window -- the DMA
 * transfer of a window overlaps the emission of the next (page-locked destinations run at the link's rate).  The run samples
 * are fetched afterwards with pfp_bwt_get(ctx, NULL, NULL, ssa, esa) once out->r says how large they are. */
int pfp_bwt_build_stream(pfp_ctx *ctx, int want_sa, int want_rssa, uint8_t *host_bwt, void *host_sa, pfp_bwt_sizes *out);
/* PfParser::get_n(): bytes of text fed so far (the w 'A's behind every record included) */
int pfp_text_length(pfp_ctx *ctx, uint64_t *n);
/* Multi-GPU emission: every rank holds the same parse state (after pfp_merge_shards + pfp_parse_bwt) and emits
 * only output rows [nout*slice/nslices, nout*(slice+1)/nslices).  out->r counts the runs that START in the slice
 * (the sum over slices is r); pfp_bwt_get / pfp_bwt_device_ptrs then refer to the slice (slice_rows entries).
 * want_rssa: the slice's part of the run samples (src/pfbwt-f.cpp:306-315, 325-328) -- out->r (row, sa) pairs for the
 * run starts in the slice and *esa_pairs pairs for the run ends they imply (the row in front of every run start, which
 * for the first start of a slice > 0 lies in the previous slice, plus the last row of the output in the last slice).
 * Concatenated over the slices in order they are the reference's .ssa / .esa files; no rank needs another rank's data. */
int pfp_bwt_build_slice(pfp_ctx *ctx, int want_sa, int want_rssa, int slice, int nslices, pfp_bwt_sizes *out,
                        uint64_t *slice_begin, uint64_t *slice_rows, uint64_t *esa_pairs);
/* copy results to host (NULL skips): bwt nout bytes; sa nout U-wide; ssa 2*r, esa 2*r (slices: 2*esa_pairs) U-wide */
int pfp_bwt_get(pfp_ctx *ctx, uint8_t *bwt, void *sa, void *ssa, void *esa);
/* `.bwt` into host memory through its run-length form (needs the state left by pfp_bwt_build(want_rssa = 1) over the whole output):
 * row `.ssa[k]` starts run k, so one byte per run crosses PCIe (r bytes instead of n + 1 -- 84 MB instead of 32 GB on a 1000-haplotype
 * collection) and `threads` host threads write the runs out.  ssa_host: the 2 * r U-wide values pfp_bwt_get returned for `.ssa`
 * (NULL: fetched again).  host_bwt receives exactly the n + 1 bytes of pfp_bwt_get.  threads < 1: one per CPU the process may run on;
 * the output is cut into 64 MiB blocks of BYTES that the threads claim from the front (runs are cut at the blocks' borders); when
 * host_bwt is page-locked (pfp_host_register) the copy engine claims blocks from the back and moves those rows over PCIe while the threads write. */
int pfp_bwt_get_expanded(pfp_ctx *ctx, uint8_t *host_bwt, const void *ssa_host, int threads);
/* The results of the last build straight to file descriptors (-1 skips one): what out_fn of src/pfbwt-f.cpp:298-328 writes with two to
 * four fwrite calls per base.  The bytes leave the device in 64 MiB blocks through page-locked buffers; the transfer of a block
 * overlaps the write of the one before; a regular file is written by several threads (pwrite at the block's offset), a pipe --
 * `-c bwt`: stdout -- in order by one.  PFP_E_IO: a write failed. */
int pfp_bwt_write(pfp_ctx *ctx, int fd_bwt, int fd_sa, int fd_ssa, int fd_esa);
/* device pointers of the same results (valid until the next pfp_* call that rebuilds them) */
int pfp_bwt_device_ptrs(pfp_ctx *ctx, const void **d_bwt, const void **d_sa, const void **d_ssa, const void **d_esa);

/* ---- marker-array post-pass --------------------------------------------------- */
/* write_marker_array, include/marker_array.hpp:138-174 (the tool src/mps_to_ma.cpp): mps = the marker-positions stream
 * written by MarkerPositionsWriter (:60-136; records: first text position, last text position, packed markers
 * (include/marker.hpp:9-52), 0xFFFFFFFFFFFFFFFF; intervals ascending and disjoint).  Every suffix-array value is looked up
 * (rle_window_arr::at, include/rle_window_array.hpp:118-131) and consecutive rows with equal, non-empty marker lists become
 * one record: first row, last row, the markers, 0xFFFFFFFFFFFFFFFF.  sa_host == NULL: fused with the build -- the suffix
 * array pfp_bwt_build(want_sa = 1) left on the device is used (the reference pipes it through `tee`, vcf_to_bwt.py:259-285);
 * otherwise sa_host holds nrows U-wide values in BWT order (row 0 = n, src/pfbwt-f.cpp:301) and the context is reset.
 * *out_words = 64-bit words of the .ma stream, fetched with pfp_marker_array_get.  Like the document, LCP and threshold
 * arrays below, a marker array is dropped by the next build or reset: pfp_marker_array_get then copies nothing. */
int pfp_marker_array(pfp_ctx *ctx, const uint64_t *mps, uint64_t mps_words, const void *sa_host, uint64_t nrows, uint64_t *out_words);
int pfp_marker_array_get(pfp_ctx *ctx, uint64_t *dst);

/* ---- document-array post-pass ------------------------------------------------------------------- */
/* The document of every SA value of the last build: the reference names the document array as its next feature (README.md,
 * "Features that will be added soon"); gsacak's DA (pfp_gsacak_*) is the same question asked of a dictionary.
 * Definition.  The text whose suffixes the SA values index is the concatenation of the records, each followed by its w 'A's
 * (pfparser.hpp:335-337); SA values are 0-based positions in it, row 0 holds n (src/pfbwt-f.cpp:301).  Record k starts at
 * b_k: b_0 = 0, b_{k+1} = b_k + len_k + w -- the get_n() coordinates that pfp_parse_doc_get returns and that .docs holds
 * (pfparser.hpp:321-324), also for a .docs written by merge_pfp --docs.  doc(s) = max{k : b_k <= s}: the w 'A's of a record
 * belong to it, row 0 (s = n) to the last record.
 * starts: the ndocs record starts b_k (host memory; starts[0] == 0, strictly ascending, all < n).  what: PFP_DA_ROWS (needs a build
 * with want_sa) and / or PFP_DA_RUNS (needs want_rssa).  Works after pfp_bwt_build and after pfp_bwt_build_slice -- on the slice's
 * rows and samples, so also on every rank of pfp_sharded_* when each is given the whole collection's table.  Results (U-wide
 * values, in the order of pfp_bwt_get): da = doc of every row (slice_rows values; file <prefix>.da); sda = the .ssa pairs with the
 * SA value replaced by its doc, sda[2i] = ssa[2i], sda[2i+1] = doc(ssa[2i+1]) (2 * r values; <prefix>.sda); eda = the same for
 * .esa (2 * esa_pairs values; <prefix>.eda).  They live on the device until the next build or reset.
 * PFP_E_ARG: a table that is empty, does not start at 0, is not strictly ascending or holds a start >= n, an unknown `what`.
 * PFP_E_STATE: no build, or no SA values of the kind asked for (a BWT-only build, ROWS without want_sa, RUNS without want_rssa);
 * from _get / _write: an array that the last pfp_doc_array did not make. */
#define PFP_DA_ROWS 1u
#define PFP_DA_RUNS 2u
int pfp_doc_array(pfp_ctx *ctx, const uint64_t *starts, uint64_t ndocs, unsigned what);
int pfp_doc_array_get(pfp_ctx *ctx, void *da, void *sda, void *eda);      /* host copies (NULL skips) */
int pfp_doc_array_device_ptrs(pfp_ctx *ctx, const void **d_da, const void **d_sda, const void **d_eda);      /* NULL: not made */
int pfp_doc_array_write(pfp_ctx *ctx, int fd_da, int fd_sda, int fd_eda); /* like pfp_bwt_write (-1 skips one) */

/* ---- LCP-array post-pass ------------------------------------------------------------------------ */
/* The LCP array of the last build, worked out on the device from the text that is still resident.
 * Definition.  T = the normalised text of the build (pfp_text_view: the records, each followed by its w 'A's, after case folding /
 * PFP_FLAG_NON_ACGT_TO_A), n its length, T[n] a terminator smaller than every byte; SA = the engine's output (row 0 holds n).
 * LCP[0] = 0, LCP[i] = length of the longest common prefix of T[SA[i-1] .. n) and T[SA[i] .. n) for i = 1 .. n: the plain LCP
 * array of T$ (the SA is the strict lexicographic order of the suffixes of T$, so record borders are no special case).
 * what: PFP_LCP_ROWS -- lcp[i] = LCP[i], n + 1 U-wide values (file <prefix>.lcp); needs pfp_bwt_build(want_sa = 1) over the whole
 * output (want_rssa optional: without it the run starts are found in bwt / sa).  PFP_LCP_RUNS -- slcp: pairs like .ssa,
 * slcp[2k] = ssa[2k] (the row that starts run k), slcp[2k+1] = LCP[ssa[2k]] (2 * r values; <prefix>.slcp); needs want_rssa; works
 * after pfp_bwt_build and after pfp_bwt_build_slice (the r pairs of the slice; concatenated over the slices = the whole .slcp) and
 * needs no full SA: the suffix in front of a run start is the previous run's end (.esa).
 * info (nullable): statistics of the values at the run starts ("irreducible" values) -- their number, maximum and sum, and how many
 * of them were longer than the single-lane limit (pfp_debug_set "lcp_long_min") and were finished by a whole wave.
 * The arrays live on the device until the next build or reset and coexist with the document arrays and a marker array of the
 * same build, in either call order.
 * PFP_E_ARG: `what` zero or unknown.  PFP_E_STATE: no build; the context does not hold the text of the build (state from
 * pfp_bwt_load, pfp_merge_shards, the ranks of pfp_sharded_*); ROWS without SA or on a slice; RUNS without samples; from _get /
 * _write: an array that the last pfp_lcp_array did not make.  PFP_E_NOMEM (ROWS: 2 * (n + 1) * U bytes at the peak, half of it
 * released afterwards) leaves the context as it was. */
#define PFP_LCP_ROWS 1u
#define PFP_LCP_RUNS 2u
typedef struct pfp_lcp_info { uint64_t pairs, max_lcp, sum_lcp, long_pairs; } pfp_lcp_info;   /* of the irreducible values */
int pfp_lcp_array(pfp_ctx *ctx, unsigned what, pfp_lcp_info *info /* nullable */);
int pfp_lcp_array_get(pfp_ctx *ctx, void *lcp, void *slcp);                 /* host copies (NULL skips) */
int pfp_lcp_array_device_ptrs(pfp_ctx *ctx, const void **d_lcp, const void **d_slcp);      /* NULL: not made */
int pfp_lcp_array_write(pfp_ctx *ctx, int fd_lcp, int fd_slcp);             /* like pfp_doc_array_write (-1 skips one) */

/* ---- matching-statistics thresholds post-pass --------------------------------------------------- */
/* The threshold of every run of the last build (Bannai, Gagie, I 2020; Rossi et al. 2022): with .ssa / .esa they make a matching-statistics
 * index that needs no LCP values at query time.  Worked out on the device from the LCP rows.
 * Definition.  BWT, SA and LCP as for pfp_lcp_array, n + 1 rows.  Run k starts at row s = ssa[2k] with the symbol c = BWT[s]; e = the
 * largest row < s with BWT[e] == c (the last row of the previous run of c).
 *   - No such e (the first run of a symbol; the one-row run of the terminator byte 0): the run has no threshold, thr = 0 and tlcp = 0.
 *     Row 0 is never a real threshold (j > e >= 0), so thr = 0 is unambiguous; tlcp = 0 also occurs for real thresholds.
 *   - Otherwise tlcp = min LCP[e+1 .. s] and thr = the LEFTMOST row j in (e, s] with LCP[j] == tlcp (any minimiser serves matching
 *     statistics; ties are pinned to the leftmost so that the output is reproducible).
 * Results, U-wide pairs shaped like .ssa: thr[2k] = ssa[2k], thr[2k+1] = j (2 * r values; file <prefix>.thr); tlcp[2k] = ssa[2k],
 * tlcp[2k+1] = LCP[j] (2 * r values; <prefix>.tlcp).  This is this project's own layout, not the packed on-disk format of MONI.
 * Needs pfp_bwt_build(want_sa = 1, want_rssa = 1) over the whole output in a context that still holds the text of the build (the
 * PFP_LCP_ROWS conditions of pfp_lcp_array plus run samples).  The rows of a preceding pfp_lcp_array(PFP_LCP_ROWS) of the same build
 * are used when they are still there; otherwise they are computed into scratch and released before returning.
 * info (nullable): runs = r, none = runs without a threshold, long_queries = runs whose gap s - e was longer than the single-lane
 * limit (pfp_debug_set "thr_long_min") and went to the wave-per-run route, max_span = the largest s - e.
 * The arrays live on the device until the next build or reset and coexist with the LCP, document and marker arrays of the same
 * build, in any call order.
 * Scope: the full SA and the LCP rows must fit on the device next to the text -- collections of the S-chr22 / S-3G class.  A
 * 32 Gbase collection built with -r only, whose SA alone exceeds the device memory, takes pfp_thresholds_windowed below.
 * PFP_E_STATE: no build; no SA; no run samples; a slice; the context does not hold the text of the build (state from pfp_bwt_load,
 * pfp_merge_shards, the ranks of pfp_sharded_*); from _get / _write: nothing was made.  PFP_E_TOO_LARGE: 2^32 runs or more.
 * PFP_E_NOMEM leaves the context as it was.  Peak memory beyond the build: with cached rows 4 * r * U (results) + 16 * r (sort) +
 * 24 * r (queue, shrunk to fit) + 2 * (n + 1) / thr_tile * U bytes; without them 2 * (n + 1) * U bytes more while the rows are
 * made (as PFP_LCP_ROWS), (n + 1) * U of it until the call returns. */
typedef struct pfp_thr_info { uint64_t runs, none, long_queries, max_span; } pfp_thr_info;
int pfp_thresholds(pfp_ctx *ctx, pfp_thr_info *info /* nullable */);
int pfp_thresholds_get(pfp_ctx *ctx, void *thr, void *tlcp);              /* host copies (NULL skips) */
int pfp_thresholds_device_ptrs(pfp_ctx *ctx, const void **d_thr, const void **d_tlcp);      /* NULL: not made */
int pfp_thresholds_write(pfp_ctx *ctx, int fd_thr, int fd_tlcp);          /* like pfp_lcp_array_write (-1 skips one) */
/* The same thresholds without a resident SA and without LCP rows: for collections whose SA does not fit on the device (built with
 * want_rssa only).  The r irreducible LCP values (pfp_lcp_array(PFP_LCP_RUNS): those of a preceding call are used when they are still
 * there, else they are computed into scratch) and their text positions determine every LCP value -- a row that does not start a
 * run has PLCP[p] = PLCP[p - 1] - 1 -- so r sorted (position, value + position) pairs and a block directory stand in for the dense
 * array; the emission runs once more as for want_sa = 1, window by window into scratch, and every window of SA values is turned into
 * LCP rows, tile minima and the partial minima of the gaps that touch it.
 * Needs pfp_bwt_build(want_rssa = 1) over the whole output in a context that still holds the text of the build; want_sa may be either
 * value -- a resident SA is ignored and left untouched, like every other array, size and flag of the build.
 * window_rows: rows per window; 0 selects the default (pfp_debug_set "thr_window_rows", 2^30: not measured yet); rounded up to a
 * multiple of thr_tile so that a tile never straddles two windows.  *windows (nullable) = the number of windows visited.
 * Results: the arrays of pfp_thresholds, bit for bit (leftmost minimiser included), served by pfp_thresholds_get / _device_ptrs /
 * _write; info as for pfp_thresholds (long_queries counts the gaps longer than thr_long_min, whatever route their pieces took).  A
 * call replaces the result of an earlier pfp_thresholds / pfp_thresholds_windowed of the build.
 * PFP_E_STATE: no build; no run samples; a slice; the context does not hold the text of the build.  PFP_E_TOO_LARGE: 2^32 runs or
 * more.  PFP_E_CORRUPT: the run samples are inconsistent (value + position decreases along the text).  PFP_E_NOMEM leaves the
 * context as it was.  Peak memory beyond the build: 4 * r * U (results) + 2 * r * U + 4 * ((n >> B) + 2) (pairs and directory, B =
 * floor(log2(n / r))) + 12 * r (sort by head byte and its inverse) + 24 * r (queue, shrunk to fit) + 2 * (n + 1) / thr_tile * U (tile
 * minima of ALL tiles) + window_rows * (2 * U + 1) (one window of SA, LCP and BWT) + the scratch of the emission pre-pass of a
 * want_sa build (about 60 bytes per dictionary byte and 8 per parse row); 24 * r + 2 * r * U more while the pairs are sorted. */
int pfp_thresholds_windowed(pfp_ctx *ctx, uint64_t window_rows, pfp_thr_info *info /* nullable */, uint64_t *windows /* nullable */);

/* ---- matching-statistics queries ---------------------------------------------------------------- */
/* The question the run samples and thresholds are built for: for every position i of a pattern P[0 .. m), a text position ptr[i] and
 * the length len[i] of the longest prefix of P[i .. m) that occurs in the text -- an occurrence starts at ptr[i].  Answered on the
 * device against the build the context holds: the run-length BWT through .ssa / .esa, the thresholds, and the text itself, so that
 * lengths are byte comparisons on the resident text (no LCP values, no grammar).  DESIGN.md section 2.
 * Definitions.  T, n, BWT, SA, .ssa, .esa, .thr as above.  Run k covers the rows start[k] = ssa[2k] .. esa[2k], head[k] =
 * BWT[start[k]], sval[k] = ssa[2k+1], eval[k] = esa[2k+1], thr[k] = the threshold row (0: none).  With the runs sorted stably by their
 * head, lfhead[k] = the exclusive sum of the run lengths in that order: LF(i) = lfhead[k] + (i - start[k]) for a row i of run k.
 * Pointers.  From row = 0, pos = n, for i = m-1 .. 0 with c = P[i]: k = the run that holds row.  No run has the head c ("absent"):
 * ptr[i] = n, row = 0, pos = n.  Else, head[k] == c ("match"): nothing to do; otherwise with kn / kp = the nearest run of c behind /
 * in front of k: when kn exists and (kp does not exist or row >= thr[kn]) ("down") k = kn, row = start[kn], pos = sval[kn]; else ("up")
 * k = kp, row = esa[2kp], pos = eval[kp].  Then row = LF(row), pos -= 1, ptr[i] = pos.  Thresholds are pinned to the leftmost
 * minimiser, so ptr is fully determined.
 * Lengths.  len[i] = the longest common prefix of P[i .. m) and T[ptr[i] .. n) -- by the theorem of Bannai, Gagie and I the length of
 * the longest prefix of P[i ..] that occurs in T.  A position i is a BREAK when i == 0 or ptr[i] != ptr[i-1] + 1; only breaks are
 * compared with the text, every other position has len[i] = len[b] - (i - b) for its last break b.
 * Patterns are byte strings: upper-cased, and in a context with PFP_FLAG_NON_ACGT_TO_A every byte outside ACGT becomes 'A', exactly as
 * the feed does to the text.  Other bytes stay; a byte that heads no run has ptr = n and length 0.  A byte 0 after normalisation is
 * refused: it would match the terminator.  An empty pattern yields no values.
 *
 * pfp_ms_index builds the index: a copy of the threshold rows (a later thresholds call may replace that slot), lfhead, head, the
 * sorted runs with the 257 borders of the symbols, and a run directory (for every block of 2^B rows the run that holds its first
 * row, B = floor(log2((n + 1) / r)); pfp_debug_set "ms_dir_log2").  .ssa, .esa and the text are read in place.  Needs
 * pfp_bwt_build(want_rssa = 1) over the whole output (want_sa either value) in a context that still holds the text of the build, and
 * the thresholds of that build from pfp_thresholds or pfp_thresholds_windowed.  The index lives until the next build or reset and
 * coexists with every other post-pass result, in any call order; a second call replaces it.
 * PFP_E_STATE: no build; no run samples; a slice; no text (pfp_bwt_load, pfp_merge_shards, pfp_sharded_*); no thresholds; a run whose
 * head is the byte 1 -- for some tiny w / p the reference writes the EndOfWord byte into .bwt and this project keeps that bit for bit;
 * such a .bwt is not the BWT of T and LF over it is meaningless.  PFP_E_TOO_LARGE: 2^32 runs or more.  PFP_E_NOMEM leaves the
 * context as it was.  Memory: r * (2 * U + 5) + 4 * ((n + 1) >> B) bytes; 24 * r + r * U more while it is built.
 *
 * pfp_ms_query: pattern j is bases[offsets[j] .. offsets[j+1]) (host memory; npatterns + 1 ascending offsets; npatterns == 0 is
 * valid).  Results: ptr and len, offsets[npatterns] - offsets[0] U-wide values each, the patterns one after the other in the order
 * given (files <prefix>.ms.ptr / .ms.len); served by pfp_ms_get / _device_ptrs / _write.  Each query replaces the results of the one
 * before it.  info (nullable): patterns, bases; the steps of each kind; breaks and how many of them compared more than the single-lane
 * limit (pfp_debug_set "ms_long_min", bytes) and went to the wave-per-break route; max_len = the largest length.
 * PFP_E_STATE: no index.  PFP_E_TOO_LARGE: 2^32 patterns or more, or more bases than U holds.  PFP_E_ARG: bases or offsets NULL,
 * offsets that descend, a 0 byte in a pattern.  PFP_E_NOMEM leaves the context as it was, without results: a query takes 2 * U bytes
 * per base for the results and, while it runs, 2 * U + 1 per base, 12 per pattern and U + 16 per break of scratch.  The default
 * workspace is sized by the text (pfp_create: 96 bytes per base of it), so a batch with more bases than the text has wants a context
 * created with workspace_bytes to match, or is cut into several queries. */
typedef struct pfp_ms_info { uint64_t patterns, bases, match, up, down, absent, breaks, long_breaks, max_len; } pfp_ms_info;
int pfp_ms_index(pfp_ctx *ctx);
int pfp_ms_query(pfp_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t npatterns, pfp_ms_info *info /* nullable */);
/* The same for the records of a FASTA / FASTQ file (plain or gzip, "-" = stdin), read on the host with the record rules of
 * pfp_parse_feed_fasta_file: one pattern per record, in file order; the whole file is held in host memory before the one query is
 * made (a caller with more reads than that allows cuts them into several files or calls pfp_ms_query).  PFP_E_IO: the file cannot be
 * opened, a read fails or the gzip stream is damaged.  pfp_ms_offsets_get: where
 * the patterns of the last query start in ptr / len -- npatterns + 1 values, the last one their total (file <prefix>.ms.off, U-wide
 * there); either pointer may be NULL.  PFP_E_STATE: no query yet. */
int pfp_ms_query_file(pfp_ctx *ctx, const char *path, pfp_ms_info *info /* nullable */);
int pfp_ms_offsets_get(pfp_ctx *ctx, uint64_t *offsets, uint64_t *npatterns);
int pfp_ms_get(pfp_ctx *ctx, void *ptr, void *len);            /* host copies, offsets[npatterns] - offsets[0] U-wide values each (NULL skips) */
int pfp_ms_device_ptrs(pfp_ctx *ctx, const void **d_ptr, const void **d_len);      /* NULL: no query yet */
int pfp_ms_write(pfp_ctx *ctx, int fd_ptr, int fd_len);        /* like pfp_thresholds_write (-1 skips one) */

/* ---- count and locate queries -------------------------------------------------------------------- */
/* The two questions the run-boundary samples of an r-index exist for (Gagie, Navarro, Prezza, JACM 2020): how often does a pattern
 * occur in the text, and where.  Answered on the device from the run-length BWT and .ssa / .esa alone: neither the text nor the
 * thresholds are needed, so both also work in a context filled by pfp_bwt_load, and a build without a resident SA (-r only) locates
 * through the samples.  DESIGN.md section 2.
 * Definitions.  T, n, the n + 1 rows of T$, BWT, SA, .ssa, .esa, run k, start[k], end[k] = esa[2k], head[k], sval[k], eval[k] and
 * lfhead[k] as in the matching-statistics section.  Patterns are byte strings, normalised exactly as pfp_ms_query does (upper-cased;
 * with PFP_FLAG_NON_ACGT_TO_A every byte outside ACGT becomes 'A'); a 0 byte after normalisation is refused.  An occurrence is an
 * occurrence in T as a byte string: the w pad 'A's between the records are text like any other.
 * Interval.  [lo, hi) = the rows whose suffix starts with P, cnt = hi - lo.  An empty pattern has cnt = 0 and no values.  Else from
 * lo = 0, hi = n + 1, for i = m-1 .. 0 with c = P[i]: LFc(row) for a row <= n of run k is lfhead[k] + (row - start[k]) when head[k] == c,
 * otherwise lfhead of the first run of c behind k, and without such a run the end of c's segment (lfhead of the first run of the next
 * symbol that has runs, or n + 1).  lo' = LFc(lo); with t = hi - 1 and k_t its run, hi' = LFc(t) + (head[k_t] == c ? 1 : 0) -- row
 * n + 1 is never looked up.  When c heads no run or lo' >= hi', cnt = 0 and the pattern is done.
 * Toehold (locate).  top = SA of row hi - 1: eval[r-1] at the start; in a step with c, top -= 1 when head[k_t] == c, otherwise top =
 * eval[kp] - 1 for kp = the last run of c in front of k_t (there is one exactly when the new interval is not empty).
 * phi.  For a text position p = SA[i] of a row i > 0, phi(p) = SA[i-1] = eval[j-1] + (p - sval[j]) for the run j whose sval[j] is the
 * largest <= p among the run starts.  Run 0 is row 0 (value n); no walk steps down from row 0.
 * Reported rows.  max_occ == 0: all of [lo, hi); otherwise the LAST min(cnt, max_occ) rows, [hi - min(cnt, max_occ), hi).  Their SA
 * values are written in row order (= the lexicographic order of the suffixes), U-wide, the patterns one after the other; cnt is
 * always the true count.  The reported rows of a pattern are cut at run borders into PIECES; the last row of a piece has a known
 * value (the run's end sample, or the toehold) and phi yields the rows above it.
 *
 * pfp_ri_index builds the index: its OWN copies of lfhead, head, the sorted runs with the 257 borders and the run directory (as
 * pfp_ms_index without the threshold rows; pfp_debug_set "ms_dir_log2" applies) -- r * (U + 5) + 4 * ((n + 1) >> B) bytes again when a
 * matching-statistics index exists too, which is cheaper to reason about than shared lifetimes -- and the phi structure: the run
 * starts sorted by sval with the end sample of the run in front (2 * r * U bytes) and a block directory over text positions, 4 *
 * (((n >> PB)) + 2) bytes, PB = floor(log2((n + 1) / r)) (pfp_debug_set "ri_dir_log2").  32 * r bytes more while it is built.  Needs
 * pfp_bwt_build(want_rssa = 1) over the whole output, want_sa either value; no text, no thresholds.  The index lives until the next
 * build or reset and coexists with every other post-pass result, in any call order; a second call replaces it.
 * PFP_E_STATE: no build; no run samples; a slice; a run headed by the EndOfWord byte (as pfp_ms_index: such a .bwt is not the BWT of
 * T).  PFP_E_TOO_LARGE: 2^32 runs or more.  PFP_E_CORRUPT: the sval are not r distinct positions <= n that include 0.  PFP_E_NOMEM
 * leaves the build and every other result as they were; there is no count / locate index then, also when one existed before the
 * call (a call gives the space of the previous index back before it allocates).
 *
 * pfp_ri_count / pfp_ri_locate: patterns as for pfp_ms_query (npatterns == 0 is valid).  Results: cnt, npatterns U-wide values (file
 * <prefix>.cnt / <prefix>.loc.cnt); locate also pos, the reported values (<prefix>.loc.pos), and 64-bit offsets into pos kept on the
 * host, npatterns + 1 values (pfp_ri_offsets_get; <prefix>.loc.off) -- their sum over the patterns can exceed what a 32-bit uint_t
 * holds.  A query replaces the results of the one before it; after a count there is no pos (PFP_E_STATE from pfp_ri_get(pos),
 * pfp_ri_offsets_get and pfp_ri_write(fd_off / fd_pos)).
 * Route of locate (pfp_debug_set "ri_route"): 0 = the reported rows are copied from the resident SA when the build has one
 * (want_sa), else walked by phi; 1 = phi always; 2 = the SA, PFP_E_STATE without one.  Both give identical arrays.
 * info (nullable): patterns, bases; found = patterns with cnt > 0; occurrences = the sum of cnt; reported = values in pos; pieces;
 * max_count = the largest cnt; route = 1 phi, 2 SA, 0 count only; on the phi route max_piece = the rows of the longest piece and
 * phi_steps = reported - pieces (both 0 on the SA route; all of reported .. phi_steps 0 after a count).
 * PFP_E_STATE: no index.  PFP_E_TOO_LARGE: 2^32 patterns or more.  PFP_E_ARG: bases or offsets NULL, offsets that descend, a 0 byte
 * in a pattern.  PFP_E_NOMEM leaves build and index as they were, without results; pfp_workspace_needed then reports the demand.  A
 * query takes U bytes per pattern and U per reported value for the results and, while it runs, 1 byte per base, U + 12 per
 * pattern (count) or 2 * U + 32 per pattern (locate) and 16 bytes per 4096 patterns of scratch; a piece costs no memory.  A pattern
 * such as a single base reports a large part of the text: call pfp_ri_count first and size the workspace from its counts, or cap
 * the reported rows with max_occ. */
typedef struct pfp_ri_info { uint64_t patterns, bases, found, occurrences /* sum of cnt */, reported, pieces, max_count, max_piece, phi_steps, route /* 1 phi, 2 SA, 0 count only */; } pfp_ri_info;
int pfp_ri_index(pfp_ctx *ctx);
int pfp_ri_count(pfp_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t npatterns, pfp_ri_info *info /* nullable */);
int pfp_ri_locate(pfp_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t npatterns, uint64_t max_occ, pfp_ri_info *info /* nullable */);
/* the records of a FASTA / FASTQ file as patterns, read like pfp_ms_query_file; locate == 0: count */
int pfp_ri_query_file(pfp_ctx *ctx, const char *path, int locate, uint64_t max_occ, pfp_ri_info *info /* nullable */);
int pfp_ri_offsets_get(pfp_ctx *ctx, uint64_t *offsets /* npatterns + 1, 64-bit */, uint64_t *npatterns);      /* either may be NULL */
int pfp_ri_get(pfp_ctx *ctx, void *cnt, void *pos);            /* host copies, U-wide (NULL skips); pos: PFP_E_STATE after a count */
int pfp_ri_device_ptrs(pfp_ctx *ctx, const void **d_cnt, const void **d_pos);      /* NULL: not made */
int pfp_ri_write(pfp_ctx *ctx, int fd_cnt, int fd_off, int fd_pos);   /* like pfp_ms_write (-1 skips one); off: 64-bit values */

/* ---- document listing ------------------------------------------------------------------------------ */
/* The third query of an r-index next to count and locate: in which records (documents) of the collection does a pattern occur, and
 * how often in each.  Over a pangenome a read occurs about once per haplotype; the caller wants the haplotypes, not a thousand text
 * positions per read.  Search and locate run as for pfp_ri_locate, the positions stay in scratch on the device, and only the
 * (document, frequency) pairs are results.  DESIGN.md section 2.
 * Definitions.  T, n, patterns, normalisation and the interval [lo, hi) with cnt = hi - lo are exactly as for pfp_ri_count.
 * Documents.  starts = the record starts b_0 = 0 < b_1 < ... < b_{ndocs-1} < n, as for pfp_doc_array (pfp_parse_doc_get, the values of
 * .docs, or any coarser table: merged records are one document); b_ndocs = n.  doc(s) = max{k : b_k <= s}.
 * Attribution.  An occurrence of P (length m) at text position s belongs to doc(s), the document of its first byte.
 * PFP_DL_INSIDE.  An occurrence counts only when it lies inside its document without touching the pad: s + m <= b_{doc(s)+1} - w.
 * The others are counted in info->outside and nowhere else.  Without the flag every occurrence counts, also those that run across
 * the w pad 'A's into the next record.
 * max_count.  When max_count != 0, a pattern with cnt > max_count is skipped: it gets no pairs, cnt still holds its true count, and
 * it is counted in info->skipped -- the guard against a read inside a 10 M run of N.  0 = no limit.
 *
 * Results.  cnt: npatterns U-wide values, the true number of occurrences whatever flags and max_count say, bit-identical to
 * pfp_ri_count (<prefix>.dl.cnt).  doc and freq: `entries` U-wide values each (<prefix>.dl.doc / .dl.freq); pattern j owns the slice
 * [doc_off[j], doc_off[j+1]): doc = the distinct documents with at least one counting occurrence, strictly ascending, freq = the
 * number of counting occurrences in each, >= 1.  For a listed pattern the sum of freq is cnt minus that pattern's outside
 * occurrences.  doc_off: 64-bit, npatterns + 1 values kept on the host like the offsets of pfp_ri_locate (<prefix>.dl.off).  An
 * empty pattern, a pattern with cnt = 0 and a skipped pattern have empty slices.
 * info (nullable): patterns, bases, found, occurrences as in pfp_ri_info; listed = patterns with at least one pair; skipped, outside
 * as above; entries = pairs in all; max_docs = the longest slice; chunks, by_wave, by_table, by_sort as below; route = 1 phi, 2 SA
 * (pfp_debug_set "ri_route" applies as for pfp_ri_locate).
 * Chunks.  The positions never all exist at once.  The patterns are cut, in their given order, into chunks: a chunk takes patterns
 * while the sum of their reported rows (cnt, 0 for a skipped pattern) stays within the budget, and one pattern at least, so a
 * pattern larger than the budget is a chunk of its own.  The budget is pfp_debug_set "dl_chunk_values" (rows); its default is what
 * the workspace leaves free behind the results over the scratch per row below.  info->chunks = the chunks.  Results do not depend on
 * the chunking.
 * Reduction.  The positions of a pattern are mapped to documents by bisection (the table in LDS as for pfp_doc_array) and reduced
 * by one of three routes, all giving identical arrays: by one wave when the pattern reports at most "dl_wave_max" rows (default and
 * most 64); else, when ndocs <= "dl_table_max" (default and most 16384), by one workgroup with ndocs counters in LDS; else by a
 * sort of (pattern, document) keys over the chunk.  0 switches a route off.  by_wave, by_table, by_sort = the patterns of each.
 *
 * The results live in a result slot of their own: they do not replace the results of pfp_ri_count / pfp_ri_locate and those calls
 * do not replace them; they coexist with every other post-pass result in any call order and survive a second pfp_ri_index.  A second
 * pfp_ri_docs replaces them; a build or reset drops them.  Needs pfp_ri_index of the build and nothing else -- no text, no
 * thresholds -- so it also works in a context filled by pfp_bwt_load (w from the context, n from the rows).
 * PFP_E_STATE: no build; no index; a slice; ri_route 2 without a whole SA; from _get / _write / _offsets_get: nothing made.
 * PFP_E_ARG: bases, offsets or starts NULL; offsets that descend; a 0 byte in a pattern; a table that is empty, does not start at 0,
 * does not strictly ascend or reaches n; unknown flag bits.  PFP_E_TOO_LARGE: 2^32 patterns or documents or more; a chunk of 2^32
 * rows or more on the sort route (one pattern with that many occurrences: use max_count).  PFP_E_NOMEM leaves the build, the index
 * and every other result as they were and no listing; pfp_workspace_needed then reports the demand.
 * Memory.  Results: npatterns * U for cnt and, at the peak, 2 * U * sum over the listed patterns of min(cnt, ndocs) for doc and freq --
 * the upper bound is allocated, the slices are written tight and the unused tail is given back, so the slot ends at 2 * U * entries.
 * Scratch while the call runs: 1 byte per base, 3 * U + 12 per pattern and ndocs * U; on top of that for the chunk at hand 41 bytes
 * per pattern, U + 4 per reported row, 8 per slot of its upper bound (min(cnt, ndocs) per pattern), and 36 more per row and 8 more
 * per pattern when a pattern of the chunk takes the sort route.  The default budget divides the free workspace by U + 48. */
#define PFP_DL_INSIDE 1u
typedef struct pfp_dl_info { uint64_t patterns, bases, found, occurrences, listed, skipped, outside, entries,
                             max_docs, chunks, by_wave, by_table, by_sort, route; } pfp_dl_info;
int pfp_ri_docs(pfp_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t npatterns,
                const uint64_t *starts, uint64_t ndocs, unsigned flags, uint64_t max_count, pfp_dl_info *info /* nullable */);
/* the records of a FASTA / FASTQ file as patterns, read like pfp_ms_query_file */
int pfp_ri_docs_file(pfp_ctx *ctx, const char *path, const uint64_t *starts, uint64_t ndocs, unsigned flags, uint64_t max_count, pfp_dl_info *info /* nullable */);
int pfp_ri_docs_offsets_get(pfp_ctx *ctx, uint64_t *doc_off /* npatterns + 1, 64-bit */, uint64_t *npatterns);   /* either may be NULL */
int pfp_ri_docs_get(pfp_ctx *ctx, void *cnt, void *doc, void *freq);            /* host copies, U-wide (NULL skips) */
int pfp_ri_docs_device_ptrs(pfp_ctx *ctx, const void **d_cnt, const void **d_doc, const void **d_freq);      /* NULL: not made */
int pfp_ri_docs_write(pfp_ctx *ctx, int fd_cnt, int fd_off, int fd_doc, int fd_freq);   /* like pfp_ri_write (-1 skips one); off: 64-bit values */

/* ---- maximal exact matches ------------------------------------------------------------------------ */
/* What matching statistics over a pangenome are computed for: the maximal exact matches (MEMs) of every pattern, as seeds, and
 * where else each of them occurs.  Found on the device from what the last pfp_ms_query / pfp_ms_query_file of the context left
 * there: len decides maximality, ptr names one occurrence in the resident text -- so the bytes of a MEM are T[ptr .. ptr + len) and
 * no pattern is kept or uploaded again -- and the count / locate index turns that into the row interval and all positions.
 * DESIGN.md section 2.
 * Definitions.  T, n, patterns, normalisation, ptr and len as in the matching-statistics section.  Patterns are numbered j = 0 ..
 * np - 1; pattern j is the global positions [off[j], off[j+1]) of that query.  For a pattern P of length m a MEM is a pair (i, l)
 * with l >= max(min_len, 1) such that P[i .. i+l) occurs in T, cannot be extended to the left (i == 0 or P[i-1 .. i+l) does not
 * occur) and cannot be extended to the right (i + l == m or P[i .. i+l+1) does not occur).  On the matching statistics: position i
 * starts a MEM iff len[i] >= max(min_len, 1) and (i is the first base of its pattern or len[i-1] <= len[i]); its length is len[i] and
 * ptr[i] is one occurrence.  (The last base of a pattern has len <= 1, so the comparison holds at every pattern start with len >= 1.)
 * As for count / locate, an occurrence is an occurrence in T as a byte string: the w pad 'A's between the records are text like any
 * other.  MEMs are listed pattern after pattern, by ascending start within a pattern; their ends ascend too.
 *
 * pfp_mem_find: min_len == 0 means 1.  Results: start, len, ptr -- `mems` U-wide values each: the start of the MEM relative to its
 * pattern and copies of the statistics at that base (files <prefix>.mem.start / .mem.len / .mem.ptr) -- and on the host mem_off,
 * 64-bit: mem_off[j] = the MEMs in front of pattern j, mem_off[np] = mems (<prefix>.mem.off).  With locate != 0 also cnt, `mems`
 * values, the true number of occurrences of every MEM in T (>= 1; <prefix>.mem.cnt), pos, the SA values of the reported rows of every
 * MEM, one MEM after the other, in row order (<prefix>.mem.pos), and on the host pos_off, 64-bit, mems + 1 values
 * (<prefix>.mem.poff).  The reported rows are those of pfp_ri_locate: all of [lo, hi) for max_occ == 0, else the last min(cnt,
 * max_occ).  locate needs pfp_ri_index of the same build; pfp_debug_set "ri_route" selects phi / the resident SA as for pfp_ri_locate
 * and both routes give identical arrays.
 * info (nullable): patterns, bases (of the query); mems; max_len; sum_len = the sum of the MEM lengths = the search steps of a
 * locate; occurrences .. route as in pfp_ri_info, over the MEMs, all 0 when locate == 0.
 * The arrays live in result slots of their own until the next build or reset and coexist with every other post-pass result in any
 * call order.  They are self-contained: a later pfp_ms_query leaves them alone; a second pfp_mem_find replaces them.  After a find
 * with locate == 0 there is no cnt / pos, as after pfp_ri_count: PFP_E_STATE from pfp_mem_get(cnt / pos), pfp_mem_offsets_get(pos_off)
 * and pfp_mem_write(fd_cnt / fd_pos), NULL from pfp_mem_device_ptrs.
 * PFP_E_ARG: NULL ctx.  PFP_E_STATE: no build; no matching-statistics result yet; locate without a count / locate index; ri_route 2
 * without a whole SA; from _get / _write / _offsets_get: nothing made.  PFP_E_TOO_LARGE: 2^32 MEMs or more (MEM indices are 32-bit
 * values in the order array).  PFP_E_NOMEM leaves build, indexes and the matching-statistics result as they were and no MEM result;
 * pfp_workspace_needed then reports the demand.  Memory: results 3 * mems * U bytes, with locate mems * U + reported * U more; while
 * the call runs, scratch of U bytes per base and 16 per pattern, and with locate 4 * U + 28 bytes per MEM (interval, toehold, the
 * two sort buffers of length and index, piece and row sums) and 16 bytes per 4096 MEMs; a piece costs no memory.  A short min_len
 * with max_occ == 0 reports a large part of the text per MEM: raise min_len or cap the reported rows. */
typedef struct pfp_mem_info { uint64_t patterns, bases, mems, max_len, sum_len,
    occurrences, reported, pieces, max_count, max_piece, phi_steps, route; } pfp_mem_info;
int pfp_mem_find(pfp_ctx *ctx, uint64_t min_len, int locate, uint64_t max_occ, pfp_mem_info *info /* nullable */);
int pfp_mem_offsets_get(pfp_ctx *ctx, uint64_t *mem_off /* npatterns+1 */, uint64_t *npatterns,
                        uint64_t *pos_off /* mems+1, locate only */, uint64_t *mems);   /* any may be NULL */
int pfp_mem_get(pfp_ctx *ctx, void *start, void *len, void *ptr, void *cnt, void *pos);  /* U-wide, NULL skips */
int pfp_mem_device_ptrs(pfp_ctx *ctx, const void **d_start, const void **d_len, const void **d_ptr, const void **d_cnt, const void **d_pos);
int pfp_mem_write(pfp_ctx *ctx, int fd_start, int fd_len, int fd_ptr, int fd_cnt, int fd_pos);   /* -1 skips one */

/* ---- marker queries ------------------------------------------------------------------------------- */
/* The one question a marker array is built for (vcf_to_bwt.py: pfbwt-f64 | tee | mps_to_ma): which variant alleles do the occurrences
 * of a read overlap, without locating them.  The marker array is indexed by BWT row and a backward search yields row intervals, so
 * the answer is an intersection of intervals with records: no phi walk, no SA.  DESIGN.md section 2.
 * Definitions.  T, n, the n + 1 rows, BWT, SA, patterns, their normalisation and the row interval [lo, hi) with cnt = hi - lo are
 * exactly as in the count / locate section.
 * Marker array.  A .ma stream (the result of pfp_marker_array, include/marker_array.hpp:138-174) is a sequence of records: first row,
 * last row, marker_1 .. marker_k (k >= 1), 0xFFFFFFFFFFFFFFFF.  Records are ascending and disjoint, first <= last <= n.  Markers are
 * opaque 64-bit values (include/marker.hpp:9-52), compared as unsigned integers.  M(j) = the SET of marker values of the record that
 * holds row j, the empty set when no record holds it; a value repeated inside one list counts once.
 * Probes.  For a pattern P of length m, step i (0 <= i < m) is the suffix P[i .. m); its interval is [lo_i, hi_i), cnt_i = hi_i - lo_i,
 * by the count definition applied to that suffix -- the states the backward search passes through anyway.  min_len == 0: only step
 * 0 (the whole pattern) is a candidate.  min_len = L >= 1: every step with m - i >= L is a candidate (suffixes of a read with
 * mismatches still carry evidence).  A candidate with cnt_i >= 1 is PROBED when max_rows == 0 or cnt_i <= max_rows; a candidate with
 * cnt_i > max_rows is CAPPED: it contributes nothing and is counted in info->capped -- the guard against unspecific suffixes.
 * Result of a pattern.  A list of pairs (X, freq), strictly ascending by X (unsigned 64-bit): freq(X) = the sum over the probed
 * steps i of the number of rows j in [lo_i, hi_i) with X in M(j); only pairs with freq >= 1 are listed.  cnt[j] = cnt_0, bit-identical
 * to pfp_ri_count whatever min_len and max_rows say; probes[j] = the number of probed steps.  An empty pattern has cnt = 0, no probes
 * and no pairs.
 * Text-space equivalent.  With the .mps stream the array was made from, row j holds the list of the mps interval that contains
 * SA[j]; so freq(X) = the sum over the probed steps of the number of occurrences s of P[i .. m) in T whose mps interval lists X.
 * Raw entries of a pattern = the sum over its probed steps, over the records that overlap [lo_i, hi_i), of the size of the record's
 * de-duplicated list.  They drive routes and chunks.
 *
 * pfp_mk_index makes the index, the context's OWN copy of a marker array: with ma == NULL (then ma_words must be 0, else PFP_E_ARG)
 * of the stream that a fused pfp_marker_array of this build left on the device -- PFP_E_STATE with none there (never made, or empty)
 * -- otherwise of the host stream (ma_words == 0 is a valid empty index): the route of builds without a resident SA (-r only,
 * pfp_bwt_load, a .ma written by mps_to_ma elsewhere).  A later pfp_marker_array does not touch the index.  Needs a build over the
 * whole output, not a slice (n comes from the rows), and nothing else: no text, no SA, no samples.  The index lives until the next
 * build or reset and coexists with every other result in any call order; a second call replaces it.  Made on the device: record
 * starts flagged and compacted, a lane per record validates it, the marker values get dense 32-bit ids in ascending value order
 * (a sort of all list entries), and a sort of (record, id) pairs with the heads kept leaves every list as ascending unique ids.
 * info (nullable): records; entries = list entries after de-duplication; distinct = marker values; max_list = the longest list;
 * rows = rows that hold a list.
 * PFP_E_CORRUPT: the stream does not end with the delimiter; a record has no marker; first > last; last > n; first <= the previous
 * last.  PFP_E_TOO_LARGE: 2^32 or more records, list entries (counted before de-duplication) or distinct markers, or a stream of 2^32
 * words or more.  A failing call leaves no marker index and everything else as it was.
 * Memory: 16 bytes per record, 4 per list entry, 8 per distinct marker; while it is made, 8 bytes per word of a host stream, 8 per
 * word and 4 per record of flags and starts, and 40 bytes per list entry (two keys, two values, record, id, flags and their sums).
 *
 * pfp_mk_query needs the marker index and pfp_ri_index of the build (the search is that index's, as for pfp_ri_docs); without
 * either PFP_E_STATE.  Results: cnt and probes, npatterns U-wide values each (<prefix>.mk.cnt / .mk.probes); marker and freq,
 * `entries` 64-bit values each whatever U is (<prefix>.mk.marker / .mk.freq); pattern j owns the slice [mk_off[j], mk_off[j+1]);
 * mk_off: 64-bit, npatterns + 1 values kept on the host (<prefix>.mk.off).  They live in result slots of their own: pfp_ri_count /
 * _locate / _docs, pfp_mem_find, pfp_ms_query and a second pfp_ri_index or pfp_mk_index leave them alone, a second pfp_mk_query
 * replaces them, a build or reset drops them.
 * info (nullable): patterns, bases, found, occurrences as in pfp_ri_info (of the whole patterns); steps = search steps taken;
 * probes, capped as above; rows = the sum of cnt_i over the probes; records = record overlaps of the probes; raw = raw entries;
 * listed = patterns with at least one pair; entries = pairs in all; max_markers = the longest slice; chunks, by_wave, by_sort below.
 * Chunks.  The raw entries never all exist at once.  The patterns are cut, in their given order, into chunks: a chunk takes
 * patterns while the sum of their raw entries stays within the budget, and one pattern at least.  The budget is pfp_debug_set
 * "mk_chunk_entries"; its default is what the workspace leaves free behind the results over 64 bytes per raw entry (not measured).
 * Results do not depend on the chunking.
 * Reduction.  Every raw entry becomes a key (pattern, id) with the weight min(hi, last + 1) - max(lo, first), the rows of the probe
 * inside the record.  A pattern with at most "mk_wave_max" raw entries (default and most 64, 0 = never) is reduced by
 * one wave, a lane per entry; every other one by a sort of the chunk's keys and one 64-bit atomic add per entry.  Both give identical
 * arrays (one measurement, DESIGN.md section 4 "Marker queries": no difference between them on short lists).  by_wave, by_sort = the patterns with raw entries of each route.
 * PFP_E_ARG: bases or offsets NULL, offsets that descend, a 0 byte in a pattern.  PFP_E_TOO_LARGE: 2^32 patterns or more; a chunk of
 * 2^32 raw entries or more (one pattern with that many: use max_rows).  PFP_E_NOMEM leaves the build, the indexes and every other
 * result as they were and no result of this query; pfp_workspace_needed then reports the demand.  From _get / _write / _offsets_get:
 * PFP_E_STATE when nothing is made.
 * Memory.  Results: 2 * U per pattern and, at the peak, 16 bytes times the sum over the patterns of min(raw entries, distinct) --
 * the upper bound is allocated, the slices are written tight and the unused tail is given back, so the slot ends at 16 * entries.
 * Scratch while the call runs: 1 + 2 * U + 12 bytes per base (the pattern, the slot's interval, its first record, the sums of the raw
 * entries), 20 per pattern; for the chunk at hand 37 bytes per pattern, 20 per raw entry, 12 per slot of its upper bound, and 24 more
 * per raw entry and 8 more per pattern when a pattern of the chunk takes the sort route. */
typedef struct pfp_mk_index_info { uint64_t records, entries /* after de-duplication */, distinct, max_list, rows /* rows that hold a list */; } pfp_mk_index_info;
int pfp_mk_index(pfp_ctx *ctx, const uint64_t *ma /* host, nullable */, uint64_t ma_words, pfp_mk_index_info *info /* nullable */);
typedef struct pfp_mk_info { uint64_t patterns, bases, found, occurrences, steps, probes, capped, rows /* sum of cnt_i over the probes */,
    records /* record overlaps */, raw, listed, entries, max_markers, chunks, by_wave, by_sort; } pfp_mk_info;
int pfp_mk_query(pfp_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t npatterns, uint64_t min_len, uint64_t max_rows, pfp_mk_info *info /* nullable */);
/* the records of a FASTA / FASTQ file as patterns, read like pfp_ms_query_file */
int pfp_mk_query_file(pfp_ctx *ctx, const char *path, uint64_t min_len, uint64_t max_rows, pfp_mk_info *info /* nullable */);
int pfp_mk_offsets_get(pfp_ctx *ctx, uint64_t *mk_off /* npatterns + 1, 64-bit */, uint64_t *npatterns);   /* either may be NULL */
int pfp_mk_get(pfp_ctx *ctx, void *cnt, void *probes /* U-wide */, uint64_t *marker, uint64_t *freq /* 64-bit */);      /* host copies (NULL skips) */
int pfp_mk_device_ptrs(pfp_ctx *ctx, const void **d_cnt, const void **d_probes, const void **d_marker, const void **d_freq);      /* NULL: not made */
int pfp_mk_write(pfp_ctx *ctx, int fd_cnt, int fd_probes, int fd_off, int fd_marker, int fd_freq);   /* -1 skips one; off, marker, freq: 64-bit values */

/* ---- drop-ins for the suffix-sorting C ABI, gsa/gsacak.h:76-103 ------------------------------- */
/* int sacak_int(int_text *s, uint_t *SA, uint_t n, uint_t k): s[n-1]==0, symbols < k.  Returns the
 * number of refinement rounds (>= 1; the reference returns its recursion depth) or -1 on error. */
int pfp_sacak_int_u32(const uint32_t *s, uint32_t *SA, uint32_t n, uint32_t k);
int pfp_sacak_int_u64(const uint32_t *s, uint64_t *SA, uint64_t n, uint64_t k);

/* int gsacak(unsigned char *s, uint_t *SA, int_t *LCP, int_t *DA, uint_t n), gsa/gsacak.h:86-96 -- the call made by
 * PrefixFreeBWT::sort_dict_suffixes, include/pfbwt.hpp:211.  s: strings over ANY byte alphabet (the parser's dictionaries use '-', A,
 * C, G, N, T and Dollar = 2 and take the tuned path), each followed by the separator 1, s[n-1] == 0 and no other 0.  SA: suffixes
 * compared up to their separator, byte-identical ones in position order (gsacak.c:877-912); LCP (nullable): stops at the
 * separator (:64), LCP[0] = 0; DA (nullable): index of the string a suffix starts in.  Returns the number of refinement rounds
 * (>= 1; the reference returns its recursion depth) or -1: NULL s / SA as the reference; also n >= 2^32 - 64 in either width (device
 * suffix indices are 32-bit: dictionaries below 4 GiB) and a 0 byte that is not the last one.  The engine itself never
 * materialises LCP (pfp_bwt_build uses class heads instead). */
int pfp_gsacak_u32(const uint8_t *s, uint32_t *SA, int32_t *LCP, int32_t *DA, uint32_t n);
int pfp_gsacak_u64(const uint8_t *s, uint64_t *SA, int64_t *LCP, int64_t *DA, uint64_t n);

/* Page-lock / release caller-owned host memory (hipHostRegister): sources of pfp_parse_feed_fasta / pfp_parse_feed_batch and
 * destinations of pfp_bwt_build_stream / pfp_bwt_get then move at the link's rate, and a caller of this C ABI need not link
 * the HIP runtime itself. */
int pfp_host_register(void *p, uint64_t bytes);
int pfp_host_unregister(void *p);

/* library build info: "hip-gfx950" for the product library */
const char *pfp_backend(void);

#ifdef __cplusplus
}
#endif
#endif
