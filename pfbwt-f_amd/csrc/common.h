// pfbwt-f_amd/csrc/common.h -- context, device arena, launch + profiling helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <sched.h>
#include <string>
#include <thread>
#include <vector>
#include "../../include/pfbwt_hip.h"
#include "devmem.h"
#include "../../include/pfbwt_hip_dev.h"

namespace pfp {

typedef uint32_t idx_t;           // device index type of this build: texts / dictionaries < 2^32

constexpr int BLOCK = 256;        // 4 wave64 per workgroup
constexpr int WAVE = 64;

// Reference constants, include/utils.h:8-10
constexpr uint8_t Dollar = 2, EndOfWord = 1, EndOfDict = 0;

// ---- kernel ids for the profile table ----------------------------------------------------------
enum KernelId {
    K_TRIGGER_SCAN, K_PHRASE_ENDS, K_PHRASE_HASH, K_PHRASE_HASH_LONG, K_DEDUP_HEADS, K_DEDUP_LONG,
    K_DICT_BUILD, K_RADIX_HIST, K_RADIX_SCATTER, K_SCAN_REDUCE, K_SCAN_SPINE, K_SCAN_APPLY,
    K_SS_INIT_KEYS, K_SS_HEADS, K_SS_MAKE_KEYS, K_SS_WRITE_RANK, K_SS_FLAG_ACTIVE, K_COMPACT,
    K_WORD_RANK, K_PARSE_RANKS, K_DICT_SORTED, K_PBWT_ROWS, K_EMIT_COUNT, K_EMIT, K_RUNS, K_SAMPLES, K_MISC, K_EMIT_BIG, K_FILL, K_CLASS_SORT, K_FASTA, K_EMIT_LARGE, K_REC_PARSE, K_REC_DEDUP, K_REC_ASSEMBLE, K_DOC, K_LCP_PAIRS, K_LCP_LONG, K_LCP_GATHER, K_THR_TILES, K_THR_QUERIES, K_THR_LONG, K_PLCP_BUILD, K_LCP_SPARSE, K_RUN_MASKS, K_MS_INDEX, K_MS_POINTERS, K_MS_BREAKS, K_MS_LONG, K_MS_FILL, K_RI_INDEX, K_RI_SEARCH, K_RI_WALK, K_RI_ROWS, K_MEM_LIST, K_MEM_SEARCH, K_DL_MAP, K_DL_WAVE, K_DL_TABLE, K_DL_SORT, K_DL_PACK, K_MK_INDEX, K_MK_SEARCH, K_MK_REDUCE, K_PANEL_CHECK, K_PANEL_DIR, K_PANEL_FILL,
    K_COUNT_
};
static const char *const kernel_names[K_COUNT_] = {
    "trigger_scan", "phrase_ends", "phrase_hash", "phrase_hash_long", "dedup_heads", "dedup_long",
    "dict_build", "radix_hist", "radix_scatter", "scan_reduce", "scan_spine", "scan_apply",
    "ss_init_keys", "ss_heads", "ss_make_keys", "ss_write_rank", "ss_flag_active", "compact",
    "word_rank", "parse_ranks", "dict_sorted", "pbwt_rows", "emit_count", "emit", "runs", "samples", "misc", "emit_big", "fill", "class_sort", "fasta_strip", "emit_large", "rec_parse", "rec_dedup", "rec_assemble", "doc_array", "lcp_pairs", "lcp_long", "lcp_gather", "thr_tiles", "thr_queries", "thr_long", "plcp_build", "lcp_sparse", "run_masks", "ms_index", "ms_pointers", "ms_breaks", "ms_long", "ms_fill", "ri_index", "ri_search", "ri_walk", "ri_rows", "mem_list", "mem_search", "dl_map", "dl_wave", "dl_table", "dl_sort", "dl_pack", "mk_index", "mk_search", "mk_reduce", "panel_check", "panel_dir", "panel_fill"};

struct ProfRec { uint64_t launches = 0; double ms = 0, bytes = 0; };

// Two-ended bump allocator over one address range (devmem.h: physical memory is committed as the two ends advance): results
// of a stage live at the low end, scratch at the high end (released with mark/release).
struct Arena {
    VmRegion vm;
    char *base = nullptr;
    size_t cap = 0, lo = 0, hi = 0, want = 0;
    size_t peak_lo = 0, peak_hi_bytes = 0;      // high-water marks (PFP_VERBOSE)
    bool failed = false;
    void reset() { lo = 0; hi = cap; failed = false; }
    void *alloc_lo(size_t bytes)
    {
        size_t a = (lo + 255) & ~(size_t)255;
        if (a + bytes > hi || !vm.commit(a, a + bytes)) { failed = true; want += bytes; return nullptr; }
        lo = a + bytes; if (lo > peak_lo) peak_lo = lo;
        return base + a;
    }
    void *alloc_hi(size_t bytes)
    {
        size_t b = (bytes + 255) & ~(size_t)255;
        if (b > hi || hi - b < lo || !vm.commit(hi - b, hi)) { failed = true; want += bytes; return nullptr; }
        hi -= b; if (cap - hi > peak_hi_bytes) peak_hi_bytes = cap - hi;
        return base + hi;
    }
    // address space only: the caller commits what it is going to touch (commit_range) -- arrays sized for the worst case of
    // which a fraction is used (run samples: r is not known in advance)
    void *reserve_lo(size_t bytes)
    {
        size_t a = (lo + 255) & ~(size_t)255;
        if (a + bytes > hi) { failed = true; want += bytes; return nullptr; }
        lo = a + bytes;
        return base + a;
    }
    bool commit_range(const void *p, size_t bytes) { const size_t o = (size_t)((const char *)p - base); return vm.commit(o, o + bytes); }
    size_t offset_of(const void *p) const { return (size_t)((const char *)p - base); }
    size_t mark_hi() const { return hi; }
    void release_hi(size_t m) { hi = m; }
    size_t mark_lo() const { return lo; }
    void release_lo(size_t m) { lo = m; }
};

// The result of one post-pass or query of a build (csrc/postpass.h, csrc/queries.h): up to three device arrays at [lo_mark, lo_end) of the arena's low end.
// The results stack there in call order and live until the next build or reset (drop_post_results); PostResult fills a slot.
struct ResultSlot {
    void *p[3] = {nullptr, nullptr, nullptr};
    size_t lo_mark = (size_t)-1, lo_end = 0;
};
// The matching-statistics index of a build (pfp_ms_index; csrc/matchstats.h): r values each -- the threshold rows (a copy), LF of every
// run's first row, the head bytes, the runs in the order of their head bytes -- the 257 borders of the symbols in that order and
// the run directory, one entry per block of 2^B rows plus a closing one.  All null: no index.
struct MsIndex {
    void *thr = nullptr, *lfhead = nullptr; uint8_t *head = nullptr; uint32_t *sorted = nullptr, *sym = nullptr, *dir = nullptr;
    uint32_t B = 0;
};
// The count / locate index of a build (pfp_ri_index; csrc/runindex.h): its own copies of the run arrays above (no thresholds) and the
// phi structure -- the run starts in text order (pq: position, pv: the end sample of the run in front), r values each, and their block
// directory, one entry per block of 2^PB text positions plus two closing ones.  All null: no index.
struct RiIndex {
    MsIndex run; void *pq = nullptr, *pv = nullptr; uint32_t *pdir = nullptr;
    uint32_t PB = 0;
};
// The marker index of a build (pfp_mk_index; csrc/markerquery.h), its own copy of a .ma stream: the records' first and last rows (nrec
// values each), the prefix sums of their list lengths (nrec + 1), the lists as ascending unique ids (entries) and the marker value of
// every id (distinct).  The slot of the context tells whether there is an index: an empty stream makes an index without records.
struct MkIndex {
    uint64_t *first = nullptr, *last = nullptr, *mval = nullptr; uint32_t *loff = nullptr, *lid = nullptr;
    uint64_t nrec = 0, entries = 0, distinct = 0;
};

// Route and tuning switches of a context.  The defaults are the product's; tests and A/B measurements change them with
// pfp_debug_set (include/pfbwt_hip_dev.h) or -- only in a process started with PFP_TEST_HOOKS=1 -- through PFP_<NAME>
// environment variables that pfp_create reads into the new context.  Nothing here is latched per process.
struct Tunables {
    int verbose = 0;                   // PFP_VERBOSE (diagnostics on stderr; honoured without PFP_TEST_HOOKS: it changes no route)
    int seg_grid = 768;                // workgroups per pass of the global radix sort (3 per CU of a 256-CU device)
    int seg_stage = 1;                 // global radix scatter staged through LDS
    int sort_k = 0;                    // 1: plain doubling in every refinement round, 3: three ranks in every round but the run round
    int sort_no_table = 0;             // the K = 3 rounds follow the chains themselves
    uint32_t class_sort_maxrange = 0;  // smaller LDS class-sort ranges (reaches the large-class route on small inputs)
    int dedup_table_log2 = 0;          // a first phrase table that overflows
    int no_trigger_table = 0;          // trigger test by hashing every window
    uint64_t emit_chunk_rows = 3ULL << 30;   // rows per emission window (32-bit offsets inside a window: < 2^32 with room for a straddling group).  2^30 until round 3: every window pays ~0.5 ms of small launches and host round trips (S-32G: 30 windows 96.8 ms, 15 windows 87.1, 8 windows 82.0)
    uint32_t fill_subs = 2;            // super-tiles (4 x 4096 rows) per workgroup of k_fill
    int fill_masks = 1;                // one-pass run samples: k_fill stores the run masks of the rows it writes, k_run_masks_fix recomputes those around the special rows (emit.h); 0 = k_run_tile_count reads the window's bytes back
    int fill_skip = 1;                 // k_fill jumps over the slots without rows by bisection; 0 = walks them, 256 per step
    uint64_t sample_cap = ~0ULL;       // cap of the one-pass run-sample arrays (forces the two-pass fallback)
    int no_runaware = 0;               // -r with every row enumerated, as with a full SA
    long big_group_members = -2;       // -2: BIG_GROUP_MEMBERS (emit.h); < 0 otherwise: never take the sort route
    int force_wide_rows = 0;           // 64-bit row counters on small texts
    uint64_t ingest_block_bytes = 0;   // block size of the file reader (0: 64 MiB)
    int expand_dma = 1;                // pfp_bwt_get_expanded: the copy engine takes blocks from the back while host threads write runs from the front (page-locked destinations)
    int ingest_readers = 0;            // pread threads of the file reader (0: one per CPU, 4 / 8 / 16)
    uint32_t emit_group_rows = 4096;   // rows per batch of the group-stationary emission of the special rows (0: every special row through k_emit; smaller: more groups left to k_emit)
    int dict_text_rounds = -1;         // dictionary suffix sort by text rounds: -1 = when the collection is not repetitive (dictionary > text / 8), 0 never, 1 always
    int force_run_round = 0;           // the run round of the dictionary sort even without a run of 256 equal bytes (tests)
    int int_key_symbols = 3;           // symbols of the parse in the initial sort key: 3 where 3 x symbol bits <= 64 (S-32G: 21-bit symbols, 8 radix passes instead of 6, one refinement round less to pay for: parse BWT 135.7 -> 131.9 ms), else 2
    int no_slot_records = 0;           // k_emit_slots by two gathers (word id | preceding byte, then the word record): the route of dictionaries with words of 64 Mbase and more
    int group_reduce = 1;              // run-aware emission: k_emit_slots reduces the first / last parse row of every group from a per-word table (emit.h, k_pack_wpq); 0 = k_big_mark reads ilist and takes two atomics per member
    uint64_t fasta_chunk_bytes = 0;    // size of the raw-FASTA device buffers (0: 1 MiB ... 256 MiB by the size of the first call)
    int parse_rec = -1;                // suffix sort of the parse through a level-2 prefix-free parse (recsort.h): -1 = when the parse is long and repetitive, 0 never, 1 wherever the route can run
    int parse_rec_p2 = 4;              // its modulus: one symbol in p2 ends a level-2 phrase
    uint64_t parse_rec_min = 1u << 21; // shortest parse that takes it (below: launch latencies, not data, bound either route)
    int parse_rec_depth = 1;           // levels (the names of one level are as long as a second level's dictionary on the collections measured)
    uint32_t parse_rec_tile_rows = 0;  // rows per assembly batch (0: a full LDS tile; smaller: reaches the large-class route on small inputs)
    int parse_rec_merge = 1;           // its assembly (recsort.h): 1 = inverted lists read off SA(P2), rows of a class merged (k_rs_merge); 2 = those lists, rows sorted in LDS (k_rs_assemble); 0 = lists by a sort by word, rows sorted in LDS
    uint32_t parse_rec_merge_members = 64;   // most member slots of a class whose rows k_rs_merge ranks by bisection (1 .. 1023); a batch with a larger class is sorted in LDS
    int dict_rec = -1;                 // suffix sort of the dictionary through a level-2 parse of the dictionary (dictrec.h): -1 = when the collection is repetitive, 0 never, 1 whenever the route can run
    int dict_rec_p2 = 16;              // its modulus (windows of four bytes)
    int dedup_variant = -1;            // k_dedup_insert<COOP> (parse.h): 1 = the representatives read by the wave together, 0 = by every lane for itself (rounds 2-3), -1 = 1 for a collection while its first table lasts
    int64_t dedup_period = 0;          // k_dedup_insert, order of the workgroups (parse.h, DedupOrder): workgroups per sequence; 0 = text workgroups / sequences fed, -1 = text order
    int64_t dedup_chunk = 0;           // workgroups per column (0 = about 32)
    int dedup_packed = 1;              // k_dedup_insert reads the 2-bit shadow of the text the trigger scan writes (parse.h, DedupText); 0 = the bytes only
    int scan_waves = 16;               // waves of a workgroup of the table trigger scan that take part (parse.h; tests: fewer waves = several runs per wave on a small text)
    int dedup_phases = 0;              // != 0: the stages of k_dedup_insert timed inside the kernel and printed (experiments)
    int parse_rec_table_log2 = 0;      // log2 of the level-2 phrase table (tests: a table that overflows -> doubling route)
    uint32_t doc_lds_max = 8192;       // pfp_doc_array: most record starts bisected in LDS (DOC_LDS_CAP, docarray.h); a larger table takes the two-level route
    uint32_t lcp_long_min = 512;       // pfp_lcp_array: bytes one lane compares before a pair is handed to a wave (LCP_LONG_MIN, lcparray.h; a multiple of 16)
    uint32_t thr_long_min = 128;       // pfp_thresholds: rows of a gap one lane scans on its own before the run is handed to a wave (THR_LONG_MIN, thresholds.h)
    uint32_t thr_tile = 1024;          // pfp_thresholds: rows per tile minimum (THR_TILE; a power of two, 16 .. 2^20)
    uint64_t thr_window_rows = 1ULL << 30;   // pfp_thresholds_windowed: rows per SA / LCP window when the caller passes 0 (not measured yet: 17 bytes per row of scratch with 64-bit values)
    int ms_dir_log2 = -1;              // pfp_ms_index: log2 of the rows per block of the run directory; -1 = floor(log2((n + 1) / r)), about one run per block (tests: 0 .. MS_DIR_LOG2_MAX, matchstats.h)
    uint32_t ms_long_min = 512;        // pfp_ms_query: bytes one lane compares at a break before the break is handed to a wave (MS_LONG_MIN, matchstats.h)
    int ri_dir_log2 = -1;              // pfp_ri_index: log2 of the text positions per block of the phi directory; -1 = floor(log2((n + 1) / r)), about one run start per block (tests: 0 .. RI_DIR_LOG2_MAX, runindex.h)
    int ri_route = 0;                  // pfp_ri_locate: 0 = the reported rows from the resident SA when the build has one, else by phi from the run samples; 1 = phi always; 2 = the SA (PFP_E_STATE without one)
    uint64_t dl_chunk_values = 0;      // pfp_ri_docs: most reported rows per chunk of patterns; 0 = from what the workspace leaves free (queries.h: dl_budget; not measured)
    uint32_t dl_wave_max = 64;         // pfp_ri_docs: most reported rows of a pattern reduced by one wave (0 .. DL_WAVE_MAX, doclist.h; 0 = never)
    uint32_t dl_table_max = 16384;     // pfp_ri_docs: most documents reduced in a table of LDS counters (0 .. DL_TABLE_CAP; 0 = never)
    uint64_t mk_chunk_entries = 0;     // pfp_mk_query: most raw entries per chunk of patterns; 0 = from what the workspace leaves free (queries.h: mk_budget; not measured)
    uint32_t mk_wave_max = 64;         // pfp_mk_query: most raw entries of a pattern reduced by one wave (0 .. MK_WAVE_MAX, markerquery.h; 0 = never; measured once against 0, no difference: DESIGN.md section 4)
    uint32_t panel_tile = 256;         // pfp_parse_feed_panel: kept sites per tile of the site directory (1 .. PANEL_TILE_MAX, panel.h; not measured)
    uint32_t panel_out_bytes = 16384;  // pfp_parse_feed_panel: text bytes per workgroup of k_panel_fill (a multiple of 16, PANEL_OUT_MIN .. 2^20; not measured)
    int panel_swizzle = 1;             // pfp_parse_feed_panel: neighbouring workgroups of k_panel_fill take the same region of neighbouring haplotypes; 0 = text order
    int plcp_block_log2 = -1;          // sparse PLCP (lcparray.h): log2 of the text positions per directory block; -1 = from n / r, about one run start per block (tests: 0 .. PLCP_BLOCK_LOG2_MAX)
};

} // namespace pfp

struct pfp_ctx {
    int w = 10; uint64_t p = 100; unsigned flags = 0; int device = 0;
    hipStream_t stream = nullptr;
    pfp::Arena arena;
    size_t arena_request = 0;
    // error detail
    uint64_t err_pos = 0; int err_ch = 0;
    // --- text staging (device): tb = 16 guard bytes (tb[15] = Dollar) + X + w Dollars + slack
    pfp::VmRegion text;          // address range of tb; committed as the text grows (never re-allocated, never copied)
    uint8_t *tb = nullptr; size_t tb_cap = 0; uint64_t n = 0; uint64_t text_hint = 0; uint64_t nseq = 0 /* sequences fed (a hint for the order in which the de-duplication visits the text) */;
    struct RowViewPending { const uint8_t *src = nullptr; uint64_t count = 0, len = 0, stride = 0; } view;      // pfp_parse_feed_device_view: the text is still the caller's rows (read in place by the trigger scan of pfp_parse_finalize)
    uint64_t left_ctx = 0;       // bytes of left context fed in front of this shard's text (pfp_parse_feed_left_context)
    uint64_t tb_n = 0;           // bytes of tb that hold the text of the current parse (0: none -- merged or loaded state)
    // --- parse results (device, arena low end)
    int stage = 0;             // 0 feeding, 1 parsed, 2 parse-bwt done
    uint64_t m = 0, dwords = 0, dsize = 0;
    uint64_t *d_ye = nullptr;       // m: Y-coordinate of each phrase's last byte (= sai); text positions are 64-bit
    uint32_t *d_pid = nullptr;      // m: phrase -> dictionary word id (D' order)
    uint32_t *d_parse = nullptr;    // m: 1-based ranks
    uint8_t *d_last = nullptr;      // m
    uint8_t *d_dict = nullptr;      // D': dictionary in word-id order (dsize bytes)
    uint32_t *d_ws = nullptr;       // dwords+1 word starts in D'
    uint32_t *d_wordid = nullptr;   // dsize: word id of each D' offset
    uint32_t *d_wrank = nullptr;    // dwords: word id -> 0-based rank (nullptr: identity)
    uint32_t *d_occ = nullptr;      // dwords, by rank
    uint8_t *d_sdict = nullptr;     // sorted .dict image (dsize), by rank
    uint32_t *d_gsa = nullptr;      // dsize: suffix array of D'
    uint8_t *d_sflag = nullptr;     // dsize (text-round sort only): per slot, 1 = the suffix there starts a word
    uint32_t *d_srank = nullptr;    // dsize: per suffix-array SLOT, the first slot of its class of equal suffixes
    uint2 *d_grank = nullptr;       // dsize: { class-head slot, covered-prefix end } of each D' offset (sufsort.h)
    bool gsa_valid = false;
    // --- parse-BWT results
    uint64_t nrows = 0;
    uint8_t *d_bwlast = nullptr; uint32_t *d_ilist = nullptr; uint64_t *d_bwsai = nullptr;
    uint8_t *d_bwl_il = nullptr;    // bwlast in ilist order, bwl_il[k] = bwlast[ilist[k]] (nullptr: not made -- loaded files, 2^29 parse rows or more)
    // --- BWT results
    uint64_t nout = 0, runs = 0, esa_pairs = 0, easy = 0, hard = 0, slice_begin = 0, slice_rows = 0;
    uint8_t *d_bwt = nullptr; void *d_sa = nullptr; void *d_ssa = nullptr; void *d_esa = nullptr;
    bool have_sa = false, have_rssa = false;
    // --- post-pass and query results of the last build (csrc/postpass.h, csrc/queries.h)
    pfp::ResultSlot ma; uint64_t ma_words = 0;      // marker array (pfp_marker_array): p[0] = ma_words 64-bit words
    pfp::ResultSlot da;                             // document arrays (pfp_doc_array): p[0] = da, p[1] = sda, p[2] = eda -- slice_rows, 2 * runs, 2 * esa_pairs U-wide values
    pfp::ResultSlot lcp;                            // LCP arrays (pfp_lcp_array): p[0] = lcp, p[1] = slcp -- slice_rows, 2 * runs U-wide values
    pfp::ResultSlot thr;                            // thresholds (pfp_thresholds, pfp_thresholds_windowed): p[0] = thr, p[1] = tlcp -- 2 * runs U-wide values each
    pfp::ResultSlot msi; pfp::MsIndex msx;          // matching-statistics index (pfp_ms_index): p[0] = the start of its arrays, msx = the arrays
    pfp::ResultSlot ms; uint64_t ms_patterns = 0, ms_bases = 0;      // matching statistics of the last pfp_ms_query: p[0] = ptr, p[1] = len -- ms_bases U-wide values each
    std::vector<uint64_t> ms_off;                   // (host) where every pattern of that query starts in them, and their end: ms_patterns + 1 values
    pfp::ResultSlot rii; pfp::RiIndex rix;          // count / locate index (pfp_ri_index): p[0] = the start of its arrays, rix = the arrays
    pfp::ResultSlot ri; uint64_t ri_patterns = 0, ri_reported = 0; int ri_route = 0;      // the last pfp_ri_count / pfp_ri_locate: p[0] = cnt (ri_patterns U-wide values), p[1] = pos (ri_reported values; null after a count)
    std::vector<uint64_t> ri_off;                   // (host) where the positions of every pattern start in pos, and their end: ri_patterns + 1 values
    pfp::ResultSlot mem; uint64_t mem_patterns = 0, mem_count = 0;      // the MEMs of the last pfp_mem_find: p[0] = start, p[1] = len, p[2] = ptr -- mem_count U-wide values each
    pfp::ResultSlot meml; uint64_t mem_reported = 0;                    // their occurrences (locate only): p[0] = cnt (mem_count values), p[1] = pos (mem_reported values)
    std::vector<uint64_t> mem_off, mem_poff;        // (host) the MEMs in front of every pattern and their number: mem_patterns + 1 values; where the positions of every MEM start in pos: mem_count + 1 values (locate only)
    pfp::ResultSlot dl; uint64_t dl_patterns = 0, dl_entries = 0;      // the last pfp_ri_docs: p[0] = cnt (dl_patterns U-wide values), p[1] = doc, p[2] = freq (dl_entries values each)
    std::vector<uint64_t> dl_off;                   // (host) where the pairs of every pattern start in doc / freq, and their end: dl_patterns + 1 values
    pfp::ResultSlot mki; pfp::MkIndex mkx;          // marker index (pfp_mk_index): p[0] = the start of its arrays, mkx = the arrays
    pfp::ResultSlot mk; uint64_t mk_patterns = 0, mk_entries = 0;      // the last pfp_mk_query: p[0] = cnt, p[1] = probes -- mk_patterns U-wide values each
    pfp::ResultSlot mkl;                            // its pairs: p[0] = marker, p[1] = freq -- mk_entries 64-bit values each
    std::vector<uint64_t> mk_off;                   // (host) where the pairs of every pattern start in marker / freq, and their end: mk_patterns + 1 values
    size_t lo_after_parse = 0, lo_after_pbwt = 0, emit_scratch_mark = 0;
    // --- instrumentation
    bool prof_on = false; int prof_only = -1;      // -1: every kernel is timed, else the one selected (pfp_profile_select)
    pfp::ProfRec prof[pfp::K_COUNT_];
    struct PendingEv { hipEvent_t a, b; int id; double bytes; };
    std::vector<PendingEv> pending;
    std::vector<hipEvent_t> ev_pool;
    double stage_ms[3] = {0, 0, 0};
    int hip_err = 0;
    // --- ingest: pageable host memory goes through two pinned staging buffers, so that the host-side copy of chunk
    //     k + 1 overlaps the DMA of chunk k (pinned sources are copied directly)
    uint8_t *hstage[2] = {nullptr, nullptr}; hipEvent_t hstage_ev[2] = {nullptr, nullptr}; bool hstage_used[2] = {false, false};
    pfp::Tunables tun;
    // --- raw FASTA ingest (csrc/fasta.h): two device buffers for raw chunks (the upload of one overlaps the stripping of the other)
    struct FastaIngest {
        uint8_t *raw[2] = {nullptr, nullptr}; size_t rawcap = 0; bool used[2] = {false, false};
        hipStream_t copy = nullptr; bool copy_ready = false; hipEvent_t ev_copied[2] = {nullptr, nullptr}, ev_free[2] = {nullptr, nullptr};
        uint8_t *tiles = nullptr; size_t tiles_cap = 0;                 // per-tile summaries of one chunk
        unsigned long long *d_tot = nullptr, *h_tot = nullptr;          // device / page-locked host: kept bytes, header starts, end state, flags
        uint32_t state = 2; bool started = false; uint64_t records = 0; // the stream's state machine (2 = at a line start)
        std::vector<uint64_t> rec_raw, rec_pos;                         // records that started in the last pfp_parse_feed_fasta call
    } fa;
    uint8_t *h_bwt = nullptr; void *h_sa = nullptr;                      // pfp_bwt_build_stream: host destinations, filled window by window during the emission
    uint8_t *ing_buf[16] = {};                                           // page-locked blocks of the file reader (csrc/ingest.h)
    uint64_t ing_next_off = 0;
    std::vector<std::string> doc_names; std::vector<uint64_t> doc_starts;   // records of the last pfp_parse_feed_fasta_file(PFP_FASTA_RECORDS)
    uint64_t hash_seed = 0x9E3779B97F4A7C15ULL;
    int num_cus = 0;                    // compute units of the device (asked for when the first table scan is sized)
    uint32_t *d_trigtab = nullptr;      // w <= 10: one bit per k-mer, "wang_hash(kmer) % p == 0" (128 KiB for w = 10; lives in LDS during the trigger scan)
    unsigned long long *d_lgtaken = nullptr;      // groups k_emit_groups_large took from its two lists in the last emission (pfp_debug_emit_large_groups)
};

namespace pfp {

inline hipEvent_t ev_get(pfp_ctx *c)
{
    if (!c->ev_pool.empty()) { hipEvent_t e = c->ev_pool.back(); c->ev_pool.pop_back(); return e; }
    hipEvent_t e; (void)hipEventCreate(&e); return e;
}
inline void prof_collect(pfp_ctx *c)
{
    if (c->pending.empty()) return;
    (void)hipStreamSynchronize(c->stream);
    for (auto &pe : c->pending) {
        float ms = 0; (void)hipEventElapsedTime(&ms, pe.a, pe.b);
        c->prof[pe.id].launches++; c->prof[pe.id].ms += ms; c->prof[pe.id].bytes += pe.bytes;
        c->ev_pool.push_back(pe.a); c->ev_pool.push_back(pe.b);
    }
    c->pending.clear();
}
struct ProfScope {
    pfp_ctx *c; int id; double bytes; hipEvent_t a = nullptr; bool on = false;
    ProfScope(pfp_ctx *c_, int id_, double bytes_) : c(c_), id(id_), bytes(bytes_)
    {
        on = c->prof_on && (c->prof_only < 0 || c->prof_only == id);
        if (on) { a = ev_get(c); (void)hipEventRecord(a, c->stream); }
    }
    ~ProfScope()
    {
        if (on) {
            hipEvent_t b = ev_get(c); (void)hipEventRecord(b, c->stream);
            c->pending.push_back({a, b, id, bytes});
            if (c->pending.size() > 4096) prof_collect(c);
        }
    }
};

// LAUNCH(ctx, kernel-id, algorithmic bytes, kernel, grid, args...)
#define PFP_LAUNCH(ctx, id, bytes, kernel, grid, ...)                                             \
    do {                                                                                          \
        pfp::ProfScope ps_((ctx), (id), (double)(bytes));                                         \
        if ((ctx)->tun.verbose >= 3) { fprintf(stderr, "[pfbwt_hip] launch %s grid %u\n", #kernel, (unsigned)(grid)); fflush(stderr); } \
        hipLaunchKernelGGL(kernel, dim3((unsigned)(grid)), dim3(pfp::BLOCK), 0, (ctx)->stream, __VA_ARGS__); \
        hipError_t le_ = hipGetLastError();            /* a rejected launch (grid, LDS size) must not pass as stale output */ \
        if ((ctx)->tun.verbose >= 3 && le_ == hipSuccess) le_ = hipStreamSynchronize((ctx)->stream);   /* fault hunting: one kernel at a time */ \
        if (le_ != hipSuccess) { (ctx)->hip_err = (int)le_; (ctx)->err_ch = (int)le_;                 \
            fprintf(stderr, "[pfbwt_hip] launch of %s failed: %s (%s:%d)\n", #kernel, hipGetErrorString(le_), __FILE__, __LINE__); \
            return PFP_E_HIP; }                                                                       \
    } while (0)

// the same with an explicit workgroup size
#define PFP_LAUNCH_B(ctx, id, bytes, kernel, grid, block, ...)                                    \
    do {                                                                                          \
        pfp::ProfScope ps_((ctx), (id), (double)(bytes));                                         \
        hipLaunchKernelGGL(kernel, dim3((unsigned)(grid)), dim3((unsigned)(block)), 0, (ctx)->stream, __VA_ARGS__); \
        hipError_t le_ = hipGetLastError();                                                       \
        if (le_ != hipSuccess) { (ctx)->hip_err = (int)le_; (ctx)->err_ch = (int)le_;                 \
            fprintf(stderr, "[pfbwt_hip] launch of %s failed: %s (%s:%d)\n", #kernel, hipGetErrorString(le_), __FILE__, __LINE__); \
            return PFP_E_HIP; }                                                                       \
    } while (0)

#define PFP_HIP(ctx, expr)                                                                        \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) { (ctx)->hip_err = (int)e_; (ctx)->err_ch = (int)e_;                \
            fprintf(stderr, "[pfbwt_hip] %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return PFP_E_HIP; }                                                                   \
    } while (0)

#define PFP_TRY(expr) do { int rc_ = (expr); if (rc_ != PFP_OK) return rc_; } while (0)

// typed arena allocation; on exhaustion the enclosing function returns PFP_E_NOMEM
#define PFP_ALLOC_HI(ctx, ptr, T, count)                                                          \
    do { (ptr) = (T *)(ctx)->arena.alloc_hi(sizeof(T) * (size_t)((count) ? (count) : 1));         \
         if (!(ptr)) return PFP_E_NOMEM; } while (0)
#define PFP_ALLOC_LO(ctx, ptr, T, count)                                                          \
    do { (ptr) = (T *)(ctx)->arena.alloc_lo(sizeof(T) * (size_t)((count) ? (count) : 1));         \
         if (!(ptr)) return PFP_E_NOMEM; } while (0)

// A stage that fails (PFP_E_NOMEM, PFP_E_INVALID_CHAR, ...) must leave the workspace as it found it, so that the
// natural retry (a cheaper request, a larger workspace) does not start from a leaked high-water mark.
struct ArenaGuard {
    pfp_ctx *c; size_t lo, hi; bool armed = true;
    explicit ArenaGuard(pfp_ctx *c_) : c(c_), lo(c_->arena.lo), hi(c_->arena.hi) {}
    int done(int rc)
    {
        if (rc != PFP_OK && armed && c->arena.base) { (void)hipStreamSynchronize(c->stream); c->arena.lo = lo; c->arena.hi = hi; c->arena.failed = false; }
        return rc;
    }
};

inline unsigned nblocks(uint64_t items, uint64_t per_block) { return (unsigned)((items + per_block - 1) / per_block); }
inline int bits_for(uint64_t maxval) { int b = 1; while (b < 64 && (maxval >> b)) ++b; return b; }

// A post-pass fills its slot: opening gives the previous result back when it is on top of the low stack, forgets it either way
// and notes where the new one starts; commit() publishes the new arrays.  Without a commit (any failure on the way) the slot stays
// empty, and the ArenaGuard of the entry has the space.
struct PostResult {
    pfp_ctx *c; ResultSlot &s; size_t mark;
    PostResult(pfp_ctx *c_, ResultSlot &s_) : c(c_), s(s_)
    {
        if (s.lo_mark != (size_t)-1 && c->arena.lo == s.lo_end) c->arena.release_lo(s.lo_mark);
        s = ResultSlot();
        mark = c->arena.mark_lo();
    }
    void commit(void *p0, void *p1 = nullptr, void *p2 = nullptr) { s.p[0] = p0; s.p[1] = p1; s.p[2] = p2; s.lo_mark = mark; s.lo_end = c->arena.mark_lo(); }
    // a result with the slot `top` stacked on it ends where that one begins, so that the two are given back one after the other
    void commit_under(const PostResult &top, void *p0, void *p1 = nullptr, void *p2 = nullptr) { commit(p0, p1, p2); s.lo_end = top.mark; }
};
// a build or a reset takes the low end back: no post-pass result outlives it
inline void drop_post_results(pfp_ctx *c) { c->ma = c->da = c->lcp = c->thr = c->msi = c->ms = ResultSlot(); c->ma_words = 0; c->msx = MsIndex(); c->ms_patterns = c->ms_bases = 0; c->ms_off.clear();
    c->rii = c->ri = ResultSlot(); c->rix = RiIndex(); c->ri_patterns = c->ri_reported = 0; c->ri_route = 0; c->ri_off.clear();
    c->mem = c->meml = ResultSlot(); c->mem_patterns = c->mem_count = c->mem_reported = 0; c->mem_off.clear(); c->mem_poff.clear();
    c->dl = ResultSlot(); c->dl_patterns = c->dl_entries = 0; c->dl_off.clear();
    c->mki = c->mk = c->mkl = ResultSlot(); c->mkx = MkIndex(); c->mk_patterns = c->mk_entries = 0; c->mk_off.clear(); }

// CPUs this process can really use: the affinity mask, capped by the cgroup's CPU quota (a one-GPU job of the pool sees 256 CPUs and
// may use 16 of them: 64 writer threads on such a box throttle each other)
static int usable_cpus()
{
    cpu_set_t cs; CPU_ZERO(&cs);
    int n = sched_getaffinity(0, sizeof cs, &cs) == 0 ? CPU_COUNT(&cs) : (int)std::thread::hardware_concurrency();
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {      // cgroup v2: "<quota> <period>" or "max <period>"
        char q[32]; long period = 0;
        if (fscanf(f, "%31s %ld", q, &period) == 2 && strcmp(q, "max") && period > 0) { const long cpus = (atol(q) + period - 1) / period; if (cpus >= 1 && cpus < n) n = (int)cpus; }
        fclose(f);
    }
    return n < 1 ? 1 : n;
}

struct HostTimer {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

} // namespace pfp
