/*
 * include/pfbwt_hip_dev.h -- measurement and development entry points of libpfbwt_hip.so.  NOT part of the
 * drop-in boundary (include/pfbwt_hip.h): nothing here stands in for a reference interface; bench.py and
 * tools/ use it for the per-kernel HIP-event timings behind the roofline figures.
 */
#ifndef PFBWT_HIP_DEV_H
#define PFBWT_HIP_DEV_H
#include "pfbwt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- instrumentation ---------------------------------------------------------------------------- */
/* per-kernel timing with hipEvents on the context's stream (off by default) */
int pfp_profile_enable(pfp_ctx *ctx, int on);
/* time only the launches of one kernel (name as reported by pfp_profile_get); keeps event overhead out of a timed run */
int pfp_profile_select(pfp_ctx *ctx, const char *kernel_name);
int pfp_profile_reset(pfp_ctx *ctx);
/* idx-th record: kernel name, launches, total ms, algorithmic bytes; returns 0 or PFP_E_ARG past the end */
int pfp_profile_get(pfp_ctx *ctx, int idx, const char **name, uint64_t *launches, double *ms, double *bytes);
/* wall-clock milliseconds of the last call of each stage (host timer around a stream sync):
 * [0] parse_finalize [1] parse_bwt [2] bwt_build */
int pfp_stage_ms(pfp_ctx *ctx, double out[3]);
/* Route and tuning switches of ONE context (tests force the routes that only huge inputs take; A/B measurements):
 *   verbose, seg_grid, seg_stage, sort_k (1 | 3), sort_no_table, class_sort_maxrange, dedup_table_log2, no_trigger_table,
 *   emit_chunk_rows, fill_subs, sample_cap (< 0: none), no_runaware, big_group_members (< 0: never), force_wide_rows,
 *   fasta_chunk_bytes, ingest_block_bytes, emit_group_rows (0: no group-stationary emission of the special rows; small: most groups left to the row-wise kernel),
 *   no_slot_records (per-slot fields by two gathers: the route of dictionaries with words of 64 Mbase and more),
 *   dict_text_rounds (-1 auto | 0 rank-based dictionary sort only | 1 text rounds forced), int_key_symbols (2 | 3: parse symbols in the initial sort key),
 *   force_run_round (the run round of the dictionary sort even without a long run).
 *   round 4: parse_rec (-1 auto | 0 never | 1 always: suffix sort of the parse through its level-2 prefix-free parse, csrc/recsort.h), parse_rec_p2, parse_rec_min,
 *   parse_rec_depth, parse_rec_tile_rows, parse_rec_table_log2,
 *   parse_rec_merge (1 default: the inverted lists of its assembly are the first-symbol slices of SA(P2), already sorted by the assembly's key, and the rows of a
 *   class are merged by bisection, k_rs_merge | 2: those lists, rows sorted in LDS by k_rs_assemble | 0: lists by a radix sort by word, rows sorted in LDS),
 *   parse_rec_merge_members (1 .. 1023, default 64: most member slots of a class that k_rs_merge ranks by bisection; a batch that holds a larger class is sorted
 *   in LDS -- tests reach that hand-off on small inputs with 2); dict_rec (-1 | 0 | 1: the same for the dictionary, csrc/dictrec.h), dict_rec_p2;
 *   dedup_variant (1: representatives read by the wave together | 0: by every lane | -1 default: 1 for a collection of >= 8 sequences while its first table lasts), dedup_period (workgroups per sequence for the per-XCD column order of
 *   k_dedup_insert: 0 = estimated from the sequences fed, -1 = text order), dedup_chunk (workgroups per column), dedup_phases (!= 0: stage times from inside the kernel on stderr);
 *   dedup_packed (1 default: the trigger scan writes a 2-bit copy of the text and k_dedup_insert hashes / compares clean phrases from it | 0: bytes only);
 *   group_reduce (1 default: run-aware emission reduces the first / last parse row of every group inside k_emit_slots from a per-word table | 0: k_big_mark reads ilist and takes atomics per member);
 *   fill_masks (1 default: in the one-pass run sampling of a run-aware emission whose windows start at multiples of 16 rows, k_fill stores the run masks of the
 *   rows it writes and only the masks around the special rows are recomputed from the bytes | 0: every window's bytes are read back for them),
 *   fill_skip (1 default: k_fill jumps over slots without rows by bisection | 0: it walks them);
 *   scan_waves (1 .. 16, default 16: waves of a workgroup of the table trigger scan that take part -- a test hook: with fewer, the runs of a wave span several groups on a small text);
 *   ingest_readers, expand_dma;
 *   doc_lds_max (2 .. 8192, default 8192: most record starts pfp_doc_array bisects in LDS; a larger table takes the two-level route;
 *   lcp_long_min (16 .. 2^30, rounded up to a multiple of 16, default 512: bytes of a pair of suffixes that one lane of pfp_lcp_array compares on its own before
 *   the pair is queued for a whole wave; tests force the long route on small texts with 16);
 *   thr_long_min (1 .. 2^30, default 128: rows of the gap of a run that one lane of pfp_thresholds scans on its own before the run is queued for a whole
 *   wave), thr_tile (16 .. 2^20, rounded up to a power of two, default 1024: rows per tile minimum of its long route),
 *   thr_window_rows (default 2^30; < 1 selects the default: rows per window of pfp_thresholds_windowed when the caller passes 0),
 *   plcp_block_log2 (-1 default: from n / r, about one run start per block | 0 .. 48: log2 of the text positions per directory block of the
 *   sparse PLCP; tests force one pair per block, dense blocks and a single block);
 *   ms_dir_log2 (-1 default: from (n + 1) / r, about one run per block | 0 .. 48: log2 of the rows per block of the run directory of pfp_ms_index),
 *   ms_long_min (1 .. 2^30, default 512: bytes one lane of pfp_ms_query compares at a break before the break is queued for a whole wave);
 *   ri_dir_log2 (-1 default: from (n + 1) / r, about one run start per block | 0 .. 48: log2 of the text positions per block of the phi directory of
 *   pfp_ri_index), ri_route (0 default: pfp_ri_locate copies the reported rows from the resident SA when the build has one, else walks them by phi |
 *   1: phi always | 2: the SA, PFP_E_STATE without one);
 *   dl_chunk_values (< 1 default: from what the workspace leaves free, not measured | rows: most reported rows per chunk of patterns of
 *   pfp_ri_docs; a pattern with more is a chunk of its own), dl_wave_max (0 .. 64, default 64: most reported rows of a pattern that one
 *   wave reduces; 0 = never), dl_table_max (0 .. 16384, default 16384: most documents reduced in a table of LDS counters; 0 = never;
 *   with both 0 every pattern takes the sort route);
 *   mk_chunk_entries (< 1 default: from what the workspace leaves free, not measured | most raw entries per chunk of patterns of
 *   pfp_mk_query; a pattern with more is a chunk of its own), mk_wave_max (0 .. 64, default 64: most raw entries of a
 *   pattern that one wave reduces; 0 = never: every pattern takes the sort route; below 0 or above 64: 64);
 *   panel_tile (1 .. 512, default 256, < 1 default: kept sites per tile of the site directory of pfp_parse_feed_panel -- one
 *   directory value per (tile, haplotype), everything finer is rebuilt in LDS by the workgroup that needs it), panel_out_bytes (256 ..
 *   2^20, rounded up to a multiple of 16, default 16384, < 1 default: text bytes per workgroup of k_panel_fill), panel_swizzle (default 1:
 *   neighbouring workgroups of k_panel_fill take the same region of neighbouring haplotypes; 0 = text order); none of the three is measured.
 * Returns PFP_E_ARG for an unknown key.  In a process started with PFP_TEST_HOOKS=1 pfp_create presets a new context from the
 * environment variables PFP_<KEY IN UPPER CASE>; without PFP_TEST_HOOKS=1 the environment is ignored (PFP_VERBOSE excepted,
 * which only prints). */
int pfp_debug_set(pfp_ctx *ctx, const char *key, long long value);
/* development aid: sorts n < 2^32 pseudo-random (key, value) pairs with `bits` significant key bits, returns the best
 * wall time of `reps` >= 1 runs, the number of out-of-order neighbours and the number of values that are no index of the
 * input or sit next to another key than the one their index was given (both must be 0; either pointer may be NULL) */
int pfp_debug_sort(pfp_ctx *ctx, uint64_t n, int bits, int reps, double *ms_out, uint32_t *unsorted_pairs, uint32_t *wrong_values);

/* ---- the device-wide primitives of csrc/prims.h on the caller's arrays (tests/test_prims.py) --------------------------
 * Every hook takes host arrays, works in the context's workspace (whatever a build left there is gone afterwards) and calls the
 * primitive unchanged.  Every device buffer of a hook has 256 guard bytes of a pattern in front of and behind its n elements;
 * *guards_changed (required) = the guard bytes that no longer hold the pattern -- for an out-of-place scan also + 1 if the input
 * changed -- and must be 0: a store past the end of an array inside the workspace faults nowhere.  Output elements that the
 * primitive does not write hold 0xEE bytes. */
/* out[0] RS_TILE (pairs per tile of the radix sort; n <= RS_TILE is sorted by one workgroup), out[1] SCAN_TILE (elements per tile
 * of the scans), out[2] SEG_SMALL_MAX (most segments whose column prefixes one workgroup makes), out[3] the default seg_grid */
int pfp_debug_prims_geometry(uint32_t out[4]);
/* The groups of special rows that were too long for a batch of k_emit_groups and were sorted in LDS by k_emit_groups_large, one
 * group per workgroup turn: out[0] groups taken from the list of the groups of at most out[2] rows, out[1] from the list of the
 * groups of at most out[3] rows -- summed over the windows of the context's last emission (a window that is emitted twice counts
 * twice; 0, 0 before the first run-aware emission).  The kernels count on the device; the build never reads the counters back. */
int pfp_debug_emit_large_groups(pfp_ctx *ctx, uint64_t out[4]);
/* radix_sort_pairs<uint32_t | uint64_t> (key_bytes 4 | 8) of n (key, value) pairs by the nranges <= 16 ranges
 * (ranges[2 r], ranges[2 r + 1]) = (lo, hi), least significant first; the arrays that its *rk / *rv name are copied to keys_out /
 * vals_out.  Returns the status of radix_sort_pairs.  Route: pfp_debug_set "seg_grid", "seg_stage". */
int pfp_debug_sort_pairs(pfp_ctx *ctx, const void *keys, int key_bytes, const uint32_t *vals, uint64_t n, const int *ranges, int nranges,
                         void *keys_out, uint32_t *vals_out, uint32_t *guards_changed);
/* n elements of elem_bytes 4 | 8; op 0 exclusive sum, 1 inclusive max.  mode 0: device_scan from one buffer into another,
 * 1: device_scan in place, 2: k_scan_spine alone in place -- ONE workgroup, the exclusive scan for both ops.  *total (NULL: the
 * primitive gets no total pointer) = the sum / the maximum of all elements. */
int pfp_debug_scan(pfp_ctx *ctx, const void *in, int elem_bytes, int op, int mode, uint64_t n, void *out, void *total, uint32_t *guards_changed);
/* device_compact: out[0 .. *count) = in[i] (in == NULL: i) of the i with flag[i] != 0, in order; all n entries of the output
 * buffer are returned, so out[*count .. n) shows what was left alone. */
int pfp_debug_compact(pfp_ctx *ctx, const uint32_t *in, const uint32_t *flag, uint64_t n, uint32_t *out, uint32_t *count, uint32_t *guards_changed);
/* position-weighted checksum of `bytes` bytes of device memory that sit at `global_offset` of a larger logical buffer:
 * out[0..1] = sum over bytes of (byte + 1) * mix_k(global position) mod 2^64.  Checksums of the pieces of a buffer add
 * up (mod 2^64) to the checksum of the whole: tools/big_check_slices.py compares the sliced (multi-GPU) outputs of a
 * 32 Gbase build with the single-context output this way, without moving them off the device. */
int pfp_debug_checksum(pfp_ctx *ctx, const void *d_buf, uint64_t bytes, uint64_t global_offset, uint64_t out[2]);

/* Order check of the run samples against the resident text, at any size: .esa[k] and .ssa[k + 1] are adjacent BWT rows, so
 * T[esa[k].sa ..] < T[ssa[k + 1].sa ..] must hold for all r - 1 pairs (the suffixes are compared byte by byte on the device; the
 * engine's own sort results are not consulted).  Needs the state left by pfp_bwt_build(want_rssa = 1) of a context that still
 * holds its text.  out[0] pairs checked, out[1] order violations, out[2] pairs whose rows are not adjacent, out[3] longest and
 * out[4] sum of the common prefixes. */
int pfp_debug_check_sample_order(pfp_ctx *ctx, uint64_t out[5]);
/* Properties of the full suffix array of the last pfp_bwt_build(want_sa = 1) against the resident text, at any size, without moving
 * it off the device: out[0] rows checked; out[1] values above n; out[2] values that occur twice (with out[1] = 0 and n + 1 rows: the
 * array is a permutation of [0, n]); out[3] rows whose BWT byte is not the text byte in front of SA[row] (0x00 in front of the whole
 * text; row 0 must hold n); out[4] 0x00 bytes in the BWT (must be 1).  What scripts/generate_truth_set.py:92-100 of the reference
 * states about its golden files, checked for a text of any length. */
int pfp_debug_check_sa(pfp_ctx *ctx, uint64_t out[5]);
/* The run samples of a build with want_sa = want_rssa = 1 against its own .bwt and .sa, on the device: run k starts where the BWT
 * byte changes, ends in front of the next start, and carries the SA values of its first and last row (src/pfbwt-f.cpp:304-315, 325-328).
 * out[0] runs checked, out[1] runs with a wrong row, out[2] runs with a wrong value. */
int pfp_debug_check_samples(pfp_ctx *ctx, uint64_t out[3]);
/* The rows the windowed thresholds work on, moved to the host: the SA of the last build window by window (the emission run again into
 * scratch, as pfp_thresholds_windowed does) and the LCP rows worked out from the sparse PLCP -- n + 1 U-wide values each, either
 * pointer may be NULL.  Thresholds only look at minima; this hook shows every value.  Preconditions and errors as for
 * pfp_thresholds_windowed; window_rows >= 1 (not rounded). */
int pfp_debug_rows_windowed(pfp_ctx *ctx, uint64_t window_rows, void *host_sa, void *host_lcp);
/* sum of the 64-bit little-endian words of a device buffer (out[0]) and of word * (word index + 1) (out[1]), modulo 2^64; a
 * trailing partial word is zero-padded.  bench.py checks the outputs that were streamed to host memory against the
 * device-resident ones with it. */
int pfp_debug_wordsum(pfp_ctx *ctx, const void *d_buf, uint64_t bytes, uint64_t out[2]);

#ifdef __cplusplus
}
#endif
#endif
