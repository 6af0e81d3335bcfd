// pfbwt-f_amd/csrc/pfbwt_hip.hip -- the C ABI of include/pfbwt_hip.h: the context and its memory (workspace, text buffer), the route
// and tuning switches, and the include list -- the kernels (parse.h / sufsort.h / emit.h / prims.h / ...) and, stage by stage, the host
// code that orchestrates them (*_host.h, postpass.h, queries.h, hooks.h, sharded.h), each with the entries of the ABI it implements.
// Built by hipcc into pfbwt-f_amd/lib/libpfbwt_hip.so.  There is no CPU fallback in this library.
#include "common.h"
#include "prims.h"
#include "parse.h"
#include "fasta.h"
#include "sufsort.h"
#include "recsort.h"
#include "dictrec.h"
#include "emit.h"
#include "markers.h"
#include "docarray.h"
#include "lcparray.h"
#include "thresholds.h"
#include "matchstats.h"
#include "runindex.h"
#include "mems.h"
#include "doclist.h"
#include "markerquery.h"
#include "panel.h"
#include "vcfread.h"
#include <algorithm>
#include <functional>
#include <map>

using namespace pfp;

#ifndef PFP_BACKEND_NAME
#define PFP_BACKEND_NAME "hip-gfx950"
#endif

// -------------------------------------------------------------------------------------------------
// The workspace is an ADDRESS range of `want` bytes (what the stages of a text of n_hint bytes could ask for, at most 15/16 of
// the card); HBM is committed only where the two ends of the arena really get to (csrc/devmem.h).
static int ensure_arena(pfp_ctx *c, uint64_t n_hint)
{
    size_t want = c->arena_request ? c->arena_request : (size_t)(96ULL * n_hint + (64ULL << 20));
    if (!c->arena_request) {   // never ask for more than the device can give (large inputs run with what there is)
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess) {
            const size_t avail = fr + c->arena.vm.committed;
            const size_t cap = avail - avail / 16;
            if (want > cap) want = cap;
        }
    }
    want &= ~(size_t)4095;     // both ends of the arena hand out 256-byte aligned blocks
    if (c->arena.base && c->arena.cap >= want) return PFP_OK;
    // a larger range for a context that already has one (the same context parsed a shard and now merges all of them): the new range
    // is reserved BEFORE the old one is given back, so that it never sits at the addresses kernels of this process used a moment ago
    // (seen on the MI355X box: memory access faults / garbage in the stages behind such a re-reservation at the same address)
    VmRegion nv;
    if (nv.reserve(want, c->device) != hipSuccess) { c->arena.want = want; return PFP_E_NOMEM; }
    if (c->arena.base) { PFP_HIP(c, hipStreamSynchronize(c->stream)); (void)hipDeviceSynchronize(); c->arena.vm.destroy(); c->arena.base = nullptr; c->arena.cap = 0; }
    c->arena.vm = nv; nv.base = nullptr;
    c->arena.base = c->arena.vm.base; c->arena.cap = want; c->arena.reset();
    return PFP_OK;
}

// The text buffer: 16 guard bytes + text + w Dollars + slack for whole trigger-scan tiles.  Its address range is reserved once
// (text_hint bytes if the caller announced a size with pfp_parse_reserve, else four times the first feed, doubled when outgrown) and
// committed as the text grows: feeding record by record rarely moves the text and never re-allocates piecemeal.
static int ensure_text(pfp_ctx *c, uint64_t need_n)
{
    const size_t need = 16 + (((size_t)need_n + 4095) / 4096) * 4096 + 4096 + 64;
    if (c->tb && c->tb_cap >= need) return PFP_OK;
    if (!c->text.live() || need > c->text.va_bytes) {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); tot = (size_t)1 << 38; }
        // An announced size (pfp_parse_reserve: the file reader knows the file's size) is reserved as it is.  Without one the range
        // is four times what the first feed needs (at least 64 MiB) and doubles when the text outgrows it: the text is then moved, a
        // device-to-device copy that costs less than 1 ms per GB and at most twice the text in total.  (Until round 3 every context
        // reserved the card's whole size and therefore committed HBM in 2 GiB pieces: a 100-byte text of a test created, mapped and
        // unmapped 2 GiB -- thousands of such contexts per process are what the rare host-side crashes inside pfp_destroy on the
        // GPU box point at.)
        size_t va = c->text_hint ? (size_t)c->text_hint + (size_t)c->text_hint / 8 + ((size_t)64 << 20) : (4 * need > ((size_t)64 << 20) ? 4 * need : ((size_t)64 << 20));
        if (!c->text_hint && c->text.live() && va < 2 * c->text.va_bytes) va = 2 * c->text.va_bytes;
        if (!c->text_hint && va > tot && tot > need + need / 4) va = tot;
        if (va < need) va = need + need / 4;
        VmRegion nr;
        if (nr.reserve(va, c->device) != hipSuccess) return PFP_E_NOMEM;
        if (c->tb) {      // the announced size was too small: move to a larger range (the one case in which text is copied)
            if (!nr.commit(0, 16 + (size_t)c->n)) { nr.destroy(); return PFP_E_NOMEM; }
            PFP_HIP(c, hipMemcpyAsync(nr.base, c->tb, 16 + (size_t)c->n, hipMemcpyDeviceToDevice, c->stream));
            PFP_HIP(c, hipStreamSynchronize(c->stream));
            c->text.destroy();
        }
        c->text = nr; nr.base = nullptr;
        c->tb = (uint8_t *)c->text.base; c->tb_cap = 0;
    }
    if (!c->text.commit(0, need)) return PFP_E_NOMEM;
    c->tb_cap = c->text.vmm ? (c->text.lo_edge < c->text.va_bytes ? c->text.lo_edge : c->text.va_bytes) : c->text.va_bytes;
    return PFP_OK;
}

static void reset_results(pfp_ctx *c)
{
    c->stage = 0; c->n = 0; c->nseq = 0; c->tb_n = 0; c->left_ctx = 0; c->view.src = nullptr; c->m = c->dwords = c->dsize = 0; c->nrows = 0; c->nout = c->runs = c->esa_pairs = 0;
    c->gsa_valid = false; c->d_wrank = nullptr; c->d_bwt = nullptr; c->d_sa = c->d_ssa = c->d_esa = nullptr;
    c->d_bwlast = nullptr; c->d_ilist = nullptr; c->d_bwsai = nullptr; c->d_bwl_il = nullptr;
    drop_post_results(c);
    c->d_ye = nullptr; c->d_pid = nullptr; c->d_parse = nullptr; c->d_last = nullptr; c->d_dict = nullptr; c->d_ws = nullptr; c->d_wordid = nullptr;
    c->d_occ = nullptr; c->d_sdict = nullptr; c->d_gsa = nullptr; c->d_grank = nullptr; c->d_srank = nullptr; c->d_sflag = nullptr;
    c->arena.reset();
    c->fa.started = false; c->fa.state = 2; c->fa.records = 0; c->fa.rec_raw.clear(); c->fa.rec_pos.clear();
}

// ---- route / tuning switches (pfbwt_hip_dev.h) -----------------------------------------------------
// One row per switch: its name -- the key of pfp_debug_set and, in capitals behind PFP_, its environment variable -- and what storing a
// value does (clamps, roundings and the defaults that stand in for "not set").  A switch is a field of Tunables (common.h) and a row here.
struct TunableRow { const char *name; void (*store)(Tunables &t, long long v); };
#define PFP_SWITCH(field, value) {#field, [](Tunables &t, long long v) { t.field = value; }}
static uint32_t pow2_from_16_to_1m(long long v) { uint32_t p2 = 16; while (p2 < (1u << 20) && (long long)p2 < v) p2 *= 2; return p2; }      // rounded up to a power of two
static const TunableRow tunable_table[] = {
    PFP_SWITCH(verbose, (int)v),
    PFP_SWITCH(seg_grid, (int)v),
    PFP_SWITCH(seg_stage, (int)v),
    PFP_SWITCH(sort_k, (int)v),
    PFP_SWITCH(sort_no_table, (int)v),
    PFP_SWITCH(class_sort_maxrange, (uint32_t)v),
    PFP_SWITCH(dedup_table_log2, (int)v),
    PFP_SWITCH(no_trigger_table, (int)v),
    PFP_SWITCH(emit_chunk_rows, v > 0 ? (uint64_t)v : (3ULL << 30)),
    PFP_SWITCH(fill_subs, (uint32_t)v),
    PFP_SWITCH(sample_cap, v < 0 ? ~0ULL : (uint64_t)v),
    PFP_SWITCH(no_runaware, (int)v),
    PFP_SWITCH(big_group_members, (long)v),
    PFP_SWITCH(force_wide_rows, (int)v),
    PFP_SWITCH(fasta_chunk_bytes, v > 0 ? (uint64_t)v : 0),
    PFP_SWITCH(ingest_block_bytes, v > 0 ? (uint64_t)v : 0),
    PFP_SWITCH(emit_group_rows, v > 0 ? (uint32_t)v : 0u),
    PFP_SWITCH(no_slot_records, (int)v),
    PFP_SWITCH(dict_text_rounds, (int)v),
    PFP_SWITCH(int_key_symbols, (int)v),
    PFP_SWITCH(force_run_round, (int)v),
    PFP_SWITCH(ingest_readers, (int)v),
    PFP_SWITCH(expand_dma, (int)v),
    PFP_SWITCH(parse_rec, (int)v),
    PFP_SWITCH(parse_rec_p2, (int)v),
    PFP_SWITCH(parse_rec_min, v > 0 ? (uint64_t)v : 0),
    PFP_SWITCH(parse_rec_depth, (int)v),
    PFP_SWITCH(parse_rec_tile_rows, v > 0 ? (uint32_t)v : 0u),
    PFP_SWITCH(parse_rec_merge, v < 0 ? 0 : v > 2 ? 2 : (int)v),
    PFP_SWITCH(parse_rec_merge_members, v < 1 ? 1u : v > 1023 ? 1023u : (uint32_t)v),
    PFP_SWITCH(parse_rec_table_log2, (int)v),
    PFP_SWITCH(dict_rec, (int)v),
    PFP_SWITCH(dict_rec_p2, (int)v),
    PFP_SWITCH(dedup_variant, (int)v),
    PFP_SWITCH(dedup_phases, (int)v),
    PFP_SWITCH(dedup_period, (int64_t)v),
    PFP_SWITCH(dedup_chunk, (int64_t)v),
    PFP_SWITCH(doc_lds_max, v < 2 ? 2u : v > (long long)DOC_LDS_CAP ? DOC_LDS_CAP : (uint32_t)v),
    PFP_SWITCH(dedup_packed, (int)v),
    PFP_SWITCH(group_reduce, (int)v),
    PFP_SWITCH(scan_waves, (int)v),
    PFP_SWITCH(lcp_long_min, v < 16 ? 16u : v > (1LL << 30) ? (1u << 30) : (((uint32_t)v + 15u) & ~15u)),
    PFP_SWITCH(thr_long_min, v < 1 ? 1u : v > (1LL << 30) ? (1u << 30) : (uint32_t)v),
    PFP_SWITCH(thr_tile, pow2_from_16_to_1m(v)),
    PFP_SWITCH(thr_window_rows, v < 1 ? (1ULL << 30) : (uint64_t)v),
    PFP_SWITCH(plcp_block_log2, v < 0 ? -1 : v > PLCP_BLOCK_LOG2_MAX ? PLCP_BLOCK_LOG2_MAX : (int)v),
    PFP_SWITCH(fill_masks, (int)v),
    PFP_SWITCH(fill_skip, (int)v),
    PFP_SWITCH(ms_dir_log2, v < 0 ? -1 : v > MS_DIR_LOG2_MAX ? MS_DIR_LOG2_MAX : (int)v),
    PFP_SWITCH(ms_long_min, v < 1 ? 1u : v > (1LL << 30) ? (1u << 30) : (uint32_t)v),
    PFP_SWITCH(ri_dir_log2, v < 0 ? -1 : v > RI_DIR_LOG2_MAX ? RI_DIR_LOG2_MAX : (int)v),
    PFP_SWITCH(ri_route, v < 0 ? 0 : v > 2 ? 2 : (int)v),
    PFP_SWITCH(dl_chunk_values, v < 1 ? 0 : (uint64_t)v),
    PFP_SWITCH(dl_wave_max, v < 0 ? DL_WAVE_MAX : v > (long long)DL_WAVE_MAX ? DL_WAVE_MAX : (uint32_t)v),
    PFP_SWITCH(dl_table_max, v < 0 ? DL_TABLE_CAP : v > (long long)DL_TABLE_CAP ? DL_TABLE_CAP : (uint32_t)v),
    PFP_SWITCH(mk_chunk_entries, v < 1 ? 0 : (uint64_t)v),
    PFP_SWITCH(mk_wave_max, v < 0 ? MK_WAVE_MAX : v > (long long)MK_WAVE_MAX ? MK_WAVE_MAX : (uint32_t)v),
    PFP_SWITCH(panel_tile, v < 1 ? PANEL_TILE_DEFAULT : v > (long long)PANEL_TILE_MAX ? PANEL_TILE_MAX : (uint32_t)v),
    PFP_SWITCH(panel_out_bytes, v < 1 ? PANEL_OUT_DEFAULT : v < (long long)PANEL_OUT_MIN ? PANEL_OUT_MIN : v > (1LL << 20) ? (1u << 20) : (((uint32_t)v + 15u) & ~15u)),
    PFP_SWITCH(panel_swizzle, v != 0)
};
#undef PFP_SWITCH
static int set_tunable(pfp_ctx *c, const char *key, long long v)
{
    for (const TunableRow &row : tunable_table) if (!strcmp(key, row.name)) { row.store(c->tun, v); return PFP_OK; }
    return PFP_E_ARG;
}
// PFP_VERBOSE is honoured always (it changes no route); every other PFP_<NAME> only in a process started with PFP_TEST_HOOKS=1,
// so that a user's environment cannot silently change routes or tile sizes
static void load_tunables_from_env(pfp_ctx *c)
{
    if (getenv("PFP_VERBOSE")) c->tun.verbose = 1;
    const char *hooks = getenv("PFP_TEST_HOOKS");
    if (!hooks || strcmp(hooks, "1")) return;
    for (const TunableRow &row : tunable_table) {
        char env[64] = "PFP_"; size_t k = 4;
        for (const char *q = row.name; *q && k + 1 < sizeof env; ++q) env[k++] = (char)((*q >= 'a' && *q <= 'z') ? *q - 32 : *q);
        env[k] = 0;
        const char *e = getenv(env);
        if (e) row.store(c->tun, *e ? atoll(e) : 1LL);
    }
}

extern "C" {

const char *pfp_backend(void) { return PFP_BACKEND_NAME; }
int pfp_debug_set(pfp_ctx *c, const char *key, long long value) { return (c && key) ? set_tunable(c, key, value) : PFP_E_ARG; }

const char *pfp_strerror(int s)
{
    switch (s) {
    case PFP_OK: return "ok";
    case PFP_E_ARG: return "invalid argument";
    case PFP_E_INVALID_CHAR: return "error, invalid character";
    case PFP_E_TOO_LARGE: return "input too long for 32-bit device indices";
    case PFP_E_NOMEM: return "device workspace exhausted";
    case PFP_E_HIP: return "HIP runtime error";
    case PFP_E_ONE_WORD: return "error: only one dict word total. Re-run with a smaller p modulus";
    case PFP_E_STATE: return "call order violated";
    case PFP_E_CORRUPT: return "something went wrong!";
    case PFP_E_IO: return "failed to open file!";
    default: return "unknown status";
    }
}

pfp_ctx *pfp_create(int w, uint64_t p, unsigned flags, int device, uint64_t workspace_bytes, int *status)
{
    int st = PFP_OK;
    pfp_ctx *c = nullptr;
    if (w < 1 || w > 32 || p == 0) st = PFP_E_ARG;           // check_w, pfparser.hpp:371-376
    else {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) st = PFP_E_HIP;
        else if (hipSetDevice(device) != hipSuccess) st = PFP_E_HIP;
        else {
            c = new pfp_ctx();
            c->w = w; c->p = p; c->flags = flags; c->device = device; c->arena_request = (size_t)workspace_bytes;
            load_tunables_from_env(c);
            if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; c = nullptr; st = PFP_E_HIP; }
        }
    }
    if (status) *status = st;
    return c;
}

void pfp_destroy(pfp_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    (void)hipDeviceSynchronize();      // other contexts may still read this one's text / shard view on their streams: unmapping does not wait for them
    prof_collect(c);
    for (auto e : c->ev_pool) (void)hipEventDestroy(e);
    c->text.destroy();
    for (int k = 0; k < 2; ++k) { if (c->fa.raw[k]) (void)hipFree(c->fa.raw[k]); if (c->fa.ev_copied[k]) (void)hipEventDestroy(c->fa.ev_copied[k]); if (c->fa.ev_free[k]) (void)hipEventDestroy(c->fa.ev_free[k]); }
    if (c->fa.tiles) (void)hipFree(c->fa.tiles);
    if (c->fa.d_tot) (void)hipFree(c->fa.d_tot);
    if (c->fa.h_tot) (void)hipHostFree(c->fa.h_tot);
    if (c->fa.copy_ready) (void)hipStreamDestroy(c->fa.copy);
    for (auto &q : c->ing_buf) if (q) (void)hipHostFree(q);
    if (c->d_trigtab) (void)hipFree(c->d_trigtab);
    if (c->d_lgtaken) (void)hipFree(c->d_lgtaken);
    for (int k = 0; k < 2; ++k) { if (c->hstage[k]) (void)hipHostFree(c->hstage[k]); if (c->hstage_ev[k]) (void)hipEventDestroy(c->hstage_ev[k]); }
    c->arena.vm.destroy();
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int pfp_error_detail(pfp_ctx *c, uint64_t *pos, int *ch)
{
    if (!c) return PFP_E_ARG;
    if (pos) *pos = c->err_pos;
    if (ch) *ch = c->err_ch;
    return PFP_OK;
}
uint64_t pfp_workspace_needed(pfp_ctx *c) { return c ? (uint64_t)(c->arena.cap + c->arena.want) : 0; }
int pfp_reset(pfp_ctx *c)
{
    if (!c) return PFP_E_ARG;
    PFP_HIP(c, hipSetDevice(c->device));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    reset_results(c);
    return PFP_OK;
}

int pfp_profile_enable(pfp_ctx *c, int on) { if (!c) return PFP_E_ARG; prof_collect(c); c->prof_on = on != 0; c->prof_only = -1; return PFP_OK; }
int pfp_profile_select(pfp_ctx *c, const char *kernel)
{
    if (!c || !kernel) return PFP_E_ARG;
    prof_collect(c);
    for (int i = 0; i < K_COUNT_; ++i) if (!strcmp(kernel, kernel_names[i])) { c->prof_on = true; c->prof_only = i; return PFP_OK; }
    return PFP_E_ARG;
}
int pfp_profile_reset(pfp_ctx *c) { if (!c) return PFP_E_ARG; prof_collect(c); for (auto &r : c->prof) r = ProfRec(); return PFP_OK; }
int pfp_profile_get(pfp_ctx *c, int idx, const char **name, uint64_t *launches, double *ms, double *bytes)
{
    if (!c || idx < 0 || idx >= K_COUNT_) return PFP_E_ARG;
    prof_collect(c);
    if (name) *name = kernel_names[idx];
    if (launches) *launches = c->prof[idx].launches;
    if (ms) *ms = c->prof[idx].ms;
    if (bytes) *bytes = c->prof[idx].bytes;
    return PFP_OK;
}
int pfp_stage_ms(pfp_ctx *c, double out[3]) { if (!c || !out) return PFP_E_ARG; for (int i = 0; i < 3; ++i) out[i] = c->stage_ms[i]; return PFP_OK; }
// page-locked host memory for the callers of pfp_bwt_build_stream / pfp_parse_feed_fasta (they need not link the HIP runtime)
int pfp_host_register(void *p, uint64_t bytes) { if (!p || !bytes) return PFP_E_ARG; if (hipHostRegister(p, (size_t)bytes, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); return PFP_E_HIP; } return PFP_OK; }
int pfp_host_unregister(void *p) { if (!p) return PFP_E_ARG; if (hipHostUnregister(p) != hipSuccess) { (void)hipGetLastError(); return PFP_E_HIP; } return PFP_OK; }

} // extern "C"

#include "feed_host.h"     // stage 1, feeding: records, batches, the row view, raw FASTA bytes and files, the text view
#include "parse_host.h"    // stages 1 and 2: parse, dictionary, shard load and merge, the BWT of the parse, pfp_bwt_load
#include "emit_host.h"     // stage 3: emission pre-pass, slot stage, windows and run samples, the SA-window visitor, pfp_bwt_build*, the ways out
#include "postpass.h"      // the array post-passes: marker array, document arrays, LCP arrays, thresholds
#include "queries.h"       // the queries: matching statistics, count / locate, document listing, MEMs, markers
#include "panel_host.h"    // the variant-panel feed and the VCF file feed on top of it
#include "hooks.h"         // development hooks: checksums, the checkers of a build's outputs, the device-wide primitives on a caller's arrays
#include "gsacak_host.h"   // the gsacak / sacak_int drop-ins
#include "sharded.h"
