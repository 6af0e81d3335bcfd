// pfbwt-f_amd/csrc/pfbwt_hip.hip -- the C ABI of include/pfbwt_hip.h: host orchestration of the
// gfx950 kernels in parse.h / sufsort.h / emit.h / prims.h.  Built by hipcc into
// pfbwt-f_amd/lib/libpfbwt_hip.so.  There is no CPU fallback in this library.
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
#include <sched.h>
#include <thread>
#if defined(__SSE2__)
#include <emmintrin.h>
#endif

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
static const char *const tunable_names[] = {"verbose", "seg_grid", "seg_stage", "sort_k", "sort_no_table", "class_sort_maxrange", "dedup_table_log2", "no_trigger_table",
                                            "emit_chunk_rows", "fill_subs", "sample_cap", "no_runaware", "big_group_members", "force_wide_rows", "fasta_chunk_bytes", "ingest_block_bytes", "emit_group_rows", "no_slot_records", "dict_text_rounds", "int_key_symbols", "force_run_round",
                                            "ingest_readers", "expand_dma", "parse_rec", "parse_rec_p2", "parse_rec_min", "parse_rec_depth", "parse_rec_tile_rows", "parse_rec_merge", "parse_rec_merge_members", "parse_rec_table_log2", "dict_rec", "dict_rec_p2", "dedup_variant", "dedup_phases", "dedup_period", "dedup_chunk", "doc_lds_max", "dedup_packed", "group_reduce", "scan_waves", "lcp_long_min", "thr_long_min", "thr_tile", "thr_window_rows", "plcp_block_log2", "fill_masks", "fill_skip", "ms_dir_log2", "ms_long_min", "ri_dir_log2", "ri_route", "dl_chunk_values", "dl_wave_max", "dl_table_max", "mk_chunk_entries", "mk_wave_max", "panel_tile", "panel_out_bytes", "panel_swizzle"};
static int set_tunable(pfp_ctx *c, const char *key, long long v)
{
    Tunables &t = c->tun;
    if (!strcmp(key, "verbose")) t.verbose = (int)v;
    else if (!strcmp(key, "seg_grid")) t.seg_grid = (int)v;
    else if (!strcmp(key, "seg_stage")) t.seg_stage = (int)v;
    else if (!strcmp(key, "sort_k")) t.sort_k = (int)v;
    else if (!strcmp(key, "sort_no_table")) t.sort_no_table = (int)v;
    else if (!strcmp(key, "class_sort_maxrange")) t.class_sort_maxrange = (uint32_t)v;
    else if (!strcmp(key, "dedup_table_log2")) t.dedup_table_log2 = (int)v;
    else if (!strcmp(key, "no_trigger_table")) t.no_trigger_table = (int)v;
    else if (!strcmp(key, "emit_chunk_rows")) t.emit_chunk_rows = v > 0 ? (uint64_t)v : (3ULL << 30);
    else if (!strcmp(key, "fill_subs")) t.fill_subs = (uint32_t)v;
    else if (!strcmp(key, "fill_masks")) t.fill_masks = (int)v;
    else if (!strcmp(key, "fill_skip")) t.fill_skip = (int)v;
    else if (!strcmp(key, "sample_cap")) t.sample_cap = v < 0 ? ~0ULL : (uint64_t)v;
    else if (!strcmp(key, "no_runaware")) t.no_runaware = (int)v;
    else if (!strcmp(key, "big_group_members")) t.big_group_members = (long)v;
    else if (!strcmp(key, "force_wide_rows")) t.force_wide_rows = (int)v;
    else if (!strcmp(key, "fasta_chunk_bytes")) t.fasta_chunk_bytes = v > 0 ? (uint64_t)v : 0;
    else if (!strcmp(key, "ingest_block_bytes")) t.ingest_block_bytes = v > 0 ? (uint64_t)v : 0;
    else if (!strcmp(key, "emit_group_rows")) t.emit_group_rows = v > 0 ? (uint32_t)v : 0u;
    else if (!strcmp(key, "no_slot_records")) t.no_slot_records = (int)v;
    else if (!strcmp(key, "dict_text_rounds")) t.dict_text_rounds = (int)v;
    else if (!strcmp(key, "int_key_symbols")) t.int_key_symbols = (int)v;
    else if (!strcmp(key, "force_run_round")) t.force_run_round = (int)v;
    else if (!strcmp(key, "ingest_readers")) t.ingest_readers = (int)v;
    else if (!strcmp(key, "expand_dma")) t.expand_dma = (int)v;
    else if (!strcmp(key, "parse_rec")) t.parse_rec = (int)v;
    else if (!strcmp(key, "parse_rec_p2")) t.parse_rec_p2 = (int)v;
    else if (!strcmp(key, "parse_rec_min")) t.parse_rec_min = v > 0 ? (uint64_t)v : 0;
    else if (!strcmp(key, "parse_rec_depth")) t.parse_rec_depth = (int)v;
    else if (!strcmp(key, "parse_rec_tile_rows")) t.parse_rec_tile_rows = v > 0 ? (uint32_t)v : 0u;
    else if (!strcmp(key, "parse_rec_merge")) t.parse_rec_merge = v < 0 ? 0 : v > 2 ? 2 : (int)v;
    else if (!strcmp(key, "parse_rec_merge_members")) t.parse_rec_merge_members = v < 1 ? 1u : v > 1023 ? 1023u : (uint32_t)v;
    else if (!strcmp(key, "parse_rec_table_log2")) t.parse_rec_table_log2 = (int)v;
    else if (!strcmp(key, "dict_rec")) t.dict_rec = (int)v;
    else if (!strcmp(key, "dict_rec_p2")) t.dict_rec_p2 = (int)v;
    else if (!strcmp(key, "dedup_variant")) t.dedup_variant = (int)v;
    else if (!strcmp(key, "dedup_phases")) t.dedup_phases = (int)v;
    else if (!strcmp(key, "dedup_packed")) t.dedup_packed = (int)v;
    else if (!strcmp(key, "group_reduce")) t.group_reduce = (int)v;
    else if (!strcmp(key, "scan_waves")) t.scan_waves = (int)v;
    else if (!strcmp(key, "dedup_period")) t.dedup_period = (int64_t)v;
    else if (!strcmp(key, "dedup_chunk")) t.dedup_chunk = (int64_t)v;
    else if (!strcmp(key, "doc_lds_max")) t.doc_lds_max = v < 2 ? 2u : v > (long long)DOC_LDS_CAP ? DOC_LDS_CAP : (uint32_t)v;
    else if (!strcmp(key, "lcp_long_min")) t.lcp_long_min = v < 16 ? 16u : v > (1LL << 30) ? (1u << 30) : (((uint32_t)v + 15u) & ~15u);
    else if (!strcmp(key, "thr_long_min")) t.thr_long_min = v < 1 ? 1u : v > (1LL << 30) ? (1u << 30) : (uint32_t)v;
    else if (!strcmp(key, "thr_tile")) { uint32_t p2 = 16; while (p2 < (1u << 20) && (long long)p2 < v) p2 *= 2; t.thr_tile = p2; }      // rounded up to a power of two
    else if (!strcmp(key, "thr_window_rows")) t.thr_window_rows = v < 1 ? (1ULL << 30) : (uint64_t)v;
    else if (!strcmp(key, "plcp_block_log2")) t.plcp_block_log2 = v < 0 ? -1 : v > PLCP_BLOCK_LOG2_MAX ? PLCP_BLOCK_LOG2_MAX : (int)v;
    else if (!strcmp(key, "ms_dir_log2")) t.ms_dir_log2 = v < 0 ? -1 : v > MS_DIR_LOG2_MAX ? MS_DIR_LOG2_MAX : (int)v;
    else if (!strcmp(key, "ms_long_min")) t.ms_long_min = v < 1 ? 1u : v > (1LL << 30) ? (1u << 30) : (uint32_t)v;
    else if (!strcmp(key, "ri_dir_log2")) t.ri_dir_log2 = v < 0 ? -1 : v > RI_DIR_LOG2_MAX ? RI_DIR_LOG2_MAX : (int)v;
    else if (!strcmp(key, "ri_route")) t.ri_route = v < 0 ? 0 : v > 2 ? 2 : (int)v;
    else if (!strcmp(key, "dl_chunk_values")) t.dl_chunk_values = v < 1 ? 0 : (uint64_t)v;
    else if (!strcmp(key, "dl_wave_max")) t.dl_wave_max = v < 0 ? DL_WAVE_MAX : v > (long long)DL_WAVE_MAX ? DL_WAVE_MAX : (uint32_t)v;
    else if (!strcmp(key, "dl_table_max")) t.dl_table_max = v < 0 ? DL_TABLE_CAP : v > (long long)DL_TABLE_CAP ? DL_TABLE_CAP : (uint32_t)v;
    else if (!strcmp(key, "mk_chunk_entries")) t.mk_chunk_entries = v < 1 ? 0 : (uint64_t)v;
    else if (!strcmp(key, "mk_wave_max")) t.mk_wave_max = v < 0 ? MK_WAVE_MAX : v > (long long)MK_WAVE_MAX ? MK_WAVE_MAX : (uint32_t)v;
    else if (!strcmp(key, "panel_tile")) t.panel_tile = v < 1 ? PANEL_TILE_DEFAULT : v > (long long)PANEL_TILE_MAX ? PANEL_TILE_MAX : (uint32_t)v;
    else if (!strcmp(key, "panel_out_bytes")) t.panel_out_bytes = v < 1 ? PANEL_OUT_DEFAULT : v < (long long)PANEL_OUT_MIN ? PANEL_OUT_MIN : v > (1LL << 20) ? (1u << 20) : (((uint32_t)v + 15u) & ~15u);
    else if (!strcmp(key, "panel_swizzle")) t.panel_swizzle = v != 0;
    else return PFP_E_ARG;
    return PFP_OK;
}
// PFP_VERBOSE is honoured always (it changes no route); every other PFP_<NAME> only in a process started with PFP_TEST_HOOKS=1,
// so that a user's environment cannot silently change routes or tile sizes
static void load_tunables_from_env(pfp_ctx *c)
{
    if (getenv("PFP_VERBOSE")) c->tun.verbose = 1;
    const char *hooks = getenv("PFP_TEST_HOOKS");
    if (!hooks || strcmp(hooks, "1")) return;
    for (const char *name : tunable_names) {
        char env[64] = "PFP_"; size_t k = 4;
        for (const char *q = name; *q && k + 1 < sizeof env; ++q) env[k++] = (char)((*q >= 'a' && *q <= 'z') ? *q - 32 : *q);
        env[k] = 0;
        const char *e = getenv(env);
        if (e) (void)set_tunable(c, name, *e ? atoll(e) : 1LL);
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

// ---- stage 1: feeding ---------------------------------------------------------------------------
constexpr size_t STAGE_BYTES = (size_t)32 << 20;
static bool host_pointer_is_pinned(const void *p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) == hipSuccess) return a.type == hipMemoryTypeHost;
    (void)hipGetLastError();      // an ordinary malloc'd pointer is reported as an error
    return false;
}
// host memory -> device: pinned sources directly, pageable ones through the staging ring (kseq's 16 KiB reads of
// include/kseq.h:228 become 32 MiB DMA transfers; the memcpy into one buffer overlaps the transfer of the other)
// *in_flight (nullable) = the caller's buffer may still be read when this returns (pinned source: the caller must wait for
// the stream); copies through the staging ring are complete as far as the caller's buffer is concerned.
static int h2d_copy(pfp_ctx *c, uint8_t *dst, const uint8_t *src, uint64_t len, bool *in_flight = nullptr)
{
    if (in_flight) *in_flight = false;
    if (!len) return PFP_OK;
    if (host_pointer_is_pinned(src)) { PFP_HIP(c, hipMemcpyAsync(dst, src, (size_t)len, hipMemcpyHostToDevice, c->stream)); if (in_flight) *in_flight = true; else PFP_HIP(c, hipStreamSynchronize(c->stream)); return PFP_OK; }
    if (len <= ((size_t)1 << 16)) { PFP_HIP(c, hipMemcpyAsync(dst, src, (size_t)len, hipMemcpyHostToDevice, c->stream)); PFP_HIP(c, hipStreamSynchronize(c->stream)); return PFP_OK; }
    for (int k = 0; k < 2; ++k) if (!c->hstage[k]) {
        PFP_HIP(c, hipHostMalloc((void **)&c->hstage[k], STAGE_BYTES, hipHostMallocDefault));
        PFP_HIP(c, hipEventCreate(&c->hstage_ev[k]));
    }
    int k = 0;
    for (uint64_t off = 0; off < len; off += STAGE_BYTES, k ^= 1) {
        const size_t chunk = (size_t)(len - off < STAGE_BYTES ? len - off : STAGE_BYTES);
        if (c->hstage_used[k]) PFP_HIP(c, hipEventSynchronize(c->hstage_ev[k]));      // the transfer that last used this buffer is done
        memcpy(c->hstage[k], src + off, chunk);
        PFP_HIP(c, hipMemcpyAsync(dst + off, c->hstage[k], chunk, hipMemcpyHostToDevice, c->stream));
        PFP_HIP(c, hipEventRecord(c->hstage_ev[k], c->stream));
        c->hstage_used[k] = true;
    }
    return PFP_OK;
}
static int feed_common(pfp_ctx *c, const void *src, uint64_t len, int end_of_seq, hipMemcpyKind kind)
{
    if (!c || (!src && len)) return PFP_E_ARG;
    PFP_HIP(c, hipSetDevice(c->device));
    if (c->stage != 0) reset_results(c);
    const uint64_t add = len + (end_of_seq ? (uint64_t)c->w : 0);
    // pfparser.hpp:326-331: the 32-bit build stops at 2^32 bases; the 64-bit build here at 2^40 (device positions are 64-bit)
    if (c->n + add + (uint64_t)c->w + 64 >= ((c->flags & PFP_FLAG_U64) ? (1ULL << 40) : 0xFFFFFFFFULL)) return PFP_E_TOO_LARGE;
    PFP_TRY(ensure_text(c, c->n + add + (uint64_t)c->w));
    bool in_flight = false;
    if (len && kind == hipMemcpyHostToDevice) PFP_TRY(h2d_copy(c, c->tb + 16 + c->n, (const uint8_t *)src, len, &in_flight));
    else if (len) PFP_HIP(c, hipMemcpyAsync(c->tb + 16 + c->n, src, (size_t)len, kind, c->stream));
    c->n += len;
    if (end_of_seq) {   // the w 'A's of pfparser.hpp:335-337
        ++c->nseq;
        PFP_HIP(c, hipMemsetAsync(c->tb + 16 + c->n, 'A', (size_t)c->w, c->stream));
        c->n += (uint64_t)c->w;
    }
    // the caller may reuse its buffer on return: a pageable source went through the staging ring (its DMA transfers overlap
    // the caller's next read / decompression, include/kseq.h:228), only a page-locked source is read in place
    // (a device source may belong to another context that its owner destroys right after this call -- PfParser::operator+= with a
    // temporary right-hand side, src/merge_pfp.cpp:100-112: unmapping on-demand committed memory does not wait for copies in flight)
    if (in_flight || (len && kind == hipMemcpyDeviceToDevice)) PFP_HIP(c, hipStreamSynchronize(c->stream));
    c->tb_n = c->n;
    return PFP_OK;
}
int pfp_parse_reopen(pfp_ctx *c)
{
    if (!c) return PFP_E_ARG;
    PFP_HIP(c, hipSetDevice(c->device));
    if (c->stage == 0) return PFP_OK;
    if (!c->tb || !c->tb_n || c->tb_n != c->n) return PFP_E_STATE;   // a context filled by pfp_merge_shards / pfp_bwt_load holds no text
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    const uint64_t n = c->n, nseq = c->nseq;
    reset_results(c);
    c->nseq = nseq;
    c->n = c->tb_n = n;                                         // the (normalised) text is still in place; more can be appended
    return PFP_OK;
}
static int flush_view(pfp_ctx *c);
int pfp_text_view(pfp_ctx *c, const uint8_t **d_text, uint64_t *n)
{
    if (!c || !d_text || !n) return PFP_E_ARG;
    PFP_TRY(flush_view(c));
    if (!c->tb || c->tb_n != c->n) { *d_text = nullptr; *n = 0; return PFP_OK; }
    PFP_HIP(c, hipSetDevice(c->device));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    *d_text = c->tb + 16; *n = c->n;
    return PFP_OK;
}
int pfp_text_get(pfp_ctx *c, uint64_t off, uint64_t len, uint8_t *host)
{
    const uint8_t *d = nullptr; uint64_t n = 0;
    if (!c || (!host && len)) return PFP_E_ARG;
    PFP_TRY(pfp_text_view(c, &d, &n));
    if (off > n || len > n - off) return PFP_E_ARG;
    if (len) { PFP_HIP(c, hipMemcpyAsync(host, d + off, (size_t)len, hipMemcpyDeviceToHost, c->stream)); PFP_HIP(c, hipStreamSynchronize(c->stream)); }
    return PFP_OK;
}
int pfp_parse_feed_left_context(pfp_ctx *c)
{
    if (!c) return PFP_E_ARG;
    if (c->stage != 0) { PFP_HIP(c, hipSetDevice(c->device)); reset_results(c); }
    if (c->n != 0) return PFP_E_STATE;                            // the context must be the first thing a shard is fed
    const std::vector<uint8_t> a((size_t)c->w, (uint8_t)'A');
    PFP_TRY(feed_common(c, a.data(), a.size(), 0, hipMemcpyHostToDevice));
    c->left_ctx = (uint64_t)c->w;
    return PFP_OK;
}
// a pending row view (pfp_parse_feed_device_view) becomes text in X: what every entry point that appends to or hands out the text
// does first (the fused scan of pfp_parse_finalize is the one consumer that does not need it)
static int flush_view(pfp_ctx *c)
{
    if (!c->view.src) return PFP_OK;
    const uint64_t count = c->view.count, len = c->view.len;
    const uint64_t blocks_per_row = ((len + 15) / 16 + BLOCK - 1) / BLOCK;
    PFP_LAUNCH(c, K_MISC, 2 * count * len, k_feed_batch, count * blocks_per_row, c->view.src, count, len, c->view.stride, c->w, c->tb + 16);
    c->view.src = nullptr;
    return PFP_OK;
}
int pfp_parse_feed_device_view(pfp_ctx *c, const void *d_bases, uint64_t count, uint64_t len, uint64_t stride)
{
    if (!c || !d_bases || !count || !len || stride < len) return PFP_E_ARG;
    PFP_HIP(c, hipSetDevice(c->device));
    if (c->stage != 0) reset_results(c);
    if (c->n != 0) return PFP_E_STATE;                                   // the view is the whole text of a parse
    const uint64_t pitch = len + (uint64_t)c->w, add = count * pitch;
    if (add + (uint64_t)c->w + 64 >= ((c->flags & PFP_FLAG_U64) ? (1ULL << 40) : 0xFFFFFFFFULL)) return PFP_E_TOO_LARGE;
    const uint64_t blocks_per_row = ((len + 15) / 16 + BLOCK - 1) / BLOCK;
    if (count * blocks_per_row >= 0x7FFFFFFFULL) return PFP_E_TOO_LARGE;
    PFP_TRY(ensure_text(c, add + (uint64_t)c->w));
    c->view.src = (const uint8_t *)d_bases; c->view.count = count; c->view.len = len; c->view.stride = stride;
    c->n = add; c->tb_n = c->n; c->nseq = count;
    return PFP_OK;
}
int pfp_parse_feed(pfp_ctx *c, const uint8_t *bases, uint64_t len, int end_of_seq) { if (c) PFP_TRY(flush_view(c)); return feed_common(c, bases, len, end_of_seq, hipMemcpyHostToDevice); }
int pfp_parse_feed_device(pfp_ctx *c, const void *d_bases, uint64_t len, int end_of_seq) { if (c) PFP_TRY(flush_view(c)); return feed_common(c, d_bases, len, end_of_seq, hipMemcpyDeviceToDevice); }
int pfp_parse_feed_device_batch(pfp_ctx *c, const void *d_bases, uint64_t count, uint64_t len, uint64_t stride)
{
    if (!c || (!d_bases && count && len) || stride < len) return PFP_E_ARG;
    if (!count) return PFP_OK;
    PFP_TRY(flush_view(c));
    if (!len) { for (uint64_t k = 0; k < count; ++k) PFP_TRY(feed_common(c, nullptr, 0, 1, hipMemcpyDeviceToDevice)); return PFP_OK; }
    PFP_HIP(c, hipSetDevice(c->device));
    if (c->stage != 0) reset_results(c);
    const uint64_t pitch = len + (uint64_t)c->w, add = count * pitch;
    if (c->n + add + (uint64_t)c->w + 64 >= ((c->flags & PFP_FLAG_U64) ? (1ULL << 40) : 0xFFFFFFFFULL)) return PFP_E_TOO_LARGE;
    PFP_TRY(ensure_text(c, c->n + add + (uint64_t)c->w));
    uint8_t *dst = c->tb + 16 + c->n;
    const uint64_t blocks_per_row = ((len + 15) / 16 + BLOCK - 1) / BLOCK;
    if (count * blocks_per_row >= 0x7FFFFFFFULL) return PFP_E_TOO_LARGE;      // grid limit (2^31 workgroups = 8 Tbase)
    PFP_LAUNCH(c, K_MISC, 2 * count * len, k_feed_batch, count * blocks_per_row, (const uint8_t *)d_bases, count, len, stride, c->w, dst);
    c->n += add; c->tb_n = c->n; c->nseq += count;
    return PFP_OK;
}

int pfp_parse_feed_batch(pfp_ctx *c, const uint8_t *bases, uint64_t count, uint64_t len, uint64_t stride)
{
    if (!c || (!bases && count && len) || stride < len) return PFP_E_ARG;
    if (!count) return PFP_OK;
    PFP_TRY(flush_view(c));
    if (!len || !host_pointer_is_pinned(bases)) {      // pageable memory: record by record through the staging ring
        for (uint64_t k = 0; k < count; ++k) PFP_TRY(feed_common(c, bases + k * stride, len, 1, hipMemcpyHostToDevice));
        return PFP_OK;
    }
    PFP_HIP(c, hipSetDevice(c->device));
    if (c->stage != 0) reset_results(c);
    const uint64_t pitch = len + (uint64_t)c->w, add = count * pitch;
    if (c->n + add + (uint64_t)c->w + 64 >= ((c->flags & PFP_FLAG_U64) ? (1ULL << 40) : 0xFFFFFFFFULL)) return PFP_E_TOO_LARGE;
    PFP_TRY(ensure_text(c, c->n + add + (uint64_t)c->w));
    uint8_t *dst = c->tb + 16 + c->n;
    // pinned host memory: one DMA transfer per record, queued back to back (the runtime's 2-D copy rejects a destination that
    // spans several pieces of the on-demand committed text, csrc/devmem.h), the pads of pfparser.hpp:335-337 by one small kernel
    for (uint64_t k = 0; k < count; ++k) PFP_HIP(c, hipMemcpyAsync(dst + k * pitch, bases + k * stride, (size_t)len, hipMemcpyHostToDevice, c->stream));
    PFP_LAUNCH(c, K_MISC, count * (uint64_t)c->w, k_pad_rows, nblocks(count * (uint64_t)c->w, BLOCK), dst, count, len, pitch, c->w);
    PFP_HIP(c, hipStreamSynchronize(c->stream));      // the caller may reuse its buffer
    c->n += add; c->tb_n = c->n; c->nseq += count;
    return PFP_OK;
}

// ---- raw FASTA bytes (csrc/fasta.h) ---------------------------------------------------------------------------------
constexpr size_t FA_RAW_MAX = (size_t)256 << 20, FA_RAW_MIN = (size_t)1 << 20;
int pfp_parse_reserve(pfp_ctx *c, uint64_t text_bytes)
{
    if (!c) return PFP_E_ARG;
    if (!c->text.live()) c->text_hint = text_bytes;      // sizes the address range of the text; ignored once text has been fed
    return PFP_OK;
}
static int ensure_copy_stream(pfp_ctx *c)
{
    auto &f = c->fa;
    if (f.copy_ready) return PFP_OK;
    PFP_HIP(c, hipStreamCreateWithFlags(&f.copy, hipStreamNonBlocking));
    f.copy_ready = true;
    for (int k = 0; k < 2; ++k) { PFP_HIP(c, hipEventCreateWithFlags(&f.ev_copied[k], hipEventDisableTiming)); PFP_HIP(c, hipEventCreateWithFlags(&f.ev_free[k], hipEventDisableTiming)); }
    PFP_HIP(c, hipMalloc((void **)&f.d_tot, 64));
    PFP_HIP(c, hipHostMalloc((void **)&f.h_tot, 64, hipHostMallocDefault));
    PFP_HIP(c, hipMemsetAsync(f.d_tot, 0, 64, c->stream));
    return PFP_OK;
}
static int fasta_buffers(pfp_ctx *c, uint64_t len)
{
    auto &f = c->fa;
    size_t want = FA_RAW_MIN; while (want < FA_RAW_MAX && want < len) want <<= 1;
    if (c->tun.fasta_chunk_bytes) want = (size_t)(c->tun.fasta_chunk_bytes < 64 ? 64 : c->tun.fasta_chunk_bytes);      // tests: many chunks on small inputs
    PFP_TRY(ensure_copy_stream(c));
    if (f.rawcap >= want || (f.rawcap && want < 4 * f.rawcap)) return PFP_OK;      // (a much larger call than the first one: take larger buffers once)
    PFP_HIP(c, hipStreamSynchronize(c->stream)); PFP_HIP(c, hipStreamSynchronize(f.copy));
    for (int k = 0; k < 2; ++k) { if (f.raw[k]) PFP_HIP(c, hipFree(f.raw[k])); f.raw[k] = nullptr; f.used[k] = false; }
    if (f.tiles) { PFP_HIP(c, hipFree(f.tiles)); f.tiles = nullptr; }
    for (int k = 0; k < 2; ++k) if (hipMalloc((void **)&f.raw[k], want) != hipSuccess) { (void)hipGetLastError(); f.rawcap = 0; return PFP_E_NOMEM; }
    const size_t T = want / FA_TILE + 1;
    f.tiles_cap = T * (1 + 12 + 12 + 1 + 8 + 4) + 256;
    if (hipMalloc((void **)&f.tiles, f.tiles_cap) != hipSuccess) { (void)hipGetLastError(); f.rawcap = 0; return PFP_E_NOMEM; }
    f.rawcap = want;
    return PFP_OK;
}
// kseq_read, include/kseq.h:186-190: everything in front of the first '>' or '@' of a stream is skipped.  Returns the offset
// of the first byte that counts (len: none yet).
static uint64_t fa_skip_preamble(pfp_ctx *c, const uint8_t *raw, uint64_t len)
{
    auto &f = c->fa;
    if (f.started || !len) return 0;
    const uint8_t *a = (const uint8_t *)memchr(raw, '>', (size_t)len), *b = (const uint8_t *)memchr(raw, '@', (size_t)len);
    const uint8_t *q = (a && b) ? (a < b ? a : b) : (a ? a : b);
    if (!q) return len;
    f.started = true; f.state = FA_L; f.records = 0;
    return (uint64_t)(q - raw);
}
// upload of one raw piece (at most rawcap bytes) into device buffer `slot`, once the kernels that read its previous content are done
static int fa_issue(pfp_ctx *c, const uint8_t *src, uint64_t len, int slot)
{
    auto &f = c->fa;
    if (f.used[slot]) PFP_HIP(c, hipStreamWaitEvent(f.copy, f.ev_free[slot], 0));
    PFP_HIP(c, hipMemcpyAsync(f.raw[slot], src, (size_t)len, hipMemcpyHostToDevice, f.copy));
    PFP_HIP(c, hipEventRecord(f.ev_copied[slot], f.copy));
    return PFP_OK;
}
// strip the piece in device buffer `slot` into the text.  Returns with the upload of the piece complete (the host waits for
// the piece's totals, which wait for the upload): the caller's buffer may be reused.  rec_base: offset of the piece in the
// caller's coordinate system (record offsets are reported in it).
static int fa_process(pfp_ctx *c, uint64_t len, int slot, bool want_recs, uint64_t rec_base, uint64_t *started)
{
    auto &f = c->fa;
    const uint64_t w = (uint64_t)c->w;
    const uint64_t limit = (c->flags & PFP_FLAG_U64) ? (1ULL << 40) : 0xFFFFFFFFULL;
    PFP_HIP(c, hipStreamWaitEvent(c->stream, f.ev_copied[slot], 0));
    FaTiles t; t.T = (len + FA_TILE - 1) / FA_TILE;
    uint8_t *q = f.tiles;
    t.kbase = (unsigned long long *)q; q += t.T * 8; t.kept = (uint32_t *)q; q += t.T * 12; t.hdr = (uint32_t *)q; q += t.T * 12; t.hbase = (uint32_t *)q; q += t.T * 4; t.func = q; q += t.T; t.st = q;
    PFP_LAUNCH(c, K_FASTA, len, k_fa_scan, t.T, (const uint8_t *)f.raw[slot], len, t);
    PFP_LAUNCH(c, K_MISC, t.T * 40, k_fa_spine, 1, t, f.state, f.d_tot);
    PFP_HIP(c, hipMemcpyAsync(f.h_tot, f.d_tot, 24, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    const uint64_t kept = f.h_tot[0], hdr = f.h_tot[1], rec0 = f.records;
    const uint64_t tbase = c->n - w * (rec0 ? rec0 - 1 : 0);
    const uint64_t n_new = tbase + kept + w * ((rec0 + hdr) ? rec0 + hdr - 1 : 0);
    if (n_new + 2 * w + 64 >= limit) return PFP_E_TOO_LARGE;                      // pfparser.hpp:326-331
    PFP_TRY(ensure_text(c, n_new + 2 * w));
    uint64_t *d_rr = nullptr, *d_rp = nullptr;
    struct DevFree { uint64_t *&p; ~DevFree() { if (p) (void)hipFree(p); } } rr_guard{d_rr};      // freed on every path out of this function
    if (want_recs && hdr) { PFP_HIP(c, hipMalloc((void **)&d_rr, hdr * 16)); d_rp = d_rr + hdr; }
    PFP_LAUNCH(c, K_FASTA, 2 * len, k_fa_compact, t.T, (const uint8_t *)f.raw[slot], len, t, c->tb + 16, tbase, rec0, c->w, d_rr, d_rp, (uint32_t *)(f.d_tot + 4));
    PFP_HIP(c, hipEventRecord(f.ev_free[slot], c->stream)); f.used[slot] = true;
    if (d_rr) {
        const size_t b = f.rec_raw.size();
        f.rec_raw.resize(b + hdr); f.rec_pos.resize(b + hdr);
        PFP_HIP(c, hipMemcpyAsync(f.rec_raw.data() + b, d_rr, hdr * 8, hipMemcpyDeviceToHost, c->stream));      // (the context's stream does not synchronise with the null stream)
        PFP_HIP(c, hipMemcpyAsync(f.rec_pos.data() + b, d_rp, hdr * 8, hipMemcpyDeviceToHost, c->stream));
        PFP_HIP(c, hipStreamSynchronize(c->stream));
        for (size_t i = b; i < b + hdr; ++i) f.rec_raw[i] += rec_base;
    }
    c->n = n_new; c->tb_n = c->n; f.records = rec0 + hdr; f.state = (uint32_t)f.h_tot[2];
    if (started) *started += hdr;
    return PFP_OK;
}
// end of a stream: the pad of its last record; a '+' line seen on the way makes the whole stream PFP_E_ARG
static int fa_finish_stream(pfp_ctx *c)
{
    auto &f = c->fa;
    const uint64_t w = (uint64_t)c->w;
    if (f.started && f.records) {
        PFP_TRY(ensure_text(c, c->n + 2 * w));
        PFP_HIP(c, hipMemsetAsync(c->tb + 16 + c->n, 'A', (size_t)w, c->stream));
        c->n += w; c->tb_n = c->n;
    }
    uint32_t fl = 0;
    if (f.d_tot) { PFP_HIP(c, hipMemcpyAsync(&fl, f.d_tot + 4, 4, hipMemcpyDeviceToHost, c->stream)); PFP_HIP(c, hipStreamSynchronize(c->stream)); PFP_HIP(c, hipMemsetAsync(f.d_tot + 4, 0, 8, c->stream)); }
    c->nseq += f.records;      // (the hint the text de-duplication orders its workgroups by)
    f.started = false; f.state = FA_L; f.records = 0;
    if (fl & 1u) { c->err_ch = '+'; return PFP_E_ARG; }                             // a FASTQ quality section: not handled on the device
    return PFP_OK;
}
static int feed_fasta_pieces(pfp_ctx *c, const uint8_t *raw, uint64_t len, unsigned flags, uint64_t *nrec);
// The header promises that the caller's buffer may be reused (freed, unregistered) when the call returns.  On the good path every
// piece's upload has completed by then (fa_process waits for the piece's totals, which wait for its upload); on an error return the
// upload of piece k + 1 may still be reading the buffer -- PFP_E_TOO_LARGE / PFP_E_NOMEM of piece k come after it was issued --
// so every error path drains both streams first.
static int feed_fasta_impl(pfp_ctx *c, const uint8_t *raw, uint64_t len, unsigned flags, uint64_t *nrec)
{
    PFP_TRY(flush_view(c));
    const int rc = feed_fasta_pieces(c, raw, len, flags, nrec);
    if (rc != PFP_OK) { if (c->fa.copy_ready) (void)hipStreamSynchronize(c->fa.copy); (void)hipStreamSynchronize(c->stream); }
    return rc;
}
static int feed_fasta_pieces(pfp_ctx *c, const uint8_t *raw, uint64_t len, unsigned flags, uint64_t *nrec)
{
    auto &f = c->fa;
    const bool want_recs = (flags & PFP_FASTA_RECORDS) != 0;
    f.rec_raw.clear(); f.rec_pos.clear();
    uint64_t started = 0;
    const uint64_t off = fa_skip_preamble(c, raw, len);
    if (off < len) {
        PFP_TRY(fasta_buffers(c, len - off));
        const uint64_t cap = f.rawcap, nsub = (len - off + cap - 1) / cap;
        auto piece = [&](uint64_t k, uint64_t *o, uint64_t *cl) { *o = off + k * cap; *cl = (len - *o < cap) ? len - *o : cap; };
        uint64_t o, cl;
        piece(0, &o, &cl); PFP_TRY(fa_issue(c, raw + o, cl, 0));
        for (uint64_t k = 0; k < nsub; ++k) {
            if (k + 1 < nsub) { piece(k + 1, &o, &cl); PFP_TRY(fa_issue(c, raw + o, cl, (int)((k + 1) & 1))); }      // its upload overlaps the stripping of piece k
            piece(k, &o, &cl);
            PFP_TRY(fa_process(c, cl, (int)(k & 1), want_recs, o, &started));
        }
    }
    if (flags & PFP_FASTA_FINAL) PFP_TRY(fa_finish_stream(c));
    if (nrec) *nrec = started;
    return PFP_OK;
}
int pfp_parse_feed_fasta(pfp_ctx *c, const uint8_t *raw, uint64_t len, unsigned flags, uint64_t *nrec)
{
    if (!c || (!raw && len)) return PFP_E_ARG;
    PFP_HIP(c, hipSetDevice(c->device));
    if (c->stage != 0) reset_results(c);
    return feed_fasta_impl(c, raw, len, flags, nrec);
}
} // extern "C"
#include "ingest.h"
extern "C" {
int pfp_parse_feed_fasta_file(pfp_ctx *c, const char *path, unsigned flags, pfp_ingest_info *info)
{
    if (!c || !path) return PFP_E_ARG;
    PFP_HIP(c, hipSetDevice(c->device));
    if (c->stage != 0) reset_results(c);
    IngestStats st;
    const int rc = ingest_file(c, path, flags, &st);
    if (info) { info->raw_bytes = st.raw_bytes; info->records = st.records; info->n = c->n; info->read_wait_ms = st.read_wait_ms; info->total_ms = st.total_ms; info->mode = st.mode; }
    return rc;
}
int pfp_bwt_write(pfp_ctx *c, int fd_bwt, int fd_sa, int fd_ssa, int fd_esa)
{
    if (!c) return PFP_E_ARG;
    if (c->stage < 3) return PFP_E_STATE;
    PFP_HIP(c, hipSetDevice(c->device));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    const size_t U = (c->flags & PFP_FLAG_U64) ? 8 : 4;
    if (fd_bwt >= 0) PFP_TRY(write_device_to_fd(c, c->d_bwt, c->slice_rows, fd_bwt));
    if (fd_sa >= 0) { if (!c->d_sa) return PFP_E_STATE; PFP_TRY(write_device_to_fd(c, c->d_sa, c->slice_rows * U, fd_sa)); }
    if (fd_ssa >= 0) { if (!c->d_ssa) return PFP_E_STATE; PFP_TRY(write_device_to_fd(c, c->d_ssa, c->runs * 2 * U, fd_ssa)); }
    if (fd_esa >= 0) { if (!c->d_esa) return PFP_E_STATE; PFP_TRY(write_device_to_fd(c, c->d_esa, c->esa_pairs * 2 * U, fd_esa)); }
    return PFP_OK;
}
// .bwt over the slow link in its run-length form: with the run samples at hand, .ssa[k].row starts run k, so ONE byte per run (r bytes:
// 84 MB on S-32G) crosses PCIe instead of n + 1 (32 GB), and host threads write the runs out (memset) at memory bandwidth.
extern "C++" {
template <typename SAT> __global__ __launch_bounds__(BLOCK) void k_run_heads(const uint8_t *bwt, const SAT *ssa, uint64_t r, uint8_t *heads)
{
    const uint64_t k = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k < r) heads[k] = bwt[(uint64_t)ssa[2 * k]];
}
}
// The runs of one block of the .bwt into host memory.  A run is a few hundred bytes on a pangenome.  Written run by run, every run
// touches two partial cache lines -- with ordinary stores every line of the 32 GB output is first READ from memory to be owned, with
// streaming stores a partially written line costs the memory controller a read-modify-write (measured on the pool's boxes: 130 ns per
// run and thread, 1.5 GB/s per thread).  So the runs are expanded into a 4 KiB buffer that lives in L1 and leave it as whole, 64-byte
// aligned lines of streaming stores; a run longer than the buffer goes out directly.
struct RunWriter {
    uint8_t *dst;                 // next byte of the destination that has not been written
    alignas(64) uint8_t buf[4096]; size_t fill = 0;
    explicit RunWriter(uint8_t *d) : dst(d) {}
    static void stream(uint8_t *d, const uint8_t *s, size_t len)      // d 16-byte aligned, len a multiple of 16
    {
#if defined(__SSE2__)
        for (size_t i = 0; i < len; i += 16) _mm_stream_si128(reinterpret_cast<__m128i *>(d + i), _mm_load_si128(reinterpret_cast<const __m128i *>(s + i)));
#else
        memcpy(d, s, len);
#endif
    }
    void flush_all()              // everything buffered goes out (the tail that is not a whole line with ordinary stores)
    {
        const size_t body = fill & ~(size_t)63;
        if (((uintptr_t)dst & 63u) == 0) { stream(dst, buf, body); memcpy(dst + body, buf + body, fill - body); }
        else memcpy(dst, buf, fill);
        dst += fill; fill = 0;
    }
    void put(uint8_t v, size_t len)
    {
        if (fill == 0 && ((uintptr_t)dst & 63u)) {      // bring the destination to a line boundary first
            const size_t head = (size_t)(-(uintptr_t)dst & 63u) < len ? (size_t)(-(uintptr_t)dst & 63u) : len;
            memset(dst, v, head); dst += head; len -= head;
        }
        while (len) {
            if (fill == 0 && len >= sizeof buf) {      // a long run: whole lines straight to the destination
                const size_t body = len & ~(size_t)63;
#if defined(__SSE2__)
                const __m128i x = _mm_set1_epi8((char)v);
                for (size_t i = 0; i < body; i += 16) _mm_stream_si128(reinterpret_cast<__m128i *>(dst + i), x);
#else
                memset(dst, v, body);
#endif
                dst += body; len -= body;
                continue;
            }
            const size_t k = len < sizeof buf - fill ? len : sizeof buf - fill;
            memset(buf + fill, v, k); fill += k; len -= k;
            if (fill == sizeof buf) { stream(dst, buf, sizeof buf); dst += sizeof buf; fill = 0; }
        }
    }
};
int pfp_bwt_get_expanded(pfp_ctx *c, uint8_t *host_bwt, const void *ssa_host, int threads)
{
    if (!c || !host_bwt) return PFP_E_ARG;
    if (c->stage < 3 || !c->d_ssa || !c->d_bwt || c->slice_rows != c->nout || c->slice_begin != 0) return PFP_E_STATE;      // needs the whole output's run samples
    PFP_HIP(c, hipSetDevice(c->device));
    const bool u64 = (c->flags & PFP_FLAG_U64) != 0;
    const uint64_t r = c->runs, nout = c->nout;
    const size_t mk = c->arena.mark_hi();
    uint8_t *d_heads; PFP_ALLOC_HI(c, d_heads, uint8_t, r);
    if (u64) PFP_LAUNCH(c, K_MISC, r * 9, (k_run_heads<uint64_t>), nblocks(r, BLOCK), (const uint8_t *)c->d_bwt, (const uint64_t *)c->d_ssa, r, d_heads);
    else PFP_LAUNCH(c, K_MISC, r * 5, (k_run_heads<uint32_t>), nblocks(r, BLOCK), (const uint8_t *)c->d_bwt, (const uint32_t *)c->d_ssa, r, d_heads);
    std::vector<uint8_t> heads((size_t)r);
    PFP_HIP(c, hipMemcpyAsync(heads.data(), d_heads, (size_t)r, hipMemcpyDeviceToHost, c->stream));
    std::vector<uint8_t> own;
    if (!ssa_host) { own.resize((size_t)r * 2 * (u64 ? 8 : 4)); PFP_HIP(c, hipMemcpyAsync(own.data(), c->d_ssa, own.size(), hipMemcpyDeviceToHost, c->stream)); ssa_host = own.data(); }
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    c->arena.release_hi(mk);
    if (threads < 1) threads = usable_cpus();      // 0 / negative: one thread per CPU this process may use
    if (threads > 64) threads = 64;
    auto row = [&](uint64_t k) -> uint64_t { return k >= r ? nout : (u64 ? ((const uint64_t *)ssa_host)[2 * k] : (uint64_t)((const uint32_t *)ssa_host)[2 * k]); };
    // The output is cut into blocks of BYTES (runs of a collection's BWT are anything from 1 to millions of rows long; equal run counts
    // gave threads unequal shares -- VERDICT r3).  Host threads claim blocks from the FRONT and write the runs that reach into them
    // (the first one is found by bisection over the run starts).  When the destination is page-locked, the copy engine claims
    // blocks from the BACK and moves those rows over PCIe as they are: host stores and DMA writes use different paths into host memory
    // (16 cores of two CCDs reach ~65 GB/s of streaming stores on the pool's boxes, the link 55 GB/s), so the two meet somewhere in the
    // middle -- wherever this box's ratio puts it -- instead of the slower one doing everything (S-32G: 472 -> ~270 ms).
    const uint64_t BLKB = c->tun.expand_dma >= 2 ? ((uint64_t)1 << 20) : ((uint64_t)64 << 20);      // (2: tests -- 1 MiB blocks, so that small outputs are split between threads and link too)
    const uint64_t nblk = (nout + BLKB - 1) / BLKB;
    std::mutex mu; uint64_t front = 0, back = nblk;      // blocks [front, back) are unclaimed
    auto claim = [&](bool from_back, uint64_t *blk) -> bool { std::lock_guard<std::mutex> g(mu); if (front >= back) return false; *blk = from_back ? --back : front++; return true; };
    std::vector<std::thread> th;
    for (int t = 0; t < threads; ++t)
        th.emplace_back([&] {
            uint64_t blk;
            while (claim(false, &blk)) {
                const uint64_t b0 = blk * BLKB, b1 = b0 + BLKB < nout ? b0 + BLKB : nout;
                uint64_t lo = 0, hi = r;                    // last run that starts at or before b0 (run 0 starts at row 0)
                while (hi - lo > 1) { const uint64_t mid = lo + (hi - lo) / 2; if (row(mid) <= b0) lo = mid; else hi = mid; }
                uint64_t a = b0;
                RunWriter wr(host_bwt + b0);
                for (uint64_t k = lo; k < r && a < b1; ++k) { uint64_t e = row(k + 1); if (e > b1) e = b1; if (e > a) { wr.put(heads[(size_t)k], (size_t)(e - a)); a = e; } }
                wr.flush_all();
            }
#if defined(__SSE2__)
            _mm_sfence();      // the streaming stores of this thread are globally visible before it ends
#endif
        });
    int dma_rc = PFP_OK; uint64_t dma_blocks = 0;
    if (nblk >= (c->tun.expand_dma >= 2 ? 2u : 8u) && c->tun.expand_dma != 0 && host_pointer_is_pinned(host_bwt) && ensure_copy_stream(c) == PFP_OK) {
        uint64_t blk;
        while (dma_rc == PFP_OK && claim(true, &blk)) {
            const uint64_t b0 = blk * BLKB, b1 = b0 + BLKB < nout ? b0 + BLKB : nout;
            if (hipMemcpyAsync(host_bwt + b0, (const uint8_t *)c->d_bwt + b0, (size_t)(b1 - b0), hipMemcpyDeviceToHost, c->fa.copy) != hipSuccess || hipStreamSynchronize(c->fa.copy) != hipSuccess) { (void)hipGetLastError(); dma_rc = PFP_E_HIP; }
            ++dma_blocks;
        }
    }
    for (auto &t : th) t.join();
    if (c->tun.verbose) fprintf(stderr, "[pfbwt_hip] .bwt from its runs: %llu blocks of 64 MiB, %llu of them over the link\n", (unsigned long long)nblk, (unsigned long long)dma_blocks);
    return dma_rc;
}
int pfp_parse_docs(pfp_ctx *c, uint64_t *count) { if (!c || !count) return PFP_E_ARG; *count = c->doc_names.size(); return PFP_OK; }
int pfp_parse_doc_get(pfp_ctx *c, uint64_t i, const char **name, uint64_t *start)
{
    if (!c || i >= c->doc_names.size()) return PFP_E_ARG;
    if (name) *name = c->doc_names[(size_t)i].c_str();
    if (start) *start = c->doc_starts[(size_t)i];
    return PFP_OK;
}
int pfp_parse_fasta_records(pfp_ctx *c, uint64_t *raw_off, uint64_t *text_pos)
{
    if (!c) return PFP_E_ARG;
    for (size_t i = 0; i < c->fa.rec_raw.size(); ++i) { if (raw_off) raw_off[i] = c->fa.rec_raw[i]; if (text_pos) text_pos[i] = c->fa.rec_pos[i]; }
    return PFP_OK;
}
} // extern "C"
#include "parse_host.h"    // stages 1 and 2: parse, dictionary, shard load and merge, the BWT of the parse, pfp_bwt_load
#include "emit_host.h"     // stage 3: emission pre-pass, slot stage, windows and run samples, the SA-window visitor, pfp_bwt_build*
#include "postpass.h"      // the array post-passes: marker array, document arrays, LCP arrays, thresholds
#include "queries.h"       // the queries: matching statistics, count / locate, document listing, MEMs, markers
#include "panel_host.h"    // the variant-panel feed and the VCF file feed on top of it
extern "C" {

// ---- development aid: position-weighted checksum of a device buffer (sum over bytes of (byte + 1) * mix(global position),
// two independent mixes, modulo 2^64): the checksums of the pieces of a buffer add up to the checksum of the whole, so
// outputs that live sliced over several builds / GPUs can be compared with a single-context output without moving them
__global__ __launch_bounds__(BLOCK) void k_checksum(const uint8_t *p, uint64_t bytes, uint64_t offset, unsigned long long *out)
{
    __shared__ unsigned long long red[4];
    const uint64_t i0 = ((uint64_t)blockIdx.x * BLOCK + threadIdx.x) * 16;
    unsigned long long a = 0, b = 0;
    for (int k = 0; k < 16 && i0 + k < bytes; ++k) {
        const uint64_t pos = offset + i0 + k, v = (uint64_t)p[i0 + k] + 1;
        a += v * mix64(pos * 0x9E3779B97F4A7C15ULL + 1); b += v * mix64(pos * 0xD6E8FEB86659FD93ULL + 7);
    }
    unsigned long long ta, tb;
    (void)block_excl_sum(a, red, &ta); (void)block_excl_sum(b, red, &tb);
    if (threadIdx.x == 0) { atomicAdd(&out[0], ta); atomicAdd(&out[1], tb); }
}
int pfp_debug_checksum(pfp_ctx *c, const void *d_buf, uint64_t bytes, uint64_t global_offset, uint64_t out[2])
{
    if (!c || (!d_buf && bytes) || !out) return PFP_E_ARG;
    PFP_HIP(c, hipSetDevice(c->device));
    unsigned long long *d_out; PFP_HIP(c, hipMalloc((void **)&d_out, 16));
    PFP_HIP(c, hipMemsetAsync(d_out, 0, 16, c->stream));
    const uint64_t per = (uint64_t)1 << 34;            // pieces of 16 GiB keep the grid below 2^31 workgroups
    for (uint64_t off = 0; off < bytes; off += per) {
        const uint64_t nb = bytes - off < per ? bytes - off : per;
        PFP_LAUNCH(c, K_MISC, nb, k_checksum, nblocks(nb, 16 * BLOCK), (const uint8_t *)d_buf + off, nb, global_offset + off, d_out);
    }
    unsigned long long h[2];
    PFP_HIP(c, hipMemcpyAsync(h, d_out, 16, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    PFP_HIP(c, hipFree(d_out));
    out[0] = h[0]; out[1] = h[1];
    return PFP_OK;
}

// sum of the 64-bit words of a device buffer and sum of word * (index + 1), modulo 2^64 (bench.py compares the outputs that
// reached host memory with the device-resident ones this way; bytes behind the last whole word count as a zero-padded word)
__global__ __launch_bounds__(BLOCK) void k_wordsum(const uint8_t *p, uint64_t bytes, unsigned long long *out)
{
    __shared__ unsigned long long red[4];
    const uint64_t nw = (bytes + 7) / 8;
    unsigned long long a = 0, b = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < nw; i += (uint64_t)gridDim.x * BLOCK) {
        unsigned long long v = 0;
        if (8 * i + 8 <= bytes) v = ld8(p + 8 * i); else for (uint64_t k = 0; 8 * i + k < bytes; ++k) v |= (unsigned long long)p[8 * i + k] << (8 * k);
        a += v; b += v * (i + 1);
    }
    unsigned long long ta, tb;
    (void)block_excl_sum(a, red, &ta); (void)block_excl_sum(b, red, &tb);
    if (threadIdx.x == 0) { atomicAdd(&out[0], ta); atomicAdd(&out[1], tb); }
}
int pfp_debug_wordsum(pfp_ctx *c, const void *d_buf, uint64_t bytes, uint64_t out[2])
{
    if (!c || (!d_buf && bytes) || !out) return PFP_E_ARG;
    PFP_HIP(c, hipSetDevice(c->device));
    unsigned long long *d_out; PFP_HIP(c, hipMalloc((void **)&d_out, 16));
    PFP_HIP(c, hipMemsetAsync(d_out, 0, 16, c->stream));
    if (bytes) PFP_LAUNCH(c, K_MISC, bytes, k_wordsum, 4096, (const uint8_t *)d_buf, bytes, d_out);
    unsigned long long h[2];
    PFP_HIP(c, hipMemcpyAsync(h, d_out, 16, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    PFP_HIP(c, hipFree(d_out));
    out[0] = h[0]; out[1] = h[1];
    return PFP_OK;
}
// Full-size order check that does not lean on the engine's own sorting: .esa[k] and .ssa[k + 1] are ADJACENT
// rows of the BWT matrix (a run ends, the next one starts), so the suffix at esa[k].sa must be lexicographically smaller than the
// suffix at ssa[k + 1].sa -- compared directly on the text that is still resident (its w Dollars stand for the terminator, which is
// smaller than every base).  One thread per pair, eight bytes per step.  out: pairs checked, order violations, pairs whose rows
// are not adjacent, longest common prefix seen, sum of the common prefixes.
extern "C++" {
template <typename SAT> __global__ __launch_bounds__(BLOCK) void k_check_sample_order(const uint8_t *X, uint64_t n, const SAT *ssa, const SAT *esa, uint64_t r, unsigned long long *out)
{
    const uint64_t k = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k + 1 >= r) return;
    const uint64_t ra = esa[2 * k], a = esa[2 * k + 1], rb = ssa[2 * k + 2], b = ssa[2 * k + 3];
    if (ra + 1 != rb) atomicAdd(&out[2], 1ULL);
    uint64_t h = 0; bool ok = false;
    for (;;) {
        const uint64_t pa = a + h, pb = b + h;
        if (pa > n || pb > n) break;                                        // (cannot happen: the Dollar at n ends every comparison)
        const uint64_t va = ld8(X + pa), vb = ld8(X + pb);                  // the buffer holds w Dollars and slack behind the text
        if (va != vb) {
            const int sh = (__ffsll((long long)(va ^ vb)) - 1) & ~7;
            const uint64_t q = (uint64_t)sh >> 3;
            if (pa + q > n || pb + q > n) break;                            // the difference lies behind the terminator of one of them: not an order
            ok = ((va >> sh) & 0xFF) < ((vb >> sh) & 0xFF); h += q;
            break;
        }
        h += 8;
    }
    if (!ok) atomicAdd(&out[1], 1ULL);
    atomicAdd(&out[0], 1ULL); atomicMax(&out[3], (unsigned long long)h); atomicAdd(&out[4], (unsigned long long)h);
}
}
int pfp_debug_check_sample_order(pfp_ctx *c, uint64_t out[5])
{
    if (!c || !out) return PFP_E_ARG;
    if (c->stage < 3 || !c->d_ssa || !c->d_esa || !c->tb || c->tb_n != c->n || c->slice_rows != c->nout) return PFP_E_STATE;      // needs the text and the whole output's samples
    PFP_HIP(c, hipSetDevice(c->device));
    unsigned long long *d_out; PFP_HIP(c, hipMalloc((void **)&d_out, 40));
    PFP_HIP(c, hipMemsetAsync(d_out, 0, 40, c->stream));
    const uint64_t r = c->runs;
    if (r > 1) {
        if (c->flags & PFP_FLAG_U64) PFP_LAUNCH(c, K_MISC, r * 64, (k_check_sample_order<uint64_t>), nblocks(r, BLOCK), (const uint8_t *)c->tb + 16, c->n, (const uint64_t *)c->d_ssa, (const uint64_t *)c->d_esa, r, d_out);
        else PFP_LAUNCH(c, K_MISC, r * 64, (k_check_sample_order<uint32_t>), nblocks(r, BLOCK), (const uint8_t *)c->tb + 16, c->n, (const uint32_t *)c->d_ssa, (const uint32_t *)c->d_esa, r, d_out);
    }
    unsigned long long h[5];
    PFP_HIP(c, hipMemcpyAsync(h, d_out, 40, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    PFP_HIP(c, hipFree(d_out));
    for (int i = 0; i < 5; ++i) out[i] = h[i];
    return PFP_OK;
}
// Properties of a full suffix array at any size, on the device (the host-side version, tools/big_check.py, needs minutes and
// 10 bytes of host memory per base): every value of [0, n] occurs exactly once (bitmap + atomicOr), row 0 holds n, BWT[row] is the
// text byte in front of SA[row] (0x00 for the one row whose suffix is the whole text).  out: rows checked, values out of range,
// values seen twice, rows with a wrong BWT byte, 0x00 bytes in the BWT.
extern "C++" {
template <typename SAT> __global__ __launch_bounds__(BLOCK) void k_check_sa(const uint8_t *X, uint64_t n, const SAT *sa, const uint8_t *bwt, uint64_t rows, uint32_t *seen, unsigned long long *out)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= rows) return;
    const uint64_t v = sa[i];
    if (v > n) { atomicAdd(&out[1], 1ULL); return; }
    const uint32_t bit = 1u << (v & 31);
    if (atomicOr(&seen[v >> 5], bit) & bit) atomicAdd(&out[2], 1ULL);
    const uint8_t want = v == 0 ? (uint8_t)0 : X[v - 1];
    if (bwt[i] != want || (i == 0 && v != n)) atomicAdd(&out[3], 1ULL);
    if (bwt[i] == 0) atomicAdd(&out[4], 1ULL);
}
}
int pfp_debug_check_sa(pfp_ctx *c, uint64_t out[5])
{
    if (!c || !out) return PFP_E_ARG;
    if (c->stage < 3 || !c->d_sa || !c->have_sa || !c->d_bwt || !c->tb || c->tb_n != c->n || c->slice_rows != c->nout) return PFP_E_STATE;      // needs the text and the whole SA
    PFP_HIP(c, hipSetDevice(c->device));
    const uint64_t rows = c->nout, words = (c->n + 32) / 32 + 1;
    unsigned long long *d_out; uint32_t *seen;
    PFP_HIP(c, hipMalloc((void **)&d_out, 40)); PFP_HIP(c, hipMalloc((void **)&seen, words * 4));
    PFP_HIP(c, hipMemsetAsync(d_out, 0, 40, c->stream)); PFP_HIP(c, hipMemsetAsync(seen, 0, words * 4, c->stream));
    if (c->flags & PFP_FLAG_U64) PFP_LAUNCH(c, K_MISC, rows * 10, (k_check_sa<uint64_t>), nblocks(rows, BLOCK), (const uint8_t *)c->tb + 16, c->n, (const uint64_t *)c->d_sa, (const uint8_t *)c->d_bwt, rows, seen, d_out);
    else PFP_LAUNCH(c, K_MISC, rows * 6, (k_check_sa<uint32_t>), nblocks(rows, BLOCK), (const uint8_t *)c->tb + 16, c->n, (const uint32_t *)c->d_sa, (const uint8_t *)c->d_bwt, rows, seen, d_out);
    unsigned long long h[5];
    PFP_HIP(c, hipMemcpyAsync(h, d_out, 40, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    PFP_HIP(c, hipFree(d_out)); PFP_HIP(c, hipFree(seen));
    out[0] = rows; for (int i = 1; i < 5; ++i) out[i] = h[i];
    return PFP_OK;
}
// The run samples of a -s -r build against its own full outputs, on the device (S-3G: 2.3 G runs = 74 GB of samples, not something
// a test moves to the host): run k starts at row ssa[k].row, a position where the BWT byte changes (or row 0), and ends at
// esa[k].row = ssa[k + 1].row - 1 (the last one at the last row); the values are the SA entries of those rows (src/pfbwt-f.cpp:304-315,
// 325-328).  r itself is the engine's count of byte changes, so r distinct change positions are all of them.
// out: runs checked, runs with a wrong row, runs with a wrong value.
extern "C++" {
template <typename SAT> __global__ __launch_bounds__(BLOCK) void k_check_samples(const SAT *ssa, const SAT *esa, uint64_t r, const SAT *sa, const uint8_t *bwt, uint64_t rows, unsigned long long *out)
{
    const uint64_t k = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= r) return;
    const uint64_t rs = ssa[2 * k], vs = ssa[2 * k + 1], re = esa[2 * k], ve = esa[2 * k + 1];
    bool row_ok = rs < rows && re < rows && rs <= re;
    if (row_ok) {
        row_ok = (k == 0 ? rs == 0 : bwt[rs] != bwt[rs - 1]) && (k + 1 == r ? re + 1 == rows : (uint64_t)ssa[2 * k + 2] == re + 1) && bwt[rs] == bwt[re];
    }
    if (!row_ok) { atomicAdd(&out[1], 1ULL); return; }
    if ((uint64_t)sa[rs] != vs || (uint64_t)sa[re] != ve) atomicAdd(&out[2], 1ULL);
}
}
int pfp_debug_check_samples(pfp_ctx *c, uint64_t out[3])
{
    if (!c || !out) return PFP_E_ARG;
    if (c->stage < 3 || !c->d_sa || !c->have_sa || !c->have_rssa || !c->d_ssa || !c->d_esa || c->slice_rows != c->nout || c->esa_pairs != c->runs) return PFP_E_STATE;
    PFP_HIP(c, hipSetDevice(c->device));
    unsigned long long *d_out; PFP_HIP(c, hipMalloc((void **)&d_out, 24));
    PFP_HIP(c, hipMemsetAsync(d_out, 0, 24, c->stream));
    const uint64_t r = c->runs;
    if (r) {
        if (c->flags & PFP_FLAG_U64) PFP_LAUNCH(c, K_MISC, r * 50, (k_check_samples<uint64_t>), nblocks(r, BLOCK), (const uint64_t *)c->d_ssa, (const uint64_t *)c->d_esa, r, (const uint64_t *)c->d_sa, (const uint8_t *)c->d_bwt, c->nout, d_out);
        else PFP_LAUNCH(c, K_MISC, r * 30, (k_check_samples<uint32_t>), nblocks(r, BLOCK), (const uint32_t *)c->d_ssa, (const uint32_t *)c->d_esa, r, (const uint32_t *)c->d_sa, (const uint8_t *)c->d_bwt, c->nout, d_out);
    }
    unsigned long long h[3];
    PFP_HIP(c, hipMemcpyAsync(h, d_out, 24, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    PFP_HIP(c, hipFree(d_out));
    out[0] = r; out[1] = h[1]; out[2] = h[2];
    return PFP_OK;
}
// page-locked host memory for the callers of pfp_bwt_build_stream / pfp_parse_feed_fasta (they need not link the HIP runtime)
int pfp_host_register(void *p, uint64_t bytes) { if (!p || !bytes) return PFP_E_ARG; if (hipHostRegister(p, (size_t)bytes, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); return PFP_E_HIP; } return PFP_OK; }
int pfp_host_unregister(void *p) { if (!p) return PFP_E_ARG; if (hipHostUnregister(p) != hipSuccess) { (void)hipGetLastError(); return PFP_E_HIP; } return PFP_OK; }

// ---- development aid: time the pair sort on pseudo-random keys (no product path calls this) ----------
// the key of pair i: a pure function of i + seed, so that the check can tell whether a value still sits next to its key
__device__ __forceinline__ uint64_t debug_key(uint64_t i, int bits, uint64_t seed)
{
    uint64_t z = (i + seed) * 0x9E3779B97F4A7C15ULL; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL; z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL; z ^= z >> 31;
    return bits >= 64 ? z : (z & ((1ULL << bits) - 1ULL));
}
__global__ __launch_bounds__(BLOCK) void k_debug_fill(uint64_t *keys, uint32_t *vals, uint64_t n, int bits, uint64_t seed)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    keys[i] = debug_key(i, bits, seed); vals[i] = (uint32_t)i;
}
// bad[0]: neighbours out of order; bad[1]: values that are no index or whose key is not the one k_debug_fill gave that index
__global__ __launch_bounds__(BLOCK) void k_debug_check_sorted(const uint64_t *keys, const uint32_t *vals, uint64_t n, int bits, uint64_t seed, uint32_t *bad)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i + 1 < n && keys[i] > keys[i + 1]) atomicAdd(&bad[0], 1u);
    if (i < n && ((uint64_t)vals[i] >= n || keys[i] != debug_key(vals[i], bits, seed))) atomicAdd(&bad[1], 1u);
}
int pfp_debug_sort(pfp_ctx *c, uint64_t n, int bits, int reps, double *ms_out, uint32_t *unsorted_pairs, uint32_t *wrong_values)
{
    if (!c || n < 2 || n > 0xFFFFFFFFULL || bits < 1 || bits > 64 || reps < 1) return PFP_E_ARG;
    PFP_HIP(c, hipSetDevice(c->device));
    PFP_TRY(ensure_arena(c, n));
    c->arena.reset(); c->stage = 0;
    uint64_t *k0, *k1; uint32_t *v0, *v1, *d_bad;
    PFP_ALLOC_HI(c, k0, uint64_t, n); PFP_ALLOC_HI(c, k1, uint64_t, n); PFP_ALLOC_HI(c, v0, uint32_t, n); PFP_ALLOC_HI(c, v1, uint32_t, n); PFP_ALLOC_HI(c, d_bad, uint32_t, 2);
    BitRange br = {0, bits};
    double best = 1e30;
    uint64_t *sk = k0; uint32_t *sv = v0;
    for (int r = 0; r < reps; ++r) {
        PFP_LAUNCH(c, K_MISC, n * 12, k_debug_fill, nblocks(n, BLOCK), k0, v0, n, bits, (uint64_t)r * 7919);
        PFP_HIP(c, hipStreamSynchronize(c->stream));
        HostTimer t;
        int rc = radix_sort_pairs<uint64_t>(c, k0, v0, k1, v1, n, &br, 1, &sk, &sv);
        if (rc != PFP_OK) return rc;
        PFP_HIP(c, hipStreamSynchronize(c->stream));
        const double ms = t.ms();
        if (ms < best) best = ms;
    }
    PFP_HIP(c, hipMemsetAsync(d_bad, 0, 8, c->stream));
    PFP_LAUNCH(c, K_MISC, n * 12, k_debug_check_sorted, nblocks(n, BLOCK), (const uint64_t *)sk, (const uint32_t *)sv, n, bits, (uint64_t)(reps - 1) * 7919, d_bad);
    uint32_t bad[2] = {0, 0};
    PFP_HIP(c, hipMemcpyAsync(bad, d_bad, 8, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    if (ms_out) *ms_out = best;
    if (unsorted_pairs) *unsorted_pairs = bad[0];
    if (wrong_values) *wrong_values = bad[1];
    c->arena.reset();
    return PFP_OK;
}

// ---- development aid: the device-wide primitives of prims.h on the caller's arrays (tests/test_prims.py) ----------
int pfp_debug_prims_geometry(uint32_t out[4])
{
    if (!out) return PFP_E_ARG;
    out[0] = (uint32_t)RS_TILE; out[1] = (uint32_t)SCAN_TILE; out[2] = SEG_SMALL_MAX; out[3] = (uint32_t)Tunables().seg_grid;
    return PFP_OK;
}
int pfp_debug_emit_large_groups(pfp_ctx *c, uint64_t out[4])
{
    if (!c || !out) return PFP_E_ARG;
    out[0] = out[1] = 0; out[2] = (uint64_t)EG1_BUF; out[3] = (uint64_t)EG2_BUF;
    if (!c->d_lgtaken) return PFP_OK;      // no emission of this context has had the lists yet
    PFP_HIP(c, hipSetDevice(c->device));
    unsigned long long h[2];
    PFP_HIP(c, hipMemcpyAsync(h, c->d_lgtaken, 16, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    out[0] = h[0]; out[1] = h[1];
    return PFP_OK;
}
namespace pfp {
extern "C++" {
// A device buffer of the hooks: DEBUG_GUARD bytes of a pattern in front of and behind its `bytes` bytes (a store past the end of an
// array inside the arena faults nowhere; the guards show it), the bytes themselves filled with `fill`.
constexpr size_t DEBUG_GUARD = 256;              // keeps the 256-byte alignment the arena gives every product buffer
constexpr uint8_t DEBUG_GUARD_BYTE = 0xA5;
struct GuardedBuf { char *raw = nullptr; size_t bytes = 0; template <typename T> T *data() const { return (T *)(raw + DEBUG_GUARD); } };
static int guarded_alloc(pfp_ctx *c, size_t bytes, uint8_t fill, GuardedBuf *g)
{
    g->raw = (char *)c->arena.alloc_hi(bytes + 2 * DEBUG_GUARD); g->bytes = bytes;
    if (!g->raw) return PFP_E_NOMEM;
    PFP_HIP(c, hipMemsetAsync(g->raw, DEBUG_GUARD_BYTE, DEBUG_GUARD, c->stream));
    if (bytes) PFP_HIP(c, hipMemsetAsync(g->raw + DEBUG_GUARD, fill, bytes, c->stream));
    PFP_HIP(c, hipMemsetAsync(g->raw + DEBUG_GUARD + bytes, DEBUG_GUARD_BYTE, DEBUG_GUARD, c->stream));
    return PFP_OK;
}
// *changed += the guard bytes of g that no longer hold the pattern (the stream is synchronised)
static int guards_check(pfp_ctx *c, const GuardedBuf &g, uint32_t *changed)
{
    uint8_t h[2 * DEBUG_GUARD];
    PFP_HIP(c, hipMemcpyAsync(h, g.raw, DEBUG_GUARD, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipMemcpyAsync(h + DEBUG_GUARD, g.raw + DEBUG_GUARD + g.bytes, DEBUG_GUARD, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    uint32_t bad = 0; size_t first = 0;
    for (size_t i = 0; i < 2 * DEBUG_GUARD; ++i) if (h[i] != DEBUG_GUARD_BYTE && !bad++) first = i;
    if (bad && c->tun.verbose) fprintf(stderr, "[pfbwt_hip] guard of the %zu-byte buffer at arena offset %zu (arena %p + %zu): %u bytes changed, the first %s the data at guard byte %zu: %02x\n", g.bytes,
                                       c->arena.offset_of(g.raw), (void *)c->arena.base, c->arena.cap, bad, first < DEBUG_GUARD ? "in front of" : "behind", first % DEBUG_GUARD, h[first]);
    *changed += bad;
    return PFP_OK;
}
template <typename K> static int debug_sort_pairs(pfp_ctx *c, const K *keys, const uint32_t *vals, uint64_t n, const BitRange *ranges, int nranges, K *keys_out, uint32_t *vals_out, uint32_t *changed)
{
    GuardedBuf k[2], v[2];
    for (int i = 0; i < 2; ++i) { PFP_TRY(guarded_alloc(c, n * sizeof(K), 0xEE, &k[i])); PFP_TRY(guarded_alloc(c, n * 4, 0xEE, &v[i])); }
    if (n) {
        PFP_HIP(c, hipMemcpyAsync(k[0].data<K>(), keys, n * sizeof(K), hipMemcpyHostToDevice, c->stream));
        PFP_HIP(c, hipMemcpyAsync(v[0].data<uint32_t>(), vals, n * 4, hipMemcpyHostToDevice, c->stream));
    }
    K *sk; uint32_t *sv;
    PFP_TRY(radix_sort_pairs<K>(c, k[0].data<K>(), v[0].data<uint32_t>(), k[1].data<K>(), v[1].data<uint32_t>(), n, ranges, nranges, &sk, &sv));
    if (n) {
        PFP_HIP(c, hipMemcpyAsync(keys_out, sk, n * sizeof(K), hipMemcpyDeviceToHost, c->stream));
        PFP_HIP(c, hipMemcpyAsync(vals_out, sv, n * 4, hipMemcpyDeviceToHost, c->stream));
    }
    for (int i = 0; i < 2; ++i) { PFP_TRY(guards_check(c, k[i], changed)); PFP_TRY(guards_check(c, v[i], changed)); }
    return PFP_OK;
}
template <typename T, int OP> static int debug_scan(pfp_ctx *c, const T *in, int mode, uint64_t n, T *out, T *total, uint32_t *changed)
{
    GuardedBuf src, dst, tot;
    PFP_TRY(guarded_alloc(c, n * sizeof(T), 0xEE, &dst));
    PFP_TRY(guarded_alloc(c, sizeof(T), 0xEE, &tot));
    T *d_total = total ? tot.data<T>() : nullptr;
    if (mode == 0) {
        PFP_TRY(guarded_alloc(c, n * sizeof(T), 0xEE, &src));
        if (n) PFP_HIP(c, hipMemcpyAsync(src.data<T>(), in, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
        PFP_TRY((device_scan<T, OP>(c, (const T *)src.data<T>(), dst.data<T>(), n, d_total)));
    } else {
        if (n) PFP_HIP(c, hipMemcpyAsync(dst.data<T>(), in, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
        if (mode == 1) PFP_TRY((device_scan<T, OP>(c, (const T *)dst.data<T>(), dst.data<T>(), n, d_total)));
        else PFP_LAUNCH(c, K_SCAN_SPINE, n * sizeof(T) * 2, (k_scan_spine<T, OP>), 1, dst.data<T>(), n, d_total);
    }
    if (n) PFP_HIP(c, hipMemcpyAsync(out, dst.data<T>(), n * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    if (total) PFP_HIP(c, hipMemcpyAsync(total, tot.data<T>(), sizeof(T), hipMemcpyDeviceToHost, c->stream));
    PFP_TRY(guards_check(c, dst, changed)); PFP_TRY(guards_check(c, tot, changed));
    if (mode == 0) {      // the input of an out-of-place scan stays as it was
        PFP_TRY(guards_check(c, src, changed));
        std::vector<T> back((size_t)n);
        if (n) PFP_HIP(c, hipMemcpy(back.data(), src.data<T>(), n * sizeof(T), hipMemcpyDeviceToHost));
        if (n && memcmp(back.data(), in, n * sizeof(T))) *changed += 1;
    }
    return PFP_OK;
}
}
}
// the arena of the context, emptied, for one call of a primitive on n elements
static int debug_prims_begin(pfp_ctx *c, uint64_t n)
{
    PFP_HIP(c, hipSetDevice(c->device));
    PFP_TRY(ensure_arena(c, n));
    c->arena.reset(); c->stage = 0;
    return PFP_OK;
}
int pfp_debug_sort_pairs(pfp_ctx *c, const void *keys, int key_bytes, const uint32_t *vals, uint64_t n, const int *ranges, int nranges, void *keys_out, uint32_t *vals_out, uint32_t *guards_changed)
{
    if (!c || (key_bytes != 4 && key_bytes != 8) || nranges < 0 || nranges > 16 || (nranges && !ranges) || !guards_changed || (n && (!keys || !vals || !keys_out || !vals_out))) return PFP_E_ARG;
    BitRange br[16];
    for (int r = 0; r < nranges; ++r) { br[r].lo = ranges[2 * r]; br[r].hi = ranges[2 * r + 1]; if (br[r].lo < 0 || br[r].hi > 8 * key_bytes || br[r].lo > br[r].hi) return PFP_E_ARG; }
    PFP_TRY(debug_prims_begin(c, n));
    *guards_changed = 0;
    const int rc = key_bytes == 8 ? debug_sort_pairs<uint64_t>(c, (const uint64_t *)keys, vals, n, br, nranges, (uint64_t *)keys_out, vals_out, guards_changed)
                                  : debug_sort_pairs<uint32_t>(c, (const uint32_t *)keys, vals, n, br, nranges, (uint32_t *)keys_out, vals_out, guards_changed);
    c->arena.reset();
    return rc;
}
int pfp_debug_scan(pfp_ctx *c, const void *in, int elem_bytes, int op, int mode, uint64_t n, void *out, void *total, uint32_t *guards_changed)
{
    if (!c || (elem_bytes != 4 && elem_bytes != 8) || (op != 0 && op != 1) || mode < 0 || mode > 2 || !guards_changed || (n && (!in || !out))) return PFP_E_ARG;
    PFP_TRY(debug_prims_begin(c, n));
    *guards_changed = 0;
    int rc;
    if (elem_bytes == 8) rc = op == 0 ? debug_scan<uint64_t, 0>(c, (const uint64_t *)in, mode, n, (uint64_t *)out, (uint64_t *)total, guards_changed)
                                      : debug_scan<uint64_t, 1>(c, (const uint64_t *)in, mode, n, (uint64_t *)out, (uint64_t *)total, guards_changed);
    else rc = op == 0 ? debug_scan<uint32_t, 0>(c, (const uint32_t *)in, mode, n, (uint32_t *)out, (uint32_t *)total, guards_changed)
                      : debug_scan<uint32_t, 1>(c, (const uint32_t *)in, mode, n, (uint32_t *)out, (uint32_t *)total, guards_changed);
    c->arena.reset();
    return rc;
}
static int debug_compact(pfp_ctx *c, const uint32_t *in, const uint32_t *flag, uint64_t n, uint32_t *out, uint32_t *count, uint32_t *changed)
{
    GuardedBuf src, flg, dst, pos, cnt;
    PFP_TRY(guarded_alloc(c, n * 4, 0xEE, &src)); PFP_TRY(guarded_alloc(c, n * 4, 0xEE, &flg)); PFP_TRY(guarded_alloc(c, n * 4, 0xEE, &dst));
    PFP_TRY(guarded_alloc(c, n * 4, 0xEE, &pos)); PFP_TRY(guarded_alloc(c, 4, 0xEE, &cnt));
    if (n) {
        if (in) PFP_HIP(c, hipMemcpyAsync(src.data<uint32_t>(), in, n * 4, hipMemcpyHostToDevice, c->stream));
        PFP_HIP(c, hipMemcpyAsync(flg.data<uint32_t>(), flag, n * 4, hipMemcpyHostToDevice, c->stream));
    }
    PFP_TRY(device_compact(c, in ? (const uint32_t *)src.data<uint32_t>() : nullptr, (const uint32_t *)flg.data<uint32_t>(), n, dst.data<uint32_t>(), pos.data<uint32_t>(), cnt.data<uint32_t>()));
    if (n) PFP_HIP(c, hipMemcpyAsync(out, dst.data<uint32_t>(), n * 4, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipMemcpyAsync(count, cnt.data<uint32_t>(), 4, hipMemcpyDeviceToHost, c->stream));
    PFP_TRY(guards_check(c, src, changed)); PFP_TRY(guards_check(c, flg, changed)); PFP_TRY(guards_check(c, dst, changed));
    PFP_TRY(guards_check(c, pos, changed)); PFP_TRY(guards_check(c, cnt, changed));
    return PFP_OK;
}
int pfp_debug_compact(pfp_ctx *c, const uint32_t *in, const uint32_t *flag, uint64_t n, uint32_t *out, uint32_t *count, uint32_t *guards_changed)
{
    if (!c || !count || !guards_changed || (n && (!flag || !out))) return PFP_E_ARG;
    PFP_TRY(debug_prims_begin(c, n));
    *guards_changed = 0;
    const int rc = debug_compact(c, in, flag, n, out, count, guards_changed);
    c->arena.reset();
    return rc;
}

// ---- gsa/gsacak.h:76-103 drop-ins ------------------------------------------------------------------
static int sacak_int_impl(const uint32_t *s, void *SA, uint64_t n, uint64_t k, bool u64)
{
    if (!s || !SA || n == 0) return -1;
    if (n + 64 >= 0xFFFFFFFFULL) return -1;
    int st = 0;
    pfp_ctx *c = pfp_create(10, 100, 0, 0, (uint64_t)(80 * n + (32ULL << 20)), &st);
    if (!c) return -1;
    int rounds = -1;
    do {
        if (ensure_arena(c, n) != PFP_OK) break;
        uint32_t *dS = (uint32_t *)c->arena.alloc_lo(n * 4), *dSA = (uint32_t *)c->arena.alloc_lo(n * 4), *dR = (uint32_t *)c->arena.alloc_lo(n * 4);
        if (!dS || !dSA || !dR) break;
        if (hipMemcpy(dS, s, n * 4, hipMemcpyHostToDevice) != hipSuccess) break;
        int r = 0;
        if (sort_int_suffixes(c, dS, n, k ? k - 1 : 0, dSA, dR, &r) != PFP_OK) break;
        if (hipStreamSynchronize(c->stream) != hipSuccess) break;
        if (!u64) { if (hipMemcpy(SA, dSA, n * 4, hipMemcpyDeviceToHost) != hipSuccess) break; }
        else {
            std::vector<uint32_t> tmp((size_t)n);
            if (hipMemcpy(tmp.data(), dSA, n * 4, hipMemcpyDeviceToHost) != hipSuccess) break;
            for (uint64_t i = 0; i < n; ++i) ((uint64_t *)SA)[i] = tmp[(size_t)i];
        }
        rounds = r;
    } while (0);
    pfp_destroy(c);
    return rounds;
}
extern "C++" {
// int gsacak(unsigned char *s, uint_t *SA, int_t *LCP, int_t *DA, uint_t n), gsa/gsacak.h:86-96 -- the call of
// include/pfbwt.hpp:211.  s = strings over any byte alphabet (the parser's dictionaries: '-', A, C, G, N, T and Dollar = 2), each
// followed by the separator 1, s[n-1] = 0.  Suffixes are compared up to their separator; suffixes that are byte-identical up to it
// are ordered by position (gsacak.c:877-912) and LCP stops at the separator (:64).
// LCP[i] of SA[i-1], SA[i]: bytes are compared eight at a time; inside runs of one byte (a 10 Mbp run of N is one phrase whose
// suffixes are neighbours in SA) the shorter of the two runs is skipped at once (M: run lengths, see k_ss_runend_marks)
template <typename LT> __global__ __launch_bounds__(BLOCK) void k_gsa_lcp(const uint8_t *D, const uint32_t *SA, const uint32_t *M, uint64_t n, LT *lcp)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    if (i == 0) { lcp[0] = 0; return; }
    const uint64_t x = SA[i - 1], y = SA[i];
    uint64_t h = 0;
    for (;;) {
        const uint64_t px = x + h, py = y + h;
        if (px >= n || py >= n) break;
        const uint8_t cx = D[px];
        if (cx != D[py] || cx <= EndOfWord) break;
        const uint32_t ix = (uint32_t)(n - 1 - px), iy = (uint32_t)(n - 1 - py);
        const uint64_t rx = ix - M[ix] + 1u, ry = iy - M[iy] + 1u;          // lengths of the runs of cx that start at px / py
        if (rx >= 16 && ry >= 16) { h += rx < ry ? rx : ry; continue; }
        const uint64_t a = ld8(D + px), b = ld8(D + py);                     // (the device buffer is padded)
        // first byte that differs or is a separator / terminator: bytes are < 0x80, so (v - 0x02..02) has its high bit set exactly for v <= 1
        const uint64_t stop = (a ^ b) | (((a - 0x0202020202020202ULL) & ~a & 0x8080808080808080ULL));
        if (stop) { h += (uint64_t)(__ffsll((long long)stop) - 1) >> 3; break; }
        h += 8;
    }
    lcp[i] = (LT)h;
}
template <typename LT> __global__ __launch_bounds__(BLOCK) void k_gsa_da(const uint32_t *SA, const uint32_t *wordid, uint64_t n, LT *da)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) da[i] = (LT)wordid[SA[i]];
}
static int gsacak_impl(const uint8_t *s, void *SA, void *LCP, void *DA, uint64_t n, bool u64)
{
    if (!s || !SA || n < 2) return -1;
    if (n + 64 >= 0xFFFFFFFFULL) return -1;
    // the alphabet: bytes 0 (terminator: only at the very end) and 1 (separator) keep their roles; every other byte that occurs gets
    // the next code in byte order.  The parser's own dictionaries ('-' A C G N T and Dollar) take the tuned 16-characters-per-key
    // kernel; any other byte set (another caller of gsa/gsacak.h:86-96) takes the generic one with as many characters as fit 51 bits
    bool seen[256] = {false};
    for (uint64_t i = 0; i < n; ++i) seen[s[i]] = true;
    if (s[n - 1] != 0) return -1;
    for (uint64_t i = 0; i + 1 < n; ++i) if (s[i] == 0) return -1;      // no unique terminator
    bool dict_alphabet = true;
    for (int b = 3; b < 256; ++b) if (seen[b] && !(b == '-' || b == 'A' || b == 'C' || b == 'G' || b == 'N' || b == 'T')) dict_alphabet = false;
    uint8_t code[256]; uint32_t sigma = 2;
    for (int b = 0; b < 256; ++b) code[b] = (uint8_t)(b <= 1 ? b : 0);
    for (int b = 2; b < 256; ++b) if (seen[b]) code[b] = (uint8_t)sigma++;
    uint32_t chars = 0; { unsigned __int128 v = 1; while (chars < 16 && v * sigma < ((unsigned __int128)1 << 51)) { v *= sigma; ++chars; } }
    int st = 0;
    pfp_ctx *c = pfp_create(10, 100, u64 ? PFP_FLAG_U64 : 0u, 0, (uint64_t)(72 * n + (64ULL << 20)), &st);
    if (!c) return -1;
    int rounds = -1;
    auto body = [&]() -> int {
        PFP_TRY(ensure_arena(c, n));
        c->arena.reset();
        c->dsize = n;
        PFP_ALLOC_LO(c, c->d_dict, uint8_t, n + 16);
        PFP_HIP(c, hipMemsetAsync(c->d_dict + n, 0, 16, c->stream));
        PFP_TRY(h2d_copy(c, c->d_dict, s, n));
        // sort_dict_suffixes with a counted round number
        uint64_t *k0, *k1; uint32_t *v0, *v1;
        PFP_ALLOC_LO(c, c->d_gsa, uint32_t, n); PFP_ALLOC_LO(c, c->d_grank, uint2, n);
        const size_t mk = c->arena.mark_hi();
        PFP_ALLOC_HI(c, k0, uint64_t, n); PFP_ALLOC_HI(c, k1, uint64_t, n); PFP_ALLOC_HI(c, v0, uint32_t, n); PFP_ALLOC_HI(c, v1, uint32_t, n);
        if (dict_alphabet) {
            PFP_LAUNCH(c, K_SS_INIT_KEYS, n * 13, k_dict_init_keys, nblocks(n, DK_TILE), (const uint8_t *)c->d_dict, n, k0, v0);
            BitRange full = {0, DK_KEY_BITS};
            PFP_TRY(suffix_sort_doubling<true>(c, n, k0, v0, k1, v1, &full, 1, DK_CHARS, c->d_dict, c->d_gsa, (uint32_t *)nullptr, c->d_grank, &rounds));
        } else {
            uint8_t *d_code; PFP_ALLOC_HI(c, d_code, uint8_t, 256);
            PFP_HIP(c, hipMemcpyAsync(d_code, code, 256, hipMemcpyHostToDevice, c->stream));
            PFP_HIP(c, hipStreamSynchronize(c->stream));
            PFP_LAUNCH(c, K_SS_INIT_KEYS, n * 13, k_dict_init_keys_any, nblocks(n, BLOCK), (const uint8_t *)c->d_dict, n, (const uint8_t *)d_code, sigma, chars, k0, v0);
            BitRange full = {0, 51};
            PFP_TRY(suffix_sort_doubling<true>(c, n, k0, v0, k1, v1, &full, 1, chars, c->d_dict, c->d_gsa, (uint32_t *)nullptr, c->d_grank, &rounds, sigma));
        }
        c->arena.release_hi(mk);
        PFP_HIP(c, hipStreamSynchronize(c->stream));
        if (!u64) PFP_HIP(c, hipMemcpy(SA, c->d_gsa, n * 4, hipMemcpyDeviceToHost));
        else PFP_TRY(download_as_u(c, c->d_gsa, n, SA, true));
        if (LCP) {
            uint32_t *M; PFP_ALLOC_HI(c, M, uint32_t, n);
            PFP_LAUNCH(c, K_MISC, n * 5, k_ss_runend_marks, nblocks(n, BLOCK), (const uint8_t *)c->d_dict, n, M);
            PFP_TRY((device_scan<uint32_t, 1>(c, M, M, n, nullptr)));
            if (u64) { int64_t *d; PFP_ALLOC_HI(c, d, int64_t, n); PFP_LAUNCH(c, K_MISC, n * 40, (k_gsa_lcp<int64_t>), nblocks(n, BLOCK), (const uint8_t *)c->d_dict, (const uint32_t *)c->d_gsa, (const uint32_t *)M, n, d);
                       PFP_HIP(c, hipStreamSynchronize(c->stream)); PFP_HIP(c, hipMemcpy(LCP, d, n * 8, hipMemcpyDeviceToHost)); }
            else { int32_t *d; PFP_ALLOC_HI(c, d, int32_t, n); PFP_LAUNCH(c, K_MISC, n * 36, (k_gsa_lcp<int32_t>), nblocks(n, BLOCK), (const uint8_t *)c->d_dict, (const uint32_t *)c->d_gsa, (const uint32_t *)M, n, d);
                   PFP_HIP(c, hipStreamSynchronize(c->stream)); PFP_HIP(c, hipMemcpy(LCP, d, n * 4, hipMemcpyDeviceToHost)); }
            c->arena.release_hi(mk);
        }
        if (DA) {   // document of every suffix = number of separators in front of it
            uint32_t *flag, *wid; PFP_ALLOC_HI(c, flag, uint32_t, n); PFP_ALLOC_HI(c, wid, uint32_t, n);
            PFP_LAUNCH(c, K_MISC, n * 5, k_eow_flags, nblocks(n, BLOCK), (const uint8_t *)c->d_dict, n, flag);
            PFP_TRY((device_scan<uint32_t, 0>(c, flag, wid, n, nullptr)));
            if (u64) { int64_t *d; PFP_ALLOC_HI(c, d, int64_t, n); PFP_LAUNCH(c, K_MISC, n * 16, (k_gsa_da<int64_t>), nblocks(n, BLOCK), (const uint32_t *)c->d_gsa, (const uint32_t *)wid, n, d);
                       PFP_HIP(c, hipStreamSynchronize(c->stream)); PFP_HIP(c, hipMemcpy(DA, d, n * 8, hipMemcpyDeviceToHost)); }
            else { int32_t *d; PFP_ALLOC_HI(c, d, int32_t, n); PFP_LAUNCH(c, K_MISC, n * 12, (k_gsa_da<int32_t>), nblocks(n, BLOCK), (const uint32_t *)c->d_gsa, (const uint32_t *)wid, n, d);
                   PFP_HIP(c, hipStreamSynchronize(c->stream)); PFP_HIP(c, hipMemcpy(DA, d, n * 4, hipMemcpyDeviceToHost)); }
            c->arena.release_hi(mk);
        }
        return PFP_OK;
    };
    const int rc = body();
    pfp_destroy(c);
    return rc == PFP_OK ? rounds : -1;
}
} // extern "C++"
int pfp_gsacak_u32(const uint8_t *s, uint32_t *SA, int32_t *LCP, int32_t *DA, uint32_t n) { return gsacak_impl(s, SA, LCP, DA, n, false); }
int pfp_gsacak_u64(const uint8_t *s, uint64_t *SA, int64_t *LCP, int64_t *DA, uint64_t n) { return gsacak_impl(s, SA, LCP, DA, n, true); }

int pfp_sacak_int_u32(const uint32_t *s, uint32_t *SA, uint32_t n, uint32_t k) { return sacak_int_impl(s, SA, n, k, false); }
int pfp_sacak_int_u64(const uint32_t *s, uint64_t *SA, uint64_t n, uint64_t k) { return sacak_int_impl(s, SA, n, k, true); }

} // extern "C"

#include "sharded.h"
