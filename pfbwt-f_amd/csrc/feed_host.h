// pfbwt-f_amd/csrc/feed_host.h -- host side of stage 1, feeding: everything that appends to the text of a context or hands it out.
// Records from host and device memory one by one and in batches, the row view, the left context of a shard, pfp_parse_reopen, the text
// view, raw FASTA bytes (kernels: csrc/fasta.h) and FASTA files (reader: csrc/ingest.h).  Every append opens with append_begin (feed_open, then
// append_reserve) and closes with append_done; a feed that is not in this file (csrc/panel_host.h) does the same.
// Host code only; included by pfbwt_hip.hip, whose memory code it uses (ensure_text, reset_results).
#pragma once

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

// ---- one append path -----------------------------------------------------------------------------------------------------------------
// pfparser.hpp:326-331: the 32-bit build stops at 2^32 bases; the 64-bit build here at 2^40 (device positions are 64-bit)
static uint64_t text_limit(const pfp_ctx *c) { return (c->flags & PFP_FLAG_U64) ? (1ULL << 40) : 0xFFFFFFFFULL; }
// a feed into a context in a later stage starts a new text
static int feed_open(pfp_ctx *c)
{
    PFP_HIP(c, hipSetDevice(c->device));
    if (c->stage != 0) reset_results(c);
    return PFP_OK;
}
// Room for `add` more bytes (pads included) in an opened context: PFP_E_TOO_LARGE before anything is reserved or read, then the text,
// its w Dollars and whole tiles behind it.  The bytes go to c->tb + 16 + c->n; append_done publishes them.
static int append_reserve(pfp_ctx *c, uint64_t add)
{
    if (c->n + add + (uint64_t)c->w + 64 >= text_limit(c)) return PFP_E_TOO_LARGE;
    return ensure_text(c, c->n + add + (uint64_t)c->w);
}
// the opening of an append: both.  (A feed that has a question of its own about the opened context -- the view, the panel -- asks it in between.)
static int append_begin(pfp_ctx *c, uint64_t add)
{
    PFP_TRY(feed_open(c));
    return append_reserve(c, add);
}
// records: a hint for the order in which the de-duplication visits the text
static void append_done(pfp_ctx *c, uint64_t add, uint64_t records) { c->n += add; c->tb_n = c->n; c->nseq += records; }

// workgroups of k_feed_batch for `count` rows of `len` bases; 0 = past the grid limit (2^31 workgroups = 8 Tbase)
static uint64_t feed_batch_grid(uint64_t count, uint64_t len)
{
    const uint64_t blocks_per_row = ((len + 15) / 16 + BLOCK - 1) / BLOCK;
    return count * blocks_per_row >= 0x7FFFFFFFULL ? 0 : count * blocks_per_row;
}
// a pending row view (pfp_parse_feed_device_view) becomes text in X: what every entry point that appends to or hands out the text
// does first (the fused scan of pfp_parse_finalize is the one consumer that does not need it)
static int flush_view(pfp_ctx *c)
{
    if (!c->view.src) return PFP_OK;
    const uint64_t count = c->view.count, len = c->view.len;
    PFP_LAUNCH(c, K_MISC, 2 * count * len, k_feed_batch, feed_batch_grid(count, len), c->view.src, count, len, c->view.stride, c->w, c->tb + 16);
    c->view.src = nullptr;
    return PFP_OK;
}
static int feed_common(pfp_ctx *c, const void *src, uint64_t len, int end_of_seq, hipMemcpyKind kind)
{
    if (!c || (!src && len)) return PFP_E_ARG;
    const uint64_t add = len + (end_of_seq ? (uint64_t)c->w : 0);
    PFP_TRY(append_begin(c, add));
    uint8_t *dst = c->tb + 16 + c->n;
    bool in_flight = false;
    if (len && kind == hipMemcpyHostToDevice) PFP_TRY(h2d_copy(c, dst, (const uint8_t *)src, len, &in_flight));
    else if (len) PFP_HIP(c, hipMemcpyAsync(dst, src, (size_t)len, kind, c->stream));
    if (end_of_seq) PFP_HIP(c, hipMemsetAsync(dst + len, 'A', (size_t)c->w, c->stream));      // the w 'A's of pfparser.hpp:335-337
    // the caller may reuse its buffer on return: a pageable source went through the staging ring (its DMA transfers overlap
    // the caller's next read / decompression, include/kseq.h:228), only a page-locked source is read in place
    // (a device source may belong to another context that its owner destroys right after this call -- PfParser::operator+= with a
    // temporary right-hand side, src/merge_pfp.cpp:100-112: unmapping on-demand committed memory does not wait for copies in flight)
    if (in_flight || (len && kind == hipMemcpyDeviceToDevice)) PFP_HIP(c, hipStreamSynchronize(c->stream));
    append_done(c, add, end_of_seq ? 1 : 0);
    return PFP_OK;
}

// ---- raw FASTA bytes (csrc/fasta.h) ---------------------------------------------------------------------------------
constexpr size_t FA_RAW_MAX = (size_t)256 << 20, FA_RAW_MIN = (size_t)1 << 20;
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
// (Not append_begin: how far the text grows is known only once k_fa_scan has run, and the pad of the stream's last record is still to come.)
static int fa_process(pfp_ctx *c, uint64_t len, int slot, bool want_recs, uint64_t rec_base, uint64_t *started)
{
    auto &f = c->fa;
    const uint64_t w = (uint64_t)c->w;
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
    if (n_new + 2 * w + 64 >= text_limit(c)) return PFP_E_TOO_LARGE;
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
    append_done(c, n_new - c->n, 0);      // (the records are counted when the stream ends)
    f.records = rec0 + hdr; f.state = (uint32_t)f.h_tot[2];
    if (started) *started += hdr;
    return PFP_OK;
}
// end of a stream: the pad of its last record (fa_process left room for it); a '+' line seen on the way makes the whole stream PFP_E_ARG
static int fa_finish_stream(pfp_ctx *c)
{
    auto &f = c->fa;
    const uint64_t w = (uint64_t)c->w;
    if (f.started && f.records) {
        PFP_TRY(ensure_text(c, c->n + 2 * w));
        PFP_HIP(c, hipMemsetAsync(c->tb + 16 + c->n, 'A', (size_t)w, c->stream));
        append_done(c, w, 0);
    }
    uint32_t fl = 0;
    if (f.d_tot) { PFP_HIP(c, hipMemcpyAsync(&fl, f.d_tot + 4, 4, hipMemcpyDeviceToHost, c->stream)); PFP_HIP(c, hipStreamSynchronize(c->stream)); PFP_HIP(c, hipMemsetAsync(f.d_tot + 4, 0, 8, c->stream)); }
    c->nseq += f.records;      // (the hint the text de-duplication orders its workgroups by)
    f.started = false; f.state = FA_L; f.records = 0;
    if (fl & 1u) { c->err_ch = '+'; return PFP_E_ARG; }                             // a FASTQ quality section: not handled on the device
    return PFP_OK;
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

#include "ingest.h"      // FASTA files: uses feed_common and the fa_* stages above

extern "C" {

int pfp_parse_feed(pfp_ctx *c, const uint8_t *bases, uint64_t len, int end_of_seq) { if (c) PFP_TRY(flush_view(c)); return feed_common(c, bases, len, end_of_seq, hipMemcpyHostToDevice); }
int pfp_parse_feed_device(pfp_ctx *c, const void *d_bases, uint64_t len, int end_of_seq) { if (c) PFP_TRY(flush_view(c)); return feed_common(c, d_bases, len, end_of_seq, hipMemcpyDeviceToDevice); }
int pfp_parse_feed_device_batch(pfp_ctx *c, const void *d_bases, uint64_t count, uint64_t len, uint64_t stride)
{
    if (!c || (!d_bases && count && len) || stride < len) return PFP_E_ARG;
    if (!count) return PFP_OK;
    PFP_TRY(flush_view(c));
    if (!len) { for (uint64_t k = 0; k < count; ++k) PFP_TRY(feed_common(c, nullptr, 0, 1, hipMemcpyDeviceToDevice)); return PFP_OK; }
    const uint64_t add = count * (len + (uint64_t)c->w), grid = feed_batch_grid(count, len);
    PFP_TRY(append_begin(c, add));
    if (!grid) return PFP_E_TOO_LARGE;
    PFP_LAUNCH(c, K_MISC, 2 * count * len, k_feed_batch, grid, (const uint8_t *)d_bases, count, len, stride, c->w, c->tb + 16 + c->n);
    append_done(c, add, count);
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
    const uint64_t pitch = len + (uint64_t)c->w, add = count * pitch;
    PFP_TRY(append_begin(c, add));
    uint8_t *dst = c->tb + 16 + c->n;
    // pinned host memory: one DMA transfer per record, queued back to back (the runtime's 2-D copy rejects a destination that
    // spans several pieces of the on-demand committed text, csrc/devmem.h), the pads of pfparser.hpp:335-337 by one small kernel
    for (uint64_t k = 0; k < count; ++k) PFP_HIP(c, hipMemcpyAsync(dst + k * pitch, bases + k * stride, (size_t)len, hipMemcpyHostToDevice, c->stream));
    PFP_LAUNCH(c, K_MISC, count * (uint64_t)c->w, k_pad_rows, nblocks(count * (uint64_t)c->w, BLOCK), dst, count, len, pitch, c->w);
    PFP_HIP(c, hipStreamSynchronize(c->stream));      // the caller may reuse its buffer
    append_done(c, add, count);
    return PFP_OK;
}
int pfp_parse_feed_device_view(pfp_ctx *c, const void *d_bases, uint64_t count, uint64_t len, uint64_t stride)
{
    if (!c || !d_bases || !count || !len || stride < len) return PFP_E_ARG;
    PFP_TRY(feed_open(c));
    if (c->n != 0) return PFP_E_STATE;                                   // the view is the whole text of a parse
    const uint64_t add = count * (len + (uint64_t)c->w);
    if (!feed_batch_grid(count, len)) return PFP_E_TOO_LARGE;           // (flush_view launches k_feed_batch on the rows)
    PFP_TRY(append_reserve(c, add));
    c->view.src = (const uint8_t *)d_bases; c->view.count = count; c->view.len = len; c->view.stride = stride;
    append_done(c, add, count);
    return PFP_OK;
}
int pfp_parse_feed_left_context(pfp_ctx *c)
{
    if (!c) return PFP_E_ARG;
    PFP_TRY(feed_open(c));
    if (c->n != 0) return PFP_E_STATE;                            // the context must be the first thing a shard is fed
    const std::vector<uint8_t> a((size_t)c->w, (uint8_t)'A');
    PFP_TRY(feed_common(c, a.data(), a.size(), 0, hipMemcpyHostToDevice));
    c->left_ctx = (uint64_t)c->w;
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
int pfp_parse_reserve(pfp_ctx *c, uint64_t text_bytes)
{
    if (!c) return PFP_E_ARG;
    if (!c->text.live()) c->text_hint = text_bytes;      // sizes the address range of the text; ignored once text has been fed
    return PFP_OK;
}
int pfp_parse_feed_fasta(pfp_ctx *c, const uint8_t *raw, uint64_t len, unsigned flags, uint64_t *nrec)
{
    if (!c || (!raw && len)) return PFP_E_ARG;
    PFP_TRY(feed_open(c));
    return feed_fasta_impl(c, raw, len, flags, nrec);
}
int pfp_parse_fasta_records(pfp_ctx *c, uint64_t *raw_off, uint64_t *text_pos)
{
    if (!c) return PFP_E_ARG;
    for (size_t i = 0; i < c->fa.rec_raw.size(); ++i) { if (raw_off) raw_off[i] = c->fa.rec_raw[i]; if (text_pos) text_pos[i] = c->fa.rec_pos[i]; }
    return PFP_OK;
}
int pfp_parse_feed_fasta_file(pfp_ctx *c, const char *path, unsigned flags, pfp_ingest_info *info)
{
    if (!c || !path) return PFP_E_ARG;
    PFP_TRY(feed_open(c));
    IngestStats st;
    const int rc = ingest_file(c, path, flags, &st);
    if (info) { info->raw_bytes = st.raw_bytes; info->records = st.records; info->n = c->n; info->read_wait_ms = st.read_wait_ms; info->total_ms = st.total_ms; info->mode = st.mode; }
    return rc;
}
int pfp_parse_docs(pfp_ctx *c, uint64_t *count) { if (!c || !count) return PFP_E_ARG; *count = c->doc_names.size(); return PFP_OK; }
int pfp_parse_doc_get(pfp_ctx *c, uint64_t i, const char **name, uint64_t *start)
{
    if (!c || i >= c->doc_names.size()) return PFP_E_ARG;
    if (name) *name = c->doc_names[(size_t)i].c_str();
    if (start) *start = c->doc_starts[(size_t)i];
    return PFP_OK;
}

} // extern "C"
