// pfbwt-f_amd/csrc/queries.h -- the queries over a finished build and their entries: matching statistics (matchstats.h), count and
// locate (runindex.h), document listing (doclist.h), maximal exact matches (mems.h), marker queries (markerquery.h).  Like the post-passes (postpass.h, whose result-slot
// protocol and fetch path they use) each computes into scratch at the high end of the arena and leaves its result in a slot of the
// context at the low end.  The three that take patterns share one batch (PatternBatch), one argument check and one offsets path; the
// counters their kernels fill are named where the kernels are (MsOut, RiOut, MemOut, DlOut, MkOut).
// Host code only; included by pfbwt_hip.hip.
#pragma once

// ---- what the pattern queries share --------------------------------------------------------------------------------------------
// The patterns of one call, bases[offsets[j] .. offsets[j + 1]).  Host: the offsets from 0 and the patterns in order of decreasing
// length, so that the lanes of a wave finish together.  upload() brings them to scratch at the high end -- P with MS_PAD zero bytes
// behind the bases, d_off, d_order -- and normalises the bases like the feed does the text (k_ms_norm, counted under the caller's
// kernel id).
struct PatternBatch {
    const uint8_t *bases; uint64_t np, total;
    std::vector<uint64_t> off; std::vector<uint32_t> order;
    uint8_t *P = nullptr; uint64_t *d_off = nullptr; uint32_t *d_order = nullptr;
    PatternBatch(const uint8_t *b, const uint64_t *offsets, uint64_t np_) : bases(b + offsets[0]), np(np_), total(offsets[np_] - offsets[0]), off((size_t)np_ + 1), order((size_t)np_)
    {
        for (uint64_t j = 0; j <= np; ++j) off[(size_t)j] = offsets[j] - offsets[0];
        for (uint64_t j = 0; j < np; ++j) order[(size_t)j] = (uint32_t)j;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return off[(size_t)a + 1] - off[a] > off[(size_t)b + 1] - off[b]; });
    }
    int upload(pfp_ctx *c, int kernel_id)
    {
        PFP_ALLOC_HI(c, P, uint8_t, total + MS_PAD); PFP_ALLOC_HI(c, d_off, uint64_t, np + 1); PFP_ALLOC_HI(c, d_order, uint32_t, np);
        PFP_HIP(c, hipMemsetAsync(P + total, 0, MS_PAD, c->stream));
        if (total) PFP_TRY(h2d_copy(c, P, bases, total));
        PFP_TRY(h2d_copy(c, (uint8_t *)d_off, (const uint8_t *)off.data(), (np + 1) * 8));      // (h2d_copy has read its source when it returns)
        if (np) PFP_TRY(h2d_copy(c, (uint8_t *)d_order, (const uint8_t *)order.data(), np * 4));
        if (total) PFP_LAUNCH(c, kernel_id, total * 2, k_ms_norm, nblocks(total, 16 * BLOCK), P, total, (int)((c->flags & PFP_FLAG_NON_ACGT_TO_A) != 0));
        return PFP_OK;
    }
};
// What every entry refuses of a batch behind its null pointers and its state, in this order: too many patterns, descending offsets,
// more than max_total bases (pfp_ms_query with U = 4), a 0 byte (with PFP_FLAG_NON_ACGT_TO_A it becomes 'A').
static int pattern_args_check(const pfp_ctx *c, const uint8_t *bases, const uint64_t *offsets, uint64_t np, uint64_t max_total = ~0ULL)
{
    if (np > 0xFFFFFFFFULL) return PFP_E_TOO_LARGE;
    for (uint64_t j = 0; j < np; ++j) if (offsets[j + 1] < offsets[j]) return PFP_E_ARG;
    const uint64_t total = offsets[np] - offsets[0];
    if (total > max_total) return PFP_E_TOO_LARGE;
    if (!(c->flags & PFP_FLAG_NON_ACGT_TO_A) && total && memchr(bases + offsets[0], 0, (size_t)total)) return PFP_E_ARG;
    return PFP_OK;
}
// the records of a FASTA / FASTQ file as the patterns of query(bases, offsets, npatterns): the bases with one byte in front (never a
// NULL pointer), the records' borders behind it
template <typename F> static int pattern_file_query(const char *path, F query)
{
    gzFile fp = strcmp(path, "-") ? gzopen(path, "r") : gzdopen(0, "r");
    if (!fp) return PFP_E_IO;
    gzbuffer(fp, 1 << 20);
    HostRecordReader rd; rd.fp = fp; rd.buf.resize(1 << 20);
    std::string name, seq;
    std::vector<uint8_t> bases(1, 0); std::vector<uint64_t> off(1, 0);
    while (rd.next(name, seq)) { bases.insert(bases.end(), seq.begin(), seq.end()); off.push_back(bases.size() - 1); }
    int zerr = Z_OK;
    (void)gzerror(fp, &zerr);
    gzclose(fp);
    if (zerr != Z_OK && zerr != Z_STREAM_END) return PFP_E_IO;                                  // a read error or a damaged gzip stream: no answer for half a file
    return query(bases.data() + 1, off.data(), off.size() - 1);
}
// the host offsets of a result (one more than there are patterns) for the caller; made: the result and its offsets are there
static int offsets_get(bool made, const std::vector<uint64_t> &v, uint64_t *dst, uint64_t *npatterns)
{
    if (!made) return PFP_E_STATE;
    if (npatterns) *npatterns = v.size() - 1;
    if (dst) memcpy(dst, v.data(), v.size() * 8);
    return PFP_OK;
}
static int write_all(int fd, const void *ptr, size_t bytes)
{
    for (const char *b = (const char *)ptr; bytes;) { const ssize_t w = write(fd, b, bytes); if (w <= 0) return PFP_E_IO; b += w; bytes -= (size_t)w; }
    return PFP_OK;
}

// ---- matching-statistics index and queries (include/pfbwt_hip.h: pfp_ms_index, pfp_ms_query; csrc/matchstats.h) ------------------
static ResultFamily ms_family(const pfp_ctx *c) { return {2, {{c->ms.p[0], c->ms_bases}, {c->ms.p[1], c->ms_bases}, {nullptr, 0}}, true}; }
static bool has_ms_index(const pfp_ctx *c) { return c->msi.p[0] && c->msx.dir; }
template <typename T> static MsView<T> ms_view(const pfp_ctx *c)
{
    return {(const T *)c->d_ssa, (const T *)c->d_esa, (const T *)c->msx.thr, (const T *)c->msx.lfhead, c->msx.head, c->msx.sorted, c->msx.sym, c->msx.dir, c->msx.B, c->runs, c->n};
}
// The run arrays that the matching-statistics index and the count / locate index share (each owns its copies): at the low end, in
// this order, [the threshold rows when thr_src is given,] lfhead, head, sorted, sym, the run directory with B from ms_dir_log2.
// PFP_E_STATE: a run of EndOfWord bytes.
template <typename T> static int run_arrays_build(pfp_ctx *c, const T *thr_src, MsIndex *out)
{
    const uint64_t r = c->runs, nrows = c->nout;
    uint32_t B = 0;
    if (c->tun.ms_dir_log2 >= 0) B = (uint32_t)c->tun.ms_dir_log2;
    else while (B < (uint32_t)MS_DIR_LOG2_MAX && (nrows >> (B + 1)) >= r) ++B;          // about one run per block
    while (((nrows - 1) >> B) + 3 > 0xFFFFFFFFULL) ++B;
    const uint64_t nblk = ((nrows - 1) >> B) + 1;                           // blocks that hold a row
    MsIndex x;
    x.B = B;
    T *thr = nullptr, *lfhead;
    if (thr_src) PFP_ALLOC_LO(c, thr, T, r);
    PFP_ALLOC_LO(c, lfhead, T, r); PFP_ALLOC_LO(c, x.head, uint8_t, r); PFP_ALLOC_LO(c, x.sorted, uint32_t, r);
    PFP_ALLOC_LO(c, x.sym, uint32_t, 257); PFP_ALLOC_LO(c, x.dir, uint32_t, nblk + 1);
    x.thr = thr; x.lfhead = lfhead;
    const size_t mk = c->arena.mark_hi();
    uint32_t *kv[4], *sk, *sv, *pos; T *len; unsigned long long *d_bad;
    for (uint32_t *&b : kv) PFP_ALLOC_HI(c, b, uint32_t, r);
    PFP_ALLOC_HI(c, pos, uint32_t, r); PFP_ALLOC_HI(c, len, T, r); PFP_ALLOC_HI(c, d_bad, unsigned long long, 1);
    PFP_HIP(c, hipMemsetAsync(d_bad, 0, 8, c->stream));
    PFP_LAUNCH(c, K_MS_INDEX, r * (1 + sizeof(T)), (k_thr_heads<T>), nblocks(r, BLOCK), (const uint8_t *)c->d_bwt, (const T *)c->d_ssa, r, nrows, kv[0], kv[1]);
    const BitRange byte_range = {0, 8};
    PFP_TRY((radix_sort_pairs<uint32_t>(c, kv[0], kv[1], kv[2], kv[3], r, &byte_range, 1, &sk, &sv)));
    PFP_LAUNCH(c, K_MS_INDEX, r * 8, k_thr_inverse, nblocks(r, BLOCK), (const uint32_t *)sv, r, pos);
    PFP_LAUNCH(c, K_MS_INDEX, r * (12 + 3 * sizeof(T)), (k_ms_sorted<T>), nblocks(r, BLOCK), (const uint32_t *)sk, (const uint32_t *)sv, (const T *)c->d_ssa, r, nrows, len, x.sorted, x.sym, d_bad);
    PFP_TRY((device_scan<T, 0>(c, len, len, r, (T *)nullptr)));
    PFP_HIP(c, hipMemsetAsync(x.dir, 0, (size_t)nblk * 4, c->stream));
    PFP_LAUNCH(c, K_MS_INDEX, r * (9 + 5 * sizeof(T)) + (nblk + 1) * 4, (k_ms_runs<T>), nblocks(r, BLOCK), (const uint32_t *)pos, (const uint32_t *)sk, (const T *)len, thr_src, (const T *)c->d_ssa, r, nrows, B, nblk,
               x.head, lfhead, thr, x.dir);
    PFP_TRY((device_scan<uint32_t, 1>(c, x.dir, x.dir, nblk, (uint32_t *)nullptr)));
    unsigned long long bad = 0;
    PFP_HIP(c, hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    c->arena.release_hi(mk);
    if (bad) return PFP_E_STATE;                                           // a run of EndOfWord bytes: this .bwt is not the BWT of the text
    *out = x;
    return PFP_OK;
}
template <typename T> static int ms_index_impl(pfp_ctx *c)
{
    PostResult res(c, c->msi);
    c->msx = MsIndex();
    MsIndex x;
    PFP_TRY(run_arrays_build<T>(c, (const T *)c->thr.p[0], &x));
    res.commit(x.thr);
    c->msx = x;
    return PFP_OK;
}
template <typename T> static int ms_query_impl(pfp_ctx *c, const uint8_t *bases, const uint64_t *offsets, uint64_t np, pfp_ms_info *info)
{
    PatternBatch pb(bases, offsets, np);
    const uint64_t total = pb.total, n = c->n;
    const uint8_t *X = (const uint8_t *)c->tb + 16;
    PostResult res(c, c->ms);
    c->ms_patterns = c->ms_bases = 0; c->ms_off.clear();
    T *ptr, *len;
    PFP_ALLOC_LO(c, ptr, T, total); PFP_ALLOC_LO(c, len, T, total);
    const size_t mk = c->arena.mark_hi();
    T *bp, *fl, *d_cnt; unsigned long long *d_out;
    PFP_TRY(pb.upload(c, K_MS_POINTERS));
    PFP_ALLOC_HI(c, bp, T, total); PFP_ALLOC_HI(c, fl, T, total); PFP_ALLOC_HI(c, d_cnt, T, 1); PFP_ALLOC_HI(c, d_out, unsigned long long, OUT_BLOCK);
    PFP_HIP(c, hipMemsetAsync(d_out, 0, sizeof(unsigned long long) * OUT_BLOCK, c->stream));
    unsigned long long h[OUT_BLOCK] = {};
    uint64_t nbreaks = 0;
    if (total) {
        const MsView<T> ix = ms_view<T>(c);
        PFP_LAUNCH(c, K_MS_POINTERS, total * (1 + 2 * sizeof(T)), (k_ms_pointers<T>), nblocks(np, BLOCK), ix, (const uint8_t *)pb.P, (const uint64_t *)pb.d_off, (const uint32_t *)pb.d_order, np, ptr, bp, d_out);
        // the breaks, one after the other
        PFP_LAUNCH(c, K_MS_BREAKS, total * 2 * sizeof(T), (k_ms_break_flags<T>), nblocks(total, BLOCK), (const T *)bp, total, fl);
        PFP_TRY((device_scan<T, 0>(c, fl, fl, total, d_cnt)));
        T cnt = 0;
        PFP_HIP(c, hipMemcpyAsync(&cnt, d_cnt, sizeof(T), hipMemcpyDeviceToHost, c->stream));
        PFP_HIP(c, hipStreamSynchronize(c->stream));
        nbreaks = cnt;
        T *list; MsLong *queue;
        PFP_ALLOC_HI(c, list, T, nbreaks); PFP_ALLOC_HI(c, queue, MsLong, nbreaks);
        PFP_LAUNCH(c, K_MS_BREAKS, total * 2 * sizeof(T) + nbreaks * sizeof(T), (k_ms_break_list<T>), nblocks(total, BLOCK), (const T *)bp, (const T *)fl, total, list);
        const uint64_t cap = c->tun.ms_long_min;
        PFP_LAUNCH(c, K_MS_BREAKS, nbreaks * (32 + 3 * sizeof(T)), (k_ms_breaks<T>), nblocks(nbreaks, BLOCK), X, n, (const uint8_t *)pb.P, (const uint64_t *)pb.d_off, np, (const T *)list, nbreaks, (const T *)ptr, cap,
                   len, queue, nbreaks, d_out);
        PFP_LAUNCH(c, K_MS_LONG, 0, (k_ms_long<T>), wave_grid(nbreaks, MS_LONG_WG), X, (const uint8_t *)pb.P, (const MsLong *)queue, nbreaks, (const T *)ptr, cap / 16 * 16, len, d_out);
        // every other position from its last break
        PFP_TRY((device_scan<T, 1>(c, bp, bp, total, (T *)nullptr)));
        PFP_LAUNCH(c, K_MS_FILL, total * 3 * sizeof(T), (k_ms_fill<T>), nblocks(total, BLOCK), (const T *)bp, total, len);
        PFP_HIP(c, hipMemcpyAsync(h, d_out, sizeof h, hipMemcpyDeviceToHost, c->stream));
    }
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    c->arena.release_hi(mk);
    res.commit(ptr, len);
    c->ms_patterns = np; c->ms_bases = total; c->ms_off.swap(pb.off);
    if (info) { info->patterns = np; info->bases = total; info->match = h[MS_MATCH]; info->up = h[MS_UP]; info->down = h[MS_DOWN]; info->absent = h[MS_ABSENT]; info->breaks = nbreaks; info->long_breaks = h[MS_LONG_BREAKS]; info->max_len = h[MS_MAX_LEN]; }
    return PFP_OK;
}

int pfp_ms_index(pfp_ctx *c)
{
    if (!c) return PFP_E_ARG;
    if (!has_build(c) || !holds_build_text(c)) return PFP_E_STATE;
    if (c->slice_rows != c->nout || c->slice_begin) return PFP_E_STATE;                        // a slice
    if (!has_run_samples(c) || !c->runs || !c->thr.p[0]) return PFP_E_STATE;
    if (c->runs > 0xFFFFFFFFULL) return PFP_E_TOO_LARGE;                                       // (run indices are 32-bit values)
    return post_entry(c, [&](auto t) { return ms_index_impl<decltype(t)>(c); });
}
int pfp_ms_query(pfp_ctx *c, const uint8_t *bases, const uint64_t *offsets, uint64_t npatterns, pfp_ms_info *info)
{
    if (!c || !bases || !offsets) return PFP_E_ARG;
    if (!has_ms_index(c) || !has_build(c) || !holds_build_text(c)) return PFP_E_STATE;
    PFP_TRY(pattern_args_check(c, bases, offsets, npatterns, (c->flags & PFP_FLAG_U64) ? ~0ULL : 0xFFFFFFF0ULL));      // (U = 4: one value per base, and their sums, in 32 bits)
    return post_entry(c, [&](auto t) { return ms_query_impl<decltype(t)>(c, bases, offsets, npatterns, info); });
}
int pfp_ms_query_file(pfp_ctx *c, const char *path, pfp_ms_info *info)
{
    if (!c || !path) return PFP_E_ARG;
    if (!has_ms_index(c)) return PFP_E_STATE;
    return pattern_file_query(path, [&](const uint8_t *bases, const uint64_t *off, uint64_t np) { return pfp_ms_query(c, bases, off, np, info); });
}
int pfp_ms_offsets_get(pfp_ctx *c, uint64_t *offsets, uint64_t *npatterns)
{
    if (!c) return PFP_E_ARG;
    return offsets_get(c->ms.p[0] && c->ms_off.size() == c->ms_patterns + 1, c->ms_off, offsets, npatterns);
}
int pfp_ms_get(pfp_ctx *c, void *ptr, void *len)
{
    if (!c) return PFP_E_ARG;
    void *const dst[2] = {ptr, len};
    return family_get(c, ms_family(c), dst);
}
int pfp_ms_device_ptrs(pfp_ctx *c, const void **d_ptr, const void **d_len)
{
    if (!c) return PFP_E_ARG;
    const void **const out[2] = {d_ptr, d_len};
    return family_device_ptrs(ms_family(c), out);
}
int pfp_ms_write(pfp_ctx *c, int fd_ptr, int fd_len)
{
    if (!c) return PFP_E_ARG;
    const int fd[2] = {fd_ptr, fd_len};
    return family_write(c, ms_family(c), fd);
}

// ---- count / locate index and queries (include/pfbwt_hip.h: pfp_ri_index, pfp_ri_count, pfp_ri_locate; csrc/runindex.h) ------------
static ResultFamily ri_family(const pfp_ctx *c) { return {2, {{c->ri.p[0], c->ri_patterns}, {c->ri.p[1], c->ri_reported}, {nullptr, 0}}, false}; }
static bool has_ri_index(const pfp_ctx *c) { return c->rii.p[0] && c->rix.run.dir && c->rix.pdir; }
// (a loaded state has no text length of its own: n from the rows)
template <typename T> static MsView<T> ri_view(const pfp_ctx *c)
{
    const MsIndex &x = c->rix.run;
    return {(const T *)c->d_ssa, (const T *)c->d_esa, (const T *)nullptr, (const T *)x.lfhead, x.head, x.sorted, x.sym, x.dir, x.B, c->runs, c->nout - 1};
}
template <typename T> static int ri_index_impl(pfp_ctx *c)
{
    const uint64_t r = c->runs, n = c->nout - 1;
    PostResult res(c, c->rii);
    c->rix = RiIndex();
    RiIndex x;
    PFP_TRY(run_arrays_build<T>(c, (const T *)nullptr, &x.run));
    uint32_t B = 0;
    if (c->tun.ri_dir_log2 >= 0) B = (uint32_t)c->tun.ri_dir_log2;
    else while (B < (uint32_t)RI_DIR_LOG2_MAX && ((n + 1) >> (B + 1)) >= r) ++B;        // about one run start per block
    while ((n >> B) + 2 > 0xFFFFFFFFULL) ++B;
    const uint64_t nblk = n >> B;
    T *pq, *pv;
    PFP_ALLOC_LO(c, pq, T, r); PFP_ALLOC_LO(c, pv, T, r); PFP_ALLOC_LO(c, x.pdir, uint32_t, nblk + 2);
    x.pq = pq; x.pv = pv; x.PB = B;
    const size_t mk = c->arena.mark_hi();
    uint64_t *k0, *k1, *sk; uint32_t *v0, *v1, *sv; unsigned long long *d_bad;
    PFP_ALLOC_HI(c, k0, uint64_t, r); PFP_ALLOC_HI(c, k1, uint64_t, r); PFP_ALLOC_HI(c, v0, uint32_t, r); PFP_ALLOC_HI(c, v1, uint32_t, r); PFP_ALLOC_HI(c, d_bad, unsigned long long, 1);
    PFP_HIP(c, hipMemsetAsync(d_bad, 0, 8, c->stream));
    PFP_LAUNCH(c, K_RI_INDEX, r * (sizeof(T) + 12), (k_plcp_keys<T>), nblocks(r, BLOCK), (const T *)c->d_ssa, r, k0, v0);
    const BitRange range = {0, bits_for(n)};
    PFP_TRY((radix_sort_pairs<uint64_t>(c, k0, v0, k1, v1, r, &range, 1, &sk, &sv)));
    PFP_HIP(c, hipMemsetAsync(x.pdir, 0, (size_t)(nblk + 2) * 4, c->stream));
    PFP_LAUNCH(c, K_RI_INDEX, r * (12 + 3 * sizeof(T)) + (nblk + 2) * 4, (k_ri_phi_fill<T>), nblocks(r, BLOCK), (const uint64_t *)sk, (const uint32_t *)sv, (const T *)c->d_esa, r, n, B, nblk, pq, pv, x.pdir, d_bad);
    PFP_TRY((device_scan<uint32_t, 1>(c, x.pdir, x.pdir, nblk + 2, (uint32_t *)nullptr)));
    unsigned long long bad = 0;
    PFP_HIP(c, hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    c->arena.release_hi(mk);
    if (bad) return PFP_E_CORRUPT;                                         // the positions of the run starts are not distinct text positions
    res.commit(x.run.lfhead);
    c->rix = x;
    return PFP_OK;
}
// The part of a locate behind the search, shared by the patterns of pfp_ri_locate and the MEMs of pfp_mem_find: np strings with their
// intervals lo / cnt and toeholds top (scratch or results of the caller).  Cuts the reported rows into pieces, sums pieces and rows,
// allocates pos at the low end and fills it by phi (route 1) or from the resident SA (route 2).  ooff: np + 1 values, where the
// positions of every string start in pos; tot[0] = pieces, tot[1] = reported values; d_out: the counters of ri_wave_sums / k_ri_walk.
// Its scratch stays at the high end for the caller to release; the stream is left running.
// A caller that reduces the positions instead of keeping them (pfp_ri_docs) passes lo / cnt / top of a sub-range of its strings, asks
// for pos at the high end too (pos_hi) and takes the device copy of ooff (d_obase: np + 1 values, scratch).
template <typename T> static int ri_report(pfp_ctx *c, const MsView<T> &ix, const T *lo, const T *cnt, const T *top, uint64_t np, int route, uint64_t max_occ, unsigned long long *d_out, T **pos_out,
                                           std::vector<uint64_t> *ooff, unsigned long long tot[2], bool pos_hi = false, const unsigned long long **d_obase = nullptr)
{
    // the pieces and the reported rows of every pattern, and where they start
    unsigned long long *pc, *rc; uint32_t *kfirst; T *pos;
    PFP_ALLOC_HI(c, pc, unsigned long long, np + 1); PFP_ALLOC_HI(c, rc, unsigned long long, np + 1); PFP_ALLOC_HI(c, kfirst, uint32_t, np);
    if (np) PFP_LAUNCH(c, K_RI_SEARCH, np * (20 + 2 * sizeof(T)), (k_ri_pieces<T>), nblocks(np, BLOCK), ix, lo, cnt, np, max_occ, pc, rc, kfirst);
    PFP_TRY((device_scan<unsigned long long, 0>(c, pc, pc, np, pc + np)));
    PFP_TRY((device_scan<unsigned long long, 0>(c, rc, rc, np, rc + np)));
    PFP_HIP(c, hipMemcpyAsync(&tot[0], pc + np, 8, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipMemcpyAsync(ooff->data(), rc, (size_t)(np + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    tot[1] = (*ooff)[(size_t)np];
    if (pos_hi) PFP_ALLOC_HI(c, pos, T, tot[1]);
    else PFP_ALLOC_LO(c, pos, T, tot[1]);                                // result: low end, survives the release of the scratch
    if (tot[1] && route == 1) {
        const RiPhi<T> ph = {(const T *)c->rix.pq, (const T *)c->rix.pv, c->rix.pdir, c->rix.PB, c->runs, c->nout - 1};
        PFP_LAUNCH(c, K_RI_WALK, tot[1] * 3 * sizeof(T), (k_ri_walk<T>), nblocks(tot[0], BLOCK), ix, ph, lo, cnt, top, (const uint32_t *)kfirst, (const unsigned long long *)pc,
                   (const unsigned long long *)rc, np, (uint64_t)tot[0], pos, d_out);
    } else if (tot[1]) {
        PFP_LAUNCH(c, K_RI_ROWS, tot[1] * 2 * sizeof(T), (k_ri_rows<T>), nblocks(tot[1], BLOCK), (const T *)c->d_sa, c->nout - 1, lo, cnt, (const unsigned long long *)rc, np, (uint64_t)tot[1], pos);
    }
    *pos_out = pos;
    if (d_obase) *d_obase = rc;
    return PFP_OK;
}
// route: 0 count only, 1 phi, 2 the resident SA
template <typename T> static int ri_query_impl(pfp_ctx *c, const uint8_t *bases, const uint64_t *offsets, uint64_t np, int route, uint64_t max_occ, pfp_ri_info *info)
{
    PatternBatch pb(bases, offsets, np);
    const uint64_t total = pb.total;
    PostResult res(c, c->ri);
    c->ri_patterns = c->ri_reported = 0; c->ri_route = 0; c->ri_off.clear();
    T *cnt, *pos = nullptr;
    PFP_ALLOC_LO(c, cnt, T, np);
    const size_t mk = c->arena.mark_hi();
    T *lo, *top = nullptr; unsigned long long *d_out;
    PFP_TRY(pb.upload(c, K_RI_SEARCH));
    PFP_ALLOC_HI(c, lo, T, np); PFP_ALLOC_HI(c, d_out, unsigned long long, OUT_BLOCK);
    if (route) PFP_ALLOC_HI(c, top, T, np);                                // (the toehold: locate only)
    PFP_HIP(c, hipMemsetAsync(d_out, 0, sizeof(unsigned long long) * OUT_BLOCK, c->stream));
    unsigned long long h[OUT_BLOCK] = {}, tot[2] = {0, 0};
    std::vector<uint64_t> ooff((size_t)np + 1, 0);
    const MsView<T> ix = ri_view<T>(c);
    if (np && route) PFP_LAUNCH(c, K_RI_SEARCH, total + np * 3 * sizeof(T), (k_ri_search<T, true>), nblocks(np, BLOCK), ix, (const uint8_t *)pb.P, (const uint64_t *)pb.d_off, (const uint32_t *)pb.d_order, np, lo, cnt, top, d_out);
    else if (np) PFP_LAUNCH(c, K_RI_SEARCH, total + np * 2 * sizeof(T), (k_ri_search<T, false>), nblocks(np, BLOCK), ix, (const uint8_t *)pb.P, (const uint64_t *)pb.d_off, (const uint32_t *)pb.d_order, np, lo, cnt, top, d_out);
    if (route) PFP_TRY(ri_report<T>(c, ix, lo, cnt, top, np, route, max_occ, d_out, &pos, &ooff, tot));
    PFP_HIP(c, hipMemcpyAsync(h, d_out, sizeof h, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    c->arena.release_hi(mk);
    res.commit(cnt, pos);
    c->ri_patterns = np; c->ri_reported = tot[1]; c->ri_route = route; c->ri_off.swap(ooff);
    if (c->tun.verbose) fprintf(stderr, "[pfbwt_hip] ri query: %llu patterns, %llu steps, %llu pieces\n", (unsigned long long)np, h[RI_STEPS], (unsigned long long)tot[0]);
    if (info) {
        info->patterns = np; info->bases = total; info->found = h[RI_FOUND]; info->occurrences = h[RI_OCCURRENCES]; info->reported = tot[1]; info->pieces = tot[0]; info->max_count = h[RI_MAX_COUNT];
        info->max_piece = h[RI_MAX_PIECE]; info->phi_steps = h[RI_PHI_STEPS]; info->route = (uint64_t)route;
    }
    return PFP_OK;
}

// what index and queries need of the build: the whole output with run samples; neither the text nor the thresholds
static int ri_state(const pfp_ctx *c)
{
    if (!has_build(c) || c->nout < 2) return PFP_E_STATE;
    if (c->slice_rows != c->nout || c->slice_begin) return PFP_E_STATE;                        // a slice
    if (!has_run_samples(c) || !c->runs || c->esa_pairs != c->runs) return PFP_E_STATE;
    if (c->runs > 0xFFFFFFFFULL) return PFP_E_TOO_LARGE;                                       // (run indices are 32-bit values)
    return PFP_OK;
}
int pfp_ri_index(pfp_ctx *c)
{
    if (!c) return PFP_E_ARG;
    PFP_TRY(ri_state(c));
    return post_entry(c, [&](auto t) { return ri_index_impl<decltype(t)>(c); });
}
// the route of a locate (pfp_debug_set "ri_route"): 1 phi, 2 the resident SA; 0: the SA is asked for and there is none
static int ri_locate_route(const pfp_ctx *c)
{
    const int route = c->tun.ri_route == 1 ? 1 : c->tun.ri_route == 2 ? 2 : has_whole_sa(c) ? 2 : 1;
    return route == 2 && !has_whole_sa(c) ? 0 : route;
}
// locate: 0 = count
static int ri_query(pfp_ctx *c, const uint8_t *bases, const uint64_t *offsets, uint64_t npatterns, int locate, uint64_t max_occ, pfp_ri_info *info)
{
    if (!c || !bases || !offsets) return PFP_E_ARG;
    if (!has_ri_index(c) || ri_state(c) != PFP_OK) return PFP_E_STATE;
    PFP_TRY(pattern_args_check(c, bases, offsets, npatterns));
    int route = 0;
    if (locate && !(route = ri_locate_route(c))) return PFP_E_STATE;
    return post_entry(c, [&](auto t) { return ri_query_impl<decltype(t)>(c, bases, offsets, npatterns, route, max_occ, info); });
}
int pfp_ri_count(pfp_ctx *c, const uint8_t *bases, const uint64_t *offsets, uint64_t npatterns, pfp_ri_info *info) { return ri_query(c, bases, offsets, npatterns, 0, 0, info); }
int pfp_ri_locate(pfp_ctx *c, const uint8_t *bases, const uint64_t *offsets, uint64_t npatterns, uint64_t max_occ, pfp_ri_info *info) { return ri_query(c, bases, offsets, npatterns, 1, max_occ, info); }
int pfp_ri_query_file(pfp_ctx *c, const char *path, int locate, uint64_t max_occ, pfp_ri_info *info)
{
    if (!c || !path) return PFP_E_ARG;
    if (!has_ri_index(c)) return PFP_E_STATE;
    return pattern_file_query(path, [&](const uint8_t *bases, const uint64_t *off, uint64_t np) { return ri_query(c, bases, off, np, locate, max_occ, info); });
}
int pfp_ri_offsets_get(pfp_ctx *c, uint64_t *offsets, uint64_t *npatterns)
{
    if (!c) return PFP_E_ARG;
    return offsets_get(c->ri.p[1] && c->ri_off.size() == c->ri_patterns + 1, c->ri_off, offsets, npatterns);      // (p[1]: null before a locate)
}
int pfp_ri_get(pfp_ctx *c, void *cnt, void *pos)
{
    if (!c) return PFP_E_ARG;
    if (!c->ri.p[0]) return PFP_E_STATE;                                                       // no query yet
    void *const dst[2] = {cnt, pos};
    return family_get(c, ri_family(c), dst);
}
int pfp_ri_device_ptrs(pfp_ctx *c, const void **d_cnt, const void **d_pos)
{
    if (!c) return PFP_E_ARG;
    const void **const out[2] = {d_cnt, d_pos};
    return family_device_ptrs(ri_family(c), out);
}
int pfp_ri_write(pfp_ctx *c, int fd_cnt, int fd_off, int fd_pos)
{
    if (!c) return PFP_E_ARG;
    if (!c->ri.p[0] || (fd_off >= 0 && !c->ri.p[1])) return PFP_E_STATE;
    const int fd[2] = {fd_cnt, fd_pos};
    PFP_TRY(family_write(c, ri_family(c), fd));
    return fd_off >= 0 ? write_all(fd_off, c->ri_off.data(), c->ri_off.size() * 8) : PFP_OK;
}

// ---- document listing (include/pfbwt_hip.h: pfp_ri_docs; csrc/doclist.h) ------------------------------------------------------------
static ResultFamily dl_family(const pfp_ctx *c) { return {3, {{c->dl.p[0], c->dl_patterns}, {c->dl.p[1], c->dl_entries}, {c->dl.p[2], c->dl_entries}}, false}; }
// scratch of a chunk per reported row (pos, dk, and on the sort route two keys, two values, flags, their sums, the heads) and per
// upper-bound slot (tdoc, tfreq); per pattern of the call
template <typename T> constexpr uint64_t dl_row_bytes() { return sizeof(T) + 4 + 16 + 8 + 12 + 8; }
constexpr uint64_t DL_PATTERN_BYTES = 96;
// the default of dl_chunk_values: what the workspace leaves free behind the results and the per-pattern scratch, over the cost of a
// row on the sort route (not measured: a guess that keeps a chunk inside the workspace)
template <typename T> static uint64_t dl_budget(const pfp_ctx *c, uint64_t np)
{
    uint64_t v = c->tun.dl_chunk_values;
    if (!v) {
        const uint64_t room = c->arena.hi > c->arena.lo ? c->arena.hi - c->arena.lo : 0, fixed = np * DL_PATTERN_BYTES + (1u << 20);
        v = room > fixed ? (room - fixed) / dl_row_bytes<T>() : 0;
    }
    if (v < 1) v = 1;
    return v < 0xFFFFFFF0ULL ? v : 0xFFFFFFF0ULL;
}
// what the chunks of one call share: interval, reported rows (cl; hc = their host copy: 0 for a skipped pattern) and toehold of every
// pattern, the record table, the results at their upper bound `cap`
template <typename T> struct DlCall {
    const T *lo, *cl, *top, *starts; const uint64_t *d_off; const std::vector<uint64_t> *hc;
    DocTable t; uint64_t ndocs; int route; unsigned flags; unsigned long long *d_out; T *doc, *freq; uint64_t cap;
};
// One chunk, the patterns [j0, j1): their positions into scratch, a document per position, the reduction of every pattern by its
// route, the pairs behind the e0 pairs of the chunks in front.  doc_off[j0 + 1 .. j1] and by[0 .. 3) (patterns per route) are filled in;
// the scratch is released, the stream has drained.
template <typename T> static int dl_chunk(pfp_ctx *c, const MsView<T> &ix, const DlCall<T> &a, uint64_t j0, uint64_t j1, uint64_t e0, std::vector<uint64_t> *doc_off, uint64_t by[3])
{
    const uint64_t npc = j1 - j0, ndocs = a.ndocs;
    const size_t mk = c->arena.mark_hi();
    // host: the route of every pattern, the wave list from the front and the table list from the back of one array, the upper-bound slices
    std::vector<uint8_t> proute((size_t)npc, 0);
    std::vector<uint32_t> list((size_t)npc, 0);
    std::vector<uint64_t> ub((size_t)npc + 1, 0), ooff((size_t)npc + 1, 0);
    uint64_t nwave = 0, ntable = 0, nsort = 0, rows = 0;
    const uint32_t wave_max = c->tun.dl_wave_max, table_max = c->tun.dl_table_max < DL_TABLE_CAP ? c->tun.dl_table_max : DL_TABLE_CAP;
    for (uint64_t q = 0; q < npc; ++q) {
        const uint64_t cq = (*a.hc)[(size_t)(j0 + q)];
        ub[(size_t)q + 1] = ub[(size_t)q] + (cq < ndocs ? cq : ndocs);
        rows += cq;
        if (!cq) continue;
        if (cq <= wave_max) { proute[(size_t)q] = 1; list[(size_t)nwave++] = (uint32_t)q; }
        else if (ndocs <= table_max && cq <= DL_TABLE_ROWS_MAX) { proute[(size_t)q] = 2; list[(size_t)(npc - 1 - ntable++)] = (uint32_t)q; }
        else { proute[(size_t)q] = 3; ++nsort; }
    }
    by[0] += nwave; by[1] += ntable; by[2] += nsort;
    const uint64_t slots = ub[(size_t)npc];
    if (!rows) { for (uint64_t q = 0; q < npc; ++q) (*doc_off)[(size_t)(j0 + q + 1)] = e0; return PFP_OK; }      // nothing to reduce
    if (nsort && rows >= 0xFFFFFFF0ULL) return PFP_E_TOO_LARGE;           // (heads are compacted as 32-bit indices)
    T *pos; const unsigned long long *obase; unsigned long long tot[2] = {0, 0};
    PFP_TRY(ri_report<T>(c, ix, a.lo + j0, a.cl + j0, a.top + j0, npc, a.route, 0, a.d_out, &pos, &ooff, tot, true, &obase));
    if (tot[1] != rows) return PFP_E_CORRUPT;                              // (the reported rows of a pattern are its count: cl <= n + 1)
    uint32_t *dk, *tdoc, *tfreq, *d_list; uint8_t *d_route; unsigned long long *d_ub, *ne;
    PFP_ALLOC_HI(c, dk, uint32_t, rows); PFP_ALLOC_HI(c, tdoc, uint32_t, slots); PFP_ALLOC_HI(c, tfreq, uint32_t, slots);
    PFP_ALLOC_HI(c, d_list, uint32_t, npc); PFP_ALLOC_HI(c, d_route, uint8_t, npc); PFP_ALLOC_HI(c, d_ub, unsigned long long, npc + 1); PFP_ALLOC_HI(c, ne, unsigned long long, npc + 1);
    PFP_TRY(h2d_copy(c, (uint8_t *)d_list, (const uint8_t *)list.data(), npc * 4));
    PFP_TRY(h2d_copy(c, d_route, proute.data(), npc));
    PFP_TRY(h2d_copy(c, (uint8_t *)d_ub, (const uint8_t *)ub.data(), (npc + 1) * 8));
    PFP_HIP(c, hipMemsetAsync(ne, 0, (size_t)(npc + 1) * 8, c->stream));
    // 1. the document of every position
    {
        const bool small = a.t.ntab <= DOC_LDS_SMALL;
        const uint64_t work = (rows + BLOCK - 1) / BLOCK, most = (uint64_t)STREAM_CUS * (small ? DOC_WG_PER_CU_SMALL : DOC_WG_PER_CU_BIG);
        const unsigned grid = (unsigned)(work < most ? work : most);
        const int inside = (a.flags & PFP_DL_INSIDE) != 0;
        if (small) PFP_LAUNCH(c, K_DL_MAP, rows * (sizeof(T) + 4), (k_dl_map<T, DOC_LDS_SMALL>), grid, (const T *)pos, rows, obase, npc, a.d_off + j0, a.starts, a.t.ndocs, a.t.shift, a.t.ntab, a.t.top, c->nout - 1, (uint32_t)c->w, inside, dk, a.d_out + DL_OUT);
        else PFP_LAUNCH(c, K_DL_MAP, rows * (sizeof(T) + 4), (k_dl_map<T, DOC_LDS_CAP>), grid, (const T *)pos, rows, obase, npc, a.d_off + j0, a.starts, a.t.ndocs, a.t.shift, a.t.ntab, a.t.top, c->nout - 1, (uint32_t)c->w, inside, dk, a.d_out + DL_OUT);
    }
    // 2. the reductions
    if (nwave) PFP_LAUNCH(c, K_DL_WAVE, nwave * 64 * 12, k_dl_wave, nblocks(nwave, BLOCK / WAVE), (const uint32_t *)dk, obase, (const unsigned long long *)d_ub, (const uint32_t *)d_list, nwave, a.t.ndocs, tdoc, tfreq, ne);
    if (ntable) {
        const uint32_t *tl = d_list + (npc - ntable);
        if (ndocs <= 1024) PFP_LAUNCH(c, K_DL_TABLE, rows * 4, (k_dl_table<1024>), ntable, (const uint32_t *)dk, obase, (const unsigned long long *)d_ub, tl, a.t.ndocs, tdoc, tfreq, ne);
        else if (ndocs <= 4096) PFP_LAUNCH(c, K_DL_TABLE, rows * 4, (k_dl_table<4096>), ntable, (const uint32_t *)dk, obase, (const unsigned long long *)d_ub, tl, a.t.ndocs, tdoc, tfreq, ne);
        else PFP_LAUNCH(c, K_DL_TABLE, rows * 4, (k_dl_table<DL_TABLE_CAP>), ntable, (const uint32_t *)dk, obase, (const unsigned long long *)d_ub, tl, a.t.ndocs, tdoc, tfreq, ne);
    }
    if (nsort) {
        uint64_t *k0, *k1, *sk; uint32_t *v0, *v1, *sv, *head, *hpos, *hl, *d_nh, *first, *last;
        PFP_ALLOC_HI(c, k0, uint64_t, rows); PFP_ALLOC_HI(c, k1, uint64_t, rows); PFP_ALLOC_HI(c, v0, uint32_t, rows); PFP_ALLOC_HI(c, v1, uint32_t, rows);
        PFP_ALLOC_HI(c, head, uint32_t, rows); PFP_ALLOC_HI(c, hpos, uint32_t, rows); PFP_ALLOC_HI(c, hl, uint32_t, rows); PFP_ALLOC_HI(c, d_nh, uint32_t, 1);
        PFP_ALLOC_HI(c, first, uint32_t, npc); PFP_ALLOC_HI(c, last, uint32_t, npc);
        const int dbits = bits_for(ndocs - 1);
        const BitRange range = {0, dbits + bits_for(npc)};
        PFP_LAUNCH(c, K_DL_SORT, rows * 16, k_dl_keys, nblocks(rows, BLOCK), (const uint32_t *)dk, rows, obase, npc, (const uint8_t *)d_route, a.t.ndocs, dbits, k0, v0);
        PFP_TRY((radix_sort_pairs<uint64_t>(c, k0, v0, k1, v1, rows, &range, 1, &sk, &sv)));
        PFP_LAUNCH(c, K_DL_SORT, rows * 12, k_dl_heads, nblocks(rows, BLOCK), (const uint64_t *)sk, rows, head);
        PFP_TRY(device_compact(c, nullptr, head, rows, hl, hpos, d_nh));
        uint32_t nh = 0; PFP_TRY(d2h_u32(c, d_nh, &nh));
        PFP_HIP(c, hipMemsetAsync(first, 0, (size_t)npc * 4, c->stream)); PFP_HIP(c, hipMemsetAsync(last, 0, (size_t)npc * 4, c->stream));
        PFP_LAUNCH(c, K_DL_SORT, (uint64_t)nh * 16, k_dl_spans, nblocks(nh, BLOCK), (const uint64_t *)sk, (const uint32_t *)hl, (uint64_t)nh, rows, npc, dbits, first, last);
        PFP_LAUNCH(c, K_DL_SORT, (uint64_t)nh * 24, k_dl_emit, nblocks(nh, BLOCK), (const uint64_t *)sk, (const uint32_t *)hl, (uint64_t)nh, rows, npc, dbits, a.t.ndocs, (const uint32_t *)first, (const uint32_t *)last,
                   (const unsigned long long *)d_ub, tdoc, tfreq, ne);
    }
    // 3. tight, in pattern order, behind the e0 pairs of the chunks in front
    PFP_TRY((device_scan<unsigned long long, 0>(c, ne, ne, npc, ne + npc)));
    if (slots) PFP_LAUNCH(c, K_DL_PACK, slots * (8 + 2 * sizeof(T)), (k_dl_pack<T>), nblocks(slots, BLOCK), (const uint32_t *)tdoc, (const uint32_t *)tfreq, (const unsigned long long *)d_ub, (const unsigned long long *)ne, npc, slots, e0, a.cap, a.doc, a.freq);
    PFP_HIP(c, hipMemcpyAsync(ooff.data(), ne, (size_t)(npc + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    for (uint64_t q = 0; q < npc; ++q) (*doc_off)[(size_t)(j0 + q + 1)] = e0 + ooff[(size_t)q + 1];
    if (e0 + ooff[(size_t)npc] > a.cap) return PFP_E_CORRUPT;
    c->arena.release_hi(mk);
    return PFP_OK;
}
template <typename T> static int ri_docs_impl(pfp_ctx *c, const uint8_t *bases, const uint64_t *offsets, uint64_t np, const uint64_t *starts, uint64_t ndocs, unsigned flags, uint64_t max_count, int route, pfp_dl_info *info)
{
    PatternBatch pb(bases, offsets, np);
    const uint64_t total = pb.total;
    std::vector<T> hs((size_t)ndocs);
    for (uint64_t k = 0; k < ndocs; ++k) hs[(size_t)k] = (T)starts[k];
    DocTable t;
    t.ndocs = (uint32_t)ndocs; t.shift = 0;
    const uint32_t lds = c->tun.doc_lds_max < DOC_LDS_CAP ? c->tun.doc_lds_max : DOC_LDS_CAP;
    while (((ndocs - 1) >> t.shift) + 1 > lds) ++t.shift;                   // two-level: every 2^shift-th start in LDS
    t.ntab = (uint32_t)(((ndocs - 1) >> t.shift) + 1);
    t.top = 1; while (2 * t.top < t.ntab) t.top *= 2;
    PostResult res(c, c->dl);
    c->dl_patterns = c->dl_entries = 0; c->dl_off.clear();
    T *cnt;
    PFP_ALLOC_LO(c, cnt, T, np);
    const size_t mk = c->arena.mark_hi();
    T *lo, *top, *cl, *d_starts; unsigned long long *d_out;
    PFP_TRY(pb.upload(c, K_RI_SEARCH));
    PFP_ALLOC_HI(c, lo, T, np); PFP_ALLOC_HI(c, top, T, np); PFP_ALLOC_HI(c, cl, T, np); PFP_ALLOC_HI(c, d_starts, T, ndocs);
    PFP_ALLOC_HI(c, d_out, unsigned long long, DL_OUT + OUT_BLOCK);        // RiOut of the search and the walk, DlOut of k_dl_map
    PFP_HIP(c, hipMemsetAsync(d_out, 0, sizeof(unsigned long long) * (DL_OUT + OUT_BLOCK), c->stream));
    PFP_TRY(h2d_copy(c, (uint8_t *)d_starts, (const uint8_t *)hs.data(), ndocs * sizeof(T)));
    const MsView<T> ix = ri_view<T>(c);
    std::vector<T> hcnt((size_t)np);
    if (np) {
        PFP_LAUNCH(c, K_RI_SEARCH, total + np * 3 * sizeof(T), (k_ri_search<T, true>), nblocks(np, BLOCK), ix, (const uint8_t *)pb.P, (const uint64_t *)pb.d_off, (const uint32_t *)pb.d_order, np, lo, cnt, top, d_out);
        PFP_HIP(c, hipMemcpyAsync(hcnt.data(), cnt, (size_t)np * sizeof(T), hipMemcpyDeviceToHost, c->stream));
        PFP_HIP(c, hipStreamSynchronize(c->stream));
    }
    // host: the rows every pattern reports (0 for a skipped one), the upper bound of the pairs
    std::vector<uint64_t> hc((size_t)np), doc_off((size_t)np + 1, 0);
    uint64_t skipped = 0, cap = 0;
    for (uint64_t j = 0; j < np; ++j) {
        const uint64_t cj = hcnt[(size_t)j];
        const bool skip = max_count && cj > max_count;
        skipped += skip;
        hc[(size_t)j] = skip ? 0 : cj;
        hcnt[(size_t)j] = (T)hc[(size_t)j];
        cap += hc[(size_t)j] < ndocs ? hc[(size_t)j] : ndocs;
    }
    if (np) PFP_TRY(h2d_copy(c, (uint8_t *)cl, (const uint8_t *)hcnt.data(), np * sizeof(T)));
    T *doc, *freq;
    PFP_ALLOC_LO(c, doc, T, cap); PFP_ALLOC_LO(c, freq, T, cap);
    const uint64_t budget = dl_budget<T>(c, np);
    const DlCall<T> call = {lo, cl, top, d_starts, pb.d_off, &hc, t, ndocs, route, flags, d_out, doc, freq, cap};
    uint64_t chunks = 0, e0 = 0, by[3] = {0, 0, 0};
    for (uint64_t j0 = 0; j0 < np;) {                                      // a chunk: patterns in order while their rows fit the budget, one at least
        uint64_t j1 = j0, rows = 0;
        while (j1 < np && (j1 == j0 || rows + hc[(size_t)j1] <= budget)) rows += hc[(size_t)j1++];
        PFP_TRY(dl_chunk<T>(c, ix, call, j0, j1, e0, &doc_off, by));
        e0 = doc_off[(size_t)j1];
        ++chunks; j0 = j1;
    }
    unsigned long long h[DL_OUT + OUT_BLOCK];
    PFP_HIP(c, hipMemcpyAsync(h, d_out, sizeof h, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    c->arena.release_hi(mk);
    // freq moves down behind the e0 pairs of doc, through a bounce buffer (source and destination may overlap), and the tail is free again
    const size_t doc_at = c->arena.offset_of(doc), freq_at = (doc_at + (size_t)(e0 ? e0 : 1) * sizeof(T) + 255) & ~(size_t)255;
    T *freq_final = (T *)(c->arena.base + freq_at);
    if (freq_final != freq && e0) {
        size_t bytes = (size_t)e0 * sizeof(T), piece = bytes < ((size_t)64 << 20) ? bytes : ((size_t)64 << 20);
        const size_t want0 = c->arena.want;
        uint8_t *bounce;
        while (!(bounce = (uint8_t *)c->arena.alloc_hi(piece))) {
            if (piece <= 4096) return PFP_E_NOMEM;
            piece /= 2; c->arena.failed = false; c->arena.want = want0;
        }
        for (size_t at = 0; at < bytes; at += piece) {
            const size_t len = bytes - at < piece ? bytes - at : piece;
            PFP_HIP(c, hipMemcpyAsync(bounce, (const uint8_t *)freq + at, len, hipMemcpyDeviceToDevice, c->stream));
            PFP_HIP(c, hipMemcpyAsync((uint8_t *)freq_final + at, bounce, len, hipMemcpyDeviceToDevice, c->stream));
        }
        PFP_HIP(c, hipStreamSynchronize(c->stream));
        c->arena.release_hi(mk);
    }
    c->arena.release_lo(freq_at + (size_t)(e0 ? e0 : 1) * sizeof(T));
    res.commit(cnt, doc, freq_final);
    uint64_t listed = 0, max_docs = 0;
    for (uint64_t j = 0; j < np; ++j) { const uint64_t d = doc_off[(size_t)j + 1] - doc_off[(size_t)j]; listed += d != 0; if (d > max_docs) max_docs = d; }
    c->dl_patterns = np; c->dl_entries = e0; c->dl_off.swap(doc_off);
    if (c->tun.verbose) fprintf(stderr, "[pfbwt_hip] ri docs: %llu patterns, %llu chunks, %llu pairs of at most %llu\n", (unsigned long long)np, (unsigned long long)chunks, (unsigned long long)e0, (unsigned long long)cap);
    if (info) {
        info->patterns = np; info->bases = total; info->found = h[RI_FOUND]; info->occurrences = h[RI_OCCURRENCES]; info->listed = listed; info->skipped = skipped; info->outside = h[DL_OUT + DL_OUTSIDE]; info->entries = e0;
        info->max_docs = max_docs; info->chunks = chunks; info->by_wave = by[0]; info->by_table = by[1]; info->by_sort = by[2]; info->route = (uint64_t)route;
    }
    return PFP_OK;
}
int pfp_ri_docs(pfp_ctx *c, const uint8_t *bases, const uint64_t *offsets, uint64_t npatterns, const uint64_t *starts, uint64_t ndocs, unsigned flags, uint64_t max_count, pfp_dl_info *info)
{
    if (!c || !bases || !offsets || !starts || !ndocs || (flags & ~(unsigned)PFP_DL_INSIDE)) return PFP_E_ARG;
    if (!has_ri_index(c) || ri_state(c) != PFP_OK) return PFP_E_STATE;
    if (ndocs > 0xFFFFFFFFULL) return PFP_E_TOO_LARGE;
    PFP_TRY(pattern_args_check(c, bases, offsets, npatterns));
    if (starts[0] != 0) return PFP_E_ARG;
    for (uint64_t k = 1; k < ndocs; ++k) if (starts[k] <= starts[k - 1]) return PFP_E_ARG;
    if (starts[ndocs - 1] >= c->nout - 1) return PFP_E_ARG;
    const int route = ri_locate_route(c);
    if (!route) return PFP_E_STATE;
    return post_entry(c, [&](auto t) { return ri_docs_impl<decltype(t)>(c, bases, offsets, npatterns, starts, ndocs, flags, max_count, route, info); });
}
int pfp_ri_docs_file(pfp_ctx *c, const char *path, const uint64_t *starts, uint64_t ndocs, unsigned flags, uint64_t max_count, pfp_dl_info *info)
{
    if (!c || !path || !starts) return PFP_E_ARG;
    if (!has_ri_index(c)) return PFP_E_STATE;
    return pattern_file_query(path, [&](const uint8_t *bases, const uint64_t *off, uint64_t np) { return pfp_ri_docs(c, bases, off, np, starts, ndocs, flags, max_count, info); });
}
int pfp_ri_docs_offsets_get(pfp_ctx *c, uint64_t *doc_off, uint64_t *npatterns)
{
    if (!c) return PFP_E_ARG;
    return offsets_get(c->dl.p[0] && c->dl_off.size() == c->dl_patterns + 1, c->dl_off, doc_off, npatterns);
}
int pfp_ri_docs_get(pfp_ctx *c, void *cnt, void *doc, void *freq)
{
    if (!c) return PFP_E_ARG;
    if (!c->dl.p[0]) return PFP_E_STATE;
    void *const dst[3] = {cnt, doc, freq};
    return family_get(c, dl_family(c), dst);
}
int pfp_ri_docs_device_ptrs(pfp_ctx *c, const void **d_cnt, const void **d_doc, const void **d_freq)
{
    if (!c) return PFP_E_ARG;
    const void **const out[3] = {d_cnt, d_doc, d_freq};
    return family_device_ptrs(dl_family(c), out);
}
int pfp_ri_docs_write(pfp_ctx *c, int fd_cnt, int fd_off, int fd_doc, int fd_freq)
{
    if (!c) return PFP_E_ARG;
    if (!c->dl.p[0]) return PFP_E_STATE;
    const int fd[3] = {fd_cnt, fd_doc, fd_freq};
    PFP_TRY(family_write(c, dl_family(c), fd));
    return fd_off >= 0 ? write_all(fd_off, c->dl_off.data(), c->dl_off.size() * 8) : PFP_OK;
}

// ---- maximal exact matches (include/pfbwt_hip.h: pfp_mem_find; csrc/mems.h) --------------------------------------------------------
static ResultFamily mem_family(const pfp_ctx *c) { return {3, {{c->mem.p[0], c->mem_count}, {c->mem.p[1], c->mem_count}, {c->mem.p[2], c->mem_count}}, true}; }
static ResultFamily meml_family(const pfp_ctx *c) { return {2, {{c->meml.p[0], c->mem_count}, {c->meml.p[1], c->mem_reported}, {nullptr, 0}}, false}; }
static bool has_ms_result(const pfp_ctx *c) { return c->ms.p[0] && c->ms.p[1] && c->ms_off.size() == c->ms_patterns + 1; }
// route: 0 no locate, 1 phi, 2 the resident SA
template <typename T> static int mem_find_impl(pfp_ctx *c, uint64_t min_len, int route, uint64_t max_occ, pfp_mem_info *info)
{
    const uint64_t np = c->ms_patterns, total = c->ms_bases, n = c->n, L = min_len ? min_len : 1;
    const T *mptr = (const T *)c->ms.p[0], *mlen = (const T *)c->ms.p[1];
    uint64_t longest = 1;                                                  // no MEM is longer than its pattern
    for (uint64_t j = 0; j < np; ++j) if (c->ms_off[(size_t)j + 1] - c->ms_off[(size_t)j] > longest) longest = c->ms_off[(size_t)j + 1] - c->ms_off[(size_t)j];
    // the result of an earlier call gives its space back first, the occurrences (on top) before the MEMs
    { PostResult drop(c, c->meml); }
    PostResult res(c, c->mem);
    c->mem_patterns = c->mem_count = c->mem_reported = 0; c->mem_off.clear(); c->mem_poff.clear();
    const size_t mk = c->arena.mark_hi();
    uint64_t *d_off; T *fl, *d_cnt; unsigned long long *d_moff, *d_out;
    PFP_ALLOC_HI(c, d_off, uint64_t, np + 1); PFP_ALLOC_HI(c, d_moff, unsigned long long, np + 1); PFP_ALLOC_HI(c, fl, T, total); PFP_ALLOC_HI(c, d_cnt, T, 1);
    PFP_ALLOC_HI(c, d_out, unsigned long long, MEM_OUT + OUT_BLOCK);       // RiOut of the search and the walk, MemOut of k_mem_list
    PFP_HIP(c, hipMemsetAsync(d_out, 0, sizeof(unsigned long long) * (MEM_OUT + OUT_BLOCK), c->stream));
    PFP_TRY(h2d_copy(c, (uint8_t *)d_off, (const uint8_t *)c->ms_off.data(), (np + 1) * 8));
    if (total) PFP_LAUNCH(c, K_MEM_LIST, total * 2 * sizeof(T), (k_mem_flags<T>), nblocks(total, BLOCK), mlen, total, L, fl);
    PFP_TRY((device_scan<T, 0>(c, fl, fl, total, d_cnt)));
    T cnt_t = 0;
    PFP_HIP(c, hipMemcpyAsync(&cnt_t, d_cnt, sizeof(T), hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    const uint64_t mems = cnt_t;
    if (mems > 0xFFFFFFFFULL) return PFP_E_TOO_LARGE;                      // (MEM indices are 32-bit values in the order array; only U = 8 gets here:
                                                                           //  with U = 4 pfp_ms_query has refused more than 0xFFFFFFF0 bases, so the T-wide sum cannot wrap)
    T *start, *len, *ptr, *cnt = nullptr, *pos = nullptr;
    PFP_ALLOC_LO(c, start, T, mems); PFP_ALLOC_LO(c, len, T, mems); PFP_ALLOC_LO(c, ptr, T, mems);
    std::vector<uint64_t> moff((size_t)np + 1, 0), poff;
    PFP_LAUNCH(c, K_MEM_LIST, (np + 1) * (16 + sizeof(T)), (k_mem_offsets<T>), nblocks(np + 1, BLOCK), (const T *)fl, (const uint64_t *)d_off, np, total, mems, d_moff);
    if (total) PFP_LAUNCH(c, K_MEM_LIST, total * 3 * sizeof(T) + mems * (8 + 4 * sizeof(T)), (k_mem_list<T>), (nblocks(total, BLOCK) < (unsigned)MEM_LIST_WG ? nblocks(total, BLOCK) : (unsigned)MEM_LIST_WG), mlen, mptr, (const T *)fl, (const uint64_t *)d_off, np, total, L, mems, start, len, ptr, d_out + MEM_OUT);
    PFP_HIP(c, hipMemcpyAsync(moff.data(), d_moff, (size_t)(np + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    unsigned long long h[MEM_OUT + OUT_BLOCK] = {}, tot[2] = {0, 0};
    PostResult resl(c, c->meml);                                           // (after the MEMs: its mark is their end)
    if (route) {
        PFP_ALLOC_LO(c, cnt, T, mems);
        poff.assign((size_t)mems + 1, 0);
        const MsView<T> ix = ri_view<T>(c);
        T *lo, *top, *k0, *k1, *sk; uint32_t *v0, *v1, *sv;
        PFP_ALLOC_HI(c, lo, T, mems); PFP_ALLOC_HI(c, top, T, mems);
        PFP_ALLOC_HI(c, k0, T, mems); PFP_ALLOC_HI(c, k1, T, mems); PFP_ALLOC_HI(c, v0, uint32_t, mems); PFP_ALLOC_HI(c, v1, uint32_t, mems);
        if (mems) {
            // the MEMs in order of decreasing length, so that the lanes of a wave finish together
            PFP_LAUNCH(c, K_MEM_SEARCH, mems * (2 * sizeof(T) + 4), (k_mem_keys<T>), nblocks(mems, BLOCK), (const T *)len, mems, longest, k0, v0);
            const BitRange range = {0, bits_for(longest)};
            PFP_TRY((radix_sort_pairs<T>(c, k0, v0, k1, v1, mems, &range, 1, &sk, &sv)));
            const MemText<T> src = {(const uint8_t *)c->tb + 16, (const T *)ptr, (const T *)len, n};
            PFP_LAUNCH(c, K_MEM_SEARCH, mems * 5 * sizeof(T), (k_mem_search<T>), nblocks(mems, BLOCK), ix, src, (const uint32_t *)sv, mems, lo, cnt, top, d_out);
        }
        PFP_TRY(ri_report<T>(c, ix, lo, cnt, top, mems, route, max_occ, d_out, &pos, &poff, tot));
    }
    PFP_HIP(c, hipMemcpyAsync(h, d_out, sizeof h, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    c->arena.release_hi(mk);
    res.commit_under(resl, start, len, ptr);                               // (ends at ptr's end, whatever the locate put behind it)
    if (route) resl.commit(cnt, pos);
    c->mem_patterns = np; c->mem_count = mems; c->mem_reported = tot[1]; c->mem_off.swap(moff); c->mem_poff.swap(poff);
    if (c->tun.verbose) fprintf(stderr, "[pfbwt_hip] mem find: %llu patterns, %llu MEMs, %llu steps, %llu pieces\n", (unsigned long long)np, (unsigned long long)mems, h[RI_STEPS], tot[0]);
    if (info) {
        info->patterns = np; info->bases = total; info->mems = mems; info->max_len = h[MEM_OUT + MEM_MAX_LEN]; info->sum_len = h[MEM_OUT + MEM_SUM_LEN];
        info->occurrences = h[RI_OCCURRENCES]; info->reported = tot[1]; info->pieces = tot[0]; info->max_count = h[RI_MAX_COUNT]; info->max_piece = h[RI_MAX_PIECE]; info->phi_steps = h[RI_PHI_STEPS]; info->route = (uint64_t)route;
    }
    return PFP_OK;
}
int pfp_mem_find(pfp_ctx *c, uint64_t min_len, int locate, uint64_t max_occ, pfp_mem_info *info)
{
    if (!c) return PFP_E_ARG;
    if (!has_build(c) || !holds_build_text(c) || !has_ms_result(c)) return PFP_E_STATE;
    int route = 0;
    if (locate) {
        if (!has_ri_index(c) || ri_state(c) != PFP_OK) return PFP_E_STATE;
        if (!(route = ri_locate_route(c))) return PFP_E_STATE;
    }
    return post_entry(c, [&](auto t) { return mem_find_impl<decltype(t)>(c, min_len, route, max_occ, info); });
}
int pfp_mem_offsets_get(pfp_ctx *c, uint64_t *mem_off, uint64_t *npatterns, uint64_t *pos_off, uint64_t *mems)
{
    if (!c) return PFP_E_ARG;
    if (pos_off && (!c->meml.p[0] || c->mem_poff.size() != c->mem_count + 1)) return PFP_E_STATE;      // found without locate
    PFP_TRY(offsets_get(c->mem.p[0] && c->mem_off.size() == c->mem_patterns + 1, c->mem_off, mem_off, npatterns));
    if (mems) *mems = c->mem_count;
    return offsets_get(true, c->mem_poff, pos_off, nullptr);                                    // (nothing without pos_off)
}
int pfp_mem_get(pfp_ctx *c, void *start, void *len, void *ptr, void *cnt, void *pos)
{
    if (!c) return PFP_E_ARG;
    void *const a[3] = {start, len, ptr}, *const b[2] = {cnt, pos};
    PFP_TRY(family_state(mem_family(c), nullptr));                                              // (a whole family: nothing is asked of `asked`)
    const bool asked[3] = {cnt != nullptr, pos != nullptr, false};
    PFP_TRY(family_state(meml_family(c), asked));
    PFP_TRY(family_get(c, mem_family(c), a));
    return family_get(c, meml_family(c), b);
}
int pfp_mem_device_ptrs(pfp_ctx *c, const void **d_start, const void **d_len, const void **d_ptr, const void **d_cnt, const void **d_pos)
{
    if (!c) return PFP_E_ARG;
    const void **const a[3] = {d_start, d_len, d_ptr}, **const b[2] = {d_cnt, d_pos};
    family_device_ptrs(mem_family(c), a);
    return family_device_ptrs(meml_family(c), b);
}
int pfp_mem_write(pfp_ctx *c, int fd_start, int fd_len, int fd_ptr, int fd_cnt, int fd_pos)
{
    if (!c) return PFP_E_ARG;
    const int a[3] = {fd_start, fd_len, fd_ptr}, b[2] = {fd_cnt, fd_pos};
    PFP_TRY(family_state(mem_family(c), nullptr));
    const bool asked[3] = {fd_cnt >= 0, fd_pos >= 0, false};
    PFP_TRY(family_state(meml_family(c), asked));                                               // (before anything is written)
    PFP_TRY(family_write(c, mem_family(c), a));
    return family_write(c, meml_family(c), b);
}

// ---- marker index and queries (include/pfbwt_hip.h: pfp_mk_index, pfp_mk_query; csrc/markerquery.h) ---------------------------------
// marker / freq are 64-bit values whatever U is: their counts in U-wide values for the one fetch path
static uint64_t mk_wide(const pfp_ctx *c, uint64_t values) { return (c->flags & PFP_FLAG_U64) ? values : 2 * values; }
static ResultFamily mk_family(const pfp_ctx *c) { return {2, {{c->mk.p[0], c->mk_patterns}, {c->mk.p[1], c->mk_patterns}, {nullptr, 0}}, true}; }
static ResultFamily mkl_family(const pfp_ctx *c) { return {2, {{c->mkl.p[0], mk_wide(c, c->mk_entries)}, {c->mkl.p[1], mk_wide(c, c->mk_entries)}, {nullptr, 0}}, true}; }
static bool has_mk_index(const pfp_ctx *c) { return c->mki.p[0] && c->mkx.loff; }
static bool has_mk_result(const pfp_ctx *c) { return c->mk.p[0] && c->mkl.p[0] && c->mk_off.size() == c->mk_patterns + 1; }
static void mk_index_drop(pfp_ctx *c) { c->mki = ResultSlot(); c->mkx = MkIndex(); }
static MkView mk_view(const pfp_ctx *c) { const MkIndex &x = c->mkx; return {x.first, x.last, x.loff, x.lid, x.nrec, x.entries, x.distinct}; }
// the stream: `words` words in host memory, or (ma == nullptr) on the device at d_src
static int mk_index_impl(pfp_ctx *c, const uint64_t *ma, const uint64_t *d_src, uint64_t words, pfp_mk_index_info *info)
{
    const uint64_t n = c->nout - 1;
    PostResult res(c, c->mki);
    c->mkx = MkIndex();
    MkIndex x;
    const size_t mk = c->arena.mark_hi();
    unsigned long long *d_out, h[OUT_BLOCK] = {};
    PFP_ALLOC_HI(c, d_out, unsigned long long, OUT_BLOCK);
    PFP_HIP(c, hipMemsetAsync(d_out, 0, sizeof(unsigned long long) * OUT_BLOCK, c->stream));
    if (words >= 0xFFFFFFF0ULL) return PFP_E_TOO_LARGE;                    // (record starts are compacted as 32-bit word indices)
    if (ma && words) {
        uint64_t *up; PFP_ALLOC_HI(c, up, uint64_t, words);
        PFP_TRY(h2d_copy(c, (uint8_t *)up, (const uint8_t *)ma, words * 8));
        d_src = up;
    }
    // 1. the records
    uint32_t *flag, *fpos, *rstart, *d_n32;
    PFP_ALLOC_HI(c, flag, uint32_t, words); PFP_ALLOC_HI(c, fpos, uint32_t, words); PFP_ALLOC_HI(c, rstart, uint32_t, words / 4 + 1); PFP_ALLOC_HI(c, d_n32, uint32_t, 2);
    uint32_t nrec32 = 0;
    if (words) {
        PFP_LAUNCH(c, K_MK_INDEX, words * 12, k_mk_flags, nblocks(words, BLOCK), d_src, words, flag);
        PFP_TRY((device_scan<uint32_t, 0>(c, flag, fpos, words, d_n32)));
        PFP_TRY(d2h_u32(c, d_n32, &nrec32));
        if ((uint64_t)nrec32 > words / 4 + 1) return PFP_E_CORRUPT;        // records of fewer than four words: some have no marker
        PFP_LAUNCH(c, K_COMPACT, words * 12, k_compact_scatter, nblocks(words, BLOCK), (const uint32_t *)nullptr, (const uint32_t *)flag, (const uint32_t *)fpos, words, rstart);
    }
    const uint64_t nrec = nrec32;
    PFP_ALLOC_LO(c, x.first, uint64_t, nrec); PFP_ALLOC_LO(c, x.last, uint64_t, nrec); PFP_ALLOC_LO(c, x.loff, uint32_t, nrec + 1);
    unsigned long long *rawoff;
    PFP_ALLOC_HI(c, rawoff, unsigned long long, nrec + 1);
    uint64_t raw = 0, distinct = 0, entries = 0;
    if (nrec) {
        PFP_LAUNCH(c, K_MK_INDEX, nrec * 60, k_mk_records, nblocks(nrec, BLOCK), d_src, words, (const uint32_t *)rstart, nrec, n, x.first, x.last, rawoff, d_out);
        PFP_TRY((device_scan<unsigned long long, 0>(c, rawoff, rawoff, nrec, rawoff + nrec)));
        PFP_HIP(c, hipMemcpyAsync(&raw, rawoff + nrec, 8, hipMemcpyDeviceToHost, c->stream));
        PFP_HIP(c, hipMemcpyAsync(h, d_out, sizeof h, hipMemcpyDeviceToHost, c->stream));
        PFP_HIP(c, hipStreamSynchronize(c->stream));
        if (h[MKI_BAD]) return PFP_E_CORRUPT;
        if (raw >= 0xFFFFFFF0ULL) return PFP_E_TOO_LARGE;                  // (list entries are sorted with 32-bit values)
        // 2. dense ids in ascending value order
        uint64_t *k0, *k1, *sk; uint32_t *v0, *v1, *sv, *rec, *eid, *head, *hpos;
        PFP_ALLOC_HI(c, k0, uint64_t, raw); PFP_ALLOC_HI(c, k1, uint64_t, raw); PFP_ALLOC_HI(c, v0, uint32_t, raw); PFP_ALLOC_HI(c, v1, uint32_t, raw);
        PFP_ALLOC_HI(c, rec, uint32_t, raw); PFP_ALLOC_HI(c, eid, uint32_t, raw); PFP_ALLOC_HI(c, head, uint32_t, raw); PFP_ALLOC_HI(c, hpos, uint32_t, raw);
        PFP_LAUNCH(c, K_MK_INDEX, raw * 32, k_mk_values, nblocks(raw, BLOCK), d_src, words, (const uint32_t *)rstart, (const unsigned long long *)rawoff, nrec, raw, k0, v0, rec);
        const BitRange all = {0, 64};
        PFP_TRY((radix_sort_pairs<uint64_t>(c, k0, v0, k1, v1, raw, &all, 1, &sk, &sv)));
        PFP_LAUNCH(c, K_MK_INDEX, raw * 12, k_dl_heads, nblocks(raw, BLOCK), (const uint64_t *)sk, raw, head);
        PFP_TRY((device_scan<uint32_t, 0>(c, head, hpos, raw, d_n32)));
        uint32_t nd = 0; PFP_TRY(d2h_u32(c, d_n32, &nd));
        distinct = nd;
        PFP_ALLOC_LO(c, x.mval, uint64_t, distinct);
        PFP_LAUNCH(c, K_MK_INDEX, raw * 24, k_mk_ids, nblocks(raw, BLOCK), (const uint64_t *)sk, (const uint32_t *)sv, (const uint32_t *)head, (const uint32_t *)hpos, raw, distinct, x.mval, eid);
        // 3. the lists: (record, id) pairs sorted, heads only
        PFP_LAUNCH(c, K_MK_INDEX, raw * 20, k_mk_pairs, nblocks(raw, BLOCK), (const uint32_t *)rec, (const uint32_t *)eid, raw, k0, v0);      // (the sorted values are used up)
        const BitRange two[2] = {{0, bits_for(distinct - 1)}, {32, 32 + bits_for(nrec - 1)}};
        PFP_TRY((radix_sort_pairs<uint64_t>(c, k0, v0, k1, v1, raw, two, 2, &sk, &sv)));
        PFP_LAUNCH(c, K_MK_INDEX, raw * 12, k_dl_heads, nblocks(raw, BLOCK), (const uint64_t *)sk, raw, head);
        PFP_TRY((device_scan<uint32_t, 0>(c, head, hpos, raw, d_n32)));
        uint32_t ne = 0; PFP_TRY(d2h_u32(c, d_n32, &ne));
        entries = ne;
        PFP_ALLOC_LO(c, x.lid, uint32_t, entries);
        PFP_LAUNCH(c, K_MK_INDEX, raw * 16, k_mk_lists, nblocks(raw, BLOCK), (const uint64_t *)sk, (const uint32_t *)head, (const uint32_t *)hpos, raw, entries, x.lid);
        PFP_LAUNCH(c, K_MK_INDEX, nrec * 12, k_mk_loff, nblocks(nrec, BLOCK), (const uint64_t *)sk, (const uint32_t *)hpos, raw, nrec, entries, x.loff, d_out);
        PFP_HIP(c, hipMemcpyAsync(h, d_out, sizeof h, hipMemcpyDeviceToHost, c->stream));
    } else {
        PFP_ALLOC_LO(c, x.mval, uint64_t, 0); PFP_ALLOC_LO(c, x.lid, uint32_t, 0);
        PFP_HIP(c, hipMemsetAsync(x.loff, 0, 4, c->stream));
    }
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    c->arena.release_hi(mk);
    x.nrec = nrec; x.entries = entries; x.distinct = distinct;
    res.commit(x.first);
    c->mkx = x;
    if (info) { info->records = nrec; info->entries = entries; info->distinct = distinct; info->max_list = h[MKI_MAX_LIST]; info->rows = h[MKI_ROWS]; }
    return PFP_OK;
}
int pfp_mk_index(pfp_ctx *c, const uint64_t *ma, uint64_t ma_words, pfp_mk_index_info *info)
{
    if (!c) return PFP_E_ARG;
    int rc = PFP_OK;
    if (!ma && ma_words) rc = PFP_E_ARG;
    else if (!has_build(c) || c->slice_rows != c->nout || c->slice_begin) rc = PFP_E_STATE;     // no build, or a slice
    else if (!ma && (!c->ma.p[0] || !c->ma_words)) rc = PFP_E_STATE;                             // no marker array on the device
    else rc = post_entry(c, [&](auto) { return mk_index_impl(c, ma, (const uint64_t *)c->ma.p[0], ma ? ma_words : c->ma_words, info); });
    if (rc != PFP_OK) mk_index_drop(c);
    return rc;
}

// scratch of a chunk per raw entry (two keys, two values, the weight, and on the sort route flags and their sums) and per slot of
// the upper bound (id, frequency, counted as one more per entry)
constexpr uint64_t MK_ENTRY_BYTES = 16 + 8 + 8 + 12 + 12 + 8, MK_PATTERN_BYTES = 64;
// the default of mk_chunk_entries: what the workspace leaves free behind the results and the per-pattern scratch, over the cost of
// a raw entry (not measured: a guess that keeps a chunk inside the workspace)
static uint64_t mk_budget(const pfp_ctx *c, uint64_t np)
{
    uint64_t v = c->tun.mk_chunk_entries;
    if (!v) {
        const uint64_t room = c->arena.hi > c->arena.lo ? c->arena.hi - c->arena.lo : 0, fixed = np * MK_PATTERN_BYTES + (1u << 20);
        v = room > fixed ? (room - fixed) / MK_ENTRY_BYTES : 0;
    }
    if (v < 1) v = 1;
    return v < 0xFFFFFFF0ULL ? v : 0xFFFFFFEFULL;
}
// what the chunks of one call share
template <typename T> struct MkCall {
    MkView mv; const uint64_t *mval; const T *slo, *scnt; const uint32_t *ka; const unsigned long long *rbase; const std::vector<uint64_t> *off, *praw;
    uint64_t *marker, *freq; uint64_t cap;
};
// One chunk, the patterns [j0, j1): their raw entries, the reduction of every pattern by its route, the pairs behind the e0 pairs of
// the chunks in front.  mk_off[j0 + 1 .. j1] and by[0 .. 2) (patterns per route) are filled in; the scratch is released, the stream
// has drained.
template <typename T> static int mk_chunk(pfp_ctx *c, const MkCall<T> &a, uint64_t j0, uint64_t j1, uint64_t e0, std::vector<uint64_t> *mk_off, uint64_t by[2])
{
    const uint64_t npc = j1 - j0, s0 = (*a.off)[(size_t)j0], nslots = (*a.off)[(size_t)j1] - s0, distinct = a.mv.distinct;
    const size_t mk = c->arena.mark_hi();
    std::vector<uint8_t> proute((size_t)npc, 0);
    std::vector<uint32_t> list((size_t)npc, 0);
    std::vector<uint64_t> ub((size_t)npc + 1, 0), pbase((size_t)npc + 1, 0), ooff((size_t)npc + 1, 0);
    uint64_t nwave = 0, nsort = 0;
    const uint32_t wave_max = c->tun.mk_wave_max < MK_WAVE_MAX ? c->tun.mk_wave_max : MK_WAVE_MAX;
    for (uint64_t q = 0; q < npc; ++q) {
        const uint64_t rq = (*a.praw)[(size_t)(j0 + q)];
        pbase[(size_t)q + 1] = pbase[(size_t)q] + rq;
        ub[(size_t)q + 1] = ub[(size_t)q] + (rq < distinct ? rq : distinct);
        if (!rq) continue;
        if (rq <= wave_max) { proute[(size_t)q] = 1; list[(size_t)nwave++] = (uint32_t)q; }
        else { proute[(size_t)q] = 2; ++nsort; }
    }
    by[0] += nwave; by[1] += nsort;
    const uint64_t raw = pbase[(size_t)npc], slots = ub[(size_t)npc];
    if (!raw) { for (uint64_t q = 0; q < npc; ++q) (*mk_off)[(size_t)(j0 + q + 1)] = e0; return PFP_OK; }      // nothing to reduce
    if (raw >= 0xFFFFFFF0ULL) return PFP_E_TOO_LARGE;                      // (entries are sorted with 32-bit values, heads compacted as 32-bit indices)
    uint64_t *k0, *k1, *sk; uint32_t *v0, *v1, *sv, *tid, *d_list; uint8_t *d_route; unsigned long long *wt, *tfreq, *d_ub, *d_pbase, *ne;
    PFP_ALLOC_HI(c, k0, uint64_t, raw); PFP_ALLOC_HI(c, v0, uint32_t, raw); PFP_ALLOC_HI(c, wt, unsigned long long, raw);
    PFP_ALLOC_HI(c, tid, uint32_t, slots); PFP_ALLOC_HI(c, tfreq, unsigned long long, slots);
    PFP_ALLOC_HI(c, d_list, uint32_t, npc); PFP_ALLOC_HI(c, d_route, uint8_t, npc); PFP_ALLOC_HI(c, d_ub, unsigned long long, npc + 1); PFP_ALLOC_HI(c, d_pbase, unsigned long long, npc + 1);
    PFP_ALLOC_HI(c, ne, unsigned long long, npc + 1);
    PFP_TRY(h2d_copy(c, (uint8_t *)d_list, (const uint8_t *)list.data(), npc * 4));
    PFP_TRY(h2d_copy(c, d_route, proute.data(), npc));
    PFP_TRY(h2d_copy(c, (uint8_t *)d_ub, (const uint8_t *)ub.data(), (npc + 1) * 8));
    PFP_TRY(h2d_copy(c, (uint8_t *)d_pbase, (const uint8_t *)pbase.data(), (npc + 1) * 8));
    PFP_HIP(c, hipMemsetAsync(ne, 0, (size_t)(npc + 1) * 8, c->stream));
    PFP_HIP(c, hipMemsetAsync(tfreq, 0, (size_t)(slots ? slots : 1) * 8, c->stream));
    const int idbits = bits_for(distinct ? distinct - 1 : 0);
    PFP_LAUNCH(c, K_MK_REDUCE, raw * 60, (k_mk_expand<T>), nblocks(raw, BLOCK), a.mv, a.slo, a.scnt, a.ka, a.rbase, s0, nslots, (const unsigned long long *)d_pbase, npc, (const uint8_t *)d_route, raw, idbits, k0, v0, wt);
    if (nwave) PFP_LAUNCH(c, K_MK_REDUCE, nwave * 64 * 28, k_mk_wave, nblocks(nwave, BLOCK / WAVE), (const uint64_t *)k0, (const unsigned long long *)wt, (const unsigned long long *)d_pbase, (const unsigned long long *)d_ub, (const uint32_t *)d_list, nwave,
                          idbits, tid, tfreq, ne);
    if (nsort) {
        uint32_t *head, *hpos, *hl, *d_nh, *first, *last;
        PFP_ALLOC_HI(c, k1, uint64_t, raw); PFP_ALLOC_HI(c, v1, uint32_t, raw);
        PFP_ALLOC_HI(c, head, uint32_t, raw); PFP_ALLOC_HI(c, hpos, uint32_t, raw); PFP_ALLOC_HI(c, hl, uint32_t, raw); PFP_ALLOC_HI(c, d_nh, uint32_t, 1);
        PFP_ALLOC_HI(c, first, uint32_t, npc); PFP_ALLOC_HI(c, last, uint32_t, npc);
        const BitRange range = {0, idbits + bits_for(npc)};
        PFP_TRY((radix_sort_pairs<uint64_t>(c, k0, v0, k1, v1, raw, &range, 1, &sk, &sv)));
        PFP_LAUNCH(c, K_MK_REDUCE, raw * 12, k_dl_heads, nblocks(raw, BLOCK), (const uint64_t *)sk, raw, head);
        PFP_TRY(device_compact(c, nullptr, head, raw, hl, hpos, d_nh));
        uint32_t nh = 0; PFP_TRY(d2h_u32(c, d_nh, &nh));
        PFP_HIP(c, hipMemsetAsync(first, 0, (size_t)npc * 4, c->stream)); PFP_HIP(c, hipMemsetAsync(last, 0, (size_t)npc * 4, c->stream));
        PFP_LAUNCH(c, K_MK_REDUCE, (uint64_t)nh * 16, k_dl_spans, nblocks(nh, BLOCK), (const uint64_t *)sk, (const uint32_t *)hl, (uint64_t)nh, raw, npc, idbits, first, last);
        PFP_LAUNCH(c, K_MK_REDUCE, raw * 40, k_mk_sum, nblocks(raw, BLOCK), (const uint64_t *)sk, (const uint32_t *)sv, (const unsigned long long *)wt, (const uint32_t *)head, (const uint32_t *)hpos, raw, npc, idbits, distinct,
                   (const uint32_t *)first, (const uint32_t *)last, (const unsigned long long *)d_ub, tid, tfreq, ne);
    }
    // tight, in pattern order, behind the e0 pairs of the chunks in front
    PFP_TRY((device_scan<unsigned long long, 0>(c, ne, ne, npc, ne + npc)));
    if (slots) PFP_LAUNCH(c, K_MK_REDUCE, slots * 36, k_mk_pack, nblocks(slots, BLOCK), (const uint32_t *)tid, (const unsigned long long *)tfreq, a.mval, distinct, (const unsigned long long *)d_ub, (const unsigned long long *)ne, npc, slots, e0,
                          a.cap, a.marker, a.freq);
    PFP_HIP(c, hipMemcpyAsync(ooff.data(), ne, (size_t)(npc + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    for (uint64_t q = 0; q < npc; ++q) (*mk_off)[(size_t)(j0 + q + 1)] = e0 + ooff[(size_t)q + 1];
    if (e0 + ooff[(size_t)npc] > a.cap) return PFP_E_CORRUPT;
    c->arena.release_hi(mk);
    return PFP_OK;
}
template <typename T> static int mk_query_impl(pfp_ctx *c, const uint8_t *bases, const uint64_t *offsets, uint64_t np, uint64_t min_len, uint64_t max_rows, pfp_mk_info *info)
{
    PatternBatch pb(bases, offsets, np);
    const uint64_t total = pb.total, distinct = c->mkx.distinct;
    // the result of an earlier call gives its space back first, the pairs (on top) before the counts
    { PostResult drop(c, c->mkl); }
    PostResult res(c, c->mk);
    c->mk_patterns = c->mk_entries = 0; c->mk_off.clear();
    T *cnt, *probes;
    PFP_ALLOC_LO(c, cnt, T, np); PFP_ALLOC_LO(c, probes, T, np);
    PostResult resl(c, c->mkl);                                            // (after the counts: its mark is their end)
    const size_t mk = c->arena.mark_hi();
    T *slo, *scnt; uint32_t *ka; unsigned long long *rbase, *d_praw, *d_out;
    PFP_TRY(pb.upload(c, K_MK_SEARCH));
    PFP_ALLOC_HI(c, slo, T, total); PFP_ALLOC_HI(c, scnt, T, total); PFP_ALLOC_HI(c, ka, uint32_t, total); PFP_ALLOC_HI(c, rbase, unsigned long long, total + 1);
    PFP_ALLOC_HI(c, d_praw, unsigned long long, np); PFP_ALLOC_HI(c, d_out, unsigned long long, OUT_BLOCK);
    PFP_HIP(c, hipMemsetAsync(d_out, 0, sizeof(unsigned long long) * OUT_BLOCK, c->stream));
    const MsView<T> ix = ri_view<T>(c);
    const MkView mv = mk_view(c);
    std::vector<uint64_t> praw((size_t)np, 0), mk_off((size_t)np + 1, 0);
    if (np) PFP_LAUNCH(c, K_MK_SEARCH, total * (1 + 2 * sizeof(T)) + np * 2 * sizeof(T), (k_mk_search<T>), nblocks(np, BLOCK), ix, (const uint8_t *)pb.P, (const uint64_t *)pb.d_off, (const uint32_t *)pb.d_order, np, min_len, max_rows,
                       slo, scnt, cnt, probes, d_out);
    if (total) PFP_LAUNCH(c, K_MK_SEARCH, total * (12 + 2 * sizeof(T)), (k_mk_span<T>), nblocks(total, BLOCK), mv, (const T *)slo, (const T *)scnt, total, ka, rbase, d_out);
    PFP_TRY((device_scan<unsigned long long, 0>(c, rbase, rbase, total, rbase + total)));
    if (np) {
        PFP_LAUNCH(c, K_MK_SEARCH, np * 32, k_mk_praw, nblocks(np, BLOCK), (const unsigned long long *)rbase, (const uint64_t *)pb.d_off, np, d_praw);
        PFP_HIP(c, hipMemcpyAsync(praw.data(), d_praw, (size_t)np * 8, hipMemcpyDeviceToHost, c->stream));
        PFP_HIP(c, hipStreamSynchronize(c->stream));
    }
    // host: the upper bound of the pairs
    uint64_t cap = 0, raw_all = 0;
    for (uint64_t j = 0; j < np; ++j) { raw_all += praw[(size_t)j]; cap += praw[(size_t)j] < distinct ? praw[(size_t)j] : distinct; }
    uint64_t *marker, *freq;
    PFP_ALLOC_LO(c, marker, uint64_t, cap); PFP_ALLOC_LO(c, freq, uint64_t, cap);
    const uint64_t budget = mk_budget(c, np);
    const MkCall<T> call = {mv, c->mkx.mval, slo, scnt, ka, rbase, &pb.off, &praw, marker, freq, cap};
    uint64_t chunks = 0, e0 = 0, by[2] = {0, 0};
    for (uint64_t j0 = 0; j0 < np;) {                                      // a chunk: patterns in order while their raw entries fit the budget, one at least
        uint64_t j1 = j0, raw = 0;
        while (j1 < np && (j1 == j0 || raw + praw[(size_t)j1] <= budget)) raw += praw[(size_t)j1++];
        PFP_TRY(mk_chunk<T>(c, call, j0, j1, e0, &mk_off, by));
        e0 = mk_off[(size_t)j1];
        ++chunks; j0 = j1;
    }
    unsigned long long h[OUT_BLOCK] = {};
    PFP_HIP(c, hipMemcpyAsync(h, d_out, sizeof h, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    c->arena.release_hi(mk);
    // freq moves down behind the e0 pairs of marker, through a bounce buffer (source and destination may overlap), and the tail is free again
    const size_t marker_at = c->arena.offset_of(marker), freq_at = (marker_at + (size_t)(e0 ? e0 : 1) * 8 + 255) & ~(size_t)255;
    uint64_t *freq_final = (uint64_t *)(c->arena.base + freq_at);
    if (freq_final != freq && e0) {
        size_t bytes = (size_t)e0 * 8, piece = bytes < ((size_t)64 << 20) ? bytes : ((size_t)64 << 20);
        const size_t want0 = c->arena.want;
        uint8_t *bounce;
        while (!(bounce = (uint8_t *)c->arena.alloc_hi(piece))) {
            if (piece <= 4096) return PFP_E_NOMEM;
            piece /= 2; c->arena.failed = false; c->arena.want = want0;
        }
        for (size_t at = 0; at < bytes; at += piece) {
            const size_t len = bytes - at < piece ? bytes - at : piece;
            PFP_HIP(c, hipMemcpyAsync(bounce, (const uint8_t *)freq + at, len, hipMemcpyDeviceToDevice, c->stream));
            PFP_HIP(c, hipMemcpyAsync((uint8_t *)freq_final + at, bounce, len, hipMemcpyDeviceToDevice, c->stream));
        }
        PFP_HIP(c, hipStreamSynchronize(c->stream));
        c->arena.release_hi(mk);
    }
    c->arena.release_lo(freq_at + (size_t)(e0 ? e0 : 1) * 8);
    res.commit_under(resl, cnt, probes);
    resl.commit(marker, freq_final);
    uint64_t listed = 0, max_markers = 0;
    for (uint64_t j = 0; j < np; ++j) { const uint64_t d = mk_off[(size_t)j + 1] - mk_off[(size_t)j]; listed += d != 0; if (d > max_markers) max_markers = d; }
    c->mk_patterns = np; c->mk_entries = e0; c->mk_off.swap(mk_off);
    if (c->tun.verbose) fprintf(stderr, "[pfbwt_hip] mk query: %llu patterns, %llu probes, %llu raw entries, %llu chunks, %llu pairs of at most %llu\n", (unsigned long long)np, h[MK_PROBES], (unsigned long long)raw_all, (unsigned long long)chunks,
                                (unsigned long long)e0, (unsigned long long)cap);
    if (info) {
        info->patterns = np; info->bases = total; info->found = h[MK_FOUND]; info->occurrences = h[MK_OCCURRENCES]; info->steps = h[MK_STEPS]; info->probes = h[MK_PROBES]; info->capped = h[MK_CAPPED]; info->rows = h[MK_ROWS];
        info->records = h[MK_RECORDS]; info->raw = raw_all; info->listed = listed; info->entries = e0; info->max_markers = max_markers; info->chunks = chunks; info->by_wave = by[0]; info->by_sort = by[1];
    }
    return PFP_OK;
}
int pfp_mk_query(pfp_ctx *c, const uint8_t *bases, const uint64_t *offsets, uint64_t npatterns, uint64_t min_len, uint64_t max_rows, pfp_mk_info *info)
{
    if (!c || !bases || !offsets) return PFP_E_ARG;
    if (!has_mk_index(c) || !has_ri_index(c) || ri_state(c) != PFP_OK) return PFP_E_STATE;
    PFP_TRY(pattern_args_check(c, bases, offsets, npatterns));
    return post_entry(c, [&](auto t) { return mk_query_impl<decltype(t)>(c, bases, offsets, npatterns, min_len, max_rows, info); });
}
int pfp_mk_query_file(pfp_ctx *c, const char *path, uint64_t min_len, uint64_t max_rows, pfp_mk_info *info)
{
    if (!c || !path) return PFP_E_ARG;
    if (!has_mk_index(c) || !has_ri_index(c)) return PFP_E_STATE;
    return pattern_file_query(path, [&](const uint8_t *bases, const uint64_t *off, uint64_t np) { return pfp_mk_query(c, bases, off, np, min_len, max_rows, info); });
}
int pfp_mk_offsets_get(pfp_ctx *c, uint64_t *mk_off, uint64_t *npatterns)
{
    if (!c) return PFP_E_ARG;
    return offsets_get(has_mk_result(c), c->mk_off, mk_off, npatterns);
}
int pfp_mk_get(pfp_ctx *c, void *cnt, void *probes, uint64_t *marker, uint64_t *freq)
{
    if (!c) return PFP_E_ARG;
    if (!has_mk_result(c)) return PFP_E_STATE;
    void *const a[2] = {cnt, probes}, *const b[2] = {marker, freq};
    PFP_TRY(family_get(c, mk_family(c), a));
    return family_get(c, mkl_family(c), b);
}
int pfp_mk_device_ptrs(pfp_ctx *c, const void **d_cnt, const void **d_probes, const void **d_marker, const void **d_freq)
{
    if (!c) return PFP_E_ARG;
    const void **const a[2] = {d_cnt, d_probes}, **const b[2] = {d_marker, d_freq};
    family_device_ptrs(mk_family(c), a);
    return family_device_ptrs(mkl_family(c), b);
}
int pfp_mk_write(pfp_ctx *c, int fd_cnt, int fd_probes, int fd_off, int fd_marker, int fd_freq)
{
    if (!c) return PFP_E_ARG;
    if (!has_mk_result(c)) return PFP_E_STATE;
    const int a[2] = {fd_cnt, fd_probes}, b[2] = {fd_marker, fd_freq};
    PFP_TRY(family_write(c, mk_family(c), a));
    PFP_TRY(family_write(c, mkl_family(c), b));
    return fd_off >= 0 ? write_all(fd_off, c->mk_off.data(), c->mk_off.size() * 8) : PFP_OK;
}
