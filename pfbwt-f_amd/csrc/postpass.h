// pfbwt-f_amd/csrc/postpass.h -- the array post-passes over a finished build and their entries: marker array (markers.h), document
// arrays (docarray.h), LCP arrays (lcparray.h), thresholds resident and windowed (thresholds.h).  Every one computes into scratch at
// the high end of the arena and leaves its result in a slot of the context at the low end (common.h: ResultSlot, PostResult), where
// it lives until the next build or reset.  post_entry, the state predicates and ResultFamily (one fetch path for every result) also
// serve the queries on top of a build, which live in queries.h.
// Host code only; included by pfbwt_hip.hip.
#pragma once

// one post-pass entry: the context's device, an arena that a failure leaves as it found it, the body for the uint_t of the context
// (body: a generic lambda, called with a value of that type)
template <typename F> static int post_entry(pfp_ctx *c, F body)
{
    PFP_HIP(c, hipSetDevice(c->device));
    ArenaGuard g(c);
    if (c->flags & PFP_FLAG_U64) return g.done(body(uint64_t()));
    return g.done(body(uint32_t()));
}
// what a post-pass may need of the state of the context
static bool has_build(const pfp_ctx *c) { return c->stage >= 3 && c->nout && c->d_bwt; }
static bool holds_build_text(const pfp_ctx *c) { return c->tb && c->tb_n && c->tb_n == c->n && c->nout == c->n + 1; }      // not so in a loaded / merged state
static bool has_whole_sa(const pfp_ctx *c) { return c->d_sa && c->have_sa && c->slice_rows == c->nout; }                  // the SA of the whole output, not a slice
static bool has_run_samples(const pfp_ctx *c) { return c->have_rssa && c->d_ssa && c->d_esa; }

// The arrays of one family of results, for the three ways out of the context: device pointer and count of U-wide values each.
// whole: the family exists as a whole or not at all, whatever is asked for (else only what is asked for has to exist).
struct ResultRow { const void *d; uint64_t count; };
struct ResultFamily { int n; ResultRow row[3]; bool whole; };
static ResultFamily doc_family(const pfp_ctx *c) { return {3, {{c->da.p[0], c->slice_rows}, {c->da.p[1], 2 * c->runs}, {c->da.p[2], 2 * c->esa_pairs}}, false}; }
static ResultFamily lcp_family(const pfp_ctx *c) { return {2, {{c->lcp.p[0], c->slice_rows}, {c->lcp.p[1], 2 * c->runs}, {nullptr, 0}}, false}; }
static ResultFamily thr_family(const pfp_ctx *c) { return {2, {{c->thr.p[0], 2 * c->runs}, {c->thr.p[1], 2 * c->runs}, {nullptr, 0}}, true}; }
static int family_state(const ResultFamily &f, const bool *asked)
{
    for (int k = 0; k < f.n; ++k) if ((f.whole || asked[k]) && !f.row[k].d) return PFP_E_STATE;
    return PFP_OK;
}
// dst[k] == nullptr: not asked for
static int family_get(pfp_ctx *c, const ResultFamily &f, void *const *dst)
{
    const bool asked[3] = {dst[0] != nullptr, dst[1] != nullptr, f.n > 2 && dst[2] != nullptr};
    PFP_TRY(family_state(f, asked));
    PFP_HIP(c, hipSetDevice(c->device));
    const size_t U = (c->flags & PFP_FLAG_U64) ? 8 : 4;
    for (int k = 0; k < f.n; ++k) if (asked[k] && f.row[k].count) PFP_HIP(c, hipMemcpy(dst[k], f.row[k].d, f.row[k].count * U, hipMemcpyDeviceToHost));      // (no run at all: nothing to copy)
    return PFP_OK;
}
static int family_device_ptrs(const ResultFamily &f, const void **const *out)
{
    for (int k = 0; k < f.n; ++k) if (out[k]) *out[k] = f.row[k].d;
    return PFP_OK;
}
// fd[k] < 0: not asked for
static int family_write(pfp_ctx *c, const ResultFamily &f, const int *fd)
{
    const bool asked[3] = {fd[0] >= 0, fd[1] >= 0, f.n > 2 && fd[2] >= 0};
    PFP_TRY(family_state(f, asked));
    PFP_HIP(c, hipSetDevice(c->device));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    const size_t U = (c->flags & PFP_FLAG_U64) ? 8 : 4;
    for (int k = 0; k < f.n; ++k) if (asked[k]) PFP_TRY(write_device_to_fd(c, (const uint8_t *)f.row[k].d, f.row[k].count * U, fd[k]));
    return PFP_OK;
}

// ---- marker-array post-pass (include/marker_array.hpp:138-174, src/mps_to_ma.cpp) ----------------------
template <typename SAT> static int marker_array_impl(pfp_ctx *c, const uint64_t *mps, uint64_t mps_words, const SAT *d_sa, uint64_t nrows, uint64_t *out_words)
{
    // host: the records of the .mps stream; every distinct marker list gets one id (the reference compares lists by content)
    std::vector<uint64_t> istart, iend, lvals; std::vector<uint32_t> ilist, loff(1, 0u);
    std::map<std::vector<uint64_t>, uint32_t> ids;
    for (uint64_t i = 0; i < mps_words;) {
        uint64_t j = i;
        while (j < mps_words && mps[j] != ~0ULL) ++j;
        if (j == mps_words || j - i < 2) return PFP_E_CORRUPT;                 // a record without its keys or its delimiter
        if (!istart.empty() && (mps[i] <= iend.back() || mps[i + 1] < mps[i])) return PFP_E_CORRUPT;   // intervals ascend and do not overlap (rle_window_array.hpp:31-34)
        std::vector<uint64_t> lst(mps + i + 2, mps + j);
        auto it = ids.find(lst);
        uint32_t id;
        if (it != ids.end()) id = it->second;
        else { id = (uint32_t)ids.size(); ids.emplace(lst, id); lvals.insert(lvals.end(), lst.begin(), lst.end()); loff.push_back((uint32_t)lvals.size()); }
        // a record with an empty list answers at() like no record at all
        if (!lst.empty()) { istart.push_back(mps[i]); iend.push_back(mps[i + 1]); ilist.push_back(id); }
        i = j + 1;
    }
    if (istart.size() >= 0xFFFFFFF0ULL || lvals.size() >= 0xFFFFFFF0ULL || nrows >= 0xFFFFFFF0ULL) return PFP_E_TOO_LARGE;      // run heads are counted and placed with 32-bit values
    const uint32_t nint = (uint32_t)istart.size();
    const size_t mk = c->arena.mark_hi();
    uint64_t *d_is, *d_ie, *d_lv; uint32_t *d_il, *d_lo, *rowlist, *head, *pos, *d_cnt;
    PFP_ALLOC_HI(c, d_is, uint64_t, nint); PFP_ALLOC_HI(c, d_ie, uint64_t, nint); PFP_ALLOC_HI(c, d_il, uint32_t, nint);
    PFP_ALLOC_HI(c, d_lo, uint32_t, loff.size()); PFP_ALLOC_HI(c, d_lv, uint64_t, lvals.size());
    PFP_ALLOC_HI(c, rowlist, uint32_t, nrows); PFP_ALLOC_HI(c, head, uint32_t, nrows); PFP_ALLOC_HI(c, pos, uint32_t, nrows); PFP_ALLOC_HI(c, d_cnt, uint32_t, 1);
    if (nint) {
        PFP_HIP(c, hipMemcpyAsync(d_is, istart.data(), (size_t)nint * 8, hipMemcpyHostToDevice, c->stream));
        PFP_HIP(c, hipMemcpyAsync(d_ie, iend.data(), (size_t)nint * 8, hipMemcpyHostToDevice, c->stream));
        PFP_HIP(c, hipMemcpyAsync(d_il, ilist.data(), (size_t)nint * 4, hipMemcpyHostToDevice, c->stream));
    }
    PFP_HIP(c, hipMemcpyAsync(d_lo, loff.data(), loff.size() * 4, hipMemcpyHostToDevice, c->stream));
    if (!lvals.empty()) PFP_HIP(c, hipMemcpyAsync(d_lv, lvals.data(), lvals.size() * 8, hipMemcpyHostToDevice, c->stream));
    const unsigned gr = nblocks(nrows, BLOCK);
    PFP_LAUNCH(c, K_MISC, nrows * (sizeof(SAT) + 4 + 40), (k_ma_lookup<SAT>), gr, d_sa, nrows, (const uint64_t *)d_is, (const uint64_t *)d_ie, (const uint32_t *)d_il, nint, rowlist);
    PFP_LAUNCH(c, K_MISC, nrows * 8, k_ma_heads, gr, (const uint32_t *)rowlist, nrows, head);
    PFP_TRY((device_scan<uint32_t, 0>(c, head, pos, nrows, d_cnt)));
    uint32_t nh = 0; PFP_TRY(d2h_u32(c, d_cnt, &nh));          // also waits for the host vectors' uploads
    uint64_t *hrow; uint32_t *hlist; unsigned long long *len, *off, *d_tot;
    PFP_ALLOC_HI(c, hrow, uint64_t, nh); PFP_ALLOC_HI(c, hlist, uint32_t, nh); PFP_ALLOC_HI(c, len, unsigned long long, nh); PFP_ALLOC_HI(c, off, unsigned long long, nh); PFP_ALLOC_HI(c, d_tot, unsigned long long, 1);
    PFP_LAUNCH(c, K_MISC, nrows * 12, k_ma_collect, gr, (const uint32_t *)rowlist, (const uint32_t *)head, (const uint32_t *)pos, nrows, hrow, hlist);
    PFP_LAUNCH(c, K_MISC, (uint64_t)nh * 16, k_ma_lengths, nblocks(nh, BLOCK), (const uint32_t *)hlist, (const uint32_t *)d_lo, (uint64_t)nh, len);
    PFP_TRY((device_scan<unsigned long long, 0>(c, len, off, nh, d_tot)));
    unsigned long long tot = 0;
    PFP_HIP(c, hipMemcpyAsync(&tot, d_tot, 8, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    // a result of an earlier call on the same build (several .mps streams against one suffix array) gives its space back first
    PostResult res(c, c->ma);
    c->ma_words = 0;
    if (tot) {
        uint64_t *d_out; PFP_ALLOC_LO(c, d_out, uint64_t, tot);                // result: low end, survives the release of the scratch
        PFP_LAUNCH(c, K_MISC, tot * 8, k_ma_write, nblocks(nh, BLOCK), (const uint64_t *)hrow, (const uint32_t *)hlist, (const unsigned long long *)off, (const uint32_t *)d_lo, (const uint64_t *)d_lv, (uint64_t)nh, nrows, d_out);
        PFP_HIP(c, hipStreamSynchronize(c->stream));
        res.commit(d_out); c->ma_words = tot;
    }
    c->arena.release_hi(mk);
    if (out_words) *out_words = tot;
    return PFP_OK;
}

int pfp_marker_array(pfp_ctx *c, const uint64_t *mps, uint64_t mps_words, const void *sa_host, uint64_t nrows, uint64_t *out_words)
{
    if (!c || (!mps && mps_words)) return PFP_E_ARG;
    if (!sa_host) {      // fused: the suffix array the last pfp_bwt_build(want_sa = 1) left on the device (whole output, not a slice)
        if (c->stage < 3 || !c->d_sa || c->slice_rows != c->nout) return PFP_E_STATE;
        return post_entry(c, [&](auto t) { return marker_array_impl(c, mps, mps_words, (const decltype(t) *)c->d_sa, c->nout, out_words); });
    }
    if (!nrows) return PFP_E_ARG;      // stand-alone (src/mps_to_ma.cpp): the suffix array comes from a file or pipe
    PFP_HIP(c, hipSetDevice(c->device));
    reset_results(c);
    PFP_TRY(ensure_arena(c, nrows));
    c->arena.reset();
    return post_entry(c, [&](auto t) -> int {
        decltype(t) *d_sa; PFP_ALLOC_HI(c, d_sa, decltype(t), nrows);
        PFP_TRY(h2d_copy(c, (uint8_t *)d_sa, (const uint8_t *)sa_host, nrows * sizeof(t)));
        return marker_array_impl(c, mps, mps_words, (const decltype(t) *)d_sa, nrows, out_words);
    });
}
int pfp_marker_array_get(pfp_ctx *c, uint64_t *dst)
{
    if (!c || (!dst && c->ma_words)) return PFP_E_ARG;
    PFP_HIP(c, hipSetDevice(c->device));
    if (c->ma_words) PFP_HIP(c, hipMemcpy(dst, c->ma.p[0], c->ma_words * 8, hipMemcpyDeviceToHost));
    return PFP_OK;
}

// ---- document-array post-pass (include/pfbwt_hip.h: pfp_doc_array; csrc/docarray.h) ---------------------------------------
struct DocTable { const void *d_starts; uint32_t ndocs, shift, ntab, top; };
// one lookup pass over cnt values of src into dst (dst allocated with the same alignment modulo 16 as src)
template <typename T> static int doc_lookup_pass(pfp_ctx *c, const T *src, T *dst, uint64_t cnt, bool pairs, const DocTable &t)
{
    if (!cnt) return PFP_OK;
    const uint32_t h = (uint32_t)vec_head(src, cnt);
    const bool small = t.ntab <= DOC_LDS_SMALL;
    const unsigned grid = stream_grid<T>(cnt, h, small ? DOC_WG_PER_CU_SMALL : DOC_WG_PER_CU_BIG);
    const T *st = (const T *)t.d_starts;
    const double bytes = (double)cnt * 2 * sizeof(T);
    if (small && pairs) PFP_LAUNCH(c, K_DOC, bytes, (k_doc_lookup<T, DOC_LDS_SMALL, true>), grid, src, dst, cnt, h, st, t.ndocs, t.shift, t.ntab, t.top);
    else if (small) PFP_LAUNCH(c, K_DOC, bytes, (k_doc_lookup<T, DOC_LDS_SMALL, false>), grid, src, dst, cnt, h, st, t.ndocs, t.shift, t.ntab, t.top);
    else if (pairs) PFP_LAUNCH(c, K_DOC, bytes, (k_doc_lookup<T, DOC_LDS_CAP, true>), grid, src, dst, cnt, h, st, t.ndocs, t.shift, t.ntab, t.top);
    else PFP_LAUNCH(c, K_DOC, bytes, (k_doc_lookup<T, DOC_LDS_CAP, false>), grid, src, dst, cnt, h, st, t.ndocs, t.shift, t.ntab, t.top);
    return PFP_OK;
}
template <typename T> static int doc_array_impl(pfp_ctx *c, const uint64_t *starts, uint64_t ndocs, unsigned what)
{
    std::vector<T> hs((size_t)ndocs);
    for (uint64_t k = 0; k < ndocs; ++k) hs[(size_t)k] = (T)starts[k];
    DocTable t;
    t.ndocs = (uint32_t)ndocs; t.shift = 0;
    const uint32_t lds = c->tun.doc_lds_max < DOC_LDS_CAP ? c->tun.doc_lds_max : DOC_LDS_CAP;
    while (((ndocs - 1) >> t.shift) + 1 > lds) ++t.shift;                   // two-level: every 2^shift-th start in LDS
    t.ntab = (uint32_t)(((ndocs - 1) >> t.shift) + 1);
    t.top = 1; while (2 * t.top < t.ntab) t.top *= 2;                      // largest power of two below ntab (1 for ntab <= 2)
    PostResult res(c, c->da);
    const size_t mk = c->arena.mark_hi();
    T *d_starts; PFP_ALLOC_HI(c, d_starts, T, ndocs);
    PFP_HIP(c, hipMemcpyAsync(d_starts, hs.data(), (size_t)ndocs * sizeof(T), hipMemcpyHostToDevice, c->stream));
    t.d_starts = d_starts;
    T *da = nullptr, *sda = nullptr, *eda = nullptr;
    if (what & PFP_DA_ROWS) { const T *s = (const T *)c->d_sa; if (!(da = alloc_congruent(c, s, c->slice_rows, false))) return PFP_E_NOMEM; PFP_TRY(doc_lookup_pass<T>(c, s, da, c->slice_rows, false, t)); }
    if (what & PFP_DA_RUNS) {
        const T *s = (const T *)c->d_ssa, *e = (const T *)c->d_esa;
        if (!(sda = alloc_congruent(c, s, 2 * c->runs, false)) || !(eda = alloc_congruent(c, e, 2 * c->esa_pairs, false))) return PFP_E_NOMEM;
        PFP_TRY(doc_lookup_pass<T>(c, s, sda, 2 * c->runs, true, t));
        PFP_TRY(doc_lookup_pass<T>(c, e, eda, 2 * c->esa_pairs, true, t));
    }
    PFP_HIP(c, hipStreamSynchronize(c->stream));                           // (hs is read by the upload until here)
    c->arena.release_hi(mk);
    res.commit(da, sda, eda);
    return PFP_OK;
}

int pfp_doc_array(pfp_ctx *c, const uint64_t *starts, uint64_t ndocs, unsigned what)
{
    if (!c || !starts || !ndocs || !what || (what & ~(unsigned)(PFP_DA_ROWS | PFP_DA_RUNS))) return PFP_E_ARG;
    if (c->stage < 3 || !c->nout) return PFP_E_STATE;
    if (((what & PFP_DA_ROWS) && !c->d_sa) || ((what & PFP_DA_RUNS) && (!c->d_ssa || !c->d_esa))) return PFP_E_STATE;      // no SA values of that kind were built (a slice will do)
    const uint64_t n = c->nout - 1;
    if (starts[0] != 0) return PFP_E_ARG;
    for (uint64_t k = 1; k < ndocs; ++k) if (starts[k] <= starts[k - 1]) return PFP_E_ARG;
    if (starts[ndocs - 1] >= n) return PFP_E_ARG;
    if (ndocs > 0xFFFFFFFFULL) return PFP_E_TOO_LARGE;
    return post_entry(c, [&](auto t) { return doc_array_impl<decltype(t)>(c, starts, ndocs, what); });
}
int pfp_doc_array_get(pfp_ctx *c, void *da, void *sda, void *eda)
{
    if (!c) return PFP_E_ARG;
    void *const dst[3] = {da, sda, eda};
    return family_get(c, doc_family(c), dst);
}
int pfp_doc_array_device_ptrs(pfp_ctx *c, const void **d_da, const void **d_sda, const void **d_eda)
{
    if (!c) return PFP_E_ARG;
    const void **const out[3] = {d_da, d_sda, d_eda};
    return family_device_ptrs(doc_family(c), out);
}
int pfp_doc_array_write(pfp_ctx *c, int fd_da, int fd_sda, int fd_eda)
{
    if (!c) return PFP_E_ARG;
    const int fd[3] = {fd_da, fd_sda, fd_eda};
    return family_write(c, doc_family(c), fd);
}

// ---- LCP-array post-pass (include/pfbwt_hip.h: pfp_lcp_array; csrc/lcparray.h) ---------------------------------------------
// The values themselves: lcp (nullable; nrows values, congruent to the SA modulo 16) and / or slcp (nullable; 2 * r values), both allocated
// by the caller.  Scratch (K, the queue) comes from the high end of the arena and is released before returning; h = the five counters
// of lcp_wave_stats.  Returns after the stream has drained.
template <typename T> static int lcp_compute(pfp_ctx *c, T *lcp, T *slcp, unsigned long long h[5])
{
    const bool rows = lcp != nullptr;
    const bool from_samples = has_run_samples(c);                          // else: run starts found in bwt / sa
    const uint64_t n = c->n, r = c->runs, nrows = c->slice_rows;
    const uint8_t *X = (const uint8_t *)c->tb + 16;
    const size_t mk = c->arena.mark_hi();
    T *K = nullptr;
    if (rows) { PFP_ALLOC_HI(c, K, T, n + 1); PFP_HIP(c, hipMemsetAsync(K, 0, (size_t)(n + 1) * sizeof(T), c->stream)); }
    const uint64_t pairs_max = from_samples ? r : nrows;
    uint64_t qcap = pairs_max < LCP_QUEUE_CAP ? pairs_max : LCP_QUEUE_CAP;
    unsigned long long *d_out; PFP_ALLOC_HI(c, d_out, unsigned long long, 8);
    LcpLong *queue = alloc_queue_shrinking<LcpLong>(c, &qcap);
    if (!queue) return PFP_E_NOMEM;
    PFP_HIP(c, hipMemsetAsync(d_out, 0, 64, c->stream));
    const uint64_t cap = c->tun.lcp_long_min;
    if (from_samples) {
        if (r) PFP_LAUNCH(c, K_LCP_PAIRS, r * (64 + 4 * sizeof(T)), (k_lcp_pairs_samples<T>), nblocks(r, BLOCK), X, n, (const T *)c->d_ssa, (const T *)c->d_esa, r, c->slice_begin == 0 ? 1u : 0u, cap, slcp, K, queue, qcap, d_out);
    } else {
        PFP_LAUNCH(c, K_LCP_PAIRS, nrows * (1 + sizeof(T)), (k_lcp_pairs_rows<T>), nblocks(nrows, BLOCK), X, n, (const uint8_t *)c->d_bwt, (const T *)c->d_sa, nrows, cap, K, queue, qcap, d_out);
    }
    if (qcap) PFP_LAUNCH(c, K_LCP_LONG, 0, (k_lcp_long<T>), wave_grid(qcap, LCP_LONG_WG), X, n, (const LcpLong *)queue, qcap, cap, slcp, K, d_out);
    if (rows) {
        PFP_TRY((device_scan<T, 1>(c, K, K, n + 1, (T *)nullptr)));
        const uint64_t head = vec_head((const T *)c->d_sa, nrows);
        PFP_LAUNCH(c, K_LCP_GATHER, nrows * 3 * sizeof(T), (k_lcp_gather<T>), stream_grid<T>(nrows, head, 8), (const T *)c->d_sa, (const T *)K, n, lcp, nrows, (uint32_t)head);
    }
    PFP_HIP(c, hipMemcpyAsync(h, d_out, 40, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    c->arena.release_hi(mk);                                               // K, the queue
    return PFP_OK;
}
template <typename T> static int lcp_array_impl(pfp_ctx *c, unsigned what, pfp_lcp_info *info)
{
    const bool rows = (what & PFP_LCP_ROWS) != 0, runs = (what & PFP_LCP_RUNS) != 0;
    const uint64_t r = c->runs, nrows = c->slice_rows;
    PostResult res(c, c->lcp);
    T *lcp = nullptr, *slcp = nullptr;
    if (rows && !(lcp = alloc_congruent(c, (const T *)c->d_sa, nrows, false))) return PFP_E_NOMEM;
    if (runs) PFP_ALLOC_LO(c, slcp, T, 2 * r);
    unsigned long long h[5];
    PFP_TRY(lcp_compute<T>(c, lcp, slcp, h));
    if (info) { info->pairs = h[0]; info->max_lcp = h[1]; info->sum_lcp = h[2]; info->long_pairs = h[3]; }
    res.commit(lcp, slcp);
    return PFP_OK;
}

// ---- thresholds post-pass (include/pfbwt_hip.h: pfp_thresholds; csrc/thresholds.h) ------------------------------------------
// What the resident and the windowed route share: the way in (the result slot, the scratch mark, the tile size, thr / tlcp at the
// low end), the runs sorted by their head byte, the way out.
template <typename T> struct ThrPass {
    pfp_ctx *c; PostResult res; size_t mk; uint32_t tile_log2 = 4; T *thr = nullptr, *tlcp = nullptr;
    explicit ThrPass(pfp_ctx *c_) : c(c_), res(c_, c_->thr), mk(c_->arena.mark_hi()) { while ((1u << tile_log2) < c->tun.thr_tile) ++tile_log2; }
    int alloc_result() { PFP_ALLOC_LO(c, thr, T, 2 * c->runs); PFP_ALLOC_LO(c, tlcp, T, 2 * c->runs); return PFP_OK; }
    // sk[i] / sv[i] = head byte and index of the i-th run in the order of the head bytes; kv: four buffers of one value per run
    int sort_heads(uint64_t nrows, uint32_t *const kv[4], uint32_t **sk, uint32_t **sv)
    {
        const uint64_t r = c->runs;
        PFP_LAUNCH(c, K_THR_QUERIES, r * (1 + sizeof(T)), (k_thr_heads<T>), nblocks(r, BLOCK), (const uint8_t *)c->d_bwt, (const T *)c->d_ssa, r, nrows, kv[0], kv[1]);
        const BitRange byte_range = {0, 8};
        return radix_sort_pairs<uint32_t>(c, kv[0], kv[1], kv[2], kv[3], r, &byte_range, 1, sk, sv);
    }
    // the stream has drained: the scratch goes back, h = the counters of thr_wave_stats, the result is published
    int finish(const unsigned long long *h, pfp_thr_info *info)
    {
        c->arena.release_hi(mk);
        if (info) { info->runs = h[0]; info->none = h[1]; info->long_queries = h[2]; info->max_span = h[3]; }
        res.commit(thr, tlcp);
        return PFP_OK;
    }
};
template <typename T> static int thresholds_impl(pfp_ctx *c, pfp_thr_info *info)
{
    const uint64_t r = c->runs, nrows = c->slice_rows;
    ThrPass<T> tp(c);
    PFP_TRY(tp.alloc_result());
    T *const thr = tp.thr, *const tlcp = tp.tlcp;
    const T *lcp = (const T *)c->lcp.p[0];                                // the rows of a preceding pfp_lcp_array(PFP_LCP_ROWS) of this build
    if (!lcp) {                                                            // else: into scratch, released with everything else below
        T *rows_scratch = alloc_congruent(c, (const T *)c->d_sa, nrows, true);
        if (!rows_scratch) return PFP_E_NOMEM;
        unsigned long long h[5];
        PFP_TRY(lcp_compute<T>(c, rows_scratch, (T *)nullptr, h));
        lcp = rows_scratch;
    }
    const uint32_t tile_log2 = tp.tile_log2;
    const uint64_t ntiles = (nrows + (1ULL << tile_log2) - 1) >> tile_log2;
    T *tmin, *trow;
    PFP_ALLOC_HI(c, tmin, T, ntiles);
    PFP_ALLOC_HI(c, trow, T, ntiles);
    uint32_t *kv[4];
    for (uint32_t *&b : kv) PFP_ALLOC_HI(c, b, uint32_t, r);
    unsigned long long *d_out; PFP_ALLOC_HI(c, d_out, unsigned long long, 8);
    uint64_t qcap = r < THR_QUEUE_CAP ? r : THR_QUEUE_CAP;
    ThrLong *queue = alloc_queue_shrinking<ThrLong>(c, &qcap);
    if (!queue) return PFP_E_NOMEM;
    PFP_HIP(c, hipMemsetAsync(d_out, 0, 64, c->stream));
    const uint32_t head = (uint32_t)vec_head(lcp, 1ULL << tile_log2);      // (the same in every tile)
    PFP_LAUNCH(c, K_THR_TILES, nrows * sizeof(T), (k_thr_tile_min<T>), wave_grid(ntiles, THR_LONG_WG), lcp, nrows, head, tile_log2, ntiles, tmin, trow, (uint64_t)0);
    uint32_t *sk, *sv;
    PFP_TRY(tp.sort_heads(nrows, kv, &sk, &sv));
    PFP_LAUNCH(c, K_THR_QUERIES, r * (8 + 6 * sizeof(T)), (k_thr_queries<T>), nblocks(r, BLOCK), (const uint32_t *)sk, (const uint32_t *)sv, (const T *)c->d_ssa, lcp, r, nrows, (uint64_t)c->tun.thr_long_min,
               thr, tlcp, queue, qcap, d_out);
    PFP_LAUNCH(c, K_THR_LONG, 0, (k_thr_long<T>), wave_grid(qcap, THR_LONG_WG), lcp, (const T *)tmin, (const T *)trow, tile_log2, (const ThrLong *)queue, qcap, thr, tlcp,
               (const unsigned long long *)d_out);
    unsigned long long h[5];
    PFP_HIP(c, hipMemcpyAsync(h, d_out, 40, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    return tp.finish(h, info);                                             // (scratch: the scratch rows, tile minima, sort buffers, queue)
}

// ---- sparse PLCP and the windowed routes (include/pfbwt_hip.h: pfp_thresholds_windowed; csrc/lcparray.h, csrc/thresholds.h) ---------
template <typename T> struct SparsePlcp { const T *pq = nullptr, *pv = nullptr; const uint32_t *dir = nullptr; uint32_t B = 0; };
// (position, K) pairs in position order and their block directory, at the high end of the arena (the caller releases them).  The
// irreducible values are those of a preceding pfp_lcp_array(PFP_LCP_RUNS) of this build, else computed into scratch here.
template <typename T> static int plcp_build(pfp_ctx *c, SparsePlcp<T> *sp)
{
    const uint64_t n = c->n, r = c->runs;
    uint32_t B = 0;
    if (c->tun.plcp_block_log2 >= 0) B = (uint32_t)c->tun.plcp_block_log2;
    else while (B < (uint32_t)PLCP_BLOCK_LOG2_MAX && (n >> (B + 1)) >= r) ++B;          // about one run start per block
    while ((n >> B) + 2 > 0xFFFFFFFFULL) ++B;
    const uint64_t nblk = n >> B;
    T *pq, *pv; uint32_t *dir;
    PFP_ALLOC_HI(c, pq, T, r); PFP_ALLOC_HI(c, pv, T, r); PFP_ALLOC_HI(c, dir, uint32_t, nblk + 2);
    const size_t mk = c->arena.mark_hi();
    const T *slcp = (const T *)c->lcp.p[1];
    if (!slcp) {
        T *scratch; PFP_ALLOC_HI(c, scratch, T, 2 * r);
        unsigned long long h[5];
        PFP_TRY(lcp_compute<T>(c, (T *)nullptr, scratch, h));
        slcp = scratch;
    }
    uint64_t *k0, *k1; uint32_t *v0, *v1; unsigned long long *d_bad;
    PFP_ALLOC_HI(c, k0, uint64_t, r); PFP_ALLOC_HI(c, k1, uint64_t, r); PFP_ALLOC_HI(c, v0, uint32_t, r); PFP_ALLOC_HI(c, v1, uint32_t, r); PFP_ALLOC_HI(c, d_bad, unsigned long long, 1);
    PFP_HIP(c, hipMemsetAsync(d_bad, 0, 8, c->stream));
    PFP_LAUNCH(c, K_PLCP_BUILD, r * (sizeof(T) + 12), (k_plcp_keys<T>), nblocks(r, BLOCK), (const T *)c->d_ssa, r, k0, v0);
    const BitRange range = {0, bits_for(n)};
    uint64_t *sk; uint32_t *sv;
    PFP_TRY((radix_sort_pairs<uint64_t>(c, k0, v0, k1, v1, r, &range, 1, &sk, &sv)));
    PFP_LAUNCH(c, K_PLCP_BUILD, r * (12 + 3 * sizeof(T)) + (nblk + 2) * 4, (k_plcp_fill<T>), nblocks(r, BLOCK), (const uint64_t *)sk, (const uint32_t *)sv, slcp, r, n, B, nblk, pq, pv, dir, d_bad);
    unsigned long long bad = 0;
    PFP_HIP(c, hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    c->arena.release_hi(mk);                                               // the sort buffers, the scratch values
    if (bad) return PFP_E_CORRUPT;                                         // K must not decrease along the text
    sp->pq = pq; sp->pv = pv; sp->dir = dir; sp->B = B;
    return PFP_OK;
}
// the LCP rows of one SA window: lcp_raw = alloc_congruent(.., nullptr, ..) for the rows of the largest window; returns the rows,
// congruent to the SA window modulo 16
template <typename T> static int plcp_rows(pfp_ctx *c, const SparsePlcp<T> &sp, const T *sa, uint64_t rows, T *lcp_raw, T **lcp_out)
{
    T *lcp = congruent_to(lcp_raw, sa);
    const uint64_t head = vec_head(sa, rows);
    PFP_LAUNCH(c, K_LCP_SPARSE, rows * 3 * sizeof(T), (k_lcp_sparse_rows<T>), stream_grid<T>(rows, head, 8), sa, sp.pq, sp.pv, sp.dir, sp.B, c->n, lcp, rows, (uint32_t)head);
    *lcp_out = lcp;
    return PFP_OK;
}
template <typename T> static int rows_windowed_impl(pfp_ctx *c, uint64_t window_rows, void *host_sa, void *host_lcp)
{
    const size_t mk = c->arena.mark_hi();
    const uint64_t W = window_rows < c->nout ? window_rows : c->nout;
    SparsePlcp<T> sp;
    PFP_TRY(plcp_build<T>(c, &sp));
    T *lcp_raw = alloc_congruent(c, (const T *)nullptr, W, true);
    if (!lcp_raw) return PFP_E_NOMEM;
    PFP_TRY(visit_sa_windows(c, W, [&](uint64_t first, uint64_t rows, const void *d_sa) -> int {
        T *lcp;
        PFP_TRY(plcp_rows<T>(c, sp, (const T *)d_sa, rows, lcp_raw, &lcp));
        PFP_HIP(c, hipStreamSynchronize(c->stream));
        if (host_sa) PFP_HIP(c, hipMemcpy((T *)host_sa + first, d_sa, (size_t)rows * sizeof(T), hipMemcpyDeviceToHost));
        if (host_lcp) PFP_HIP(c, hipMemcpy((T *)host_lcp + first, lcp, (size_t)rows * sizeof(T), hipMemcpyDeviceToHost));
        return PFP_OK;
    }));
    c->arena.release_hi(mk);
    return PFP_OK;
}
template <typename T> static int thresholds_windowed_impl(pfp_ctx *c, uint64_t window_rows, pfp_thr_info *info, uint64_t *windows)
{
    const uint64_t r = c->runs, nrows = c->nout;
    ThrPass<T> tp(c);
    const uint32_t tile_log2 = tp.tile_log2;
    const uint64_t tile = 1ULL << tile_log2;
    uint64_t W = window_rows ? window_rows : c->tun.thr_window_rows;
    if (W > nrows) W = nrows;
    W = (W + tile - 1) / tile * tile;                                      // a tile never straddles two windows
    const uint64_t nwin = (nrows + W - 1) / W, ntiles = (nrows + tile - 1) >> tile_log2;
    PFP_TRY(tp.alloc_result());
    T *const thr = tp.thr, *const tlcp = tp.tlcp;
    SparsePlcp<T> sp;
    PFP_TRY(plcp_build<T>(c, &sp));
    // the runs by head byte, the inverse of that order, the first run of every window
    uint32_t *kv[4], *sk, *sv, *pos; unsigned long long *d_first, *d_out;
    for (uint32_t *&b : kv) PFP_ALLOC_HI(c, b, uint32_t, r);
    PFP_ALLOC_HI(c, pos, uint32_t, r); PFP_ALLOC_HI(c, d_first, unsigned long long, nwin + 1); PFP_ALLOC_HI(c, d_out, unsigned long long, 8);
    PFP_TRY(tp.sort_heads(nrows, kv, &sk, &sv));
    PFP_LAUNCH(c, K_THR_QUERIES, r * 8, k_thr_inverse, nblocks(r, BLOCK), (const uint32_t *)sv, r, pos);
    PFP_LAUNCH(c, K_THR_QUERIES, (nwin + 1) * 8, (k_thr_win_bounds<T>), nblocks(nwin + 1, BLOCK), (const T *)c->d_ssa, r, W, nwin, d_first);
    PFP_HIP(c, hipMemsetAsync(d_out, 0, 64, c->stream));
    PFP_LAUNCH(c, K_THR_QUERIES, r * (8 + 6 * sizeof(T)), (k_thr_win_init<T>), nblocks(r, BLOCK), (const uint32_t *)sk, (const uint32_t *)sv, (const T *)c->d_ssa, r, nrows, (uint64_t)c->tun.thr_long_min, thr, tlcp, d_out);
    std::vector<unsigned long long> first((size_t)nwin + 1);
    unsigned long long h[5];
    PFP_HIP(c, hipMemcpyAsync(first.data(), d_first, (size_t)(nwin + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipMemcpyAsync(h, d_out, 40, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    uint64_t max_jobs = 1;                                                 // a run of a window owns at most two jobs
    for (uint64_t w = 0; w < nwin; ++w) if (2 * (first[(size_t)w + 1] - first[(size_t)w]) > max_jobs) max_jobs = 2 * (first[(size_t)w + 1] - first[(size_t)w]);
    if (r > max_jobs) max_jobs = r;                                        // (the fold pass queues at most one entry per run)
    T *tmin, *trow;
    PFP_ALLOC_HI(c, tmin, T, ntiles);
    PFP_ALLOC_HI(c, trow, T, ntiles);
    T *lcp_raw = alloc_congruent(c, (const T *)nullptr, W, true);
    if (!lcp_raw) return PFP_E_NOMEM;
    // the window buffers of the emission, its scratch and the queue share what is left: the queue takes at most a quarter of it
    uint64_t qcap = max_jobs < THR_QUEUE_CAP ? max_jobs : THR_QUEUE_CAP;
    const size_t room = c->arena.hi > c->arena.lo ? (c->arena.hi - c->arena.lo) / 4 : 0;
    while (qcap > 4096 && sizeof(ThrLong) * (size_t)qcap > room) qcap /= 2;
    ThrLong *queue; PFP_ALLOC_HI(c, queue, ThrLong, qcap);
    const unsigned qgrid = wave_grid(qcap, THR_LONG_WG);
    uint64_t seen = 0;
    PFP_TRY(visit_sa_windows(c, W, [&](uint64_t ws, uint64_t rows, const void *d_sa) -> int {
        const uint64_t w = ws / W, we = ws + rows;
        if (ws % W || w >= nwin) return PFP_E_CORRUPT;
        T *lcp;
        PFP_TRY(plcp_rows<T>(c, sp, (const T *)d_sa, rows, lcp_raw, &lcp));
        const uint32_t head = (uint32_t)vec_head(lcp, tile);                // (the same in every tile)
        const uint64_t wt = (rows + tile - 1) >> tile_log2, t0 = ws >> tile_log2;
        PFP_LAUNCH(c, K_THR_TILES, rows * sizeof(T), (k_thr_tile_min<T>), wave_grid(wt, THR_LONG_WG), (const T *)lcp, rows, head, tile_log2, wt, tmin + t0, trow + t0, ws);
        const uint64_t ka = first[(size_t)w], kb = first[(size_t)w + 1];
        if (kb > ka) {
            PFP_HIP(c, hipMemsetAsync(d_out + 4, 0, 8, c->stream));
            PFP_LAUNCH(c, K_THR_QUERIES, (kb - ka) * (16 + 8 * sizeof(T)), (k_thr_win_queries<T>), nblocks(kb - ka, BLOCK), (const uint32_t *)sk, (const uint32_t *)sv, (const uint32_t *)pos, (const T *)c->d_ssa, (const T *)lcp, ws, we, ka, kb,
                       r, nrows, (uint64_t)c->tun.thr_long_min, tile_log2, thr, tlcp, queue, qcap, d_out);
            const uint64_t jobs = 2 * (kb - ka) < qcap ? 2 * (kb - ka) : qcap;      // queue entries of this window at most
            PFP_LAUNCH(c, K_THR_LONG, 0, (k_thr_win_long<T>), wave_grid(jobs, THR_LONG_WG), (const T *)lcp, ws, we, tile_log2, (const ThrLong *)queue, qcap, thr, tlcp, (const unsigned long long *)d_out);
        }
        ++seen;
        return PFP_OK;
    }));
    if (seen != nwin) return PFP_E_CORRUPT;
    // the whole tiles inside the gaps
    PFP_HIP(c, hipMemsetAsync(d_out + 4, 0, 8, c->stream));
    PFP_LAUNCH(c, K_THR_QUERIES, r * (8 + 4 * sizeof(T)), (k_thr_fold_queries<T>), nblocks(r, BLOCK), (const uint32_t *)sk, (const uint32_t *)sv, (const T *)c->d_ssa, (const T *)tmin, (const T *)trow, r, nrows, tile_log2,
               thr, tlcp, queue, qcap, d_out);
    PFP_LAUNCH(c, K_THR_LONG, 0, (k_thr_fold_long<T>), qgrid, (const T *)tmin, (const T *)trow, (const ThrLong *)queue, qcap, thr, tlcp, (const unsigned long long *)d_out);
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    if (windows) *windows = nwin;
    return tp.finish(h, info);
}

int pfp_lcp_array(pfp_ctx *c, unsigned what, pfp_lcp_info *info)
{
    if (!c || !what || (what & ~(unsigned)(PFP_LCP_ROWS | PFP_LCP_RUNS))) return PFP_E_ARG;
    if (!has_build(c) || !holds_build_text(c)) return PFP_E_STATE;
    if ((what & PFP_LCP_ROWS) && !has_whole_sa(c)) return PFP_E_STATE;
    if ((what & PFP_LCP_RUNS) && !has_run_samples(c)) return PFP_E_STATE;
    return post_entry(c, [&](auto t) { return lcp_array_impl<decltype(t)>(c, what, info); });
}
int pfp_lcp_array_get(pfp_ctx *c, void *lcp, void *slcp)
{
    if (!c) return PFP_E_ARG;
    void *const dst[2] = {lcp, slcp};
    return family_get(c, lcp_family(c), dst);
}
int pfp_lcp_array_device_ptrs(pfp_ctx *c, const void **d_lcp, const void **d_slcp)
{
    if (!c) return PFP_E_ARG;
    const void **const out[2] = {d_lcp, d_slcp};
    return family_device_ptrs(lcp_family(c), out);
}
int pfp_lcp_array_write(pfp_ctx *c, int fd_lcp, int fd_slcp)
{
    if (!c) return PFP_E_ARG;
    const int fd[2] = {fd_lcp, fd_slcp};
    return family_write(c, lcp_family(c), fd);
}

int pfp_thresholds(pfp_ctx *c, pfp_thr_info *info)
{
    if (!c) return PFP_E_ARG;
    if (!has_build(c) || !holds_build_text(c)) return PFP_E_STATE;
    if (!has_whole_sa(c) || !has_run_samples(c) || !c->runs) return PFP_E_STATE;
    if (c->runs > 0xFFFFFFFFULL) return PFP_E_TOO_LARGE;                                       // (run indices are sorted as 32-bit values)
    return post_entry(c, [&](auto t) { return thresholds_impl<decltype(t)>(c, info); });
}
// what both windowed routes need: a build over the whole output with run samples in a context that still holds its text
static int windowed_state(pfp_ctx *c)
{
    if (!has_build(c) || !holds_build_text(c)) return PFP_E_STATE;
    if (c->slice_rows != c->nout || c->slice_begin) return PFP_E_STATE;                        // a slice
    if (!has_run_samples(c) || !c->runs || !c->d_bwsai) return PFP_E_STATE;
    if (c->runs > 0xFFFFFFFFULL) return PFP_E_TOO_LARGE;                                       // (run indices are sorted as 32-bit values)
    return PFP_OK;
}
int pfp_thresholds_windowed(pfp_ctx *c, uint64_t window_rows, pfp_thr_info *info, uint64_t *windows)
{
    if (!c) return PFP_E_ARG;
    PFP_TRY(windowed_state(c));
    return post_entry(c, [&](auto t) { return thresholds_windowed_impl<decltype(t)>(c, window_rows, info, windows); });
}
int pfp_debug_rows_windowed(pfp_ctx *c, uint64_t window_rows, void *host_sa, void *host_lcp)
{
    if (!c || !window_rows) return PFP_E_ARG;
    PFP_TRY(windowed_state(c));
    return post_entry(c, [&](auto t) { return rows_windowed_impl<decltype(t)>(c, window_rows, host_sa, host_lcp); });
}
int pfp_thresholds_get(pfp_ctx *c, void *thr, void *tlcp)
{
    if (!c) return PFP_E_ARG;
    void *const dst[2] = {thr, tlcp};
    return family_get(c, thr_family(c), dst);
}
int pfp_thresholds_device_ptrs(pfp_ctx *c, const void **d_thr, const void **d_tlcp)
{
    if (!c) return PFP_E_ARG;
    const void **const out[2] = {d_thr, d_tlcp};
    return family_device_ptrs(thr_family(c), out);
}
int pfp_thresholds_write(pfp_ctx *c, int fd_thr, int fd_tlcp)
{
    if (!c) return PFP_E_ARG;
    const int fd[2] = {fd_thr, fd_tlcp};
    return family_write(c, thr_family(c), fd);
}
