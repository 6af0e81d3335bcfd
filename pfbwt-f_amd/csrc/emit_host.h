// pfbwt-f_amd/csrc/emit_host.h -- host side of stage 3 (pfp_bwt_build*): the emission pre-pass (per-word and per-slot tables), the
// slot stage (row counts, groups, tile index, list of the special slots), the emission of the rows window by window with the run
// samples, the SA-window visitor of the post-passes, the entries, and the ways out of a build: to host memory (pfp_bwt_get, pfp_bwt_get_expanded) and
// to file descriptors (write_device_to_fd, pfp_bwt_write).  The kernels are in emit.h.
// Host code only (but for three small kernels); included by pfbwt_hip.hip behind feed_host.h (ensure_copy_stream, host_pointer_is_pinned, the ring of ingest.h).
#pragma once
#include <thread>
#if defined(__SSE2__)
#include <emmintrin.h>
#endif

__global__ __launch_bounds__(BLOCK) void k_flag_special(const uint8_t *s_fl, uint64_t dsize, uint32_t *flag)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < dsize) flag[i] = slot_is_special(s_fl[i]) ? 1u : 0u;
}
template <typename EBT> __global__ __launch_bounds__(BLOCK) void k_gather_counts(const EBT *cnt, const uint32_t *list, uint64_t n, EBT *out)
{
    const uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j < n) out[j] = cnt[list[j]];
}

// visit != nullptr (visit_sa_windows; want_sa, the whole output): nothing is published -- every window of visit->window_rows rows is
// emitted into scratch at the high end of the arena and its SA values are handed to visit->fn; no field of the context changes.
struct EmitVisit { uint64_t window_rows; std::function<int(uint64_t first_row, uint64_t rows, const void *d_sa_window)> fn; };
// a window: rows [cs - cl, ce) are written, [e0, e1) (all rows) resp. [q0, q1) (special rows, those of the special slots [j0, j1)) are enumerated for them
struct EmitWin { uint64_t cs, ce, cl, e0, e1, q0, q1, j0, j1; };
// first row of slice `slice` of `nslices` equal slices of `total` rows (slice == nslices: total)
static uint64_t slice_first_row(uint64_t total, int slice, int nslices)
{
    const uint64_t k = (uint64_t)nslices, s = (uint64_t)slice;
    return total / k * s + (total % k) * s / k;
}
static void print_left_rows(const unsigned long long *d_gstat)
{
    unsigned long long h[12];
    if (hipMemcpy(h, d_gstat, 96, hipMemcpyDeviceToHost) != hipSuccess) return;
    fprintf(stderr, "[pfbwt_hip] special rows left to the row-wise kernel (counted once per window that enumerates them): whole-word member %llu, sort route %llu, too many rows %llu, too many slots %llu; by group rows (<1K <4K <16K <64K <256K <1M <4M more):",
            h[0], h[1], h[2], h[3]);
    for (int b = 0; b < 8; ++b) fprintf(stderr, " %llu", h[4 + b]);
    fprintf(stderr, "\n");
}

// Emission of the rows [s0, s1) of this slice (all rows when nslices == 1), in windows of at most `chunk_rows` rows so
// that the per-window scratch (parse rows of the enumerated rows, run counts) stays bounded for texts of tens of
// Gbases.  run() plans the windows, allocates the scratch of the routes and takes one of three drivers.
template <typename SAT, typename EBT> struct Emission {
    pfp_ctx *const c; EmitArgs ea; const bool want_rssa; const uint64_t tot2 /*rows of the special slots*/; const EmitVisit *const visit;
    const uint64_t total, s0, s1;
    const uint64_t lead;                                  // the row in front of the slice (run detection needs its BWT byte)
    const uint64_t nrows, chunk_rows, nchunks;
    const bool windowed, runaware;
    const bool keep_sa;                                   // a full SA array for this slice lives in the arena
    uint8_t *bwtbuf = nullptr; SAT *sabuf = nullptr; unsigned long long *d_b = nullptr;
    std::vector<EmitWin> wins; uint64_t maxq = 0, maxrows = 0;
    uint64_t *bk0 = nullptr, *bk1 = nullptr; uint32_t *bv0 = nullptr, *bv1 = nullptr, *btg = nullptr;      // sort route
    uint32_t *tilecnt = nullptr, *tilebase = nullptr, *d_cnt = nullptr, *qtmp = nullptr; uint16_t *rmask = nullptr;      // sampling
    bool fill_masks = false;                              // k_fill stores the run masks of the windows (run_one_pass_samples)
    std::vector<hipEvent_t> wev;                          // stream_out

    Emission(pfp_ctx *c_, const EmitArgs &ea_, bool want_sa, bool want_rssa_, int slice, int nslices, uint64_t tot2_, const EmitVisit *visit_)
        : c(c_), ea(ea_), want_rssa(want_rssa_), tot2(tot2_), visit(visit_), total(ea_.nout), s0(slice_first_row(total, slice, nslices)), s1(slice_first_row(total, slice + 1, nslices)),
          lead(s0 ? 1 : 0), nrows(s1 - s0), chunk_rows(visit_ ? visit_->window_rows : c_->tun.emit_chunk_rows ? c_->tun.emit_chunk_rows : (3ULL << 30)), nchunks((nrows + chunk_rows - 1) / chunk_rows),
          windowed(nslices > 1 || nchunks > 1), runaware(ea_.special != 0), keep_sa(want_sa && !visit_) {}
    ~Emission() { for (auto e : wev) (void)hipEventDestroy(e); }

    int run()
    {
        PFP_TRY(place_outputs());
        PFP_TRY(plan_windows());
        PFP_TRY(alloc_routes());
        struct LeftRows { const EmitArgs &ea; ~LeftRows() { if (ea.gstat) print_left_rows(ea.gstat); } } left_rows{ea};      // verbose; on the error paths too
        if (visit) return run_visit();
        if (!want_rssa || keep_sa) return run_bwt_then_exact_samples(false);
        bool overflow = false;
        PFP_TRY(run_one_pass_samples(&overflow));
        return overflow ? run_bwt_then_exact_samples(true) : PFP_OK;
    }

    // the byte of output row o lives at (bwtbuf - (s0 - lead)) + o, and that address is congruent to o modulo 16 (k_fill stores 16 aligned rows at a time)
    int place_outputs()
    {
        if (!visit) { c->slice_begin = s0; c->slice_rows = nrows; }
        uint8_t *bwtraw = nullptr;
        if (!visit) PFP_ALLOC_LO(c, bwtraw, uint8_t, nrows + lead + 48);
        bwtbuf = bwtraw + ((s0 - lead) & 15);
        if (keep_sa) PFP_ALLOC_LO(c, sabuf, SAT, nrows + lead);
        if (!visit) { c->d_bwt = bwtbuf + lead; c->d_sa = sabuf ? sabuf + lead : nullptr; c->d_ssa = c->d_esa = nullptr; }
        PFP_ALLOC_HI(c, d_b, unsigned long long, 6);
        return PFP_OK;
    }
    uint8_t *bwt_of(const EmitWin &wn) const { return bwtbuf + (wn.cs - wn.cl - (s0 - lead)); }      // position cs - cl
    SAT *sa_of(const EmitWin &wn) const { return sabuf ? sabuf + (wn.cs - wn.cl - (s0 - lead)) : (SAT *)nullptr; }

    // Rows of a group of equal suffixes that straddles a window boundary are enumerated for both windows.
    int plan_windows()
    {
        wins.resize((size_t)nchunks);
        for (uint64_t ch = 0; ch < nchunks; ++ch) {
            EmitWin &wn = wins[(size_t)ch];
            wn.cs = s0 + ch * chunk_rows; wn.ce = (wn.cs + chunk_rows < s1) ? wn.cs + chunk_rows : s1; wn.cl = wn.cs ? 1 : 0;
            wn.e0 = 0; wn.e1 = total; wn.q0 = 0; wn.q1 = tot2; wn.j0 = 0; wn.j1 = runaware ? ea.ecount : 0;
        }
        if (windowed) {
            unsigned long long *d_bounds; PFP_ALLOC_HI(c, d_bounds, unsigned long long, 6 * nchunks);
            for (uint64_t ch = 0; ch < nchunks; ++ch)
                PFP_LAUNCH(c, K_MISC, 64, (k_slice_bounds<EBT>), 1, ea, wins[(size_t)ch].cs - wins[(size_t)ch].cl, wins[(size_t)ch].ce, d_bounds + 6 * ch);
            std::vector<unsigned long long> hb(6 * (size_t)nchunks);
            PFP_HIP(c, hipMemcpyAsync(hb.data(), d_bounds, hb.size() * 8, hipMemcpyDeviceToHost, c->stream));
            PFP_HIP(c, hipStreamSynchronize(c->stream));
            for (uint64_t ch = 0; ch < nchunks; ++ch) { EmitWin &wn = wins[(size_t)ch]; const unsigned long long *b = &hb[6 * (size_t)ch]; wn.e0 = b[0]; wn.e1 = b[1]; wn.q0 = b[2]; wn.q1 = b[3]; wn.j0 = b[4]; wn.j1 = b[5]; }
        }
        for (const EmitWin &wn : wins) { if (wn.q1 - wn.q0 > maxq) maxq = wn.q1 - wn.q0; if (wn.ce - wn.cs > maxrows) maxrows = wn.ce - wn.cs; }
        return PFP_OK;
    }

    // scratch of the routes that a window's rows can take besides the row-wise kernel (allocation order matters: high end of the arena)
    int alloc_routes()
    {
        // list of the rows of many-member groups (sorted per window instead of ranked row by row)
        if (ea.big_total) {
            if (ea.big_total >= 0xFFFFFFF0ULL) return PFP_E_TOO_LARGE;
            PFP_ALLOC_HI(c, bk0, uint64_t, ea.big_total); PFP_ALLOC_HI(c, bk1, uint64_t, ea.big_total);
            PFP_ALLOC_HI(c, bv0, uint32_t, ea.big_total); PFP_ALLOC_HI(c, bv1, uint32_t, ea.big_total); PFP_ALLOC_HI(c, btg, uint32_t, ea.big_total);
        }
        ea.big_keys = bk0; ea.big_vals = bv0; ea.big_count = d_b + 4; ea.big_cap = ea.big_total;
        // group-stationary route of the special rows (k_emit_groups); what it leaves behind is marked for k_emit
        ea.group_rows_cap = c->tun.emit_group_rows; ea.rank_members_max = c->tun.big_group_members != -2 ? 0xFFFFFFFFu : c->tun.emit_group_rows >= (uint32_t)EG_BUF ? BIG_GROUP_MEMBERS : 3u;      // (tests with small batches: groups of more than three members through the LDS sort)
        const uint64_t max_etiles = maxq / EMIT_TILE + 3;
        if (runaware && ea.group_rows_cap && tot2 && ea.cinfo) {
            PFP_ALLOC_HI(c, ea.gleft, uint8_t, (size_t)ea.ecount + 1); PFP_ALLOC_HI(c, ea.tile_left, uint8_t, max_etiles);
            PFP_HIP(c, hipMemsetAsync(ea.gleft, 0, (size_t)ea.ecount + 1, c->stream));      // which groups are left is a property of the build, not of a window
        }
        ea.qpasses = (bits_for(c->nrows ? c->nrows : 0xFFFFFFFFULL) + 7) / 8;
        if (ea.gleft) {
            const uint32_t cap = ea.group_rows_cap < (uint32_t)EG_BUF ? ea.group_rows_cap : (uint32_t)EG_BUF;
            ea.lgcap = maxq / cap + 2;
            PFP_ALLOC_HI(c, ea.lglist, uint32_t, 2 * ea.lgcap); PFP_ALLOC_HI(c, ea.lgcount, unsigned long long, 2);
            if (!c->d_lgtaken) PFP_HIP(c, hipMalloc((void **)&c->d_lgtaken, 16));      // outlives the arena's scratch: pfp_debug_emit_large_groups reads it after the build
            PFP_HIP(c, hipMemsetAsync(c->d_lgtaken, 0, 16, c->stream));
            ea.lgtaken = c->d_lgtaken;
        }
        if (ea.gleft && c->tun.verbose) { PFP_ALLOC_HI(c, ea.gstat, unsigned long long, 12); PFP_HIP(c, hipMemsetAsync(ea.gstat, 0, 96, c->stream)); }
        return PFP_OK;
    }

    // emits the rows whose output position lies in [cs - cl, ce); bwt_at / sa_at point at that first position; q_at receives
    // the parse row of every row written (all rows) resp. of every special row enumerated (run-aware)
    int emit_window(const EmitWin &wn, uint8_t *bwt_at, SAT *sa_at, uint32_t *q_at, bool fill)
    {
        ea.w0 = wn.cs - wn.cl; ea.w1 = wn.ce;
        if (ea.big_total) PFP_HIP(c, hipMemsetAsync(ea.big_count, 0, 16, c->stream));
        if (runaware) PFP_TRY(emit_runaware(wn, bwt_at, q_at, fill));
        else PFP_TRY(emit_all_rows(wn, bwt_at, sa_at, q_at));
        return ea.big_total ? place_big_groups(bwt_at, sa_at, q_at) : PFP_OK;
    }
    // ea.special != 0 (no full SA wanted): run-aware emission -- k_fill writes every row as a run of its slot's preceding
    // byte, k_emit walks only the rows of the special slots (tot2 of them), samples look their parse rows up.
    int emit_runaware(const EmitWin &wn, uint8_t *bwt_at, uint32_t *q_at, bool fill)
    {
        ea.e0 = wn.q0; ea.e1 = wn.q1; ea.q0 = wn.q0;
        if (fill) {
            const uint32_t fill_subs = c->tun.fill_subs < 1u ? 1u : c->tun.fill_subs > FILL_MAX_SUBS ? FILL_MAX_SUBS : c->tun.fill_subs;     // super-tiles (4 x 4096 rows) per workgroup
            const uint64_t super = (uint64_t)FILL_GROUPS * FILL_SUB;
            const uint64_t nsub = (ea.w1 - 1) / super - ea.w0 / super + 1;
            const int skip = c->tun.fill_skip ? 1 : 0;
            if (fill_masks) PFP_LAUNCH(c, K_FILL, (ea.w1 - ea.w0) * 9 / 8, (k_fill<EBT, true>), nblocks(nsub, fill_subs), ea, bwt_at, fill_subs, skip, rmask, wn.cs);
            else PFP_LAUNCH(c, K_FILL, ea.w1 - ea.w0, (k_fill<EBT, false>), nblocks(nsub, fill_subs), ea, bwt_at, fill_subs, skip, (uint16_t *)nullptr, (uint64_t)0);
        }
        if (ea.e1 <= ea.e0) return PFP_OK;
        const unsigned ge = (unsigned)((ea.e1 - 1) / EMIT_TILE - ea.e0 / EMIT_TILE + 1);
        if (ea.gleft) {
            PFP_HIP(c, hipMemsetAsync(ea.tile_left, 0, (size_t)ge, c->stream));
            PFP_HIP(c, hipMemsetAsync(ea.lgcount, 0, 16, c->stream));
            PFP_LAUNCH(c, K_EMIT, (ea.e1 - ea.e0) * (1 + 4 + (q_at ? 4 : 0)), (k_emit_groups<EBT>), ge, ea, bwt_at, q_at);
            // the groups too long for a batch, one per workgroup turn: two rounds of the workgroups that are resident at a time
            const unsigned cus = c->num_cus > 0 ? (unsigned)c->num_cus : 256u;
            const unsigned cap1 = 2u * EGL1_WG_PER_CU * cus, cap2 = 2u * EGL2_WG_PER_CU * cus;
            PFP_LAUNCH_B(c, K_EMIT_LARGE, 0, (k_emit_groups_large<EBT, EG1_BUF, EGL1_THREADS>), ge < cap1 ? ge : cap1, EGL1_THREADS, ea, bwt_at, q_at);
            PFP_LAUNCH_B(c, K_EMIT_LARGE, 0, (k_emit_groups_large<EBT, EG2_BUF, EGL2_THREADS>), ge < cap2 ? ge : cap2, EGL2_THREADS, ea, bwt_at, q_at);
            PFP_LAUNCH(c, K_EMIT_BIG, 0, (k_emit<SAT, EBT>), ge, ea, bwt_at, (SAT *)nullptr, q_at);      // the groups left over (workgroups of other tiles return at once)
        } else
            PFP_LAUNCH(c, K_EMIT, (ea.e1 - ea.e0) * (1 + 4 + (q_at ? 4 : 0)), (k_emit<SAT, EBT>), ge, ea, bwt_at, (SAT *)nullptr, q_at);
        return PFP_OK;
    }
    int emit_all_rows(const EmitWin &wn, uint8_t *bwt_at, SAT *sa_at, uint32_t *q_at)
    {
        ea.e0 = wn.e0; ea.e1 = wn.e1; ea.q0 = 0;
        PFP_LAUNCH(c, K_EMIT, (ea.w1 - ea.w0) * (1 + 4 + (sa_at ? 8 + sizeof(SAT) : 0) + (q_at ? 4 : 0)),   // per row: BWT byte out, ilist entry in, (bwsai gather + SA out | parse row out)
                   (k_emit<SAT, EBT>), (unsigned)((ea.e1 - 1) / EMIT_TILE - ea.e0 / EMIT_TILE + 1), ea, bwt_at, sa_at, q_at);
        return PFP_OK;
    }
    // the rows that the kernels of this window put on the list of the many-member groups: sorted by (group, parse row), then placed
    int place_big_groups(uint8_t *bwt_at, SAT *sa_at, uint32_t *q_at)
    {
        unsigned long long hb[2];
        PFP_HIP(c, hipMemcpyAsync(hb, ea.big_count, 16, hipMemcpyDeviceToHost, c->stream));
        PFP_HIP(c, hipStreamSynchronize(c->stream));
        if (hb[1] || hb[0] > ea.big_total) return PFP_E_CORRUPT;
        const uint64_t nb = hb[0];
        if (!nb) return PFP_OK;
        const BitRange big_ranges[2] = {{0, bits_for(c->nrows)}, {32, 32 + bits_for(ea.dsize)}};
        uint64_t *sk; uint32_t *sv;
        PFP_TRY(radix_sort_pairs<uint64_t>(c, bk0, bv0, bk1, bv1, nb, big_ranges, 2, &sk, &sv));
        PFP_LAUNCH(c, K_EMIT_BIG, nb * 12, k_big_heads, nblocks(nb, BLOCK), (const uint64_t *)sk, nb, btg);
        PFP_TRY((device_scan<uint32_t, 1>(c, btg, btg, nb, nullptr)));
        PFP_LAUNCH(c, K_EMIT_BIG, nb * (30 + sizeof(SAT)), (k_big_place<SAT, EBT>), nblocks(nb, BLOCK), ea, (const uint64_t *)sk, (const uint32_t *)sv, (const uint32_t *)btg, nb, bwt_at, sa_at, q_at);
        return PFP_OK;
    }

    // pfp_bwt_build_stream: the rows of a finished window start their way to the host while the next window is emitted.  Window k + 1
    // WRITES row cs - 1, the last row of window k, once more (k_fill puts a slot's placeholder byte there before k_emit_groups / k_emit
    // restore the true one; run detection needs that row): a copy of window k that included it could deliver the placeholder.
    // So every window sends its rows shifted by one -- [cs - cl, ce - 1), the last window up to ce -- and no row is in flight while a
    // later window's kernels can still store to it.  (The row in front of a slice belongs to the neighbouring slice's buffers.)
    int stream_out(const EmitWin &wn)
    {
        if (!c->h_bwt && !c->h_sa) return PFP_OK;
        const uint64_t r0 = wn.cs - wn.cl < s0 ? s0 : wn.cs - wn.cl, r1 = wn.ce == s1 ? wn.ce : wn.ce - 1;
        if (r1 <= r0) return PFP_OK;
        hipEvent_t e; PFP_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming)); wev.push_back(e);      // destroyed with the emission
        PFP_HIP(c, hipEventRecord(e, c->stream));
        PFP_HIP(c, hipStreamWaitEvent(c->fa.copy, e, 0));
        const uint64_t rows = r1 - r0;
        if (c->h_bwt) PFP_HIP(c, hipMemcpyAsync(c->h_bwt + (r0 - s0), bwtbuf + (r0 - (s0 - lead)), (size_t)rows, hipMemcpyDeviceToHost, c->fa.copy));
        if (c->h_sa && sabuf) PFP_HIP(c, hipMemcpyAsync((char *)c->h_sa + (r0 - s0) * sizeof(SAT), sabuf + (r0 - (s0 - lead)), (size_t)rows * sizeof(SAT), hipMemcpyDeviceToHost, c->fa.copy));
        return PFP_OK;
    }

    // Run samples of one window, in two steps with the route's own check of the count between them.
    // with_q: the samples take the parse rows of a window from qtmp (no full SA array to read them from)
    int alloc_sample_scratch(bool with_q)
    {
        const uint64_t maxtiles = nblocks(maxrows, RUN_TILE);
        PFP_ALLOC_HI(c, tilecnt, uint32_t, maxtiles); PFP_ALLOC_HI(c, tilebase, uint32_t, maxtiles); PFP_ALLOC_HI(c, d_cnt, uint32_t, 1);
        PFP_ALLOC_HI(c, rmask, uint16_t, maxtiles * BLOCK);
        qtmp = nullptr;
        if (with_q) PFP_ALLOC_HI(c, qtmp, uint32_t, (runaware ? maxq : maxrows) + 1);     // parse rows kept per window
        ea.qspec = qtmp;
        return PFP_OK;
    }
    // *rc: the runs that start in the rows [cs, ce) of the window, whose BWT bytes are written.  masks_filled: k_fill has stored the
    // window's run masks -- those that the final bytes of the special rows change are recomputed (1.3 G of S-32G's 32 G rows), and the
    // tile counts come from the masks; else one pass over the window's bytes makes both.
    int count_window_runs(const EmitWin &wn, uint32_t *rc, bool masks_filled)
    {
        const uint64_t rows = wn.ce - wn.cs, ntiles = nblocks(rows, RUN_TILE);
        const uint8_t *bytes = bwt_of(wn) + wn.cl;
        if (masks_filled) {
            const uint64_t nsp = wn.j1 > wn.j0 ? wn.j1 - wn.j0 : 0, nedge = 2 + (wn.ce - 1) / FILL_SUB - wn.cs / FILL_SUB;
            const unsigned nsb = nblocks(nsp, BLOCK);
            PFP_LAUNCH(c, K_RUN_MASKS, (wn.q1 - wn.q0) * 9 / 8 + nsp * 24, (k_run_masks_fix<EBT>), nsb + nblocks(nedge, BLOCK), ea, bytes, wn.cs, rows, (int)wn.cl, wn.j0, wn.j1, (uint32_t)nsb, rmask);
            PFP_LAUNCH(c, K_RUN_MASKS, rows / 8, k_mask_tile_count, nblocks(ntiles, MT_TILES), (const uint16_t *)rmask, rows, (uint64_t)ntiles, tilecnt);
        } else
            PFP_LAUNCH(c, K_RUNS, rows, k_run_tile_count, ntiles, bytes, rows, (int)wn.cl, tilecnt, rmask);
        PFP_TRY((device_scan<uint32_t, 0>(c, tilecnt, tilebase, ntiles, d_cnt)));
        return d2h_u32(c, d_cnt, rc);
    }
    // the window's rc runs become the samples run_base .. run_base + rc of ssa / esa_w: the sampled rows (k_sample_rows), then their SA
    // values from sa_win (the window's SA values, first at row cs - cl) or else from the parse rows in qtmp (k_sample_values).
    // r_total: all runs of the slice, as far as the last window has to know them (the closing pair of the whole output)
    int sample_window(const EmitWin &wn, uint32_t rc, uint64_t run_base, uint64_t r_total, SAT *ssa, SAT *esa_w, const SAT *sa_win)
    {
        const uint64_t rows = wn.ce - wn.cs, ntiles = nblocks(rows, RUN_TILE);
        const bool last = wn.ce == total;
        PFP_LAUNCH(c, K_SAMPLES, rows / 8 + (uint64_t)rc * 4 * sizeof(SAT), (k_sample_rows<SAT>), nblocks(ntiles, SR_TILES), (const uint16_t *)rmask, rows, (uint64_t)ntiles, (const uint32_t *)tilebase, wn.cs, run_base, total,
                   last ? r_total + 1 : (uint64_t)0, ssa, esa_w);
        PFP_LAUNCH(c, K_SAMPLES, (uint64_t)rc * (2 * 60 + 4 * sizeof(SAT)), (k_sample_values<SAT, EBT>), nblocks((uint64_t)rc + 1, BLOCK), ea, sa_win, (const uint32_t *)qtmp, wn.cs - wn.cl, (uint64_t)rc, run_base,
                   (int)last, last ? (uint64_t)(r_total - 1) : (uint64_t)0, ssa, esa_w);
        return PFP_OK;
    }
    void publish_run_count(uint64_t r) { c->runs = r; c->esa_pairs = r - (s0 == 0 ? 1 : 0) + (s1 == total ? 1 : 0); }

    // one window's BWT bytes and SA values (with the row in front of it) at a time; the consumer works on the context's stream, so
    // the next window's kernels wait for it
    int run_visit()
    {
        const uint64_t wrows = (chunk_rows < nrows ? chunk_rows : nrows) + 1;
        uint8_t *wbraw; SAT *wsa;
        PFP_ALLOC_HI(c, wbraw, uint8_t, wrows + 48); PFP_ALLOC_HI(c, wsa, SAT, wrows);
        for (const EmitWin &wn : wins) {
            PFP_TRY(emit_window(wn, wbraw + ((wn.cs - wn.cl) & 15), wsa, (uint32_t *)nullptr, false));
            PFP_TRY(visit->fn(wn.cs, wn.ce - wn.cs, (const void *)(wsa + wn.cl)));
        }
        return PFP_OK;
    }

    // Samples only: ONE pass per window -- emit the BWT bytes and the parse rows q needed for sampling into scratch, find
    // the run starts, compute SA values for the 2r sampled rows only (k_sample_rows, k_sample_values), forget the q's.  r is not known in
    // advance, so the sample arrays get a capacity from the free workspace.  *overflow: r exceeds it -- the BWT bytes are complete (the
    // windows behind the overflow are still emitted and streamed, and counted), the samples are to be redone with exact sizes.
    int run_one_pass_samples(bool *overflowed)
    {
        const size_t lo_mark = c->arena.mark_lo(), hi_mark = c->arena.mark_hi();
        PFP_TRY(alloc_sample_scratch(true));
        // run masks out of k_fill's registers instead of a second pass over the bytes: decided once, for windows whose pieces of 16 rows
        // are the pieces k_fill stores (every window start a multiple of 16)
        fill_masks = c->tun.fill_masks && runaware;
        for (const EmitWin &wn : wins) if (wn.cs % FILL_PER_THREAD) fill_masks = false;
        struct MasksOff { bool &f; ~MasksOff() { f = false; } } masks_off{fill_masks};      // the exact route that may follow fills nothing
        const bool masks_filled = fill_masks;
        const size_t freeb = c->arena.hi > c->arena.lo + ((size_t)256 << 20) ? c->arena.hi - c->arena.lo - ((size_t)256 << 20) : 0;
        uint64_t cap = freeb / (4 * sizeof(SAT));
        if (cap > nrows) cap = nrows;
        if (c->tun.sample_cap < cap) cap = c->tun.sample_cap;   // tests: force the fallback
        SAT *samp = nullptr;
        if (cap) { samp = (SAT *)c->arena.reserve_lo(sizeof(SAT) * (4 * cap + 4)); if (!samp) return PFP_E_NOMEM; }      // address space for the worst case; committed window by window
        SAT *ssa = samp, *esa = samp ? samp + 2 * cap : nullptr;
        SAT *esa_w = esa ? esa + 2 * lead : nullptr;      // slices > 0: the first run start of the slice closes a run of the previous slice
        uint64_t run_base = 0; bool overflow = cap == 0;
        for (const EmitWin &wn : wins) {
            PFP_TRY(emit_window(wn, bwt_of(wn), (SAT *)nullptr, qtmp, true));
            PFP_TRY(stream_out(wn));
            uint32_t rc = 0; PFP_TRY(count_window_runs(wn, &rc, masks_filled));
            if (!overflow && run_base + rc > cap) overflow = true;
            if (!overflow && !(c->arena.commit_range(ssa + 2 * run_base, sizeof(SAT) * (2 * (size_t)rc + 4)) && c->arena.commit_range(esa + 2 * run_base, sizeof(SAT) * (2 * (size_t)rc + 8)))) overflow = true;
            if (!overflow) PFP_TRY(sample_window(wn, rc, run_base, run_base + rc, ssa, esa_w, (const SAT *)nullptr));
            run_base += rc;
        }
        publish_run_count(run_base);
        c->arena.release_hi(hi_mark);
        *overflowed = overflow;
        if (overflow) { c->arena.release_lo(lo_mark); return PFP_OK; }
        c->d_ssa = ssa; c->d_esa = esa;
        c->arena.release_lo(c->arena.offset_of(esa) + sizeof(SAT) * (2 * (size_t)run_base + 8));      // what lies behind the run ends that were written is free again
        return PFP_OK;
    }

    // The exact route: the BWT bytes (and SA values if a full SA is kept) of every window, the number of runs, then -- if wanted -- the
    // samples into arrays of exactly that size.  bwt_done: the one-pass route has written the bytes and counted the runs already.
    int run_bwt_then_exact_samples(bool bwt_done)
    {
        if (!bwt_done) {
            for (const EmitWin &wn : wins) {
                PFP_TRY(emit_window(wn, bwt_of(wn), sa_of(wn), (uint32_t *)nullptr, true));
                PFP_TRY(stream_out(wn));
            }
            PFP_TRY(count_slice_runs());
        }
        return want_rssa ? exact_samples() : PFP_OK;
    }
    // runs (src/pfbwt-f.cpp:304-305): runs that start in this slice
    int count_slice_runs()
    {
        unsigned long long *d_runs = d_b + 2;
        PFP_HIP(c, hipMemsetAsync(d_runs, 0, 8, c->stream));
        PFP_LAUNCH(c, K_RUNS, nrows, k_run_count, nblocks(nrows, 16 * BLOCK), (const uint8_t *)c->d_bwt, nrows, (int)lead, d_runs);
        unsigned long long r = 0;
        PFP_HIP(c, hipMemcpyAsync(&r, d_runs, 8, hipMemcpyDeviceToHost, c->stream));
        PFP_HIP(c, hipStreamSynchronize(c->stream));
        publish_run_count(r);
        return PFP_OK;
    }
    // .ssa / .esa samples (pfbwt-f.cpp:306-315, 325-328) of the c->runs runs that start in this slice
    int exact_samples()
    {
        const uint64_t r = c->runs;
        if (sabuf) {      // with a full SA the samples need nothing of the per-slot arrays any more (~60 B per dictionary byte): on a
            PFP_HIP(c, hipStreamSynchronize(c->stream));      // non-repetitive genome (S-3G: r = 0.74 n) they and the samples do not fit together
            c->arena.release_hi(c->emit_scratch_mark);
        }
        SAT *ssa, *esa;
        PFP_ALLOC_LO(c, ssa, SAT, 2 * r + 2); PFP_ALLOC_LO(c, esa, SAT, 2 * r + 4);
        c->d_ssa = ssa; c->d_esa = esa;
        SAT *esa_w = esa + 2 * lead;
        PFP_TRY(alloc_sample_scratch(!sabuf));
        uint64_t run_base = 0;
        for (const EmitWin &wn : wins) {
            if (!sabuf) PFP_TRY(emit_window(wn, bwt_of(wn), (SAT *)nullptr, qtmp, false));   // pass 2 of this window: the same rows again, now with their q
            uint32_t rc = 0; PFP_TRY(count_window_runs(wn, &rc, false));
            if (run_base + rc > r) return PFP_E_CORRUPT;
            PFP_TRY(sample_window(wn, rc, run_base, r, ssa, esa_w, (const SAT *)sa_of(wn)));
            run_base += rc;
        }
        return run_base == r ? PFP_OK : PFP_E_CORRUPT;
    }
};

// Everything of stage 3 that depends on the width of the row counter (EBT = uint32_t while n + 1 < 2^32) and comes before the rows:
// per slot the rows it produces and its group of equal suffixes, the groups of the sort route, the tile index, the special slots.
template <typename EBT> struct SlotStage {
    pfp_ctx *const c; EmitArgs ea; const bool runaware; const uint64_t dsize;
    EBT *cnt = nullptr, *EB = nullptr, *d_tot = nullptr, *cnt2 = nullptr; unsigned long long *d_hard = nullptr;
    uint32_t *s_g0 = nullptr, *gk = nullptr, *gqf = nullptr, *gql = nullptr; uint8_t *gfl = nullptr, *gnu = nullptr;
    bool gq_done = false;                   // k_emit_slots has reduced gqf / gql
    EBT tot = 0;                            // output rows
    unsigned long long hh[2] = {0, 0};      // hard rows, rows of the sort route
    uint64_t tot2 = 0;                      // rows of the special slots

    int alloc_slot_arrays()
    {
        PFP_ALLOC_HI(c, cnt, EBT, dsize); PFP_ALLOC_HI(c, EB, EBT, dsize); PFP_ALLOC_HI(c, d_hard, unsigned long long, 2); PFP_ALLOC_HI(c, d_tot, EBT, 2);
        PFP_HIP(c, hipMemsetAsync(d_hard, 0, 16, c->stream));
        PFP_ALLOC_HI(c, s_g0, uint32_t, dsize); PFP_ALLOC_HI(c, gk, uint32_t, dsize); PFP_ALLOC_HI(c, gfl, uint8_t, dsize); PFP_ALLOC_HI(c, gnu, uint8_t, dsize);
        PFP_HIP(c, hipMemsetAsync(gfl, 0, dsize, c->stream));
        PFP_HIP(c, hipMemsetAsync(gnu, 0, dsize, c->stream));
        if (runaware) {
            PFP_ALLOC_HI(c, cnt2, EBT, dsize); PFP_ALLOC_HI(c, gqf, uint32_t, dsize); PFP_ALLOC_HI(c, gql, uint32_t, dsize);
            PFP_HIP(c, hipMemsetAsync(gqf, 0xFF, dsize * 4, c->stream));
            PFP_HIP(c, hipMemsetAsync(gql, 0, dsize * 4, c->stream));
        }
        ea.EB = EB; ea.s_g0 = s_g0; ea.gk = gk; ea.cnt = cnt; ea.gqf = gqf; ea.gql = gql;
        return PFP_OK;
    }
    // per dictionary offset, for k_emit_slots only: ONE 16-byte record (suffix lengths must fit 26 bits), else word id | preceding
    // byte + class head and a second gather of the word record.  The array lives only for that kernel: what is allocated behind
    // it (the 16-byte per-slot records of the row kernels) takes its place -- same stream, so the reuse is ordered
    int slot_prepass()
    {
        const size_t mkp = c->arena.mark_hi();
        if (ea.use_prec) {
            uint4 *prec; PFP_ALLOC_HI(c, prec, uint4, dsize);
            PFP_LAUNCH(c, K_EMIT_COUNT, dsize * 29, k_pack_prec, nblocks(dsize, BLOCK), ea.D, ea.wordid, ea.winfo, dsize, ea.dwords, prec, ea.use_e0 ? ea.bwsai_il : (const tpos_t *)nullptr);
            ea.prec = prec;
        } else {
            uint2 *posinfo; PFP_ALLOC_HI(c, posinfo, uint2, dsize);
            PFP_LAUNCH(c, K_EMIT_COUNT, dsize * 17, k_pack_posinfo, nblocks(dsize, BLOCK), ea.D, ea.wordid, dsize, posinfo);
            ea.posinfo = posinfo;
        }
        // run-aware: the first / last parse row of every group reduced by k_emit_slots from a per-word table (the word id rides in prec.x)
        uint2 *wpq = nullptr;
        if (runaware && c->tun.group_reduce && !ea.use_e0) {
            PFP_ALLOC_HI(c, wpq, uint2, ea.dwords);
            PFP_LAUNCH(c, K_EMIT_COUNT, (uint64_t)ea.dwords * 24, k_pack_wpq, nblocks(ea.dwords, BLOCK), ea.ilist, ea.wrank, ea.occ, ea.F, (uint64_t)ea.dwords, wpq);
        }
        PFP_LAUNCH(c, K_EMIT_COUNT, dsize * (30 + sizeof(EBT)) + (wpq ? dsize * 8 : 0), (k_emit_slots<EBT>), nblocks(dsize, BLOCK), ea, cnt, d_hard, (uint32_t *)ea.s_sl, (uint32_t *)ea.s_fb, (uint8_t *)ea.s_fl, (uint8_t *)ea.s_pc, s_g0, gk, gfl, gnu,
                   (const uint2 *)wpq, gqf, gql);
        if (wpq) gq_done = true;
        c->arena.release_hi(mkp);
        ea.prec = nullptr; ea.posinfo = nullptr;
        return PFP_OK;
    }
    // first output row of every slot, the groups of the sort route (SF_BIG), the per-slot records of the row kernels
    int mark_big_groups()
    {
        uint4 *sinfo; PFP_ALLOC_HI(c, sinfo, uint4, dsize); ea.sinfo = sinfo;
        const long big_members = c->tun.big_group_members == -2 ? (long)BIG_GROUP_MEMBERS : c->tun.big_group_members;   // < 0: never
        PFP_TRY((device_scan<EBT, 0>(c, cnt, EB, dsize, d_tot)));
        // run-aware: a group of more rows than k_emit_groups_large holds in LDS takes the sort route too (S-32G: 1.4 M rows in groups of 16-64 K
        // rows and ~100 members were ranked row by row in memory by k_emit: 9 ms)
        const uint32_t big_rows = !(runaware && big_members >= 0 && c->tun.emit_group_rows) ? 0u : c->tun.emit_group_rows >= (uint32_t)EG_BUF ? (uint32_t)EG2_BUF : 4u * c->tun.emit_group_rows;      // (tests: small batches -> small limit)
        PFP_LAUNCH(c, K_EMIT_COUNT, dsize * 14, (k_big_mark<EBT>), nblocks(dsize, BLOCK), (const EBT *)cnt, (const uint32_t *)s_g0, (const uint32_t *)gk, (const uint8_t *)gfl, (const uint8_t *)gnu, (const uint32_t *)ea.s_fb, ea.ilist, dsize,
                   big_members >= 0 ? (uint32_t)big_members : 0xFFFFFFFFu, runaware ? 1 : 0, (uint8_t *)ea.s_fl, sinfo, cnt2, gq_done ? nullptr : gqf, gq_done ? nullptr : gql, d_hard + 1, (const EBT *)EB, (const EBT *)d_tot, big_rows, (big_rows && c->tun.big_group_members == -2) ? 1 : 0);
        PFP_HIP(c, hipMemcpyAsync(hh, d_hard, 16, hipMemcpyDeviceToHost, c->stream));
        PFP_HIP(c, hipMemcpyAsync(&tot, d_tot, sizeof(EBT), hipMemcpyDeviceToHost, c->stream));
        PFP_HIP(c, hipStreamSynchronize(c->stream));
        ea.big_total = hh[1];
        return PFP_OK;
    }
    // slot under every EMIT_TILE-th output row (k_emit, k_fill, k_sample_values, k_slice_bounds start their searches there)
    int build_tile_index()
    {
        const uint64_t ntiles = ((uint64_t)tot + EMIT_TILE - 1) / EMIT_TILE;
        uint32_t *tile_slot; PFP_ALLOC_HI(c, tile_slot, uint32_t, ntiles + 1);
        PFP_LAUNCH(c, K_EMIT_COUNT, dsize * 2 * sizeof(EBT) + ntiles * 4, (k_tile_slots<EBT>), nblocks(dsize, BLOCK), (const EBT *)cnt, (const EBT *)EB, dsize, ntiles, tile_slot);
        ea.tile_slot = tile_slot;
        // enumeration order of k_emit: every row, unless build_special_list replaces it
        ea.ENB = EB; ea.etile_slot = tile_slot; ea.ecount = (uint32_t)dsize;
        return PFP_OK;
    }
    // run-aware enumeration order of k_emit: the rows of the special slots through a compacted list of them
    int build_special_list()
    {
        uint32_t *flag, *cpos, *spl, *d_cnt;
        PFP_ALLOC_HI(c, flag, uint32_t, dsize); PFP_ALLOC_HI(c, cpos, uint32_t, dsize + 1); PFP_ALLOC_HI(c, d_cnt, uint32_t, 1);
        PFP_LAUNCH(c, K_EMIT_COUNT, dsize * 5, k_flag_special, nblocks(dsize, BLOCK), (const uint8_t *)ea.s_fl, dsize, flag);
        PFP_TRY((device_scan<uint32_t, 0>(c, flag, cpos, dsize, d_cnt)));
        uint32_t nsp = 0; PFP_TRY(d2h_u32(c, d_cnt, &nsp));
        PFP_ALLOC_HI(c, spl, uint32_t, (size_t)nsp + 1);
        if (nsp) PFP_LAUNCH(c, K_COMPACT, dsize * 12, k_compact_scatter, nblocks(dsize, BLOCK), (const uint32_t *)nullptr, (const uint32_t *)flag, (const uint32_t *)cpos, dsize, spl);
        EBT *cntc, *ENBc;
        PFP_ALLOC_HI(c, cntc, EBT, (size_t)nsp + 1); PFP_ALLOC_HI(c, ENBc, EBT, (size_t)nsp + 1);
        uint64_t ntiles2 = 0;
        if (nsp) {
            PFP_LAUNCH(c, K_EMIT_COUNT, (uint64_t)nsp * (4 + 2 * sizeof(EBT)), (k_gather_counts<EBT>), nblocks(nsp, BLOCK), (const EBT *)cnt, (const uint32_t *)spl, (uint64_t)nsp, cntc);
            PFP_TRY((device_scan<EBT, 0>(c, cntc, ENBc, nsp, ENBc + nsp)));
            EBT t2 = 0;
            PFP_HIP(c, hipMemcpyAsync(&t2, ENBc + nsp, sizeof(EBT), hipMemcpyDeviceToHost, c->stream));
            PFP_HIP(c, hipStreamSynchronize(c->stream));
            tot2 = (uint64_t)t2;
            ntiles2 = (tot2 + EMIT_TILE - 1) / EMIT_TILE;
            uint32_t *et; PFP_ALLOC_HI(c, et, uint32_t, ntiles2 + 1);
            PFP_LAUNCH(c, K_EMIT_COUNT, (uint64_t)nsp * 2 * sizeof(EBT) + ntiles2 * 4, (k_tile_slots<EBT>), nblocks(nsp, BLOCK), (const EBT *)cntc, (const EBT *)ENBc, (uint64_t)nsp, ntiles2, et);
            ea.etile_slot = et;
        } else PFP_HIP(c, hipMemsetAsync(ENBc, 0, sizeof(EBT), c->stream));
        ea.ENB = ENBc; ea.elist = spl; ea.cpos = cpos; ea.ecount = nsp; ea.special = 1;
        if (nsp && c->tun.emit_group_rows) {      // per special slot / per enumeration tile: what k_emit_groups would otherwise chase through three arrays per batch
            uint4 *cinfo; unsigned long long *cgb; uint32_t *town;
            PFP_ALLOC_HI(c, cinfo, uint4, nsp); PFP_ALLOC_HI(c, cgb, unsigned long long, nsp); PFP_ALLOC_HI(c, town, uint32_t, ntiles2 + 1);
            PFP_LAUNCH(c, K_EMIT_COUNT, (uint64_t)nsp * 50, (k_special_pack<EBT>), nblocks(nsp, BLOCK), ea, nsp, cinfo, cgb);
            PFP_LAUNCH(c, K_EMIT_COUNT, (ntiles2 + 1) * 40, (k_tile_own<EBT>), nblocks(ntiles2 + 1, BLOCK), (const EBT *)ENBc, (const uint4 *)cinfo, (const uint32_t *)ea.etile_slot, (uint64_t)nsp, ntiles2, town);
            ea.cinfo = cinfo; ea.cgb = cgb; ea.town = town;
        }
        return PFP_OK;
    }
    // verbose: the histogram of the rows by members and rows of their group
    int print_group_stats()
    {
        unsigned long long *d_hist, hist[64]; PFP_ALLOC_HI(c, d_hist, unsigned long long, 64);
        PFP_HIP(c, hipMemsetAsync(d_hist, 0, 512, c->stream));
        PFP_LAUNCH(c, K_MISC, dsize * 20, (k_group_stats<EBT>), nblocks(dsize, BLOCK), (const EBT *)cnt, (const EBT *)EB, (const uint32_t *)s_g0, (const uint32_t *)gk, (const uint8_t *)ea.s_fl, dsize, (uint64_t)tot, d_hist);
        PFP_HIP(c, hipMemcpyAsync(hist, d_hist, 512, hipMemcpyDeviceToHost, c->stream));
        PFP_HIP(c, hipStreamSynchronize(c->stream));
        fprintf(stderr, "[pfbwt_hip] rows by group members (rows) x group rows (cols: <1K <4K <16K <64K <256K <1M <4M more); hard %llu, sort-route %llu of %llu; run-aware %d: %llu rows of %u special slots enumerated\n",
                hh[0], hh[1], (unsigned long long)tot, (int)runaware, (unsigned long long)tot2, (unsigned)ea.ecount);
        static const char *kn[8] = {"1", "2-3", "4-7", "8-15", "16-31", "32-63", "64-127", "128+"};
        for (int a = 0; a < 8; ++a) { fprintf(stderr, "[pfbwt_hip]  k %-7s", kn[a]); for (int b = 0; b < 8; ++b) fprintf(stderr, " %13llu", hist[a * 8 + b]); fprintf(stderr, "\n"); }
        return PFP_OK;
    }
};
template <typename EBT> static int emit_stage(pfp_ctx *c, const EmitArgs &prepass, int want_sa, int want_rssa, int slice, int nslices, const EmitVisit *visit)
{
    // c->tun.no_runaware: tests / measurements: every row enumerated, as with a full SA
    SlotStage<EBT> st{c, prepass, !want_sa && !c->tun.no_runaware, c->dsize};
    PFP_TRY(st.alloc_slot_arrays());
    PFP_TRY(st.slot_prepass());
    PFP_TRY(st.mark_big_groups());
    PFP_TRY(st.build_tile_index());
    if (st.runaware) PFP_TRY(st.build_special_list());
    if (c->tun.verbose) PFP_TRY(st.print_group_stats());
    const uint64_t nout = st.tot;
    if (nout < 2) return PFP_E_CORRUPT;
    if (c->n && nout != c->n + 1) return PFP_E_CORRUPT;         // emission must produce exactly n+1 rows
    if (!c->n) c->n = nout - 1;
    st.ea.nout = nout; st.ea.n = c->n;
    if (!visit) { c->nout = nout; c->hard = st.hh[0]; c->easy = nout - st.hh[0]; }
    if (c->flags & PFP_FLAG_U64) return Emission<uint64_t, EBT>(c, st.ea, want_sa != 0, want_rssa != 0, slice, nslices, st.tot2, visit).run();
    if (nout > 0xFFFFFFFFULL) return PFP_E_TOO_LARGE;           // 32-bit uint_t cannot hold the SA values (pfparser.hpp:326-331)
    return Emission<uint32_t, EBT>(c, st.ea, want_sa != 0, want_rssa != 0, slice, nslices, st.tot2, visit).run();
}

// The emission pre-pass (per-word and per-slot tables at the high end of the arena) and the emission itself: the build (visit ==
// nullptr) or a visit of the SA window by window that leaves the published build alone (visit_sa_windows).
static int emit_prepass_and_run(pfp_ctx *c, int want_sa, int want_rssa, int slice, int nslices, const EmitVisit *visit)
{
    const uint64_t dsize = c->dsize, dwords = c->dwords;
    uint32_t *F, *s_sl, *s_fb; uint8_t *s_fl, *s_pc; uint4 *winfo;
    if (dwords > WID_MASK) return PFP_E_TOO_LARGE;
    PFP_ALLOC_HI(c, F, uint32_t, dwords + 1);
    PFP_ALLOC_HI(c, s_sl, uint32_t, dsize); PFP_ALLOC_HI(c, s_fb, uint32_t, dsize);
    PFP_ALLOC_HI(c, s_fl, uint8_t, dsize); PFP_ALLOC_HI(c, s_pc, uint8_t, dsize);
    // F[r] = 1 + sum_{r' < r} occ[r']  (ilist[0] is the EOS row; pfbwt.hpp:259-268)
    PFP_TRY((device_scan<uint32_t, 0>(c, c->d_occ, F, dwords, nullptr)));
    PFP_LAUNCH(c, K_MISC, dwords * 8, k_u32_add_store, nblocks(dwords, BLOCK), (const uint32_t *)F, dwords, 1u, F);
    EmitArgs ea;
    ea.D = c->d_dict; ea.dsize = dsize; ea.dwords = (uint32_t)dwords; ea.w = c->w;
    ea.SA = c->d_gsa; ea.srank = c->d_srank; ea.ws = c->d_ws; ea.wrank = c->d_wrank;
    ea.occ = c->d_occ; ea.F = F; ea.ilist = c->d_ilist; ea.bwsai = c->d_bwsai; ea.bwlast = c->d_bwlast; ea.bwl_il = c->d_bwl_il;
    PFP_ALLOC_HI(c, winfo, uint4, dwords);
    PFP_LAUNCH(c, K_MISC, dwords * 32, k_pack_winfo, nblocks(dwords, BLOCK), (const uint32_t *)c->d_ws, (const uint32_t *)c->d_wrank, (const uint32_t *)c->d_occ, (const uint32_t *)F, dwords, winfo);
    ea.winfo = winfo;
    // per dictionary offset: one 16-byte record for k_emit_slots (suffix lengths must fit 26 bits), else word id | preceding byte + class head
    uint32_t maxlen = 0;
    {
        uint32_t *d_ml; PFP_ALLOC_HI(c, d_ml, uint32_t, 1);
        PFP_HIP(c, hipMemsetAsync(d_ml, 0, 4, c->stream));
        PFP_LAUNCH(c, K_MISC, dwords * 4, k_max_word_length, nblocks(dwords, BLOCK), (const uint32_t *)c->d_ws, dwords, d_ml);
        PFP_TRY(d2h_u32(c, d_ml, &maxlen));
    }
    if (want_sa && c->d_bwsai && c->nrows) {      // bwsai in ilist order: one gather per parse row here instead of a second dependent gather per OUTPUT row
        tpos_t *E; PFP_ALLOC_HI(c, E, tpos_t, c->nrows);
        PFP_LAUNCH(c, K_MISC, c->nrows * 20, k_bwsai_by_ilist, nblocks(c->nrows, BLOCK), (const uint32_t *)c->d_ilist, (const tpos_t *)c->d_bwsai, c->nrows, E);
        ea.bwsai_il = E;
        ea.use_e0 = (c->n != 0 && c->n + (uint64_t)c->w + 2 < 0xFFFFFFFFULL && !c->tun.no_slot_records) ? 1 : 0;      // positions fit the 32 bits of prec.x / s_g0
    }
    ea.wordid = c->d_wordid; ea.use_prec = (maxlen < (1u << PREC_SL_BITS) && !c->tun.no_slot_records) ? 1 : 0;
    ea.s_sl = s_sl; ea.s_fb = s_fb; ea.s_fl = s_fl; ea.s_pc = s_pc;
    if (!visit) { c->have_sa = want_sa != 0; c->have_rssa = want_rssa != 0; }
    // 64-bit row counters when the text may have 2^32 - 1 positions or more (n unknown after pfp_bwt_load without a hint)
    const bool force_wide = c->tun.force_wide_rows != 0;
    const bool wide = force_wide || c->n == 0 || c->n + 2 >= 0xFFFFFFFFULL;
    return wide ? emit_stage<uint64_t>(c, ea, want_sa, want_rssa, slice, nslices, visit) : emit_stage<uint32_t>(c, ea, want_sa, want_rssa, slice, nslices, visit);
}

static int bwt_build_body(pfp_ctx *c, int want_sa, int want_rssa, int slice, int nslices, pfp_bwt_sizes *out)
{
    HostTimer timer;
    const size_t mk = c->arena.mark_hi();
    c->emit_scratch_mark = mk;
    PFP_TRY(emit_prepass_and_run(c, want_sa, want_rssa, slice, nslices, nullptr));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    c->arena.release_hi(mk);
    c->stage = 3;
    c->stage_ms[2] = timer.ms();
    if (out) { out->nout = c->nout; out->r = c->runs; out->easy_cases = c->easy; out->hard_cases = c->hard; }
    return PFP_OK;
}
static int bwt_build_impl(pfp_ctx *c, int want_sa, int want_rssa, int slice, int nslices, pfp_bwt_sizes *out)
{
    if (!c || nslices < 1 || slice < 0 || slice >= nslices) return PFP_E_ARG;
    if (c->stage < 2) return PFP_E_STATE;
    if ((want_sa || want_rssa) && !c->d_bwsai) return PFP_E_STATE;
    PFP_HIP(c, hipSetDevice(c->device));
    c->arena.release_lo(c->lo_after_pbwt);
    drop_post_results(c);      // the marker array, document arrays, LCP arrays and thresholds of the previous build lived above that mark
    if (!c->gsa_valid) {   // gsacak, pfbwt.hpp:211 (--pfbwt-only: the loaded dictionary has not been sorted yet)
        ArenaGuard gs(c);
        const int rs = gs.done(sort_dict_suffixes(c));
        if (rs != PFP_OK) { c->gsa_valid = false; return rs; }
        c->lo_after_pbwt = c->arena.mark_lo();
    }
    ArenaGuard g(c);
    const int rc = g.done(bwt_build_body(c, want_sa, want_rssa, slice, nslices, out));
    if (rc != PFP_OK) { c->stage = 2; c->d_bwt = nullptr; c->d_sa = c->d_ssa = c->d_esa = nullptr; }   // e.g. PFP_E_NOMEM with want_sa: retry without, or in slices
    return rc;
}
// The SA of the last build (the whole output) window by window, without a resident SA: the emission pre-pass runs again as for
// want_sa = 1 (every row enumerated, bwsai in ilist order, the sort route of the many-member groups) and fn is called once per
// window of window_rows rows with (first row, rows, SA values of the window on the device).  Everything it allocates comes from the
// high end of the arena and is released before returning; the published build -- arrays, sizes, flags, stage times -- is untouched.
static int visit_sa_windows(pfp_ctx *c, uint64_t window_rows, std::function<int(uint64_t, uint64_t, const void *)> fn)
{
    if (!c->d_bwsai) return PFP_E_STATE;
    const size_t mk = c->arena.mark_hi();
    const EmitVisit visit{window_rows, std::move(fn)};
    PFP_TRY(emit_prepass_and_run(c, 1, 0, 0, 1, &visit));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    c->arena.release_hi(mk);
    return PFP_OK;
}

// ---- the way out: a device-resident result goes to a file descriptor through the ring of page-locked blocks of the file reader (csrc/ingest.h) -- the DMA
// transfer of block k + 1 overlaps the write of block k; a regular file is written by several threads with pwrite at the blocks'
// own offsets, a pipe (`-c bwt`: stdout) by one thread in order.  Stands in for the per-row fwrite of out_fn,
// src/pfbwt-f.cpp:298-328 (two to four calls per base there).
static int write_device_to_fd(pfp_ctx *c, const void *d_src, uint64_t bytes, int fd)
{
    if (!bytes) return PFP_OK;
    PFP_TRY(ensure_copy_stream(c));
    constexpr int NB = ING_RING;
    const off_t base = lseek(fd, 0, SEEK_CUR);
    // pwrite at computed offsets only where offsets mean something: a regular file that was not opened for appending (Linux ignores
    // pwrite's offset on an O_APPEND descriptor: `pfbwt-f -c bwt ... >> out` would get its blocks in completion order; the reference
    // writes sequentially with fwrite, src/pfbwt-f.cpp:298-328) -- everything else gets ONE in-order writer
    struct stat st; const int fl = fcntl(fd, F_GETFL);
    const bool seekable = base != (off_t)-1 && fl != -1 && !(fl & O_APPEND) && fstat(fd, &st) == 0 && S_ISREG(st.st_mode);
    const int nw = seekable ? 4 : 1;      // (measured on a memory-resident file system: 4 writers 6 GB/s, 8 writers 4.3 GB/s -- page allocation, not the copy, bounds a pwrite)
    for (int k = 0; k < NB; ++k) if (!c->ing_buf[k]) PFP_HIP(c, hipHostMalloc((void **)&c->ing_buf[k], ING_BLOCK, hipHostMallocDefault));
    hipEvent_t ev[NB];
    for (int k = 0; k < NB; ++k) PFP_HIP(c, hipEventCreateWithFlags(&ev[k], hipEventDisableTiming));
    const uint64_t nblk = (bytes + ING_BLOCK - 1) / ING_BLOCK;
    std::mutex mu; std::condition_variable cv;
    uint64_t issued = 0, written[NB]; bool fail = false;          // written[s]: blocks of slot s that are on the file (a slot is re-used when its previous block is)
    for (auto &x : written) x = 0;
    auto writer = [&](int tid) {
        for (uint64_t b = (uint64_t)tid; b < nblk; b += (uint64_t)nw) {
            const int slot = (int)(b % NB);
            { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return fail || issued > b; }); if (fail) return; }
            bool ok = hipEventSynchronize(ev[slot]) == hipSuccess;
            const uint64_t off = b * ING_BLOCK, len = bytes - off < ING_BLOCK ? bytes - off : ING_BLOCK;
            for (uint64_t done = 0; ok && done < len;) {
                const ssize_t r = seekable ? pwrite(fd, c->ing_buf[slot] + done, (size_t)(len - done), base + (off_t)(off + done)) : write(fd, c->ing_buf[slot] + done, (size_t)(len - done));
                if (r <= 0) ok = false; else done += (uint64_t)r;
            }
            std::lock_guard<std::mutex> lk(mu);
            if (!ok) fail = true;
            written[slot] += 1;
            cv.notify_all();
            if (!ok) return;
        }
    };
    std::vector<std::thread> th;
    for (int t = 0; t < nw; ++t) th.emplace_back(writer, t);
    int rc = PFP_OK;
    for (uint64_t b = 0; b < nblk && rc == PFP_OK; ++b) {
        const int slot = (int)(b % NB);
        { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return fail || written[slot] >= b / NB; }); if (fail) { rc = PFP_E_IO; break; } }
        const uint64_t off = b * ING_BLOCK, len = bytes - off < ING_BLOCK ? bytes - off : ING_BLOCK;
        if (hipMemcpyAsync(c->ing_buf[slot], (const uint8_t *)d_src + off, (size_t)len, hipMemcpyDeviceToHost, c->fa.copy) != hipSuccess || hipEventRecord(ev[slot], c->fa.copy) != hipSuccess) { (void)hipGetLastError(); rc = PFP_E_HIP; }
        std::lock_guard<std::mutex> lk(mu);
        if (rc != PFP_OK) fail = true; else issued = b + 1;
        cv.notify_all();
    }
    { std::lock_guard<std::mutex> lk(mu); if (rc != PFP_OK) fail = true; } cv.notify_all();
    for (auto &t : th) t.join();
    (void)hipStreamSynchronize(c->fa.copy);
    for (int k = 0; k < NB; ++k) (void)hipEventDestroy(ev[k]);
    if (rc == PFP_OK && fail) rc = PFP_E_IO;
    if (rc == PFP_OK && seekable && lseek(fd, base + (off_t)bytes, SEEK_SET) == (off_t)-1) rc = PFP_E_IO;
    return rc;
}

// .bwt over the slow link in its run-length form: with the run samples at hand, .ssa[k].row starts run k, so ONE byte per run (r bytes:
// 84 MB on S-32G) crosses PCIe instead of n + 1 (32 GB), and host threads write the runs out (memset) at memory bandwidth.
template <typename SAT> __global__ __launch_bounds__(BLOCK) void k_run_heads(const uint8_t *bwt, const SAT *ssa, uint64_t r, uint8_t *heads)
{
    const uint64_t k = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k < r) heads[k] = bwt[(uint64_t)ssa[2 * k]];
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

extern "C" {
int pfp_bwt_build(pfp_ctx *c, int want_sa, int want_rssa, pfp_bwt_sizes *out) { return bwt_build_impl(c, want_sa, want_rssa, 0, 1, out); }
int pfp_bwt_build_stream(pfp_ctx *c, int want_sa, int want_rssa, uint8_t *host_bwt, void *host_sa, pfp_bwt_sizes *out)
{
    if (!c || !host_bwt || (want_sa && !host_sa)) return PFP_E_ARG;
    PFP_HIP(c, hipSetDevice(c->device));
    PFP_TRY(ensure_copy_stream(c));
    c->h_bwt = host_bwt; c->h_sa = want_sa ? host_sa : nullptr;
    const int rc = bwt_build_impl(c, want_sa, want_rssa, 0, 1, out);
    c->h_bwt = nullptr; c->h_sa = nullptr;
    const hipError_t e = hipStreamSynchronize(c->fa.copy);               // the last windows' rows have arrived
    if (rc == PFP_OK && e != hipSuccess) { c->hip_err = (int)e; return PFP_E_HIP; }
    return rc;
}
int pfp_text_length(pfp_ctx *c, uint64_t *n) { if (!c || !n) return PFP_E_ARG; *n = c->n; return PFP_OK; }
int pfp_bwt_build_slice(pfp_ctx *c, int want_sa, int want_rssa, int slice, int nslices, pfp_bwt_sizes *out, uint64_t *slice_begin, uint64_t *slice_rows, uint64_t *esa_pairs)
{
    int rc = bwt_build_impl(c, want_sa, want_rssa, slice, nslices, out);
    if (rc != PFP_OK) return rc;
    if (slice_begin) *slice_begin = c->slice_begin;
    if (slice_rows) *slice_rows = c->slice_rows;
    if (esa_pairs) *esa_pairs = c->esa_pairs;
    return PFP_OK;
}

int pfp_bwt_get(pfp_ctx *c, uint8_t *bwt, void *sa, void *ssa, void *esa)
{
    if (!c) return PFP_E_ARG;
    if (c->stage < 3) return PFP_E_STATE;
    PFP_HIP(c, hipSetDevice(c->device));
    const size_t U = (c->flags & PFP_FLAG_U64) ? 8 : 4;
    if (bwt) PFP_HIP(c, hipMemcpy(bwt, c->d_bwt, c->slice_rows, hipMemcpyDeviceToHost));
    if (sa) { if (!c->d_sa) return PFP_E_STATE; PFP_HIP(c, hipMemcpy(sa, c->d_sa, c->slice_rows * U, hipMemcpyDeviceToHost)); }
    if (ssa) { if (!c->d_ssa) return PFP_E_STATE; PFP_HIP(c, hipMemcpy(ssa, c->d_ssa, c->runs * 2 * U, hipMemcpyDeviceToHost)); }
    if (esa) { if (!c->d_esa) return PFP_E_STATE; PFP_HIP(c, hipMemcpy(esa, c->d_esa, c->esa_pairs * 2 * U, hipMemcpyDeviceToHost)); }
    return PFP_OK;
}

int pfp_bwt_device_ptrs(pfp_ctx *c, const void **d_bwt, const void **d_sa, const void **d_ssa, const void **d_esa)
{
    if (!c) return PFP_E_ARG;
    if (c->stage < 3) return PFP_E_STATE;
    if (d_bwt) *d_bwt = c->d_bwt;
    if (d_sa) *d_sa = c->d_sa;
    if (d_ssa) *d_ssa = c->d_ssa;
    if (d_esa) *d_esa = c->d_esa;
    return PFP_OK;
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
} // extern "C"
