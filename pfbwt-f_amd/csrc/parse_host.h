// pfbwt-f_amd/csrc/parse_host.h -- host side of stages 1 and 2.  In the order the stages run:
//   pfp_parse_finalize / pfp_parse_finalize_shard: pad the text, scan_triggers, phrase ends, dedup_strings, build_dictionary and
//     (not for a shard) finish_parse, which starts with sort_dict_suffixes -- the sort the --pfbwt-only path of emit_host.h calls too;
//   pfp_shard_load / pfp_shard_view_get / pfp_merge_shards: a saved parse as a shard, and the merge of shard parses into the parse of
//     the whole text (view checks, fragment fetch, junction_pieces, candidate words, dedup_strings, build_dictionary, phrase sequence,
//     finish_parse); both derive phrase ends from word lengths with phrase_ends_from_words;
//   pfp_parse_get; pfp_parse_bwt (stage 2: the BWT of the parse) and pfp_parse_bwt_get;
//   pfp_bwt_load: the files of a finished stage 2 in place of the two stages.
// The kernels are in parse.h, sufsort.h, recsort.h, dictrec.h and prims.h, but for the small merge and shard kernels below.
// Included by pfbwt_hip.hip (ensure_arena, reset_results) behind feed_host.h (flush_view, h2d_copy, text_limit).
#pragma once

// ---- the device's width and the caller's U ------------------------------------------------------------------------------------------
// Index-valued arrays are D = 32 or 64 bits wide on the device and U = 32 (u64 == false) or 64 bits wide at the caller.
// Device to host: a null or empty destination is skipped; narrowing wraps like the reference's uint_t = 32 bit build.
template <typename D> static int download_as_u(pfp_ctx *c, const D *d, uint64_t cnt, void *dst, bool u64)
{
    if (!dst || !cnt) return PFP_OK;
    if (u64 == (sizeof(D) == 8)) { PFP_HIP(c, hipMemcpy(dst, d, cnt * sizeof(D), hipMemcpyDeviceToHost)); return PFP_OK; }
    std::vector<D> tmp((size_t)cnt);
    PFP_HIP(c, hipMemcpy(tmp.data(), d, cnt * sizeof(D), hipMemcpyDeviceToHost));
    if (u64) { uint64_t *o = (uint64_t *)dst; for (uint64_t i = 0; i < cnt; ++i) o[i] = tmp[(size_t)i]; }
    else { uint32_t *o = (uint32_t *)dst; for (uint64_t i = 0; i < cnt; ++i) o[i] = (uint32_t)tmp[(size_t)i]; }
    return PFP_OK;
}
// Host to device: a value that does not fit into D is PFP_E_TOO_LARGE.
template <typename D> static int upload_from_u(pfp_ctx *c, const void *src, uint64_t cnt, bool u64, D *d)
{
    if (u64 == (sizeof(D) == 8)) { PFP_HIP(c, hipMemcpy(d, src, cnt * sizeof(D), hipMemcpyHostToDevice)); return PFP_OK; }
    std::vector<D> tmp((size_t)cnt);
    if (u64) { const uint64_t *s = (const uint64_t *)src; for (uint64_t i = 0; i < cnt; ++i) { if (s[i] > (uint64_t)(D)~(D)0) return PFP_E_TOO_LARGE; tmp[(size_t)i] = (D)s[i]; } }
    else { const uint32_t *s = (const uint32_t *)src; for (uint64_t i = 0; i < cnt; ++i) tmp[(size_t)i] = s[i]; }
    PFP_HIP(c, hipMemcpy(d, tmp.data(), cnt * sizeof(D), hipMemcpyHostToDevice));
    return PFP_OK;
}

// what the trigger scan hands on: m phrases, the trigger bits per 16 bases with their counts per block of the scan in front of them
// (blockcnt[gts] = all), the packed shadow of the text for the de-duplication (dt.Xp == nullptr: none)
struct TriggerScan { uint64_t m; unsigned gts; uint16_t *mask16; uint64_t *blockcnt; DedupText dt; };

// ---- the merge of shard parses: what its pieces hand to each other ---------------------------------------------------------------------
struct ShardFrag { uint32_t id0 = 0xFFFFFFFFu, idl = 0xFFFFFFFFu; std::vector<uint8_t> w0, wl; };      // word id and bytes of a shard's first (head fragment) and last phrase (tail fragment)
struct JuncPiece { uint32_t js, je; tpos_t ye; uint8_t last; };              // a junction phrase: span in the junction buffer, global end position, last char
struct MergePlan {
    int nshards; const pfp_shard_view *v;
    uint64_t ntot = 0, mtot = 0, dtot = 0, ctot = 0, extra = 0;             // text, phrases, dictionary bytes and words of the shards together; junction phrases
    // interior phrases of shard r = [ia[r], ib[r]): all but the head fragment (r > 0) and the tail fragment (r < N-1); a shard
    // of ONE phrase (a short record or contig without a trigger window) in the middle is both at once and has none
    std::vector<uint64_t> ia, ib, lc;                                        // lc = left_context
    std::vector<uint8_t> one;                                                // m == 1
    std::vector<tpos_t> shift;                                               // shard r's Y coordinate + shift[r] = its global one
    std::vector<uint32_t> ubase, coff;                                       // where shard r's dictionary starts in the united buffer, its words among the candidates
    std::vector<ShardFrag> fr;
    std::vector<uint8_t> junc; std::vector<std::vector<JuncPiece>> pieces;   // pieces[s]: the junction phrases in front of the interior phrases of shard s
    MergePlan(int n_, const pfp_shard_view *v_) : nshards(n_), v(v_), ia((size_t)n_), ib((size_t)n_), lc((size_t)n_), one((size_t)n_), shift((size_t)n_), ubase((size_t)n_), coff((size_t)n_), fr((size_t)n_), pieces((size_t)n_) {}
    // first phrase: head fragment (shard 0 with one phrase: the start of the first junction phrase)
    bool has_head_fragment(int r) const { return r > 0 || (v[r].m == 1 && nshards > 1); }
    bool has_tail_fragment(int r) const { return r + 1 < nshards && v[r].m > 1; }
};
// the candidate words of the united dictionary: the shards' dictionaries and the junction words in one buffer, a span per candidate
struct MergeCand { uint8_t *U; uint32_t *cys, *cye, *cand_id; uint64_t call; tpos_t *d_xye = nullptr; uint32_t *d_xlast = nullptr; std::vector<uint32_t> xfirst; };

extern "C" {

// ---- dictionary suffix sort (shared by the parse and the --pfbwt-only path) ---------------------
static int sort_dict_suffixes(pfp_ctx *c)
{
    const uint64_t N = c->dsize;
    const size_t mk = c->arena.mark_hi();
    uint64_t *k0, *k1; uint32_t *v0, *v1;
    PFP_ALLOC_LO(c, c->d_gsa, uint32_t, N);
    PFP_ALLOC_LO(c, c->d_srank, uint32_t, N);
    const size_t lo_state = c->arena.mark_lo();
    PFP_ALLOC_HI(c, k0, uint64_t, N); PFP_ALLOC_HI(c, k1, uint64_t, N);
    PFP_ALLOC_HI(c, v0, uint32_t, N); PFP_ALLOC_HI(c, v1, uint32_t, N);
    BitRange full = {0, DK_KEY_BITS};
    int rounds = 0;
    // A collection that is not repetitive has a dictionary about as large as its text whose suffixes are told apart by their first
    // few dozen characters: the rounds then read the text itself (sufsort.h, text rounds) and no per-offset rank array exists -- the
    // emission takes the class heads per SLOT (d_srank), the word ranks come from the word-start flags that travel with the
    // suffixes (d_sflag).  A repetitive collection (pangenome: dictionary << text, variant words share long prefixes) keeps the
    // rank-based rounds, whose covered prefix doubles / quadruples; so does a dictionary on which the text rounds are given up.
    // A repetitive collection's dictionary is repetitive itself: sorted through its own level-2 parse (dictrec.h); outputs as of the text rounds
    if (c->tun.dict_rec > 0 || (c->tun.dict_rec < 0 && c->n != 0 && N <= c->n / 8 && N >= ((uint64_t)1 << 22))) {
        PFP_ALLOC_LO(c, c->d_sflag, uint8_t, N);
        int taken = 0;
        PFP_TRY(dict_sort_pfp(c, c->d_gsa, c->d_srank, c->d_sflag, &taken));
        if (taken) { c->d_grank = nullptr; c->arena.release_hi(mk); c->gsa_valid = true; return PFP_OK; }
        c->d_sflag = nullptr; c->arena.release_lo(lo_state);
    }
    const int want = c->tun.dict_text_rounds;
    bool text_mode = want > 0 || (want < 0 && c->n != 0 && N > c->n / 8);
    if (text_mode) {
        PFP_ALLOC_LO(c, c->d_sflag, uint8_t, N);
        c->d_grank = nullptr;
        PFP_LAUNCH(c, K_SS_INIT_KEYS, N * 13, k_dict_init_keys, nblocks(N, DK_TILE), (const uint8_t *)c->d_dict, N, k0, v0);
        int conv = 1;
        PFP_TRY(suffix_sort_doubling<true>(c, N, k0, v0, k1, v1, &full, 1, DK_CHARS, c->d_dict, c->d_gsa, (uint32_t *)nullptr, (uint2 *)nullptr, &rounds, 9, c->d_srank, c->d_sflag, 1, &conv));
        if (!conv) { text_mode = false; c->d_sflag = nullptr; c->arena.release_lo(lo_state); }
    }
    if (!text_mode) {
        PFP_ALLOC_LO(c, c->d_grank, uint2, N);
        PFP_LAUNCH(c, K_SS_INIT_KEYS, N * 13, k_dict_init_keys, nblocks(N, DK_TILE), (const uint8_t *)c->d_dict, N, k0, v0);
        PFP_TRY(suffix_sort_doubling<true>(c, N, k0, v0, k1, v1, &full, 1, DK_CHARS, c->d_dict, c->d_gsa, (uint32_t *)nullptr, c->d_grank, &rounds, 9, c->d_srank));
    }
    c->arena.release_hi(mk);
    c->gsa_valid = true;
    return PFP_OK;
}

// ---- de-duplication of byte strings ------------------------------------------------------------------------------------------------
// verbose: where thread 0 of every workgroup of k_dedup_insert spent its time (dedup_phases)
static int dedup_report_phases(pfp_ctx *c, const unsigned long long *d_phase, bool coop)
{
    unsigned long long hp[512], tot[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    PFP_HIP(c, hipMemcpyAsync(hp, d_phase, 4096, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    for (int q = 0; q < 64; ++q) for (int k = 0; k < 8; ++k) tot[k] += hp[q * 8 + k];
    const double nwg = tot[5] ? (double)tot[5] : 1.0;
    fprintf(stderr, "[pfbwt_hip] k_dedup_insert (%s), thread 0 of %llu workgroups, mean us per stage: abandon flag %.2f, spans + window bounds %.2f, window into LDS %.2f, hash %.2f, table + compare %.2f\n",
            coop ? "cooperative" : "per lane", tot[5], tot[0] / nwg / 100.0, tot[1] / nwg / 100.0, tot[2] / nwg / 100.0, tot[3] / nwg / 100.0, tot[4] / nwg / 100.0);
    return PFP_OK;
}
// verbose: how many phrases and compares used the packed shadow of the text; the counters start from 0 again
static int dedup_report_packed(pfp_ctx *c, unsigned long long *d_stats, bool coop)
{
    unsigned long long st[4];
    PFP_HIP(c, hipMemcpyAsync(st, d_stats, 32, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    fprintf(stderr, "[pfbwt_hip] k_dedup_insert (%s): %llu phrases in packed windows, %llu in byte windows; compares in packed windows: %llu in 2-bit form, %llu by bytes\n",
            coop ? "cooperative" : "per lane", st[0], st[1], st[2], st[3]);
    PFP_HIP(c, hipMemsetAsync(d_stats, 0, 64, c->stream));
    return PFP_OK;
}
// The table of representatives of the m strings (parse.h): at most two attempts.  Hands back the table (t->slotof[j] = where string
// j went, t->dhash = the hashes of the *nd distinct strings) and, with last_out, last_out[j].  The table stays allocated at the high end.
static int dedup_fill_table(pfp_ctx *c, const uint8_t *Y, Spans sp, uint64_t m, uint64_t total_bytes, uint8_t *last_out, DedupText dt, DedupTable *tab, uint32_t *ndistinct)
{
    uint32_t *longlist, *d_u32, *slotof;
    const uint64_t maxlong = total_bytes / LONG_PHRASE + 2;
    PFP_ALLOC_HI(c, longlist, uint32_t, maxlong);
    PFP_ALLOC_HI(c, d_u32, uint32_t, 8);
    uint32_t *d_abandon; PFP_ALLOC_HI(c, d_abandon, uint32_t, 64);      // a 256-byte block of its own
    PFP_ALLOC_HI(c, slotof, uint32_t, m);
    dt.stats = nullptr;
    if (dt.Xp && c->tun.verbose) { PFP_ALLOC_HI(c, dt.stats, unsigned long long, 8); PFP_HIP(c, hipMemsetAsync(dt.stats, 0, 64, c->stream)); }
    const int force_small = c->tun.dedup_table_log2;      // tests: a first table that overflows
    DedupTable &t = *tab;
    for (int attempt = 0;; ++attempt) {
        if (attempt == 2) return PFP_E_CORRUPT;
        const size_t mk = c->arena.mark_hi();
        // first guess: a collection is repetitive (distinct strings << strings); if more than half of that table fills up, the
        // second table holds twice the number of strings, which cannot overflow
        uint64_t want = attempt == 0 ? m / 4 : 2 * m;
        const uint64_t floor_ = 4 * m < (1ULL << 20) ? 4 * m : (1ULL << 20);     // small inputs: 4 entries per string (cannot overflow); else at least 2^20
        if (want < floor_) want = floor_;
        int lg = 10; while ((1ULL << lg) < want) ++lg;
        if (attempt == 0 && force_small) lg = force_small;
        const uint64_t T = 1ULL << lg;
        const uint64_t limit = T >= 2 * m ? m + 1 : T / 2;
        if (limit >= 0x7FFFFFFFULL || T > 0x80000000ULL) return PFP_E_TOO_LARGE;      // dense entry indices and slots share 31 bits of slotof[]
        PFP_ALLOC_HI(c, t.ent, DedupEntry, T);
        PFP_ALLOC_HI(c, t.dslot, uint32_t, limit); PFP_ALLOC_HI(c, t.dhash, uint64_t, limit);
        t.mask = T - 1; t.slotof = slotof; t.nd = d_u32; t.limit = (uint32_t)limit; t.overflow = d_u32 + 1; t.abandon = d_abandon;
        PFP_HIP(c, hipMemsetAsync(d_abandon, 0, 4, c->stream));
        PFP_HIP(c, hipMemsetAsync(t.ent, 0xFF, T * sizeof(DedupEntry), c->stream));
        PFP_HIP(c, hipMemsetAsync(d_u32, 0, 32, c->stream));
        unsigned long long *d_phase = nullptr;
        if (c->tun.dedup_phases) { PFP_ALLOC_HI(c, d_phase, unsigned long long, 512); PFP_HIP(c, hipMemsetAsync(d_phase, 0, 4096, c->stream)); }
        // the order of the workgroups (parse.h, DedupOrder): columns of loci per XCD when the text is a collection of similar sequences
        const uint64_t nb = nblocks(m, BLOCK);
        uint64_t grid = nb;
        const DedupOrder ord = make_dedup_order(nb, sp.ys32 ? 0 : c->nseq + c->fa.records, c->tun.dedup_period, c->tun.dedup_chunk, 64 /* sequences of less than ~1.6 Mbase: nothing to gain */, &grid);
        if (c->tun.verbose && ord.period) fprintf(stderr, "[pfbwt_hip] text de-duplication: %llu workgroups visited as %u sequences x %u loci, columns of %u per XCD (grid %llu)\n", (unsigned long long)nb, ord.rows, ord.period, ord.chunk, (unsigned long long)grid);
        // variant: 1 = cooperative, 0 = per lane, -1 (default) = cooperative for a collection (>= 8 sequences fed) as long as its first table lasts (parse.h)
        const bool coop = c->tun.dedup_variant > 0 || (c->tun.dedup_variant < 0 && attempt == 0 && !sp.ys32 && c->nseq + c->fa.records >= 8);
        if (!coop) PFP_LAUNCH(c, K_PHRASE_HASH, 2 * total_bytes + m * 24, k_dedup_insert<false>, grid, Y, sp, m, c->hash_seed, t, longlist, d_u32 + 2, last_out, d_phase, ord, dt);
        else PFP_LAUNCH(c, K_PHRASE_HASH, 2 * total_bytes + m * 24, k_dedup_insert<true>, grid, Y, sp, m, c->hash_seed, t, longlist, d_u32 + 2, last_out, d_phase, ord, dt);
        if (d_phase) PFP_TRY(dedup_report_phases(c, d_phase, coop));
        uint32_t h3[3];
        PFP_HIP(c, hipMemcpyAsync(h3, d_u32, 12, hipMemcpyDeviceToHost, c->stream));
        PFP_HIP(c, hipStreamSynchronize(c->stream));
        if (!h3[1] && h3[2]) {
            PFP_LAUNCH_B(c, K_PHRASE_HASH_LONG, 2.0 * total_bytes / 64, k_dedup_insert_long, h3[2], DL_THREADS, Y, sp, (const uint32_t *)longlist, c->hash_seed, t);
            PFP_HIP(c, hipMemcpyAsync(h3, d_u32, 12, hipMemcpyDeviceToHost, c->stream));
            PFP_HIP(c, hipStreamSynchronize(c->stream));
        }
        if (dt.stats) PFP_TRY(dedup_report_packed(c, dt.stats, coop));
        if (!h3[1]) { *ndistinct = h3[0]; return PFP_OK; }
        if (c->tun.verbose) fprintf(stderr, "[pfbwt_hip] phrase table of 2^%d entries overflowed (%u distinct so far, state %u): retry\n", lg, h3[0], h3[1]);
        c->arena.release_hi(mk);
    }
}
// Ids in the order of the hashes of the nd distinct strings: d_id[j] for every string, rep[id] = a string with that id, occw[id] = how
// many strings have it.  mk0 = the high mark from before the table: the table is given back, rep / occw are all that stays above it.
static int dedup_assign_ids(pfp_ctx *c, const DedupTable &t, uint32_t nd, uint64_t m, size_t mk0, uint32_t *d_id, uint32_t **rep_out, uint32_t **occw_out)
{
    uint64_t *k1, *sk; uint32_t *v0, *v1, *sv, *rep, *occw;
    PFP_ALLOC_HI(c, rep, uint32_t, (size_t)nd + 1); PFP_ALLOC_HI(c, occw, uint32_t, (size_t)nd + 1);
    PFP_ALLOC_HI(c, k1, uint64_t, nd); PFP_ALLOC_HI(c, v0, uint32_t, nd); PFP_ALLOC_HI(c, v1, uint32_t, nd);
    PFP_LAUNCH(c, K_MISC, nd * 4, k_iota_u32, nblocks(nd, BLOCK), v0, (uint64_t)nd);
    BitRange full = {0, 64};
    PFP_TRY(radix_sort_pairs<uint64_t>(c, t.dhash, v0, k1, v1, nd, &full, 1, &sk, &sv));
    uint32_t *idofk;
    PFP_ALLOC_HI(c, idofk, uint32_t, nd);
    PFP_LAUNCH(c, K_DEDUP_HEADS, (uint64_t)nd * 44, k_dedup_assign, nblocks(nd, BLOCK), (const uint32_t *)sv, (uint64_t)nd, t, rep, occw, idofk);
    PFP_LAUNCH(c, K_DEDUP_HEADS, m * 12, k_dedup_ids, nblocks(m, BLOCK), (const DedupEntry *)t.ent, (const uint32_t *)idofk, (const uint32_t *)t.slotof, m, d_id);
    // the table (32 bytes per entry) is dead now: give its space back and keep only rep / occw, moved to the top of what it
    // occupied (they were allocated below it, and are smaller than it: the two regions cannot overlap)
    c->arena.release_hi(mk0);
    uint32_t *rep2, *occw2;
    PFP_ALLOC_HI(c, rep2, uint32_t, (size_t)nd + 1); PFP_ALLOC_HI(c, occw2, uint32_t, (size_t)nd + 1);
    if ((char *)occw2 < (char *)(rep + nd + 1) + ((size_t)nd + 1) * 4) return PFP_E_CORRUPT;      // cannot happen (see above)
    PFP_HIP(c, hipMemcpyAsync(rep2, rep, ((size_t)nd + 1) * 4, hipMemcpyDeviceToDevice, c->stream));
    PFP_HIP(c, hipMemcpyAsync(occw2, occw, ((size_t)nd + 1) * 4, hipMemcpyDeviceToDevice, c->stream));
    *rep_out = rep2; *occw_out = occw2;
    return PFP_OK;
}
// De-duplicates the m byte strings described by (Y, sp) -- the std::map of pfparser.hpp:69-70, 595-597 -- exactly, with a
// hash table of representatives (parse.h).  Outputs: number of distinct strings, d_id[j] = id of string j (ids follow the
// sorted hashes of the distinct strings), rep[id] = a string with that id, occw[id] = how many strings have it.
// dt: the packed shadow of the text (parse.h, DedupText), or dt.Xp == nullptr (bytes only).
static int dedup_strings(pfp_ctx *c, const uint8_t *Y, Spans sp, uint64_t m, uint64_t total_bytes, uint32_t *d_id, uint64_t *ndistinct, uint32_t **rep_out, uint32_t **occw_out, uint8_t *last_out,
                         DedupText dt)
{
    const size_t mk0 = c->arena.mark_hi();
    DedupTable t; uint32_t nd = 0;
    PFP_TRY(dedup_fill_table(c, Y, sp, m, total_bytes, last_out, dt, &t, &nd));
    PFP_TRY(dedup_assign_ids(c, t, nd, m, mk0, d_id, rep_out, occw_out));
    *ndistinct = nd;
    return PFP_OK;
}

// The dictionary D' (distinct strings in id order, each + EndOfWord, then EndOfDict), its word starts and the
// word id of every offset.
static int build_dictionary(pfp_ctx *c, const uint8_t *Y, Spans sp, const uint32_t *rep, uint64_t dwords)
{
    uint32_t *wlen1; tpos_t *srcstart;
    PFP_ALLOC_HI(c, wlen1, uint32_t, dwords); PFP_ALLOC_HI(c, srcstart, tpos_t, dwords);
    const unsigned gd = nblocks(dwords, BLOCK);
    PFP_LAUNCH(c, K_MISC, dwords * 16, k_word_lengths, gd, sp, rep, dwords, wlen1);
    PFP_ALLOC_LO(c, c->d_ws, uint32_t, dwords + 1);
    PFP_TRY((device_scan<uint32_t, 0>(c, wlen1, c->d_ws, dwords, c->d_ws + dwords)));
    uint32_t dsm1 = 0; PFP_TRY(d2h_u32(c, c->d_ws + dwords, &dsm1));
    const uint64_t dsize = (uint64_t)dsm1 + 1;
    c->dwords = dwords; c->dsize = dsize;
    if (dsize + 64 >= 0xFFFFFFFFULL) return PFP_E_TOO_LARGE;
    PFP_ALLOC_LO(c, c->d_dict, uint8_t, dsize + 16);
    PFP_ALLOC_LO(c, c->d_wordid, uint32_t, dsize);
    PFP_LAUNCH(c, K_MISC, dwords * 12, k_rep_starts, gd, sp, rep, dwords, srcstart);
    PFP_LAUNCH(c, K_DICT_BUILD, dsize * 6, k_dict_build, nblocks(dsize, 16 * BLOCK), Y, (const tpos_t *)srcstart, (const uint32_t *)c->d_ws, (uint32_t)dwords, dsize, c->d_dict, c->d_wordid);
    return PFP_OK;
}

// From the dictionary to ranks (sort_dict + generate_ranks, pfparser.hpp:494-517), occ (:471-480), the parse
// and the sorted .dict image.  Needs c->m, d_pid, dwords/dsize/d_ws/d_dict/d_wordid; occw = occurrences per word id.
static int finish_parse(pfp_ctx *c, const uint32_t *occw)
{
    const uint64_t m = c->m, dwords = c->dwords, dsize = c->dsize;
    const unsigned gm = nblocks(m, BLOCK), gd = nblocks(dwords, BLOCK);
    // suffix sort of the dictionary: gives word ranks now and the emission order later
    PFP_TRY(sort_dict_suffixes(c));
    uint32_t *wk0, *wk1, *wv0, *wv1, *idofrank, *len1; tpos_t *srcstart;
    PFP_ALLOC_HI(c, wk0, uint32_t, dwords); PFP_ALLOC_HI(c, wk1, uint32_t, dwords); PFP_ALLOC_HI(c, wv0, uint32_t, dwords); PFP_ALLOC_HI(c, wv1, uint32_t, dwords);
    PFP_ALLOC_HI(c, idofrank, uint32_t, dwords); PFP_ALLOC_HI(c, len1, uint32_t, dwords + 1); PFP_ALLOC_HI(c, srcstart, tpos_t, dwords);
    PFP_ALLOC_LO(c, c->d_wrank, uint32_t, dwords);
    PFP_ALLOC_LO(c, c->d_occ, uint32_t, dwords);
    PFP_ALLOC_LO(c, c->d_parse, uint32_t, m + 1);
    PFP_ALLOC_LO(c, c->d_sdict, uint8_t, dsize + 16);
    if (c->d_grank) {
        PFP_LAUNCH(c, K_WORD_RANK, dwords * 16, k_wordstart_keys, gd, (const uint32_t *)c->d_ws, (const uint2 *)c->d_grank, dwords, wk0, wv0);
        BitRange br = {0, bits_for(dsize)};
        uint32_t *sk32, *sv32;
        PFP_TRY(radix_sort_pairs<uint32_t>(c, wk0, wv0, wk1, wv1, dwords, &br, 1, &sk32, &sv32));
        PFP_LAUNCH(c, K_WORD_RANK, dwords * 20, k_word_rank, gd, (const uint32_t *)sv32, dwords, occw, c->d_wrank, idofrank, c->d_occ);
    } else {
        // text-round sort: the suffixes that start a word carry a flag to their slots; in slot order they ARE the words in
        // lexicographic order (two distinct words are never byte-identical), so their word ids, compacted, are the ids by rank
        const size_t mkf = c->arena.mark_hi();
        const uint64_t nt = nblocks(dsize, WF_TILE);
        uint32_t *tcnt, *tbase, *d_cnt;
        PFP_ALLOC_HI(c, tcnt, uint32_t, nt); PFP_ALLOC_HI(c, tbase, uint32_t, nt); PFP_ALLOC_HI(c, d_cnt, uint32_t, 1);
        PFP_LAUNCH(c, K_WORD_RANK, dsize, k_flag_tile_count, nt, (const uint8_t *)c->d_sflag, dsize, tcnt);
        PFP_TRY((device_scan<uint32_t, 0>(c, tcnt, tbase, nt, d_cnt)));
        uint32_t nst = 0; PFP_TRY(d2h_u32(c, d_cnt, &nst));
        if (nst != dwords) return PFP_E_CORRUPT;
        PFP_LAUNCH(c, K_WORD_RANK, dsize + dwords * 24, k_word_rank_flags, nt, (const uint8_t *)c->d_sflag, (const uint32_t *)tbase, (const uint32_t *)c->d_gsa, (const uint32_t *)c->d_wordid, dsize, (uint32_t)dwords,
                   occw, c->d_wrank, idofrank, c->d_occ);
        c->arena.release_hi(mkf);
    }
    PFP_LAUNCH(c, K_PARSE_RANKS, m * 12, k_parse_ranks, gm, (const uint32_t *)c->d_pid, (const uint32_t *)c->d_wrank, m, c->d_parse);
    PFP_LAUNCH(c, K_DICT_SORTED, dwords * 12, k_sorted_lengths, gd, (const uint32_t *)c->d_ws, (const uint32_t *)idofrank, dwords, len1, srcstart);
    PFP_TRY((device_scan<uint32_t, 0>(c, len1, len1, dwords, len1 + dwords)));
    PFP_LAUNCH(c, K_DICT_SORTED, dsize * 2, k_dict_build, nblocks(dsize, 16 * BLOCK), (const uint8_t *)c->d_dict, (const tpos_t *)srcstart, (const uint32_t *)len1, (uint32_t)dwords, dsize,
               c->d_sdict, (uint32_t *)nullptr);
    return PFP_OK;
}

// ---- stage 1: the parse of the fed text ---------------------------------------------------------------------------------------------
// the k-mer of the rolling hash keeps 2 bits per base of the window: hash.hpp:26 (w == 32: observed x86 value)
static uint64_t trigger_kmask(int w) { return (w == 32) ? 0ULL : ((1ULL << (2 * w)) - 1ULL); }

// The end of stage 1, for the parse of a text and for the merge of shard parses alike: the scratch above `mk` goes back, what
// lies at the low end is the parse.
static int parse_done(pfp_ctx *c, size_t mk, const HostTimer &timer, pfp_parse_sizes *out)
{
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    c->arena.release_hi(mk);
    c->stage = 1;
    c->lo_after_parse = c->arena.mark_lo();
    c->stage_ms[0] = timer.ms();
    if (out) { out->n = c->n; out->m = c->m; out->dwords = c->dwords; out->dsize = c->dsize; }
    return PFP_OK;
}

// The trigger windows of the padded text X[0, n + w): one of three scans -- the table scan over a pending row view (which writes
// the text as it goes), the table scan over X, the hash per window (w > TS_MAX_W, or no_trigger_table) --, the counts in front of
// every block, and the first invalid character if there is one (PFP_E_INVALID_CHAR, pfp_error_detail).
static int scan_triggers(pfp_ctx *c, TriggerScan *ts)
{
    const uint64_t n = c->n; const int w = c->w;
    uint8_t *X = c->tb + 16;
    const unsigned gts = nblocks(n, 16 * BLOCK);
    uint16_t *mask16; uint64_t *blockcnt; uint32_t *d_u32; unsigned long long *d_err;
    PFP_ALLOC_HI(c, mask16, uint16_t, (size_t)gts * BLOCK);
    PFP_ALLOC_HI(c, blockcnt, uint64_t, (size_t)gts + 1);
    PFP_ALLOC_HI(c, d_u32, uint32_t, 8);
    PFP_ALLOC_HI(c, d_err, unsigned long long, 1);
    PFP_HIP(c, hipMemsetAsync(d_err, 0xff, 8, c->stream));
    PFP_HIP(c, hipMemsetAsync(d_u32, 0, 32, c->stream));
    const uint64_t kmask = trigger_kmask(w);
    const bool no_trigtab = c->tun.no_trigger_table != 0;      // tests / measurements: the hash evaluated per base
    // the packed shadow of the text for the de-duplication (parse.h, DedupText): written by the table scan, n / 4 + n / 128 bytes, with guard
    // words in front of word 0 and behind the last (the window and compare loads read whole 16-byte pieces)
    DedupText dt = {nullptr, nullptr, 0, nullptr};
    if (w <= TS_MAX_W && !no_trigtab && c->tun.dedup_packed) {
        const uint64_t nw = (uint64_t)gts * BLOCK;
        uint32_t *xp; unsigned long long *xc;
        PFP_ALLOC_HI(c, xp, uint32_t, nw + 128);
        PFP_ALLOC_HI(c, xc, unsigned long long, nw / 64 + 1);
        dt.Xp = xp + 64; dt.Xc = xc; dt.nwords = nw;
    }
    if (c->view.src && !(w <= TS_MAX_W && !no_trigtab)) PFP_TRY(flush_view(c));      // the hash-per-window scan reads the text from X
    if (w <= TS_MAX_W && !no_trigtab) {
        const uint32_t tabwords = (1u << (2 * w)) >= 32u ? (1u << (2 * w)) / 32u : 1u;
        if (!c->d_trigtab) {      // w and p are fixed for the life of a context
            PFP_HIP(c, hipMalloc((void **)&c->d_trigtab, (size_t)TS_TAB_WORDS * 4));
            PFP_LAUNCH(c, K_MISC, tabwords * 4, k_trigger_table, nblocks(tabwords, BLOCK), w, make_divtest(c->p), c->d_trigtab);
        }
        const uint64_t nthreads_total = (uint64_t)gts * BLOCK;
        // a few workgroups per CU, each with a contiguous share of the groups (the table is loaded once per workgroup); small texts: no fewer
        // workgroups than one per 16 Kbase, so that they still spread over the CUs
        if (!c->num_cus) {
#if !defined(PFBWT_EMU_HIP_RUNTIME_H)
            int cus = 0;
            PFP_HIP(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
            c->num_cus = cus > 0 ? cus : 1;
#else
            c->num_cus = 2;
#endif
        }
        uint64_t nwg = ((uint64_t)gts + 3) / 4;
        if (nwg > (uint64_t)c->num_cus * TS_WG_PER_CU) nwg = (uint64_t)c->num_cus * TS_WG_PER_CU;
        const uint32_t gpw = (uint32_t)((gts + nwg - 1) / nwg);
        nwg = (gts + (uint64_t)gpw - 1) / gpw;
        const uint32_t waves = c->tun.scan_waves < 1 ? 1u : c->tun.scan_waves > (int)TS_WAVES ? TS_WAVES : (uint32_t)c->tun.scan_waves;
        const uint32_t run = (gpw + waves - 1) / waves;      // one run per wave: the wave streams its own piece of the share
        if (c->view.src) {      // the rows of pfp_parse_feed_device_view are read where they are; the scan writes the text (2 B per base instead of 1 + a copy pass)
            const RowView rv = {c->view.src, c->view.count, c->view.len, c->view.stride, c->view.len + (uint64_t)w};
            PFP_LAUNCH_B(c, K_TRIGGER_SCAN, 2 * n + n / 8, (k_trigger_scan_tab<true>), nwg, TS_THREADS, X, n, w, (const uint32_t *)c->d_trigtab, tabwords, (uint32_t)kmask,
                         (int)((c->flags & PFP_FLAG_NON_ACGT_TO_A) != 0), gpw, waves, run, nthreads_total, mask16, blockcnt, d_err, rv, (uint32_t *)dt.Xp, (unsigned long long *)dt.Xc);
            c->view.src = nullptr;      // X holds the text from here on
        } else
        PFP_LAUNCH_B(c, K_TRIGGER_SCAN, n + n / 8, (k_trigger_scan_tab<false>), nwg, TS_THREADS, X, n, w, (const uint32_t *)c->d_trigtab, tabwords, (uint32_t)kmask,
                     (int)((c->flags & PFP_FLAG_NON_ACGT_TO_A) != 0), gpw, waves, run, nthreads_total, mask16, blockcnt, d_err, RowView{nullptr, 0, 0, 0, 1}, (uint32_t *)dt.Xp, (unsigned long long *)dt.Xc);
    } else
    PFP_LAUNCH(c, K_TRIGGER_SCAN, n * 2 + n / 8, k_trigger_scan, gts, X, n, w, make_divtest(c->p), kmask, (int)((c->flags & PFP_FLAG_NON_ACGT_TO_A) != 0), mask16, blockcnt, d_err);
    PFP_TRY((device_scan<uint64_t, 0>(c, blockcnt, blockcnt, gts, blockcnt + gts)));
    uint64_t ntrig = 0; unsigned long long herr = 0;
    PFP_HIP(c, hipMemcpyAsync(&herr, d_err, 8, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipMemcpyAsync(&ntrig, blockcnt + gts, 8, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    if (herr != ~0ULL) {   // hash.hpp:31
        uint8_t ch = 0;
        PFP_HIP(c, hipMemcpy(&ch, X + herr, 1, hipMemcpyDeviceToHost));
        c->err_pos = herr; c->err_ch = ch;
        return PFP_E_INVALID_CHAR;
    }
    ts->m = ntrig + 1; ts->gts = gts; ts->mask16 = mask16; ts->blockcnt = blockcnt; ts->dt = dt;
    return PFP_OK;
}

// A stage that fails (PFP_E_NOMEM, PFP_E_INVALID_CHAR, ...) leaves the workspace as it found it (ArenaGuard, common.h)
static int parse_finalize_impl(pfp_ctx *c, pfp_parse_sizes *out, bool shard_only);
static int parse_finalize_entry(pfp_ctx *c, pfp_parse_sizes *out, bool shard_only)
{
    if (!c) return PFP_E_ARG;
    if (c->stage != 0) return PFP_E_STATE;
    if (c->n == 0) return PFP_E_ARG;
    PFP_HIP(c, hipSetDevice(c->device));
    ArenaGuard g(c);
    const int rc = g.done(parse_finalize_impl(c, out, shard_only));
    // after a failure the fed text is still there (stage 0): finalize can be retried (more workspace), more text can be
    // appended, or pfp_reset drops it
    if (rc != PFP_OK) { c->m = c->dwords = c->dsize = 0; c->gsa_valid = false; }
    return rc;
}
int pfp_parse_finalize(pfp_ctx *c, pfp_parse_sizes *out) { return parse_finalize_entry(c, out, false); }
int pfp_parse_finalize_shard(pfp_ctx *c, pfp_parse_sizes *out) { return parse_finalize_entry(c, out, true); }
static int parse_finalize_impl(pfp_ctx *c, pfp_parse_sizes *out, bool shard_only)
{
    HostTimer timer;
    const uint64_t n = c->n; const int w = c->w;
    PFP_TRY(ensure_arena(c, n));
    c->arena.reset();
    uint8_t *X = c->tb + 16; const uint8_t *Y = c->tb + 15;
    // Dollar in front, w Dollars behind (pfparser.hpp:315-318, 484-489)
    PFP_HIP(c, hipMemsetAsync(c->tb, Dollar, 16, c->stream));
    PFP_HIP(c, hipMemsetAsync(X + n, Dollar, (size_t)w, c->stream));
    const size_t mk = c->arena.mark_hi();

    // 1. trigger scan
    TriggerScan ts;
    PFP_TRY(scan_triggers(c, &ts));
    const uint64_t m = ts.m;
    if (m > 0xFFFFFFFEULL - 64) return PFP_E_TOO_LARGE;       // pfparser.hpp:399-404: more than 2^32-2 phrases is a hard limit of the reference too
    c->m = m;
    PFP_ALLOC_LO(c, c->d_ye, tpos_t, m);
    PFP_LAUNCH(c, K_PHRASE_ENDS, n / 8 + m * 4, k_phrase_ends, nblocks(ts.gts, PE_BLOCKS), (const uint16_t *)ts.mask16, (const uint64_t *)ts.blockcnt, (uint64_t)ts.gts, c->d_ye);
    PFP_LAUNCH(c, K_MISC, 8, k_set_u64, 1, c->d_ye, m - 1, (uint64_t)(n + (uint64_t)w));

    // 2. distinct phrases, dictionary
    Spans sp; sp.ye = c->d_ye; sp.ys32 = nullptr; sp.ye32 = nullptr; sp.w = w;
    uint64_t dwords = 0; uint32_t *rep, *occw;
    PFP_ALLOC_LO(c, c->d_pid, uint32_t, m);
    PFP_ALLOC_LO(c, c->d_last, uint8_t, m);
    PFP_TRY(dedup_strings(c, Y, sp, m, n + (uint64_t)w + 1 + m * (uint64_t)w, c->d_pid, &dwords, &rep, &occw, c->d_last, ts.dt));      // + last[j] = Y[ye[j] - w], pfparser.hpp:599
    PFP_TRY(build_dictionary(c, Y, sp, rep, dwords));
    // 3. dictionary suffix sort, ranks, occ, parse, sorted .dict image -- not for a shard that is only going to be merged: the
    //    merge sorts the united dictionary, and a shard's dictionary is nearly as large as the whole collection's
    if (!shard_only) PFP_TRY(finish_parse(c, occw));
    return parse_done(c, mk, timer, out);
}

// ---- multi-GPU: merge of shard parses (semantics of PfParser::operator+=, pfparser.hpp:194-263) -----
// Shard r > 0 was parsed as the text  A^w + X_r  (the w 'A's that end shard r-1, pfparser.hpp:335-337, as left
// context), so its closed phrases are exactly the phrases of the whole text; only its first phrase (Dollar +
// context + head) and, for r < N-1, its last phrase (tail + w Dollars) are fragments: tail_r + head_{r+1} is
// the phrase that straddles the boundary.  All dictionaries are laid out in one buffer, the two fragment
// words of a boundary are re-pointed at the junction word, and the union is de-duplicated like phrases are.
__global__ __launch_bounds__(BLOCK) void k_merge_spans(const uint32_t *ws, uint32_t dwords, uint32_t ubase, uint32_t coff, uint32_t frag0, uint32_t frag0_ys, uint32_t frag0_ye,
                                                       uint32_t fragl, uint32_t fragl_ys, uint32_t fragl_ye, uint32_t *ys, uint32_t *ye)
{
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= dwords) return;
    uint32_t a = ubase + ws[k], b = ubase + ws[k + 1] - 2u;   // word bytes without its EndOfWord
    if (k == frag0) { a = frag0_ys; b = frag0_ye; }
    if (k == fragl) { a = fragl_ys; b = fragl_ye; }
    ys[coff + k] = a; ye[coff + k] = b;
}
__global__ __launch_bounds__(BLOCK) void k_merge_phrases(const uint32_t *pid, const tpos_t *ye, const uint8_t *last, uint32_t m, uint32_t j0, uint32_t goff, uint32_t coff, tpos_t shift,
                                                         const uint32_t *cand_id, tpos_t junction_ye, uint32_t junction_last, int has_junction,
                                                         uint32_t *gpid, tpos_t *gye, uint8_t *glast, uint32_t *occw)
{
    const uint32_t j = j0 + blockIdx.x * BLOCK + threadIdx.x;
    if (j >= m) return;
    const uint32_t g = goff + j - j0;
    const uint32_t id = cand_id[coff + pid[j]];
    gpid[g] = id;
    atomicAdd(&occw[id], 1u);
    if (has_junction && j + 1 == m) { gye[g] = junction_ye; glast[g] = (uint8_t)junction_last; }   // the phrase that ends in the next shard
    else { gye[g] = ye[j] + shift; glast[g] = last[j]; }
}

__global__ __launch_bounds__(BLOCK) void k_merge_extra(const uint32_t *cand_id, const tpos_t *xye, const uint32_t *xlast, uint32_t nx, uint32_t goff, uint32_t *gpid, tpos_t *gye, uint8_t *glast, uint32_t *occw)
{
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= nx) return;
    const uint32_t id = cand_id[k];
    gpid[goff + k] = id; gye[goff + k] = xye[k]; glast[goff + k] = (uint8_t)xlast[k];
    atomicAdd(&occw[id], 1u);
}

// ---- phrases as words of a dictionary image: a saved parse (.dict + .parse; load_parser pfbwt_io.hpp:211-222, init_from_dict_ranks
// pfparser.hpp:549-567) and a shard view without d_ye / d_last (what travels over xGMI is dictionary + word starts + phrase ids only).
// Phrase j is word in[j] - base (base 1: in = the ranks of a .parse, whose dictionary image is in rank order: word id = rank - 1;
// base 0: in = word ids; rank 0 wraps to an id >= dwords); it advances the text by its length minus the w bytes it shares with its
// predecessor, its `last` byte sits in the word.  pid (nullable) takes the word ids.
__global__ __launch_bounds__(BLOCK) void k_word_phrases(const uint32_t *in, uint32_t base, const uint32_t *ws, const uint8_t *dict, uint64_t m, uint32_t dwords, int w, uint32_t *pid, unsigned long long *adv, uint8_t *last, uint32_t *bad)
{
    const uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= m) return;
    const uint32_t id = in[j] - base;
    uint32_t s = 0, len = 0;
    if (id < dwords) { s = ws[id]; len = ws[id + 1] - s - 1u; }
    if (len <= (uint32_t)w) { atomicAdd(bad, 1u); if (pid) pid[j] = 0; adv[j] = 0; last[j] = 0; return; }      // an id outside the dictionary, or a word of at most w bytes
    if (pid) pid[j] = id;
    adv[j] = j ? (unsigned long long)(len - (uint32_t)w) : (unsigned long long)len;      // phrase 0 starts at Y[0] (its Dollar); later ones overlap by w
    last[j] = dict[s + len - (uint32_t)w - 1u];                                          // pfparser.hpp:599
}
__global__ __launch_bounds__(BLOCK) void k_shard_ends(const unsigned long long *adv_ex, const unsigned long long *adv, uint64_t m, tpos_t *ye)
{
    const uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j < m) ye[j] = (tpos_t)(adv_ex[j] + adv[j] - 1ULL);                              // Y coordinate of the phrase's last byte
}
// Phrase ends ye[j] (Y coordinates), last[j] and, if asked for, pid[j] of the m phrases in[] (k_word_phrases); *total = the bytes of
// Y = Dollar + text + w Dollars.  PFP_E_CORRUPT for an id outside the dictionary or a word of at most w bytes.  Scratch: 16 bytes
// per phrase and two counters at the high end, given back.
static int phrase_ends_from_words(pfp_ctx *c, const uint32_t *in, uint32_t base, const uint32_t *ws, const uint8_t *dict, uint64_t m, uint32_t dwords, uint32_t *pid, tpos_t *ye, uint8_t *last, uint64_t *total)
{
    const size_t mk = c->arena.mark_hi();
    unsigned long long *adv, *advx, *d_tot; uint32_t *d_bad;
    PFP_ALLOC_HI(c, adv, unsigned long long, m); PFP_ALLOC_HI(c, advx, unsigned long long, m); PFP_ALLOC_HI(c, d_tot, unsigned long long, 1); PFP_ALLOC_HI(c, d_bad, uint32_t, 1);
    PFP_HIP(c, hipMemsetAsync(d_bad, 0, 4, c->stream));
    PFP_LAUNCH(c, K_MISC, m * 24, k_word_phrases, nblocks(m, BLOCK), in, base, ws, dict, m, dwords, c->w, pid, adv, last, d_bad);
    PFP_TRY((device_scan<unsigned long long, 0>(c, adv, advx, m, d_tot)));
    PFP_LAUNCH(c, K_MISC, m * 24, k_shard_ends, nblocks(m, BLOCK), (const unsigned long long *)advx, (const unsigned long long *)adv, m, ye);
    uint32_t bad = 0; unsigned long long tot = 0;
    PFP_HIP(c, hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipMemcpyAsync(&tot, d_tot, 8, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    if (bad) return PFP_E_CORRUPT;
    c->arena.release_hi(mk);
    *total = tot;
    return PFP_OK;
}
// Word index of every offset of a dictionary image = number of EndOfWord bytes before it (dict_idx.rank, pfbwt.hpp:83-85), and the
// number of words; k_ws_from_flags makes the word starts from wordid.  Scratch: 4 bytes per offset at the high end, given back.
static int dict_word_index(pfp_ctx *c, const uint8_t *d_dict, uint64_t dsize, uint32_t *wordid, uint32_t *nwords)
{
    const size_t mk = c->arena.mark_hi();
    uint32_t *flag, *d_cnt;
    PFP_ALLOC_HI(c, flag, uint32_t, dsize); PFP_ALLOC_HI(c, d_cnt, uint32_t, 1);
    PFP_LAUNCH(c, K_MISC, dsize * 5, k_eow_flags, nblocks(dsize, BLOCK), d_dict, dsize, flag);
    PFP_TRY((device_scan<uint32_t, 0>(c, flag, wordid, dsize, d_cnt)));
    PFP_TRY(d2h_u32(c, d_cnt, nwords));
    c->arena.release_hi(mk);
    return PFP_OK;
}
int pfp_shard_load(pfp_ctx *c, const uint8_t *dict, uint64_t dsize, const uint32_t *parse, uint64_t m)
{
    if (!c || !dict || !parse || dsize < 3 || m < 1) return PFP_E_ARG;
    if (dsize + 64 >= 0xFFFFFFFFULL || m > 0xFFFFFFFEULL - 64) return PFP_E_TOO_LARGE;
    if (dict[dsize - 1] != EndOfDict || dict[dsize - 2] != EndOfWord) return PFP_E_CORRUPT;
    PFP_HIP(c, hipSetDevice(c->device));
    reset_results(c);
    auto body = [&]() -> int {
        // a shard context stays small: merge_pfp may hold thousands of them
        const size_t saved = c->arena_request;
        if (!saved) c->arena_request = (size_t)(dsize * 26 + m * 48 + ((size_t)4 << 20));
        const int ra = ensure_arena(c, 0);
        c->arena_request = saved;
        if (ra != PFP_OK) return ra;
        c->arena.reset();
        PFP_ALLOC_LO(c, c->d_dict, uint8_t, dsize + 16);
        PFP_ALLOC_LO(c, c->d_pid, uint32_t, m); PFP_ALLOC_LO(c, c->d_ye, tpos_t, m); PFP_ALLOC_LO(c, c->d_last, uint8_t, m);
        PFP_HIP(c, hipMemsetAsync(c->d_dict + dsize, 0, 16, c->stream));
        PFP_TRY(h2d_copy(c, c->d_dict, dict, dsize));
        const size_t mk = c->arena.mark_hi();
        uint32_t *wid, *d_parse, nw = 0;
        PFP_ALLOC_HI(c, wid, uint32_t, dsize);
        PFP_TRY(dict_word_index(c, c->d_dict, dsize, wid, &nw));
        if (nw < 1) return PFP_E_CORRUPT;
        PFP_ALLOC_LO(c, c->d_ws, uint32_t, (size_t)nw + 2);
        PFP_LAUNCH(c, K_MISC, dsize * 5, k_ws_from_flags, nblocks(dsize, BLOCK), (const uint8_t *)c->d_dict, dsize, (const uint32_t *)wid, c->d_ws);
        PFP_ALLOC_HI(c, d_parse, uint32_t, m);
        PFP_TRY(h2d_copy(c, (uint8_t *)d_parse, (const uint8_t *)parse, m * 4));
        uint64_t tot = 0;
        PFP_TRY(phrase_ends_from_words(c, d_parse, 1u, c->d_ws, c->d_dict, m, nw, c->d_pid, c->d_ye, c->d_last, &tot));
        if (tot < (uint64_t)c->w + 2) return PFP_E_CORRUPT;
        c->arena.release_hi(mk);
        c->dwords = nw; c->dsize = dsize; c->m = m;
        c->n = tot - 1 - (uint64_t)c->w;                                               // Y holds Dollar + X + w Dollars
        c->left_ctx = 0; c->stage = 1;
        return PFP_OK;
    };
    const int rc = body();
    if (rc != PFP_OK) reset_results(c);
    return rc;
}

int pfp_shard_view_get(pfp_ctx *c, pfp_shard_view *v)
{
    if (!c || !v) return PFP_E_ARG;
    if (c->stage < 1 || !c->d_pid || !c->d_last) return PFP_E_STATE;
    v->n = c->n; v->m = c->m; v->dwords = c->dwords; v->dsize = c->dsize;
    v->d_dict = c->d_dict; v->d_ws = c->d_ws; v->d_pid = c->d_pid; v->d_ye = c->d_ye; v->d_last = c->d_last;
    v->left_context = c->left_ctx;
    return PFP_OK;
}

int pfp_device_copy(pfp_ctx *c, void *d_dst, const void *d_src, uint64_t bytes)
{
    if (!c || (!d_dst && bytes) || (!d_src && bytes)) return PFP_E_ARG;
    PFP_HIP(c, hipSetDevice(c->device));
    if (bytes) PFP_HIP(c, hipMemcpyAsync(d_dst, d_src, (size_t)bytes, hipMemcpyDeviceToDevice, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    return PFP_OK;
}

// the views' own consistency, the interior phrases and the totals; where every shard goes in the global text, the united buffer and the candidates
static int merge_check_views(const pfp_ctx *c, MergePlan &pl)
{
    const uint32_t w = (uint32_t)c->w;
    const pfp_shard_view *v = pl.v;
    uint64_t g = 0;
    for (int r = 0; r < pl.nshards; ++r) {
        const uint64_t lc = v[r].left_context;
        if ((lc != 0 && lc != w) || (r == 0 && lc != 0)) return PFP_E_ARG;
        if (v[r].m < 1 || v[r].n < lc + 1 || !v[r].d_dict || !v[r].d_ws || !v[r].d_pid || (!v[r].d_ye) != (!v[r].d_last)) return PFP_E_ARG;      // d_ye and d_last: both or neither (derived from the words)
        pl.ia[r] = r ? 1 : 0; pl.ib[r] = r + 1 < pl.nshards ? v[r].m - 1 : v[r].m;
        if (pl.ib[r] < pl.ia[r]) pl.ib[r] = pl.ia[r];
        pl.lc[r] = lc; pl.one[r] = v[r].m == 1;
        pl.shift[r] = (tpos_t)(g - lc); g += v[r].n - lc;
        pl.ubase[r] = (uint32_t)pl.dtot; pl.coff[r] = (uint32_t)pl.ctot;
        pl.ntot += v[r].n - lc; pl.mtot += pl.ib[r] - pl.ia[r]; pl.dtot += v[r].dsize; pl.ctot += v[r].dwords;
    }
    if (pl.ntot + w + 64 >= text_limit(c) || pl.dtot + 64 >= 0xFFFFFFFFULL || pl.mtot > 0xFFFFFFFEULL - 64) return PFP_E_TOO_LARGE;
    return PFP_OK;
}
// host: the fragment words of every boundary
static int merge_fetch_fragments(pfp_ctx *c, MergePlan &pl)
{
    const uint32_t w = (uint32_t)c->w;
    const pfp_shard_view *v = pl.v;
    auto fetch_word = [&](const pfp_shard_view &sv, uint32_t id, std::vector<uint8_t> &dst) -> int {
        uint32_t se[2];
        PFP_HIP(c, hipMemcpy(se, sv.d_ws + id, 8, hipMemcpyDeviceToHost));
        dst.resize(se[1] - se[0] - 1);
        if (!dst.empty()) PFP_HIP(c, hipMemcpy(dst.data(), sv.d_dict + se[0], dst.size(), hipMemcpyDeviceToHost));
        return PFP_OK;
    };
    for (int r = 0; r < pl.nshards; ++r) {
        ShardFrag &f = pl.fr[r];
        if (pl.has_head_fragment(r)) {
            PFP_HIP(c, hipMemcpy(&f.id0, v[r].d_pid, 4, hipMemcpyDeviceToHost));
            PFP_TRY(fetch_word(v[r], f.id0, f.w0));
            if (f.w0.size() < 1 + (size_t)w) return PFP_E_CORRUPT;
        }
        if (pl.has_tail_fragment(r)) {
            PFP_HIP(c, hipMemcpy(&f.idl, v[r].d_pid + (v[r].m - 1), 4, hipMemcpyDeviceToHost));
            PFP_TRY(fetch_word(v[r], f.idl, f.wl));
            if (f.wl.size() < (size_t)w) return PFP_E_CORRUPT;
        }
    }
    return PFP_OK;
}
// Junction phrases.  PfParser::operator+= (pfparser.hpp:194-263) pops the last phrase of the left operand, strips its w Dollars and
// goes on appending the first phrase of the right operand without its Dollar (and without the left context, if the shard was
// parsed with one).  A shard that knew its left context has already cut its head at every trigger; a stand-alone shard could
// not trigger in its first w windows (pfparser.hpp:347 "pos_ > w"), so those windows are re-tested here exactly as :226-245 does:
// the hasher starts from w 'A's, a trigger closes the open phrase and the next one starts with the open phrase's real last
// w characters (:241).  The head of a shard with two or more phrases ends in a trigger window and closes the open phrase; the
// head of a one-phrase shard (no window of its own triggered) leaves it open for the next operand -- folding the operands one
// by one, as the reference does, gives the same chain.  All junction phrases are "extra" phrases: pieces[s] = the phrases
// closed while the head of shard s was appended, in text order; they sit between the interior phrases of shards s-1 and s.
// Host data only: fr = the fragment words, lc[s] = left context, one[s] = the shard is one phrase, shift[s] = where it starts globally.
static int junction_pieces(const std::vector<ShardFrag> &fr, const std::vector<uint64_t> &lcs, const std::vector<uint8_t> &ones, const std::vector<tpos_t> &shift, uint32_t w, uint64_t p,
                           std::vector<uint8_t> &junc, std::vector<std::vector<JuncPiece>> &pieces)
{
    const int nshards = (int)fr.size();
    if (nshards < 2) return PFP_OK;
    const DivTest dt = make_divtest(p);
    const uint64_t kmask = trigger_kmask((int)w);
    std::vector<uint8_t> cur;                                              // the open phrase
    if (ones[0]) cur.assign(fr[0].w0.begin(), fr[0].w0.end() - w);         // Dollar + text of shard 0 (its w Dollars stripped, :211-214)
    else cur.assign(fr[0].wl.begin(), fr[0].wl.end() - w);
    for (int s = 1; s < nshards; ++s) {
        const uint32_t lc = (uint32_t)lcs[s];
        const bool one = ones[s] != 0, lastshard = s + 1 == nshards;
        const bool closes = !one || lastshard;                             // the head ends the open phrase (a trigger window, or the end of the text)
        if (fr[s].w0.size() < 1 + (size_t)lc + 1 + ((one && !lastshard) ? (size_t)w : 0)) return PFP_E_CORRUPT;
        const std::vector<uint8_t> head(fr[s].w0.begin() + 1 + lc, fr[s].w0.end() - ((one && !lastshard) ? w : 0));
        const size_t textlen = one && lastshard ? (head.size() >= (size_t)w ? head.size() - w : 0) : head.size();      // head characters that are text (not the final Dollars)
        const tpos_t G = shift[s] + lc;                                    // global index of the head's first character
        auto add_piece = [&](tpos_t ye) -> int {
            if (cur.size() <= (size_t)w) return PFP_E_CORRUPT;
            JuncPiece pc; pc.js = (uint32_t)junc.size(); junc.insert(junc.end(), cur.begin(), cur.end()); pc.je = (uint32_t)junc.size() - 1u;
            pc.ye = ye; pc.last = cur[cur.size() - w - 1];
            pieces[s].push_back(pc);
            return PFP_OK;
        };
        size_t from = 0;                                                   // first head character not yet appended to the open phrase
        if (lc == 0) {
            uint64_t kmer = 0;
            for (uint32_t i = 0; i < w && i < textlen; ++i) {
                const uint8_t ch = head[i];
                const uint64_t code = (ch == 'C') ? 1 : (ch == 'G') ? 2 : (ch == 'T' || ch == '-') ? 3 : 0;      // the text is normalised: A, N -> 0
                kmer = ((kmer << 2) | code) & kmask;
                if (!divisible(wang_hash(kmer), dt)) continue;
                if (closes && (size_t)i + 1 == head.size()) continue;      // the head's own last character ends the phrase anyway
                cur.insert(cur.end(), head.begin() + from, head.begin() + i + 1); from = (size_t)i + 1;
                PFP_TRY(add_piece((tpos_t)(G + i + 1)));
                if (cur.size() < (size_t)w) return PFP_E_ARG;              // (the reference's phrase.erase would throw)
                cur.erase(cur.begin(), cur.end() - w);                     // the next phrase starts with the real last w characters, :241
            }
        }
        cur.insert(cur.end(), head.begin() + from, head.end());
        if (closes) {
            PFP_TRY(add_piece((tpos_t)(G + head.size())));
            if (!lastshard) cur.assign(fr[s].wl.begin(), fr[s].wl.end() - w);      // the next open phrase: this shard's last one without its Dollars
        }
    }
    return PFP_OK;
}
// device: one buffer with all dictionaries + junction words, candidate spans
static int merge_candidates(pfp_ctx *c, const MergePlan &pl, MergeCand &cd)
{
    const int nshards = pl.nshards; const pfp_shard_view *v = pl.v;
    const uint64_t dtot = pl.dtot, ctot = pl.ctot, extra = pl.extra;
    cd.call = ctot + extra;                                                // the shards' words + the junction phrases
    PFP_ALLOC_HI(c, cd.U, uint8_t, dtot + pl.junc.size() + 64);
    PFP_ALLOC_HI(c, cd.cys, uint32_t, cd.call); PFP_ALLOC_HI(c, cd.cye, uint32_t, cd.call); PFP_ALLOC_HI(c, cd.cand_id, uint32_t, cd.call);
    for (int r = 0; r < nshards; ++r) PFP_HIP(c, hipMemcpyAsync(cd.U + pl.ubase[r], v[r].d_dict, (size_t)v[r].dsize, hipMemcpyDeviceToDevice, c->stream));
    if (!pl.junc.empty()) PFP_HIP(c, hipMemcpyAsync(cd.U + dtot, pl.junc.data(), pl.junc.size(), hipMemcpyHostToDevice, c->stream));
    const uint32_t jb = (uint32_t)dtot;
    std::vector<uint32_t> xs, xe, xlast; std::vector<tpos_t> xye;
    cd.xfirst.assign((size_t)nshards + 1, 0);
    for (int s = 0; s < nshards; ++s) {
        cd.xfirst[s] = (uint32_t)xs.size();
        for (const JuncPiece &pc : pl.pieces[s]) { xs.push_back(jb + pc.js); xe.push_back(jb + pc.je); xye.push_back(pc.ye); xlast.push_back(pc.last); }
    }
    cd.xfirst[nshards] = (uint32_t)xs.size();
    for (int r = 0; r < nshards; ++r) {
        // fragment words are referenced by no phrase that is kept: they are re-pointed at the first junction phrase, so that the
        // united dictionary holds no orphan
        const uint32_t fs = extra ? xs[0] : 0u, fe = extra ? xe[0] : 0u;
        PFP_LAUNCH(c, K_MISC, v[r].dwords * 12, k_merge_spans, nblocks(v[r].dwords, BLOCK), v[r].d_ws, (uint32_t)v[r].dwords, pl.ubase[r], pl.coff[r],
                   pl.has_head_fragment(r) ? pl.fr[r].id0 : 0xFFFFFFFFu, fs, fe, pl.has_tail_fragment(r) ? pl.fr[r].idl : 0xFFFFFFFFu, fs, fe, cd.cys, cd.cye);
    }
    if (extra) {
        PFP_ALLOC_HI(c, cd.d_xye, tpos_t, extra); PFP_ALLOC_HI(c, cd.d_xlast, uint32_t, extra);
        PFP_HIP(c, hipMemcpyAsync(cd.cys + ctot, xs.data(), extra * 4, hipMemcpyHostToDevice, c->stream));
        PFP_HIP(c, hipMemcpyAsync(cd.cye + ctot, xe.data(), extra * 4, hipMemcpyHostToDevice, c->stream));
        PFP_HIP(c, hipMemcpyAsync(cd.d_xye, xye.data(), extra * sizeof(tpos_t), hipMemcpyHostToDevice, c->stream));
        PFP_HIP(c, hipMemcpyAsync(cd.d_xlast, xlast.data(), extra * 4, hipMemcpyHostToDevice, c->stream));
        PFP_HIP(c, hipStreamSynchronize(c->stream));                          // the host vectors go out of use below
    }
    return PFP_OK;
}
// Global phrase sequence: junction phrases closed by the head of shard r, then the interior phrases of shard r.  A compact view (no
// d_ye / d_last) gets its phrase ends and last bytes from the shard's own dictionary and phrase ids first.  occw[id] counts the phrases per word.
static int merge_phrase_sequence(pfp_ctx *c, const MergePlan &pl, const MergeCand &cd, uint32_t *occw)
{
    const int nshards = pl.nshards; const pfp_shard_view *v = pl.v;
    std::vector<const tpos_t *> vye((size_t)nshards); std::vector<const uint8_t *> vlast((size_t)nshards);
    for (int r = 0; r < nshards; ++r) {
        vye[r] = v[r].d_ye; vlast[r] = v[r].d_last;
        if (v[r].d_ye) continue;
        tpos_t *ye; uint8_t *la; uint64_t tot = 0;
        PFP_ALLOC_HI(c, ye, tpos_t, v[r].m); PFP_ALLOC_HI(c, la, uint8_t, v[r].m);
        PFP_TRY(phrase_ends_from_words(c, v[r].d_pid, 0u, v[r].d_ws, v[r].d_dict, v[r].m, (uint32_t)v[r].dwords, (uint32_t *)nullptr, ye, la, &tot));
        if (tot != v[r].n + 1 + (uint64_t)c->w) return PFP_E_CORRUPT;          // Y holds Dollar + (context +) text + w Dollars
        vye[r] = ye; vlast[r] = la;
    }
    uint64_t goff = 0;
    for (int r = 0; r < nshards; ++r) {
        const uint32_t nx = cd.xfirst[r + 1] - cd.xfirst[r];
        if (nx) {
            PFP_LAUNCH(c, K_MISC, nx * 24, k_merge_extra, nblocks(nx, BLOCK), (const uint32_t *)cd.cand_id + pl.ctot + cd.xfirst[r], (const tpos_t *)cd.d_xye + cd.xfirst[r], (const uint32_t *)cd.d_xlast + cd.xfirst[r], nx, (uint32_t)goff,
                       c->d_pid, c->d_ye, c->d_last, occw);
            goff += nx;
        }
        const uint32_t cnt = (uint32_t)(pl.ib[r] - pl.ia[r]);
        if (cnt) {
            PFP_LAUNCH(c, K_MISC, cnt * 24, k_merge_phrases, nblocks(cnt, BLOCK), v[r].d_pid, vye[r], vlast[r], (uint32_t)pl.ib[r], (uint32_t)pl.ia[r], (uint32_t)goff, pl.coff[r], pl.shift[r],
                       (const uint32_t *)cd.cand_id, (tpos_t)0, 0u, 0, c->d_pid, c->d_ye, c->d_last, occw);
            goff += cnt;
        }
    }
    if (goff != pl.mtot) return PFP_E_CORRUPT;
    return PFP_OK;
}

static int merge_shards_impl(pfp_ctx *c, int nshards, const pfp_shard_view *v, pfp_parse_sizes *out);
int pfp_merge_shards(pfp_ctx *c, int nshards, const pfp_shard_view *v, pfp_parse_sizes *out)
{
    if (!c || nshards < 1 || !v) return PFP_E_ARG;
    PFP_HIP(c, hipSetDevice(c->device));
    const int rc = merge_shards_impl(c, nshards, v, out);
    if (rc != PFP_OK) reset_results(c);      // a failed merge leaves an empty context (the shards are untouched)
    return rc;
}
static int merge_shards_impl(pfp_ctx *c, int nshards, const pfp_shard_view *v, pfp_parse_sizes *out)
{
    HostTimer timer;
    MergePlan pl(nshards, v);
    PFP_TRY(merge_check_views(c, pl));
    reset_results(c);
    PFP_TRY(ensure_arena(c, pl.ntot + pl.dtot));
    c->arena.reset();
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    const size_t mk = c->arena.mark_hi();
    PFP_TRY(merge_fetch_fragments(c, pl));
    PFP_TRY(junction_pieces(pl.fr, pl.lc, pl.one, pl.shift, (uint32_t)c->w, c->p, pl.junc, pl.pieces));
    for (const auto &ps : pl.pieces) pl.extra += ps.size();
    if (pl.mtot + pl.extra > 0xFFFFFFFEULL - 64) return PFP_E_TOO_LARGE;
    pl.mtot += pl.extra;
    MergeCand cd;
    PFP_TRY(merge_candidates(c, pl, cd));
    // global distinct words, dictionary
    Spans sp; sp.ye = nullptr; sp.ys32 = cd.cys; sp.ye32 = cd.cye; sp.w = 0;
    uint64_t dwords = 0; uint32_t *rep, *occ_cand, *occw;
    PFP_TRY(dedup_strings(c, cd.U, sp, cd.call, pl.dtot + pl.junc.size(), cd.cand_id, &dwords, &rep, &occ_cand, (uint8_t *)nullptr, DedupText{nullptr, nullptr, 0, nullptr}));      // (a dictionary, not a scanned text: bytes)
    PFP_TRY(build_dictionary(c, cd.U, sp, rep, dwords));
    c->n = pl.ntot; c->m = pl.mtot;
    PFP_ALLOC_LO(c, c->d_pid, uint32_t, pl.mtot); PFP_ALLOC_LO(c, c->d_ye, tpos_t, pl.mtot); PFP_ALLOC_LO(c, c->d_last, uint8_t, pl.mtot);
    PFP_ALLOC_HI(c, occw, uint32_t, dwords);
    PFP_HIP(c, hipMemsetAsync(occw, 0, dwords * 4, c->stream));
    PFP_TRY(merge_phrase_sequence(c, pl, cd, occw));
    PFP_TRY(finish_parse(c, occw));
    return parse_done(c, mk, timer, out);
}

int pfp_parse_get(pfp_ctx *c, uint8_t *dict, void *occ, uint32_t *parse, uint8_t *last, void *sai)
{
    if (!c) return PFP_E_ARG;
    if (c->stage < 1 || !c->d_sdict) return PFP_E_STATE;
    PFP_HIP(c, hipSetDevice(c->device));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    const bool u64 = (c->flags & PFP_FLAG_U64) != 0;
    if (dict) PFP_HIP(c, hipMemcpy(dict, c->d_sdict, c->dsize, hipMemcpyDeviceToHost));
    PFP_TRY(download_as_u(c, c->d_occ, c->dwords, occ, u64));
    if (parse) PFP_HIP(c, hipMemcpy(parse, c->d_parse, c->m * 4, hipMemcpyDeviceToHost));
    if (last) PFP_HIP(c, hipMemcpy(last, c->d_last, c->m, hipMemcpyDeviceToHost));
    PFP_TRY(download_as_u(c, c->d_ye, c->m, sai, u64));   // sai[j] = pos_ at process_phrase = ye[j]  (pfparser.hpp:600)
    return PFP_OK;
}

// ---- stage 2: the BWT of the parse ------------------------------------------------------------------------------------------------
static int parse_bwt_impl(pfp_ctx *c);
int pfp_parse_bwt(pfp_ctx *c)
{
    if (!c) return PFP_E_ARG;
    if (c->stage < 1 || !c->d_parse) return PFP_E_STATE;
    if (c->m < 2) return PFP_E_ONE_WORD;                        // pfparser.hpp:390-392
    PFP_HIP(c, hipSetDevice(c->device));
    c->arena.release_lo(c->lo_after_parse);
    ArenaGuard g(c);
    const int rc = g.done(parse_bwt_impl(c));
    if (rc != PFP_OK) { c->stage = 1; c->d_bwlast = nullptr; c->d_ilist = nullptr; c->d_bwsai = nullptr; c->d_bwl_il = nullptr; c->nrows = 0; }
    return rc;
}
static int parse_bwt_impl(pfp_ctx *c)
{
    HostTimer timer;
    const uint64_t m = c->m, N = m + 1;
    const size_t mk = c->arena.mark_hi();
    PFP_LAUNCH(c, K_MISC, 4, k_set_u32, 1, c->d_parse, m, 0u);  // :407-410 (d_parse has m+1 slots)
    uint32_t *SAP, *W, *rowid, *W2, *rowid2, *rk;
    PFP_ALLOC_LO(c, c->d_bwlast, uint8_t, N);
    PFP_ALLOC_LO(c, c->d_ilist, uint32_t, N);
    const bool sai = (c->flags & PFP_FLAG_SAI) != 0;
    if (sai) PFP_ALLOC_LO(c, c->d_bwsai, tpos_t, N); else c->d_bwsai = nullptr;
    PFP_ALLOC_LO(c, c->d_bwl_il, uint8_t, N);
    uint32_t *d_bad; PFP_ALLOC_HI(c, d_bad, uint32_t, 1);
    PFP_HIP(c, hipMemsetAsync(d_bad, 0, 4, c->stream));
    const int pack = N <= (1ULL << BWL_SHIFT) ? 1 : 0;
    PFP_ALLOC_HI(c, SAP, uint32_t, N); PFP_ALLOC_HI(c, rk, uint32_t, N);
    PFP_ALLOC_HI(c, W, uint32_t, N); PFP_ALLOC_HI(c, rowid, uint32_t, N);
    PFP_ALLOC_HI(c, W2, uint32_t, N); PFP_ALLOC_HI(c, rowid2, uint32_t, N);
    int rounds = 0;
    PFP_TRY(sort_int_suffixes(c, c->d_parse, N, c->dwords, SAP, rk, &rounds, 0, false));   // sacak_int, :425 (recsort.h; the ranks are not asked for)
    {
        uint4 *rec; PFP_ALLOC_HI(c, rec, uint4, m);
        PFP_LAUNCH(c, K_PBWT_ROWS, m * 29, k_pbwt_pack, nblocks(m, BLOCK), (const uint32_t *)c->d_parse, (const uint8_t *)c->d_last, sai ? (const tpos_t *)c->d_ye : (const tpos_t *)nullptr, m, rec);
        PFP_LAUNCH(c, K_PBWT_ROWS, N * (4 + 16 + 17), k_pbwt_rows, nblocks(N, BLOCK), (const uint32_t *)SAP, (const uint4 *)rec, m, c->d_bwlast, c->d_bwsai, W, rowid, pack, d_bad);
    }
    // ilist: rows grouped by word, ascending inside a word (:452-462) = stable sort of row ids by word
    BitRange wr = {0, bits_for(c->dwords)};
    uint32_t *sw, *sr;
    PFP_TRY(radix_sort_pairs<uint32_t>(c, W, rowid, W2, rowid2, N, &wr, 1, &sw, &sr));
    uint32_t bad = 0;
    if (pack) PFP_TRY(d2h_u32(c, d_bad, &bad));
    if (pack && !bad) PFP_LAUNCH(c, K_PBWT_ROWS, N * 9, k_ilist_split, nblocks(N, BLOCK), (const uint32_t *)sr, N, c->d_ilist, c->d_bwl_il);
    else PFP_LAUNCH(c, K_PBWT_ROWS, N * 10, k_ilist_gather, nblocks(N, BLOCK), (const uint32_t *)sr, N, pack ? (1u << BWL_SHIFT) - 1u : 0xFFFFFFFFu, (const uint8_t *)c->d_bwlast, c->d_ilist, c->d_bwl_il);
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    c->arena.release_hi(mk);
    c->nrows = N; c->stage = 2;
    c->lo_after_pbwt = c->arena.mark_lo();
    c->stage_ms[1] = timer.ms();
    return PFP_OK;
}

int pfp_parse_bwt_get(pfp_ctx *c, uint8_t *bwlast, void *ilist, void *bwsai)
{
    if (!c) return PFP_E_ARG;
    if (c->stage < 2) return PFP_E_STATE;
    PFP_HIP(c, hipSetDevice(c->device));
    const bool u64 = (c->flags & PFP_FLAG_U64) != 0;
    if (bwlast) PFP_HIP(c, hipMemcpy(bwlast, c->d_bwlast, c->nrows, hipMemcpyDeviceToHost));
    PFP_TRY(download_as_u(c, c->d_ilist, c->nrows, ilist, u64));
    if (bwsai) { if (!c->d_bwsai) return PFP_E_STATE; PFP_TRY(download_as_u(c, c->d_bwsai, c->nrows, bwsai, u64)); }
    return PFP_OK;
}

// ---- the files of a finished stage 2 ------------------------------------------------------------------------------------------------
// consistency of a loaded file set (the emission gathers ilist[F[rank] + r], bwsai[q], bwlast[q] with these values as
// indices: a truncated or mismatched set must become PFP_E_CORRUPT here, not an out-of-bounds device read there)
__global__ __launch_bounds__(BLOCK) void k_load_check(const uint32_t *ilist, uint64_t nrows, const uint32_t *occ, uint64_t dwords, unsigned long long *out /*[0] sum of occ, [1] ilist entries >= nrows*/)
{
    __shared__ unsigned long long red[4];
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    unsigned long long tot;
    (void)block_excl_sum((unsigned long long)(i < dwords ? occ[i] : 0u), red, &tot);
    if (threadIdx.x == 0 && tot) atomicAdd(&out[0], tot);
    (void)block_excl_sum((unsigned long long)((i < nrows && ilist[i] >= nrows) ? 1u : 0u), red, &tot);
    if (threadIdx.x == 0 && tot) atomicAdd(&out[1], tot);
}

static int bwt_load_impl(pfp_ctx *c, const uint8_t *dict, uint64_t dsize, const void *occ, uint64_t dwords,
                         const uint8_t *bwlast, const void *ilist, const void *bwsai, uint64_t nrows, uint64_t n_hint);
int pfp_bwt_load(pfp_ctx *c, const uint8_t *dict, uint64_t dsize, const void *occ, uint64_t dwords,
                 const uint8_t *bwlast, const void *ilist, const void *bwsai, uint64_t nrows, uint64_t n_hint)
{
    if (!c || !dict || !occ || !bwlast || !ilist || dsize < 2 || dwords < 1 || nrows < 2) return PFP_E_ARG;
    if (dsize + 64 >= 0xFFFFFFFFULL || nrows + 64 >= 0xFFFFFFFFULL) return PFP_E_TOO_LARGE;
    if (dict[dsize - 1] != EndOfDict || dict[dsize - 2] != EndOfWord) return PFP_E_CORRUPT;       // pfbwt_io.hpp:71-82
    if (n_hint && nrows > n_hint + 1) return PFP_E_CORRUPT;                                       // more phrases than text positions
    PFP_HIP(c, hipSetDevice(c->device));
    reset_results(c);
    const int rc = bwt_load_impl(c, dict, dsize, occ, dwords, bwlast, ilist, bwsai, nrows, n_hint);
    if (rc != PFP_OK) reset_results(c);
    return rc;
}
static int bwt_load_impl(pfp_ctx *c, const uint8_t *dict, uint64_t dsize, const void *occ, uint64_t dwords,
                         const uint8_t *bwlast, const void *ilist, const void *bwsai, uint64_t nrows, uint64_t n_hint)
{
    // n (the .n file, src/pfbwt-f.cpp:282-285) sizes the outputs; without it assume n <= 4 * dsize
    PFP_TRY(ensure_arena(c, (n_hint ? n_hint : 4 * dsize) + dsize + nrows));
    c->arena.reset();
    const bool u64 = (c->flags & PFP_FLAG_U64) != 0;
    c->dsize = dsize; c->dwords = dwords; c->nrows = nrows; c->m = nrows - 1;
    PFP_ALLOC_LO(c, c->d_dict, uint8_t, dsize + 16);
    PFP_ALLOC_LO(c, c->d_wordid, uint32_t, dsize);
    PFP_ALLOC_LO(c, c->d_ws, uint32_t, dwords + 2);
    PFP_ALLOC_LO(c, c->d_occ, uint32_t, dwords);
    PFP_ALLOC_LO(c, c->d_bwlast, uint8_t, nrows);
    PFP_ALLOC_LO(c, c->d_ilist, uint32_t, nrows);
    PFP_HIP(c, hipMemcpy(c->d_dict, dict, dsize, hipMemcpyHostToDevice));
    PFP_HIP(c, hipMemcpy(c->d_bwlast, bwlast, nrows, hipMemcpyHostToDevice));
    PFP_TRY(upload_from_u(c, occ, dwords, u64, c->d_occ));
    PFP_TRY(upload_from_u(c, ilist, nrows, u64, c->d_ilist));
    if (bwsai) {
        PFP_ALLOC_LO(c, c->d_bwsai, tpos_t, nrows);
        PFP_TRY(upload_from_u(c, bwsai, nrows, u64, c->d_bwsai));
    }
    const size_t mk = c->arena.mark_hi();
    uint32_t nw = 0;
    PFP_TRY(dict_word_index(c, c->d_dict, dsize, c->d_wordid, &nw));
    if (nw != dwords) return PFP_E_CORRUPT;
    PFP_LAUNCH(c, K_MISC, dsize * 5, k_ws_from_flags, nblocks(dsize, BLOCK), (const uint8_t *)c->d_dict, dsize, (const uint32_t *)c->d_wordid, c->d_ws);
    {   // sum(occ) + 1 == rows of the parse BWT (pfparser.hpp:452-462), every ilist entry is a row
        unsigned long long *d_chk, chk[2];
        PFP_ALLOC_HI(c, d_chk, unsigned long long, 2);
        PFP_HIP(c, hipMemsetAsync(d_chk, 0, 16, c->stream));
        PFP_LAUNCH(c, K_MISC, (nrows + dwords) * 4, k_load_check, nblocks(nrows > dwords ? nrows : dwords, BLOCK), (const uint32_t *)c->d_ilist, nrows, (const uint32_t *)c->d_occ, dwords, d_chk);
        PFP_HIP(c, hipMemcpyAsync(chk, d_chk, 16, hipMemcpyDeviceToHost, c->stream));
        PFP_HIP(c, hipStreamSynchronize(c->stream));
        if (chk[0] + 1 != nrows || chk[1] != 0) return PFP_E_CORRUPT;
    }
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    c->arena.release_hi(mk);
    c->d_wrank = nullptr; c->gsa_valid = false; c->stage = 2; c->n = n_hint;     // n known: the emission checks that it produces exactly n + 1 rows
    c->lo_after_pbwt = c->arena.mark_lo();
    return PFP_OK;
}
} // extern "C"
