// pfbwt-f_amd/csrc/panel_host.h -- host side of the variant-panel feed (pfp_parse_feed_panel; kernels: csrc/panel.h) and the VCF file
// feed on top of it (pfp_parse_feed_vcf_file; reader: csrc/vcfread.h).  Included by pfbwt_hip.hip (ensure_arena) behind feed_host.h, whose
// append path it uses (feed_open, flush_view, append_reserve, append_done, h2d_copy).
#pragma once

// What the host decides before anything is uploaded: the argument checks of the header and the kept sites (vcf_scan.cpp:175-213 --
// geometry only, so once per site and not once per haplotype).
struct PanelPlan {
    std::vector<uint64_t> krpos, kafirst, tfirst, tk0; std::vector<uint32_t> kspan, ksite, knalt, snalt, tcontig;
    uint64_t skipped = 0;
};
static int panel_plan(const pfp_panel *P, uint32_t tile, PanelPlan *pl)
{
    if (P->ncontigs && (!P->ref_off || !P->site_first)) return PFP_E_ARG;
    if (P->ncontigs >= (1ULL << 32) || P->nhap >= (1ULL << 32) - 1 || (P->nhap + 1) * P->ncontigs >= (1ULL << 32) || P->nsites >= (1ULL << 32)) return PFP_E_TOO_LARGE;
    if (!P->ncontigs) return P->nsites ? PFP_E_ARG : PFP_OK;
    for (uint64_t c = 0; c < P->ncontigs; ++c) if (P->ref_off[c + 1] < P->ref_off[c] || P->site_first[c + 1] < P->site_first[c]) return PFP_E_ARG;
    if (P->site_first[0] != 0 || P->site_first[P->ncontigs] != P->nsites) return PFP_E_ARG;
    if (P->ref_off[P->ncontigs] > P->ref_off[0] && !P->ref) return PFP_E_ARG;
    if (P->nsites && (!P->pos || !P->span || !P->allele_first || (P->nhap && !P->gt))) return PFP_E_ARG;
    if (P->nalt && !P->alt_off) return PFP_E_ARG;
    for (uint64_t a = 0; a < P->nalt; ++a) if (P->alt_off[a + 1] < P->alt_off[a]) return PFP_E_ARG;
    if (P->nalt && P->alt_off[P->nalt] > P->alt_off[0] && !P->alt_bytes) return PFP_E_ARG;
    for (uint64_t v = 0; v < P->nsites; ++v) if (P->allele_first[v + 1] < P->allele_first[v]) return PFP_E_ARG;
    if (P->nsites && P->allele_first[P->nsites] > P->nalt) return PFP_E_ARG;
    pl->snalt.resize((size_t)P->nsites); pl->tfirst.assign(1, 0);
    for (uint64_t c = 0; c < P->ncontigs; ++c) {
        const uint64_t clen = P->ref_off[c + 1] - P->ref_off[c], kc0 = pl->krpos.size();
        uint64_t end = 0, prev = 0;
        for (uint64_t v = P->site_first[c]; v < P->site_first[c + 1]; ++v) {
            const uint64_t pos = P->pos[v], na = P->allele_first[v + 1] - P->allele_first[v];
            if (pos < prev || pos > clen || P->span[v] > clen - pos) return PFP_E_ARG;
            prev = pos;
            pl->snalt[(size_t)v] = na > 255 ? 255u : (uint32_t)na;      // a genotype is a byte
            if (pos < end) { ++pl->skipped; continue; }
            end = pos + P->span[v];
            pl->krpos.push_back(P->ref_off[c] + pos); pl->kspan.push_back(P->span[v]); pl->ksite.push_back((uint32_t)v);
            pl->knalt.push_back(pl->snalt[(size_t)v]); pl->kafirst.push_back(P->allele_first[v]);
        }
        for (uint64_t k = kc0; k < pl->krpos.size(); k += tile) { pl->tk0.push_back(k); pl->tcontig.push_back((uint32_t)c); }
        pl->tfirst.push_back(pl->tk0.size());
    }
    pl->tk0.push_back(pl->krpos.size());
    return PFP_OK;
}

template <typename T> static int panel_upload(pfp_ctx *c, const T **d, const T *h, uint64_t count)
{
    T *p; PFP_ALLOC_HI(c, p, T, count + 16 / sizeof(T));      // 16 bytes of slack: no array ends where the next page is not mapped
    *d = p;
    return h2d_copy(c, (uint8_t *)p, (const uint8_t *)h, count * sizeof(T));
}

static int feed_panel_impl(pfp_ctx *c, const pfp_panel *P, unsigned flags, const PanelPlan &pl, pfp_panel_info *info, std::vector<uint64_t> *starts)
{
    using namespace pfp;
    const uint32_t ref_first = (flags & PFP_PANEL_REF_FIRST) ? 1u : 0u;
    const uint64_t nrec = (P->nhap + ref_first) * P->ncontigs, nk = pl.krpos.size(), ntiles = pl.tcontig.size();
    if (!nrec) return PFP_OK;
    PanelDev D = {};
    D.nhap = P->nhap; D.ntiles = ntiles; D.nkept = nk; D.ncontigs = (uint32_t)P->ncontigs; D.nrec = (uint32_t)nrec; D.ref_first = ref_first; D.w = (uint32_t)c->w;
    const uint32_t *d_snalt = nullptr;
    PFP_TRY(panel_upload(c, &D.ref, P->ref, P->ref_off[P->ncontigs]));
    PFP_TRY(panel_upload(c, &D.ref_off, P->ref_off, P->ncontigs + 1));
    PFP_TRY(panel_upload(c, &D.krpos, pl.krpos.data(), nk));
    PFP_TRY(panel_upload(c, &D.kspan, pl.kspan.data(), nk));
    PFP_TRY(panel_upload(c, &D.ksite, pl.ksite.data(), nk));
    PFP_TRY(panel_upload(c, &D.knalt, pl.knalt.data(), nk));
    PFP_TRY(panel_upload(c, &D.kafirst, pl.kafirst.data(), nk));
    PFP_TRY(panel_upload(c, &D.alt_off, P->alt_off, P->nalt ? P->nalt + 1 : 0));
    PFP_TRY(panel_upload(c, &D.alt_bytes, P->alt_bytes, P->nalt ? P->alt_off[P->nalt] : 0));
    PFP_TRY(panel_upload(c, &D.gt, P->gt, P->nsites * P->nhap));
    PFP_TRY(panel_upload(c, &d_snalt, pl.snalt.data(), P->nsites));
    PFP_TRY(panel_upload(c, &D.tfirst, pl.tfirst.data(), P->ncontigs + 1));
    PFP_TRY(panel_upload(c, &D.tk0, pl.tk0.data(), ntiles + 1));
    PFP_TRY(panel_upload(c, &D.tcontig, pl.tcontig.data(), ntiles));
    PFP_ALLOC_HI(c, D.dir, uint64_t, ntiles * P->nhap);
    PFP_ALLOC_HI(c, D.rstart, uint64_t, nrec + 3);
    PFP_HIP(c, hipMemsetAsync(D.rstart + nrec + 1, 0, 8, c->stream));
    PFP_HIP(c, hipMemsetAsync(D.rstart + nrec + 2, 0xFF, 8, c->stream));

    // the genotypes are checked before anything is derived from them
    const uint64_t ngt = P->nsites * P->nhap;
    if (ngt / 16 / BLOCK >= 0x7FFFFFFFULL || ntiles * P->nhap / BLOCK >= 0x7FFFFFFFULL) return PFP_E_TOO_LARGE;
    if (ngt) PFP_LAUNCH(c, K_PANEL_CHECK, ngt, k_panel_check_gt, nblocks(ngt, 16 * BLOCK), D.gt, d_snalt, P->nhap, ngt, (unsigned long long *)(D.rstart + nrec + 2));
    // lengths and the site directory, then the record starts
    if (ntiles * P->nhap) PFP_LAUNCH(c, K_PANEL_DIR, nk * P->nhap + 8 * ntiles * P->nhap, k_panel_tile_delta, nblocks(ntiles * P->nhap, BLOCK), D);
    PFP_LAUNCH(c, K_PANEL_DIR, 16 * ntiles * P->nhap + 8 * nrec, k_panel_record_lengths, nblocks(P->ncontigs * (P->nhap + ref_first), BLOCK), D);
    PFP_TRY((device_scan<uint64_t, 0>(c, D.rstart, D.rstart, nrec, D.rstart + nrec)));
    // the one fetch: record starts, their total, the ALT count and the genotype verdict
    starts->resize((size_t)nrec + 3);
    PFP_HIP(c, hipMemcpyAsync(starts->data(), D.rstart, (size_t)(nrec + 3) * 8, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    const uint64_t total = (*starts)[(size_t)nrec], applied = (*starts)[(size_t)nrec + 1], bad = (*starts)[(size_t)nrec + 2];
    if (bad != ~0ULL) { c->err_pos = bad; c->err_ch = P->gt[bad]; return PFP_E_ARG; }
    const uint32_t ob = c->tun.panel_out_bytes;
    const uint64_t base = c->n, nchunks = (base + total - (base & ~15ULL) + ob - 1) / ob;
    uint64_t stripes = c->tun.panel_swizzle ? P->nhap + ref_first : 1;
    if (stripes > nchunks) stripes = nchunks;
    const uint64_t per = (nchunks + stripes - 1) / stripes;
    if (stripes * per >= 0x7FFFFFFFULL) return PFP_E_TOO_LARGE;      // grid limit
    PFP_TRY(append_reserve(c, total));      // (PFP_E_TOO_LARGE by the bound of every feed: pfparser.hpp:326-331 for the 32-bit build, 2^40 for the 64-bit one)
    PFP_LAUNCH(c, K_PANEL_FILL, 2 * total, k_panel_fill, stripes * per, D, c->tb + 16, base, total, ob, nchunks, stripes, per);
    PFP_HIP(c, hipStreamSynchronize(c->stream));      // the scratch goes back to the arena on return
    if (info) {
        info->alt_applied = applied; info->bases = total; info->records = nrec;
        info->min_record = ~0ULL; info->max_record = 0;
        for (uint64_t r = 0; r < nrec; ++r) {
            const uint64_t len = (*starts)[(size_t)r + 1] - (*starts)[(size_t)r] - (uint64_t)c->w;
            if (len < info->min_record) info->min_record = len;
            if (len > info->max_record) info->max_record = len;
        }
    }
    starts->resize((size_t)nrec);
    append_done(c, total, nrec);
    return PFP_OK;
}

extern "C" {

int pfp_parse_feed_panel(pfp_ctx *c, const pfp_panel *P, unsigned flags, pfp_panel_info *info)
{
    if (!c || !P || (flags & ~(PFP_PANEL_REF_FIRST | PFP_PANEL_RECORDS))) return PFP_E_ARG;
    PanelPlan pl;
    PFP_TRY(panel_plan(P, c->tun.panel_tile, &pl));
    PFP_TRY(feed_open(c));
    PFP_TRY(flush_view(c));
    if (info) { *info = pfp_panel_info(); info->contigs = P->ncontigs; info->haplotypes = P->nhap; info->sites = P->nsites; info->kept = pl.krpos.size(); info->skipped_overlap = pl.skipped; }
    std::vector<uint64_t> starts;
    const uint64_t base = c->n;
    // scratch (the uploaded inputs, the directory) lives at the arena's high end for the length of the call
    const uint64_t up = P->ncontigs ? P->ref_off[P->ncontigs] + P->nsites * P->nhap + (P->nalt ? P->alt_off[P->nalt] : 0) + 40 * P->nsites + 8 * P->nalt + 8 * pl.tcontig.size() * (P->nhap + 3) + 16 * P->ncontigs + 8 * (P->nhap + 1) * P->ncontigs : 0;
    // The workspace is sized here for the text this call appends, not only for its scratch: every haplotype is at most the reference plus every
    // ALT byte once, so pfp_parse_finalize finds a range that is large enough and does not reserve a second one right behind this call.
    unsigned __int128 tb128 = 0;
    if (P->ncontigs) tb128 = (unsigned __int128)(P->nhap + 1) * (P->ref_off[P->ncontigs] + P->ncontigs * (uint64_t)c->w) + (unsigned __int128)P->nhap * (P->nalt ? P->alt_off[P->nalt] : 0);
    const uint64_t text_bound = tb128 > ((unsigned __int128)1 << 40) ? (1ULL << 40) : (uint64_t)tb128;      // (beyond the width's limit the call fails anyway)
    c->arena.want = 0;
    if (!c->arena.base || c->arena.hi - c->arena.lo < up + ((size_t)1 << 20)) PFP_TRY(ensure_arena(c, c->n + text_bound + up / 64 + 1));      // (a workspace that holds the scratch is kept as it is)
    pfp::ArenaGuard g(c);
    const size_t mk = c->arena.mark_hi();
    const int rc = g.done(feed_panel_impl(c, P, flags, pl, info, &starts));
    if (rc == PFP_OK) c->arena.release_hi(mk);
    if (rc != PFP_OK) { if (info) info->records = info->bases = info->alt_applied = info->min_record = info->max_record = 0; return rc; }
    if (flags & PFP_PANEL_RECORDS) {
        if (!base) { c->doc_names.clear(); c->doc_starts.clear(); }
        const uint64_t ref_first = (flags & PFP_PANEL_REF_FIRST) ? 1 : 0;
        auto cname = [&](uint64_t k) { return (P->contig_names && P->contig_names[k]) ? std::string(P->contig_names[k]) : "c" + std::to_string(k); };
        for (uint64_t r = 0; r < starts.size(); ++r) {
            const bool is_ref = ref_first && r < P->ncontigs;
            const uint64_t rr = is_ref ? r : r - ref_first * P->ncontigs, h = rr / P->ncontigs, k = rr % P->ncontigs;
            c->doc_names.push_back(is_ref ? cname(k) : ((P->hap_names && P->hap_names[h]) ? std::string(P->hap_names[h]) : "h" + std::to_string(h)) + "." + cname(k));
            c->doc_starts.push_back(base + starts[(size_t)r]);
        }
    }
    return PFP_OK;
}

// ---- reference FASTA + VCF (csrc/vcfread.h) -------------------------------------------------------------------------------------------
int pfp_parse_feed_vcf_file(pfp_ctx *c, const char *ref_fasta, const char *vcf, const char *samples, unsigned flags, pfp_vcf_info *info)
{
    if (!c || !ref_fasta || !vcf || (flags & ~(PFP_PANEL_REF_FIRST | PFP_PANEL_RECORDS))) return PFP_E_ARG;
    pfpvcf::Panel V;
    int rc = pfpvcf::load_fasta(ref_fasta, &V);
    if (rc != pfpvcf::VCF_OK) return rc;
    uint64_t line = 0;
    rc = pfpvcf::load_vcf(vcf, samples, &V, &line);
    if (rc == pfpvcf::VCF_E_CORRUPT) { c->err_pos = line; c->err_ch = 0; }
    if (rc != pfpvcf::VCF_OK) return rc;
    std::vector<const char *> cn, hn;
    for (auto &s : V.contig_names) cn.push_back(s.c_str());
    for (auto &s : V.hap_names) hn.push_back(s.c_str());
    pfp_panel P = {};
    P.ncontigs = V.contig_names.size(); P.ref = (const uint8_t *)V.ref.data(); P.ref_off = V.ref_off.data(); P.contig_names = cn.data();
    P.nsites = V.pos.size(); P.site_first = V.site_first.data(); P.pos = V.pos.data(); P.span = V.span.data(); P.allele_first = V.allele_first.data();
    P.nalt = V.alt_off.size() - 1; P.alt_off = V.alt_off.data(); P.alt_bytes = (const uint8_t *)V.alt_bytes.data();
    P.nhap = V.nhap; P.gt = V.gt.data(); P.hap_names = hn.data();
    pfp_panel_info pi = pfp_panel_info();
    rc = pfp_parse_feed_panel(c, &P, flags, &pi);
    if (info) { info->lines = V.lines; info->samples = V.samples; info->skipped_symbolic = V.skipped_symbolic; info->missing_gt = V.missing_gt; info->panel = pi; }
    return rc;
}

} // extern "C"
