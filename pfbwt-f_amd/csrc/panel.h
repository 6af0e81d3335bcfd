// pfbwt-f_amd/csrc/panel.h -- variant-panel feed on the device (include/pfbwt_hip.h: pfp_parse_feed_panel): the haplotype records of a
// reference + variant sites + genotype matrix are written straight into the text buffer.
//
// Stands in for the reference's front end: src/vcf_scan.cpp:175-213 (the consensus of one haplotype: a site is applied iff its position
// is not in front of the end of the last applied site), run once per haplotype by vcf_to_bwt.py:191-242, whose outputs go through
// pfbwt-f64 --parse-only one by one.  Here the kept sites are decided once on the host (geometry only), and three device steps follow:
//   k_panel_tile_delta / k_panel_record_lengths   the length change of every (tile of kept sites, haplotype), then its exclusive sum
//                                                 along each contig -- the site directory, one value per tile border -- and the record lengths
//   device_scan                                   record starts = exclusive sum of (length + w) in output order
//   k_panel_fill                                  output-stationary: a workgroup owns a 16-byte aligned range of the text, finds the
//                                                 (record, tile) pairs that meet it, rebuilds the tile's site starts in LDS and copies
// No array of sites x haplotypes exists besides the genotype bytes themselves.
#pragma once
#include "prims.h"

namespace pfp {

constexpr uint32_t PANEL_TILE_MAX = 2 * BLOCK;      // kept sites per directory tile: two per thread of the workgroup that rebuilds it
constexpr uint32_t PANEL_TILE_DEFAULT = 256;
constexpr uint32_t PANEL_OUT_MIN = 256;             // output bytes per workgroup (a multiple of 16)
constexpr uint32_t PANEL_OUT_DEFAULT = 16384;       // four 16-byte stores per thread for every tile rebuilt (not measured against other sizes)

struct PanelDev {
    const uint8_t *ref; const uint64_t *ref_off;      // ncontigs + 1
    const uint64_t *krpos;                            // per kept site: offset of the site in `ref`
    const uint32_t *kspan, *ksite, *knalt;            // ... reference bytes replaced, row of gt, ALT alleles
    const uint64_t *kafirst;                          // ... number of its first ALT string in alt_off
    const uint64_t *alt_off; const uint8_t *alt_bytes;
    const uint8_t *gt; uint64_t nhap;
    const uint64_t *tfirst;                           // ncontigs + 1: first tile of every contig
    const uint64_t *tk0;                              // ntiles + 1: first kept site of every tile (tiles never straddle contigs)
    const uint32_t *tcontig;                          // ntiles
    uint64_t *dir;                                    // ntiles * nhap, [t * nhap + h]: length change in front of tile t in record (h, contig of t)
    uint64_t *rstart;                                 // nrec + 1 record starts (relative to the first); [nrec + 1] ALT alleles applied, [nrec + 2] first bad genotype
    uint64_t ntiles, nkept;
    uint32_t ncontigs, nrec, ref_first, w;
};

// a genotype must name an allele of its site: the smallest offending index into gt wins
__global__ __launch_bounds__(BLOCK) void k_panel_check_gt(const uint8_t *gt, const uint32_t *snalt, uint64_t nhap, uint64_t total, unsigned long long *bad)
{
    const uint64_t i0 = ((uint64_t)blockIdx.x * BLOCK + threadIdx.x) * 16;
    if (i0 >= total) return;
    uint8_t v[16];
    const uint32_t cnt = total - i0 < 16 ? (uint32_t)(total - i0) : 16u;
    if (cnt == 16) __builtin_memcpy(v, gt + i0, 16);
    else for (uint32_t k = 0; k < cnt; ++k) v[k] = gt[i0 + k];
    uint64_t site = i0 / nhap, h = i0 - site * nhap;
    uint32_t lim = snalt[site];
    for (uint32_t k = 0; k < cnt; ++k) {
        if (v[k] > lim) { atomicMin(bad, (unsigned long long)(i0 + k)); return; }
        if (++h == nhap && k + 1 < cnt) { h = 0; lim = snalt[++site]; }
    }
}

// length of the allele that genotype g selects at kept site k, and where its bytes are
__device__ __forceinline__ uint64_t panel_allele(const PanelDev &P, uint64_t k, uint32_t g, const uint8_t **src)
{
    if (g == 0 || g > P.knalt[k]) { *src = P.ref + P.krpos[k]; return P.kspan[k]; }
    const uint64_t a = P.kafirst[k] + g - 1, o = P.alt_off[a];
    *src = P.alt_bytes + o;
    return P.alt_off[a + 1] - o;
}

// one thread per (tile, haplotype), haplotypes along the lanes (the genotype rows are read coalesced)
__global__ __launch_bounds__(BLOCK) void k_panel_tile_delta(PanelDev P)
{
    const uint64_t x = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (x >= P.ntiles * P.nhap) return;
    const uint64_t t = x / P.nhap, h = x - t * P.nhap;
    uint64_t d = 0, applied = 0;
    for (uint64_t k = P.tk0[t]; k < P.tk0[t + 1]; ++k) {
        const uint32_t g = P.gt[(uint64_t)P.ksite[k] * P.nhap + h];
        if (!g) continue;
        const uint8_t *src; d += panel_allele(P, k, g, &src) - P.kspan[k]; ++applied;
    }
    P.dir[x] = d;
    if (applied) atomicAdd((unsigned long long *)&P.rstart[P.nrec + 1], (unsigned long long)applied);
}

// one thread per (contig, haplotype): the tiles' changes become their exclusive sums; record length + w into rstart (scanned next)
__global__ __launch_bounds__(BLOCK) void k_panel_record_lengths(PanelDev P)
{
    const uint64_t x = (uint64_t)blockIdx.x * BLOCK + threadIdx.x, nh = (uint64_t)P.ncontigs * P.nhap;
    if (x < nh) {
        const uint64_t c = x / P.nhap, h = x - c * P.nhap;
        uint64_t run = 0;
        for (uint64_t t = P.tfirst[c]; t < P.tfirst[c + 1]; ++t) { const uint64_t d = P.dir[t * P.nhap + h]; P.dir[t * P.nhap + h] = run; run += d; }
        P.rstart[(P.ref_first ? P.ncontigs : 0u) + h * P.ncontigs + c] = P.ref_off[c + 1] - P.ref_off[c] + run + P.w;
    } else if (P.ref_first && x < nh + P.ncontigs) {
        const uint64_t c = x - nh;
        P.rstart[c] = P.ref_off[c + 1] - P.ref_off[c] + P.w;
    }
}

// What a workgroup of k_panel_fill knows about the (record, tile) pair it is writing; the per-site arrays live in LDS.
struct PanelStretch { const uint8_t *p; uint64_t left; };      // p == nullptr: the pad
__device__ __forceinline__ PanelStretch panel_locate(uint64_t q, uint64_t L, uint32_t w, uint32_t cnt, const uint64_t *s_out, const uint64_t *s_alen,
                                                     const uint8_t *const *s_src, const uint8_t *const *s_after, const uint8_t *ref_c)
{
    PanelStretch r;
    if (q >= L) { r.p = nullptr; r.left = L + w - q; return r; }
    uint32_t lo = 0, hi = cnt;                       // the first site that starts behind q
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (s_out[mid] <= q) lo = mid + 1; else hi = mid; }
    const uint64_t next = s_out[lo] < L ? s_out[lo] : L;      // s_out[cnt]: where the next tile (or the pad) starts
    if (lo == 0) { r.p = ref_c + q; r.left = next - q; return r; }      // in front of the contig's first kept site
    const uint32_t j = lo - 1;
    const uint64_t o = q - s_out[j];
    if (o < s_alen[j]) { r.p = s_src[j] + o; r.left = s_alen[j] - o; }
    else { r.p = s_after[j] + (o - s_alen[j]); r.left = next - q; }
    return r;
}

// Workgroup b owns the text bytes [x0 + g * out_bytes, x0 + (g + 1) * out_bytes) of [base, base + total), g = the chunk that `stripes`
// and `per` deal to b: neighbouring workgroups take the same region of neighbouring haplotypes, whose genotype bytes share cache lines.
__global__ __launch_bounds__(BLOCK) void k_panel_fill(PanelDev P, uint8_t *text, uint64_t base, uint64_t total, uint32_t out_bytes, uint64_t nchunks, uint64_t stripes, uint64_t per)
{
    __shared__ uint64_t s_out[PANEL_TILE_MAX + 1], s_alen[PANEL_TILE_MAX], s_sum[BLOCK / WAVE];
    __shared__ const uint8_t *s_src[PANEL_TILE_MAX], *s_after[PANEL_TILE_MAX];
    const uint64_t g = ((uint64_t)blockIdx.x % stripes) * per + (uint64_t)blockIdx.x / stripes;
    if (g >= nchunks) return;
    const uint64_t x0 = (base & ~15ULL) + g * out_bytes, end = base + total;
    uint64_t cur = x0 < base ? base : x0;
    const uint64_t cend = x0 + out_bytes < end ? x0 + out_bytes : end;
    while (cur < cend) {
        // the record that holds cur (every record has its pad, so the starts ascend strictly)
        const uint64_t rel = cur - base;
        uint32_t rlo = 0, rhi = P.nrec;
        while (rhi - rlo > 1) { const uint32_t mid = (rlo + rhi) >> 1; if (P.rstart[mid] <= rel) rlo = mid; else rhi = mid; }
        const uint64_t rs = P.rstart[rlo], L = P.rstart[rlo + 1] - rs - P.w, q0 = rel - rs;
        const bool is_ref = P.ref_first && rlo < P.ncontigs;
        const uint32_t rr = is_ref ? rlo : rlo - (P.ref_first ? P.ncontigs : 0u);
        const uint64_t h = is_ref ? 0 : rr / P.ncontigs;
        const uint32_t c = is_ref ? rr : rr % P.ncontigs;
        const uint64_t cbeg = P.ref_off[c];
        // the last tile of the contig that starts at or in front of q0 (the first one also serves the bytes in front of it)
        const uint64_t t0 = P.tfirst[c], t1 = P.tfirst[c + 1];
        auto tile_out = [&](uint64_t t) { return P.krpos[P.tk0[t]] - cbeg + (is_ref ? 0 : P.dir[t * P.nhap + h]); };
        uint64_t t = t0, E = L + P.w, dbase = 0;
        uint32_t cnt = 0;
        if (t1 > t0) {
            uint64_t lo = t0, hi = t1;
            while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (tile_out(mid) <= q0) lo = mid; else hi = mid; }
            t = lo;
            if (t + 1 < t1) E = tile_out(t + 1);
            cnt = (uint32_t)(P.tk0[t + 1] - P.tk0[t]);
            dbase = is_ref ? 0 : P.dir[t * P.nhap + h];
        }
        __syncthreads();      // the last pass is done with the arrays
        if (cnt) {
            const uint64_t k0 = P.tk0[t];
            uint64_t d[2] = {0, 0};
            for (uint32_t i = 0; i < 2; ++i) {
                const uint32_t j = 2 * threadIdx.x + i;
                if (j >= cnt) break;
                const uint64_t k = k0 + j;
                const uint32_t gq = is_ref ? 0u : P.gt[(uint64_t)P.ksite[k] * P.nhap + h];
                const uint8_t *src; const uint64_t al = panel_allele(P, k, gq, &src);
                s_alen[j] = al; s_src[j] = src; s_after[j] = P.ref + P.krpos[k] + P.kspan[k];
                d[i] = al - P.kspan[k];
            }
            uint64_t tot;
            const uint64_t ex = block_excl_sum<uint64_t>(d[0] + d[1], s_sum, &tot);
            for (uint32_t i = 0; i < 2; ++i) {
                const uint32_t j = 2 * threadIdx.x + i;
                if (j < cnt) s_out[j] = P.krpos[k0 + j] - cbeg + dbase + ex + (i ? d[0] : 0);
            }
        }
        if (threadIdx.x == 0) s_out[cnt] = E;
        __syncthreads();
        const uint64_t rbase = base + rs;                                   // text position of the record's first byte
        const uint64_t segend = rbase + E < cend ? rbase + E : cend;        // this pass writes [cur, segend)
        const uint8_t *ref_c = P.ref + cbeg;
        for (uint64_t xs = (cur & ~15ULL) + 16ULL * threadIdx.x; xs < segend; xs += 16ULL * BLOCK) {
            const uint64_t lo = xs < cur ? cur : xs, hi = xs + 16 < segend ? xs + 16 : segend;
            PanelStretch st = panel_locate(lo - rbase, L, P.w, cnt, s_out, s_alen, s_src, s_after, ref_c);
            if (hi - lo == 16 && st.left >= 16) {      // one aligned store from one stretch
                uint4 v;
                if (st.p) __builtin_memcpy(&v, st.p, 16); else v = make_uint4(0x41414141u, 0x41414141u, 0x41414141u, 0x41414141u);
                *(uint4 *)(text + xs) = v;
            } else {
                for (uint64_t x = lo; x < hi; ++x) {
                    if (!st.left) st = panel_locate(x - rbase, L, P.w, cnt, s_out, s_alen, s_src, s_after, ref_c);
                    text[x] = st.p ? *st.p++ : (uint8_t)'A';
                    --st.left;
                }
            }
        }
        cur = segend;
    }
}

} // namespace pfp
