// pfbwt-f_amd/csrc/dictrec.h -- the suffix sort of the DICTIONARY through one level of prefix-free parsing of the dictionary itself: what
// recsort.h does for the parse, for a string of bytes whose words end in EndOfWord and whose byte-identical suffixes must stay ONE class.
//
// Reference: sort_dict_suffixes, include/pfbwt.hpp:206-223 -> gsacak (+ LCP), gsa/gsacak.c:2504-2524 -> gSACA_K_LCP :1649-1929 -- again an
// induced sort with a recursion on the names of sampled substrings (:1769), and only "glcp[j] >= suff_len" is consumed (pfbwt.hpp:137).
// The dictionary of a pangenome is itself repetitive: 870 K words for the 325 K loci of S-32G, the variants of a locus identical up to a SNP
// (its level-2 dictionary is 0.3 of it, measured before this file was written).  So:
//   * level-2 phrases inside every word: a phrase ends where a hash of the last DR_W bytes is 0 mod p2 (windows never cross a word end) and
//     at the word's EndOfWord; consecutive phrases overlap by DR_W bytes (prefix-free parsing proper, pfparser.hpp:335-352, per word);
//   * every dictionary offset x is owned by the phrase in which its suffix is longer than DR_W (the last phrase of a word owns all that
//     is left, the EndOfWord position included); suffix x sorts by (its string up to the phrase end, the sampled suffix at the next phrase);
//   * D2 = the distinct phrases as a small dictionary of their own (EndOfWord-separated, the last phrases of words without their
//     EndOfWord -- the separator stands for it): sorted by the EXISTING dictionary sorter (sufsort.h, k_round<true>), whose classes of
//     identical suffixes are exactly the classes of phrase-suffix strings;
//   * P2 = per word the ranks of its phrases, words separated by 1: sorted by the integer sorter (recsort.h / sufsort.h); two sampled
//     suffixes that agree up to their separator are the SAME suffix of the dictionary: tie classes by comparing neighbours;
//   * assembly (k_rs_assemble of recsort.h, with the keys kept): the rows of a D2 class are the occurrences of its member phrases, sorted by
//     the tie class of the sampled suffix behind them; equal (class, key) = byte-identical dictionary suffixes = one class (srank).
// Outputs: gsa (slot -> offset), srank (slot -> first slot of its class), sflag (slot -> the suffix starts a word) -- what the text-round
// sort of sufsort.h leaves for the emission and the word ranks.  The order INSIDE a class is not the offset order of gsacak (nothing in
// the engine asks for it: emit.h finds a group's first member by word rank); the gsacak drop-in keeps the old sorter.
// Here: the kernels that differ from the parse's (triggers inside words, de-duplication of byte strings, D2 with EndOfWord, P2 per word
// and its tie classes, final classes) and dict_sort_pfp, the list of stages.  The stages both sorts run alike (distinct phrases, word
// ids, inverted lists, slots to classes, assembly, big classes: l2_*), the counter slots and k_rs_word_ranks / k_rs_slot_records /
// rs_phrase_hash, which this route launches too, are in recsort.h.
#pragma once
#include "recsort.h"

namespace pfp {

constexpr int DR_W = 4;                        // bytes of a level-2 trigger window
constexpr uint32_t DR_MAX_PHRASE = 1024;       // longest level-2 phrase this route accepts (a run of N without a trigger is one phrase: old route)

__device__ __forceinline__ uint32_t dr_trigger(const uint8_t *D, uint64_t x, uint32_t p2)
{
    const uint8_t c = D[x];
    if (c == EndOfWord) return 1u;
    if (c == EndOfDict || x < (uint64_t)(DR_W - 1)) return 0u;
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < DR_W; ++k) { const uint32_t b = D[x - (DR_W - 1) + k]; if (b <= 1u) return 0u; v = (v << 8) | b; }
    uint32_t h = v * 0x9E3779B1u; h ^= h >> 15; h *= 0x85EBCA77u; h ^= h >> 13;
    return (h % p2 == 0u) ? 1u : 0u;
}
__global__ __launch_bounds__(BLOCK) void k_dr_trig_count(const uint8_t *D, uint64_t N, uint32_t p2, uint32_t *cnt)
{
    __shared__ uint32_t red[4];
    const uint64_t x0 = ((uint64_t)blockIdx.x * BLOCK + threadIdx.x) * 16;
    uint32_t n = 0;
    for (int k = 0; k < 16; ++k) if (x0 + k < N) n += dr_trigger(D, x0 + k, p2);
    uint32_t tot;
    (void)block_excl_sum(n, red, &tot);
    if (threadIdx.x == 0) cnt[blockIdx.x] = tot;
}
// pe[j] = position of the j-th phrase end (ascending)
__global__ __launch_bounds__(BLOCK) void k_dr_trig_write(const uint8_t *D, uint64_t N, uint32_t p2, const uint32_t *blockoff, uint32_t *pe)
{
    __shared__ uint32_t red[4];
    const uint64_t x0 = ((uint64_t)blockIdx.x * BLOCK + threadIdx.x) * 16;
    uint32_t m = 0;
    for (int k = 0; k < 16; ++k) if (x0 + k < N) m |= dr_trigger(D, x0 + k, p2) << k;
    uint32_t tot;
    uint32_t o = blockoff[blockIdx.x] + block_excl_sum((uint32_t)__popc(m), red, &tot);
    while (m) { const int b = __ffs((int)m) - 1; pe[o++] = (uint32_t)(x0 + (uint32_t)b); m &= m - 1u; }
}
// phrase j = D[ps[j] .. pe[j]]: it starts at its word's first byte, or DR_W - 1 bytes in front of the previous phrase's end
__global__ __launch_bounds__(BLOCK) void k_dr_starts(const uint8_t *D, const uint32_t *pe, uint64_t k, uint32_t *ps, uint32_t *maxlen)
{
    __shared__ uint32_t red[4];
    const uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t len = 0;
    if (j < k) {
        uint32_t s = 0;
        if (j) { const uint32_t pv = pe[j - 1]; s = D[pv] == EndOfWord ? pv + 1u : pv - (uint32_t)(DR_W - 1); }
        ps[j] = s; len = pe[j] - s + 1u;
    }
    uint32_t tot;
    (void)block_incl_max(len, red, &tot);
    if (threadIdx.x == 0 && tot > *(volatile uint32_t *)maxlen) atomicMax(maxlen, tot);
}
// exact de-duplication of the phrases (bytes, the EndOfWord of a word's last phrase included): entry = tag << 32 | (phrase index + 1)
__global__ __launch_bounds__(BLOCK) void k_dr_dedup(const uint8_t *D, const uint32_t *ps, const uint32_t *pe, uint64_t k, unsigned long long *table, uint32_t tmask, uint32_t *eid, uint32_t *isrep, uint32_t *overflow)
{
    const uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= k) return;
    const uint32_t a = ps[j], b = pe[j];
    const uint64_t h = rs_phrase_hash(D, a, b);
    const uint32_t tag = (uint32_t)(h >> 32);
    const unsigned long long mine = ((unsigned long long)tag << 32) | (unsigned long long)(uint32_t)(j + 1);
    uint32_t slot = (uint32_t)h & tmask, rep = 0, probe = 0;
    for (; probe < REC_MAX_PROBES; ++probe) {
        unsigned long long e = table[slot];
        if (e == 0ULL) {
            e = atomicCAS(&table[slot], 0ULL, mine);
            if (e == 0ULL) { rep = 1; break; }
        }
        if ((uint32_t)(e >> 32) == tag) {
            const uint32_t r = (uint32_t)e - 1u, ra = ps[r];
            if (pe[r] - ra == b - a) {
                bool eq = true;
                for (uint32_t d = 0; d <= b - a; ++d) if (D[ra + d] != D[a + d]) { eq = false; break; }
                if (eq) break;
            }
        }
        slot = (slot + 1u) & tmask;
    }
    if (probe == REC_MAX_PROBES) atomicExch(overflow, 1u);
    eid[j] = slot; isrep[j] = rep;
}
__global__ __launch_bounds__(BLOCK) void k_dr_rep_keys(const uint8_t *D, const uint32_t *ps, const uint32_t *pe, const uint32_t *replist, uint64_t nw2, uint64_t *keys, uint32_t *vals)
{
    const uint64_t t = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= nw2) return;
    const uint32_t j = replist[t];
    keys[t] = rs_phrase_hash(D, ps[j], pe[j]); vals[t] = (uint32_t)t;
}
// per distinct phrase i (in the order of the sorted hashes): its representative, whether it closes a word, its D2 length + separator
__global__ __launch_bounds__(BLOCK) void k_dr_assign_ids(const uint8_t *D, const uint32_t *sorted_t, const uint32_t *replist, const uint32_t *eid, const uint32_t *ps, const uint32_t *pe, uint64_t nw2,
                                                         uint32_t *slot2id, uint32_t *wrep, uint32_t *wlen1, uint8_t *lastw)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i > nw2) return;
    if (i == nw2) { wlen1[i] = 0u; return; }
    const uint32_t j = replist[sorted_t[i]];
    const uint32_t last = D[pe[j]] == EndOfWord ? 1u : 0u;
    slot2id[eid[j]] = (uint32_t)i; wrep[i] = j; lastw[i] = (uint8_t)last;
    wlen1[i] = pe[j] - ps[j] + 1u - last + 1u;             // bytes without the word's EndOfWord, + the separator
}
__global__ __launch_bounds__(BLOCK) void k_dr_dict_build(const uint8_t *D, const uint32_t *ps, const uint32_t *wrep, const uint32_t *wstart, uint64_t nw2, uint64_t ND, uint8_t *D2, uint32_t *wd2)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i > nw2) return;
    if (i == nw2) { D2[ND - 1] = EndOfDict; wd2[ND - 1] = (uint32_t)(nw2 ? nw2 - 1 : 0); return; }
    const uint32_t j = wrep[i], a = ps[j], o = wstart[i], L = wstart[i + 1] - o - 1u;
    for (uint32_t d = 0; d < L; ++d) { D2[o + d] = D[a + d]; wd2[o + d] = (uint32_t)i; }
    D2[o + L] = EndOfWord; wd2[o + L] = (uint32_t)i;
}
// P2: per dictionary word the ranks (+ 2) of its phrases, then the separator 1; the final 0 behind the last word.  Phrase j of word wj
// sits at P2[j + wj]
__global__ __launch_bounds__(BLOCK) void k_dr_names(const uint8_t *D, const uint32_t *pe, const uint32_t *wordid, const uint32_t *wid2, const uint32_t *wrank2, uint64_t k, uint64_t nwords, uint32_t *P2)
{
    const uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j < k) {
        const uint32_t e = pe[j], wj = wordid[e];
        P2[j + wj] = wrank2[wid2[j]] + 2u;
        if (D[e] == EndOfWord) P2[j + wj + 1] = 1u;
    } else if (j == k) P2[k + nwords] = 0u;
}
// neighbours in SA(P2) that agree up to their separator are the same suffix of the dictionary.  First pass: DR_TIE_CAP symbols.  A pair
// that still agrees there without a separator (a run of one level-2 phrase: every byte of an A run ends one) is left open in one class;
// the classes are then those of the strings cut at DR_TIE_CAP symbols or at the separator, which k_dr_p2_double refines.  (S-32G: with a
// cap of 64 some pairs stayed open and the doubling round cost 1 % of a step; at 1024 the first pass decides every pair there)
constexpr uint32_t DR_TIE_CAP = 1024;
__global__ __launch_bounds__(BLOCK) void k_dr_p2_heads(const uint32_t *P2, const uint32_t *SA2, uint64_t n2, uint32_t *headslot, uint8_t *open, uint32_t *nopen)
{
    __shared__ uint32_t red[4];
    const uint64_t s = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t op = 0u;
    if (s < n2) {
        uint32_t hd = 1u;
        if (s > 0) {
            const uint32_t x = SA2[s], y = SA2[s - 1];
            uint32_t d = 0;
            for (; d < DR_TIE_CAP; ++d) {
                const uint32_t a = x + d < n2 ? P2[x + d] : 0u, b = y + d < n2 ? P2[y + d] : 0u;
                if (a != b) { hd = (a | b) > 1u ? 1u : 0u; break; }
                if (a <= 1u) { hd = 0u; break; }
            }
            if (d == DR_TIE_CAP) { hd = 0u; op = 1u; }
        }
        headslot[s] = hd ? (uint32_t)s : 0u;
        open[s] = (uint8_t)op;
    }
    uint32_t tot;
    (void)block_excl_sum(op, red, &tot);
    if (threadIdx.x == 0 && tot) atomicAdd(nopen, tot);
}
// E[n2 - 1 - i] = n2 - 1 - i where P2[i] ends a word (a separator or the final 0), else 0: after an inclusive max-scan, the end of the
// word that holds position x is n2 - 1 - E[n2 - 1 - x]
__global__ __launch_bounds__(BLOCK) void k_dr_p2_ends(const uint32_t *P2, uint64_t n2, uint32_t *E)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < n2) E[n2 - 1 - i] = P2[i] <= 1u ? (uint32_t)(n2 - 1 - i) : 0u;
}
// one prefix-doubling round over the open pairs.  rc: the classes of the strings cut at h symbols or at the separator.  An open pair agrees
// on h symbols, none of them a separator, so x + h and y + h still lie in their words: the pair agrees on 2h symbols iff their classes are
// equal, and is a tie once its word ends inside them.  headslot holds the max-scanned heads of the last round (every entry at most its
// slot): a new head is written as its own slot, and the next max-scan gives the refined classes
__global__ __launch_bounds__(BLOCK) void k_dr_p2_double(const uint32_t *SA2, const uint32_t *rc, const uint32_t *E, uint64_t n2, uint64_t h, uint8_t *open, uint32_t *headslot, uint32_t *nopen)
{
    __shared__ uint32_t red[4];
    const uint64_t s = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t op = 0u;
    if (s < n2 && open[s]) {
        const uint32_t x = SA2[s], y = SA2[s - 1];
        if (rc[x + h] != rc[y + h]) headslot[s] = (uint32_t)s;
        else if (n2 - 1 - E[n2 - 1 - x] - x >= 2 * h) op = 1u;
        open[s] = (uint8_t)op;
    }
    uint32_t tot;
    (void)block_excl_sum(op, red, &tot);
    if (threadIdx.x == 0 && tot) atomicAdd(nopen, tot);
}
__global__ __launch_bounds__(BLOCK) void k_dr_p2_class(const uint32_t *SA2, const uint32_t *headslot /*max-scanned*/, uint64_t n2, uint32_t *rc)
{
    const uint64_t s = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s < n2) rc[SA2[s]] = headslot[s];
}
// list entry (a phrase occurrence, grouped by distinct phrase): key = tie class of the sampled suffix at the next phrase of its word (0 behind
// a word's last phrase: nothing follows), position = first byte of the occurrence (| bit 31 when that byte starts a word)
__global__ __launch_bounds__(BLOCK) void k_dr_list_payload(const uint8_t *D, const uint32_t *inv, const uint32_t *ps, const uint32_t *pe, const uint32_t *wordid, const uint32_t *rc, uint64_t k, uint32_t *ikey, uint32_t *ipos)
{
    const uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e >= k) return;
    const uint32_t j = inv[e], en = pe[j];
    ikey[e] = D[en] == EndOfWord ? 0u : rc[j + 1u + wordid[en]];
    const uint32_t x = ps[j];      // bit 31: the occurrence starts a dictionary word (row `x` itself then gets sflag = 1 from the assembly; positions stay below 2^31)
    ipos[e] = x | ((D[x] > EndOfWord && (x == 0 || D[x - 1] == EndOfWord)) ? 0x80000000u : 0u);
}
// per slot of SA(D2): rows it stands for, whole-phrase flag.  Offset o of phrase W (L bytes): a closing phrase owns every offset up to its
// separator (the word's EndOfWord), any other phrase the offsets whose suffix is longer than the window
__global__ __launch_bounds__(BLOCK) void k_dr_slots(const uint32_t *SA2d, const uint32_t *wd2, const uint32_t *wstart, const uint8_t *lastw, const uint32_t *woff, uint64_t ND, uint32_t *rows, uint32_t *whole, uint32_t *valid)
{
    const uint64_t s = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= ND) return;
    const uint32_t y = SA2d[s];
    uint32_t v = 0u, r = 0u, wh = 0u;
    if (y + 1 < ND) {                                         // (the final EndOfDict stands for nothing)
        const uint32_t W = wd2[y], o = y - wstart[W], L = wstart[W + 1] - wstart[W] - 1u;
        v = lastw[W] ? 1u : (o + (uint32_t)DR_W + 1u <= L ? 1u : 0u);
        r = v ? woff[W + 1] - woff[W] : 0u;
        wh = (o == 0u && L > 0u) ? 1u : 0u;
    }
    rows[s] = r; whole[s] = wh; valid[s] = v;
}
// valid slots: head of a D2 class iff the class head slot differs from the previous valid slot's
__global__ __launch_bounds__(BLOCK) void k_dr_heads(const uint32_t *vlist, const uint32_t *srank2, uint64_t nv, uint32_t *head)
{
    const uint64_t v = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (v >= nv) return;
    head[v] = (v == 0 || srank2[vlist[v]] != srank2[vlist[v - 1]]) ? 1u : 0u;
}
// rows of the assembled array: a class of identical dictionary suffixes starts where a D2 class starts or the key changes
__global__ __launch_bounds__(BLOCK) void k_dr_mark_class_rows(const uint32_t *crow, uint64_t nc, uint32_t *cstart)
{
    const uint64_t ci = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (ci < nc) cstart[1u + crow[ci]] = 1u;
}
__global__ __launch_bounds__(BLOCK) void k_dr_final_heads(const uint32_t *okey, const uint32_t *cstart, uint64_t N, uint32_t *headslot)
{
    const uint64_t r = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= N) return;
    const bool hd = r <= 1 || cstart[r] || okey[r] != okey[r - 1];
    headslot[r] = hd ? (uint32_t)r : 0u;
}
// 6 (second half). tie classes of SA(P2): rc[x] = first slot of the class of sampled suffix x.  R2 is reused for the head slots
inline int dr_tie_classes(pfp_ctx *c, const Level2 &L, const uint32_t *P2, const uint32_t *SA2, uint32_t *R2, uint32_t *rc, uint64_t n2)
{
    uint32_t *d_open = L.d_cnt + L2_OPEN;
    uint8_t *open; PFP_ALLOC_HI(c, open, uint8_t, n2);
    PFP_HIP(c, hipMemsetAsync(d_open, 0, 4, c->stream));
    PFP_LAUNCH(c, K_REC_PARSE, n2 * 17, k_dr_p2_heads, nblocks(n2, BLOCK), P2, SA2, n2, R2, open, d_open);
    PFP_TRY((device_scan<uint32_t, 1>(c, R2, R2, n2, nullptr)));
    PFP_LAUNCH(c, K_REC_PARSE, n2 * 12, k_dr_p2_class, nblocks(n2, BLOCK), SA2, (const uint32_t *)R2, n2, rc);
    uint32_t nopen = 0; PFP_TRY(d2h_u32(c, d_open, &nopen));
    if (!nopen) return PFP_OK;
    // ties longer than the first pass: ceil(log2(longest word of P2 / DR_TIE_CAP)) rounds of O(n2)
    const uint32_t open0 = nopen;
    int rounds = 0;
    uint32_t *E; PFP_ALLOC_HI(c, E, uint32_t, n2);
    PFP_LAUNCH(c, K_REC_PARSE, n2 * 8, k_dr_p2_ends, nblocks(n2, BLOCK), P2, n2, E);
    PFP_TRY((device_scan<uint32_t, 1>(c, E, E, n2, nullptr)));
    for (uint64_t h = DR_TIE_CAP; nopen; h *= 2, ++rounds) {
        PFP_HIP(c, hipMemsetAsync(d_open, 0, 4, c->stream));
        PFP_LAUNCH(c, K_REC_PARSE, n2 + (uint64_t)nopen * 24, k_dr_p2_double, nblocks(n2, BLOCK), SA2, (const uint32_t *)rc, (const uint32_t *)E, n2, h, open, R2, d_open);
        PFP_TRY((device_scan<uint32_t, 1>(c, R2, R2, n2, nullptr)));
        PFP_LAUNCH(c, K_REC_PARSE, n2 * 12, k_dr_p2_class, nblocks(n2, BLOCK), SA2, (const uint32_t *)R2, n2, rc);
        PFP_TRY(d2h_u32(c, d_open, &nopen));
    }
    if (c->tun.verbose) fprintf(stderr, "[pfbwt_hip]   P2 tie classes: %u neighbour pairs agree on %u symbols, resolved in %d doubling rounds\n", open0, DR_TIE_CAP, rounds);
    return PFP_OK;
}
// *taken = 0: nothing was written (the dictionary does not shrink, a phrase is too long, ...): the caller sorts with sufsort.h.
// The stages are those of suffix_sort_pfp; the shared ones (l2_*) are in recsort.h
inline int dict_sort_pfp(pfp_ctx *c, uint32_t *gsa, uint32_t *srank, uint8_t *sflag, int *taken)
{
    *taken = 0;
    const uint64_t N = c->dsize, nwords = c->dwords;
    const uint8_t *D = c->d_dict;
    const bool forced = c->tun.dict_rec > 0, verbose = c->tun.verbose != 0;
    const uint32_t p2 = c->tun.dict_rec_p2 >= 2 ? (uint32_t)c->tun.dict_rec_p2 : 16u;
    Level2 L = {}; L.N = N;
    // ---- when the route is given up (every line under PFP_VERBOSE)
    const auto too_few_or_many_phrases = [&] { return L.k < nwords || (!forced && L.k * 6 > N); };
    const auto phrase_too_long = [&] { if (L.maxlen > DR_MAX_PHRASE && verbose) fprintf(stderr, "[pfbwt_hip] recursive dictionary sort given up: a level-2 phrase of %u bytes\n", L.maxlen); return L.maxlen > DR_MAX_PHRASE; };
    const auto table_too_full = [&] { if (L.overflow && verbose) fprintf(stderr, "[pfbwt_hip] recursive dictionary sort given up: phrase table too full\n"); return L.overflow != 0; };
    const auto not_repetitive = [&](uint64_t ND) { return !forced && ND * 2 > N; };      // does not shrink enough to pay for the assembly

    if (N < 64 || !dr_fits_32(N) || !c->d_wordid) return PFP_OK;      // too short; over 32 bits; no word ids
    L.mk = c->arena.mark_hi();
    HostTimer tm;
    // 1. level-2 phrases inside every word
    const unsigned gt = nblocks(N, 16 * BLOCK);
    PFP_TRY(l2_count_phrases(c, L, gt, 16, [&](uint32_t *bcnt) -> int { PFP_LAUNCH(c, K_REC_PARSE, N, k_dr_trig_count, gt, D, N, p2, bcnt); return PFP_OK; }));
    const uint64_t k = L.k;
    if (too_few_or_many_phrases()) return l2_give_up(c, L);
    uint32_t *pe_;
    PFP_ALLOC_HI(c, pe_, uint32_t, k + 1); PFP_ALLOC_HI(c, L.ps, uint32_t, k + 1);
    const uint32_t *pe = pe_, *ps = L.ps;
    PFP_LAUNCH(c, K_REC_PARSE, N + k * 4, k_dr_trig_write, gt, D, N, p2, (const uint32_t *)L.bcnt, pe_);
    PFP_LAUNCH(c, K_REC_PARSE, k * 9, k_dr_starts, nblocks(k, BLOCK), D, pe, k, L.ps, L.d_cnt + L2_LONGEST);
    PFP_TRY(d2h_u32(c, L.d_cnt + L2_LONGEST, &L.maxlen));
    if (phrase_too_long()) return l2_give_up(c, L);
    // 2. distinct phrases
    PFP_TRY(l2_dedup(c, L, 2, [&](unsigned long long *table, uint32_t tmask) -> int {
        PFP_LAUNCH(c, K_REC_DEDUP, N * 2 + k * 24, k_dr_dedup, nblocks(k, BLOCK), D, ps, pe, k, table, tmask, L.eid, L.isrep, L.d_cnt + L2_OVERFLOW); return PFP_OK; }));
    if (table_too_full()) return l2_give_up(c, L);
    const uint64_t nw2 = L.nw;
    uint8_t *lastw;
    PFP_ALLOC_HI(c, L.slot2id, uint32_t, L.tsize); PFP_ALLOC_HI(c, L.wrep, uint32_t, nw2); PFP_ALLOC_HI(c, L.wstart, uint32_t, nw2 + 1); PFP_ALLOC_HI(c, lastw, uint8_t, nw2 + 1);
    PFP_ALLOC_HI(c, L.inv0, uint32_t, k); PFP_ALLOC_HI(c, L.wid1, uint32_t, k); PFP_ALLOC_HI(c, L.inv1, uint32_t, k); PFP_ALLOC_HI(c, L.woff, uint32_t, nw2 + 1);
    PFP_TRY(l2_word_ids(c, L,
        [&](uint64_t *hk, uint32_t *hv) -> int { PFP_LAUNCH(c, K_REC_DEDUP, nw2 * 40, k_dr_rep_keys, nblocks(nw2, BLOCK), D, ps, pe, (const uint32_t *)L.replist, nw2, hk, hv); return PFP_OK; },
        [&](const uint32_t *sorted) -> int { PFP_LAUNCH(c, K_REC_DEDUP, nw2 * 24, k_dr_assign_ids, nblocks(nw2 + 1, BLOCK), D, sorted, (const uint32_t *)L.replist, (const uint32_t *)L.eid, ps, pe, nw2, L.slot2id, L.wrep, L.wstart, lastw); return PFP_OK; }));
    const uint64_t ND = (uint64_t)L.nd32 + 1;                  // + the final EndOfDict
    const uint64_t n2 = k + nwords + 1;                        // length of P2
    if (verbose) fprintf(stderr, "[pfbwt_hip] recursive dictionary sort: %llu bytes, %llu words -> %llu level-2 phrases (longest %u), %llu distinct, D2 = %llu bytes (%.1f ms so far)\n",
                         (unsigned long long)N, (unsigned long long)nwords, (unsigned long long)k, L.maxlen, (unsigned long long)nw2, (unsigned long long)ND, tm.ms());
    if (not_repetitive(ND)) return l2_give_up(c, L);
    // 3. inverted lists
    PFP_TRY(l2_inverted_lists(c, L));
    const uint32_t *widp = L.eid;
    // 4. D2 and its suffix array with classes (the dictionary sorter of sufsort.h)
    uint8_t *D2; uint32_t *wd2, *gsa2, *srank2;
    PFP_ALLOC_HI(c, D2, uint8_t, ND + 64); PFP_ALLOC_HI(c, wd2, uint32_t, ND); PFP_ALLOC_HI(c, gsa2, uint32_t, ND); PFP_ALLOC_HI(c, srank2, uint32_t, ND);
    PFP_HIP(c, hipMemsetAsync(D2 + ND, 0, 64, c->stream));
    PFP_LAUNCH(c, K_REC_PARSE, ND * 6, k_dr_dict_build, nblocks(nw2 + 1, BLOCK), D, ps, (const uint32_t *)L.wrep, (const uint32_t *)L.wstart, nw2, ND, D2, wd2);
    {
        const size_t mk2 = c->arena.mark_hi();
        uint64_t *k0, *k1; uint32_t *v0, *v1; uint2 *rj2;
        PFP_ALLOC_HI(c, k0, uint64_t, ND); PFP_ALLOC_HI(c, k1, uint64_t, ND); PFP_ALLOC_HI(c, v0, uint32_t, ND); PFP_ALLOC_HI(c, v1, uint32_t, ND); PFP_ALLOC_HI(c, rj2, uint2, ND);
        PFP_LAUNCH(c, K_SS_INIT_KEYS, ND * 13, k_dict_init_keys, nblocks(ND, DK_TILE), (const uint8_t *)D2, ND, k0, v0);
        BitRange full = {0, DK_KEY_BITS};
        int rounds = 0;
        PFP_TRY(suffix_sort_doubling<true>(c, ND, k0, v0, k1, v1, &full, 1, DK_CHARS, D2, gsa2, (uint32_t *)nullptr, rj2, &rounds, 9, srank2));
        c->arena.release_hi(mk2);
    }
    if (verbose) fprintf(stderr, "[pfbwt_hip]   D2 sorted (%.1f ms so far)\n", tm.ms());
    // 5. slots, phrase ranks, names
    uint32_t *P2, *SA2, *R2, *rc;
    PFP_ALLOC_HI(c, L.valid, uint32_t, ND); PFP_ALLOC_HI(c, L.rows, uint32_t, ND); PFP_ALLOC_HI(c, L.whole, uint32_t, ND); PFP_ALLOC_HI(c, L.rowoff, uint32_t, ND); PFP_ALLOC_HI(c, L.wposs, uint32_t, ND);
    PFP_ALLOC_HI(c, L.wrank, uint32_t, nw2); PFP_ALLOC_HI(c, P2, uint32_t, n2); PFP_ALLOC_HI(c, SA2, uint32_t, n2); PFP_ALLOC_HI(c, R2, uint32_t, n2); PFP_ALLOC_HI(c, rc, uint32_t, n2);
    PFP_LAUNCH(c, K_REC_PARSE, ND * 28, k_dr_slots, nblocks(ND, BLOCK), (const uint32_t *)gsa2, (const uint32_t *)wd2, (const uint32_t *)L.wstart, (const uint8_t *)lastw, (const uint32_t *)L.woff, ND, L.rows, L.whole, L.valid);
    PFP_TRY((device_scan<uint32_t, 0>(c, L.whole, L.wposs, ND, nullptr)));
    PFP_LAUNCH(c, K_REC_PARSE, ND * 16, k_rs_word_ranks, nblocks(ND, BLOCK), (const uint32_t *)gsa2, (const uint32_t *)wd2, (const uint32_t *)L.whole, (const uint32_t *)L.wposs, ND, 0u, L.wrank);
    PFP_LAUNCH(c, K_REC_PARSE, k * 16, k_dr_names, nblocks(k + 1, BLOCK), D, pe, (const uint32_t *)c->d_wordid, widp, (const uint32_t *)L.wrank, k, nwords, P2);
    // 6. P2 and its suffix array (depth 1: prefix doubling), tie classes
    {
        int r2 = 0;
        PFP_TRY(sort_int_suffixes(c, P2, n2, nw2 + 1, SA2, R2, &r2, 1, true));
    }
    PFP_TRY(dr_tie_classes(c, L, P2, SA2, R2, rc, n2));
    if (verbose) fprintf(stderr, "[pfbwt_hip]   P2 sorted (%.1f ms so far)\n", tm.ms());
    // 7. list payload, slot records and classes
    L.ikey = SA2; L.ipos = P2;
    PFP_LAUNCH(c, K_REC_PARSE, k * 24, k_dr_list_payload, nblocks(k, BLOCK), D, (const uint32_t *)L.inv, ps, pe, (const uint32_t *)c->d_wordid, (const uint32_t *)rc, k, L.ikey, L.ipos);
    PFP_TRY(l2_classes(c, L, gsa2, wd2, ND, (const uint32_t *)nullptr, [&](const uint32_t *vlist, uint64_t nv, uint32_t *head) -> int {
        PFP_LAUNCH(c, K_REC_PARSE, nv * 12, k_dr_heads, nblocks(nv, BLOCK), vlist, (const uint32_t *)srank2, nv, head); return PFP_OK; }));
    // 8. assembly with the keys kept, 9. big classes
    L.tile_rows = l2_tile_rows(c); L.keybits = bits_for(n2);
    uint32_t *okey, *cstart;
    PFP_ALLOC_HI(c, L.bigc, uint32_t, L.nc + 1); PFP_ALLOC_HI(c, okey, uint32_t, N); PFP_ALLOC_HI(c, cstart, uint32_t, N + 1);
    PFP_HIP(c, hipMemsetAsync(cstart, 0, (N + 1) * 4, c->stream));
    const L2Rows out = {gsa, nullptr, okey, sflag};
    PFP_TRY(l2_assemble(c, L, out));
    // 10. classes of identical dictionary suffixes, word-start flags
    PFP_LAUNCH(c, K_REC_PARSE, L.nc * 8, k_dr_mark_class_rows, nblocks(L.nc, BLOCK), (const uint32_t *)L.crow, L.nc, cstart);
    PFP_LAUNCH(c, K_REC_PARSE, N * 12, k_dr_final_heads, nblocks(N, BLOCK), (const uint32_t *)okey, (const uint32_t *)cstart, N, srank);
    PFP_TRY((device_scan<uint32_t, 1>(c, srank, srank, N, nullptr)));
    PFP_HIP(c, hipMemsetAsync(sflag, 0, 1, c->stream));      // row 0 is the final EndOfDict; every other row's flag came out of the assembly (k_rs_assemble / k_rs_big_store)
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    if (verbose) fprintf(stderr, "[pfbwt_hip]   dictionary assembled: %llu slots, %llu D2 classes (%.1f ms)\n", (unsigned long long)L.nv, (unsigned long long)L.nc, tm.ms());
    c->arena.release_hi(L.mk);
    *taken = 1;
    return PFP_OK;
}

} // namespace pfp
