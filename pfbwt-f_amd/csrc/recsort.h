// pfbwt-f_amd/csrc/recsort.h -- suffix array of an integer string S (the parse) by ONE level of prefix-free parsing of S itself,
// the recursion of the reference's SACA-K restated for a data-parallel machine.
//
// Reference: sacak_int -> SACA_K, gsa/gsacak.c:1397-1526: sort the LMS substrings (:852-874, induce :215-252), NAME them (nameSubstr
// :1165-1220), recurse on the string of names (level >= 1, :928-1145), then induce the order of all suffixes from the order of the
// sampled ones (getSAlms :1347-1361, putSuffix0 :97-111).  Called at include/pfparser.hpp:425 for the parse of a collection.
// Induced sorting is sequential.  What carries over is the shape -- sample, name, recurse on the names, derive the rest -- and the
// sampling that makes it data-parallel is the parser's own: prefix-free parsing (pfparser.hpp:335-352) applied to S.
//
//   * a symbol is a TRIGGER when a hash of its value is 0 mod p2 (the last symbol, the unique 0, always is); level-2 phrase j is
//     S[ps[j] .. ps[j+1]], two consecutive phrases share their trigger symbol (w = 1).  The strings S[i .. next trigger behind i]
//     of all positions i are a prefix-free set (a string ends in a trigger and has none inside), so
//         suffix(i) < suffix(i')  <=>  (string of i, rank of the sampled suffix that starts at its last symbol) compares smaller;
//   * the distinct phrases ("words", exact hash table like the text's own de-duplication, pfparser.hpp:595-601) are written one
//     behind the other, separated, into D2; ONE suffix sort of D2 (small: the collection is repetitive) names every string above
//     (class = run of equal strings in SA(D2)) and ranks the words; P2 = the word ranks of the phrases is the string of names;
//   * SA(P2) (recursive call; prefix doubling at the bottom) ranks the sampled suffixes;
//   * assembly: the rows of a class are the occurrences of its member words (inverted lists of P2), ordered by the rank of the
//     sampled suffix behind the occurrence: whole classes are gathered into LDS, sorted there by that ONE 32-bit key and stored.
//     This is generate_bwt_lcp's grouping (include/pfbwt.hpp:137-181) one level up, with integers for characters.
// On S-32G (325 M phrases of 1000 near-identical haplotypes) four refinement rounds over all 325 M suffixes become two over the 81 M
// sampled ones plus one LDS sort pass over the rows.  Inputs that do not shrink (alphabet ~ length, dictionaries that stay large, a
// phrase without trigger for > REC_MAX_PHRASE symbols) take the doubling route of sufsort.h, which stays the bottom of the recursion.
// Layout: the kernels; the host stages that this sort shares with the dictionary's (dictrec.h) -- counter slots (L2Counter), 32-bit
// bounds, struct Level2, l2_count_phrases, l2_dedup, l2_word_ids, l2_inverted_lists, l2_classes, l2_assemble --; then suffix_sort_pfp,
// the list of stages of the parse route, and sort_int_suffixes, which chooses between it and prefix doubling.
#pragma once
#include "sufsort.h"

namespace pfp {

constexpr uint32_t REC_MAX_PHRASE = 1024;      // longest level-2 phrase this route accepts (class heads compare strings symbol by symbol)
constexpr int RS_TRIG_PER = 16;                // symbols per thread of the trigger kernels
constexpr int RS_TRIG_TILE = BLOCK * RS_TRIG_PER;

__device__ __forceinline__ uint32_t rs_trigger(uint32_t s, uint32_t p2)
{
    uint32_t h = s * 0x9E3779B1u; h ^= h >> 15; h *= 0x85EBCA77u; h ^= h >> 13;
    return (h % p2 == 0u) ? 1u : 0u;
}
// trigger bits of the 16 positions i0 .. i0+15 (position 0 never starts a new phrase, the last position always ends one)
__device__ __forceinline__ uint32_t rs_trig_mask16(const uint32_t *S, uint64_t N, uint64_t i0, uint32_t p2)
{
    uint32_t m = 0;
    if (i0 + RS_TRIG_PER <= N) {
        const uint4 *q = reinterpret_cast<const uint4 *>(S + i0);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const uint4 a = q[v];
            m |= (rs_trigger(a.x, p2) | (rs_trigger(a.y, p2) << 1) | (rs_trigger(a.z, p2) << 2) | (rs_trigger(a.w, p2) << 3)) << (4 * v);
        }
    } else {
        for (int k = 0; k < RS_TRIG_PER; ++k) if (i0 + k < N) m |= rs_trigger(S[i0 + k], p2) << k;
    }
    if (i0 == 0) m &= ~1u;
    if (N - 1 >= i0 && N - 1 < i0 + RS_TRIG_PER) m |= 1u << (uint32_t)(N - 1 - i0);
    return m;
}
__global__ __launch_bounds__(BLOCK) void k_rs_trig_count(const uint32_t *S, uint64_t N, uint32_t p2, uint32_t *cnt)
{
    __shared__ uint32_t red[4];
    const uint64_t i0 = ((uint64_t)blockIdx.x * BLOCK + threadIdx.x) * RS_TRIG_PER;
    const uint32_t m = i0 < N ? rs_trig_mask16(S, N, i0, p2) : 0u;
    uint32_t tot;
    (void)block_excl_sum((uint32_t)__popc(m), red, &tot);
    if (threadIdx.x == 0) cnt[blockIdx.x] = tot;
}
// ps[0] = 0, ps[1 + t] = position of the t-th trigger (ascending): phrase j = S[ps[j] .. ps[j+1]]
__global__ __launch_bounds__(BLOCK) void k_rs_trig_write(const uint32_t *S, uint64_t N, uint32_t p2, const uint32_t *blockoff, uint32_t *ps)
{
    __shared__ uint32_t red[4];
    const uint64_t i0 = ((uint64_t)blockIdx.x * BLOCK + threadIdx.x) * RS_TRIG_PER;
    uint32_t m = i0 < N ? rs_trig_mask16(S, N, i0, p2) : 0u;
    uint32_t tot;
    uint32_t o = 1u + blockoff[blockIdx.x] + block_excl_sum((uint32_t)__popc(m), red, &tot);
    while (m) { const int b = __ffs((int)m) - 1; ps[o++] = (uint32_t)(i0 + (uint32_t)b); m &= m - 1u; }
    if (blockIdx.x == 0 && threadIdx.x == 0) ps[0] = 0u;
}
__global__ __launch_bounds__(BLOCK) void k_rs_max_phrase(const uint32_t *ps, uint64_t k, uint32_t *out)
{
    __shared__ uint32_t red[4];
    const uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t len = j < k ? ps[j + 1] - ps[j] + 1u : 0u;
    uint32_t tot;
    (void)block_incl_max(len, red, &tot);
    if (threadIdx.x == 0 && tot > *(volatile uint32_t *)out) atomicMax(out, tot);
}

// ---- exact de-duplication of the level-2 phrases (the std::map of pfparser.hpp:69-70, 595-601, for strings of integers) ----------
// table entry = hash tag << 32 | (position of the representative phrase's first symbol + 1); 0 = empty.  A lookup matches when the
// tags agree AND the symbols are equal: a phrase is its first symbol, non-triggers, one trigger, so a representative that agrees with
// the len symbols of this phrase ends where it does -- the representative's own length is never looked up.  Entries are write-once:
// a stale "empty" is corrected by the value the device-scope CAS returns.  A probe sequence longer than REC_MAX_PROBES means the table
// is too full (more distinct phrases than a repetitive collection has): the caller gives this route up.
// (First version, S-32G, 81 M phrases: 37 ms -- every insertion bumped ONE global counter and every lookup read the representative's
//  bounds, a third random sector per phrase.)
constexpr uint32_t REC_MAX_PROBES = 128;
// (T: uint32_t symbols of the parse, uint8_t bytes of the dictionary, dictrec.h)
template <typename T> __device__ __forceinline__ uint64_t rs_phrase_hash(const T *S, uint32_t a, uint32_t b)
{
    uint64_t h = 0x243F6A8885A308D3ULL;
    for (uint32_t i = a; i <= b; ++i) { h = (h ^ S[i]) * 0x9E3779B97F4A7C15ULL; h ^= h >> 29; }
    h *= 0xBF58476D1CE4E5B9ULL; h ^= h >> 32;
    return h;
}
__global__ __launch_bounds__(BLOCK) void k_rs_dedup(const uint32_t *S, const uint32_t *ps, uint64_t k, unsigned long long *table, uint32_t tmask, uint32_t *eid, uint32_t *isrep, uint32_t *overflow)
{
    const uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= k) return;
    const uint32_t a = ps[j], b = ps[j + 1];
    const uint64_t h = rs_phrase_hash(S, a, b);
    const uint32_t tag = (uint32_t)(h >> 32);
    const unsigned long long mine = ((unsigned long long)tag << 32) | (unsigned long long)(a + 1u);
    uint32_t slot = (uint32_t)h & tmask, rep = 0, probe = 0;
    for (; probe < REC_MAX_PROBES; ++probe) {
        unsigned long long e = table[slot];
        if (e == 0ULL) {
            e = atomicCAS(&table[slot], 0ULL, mine);
            if (e == 0ULL) { rep = 1; break; }
        }
        if ((uint32_t)(e >> 32) == tag) {
            const uint32_t ra = (uint32_t)e - 1u;
            bool eq = true;
            for (uint32_t d = 0; d <= b - a; ++d) if (S[ra + d] != S[a + d]) { eq = false; break; }
            if (eq) break;
        }
        slot = (slot + 1u) & tmask;
    }
    if (probe == REC_MAX_PROBES) atomicExch(overflow, 1u);
    eid[j] = slot; isrep[j] = rep;
}
// deterministic word ids: the distinct phrases in the order of their 64-bit content hashes; the phrase that holds the final 0 last
__global__ __launch_bounds__(BLOCK) void k_rs_rep_keys(const uint32_t *S, const uint32_t *ps, const uint32_t *replist, uint64_t nw, uint64_t k, uint64_t *keys, uint32_t *vals)
{
    const uint64_t t = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= nw) return;
    const uint32_t j = replist[t];
    keys[t] = (uint64_t)j + 1 == k ? ~0ULL : (rs_phrase_hash(S, ps[j], ps[j + 1]) >> 1);
    vals[t] = (uint32_t)t;
}
__global__ __launch_bounds__(BLOCK) void k_rs_assign_ids(const uint32_t *sorted_t, const uint32_t *replist, const uint32_t *eid, const uint32_t *ps, uint64_t nw, uint32_t *slot2id, uint32_t *wrep, uint32_t *wlen1)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i > nw) return;
    if (i == nw) { wlen1[i] = 0u; return; }
    const uint32_t j = replist[sorted_t[i]];
    slot2id[eid[j]] = (uint32_t)i; wrep[i] = j;
    wlen1[i] = ps[j + 1] - ps[j] + 2u;                      // symbols + separator
}
__global__ __launch_bounds__(BLOCK) void k_rs_wid(const uint32_t *eid, const uint32_t *slot2id, uint64_t k, uint32_t *wid, uint32_t *wid_keep, uint32_t *idx)
{
    const uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j < k) { const uint32_t id = slot2id[eid[j]]; wid[j] = id; wid_keep[j] = id; idx[j] = (uint32_t)j; }      // (wid is the sort's input; wid_keep stays in phrase order for the names)
}
// (lists from SA(P2), below: nothing is sorted by word, only the ids in phrase order are needed -- in place of the entry indices)
__global__ __launch_bounds__(BLOCK) void k_rs_wid_keep(const uint32_t *eid, const uint32_t *slot2id, uint64_t k, uint32_t *wid_keep)
{
    const uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j < k) wid_keep[j] = slot2id[eid[j]];
}
// D2 = the words in id order, symbols + 2, each followed by the separator 1 (the last one, which ends in S's own 0, by the final 0):
// strings compare before any separator is reached (prefix-free), a separator is below every symbol, so the suffixes with ONE string
// are neighbours in SA(D2) and the positions that stand for no string (separators, last symbols) never lie between them
__global__ __launch_bounds__(BLOCK) void k_rs_dict_build(const uint32_t *S, const uint32_t *ps, const uint32_t *wrep, const uint32_t *wstart, uint64_t nw, uint32_t *D, uint32_t *wd)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nw) return;
    const uint32_t j = wrep[i], a = ps[j], L = ps[j + 1] - a + 1u, o = wstart[i];
    for (uint32_t d = 0; d < L; ++d) { D[o + d] = S[a + d] + 2u; wd[o + d] = (uint32_t)i; }
    D[o + L] = i + 1 == nw ? 0u : 1u; wd[o + L] = (uint32_t)i;
}
// woff[id] = first entry of word id in the list of phrases sorted by word (every word occurs)
__global__ __launch_bounds__(BLOCK) void k_rs_list_bounds(const uint32_t *skeys, uint64_t k, uint64_t nw, uint32_t *woff)
{
    const uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e >= k) return;
    const uint32_t id = skeys[e];
    if (e == 0 || skeys[e - 1] != id) woff[id] = (uint32_t)e;
    if (e + 1 == k) woff[nw] = (uint32_t)k;
}
// per suffix-array slot of D2: rows it stands for (0: a separator or the last symbol of a word), whole-word flag
__global__ __launch_bounds__(BLOCK) void k_rs_slots(const uint32_t *SAD, const uint32_t *wd, const uint32_t *wstart, const uint32_t *woff, uint64_t ND, uint32_t *rows, uint32_t *whole, uint32_t *valid)
{
    const uint64_t s = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= ND) return;
    const uint32_t x = SAD[s], i = wd[x], o = x - wstart[i], L = wstart[i + 1] - wstart[i] - 1u;
    rows[s] = o + 1u < L ? woff[i + 1] - woff[i] : 0u;
    valid[s] = o + 1u < L ? 1u : 0u;
    whole[s] = o == 0u ? 1u : 0u;
}
// rank of a word = base + whole-word slots in front of its own (base 1: the parse's names, 0 is the final symbol of P2; base 0: dictrec.h)
__global__ __launch_bounds__(BLOCK) void k_rs_word_ranks(const uint32_t *SAD, const uint32_t *wd, const uint32_t *whole, const uint32_t *wpos, uint64_t ND, uint32_t base, uint32_t *wrank)
{
    const uint64_t s = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s < ND && whole[s]) wrank[wd[SAD[s]]] = wpos[s] + base;
}
__global__ __launch_bounds__(BLOCK) void k_rs_names(const uint32_t *wid, const uint32_t *wrank, uint64_t k, uint32_t *P2)
{
    const uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j < k) P2[j] = wrank[wid[j]];
    else if (j == k) P2[j] = 0u;
}
// ---- lists from SA(P2) (parse_rec_merge != 0) ---------------------------------------------------------------------------------------
// All suffixes of P2 that begin with one word are neighbours in SA(P2), ordered by the suffix behind the first symbol: the slice of
// SA2 whose suffixes start with word rank r IS the inverted list of that word, sorted by the assembly's key R2[j + 1].  List entry t
// (1 <= t <= k; SA2[0] = k is the final 0) is phrase SA2[t]; the list of rank r starts at roff[r], the first row of SA2 whose phrase
// has that rank (every word occurs, so every rank 1 .. nw has a start; roff[nw + 1] = k + 1).  No sort by word, and the keys of a
// list ascend.  The occurrence count of a word is only known behind the sort of P2, so the slots' flags (all that the names need)
// and their rows are two kernels.
__global__ __launch_bounds__(BLOCK) void k_rs_slot_flags(const uint32_t *SAD, const uint32_t *wd, const uint32_t *wstart, uint64_t ND, uint32_t *whole, uint32_t *valid)
{
    const uint64_t s = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= ND) return;
    const uint32_t x = SAD[s], i = wd[x], o = x - wstart[i], L = wstart[i + 1] - wstart[i] - 1u;
    valid[s] = o + 1u < L ? 1u : 0u;
    whole[s] = o == 0u ? 1u : 0u;
}
__global__ __launch_bounds__(BLOCK) void k_rs_slot_rows(const uint32_t *SAD, const uint32_t *wd, const uint32_t *valid, const uint32_t *wrank, const uint32_t *roff, uint64_t ND, uint32_t *rows)
{
    const uint64_t s = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= ND) return;
    uint32_t n = 0;
    if (valid[s]) { const uint32_t r = wrank[wd[SAD[s]]]; n = roff[r + 1] - roff[r]; }
    rows[s] = n;
}
// the names, and { text position, name } of every phrase in one record: the payload kernel gathers both with one read
__global__ __launch_bounds__(BLOCK) void k_rs_names_pos(const uint32_t *wid, const uint32_t *wrank, const uint32_t *ps, uint64_t k, uint32_t *P2, uint2 *pp)
{
    const uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j < k) { const uint32_t r = wrank[wid[j]]; P2[j] = r; pp[j] = make_uint2(ps[j], r); }
    else if (j == k) P2[j] = 0u;
}
// per list entry t: key and text position as k_rs_list_payload; a list starts where the name differs from the entry in front (the
// neighbour's name through LDS: one gather per entry, the first thread of a workgroup makes a second one)
__global__ __launch_bounds__(BLOCK) void k_rs_slice_payload(const uint32_t *SA2, const uint2 *pp, const uint32_t *R2, uint64_t k, uint64_t nw, uint32_t *ikey, uint32_t *ipos, uint32_t *roff)
{
    __shared__ uint32_t sr[BLOCK];
    const uint64_t t = (uint64_t)blockIdx.x * BLOCK + threadIdx.x + 1u;
    uint32_t r = 0;
    if (t <= k) {
        const uint32_t j = SA2[t];
        const uint2 q = pp[j];
        r = q.y; ikey[t] = R2[j + 1]; ipos[t] = q.x;
    }
    sr[threadIdx.x] = r;
    __syncthreads();
    if (t > k) return;
    const uint32_t rp = threadIdx.x ? sr[threadIdx.x - 1] : (t > 1 ? pp[SA2[t - 1]].y : 0u);
    if (r != rp) roff[r] = (uint32_t)t;
    if (t == k) roff[nw + 1] = (uint32_t)(k + 1);
}
// per list entry (a phrase, grouped by word): rank of the sampled suffix behind it, text position of its first symbol
__global__ __launch_bounds__(BLOCK) void k_rs_list_payload(const uint32_t *inv, const uint32_t *R2, const uint32_t *ps, uint64_t k, uint32_t *ikey, uint32_t *ipos)
{
    const uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e >= k) return;
    const uint32_t j = inv[e];
    ikey[e] = R2[j + 1]; ipos[e] = ps[j];
}
// valid slots (v = index in the compacted list): head of a class iff the string differs from the previous valid slot's
__global__ __launch_bounds__(BLOCK) void k_rs_heads(const uint32_t *D, const uint32_t *SAD, const uint32_t *vlist, uint64_t nv, uint32_t *head)
{
    const uint64_t v = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (v >= nv) return;
    // (everything that depends on s is loaded before the loop: hipcc 7.2 -O3 lost s across it for the lanes that skip the loop --
    //  the copy it keeps around the loop body is only written inside -- and a row offset was read at a wild address behind it: the one
    //  GPU fault of this file's first run on the card, invisible to the CPU interpreter)
    const uint32_t s = vlist[v];
    const uint32_t sp = v ? vlist[v - 1] : 0u;
    uint32_t hd = (v == 0 || sp + 1u != s) ? 1u : 0u;
    uint32_t x = SAD[s], y = SAD[s ? s - 1 : 0];
    if (!hd) {
        for (uint32_t d = 0; d <= REC_MAX_PHRASE + 1u; ++d) {
            const uint32_t a = D[x + d], b = D[y + d];
            if (a != b) { hd = (a | b) > 1u ? 1u : 0u; break; }
            if (a <= 1u) break;
        }
    }
    head[v] = hd;
}
// srec[v] = { first row, first list entry of its word, offset of the string in the word, index of its class }
// (woff is indexed by word id, or -- lists from SA(P2): wrank given -- by word rank)
__global__ __launch_bounds__(BLOCK) void k_rs_slot_records(const uint32_t *SAD, const uint32_t *vlist, const uint32_t *rowoff, const uint32_t *head, const uint32_t *hpos /*heads in front of v*/, const uint32_t *wd, const uint32_t *wstart,
                                                            const uint32_t *woff, const uint32_t *wrank /*nullable*/, uint64_t nv, uint4 *srec)
{
    const uint64_t v = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (v >= nv) return;
    const uint32_t s = vlist[v], x = SAD[s], i = wd[x];
    srec[v] = make_uint4(rowoff[s], woff[wrank ? wrank[i] : i], x - wstart[i], hpos[v] + head[v] - 1u);
}
__global__ __launch_bounds__(BLOCK) void k_rs_class_rows(const uint32_t *chead, const uint4 *srec, uint64_t nc, uint64_t nv, uint64_t R, uint32_t *crow, uint32_t *chead_end)
{
    const uint64_t ci = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (ci < nc) crow[ci] = srec[chead[ci]].x;
    else if (ci == nc) { crow[ci] = (uint32_t)R; *chead_end = (uint32_t)nv; }
}

// first index in [lo, hi) with a[idx] >= key
__device__ __forceinline__ uint32_t rs_lower_bound(const uint32_t *a, uint32_t lo, uint32_t hi, uint64_t key)
{
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if ((uint64_t)a[mid] < key) lo = mid + 1; else hi = mid; }
    return lo;
}

// lanes of the wave that hold the same NB-bit digit as this one (prims.h: same_digit_lanes is the 8-bit form)
template <int NB> __device__ __forceinline__ void rs_same_digit_lanes(uint32_t d, uint32_t &plo, uint32_t &phi)
{
#pragma unroll
    for (int bb = 0; bb < NB; ++bb) {
        const uint32_t neg = (uint32_t)(((int32_t)(d << (31 - bb))) >> 31);
        const unsigned long long m = __builtin_amdgcn_ballot_w64(neg != 0u);
        plo &= ~((uint32_t)m ^ neg); phi &= ~((uint32_t)(m >> 32) ^ neg);
    }
}

// Assembly.  Workgroup b owns the classes whose first row lies in [b*STEP, (b+1)*STEP); it takes them in batches of whole classes
// of at most tile_rows rows: the rows (list entries of the member words) are gathered into LDS, sorted there by
// (index of the class in the batch, rank of the sampled suffix behind the occurrence) -- stable LSD passes over 9-bit digits with
// wave-ballot ranking, the pass of the class sort of sufsort.h with a wider digit: S-32G has 27 key bits and ~125 classes per batch,
// 35 bits = 4 passes (8-bit digits and the class's first row as high part: 6 passes, 13.1 ms) -- and stored: SA[1 + row] = text
// position (row 0 is the final 0).  A class with more rows than a tile is appended to `bigc` (global sort route).
// LIST: workgroup b takes the one batch of classes [blist[2b], blist[2b + 1]) that k_rs_merge handed over, instead of a stripe.
constexpr int RA_DB = 9, RA_RADIX = 1 << RA_DB;
template <bool RANK, bool KEYOUT, bool LIST = false> __global__ __launch_bounds__(BLOCK) void k_rs_assemble(const uint4 *srec, const uint32_t *chead /*nc + 1*/, const uint32_t *crow /*nc + 1*/, uint32_t nc,
                                                                            const uint32_t *ikey, const uint32_t *ipos, int keybits, uint32_t tile_rows, uint32_t *SA, uint32_t *rank,
                                                                            uint32_t *bigc, uint32_t *nbig, uint32_t *okey /*KEYOUT (dictrec.h): the key of every row, in row order*/,
                                                                            uint8_t *oflag /*KEYOUT: bit 31 of a list position marks the start of a dictionary word; oflag[row] = the row is that position itself (sflag)*/,
                                                                            const uint32_t *blist /*LIST*/)
{
    constexpr int ITEMS = RS_ITEMS, TILE = RS_TILE;
    constexpr uint32_t STEP = TILE / 2;
    __shared__ uint32_t wh[BLOCK / WAVE][RA_RADIX];
    __shared__ uint64_t skeys[TILE];
    __shared__ uint16_t sidx[TILE];
    __shared__ uint16_t srow[TILE + 1];
    __shared__ uint32_t red[4];
    __shared__ uint32_t ctl[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t ci, ci1;
    if (LIST) { ci = blist[2u * blockIdx.x]; ci1 = blist[2u * blockIdx.x + 1u]; }
    else {
        const uint64_t w0 = (uint64_t)blockIdx.x * STEP;
        if (threadIdx.x == 0) { ctl[0] = rs_lower_bound(crow, 0u, nc, w0); ctl[1] = rs_lower_bound(crow, 0u, nc, w0 + STEP); }
        __syncthreads();
        ci = ctl[0]; ci1 = ctl[1];
    }
    while (ci < ci1) {
        __syncthreads();                                       // ctl / LDS of the previous batch are free
        if (threadIdx.x == 0) {
            // largest cj in (ci, ci1] with crow[cj] - crow[ci] <= tile_rows (crow ascends strictly: every class has rows)
            const uint64_t lim = (uint64_t)crow[ci] + tile_rows;
            uint32_t lo = ci, hi = ci1;                        // invariant: crow[lo] <= lim
            while (lo < hi) { const uint32_t mid = lo + ((hi - lo + 1) >> 1); if ((uint64_t)crow[mid] <= lim) lo = mid; else hi = mid - 1; }
            ctl[2] = lo;
            if (lo == ci) bigc[atomicAdd(nbig, 1u)] = ci;
        }
        __syncthreads();
        const uint32_t cj = ctl[2];
        if (cj == ci) { ++ci; continue; }
        const uint32_t r0 = crow[ci], n = crow[cj] - r0, v0 = chead[ci], ns = chead[cj] - v0;
        for (uint32_t t = threadIdx.x; t < ns; t += BLOCK) srow[t] = (uint16_t)(srec[v0 + t].x - r0);
        if (threadIdx.x == 0) srow[ns] = (uint16_t)n;
        __syncthreads();
        const uint32_t nit = (n + BLOCK - 1) / BLOCK;
        uint32_t xi[ITEMS];
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
            const uint32_t i = threadIdx.x + (uint32_t)it * BLOCK;
            xi[it] = 0u;
            if (i < n) {
                uint32_t lo = 0, hi = ns - 1;                  // largest t with srow[t] <= i
                while (lo < hi) { const uint32_t mid = lo + ((hi - lo + 1) >> 1); if (srow[mid] <= i) lo = mid; else hi = mid - 1; }
                const uint4 rec = srec[v0 + lo];
                const uint32_t e = rec.y + (i - (rec.x - r0));
                xi[it] = KEYOUT ? (rec.z ? (ipos[e] & 0x7FFFFFFFu) + rec.z : ipos[e]) : ipos[e] + rec.z;
                skeys[i] = ((uint64_t)(rec.w - ci) << keybits) | ikey[e];
                sidx[i] = (uint16_t)i;
            }
        }
        for (uint32_t i = n + threadIdx.x; i < nit * BLOCK; i += BLOCK) { skeys[i] = ~0ULL; sidx[i] = (uint16_t)i; }
        __syncthreads();
        int tbits = keybits;                                   // key bits + bits of the largest class index of the batch
        for (uint32_t hs = cj - 1 - ci; hs; hs >>= 1) ++tbits;
        const int npass = (tbits + RA_DB - 1) / RA_DB;
        const uint32_t base = (uint32_t)wave * (nit * WAVE) + lane;
        for (int p = 0; p < npass; ++p) {
            const int sh = RA_DB * p;
            uint64_t kk[ITEMS]; uint16_t vv[ITEMS]; unsigned dg[ITEMS];
#pragma unroll
            for (int w = 0; w < BLOCK / WAVE; ++w) { wh[w][threadIdx.x] = 0; wh[w][threadIdx.x + BLOCK] = 0; }
            __syncthreads();
#pragma unroll
            for (int it = 0; it < ITEMS; ++it) {
                if ((uint32_t)it < nit) {
                    const uint32_t i = base + (uint32_t)it * WAVE;
                    kk[it] = skeys[i]; vv[it] = sidx[i];
                    const uint32_t d = (uint32_t)(kk[it] >> sh) & (RA_RADIX - 1);
                    uint32_t plo = 0xFFFFFFFFu, phi = 0xFFFFFFFFu;
                    rs_same_digit_lanes<RA_DB>(d, plo, phi);
                    const int leader = plo ? __builtin_ctz(plo) : 32 + __builtin_ctz(phi);
                    uint32_t old = 0;
                    if (lane == leader) { old = wh[wave][d]; wh[wave][d] = old + (uint32_t)__builtin_popcount(plo) + (uint32_t)__builtin_popcount(phi); }
                    old = __shfl(old, leader);
                    dg[it] = d | ((old + __builtin_amdgcn_mbcnt_hi(phi, __builtin_amdgcn_mbcnt_lo(plo, 0u))) << RA_DB);
                }
            }
            __syncthreads();
            {   // thread t owns the digits 2t and 2t + 1
                const unsigned d0 = 2u * threadIdx.x;
                uint32_t c0[BLOCK / WAVE], c1[BLOCK / WAVE]; uint32_t total = 0;
#pragma unroll
                for (int w = 0; w < BLOCK / WAVE; ++w) { const uint2 q = *reinterpret_cast<const uint2 *>(&wh[w][d0]); c0[w] = q.x; c1[w] = q.y; total += q.x + q.y; }
                uint32_t tt;
                uint32_t run = block_excl_sum(total, red, &tt);
                uint32_t o0[BLOCK / WAVE];
#pragma unroll
                for (int w = 0; w < BLOCK / WAVE; ++w) { o0[w] = run; run += c0[w]; }
#pragma unroll
                for (int w = 0; w < BLOCK / WAVE; ++w) { *reinterpret_cast<uint2 *>(&wh[w][d0]) = make_uint2(o0[w], run); run += c1[w]; }
            }
            __syncthreads();
#pragma unroll
            for (int it = 0; it < ITEMS; ++it) {
                if ((uint32_t)it < nit) {
                    const uint32_t li = wh[wave][dg[it] & (RA_RADIX - 1)] + (dg[it] >> RA_DB);
                    skeys[li] = kk[it]; sidx[li] = vv[it];
                }
            }
            __syncthreads();
        }
        if (KEYOUT) {
            const uint64_t km = keybits >= 32 ? 0xFFFFFFFFULL : ((1ULL << keybits) - 1ULL);
            for (uint32_t i = threadIdx.x; i < n; i += BLOCK) okey[1u + r0 + i] = (uint32_t)(skeys[i] & km);
            __syncthreads();
        }
        // the keys are not needed any more: their LDS holds the text positions, indexed by row before the sort
        uint32_t *sx = reinterpret_cast<uint32_t *>(skeys);
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) { const uint32_t i = threadIdx.x + (uint32_t)it * BLOCK; if (i < n) sx[i] = xi[it]; }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n; i += BLOCK) {
            uint32_t x = sx[sidx[i]];
            if (KEYOUT) { oflag[1u + r0 + i] = (uint8_t)(x >> 31); x &= 0x7FFFFFFFu; }
            SA[1u + r0 + i] = x;
            if (RANK) rank[x] = 1u + r0 + i;
        }
        ci = cj;
    }
}

// Assembly by merging (lists from SA(P2): the keys of every list ascend, and the keys of a class are distinct -- two rows of one
// phrase have strings of different lengths).  Ownership, batches of whole classes and the hand-off of classes larger than a tile as
// in k_rs_assemble; per batch only the slot bounds and ONE 32-bit key per row are in LDS:
//   * a class of one member slot is a copy of its list: the row is stored at its own index, its key is never read;
//   * a row of a class of m <= cap members stands at its index in its own list plus, for each other member, the number of that
//     member's keys below its own (a bisection in LDS) -- the ranking of k_emit_groups (emit.h) one level up;
//   * a batch that holds a class of more than cap members is appended to `fbl` and sorted by k_rs_assemble<., false, true>.
// pk = first slot of the class (12 bits: a batch has at most 3840 slots) | own slot - first (10) | members (10): cap <= 1023.
// Every bisection has a bounded trip count (ranges below 2^12) and nothing behind a loop depends on a value first set inside it (see k_rs_heads).
constexpr uint32_t RM_MAX_MEMBERS = 1023;
template <bool RANK> __global__ __launch_bounds__(BLOCK) void k_rs_merge(const uint4 *srec, const uint32_t *chead /*nc + 1*/, const uint32_t *crow /*nc + 1*/, uint32_t nc, const uint32_t *ikey, const uint32_t *ipos,
                                                                         uint32_t tile_rows, uint32_t cap, uint32_t *SA, uint32_t *rank, uint32_t *bigc, uint32_t *nbig, uint32_t *fbl, uint32_t *nfb)
{
    constexpr int ITEMS = RS_ITEMS, TILE = RS_TILE;
    constexpr uint32_t STEP = TILE / 2;
    static_assert(TILE <= 4096, "pk holds 12-bit slot indices");
    __shared__ uint32_t skey[TILE];
    __shared__ uint16_t srow[TILE + 1];
    __shared__ uint32_t ctl[4];
    const uint64_t w0 = (uint64_t)blockIdx.x * STEP;
    if (threadIdx.x == 0) { ctl[0] = rs_lower_bound(crow, 0u, nc, w0); ctl[1] = rs_lower_bound(crow, 0u, nc, w0 + STEP); }
    __syncthreads();
    uint32_t ci = ctl[0];
    const uint32_t ci1 = ctl[1];
    while (ci < ci1) {
        __syncthreads();                                       // ctl / LDS of the previous batch are free
        if (threadIdx.x == 0) {
            const uint64_t lim = (uint64_t)crow[ci] + tile_rows;
            uint32_t lo = ci, hi = ci1;                        // invariant: crow[lo] <= lim
            while (lo < hi) { const uint32_t mid = lo + ((hi - lo + 1) >> 1); if ((uint64_t)crow[mid] <= lim) lo = mid; else hi = mid - 1; }
            ctl[2] = lo; ctl[3] = 0u;
            if (lo == ci) bigc[atomicAdd(nbig, 1u)] = ci;
        }
        __syncthreads();
        const uint32_t cj = ctl[2];
        if (cj == ci) { ++ci; continue; }
        const uint32_t r0 = crow[ci], n = crow[cj] - r0, v0 = chead[ci], ns = chead[cj] - v0;
        for (uint32_t cc = ci + threadIdx.x; cc < cj; cc += BLOCK) if (chead[cc + 1] - chead[cc] > cap) ctl[3] = 1u;
        for (uint32_t t = threadIdx.x; t < ns; t += BLOCK) srow[t] = (uint16_t)(srec[v0 + t].x - r0);
        if (threadIdx.x == 0) srow[ns] = (uint16_t)n;
        __syncthreads();
        if (ctl[3]) {
            if (threadIdx.x == 0) { const uint32_t f = atomicAdd(nfb, 1u); fbl[2u * f] = ci; fbl[2u * f + 1u] = cj; }
            ci = cj; continue;
        }
        uint32_t xi[ITEMS], pk[ITEMS];
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
            const uint32_t i = threadIdx.x + (uint32_t)it * BLOCK;
            xi[it] = 0u; pk[it] = 0u;
            if (i < n) {
                uint32_t lo = 0, hi = ns - 1;                  // largest t with srow[t] <= i
                for (int b = 0; b < 12 && lo < hi; ++b) { const uint32_t mid = lo + ((hi - lo + 1) >> 1); if (srow[mid] <= i) lo = mid; else hi = mid - 1; }
                const uint4 rec = srec[v0 + lo];
                const uint32_t e = rec.y + (i - (rec.x - r0));
                const uint32_t sa = chead[rec.w] - v0, m = chead[rec.w + 1] - chead[rec.w];
                xi[it] = ipos[e] + rec.z;
                pk[it] = sa | ((lo - sa) << 12) | (m << 22);
                if (m > 1u) skey[i] = ikey[e];
            }
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
            const uint32_t i = threadIdx.x + (uint32_t)it * BLOCK;
            if (i < n) {
                const uint32_t sa = pk[it] & 0xFFFu, me = (pk[it] >> 12) & 0x3FFu, m = pk[it] >> 22;
                uint32_t place = i;
                if (m > 1u) {
                    const uint32_t key = skey[i];
                    place = (uint32_t)srow[sa] + (i - (uint32_t)srow[sa + me]);
                    for (uint32_t u = 0; u < m; ++u) {
                        if (u == me) continue;
                        const uint32_t a = srow[sa + u];
                        uint32_t lo = a, hi = srow[sa + u + 1u];   // keys of this member below `key`
                        for (int b = 0; b < 12 && lo < hi; ++b) { const uint32_t mid = lo + ((hi - lo) >> 1); if (skey[mid] < key) lo = mid + 1u; else hi = mid; }
                        place += lo - a;
                    }
                }
                SA[1u + r0 + place] = xi[it];
                if (RANK) rank[xi[it]] = 1u + r0 + place;
            }
        }
        ci = cj;
    }
}
// PFP_VERBOSE only: classes and rows by the member slots of the class -- hist[2b], hist[2b + 1] for 1, 2, 3-4, 5-8, 9-16, 17-64, > 64 members
__global__ __launch_bounds__(BLOCK) void k_rs_member_hist(const uint32_t *chead, const uint32_t *crow, uint64_t nc, unsigned long long *hist)
{
    const uint64_t ci = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (ci >= nc) return;
    const uint32_t m = chead[ci + 1] - chead[ci];
    const int b = m <= 1u ? 0 : m <= 2u ? 1 : m <= 4u ? 2 : m <= 8u ? 3 : m <= 16u ? 4 : m <= 64u ? 5 : 6;
    atomicAdd(&hist[2 * b], 1ULL); atomicAdd(&hist[2 * b + 1], (unsigned long long)(crow[ci + 1] - crow[ci]));
}

// ---- classes with more rows than a tile: their rows through the global radix sort ------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_rs_big_sizes(const uint32_t *bigc, uint64_t nb, const uint32_t *crow, uint32_t *sizes)
{
    const uint64_t b = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (b < nb) sizes[b] = crow[bigc[b] + 1] - crow[bigc[b]];
    else if (b == nb) sizes[b] = 0u;
}
__global__ __launch_bounds__(BLOCK) void k_rs_big_rows(const uint32_t *bigc, const uint32_t *bigoff /*nb + 1*/, uint32_t nb, uint64_t nbr, const uint32_t *crow, const uint32_t *chead, const uint4 *srec,
                                                       const uint32_t *ikey, const uint32_t *ipos, uint64_t *keys, uint32_t *vals, int flagged /*dictrec.h: bit 31 of a list position is a flag (see k_rs_assemble)*/)
{
    const uint64_t q = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= nbr) return;
    uint32_t lo = 0, hi = nb - 1;                              // largest b with bigoff[b] <= q
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo + 1) >> 1); if ((uint64_t)bigoff[mid] <= q) lo = mid; else hi = mid - 1; }
    const uint32_t b = lo, c = bigc[b], row = crow[c] + (uint32_t)(q - bigoff[b]);
    uint32_t vl = chead[c], vh = chead[c + 1] - 1;             // largest v with srec[v].x <= row
    while (vl < vh) { const uint32_t mid = vl + ((vh - vl + 1) >> 1); if (srec[mid].x <= row) vl = mid; else vh = mid - 1; }
    const uint4 rec = srec[vl];
    const uint32_t e = rec.y + (row - rec.x);
    keys[q] = ((uint64_t)b << 32) | ikey[e];
    vals[q] = flagged ? (rec.z ? (ipos[e] & 0x7FFFFFFFu) + rec.z : ipos[e]) : ipos[e] + rec.z;
}
template <bool RANK, bool KEYOUT> __global__ __launch_bounds__(BLOCK) void k_rs_big_store(const uint64_t *keys, const uint32_t *vals, uint64_t nbr, const uint32_t *bigc, const uint32_t *bigoff, const uint32_t *crow, uint32_t *SA, uint32_t *rank, uint32_t *okey, uint8_t *oflag)
{
    const uint64_t q = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= nbr) return;
    const uint32_t b = (uint32_t)(keys[q] >> 32);
    const uint32_t row = crow[bigc[b]] + (uint32_t)(q - bigoff[b]);
    uint32_t x = vals[q];
    if (KEYOUT) { oflag[1u + row] = (uint8_t)(x >> 31); x &= 0x7FFFFFFFu; }
    SA[1u + row] = x;
    if (RANK) rank[x] = 1u + row;
    if (KEYOUT) okey[1u + row] = (uint32_t)keys[q];
}
__global__ __launch_bounds__(BLOCK) void k_rs_first_row(uint32_t *SA, uint32_t *rank, uint64_t N)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) { SA[0] = (uint32_t)(N - 1); if (rank) rank[N - 1] = 0u; }
}

inline int sort_int_suffixes(pfp_ctx *c, const uint32_t *dS, uint64_t N, uint64_t maxsym, uint32_t *SA, uint32_t *rank, int *rounds, int depth = 0, bool want_rank = true);

// prefix doubling (sufsort.h): the bottom of the recursion and the route of inputs that do not shrink
inline int sort_int_suffixes_doubling(pfp_ctx *c, const uint32_t *dS, uint64_t N, uint64_t maxsym, uint32_t *SA, uint32_t *rank, int *rounds)
{
    const size_t mk = c->arena.mark_hi();
    uint64_t *k0, *k1; uint32_t *v0, *v1;
    PFP_ALLOC_HI(c, k0, uint64_t, N); PFP_ALLOC_HI(c, k1, uint64_t, N);
    PFP_ALLOC_HI(c, v0, uint32_t, N); PFP_ALLOC_HI(c, v1, uint32_t, N);
    const int sb = bits_for(maxsym);
    const int nsym = (c->tun.int_key_symbols == 3 && 3 * sb <= 64) ? 3 : 2;
    PFP_LAUNCH(c, K_SS_INIT_KEYS, N * 16, k_int_init_keys, nblocks(N, BLOCK), dS, N, sb, nsym, k0, v0);
    BitRange rr = {0, nsym * sb};
    PFP_TRY(suffix_sort_doubling<false>(c, N, k0, v0, k1, v1, &rr, 1, (uint32_t)nsym, (const uint8_t *)nullptr, SA, rank, (uint2 *)nullptr, rounds));
    c->arena.release_hi(mk);
    return PFP_OK;
}

// ---- host: the stages that the two level-2 sorts share (suffix_sort_pfp below; dict_sort_pfp, dictrec.h) ---------------------------
// Slots of the counter block d_cnt (uint32_t; the parse route allocates 8, the dictionary route 16).  Three slots have two lives.  The memset
// in l2_assemble starts the second lives of L2_LONGEST and L2_OVERFLOW; every first life has been read back by then.  L2_PHRASES has no reset:
// its second life starts in l2_classes, where a compaction stores its total over k (device_scan writes the total, it does not add to it);
// nc is read back in l2_classes, so the memset in l2_assemble only wipes a value that nobody reads again.
enum L2Counter {
    L2_PHRASES = 0,      // k, the total of the trigger counts; from l2_classes on, without a reset (above): nc, the number of classes
    L2_LONGEST = 1,      // longest level-2 phrase (atomicMax); from l2_assemble on: the classes with more rows than a tile (fill of bigc)
    L2_BIG_ROWS = 2,     // rows of those classes
    L2_OVERFLOW = 3,     // the phrase table is too full; from l2_assemble on: batches the merge hands to the LDS sort (fill of fbl)
    L2_WORDS = 4,        // nw, distinct phrases
    L2_D2 = 5,           // length of D2 (without the dictionary route's final EndOfDict)
    L2_ROWS = 6,         // rows of all slots: N - 1
    L2_SLOTS = 7,        // nv, slots of SA(D2) that stand for a string
    L2_OPEN = 8,         // dictionary route only: neighbour pairs of SA(P2) that the last tie pass left open
};
// the 32-bit bounds of the two routes, side by side.  Parse: positions, D2 offsets and symbols + 2 are uint32_t; D2 has at most N - 1 + 2k
// symbols (phrases overlap by one, + a separator each).  Dictionary: bit 31 of a list position is the word-start flag (k_dr_list_payload)
inline bool rs_fits_32(uint64_t N, uint64_t maxsym) { return N + 64 < 0xFFFFFFFFULL && maxsym + 2 < 0xFFFFFFFFULL; }
inline bool rs_d2_fits_32(uint64_t N, uint64_t k) { return N + 2 * k < 0xFFFFFFFFULL; }
inline bool dr_fits_32(uint64_t N) { return N + 64 < 0x7FFFFFFFULL; }

// the arrays and counts that travel between the stages.  inv0 / wid1 / inv1 (buffers of l2_inverted_lists) and bigc (l2_assemble) serve one
// stage only; the routes allocate them, each at its own place in the order of allocations
struct Level2 {
    size_t mk;                                 // the route's arena mark
    uint64_t N, k, nw, nv, nc, tsize;          // string length (rows: N - 1), phrases, distinct phrases, valid slots, classes, table slots
    uint32_t maxlen, overflow, nd32, nb, nfb;  // longest phrase, table too full, wstart[nw], classes larger than a tile, batches of the merge sorted in LDS
    uint32_t *bcnt, *d_cnt;
    uint32_t *ps, *eid, *isrep, *replist, *slot2id, *wrep, *wstart, *woff, *inv0, *wid1, *inv1, *inv;
    uint32_t *valid, *rows, *whole, *rowoff, *wposs, *wrank;
    uint32_t *vlist, *chead, *crow, *bigc, *ikey, *ipos; uint4 *srec;
    int keybits; uint32_t tile_rows, cap; bool merge;      // assembly: key width, rows per batch; parse route: member cap of the merge, rows merged
};
// where the assembly writes: rank (nullable) for the parse; okey / oflag (the key of every row, word-start flags) for the dictionary
struct L2Rows { uint32_t *SA, *rank, *okey; uint8_t *oflag; };

inline int l2_give_up(pfp_ctx *c, const Level2 &L, int rc = PFP_OK) { c->arena.release_hi(L.mk); return rc; }
inline uint32_t l2_tile_rows(const pfp_ctx *c)
{
    const uint32_t t = c->tun.parse_rec_tile_rows ? c->tun.parse_rec_tile_rows : (uint32_t)RS_TILE;
    return t > (uint32_t)RS_TILE ? (uint32_t)RS_TILE : t < 2 ? 2u : t;
}

// 1. the counter block (ncnt slots) and the number of phrases: count(bcnt) launches the route's trigger count over gt workgroups
template <class Count> inline int l2_count_phrases(pfp_ctx *c, Level2 &L, unsigned gt, uint32_t ncnt, Count count)
{
    PFP_ALLOC_HI(c, L.bcnt, uint32_t, gt); PFP_ALLOC_HI(c, L.d_cnt, uint32_t, ncnt);
    PFP_HIP(c, hipMemsetAsync(L.d_cnt, 0, ncnt * 4, c->stream));
    PFP_TRY(count(L.bcnt));
    PFP_TRY((device_scan<uint32_t, 0>(c, L.bcnt, L.bcnt, (uint64_t)gt, L.d_cnt + L2_PHRASES)));
    uint32_t k32 = 0; PFP_TRY(d2h_u32(c, L.d_cnt + L2_PHRASES, &k32));
    L.k = k32;
    return PFP_OK;
}
// 2. distinct phrases.  The table has 2^parse_rec_table_log2 slots, or by default one per `per_slot` phrases; dedup(table, tmask) launches
// the route's k_*_dedup (-> eid, isrep, L2_OVERFLOW).  L.overflow: nothing more was done, the caller gives the route up
template <class Dedup> inline int l2_dedup(pfp_ctx *c, Level2 &L, uint64_t per_slot, Dedup dedup)
{
    int tl = c->tun.parse_rec_table_log2 > 0 ? c->tun.parse_rec_table_log2 : bits_for(L.k / per_slot + 1023);
    if (tl > 31) tl = 31;
    L.tsize = 1ULL << tl;
    unsigned long long *table; uint32_t *pos;
    PFP_ALLOC_HI(c, table, unsigned long long, L.tsize); PFP_ALLOC_HI(c, L.eid, uint32_t, L.k); PFP_ALLOC_HI(c, L.isrep, uint32_t, L.k); PFP_ALLOC_HI(c, pos, uint32_t, L.k);
    PFP_HIP(c, hipMemsetAsync(table, 0, L.tsize * 8, c->stream));
    PFP_TRY(dedup(table, (uint32_t)(L.tsize - 1)));
    PFP_TRY(d2h_u32(c, L.d_cnt + L2_OVERFLOW, &L.overflow));
    if (L.overflow) return PFP_OK;
    PFP_ALLOC_HI(c, L.replist, uint32_t, L.k < L.tsize ? L.k : L.tsize);
    PFP_TRY(device_compact(c, nullptr, L.isrep, L.k, L.replist, pos, L.d_cnt + L2_WORDS));
    uint32_t nw32 = 0; PFP_TRY(d2h_u32(c, L.d_cnt + L2_WORDS, &nw32));
    L.nw = nw32;
    return PFP_OK;
}
// deterministic ids: the distinct phrases in the order of the 64-bit keys that keys(hk, hv) launches (k_*_rep_keys); ids(sorted) launches the
// route's k_*_assign_ids, which leaves the D2 length of every word in wstart.  L.nd32 = their sum, wstart = their offsets
template <class Keys, class Ids> inline int l2_word_ids(pfp_ctx *c, Level2 &L, Keys keys, Ids ids)
{
    const size_t mk2 = c->arena.mark_hi();
    uint64_t *hk0, *hk1; uint32_t *hv0, *hv1;
    PFP_ALLOC_HI(c, hk0, uint64_t, L.nw); PFP_ALLOC_HI(c, hk1, uint64_t, L.nw); PFP_ALLOC_HI(c, hv0, uint32_t, L.nw); PFP_ALLOC_HI(c, hv1, uint32_t, L.nw);
    PFP_TRY(keys(hk0, hv0));
    BitRange hr = {0, 64};
    uint64_t *sk; uint32_t *sv;
    PFP_TRY(radix_sort_pairs<uint64_t>(c, hk0, hv0, hk1, hv1, L.nw, &hr, 1, &sk, &sv));
    PFP_TRY(ids((const uint32_t *)sv));
    c->arena.release_hi(mk2);
    PFP_TRY((device_scan<uint32_t, 0>(c, L.wstart, L.wstart, L.nw + 1, L.d_cnt + L2_D2)));      // wstart[nw] = the sum
    return d2h_u32(c, L.d_cnt + L2_D2, &L.nd32);
}
// 3. inverted lists: the phrases grouped by word id (stable: ascending inside a word), inv = the phrases, woff[id] = first entry of a word.
// The ids in phrase order stay behind in eid (in place: the table slot is not needed any more); the sort consumes its own copy in isrep
inline int l2_inverted_lists(pfp_ctx *c, Level2 &L)
{
    PFP_LAUNCH(c, K_REC_DEDUP, L.k * 16, k_rs_wid, nblocks(L.k, BLOCK), (const uint32_t *)L.eid, (const uint32_t *)L.slot2id, L.k, L.isrep, L.eid, L.inv0);
    BitRange wr = {0, bits_for(L.nw ? L.nw - 1 : 0)};
    uint32_t *swid;
    PFP_TRY(radix_sort_pairs<uint32_t>(c, L.isrep, L.inv0, L.wid1, L.inv1, L.k, &wr, 1, &swid, &L.inv));
    PFP_LAUNCH(c, K_REC_PARSE, L.k * 4, k_rs_list_bounds, nblocks(L.k, BLOCK), (const uint32_t *)swid, L.k, L.nw, L.woff);
    return PFP_OK;
}
// 7. slots to classes: first row of every slot (their sum must be N - 1), the valid slots, heads(vlist, nv, head) launches the route's head
// kernel, the slot records and the first row of every class.  woff is indexed by word id, or -- wrank given -- by word rank
template <class Heads> inline int l2_classes(pfp_ctx *c, Level2 &L, const uint32_t *SAD, const uint32_t *wd, uint64_t ND, const uint32_t *wrank /*nullable*/, Heads heads)
{
    PFP_TRY((device_scan<uint32_t, 0>(c, L.rows, L.rowoff, ND, L.d_cnt + L2_ROWS)));
    uint32_t R32 = 0; PFP_TRY(d2h_u32(c, L.d_cnt + L2_ROWS, &R32));
    if ((uint64_t)R32 != L.N - 1) return l2_give_up(c, L, PFP_E_CORRUPT);
    uint32_t *head;
    PFP_ALLOC_HI(c, L.vlist, uint32_t, ND); PFP_ALLOC_HI(c, head, uint32_t, ND); PFP_ALLOC_HI(c, L.chead, uint32_t, ND + 1); PFP_ALLOC_HI(c, L.crow, uint32_t, ND + 1);
    PFP_TRY(device_compact(c, nullptr, L.valid, ND, L.vlist, L.wposs, L.d_cnt + L2_SLOTS));      // the slots that stand for a string
    uint32_t nv32 = 0; PFP_TRY(d2h_u32(c, L.d_cnt + L2_SLOTS, &nv32));
    L.nv = nv32;
    PFP_ALLOC_HI(c, L.srec, uint4, L.nv);
    PFP_TRY(heads((const uint32_t *)L.vlist, L.nv, head));
    PFP_TRY(device_compact(c, nullptr, head, L.nv, L.chead, L.wposs, L.d_cnt + L2_PHRASES));      // wposs[v] = heads in front of v; the slot's second life: nc
    PFP_LAUNCH(c, K_REC_PARSE, L.nv * 44, k_rs_slot_records, nblocks(L.nv, BLOCK), SAD, (const uint32_t *)L.vlist, (const uint32_t *)L.rowoff, (const uint32_t *)head, (const uint32_t *)L.wposs, wd,
               (const uint32_t *)L.wstart, (const uint32_t *)L.woff, wrank, L.nv, L.srec);
    uint32_t nc32 = 0; PFP_TRY(d2h_u32(c, L.d_cnt + L2_PHRASES, &nc32));
    L.nc = nc32;
    PFP_LAUNCH(c, K_REC_PARSE, L.nc * 24, k_rs_class_rows, nblocks(L.nc + 1, BLOCK), (const uint32_t *)L.chead, (const uint4 *)L.srec, L.nc, L.nv, L.N - 1, L.crow, L.chead + L.nc);
    return PFP_OK;
}
// 8. assembly: every class of at most tile_rows rows is stored (k_rs_assemble; L.merge: k_rs_merge, which hands the batches with a class of
// more than cap members to k_rs_assemble), the others are listed in bigc (L.nb of them); row 0.  Algorithmic bytes per row: list entry 8 in, text
// position 4 out (+ 4 rank or key); per slot 16
template <bool RANK, bool KEYOUT> inline int l2_assemble_as(pfp_ctx *c, Level2 &L, const L2Rows &o)
{
    const uint64_t N = L.N, bytes = (N - 1) * (RANK || KEYOUT ? 16 : 12) + L.nv * 16;
    const unsigned ga = nblocks(N - 1, RS_TILE / 2);
    const bool merge = !KEYOUT && L.merge;
    uint32_t *d_nbig = L.d_cnt + L2_LONGEST, *d_nfb = L.d_cnt + L2_OVERFLOW;
    PFP_HIP(c, hipMemsetAsync(L.d_cnt, 0, 32, c->stream));      // the second lives of L2_LONGEST and L2_OVERFLOW start at 0
    if constexpr (!KEYOUT) if (merge) {
        uint32_t *fbl; PFP_ALLOC_HI(c, fbl, uint32_t, 2 * (L.nv / (L.cap + 1u) + 1u));      // such a batch has more than cap slots, and batches share none
        PFP_LAUNCH(c, K_REC_ASSEMBLE, bytes, (k_rs_merge<RANK>), ga, (const uint4 *)L.srec, (const uint32_t *)L.chead, (const uint32_t *)L.crow, (uint32_t)L.nc, (const uint32_t *)L.ikey, (const uint32_t *)L.ipos,
                   L.tile_rows, L.cap, o.SA, o.rank, L.bigc, d_nbig, fbl, d_nfb);
        PFP_TRY(d2h_u32(c, d_nfb, &L.nfb));
        if (L.nfb) PFP_LAUNCH(c, K_REC_ASSEMBLE, 0, (k_rs_assemble<RANK, false, true>), L.nfb, (const uint4 *)L.srec, (const uint32_t *)L.chead, (const uint32_t *)L.crow, (uint32_t)L.nc, (const uint32_t *)L.ikey, (const uint32_t *)L.ipos,
                              L.keybits, L.tile_rows, o.SA, o.rank, L.bigc, d_nbig, (uint32_t *)nullptr, (uint8_t *)nullptr, (const uint32_t *)fbl);
    }
    if (!merge) PFP_LAUNCH(c, K_REC_ASSEMBLE, bytes, (k_rs_assemble<RANK, KEYOUT>), ga, (const uint4 *)L.srec, (const uint32_t *)L.chead, (const uint32_t *)L.crow, (uint32_t)L.nc, (const uint32_t *)L.ikey, (const uint32_t *)L.ipos,
                           L.keybits, L.tile_rows, o.SA, o.rank, L.bigc, d_nbig, o.okey, o.oflag, (const uint32_t *)nullptr);
    PFP_LAUNCH(c, K_MISC, 8, k_rs_first_row, 1, o.SA, o.rank, N);
    PFP_TRY(d2h_u32(c, d_nbig, &L.nb));
    if (!L.nb) return PFP_OK;
    // 9. the classes with more rows than a tile: their rows through the global radix sort, keyed by (class, rank of the sampled suffix)
    const uint64_t nb = L.nb;
    uint32_t *bigoff; PFP_ALLOC_HI(c, bigoff, uint32_t, nb + 1);
    PFP_LAUNCH(c, K_REC_PARSE, nb * 12, k_rs_big_sizes, nblocks(nb + 1, BLOCK), (const uint32_t *)L.bigc, nb, (const uint32_t *)L.crow, bigoff);
    PFP_TRY((device_scan<uint32_t, 0>(c, bigoff, bigoff, nb + 1, L.d_cnt + L2_BIG_ROWS)));
    uint32_t nbr32 = 0; PFP_TRY(d2h_u32(c, L.d_cnt + L2_BIG_ROWS, &nbr32));
    const uint64_t nbr = nbr32;
    if (c->tun.verbose) fprintf(stderr, "[pfbwt_hip]   assembly: %llu classes with more than %u rows (%llu rows) through the global sort\n", (unsigned long long)nb, L.tile_rows, (unsigned long long)nbr);
    uint64_t *bk0, *bk1; uint32_t *bv0, *bv1;
    PFP_ALLOC_HI(c, bk0, uint64_t, nbr); PFP_ALLOC_HI(c, bk1, uint64_t, nbr); PFP_ALLOC_HI(c, bv0, uint32_t, nbr); PFP_ALLOC_HI(c, bv1, uint32_t, nbr);
    PFP_LAUNCH(c, K_REC_PARSE, nbr * 40, k_rs_big_rows, nblocks(nbr, BLOCK), (const uint32_t *)L.bigc, (const uint32_t *)bigoff, (uint32_t)nb, nbr, (const uint32_t *)L.crow, (const uint32_t *)L.chead, (const uint4 *)L.srec,
               (const uint32_t *)L.ikey, (const uint32_t *)L.ipos, bk0, bv0, KEYOUT ? 1 : 0);
    BitRange br[2] = {{0, L.keybits}, {32, 32 + bits_for(nb - 1)}};
    uint64_t *sk; uint32_t *sv;
    PFP_TRY(radix_sort_pairs<uint64_t>(c, bk0, bv0, bk1, bv1, nbr, br, 2, &sk, &sv));
    PFP_LAUNCH(c, K_REC_PARSE, nbr * (RANK || KEYOUT ? 24 : 20), (k_rs_big_store<RANK, KEYOUT>), nblocks(nbr, BLOCK), (const uint64_t *)sk, (const uint32_t *)sv, nbr, (const uint32_t *)L.bigc, (const uint32_t *)bigoff,
               (const uint32_t *)L.crow, o.SA, o.rank, o.okey, o.oflag);
    return PFP_OK;
}
// the template arguments from the output: keys are kept (and never a rank) for the dictionary; rank != nullptr for the parse
inline int l2_assemble(pfp_ctx *c, Level2 &L, const L2Rows &o)
{
    return o.okey ? l2_assemble_as<false, true>(c, L, o) : o.rank ? l2_assemble_as<true, false>(c, L, o) : l2_assemble_as<false, false>(c, L, o);
}

// ---- the parse route -------------------------------------------------------------------------------------------------------------------
// PFP_VERBOSE: rows and classes by the member slots of the class (what decides between merging and sorting), batches the merge handed to the LDS sort
inline int rs_report(pfp_ctx *c, const Level2 &L, HostTimer &tm, bool slices)
{
    unsigned long long *d_hist, h[14];
    PFP_ALLOC_HI(c, d_hist, unsigned long long, 14);
    PFP_HIP(c, hipMemsetAsync(d_hist, 0, sizeof h, c->stream));
    PFP_LAUNCH(c, K_MISC, L.nc * 8, k_rs_member_hist, nblocks(L.nc, BLOCK), (const uint32_t *)L.chead, (const uint32_t *)L.crow, L.nc, d_hist);
    PFP_HIP(c, hipMemcpyAsync(h, d_hist, sizeof h, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    fprintf(stderr, "[pfbwt_hip]   assembled: %llu slots, %llu classes (%.1f ms); lists %s, rows %s; classes / rows by members 1: %llu / %llu, 2: %llu / %llu, 3-4: %llu / %llu, 5-8: %llu / %llu, "
                    "9-16: %llu / %llu, 17-64: %llu / %llu, >64: %llu / %llu; %u batches with a class of more than %u members sorted\n", (unsigned long long)L.nv, (unsigned long long)L.nc, tm.ms(),
            slices ? "from SA(P2) slices" : "sorted by word", L.merge ? "merged" : "sorted in LDS", h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], h[9], h[10], h[11], h[12], h[13], L.nfb, L.cap);
    return PFP_OK;
}
// *taken = 0: nothing was written, the caller sorts by doubling
inline int suffix_sort_pfp(pfp_ctx *c, const uint32_t *dS, uint64_t N, uint64_t maxsym, uint32_t *SA, uint32_t *rank /*nullable*/, int depth, int *taken)
{
    *taken = 0;
    const bool forced = c->tun.parse_rec > 0, verbose = c->tun.verbose != 0;
    const bool slices = c->tun.parse_rec_merge != 0;           // lists from SA(P2); rows merged (parse_rec_merge == 1) or sorted in LDS
    const uint32_t p2 = c->tun.parse_rec_p2 >= 2 ? (uint32_t)c->tun.parse_rec_p2 : 4u;
    Level2 L = {}; L.N = N;
    // ---- when the route is given up (every line under PFP_VERBOSE)
    const auto too_few_or_many_phrases = [&] { return L.k < 2 || (!forced && L.k * 2 > N); };
    const auto d2_over_32_bits = [&] { const bool out = !rs_d2_fits_32(N, L.k); if (out && verbose) fprintf(stderr, "[pfbwt_hip] recursive parse sort given up: N + 2 * %llu phrases do not fit 32 bits\n", (unsigned long long)L.k); return out; };
    const auto phrase_too_long = [&] { if (L.maxlen > REC_MAX_PHRASE && verbose) fprintf(stderr, "[pfbwt_hip] recursive parse sort given up: a level-2 phrase of %u symbols\n", L.maxlen); return L.maxlen > REC_MAX_PHRASE; };
    const auto table_too_full = [&] {
        if (L.overflow && verbose) fprintf(stderr, "[pfbwt_hip] recursive parse sort given up: the table of %llu slots is too full for the distinct level-2 phrases among %llu\n", (unsigned long long)L.tsize, (unsigned long long)L.k);
        return L.overflow != 0;
    };
    const auto not_repetitive = [&](uint64_t ND) { return !forced && (ND + L.k) * 10 > N * 6; };      // does not shrink enough to pay for the assembly

    if (N < 8 || !rs_fits_32(N, maxsym)) return PFP_OK;        // too short; over 32 bits
    L.mk = c->arena.mark_hi();
    HostTimer tm;
    // 1. level-2 phrases; the last one ends in the final 0
    const unsigned gt = nblocks(N, RS_TRIG_TILE);
    PFP_TRY(l2_count_phrases(c, L, gt, 8, [&](uint32_t *bcnt) -> int { PFP_LAUNCH(c, K_REC_PARSE, N * 4, k_rs_trig_count, gt, dS, N, p2, bcnt); return PFP_OK; }));
    const uint64_t k = L.k;
    if (too_few_or_many_phrases() || d2_over_32_bits()) return l2_give_up(c, L);
    PFP_ALLOC_HI(c, L.ps, uint32_t, k + 1);
    const uint32_t *ps = L.ps;
    PFP_LAUNCH(c, K_REC_PARSE, N * 4 + k * 4, k_rs_trig_write, gt, dS, N, p2, (const uint32_t *)L.bcnt, L.ps);
    PFP_LAUNCH(c, K_REC_PARSE, k * 4, k_rs_max_phrase, nblocks(k, BLOCK), ps, k, L.d_cnt + L2_LONGEST);
    PFP_TRY(d2h_u32(c, L.d_cnt + L2_LONGEST, &L.maxlen));
    if (phrase_too_long()) return l2_give_up(c, L);
    // 2. distinct phrases (S-32G: 16 M slots for 2.6 M distinct among 81 M phrases)
    // (the per-XCD column order of the text de-duplication, parse.h, was tried here too: the parse of a collection is laid out like its text.  No gain: 72.4 against 72.1 ms of parse BWT, r04po)
    PFP_TRY(l2_dedup(c, L, 8, [&](unsigned long long *table, uint32_t tmask) -> int {
        PFP_LAUNCH(c, K_REC_DEDUP, N * 8 + k * 24, k_rs_dedup, nblocks(k, BLOCK), dS, ps, k, table, tmask, L.eid, L.isrep, L.d_cnt + L2_OVERFLOW); return PFP_OK; }));
    if (table_too_full()) return l2_give_up(c, L);
    const uint64_t nw = L.nw;
    PFP_ALLOC_HI(c, L.slot2id, uint32_t, L.tsize); PFP_ALLOC_HI(c, L.wrep, uint32_t, nw); PFP_ALLOC_HI(c, L.wstart, uint32_t, nw + 1);
    if (!slices) { PFP_ALLOC_HI(c, L.inv0, uint32_t, k); PFP_ALLOC_HI(c, L.wid1, uint32_t, k); PFP_ALLOC_HI(c, L.inv1, uint32_t, k); }
    PFP_ALLOC_HI(c, L.woff, uint32_t, nw + 2);                 // list starts by word id [0, nw], or (slices) by word rank [1, nw + 1]
    // (word ids: the order of the content hashes; the phrase that holds the final 0 last)
    PFP_TRY(l2_word_ids(c, L,
        [&](uint64_t *hk, uint32_t *hv) -> int { PFP_LAUNCH(c, K_REC_DEDUP, nw * 40, k_rs_rep_keys, nblocks(nw, BLOCK), dS, ps, (const uint32_t *)L.replist, nw, k, hk, hv); return PFP_OK; },
        [&](const uint32_t *sorted) -> int { PFP_LAUNCH(c, K_REC_DEDUP, nw * 24, k_rs_assign_ids, nblocks(nw + 1, BLOCK), sorted, (const uint32_t *)L.replist, (const uint32_t *)L.eid, ps, nw, L.slot2id, L.wrep, L.wstart); return PFP_OK; }));
    const uint64_t ND = L.nd32;
    if (verbose) fprintf(stderr, "[pfbwt_hip] recursive parse sort (depth %d): N=%llu -> %llu phrases (longest %u), %llu distinct, D2=%llu symbols (%.1f ms so far)\n", depth, (unsigned long long)N,
                         (unsigned long long)k, L.maxlen, (unsigned long long)nw, (unsigned long long)ND, tm.ms());
    if (not_repetitive(ND)) return l2_give_up(c, L);
    // 3. inverted lists; with `slices` they are read off SA(P2) in stage 7 and only the ids in phrase order are made
    if (slices) PFP_LAUNCH(c, K_REC_DEDUP, k * 8, k_rs_wid_keep, nblocks(k, BLOCK), (const uint32_t *)L.eid, (const uint32_t *)L.slot2id, k, L.eid /*in place*/);
    else PFP_TRY(l2_inverted_lists(c, L));
    const uint32_t *widp = L.eid;                              // word ids in phrase order
    // 4. D2 and its suffix array
    uint32_t *D, *wd, *SAD;
    PFP_ALLOC_HI(c, D, uint32_t, ND + 4); PFP_ALLOC_HI(c, wd, uint32_t, ND); PFP_ALLOC_HI(c, SAD, uint32_t, ND);
    PFP_LAUNCH(c, K_REC_PARSE, ND * 12, k_rs_dict_build, nblocks(nw, BLOCK), dS, ps, (const uint32_t *)L.wrep, (const uint32_t *)L.wstart, nw, D, wd);
    {
        const size_t mk2 = c->arena.mark_hi();
        uint32_t *rkD; PFP_ALLOC_HI(c, rkD, uint32_t, ND);
        int r2 = 0;
        PFP_TRY(sort_int_suffixes(c, D, ND, maxsym + 2, SAD, rkD, &r2, depth + 1, false));
        c->arena.release_hi(mk2);
    }
    if (verbose) fprintf(stderr, "[pfbwt_hip]   D2 sorted (%.1f ms so far)\n", tm.ms());
    // 5. slots (with `slices` only their flags: the rows are known behind the sort of P2), word ranks, names
    uint32_t *P2, *SA2, *R2; uint2 *pp = nullptr;
    PFP_ALLOC_HI(c, L.valid, uint32_t, ND); PFP_ALLOC_HI(c, L.rows, uint32_t, ND); PFP_ALLOC_HI(c, L.whole, uint32_t, ND); PFP_ALLOC_HI(c, L.rowoff, uint32_t, ND); PFP_ALLOC_HI(c, L.wposs, uint32_t, ND);
    PFP_ALLOC_HI(c, L.wrank, uint32_t, nw); PFP_ALLOC_HI(c, P2, uint32_t, k + 1); PFP_ALLOC_HI(c, SA2, uint32_t, k + 1); PFP_ALLOC_HI(c, R2, uint32_t, k + 1);
    if (slices) PFP_LAUNCH(c, K_REC_PARSE, ND * 24, k_rs_slot_flags, nblocks(ND, BLOCK), (const uint32_t *)SAD, (const uint32_t *)wd, (const uint32_t *)L.wstart, ND, L.whole, L.valid);
    else PFP_LAUNCH(c, K_REC_PARSE, ND * 28, k_rs_slots, nblocks(ND, BLOCK), (const uint32_t *)SAD, (const uint32_t *)wd, (const uint32_t *)L.wstart, (const uint32_t *)L.woff, ND, L.rows, L.whole, L.valid);
    PFP_TRY((device_scan<uint32_t, 0>(c, L.whole, L.wposs, ND, nullptr)));
    PFP_LAUNCH(c, K_REC_PARSE, ND * 16, k_rs_word_ranks, nblocks(ND, BLOCK), (const uint32_t *)SAD, (const uint32_t *)wd, (const uint32_t *)L.whole, (const uint32_t *)L.wposs, ND, 1u, L.wrank);
    if (slices) {
        PFP_ALLOC_HI(c, pp, uint2, k);
        PFP_LAUNCH(c, K_REC_PARSE, k * 24, k_rs_names_pos, nblocks(k + 1, BLOCK), widp, (const uint32_t *)L.wrank, ps, k, P2, pp);
    } else PFP_LAUNCH(c, K_REC_PARSE, k * 12, k_rs_names, nblocks(k + 1, BLOCK), widp, (const uint32_t *)L.wrank, k, P2);
    // 6. P2 and its suffix array
    {
        int r2 = 0;
        PFP_TRY(sort_int_suffixes(c, P2, k + 1, nw, SA2, R2, &r2, depth + 1, true));
    }
    if (verbose) fprintf(stderr, "[pfbwt_hip]   P2 sorted (%.1f ms so far)\n", tm.ms());
    // 7. list payload, slot records and classes
    L.ikey = SA2 /*not needed any more*/; L.ipos = P2;
    if (slices) {
        // (the keys get an array of their own: a workgroup's first thread reads the SA2 entry of its neighbour workgroup; P2 is free, its names are in pp)
        PFP_ALLOC_HI(c, L.ikey, uint32_t, k + 1);
        PFP_LAUNCH(c, K_REC_PARSE, k * 24, k_rs_slice_payload, nblocks(k, BLOCK), (const uint32_t *)SA2, (const uint2 *)pp, (const uint32_t *)R2, k, nw, L.ikey, L.ipos, L.woff);
        PFP_LAUNCH(c, K_REC_PARSE, ND * 20, k_rs_slot_rows, nblocks(ND, BLOCK), (const uint32_t *)SAD, (const uint32_t *)wd, (const uint32_t *)L.valid, (const uint32_t *)L.wrank, (const uint32_t *)L.woff, ND, L.rows);
    } else PFP_LAUNCH(c, K_REC_PARSE, k * 20, k_rs_list_payload, nblocks(k, BLOCK), (const uint32_t *)L.inv, (const uint32_t *)R2, ps, k, L.ikey, L.ipos);
    PFP_TRY(l2_classes(c, L, SAD, wd, ND, slices ? (const uint32_t *)L.wrank : (const uint32_t *)nullptr, [&](const uint32_t *vlist, uint64_t nv, uint32_t *head) -> int {
        PFP_LAUNCH(c, K_REC_PARSE, nv * 40, k_rs_heads, nblocks(nv, BLOCK), (const uint32_t *)D, (const uint32_t *)SAD, vlist, nv, head); return PFP_OK; }));
    // 8. assembly, 9. big classes
    L.tile_rows = l2_tile_rows(c); L.keybits = bits_for(k);
    L.merge = c->tun.parse_rec_merge == 1;
    L.cap = c->tun.parse_rec_merge_members ? c->tun.parse_rec_merge_members : 1u;
    if (L.cap > RM_MAX_MEMBERS) L.cap = RM_MAX_MEMBERS;
    PFP_ALLOC_HI(c, L.bigc, uint32_t, L.nc + 1);
    const L2Rows out = {SA, rank, nullptr, nullptr};
    PFP_TRY(l2_assemble(c, L, out));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    if (verbose) PFP_TRY(rs_report(c, L, tm, slices));
    c->arena.release_hi(L.mk);
    *taken = 1;
    return PFP_OK;
}

// suffix array of S[0..N) (S[N-1] == 0 unique smallest), integer alphabet with values <= maxsym; rank[x] = slot of suffix x
// (written when want_rank; always by the doubling route, which works in it)
inline int sort_int_suffixes(pfp_ctx *c, const uint32_t *dS, uint64_t N, uint64_t maxsym, uint32_t *SA, uint32_t *rank, int *rounds, int depth, bool want_rank)
{
    const int mode = c->tun.parse_rec;                         // -1: by the input's shape, 0: never, 1: wherever the route can run at all
    const int max_depth = c->tun.parse_rec_depth > 0 ? c->tun.parse_rec_depth : 1;
    if (mode != 0 && depth < max_depth) {
        // a repetitive collection: few distinct symbols for its length (S-32G: 1.5 M words, 325 M phrases); a single genome's parse
        // (nearly every phrase its own word) has nothing to gain
        const bool shape = N >= c->tun.parse_rec_min && maxsym * 8 <= N;
        if (mode > 0 || shape) {
            int taken = 0;
            PFP_TRY(suffix_sort_pfp(c, dS, N, maxsym, SA, want_rank ? rank : (uint32_t *)nullptr, depth, &taken));
            if (taken) { if (rounds) *rounds = 1; return PFP_OK; }
        }
    }
    return sort_int_suffixes_doubling(c, dS, N, maxsym, SA, rank, rounds);
}

} // namespace pfp
