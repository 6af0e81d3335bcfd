// pfbwt-f_amd/csrc/doclist.h -- document listing with frequencies on the device (pfp_ri_docs, include/pfbwt_hip.h; DESIGN.md
// section 2): in which records a pattern occurs and how often in each.  The search is k_ri_search and the positions of a pattern come
// from k_ri_pieces / k_ri_walk / k_ri_rows (runindex.h) into scratch; what is new here is the reduction of a pattern's positions to
// (document, frequency) pairs.  The host (queries.h) cuts the patterns into chunks whose reported rows fit a budget; per chunk:
//   1. k_dl_map: one lane per position, doc(s) by the bisection of docarray.h (the start table, or every 2^shift-th start of a large
//      one, in LDS) and, with PFP_DL_INSIDE, the test s + m + w <= b_{doc+1}; dk[x] = the document or DL_NONE.
//   2. one of three reductions per pattern, chosen by the host from the reported count c and ndocs -- all give identical arrays:
//      k_dl_wave   c <= 64: one wave per pattern, one lane per occurrence; rank and frequency from all pairs (__shfl / ballot).
//      k_dl_table  one workgroup per pattern: ndocs 32-bit counters in LDS, c LDS atomic adds, a block scan over the counters that
//                  are not zero.  Instantiated for 1024 / 4096 / 16384 counters (4 / 16 / 64 KiB of the CU's 160 KiB).
//      sort        keys (pattern in chunk, doc) through radix_sort_pairs, heads flagged and compacted, frequencies from the distance
//                  of the heads (k_dl_keys, k_dl_heads, k_dl_spans, k_dl_emit).
//      Each writes the pairs of pattern j from ub[j] on, the start of the pattern's upper-bound slice of min(c_j, ndocs) slots, and
//      the number of pairs into ne[j].
//   3. an exclusive sum of ne and k_dl_pack: the slices move, tight and in pattern order, to the results.
// Bounds: a document is used only when it is < ndocs, a counter only inside the table, an output slot only inside the pattern's
// upper-bound slice, a result slot only below `cap`, whatever the arrays hold (cf. the rule at the top of runindex.h).
#pragma once
#include "runindex.h"
#include "docarray.h"

namespace pfp {

constexpr uint32_t DL_NONE = 0xFFFFFFFFu;          // no document: an occurrence that does not count (ndocs < 2^32, so no document has it)
constexpr uint32_t DL_WAVE_MAX = 64;               // most occurrences of the wave route: one lane each
constexpr uint32_t DL_TABLE_CAP = 16384;           // most documents of the table route: 64 KiB of counters
constexpr uint64_t DL_TABLE_ROWS_MAX = 0xFFFFFFFFULL;      // most occurrences of the table route (32-bit counters)
// the counter of k_dl_map (occurrences that do not count): the second block of a call's counters, behind RiOut of its search and walk
constexpr int DL_OUT = OUT_BLOCK;
enum DlOut { DL_OUTSIDE, DL_OUT_COUNT_ };
static_assert(DL_OUT_COUNT_ <= OUT_BLOCK, "the counters of k_dl_map fit one block");

// One lane per position x of the chunk (a persistent grid: every workgroup loads the table once): pattern j = the owner of x in
// obase, m = its length.  out[DL_OUTSIDE] += occurrences that do not count.
template <typename T, uint32_t TAB>
__global__ __launch_bounds__(BLOCK) void k_dl_map(const T *pos, uint64_t total, const ms_u64 *obase, uint64_t np, const uint64_t *off, const T *starts, uint32_t ndocs, uint32_t shift, uint32_t ntab, uint32_t top,
                                                uint64_t n, uint32_t w, int inside, uint32_t *dk, ms_u64 *out)
{
    __shared__ T tab[TAB];
    for (uint32_t j = threadIdx.x; j < ntab && j < TAB; j += BLOCK) tab[j] = starts[(uint64_t)j << shift];
    __syncthreads();
    const uint32_t gtop = shift ? 1u << (shift - 1) : 0u, nt = ntab < TAB ? ntab : TAB;
    const uint64_t stride = (uint64_t)gridDim.x * BLOCK, rounds = (total + stride - 1) / stride;
    ms_u64 dropped = 0;
    for (uint64_t it = 0; it < rounds; ++it) {
        const uint64_t x = it * stride + (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
        if (x >= total) continue;
        const uint64_t s = pos[x];
        uint32_t k = 0;
        for (uint32_t st = top; st; st >>= 1) if (k + st < nt && (uint64_t)tab[k + st] <= s) k += st;
        uint64_t g = (uint64_t)k << shift;                                 // two-level: starts[g] <= s < starts[g + 2^shift]
        for (uint32_t st = gtop; st; st >>= 1) if (g + st < ndocs && (uint64_t)starts[g + st] <= s) g += st;
        bool counts = g < ndocs;
        if (counts && inside) {
            const uint64_t j = ri_owner(obase, np, x), m = off[j + 1] - off[j];
            const uint64_t end = g + 1 < ndocs ? (uint64_t)starts[g + 1] : n;
            counts = s + m + w <= end;
        }
        dk[x] = counts ? (uint32_t)g : DL_NONE;
        dropped += !counts;
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) dropped += __shfl_xor(dropped, d);
    if ((threadIdx.x & 63) == 0 && dropped) atomicAdd(&out[DL_OUTSIDE], dropped);
}

// One wave per pattern list[q] (c <= 64 occurrences): lane l holds the document of occurrence l.  For every lane i whose document is
// the first of its value, the ballot of the lanes that hold the same value gives the frequency; a lane's rank is the number of such
// values below its own.
__global__ __launch_bounds__(BLOCK) void k_dl_wave(const uint32_t *dk, const ms_u64 *obase, const ms_u64 *ub, const uint32_t *list, uint64_t nlist, uint32_t ndocs, uint32_t *tdoc, uint32_t *tfreq, ms_u64 *ne)
{
    const uint64_t q = (uint64_t)blockIdx.x * (BLOCK / WAVE) + (threadIdx.x >> 6);
    if (q >= nlist) return;                                                // (the whole wave)
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t j = list[q], ob = obase[j];
    uint64_t c = obase[j + 1] - ob; if (c > DL_WAVE_MAX) c = DL_WAVE_MAX;
    const uint64_t u0 = ub[j], ulen = ub[j + 1] - u0;
    const uint32_t d = lane < c ? dk[ob + lane] : DL_NONE;
    const bool valid = d < ndocs;
    uint32_t rank = 0, freq = 0, distinct = 0;
    for (uint32_t i = 0; i < (uint32_t)c; ++i) {
        const uint32_t di = __shfl(d, (int)i);
        const unsigned long long same = __ballot(valid && d == di);
        if (di >= ndocs || (uint32_t)(__ffsll((long long)same) - 1) != i) continue;      // (uniform: not a document, or not the first lane with it)
        ++distinct;
        if (valid && di < d) ++rank;
        if (lane == i) freq = (uint32_t)__popcll(same);
    }
    if (freq && rank < ulen) { tdoc[u0 + rank] = d; tfreq[u0 + rank] = freq; }
    if (lane == 0) ne[j] = distinct < ulen ? distinct : ulen;
}

// One workgroup per pattern list[q]: counters tab[0 .. ndocs) in LDS, one atomic add per occurrence, then the counters that are not
// zero in ascending order, a tile of BLOCK counters per block scan.
template <uint32_t TAB>
__global__ __launch_bounds__(BLOCK) void k_dl_table(const uint32_t *dk, const ms_u64 *obase, const ms_u64 *ub, const uint32_t *list, uint32_t ndocs, uint32_t *tdoc, uint32_t *tfreq, ms_u64 *ne)
{
    __shared__ uint32_t tab[TAB];
    __shared__ uint32_t red[4];
    const uint64_t j = list[blockIdx.x], ob = obase[j], c = obase[j + 1] - ob, u0 = ub[j], ulen = ub[j + 1] - u0;
    const uint32_t nd = ndocs < TAB ? ndocs : TAB;
    for (uint32_t k = threadIdx.x; k < nd; k += BLOCK) tab[k] = 0;
    __syncthreads();
    for (uint64_t x = threadIdx.x; x < c; x += BLOCK) { const uint32_t d = dk[ob + x]; if (d < nd) atomicAdd(&tab[d], 1u); }
    __syncthreads();
    uint32_t done = 0;
    for (uint32_t b = 0; b < nd; b += BLOCK) {                             // (uniform)
        const uint32_t k = b + threadIdx.x, f = k < nd ? tab[k] : 0u;
        uint32_t tot;
        const uint32_t at = done + block_excl_sum<uint32_t>(f ? 1u : 0u, red, &tot);
        if (f && at < ulen) { tdoc[u0 + at] = k; tfreq[u0 + at] = f; }
        done += tot;
    }
    if (threadIdx.x == 0) ne[j] = done < ulen ? done : ulen;
}

// ---- the sort route ----
// key[x] = (pattern in chunk << dbits) | doc for the occurrences of the patterns with route[j] == 3 that count, else the key of no
// pattern (np << dbits): those sort behind every pattern
__global__ __launch_bounds__(BLOCK) void k_dl_keys(const uint32_t *dk, uint64_t total, const ms_u64 *obase, uint64_t np, const uint8_t *route, uint32_t ndocs, int dbits, uint64_t *key, uint32_t *val)
{
    const uint64_t x = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (x >= total) return;
    const uint64_t j = ri_owner(obase, np, x);
    const uint32_t d = dk[x];
    key[x] = route[j] == 3 && d < ndocs ? (j << dbits) | d : np << dbits;
    val[x] = (uint32_t)x;
}
__global__ __launch_bounds__(BLOCK) void k_dl_heads(const uint64_t *key, uint64_t total, uint32_t *head)
{
    const uint64_t x = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (x < total) head[x] = !x || key[x] != key[x - 1];
}
// head q (the hl[q]-th sorted key) of pattern j: the first one of j notes q in first[j], the last one q + 1 in last[j]
__global__ __launch_bounds__(BLOCK) void k_dl_spans(const uint64_t *key, const uint32_t *hl, uint64_t nh, uint64_t total, uint64_t np, int dbits, uint32_t *first, uint32_t *last)
{
    const uint64_t q = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= nh) return;
    const uint64_t at = hl[q];
    if (at >= total) return;
    const uint64_t j = key[at] >> dbits;
    if (j >= np) return;
    const uint64_t before = q ? hl[q - 1] : 0, behind = q + 1 < nh ? hl[q + 1] : 0;
    if (!q || before >= total || (key[before] >> dbits) != j) first[j] = (uint32_t)q;
    if (q + 1 == nh || behind >= total || (key[behind] >> dbits) != j) last[j] = (uint32_t)(q + 1);
}
__global__ __launch_bounds__(BLOCK) void k_dl_emit(const uint64_t *key, const uint32_t *hl, uint64_t nh, uint64_t total, uint64_t np, int dbits, uint32_t ndocs, const uint32_t *first, const uint32_t *last, const ms_u64 *ub,
                                                 uint32_t *tdoc, uint32_t *tfreq, ms_u64 *ne)
{
    const uint64_t q = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= nh) return;
    const uint64_t at = hl[q];
    if (at >= total) return;
    const uint64_t j = key[at] >> dbits, d = key[at] & ((1ULL << dbits) - 1);
    if (j >= np || d >= ndocs) return;
    uint64_t end = q + 1 < nh ? hl[q + 1] : total; if (end > total || end <= at) end = at + 1;
    const uint64_t f = first[j], l = last[j], u0 = ub[j], ulen = ub[j + 1] - u0;
    if (q < f || q >= l) return;                                           // (inconsistent arrays only)
    const uint64_t rank = q - f;
    if (rank < ulen) { tdoc[u0 + rank] = (uint32_t)d; tfreq[u0 + rank] = (uint32_t)(end - at); }
    if (q == f) ne[j] = l - f < ulen ? l - f : ulen;
}

// One lane per slot y of the upper-bound slices: slot r of pattern j moves to e0 + eoff[j] + r of the results when r < ne[j]
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_dl_pack(const uint32_t *tdoc, const uint32_t *tfreq, const ms_u64 *ub, const ms_u64 *eoff, uint64_t np, uint64_t slots, uint64_t e0, uint64_t cap, T *doc, T *freq)
{
    const uint64_t y = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (y >= slots) return;
    const uint64_t j = ri_owner(ub, np, y), r = y - ub[j];
    if (r >= eoff[j + 1] - eoff[j]) return;
    const uint64_t at = e0 + eoff[j] + r;
    if (at < cap) { doc[at] = (T)tdoc[y]; freq[at] = (T)tfreq[y]; }
}

} // namespace pfp
