// pfbwt-f_amd/csrc/mems.h -- maximal exact matches on the device (pfp_mem_find, include/pfbwt_hip.h): the MEMs of
// the patterns of the last pfp_ms_query, read off its matching statistics, and -- with locate -- their occurrences through the count /
// locate index (runindex.h).
//
// Position x of the patterns starts a MEM iff len[x] >= L (L = max(min_len, 1)) and (x == 0 or len[x - 1] <= len[x]); its length is
// len[x] and ptr[x] is one occurrence.  The last base of a pattern has len <= 1, so the comparison holds at every pattern start
// whose len is >= 1 and only the global position 0 needs the guard.
//   1. k_mem_flags: one lane per base, the rule into a flag array; an exclusive sum (prims.h) numbers the MEMs, its total comes
//      back to the host (the one round trip of the call).  k_mem_offsets reads the sum at every pattern start: the MEMs in front of
//      every pattern.  k_mem_list: a capped grid striding over the bases, a flagged base finds its pattern by bisection of the
//      offsets and writes start / len / ptr.
//   2. k_mem_search: one lane per MEM, the MEMs in order of decreasing length (k_mem_keys + a radix sort by length, prims.h).  The
//      step is ri_search_steps of runindex.h -- row interval and toehold -- and byte i of MEM k is X[ptr[k] + i] on the resident
//      text: no pattern is kept or uploaded.
//   3. k_ri_pieces, k_ri_walk and k_ri_rows (runindex.h) run as they are on lo / cnt / top of the MEMs: their "pattern" is the MEM.
// Bounds: len[x - 1] is read only for x >= 1; the list index of a flagged base is < mems (the sum of the same flags); a pattern
// index comes from a bisection inside [0, np); MemText cuts every MEM to the text, ptr + i < n, whatever the arrays hold.
#pragma once
#include "runindex.h"

namespace pfp {

constexpr int MEM_LIST_WG = 256 * 8;             // workgroups of k_mem_list at most
// the counters of k_mem_list (sum of the lengths, largest length): the second block of a call's counters, behind RiOut of its locate
constexpr int MEM_OUT = OUT_BLOCK;
enum MemOut { MEM_SUM_LEN, MEM_MAX_LEN, MEM_OUT_COUNT_ };
static_assert(MEM_OUT_COUNT_ <= OUT_BLOCK, "the counters of k_mem_list fit one block");

// does position x start a MEM of at least L bases (L >= 1)
template <typename T>
__device__ __forceinline__ bool mem_starts(const T *len, uint64_t x, uint64_t L)
{
    const uint64_t l = len[x];
    return l >= L && (x == 0 || (uint64_t)len[x - 1] <= l);
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void k_mem_flags(const T *len, uint64_t total, uint64_t L, T *fl)
{
    const uint64_t x = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (x < total) fl[x] = mem_starts<T>(len, x, L) ? (T)1 : (T)0;
}

// moff[j] = MEMs in front of pattern j (idx = the exclusive sum of the flags), moff[np] = all of them; an empty pattern at the
// end of the batch starts at `total`
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_mem_offsets(const T *idx, const uint64_t *off, uint64_t np, uint64_t total, uint64_t mems, ms_u64 *moff)
{
    const uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j > np) return;
    const uint64_t x = off[j];
    moff[j] = j < np && x < total ? (ms_u64)idx[x] : (ms_u64)mems;
}

// The k-th MEM (k = idx[x]) starts at x.  start[k] = x - the start of its pattern, len / ptr: copies of the statistics.  The grid is
// capped (MEM_LIST_WG workgroups) and strides over the bases, so that the two counters take one atomic per wave of the grid and not
// one per 64 bases: every one of them lands on the same address.  out: its own block (MemOut)
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_mem_list(const T *mlen, const T *mptr, const T *idx, const uint64_t *off, uint64_t np, uint64_t total, uint64_t L, uint64_t mems, T *start, T *len, T *ptr, ms_u64 *out)
{
    ms_u64 s = 0, mx = 0;
    for (uint64_t x = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; x < total; x += (uint64_t)gridDim.x * BLOCK) {
        if (!mem_starts<T>(mlen, x, L)) continue;
        const uint64_t k = idx[x];
        uint64_t lo = 0, hi = np;                                          // the last pattern that starts at or in front of x
        while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (off[mid] <= x) lo = mid; else hi = mid; }
        if (k < mems) { const ms_u64 l = mlen[x]; start[k] = (T)(x - off[lo]); len[k] = (T)l; ptr[k] = mptr[x]; s += l; mx = l > mx ? l : mx; }
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) { s += __shfl_xor(s, d); const ms_u64 y = __shfl_xor(mx, d); mx = y > mx ? y : mx; }
    if ((threadIdx.x & 63) == 0 && s) { atomicAdd(&out[MEM_SUM_LEN], s); atomicMax(&out[MEM_MAX_LEN], mx); }
}

// sort keys: the longest MEM first (top >= every length), the MEM's index as the value
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_mem_keys(const T *len, uint64_t mems, uint64_t top, T *key, uint32_t *val)
{
    const uint64_t k = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= mems) return;
    const uint64_t l = len[k];
    key[k] = (T)(l < top ? top - l : 0); val[k] = (uint32_t)k;
}

// The byte source of a search over MEMs (cf. RiPatterns, runindex.h): MEM k is X[ptr[k] .. ptr[k] + len[k]), cut to the text
template <typename T> struct MemText {
    const uint8_t *X; const T *ptr, *len; uint64_t n;
    __device__ __forceinline__ void span(uint64_t k, uint64_t *x0, uint64_t *m) const
    {
        const uint64_t p = ptr[k], l = len[k];
        *x0 = p < n ? p : n; *m = p < n ? (l < n - p ? l : n - p) : 0;
    }
    __device__ __forceinline__ uint32_t byte(uint64_t x) const { return X[x]; }
};

// One lane per MEM: lane g takes MEM order[g].  lo / cnt / top as k_ri_search<T, true>
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_mem_search(MsView<T> ix, MemText<T> src, const uint32_t *order, uint64_t mems, T *lo_out, T *cnt_out, T *top_out, ms_u64 *out)
{
    const uint64_t g = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    ms_u64 nfound = 0, nsteps = 0, cnt = 0;
    if (g < mems) {
        uint64_t k = order[g]; if (k >= mems) k = mems - 1;
        uint64_t lo, top;
        cnt = ri_search_steps<T, true>(ix, src, k, &lo, &top, &nsteps);
        lo_out[k] = (T)lo; cnt_out[k] = (T)cnt; top_out[k] = (T)top;
        nfound = cnt != 0;
    }
    ri_wave_sums(nfound, nsteps, cnt, cnt, out);
}

} // namespace pfp
