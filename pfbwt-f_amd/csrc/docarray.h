// pfbwt-f_amd/csrc/docarray.h -- document-array post-pass (pfp_doc_array, include/pfbwt_hip.h).
//
// doc(s) = max{k : b_k <= s} over the ascending record starts b_0 = 0 < b_1 < ... (get_n() coordinates, the values of .docs):
// `upper_bound(b, s) - 1`, the "index of the string a suffix starts in" of gsacak's DA, for every value of the device SA (full
// or a slice) or every second value of the .ssa / .esa pairs.  A stream: U bytes in and U bytes out per value.
//   * The grid is persistent (DOC_WG_PER_CU_* workgroups per CU, each walking many 16-byte vectors): every workgroup loads the
//     start table into LDS once, so the table is read grid x table bytes in all, not once per 256 rows.
//   * Table of at most `lds_max` entries (<= DOC_LDS_CAP = 8192: 64 KiB at 8 B): one bisection in LDS.
//   * Larger tables (collections of short records): every 2^shift-th start in LDS, then a bisection over the <= 2^shift entries
//     of that bucket in global memory (the table stays in L2 / the Infinity Cache).
// Bisection without an upper bound per step: k is the largest index with tab[k] <= s after the steps top, top/2, .., 1, where
// top is the largest power of two below the table length (tab[0] = 0 <= s holds for every s).
#pragma once
#include "prims.h"

namespace pfp {

constexpr uint32_t DOC_LDS_CAP = 8192;          // entries of the LDS table (64 KiB of uint64_t)
constexpr uint32_t DOC_LDS_SMALL = 1024;        // the instantiation for tables of up to 1024 entries (8 KiB: 8 workgroups per CU)
constexpr int DOC_WG_PER_CU_SMALL = 8, DOC_WG_PER_CU_BIG = 2;    // 32 waves per CU / LDS: 2 x 64 KiB of 160 KiB

// src / dst: cnt values; the first `head` of them are not 16-byte aligned (dst has the same alignment as src), the vectors start
// at src + head.  PAIRS: (row, value) pairs -- only the odd positions are looked up, the rows are copied.
template <typename T, uint32_t TAB, bool PAIRS>
__global__ __launch_bounds__(BLOCK) void k_doc_lookup(const T *src, T *dst, uint64_t cnt, uint32_t head, const T *starts, uint32_t ndocs, uint32_t shift, uint32_t ntab, uint32_t top)
{
    __shared__ T tab[TAB];
    for (uint32_t j = threadIdx.x; j < ntab; j += BLOCK) tab[j] = starts[(uint64_t)j << shift];
    __syncthreads();
    const uint32_t gtop = shift ? 1u << (shift - 1) : 0u;
    auto doc = [&](T s) -> T {
        uint32_t k = 0;
        for (uint32_t st = top; st; st >>= 1) if (k + st < ntab && tab[k + st] <= s) k += st;
        uint64_t g = (uint64_t)k << shift;                 // two-level: starts[g] <= s < starts[g + 2^shift]
        for (uint32_t st = gtop; st; st >>= 1) if (g + st < ndocs && starts[g + st] <= s) g += st;
        return (T)g;
    };
    constexpr int VW = 16 / sizeof(T);
    const uint64_t nvec = (cnt - head) / VW, tail0 = head + nvec * VW;
    const uint64_t gid = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    // the unaligned head and the tail (fewer than VW values each)
    if (gid < head) { const T x = src[gid]; dst[gid] = (PAIRS && !(gid & 1)) ? x : doc(x); }
    if (gid < cnt - tail0) { const uint64_t i = tail0 + gid; const T x = src[i]; dst[i] = (PAIRS && !(i & 1)) ? x : doc(x); }
    const Vec16<T> *vs = (const Vec16<T> *)(src + head);
    Vec16<T> *vd = (Vec16<T> *)(dst + head);
    const uint64_t stride = (uint64_t)gridDim.x * BLOCK * STREAM_UNROLL;
    for (uint64_t b = (uint64_t)blockIdx.x * BLOCK * STREAM_UNROLL + threadIdx.x; b < nvec; b += stride) {
        Vec16<T> v[STREAM_UNROLL];
#pragma unroll
        for (int u = 0; u < STREAM_UNROLL; ++u) if (b + (uint64_t)u * BLOCK < nvec) v[u] = vs[b + (uint64_t)u * BLOCK];
#pragma unroll
        for (int u = 0; u < STREAM_UNROLL; ++u) {
            const uint64_t q = b + (uint64_t)u * BLOCK;
            if (q >= nvec) break;
#pragma unroll
            for (int e = 0; e < VW; ++e) if (!PAIRS || ((head + q * VW + e) & 1)) v[u].v[e] = doc(v[u].v[e]);
            vd[q] = v[u];
        }
    }
}

} // namespace pfp
