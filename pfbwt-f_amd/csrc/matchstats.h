// pfbwt-f_amd/csrc/matchstats.h -- matching-statistics queries on the device (pfp_ms_index / pfp_ms_query, include/pfbwt_hip.h; DESIGN.md
// section 2).
//
// The index is the run-length BWT seen through its run samples: run k covers the rows [ssa[2k], esa[2k]], has the head byte
// head[k] and the threshold row thr[k]; the suffixes of its first and last row are ssa[2k + 1] and esa[2k + 1].
//   1. k_thr_heads + a stable 8-bit radix sort (prims.h) put the runs of one symbol next to each other, in row order: `sorted`.
//      k_ms_sorted writes the run lengths in that order and the 257 borders of the symbols' segments (`sym`); an exclusive sum of the
//      lengths is LF of every run's first row, LF(i) = lfhead[k] + (i - ssa[2k]) for a row i of run k.
//   2. k_ms_runs brings head / lfhead / thr into run order (k_thr_inverse) and, with a max-scan, fills the run DIRECTORY: dir[b] =
//      the run that holds row b << B.  The run of a row is then a bisection of ssa between two neighbouring directory entries (about one run per block
//      for B = floor(log2((n + 1) / r))), not over all r starts.
// A query walks every pattern right to left (Bannai, Gagie, I 2020; Rossi et al. 2022):
//   3. k_ms_pointers: one lane per pattern, the patterns in order of decreasing length so that the lanes of a wave finish together.
//      A step is a chain of dependent reads (directory, run starts, head, and on a mismatch the neighbouring runs of the symbol and
//      a threshold); nothing but the number of patterns in flight hides their latency.  It also marks the BREAKS: position i with
//      i == 0 or ptr[i] != ptr[i - 1] + 1.  Between two breaks the alignment of pattern and text does not change.
//   4. k_ms_breaks: one lane per break compares P[b ..] with T[ptr[b] ..] on the resident text, 16 bytes per step; a comparison
//      longer than `cap` bytes is queued (one atomic per wave, lcp_queue_slot) for k_ms_long, one WAVE per break (cf. k_lcp_long).
//   5. an inclusive max-scan of the break positions (prims.h) gives every position its last break b; k_ms_fill: len[i] = len[b] -
//      (i - b).
// Bounds: a row is used only when it is < n + 1 and a run only when it is < r, whatever the arrays hold; a comparison reads 16
// bytes at offsets <= lim, lim <= the bytes left in the pattern and in the text: the pattern buffer has MS_PAD bytes of slack, the
// text 4 KiB.
#pragma once
#include "thresholds.h"

namespace pfp {

constexpr uint32_t MS_LONG_MIN = 512;           // bytes one lane compares on its own before the break is queued for a wave
constexpr int MS_DIR_LOG2_MAX = 48;
constexpr int MS_LONG_WG = 256 * 8;             // workgroups of k_ms_long at most (4 waves each)
constexpr int MS_LONG_UNROLL = 4;               // 16-byte loads per lane and side in flight in k_ms_long from the third step on
constexpr int MS_LONG_NARROW = 2;               // its first steps read one load per lane
constexpr size_t MS_PAD = 64;                   // bytes behind the patterns on the device

typedef unsigned long long ms_u64;

// The counters a query's kernels fill (`out`, zeroed by the host) come in blocks of OUT_BLOCK values: the first block belongs to the
// search and what follows it -- MsOut here, RiOut for the searches of runindex.h --, a second one at OUT_BLOCK to the kernels a query
// adds behind them (mems.h: MEM_OUT, doclist.h: DL_OUT).
constexpr int OUT_BLOCK = 8;
// steps by kind, queue entries asked for (= breaks handed to a wave), largest length
enum MsOut { MS_MATCH, MS_UP, MS_DOWN, MS_ABSENT, MS_LONG_BREAKS, MS_MAX_LEN, MS_OUT_COUNT_ };
static_assert(MS_OUT_COUNT_ <= OUT_BLOCK, "the counters of pfp_ms_query fit one block");

// the index as the kernels see it
template <typename T> struct MsView {
    const T *ssa, *esa, *thr, *lfhead; const uint8_t *head; const uint32_t *sorted, *sym, *dir;
    uint32_t B; uint64_t r, n;
};
struct alignas(8) MsLong { uint64_t x, lim; };          // the break at position x of the patterns, lim bytes to compare at most

// i-th run in the order of the head bytes: its length, its index, the borders of the symbols' segments; bad: runs whose head is
// the EndOfWord byte
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_ms_sorted(const uint32_t *skey, const uint32_t *sval, const T *ssa, uint64_t r, uint64_t rows, T *len, uint32_t *sorted, uint32_t *sym, ms_u64 *bad)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= r) return;
    const uint64_t k = sval[i];
    const uint32_t c = skey[i] & 255u;
    const uint64_t s = ssa[2 * k], e1 = k + 1 < r ? (uint64_t)ssa[2 * (k + 1)] : rows;
    len[i] = (T)(e1 - s);
    sorted[i] = (uint32_t)k;
    if (c == EndOfWord) atomicAdd(bad, 1ULL);
    for (uint32_t x = i ? (skey[i - 1] & 255u) + 1 : 0u; x <= c; ++x) sym[x] = (uint32_t)i;          // (nothing when the run before has the same head)
    if (i + 1 == r) for (uint32_t x = c + 1; x <= 256; ++x) sym[x] = (uint32_t)r;
}
// run k: head byte, LF of its first row, threshold row; the directory entry of the FIRST block whose first row it holds (dir starts
// as zeros; run indices ascend with the rows, so an inclusive max-scan of dir[0 .. nblk) then gives every block its run -- one
// thread never walks the blocks of a long run, 10 M of them for the N run of a chromosome); the last run also writes the closing
// entry dir[nblk]
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_ms_runs(const uint32_t *pos, const uint32_t *skey, const T *lfs, const T *thr, const T *ssa, uint64_t r, uint64_t rows, uint32_t B, uint64_t nblk,
                                                 uint8_t *head, T *lfhead, T *thrrow, uint32_t *dir)
{
    const uint64_t k = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= r) return;
    const uint32_t i = pos[k];
    head[k] = (uint8_t)skey[i]; lfhead[k] = lfs[i];
    if (thr) thrrow[k] = thr[2 * k + 1];                                   // (null: an index without thresholds, runindex.h)
    const uint64_t s = ssa[2 * k], e1 = k + 1 < r ? (uint64_t)ssa[2 * (k + 1)] : rows;
    const uint64_t b = (s + (1ULL << B) - 1) >> B;
    if (b < nblk && (b << B) < e1) dir[b] = (uint32_t)k;
    if (k + 1 == r) dir[nblk] = (uint32_t)k;
}

// the run that holds `row` (< n + 1)
template <typename T>
__device__ __forceinline__ uint64_t ms_run_of(const MsView<T> &ix, uint64_t row)
{
    const uint64_t b = row >> ix.B;
    uint64_t lo = ix.dir[b], hi = ix.dir[b + 1];                           // the last run that starts at or in front of row lies in [lo, hi]
    if (hi >= ix.r) hi = ix.r - 1;                                         // (inconsistent samples only)
    if (lo > hi) lo = hi;
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if ((uint64_t)ix.ssa[2 * mid] <= row) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// toupper + optional non-ACGT->A of the patterns, 16 bytes per thread (norm_base, parse.h: what the feed does to the text)
__global__ __launch_bounds__(BLOCK) void k_ms_norm(uint8_t *P, uint64_t total, int ntoa)
{
    const uint64_t x0 = ((uint64_t)blockIdx.x * BLOCK + threadIdx.x) * 16;
    for (uint64_t x = x0; x < x0 + 16 && x < total; ++x) P[x] = (uint8_t)norm_base(P[x], ntoa != 0);
}

__device__ __forceinline__ void ms_wave_steps(ms_u64 nm, ms_u64 nu, ms_u64 nd, ms_u64 na, ms_u64 *out)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) { nm += __shfl_xor(nm, d); nu += __shfl_xor(nu, d); nd += __shfl_xor(nd, d); na += __shfl_xor(na, d); }
    if ((threadIdx.x & 63) == 0) {
        if (nm) atomicAdd(&out[MS_MATCH], nm);
        if (nu) atomicAdd(&out[MS_UP], nu);
        if (nd) atomicAdd(&out[MS_DOWN], nd);
        if (na) atomicAdd(&out[MS_ABSENT], na);
    }
}
__device__ __forceinline__ void ms_wave_max(ms_u64 mx, ms_u64 *out)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) { const ms_u64 y = __shfl_xor(mx, d); mx = y > mx ? y : mx; }
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(&out[MS_MAX_LEN], mx);
}

// One lane per pattern: lane g takes pattern order[g] (P[off[j] .. off[j + 1])) from its last byte to its first, from row 0 and
// text position n.  ptr[x]: the pointer of position x of the patterns; bp[x] = x when x is a break, else 0 (position 0 is one).
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_ms_pointers(MsView<T> ix, const uint8_t *P, const uint64_t *off, const uint32_t *order, uint64_t np, T *ptr, T *bp, ms_u64 *out)
{
    const uint64_t g = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    ms_u64 nm = 0, nu = 0, nd = 0, na = 0;
    if (g < np) {
        const uint64_t j = order[g], x0 = off[j], m = off[j + 1] - x0;
        uint64_t row = 0, pos = ix.n, next = 0;                            // next: the pointer of position i + 1
        for (uint64_t i = m; i-- > 0;) {
            const uint32_t c = P[x0 + i];
            const uint32_t f = ix.sym[c], l = ix.sym[c + 1];               // the runs of c in `sorted`
            uint64_t p;
            if (f == l) { p = ix.n; row = 0; pos = ix.n; ++na; }
            else {
                uint64_t k = ms_run_of<T>(ix, row);
                if (ix.head[k] == c) ++nm;
                else {
                    uint32_t lo = f, hi = l;                               // first run of c behind k
                    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((uint64_t)ix.sorted[mid] > k) hi = mid; else lo = mid + 1; }
                    const uint64_t kn = lo < l ? ix.sorted[lo] : 0;
                    if (lo < l && (lo == f || row >= (uint64_t)ix.thr[kn])) { ++nd; k = kn; row = ix.ssa[2 * k]; pos = ix.ssa[2 * k + 1]; }
                    else { ++nu; k = ix.sorted[lo - 1]; row = ix.esa[2 * k]; pos = ix.esa[2 * k + 1]; }
                }
                row = (uint64_t)ix.lfhead[k] + (row - (uint64_t)ix.ssa[2 * k]);
                if (row > ix.n) row = 0;                                   // (inconsistent samples only)
                pos -= 1; p = pos;
            }
            ptr[x0 + i] = (T)p;
            if (i + 1 < m) bp[x0 + i + 1] = next != p + 1 ? (T)(x0 + i + 1) : (T)0;
            next = p;
        }
        if (m) bp[x0] = (T)x0;
    }
    ms_wave_steps(nm, nu, nd, na, out);
}

// fl[x] = 1 when x is a break; after the exclusive sum idx of fl: list[idx[x]] = x
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_ms_break_flags(const T *bp, uint64_t total, T *fl)
{
    const uint64_t x = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (x < total) fl[x] = (uint64_t)bp[x] == x ? (T)1 : (T)0;
}
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_ms_break_list(const T *bp, const T *idx, uint64_t total, T *list)
{
    const uint64_t x = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (x < total && (uint64_t)bp[x] == x) list[idx[x]] = (T)x;
}

// One lane: common prefix of a[0 .. lim) and b[0 .. lim).  Returns true when the value is final (*h_out = it); false: the first
// *h_out > cap bytes are equal and *h_out < lim.
__device__ __forceinline__ bool ms_walk(const uint8_t *a, const uint8_t *b, uint64_t lim, uint64_t cap, uint64_t *h_out)
{
    uint64_t h = 0;
    while (h <= cap && h < lim) {
        const uint32_t d = lcp_first_diff(lcp_ld16(a + h), lcp_ld16(b + h));
        if (d < 16) { h += d; *h_out = h < lim ? h : lim; return true; }
        h += 16;
    }
    if (h >= lim) { *h_out = lim; return true; }
    *h_out = h;
    return false;
}
// One lane per break: list[q] = its position x.  The pattern of x ends at the first offset above x; lim = the bytes left in the
// pattern and in the text.  A length of at most `cap` is written; a longer one goes to the queue.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_ms_breaks(const uint8_t *X, uint64_t n, const uint8_t *P, const uint64_t *off, uint64_t np, const T *list, uint64_t nbreaks, const T *ptr, uint64_t cap,
                                                   T *len, MsLong *queue, uint64_t qcap, ms_u64 *out)
{
    const uint64_t q = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = q < nbreaks;
    uint64_t x = 0, p = 0, lim = 0, h = 0;
    bool fin = true;
    if (live) {
        x = list[q]; p = ptr[x];
        uint64_t lo = 0, hi = np;                                          // the last pattern that starts at or in front of x
        while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (off[mid] <= x) lo = mid; else hi = mid; }
        const uint64_t pe = off[lo + 1];
        if (pe > x && p <= n) lim = pe - x < n - p ? pe - x : n - p;
        fin = ms_walk(P + x, X + p, lim, cap, &h);
    }
    const bool is_long = live && (!fin || h > cap);
    const uint64_t slot = lcp_queue_slot(is_long, &out[MS_LONG_BREAKS]);
    bool write = live && !is_long;
    if (is_long) {
        if (slot < qcap) { queue[slot].x = x; queue[slot].lim = lim; }
        else { (void)ms_walk(P + x, X + p, lim, ~0ULL >> 1, &h); write = true; }      // queue full: this lane goes on alone
    }
    if (write) len[x] = (T)h;
    ms_wave_max(write ? h : 0, out);
}

// one step of a wave: UN x 64 x 16 bytes of both sides from offset h on (cf. lcp_wave_step, lcparray.h)
template <int UN>
__device__ __forceinline__ bool ms_wave_step(const uint8_t *a, const uint8_t *b, uint64_t h, uint64_t lim, int lane, uint64_t *res)
{
    Lcp16 va[UN], vb[UN];
    bool in[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
        const uint64_t o = h + (uint64_t)(u * WAVE + lane) * 16;
        in[u] = o <= lim;
        if (in[u]) { va[u] = lcp_ld16(a + o); vb[u] = lcp_ld16(b + o); }
    }
    bool found = false;
#pragma unroll
    for (int u = 0; u < UN; ++u) {
        const uint32_t d = in[u] ? lcp_first_diff(va[u], vb[u]) : 0u;
        const unsigned long long m = __ballot(d < 16);
        if (m && !found) {
            const int L = (int)(__ffsll((long long)m) - 1);
            *res = h + (uint64_t)(u * WAVE + L) * 16 + __shfl(d, L);
            found = true;
        }
    }
    return found;
}
// One wave per queued break; the first h0 bytes are known to be equal.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_ms_long(const uint8_t *X, const uint8_t *P, const MsLong *queue, uint64_t qcap, const T *ptr, uint64_t h0, T *len, ms_u64 *out)
{
    const int lane = threadIdx.x & 63;
    const uint64_t asked = out[MS_LONG_BREAKS], cnt = asked < qcap ? asked : qcap;
    const uint64_t nw = (uint64_t)gridDim.x * (BLOCK / WAVE);
    ms_u64 mx = 0;
    for (uint64_t q = (uint64_t)blockIdx.x * (BLOCK / WAVE) + (threadIdx.x >> 6); q < cnt; q += nw) {
        const uint64_t x = queue[q].x, lim = queue[q].lim;
        const uint8_t *a = P + x, *b = X + (uint64_t)ptr[x];
        uint64_t h = h0, res = lim;
        bool found = false;
        for (int k = 0; k < MS_LONG_NARROW && !found; ++k) {               // (trip counts uniform over the wave)
            found = ms_wave_step<1>(a, b, h, lim, lane, &res);
            h += (uint64_t)WAVE * 16;
        }
        while (!found) {
            found = ms_wave_step<MS_LONG_UNROLL>(a, b, h, lim, lane, &res);
            h += (uint64_t)MS_LONG_UNROLL * WAVE * 16;
        }
        if (res > lim) res = lim;
        if (lane == 0) len[x] = (T)res;
        mx = res > mx ? res : mx;
    }
    if (lane == 0 && mx) atomicMax(&out[MS_MAX_LEN], mx);
}

// lastb[x] = the last break at or in front of x: every other position takes its length from there
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_ms_fill(const T *lastb, uint64_t total, T *len)
{
    const uint64_t x = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (x >= total) return;
    const uint64_t b = lastb[x];
    if (b < x) { const uint64_t L = len[b], d = x - b; len[x] = L > d ? (T)(L - d) : (T)0; }
}

} // namespace pfp
