// pfbwt-f_amd/csrc/runindex.h -- count and locate queries on the device (pfp_ri_index / pfp_ri_count / pfp_ri_locate,
// include/pfbwt_hip.h): the r-index of Gagie, Navarro and Prezza (JACM 2020) over the run samples.
//
// The index is the run view of matchstats.h without thresholds (head, lfhead, sorted, sym, the run directory) plus the PHI
// structure: the run starts in the order of their text positions, pq[i] = the i-th position, pv[i] = the SA value of the row in front
// of that run start (the end sample of the run before), and a block directory over text positions like the sparse PLCP's
// (lcparray.h): pdir[b] = pairs with a position < b << PB.  phi(p) = pv[i] + (p - pq[i]) for the last pair with pq[i] <= p.
//   1. k_ri_search: one lane per pattern, the patterns in order of decreasing length (cf. k_ms_pointers).  A step (ri_search_steps,
//      shared with the search over MEMs of mems.h) maps the row
//      interval [lo, hi) through LF of one symbol -- two run lookups and, where a border row does not carry the symbol, a bisection of
//      the symbol's runs -- and, for locate, carries the SA value of row hi - 1 along (the toehold).
//   2. k_ri_pieces: the reported rows of a pattern are cut at run borders; the number of pieces and of reported rows per pattern,
//      two exclusive sums (prims.h) give every pattern its first piece and its first output value.
//   3. k_ri_walk: one lane per piece.  The SA value of the piece's last row is known (the run's end sample, or the toehold); phi
//      gives the row above, and so on down to the piece's first row.  k_ri_rows is the other route: a build that holds the SA
//      copies the reported rows from it.
// Both walks are chains of dependent reads; only patterns / pieces in flight hide their latency.
// Bounds: a row is used only when it is <= n, a run only when it is < r, a text position only when it is <= n, whatever the
// arrays hold; the loop of a piece is bounded by its row count and its output index lies inside the pattern's reported rows.
#pragma once
#include "matchstats.h"

namespace pfp {

constexpr int RI_DIR_LOG2_MAX = 48;

// the phi structure as the kernels see it
template <typename T> struct RiPhi { const T *pq, *pv; const uint32_t *dir; uint32_t B; uint64_t r, n; };

// pq[i] / pv[i] = the i-th run-start position and the end sample of the run in front of that run (run 0, the row of the
// terminator's suffix n, has none: n).  The directory starts as zeros: the LAST pair of every block b writes its count i + 1 into
// dir[b + 1], and an inclusive max-scan of dir[0 .. nblk + 2) then gives every entry the pairs in front of its block (cf.
// k_ms_runs: no thread walks the blocks of a long gap, 10 M of them behind the N run of a chromosome).
// bad: positions that do not strictly ascend, lie above n, or a first position that is not 0.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_ri_phi_fill(const uint64_t *skey, const uint32_t *sval, const T *esa, uint64_t r, uint64_t n, uint32_t B, uint64_t nblk, T *pq, T *pv, uint32_t *dir, ms_u64 *bad)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= r) return;
    const uint64_t p = skey[i], k = sval[i];
    pq[i] = (T)p; pv[i] = k ? esa[2 * (k - 1) + 1] : (T)n;
    const bool wrong = p > n || (i ? skey[i - 1] >= p : p != 0);
    if (wrong) { atomicAdd(bad, 1ULL); return; }                           // (the directory is not used then)
    const uint64_t b = p >> B;                                             // <= nblk
    if (i + 1 == r || (skey[i + 1] >> B) != b) dir[b + 1] = (uint32_t)(i + 1);
}

// SA of the row above the row whose SA is p (p <= n)
template <typename T>
__device__ __forceinline__ uint64_t ri_phi(const RiPhi<T> &ph, uint64_t p)
{
    const uint64_t b = p >> ph.B;
    uint64_t lo = ph.dir[b], hi = ph.dir[b + 1];
    if (hi > ph.r) hi = ph.r;                                              // (inconsistent samples only)
    if (lo > hi) lo = hi;
    while (lo < hi) {                                                      // first pair of the block with a position > p
        const uint64_t mid = (lo + hi) >> 1;
        if ((uint64_t)ph.pq[mid] <= p) lo = mid + 1; else hi = mid;
    }
    if (!lo) return p;                                                     // (position 0 starts a run: inconsistent samples only)
    const uint64_t q = (uint64_t)ph.pv[lo - 1] + (p - (uint64_t)ph.pq[lo - 1]);
    return q <= ph.n ? q : ph.n;
}

// LF of symbol c (runs sorted[f .. l)) for a row <= n of run k: *idx = the place in `sorted` of the first run of c behind k when
// the row does not carry c (l: none)
template <typename T>
__device__ __forceinline__ uint64_t ri_lf(const MsView<T> &ix, uint32_t c, uint32_t f, uint32_t l, uint64_t row, uint64_t k, bool *hit, uint32_t *idx)
{
    *hit = ix.head[k] == c;
    if (*hit) { const uint64_t s = ix.ssa[2 * k]; *idx = f; return (uint64_t)ix.lfhead[k] + (row >= s ? row - s : 0); }
    uint32_t lo = f, hi = l;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((uint64_t)ix.sorted[mid] > k) hi = mid; else lo = mid + 1; }
    *idx = lo;
    if ((uint64_t)lo >= ix.r) return ix.n + 1;                             // behind the last symbol's segment
    uint64_t kk = ix.sorted[lo];                                           // (lo == l: the first run of the next symbol that has runs)
    if (kk >= ix.r) kk = ix.r - 1;
    return ix.lfhead[kk];
}

// the counters of a search (found patterns, steps, sum of the counts, largest count) and of k_ri_walk (pieces, phi steps, longest
// piece): the first block of `out` (matchstats.h: OUT_BLOCK)
enum RiOut { RI_FOUND, RI_STEPS, RI_OCCURRENCES, RI_MAX_COUNT, RI_LIVE, RI_PHI_STEPS, RI_MAX_PIECE, RI_OUT_COUNT_ };
static_assert(RI_OUT_COUNT_ <= OUT_BLOCK, "the counters of a search and a walk fit one block");
__device__ __forceinline__ void ri_wave_sums(ms_u64 a, ms_u64 b, ms_u64 s, ms_u64 mx, ms_u64 *out)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) { a += __shfl_xor(a, d); b += __shfl_xor(b, d); s += __shfl_xor(s, d); const ms_u64 y = __shfl_xor(mx, d); mx = y > mx ? y : mx; }
    if ((threadIdx.x & 63) == 0) {
        if (a) atomicAdd(&out[RI_FOUND], a);
        if (b) atomicAdd(&out[RI_STEPS], b);
        if (s) atomicAdd(&out[RI_OCCURRENCES], s);
        if (mx) atomicMax(&out[RI_MAX_COUNT], mx);
    }
}

// The byte source of a search over uploaded patterns: pattern j is P[off[j] .. off[j + 1]).  A source names the bytes of string j by
// a first index x0 and a length m (span) and hands out the byte at an index (byte); mems.h has the one that reads the text.
struct RiPatterns {
    const uint8_t *P; const uint64_t *off;
    __device__ __forceinline__ void span(uint64_t j, uint64_t *x0, uint64_t *m) const { *x0 = off[j]; *m = off[j + 1] - *x0; }
    __device__ __forceinline__ uint32_t byte(uint64_t x) const { return P[x]; }
};

// String j of `src` from its last byte to its first.  Returns cnt and *lo: the interval of rows whose suffix starts with the string
// (cnt 0: lo is 0); LOCATE: *top = SA of row lo + cnt - 1.  *nsteps: the steps taken.
template <typename T, bool LOCATE, typename SRC>
__device__ __forceinline__ uint64_t ri_search_steps(const MsView<T> &ix, const SRC &src, uint64_t j, uint64_t *lo_out, uint64_t *top_out, ms_u64 *nsteps)
{
    uint64_t x0, m;
    src.span(j, &x0, &m);
    uint64_t lo = 0, hi = m ? ix.n + 1 : 0, top = 0;
    if (LOCATE) { top = ix.esa[2 * (ix.r - 1) + 1]; if (top > ix.n) top = ix.n; }
    for (uint64_t i = m; i-- > 0 && lo < hi;) {
        const uint32_t c = src.byte(x0 + i);
        const uint32_t f = ix.sym[c], l = ix.sym[c + 1];                   // the runs of c in `sorted`
        ++*nsteps;
        if (f >= l) { hi = lo; break; }
        bool hit; uint32_t idx;
        const uint64_t t = hi - 1, kl = ms_run_of<T>(ix, lo), kt = ms_run_of<T>(ix, t);
        uint64_t nlo = ri_lf<T>(ix, c, f, l, lo, kl, &hit, &idx);
        uint64_t nhi = ri_lf<T>(ix, c, f, l, t, kt, &hit, &idx);
        if (hit) { ++nhi; if (LOCATE) top = top ? top - 1 : 0; }
        else if (LOCATE && idx > f) {                                      // the last run of c in front of kt
            uint64_t kp = ix.sorted[idx - 1]; if (kp >= ix.r) kp = ix.r - 1;
            const uint64_t e = ix.esa[2 * kp + 1];
            top = e ? e - 1 : 0; if (top > ix.n) top = ix.n;
        }
        if (nhi > ix.n + 1) nhi = ix.n + 1;                                // (inconsistent samples only)
        if (nlo > nhi) nlo = nhi;
        lo = nlo; hi = nhi;
    }
    const uint64_t cnt = hi - lo;
    *lo_out = cnt ? lo : 0; *top_out = top;
    return cnt;
}

// One lane per pattern: lane g takes pattern order[g] (P[off[j] .. off[j + 1])).  lo[j] / cnt[j]: the interval of rows whose suffix
// starts with the pattern (cnt 0: lo is 0); LOCATE: top[j] = SA of row lo + cnt - 1.
template <typename T, bool LOCATE>
__global__ __launch_bounds__(BLOCK) void k_ri_search(MsView<T> ix, const uint8_t *P, const uint64_t *off, const uint32_t *order, uint64_t np, T *lo_out, T *cnt_out, T *top_out, ms_u64 *out)
{
    const uint64_t g = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    ms_u64 nfound = 0, nsteps = 0, cnt = 0;
    if (g < np) {
        const uint64_t j = order[g];
        const RiPatterns src = {P, off};
        uint64_t lo, top;
        cnt = ri_search_steps<T, LOCATE>(ix, src, j, &lo, &top, &nsteps);
        lo_out[j] = (T)lo; cnt_out[j] = (T)cnt;
        if (LOCATE) top_out[j] = (T)top;
        nfound = cnt != 0;
    }
    ri_wave_sums(nfound, nsteps, cnt, cnt, out);
}

// pattern j: rc[j] = its reported rows (all, or the last max_occ), pc[j] = the runs they touch, kfirst[j] = the run of the first one
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_ri_pieces(MsView<T> ix, const T *lo, const T *cnt, uint64_t np, uint64_t max_occ, ms_u64 *pc, ms_u64 *rc, uint32_t *kfirst)
{
    const uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= np) return;
    const uint64_t c = cnt[j];
    uint64_t rep = 0, pieces = 0, k0 = 0;
    if (c) {
        uint64_t hi = (uint64_t)lo[j] + c; if (hi > ix.n + 1) hi = ix.n + 1;
        rep = max_occ && max_occ < c ? max_occ : c; if (rep > hi) rep = hi;
        k0 = ms_run_of<T>(ix, hi - rep);
        const uint64_t k1 = ms_run_of<T>(ix, hi - 1);
        pieces = k1 >= k0 ? k1 - k0 + 1 : 1;
    }
    pc[j] = pieces; rc[j] = rep; kfirst[j] = (uint32_t)k0;
}

// the last pattern whose base is <= x (bases ascend; patterns without entries share their base with the next one)
__device__ __forceinline__ uint64_t ri_owner(const ms_u64 *base, uint64_t np, uint64_t x)
{
    uint64_t lo = 0, hi = np;
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (base[mid] <= x) lo = mid; else hi = mid; }
    return lo;
}

// One lane per piece q: pattern j = the owner of q in pbase, run k = kfirst[j] + (q - pbase[j]); rows [a, b] = the reported rows of j
// inside run k.  SA of row b: the toehold when b is the pattern's last row, else the run's end sample.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_ri_walk(MsView<T> ix, RiPhi<T> ph, const T *lo, const T *cnt, const T *top, const uint32_t *kfirst, const ms_u64 *pbase, const ms_u64 *obase, uint64_t np, uint64_t npieces,
                                                 T *pos, ms_u64 *out)
{
    const uint64_t q = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    ms_u64 live = 0, steps = 0, rows = 0;
    if (q < npieces) {
        const uint64_t j = ri_owner(pbase, np, q);
        const uint64_t k = (uint64_t)kfirst[j] + (q - pbase[j]);
        uint64_t hi = (uint64_t)lo[j] + (uint64_t)cnt[j]; if (hi > ix.n + 1) hi = ix.n + 1;
        const uint64_t ob = obase[j], rep = obase[j + 1] - ob;
        if (k < ix.r && rep && rep <= hi) {
            const uint64_t first = hi - rep, s = ix.ssa[2 * k], e = ix.esa[2 * k];
            const uint64_t a = s > first ? s : first, b = e < hi - 1 ? e : hi - 1;
            if (a <= b) {
                uint64_t p = b == hi - 1 ? (uint64_t)top[j] : (uint64_t)ix.esa[2 * k + 1];
                if (p > ix.n) p = ix.n;
                live = 1; rows = b - a + 1;
                for (uint64_t row = b;; --row) {
                    pos[ob + (row - first)] = (T)p;
                    if (row == a) break;
                    p = ri_phi<T>(ph, p); ++steps;
                }
            }
        }
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) { live += __shfl_xor(live, d); steps += __shfl_xor(steps, d); const ms_u64 y = __shfl_xor(rows, d); rows = y > rows ? y : rows; }
    if ((threadIdx.x & 63) == 0) {
        if (live) atomicAdd(&out[RI_LIVE], live);
        if (steps) atomicAdd(&out[RI_PHI_STEPS], steps);
        if (rows) atomicMax(&out[RI_MAX_PIECE], rows);
    }
}

// The route of a build that holds the SA: one lane per output value x, pos[x] = sa[first reported row of its pattern + (x - obase)]
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_ri_rows(const T *sa, uint64_t n, const T *lo, const T *cnt, const ms_u64 *obase, uint64_t np, uint64_t total, T *pos)
{
    const uint64_t x = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (x >= total) return;
    const uint64_t j = ri_owner(obase, np, x);
    const uint64_t hi = (uint64_t)lo[j] + (uint64_t)cnt[j], rep = obase[j + 1] - obase[j];
    uint64_t row = hi - rep + (x - obase[j]);
    if (hi < rep || row > n) row = n;                                      // (inconsistent arrays only)
    pos[x] = sa[row];
}

} // namespace pfp
