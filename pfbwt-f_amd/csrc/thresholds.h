// pfbwt-f_amd/csrc/thresholds.h -- matching-statistics thresholds post-pass (pfp_thresholds, include/pfbwt_hip.h).
//
// Run k starts at row s = ssa[2k] with the symbol c = BWT[s]; e = the largest row < s with BWT[e] == c (the last row of the run
// of c before it).  Its threshold is the LEFTMOST row j in (e, s] with LCP[j] = min LCP[e+1 .. s] (Bannai, Gagie, I 2020); a run
// without such an e has none (thr = tlcp = 0).  A segmented range-minimum over the LCP rows, keyed by the BWT symbol:
//   1. k_thr_heads + a stable 8-bit radix sort (prims.h) of (head byte, run): the runs of one symbol become neighbours, in row
//      order, whatever the byte values are (no alphabet is assumed).  The sorted predecessor k' of k gives e + 1 = ssa[2(k' + 1)],
//      the start of the run behind k'.
//   2. k_thr_tile_min: (minimum, leftmost row) of every tile of `tile` rows -- one wave per tile, 16-byte loads (the rows have the
//      alignment of the SA modulo 16: up to VW - 1 rows at either end of a tile are read one by one).
//   3. k_thr_queries: one lane per run in sorted order (the gaps of neighbouring lanes follow each other in the rows).  A gap of at
//      most `long_min` rows is scanned by its lane; a longer one is appended to a queue (one atomic per wave, lcp_queue_slot).
//   4. k_thr_long: one WAVE per queued run: the rows up to the first tile border, whole tiles from the tile minima, the rows
//      behind the last border; lanes strided, four loads in flight each.
// Every reduction is over (value, row) with the smaller row winning a tie, so "leftmost" does not depend on the order of visits.
// Work: every row lies in at most one gap per symbol, so all gaps together cover at most sigma * (n + 1) rows (sigma <= 8 here);
// the long route reads fewer than 2 * tile rows plus (s - e) / tile tile entries per run.
// Bounds: a gap is used only when 1 <= e + 1 <= s < rows; every read of lcp is at a row in [e + 1, s], every read of the tile
// arrays at a tile that lies inside the gap.
#pragma once
#include "lcparray.h"

namespace pfp {

constexpr uint32_t THR_LONG_MIN = 128;          // rows one lane scans on its own; a longer gap is queued for a wave
constexpr uint32_t THR_TILE = 1024;             // rows per tile minimum (a power of two >= 16)
constexpr uint64_t THR_QUEUE_CAP = 1u << 27;    // queue entries at most (24 B each; halved until the workspace has room); a run that finds the queue full is finished by its lane
constexpr int THR_LONG_WG = 256 * 8;            // workgroups of k_thr_long / k_thr_tile_min at most (4 waves each)
constexpr int THR_UNROLL = 4;                   // loads per lane in flight

struct alignas(8) ThrLong { uint64_t lo, s, k; };          // rows [lo, s] of run k

typedef unsigned long long thr_u64;
constexpr thr_u64 THR_NONE = ~0ULL;

// (value, row) minimum: the smaller row wins a tie
__device__ __forceinline__ void thr_take(thr_u64 v, thr_u64 row, thr_u64 &bv, thr_u64 &br)
{
    if (v < bv || (v == bv && row < br)) { bv = v; br = row; }
}
__device__ __forceinline__ void thr_wave_min(thr_u64 &bv, thr_u64 &br)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) { const thr_u64 ov = __shfl_xor(bv, d), orow = __shfl_xor(br, d); thr_take(ov, orow, bv, br); }
}
// rows [x0, x1) of lcp by the lanes of a wave, strided (trip count uniform over the wave); lcp[0] is row `row0`
template <typename T>
__device__ __forceinline__ void thr_scan_rows(const T *lcp, uint64_t x0, uint64_t x1, int lane, thr_u64 &bv, thr_u64 &br, uint64_t row0 = 0)
{
    for (uint64_t base = x0; base < x1; base += (uint64_t)THR_UNROLL * WAVE) {
        T v[THR_UNROLL];
#pragma unroll
        for (int u = 0; u < THR_UNROLL; ++u) { const uint64_t row = base + (uint64_t)(u * WAVE + lane); v[u] = row < x1 ? lcp[row - row0] : (T)0; }
#pragma unroll
        for (int u = 0; u < THR_UNROLL; ++u) { const uint64_t row = base + (uint64_t)(u * WAVE + lane); if (row < x1) thr_take(v[u], row, bv, br); }
    }
}

// keys[k] = BWT byte of the first row of run k, vals[k] = k
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_thr_heads(const uint8_t *bwt, const T *ssa, uint64_t r, uint64_t rows, uint32_t *keys, uint32_t *vals)
{
    const uint64_t k = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= r) return;
    const uint64_t s = ssa[2 * k];
    keys[k] = s < rows ? bwt[s] : 0u;
    vals[k] = (uint32_t)k;
}

// tmin[t] / trow[t] = minimum of lcp over the rows [t * tile, (t + 1) * tile) and the leftmost row that holds it.  One wave per
// tile; `head` (< VW) = rows in front of the first 16-byte aligned one, the same in every tile (tile is a multiple of VW).  lcp[0]
// is row `row0` of the output (a multiple of the tile; 0 unless lcp is a window of the rows): trow holds output rows.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_thr_tile_min(const T *lcp, uint64_t rows, uint32_t head, uint32_t tile_log2, uint64_t ntiles, T *tmin, T *trow, uint64_t row0)
{
    constexpr int VW = 16 / sizeof(T);
    const int lane = threadIdx.x & 63;
    const uint64_t nw = (uint64_t)gridDim.x * (BLOCK / WAVE);
    for (uint64_t t = (uint64_t)blockIdx.x * (BLOCK / WAVE) + (threadIdx.x >> 6); t < ntiles; t += nw) {
        const uint64_t t0 = t << tile_log2, t1 = t0 + (1ULL << tile_log2) < rows ? t0 + (1ULL << tile_log2) : rows;
        const uint64_t v0 = t0 + head < t1 ? t0 + head : t1;              // first aligned row of the tile
        const uint64_t nvec = (t1 - v0) / VW, tail0 = v0 + nvec * VW;
        thr_u64 bv = THR_NONE, br = THR_NONE;
        if ((uint64_t)lane < v0 - t0) thr_take(lcp[t0 + lane], t0 + lane, bv, br);
        if ((uint64_t)lane < t1 - tail0) thr_take(lcp[tail0 + lane], tail0 + lane, bv, br);
        const Vec16<T> *vs = (const Vec16<T> *)(lcp + v0);
        for (uint64_t base = 0; base < nvec; base += (uint64_t)THR_UNROLL * WAVE) {
            Vec16<T> v[THR_UNROLL];
#pragma unroll
            for (int u = 0; u < THR_UNROLL; ++u) { const uint64_t j = base + (uint64_t)(u * WAVE + lane); if (j < nvec) v[u] = vs[j]; }
#pragma unroll
            for (int u = 0; u < THR_UNROLL; ++u) {
                const uint64_t j = base + (uint64_t)(u * WAVE + lane);
                if (j >= nvec) continue;
#pragma unroll
                for (int e = 0; e < VW; ++e) thr_take(v[u].v[e], v0 + j * VW + e, bv, br);
            }
        }
        thr_wave_min(bv, br);
        if (lane == 0) { tmin[t] = (T)bv; trow[t] = (T)(br + row0); }
    }
}

// out: [0] runs, [1] runs without a threshold, [2] runs handed to the long route, [3] largest s - e, [4] queue entries asked for
__device__ __forceinline__ void thr_wave_stats(bool live, bool none, bool is_long, thr_u64 span, unsigned long long *out)
{
    thr_u64 mx = span;
#pragma unroll
    for (int d = 32; d; d >>= 1) { const thr_u64 y = __shfl_xor(mx, d); mx = y > mx ? y : mx; }
    const unsigned long long nl = __popcll(__ballot(live)), nn = __popcll(__ballot(none)), ng = __popcll(__ballot(is_long));
    if ((threadIdx.x & 63) == 0) {
        if (nl) atomicAdd(&out[0], nl);
        if (nn) atomicAdd(&out[1], nn);
        if (ng) atomicAdd(&out[2], ng);
        if (mx) atomicMax(&out[3], mx);
    }
}

// One lane per run, in the order of the sort by head byte: skey[i] / sval[i] = head byte and index k of the i-th run.  Writes the
// rows of both pairs, and the values of every run that has no threshold or a gap of at most long_min rows.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_thr_queries(const uint32_t *skey, const uint32_t *sval, const T *ssa, const T *lcp, uint64_t r, uint64_t rows, uint64_t long_min,
                                                     T *thr, T *tlcp, ThrLong *queue, uint64_t qcap, unsigned long long *out)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = i < r;
    uint64_t k = 0, s = 0, lo = 0;
    bool has = false;
    if (live) {
        k = sval[i];
        s = ssa[2 * k];
        thr[2 * k] = (T)s; tlcp[2 * k] = (T)s;
        if (i && skey[i] == skey[i - 1]) {
            lo = ssa[2 * ((uint64_t)sval[i - 1] + 1)];          // e + 1: the run behind the previous run of this symbol starts there
            has = lo >= 1 && lo <= s && s < rows;              // (always, with consistent samples)
        }
    }
    const uint64_t span = has ? s - lo + 1 : 0;
    const bool is_long = has && span > long_min;
    bool fin = live && !is_long;
    const uint64_t slot = lcp_queue_slot(is_long, &out[4]);
    if (is_long) {
        if (slot < qcap) { queue[slot].lo = lo; queue[slot].s = s; queue[slot].k = k; }
        else fin = true;                                        // queue full: this lane goes on alone
    }
    if (fin) {
        thr_u64 bv = 0, br = 0;
        if (has) {
            bv = THR_NONE;
            for (uint64_t row = lo; row <= s; ++row) { const thr_u64 v = lcp[row]; if (v < bv) { bv = v; br = row; } }
        }
        thr[2 * k + 1] = (T)br; tlcp[2 * k + 1] = (T)bv;
    }
    thr_wave_stats(live, live && !has, is_long, span, out);
}

// One wave per queued run: rows [lo, a), the tiles [a, b) from tmin / trow, rows [b, s] (a, b: the first tile border >= lo and the
// last one <= s + 1; no whole tile inside: the rows themselves).
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_thr_long(const T *lcp, const T *tmin, const T *trow, uint32_t tile_log2, const ThrLong *queue, uint64_t qcap,
                                                  T *thr, T *tlcp, const unsigned long long *out)
{
    const int lane = threadIdx.x & 63;
    const uint64_t asked = out[4], cnt = asked < qcap ? asked : qcap;
    const uint64_t nw = (uint64_t)gridDim.x * (BLOCK / WAVE);
    for (uint64_t q = (uint64_t)blockIdx.x * (BLOCK / WAVE) + (threadIdx.x >> 6); q < cnt; q += nw) {
        const uint64_t lo = queue[q].lo, s = queue[q].s, k = queue[q].k;
        const uint64_t a = ((lo + (1ULL << tile_log2) - 1) >> tile_log2) << tile_log2, b = ((s + 1) >> tile_log2) << tile_log2;
        thr_u64 bv = THR_NONE, br = THR_NONE;
        if (a >= b) thr_scan_rows(lcp, lo, s + 1, lane, bv, br);
        else {
            thr_scan_rows(lcp, lo, a, lane, bv, br);
            const uint64_t ta = a >> tile_log2, tb = b >> tile_log2;
            for (uint64_t base = ta; base < tb; base += (uint64_t)THR_UNROLL * WAVE) {
                T v[THR_UNROLL], w[THR_UNROLL];
#pragma unroll
                for (int u = 0; u < THR_UNROLL; ++u) { const uint64_t t = base + (uint64_t)(u * WAVE + lane); v[u] = t < tb ? tmin[t] : (T)0; w[u] = t < tb ? trow[t] : (T)0; }
#pragma unroll
                for (int u = 0; u < THR_UNROLL; ++u) { const uint64_t t = base + (uint64_t)(u * WAVE + lane); if (t < tb) thr_take(v[u], w[u], bv, br); }
            }
            thr_scan_rows(lcp, b, s + 1, lane, bv, br);
        }
        thr_wave_min(bv, br);
        if (lane == 0) { thr[2 * k + 1] = (T)br; tlcp[2 * k + 1] = (T)bv; }
    }
}

// ---- the windowed route (pfp_thresholds_windowed): the LCP rows exist one window [ws, we) at a time ----------------------------
// ws is a multiple of the tile, so a tile never straddles two windows.  The gap [lo, s] of a run is cut at the tile borders:
//   lo and s in one tile: the rows [lo, s], all in the window of s;
//   else: the head piece [lo, A) in the window of lo, the whole tiles [A, B) from tmin / trow, which hold ALL tiles of the output and
//   are folded after the last window (k_thr_fold_*), and the tail piece [B, s] in the window of s.
// k_thr_win_queries runs over the runs that START in the window (ssa is ascending in rows: a range of k).  Run h owns the pieces
// of its own gap that lie in the window -- the tail piece or the whole gap, and the head piece too when lo is in the same window
// -- and, as the run behind h - 1, the head piece of the gap that begins at ITS first row (the gap of the next run with the symbol
// of h - 1) when that gap ends in a later window.  So every run is touched by one lane (or, queued, one wave) per kernel; partial
// minima are combined in thr[2k + 1] / tlcp[2k + 1] with thr_take, which k_thr_win_init presets to the largest value of T.
constexpr uint32_t THR_FOLD_LANE = 8;           // whole tiles one lane folds on its own; a longer range is queued for a wave

// the gap of the run at index i of the sort by head byte: k, rows [lo, s]; false: the run has no threshold
template <typename T>
__device__ __forceinline__ bool thr_gap(const uint32_t *skey, const uint32_t *sval, const T *ssa, uint64_t rows, uint64_t i, uint64_t &k, uint64_t &lo, uint64_t &s)
{
    k = sval[i]; s = ssa[2 * k]; lo = 0;
    if (!i || skey[i] != skey[i - 1]) return false;
    lo = ssa[2 * ((uint64_t)sval[i - 1] + 1)];
    return lo >= 1 && lo <= s && s < rows;
}
// the raw-row pieces [x0, x1) and [y0, y1) of the gap [lo, s] that lie in the window [ws, we)
__device__ __forceinline__ void thr_pieces(uint64_t lo, uint64_t s, uint64_t ws, uint64_t we, uint32_t tile_log2, uint64_t &x0, uint64_t &x1, uint64_t &y0, uint64_t &y1)
{
    const uint64_t a = lo >> tile_log2, b = s >> tile_log2;
    const bool lo_in = lo >= ws && lo < we, s_in = s >= ws && s < we;
    x0 = x1 = y0 = y1 = 0;
    if (a == b) { if (s_in) { x0 = lo; x1 = s + 1; } return; }
    if (lo_in) { x0 = lo; x1 = (a + 1) << tile_log2; }
    if (s_in) { y0 = b << tile_log2; y1 = s + 1; }
}
template <typename T>
__device__ __forceinline__ void thr_lane_rows(const T *lcp, uint64_t row0, uint64_t x0, uint64_t x1, thr_u64 &bv, thr_u64 &br)
{
    for (uint64_t row = x0; row < x1; ++row) thr_take(lcp[row - row0], row, bv, br);
}

// pos[k] = index of run k in the sort by head byte
__global__ __launch_bounds__(BLOCK) void k_thr_inverse(const uint32_t *sval, uint64_t r, uint32_t *pos)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < r) pos[sval[i]] = (uint32_t)i;
}
// first[w] = the first run that starts at or behind row w * window_rows (w = 0 .. nwin)
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_thr_win_bounds(const T *ssa, uint64_t r, uint64_t window_rows, uint64_t nwin, unsigned long long *first)
{
    const uint64_t w = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (w > nwin) return;
    const uint64_t row = w * window_rows;
    uint64_t lo = 0, hi = r;
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if ((uint64_t)ssa[2 * mid] < row) lo = mid + 1; else hi = mid; }
    first[w] = lo;
}
// One lane per run in sorted order: the rows of both pairs, the start values of the reduction, and the statistics of pfp_thr_info
// (a gap counts as long by its length, whatever route its pieces take).
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_thr_win_init(const uint32_t *skey, const uint32_t *sval, const T *ssa, uint64_t r, uint64_t rows, uint64_t long_min, T *thr, T *tlcp, unsigned long long *out)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = i < r;
    uint64_t k = 0, s = 0, lo = 0;
    bool has = false;
    if (live) {
        has = thr_gap<T>(skey, sval, ssa, rows, i, k, lo, s);
        thr[2 * k] = (T)s; tlcp[2 * k] = (T)s;
        thr[2 * k + 1] = has ? (T)~(T)0 : (T)0; tlcp[2 * k + 1] = has ? (T)~(T)0 : (T)0;
    }
    const uint64_t span = has ? s - lo + 1 : 0;
    thr_wave_stats(live, live && !has, has && span > long_min, span, out);
}
// one job of k_thr_win_queries: the pieces of the gap [lo, s] of run k in the window, by this lane or -- more than long_min rows -- a wave
template <typename T>
__device__ __forceinline__ void thr_win_job(bool want, uint64_t k, uint64_t lo, uint64_t s, const T *lcp, uint64_t ws, uint64_t we, uint64_t long_min, uint32_t tile_log2,
                                            T *thr, T *tlcp, ThrLong *queue, uint64_t qcap, unsigned long long *out)
{
    uint64_t x0 = 0, x1 = 0, y0 = 0, y1 = 0;
    if (want) thr_pieces(lo, s, ws, we, tile_log2, x0, x1, y0, y1);
    const bool is_long = want && (x1 - x0) + (y1 - y0) > long_min;
    bool fin = want && !is_long;
    const uint64_t slot = lcp_queue_slot(is_long, &out[4]);
    if (is_long) {
        if (slot < qcap) { queue[slot].lo = lo; queue[slot].s = s; queue[slot].k = k; }
        else fin = true;                                        // queue full: this lane goes on alone
    }
    if (fin && (x1 > x0 || y1 > y0)) {
        thr_u64 bv = tlcp[2 * k + 1], br = thr[2 * k + 1];
        thr_lane_rows(lcp, ws, x0, x1, bv, br);
        thr_lane_rows(lcp, ws, y0, y1, bv, br);
        thr[2 * k + 1] = (T)br; tlcp[2 * k + 1] = (T)bv;
    }
}
// One lane per run h in [k0, k1), the runs that start in the window [ws, we); lcp[0] is row ws.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_thr_win_queries(const uint32_t *skey, const uint32_t *sval, const uint32_t *pos, const T *ssa, const T *lcp, uint64_t ws, uint64_t we, uint64_t k0, uint64_t k1,
                                                         uint64_t r, uint64_t rows, uint64_t long_min, uint32_t tile_log2, T *thr, T *tlcp, ThrLong *queue, uint64_t qcap, unsigned long long *out)
{
    const uint64_t h = k0 + (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = h < k1;
    // its own gap: it ends in this window
    uint64_t k = 0, lo = 0, s = 0;
    bool own = false;
    if (live) own = thr_gap<T>(skey, sval, ssa, rows, pos[h], k, lo, s) && s >= ws && s < we;
    thr_win_job<T>(own, k, lo, s, lcp, ws, we, long_min, tile_log2, thr, tlcp, queue, qcap, out);
    // the gap that begins at its first row: that of the next run with the symbol of run h - 1, when it ends behind the window
    bool next = false;
    if (live && h) {
        const uint64_t i = (uint64_t)pos[h - 1] + 1;
        if (i < r) next = thr_gap<T>(skey, sval, ssa, rows, i, k, lo, s) && lo >= ws && lo < we && s >= we;
    }
    thr_win_job<T>(next, k, lo, s, lcp, ws, we, long_min, tile_log2, thr, tlcp, queue, qcap, out);
}
// One wave per queued job of the window
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_thr_win_long(const T *lcp, uint64_t ws, uint64_t we, uint32_t tile_log2, const ThrLong *queue, uint64_t qcap, T *thr, T *tlcp, const unsigned long long *out)
{
    const int lane = threadIdx.x & 63;
    const uint64_t asked = out[4], cnt = asked < qcap ? asked : qcap;
    const uint64_t nw = (uint64_t)gridDim.x * (BLOCK / WAVE);
    for (uint64_t q = (uint64_t)blockIdx.x * (BLOCK / WAVE) + (threadIdx.x >> 6); q < cnt; q += nw) {
        const uint64_t lo = queue[q].lo, s = queue[q].s, k = queue[q].k;
        uint64_t x0, x1, y0, y1;
        thr_pieces(lo, s, ws, we, tile_log2, x0, x1, y0, y1);
        thr_u64 bv = THR_NONE, br = THR_NONE;
        thr_scan_rows(lcp, x0, x1, lane, bv, br, ws);
        thr_scan_rows(lcp, y0, y1, lane, bv, br, ws);
        thr_wave_min(bv, br);
        if (lane == 0) {
            thr_take(tlcp[2 * k + 1], thr[2 * k + 1], bv, br);
            thr[2 * k + 1] = (T)br; tlcp[2 * k + 1] = (T)bv;
        }
    }
}
// After the last window, one lane per run in sorted order: the whole tiles inside its gap.  Up to THR_FOLD_LANE tiles by the lane, a
// longer range is queued for a wave (lo, s of the entry: the tile range).
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_thr_fold_queries(const uint32_t *skey, const uint32_t *sval, const T *ssa, const T *tmin, const T *trow, uint64_t r, uint64_t rows, uint32_t tile_log2,
                                                          T *thr, T *tlcp, ThrLong *queue, uint64_t qcap, unsigned long long *out)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    uint64_t k = 0, lo = 0, s = 0, ta = 0, tb = 0;
    if (i < r && thr_gap<T>(skey, sval, ssa, rows, i, k, lo, s)) { ta = (lo >> tile_log2) + 1; tb = s >> tile_log2; }
    const bool any = tb > ta, is_long = any && tb - ta > THR_FOLD_LANE;
    bool fin = any && !is_long;
    const uint64_t slot = lcp_queue_slot(is_long, &out[4]);
    if (is_long) {
        if (slot < qcap) { queue[slot].lo = ta; queue[slot].s = tb; queue[slot].k = k; }
        else fin = true;
    }
    if (fin) {
        thr_u64 bv = tlcp[2 * k + 1], br = thr[2 * k + 1];
        for (uint64_t t = ta; t < tb; ++t) thr_take(tmin[t], trow[t], bv, br);
        thr[2 * k + 1] = (T)br; tlcp[2 * k + 1] = (T)bv;
    }
}
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_thr_fold_long(const T *tmin, const T *trow, const ThrLong *queue, uint64_t qcap, T *thr, T *tlcp, const unsigned long long *out)
{
    const int lane = threadIdx.x & 63;
    const uint64_t asked = out[4], cnt = asked < qcap ? asked : qcap;
    const uint64_t nw = (uint64_t)gridDim.x * (BLOCK / WAVE);
    for (uint64_t q = (uint64_t)blockIdx.x * (BLOCK / WAVE) + (threadIdx.x >> 6); q < cnt; q += nw) {
        const uint64_t ta = queue[q].lo, tb = queue[q].s, k = queue[q].k;
        thr_u64 bv = THR_NONE, br = THR_NONE;
        for (uint64_t base = ta; base < tb; base += (uint64_t)THR_UNROLL * WAVE) {
            T v[THR_UNROLL], w[THR_UNROLL];
#pragma unroll
            for (int u = 0; u < THR_UNROLL; ++u) { const uint64_t t = base + (uint64_t)(u * WAVE + lane); v[u] = t < tb ? tmin[t] : (T)0; w[u] = t < tb ? trow[t] : (T)0; }
#pragma unroll
            for (int u = 0; u < THR_UNROLL; ++u) { const uint64_t t = base + (uint64_t)(u * WAVE + lane); if (t < tb) thr_take(v[u], w[u], bv, br); }
        }
        thr_wave_min(bv, br);
        if (lane == 0) {
            thr_take(tlcp[2 * k + 1], thr[2 * k + 1], bv, br);
            thr[2 * k + 1] = (T)br; tlcp[2 * k + 1] = (T)bv;
        }
    }
}

} // namespace pfp
