// pfbwt-f_amd/csrc/markerquery.h -- marker queries on the device (pfp_mk_index / pfp_mk_query, include/pfbwt_hip.h; DESIGN.md
// section 2): which markers do the occurrences of a pattern overlap, and in how many rows each.  The marker array (markers.h) is
// indexed by BWT row and a backward search yields row intervals, so the answer is an intersection of intervals with records: no
// phi walk, no SA.
//
// The index is made from a .ma stream on the device:
//   k_mk_flags / compaction: the words that start a record; k_mk_records: one lane per record, first / last row, list length, and
//   `bad` for a stream that is not a marker array; k_mk_values + a sort of all list entries by value + heads + a scan: dense 32-bit
//   ids in ascending value order (mval[id] = the value); k_mk_pairs + a sort of (record << 32 | id) with heads only: every record's
//   list as ascending unique ids, lid[loff[k] .. loff[k + 1]).
// A query (the host side is in queries.h):
//   1. k_mk_search: one lane per pattern, the search of runindex.h with the interval of every candidate step kept in slot
//      off[j] + i of a per-base scratch (cnt 0: not probed).
//   2. k_mk_span: one lane per slot, two bisections of the record table: records [ka, kb) overlap the interval, the slot owns
//      loff[kb] - loff[ka] raw entries.  k_mk_praw: the raw entries of every pattern, for the host's chunks.
//   3. k_mk_expand: one lane per raw entry of a chunk: its slot, its record, key (pattern in chunk << idbits) | id and the weight
//      min(hi, last + 1) - max(lo, first), the rows of the interval inside the record.
//   4. one of two reductions per pattern, both giving identical arrays: k_mk_wave (at most 64 raw entries: one wave, one lane per
//      entry) or a sort of the keys, heads, and one 64-bit atomic add of every entry's weight into its head's slot (k_mk_sum;
//      k_dl_heads / k_dl_spans of doclist.h serve as they are).
//   5. k_mk_pack: the slices move, tight and in pattern order, to the results; ids become values again.
// Bounds: a word of the stream is used only when it is < words, a record only when it is < nrec, a list entry only when it is <
// entries, an id only when it is < distinct, an output slot only inside the pattern's upper-bound slice, a result slot only below
// `cap`, whatever the arrays hold (cf. the rule at the top of runindex.h).
#pragma once
#include "doclist.h"

namespace pfp {

constexpr uint64_t MK_DELIM = ~0ULL;               // ends a record (marker_array.hpp:143)
constexpr uint32_t MK_WAVE_MAX = 64;               // most raw entries of the wave route: one lane each
constexpr uint32_t MK_NONE = 0xFFFFFFFFu;          // no id (distinct < 2^32, so no marker has it)

// the marker index as the kernels see it: records first[k] .. last[k] (ascending, disjoint) with the ids lid[loff[k] .. loff[k + 1])
struct MkView { const uint64_t *first, *last; const uint32_t *loff, *lid; uint64_t nrec, entries, distinct; };

// the counters of the index build and of a query's kernels (`out`, zeroed by the host)
enum MkIndexOut { MKI_BAD, MKI_ROWS, MKI_MAX_LIST, MKI_OUT_COUNT_ };
enum MkOut { MK_FOUND, MK_STEPS, MK_OCCURRENCES, MK_PROBES, MK_CAPPED, MK_ROWS, MK_RECORDS, MK_OUT_COUNT_ };
static_assert(MK_OUT_COUNT_ <= OUT_BLOCK && MKI_OUT_COUNT_ <= OUT_BLOCK, "the counters of a marker query fit one block");

__device__ __forceinline__ ms_u64 mk_wave_sum(ms_u64 v)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ ms_u64 mk_wave_max(ms_u64 v)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) { const ms_u64 y = __shfl_xor(v, d); v = y > v ? y : v; }
    return v;
}

// ---- the index ----
// flag[x] = word x starts a record: word 0 and every word behind a delimiter
__global__ __launch_bounds__(BLOCK) void k_mk_flags(const uint64_t *ma, uint64_t words, uint32_t *flag)
{
    const uint64_t x = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (x < words) flag[x] = !x || ma[x - 1] == MK_DELIM;
}
// Record k = the words [rstart[k], rstart[k + 1]) (the last one: to the end of the stream): first row, last row, markers, delimiter.
// bad: no delimiter at its end (the last record of a stream that is cut short), no marker, first > last, last > n, first <= the
// last row of the record in front.
__global__ __launch_bounds__(BLOCK) void k_mk_records(const uint64_t *ma, uint64_t words, const uint32_t *rstart, uint64_t nrec, uint64_t n, uint64_t *first, uint64_t *last, ms_u64 *rawlen, ms_u64 *out)
{
    const uint64_t k = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    ms_u64 bad = 0, rows = 0;
    if (k < nrec) {
        const uint64_t s = rstart[k];
        uint64_t e = k + 1 < nrec ? (uint64_t)rstart[k + 1] : words; if (e > words) e = words;
        uint64_t f = 0, l = 0, len = 0;
        if (e < s + 4 || ma[e - 1] != MK_DELIM) bad = 1;
        else {
            f = ma[s]; l = ma[s + 1]; len = e - s - 3;
            if (f > l || l > n) bad = 1;
            if (k) { const uint64_t ps = rstart[k - 1]; if (ps + 1 >= words || f <= ma[ps + 1]) bad = 1; }
            if (!bad) rows = l - f + 1;
        }
        first[k] = f; last[k] = l; rawlen[k] = bad ? 0 : len;
    }
    bad = mk_wave_sum(bad); rows = mk_wave_sum(rows);
    if ((threadIdx.x & 63) == 0) { if (bad) atomicAdd(&out[MKI_BAD], bad); if (rows) atomicAdd(&out[MKI_ROWS], rows); }
}
// raw list entry x of record k = the owner of x in rawoff: its value as a sort key, x as the value
__global__ __launch_bounds__(BLOCK) void k_mk_values(const uint64_t *ma, uint64_t words, const uint32_t *rstart, const ms_u64 *rawoff, uint64_t nrec, uint64_t total, uint64_t *key, uint32_t *val, uint32_t *rec)
{
    const uint64_t x = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (x >= total) return;
    const uint64_t k = ri_owner(rawoff, nrec, x), w = (uint64_t)rstart[k] + 2 + (x - rawoff[k]);
    key[x] = w < words ? ma[w] : 0;
    val[x] = (uint32_t)x; rec[x] = (uint32_t)k;
}
// sorted entry x with hpos[x] heads in front: its id is the number of heads up to and including its own; the head keeps the value
__global__ __launch_bounds__(BLOCK) void k_mk_ids(const uint64_t *skey, const uint32_t *sval, const uint32_t *head, const uint32_t *hpos, uint64_t total, uint64_t distinct, uint64_t *mval, uint32_t *eid)
{
    const uint64_t x = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (x >= total) return;
    const uint64_t id = (uint64_t)hpos[x] + head[x] - 1, at = sval[x];
    if (id >= distinct || at >= total) return;                             // (inconsistent arrays only)
    if (head[x]) mval[id] = skey[x];
    eid[at] = (uint32_t)id;
}
__global__ __launch_bounds__(BLOCK) void k_mk_pairs(const uint32_t *rec, const uint32_t *eid, uint64_t total, uint64_t *key, uint32_t *val)
{
    const uint64_t x = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (x < total) { key[x] = ((uint64_t)rec[x] << 32) | eid[x]; val[x] = (uint32_t)x; }
}
// the heads of the sorted (record, id) pairs are the lists: head x goes to lid[hpos[x]]
__global__ __launch_bounds__(BLOCK) void k_mk_lists(const uint64_t *skey, const uint32_t *head, const uint32_t *hpos, uint64_t total, uint64_t entries, uint32_t *lid)
{
    const uint64_t x = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (x < total && head[x] && hpos[x] < entries) lid[hpos[x]] = (uint32_t)skey[x];
}
// loff[k] = the heads in front of the first pair of record k (that pair is a head); loff[nrec] = entries
__global__ __launch_bounds__(BLOCK) void k_mk_loff(const uint64_t *skey, const uint32_t *hpos, uint64_t total, uint64_t nrec, uint64_t entries, uint32_t *loff, ms_u64 *out)
{
    const uint64_t k = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    ms_u64 mx = 0;
    if (k < nrec) {
        uint64_t at[2];
        for (int s = 0; s < 2; ++s) {
            uint64_t lo = 0, hi = total;                                   // first pair of a record >= k + s
            while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if ((skey[mid] >> 32) >= k + s) hi = mid; else lo = mid + 1; }
            at[s] = lo < total ? (uint64_t)hpos[lo] : entries;
            if (at[s] > entries) at[s] = entries;
        }
        loff[k] = (uint32_t)at[0];
        if (k + 1 == nrec) loff[nrec] = (uint32_t)entries;
        mx = at[1] > at[0] ? at[1] - at[0] : 0;
    }
    mx = mk_wave_max(mx);
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(&out[MKI_MAX_LIST], mx);
}

// ---- the query ----
// One lane per pattern: lane g takes pattern order[g].  The loop is ri_search_steps (runindex.h) without a toehold, except that it
// goes on to the pattern's first byte after the interval has become empty, because every step has a slot: step i (the suffix
// P[i .. m)) is a candidate when min_len == 0 ? i == 0 : m - i >= min_len; a candidate with cnt_i >= 1 is probed when max_rows == 0
// or cnt_i <= max_rows -- slo / scnt[off[j] + i] = its interval -- and capped otherwise; every other slot gets cnt 0.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_mk_search(MsView<T> ix, const uint8_t *P, const uint64_t *off, const uint32_t *order, uint64_t np, uint64_t min_len, uint64_t max_rows, T *slo, T *scnt, T *cnt_out, T *probes_out, ms_u64 *out)
{
    const uint64_t g = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    ms_u64 nfound = 0, nsteps = 0, cnt0 = 0, nprobes = 0, ncapped = 0, nrows = 0;
    if (g < np) {
        const uint64_t j = order[g], x0 = off[j], m = off[j + 1] - x0;
        uint64_t lo = 0, hi = m ? ix.n + 1 : 0;
        for (uint64_t i = m; i-- > 0;) {
            if (lo < hi) {
                const uint32_t c = P[x0 + i];
                const uint32_t f = ix.sym[c], l = ix.sym[c + 1];           // the runs of c in `sorted`
                ++nsteps;
                if (f >= l) hi = lo;
                else {
                    bool hit; uint32_t idx;
                    const uint64_t t = hi - 1, kl = ms_run_of<T>(ix, lo), kt = ms_run_of<T>(ix, t);
                    uint64_t nlo = ri_lf<T>(ix, c, f, l, lo, kl, &hit, &idx);
                    uint64_t nhi = ri_lf<T>(ix, c, f, l, t, kt, &hit, &idx);
                    if (hit) ++nhi;
                    if (nhi > ix.n + 1) nhi = ix.n + 1;                    // (inconsistent samples only)
                    if (nlo > nhi) nlo = nhi;
                    lo = nlo; hi = nhi;
                }
            }
            const uint64_t ci = hi - lo;
            const bool cand = min_len ? m - i >= min_len : i == 0;
            const bool probe = cand && ci && (!max_rows || ci <= max_rows);
            slo[x0 + i] = (T)(probe ? lo : 0); scnt[x0 + i] = (T)(probe ? ci : 0);
            nprobes += probe; ncapped += cand && ci && !probe; nrows += probe ? ci : 0;
            if (!i) cnt0 = ci;
        }
        cnt_out[j] = (T)cnt0; probes_out[j] = (T)nprobes;
        nfound = cnt0 != 0;
    }
    nfound = mk_wave_sum(nfound); nsteps = mk_wave_sum(nsteps); cnt0 = mk_wave_sum(cnt0); nprobes = mk_wave_sum(nprobes); ncapped = mk_wave_sum(ncapped); nrows = mk_wave_sum(nrows);
    if ((threadIdx.x & 63) == 0) {
        if (nfound) atomicAdd(&out[MK_FOUND], nfound);
        if (nsteps) atomicAdd(&out[MK_STEPS], nsteps);
        if (cnt0) atomicAdd(&out[MK_OCCURRENCES], cnt0);
        if (nprobes) atomicAdd(&out[MK_PROBES], nprobes);
        if (ncapped) atomicAdd(&out[MK_CAPPED], ncapped);
        if (nrows) atomicAdd(&out[MK_ROWS], nrows);
    }
}
// One lane per slot x: ka = the first record with last >= lo, kb = the first record with first >= hi; raw[x] = the list entries of
// the records [ka, kb).  out[MK_RECORDS] += kb - ka.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_mk_span(MkView mv, const T *slo, const T *scnt, uint64_t total, uint32_t *ka_out, ms_u64 *raw, ms_u64 *out)
{
    const uint64_t x = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    ms_u64 nrecs = 0;
    if (x < total) {
        const uint64_t c = scnt[x];
        uint64_t ka = 0, kb = 0;
        if (c) {
            const uint64_t lo = slo[x], hi = lo + c;
            uint64_t a = 0, b = mv.nrec;
            while (a < b) { const uint64_t mid = (a + b) >> 1; if (mv.last[mid] >= lo) b = mid; else a = mid + 1; }
            ka = a; b = mv.nrec;
            while (a < b) { const uint64_t mid = (a + b) >> 1; if (mv.first[mid] >= hi) b = mid; else a = mid + 1; }
            kb = a;
        }
        const uint64_t ea = mv.loff[ka], eb = mv.loff[kb];                  // (ka <= kb <= nrec)
        ka_out[x] = (uint32_t)ka; raw[x] = eb > ea ? eb - ea : 0;
        nrecs = kb - ka;
    }
    nrecs = mk_wave_sum(nrecs);
    if ((threadIdx.x & 63) == 0 && nrecs) atomicAdd(&out[MK_RECORDS], nrecs);
}
// praw[j] = the raw entries of pattern j, from the exclusive sums rbase[0 .. total] over the slots
__global__ __launch_bounds__(BLOCK) void k_mk_praw(const ms_u64 *rbase, const uint64_t *off, uint64_t np, ms_u64 *praw)
{
    const uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j < np) praw[j] = rbase[off[j + 1]] - rbase[off[j]];
}
// One lane per raw entry y of the chunk (the patterns [j0, j0 + npc), slots [s0, s0 + nslots), global entries from g0 = rbase[s0]):
// pattern q = the owner of y in pbase, slot x = the owner of g0 + y in rbase, record k = the one of [ka[x], nrec) whose list holds
// entry loff[ka[x]] + (g0 + y - rbase[x]).  key[y] = (q << idbits) | id for a pattern of the sort route (route[q] == 2), else behind
// every pattern (npc << idbits) | id; wt[y] = the rows of the slot's interval inside record k.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_mk_expand(MkView mv, const T *slo, const T *scnt, const uint32_t *ka, const ms_u64 *rbase, uint64_t s0, uint64_t nslots, const ms_u64 *pbase, uint64_t npc, const uint8_t *route,
                                                   uint64_t total, int idbits, uint64_t *key, uint32_t *val, ms_u64 *wt)
{
    const uint64_t y = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (y >= total) return;
    const uint64_t q = ri_owner(pbase, npc, y), g = rbase[s0] + y;
    const uint64_t x = s0 + ri_owner(rbase + s0, nslots, g);
    uint64_t id = MK_NONE, w = 0;
    const uint64_t k0 = ka[x];
    if (k0 < mv.nrec) {
        const uint64_t e = (uint64_t)mv.loff[k0] + (g - rbase[x]);
        uint64_t a = k0, b = mv.nrec;                                      // the last record of [k0, nrec) with loff <= e
        while (b - a > 1) { const uint64_t mid = (a + b) >> 1; if ((uint64_t)mv.loff[mid] <= e) a = mid; else b = mid; }
        if (e < mv.entries) {
            const uint64_t lo = slo[x], hi = lo + (uint64_t)scnt[x], f = mv.first[a], l = mv.last[a] + 1;
            const uint64_t from = lo > f ? lo : f, to = hi < l ? hi : l;
            id = mv.lid[e]; w = to > from ? to - from : 0;
        }
    }
    if (id >= mv.distinct) { id = 0; w = 0; }                              // (inconsistent arrays only: weight 0 lists nothing)
    key[y] = ((route[q] == 2 ? q : npc) << idbits) | id;
    val[y] = (uint32_t)y; wt[y] = w;
}

// One wave per pattern list[q] (at most 64 raw entries): lane l holds the id and the weight of entry l.  For every lane i whose id
// is the first of its value the weights of the lanes with that id are summed over the wave (they differ, so no population count
// will do); a lane's rank is the number of such values below its own.  Ids of weight 0 (inconsistent arrays only) are not listed.
__global__ __launch_bounds__(BLOCK) void k_mk_wave(const uint64_t *key, const ms_u64 *wt, const ms_u64 *pbase, const ms_u64 *ub, const uint32_t *list, uint64_t nlist, int idbits, uint32_t *tid, ms_u64 *tfreq, ms_u64 *ne)
{
    const uint64_t p = (uint64_t)blockIdx.x * (BLOCK / WAVE) + (threadIdx.x >> 6);
    if (p >= nlist) return;                                                // (the whole wave)
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t q = list[p], ob = pbase[q];
    uint64_t c = pbase[q + 1] - ob; if (c > MK_WAVE_MAX) c = MK_WAVE_MAX;
    const uint64_t u0 = ub[q], ulen = ub[q + 1] - u0, mask = (1ULL << idbits) - 1;
    const bool valid = lane < c;
    const uint32_t d = valid ? (uint32_t)(key[ob + lane] & mask) : MK_NONE;
    const ms_u64 w = valid ? wt[ob + lane] : 0;
    uint32_t rank = 0, distinct = 0;
    ms_u64 freq = 0;
    for (uint32_t i = 0; i < (uint32_t)c; ++i) {
        const uint32_t di = __shfl(d, (int)i);
        const unsigned long long same = __ballot(valid && d == di);
        if ((uint32_t)(__ffsll((long long)same) - 1) != i) continue;       // (uniform: not the first lane with this id)
        const ms_u64 sum = mk_wave_sum(valid && d == di ? w : 0);
        if (!sum) continue;                                                // (uniform)
        ++distinct;
        if (valid && di < d) ++rank;
        if (lane == i) freq = sum;
    }
    if (freq && rank < ulen) { tid[u0 + rank] = d; tfreq[u0 + rank] = freq; }
    if (lane == 0) ne[q] = distinct < ulen ? distinct : ulen;
}

// The sort route, one lane per sorted entry x: its head is number hpos[x] + head[x] - 1; the head writes the id into its slot of the
// pattern's slice and the count of the pattern's heads, every entry adds its weight to the slot's frequency (tfreq zeroed by the host).
__global__ __launch_bounds__(BLOCK) void k_mk_sum(const uint64_t *skey, const uint32_t *sval, const ms_u64 *wt, const uint32_t *head, const uint32_t *hpos, uint64_t total, uint64_t npc, int idbits, uint64_t distinct,
                                                const uint32_t *first, const uint32_t *last, const ms_u64 *ub, uint32_t *tid, ms_u64 *tfreq, ms_u64 *ne)
{
    const uint64_t x = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (x >= total) return;
    const uint64_t q = skey[x] >> idbits, id = skey[x] & ((1ULL << idbits) - 1), at = sval[x];
    if (q >= npc || id >= distinct || at >= total) return;
    const uint64_t h = (uint64_t)hpos[x] + head[x] - 1, f = first[q], l = last[q], u0 = ub[q], ulen = ub[q + 1] - u0;
    if (h < f || h >= l) return;                                           // (inconsistent arrays only)
    const uint64_t rank = h - f;
    if (rank < ulen) {
        if (head[x]) tid[u0 + rank] = (uint32_t)id;
        atomicAdd(&tfreq[u0 + rank], wt[at]);
    }
    if (head[x] && h == f) ne[q] = l - f < ulen ? l - f : ulen;
}

// One lane per slot y of the upper-bound slices: slot r of pattern j moves to e0 + eoff[j] + r of the results when r < ne[j]
__global__ __launch_bounds__(BLOCK) void k_mk_pack(const uint32_t *tid, const ms_u64 *tfreq, const uint64_t *mval, uint64_t distinct, const ms_u64 *ub, const ms_u64 *eoff, uint64_t npc, uint64_t slots, uint64_t e0, uint64_t cap,
                                                 uint64_t *marker, uint64_t *freq)
{
    const uint64_t y = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (y >= slots) return;
    const uint64_t j = ri_owner(ub, npc, y), r = y - ub[j];
    if (r >= eoff[j + 1] - eoff[j]) return;
    const uint64_t at = e0 + eoff[j] + r, id = tid[y];
    if (at < cap && id < distinct) { marker[at] = mval[id]; freq[at] = tfreq[y]; }
}

} // namespace pfp
