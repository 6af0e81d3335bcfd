// pfbwt-f_amd/csrc/hooks.h -- the development hooks of include/pfbwt_hip_dev.h that look at a context from outside: checksums of device
// buffers, the checkers of a build's outputs (sample order, suffix array, run samples), the timing of the pair sort, and the device-wide
// primitives of prims.h on a caller's arrays (tests/test_prims.py).  No product path calls any of this.  First the kernels and the host
// helpers, then the entries.  Included by pfbwt_hip.hip (ensure_arena).
#pragma once

// The counters of a checker: N zeroed 64-bit counters on the device that the kernels add to; fetch() brings them into h, and they are
// freed on every path out.  (hipMalloc, not the arena: the checkers run while the arena holds the results they look at.)
// A launch gets the plain pointer that open() hands out, never `cnt.d`: the CPU interpreter of the tests runs a launch from a lambda that
// copies every variable its argument list names, and a copy of this struct would free the counters when that lambda ends.
template <int N> struct DevCounters {
    unsigned long long *d = nullptr, h[N] = {};
    DevCounters() = default;
    DevCounters(const DevCounters &) = delete;
    ~DevCounters() { if (d) (void)hipFree(d); }
    int open(pfp_ctx *c, unsigned long long **d_out) { PFP_HIP(c, hipMalloc((void **)&d, N * 8)); PFP_HIP(c, hipMemsetAsync(d, 0, N * 8, c->stream)); *d_out = d; return PFP_OK; }
    int fetch(pfp_ctx *c) { PFP_HIP(c, hipMemcpyAsync(h, d, N * 8, hipMemcpyDeviceToHost, c->stream)); PFP_HIP(c, hipStreamSynchronize(c->stream)); return PFP_OK; }
};

// (the kernels that are no templates keep C linkage: the names profiles and kernel statistics know them by)
// ---- development aid: position-weighted checksum of a device buffer (sum over bytes of (byte + 1) * mix(global position),
// two independent mixes, modulo 2^64): the checksums of the pieces of a buffer add up to the checksum of the whole, so
// outputs that live sliced over several builds / GPUs can be compared with a single-context output without moving them
extern "C" __global__ __launch_bounds__(BLOCK) void k_checksum(const uint8_t *p, uint64_t bytes, uint64_t offset, unsigned long long *out)
{
    __shared__ unsigned long long red[4];
    const uint64_t i0 = ((uint64_t)blockIdx.x * BLOCK + threadIdx.x) * 16;
    unsigned long long a = 0, b = 0;
    for (int k = 0; k < 16 && i0 + k < bytes; ++k) {
        const uint64_t pos = offset + i0 + k, v = (uint64_t)p[i0 + k] + 1;
        a += v * mix64(pos * 0x9E3779B97F4A7C15ULL + 1); b += v * mix64(pos * 0xD6E8FEB86659FD93ULL + 7);
    }
    unsigned long long ta, tb;
    (void)block_excl_sum(a, red, &ta); (void)block_excl_sum(b, red, &tb);
    if (threadIdx.x == 0) { atomicAdd(&out[0], ta); atomicAdd(&out[1], tb); }
}

// sum of the 64-bit words of a device buffer and sum of word * (index + 1), modulo 2^64 (bench.py compares the outputs that
// reached host memory with the device-resident ones this way; bytes behind the last whole word count as a zero-padded word)
extern "C" __global__ __launch_bounds__(BLOCK) void k_wordsum(const uint8_t *p, uint64_t bytes, unsigned long long *out)
{
    __shared__ unsigned long long red[4];
    const uint64_t nw = (bytes + 7) / 8;
    unsigned long long a = 0, b = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < nw; i += (uint64_t)gridDim.x * BLOCK) {
        unsigned long long v = 0;
        if (8 * i + 8 <= bytes) v = ld8(p + 8 * i); else for (uint64_t k = 0; 8 * i + k < bytes; ++k) v |= (unsigned long long)p[8 * i + k] << (8 * k);
        a += v; b += v * (i + 1);
    }
    unsigned long long ta, tb;
    (void)block_excl_sum(a, red, &ta); (void)block_excl_sum(b, red, &tb);
    if (threadIdx.x == 0) { atomicAdd(&out[0], ta); atomicAdd(&out[1], tb); }
}

// Full-size order check that does not lean on the engine's own sorting: .esa[k] and .ssa[k + 1] are ADJACENT
// rows of the BWT matrix (a run ends, the next one starts), so the suffix at esa[k].sa must be lexicographically smaller than the
// suffix at ssa[k + 1].sa -- compared directly on the text that is still resident (its w Dollars stand for the terminator, which is
// smaller than every base).  One thread per pair, eight bytes per step.  out: pairs checked, order violations, pairs whose rows
// are not adjacent, longest common prefix seen, sum of the common prefixes.
template <typename SAT> __global__ __launch_bounds__(BLOCK) void k_check_sample_order(const uint8_t *X, uint64_t n, const SAT *ssa, const SAT *esa, uint64_t r, unsigned long long *out)
{
    const uint64_t k = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k + 1 >= r) return;
    const uint64_t ra = esa[2 * k], a = esa[2 * k + 1], rb = ssa[2 * k + 2], b = ssa[2 * k + 3];
    if (ra + 1 != rb) atomicAdd(&out[2], 1ULL);
    uint64_t h = 0; bool ok = false;
    for (;;) {
        const uint64_t pa = a + h, pb = b + h;
        if (pa > n || pb > n) break;                                        // (cannot happen: the Dollar at n ends every comparison)
        const uint64_t va = ld8(X + pa), vb = ld8(X + pb);                  // the buffer holds w Dollars and slack behind the text
        if (va != vb) {
            const int sh = (__ffsll((long long)(va ^ vb)) - 1) & ~7;
            const uint64_t q = (uint64_t)sh >> 3;
            if (pa + q > n || pb + q > n) break;                            // the difference lies behind the terminator of one of them: not an order
            ok = ((va >> sh) & 0xFF) < ((vb >> sh) & 0xFF); h += q;
            break;
        }
        h += 8;
    }
    if (!ok) atomicAdd(&out[1], 1ULL);
    atomicAdd(&out[0], 1ULL); atomicMax(&out[3], (unsigned long long)h); atomicAdd(&out[4], (unsigned long long)h);
}

// Properties of a full suffix array at any size, on the device (the host-side version, tools/big_check.py, needs minutes and
// 10 bytes of host memory per base): every value of [0, n] occurs exactly once (bitmap + atomicOr), row 0 holds n, BWT[row] is the
// text byte in front of SA[row] (0x00 for the one row whose suffix is the whole text).  out: rows checked, values out of range,
// values seen twice, rows with a wrong BWT byte, 0x00 bytes in the BWT.
template <typename SAT> __global__ __launch_bounds__(BLOCK) void k_check_sa(const uint8_t *X, uint64_t n, const SAT *sa, const uint8_t *bwt, uint64_t rows, uint32_t *seen, unsigned long long *out)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= rows) return;
    const uint64_t v = sa[i];
    if (v > n) { atomicAdd(&out[1], 1ULL); return; }
    const uint32_t bit = 1u << (v & 31);
    if (atomicOr(&seen[v >> 5], bit) & bit) atomicAdd(&out[2], 1ULL);
    const uint8_t want = v == 0 ? (uint8_t)0 : X[v - 1];
    if (bwt[i] != want || (i == 0 && v != n)) atomicAdd(&out[3], 1ULL);
    if (bwt[i] == 0) atomicAdd(&out[4], 1ULL);
}

// The run samples of a -s -r build against its own full outputs, on the device (S-3G: 2.3 G runs = 74 GB of samples, not something
// a test moves to the host): run k starts at row ssa[k].row, a position where the BWT byte changes (or row 0), and ends at
// esa[k].row = ssa[k + 1].row - 1 (the last one at the last row); the values are the SA entries of those rows (src/pfbwt-f.cpp:304-315,
// 325-328).  r itself is the engine's count of byte changes, so r distinct change positions are all of them.
// out: runs checked, runs with a wrong row, runs with a wrong value.
template <typename SAT> __global__ __launch_bounds__(BLOCK) void k_check_samples(const SAT *ssa, const SAT *esa, uint64_t r, const SAT *sa, const uint8_t *bwt, uint64_t rows, unsigned long long *out)
{
    const uint64_t k = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= r) return;
    const uint64_t rs = ssa[2 * k], vs = ssa[2 * k + 1], re = esa[2 * k], ve = esa[2 * k + 1];
    bool row_ok = rs < rows && re < rows && rs <= re;
    if (row_ok) {
        row_ok = (k == 0 ? rs == 0 : bwt[rs] != bwt[rs - 1]) && (k + 1 == r ? re + 1 == rows : (uint64_t)ssa[2 * k + 2] == re + 1) && bwt[rs] == bwt[re];
    }
    if (!row_ok) { atomicAdd(&out[1], 1ULL); return; }
    if ((uint64_t)sa[rs] != vs || (uint64_t)sa[re] != ve) atomicAdd(&out[2], 1ULL);
}

// ---- development aid: time the pair sort on pseudo-random keys (no product path calls this) ----------
// the key of pair i: a pure function of i + seed, so that the check can tell whether a value still sits next to its key
__device__ __forceinline__ uint64_t debug_key(uint64_t i, int bits, uint64_t seed)
{
    uint64_t z = (i + seed) * 0x9E3779B97F4A7C15ULL; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL; z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL; z ^= z >> 31;
    return bits >= 64 ? z : (z & ((1ULL << bits) - 1ULL));
}
extern "C" __global__ __launch_bounds__(BLOCK) void k_debug_fill(uint64_t *keys, uint32_t *vals, uint64_t n, int bits, uint64_t seed)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    keys[i] = debug_key(i, bits, seed); vals[i] = (uint32_t)i;
}
// bad[0]: neighbours out of order; bad[1]: values that are no index or whose key is not the one k_debug_fill gave that index
extern "C" __global__ __launch_bounds__(BLOCK) void k_debug_check_sorted(const uint64_t *keys, const uint32_t *vals, uint64_t n, int bits, uint64_t seed, uint32_t *bad)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i + 1 < n && keys[i] > keys[i + 1]) atomicAdd(&bad[0], 1u);
    if (i < n && ((uint64_t)vals[i] >= n || keys[i] != debug_key(vals[i], bits, seed))) atomicAdd(&bad[1], 1u);
}

namespace pfp {
// ---- the device-wide primitives of prims.h on the caller's arrays (tests/test_prims.py)
// A device buffer of these hooks: DEBUG_GUARD bytes of a pattern in front of and behind its `bytes` bytes (a store past the end of an
// array inside the arena faults nowhere; the guards show it), the bytes themselves filled with `fill`.
constexpr size_t DEBUG_GUARD = 256;              // keeps the 256-byte alignment the arena gives every product buffer
constexpr uint8_t DEBUG_GUARD_BYTE = 0xA5;
struct GuardedBuf { char *raw = nullptr; size_t bytes = 0; template <typename T> T *data() const { return (T *)(raw + DEBUG_GUARD); } };
static int guarded_alloc(pfp_ctx *c, size_t bytes, uint8_t fill, GuardedBuf *g)
{
    g->raw = (char *)c->arena.alloc_hi(bytes + 2 * DEBUG_GUARD); g->bytes = bytes;
    if (!g->raw) return PFP_E_NOMEM;
    PFP_HIP(c, hipMemsetAsync(g->raw, DEBUG_GUARD_BYTE, DEBUG_GUARD, c->stream));
    if (bytes) PFP_HIP(c, hipMemsetAsync(g->raw + DEBUG_GUARD, fill, bytes, c->stream));
    PFP_HIP(c, hipMemsetAsync(g->raw + DEBUG_GUARD + bytes, DEBUG_GUARD_BYTE, DEBUG_GUARD, c->stream));
    return PFP_OK;
}
// *changed += the guard bytes of g that no longer hold the pattern (the stream is synchronised)
static int guards_check(pfp_ctx *c, const GuardedBuf &g, uint32_t *changed)
{
    uint8_t h[2 * DEBUG_GUARD];
    PFP_HIP(c, hipMemcpyAsync(h, g.raw, DEBUG_GUARD, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipMemcpyAsync(h + DEBUG_GUARD, g.raw + DEBUG_GUARD + g.bytes, DEBUG_GUARD, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    uint32_t bad = 0; size_t first = 0;
    for (size_t i = 0; i < 2 * DEBUG_GUARD; ++i) if (h[i] != DEBUG_GUARD_BYTE && !bad++) first = i;
    if (bad && c->tun.verbose) fprintf(stderr, "[pfbwt_hip] guard of the %zu-byte buffer at arena offset %zu (arena %p + %zu): %u bytes changed, the first %s the data at guard byte %zu: %02x\n", g.bytes,
                                       c->arena.offset_of(g.raw), (void *)c->arena.base, c->arena.cap, bad, first < DEBUG_GUARD ? "in front of" : "behind", first % DEBUG_GUARD, h[first]);
    *changed += bad;
    return PFP_OK;
}
template <typename K> static int debug_sort_pairs(pfp_ctx *c, const K *keys, const uint32_t *vals, uint64_t n, const BitRange *ranges, int nranges, K *keys_out, uint32_t *vals_out, uint32_t *changed)
{
    GuardedBuf k[2], v[2];
    for (int i = 0; i < 2; ++i) { PFP_TRY(guarded_alloc(c, n * sizeof(K), 0xEE, &k[i])); PFP_TRY(guarded_alloc(c, n * 4, 0xEE, &v[i])); }
    if (n) {
        PFP_HIP(c, hipMemcpyAsync(k[0].data<K>(), keys, n * sizeof(K), hipMemcpyHostToDevice, c->stream));
        PFP_HIP(c, hipMemcpyAsync(v[0].data<uint32_t>(), vals, n * 4, hipMemcpyHostToDevice, c->stream));
    }
    K *sk; uint32_t *sv;
    PFP_TRY(radix_sort_pairs<K>(c, k[0].data<K>(), v[0].data<uint32_t>(), k[1].data<K>(), v[1].data<uint32_t>(), n, ranges, nranges, &sk, &sv));
    if (n) {
        PFP_HIP(c, hipMemcpyAsync(keys_out, sk, n * sizeof(K), hipMemcpyDeviceToHost, c->stream));
        PFP_HIP(c, hipMemcpyAsync(vals_out, sv, n * 4, hipMemcpyDeviceToHost, c->stream));
    }
    for (int i = 0; i < 2; ++i) { PFP_TRY(guards_check(c, k[i], changed)); PFP_TRY(guards_check(c, v[i], changed)); }
    return PFP_OK;
}
template <typename T, int OP> static int debug_scan(pfp_ctx *c, const T *in, int mode, uint64_t n, T *out, T *total, uint32_t *changed)
{
    GuardedBuf src, dst, tot;
    PFP_TRY(guarded_alloc(c, n * sizeof(T), 0xEE, &dst));
    PFP_TRY(guarded_alloc(c, sizeof(T), 0xEE, &tot));
    T *d_total = total ? tot.data<T>() : nullptr;
    if (mode == 0) {
        PFP_TRY(guarded_alloc(c, n * sizeof(T), 0xEE, &src));
        if (n) PFP_HIP(c, hipMemcpyAsync(src.data<T>(), in, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
        PFP_TRY((device_scan<T, OP>(c, (const T *)src.data<T>(), dst.data<T>(), n, d_total)));
    } else {
        if (n) PFP_HIP(c, hipMemcpyAsync(dst.data<T>(), in, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
        if (mode == 1) PFP_TRY((device_scan<T, OP>(c, (const T *)dst.data<T>(), dst.data<T>(), n, d_total)));
        else PFP_LAUNCH(c, K_SCAN_SPINE, n * sizeof(T) * 2, (k_scan_spine<T, OP>), 1, dst.data<T>(), n, d_total);
    }
    if (n) PFP_HIP(c, hipMemcpyAsync(out, dst.data<T>(), n * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    if (total) PFP_HIP(c, hipMemcpyAsync(total, tot.data<T>(), sizeof(T), hipMemcpyDeviceToHost, c->stream));
    PFP_TRY(guards_check(c, dst, changed)); PFP_TRY(guards_check(c, tot, changed));
    if (mode == 0) {      // the input of an out-of-place scan stays as it was
        PFP_TRY(guards_check(c, src, changed));
        std::vector<T> back((size_t)n);
        if (n) PFP_HIP(c, hipMemcpy(back.data(), src.data<T>(), n * sizeof(T), hipMemcpyDeviceToHost));
        if (n && memcmp(back.data(), in, n * sizeof(T))) *changed += 1;
    }
    return PFP_OK;
}
static int debug_compact(pfp_ctx *c, const uint32_t *in, const uint32_t *flag, uint64_t n, uint32_t *out, uint32_t *count, uint32_t *changed)
{
    GuardedBuf src, flg, dst, pos, cnt;
    PFP_TRY(guarded_alloc(c, n * 4, 0xEE, &src)); PFP_TRY(guarded_alloc(c, n * 4, 0xEE, &flg)); PFP_TRY(guarded_alloc(c, n * 4, 0xEE, &dst));
    PFP_TRY(guarded_alloc(c, n * 4, 0xEE, &pos)); PFP_TRY(guarded_alloc(c, 4, 0xEE, &cnt));
    if (n) {
        if (in) PFP_HIP(c, hipMemcpyAsync(src.data<uint32_t>(), in, n * 4, hipMemcpyHostToDevice, c->stream));
        PFP_HIP(c, hipMemcpyAsync(flg.data<uint32_t>(), flag, n * 4, hipMemcpyHostToDevice, c->stream));
    }
    PFP_TRY(device_compact(c, in ? (const uint32_t *)src.data<uint32_t>() : nullptr, (const uint32_t *)flg.data<uint32_t>(), n, dst.data<uint32_t>(), pos.data<uint32_t>(), cnt.data<uint32_t>()));
    if (n) PFP_HIP(c, hipMemcpyAsync(out, dst.data<uint32_t>(), n * 4, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipMemcpyAsync(count, cnt.data<uint32_t>(), 4, hipMemcpyDeviceToHost, c->stream));
    PFP_TRY(guards_check(c, src, changed)); PFP_TRY(guards_check(c, flg, changed)); PFP_TRY(guards_check(c, dst, changed));
    PFP_TRY(guards_check(c, pos, changed)); PFP_TRY(guards_check(c, cnt, changed));
    return PFP_OK;
}
// the arena of the context, emptied, for one call of a primitive on n elements
static int debug_prims_begin(pfp_ctx *c, uint64_t n)
{
    PFP_HIP(c, hipSetDevice(c->device));
    PFP_TRY(ensure_arena(c, n));
    c->arena.reset(); c->stage = 0;
    return PFP_OK;
}
} // namespace pfp

extern "C" {

int pfp_debug_checksum(pfp_ctx *c, const void *d_buf, uint64_t bytes, uint64_t global_offset, uint64_t out[2])
{
    if (!c || (!d_buf && bytes) || !out) return PFP_E_ARG;
    PFP_HIP(c, hipSetDevice(c->device));
    DevCounters<2> cnt; unsigned long long *d_out; PFP_TRY(cnt.open(c, &d_out));
    const uint64_t per = (uint64_t)1 << 34;            // pieces of 16 GiB keep the grid below 2^31 workgroups
    for (uint64_t off = 0; off < bytes; off += per) {
        const uint64_t nb = bytes - off < per ? bytes - off : per;
        PFP_LAUNCH(c, K_MISC, nb, k_checksum, nblocks(nb, 16 * BLOCK), (const uint8_t *)d_buf + off, nb, global_offset + off, d_out);
    }
    PFP_TRY(cnt.fetch(c));
    out[0] = cnt.h[0]; out[1] = cnt.h[1];
    return PFP_OK;
}
int pfp_debug_wordsum(pfp_ctx *c, const void *d_buf, uint64_t bytes, uint64_t out[2])
{
    if (!c || (!d_buf && bytes) || !out) return PFP_E_ARG;
    PFP_HIP(c, hipSetDevice(c->device));
    DevCounters<2> cnt; unsigned long long *d_out; PFP_TRY(cnt.open(c, &d_out));
    if (bytes) PFP_LAUNCH(c, K_MISC, bytes, k_wordsum, 4096, (const uint8_t *)d_buf, bytes, d_out);
    PFP_TRY(cnt.fetch(c));
    out[0] = cnt.h[0]; out[1] = cnt.h[1];
    return PFP_OK;
}
int pfp_debug_check_sample_order(pfp_ctx *c, uint64_t out[5])
{
    if (!c || !out) return PFP_E_ARG;
    if (c->stage < 3 || !c->d_ssa || !c->d_esa || !c->tb || c->tb_n != c->n || c->slice_rows != c->nout) return PFP_E_STATE;      // needs the text and the whole output's samples
    PFP_HIP(c, hipSetDevice(c->device));
    DevCounters<5> cnt; unsigned long long *d_out; PFP_TRY(cnt.open(c, &d_out));
    const uint64_t r = c->runs;
    if (r > 1) {
        if (c->flags & PFP_FLAG_U64) PFP_LAUNCH(c, K_MISC, r * 64, (k_check_sample_order<uint64_t>), nblocks(r, BLOCK), (const uint8_t *)c->tb + 16, c->n, (const uint64_t *)c->d_ssa, (const uint64_t *)c->d_esa, r, d_out);
        else PFP_LAUNCH(c, K_MISC, r * 64, (k_check_sample_order<uint32_t>), nblocks(r, BLOCK), (const uint8_t *)c->tb + 16, c->n, (const uint32_t *)c->d_ssa, (const uint32_t *)c->d_esa, r, d_out);
    }
    PFP_TRY(cnt.fetch(c));
    for (int i = 0; i < 5; ++i) out[i] = cnt.h[i];
    return PFP_OK;
}
int pfp_debug_check_sa(pfp_ctx *c, uint64_t out[5])
{
    if (!c || !out) return PFP_E_ARG;
    if (c->stage < 3 || !c->d_sa || !c->have_sa || !c->d_bwt || !c->tb || c->tb_n != c->n || c->slice_rows != c->nout) return PFP_E_STATE;      // needs the text and the whole SA
    PFP_HIP(c, hipSetDevice(c->device));
    const uint64_t rows = c->nout, words = (c->n + 32) / 32 + 1;
    DevCounters<5> cnt; unsigned long long *d_out; PFP_TRY(cnt.open(c, &d_out));
    uint32_t *seen = nullptr;
    struct DevFree { uint32_t *&p; ~DevFree() { if (p) (void)hipFree(p); } } seen_guard{seen};
    PFP_HIP(c, hipMalloc((void **)&seen, words * 4));
    PFP_HIP(c, hipMemsetAsync(seen, 0, words * 4, c->stream));
    if (c->flags & PFP_FLAG_U64) PFP_LAUNCH(c, K_MISC, rows * 10, (k_check_sa<uint64_t>), nblocks(rows, BLOCK), (const uint8_t *)c->tb + 16, c->n, (const uint64_t *)c->d_sa, (const uint8_t *)c->d_bwt, rows, seen, d_out);
    else PFP_LAUNCH(c, K_MISC, rows * 6, (k_check_sa<uint32_t>), nblocks(rows, BLOCK), (const uint8_t *)c->tb + 16, c->n, (const uint32_t *)c->d_sa, (const uint8_t *)c->d_bwt, rows, seen, d_out);
    PFP_TRY(cnt.fetch(c));
    out[0] = rows; for (int i = 1; i < 5; ++i) out[i] = cnt.h[i];
    return PFP_OK;
}
int pfp_debug_check_samples(pfp_ctx *c, uint64_t out[3])
{
    if (!c || !out) return PFP_E_ARG;
    if (c->stage < 3 || !c->d_sa || !c->have_sa || !c->have_rssa || !c->d_ssa || !c->d_esa || c->slice_rows != c->nout || c->esa_pairs != c->runs) return PFP_E_STATE;
    PFP_HIP(c, hipSetDevice(c->device));
    DevCounters<3> cnt; unsigned long long *d_out; PFP_TRY(cnt.open(c, &d_out));
    const uint64_t r = c->runs;
    if (r) {
        if (c->flags & PFP_FLAG_U64) PFP_LAUNCH(c, K_MISC, r * 50, (k_check_samples<uint64_t>), nblocks(r, BLOCK), (const uint64_t *)c->d_ssa, (const uint64_t *)c->d_esa, r, (const uint64_t *)c->d_sa, (const uint8_t *)c->d_bwt, c->nout, d_out);
        else PFP_LAUNCH(c, K_MISC, r * 30, (k_check_samples<uint32_t>), nblocks(r, BLOCK), (const uint32_t *)c->d_ssa, (const uint32_t *)c->d_esa, r, (const uint32_t *)c->d_sa, (const uint8_t *)c->d_bwt, c->nout, d_out);
    }
    PFP_TRY(cnt.fetch(c));
    out[0] = r; out[1] = cnt.h[1]; out[2] = cnt.h[2];
    return PFP_OK;
}
int pfp_debug_sort(pfp_ctx *c, uint64_t n, int bits, int reps, double *ms_out, uint32_t *unsorted_pairs, uint32_t *wrong_values)
{
    if (!c || n < 2 || n > 0xFFFFFFFFULL || bits < 1 || bits > 64 || reps < 1) return PFP_E_ARG;
    PFP_HIP(c, hipSetDevice(c->device));
    PFP_TRY(ensure_arena(c, n));
    c->arena.reset(); c->stage = 0;
    uint64_t *k0, *k1; uint32_t *v0, *v1, *d_bad;
    PFP_ALLOC_HI(c, k0, uint64_t, n); PFP_ALLOC_HI(c, k1, uint64_t, n); PFP_ALLOC_HI(c, v0, uint32_t, n); PFP_ALLOC_HI(c, v1, uint32_t, n); PFP_ALLOC_HI(c, d_bad, uint32_t, 2);
    BitRange br = {0, bits};
    double best = 1e30;
    uint64_t *sk = k0; uint32_t *sv = v0;
    for (int r = 0; r < reps; ++r) {
        PFP_LAUNCH(c, K_MISC, n * 12, k_debug_fill, nblocks(n, BLOCK), k0, v0, n, bits, (uint64_t)r * 7919);
        PFP_HIP(c, hipStreamSynchronize(c->stream));
        HostTimer t;
        int rc = radix_sort_pairs<uint64_t>(c, k0, v0, k1, v1, n, &br, 1, &sk, &sv);
        if (rc != PFP_OK) return rc;
        PFP_HIP(c, hipStreamSynchronize(c->stream));
        const double ms = t.ms();
        if (ms < best) best = ms;
    }
    PFP_HIP(c, hipMemsetAsync(d_bad, 0, 8, c->stream));
    PFP_LAUNCH(c, K_MISC, n * 12, k_debug_check_sorted, nblocks(n, BLOCK), (const uint64_t *)sk, (const uint32_t *)sv, n, bits, (uint64_t)(reps - 1) * 7919, d_bad);
    uint32_t bad[2] = {0, 0};
    PFP_HIP(c, hipMemcpyAsync(bad, d_bad, 8, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    if (ms_out) *ms_out = best;
    if (unsorted_pairs) *unsorted_pairs = bad[0];
    if (wrong_values) *wrong_values = bad[1];
    c->arena.reset();
    return PFP_OK;
}

int pfp_debug_prims_geometry(uint32_t out[4])
{
    if (!out) return PFP_E_ARG;
    out[0] = (uint32_t)RS_TILE; out[1] = (uint32_t)SCAN_TILE; out[2] = SEG_SMALL_MAX; out[3] = (uint32_t)Tunables().seg_grid;
    return PFP_OK;
}
int pfp_debug_emit_large_groups(pfp_ctx *c, uint64_t out[4])
{
    if (!c || !out) return PFP_E_ARG;
    out[0] = out[1] = 0; out[2] = (uint64_t)EG1_BUF; out[3] = (uint64_t)EG2_BUF;
    if (!c->d_lgtaken) return PFP_OK;      // no emission of this context has had the lists yet
    PFP_HIP(c, hipSetDevice(c->device));
    unsigned long long h[2];
    PFP_HIP(c, hipMemcpyAsync(h, c->d_lgtaken, 16, hipMemcpyDeviceToHost, c->stream));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    out[0] = h[0]; out[1] = h[1];
    return PFP_OK;
}
int pfp_debug_sort_pairs(pfp_ctx *c, const void *keys, int key_bytes, const uint32_t *vals, uint64_t n, const int *ranges, int nranges, void *keys_out, uint32_t *vals_out, uint32_t *guards_changed)
{
    if (!c || (key_bytes != 4 && key_bytes != 8) || nranges < 0 || nranges > 16 || (nranges && !ranges) || !guards_changed || (n && (!keys || !vals || !keys_out || !vals_out))) return PFP_E_ARG;
    BitRange br[16];
    for (int r = 0; r < nranges; ++r) { br[r].lo = ranges[2 * r]; br[r].hi = ranges[2 * r + 1]; if (br[r].lo < 0 || br[r].hi > 8 * key_bytes || br[r].lo > br[r].hi) return PFP_E_ARG; }
    PFP_TRY(debug_prims_begin(c, n));
    *guards_changed = 0;
    const int rc = key_bytes == 8 ? debug_sort_pairs<uint64_t>(c, (const uint64_t *)keys, vals, n, br, nranges, (uint64_t *)keys_out, vals_out, guards_changed)
                                  : debug_sort_pairs<uint32_t>(c, (const uint32_t *)keys, vals, n, br, nranges, (uint32_t *)keys_out, vals_out, guards_changed);
    c->arena.reset();
    return rc;
}
int pfp_debug_scan(pfp_ctx *c, const void *in, int elem_bytes, int op, int mode, uint64_t n, void *out, void *total, uint32_t *guards_changed)
{
    if (!c || (elem_bytes != 4 && elem_bytes != 8) || (op != 0 && op != 1) || mode < 0 || mode > 2 || !guards_changed || (n && (!in || !out))) return PFP_E_ARG;
    PFP_TRY(debug_prims_begin(c, n));
    *guards_changed = 0;
    int rc;
    if (elem_bytes == 8) rc = op == 0 ? debug_scan<uint64_t, 0>(c, (const uint64_t *)in, mode, n, (uint64_t *)out, (uint64_t *)total, guards_changed)
                                      : debug_scan<uint64_t, 1>(c, (const uint64_t *)in, mode, n, (uint64_t *)out, (uint64_t *)total, guards_changed);
    else rc = op == 0 ? debug_scan<uint32_t, 0>(c, (const uint32_t *)in, mode, n, (uint32_t *)out, (uint32_t *)total, guards_changed)
                      : debug_scan<uint32_t, 1>(c, (const uint32_t *)in, mode, n, (uint32_t *)out, (uint32_t *)total, guards_changed);
    c->arena.reset();
    return rc;
}
int pfp_debug_compact(pfp_ctx *c, const uint32_t *in, const uint32_t *flag, uint64_t n, uint32_t *out, uint32_t *count, uint32_t *guards_changed)
{
    if (!c || !count || !guards_changed || (n && (!flag || !out))) return PFP_E_ARG;
    PFP_TRY(debug_prims_begin(c, n));
    *guards_changed = 0;
    const int rc = debug_compact(c, in, flag, n, out, count, guards_changed);
    c->arena.reset();
    return rc;
}

} // extern "C"
