// pfbwt-f_amd/csrc/gsacak_host.h -- drop-ins for gsa/gsacak.h:76-103 on the device: sacak_int (the suffix array of an integer string) and
// gsacak (suffix array, LCP and document array of a collection of strings; the call of include/pfbwt.hpp:211), each in the two widths of
// uint_t.  Every call makes a context of its own.  Included by pfbwt_hip.hip (ensure_arena, h2d_copy, the sorts of sufsort.h).
#pragma once

static int sacak_int_impl(const uint32_t *s, void *SA, uint64_t n, uint64_t k, bool u64)
{
    if (!s || !SA || n == 0) return -1;
    if (n + 64 >= 0xFFFFFFFFULL) return -1;
    int st = 0;
    pfp_ctx *c = pfp_create(10, 100, 0, 0, (uint64_t)(80 * n + (32ULL << 20)), &st);
    if (!c) return -1;
    int rounds = -1;
    do {
        if (ensure_arena(c, n) != PFP_OK) break;
        uint32_t *dS = (uint32_t *)c->arena.alloc_lo(n * 4), *dSA = (uint32_t *)c->arena.alloc_lo(n * 4), *dR = (uint32_t *)c->arena.alloc_lo(n * 4);
        if (!dS || !dSA || !dR) break;
        if (hipMemcpy(dS, s, n * 4, hipMemcpyHostToDevice) != hipSuccess) break;
        int r = 0;
        if (sort_int_suffixes(c, dS, n, k ? k - 1 : 0, dSA, dR, &r) != PFP_OK) break;
        if (hipStreamSynchronize(c->stream) != hipSuccess) break;
        if (!u64) { if (hipMemcpy(SA, dSA, n * 4, hipMemcpyDeviceToHost) != hipSuccess) break; }
        else {
            std::vector<uint32_t> tmp((size_t)n);
            if (hipMemcpy(tmp.data(), dSA, n * 4, hipMemcpyDeviceToHost) != hipSuccess) break;
            for (uint64_t i = 0; i < n; ++i) ((uint64_t *)SA)[i] = tmp[(size_t)i];
        }
        rounds = r;
    } while (0);
    pfp_destroy(c);
    return rounds;
}

// int gsacak(unsigned char *s, uint_t *SA, int_t *LCP, int_t *DA, uint_t n), gsa/gsacak.h:86-96 -- the call of
// include/pfbwt.hpp:211.  s = strings over any byte alphabet (the parser's dictionaries: '-', A, C, G, N, T and Dollar = 2), each
// followed by the separator 1, s[n-1] = 0.  Suffixes are compared up to their separator; suffixes that are byte-identical up to it
// are ordered by position (gsacak.c:877-912) and LCP stops at the separator (:64).
// LCP[i] of SA[i-1], SA[i]: bytes are compared eight at a time; inside runs of one byte (a 10 Mbp run of N is one phrase whose
// suffixes are neighbours in SA) the shorter of the two runs is skipped at once (M: run lengths, see k_ss_runend_marks)
template <typename LT> __global__ __launch_bounds__(BLOCK) void k_gsa_lcp(const uint8_t *D, const uint32_t *SA, const uint32_t *M, uint64_t n, LT *lcp)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    if (i == 0) { lcp[0] = 0; return; }
    const uint64_t x = SA[i - 1], y = SA[i];
    uint64_t h = 0;
    for (;;) {
        const uint64_t px = x + h, py = y + h;
        if (px >= n || py >= n) break;
        const uint8_t cx = D[px];
        if (cx != D[py] || cx <= EndOfWord) break;
        const uint32_t ix = (uint32_t)(n - 1 - px), iy = (uint32_t)(n - 1 - py);
        const uint64_t rx = ix - M[ix] + 1u, ry = iy - M[iy] + 1u;          // lengths of the runs of cx that start at px / py
        if (rx >= 16 && ry >= 16) { h += rx < ry ? rx : ry; continue; }
        const uint64_t a = ld8(D + px), b = ld8(D + py);                     // (the device buffer is padded)
        // first byte that differs or is a separator / terminator: bytes are < 0x80, so (v - 0x02..02) has its high bit set exactly for v <= 1
        const uint64_t stop = (a ^ b) | (((a - 0x0202020202020202ULL) & ~a & 0x8080808080808080ULL));
        if (stop) { h += (uint64_t)(__ffsll((long long)stop) - 1) >> 3; break; }
        h += 8;
    }
    lcp[i] = (LT)h;
}
template <typename LT> __global__ __launch_bounds__(BLOCK) void k_gsa_da(const uint32_t *SA, const uint32_t *wordid, uint64_t n, LT *da)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) da[i] = (LT)wordid[SA[i]];
}
// one output array of gsacak in the caller's width: n values at the high end of the arena, made by `launch`, fetched into host memory
template <typename LT, typename Launch> static int gsa_fetch(pfp_ctx *c, uint64_t n, void *host, Launch launch)
{
    LT *d; PFP_ALLOC_HI(c, d, LT, n);
    PFP_TRY(launch(d));
    PFP_HIP(c, hipStreamSynchronize(c->stream));
    PFP_HIP(c, hipMemcpy(host, d, n * sizeof(LT), hipMemcpyDeviceToHost));
    return PFP_OK;
}
static int gsacak_impl(const uint8_t *s, void *SA, void *LCP, void *DA, uint64_t n, bool u64)
{
    if (!s || !SA || n < 2) return -1;
    if (n + 64 >= 0xFFFFFFFFULL) return -1;
    // the alphabet: bytes 0 (terminator: only at the very end) and 1 (separator) keep their roles; every other byte that occurs gets
    // the next code in byte order.  The parser's own dictionaries ('-' A C G N T and Dollar) take the tuned 16-characters-per-key
    // kernel; any other byte set (another caller of gsa/gsacak.h:86-96) takes the generic one with as many characters as fit 51 bits
    bool seen[256] = {false};
    for (uint64_t i = 0; i < n; ++i) seen[s[i]] = true;
    if (s[n - 1] != 0) return -1;
    for (uint64_t i = 0; i + 1 < n; ++i) if (s[i] == 0) return -1;      // no unique terminator
    bool dict_alphabet = true;
    for (int b = 3; b < 256; ++b) if (seen[b] && !(b == '-' || b == 'A' || b == 'C' || b == 'G' || b == 'N' || b == 'T')) dict_alphabet = false;
    uint8_t code[256]; uint32_t sigma = 2;
    for (int b = 0; b < 256; ++b) code[b] = (uint8_t)(b <= 1 ? b : 0);
    for (int b = 2; b < 256; ++b) if (seen[b]) code[b] = (uint8_t)sigma++;
    uint32_t chars = 0; { unsigned __int128 v = 1; while (chars < 16 && v * sigma < ((unsigned __int128)1 << 51)) { v *= sigma; ++chars; } }
    int st = 0;
    pfp_ctx *c = pfp_create(10, 100, u64 ? PFP_FLAG_U64 : 0u, 0, (uint64_t)(72 * n + (64ULL << 20)), &st);
    if (!c) return -1;
    int rounds = -1;
    auto body = [&]() -> int {
        PFP_TRY(ensure_arena(c, n));
        c->arena.reset();
        c->dsize = n;
        PFP_ALLOC_LO(c, c->d_dict, uint8_t, n + 16);
        PFP_HIP(c, hipMemsetAsync(c->d_dict + n, 0, 16, c->stream));
        PFP_TRY(h2d_copy(c, c->d_dict, s, n));
        // sort_dict_suffixes with a counted round number
        uint64_t *k0, *k1; uint32_t *v0, *v1;
        PFP_ALLOC_LO(c, c->d_gsa, uint32_t, n); PFP_ALLOC_LO(c, c->d_grank, uint2, n);
        const size_t mk = c->arena.mark_hi();
        PFP_ALLOC_HI(c, k0, uint64_t, n); PFP_ALLOC_HI(c, k1, uint64_t, n); PFP_ALLOC_HI(c, v0, uint32_t, n); PFP_ALLOC_HI(c, v1, uint32_t, n);
        if (dict_alphabet) {
            PFP_LAUNCH(c, K_SS_INIT_KEYS, n * 13, k_dict_init_keys, nblocks(n, DK_TILE), (const uint8_t *)c->d_dict, n, k0, v0);
            BitRange full = {0, DK_KEY_BITS};
            PFP_TRY(suffix_sort_doubling<true>(c, n, k0, v0, k1, v1, &full, 1, DK_CHARS, c->d_dict, c->d_gsa, (uint32_t *)nullptr, c->d_grank, &rounds));
        } else {
            uint8_t *d_code; PFP_ALLOC_HI(c, d_code, uint8_t, 256);
            PFP_HIP(c, hipMemcpyAsync(d_code, code, 256, hipMemcpyHostToDevice, c->stream));
            PFP_HIP(c, hipStreamSynchronize(c->stream));
            PFP_LAUNCH(c, K_SS_INIT_KEYS, n * 13, k_dict_init_keys_any, nblocks(n, BLOCK), (const uint8_t *)c->d_dict, n, (const uint8_t *)d_code, sigma, chars, k0, v0);
            BitRange full = {0, 51};
            PFP_TRY(suffix_sort_doubling<true>(c, n, k0, v0, k1, v1, &full, 1, chars, c->d_dict, c->d_gsa, (uint32_t *)nullptr, c->d_grank, &rounds, sigma));
        }
        c->arena.release_hi(mk);
        PFP_HIP(c, hipStreamSynchronize(c->stream));
        if (!u64) PFP_HIP(c, hipMemcpy(SA, c->d_gsa, n * 4, hipMemcpyDeviceToHost));
        else PFP_TRY(download_as_u(c, c->d_gsa, n, SA, true));
        if (LCP) {
            uint32_t *M; PFP_ALLOC_HI(c, M, uint32_t, n);
            PFP_LAUNCH(c, K_MISC, n * 5, k_ss_runend_marks, nblocks(n, BLOCK), (const uint8_t *)c->d_dict, n, M);
            PFP_TRY((device_scan<uint32_t, 1>(c, M, M, n, nullptr)));
            if (u64) PFP_TRY(gsa_fetch<int64_t>(c, n, LCP, [&](int64_t *d) { PFP_LAUNCH(c, K_MISC, n * 40, (k_gsa_lcp<int64_t>), nblocks(n, BLOCK), (const uint8_t *)c->d_dict, (const uint32_t *)c->d_gsa, (const uint32_t *)M, n, d); return PFP_OK; }));
            else PFP_TRY(gsa_fetch<int32_t>(c, n, LCP, [&](int32_t *d) { PFP_LAUNCH(c, K_MISC, n * 36, (k_gsa_lcp<int32_t>), nblocks(n, BLOCK), (const uint8_t *)c->d_dict, (const uint32_t *)c->d_gsa, (const uint32_t *)M, n, d); return PFP_OK; }));
            c->arena.release_hi(mk);
        }
        if (DA) {   // document of every suffix = number of separators in front of it
            uint32_t *flag, *wid; PFP_ALLOC_HI(c, flag, uint32_t, n); PFP_ALLOC_HI(c, wid, uint32_t, n);
            PFP_LAUNCH(c, K_MISC, n * 5, k_eow_flags, nblocks(n, BLOCK), (const uint8_t *)c->d_dict, n, flag);
            PFP_TRY((device_scan<uint32_t, 0>(c, flag, wid, n, nullptr)));
            if (u64) PFP_TRY(gsa_fetch<int64_t>(c, n, DA, [&](int64_t *d) { PFP_LAUNCH(c, K_MISC, n * 16, (k_gsa_da<int64_t>), nblocks(n, BLOCK), (const uint32_t *)c->d_gsa, (const uint32_t *)wid, n, d); return PFP_OK; }));
            else PFP_TRY(gsa_fetch<int32_t>(c, n, DA, [&](int32_t *d) { PFP_LAUNCH(c, K_MISC, n * 12, (k_gsa_da<int32_t>), nblocks(n, BLOCK), (const uint32_t *)c->d_gsa, (const uint32_t *)wid, n, d); return PFP_OK; }));
            c->arena.release_hi(mk);
        }
        return PFP_OK;
    };
    const int rc = body();
    pfp_destroy(c);
    return rc == PFP_OK ? rounds : -1;
}

extern "C" {
int pfp_gsacak_u32(const uint8_t *s, uint32_t *SA, int32_t *LCP, int32_t *DA, uint32_t n) { return gsacak_impl(s, SA, LCP, DA, n, false); }
int pfp_gsacak_u64(const uint8_t *s, uint64_t *SA, int64_t *LCP, int64_t *DA, uint64_t n) { return gsacak_impl(s, SA, LCP, DA, n, true); }

int pfp_sacak_int_u32(const uint32_t *s, uint32_t *SA, uint32_t n, uint32_t k) { return sacak_int_impl(s, SA, n, k, false); }
int pfp_sacak_int_u64(const uint32_t *s, uint64_t *SA, uint64_t n, uint64_t k) { return sacak_int_impl(s, SA, n, k, true); }
} // extern "C"
