// tools/asan_emit_large.cpp -- the emission of the long groups (k_emit_groups_large, pfbwt-f_amd/csrc/emit.h, and its host side in
// emit_host.h) under AddressSanitizer + UBSan: a stand-alone program that includes the engine interpreted on the CPU (tests/emu) and
// builds the H = 16384 panel of tests/test_emit_large_groups.py -- copies of one 40-base sequence with three sites changed in a
// fixed half of the copies: full buffers of both instantiations -- at both widths of the text positions, with 32- and 64-bit row
// counters, BWT + run samples in one build and in three slices.  It writes every array to the file named on the command line; the
// same source built without the sanitizers must write the same bytes:
//
//   F="-O1 -g -std=c++17 -x c++ -Itests/emu -DPFP_BACKEND_NAME=\"cpu-emu-TEST-ONLY\" -Wno-unused-function"
//   g++ $F -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o tests/emu/build/asan_emit_large tools/asan_emit_large.cpp -lz -lpthread
//   g++ $F -o tests/emu/build/plain_emit_large tools/asan_emit_large.cpp -lz -lpthread
//   ASAN_OPTIONS=detect_leaks=0 tests/emu/build/asan_emit_large /tmp/a.bin && tests/emu/build/plain_emit_large /tmp/b.bin && cmp /tmp/a.bin /tmp/b.bin
#include "../pfbwt-f_amd/csrc/pfbwt_hip.hip"
#include <string>

static void put(FILE *f, const void *p, size_t bytes) { const uint64_t n = bytes; fwrite(&n, 8, 1, f); if (bytes) fwrite(p, 1, bytes, f); }

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s OUTPUT [COPIES]\n", argv[0]); return 2; }
    setenv("PFP_EMU_POISON", "1", 1);
    const uint32_t H = argc > 2 ? (uint32_t)atoi(argv[2]) : 16384u;
    const std::string base = "TTTTATTCACTTGGTATTATTCGTTCGCCTGCTGTATTGC";
    const auto next = [](char ch) { const std::string a = "ACGT"; return a[(a.find(ch) + 1) % 4]; };
    FILE *f = fopen(argv[1], "wb");
    if (!f) { perror(argv[1]); return 2; }
    int bad = 0;
    for (int wide = 0; wide < 2; ++wide) {
        int st = 0;
        pfp_ctx *c = pfp_create(6, 13, (wide ? PFP_FLAG_U64 : 0) | PFP_FLAG_SAI, 0, 0, &st);
        bool ok = c != nullptr;
        for (uint32_t h = 0; ok && h < H; ++h) {
            std::string s = base;
            if (h < H / 2) { s[9] = next(base[9]); s[22] = next(base[22]); }
            if (h % 2 == 0) s[25] = next(base[25]);
            ok = pfp_parse_feed(c, (const uint8_t *)s.data(), s.size(), 1) == PFP_OK;
        }
        pfp_parse_sizes ps; pfp_bwt_sizes bs;
        ok = ok && pfp_parse_finalize(c, &ps) == PFP_OK && pfp_parse_bwt(c) == PFP_OK;
        const size_t U = wide ? 8 : 4;
        for (int fw = 0; ok && fw < 2; ++fw) {
            ok = pfp_debug_set(c, "force_wide_rows", fw) == PFP_OK && pfp_bwt_build(c, 0, 1, &bs) == PFP_OK;
            uint64_t g[4] = {0, 0, 0, 0};
            ok = ok && pfp_debug_emit_large_groups(c, g) == PFP_OK;
            std::vector<uint8_t> bwt(ok ? bs.nout : 0), ssa(ok ? 2 * bs.r * U : 0), esa(ok ? 2 * bs.r * U : 0);
            ok = ok && pfp_bwt_get(c, bwt.data(), nullptr, ssa.data(), esa.data()) == PFP_OK;
            if (H == 16384u) ok = ok && g[0] > 0 && g[1] > 0;      // both instantiations ran (the counts themselves: tests/test_emit_large_groups.py)
            put(f, bwt.data(), bwt.size()); put(f, ssa.data(), ssa.size()); put(f, esa.data(), esa.size()); put(f, &bs.r, 8);
            printf("U = %zu, force_wide_rows %d: %s (n = %llu, r = %llu, groups taken %llu + %llu)\n", U, fw, ok ? "built" : "FAILED", ok ? (unsigned long long)ps.n : 0ULL, ok ? (unsigned long long)bs.r : 0ULL,
                   (unsigned long long)g[0], (unsigned long long)g[1]);
            for (int sl = 0; ok && sl < 3; ++sl) {
                uint64_t beg = 0, rows = 0, pairs = 0;
                ok = pfp_bwt_build_slice(c, 0, 1, sl, 3, &bs, &beg, &rows, &pairs) == PFP_OK;
                std::vector<uint8_t> b(ok ? rows : 0), s(ok ? 2 * bs.r * U : 0), e(ok ? 2 * pairs * U : 0);
                ok = ok && pfp_bwt_get(c, b.data(), nullptr, s.data(), e.data()) == PFP_OK;
                put(f, b.data(), b.size()); put(f, s.data(), s.size()); put(f, e.data(), e.size()); put(f, &bs.r, 8);
            }
        }
        bad += !ok;
        if (c) pfp_destroy(c);
    }
    fclose(f);
    printf(bad ? "asan_emit_large: %d FAILED\n" : "asan_emit_large: all built\n", bad);
    return bad != 0;
}
