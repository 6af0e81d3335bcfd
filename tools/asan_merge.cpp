// tools/asan_merge.cpp -- the shard paths of pfbwt-f_amd/csrc/parse_host.h (pfp_shard_load, pfp_merge_shards, pfp_bwt_load and the
// stages of the parse they share) under AddressSanitizer + UBSan: a stand-alone program that includes the engine interpreted on the
// CPU (tests/emu) and uses only the public ABI.  A panel of four haplotypes of 3000 bases and two records short enough to be shards of
// one phrase, (w, p) = (4, 7) and (10, 100), both widths: parsed once whole, then parsed and merged as 2 and as 4 shards -- with left
// context, stand-alone, and re-loaded through pfp_shard_load from each shard's own pfp_parse_get image --, each with full and with
// compact views; behind every merge pfp_parse_bwt, and pfp_bwt_load from the merged arrays followed by a build.  Every variant must
// give the arrays of the whole parse; those are written to the file named on the command line, and the same source built without the
// sanitizers must write the same bytes:
//
//   F="-O1 -g -std=c++17 -x c++ -Itests/emu -DPFP_BACKEND_NAME=\"cpu-emu-TEST-ONLY\" -Wno-unused-function"
//   g++ $F -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o tests/emu/build/asan_merge tools/asan_merge.cpp -lz -lpthread
//   g++ $F -o tests/emu/build/plain_merge tools/asan_merge.cpp -lz -lpthread
//   ASAN_OPTIONS=detect_leaks=0 tests/emu/build/asan_merge /tmp/a.bin && tests/emu/build/plain_merge /tmp/b.bin && cmp /tmp/a.bin /tmp/b.bin
#include "../pfbwt-f_amd/csrc/pfbwt_hip.hip"
#include <string>

static void put(FILE *f, const void *p, size_t bytes) { const uint64_t n = bytes; fwrite(&n, 8, 1, f); if (bytes) fwrite(p, 1, bytes, f); }

struct Rng { uint64_t s; uint32_t next() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(s >> 33); } uint32_t below(uint32_t k) { return next() % k; } };

// four haplotypes (a random sequence and copies with a substitution every ~60 bases), a record of 12 bases and one of 1 base
static std::vector<std::string> panel()
{
    Rng r = {41};
    std::string base;
    for (int i = 0; i < 3000; ++i) base += "ACGT"[r.below(4)];
    std::vector<std::string> hap(4, base);
    for (int h = 1; h < 4; ++h) for (size_t i = r.below(60); i < base.size(); i += 1 + r.below(120)) hap[(size_t)h][i] = "ACGT"[r.below(4)];
    return {hap[0], hap[1], base.substr(100, 12), hap[2], "G", hap[3]};
}

// the arrays of stage 1 and 2 of a context: dict, occ, parse, last, sai, bwlast, ilist, bwsai
struct Arrays {
    pfp_parse_sizes ps; std::vector<uint8_t> a[8];
    bool operator==(const Arrays &o) const { for (int k = 0; k < 8; ++k) if (a[k] != o.a[k]) return false; return ps.n == o.ps.n && ps.m == o.ps.m && ps.dwords == o.ps.dwords && ps.dsize == o.ps.dsize; }
};
static bool fetch(pfp_ctx *c, const pfp_parse_sizes &ps, size_t U, Arrays *out)
{
    out->ps = ps;
    auto *a = out->a;
    a[0].resize(ps.dsize); a[1].resize(ps.dwords * U); a[2].resize(ps.m * 4); a[3].resize(ps.m); a[4].resize(ps.m * U);
    a[5].resize(ps.m + 1); a[6].resize((ps.m + 1) * U); a[7].resize((ps.m + 1) * U);
    return pfp_parse_get(c, a[0].data(), a[1].data(), (uint32_t *)a[2].data(), a[3].data(), a[4].data()) == PFP_OK && pfp_parse_bwt(c) == PFP_OK &&
           pfp_parse_bwt_get(c, a[5].data(), a[6].data(), a[7].data()) == PFP_OK;
}
// .bwt and SA of a build from the files of stage 2 (pfp_bwt_load)
static bool build_from(const Arrays &x, int w, uint64_t p, unsigned flags, size_t U, std::vector<uint8_t> *bwt, std::vector<uint8_t> *sa)
{
    int st = 0;
    pfp_ctx *c = pfp_create(w, p, flags, 0, 0, &st);
    if (!c) return false;
    pfp_bwt_sizes bs;
    bool ok = pfp_bwt_load(c, x.a[0].data(), x.ps.dsize, x.a[1].data(), x.ps.dwords, x.a[5].data(), x.a[6].data(), x.a[7].data(), x.ps.m + 1, x.ps.n) == PFP_OK && pfp_bwt_build(c, 1, 0, &bs) == PFP_OK;
    if (ok) { bwt->resize(bs.nout); sa->resize(bs.nout * U); ok = pfp_bwt_get(c, bwt->data(), sa->data(), nullptr, nullptr) == PFP_OK; }
    pfp_destroy(c);
    return ok;
}

enum Mode { CONTEXT, STANDALONE, LOADED };
static const char *const mode_names[] = {"context", "standalone", "loaded"};

static bool merged(const std::vector<std::string> &seqs, const std::vector<std::vector<int>> &shards, int w, uint64_t p, unsigned flags, size_t U, Mode mode, bool compact, Arrays *out)
{
    std::vector<pfp_ctx *> ctx; std::vector<pfp_shard_view> views;
    bool ok = true; int st = 0;
    for (size_t r = 0; ok && r < shards.size(); ++r) {
        pfp_ctx *c = pfp_create(w, p, flags, 0, 0, &st);
        if (!c) { ok = false; break; }
        ctx.push_back(c);
        if (r > 0 && mode == CONTEXT) ok = ok && pfp_parse_feed_left_context(c) == PFP_OK;
        for (int i : shards[r]) ok = ok && pfp_parse_feed(c, (const uint8_t *)seqs[(size_t)i].data(), seqs[(size_t)i].size(), 1) == PFP_OK;
        pfp_parse_sizes ps;
        if (mode == LOADED) {      // the shard's own .dict / .parse images, loaded into the context they came from
            ok = ok && pfp_parse_finalize(c, &ps) == PFP_OK;
            std::vector<uint8_t> dict; std::vector<uint32_t> parse;
            if (ok) { dict.resize(ps.dsize); parse.resize(ps.m); }
            ok = ok && pfp_parse_get(c, dict.data(), nullptr, parse.data(), nullptr, nullptr) == PFP_OK && pfp_shard_load(c, dict.data(), dict.size(), parse.data(), parse.size()) == PFP_OK;
        } else ok = ok && (((shards.size() + r) & 1) ? pfp_parse_finalize_shard(c, &ps) : pfp_parse_finalize(c, &ps)) == PFP_OK;
        pfp_shard_view v;
        ok = ok && pfp_shard_view_get(c, &v) == PFP_OK;
        if (ok && compact) v.d_ye = nullptr, v.d_last = nullptr;
        views.push_back(v);
    }
    pfp_ctx *g = ok ? pfp_create(w, p, flags, 0, 0, &st) : nullptr;
    pfp_parse_sizes ps;
    ok = ok && g && pfp_merge_shards(g, (int)views.size(), views.data(), &ps) == PFP_OK && fetch(g, ps, U, out);
    if (g) pfp_destroy(g);
    for (pfp_ctx *c : ctx) pfp_destroy(c);
    return ok;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s OUTPUT\n", argv[0]); return 2; }
    setenv("PFP_EMU_POISON", "1", 1);
    FILE *f = fopen(argv[1], "wb");
    if (!f) { perror(argv[1]); return 2; }
    const std::vector<std::string> seqs = panel();
    const std::vector<std::vector<int>> two = {{0, 1, 2}, {3, 4, 5}}, four = {{0, 1}, {2}, {3}, {4, 5}};
    const struct { int w; uint64_t p; } wp[] = {{4, 7}, {10, 100}};
    int bad = 0;
    for (const auto &q : wp) for (int wide = 0; wide < 2; ++wide) {
        const size_t U = wide ? 8 : 4;
        const unsigned flags = (wide ? PFP_FLAG_U64 : 0) | PFP_FLAG_SAI;
        int st = 0;
        pfp_ctx *c = pfp_create(q.w, q.p, flags, 0, 0, &st);
        if (!c) { ++bad; continue; }
        bool ok = true;
        for (const std::string &s : seqs) ok = ok && pfp_parse_feed(c, (const uint8_t *)s.data(), s.size(), 1) == PFP_OK;
        pfp_parse_sizes ps; Arrays whole;
        ok = ok && pfp_parse_finalize(c, &ps) == PFP_OK && fetch(c, ps, U, &whole);
        std::vector<uint8_t> bwt, sa;
        pfp_bwt_sizes bs;
        ok = ok && pfp_bwt_build(c, 1, 0, &bs) == PFP_OK;
        if (ok) { bwt.resize(bs.nout); sa.resize(bs.nout * U); ok = pfp_bwt_get(c, bwt.data(), sa.data(), nullptr, nullptr) == PFP_OK; }
        pfp_destroy(c);
        if (!ok) { printf("w = %d, p = %llu, U = %zu: the whole parse FAILED\n", q.w, (unsigned long long)q.p, U); ++bad; continue; }
        for (int k = 0; k < 8; ++k) put(f, whole.a[k].data(), whole.a[k].size());
        put(f, &whole.ps, sizeof whole.ps); put(f, bwt.data(), bwt.size()); put(f, sa.data(), sa.size());
        printf("w = %d, p = %llu, U = %zu: n = %llu, m = %llu, %llu words, r = %llu\n", q.w, (unsigned long long)q.p, U, (unsigned long long)ps.n, (unsigned long long)ps.m, (unsigned long long)ps.dwords, (unsigned long long)bs.r);
        for (const auto *shards : {&two, &four}) for (int mode = 0; mode < 3; ++mode) for (int compact = 0; compact < 2; ++compact) {
            Arrays got; std::vector<uint8_t> bwt2, sa2;
            const bool same = merged(seqs, *shards, q.w, q.p, flags, U, (Mode)mode, compact != 0, &got) && got == whole && build_from(got, q.w, q.p, flags, U, &bwt2, &sa2) && bwt2 == bwt && sa2 == sa;
            printf("  %zu shards, %s, %s views: %s\n", shards->size(), mode_names[mode], compact ? "compact" : "full", same ? "same arrays" : "FAILED");
            bad += !same;
        }
    }
    fclose(f);
    printf(bad ? "asan_merge: %d FAILED\n" : "asan_merge: all variants agree\n", bad);
    return bad != 0;
}
