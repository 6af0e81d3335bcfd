// tools/asan_recsort.cpp -- the host code of the two recursive sorts (pfbwt-f_amd/csrc/recsort.h, dictrec.h) under AddressSanitizer +
// UBSan: a stand-alone program that includes the engine interpreted on the CPU (tests/emu) and runs the sacak_int drop-in on two
// repetitive panels, full and 5-row batches, and whole builds of tests/golden/w4p7: the parse's assembly by either route
// (PFP_PARSE_REC_MERGE 0 / 1 / 2), then the dictionary through its own level-2 parse (PFP_DICT_REC=1), alone and together with
// PFP_PARSE_REC=1, full and 5-row batches.  Every suffix array of a panel is checked by comparing neighbouring suffixes; the routes
// and the builds must agree byte for byte.
//
//   g++ -O1 -g -std=c++17 -x c++ -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Itests/emu \
//       -DPFP_BACKEND_NAME='"cpu-emu-TEST-ONLY"' -Wno-unused-function -o tests/emu/build/asan_recsort tools/asan_recsort.cpp -lz -lpthread
//   ASAN_OPTIONS=detect_leaks=0 tests/emu/build/asan_recsort tests/golden/w4p7/input.fa
#include "../pfbwt-f_amd/csrc/pfbwt_hip.hip"
#include <fstream>
#include <string>

static uint64_t rng_state = 7;
static uint32_t rnd(uint32_t mod) { rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)((rng_state >> 33) % mod); }

static std::vector<uint32_t> panel(uint32_t L, uint32_t H, uint32_t sigma, uint32_t mut_per_1000)
{
    std::vector<uint32_t> base(L), s;
    for (auto &x : base) x = 1 + rnd(sigma - 1);
    for (uint32_t h = 0; h < H; ++h) for (uint32_t i = 0; i < L; ++i) s.push_back(rnd(1000) < mut_per_1000 ? 1 + rnd(sigma - 1) : base[i]);
    s.push_back(0);
    return s;
}
static bool sa_ok(const std::vector<uint32_t> &s, const std::vector<uint32_t> &SA)
{
    const size_t n = s.size();
    std::vector<char> seen(n, 0);
    for (size_t i = 0; i < n; ++i) { if (SA[i] >= n || seen[SA[i]]) return false; seen[SA[i]] = 1; }
    for (size_t i = 1; i < n; ++i) if (!std::lexicographical_compare(s.begin() + SA[i - 1], s.end(), s.begin() + SA[i], s.end())) return false;
    return true;
}

int main(int argc, char **argv)
{
    setenv("PFP_TEST_HOOKS", "1", 1); setenv("PFP_PARSE_REC", "1", 1); setenv("PFP_EMU_POISON", "1", 1);
    int bad = 0;
    const char *tiles[2] = {nullptr, "5"};
    const std::vector<uint32_t> in[2] = {panel(300, 20, 50, 20), panel(2000, 8, 5, 10)};
    const uint32_t sig[2] = {50, 5};
    for (int p = 0; p < 2; ++p)
        for (const char *tile : tiles) {
            if (tile) setenv("PFP_PARSE_REC_TILE_ROWS", tile, 1); else unsetenv("PFP_PARSE_REC_TILE_ROWS");
            std::vector<uint32_t> first;
            for (const char *merge : {"0", "1", "2"}) {
                setenv("PFP_PARSE_REC_MERGE", merge, 1);
                std::vector<uint32_t> SA(in[p].size());
                const int r = pfp_sacak_int_u32(in[p].data(), SA.data(), (uint32_t)in[p].size(), sig[p]);
                const bool ok = r >= 0 && sa_ok(in[p], SA) && (first.empty() || SA == first);
                if (first.empty()) first = SA;
                printf("panel %d tile %s merge %s: %s\n", p, tile ? tile : "full", merge, ok ? "ok" : "WRONG");
                bad += !ok;
            }
        }
    unsetenv("PFP_PARSE_REC_TILE_ROWS");
    if (argc > 1) {      // a FASTA file: whole build, BWT and SA equal by either route
        std::ifstream f(argv[1]);
        std::vector<std::string> recs; std::string line;
        while (std::getline(f, line)) { if (!line.empty() && line[0] == '>') recs.emplace_back(); else if (!recs.empty()) recs.back() += line; }
        std::vector<uint8_t> bwt0; std::vector<uint64_t> sa0;
        auto build = [&](const char *what, const char *val) {
            int st = 0;
            pfp_ctx *c = pfp_create(4, 7, PFP_FLAG_U64 | PFP_FLAG_SAI, 0, 0, &st);
            pfp_parse_sizes ps; pfp_bwt_sizes bs;
            bool ok = c != nullptr;
            for (auto &r : recs) ok = ok && pfp_parse_feed(c, (const uint8_t *)r.data(), r.size(), 1) == PFP_OK;
            ok = ok && pfp_parse_finalize(c, &ps) == PFP_OK && pfp_parse_bwt(c) == PFP_OK && pfp_bwt_build(c, 1, 0, &bs) == PFP_OK;
            std::vector<uint8_t> bwt(ok ? bs.nout : 0); std::vector<uint64_t> sa(ok ? bs.nout : 0);
            ok = ok && pfp_bwt_get(c, bwt.data(), sa.data(), nullptr, nullptr) == PFP_OK && (bwt0.empty() || (bwt == bwt0 && sa == sa0));
            if (bwt0.empty()) { bwt0 = bwt; sa0 = sa; }
            printf("%s %s %s: %s (n = %llu, r = %llu)\n", argv[1], what, val, ok ? "ok" : "WRONG", ok ? (unsigned long long)ps.n : 0ULL, ok ? (unsigned long long)bs.r : 0ULL);
            bad += !ok;
            if (c) pfp_destroy(c);
        };
        for (const char *merge : {"0", "1", "2"}) { setenv("PFP_PARSE_REC_MERGE", merge, 1); build("merge", merge); }
        unsetenv("PFP_PARSE_REC_MERGE");
        // the dictionary through its own level-2 parse (dictrec.h), alone and with the parse route behind it, full and 5-row batches
        setenv("PFP_DICT_REC", "1", 1);
        for (const char *tile : tiles) {
            if (tile) setenv("PFP_PARSE_REC_TILE_ROWS", tile, 1); else unsetenv("PFP_PARSE_REC_TILE_ROWS");
            for (const char *prec : {(const char *)nullptr, "1"}) {
                if (prec) setenv("PFP_PARSE_REC", prec, 1); else unsetenv("PFP_PARSE_REC");
                build(tile ? "dict_rec tile 5 parse_rec" : "dict_rec tile full parse_rec", prec ? prec : "default");
            }
        }
    }
    printf(bad ? "asan_recsort: %d FAILED\n" : "asan_recsort: all ok\n", bad);
    return bad != 0;
}
