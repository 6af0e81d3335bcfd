// tools/asan_markerquery.cpp -- marker index and queries (pfp_mk_index / pfp_mk_query: pfbwt-f_amd/csrc/markerquery.h and their host
// side in queries.h) under AddressSanitizer + UBSan: a stand-alone program that includes the engine interpreted on the CPU
// (tests/emu) and runs a seeded collection of 40 records at both widths.  The wide build keeps its SA: the marker array is made on the
// device from a seeded marker-positions stream and indexed where it lies; the narrow one has run samples only and indexes a
// hand-made stream from host memory -- a record every few rows, lists of 1 .. 70 markers with repeated values and bit 63.  Every
// mode (whole patterns, suffixes, suffixes with a cap) runs through both reductions and with chunks of 7 raw entries and of the
// default budget; every variant must give the arrays of the first; they are written to the file named on the command line, and
// the same source built without the sanitizers must write the same bytes.  A stream that is no marker array is refused in between:
//
//   F="-O1 -g -std=c++17 -x c++ -Itests/emu -DPFP_BACKEND_NAME=\"cpu-emu-TEST-ONLY\" -Wno-unused-function"
//   g++ $F -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o tests/emu/build/asan_markerquery tools/asan_markerquery.cpp -lz -lpthread
//   g++ $F -o tests/emu/build/plain_markerquery tools/asan_markerquery.cpp -lz -lpthread
//   ASAN_OPTIONS=detect_leaks=0 tests/emu/build/asan_markerquery /tmp/a.bin && tests/emu/build/plain_markerquery /tmp/b.bin && cmp /tmp/a.bin /tmp/b.bin
#include "../pfbwt-f_amd/csrc/pfbwt_hip.hip"
#include <string>

static void put(FILE *f, const void *p, size_t bytes) { const uint64_t n = bytes; fwrite(&n, 8, 1, f); if (bytes) fwrite(p, 1, bytes, f); }

struct Rng { uint64_t s; uint32_t next() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(s >> 33); } uint32_t below(uint32_t k) { return next() % k; } };

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s OUTPUT\n", argv[0]); return 2; }
    setenv("PFP_EMU_POISON", "1", 1);
    FILE *f = fopen(argv[1], "wb");
    if (!f) { perror(argv[1]); return 2; }
    const uint64_t DELIM = ~0ULL;
    int bad = 0;
    for (int wide = 0; wide < 2; ++wide) {
        const size_t U = wide ? 8 : 4;
        pfp_ctx *c = nullptr;
        std::vector<std::string> seqs;
        pfp_parse_sizes ps; pfp_bwt_sizes bs;
        bool ok = false;
        for (uint64_t seed = 1; seed < 200 && !ok; ++seed) {               // a text whose .bwt holds no EndOfWord byte (pfp_ri_index refuses the others)
            int st = 0;
            if (c) pfp_destroy(c);
            c = pfp_create(4, 5, (wide ? PFP_FLAG_U64 : 0) | PFP_FLAG_SAI, 0, 0, &st);
            if (!c) break;
            Rng r = {seed};
            seqs.clear();
            std::string base;
            for (int j = 0; j < 60; ++j) base += "ACGT"[r.below(4)];
            for (int i = 0; i < 40; ++i) { std::string s = base; for (int k = 0; k < 3; ++k) s[r.below(60)] = "ACGT"[r.below(4)]; seqs.push_back(s); }      // (a repetitive panel: long intervals)
            ok = true;
            for (const std::string &s : seqs) ok = ok && pfp_parse_feed(c, (const uint8_t *)s.data(), s.size(), 1) == PFP_OK;
            ok = ok && pfp_parse_finalize(c, &ps) == PFP_OK && pfp_parse_bwt(c) == PFP_OK && pfp_bwt_build(c, wide, 1, &bs) == PFP_OK && pfp_ri_index(c) == PFP_OK;
            if (ok) printf("U = %zu: seed %llu, n = %llu, r = %llu\n", U, (unsigned long long)seed, (unsigned long long)ps.n, (unsigned long long)bs.r);
        }
        if (!ok) { ++bad; if (c) pfp_destroy(c); continue; }
        const uint64_t n = ps.n;
        Rng r = {77};
        std::vector<uint64_t> stream;                                      // .mps (text positions) for the wide build, .ma (rows) for the narrow one: the same shape
        for (uint64_t at = 2 + r.below(5), k = 0; at + 12 < n; ++k) {
            const uint64_t len = 1 + r.below(9), nm = k % 9 == 4 ? 70 : 1 + r.below(4);
            stream.push_back(at); stream.push_back(at + len - 1);
            for (uint64_t m = 0; m < nm; ++m) stream.push_back((m % 5 == 3 ? 1ULL << 63 : 0) + 100 + (nm == 70 ? m / 2 : r.below(40)) + ((uint64_t)(m % 3) << 32));
            stream.push_back(DELIM);
            at += len + (k % 4 == 1 ? 0 : r.below(12));
        }
        pfp_mk_index_info ii;
        if (wide) {
            uint64_t words = 0;
            ok = pfp_mk_index(c, nullptr, 0, &ii) == PFP_E_STATE && pfp_marker_array(c, stream.data(), stream.size(), nullptr, 0, &words) == PFP_OK && words > 0 && pfp_mk_index(c, nullptr, 0, &ii) == PFP_OK;
        } else {
            stream.push_back(n - 1); stream.push_back(n); stream.push_back(5); stream.push_back(DELIM);      // a record that ends at row n
            std::vector<uint64_t> cut(stream.begin(), stream.end() - 1), swapped = stream;
            std::swap(swapped[0], swapped[1]); if (swapped[0] == swapped[1]) swapped[0] += 1;
            ok = pfp_mk_index(c, cut.data(), cut.size(), &ii) == PFP_E_CORRUPT && pfp_mk_index(c, swapped.data(), swapped.size(), &ii) == PFP_E_CORRUPT && pfp_mk_query(c, (const uint8_t *)"A", stream.data(), 0, 0, 0, nullptr) == PFP_E_STATE;
            ok = ok && pfp_mk_index(c, stream.data(), 0, &ii) == PFP_OK && ii.records == 0 && pfp_mk_index(c, stream.data(), stream.size(), &ii) == PFP_OK;
        }
        if (ok) printf("U = %zu: %llu records, %llu entries, %llu distinct, longest list %llu, %llu rows\n", U, (unsigned long long)ii.records, (unsigned long long)ii.entries, (unsigned long long)ii.distinct, (unsigned long long)ii.max_list, (unsigned long long)ii.rows);
        ok = ok && ii.max_list >= 35 && ii.records > 50;
        std::vector<std::string> pats = {"A", "C", "", "X", "AC", "GT", "ACG", seqs[3], seqs[7].substr(5, 30), seqs[11].substr(40), seqs[20].substr(0, 12) + "T" + seqs[20].substr(13, 20), "T", "G"};
        for (int i = 0; i < 270; ++i) { const std::string &s = seqs[r.below(40)]; const size_t a = r.below(50); pats.push_back(s.substr(a, 1 + r.below(20))); }
        std::string bases; std::vector<uint64_t> off(1, 0);
        for (const std::string &p : pats) { bases += p; off.push_back(bases.size()); }
        bases += '\0';                                                     // (never a NULL pointer)
        const uint64_t np = pats.size();
        const struct { uint64_t min_len, max_rows; } modes[] = {{0, 0}, {3, 0}, {2, 5}};
        const struct { const char *name; long long wave, chunk; } variants[] = {{"defaults", 64, 0}, {"chunks of 7", 64, 7}, {"sort", 0, 0}, {"sort, chunks of 7", 0, 7}, {"chunks of 1", 64, 1}};
        for (const auto &m : modes) {
            std::vector<uint8_t> first[5];                                  // cnt, probes, off, marker, freq
            for (const auto &v : variants) {
                ok = ok && pfp_debug_set(c, "mk_wave_max", v.wave) == PFP_OK && pfp_debug_set(c, "mk_chunk_entries", v.chunk) == PFP_OK;
                pfp_mk_info info;
                ok = ok && pfp_mk_query(c, (const uint8_t *)bases.data(), off.data(), np, m.min_len, m.max_rows, &info) == PFP_OK;
                if (!ok) break;
                std::vector<uint8_t> a[5];
                a[0].resize(np * U); a[1].resize(np * U); a[2].resize((np + 1) * 8); a[3].resize(info.entries * 8); a[4].resize(info.entries * 8);
                ok = pfp_mk_offsets_get(c, (uint64_t *)a[2].data(), nullptr) == PFP_OK && pfp_mk_get(c, a[0].data(), a[1].data(), (uint64_t *)a[3].data(), (uint64_t *)a[4].data()) == PFP_OK;
                if (!ok) break;
                if (first[2].empty()) {
                    for (int k = 0; k < 5; ++k) { first[k] = a[k]; put(f, a[k].data(), a[k].size()); }
                    printf("U = %zu, min_len %llu, max_rows %llu: %llu probes, %llu capped, %llu raw entries, %llu pairs, longest list %llu; wave %llu sort %llu\n", U, (unsigned long long)m.min_len, (unsigned long long)m.max_rows,
                           (unsigned long long)info.probes, (unsigned long long)info.capped, (unsigned long long)info.raw, (unsigned long long)info.entries, (unsigned long long)info.max_markers, (unsigned long long)info.by_wave, (unsigned long long)info.by_sort);
                    ok = info.by_wave > 0 && info.by_sort > 0 && info.entries > 100 && (!m.max_rows || info.capped > 0);
                } else {
                    for (int k = 0; k < 5; ++k) if (a[k] != first[k]) { printf("U = %zu, %s: array %d DIFFERS\n", U, v.name, k); ok = false; }
                    if (v.chunk && info.chunks < 10) { printf("%s: %llu chunks\n", v.name, (unsigned long long)info.chunks); ok = false; }
                    if (!v.wave && info.by_wave) ok = false;
                }
                printf("U = %zu, min_len %llu, max_rows %llu, %s: %s\n", U, (unsigned long long)m.min_len, (unsigned long long)m.max_rows, v.name, ok ? "same arrays" : "FAILED");
            }
        }
        bad += !ok;
        pfp_destroy(c);
    }
    fclose(f);
    printf(bad ? "asan_markerquery: %d FAILED\n" : "asan_markerquery: all variants agree\n", bad);
    return bad != 0;
}
