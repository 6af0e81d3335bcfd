// tools/asan_doclist.cpp -- document listing (pfp_ri_docs: pfbwt-f_amd/csrc/doclist.h and its host side in queries.h) under
// AddressSanitizer + UBSan: a stand-alone program that includes the engine interpreted on the CPU (tests/emu) and runs a panel of
// 300 short records like the one of tests/test_doclist.py -- every record with a tag, most with a prefix of one motif planted, one
// with a tandem repeat; as documents the records, and a document every 4 bytes and every byte (the larger tables of counters and
// of starts) -- at both widths, with and without a resident SA, through all three reduction routes (the defaults, the table
// switched off, wave and table switched off) and with chunks of 7 rows and of the default budget, with and without PFP_DL_INSIDE
// and with max_count.  Every variant must give the arrays of the first; they are written to the file named on the
// command line, and the same source built without the sanitizers must write the same bytes.  Behind the listings the other
// callers of the pattern batch they share run on the same patterns: pfp_ms_query, pfp_ri_locate by phi and from the SA,
// pfp_mem_find with locate on both routes; the routes must agree, nothing of it is written:
//
//   F="-O1 -g -std=c++17 -x c++ -Itests/emu -DPFP_BACKEND_NAME=\"cpu-emu-TEST-ONLY\" -Wno-unused-function"
//   g++ $F -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o tests/emu/build/asan_doclist tools/asan_doclist.cpp -lz -lpthread
//   g++ $F -o tests/emu/build/plain_doclist tools/asan_doclist.cpp -lz -lpthread
//   ASAN_OPTIONS=detect_leaks=0 tests/emu/build/asan_doclist /tmp/a.bin && tests/emu/build/plain_doclist /tmp/b.bin && cmp /tmp/a.bin /tmp/b.bin
#include "../pfbwt-f_amd/csrc/pfbwt_hip.hip"
#include <string>

static void put(FILE *f, const void *p, size_t bytes) { const uint64_t n = bytes; fwrite(&n, 8, 1, f); if (bytes) fwrite(p, 1, bytes, f); }

struct Rng { uint64_t s; uint32_t next() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(s >> 33); } uint32_t below(uint32_t k) { return next() % k; } };

static const std::string MOTIF = "GTCCGATAGCTT", TAG = "TGGCATTC";

// record i holds TAG once and, for i % 300 < planted[k], the prefix MOTIF[:k] followed by another base
static std::vector<std::string> panel(uint64_t seed)
{
    Rng r = {seed};
    const int ks[6] = {12, 10, 9, 8, 7, 6}, upto[6] = {1, 63, 64, 65, 256, 257};
    std::vector<std::string> out;
    for (int i = 0; i < 300; ++i) {
        int k = 0;
        for (int q = 0; q < 6 && !k; ++q) if (i < upto[q]) k = ks[q];
        std::string plant = k ? MOTIF.substr(0, (size_t)k) : "";
        if (k && k < 12) { char x; do x = "ACGT"[r.below(4)]; while (x == MOTIF[(size_t)k]); plant += x; }
        for (;;) {
            const size_t L = 24 + r.below(17), free = L - TAG.size() - plant.size(), cut = r.below((uint32_t)free + 1);
            std::string fill;
            for (size_t j = 0; j < free; ++j) fill += "ACGT"[r.below(4)];
            const std::string s = TAG + fill.substr(0, cut) + plant + fill.substr(cut);
            const bool clean = s.find(TAG, 1) == std::string::npos && s.find("AAAA") == std::string::npos && (k ? s.find(MOTIF.substr(0, 6), s.find(MOTIF.substr(0, 6)) + 1) : s.find(MOTIF.substr(0, 6))) == std::string::npos;
            if (clean) { out.push_back(s); break; }
        }
    }
    for (int j = 0; j < 80; ++j) out[150] += "AC";
    out[299] = out[298];                                                   // two equal records
    return out;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s OUTPUT\n", argv[0]); return 2; }
    setenv("PFP_EMU_POISON", "1", 1);
    FILE *f = fopen(argv[1], "wb");
    if (!f) { perror(argv[1]); return 2; }
    const int w = 4;
    int bad = 0;
    for (int wide = 0; wide < 2; ++wide) {
        const size_t U = wide ? 8 : 4;
        pfp_ctx *c = nullptr;
        std::vector<std::string> seqs;
        bool ok = false;
        for (uint64_t seed = 1; seed < 200 && !ok; ++seed) {               // a text whose .bwt holds no EndOfWord byte (pfp_ri_index refuses the others)
            int st = 0;
            if (c) pfp_destroy(c);
            c = pfp_create(w, 5, (wide ? PFP_FLAG_U64 : 0) | PFP_FLAG_SAI, 0, 0, &st);
            if (!c) break;
            seqs = panel(seed);
            ok = true;
            for (const std::string &s : seqs) ok = ok && pfp_parse_feed(c, (const uint8_t *)s.data(), s.size(), 1) == PFP_OK;
            pfp_parse_sizes ps; pfp_bwt_sizes bs;
            ok = ok && pfp_parse_finalize(c, &ps) == PFP_OK && pfp_parse_bwt(c) == PFP_OK && pfp_bwt_build(c, wide, 1, &bs) == PFP_OK && pfp_ri_index(c) == PFP_OK;
            if (ok) printf("U = %zu: seed %llu, n = %llu, r = %llu\n", U, (unsigned long long)seed, (unsigned long long)ps.n, (unsigned long long)bs.r);
        }
        if (!ok) { ++bad; if (c) pfp_destroy(c); continue; }
        std::vector<uint64_t> records;
        uint64_t at = 0;
        for (const std::string &s : seqs) { records.push_back(at); at += s.size() + w; }
        // patterns: the prefixes of the motif, the tag, the tandem repeat, a record, record ends and pads, a string that does not occur, an empty one
        std::vector<std::string> pats = {MOTIF, MOTIF.substr(0, 10), MOTIF.substr(0, 9), MOTIF.substr(0, 8), MOTIF.substr(0, 7), MOTIF.substr(0, 6), TAG, "ACAC", seqs[298], "", "AAAA", "AAA",
                                         seqs[40].substr(seqs[40].size() - 9), seqs[40].substr(seqs[40].size() - 8) + "A", seqs[40].substr(seqs[40].size() - 5) + "AAAA" + seqs[41].substr(0, 5), seqs[299].substr(seqs[299].size() - 9),
                                         MOTIF.substr(0, 11) + "A", "X", "c", "GT"};
        std::string bases; std::vector<uint64_t> off(1, 0);
        for (const std::string &p : pats) { bases += p; off.push_back(bases.size()); }
        bases += '\0';                                                     // (never a NULL pointer)
        const uint64_t np = pats.size();
        // the tables: the records; a document every 4 bytes (k_dl_table<4096>, the large LDS table of starts) and every byte (k_dl_table<16384>,
        // the starts bisected in two levels) with the defaults, the sort route and the table route in chunks of 7
        for (int tab = 0; tab < 3; ++tab) {
        std::vector<uint64_t> starts = records;
        if (tab) { starts.clear(); for (uint64_t b = 0; b + 1 < at; b += tab == 1 ? 4 : 1) starts.push_back(b); }
        std::vector<uint8_t> first[2][2][4];                                // [inside][max_count][cnt, off, doc, freq]
        const struct { const char *name; long long wave, table, chunk; } variants[] = {{"defaults", 64, 16384, 0}, {"chunks of 7", 64, 16384, 7}, {"no table", 64, 0, 0}, {"no table, chunks of 7", 64, 0, 7},
                                                                                     {"sort", 0, 0, 0}, {"sort, chunks of 7", 0, 0, 7}, {"table", 0, 16384, 0}, {"table, chunks of 7", 0, 16384, 7}};
        for (const auto &v : variants) {
            if (tab && &v != &variants[0] && &v != &variants[4] && &v != &variants[7]) continue;
            ok = ok && pfp_debug_set(c, "dl_wave_max", v.wave) == PFP_OK && pfp_debug_set(c, "dl_table_max", v.table) == PFP_OK && pfp_debug_set(c, "dl_chunk_values", v.chunk) == PFP_OK;
            for (int inside = 0; ok && inside < 2; ++inside) for (int mc = 0; ok && mc < 2; ++mc) {
                pfp_dl_info info;
                ok = pfp_ri_docs(c, (const uint8_t *)bases.data(), off.data(), np, starts.data(), starts.size(), inside ? PFP_DL_INSIDE : 0u, mc ? 64 : 0, &info) == PFP_OK;
                std::vector<uint8_t> a[4];
                if (ok) { a[0].resize(np * U); a[1].resize((np + 1) * 8); a[2].resize(info.entries * U); a[3].resize(info.entries * U); }
                ok = ok && pfp_ri_docs_offsets_get(c, (uint64_t *)a[1].data(), nullptr) == PFP_OK && pfp_ri_docs_get(c, a[0].data(), a[2].data(), a[3].data()) == PFP_OK;
                if (!ok) break;
                if (first[inside][mc][1].empty()) {
                    for (int k = 0; k < 4; ++k) { first[inside][mc][k] = a[k]; put(f, a[k].data(), a[k].size()); }
                    put(f, &info, sizeof info);
                    printf("U = %zu, inside %d, max_count %d: %llu occurrences, %llu pairs, longest list %llu, %llu skipped, %llu outside; wave %llu table %llu sort %llu\n", U, inside, mc ? 64 : 0, (unsigned long long)info.occurrences,
                           (unsigned long long)info.entries, (unsigned long long)info.max_docs, (unsigned long long)info.skipped, (unsigned long long)info.outside, (unsigned long long)info.by_wave, (unsigned long long)info.by_table, (unsigned long long)info.by_sort);
                    if (!inside && !mc) ok = info.by_wave > 0 && info.by_table > 0 && info.max_docs >= 300 && info.entries > 1000 && (tab || info.max_docs == 300);
                } else {
                    for (int k = 0; k < 4; ++k) if (a[k] != first[inside][mc][k]) { printf("U = %zu, %s, inside %d, max_count %d: array %d DIFFERS\n", U, v.name, inside, mc, k); ok = false; }
                    if (v.chunk && !mc && info.chunks < 10) { printf("%s: %llu chunks\n", v.name, (unsigned long long)info.chunks); ok = false; }
                    if (!v.wave && !v.table && !info.by_sort) ok = false;
                }
            }
            printf("U = %zu, %zu documents, %s: %s\n", U, starts.size(), v.name, ok ? "same arrays" : "FAILED");
        }
        }
        // the other callers of the shared pattern batch (queries.h) on the same patterns: matching statistics, a locate per route (the SA
        // route exists only beside a resident SA), MEMs with their occurrences.  Nothing of this goes to the file; the routes must agree.
        ok = ok && pfp_debug_set(c, "dl_wave_max", 64) == PFP_OK && pfp_debug_set(c, "dl_table_max", 16384) == PFP_OK && pfp_debug_set(c, "dl_chunk_values", 0) == PFP_OK;
        ok = ok && (wide ? pfp_thresholds(c, nullptr) : pfp_thresholds_windowed(c, 0, nullptr, nullptr)) == PFP_OK && pfp_ms_index(c) == PFP_OK;
        pfp_ms_info msi;
        ok = ok && pfp_ms_query(c, (const uint8_t *)bases.data(), off.data(), np, &msi) == PFP_OK && msi.patterns == np && msi.bases == off[np];
        std::vector<uint8_t> ms[2], loc[2][3], mem[2][5];                     // [route - 1][cnt, off, pos] and [route - 1][start, len, ptr, cnt, pos]
        if (ok) { ms[0].resize(msi.bases * U); ms[1].resize(msi.bases * U); ok = pfp_ms_get(c, ms[0].data(), ms[1].data()) == PFP_OK; }
        for (int route = 1; ok && route <= 2; ++route) {
            pfp_ri_info ri; pfp_mem_info mi;
            ok = pfp_debug_set(c, "ri_route", route) == PFP_OK;
            if (route == 2 && !wide) { ok = ok && pfp_ri_locate(c, (const uint8_t *)bases.data(), off.data(), np, 0, &ri) == PFP_E_STATE && pfp_mem_find(c, 6, 1, 0, &mi) == PFP_E_STATE; break; }
            ok = ok && pfp_ri_locate(c, (const uint8_t *)bases.data(), off.data(), np, 0, &ri) == PFP_OK && ri.route == (uint64_t)route && ri.reported == ri.occurrences;
            auto *l = loc[route - 1];
            if (ok) { l[0].resize(np * U); l[1].resize((np + 1) * 8); l[2].resize(ri.reported * U); }
            ok = ok && pfp_ri_offsets_get(c, (uint64_t *)l[1].data(), nullptr) == PFP_OK && pfp_ri_get(c, l[0].data(), l[2].data()) == PFP_OK;
            ok = ok && pfp_mem_find(c, 6, 1, 0, &mi) == PFP_OK && mi.route == (uint64_t)route && mi.mems > 0 && mi.reported == mi.occurrences;
            auto *m = mem[route - 1];
            if (ok) { for (int k = 0; k < 4; ++k) m[k].resize(mi.mems * U); m[4].resize(mi.reported * U); }
            ok = ok && pfp_mem_get(c, m[0].data(), m[1].data(), m[2].data(), m[3].data(), m[4].data()) == PFP_OK;
            if (ok) printf("U = %zu, route %d: %llu bases, %llu breaks; locate %llu occurrences, %llu pieces; %llu MEMs of at least 6, %llu occurrences\n", U, route, (unsigned long long)msi.bases, (unsigned long long)msi.breaks,
                           (unsigned long long)ri.occurrences, (unsigned long long)ri.pieces, (unsigned long long)mi.mems, (unsigned long long)mi.occurrences);
        }
        if (ok && wide) for (int k = 0; k < 5; ++k) if ((k < 3 && loc[0][k] != loc[1][k]) || mem[0][k] != mem[1][k]) { printf("U = %zu: the locate routes DIFFER in array %d\n", U, k); ok = false; }
        ok = ok && pfp_debug_set(c, "ri_route", 0) == PFP_OK;
        bad += !ok;
        pfp_destroy(c);
    }
    fclose(f);
    printf(bad ? "asan_doclist: %d FAILED\n" : "asan_doclist: all variants agree\n", bad);
    return bad != 0;
}
