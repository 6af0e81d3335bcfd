// tools/asan_feed.cpp -- the feeding entries of pfbwt-f_amd/csrc/feed_host.h (and the panel feed on top of them) and the table of route /
// tuning switches of pfbwt-f_amd/csrc/pfbwt_hip.hip under AddressSanitizer + UBSan: a stand-alone program that includes the engine
// interpreted on the CPU (tests/emu).  Three parts, everything written to the file named on the command line:
//   1. every way of appending to the text -- records one by one and in parts, host and device batches, a row view followed by a feed and
//      by a text view, a left context, a feed behind a finalize with and without pfp_parse_reopen, raw FASTA bytes in pieces of 64 bytes
//      with fasta_chunk_bytes = 64, a FASTA file in blocks of 256 bytes, a variant panel, a record that outgrows the announced range --
//      and every call the entries refuse, (w, p) = (4, 7), both widths: the status of every call and the text behind it;
//   2. every switch (the literal list below) set to -5, 0, 1, 17, 2^21 and 2^40 through pfp_debug_set on a fresh context: the status and
//      every field of the context's Tunables, by name;
//   3. the same through PFP_<NAME> in the environment of a process with PFP_TEST_HOOKS=1, and once without PFP_TEST_HOOKS, which must
//      change nothing but `verbose`.
// The same source built without the sanitizers must write the same bytes, and so must a build of any commit that leaves behaviour alone:
//
//   F="-O1 -g -std=c++17 -x c++ -Itests/emu -DPFP_BACKEND_NAME=\"cpu-emu-TEST-ONLY\" -Wno-unused-function"
//   g++ $F -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o tests/emu/build/asan_feed tools/asan_feed.cpp -lz -lpthread
//   g++ $F -o tests/emu/build/plain_feed tools/asan_feed.cpp -lz -lpthread
//   ASAN_OPTIONS=detect_leaks=0 tests/emu/build/asan_feed /tmp/a.bin && tests/emu/build/plain_feed /tmp/b.bin && cmp /tmp/a.bin /tmp/b.bin
#include "../pfbwt-f_amd/csrc/pfbwt_hip.hip"
#include <string>

static FILE *g_out;
static int bad;
static void put(const void *p, size_t bytes) { const uint64_t n = bytes; fwrite(&n, 8, 1, g_out); if (bytes) fwrite(p, 1, bytes, g_out); }
static void put_u64(uint64_t v) { fwrite(&v, 8, 1, g_out); }
static void put_str(const char *s) { put(s, strlen(s)); }

struct Rng { uint64_t s; uint32_t next() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(s >> 33); } uint32_t below(uint32_t k) { return next() % k; } };
static std::string bases(Rng &r, size_t n) { std::string s(n, 'A'); for (auto &ch : s) ch = "ACGT"[r.below(4)]; return s; }

// the switches of include/pfbwt_hip_dev.h: X(field of Tunables); the key of pfp_debug_set is the field's name
#define SWITCHES(X) \
    X(verbose) X(seg_grid) X(seg_stage) X(sort_k) X(sort_no_table) X(class_sort_maxrange) X(dedup_table_log2) X(no_trigger_table) X(emit_chunk_rows) X(fill_subs) \
    X(sample_cap) X(no_runaware) X(big_group_members) X(force_wide_rows) X(fasta_chunk_bytes) X(ingest_block_bytes) X(emit_group_rows) X(no_slot_records) \
    X(dict_text_rounds) X(int_key_symbols) X(force_run_round) X(ingest_readers) X(expand_dma) X(parse_rec) X(parse_rec_p2) X(parse_rec_min) X(parse_rec_depth) \
    X(parse_rec_tile_rows) X(parse_rec_merge) X(parse_rec_merge_members) X(parse_rec_table_log2) X(dict_rec) X(dict_rec_p2) X(dedup_variant) X(dedup_phases) \
    X(dedup_period) X(dedup_chunk) X(doc_lds_max) X(dedup_packed) X(group_reduce) X(scan_waves) X(lcp_long_min) X(thr_long_min) X(thr_tile) X(thr_window_rows) \
    X(plcp_block_log2) X(fill_masks) X(fill_skip) X(ms_dir_log2) X(ms_long_min) X(ri_dir_log2) X(ri_route) X(dl_chunk_values) X(dl_wave_max) X(dl_table_max) \
    X(mk_chunk_entries) X(mk_wave_max) X(panel_tile) X(panel_out_bytes) X(panel_swizzle)
#define X(name) #name,
static const char *const switch_names[] = {SWITCHES(X)};
#undef X
static_assert(sizeof switch_names / sizeof switch_names[0] == 60, "sixty switches");
static void put_tunables(const pfp::Tunables &t)
{
#define X(name) put_str(#name); put_u64((uint64_t)t.name);
    SWITCHES(X)
#undef X
}
static bool same_but_verbose(pfp::Tunables a, const pfp::Tunables &b)
{
    a.verbose = b.verbose;
#define X(name) if (a.name != b.name) return false;
    SWITCHES(X)
#undef X
    return true;
}

// ---- part 1 --------------------------------------------------------------------------------------------------------------------------
static pfp_ctx *create(int wide)
{
    int st = 0;
    pfp_ctx *c = pfp_create(4, 7, (wide ? PFP_FLAG_U64 : 0u) | PFP_FLAG_SAI, 0, 0, &st);
    if (!c) { fprintf(stderr, "pfp_create: %d\n", st); exit(2); }
    return c;
}
// the status of a call, then the length of the text and the text itself (or the status pfp_text_get answers)
static void put_state(pfp_ctx *c, const char *what, int status, bool digest_only = false)
{
    put_str(what); put_u64((uint64_t)(int64_t)status);
    uint64_t n = 0;
    put_u64((uint64_t)(int64_t)pfp_text_length(c, &n)); put_u64(n);
    std::vector<uint8_t> t((size_t)n);
    const int rc = pfp_text_get(c, 0, n, t.data());
    put_u64((uint64_t)(int64_t)rc);
    if (rc != PFP_OK) return;
    if (!digest_only) { put(t.data(), t.size()); return; }
    uint64_t h = 1469598103934665603ULL;
    for (uint8_t b : t) h = (h ^ b) * 1099511628211ULL;
    put_u64(h);
}
#define CALL(c, expr) put_state((c), #expr, (expr))
// the status alone: reading the text would turn a pending view into text
#define CALL_ONLY(expr) do { put_str(#expr); put_u64((uint64_t)(int64_t)(expr)); } while (0)

static void feeds(int wide, const char *tmp_path)
{
    Rng r = {77 + (uint64_t)wide};
    const uint64_t big = wide ? (1ULL << 40) : (1ULL << 32);
    // rows of a batch: 5 of 33 bases, 40 apart; rows of a view: 2 of 21 bases, 32 apart
    std::string rows(5 * 40, 'N'), vrows(2 * 32, 'N');
    for (int k = 0; k < 5; ++k) rows.replace((size_t)k * 40, 33, bases(r, 33));
    for (int k = 0; k < 2; ++k) vrows.replace((size_t)k * 32, 21, bases(r, 21));
    const uint8_t *hp = (const uint8_t *)rows.data(), *vp = (const uint8_t *)vrows.data();
    const std::string a = bases(r, 40), b = bases(r, 31), x = bases(r, 13), y = bases(r, 27), one = bases(r, 1);
    auto u8 = [](const std::string &s) { return (const uint8_t *)s.data(); };
    pfp_parse_sizes ps; pfp_bwt_sizes bs;

    pfp_ctx *c = create(wide);      // records one by one and in parts, then everything a context with text refuses
    CALL(c, pfp_parse_feed(c, u8(one), 1, 1));
    CALL(c, pfp_parse_feed(c, u8(x), x.size(), 0));
    CALL(c, pfp_parse_feed(c, u8(y), y.size(), 1));
    CALL(c, pfp_parse_feed(c, nullptr, 0, 1));
    CALL(c, pfp_parse_feed_device(c, u8(a), a.size(), 1));
    CALL(c, pfp_parse_feed(c, nullptr, 5, 1));
    CALL(c, pfp_parse_feed_batch(c, hp, 2, 33, 32));
    CALL(c, pfp_parse_feed_device_batch(c, hp, 2, 33, 32));
    CALL(c, pfp_parse_feed_batch(c, nullptr, 2, 33, 40));
    CALL(c, pfp_parse_feed_device_batch(c, nullptr, 2, 33, 40));
    CALL(c, pfp_parse_feed_batch(c, hp, 0, 33, 40));
    CALL(c, pfp_parse_feed_device_batch(c, hp, 0, 33, 40));
    CALL(c, pfp_parse_feed_device_view(c, vp, 0, 21, 32));
    CALL(c, pfp_parse_feed_device_view(c, vp, 2, 0, 32));
    CALL(c, pfp_parse_feed_device_view(c, vp, 2, 21, 20));
    CALL(c, pfp_parse_feed_device_view(c, nullptr, 2, 21, 32));
    CALL(c, pfp_parse_feed_device_view(c, vp, 2, 21, 32));
    CALL(c, pfp_parse_feed_left_context(c));
    CALL(c, pfp_text_get(c, c->n + 1, 0, (uint8_t *)rows.data()));
    CALL(c, pfp_text_get(c, 0, c->n + 1, (uint8_t *)rows.data()));
    CALL(c, pfp_parse_reopen(c));
    CALL(c, pfp_debug_set(c, "no_such_switch", 1));
    CALL(c, pfp_debug_set(c, nullptr, 1));
    CALL(c, pfp_parse_feed(c, hp, big, 1));
    CALL(c, pfp_parse_feed_device(c, hp, big, 1));
    CALL(c, pfp_parse_feed_batch(c, hp, 1, big, big));
    CALL(c, pfp_parse_feed_device_batch(c, hp, 1, big, big));
    CALL(c, pfp_parse_feed_batch(c, hp, 5, 33, 40));
    CALL(c, pfp_parse_feed_device_batch(c, hp, 5, 33, 40));
    CALL(c, pfp_parse_feed_batch(c, nullptr, 3, 0, 0));
    CALL(c, pfp_parse_feed_device_batch(c, nullptr, 3, 0, 0));
    pfp_destroy(c);

    c = create(wide);               // an empty context: the limit of every entry, the view, a feed behind it
    CALL(c, pfp_parse_feed(c, hp, big, 1));
    CALL(c, pfp_parse_feed_device(c, hp, big, 1));
    CALL(c, pfp_parse_feed_batch(c, hp, 1, big, big));
    CALL(c, pfp_parse_feed_device_batch(c, hp, 1, big, big));
    CALL(c, pfp_parse_feed_device_view(c, hp, 1, big, big));
    CALL_ONLY(pfp_parse_feed_device_view(c, vp, 2, 21, 32));    // a view whose first reader is a feed
    CALL(c, pfp_parse_feed(c, u8(b), b.size(), 1));
    CALL(c, pfp_reset(c));
    CALL(c, pfp_parse_feed_device_view(c, vp, 2, 21, 32));      // ... the text view
    CALL(c, pfp_parse_finalize(c, &ps));
    CALL_ONLY(pfp_parse_feed_device_view(c, vp, 2, 21, 32));    // ... the trigger scan of the parse, which reads the rows in place
    CALL(c, pfp_parse_finalize(c, &ps));
    pfp_destroy(c);

    c = create(wide);               // a left context, a finalize, a feed behind it (a new text), a reopen behind a parse and behind a build
    CALL(c, pfp_parse_feed_left_context(c));
    CALL(c, pfp_parse_feed(c, u8(a), a.size(), 1));
    CALL(c, pfp_parse_finalize(c, &ps));
    CALL(c, pfp_parse_feed(c, u8(b), b.size(), 1));
    CALL(c, pfp_parse_finalize(c, &ps));
    CALL(c, pfp_parse_reopen(c));
    CALL(c, pfp_parse_feed(c, u8(a), a.size(), 1));
    CALL(c, pfp_parse_finalize(c, &ps));
    CALL(c, pfp_parse_bwt(c));
    CALL(c, pfp_bwt_build(c, 1, 1, &bs));
    CALL(c, pfp_parse_reopen(c));
    CALL(c, pfp_parse_feed_batch(c, hp, 5, 33, 40));
    CALL(c, pfp_parse_finalize(c, &ps));
    put(&ps, sizeof ps);
    pfp_destroy(c);

    // raw FASTA: bytes in pieces of 64 through device buffers of 64 bytes, then the same file in blocks of 256 bytes
    std::string fa = "preamble\n";
    for (int k = 0; k < 6; ++k) {
        const std::string s = bases(r, 1 + r.below(k == 3 ? 600 : 40));
        fa += ">rec" + std::to_string(k) + " comment\n";
        for (size_t i = 0; i < s.size(); i += 25) fa += s.substr(i, 25) + (k & 1 ? "\r\n" : "\n");
    }
    c = create(wide);
    CALL(c, pfp_debug_set(c, "fasta_chunk_bytes", 64));
    CALL(c, pfp_parse_feed(c, u8(x), x.size(), 1));
    for (size_t o = 0; o < fa.size(); o += 64) {
        const size_t len = fa.size() - o < 64 ? fa.size() - o : 64;
        uint64_t nrec = 0;
        put_state(c, "pfp_parse_feed_fasta", pfp_parse_feed_fasta(c, (const uint8_t *)fa.data() + o, len, PFP_FASTA_RECORDS | (o + 64 >= fa.size() ? PFP_FASTA_FINAL : 0u), &nrec));
        std::vector<uint64_t> ro((size_t)nrec + 1), tp((size_t)nrec + 1);
        put_u64(nrec); put_u64((uint64_t)(int64_t)pfp_parse_fasta_records(c, ro.data(), tp.data()));
        put(ro.data(), (size_t)nrec * 8); put(tp.data(), (size_t)nrec * 8);
    }
    CALL(c, pfp_parse_feed_fasta(c, nullptr, 5, PFP_FASTA_FINAL, nullptr));
    CALL(c, pfp_parse_finalize(c, &ps));
    pfp_destroy(c);
    if (FILE *f = fopen(tmp_path, "wb")) { fwrite(fa.data(), 1, fa.size(), f); fclose(f); } else { perror(tmp_path); exit(2); }
    c = create(wide);
    CALL(c, pfp_debug_set(c, "ingest_block_bytes", 256));
    CALL(c, pfp_parse_feed(c, u8(y), y.size(), 1));
    pfp_ingest_info ii;
    CALL(c, pfp_parse_feed_fasta_file(c, tmp_path, PFP_FASTA_RECORDS, &ii));
    put_u64(ii.raw_bytes); put_u64(ii.records); put_u64(ii.n); put_u64((uint64_t)ii.mode);
    CALL(c, pfp_parse_feed_fasta_file(c, nullptr, 0, nullptr));
    CALL(c, pfp_parse_feed_fasta_file(c, "/nonexistent/asan_feed.fa", 0, nullptr));
    uint64_t ndocs = 0;
    CALL(c, pfp_parse_docs(c, &ndocs));
    put_u64(ndocs);
    for (uint64_t i = 0; i <= ndocs; ++i) {
        const char *name = ""; uint64_t start = 0;
        put_u64((uint64_t)(int64_t)pfp_parse_doc_get(c, i, &name, &start)); put_str(name); put_u64(start);
    }
    pfp_destroy(c);
    remove(tmp_path);

    // a variant panel behind a record: one contig of 60 bases, three sites (a substitution, a deletion, an insertion), two haplotypes
    const std::string ref = bases(r, 60), alts = "T" "GGA";
    const uint64_t ref_off[2] = {0, 60}, site_first[2] = {0, 3}, pos[3] = {5, 20, 41}, allele_first[4] = {0, 1, 2, 3}, alt_off[4] = {0, 1, 1, 4};
    const uint32_t span[3] = {1, 4, 0};
    uint8_t gt[6] = {1, 0, 0, 1, 1, 1};
    pfp_panel P = {};
    P.ncontigs = 1; P.ref = u8(ref); P.ref_off = ref_off; P.nsites = 3; P.site_first = site_first; P.pos = pos; P.span = span; P.allele_first = allele_first;
    P.nalt = 3; P.alt_off = alt_off; P.alt_bytes = u8(alts); P.nhap = 2; P.gt = gt;
    c = create(wide);
    pfp_panel_info pi;
    CALL(c, pfp_parse_feed(c, u8(x), x.size(), 1));
    CALL(c, pfp_parse_feed_panel(c, &P, PFP_PANEL_REF_FIRST | PFP_PANEL_RECORDS, &pi));
    put(&pi, sizeof pi);
    gt[2] = 7;
    CALL(c, pfp_parse_feed_panel(c, &P, PFP_PANEL_REF_FIRST, &pi));      // a genotype without an allele: refused, the text as it was
    gt[2] = 0;
    CALL(c, pfp_parse_feed_panel(c, &P, 4u, nullptr));
    CALL(c, pfp_parse_feed_panel(c, nullptr, 0, nullptr));
    CALL(c, pfp_parse_feed_device_view(c, vp, 2, 21, 32));
    CALL(c, pfp_reset(c));
    CALL_ONLY(pfp_parse_feed_device_view(c, vp, 2, 21, 32));             // a pending view in front of a panel
    CALL(c, pfp_parse_feed_panel(c, &P, 0, &pi));
    CALL(c, pfp_parse_finalize(c, &ps));
    pfp_destroy(c);

    if (wide) {                     // the announced range (1 + 1 / 8 + 64 MiB, in pieces of 2 MiB) outgrown: the one path that copies text
        const std::string head = bases(r, 1000);
        std::string huge((size_t)66 << 20, 'A');
        for (size_t i = 0; i < huge.size(); i += 7) huge[i] = "ACGT"[r.below(4)];
        c = create(wide);
        CALL(c, pfp_parse_reserve(c, 1));
        CALL(c, pfp_parse_feed(c, u8(head), head.size(), 1));
        put_state(c, "outgrow", pfp_parse_feed(c, u8(huge), huge.size(), 1), true);
        std::vector<uint8_t> t(1004);
        put_u64((uint64_t)(int64_t)pfp_text_get(c, 0, 1004, t.data())); put(t.data(), t.size());
        pfp_destroy(c);
    }
}

// ---- parts 2 and 3 -----------------------------------------------------------------------------------------------------------------------
static void switches()
{
    const long long values[] = {-5, 0, 1, 17, 1LL << 21, 1LL << 40};
    int st = 0;
    for (const char *key : switch_names) for (long long v : values) {
        pfp_ctx *c = pfp_create(4, 7, 0, 0, 0, &st);
        put_str(key); put_u64((uint64_t)v); put_u64((uint64_t)(int64_t)pfp_debug_set(c, key, v));
        put_tunables(c->tun);
        pfp_destroy(c);
    }
    const char *const texts[] = {"", "-5", "0", "1", "17", "2097152", "1099511627776"};
    for (int hooks = 1; hooks >= 0; --hooks) {
        if (hooks) setenv("PFP_TEST_HOOKS", "1", 1); else unsetenv("PFP_TEST_HOOKS");
        for (const char *key : switch_names) for (const char *text : texts) {
            std::string env = "PFP_";
            for (const char *q = key; *q; ++q) env += (char)toupper(*q);
            setenv(env.c_str(), text, 1);
            pfp_ctx *c = pfp_create(4, 7, 0, 0, 0, &st);
            unsetenv(env.c_str());
            put_str(env.c_str()); put_str(text); put_u64((uint64_t)hooks);
            put_tunables(c->tun);
            if (!hooks && (!same_but_verbose(c->tun, pfp::Tunables()) || c->tun.verbose != (strcmp(key, "verbose") ? 0 : 1))) { printf("%s=%s without PFP_TEST_HOOKS changed a switch\n", env.c_str(), text); ++bad; }
            pfp_destroy(c);
            if (!hooks) break;      // (one value per key: the variable must not be looked at)
        }
    }
    unsetenv("PFP_TEST_HOOKS");
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s OUTPUT\n", argv[0]); return 2; }
    setenv("PFP_EMU_POISON", "1", 1);
    unsetenv("PFP_VERBOSE");
    g_out = fopen(argv[1], "wb");
    if (!g_out) { perror(argv[1]); return 2; }
    const std::string tmp = std::string(argv[1]) + ".fa";
    for (int wide = 0; wide < 2; ++wide) feeds(wide, tmp.c_str());
    switches();
    fclose(g_out);
    printf(bad ? "asan_feed: %d FAILED\n" : "asan_feed: written\n", bad);
    return bad != 0;
}
