// pfbwt-f_amd/csrc/vcfread.h -- a small reader of text VCF (plain or gzip / bgzip) and of the reference FASTA that goes with it: the
// input side of pfp_parse_feed_vcf_file (include/pfbwt_hip.h states the rules).  Stands in for what the reference does with htslib in
// include/vcf_scanner.hpp (genotypes: :32-38, 185-188, 217-219) as far as a variant panel needs it; BCF, indexes and regions are out of
// scope.  Host code that depends on zlib and the standard library only: it is included by pfbwt_hip.hip and, on its own, by
// tools/vcfread_check.cpp (the sanitizer build of `make vcfread-asan`).
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include <zlib.h>

namespace pfpvcf {

enum { VCF_OK = 0, VCF_E_CORRUPT = -8, VCF_E_IO = -9 };      // the values of PFP_E_CORRUPT / PFP_E_IO

// The arrays of a pfp_panel, owned.
struct Panel {
    std::vector<std::string> contig_names, hap_names;
    std::string ref, alt_bytes;
    std::vector<uint64_t> ref_off, site_first, pos, allele_first, alt_off;
    std::vector<uint32_t> span;
    std::vector<uint8_t> gt;
    uint64_t nhap = 0, lines = 0, samples = 0, skipped_symbolic = 0, missing_gt = 0;
};

struct LineReader {
    gzFile fp = nullptr; std::vector<char> buf; int pos = 0, len = 0; bool failed = false;
    explicit LineReader(const char *path) : buf(1 << 16) { fp = gzopen(path, "rb"); }
    ~LineReader() { if (fp) gzclose(fp); }
    bool next(std::string &line)      // without its line end; false at the end of the file
    {
        line.clear();
        bool any = false;
        for (;;) {
            if (pos == len) {
                len = fp ? gzread(fp, buf.data(), (unsigned)buf.size()) : -1; pos = 0;
                if (len < 0) { failed = true; len = 0; }
                if (len == 0) break;
            }
            any = true;
            const char *nl = (const char *)memchr(buf.data() + pos, '\n', (size_t)(len - pos));
            if (nl) { line.append(buf.data() + pos, (size_t)(nl - (buf.data() + pos))); pos = (int)(nl - buf.data()) + 1; break; }
            line.append(buf.data() + pos, (size_t)(len - pos)); pos = len;
        }
        if (!line.empty() && line.back() == '\r') line.pop_back();
        return any;
    }
    bool bad()      // a damaged gzip stream shows at the end
    {
        if (failed || !fp) return true;
        int zerr = Z_OK; (void)gzerror(fp, &zerr);
        return zerr != Z_OK && zerr != Z_STREAM_END;
    }
};

// FASTA records with the rules of the engine's record reader (kseq: the name is the header's first word, the other lines are joined)
inline int load_fasta(const char *path, Panel *P)
{
    LineReader rd(path);
    if (!rd.fp) return VCF_E_IO;
    P->contig_names.clear(); P->ref.clear(); P->ref_off.assign(1, 0);
    std::string line; bool open = false;
    while (rd.next(line)) {
        if (!line.empty() && line[0] == '>') {
            if (open) P->ref_off.push_back(P->ref.size());
            size_t e = 1; while (e < line.size() && line[e] != ' ' && line[e] != '\t') ++e;
            P->contig_names.push_back(line.substr(1, e - 1)); open = true;
        } else if (open) P->ref += line;
    }
    if (open) P->ref_off.push_back(P->ref.size());
    return rd.bad() ? VCF_E_IO : VCF_OK;
}

inline void split(const std::string &s, char sep, std::vector<std::string> *out)
{
    out->clear();
    size_t a = 0;
    for (;;) { const size_t b = s.find(sep, a); if (b == std::string::npos) { out->push_back(s.substr(a)); return; } out->push_back(s.substr(a, b - a)); a = b + 1; }
}
inline bool symbolic(const std::string &a)
{
    return a.empty() || a == "." || a == "*" || a[0] == '<' || a.find('[') != std::string::npos || a.find(']') != std::string::npos;
}
inline bool parse_uint(const char *b, const char *e, uint64_t *v)
{
    if (b == e || e - b > 18) return false;
    uint64_t x = 0;
    for (; b < e; ++b) { if (*b < '0' || *b > '9') return false; x = x * 10 + (uint64_t)(*b - '0'); }
    *v = x; return true;
}

// The VCF on top of a loaded FASTA.  *err_line = the 1-based line of a VCF_E_CORRUPT.
inline int load_vcf(const char *path, const char *samples, Panel *P, uint64_t *err_line)
{
    LineReader rd(path);
    if (!rd.fp) return VCF_E_IO;
    const uint64_t ncontigs = P->contig_names.size();
    std::map<std::string, uint64_t> contig_of;
    for (uint64_t c = 0; c < ncontigs; ++c) contig_of.emplace(P->contig_names[c], c);
    // in file order: the block of every contig is moved into FASTA order at the end
    std::vector<uint64_t> f_pos, f_afirst(1, 0), blk0(ncontigs, ~0ULL), blk1(ncontigs, 0);
    std::vector<uint32_t> f_span; std::vector<uint8_t> f_gt; std::vector<std::string> alts;
    std::vector<size_t> cols;      // field index of every selected sample
    std::string line; std::vector<std::string> f, al;
    uint64_t lineno = 0, cur = ~0ULL, prev_pos = 0, nsamp_file = 0;
    bool have_header = false;
    P->lines = P->skipped_symbolic = P->missing_gt = 0;
    auto corrupt = [&]() { *err_line = lineno; return (int)VCF_E_CORRUPT; };
    while (rd.next(line)) {
        ++lineno;
        if (line.empty() || (line.size() >= 2 && line[0] == '#' && line[1] == '#')) continue;
        if (line[0] == '#') {
            split(line, '\t', &f);
            if (f.size() < 8 || f[0] != "#CHROM") return corrupt();
            have_header = true;
            nsamp_file = f.size() > 9 ? f.size() - 9 : 0;
            cols.clear(); P->hap_names.clear();
            std::vector<std::string> want;
            if (samples && *samples) split(samples, ',', &want);
            else for (size_t k = 9; k < f.size(); ++k) want.push_back(f[k]);
            for (auto &nm : want) {
                size_t k = 9; while (k < f.size() && f[k] != nm) ++k;
                if (k >= f.size()) return corrupt();
                cols.push_back(k); P->hap_names.push_back(nm + ".0"); P->hap_names.push_back(nm + ".1");
            }
            P->samples = cols.size(); P->nhap = 2 * cols.size();
            continue;
        }
        if (!have_header) return corrupt();
        split(line, '\t', &f);
        if (f.size() < 8 || (nsamp_file && f.size() < 9 + nsamp_file)) return corrupt();      // a short line
        ++P->lines;
        const auto it = contig_of.find(f[0]);
        if (it == contig_of.end()) return corrupt();
        const uint64_t c = it->second, clen = P->ref_off[c + 1] - P->ref_off[c];
        if (c != cur) {
            if (blk0[c] != ~0ULL) return corrupt();      // the lines of a contig are one block
            if (cur != ~0ULL) blk1[cur] = f_pos.size();
            cur = c; blk0[c] = f_pos.size(); prev_pos = 0;
        }
        uint64_t pos1 = 0;
        if (!parse_uint(f[1].data(), f[1].data() + f[1].size(), &pos1) || pos1 < 1) return corrupt();
        const uint64_t pos = pos1 - 1, span = f[3].size();
        if (pos < prev_pos) return corrupt();
        prev_pos = pos;
        if (pos > clen || span > clen - pos || span >= (1ULL << 32)) return corrupt();
        for (uint64_t k = 0; k < span; ++k) {
            const int a = (unsigned char)f[3][k], b = (unsigned char)P->ref[P->ref_off[c] + pos + k];
            if ((a >= 'a' && a <= 'z' ? a - 32 : a) != (b >= 'a' && b <= 'z' ? b - 32 : b)) return corrupt();
        }
        split(f[4], ',', &al);
        if (al.size() > 255) return corrupt();
        bool sym = false;
        for (auto &a : al) sym = sym || symbolic(a);
        if (sym) { ++P->skipped_symbolic; blk1[cur] = f_pos.size(); continue; }
        if (!cols.empty() && !(f[8].compare(0, 2, "GT") == 0 && (f[8].size() == 2 || f[8][2] == ':'))) return corrupt();
        for (size_t k : cols) {
            const std::string &s = f[k];
            const size_t e = s.find(':') == std::string::npos ? s.size() : s.find(':');
            uint8_t g[2] = {0, 0}; int ng = 0;
            size_t a = 0;
            while (a <= e) {
                size_t b = a; while (b < e && s[b] != '|' && s[b] != '/') ++b;
                if (ng == 2) return corrupt();      // ploidy above 2
                uint64_t v = 0;
                if (b == a || (b == a + 1 && s[a] == '.')) ++P->missing_gt;
                else if (!parse_uint(s.data() + a, s.data() + b, &v) || v > al.size()) return corrupt();
                g[ng++] = (uint8_t)v;
                a = b + 1;
            }
            if (ng == 1) g[1] = g[0];      // a haploid call serves both haplotypes
            f_gt.push_back(g[0]); f_gt.push_back(g[1]);
        }
        f_pos.push_back(pos); f_span.push_back((uint32_t)span);
        for (auto &a : al) alts.push_back(a);
        f_afirst.push_back(alts.size());
        blk1[cur] = f_pos.size();
    }
    if (rd.bad()) return VCF_E_IO;
    if (!have_header) { lineno = lineno ? lineno : 1; return corrupt(); }
    // into FASTA order
    P->site_first.assign(1, 0); P->pos.clear(); P->span.clear(); P->allele_first.assign(1, 0); P->alt_off.assign(1, 0); P->alt_bytes.clear(); P->gt.clear();
    for (uint64_t c = 0; c < ncontigs; ++c) {
        for (uint64_t v = blk0[c] == ~0ULL ? 0 : blk0[c]; blk0[c] != ~0ULL && v < blk1[c]; ++v) {
            P->pos.push_back(f_pos[v]); P->span.push_back(f_span[v]);
            for (uint64_t a = f_afirst[v]; a < f_afirst[v + 1]; ++a) { P->alt_bytes += alts[a]; P->alt_off.push_back(P->alt_bytes.size()); }
            P->allele_first.push_back(P->alt_off.size() - 1);
            P->gt.insert(P->gt.end(), f_gt.begin() + (size_t)(v * P->nhap), f_gt.begin() + (size_t)((v + 1) * P->nhap));
        }
        P->site_first.push_back(P->pos.size());
    }
    return VCF_OK;
}

} // namespace pfpvcf
