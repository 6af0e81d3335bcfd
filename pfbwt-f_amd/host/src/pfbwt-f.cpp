// pfbwt-f_amd/host/src/pfbwt-f.cpp -- command-line front end with the flag surface, stage timer
// lines, stderr statistics and output files of the reference's src/pfbwt-f.cpp (flags :113-153, timers
// :35-50, run_parser :209-245, run_pfbwt :275-349), driving the MI355X engine through the host mirror of
// the reference classes.  Build with -DM64 for pfbwt-f64 (uint_t = 64 bit), without for pfbwt-f.
#include <chrono>
#include <cstdlib>
#include <fcntl.h>
#include <getopt.h>
#include <string>
#include <sys/mman.h>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>
#include "file_wrappers.hpp"
#include "pfbwt.hpp"
#include "pfbwt_io.hpp"
#include "pfparser.hpp"

namespace {

struct Options {
    std::string in_fname, output, stdout_ext;
    size_t w = 10, p = 100, n = 0;
    int sa = 0, rssa = 0, mmap = 0, parse_only = 0, trim_non_acgt = 0, non_acgt_to_a = 0, pfbwt_only = 0, verbose = 0, print_docs = 0, gpus = 0, da = 0, lcp = 0, thr = 0, thr_windowed = 0;
    unsigned long long thr_window = 0;      // --thr-window <rows> (0: the engine's default window)
    std::string ms;           // --ms <reads>: matching statistics of the reads against the build
    unsigned long long mems = 0, mems_max = 0; int have_mems = 0, mems_locate = 0, have_mems_max = 0;      // --mems <L> [--mems-locate [--mems-max <K>]]: maximal exact matches of the reads of --ms
    std::string count, locate;      // --count <reads> / --locate <reads>: occurrences of the reads in the text, counted / listed
    unsigned long long locate_max = 0; int have_locate_max = 0;      // --locate-max <K>: at most K positions per read (0: all)
    std::string doclist;      // --doclist <reads>: the records every read occurs in, and how often in each
    unsigned long long doclist_max = 0; int doclist_inside = 0, have_doclist_max = 0;      // --doclist-inside, --doclist-max <K>
    std::string mps, ma, markers;      // --mps <file> / --ma <file>: the marker array made on the device / read; --markers <reads>: the markers their occurrences overlap
    unsigned long long markers_min_len = 0, markers_max_rows = 0; int have_markers_min_len = 0, have_markers_max_rows = 0;      // --markers-min-len <L>, --markers-max-rows <K>
    std::string devices;      // --devices 0,1,2 (default: 0 .. gpus-1)
    std::string vcf, vcf_samples; int vcf_no_ref = 0;      // --vcf <file> [--vcf-samples a,b] [--vcf-no-ref]: the positional argument is the reference FASTA
};

struct StageTimer {   // "TASK\t<what>\t<sec>s" on destruction (src/pfbwt-f.cpp:35-50)
    explicit StageTimer(const char *m) : msg(m), t0(std::chrono::system_clock::now()) {}
    ~StageTimer() { fprintf(stderr, "%s%.2fs\n", msg, std::chrono::duration<double>(std::chrono::system_clock::now() - t0).count()); }
    const char *msg; std::chrono::time_point<std::chrono::system_clock> t0;
};

void usage()
{
    fprintf(stderr, "%s. use the prefix-free parsing algorithm to build a BWT for %sgenomic data (MI355X engine).\n\nusage\n    ./%s [options] <fasta file>\n\n", M64 ? "pfbwt-f64" : "pfbwt-f",
            M64 ? "BIG " : "", M64 ? "pfbwt-f64" : "pfbwt-f");
    fprintf(stderr, "results\n    BWT of input saved to <fasta file>.bwt. Header lines are excluded.\n\noptions\n"
                    "    -o                  output prefix.\n    -s                  Output full suffix array to <fasta file>.sa\n"
                    "    -r                  Output run-length sampled suffix arrray to <fasta file>.ssa (run-starts) and <fasta file>.esa (run-ends)\n"
                    "    -w <int>            window-size for parsing [default: 10]\n    -p <int>            modulo for parsing [default: 100]\n"
                    "    -m                  accepted for compatibility (the workspace lives in HBM)\n"
                    "    --parse-only        only produce parse (dict, occ, ilist, last, bwlast)\n"
                    "    --pfbwt-only        build pfbwt from parse + parse-bwt. Requires -o to match parse files' prefix.\n"
                    "    --non-acgt-to-a     map every character outside ACGT to A\n    --print-docs        write <prefix>.docs\n"
                    "    -c/--stdout <ext>   output file ending <ext> will be stdout instead (bwt, sa)\n"
                    "    --da                (extension) document array: the record of every SA value, <prefix>.da with -s and <prefix>.sda/.eda\n"
                    "                        (the .ssa/.esa pairs with the SA value replaced by its record) with -r; with --pfbwt-only the records\n"
                    "                        come from <prefix>.docs (--print-docs of the parse)\n"
                    "    --lcp               (extension) LCP array of the text: <prefix>.lcp with -s (the LCP of every row with the row above, same width\n"
                    "                        as .sa) and <prefix>.slcp with -r ((run-start row, LCP of that row) pairs like .ssa); needs the text, so\n"
                    "                        not with --pfbwt-only\n"
                    "    --thr               (extension) matching-statistics thresholds, needs -r: <prefix>.thr ((run-start row, threshold row) pairs like\n"
                    "                        .ssa: the leftmost row with the smallest LCP between a run and the previous run of its symbol; 0 = none) and\n"
                    "                        <prefix>.tlcp ((run-start row, LCP of the threshold row) pairs); builds the SA on the device also without -s\n"
                    "                        (no .sa is written then); needs the text, so not with --pfbwt-only\n"
                    "    --thr-window <rows> (extension) with --thr: the windowed route for collections whose SA does not fit on the device -- no SA is\n"
                    "                        built for the thresholds (-r alone stays a samples-only build); the rows are visited <rows> at a time\n"
                    "                        (0: the default window) and their LCP values come from the run samples; same .thr / .tlcp\n"
                    "    --ms <reads>        (extension) matching statistics of the reads of a FASTA / FASTQ file (plain or gzip) against the build, needs\n"
                    "                        -r --thr (with or without --thr-window): for every base of every read a text position and the length of the\n"
                    "                        longest prefix of the read from there on that occurs in the text -- <prefix>.ms.ptr and <prefix>.ms.len, the\n"
                    "                        reads one after the other, and <prefix>.ms.off (reads + 1 offsets into them); same width as .ssa\n"
                    "    --mems <L>          (extension) with --ms: the maximal exact matches of at least L bases of every read (0: 1), read off its\n"
                    "                        matching statistics on the device -- <prefix>.mem.start (where the match starts in its read), <prefix>.mem.len\n"
                    "                        and <prefix>.mem.ptr (a text position where it occurs), one value per match, the reads one after the other,\n"
                    "                        same width as .ssa, and <prefix>.mem.off (reads + 1 values, 64 bit: the matches in front of every read)\n"
                    "    --mems-locate       (extension) with --mems: also where every match occurs -- <prefix>.mem.cnt (occurrences per match),\n"
                    "                        <prefix>.mem.pos (their text positions in suffix order, the matches one after the other, same width as\n"
                    "                        .ssa) and <prefix>.mem.poff (matches + 1 offsets into .mem.pos, 64 bit)\n"
                    "    --mems-max <K>      (extension) with --mems-locate: at most K positions per match, those of the last K rows of its interval [default: all]\n"
                    "    --count <reads>     (extension) how often every read of a FASTA / FASTQ file (plain or gzip) occurs in the text, needs -r:\n"
                    "                        <prefix>.cnt, one value per read, same width as .ssa; answered from the run samples alone, so also with\n"
                    "                        --pfbwt-only and without -s / --thr\n"
                    "    --locate <reads>    (extension) where every read occurs, needs -r: <prefix>.loc.cnt (as .cnt), <prefix>.loc.pos (the text positions\n"
                    "                        of the occurrences in suffix order, the reads one after the other, same width as .ssa) and <prefix>.loc.off\n"
                    "                        (reads + 1 offsets into .loc.pos, 64 bit)\n"
                    "    --locate-max <K>    (extension) with --locate: at most K positions per read, those of the last K rows of its interval [default: all]\n"
                    "    --doclist <reads>   (extension) in which records every read occurs and how often in each, needs -r: <prefix>.dl.cnt (as .cnt),\n"
                    "                        <prefix>.dl.doc (the records with an occurrence, ascending) and <prefix>.dl.freq (the occurrences in each),\n"
                    "                        the reads one after the other, same width as .ssa, and <prefix>.dl.off (reads + 1 offsets into them, 64 bit);\n"
                    "                        the positions never leave the device; with --pfbwt-only the records come from <prefix>.docs\n"
                    "    --doclist-inside    (extension) with --doclist: only occurrences that lie inside their record without touching its pad count\n"
                    "    --doclist-max <K>   (extension) with --doclist: a read that occurs more than K times is skipped (no records listed) [default: no limit]\n"
                    "    --mps <file>        (extension) marker array of a marker-positions stream (.mps) on the device, as mps_to_ma writes it: <prefix>.ma;\n"
                    "                        builds the SA on the device also without -s (no .sa is written then)\n"
                    "    --ma <file>         (extension) a ready marker array (.ma) for --markers: needs no SA, so also with -r alone and --pfbwt-only\n"
                    "    --markers <reads>   (extension) which markers the occurrences of every read overlap and in how many rows each, needs -r and one of\n"
                    "                        --mps / --ma: <prefix>.mk.cnt (as .cnt) and <prefix>.mk.probes (the suffixes of the read that were looked up), same\n"
                    "                        width as .ssa, <prefix>.mk.marker (the markers, ascending) and <prefix>.mk.freq (the rows that carry each), the reads\n"
                    "                        one after the other, and <prefix>.mk.off (reads + 1 offsets into them), 64 bit; nothing is located\n"
                    "    --markers-min-len <L> (extension) with --markers: every suffix of a read of at least L bases is looked up [default: the whole read only]\n"
                    "    --markers-max-rows <K> (extension) with --markers: a suffix that occurs more than K times contributes nothing [default: no limit]\n"
                    "    --vcf <file>        (extension) build the index of a variant panel: <fasta file> is the reference, <file> a text VCF (plain or gzip)\n"
                    "                        with phased or unphased diploid genotypes; the reference's records come first, then for every sample its two\n"
                    "                        haplotypes (records <sample>.0.<contig>, <sample>.1.<contig>), expanded on the device; a site that starts inside\n"
                    "                        the previous kept site is skipped, a line with a symbolic ALT is dropped; works with every other option but\n"
                    "                        --gpus, --pfbwt-only and stdin input\n"
                    "    --vcf-samples <list> (extension) with --vcf: only these samples, comma separated, in this order [default: all, in file order]\n"
                    "    --vcf-no-ref        (extension) with --vcf: without the reference's own records in front\n"
                    "    --gpus <int>        (extension) shard the records of a plain FASTA file over <int> devices of this node: sharded parse,\n"
                    "                        one RCCL all-gather of dictionaries, sliced emission; writes .bwt [.sa .ssa .esa] only\n"
                    "    --devices <list>    (extension) the device ids to use with --gpus, comma separated [default: 0,1,...]\n"
                    "    -h                  print this help message\n");
}

Options parse_options(int argc, char **argv)
{
    Options o;
    fputs("==== Command line:", stderr);
    for (int i = 0; i < argc; ++i) fprintf(stderr, " %s", argv[i]);
    fputs("\n", stderr);
    static struct option lopts[] = {{"parse-only", no_argument, NULL, 1000}, {"pfbwt-only", no_argument, NULL, 1001}, {"trim-non-acgt", no_argument, NULL, 1002},
                                    {"non-acgt-to-a", no_argument, NULL, 1003}, {"print-docs", no_argument, NULL, 1004}, {"stdout", required_argument, NULL, 'c'},
                                    {"verbose", no_argument, NULL, 1005}, {"sa", no_argument, NULL, 's'}, {"rssa", no_argument, NULL, 'r'}, {"mmap", no_argument, NULL, 'm'},
                                    {"output", required_argument, NULL, 'o'}, {"gpus", required_argument, NULL, 1006}, {"devices", required_argument, NULL, 1007}, {"da", no_argument, NULL, 1008}, {"lcp", no_argument, NULL, 1009}, {"thr", no_argument, NULL, 1010}, {"thr-window", required_argument, NULL, 1011}, {"ms", required_argument, NULL, 1012}, {"count", required_argument, NULL, 1013}, {"locate", required_argument, NULL, 1014}, {"locate-max", required_argument, NULL, 1015}, {"mems", required_argument, NULL, 1016}, {"mems-locate", no_argument, NULL, 1017}, {"mems-max", required_argument, NULL, 1018}, {"doclist", required_argument, NULL, 1019}, {"doclist-inside", no_argument, NULL, 1020}, {"doclist-max", required_argument, NULL, 1021}, {"mps", required_argument, NULL, 1022}, {"ma", required_argument, NULL, 1023}, {"markers", required_argument, NULL, 1024}, {"markers-min-len", required_argument, NULL, 1025}, {"markers-max-rows", required_argument, NULL, 1026}, {"vcf", required_argument, NULL, 1027}, {"vcf-samples", required_argument, NULL, 1028}, {"vcf-no-ref", no_argument, NULL, 1029}, {"window-size", required_argument, NULL, 'w'}, {"mod-val", required_argument, NULL, 'p'}, {0, 0, 0, 0}};
    int c;
    while ((c = getopt_long(argc, argv, "w:p:o:c:hsrfm", lopts, NULL)) != -1) {
        switch (c) {
        case 1000: o.parse_only = 1; break;
        case 1001: o.pfbwt_only = 1; break;
        case 1002: o.trim_non_acgt = 1; break;
        case 1003: o.non_acgt_to_a = 1; break;
        case 1004: o.print_docs = 1; break;
        case 1005: o.verbose = 1; break;
        case 1006: o.gpus = atoi(optarg); break;
        case 1007: o.devices = optarg; break;
        case 1008: o.da = 1; break;
        case 1009: o.lcp = 1; break;
        case 1010: o.thr = 1; break;
        case 1011: o.thr_windowed = 1; o.thr_window = strtoull(optarg, NULL, 10); break;
        case 1012: o.ms = optarg; break;
        case 1013: o.count = optarg; break;
        case 1014: o.locate = optarg; break;
        case 1015: o.locate_max = strtoull(optarg, NULL, 10); o.have_locate_max = 1; break;
        case 1016: o.mems = strtoull(optarg, NULL, 10); o.have_mems = 1; break;
        case 1017: o.mems_locate = 1; break;
        case 1018: o.mems_max = strtoull(optarg, NULL, 10); o.have_mems_max = 1; break;
        case 1019: o.doclist = optarg; break;
        case 1020: o.doclist_inside = 1; break;
        case 1021: o.doclist_max = strtoull(optarg, NULL, 10); o.have_doclist_max = 1; break;
        case 1022: o.mps = optarg; break;
        case 1023: o.ma = optarg; break;
        case 1024: o.markers = optarg; break;
        case 1025: o.markers_min_len = strtoull(optarg, NULL, 10); o.have_markers_min_len = 1; break;
        case 1026: o.markers_max_rows = strtoull(optarg, NULL, 10); o.have_markers_max_rows = 1; break;
        case 1027: o.vcf = optarg; break;
        case 1028: o.vcf_samples = optarg; break;
        case 1029: o.vcf_no_ref = 1; break;
        case 'f': break;
        case 's': o.sa = 1; break;
        case 'r': o.rssa = 1; break;
        case 'w': o.w = (size_t)atoi(optarg); break;
        case 'm': o.mmap = 1; break;
        case 'p': o.p = (size_t)atoi(optarg); break;
        case 'h': usage(); exit(0);
        case 'o': o.output.assign(optarg); break;
        case 'c': o.stdout_ext = optarg; break;
        default: fprintf(stderr, "Unknown option. Use -h for help.\n"); exit(1);
        }
    }
    if (argc == optind + 1) o.in_fname.assign(argv[optind]);
    else { fprintf(stderr, "reading from stdin. Parsing might be a bit slow.\n"); o.in_fname.assign("-"); }
    if (o.non_acgt_to_a && o.trim_non_acgt) die("cannot have both --non-acgt-to-a and --trim-non-acgt options enabled at same time");
    if (o.in_fname == "-" && o.output == "" && !o.pfbwt_only) die("if reading from stdin, need a prefix for output files (-o, --output)");
    if (o.in_fname != "-" && o.output == "") o.output = o.in_fname;
    if (o.parse_only && o.pfbwt_only) die("cannot simulatneously do parse_only and pfbwt_only");
    if (o.da && o.gpus) die("--da is not available with --gpus (the C API pfp_doc_array works on every rank of a sharded build)");
    if (o.da && o.parse_only) die("--da needs the BWT build: not with --parse-only");
    if (o.da && !o.sa && !o.rssa) die("--da needs -s (writes .da) and/or -r (writes .sda and .eda)");
    if (o.lcp && o.gpus) die("--lcp is not available with --gpus (no rank holds the whole text)");
    if (o.lcp && o.parse_only) die("--lcp needs the BWT build: not with --parse-only");
    if (o.lcp && o.pfbwt_only) die("--lcp needs the text, which a --pfbwt-only process does not have: build parse and BWT in one run");
    if (o.lcp && !o.sa && !o.rssa) die("--lcp needs -s (writes .lcp) and/or -r (writes .slcp)");
    if (o.thr && o.gpus) die("--thr is not available with --gpus (no rank holds the whole text)");
    if (o.thr && o.parse_only) die("--thr needs the BWT build: not with --parse-only");
    if (o.thr && o.pfbwt_only) die("--thr needs the text, which a --pfbwt-only process does not have: build parse and BWT in one run");
    if (o.thr && !o.rssa) die("--thr needs -r (one threshold per run: writes .thr and .tlcp)");
    if (o.thr_windowed && !o.thr) die("--thr-window needs --thr (it selects the windowed route of the thresholds)");
    if (!o.ms.empty() && o.gpus) die("--ms is not available with --gpus (no rank holds the whole text)");
    if (!o.ms.empty() && o.parse_only) die("--ms needs the BWT build: not with --parse-only");
    if (!o.ms.empty() && o.pfbwt_only) die("--ms needs the text, which a --pfbwt-only process does not have: build parse and BWT in one run");
    if (!o.ms.empty() && (!o.rssa || !o.thr)) die("--ms needs -r --thr (the run samples and thresholds are its index)");
    if (o.have_mems && o.ms.empty()) die("--mems needs --ms (the maximal exact matches are read off the matching statistics of its reads)");
    if (o.mems_locate && !o.have_mems) die("--mems-locate needs --mems (it lists the occurrences of the matches)");
    if (o.have_mems_max && !o.have_mems) die("--mems-max needs --mems --mems-locate (it caps the positions listed per match)");
    if (o.have_mems_max && !o.mems_locate) die("--mems-max needs --mems-locate (it caps the positions listed per match)");
    auto needs_run_samples = [&](const char *opt, const std::string &reads) {      // --count / --locate: the same three refusals
        if (reads.empty()) return;
        const std::string name(opt);
        if (o.gpus) die((name + " is not available with --gpus (no rank holds all run samples)").c_str());
        if (o.parse_only) die((name + " needs the BWT build: not with --parse-only").c_str());
        if (!o.rssa) die((name + " needs -r (the run samples are its index)").c_str());
    };
    needs_run_samples("--count", o.count);
    needs_run_samples("--locate", o.locate);
    needs_run_samples("--doclist", o.doclist);
    if (o.doclist_inside && o.doclist.empty()) die("--doclist-inside needs --doclist (it restricts the occurrences that are listed)");
    if (o.have_doclist_max && o.doclist.empty()) die("--doclist-max needs --doclist (it skips the reads that occur more often)");
    needs_run_samples("--markers", o.markers);
    if (!o.markers.empty() && o.mps.empty() && o.ma.empty()) die("--markers needs a marker array: --mps <file> (made on the device) or --ma <file>");
    if (o.have_markers_min_len && o.markers.empty()) die("--markers-min-len needs --markers (it selects the suffixes of the reads that are looked up)");
    if (o.have_markers_max_rows && o.markers.empty()) die("--markers-max-rows needs --markers (it drops the suffixes that occur more often)");
    if (!o.mps.empty() && !o.ma.empty()) die("--mps and --ma exclude one another (one marker array per run)");
    if (!o.mps.empty() && o.gpus) die("--mps is not available with --gpus (no rank holds the whole SA)");
    if (!o.mps.empty() && o.parse_only) die("--mps needs the BWT build: not with --parse-only");
    if (!o.ma.empty() && o.markers.empty()) die("--ma needs --markers (a ready marker array is only read for the query)");
    if (o.have_locate_max && o.locate.empty()) die("--locate-max needs --locate (it caps the positions listed per read)");
    if (!o.vcf.empty() && o.gpus) die("--vcf is not available with --gpus (every rank expanding its own haplotypes is not built yet)");
    if (!o.vcf.empty() && o.pfbwt_only) die("--vcf is an input of the parse: not with --pfbwt-only");
    if (!o.vcf.empty() && o.in_fname == "-") die("--vcf needs the reference FASTA as a file argument, not stdin");
    if (o.vcf.empty() && (!o.vcf_samples.empty() || o.vcf_no_ref)) die("--vcf-samples and --vcf-no-ref need --vcf");
    if (o.gpus && (o.parse_only || o.pfbwt_only || o.in_fname == "-" || o.print_docs)) die("--gpus builds the index of a plain FASTA file in one go (no --parse-only / --pfbwt-only / stdin / --print-docs)");
    return o;
}

FILE *open_out(const Options &o, const char *ext)
{
    if (o.stdout_ext == ext) return stdout;
    std::string name = o.output + "." + ext;
    FILE *f = fopen(name.c_str(), "wb");
    if (f == NULL) die(name.c_str());
    return f;
}

using parser_t = pfbwtf::PfParser<WangHash>;

/* saves dict, occs, ilist, bwlast (and bwsai) to disk; returns the parser so that stage 2 can adopt its device state */
size_t run_parser(const Options &o, parser_t &p)
{
    size_t n = 0;
    fprintf(stderr, "starting...\n");
    { StageTimer t("TASK\tparsing input\t"); if (o.vcf.empty()) p.add_fasta(o.in_fname); else p.add_vcf(o.in_fname, o.vcf, o.vcf_samples, !o.vcf_no_ref); }
    {
        StageTimer t("TASK\tfinalizing parse, writing dict, occs, and ranks\t");
        p.finalize(); n = p.get_n();
        pfbwtf::save_parser(p, o.output);
    }
    {
        StageTimer t("TASK\tranking and bwt-ing parse and processing last-chars\t");
        p.bwt_of_parse([&](const std::vector<char> &bwlast, const std::vector<parser_t::UIntType> &ilist, const std::vector<parser_t::UIntType> &bwsai) {
            pfbwtf::vec_to_file<char>(bwlast, o.output + "." + EXTBWLST);
            pfbwtf::vec_to_file<parser_t::UIntType>(ilist, o.output + "." + EXTILIST);
            if (o.sa || o.rssa) pfbwtf::vec_to_file<parser_t::UIntType>(bwsai, o.output + "." + EXTBWSAI);
        });
    }
    FILE *nf = fopen((o.output + ".n").c_str(), "w");
    if (nf == NULL) die("n file");
    fprintf(nf, "%lu\n", (unsigned long)n);
    fclose(nf);
    return n;
}

size_t read_n_file(const std::string &prefix)
{
    FILE *f = fopen((prefix + ".n").c_str(), "r");
    unsigned long n = 0;
    if (f == NULL || fscanf(f, "%lu", &n) != 1) die("could not read '.n' file");
    fclose(f);
    return n;
}

template <template <typename, typename...> class R, template <typename, typename...> class W> void run_pfbwt(const Options &o, parser_t *parsed)
{
    using pfbwt_t = pfbwtf::PrefixFreeBWT<R, W>;
    pfbwtf::PrefixFreeBWTParams a;
    a.prefix = o.output; a.w = o.w; a.sa = o.sa || !o.mps.empty() || (o.thr && !o.thr_windowed) /* the thresholds need the SA on the device (.sa is written only with -s) -- unless they visit it window by window */; a.rssa = o.rssa; a.verb = o.verbose;
    size_t n = o.n;
    if (!n) { fprintf(stderr, "reading n from file\n"); n = read_n_file(o.output); }
    std::vector<uint64_t> doc_starts;      // --da: record starts b_k, from this run's parse or from <prefix>.docs
    if (o.da || !o.doclist.empty()) {
        if (parsed) for (auto s : parsed->get_doc_starts()) doc_starts.push_back((uint64_t)s);
        else {
            const std::string docs = o.output + ".docs";
            if (!pfbwtf::file_exists(docs)) { fprintf(stderr, "%s with --pfbwt-only needs %s (write it with --parse-only --print-docs)\n", o.da ? "--da" : "--doclist", docs.c_str()); exit(1); }
            doc_starts = pfbwtf::load_doc_info<uint64_t>(docs).second;
        }
        if (doc_starts.empty()) die(o.da ? "--da: no records" : "--doclist: no records");
    }
    FILE *bwt_fp = open_out(o, "bwt");
    // in one process the parse is still resident on the device: adopt it instead of re-reading the files
    pfbwt_t *p = (parsed && parsed->engine() && parsed->parse_bwt_done()) ? new pfbwt_t(parsed->engine(), a) : new pfbwt_t(a, n);
    {
        StageTimer t((o.sa || o.rssa) ? "TASK\tgenerating final BWT w/ full and/or run-length SA\t" : "TASK\tgenerating final BWT w/o SA\t");
        // generate_bwt_lcp + out_fn, fused on the device; the outputs go from the device to the files in blocks
        FILE *sa_fp = o.sa ? open_out(o, "sa") : NULL, *ssa_fp = o.rssa ? open_out(o, "ssa") : NULL, *esa_fp = o.rssa ? open_out(o, "esa") : NULL;
        fflush(stdout);
        p->build_to_files(fileno(bwt_fp), sa_fp ? fileno(sa_fp) : -1, ssa_fp ? fileno(ssa_fp) : -1, esa_fp ? fileno(esa_fp) : -1);
        for (FILE *f : {bwt_fp, sa_fp, ssa_fp, esa_fp}) if (f && f != stdout) fclose(f);
    }
    if (o.da) {
        StageTimer t("TASK\tdocument array\t");
        pfp_ctx *ctx = p->engine();
        pfbwtf::engine_check(ctx, pfp_doc_array(ctx, doc_starts.data(), doc_starts.size(), (o.sa ? PFP_DA_ROWS : 0u) | (o.rssa ? PFP_DA_RUNS : 0u)), "pfp_doc_array");
        FILE *da_fp = o.sa ? open_out(o, "da") : NULL, *sda_fp = o.rssa ? open_out(o, "sda") : NULL, *eda_fp = o.rssa ? open_out(o, "eda") : NULL;
        fflush(stdout);
        pfbwtf::engine_check(ctx, pfp_doc_array_write(ctx, da_fp ? fileno(da_fp) : -1, sda_fp ? fileno(sda_fp) : -1, eda_fp ? fileno(eda_fp) : -1), "pfp_doc_array_write");
        for (FILE *f : {da_fp, sda_fp, eda_fp}) if (f && f != stdout) fclose(f);
    }
    if (o.lcp) {
        StageTimer t("TASK\tLCP array\t");
        pfp_ctx *ctx = p->engine();
        pfbwtf::engine_check(ctx, pfp_lcp_array(ctx, (o.sa ? PFP_LCP_ROWS : 0u) | (o.rssa ? PFP_LCP_RUNS : 0u), NULL), "pfp_lcp_array");
        FILE *lcp_fp = o.sa ? open_out(o, "lcp") : NULL, *slcp_fp = o.rssa ? open_out(o, "slcp") : NULL;
        fflush(stdout);
        pfbwtf::engine_check(ctx, pfp_lcp_array_write(ctx, lcp_fp ? fileno(lcp_fp) : -1, slcp_fp ? fileno(slcp_fp) : -1), "pfp_lcp_array_write");
        for (FILE *f : {lcp_fp, slcp_fp}) if (f && f != stdout) fclose(f);
    }
    if (o.thr) {
        StageTimer t("TASK\tthresholds\t");
        pfp_ctx *ctx = p->engine();
        if (o.thr_windowed) pfbwtf::engine_check(ctx, pfp_thresholds_windowed(ctx, o.thr_window, NULL, NULL), "pfp_thresholds_windowed");      // after --lcp -r: on the values it left
        else pfbwtf::engine_check(ctx, pfp_thresholds(ctx, NULL), "pfp_thresholds");      // after --lcp -s: on the rows it left
        FILE *thr_fp = open_out(o, "thr"), *tlcp_fp = open_out(o, "tlcp");
        fflush(stdout);
        pfbwtf::engine_check(ctx, pfp_thresholds_write(ctx, fileno(thr_fp), fileno(tlcp_fp)), "pfp_thresholds_write");
        for (FILE *f : {thr_fp, tlcp_fp}) if (f && f != stdout) fclose(f);
    }
    if (!o.ms.empty()) {
        StageTimer t("TASK\tmatching statistics\t");
        pfp_ctx *ctx = p->engine();
        pfbwtf::engine_check(ctx, pfp_ms_index(ctx), "pfp_ms_index");
        pfp_ms_info info;
        pfbwtf::engine_check(ctx, pfp_ms_query_file(ctx, o.ms.c_str(), &info), "pfp_ms_query_file");
        std::vector<uint64_t> off((size_t)info.patterns + 1);
        pfbwtf::engine_check(ctx, pfp_ms_offsets_get(ctx, off.data(), NULL), "pfp_ms_offsets_get");
        std::vector<uint_t> offu(off.begin(), off.end());
        FILE *ptr_fp = open_out(o, "ms.ptr"), *len_fp = open_out(o, "ms.len"), *off_fp = open_out(o, "ms.off");
        fflush(stdout);
        pfbwtf::engine_check(ctx, pfp_ms_write(ctx, fileno(ptr_fp), fileno(len_fp)), "pfp_ms_write");
        if (fwrite(offu.data(), sizeof(uint_t), offu.size(), off_fp) != offu.size()) die("error writing .ms.off");
        for (FILE *f : {ptr_fp, len_fp, off_fp}) if (f && f != stdout) fclose(f);
        fprintf(stderr, "ms: %lu reads, %lu bases, %lu breaks, longest match %lu\n", (unsigned long)info.patterns, (unsigned long)info.bases, (unsigned long)info.breaks, (unsigned long)info.max_len);
    }
    uint64_t ma_words = 0;      // --mps: the words of the marker array it left on the device
    if (!o.mps.empty()) {
        StageTimer t("TASK\tmarker array\t");
        pfp_ctx *ctx = p->engine();
        std::vector<uint64_t> mps = pfbwtf::read_vec<uint64_t>(o.mps);
        uint64_t words = 0;
        pfbwtf::engine_check(ctx, pfp_marker_array(ctx, mps.data(), mps.size(), NULL, 0, &words), "pfp_marker_array");
        std::vector<uint64_t> out(words);
        pfbwtf::engine_check(ctx, pfp_marker_array_get(ctx, out.data()), "pfp_marker_array_get");
        ma_words = words;
        FILE *ma_fp = open_out(o, "ma");
        if (words && fwrite(out.data(), 8, words, ma_fp) != words) die("error writing .ma");
        if (ma_fp != stdout) fclose(ma_fp);
    }
    if (!o.count.empty() || !o.locate.empty() || o.mems_locate || !o.doclist.empty() || !o.markers.empty()) pfbwtf::engine_check(p->engine(), pfp_ri_index(p->engine()), "pfp_ri_index");
    if (o.have_mems) {
        StageTimer t("TASK\tmems\t");
        pfp_ctx *ctx = p->engine();
        pfp_mem_info info;
        pfbwtf::engine_check(ctx, pfp_mem_find(ctx, o.mems, o.mems_locate, o.mems_max, &info), "pfp_mem_find");
        std::vector<uint64_t> off((size_t)info.patterns + 1), poff(o.mems_locate ? (size_t)info.mems + 1 : 0);
        pfbwtf::engine_check(ctx, pfp_mem_offsets_get(ctx, off.data(), NULL, o.mems_locate ? poff.data() : NULL, NULL), "pfp_mem_offsets_get");
        FILE *start_fp = open_out(o, "mem.start"), *len_fp = open_out(o, "mem.len"), *ptr_fp = open_out(o, "mem.ptr"), *off_fp = open_out(o, "mem.off");
        FILE *cnt_fp = o.mems_locate ? open_out(o, "mem.cnt") : NULL, *pos_fp = o.mems_locate ? open_out(o, "mem.pos") : NULL, *poff_fp = o.mems_locate ? open_out(o, "mem.poff") : NULL;
        fflush(stdout);
        pfbwtf::engine_check(ctx, pfp_mem_write(ctx, fileno(start_fp), fileno(len_fp), fileno(ptr_fp), cnt_fp ? fileno(cnt_fp) : -1, pos_fp ? fileno(pos_fp) : -1), "pfp_mem_write");
        if (fwrite(off.data(), 8, off.size(), off_fp) != off.size()) die("error writing .mem.off");
        if (poff_fp && fwrite(poff.data(), 8, poff.size(), poff_fp) != poff.size()) die("error writing .mem.poff");
        for (FILE *f : {start_fp, len_fp, ptr_fp, off_fp, cnt_fp, pos_fp, poff_fp}) if (f && f != stdout) fclose(f);
        fprintf(stderr, "mems: %lu reads, %lu matches of %lu bases and more, longest %lu", (unsigned long)info.patterns, (unsigned long)info.mems, (unsigned long)(o.mems ? o.mems : 1), (unsigned long)info.max_len);
        if (o.mems_locate) fprintf(stderr, ", %lu occurrences, %lu positions listed", (unsigned long)info.occurrences, (unsigned long)info.reported);
        fputs("\n", stderr);
    }
    if (!o.count.empty()) {
        StageTimer t("TASK\tcount\t");
        pfp_ctx *ctx = p->engine();
        pfp_ri_info info;
        pfbwtf::engine_check(ctx, pfp_ri_query_file(ctx, o.count.c_str(), 0, 0, &info), "pfp_ri_query_file");
        FILE *cnt_fp = open_out(o, "cnt");
        fflush(stdout);
        pfbwtf::engine_check(ctx, pfp_ri_write(ctx, fileno(cnt_fp), -1, -1), "pfp_ri_write");
        if (cnt_fp != stdout) fclose(cnt_fp);
        fprintf(stderr, "count: %lu reads, %lu found, %lu occurrences\n", (unsigned long)info.patterns, (unsigned long)info.found, (unsigned long)info.occurrences);
    }
    if (!o.locate.empty()) {
        StageTimer t("TASK\tlocate\t");
        pfp_ctx *ctx = p->engine();
        pfp_ri_info info;
        pfbwtf::engine_check(ctx, pfp_ri_query_file(ctx, o.locate.c_str(), 1, o.locate_max, &info), "pfp_ri_query_file");
        FILE *cnt_fp = open_out(o, "loc.cnt"), *off_fp = open_out(o, "loc.off"), *pos_fp = open_out(o, "loc.pos");
        fflush(stdout);
        pfbwtf::engine_check(ctx, pfp_ri_write(ctx, fileno(cnt_fp), fileno(off_fp), fileno(pos_fp)), "pfp_ri_write");
        for (FILE *f : {cnt_fp, off_fp, pos_fp}) if (f && f != stdout) fclose(f);
        fprintf(stderr, "locate: %lu reads, %lu found, %lu occurrences, %lu positions listed\n", (unsigned long)info.patterns, (unsigned long)info.found, (unsigned long)info.occurrences, (unsigned long)info.reported);
    }
    if (!o.doclist.empty()) {
        StageTimer t("TASK\tdoclist\t");
        pfp_ctx *ctx = p->engine();
        pfp_dl_info info;
        pfbwtf::engine_check(ctx, pfp_ri_docs_file(ctx, o.doclist.c_str(), doc_starts.data(), doc_starts.size(), o.doclist_inside ? PFP_DL_INSIDE : 0u, o.doclist_max, &info), "pfp_ri_docs_file");
        FILE *cnt_fp = open_out(o, "dl.cnt"), *off_fp = open_out(o, "dl.off"), *doc_fp = open_out(o, "dl.doc"), *freq_fp = open_out(o, "dl.freq");
        fflush(stdout);
        pfbwtf::engine_check(ctx, pfp_ri_docs_write(ctx, fileno(cnt_fp), fileno(off_fp), fileno(doc_fp), fileno(freq_fp)), "pfp_ri_docs_write");
        for (FILE *f : {cnt_fp, off_fp, doc_fp, freq_fp}) if (f && f != stdout) fclose(f);
        fprintf(stderr, "doclist: %lu reads, %lu found, %lu occurrences, %lu listed, %lu pairs, %lu skipped, %lu outside\n", (unsigned long)info.patterns, (unsigned long)info.found, (unsigned long)info.occurrences,
                (unsigned long)info.listed, (unsigned long)info.entries, (unsigned long)info.skipped, (unsigned long)info.outside);
    }
    if (!o.markers.empty()) {
        StageTimer t("TASK\tmarkers\t");
        pfp_ctx *ctx = p->engine();
        if (!o.ma.empty()) {
            std::vector<uint64_t> ma = pfbwtf::read_vec<uint64_t>(o.ma);
            uint64_t none = 0;
            pfbwtf::engine_check(ctx, pfp_mk_index(ctx, ma.empty() ? &none : ma.data(), ma.size(), NULL), "pfp_mk_index");
        } else {
            uint64_t none = 0;      // (no marker on any row: an empty index, which only a host stream can name)
            pfbwtf::engine_check(ctx, ma_words ? pfp_mk_index(ctx, NULL, 0, NULL) : pfp_mk_index(ctx, &none, 0, NULL), "pfp_mk_index");
        }
        pfp_mk_info info;
        pfbwtf::engine_check(ctx, pfp_mk_query_file(ctx, o.markers.c_str(), o.markers_min_len, o.markers_max_rows, &info), "pfp_mk_query_file");
        FILE *cnt_fp = open_out(o, "mk.cnt"), *probes_fp = open_out(o, "mk.probes"), *off_fp = open_out(o, "mk.off"), *marker_fp = open_out(o, "mk.marker"), *freq_fp = open_out(o, "mk.freq");
        fflush(stdout);
        pfbwtf::engine_check(ctx, pfp_mk_write(ctx, fileno(cnt_fp), fileno(probes_fp), fileno(off_fp), fileno(marker_fp), fileno(freq_fp)), "pfp_mk_write");
        for (FILE *f : {cnt_fp, probes_fp, off_fp, marker_fp, freq_fp}) if (f && f != stdout) fclose(f);
        fprintf(stderr, "markers: %lu reads, %lu found, %lu probes, %lu capped, %lu listed, %lu pairs\n", (unsigned long)info.patterns, (unsigned long)info.found, (unsigned long)info.probes, (unsigned long)info.capped,
                (unsigned long)info.listed, (unsigned long)info.entries);
    }
    fprintf(stderr, "# easy cases: %lu, # hard cases: %lu\n", (unsigned long)p->easy_cases(), (unsigned long)p->hard_cases());
    fprintf(stderr, "n: %lu\n", (unsigned long)n);
    fprintf(stderr, "r: %lu\n", (unsigned long)p->runs());
    fprintf(stderr, "n/r: %.3f\n", static_cast<double>(n) / (double)p->runs());
    delete p;
}

/* --gpus N (extension; the reference parallelises only merge_pfp, one PfParser per std::thread, src/merge_pfp.cpp:131-152): the
 * records of a plain FASTA file are cut into N runs of whole records of about equal size, rank r's run goes to device r
 * (pfp_parse_feed_fasta on its own host thread), pfp_sharded_build does the rest; the slices are appended to the output files in
 * rank order -- the same .bwt / .sa / .ssa / .esa as the single-device build. */
void run_sharded(const Options &o)
{
    std::vector<int> dev;
    for (size_t i = 0; i < o.devices.size();) { size_t j = o.devices.find(',', i); if (j == std::string::npos) j = o.devices.size(); dev.push_back(atoi(o.devices.substr(i, j - i).c_str())); i = j + 1; }
    if (!dev.empty() && (int)dev.size() != o.gpus) die("--devices must name --gpus devices");
    const int fd = open(o.in_fname.c_str(), O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode) || sb.st_size < 2) die(o.in_fname.c_str());
    const size_t fsz = (size_t)sb.st_size;
    const uint8_t *raw = (const uint8_t *)mmap(NULL, fsz, PROT_READ, MAP_PRIVATE, fd, 0);
    if (raw == MAP_FAILED) die("mmap");
    if (raw[0] == 0x1f && raw[1] == 0x8b) die("--gpus needs a plain (not gzip-compressed) FASTA file");
    std::vector<size_t> cut((size_t)o.gpus + 1, fsz);
    cut[0] = 0;
    for (int r = 1; r < o.gpus; ++r) {      // first record start at or behind r / N of the file (a '>' at a line start)
        size_t q = fsz / (size_t)o.gpus * (size_t)r;
        if (q < cut[(size_t)r - 1]) q = cut[(size_t)r - 1];
        while (q < fsz) { const uint8_t *nl = (const uint8_t *)memchr(raw + q, '\n', fsz - q); if (!nl) { q = fsz; break; } q = (size_t)(nl - raw) + 1; if (q < fsz && raw[q] == '>') break; }
        cut[(size_t)r] = q;
    }
    // fewer records than devices (or records of very different sizes): runs without a record are dropped, the build uses fewer ranks
    std::vector<size_t> cuts2; cuts2.push_back(0);
    for (int r = 1; r <= o.gpus; ++r) if (cut[(size_t)r] > cuts2.back()) cuts2.push_back(cut[(size_t)r]);
    if ((int)cuts2.size() - 1 < o.gpus) fprintf(stderr, "only %d run(s) of whole records: using %d device(s)\n", (int)cuts2.size() - 1, (int)cuts2.size() - 1);
    cut = cuts2;
    const_cast<Options &>(o).gpus = (int)cut.size() - 1;
    if (!dev.empty()) dev.resize((size_t)o.gpus);
    int st = 0;
    const unsigned flags = (M64 ? PFP_FLAG_U64 : 0u) | (o.non_acgt_to_a ? PFP_FLAG_NON_ACGT_TO_A : 0u) | ((o.sa || o.rssa) ? PFP_FLAG_SAI : 0u);
    pfp_sharded *sh = pfp_sharded_create((int)o.w, o.p, flags, o.gpus, dev.empty() ? NULL : dev.data(), 0, &st);
    if (!sh) { fprintf(stderr, "pfp_sharded_create: %s\n", pfp_strerror(st)); exit(1); }
    {
        StageTimer t("TASK\tparsing input\t");
        std::vector<int> rc((size_t)o.gpus, PFP_OK);
        std::vector<std::thread> th;
        auto feed = [&](int r) { uint64_t nrec = 0; if (cut[(size_t)r + 1] > cut[(size_t)r]) rc[(size_t)r] = pfp_parse_feed_fasta(pfp_sharded_ctx(sh, r), raw + cut[(size_t)r], cut[(size_t)r + 1] - cut[(size_t)r], PFP_FASTA_FINAL, &nrec); };
        const bool threads = !strcmp(pfp_backend(), "hip-gfx950");      // (the CPU interpreter of the tests runs one kernel at a time)
        for (int r = 0; r < o.gpus; ++r) { if (threads) th.emplace_back(feed, r); else feed(r); }
        for (auto &x : th) x.join();
        for (int r = 0; r < o.gpus; ++r) pfbwtf::engine_check(pfp_sharded_ctx(sh, r), rc[(size_t)r], "pfp_parse_feed_fasta");
    }
    pfp_parse_sizes ps; std::vector<pfp_bwt_sizes> bs((size_t)o.gpus);
    {
        StageTimer t((o.sa || o.rssa) ? "TASK\tgenerating final BWT w/ full and/or run-length SA\t" : "TASK\tgenerating final BWT w/o SA\t");
        st = pfp_sharded_build(sh, o.sa, o.rssa, &ps, bs.data(), NULL, NULL, NULL);
        if (st != PFP_OK) { for (int r = 0; r < o.gpus; ++r) if (st == PFP_E_INVALID_CHAR) pfbwtf::engine_check(pfp_sharded_ctx(sh, r), PFP_OK, ""); fprintf(stderr, "pfp_sharded_build: %s [%s]\n", pfp_strerror(st), pfp_sharded_error(sh)); exit(1); }
        FILE *bwt_fp = open_out(o, "bwt"), *sa_fp = o.sa ? open_out(o, "sa") : NULL, *ssa_fp = o.rssa ? open_out(o, "ssa") : NULL, *esa_fp = o.rssa ? open_out(o, "esa") : NULL;
        fflush(stdout);
        for (int r = 0; r < o.gpus; ++r)      // slice r behind slice r - 1
            pfbwtf::engine_check(pfp_sharded_ctx(sh, r), pfp_bwt_write(pfp_sharded_ctx(sh, r), fileno(bwt_fp), sa_fp ? fileno(sa_fp) : -1, ssa_fp ? fileno(ssa_fp) : -1, esa_fp ? fileno(esa_fp) : -1), "pfp_bwt_write");
        for (FILE *f : {bwt_fp, sa_fp, ssa_fp, esa_fp}) if (f && f != stdout) fclose(f);
    }
    uint64_t r_tot = 0, easy = 0, hard = 0;
    for (auto &b : bs) { r_tot += b.r; easy += b.easy_cases; hard += b.hard_cases; }
    FILE *nf = fopen((o.output + ".n").c_str(), "w");
    if (nf == NULL) die("n file");
    fprintf(nf, "%lu\n", (unsigned long)ps.n); fclose(nf);
    fprintf(stderr, "# easy cases: %lu, # hard cases: %lu\n", (unsigned long)easy, (unsigned long)hard);
    fprintf(stderr, "n: %lu\n", (unsigned long)ps.n);
    fprintf(stderr, "r: %lu\n", (unsigned long)r_tot);
    fprintf(stderr, "n/r: %.3f\n", static_cast<double>(ps.n) / (double)r_tot);
    pfp_sharded_destroy(sh);
    munmap((void *)raw, fsz); close(fd);
}

} // namespace

int main(int argc, char **argv)
{
    Options o = parse_options(argc, argv);
    if (o.gpus > 0) {
        fprintf(stderr, "sharded build over %d device(s)...\n", o.gpus);
        run_sharded(o);
        return 0;
    }
    pfbwtf::PfParserParams pp;
    pp.w = o.w; pp.p = o.p; pp.get_sai = o.sa || o.rssa || !o.mps.empty(); pp.verbose = o.verbose; pp.trim_non_acgt = o.trim_non_acgt; pp.non_acgt_to_a = o.non_acgt_to_a; pp.store_docs = o.print_docs; pp.collect_docs = o.da || !o.doclist.empty();
    parser_t parser(pp);
    bool have_parse = false;
    if (!o.pfbwt_only) {
        fprintf(stderr, "running parser...\n");
        o.n = run_parser(o, parser);
        have_parse = true;
    }
    if (!o.parse_only) {
        fprintf(stderr, "generating BWT using pfbwt algorithm...\n");
        fprintf(stderr, "workspace will be contained in device memory (HBM)\n");
        if (o.mmap) run_pfbwt<MMapFileSource, MMapFileSink>(o, have_parse ? &parser : nullptr);
        else run_pfbwt<VecFileSource, VecFileSinkPrivate>(o, have_parse ? &parser : nullptr);
    }
    return 0;
}
