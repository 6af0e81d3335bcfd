// pfbwt-f_amd/tools/vcfread_check.cpp -- TEST-ONLY stand-alone driver of csrc/vcfread.h for the sanitizer build (`make vcfread-asan`):
// parses a reference FASTA and a VCF exactly as pfp_parse_feed_vcf_file does and prints the counts, or the status and line of a
// refusal.  Host code only: it needs no GPU and is never loaded into another process.
//   usage: vcfread_check <ref.fa> <file.vcf[.gz]> [samples]
#include <cstdio>
#include "../csrc/vcfread.h"

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s <ref.fa> <file.vcf[.gz]> [samples]\n", argv[0]); return 2; }
    pfpvcf::Panel P;
    int rc = pfpvcf::load_fasta(argv[1], &P);
    if (rc != pfpvcf::VCF_OK) { printf("fasta status %d\n", rc); return 1; }
    uint64_t line = 0;
    rc = pfpvcf::load_vcf(argv[2], argc > 3 ? argv[3] : nullptr, &P, &line);
    if (rc != pfpvcf::VCF_OK) { printf("vcf status %d line %lu\n", rc, (unsigned long)line); return 1; }
    uint64_t gtsum = 0;
    for (uint8_t g : P.gt) gtsum += g;
    printf("contigs %zu ref %zu lines %lu samples %lu haplotypes %lu sites %zu alts %zu alt_bytes %zu gt %zu gtsum %lu skipped_symbolic %lu missing_gt %lu\n", P.contig_names.size(), P.ref.size(),
           (unsigned long)P.lines, (unsigned long)P.samples, (unsigned long)P.nhap, P.pos.size(), P.alt_off.size() - 1, P.alt_bytes.size(), P.gt.size(), (unsigned long)gtsum,
           (unsigned long)P.skipped_symbolic, (unsigned long)P.missing_gt);
    return 0;
}
