// Vcf.hpp -- the VCF of `real -vcf`: the header, and one line for a call record (real_hip_call, computed on the
// device: real_hip_call_*).  Fragment names and lengths are what -sam's @SQ lines carry (SamRefs).  Host code only, in the
// manner of Sam.hpp: nothing here calls into the library.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <string>

#include "Sam.hpp"
#include "real_hip.h"

inline std::string vcfHeader(const SamRefs &refs)
{
    std::string h = "##fileformat=VCFv4.2\n";
    for (size_t f = 0; f < refs.names.size(); ++f)
        for (size_t k = 0; k < refs.names[f].size(); ++k)
            h += "##contig=<ID=" + refs.names[f][k] + ",length=" + std::to_string(refs.starts[f][k + 1] - refs.starts[f][k]) + ">\n";
    h += "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Depth of the placements, no quality filter\">\n"
         "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
         "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype quality\">\n"
         "##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"Bases of sufficient quality\">\n"
         "##FORMAT=<ID=AD,Number=R,Type=Integer,Description=\"Bases of sufficient quality per allele\">\n"
         "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsample\n";
    return h;
}

// one call at 1-based position pos1 of the fragment `name`: ALT is the genotype's non-reference alleles in ascending base
// order, GT is in allele indices (a1 <= a2 as bases; the reference is index 0, so the smaller index comes first), AD the counts
// of REF and then of each ALT
inline void writeVcfLine(FILE *f, const std::string &name, uint64_t pos1, const real_hip_call &c)
{
    unsigned alleles[3] = {c.ref, 0, 0}, n = 1;
    if (c.a1 != c.ref) alleles[n++] = c.a1;
    if (c.a2 != c.ref && c.a2 != c.a1) alleles[n++] = c.a2;
    auto index = [&](unsigned b) { for (unsigned k = 0; k < n; ++k) if (alleles[k] == b) return k; return 0u; };
    unsigned g1 = index(c.a1), g2 = index(c.a2);
    if (g1 > g2) { const unsigned t = g1; g1 = g2; g2 = t; }
    fprintf(f, "%s\t%llu\t.\t%c\t%c", name.c_str(), (unsigned long long)pos1, "ACGT"[c.ref & 3u], "ACGT"[alleles[1] & 3u]);
    if (n == 3) fprintf(f, ",%c", "ACGT"[alleles[2] & 3u]);
    fprintf(f, "\t%u\t.\tDP=%u\tGT:GQ:DP:AD\t%u/%u:%u:%u:%u,%u", c.qual, c.depth, g1, g2, (unsigned)c.gq, c.cnt[0] + c.cnt[1] + c.cnt[2] + c.cnt[3],
            c.cnt[c.ref & 3u], c.cnt[alleles[1] & 3u]);
    if (n == 3) fprintf(f, ",%u", c.cnt[alleles[2] & 3u]);
    fputc('\n', f);
}
