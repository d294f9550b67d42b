// Vcf.hpp -- the VCF of `real -vcf`: the header, and one line for a call record (real_hip_call, computed on the
// device: real_hip_call_*).  Fragment names and lengths are what -sam's @SQ lines carry (SamRefs).  Host code only, in the
// manner of Sam.hpp: nothing here calls into the library.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "Sam.hpp"
#include "real_hip.h"

// indels: the three ##INFO lines of -vcf_indels 1 behind DP's
inline std::string vcfHeader(const SamRefs &refs, bool indels = false)
{
    std::string h = "##fileformat=VCFv4.2\n";
    for (size_t f = 0; f < refs.names.size(); ++f)
        for (size_t k = 0; k < refs.names[f].size(); ++k)
            h += "##contig=<ID=" + refs.names[f][k] + ",length=" + std::to_string(refs.starts[f][k + 1] - refs.starts[f][k]) + ">\n";
    h += "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Depth of the placements, no quality filter\">\n";
    if (indels)
        h += "##INFO=<ID=INDEL,Number=0,Type=Flag,Description=\"An insertion or deletion shown by gap-rescued mates\">\n"
             "##INFO=<ID=SF,Number=1,Type=Integer,Description=\"Supporting mates on the forward strand\">\n"
             "##INFO=<ID=SR,Number=1,Type=Integer,Description=\"Supporting mates on the reverse strand\">\n";
    h += "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
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

// -vcf_indels 1: one indel call (real_hip_indel, computed on the device: real_hip_indel_*) whose anchor is 1-based
// position pos1 of the fragment `name`; sym: the genome file's symbols.  A deletion: REF = the anchor's base and the deleted
// bases, ALT = the anchor's base; an insertion: REF = the anchor's base, ALT = it and the inserted bases
inline void writeVcfIndelLine(FILE *f, const std::string &name, uint64_t pos1, const real_hip_indel &c, const uint8_t *sym)
{
    const char anchor = "ACGT"[c.ref & 3u];
    std::string ref(1, anchor), alt(1, anchor);
    for (int k = 0; k < c.gap; ++k) ref += "ACGTN"[sym[(uint64_t)c.pos + 1 + k] > 3 ? 4 : sym[(uint64_t)c.pos + 1 + k]];
    for (int k = 0; k < -c.gap; ++k) alt += "ACGT"[(c.seq >> (2 * k)) & 3u];
    const unsigned long long dp = (unsigned long long)c.ref_n + c.alt_n;
    fprintf(f, "%s\t%llu\t.\t%s\t%s\t%u\t.\tDP=%llu;INDEL;SF=%u;SR=%u\tGT:GQ:DP:AD\t%s:%u:%llu:%u,%u\n", name.c_str(), (unsigned long long)pos1, ref.c_str(),
            alt.c_str(), c.qual, dp, c.alt_fwd, c.alt_n - c.alt_fwd, c.gt == 2 ? "1/1" : "0/1", (unsigned)c.gq, dp, c.ref_n, c.alt_n);
}

// the lines of one genome file: its SNP calls and its indel calls (both in ascending text position) merged by position, the SNP
// line first at an equal one; names / frag_start: the file's fragments
inline void writeVcfMerged(FILE *f, const std::vector<std::string> &names, const uint64_t *frag_start, const uint8_t *sym, const real_hip_call *calls,
                           uint64_t n_calls, const real_hip_indel *indels, uint64_t n_indels)
{
    size_t fr = 0;
    uint64_t a = 0, b = 0;
    while (a < n_calls || b < n_indels) {
        const bool snp = b == n_indels || (a < n_calls && calls[a].pos <= indels[b].pos);
        const uint64_t pos = snp ? calls[a].pos : indels[b].pos;
        while (fr + 1 < names.size() && frag_start[fr + 1] <= pos) ++fr; // (ascending positions)
        if (snp) writeVcfLine(f, names[fr], pos - frag_start[fr] + 1, calls[a++]);
        else writeVcfIndelLine(f, names[fr], pos - frag_start[fr] + 1, indels[b++], sym);
    }
}
