#include "RealOptions.hpp"

#include "real_hip.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>
#include <unistd.h>

bool RealOptions::isFastQ(const std::string &filename)
{
    std::ifstream istr(filename.c_str());
    if (!istr.is_open()) throw std::runtime_error("Unable to open pattern file.");
    int first = istr.get();
    if (first < 0) throw std::runtime_error("Failed to read first character from pattern file.");
    if (first == '>') return false;
    if (first == '@') return true;
    throw std::runtime_error("Unable to determine type of pattern file.");
}

SpoolFile::~SpoolFile()
{
    if (!path.empty()) unlink(path.c_str());
}

void RealOptions::printHelp() const
{
    std::cerr << "Options:\n"
              << "-t <textfilename: a .fa file, or a directory searched for .fa files>\n-p <patternfilename, - = standard input>\n-o <outputfilename, - = standard output>\n"
              << "-s <maximum number of errors in seed, default=2>\n"
              << "-e <total maximum number of errors, default=5>\n"
              << "-l <length of seed, default=32>\n"
              << "-u <search for unique match, default=1>\n"
              << "-f <fraction of device memory to use for the index, default=0.75>\n"
              << "-q <compute scores, default=1>\n-Q <quality offset, default=autodetect>\n"
              << "-filter_level <0..4, default=2>\n-similarity -err -trans -gc -gcmut_bias <scoring parameters>\n"
              << "-p2 <second pattern file: paired-end reads, read i of -p and of -p2 are mates (FR); one placement per fragment>\n"
              << "-insert_min <smallest outer distance of a concordant pair, default=0>\n-insert_max <largest, default=1000>\n"
              << "   (with -p2: needs -u 1 and -gpus 1; a genome file must fit one index block)\n"
              << "-mate_search <0|1: with -p2, search the window every hit of one mate allows for a placement of the other mate that\n"
              << "   the seeds missed (more than -s mismatches in its first -l bases, at most -e in the whole read), default=0>\n"
              << "-mate_search_anchors <a mate with more hits than this in a genome file starts no search, 0=no limit, default=0>\n"
              << "-pairs_all <0|1: with -p2, print EVERY concordant pair of a fragment (two lines each, per genome file, in the order of\n"
              << "   the two mates' hit lists) instead of the unique one; pairs of two seed hits: not with -mate_search 1, default=0>\n"
              << "-unpaired <file: with -p2, receives the mates of the fragments WITHOUT a concordant pair (after the last genome file, and\n"
              << "   after the search with -mate_search 1) that are placed uniquely on their own: mate 1's line, then mate 2's, as the\n"
              << "   single-end mode prints that hit; -o is unchanged; not with -pairs_all 1>\n"
              << "-gapped <file: with -p2, after the last genome file one more pass over the genome files (the text alone, one fresh context on\n"
              << "   -device) places the mate of a fragment WITHOUT a concordant pair whose other mate is placed uniquely on its own and which\n"
              << "   is itself placed nowhere, with at most ONE insertion or deletion, inside the window -insert_min .. -insert_max allows;\n"
              << "   <file> gets one line per mate placed uniquely that way, in read order: read id, mate (1|2), strand, fragment name,\n"
              << "   1-based position, CIGAR, NM, mismatches, cost, second best cost (* = none), 1-based position of the placed mate; a\n"
              << "   summary line goes to standard error; -o, -unpaired and -sam are unchanged; -insert_max of at most "
              << REAL_HIP_MATE_SEARCH_MAX_INSERT << "; not with -pairs_all 1>\n"
              << "-gapped_single <file: WITHOUT -p2, behind the other passes one more pass over every genome file and every index block of\n"
              << "   it places each read that is placed nowhere with at most ONE insertion or deletion, around the ungapped hits of its\n"
              << "   first and of its last -gap_anchor bases (-gap_max, -gap_flank, -gap_maxcost and -gap_margin apply); <file> gets one\n"
              << "   line per read placed uniquely that way, in read order: read id, strand, fragment name, 1-based position, CIGAR, NM,\n"
              << "   mismatches, cost, second best cost (* = none); a summary line goes to standard error; -o and every other output are\n"
              << "   unchanged; with -p2: -gapped>\n"
              << "-gap_anchor <bases of the two sub-reads that anchor a read, 1.." << REAL_HIP_MAX_PATL << ", default=max(-l, 32)>\n"
              << "-gap_anchors <a read whose two sub-reads have more hits than this together is left alone, 1.." << REAL_HIP_GAP_ANCHORS_MAX << ", default=32>\n"
              << "-gap_max <longest insertion or deletion, 1.." << REAL_HIP_GAP_MAX << ", default=8>\n"
              << "-gap_flank <fewest aligned bases on either side of the gap, default=8>\n"
              << "-gap_maxcost <a placement costs 4 per mismatch and 6 + its length for the gap, and at most this, default=4 * (-e) + 6 + (-gap_max)>\n"
              << "-gap_margin <a placement is unique if no other locus of the window costs at most its cost + this, default=0>\n"
              << "-sam_gapped <0|1: with -sam, -gapped and -p2, a mate -gapped places uniquely is written to the -sam file as placed: FLAG,\n"
              << "   POS, the CIGAR with its insertion or deletion (40M2D60M), NM:i, MD:Z (40^AC60) and ZC:i:<cost>, MAPQ 255; its mate's line\n"
              << "   names it (RNEXT, PNEXT, TLEN over the span on the text, FLAG 32), and both carry FLAG 2 if the outer distance lies in\n"
              << "   -insert_min .. -insert_max; the rescue then runs with the -sam pass, once; the -gapped file is unchanged; a summary line\n"
              << "   goes to standard error; default=0: the -sam file is what it is without -gapped.  WITHOUT -p2 (it then needs -sam and\n"
              << "   -gapped_single): a read -gapped_single places uniquely is written as placed, in the pass of its genome file: FLAG 0 / 16\n"
              << "   (+ 1024 with -dedup 1 if marked), POS, CIGAR, MAPQ 255, NM:i, MD:Z, ZC:i:<cost>; every other line and the -gapped_single\n"
              << "   file are unchanged; the gapped pass then runs before the -sam pass>\n"
              << "-insert_hist <file: with -p2, receives the histogram of the outer distances of the Unique fragments (after the last\n"
              << "   genome file) as lines outer<TAB>count, the last bin (-insert_max + 1) holding what lies beyond; the quartiles go to\n"
              << "   standard error; -o is unchanged; not with -pairs_all 1>\n"
              << "-insert_auto <N: with -p2, estimate the insert bounds from the first N fragments before the run: the quartiles q1, q3 of\n"
              << "   their Unique outer distances give [q1 - 3 (q3 - q1), q3 + 3 (q3 - q1)], cut to -insert_min .. -insert_max; the estimate\n"
              << "   judges uniqueness in the FIRST genome file only and under the window -insert_min .. -insert_max; not with\n"
              << "   -pairs_all 1, default=0 (off)>\n"
              << "   (-insert_hist and -insert_auto take an -insert_max of at most " << (REAL_HIP_INSERT_HIST_MAX_BINS - 2) << ")\n"
              << "-pileup <file: after the output pass, pile the FINAL unique placements (single-end: the printed lines; with -p2: both\n"
              << "   mates of the Unique fragments) up over every genome file on one fresh context on -device, and write one line per\n"
              << "   position where a placed read shows another base than the genome: fragment name, 1-based position in the fragment,\n"
              << "   reference base, depth, and how often A, C, G, T were seen there as a mismatch (the reference base's column is 0);\n"
              << "   a summary line per genome file goes to standard error; -o is unchanged; needs -u 1, not with -pairs_all 1;\n"
              << "   the placements of -unpaired are NOT part of the pileup; 20 bytes of device memory per genome base>\n"
              << "-pileup_depth <file: the depth as runs: fragment name, 0-based start, end, depth, for the maximal runs of equal\n"
              << "   non-zero depth inside a fragment; same conditions as -pileup>\n"
              << "-pileup_minq <Q: with -pileup, a mismatch of quality below Q is not counted, 0..63, default=0>\n"
              << "-pileup_gapped <0|1: with -p2 and one of -pileup / -pileup_depth / -vcf, the mates the gap rescue places with one insertion or\n"
              << "   deletion are piled up too: in the pileup pass of a genome file, behind the ungapped placements, the reads once more through\n"
              << "   the gap rescue (-gap_* apply; it runs once per run, -vcf_indels 1, -gapped and -sam_gapped 1 find its records); depth and\n"
              << "   mismatch counts on the aligned positions, none on the deleted ones; with -vcf the same mates count as evidence at the\n"
              << "   sites; the indel lines of -vcf_indels 1 do not change; with -p2, -dedup and -pileup_minmapq do NOT apply to gapped placements\n"
              << "   (they carry no duplicate mark and their MAPQ is 255); a summary line per genome file goes to standard error, default=0.\n"
              << "   WITHOUT -p2 (it then needs -gapped_single): the single reads -gapped_single places uniquely are piled up and counted as\n"
              << "   evidence the same way, from the records of the gapped pass, which then runs before the pileup; -dedup 1 DOES apply (gapped\n"
              << "   and ungapped reads of one 5' end are marked together), -pileup_minmapq does not (their MAPQ is 255)>\n"
              << "-vcf <file: after the pileup of a genome file (it runs also without -pileup; -pileup_minq then applies to it), call SNPs at\n"
              << "   its sites: the reads once more, bases of quality >= -pileup_minq counted per site, ten genotype likelihoods in integers,\n"
              << "   VCF 4.2 with GT:GQ:DP:AD; same conditions as -pileup; -dedup 1 leaves the duplicates out; indels only with -vcf_indels 1, one sample>\n"
              << "-vcf_minqual <Q: with -vcf, a call needs QUAL >= Q, default=20>\n"
              << "-vcf_mindepth <D: with -vcf, a call needs D bases of sufficient quality, default=4>\n"
              << "-vcf_indels <0|1: with -vcf and -p2, behind the SNP calls of a genome file the reads once more: the gap rescue (-gap_* apply; it\n"
              << "   runs once per run, -gapped and -sam_gapped 1 find its records), and the insertions and deletions the rescued mates show,\n"
              << "   left-aligned, added up and genotyped on the device; their lines (INFO DP;INDEL;SF;SR) are merged into the -vcf file by\n"
              << "   position; -vcf_minqual and -vcf_mindepth apply; -dedup and -pileup_minmapq do NOT reach the rescued mates; a summary line\n"
              << "   per genome file goes to standard error, default=0.  WITHOUT -p2 (it then needs -gapped_single): the insertions and\n"
              << "   deletions of the single reads -gapped_single places uniquely are called the same way; -dedup 1 leaves the marked ones out>\n"
              << "-vcf_minalt <N: with -vcf_indels 1, an indel call needs N rescued mates that show it, default=2>\n"
              << "-sam <file: after the output pass, write EVERY read as a SAM line (header: one @SQ per fragment of every genome file): a\n"
              << "   finally placed read with FLAG, RNAME, 1-based POS, MAPQ 255 (-mapq 1: 0..60), CIGAR <length>M, the sequence as placed, and NM:i / MD:Z from\n"
              << "   its mismatch list, computed on one fresh context on -device (ZS:f: the score, with -q 1); an unplaced read with FLAG 4.\n"
              << "   With -p2 the final placement of a mate is its Unique pair's, else -- for a fragment without any concordant pair -- its\n"
              << "   own unique one (the rule of -unpaired), and the lines carry the pair flags, RNEXT / PNEXT and TLEN (the outer distance,\n"
              << "   Unique pairs only).  Order: per genome file the reads placed in it, in read order, an unplaced mate beside its placed\n"
              << "   mate; reads and fragments with nothing placed in the pass of the last file; two mates placed in different files\n"
              << "   appear each in its own file's pass (@HD SO:unknown).  -o is unchanged; needs -u 1, not with -pairs_all 1>\n"
              << "-dedup <0|1: mark duplicates: the placed reads with one 5' end (file, strand, position of the first sequenced base), with\n"
              << "   -p2 the Unique fragments with one pair of 5' ends, are copies of one another; the copy with the largest sum of base\n"
              << "   qualities stays (ties: the first in the read file), the others are marked on the first device after the matching: their\n"
              << "   -sam lines carry FLAG 1024 (both mates of a fragment), -pileup / -pileup_depth leave them out; -o and -unpaired are\n"
              << "   unchanged; a summary line goes to standard error; needs -u 1, not with -pairs_all 1, default=0>\n"
              << "-dedup_minq <n: with -dedup 1, a base quality below n does not count in the sum, 0..63, default=15>\n"
              << "-mapq <0|1: mapping qualities: every candidate location of a read (with -p2: every concordant pair of a fragment, and every\n"
              << "   hit of a mate) is counted by its score on the device, over all index blocks and genome files; after the matching a\n"
              << "   finally placed read gets MAPQ 0..60 from the share of the other candidates (60: none): -sam writes it in the MAPQ\n"
              << "   column instead of 255, and a summary line goes to standard error; -o is unchanged; the single-end matcher runs twice;\n"
              << "   needs -u 1, not with -pairs_all 1, default=0>\n"
              << "-pileup_minmapq <Q: with -mapq 1 and -pileup / -pileup_depth / -vcf, placements of a mapping quality below Q are left out of\n"
              << "   them (-o and -sam are unchanged), 0..60, default=0>\n"
              << "-device <first HIP device, default=0>\n-gpus <number of devices, default=1>\n"
              << "-index <device|host, where the signature lists are sorted, default=device>\n"
              << "-block <positions per index block, default=as many as fit>\n-batch <reads per device batch>\n"
              << "-gpuparse <parse the read file on the device, default=1>\n-chunk <bytes of read-file text per device call, default=268435456>\n"
              << "Reads longer than 16384 bases are refused (the reference has no such limit); reads longer than 320 bases are slow.\n";
}

// The hand-rolled argv loop of RealOptions.cpp:140-396: "-x value" pairs, unknown arguments are
// reported and skipped, a missing value is an error.
RealOptions::RealOptions(int argc, char *argv[])
{
    std::vector<std::string> o;
    for (int i = 1; i < argc; ++i) o.push_back(argv[i]);
    size_t i = 0;
    auto need = [&](const char *flag) -> const std::string & {
        if (i + 1 >= o.size()) throw std::runtime_error(std::string("Parameter for argument ") + flag + " is missing.");
        return o[i + 1];
    };
    while (i < o.size()) {
        const std::string &a = o[i];
        if (a == "-t") { textfilename = need("-t"); i += 2; }
        else if (a == "-p") { patternfilename = need("-p"); i += 2; }
        else if (a == "-o") { outputfilename = need("-o"); i += 2; }
        else if (a == "-s") { seedkmax = atoi(need("-s").c_str()); i += 2; }
        else if (a == "-e") {
            totalkmax = atoi(need("-e").c_str());
            if (totalkmax > 15) { // UniqueMatchInfoBase::getMaxErrors(), RealOptions.cpp:176-180
                totalkmax = 15;
                std::cerr << "Warning: reducing maximum amount of errors to " << totalkmax << std::endl;
            }
            i += 2;
        }
        else if (a == "-l") { seedl = atoi(need("-l").c_str()); i += 2; }
        else if (a == "-u") { match_unique = atoi(need("-u").c_str()); i += 2; }
        else if (a == "-g") { gaps = atoi(need("-g").c_str()); i += 2; }
        else if (a == "-f" || a == "-m") { fracmem = atof(need("-f").c_str()); i += 2; }
        else if (a == "-q") { scores = atoi(need("-q").c_str()); i += 2; }
        else if (a == "-Q") { qualityOffset = atoi(need("-Q").c_str()); i += 2; }
        else if (a == "-R") { rewritepatterns = atoi(need("-R").c_str()); i += 2; }
        else if (a == "-T") { sort_threads = atoi(need("-T").c_str()); i += 2; }
        else if (a == "-similarity") { similarity = atof(need("-similarity").c_str()); i += 2; }
        else if (a == "-err") { err = atof(need("-err").c_str()); i += 2; }
        else if (a == "-trans") { trans = atof(need("-trans").c_str()); i += 2; }
        else if (a == "-gc") { gc = atof(need("-gc").c_str()); i += 2; }
        else if (a == "-gcmut_bias") { gcmut_bias = atof(need("-gcmut_bias").c_str()); i += 2; }
        else if (a == "-filter_level") { filter_level = atoi(need("-filter_level").c_str()); i += 2; }
        else if (a == "-device") { device = atoi(need("-device").c_str()); i += 2; }
        else if (a == "-gpus") { gpus = atoi(need("-gpus").c_str()); i += 2; }
        else if (a == "-gpus_share_device") { gpus_share_device = atoi(need("-gpus_share_device").c_str()) != 0; i += 2; }
        else if (a == "-index") { host_index = (need("-index") == "host"); i += 2; }
        else if (a == "-block") { block_entries = strtoull(need("-block").c_str(), 0, 10); i += 2; }
        else if (a == "-batch") { batch_reads = strtoull(need("-batch").c_str(), 0, 10); i += 2; }
        else if (a == "-prefix_bits") { prefix_bits = atoi(need("-prefix_bits").c_str()); i += 2; }
        else if (a == "-gpuparse") { gpuparse = atoi(need("-gpuparse").c_str()); i += 2; }
        else if (a == "-chunk") { chunk_bytes = strtoull(need("-chunk").c_str(), 0, 10); i += 2; }
        else if (a == "-p2") { pattern2filename = need("-p2"); i += 2; }
        else if (a == "-insert_min") { insert_min = (uint32_t)strtoul(need("-insert_min").c_str(), 0, 10); i += 2; }
        else if (a == "-insert_max") { insert_max = (uint32_t)strtoul(need("-insert_max").c_str(), 0, 10); i += 2; }
        else if (a == "-mate_search") { mate_search = atoi(need("-mate_search").c_str()) != 0; mate_search_given = true; i += 2; }
        else if (a == "-pairs_all") { pairs_all = atoi(need("-pairs_all").c_str()) != 0; pairs_all_given = true; i += 2; }
        else if (a == "-mate_search_anchors") { mate_search_anchors = (uint32_t)strtoul(need("-mate_search_anchors").c_str(), 0, 10); mate_search_given = true; i += 2; }
        else if (a == "-unpaired") { unpairedfilename = need("-unpaired"); unpaired_given = true; i += 2; }
        else if (a == "-gapped") { gappedfilename = need("-gapped"); gapped_given = true; i += 2; }
        else if (a == "-gapped_single") { gappedsinglefilename = need("-gapped_single"); gapped_single_given = true; i += 2; }
        else if (a == "-gap_anchor") { gap_anchor = strtol(need("-gap_anchor").c_str(), 0, 10); gap_anchor_flags_given = true; i += 2; }
        else if (a == "-gap_anchors") { gap_anchors = strtoul(need("-gap_anchors").c_str(), 0, 10); gap_anchor_flags_given = true; i += 2; }
        else if (a == "-gap_max") { gap_max = strtoul(need("-gap_max").c_str(), 0, 10); gap_flags_given = true; i += 2; }
        else if (a == "-gap_flank") { gap_flank = strtoul(need("-gap_flank").c_str(), 0, 10); gap_flags_given = true; i += 2; }
        else if (a == "-gap_maxcost") { gap_maxcost = strtol(need("-gap_maxcost").c_str(), 0, 10); gap_flags_given = true; i += 2; }
        else if (a == "-sam_gapped") { sam_gapped = atoi(need("-sam_gapped").c_str()) != 0; sam_gapped_given = true; i += 2; }
        else if (a == "-gap_margin") { gap_margin = strtoul(need("-gap_margin").c_str(), 0, 10); gap_flags_given = true; i += 2; }
        else if (a == "-insert_hist") { inserthistfilename = need("-insert_hist"); insert_flags_given = true; i += 2; }
        else if (a == "-insert_auto") { insert_auto = strtoull(need("-insert_auto").c_str(), 0, 10); insert_flags_given = true; i += 2; }
        else if (a == "-pileup") { pileupfilename = need("-pileup"); pileup_given = true; i += 2; }
        else if (a == "-pileup_depth") { pileupdepthfilename = need("-pileup_depth"); pileup_depth_given = true; i += 2; }
        else if (a == "-pileup_minq") { pileup_minq = strtoul(need("-pileup_minq").c_str(), 0, 10); pileup_minq_given = true; i += 2; }
        else if (a == "-vcf") { vcffilename = need("-vcf"); vcf_given = true; i += 2; }
        else if (a == "-vcf_minqual") { vcf_minqual = strtoul(need("-vcf_minqual").c_str(), 0, 10); vcf_minqual_given = true; i += 2; }
        else if (a == "-pileup_gapped") { pileup_gapped = atoi(need("-pileup_gapped").c_str()) != 0; pileup_gapped_given = true; i += 2; }
        else if (a == "-vcf_indels") { vcf_indels = atoi(need("-vcf_indels").c_str()) != 0; vcf_indels_given = true; i += 2; }
        else if (a == "-vcf_minalt") { vcf_minalt = strtoul(need("-vcf_minalt").c_str(), 0, 10); vcf_minalt_given = true; i += 2; }
        else if (a == "-vcf_mindepth") { vcf_mindepth = strtoul(need("-vcf_mindepth").c_str(), 0, 10); vcf_mindepth_given = true; i += 2; }
        else if (a == "-sam") { samfilename = need("-sam"); sam_given = true; i += 2; }
        else if (a == "-dedup") { dedup = atoi(need("-dedup").c_str()) != 0; dedup_given = true; i += 2; }
        else if (a == "-dedup_minq") { dedup_minq = strtol(need("-dedup_minq").c_str(), 0, 10); dedup_minq_given = true; i += 2; }
        else if (a == "-mapq") { mapq = atoi(need("-mapq").c_str()) != 0; i += 2; }
        else if (a == "-pileup_minmapq") { pileup_minmapq = strtol(need("-pileup_minmapq").c_str(), 0, 10); pileup_minmapq_given = true; i += 2; }
        else if (a == "-table_kind") { table_kind = atoi(need("-table_kind").c_str()); i += 2; }
        else if (a == "-h") { printHelp(); i += 1; }
        else { std::cerr << "Ignoring unknown argument " << a << std::endl; i += 1; }
    }
    if (!(textfilename.size() && patternfilename.size() && outputfilename.size())) printHelp();
    if (!textfilename.size()) throw std::runtime_error("Mandatory argument -t (text file name) is not given.");
    if (!patternfilename.size()) throw std::runtime_error("Mandatory argument -p (pattern file name) is not given.");
    if (!outputfilename.size()) throw std::runtime_error("Mandatory argument -o (output file name) is not given.");
    if (fracmem > 1.0) fracmem = 1.0;
    if (patternfilename == "-") {
        // Reads from standard input (RealOptions.cpp:418-426, real.cpp:240-257).  The reference rewrites them into its
        // temporary pattern file because it reads the patterns once per genome block and once more for the output; so does
        // this driver, through a spool file of the text as it came (the rewritten binary format is out of scope).
        const char *tmp = getenv("TMPDIR");
        std::string name = std::string(tmp && *tmp ? tmp : "/tmp") + "/real_stdin_XXXXXX";
        std::vector<char> path(name.begin(), name.end());
        path.push_back(0);
        const int fd = mkstemp(path.data());
        if (fd < 0) throw std::runtime_error("Unable to create a temporary file for the patterns from standard input.");
        stdin_spool.path = path.data();
        std::cerr << "Reading patterns from stdin, writing them to temporary file " << stdin_spool.path << std::endl;
        std::vector<char> buf((size_t)8 << 20);
        size_t got;
        bool ok = true;
        while (ok && (got = fread(buf.data(), 1, buf.size(), stdin)) > 0)
            for (size_t off = 0; ok && off < got;) {
                const ssize_t w = write(fd, buf.data() + off, got - off);
                if (w <= 0) ok = false; else off += (size_t)w;
            }
        close(fd);
        if (!ok) throw std::runtime_error("Failed to write the patterns from standard input to the temporary file.");
        patternfilename = stdin_spool.path;
        rewritepatterns = true;
    }
    fastq = isFastQ(patternfilename);
    if (fastq && !qualityOffset && !stdin_spool.empty()) {
        // real.cpp:248-257: no detection on standard input, Illumina GA assumed
        std::cerr << "WARNING: automatic quality offset detection not supported when" << std::endl;
        std::cerr << "         reading patterns from standard input. Assuming input" << std::endl;
        std::cerr << "         was produced by an Illumina  GA (i.e. -Q 64)" << std::endl;
        qualityOffset = 64;
    }
    std::cerr << "pattern file is " << (fastq ? "FASTQ" : "FASTA") << std::endl;
    // clamps of RealOptions.cpp:434-453
    if (seedl > 64) { seedl = 64; std::cerr << "reduced seed size to " << seedl << " to not exceed 64." << std::endl; }
    if (seedl % 4) { seedl -= (seedl % 4); std::cerr << "reduced seed size to " << seedl << " to have a multiple of 4." << std::endl; }
    if (seedl < 4) throw std::runtime_error("cannot handle seed length < 4");
    if (seedkmax > 2) { seedkmax = 2; std::cerr << "reduced number of mismatches in seed to " << seedkmax << " as we cannot handle more." << std::endl; }
    if (gaps) std::cerr << "gapped matching is not implemented (nor completed in the reference); ignoring -g" << std::endl;
    // RealOptions.cpp:455-463
    switch (filter_level) {
    case 1: filter_mult = 0.5 * totalkmax; break;
    case 2: filter_mult = 1 * totalkmax; break;
    case 3: filter_mult = 2 * totalkmax; break;
    case 4: filter_mult = 3 * totalkmax; break;
    case 0: default: filter_mult = 0 * totalkmax; break;
    }
    filter_mult /= 70.0;
    std::cerr << "filter_mult=" << filter_mult << std::endl;
    if (gpus < 1) gpus = 1;
    if (pileup_given || pileup_depth_given) { // the pileup: loud errors before anything runs
        const char *flag = pileup_given ? "-pileup" : "-pileup_depth";
        if (!match_unique) throw std::runtime_error(std::string(flag) + " piles up the unique placements: it cannot be combined with -u 0.");
        if (pairs_all) throw std::runtime_error(std::string(flag) + " piles up the unique placement of a fragment: it cannot be combined with -pairs_all 1.");
        for (const std::string *f : {&pileupfilename, &pileupdepthfilename}) {
            const bool given = f == &pileupfilename ? pileup_given : pileup_depth_given;
            if (!given) continue;
            if (f->empty()) throw std::runtime_error("-pileup / -pileup_depth need a file name: an empty one was given.");
            if (*f == "-") throw std::runtime_error("-pileup / -pileup_depth write to a file: standard output (-) cannot be it.");
            if (*f == outputfilename) throw std::runtime_error("-pileup / -pileup_depth must name a file of its own: it names the same file as -o.");
            if (unpaired_given && *f == unpairedfilename) throw std::runtime_error("-pileup / -pileup_depth must name a file of its own: it names the same file as -unpaired.");
            if (!inserthistfilename.empty() && *f == inserthistfilename) throw std::runtime_error("-pileup / -pileup_depth must name a file of its own: it names the same file as -insert_hist.");
        }
        if (pileup_given && pileup_depth_given && pileupfilename == pileupdepthfilename)
            throw std::runtime_error("-pileup and -pileup_depth must name two files.");
    }
    if (sam_given) { // SAM output: loud errors before anything runs
        if (!match_unique) throw std::runtime_error("-sam writes the unique placement of a read: it cannot be combined with -u 0.");
        if (pairs_all) throw std::runtime_error("-sam writes the unique placement of a fragment: it cannot be combined with -pairs_all 1.");
        if (samfilename.empty()) throw std::runtime_error("-sam needs a file name: an empty one was given.");
        if (samfilename == "-") throw std::runtime_error("-sam writes to a file: standard output (-) cannot be it.");
        if (samfilename == outputfilename) throw std::runtime_error("-sam must name a file of its own: it names the same file as -o.");
        if (unpaired_given && samfilename == unpairedfilename) throw std::runtime_error("-sam must name a file of its own: it names the same file as -unpaired.");
        if (!inserthistfilename.empty() && samfilename == inserthistfilename) throw std::runtime_error("-sam must name a file of its own: it names the same file as -insert_hist.");
        if ((pileup_given && samfilename == pileupfilename) || (pileup_depth_given && samfilename == pileupdepthfilename))
            throw std::runtime_error("-sam must name a file of its own: it names the same file as -pileup / -pileup_depth.");
    }
    if (vcf_given) { // SNP calls: loud errors before anything runs
        if (!match_unique) throw std::runtime_error("-vcf calls variants from the unique placements: it cannot be combined with -u 0.");
        if (pairs_all) throw std::runtime_error("-vcf calls variants from the unique placement of a fragment: it cannot be combined with -pairs_all 1.");
        if (vcffilename.empty()) throw std::runtime_error("-vcf needs a file name: an empty one was given.");
        if (vcffilename == "-") throw std::runtime_error("-vcf writes to a file: standard output (-) cannot be it.");
        if (vcffilename == outputfilename) throw std::runtime_error("-vcf must name a file of its own: it names the same file as -o.");
        if (unpaired_given && vcffilename == unpairedfilename) throw std::runtime_error("-vcf must name a file of its own: it names the same file as -unpaired.");
        if (!inserthistfilename.empty() && vcffilename == inserthistfilename) throw std::runtime_error("-vcf must name a file of its own: it names the same file as -insert_hist.");
        if ((pileup_given && vcffilename == pileupfilename) || (pileup_depth_given && vcffilename == pileupdepthfilename))
            throw std::runtime_error("-vcf must name a file of its own: it names the same file as -pileup / -pileup_depth.");
        if (sam_given && vcffilename == samfilename) throw std::runtime_error("-vcf must name a file of its own: it names the same file as -sam.");
        if (vcf_minqual > 0xfffffffful || vcf_mindepth > 0xfffffffful) throw std::runtime_error("-vcf_minqual / -vcf_mindepth take a number below 2^32.");
    }
    if (vcf_indels) { // indel calls: loud errors before anything runs
        if (!vcf_given) throw std::runtime_error("-vcf_indels 1 writes its calls into the -vcf file: it needs -vcf.");
        if (pattern2filename.empty() && !gapped_single_given)
            throw std::runtime_error("-vcf_indels 1 calls the indels of gap-rescued mates with -p2 (paired-end reads); without -p2 it calls those of the single reads -gapped_single places: it needs -gapped_single.");
        if (vcf_minalt > 0xfffffffful) throw std::runtime_error("-vcf_minalt takes a number below 2^32.");
    }
    if (pileup_gapped) { // gapped placements in the pileup: loud errors before anything runs
        if (pattern2filename.empty() && !gapped_single_given)
            throw std::runtime_error("-pileup_gapped 1 piles up the mates the gap rescue places with -p2 (paired-end reads); without -p2 it needs -gapped_single: without it the single-end drivers are not there yet, nothing places a single read with a gap.");
        if (!pileup_given && !pileup_depth_given && !vcf_given) throw std::runtime_error("-pileup_gapped 1 needs one of -pileup / -pileup_depth / -vcf.");
        if (pairs_all) throw std::runtime_error("-pileup_gapped 1 cannot be combined with -pairs_all 1.");
    }
    if (vcf_minalt_given && !vcf_indels) throw std::runtime_error("-vcf_minalt is only meaningful with -vcf_indels 1.");
    if (vcf_minqual_given && !vcf_given) throw std::runtime_error("-vcf_minqual is only meaningful with -vcf.");
    if (vcf_mindepth_given && !vcf_given) throw std::runtime_error("-vcf_mindepth is only meaningful with -vcf.");
    if (dedup) { // duplicate marking: loud errors before anything runs
        if (!match_unique) throw std::runtime_error("-dedup marks copies of the unique placement of a read: it cannot be combined with -u 0.");
        if (pairs_all) throw std::runtime_error("-dedup marks copies of the unique placement of a fragment: it cannot be combined with -pairs_all 1.");
    }
    if (dedup_minq_given && !dedup) throw std::runtime_error("-dedup_minq needs -dedup 1.");
    if (dedup_minq < 0 || dedup_minq > 63) throw std::runtime_error("-dedup_minq must be in 0..63.");
    if (pileup_minq_given && !pileup_given && !vcf_given) throw std::runtime_error("-pileup_minq is only meaningful with -pileup.");
    if (pileup_minq > 63) throw std::runtime_error("-pileup_minq takes a quality of at most 63.");
    if (mapq) { // mapping quality: loud errors before anything runs
        if (!match_unique) throw std::runtime_error("-mapq 1 rates the unique placement of a read: it cannot be combined with -u 0.");
        if (pairs_all) throw std::runtime_error("-mapq 1 rates the unique placement of a fragment: it cannot be combined with -pairs_all 1.");
    }
    if (pileup_minmapq_given) {
        if (!mapq) throw std::runtime_error("-pileup_minmapq needs -mapq 1.");
        if (!pileup_given && !pileup_depth_given && !vcf_given) throw std::runtime_error("-pileup_minmapq is only meaningful with -pileup / -vcf.");
        if (pileup_minmapq < 0 || pileup_minmapq > (long)REAL_HIP_MAPQ_MAX) throw std::runtime_error("-pileup_minmapq must be in 0..60.");
    }
    if (sam_gapped) { // the rescued mates in the -sam file: loud errors before anything runs
        if (pattern2filename.empty() && !gapped_single_given)
            throw std::runtime_error("-sam_gapped 1 writes the mates the gap rescue places with -p2 (paired-end reads); without -p2 it writes the single reads -gapped_single places: it needs -gapped_single.");
        if (!sam_given) throw std::runtime_error("-sam_gapped 1 writes the rescued mates into the -sam file: it needs -sam.");
        if (!pattern2filename.empty() && !gapped_given) throw std::runtime_error("-sam_gapped 1 writes the mates the gap rescue places: it needs -gapped.");
        if (pairs_all) throw std::runtime_error("-sam_gapped 1 cannot be combined with -pairs_all 1.");
    }
    if (gapped_given) { // gap rescue: loud errors before anything runs
        if (pattern2filename.empty()) throw std::runtime_error("-gapped is only meaningful with -p2 (paired-end reads).");
        if (pairs_all) throw std::runtime_error("-gapped places the mate of a fragment without a pair: it cannot be combined with -pairs_all 1.");
        if (gappedfilename.empty()) throw std::runtime_error("-gapped needs a file name: an empty one was given.");
        if (gappedfilename == "-") throw std::runtime_error("-gapped writes to a file: standard output (-) cannot be it.");
        if (gappedfilename == outputfilename) throw std::runtime_error("-gapped must name a file of its own: it names the same file as -o.");
        if ((unpaired_given && gappedfilename == unpairedfilename) || (sam_given && gappedfilename == samfilename) ||
            (!inserthistfilename.empty() && gappedfilename == inserthistfilename) || (pileup_given && gappedfilename == pileupfilename) ||
            (pileup_depth_given && gappedfilename == pileupdepthfilename) || (vcf_given && gappedfilename == vcffilename))
            throw std::runtime_error("-gapped must name a file of its own: it names the same file as another output.");
    }
    if (gapped_single_given) { // anchored gap placement of single reads: loud errors before anything runs
        const std::string &f = gappedsinglefilename;
        if (!pattern2filename.empty()) throw std::runtime_error("-gapped_single places single reads: with -p2 (paired-end reads) the flag is -gapped.");
        if (!match_unique) throw std::runtime_error("-gapped_single places the reads the unique matcher places nowhere: it cannot be combined with -u 0.");
        if (f.empty()) throw std::runtime_error("-gapped_single needs a file name: an empty one was given.");
        if (f == "-") throw std::runtime_error("-gapped_single writes to a file: standard output (-) cannot be it.");
        if (f == outputfilename) throw std::runtime_error("-gapped_single must name a file of its own: it names the same file as -o.");
        if ((sam_given && f == samfilename) || (pileup_given && f == pileupfilename) || (pileup_depth_given && f == pileupdepthfilename) ||
            (vcf_given && f == vcffilename))
            throw std::runtime_error("-gapped_single must name a file of its own: it names the same file as another output.");
        if (gap_anchor < 0) gap_anchor = std::max<long>((long)seedl, 32);
        if (gap_anchor < 1 || gap_anchor > (long)REAL_HIP_MAX_PATL) throw std::runtime_error("-gap_anchor must be in 1.." + std::to_string(REAL_HIP_MAX_PATL) + ".");
        if (gap_anchors < 1 || gap_anchors > REAL_HIP_GAP_ANCHORS_MAX) throw std::runtime_error("-gap_anchors must be in 1.." + std::to_string(REAL_HIP_GAP_ANCHORS_MAX) + ".");
    } else if (gap_anchor_flags_given) {
        throw std::runtime_error("-gap_anchor / -gap_anchors need -gapped_single.");
    }
    if (gapped_given || vcf_indels || pileup_gapped || gapped_single_given) { // the rescue's own parameters: -gapped, -vcf_indels 1, -pileup_gapped 1 and -gapped_single run it
        if (gap_max < 1 || gap_max > REAL_HIP_GAP_MAX) throw std::runtime_error("-gap_max must be in 1.." + std::to_string(REAL_HIP_GAP_MAX) + ".");
        if (gap_flank < 1) throw std::runtime_error("-gap_flank must be at least 1.");
        if (gap_maxcost < 0) gap_maxcost = 4 * (long)totalkmax + 6 + (long)gap_max;
        if (gap_maxcost > 65534 || gap_margin > 65535) throw std::runtime_error("-gap_maxcost takes at most 65534, -gap_margin at most 65535.");
        if (!pattern2filename.empty() && (gapped_given || vcf_indels || pileup_gapped) && insert_max > REAL_HIP_MATE_SEARCH_MAX_INSERT)
            throw std::runtime_error(std::string(gapped_given ? "-gapped" : vcf_indels ? "-vcf_indels 1" : "-pileup_gapped 1") + " takes an -insert_max of at most " + std::to_string(REAL_HIP_MATE_SEARCH_MAX_INSERT) + ".");
    } else if (gap_flags_given) {
        throw std::runtime_error("-gap_max / -gap_flank / -gap_maxcost / -gap_margin need -gapped (with -p2) or -gapped_single.");
    }
    if (!pattern2filename.empty()) { // paired-end reads: loud errors, not silent differences
        if (!match_unique) throw std::runtime_error("-p2 (paired-end reads) reports one placement per fragment: it cannot be combined with -u 0 (every concordant pair: -pairs_all 1).");
        if (gpus > 1) throw std::runtime_error("-p2 (paired-end reads) runs on one device: it cannot be combined with -gpus > 1.");
        if (pattern2filename == "-" || !stdin_spool.empty()) throw std::runtime_error("-p2 (paired-end reads) needs two files: standard input cannot be one of them.");
        if (insert_min > insert_max) throw std::runtime_error("-insert_min is larger than -insert_max.");
        if (mate_search && insert_max > REAL_HIP_MATE_SEARCH_MAX_INSERT)
            throw std::runtime_error("-mate_search 1 takes an -insert_max of at most " + std::to_string(REAL_HIP_MATE_SEARCH_MAX_INSERT) + ".");
        if (pairs_all && mate_search)
            throw std::runtime_error("-pairs_all 1 lists the concordant pairs of two seed hits: it cannot be combined with -mate_search 1.");
        if (unpaired_given && pairs_all)
            throw std::runtime_error("-unpaired lists the mates of the fragments without a pair: it cannot be combined with -pairs_all 1.");
        if (unpaired_given && (unpairedfilename.empty() || unpairedfilename == outputfilename))
            throw std::runtime_error("-unpaired must name a file of its own: it names the same file as -o.");
        if (insert_flags_given) {
            const bool hist = !inserthistfilename.empty();
            if (pairs_all) throw std::runtime_error("-insert_hist / -insert_auto look at the unique placement of a fragment: they cannot be combined with -pairs_all 1.");
            if ((hist || insert_auto) && insert_max > REAL_HIP_INSERT_HIST_MAX_BINS - 2)
                throw std::runtime_error("-insert_hist / -insert_auto take an -insert_max of at most " + std::to_string(REAL_HIP_INSERT_HIST_MAX_BINS - 2) + ".");
            if (hist && inserthistfilename == outputfilename) throw std::runtime_error("-insert_hist must name a file of its own: it names the same file as -o.");
            if (hist && unpaired_given && inserthistfilename == unpairedfilename)
                throw std::runtime_error("-insert_hist must name a file of its own: it names the same file as -unpaired.");
        }
        fastq2 = isFastQ(pattern2filename);
    } else if (insert_flags_given) {
        throw std::runtime_error("-insert_hist / -insert_auto are only meaningful with -p2 (paired-end reads).");
    } else if (mate_search_given) {
        throw std::runtime_error("-mate_search / -mate_search_anchors are only meaningful with -p2 (paired-end reads).");
    } else if (unpaired_given) {
        throw std::runtime_error("-unpaired is only meaningful with -p2 (paired-end reads).");
    } else if (pairs_all_given) {
        throw std::runtime_error("-pairs_all is only meaningful with -p2 (paired-end reads).");
    }
    if (chunk_bytes < 4096) chunk_bytes = 4096;
    if (chunk_bytes > (4ull << 30) - (1ull << 20)) chunk_bytes = (4ull << 30) - (1ull << 20); // real_hip_parse_reads: n_bytes < 4 GiB
}
