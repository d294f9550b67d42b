// RealOptions -- the `real` command line of the reference (RealOptions.hpp:26-78, parser
// RealOptions.cpp:122-466), kept flag for flag, plus the device flags of this build.
#pragma once
#include <stdint.h>
#include <string>

// a file that is removed with its owner (also when the owner's constructor throws behind it)
struct SpoolFile {
    std::string path;
    SpoolFile() {}
    ~SpoolFile();
    SpoolFile(const SpoolFile &) = delete;
    SpoolFile &operator=(const SpoolFile &) = delete;
    bool empty() const { return path.empty(); }
};

struct RealOptions {
    // defaults: RealOptions.hpp:27-36
    std::string textfilename, patternfilename, outputfilename;
    unsigned seedkmax = 2;
    unsigned totalkmax = 5;
    int seedl = 32;
    bool match_unique = true;
    double fracmem = 0.75;   // -f / -m: here the fraction of *HBM* the index blocks may use
    bool scores = true;
    unsigned qualityOffset = 0;
    bool rewritepatterns = true; // -R: accepted and ignored (the binary temp format is out of scope)
    unsigned sort_threads = 2;   // -T: threads of the host index sort (only with -index host)
    int filter_level = 2;
    double filter_mult = 0;
    double similarity = 0.995, err = 0.0, trans = 0.71, gc = 0.41, gcmut_bias = 2.0; // Scoring.cpp:204-208
    bool gaps = false;
    bool fastq = false;
    SpoolFile stdin_spool;    // -p -: the file the reads from standard input were written to (removed when the options go)
    // this build
    int device = 0;           // -device: first HIP device
    int gpus = 1;             // -gpus: read batches are dealt round-robin to this many devices
    bool gpus_share_device = false; // -gpus_share_device 1: the contexts of -gpus N all sit on -device (rehearsal of the N-context paths on a one-GPU box)
    bool host_index = false;  // -index host|device: where the six lists are sorted
    uint64_t block_entries = 0; // -block: positions per index block (0 = as many as fit)
    uint64_t batch_reads = 4u << 20; // -batch: reads per device batch
    unsigned prefix_bits = 0;
    unsigned table_kind = 0;         // -table_kind: device bucket tables (real_hip.h), 0 = auto
    unsigned gpuparse = 1;           // -gpuparse: parse the read file on the device when it is in one-line-per-field form
    // paired-end reads (no counterpart in the reference): -p holds mate 1, -p2 mate 2 of every fragment, in the same order
    std::string pattern2filename;    // -p2
    bool fastq2 = false;             // format of the -p2 file
    uint32_t insert_min = 0;         // -insert_min / -insert_max: bounds of the outer distance of a concordant pair, inclusive
    uint32_t insert_max = 1000;
    bool mate_search = false;         // -mate_search: real_hip_match_pairs_search instead of real_hip_match_pairs
    uint32_t mate_search_anchors = 0; // -mate_search_anchors: real_hip_mate_search_params.max_anchors
    bool pairs_all = false;           // -pairs_all: every concordant pair of a fragment (real_hip_match_pairs_all) instead of the unique one
    bool pairs_all_given = false;     // (the flag was on the command line: an error without -p2)
    std::string unpairedfilename;     // -unpaired: the file that receives the Unique mates of the fragments without a pair (real_hip_match_pairs_singles)
    bool unpaired_given = false;      // (the flag was on the command line: an error without -p2)
    std::string gappedfilename;       // -gapped: the file that receives the mates placed with one insertion or deletion (real_hip_gap_rescue)
    bool gapped_given = false, gap_flags_given = false; // (-gapped / one of -gap_* was on the command line)
    unsigned long gap_max = 8, gap_flank = 8, gap_margin = 0; // -gap_max, -gap_flank, -gap_margin
    long gap_maxcost = -1;            // -gap_maxcost: -1 = 4 * (-e) + 6 + (-gap_max)
    std::string gappedsinglefilename; // -gapped_single: the file that receives the single reads placed with one insertion or deletion (real_hip_match_gapped)
    bool gapped_single_given = false, gap_anchor_flags_given = false; // (-gapped_single / one of -gap_anchor, -gap_anchors was on the command line)
    long gap_anchor = -1;             // -gap_anchor: bases of the two sub-reads that anchor a read, -1 = max(-l, 32)
    unsigned long gap_anchors = 32;   // -gap_anchors: a read whose sub-reads have more hits is left alone
    bool sam_gapped = false, sam_gapped_given = false; // -sam_gapped: with -sam and -gapped, the rescued mates' SAM lines carry their gapped placement (real_hip_mismatches_gapped)
    bool mate_search_given = false;   // (either flag was on the command line: an error without -p2)
    std::string inserthistfilename;   // -insert_hist: the file that receives the histogram of the Unique fragments' outer distances (real_hip_pair_insert_hist)
    std::string pileupfilename;       // -pileup: the file that receives the sites of the pileup of the final placements (real_hip_pileup_*)
    std::string pileupdepthfilename;  // -pileup_depth: the file that receives the depth as runs
    unsigned long pileup_minq = 0;    // -pileup_minq: a mismatch of lower quality is not counted
    bool pileup_given = false, pileup_depth_given = false, pileup_minq_given = false;
    std::string samfilename;          // -sam: the file that receives the final placements as SAM with NM / MD (real_hip_mismatches*)
    bool sam_given = false;
    std::string vcffilename;          // -vcf: the file that receives the SNP calls of the pileup's sites as VCF (real_hip_call_*)
    unsigned long vcf_minqual = 20;   // -vcf_minqual: a call needs QUAL of at least this
    unsigned long vcf_mindepth = 4;   // -vcf_mindepth: and this many bases of sufficient quality
    bool vcf_given = false, vcf_minqual_given = false, vcf_mindepth_given = false;
    bool pileup_gapped = false, pileup_gapped_given = false; // -pileup_gapped: with -p2 and -pileup / -pileup_depth / -vcf, the gap-rescued mates are piled up and counted as evidence too (real_hip_pileup_add_gapped, real_hip_call_add_gapped)
    bool vcf_indels = false, vcf_indels_given = false; // -vcf_indels: with -vcf and -p2, the indels the gap-rescued mates show are called too (real_hip_indel_*)
    unsigned long vcf_minalt = 2;     // -vcf_minalt: an indel call needs this many rescued mates
    bool vcf_minalt_given = false;
    bool dedup = false;               // -dedup: mark the copies of a placed read / fragment (real_hip_mark_duplicates*): FLAG 1024 in -sam, left out of -pileup
    long dedup_minq = 15;             // -dedup_minq: a base quality below it does not count in the sum that chooses the copy that stays
    bool dedup_given = false, dedup_minq_given = false;
    bool mapq = false;                // -mapq: mapping qualities from all candidates of a read / fragment (real_hip_match_mapq, real_hip_match_pairs_mapq, real_hip_mapq*): MAPQ in -sam
    long pileup_minmapq = 0;          // -pileup_minmapq: with -mapq 1, placements of a lower quality are left out of -pileup / -pileup_depth / -vcf
    bool pileup_minmapq_given = false;
    uint64_t insert_auto = 0;         // -insert_auto: fragments the insert bounds are estimated from before the run (real_hip_insert_bounds), 0 = off
    bool insert_flags_given = false;  // (either flag was on the command line: an error without -p2)
    uint64_t chunk_bytes = 256ull << 20; // -chunk: bytes of read-file text handed to a device at a time (< 4 GiB)

    RealOptions() {}
    RealOptions(int argc, char *argv[]); // throws std::runtime_error like the reference

    void printHelp() const;
    static bool isFastQ(const std::string &filename); // RealOptions.cpp:43-72
    double getFilterValue(unsigned patl) const { return filter_mult * patl; } // RealOptions.hpp:74-77
};
