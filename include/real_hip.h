/*
 * real_hip.h -- C ABI of the MI355X (gfx950) read-matching hot path of REAL.
 *
 * The reference (solonas13/REAL) has no plugin / FFI interface: the hot path
 * sits behind C++ template seams inside one binary.  This
 * header is the drop-in boundary a maintainer would bind instead of the
 * per-read loops
 *
 *     for z in block: UM.match(pattern, uniqueinfo[patid], fi, RWB, handled)
 *                                   matchUniqueImplementation.cpp:1268-1295
 *     for z in block: AM.match(pattern, fi, RWB, handled, localmatches);
 *                     unifyMatches(localmatches)
 *                                   matchAllImplementation.cpp:459-533
 *
 * Plain pointers and sizes only; no C++ / torch types; nothing throws across
 * the boundary: every entry point returns 0 or a negative real_hip_status.
 * Each entry point cites the reference interface it replaces.
 *
 * Threading: one submitting thread per ctx (calls on one ctx are not
 * re-entrant); distinct ctx (one per GPU) are independent.
 *
 * Streams: every ctx owns one non-blocking HIP stream and runs all its copies
 * and kernels there; it knows nothing about the caller's streams.  Device
 * memory handed to a call (on_device / text_on_device / sym_on_device inputs
 * and the in/out records of on_device = 1) must therefore be COMPLETE before
 * the call -- the producing stream synchronised, or an event of it waited for
 * with real_hip_wait_event() -- and must not be touched until the call (or,
 * for the _submit forms, the matching real_hip_wait) has returned.  Results
 * are complete when the synchronous entry points return.
 */
#ifndef REAL_HIP_H
#define REAL_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define REAL_HIP_ABI_VERSION 2

typedef struct real_hip_ctx real_hip_ctx;

typedef enum real_hip_status {
    REAL_HIP_OK            =  0,
    REAL_HIP_E_INVALID     = -1,  /* bad argument / struct_size                       */
    REAL_HIP_E_NOMEM       = -2,  /* host or device allocation failed (std::bad_alloc
                                     in the reference, matchUniqueImplementation.cpp:1215-1219) */
    REAL_HIP_E_DEVICE      = -3,  /* HIP runtime error (see real_hip_last_error)      */
    REAL_HIP_E_OVERFLOW    = -4,  /* output capacity too small; *n_out = needed size  */
    REAL_HIP_E_STATE       = -5,  /* text / index not set                             */
    REAL_HIP_E_UNSUPPORTED = -6   /* e.g. read longer than REAL_HIP_MAX_PATL_LONG     */
} real_hip_status;

#define REAL_HIP_MAX_PATL 320u        /* longest read the lane-per-read kernels hold in registers                */
#define REAL_HIP_MAX_PATL_LONG 16384u /* longest read at all: reads beyond REAL_HIP_MAX_PATL get a wave each and are
                                         read from LDS (slower, and only those reads); longer ones are refused with
                                         REAL_HIP_E_UNSUPPORTED -- the reference has no limit (RestMatch.hpp:34-37)  */

/* ---- parameters: what RealOptions (RealOptions.hpp:27-77) hands the matcher */
typedef struct real_hip_params {
    uint32_t struct_size;   /* = sizeof(real_hip_params)                              */
    uint32_t seedl;         /* -l : 4..64, multiple of 4 (RealOptions.cpp:434-447)    */
    uint32_t seedkmax;      /* -s : <= 2 (RealOptions.cpp:449-453)                    */
    uint32_t totalkmax;     /* -e : <= 15 (RealOptions.cpp:172-180)                   */
    uint32_t scores;        /* -q : 0/1                                               */
    uint32_t prefix_bits;   /* device bucket-table width; 0 = auto from index size.
                               (The reference's 22-bit getSampleBits() table is a
                               host-layout detail; results do not depend on it.)      */
    int32_t  device;        /* HIP device ordinal                                     */
    uint32_t table_kind;    /* device bucket tables: 0 = auto from index size and device memory, 1 = bucket starts only,
                               2 = directory entries (group sizes + partner digests for seedl <= 32,
                               key fingerprints for wider signatures), 3 = bucket rows (one 128-byte
                               row per bucket holds directory and entries, lookups by groups of eight
                               lanes); a request: a geometry that cannot hold it gets another layout
                               (real_hip_index_table_kind reports the one built); a host-layout detail like
                               prefix_bits, results do not depend on it                   */
    double   filter_mult;   /* RealOptions.cpp:455-463; epsilon=(float)(filter_mult*patl),
                               RealOptions.hpp:74-77, matchUniqueImplementation.cpp:405;
                               >= 0 (filter levels 0..4), negative or NaN is E_INVALID  */
    double   LL[1024];      /* Scoring::getRawLogScoreTable, index (ref<<8)|(read<<6)|q
                               (Scoring.hpp:70-73); ignored if !scores                */
} real_hip_params;

/* Scoring::init + getScore (Scoring.cpp:61-133,155-171): fills LL for the
 * -similarity -gc -trans -err -gcmut_bias flags; host-side helper.            */
void real_hip_scoring_table(double similarity, double gc, double trans, double err,
                            double gcmut_bias, double LL[1024]);

int  real_hip_create(real_hip_ctx **out, const real_hip_params *p);
void real_hip_destroy(real_hip_ctx *ctx);
/* make the ctx's stream wait for a hipEvent_t the caller recorded on a stream of his own (the asynchronous way to
 * satisfy the "Streams" contract above); returns at once                                                       */
int  real_hip_wait_event(real_hip_ctx *ctx, void *hip_event);
/* -s / -e / -q / -filter_level for the calls that follow, with the resident text and index kept (they depend on
 * -l only): what constructing another UniqueMatcher / AllMatcher over the same ListSet is to the reference
 * (matchUniqueImplementation.cpp:348-367, matchAllImplementation.cpp:240-259).                                  */
int  real_hip_set_match_params(real_hip_ctx *ctx, uint32_t seedkmax, uint32_t totalkmax, uint32_t scores, double filter_mult);
const char *real_hip_strerror(int status);
const char *real_hip_last_error(const real_hip_ctx *ctx);
int  real_hip_abi_version(void);

/* free / total HBM of the ctx's device in bytes: what getPhysicalMemory() * -f is to the
 * reference's block sizing (matchUniqueImplementation.cpp:1208-1244)           */
int real_hip_device_memory(real_hip_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes);

/* ---- genome text: replaces what getText<sse4>() + RangeVector hand the
 * matcher (getText.hpp:31-55, AutoTextArray.hpp:63-109, RangeVector.hpp:46-58).
 * text2bit: 2 bits/base, base i at bits 63-2(i%32)-1.. of word i/32 (MSB
 * first, N stored as 0); wildbits: bit i (MSB first) set iff base i is N;
 * frag_start[n_frag] = n_bases ("terminal", countReads.cpp:81).  Host pointers;
 * copied to HBM.                                                              */
int real_hip_set_text(real_hip_ctx *ctx, uint32_t fileid,
                      const uint64_t *text2bit, const uint64_t *wildbits, uint64_t n_bases,
                      const uint64_t *frag_start, uint32_t n_frag);
/* same from mapped symbols 0..4 (countReads.cpp:83-125 readFile); packed on
 * the device.  sym_on_device != 0: sym is a device pointer.                   */
int real_hip_set_text_symbols(real_hip_ctx *ctx, uint32_t fileid,
                              const uint8_t *sym, uint64_t n_bases, int sym_on_device,
                              const uint64_t *frag_start, uint32_t n_frag);

/* ---- genome index block: what ListSetBlockReader::readNextBlock() exposes
 * (ListSetBlockReader.hpp:24-52, ListSet.hpp:23-31).
 * Host-built form: six lists in the host's sorted order (stable => ascending
 * position inside equal signatures); sign[k] has n_entries elements of
 * sig_bytes (4 if seedl <= 32 else 8, real.cpp:219-229); pos[k][j] = window
 * start of entry j (Mask::getPos, Mask.hpp:36-40,55-59).                      */
int real_hip_set_index_block(real_hip_ctx *ctx, uint64_t n_entries,
                             const void *const sign[6], const uint32_t *const pos[6]);
/* Device-built form: enumerates the N-free windows
 * [first_window, first_window+max_entries) of the resident text
 * (MapTextFile.hpp:118-230), sorts the six lists on the GPU.  Same device
 * arrays as the host-built form.                                              */
int real_hip_build_index_block(real_hip_ctx *ctx, uint64_t first_window, uint64_t max_entries,
                               uint64_t *n_entries, int *have_next);
/* where the wall time of the index builds of this ctx went, accumulated since the last reset: the kernels of the
 * build (HIP events), hipMalloc and hipFree (host clock; the driver maps and clears every page), the rest is
 * synchronisation and host code.  The counterpart of the reference's "Sorting fragments..." clock
 * (ListSetBlockReader.hpp:42-48).                                                                             */
typedef struct real_hip_build_stats {
    uint32_t struct_size, reserved;
    double   wall_ms, kernel_ms, alloc_ms, free_ms;
    uint64_t alloc_bytes, alloc_calls, free_calls;
} real_hip_build_stats;
int real_hip_index_build_stats(real_hip_ctx *ctx, real_hip_build_stats *out, int reset);
/* introspection (tests, CPU baseline): device layout of list k               */
int real_hip_index_info(const real_hip_ctx *ctx, uint64_t *n_entries, uint32_t *prefix_bits);
/* layout of the resident bucket tables: 0 bucket starts, 1 digest directory (group sizes + partner digests), 2 fingerprint directory, 3 bucket rows */
int real_hip_index_table_kind(const real_hip_ctx *ctx, uint32_t *kind);
int real_hip_index_download(real_hip_ctx *ctx, int list,
                            uint32_t *entries      /* n_entries x {key, pos} (raw device layout), nullable */,
                            uint32_t *bucket_start /* 2^prefix_bits + 1, nullable                        */);
/* list k in the reference's own form: sign[j] (sig_bytes each) and pos[j] of
 * the sorted Mask entries (Mask.hpp:22-64); either pointer may be NULL.       */
int real_hip_index_export(real_hip_ctx *ctx, int list, void *sign, uint32_t *pos);

/* ---- read batch: a decoded pattern block (PatternBlock / FastSubDecoder::
 * fillPatternBlock, FastSubDecoder.hpp:107-161): mapped symbols A,C,G,T->0..3,
 * other->4 (acgtnMap.hpp:39-50) and quality = ASCII - offset in 0..63.
 * Quality bytes 64..127 (offset 33 hands over up to 93 for characters up to
 * '~') are taken as the reference takes them: the score's table index is
 * (ref<<8)|(read<<6)|q, so bit 6 of q falls into the read-base bits and the
 * entry read is that of read base (read | 1) with quality q - 64.  Every other
 * stage takes the byte as a number (pileup and call thresholds, quality sums).
 * Bytes 128..255 are outside the reference's defined behaviour (it reads the
 * byte as a signed char and indexes in front of its table): not supported.   */
typedef struct real_hip_batch {
    uint32_t        struct_size;
    uint32_t        on_device;  /* 0: all pointers of the call are host memory (copied);
                                   1: all are device pointers (bases, qual, offsets and the
                                      info / score / hit outputs);
                                   2: bases, qual, offsets are device pointers (e.g. the arrays
                                      real_hip_parse_reads returned), the outputs host memory   */
    uint64_t        n_reads;
    const uint8_t  *bases;      /* concatenated mapped symbols                          */
    const uint8_t  *qual;       /* concatenated qualities; NULL => 30 (Pattern.hpp:42-45) */
    const uint64_t *offsets;    /* n_reads+1 start offsets; NULL => uniform length patl  */
    uint32_t        patl;       /* uniform read length if offsets == NULL               */
    uint32_t        max_patl;   /* upper bound of read length when offsets != NULL and
                                   on_device (0: library computes it); a read that turns out
                                   longer fails the call with REAL_HIP_E_INVALID: its own
                                   record stays as it was, those of other reads of the
                                   batch may have been written by then                    */
    /* -- since ABI version 2 (struct_size tells; a version-1 struct of 48 bytes is still accepted) -- */
    uint32_t        packed;     /* 1: bases holds 2 bits per base instead of a byte: base g of the
                                   concatenated batch at bits 7-2(g%4)-1.. of byte g/4 (MSB first, the
                                   packing of TemporaryFile.hpp:335-373); offsets / patl still count bases */
    uint32_t        fresh;      /* matchUnique: 1 = the records start as uniqueinfo(numpat) does (NoMatch, score -FLT_MAX,
                                   matchUniqueImplementation.cpp:1094-1097, UniqueMatchInfo.hpp:191) and info / score are
                                   outputs only -- the first genome block of a run; 0 = in/out, folds compose          */
    const uint8_t  *nflags;     /* packed only, nullable: bit (i%8) of byte i/8 set => read i holds a symbol
                                   > 3 (it cannot be packed) and is skipped as the reference skips it
                                   (matchUniqueImplementation.cpp:376-394)                              */
} real_hip_batch;

/* matchUnique: replaces the loop over UniqueMatcher::match
 * (matchUniqueImplementation.cpp:369-500) including the best/unique fold
 * UpdateUniqueInfo<scores>::update (:97-160, :179-248).  info[i] is the 64-bit
 * UniqueMatchInfo record {state:3@61, fragment:16@45, errors:4@41, fileid:6@35,
 * pos:35@0} (UniqueMatchInfo.hpp:29-39), score[i] its float (init -FLT_MAX,
 * :191); both in/out so folds compose across genome blocks and files exactly
 * as uniqueinfo[] does (matchUniqueImplementation.cpp:1094-1097).  Reads
 * shorter than seedl or containing a symbol > 3 are skipped (:376-394).
 * score may be NULL iff !scores.  Synchronous on return.                      */
int real_hip_match_unique(real_hip_ctx *ctx, const real_hip_batch *b,
                          uint64_t *info, float *score);

/* Pipelined form for host batches -- the producer/consumer block ring of AsynchronousReader.hpp:181-259 as a
 * two-slot ring: submit queues upload, kernels and download of one batch and returns; the upload of the next
 * batch and the download of the previous records run beside the kernels.  A slot's batch, info and score must
 * stay untouched until real_hip_wait(slot) has returned (its status is the batch's).  For the copies to be
 * asynchronous the host memory has to be pinned: real_hip_host_alloc, or the caller's own hipHostRegister.
 * fresh != 0: the records are initialised on the device (NoMatch, score -FLT_MAX: the state of
 * uniqueinfo(numpat), matchUniqueImplementation.cpp:1094-1097) instead of being uploaded.                   */
#define REAL_HIP_SLOTS 2
int real_hip_match_unique_submit(real_hip_ctx *ctx, const real_hip_batch *b, uint64_t *info, float *score,
                                 uint32_t slot, int fresh);
int real_hip_wait(real_hip_ctx *ctx, uint32_t slot);
void *real_hip_host_alloc(size_t bytes);   /* pinned host memory; NULL on failure */
void  real_hip_host_free(void *p);

/* matchAll: replaces AllMatcher::match + unifyMatches
 * (matchAllImplementation.cpp:261-355, :150-161) for the resident block.      */
typedef struct real_hip_hit {       /* MatchPosAndError, matchAllImplementation.cpp:99-120 */
    uint32_t read;                  /* index inside the batch                              */
    uint32_t pos;                   /* 0-based position in the text of fileid              */
    float    score;                 /* 1.0f if !scores (ComputeScore.hpp:31-45)            */
    uint16_t frag;
    uint8_t  k;                     /* mismatches                                          */
    uint8_t  inverted;              /* 0 '+', 1 '-'                                        */
} real_hip_hit;
/* out[hit_offsets[i] .. hit_offsets[i+1]) = hits of read i in unifyMatches order
 * (k, pos, file, frag, score, inverted; duplicates removed).  cap = capacity of
 * out; on REAL_HIP_E_OVERFLOW *n_out is the size needed.  hit_offsets has
 * n_reads+1 entries (may be NULL).                                            */
int real_hip_match_all(real_hip_ctx *ctx, const real_hip_batch *b,
                       real_hip_hit *out, uint64_t cap, uint64_t *n_out, uint64_t *hit_offsets);

/* ---- paired-end reads: one placement per fragment.  The reference has no paired-end mode; the semantics are this
 * project's own ("Paired-end reads") and are independent of the order of hits, lanes and genome files.
 * Read i of batch 1 and read i of batch 2 are mates.  Candidates of a mate are its real_hip_match_all hits.  A hit f with
 * inverted = 0 of one mate and a hit r with inverted = 1 of the other are CONCORDANT (orientation FR) iff same frag,
 * f.pos <= r.pos, f.pos + len_f <= r.pos + len_r and min_insert <= r.pos + len_r - f.pos <= max_insert (outer distance
 * in bases; either mate may be the forward one).  VALUE of a pair: (double)score1 + (double)score2 with scores on,
 * -(double)(k1 + k2) with scores off.  LOCATION: (fileid, frag, pos1, pos2, inverted1).  The record keeps `best` (highest
 * value; equal values: the smallest location in lexicographic order) and `second` (highest value at any OTHER location,
 * -inf if none); merging two records is taking the top two of their union, so genome files fold in any order.  state:
 * NoMatch without a concordant pair, NonUnique if second >= best - eps, else Unique, with
 * eps = (double)(float)(filter_mult * (len1 + len2)) with scores on and 0 with scores off.                           */
typedef struct real_hip_pair_params {
    uint32_t struct_size;   /* = sizeof(real_hip_pair_params)                                         */
    uint32_t min_insert;    /* bounds of the outer distance, inclusive; min > max is E_INVALID        */
    uint32_t max_insert;
    uint32_t orientation;   /* 0 = FR; anything else is REAL_HIP_E_UNSUPPORTED                        */
} real_hip_pair_params;
enum { REAL_HIP_PAIR_NOMATCH = 0, REAL_HIP_PAIR_UNIQUE = 1, REAL_HIP_PAIR_NONUNIQUE = 2 };
typedef struct real_hip_pair {      /* 40 bytes, 8-byte aligned; in/out across genome files as uniqueinfo[] is   */
    double   best;                  /* value of the best pair; -inf: none (the fields below are then 0)         */
    double   second;                /* highest value at another location; -inf: none                            */
    uint32_t pos1, pos2;            /* 0-based positions of mate 1 / mate 2 in the text of fileid               */
    float    score1, score2;        /* the hits' scores (1.0f if !scores)                                        */
    uint16_t frag;
    uint8_t  fileid;
    uint8_t  k1, k2;                /* mismatches of mate 1 / mate 2                                             */
    uint8_t  inverted1;             /* strand of mate 1 (0 '+', 1 '-'); mate 2 has the other one                 */
    uint8_t  state;                 /* REAL_HIP_PAIR_NOMATCH / _UNIQUE / _NONUNIQUE                               */
    uint8_t  reserved;              /* 0                                                                         */
} real_hip_pair;
/* The join alone, on hit lists the caller holds: hits_m[off_m[i] .. off_m[i+1]) are the candidates of mate m of pair i
 * (any order, e.g. the per-block lists of a genome file that needs several index blocks, concatenated per read),
 * len_m[i] the mate's length in bases (uint32).  on_device: 0 all pointers host memory (copied), 1 all device
 * pointers.  fresh != 0: pairs[] is output only (every record starts empty); 0: in/out, the fold of another genome
 * file.  A hit must not appear twice in one list.  Uses the ctx's -q and -filter_level; needs neither text nor index.  */
int real_hip_pair_hits(real_hip_ctx *ctx, const real_hip_pair_params *pp,
                       const real_hip_hit *hits1, const uint64_t *off1, const uint32_t *len1,
                       const real_hip_hit *hits2, const uint64_t *off2, const uint32_t *len2,
                       uint64_t n_pairs, uint32_t fileid, int on_device, int fresh, real_hip_pair *pairs);
/* matchAll of both mates against the resident text and index block with the hits kept on the device, then the join:
 * only the pair records cross to the host (on_device 0 / 2; 1: pairs is a device pointer).  batch1 and batch2 must
 * agree in n_reads and on_device; batch1->fresh says whether pairs[] is output only.  The hit buffers grow inside
 * (a match is redone when they were too small).  Pairs across index blocks are not seen: a genome file that needs
 * several blocks goes through real_hip_match_all + real_hip_pair_hits.                                            */
int real_hip_match_pairs(real_hip_ctx *ctx, const real_hip_batch *batch1, const real_hip_batch *batch2,
                         const real_hip_pair_params *pp, real_hip_pair *pairs);
/* work of the join, accumulated since the last reset                                                              */
typedef struct real_hip_pair_stats {
    uint32_t struct_size, reserved; /* = sizeof(real_hip_pair_stats), 0                               */
    uint64_t pairs;         /* fragments joined                                                       */
    uint64_t products;      /* sum over the fragments of (hits of mate 1) x (hits of mate 2)          */
    uint64_t handed_over;   /* fragments whose product exceeded a lane's budget: joined by a wave each */
} real_hip_pair_stats;
int real_hip_pair_stats_get(real_hip_ctx *ctx, real_hip_pair_stats *out, int reset);

/* ---- mate search: place a mate the seeds missed (off unless these entry points are called).  real_hip_match_all finds a
 * read only where its first seedl bases carry at most seedkmax mismatches; with pairs the other mate's hit says where
 * the missing mate must lie, and every position there is compared over the whole read.
 * A PLACEMENT of a read on a strand at text position p is what real_hip_match_all would report there if the seed filter
 * did not exist: the read (reverse-complemented for inverted = 1) lies inside one fragment, the window holds no N and
 * the Hamming distance to the text is k <= totalkmax; score as real_hip_match_all computes it (1.0f if !scores), frag
 * the fragment of p.  An ANCHOR is a real_hip_match_all hit of either mate.  The WINDOW of an anchor a is the set of
 * positions p at which a hit of the OTHER mate on the OPPOSITE strand would be concordant with a (the definition above,
 * either mate forward) and lie wholly inside a's fragment; every position of the window is tested for a placement.
 * The candidate set of a fragment in one genome file becomes: all concordant pairs of two hits (as before) PLUS all
 * pairs (anchor, placement found in its window) -- every concordant pair of placements of which at least one mate was
 * found by the seeds.  A location counts once (a placement that is also a hit adds nothing: score and k are functions
 * of the location); value, location, best / second, eps, the states and the fold across files are unchanged, and the
 * set does not depend on the order of hits, lanes or files.  A fragment with a mate the matcher skips (shorter than
 * seedl, a symbol > 3) is not searched.  max_anchors (0 = no limit): a mate with more than max_anchors hits in this
 * file contributes no anchors (its hits still join); the rule looks at the count only.
 * Limits (REAL_HIP_E_UNSUPPORTED before anything is launched): a read longer than REAL_HIP_MAX_PATL, max_insert beyond
 * REAL_HIP_MATE_SEARCH_MAX_INSERT (the text of one window sits in the wave's LDS).                                    */
#define REAL_HIP_MATE_SEARCH_MAX_INSERT 4096u
typedef struct real_hip_mate_search_params {
    uint32_t struct_size;   /* = sizeof(real_hip_mate_search_params)                                  */
    uint32_t max_anchors;   /* 0 = no limit                                                           */
    uint32_t reserved[2];   /* 0                                                                      */
} real_hip_mate_search_params;
/* The search alone, on anchors the caller holds: folds the pairs (anchor, placement in its window) into the in/out
 * records (fresh != 0: output only).  hits_m[off_m[i] .. off_m[i+1]) are the anchors of mate m of fragment i, batch1 /
 * batch2 the mates' reads (same n_reads and on_device; on_device says where ALL pointers of the call live: 0 host
 * memory (copied), 1 device).  Needs the text, not the index.  real_hip_pair_hits followed by this gives the full
 * candidate set: the form for a genome file of several index blocks.                                             */
int real_hip_pair_search(real_hip_ctx *ctx, const real_hip_pair_params *pp, const real_hip_mate_search_params *sp,
                         const real_hip_batch *batch1, const real_hip_batch *batch2,
                         const real_hip_hit *hits1, const uint64_t *off1, const real_hip_hit *hits2, const uint64_t *off2,
                         uint32_t fileid, int fresh, real_hip_pair *pairs);
/* real_hip_match_pairs with the search behind the join: only the pair records cross to the host                   */
int real_hip_match_pairs_search(real_hip_ctx *ctx, const real_hip_batch *batch1, const real_hip_batch *batch2,
                                const real_hip_pair_params *pp, const real_hip_mate_search_params *sp, real_hip_pair *pairs);
/* work of the search, accumulated since the last reset; kernel_ms: HIP events on the ctx's stream around the kernel */
typedef struct real_hip_mate_search_stats {
    uint32_t struct_size, reserved; /* = sizeof(real_hip_mate_search_stats), 0                        */
    uint64_t fragments;       /* fragments handed to the search                                       */
    uint64_t anchors;         /* anchors whose window was searched                                    */
    uint64_t anchors_skipped; /* hits that were no anchors because their mate had more than max_anchors */
    uint64_t positions;       /* window positions tested                                              */
    uint64_t placements;      /* placements found (per anchor: one seen from two anchors counts twice) */
    uint64_t launches;
    double   kernel_ms;
} real_hip_mate_search_stats;
int real_hip_mate_search_stats_get(real_hip_ctx *ctx, real_hip_mate_search_stats *out, int reset);

/* ---- paired-end reads: every concordant pair of a fragment (what matchAll is to matchUnique).  The record of
 * real_hip_match_pairs keeps the values of the top two pairs only; these calls list every concordant pair of two
 * real_hip_match_all hits, with the definition of CONCORDANT above (FR only, either mate forward).  Pairs with a
 * placement only the mate search finds are NOT listed: the enumeration covers pairs of two seed hits.
 * ORDER: out[pair_offsets[i] .. pair_offsets[i+1]) holds the pairs of fragment i, row-major over the product of its two
 * lists -- ascending index of the mate-1 hit in its list, then ascending index of the mate-2 hit.  The output order is a
 * function of the input order alone (nothing is sorted, and nothing depends on lanes or waves); with lists in
 * unifyMatches order (real_hip_match_all's) it is fixed.  A hit must not appear twice in a list.                       */
typedef struct real_hip_pair_hit {   /* 32 bytes, one concordant pair */
    uint32_t pair;        /* index of the fragment inside the batch                                                 */
    uint32_t pos1, pos2;  /* 0-based positions of mate 1 / mate 2 in the text of fileid                             */
    uint32_t outer;       /* outer distance r.pos + len_r - f.pos, the quantity the insert bounds test              */
    float    score1, score2;   /* the hits' scores (1.0f if !scores)                                                */
    uint16_t frag;
    uint8_t  fileid, inverted1, k1, k2;   /* inverted1: strand of mate 1 (0 '+', 1 '-'), mate 2 has the other one   */
    uint16_t reserved;    /* 0 */
} real_hip_pair_hit;
/* The enumeration alone, on hit lists the caller holds; the inputs and on_device are those of real_hip_pair_hits (0: all
 * pointers host memory, 1: all device pointers, out and pair_offsets included; a device out must be 16-byte aligned).
 * Needs neither text nor index.  cap = capacity of out in records; n_out is host memory and always receives the number
 * of pairs; when that exceeds cap the call returns REAL_HIP_E_OVERFLOW and writes nothing to out (the count is known
 * before anything is emitted).  pair_offsets has n_pairs + 1 entries (may be NULL).                                    */
int real_hip_pair_all_hits(real_hip_ctx *ctx, const real_hip_pair_params *pp,
                           const real_hip_hit *hits1, const uint64_t *off1, const uint32_t *len1,
                           const real_hip_hit *hits2, const uint64_t *off2, const uint32_t *len2,
                           uint64_t n_pairs, uint32_t fileid, int on_device,
                           real_hip_pair_hit *out, uint64_t cap, uint64_t *n_out, uint64_t *pair_offsets);
/* matchAll of both mates against the resident text and index block with the hits kept on the device (as
 * real_hip_match_pairs does), then the enumeration: only the pair hits and offsets cross to the host (on_device 0 / 2;
 * 1: out and pair_offsets are device pointers).  fileid is the resident text's.  One index block, as for
 * real_hip_match_pairs: a genome file that needs several goes through real_hip_match_all + real_hip_pair_all_hits.    */
int real_hip_match_pairs_all(real_hip_ctx *ctx, const real_hip_batch *batch1, const real_hip_batch *batch2,
                             const real_hip_pair_params *pp,
                             real_hip_pair_hit *out, uint64_t cap, uint64_t *n_out, uint64_t *pair_offsets);
/* work of the enumeration, accumulated since the last reset.  The count pass of a call that ended in
 * REAL_HIP_E_OVERFLOW is work too: fragments, products and handed_over include it, pairs_out does not.
 * kernel_ms: HIP events on the ctx's stream around the kernels (count + scan, emit)                                    */
typedef struct real_hip_pair_all_stats {
    uint32_t struct_size, reserved; /* = sizeof(real_hip_pair_all_stats), 0                                */
    uint64_t fragments;     /* fragments counted                                                          */
    uint64_t products;      /* sum over the fragments of (hits of mate 1) x (hits of mate 2)              */
    uint64_t pairs_out;     /* concordant pairs written                                                   */
    uint64_t handed_over;   /* fragments whose product exceeded a lane's budget: a wave each              */
    uint64_t launches;      /* kernels launched                                                           */
    double   kernel_ms;
} real_hip_pair_all_stats;
int real_hip_pair_all_stats_get(real_hip_ctx *ctx, real_hip_pair_all_stats *out, int reset);

/* ---- single placements of a mate: where each mate of a fragment lies on its own, for the fragments without a concordant
 * pair (one mate placed and the other not, or both placed but not concordantly).  The semantics are this project's own, in
 * the words of the paired-end block above, and are independent of the order of hits, lanes, waves, index blocks and genome
 * files.  Candidates of a read are its real_hip_match_all hits in one genome file.  VALUE of a hit: (double)score with
 * scores on, -(double)k with scores off (k = 0 gives -0.0).  LOCATION: (fileid, frag, pos, inverted).  The record keeps
 * `best` (highest value; equal values: the smallest location in lexicographic order) and `second` (highest value at any
 * OTHER location, -inf if none; of +0.0 and -0.0 the latter); merging two records is taking the top two of their union,
 * a location counts once, so genome files and index blocks fold in any order.  state: NoMatch without a hit, NonUnique if
 * second >= best - eps (in FP64), else Unique, with eps = (double)(float)(filter_mult * len) with scores on and 0 with
 * scores off; the values are REAL_HIP_PAIR_NOMATCH / _UNIQUE / _NONUNIQUE.
 * This is deliberately NOT the record of real_hip_match_unique: that one reproduces the reference's fold over update()
 * calls, whose outcome depends on the order of the calls (matchUniqueImplementation.cpp:97-160); this one is a function of
 * the set of hits alone, as the pair record is.                                                                       */
typedef struct real_hip_single {    /* 16 bytes, 16-byte aligned on the device (one vector store); in/out across genome files */
    float    score;                 /* the best hit's score (1.0f if !scores)                                              */
    float    second;                /* (float) of the second value (exact: the values are floats or small integers); -inf: none;
                                       -(float)k with scores off (-0.0f for k = 0)                                       */
    uint32_t pos;                   /* 0-based position in the text of fileid                                              */
    uint16_t frag;
    uint8_t  fileid;
    uint8_t  tag;                   /* k in bits 0-3 (k <= 15, as everywhere in this ABI), inverted in bit 4, state in bits 5-6 */
} real_hip_single;
#define REAL_HIP_SINGLE_K(tag)        ((tag) & 15u)
#define REAL_HIP_SINGLE_INVERTED(tag) (((tag) >> 4) & 1u)
#define REAL_HIP_SINGLE_STATE(tag)    (((tag) >> 5) & 3u)
/* A record is empty iff its state is NoMatch: on input its other fields are ignored, on output they are score 0, second
 * -inf, everything else 0.
 * The fold alone, on one mate's lists as the caller holds them: hits[off[i] .. off[i+1]) are the candidates of read i (any
 * order, e.g. the per-block lists of a genome file that needs several index blocks), len[i] its length in bases (uint32).
 * Staging and checks are those of real_hip_pair_hits: on_device 0 all pointers host memory (copied), 1 all device pointers
 * (singles 16-byte aligned); the offsets start at 0 and do not run backwards; fileid <= 255; fresh != 0: singles[] is
 * output only, 0: in/out.  A hit may appear twice (a location counts once).  Uses the ctx's -q and -filter_level; needs
 * neither text nor index.                                                                                             */
int real_hip_single_hits(real_hip_ctx *ctx, const real_hip_hit *hits, const uint64_t *off, const uint32_t *len,
                         uint64_t n_reads, uint32_t fileid, int on_device, int fresh, real_hip_single *singles);
/* real_hip_match_pairs (sp == NULL) or real_hip_match_pairs_search (sp != NULL), and in the same call each mate's
 * device-resident hit list folded into singles1[] / singles2[]: no hit crosses to the host.  batch1->fresh governs all three
 * arrays, on_device where all three live (0 / 2 host memory, 1 device pointers).  pairs[] is bit for bit what the existing
 * calls give.  The singles are folds of SEED hits only: a placement that only the mate search finds is not a candidate
 * of its mate's record.                                                                                               */
int real_hip_match_pairs_singles(real_hip_ctx *ctx, const real_hip_batch *batch1, const real_hip_batch *batch2,
                                 const real_hip_pair_params *pp, const real_hip_mate_search_params *sp, real_hip_pair *pairs,
                                 real_hip_single *singles1, real_hip_single *singles2);
/* work of the fold, accumulated since the last reset; kernel_ms: HIP events on the ctx's stream around the kernels     */
typedef struct real_hip_single_stats {
    uint32_t struct_size, reserved; /* = sizeof(real_hip_single_stats), 0                                       */
    uint64_t reads;         /* reads folded                                                                    */
    uint64_t hits;          /* hits walked                                                                     */
    uint64_t handed_over;   /* reads whose list exceeded a lane's budget: folded by a wave each                */
    uint64_t launches;      /* kernels launched                                                                */
    double   kernel_ms;
} real_hip_single_stats;
int real_hip_single_stats_get(real_hip_ctx *ctx, real_hip_single_stats *out, int reset);

/* ---- insert sizes: the histogram of the Unique fragments' outer distances, computed where the pair records live, and the
 * insert bounds it suggests.  The OUTER DISTANCE of a record is r.pos + len_r - f.pos in 64-bit arithmetic, the quantity the
 * insert bounds of CONCORDANT test; the forward mate f is mate 1 iff inverted1 == 0, r is the other one.  Only records with
 * state == REAL_HIP_PAIR_UNIQUE count.  hist[d] counts the records with outer == d for d < n_bins - 1, hist[n_bins - 1]
 * those with outer >= n_bins - 1 (the overflow bin).  A Unique record that is no valid placement -- the forward mate starts
 * behind the reverse one, or the reverse mate ends before the forward one starts -- goes nowhere in hist and is counted as
 * `invalid` in the stats: sum(hist) is the number of valid Unique records.  The counts are integers and a function of the
 * set of records alone (nothing depends on lanes, blocks or the order of the records).
 * fresh != 0: hist is output only; 0: the counts are added to what hist holds (the next batch, the next call).  on_device
 * 0: all pointers host memory (copied), 1: all device pointers, hist included.  n_bins in 2 .. REAL_HIP_INSERT_HIST_MAX_BINS,
 * else REAL_HIP_E_INVALID; n_pairs == 0 is valid (a fresh hist is cleared).  Needs neither text nor index.             */
#define REAL_HIP_INSERT_HIST_MAX_BINS 16384u   /* one block's private histogram sits in LDS: 64 KiB of the CU's 160 */
#define REAL_HIP_INSERT_MIN_COUNT 32u          /* the fewest valid Unique records `real` takes insert bounds from   */
int real_hip_pair_insert_hist(real_hip_ctx *ctx, const real_hip_pair *pairs, const uint32_t *len1, const uint32_t *len2,
                              uint64_t n_pairs, int on_device, int fresh, uint32_t n_bins, uint64_t *hist);
/* Insert bounds from a histogram by the quartile rule BWA-MEM uses for its mapping bounds; host only, integers only.
 * n = sum(hist); q_j (j = 1, 2, 3) is the smallest d with hist[0] + .. + hist[d] >= (j * n + 3) / 4 (integer division);
 * iqr = q3 - q1; low = q1 - min(q1, iqr_mult * iqr); high = min(UINT32_MAX, q3 + iqr_mult * iqr), formed in 64 bits.
 * `real` calls it with iqr_mult = 3.  n < min_count (or n == 0): REAL_HIP_E_STATE; q3 in the overflow bin (the histogram is too
 * narrow to say): REAL_HIP_E_OVERFLOW; null pointers, a wrong struct_size or n_bins < 2: REAL_HIP_E_INVALID.            */
typedef struct real_hip_insert_estimate {
    uint32_t struct_size, reserved; /* = sizeof(real_hip_insert_estimate), 0                          */
    uint64_t n;                     /* sum(hist)                                                      */
    uint32_t q1, median, q3;        /* the quartiles of the outer distance                            */
    uint32_t low, high;             /* the suggested bounds, inclusive                                */
    uint32_t pad;                   /* 0                                                              */
} real_hip_insert_estimate;
int real_hip_insert_bounds(const uint64_t *hist, uint32_t n_bins, uint64_t min_count, uint32_t iqr_mult, real_hip_insert_estimate *out);
/* work of the histogram, accumulated since the last reset; kernel_ms: HIP events on the ctx's stream around the kernel  */
typedef struct real_hip_insert_stats {
    uint32_t struct_size, reserved; /* = sizeof(real_hip_insert_stats), 0                             */
    uint64_t records;       /* records handed in                                                      */
    uint64_t counted;       /* valid Unique records: what was added to hist, the overflow bin included */
    uint64_t overflow;      /* of those, the ones that went to the overflow bin                       */
    uint64_t invalid;       /* Unique records that are no valid placement                             */
    uint64_t launches;      /* kernels launched                                                       */
    double   kernel_ms;
} real_hip_insert_stats;
int real_hip_insert_stats_get(real_hip_ctx *ctx, real_hip_insert_stats *out, int reset);

/* ---- pileup: what the final placements add up to over one genome file -- the depth of every text position and, where a
 * placed read shows another base than the text, how often each base was seen.  The reference has no such output; the
 * semantics are this project's own.  The pileup covers the RESIDENT text: n bases, file id f.  A PLACEMENT
 * is a read of length L at 0-based text position p on a strand, with p + L <= n; its ORIENTED base at text position p + i is
 * read[i] with quality qual[i] on the forward strand and 3 - read[L-1-i] with quality qual[L-1-i] on the reverse strand (a
 * batch without qualities counts as quality 30).  Single-end: every info record of state 1 or 2 (Unique forward / reverse,
 * UniqueMatchInfo.hpp:29-39) is a placement of its read at the record's pos, on the reverse strand iff the state is 2.
 * Paired-end: every real_hip_pair of state REAL_HIP_PAIR_UNIQUE gives two placements, mate 1 at pos1 on strand inverted1
 * and mate 2 at pos2 on the other strand.  Records of another state are skipped; then records of another file id than f are
 * skipped and counted as other_file; then a placement with p + L > n is skipped and counted as invalid (per read: a pair
 * record counts once for each mate).
 *   depth[x]   = the number of placements with p <= x < p + L (no quality filter);
 *   alt[x][b]  = the number of placements covering x whose oriented base at x is b != ref[x] (the 2-bit text, N stored as
 *                0), whose quality there is >= min_qual, and where the text's N bit at x is clear;
 *   a SITE is a position with alt[x][0] + .. + alt[x][3] > 0; the site list is in ascending position.
 * All results are integer sums: nothing depends on the order of reads, batches, lanes or calls, and two add calls give
 * exactly what one call on the concatenated batch gives.
 * Device memory: the accumulators are a dense table of 4 x u32 per text position and the depth's difference array of
 * n + 1 u32 (scanned in place by finish): 20 bytes per base, 60 GB for a text of 3 Gbp.  begin fails with
 * REAL_HIP_E_NOMEM and a message when that does not fit.
 * Protocol: begin (needs the text, not the index; allocates and zeroes; a second begin starts again), any number of add /
 * add_pairs, finish (synchronises; once per begin), depth / sites any number of times, end (releases the accumulators).
 * add without begin, after finish, or after the text was replaced by one of another n_bases or file id (finish likewise:
 * it takes the sites' reference bases from the text), and finish / depth / sites out of turn are REAL_HIP_E_INVALID with
 * a message, nothing launched; a finish that fails for another reason ends the pileup as end does; so are more than 2^32 reads in one
 * call and a depth window that reaches beyond n.
 * info / pairs live where the records of real_hip_match_unique / real_hip_match_pairs live for the batch's on_device:
 * host memory for 0 and 2, device memory for 1 -- a caller passes the arrays it matched with.  Reads of any length up
 * to REAL_HIP_MAX_PATL_LONG.                                                                                       */
typedef struct real_hip_pileup_params {
    uint32_t struct_size;   /* = sizeof(real_hip_pileup_params)                                       */
    uint32_t min_qual;      /* a mismatch of lower quality is not counted in alt (0: qualities are not read); <= 63 */
} real_hip_pileup_params;
typedef struct real_hip_pileup_site {   /* 32 bytes */
    uint32_t pos;           /* 0-based position in the text                                           */
    uint32_t depth;
    uint32_t alt[4];        /* alt[ref] is 0                                                          */
    uint32_t ref;           /* the text's base 0..3                                                   */
    uint32_t reserved;      /* 0                                                                      */
} real_hip_pileup_site;
int real_hip_pileup_begin(real_hip_ctx *ctx, const real_hip_pileup_params *p);
int real_hip_pileup_add(real_hip_ctx *ctx, const real_hip_batch *b, const uint64_t *info);
/* batch1 and batch2 must agree in n_reads and on_device                                              */
int real_hip_pileup_add_pairs(real_hip_ctx *ctx, const real_hip_batch *b1, const real_hip_batch *b2, const real_hip_pair *pairs);
int real_hip_pileup_finish(real_hip_ctx *ctx, uint64_t *n_sites);
/* depth[first .. first + count) into depth (host memory, or device memory if on_device); after finish */
int real_hip_pileup_depth(real_hip_ctx *ctx, uint64_t first, uint64_t count, uint32_t *depth, int on_device);
/* the site list into out (cap records; host memory, or device memory if on_device); *n_out (host memory) always receives
 * the number of sites; when that exceeds cap the call returns REAL_HIP_E_OVERFLOW and writes nothing to out; after finish */
int real_hip_pileup_sites(real_hip_ctx *ctx, real_hip_pileup_site *out, uint64_t cap, uint64_t *n_out, int on_device);
int real_hip_pileup_end(real_hip_ctx *ctx);
/* work of the pileup.  reads .. n_dropped, launches and kernel_ms are accumulated since the last reset; covered, sites
 * and max_depth are those of the last finish (0 from begin until then).  A mismatch is tested for quality first, then
 * for the N bit: low_qual counts the mismatches min_qual dropped, n_dropped those of sufficient quality on an N.      */
typedef struct real_hip_pileup_stats {
    uint32_t struct_size, reserved; /* = sizeof(real_hip_pileup_stats), 0                             */
    uint64_t reads;         /* reads handed in (a pair counts two)                                    */
    uint64_t placed;        /* placements piled up                                                    */
    uint64_t other_file;    /* placed reads of another file id                                        */
    uint64_t invalid;       /* placements that end behind the text                                    */
    uint64_t bases;         /* sum of L over the placements = sum of depth[]                          */
    uint64_t mismatches;    /* increments of alt                                                      */
    uint64_t low_qual;      /* mismatches that min_qual dropped                                       */
    uint64_t n_dropped;     /* mismatches on an N of the text                                         */
    uint64_t covered;       /* positions with depth > 0                                               */
    uint64_t sites;
    uint64_t max_depth;
    uint64_t launches;      /* kernels launched (the scans of finish count one each)                  */
    double   kernel_ms;     /* HIP events on the ctx's stream around the kernels of add and finish    */
} real_hip_pileup_stats;
int real_hip_pileup_stats_get(real_hip_ctx *ctx, real_hip_pileup_stats *out, int reset);

/* ---- variant calls: which sites of a finished pileup are single-base variants, and with which genotype.  The reference has
 * no caller; the semantics are this project's own.  PLACEMENT, ORIENTED base, the resident text, the state,
 * file-id and validity skips, and "a batch without qualities counts 30" are the pileup's, word for word.  The calls sit on
 * a FINISHED pileup: its sites (ascending position; slot s = index in the site list) and its min_qual.
 * EVIDENCE, per site s at text position x: for every placement covering x take its oriented base b there with quality q; if
 * q >= min_qual, cnt[s][b] += 1 and qsum[s][b] += q (b == ref included), otherwise low_qual += 1.  All counters are u32:
 * more than 2^26 placements on one position are out of scope (qsum and QUAL would wrap).  The text's N bit is clear at
 * every site by construction, so for b != ref cnt[s][b] == site.alt[b] when the same records were added to both.
 * GENOTYPE, per site, in integers in phred units: E[b] = qsum[b] + REAL_HIP_CALL_ERR * cnt[b] (an error towards one given
 * base, e/3).  Genotypes (a, b), a <= b, over the bases 0..3:
 *   PL(a,a) = sum over d != a of E[d]
 *   PL(a,b) = REAL_HIP_CALL_HET * (cnt[a] + cnt[b]) + sum over d not in {a, b} of E[d]
 * plus a prior on every genotype but (ref, ref): REAL_HIP_CALL_PRIOR_HET for a heterozygote holding ref,
 * REAL_HIP_CALL_PRIOR_HOM for a homozygote of another base, REAL_HIP_CALL_PRIOR_HET2 for a heterozygote of two other bases.
 * The ten genotypes are ordered (ref, ref) first, then the other nine by ascending (a, b); the best is the first of minimal
 * PL.  QUAL = PL(ref,ref) - PL(best) (as u32; beyond 2^32 - 1 it counts as that), GQ = min(99, smallest other PL -
 * PL(best)), DP = cnt[0] + .. + cnt[3].  A CALL is a site with best != (ref, ref), QUAL >= min_call_qual and DP >=
 * min_depth; the call list is in ascending position.  Everything is an integer sum or a function of one: nothing depends
 * on the order of reads, lanes, batches or calls.
 * Device memory beside what the pileup holds until its end: one bit per text position, a u32 per 64 positions and 32 bytes
 * per site (n/8 + n/16 + 32 * sites bytes); begin fails with REAL_HIP_E_NOMEM and a message when that does not fit.
 * Protocol: call_begin (needs a finished pileup of the resident text; a second begin starts again), any number of call_add /
 * call_add_pairs, call_finish (synchronises; may be called again with other thresholds, it only re-reads the evidence),
 * call_evidence / call_variants any number of times after a finish, call_end.  real_hip_pileup_end and a new
 * real_hip_pileup_begin end the calls as well.  Calls out of turn, a text replaced by one of another n_bases or file id and
 * more than 2^32 reads in one call are REAL_HIP_E_INVALID with a message, nothing launched.  A pileup with zero sites is
 * valid: zero calls.  Records and batches live where the pileup's live for the batch's on_device.                      */
#define REAL_HIP_CALL_HET        3u  /* phred cost of a read of either allele under a heterozygote: -10 log10(1/2)      */
#define REAL_HIP_CALL_ERR        5u  /* added to a base's quality: an error towards one given base of three (e/3)       */
#define REAL_HIP_CALL_PRIOR_HET  30u /* heterozygote holding the reference base                                         */
#define REAL_HIP_CALL_PRIOR_HOM  33u /* homozygote of another base                                                      */
#define REAL_HIP_CALL_PRIOR_HET2 60u /* heterozygote of two other bases                                                 */
typedef struct real_hip_call_params {
    uint32_t struct_size;   /* = sizeof(real_hip_call_params)                                         */
    uint32_t min_call_qual; /* a call needs QUAL >= this                                              */
    uint32_t min_depth;     /* and DP >= this                                                         */
} real_hip_call_params;
typedef struct real_hip_call_evidence_rec {   /* 32 bytes; record s belongs to site s of the pileup */
    uint32_t cnt[4];        /* bases of quality >= min_qual seen at the site, the reference base too  */
    uint32_t qsum[4];       /* the sums of their qualities                                            */
} real_hip_call_evidence_rec;
typedef struct real_hip_call {   /* 32 bytes */
    uint32_t pos;           /* 0-based position in the text                                           */
    uint32_t depth;         /* the site's depth (no quality filter)                                   */
    uint32_t cnt[4];        /* the evidence's counts: DP is their sum                                 */
    uint32_t qual;          /* QUAL                                                                   */
    uint8_t  ref, a1, a2;   /* the text's base; the genotype (a1 <= a2)                               */
    uint8_t  gq;            /* GQ                                                                     */
} real_hip_call;
int real_hip_call_begin(real_hip_ctx *ctx);
int real_hip_call_add(real_hip_ctx *ctx, const real_hip_batch *b, const uint64_t *info);
/* batch1 and batch2 must agree in n_reads and on_device                                              */
int real_hip_call_add_pairs(real_hip_ctx *ctx, const real_hip_batch *b1, const real_hip_batch *b2, const real_hip_pair *pairs);
int real_hip_call_finish(real_hip_ctx *ctx, const real_hip_call_params *p, uint64_t *n_calls);
/* the evidence table (one record per site of the pileup) / the call list into out (cap records; host memory, or device
 * memory if on_device); *n_out (host memory) always receives the number of records; when that exceeds cap the call returns
 * REAL_HIP_E_OVERFLOW and writes nothing to out; after finish                                                          */
int real_hip_call_evidence(real_hip_ctx *ctx, real_hip_call_evidence_rec *out, uint64_t cap, uint64_t *n_out, int on_device);
int real_hip_call_variants(real_hip_ctx *ctx, real_hip_call *out, uint64_t cap, uint64_t *n_out, int on_device);
int real_hip_call_end(real_hip_ctx *ctx);
/* work of the calls.  reads .. low_qual, launches and kernel_ms are accumulated since the last reset; calls, het and hom
 * are those of the last finish (0 from begin until then)                                                               */
typedef struct real_hip_call_stats {
    uint32_t struct_size, reserved; /* = sizeof(real_hip_call_stats), 0                               */
    uint64_t reads;         /* reads handed in (a pair counts two)                                    */
    uint64_t placed;        /* placements walked                                                      */
    uint64_t other_file;    /* placed reads of another file id                                        */
    uint64_t invalid;       /* placements that end behind the text                                    */
    uint64_t site_bases;    /* increments of cnt                                                      */
    uint64_t low_qual;      /* bases over a site that min_qual dropped                                */
    uint64_t calls;
    uint64_t het;           /* calls with a1 != a2                                                    */
    uint64_t hom;
    uint64_t launches;      /* kernels launched (the scan of finish counts one)                       */
    double   kernel_ms;     /* HIP events on the ctx's stream around the kernels of begin, add, finish */
} real_hip_call_stats;
int real_hip_call_stats_get(real_hip_ctx *ctx, real_hip_call_stats *out, int reset);

/* ---- mismatch lists: where each finally placed read differs from the resident text -- what NM / MD of a SAM line are
 * written from.  The reference has no such output; the semantics are this project's own.  PLACEMENT, ORIENTED
 * base, the resident text (n bases, file id f) are the pileup's, word for word.
 * Single-end (real_hip_mismatches): read i is list i.  An info record of state 1 or 2 is a placement of its read at the
 * record's pos, on the reverse strand iff the state is 2; the mismatch count it carries is its errors field.
 * Paired-end (real_hip_mismatches_pairs): mate 1 of fragment i is list 2i, mate 2 list 2i + 1.  The FINAL placement of a
 * mate: if the pair record's state is REAL_HIP_PAIR_UNIQUE, mate 1 lies at pos1 on strand inverted1 with k1 mismatches, mate
 * 2 at pos2 on the other strand with k2; otherwise, if singles are given AND the pair record's state is REAL_HIP_PAIR_NOMATCH
 * AND the mate's single record is Unique, the mate lies at the single's pos on the single's strand with REAL_HIP_SINGLE_K
 * mismatches (the rule `real -unpaired` prints by); a NonUnique pair record places nothing, whatever the singles say.
 * A record of another state gets an empty list; then a record of another file id than f gets an empty list and is counted as
 * other_file; then a placement with p + L > n gets an empty list and is counted as invalid.
 * The list of a placement holds every offset i in 0 .. L-1 where the text's N bit at p + i is set (ref = 4, whatever the
 * read shows) and, elsewhere, every offset where the oriented base differs from the 2-bit text; ascending offset.  A placed
 * read holds symbols 0..3 only (the matcher places no other read): the lists of a read with another symbol are undefined.
 * out[mm_offsets[j] .. mm_offsets[j+1]) is list j; mm_offsets has one entry more than there are lists and starts at 0.
 * The output is a function of records, reads and text alone: nothing depends on lanes, blocks or calls, and two calls on
 * the halves of a batch give the lists of one call on the whole, up to rebasing the offsets.
 * info / pairs / singles live where the match left them for the batch's on_device: host memory for 0 and 2, device memory
 * for 1 (pairs 8-byte, singles 16-byte aligned).  out and mm_offsets are host memory for 0 and 2 and device memory for 1
 * (out 4-byte aligned); n_out is host memory and always receives the total.  When the total exceeds cap the call returns
 * REAL_HIP_E_OVERFLOW and writes nothing to out (mm_offsets is still written): the count is known before anything is
 * emitted, the protocol of real_hip_pair_all_hits.  n_reads == 0 is valid: mm_offsets[0] = 0.  The calls need the text,
 * not the index: REAL_HIP_E_STATE without it.  REAL_HIP_E_INVALID with a message, nothing launched: a NULL mm_offsets or
 * n_out, a NULL out with cap > 0, NULL records with n_reads > 0, one singles pointer without the other, batches that
 * disagree in n_reads or on_device, more than 2^32 reads.  Reads of any length up to REAL_HIP_MAX_PATL_LONG.            */
typedef struct real_hip_mismatch {   /* 4 bytes */
    uint16_t off;    /* 0-based offset from the placement's text position p: text position p + off; < L <= 16384 */
    uint8_t  ref;    /* the text's base 0..3, or 4 where the text's N bit is set                                  */
    uint8_t  base;   /* the read's ORIENTED base there, 0..3                                                      */
} real_hip_mismatch;
int real_hip_mismatches(real_hip_ctx *ctx, const real_hip_batch *b, const uint64_t *info,
                        real_hip_mismatch *out, uint64_t cap, uint64_t *n_out, uint64_t *mm_offsets /* n_reads + 1 */);
int real_hip_mismatches_pairs(real_hip_ctx *ctx, const real_hip_batch *b1, const real_hip_batch *b2, const real_hip_pair *pairs,
                              const real_hip_single *singles1, const real_hip_single *singles2 /* both or neither NULL */,
                              real_hip_mismatch *out, uint64_t cap, uint64_t *n_out, uint64_t *mm_offsets /* 2 * n_reads + 1 */);
/* work of the lists, accumulated since the last reset.  disagree counts the placements whose list length differs from the
 * mismatch count their record carries: the cross-check between the matcher's verification and this kernel, 0 for records
 * that come from this library's matchers (they place no read over an N).                                                 */
typedef struct real_hip_mismatch_stats {
    uint32_t struct_size, reserved; /* = sizeof(real_hip_mismatch_stats), 0                           */
    uint64_t reads;         /* lists asked for (a pair counts two)                                    */
    uint64_t placed;        /* placements walked                                                      */
    uint64_t other_file;    /* placed reads of another file id                                        */
    uint64_t invalid;       /* placements that end behind the text                                    */
    uint64_t bases;         /* sum of L over the placements                                           */
    uint64_t mismatches;    /* entries written, or counted by a call that overflowed                  */
    uint64_t on_n;          /* of those, the entries with ref = 4                                     */
    uint64_t disagree;      /* placements whose list length is not the record's mismatch count        */
    uint64_t launches;      /* kernels launched (the scan counts one)                                 */
    double   kernel_ms;     /* HIP events on the ctx's stream around count, scan and emit             */
} real_hip_mismatch_stats;
int real_hip_mismatch_stats_get(real_hip_ctx *ctx, real_hip_mismatch_stats *out, int reset);

/* ---- duplicates: which placed reads (fragments) are copies of one another -- PCR / optical duplicates as samtools markdup
 * and Picard MarkDuplicates mark them.  The reference has no such step; the semantics are this project's own.
 * Every result is a function of the input arrays alone: nothing depends on lanes, blocks, the sort's internals or the order
 * of calls.
 * READ SUMMARY (real_hip_read_summary): len is the read's length, qsum the sum of the read's qualities that are >= min_qual
 * (a batch without qualities counts 30 per base: 30 * len if min_qual <= 30, else 0).  Every read of the batch gets one, also
 * the reads the matcher skips.  min_qual <= 63, else REAL_HIP_E_INVALID.  The call needs neither text nor index and does not
 * read the bases (packed or not: the qualities stay bytes).  Reads up to REAL_HIP_MAX_PATL_LONG: qsum <= 16384 * 63 < 2^20.
 * out lives where the batch's outputs live: host memory for on_device 0 and 2, device memory for 1.
 * SINGLE-END (real_hip_mark_duplicates): a read is PLACED iff its info record has state 1 or 2.  Its END5 is pos for state
 * 1 and pos + len - 1 for state 2 (len from its summary), in 64 bits.  Its KEY is (fileid, state, END5): the fragment is
 * implied by the text position.  A GROUP is the set of placed reads of one KEY; its REPRESENTATIVE the read with the largest
 * qsum, among equals the one of the smallest index.  dup[i] = 1 iff read i is placed and is not its group's representative,
 * else 0.  No validity test is made (the marking needs no text).
 * PAIRED-END (real_hip_mark_duplicates_pairs): a fragment is PLACED iff its real_hip_pair has state REAL_HIP_PAIR_UNIQUE.  The
 * forward mate f is mate 1 iff inverted1 == 0, r is the other one; START = f.pos, END = r.pos + len_r - 1 in 64 bits; KEY =
 * (fileid, inverted1, START, END); the quality of a fragment is qsum1 + qsum2; representative and dup[] as above, one byte
 * per fragment.  Single records of unpaired mates take no part.
 * SINGLE-END WITH GAPPED PLACEMENTS (real_hip_mark_duplicates_gapped): read i has an info word and a gap record
 * (real_hip_match_gapped's).  It is PLACED UNGAPPED iff its info word has state 1 or 2 -- the single-end rule, with its END5 and
 * its reverse bit (state 2).  Otherwise it is PLACED GAPPED iff gaps[i] has state REAL_HIP_PAIR_UNIQUE: the info word wins
 * where both hold, a NonUnique or NoMatch gap record places nothing.  Of a gapped placement reverse =
 * REAL_HIP_GAP_INVERTED(tag) and END5 = pos if forward, pos + len + gap - 1 if reverse (len from the summary; gap > 0 is a
 * deletion, gap < 0 an insertion: len + gap is the span on the text), in 64 bits and then modulo 2^36; the file id is taken
 * modulo 64.  KEY = (fileid, reverse, END5) is ONE key space for both kinds: a gapped and an ungapped read of one key are one
 * group.  Representative and dup[] as above.  When no gap record is Unique, dup[] is real_hip_mark_duplicates' bit for bit and
 * the statistics count the same; placed, groups and duplicates count both kinds.  gaps: host memory, or 16-byte aligned device
 * memory; NULL with n > 0 or misaligned: REAL_HIP_E_INVALID, nothing launched; 16 more bytes per record when staged.
 * Both: a qsum beyond 2^20 - 1 counts as 2^20 - 1; END5 is taken modulo 2^36 and END modulo 2^33 (summaries of
 * real_hip_read_summary and records of this library's matchers stay inside).  on_device 0: all pointers host memory
 * (copied), 1: all device pointers, dup included (pairs 8-byte, summaries 8-byte aligned).  n == 0 is valid.  NULL arrays
 * with n > 0 or more than 2^32 records: REAL_HIP_E_INVALID with a message, nothing launched; buffers that do not fit (24 bytes
 * per record single-end, 40 paired-end, beside the sort's own): REAL_HIP_E_NOMEM.                                          */
typedef struct real_hip_read_sum {
    uint32_t len;    /* bases                                        */
    uint32_t qsum;   /* sum of the qualities >= min_qual             */
} real_hip_read_sum;
int real_hip_read_summary(real_hip_ctx *ctx, const real_hip_batch *b, uint32_t min_qual, real_hip_read_sum *out);
int real_hip_mark_duplicates(real_hip_ctx *ctx, const uint64_t *info, const real_hip_read_sum *sum,
                             uint64_t n_reads, int on_device, uint8_t *dup);
struct real_hip_gap_place; /* (defined below, "gap rescue") */
int real_hip_mark_duplicates_gapped(real_hip_ctx *ctx, const uint64_t *info, const struct real_hip_gap_place *gaps,
                                    const real_hip_read_sum *sum, uint64_t n_reads, int on_device, uint8_t *dup);
int real_hip_mark_duplicates_pairs(real_hip_ctx *ctx, const real_hip_pair *pairs, const real_hip_read_sum *sum1,
                                   const real_hip_read_sum *sum2, uint64_t n_pairs, int on_device, uint8_t *dup);
/* work of the marking, accumulated since the last reset.  placed, groups and duplicates count the marking calls; launches and
 * kernel_ms (HIP events on the ctx's stream around the kernels) also those of real_hip_read_summary; a sort counts as one
 * launch                                                                                                                */
typedef struct real_hip_dup_stats {
    uint32_t struct_size, reserved; /* = sizeof(real_hip_dup_stats), 0                                */
    uint64_t reads;         /* records handed in to the marking calls                                 */
    uint64_t placed;        /* placed reads or fragments                                              */
    uint64_t groups;
    uint64_t duplicates;    /* placed - groups                                                        */
    uint64_t launches;
    double   kernel_ms;
} real_hip_dup_stats;
int real_hip_dup_stats_get(real_hip_ctx *ctx, real_hip_dup_stats *out, int reset);

/* ---- mapping quality: how sure a placement is, from ALL candidate locations of its read (fragment), not only the top two the
 * records keep.  The reference has no such output; the semantics are this project's own.  Everything is integer
 * arithmetic on the candidate multiset: nothing depends on the order of hits, lanes, waves, index blocks or genome files, and
 * every result can be checked bit for bit.  Off unless these entry points are called.
 * LEVEL of a candidate, one level = half a bit of log2-odds:
 *   scores on   L = (int32) floor(2 * v), v the candidate's value as a double: (double)score of a hit, (double)score1 +
 *               (double)score2 of a concordant pair (exact); a value whose 2 * v lies outside int32 counts as INT32_MIN + 1 /
 *               INT32_MAX (no score of this library's matchers comes near)
 *   scores off  L = -REAL_HIP_MAPQ_MISMATCH_LEVELS * k, or * (k1 + k2) for a pair: six bits per mismatch.  This is a CONVENTION,
 *               not a calibration: it only makes the mismatch counts comparable on the scale the scores live on.
 * ACCUMULATOR (real_hip_mapq_acc, in/out across index blocks and genome files as uniqueinfo[] is): level = the highest level
 * seen; n = the candidates seen, saturating at 2^32 - 1; cnt[j] = the candidates at level - j, saturating at 255; candidates
 * more than REAL_HIP_MAPQ_LEVELS - 1 levels below `level` are dropped (they still count in n).  EMPTY: n = 0, level = INT32_MIN,
 * every cnt 0; an accumulator with n = 0 is empty whatever its other fields say on input.  MERGE of two accumulators: align
 * both to the larger level, shift the other's counts down (what leaves the window is dropped), add with saturation.  The merge
 * is associative and commutative; the window's top only rises, so what is dropped lies outside the final window too, and the
 * result is a function of the candidate multiset alone.  A hit must not appear twice across the lists folded into one
 * accumulator (real_hip_match_all's lists of different index blocks and files satisfy this).
 * QUALITY of a placement of level Lp against an accumulator: j = level - Lp.  If j < 0, j > 31 or cnt[j] == 0 the placement is
 * UNLISTED (a placement only the mate search found is the case in mind): a one-candidate accumulator at Lp is merged into a
 * copy first and j recomputed.  With W[j] = round(2^24 * 2^(-j/2)) and A[Q] = round(16 * 10^(Q/10)), the literals below:
 *   S = sum over t of cnt[t] * W[t],  E = S - W[j],  MAPQ = max{ Q in 0..60 : E * A[Q] <= 16 * S }
 * all in uint64 (S < 2^34, E * A[60] < 2^58): the phred-scaled share of the other candidates in the total weight, capped at
 * 60.  A lone candidate gives 60, two candidates at one level 3.  An accumulator that is empty before the merge gives 60.  An
 * unlisted placement more than 31 levels below `level` is dropped by that merge as any candidate is: W[j] counts as 0 for
 * j > 31 and the quality is 0.                                                                                                  */
#define REAL_HIP_MAPQ_LEVELS 32
#define REAL_HIP_MAPQ_MISMATCH_LEVELS 12
#define REAL_HIP_MAPQ_MAX 60u
#define REAL_HIP_MAPQ_NONE 255u   /* the MAPQ of a read (mate) without a final placement: SAM's "not available" */
#define REAL_HIP_MAPQ_W_INIT { 16777216, 11863283, 8388608, 5931642, 4194304, 2965821, 2097152, 1482910, 1048576, 741455, 524288, \
        370728, 262144, 185364, 131072, 92682, 65536, 46341, 32768, 23170, 16384, 11585, 8192, 5793, 4096, 2896, 2048, 1448, 1024, \
        724, 512, 362 }
#define REAL_HIP_MAPQ_A_INIT { 16, 20, 25, 32, 40, 51, 64, 80, 101, 127, 160, 201, 254, 319, 402, 506, 637, 802, 1010, 1271, 1600, \
        2014, 2536, 3192, 4019, 5060, 6370, 8019, 10095, 12709, 16000, 20143, 25358, 31924, 40190, 50596, 63697, 80190, 100953, \
        127093, 160000, 201428, 253583, 319242, 401902, 505964, 636971, 801900, 1009532, 1270925, 1600000, 2014281, 2535829, \
        3192420, 4019018, 5059644, 6369715, 8018996, 10095318, 12709252, 16000000 }
typedef struct real_hip_mapq_acc {   /* 40 bytes, 8-byte aligned on the device */
    int32_t  level;                  /* the highest level seen; INT32_MIN: empty                       */
    uint32_t n;                      /* candidates seen, saturating                                    */
    uint8_t  cnt[REAL_HIP_MAPQ_LEVELS]; /* cnt[j]: candidates at level - j, saturating at 255          */
} real_hip_mapq_acc;
/* Host-only helpers, of the standing of real_hip_insert_bounds (no ctx, no GPU; the arithmetic is the kernels', compiled from
 * the same header).  merge: a := merge(a, b).  of: the quality (0..60) of a placement of level `level`; *unlisted (nullable)
 * receives 1 if the placement was unlisted, else 0.  NULL a / b / acc: REAL_HIP_E_INVALID.                                     */
int real_hip_mapq_acc_merge(real_hip_mapq_acc *a, const real_hip_mapq_acc *b);
int real_hip_mapq_of(const real_hip_mapq_acc *acc, int32_t level, int *unlisted);
/* The folds alone, on hit lists the caller holds.  real_hip_mapq_hits: the candidates of read i are hits[off[i] .. off[i+1]);
 * staging and checks are those of real_hip_single_hits (on_device 0: all pointers host memory, 1: all device pointers, acc
 * 8-byte aligned; the offsets start at 0 and do not run backwards; fresh != 0: acc[] is output only, 0: in/out).
 * real_hip_mapq_pair_hits: the candidates of fragment i are the CONCORDANT pairs (the paired-end block above) among its two
 * mates' lists; inputs and checks are those of real_hip_pair_hits.  Both use the ctx's -q; they need neither text nor index.    */
int real_hip_mapq_hits(real_hip_ctx *ctx, const real_hip_hit *hits, const uint64_t *off, uint64_t n_reads, int on_device, int fresh,
                       real_hip_mapq_acc *acc);
int real_hip_mapq_pair_hits(real_hip_ctx *ctx, const real_hip_pair_params *pp, const real_hip_hit *hits1, const uint64_t *off1,
                            const uint32_t *len1, const real_hip_hit *hits2, const uint64_t *off2, const uint32_t *len2,
                            uint64_t n_pairs, int on_device, int fresh, real_hip_mapq_acc *acc);
/* real_hip_match_all of the batch against the resident text and index block with the hits kept on the device (the hit buffer
 * grows inside), then the fold: only the accumulators cross to the host (on_device 0 / 2; 1: acc is a device pointer).
 * batch->fresh governs acc[].                                                                                                 */
int real_hip_match_mapq(real_hip_ctx *ctx, const real_hip_batch *batch, real_hip_mapq_acc *acc);
/* Everything real_hip_match_pairs_singles does, and in the same call the three folds from the same device-resident lists:
 * acc_pair[] over the concordant pairs, acc1[] / acc2[] over each mate's hits.  pairs[] / singles*[] are bit for bit what
 * real_hip_match_pairs_singles gives; batch1->fresh governs all six arrays.  Pairs across index blocks are not seen, as there.
 * Placements that only the mate search finds are not candidates: they arrive as UNLISTED at the finish.                      */
int real_hip_match_pairs_mapq(real_hip_ctx *ctx, const real_hip_batch *batch1, const real_hip_batch *batch2,
                              const real_hip_pair_params *pp, const real_hip_mate_search_params *sp, real_hip_pair *pairs,
                              real_hip_single *singles1, real_hip_single *singles2, real_hip_mapq_acc *acc_pair,
                              real_hip_mapq_acc *acc1, real_hip_mapq_acc *acc2);
/* The finish: from the final records and the accumulators to one byte per read.  WHICH PLACEMENT is the rule of the mismatch
 * lists.  Single-end (real_hip_mapq): an info record of state 1 or 2 places read i; its level comes from score[i] with scores
 * on (score must then be given) and from the record's errors field with scores off; out[i] is its quality against acc[i], and
 * REAL_HIP_MAPQ_NONE for every other state.  Paired-end (real_hip_mapq_pairs): out[2i] is mate 1 and out[2i + 1] mate 2 of
 * fragment i.  A Unique pair record gives both mates the quality of acc_pair[i] at the level of `best` (of k1 + k2 with scores
 * off).  Otherwise, if singles are given (both or neither NULL; acc1 / acc2 may be NULL without them) and the pair record is
 * NoMatch, a mate whose single record is Unique takes its quality from its own accumulator at the level of its single
 * record's score / k.  Everything else gets REAL_HIP_MAPQ_NONE.  File ids play no part: the accumulators span the files.
 * on_device 0: all pointers host memory (copied), 1: all device pointers (pairs and acc 8-byte, singles 16-byte aligned).
 * n == 0 is valid.  NULL arrays with n > 0, one singles pointer without the other, more than 2^32 items:
 * REAL_HIP_E_INVALID with a message, nothing launched.  Uses the ctx's -q; needs neither text nor index.                     */
int real_hip_mapq(real_hip_ctx *ctx, const uint64_t *info, const float *score, const real_hip_mapq_acc *acc, uint64_t n,
                  int on_device, uint8_t *out);
int real_hip_mapq_pairs(real_hip_ctx *ctx, const real_hip_pair *pairs, const real_hip_single *singles1, const real_hip_single *singles2,
                        const real_hip_mapq_acc *acc_pair, const real_hip_mapq_acc *acc1, const real_hip_mapq_acc *acc2, uint64_t n,
                        int on_device, uint8_t *out /* 2 * n bytes */);
/* work of the stage, accumulated since the last reset; kernel_ms: HIP events on the ctx's stream around the kernels        */
typedef struct real_hip_mapq_stats {
    uint32_t struct_size, reserved; /* = sizeof(real_hip_mapq_stats), 0                                           */
    uint64_t folded;        /* reads and fragments folded (a list each)                                           */
    uint64_t candidates;    /* hits walked by the single folds + product cells walked by the pair folds           */
    uint64_t handed_over;   /* lists / products beyond a lane's budget: folded by a wave each                     */
    uint64_t placements;    /* placements the finish gave a quality                                               */
    uint64_t unlisted;      /* of those, the ones that were not among their accumulator's candidates              */
    uint64_t launches;      /* kernels launched                                                                   */
    double   kernel_ms;
} real_hip_mapq_stats;
int real_hip_mapq_stats_get(real_hip_ctx *ctx, real_hip_mapq_stats *out, int reset);

/* ---- gap rescue: place a mate that differs from the text by one insertion or deletion (off unless these entry points are
 * called).  Every other placement of this library is ungapped: a read with one indel shows dozens of mismatches at its true
 * position and is found nowhere.  With pairs the placed mate says where the other one must lie, and there an alignment with
 * one gap is a prefix on one diagonal plus a suffix on a neighbouring one.  The reference has no counterpart (its -g is
 * unfinished); the semantics are this project's own.  Everything is an integer and a function of reads, records
 * and text alone: nothing depends on lanes, waves, tiles or calls, and two calls on the halves of a batch give the records of
 * one call on the whole.
 * WHICH FRAGMENTS.  The records are the FINAL ones, after all genome files, as real_hip_mismatches_pairs takes them.  Fragment i
 * is ELIGIBLE in the resident genome file f (n bases) iff its pair record's state is REAL_HIP_PAIR_NOMATCH, exactly one mate's
 * single record is Unique (the ANCHOR, at a on strand inv, length La), the other mate's single record is NoMatch (the TARGET,
 * length L) and the anchor's fileid == f.  A fragment that meets the first three conditions with an anchor of another file is
 * left untouched and counted as other_file.  An eligible fragment is SKIPPED and counted if the target holds a symbol > 3, is
 * longer than REAL_HIP_MAX_PATL or shorter than 2 * min_flank + max_gap + 1, or if the anchor does not lie wholly inside
 * fragment `frag` of the resident text (no record of this library's matchers does that); its record is NoMatch.
 * WINDOW.  The target is searched on the strand opposite to the anchor's; R is the ORIENTED target: the read itself on '+', its
 * reverse complement on '-'.  [lo, hi] is the set of start positions at which an ungapped hit of the target would be CONCORDANT
 * with the anchor (the paired-end block above), in 64 bits:
 *   anchor forward  p in [max(a, a + La - L, a + min_insert - L), a + max_insert - L]
 *   anchor reverse  p in [a + La - max_insert, min(a, a + La - L, a + La - min_insert)]
 * With [fs, fe) the anchor's fragment, every start p in [max(lo - max_gap, fs), min(hi + max_gap, fe - 1)] is EXAMINED (none if
 * lo > hi).  max_insert beyond REAL_HIP_MATE_SEARCH_MAX_INSERT is REAL_HIP_E_UNSUPPORTED before anything is launched.
 * CANDIDATES.  A candidate is a triple (p, g, j) with p examined and |g| <= max_gap:
 *   g = 0            j = 0; R[0..L) on text[p..p+L); the span is L
 *   g > 0  deletion  of g text bases: min_flank <= j <= L - min_flank; R[0..j) on text[p..p+j) and R[j..L) on
 *                    text[p+j+g..p+L+g); the span is L + g
 *   g < 0  insertion of d = -g read bases: min_flank <= j <= L - min_flank - d; R[0..j) on text[p..p+j), R[j..j+d) unaligned,
 *                    R[j+d..L) on text[p+j..p+L-d); the span is L - d
 * k is the number of mismatching aligned bases, cost = cost_mismatch * k + (g != 0 ? cost_open + cost_extend * |g| : 0).  A
 * triple is a candidate iff [p, p + span) lies inside the anchor's fragment, no N bit is set in the span, k <= 15 and
 * cost <= max_cost.
 * RECORD.  best is the lexicographically smallest (cost, |g|, p, g, j): among equal costs the ungapped alignment wins, then the
 * shorter gap, then the leftmost start, then an insertion before a deletion, then the leftmost split -- the VCF
 * left-alignment of a gap inside a repeat.  second is the smallest cost among the candidates with |p - best.pos| > max_gap:
 * every other alignment of the same locus starts within max_gap of best, so they do not vote against their own locus.  state:
 * NoMatch without a candidate (every other field 0, second 0xFFFF), NonUnique if second <= cost + margin, else Unique.
 * PARAMETERS (anything else is REAL_HIP_E_INVALID with a message, nothing launched): max_gap in 1..REAL_HIP_GAP_MAX, min_flank >=
 * 1, the three costs <= 65535, max_cost <= 65534 (0xFFFF is "none"), margin <= 65535, reserved words 0.
 * real_hip_gap_rescue: where the arrays live follows the batches' on_device as for real_hip_mismatches_pairs: records and out
 * are host memory for 0 and 2, device memory for 1 (pairs 8-byte, singles and out 16-byte aligned).  fresh != 0: out is output
 * only and every record starts NoMatch; 0: in/out, only the fragments eligible in the resident file are written -- how a run
 * over several genome files fills one array.  Needs the text, not the index (REAL_HIP_E_STATE without it).  n_reads == 0 is
 * valid.  REAL_HIP_E_INVALID with a message: NULL params, records or out with n_reads > 0, a wrong struct_size, batches that
 * disagree in n_reads or on_device, more than 2^32 fragments.                                                                  */
#define REAL_HIP_GAP_MAX 16u
#define REAL_HIP_GAP_NONE 0xFFFFu   /* `second` of a record without a rival */
typedef struct real_hip_gap_params {
    uint32_t struct_size;    /* = sizeof(real_hip_gap_params)                                          */
    uint32_t max_gap;        /* longest insertion or deletion, 1..REAL_HIP_GAP_MAX                     */
    uint32_t min_flank;      /* fewest aligned bases on either side of a gap, >= 1                     */
    uint32_t cost_mismatch, cost_open, cost_extend;
    uint32_t max_cost;       /* a candidate costs at most this                                         */
    uint32_t margin;         /* NonUnique if second <= cost + margin                                   */
    uint32_t reserved[2];    /* 0                                                                      */
} real_hip_gap_params;
typedef struct real_hip_gap_place {   /* 16 bytes, 16-byte aligned on the device (one vector store) */
    uint32_t pos;            /* p: 0-based start in the text of fileid                                 */
    uint16_t frag;
    uint8_t  fileid;
    uint8_t  tag;            /* bit 0: which mate is the target (0 = mate 1); bit 4: inverted; bits 5-6: state */
    uint16_t split;          /* j                                                                      */
    int8_t   gap;            /* g: > 0 deletion, < 0 insertion                                         */
    uint8_t  k;              /* mismatching aligned bases                                              */
    uint16_t cost, second;   /* second: REAL_HIP_GAP_NONE = none                                       */
} real_hip_gap_place;
#define REAL_HIP_GAP_TARGET(tag)   ((tag) & 1u)
#define REAL_HIP_GAP_INVERTED(tag) (((tag) >> 4) & 1u)
#define REAL_HIP_GAP_STATE(tag)    (((tag) >> 5) & 3u)
int real_hip_gap_rescue(real_hip_ctx *ctx, const real_hip_pair_params *pp, const real_hip_gap_params *gp,
                        const real_hip_batch *b1, const real_hip_batch *b2, const real_hip_pair *pairs,
                        const real_hip_single *singles1, const real_hip_single *singles2, int fresh, real_hip_gap_place *out);
/* Host only: the CIGAR of a record of a read of `len` bases -- "100M", "40M2D60M", "40M3I57M" -- in forward-text coordinates
 * (the ORIENTED read is what is aligned, so nothing is reversed).  Returns the string's length; REAL_HIP_E_INVALID for NULL
 * arguments, a NoMatch record or a record that does not fit the length; REAL_HIP_E_OVERFLOW when cap is too small.       */
int real_hip_gap_cigar(const real_hip_gap_place *g, uint32_t len, char *buf, size_t cap);
/* work of the stage, accumulated since the last reset.  Every counter but the last two is a function of the inputs.       */
typedef struct real_hip_gap_stats {
    uint32_t struct_size, reserved; /* = sizeof(real_hip_gap_stats), 0                                 */
    uint64_t fragments;      /* fragments handed in                                                    */
    uint64_t eligible;       /* eligible in the resident file, the skipped ones included               */
    uint64_t other_file;     /* anchor in another file                                                 */
    uint64_t skipped;
    uint64_t positions;      /* sum of the numbers of examined starts                                  */
    uint64_t placed;         /* records that are not NoMatch                                           */
    uint64_t unique;
    uint64_t gapped;         /* placed with g != 0                                                     */
    uint64_t launches;       /* kernels launched                                                       */
    double   kernel_ms;      /* HIP events on the ctx's stream around the kernels                      */
} real_hip_gap_stats;
int real_hip_gap_stats_get(real_hip_ctx *ctx, real_hip_gap_stats *out, int reset);

/* ---- anchored gap placement: place a SINGLE read that differs from the text by one insertion or deletion (off unless these
 * entry points are called).  Without a mate nothing says where to look; the matcher itself does: an alignment with one gap is
 * a prefix on one diagonal plus a suffix on a neighbouring one, so whenever 2 A + max_gap <= L either the first A or the last A
 * bases of the read lie wholly on one diagonal, and matchAll finds that sub-read ungapped.  Those hits are the ANCHORS; around
 * each the search is the gap rescue's, in a window of 2 * max_gap + 1 starts.  The semantics are this project's own (DESIGN.md
 * 7k): all integers, a function of reads, records, hit lists and text alone -- nothing depends on lanes, waves, the order of a
 * hit list or the split of a batch into calls.  G = max_gap, m = min_flank; the costs, max_cost and margin are those of
 * real_hip_gap_params with its parameter checks; A = anchor_len in 1..REAL_HIP_MAX_PATL and max_anchors in
 * 1..REAL_HIP_GAP_ANCHORS_MAX are the fields of struct real_hip_gap_anchor_params; its reserved words are 0.
 * SUB-READ BATCH S(b, A).  2 n reads of uniform length A: sub-read 2i holds bases and qualities [0, A) of read i (the prefix,
 * e = 0), sub-read 2i + 1 holds [L_i - A, L_i) (the suffix, e = 1).  The anchor hits of read i are the real_hip_hit entries of
 * these two sub-reads in one hit list with 2 n + 1 offsets; real_hip_match_gapped takes exactly what real_hip_match_all returns
 * for S(b, A) under the context's current match parameters.
 * WHICH READS.  Read i is ELIGIBLE iff info == NULL or the state of info[i] is NoMatch (the state of a fresh record); info holds
 * the FINAL records of the run.  An eligible read is SKIPPED and counted if it holds a symbol > 3, or L > REAL_HIP_MAX_PATL, or
 * L < 2 m + G + 1, or L < A.  An eligible read that is not skipped is CROWDED and counted if its two sub-reads have more than
 * max_anchors hits together, UNANCHORED and counted if they have none; every other one is SEARCHED.  Skipped, crowded and
 * unanchored reads give NoMatch.
 * ANCHOR DIAGONAL.  A hit of sub-read 2i + e at q, strand v (inverted), fragment f = [fs, fe) orients the read as v says: R is
 * the read for v = 0, its reverse complement for v = 1.  It names the start c of R's ungapped diagonal, in 64 bits: c = q if
 * e == v (the sub-read is the head of R), c = q - (L - A) otherwise (it is the tail of R; c may be negative).  A hit with
 * f >= n_frag, q < fs or q + A > fe is counted as invalid and ignored; no byte outside the arrays is read for it.  `anchors`
 * counts the valid hits of the searched reads, `invalid_anchors` their other hits.
 * EXAMINED STARTS.  For each valid anchor the starts (v, p) with p in [max(c - G, fs), min(c + G, fe - 1)].  `positions` is the
 * sum of these window sizes over the valid anchors: overlapping windows count twice.
 * CANDIDATES.  A candidate is (v, p, g, j) with (v, p) examined; the rest is the CANDIDATES paragraph of the gap rescue word for
 * word: the geometry of g = 0, g > 0 and g < 0, k <= 15, cost <= max_cost, no N bit in the span, the span inside fragment f.
 * The candidates of a read are a SET: an alignment two anchors reach counts once.
 * RECORD.  best is the smallest (cost, |g|, p, v, g, j); second is the smallest cost among the candidates with v != best.v or
 * |p - best.pos| > G.  State and fields as in the gap rescue; tag bit 0 (target) is 0, bit 4 is v, bits 5-6 the state; fileid
 * is the resident file.  placed / unique / gapped count these records, before any fold.
 * FOLD (fresh == 0).  A searched read with a candidate gets out[i] = M(out[i], r); every other record is untouched.  NoMatch is
 * M's neutral element.  Otherwise the winner w is the smaller by (cost, |g|, fileid, pos, v, g, j) and l the other; they are the
 * SAME LOCUS iff fileid and v are equal and |w.pos - l.pos| <= G; the result is w with second = min(w.second, l.second, same
 * locus ? NONE : l.cost) and the state recomputed with the call's margin.  Across genome files M is exact, commutative and
 * associative (loci of different files are never the same).  Across index blocks of ONE file it is CONSERVATIVE: a rival of the
 * loser's call that lies at the winner's locus still counts in l.second, so a record may turn NonUnique; it never turns
 * wrongly Unique.  fresh != 0: every record starts NoMatch and all are written.
 * COVERAGE (a remark).  If 2 A + G <= L, every candidate of cost <= max_cost whose wholly aligned sub-read is found by the
 * matcher is examined.  Shorter reads are searched with partial coverage.
 * real_hip_gap_anchor_hits: the stage on hit lists the caller holds.  Where the arrays live follows batch->on_device as for
 * real_hip_gap_rescue: info, hits, hit_offsets and out are host memory for 0 and 2, device memory for 1 (info and hit_offsets
 * 8-byte, hits and out 16-byte aligned).  Needs the text, not the index (REAL_HIP_E_STATE without it).  hit_offsets start at 0;
 * host offsets must not run backwards, device offsets are clamped.  n_reads == 0 is valid.
 * real_hip_match_gapped: the composite.  Needs the text and a resident index block (REAL_HIP_E_STATE otherwise).  On the device
 * it selects the eligible, not skipped reads, writes their sub-reads, runs the library's matchAll on them with hits and offsets
 * left on the device, then the stage: its records equal real_hip_gap_anchor_hits on real_hip_match_all(S(b, A)).
 * REAL_HIP_E_INVALID with a message, nothing launched: NULL params, batch, hit_offsets or out with n_reads > 0, NULL hits with
 * hits in the lists, a wrong struct_size, a parameter out of range, misaligned device arrays, more than 2^32 reads.        */
#define REAL_HIP_GAP_ANCHORS_MAX 64u
typedef struct real_hip_gap_anchor_params {
    uint32_t struct_size;    /* = sizeof(real_hip_gap_anchor_params)                                   */
    uint32_t anchor_len;     /* A: bases of the prefix and of the suffix sub-read, 1..REAL_HIP_MAX_PATL */
    uint32_t max_anchors;    /* a read with more hits of its two sub-reads is crowded, 1..REAL_HIP_GAP_ANCHORS_MAX */
    uint32_t reserved[2];    /* 0                                                                      */
} real_hip_gap_anchor_params;
int real_hip_gap_anchor_hits(real_hip_ctx *ctx, const real_hip_gap_params *gp, const real_hip_gap_anchor_params *ap, const real_hip_batch *batch,
                             const uint64_t *info /* nullable */, const real_hip_hit *hits, const uint64_t *hit_offsets /* 2 n + 1 */, int fresh,
                             real_hip_gap_place *out);
int real_hip_match_gapped(real_hip_ctx *ctx, const real_hip_gap_params *gp, const real_hip_gap_anchor_params *ap, const real_hip_batch *batch,
                          const uint64_t *info /* nullable */, int fresh, real_hip_gap_place *out);
/* work of the stage, accumulated since the last reset.  Every counter but the last two is a function of the inputs; launches
 * and kernel_ms cover the stage's own kernels, not the matcher's.                                                          */
typedef struct real_hip_gap_anchor_stats {
    uint32_t struct_size, reserved; /* = sizeof(real_hip_gap_anchor_stats), 0                          */
    uint64_t reads;          /* reads handed in                                                        */
    uint64_t eligible;       /* the skipped ones included                                              */
    uint64_t skipped;
    uint64_t crowded;
    uint64_t unanchored;
    uint64_t anchors;        /* valid hits of the searched reads                                       */
    uint64_t invalid_anchors;
    uint64_t positions;      /* sum of the numbers of examined starts                                  */
    uint64_t placed;         /* records of the calls that are not NoMatch                              */
    uint64_t unique;
    uint64_t gapped;         /* placed with g != 0                                                     */
    uint64_t launches;       /* kernels launched                                                       */
    double   kernel_ms;      /* HIP events on the ctx's stream around the kernels                      */
} real_hip_gap_anchor_stats;
int real_hip_gap_anchor_stats_get(real_hip_ctx *ctx, real_hip_gap_anchor_stats *out, int reset);

/* ---- gapped mismatch lists: where a gap-rescued mate differs from the resident text, and which text bases its deletion skips
 * -- what CIGAR, NM and MD of such a mate's SAM line are written from.  ORIENTED read and the resident text (n
 * bases, file id f) are those of the block "mismatch lists".
 * List i belongs to fragment i's gap record.  The read is the record's target mate: REAL_HIP_GAP_TARGET(tag) picks b1 (0) or
 * b2 (1); it is oriented by REAL_HIP_GAP_INVERTED(tag).  With L the read's length, p = pos, j = split, g = gap, d = max(-g, 0)
 * and span = L + g, in this order:
 *   1. a record whose state is not Unique gets an empty list;
 *   2. a Unique record of another file id than f gets an empty list and is counted as other_file;
 *   3. a Unique record of file f that does not FIT gets an empty list and is counted as invalid, and no byte of text or read
 *      outside their arrays is read for it.  It does not fit when |g| > REAL_HIP_GAP_MAX; or g != 0 and not (1 <= j and
 *      j + d <= L - 1); or g == 0 and j != 0; or p + span > n; or L > REAL_HIP_MAX_PATL.  The geometry is the whole contract:
 *      no min_flank is checked;
 *   4. otherwise the list holds one entry per LISTED text offset t in 0 .. span - 1, ascending; off = t, ref is the text's
 *      base at p + t, or 4 where the text's N bit is set there.
 *      DELETED position (g > 0 and j <= t < j + g): always listed, base = REAL_HIP_MISMATCH_DELETED.
 *      ALIGNED position: oriented read offset t aligns with text offset t when t < j; read offset t - g aligns with text offset
 *      t when t >= j + max(g, 0).  With an insertion the read offsets j .. j + d - 1 align with nothing.  An aligned position is
 *      listed by the rule of the ungapped lists: where the N bit is set (ref = 4, whatever the read shows) and, elsewhere,
 *      where the oriented base differs from the text; base is the oriented base.
 *      For g == 0 the list is what real_hip_mismatches gives for that placement.
 * Everything else is real_hip_mismatches_pairs' rule word for word: gaps, out and mm_offsets are host memory for on_device 0 and
 * 2, device memory for 1 (gaps 16-byte, out 4-byte aligned); n_out is host memory and always receives the total; when the total
 * exceeds cap the call returns REAL_HIP_E_OVERFLOW and writes nothing to out (mm_offsets, n_reads + 1 entries from 0, is still
 * written); n_reads == 0 is valid; REAL_HIP_E_STATE without a text; REAL_HIP_E_INVALID with a message, nothing launched: a NULL
 * mm_offsets or n_out, a NULL out with cap > 0, NULL gaps with n_reads > 0, batches that disagree in n_reads or on_device, more
 * than 2^32 fragments.  The output is a function of records, reads and text alone, and two calls on the halves of a batch give
 * the lists of one call on the whole, up to rebasing the offsets.                                                             */
#define REAL_HIP_MISMATCH_DELETED 4u   /* real_hip_mismatch::base of a text position the read's deletion skips */
int real_hip_mismatches_gapped(real_hip_ctx *ctx, const real_hip_batch *b1, const real_hip_batch *b2,
                               const real_hip_gap_place *gaps,
                               real_hip_mismatch *out, uint64_t cap, uint64_t *n_out,
                               uint64_t *mm_offsets /* n_reads + 1 */);
/* work of the gapped lists, accumulated since the last reset.  disagree is 0 for records of real_hip_gap_rescue: it admits no N
 * in a span, and its k is the number of differing aligned bases.                                                               */
typedef struct real_hip_gapped_list_stats {
    uint32_t struct_size, reserved; /* = sizeof(real_hip_gapped_list_stats), 0                          */
    uint64_t fragments;      /* lists asked for                                                        */
    uint64_t placed;         /* Unique records of this file that fit: placements walked                */
    uint64_t other_file;     /* Unique records of another file id                                      */
    uint64_t invalid;        /* Unique records of this file that do not fit                            */
    uint64_t aligned_bases;  /* sum of L - d over the placed records                                   */
    uint64_t mismatches;     /* entries on aligned positions, written or counted by a call that overflowed */
    uint64_t deleted;        /* entries on deleted positions: sum of max(g, 0) over the placed records */
    uint64_t inserted;       /* sum of d over the placed records                                       */
    uint64_t on_n;           /* entries with ref = 4, aligned or deleted                               */
    uint64_t disagree;       /* placed records whose number of aligned entries is not the record's k   */
    uint64_t launches;       /* kernels launched (the scan counts one)                                 */
    double   kernel_ms;      /* HIP events on the ctx's stream around count, scan and emit             */
} real_hip_gapped_list_stats;
int real_hip_gapped_list_stats_get(real_hip_ctx *ctx, real_hip_gapped_list_stats *out, int reset);

/* ---- indel calls: what the gap-rescued mates add up to over one genome file -- which insertions and deletions they show, how
 * many mates show each, and with which genotype (off unless these entry points are called).  The reference has no caller and
 * no finished gapped mode; the semantics are this project's own.  Everything is an integer.
 * PROTOCOL.  The stage sits on a FINISHED pileup of the resident text (n bases, file id f), as the variant calls do, and uses
 * that pileup's depth[] and its min_qual.  indel_begin (a second begin starts again), any number of indel_add, indel_finish
 * (synchronises; may be called again with other thresholds, it then only re-reads the grouped events), indel_events /
 * indel_calls any number of times after a finish (the capacity protocol of real_hip_pileup_sites: *n_out always receives the
 * count, REAL_HIP_E_OVERFLOW writes nothing), indel_end.  real_hip_pileup_end and a new real_hip_pileup_begin end the stage as
 * well.  REAL_HIP_E_INVALID with a message, nothing launched: calls out of turn (begin without a finished pileup, add without
 * begin or after finish, finish without begin, events / calls before finish), a text replaced by one of another n_bases or
 * file id, NULL batches, NULL gaps with n_reads > 0, batches that disagree in n_reads or on_device, a wrong struct_size, more
 * than 2^32 fragments in one call.  gaps and the output lists live where real_hip_mismatches_gapped's live for the batches'
 * on_device: gaps are host memory for 0 and 2, device memory (16-byte aligned) for 1; the lists go to host memory unless the
 * list call's own on_device says otherwise.
 * WHICH RECORDS.  Fragment i's record, its target mate REAL_HIP_GAP_TARGET(tag), its orientation and the ORIENTED read R are
 * those of the block "gapped mismatch lists", word for word.  In this order: 1. a record that is not Unique is skipped; 2. a
 * Unique record of another file id than f is skipped and counted as other_file; 3. a Unique record of file f that does not FIT
 * by that block's rule, or whose frag is not a fragment of the text, or whose span [p, p + L + g) does not lie inside fragment
 * frag = [fs, fe), is counted as invalid, and nothing outside the arrays is read for it; 4. a fitting record with g == 0 is
 * counted as ungapped and gives no event.
 * EVENT.  A fitting record with g != 0, p = pos, j = split and d = max(-g, 0) gives one event (x, g, S) with x = p + j: for
 * g > 0 the text bases [x, x + g) are deleted and S is empty; for g < 0 S = R[j .. j + d) is inserted in front of text position
 * x.  The ANCHOR is text position x - 1 (>= fs, because j >= 1).  If the text's N bit is set at the anchor or anywhere in
 * [x, x + max(g, 0)), the event is dropped and counted as on_n.
 * QUALITY.  q is the minimum of the quality bytes of the oriented read offsets j - 1, j + d and, for an insertion,
 * j .. j + d - 1 (the reverse strand indexes L - 1 - i, as the pileup does; a batch without qualities counts as 30).  If
 * q < min_qual of the pileup the event is dropped and counted as low_qual.
 * LEFT-NORMALISATION against the text, so that two reads name one event whatever the rescue's split was.  At most
 * REAL_HIP_INDEL_SHIFT_MAX times, while x - 1 > fs, the N bits at x - 1 and x - 2 are clear, and
 *   deletion:  text[x - 1] == text[x + g - 1]                       then x -= 1
 *   insertion: text[x - 1] == S[d - 1]                              then S = text[x - 1] . S[0 .. d - 1), x -= 1
 * An event that stops only because of the cap is counted as shift_capped.  (The number of shifts is the length of the run,
 * ending at x, of positions i with T'[i] == T'[i + |g|], T' the text for a deletion and text[0, x) . S for an insertion.)
 * GROUPS.  Two events are equal iff (x, g, S) are equal after normalisation; S is packed 2 bits a base, the first base lowest,
 * in a u32 (REAL_HIP_GAP_MAX bases fill it exactly; 0 for a deletion).  Per distinct event: alt_n, the supporting mates;
 * alt_fwd, those whose record is not inverted; qsum, the sum of their q; ref_n = min(u[x - 1], u[x]) with u = depth - gdepth
 * of the finished pileup: the ungapped placements alone, whether or not gapped ones were piled up beside them ("gapped
 * placements in the pileup and the calls"), so no mate counts on both sides.  All counters are u32.  The event list is in
 * ascending (x, g, S), g compared as a signed number.
 * GENOTYPE, in phred units: PL(0/0) = qsum, PL(0/1) = REAL_HIP_CALL_HET * (ref_n + alt_n) + REAL_HIP_INDEL_PRIOR_HET,
 * PL(1/1) = REAL_HIP_INDEL_REF_Q * ref_n + REAL_HIP_INDEL_PRIOR_HOM (the SNP priors plus 10: indels are about ten times
 * rarer).  The best genotype is the first of minimal PL in the order 0/0, 0/1, 1/1; QUAL = PL(0/0) - PL(best) (as u32; beyond
 * 2^32 - 1 it counts as that), GQ = min(99, smallest other PL - PL(best)).  A CALL is an event with best != 0/0, QUAL >=
 * min_call_qual, alt_n >= min_alt and ref_n + alt_n >= min_depth.  The call list is the calls in the events' order.
 * Nothing depends on lanes, waves, the order of the records, the split into add calls or on_device: two adds give what one add
 * on the concatenation gives.                                                                                                 */
#define REAL_HIP_INDEL_SHIFT_MAX 256u
#define REAL_HIP_INDEL_REF_Q     30u /* phred cost of a read without the indel under a homozygous indel                   */
#define REAL_HIP_INDEL_PRIOR_HET 40u
#define REAL_HIP_INDEL_PRIOR_HOM 43u
typedef struct real_hip_indel_params {
    uint32_t struct_size;   /* = sizeof(real_hip_indel_params)                                        */
    uint32_t min_call_qual; /* a call needs QUAL >= this                                              */
    uint32_t min_alt;       /* and alt_n >= this                                                      */
    uint32_t min_depth;     /* and ref_n + alt_n >= this                                              */
} real_hip_indel_params;
typedef struct real_hip_indel {   /* 32 bytes; the records of the event list and of the call list */
    uint32_t pos;           /* the anchor x - 1, 0-based position in the text                         */
    uint32_t ref_n;
    uint32_t alt_n;
    uint32_t alt_fwd;
    uint32_t qsum;
    uint32_t qual;          /* QUAL                                                                   */
    uint32_t seq;           /* the packed S; 0 for a deletion                                         */
    int8_t   gap;           /* g: > 0 deletion, < 0 insertion                                         */
    uint8_t  gt;            /* 0: no call under the last finish's thresholds, 1: 0/1, 2: 1/1          */
    uint8_t  gq;            /* GQ                                                                     */
    uint8_t  ref;           /* the text's base 0..3 at the anchor                                     */
} real_hip_indel;
int real_hip_indel_begin(real_hip_ctx *ctx);
/* batch1 and batch2 must agree in n_reads and on_device; gaps: what real_hip_gap_rescue wrote for them */
int real_hip_indel_add(real_hip_ctx *ctx, const real_hip_batch *b1, const real_hip_batch *b2, const real_hip_gap_place *gaps);
int real_hip_indel_finish(real_hip_ctx *ctx, const real_hip_indel_params *p, uint64_t *n_events, uint64_t *n_calls);
int real_hip_indel_events(real_hip_ctx *ctx, real_hip_indel *out, uint64_t cap, uint64_t *n_out, int on_device);
int real_hip_indel_calls(real_hip_ctx *ctx, real_hip_indel *out, uint64_t cap, uint64_t *n_out, int on_device);
int real_hip_indel_end(real_hip_ctx *ctx);
/* work of the stage.  fragments .. shift_capped, launches and kernel_ms are accumulated since the last reset; distinct ..
 * insertions are those of the last finish (0 from begin until then)                                                       */
typedef struct real_hip_indel_stats {
    uint32_t struct_size, reserved; /* = sizeof(real_hip_indel_stats), 0                              */
    uint64_t fragments;      /* fragments handed in                                                    */
    uint64_t placed;         /* Unique records of this file that fit                                   */
    uint64_t other_file;     /* Unique records of another file id                                      */
    uint64_t invalid;        /* Unique records of this file that do not fit                            */
    uint64_t ungapped;       /* placed with g == 0                                                     */
    uint64_t events;         /* increments of alt_n                                                    */
    uint64_t on_n;           /* events dropped on an N of the text                                     */
    uint64_t low_qual;       /* events that min_qual dropped                                           */
    uint64_t shifted;        /* events the normalisation moved by at least one base                    */
    uint64_t shift_capped;   /* events that stopped only at REAL_HIP_INDEL_SHIFT_MAX                   */
    uint64_t distinct;       /* distinct events                                                        */
    uint64_t calls;
    uint64_t het;
    uint64_t hom;
    uint64_t deletions;      /* calls with g > 0                                                       */
    uint64_t insertions;     /* calls with g < 0                                                       */
    uint64_t launches;       /* kernels launched (a sort or a scan counts one)                         */
    double   kernel_ms;      /* HIP events on the ctx's stream around the kernels of add and finish    */
} real_hip_indel_stats;
int real_hip_indel_stats_get(real_hip_ctx *ctx, real_hip_indel_stats *out, int reset);

/* ---- gapped placements in the pileup and the calls: the placements with one insertion or deletion (the records of
 * real_hip_gap_rescue and real_hip_match_gapped) in the per-position accounting, so that the depth does not dip and a site is
 * not genotyped short of reads where the reads carry an indel (off unless these entry points are called).
 * Everything is an integer sum.
 * WHICH RECORDS.  Fragment i's record, its target mate REAL_HIP_GAP_TARGET(tag), its orientation REAL_HIP_GAP_INVERTED(tag) and
 * the ORIENTED read R are those of the block "gapped mismatch lists", word for word.  In this order: 1. a record that is not
 * Unique is skipped; 2. a Unique record of another file id than f is skipped and counted as other_file; 3. a Unique record of
 * file f that does not FIT by that block's rule (p + span <= n, L <= REAL_HIP_MAX_PATL, the split inside the read, |g| <=
 * REAL_HIP_GAP_MAX) is counted as invalid, and no byte of read or text is touched for it.  Single-end records of
 * real_hip_match_gapped are passed with the batch given as both mates.
 * WHAT A FITTING RECORD ADDS.  With p = pos, j = split, g = gap and d = max(-g, 0), the ALIGNED text positions are
 * [p, p + L - d) for g <= 0 and [p, p + j) and [p + j + g, p + L + g) for g > 0: a deleted position is not covered, the read
 * shows no base there.  Text offset t < j pairs with oriented read offset t; text offset t >= j + max(g, 0) pairs with oriented
 * read offset t - g; the read offsets j .. j + d - 1 of an insertion pair with nothing.
 *   depth[x] += 1 on the aligned positions, in the pileup's difference array (a deletion costs four atomics, anything else
 *     two), and the same increments go into a second difference array of n + 1 u32, allocated and zeroed by the first
 *     add_gapped of a pileup (REAL_HIP_E_NOMEM with a message when that fails; the pileup stays valid) and scanned by the
 *     pileup's finish into gdepth[x], the gapped placements' share of depth[x];
 *   alt[x][b] += 1 by the pileup's rule on every aligned pair (x, r): the oriented base R[r] = b differs from ref[x], the
 *     quality byte of oriented offset r (on the reverse strand the byte at index L - 1 - r; a batch without qualities counts
 *     as 30) is >= min_qual, and the text's N bit at x is clear -- the quality is tested first, then the N bit;
 *   call_add_gapped adds the evidence of the same aligned pairs over the sites of the finished pileup by the rule of "variant
 *     calls"; cnt[s][b] == site.alt[b] for b != ref keeps holding when the same records went to both.
 * real_hip_pileup_depth returns the total; real_hip_pileup_depth_gapped returns gdepth (zeros when no gapped add was made;
 * the window checks are real_hip_pileup_depth's).  The indel calls take ref_n from depth - gdepth: they do not move.
 * PROTOCOL AND ERRORS are the pileup's and the calls' own: pileup_add_gapped between the pileup's begin and finish, in any
 * order with add / add_pairs; call_add_gapped between call_begin and call_finish, in any order with call_add / call_add_pairs.
 * REAL_HIP_E_INVALID with a message, nothing launched: pileup_add_gapped without a begin or after finish, call_add_gapped
 * without call_begin or before the pileup's finish, a text replaced by one of another n_bases or file id, NULL batches, NULL
 * gaps with n_reads > 0, batches that disagree in n_reads or on_device, more than 2^32 fragments in one call.  n_reads == 0 is
 * valid.  gaps live where real_hip_mismatches_gapped's live: host memory for on_device 0 and 2, device memory, 16-byte aligned,
 * for 1.  real_hip_pileup_end, a new real_hip_pileup_begin and real_hip_destroy release the second array.  Nothing depends on
 * lanes, waves, the order of the records, the split into add calls or on_device: two adds give what one add on the
 * concatenation gives.
 * STATISTICS.  The counters of real_hip_pileup_stats and real_hip_call_stats that add / add_pairs count keep their meaning
 * (reads .. n_dropped, site_bases, low_qual: ungapped records only); covered, sites and max_depth are read from the arrays, so
 * they see everything.  The sum of depth[] equals real_hip_pileup_stats::bases + real_hip_pileup_gapped_stats::aligned_bases.  */
int real_hip_pileup_add_gapped(real_hip_ctx *ctx, const real_hip_batch *b1, const real_hip_batch *b2, const real_hip_gap_place *gaps);
int real_hip_call_add_gapped(real_hip_ctx *ctx, const real_hip_batch *b1, const real_hip_batch *b2, const real_hip_gap_place *gaps);
/* gdepth[first .. first + count) into depth (host memory, or device memory if on_device); after finish */
int real_hip_pileup_depth_gapped(real_hip_ctx *ctx, uint64_t first, uint64_t count, uint32_t *depth, int on_device);
/* work of the stage, accumulated since the last reset.  records .. n_dropped are the pileup leg's (real_hip_pileup_add_gapped),
 * site_bases and site_low_qual the call leg's (real_hip_call_add_gapped); launches and kernel_ms are those of both.          */
typedef struct real_hip_pileup_gapped_stats {
    uint32_t struct_size, reserved; /* = sizeof(real_hip_pileup_gapped_stats), 0                       */
    uint64_t records;        /* records handed to real_hip_pileup_add_gapped                           */
    uint64_t placed;         /* Unique records of this file that fit: placements piled up              */
    uint64_t other_file;     /* Unique records of another file id                                      */
    uint64_t invalid;        /* Unique records of this file that do not fit                            */
    uint64_t ungapped;       /* placed with g == 0                                                     */
    uint64_t aligned_bases;  /* sum of L - d over the placed records = their share of the sum of depth[] */
    uint64_t deleted;        /* sum of max(g, 0) over the placed records                               */
    uint64_t inserted;       /* sum of d over the placed records                                       */
    uint64_t mismatches;     /* increments of alt                                                      */
    uint64_t low_qual;       /* mismatches that min_qual dropped                                       */
    uint64_t n_dropped;      /* mismatches of sufficient quality on an N of the text                   */
    uint64_t site_bases;     /* increments of cnt                                                      */
    uint64_t site_low_qual;  /* bases on a site that min_qual dropped                                  */
    uint64_t launches;       /* kernels launched                                                       */
    double   kernel_ms;      /* HIP events on the ctx's stream around the kernels of both legs         */
} real_hip_pileup_gapped_stats;
int real_hip_pileup_gapped_stats_get(real_hip_ctx *ctx, real_hip_pileup_gapped_stats *out, int reset);

/* ---- multi-GPU: one process per GPU, reads sharded contiguously over the ranks, the index replicated.
 * The path has ONE collective: the shards' results to the root, over RCCL (xGMI point-to-point links) -- a
 * concatenation in rank order, nothing is reduced because no read is seen by two ranks.  The reference is a single
 * process; what this replaces is the hand-over of results from its OpenMP threads to the output loop
 * (uniqueinfo[] shared by the threads, matchUniqueImplementation.cpp:1268-1295; the per-block hit emission of
 * matchAllImplementation.cpp:451-535).  Bootstrap: rank 0 calls real_hip_comm_id and hands the 128 bytes to the other
 * ranks by the launcher's own means (MPI_Bcast, a file, the rendezvous store); every rank then calls
 * real_hip_comm_init on its ctx.  All array arguments are DEVICE pointers of the ctx's device; the receive arrays
 * matter on the root only.  Counts travel first: every rank learns every rank's sizes, the root's capacities, which
 * receive arrays the root was given, and whether a rank found something wrong on its own side (a null send array, a
 * scratch buffer it could not reserve).  Every decision to give up is taken from those exchanged tuples alone -- a too
 * small receive array is REAL_HIP_E_OVERFLOW on ALL ranks (with the needed sizes in *n_..._all), null receive arrays on
 * the root or a failed peer are the same error on ALL ranks -- and is taken before any rank posts a send or a receive:
 * nobody is left waiting for a root that has returned.  Then the payload.  `root` must be the same valid rank everywhere.
 * A single process that drives several GPUs through several ctx (real -gpus N) needs none of this: its calls write
 * the shards' results into the caller's host arrays directly.                                                       */
#define REAL_HIP_COMM_ID_BYTES 128
int real_hip_comm_id(uint8_t id[REAL_HIP_COMM_ID_BYTES]);
int real_hip_comm_init(real_hip_ctx *ctx, const uint8_t id[REAL_HIP_COMM_ID_BYTES], int rank, int n_ranks);
int real_hip_comm_destroy(real_hip_ctx *ctx);
/* matchUnique: info_all / score_all (root) = the shards' records in rank order; score may be NULL iff !scores      */
int real_hip_gather_records(real_hip_ctx *ctx, int root, const uint64_t *info, const float *score, uint64_t n_local,
                            uint64_t *info_all, float *score_all, uint64_t cap_all, uint64_t *n_all);
/* matchAll: the shards' unified hit lists as real_hip_match_all returned them (hit_offsets: n_local + 1 entries);
 * on the root hits_all holds all hits with .read rebased to the whole batch and offsets_all (n_reads_all + 1) the
 * rebased offsets                                                                                                   */
int real_hip_gather_hits(real_hip_ctx *ctx, int root, const real_hip_hit *hits, const uint64_t *hit_offsets, uint64_t n_local,
                         uint64_t n_hits_local, real_hip_hit *hits_all, uint64_t cap_hits, uint64_t *offsets_all, uint64_t cap_reads,
                         uint64_t *n_reads_all, uint64_t *n_hits_all);

/* ---- read ingestion on the device: FASTA / FASTQ text -> the arrays of a batch.
 * Replaces FastQReader / FastAReader::getNextPatternUnlocked (FastQReader.hpp:130-180,
 * FastAReader.hpp:107-138), Pattern::computeMapped (Pattern.hpp:105-128, acgtnMap.hpp:39-50) and the
 * quality offset subtraction (FastQReader.hpp:165-173) for text in canonical form: whole records, every
 * field (id, sequence, '+', quality) on one line; "\r\n" accepted.  Anything else -- wrapped sequences,
 * white space inside a field, a chunk that ends inside a record -- is refused with
 * REAL_HIP_E_UNSUPPORTED and left to the caller's reader.  text: n_bytes < 4 GiB, host memory
 * (copied) or device memory (text_on_device).  The returned arrays are device memory owned by ctx,
 * valid until the next real_hip_parse_reads on it; id_start/id_len locate each record's id inside
 * the text (behind its '@' / '>').                                                            */
typedef struct real_hip_parsed {
    uint32_t        struct_size;
    uint32_t        max_patl;    /* longest read of the chunk                              */
    uint64_t        n_reads;
    uint64_t        n_symbols;   /* = offsets[n_reads]                                     */
    const uint8_t  *bases;       /* mapped symbols 0..4, concatenated                      */
    const uint8_t  *qual;        /* quality character - offset; NULL for FASTA             */
    const uint64_t *offsets;     /* n_reads + 1                                            */
    const uint32_t *id_start;    /* n_reads                                                */
    const uint32_t *id_len;      /* n_reads                                                */
} real_hip_parsed;
int real_hip_parse_reads(real_hip_ctx *ctx, const char *text, uint64_t n_bytes, int text_on_device,
                         int fastq, int quality_offset, real_hip_parsed *out);
/* copy of a device array the library returned (the spans of real_hip_parsed: what the output formatter needs
 * beside the records) to host memory; synchronous                                                          */
int real_hip_download(real_hip_ctx *ctx, const void *device_ptr, void *host_ptr, size_t bytes);

/* ---- work counters: accumulated since the last reset ---------- */
typedef struct real_hip_counters {
    uint64_t reads;       /* R  reads matched (not skipped)                           */
    uint64_t lookups;     /* L  ::match calls (12 per read, 7 with the uni0 early-out) */
    uint64_t probes;      /* P  index entries examined inside the buckets             */
    uint64_t candidates;  /* C  entries of the reference's equal range                */
    uint64_t seedpass;    /* S  candidates with seedk <= seedkmax                     */
    uint64_t hits;        /* H  updater::update calls                                 */
    uint64_t verified;    /* distinct (read,strand,pos) actually verified on text     */
    uint64_t handed_over; /* reads (among R) the first pass of the lane matcher did not finish itself: matched by its second
                             pass (many locations, long equal ranges) or by the wave-per-read kernel */
} real_hip_counters;
int real_hip_counters_get(real_hip_ctx *ctx, real_hip_counters *out, int reset);

/* ---- timing: HIP events recorded on the ctx's own stream around every kernel
 * of the path; times are accumulated per kernel since the last reset.         */
enum { REAL_HIP_K_MATCH_UNIQUE = 0, REAL_HIP_K_MATCH_ALL = 1, REAL_HIP_K_ALL_SORT = 2, REAL_HIP_K_INDEX = 3,
       REAL_HIP_K_MATCH_REPEAT = 4, /* second pass over the repeat-rich reads the matcher hands over (scores on) */
       REAL_HIP_K_PARSE = 5,        /* real_hip_parse_reads                                                      */
       REAL_HIP_K_PAIR = 6,         /* paired-end join, lane per fragment                                        */
       REAL_HIP_K_PAIR_WAVE = 7,    /* paired-end join, wave per fragment (the fragments the lanes handed over)  */
       REAL_HIP_K_COUNT = 8 };
int real_hip_kernel_time(real_hip_ctx *ctx, int which, double *total_ms, uint64_t *launches, int reset);
int real_hip_timing_enable(real_hip_ctx *ctx, int on);

#ifdef __cplusplus
}
#endif
#endif
