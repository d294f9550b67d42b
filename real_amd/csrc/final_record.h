// final_record.h -- what a final record says of its read: the info word of a single-end read, the real_hip_pair of a fragment,
// the real_hip_single of a mate (include/real_hip.h).  The one decoder of the stages that consume these records: read_walk.h's
// placed_read (pileup.hip, snp_call.hip, mismatch_list.hip) places a read on the text with it, duplicates.hip and
// insert_hist.hip read their fragment's fields through it.
// No HIP in here: libreal_hip.so's translation units get it through read_walk.h / stage_common.h, real_amd/host/host_selftest.cpp
// compiles it with the host compiler and checks it against records written through the public structs (tests/test_host_cpp.py).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define RH_HD __host__ __device__
#else
#define RH_HD
#endif

#include "real_hip.h"

// the info word (UniqueMatchInfo): state:3 | frag:16 | errors:4 | file id:6 | position:35.  Literals, because kernel_common.h
// is HIP: read_walk.h ties them to ST_SHIFT, ER_SHIFT, FI_SHIFT, POS_MASK and the state values
#define RH_INFO_ST_SHIFT 61
#define RH_INFO_ER_SHIFT 41
#define RH_INFO_FI_SHIFT 35
#define RH_INFO_POS_MASK ((1ull << 35) - 1)
#define RH_INFO_STRAIGHT 1u
#define RH_INFO_REVERSE 2u

// The kernels read a real_hip_pair as five 8-byte words, each as two dwords {x, y} (little endian): word 2 = {pos1, pos2},
// word 4 (the tail) = {frag:16 | fileid:8 | k1:8, k2:8 | inverted1:8 | state:8 | reserved:8}; and a real_hip_single as one
// uint4 {score, second, pos, frag:16 | fileid:8 | tag:8}.  Every shift below rests on this:
static_assert(sizeof(real_hip_pair) == 40 && offsetof(real_hip_pair, pos1) == 16 && offsetof(real_hip_pair, pos2) == 20 &&
                  offsetof(real_hip_pair, frag) == 32 && offsetof(real_hip_pair, fileid) == 34 && offsetof(real_hip_pair, k1) == 35 &&
                  offsetof(real_hip_pair, k2) == 36 && offsetof(real_hip_pair, inverted1) == 37 && offsetof(real_hip_pair, state) == 38,
              "the decoders read words 2 and 4 of a pair record");
static_assert(sizeof(real_hip_single) == 16 && offsetof(real_hip_single, pos) == 8 && offsetof(real_hip_single, fileid) == 14 &&
                  offsetof(real_hip_single, tag) == 15,
              "the decoders read words z and w of a single record");

// the fragment's fields in the tail word {x, y} of a pair record
static inline RH_HD uint32_t rh_pair_fileid(uint32_t tail_x) { return (tail_x >> 16) & 0xffu; }
static inline RH_HD uint32_t rh_pair_k1(uint32_t tail_x) { return tail_x >> 24; }
static inline RH_HD uint32_t rh_pair_k2(uint32_t tail_y) { return tail_y & 0xffu; }
static inline RH_HD bool rh_pair_inverted1(uint32_t tail_y) { return ((tail_y >> 8) & 0xffu) != 0; } // the forward mate is mate 1 iff false
static inline RH_HD uint32_t rh_pair_state(uint32_t tail_y) { return (tail_y >> 16) & 0xffu; }

// what a record says of its read: a placement or not, on which strand, in which file, with how many mismatches, where
struct RhPlace {
    bool place, inv;
    uint32_t file, k;
    uint64_t pos;
};
static inline RH_HD RhPlace rh_place_info(uint64_t info)
{
    const uint32_t st = (uint32_t)(info >> RH_INFO_ST_SHIFT);
    return RhPlace{st == RH_INFO_STRAIGHT || st == RH_INFO_REVERSE, st == RH_INFO_REVERSE, (uint32_t)(info >> RH_INFO_FI_SHIFT) & 63u,
                   (uint32_t)(info >> RH_INFO_ER_SHIFT) & 15u, info & RH_INFO_POS_MASK};
}
// mate `mate` (0 = mate 1, 1 = mate 2) of a pair record from its words 2 {pos1, pos2} and 4 {tail_x, tail_y}: a Unique record
// places both mates, mate 2 on the other strand; *state: the record's
static inline RH_HD RhPlace rh_place_pair(uint32_t pos1, uint32_t pos2, uint32_t tail_x, uint32_t tail_y, uint32_t mate, uint32_t *state)
{
    *state = rh_pair_state(tail_y);
    return RhPlace{*state == REAL_HIP_PAIR_UNIQUE, rh_pair_inverted1(tail_y) != (mate != 0), rh_pair_fileid(tail_x),
                   mate ? rh_pair_k2(tail_y) : rh_pair_k1(tail_x), mate ? pos2 : pos1};
}
// a single record from its words z (pos) and w
static inline RH_HD RhPlace rh_place_single(uint32_t z, uint32_t w)
{
    const uint32_t tag = w >> 24;
    return RhPlace{REAL_HIP_SINGLE_STATE(tag) == REAL_HIP_PAIR_UNIQUE, REAL_HIP_SINGLE_INVERTED(tag) != 0, (w >> 16) & 0xffu, REAL_HIP_SINGLE_K(tag), z};
}

// ---- the gap record ---------------------------------------------------------------------------------------------
// The kernels write and read a real_hip_gap_place as one uint4 {x, y, z, w} (little endian): x = pos, y = frag:16 | fileid:8 |
// tag:8, z = split:16 | gap:8 | k:8, w = cost:16 | second:16 (gap_core.h packs it).  Every shift below rests on this:
static_assert(sizeof(real_hip_gap_place) == 16 && offsetof(real_hip_gap_place, pos) == 0 && offsetof(real_hip_gap_place, frag) == 4 &&
                  offsetof(real_hip_gap_place, fileid) == 6 && offsetof(real_hip_gap_place, tag) == 7 && offsetof(real_hip_gap_place, split) == 8 &&
                  offsetof(real_hip_gap_place, gap) == 10 && offsetof(real_hip_gap_place, k) == 11 && offsetof(real_hip_gap_place, cost) == 12 &&
                  offsetof(real_hip_gap_place, second) == 14,
              "a gap record is one uint4");
static_assert(REAL_HIP_GAP_TARGET(0x01u) == 1u && REAL_HIP_GAP_TARGET(0xfeu) == 0u && REAL_HIP_GAP_INVERTED(0x10u) == 1u &&
                  REAL_HIP_GAP_INVERTED(0xefu) == 0u && REAL_HIP_GAP_STATE(0x60u) == 3u && REAL_HIP_GAP_STATE(0x9fu) == 0u,
              "the tag: bit 0 the target mate, bit 4 inverted, bits 5-6 the state");
static_assert(REAL_HIP_GAP_MAX < 128u && REAL_HIP_MAX_PATL + REAL_HIP_GAP_MAX < 65536u, "a gap fits its int8, a split and a text offset of a span 16 bits");

// what a gap record says: the state, the file, which mate is placed (target: 0 = mate 1) and on which strand, the fragment of
// the text, the position p, the split j, the gap g (> 0 deleted text positions, < 0 inserted read bases) and the mismatch count
struct RhGapRecord {
    uint32_t state, file, target, inv, frag, p, j, k; // (a register each)
    int32_t g;
};
static inline RH_HD RhGapRecord rh_place_gap(uint32_t x, uint32_t y, uint32_t z, uint32_t w)
{
    (void)w; // (cost and second say nothing of the placement)
    const uint32_t tag = y >> 24;
    return RhGapRecord{REAL_HIP_GAP_STATE(tag), (y >> 16) & 0xffu, REAL_HIP_GAP_TARGET(tag), REAL_HIP_GAP_INVERTED(tag), y & 0xffffu, x, z & 0xffffu, z >> 24,
                       (int32_t)(int8_t)((z >> 16) & 0xffu)};
}
// The geometry of a gapped placement of a read of L bases at p in a text of n: the two diagonals read[0, j) on text[p, p + j)
// and read[j + d, L) on text[p + j + del, p + L + g), with d = max(-g, 0) inserted read bases and del = max(g, 0) deleted text
// positions.  It fits iff the read is no longer than REAL_HIP_MAX_PATL (read_extent's 0xffffffff is not), |g| <=
// REAL_HIP_GAP_MAX, the split leaves a base on either side of a gap (1 <= j, j + d + 1 <= L; j == 0 without a gap) and the span
// ends inside the text (L + g >= 2 for a split that fits).
struct RhGapFit {
    uint32_t fits, d, del;
};
static inline RH_HD RhGapFit rh_gap_fit(uint32_t L, int32_t g, uint32_t j, uint32_t p, uint64_t n)
{
    const uint32_t ag = (uint32_t)(g < 0 ? -g : g), d = g < 0 ? ag : 0u, del = g > 0 ? ag : 0u;
    bool fits = L <= REAL_HIP_MAX_PATL && ag <= REAL_HIP_GAP_MAX;
    if (fits) fits = g ? (j >= 1u && j + d + 1u <= L) : j == 0u;
    if (fits) fits = (uint64_t)p + (uint64_t)((int64_t)L + g) <= n;
    return RhGapFit{fits ? 1u : 0u, d, del};
}
