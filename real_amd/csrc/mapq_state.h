// mapq_state.h -- the accumulator of the mapping quality (include/real_hip.h, "mapping quality"): the histogram of a read's
// candidate levels below the highest one, its merge, and the quality of a placement against it.  The kernels of mapq.hip and
// the host helpers real_hip_mapq_acc_merge / real_hip_mapq_of compile the same functions, so the arithmetic is tested without
// a GPU.
// The 32 one-byte counts live in four 64-bit words (cnt[j] is byte j & 7 of word j >> 3, the record's own layout): the shift,
// the saturating byte add and the read of one count are word arithmetic and selects.  Nothing is an array indexed at run time
// (it would live in scratch memory); the loops over the tables are unrolled, their indices constants.
#pragma once
#include <math.h>
#include <stdint.h>
#include "final_record.h" // RH_HD, real_hip.h

static_assert(sizeof(real_hip_mapq_acc) == 40 && offsetof(real_hip_mapq_acc, n) == 4 && offsetof(real_hip_mapq_acc, cnt) == 8 &&
                  REAL_HIP_MAPQ_LEVELS == 32,
              "the kernels read an accumulator as five 8-byte words: level | n << 32, then the counts");

static constexpr uint32_t RH_MAPQ_W[REAL_HIP_MAPQ_LEVELS] = REAL_HIP_MAPQ_W_INIT;
static constexpr uint32_t RH_MAPQ_A[REAL_HIP_MAPQ_MAX + 1] = REAL_HIP_MAPQ_A_INIT;
#define RH_MAPQ_EMPTY_LEVEL INT32_MIN

struct MapqState {
    int32_t  level;                // the highest level seen; RH_MAPQ_EMPTY_LEVEL: none
    uint32_t n;                    // candidates seen, saturating
    uint64_t c0, c1, c2, c3;       // the counts, cnt[0] in the lowest byte of c0
};

static inline RH_HD void mq_clear(MapqState &s)
{
    s.level = RH_MAPQ_EMPTY_LEVEL; s.n = 0;
    s.c0 = s.c1 = s.c2 = s.c3 = 0;
}
// the level of a value in bits (scores on) and of a mismatch count (scores off)
static inline RH_HD int32_t mq_level_of_value(double v)
{
    const double f = floor(2.0 * v);
    if (!(f > -2147483648.0)) return INT32_MIN + 1; // (NaN too)
    if (f >= 2147483647.0) return INT32_MAX;
    return (int32_t)f;
}
static inline RH_HD int32_t mq_level_of_k(uint32_t k) { return -(int32_t)(REAL_HIP_MAPQ_MISMATCH_LEVELS * k); }
// one candidate
static inline RH_HD void mq_one(MapqState &s, int32_t level)
{
    s.level = level; s.n = 1;
    s.c0 = 1; s.c1 = s.c2 = s.c3 = 0;
}
// the counts move d levels down the window (cnt[j] -> cnt[j + d]); what leaves it is dropped
static inline RH_HD void mq_shift(MapqState &s, uint64_t d)
{
    const uint32_t w = d > 31 ? 4u : (uint32_t)(d >> 3), b = (uint32_t)(d & 7u) * 8u;
    const uint64_t a0 = s.c0, a1 = s.c1, a2 = s.c2, a3 = s.c3;
    s.c3 = w == 0 ? a3 : w == 1 ? a2 : w == 2 ? a1 : w == 3 ? a0 : 0;
    s.c2 = w == 0 ? a2 : w == 1 ? a1 : w == 2 ? a0 : 0;
    s.c1 = w == 0 ? a1 : w == 1 ? a0 : 0;
    s.c0 = w == 0 ? a0 : 0;
    if (b) {
        s.c3 = (s.c3 << b) | (s.c2 >> (64 - b));
        s.c2 = (s.c2 << b) | (s.c1 >> (64 - b));
        s.c1 = (s.c1 << b) | (s.c0 >> (64 - b));
        s.c0 <<= b;
    }
}
// eight byte sums at once, each saturating at 255
static inline RH_HD uint64_t mq_sat_add8(uint64_t a, uint64_t b)
{
    const uint64_t H = 0x8080808080808080ull;
    const uint64_t low = (a & ~H) + (b & ~H);           // the low seven bits of every byte: no carry leaves a byte
    const uint64_t sum = low ^ ((a ^ b) & H);
    const uint64_t carry = ((a & b) | ((a | b) & low)) & H; // the carry out of every byte's top bit
    return sum | ((carry >> 7) * 0xffull);
}
// a := merge(a, b): both aligned to the larger level, the counts added.  An empty state holds zeros below INT32_MIN.
static inline RH_HD void mq_merge(MapqState &a, const MapqState &b)
{
    MapqState o = b;
    const int32_t top = a.level > o.level ? a.level : o.level;
    mq_shift(a, (uint64_t)((int64_t)top - a.level));
    mq_shift(o, (uint64_t)((int64_t)top - o.level));
    a.level = top;
    const uint64_t n = (uint64_t)a.n + o.n;
    a.n = n > 0xffffffffull ? 0xffffffffu : (uint32_t)n;
    a.c0 = mq_sat_add8(a.c0, o.c0); a.c1 = mq_sat_add8(a.c1, o.c1);
    a.c2 = mq_sat_add8(a.c2, o.c2); a.c3 = mq_sat_add8(a.c3, o.c3);
}
static inline RH_HD void mq_add_level(MapqState &a, int32_t level)
{
    MapqState c;
    mq_one(c, level);
    mq_merge(a, c);
}
// the record as five 8-byte words; a record with n = 0 is empty whatever else it says
static inline RH_HD void mq_from_words(MapqState &s, uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3, uint64_t w4)
{
    s.level = (int32_t)(uint32_t)w0; s.n = (uint32_t)(w0 >> 32);
    s.c0 = w1; s.c1 = w2; s.c2 = w3; s.c3 = w4;
    if (!s.n) mq_clear(s);
}
static inline RH_HD uint64_t mq_word0(const MapqState &s) { return (uint64_t)(uint32_t)s.level | ((uint64_t)s.n << 32); }
// cnt[j], 0 <= j <= 31
static inline RH_HD uint32_t mq_count(const MapqState &s, uint32_t j)
{
    // (masks, not a choice between the four fields: the compiler turns that into one load at a run-time offset of the state)
    const uint64_t w = j >> 3;
    const uint64_t c = (s.c0 & (0 - (uint64_t)(w == 0))) | (s.c1 & (0 - (uint64_t)(w == 1))) | (s.c2 & (0 - (uint64_t)(w == 2))) |
                       (s.c3 & (0 - (uint64_t)(w == 3)));
    return (uint32_t)(c >> ((j & 7u) * 8u)) & 255u;
}
// the quality of a placement of level lp against acc (include/real_hip.h, QUALITY); unlisted: it was not among the candidates
static inline RH_HD uint32_t mq_quality(const MapqState &acc, int32_t lp, bool &unlisted)
{
    MapqState s = acc;
    int64_t j = (int64_t)s.level - lp;
    unlisted = j < 0 || j > 31 || mq_count(s, (uint32_t)(j & 31)) == 0;
    if (unlisted) {
        mq_add_level(s, lp);
        j = (int64_t)s.level - lp;
    }
    // (the words' bytes at constant shifts: the loops below run over the tables alone)
#define MQ_DOT8(c, b)                                                                                                              \
    ((((c) >> 0) & 255u) * (uint64_t)RH_MAPQ_W[(b) + 0] + (((c) >> 8) & 255u) * (uint64_t)RH_MAPQ_W[(b) + 1] +                       \
     (((c) >> 16) & 255u) * (uint64_t)RH_MAPQ_W[(b) + 2] + (((c) >> 24) & 255u) * (uint64_t)RH_MAPQ_W[(b) + 3] +                     \
     (((c) >> 32) & 255u) * (uint64_t)RH_MAPQ_W[(b) + 4] + (((c) >> 40) & 255u) * (uint64_t)RH_MAPQ_W[(b) + 5] +                     \
     (((c) >> 48) & 255u) * (uint64_t)RH_MAPQ_W[(b) + 6] + (((c) >> 56) & 255u) * (uint64_t)RH_MAPQ_W[(b) + 7])
    const uint64_t S = MQ_DOT8(s.c0, 0) + MQ_DOT8(s.c1, 8) + MQ_DOT8(s.c2, 16) + MQ_DOT8(s.c3, 24);
#undef MQ_DOT8
    uint64_t wj = 0; // (stays 0 for a placement below the window)
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (uint32_t t = 0; t < REAL_HIP_MAPQ_LEVELS; ++t)
        if ((int64_t)t == j) wj = RH_MAPQ_W[t];
    const uint64_t E = S - wj;
    uint32_t q = 0; // A[] rises: the Q that qualify are 0 .. q
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (uint32_t t = 1; t <= REAL_HIP_MAPQ_MAX; ++t) q += E * RH_MAPQ_A[t] <= 16 * S ? 1u : 0u;
    return q;
}
