// pair_state.h -- the fold state of the paired-end records (include/real_hip.h, "paired-end reads"): shared by the join
// (pair_kernel.hip) and the mate search (mate_search.hip), which fold candidates of the same kind into the same records;
// and what the join shares with the enumeration of all concordant pairs (pair_all.hip): the concordance test, the
// clamped range of a fragment's hits and the lane budget.
#pragma once
#include "real_hip_internal.h"

#define RH_PAIR_LANE_BUDGET 32u   /* product cells a lane walks itself */
#define RH_PAIR_STRIPES 256u      /* the statistics are striped over this many 128-byte lines (see RH_CSTRIPES) */

// real_hip_hit as a uint4: x read, y pos, z score bits, w frag:16 | k:8 | inverted:8.
// Hit a of mate 1 and hit b of mate 2 (read lengths la, lb) are concordant: same fragment, opposite strands, the forward
// hit neither starts nor ends behind the reverse one, outer distance within the bounds.  outer: r.pos + len_r - f.pos
static __device__ __forceinline__ bool pair_concordant(const uint4 a, const uint4 b, uint32_t la, uint32_t lb, uint32_t min_insert,
                                                       uint32_t max_insert, uint64_t &outer)
{
    const uint32_t inva = a.w >> 24, invb = b.w >> 24;
    if ((a.w & 0xffffu) != (b.w & 0xffffu) || (inva != 0) == (invb != 0)) return false;
    const bool a_fwd = inva == 0;
    const uint64_t fp = a_fwd ? a.y : b.y, rp = a_fwd ? b.y : a.y;
    const uint64_t fe = fp + (a_fwd ? la : lb), re = rp + (a_fwd ? lb : la);
    if (fp > rp || fe > re) return false;
    outer = re - fp;
    return outer >= min_insert && outer <= max_insert;
}
// hits [lo, hi) of fragment i: the offsets clamped to `total`, an upper bound of the hits inside the buffer
static __device__ __forceinline__ void pair_range(const uint64_t *o, uint64_t i, uint64_t total, uint64_t &lo, uint64_t &hi)
{
    hi = o[i + 1]; lo = o[i];
    if (hi > total) hi = total;
    if (lo > hi) lo = hi;
}

// top two of a set of (value, location): the best with its payload, and the highest value at another location
struct PairState {
    double best, second;
    uint64_t lhi, llo;             // location: fileid:16 | frag:16 | pos1:32, then pos2:32 | inverted1:1
    uint32_t s1, s2;               // score bits
    uint32_t k;                    // k1 | k2 << 8
};

static __device__ __forceinline__ double pair_neg_inf() { return -__builtin_huge_val(); }
static __device__ __forceinline__ void ps_clear(PairState &s)
{
    s.best = s.second = pair_neg_inf();
    s.lhi = s.llo = 0; s.s1 = s.s2 = s.k = 0;
}
static __device__ __forceinline__ void ps_take(PairState &a, const PairState &b)
{
    a.best = b.best; a.lhi = b.lhi; a.llo = b.llo; a.s1 = b.s1; a.s2 = b.s2; a.k = b.k;
}
// a := top two of (a union b)
static __device__ __forceinline__ void ps_merge(PairState &a, const PairState &b)
{
    const double ninf = pair_neg_inf();
    if (b.best == ninf) return;
    if (a.best == ninf) { ps_take(a, b); a.second = b.second; return; }
    if (a.lhi == b.lhi && a.llo == b.llo) { // the same location twice (a set: it counts once)
        if (b.best > a.best) ps_take(a, b);
        a.second = fmax(a.second, b.second);
        return;
    }
    const bool b_wins = b.best > a.best || (b.best == a.best && (b.lhi < a.lhi || (b.lhi == a.lhi && b.llo < a.llo)));
    if (b_wins) { const double s = fmax(b.second, a.best); ps_take(a, b); a.second = s; }
    else a.second = fmax(a.second, b.best);
}

static __device__ __forceinline__ void ps_from_record(PairState &s, const real_hip_pair &r)
{
    s.best = r.best; s.second = r.second;
    s.lhi = ((uint64_t)r.fileid << 48) | ((uint64_t)r.frag << 32) | r.pos1;
    s.llo = ((uint64_t)r.pos2 << 1) | (r.inverted1 & 1u);
    s.s1 = __float_as_uint(r.score1); s.s2 = __float_as_uint(r.score2);
    s.k = r.k1 | ((uint32_t)r.k2 << 8);
    if (s.best == pair_neg_inf()) ps_clear(s);
}
static __device__ __forceinline__ void ps_to_record(const PairState &s, double eps, real_hip_pair &r)
{
    const bool none = s.best == pair_neg_inf();
    r.best = s.best; r.second = none ? pair_neg_inf() : s.second;
    r.pos1 = none ? 0u : (uint32_t)s.lhi; r.pos2 = none ? 0u : (uint32_t)(s.llo >> 1);
    r.score1 = none ? 0.f : __uint_as_float(s.s1); r.score2 = none ? 0.f : __uint_as_float(s.s2);
    r.frag = none ? 0 : (uint16_t)(s.lhi >> 32); r.fileid = none ? 0 : (uint8_t)(s.lhi >> 48);
    r.k1 = none ? 0 : (uint8_t)s.k; r.k2 = none ? 0 : (uint8_t)(s.k >> 8);
    r.inverted1 = none ? 0 : (uint8_t)(s.llo & 1u);
    r.state = none ? REAL_HIP_PAIR_NOMATCH : (s.second >= s.best - eps ? REAL_HIP_PAIR_NONUNIQUE : REAL_HIP_PAIR_UNIQUE);
    r.reserved = 0;
}
