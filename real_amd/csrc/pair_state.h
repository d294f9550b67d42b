// pair_state.h -- what the paired-end stages share (include/real_hip.h, "paired-end reads"): the view of the two mates' hit
// lists with the clamped range of a fragment's hits, the concordance test, the lane budget and the hand-over of what is
// beyond it to a wave kernel (the join pair_kernel.hip, the enumeration pair_all.hip, the single placements single_fold.hip);
// and the fold state of the pair records with the candidate made of two placements (the join and the mate search
// mate_search.hip, which fold candidates of the same kind into the same records).
#pragma once
#include "stage_common.h" // RH_PAIR_STRIPES: the statistics lines of every stage

#define RH_PAIR_LANE_BUDGET 32u   /* product cells a lane walks itself */

// real_hip_hit as a uint4: x read, y pos, z score bits, w frag:16 | k:8 | inverted:8.
// Hit a of mate 1 and hit b of mate 2 (read lengths la, lb) are concordant: same fragment, opposite strands, the forward
// hit neither starts nor ends behind the reverse one, outer distance within the bounds.  outer: r.pos + len_r - f.pos
// the outer distance of a forward placement at fp and a reverse one of len_r bases at rp (64-bit: positions reach 2^32)
static __device__ __forceinline__ uint64_t pair_outer(uint64_t fp, uint64_t rp, uint32_t len_r) { return rp + len_r - fp; }
static __device__ __forceinline__ bool pair_concordant(const uint4 a, const uint4 b, uint32_t la, uint32_t lb, uint32_t min_insert,
                                                       uint32_t max_insert, uint64_t &outer)
{
    const uint32_t inva = a.w >> 24, invb = b.w >> 24;
    if ((a.w & 0xffffu) != (b.w & 0xffffu) || (inva != 0) == (invb != 0)) return false;
    const bool a_fwd = inva == 0;
    const uint64_t fp = a_fwd ? a.y : b.y, rp = a_fwd ? b.y : a.y;
    const uint64_t fe = fp + (a_fwd ? la : lb), re = rp + (a_fwd ? lb : la);
    if (fp > rp || fe > re) return false;
    outer = pair_outer(fp, rp, a_fwd ? lb : la);
    return outer >= min_insert && outer <= max_insert;
}

// The hit lists of the two mates (of the two lists of a fold): real_hip_hit records, n + 1 offsets into them, the read
// lengths, and per list an upper bound `total` of the hits inside its buffer (real_hip_match_pairs passes the matcher's
// count before duplicates go): the offsets are clamped to it, o[n] is the real end.
struct MateLists {
    const uint4 *h[2];
    const uint64_t *o[2];
    const uint32_t *len[2];
    uint64_t total[2];
    // hits [lo, hi) of fragment i in list m
    __device__ __forceinline__ void range(uint32_t m, uint64_t i, uint64_t &lo, uint64_t &hi) const
    {
        hi = o[m][i + 1]; lo = o[m][i];
        if (hi > total[m]) hi = total[m];
        if (lo > hi) lo = hi;
    }
};

// The end of a lane kernel: the lanes with more work than a lane's budget (`handed`) append their entry to the hand-over
// list (one atomic per wave, the slots in lane order), and the wave adds its work and the number handed over to words 0
// and 1 of a statistics stripe (one stripe per block).  Every lane of the wave calls it.
template <typename E>
static __device__ __forceinline__ void pair_hand_over(bool handed, E entry, unsigned long long work, uint32_t stripe, E *list,
                                                      unsigned long long *list_count, unsigned long long *stats)
{
    const unsigned long long mask = __ballot(handed);
    const uint32_t lane = threadIdx.x & 63u;
    if (mask) {
        unsigned long long base = 0;
        const int leader = __ffsll((long long)mask) - 1;
        if ((int)lane == leader) base = atomicAdd(list_count, (unsigned long long)__popcll(mask));
        base = __shfl(base, leader);
        if (handed) list[base + __popcll(mask & ((1ull << lane) - 1ull))] = entry;
    }
    for (int d = 32; d; d >>= 1) work += __shfl_xor(work, d);
    if (lane == 0) {
        unsigned long long *s = stats + (size_t)(stripe % RH_PAIR_STRIPES) * 16;
        if (work) atomicAdd(s, work);
        if (mask) atomicAdd(s + 1, (unsigned long long)__popcll(mask));
    }
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
// the candidate made of a placement of mate 1 (pos1, score bits s1, k1 mismatches, inv1: reverse strand) and one of mate 2
static __device__ __forceinline__ void ps_candidate(PairState &c, uint32_t scores, uint32_t fileid, uint32_t frag, uint32_t pos1, uint32_t pos2,
                                                    uint32_t inv1, uint32_t s1, uint32_t s2, uint32_t k1, uint32_t k2)
{
    c.best = scores ? (double)__uint_as_float(s1) + (double)__uint_as_float(s2) : -(double)(k1 + k2);
    c.second = pair_neg_inf();
    c.lhi = ((uint64_t)fileid << 48) | ((uint64_t)frag << 32) | pos1;
    c.llo = ((uint64_t)pos2 << 1) | inv1;
    c.s1 = s1; c.s2 = s2; c.k = k1 | (k2 << 8);
}
// butterfly: every lane ends with the wave's state
static __device__ __forceinline__ void ps_butterfly(PairState &st)
{
    for (int d = 32; d; d >>= 1) {
        PairState o;
        o.best = __shfl_xor(st.best, d); o.second = __shfl_xor(st.second, d);
        o.lhi = __shfl_xor((unsigned long long)st.lhi, d); o.llo = __shfl_xor((unsigned long long)st.llo, d);
        o.s1 = __shfl_xor(st.s1, d); o.s2 = __shfl_xor(st.s2, d); o.k = __shfl_xor(st.k, d);
        ps_merge(st, o);
    }
}
// the eps of a pair record (ps_to_record) of mates la and lb bases long
static __device__ __forceinline__ double ps_eps(uint32_t scores, double filter_mult, uint32_t la, uint32_t lb)
{
    return scores ? (double)(float)(filter_mult * (double)((uint64_t)la + lb)) : 0.0;
}
