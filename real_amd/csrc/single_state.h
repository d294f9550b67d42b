// single_state.h -- the fold state of the single placements of a mate (include/real_hip.h, "single placements of a
// mate"): the top two of a set of (value, location) under the total order (value descending, location ascending), as
// pair_state.h keeps them for the pairs.  The values are scores (floats) or small integers, so the record holds floats;
// the fold and the state's comparison are in FP64, which holds every float exactly.
#pragma once
#include "real_hip_ctx.h"
#include "pair_state.h"

#define RH_SINGLE_LANE_BUDGET 32u /* hits a lane walks itself (the join's budget, RH_PAIR_LANE_BUDGET; not measured for the fold) */

struct SingleState {
    double best, second;           // -inf: none
    uint64_t loc;                  // fileid:8 | frag:16 | pos:32 | inverted:1
    uint32_t s;                    // score bits of the best hit
    uint32_t k;
};

static __device__ __forceinline__ void ss_clear(SingleState &s)
{
    s.best = s.second = pair_neg_inf();
    s.loc = 0; s.s = s.k = 0;
}
// the larger value; of +0.0 and -0.0 (equal values, different bits) always the same one, whatever the order of the arguments
static __device__ __forceinline__ double ss_max(double a, double b)
{
    if (a > b) return a;
    if (b > a) return b;
    return __double_as_longlong(a) <= __double_as_longlong(b) ? a : b;
}
// a := top two of (a union b); a location counts once (its value is a function of the location)
static __device__ __forceinline__ void ss_merge(SingleState &a, const SingleState &b)
{
    const double ninf = pair_neg_inf();
    if (b.best == ninf) return;
    if (a.best == ninf) { a = b; return; }
    if (a.loc == b.loc) { a.second = ss_max(a.second, b.second); return; }
    const bool b_wins = b.best > a.best || (b.best == a.best && b.loc < a.loc);
    if (b_wins) { const double s = ss_max(b.second, a.best); a = b; a.second = s; }
    else a.second = ss_max(a.second, b.best);
}
// one hit (real_hip_hit as a uint4: x read, y pos, z score bits, w frag:16 | k:8 | inverted:8) as a state
static __device__ __forceinline__ void ss_from_hit(SingleState &s, const uint4 h, uint32_t fileid, uint32_t scores)
{
    const uint32_t k = (h.w >> 16) & 15u;
    s.best = scores ? (double)__uint_as_float(h.z) : -(double)k;
    s.second = pair_neg_inf();
    s.loc = ((uint64_t)fileid << 49) | ((uint64_t)(h.w & 0xffffu) << 33) | ((uint64_t)h.y << 1) | ((h.w >> 24) ? 1u : 0u);
    s.s = h.z; s.k = k;
}
// real_hip_single as a uint4: x score bits, y second bits, z pos, w frag:16 | fileid:8 | tag:8 (k:4, inverted:1, state:2)
static __device__ __forceinline__ void ss_from_record(SingleState &s, const uint4 r, uint32_t scores)
{
    const uint32_t tag = r.w >> 24;
    if (REAL_HIP_SINGLE_STATE(tag) == REAL_HIP_PAIR_NOMATCH) { ss_clear(s); return; } // (the other fields of an empty record are ignored)
    s.k = REAL_HIP_SINGLE_K(tag);
    s.best = scores ? (double)__uint_as_float(r.x) : -(double)s.k;
    s.second = (double)__uint_as_float(r.y);
    s.loc = ((uint64_t)((r.w >> 16) & 0xffu) << 49) | ((uint64_t)(r.w & 0xffffu) << 33) | ((uint64_t)r.z << 1) | REAL_HIP_SINGLE_INVERTED(tag);
    s.s = r.x;
}
static __device__ __forceinline__ uint4 ss_to_record(const SingleState &s, double eps)
{
    if (s.best == pair_neg_inf()) return make_uint4(0u, 0xff800000u, 0u, 0u); // score 0, second -inf, everything else 0
    const uint32_t state = s.second >= s.best - eps ? REAL_HIP_PAIR_NONUNIQUE : REAL_HIP_PAIR_UNIQUE;
    const uint32_t tag = (s.k & 15u) | ((uint32_t)(s.loc & 1u) << 4) | (state << 5);
    return make_uint4(s.s, __float_as_uint((float)s.second), (uint32_t)(s.loc >> 1),
                      (uint32_t)((s.loc >> 33) & 0xffffu) | ((uint32_t)((s.loc >> 49) & 0xffu) << 16) | (tag << 24));
}
