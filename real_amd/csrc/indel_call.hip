// indel_call.hip -- from the gap rescue's records to indel calls (include/real_hip.h, "indel calls"): the insertion or
// deletion every rescued mate shows, left-normalised against the text, the mates that show the same one added up, the
// pileup's depth beside them, three genotype likelihoods per distinct event and the compacted call list.
//
// indel_add_kernel: one lane per fragment (wave64, blocks of 256).  read_walk.h's placed_gap takes the gap record to a placement
// (about one fragment in fifty carries a gap: DESIGN.md 7h, so nothing is compacted), then the span must lie inside the
// record's fragment -- every check comes before the first byte of read or text is touched.  The N bits of the anchor and of the
// deleted range are one funnel-shifted word of the N vector; the quality is the minimum over the at most 18 oriented read
// offsets j - 1 .. j + d; the inserted bases are ReadWalk::oriented_from's word.  The left shift is the length of the run,
// ending at x, of positions i with T'[i] == T'[i + |g|] (T' = the text, for an insertion with S spliced in at x): 32 positions
// a step -- T' at a and at a + |g| funnel-shifted, XOR, the N bits of a and a - 1 ORed in, count of trailing zeros -- and no
// loop over bases.  A surviving lane appends its 16-byte event {x, g + 128, S, q | forward << 8} to the event list with one
// atomic per wave (pair_hand_over); the list has room for one event per fragment of the call, so it cannot overflow.
//
// finish, once per set of adds: two stable passes of rocPRIM's radix sort -- the key (x, g, S) is 72 bits wide, so S first
// (32 bits) and then x << 8 | g + 128 (40 bits), the 16-byte events as the values; a head-flag pass over the sorted events
// (count, scan, emit: the index of every group's first event); one lane per distinct event sums its group (a group may span
// any number of blocks of the head pass: the lane walks the sorted list), reads the two depths and the anchor's base,
// computes the three PLs and writes the grouped table.  Every finish: count, scan, emit over the table -- the count pass also
// writes the event list with the thresholds' decision -- as call_finish does.
//
// Everything is an integer sum or a function of one.  No LDS beyond the block counts, no scratch memory, no register array
// indexed at run time; plain C++ and vector stores.
#include "read_walk.h"
#include "pair_state.h" // pair_hand_over

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cstring>

#define RH_ID_BLOCK 256u

// ---- the stage's state (real_hip_ctx::indel) ------------------------------------------------------------------------------
void rh_indel_release(real_hip_ctx *ctx)
{
    RhIndelStage *s = &ctx->indel; // (releasing a buffer that was never made does nothing)
    rh_release(ctx, s->ev); rh_release(ctx, s->ev2); rh_release(ctx, s->key[0]); rh_release(ctx, s->key[1]); rh_release(ctx, s->blk);
    rh_release(ctx, s->starts); rh_release(ctx, s->table); rh_release(ctx, s->events); rh_release(ctx, s->calls);
    s->state = 0; s->grouped = false;
    s->n_ev = s->n_groups = s->n_calls = s->het = s->hom = s->dels = s->ins = 0;
}

// ---- add: the events of the records ---------------------------------------------------------------------------------------
struct IndelAddArgs : GapRecordArgs {
    uint32_t min_qual;
    uint4 *ev;                     // the event list
    unsigned long long *ev_count;  // its length
    unsigned long long *stats;     // RH_PAIR_STRIPES x 16 words: [0] placed, [1] events, [2] other_file, [3] invalid, [4] ungapped,
                                   // [5] on_n, [6] low_qual, [7] shifted, [8] shift_capped
};

// the 32 text bases from position pos on (base u at bits 63 - 2u, 62 - 2u); the text is padded behind its end
static __device__ __forceinline__ uint64_t id_text_at(const uint64_t *__restrict__ T, uint64_t pos)
{
    const uint64_t wi = pos >> 5;
    const uint32_t sh = 2u * (uint32_t)(pos & 31u);
    const uint64_t t0 = T[wi], t1 = T[wi + 1];
    return sh ? ((t0 << sh) | (t1 >> (64 - sh))) : t0;
}
// the 32 bases of T' from position pos on: the text, for an insertion (ins) text[0, x) followed by the bases of sw
static __device__ __forceinline__ uint64_t id_tprime_at(const uint64_t *__restrict__ T, uint64_t pos, bool ins, uint64_t x, uint64_t sw)
{
    if (!ins) return id_text_at(T, pos);
    const int64_t tb = (int64_t)x - (int64_t)pos; // text bases in front of S
    if (tb >= 32) return id_text_at(T, pos);
    if (tb <= 0) return sw << (2u * (uint32_t)(-tb));
    return (id_text_at(T, pos) & (~0ull << (64 - 2 * tb))) | (sw >> (2 * tb));
}

__global__ void __launch_bounds__(RH_ID_BLOCK) indel_add_kernel(const IndelAddArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * RH_ID_BLOCK + threadIdx.x;
    uint32_t placed = 0, other = 0, invalid = 0, ungapped = 0, on_n = 0, lowq = 0, shifted = 0, capped = 0;
    bool live = false;
    uint4 event = make_uint4(0, 0, 0, 0);
    if (i < A.n) {
        const PlacedGap c = placed_gap(A, i);
        other = c.other; invalid = c.bad;
        if (c.place) {
            const DevBatch b = A.mate(c.second);
            const bool inv = c.inv != 0;
            const uint32_t p = c.p, L = c.L, j = c.j, d = c.d, del = c.del, ag = d | del; // (one of d, del is 0)
            const uint64_t start = c.start;
            const int32_t g = (int32_t)del - (int32_t)d;
            // the fragment, on top of the rule of the gapped lists and as that before anything is read
            const uint64_t end = (uint64_t)p + L - d + del;
            bool fits = c.frag < A.t.n_frag;
            uint64_t fs = 0;
            if (fits) {
                fs = A.t.frag_start[c.frag];
                fits = p >= fs && end <= A.t.frag_start[c.frag + 1];
            }
            if (!fits) {
                invalid = 1;
            } else if (!ag) {
                placed = 1; ungapped = 1;
            } else {
                placed = 1;
                const uint64_t x = (uint64_t)p + c.len1(); // behind the first diagonal (x - 1 >= p >= fs; x + del <= end - 1 < n)
                // the N bits of the anchor and of the deleted range: positions x - 1 .. x + del - 1
                const uint64_t nf = A.t.has_wild ? mm_n_flags(A.t.wild, x - 1) & (~0ull << (62 - 2 * del)) : 0ull;
                if (nf) {
                    on_n = 1;
                } else {
                    uint32_t q = 30u;
                    if (b.qual) {
                        q = 0xffu;
                        for (uint32_t k = j - 1; k <= j + d; ++k) q = min(q, (uint32_t)b.qual[start + (inv ? L - 1 - k : k)]);
                    }
                    if (q < A.min_qual) {
                        lowq = 1;
                    } else {
                        const bool ins = d != 0;
                        uint64_t sw = 0;
                        if (ins) sw = ReadWalk::oriented_from(b, start, L, inv, j, d) & (~0ull << (64 - 2 * d));
                        // the run of T'[i] == T'[i + |g|] below x, the steps allowed being i > fs with the N bits of i and
                        // i - 1 clear; one step beyond the cap is looked at: is the cap what stops the event
                        const uint64_t room = x - 1 - fs;
                        const uint32_t lim = room > REAL_HIP_INDEL_SHIFT_MAX ? REAL_HIP_INDEL_SHIFT_MAX + 1u : (uint32_t)room;
                        uint32_t done = 0;
                        while (done < lim) {
                            const uint32_t nb = min(32u, lim - done);
                            const uint64_t a = x - done - nb; // (>= fs + 1)
                            const uint64_t df = id_tprime_at(A.t.text, a, ins, x, sw) ^ id_tprime_at(A.t.text, a + ag, ins, x, sw);
                            uint64_t flags = ((df >> 1) | df) & M55;
                            if (A.t.has_wild) flags |= mm_n_flags(A.t.wild, a) | mm_n_flags(A.t.wild, a - 1);
                            flags >>= 64 - 2 * nb; // position a + nb - 1 at bit 0
                            const uint32_t run = flags ? (uint32_t)__builtin_ctzll(flags) >> 1 : nb;
                            done += run;
                            if (run < nb) break;
                        }
                        if (done > REAL_HIP_INDEL_SHIFT_MAX) { capped = 1; done = REAL_HIP_INDEL_SHIFT_MAX; }
                        shifted = done ? 1u : 0u;
                        const uint64_t xf = x - done;
                        uint32_t seq = 0;
                        if (ins) {
                            // S after the shifts is T' from xf on; its first base goes lowest: the 2-bit groups turned round
                            const uint32_t hi = (uint32_t)((id_tprime_at(A.t.text, xf, true, x, sw) & (~0ull << (64 - 2 * d))) >> 32);
                            const uint32_t rv = __brev(hi);
                            seq = ((rv >> 1) & 0x55555555u) | ((rv & 0x55555555u) << 1);
                        }
                        live = true;
                        event = make_uint4((uint32_t)xf, (uint32_t)(g + 128), seq, q | (inv ? 0u : 256u));
                    }
                }
            }
        }
    }
    pair_hand_over(live, event, (unsigned long long)placed, blockIdx.x, A.ev, A.ev_count, A.stats);
    uint32_t s[7] = {other, invalid, ungapped, on_n, lowq, shifted, capped}; // (a wave's sums are at most 64)
    rh_stats_add(A.stats + 2, s);
}

// ---- finish: sort, group, genotype, compact -------------------------------------------------------------------------------
// the sort's keys from the events: PASS 0 the packed S, PASS 1 x << 8 | g + 128
template <int PASS>
__global__ void __launch_bounds__(RH_ID_BLOCK) indel_key_kernel(const uint4 *ev, uint64_t n, uint64_t *key)
{
    const uint64_t i = (uint64_t)blockIdx.x * RH_ID_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint4 e = ev[i];
    key[i] = PASS == 0 ? (uint64_t)e.z : ((uint64_t)e.x << 8) | e.y;
}

// one lane per sorted event: a HEAD differs from its predecessor in (x, g, S).  EMIT = false counts the block's heads, EMIT =
// true writes their indices behind the block's offset; starts[n_groups] = n
template <bool EMIT>
__global__ void __launch_bounds__(RH_ID_BLOCK) indel_heads_kernel(const uint4 *ev, uint64_t n, uint64_t *blk, const uint64_t *blk_off, uint32_t *starts,
                                                                  uint64_t n_groups)
{
    __shared__ uint32_t wave_cnt[RH_ID_BLOCK / 64];
    const uint64_t i = (uint64_t)blockIdx.x * RH_ID_BLOCK + threadIdx.x;
    bool head = false;
    if (i < n) {
        head = i == 0;
        if (i) {
            const uint4 e = ev[i], f = ev[i - 1];
            head = e.x != f.x || e.y != f.y || e.z != f.z;
        }
    }
    const unsigned long long mask = __ballot(head);
    if (!EMIT) {
        const uint32_t c = rh_block_count(mask, wave_cnt);
        if (threadIdx.x == 0) {
            blk[blockIdx.x] = c;
            if (blockIdx.x + 1 == gridDim.x) blk[gridDim.x] = 0;
        }
        return;
    }
    const uint64_t slot = rh_emit_slot(mask, blk_off[blockIdx.x], wave_cnt);
    if (head && slot < n_groups) starts[slot] = (uint32_t)i;
    if (i == 0) starts[n_groups] = (uint32_t)n;
}

struct IndelGroupArgs {
    DevText t;
    const uint4 *ev;               // the sorted events
    const uint32_t *starts;        // n_groups + 1
    uint64_t n_groups;
    const uint32_t *depth;         // the finished pileup's
    const uint32_t *gdepth;        // its gapped placements' share (null: none were piled up)
    uint4 *table;                  // real_hip_indel records, two uint4 each; gt = the best genotype
};

// one lane per distinct event
__global__ void __launch_bounds__(RH_ID_BLOCK) indel_group_kernel(const IndelGroupArgs A)
{
    const uint64_t k = (uint64_t)blockIdx.x * RH_ID_BLOCK + threadIdx.x;
    if (k >= A.n_groups) return;
    const uint32_t a = A.starts[k], e = A.starts[k + 1];
    const uint4 first = A.ev[a];
    uint32_t fwd = 0, qsum = 0;
    for (uint32_t i = a; i < e; ++i) {
        const uint32_t w = A.ev[i].w;
        fwd += (w >> 8) & 1u;
        qsum += w & 0xffu;
    }
    const uint32_t x = first.x, alt_n = e - a; // (1 <= x <= n - 1: the add kernel's geometry)
    uint32_t u0 = A.depth[x - 1], u1 = A.depth[x]; // the ungapped placements alone: no mate counts on both sides
    if (A.gdepth) { u0 -= A.gdepth[x - 1]; u1 -= A.gdepth[x]; }
    const uint32_t ref_n = min(u0, u1);
    const uint32_t ref = (uint32_t)(A.t.text[(x - 1) >> 5] >> (62 - 2 * ((x - 1) & 31u))) & 3u;
    // the three PLs, the first of minimal PL in the order 0/0, 0/1, 1/1
    const uint64_t pl0 = qsum, pl1 = (uint64_t)REAL_HIP_CALL_HET * ((uint64_t)ref_n + alt_n) + REAL_HIP_INDEL_PRIOR_HET,
                   pl2 = (uint64_t)REAL_HIP_INDEL_REF_Q * ref_n + REAL_HIP_INDEL_PRIOR_HOM;
    uint32_t gt = 0;
    uint64_t best = pl0, other = min(pl1, pl2);
    if (pl1 < best) { gt = 1; best = pl1; other = min(pl0, pl2); }
    if (pl2 < best) { gt = 2; best = pl2; other = min(pl0, pl1); }
    const uint64_t qv = pl0 - best, gq = other - best;
    const uint32_t qual = qv > 0xffffffffull ? 0xffffffffu : (uint32_t)qv;
    const uint32_t tail = ((first.y - 128u) & 0xffu) | (gt << 8) | ((gq > 99 ? 99u : (uint32_t)gq) << 16) | (ref << 24);
    A.table[2 * k] = make_uint4(x - 1, ref_n, alt_n, fwd);
    A.table[2 * k + 1] = make_uint4(qsum, qual, first.z, tail);
}

struct IndelCallArgs {
    const uint4 *table;
    uint64_t n_groups;
    uint32_t min_call_qual, min_alt, min_depth;
    uint4 *events;                 // count pass: the event list, gt = the decision
    uint64_t *blk;                 // count pass: calls per block (blocks + 1, the last one 0)
    const uint64_t *blk_off;       // emit pass: their exclusive scan
    uint4 *calls;
    uint64_t cap;
    unsigned long long *fin;       // RH_PAIR_STRIPES x 16 words: [0] het, [1] hom, [2] deletions, [3] insertions
};

// one lane per distinct event; EMIT = false counts the block's calls and writes the event list, EMIT = true writes the calls
template <bool EMIT>
__global__ void __launch_bounds__(RH_ID_BLOCK) indel_calls_kernel(const IndelCallArgs A)
{
    __shared__ uint32_t wave_cnt[RH_ID_BLOCK / 64];
    const uint64_t k = (uint64_t)blockIdx.x * RH_ID_BLOCK + threadIdx.x;
    uint4 r0 = make_uint4(0, 0, 0, 0), r1 = r0;
    if (k < A.n_groups) { r0 = A.table[2 * k]; r1 = A.table[2 * k + 1]; }
    const uint32_t gt = (r1.w >> 8) & 0xffu;
    const bool call = k < A.n_groups && gt != 0 && r1.y >= A.min_call_qual && r0.z >= A.min_alt && (uint64_t)r0.y + r0.z >= A.min_depth;
    const unsigned long long mask = __ballot(call);
    if (!EMIT) {
        if (k < A.n_groups) {
            A.events[2 * k] = r0;
            A.events[2 * k + 1] = make_uint4(r1.x, r1.y, r1.z, call ? r1.w : r1.w & ~0xff00u);
        }
        const uint32_t c = rh_block_count(mask, wave_cnt);
        if (threadIdx.x == 0) {
            A.blk[blockIdx.x] = c;
            if (blockIdx.x + 1 == gridDim.x) A.blk[gridDim.x] = 0;
        }
        const bool deletion = (r1.w & 0x80u) == 0; // (the sign of g)
        uint32_t s[4] = {call && gt == 1 ? 1u : 0u, call && gt == 2 ? 1u : 0u, call && deletion ? 1u : 0u, call && !deletion ? 1u : 0u};
        rh_stats_add(A.fin, s);
        return;
    }
    const uint64_t slot = rh_emit_slot(mask, A.blk_off[blockIdx.x], wave_cnt);
    if (!call || slot >= A.cap) return; // (the latter cannot happen: the table is what the count saw)
    A.calls[2 * slot] = r0;
    A.calls[2 * slot + 1] = r1;
}

// ---- host side --------------------------------------------------------------------------------------------------
// room for `bytes` with the first `keep` bytes kept
static int indel_grow(real_hip_ctx *ctx, DevBuf &b, size_t keep, size_t bytes)
{
    if (bytes <= b.cap) return REAL_HIP_OK;
    if (!keep) return rh_reserve(ctx, b, bytes);
    DevBuf wider;
    int rc = rh_reserve(ctx, wider, bytes + bytes / 2);
    if (rc) return rc;
    RH_HIP(ctx, hipMemcpyAsync(wider.p, b.p, keep, hipMemcpyDeviceToDevice, ctx->stream));
    RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    rh_release(ctx, b);
    b.p = wider.p; b.cap = wider.cap;
    wider.p = nullptr; wider.cap = 0;
    return REAL_HIP_OK;
}

int rh_indel_begin(real_hip_ctx *ctx)
{
    static_assert(sizeof(real_hip_indel) == 32 && offsetof(real_hip_indel, qsum) == 16 && offsetof(real_hip_indel, seq) == 24 &&
                      offsetof(real_hip_indel, gap) == 28 && offsetof(real_hip_indel, gt) == 29 && offsetof(real_hip_indel, gq) == 30 &&
                      offsetof(real_hip_indel, ref) == 31,
                  "an indel record is two 16-byte stores");
    static_assert(REAL_HIP_GAP_MAX == 16u, "S fills a u32 exactly");
    RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    rh_indel_release(ctx);
    RhIndelStage &S = ctx->indel;
    int rc;
    if ((rc = rh_stats_reserve(ctx, S.stage.stats, RH_PAIR_STRIPES, 0))) return rc;
    if ((rc = rh_reserve(ctx, S.fin, (size_t)RH_PAIR_STRIPES * 16 * 8)) || (rc = rh_reserve(ctx, S.count, 8))) return rc;
    RH_HIP(ctx, hipMemsetAsync(S.count.p, 0, 8, ctx->stream));
    RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    S.state = 1;
    return REAL_HIP_OK;
}

int rh_indel_add(real_hip_ctx *ctx, const DevBatch &b1, const DevBatch &b2, const real_hip_gap_place *d_gaps, uint64_t n)
{
    if (!n) return REAL_HIP_OK;
    RhIndelStage &S = ctx->indel;
    int rc;
    if ((rc = rh_stats_reserve(ctx, S.stage.stats, RH_PAIR_STRIPES, 0))) return rc;
    // the worst case of this call: one event per fragment
    if ((rc = indel_grow(ctx, S.ev, (size_t)S.n_ev * 16, (size_t)(S.n_ev + n) * 16))) return rc;
    IndelAddArgs A;
    memset(&A, 0, sizeof A);
    rh_gap_record_args(A, ctx, b1, b2, d_gaps, n);
    A.min_qual = ctx->pileup.min_qual;
    A.ev = (uint4 *)S.ev.p; A.ev_count = (unsigned long long *)S.count.p;
    A.stats = (unsigned long long *)S.stage.stats.p;
    rh_time_begin(ctx, ctx->stream, S.stage);
    hipLaunchKernelGGL(indel_add_kernel, dim3((unsigned)((n + RH_ID_BLOCK - 1) / RH_ID_BLOCK)), dim3(RH_ID_BLOCK), 0, ctx->stream, A);
    const hipError_t e = hipGetLastError();
    rh_time_end(ctx, ctx->stream);
    if (e != hipSuccess) return rh_fail(ctx, REAL_HIP_E_DEVICE, "indel calls: add", e);
    S.stage.items += n;
    S.stage.launches += 1;
    uint64_t n_ev = 0;
    RH_HIP(ctx, hipMemcpyAsync(&n_ev, S.count.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    S.n_ev = n_ev;
    return REAL_HIP_OK;
}

// sort and group the events: S.table, S.n_groups
static int indel_group(real_hip_ctx *ctx, RhIndelStage &S)
{
    const uint64_t n = S.n_ev;
    S.n_groups = 0;
    if (!n) { S.grouped = true; return REAL_HIP_OK; }
    if (n > 0xffffffffull) return rh_fail(ctx, REAL_HIP_E_UNSUPPORTED, "indel calls: more than 2^32 events", hipSuccess);
    const uint64_t blocks = (n + RH_ID_BLOCK - 1) / RH_ID_BLOCK;
    int rc;
    if ((rc = rh_reserve(ctx, S.ev2, (size_t)n * 16)) || (rc = rh_reserve(ctx, S.key[0], (size_t)n * 8)) || (rc = rh_reserve(ctx, S.key[1], (size_t)n * 8)) ||
        (rc = rh_reserve(ctx, S.blk, (size_t)(blocks + 1) * 16)))
        return rc;
    uint4 *ev = (uint4 *)S.ev.p, *ev2 = (uint4 *)S.ev2.p;
    uint64_t *k0 = (uint64_t *)S.key[0].p, *k1 = (uint64_t *)S.key[1].p, *blk = (uint64_t *)S.blk.p, *blk_off = blk + blocks + 1;
    size_t t0 = 0, t1 = 0, t2 = 0;
    RH_HIP(ctx, rocprim::radix_sort_pairs(nullptr, t0, k0, k1, ev, ev2, (size_t)n, 0u, 32u, ctx->stream));
    RH_HIP(ctx, rocprim::radix_sort_pairs(nullptr, t1, k0, k1, ev2, ev, (size_t)n, 0u, 40u, ctx->stream));
    RH_HIP(ctx, rocprim::exclusive_scan(nullptr, t2, blk, blk_off, (uint64_t)0, (size_t)(blocks + 1), rocprim::plus<uint64_t>(), ctx->stream));
    const size_t tmp = std::max(std::max(t0, t1), std::max(t2, (size_t)8));
    if ((rc = rh_reserve(ctx, ctx->sort_tmp, tmp))) return rc;
    const dim3 grid((unsigned)blocks), block(RH_ID_BLOCK);
    rh_time_begin(ctx, ctx->stream, S.stage); // (no return inside the bracket: a failing step is reported behind rh_time_end)
    hipLaunchKernelGGL(indel_key_kernel<0>, grid, block, 0, ctx->stream, ev, n, k0);
    hipError_t e = hipGetLastError();
    size_t t = tmp;
    if (e == hipSuccess) e = rocprim::radix_sort_pairs(ctx->sort_tmp.p, t, k0, k1, ev, ev2, (size_t)n, 0u, 32u, ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(indel_key_kernel<1>, grid, block, 0, ctx->stream, ev2, n, k0);
        e = hipGetLastError();
    }
    t = tmp;
    if (e == hipSuccess) e = rocprim::radix_sort_pairs(ctx->sort_tmp.p, t, k0, k1, ev2, ev, (size_t)n, 0u, 40u, ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(indel_heads_kernel<false>, grid, block, 0, ctx->stream, ev, n, blk, blk_off, (uint32_t *)nullptr, (uint64_t)0);
        e = hipGetLastError();
    }
    t = tmp;
    if (e == hipSuccess) e = rocprim::exclusive_scan(ctx->sort_tmp.p, t, blk, blk_off, (uint64_t)0, (size_t)(blocks + 1), rocprim::plus<uint64_t>(), ctx->stream);
    rh_time_end(ctx, ctx->stream);
    if (e != hipSuccess) return rh_fail(ctx, REAL_HIP_E_DEVICE, "indel calls: sort of the events / count of the groups", e);
    S.stage.launches += 6;
    uint64_t groups = 0;
    RH_HIP(ctx, hipMemcpyAsync(&groups, blk_off + blocks, 8, hipMemcpyDeviceToHost, ctx->stream));
    RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if ((rc = rh_reserve(ctx, S.starts, (size_t)(groups + 1) * 4)) || (rc = rh_reserve(ctx, S.table, (size_t)groups * sizeof(real_hip_indel))) ||
        (rc = rh_reserve(ctx, S.events, (size_t)groups * sizeof(real_hip_indel))))
        return rc;
    IndelGroupArgs G;
    G.t = rh_dev_text(ctx, ctx->fileid);
    G.ev = ev; G.starts = (const uint32_t *)S.starts.p; G.n_groups = groups;
    G.depth = (const uint32_t *)ctx->pileup.diff.p; // (scanned in place by the pileup's finish)
    G.gdepth = rh_pileup_gapped_array(ctx);
    G.table = (uint4 *)S.table.p;
    rh_time_begin(ctx, ctx->stream, S.stage);
    hipLaunchKernelGGL(indel_heads_kernel<true>, grid, block, 0, ctx->stream, ev, n, blk, blk_off, (uint32_t *)S.starts.p, groups);
    e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(indel_group_kernel, dim3((unsigned)((groups + RH_ID_BLOCK - 1) / RH_ID_BLOCK)), block, 0, ctx->stream, G);
        e = hipGetLastError();
    }
    rh_time_end(ctx, ctx->stream);
    if (e != hipSuccess) return rh_fail(ctx, REAL_HIP_E_DEVICE, "indel calls: the groups", e);
    S.stage.launches += 2;
    S.n_groups = groups;
    S.grouped = true;
    return REAL_HIP_OK;
}

int rh_indel_finish(real_hip_ctx *ctx, const real_hip_indel_params &p, uint64_t *n_events, uint64_t *n_calls)
{
    RhIndelStage &S = ctx->indel;
    int rc;
    S.n_calls = S.het = S.hom = S.dels = S.ins = 0;
    if (!S.grouped && (rc = indel_group(ctx, S))) return rc;
    const uint64_t groups = S.n_groups;
    if (n_events) *n_events = groups;
    if (n_calls) *n_calls = 0;
    if (!groups) { S.state = 2; return REAL_HIP_OK; } // (no kernel over an empty table)
    const uint64_t blocks = (groups + RH_ID_BLOCK - 1) / RH_ID_BLOCK;
    if ((rc = rh_reserve(ctx, S.blk, (size_t)(blocks + 1) * 16))) return rc;
    uint64_t *blk = (uint64_t *)S.blk.p, *blk_off = blk + blocks + 1;
    size_t tmp = 0;
    RH_HIP(ctx, rocprim::exclusive_scan(nullptr, tmp, blk, blk_off, (uint64_t)0, (size_t)(blocks + 1), rocprim::plus<uint64_t>(), ctx->stream));
    if ((rc = rh_reserve(ctx, ctx->sort_tmp, tmp ? tmp : 8))) return rc;
    RH_HIP(ctx, hipMemsetAsync(S.fin.p, 0, (size_t)RH_PAIR_STRIPES * 16 * 8, ctx->stream));
    IndelCallArgs F;
    F.table = (const uint4 *)S.table.p; F.n_groups = groups;
    F.min_call_qual = p.min_call_qual; F.min_alt = p.min_alt; F.min_depth = p.min_depth;
    F.events = (uint4 *)S.events.p; F.blk = blk; F.blk_off = blk_off; F.calls = nullptr; F.cap = 0;
    F.fin = (unsigned long long *)S.fin.p;
    rh_time_begin(ctx, ctx->stream, S.stage); // (no return inside the bracket)
    hipLaunchKernelGGL(indel_calls_kernel<false>, dim3((unsigned)blocks), dim3(RH_ID_BLOCK), 0, ctx->stream, F);
    hipError_t e = hipGetLastError();
    size_t t = tmp;
    if (e == hipSuccess) e = rocprim::exclusive_scan(ctx->sort_tmp.p, t, blk, blk_off, (uint64_t)0, (size_t)(blocks + 1), rocprim::plus<uint64_t>(), ctx->stream);
    rh_time_end(ctx, ctx->stream);
    if (e != hipSuccess) return rh_fail(ctx, REAL_HIP_E_DEVICE, "indel calls: count of the calls / scan of the block counts", e);
    S.stage.launches += 2;
    uint64_t total = 0;
    std::vector<uint64_t> fin((size_t)RH_PAIR_STRIPES * 16);
    RH_HIP(ctx, hipMemcpyAsync(&total, blk_off + blocks, 8, hipMemcpyDeviceToHost, ctx->stream));
    RH_HIP(ctx, hipMemcpyAsync(fin.data(), S.fin.p, fin.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t sum[4] = {0, 0, 0, 0};
    for (size_t s = 0; s < RH_PAIR_STRIPES; ++s)
        for (int k = 0; k < 4; ++k) sum[k] += fin[s * 16 + k];
    if (total) {
        if ((rc = rh_reserve(ctx, S.calls, (size_t)total * sizeof(real_hip_indel)))) return rc;
        F.calls = (uint4 *)S.calls.p; F.cap = total;
        rh_time_begin(ctx, ctx->stream, S.stage);
        hipLaunchKernelGGL(indel_calls_kernel<true>, dim3((unsigned)blocks), dim3(RH_ID_BLOCK), 0, ctx->stream, F);
        rh_time_end(ctx, ctx->stream);
        RH_HIP(ctx, hipGetLastError());
        S.stage.launches += 1;
        RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    rh_time_resolve(ctx);
    S.n_calls = total; S.het = sum[0]; S.hom = sum[1]; S.dels = sum[2]; S.ins = sum[3];
    S.state = 2;
    if (n_calls) *n_calls = total;
    return REAL_HIP_OK;
}

int rh_indel_stats(real_hip_ctx *ctx, real_hip_indel_stats *out, int reset)
{
    uint64_t h[9];
    RhStageCount was;
    RhIndelStage &S = ctx->indel;
    int rc;
    if ((rc = rh_stage_read(ctx, S.stage, RH_PAIR_STRIPES, 9, reset, h, was))) return rc;
    if (out) {
        out->reserved = 0;
        out->fragments = was.items; out->placed = h[0]; out->events = h[1]; out->other_file = h[2]; out->invalid = h[3]; out->ungapped = h[4];
        out->on_n = h[5]; out->low_qual = h[6]; out->shifted = h[7]; out->shift_capped = h[8];
        const bool done = S.state == 2;
        out->distinct = done ? S.n_groups : 0; out->calls = S.n_calls; out->het = S.het; out->hom = S.hom; out->deletions = S.dels; out->insertions = S.ins;
        out->launches = was.launches; out->kernel_ms = was.kernel_ms;
    }
    return REAL_HIP_OK;
}
