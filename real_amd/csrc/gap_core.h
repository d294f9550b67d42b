// gap_core.h -- the device functions the two gapped placement stages share (gap_rescue.hip: inside the window of a placed mate;
// gap_anchor.hip: around the anchors of a single read): a read's span in its batch, whether a base of the oriented read differs
// from the staged text, the three numbers of a diagonal, and the packing of a real_hip_gap_place record.  One copy, so that a
// candidate costs the same in both stages.
#pragma once
#include "read_words.h"

#include "final_record.h" // the layout of a gap record, asserted there

// real_hip_gap_place as a uint4: x pos, y frag:16 | fileid:8 | tag:8, z split:16 | gap:8 | k:8, w cost:16 | second:16
static __device__ __forceinline__ uint4 gap_empty_record() { return make_uint4(0u, 0u, 0u, (uint32_t)REAL_HIP_GAP_NONE << 16); }
static __device__ __forceinline__ uint4 gap_pack_record(uint32_t pos, uint32_t frag, uint32_t fileid, uint32_t tag, uint32_t split, int32_t g, uint32_t k,
                                                        uint32_t cost, uint32_t second)
{
    return make_uint4(pos, frag | (fileid << 16) | (tag << 24), split | (((uint32_t)g & 0xffu) << 16) | (k << 24), cost | (second << 16));
}
// length and first base of read i of a batch
static __device__ __forceinline__ uint64_t gap_read_span(const DevBatch &b, uint64_t i, uint64_t *o0)
{
    *o0 = b.off ? b.off[i] : i * (uint64_t)b.upatl;
    return b.off ? (b.off[i + 1] >= *o0 ? b.off[i + 1] - *o0 : 0) : (uint64_t)b.upatl;
}

// does base i of the oriented read R differ from the staged text at base trel + i
static __device__ __forceinline__ uint32_t gap_mm(const uint64_t *R, const uint64_t *sT, uint32_t trel, uint32_t i)
{
    const uint32_t u = trel + i;
    return (((R[i >> 5] >> (62u - 2u * (i & 31u))) ^ (sT[u >> 5] >> (62u - 2u * (u & 31u)))) & 3ull) ? 1u : 0u;
}
// the diagonal at staged base trel: total:16 | head:8 | tail:8 = the mismatches of the whole read, of its first m and of its
// last m bases (m < 256: a read of at most REAL_HIP_MAX_PATL bases holds two flanks and a gap)
static __device__ __forceinline__ uint32_t gap_diagonal(const uint64_t *R, const uint64_t *sT, uint32_t trel, uint32_t L, uint32_t m)
{
    const uint32_t nw = (L + 31u) >> 5, wi = trel >> 5, sh = 2u * (trel & 31u);
    uint32_t total = 0, head = 0, tail = 0;
    uint64_t t0 = sT[wi];
    for (uint32_t j = 0; j < nw; ++j) {
        const uint64_t t1 = sT[wi + j + 1];
        const uint64_t al = sh ? ((t0 << sh) | (t1 >> (64u - sh))) : t0;
        const uint64_t xw = al ^ R[j];
        uint64_t d = ((xw >> 1) | xw) & M55;
        const uint32_t nb = min(32u, L - 32u * j);                // bases of this word
        if (nb < 32u) d &= ~0ull << (64u - 2u * nb);
        const uint32_t nh = m > 32u * j ? min(32u, m - 32u * j) : 0u;                // of them in the first m of the read
        const uint32_t lt = L - m > 32u * j ? min(32u, L - m - 32u * j) : 0u;        // of them in front of the last m
        total += __popcll(d);
        if (nh) head += __popcll(d & (~0ull << (64u - 2u * nh)));
        if (lt < 32u) tail += __popcll(d & (~0ull >> (2u * lt)));
        t0 = t1;
    }
    return (total << 16) | (head << 8) | tail;
}
// The fewest mismatches of a gapped alignment of the read on the pair of diagonals prel (prefix) and qrel (suffix, the staged
// base of diagonal p + g), over the allowed split points, left to right: c = mismatches of R[0..j) on p + those of R[j+d..L) on
// p + g, one base a step, the base that joins the prefix added and the one that leaves the suffix taken off; the leftmost
// minimum is kept.  head: the first m bases of p; qtotal: the whole of q; d: the read bases an insertion leaves unaligned
static __device__ __forceinline__ uint32_t gap_best_split(const uint64_t *R, const uint64_t *sT, uint32_t prel, uint32_t qrel, uint32_t L, uint32_t m,
                                                          uint32_t d, uint32_t head, uint32_t qtotal, uint32_t *bj)
{
    const uint32_t jhi = L - m - d;
    uint32_t c = qtotal;
    for (uint32_t x = 0; x < m + d; ++x) c -= gap_mm(R, sT, qrel, x);
    c += head;
    uint32_t k = c;
    *bj = m;
    for (uint32_t j = m; j < jhi; ++j) {
        c += gap_mm(R, sT, prel, j);
        c -= gap_mm(R, sT, qrel, j + d);
        if (c < k) { k = c; *bj = j + 1; }
    }
    return k;
}
