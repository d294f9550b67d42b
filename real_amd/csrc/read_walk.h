// read_walk.h -- a lane walks one placed read word by word against the 2-bit text: what pileup.hip (counts per text position)
// and mismatch_list.hip (the list of one read) share.  32 bases per step, whatever the length (up to
// REAL_HIP_MAX_PATL_LONG): no register array of the read.  No LDS, no scratch memory.
#pragma once
#include "match_common.h"

// a read's bytes in place, a dword per request: the aligned dword that holds the first byte asked for and, where the request
// straddles it and the row goes on, the next one.  Never a dword without a byte of the row in it (an aligned dword does not
// cross a page, so nothing outside the caller's allocation's pages is touched); bytes behind the row's end come back as
// whatever lies there, and pack_read / pack_read_packed mask them off.
struct DwordRow {
    const uint8_t *row;
    __device__ __forceinline__ uint32_t dword(int byteoff, uint32_t nbytes) const
    {
        if (byteoff < 0 || (uint32_t)byteoff >= nbytes) return 0;
        const uintptr_t a = (uintptr_t)(row + byteoff);
        const uint32_t mis = (uint32_t)(a & 3u);
        const uint32_t *p = reinterpret_cast<const uint32_t *>(a - mis);
        const uint32_t lo = p[0];
        uint32_t hi = 0;
        if (mis && (uint32_t)byteoff + (4u - mis) < nbytes) hi = p[1];
        return __builtin_amdgcn_alignbyte(hi, lo, mis);
    }
};

// The walk of a read of L bases that starts at base `start` of the batch and lies at text position p (p + L <= n), reverse
// strand iff inv.  step(j) is word j = the text positions p + 32j .. p + 32j + nb - 1, j ascending from 0:
//   al     the text there, funnel-shifted to the placement (base u of the word at bits 63 - 2u, 62 - 2u)
//   o      the ORIENTED read there: read[32j ..] forward, read[L - 32j - nb ..] turned round with revcomp_words
//   return one flag per base that differs, base u at bit 62 - 2u; nothing behind the read's end
struct ReadWalk {
    const uint64_t *text;
    uint64_t wi, t0;
    uint32_t sh;
    __device__ __forceinline__ void begin(const uint64_t *T, uint32_t p, uint32_t L)
    {
        text = T; wi = p >> 5; sh = 2u * (p & 31u);
        t0 = L ? T[wi] : 0;
    }
    // word j of the oriented read alone (step's `o` and `nb`): what a caller takes that needs no text (snp_call.hip)
    static __device__ __forceinline__ uint64_t oriented(const DevBatch &b, uint64_t start, uint32_t L, bool inv, uint32_t j, uint32_t &nb)
    {
        nb = min(32u, L - 32u * j);
        const uint64_t s = start + (inv ? L - 32u * j - nb : 32u * j);
        uint64_t w, o;
        if (b.packed) pack_read_packed<1>(DwordRow{b.bases + (s >> 2)}, nb, (uint32_t)(s & 3u), &w);
        else (void)pack_read<1>(DwordRow{b.bases + s}, nb, &w);
        if (inv) revcomp_words<1>(&w, &o, nb); else o = w;
        return o;
    }
    __device__ __forceinline__ uint64_t step(const DevBatch &b, uint64_t start, uint32_t L, bool inv, uint32_t j, uint32_t &nb, uint64_t &al,
                                             uint64_t &o)
    {
        o = oriented(b, start, L, inv, j, nb);
        const uint64_t t1 = text[wi + j + 1]; // (the text is padded behind its end)
        al = sh ? ((t0 << sh) | (t1 >> (64 - sh))) : t0;
        t0 = t1;
        const uint64_t x = al ^ o;
        uint64_t flags = ((x >> 1) | x) & M55;
        if (nb < 32) flags &= ~0ull << (64 - 2 * nb);
        return flags;
    }
};

// where a read starts in its batch and how long it is; 0xffffffff for a read of a ragged batch whose offsets run backwards or
// span more than REAL_HIP_MAX_PATL_LONG (no placement of it fits any text)
static __device__ __forceinline__ uint32_t read_extent(const DevBatch &b, uint64_t i, uint64_t &start)
{
    if (!b.off) { start = i * (uint64_t)b.upatl; return b.upatl; }
    start = b.off[i];
    const uint64_t e = b.off[i + 1];
    return e >= start && e - start <= REAL_HIP_MAX_PATL_LONG ? (uint32_t)(e - start) : 0xffffffffu;
}

// Record i of a launch as a placement on the text t: single-end records `info`, or mate `mate` (0 = mate 1, 1 = mate 2) of the
// real_hip_pair records `pairs`, read as five 8-byte words (insert_hist.hip).  A record of another state places nothing; then
// one of another file id is flagged `other`; then one that ends behind the text (or holds more than 32 bits of position)
// `bad`.  What pileup.hip and snp_call.hip share: the same records are skipped and counted in both.
struct PlacedRead {
    bool place, inv;   // a placement; on the reverse strand
    bool other, bad;   // no placement: a record of another file; one that ends behind the text
    uint32_t p, L;     // text position, length
    uint64_t start;    // first base in the batch
};
template <bool PAIRS>
static __device__ __forceinline__ PlacedRead placed_read(const DevText &t, const DevBatch &b, const uint64_t *info, const uint2 *pairs, uint32_t mate,
                                                         uint64_t i)
{
    PlacedRead r;
    uint32_t file;
    r.other = r.bad = false;
    if (PAIRS) {
        const uint2 pos = pairs[i * 5 + 2], tail = pairs[i * 5 + 4];
        r.place = ((tail.y >> 16) & 0xffu) == REAL_HIP_PAIR_UNIQUE;
        r.inv = (((tail.y >> 8) & 0xffu) != 0) != (mate != 0); // mate 2 has the other strand
        file = (tail.x >> 16) & 0xffu;
        r.p = mate ? pos.y : pos.x;
    } else {
        const uint64_t rec = info[i];
        const uint32_t st = (uint32_t)(rec >> ST_SHIFT);
        r.place = st == ST_STRAIGHT || st == ST_REVERSE;
        r.inv = st == ST_REVERSE;
        file = (uint32_t)(rec >> FI_SHIFT) & 63u;
        const uint64_t p64 = rec & POS_MASK;
        r.p = (uint32_t)p64;
        if (r.place && file == t.fileid && p64 > 0xffffffffull) { r.place = false; r.bad = true; } // (35 bits of position, 32 of text)
    }
    if (r.place && file != t.fileid) { r.place = false; r.other = true; }
    r.start = 0; r.L = 0;
    if (r.place) {
        r.L = read_extent(b, i, r.start);
        if ((uint64_t)r.p + r.L > t.n) { r.place = false; r.bad = true; }
    }
    return r;
}
