// read_walk.h -- from a final record to a placement on the resident text (placed_read; placed_gap for a gap record), and a
// lane's walk of the placed read word by word against the 2-bit text: what pileup.hip (counts per text position), snp_call.hip
// (evidence per site), mismatch_list.hip (the list of one read) and the stages of the gapped placements (gapped_list.hip,
// indel_call.hip, pileup_gapped.hip) share.  32 bases per step, whatever the length (up to REAL_HIP_MAX_PATL_LONG):
// no register array of the read.  No LDS, no scratch memory.
#pragma once
#include "match_common.h"
#include "stage_common.h"
#include "real_hip_ctx.h" // rh_gap_record_args

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
    // the nb <= 32 bases of the ORIENTED read from its offset r on (r + nb <= L), whatever r is: forward the read's bases
    // r .. r + nb - 1, turned round the reverse complement of its bases L - r - nb .. L - r - 1
    static __device__ __forceinline__ uint64_t oriented_from(const DevBatch &b, uint64_t start, uint32_t L, bool inv, uint32_t r, uint32_t nb)
    {
        const uint64_t s = start + (inv ? L - r - nb : r);
        uint64_t w, o;
        if (b.packed) pack_read_packed<1>(DwordRow{b.bases + (s >> 2)}, nb, (uint32_t)(s & 3u), &w);
        else (void)pack_read<1>(DwordRow{b.bases + s}, nb, &w);
        if (inv) revcomp_words<1>(&w, &o, nb); else o = w;
        return o;
    }
    // word j of the oriented read alone (step's `o` and `nb`): what a caller takes that needs no text (snp_call.hip)
    static __device__ __forceinline__ uint64_t oriented(const DevBatch &b, uint64_t start, uint32_t L, bool inv, uint32_t j, uint32_t &nb)
    {
        nb = min(32u, L - 32u * j);
        return oriented_from(b, start, L, inv, 32u * j, nb);
    }
    // word j of the text alone (step's `al`), j ascending from 0
    __device__ __forceinline__ uint64_t text_step(uint32_t j)
    {
        const uint64_t t1 = text[wi + j + 1]; // (the text is padded behind its end)
        const uint64_t al = sh ? ((t0 << sh) | (t1 >> (64 - sh))) : t0;
        t0 = t1;
        return al;
    }
    // word j of a SEGMENT: `len` bases of the oriented read from its offset r0 on, aligned with the len text positions
    // begin() was given (gapped_list.hip: the two diagonals of a gapped placement start at arbitrary read and text offsets)
    __device__ __forceinline__ uint64_t step_from(const DevBatch &b, uint64_t start, uint32_t L, bool inv, uint32_t r0, uint32_t len, uint32_t j,
                                                  uint32_t &nb, uint64_t &al, uint64_t &o)
    {
        nb = min(32u, len - 32u * j);
        o = oriented_from(b, start, L, inv, r0 + 32u * j, nb);
        al = text_step(j);
        const uint64_t x = al ^ o;
        uint64_t flags = ((x >> 1) | x) & M55;
        if (nb < 32) flags &= ~0ull << (64 - 2 * nb);
        return flags;
    }
    __device__ __forceinline__ uint64_t step(const DevBatch &b, uint64_t start, uint32_t L, bool inv, uint32_t j, uint32_t &nb, uint64_t &al,
                                             uint64_t &o)
    {
        return step_from(b, start, L, inv, 0u, L, j, nb, al, o);
    }
};

// the text's N bits of the 32 positions from x on, as flags: position x + u at bit 62 - 2u
static __device__ __forceinline__ uint64_t mm_n_flags(const uint64_t *__restrict__ wild, uint64_t x)
{
    const uint64_t w = x >> 6;
    const uint32_t s = (uint32_t)(x & 63u);
    uint64_t v = wild[w] << s;
    if (s > 32) v |= wild[w + 1] >> (64 - s); // (the vector is padded behind its end)
    v >>= 32; // bit 31 - u = position x + u; now every bit to twice its place
    v = (v | (v << 16)) & 0x0000ffff0000ffffull;
    v = (v | (v << 8)) & 0x00ff00ff00ff00ffull;
    v = (v | (v << 4)) & 0x0f0f0f0f0f0f0f0full;
    v = (v | (v << 2)) & 0x3333333333333333ull;
    v = (v | (v << 1)) & M55;
    return v;
}

// where a read starts in its batch and how long it is; 0xffffffff for a read of a ragged batch whose offsets run backwards or
// span more than REAL_HIP_MAX_PATL_LONG (no placement of it fits any text)
static __device__ __forceinline__ uint32_t read_extent(const DevBatch &b, uint64_t i, uint64_t &start)
{
    if (!b.off) { start = i * (uint64_t)b.upatl; return b.upatl; }
    start = b.off[i];
    const uint64_t e = b.off[i + 1];
    return e >= start && e - start <= REAL_HIP_MAX_PATL_LONG ? (uint32_t)(e - start) : 0xffffffffu;
}

static_assert(RH_INFO_ST_SHIFT == ST_SHIFT && RH_INFO_ER_SHIFT == ER_SHIFT && RH_INFO_FI_SHIFT == FI_SHIFT && RH_INFO_POS_MASK == POS_MASK &&
                  RH_INFO_STRAIGHT == ST_STRAIGHT && RH_INFO_REVERSE == ST_REVERSE,
              "final_record.h reads the info word the matcher writes");

// Record i of a launch as a placement on the text t, the one step from a record to a placement: single-end
// records `info`, or mate `mate` (0 = mate 1, 1 = mate 2) of the real_hip_pair records `pairs`, read as five 8-byte words, and
// -- where the pair's state is NoMatch and `singles` is not null -- the mate's own real_hip_single (a NonUnique pair places
// nothing).  A record of another state places nothing; then one of another file id is flagged `other`; then one that ends
// behind the text `bad`: one 64-bit comparison, which also catches the positions of an info word beyond 32 bits (t.n is
// below 2^32: real_hip_set_text* refuse a longer text).  The same records are skipped and counted in every stage.
struct PlacedRead {
    bool place, inv;   // a placement; on the reverse strand
    bool other, bad;   // no placement: a record of another file; one that ends behind the text
    uint32_t p, L;     // text position, length
    uint32_t k;        // the record's mismatch count
    uint64_t start;    // first base in the batch
};
template <bool PAIRS>
static __device__ __forceinline__ PlacedRead placed_read(const DevText &t, const DevBatch &b, const uint64_t *info, const uint2 *pairs,
                                                         const uint4 *singles, uint32_t mate, uint64_t i)
{
    RhPlace c;
    if (PAIRS) {
        const uint2 pos = pairs[i * 5 + 2], tail = pairs[i * 5 + 4];
        uint32_t state;
        c = rh_place_pair(pos.x, pos.y, tail.x, tail.y, mate, &state);
        if (state == REAL_HIP_PAIR_NOMATCH && singles) { const uint4 s = singles[i]; c = rh_place_single(s.z, s.w); }
    } else {
        c = rh_place_info(info[i]);
    }
    PlacedRead r;
    r.inv = c.inv; r.k = c.k; r.p = (uint32_t)c.pos;
    r.other = c.place && c.file != t.fileid;
    r.place = c.place && !r.other;
    r.bad = false;
    r.start = 0; r.L = 0;
    if (r.place) {
        r.L = read_extent(b, i, r.start);
        if (c.pos + r.L > t.n) { r.place = false; r.bad = true; }
    }
    return r;
}

// ---- gap records ------------------------------------------------------------------------------------------------
// what every stage that consumes real_hip_gap_place records is launched with: the text, the two mates' reads, the records
struct GapRecordArgs {
    DevText  t;
    DevBatch b[2];                 // the mates' reads
    const uint4 *gaps;             // real_hip_gap_place records (final_record.h names the words)
    uint64_t n;                    // fragments
    // the reads of mate 2 iff `second` (two copies and a select: an index chosen by the lane would be scratch memory)
    __device__ __forceinline__ DevBatch mate(uint32_t second) const
    {
        DevBatch m = b[0];
        if (second) m = b[1];
        return m;
    }
};
// the stage decides which of them drops the qualities
static inline void rh_gap_record_args(GapRecordArgs &A, const real_hip_ctx *ctx, const DevBatch &b1, const DevBatch &b2, const real_hip_gap_place *d_gaps,
                                      uint64_t n)
{
    A.t = rh_dev_text(ctx, ctx->fileid);
    A.b[0] = b1; A.b[1] = b2;
    A.gaps = (const uint4 *)d_gaps;
    A.n = n;
}

// Fragment i's gap record as a placement on the text A.t, the one step from a gap record to a placement: one 16-byte load; a
// record that is not Unique places nothing; then one of another file id is `other`; then one that does not FIT (final_record.h,
// rh_gap_fit) is `bad`.  Nothing but the record and the read's offsets is read: every check comes before the first byte of read
// or text is touched.  The same records are skipped and counted in every stage.
// A gapped placement is two diagonals joined at the split, and this is the one place that says where they lie: the first is
// read[0, len1()) on text[p, ..), the second read[r2(), r2() + len2()) on text[p + t2(), ..); the del text positions from
// p + len1() on are covered by nothing.  Without a gap the first is the whole read and the second is empty.
struct PlacedGap {
    uint32_t place, inv, other, bad; // flags, a register each
    uint32_t second;   // the target is mate 2
    uint32_t p, L, j;  // text position, length, split
    uint32_t d, del;   // inserted read bases, deleted text positions
    uint32_t frag, k;  // the record's fragment of the text and mismatch count
    uint64_t start;    // first base in the target's batch
    __device__ __forceinline__ uint32_t gapped() const { return d | del; }
    __device__ __forceinline__ uint32_t len1() const { return gapped() ? j : L; }
    __device__ __forceinline__ uint32_t r2() const { return j + d; }
    __device__ __forceinline__ uint32_t t2() const { return j + del; }
    __device__ __forceinline__ uint32_t len2() const { return gapped() ? L - j - d : 0u; } // (>= 1 with a gap: the record fits)
};
static __device__ __forceinline__ PlacedGap placed_gap(const GapRecordArgs &A, uint64_t i)
{
    PlacedGap c;
    c.place = c.inv = c.other = c.bad = c.second = 0;
    c.p = c.L = c.j = c.d = c.del = c.frag = c.k = 0;
    c.start = 0;
    const uint4 w = A.gaps[i];
    const RhGapRecord r = rh_place_gap(w.x, w.y, w.z, w.w);
    if (r.state != REAL_HIP_PAIR_UNIQUE) return c;
    if (r.file != A.t.fileid) { c.other = 1; return c; }
    c.second = r.target; c.inv = r.inv; c.frag = r.frag; c.k = r.k;
    c.p = r.p; c.j = r.j;
    uint64_t start;
    c.L = read_extent(A.mate(c.second), i, start); // (0xffffffff: offsets that run backwards, or longer than any read)
    c.start = start;
    const RhGapFit f = rh_gap_fit(c.L, r.g, r.j, r.p, A.t.n);
    c.d = f.d; c.del = f.del;
    c.place = f.fits; c.bad = 1u - f.fits;
    return c;
}
