// complex_walk.h -- the pure parts of the paired driver's deferred walk over the overflow entries of complex rows
// (match_rows_paired): the descriptor of one key group whose walk is put off, the header of a complex row judged for both
// key groups at once, and the mapping of a flat slot number to (descriptor, entry).  No HIP in here (as row_bytes.h):
// tests/test_complex_walk_cpu.py compiles it with the host compiler and compares it with plain loops.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define RH_HD __host__ __device__
#else
#define RH_HD
#endif

// A descriptor is two words: the index of the group's first entry in the table's overflow array, and
//   owner lane : 6 | entries - 1 : 6 | table : 2 | list : 3 | strand : 1
// (a group that is walked by a lane has 1 .. 48 entries; the field holds up to 64).  The partner key is not carried: it is
// the owner's signature of list 5 - list on that strand.
#define CW_MAX_DESC 64u  // descriptors the flat mapping is made for (one per lane builds the prefix sums)
#define CW_NONE 0xffffffffu // no descriptor: a flat slot behind the last entry
static inline RH_HD uint32_t cw_pack(uint32_t lane, uint32_t cnt, uint32_t table, uint32_t list, uint32_t strand)
{
    return lane | ((cnt - 1u) << 6) | (table << 12) | (list << 14) | (strand << 17);
}
static inline RH_HD uint32_t cw_lane(uint32_t m) { return m & 63u; }
static inline RH_HD uint32_t cw_cnt(uint32_t m) { return ((m >> 6) & 63u) + 1u; }
static inline RH_HD uint32_t cw_table(uint32_t m) { return (m >> 12) & 3u; }
static inline RH_HD uint32_t cw_list(uint32_t m) { return (m >> 14) & 7u; }
static inline RH_HD uint32_t cw_strand(uint32_t m) { return (m >> 17) & 1u; }

// the sum of the four bytes of x, added to acc
static inline RH_HD uint32_t cw_byte_sum(uint32_t x, uint32_t acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sad_u8(x, 0u, acc);
#else
    return acc + (x & 255u) + ((x >> 8) & 255u) + ((x >> 16) & 255u) + (x >> 24);
#endif
}

// The header of a complex row holds sixteen 8-bit group counts in four words (group 0 in the low byte of w[0]).  For key
// group g: off = the sum of the counts in front of it, cnt = its own, sat = one of the counts 0 .. g is 255 -- a saturated
// count, so that off and cnt are no bounds and the caller finds them by binary search (key_group_range).
struct CwGroup { uint32_t off, cnt, sat; };
static inline RH_HD void cw_header_word(uint32_t w, int nb, CwGroup &o) // nb = counts of this word in front of the group's
{
    const uint32_t below = nb <= 0 ? 0u : (nb >= 4 ? 0xffffffffu : ((1u << (8 * nb)) - 1u));
    const uint32_t upto = nb < 0 ? 0u : (nb >= 3 ? 0xffffffffu : ((1u << (8 * (nb + 1))) - 1u)); // ... and its own
    o.off = cw_byte_sum(w & below, o.off);
    if (nb >= 0 && nb < 4) o.cnt = (w >> (8 * nb)) & 255u;
    const uint32_t y = ~w | ~upto; // a zero byte = a count of 255 among them
    o.sat |= (y - 0x01010101u) & ~y & 0x80808080u;
}
// both key groups of a row from one pass over the four words (g0 == g1: the same group twice)
static inline RH_HD void cw_header2(const uint32_t (&w)[4], uint32_t g0, uint32_t g1, CwGroup &a, CwGroup &b)
{
    a.off = a.cnt = a.sat = 0u;
    b.off = b.cnt = b.sat = 0u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int q = 0; q < 4; ++q) {
        cw_header_word(w[q], (int)g0 - 4 * q, a);
        cw_header_word(w[q], (int)g1 - 4 * q, b);
    }
}

// The entries of n descriptors, flattened: pre[d] = the entries of the descriptors in front of d (every descriptor has at
// least one, so pre rises strictly).  Flat slot t < pre[n - 1] + cnt[n - 1] is entry t - pre[d] of the descriptor d this
// returns: the last one with pre[d] <= t.  (Six steps for up to CW_MAX_DESC descriptors, no branch on the way; n >= 1.)
static inline RH_HD uint32_t cw_flat_find(const uint32_t *pre, uint32_t n, uint32_t t)
{
    uint32_t d = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t step = CW_MAX_DESC / 2u; step; step >>= 1) {
        const uint32_t c = d + step;
        if (c < n && pre[c] <= t) d = c;
    }
    return d;
}
