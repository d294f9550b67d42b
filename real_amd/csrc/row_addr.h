// row_addr.h -- how a signature finds its bucket row: the mixing bijection and the addressing of the pair tables.
// No HIP in here: libreal_hip.so's translation units get it through real_hip_internal.h, real_amd/host/host_selftest.cpp
// compiles it with the host compiler and checks it exhaustively (tests/test_host_cpp.py).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define RH_HD __host__ __device__
#else
#define RH_HD
#endif

#define RH_MIX32 0x9E3779B1u
#define RH_MIX64 0x9E3779B97F4A7C15ull
static inline RH_HD uint32_t rh_mix32(uint32_t sign, uint32_t l) { return (sign * RH_MIX32) & (l >= 32 ? 0xffffffffu : ((1u << l) - 1u)); }
static inline RH_HD uint64_t rh_mix64(uint64_t sign, uint32_t l) { return (sign * RH_MIX64) & (l >= 64 ? ~0ull : ((1ull << l) - 1ull)); }

// ---- bucket rows that answer both strands (narrow rows, seedl <= 32) ---------------------------------------------------
// The reverse strand's seed is the reverse complement of the forward one, so the signature the reverse strand looks up in
// list 5 - k is the rc-form of the signature the forward strand looks up in list k: rc-form of (a, c) = (rc c, rc a), the
// reverse complement of the signature read as one string of bases.  Every list is placed so that a signature and its
// rc-form meet in ONE row and differ in the `which` bit of the key group alone, bit gbits - 1.  Three kinds of table:
//   own table        wide rows only (seedl > 32; rh_mix64, match_kernel.hip): 2^pb rows, row = mixed >> gbits.
//   pair table       the conjugate lists (0, 5) and (1, 4): the entries of lists 5 and 4 are PLACED by the rc-form of their
//                    signature, and lists 0 / 5 (1 / 4) share one table of 2^(pb+1) rows: the row found with the forward
//                    list-k signature also holds the list 5-k entries the reverse strand asks for.  row = mixed >> (gbits - 1),
//                    which = 0 for lists 0, 1 and 1 for lists 5, 4; the first list's entries precede the second's.
//   canonical table  the self-conjugate lists 2 (m0, m3) and 3 (m1, m2): the reverse strand looks the rc-form up in the SAME
//                    list.  The entries are placed by a canonical index of l - 1 bits that a signature shares with its
//                    rc-form (rh_canon), mixed over l - 1 bits; 2^pb rows, row = mixed >> (gbits - 1), which = the orientation.
//                    A signature that is its own rc-form has one group, which both strands read.
// In all three (table, row, group) <-> (list, signature) is a bijection, a row holds 2^gbits groups with the same mean load,
// and the partner key of an entry stays the plain leading bits of its own partner list.
enum RhTableKind : uint32_t { RH_TABLE_PAIR = 0, RH_TABLE_CANONICAL = 1 };
static inline RH_HD RhTableKind rh_table_kind(uint32_t la) { return (la < 2 || la > 3) ? RH_TABLE_PAIR : RH_TABLE_CANONICAL; }
// the table list la lives in: bkt[table] / ent[table]
static inline RH_HD uint32_t rh_table_of(uint32_t la) { return la > 3 ? 5 - la : la; }
// rows of the table list la lives in (narrow rows)
static inline RH_HD uint64_t rh_table_rows(uint32_t la, uint32_t pb) { return rh_table_kind(la) == RH_TABLE_PAIR ? 2ull << pb : 1ull << pb; }
static inline RH_HD uint32_t rh_sig_rcform(uint32_t sign, uint32_t l)
{
    uint32_t x = sign; // the sixteen 2-bit bases of the word in reverse order, complemented (3 - base)
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0f0f0f0fu) | ((x & 0x0f0f0f0fu) << 4);
    x = ((x >> 8) & 0x00ff00ffu) | ((x & 0x00ff00ffu) << 8);
    x = (x >> 16) | (x << 16);
    return ~x >> (32 - l);
}
// Canonical index of a self-conjugate list's signature.  a = its high half, b = rc(its low half), h2 = l / 2 bits each: the
// rc-form swaps a and b.  With N = 2^h2 and d = (b - a) mod N the pair {(a, b), (b, a)} is named by its member with
// d <= N/2: index = x << (h2 - 1) | dslot, l - 1 bits,
//   0 < d < N/2   (a, d), which 0          d > N/2   (b, N - d), which 1          d = N/2   (min(a, b), 0), which = a > b
//   d = 0 (the signature is its own rc-form: no partner)   (N/2 + a mod N/2, 0), which = the top bit of a
// -- the x of the d = N/2 class is below N/2 (one of a, a + N/2 is), so the two classes with dslot 0 share the 2^h2 values of x.
struct RhCanon { uint32_t index, which; bool self; };
static inline RH_HD RhCanon rh_canon(uint32_t a, uint32_t b, uint32_t h2)
{
    const uint32_t half = 1u << (h2 - 1), d = (b - a) & (2u * half - 1u);
    const bool self = d == 0, swap = d > half || (d == half && a > b);
    const uint32_t x = self ? (half | (a & (half - 1u))) : (swap ? b : a);
    const uint32_t ds = (swap ? 2u * half - d : d) & (half - 1u); // (d = N/2: slot 0)
    return {(x << (h2 - 1)) | ds, self ? a >> (h2 - 1) : (swap ? 1u : 0u), self};
}
static inline RH_HD RhCanon rh_sig_canon(uint32_t sign, uint32_t l)
{
    const uint32_t h2 = l >> 1;
    return rh_canon(sign >> h2, rh_sig_rcform(sign & ((1u << h2) - 1u), h2), h2);
}
// where the equal range of signature `sign` of list la lies: bkt[table] (bkt[5 - k] aliases bkt[k] for the pairs), row, key group
struct RhRowAddr { uint32_t table, row, group; };
static inline RH_HD RhRowAddr rh_row_addr_pair(uint32_t la, uint32_t sign, uint32_t l, uint32_t gbits)
{
    const uint32_t h = gbits - 1, mixed = rh_mix32(la > 3 ? rh_sig_rcform(sign, l) : sign, l);
    return {rh_table_of(la), mixed >> h, ((la > 3 ? 1u : 0u) << h) | (mixed & ((1u << h) - 1u))};
}
static inline RH_HD RhRowAddr rh_row_addr_canon(uint32_t la, const RhCanon &c, uint32_t l, uint32_t gbits)
{
    const uint32_t h = gbits - 1, mixed = rh_mix32(c.index, l - 1);
    return {la, mixed >> h, (c.which << h) | (mixed & ((1u << h) - 1u))};
}
static inline RH_HD RhRowAddr rh_row_addr(uint32_t la, uint32_t sign, uint32_t l, uint32_t gbits)
{
    return rh_table_kind(la) == RH_TABLE_PAIR ? rh_row_addr_pair(la, sign, l, gbits) : rh_row_addr_canon(la, rh_sig_canon(sign, l), l, gbits);
}
// the key the entries of list la are sorted by when the rows are built: row, then group (row << gbits | group), l bits for a
// canonical table and l + 1 for a pair table, whose second list is merged in behind the first -- it is sorted by row << (gbits
// - 1) | low group bits = the mixed placement signature, and gets its `which` bit when the entries are made
static inline RH_HD uint32_t rh_place_key(uint32_t la, uint32_t sign, uint32_t l, uint32_t gbits)
{
    if (rh_table_kind(la) == RH_TABLE_PAIR) return rh_mix32(la > 3 ? rh_sig_rcform(sign, l) : sign, l);
    const RhRowAddr a = rh_row_addr_canon(la, rh_sig_canon(sign, l), l, gbits);
    return (a.row << gbits) | a.group;
}

