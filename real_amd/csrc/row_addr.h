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

// ---- paired bucket rows (narrow rows, seedl <= 32) -------------------------------------------------------------------
// The reverse strand's seed is the reverse complement of the forward one, so the signature the reverse strand looks up in
// list 5 - k is the rc-form of the signature the forward strand looks up in list k, for the conjugate lists (0, 5) and
// (1, 4): rc-form of (a, c) = (rc c, rc a), the reverse complement of the signature read as one string of bases.  The
// entries of lists 5 and 4 are therefore PLACED by the rc-form of their signature, and lists 0 / 5 (1 / 4) share one table
// of 2^(pb+1) rows: the row found with the forward list-k signature also holds the list 5-k entries the reverse strand
// asks for.  row = mixed >> (gbits - 1), key group = which << (gbits - 1) | low bits of mixed, which = 0 for lists 0, 1
// and 1 for lists 5, 4: (table, row, group) <-> (list, signature) stays a bijection, a row still holds 2^gbits groups
// with the same mean load, the first list's entries precede the second's, and the partner key of an entry stays the plain
// leading bits of its own partner list.  Lists 2 and 3 are self-conjugate and keep a table of 2^pb rows each.
static inline RH_HD bool rh_list_paired(uint32_t la) { return la < 2 || la > 3; }
static inline RH_HD uint32_t rh_sig_rcform(uint32_t sign, uint32_t l)
{
    uint32_t x = sign; // the sixteen 2-bit bases of the word in reverse order, complemented (3 - base)
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0f0f0f0fu) | ((x & 0x0f0f0f0fu) << 4);
    x = ((x >> 8) & 0x00ff00ffu) | ((x & 0x00ff00ffu) << 8);
    x = (x >> 16) | (x << 16);
    return ~x >> (32 - l);
}
// the signature list la's entries are placed by
static inline RH_HD uint32_t rh_place_sig(uint32_t la, uint32_t sign, uint32_t l) { return la > 3 ? rh_sig_rcform(sign, l) : sign; }
// where the equal range of signature `sign` of list la lies: bkt[table] (bkt[5 - k] aliases bkt[k] for the pairs), row, key group
struct RhRowAddr { uint32_t table, row, group; };
static inline RH_HD RhRowAddr rh_row_addr(uint32_t la, uint32_t sign, uint32_t l, uint32_t gbits)
{
    const uint32_t mixed = rh_mix32(rh_place_sig(la, sign, l), l);
    if (!rh_list_paired(la)) return {la, mixed >> gbits, mixed & ((1u << gbits) - 1u)};
    const uint32_t h = gbits - 1;
    return {la > 3 ? 5 - la : la, mixed >> h, ((la > 3 ? 1u : 0u) << h) | (mixed & ((1u << h) - 1u))};
}
// rows of the table list la lives in
static inline RH_HD uint64_t rh_table_rows(uint32_t la, uint32_t l, uint32_t pb) { return (l <= 32 && rh_list_paired(la)) ? 2ull << pb : 1ull << pb; }

