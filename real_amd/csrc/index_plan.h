// index_plan.h -- which tables an index of n entries per list gets: the bucket prefix width, the layout and the entry geometry.
// No HIP in here: libreal_hip.so's translation units get it through real_hip_internal.h, real_amd/host/host_selftest.cpp
// compiles it with the host compiler and prints the plan over a grid of inputs (tests/test_host_cpp.py: test_table_plan),
// the large-index branches included, which no GPU test reaches.
#pragma once
#include <stdint.h>

// The resident index layout, what the bucket tables bkt[] hold (the values real_hip_index_table_kind reports): 2^pb + 1 bucket
// starts (u32); a digest or a fingerprint directory (uint4 per bucket); one 128-byte row per bucket (real_hip_internal.h)
enum RhLayout : uint32_t { RH_LAYOUT_STARTS = 0, RH_LAYOUT_DIGEST = 1, RH_LAYOUT_FINGERPRINT = 2, RH_LAYOUT_ROWS = 3 };

// the bucket prefix width and layout of an index of n_entries per list
struct RhTables { uint32_t pb; RhLayout layout; };

// entry geometry shared by the index build and the matcher
static inline void rh_index_geometry(uint32_t l, uint32_t pb, uint32_t *pshift, uint32_t *fshift, uint32_t *fbits, uint32_t *pbits)
{
    const uint32_t R = l - pb; // signature bits below the bucket prefix
    *pshift = R;
    if (R <= 30) {
        uint32_t pbts = (32 - R) & ~1u;
        if (pbts > l) pbts = l;
        if (pbts > 30) pbts = 30;
        *fshift = 0; *fbits = R; *pbits = pbts;
    } else {
        *fshift = R - 32; *fbits = 32; *pbits = 0;
    }
}

// digest directories: uint4 {start, 8 x {size:4, partner digest:8}}: the prefix is all signature bits but one to three, so a
// bucket has at most eight key groups (= signature values) and its 16-byte table entry describes each of them
static inline bool rh_digest_geometry(uint32_t l, uint32_t pb) { return l >= pb && l - pb >= 1 && l - pb <= 3; }

// prefix bits of bucket rows: about 11 entries per 128-byte row of 20; 32-bit signatures: at most 16 signature values per row
static inline uint32_t rows_prefix_bits(uint32_t l, uint64_t n_entries)
{
    uint32_t pb = 1;
    while (pb < 30 && (double)n_entries / (double)(1ull << pb) > 11.5) pb++;
    if (l <= 32 && pb + 4 < l) pb = l - 4;
    return pb;
}

// the decision itself, without the device: pure in its arguments (device_bytes = the device's total memory)
static inline RhTables rh_plan_tables(uint32_t l, uint32_t request, uint32_t prefix_bits, uint64_t n_entries, uint64_t device_bytes, bool no_rows)
{
    // the ABI request (real_hip_params.table_kind): 0 auto, 1 bucket starts, 2 directory, 3 bucket rows
    const bool want_auto = request == 0, want_starts = request == 1, want_dir = request == 2, want_rows = request == 3;
    const bool auto_pb = prefix_bits == 0;
    uint32_t lg = 0;
    while ((1ull << (lg + 1)) <= (n_entries ? n_entries : 1)) lg++;
    const bool big = lg >= 27 && !want_starts;
    const uint32_t rpb = rows_prefix_bits(l, n_entries);
    bool rows = want_rows;
    if (want_auto && auto_pb && big && !no_rows) {
        // bucket rows are the faster layout (one HBM line per lookup) when they fit: 128 B x 2^pb x 6 lists plus the
        // build's transients (the full entry array of one list, the window positions, the bucket starts and overflow scans)
        const double need = 6.0 * 128.0 * (double)(1ull << rpb) + 12.0 * (double)n_entries + (l <= 32 ? 16.0 : 12.0) * (double)(1ull << rpb);
        // (only when the rows are reasonably full: a 200 Mbp genome would take the same 2^(l-4) rows as a 3 Gbp one)
        rows = (l <= 32 ? rpb < l : rpb + 32 <= l) && (double)n_entries / (double)(1ull << rpb) >= 4.0 && need * 1.08 <= (double)device_bytes;
    }
    uint32_t pb = prefix_bits;
    if (auto_pb && rows) { // (the room check above holds these bounds already; an explicit request may not)
        pb = rpb;
        if (l <= 32 && pb + 1 > l) pb = l > 1 ? l - 1 : 1;
        else if (l > 32 && pb + 32 > l) pb = l - 32;
    } else if (auto_pb) {
        if (l <= 32 && big) {
            // large index, 32-bit signatures: prefix = all signature bits but three (digest directories: the bucket
            // table also holds size and partner digest of the (at most eight) key groups of a bucket, so a
            // lookup lands on the reference's equal range without scanning, and on nothing at all when the
            // range is one chance entry); 16 B x 2^(l-3) per list
            pb = l - 3;
        } else if (l > 32 && big) {
            // large index, 64-bit signatures: mean bucket of 4..8 entries, described by fingerprints
            pb = lg - 2;
        } else {
            // mean bucket of 2..4 entries (the first two entries of every bucket are prefetched together)
            pb = lg > 1 ? lg - 1 : 1;
            if (pb < 8) pb = 8;
        }
    }
    if (pb > l) pb = l; // a signature has seedl bits (two segments of seedl/4 bases)
    if (pb > 30) pb = 30;
    if (pb < 1) pb = 1;
    uint32_t pshift, fshift, fbits, pbits;
    rh_index_geometry(l, pb, &pshift, &fshift, &fbits, &pbits);
    // rows: at most 16 key groups (signature values) per row
    const bool row_groups = l <= 32 ? (l >= pb && l - pb >= 1 && l - pb <= 4) : pb + 32 <= l;
    const RhLayout layout = want_starts ? RH_LAYOUT_STARTS
                          : (rows && row_groups) ? RH_LAYOUT_ROWS
                          : rh_digest_geometry(l, pb) ? RH_LAYOUT_DIGEST
                          : (pbits == 0 && (want_dir || (auto_pb && big))) ? RH_LAYOUT_FINGERPRINT
                          : RH_LAYOUT_STARTS;
    return {pb, layout};
}
