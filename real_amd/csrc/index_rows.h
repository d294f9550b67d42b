// index_rows.h -- what the index build (index_build.hip) and the cutting of the bucket rows (index_rows.hip) share: where a
// list lies in the resident tables, the scratch of one build, the row cutter.
#pragma once
#include "real_hip_ctx.h"

// Where list `list` lies and what its entries hold.  Pair tables (narrow rows): list 0 / 1 fills a table of twice the rows,
// list 5 / 4 (`second`) is merged into it: the row takes one prefix bit more, the `which` bit of the second list's key groups is
// `gor`.  A canonical table (lists 2, 3) is cut like a table of its own: its list comes sorted by row, then group
// (rh_place_key), `which` included.
struct ListPlan {
    int list, table;                       // bkt[table] / ent[table] hold the rows
    bool rows, paired, second;
    uint32_t nb;                           // buckets (rows) of the table
    uint32_t pshift, fshift, fbits, pbits; // the entries' geometry (rh_index_geometry; a pair table: one prefix bit more)
    uint32_t gbits, gor;                   // key-group bits of a row (`which` included); the second list's `which` bit
};
ListPlan rh_list_plan(const real_hip_ctx *ctx, int list);

// The tables of a previous block stay allocated when they have about the size this block needs (the next block of
// a genome, the next file of a directory: same layout, and hipMalloc of 200 GB costs seconds); otherwise they go
// first, their bytes are needed.
int rh_fit_table(real_hip_ctx *ctx, DevBuf &b, size_t need);

// ---------------------------------------------------------------------------
// scratch of one index build: ONE allocation for all six lists.  (hipMalloc / hipFree of tens of gigabytes cost
// far more than the kernels of the build -- the driver clears and maps every page -- so the transients are laid
// out once, by offset, and regions whose lifetimes do not overlap share their bytes.)
//   pair B         keys_b (n x sig_bytes) + vals_b (n x 4): destination of the upload (host-built lists); one of the
//   pair A         keys_a + vals_x                          two buffers of the device sort (rocPRIM double buffers:
//                  the sort ping-pongs between the pairs and needs no temporary of its own beyond histograms)
//   entries        bucket rows only: the full entry array {key, pos} the rows are cut from lies over whichever pair
//                  does NOT hold the sorted list
//   tables         bucket starts; rows: overflow counts, scanned in place (a pair table has twice the rows: two arrays of
//                  2^(pb+1) + 1 where three of 2^pb + 1 were)
// Persistent outputs (rows / overflow entries, or entries / bucket tables) are allocations of their own.
// ---------------------------------------------------------------------------
struct BuildScratch {
    ScopedBuf arena;
    uint8_t *keys_a = nullptr, *keys_b = nullptr;
    uint32_t *vals_x = nullptr, *vals_b = nullptr;
    void *sort_tmp = nullptr;
    size_t sort_tmp_bytes = 0;
    uint2 *ent = nullptr;
    uint32_t *bkt = nullptr, *ocnt = nullptr, *ostart = nullptr;
    ScopedBuf first_ovf; // pair tables: the overflow entries of the first list until the second is merged in
    void *scan_tmp = nullptr;
    size_t scan_tmp_bytes = 0;
    explicit BuildScratch(real_hip_ctx *c) : arena(c), first_ovf(c) {}
};

// the temporary bytes of the row cutter's scan over nb1 = buckets + 1 counts, folded into max_bytes (for S.scan_tmp)
int rh_rows_scan_size(real_hip_ctx *ctx, size_t nb1, size_t &max_bytes);
// The rows of list P.list from its entries and bucket starts (both on the device, S.ocnt / S.ostart / S.scan_tmp planned), in
// two steps, because the host reads the overflow count between them and no timing bracket spans a host synchronisation:
//   rh_rows_sizes   overflow sizes and their scan; asynchronous, inside the caller's bracket around the entries' launch
//   rh_rows_fill    the overflow count read back (synchronises), the tables fitted, the rows filled in a bracket of its own
int rh_rows_sizes(real_hip_ctx *ctx, BuildScratch &S, const ListPlan &P, const uint2 *d_ent, const uint32_t *d_bkt);
int rh_rows_fill(real_hip_ctx *ctx, BuildScratch &S, const ListPlan &P, const uint2 *d_ent, const uint32_t *d_bkt);
