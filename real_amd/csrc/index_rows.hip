// index_rows.hip -- bucket rows (RH_LAYOUT_ROWS, format: real_hip_internal.h): one 128-byte row per bucket holds the directory
// AND the entries, so that a lookup is ONE line of HBM, fetched by eight lanes with one coalesced request (match_lists_rows).
// The rows of a list are cut from its entry array and bucket starts (index_build.hip): tables of their own, and the pair
// tables two conjugate lists share.
#include "index_device.h"
#include "index_rows.h"
#include "rocprim_call.h"

#include <rocprim/device/device_scan.hpp>

// (pbits == 0: wide signatures, the entries hold a 32-bit key; key group = its leading four bits)
__device__ __forceinline__ void bucket_groups(const uint2 *__restrict__ ent, uint32_t start, uint32_t end, uint32_t pbits, uint32_t gmask,
                                              uint32_t cnt[16])
{
#pragma unroll
    for (int g = 0; g < 16; ++g) cnt[g] = 0;
    for (uint32_t j = start; j < end; ++j) {
        const uint32_t k = pbits ? ((ent[j].x >> pbits) & gmask) : (ent[j].x >> 28);
#pragma unroll
        for (int g = 0; g < 16; ++g) if (k == (uint32_t)g) cnt[g]++;
    }
}

// The entries a row sends to the overflow array: all of them when it is complex, none when it is simple.  A row is complex
// with more than RH_ROW_CAP entries or a key group above 15 among ent[start, end); ca, first_complex: what the first list of a
// pair table left in the row (0, false for a table of its own), whose entries count and whose verdict stands.
__device__ __forceinline__ uint32_t row_overflow(const uint2 *__restrict__ ent, uint32_t start, uint32_t end, uint32_t pbits, uint32_t gmask,
                                                 uint32_t ca, bool first_complex)
{
    const uint32_t c = end - start;
    bool complex_ = first_complex || ca + c > RH_ROW_CAP;
    if (!complex_ && c > 15) {
        uint32_t cnt[16];
        bucket_groups(ent, start, end, pbits, gmask, cnt);
#pragma unroll
        for (int g = 0; g < 16; ++g) complex_ = complex_ || cnt[g] > 15;
    }
    return complex_ ? ca + c : 0u;
}

__global__ void rows_overflow_kernel(const uint32_t *__restrict__ bkt, const uint2 *__restrict__ ent, uint64_t nbuckets, uint32_t pbits,
                                     uint32_t fbits, uint32_t *__restrict__ ovf_cnt)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p > nbuckets) return;
    ovf_cnt[p] = p < nbuckets ? row_overflow(ent, bkt[p], bkt[p + 1], pbits, rh_group_mask(fbits), 0, false) : 0u;
}

__global__ void rows_fill_kernel(const uint32_t *__restrict__ bkt, const uint2 *__restrict__ ent, uint64_t nbuckets, uint32_t pbits,
                                 uint32_t fbits, const uint32_t *__restrict__ ovf_start, uint4 *__restrict__ rows, uint2 *__restrict__ ovf)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nbuckets) return;
    const uint32_t start = bkt[p], end = bkt[p + 1], c = end - start;
    const uint32_t os = ovf_start[p], oc = ovf_start[p + 1] - os;
    uint32_t w[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) w[i] = 0;
    uint32_t cnt[16];
    bucket_groups(ent, start, end, pbits, rh_group_mask(fbits), cnt);
    if (oc) { // complex
        rh_row_set_complex(w, os, c);
#pragma unroll
        for (int g = 0; g < 16; ++g) rh_row_set_count8(w, g, cnt[g]);
        for (uint32_t j = 0; j < c; ++j) ovf[os + j] = ent[start + j];
    } else {
#pragma unroll
        for (int g = 0; g < 16; ++g) rh_row_set_count4(w, g, cnt[g]);
        const uint32_t p16 = pbits < 16 ? pbits : 16;
        const uint32_t pmask = pbits ? ((1u << pbits) - 1) : 0u;
        for (uint32_t j = 0; j < c; ++j) {
            const uint2 e = ent[start + j];
            const uint32_t key = pbits ? ((e.x & pmask) >> (pbits - p16)) : rh_fp16(e.x);
            const uint32_t hw[3] = {key & 0xffffu, e.y & 0xffffu, e.y >> 16};
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const uint32_t h = rh_row_entry_hw(j) + t;
                const uint32_t v = hw[t] << (16 * (h & 1));
#pragma unroll
                for (int i = 2; i < 32; ++i) if ((h >> 1) == (uint32_t)i) w[i] |= v; // (w stays in registers)
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) rows[p * 8 + i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}

// Pair tables (real_hip_internal.h: paired bucket rows).  The first list of a pair (0, 1) is written as above into a table of
// twice the rows; the second (5, 4: sorted by the mixed rc-form of its signature) is merged into the rows in place, from
// the counts already there: a pair row is complex when the first list's part was, when both parts together exceed
// RH_ROW_CAP or when a group of the second list exceeds 15.  Entries of the first list that sat in a simple row and move
// to the overflow array get their full key back from the text (the row kept sixteen bits of it).
__device__ __forceinline__ uint32_t row_entries(uint32_t h0, uint32_t h1, uint32_t w3) { return rh_row_complex(h0, h1) ? w3 : rh_row_group4(h0, h1, 16).x; }

__global__ void pair_overflow_kernel(const uint32_t *__restrict__ bkt, const uint2 *__restrict__ ent, uint64_t nbuckets, uint32_t pbits,
                                     uint32_t gbits, const uint4 *__restrict__ rows, uint32_t *__restrict__ ovf_cnt)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p > nbuckets) return;
    uint32_t out = 0;
    if (p < nbuckets) {
        const uint4 h = rows[p * 8];
        out = row_overflow(ent, bkt[p], bkt[p + 1], pbits, rh_group_mask(gbits), row_entries(h.x, h.y, h.w), rh_row_complex(h.x, h.y));
    }
    ovf_cnt[p] = out;
}

__global__ void pair_fill_kernel(const uint32_t *__restrict__ bkt, const uint2 *__restrict__ ent, uint64_t nbuckets, uint32_t pbits,
                                 uint32_t gbits, const uint32_t *__restrict__ ovf_start, uint32_t *rows, const uint2 *__restrict__ first_ovf,
                                 uint2 *__restrict__ ovf, const uint64_t *__restrict__ T, uint32_t l, int first_list)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nbuckets) return;
    const uint32_t start = bkt[p], end = bkt[p + 1], c = end - start;
    const uint32_t os = ovf_start[p], oc = ovf_start[p + 1] - os;
    if (!c && !oc) return;
    uint32_t *w = rows + p * 32;
    const uint32_t h0 = w[0], h1 = w[1];
    const bool first_complex = rh_row_complex(h0, h1);
    const uint32_t ca = row_entries(h0, h1, w[3]);
    uint32_t cnt[16];
    bucket_groups(ent, start, end, pbits, rh_group_mask(gbits), cnt);
    if (oc) { // complex: both parts in the overflow array, the first list's in front
        uint32_t hd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        rh_row_set_complex(hd, os, ca + c);
        if (first_complex) {
            const uint32_t fo = w[2];
            for (int i = 4; i < 8; ++i) hd[i] = w[i];
            for (uint32_t j = 0; j < ca; ++j) ovf[os + j] = first_ovf[fo + j];
        } else {
            uint32_t j = 0;
            for (uint32_t g = 0; g < 16; ++g) {
                const uint32_t cg = rh_row_group4(h0, h1, g).y;
                rh_row_set_count8(hd, g, cg);
                for (uint32_t i = 0; i < cg; ++i, ++j) {
                    const uint32_t wp = rh_row_entry(w, j).y;
                    const uint32_t partner = (uint32_t)(window_signature(T, wp, l, 5 - first_list) >> (l - pbits));
                    ovf[os + j] = make_uint2((g << pbits) | partner, wp);
                }
            }
        }
        for (uint32_t g = 0; g < 16; ++g) if (cnt[g]) rh_row_set_count8(hd, g, cnt[g]);
        for (uint32_t j = 0; j < c; ++j) ovf[os + ca + j] = ent[start + j];
        for (int i = 0; i < 32; ++i) w[i] = i < 8 ? hd[i] : 0u;
    } else { // simple: the second list's counts and entries behind the first's
        uint32_t hd[2] = {h0, h1};
        for (uint32_t g = 0; g < 16; ++g) rh_row_set_count4(hd, g, cnt[g]);
        w[0] = hd[0]; w[1] = hd[1];
        uint16_t *hw = reinterpret_cast<uint16_t *>(w);
        const uint32_t p16 = pbits < 16 ? pbits : 16, pmask = (1u << pbits) - 1;
        for (uint32_t j = 0; j < c; ++j) {
            const uint2 e = ent[start + j];
            const uint32_t h = rh_row_entry_hw(ca + j);
            hw[h] = (uint16_t)((e.x & pmask) >> (pbits - p16)); hw[h + 1] = (uint16_t)(e.y & 0xffffu); hw[h + 2] = (uint16_t)(e.y >> 16);
        }
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
ListPlan rh_list_plan(const real_hip_ctx *ctx, int list)
{
    const uint32_t l = ctx->prm.seedl, pb = ctx->pb;
    ListPlan P;
    rh_index_geometry(l, pb, &P.pshift, &P.fshift, &P.fbits, &P.pbits);
    P.list = list;
    P.rows = ctx->layout == RH_LAYOUT_ROWS;
    P.paired = P.rows && l <= 32 && rh_table_kind((uint32_t)list) == RH_TABLE_PAIR;
    P.second = P.paired && list > 3;
    P.table = P.second ? 5 - list : list;
    P.nb = (uint32_t)(P.rows && l <= 32 ? rh_table_rows((uint32_t)list, pb) : 1ull << pb);
    P.gbits = P.fbits;
    if (P.paired) { P.pshift -= 1; P.fbits -= 1; }
    P.gor = P.second ? 1u << P.fbits : 0u;
    return P;
}

int rh_fit_table(real_hip_ctx *ctx, DevBuf &b, size_t need)
{
    if (b.cap >= need && b.cap <= 2 * need + ((size_t)1 << 20)) return REAL_HIP_OK;
    rh_release(ctx, b);
    return rh_reserve(ctx, b, need);
}

// the scan of the overflow counts into the rows' first overflow entries (in place when start == cnt)
static auto overflow_scan(uint32_t *cnt, uint32_t *start, size_t nb1, hipStream_t st)
{
    return [=](void *tmp, size_t &bytes) { return rocprim::exclusive_scan(tmp, bytes, cnt, start, 0u, nb1, rocprim::plus<uint32_t>(), st); };
}

int rh_rows_scan_size(real_hip_ctx *ctx, size_t nb1, size_t &max_bytes)
{
    return rh_prim_size(ctx, overflow_scan(nullptr, nullptr, nb1, ctx->stream), max_bytes, "scan (size query)");
}

// overflow sizes and their scan (the key groups of a row count gbits bits, `which` included)
int rh_rows_sizes(real_hip_ctx *ctx, BuildScratch &S, const ListPlan &P, const uint2 *d_ent, const uint32_t *d_bkt)
{
    const uint64_t nb = P.nb;
    if (P.second) rh_launch_each(pair_overflow_kernel, nb + 1, ctx->stream, d_bkt, d_ent, nb, P.pbits, P.gbits, (const uint4 *)ctx->bkt[P.table].p, S.ocnt);
    else rh_launch_each(rows_overflow_kernel, nb + 1, ctx->stream, d_bkt, d_ent, nb, P.pbits, P.gbits, S.ocnt);
    return rh_prim_run(ctx, S.scan_tmp, S.scan_tmp_bytes, overflow_scan(S.ocnt, S.ostart, (size_t)nb + 1, ctx->stream), "overflow scan");
}

int rh_rows_fill(real_hip_ctx *ctx, BuildScratch &S, const ListPlan &P, const uint2 *d_ent, const uint32_t *d_bkt)
{
    const uint64_t nb = P.nb;
    DevBuf &rows = ctx->bkt[P.table];
    // (the first list of a pair: its overflow entries wait in the scratch for the second)
    DevBuf &ovf = P.paired && !P.second ? (DevBuf &)S.first_ovf : ctx->ent[P.table];
    int rc;
    uint32_t n_ovf = 0;
    RH_HIP(ctx, hipMemcpyAsync(&n_ovf, S.ostart + nb, 4, hipMemcpyDeviceToHost, ctx->stream));
    RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (!P.second && (rc = rh_fit_table(ctx, rows, (size_t)nb * 128))) return rc;
    if ((rc = rh_fit_table(ctx, ovf, ((size_t)n_ovf + 1) * sizeof(uint2)))) return rc;
    {
        RhTimed fill(ctx, ctx->stream, REAL_HIP_K_INDEX);
        if (P.second)
            rh_launch_each(pair_fill_kernel, nb, ctx->stream, d_bkt, d_ent, nb, P.pbits, P.gbits, S.ostart, (uint32_t *)rows.p, (const uint2 *)S.first_ovf.p,
                           (uint2 *)ovf.p, (const uint64_t *)ctx->text.p, ctx->prm.seedl, P.table);
        else
            rh_launch_each(rows_fill_kernel, nb, ctx->stream, d_bkt, d_ent, nb, P.pbits, P.gbits, S.ostart, (uint4 *)rows.p, (uint2 *)ovf.p);
    }
    RH_HIP(ctx, hipGetLastError());
    if (P.second) { RH_HIP(ctx, hipStreamSynchronize(ctx->stream)); rh_release(ctx, S.first_ovf); }
    return REAL_HIP_OK;
}
