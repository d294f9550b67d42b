// index_readback.hip -- the resident index read back for the tests and the CPU baseline: the entries and bucket starts of a list
// out of its bucket rows (rh_rows_unpack: real_hip_index_download), a list in the reference's form {signature, position}
// (rh_index_export).  Not on any hot path.
#include "index_device.h"

#include <rocprim/device/device_scan.hpp>

// ordered traversal of the rows: per-bucket sizes, then (after a scan) the entries in list order.  [g0, g1): the key groups
// of the row that belong to the list (a table of its own: 0, 16; a pair table: the list's half)
__device__ __forceinline__ uint32_t ovf_groups_below(const uint2 *__restrict__ ovf, uint32_t o0, uint32_t tot, uint32_t pbits, uint32_t g)
{
    if (g == 0) return 0;
    if (g >= 16) return tot;
    uint32_t x = 0, y = tot;
    while (x < y) { const uint32_t mid = x + ((y - x) >> 1); if ((ovf[o0 + mid].x >> pbits) < g) x = mid + 1; else y = mid; }
    return x;
}
__global__ void rows_sizes_kernel(const uint4 *__restrict__ rows, const uint2 *__restrict__ ovf, uint64_t nbuckets, uint32_t pbits, uint32_t g0,
                                  uint32_t g1, uint32_t *__restrict__ size)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p > nbuckets) return;
    uint32_t c = 0;
    if (p < nbuckets) {
        const uint4 h = rows[p * 8];
        c = rh_row_complex(h.x, h.y) ? ovf_groups_below(ovf, h.z, h.w, pbits, g1) - ovf_groups_below(ovf, h.z, h.w, pbits, g0)
                                     : rh_row_group4(h.x, h.y, g1).x - rh_row_group4(h.x, h.y, g0).x;
    }
    size[p] = c;
}
__global__ void rows_unpack_kernel(const uint4 *__restrict__ rows, const uint2 *__restrict__ ovf, uint64_t nbuckets, uint32_t pbits, uint32_t g0,
                                   const uint32_t *__restrict__ off, uint2 *__restrict__ out)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nbuckets) return;
    const uint32_t *w = reinterpret_cast<const uint32_t *>(rows + p * 8);
    const uint32_t o = off[p], c = off[p + 1] - o;
    if (rh_row_complex(w[0], w[1])) {
        const uint32_t base = w[2] + ovf_groups_below(ovf, w[2], w[3], pbits, g0);
        for (uint32_t j = 0; j < c; ++j) out[o + j] = ovf[base + j];
    } else {
        const uint32_t base = rh_row_group4(w[0], w[1], g0).x;
        for (uint32_t j = 0; j < c; ++j) out[o + j] = rh_row_entry(w, base + j);
    }
}

// the order index_download presents of a list that is not placed by its own signature (lists 5, 4 of the pair tables, lists 2, 3
// of the canonical tables): by rh_mix32 of its OWN signature
__global__ void own_keys_kernel(const uint2 *__restrict__ ent, const uint64_t *__restrict__ T, uint64_t n, uint32_t l, int list,
                                uint32_t *__restrict__ keys)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) keys[j] = rh_mix32((uint32_t)window_signature(T, ent[j].y, l, list), l);
}
// the starts of the 2^pb prefixes of a pair table's list: every second row's
__global__ void every_second_kernel(const uint32_t *__restrict__ in, uint64_t n, uint32_t *__restrict__ out)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) out[j] = in[2 * j];
}
__global__ void starts_kernel(const uint32_t *__restrict__ keys, uint64_t n, uint32_t pshift, uint64_t nbuckets, uint32_t *__restrict__ bkt)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    bucket_starts_fill(bkt, j, keys[j] >> pshift, j ? (int64_t)(keys[j - 1] >> pshift) : -1, n, nbuckets);
}

// entries of list `list` as {key, pos} (key = the row's 16 partner bits, or the overflow entry's key) and the 2^pb + 1 bucket
// starts; either output may be null.  Used by index_download / index_export.  The order is the one of the rows, which for
// lists 5 and 4 of a pair table is that of the rc-form of their signatures and for lists 2 and 3 that of their canonical
// index (row_addr.h); `canonical` (both outputs wanted) sorts those four back to the order of rh_mix32 of their own signature,
// the one lists 0 and 1 have: what index_download presents is that order, not the physical one.
int rh_rows_unpack(real_hip_ctx *ctx, int list, uint2 *d_entries, uint32_t *d_starts, bool canonical)
{
    const uint32_t l = ctx->prm.seedl;
    const bool narrow = l <= 32, paired = narrow && rh_table_kind((uint32_t)list) == RH_TABLE_PAIR;
    const int table = narrow ? (int)rh_table_of((uint32_t)list) : list;
    const uint64_t nb = narrow ? rh_table_rows((uint32_t)list, ctx->pb) : 1ull << ctx->pb, n = ctx->n_entries;
    uint32_t pshift, fshift, fbits, pbits;
    rh_index_geometry(l, ctx->pb, &pshift, &fshift, &fbits, &pbits);
    const uint32_t half = paired ? 1u << (fbits - 1) : 16u, g0 = paired && list > 3 ? half : 0u, g1 = paired && list < 2 ? half : 16u;
    const bool resort = canonical && narrow && list > 1 && n;
    if (resort && !(d_entries && d_starts)) return rh_fail(ctx, REAL_HIP_E_INVALID, "rows unpack: canonical order needs both outputs", hipSuccess);
    int rc;
    // (the entries themselves are the values of the re-sort: two key arrays and one more entry array beside the caller's)
    ScopedBuf sizes(ctx), offs(ctx), k0(ctx), k1(ctx), other(ctx);
    RhSyncOnExit sync(ctx); // (whichever way out: the stream is idle before the buffers go)
    if ((rc = rh_reserve(ctx, sizes, (nb + 1) * 4))) return rc;
    if ((rc = rh_reserve(ctx, offs, (nb + 1) * 4))) return rc;
    const uint4 *rows = (const uint4 *)ctx->bkt[table].p;
    const uint2 *ovf = (const uint2 *)ctx->ent[table].p;
    rh_launch_each(rows_sizes_kernel, nb + 1, ctx->stream, rows, ovf, nb, pbits, g0, g1, (uint32_t *)sizes.p);
    auto scan = [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, (uint32_t *)sizes.p, (uint32_t *)offs.p, 0u, (size_t)(nb + 1), rocprim::plus<uint32_t>(), ctx->stream);
    };
    if ((rc = rh_prim_run(ctx, ctx->sort_tmp, scan, "rows unpack"))) return rc;
    if (d_entries) rh_launch_each(rows_unpack_kernel, nb, ctx->stream, rows, ovf, nb, pbits, g0, (const uint32_t *)offs.p, d_entries);
    // the starts of the 2^pb prefixes: every row's of a table of its own, every second row's of a pair table
    if (d_starts && !resort) {
        const uint64_t ns = ((uint64_t)1 << ctx->pb) + 1;
        if (paired) rh_launch_each(every_second_kernel, ns, ctx->stream, (const uint32_t *)offs.p, ns, d_starts);
        else RH_HIP(ctx, hipMemcpyAsync(d_starts, offs.p, (nb + 1) * 4, hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (resort) {
        if ((rc = rh_reserve(ctx, k0, n * 4))) return rc;
        if ((rc = rh_reserve(ctx, k1, n * 4))) return rc;
        if ((rc = rh_reserve(ctx, other, n * sizeof(uint2)))) return rc;
        rocprim::double_buffer<uint32_t> keys((uint32_t *)k0.p, (uint32_t *)k1.p);
        rocprim::double_buffer<uint2> vals(d_entries, (uint2 *)other.p);
        size_t st = 0;
        if ((rc = rh_sort_pairs_size<uint32_t, uint2>(ctx, n, l, st))) return rc;
        if ((rc = rh_reserve(ctx, ctx->sort_tmp, st ? st : 8))) return rc;
        rh_launch_each(own_keys_kernel, n, ctx->stream, d_entries, (const uint64_t *)ctx->text.p, n, l, list, (uint32_t *)k0.p);
        // (stable: equal signatures keep ascending position)
        if ((rc = rh_prim_run(ctx, ctx->sort_tmp.p, st, rh_sort_pairs(keys, vals, n, l, ctx->stream), "rows unpack"))) return rc;
        rh_launch_each(starts_kernel, n, ctx->stream, keys.current(), n, pshift, (uint64_t)1 << ctx->pb, d_starts);
        if (vals.current() != d_entries) RH_HIP(ctx, hipMemcpyAsync(d_entries, vals.current(), n * sizeof(uint2), hipMemcpyDeviceToDevice, ctx->stream));
    }
    RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return REAL_HIP_OK;
}

// ---------------------------------------------------------------------------
// export of a device list in the reference's form {signature, position} (tests, CPU baseline)
// ---------------------------------------------------------------------------
template <typename K>
__global__ void export_kernel(const uint2 *__restrict__ ent, const uint64_t *__restrict__ T, uint64_t n, uint32_t l, int list,
                              K *__restrict__ sign, uint32_t *__restrict__ pos)
{
    uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t p = ent[j].y;
    sign[j] = (K)window_signature(T, p, l, list);
    pos[j] = p;
}

int rh_index_export(real_hip_ctx *ctx, int list, void *h_sign, uint32_t *h_pos)
{
    const uint64_t n = ctx->n_entries;
    if (!n) return REAL_HIP_OK;
    const uint32_t l = ctx->prm.seedl;
    const unsigned sb = l <= 32 ? 4 : 8;
    const bool rows = ctx->layout == RH_LAYOUT_ROWS;
    return rh_by_sig_width(sb, [&](auto k) -> int {
        using K = decltype(k);
        int rc;
        if ((rc = rh_reserve(ctx, ctx->keys_a, n * sb))) return rc;
        if ((rc = rh_reserve(ctx, ctx->vals_a, n * 4))) return rc;
        ScopedBuf unpacked(ctx); // bucket rows: the entries in list order first
        const uint2 *d_ent = (const uint2 *)ctx->ent[list].p;
        if (rows) {
            // ... and that order is the one of the mixed signatures (real_hip_internal.h: rh_mix32): signatures and positions are
            // sorted back into the reference's list order (stable: equal signatures are together and in ascending position
            // already).  The unpacked entries are dead once the signatures are computed: their room is the sort's other buffer.
            size_t sort_tmp = 0;
            if ((rc = rh_sort_pairs_size<K, uint32_t>(ctx, n, l, sort_tmp))) return rc;
            const size_t room = n * (sb + 4) > n * sizeof(uint2) ? n * (sb + 4) : n * sizeof(uint2);
            if ((rc = rh_reserve(ctx, unpacked, room))) return rc;
            if ((rc = rh_reserve(ctx, ctx->sort_tmp, sort_tmp ? sort_tmp : 8))) return rc; // (one allocation for the unpack's scan and the sort)
            if ((rc = rh_rows_unpack(ctx, list, (uint2 *)unpacked.p, nullptr, false))) return rc;
            d_ent = (const uint2 *)unpacked.p;
        }
        uint8_t *alt = (uint8_t *)unpacked.p; // (rows only)
        rocprim::double_buffer<K> keys((K *)ctx->keys_a.p, (K *)alt);
        rocprim::double_buffer<uint32_t> vals((uint32_t *)ctx->vals_a.p, alt ? (uint32_t *)(alt + n * sb) : nullptr);
        rh_launch_each(export_kernel<K>, n, ctx->stream, d_ent, (const uint64_t *)ctx->text.p, n, l, list, keys.current(), vals.current());
        RH_HIP(ctx, hipGetLastError());
        if (rows && (rc = rh_prim_run(ctx, ctx->sort_tmp, rh_sort_pairs(keys, vals, n, l, ctx->stream), "radix sort"))) return rc;
        if (h_sign) RH_HIP(ctx, hipMemcpyAsync(h_sign, keys.current(), n * sb, hipMemcpyDeviceToHost, ctx->stream));
        if (h_pos) RH_HIP(ctx, hipMemcpyAsync(h_pos, vals.current(), n * 4, hipMemcpyDeviceToHost, ctx->stream));
        RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return REAL_HIP_OK;
    });
}
