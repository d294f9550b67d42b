// index_device.h -- what the index files share (index_build.hip, index_rows.hip, index_readback.hip): reading a window's
// signature from the 2-bit text, the bucket-start rule of a sorted list, the key-group mask, the dispatch on the signature width.
#pragma once
#include "real_hip_ctx.h"
#include "rocprim_call.h"

#include <rocprim/device/device_radix_sort.hpp>

__device__ __forceinline__ uint64_t dev_text_bits(const uint64_t *__restrict__ T, uint64_t i, unsigned nb)
{
    uint64_t w = i >> 5;
    unsigned sh = 2u * (unsigned)(i & 31);
    uint64_t v = T[w] << sh;
    if (sh + 2 * nb > 64) v |= T[w + 1] >> (64 - sh);
    return v >> (64 - 2 * nb);
}

// signature of list `list` of the window at text position p (MapTextFile::readLists, MapTextFile.hpp:211-216)
__device__ __forceinline__ uint64_t window_signature(const uint64_t *__restrict__ T, uint64_t p, uint32_t l, int list)
{
    const uint32_t q = l >> 2, bb = 2 * q;
    const int sa_seg = (list < 3) ? 0 : (list < 5) ? 1 : 2;
    const int sc_seg = (list == 0) ? 1 : (list == 1 || list == 3) ? 2 : 3;
    return (dev_text_bits(T, p + (uint64_t)sa_seg * q, q) << bb) | dev_text_bits(T, p + (uint64_t)sc_seg * q, q);
}

// The bucket starts entry j of a sorted list of n writes: bucket q starts at the first entry whose prefix is >= q
// (getLookupTable.hpp:26-51 keeps [low,high) per prefix; consecutive starts carry the same information, empty = [x,x)).
// p = the prefix of entry j, pprev = that of entry j - 1 (-1 for j = 0); the last entry also closes the table up to nbuckets.
__device__ __forceinline__ void bucket_starts_fill(uint32_t *__restrict__ bkt, uint64_t j, uint32_t p, int64_t pprev, uint64_t n, uint64_t nbuckets)
{
    for (int64_t q = pprev + 1; q <= (int64_t)p; ++q) bkt[q] = (uint32_t)j;
    if (j == n - 1)
        for (uint64_t q = (uint64_t)p + 1; q <= nbuckets; ++q) bkt[q] = (uint32_t)n;
}

// the mask of a row's key group: gbits signature bits below the row's prefix (wide signatures, 32 and more: the leading four
// bits of the entry's 32-bit key)
static inline __host__ __device__ uint32_t rh_group_mask(uint32_t gbits) { return gbits >= 32 ? 15u : (1u << gbits) - 1; }

// The sort of a list as a rocPRIM call (rocprim_call.h): a stable LSD radix sort over the low `bits` bits of the keys, so equal
// signatures keep ascending position, as the reference's ParallelRadixSort (ParallelRadixSort.hpp:160-203) does.
template <typename K, typename V>
static inline auto rh_sort_pairs(rocprim::double_buffer<K> &keys, rocprim::double_buffer<V> &vals, uint64_t n, uint32_t bits, hipStream_t st)
{
    return [&keys, &vals, n, bits, st](void *tmp, size_t &bytes) { return rocprim::radix_sort_pairs(tmp, bytes, keys, vals, (size_t)n, 0u, bits, st); };
}
// ... and the temporary bytes it needs, folded into max_bytes
template <typename K, typename V> static inline int rh_sort_pairs_size(real_hip_ctx *ctx, uint64_t n, uint32_t bits, size_t &max_bytes)
{
    rocprim::double_buffer<K> k(nullptr, nullptr);
    rocprim::double_buffer<V> v(nullptr, nullptr);
    return rh_prim_size(ctx, rh_sort_pairs(k, v, n, bits, ctx->stream), max_bytes, "radix sort (size query)");
}

// f(K()) with K the type of a signature of sig_bytes bytes: f is a generic lambda, `using K = decltype(k)` inside
template <typename F> static inline auto rh_by_sig_width(unsigned sig_bytes, F &&f) { return sig_bytes == 4 ? f(uint32_t()) : f(uint64_t()); }
