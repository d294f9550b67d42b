// read_words.h -- what the wave-per-fragment kernels that compare a whole read to a window of text share (mate_search.hip,
// gap_rescue.hip): the wave's LDS hand-over, a read's words of 32 bases from the batch, their reverse complement.
#pragma once
#include "real_hip_internal.h"
#include "kernel_common.h"

static __device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// word j of a read (32 bases, MSB first) from the batch; *bad is set if a base is > 3 (byte input)
static __device__ __forceinline__ uint64_t ms_word(const DevBatch &b, uint64_t o0, uint32_t patl, uint32_t j, bool *bad)
{
    const uint32_t nb = min(32u, patl - 32u * j);
    uint64_t w = 0;
    if (b.packed) {
        const uint64_t g0 = o0 + 32ull * j; // first base of the word inside the batch
        const uint8_t *p = b.bases + (g0 >> 2);
        const uint32_t sh = 2u * (uint32_t)(g0 & 3);
        const uint32_t nbytes = (uint32_t)(((g0 & 3) + nb + 3) >> 2);
        for (uint32_t k = 0; k < 8 && k < nbytes; ++k) w |= (uint64_t)p[k] << (56 - 8 * k);
        if (sh) { w <<= sh; if (nbytes > 8) w |= (uint64_t)p[8] >> (8 - sh); }
    } else {
        const uint8_t *p = b.bases + o0 + 32ull * j;
        for (uint32_t i = 0; i < nb; ++i) { const uint32_t c = p[i]; if (c > 3) *bad = true; w |= (uint64_t)(c & 3) << (62 - 2 * i); }
    }
    if (nb < 32) w &= ~0ull << (64 - 2 * nb);
    return w;
}

// the reverse complement of a read of `len` bases whose words sO[] the wave has in LDS, into sRc[]: the complement of the
// 2-bit reversal, shifted by the pad of the last word; the lanes stride over the words
static __device__ __forceinline__ void ms_revcomp(const uint64_t *sO, uint64_t *sRc, uint32_t len, uint32_t lane)
{
    const uint32_t nw = (len + 31) >> 5, pad = 64 * nw - 2 * len;
    for (uint32_t j = lane; j < nw; j += 64) {
        const uint64_t x = rev2(sO[nw - 1 - j]), y = (j + 2 <= nw) ? rev2(sO[nw - 2 - j]) : 0ull;
        const uint64_t v = pad ? ((x << pad) | (y >> (64 - pad))) : x;
        sRc[j] = ~v & ((j + 1 < nw) ? ~0ull : (~0ull << pad));
    }
}
