// index_build.hip -- device-resident genome text and index.
//
//   * text packing: AutoTextArray's layout (AutoTextArray.hpp:28-61) from mapped symbols;
//   * index layout: each of the reference's six sorted lists (ListSet.hpp:23-31,
//     Mask.hpp:22-64) becomes an array of {fingerprint, position} in the same order,
//     plus a table of bucket starts keyed by the top `pb` signature bits.  `ptr`
//     and the partner list are not needed on the device: list_b[p->ptr].sign is
//     the other two seed segments of the same text window and is re-read from the
//     2-bit text at `pos`;
//   * device index build: window enumeration (MapTextFile.hpp:118-230),
//     six stable LSD radix sorts (rocPRIM; the index build is outside the hot path)
//     and the bucket tables.
// Which tables an index gets: index_plan.h.  The bucket rows: index_rows.hip.  The read-back: index_readback.hip.
#include "index_device.h"
#include "index_rows.h"

#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

// ---------------------------------------------------------------------------
// text
// ---------------------------------------------------------------------------
__global__ void pack_text_kernel(const uint8_t *__restrict__ sym, uint64_t n, uint64_t *__restrict__ text,
                                 uint64_t *__restrict__ wild, unsigned long long *n_wild)
{
    uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; // one wildcard word = 64 symbols
    uint64_t base = w * 64;
    if (base >= n) return;
    uint64_t t0 = 0, t1 = 0, wd = 0;
    for (int b = 0; b < 64; ++b) {
        uint64_t i = base + b;
        if (i < n) {
            uint64_t c = sym[i];
            if (c > 3) wd |= 1ull << (63 - b); // writeBit(utext[i] > 3)
            c &= 3;                              // writer.write(utext[i] & 0x3, 2)
            if (b < 32) t0 |= c << (62 - 2 * b); else t1 |= c << (62 - 2 * (b - 32));
        }
    }
    text[2 * w] = t0;
    text[2 * w + 1] = t1; // buffers are padded, 2w+1 is always inside
    wild[w] = wd;
    if (wd) atomicAdd(n_wild, (unsigned long long)__popcll(wd));
}

__global__ void count_wild_kernel(const uint64_t *__restrict__ wild, uint64_t nw, unsigned long long *n_wild)
{
    uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w < nw && wild[w]) atomicAdd(n_wild, (unsigned long long)__popcll(wild[w]));
}

// n_wild of the text: the slot zeroed, `launch` (a kernel that adds to the slot), the count read back
template <typename Launch> static int read_wild_count(real_hip_ctx *ctx, Launch &&launch)
{
    unsigned long long *d_cnt = (unsigned long long *)ctx->counters.p + (size_t)RH_CSTRIPES * 16; // scratch slot behind the stripes
    RH_HIP(ctx, hipMemsetAsync(d_cnt, 0, 8, ctx->stream));
    launch(d_cnt);
    RH_HIP(ctx, hipGetLastError());
    unsigned long long h = 0;
    RH_HIP(ctx, hipMemcpyAsync(&h, d_cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
    RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->n_wild = h;
    return REAL_HIP_OK;
}

int rh_pack_text(real_hip_ctx *ctx, const uint8_t *d_sym, uint64_t n)
{
    const uint64_t nw = (n + 63) / 64;
    return read_wild_count(ctx, [&](unsigned long long *d_cnt) {
        rh_launch_each(pack_text_kernel, nw, ctx->stream, d_sym, n, (uint64_t *)ctx->text.p, (uint64_t *)ctx->wild.p, d_cnt);
    });
}

int rh_count_wild(real_hip_ctx *ctx, uint64_t n)
{
    const uint64_t nw = (n + 63) / 64;
    return read_wild_count(ctx, [&](unsigned long long *d_cnt) {
        rh_launch_each(count_wild_kernel, nw, ctx->stream, (const uint64_t *)ctx->wild.p, nw, d_cnt);
    });
}

// ---------------------------------------------------------------------------
// index layout from a sorted list
// ---------------------------------------------------------------------------
void rh_choose_tables(real_hip_ctx *ctx, uint64_t n_entries)
{
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    const RhTables t = rh_plan_tables(ctx->prm.seedl, ctx->prm.table_kind, ctx->prm.prefix_bits, n_entries, total_b, ctx->no_rows);
    ctx->pb = t.pb; ctx->layout = t.layout;
}

// entry j of the device list: {signature bits below the bucket prefix | top bits of the partner
// signature, window start}.  The partner signature list_b[p->ptr].sign (match.hpp:386) is the
// signature of list 5-k of the same window; keeping its top bits lets the matcher discard nearly
// every chance candidate (seed popcount filter on the known symbols) without touching the text.
template <typename K>
__global__ void entries_kernel(const K *__restrict__ sign, const uint32_t *__restrict__ pos, uint64_t n, uint32_t l,
                               int list, const uint64_t *__restrict__ T, uint32_t pshift, uint32_t fshift, uint32_t fbits,
                               uint32_t pbits, uint32_t gor, uint32_t nbuckets, uint2 *__restrict__ ent, uint32_t *__restrict__ bkt)
{
    uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint64_t s = (uint64_t)sign[j];
    const uint32_t wp = pos[j];
    uint64_t x = ((s >> fshift) & ((fbits >= 32) ? 0xffffffffull : ((1ull << fbits) - 1))) | gor; // (gor: the `which` bit of a pair table's second list)
    if (pbits) {
        const uint64_t partner = window_signature(T, wp, l, 5 - list);
        x = (x << pbits) | (partner >> (l - pbits));
    }
    ent[j] = make_uint2((uint32_t)x, wp);
    uint32_t p = (uint32_t)(s >> pshift);
    bucket_starts_fill(bkt, j, p, j ? (int64_t)(uint32_t)((uint64_t)sign[j - 1] >> pshift) : -1, n, nbuckets);
}

// digest directory (RH_LAYOUT_DIGEST): uint4 {start, 96 bits = 8 x {size:4, digest:8}} per bucket, field g = key group g
// (= signature value g of the bucket).  size 15 means "15 or more": the matcher then finds that group's
// bounds by binary search inside the bucket.  digest = the leading (at most 8) partner-signature bits of
// the group's first entry: for a group of one entry the matcher evaluates the seed popcount filter on
// those symbols first and, if it already fails, never touches the entry (a whole 128-byte line saved
// for 3/4 of the chance candidates).
__global__ void fine_table_kernel(const uint32_t *__restrict__ bkt, const uint2 *__restrict__ ent, uint64_t nbuckets,
                                  uint32_t pbits, uint32_t fbits, uint4 *__restrict__ out)
{
    uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p > nbuckets) return;
    const uint32_t start = bkt[p];
    uint32_t fld[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (p < nbuckets) {
        const uint32_t end = bkt[p + 1];
        const uint32_t dbits = pbits < 8 ? pbits : 8, gmask = (1u << fbits) - 1, pmask = pbits ? ((1u << pbits) - 1) : 0u;
        for (uint32_t j = start; j < end; ++j) {
            const uint32_t x = ent[j].x;
            const uint32_t k = (x >> pbits) & gmask;
            uint32_t f = 0;
#pragma unroll
            for (int g = 0; g < 8; ++g) if (k == (uint32_t)g) f = fld[g];
            if ((f & 15u) == 0) f = (((x & pmask) >> (pbits - dbits)) << 4) | 1u;
            else if ((f & 15u) < RH_DIGEST_SAT) f++;
#pragma unroll
            for (int g = 0; g < 8; ++g) if (k == (uint32_t)g) fld[g] = f;
        }
    }
    uint64_t lo = 0;
#pragma unroll
    for (int g = 0; g < 5; ++g) lo |= (uint64_t)fld[g] << (12 * g);
    lo |= (uint64_t)(fld[5] & 15u) << 60;
    const uint32_t hi = (fld[5] >> 4) | (fld[6] << 8) | (fld[7] << 20);
    out[p] = make_uint4(start, (uint32_t)lo, (uint32_t)(lo >> 32), hi);
}

// fingerprint bucket table (entries hold a 32-bit key, the signature is wider): uint4 {start, count:8 |
// fingerprint:11 x 8}.  count saturates at 255; only the first RH_FP_SLOTS entries are described, a bucket
// with more is searched by key.
__global__ void fp_table_kernel(const uint32_t *__restrict__ bkt, const uint2 *__restrict__ ent, uint64_t nbuckets,
                                uint4 *__restrict__ out)
{
    uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p > nbuckets) return;
    const uint32_t start = bkt[p];
    uint32_t cnt = 0;
    uint64_t lo = 0, hi = 0; // 96-bit string: count in bits 0..7, fingerprint j in bits 8+11j ..
    if (p < nbuckets) {
        const uint32_t end = bkt[p + 1];
        cnt = end - start;
        for (uint32_t j = 0; j < cnt && j < RH_FP_SLOTS; ++j) {
            const uint64_t f = rh_fp11(ent[start + j].x);
            const uint32_t b = 8 + 11 * j;
            if (b < 64) { lo |= f << b; if (b + 11 > 64) hi |= f >> (64 - b); }
            else hi |= f << (b - 64);
        }
        lo |= cnt < 255 ? cnt : 255;
    }
    out[p] = make_uint4(start, (uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi);
}


static int plan_scratch(real_hip_ctx *ctx, BuildScratch &S, uint64_t n, unsigned sig_bytes, bool need_sort)
{
    const uint32_t l = ctx->prm.seedl;
    const bool rows = ctx->layout == RH_LAYOUT_ROWS;
    const size_t nn = n ? n : 1, nb1 = (rows && l <= 32 ? (size_t)rh_table_rows(0, ctx->pb) : (size_t)1 << ctx->pb) + 1;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    size_t sort_tmp = 0, scan_tmp = 0;
    int rc;
    if (need_sort && n && (rc = rh_by_sig_width(sig_bytes, [&](auto k) { return rh_sort_pairs_size<decltype(k), uint32_t>(ctx, n, l, sort_tmp); }))) return rc;
    if (rows && (rc = rh_rows_scan_size(ctx, nb1, scan_tmp))) return rc;
    // (a pair = keys then values, back to back: the entry array of the rows lies over a whole pair, n x (sig_bytes + 4) >= n x 8)
    const size_t pair = al(nn * sig_bytes + nn * 4);
    const size_t o_keys_b = 0, o_vals_b = nn * sig_bytes, o_x = pair;
    size_t x = need_sort ? pair + al(sort_tmp ? sort_tmp : 8) : 0;
    if (rows && !need_sort) x = al(nn * sizeof(uint2)); // (host-built lists: no pair A, the entries get room of their own)
    const size_t o_bkt = o_x + x;
    const size_t o_ocnt = o_bkt + (ctx->layout != RH_LAYOUT_STARTS ? al(nb1 * 4) : 0);       // (bucket starts keep them: an allocation of their own)
    const size_t o_ostart = o_ocnt; // (scanned in place)
    const size_t o_scan = o_ostart + (rows ? al(nb1 * 4) : 0);
    const size_t total = o_scan + al(scan_tmp ? scan_tmp : 8);
    if ((rc = rh_reserve(ctx, S.arena, total))) return rc;
    uint8_t *base = (uint8_t *)S.arena.p;
    S.keys_b = base + o_keys_b; S.vals_b = (uint32_t *)(base + o_vals_b);
    S.keys_a = base + o_x; S.vals_x = (uint32_t *)(base + o_x + nn * sig_bytes); S.sort_tmp = base + o_x + pair; S.sort_tmp_bytes = sort_tmp;
    S.ent = rows ? (uint2 *)(base + o_x) : nullptr; // (the device build moves it to the pair that is free after the sort)
    S.bkt = ctx->layout != RH_LAYOUT_STARTS ? (uint32_t *)(base + o_bkt) : nullptr;
    S.ocnt = rows ? (uint32_t *)(base + o_ocnt) : nullptr;
    S.ostart = rows ? (uint32_t *)(base + o_ostart) : nullptr;
    S.scan_tmp = base + o_scan; S.scan_tmp_bytes = scan_tmp;
    return REAL_HIP_OK;
}

// the device tables of list `list` from its sorted {sign, pos} arrays (in S.keys_b / S.vals_b or anywhere else on the device):
// the entries and bucket starts, then the rows, a directory, or nothing more
static int index_from_sorted(real_hip_ctx *ctx, BuildScratch &S, int list, const void *d_sign, const uint32_t *d_pos, uint64_t n,
                             unsigned sig_bytes)
{
    const ListPlan P = rh_list_plan(ctx, list);
    const bool starts = ctx->layout == RH_LAYOUT_STARTS;
    const size_t nb1 = (size_t)P.nb + 1;
    int rc;
    if (!n && P.second) return REAL_HIP_OK; // (the first list left the rows empty)
    if (!n) {
        const size_t esz = P.rows ? 128 : (!starts ? 16 : 4);
        if ((rc = rh_fit_table(ctx, ctx->bkt[list], nb1 * esz))) return rc;
        if ((rc = rh_fit_table(ctx, ctx->ent[list], sizeof(uint2)))) return rc;
        RH_HIP(ctx, hipMemsetAsync(ctx->bkt[list].p, 0, nb1 * esz, ctx->stream));
        return REAL_HIP_OK;
    }
    // entries and bucket starts go to the scratch, or where the layout keeps them as they are to the resident tables
    uint2 *d_ent = S.ent;
    if (!P.rows) {
        if ((rc = rh_fit_table(ctx, ctx->ent[list], n * sizeof(uint2)))) return rc;
        d_ent = (uint2 *)ctx->ent[list].p;
    }
    uint32_t *d_bkt = S.bkt;
    if (starts) {
        if ((rc = rh_fit_table(ctx, ctx->bkt[list], nb1 * 4))) return rc;
        d_bkt = (uint32_t *)ctx->bkt[list].p;
    }
    { // one bracket: the entries and, asynchronous behind them, the rows' overflow sizes or the directory
        RhTimed timed(ctx, ctx->stream, REAL_HIP_K_INDEX);
        rh_by_sig_width(sig_bytes, [&](auto k) {
            using K = decltype(k);
            rh_launch_each(entries_kernel<K>, n, ctx->stream, (const K *)d_sign, d_pos, n, ctx->prm.seedl, list, (const uint64_t *)ctx->text.p, P.pshift,
                           P.fshift, P.fbits, P.pbits, P.gor, P.nb, d_ent, d_bkt);
        });
        RH_HIP(ctx, hipGetLastError());
        if (P.rows) {
            if ((rc = rh_rows_sizes(ctx, S, P, d_ent, d_bkt))) return rc;
        } else if (!starts) {
            if ((rc = rh_fit_table(ctx, ctx->bkt[list], nb1 * sizeof(uint4)))) return rc;
            uint4 *dir = (uint4 *)ctx->bkt[list].p;
            if (ctx->layout == RH_LAYOUT_DIGEST) rh_launch_each(fine_table_kernel, nb1, ctx->stream, d_bkt, d_ent, (uint64_t)P.nb, P.pbits, P.fbits, dir);
            else rh_launch_each(fp_table_kernel, nb1, ctx->stream, d_bkt, d_ent, (uint64_t)P.nb, dir);
            RH_HIP(ctx, hipGetLastError());
        }
    }
    return P.rows ? rh_rows_fill(ctx, S, P, d_ent, d_bkt) : REAL_HIP_OK; // (the rows: behind a read-back of the overflow count)
}

// ---------------------------------------------------------------------------
// the sort of a list
// ---------------------------------------------------------------------------
__global__ void iota_kernel(uint32_t *out, uint64_t first, uint64_t n)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (uint32_t)(first + i);
}

// list k signature of the window at wpos[j]; mix: the sort key of the bucket rows (narrow rows: rh_place_key, the key that
// orders the list's entries by row, then group; wide rows: rh_mix64)
template <typename K>
__device__ __forceinline__ K mixed_key(K v, uint32_t l, int list, uint32_t gbits) { return sizeof(K) == 4 ? (K)rh_place_key((uint32_t)list, (uint32_t)v, l, gbits) : (K)rh_mix64((uint64_t)v, l); }
template <typename K>
__global__ void keys_kernel(const uint64_t *__restrict__ T, const uint32_t *__restrict__ wpos, uint64_t n, uint32_t l,
                            int list, bool mix, uint32_t gbits, K *__restrict__ keys)
{
    uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const K v = (K)window_signature(T, wpos[j], l, list);
    keys[j] = mix ? mixed_key<K>(v, l, list, gbits) : v;
}
template <typename K>
__global__ void mix_keys_kernel(K *__restrict__ keys, uint64_t n, uint32_t l, int list, uint32_t gbits)
{
    uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) keys[j] = mixed_key<K>(keys[j], l, list, gbits);
}

// d_wpos: the window starts of the block in ascending order, or null = every window from first_window on (no N in the text)
// uploaded: the list is in (S.keys_b, S.vals_b) already, sorted by signature (host-built lists for bucket rows): only
// mixed and sorted again
template <typename K>
static int sort_list(real_hip_ctx *ctx, BuildScratch &S, int list, const uint32_t *d_wpos, uint64_t first_window, uint64_t n, bool uploaded = false)
{
    const uint32_t l = ctx->prm.seedl;
    const void *d_sign = S.keys_b;
    const uint32_t *d_pos = S.vals_b;
    const bool mix = ctx->layout == RH_LAYOUT_ROWS;
    uint32_t pshift, fshift, gbits, pbits;
    rh_index_geometry(l, ctx->pb, &pshift, &fshift, &gbits, &pbits);
    if (n) {
        RhTimed timed(ctx, ctx->stream, REAL_HIP_K_INDEX);
        rocprim::double_buffer<K> keys((K *)S.keys_a, (K *)S.keys_b);
        rocprim::double_buffer<uint32_t> vals(S.vals_x, S.vals_b);
        if (uploaded) {
            rh_launch_each(mix_keys_kernel<K>, n, ctx->stream, (K *)S.keys_b, n, l, list, gbits);
            keys = rocprim::double_buffer<K>((K *)S.keys_b, (K *)S.keys_a);
            vals = rocprim::double_buffer<uint32_t>(S.vals_b, S.vals_x);
        } else {
            // the values of the sort: a fresh copy of the window starts for every list (the sort clobbers both buffers)
            if (d_wpos) RH_HIP(ctx, hipMemcpyAsync(S.vals_x, d_wpos, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
            else rh_launch_each(iota_kernel, n, ctx->stream, S.vals_x, first_window, n);
            rh_launch_each(keys_kernel<K>, n, ctx->stream, (const uint64_t *)ctx->text.p, S.vals_x, n, l, list, mix, gbits, (K *)S.keys_a);
        }
        const int rc = rh_prim_run(ctx, S.sort_tmp, S.sort_tmp_bytes, rh_sort_pairs(keys, vals, n, l, ctx->stream), "radix sort");
        if (rc) return rc;
        d_sign = keys.current(); d_pos = vals.current();
        // the entry array of the rows goes over the pair the sorted list is NOT in
        if (S.ent) S.ent = (uint2 *)((const void *)keys.current() == (const void *)S.keys_a ? S.keys_b : S.keys_a);
    }
    return index_from_sorted(ctx, S, list, d_sign, d_pos, n, sizeof(K));
}

// the lists in the order they are built: the second list of a pair table right behind the first
static const int rh_build_order[6] = {0, 5, 1, 4, 2, 3};

// host-built form (real_hip_set_index_block): the six sorted lists are uploaded one after the other through the scratch
int rh_index_from_host_lists(real_hip_ctx *ctx, uint64_t n, const void *const sign[6], const uint32_t *const pos[6], unsigned sig_bytes)
{
    const double t0 = rh_now_ms();
    BuildScratch S(ctx);
    const bool rows = ctx->layout == RH_LAYOUT_ROWS; // bucket rows: the lists are sorted once more, by the mixed signature (sort_list)
    int rc = plan_scratch(ctx, S, n, sig_bytes, rows);
    if (rc) return rc;
    for (int i = 0; i < 6; ++i) {
        const int k = rh_build_order[i];
        if (n) {
            RH_HIP(ctx, hipMemcpyAsync(S.keys_b, sign[k], n * sig_bytes, hipMemcpyHostToDevice, ctx->stream));
            RH_HIP(ctx, hipMemcpyAsync(S.vals_b, pos[k], n * 4, hipMemcpyHostToDevice, ctx->stream));
        }
        if (rows) rc = rh_by_sig_width(sig_bytes, [&](auto key) { return sort_list<decltype(key)>(ctx, S, k, nullptr, 0, n, true); });
        else rc = index_from_sorted(ctx, S, k, S.keys_b, S.vals_b, n, sig_bytes);
        if (rc) return rc;
    }
    RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    rh_time_resolve(ctx);
    ctx->build_wall_ms += rh_now_ms() - t0;
    return REAL_HIP_OK;
}

// ---------------------------------------------------------------------------
// device index build
// ---------------------------------------------------------------------------
// window [i,i+l) is emitted iff it holds no N (MapTextFile::readNextSignature /
// readFullSignature, MapTextFile.hpp:118-179); fragment boundaries do not cut windows.
__global__ void window_flags_kernel(const uint64_t *__restrict__ wild, uint64_t nwin, uint32_t l, uint8_t *__restrict__ flags)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nwin) return;
    uint64_t a = i, e = i + l - 1, wa = a >> 6, we = e >> 6;
    bool ok = true;
    for (uint64_t w = wa; w <= we; ++w) {
        uint64_t m = ~0ull;
        if (w == wa) m &= ~0ull >> (a & 63);
        if (w == we) m &= ~0ull << (63 - (e & 63));
        if (wild[w] & m) ok = false;
    }
    flags[i] = ok ? 1 : 0;
}

int rh_index_build_device(real_hip_ctx *ctx, uint64_t first_window, uint64_t max_entries, uint64_t *n_entries,
                          int *have_next)
{
    const double t0 = rh_now_ms();
    const uint32_t l = ctx->prm.seedl;
    const uint64_t n = ctx->n_bases;
    const uint64_t nwin_all = (n >= l) ? (n - l + 1) : 0;
    uint64_t total_valid = nwin_all;
    const uint32_t *d_wpos = nullptr;
    uint64_t cnt = 0;
    int rc;
    if (ctx->n_wild == 0) { // every window from first_window on: the starts are generated, not stored
        cnt = (first_window < nwin_all) ? (nwin_all - first_window) : 0;
        if (cnt > max_entries) cnt = max_entries;
        d_wpos = nullptr;
    } else {
        // flags -> compacted ascending window starts (all blocks), then slice
        ScopedBuf flags(ctx), sel(ctx), dcount(ctx);
        if ((rc = rh_reserve(ctx, flags, nwin_all ? nwin_all : 1))) return rc;
        if ((rc = rh_reserve(ctx, ctx->vals_a, (nwin_all ? nwin_all : 1) * 4))) return rc;
        if ((rc = rh_reserve(ctx, dcount, 8))) return rc;
        RH_HIP(ctx, hipMemsetAsync(dcount.p, 0, 8, ctx->stream));
        if (nwin_all) {
            auto select = [&](void *tmp, size_t &bytes) {
                return rocprim::select(tmp, bytes, rocprim::counting_iterator<uint32_t>(0), (uint8_t *)flags.p, (uint32_t *)ctx->vals_a.p, (size_t *)dcount.p,
                                       (size_t)nwin_all, ctx->stream);
            };
            size_t tmp = 0;
            if ((rc = rh_prim_size(ctx, select, tmp, "select (size query)"))) return rc;
            if ((rc = rh_reserve(ctx, sel, tmp ? tmp : 8))) return rc;
            RhTimed timed(ctx, ctx->stream, REAL_HIP_K_INDEX);
            rh_launch_each(window_flags_kernel, nwin_all, ctx->stream, (const uint64_t *)ctx->wild.p, nwin_all, l, (uint8_t *)flags.p);
            if ((rc = rh_prim_run(ctx, sel.p, tmp, select, "select"))) return rc;
        }
        size_t hcount = 0;
        RH_HIP(ctx, hipMemcpyAsync(&hcount, dcount.p, 8, hipMemcpyDeviceToHost, ctx->stream));
        RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
        total_valid = hcount;
        cnt = (first_window < total_valid) ? (total_valid - first_window) : 0;
        if (cnt > max_entries) cnt = max_entries;
        d_wpos = (const uint32_t *)ctx->vals_a.p + first_window;
    }
    ctx->n_entries = cnt;
    rh_choose_tables(ctx, cnt);
    for (int attempt = 0;; ++attempt) {
        BuildScratch S(ctx);
        rc = plan_scratch(ctx, S, cnt, l <= 32 ? 4 : 8, true);
        for (int i = 0; i < 6 && !rc; ++i) {
            const int k = rh_build_order[i];
            rc = rh_by_sig_width(l <= 32 ? 4 : 8, [&](auto key) { return sort_list<decltype(key)>(ctx, S, k, d_wpos, first_window, cnt); });
        }
        if (!rc) RH_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (before the scratch goes)
        if (rc == REAL_HIP_E_NOMEM && ctx->layout == RH_LAYOUT_ROWS && ctx->prm.table_kind == 0 && !ctx->no_rows && attempt == 0) {
            // the rows did not fit after all (memory held by others): once more with directory tables
            (void)hipStreamSynchronize(ctx->stream);
            for (int j = 0; j < 6; ++j) { rh_release(ctx, ctx->ent[j]); rh_release(ctx, ctx->bkt[j]); }
            ctx->no_rows = true;
            rh_choose_tables(ctx, cnt);
            continue;
        }
        if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
        break;
    }
    rh_release(ctx, ctx->vals_a); // 4 bytes per window: give it back
    rh_time_resolve(ctx);
    ctx->have_index = true;
    if (n_entries) *n_entries = cnt;
    if (have_next) *have_next = (first_window + cnt < total_valid) ? 1 : 0;
    ctx->build_wall_ms += rh_now_ms() - t0;
    return REAL_HIP_OK;
}
