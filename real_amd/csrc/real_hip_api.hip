// real_hip_api.hip -- the C ABI of include/real_hip.h: context, uploads, staging,
// launches.  No CPU fallback: every entry point either runs the HIP path or fails.
#include "real_hip_ctx.h"
#include "pair_state.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

// ---------------------------------------------------------------------------
// plumbing
// ---------------------------------------------------------------------------
int rh_fail(real_hip_ctx *ctx, int status, const char *what, hipError_t e)
{
    if (ctx) {
        char buf[512];
        snprintf(buf, sizeof buf, "%s: %s%s%s", real_hip_strerror(status), what, e != hipSuccess ? ": " : "",
                 e != hipSuccess ? hipGetErrorString(e) : "");
        ctx->last_error = buf;
    }
    (void)hipGetLastError(); // clear sticky state
    return status;
}

double rh_now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
int rh_reserve(real_hip_ctx *ctx, DevBuf &b, size_t bytes)
{
    if (bytes <= b.cap) return REAL_HIP_OK;
    rh_release(ctx, b);
    const double t0 = rh_now_ms();
    hipError_t e = hipMalloc(&b.p, bytes);
    if (ctx) { ctx->alloc_ms += rh_now_ms() - t0; ctx->alloc_calls++; ctx->alloc_bytes += bytes; }
    if (e != hipSuccess) { b.p = nullptr; return rh_fail(ctx, REAL_HIP_E_NOMEM, "hipMalloc", e); }
    b.cap = bytes;
    return REAL_HIP_OK;
}
void rh_release(real_hip_ctx *ctx, DevBuf &b)
{
    if (b.p) {
        const double t0 = rh_now_ms();
        (void)hipFree(b.p); // (waits for the device to go idle)
        if (ctx) { ctx->free_ms += rh_now_ms() - t0; ctx->free_calls++; }
    }
    b.p = nullptr; b.cap = 0;
}
void rh_release(DevBuf &b) { rh_release(nullptr, b); }

int RhStaging::view(DevBuf &buf, const void *src, size_t bytes, size_t room, bool upload, void **dev) const
{
    *dev = const_cast<void *>(src);
    if (!host) return REAL_HIP_OK;
    int rc = rh_reserve(ctx, buf, room > bytes ? room : bytes);
    if (rc) return rc;
    *dev = buf.p;
    if (upload && bytes) RH_HIP(ctx, hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, up));
    return REAL_HIP_OK;
}
int RhStaging::back_bytes(void *dst, const void *dev, size_t bytes, const char *what) const
{
    if (!host || !bytes) return REAL_HIP_OK;
    hipError_t e = hipMemcpyAsync(dst, dev, bytes, hipMemcpyDeviceToHost, down);
    return e == hipSuccess ? REAL_HIP_OK : rh_fail(ctx, REAL_HIP_E_DEVICE, what, e);
}

RhTimer::RhTimer(real_hip_ctx *ctx, int w) : c(ctx), which(w)
{
    if (c->timing) (void)hipEventRecord(c->ev0, c->stream);
}
RhTimer::~RhTimer()
{
    if (!c->timing) return;
    (void)hipEventRecord(c->ev1, c->stream);
    if (hipEventSynchronize(c->ev1) == hipSuccess) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->ev0, c->ev1) == hipSuccess) { c->k_ms[which] += ms; c->k_n[which] += 1; }
    }
}

// asynchronous timing: one event pair per launch, resolved (elapsed time read) after the next sync
static hipEvent_t rh_event(real_hip_ctx *c)
{
    if (!c->ev_pool.empty()) { hipEvent_t e = c->ev_pool.back(); c->ev_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}
static void time_begin(real_hip_ctx *c, hipStream_t st, double *ms, uint64_t *n)
{
    if (!c->timing) return;
    real_hip_ctx::Pending p; p.a = rh_event(c); p.b = nullptr; p.ms = ms; p.n = n;
    (void)hipEventRecord(p.a, st);
    c->pending.push_back(p);
}
void rh_time_begin(real_hip_ctx *c, hipStream_t st, int which) { time_begin(c, st, &c->k_ms[which], &c->k_n[which]); }
void rh_time_begin(real_hip_ctx *c, hipStream_t st, RhStage &stage) { time_begin(c, st, &stage.kernel_ms, nullptr); }
void rh_time_end(real_hip_ctx *c, hipStream_t st)
{
    if (!c->timing || c->pending.empty()) return;
    for (size_t i = c->pending.size(); i-- > 0;)
        if (!c->pending[i].b) { c->pending[i].b = rh_event(c); (void)hipEventRecord(c->pending[i].b, st); break; }
}
void rh_time_resolve(real_hip_ctx *c)
{
    // (pairs whose end has not executed yet -- a batch still in flight in the other slot -- stay pending)
    size_t keep = 0;
    for (auto &p : c->pending) {
        if (p.a && p.b && hipEventQuery(p.b) == hipSuccess) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) { *p.ms += ms; if (p.n) *p.n += 1; }
            c->ev_pool.push_back(p.a);
            c->ev_pool.push_back(p.b);
        } else {
            c->pending[keep++] = p;
        }
    }
    (void)hipGetLastError(); // (hipErrorNotReady of the queries)
    c->pending.resize(keep);
}
// the tail of a synchronous call: the stream is synchronised also behind an error (nothing of the caller's memory stays in
// flight), and the call's own error is reported before the synchronisation's
static int rh_sync_tail(real_hip_ctx *ctx, int rc)
{
    hipError_t e = hipStreamSynchronize(ctx->stream);
    rh_time_resolve(ctx);
    if (rc) return rc;
    if (e != hipSuccess) return rh_fail(ctx, REAL_HIP_E_DEVICE, "hipStreamSynchronize", e);
    return REAL_HIP_OK;
}

extern "C" const char *real_hip_strerror(int s)
{
    switch (s) {
    case REAL_HIP_OK: return "ok";
    case REAL_HIP_E_INVALID: return "invalid argument";
    case REAL_HIP_E_NOMEM: return "out of memory";
    case REAL_HIP_E_DEVICE: return "HIP runtime error";
    case REAL_HIP_E_OVERFLOW: return "output capacity too small";
    case REAL_HIP_E_STATE: return "text or index not set";
    case REAL_HIP_E_UNSUPPORTED: return "unsupported";
    default: return "unknown status";
    }
}
extern "C" const char *real_hip_last_error(const real_hip_ctx *ctx) { return ctx ? ctx->last_error.c_str() : ""; }
extern "C" int real_hip_abi_version(void) { return REAL_HIP_ABI_VERSION; }

// ---------------------------------------------------------------------------
// scoring table: Scoring::init + Scoring::getScore(char,char,int)
// (Scoring.cpp:28-36, 61-133, 155-171).  Plain IEEE double arithmetic in the
// reference's operation order; built once on the host.
// ---------------------------------------------------------------------------
static const double kQPrb[65] = {
    1.0000000, 0.7943282, 0.6309573, 0.5011872, 0.3981072, 0.3162278, 0.2511886, 0.1995262, 0.1584893, 0.1258925,
    0.1000000, 0.0794328, 0.0630957, 0.0501187, 0.0398107, 0.0316228, 0.0251189, 0.0199526, 0.0158489, 0.0125893,
    0.0100000, 0.0079433, 0.0063096, 0.0050119, 0.0039811, 0.0031623, 0.0025119, 0.0019953, 0.0015849, 0.0012589,
    0.0010000, 0.0007943, 0.0006310, 0.0005012, 0.0003981, 0.0003162, 0.0002512, 0.0001995, 0.0001585, 0.0001259,
    0.0001000, 0.0000794, 0.0000631, 0.0000501, 0.0000398, 0.0000316, 0.0000251, 0.0000200, 0.0000158, 0.0000126,
    0.0000100, 0.0000079, 0.0000063, 0.0000050, 0.0000040, 0.0000032, 0.0000025, 0.0000020, 0.0000016, 0.0000013,
    0.0000010, 0.0000008, 0.0000006, 0.0000005, 0.0000004};

extern "C" void real_hip_scoring_table(double similarity, double gc, double trans, double err, double bias, double LL[1024])
{
    volatile double R[4][4]; // the reference stores every intermediate (-ffloat-store, src/Makefile.am:95-96)
    volatile double t1 = trans * (1 - similarity);
    volatile double t2 = (1 - trans) * (1 - similarity);
    const double transit = t1, transver = t2;
    double bg[4] = {(1 - gc) / 2, gc / 2, gc / 2, (1 - gc) / 2};
    bias = bias * (1 - gc) / gc;
    R[0][2] = transit / (bias + 1) / (1 - gc);
    R[3][1] = transit / (bias + 1) / (1 - gc);
    R[2][0] = transit / (bias + 1) / gc * bias;
    R[1][3] = transit / (bias + 1) / gc * bias;
    R[0][1] = transver / 2 / (bias + 1) / (1 - gc);
    R[3][2] = transver / 2 / (bias + 1) / (1 - gc);
    R[0][3] = transver / 2 / (bias + 1) / (1 - gc);
    R[3][0] = transver / 2 / (bias + 1) / (1 - gc);
    R[1][0] = transver / 2 / (bias + 1) / gc * bias;
    R[2][3] = transver / 2 / (bias + 1) / gc * bias;
    R[1][2] = transver / 2 / (bias + 1) / gc * bias;
    R[2][1] = transver / 2 / (bias + 1) / gc * bias;
    R[0][0] = 1 - R[0][1] - R[0][2] - R[0][3];
    R[3][3] = 1 - R[3][0] - R[3][1] - R[3][2];
    R[2][2] = 1 - R[2][0] - R[2][1] - R[2][3];
    R[1][1] = 1 - R[1][0] - R[1][2] - R[1][3];
    for (int x = 0; x < 4; ++x)
        for (int y = 0; y < 4; ++y) {
            R[x][y] *= 1 - err;
            R[x][y] /= bg[y];
        }
    for (unsigned c0 = 0; c0 < 4; ++c0)
        for (unsigned c1 = 0; c1 < 4; ++c1)
            for (unsigned q = 0; q < 64; ++q)
                LL[(c0 << 8) | (c1 << 6) | q] = std::log(R[c0][c1]) / std::log(2.0) * (1 - kQPrb[q]);
}

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------
extern "C" int real_hip_create(real_hip_ctx **out, const real_hip_params *p)
{
    if (!out || !p || p->struct_size != sizeof(real_hip_params)) return REAL_HIP_E_INVALID;
    // RealOptions.cpp:434-453 clamps these; at the ABI they are errors
    if (p->seedl < 4 || p->seedl > 64 || (p->seedl % 4) || p->seedkmax > 2 || p->totalkmax > 15) return REAL_HIP_E_INVALID;
    if (!(p->filter_mult >= 0.0)) return REAL_HIP_E_INVALID; // negative or NaN: the matcher's merge of repeated update() calls needs eps >= 0
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || p->device < 0 || p->device >= ndev) {
        (void)hipGetLastError();
        return REAL_HIP_E_DEVICE; // no GPU: the product path fails loudly, there is no CPU fallback
    }
    real_hip_ctx *c = new (std::nothrow) real_hip_ctx();
    if (!c) return REAL_HIP_E_NOMEM;
    c->prm = *p;
    c->device = p->device;
    int rc = REAL_HIP_OK;
    do {
        if (hipSetDevice(c->device) != hipSuccess) { rc = REAL_HIP_E_DEVICE; break; }
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { rc = REAL_HIP_E_DEVICE; break; }
        if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) { rc = REAL_HIP_E_DEVICE; break; }
        if (hipHostMalloc((void **)&c->h_state, 3 * 2 * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess) { rc = REAL_HIP_E_NOMEM; break; }
        memset(c->h_state, 0, 3 * 2 * sizeof(unsigned long long));
        if ((rc = rh_reserve(c, c->LL, 1024 * sizeof(double)))) break;
        if ((rc = rh_reserve(c, c->counters, (size_t)(RH_CSTRIPES + 1) * 16 * sizeof(uint64_t)))) break;
        if (hipMemcpy(c->LL.p, p->LL, 1024 * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) { rc = REAL_HIP_E_DEVICE; break; }
        if (hipMemset(c->counters.p, 0, (size_t)(RH_CSTRIPES + 1) * 16 * sizeof(uint64_t)) != hipSuccess) { rc = REAL_HIP_E_DEVICE; break; }
    } while (0);
    if (rc) { real_hip_destroy(c); return rc; }
    *out = c;
    return REAL_HIP_OK;
}

extern "C" void real_hip_destroy(real_hip_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    rh_comm_destroy(c);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    if (c->down_stream) (void)hipStreamSynchronize(c->down_stream);
    for (int i = 0; i < REAL_HIP_SLOTS; ++i) {
        RhSlot &S = c->slot[i];
        if (S.up) (void)hipEventDestroy(S.up);
        if (S.matched) (void)hipEventDestroy(S.matched);
        if (S.done) (void)hipEventDestroy(S.done);
    }
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->down_stream) (void)hipStreamDestroy(c->down_stream);
    if (c->h_state) (void)hipHostFree(c->h_state);
    rh_time_resolve(c);
    for (auto &p : c->pending) { if (p.a) (void)hipEventDestroy(p.a); if (p.b) (void)hipEventDestroy(p.b); }
    c->pending.clear();
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c; // (every DevBuf the ctx holds goes with it)
}

#define RH_ENTER(ctx)                                   \
    if (!(ctx)) return REAL_HIP_E_INVALID;              \
    RH_HIP((ctx), hipSetDevice((ctx)->device));

// every real_hip_*_stats_get: `what` is the stage's words for a wrong struct_size, `get` the stage's own read
template <typename S>
static int stats_get(real_hip_ctx *ctx, S *out, int reset, const char *what, int (*get)(real_hip_ctx *, S *, int))
{
    RH_ENTER(ctx);
    if (out && out->struct_size != sizeof(S)) return rh_fail(ctx, REAL_HIP_E_INVALID, what, hipSuccess);
    return get(ctx, out, reset);
}
// E_INVALID with the stage's prefix in front ("" : none)
static int stage_invalid(real_hip_ctx *ctx, const char *stage, const char *what)
{
    return rh_fail(ctx, REAL_HIP_E_INVALID, (std::string(stage) + (*stage ? ": " : "") + what).c_str(), hipSuccess);
}
// The capacity protocol of a finished list of `total` records of `size` bytes at `src`: *n_out = total whatever happens next;
// more than cap is E_OVERFLOW; then the copy.  `what` and `list` name the records and their list in the messages of `stage`.
static int list_out(real_hip_ctx *ctx, bool finished, const char *stage, const char *what, const char *list, const void *src, uint64_t total, size_t size,
                    void *out, uint64_t cap, uint64_t *n_out, int on_device)
{
    if (!finished) return stage_invalid(ctx, stage, (std::string(what) + " before finish").c_str());
    if (!n_out) return stage_invalid(ctx, stage, "null n_out");
    *n_out = total;
    if (total > cap) return rh_fail(ctx, REAL_HIP_E_OVERFLOW, (std::string(stage) + ": the " + list + " needs more room").c_str(), hipSuccess);
    if (!total) return REAL_HIP_OK;
    if (!out) return stage_invalid(ctx, stage, "null out");
    RH_HIP(ctx, hipMemcpyAsync(out, src, (size_t)total * size, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    return rh_sync_tail(ctx, REAL_HIP_OK);
}
// behind a finish: one that failed leaves nothing half-finished readable -- `release` what there is; the message of rc is kept
static int finish_tail(real_hip_ctx *ctx, int rc, void (*release)(real_hip_ctx *))
{
    if (rc) {
        const std::string msg = ctx->last_error;
        release(ctx);
        ctx->last_error = msg;
    }
    return rc;
}

extern "C" int real_hip_set_match_params(real_hip_ctx *ctx, uint32_t seedkmax, uint32_t totalkmax, uint32_t scores, double filter_mult)
{
    if (!ctx) return REAL_HIP_E_INVALID;
    if (seedkmax > 2 || totalkmax > 15) return rh_fail(ctx, REAL_HIP_E_INVALID, "seedkmax <= 2, totalkmax <= 15 (RealOptions.cpp:172-180, 449-453)", hipSuccess);
    if (!(filter_mult >= 0.0)) return rh_fail(ctx, REAL_HIP_E_INVALID, "filter_mult must be >= 0 (flush_pending merges repeated update() calls: sound for eps >= 0 only)", hipSuccess);
    ctx->prm.seedkmax = seedkmax; ctx->prm.totalkmax = totalkmax; ctx->prm.scores = scores ? 1u : 0u; ctx->prm.filter_mult = filter_mult;
    return REAL_HIP_OK;
}

extern "C" int real_hip_wait_event(real_hip_ctx *ctx, void *hip_event)
{
    if (!ctx || !hip_event) return REAL_HIP_E_INVALID;
    RH_HIP(ctx, hipSetDevice(ctx->device));
    RH_HIP(ctx, hipStreamWaitEvent(ctx->stream, (hipEvent_t)hip_event, 0));
    return REAL_HIP_OK;
}

extern "C" int real_hip_device_memory(real_hip_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes)
{
    RH_ENTER(ctx);
    size_t f = 0, t = 0;
    RH_HIP(ctx, hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return REAL_HIP_OK;
}

// ---------------------------------------------------------------------------
// text
// ---------------------------------------------------------------------------
static int set_frag(real_hip_ctx *ctx, uint32_t fileid, uint64_t n, const uint64_t *frag_start, uint32_t n_frag)
{
    if (!frag_start || !n_frag || frag_start[0] != 0 || frag_start[n_frag] != n)
        return rh_fail(ctx, REAL_HIP_E_INVALID, "frag_start must begin at 0 and end at n_bases", hipSuccess);
    for (uint32_t i = 0; i < n_frag; ++i)
        if (frag_start[i + 1] <= frag_start[i])
            return rh_fail(ctx, REAL_HIP_E_INVALID, "fragment starts must be strictly increasing (empty FASTA records are not representable in the reference's RangeVector)", hipSuccess);
    // UniqueMatchInfo.hpp:31-32: 6 bits of file id, 16 bits of fragment id; positions are u32
    if (fileid >= 64 || n_frag > 65536 || n > 0xffffffffull)
        return rh_fail(ctx, REAL_HIP_E_INVALID, "fileid/fragment/length exceeds the UniqueMatchInfo record", hipSuccess);
    int rc = rh_reserve(ctx, ctx->frag, ((size_t)n_frag + 1) * 8);
    if (rc) return rc;
    RH_HIP(ctx, hipMemcpyAsync(ctx->frag.p, frag_start, ((size_t)n_frag + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->n_frag = n_frag; ctx->fileid = fileid; ctx->n_bases = n;
    return REAL_HIP_OK;
}

static int alloc_text(real_hip_ctx *ctx, uint64_t n)
{
    // padded: kernels write whole 64-symbol groups, and the matcher requests the words of text[pos, pos + patl) of a
    // candidate before it has checked that the read ends inside the text (cand_load: up to RH_MAXW + 2 words from the
    // last window start on)
    size_t tw = (size_t)((n + 63) / 64) * 2 + RH_MAXW + 6, ww = (size_t)((n + 63) / 64) + 4;
    int rc = rh_reserve(ctx, ctx->text, tw * 8);
    if (rc) return rc;
    if ((rc = rh_reserve(ctx, ctx->wild, ww * 8))) return rc;
    RH_HIP(ctx, hipMemsetAsync(ctx->text.p, 0, tw * 8, ctx->stream));
    RH_HIP(ctx, hipMemsetAsync(ctx->wild.p, 0, ww * 8, ctx->stream));
    return REAL_HIP_OK;
}

extern "C" int real_hip_set_text(real_hip_ctx *ctx, uint32_t fileid, const uint64_t *text2bit, const uint64_t *wildbits,
                                 uint64_t n, const uint64_t *frag_start, uint32_t n_frag)
{
    RH_ENTER(ctx);
    if (!text2bit || !wildbits) return rh_fail(ctx, REAL_HIP_E_INVALID, "null text", hipSuccess);
    ctx->have_text = false; ctx->have_index = false;
    int rc = set_frag(ctx, fileid, n, frag_start, n_frag);
    if (rc) return rc;
    if ((rc = alloc_text(ctx, n))) return rc;
    RH_HIP(ctx, hipMemcpyAsync(ctx->text.p, text2bit, (size_t)((2 * n + 63) / 64) * 8, hipMemcpyHostToDevice, ctx->stream));
    RH_HIP(ctx, hipMemcpyAsync(ctx->wild.p, wildbits, (size_t)((n + 63) / 64) * 8, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = rh_count_wild(ctx, n))) return rc;
    ctx->have_text = true;
    return REAL_HIP_OK;
}

extern "C" int real_hip_set_text_symbols(real_hip_ctx *ctx, uint32_t fileid, const uint8_t *sym, uint64_t n, int on_device,
                                         const uint64_t *frag_start, uint32_t n_frag)
{
    RH_ENTER(ctx);
    if (!sym && n) return rh_fail(ctx, REAL_HIP_E_INVALID, "null symbols", hipSuccess);
    ctx->have_text = false; ctx->have_index = false;
    int rc = set_frag(ctx, fileid, n, frag_start, n_frag);
    if (rc) return rc;
    if ((rc = alloc_text(ctx, n))) return rc;
    const uint8_t *d_sym = sym;
    ScopedBuf tmp(ctx);
    if (!on_device) {
        if ((rc = rh_reserve(ctx, tmp, n ? n : 1))) return rc;
        RH_HIP(ctx, hipMemcpyAsync(tmp.p, sym, n, hipMemcpyHostToDevice, ctx->stream));
        d_sym = (const uint8_t *)tmp.p;
    }
    if ((rc = rh_pack_text(ctx, d_sym, n))) return rc; // (synchronous: tmp may go)
    ctx->have_text = true;
    return REAL_HIP_OK;
}

// ---------------------------------------------------------------------------
// index
// ---------------------------------------------------------------------------
extern "C" int real_hip_set_index_block(real_hip_ctx *ctx, uint64_t n, const void *const sign[6], const uint32_t *const pos[6])
{
    RH_ENTER(ctx);
    if (!ctx->have_text) return rh_fail(ctx, REAL_HIP_E_STATE, "set the text first", hipSuccess);
    if (!sign || !pos || n > 0xffffffffull) return rh_fail(ctx, REAL_HIP_E_INVALID, "bad index block", hipSuccess);
    const unsigned sb = ctx->prm.seedl <= 32 ? 4 : 8; // real.cpp:219-229
    ctx->have_index = false;
    for (int k = 0; k < 6; ++k)
        if (n && (!sign[k] || !pos[k])) return rh_fail(ctx, REAL_HIP_E_INVALID, "null list", hipSuccess);
    ctx->n_entries = n;
    rh_choose_tables(ctx, n);
    int rc = rh_index_from_host_lists(ctx, n, sign, pos, sb);
    if (rc) return rc;
    ctx->have_index = true;
    return REAL_HIP_OK;
}

extern "C" int real_hip_build_index_block(real_hip_ctx *ctx, uint64_t first_window, uint64_t max_entries,
                                          uint64_t *n_entries, int *have_next)
{
    RH_ENTER(ctx);
    if (!ctx->have_text) return rh_fail(ctx, REAL_HIP_E_STATE, "set the text first", hipSuccess);
    ctx->have_index = false;
    return rh_index_build_device(ctx, first_window, max_entries, n_entries, have_next);
}

extern "C" int real_hip_index_build_stats(real_hip_ctx *ctx, real_hip_build_stats *out, int reset)
{
    if (!ctx || !out || out->struct_size != sizeof(real_hip_build_stats)) return REAL_HIP_E_INVALID;
    out->wall_ms = ctx->build_wall_ms; out->kernel_ms = ctx->k_ms[REAL_HIP_K_INDEX];
    out->alloc_ms = ctx->alloc_ms; out->free_ms = ctx->free_ms;
    out->alloc_bytes = ctx->alloc_bytes; out->alloc_calls = ctx->alloc_calls; out->free_calls = ctx->free_calls;
    if (reset) {
        ctx->build_wall_ms = ctx->alloc_ms = ctx->free_ms = 0; ctx->alloc_bytes = ctx->alloc_calls = ctx->free_calls = 0;
        ctx->k_ms[REAL_HIP_K_INDEX] = 0; ctx->k_n[REAL_HIP_K_INDEX] = 0;
    }
    return REAL_HIP_OK;
}

extern "C" int real_hip_index_info(const real_hip_ctx *ctx, uint64_t *n_entries, uint32_t *prefix_bits)
{
    if (!ctx || !ctx->have_index) return REAL_HIP_E_STATE;
    if (n_entries) *n_entries = ctx->n_entries;
    if (prefix_bits) *prefix_bits = ctx->pb;
    return REAL_HIP_OK;
}

extern "C" int real_hip_index_table_kind(const real_hip_ctx *ctx, uint32_t *kind)
{
    if (!ctx || !kind) return REAL_HIP_E_INVALID;
    if (!ctx->have_index) return REAL_HIP_E_STATE;
    *kind = (uint32_t)ctx->layout;
    return REAL_HIP_OK;
}

extern "C" int real_hip_index_download(real_hip_ctx *ctx, int list, uint32_t *entries, uint32_t *bucket)
{
    RH_ENTER(ctx);
    if (!ctx->have_index) return rh_fail(ctx, REAL_HIP_E_STATE, "no index", hipSuccess);
    if (list < 0 || list > 5) return rh_fail(ctx, REAL_HIP_E_INVALID, "list", hipSuccess);
    const uint64_t n = ctx->n_entries;
    if (ctx->layout == RH_LAYOUT_ROWS) { // bucket rows: entries and bucket starts by an ordered traversal of the rows
        const size_t nbk = ((size_t)1 << ctx->pb) + 1;
        ScopedBuf e(ctx), st(ctx);
        RhSyncOnExit sync(ctx); // (before the two go)
        int rc;
        if ((rc = rh_reserve(ctx, e, (n ? n : 1) * sizeof(uint2)))) return rc;
        if ((rc = rh_reserve(ctx, st, nbk * 4))) return rc;
        if ((rc = rh_rows_unpack(ctx, list, (uint2 *)e.p, (uint32_t *)st.p, true))) return rc; // (the canonical order, not the physical one)
        if (n && entries) RH_HIP(ctx, hipMemcpy(entries, e.p, n * sizeof(uint2), hipMemcpyDeviceToHost));
        if (bucket) RH_HIP(ctx, hipMemcpy(bucket, st.p, nbk * 4, hipMemcpyDeviceToHost));
        return REAL_HIP_OK;
    }
    if (n && entries) RH_HIP(ctx, hipMemcpy(entries, ctx->ent[list].p, n * sizeof(uint2), hipMemcpyDeviceToHost));
    if (bucket) {
        const size_t nbk = ((size_t)1 << ctx->pb) + 1;
        if (ctx->layout != RH_LAYOUT_STARTS) RH_HIP(ctx, hipMemcpy2D(bucket, 4, ctx->bkt[list].p, 16, 4, nbk, hipMemcpyDeviceToHost)); // the .x of every uint4 (directories)
        else RH_HIP(ctx, hipMemcpy(bucket, ctx->bkt[list].p, nbk * 4, hipMemcpyDeviceToHost));
    }
    return REAL_HIP_OK;
}

extern "C" int real_hip_index_export(real_hip_ctx *ctx, int list, void *sign, uint32_t *pos)
{
    RH_ENTER(ctx);
    if (!ctx->have_index) return rh_fail(ctx, REAL_HIP_E_STATE, "no index", hipSuccess);
    if (list < 0 || list > 5) return rh_fail(ctx, REAL_HIP_E_INVALID, "list", hipSuccess);
    int rc = rh_index_export(ctx, list, sign, pos);
    rh_release(ctx->keys_a); rh_release(ctx->vals_a);
    return rc;
}

// ---------------------------------------------------------------------------
// batches
// ---------------------------------------------------------------------------
struct Staged {
    const uint8_t *bases = nullptr, *qual = nullptr;
    const uint64_t *off = nullptr;
    uint32_t upatl = 0, maxpatl = 0, W = 0;
    bool maxpatl_declared = false; // device offsets with the caller's bound: longer reads may exist (they get a wave each)
    uint32_t packed = 0;             // the matcher reads the 2-bit packed bases itself
    const uint8_t *nflags = nullptr;
};

// the batch struct of ABI version 1 ended behind max_patl
#define RH_BATCH_V1_SIZE 48u
static int batch_view(real_hip_ctx *ctx, const real_hip_batch *b, real_hip_batch &v)
{
    if (!b || (b->struct_size != sizeof(real_hip_batch) && b->struct_size != RH_BATCH_V1_SIZE))
        return rh_fail(ctx, REAL_HIP_E_INVALID, "batch struct_size", hipSuccess);
    memset(&v, 0, sizeof v);
    memcpy(&v, b, b->struct_size);
    return REAL_HIP_OK;
}

// Uploads (host batches; on `up`, which is ctx->stream for the synchronous calls and the copy stream for submitted ones).
// After it the arrays of `s` are valid for kernels on ctx->stream.
static int stage_batch(real_hip_ctx *ctx, const real_hip_batch &b, Staged &s, BatchBufs &sb, hipStream_t up, hipEvent_t up_done,
                       bool need_index = true)
{
    if (!ctx->have_text || (need_index && !ctx->have_index))
        return rh_fail(ctx, REAL_HIP_E_STATE, need_index ? "text and index must be set" : "the text must be set", hipSuccess);
    if (b.n_reads > 0xffffffffull) return rh_fail(ctx, REAL_HIP_E_INVALID, "more than 2^32 reads in one batch", hipSuccess);
    const uint64_t n = b.n_reads;
    if (!n) return REAL_HIP_OK;
    if (!b.bases) return rh_fail(ctx, REAL_HIP_E_INVALID, "null bases", hipSuccess);
    if (b.nflags && !b.packed) return rh_fail(ctx, REAL_HIP_E_INVALID, "nflags belong to packed batches (unpacked ones carry symbol 4)", hipSuccess);
    int rc;
    uint64_t total = 0;
    const RhStaging io{ctx, !b.on_device, up, up};
    if (b.offsets) {
        if (!b.on_device) {
            for (uint64_t i = 0; i < n; ++i) {
                if (b.offsets[i + 1] < b.offsets[i]) return rh_fail(ctx, REAL_HIP_E_INVALID, "offsets not monotone", hipSuccess);
                uint64_t len = b.offsets[i + 1] - b.offsets[i];
                if (len > s.maxpatl) s.maxpatl = (uint32_t)(len > 0xffffffffull ? 0xffffffffull : len);
            }
            total = b.offsets[n];
        }
        if ((rc = io.in(sb.off, b.offsets, n + 1, s.off))) return rc;
        if (b.on_device) {
            s.maxpatl = b.max_patl;
            s.maxpatl_declared = b.max_patl != 0;
            if (!s.maxpatl && (rc = rh_max_patl(ctx, s.off, n, &s.maxpatl))) return rc;
        }
    } else {
        s.upatl = b.patl; s.maxpatl = b.patl;
        total = n * (uint64_t)b.patl;
    }
    // Reads longer than the register budget of the lane-per-read kernels are matched by a wave each (match_wave.hip, from
    // LDS); beyond REAL_HIP_MAX_PATL_LONG nothing can: the reference has no such limit (RestWordBuffer grows), so that is
    // an explicit, loud error and not a skip.
    if (s.maxpatl > REAL_HIP_MAX_PATL_LONG) return rh_fail(ctx, REAL_HIP_E_UNSUPPORTED, "read longer than REAL_HIP_MAX_PATL_LONG", hipSuccess);
    const uint64_t base_bytes = b.packed ? (total + 3) / 4 : total;
    const uint8_t *d_flags = b.nflags;
    if ((rc = io.in(sb.bases, b.bases, base_bytes, s.bases, (base_bytes ? base_bytes : 1) + 16))) return rc;
    if (b.qual && (rc = io.in(sb.qual, b.qual, total, s.qual, total ? total : 1))) return rc;
    if (b.nflags && (rc = io.in(sb.nflags, b.nflags, (n + 7) / 8, d_flags))) return rc;
    if (up != ctx->stream) { // the kernels wait for the upload, the host does not
        RH_HIP(ctx, hipEventRecord(up_done, up));
        RH_HIP(ctx, hipStreamWaitEvent(ctx->stream, up_done, 0));
    }
    // packed: the matcher packs its words straight from the packed bytes (25 instead of 100 bytes of HBM per 100 bp read);
    // a read may start anywhere inside a byte
    if (b.packed) { s.packed = 1; s.nflags = d_flags; }
    s.W = (s.maxpatl + 31) / 32;
    if (s.W < 1) s.W = 1;
    if (s.W > RH_MAXW) s.W = RH_MAXW; // (longer reads: handed over to the wave-per-read kernel)
    return REAL_HIP_OK;
}

static void fill_args(real_hip_ctx *ctx, const Staged &s, uint64_t n, MatchArgs &a)
{
    memset(&a, 0, sizeof a);
    a.t.text = (const uint64_t *)ctx->text.p; a.t.wild = (const uint64_t *)ctx->wild.p;
    a.t.frag_start = (const uint64_t *)ctx->frag.p; a.t.n = ctx->n_bases; a.t.n_frag = ctx->n_frag;
    a.t.has_wild = ctx->n_wild ? 1 : 0; a.t.fileid = ctx->fileid;
    const uint32_t l = ctx->prm.seedl, pb = ctx->pb;
    for (int k = 0; k < 6; ++k) {
        // (narrow bucket rows: lists 5 and 4 live in the pair tables of lists 0 and 1, lists 2 and 3 in canonical tables of their own, rh_row_addr)
        const int t = (ctx->layout == RH_LAYOUT_ROWS && l <= 32 && k > 3) ? 5 - k : k;
        a.ix.ent[k] = (const uint2 *)ctx->ent[t].p; a.ix.bkt[k] = (const uint32_t *)ctx->bkt[t].p;
    }
    a.ix.n = ctx->n_entries; a.ix.pb = pb;
    rh_index_geometry(l, pb, &a.ix.pshift, &a.ix.fshift, &a.ix.fbits, &a.ix.pbits);
    a.ix.layout = ctx->layout;
    a.b.bases = s.bases; a.b.qual = ctx->prm.scores ? s.qual : nullptr; a.b.off = s.off;
    a.b.n_reads = n; a.b.upatl = s.upatl; a.b.W = s.W; a.b.maxpatl = s.maxpatl_declared ? REAL_HIP_MAX_PATL_LONG : s.maxpatl;
    a.b.packed = s.packed; a.b.nflags = s.nflags;
    a.LL = (const double *)ctx->LL.p;
    a.counters = (unsigned long long *)ctx->counters.p;
    a.filter_mult = ctx->prm.filter_mult;
    a.l = l; a.q = l / 4; a.b_bits = 2 * (l / 4); a.seedkmax = ctx->prm.seedkmax; a.totalkmax = ctx->prm.totalkmax;
}

extern "C" int real_hip_match_unique(real_hip_ctx *ctx, const real_hip_batch *b, uint64_t *info, float *score)
{
    RH_ENTER(ctx);
    Staged s;
    real_hip_batch bv;
    int rc = batch_view(ctx, b, bv);
    if (rc) return rc;
    b = &bv;
    const uint64_t n = b->n_reads;
    // from the first copy out of the caller's memory on, every path ends in rh_sync_tail
    if ((rc = stage_batch(ctx, bv, s, ctx->stage[0], ctx->stream, nullptr))) return rh_sync_tail(ctx, rc);
    if (!n) return REAL_HIP_OK;
    const bool sc = ctx->prm.scores != 0;
    const RhStaging io{ctx, b->on_device != 1, ctx->stream, ctx->stream}; // (host: the outputs are host memory)
    uint64_t *d_info = info;
    float *d_score = score;
    if (!info || (sc && !score)) rc = rh_fail(ctx, REAL_HIP_E_INVALID, "null info/score", hipSuccess);
    if (!rc) rc = io.inout(ctx->s_info, info, n, b->fresh != 0, d_info);
    if (!rc && sc) rc = io.inout(ctx->s_score, score, n, b->fresh != 0, d_score);
    if (!rc) {
        MatchArgs a;
        fill_args(ctx, s, n, a);
        a.info = d_info; a.score = d_score; a.b.fresh = b->fresh ? 1u : 0u;
        rc = rh_launch_match(ctx, a, false, 2);
    }
    if (!rc) rc = io.back(info, d_info, n, "download of the records");
    if (!rc && sc) rc = io.back(score, d_score, n, "download of the scores");
    rc = rh_sync_tail(ctx, rc);
    return rc ? rc : rh_match_finish(ctx, 2);
}

// ---------------------------------------------------------------------------
// pipelined host batches: submit / wait over two slots.  The upload of batch k+1 (copy stream) and the download of
// the records of batch k-1 (download stream) run beside the kernels of batch k (ctx stream); the counterpart of the
// reference's producer / consumer block ring (AsynchronousReader.hpp:181-259).
// ---------------------------------------------------------------------------
__global__ void fill_f32_kernel(float *p, uint64_t n, float v)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

static int pipeline_init(real_hip_ctx *ctx)
{
    if (ctx->copy_stream) return REAL_HIP_OK;
    RH_HIP(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    RH_HIP(ctx, hipStreamCreateWithFlags(&ctx->down_stream, hipStreamNonBlocking));
    for (int i = 0; i < REAL_HIP_SLOTS; ++i) {
        RH_HIP(ctx, hipEventCreateWithFlags(&ctx->slot[i].up, hipEventDisableTiming));
        RH_HIP(ctx, hipEventCreateWithFlags(&ctx->slot[i].matched, hipEventDisableTiming));
        RH_HIP(ctx, hipEventCreateWithFlags(&ctx->slot[i].done, hipEventDisableTiming));
    }
    return REAL_HIP_OK;
}

// everything of a submit that touches the streams; a failure half way leaves copies of the caller's memory in flight,
// which the wrapper below drains before it reports the error
static int submit_unique(real_hip_ctx *ctx, RhSlot &S, int slot, const real_hip_batch &bv, uint64_t *info, float *score, int fresh)
{
    const uint64_t n = bv.n_reads;
    const bool sc = ctx->prm.scores != 0;
    int rc;
    // records: uploaded (they are in/out: folds compose across genome blocks), or initialised on the device (fresh:
    // uniqueinfo(numpat), matchUniqueImplementation.cpp:1094-1097 -- NoMatch, score -FLT_MAX)
    const RhStaging io{ctx, true, ctx->copy_stream, ctx->down_stream};
    uint64_t *d_info = nullptr;
    float *d_score = nullptr;
    if ((rc = io.inout(S.info, info, n, fresh != 0, d_info))) return rc; // (fresh: the kernel starts every record itself)
    if (sc && (rc = io.inout(S.score, score, n, fresh != 0, d_score))) return rc;
    Staged s;
    if ((rc = stage_batch(ctx, bv, s, S.in, ctx->copy_stream, S.up))) return rc;
    MatchArgs a;
    fill_args(ctx, s, n, a);
    a.info = d_info; a.score = d_score; a.b.fresh = (fresh || bv.fresh) ? 1u : 0u;
    if ((rc = rh_launch_match(ctx, a, false, slot))) return rc;
    RH_HIP(ctx, hipEventRecord(S.matched, ctx->stream));
    RH_HIP(ctx, hipStreamWaitEvent(ctx->down_stream, S.matched, 0));
    if ((rc = io.back(info, d_info, n, "download of the records"))) return rc;
    if (sc && (rc = io.back(score, d_score, n, "download of the scores"))) return rc;
    RH_HIP(ctx, hipEventRecord(S.done, ctx->down_stream));
    return REAL_HIP_OK;
}

extern "C" int real_hip_match_unique_submit(real_hip_ctx *ctx, const real_hip_batch *b, uint64_t *info, float *score, uint32_t slot, int fresh)
{
    RH_ENTER(ctx);
    if (slot >= REAL_HIP_SLOTS) return rh_fail(ctx, REAL_HIP_E_INVALID, "slot", hipSuccess);
    RhSlot &S = ctx->slot[slot];
    if (S.busy) return rh_fail(ctx, REAL_HIP_E_STATE, "slot in flight: real_hip_wait first", hipSuccess);
    real_hip_batch bv;
    int rc = batch_view(ctx, b, bv);
    if (rc) return rc;
    if (bv.on_device) return rh_fail(ctx, REAL_HIP_E_INVALID, "submit takes host batches (device batches: the synchronous calls)", hipSuccess);
    const uint64_t n = bv.n_reads;
    if (n && (!info || (ctx->prm.scores && !score))) return rh_fail(ctx, REAL_HIP_E_INVALID, "null info/score", hipSuccess);
    if ((rc = pipeline_init(ctx))) return rc;
    S.n = n; S.status = REAL_HIP_OK;
    if (!n) { S.busy = true; S.empty = true; return REAL_HIP_OK; }
    S.empty = false;
    if ((rc = submit_unique(ctx, S, (int)slot, bv, info, score, fresh))) {
        // nothing of the caller's memory may stay in flight behind an error
        const std::string msg = ctx->last_error;
        (void)hipStreamSynchronize(ctx->copy_stream); (void)hipStreamSynchronize(ctx->stream); (void)hipStreamSynchronize(ctx->down_stream);
        (void)hipGetLastError();
        ctx->last_error = msg;
        return rc;
    }
    S.busy = true;
    return REAL_HIP_OK;
}

extern "C" int real_hip_wait(real_hip_ctx *ctx, uint32_t slot)
{
    RH_ENTER(ctx);
    if (slot >= REAL_HIP_SLOTS) return rh_fail(ctx, REAL_HIP_E_INVALID, "slot", hipSuccess);
    RhSlot &S = ctx->slot[slot];
    if (!S.busy) return REAL_HIP_OK;
    S.busy = false;
    if (S.empty) return REAL_HIP_OK;
    RH_HIP(ctx, hipEventSynchronize(S.done));
    rh_time_resolve(ctx);
    return rh_match_finish(ctx, (int)slot);
}

extern "C" void *real_hip_host_alloc(size_t bytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
extern "C" void real_hip_host_free(void *p)
{
    if (p) (void)hipHostFree(p);
}

// matchAll of one batch; dev_out: out / hit_offsets are device memory whatever the batch's inputs are.  staged (nullable)
// receives the device view of the batch's arrays (valid until the next batch is staged into the same buffers: bufs).
// match_all_run wraps the steps: once they may have queued copies of the caller's memory, every path ends in rh_sync_tail.
static int match_all_steps(real_hip_ctx *ctx, const real_hip_batch &bv, bool dev_out, real_hip_hit *out, uint64_t cap,
                           uint64_t *n_out, uint64_t *hit_offsets, Staged *staged, BatchBufs &bufs)
{
    Staged s;
    int rc;
    if ((rc = stage_batch(ctx, bv, s, bufs, ctx->stream, nullptr))) return rc;
    const uint64_t n = bv.n_reads;
    if (n_out) *n_out = 0;
    if (cap > 0xffffffffull) cap = 0xffffffffull; // record indices are 32 bit inside the post-pass
    if (staged) *staged = s;
    if ((rc = rh_reserve(ctx, ctx->raw_count, 8))) return rc;
    RH_HIP(ctx, hipMemsetAsync(ctx->raw_count.p, 0, 8, ctx->stream));
    if ((rc = rh_reserve(ctx, ctx->raw, (cap ? cap : 1) * sizeof(uint4)))) return rc;
    unsigned long long n_raw = 0;
    if (n) {
        MatchArgs a;
        fill_args(ctx, s, n, a);
        if ((rc = rh_reserve(ctx, ctx->hit_cnt, (n + 1) * 4))) return rc;
        a.raw = (uint4 *)ctx->raw.p; a.raw_count = (unsigned long long *)ctx->raw_count.p; a.raw_cap = cap;
        a.hit_cnt = (uint32_t *)ctx->hit_cnt.p;
        if ((rc = rh_launch_match(ctx, a, true, 2))) return rc;
        RH_HIP(ctx, hipMemcpyAsync(&n_raw, ctx->raw_count.p, 8, hipMemcpyDeviceToHost, ctx->stream));
        RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if ((rc = rh_match_finish(ctx, 2))) return rc;
    }
    if (n_out) *n_out = n_raw;
    if (n_raw > cap) return rh_fail(ctx, REAL_HIP_E_OVERFLOW, "hit buffer too small", hipSuccess);
    const RhStaging io{ctx, !dev_out, ctx->stream, ctx->stream};
    real_hip_hit *d_out = out;
    uint64_t *d_off = hit_offsets;
    if ((rc = io.inout(ctx->s_hits, out, n_raw, true, d_out, sizeof(real_hip_hit)))) return rc; // (outputs: nothing is uploaded)
    if (hit_offsets && (rc = io.inout(ctx->hit_off, hit_offsets, n + 1, true, d_off))) return rc;
    if (n_raw && !out) return rh_fail(ctx, REAL_HIP_E_INVALID, "null hit buffer", hipSuccess);
    if ((rc = rh_all_finish(ctx, n_raw, n, d_out, d_off))) return rc;
    if ((rc = io.back(out, d_out, n_raw, "download of the hits"))) return rc;
    return hit_offsets ? io.back(hit_offsets, d_off, n + 1, "download of the hit offsets") : REAL_HIP_OK;
}
static int match_all_run(real_hip_ctx *ctx, const real_hip_batch &bv, bool dev_out, real_hip_hit *out, uint64_t cap,
                         uint64_t *n_out, uint64_t *hit_offsets, Staged *staged, BatchBufs *bufs = nullptr)
{
    return rh_sync_tail(ctx, match_all_steps(ctx, bv, dev_out, out, cap, n_out, hit_offsets, staged, bufs ? *bufs : ctx->stage[0]));
}

extern "C" int real_hip_match_all(real_hip_ctx *ctx, const real_hip_batch *b, real_hip_hit *out, uint64_t cap,
                                  uint64_t *n_out, uint64_t *hit_offsets)
{
    RH_ENTER(ctx);
    real_hip_batch bv;
    int rc = batch_view(ctx, b, bv);
    if (rc) return rc;
    return match_all_run(ctx, bv, bv.on_device == 1, out, cap, n_out, hit_offsets, nullptr);
}

// ---------------------------------------------------------------------------
// paired-end reads: the join of the two mates' hit lists (pair_kernel.hip)
// ---------------------------------------------------------------------------
static int pair_params_check(real_hip_ctx *ctx, const real_hip_pair_params *pp)
{
    if (!pp || pp->struct_size != sizeof(real_hip_pair_params)) return rh_fail(ctx, REAL_HIP_E_INVALID, "pair params struct_size", hipSuccess);
    if (pp->orientation != 0) return rh_fail(ctx, REAL_HIP_E_UNSUPPORTED, "pair orientation other than FR (0)", hipSuccess);
    if (pp->min_insert > pp->max_insert) return rh_fail(ctx, REAL_HIP_E_INVALID, "min_insert > max_insert", hipSuccess);
    return REAL_HIP_OK;
}

// the two mates' hit lists of n fragments (lists = 1: one read's lists alone) as the caller holds them -> the device view L:
// the offsets start at 0 and do not run backwards, off[n] is the number of hits; host lists are copied into the ctx's pair
// buffers, the read lengths with them (len: null for the mate search, which takes them from the batches)
static int stage_hit_lists(real_hip_ctx *ctx, const real_hip_hit *const hits[2], const uint64_t *const off[2], const uint32_t *const len[2], uint64_t n,
                           bool on_device, MateLists &L, int lists = 2)
{
    int rc;
    memset(&L, 0, sizeof L);
    for (int m = 0; m < lists; ++m) {
        if (on_device) {
            uint64_t ends[1] = {0}, first = 0;
            RH_HIP(ctx, hipMemcpyAsync(&first, off[m], 8, hipMemcpyDeviceToHost, ctx->stream));
            RH_HIP(ctx, hipMemcpyAsync(ends, off[m] + n, 8, hipMemcpyDeviceToHost, ctx->stream));
            RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
            if (first) return rh_fail(ctx, REAL_HIP_E_INVALID, "hit offsets must start at 0", hipSuccess);
            L.total[m] = ends[0]; // (offsets in between are clamped to it by the kernels)
        } else {
            const uint64_t *o = off[m];
            if (o[0]) return rh_fail(ctx, REAL_HIP_E_INVALID, "hit offsets must start at 0", hipSuccess);
            for (uint64_t i = 0; i < n; ++i)
                if (o[i + 1] < o[i]) return rh_fail(ctx, REAL_HIP_E_INVALID, "hit offsets not monotone", hipSuccess);
            L.total[m] = o[n];
        }
        if (L.total[m] && !hits[m]) return rh_fail(ctx, REAL_HIP_E_INVALID, "null hit list", hipSuccess);
    }
    const RhStaging io{ctx, !on_device, ctx->stream, ctx->stream};
    for (int m = 0; m < lists; ++m) {
        if ((rc = io.in(ctx->join.hits[m], (const uint4 *)hits[m], L.total[m], L.h[m], sizeof(real_hip_hit)))) return rc;
        if ((rc = io.in(ctx->join.off[m], off[m], n + 1, L.o[m]))) return rc;
        if (len && (rc = io.in(ctx->join.len[m], len[m], n, L.len[m]))) return rc;
    }
    if (!on_device) ctx->join.cap = 0; // (the two hit buffers may now differ in size: real_hip_match_pairs sizes them again)
    return REAL_HIP_OK;
}
// the lists match_mates leaves resident in the ctx's pair buffers
static MateLists resident_lists(real_hip_ctx *ctx, const uint64_t total[2])
{
    MateLists L;
    for (int m = 0; m < 2; ++m) {
        L.h[m] = (const uint4 *)ctx->join.hits[m].p; L.o[m] = (const uint64_t *)ctx->join.off[m].p;
        L.len[m] = (const uint32_t *)ctx->join.len[m].p; L.total[m] = total[m];
    }
    return L;
}

extern "C" int real_hip_pair_hits(real_hip_ctx *ctx, const real_hip_pair_params *pp, const real_hip_hit *hits1, const uint64_t *off1,
                                  const uint32_t *len1, const real_hip_hit *hits2, const uint64_t *off2, const uint32_t *len2,
                                  uint64_t n_pairs, uint32_t fileid, int on_device, int fresh, real_hip_pair *pairs)
{
    RH_ENTER(ctx);
    int rc = pair_params_check(ctx, pp);
    if (rc) return rc;
    if (fileid > 255) return rh_fail(ctx, REAL_HIP_E_INVALID, "fileid > 255", hipSuccess);
    const uint64_t n = n_pairs;
    if (!n) return REAL_HIP_OK;
    if (n > 0xffffffffull) return rh_fail(ctx, REAL_HIP_E_INVALID, "more than 2^32 pairs in one call", hipSuccess);
    if (!off1 || !off2 || !len1 || !len2 || !pairs) return rh_fail(ctx, REAL_HIP_E_INVALID, "null offsets / lengths / pairs", hipSuccess);
    const real_hip_hit *const hits[2] = {hits1, hits2};
    const uint64_t *const off[2] = {off1, off2};
    const uint32_t *const len[2] = {len1, len2};
    MateLists L;
    real_hip_pair *d_pairs = pairs;
    const RhStaging io{ctx, !on_device, ctx->stream, ctx->stream};
    if ((rc = stage_hit_lists(ctx, hits, off, len, n, on_device != 0, L))) return rc;
    if ((rc = io.inout(ctx->join.rec, pairs, n, fresh != 0, d_pairs))) return rc;
    rc = rh_launch_pair(ctx, *pp, L, n, fileid, fresh, d_pairs);
    if (!rc) rc = io.back(pairs, d_pairs, n, "download of the pair records");
    return rh_sync_tail(ctx, rc);
}

// ---- mate search (mate_search.hip): what both of its entry points check before anything is launched
static int search_params_check(real_hip_ctx *ctx, const real_hip_pair_params *pp, const real_hip_mate_search_params *sp)
{
    if (!sp || sp->struct_size != sizeof(real_hip_mate_search_params)) return rh_fail(ctx, REAL_HIP_E_INVALID, "mate search params struct_size", hipSuccess);
    if (pp->max_insert > REAL_HIP_MATE_SEARCH_MAX_INSERT)
        return rh_fail(ctx, REAL_HIP_E_UNSUPPORTED, "mate search: max_insert beyond REAL_HIP_MATE_SEARCH_MAX_INSERT", hipSuccess);
    return REAL_HIP_OK;
}
// the two mates' batches in every entry point that takes two: equal in n_reads and on_device; need_index: they are to be
// matched, text and index are set.  `stage` is the prefix of the messages ("": none)
static int mates_agree(real_hip_ctx *ctx, const char *stage, const real_hip_batch bv[2], bool need_index)
{
    if (bv[0].n_reads != bv[1].n_reads) return stage_invalid(ctx, stage, "the two batches hold different numbers of reads");
    if (bv[0].on_device != bv[1].on_device) return stage_invalid(ctx, stage, "the two batches differ in on_device");
    if (need_index && (!ctx->have_text || !ctx->have_index)) return rh_fail(ctx, REAL_HIP_E_STATE, "text and index must be set", hipSuccess);
    return REAL_HIP_OK;
}
// their views bv[], then that.  An entry point with a check of its own between the two steps (real_hip_pair_search: E_STATE
// without a text; real_hip_mismatches_pairs: its outputs, *n_out = 0) makes the views itself and calls mates_agree
static int mates_view(real_hip_ctx *ctx, const char *stage, const real_hip_batch *b1, const real_hip_batch *b2, bool need_index, real_hip_batch bv[2])
{
    int rc;
    if ((rc = batch_view(ctx, b1, bv[0])) || (rc = batch_view(ctx, b2, bv[1]))) return rc;
    return mates_agree(ctx, stage, bv, need_index);
}
// what the mate search asks of them beyond that: no read longer than REAL_HIP_MAX_PATL
static int search_batches_check(real_hip_ctx *ctx, const real_hip_batch bv[2])
{
    int rc;
    const uint64_t n = bv[0].n_reads;
    if (n > 0xffffffffull) return rh_fail(ctx, REAL_HIP_E_INVALID, "more than 2^32 reads in one batch", hipSuccess);
    for (int m = 0; m < 2 && n; ++m) {
        const real_hip_batch &b = bv[m];
        uint64_t longest = b.patl;
        if (b.offsets && !b.on_device) {
            longest = 0;
            for (uint64_t i = 0; i < n; ++i)
                if (b.offsets[i + 1] >= b.offsets[i] && b.offsets[i + 1] - b.offsets[i] > longest) longest = b.offsets[i + 1] - b.offsets[i];
        } else if (b.offsets) {
            uint32_t mp = b.max_patl; // (the declared bound; a read beyond it is caught by the kernel: E_INVALID)
            if (!mp && (rc = rh_max_patl(ctx, b.offsets, n, &mp))) return rc;
            longest = mp;
        }
        if (longest > REAL_HIP_MAX_PATL) return rh_fail(ctx, REAL_HIP_E_UNSUPPORTED, "mate search: read longer than REAL_HIP_MAX_PATL", hipSuccess);
    }
    return REAL_HIP_OK;
}
static DevBatch dev_batch(real_hip_ctx *ctx, const Staged &s, uint64_t n)
{
    DevBatch b;
    memset(&b, 0, sizeof b);
    b.bases = s.bases; b.qual = ctx->prm.scores ? s.qual : nullptr; b.off = s.off;
    b.n_reads = n; b.upatl = s.upatl; b.W = s.W; b.maxpatl = s.maxpatl; b.packed = s.packed; b.nflags = s.nflags;
    return b;
}

extern "C" int real_hip_pair_search(real_hip_ctx *ctx, const real_hip_pair_params *pp, const real_hip_mate_search_params *sp,
                                    const real_hip_batch *batch1, const real_hip_batch *batch2, const real_hip_hit *hits1, const uint64_t *off1,
                                    const real_hip_hit *hits2, const uint64_t *off2, uint32_t fileid, int fresh, real_hip_pair *pairs)
{
    RH_ENTER(ctx);
    int rc = pair_params_check(ctx, pp);
    if (rc || (rc = search_params_check(ctx, pp, sp))) return rc;
    if (fileid > 255) return rh_fail(ctx, REAL_HIP_E_INVALID, "fileid > 255", hipSuccess);
    real_hip_batch bv[2];
    if ((rc = batch_view(ctx, batch1, bv[0])) || (rc = batch_view(ctx, batch2, bv[1]))) return rc;
    if (bv[0].on_device > 1) return rh_fail(ctx, REAL_HIP_E_INVALID, "real_hip_pair_search: on_device is 0 or 1", hipSuccess);
    if (!ctx->have_text) return rh_fail(ctx, REAL_HIP_E_STATE, "the text must be set", hipSuccess);
    if ((rc = mates_agree(ctx, "", bv, false)) || (rc = search_batches_check(ctx, bv))) return rc;
    const uint64_t n = bv[0].n_reads;
    if (!n) return REAL_HIP_OK;
    if (!off1 || !off2 || !pairs) return rh_fail(ctx, REAL_HIP_E_INVALID, "null offsets / pairs", hipSuccess);
    const bool on_device = bv[0].on_device == 1;
    const real_hip_hit *const hits[2] = {hits1, hits2};
    const uint64_t *const off[2] = {off1, off2};
    MateLists L;
    if ((rc = stage_hit_lists(ctx, hits, off, nullptr, n, on_device, L))) return rc;
    Staged st[2];
    for (int m = 0; m < 2; ++m)
        if ((rc = stage_batch(ctx, bv[m], st[m], ctx->stage[m], ctx->stream, nullptr, false))) return rc;
    real_hip_pair *d_pairs = pairs;
    const RhStaging io{ctx, !on_device, ctx->stream, ctx->stream};
    if ((rc = io.inout(ctx->join.rec, pairs, n, fresh != 0, d_pairs))) return rc;
    rc = rh_launch_mate_search(ctx, *pp, *sp, dev_batch(ctx, st[0], n), dev_batch(ctx, st[1], n), L, n, fileid, fresh, d_pairs);
    if (!rc) rc = io.back(pairs, d_pairs, n, "download of the pair records");
    rc = rh_sync_tail(ctx, rc);
    return rc ? rc : rh_mate_search_finish(ctx);
}

// ---- single placements of a mate (single_fold.hip): the in/out records of `lists` lists (device records: 16-byte aligned)
static int stage_singles(const RhStaging &io, int lists, real_hip_single *const singles[2], uint64_t n, int fresh, real_hip_single *d_singles[2])
{
    int rc = REAL_HIP_OK;
    for (int m = 0; m < lists && !rc; ++m) {
        if (!io.host && ((uintptr_t)singles[m] & 15u)) return rh_fail(io.ctx, REAL_HIP_E_INVALID, "the single records must be 16-byte aligned", hipSuccess);
        rc = io.inout(io.ctx->single.rec[m], singles[m], n, fresh != 0, d_singles[m]);
    }
    return rc;
}
static int download_singles(const RhStaging &io, int lists, real_hip_single *const singles[2], uint64_t n, real_hip_single *const d_singles[2])
{
    int rc = REAL_HIP_OK;
    for (int m = 0; m < lists && !rc; ++m) rc = io.back(singles[m], d_singles[m], n, "download of the single records");
    return rc;
}

extern "C" int real_hip_single_hits(real_hip_ctx *ctx, const real_hip_hit *hits, const uint64_t *off, const uint32_t *len, uint64_t n_reads,
                                    uint32_t fileid, int on_device, int fresh, real_hip_single *singles)
{
    RH_ENTER(ctx);
    int rc;
    if (fileid > 255) return rh_fail(ctx, REAL_HIP_E_INVALID, "fileid > 255", hipSuccess);
    const uint64_t n = n_reads;
    if (!n) return REAL_HIP_OK;
    if (n > 0xffffffffull) return rh_fail(ctx, REAL_HIP_E_INVALID, "more than 2^32 reads in one call", hipSuccess);
    if (!off || !len || !singles) return rh_fail(ctx, REAL_HIP_E_INVALID, "null offsets / lengths / singles", hipSuccess);
    const real_hip_hit *const hv[2] = {hits, nullptr};
    const uint64_t *const ov[2] = {off, nullptr};
    const uint32_t *const lv[2] = {len, nullptr};
    MateLists L;
    real_hip_single *const sv[2] = {singles, nullptr};
    real_hip_single *d_singles[2] = {nullptr, nullptr};
    const RhStaging io{ctx, !on_device, ctx->stream, ctx->stream};
    if ((rc = stage_hit_lists(ctx, hv, ov, lv, n, on_device != 0, L, 1))) return rc;
    rc = stage_singles(io, 1, sv, n, fresh, d_singles);
    if (!rc) rc = rh_launch_single(ctx, 1, L, n, fileid, fresh, d_singles);
    if (!rc) rc = download_singles(io, 1, sv, n, d_singles);
    return rh_sync_tail(ctx, rc);
}

extern "C" int real_hip_single_stats_get(real_hip_ctx *ctx, real_hip_single_stats *out, int reset)
{
    return stats_get(ctx, out, reset, "single stats struct_size", rh_single_stats);
}

// ---- mapping quality (mapq.hip): the in/out accumulators of `count` arrays (device records: 8-byte aligned)
static int stage_mapq_accs(const RhStaging &io, int count, real_hip_mapq_acc *const accs[], uint64_t n, int fresh, real_hip_mapq_acc *d_accs[])
{
    int rc = REAL_HIP_OK;
    for (int m = 0; m < count && !rc; ++m) {
        if (!io.host && ((uintptr_t)accs[m] & 7u)) return rh_fail(io.ctx, REAL_HIP_E_INVALID, "the mapping quality accumulators must be 8-byte aligned", hipSuccess);
        rc = io.inout(io.ctx->mapq.acc[m], accs[m], n, fresh != 0, d_accs[m]);
    }
    return rc;
}

extern "C" int real_hip_mapq_hits(real_hip_ctx *ctx, const real_hip_hit *hits, const uint64_t *off, uint64_t n_reads, int on_device, int fresh,
                                  real_hip_mapq_acc *acc)
{
    RH_ENTER(ctx);
    int rc;
    const uint64_t n = n_reads;
    if (!n) return REAL_HIP_OK;
    if (n > 0xffffffffull) return rh_fail(ctx, REAL_HIP_E_INVALID, "more than 2^32 reads in one call", hipSuccess);
    if (!off || !acc) return rh_fail(ctx, REAL_HIP_E_INVALID, "null offsets / accumulators", hipSuccess);
    const real_hip_hit *const hv[2] = {hits, nullptr};
    const uint64_t *const ov[2] = {off, nullptr};
    MateLists L;
    real_hip_mapq_acc *const av[1] = {acc};
    real_hip_mapq_acc *d_acc[2] = {nullptr, nullptr};
    const RhStaging io{ctx, !on_device, ctx->stream, ctx->stream};
    if ((rc = stage_hit_lists(ctx, hv, ov, nullptr, n, on_device != 0, L, 1))) return rc;
    rc = stage_mapq_accs(io, 1, av, n, fresh, d_acc);
    if (!rc) rc = rh_launch_mapq_fold(ctx, 1, L, n, fresh, d_acc);
    if (!rc) rc = io.back(acc, d_acc[0], n, "download of the mapping quality accumulators");
    return rh_sync_tail(ctx, rc);
}

extern "C" int real_hip_mapq_pair_hits(real_hip_ctx *ctx, const real_hip_pair_params *pp, const real_hip_hit *hits1, const uint64_t *off1,
                                       const uint32_t *len1, const real_hip_hit *hits2, const uint64_t *off2, const uint32_t *len2,
                                       uint64_t n_pairs, int on_device, int fresh, real_hip_mapq_acc *acc)
{
    RH_ENTER(ctx);
    int rc = pair_params_check(ctx, pp);
    if (rc) return rc;
    const uint64_t n = n_pairs;
    if (!n) return REAL_HIP_OK;
    if (n > 0xffffffffull) return rh_fail(ctx, REAL_HIP_E_INVALID, "more than 2^32 pairs in one call", hipSuccess);
    if (!off1 || !off2 || !len1 || !len2 || !acc) return rh_fail(ctx, REAL_HIP_E_INVALID, "null offsets / lengths / accumulators", hipSuccess);
    const real_hip_hit *const hits[2] = {hits1, hits2};
    const uint64_t *const off[2] = {off1, off2};
    const uint32_t *const len[2] = {len1, len2};
    MateLists L;
    real_hip_mapq_acc *const av[1] = {acc};
    real_hip_mapq_acc *d_acc[1] = {nullptr};
    const RhStaging io{ctx, !on_device, ctx->stream, ctx->stream};
    if ((rc = stage_hit_lists(ctx, hits, off, len, n, on_device != 0, L))) return rc;
    rc = stage_mapq_accs(io, 1, av, n, fresh, d_acc);
    if (!rc) rc = rh_launch_mapq_pair_fold(ctx, *pp, L, n, fresh, d_acc[0]);
    if (!rc) rc = io.back(acc, d_acc[0], n, "download of the mapping quality accumulators");
    return rh_sync_tail(ctx, rc);
}

// the finish of n reads (pairs null) or fragments
static int mapq_finish_run(real_hip_ctx *ctx, const uint64_t *info, const float *score, const real_hip_pair *pairs, const real_hip_single *const singles[2],
                           const real_hip_mapq_acc *const accs[3], uint64_t n, int on_device, uint8_t *out)
{
    int rc;
    RhMapqStage &S = ctx->mapq;
    const RhStaging io{ctx, !on_device, ctx->stream, ctx->stream};
    const bool have_singles = pairs && singles[0];
    if (!io.host && (((uintptr_t)pairs & 7u) || (have_singles && (((uintptr_t)singles[0] | (uintptr_t)singles[1]) & 15u))))
        return rh_fail(ctx, REAL_HIP_E_INVALID, "mapq: the pair records must be 8-byte, the single records 16-byte aligned", hipSuccess);
    const uint64_t *d_info = info;
    const float *d_score = score;
    const real_hip_pair *d_pairs = pairs;
    const real_hip_single *d_singles[2] = {nullptr, nullptr};
    const real_hip_mapq_acc *d_accs[3] = {nullptr, nullptr, nullptr};
    uint8_t *d_out = out;
    if (pairs) rc = io.in(S.rec, pairs, n, d_pairs);
    else rc = io.in(S.rec, info, n, d_info);
    if (!rc && score) rc = io.in(S.score, score, n, d_score);
    for (int m = 0; m < 2 && !rc && have_singles; ++m) rc = io.in(S.sg[m], singles[m], n, d_singles[m]);
    for (int m = 0; m < 3 && !rc; ++m) {
        if (!accs[m]) continue;
        if (!io.host && ((uintptr_t)accs[m] & 7u)) return rh_fail(ctx, REAL_HIP_E_INVALID, "the mapping quality accumulators must be 8-byte aligned", hipSuccess);
        rc = io.in(S.acc[m], accs[m], n, d_accs[m]);
    }
    const uint64_t n_out = pairs ? 2 * n : n;
    if (!rc) rc = io.inout(S.out, out, n_out, true, d_out); // (an output: nothing is uploaded)
    if (!rc) rc = rh_launch_mapq_finish(ctx, d_info, d_score, d_pairs, have_singles ? d_singles : nullptr, d_accs, n, d_out);
    if (!rc) rc = io.back(out, d_out, n_out, "download of the mapping qualities");
    return rh_sync_tail(ctx, rc);
}

extern "C" int real_hip_mapq(real_hip_ctx *ctx, const uint64_t *info, const float *score, const real_hip_mapq_acc *acc, uint64_t n, int on_device,
                             uint8_t *out)
{
    RH_ENTER(ctx);
    if (!n) return REAL_HIP_OK;
    if (n > 0xffffffffull) return stage_invalid(ctx, "mapq", "more than 2^32 reads in one call");
    if (!info || !acc || !out) return stage_invalid(ctx, "mapq", "null info / accumulators / out");
    if (ctx->prm.scores && !score) return stage_invalid(ctx, "mapq", "null score with scores on");
    const real_hip_mapq_acc *const accs[3] = {acc, nullptr, nullptr};
    return mapq_finish_run(ctx, info, ctx->prm.scores ? score : nullptr, nullptr, nullptr, accs, n, on_device, out);
}

extern "C" int real_hip_mapq_pairs(real_hip_ctx *ctx, const real_hip_pair *pairs, const real_hip_single *singles1, const real_hip_single *singles2,
                                   const real_hip_mapq_acc *acc_pair, const real_hip_mapq_acc *acc1, const real_hip_mapq_acc *acc2, uint64_t n,
                                   int on_device, uint8_t *out)
{
    RH_ENTER(ctx);
    if ((singles1 == nullptr) != (singles2 == nullptr)) return stage_invalid(ctx, "mapq", "one singles pointer without the other");
    if (!n) return REAL_HIP_OK;
    if (n > 0xffffffffull) return stage_invalid(ctx, "mapq", "more than 2^32 pairs in one call");
    if (!pairs || !acc_pair || !out) return stage_invalid(ctx, "mapq", "null pairs / accumulators / out");
    if (singles1 && (!acc1 || !acc2)) return stage_invalid(ctx, "mapq", "singles without the mates' accumulators");
    const real_hip_single *const singles[2] = {singles1, singles2};
    const real_hip_mapq_acc *const accs[3] = {acc_pair, singles1 ? acc1 : nullptr, singles1 ? acc2 : nullptr};
    return mapq_finish_run(ctx, nullptr, nullptr, pairs, singles, accs, n, on_device, out);
}

extern "C" int real_hip_mapq_stats_get(real_hip_ctx *ctx, real_hip_mapq_stats *out, int reset)
{
    return stats_get(ctx, out, reset, "mapq stats struct_size", rh_mapq_stats);
}

// ---- insert sizes (insert_hist.hip): staging as real_hip_pair_hits does it
extern "C" int real_hip_pair_insert_hist(real_hip_ctx *ctx, const real_hip_pair *pairs, const uint32_t *len1, const uint32_t *len2,
                                         uint64_t n_pairs, int on_device, int fresh, uint32_t n_bins, uint64_t *hist)
{
    RH_ENTER(ctx);
    if (n_bins < 2 || n_bins > REAL_HIP_INSERT_HIST_MAX_BINS)
        return rh_fail(ctx, REAL_HIP_E_INVALID, "n_bins must be in 2 .. REAL_HIP_INSERT_HIST_MAX_BINS", hipSuccess);
    const uint64_t n = n_pairs;
    if (n > 0xffffffffull) return rh_fail(ctx, REAL_HIP_E_INVALID, "more than 2^32 pairs in one call", hipSuccess);
    if (!hist || (n && (!pairs || !len1 || !len2))) return rh_fail(ctx, REAL_HIP_E_INVALID, "null pairs / lengths / hist", hipSuccess);
    if (on_device && ((uintptr_t)pairs & 7u)) return rh_fail(ctx, REAL_HIP_E_INVALID, "the pair records must be 8-byte aligned", hipSuccess);
    int rc;
    const real_hip_pair *d_pairs = pairs;
    const uint32_t *d_len[2] = {len1, len2};
    uint64_t *d_hist = hist;
    const RhStaging io{ctx, !on_device, ctx->stream, ctx->stream};
    if ((rc = io.inout(ctx->insert.hist, hist, n_bins, fresh != 0, d_hist))) return rc;
    if (n) {
        if ((rc = io.in(ctx->insert.rec, pairs, n, d_pairs))) return rc;
        for (int m = 0; m < 2; ++m)
            if ((rc = io.in(ctx->insert.len[m], m ? len2 : len1, n, d_len[m]))) return rc;
    }
    if (fresh) RH_HIP(ctx, hipMemsetAsync(d_hist, 0, (size_t)n_bins * 8, ctx->stream));
    rc = rh_launch_insert_hist(ctx, d_pairs, d_len[0], d_len[1], n, n_bins, d_hist);
    if (!rc) rc = io.back(hist, d_hist, n_bins, "download of the histogram");
    return rh_sync_tail(ctx, rc);
}

extern "C" int real_hip_insert_stats_get(real_hip_ctx *ctx, real_hip_insert_stats *out, int reset)
{
    return stats_get(ctx, out, reset, "insert stats struct_size", rh_insert_stats);
}

// the quartile rule on a histogram: host only, integers only (include/real_hip.h)
extern "C" int real_hip_insert_bounds(const uint64_t *hist, uint32_t n_bins, uint64_t min_count, uint32_t iqr_mult, real_hip_insert_estimate *out)
{
    if (!hist || !out || out->struct_size != sizeof(real_hip_insert_estimate) || n_bins < 2) return REAL_HIP_E_INVALID;
    uint64_t n = 0;
    for (uint32_t d = 0; d < n_bins; ++d) n += hist[d];
    out->reserved = 0; out->pad = 0;
    out->n = n;
    out->q1 = out->median = out->q3 = out->low = out->high = 0;
    if (n < min_count || !n) return REAL_HIP_E_STATE;
    uint32_t q[3] = {0, 0, 0};
    uint64_t cum = 0;
    uint32_t j = 0;
    for (uint32_t d = 0; d < n_bins && j < 3; ++d) {
        cum += hist[d];
        while (j < 3 && cum >= ((uint64_t)(j + 1) * n + 3) / 4) q[j++] = d;
    }
    out->q1 = q[0]; out->median = q[1]; out->q3 = q[2];
    if (q[2] == n_bins - 1) return REAL_HIP_E_OVERFLOW;
    const uint64_t reach = (uint64_t)iqr_mult * (q[2] - q[0]);
    out->low = q[0] - (uint32_t)(reach < q[0] ? reach : q[0]);
    const uint64_t high = q[2] + reach;
    out->high = high > 0xffffffffull ? 0xffffffffu : (uint32_t)high;
    return REAL_HIP_OK;
}

// ---- pileup (pileup.hip): the reads are staged as a match stages them, the records as the match's outputs
// the resident text is still the one begin saw (add reads it, finish takes the sites' reference bases from it)
static int pileup_text_check(real_hip_ctx *ctx)
{
    if (!ctx->have_text || ctx->n_bases != ctx->pileup.n || ctx->fileid != ctx->pileup.fileid)
        return rh_fail(ctx, REAL_HIP_E_INVALID, "pileup: the text was replaced since begin", hipSuccess);
    return REAL_HIP_OK;
}
static int pileup_add_check(real_hip_ctx *ctx)
{
    if (ctx->pileup.state == 0) return rh_fail(ctx, REAL_HIP_E_INVALID, "pileup: add without begin", hipSuccess);
    if (ctx->pileup.state == 2) return rh_fail(ctx, REAL_HIP_E_INVALID, "pileup: add after finish", hipSuccess);
    return pileup_text_check(ctx);
}

extern "C" int real_hip_pileup_begin(real_hip_ctx *ctx, const real_hip_pileup_params *p)
{
    RH_ENTER(ctx);
    if (!p || p->struct_size != sizeof(real_hip_pileup_params)) return rh_fail(ctx, REAL_HIP_E_INVALID, "pileup params struct_size", hipSuccess);
    if (p->min_qual > 63) return rh_fail(ctx, REAL_HIP_E_INVALID, "pileup: min_qual beyond 63", hipSuccess);
    if (!ctx->have_text) return rh_fail(ctx, REAL_HIP_E_STATE, "the text must be set", hipSuccess);
    return rh_pileup_begin(ctx, p->min_qual);
}

// Reads and the final records that place them, staged for the kernels: what real_hip_pileup_add*, real_hip_call_add* and
// real_hip_mismatches* share.  bv[]: the views of the reads (mates == 1, with info) or of the two mates (mates == 2, with
// pairs; mates_agree has checked them).  At most 2^32 reads, the null and alignment checks on the records, then the reads as a match stages
// them into ctx->stage[m], then the records into `rec` where they are host memory, then the device views.  keep_qual: the
// qualities are handed on whatever -q says; otherwise not at all.  n_reads == 0 is valid: nothing is copied.  need_rec false:
// the stage takes null records (anchored gap placement: every read is eligible).
struct PlacedReads {
    DevBatch b[2];
    const uint64_t *info;
    const real_hip_pair *pairs;
};
static int stage_placements(real_hip_ctx *ctx, const char *stage, const real_hip_batch bv[], int mates, const uint64_t *info, const real_hip_pair *pairs,
                            DevBuf &rec, bool keep_qual, PlacedReads &p, bool need_rec = true)
{
    const uint64_t n = bv[0].n_reads;
    const bool dev = bv[0].on_device == 1;
    if (n > 0xffffffffull) return stage_invalid(ctx, stage, "more than 2^32 reads in one call");
    if (n && need_rec && !(mates == 2 ? (const void *)pairs : (const void *)info)) return stage_invalid(ctx, stage, mates == 2 ? "null pairs" : "null info");
    if (dev && ((uintptr_t)pairs & 7u)) return stage_invalid(ctx, stage, "the pair records must be 8-byte aligned");
    int rc;
    Staged st[2];
    for (int m = 0; m < mates; ++m)
        if ((rc = stage_batch(ctx, bv[m], st[m], ctx->stage[m], ctx->stream, nullptr, false))) return rc;
    const RhStaging io{ctx, !dev, ctx->stream, ctx->stream};
    p.info = info; p.pairs = pairs;
    if (n && (pairs || info) && (rc = mates == 2 ? io.in(rec, pairs, n, p.pairs) : io.in(rec, info, n, p.info))) return rc;
    for (int m = 0; m < mates; ++m) {
        p.b[m] = dev_batch(ctx, st[m], n);
        p.b[m].qual = keep_qual ? st[m].qual : nullptr;
    }
    return REAL_HIP_OK;
}

// The same for the stages that consume gap records (real_hip_mismatches_gapped, real_hip_indel_add, real_hip_pileup_add_gapped,
// real_hip_call_add_gapped): bv[] are the views of the two mates (mates_agree has checked them).  At most 2^32
// fragments, the null and alignment checks on the records, then both mates' reads into ctx->stage[m], then the records into
// `rec` where they are host memory, then the device views.  n_reads == 0 is valid: nothing is copied.
struct GappedReads {
    DevBatch b[2];
    const real_hip_gap_place *gaps;
};
static int stage_gapped(real_hip_ctx *ctx, const char *stage, const real_hip_batch bv[2], const real_hip_gap_place *gaps, DevBuf &rec, bool keep_qual,
                        GappedReads &p)
{
    const uint64_t n = bv[0].n_reads;
    const bool dev = bv[0].on_device == 1;
    if (n > 0xffffffffull) return stage_invalid(ctx, stage, "more than 2^32 fragments in one call");
    if (n && !gaps) return stage_invalid(ctx, stage, "null gaps");
    if (dev && ((uintptr_t)gaps & 15u)) return stage_invalid(ctx, stage, "the gap records must be 16-byte aligned");
    int rc;
    Staged st[2];
    for (int m = 0; m < 2; ++m)
        if ((rc = stage_batch(ctx, bv[m], st[m], ctx->stage[m], ctx->stream, nullptr, false))) return rc;
    const RhStaging io{ctx, !dev, ctx->stream, ctx->stream};
    p.gaps = gaps;
    if (n && (rc = io.in(rec, gaps, n, p.gaps))) return rc;
    for (int m = 0; m < 2; ++m) {
        p.b[m] = dev_batch(ctx, st[m], n);
        p.b[m].qual = keep_qual ? st[m].qual : nullptr; // (handed on whatever -q says, as the pileup does; or not at all)
    }
    return REAL_HIP_OK;
}

// what real_hip_pileup_add* and real_hip_call_add* share: both hand the placements of a batch to a kernel of their own
struct PlacementSink {
    const char *name;                    // the prefix of its messages
    int (*check)(real_hip_ctx *);        // may an add come now
    DevBuf &(*rec)(real_hip_ctx *);      // the staged records when the caller's are host memory
    int (*launch)(real_hip_ctx *, const DevBatch &, const uint64_t *, const real_hip_pair *, uint32_t);
};
// the placements of a batch (mates == 1: b1 and info) or of both mates of a batch of pairs (mates == 2: b1, b2 and pairs)
static int placements_add(real_hip_ctx *ctx, const PlacementSink &k, int mates, const real_hip_batch *b1, const real_hip_batch *b2, const uint64_t *info,
                          const real_hip_pair *pairs)
{
    real_hip_batch bv[2];
    int rc = mates == 2 ? mates_view(ctx, k.name, b1, b2, false, bv) : batch_view(ctx, b1, bv[0]);
    if (rc || (rc = k.check(ctx))) return rc;
    if (!bv[0].n_reads) return REAL_HIP_OK;
    PlacedReads p;
    rc = stage_placements(ctx, k.name, bv, mates, info, pairs, k.rec(ctx), true, p);
    for (int m = 0; m < mates && !rc; ++m) rc = k.launch(ctx, p.b[m], p.info, p.pairs, (uint32_t)m);
    return rh_sync_tail(ctx, rc);
}

static const PlacementSink kPileupSink = {"pileup", pileup_add_check, [](real_hip_ctx *c) -> DevBuf & { return c->pileup.rec; }, rh_launch_pileup_add};

extern "C" int real_hip_pileup_add(real_hip_ctx *ctx, const real_hip_batch *b, const uint64_t *info)
{
    RH_ENTER(ctx);
    return placements_add(ctx, kPileupSink, 1, b, nullptr, info, nullptr);
}

extern "C" int real_hip_pileup_add_pairs(real_hip_ctx *ctx, const real_hip_batch *b1, const real_hip_batch *b2, const real_hip_pair *pairs)
{
    RH_ENTER(ctx);
    return placements_add(ctx, kPileupSink, 2, b1, b2, nullptr, pairs);
}

extern "C" int real_hip_pileup_finish(real_hip_ctx *ctx, uint64_t *n_sites)
{
    RH_ENTER(ctx);
    if (ctx->pileup.state != 1) return rh_fail(ctx, REAL_HIP_E_INVALID, ctx->pileup.state ? "pileup: finish twice" : "pileup: finish without begin", hipSuccess);
    int rc = pileup_text_check(ctx);
    if (rc) return rc;
    return finish_tail(ctx, rh_sync_tail(ctx, rh_pileup_finish(ctx, n_sites)), rh_pileup_end); // (a failed finish: the pileup is over, as after end)
}

extern "C" int real_hip_pileup_depth(real_hip_ctx *ctx, uint64_t first, uint64_t count, uint32_t *depth, int on_device)
{
    RH_ENTER(ctx);
    if (ctx->pileup.state != 2) return rh_fail(ctx, REAL_HIP_E_INVALID, "pileup: depth before finish", hipSuccess);
    if (first > ctx->pileup.n || count > ctx->pileup.n - first) return rh_fail(ctx, REAL_HIP_E_INVALID, "pileup: the depth window reaches beyond the text", hipSuccess);
    if (!count) return REAL_HIP_OK;
    if (!depth) return rh_fail(ctx, REAL_HIP_E_INVALID, "pileup: null depth", hipSuccess);
    RH_HIP(ctx, hipMemcpyAsync(depth, (const uint32_t *)ctx->pileup.diff.p + first, (size_t)count * 4,
                               on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    return rh_sync_tail(ctx, REAL_HIP_OK);
}

extern "C" int real_hip_pileup_sites(real_hip_ctx *ctx, real_hip_pileup_site *out, uint64_t cap, uint64_t *n_out, int on_device)
{
    RH_ENTER(ctx);
    return list_out(ctx, ctx->pileup.state == 2, "pileup", "sites", "site list", ctx->pileup.sites.p, ctx->pileup.n_sites, sizeof(real_hip_pileup_site), out, cap, n_out, on_device);
}

extern "C" int real_hip_pileup_end(real_hip_ctx *ctx)
{
    RH_ENTER(ctx);
    rh_pileup_end(ctx);
    return REAL_HIP_OK;
}

extern "C" int real_hip_pileup_stats_get(real_hip_ctx *ctx, real_hip_pileup_stats *out, int reset)
{
    return stats_get(ctx, out, reset, "pileup stats struct_size", rh_pileup_stats);
}

// ---- variant calls (snp_call.hip): on top of the finished pileup; the reads and records are staged as the pileup stages them
static int call_pileup_check(real_hip_ctx *ctx, const char *unfinished)
{
    if (ctx->pileup.state != 2) return rh_fail(ctx, REAL_HIP_E_INVALID, unfinished, hipSuccess);
    if (!ctx->have_text || ctx->n_bases != ctx->pileup.n || ctx->fileid != ctx->pileup.fileid)
        return rh_fail(ctx, REAL_HIP_E_INVALID, "calls: the text was replaced since the pileup's begin", hipSuccess);
    return REAL_HIP_OK;
}
static int call_add_check(real_hip_ctx *ctx)
{
    if (ctx->call.state == 0) return rh_fail(ctx, REAL_HIP_E_INVALID, "calls: add without begin", hipSuccess);
    if (ctx->call.state == 2) return rh_fail(ctx, REAL_HIP_E_INVALID, "calls: add after finish", hipSuccess);
    return call_pileup_check(ctx, "calls: add without a finished pileup");
}
static const PlacementSink kCallSink = {"calls", call_add_check, [](real_hip_ctx *c) -> DevBuf & { return c->call.rec; }, rh_launch_call_add};

extern "C" int real_hip_call_begin(real_hip_ctx *ctx)
{
    RH_ENTER(ctx);
    int rc = call_pileup_check(ctx, "calls: begin needs a finished pileup");
    if (rc) return rc;
    return rh_sync_tail(ctx, rh_call_begin(ctx));
}

extern "C" int real_hip_call_add(real_hip_ctx *ctx, const real_hip_batch *b, const uint64_t *info)
{
    RH_ENTER(ctx);
    return placements_add(ctx, kCallSink, 1, b, nullptr, info, nullptr);
}

extern "C" int real_hip_call_add_pairs(real_hip_ctx *ctx, const real_hip_batch *b1, const real_hip_batch *b2, const real_hip_pair *pairs)
{
    RH_ENTER(ctx);
    return placements_add(ctx, kCallSink, 2, b1, b2, nullptr, pairs);
}

extern "C" int real_hip_call_finish(real_hip_ctx *ctx, const real_hip_call_params *p, uint64_t *n_calls)
{
    RH_ENTER(ctx);
    if (!p || p->struct_size != sizeof(real_hip_call_params)) return rh_fail(ctx, REAL_HIP_E_INVALID, "call params struct_size", hipSuccess);
    if (ctx->call.state == 0) return rh_fail(ctx, REAL_HIP_E_INVALID, "calls: finish without begin", hipSuccess);
    int rc = call_pileup_check(ctx, "calls: finish without a finished pileup");
    if (rc) return rc;
    return finish_tail(ctx, rh_sync_tail(ctx, rh_call_finish(ctx, p->min_call_qual, p->min_depth, n_calls)), rh_call_release);
}

extern "C" int real_hip_call_evidence(real_hip_ctx *ctx, real_hip_call_evidence_rec *out, uint64_t cap, uint64_t *n_out, int on_device)
{
    RH_ENTER(ctx);
    return list_out(ctx, ctx->call.state == 2, "calls", "evidence", "evidence list", ctx->call.ev.p, ctx->pileup.n_sites, sizeof(real_hip_call_evidence_rec), out, cap, n_out, on_device);
}

extern "C" int real_hip_call_variants(real_hip_ctx *ctx, real_hip_call *out, uint64_t cap, uint64_t *n_out, int on_device)
{
    RH_ENTER(ctx);
    return list_out(ctx, ctx->call.state == 2, "calls", "variants", "variants list", ctx->call.calls.p, ctx->call.n_calls, sizeof(real_hip_call), out, cap, n_out, on_device);
}

extern "C" int real_hip_call_end(real_hip_ctx *ctx)
{
    RH_ENTER(ctx);
    (void)hipStreamSynchronize(ctx->stream);
    rh_call_release(ctx);
    return REAL_HIP_OK;
}

extern "C" int real_hip_call_stats_get(real_hip_ctx *ctx, real_hip_call_stats *out, int reset)
{
    return stats_get(ctx, out, reset, "call stats struct_size", rh_call_stats);
}

// ---- mismatch lists (mismatch_list.hip): the reads are staged as the pileup stages them, the records as the match's outputs;
// count, then -- the total being known -- the overflow decision, then the lists (pair_all_run's protocol)
static const char *const kMismatch = "mismatch lists";
static int mismatch_outputs_check(real_hip_ctx *ctx, const real_hip_mismatch *out, uint64_t cap, uint64_t *n_out, const uint64_t *mm_offsets, bool dev_out,
                                  const char *stage = kMismatch)
{
    if (!mm_offsets || !n_out) return stage_invalid(ctx, stage, "null mm_offsets / n_out");
    *n_out = 0;
    if (cap && !out) return stage_invalid(ctx, stage, "null out");
    if (dev_out && ((uintptr_t)out & 3u)) return stage_invalid(ctx, stage, "out must be 4-byte aligned");
    return REAL_HIP_OK;
}
static int mismatch_run(real_hip_ctx *ctx, const RhStaging &io, const RhMismatchLaunch l[], int n_launch, real_hip_mismatch *out, uint64_t cap,
                        uint64_t *n_out, uint64_t *mm_offsets)
{
    const uint64_t lists = l[0].b.n_reads * (uint64_t)n_launch;
    uint64_t *d_off = mm_offsets;
    int rc;
    if ((rc = io.inout(ctx->mismatch.off, mm_offsets, lists + 1, true, d_off))) return rc; // (outputs: nothing is uploaded)
    uint64_t total = 0;
    if ((rc = rh_mismatch_count(ctx, l, n_launch, d_off, &total))) return rc;
    *n_out = total;
    if ((rc = io.back(mm_offsets, d_off, lists + 1, "download of the mismatch offsets"))) return rc;
    if (total > cap) return rh_fail(ctx, REAL_HIP_E_OVERFLOW, "mismatch lists: the buffer needs more room", hipSuccess);
    real_hip_mismatch *d_out = out;
    if ((rc = io.inout(ctx->mismatch.out, out, total, true, d_out, sizeof(real_hip_mismatch)))) return rc;
    if ((rc = rh_mismatch_emit(ctx, l, n_launch, d_off, d_out, total))) return rc;
    return io.back(out, d_out, total, "download of the mismatch lists");
}

extern "C" int real_hip_mismatches(real_hip_ctx *ctx, const real_hip_batch *b, const uint64_t *info, real_hip_mismatch *out, uint64_t cap,
                                   uint64_t *n_out, uint64_t *mm_offsets)
{
    RH_ENTER(ctx);
    real_hip_batch bv;
    int rc = batch_view(ctx, b, bv);
    if (rc || (rc = mismatch_outputs_check(ctx, out, cap, n_out, mm_offsets, bv.on_device == 1))) return rc;
    PlacedReads p;
    if ((rc = stage_placements(ctx, kMismatch, &bv, 1, info, nullptr, ctx->mismatch.rec, false, p))) return rh_sync_tail(ctx, rc);
    const RhStaging io{ctx, bv.on_device != 1, ctx->stream, ctx->stream};
    const RhMismatchLaunch l{p.b[0], p.info, nullptr, nullptr};
    return rh_sync_tail(ctx, mismatch_run(ctx, io, &l, 1, out, cap, n_out, mm_offsets)); // (n == 0 too: mm_offsets[0] is written)
}

extern "C" int real_hip_mismatches_pairs(real_hip_ctx *ctx, const real_hip_batch *b1, const real_hip_batch *b2, const real_hip_pair *pairs,
                                         const real_hip_single *singles1, const real_hip_single *singles2, real_hip_mismatch *out, uint64_t cap,
                                         uint64_t *n_out, uint64_t *mm_offsets)
{
    RH_ENTER(ctx);
    real_hip_batch bv[2];
    int rc;
    if ((rc = batch_view(ctx, b1, bv[0])) || (rc = batch_view(ctx, b2, bv[1]))) return rc;
    const bool dev = bv[0].on_device == 1;
    if ((rc = mismatch_outputs_check(ctx, out, cap, n_out, mm_offsets, dev)) || (rc = mates_agree(ctx, kMismatch, bv, false))) return rc;
    if ((singles1 != nullptr) != (singles2 != nullptr)) return stage_invalid(ctx, kMismatch, "one singles array without the other");
    if (dev && (((uintptr_t)singles1 | (uintptr_t)singles2) & 15u)) return stage_invalid(ctx, kMismatch, "the single records must be 16-byte aligned");
    const uint64_t n = bv[0].n_reads;
    PlacedReads p;
    if ((rc = stage_placements(ctx, kMismatch, bv, 2, nullptr, pairs, ctx->mismatch.rec, false, p))) return rh_sync_tail(ctx, rc);
    const RhStaging io{ctx, !dev, ctx->stream, ctx->stream};
    RhMismatchLaunch l[2] = {{p.b[0], nullptr, p.pairs, singles1}, {p.b[1], nullptr, p.pairs, singles2}};
    for (int m = 0; m < 2 && !rc && n && singles1; ++m) rc = io.in(ctx->mismatch.sg[m], m ? singles2 : singles1, n, l[m].singles);
    if (!rc) rc = mismatch_run(ctx, io, l, 2, out, cap, n_out, mm_offsets);
    return rh_sync_tail(ctx, rc);
}

extern "C" int real_hip_mismatch_stats_get(real_hip_ctx *ctx, real_hip_mismatch_stats *out, int reset)
{
    return stats_get(ctx, out, reset, "mismatch stats struct_size", rh_mismatch_stats);
}

// ---- gap rescue (gap_rescue.hip): the reads and the pair records are staged as the mismatch lists stage them, the singles and
// the in/out gap records beside them
static const char *const kGap = "gap rescue";
// what real_hip_gap_params may hold, for both stages that take it; `stage` is the prefix of the messages
static int gap_costs_check(real_hip_ctx *ctx, const char *stage, const real_hip_gap_params *gp)
{
    if (!gp || gp->struct_size != sizeof(real_hip_gap_params)) return stage_invalid(ctx, stage, "params struct_size");
    if (gp->max_gap < 1 || gp->max_gap > REAL_HIP_GAP_MAX) return stage_invalid(ctx, stage, "max_gap must be in 1 .. REAL_HIP_GAP_MAX");
    if (gp->min_flank < 1) return stage_invalid(ctx, stage, "min_flank must be at least 1");
    if (gp->cost_mismatch > 65535u || gp->cost_open > 65535u || gp->cost_extend > 65535u) return stage_invalid(ctx, stage, "a cost beyond 65535");
    if (gp->max_cost > 65534u) return stage_invalid(ctx, stage, "max_cost beyond 65534");
    if (gp->margin > 65535u) return stage_invalid(ctx, stage, "margin beyond 65535");
    if (gp->reserved[0] || gp->reserved[1]) return stage_invalid(ctx, stage, "reserved words must be 0");
    return REAL_HIP_OK;
}
static int gap_params_check(real_hip_ctx *ctx, const real_hip_pair_params *pp, const real_hip_gap_params *gp)
{
    if (!gp || gp->struct_size != sizeof(real_hip_gap_params)) return stage_invalid(ctx, kGap, "params struct_size");
    if (pp->max_insert > REAL_HIP_MATE_SEARCH_MAX_INSERT)
        return rh_fail(ctx, REAL_HIP_E_UNSUPPORTED, "gap rescue: max_insert beyond REAL_HIP_MATE_SEARCH_MAX_INSERT", hipSuccess);
    return gap_costs_check(ctx, kGap, gp);
}

extern "C" int real_hip_gap_rescue(real_hip_ctx *ctx, const real_hip_pair_params *pp, const real_hip_gap_params *gp, const real_hip_batch *b1,
                                   const real_hip_batch *b2, const real_hip_pair *pairs, const real_hip_single *singles1, const real_hip_single *singles2,
                                   int fresh, real_hip_gap_place *out)
{
    RH_ENTER(ctx);
    int rc = pair_params_check(ctx, pp);
    if (rc || (rc = gap_params_check(ctx, pp, gp))) return rc;
    real_hip_batch bv[2];
    if ((rc = mates_view(ctx, kGap, b1, b2, false, bv))) return rc;
    const bool dev = bv[0].on_device == 1;
    const uint64_t n = bv[0].n_reads;
    if (n && (!singles1 || !singles2 || !out)) return stage_invalid(ctx, kGap, "null singles / out");
    if (dev && (((uintptr_t)singles1 | (uintptr_t)singles2 | (uintptr_t)out) & 15u)) return stage_invalid(ctx, kGap, "the single and the gap records must be 16-byte aligned");
    RhGapStage &S = ctx->gap;
    PlacedReads p;
    if ((rc = stage_placements(ctx, kGap, bv, 2, nullptr, pairs, S.rec, false, p))) return rh_sync_tail(ctx, rc);
    if (!n) return REAL_HIP_OK;
    const RhStaging io{ctx, !dev, ctx->stream, ctx->stream};
    const real_hip_single *d_singles[2] = {singles1, singles2};
    real_hip_gap_place *d_out = out;
    for (int m = 0; m < 2 && !rc; ++m) rc = io.in(S.sg[m], m ? singles2 : singles1, n, d_singles[m]);
    if (!rc) rc = io.inout(S.out, out, n, fresh != 0, d_out);
    if (!rc) rc = rh_launch_gap_rescue(ctx, *pp, *gp, p.b[0], p.b[1], p.pairs, d_singles, n, fresh, d_out);
    if (!rc) rc = io.back(out, d_out, n, "download of the gap records");
    rc = rh_sync_tail(ctx, rc);
    return rc ? rc : rh_gap_finish(ctx);
}

extern "C" int real_hip_gap_stats_get(real_hip_ctx *ctx, real_hip_gap_stats *out, int reset)
{
    return stats_get(ctx, out, reset, "gap stats struct_size", rh_gap_stats);
}

// ---- anchored gap placement (gap_anchor.hip): the reads and the info words are staged as the mismatch lists stage them
// (qualities kept: the sub-reads carry them to the matcher), the in/out gap records beside them.  Every check comes before
// the first launch
static const char *const kAnchor = "anchored gap placement";
static int anchor_checks(real_hip_ctx *ctx, const real_hip_gap_params *gp, const real_hip_gap_anchor_params *ap, const real_hip_batch *batch,
                         const uint64_t *info, const real_hip_gap_place *out, bool need_index, real_hip_batch &bv)
{
    int rc = gap_costs_check(ctx, kAnchor, gp);
    if (rc) return rc;
    if (!ap || ap->struct_size != sizeof(real_hip_gap_anchor_params)) return stage_invalid(ctx, kAnchor, "anchor params struct_size");
    if (ap->anchor_len < 1 || ap->anchor_len > REAL_HIP_MAX_PATL) return stage_invalid(ctx, kAnchor, "anchor_len must be in 1 .. REAL_HIP_MAX_PATL");
    if (ap->max_anchors < 1 || ap->max_anchors > REAL_HIP_GAP_ANCHORS_MAX) return stage_invalid(ctx, kAnchor, "max_anchors must be in 1 .. REAL_HIP_GAP_ANCHORS_MAX");
    if (ap->reserved[0] || ap->reserved[1]) return stage_invalid(ctx, kAnchor, "reserved words of the anchor params must be 0");
    if ((rc = batch_view(ctx, batch, bv))) return rc;
    if (!ctx->have_text || (need_index && !ctx->have_index))
        return rh_fail(ctx, REAL_HIP_E_STATE, need_index ? "text and index must be set" : "the text must be set", hipSuccess);
    if (bv.n_reads > 0xffffffffull) return stage_invalid(ctx, kAnchor, "more than 2^32 reads in one call");
    if (bv.n_reads && !out) return stage_invalid(ctx, kAnchor, "null out");
    if (bv.on_device == 1 && ((uintptr_t)out & 15u)) return stage_invalid(ctx, kAnchor, "the gap records must be 16-byte aligned");
    if (bv.on_device == 1 && ((uintptr_t)info & 7u)) return stage_invalid(ctx, kAnchor, "the info words must be 8-byte aligned");
    return REAL_HIP_OK;
}
// the reads, info words and gap records staged -> what the launchers take
static int anchor_stage(real_hip_ctx *ctx, const real_hip_gap_params *gp, const real_hip_gap_anchor_params *ap, const real_hip_batch &bv,
                        const uint64_t *info, int fresh, real_hip_gap_place *out, const RhStaging &io, RhAnchorRun &r)
{
    RhGapStage &S = ctx->gap;
    PlacedReads p;
    int rc;
    if ((rc = stage_placements(ctx, kAnchor, &bv, 1, info, nullptr, S.an_info, true, p, false))) return rc;
    r.gp = *gp; r.ap = *ap; r.b = p.b[0]; r.d_info = info ? p.info : nullptr; r.n = bv.n_reads; r.fresh = fresh; r.d_out = out;
    return io.inout(S.an_out, out, r.n, fresh != 0, r.d_out);
}

extern "C" int real_hip_gap_anchor_hits(real_hip_ctx *ctx, const real_hip_gap_params *gp, const real_hip_gap_anchor_params *ap, const real_hip_batch *batch,
                                        const uint64_t *info, const real_hip_hit *hits, const uint64_t *hit_offsets, int fresh, real_hip_gap_place *out)
{
    RH_ENTER(ctx);
    real_hip_batch bv;
    int rc = anchor_checks(ctx, gp, ap, batch, info, out, false, bv);
    if (rc) return rc;
    const uint64_t n = bv.n_reads;
    if (!n) return REAL_HIP_OK;
    const bool dev = bv.on_device == 1;
    if (!hit_offsets) return stage_invalid(ctx, kAnchor, "null hit_offsets");
    if (dev && (((uintptr_t)hits & 15u) || ((uintptr_t)hit_offsets & 7u))) return stage_invalid(ctx, kAnchor, "the hits must be 16-byte, their offsets 8-byte aligned");
    const RhStaging io{ctx, !dev, ctx->stream, ctx->stream};
    const real_hip_hit *const hv[2] = {hits, nullptr};
    const uint64_t *const ov[2] = {hit_offsets, nullptr};
    MateLists L;
    RhAnchorRun r;
    if ((rc = stage_hit_lists(ctx, hv, ov, nullptr, 2 * n, dev, L, 1))) return rh_sync_tail(ctx, rc); // (a device list: its ends are read back)
    if ((rc = anchor_stage(ctx, gp, ap, bv, info, fresh, out, io, r))) return rh_sync_tail(ctx, rc);
    rc = rh_gap_anchor_select(ctx, r, nullptr);
    if (!rc) rc = rh_gap_anchor_search(ctx, r, (const real_hip_hit *)L.h[0], L.o[0], L.total[0], false);
    if (!rc) rc = io.back(out, r.d_out, n, "download of the gap records");
    rc = rh_sync_tail(ctx, rc);
    return rc ? rc : rh_gap_anchor_finish(ctx);
}

extern "C" int real_hip_match_gapped(real_hip_ctx *ctx, const real_hip_gap_params *gp, const real_hip_gap_anchor_params *ap, const real_hip_batch *batch,
                                     const uint64_t *info, int fresh, real_hip_gap_place *out)
{
    RH_ENTER(ctx);
    real_hip_batch bv;
    int rc = anchor_checks(ctx, gp, ap, batch, info, out, true, bv);
    if (rc) return rc;
    const uint64_t n = bv.n_reads;
    if (!n) return REAL_HIP_OK;
    const RhStaging io{ctx, bv.on_device != 1, ctx->stream, ctx->stream};
    RhGapStage &S = ctx->gap;
    RhAnchorRun r;
    uint64_t count = 0, total = 0;
    if ((rc = anchor_stage(ctx, gp, ap, bv, info, fresh, out, io, r))) return rh_sync_tail(ctx, rc);
    if ((rc = rh_gap_anchor_select(ctx, r, &count))) return rh_sync_tail(ctx, rc);
    if (count) {
        // the listed reads' sub-reads as a device batch of uniform length, matched with the hits left on the device; the
        // buffer only ever grows: a match that needs more reports the size and is done again
        real_hip_batch sub;
        memset(&sub, 0, sizeof sub);
        sub.struct_size = sizeof sub; sub.on_device = 1; sub.n_reads = 2 * count; sub.patl = ap->anchor_len;
        if ((rc = rh_gap_anchor_extract(ctx, r, count, &sub.bases, &sub.qual))) return rh_sync_tail(ctx, rc);
        if ((rc = rh_reserve(ctx, S.an_off, (2 * count + 1) * 8))) return rh_sync_tail(ctx, rc);
        uint64_t want = 2 * count + count / 2 + 1024;
        for (int attempt = 0;; ++attempt) {
            if ((rc = rh_reserve(ctx, S.an_hits, want * sizeof(real_hip_hit)))) return rh_sync_tail(ctx, rc);
            rc = match_all_run(ctx, sub, true, (real_hip_hit *)S.an_hits.p, S.an_hits.cap / sizeof(real_hip_hit), &total, (uint64_t *)S.an_off.p, nullptr);
            if (rc != REAL_HIP_E_OVERFLOW) break;
            if (attempt >= 2) return rh_fail(ctx, REAL_HIP_E_OVERFLOW, "anchored gap placement: the hit buffer kept overflowing", hipSuccess);
            if (total > 0xffffffffull) return rh_fail(ctx, REAL_HIP_E_OVERFLOW, "anchored gap placement: more than 2^32 anchor hits in one batch", hipSuccess);
            want = total;
        }
        if (rc) return rc;
        rc = rh_gap_anchor_search(ctx, r, (const real_hip_hit *)S.an_hits.p, (const uint64_t *)S.an_off.p, total, true);
    }
    if (!rc) rc = io.back(out, r.d_out, n, "download of the gap records");
    rc = rh_sync_tail(ctx, rc);
    return rc ? rc : rh_gap_anchor_finish(ctx);
}

extern "C" int real_hip_gap_anchor_stats_get(real_hip_ctx *ctx, real_hip_gap_anchor_stats *out, int reset)
{
    return stats_get(ctx, out, reset, "gap anchor stats struct_size", rh_gap_anchor_stats);
}

// ---- gapped mismatch lists (gapped_list.hip): reads and gap records through stage_gapped, without the qualities; count, the
// overflow decision, then the lists (mismatch_run's protocol)
static const char *const kGapped = "gapped mismatch lists";
extern "C" int real_hip_mismatches_gapped(real_hip_ctx *ctx, const real_hip_batch *b1, const real_hip_batch *b2, const real_hip_gap_place *gaps,
                                          real_hip_mismatch *out, uint64_t cap, uint64_t *n_out, uint64_t *mm_offsets)
{
    RH_ENTER(ctx);
    real_hip_batch bv[2];
    int rc;
    if ((rc = batch_view(ctx, b1, bv[0])) || (rc = batch_view(ctx, b2, bv[1]))) return rc;
    const bool dev = bv[0].on_device == 1;
    if ((rc = mismatch_outputs_check(ctx, out, cap, n_out, mm_offsets, dev, kGapped)) || (rc = mates_agree(ctx, kGapped, bv, false))) return rc;
    const uint64_t n = bv[0].n_reads;
    RhGapStage &S = ctx->gap;
    GappedReads p;
    if ((rc = stage_gapped(ctx, kGapped, bv, gaps, S.gl_rec, false, p))) return rh_sync_tail(ctx, rc); // (n == 0 goes on: offsets of one entry)
    const RhStaging io{ctx, !dev, ctx->stream, ctx->stream};
    uint64_t *d_off = mm_offsets;
    real_hip_mismatch *d_out = out;
    uint64_t total = 0;
    rc = io.inout(S.gl_off, mm_offsets, n + 1, true, d_off); // (outputs: nothing is uploaded)
    if (!rc) rc = rh_gapped_list_count(ctx, p.b[0], p.b[1], p.gaps, n, d_off, &total);
    if (!rc) {
        *n_out = total;
        rc = io.back(mm_offsets, d_off, n + 1, "download of the gapped mismatch offsets");
    }
    if (!rc && total > cap) rc = rh_fail(ctx, REAL_HIP_E_OVERFLOW, "gapped mismatch lists: the buffer needs more room", hipSuccess);
    if (!rc) rc = io.inout(S.gl_out, out, total, true, d_out, sizeof(real_hip_mismatch));
    if (!rc) rc = rh_gapped_list_emit(ctx, p.b[0], p.b[1], p.gaps, n, d_off, d_out, total);
    if (!rc) rc = io.back(out, d_out, total, "download of the gapped mismatch lists");
    return rh_sync_tail(ctx, rc);
}

extern "C" int real_hip_gapped_list_stats_get(real_hip_ctx *ctx, real_hip_gapped_list_stats *out, int reset)
{
    return stats_get(ctx, out, reset, "gapped list stats struct_size", rh_gapped_list_stats);
}

// ---- indel calls (indel_call.hip): on top of the finished pileup; reads and gap records through stage_gapped, with the
// qualities.  Every check comes before the first launch
static const char *const kIndel = "indel calls";
static int indel_pileup_check(real_hip_ctx *ctx, const char *unfinished)
{
    if (ctx->pileup.state != 2) return stage_invalid(ctx, kIndel, unfinished);
    if (!ctx->have_text || ctx->n_bases != ctx->pileup.n || ctx->fileid != ctx->pileup.fileid)
        return stage_invalid(ctx, kIndel, "the text was replaced since the pileup's begin");
    return REAL_HIP_OK;
}

extern "C" int real_hip_indel_begin(real_hip_ctx *ctx)
{
    RH_ENTER(ctx);
    int rc = indel_pileup_check(ctx, "begin needs a finished pileup");
    if (rc) return rc;
    return rh_sync_tail(ctx, rh_indel_begin(ctx));
}

extern "C" int real_hip_indel_add(real_hip_ctx *ctx, const real_hip_batch *b1, const real_hip_batch *b2, const real_hip_gap_place *gaps)
{
    RH_ENTER(ctx);
    real_hip_batch bv[2];
    int rc;
    if ((rc = mates_view(ctx, kIndel, b1, b2, false, bv))) return rc;
    RhIndelStage &S = ctx->indel;
    if (S.state == 0) return stage_invalid(ctx, kIndel, "add without begin");
    if (S.state == 2) return stage_invalid(ctx, kIndel, "add after finish");
    if ((rc = indel_pileup_check(ctx, "add without a finished pileup"))) return rc;
    GappedReads p;
    if ((rc = stage_gapped(ctx, kIndel, bv, gaps, S.rec, true, p))) return rh_sync_tail(ctx, rc);
    if (!bv[0].n_reads) return REAL_HIP_OK;
    return rh_sync_tail(ctx, rh_indel_add(ctx, p.b[0], p.b[1], p.gaps, bv[0].n_reads));
}

extern "C" int real_hip_indel_finish(real_hip_ctx *ctx, const real_hip_indel_params *p, uint64_t *n_events, uint64_t *n_calls)
{
    RH_ENTER(ctx);
    if (!p || p->struct_size != sizeof(real_hip_indel_params)) return stage_invalid(ctx, kIndel, "params struct_size");
    if (ctx->indel.state == 0) return stage_invalid(ctx, kIndel, "finish without begin");
    int rc = indel_pileup_check(ctx, "finish without a finished pileup");
    if (rc) return rc;
    return finish_tail(ctx, rh_sync_tail(ctx, rh_indel_finish(ctx, *p, n_events, n_calls)), rh_indel_release);
}

extern "C" int real_hip_indel_events(real_hip_ctx *ctx, real_hip_indel *out, uint64_t cap, uint64_t *n_out, int on_device)
{
    RH_ENTER(ctx);
    RhIndelStage &S = ctx->indel;
    return list_out(ctx, S.state == 2, kIndel, "events", "event list", S.events.p, S.n_groups, sizeof(real_hip_indel), out, cap, n_out, on_device);
}

extern "C" int real_hip_indel_calls(real_hip_ctx *ctx, real_hip_indel *out, uint64_t cap, uint64_t *n_out, int on_device)
{
    RH_ENTER(ctx);
    RhIndelStage &S = ctx->indel;
    return list_out(ctx, S.state == 2, kIndel, "calls", "call list", S.calls.p, S.n_calls, sizeof(real_hip_indel), out, cap, n_out, on_device);
}

extern "C" int real_hip_indel_end(real_hip_ctx *ctx)
{
    RH_ENTER(ctx);
    (void)hipStreamSynchronize(ctx->stream);
    rh_indel_release(ctx);
    return REAL_HIP_OK;
}

extern "C" int real_hip_indel_stats_get(real_hip_ctx *ctx, real_hip_indel_stats *out, int reset)
{
    return stats_get(ctx, out, reset, "indel stats struct_size", rh_indel_stats);
}

// ---- gapped placements in the pileup and the calls (pileup_gapped.hip): reads and gap records through stage_gapped, with the
// qualities.  Every check comes before the first launch
static int gapped_add(real_hip_ctx *ctx, const char *stage, int (*check)(real_hip_ctx *), const real_hip_batch *b1, const real_hip_batch *b2,
                      const real_hip_gap_place *gaps,
                      int (*add)(real_hip_ctx *, const DevBatch &, const DevBatch &, const real_hip_gap_place *, uint64_t))
{
    real_hip_batch bv[2];
    int rc;
    if ((rc = mates_view(ctx, stage, b1, b2, false, bv)) || (rc = check(ctx))) return rc;
    GappedReads p;
    if ((rc = stage_gapped(ctx, stage, bv, gaps, ctx->pileup_gapped.rec, true, p))) return rh_sync_tail(ctx, rc);
    if (!bv[0].n_reads) return REAL_HIP_OK;
    return rh_sync_tail(ctx, add(ctx, p.b[0], p.b[1], p.gaps, bv[0].n_reads));
}

extern "C" int real_hip_pileup_add_gapped(real_hip_ctx *ctx, const real_hip_batch *b1, const real_hip_batch *b2, const real_hip_gap_place *gaps)
{
    RH_ENTER(ctx);
    return gapped_add(ctx, "pileup", pileup_add_check, b1, b2, gaps, rh_pileup_gapped_add);
}

extern "C" int real_hip_call_add_gapped(real_hip_ctx *ctx, const real_hip_batch *b1, const real_hip_batch *b2, const real_hip_gap_place *gaps)
{
    RH_ENTER(ctx);
    return gapped_add(ctx, "calls", call_add_check, b1, b2, gaps, rh_call_gapped_add);
}

extern "C" int real_hip_pileup_depth_gapped(real_hip_ctx *ctx, uint64_t first, uint64_t count, uint32_t *depth, int on_device)
{
    RH_ENTER(ctx);
    if (ctx->pileup.state != 2) return rh_fail(ctx, REAL_HIP_E_INVALID, "pileup: depth before finish", hipSuccess);
    if (first > ctx->pileup.n || count > ctx->pileup.n - first) return rh_fail(ctx, REAL_HIP_E_INVALID, "pileup: the depth window reaches beyond the text", hipSuccess);
    if (!count) return REAL_HIP_OK;
    if (!depth) return rh_fail(ctx, REAL_HIP_E_INVALID, "pileup: null depth", hipSuccess);
    const uint32_t *g = rh_pileup_gapped_array(ctx);
    if (!g) { // (no gapped add was made: zeros)
        if (on_device) RH_HIP(ctx, hipMemsetAsync(depth, 0, (size_t)count * 4, ctx->stream));
        else memset(depth, 0, (size_t)count * 4);
    } else {
        RH_HIP(ctx, hipMemcpyAsync(depth, g + first, (size_t)count * 4, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    }
    return rh_sync_tail(ctx, REAL_HIP_OK);
}

extern "C" int real_hip_pileup_gapped_stats_get(real_hip_ctx *ctx, real_hip_pileup_gapped_stats *out, int reset)
{
    return stats_get(ctx, out, reset, "pileup gapped stats struct_size", rh_pileup_gapped_stats);
}

// ---- duplicates (duplicates.hip): the summary stages the offsets and the qualities alone (it reads no bases and needs no
// text); the marking stages records and summaries as real_hip_pair_insert_hist stages its arrays
extern "C" int real_hip_read_summary(real_hip_ctx *ctx, const real_hip_batch *b, uint32_t min_qual, real_hip_read_sum *out)
{
    RH_ENTER(ctx);
    real_hip_batch bv;
    int rc = batch_view(ctx, b, bv);
    if (rc) return rc;
    if (min_qual > 63) return rh_fail(ctx, REAL_HIP_E_INVALID, "read summary: min_qual beyond 63", hipSuccess);
    const uint64_t n = bv.n_reads;
    if (n > 0xffffffffull) return rh_fail(ctx, REAL_HIP_E_INVALID, "read summary: more than 2^32 reads in one batch", hipSuccess);
    if (!n) return REAL_HIP_OK;
    if (!out) return rh_fail(ctx, REAL_HIP_E_INVALID, "read summary: null out", hipSuccess);
    if (bv.on_device == 1 && ((uintptr_t)out & 7u)) return rh_fail(ctx, REAL_HIP_E_INVALID, "read summary: out must be 8-byte aligned", hipSuccess);
    DevBatch db;
    memset(&db, 0, sizeof db);
    db.n_reads = n; db.upatl = bv.patl;
    uint64_t total = n * (uint64_t)bv.patl, longest = bv.patl;
    const RhStaging in{ctx, !bv.on_device, ctx->stream, ctx->stream};
    if (bv.offsets) {
        if (!bv.on_device) {
            longest = 0;
            for (uint64_t i = 0; i < n; ++i) {
                if (bv.offsets[i + 1] < bv.offsets[i]) return rh_fail(ctx, REAL_HIP_E_INVALID, "offsets not monotone", hipSuccess);
                if (bv.offsets[i + 1] - bv.offsets[i] > longest) longest = bv.offsets[i + 1] - bv.offsets[i];
            }
            total = bv.offsets[n];
        }
        if ((rc = in.in(ctx->stage[0].off, bv.offsets, n + 1, db.off))) return rh_sync_tail(ctx, rc);
        if (bv.on_device) {
            uint32_t m = bv.max_patl;
            if (!m && (rc = rh_max_patl(ctx, db.off, n, &m))) return rh_sync_tail(ctx, rc);
            longest = m;
        }
    }
    if (longest > REAL_HIP_MAX_PATL_LONG) return rh_sync_tail(ctx, rh_fail(ctx, REAL_HIP_E_UNSUPPORTED, "read longer than REAL_HIP_MAX_PATL_LONG", hipSuccess));
    if (bv.qual && (rc = in.in(ctx->stage[0].qual, bv.qual, total, db.qual, total ? total : 1))) return rh_sync_tail(ctx, rc);
    const RhStaging io{ctx, bv.on_device != 1, ctx->stream, ctx->stream}; // (host: the output is host memory)
    real_hip_read_sum *d_out = out;
    rc = io.inout(ctx->dup.out, out, n, true, d_out);
    if (!rc) rc = rh_launch_read_summary(ctx, db, min_qual, d_out);
    if (!rc) rc = io.back(out, d_out, n, "download of the read summaries");
    return rh_sync_tail(ctx, rc);
}

// gaps (nullable): the reads' gap records beside their info words -- the joint marking (dup_gapped_stage.h)
static int mark_duplicates_run(real_hip_ctx *ctx, const uint64_t *info, const real_hip_pair *pairs, const real_hip_gap_place *gaps,
                               const real_hip_read_sum *sum1, const real_hip_read_sum *sum2, uint64_t n, int on_device, uint8_t *dup)
{
    if (n > (1ull << 32)) return rh_fail(ctx, REAL_HIP_E_INVALID, "duplicates: more than 2^32 records in one call", hipSuccess);
    if (!n) return REAL_HIP_OK;
    if ((!info && !pairs) || !sum1 || (pairs && !sum2) || !dup) return rh_fail(ctx, REAL_HIP_E_INVALID, "duplicates: null records / summaries / dup", hipSuccess);
    if (on_device && (((uintptr_t)info | (uintptr_t)pairs | (uintptr_t)sum1 | (uintptr_t)sum2) & 7u))
        return rh_fail(ctx, REAL_HIP_E_INVALID, "duplicates: records and summaries must be 8-byte aligned", hipSuccess);
    if (on_device && ((uintptr_t)gaps & 15u)) return rh_fail(ctx, REAL_HIP_E_INVALID, "duplicates: gap records must be 16-byte aligned", hipSuccess);
    const RhStaging io{ctx, !on_device, ctx->stream, ctx->stream};
    const uint64_t *d_info = info;
    const real_hip_pair *d_pairs = pairs;
    const real_hip_gap_place *d_gaps = gaps;
    const real_hip_read_sum *d_sum[2] = {sum1, sum2};
    uint8_t *d_dup = dup;
    int rc = info ? io.in(ctx->dup.rec, info, n, d_info) : io.in(ctx->dup.rec, pairs, n, d_pairs);
    if (!rc && gaps) rc = io.in(ctx->dup_gapped.rec, gaps, n, d_gaps);
    for (int m = 0; m < (pairs ? 2 : 1) && !rc; ++m) rc = io.in(ctx->dup.sum[m], m ? sum2 : sum1, n, d_sum[m]);
    if (!rc) rc = io.inout(ctx->dup.out, dup, n, true, d_dup);
    if (!rc) rc = gaps ? rh_launch_mark_duplicates_gapped(ctx, d_info, d_gaps, d_sum[0], n, d_dup)
                       : rh_launch_mark_duplicates(ctx, d_info, d_pairs, d_sum[0], d_sum[1], n, d_dup);
    if (!rc) rc = io.back(dup, d_dup, n, "download of the duplicate marks");
    return rh_sync_tail(ctx, rc);
}

extern "C" int real_hip_mark_duplicates(real_hip_ctx *ctx, const uint64_t *info, const real_hip_read_sum *sum, uint64_t n_reads, int on_device,
                                        uint8_t *dup)
{
    RH_ENTER(ctx);
    if (n_reads && !info) return rh_fail(ctx, REAL_HIP_E_INVALID, "duplicates: null info", hipSuccess);
    return mark_duplicates_run(ctx, info, nullptr, nullptr, sum, nullptr, n_reads, on_device, dup);
}

extern "C" int real_hip_mark_duplicates_gapped(real_hip_ctx *ctx, const uint64_t *info, const real_hip_gap_place *gaps,
                                               const real_hip_read_sum *sum, uint64_t n_reads, int on_device, uint8_t *dup)
{
    RH_ENTER(ctx);
    if (n_reads <= (1ull << 32) && n_reads && (!info || !gaps)) return rh_fail(ctx, REAL_HIP_E_INVALID, "duplicates: null info / gap records", hipSuccess);
    return mark_duplicates_run(ctx, info, nullptr, gaps, sum, nullptr, n_reads, on_device, dup);
}

extern "C" int real_hip_mark_duplicates_pairs(real_hip_ctx *ctx, const real_hip_pair *pairs, const real_hip_read_sum *sum1,
                                              const real_hip_read_sum *sum2, uint64_t n_pairs, int on_device, uint8_t *dup)
{
    RH_ENTER(ctx);
    if (n_pairs && !pairs) return rh_fail(ctx, REAL_HIP_E_INVALID, "duplicates: null pairs", hipSuccess);
    return mark_duplicates_run(ctx, nullptr, pairs, nullptr, sum1, sum2, n_pairs, on_device, dup);
}

extern "C" int real_hip_dup_stats_get(real_hip_ctx *ctx, real_hip_dup_stats *out, int reset)
{
    return stats_get(ctx, out, reset, "duplicate stats struct_size", rh_dup_stats);
}

// matchAll of both mates of n fragments with the hits kept on the device: afterwards pair_hits[m] / pair_off[m] / pair_len[m]
// hold mate m's unified hit lists, their n + 1 offsets and the read lengths; total[m] is an upper bound of the hits inside
// the buffer (the matcher's count before duplicates go).  both_resident: mate 2 is staged into buffers of its own, so that
// both mates' reads stay on the device (st[] are their views).
static int match_mates(real_hip_ctx *ctx, const real_hip_batch bv[2], bool both_resident, Staged st[2], uint64_t total[2])
{
    int rc;
    const uint64_t n = bv[0].n_reads;
    total[0] = total[1] = 0;
    for (int m = 0; m < 2; ++m) {
        if ((rc = rh_reserve(ctx, ctx->join.off[m], (n + 1) * 8))) return rc;
        if ((rc = rh_reserve(ctx, ctx->join.len[m], n * 4))) return rc;
    }
    // the hit capacity is the library's problem: both buffers hold pair_cap hits; a match that needs more reports the size,
    // the buffers grow and the matches are done again
    if (ctx->join.cap < n + n / 4 + 1024) ctx->join.cap = 0;
    for (int attempt = 0;; ++attempt) {
        if (!ctx->join.cap) {
            uint64_t want = n + n / 4 + 1024;
            if (total[0] > want) want = total[0];
            if (total[1] > want) want = total[1];
            for (int m = 0; m < 2; ++m)
                if ((rc = rh_reserve(ctx, ctx->join.hits[m], want * sizeof(real_hip_hit)))) return rc;
            ctx->join.cap = want;
        }
        bool overflow = false;
        for (int m = 0; m < 2; ++m) {
            Staged &s = st[m];
            s = Staged();
            rc = match_all_run(ctx, bv[m], true, (real_hip_hit *)ctx->join.hits[m].p, ctx->join.cap, &total[m], (uint64_t *)ctx->join.off[m].p, &s,
                               both_resident ? &ctx->stage[m] : nullptr);
            if (rc == REAL_HIP_E_OVERFLOW) { overflow = true; continue; } // (the other mate still reports its size)
            if (rc) return rc;
            // the read lengths, while this mate's offsets are staged
            if ((rc = rh_pair_lens(ctx, s.off, s.upatl, n, (uint32_t *)ctx->join.len[m].p))) return rc;
        }
        if (!overflow) break;
        if (attempt >= 2) return rh_fail(ctx, REAL_HIP_E_OVERFLOW, "hit buffers of the pair join kept overflowing", hipSuccess);
        if (total[0] > 0xffffffffull || total[1] > 0xffffffffull) return rh_fail(ctx, REAL_HIP_E_OVERFLOW, "more than 2^32 hits of one mate in one batch", hipSuccess);
        ctx->join.cap = 0;
    }
    return REAL_HIP_OK;
}

// real_hip_match_pairs, and with sp (real_hip_match_pairs_search) the mate search behind the join; with singles
// (real_hip_match_pairs_singles: both arrays or none) each mate's hit list is folded into its records while it is resident
static int match_pairs_run(real_hip_ctx *ctx, const real_hip_batch *batch1, const real_hip_batch *batch2, const real_hip_pair_params *pp,
                           const real_hip_mate_search_params *sp, real_hip_pair *pairs, real_hip_single *const singles[2] = nullptr,
                           real_hip_mapq_acc *const accs[3] = nullptr)
{
    int rc;
    real_hip_batch bv[2];
    if ((rc = mates_view(ctx, "", batch1, batch2, true, bv))) return rc;
    if (sp && (rc = search_batches_check(ctx, bv))) return rc;
    const uint64_t n = bv[0].n_reads;
    if (!n) return REAL_HIP_OK;
    if (!pairs) return rh_fail(ctx, REAL_HIP_E_INVALID, "null pairs", hipSuccess);
    Staged st[2];
    uint64_t total[2] = {0, 0};
    if ((rc = match_mates(ctx, bv, sp != nullptr, st, total))) return rc;
    const MateLists L = resident_lists(ctx, total);
    const bool host_out = bv[0].on_device != 1;
    const int fresh = bv[0].fresh != 0;
    real_hip_pair *d_pairs = pairs;
    const RhStaging io{ctx, host_out, ctx->stream, ctx->stream};
    if ((rc = io.inout(ctx->join.rec, pairs, n, fresh != 0, d_pairs))) return rc;
    rc = rh_launch_pair(ctx, *pp, L, n, ctx->fileid, fresh, d_pairs);
    real_hip_single *d_singles[2] = {nullptr, nullptr};
    if (!rc && singles) { // seed hits only: the search below adds nothing to the lists
        rc = stage_singles(io, 2, singles, n, fresh, d_singles);
        if (!rc) rc = rh_launch_single(ctx, 2, L, n, ctx->fileid, fresh, d_singles);
    }
    real_hip_mapq_acc *d_accs[3] = {nullptr, nullptr, nullptr};
    if (!rc && accs) { // the pair's, then the two mates': seed hits only, as the singles
        rc = stage_mapq_accs(io, 3, accs, n, fresh, d_accs);
        if (!rc) rc = rh_launch_mapq_pair_fold(ctx, *pp, L, n, fresh, d_accs[0]);
        if (!rc) rc = rh_launch_mapq_fold(ctx, 2, L, n, fresh, d_accs + 1);
    }
    if (!rc && sp) // the records of the join are the search's in/out records
        rc = rh_launch_mate_search(ctx, *pp, *sp, dev_batch(ctx, st[0], n), dev_batch(ctx, st[1], n), L, n, ctx->fileid, 0, d_pairs);
    if (!rc) rc = io.back(pairs, d_pairs, n, "download of the pair records");
    if (!rc && singles) rc = download_singles(io, 2, singles, n, d_singles);
    for (int m = 0; m < 3 && !rc && accs; ++m) rc = io.back(accs[m], d_accs[m], n, "download of the mapping quality accumulators");
    rc = rh_sync_tail(ctx, rc);
    return rc || !sp ? rc : rh_mate_search_finish(ctx);
}

extern "C" int real_hip_match_pairs(real_hip_ctx *ctx, const real_hip_batch *batch1, const real_hip_batch *batch2,
                                    const real_hip_pair_params *pp, real_hip_pair *pairs)
{
    RH_ENTER(ctx);
    int rc = pair_params_check(ctx, pp);
    if (rc) return rc;
    return match_pairs_run(ctx, batch1, batch2, pp, nullptr, pairs);
}

extern "C" int real_hip_match_pairs_search(real_hip_ctx *ctx, const real_hip_batch *batch1, const real_hip_batch *batch2,
                                           const real_hip_pair_params *pp, const real_hip_mate_search_params *sp, real_hip_pair *pairs)
{
    RH_ENTER(ctx);
    int rc = pair_params_check(ctx, pp);
    if (rc || (rc = search_params_check(ctx, pp, sp))) return rc;
    return match_pairs_run(ctx, batch1, batch2, pp, sp, pairs);
}

extern "C" int real_hip_match_pairs_singles(real_hip_ctx *ctx, const real_hip_batch *batch1, const real_hip_batch *batch2,
                                            const real_hip_pair_params *pp, const real_hip_mate_search_params *sp, real_hip_pair *pairs,
                                            real_hip_single *singles1, real_hip_single *singles2)
{
    RH_ENTER(ctx);
    int rc = pair_params_check(ctx, pp);
    if (rc || (sp && (rc = search_params_check(ctx, pp, sp)))) return rc;
    if (!singles1 || !singles2) return rh_fail(ctx, REAL_HIP_E_INVALID, "null singles", hipSuccess);
    real_hip_single *const singles[2] = {singles1, singles2};
    return match_pairs_run(ctx, batch1, batch2, pp, sp, pairs, singles);
}

extern "C" int real_hip_match_pairs_mapq(real_hip_ctx *ctx, const real_hip_batch *batch1, const real_hip_batch *batch2,
                                         const real_hip_pair_params *pp, const real_hip_mate_search_params *sp, real_hip_pair *pairs,
                                         real_hip_single *singles1, real_hip_single *singles2, real_hip_mapq_acc *acc_pair,
                                         real_hip_mapq_acc *acc1, real_hip_mapq_acc *acc2)
{
    RH_ENTER(ctx);
    int rc = pair_params_check(ctx, pp);
    if (rc || (sp && (rc = search_params_check(ctx, pp, sp)))) return rc;
    if (!singles1 || !singles2) return rh_fail(ctx, REAL_HIP_E_INVALID, "null singles", hipSuccess);
    if (!acc_pair || !acc1 || !acc2) return rh_fail(ctx, REAL_HIP_E_INVALID, "null mapping quality accumulators", hipSuccess);
    real_hip_single *const singles[2] = {singles1, singles2};
    real_hip_mapq_acc *const accs[3] = {acc_pair, acc1, acc2};
    return match_pairs_run(ctx, batch1, batch2, pp, sp, pairs, singles, accs);
}

// matchAll of one batch with the hits kept on the device, in mate 1's buffers: pair_hits[0] / pair_off[0] hold the unified hit
// lists and their n + 1 offsets, *total the hits.  The buffer only ever grows (pair_cap, the size BOTH mates' buffers have at
// least, stays true); a match that needs more reports the size and is done again.
static int match_resident(real_hip_ctx *ctx, const real_hip_batch &bv, uint64_t *total)
{
    int rc;
    const uint64_t n = bv.n_reads;
    if ((rc = rh_reserve(ctx, ctx->join.off[0], (n + 1) * 8))) return rc;
    uint64_t want = n + n / 4 + 1024;
    for (int attempt = 0;; ++attempt) {
        if ((rc = rh_reserve(ctx, ctx->join.hits[0], want * sizeof(real_hip_hit)))) return rc;
        const uint64_t cap = ctx->join.hits[0].cap / sizeof(real_hip_hit);
        Staged s;
        rc = match_all_run(ctx, bv, true, (real_hip_hit *)ctx->join.hits[0].p, cap, total, (uint64_t *)ctx->join.off[0].p, &s);
        if (rc != REAL_HIP_E_OVERFLOW) return rc;
        if (attempt >= 2) return rh_fail(ctx, REAL_HIP_E_OVERFLOW, "hit buffer of the mapping quality fold kept overflowing", hipSuccess);
        if (*total > 0xffffffffull) return rh_fail(ctx, REAL_HIP_E_OVERFLOW, "more than 2^32 hits in one batch", hipSuccess);
        want = *total;
    }
}

extern "C" int real_hip_match_mapq(real_hip_ctx *ctx, const real_hip_batch *batch, real_hip_mapq_acc *acc)
{
    RH_ENTER(ctx);
    real_hip_batch bv;
    int rc = batch_view(ctx, batch, bv);
    if (rc) return rc;
    if (!ctx->have_text || !ctx->have_index) return rh_fail(ctx, REAL_HIP_E_STATE, "text and index must be set", hipSuccess);
    const uint64_t n = bv.n_reads;
    if (!n) return REAL_HIP_OK;
    if (n > 0xffffffffull) return rh_fail(ctx, REAL_HIP_E_INVALID, "more than 2^32 reads in one call", hipSuccess);
    if (!acc) return rh_fail(ctx, REAL_HIP_E_INVALID, "null mapping quality accumulators", hipSuccess);
    uint64_t total = 0;
    if ((rc = match_resident(ctx, bv, &total))) return rc;
    MateLists L;
    memset(&L, 0, sizeof L);
    L.h[0] = (const uint4 *)ctx->join.hits[0].p; L.o[0] = (const uint64_t *)ctx->join.off[0].p; L.total[0] = total;
    const int fresh = bv.fresh != 0;
    real_hip_mapq_acc *const av[1] = {acc};
    real_hip_mapq_acc *d_acc[2] = {nullptr, nullptr};
    const RhStaging io{ctx, bv.on_device != 1, ctx->stream, ctx->stream};
    rc = stage_mapq_accs(io, 1, av, n, fresh, d_acc);
    if (!rc) rc = rh_launch_mapq_fold(ctx, 1, L, n, fresh, d_acc);
    if (!rc) rc = io.back(acc, d_acc[0], n, "download of the mapping quality accumulators");
    return rh_sync_tail(ctx, rc);
}

extern "C" int real_hip_mate_search_stats_get(real_hip_ctx *ctx, real_hip_mate_search_stats *out, int reset)
{
    return stats_get(ctx, out, reset, "mate search stats struct_size", rh_mate_search_stats);
}

extern "C" int real_hip_pair_stats_get(real_hip_ctx *ctx, real_hip_pair_stats *out, int reset)
{
    return stats_get(ctx, out, reset, "pair stats struct_size", rh_pair_stats);
}

// ---- every concordant pair of a fragment (pair_all.hip) -----------------------------------------------------------
// count, then -- the total being known -- the overflow decision, then the records; dev_out: out / pair_offsets are device memory
static int pair_all_run(real_hip_ctx *ctx, const real_hip_pair_params &pp, const MateLists &L, uint64_t n, uint32_t fileid, bool dev_out,
                        real_hip_pair_hit *out, uint64_t cap, uint64_t *n_out, uint64_t *pair_offsets)
{
    int rc;
    // (outputs: nothing is uploaded; without pair_offsets the scan still needs a device array)
    const RhStaging io{ctx, !dev_out, ctx->stream, ctx->stream}, off_io{ctx, !dev_out || !pair_offsets, ctx->stream, ctx->stream};
    uint64_t *d_off = pair_offsets;
    if ((rc = off_io.inout(ctx->pair_all.off, pair_offsets, n + 1, true, d_off))) return rc;
    uint64_t found = 0;
    rc = rh_pair_all_count(ctx, pp, L, n, d_off, &found);
    rh_time_resolve(ctx);
    if (rc) return rc;
    *n_out = found;
    if (found > cap) return rh_fail(ctx, REAL_HIP_E_OVERFLOW, "pair hit buffer too small", hipSuccess);
    real_hip_pair_hit *d_out = out;
    if ((rc = io.inout(ctx->pair_all.out, out, found, true, d_out, sizeof(real_hip_pair_hit)))) return rc;
    rc = rh_pair_all_emit(ctx, pp, L, n, fileid, d_off, d_out, dev_out ? cap : found, found);
    if (!rc) rc = io.back(out, d_out, found, "download of the pair hits");
    if (!rc && pair_offsets) rc = io.back(pair_offsets, d_off, n + 1, "download of the pair hits");
    return rh_sync_tail(ctx, rc);
}
// what both entry points check of their outputs; n == 0 is answered here (*done)
static int pair_all_outputs_check(real_hip_ctx *ctx, uint64_t n, bool dev_out, real_hip_pair_hit *out, uint64_t cap, uint64_t *n_out,
                                  uint64_t *pair_offsets, bool *done)
{
    *done = false;
    if (!n_out) return rh_fail(ctx, REAL_HIP_E_INVALID, "null n_out", hipSuccess);
    *n_out = 0;
    if (n > 0xffffffffull) return rh_fail(ctx, REAL_HIP_E_INVALID, "more than 2^32 pairs in one call", hipSuccess);
    if (cap && !out) return rh_fail(ctx, REAL_HIP_E_INVALID, "null pair hit buffer", hipSuccess);
    if (dev_out && ((uintptr_t)out & 15u)) return rh_fail(ctx, REAL_HIP_E_INVALID, "the pair hit buffer must be 16-byte aligned", hipSuccess);
    if (n) return REAL_HIP_OK;
    *done = true;
    if (pair_offsets) {
        if (!dev_out) pair_offsets[0] = 0;
        else {
            RH_HIP(ctx, hipMemsetAsync(pair_offsets, 0, 8, ctx->stream));
            RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
    }
    return REAL_HIP_OK;
}

extern "C" int real_hip_pair_all_hits(real_hip_ctx *ctx, const real_hip_pair_params *pp, const real_hip_hit *hits1, const uint64_t *off1,
                                      const uint32_t *len1, const real_hip_hit *hits2, const uint64_t *off2, const uint32_t *len2,
                                      uint64_t n_pairs, uint32_t fileid, int on_device, real_hip_pair_hit *out, uint64_t cap, uint64_t *n_out,
                                      uint64_t *pair_offsets)
{
    RH_ENTER(ctx);
    int rc = pair_params_check(ctx, pp);
    if (rc) return rc;
    if (fileid > 255) return rh_fail(ctx, REAL_HIP_E_INVALID, "fileid > 255", hipSuccess);
    const uint64_t n = n_pairs;
    bool done;
    if ((rc = pair_all_outputs_check(ctx, n, on_device != 0, out, cap, n_out, pair_offsets, &done)) || done) return rc;
    if (!off1 || !off2 || !len1 || !len2) return rh_fail(ctx, REAL_HIP_E_INVALID, "null offsets / lengths", hipSuccess);
    const real_hip_hit *const hits[2] = {hits1, hits2};
    const uint64_t *const off[2] = {off1, off2};
    const uint32_t *const len[2] = {len1, len2};
    MateLists L;
    if ((rc = stage_hit_lists(ctx, hits, off, len, n, on_device != 0, L))) return rc;
    return pair_all_run(ctx, *pp, L, n, fileid, on_device != 0, out, cap, n_out, pair_offsets);
}

extern "C" int real_hip_match_pairs_all(real_hip_ctx *ctx, const real_hip_batch *batch1, const real_hip_batch *batch2,
                                        const real_hip_pair_params *pp, real_hip_pair_hit *out, uint64_t cap, uint64_t *n_out, uint64_t *pair_offsets)
{
    RH_ENTER(ctx);
    int rc = pair_params_check(ctx, pp);
    if (rc) return rc;
    real_hip_batch bv[2];
    if ((rc = mates_view(ctx, "", batch1, batch2, true, bv))) return rc;
    const uint64_t n = bv[0].n_reads;
    const bool dev_out = bv[0].on_device == 1;
    bool done;
    if ((rc = pair_all_outputs_check(ctx, n, dev_out, out, cap, n_out, pair_offsets, &done)) || done) return rc;
    Staged st[2];
    uint64_t total[2] = {0, 0};
    if ((rc = match_mates(ctx, bv, false, st, total))) return rc;
    return pair_all_run(ctx, *pp, resident_lists(ctx, total), n, ctx->fileid, dev_out, out, cap, n_out, pair_offsets);
}

extern "C" int real_hip_pair_all_stats_get(real_hip_ctx *ctx, real_hip_pair_all_stats *out, int reset)
{
    return stats_get(ctx, out, reset, "pair all stats struct_size", rh_pair_all_stats);
}

// ---------------------------------------------------------------------------
// read ingestion
// ---------------------------------------------------------------------------
extern "C" int real_hip_parse_reads(real_hip_ctx *ctx, const char *text, uint64_t n_bytes, int text_on_device, int fastq,
                                    int quality_offset, real_hip_parsed *out)
{
    RH_ENTER(ctx);
    if (!out || (n_bytes && !text)) return rh_fail(ctx, REAL_HIP_E_INVALID, "null text / out", hipSuccess);
    const char *d_text = text;
    const RhStaging io{ctx, !text_on_device, ctx->stream, ctx->stream};
    int rc;
    if (n_bytes && (rc = io.in(ctx->p_text, text, n_bytes, d_text))) return rc;
    RhTimer tm(ctx, REAL_HIP_K_PARSE);
    return rh_parse_reads(ctx, d_text, n_bytes, fastq, quality_offset, out);
}

extern "C" int real_hip_download(real_hip_ctx *ctx, const void *device_ptr, void *host_ptr, size_t bytes)
{
    RH_ENTER(ctx);
    if (bytes && (!device_ptr || !host_ptr)) return rh_fail(ctx, REAL_HIP_E_INVALID, "null pointer", hipSuccess);
    if (bytes) RH_HIP(ctx, hipMemcpyAsync(host_ptr, device_ptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
    RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return REAL_HIP_OK;
}

// ---------------------------------------------------------------------------
// counters / timing
// ---------------------------------------------------------------------------
int rh_stats_reserve(real_hip_ctx *ctx, DevBuf &buf, size_t stripes, size_t extra_bytes)
{
    if (buf.p) return REAL_HIP_OK;
    const size_t bytes = stripes * 16 * 8 + extra_bytes;
    int rc = rh_reserve(ctx, buf, bytes);
    if (rc) return rc;
    RH_HIP(ctx, hipMemsetAsync(buf.p, 0, bytes, ctx->stream));
    return REAL_HIP_OK;
}

int rh_stats_read(real_hip_ctx *ctx, const DevBuf &buf, size_t stripes, int n_words, int reset, uint64_t out[])
{
    for (int k = 0; k < n_words; ++k) out[k] = 0;
    if (!buf.p) return REAL_HIP_OK;
    std::vector<uint64_t> all(stripes * 16);
    RH_HIP(ctx, hipMemcpyAsync(all.data(), buf.p, all.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (reset) RH_HIP(ctx, hipMemsetAsync(buf.p, 0, all.size() * 8, ctx->stream));
    RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t st = 0; st < stripes; ++st)
        for (int k = 0; k < n_words; ++k) out[k] += all[st * 16 + k];
    return REAL_HIP_OK;
}

int rh_stage_read(real_hip_ctx *ctx, RhStage &stage, size_t stripes, int n_words, int reset, uint64_t h[], RhStageCount &was)
{
    int rc = rh_stats_read(ctx, stage.stats, stripes, n_words, reset, h);
    if (rc) return rc;
    rh_time_resolve(ctx);
    was = stage;
    if (reset) static_cast<RhStageCount &>(stage) = RhStageCount();
    return REAL_HIP_OK;
}

extern "C" int real_hip_counters_get(real_hip_ctx *ctx, real_hip_counters *out, int reset)
{
    RH_ENTER(ctx);
    uint64_t h[8];
    int rc;
    if ((rc = rh_stats_read(ctx, ctx->counters, RH_CSTRIPES, 8, reset, h))) return rc; // (not the scratch stripe behind them)
    if (out) {
        out->reads = h[0]; out->lookups = h[1]; out->probes = h[2]; out->candidates = h[3];
        out->seedpass = h[4]; out->hits = h[5]; out->verified = h[6]; out->handed_over = h[7];
    }
    return REAL_HIP_OK;
}

extern "C" int real_hip_kernel_time(real_hip_ctx *ctx, int which, double *total_ms, uint64_t *launches, int reset)
{
    if (!ctx || which < 0 || which >= REAL_HIP_K_COUNT) return REAL_HIP_E_INVALID;
    if (total_ms) *total_ms = ctx->k_ms[which];
    if (launches) *launches = ctx->k_n[which];
    if (reset) { ctx->k_ms[which] = 0; ctx->k_n[which] = 0; }
    return REAL_HIP_OK;
}

extern "C" int real_hip_timing_enable(real_hip_ctx *ctx, int on)
{
    if (!ctx) return REAL_HIP_E_INVALID;
    ctx->timing = on != 0;
    return REAL_HIP_OK;
}
