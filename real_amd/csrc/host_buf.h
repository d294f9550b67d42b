// host_buf.h -- the host layer's building blocks, below the context: owned device buffers, the staging rule for an array that
// crosses the ABI, a stage's counts and striped statistics, error plumbing.  The stage headers (<stage>_stage.h) build their
// records from these; real_hip_ctx.h puts the records together.  Kernels do not read this file: what they read is
// real_hip_internal.h.
#pragma once
#include "real_hip_internal.h"

struct DevBuf;
struct real_hip_ctx;
void rh_release(DevBuf &b);
// a device allocation and its owner: it goes with whatever holds it (the ctx, a slot, a function's scope)
struct DevBuf {
    void  *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { rh_release(*this); }
};

// device copies of a host batch's four arrays: the ctx's own two sets (synchronous calls; the second holds mate 2 while
// both mates are resident) or those of a slot (submit / wait)
struct BatchBufs {
    DevBuf bases, qual, off, nflags;
};

// one slot of the submit / wait pipeline: device copies of a host batch and its records
struct RhSlot {
    BatchBufs in;
    DevBuf info, score;
    hipEvent_t up = nullptr, matched = nullptr, done = nullptr;
    uint64_t n = 0;
    int status = 0;
    bool busy = false, empty = false;
};

// what the ctx keeps of one paired stage: the items it was given, its launches and their event times since the last reset,
// and the striped statistics its kernels add to (rh_stats_reserve)
struct RhStageCount {
    uint64_t items = 0, launches = 0;
    double   kernel_ms = 0;
};
struct RhStage : RhStageCount {
    DevBuf stats;
};

// error plumbing: never throw across the ABI
int rh_fail(real_hip_ctx *ctx, int status, const char *what, hipError_t e);
#define RH_HIP(ctx, call)                                                          \
    do {                                                                           \
        hipError_t _e = (call);                                                    \
        if (_e != hipSuccess) return rh_fail((ctx), REAL_HIP_E_DEVICE, #call, _e); \
    } while (0)
int rh_reserve(real_hip_ctx *ctx, DevBuf &b, size_t bytes);
void rh_release(real_hip_ctx *ctx, DevBuf &b); // (timed: real_hip_index_build_stats)
double rh_now_ms();
// a function-local device buffer whose release is charged to the ctx's build statistics
struct ScopedBuf : DevBuf {
    real_hip_ctx *c;
    explicit ScopedBuf(real_hip_ctx *ctx) : c(ctx) {}
    ~ScopedBuf() { rh_release(c, *this); }
};

// The one rule for an array that crosses the ABI.  host: the caller's arrays are host memory, each is copied into a DevBuf
// of the ctx on `up` and the kernels read the copy; otherwise the caller's pointer is the device view.
//   in     the device view of `count` elements (room: bytes to reserve where that is more than the elements take)
//   inout  the same, the upload skipped when `fresh` (the kernel starts every record itself)
//   back   the download on `down`; its error is returned, so that the caller's rh_sync_tail still runs
struct RhStaging {
    real_hip_ctx *ctx;
    bool host;
    hipStream_t up, down;
    int view(DevBuf &buf, const void *src, size_t bytes, size_t room, bool upload, void **dev) const;
    int back_bytes(void *dst, const void *dev, size_t bytes, const char *what) const;
    template <typename T> int in(DevBuf &buf, const T *src, size_t count, const T *&dev, size_t room = 0) const
    {
        void *d = nullptr;
        const int rc = view(buf, src, count * sizeof(T), room, true, &d);
        dev = static_cast<const T *>(d);
        return rc;
    }
    template <typename T> int inout(DevBuf &buf, T *src, size_t count, bool fresh, T *&dev, size_t room = 0) const
    {
        void *d = nullptr;
        const int rc = view(buf, src, count * sizeof(T), room, !fresh, &d);
        dev = static_cast<T *>(d);
        return rc;
    }
    template <typename T> int back(T *dst, const T *dev, size_t count, const char *what) const
    {
        return back_bytes(dst, dev, count * sizeof(T), what);
    }
};

// ---- what the paired-end stages share ---------------------------------------------
struct MateLists; // the two mates' hit lists on the device (pair_state.h)
// a fixed grid of waves (four per block) takes `work` items in turn: the number of handed-over fragments stays on the
// device, and what a block loads once (the mate search's score table) is loaded at most this often
static inline unsigned rh_wave_blocks(uint64_t work) { return (unsigned)((work + 3) / 4 < 2048 ? (work + 3) / 4 : 2048); }
// striped statistics: `stripes` 128-byte lines of 16 words, summed on the host (see RH_CSTRIPES), with extra_bytes behind
// them.  rh_stats_reserve allocates and zeroes the buffer on first use; rh_stats_read sums words 0 .. n_words - 1 over the
// stripes into out[] (zeros while there is no buffer), clears the stripes if `reset`, and synchronises the stream
int rh_stats_reserve(real_hip_ctx *ctx, DevBuf &buf, size_t stripes, size_t extra_bytes);
int rh_stats_read(real_hip_ctx *ctx, const DevBuf &buf, size_t stripes, int n_words, int reset, uint64_t out[]);
// what the stages' stats functions share: the striped words into h[], the pending event times resolved, `was` = the counts
// as they stand, which then start again if `reset`
int rh_stage_read(real_hip_ctx *ctx, RhStage &stage, size_t stripes, int n_words, int reset, uint64_t h[], RhStageCount &was);
