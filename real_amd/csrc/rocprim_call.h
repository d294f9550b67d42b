// rocprim_call.h -- one way to make a rocPRIM device call.  rocPRIM wants every call twice: with a null temporary it only
// reports the bytes it needs, with a temporary of that size it runs.  Here the call is written ONCE, as a callable
//     [&](void *tmp, size_t &bytes) { return rocprim::exclusive_scan(tmp, bytes, in, out, ...); }
// and asked for its size (rh_prim_size) or run (rh_prim_run) through it.
#pragma once
#include "real_hip_ctx.h"

// the temporary bytes `call` needs, folded into a running maximum (one temporary serves several calls)
template <typename F> static inline int rh_prim_size(real_hip_ctx *ctx, F &&call, size_t &max_bytes, const char *what)
{
    size_t bytes = 0;
    const hipError_t e = call(nullptr, bytes);
    if (e != hipSuccess) return rh_fail(ctx, REAL_HIP_E_DEVICE, what, e);
    if (bytes > max_bytes) max_bytes = bytes;
    return REAL_HIP_OK;
}
// runs `call` on a temporary of `bytes` the caller holds (a region of an arena planned with rh_prim_size)
template <typename F> static inline int rh_prim_run(real_hip_ctx *ctx, void *tmp, size_t bytes, F &&call, const char *what)
{
    const hipError_t e = call(tmp, bytes);
    return e == hipSuccess ? REAL_HIP_OK : rh_fail(ctx, REAL_HIP_E_DEVICE, what, e);
}
// runs `call` on `tmp`, grown to what the call asks for
template <typename F> static inline int rh_prim_run(real_hip_ctx *ctx, DevBuf &tmp, F &&call, const char *what)
{
    size_t bytes = 0;
    int rc = rh_prim_size(ctx, call, bytes, what);
    if (!rc) rc = rh_reserve(ctx, tmp, bytes ? bytes : 8);
    return rc ? rc : rh_prim_run(ctx, tmp.p, bytes, call, what);
}
