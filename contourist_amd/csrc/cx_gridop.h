// cx_gridop.h -- the host-side frame of the whole-volume operations (cx_filter, cx_dist, cx_label, cx_resample, cx_rank, cx_recon, cx_watershed, cx_regions):
// where an operation's samples come from, and the slot that keeps its result in the context until it is bound.
#pragma once
#include <new>
#include <string>
#include <utility>

#include "cx_ctx.h"

// two byte ranges share a byte (a range without memory shares none)
static inline bool cx_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a0 < b0 + nb && b0 < a0 + na;
}

// an operation's state, made at its first call (null: no memory)
template <typename S>
static inline S* cx_state_of(S*& state) {
    if (!state) state = new (std::nothrow) S();
    return state;
}

// `samples == NULL` and no grid bound for it to mean (`mask`: in cx_grid_reconstruct3d's words)
static inline int cx_no_grid(cx_ctx* ctx, const char* who, bool mask = false) {
    return cx_fail(ctx, CX_ERR_STATE, (std::string(who) + (mask ? ": no mask given and no grid bound" : ": no samples given and no grid bound")).c_str());
}

// The samples an operation reads: the caller's (device memory, or host memory where !on_device) or, for samples == NULL, the bound grid.
struct cx_source {
    const void* p;
    int32_t dtype;
    int on_device;
    int64_t n[3];
    size_t count, bytes;
};
// At most 2^limit_log2 samples.  `who` names the entry point in the refusals.  `mask`: cx_grid_reconstruct3d, whose header words and
// grades them differently (an empty axis is CX_ERR_INVALID, too many samples CX_ERR_UNSUPPORTED).
static inline int cx_source_resolve(cx_ctx* ctx, const char* who, const void* samples, int32_t dtype, int on_device, int64_t n0, int64_t n1, int64_t n2,
                                    int limit_log2, cx_source* S, bool mask = false) {
    auto refuse = [&](int code, const std::string& what) { return cx_fail(ctx, code, (std::string(who) + ": " + what).c_str()); };
    if (!samples) {
        if (!ctx->grid.p) return cx_no_grid(ctx, who, mask);
        samples = ctx->grid.p; dtype = ctx->grid.dtype; n0 = ctx->n0; n1 = ctx->n1; n2 = ctx->n2; on_device = 1;
    } else {
        if (!cx_dtype_valid(dtype)) return refuse(CX_ERR_INVALID, "unknown sample type");
        const int64_t lim = 1LL << limit_log2;
        const bool empty = n0 < 1 || n1 < 1 || n2 < 1;
        const bool many = !empty && (n0 > lim || n1 > lim || n2 > lim || n0 * n1 > lim || n0 * n1 * n2 > lim);
        if (mask && empty) return refuse(CX_ERR_INVALID, "at least 1 sample per axis");
        if (mask && many) return refuse(CX_ERR_UNSUPPORTED, "at most 2^" + std::to_string(limit_log2) + " samples");
        if (empty || many) return refuse(CX_ERR_INVALID, "at least 1 sample per axis, at most 2^" + std::to_string(limit_log2) + " in all");
    }
    S->p = samples; S->dtype = dtype; S->on_device = on_device;
    S->n[0] = n0; S->n[1] = n1; S->n[2] = n2;
    S->count = (size_t)(n0 * n1 * n2); S->bytes = S->count * cx_dtype_size(dtype);
    return CX_OK;
}

// host samples into `buf` on the context's stream; *dev: where they are
static inline int cx_upload(cx_ctx* ctx, cx_buf<uint8_t>& buf, const void* host, size_t bytes, const void** dev) {
    const int rc = buf.grow(ctx, bytes);
    if (rc) return rc;
    CX_HIP(ctx, hipMemcpyAsync(buf, host, bytes, hipMemcpyHostToDevice, ctx->stream));
    *dev = buf.get();
    return CX_OK;
}

// What an operation keeps in the context between calls: the device copy of host samples and its own result, pending from the call that
// wrote it until the next call or the bind.  One per operation.
struct cx_slot {
    cx_buf<uint8_t> in;        // host samples; the result of the call before where that is this call's input
    cx_buf<uint8_t> result;    // the context's own result, as bytes: the bind moves it into ctx->grid_owned
    int64_t shape[3] = {0, 0, 0};
    bool pending = false;      // `result` holds the result of the last call and has not been bound

    // The one step-aside rule: device memory [p, p + bytes) that overlaps `result` is (part of) the result of the call before.  That
    // result is consumed: its buffer changes places with `aside`, so that this call's own result cannot land on it.  The memory does
    // not move, so the caller's pointer stays good for this call.
    void step_aside(const void* p, size_t bytes, cx_buf<uint8_t>& aside) {
        if (!cx_overlap(p, bytes, result.get(), result.bytes())) return;
        std::swap(result, aside);
        pending = false;
    }
    // the input where the kernels read it: host samples go up into `in`, device samples stay where they are (and `result` steps aside)
    int stage(cx_ctx* ctx, const cx_source& S, const void** dev) {
        *dev = S.p;
        if (!S.on_device) return cx_upload(ctx, in, S.p, S.bytes, dev);
        step_aside(S.p, S.bytes, in);
        return CX_OK;
    }
    // where this call writes: the caller's `out_device`, or `result` with room for out_bytes.  Whatever was pending is gone: a
    // caller's output leaves nothing to hand out or bind
    int open(cx_ctx* ctx, void* out_device, size_t out_bytes, void** out) {
        pending = false;
        *out = out_device;
        if (out_device) return CX_OK;
        const int rc = result.grow(ctx, out_bytes);
        *out = result.get();
        return rc;
    }
    void publish(int64_t m0, int64_t m1, int64_t m2) {
        shape[0] = m0; shape[1] = m1; shape[2] = m2;
        pending = true;
    }
};

// the common part of an operation's _result and _bind; `s` is null before the operation's first call, `none` the refusal without a
// pending result
static inline int cx_slot_result(cx_ctx* ctx, const cx_slot* s, const char* none, void** out_device, int64_t out_shape[3]) {
    if (!s || !s->pending) return cx_fail(ctx, CX_ERR_STATE, none);
    if (out_device) *out_device = s->result.get();
    if (out_shape) { out_shape[0] = s->shape[0]; out_shape[1] = s->shape[1]; out_shape[2] = s->shape[2]; }
    return CX_OK;
}
static inline int cx_slot_bind(cx_ctx* ctx, cx_slot* s, const char* none, int32_t dtype) {
    if (!s || !s->pending) return cx_fail(ctx, CX_ERR_STATE, none);
    CX_HIP(ctx, hipSetDevice(ctx->device));
    CX_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the operation may still be reading the grid that goes
    const int rc = cx_grid_bind_owned(ctx, s->result, dtype, s->shape[0], s->shape[1], s->shape[2]);
    if (rc == CX_OK) s->pending = false;
    return rc;
}
