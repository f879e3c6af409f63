// cx_resample.hip -- a volume on another lattice (include/contourist_hip.h, section "resampling through an affine map"): the samples of a
// 3-D array of any CX_DTYPE_* read through c = offset + M i, nearest (the input's own type out) or trilinear (fp32 out), with the
// filter's boundary rules (cx_grid_resample3d), and the result as the bound grid (cx_grid_resample3d_bind).
//
// The arithmetic is fixed by the header and every double operation is rounded on its own: the file is compiled without contraction
// (the pragma below), and the coordinate and the blend are written with the plain operators it governs.  The runtime header's
// __dmul_rn / __dadd_rn are parsed before this file begins, under the compiler's default, and fuse once they are inlined.
//
// Everything an input axis contributes to one output is a cxr_ent: the two indices read (boundary rule applied, -1 = cval), the
// fraction, and whether the coordinate lies off the array.  Two ways to get the three of them:
//   general      every lane computes its coordinates and entries (about 30 double operations).  A workgroup owns a compact brick of
//                the output, 256 samples, longest along the output axis that runs most nearly along input axis 2: under a rotation
//                the eight corners of a wave then stay inside few cache lines, and the loads are as coalesced as the map allows.
//   table        a matrix with at most one entry per row (zoom, crop, regrid, flip, transpose): each coordinate depends on one output
//                index, so cxr_k_table writes the entries of every output index once and the lanes load theirs (16 + 8 bytes, shared
//                by the whole wave on two of the axes).  Lanes run along output axis 2: 2 x 2 x 64 bricks.
// The entries are the same either way (a term M[a][k] i_k with M[a][k] == +-0.0 changes at most the sign of a zero coordinate, which
// no later step sees), so both give the bits of the header's formula; tests/resample_ref.py restates it.
// Bricks are numbered along the output axes in the order of the input axes they run along, and each XCD takes one contiguous run of
// them: neighbours in the source share an L2.  n_outside: one ballot and one device add per wave, spread over 256 words (CXR_SHARDS).
// No scratch, no other atomics.
// DESIGN.md section 9p has the resources.
#pragma clang fp contract(off)
#include <cmath>
#include <cstring>
#include <new>
#include <utility>

#include "cx_dev.h"
#include "cx_gridop.h"

#define CXR_LIMIT 1048576.0               // |matrix|, |offset| <= 2^20
#define CXR_TABLE_MAX (1LL << 20)         // entries of the table kernel's table; a longer output takes the general kernel
// n_outside is added up in CXR_SHARDS words, one per 128-byte line, and summed on the host: adds to one address run at about 88 per
// microsecond whoever issues them, and under a rotation a sixth of the waves of a 512^3 output have one to make: with one word that
// was most of the call's time
#define CXR_SHARDS 256u
#define CXR_SHARD_WORDS 16u

struct cxr_ent {      // 24 bytes
    double t;             // order 1: c - floor(c)
    int32_t lo, hi;       // the indices read for floor(c) and floor(c) + 1 (order 0: lo for floor(c + 0.5)); -1: cval
    uint32_t outside;     // c < 0 or c > n - 1
    uint32_t pad;
};

struct cx_resample_state : cx_slot {
    cx_buf<cxr_ent> table;
    cx_buf<unsigned long long> count;     // the shards of n_outside
    unsigned long long shards[CXR_SHARDS * CXR_SHARD_WORDS];      // ... and where they land on the host
    int32_t dtype = CX_DTYPE_F32;      // of the result
    int64_t n_outside = 0;
};

void cx_resample_free(cx_ctx* ctx) {
    delete ctx->resample;
    ctx->resample = nullptr;
}

struct cxr_args {
    const void* in;
    void* out;
    const cxr_ent* table;
    unsigned long long* count;  // [CXR_SHARDS] words CXR_SHARD_WORDS apart
    double M[3][4];            // row a: offset[a], M[a][0], M[a][1], M[a][2]
    int64_t n[3], m[3];        // input and output shape
    int64_t toff[3];           // table: the first entry of input axis a ...
    int32_t tax[3];            // ... which output axis tax[a] indexes
    int32_t mode, order;
    double fill;               // order 1: (double)(float)cval
    uint32_t fill_bits;        // order 0: cval in the input's type
    int32_t lb[3];             // log2 of the brick's sides
    int32_t slot[3];           // where output axis k stands in the numbering of the bricks: 0 slowest .. 2 fastest
    int64_t gs[3];             // bricks along the axis in slot s
    unsigned long long bricks;
};

__device__ __forceinline__ double cxr_coord(const double (&r)[4], int64_t i0, int64_t i1, int64_t i2) {
    return ((r[0] + r[1] * (double)i0) + r[2] * (double)i1) + r[3] * (double)i2;
}

// |c| < 2^53: floor(c) fits an int64 and c - floor(c) is exact
__device__ __forceinline__ cxr_ent cxr_entry(double c, int64_t n, int32_t mode, int32_t order) {
    cxr_ent e;
    e.outside = (c < 0.0 || c > (double)(n - 1)) ? 1u : 0u;
    e.pad = 0u;
    if (order == 0) {
        e.lo = e.hi = cxd_boundary_src((int64_t)floor(c + 0.5), n, mode);
        e.t = 0.0;
    } else {
        const double f = floor(c);
        const int64_t j = (int64_t)f;
        e.t = c - f;
        e.lo = cxd_boundary_src(j, n, mode);
        e.hi = cxd_boundary_src(j + 1, n, mode);
    }
    return e;
}

__global__ __launch_bounds__(256) void cxr_k_table(const cxr_args A) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const int32_t k = A.tax[a];
        const int64_t len = k == 0 ? A.m[0] : k == 1 ? A.m[1] : A.m[2], i = e - A.toff[a];
        if (i >= 0 && i < len)
            ((cxr_ent*)A.table)[e] = cxr_entry(cxr_coord(A.M[a], k == 0 ? i : 0, k == 1 ? i : 0, k == 2 ? i : 0), A.n[a], A.mode, A.order);
    }
}

// the lane's output sample: false beyond the output (a partial brick)
__device__ __forceinline__ bool cxr_place(const cxr_args& A, int64_t& i0, int64_t& i1, int64_t& i2) {
    // bricks b and b + 8 share an XCD: XCD x takes the bricks [x q + min(x, r), ...) of the numbering, q = bricks / 8, r = bricks % 8
    const unsigned long long b = blockIdx.x, q = A.bricks >> 3, r = A.bricks & 7ull, x = b & 7ull;
    unsigned long long id = x * q + (x < r ? x : r) + (b >> 3);
    const int64_t s2 = (int64_t)(id % (unsigned long long)A.gs[2]);
    id /= (unsigned long long)A.gs[2];
    const int64_t s1 = (int64_t)(id % (unsigned long long)A.gs[1]), s0 = (int64_t)(id / (unsigned long long)A.gs[1]);
    const uint32_t t = threadIdx.x;
    const uint32_t d2 = t & ((1u << A.lb[2]) - 1u), d1 = (t >> A.lb[2]) & ((1u << A.lb[1]) - 1u), d0 = t >> (A.lb[2] + A.lb[1]);
    i0 = ((A.slot[0] == 0 ? s0 : A.slot[0] == 1 ? s1 : s2) << A.lb[0]) + d0;
    i1 = ((A.slot[1] == 0 ? s0 : A.slot[1] == 1 ? s1 : s2) << A.lb[1]) + d1;
    i2 = ((A.slot[2] == 0 ? s0 : A.slot[2] == 1 ? s1 : s2) << A.lb[2]) + d2;
    return d0 < (1u << A.lb[0]) && i0 < A.m[0] && i1 < A.m[1] && i2 < A.m[2];
}

template <bool TABLE>
__device__ __forceinline__ cxr_ent cxr_entry_of(const cxr_args& A, int a, int64_t i0, int64_t i1, int64_t i2) {
    if constexpr (TABLE) {
        const int32_t k = A.tax[a];
        return A.table[A.toff[a] + (k == 0 ? i0 : k == 1 ? i1 : i2)];
    } else return cxr_entry(cxr_coord(A.M[a], i0, i1, i2), A.n[a], A.mode, A.order);
}

// every lane of the wave calls it
__device__ __forceinline__ void cxr_count_outside(const cxr_args& A, bool outside) {
    const unsigned long long mask = __ballot(outside);
    if (mask != 0ull && (threadIdx.x & 63u) == 0u)
        atomicAdd(A.count + (size_t)((blockIdx.x * 4u + (threadIdx.x >> 6)) & (CXR_SHARDS - 1u)) * CXR_SHARD_WORDS, (unsigned long long)__popcll(mask));
}

__device__ __forceinline__ double cxr_lerp(double a, double b, double t) {
    return t == 0.0 ? a : a + t * (b - a);
}

// order 1.  Every load is unconditional, from an index inside the array; cval takes its place afterwards
template <int DT, bool TABLE>
__global__ __launch_bounds__(256) void cxr_k_linear(const cxr_args A) {
    int64_t i0, i1, i2;
    const bool active = cxr_place(A, i0, i1, i2);
    bool outside = false;
    if (active) {
        const cxr_ent e0 = cxr_entry_of<TABLE>(A, 0, i0, i1, i2), e1 = cxr_entry_of<TABLE>(A, 1, i0, i1, i2), e2 = cxr_entry_of<TABLE>(A, 2, i0, i1, i2);
        outside = (e0.outside | e1.outside | e2.outside) != 0u;
        const cx_grid_ref ref = {A.in, DT};
        const size_t n1 = (size_t)A.n[1], n2 = (size_t)A.n[2];
        const int32_t x0[2] = {e0.lo, e0.hi}, x1[2] = {e1.lo, e1.hi}, x2[2] = {e2.lo, e2.hi};
        double s[2][2][2];
#pragma unroll
        for (int d0 = 0; d0 < 2; d0++)
#pragma unroll
            for (int d1 = 0; d1 < 2; d1++)
#pragma unroll
                for (int d2 = 0; d2 < 2; d2++) {
                    const bool fill = (x0[d0] | x1[d1] | x2[d2]) < 0;
                    const size_t at = ((size_t)(x0[d0] < 0 ? 0 : x0[d0]) * n1 + (size_t)(x1[d1] < 0 ? 0 : x1[d1])) * n2 + (size_t)(x2[d2] < 0 ? 0 : x2[d2]);
                    const double v = (double)cx_sample<DT>(ref, at);
                    s[d0][d1][d2] = fill ? A.fill : v;
                }
        const double a00 = cxr_lerp(s[0][0][0], s[0][0][1], e2.t), a01 = cxr_lerp(s[0][1][0], s[0][1][1], e2.t);
        const double a10 = cxr_lerp(s[1][0][0], s[1][0][1], e2.t), a11 = cxr_lerp(s[1][1][0], s[1][1][1], e2.t);
        const double b0 = cxr_lerp(a00, a01, e1.t), b1 = cxr_lerp(a10, a11, e1.t);
        static_cast<float*>(A.out)[((size_t)i0 * (size_t)A.m[1] + (size_t)i1) * (size_t)A.m[2] + (size_t)i2] = (float)cxr_lerp(b0, b1, e0.t);
    }
    cxr_count_outside(A, outside);
}

// order 0: T is an unsigned integer of the sample's size, its bytes are copied
template <typename T, bool TABLE>
__global__ __launch_bounds__(256) void cxr_k_nearest(const cxr_args A) {
    int64_t i0, i1, i2;
    const bool active = cxr_place(A, i0, i1, i2);
    bool outside = false;
    if (active) {
        const cxr_ent e0 = cxr_entry_of<TABLE>(A, 0, i0, i1, i2), e1 = cxr_entry_of<TABLE>(A, 1, i0, i1, i2), e2 = cxr_entry_of<TABLE>(A, 2, i0, i1, i2);
        outside = (e0.outside | e1.outside | e2.outside) != 0u;
        const bool fill = (e0.lo | e1.lo | e2.lo) < 0;
        const size_t at = ((size_t)(e0.lo < 0 ? 0 : e0.lo) * (size_t)A.n[1] + (size_t)(e1.lo < 0 ? 0 : e1.lo)) * (size_t)A.n[2] + (size_t)(e2.lo < 0 ? 0 : e2.lo);
        const T v = static_cast<const T*>(A.in)[at];
        static_cast<T*>(A.out)[((size_t)i0 * (size_t)A.m[1] + (size_t)i1) * (size_t)A.m[2] + (size_t)i2] = fill ? (T)A.fill_bits : v;
    }
    cxr_count_outside(A, outside);
}

static int32_t cxr_ceil_log2(int64_t m) {
    int32_t l = 0;
    while ((1LL << l) < m) l++;
    return l;
}

// the brick: `want` bits per axis, none beyond the axis's own length; what an axis cannot take goes to the axes in `prefer` order
static void cxr_brick(cxr_args& A, const int32_t want[3], const int prefer[3]) {
    int32_t spare = 0;
    for (int k = 0; k < 3; k++) {
        const int32_t cap = cxr_ceil_log2(A.m[k]);
        A.lb[k] = want[k] < cap ? want[k] : cap;
        spare += want[k] - A.lb[k];
    }
    for (int p = 0; p < 3 && spare > 0; p++) {
        const int k = prefer[p];
        const int32_t cap = cxr_ceil_log2(A.m[k]);
        while (spare > 0 && A.lb[k] < cap) { A.lb[k]++; spare--; }
    }
}

extern "C" int cx_grid_resample3d(cx_ctx* ctx, const void* samples, int32_t dtype, int on_device, int64_t n0, int64_t n1, int64_t n2,
                                  const double matrix[9], const double offset[3], const int64_t out_shape[3], int32_t order, int32_t mode,
                                  double cval, void* out_device, void* out_host, int64_t* n_outside) {
    if (!ctx) return CX_ERR_INVALID;
    if (!matrix || !offset || !out_shape) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_resample3d: no matrix, offset or output shape");
    if (order != 0 && order != 1) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_resample3d: order 0 or 1");
    if (mode != CX_FILTER_NEAREST && mode != CX_FILTER_REFLECT && mode != CX_FILTER_CONSTANT) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_resample3d: unknown mode");
    if (!std::isfinite(cval)) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_resample3d: cval is NaN or infinite");
    for (int e = 0; e < 12; e++) {
        const double x = e < 9 ? matrix[e] : offset[e - 9];
        if (!std::isfinite(x) || std::fabs(x) > CXR_LIMIT) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_resample3d: matrix and offset are finite and at most 2^20 in magnitude");
    }
    const int64_t m0 = out_shape[0], m1 = out_shape[1], m2 = out_shape[2];
    if (m0 < 1 || m1 < 1 || m2 < 1 || m0 > (1LL << 31) || m1 > (1LL << 31) || m2 > (1LL << 31) || m0 * m1 > (1LL << 31) || m0 * m1 * m2 > (1LL << 31))
        return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_resample3d: at least 1 output sample per axis, at most 2^31 in all");
    cx_source src;
    int rc = cx_source_resolve(ctx, "cx_grid_resample3d", samples, dtype, on_device, n0, n1, n2, 31, &src);
    if (rc) return rc;
    dtype = src.dtype; n0 = src.n[0]; n1 = src.n[1]; n2 = src.n[2];
    cxr_args A;
    memset(&A, 0, sizeof(A));
    if (order == 0 && !cx_dtype_value_bits(dtype, cval, A.fill_bits)) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_resample3d: cval is not a value of the sample type (order 0)");
    const int32_t out_dtype = order == 0 ? dtype : CX_DTYPE_F32;
    const size_t out_bytes = (size_t)(m0 * m1 * m2) * cx_dtype_size(out_dtype);
    if (out_device && src.on_device && cx_overlap(src.p, src.bytes, out_device, out_bytes))
        return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_resample3d: the output overlaps the input");
    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_resample_state* S = cx_state_of(ctx->resample);
    if (!S) return CX_ERR_NOMEM;
    hipStream_t st = ctx->stream;
    const void* dev;
    void* final_out;
    if ((rc = S->stage(ctx, src, &dev)) || (rc = S->open(ctx, out_device, out_bytes, &final_out))) return rc;
    const size_t count_words = (size_t)CXR_SHARDS * CXR_SHARD_WORDS;
    if ((rc = S->count.grow(ctx, count_words))) return rc;
    CX_HIP(ctx, hipMemsetAsync(S->count, 0, count_words * sizeof(unsigned long long), st));
    A.in = dev; A.out = final_out; A.count = S->count.get();
    A.n[0] = n0; A.n[1] = n1; A.n[2] = n2; A.m[0] = m0; A.m[1] = m1; A.m[2] = m2;
    A.mode = mode; A.order = order; A.fill = (double)(float)cval;
    for (int a = 0; a < 3; a++) {
        A.M[a][0] = offset[a];
        for (int k = 0; k < 3; k++) A.M[a][1 + k] = matrix[3 * a + k];
    }
    // which output axis runs most nearly along each input axis, input axis 2 choosing first: `along[a]`
    int along[3] = {-1, -1, -1};
    bool taken[3] = {false, false, false};
    for (int a = 2; a >= 0; a--) {
        int best = -1;
        for (int k = 0; k < 3; k++)
            if (!taken[k] && (best < 0 || std::fabs(matrix[3 * a + k]) > std::fabs(matrix[3 * a + best]))) best = k;
        along[a] = best; taken[best] = true;
    }
    // the table kernel: every row of the matrix has at most one entry, and the entries of all output indices are few
    bool table = true;
    int64_t entries = 0;
    for (int a = 0; a < 3; a++) {
        int nz = 0;
        for (int k = 0; k < 3; k++)
            if (matrix[3 * a + k] != 0.0) { nz++; A.tax[a] = k; }
        if (nz > 1) table = false;
        A.toff[a] = entries;
        entries += A.m[A.tax[a]];
    }
    if (entries > CXR_TABLE_MAX) table = false;
    if (table) {
        const int32_t want[3] = {1, 1, 6};
        const int prefer[3] = {2, 1, 0};
        cxr_brick(A, want, prefer);
        if ((rc = S->table.grow(ctx, (size_t)entries))) return rc;
        A.table = S->table.get();
        hipLaunchKernelGGL(cxr_k_table, cx_grid1((size_t)entries), dim3(256), 0, st, A);
        CX_HIP(ctx, hipGetLastError());
    } else {
        int32_t want[3] = {2, 2, 2};
        want[along[2]] = 4;
        const int prefer[3] = {along[2], along[1], along[0]};
        cxr_brick(A, want, prefer);
    }
    int64_t g[3];
    for (int k = 0; k < 3; k++) g[k] = (A.m[k] + (1LL << A.lb[k]) - 1) >> A.lb[k];
    for (int a = 0; a < 3; a++) { A.slot[along[a]] = a; A.gs[a] = g[along[a]]; }
    A.bricks = (unsigned long long)g[0] * (unsigned long long)g[1] * (unsigned long long)g[2];      // (<= 2^31: a brick holds a sample at least)
    const dim3 grid((uint32_t)A.bricks);
    if (order == 1) {
#define CX_LAUNCH(DT)                                                                            \
    if (table) hipLaunchKernelGGL((cxr_k_linear<DT, true>), grid, dim3(256), 0, st, A);          \
    else hipLaunchKernelGGL((cxr_k_linear<DT, false>), grid, dim3(256), 0, st, A);
        CX_DISPATCH_DTYPE(dtype, CX_LAUNCH)
#undef CX_LAUNCH
    } else {
#define CX_LAUNCH(T)                                                                             \
    if (table) hipLaunchKernelGGL((cxr_k_nearest<T, true>), grid, dim3(256), 0, st, A);          \
    else hipLaunchKernelGGL((cxr_k_nearest<T, false>), grid, dim3(256), 0, st, A);
        switch (cx_dtype_size(dtype)) {
            case 1: CX_LAUNCH(uint8_t) break;
            case 2: CX_LAUNCH(uint16_t) break;
            default: CX_LAUNCH(uint32_t) break;
        }
#undef CX_LAUNCH
    }
    CX_HIP(ctx, hipGetLastError());
    static_assert(sizeof(S->shards) == (size_t)CXR_SHARDS * CXR_SHARD_WORDS * sizeof(unsigned long long), "the host copy of the shards");
    CX_HIP(ctx, hipMemcpyAsync(S->shards, S->count, sizeof(S->shards), hipMemcpyDeviceToHost, st));
    if (out_host) CX_HIP(ctx, hipMemcpyAsync(out_host, final_out, out_bytes, hipMemcpyDeviceToHost, st));
    CX_HIP(ctx, hipStreamSynchronize(st));      // the count is the caller's, and its host memory is its own again
    unsigned long long count = 0;
    for (uint32_t k = 0; k < CXR_SHARDS; k++) count += S->shards[k * CXR_SHARD_WORDS];
    if (!out_device) { S->publish(m0, m1, m2); S->dtype = out_dtype; S->n_outside = (int64_t)count; }
    if (n_outside) *n_outside = (int64_t)count;
    return CX_OK;
}

extern "C" int cx_grid_resample3d_result(cx_ctx* ctx, void** out_device, int64_t out_shape[3], int32_t* out_dtype, int64_t* n_outside) {
    if (!ctx) return CX_ERR_INVALID;
    const cx_resample_state* S = ctx->resample;
    const int rc = cx_slot_result(ctx, S, "cx_grid_resample3d_result: no result of cx_grid_resample3d in the context", out_device, out_shape);
    if (rc) return rc;
    if (out_dtype) *out_dtype = S->dtype;
    if (n_outside) *n_outside = S->n_outside;
    return CX_OK;
}

extern "C" int cx_grid_resample3d_bind(cx_ctx* ctx) {
    if (!ctx) return CX_ERR_INVALID;
    cx_resample_state* S = ctx->resample;
    return cx_slot_bind(ctx, S, "cx_grid_resample3d_bind: no result of cx_grid_resample3d in the context", S ? S->dtype : 0);
}
