// cx_rank.hip -- rank filters of a volume (include/contourist_hip.h, section "rank filters"): the element at position `rank` of the
// sorted window around every sample of a 3-D array of any CX_DTYPE_*, in the array's own type (cx_grid_rank3d), and the result as the
// bound grid (cx_grid_rank3d_bind).  Median, percentile, grey erosion and dilation are ranks of it.
//
// Nothing is computed: a sample is selected.  Every sample becomes a key of its own width (8, 16 or 32 bits) whose unsigned order is
// the header's order and which has an inverse (cx_dev.h: cxd_orderable32 / 16; integers: the sign bit flipped), the selection works on
// keys, and the selected key is turned back on the way out.  Every NaN has the one key of all ones and comes back as the canonical
// quiet NaN.
//
// A workgroup of 256 threads owns a tile of CXQ_T0 x CXQ_T1 x CXQ_T2 = 4 x 4 x 64 outputs.  It stages the keys of the tile and its
// halo, (4 + s0 - 1) x (4 + s1 - 1) x (64 + s2 - 1) of them, in LDS once, boundary rule and cval applied, so that the selection never
// looks at the array again.  Two ways to select:
//   cxq_k_rank     any footprint, any rank.  The footprint's offsets into the staged halo are a table in LDS (at most 343 words, built
//                  from the 343 mask bits in the kernel's arguments).  Wave w takes row d1 = w of the tile, the lanes run along axis 2,
//                  and a lane selects its four outputs d0 = 0..3 together, so a table entry is read once for four keys.  The key is
//                  found bit by bit from the top: with the bits above b decided (`pre`), bit b is set iff at most `rank` entries of the
//                  window are below pre | 1 << b.  8, 16 or 32 passes over W LDS reads per output; the lanes of a wave read
//                  neighbouring addresses, no barrier inside.
//   cxq_k_extreme  rank 0 or W - 1 of a full box (no mask given): minimum and maximum are separable, so three running passes inside the
//                  staged tile -- along axis 2 into a second LDS array, along axis 1 back into the first, along axis 0 into memory --
//                  cost (s2, s1, s0) reads per element they produce in place of s0 s1 s2 times the key's bits.
// Both give the same bytes.  No scratch, no atomics.  Tiles are numbered with axis 2 fastest and each XCD takes one contiguous run of
// them, so that neighbours share their halos in one L2.  DESIGN.md section 9q has the budget and the measurements.
#include <cmath>
#include <cstring>
#include <new>
#include <utility>

#include "cx_dev.h"
#include "cx_gridop.h"

#define CXQ_T0 4
#define CXQ_T1 4
#define CXQ_T2 64
#define CXQ_MAX_SIZE 7                                     // per axis of the footprint's box
#define CXQ_MASK_WORDS 11                                  // 343 bits
#define CXQ_TAB_BYTES 1376u                                // 343 words, rounded up to 16 bytes

struct cx_rank_state : cx_slot {
    int32_t dtype = CX_DTYPE_F32;      // of the result
};

void cx_rank_free(cx_ctx* ctx) {
    delete ctx->rank;
    ctx->rank = nullptr;
}

struct cxq_args {
    const void* in;
    void* out;
    int64_t n[3];
    int32_t s[3], o[3];                  // the box and the origin
    uint32_t mask[CXQ_MASK_WORDS];       // bit (d0 s1 + d1) s2 + d2: the offset belongs to the footprint
    uint32_t rank;
    int32_t mode, dtype;
    uint32_t fill_key;                   // the key of cval
    uint32_t take_max;                   // cxq_k_extreme: 1 = the maximum
    uint32_t g1, g2;                     // tiles along axes 1 and 2
    unsigned long long tiles;
};

__device__ __forceinline__ uint32_t cxq_key(int32_t dtype, uint32_t raw) { return cxd_sample_key(dtype, raw); }
__device__ __forceinline__ uint32_t cxq_unkey(int32_t dtype, uint32_t key) { return cxd_sample_unkey(dtype, key); }

// the first output of this workgroup's tile
__device__ __forceinline__ void cxq_place(const cxq_args& A, int64_t& b0, int64_t& b1, int64_t& b2) {
    // tiles t and t + 8 share an XCD: XCD x takes the tiles [x q + min(x, r), ...) of the numbering, q = tiles / 8, r = tiles % 8
    const unsigned long long b = blockIdx.x, q = A.tiles >> 3, r = A.tiles & 7ull, x = b & 7ull;
    unsigned long long id = x * q + (x < r ? x : r) + (b >> 3);
    b2 = (int64_t)(id % A.g2) * CXQ_T2;
    id /= A.g2;
    b1 = (int64_t)(id % A.g1) * CXQ_T1;
    b0 = (int64_t)(id / A.g1) * CXQ_T0;
}

// the keys of the tile and its halo: keys[(h0 H1 + h1) H2 + h2] is the key of the element at b + h - o, every index inside the array
// by the boundary rule or the key of cval
template <typename K>
__device__ __forceinline__ void cxq_stage(const cxq_args& A, K* keys, int64_t b0, int64_t b1, int64_t b2, uint32_t H0, uint32_t H1, uint32_t H2) {
    const K* __restrict__ in = static_cast<const K*>(A.in);
    const uint32_t total = H0 * H1 * H2;
    for (uint32_t e = threadIdx.x; e < total; e += 256u) {
        const uint32_t row = e / H2, h2 = e - row * H2, h0 = row / H1, h1 = row - h0 * H1;
        const int32_t j0 = cxd_boundary_src(b0 + (int64_t)h0 - A.o[0], A.n[0], A.mode);
        const int32_t j1 = cxd_boundary_src(b1 + (int64_t)h1 - A.o[1], A.n[1], A.mode);
        const int32_t j2 = cxd_boundary_src(b2 + (int64_t)h2 - A.o[2], A.n[2], A.mode);
        uint32_t key = A.fill_key;
        if ((j0 | j1 | j2) >= 0) key = cxq_key(A.dtype, (uint32_t)in[((size_t)j0 * (size_t)A.n[1] + (size_t)j1) * (size_t)A.n[2] + (size_t)j2]);
        keys[e] = (K)key;
    }
}

extern __shared__ __align__(16) unsigned char cxq_smem[];

template <typename K>
__global__ __launch_bounds__(256) void cxq_k_rank(const cxq_args A) {
    constexpr int BITS = 8 * (int)sizeof(K);
    uint32_t* tab = reinterpret_cast<uint32_t*>(cxq_smem);
    K* keys = reinterpret_cast<K*>(cxq_smem + CXQ_TAB_BYTES);
    const uint32_t H0 = CXQ_T0 + (uint32_t)A.s[0] - 1u, H1 = CXQ_T1 + (uint32_t)A.s[1] - 1u, H2 = CXQ_T2 + (uint32_t)A.s[2] - 1u;
    int64_t b0, b1, b2;
    cxq_place(A, b0, b1, b2);
    cxq_stage<K>(A, keys, b0, b1, b2, H0, H1, H2);
    // the table: the footprint's e-th set bit, in C order, as an offset into the staged keys
    const uint32_t box = (uint32_t)(A.s[0] * A.s[1] * A.s[2]), s12 = (uint32_t)(A.s[1] * A.s[2]);
    uint32_t W = 0;
#pragma unroll
    for (int w = 0; w < CXQ_MASK_WORDS; w++) W += (uint32_t)__popc(A.mask[w]);
    for (uint32_t e = threadIdx.x; e < box; e += 256u) {
        uint32_t before = 0, word = 0;
#pragma unroll
        for (int w = 0; w < CXQ_MASK_WORDS; w++) {
            const uint32_t m = A.mask[w];
            if ((uint32_t)w < (e >> 5)) before += (uint32_t)__popc(m);
            if ((uint32_t)w == (e >> 5)) word = m;
        }
        if ((word >> (e & 31u)) & 1u) {
            const uint32_t d0 = e / s12, rest = e - d0 * s12, d1 = rest / (uint32_t)A.s[2], d2 = rest - d1 * (uint32_t)A.s[2];
            tab[before + (uint32_t)__popc(word & ((1u << (e & 31u)) - 1u))] = (d0 * H1 + d1) * H2 + d2;
        }
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, d1 = threadIdx.x >> 6;
    const int64_t i1 = b1 + d1, i2 = b2 + lane;
    if (i1 >= A.n[1]) return;      // (the whole wave)
    const uint32_t plane = H1 * H2;
    const K* __restrict__ mine = keys + d1 * H2 + lane;
    uint32_t pre[CXQ_T0];
#pragma unroll
    for (int j = 0; j < CXQ_T0; j++) pre[j] = 0u;
    for (int b = BITS - 1; b >= 0; b--) {
        uint32_t cand[CXQ_T0], below[CXQ_T0];
#pragma unroll
        for (int j = 0; j < CXQ_T0; j++) { cand[j] = pre[j] | (1u << b); below[j] = 0u; }
#pragma unroll 4
        for (uint32_t e = 0; e < W; e++) {
            const K* __restrict__ at = mine + tab[e];
#pragma unroll
            for (int j = 0; j < CXQ_T0; j++) below[j] += ((uint32_t)at[j * plane] < cand[j]) ? 1u : 0u;
        }
#pragma unroll
        for (int j = 0; j < CXQ_T0; j++) pre[j] = below[j] <= A.rank ? cand[j] : pre[j];
    }
    if (i2 >= A.n[2]) return;
    K* __restrict__ out = static_cast<K*>(A.out);
#pragma unroll
    for (int j = 0; j < CXQ_T0; j++)
        if (b0 + j < A.n[0]) out[((size_t)(b0 + j) * (size_t)A.n[1] + (size_t)i1) * (size_t)A.n[2] + (size_t)i2] = (K)cxq_unkey(A.dtype, pre[j]);
}

template <typename K>
__global__ __launch_bounds__(256) void cxq_k_extreme(const cxq_args A) {
    const uint32_t s0 = (uint32_t)A.s[0], s1 = (uint32_t)A.s[1], s2 = (uint32_t)A.s[2];
    const uint32_t H0 = CXQ_T0 + s0 - 1u, H1 = CXQ_T1 + s1 - 1u, H2 = CXQ_T2 + s2 - 1u;
    K* a = reinterpret_cast<K*>(cxq_smem);      // [H0][H1][H2], then [H0][T1][T2]
    K* b = a + H0 * H1 * H2;                    // [H0][H1][T2]
    const bool take_max = A.take_max != 0u;
    int64_t b0, b1, b2;
    cxq_place(A, b0, b1, b2);
    cxq_stage<K>(A, a, b0, b1, b2, H0, H1, H2);
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < H0 * H1 * CXQ_T2; e += 256u) {      // along axis 2
        const K* __restrict__ at = a + (e >> 6) * H2 + (e & 63u);
        uint32_t m = at[0];
        for (uint32_t k = 1; k < s2; k++) { const uint32_t v = at[k]; m = take_max ? max(m, v) : min(m, v); }
        b[e] = (K)m;
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < H0 * CXQ_T1 * CXQ_T2; e += 256u) {      // along axis 1
        const K* __restrict__ at = b + ((e >> 8) * H1 + ((e >> 6) & 3u)) * CXQ_T2 + (e & 63u);
        uint32_t m = at[0];
        for (uint32_t k = 1; k < s1; k++) { const uint32_t v = at[k * CXQ_T2]; m = take_max ? max(m, v) : min(m, v); }
        a[e] = (K)m;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, d1 = threadIdx.x >> 6;      // along axis 0
    const int64_t i1 = b1 + d1, i2 = b2 + lane;
    if (i1 >= A.n[1] || i2 >= A.n[2]) return;
    K* __restrict__ out = static_cast<K*>(A.out);
    for (uint32_t d0 = 0; d0 < CXQ_T0 && b0 + d0 < A.n[0]; d0++) {
        const K* __restrict__ at = a + (d0 * CXQ_T1 + d1) * CXQ_T2 + lane;
        uint32_t m = at[0];
        for (uint32_t k = 1; k < s0; k++) { const uint32_t v = at[k * CXQ_T1 * CXQ_T2]; m = take_max ? max(m, v) : min(m, v); }
        out[((size_t)(b0 + d0) * (size_t)A.n[1] + (size_t)i1) * (size_t)A.n[2] + (size_t)i2] = (K)cxq_unkey(A.dtype, m);
    }
}

static_assert(CXQ_T1 == 4 && CXQ_T2 == 64 && CXQ_T1 * CXQ_T2 == 256, "a wave per row of the tile, a lane per sample of the row");
static_assert(CXQ_MAX_SIZE * CXQ_MAX_SIZE * CXQ_MAX_SIZE <= 32 * CXQ_MASK_WORDS, "a mask bit per offset of the largest box");
static_assert(4u * CXQ_MAX_SIZE * CXQ_MAX_SIZE * CXQ_MAX_SIZE <= CXQ_TAB_BYTES && CXQ_TAB_BYTES % 16u == 0u, "a table word per offset of the largest box");

// the key of a sample's bits, as cxq_key makes it (cval is finite: no NaN)
static uint32_t cxq_host_key(int32_t dtype, uint32_t raw) {
    switch (dtype) {
        case CX_DTYPE_U8: case CX_DTYPE_U16: return raw;
        case CX_DTYPE_I8: return raw ^ 0x80u;
        case CX_DTYPE_I16: return raw ^ 0x8000u;
        case CX_DTYPE_F16: case CX_DTYPE_BF16: return (raw & 0x8000u) ? (~raw & 0xFFFFu) : (raw | 0x8000u);
        default: return (raw & 0x80000000u) ? ~raw : (raw | 0x80000000u);
    }
}

extern "C" int cx_grid_rank3d(cx_ctx* ctx, const void* samples, int32_t dtype, int on_device, int64_t n0, int64_t n1, int64_t n2,
                              const int32_t size[3], const int32_t origin[3], const uint8_t* footprint, int32_t rank, int32_t mode, double cval,
                              void* out_device, void* out_host) {
    if (!ctx) return CX_ERR_INVALID;
    if (!size || !origin) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_rank3d: no size or origin");
    if (mode != CX_FILTER_NEAREST && mode != CX_FILTER_REFLECT && mode != CX_FILTER_CONSTANT) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_rank3d: unknown mode");
    if (!std::isfinite(cval)) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_rank3d: cval is NaN or infinite");
    cxq_args A;
    memset(&A, 0, sizeof(A));
    for (int a = 0; a < 3; a++) {
        if (size[a] < 1 || size[a] > CXQ_MAX_SIZE) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_rank3d: a size of 1 to 7 per axis");
        if (origin[a] < 0 || origin[a] >= size[a]) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_rank3d: an origin of 0 to size - 1 per axis");
        A.s[a] = size[a]; A.o[a] = origin[a];
    }
    const int32_t box = size[0] * size[1] * size[2];
    int32_t W = 0;
    for (int32_t e = 0; e < box; e++)
        if (!footprint || footprint[e]) { A.mask[e >> 5] |= 1u << (e & 31); W++; }
    if (W == 0) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_rank3d: the footprint is empty");
    if (rank < 0 || rank >= W) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_rank3d: a rank of 0 to W - 1, W the number of offsets in the footprint");
    cx_source src;
    int rc = cx_source_resolve(ctx, "cx_grid_rank3d", samples, dtype, on_device, n0, n1, n2, 31, &src);
    if (rc) return rc;
    dtype = src.dtype; n0 = src.n[0]; n1 = src.n[1]; n2 = src.n[2];
    uint32_t fill_bits;
    if (!cx_dtype_value_bits(dtype, cval, fill_bits)) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_rank3d: cval is not a value of the sample type");
    const size_t esize = cx_dtype_size(dtype), bytes = src.bytes;
    if (out_device && src.on_device && cx_overlap(src.p, bytes, out_device, bytes)) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_rank3d: the output overlaps the input");
    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_rank_state* S = cx_state_of(ctx->rank);
    if (!S) return CX_ERR_NOMEM;
    hipStream_t st = ctx->stream;
    const void* dev;
    void* final_out;
    if ((rc = S->stage(ctx, src, &dev)) || (rc = S->open(ctx, out_device, bytes, &final_out))) return rc;
    A.in = dev; A.out = final_out;
    A.n[0] = n0; A.n[1] = n1; A.n[2] = n2;
    A.rank = (uint32_t)rank; A.mode = mode; A.dtype = dtype;
    A.fill_key = cxq_host_key(dtype, fill_bits);
    const int64_t g0 = (n0 + CXQ_T0 - 1) / CXQ_T0, g1 = (n1 + CXQ_T1 - 1) / CXQ_T1, g2 = (n2 + CXQ_T2 - 1) / CXQ_T2;
    A.g1 = (uint32_t)g1; A.g2 = (uint32_t)g2;
    A.tiles = (unsigned long long)g0 * (unsigned long long)g1 * (unsigned long long)g2;      // (<= 2^29: a tile holds four samples at least, or the whole axis 0)
    const dim3 grid((uint32_t)A.tiles);
    const size_t halo = (size_t)(CXQ_T0 + size[0] - 1) * (size_t)(CXQ_T1 + size[1] - 1) * (size_t)(CXQ_T2 + size[2] - 1);
    if (!footprint && (rank == 0 || rank == W - 1)) {
        A.take_max = (rank == W - 1 && W > 1) ? 1u : 0u;
        const size_t lds = (halo + (size_t)(CXQ_T0 + size[0] - 1) * (size_t)(CXQ_T1 + size[1] - 1) * CXQ_T2) * esize;      // <= 53600 bytes
        switch (esize) {
            case 1: hipLaunchKernelGGL(cxq_k_extreme<uint8_t>, grid, dim3(256), lds, st, A); break;
            case 2: hipLaunchKernelGGL(cxq_k_extreme<uint16_t>, grid, dim3(256), lds, st, A); break;
            default: hipLaunchKernelGGL(cxq_k_extreme<uint32_t>, grid, dim3(256), lds, st, A); break;
        }
    } else {
        const size_t lds = CXQ_TAB_BYTES + halo * esize;      // <= 29376 bytes
        switch (esize) {
            case 1: hipLaunchKernelGGL(cxq_k_rank<uint8_t>, grid, dim3(256), lds, st, A); break;
            case 2: hipLaunchKernelGGL(cxq_k_rank<uint16_t>, grid, dim3(256), lds, st, A); break;
            default: hipLaunchKernelGGL(cxq_k_rank<uint32_t>, grid, dim3(256), lds, st, A); break;
        }
    }
    CX_HIP(ctx, hipGetLastError());
    if (out_host) CX_HIP(ctx, hipMemcpyAsync(out_host, final_out, bytes, hipMemcpyDeviceToHost, st));
    CX_HIP(ctx, hipStreamSynchronize(st));      // the caller's host memory is its own again
    if (!out_device) { S->publish(n0, n1, n2); S->dtype = dtype; }
    return CX_OK;
}

extern "C" int cx_grid_rank3d_result(cx_ctx* ctx, void** out_device, int64_t out_shape[3], int32_t* out_dtype) {
    if (!ctx) return CX_ERR_INVALID;
    const int rc = cx_slot_result(ctx, ctx->rank, "cx_grid_rank3d_result: no result of cx_grid_rank3d in the context", out_device, out_shape);
    if (rc == CX_OK && out_dtype) *out_dtype = ctx->rank->dtype;
    return rc;
}

extern "C" int cx_grid_rank3d_bind(cx_ctx* ctx) {
    if (!ctx) return CX_ERR_INVALID;
    cx_rank_state* S = ctx->rank;
    return cx_slot_bind(ctx, S, "cx_grid_rank3d_bind: no result of cx_grid_rank3d in the context", S ? S->dtype : 0);
}
