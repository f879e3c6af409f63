// cx_dist.hip -- the exact Euclidean distance transform of a thresholded volume (include/contourist_hip.h, section "distance fields"):
// cx_grid_distance3d, its pending result (cx_grid_distance3d_result) and the result as the bound grid (cx_grid_distance3d_bind).
//
// The header fixes the value of every sample: per axis a minimum over candidates of fl(g + fl(w d^2)), last axis first.  A minimum does
// not depend on the order its candidates are visited in, and a candidate is skipped here only where fl(w d^2) >= the best so far
// (g >= 0 and fl is monotone, so neither it nor any candidate further out can be smaller).  No product is fused with a sum: the file
// is compiled with contraction off (a fused fl(g + w d^2) is one rounding where the contract has two).
//
// One signed double per sample between the passes.  A sample is LOW or it is not, on every axis: the transform whose sites include
// the sample is 0 there, the other one is > 0, so  s = gA - gB  carries both (s < 0: low, gB = -s; s > 0: not low, gA = s; never 0),
// and a sample only ever searches for the nearest sample of the other class.  CX_DIST_SIGNED costs what one side costs.
//
// Lanes run along axis 2.  Three trips through memory:
//   cxd_k_rows<DT>   axis 2.  A wave owns a row.  It walks the row's tiles of 64 columns from the far end (classify in the sample's own
//                    type, one ballot per tile, the first set bit above the lane or the nearest position carried over from the tiles
//                    behind), stores fl(w2 dr^2), then walks forward and takes the minimum with fl(w2 dl^2): linear in the row whatever
//                    the sites.  The low samples are counted here (one integer atomic per row).
//   cxd_k_walk<LAST> axis 1, then axis 0.  A wave owns 64 columns of one position of the walked axis; every candidate is a whole
//                    coalesced row segment.  Each lane scans outward from its own sample, four distances (eight loads) in flight, and
//                    stops by the rule above.  LAST writes the requested kind: sign, sqrt and threshold are applied in registers.
// Waves are independent: no workgroup barrier, no LDS.  No float atomics: every call gives the same bits.  DESIGN.md section 9n.
#include <cmath>
#include <cstring>
#include <new>
#include <string>

#include "cx_dev.h"
#include "cx_gridop.h"

#pragma clang fp contract(off)

#define CXD_WAVES 4u
#define CXD_BATCH 4      // distances per round of the outward scan: 2 CXD_BATCH loads in flight

struct cx_dist_state : cx_slot {      // (the result is bytes of `kind`)
    cx_buf<double> a, b;       // the signed squared distances after axis 2 / axis 1
    cx_buf<unsigned long long> nlow;
    int32_t kind = 0;
    int64_t n_sites = 0;
};

void cx_dist_free(cx_ctx* ctx) {
    delete ctx->dist;
    ctx->dist = nullptr;
}

struct cxd_rows_args {
    const void* in;
    double* out;
    unsigned long long* nlow;
    int64_t rows, n2;
    double value, w2;
};

// fl(w d^2): d^2 is the exact integer (converted once: exact below 2^53)
__device__ __forceinline__ double cxd_cost(double w, int64_t d) { return w * (double)(d * d); }

template <int DT>
__global__ __launch_bounds__(256) void cxd_k_rows(const cxd_rows_args A) {
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    const cx_grid_ref G = {A.in, DT};
    const int64_t tiles = (A.n2 + 63) / 64;
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    const u64 above_me = ~((2ull << lane) - 1ull), below_me = (1ull << lane) - 1ull;
    for (int64_t row = (int64_t)blockIdx.x * CXD_WAVES + wave; row < A.rows; row += (int64_t)gridDim.x * CXD_WAVES) {
        const size_t base = (size_t)row * (size_t)A.n2;
        double* __restrict__ out = A.out + base;
        // from the far end: the nearest sample of the other class above this one
        int64_t near_low = -1, near_high = -1;      // the nearest low / non-low sample in the tiles already walked
        unsigned long long count = 0;
        for (int64_t t = tiles - 1; t >= 0; t--) {
            const int64_t k = t * 64 + (int64_t)lane;
            const bool active = k < A.n2;
            const double f = (double)cx_sample<DT>(G, base + (size_t)(active ? k : A.n2 - 1));
            const bool low = active && f < A.value;
            const u64 m = __ballot(low), h = __ballot(active && !low);
            const u64 other = (low ? h : m) & above_me;
            const int64_t far = low ? near_high : near_low;
            double g = inf;
            if (other) g = cxd_cost(A.w2, (int64_t)__builtin_ctzll(other) - (int64_t)lane);
            else if (far >= 0) g = cxd_cost(A.w2, far - k);
            if (active) out[k] = low ? -g : g;
            if (m) near_low = t * 64 + (int64_t)__builtin_ctzll(m);
            if (h) near_high = t * 64 + (int64_t)__builtin_ctzll(h);
            count += (unsigned long long)__builtin_popcountll(m);
        }
        // forward: the nearest one below, and the smaller of the two (every lane reads what it wrote itself)
        near_low = -1; near_high = -1;
        for (int64_t t = 0; t < tiles; t++) {
            const int64_t k = t * 64 + (int64_t)lane;
            const bool active = k < A.n2;
            const double s = active ? out[k] : 0.0;
            const bool low = active && (__double_as_longlong(s) < 0);
            const u64 m = __ballot(low), h = __ballot(active && !low);
            const u64 other = (low ? h : m) & below_me;
            const int64_t far = low ? near_high : near_low;
            double g = low ? -s : s;
            if (other) g = fmin(g, cxd_cost(A.w2, (int64_t)lane - (63 - (int64_t)__builtin_clzll(other))));
            else if (far >= 0) g = fmin(g, cxd_cost(A.w2, k - far));
            if (active) out[k] = low ? -g : g;
            if (m) near_low = t * 64 + 63 - (int64_t)__builtin_clzll(m);
            if (h) near_high = t * 64 + 63 - (int64_t)__builtin_clzll(h);
        }
        if (lane == 0u && count) atomicAdd(A.nlow, count);
    }
}

struct cxd_walk_args {
    const double* in;
    void* out;
    int64_t n;                        // length of the walked axis
    int64_t outer, cols, tiles;       // what is not walked: `outer` rows of `cols` columns, ceil(cols / 64) tiles
    size_t walk_stride, outer_stride; // in samples
    unsigned long long items;
    double w;
    int32_t side, kind;
    double radius2;
};

// the other class's transform at a sample holding s, seen from a low sample (gB) or from one that is not (gA)
__device__ __forceinline__ double cxd_other(double s, bool low) {
    const bool s_low = __double_as_longlong(s) < 0;
    return low ? (s_low ? -s : 0.0) : (s_low ? 0.0 : s);
}

template <bool LAST>
__global__ __launch_bounds__(256) void cxd_k_walk(const cxd_walk_args A) {
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    for (unsigned long long it = (unsigned long long)blockIdx.x * CXD_WAVES + wave; it < A.items; it += (unsigned long long)gridDim.x * CXD_WAVES) {
        const int64_t tile = (int64_t)(it % (unsigned long long)A.tiles), rest = (int64_t)(it / (unsigned long long)A.tiles);
        const int64_t p = rest % A.n, o = rest / A.n;
        const int64_t k = tile * 64 + (int64_t)lane;
        if (k >= A.cols) continue;
        const size_t col = (size_t)o * A.outer_stride + (size_t)k;
        const double* __restrict__ in = A.in + col;
        const double s = in[(size_t)p * A.walk_stride];
        const bool low = __double_as_longlong(s) < 0;
        double best = low ? -s : s;      // d = 0
        const int64_t reach = p > A.n - 1 - p ? p : A.n - 1 - p;
        for (int64_t d0 = 1; d0 <= reach; d0 += CXD_BATCH) {
            if (!(cxd_cost(A.w, d0) < best)) break;      // nothing at d0 or beyond can be smaller
            double x[2 * CXD_BATCH];
#pragma unroll
            for (int b = 0; b < CXD_BATCH; b++) {      // (outside the axis: the lane's own sample once more, a candidate that changes nothing)
                const int64_t d = d0 + b, lo = p - d, hi = p + d;
                x[2 * b] = in[(size_t)(lo >= 0 ? lo : p) * A.walk_stride];
                x[2 * b + 1] = in[(size_t)(hi < A.n ? hi : p) * A.walk_stride];
            }
#pragma unroll
            for (int b = 0; b < CXD_BATCH; b++) {
                const int64_t d = d0 + b, lo = p - d, hi = p + d;
                const double c = cxd_cost(A.w, d);
                const double a0 = cxd_other(x[2 * b], low) + c, a1 = cxd_other(x[2 * b + 1], low) + c;
                if (lo >= 0 && a0 < best) best = a0;
                if (hi < A.n && a1 < best) best = a1;
            }
        }
        const size_t at = col + (size_t)p * A.walk_stride;
        if constexpr (!LAST) static_cast<double*>(A.out)[at] = low ? -best : best;
        else {
            const double gA = low ? 0.0 : best, gB = low ? best : 0.0;
            if (A.kind == CX_DIST_OUT_SQUARED_F64) {
                static_cast<double*>(A.out)[at] = A.side == CX_DIST_BELOW ? gB : A.side == CX_DIST_ABOVE ? gA : gA - gB;
            } else if (A.kind == CX_DIST_OUT_F32) {
                const double rA = sqrt(gA), rB = sqrt(gB);
                static_cast<float*>(A.out)[at] = (float)(A.side == CX_DIST_BELOW ? rB : A.side == CX_DIST_ABOVE ? rA : rA - rB);
            } else {
                static_cast<uint8_t*>(A.out)[at] = (A.side == CX_DIST_BELOW ? gB : gA) <= A.radius2 ? (uint8_t)1 : (uint8_t)0;
            }
        }
    }
}

static size_t cxd_kind_size(int32_t kind) { return kind == CX_DIST_OUT_SQUARED_F64 ? 8u : kind == CX_DIST_OUT_F32 ? 4u : 1u; }
static uint32_t cxd_grid(unsigned long long items) {
    const unsigned long long blocks = (items + CXD_WAVES - 1u) / CXD_WAVES;
    return (uint32_t)(blocks < (1ull << 20) ? (blocks ? blocks : 1ull) : (1ull << 20));
}

extern "C" int cx_grid_distance3d(cx_ctx* ctx, const void* samples, int32_t dtype, int on_device, int64_t n0, int64_t n1, int64_t n2,
                                  double value, const double sampling[3], int32_t side, int32_t out_kind, double radius2,
                                  void* out_device, void* out_host, int64_t* n_sites) {
    if (!ctx) return CX_ERR_INVALID;
    if (!std::isfinite(value)) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_distance3d: value is NaN or infinite");
    if (side != CX_DIST_BELOW && side != CX_DIST_ABOVE && side != CX_DIST_SIGNED) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_distance3d: unknown side");
    if (out_kind != CX_DIST_OUT_SQUARED_F64 && out_kind != CX_DIST_OUT_F32 && out_kind != CX_DIST_OUT_MASK_U8)
        return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_distance3d: unknown output kind");
    if (out_kind == CX_DIST_OUT_MASK_U8) {
        if (side == CX_DIST_SIGNED) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_distance3d: a mask of a signed distance");
        if (!std::isfinite(radius2) || radius2 < 0.0) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_distance3d: radius2 is a finite number >= 0");
    }
    double w[3] = {1.0, 1.0, 1.0};
    if (sampling)
        for (int a = 0; a < 3; a++) {
            if (!std::isfinite(sampling[a]) || !(sampling[a] > 0.0)) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_distance3d: sampling is finite and > 0 on every axis");
            w[a] = sampling[a] * sampling[a];
            if (!std::isnormal(w[a])) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_distance3d: the square of a sampling step is not a normal double");
        }
    cx_source S;
    int rc = cx_source_resolve(ctx, "cx_grid_distance3d", samples, dtype, on_device, n0, n1, n2, 29, &S);
    if (rc) return rc;
    n0 = S.n[0]; n1 = S.n[1]; n2 = S.n[2];
    const size_t count = S.count, out_bytes = count * cxd_kind_size(out_kind);
    if (out_device && S.on_device && cx_overlap(S.p, S.bytes, out_device, out_bytes))
        return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_distance3d: the output overlaps the input");
    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_dist_state* D = cx_state_of(ctx->dist);
    if (!D) return CX_ERR_NOMEM;
    hipStream_t st = ctx->stream;
    const void* dev;
    void* final_out;
    // (the result of the call before may be the input of this one: the second step of an opening or closing)
    if ((rc = D->stage(ctx, S, &dev)) || (rc = D->open(ctx, out_device, out_bytes, &final_out))) return rc;
    if ((rc = D->a.grow(ctx, count)) || (rc = D->b.grow(ctx, count)) || (rc = D->nlow.grow(ctx, 1))) return rc;
    CX_HIP(ctx, hipMemsetAsync(D->nlow, 0, sizeof(unsigned long long), st));
    cxd_rows_args R;
    memset(&R, 0, sizeof(R));
    R.in = dev; R.out = D->a.get(); R.nlow = D->nlow.get();
    R.rows = n0 * n1; R.n2 = n2; R.value = value; R.w2 = w[2];
#define CX_LAUNCH(DT) hipLaunchKernelGGL((cxd_k_rows<DT>), dim3(cxd_grid((unsigned long long)R.rows)), dim3(256), 0, st, R);
    CX_DISPATCH_DTYPE(S.dtype, CX_LAUNCH)
#undef CX_LAUNCH
    CX_HIP(ctx, hipGetLastError());
    cxd_walk_args W;
    memset(&W, 0, sizeof(W));
    W.cols = n2; W.tiles = (n2 + 63) / 64;
    W.side = side; W.kind = out_kind; W.radius2 = radius2;
    // axis 1: the rows of a plane
    W.in = D->a.get(); W.out = D->b.get();
    W.n = n1; W.outer = n0; W.walk_stride = (size_t)n2; W.outer_stride = (size_t)(n1 * n2); W.w = w[1];
    W.items = (unsigned long long)W.outer * (unsigned long long)W.n * (unsigned long long)W.tiles;
    hipLaunchKernelGGL(cxd_k_walk<false>, dim3(cxd_grid(W.items)), dim3(256), 0, st, W);
    CX_HIP(ctx, hipGetLastError());
    // axis 0: the planes
    W.in = D->b.get(); W.out = final_out;
    W.n = n0; W.outer = n1; W.walk_stride = (size_t)(n1 * n2); W.outer_stride = (size_t)n2; W.w = w[0];
    W.items = (unsigned long long)W.outer * (unsigned long long)W.n * (unsigned long long)W.tiles;
    hipLaunchKernelGGL(cxd_k_walk<true>, dim3(cxd_grid(W.items)), dim3(256), 0, st, W);
    CX_HIP(ctx, hipGetLastError());
    unsigned long long nlow = 0;
    CX_HIP(ctx, hipMemcpyAsync(&nlow, D->nlow, sizeof(nlow), hipMemcpyDeviceToHost, st));
    if (out_host) CX_HIP(ctx, hipMemcpyAsync(out_host, final_out, out_bytes, hipMemcpyDeviceToHost, st));
    CX_HIP(ctx, hipStreamSynchronize(st));      // the count is the caller's, and its host memory is its own again
    const int64_t low = (int64_t)nlow, high = (int64_t)count - low;
    const int64_t sites = side == CX_DIST_BELOW ? high : side == CX_DIST_ABOVE ? low : (low < high ? low : high);
    if (!out_device) { D->publish(n0, n1, n2); D->kind = out_kind; D->n_sites = sites; }
    if (n_sites) *n_sites = sites;
    return CX_OK;
}

extern "C" int cx_grid_distance3d_result(cx_ctx* ctx, void** out_device, int64_t out_shape[3], int32_t* out_kind, int64_t* n_sites) {
    if (!ctx) return CX_ERR_INVALID;
    const cx_dist_state* D = ctx->dist;
    const int rc = cx_slot_result(ctx, D, "cx_grid_distance3d_result: no result of cx_grid_distance3d in the context", out_device, out_shape);
    if (rc) return rc;
    if (out_kind) *out_kind = D->kind;
    if (n_sites) *n_sites = D->n_sites;
    return CX_OK;
}

extern "C" int cx_grid_distance3d_bind(cx_ctx* ctx) {
    if (!ctx) return CX_ERR_INVALID;
    cx_dist_state* D = ctx->dist;
    if (D && D->pending) {
        if (D->kind == CX_DIST_OUT_SQUARED_F64) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_distance3d_bind: squared distances in double are not a grid the march reads");
        if (D->kind == CX_DIST_OUT_F32 && D->n_sites == 0) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_distance3d_bind: the result is infinite (a side without a site)");
    }
    return cx_slot_bind(ctx, D, "cx_grid_distance3d_bind: no result of cx_grid_distance3d in the context", D && D->kind == CX_DIST_OUT_F32 ? CX_DTYPE_F32 : CX_DTYPE_U8);
}
