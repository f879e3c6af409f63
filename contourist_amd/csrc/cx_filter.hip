// cx_filter.hip -- preparing the volume on the device (include/contourist_hip.h, section "preparing the volume"): a separable filter with
// a stride per axis over a 3-D sample array of any CX_DTYPE_*, fp32 out (cx_grid_filter3d), and the result as the bound grid
// (cx_grid_filter3d_bind).
//
// The arithmetic is fixed by the header: per axis a sum over the taps in double, k ascending from +0.0, rounded to fp32 once; the passes
// run axis 2, axis 1, axis 0 with fp32 between them.  A product of two fp32 numbers is exact in double, so fma(w, x, acc) and
// w * x + acc are the same double: contraction cannot change a bit.
//
// Lanes run along axis 2.  Two trips through memory:
//   cxf_k_rows<DT, BIG>  axes 2 and 1.  A wave owns 64 output columns of up to CXF_R consecutive output rows of one i-plane and walks the
//                    input rows those outputs need.  Per input row: the segment of the row under its 64 columns (with its halo, boundary
//                    rule applied, converted from the sample type) into the wave's own LDS, one axis-2 sum per lane, rounded to fp32 --
//                    that value is a sample of the axis-2 result and never reaches memory.
//   cxf_k_planes<BIG>  axis 0.  The same walk along i over the fp32 result of cxf_k_rows: every tap reads a whole coalesced row.
// The samples a wave's walk visits go into its window in LDS (CXF_WROWS rows of 64) and the sums then run tap by tap, one weight for
// all outputs; a wave takes as many outputs as keep its rows within the window.  More taps than the window has rows: every sample is
// added, as it arrives, to the sums it belongs to.  Ascending positions are ascending taps for every output in both.  An axis-2 segment
// is staged only where its taps overlap (stride < taps) and it fits CXF_SPAN words; otherwise the lanes read their taps from memory.
// Axis 0 not filtered: cxf_k_rows visits only the kept planes and writes the result itself (one trip).  Waves are independent: no
// workgroup barrier.  No atomics: every call gives the same bits.  DESIGN.md section 9m has the measurements.
#include <cmath>
#include <cstring>
#include <new>
#include <string>

#include "cx_dev.h"
#include "cx_gridop.h"

#define CXF_MAXW 129
#define CXF_R 16          // outputs along the walked axis per wave: (CXF_R - 1) stride + taps input rows for CXF_R output rows
#define CXF_SPAN 256u     // doubles of LDS per wave (four per lane): a row segment of 63 stride + taps samples is staged where it fits
#define CXF_WAVES 4u
#define CXF_WROWS 32u     // rows of the wave's window of walked samples (fp32, 64 lanes each): 8 KB per wave

struct cx_filter_state : cx_slot {      // (the result is fp32)
    cx_buf<float> mid;         // the result of cxf_k_rows where cxf_k_planes follows
};

void cx_filter_free(cx_ctx* ctx) {
    delete ctx->filt;
    ctx->filt = nullptr;
}

// one axis of one kernel
struct cxf_axis {
    int64_t n, m, stride;      // input length, output length = ceil(n / stride)
    int32_t nw, origin;        // nw = 0: not filtered (out[i] = in[i stride]); origin is 0 then
    float w[CXF_MAXW];
};
struct cxf_args {
    const void* in;
    float* out;
    int64_t planes, plane_step;   // cxf_k_rows: planes to visit, and the input plane of visited plane p = p * plane_step
    int64_t rows;                 // cxf_k_planes: rows of a plane (m1)
    int64_t chunks, tiles;        // chunks of CXF_R outputs along the walked axis, tiles of 64 columns
    unsigned long long items;     // waves' worth of work
    int32_t mode;
    float cval;
    int32_t rc, window;           // outputs of the walked axis per wave (<= CXF_R); 1: the samples the walk visits fit the window
    cxf_axis inner;               // axis 2 (cxf_k_rows only)
    cxf_axis walk;                // axis 1 (cxf_k_rows) or axis 0 (cxf_k_planes)
};

// the boundary rule: false = outside under CX_FILTER_CONSTANT, else s = the index read
__device__ __forceinline__ bool cxf_src(int64_t j, int64_t n, int32_t mode, int64_t& s) {
    s = j;
    if (j >= 0 && j < n) return true;
    if (mode == CX_FILTER_CONSTANT) { s = 0; return false; }
    if (mode == CX_FILTER_NEAREST) { s = j < 0 ? 0 : n - 1; return true; }
    int64_t p = j % (2 * n);
    if (p < 0) p += 2 * n;
    s = p < n ? p : 2 * n - 1 - p;
    return true;
}

template <int DT>
__device__ __forceinline__ float cxf_elem(const cx_grid_ref& row, int64_t c, int64_t n, int32_t mode, float cval) {
    int64_t s;
    return cxf_src(c, n, mode, s) ? cx_sample<DT>(row, (size_t)s) : cval;
}

// what the wave's own stores to its LDS words and its reads of them need between them: the LDS executes a wave's instructions in
// order, so only the compiler has to be kept from moving them past each other (no wait for the row loads in flight)
__device__ __forceinline__ void cxf_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- weights: fp32 in the kernel's arguments, held as doubles in registers (lane l: taps l, 64 + l, 128 + l) and read back by tap with
// v_readlane -- a tap's weight is the same for every lane, and a scalar load per tap put its latency in front of every multiply-add.
// BIG: more than 64 taps on an axis of the kernel (three registers instead of one)
template <bool BIG> struct cxf_wregs { double r0, r1, r2; };      // (r1, r2 unused without BIG)
__device__ __forceinline__ double cxf_weight_of_lane(const cxf_axis& X, int32_t t) { return t < X.nw ? (double)X.w[t] : 0.0; }
template <bool BIG>
__device__ __forceinline__ cxf_wregs<BIG> cxf_weights_load(const cxf_axis& X, uint32_t lane) {
    cxf_wregs<BIG> W;
    W.r0 = cxf_weight_of_lane(X, (int32_t)lane);
    W.r1 = BIG ? cxf_weight_of_lane(X, (int32_t)lane + 64) : 0.0;
    W.r2 = BIG ? cxf_weight_of_lane(X, (int32_t)lane + 128) : 0.0;
    return W;
}
__device__ __forceinline__ double cxf_lane_double(double v, uint32_t l) {
    const u64 b = (u64)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, (int)l), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), (int)l);
    return __longlong_as_double((long long)(((u64)hi << 32) | lo));
}
template <bool BIG>
__device__ __forceinline__ double cxf_weight(const cxf_wregs<BIG>& W, uint32_t t) {      // t: the same in every lane
    if constexpr (!BIG) return cxf_lane_double(W.r0, t);
    else {
        const uint32_t s = t >> 6;
        if (s == 0u) return cxf_lane_double(W.r0, t & 63u);
        if (s == 1u) return cxf_lane_double(W.r1, t & 63u);
        return cxf_lane_double(W.r2, t & 63u);
    }
}

// ---- the walk.  A wave produces outputs o0 .. o0 + rv - 1 (rv <= CXF_R) of the walked axis for its 64 columns.  It visits the input
// positions those outputs need in ascending order -- all of p0 .. p0 + (rv - 1) stride + taps - 1 where the taps of neighbouring
// outputs overlap (stride < taps), else the taps of one output after the other -- and adds each sample to the sums it belongs to:
// output r takes the sample `off` positions behind p0 as tap off - r stride.  Ascending positions are ascending taps for every output.
// Everything about a step is the same in every lane and small: 32-bit scalar arithmetic.
struct cxf_walk {
    int32_t nwe, stride32, rv;      // taps (1 for an axis that is not filtered), the stride where taps overlap, outputs
    bool overlap, filtered;
    uint32_t nq;                    // steps
    int64_t p0, stride;
    uint32_t q, rr, tt;             // the step; where taps do not overlap: the output it belongs to and its tap
    __device__ __forceinline__ void start(const cxf_axis& X, int64_t o0, int32_t rv_) {
        nwe = X.nw ? X.nw : 1; filtered = X.nw != 0; rv = rv_; stride = X.stride;
        overlap = X.stride < (int64_t)nwe;
        stride32 = overlap ? (int32_t)X.stride : 0;
        nq = overlap ? (uint32_t)((rv - 1) * stride32 + nwe) : (uint32_t)(rv * nwe);
        p0 = o0 * X.stride - X.origin;
        q = 0u; rr = 0u; tt = 0u;
    }
    __device__ __forceinline__ int64_t pos() const { return overlap ? p0 + (int64_t)q : p0 + (int64_t)rr * stride + (int64_t)tt; }
    // the position one step on (what is fetched while this step is summed)
    __device__ __forceinline__ int64_t pos_next() const {
        if (overlap) return p0 + (int64_t)q + 1;
        return tt + 1u == (uint32_t)nwe ? p0 + (int64_t)(rr + 1u) * stride : p0 + (int64_t)rr * stride + (int64_t)tt + 1;
    }
    __device__ __forceinline__ void step() {
        q++;
        if (++tt == (uint32_t)nwe) { tt = 0u; rr++; }
    }
    template <bool BIG>
    __device__ __forceinline__ void add(double (&acc)[CXF_R], const cxf_wregs<BIG>& W, float x) const {
        const double xd = (double)x;
#pragma unroll
        for (int r = 0; r < CXF_R; r++) {
            const int32_t t = overlap ? (int32_t)q - r * stride32 : ((uint32_t)r == rr ? (int32_t)tt : -1);
            if (r < rv && (uint32_t)t < (uint32_t)nwe) acc[r] = filtered ? fma(cxf_weight<BIG>(W, (uint32_t)t), xd, acc[r]) : xd;
        }
    }
};

// The window: where the samples one wave's walk visits number at most CXF_WROWS, they go into LDS first (step q into row q), and the
// sums then run tap by tap: one weight per tap for all CXF_R outputs, no question per output and step which tap it is.  Output r
// reads rows r sw .. r sw + taps - 1 (sw = the stride where taps overlap, else the taps), in ascending tap order as before.
template <bool BIG>
__device__ __forceinline__ void cxf_window_sums(double (&acc)[CXF_R], const cxf_walk& K, const cxf_wregs<BIG>& W, const float* __restrict__ win, uint32_t lane) {
    const uint32_t sw = K.overlap ? (uint32_t)K.stride32 : (uint32_t)K.nwe;
    for (uint32_t t = 0; t < (uint32_t)K.nwe; t++) {
        const double wv = K.filtered ? cxf_weight<BIG>(W, t) : 0.0;
        const float* __restrict__ col = win + t * 64u + lane;
#pragma unroll
        for (int r = 0; r < CXF_R; r++)
            if (r < K.rv) {
                const double v = (double)col[(uint32_t)r * sw * 64u];
                acc[r] = K.filtered ? fma(wv, v, acc[r]) : v;
            }
    }
}

// what a wave of cxf_k_rows has loaded of one input row and not converted yet: up to four samples of the staged segment per lane (or
// the finished axis-2 sum where the lanes read their taps from memory), bit i of `outside`: sample i is (float)cval
template <int DT>
struct cxf_rowregs {
    typename cx_dt<DT>::T raw[4];
    uint32_t outside;
    float x;
    uint32_t row_outside;      // (a word: no padding bytes for the copies to carry)
};
template <int DT>
__device__ __forceinline__ float cxf_cvt(typename cx_dt<DT>::T v) {
    if constexpr (DT == CX_DTYPE_F32) return v;
    else return cx_dt<DT>::cvt((uint32_t)(typename cx_dt<DT>::bits)v);
}

template <int DT, bool BIG>
__global__ __launch_bounds__(256) void cxf_k_rows(const cxf_args A) {
    __shared__ __attribute__((aligned(16))) double lds_all[CXF_WAVES * CXF_SPAN];
    __shared__ __attribute__((aligned(16))) float win_all[CXF_WAVES * CXF_WROWS * 64u];
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    double* __restrict__ lds = lds_all + wave * CXF_SPAN;
    float* __restrict__ win = win_all + wave * (CXF_WROWS * 64u);
    const cxf_axis& I = A.inner;
    const int32_t nwe2 = I.nw ? I.nw : 1;
    const cxf_wregs<BIG> W2 = cxf_weights_load<BIG>(I, lane), W1 = cxf_weights_load<BIG>(A.walk, lane);
    typedef typename cx_dt<DT>::T T;
    for (unsigned long long it = (unsigned long long)blockIdx.x * CXF_WAVES + wave; it < A.items; it += (unsigned long long)gridDim.x * CXF_WAVES) {
        const int64_t tile = (int64_t)(it % (unsigned long long)A.tiles), rest = (int64_t)(it / (unsigned long long)A.tiles);
        const int64_t chunk = rest % A.chunks, plane = rest / A.chunks;
        const int64_t k0 = tile * 64, o0 = chunk * A.rc;
        const int rv = (int)(A.walk.m - o0 < A.rc ? A.walk.m - o0 : A.rc);
        const int ncols = (int)(I.m - k0 < 64 ? I.m - k0 : 64);
        const bool active = (int)lane < ncols;
        const int64_t c0 = k0 * I.stride - I.origin;                                      // position of the first tap of the first column
        const int64_t span = (int64_t)(ncols - 1) * I.stride + nwe2;
        const bool staged = I.stride < (int64_t)nwe2 && span <= (int64_t)CXF_SPAN;
        const size_t plane_base = (size_t)(plane * A.plane_step) * (size_t)A.walk.n;      // in rows
        double acc[CXF_R];
#pragma unroll
        for (int r = 0; r < CXF_R; r++) acc[r] = 0.0;
        // row `pos` of the plane (boundary rule of axis 1): its loads
        // Every load is unconditional, from an index inside the array, and what it stands for (cval, nothing) is decided when the row
        // is summed: a load whose register is also written on another path waits for every load before it.
        auto fetch = [&](int64_t pos) -> cxf_rowregs<DT> {
            cxf_rowregs<DT> G;
            G.outside = 0u; G.x = 0.0f;
            int64_t srow;
            G.row_outside = cxf_src(pos, A.walk.n, A.mode, srow) ? 0u : 1u;      // (srow = 0 then)
            const T* __restrict__ row = static_cast<const T*>(A.in) + (plane_base + (size_t)srow) * (size_t)I.n;
            if (staged) {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    int64_t q = (int64_t)lane + 64 * i, sc;
                    if (q > span - 1) q = span - 1;
                    if (!cxf_src(c0 + q, I.n, A.mode, sc)) G.outside |= 1u << i;
                    G.raw[i] = row[sc];
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) G.raw[i] = (T)0;
                if (active && !G.row_outside) {
                    const cx_grid_ref ref = {row, DT};
                    const int64_t c = c0 + (int64_t)lane * I.stride;
                    if (I.nw) {
                        double a = 0.0;
                        for (int32_t t = 0; t < I.nw; t++) a = fma(cxf_weight<BIG>(W2, (uint32_t)t), (double)cxf_elem<DT>(ref, c + t, I.n, A.mode, A.cval), a);
                        G.x = (float)a;
                    } else G.x = cx_sample<DT>(ref, (size_t)c);      // (inside the row: c = column * stride)
                }
            }
            return G;
        };
        // ... and its sample of the axis-2 result for every column of the wave
        auto finish = [&](const cxf_rowregs<DT>& G) -> float {
            if (G.row_outside) return A.cval;
            if (!staged) return G.x;
            cxf_wave_sync();      // the row before this one has been read
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int64_t q = (int64_t)lane + 64 * i;
                if (q < span) lds[q] = (double)(((G.outside >> i) & 1u) ? A.cval : cxf_cvt<DT>(G.raw[i]));
            }
            cxf_wave_sync();
            float x = 0.0f;
            if (active) {
                const double* __restrict__ mine = lds + (size_t)lane * (size_t)I.stride;
                double a = 0.0;
                for (int32_t t = 0; t < I.nw; t++) a = fma(cxf_weight<BIG>(W2, (uint32_t)t), mine[t], a);
                x = (float)a;
            }
            return x;
        };
        cxf_walk K;
        K.start(A.walk, o0, rv);
        cxf_rowregs<DT> cur = fetch(K.pos());
        while (K.q < K.nq) {
            const cxf_rowregs<DT> nxt = fetch(K.q + 1u < K.nq ? K.pos_next() : K.pos());      // in flight while this row is summed (the last row: once more)
            const float x = finish(cur);
            if (A.window) win[K.q * 64u + lane] = x;
            else K.add<BIG>(acc, W1, x);
            cur = nxt;
            K.step();
        }
        if (A.window) {
            cxf_wave_sync();
            cxf_window_sums<BIG>(acc, K, W1, win, lane);
            cxf_wave_sync();      // (before the next item's rows)
        }
        if (active) {
            float* __restrict__ out = A.out + ((size_t)plane * (size_t)A.walk.m + (size_t)o0) * (size_t)I.m + (size_t)k0 + lane;
#pragma unroll
            for (int r = 0; r < CXF_R; r++)
                if (r < rv) out[(size_t)r * (size_t)I.m] = (float)acc[r];
        }
    }
}

// axis 0 over fp32 [n0][rows][cols]: A.inner carries only the row length (n = m = cols)
template <bool BIG>
__global__ __launch_bounds__(256) void cxf_k_planes(const cxf_args A) {
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    const float* __restrict__ in = static_cast<const float*>(A.in);
    const size_t cols = (size_t)A.inner.m, rows = (size_t)A.rows;
    const cxf_wregs<BIG> W0 = cxf_weights_load<BIG>(A.walk, lane);
    __shared__ __attribute__((aligned(16))) float win_all[CXF_WAVES * CXF_WROWS * 64u];
    float* __restrict__ win = win_all + wave * (CXF_WROWS * 64u);
    for (unsigned long long it = (unsigned long long)blockIdx.x * CXF_WAVES + wave; it < A.items; it += (unsigned long long)gridDim.x * CXF_WAVES) {
        const int64_t tile = (int64_t)(it % (unsigned long long)A.tiles), rest = (int64_t)(it / (unsigned long long)A.tiles);
        const int64_t j = rest % A.rows, chunk = rest / A.rows;
        const int64_t o0 = chunk * A.rc;
        const int rv = (int)(A.walk.m - o0 < A.rc ? A.walk.m - o0 : A.rc);
        const size_t k = (size_t)tile * 64u + lane;
        const bool active = k < cols;
        double acc[CXF_R];
#pragma unroll
        for (int r = 0; r < CXF_R; r++) acc[r] = 0.0;
        // (unconditional loads from inside the array; cval takes their place afterwards: see cxf_k_rows)
        const size_t kc = active ? k : cols - 1u;
        auto fetch = [&](int64_t pos, bool& outside) -> float {
            int64_t sp;
            outside = !cxf_src(pos, A.walk.n, A.mode, sp);
            return in[((size_t)sp * rows + (size_t)j) * cols + kc];
        };
        cxf_walk K;
        K.start(A.walk, o0, rv);
        if (A.window) {
            while (K.q < K.nq) {      // eight loads in flight, then their stores
                float x[8];
                uint32_t outside = 0u;
                cxf_walk L = K;
                const uint32_t left = K.nq - K.q;
#pragma unroll
                for (uint32_t b = 0; b < 8u; b++) {      // (behind the last step: its load once more)
                    bool o;
                    x[b] = fetch(L.pos(), o);
                    if (o) outside |= 1u << b;
                    if (b + 1u < left) L.step();
                }
#pragma unroll
                for (uint32_t b = 0; b < 8u; b++)
                    if (b < left) { win[K.q * 64u + lane] = ((outside >> b) & 1u) ? A.cval : x[b]; K.step(); }
            }
            cxf_wave_sync();
            cxf_window_sums<BIG>(acc, K, W0, win, lane);
            cxf_wave_sync();      // (before the next item's rows)
        } else {
            bool cur_o, nxt_o;
            float cur = fetch(K.pos(), cur_o);
            while (K.q < K.nq) {
                const float nxt = fetch(K.q + 1u < K.nq ? K.pos_next() : K.pos(), nxt_o);
                K.add<BIG>(acc, W0, cur_o ? A.cval : cur);
                cur = nxt; cur_o = nxt_o;
                K.step();
            }
        }
        if (active) {
            float* __restrict__ out = A.out + ((size_t)o0 * rows + (size_t)j) * cols + k;
#pragma unroll
            for (int r = 0; r < CXF_R; r++)
                if (r < rv) out[(size_t)r * rows * cols] = (float)acc[r];
        }
    }
}

static void cxf_axis_fill(cxf_axis& X, const cx_filter_axis& a, int64_t n) {
    memset(&X, 0, sizeof(X));
    const bool filtered = a.weights && a.n_weights > 0;
    X.n = n; X.stride = a.stride; X.m = (n + a.stride - 1) / a.stride;
    X.nw = filtered ? a.n_weights : 0;
    X.origin = filtered ? a.origin : 0;
    if (filtered) memcpy(X.w, a.weights, (size_t)a.n_weights * sizeof(float));
}

// outputs of the walked axis per wave: as many (up to CXF_R) as keep the samples their walk visits inside the window; a kernel of more
// taps than the window has rows takes the walk without it
static void cxf_chunking(cxf_args& A) {
    const int64_t nwe = A.walk.nw ? A.walk.nw : 1;
    A.rc = CXF_R; A.window = 0;
    if (nwe > (int64_t)CXF_WROWS) return;
    const int64_t fit = A.walk.stride < nwe ? ((int64_t)CXF_WROWS - nwe) / A.walk.stride + 1 : (int64_t)CXF_WROWS / nwe;
    A.rc = (int32_t)(fit < CXF_R ? fit : CXF_R); A.window = 1;
}

static uint32_t cxf_grid(unsigned long long items) {
    const unsigned long long blocks = (items + CXF_WAVES - 1u) / CXF_WAVES;
    return (uint32_t)(blocks < (1ull << 22) ? (blocks ? blocks : 1ull) : (1ull << 22));
}

extern "C" int cx_grid_filter3d(cx_ctx* ctx, const void* samples, int32_t dtype, int on_device, int64_t n0, int64_t n1, int64_t n2,
                                const cx_filter_axis axes[3], int32_t mode, double cval, void* out_device, float* out_host, int64_t out_shape[3]) {
    if (!ctx) return CX_ERR_INVALID;
    if (!axes) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_filter3d: no axes");
    if (mode != CX_FILTER_NEAREST && mode != CX_FILTER_REFLECT && mode != CX_FILTER_CONSTANT) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_filter3d: unknown mode");
    if (!std::isfinite(cval)) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_filter3d: cval is NaN or infinite");
    cx_source S;
    int rc = cx_source_resolve(ctx, "cx_grid_filter3d", samples, dtype, on_device, n0, n1, n2, 31, &S);
    if (rc) return rc;
    n0 = S.n[0]; n1 = S.n[1]; n2 = S.n[2];
    for (int a = 0; a < 3; a++) {
        if (axes[a].stride < 1 || (int64_t)axes[a].stride > S.n[a]) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_filter3d: a stride outside 1..n");
        if (axes[a].weights && axes[a].n_weights != 0) {
            if (axes[a].n_weights < 1 || axes[a].n_weights > CXF_MAXW) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_filter3d: 1..129 weights per axis");
            if (axes[a].origin < 0 || axes[a].origin >= axes[a].n_weights) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_filter3d: an origin outside 0..n_weights-1");
        }
    }
    cxf_args R, P;      // the two kernels
    memset(&R, 0, sizeof(R)); memset(&P, 0, sizeof(P));
    cxf_axis_fill(R.inner, axes[2], n2);
    cxf_axis_fill(R.walk, axes[1], n1);
    cxf_axis_fill(P.walk, axes[0], n0);
    const int64_t m0 = P.walk.m, m1 = R.walk.m, m2 = R.inner.m;
    const bool two = P.walk.nw != 0;      // axis 0 filtered: cxf_k_planes follows; else cxf_k_rows visits the kept planes only
    const size_t out_count = (size_t)(m0 * m1 * m2);
    if (out_device && S.on_device && cx_overlap(S.p, S.bytes, out_device, out_count * sizeof(float)))
        return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_filter3d: the output overlaps the input");
    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_filter_state* F = cx_state_of(ctx->filt);
    if (!F) return CX_ERR_NOMEM;
    hipStream_t st = ctx->stream;
    const void* dev;
    void* out;
    if ((rc = F->stage(ctx, S, &dev)) || (rc = F->open(ctx, out_device, out_count * sizeof(float), &out))) return rc;
    float* final_out = static_cast<float*>(out);
    if (two && (rc = F->mid.grow(ctx, (size_t)(n0 * m1 * m2)))) return rc;
    R.in = dev; R.out = two ? F->mid.get() : final_out;
    R.planes = two ? n0 : m0; R.plane_step = two ? 1 : P.walk.stride;
    cxf_chunking(R);
    R.chunks = (m1 + R.rc - 1) / R.rc; R.tiles = (m2 + 63) / 64;
    R.items = (unsigned long long)R.planes * (unsigned long long)R.chunks * (unsigned long long)R.tiles;
    R.mode = mode; R.cval = (float)cval;
    const bool big = R.inner.nw > 64 || R.walk.nw > 64 || P.walk.nw > 64;      // more than 64 taps on an axis: three weight registers per axis
#define CX_LAUNCH(DT)                                                                                          \
    if (big) hipLaunchKernelGGL((cxf_k_rows<DT, true>), dim3(cxf_grid(R.items)), dim3(256), 0, st, R);         \
    else hipLaunchKernelGGL((cxf_k_rows<DT, false>), dim3(cxf_grid(R.items)), dim3(256), 0, st, R);
    CX_DISPATCH_DTYPE(S.dtype, CX_LAUNCH)
#undef CX_LAUNCH
    CX_HIP(ctx, hipGetLastError());
    if (two) {
        P.in = F->mid.get(); P.out = final_out;
        P.inner.n = P.inner.m = m2; P.inner.stride = 1;
        P.rows = m1;
        cxf_chunking(P);
        P.chunks = (m0 + P.rc - 1) / P.rc; P.tiles = R.tiles;
        P.items = (unsigned long long)P.chunks * (unsigned long long)m1 * (unsigned long long)P.tiles;
        P.mode = mode; P.cval = (float)cval;
        if (big) hipLaunchKernelGGL(cxf_k_planes<true>, dim3(cxf_grid(P.items)), dim3(256), 0, st, P);
        else hipLaunchKernelGGL(cxf_k_planes<false>, dim3(cxf_grid(P.items)), dim3(256), 0, st, P);
        CX_HIP(ctx, hipGetLastError());
    }
    if (!out_device) F->publish(m0, m1, m2);
    if (out_shape) { out_shape[0] = m0; out_shape[1] = m1; out_shape[2] = m2; }
    if (out_host) CX_HIP(ctx, hipMemcpyAsync(out_host, final_out, out_count * sizeof(float), hipMemcpyDeviceToHost, st));
    if (out_host || !S.on_device) CX_HIP(ctx, hipStreamSynchronize(st));      // the caller's host memory is its own again
    return CX_OK;
}

extern "C" int cx_grid_filter3d_result(cx_ctx* ctx, void** out_device, int64_t out_shape[3]) {
    if (!ctx) return CX_ERR_INVALID;
    return cx_slot_result(ctx, ctx->filt, "cx_grid_filter3d_result: no result of cx_grid_filter3d in the context", out_device, out_shape);
}

extern "C" int cx_grid_filter3d_bind(cx_ctx* ctx) {
    if (!ctx) return CX_ERR_INVALID;
    return cx_slot_bind(ctx, ctx->filt, "cx_grid_filter3d_bind: no result of cx_grid_filter3d in the context", CX_DTYPE_F32);
}
