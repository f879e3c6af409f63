// cx_pick.hip -- choosing isovalues on the device (include/contourist_hip.h, section "choosing isovalues"): exact order statistics of a
// sample array (cx_samples_select) and the size of the isosurface at every one of many candidate values (cx_level_spectrum3d).
//
// Select: a most-significant-digit radix select on order-preserving keys.  A key has the width of the sample type (8, 16 or 32 bits) and
// sorts as numpy sorts the fp32 values: -inf < finite < +inf < NaN, -0.0 folded onto +0.0.  Digits: 8 | 8+8 | 12+10+10 bits (the first
// pass has one histogram and can afford the widest digit; 12 prefixes of 10 bits then share a pass, so 9 deciles take three passes).
//   cxk_k_hist<DT>      one pass over the samples: per prefix of the round (the key bits above the digit, up to CXK_ROUND of them) a
//                       histogram of the digit, privatised in LDS, flushed once per workgroup with 64-bit adds of its non-zero bins.
//                       16-byte loads in a grid-stride loop, head and tail for any alignment; a wave whose lanes agree adds once.
// The host walks the cumulative counts (64-bit integers) and hands the next pass the prefixes its ranks fell under.
//
// Spectrum: with the levels' thresholds sorted, c(f) = the number of thresholds <= f says everything about a sample: level s (in sorted
// order) sees it low iff s >= c(f).  An edge, a cell and a tetrahedron then add +-1 at a few indices of a difference array each, and the
// counts per level are prefix sums.
//   cxk_k_spectrum<DT>  persistent workgroups walk tiles of 4 x 8 x 64 lattice points: c of the tile and its +1 halo into LDS (16-bit),
//                       then one lane per lattice point: its 7 forward edges, its cell and the cell's 6 Kuhn tetrahedra where not all the
//                       c agree.  Difference arrays private in LDS, non-zero entries flushed with 64-bit integer adds at the end.
//                       One bisection per sample, into the merged keys of the thresholds and the bounds of the levels' tolerance
//                       screens, gives c and says whether a screen holds the sample: those are counted per bucket in global memory
//                       (they are rare).
// Integer atomics only: every count is the same in every call.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "cx_dev.h"
#include "cx_gridop.h"

#define CXK_ROUND 12u           // prefixes per refinement pass: 12 histograms of 1024 bins are 48 KB of LDS
#define CXK_HIST 12288u         // histogram words of one pass (the first fp32 pass has 4096 bins and no prefix)
#define CXK_MAX_RANKS 1024
#define CXK_MAX_LEVELS 4096
#define CXK_TI 4u
#define CXK_TJ 8u
#define CXK_TK 64u
#define CXK_HALO ((CXK_TI + 1u) * (CXK_TJ + 1u) * (CXK_TK + 1u))
#define CXK_TAB_LDS_MAX 1536u   // levels up to which the merged key table sits in LDS beside the difference arrays (53 KB there)

struct cx_pick_state {
    cx_buf<uint8_t> samples;              // host samples of cx_samples_select
    cx_buf<unsigned long long> hist;      // [prefix of the pass][bins] digit counts (CXK_HIST words), then the NaN count
    cx_buf<unsigned long long> acc;       // spectrum: three difference arrays of K + 1, then 3 K + 1 buckets of the merged keys
    cx_buf<uint32_t> keys;                // spectrum: the merged keys of thresholds and screen bounds (3 K), then the live bits of the buckets
    cx_buf<uint16_t> cof;                 // spectrum: thresholds among the first p merged keys (3 K + 1)
    std::vector<unsigned long long> host; // what comes back
};

void cx_pick_free(cx_ctx* ctx) {
    delete ctx->pick;
    ctx->pick = nullptr;
}

static cx_pick_state* cxk_state(cx_ctx* ctx) {
    if (!ctx->pick) ctx->pick = new (std::nothrow) cx_pick_state();
    return ctx->pick;
}

// ---- keys ---------------------------------------------------------------------------------------------------------------------------
// fp32: sign flip for non-negative values, full inversion for negative ones, NaN of either sign on top, -0.0 as +0.0
__host__ __device__ __forceinline__ uint32_t cxk_key_f32(uint32_t u) {
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
static inline uint32_t cxk_unkey_f32(uint32_t k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }   // (not of the NaN key)
// the same in 16 bits; `inf` = the bits of +infinity (0x7C00 half, 0x7F80 bfloat16)
__device__ __forceinline__ uint32_t cxk_key_f16(uint32_t u, uint32_t inf) {
    if ((u & 0x7FFFu) > inf) return 0xFFFFu;
    if (u == 0x8000u) u = 0u;
    return (u & 0x8000u) ? (~u & 0xFFFFu) : (u | 0x8000u);
}
template <int DT> struct cxk_keys;
template <> struct cxk_keys<CX_DTYPE_F32> { enum { BITS = 32, ISFLOAT = 1 }; static __device__ __forceinline__ uint32_t key(uint32_t v) { return cxk_key_f32(v); } };
template <> struct cxk_keys<CX_DTYPE_U8> { enum { BITS = 8, ISFLOAT = 0 }; static __device__ __forceinline__ uint32_t key(uint32_t v) { return v; } };
template <> struct cxk_keys<CX_DTYPE_I8> { enum { BITS = 8, ISFLOAT = 0 }; static __device__ __forceinline__ uint32_t key(uint32_t v) { return v ^ 0x80u; } };
template <> struct cxk_keys<CX_DTYPE_U16> { enum { BITS = 16, ISFLOAT = 0 }; static __device__ __forceinline__ uint32_t key(uint32_t v) { return v; } };
template <> struct cxk_keys<CX_DTYPE_I16> { enum { BITS = 16, ISFLOAT = 0 }; static __device__ __forceinline__ uint32_t key(uint32_t v) { return v ^ 0x8000u; } };
template <> struct cxk_keys<CX_DTYPE_F16> { enum { BITS = 16, ISFLOAT = 1 }; static __device__ __forceinline__ uint32_t key(uint32_t v) { return cxk_key_f16(v, 0x7C00u); } };
template <> struct cxk_keys<CX_DTYPE_BF16> { enum { BITS = 16, ISFLOAT = 1 }; static __device__ __forceinline__ uint32_t key(uint32_t v) { return cxk_key_f16(v, 0x7F80u); } };

// the sample a key stands for, as the fp32 value every type converts to exactly
static double cxk_value_of_key(int32_t dt, uint32_t k) {
    switch (dt) {
        case CX_DTYPE_U8: case CX_DTYPE_U16: return (double)k;
        case CX_DTYPE_I8: return (double)(int8_t)(uint8_t)(k ^ 0x80u);
        case CX_DTYPE_I16: return (double)(int16_t)(uint16_t)(k ^ 0x8000u);
        case CX_DTYPE_F16: {
            if (k == 0xFFFFu) return (double)NAN;
            const uint32_t h = (k & 0x8000u) ? (k ^ 0x8000u) : (~k & 0xFFFFu);
            const int e = (int)((h >> 10) & 31u);
            const double m = (double)(h & 1023u);
            const double a = e == 31 ? (double)INFINITY : (e ? std::ldexp(1024.0 + m, e - 25) : std::ldexp(m, -24));
            return (h & 0x8000u) ? -a : a;
        }
        case CX_DTYPE_BF16: {
            if (k == 0xFFFFu) return (double)NAN;
            const uint32_t u = ((k & 0x8000u) ? (k ^ 0x8000u) : (~k & 0xFFFFu)) << 16;
            float f; memcpy(&f, &u, 4);
            return (double)f;
        }
        default: {
            if (k == 0xFFFFFFFFu) return (double)NAN;
            const uint32_t u = cxk_unkey_f32(k);
            float f; memcpy(&f, &u, 4);
            return (double)f;
        }
    }
}

// ---- select: the histogram pass -----------------------------------------------------------------------------------------------------
struct cxk_pass {
    uint32_t nprefix;              // histograms of this launch (1..CXK_ROUND)
    uint32_t pshift;               // key >> pshift is the prefix (32: there is none, every sample counts)
    uint32_t dshift, dmask;        // digit = (key >> dshift) & dmask
    uint32_t bins;                 // dmask + 1
    uint32_t count_nan;            // first pass of a float type: count the NaN keys too
    uint32_t prefix[CXK_ROUND];
};

// the bits of a loaded sample, zero-extended
template <typename B> __device__ __forceinline__ uint32_t cxk_raw(B v) {
    if constexpr (std::is_same<B, float>::value) return __float_as_uint(v);
    else return (uint32_t)v;
}

// One sample of every lane (ok: the lane has one).  Lanes that agree with the first add once for all of them.
__device__ __forceinline__ void cxk_count(uint32_t* __restrict__ h, const cxk_pass& P, uint32_t key, bool ok) {
    uint32_t slot = 0xFFFFFFFFu;
    if (ok) {
        const uint32_t digit = (key >> P.dshift) & P.dmask;
        if (P.pshift >= 32u) slot = digit;
        else {
            const uint32_t pre = key >> P.pshift;
#pragma unroll
            for (uint32_t r = 0; r < CXK_ROUND; r++)
                if (r < P.nprefix && pre == P.prefix[r]) slot = r * P.bins + digit;
        }
    }
    const u64 live = __ballot(slot != 0xFFFFFFFFu);
    if (!live) return;
    const int first = __ffsll((unsigned long long)live) - 1;
    const uint32_t lead = (uint32_t)__shfl((int)slot, first);
    const u64 same = __ballot(slot == lead);
    const uint32_t lane = threadIdx.x & 63u;
    if (lane == (uint32_t)first) atomicAdd(&h[lead], (uint32_t)__popcll(same));
    else if (slot != 0xFFFFFFFFu && slot != lead) atomicAdd(&h[slot], 1u);
}

template <int DT>
__global__ __launch_bounds__(256) void cxk_k_hist(const void* __restrict__ samples, unsigned long long n, cxk_pass P, unsigned long long* __restrict__ out) {
    typedef typename cx_dt<DT>::bits B;
    typedef cxk_keys<DT> K;
    constexpr uint32_t PER = 16u / (uint32_t)sizeof(B);
    extern __shared__ __attribute__((aligned(16))) uint32_t cxk_lds[];
    const uint32_t nslots = P.nprefix * P.bins;      // (+ one word behind them: the workgroup's NaN count)
    for (uint32_t s = threadIdx.x; s <= nslots; s += 256u) cxk_lds[s] = 0u;
    __syncthreads();
    const B* __restrict__ src = static_cast<const B*>(samples);
    // head: the samples in front of the first 16-byte boundary; body: whole 16-byte vectors; tail: what is left
    const unsigned long long addr = (unsigned long long)(uintptr_t)samples;
    unsigned long long head = (((16ull - (addr & 15ull)) & 15ull)) / sizeof(B);
    if (head > n) head = n;
    const unsigned long long nvec = (n - head) / PER, tail0 = head + nvec * PER;
    uint32_t nans = 0u;
    if (blockIdx.x == 0u && threadIdx.x < 64u) {      // the first wave: lanes 0..31 the head, 32..63 the tail (at most 15 samples each)
        const unsigned long long e = threadIdx.x < 32u ? (unsigned long long)threadIdx.x : tail0 + (threadIdx.x - 32u);
        const bool ok = threadIdx.x < 32u ? e < head : e < n;
        const uint32_t key = ok ? K::key(cxk_raw<B>(src[e])) : 0u;
        cxk_count(cxk_lds, P, key, ok);
        if (K::ISFLOAT && ok && key == (K::BITS == 32 ? 0xFFFFFFFFu : 0xFFFFu)) nans++;
    }
    const uint4* __restrict__ vec = reinterpret_cast<const uint4*>(src + head);
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long base = (unsigned long long)blockIdx.x * 256ull; base < nvec; base += stride) {      // (uniform per workgroup)
        const unsigned long long v = base + threadIdx.x;
        const bool ok = v < nvec;
        uint4 q = make_uint4(0u, 0u, 0u, 0u);
        if (ok) q = vec[v];
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (uint32_t e = 0; e < PER; e++) {
            const uint32_t raw = sizeof(B) == 4 ? w[e] : (sizeof(B) == 2 ? (w[e >> 1] >> (16u * (e & 1u))) & 0xFFFFu : (w[e >> 2] >> (8u * (e & 3u))) & 0xFFu);
            const uint32_t key = K::key(raw);
            cxk_count(cxk_lds, P, key, ok);
            if (K::ISFLOAT && ok && key == (K::BITS == 32 ? 0xFFFFFFFFu : 0xFFFFu)) nans++;
        }
    }
    if (K::ISFLOAT && P.count_nan && nans) atomicAdd(&cxk_lds[nslots], nans);
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < nslots; s += 256u) {
        const uint32_t c = cxk_lds[s];
        if (c) atomicAdd(&out[s], (unsigned long long)c);
    }
    if (threadIdx.x == 0u && cxk_lds[nslots]) atomicAdd(&out[CXK_HIST], (unsigned long long)cxk_lds[nslots]);
}

static int cxk_invalid(cx_ctx* ctx, const char* msg) {
    ctx->err = msg;
    return CX_ERR_INVALID;
}

// one launch: the histograms of `P` into Z->host[0 .. nprefix * bins) (and the NaN count behind them)
static int cxk_run_pass(cx_ctx* ctx, cx_pick_state* Z, const void* dev, int32_t dt, unsigned long long n, const cxk_pass& P) {
    hipStream_t st = ctx->stream;
    const size_t words = (size_t)CXK_HIST + 1u;
    CX_HIP(ctx, hipMemsetAsync(Z->hist, 0, words * sizeof(unsigned long long), st));
    const unsigned long long per = 16u / cx_dtype_size(dt);
    const unsigned long long nvec = n / per + 1ull;
    const uint32_t grid = (uint32_t)std::min<unsigned long long>(1024ull, (nvec + 255ull) / 256ull);
    const size_t lds = ((size_t)P.nprefix * P.bins + 1u) * sizeof(uint32_t);
#define CX_LAUNCH(DT) hipLaunchKernelGGL((cxk_k_hist<DT>), dim3(grid), dim3(256), lds, st, dev, n, P, Z->hist.get());
    CX_DISPATCH_DTYPE(dt, CX_LAUNCH)
#undef CX_LAUNCH
    CX_HIP(ctx, hipGetLastError());
    Z->host.resize(words);
    CX_HIP(ctx, hipMemcpyAsync(Z->host.data(), Z->hist, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    CX_HIP(ctx, hipStreamSynchronize(st));
    return CX_OK;
}

extern "C" int cx_samples_select(cx_ctx* ctx, const void* samples, int32_t dtype, int on_device, int64_t n, const int64_t* ranks, int32_t nranks,
                                 double* out_values, int64_t* out_n_nan) {
    if (!ctx) return CX_ERR_INVALID;
    if (!ranks || nranks < 1 || nranks > CXK_MAX_RANKS) return cxk_invalid(ctx, "cx_samples_select: 1..1024 ranks");
    if (!samples) {
        if (!ctx->grid.p) return cx_no_grid(ctx, "cx_samples_select");
        dtype = ctx->grid.dtype; n = ctx->n0 * ctx->n1 * ctx->n2; on_device = 1;
    } else {
        if (!cx_dtype_valid(dtype)) return cxk_invalid(ctx, "cx_samples_select: unknown sample type");
        if (n < 1 || n > (1LL << 31)) return cxk_invalid(ctx, "cx_samples_select: 1..2^31 samples");
    }
    for (int32_t k = 0; k < nranks; k++)
        if (ranks[k] < 0 || ranks[k] >= n) return cxk_invalid(ctx, "cx_samples_select: a rank outside 0..n-1");
    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_pick_state* Z = cxk_state(ctx);
    if (!Z) return CX_ERR_NOMEM;
    int rc;
    if ((rc = Z->hist.grow(ctx, (size_t)CXK_HIST + 1u))) return rc;
    const void* dev = samples ? samples : ctx->grid.p;
    if (samples && !on_device) {
        const size_t bytes = (size_t)n * cx_dtype_size(dtype);
        if ((rc = Z->samples.grow(ctx, bytes))) return rc;
        CX_HIP(ctx, hipMemcpyAsync(Z->samples, samples, bytes, hipMemcpyHostToDevice, ctx->stream));
        dev = Z->samples.get();
    }
    // the digits of a key, most significant first
    const uint32_t width = (uint32_t)cx_dtype_size(dtype) * 8u;
    uint32_t digits[3], ndigits;
    if (width == 8u) { digits[0] = 8u; ndigits = 1u; }
    else if (width == 16u) { digits[0] = 8u; digits[1] = 8u; ndigits = 2u; }
    else { digits[0] = 12u; digits[1] = 10u; digits[2] = 10u; ndigits = 3u; }
    // a group: the distinct ranks that share the key bits found so far, and the samples whose keys sort before that prefix
    struct group { uint32_t prefix; unsigned long long below; std::vector<unsigned long long> ranks; };
    std::vector<unsigned long long> want(ranks, ranks + nranks);
    std::sort(want.begin(), want.end());
    want.erase(std::unique(want.begin(), want.end()), want.end());
    std::vector<group> groups(1), next;
    groups[0].prefix = 0u; groups[0].below = 0ull; groups[0].ranks = want;
    unsigned long long n_nan = 0ull;
    uint32_t left = width;
    for (uint32_t d = 0; d < ndigits; d++) {
        left -= digits[d];
        next.clear();
        for (size_t g0 = 0; g0 < groups.size(); g0 += CXK_ROUND) {
            cxk_pass P;
            memset(&P, 0, sizeof(P));
            P.nprefix = (uint32_t)std::min<size_t>(CXK_ROUND, groups.size() - g0);
            P.pshift = d == 0u ? 32u : left + digits[d];
            P.dshift = left; P.bins = 1u << digits[d]; P.dmask = P.bins - 1u;
            P.count_nan = d == 0u ? 1u : 0u;
            for (uint32_t r = 0; r < P.nprefix; r++) P.prefix[r] = groups[g0 + r].prefix;
            if ((rc = cxk_run_pass(ctx, Z, dev, dtype, (unsigned long long)n, P))) return rc;
            if (d == 0u) n_nan = Z->host[(size_t)CXK_HIST];
            for (uint32_t r = 0; r < P.nprefix; r++) {
                const group& G = groups[g0 + r];
                const unsigned long long* H = Z->host.data() + (size_t)r * P.bins;
                unsigned long long cum = G.below;      // samples before bin b
                uint32_t b = 0;
                for (size_t q = 0; q < G.ranks.size(); q++) {      // (ascending)
                    while (b < P.bins && cum + H[b] <= G.ranks[q]) cum += H[b++];
                    if (b >= P.bins) { ctx->err = "cx_samples_select: the counts do not add up"; return CX_ERR_HIP; }
                    const uint32_t pre = (G.prefix << digits[d]) | b;
                    if (next.empty() || next.back().prefix != pre || next.back().below != cum) {
                        next.emplace_back();
                        next.back().prefix = pre; next.back().below = cum;
                    }
                    next.back().ranks.push_back(G.ranks[q]);
                }
            }
        }
        groups.swap(next);
    }
    // every group is one key now
    for (int32_t k = 0; k < nranks; k++) {
        const unsigned long long r = (unsigned long long)ranks[k];
        double v = 0.0;
        bool found = false;
        for (const group& G : groups)
            if (std::binary_search(G.ranks.begin(), G.ranks.end(), r)) { v = cxk_value_of_key(dtype, G.prefix); found = true; break; }
        if (!found) { ctx->err = "cx_samples_select: a rank was lost"; return CX_ERR_HIP; }
        if (out_values) out_values[k] = v;
    }
    if (out_n_nan) *out_n_nan = (int64_t)n_nan;
    return CX_OK;
}

// ---- spectrum -----------------------------------------------------------------------------------------------------------------------
struct cxk_spec {
    cx_grid_ref grid;
    uint32_t n0, n1, n2, K;
    uint32_t ti, tj, tk, ntiles;      // tiles per axis and in all
    cx_fdiv dtk, dtj;                 // / tk, / tj
};

// entries <= key of an ascending table
__device__ __forceinline__ uint32_t cxk_bisect_u(const uint32_t* __restrict__ tab, uint32_t n, uint32_t key) {
    uint32_t lo = 0u, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tab[mid] <= key) lo = mid + 1u; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ void cxk_sort2(uint32_t& a, uint32_t& b) { const uint32_t lo = min(a, b), hi = max(a, b); a = lo; b = hi; }

// One table answers both questions about a sample: the keys of the K thresholds and of the 2 K screen bounds (first key inside a level's
// screen, first key behind it), merged and sorted.  p = entries <= key(f); cof[p] = thresholds among the first p entries = c(f) (a NaN
// has the top key: c = K, never low); bit p of `live`: some screen holds the keys of bucket p -- only those samples are counted, and
// they are rare.
// LDS: [3][K + 1] difference arrays (int32); TAB_LDS only: the 3 K keys, cof (3 K + 1 16-bit words), live ((3 K + 32) / 32 words); the
// tile's c values (CXK_HALO 16-bit words; 0xFFFF = outside the array).  Every part starts on a multiple of 16 bytes.
static inline size_t cxk_up16(size_t b) { return (b + 15u) & ~(size_t)15u; }
static inline size_t cxk_spectrum_lds(uint32_t K, bool tab_lds) {
    size_t b = cxk_up16(3u * ((size_t)K + 1u) * 4u);
    if (tab_lds) b = cxk_up16(cxk_up16(cxk_up16(b + 3u * (size_t)K * 4u) + (3u * (size_t)K + 1u) * 2u) + ((3u * (size_t)K + 32u) >> 5) * 4u);
    return b + CXK_HALO * sizeof(uint16_t);
}
template <int DT, bool TAB_LDS>
__global__ __launch_bounds__(256) void cxk_k_spectrum(cxk_spec S, const uint32_t* __restrict__ gkeys, const uint16_t* __restrict__ gcof,
                                                      const uint32_t* __restrict__ glive, unsigned long long* __restrict__ acc) {
    extern __shared__ __attribute__((aligned(16))) uint8_t cxk_smem[];
    const uint32_t K = S.K, nd = 3u * (K + 1u), nk = 3u * K, nlw = (nk + 32u) >> 5;
    const uint32_t off_keys = (nd * 4u + 15u) & ~15u, off_cof = (off_keys + nk * 4u + 15u) & ~15u, off_live = (off_cof + (nk + 1u) * 2u + 15u) & ~15u;
    const uint32_t off_tile = TAB_LDS ? ((off_live + nlw * 4u + 15u) & ~15u) : off_keys;
    int* __restrict__ D = reinterpret_cast<int*>(cxk_smem);
    uint16_t* __restrict__ C = reinterpret_cast<uint16_t*>(cxk_smem + off_tile);
    for (uint32_t s = threadIdx.x; s < nd; s += 256u) D[s] = 0;
    if (TAB_LDS) {
        uint32_t* lk = reinterpret_cast<uint32_t*>(cxk_smem + off_keys);
        uint16_t* lc = reinterpret_cast<uint16_t*>(cxk_smem + off_cof);
        uint32_t* ll = reinterpret_cast<uint32_t*>(cxk_smem + off_live);
        for (uint32_t s = threadIdx.x; s < nk; s += 256u) lk[s] = gkeys[s];
        for (uint32_t s = threadIdx.x; s <= nk; s += 256u) lc[s] = gcof[s];
        for (uint32_t s = threadIdx.x; s < nlw; s += 256u) ll[s] = glive[s];
    }
    const uint32_t* __restrict__ keys = TAB_LDS ? (const uint32_t*)reinterpret_cast<uint32_t*>(cxk_smem + off_keys) : gkeys;
    const uint16_t* __restrict__ cof = TAB_LDS ? (const uint16_t*)reinterpret_cast<uint16_t*>(cxk_smem + off_cof) : gcof;
    const uint32_t* __restrict__ live = TAB_LDS ? (const uint32_t*)reinterpret_cast<uint32_t*>(cxk_smem + off_live) : glive;
    int* __restrict__ De = D;
    int* __restrict__ Dc = D + (K + 1u);
    int* __restrict__ Dt = D + 2u * (K + 1u);
    unsigned long long* __restrict__ near = acc + nd;
    constexpr uint32_t HK = CXK_TK + 1u, HJ = CXK_TJ + 1u;
    for (uint32_t tile = blockIdx.x; tile < S.ntiles; tile += gridDim.x) {
        const uint32_t tij = cx_div(tile, S.dtk), tkk = tile - tij * S.tk, tii = cx_div(tij, S.dtj), tjj = tij - tii * S.tj;
        const uint32_t i0 = tii * CXK_TI, j0 = tjj * CXK_TJ, k0 = tkk * CXK_TK;
        __syncthreads();      // the tile before this one has been read (and the tables are in place)
        for (uint32_t s0 = 0; s0 < CXK_HALO; s0 += 256u) {      // (uniform: the lanes of a wave count their screened samples together)
            const uint32_t s = s0 + threadIdx.x;
            const uint32_t a = s / (HJ * HK), r = s - a * (HJ * HK), b = r / HK, c = r - b * HK;
            const uint32_t i = i0 + a, j = j0 + b, k = k0 + c;
            uint32_t cv = 0xFFFFu, p = 0u;
            bool screened = false;
            if (s < CXK_HALO && i < S.n0 && j < S.n1 && k < S.n2) {
                const float f = cx_sample<DT>(S.grid, ((size_t)i * S.n1 + j) * S.n2 + k);
                p = cxk_bisect_u(keys, nk, cxk_key_f32(__float_as_uint(f)));
                cv = cof[p];
                // the samples this tile owns that lie inside some level's tolerance screen
                screened = a < CXK_TI && b < CXK_TJ && c < CXK_TK && ((live[p >> 5] >> (p & 31u)) & 1u);
            }
            if (s < CXK_HALO) C[s] = (uint16_t)cv;
            // rare on a smooth field; on a quantised one, or with a level at a value many samples share, whole waves land in one
            // bucket: one add per wave and bucket
            u64 todo = __ballot(screened);
            while (todo) {
                const int first = __ffsll((unsigned long long)todo) - 1;
                const uint32_t pb = (uint32_t)__shfl((int)p, first);
                const u64 same = __ballot(screened && p == pb);
                if ((threadIdx.x & 63u) == (uint32_t)first) atomicAdd(&near[pb], (unsigned long long)__popcll(same));
                todo &= ~same;
            }
        }
        __syncthreads();
#pragma unroll 1
        for (uint32_t q = 0; q < (CXK_TI * CXK_TJ * CXK_TK) / 256u; q++) {
            const uint32_t p = threadIdx.x + 256u * q, c = p & (CXK_TK - 1u), b = (p / CXK_TK) & (CXK_TJ - 1u), a = p / (CXK_TK * CXK_TJ);
            const uint32_t base = (a * HJ + b) * HK + c;
            const uint32_t c0 = C[base];
            if (c0 == 0xFFFFu) continue;      // no lattice point
            // corner d = 4 di + 2 dj + dk; one outside the array reads as the point itself (no edge, no cell)
            uint32_t cc[8];
            bool all_in = true, differ = false;
            cc[0] = c0;
#pragma unroll
            for (uint32_t d = 1; d < 8u; d++) {
                const uint32_t v = C[base + ((d >> 2) & 1u) * (HJ * HK) + ((d >> 1) & 1u) * HK + (d & 1u)];
                all_in = all_in && v != 0xFFFFu;
                cc[d] = v == 0xFFFFu ? c0 : v;
                differ = differ || cc[d] != c0;
            }
            if (!differ) continue;
#pragma unroll
            for (uint32_t d = 1; d < 8u; d++)
                if (cc[d] != c0) { atomicAdd(&De[min(c0, cc[d])], 1); atomicAdd(&De[max(c0, cc[d])], -1); }
            if (!all_in) continue;
            uint32_t lo = c0, hi = c0;
#pragma unroll
            for (uint32_t d = 1; d < 8u; d++) { lo = min(lo, cc[d]); hi = max(hi, cc[d]); }
            atomicAdd(&Dc[lo], 1); atomicAdd(&Dc[hi], -1);
            // the 6 Kuhn tetrahedra {0, 7, x, y} (cx_tables.h: CX_TET_CORNERS_INIT)
            const uint32_t tx[6] = {cc[1], cc[3], cc[2], cc[6], cc[4], cc[5]}, ty[6] = {cc[3], cc[2], cc[6], cc[4], cc[5], cc[1]};
#pragma unroll
            for (uint32_t t = 0; t < 6u; t++) {
                uint32_t s0 = cc[0], s1 = cc[7], s2 = tx[t], s3 = ty[t];
                cxk_sort2(s0, s1); cxk_sort2(s2, s3); cxk_sort2(s0, s2); cxk_sort2(s1, s3); cxk_sort2(s1, s2);
                if (s0 == s3) continue;
                atomicAdd(&Dt[s0], 1); atomicAdd(&Dt[s3], -1);
                if (s1 != s2) { atomicAdd(&Dt[s1], 1); atomicAdd(&Dt[s2], -1); }
            }
        }
    }
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < nd; s += 256u) {
        const int v = D[s];
        if (v) atomicAdd(&acc[s], (unsigned long long)(long long)v);      // (two's complement: the sums are exact)
    }
}

// the tolerance screen of one level, as the march evaluates it in fp32 (cx_cell.h: fabsf(f - vcmp) <= near_abs)
static inline bool cxk_screen(uint32_t key, float vcmp, float near_abs) {
    const uint32_t u = cxk_unkey_f32(key);
    float f; memcpy(&f, &u, 4);
    volatile float d = f - vcmp;
    return std::fabs(d) <= near_abs;
}

extern "C" int cx_level_spectrum3d(cx_ctx* ctx, const double* values, int32_t nlevels, int64_t* n_cells, int64_t* n_vertices, int64_t* n_triangles,
                                   int64_t* n_near) {
    if (!ctx) return CX_ERR_INVALID;
    if (!ctx->grid.p) { ctx->err = "cx_level_spectrum3d: no grid bound"; return CX_ERR_STATE; }
    if (!values || nlevels < 1 || nlevels > CXK_MAX_LEVELS) return cxk_invalid(ctx, "cx_level_spectrum3d: 1..4096 values");
    if (ctx->n0 < 2 || ctx->n1 < 2 || ctx->n2 < 2) return cxk_invalid(ctx, "cx_level_spectrum3d: at least 2 samples per axis");
    const uint32_t K = (uint32_t)nlevels;
    // per level the march's own threshold and screen (cx_fill_value_params), then the levels in ascending threshold
    std::vector<float> vcmp(K), nabs(K);
    for (uint32_t l = 0; l < K; l++) {
        if (!std::isfinite(values[l]) || std::fabs(values[l]) > 3.4028234663852886e38) return cxk_invalid(ctx, "cx_level_spectrum3d: a value that is not a finite fp32 number");
        cx_params P;
        cx_fill_value_params(P, values[l]);
        vcmp[l] = P.vcmp; nabs[l] = P.near_abs;
    }
    std::vector<uint32_t> order(K);
    for (uint32_t l = 0; l < K; l++) order[l] = l;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return vcmp[a] < vcmp[b]; });
    // the screen of level l holds the keys klo .. khi1 - 1: both ends found on the fp32 number line with the march's own expression
    std::vector<uint32_t> klo(K), khi1(K);
    std::vector<std::pair<uint32_t, uint32_t>> merged;      // {key, 1 = a threshold}
    merged.reserve(3u * (size_t)K);
    const uint32_t key_ninf = 0x007FFFFFu, key_pinf = 0xFF800000u;
    for (uint32_t l = 0; l < K; l++) {
        uint32_t u; memcpy(&u, &vcmp[l], 4);
        const uint32_t kv = cxk_key_f32(u);
        uint32_t a = key_ninf, b = kv;      // first key in [a, b] inside the screen (kv is)
        while (a < b) { const uint32_t m = a + ((b - a) >> 1); if (cxk_screen(m, vcmp[l], nabs[l])) b = m; else a = m + 1u; }
        klo[l] = a;
        a = kv; b = key_pinf;               // last key in [a, b] inside the screen
        while (a < b) { const uint32_t m = a + ((b - a + 1u) >> 1); if (cxk_screen(m, vcmp[l], nabs[l])) a = m; else b = m - 1u; }
        khi1[l] = a + 1u;
        merged.emplace_back(kv, 1u); merged.emplace_back(klo[l], 0u); merged.emplace_back(khi1[l], 0u);
    }
    std::sort(merged.begin(), merged.end());
    const uint32_t nk = 3u * K, nlw = (nk + 32u) >> 5;
    std::vector<uint32_t> keys(nk), livew(nlw, 0u);
    std::vector<uint16_t> cof(nk + 1u);
    cof[0] = 0;
    for (uint32_t e = 0; e < nk; e++) { keys[e] = merged[e].first; cof[e + 1u] = (uint16_t)(cof[e] + merged[e].second); }
    // bucket p = the samples with p entries <= their key.  The buckets of a screen: entries <= klo  ..  entries <= khi1, the last excluded
    auto bucket = [&](uint32_t key) { return (uint32_t)(std::upper_bound(keys.begin(), keys.end(), key) - keys.begin()); };
    std::vector<int32_t> cover(nk + 2u, 0);
    for (uint32_t l = 0; l < K; l++) { cover[bucket(klo[l])]++; cover[bucket(khi1[l])]--; }
    int32_t run = 0;
    for (uint32_t b = 0; b <= nk; b++) { run += cover[b]; if (run > 0) livew[b >> 5] |= 1u << (b & 31u); }

    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_pick_state* Z = cxk_state(ctx);
    if (!Z) return CX_ERR_NOMEM;
    hipStream_t st = ctx->stream;
    const size_t nd = 3u * ((size_t)K + 1u), nacc = nd + (size_t)nk + 1u;
    int rc;
    if ((rc = Z->acc.grow(ctx, nacc))) return rc;
    if ((rc = Z->keys.grow(ctx, (size_t)nk + nlw))) return rc;
    if ((rc = Z->cof.grow(ctx, (size_t)nk + 1u))) return rc;
    CX_HIP(ctx, hipMemsetAsync(Z->acc, 0, nacc * sizeof(unsigned long long), st));
    CX_HIP(ctx, hipMemcpyAsync(Z->keys, keys.data(), (size_t)nk * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    CX_HIP(ctx, hipMemcpyAsync(Z->keys + nk, livew.data(), (size_t)nlw * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    CX_HIP(ctx, hipMemcpyAsync(Z->cof, cof.data(), ((size_t)nk + 1u) * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    cxk_spec S;
    memset(&S, 0, sizeof(S));
    S.grid = ctx->grid;
    S.n0 = (uint32_t)ctx->n0; S.n1 = (uint32_t)ctx->n1; S.n2 = (uint32_t)ctx->n2; S.K = K;
    S.ti = (S.n0 + CXK_TI - 1u) / CXK_TI; S.tj = (S.n1 + CXK_TJ - 1u) / CXK_TJ; S.tk = (S.n2 + CXK_TK - 1u) / CXK_TK;
    S.ntiles = S.ti * S.tj * S.tk;      // (at most 2^29 samples: fits)
    S.dtk = cx_fdiv_make(S.tk); S.dtj = cx_fdiv_make(S.tj);
    const bool tab_lds = K <= CXK_TAB_LDS_MAX;
    const size_t lds = cxk_spectrum_lds(K, tab_lds);
    // persistent workgroups: the difference arrays are zeroed and flushed once each, so their number follows K, not the grid
    const uint32_t grid = std::min<uint32_t>(S.ntiles, K <= 256u ? 2048u : (K <= 1024u ? 1024u : 512u));
#define CX_LAUNCH(DT)                                                                                                                          \
    if (tab_lds) hipLaunchKernelGGL((cxk_k_spectrum<DT, true>), dim3(grid), dim3(256), lds, st, S, (const uint32_t*)Z->keys.get(),              \
                                    (const uint16_t*)Z->cof.get(), (const uint32_t*)Z->keys.get() + nk, Z->acc.get());                        \
    else hipLaunchKernelGGL((cxk_k_spectrum<DT, false>), dim3(grid), dim3(256), lds, st, S, (const uint32_t*)Z->keys.get(),                     \
                            (const uint16_t*)Z->cof.get(), (const uint32_t*)Z->keys.get() + nk, Z->acc.get());
    CX_DISPATCH_DTYPE(ctx->grid.dtype, CX_LAUNCH)
#undef CX_LAUNCH
    CX_HIP(ctx, hipGetLastError());
    Z->host.resize(nacc);
    CX_HIP(ctx, hipMemcpyAsync(Z->host.data(), Z->acc, nacc * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    CX_HIP(ctx, hipStreamSynchronize(st));
    // prefix sums of the difference arrays in sorted order, suffix sums of the buckets
    const unsigned long long* H = Z->host.data();
    std::vector<unsigned long long> above((size_t)nk + 2u, 0ull);      // above[b]: counted samples in buckets >= b
    for (size_t b = (size_t)nk + 1u; b-- > 0;) above[b] = above[b + 1u] + H[nd + b];
    long long se = 0, sc = 0, stt = 0;
    for (uint32_t s = 0; s < K; s++) {
        se += (long long)H[s]; sc += (long long)H[(K + 1u) + s]; stt += (long long)H[2u * (K + 1u) + s];
        const uint32_t l = order[s];
        if (n_vertices) n_vertices[l] = se;
        if (n_cells) n_cells[l] = sc;
        if (n_triangles) n_triangles[l] = stt;
    }
    if (n_near)
        for (uint32_t l = 0; l < K; l++) n_near[l] = (int64_t)(above[bucket(klo[l])] - above[bucket(khi1[l])]);
    return CX_OK;
}
