// cx_recon.hip -- grey morphological reconstruction of a volume (include/contourist_hip.h, section "reconstruction"): the largest array
// R <= mask that dominates the clamped marker and in which every sample is reached from it by a non-increasing path of neighbours
// (cx_grid_reconstruct3d), its dual by erosion, and the result as the bound grid (cx_grid_reconstruct3d_bind).  h-maxima, regional
// extrema, grey fill-holes, grey clear-border and binary propagation are marker kinds of it.
//
// Nothing is computed but minima and maxima of keys.  Every sample becomes a key of its own width whose unsigned order is the header's
// order (cx_dev.h: cxd_sample_key); reconstruction by erosion runs the same kernels on the complemented keys.  `state` holds one
// working key per sample: the clamped marker after cxr_k_init, the result after the last round.  The result is the unique fixed point of
//     v[i] = min(mask[i], max(v[i], v[j] for the neighbours j of i))
// above the clamped marker, whatever order the updates are applied in.
//
// A workgroup of 256 threads owns a tile of CXR_T0 x CXR_T1 x CXR_T2 = 8 x 8 x 64 samples (cxr_k_round).  It stages the tile's mask keys
// and the state keys of the tile and a halo of one sample (10 x 10 x 66, zero = the bottom of the order outside the array) in LDS and
// iterates to the tile's fixed point there.  One sweep is
//   along axis 2   a wave per row, a lane per sample: v[k] = min(m[k], max(v[k], v[k-1])) is the clamp x -> min(b, max(a, x)) with
//                  a = v[k], b = m[k]; clamps compose to clamps (lo = min(b2, max(a2, a1)), hi = min(b2, max(a2, b1))), so a forward
//                  and a backward Kogge-Stone scan over the 64 lanes do the work of 2 x 64 sequential steps;
//   along axis 1 and 0   a thread per column, 8 sequential steps forward and 8 back, the lanes along axis 2; the diagonal neighbours of
//                  connectivity 2 and 3 are read from the plane the sweep comes from.
// Sweeps repeat until a workgroup-wide OR says that nothing moved, at most CXR_TILE + 1 times: a value reaches a sample along a path
// of at most CXR_TILE steps inside the tile, and every sweep advances it by one step at least.  (A tile still moving at the bound --
// no correct run gets there -- puts itself on the list again, so not even the bound is a matter of correctness.)
//
// Rounds.  One launch per round over the list of active tiles; round 0 visits every tile.  A tile that raised a sample writes its
// interior back with plain stores and puts on the next round's list the neighbour tiles in whose halo a raised sample lies (a flag
// word per tile and round parity, claimed by atomicExch, so a tile is listed once; one atomicAdd per visited tile appends the claims
// of a wave).  The host reads the counters after every CXR_BATCH launches and stops when the next list is empty.
//
// Why the order does not matter.  A tile may read a neighbour's samples for its halo while that neighbour writes
// them in the same launch.  (1) Every key ever stored in `state` lies between the clamped marker and the result: a stored key is a
// minimum or maximum of keys that do, and the update never lowers a key.  (2) A sample is one aligned access of 1, 2 or 4 bytes, which
// does not tear: a racing read returns some key that was stored.  So a stale halo can only leave the tile BELOW the result, never take
// it above or to a wrong fixed point.  (3) The neighbour that stored the newer key raised a sample of its shell, so it lists this tile
// for the next round, whose launch boundary makes the key visible.  When no tile is listed every tile has seen the final halo and is
// at its fixed point: the whole array is at the fixed point, which is unique.  No workgroup waits for another: no grid barrier, no
// flag is polled, no kernel is persistent.
//
// Every loop is bounded: the sweeps by CXR_TILE + 1, the rounds by the number of samples + 8.  (The number of tiles is NOT a bound: a
// front crosses one tile boundary per round at least, but a winding corridor crosses the same boundary many times.  A path without
// repeats has fewer steps than the array has samples.)  Past the bound the call returns CX_ERR_HIP.
#include <cmath>
#include <cstring>
#include <new>
#include <utility>

#include "cx_dev.h"
#include "cx_gridop.h"

#define CXR_T0 8
#define CXR_T1 8
#define CXR_T2 64
#define CXR_H1 (CXR_T1 + 2)
#define CXR_H2 (CXR_T2 + 2)
#define CXR_TILE (CXR_T0 * CXR_T1 * CXR_T2)                         // 4096 samples
#define CXR_HALO ((CXR_T0 + 2) * CXR_H1 * CXR_H2)                   // 6600 state keys
#define CXR_BATCH 4u                                                // launches between two reads of the counters
#define CXR_GRID 4096u                                              // workgroups of a round whose list the host has not read
#define CXR_INIT_GRID 2048u                                         // workgroups of the first and the last pass (a counter add per wave)

struct cxr_counters {          // 64 bytes, zeroed before every call
    uint32_t cnt[3];           // tiles on the list of round r: cnt[r % 3]
    uint32_t pad;
    u64 visits, rounds;        // tiles visited, launches that visited one
    u64 n_changed, n_clamped;
    u64 n_moved;               // samples whose clamped marker differs from the mask
    u64 pad2;
};

struct cx_recon_state : cx_slot {      // (`in`: a host mask)
    cx_buf<uint8_t> in2;       // a host marker
    cx_buf<uint8_t> state;     // a working key per sample
    cx_buf<uint32_t> work;     // two lists and two flag arrays of one word per tile
    cx_buf<uint8_t> counters;  // cxr_counters
    cx_buf<uint8_t> prev;      // the result of the call before, where that is an input of this call
    int32_t dtype = CX_DTYPE_F32, out_kind = CX_RECON_OUT_VALUES;      // of the result
};

void cx_recon_free(cx_ctx* ctx) {
    delete ctx->recon;
    ctx->recon = nullptr;
}

struct cxr_args {
    const void* mask;
    const void* marker;
    void* state;
    void* out;
    uint32_t* list[2];
    uint32_t* flags[2];
    cxr_counters* C;
    int64_t n[3];
    uint32_t g[3], tiles;                // tiles per axis and in all
    int32_t dtype, kind, conn, erosion, out_kind;
    uint32_t faces;
    double h;
    uint32_t h_int;                      // h of an integer type, at most 65536
    uint32_t round, first;
    uint32_t all_ones;                   // the last pass writes ones everywhere (the CHANGED mask of a constant integer extreme)
};

// the bits of double d rounded once to the float type (round to nearest even).  16-bit types: d to fp32 rounded to ODD (truncated, the
// last bit set when inexact), which the second rounding of 13 or 16 fewer bits cannot tell from d itself
__device__ __forceinline__ uint32_t cxr_float_bits(int32_t dtype, double d) {
    if (dtype == CX_DTYPE_F32) return __float_as_uint((float)d);
    float f = __double2float_rz(d);
    if ((double)f != d) f = __uint_as_float(__float_as_uint(f) | 1u);
    const uint32_t u = __float_as_uint(f);
    if (dtype == CX_DTYPE_F16) {
        const _Float16 hh = (_Float16)f;
        return (uint32_t)__builtin_bit_cast(uint16_t, hh);
    }
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0x7FC0u;
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ double cxr_float_value(int32_t dtype, uint32_t raw) {
    if (dtype == CX_DTYPE_F32) return (double)__uint_as_float(raw);
    if (dtype == CX_DTYPE_BF16) return (double)__uint_as_float(raw << 16);
    return (double)(float)__builtin_bit_cast(_Float16, (uint16_t)raw);
}
__device__ __forceinline__ bool cxr_is_float(int32_t dtype) { return dtype == CX_DTYPE_F32 || dtype == CX_DTYPE_F16 || dtype == CX_DTYPE_BF16; }

// the marker's key for a sample with bits `raw` and key k, CX_RECON_MARKER_SHIFT and _STEP (in the order of the keys, not the working one)
template <uint32_t ONES>
__device__ __forceinline__ uint32_t cxr_shift(const cxr_args& A, uint32_t raw, uint32_t k) {
    if (!cxr_is_float(A.dtype)) {
        if (A.erosion) return min(k + A.h_int, ONES);
        return k > A.h_int ? k - A.h_int : 0u;
    }
    if (k == ONES) return ONES;
    const double v = cxr_float_value(A.dtype, raw);
    return cxd_sample_key(A.dtype, cxr_float_bits(A.dtype, A.erosion ? v + A.h : v - A.h));
}
template <uint32_t ONES>
__device__ __forceinline__ uint32_t cxr_step(const cxr_args& A, uint32_t k) {
    uint32_t low = 0u, high = ONES;      // the ends of the order without NaN
    const bool fl = cxr_is_float(A.dtype);
    if (A.dtype == CX_DTYPE_F32) { low = 0x007FFFFFu; high = 0xFF800000u; }
    else if (A.dtype == CX_DTYPE_F16) { low = 0x03FFu; high = 0xFC00u; }
    else if (A.dtype == CX_DTYPE_BF16) { low = 0x007Fu; high = 0xFF80u; }
    if (A.erosion) return (fl && k == ONES) ? ONES : (k >= high ? k : k + 1u);
    return (fl && k == ONES) ? high : (k <= low ? k : k - 1u);
}

// round 0: the clamped marker, as working keys
template <typename K>
__global__ __launch_bounds__(256) void cxr_k_init(const cxr_args A) {
    constexpr uint32_t ONES = (uint32_t)(K) ~(K)0;
    const K* __restrict__ mask = static_cast<const K*>(A.mask);
    const K* __restrict__ marker = static_cast<const K*>(A.marker);
    K* __restrict__ state = static_cast<K*>(A.state);
    const size_t total = (size_t)A.n[0] * (size_t)A.n[1] * (size_t)A.n[2], plane = (size_t)A.n[1] * (size_t)A.n[2];
    const uint32_t flip = A.erosion ? ONES : 0u;
    long long clamped = 0, moved = 0;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < total; i += (size_t)gridDim.x * 256u) {
        const uint32_t raw = (uint32_t)mask[i], k = cxd_sample_key(A.dtype, raw);
        uint32_t g;
        if (A.kind == CX_RECON_MARKER_ARRAY) g = cxd_sample_key(A.dtype, (uint32_t)marker[i]);
        else if (A.kind == CX_RECON_MARKER_SHIFT) g = cxr_shift<ONES>(A, raw, k);
        else if (A.kind == CX_RECON_MARKER_STEP) g = cxr_step<ONES>(A, k);
        else {
            const size_t i0 = i / plane, rest = i - i0 * plane, i1 = rest / (size_t)A.n[2], i2 = rest - i1 * (size_t)A.n[2];
            const uint32_t on = (i0 == 0 ? 1u : 0u) | ((int64_t)i0 == A.n[0] - 1 ? 2u : 0u) | (i1 == 0 ? 4u : 0u) | ((int64_t)i1 == A.n[1] - 1 ? 8u : 0u) |
                                (i2 == 0 ? 16u : 0u) | ((int64_t)i2 == A.n[2] - 1 ? 32u : 0u);
            g = (on & A.faces) ? k : flip;
        }
        const uint32_t w = k ^ flip;
        uint32_t gw = g ^ flip;
        if (gw > w) { clamped++; gw = w; }
        if (gw != w) moved++;
        state[i] = (K)gw;
    }
    clamped = cxd_wave_add(clamped);
    moved = cxd_wave_add(moved);
    if ((threadIdx.x & 63u) == 0u) {
        if (clamped) atomicAdd(&A.C->n_clamped, (u64)clamped);
        if (moved) atomicAdd(&A.C->n_moved, (u64)moved);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) A.C->cnt[0] = A.tiles;
}

extern __shared__ __align__(16) unsigned char cxr_smem[];

// where a sample of the tile lies on the tile's shell, per axis 0 = low face, 1 = inside, 2 = high face: bit (c0 3 + c1) 3 + c2
__device__ __forceinline__ uint32_t cxr_class(uint32_t d0, uint32_t d1, uint32_t d2) {
    const uint32_t c0 = d0 == 0u ? 0u : (d0 == CXR_T0 - 1u ? 2u : 1u), c1 = d1 == 0u ? 0u : (d1 == CXR_T1 - 1u ? 2u : 1u), c2 = d2 == 0u ? 0u : (d2 == CXR_T2 - 1u ? 2u : 1u);
    return 1u << ((c0 * 3u + c1) * 3u + c2);
}

// one round: every tile of the list to its fixed point under the halo it finds
template <typename K>
__global__ __launch_bounds__(256) void cxr_k_round(const cxr_args A) {
    constexpr uint32_t ONES = (uint32_t)(K) ~(K)0;
    constexpr uint32_t V_BYTES = (CXR_HALO * (uint32_t)sizeof(K) + 15u) & ~15u;
    uint32_t* words = reinterpret_cast<uint32_t*>(cxr_smem);      // [0]: the classes of the samples this visit raised
    K* V = reinterpret_cast<K*>(cxr_smem + 16);                   // state keys [10][10][66]
    K* M = reinterpret_cast<K*>(cxr_smem + 16 + V_BYTES);         // mask keys [8][8][64]
    const K* __restrict__ mask = static_cast<const K*>(A.mask);
    K* state = static_cast<K*>(A.state);
    cxr_counters* C = A.C;
    const uint32_t r = A.round, n_active = min(C->cnt[r % 3u], A.tiles);      // (a tile is listed once: never more than all of them)
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t flip = A.erosion ? ONES : 0u;
    const int conn = A.conn;
    if (blockIdx.x == 0 && tid == 0) {
        C->cnt[(r + 2u) % 3u] = 0u;      // the list after the next one: nobody reads or appends to it in this launch
        C->visits += n_active;
        if (n_active) C->rounds += 1ull;
    }
    uint32_t* list_next = A.list[(r + 1u) & 1u];
    uint32_t* flags_next = A.flags[(r + 1u) & 1u];
    for (uint32_t it = blockIdx.x; it < n_active; it += gridDim.x) {
        const uint32_t tile = A.first ? it : A.list[r & 1u][it];
        if (tile >= A.tiles) continue;      // (never: the lists hold tile numbers)
        const uint32_t t2 = tile % A.g[2], t01 = tile / A.g[2], t1 = t01 % A.g[1], t0 = t01 / A.g[1];
        const int64_t b0 = (int64_t)t0 * CXR_T0, b1 = (int64_t)t1 * CXR_T1, b2 = (int64_t)t2 * CXR_T2;
        for (uint32_t e = tid; e < CXR_HALO; e += 256u) {
            const uint32_t row = e / CXR_H2, h2 = e - row * CXR_H2, h0 = row / CXR_H1, h1 = row - h0 * CXR_H1;
            const int64_t i0 = b0 + (int64_t)h0 - 1, i1 = b1 + (int64_t)h1 - 1, i2 = b2 + (int64_t)h2 - 1;
            K v = 0;
            if (i0 >= 0 && i0 < A.n[0] && i1 >= 0 && i1 < A.n[1] && i2 >= 0 && i2 < A.n[2]) v = state[((size_t)i0 * (size_t)A.n[1] + (size_t)i1) * (size_t)A.n[2] + (size_t)i2];
            V[e] = v;
        }
        for (uint32_t e = tid; e < CXR_TILE; e += 256u) {
            const int64_t i0 = b0 + (e >> 9), i1 = b1 + ((e >> 6) & 7u), i2 = b2 + (e & 63u);
            uint32_t m = 0u;      // outside the array: nothing rises there and nothing passes
            if (i0 < A.n[0] && i1 < A.n[1] && i2 < A.n[2])
                m = cxd_sample_key(A.dtype, (uint32_t)mask[((size_t)i0 * (size_t)A.n[1] + (size_t)i1) * (size_t)A.n[2] + (size_t)i2]) ^ flip;
            M[e] = (K)m;
        }
        if (tid == 0) words[0] = 0u;
        __syncthreads();
        uint32_t cls = 0u;
        int moving = 1;
        for (uint32_t sweep = 0; sweep <= CXR_TILE && moving; sweep++) {
            int ch = 0;
            // along axis 2: a wave per row
            for (uint32_t row = wave; row < CXR_T0 * CXR_T1; row += 4u) {
                const uint32_t d0 = row >> 3, d1 = row & 7u;
                K* vr = V + ((d0 + 1u) * CXR_H1 + d1 + 1u) * CXR_H2;
                const uint32_t m = M[row * CXR_T2 + lane], v = vr[lane + 1u];
                const uint32_t left = vr[0], right = vr[CXR_H2 - 1];
                const uint32_t before = (uint32_t)__shfl_up((int)v, 1), after = (uint32_t)__shfl_down((int)v, 1);
                // no sample below its mask with a higher neighbour in the row: the row is at its fixed point, the scans would move nothing
                if (!__any(v < m && max(lane == 0u ? left : before, lane == 63u ? right : after) > v)) continue;
                uint32_t a = lane == 0u ? min(m, max(v, left)) : v, b = m;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t pa = (uint32_t)__shfl_up((int)a, o), pb = (uint32_t)__shfl_up((int)b, o);
                    if (lane >= (uint32_t)o) { const uint32_t na = min(b, max(a, pa)); b = min(b, max(a, pb)); a = na; }
                }
                a = lane == 63u ? min(m, max(a, right)) : a;
                b = m;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t pa = (uint32_t)__shfl_down((int)a, o), pb = (uint32_t)__shfl_down((int)b, o);
                    if (lane + (uint32_t)o < 64u) { const uint32_t na = min(b, max(a, pa)); b = min(b, max(a, pb)); a = na; }
                }
                if (a != v) { vr[lane + 1u] = (K)a; ch = 1; cls |= cxr_class(d0, d1, lane); }
            }
            __syncthreads();
            // along axis 1: a thread per column (d0, lane), forward and back; connectivity 2: the plane's neighbours along axis 2 too
            for (uint32_t col = tid; col < CXR_T0 * CXR_T2; col += 256u) {
                const uint32_t d0 = col >> 6;
                K* p = V + ((d0 + 1u) * CXR_H1) * CXR_H2 + lane + 1u;      // the halo row d1 = -1 of the column
                const K* mp = M + (d0 * CXR_T1) * CXR_T2 + lane;
                for (int s = 0; s < 2 * CXR_T1; s++) {
                    const int d1 = s < CXR_T1 ? s : 2 * CXR_T1 - 1 - s;
                    const K* from = p + (s < CXR_T1 ? d1 : d1 + 2) * CXR_H2;
                    uint32_t nb = from[0];
                    if (conn >= 2) nb = max(nb, max((uint32_t)from[-1], (uint32_t)from[1]));
                    const uint32_t v = p[(d1 + 1) * CXR_H2], m = mp[d1 * CXR_T2], nv = min(m, max(v, nb));
                    if (nv != v) { p[(d1 + 1) * CXR_H2] = (K)nv; ch = 1; cls |= cxr_class(d0, (uint32_t)d1, lane); }
                }
            }
            __syncthreads();
            // along axis 0: a thread per column (d1, lane); connectivity 2: the plane's four edge neighbours, 3: its four corners too
            for (uint32_t col = tid; col < CXR_T1 * CXR_T2; col += 256u) {
                const uint32_t d1 = col >> 6;
                K* p = V + (d1 + 1u) * CXR_H2 + lane + 1u;      // the halo plane d0 = -1 of the column
                const K* mp = M + d1 * CXR_T2 + lane;
                for (int s = 0; s < 2 * CXR_T0; s++) {
                    const int d0 = s < CXR_T0 ? s : 2 * CXR_T0 - 1 - s;
                    const K* from = p + (s < CXR_T0 ? d0 : d0 + 2) * (CXR_H1 * CXR_H2);
                    uint32_t nb = from[0];
                    if (conn >= 2) nb = max(max(nb, max((uint32_t)from[-1], (uint32_t)from[1])), max((uint32_t)from[-CXR_H2], (uint32_t)from[CXR_H2]));
                    if (conn >= 3) nb = max(max(nb, max((uint32_t)from[-CXR_H2 - 1], (uint32_t)from[-CXR_H2 + 1])), max((uint32_t)from[CXR_H2 - 1], (uint32_t)from[CXR_H2 + 1]));
                    const uint32_t v = p[(d0 + 1) * (CXR_H1 * CXR_H2)], m = mp[d0 * (CXR_T1 * CXR_T2)], nv = min(m, max(v, nb));
                    if (nv != v) { p[(d0 + 1) * (CXR_H1 * CXR_H2)] = (K)nv; ch = 1; cls |= cxr_class((uint32_t)d0, d1, lane); }
                }
            }
            moving = __syncthreads_or(ch);
        }
        if (cls) atomicOr(&words[0], cls);
        __syncthreads();
        const uint32_t raised = words[0];
        if (raised) {
            for (uint32_t e = tid; e < CXR_TILE; e += 256u) {
                const uint32_t d0 = e >> 9, d1 = (e >> 6) & 7u, d2 = e & 63u;
                const int64_t i0 = b0 + d0, i1 = b1 + d1, i2 = b2 + d2;
                if (i0 < A.n[0] && i1 < A.n[1] && i2 < A.n[2])
                    state[((size_t)i0 * (size_t)A.n[1] + (size_t)i1) * (size_t)A.n[2] + (size_t)i2] = V[((d0 + 1u) * CXR_H1 + d1 + 1u) * CXR_H2 + d2 + 1u];
            }
        }
        if (wave == 0u) {
            // lane j < 27 speaks for the tile at offset (j / 9 - 1, j / 3 % 3 - 1, j % 3 - 1): listed when a raised sample lies in its halo
            bool want = false;
            uint32_t nt = 0u;
            if (lane < 27u) {
                const int o0 = (int)(lane / 9u) - 1, o1 = (int)((lane / 3u) % 3u) - 1, o2 = (int)(lane % 3u) - 1;
                const int nz = (o0 != 0) + (o1 != 0) + (o2 != 0);
                if (nz == 0) want = moving != 0;      // still moving at the sweep bound: this tile again
                else if (nz <= conn) {
                    for (uint32_t c = 0; c < 27u; c++) {
                        const int s0 = (int)(c / 9u) - 1, s1 = (int)((c / 3u) % 3u) - 1, s2 = (int)(c % 3u) - 1;
                        if (((raised >> c) & 1u) && (o0 == 0 || s0 == o0) && (o1 == 0 || s1 == o1) && (o2 == 0 || s2 == o2)) want = true;
                    }
                }
                const int64_t q0 = (int64_t)t0 + o0, q1 = (int64_t)t1 + o1, q2 = (int64_t)t2 + o2;
                if (q0 < 0 || q0 >= (int64_t)A.g[0] || q1 < 0 || q1 >= (int64_t)A.g[1] || q2 < 0 || q2 >= (int64_t)A.g[2]) want = false;
                else nt = (uint32_t)((q0 * (int64_t)A.g[1] + q1) * (int64_t)A.g[2] + q2);
            }
            const bool won = want && atomicExch(&flags_next[nt], 1u) == 0u;
            const uint64_t winners = __ballot(won);
            if (winners != 0ULL) {      // (wave-uniform)
                const int leader = __ffsll((long long)winners) - 1;
                uint32_t base = 0u;
                if ((int)lane == leader) base = atomicAdd(&C->cnt[(r + 1u) % 3u], (uint32_t)__popcll(winners));
                base = (uint32_t)__shfl((int)base, leader);
                const uint32_t pos = base + (uint32_t)__popcll(winners & ((1ULL << lane) - 1ULL));
                if (won && pos < A.tiles) list_next[pos] = nt;
            }
            if (!A.first && lane == 0u) A.flags[r & 1u][tile] = 0u;      // this round's claim on the tile is spent
        }
        __syncthreads();      // LDS is staged again
    }
}

// the last pass: the result in the samples' type or the CHANGED mask, and n_changed
template <typename K>
__global__ __launch_bounds__(256) void cxr_k_final(const cxr_args A) {
    constexpr uint32_t ONES = (uint32_t)(K) ~(K)0;
    const K* __restrict__ mask = static_cast<const K*>(A.mask);
    const K* __restrict__ state = static_cast<const K*>(A.state);
    const size_t total = (size_t)A.n[0] * (size_t)A.n[1] * (size_t)A.n[2];
    const uint32_t flip = A.erosion ? ONES : 0u;
    long long changed = 0;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < total; i += (size_t)gridDim.x * 256u) {
        const uint32_t w = cxd_sample_key(A.dtype, (uint32_t)mask[i]) ^ flip, s = state[i];
        const bool differs = s != w;
        changed += differs ? 1 : 0;
        if (A.out_kind == CX_RECON_OUT_VALUES) static_cast<K*>(A.out)[i] = (K)cxd_sample_unkey(A.dtype, s ^ flip);
        else static_cast<uint8_t*>(A.out)[i] = (differs || A.all_ones) ? 1u : 0u;
    }
    changed = cxd_wave_add(changed);
    if ((threadIdx.x & 63u) == 0u && changed) atomicAdd(&A.C->n_changed, (u64)changed);
}

static_assert(CXR_T2 == 64 && CXR_T0 * CXR_T2 == 512 && CXR_T1 * CXR_T2 == 512, "a lane per sample of a row; two columns per thread");
static_assert(16u + ((CXR_HALO * 4u + 15u) & ~15u) + CXR_TILE * 4u <= 65536u, "the LDS of a tile of 32-bit keys");

template <typename K>
static void cxr_launch_init(const cxr_args& A, dim3 grid, hipStream_t st) { hipLaunchKernelGGL(cxr_k_init<K>, grid, dim3(256), 0, st, A); }
template <typename K>
static void cxr_launch_round(const cxr_args& A, dim3 grid, hipStream_t st) {
    const size_t lds = 16u + ((CXR_HALO * sizeof(K) + 15u) & ~(size_t)15u) + CXR_TILE * sizeof(K);      // 10720, 21408 or 42800 bytes
    hipLaunchKernelGGL(cxr_k_round<K>, grid, dim3(256), lds, st, A);
}
template <typename K>
static void cxr_launch_final(const cxr_args& A, dim3 grid, hipStream_t st) { hipLaunchKernelGGL(cxr_k_final<K>, grid, dim3(256), 0, st, A); }

#define CXR_BY_WIDTH(esize, call)                         \
    switch (esize) {                                      \
        case 1: call<uint8_t>(A, grid, st); break;        \
        case 2: call<uint16_t>(A, grid, st); break;       \
        default: call<uint32_t>(A, grid, st); break;      \
    }

extern "C" int cx_grid_reconstruct3d(cx_ctx* ctx, const void* mask, int32_t dtype, int on_device, int64_t n0, int64_t n1, int64_t n2,
                                     const void* marker, int32_t marker_kind, double h, int32_t faces, int32_t method, int32_t connectivity,
                                     int32_t out_kind, void* out_device, void* out_host, cx_recon_stats* stats) {
    if (!ctx) return CX_ERR_INVALID;
    if (method != CX_RECON_DILATION && method != CX_RECON_EROSION) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_reconstruct3d: unknown method");
    if (connectivity < 1 || connectivity > 3) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_reconstruct3d: a connectivity of 1, 2 or 3");
    if (out_kind != CX_RECON_OUT_VALUES && out_kind != CX_RECON_OUT_CHANGED) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_reconstruct3d: unknown output kind");
    if (marker_kind < CX_RECON_MARKER_ARRAY || marker_kind > CX_RECON_MARKER_RIM) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_reconstruct3d: unknown marker kind");
    if (marker_kind == CX_RECON_MARKER_ARRAY && !marker) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_reconstruct3d: CX_RECON_MARKER_ARRAY without a marker");
    if (marker_kind == CX_RECON_MARKER_RIM && (faces <= 0 || faces > 63)) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_reconstruct3d: CX_RECON_MARKER_RIM takes 1 to 6 of the face bits");
    if (marker_kind == CX_RECON_MARKER_SHIFT && !(std::isfinite(h) && h > 0.0)) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_reconstruct3d: h must be finite and above 0");
    cx_source M;
    int rc = cx_source_resolve(ctx, "cx_grid_reconstruct3d", mask, dtype, on_device, n0, n1, n2, 31, &M, true);
    if (rc) return rc;
    dtype = M.dtype; n0 = M.n[0]; n1 = M.n[1]; n2 = M.n[2]; on_device = M.on_device;      // (a marker array lives where the mask does)
    const bool is_float = dtype == CX_DTYPE_F32 || dtype == CX_DTYPE_F16 || dtype == CX_DTYPE_BF16;
    if (marker_kind == CX_RECON_MARKER_SHIFT && !is_float && h != std::floor(h)) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_reconstruct3d: h of an integer type must be an integer");
    const size_t esize = cx_dtype_size(dtype), total = M.count, bytes = M.bytes;
    const size_t out_bytes = out_kind == CX_RECON_OUT_VALUES ? bytes : total;
    const bool marker_dev = marker_kind == CX_RECON_MARKER_ARRAY && on_device;
    if ((on_device && cx_overlap(M.p, bytes, out_device, out_bytes)) || (marker_dev && cx_overlap(marker, bytes, out_device, out_bytes)))
        return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_reconstruct3d: the output overlaps an input");
    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_recon_state* S = cx_state_of(ctx->recon);
    if (!S) return CX_ERR_NOMEM;
    hipStream_t st = ctx->stream;
    // an input that lies in the result of the call before: that buffer steps aside into `prev`, the mask's scratch keeps its memory
    const void* mask_d = M.p;
    const void* marker_d = marker_kind == CX_RECON_MARKER_ARRAY ? marker : nullptr;
    if (on_device) S->step_aside(M.p, bytes, S->prev);
    else if ((rc = cx_upload(ctx, S->in, M.p, bytes, &mask_d))) return rc;
    if (marker_dev) S->step_aside(marker, bytes, S->prev);
    else if (marker_d && (rc = cx_upload(ctx, S->in2, marker, bytes, &marker_d))) return rc;
    const int64_t g0 = (n0 + CXR_T0 - 1) / CXR_T0, g1 = (n1 + CXR_T1 - 1) / CXR_T1, g2 = (n2 + CXR_T2 - 1) / CXR_T2;
    const size_t tiles = (size_t)g0 * (size_t)g1 * (size_t)g2;      // (<= 2^28: a tile holds eight samples at least, or the whole axis 0)
    void* final_out;
    if ((rc = S->open(ctx, out_device, out_bytes, &final_out))) return rc;
    if ((rc = S->state.grow(ctx, bytes))) return rc;
    if ((rc = S->work.grow(ctx, 4 * tiles))) return rc;
    if ((rc = S->counters.grow(ctx, sizeof(cxr_counters)))) return rc;
    cxr_args A;
    memset(&A, 0, sizeof(A));
    A.mask = mask_d; A.marker = marker_d; A.state = S->state.get(); A.out = final_out;
    A.list[0] = S->work.get(); A.list[1] = A.list[0] + tiles;
    A.flags[0] = A.list[1] + tiles; A.flags[1] = A.flags[0] + tiles;
    A.C = S->counters.as<cxr_counters>();
    A.n[0] = n0; A.n[1] = n1; A.n[2] = n2;
    A.g[0] = (uint32_t)g0; A.g[1] = (uint32_t)g1; A.g[2] = (uint32_t)g2; A.tiles = (uint32_t)tiles;
    A.dtype = dtype; A.kind = marker_kind; A.conn = connectivity; A.erosion = method == CX_RECON_EROSION ? 1 : 0; A.out_kind = out_kind;
    A.faces = (uint32_t)faces; A.h = h; A.h_int = (uint32_t)(h < 65536.0 ? h : 65536.0);
    CX_HIP(ctx, hipMemsetAsync(S->counters, 0, sizeof(cxr_counters), st));
    CX_HIP(ctx, hipMemsetAsync(A.flags[0], 0, 2 * tiles * sizeof(uint32_t), st));
    const uint32_t pass_blocks = (uint32_t)((total + 255u) / 256u < CXR_INIT_GRID ? (total + 255u) / 256u : CXR_INIT_GRID);
    {
        const dim3 grid(pass_blocks);
        CXR_BY_WIDTH(esize, cxr_launch_init);
        CX_HIP(ctx, hipGetLastError());
    }
    // the rounds: CXR_BATCH launches, then one look at the counters.  Launches behind the last round that listed a tile find an empty list
    const unsigned long long bound = (unsigned long long)total + 8ull;
    cxr_counters hc;
    for (unsigned long long r = 0;;) {
        for (uint32_t j = 0; j < CXR_BATCH; j++, r++) {
            A.round = (uint32_t)(r % 6ull);      // (the kernel looks at the round modulo 2 and modulo 3)
            A.first = r == 0 ? 1u : 0u;
            const dim3 grid((uint32_t)(r == 0 ? tiles : (tiles < CXR_GRID ? tiles : CXR_GRID)));
            CXR_BY_WIDTH(esize, cxr_launch_round);
            CX_HIP(ctx, hipGetLastError());
        }
        CX_HIP(ctx, hipMemcpyAsync(&hc, S->counters, sizeof(hc), hipMemcpyDeviceToHost, st));
        CX_HIP(ctx, hipStreamSynchronize(st));
        if (hc.cnt[r % 3ull] == 0u) break;
        if (r >= bound) return cx_fail(ctx, CX_ERR_HIP, "cx_grid_reconstruct3d: tiles still active after as many rounds as the array has samples");
    }
    A.all_ones = (marker_kind == CX_RECON_MARKER_STEP && out_kind == CX_RECON_OUT_CHANGED && !is_float && hc.n_moved == 0ull) ? 1u : 0u;
    {
        const dim3 grid(pass_blocks);
        CXR_BY_WIDTH(esize, cxr_launch_final);
        CX_HIP(ctx, hipGetLastError());
    }
    CX_HIP(ctx, hipMemcpyAsync(&hc, S->counters, sizeof(hc), hipMemcpyDeviceToHost, st));
    if (out_host) CX_HIP(ctx, hipMemcpyAsync(out_host, final_out, out_bytes, hipMemcpyDeviceToHost, st));
    CX_HIP(ctx, hipStreamSynchronize(st));      // the caller's host memory is its own again
    if (stats) {
        stats->n_changed = (int64_t)hc.n_changed; stats->n_clamped = (int64_t)hc.n_clamped;
        stats->rounds = (int64_t)hc.rounds; stats->tile_visits = (int64_t)hc.visits;
    }
    if (!out_device) { S->publish(n0, n1, n2); S->dtype = out_kind == CX_RECON_OUT_VALUES ? dtype : CX_DTYPE_U8; S->out_kind = out_kind; }
    return CX_OK;
}

extern "C" int cx_grid_reconstruct3d_result(cx_ctx* ctx, void** out_device, int64_t out_shape[3], int32_t* out_dtype, int32_t* out_kind) {
    if (!ctx) return CX_ERR_INVALID;
    const cx_recon_state* S = ctx->recon;
    const int rc = cx_slot_result(ctx, S, "cx_grid_reconstruct3d_result: no result of cx_grid_reconstruct3d in the context", out_device, out_shape);
    if (rc) return rc;
    if (out_dtype) *out_dtype = S->dtype;
    if (out_kind) *out_kind = S->out_kind;
    return CX_OK;
}

extern "C" int cx_grid_reconstruct3d_bind(cx_ctx* ctx) {
    if (!ctx) return CX_ERR_INVALID;
    cx_recon_state* S = ctx->recon;
    return cx_slot_bind(ctx, S, "cx_grid_reconstruct3d_bind: no result of cx_grid_reconstruct3d in the context", S ? S->dtype : 0);
}
