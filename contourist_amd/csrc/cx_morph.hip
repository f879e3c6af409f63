// cx_morph.hip -- morph triangles of a 4-D extraction, their sort by start time, and the per-t isosurface stream:
// cx_morph_triangles, cx_morph_download, cx_morph_eval*.
//
// Reference semantics restated (paths relative to the reference checkout, contourist/...), 4-D rows B4 / B5: morph triangles
//   GridContour4D.collect_morph_triangles                     pentatopes.py:314-368
//   MorphGeometry.triangulate_tetrahedron_at_midpoints / add_tetrahedron / interpolate_pair_3d
//                                                             morph_geometry.py:145-237
//   MorphTriangles.__init__ / orient_triangles / compute_triangle_stats / time_compatible_triangles
//                                                             morph_geometry.py:7-22, 49-89
// Canonical numbering: the 4 vertices of a tetrahedron are ordered by edge id (the reference orders them by
// its dict numbering, which only decides how a 4-segment slice is split).
// Row B6, the surfaces at given times (misc/morph_triangles.js:26-140; MorphTriangles.triangles_at), is the last section of the file.
// The orientation of the triangles is the component orientation of the 3-D post-pass (cxp_orient_pick / cxp_orient_decide, cx_post.h).
#include <algorithm>
#include <cstring>
#include <vector>

#include "cx_post.h"
#include "cx_state4.h"

// (grid-stride, reduced per wave before the two read-before-atomic updates: one thread per point with its own pair of updates took
// 0.28 ms for 4.7 M points -- the first waves all raise the maximum)
__global__ __launch_bounds__(256) void cxp_k_minmax_t(const double* pts, uint32_t nv, u64* mm) {
    u64 lo = ~0ULL, hi = 0ULL;
    for (uint32_t v = blockIdx.x * 256u + threadIdx.x; v < nv; v += gridDim.x * 256u) {
        const u64 o = cxd_orderable(pts[(size_t)v * 4 + 3]);
        lo = o < lo ? o : lo;
        hi = o > hi ? o : hi;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 l2 = ((u64)(uint32_t)__shfl_xor((int)(uint32_t)(lo >> 32), o) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)lo, o);
        const u64 h2 = ((u64)(uint32_t)__shfl_xor((int)(uint32_t)(hi >> 32), o) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)hi, o);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if ((threadIdx.x & 63u) == 0u) {
        cxd_min64(&mm[0], lo);
        cxd_max64(&mm[1], hi);
    }
}

// slices of one tetrahedron: calls emit(p0, p1, p2) with vertex-index pairs packed (i << 32 | j), i before j in
// canonical order; returns the number of triangles
template <typename Emit>
__device__ __forceinline__ uint32_t cxp_morph_slices(const int32_t* tets, uint32_t t, const double* pts, const uint32_t* prio, double t_eps,
                                                     Emit emit) {
    uint32_t v[4];
    double tv[4];
#pragma unroll
    for (int s = 0; s < 4; s++) v[s] = (uint32_t)tets[(size_t)t * 4 + s];
    // (a,b,c,d) = vertices in ascending priority (sorting network); the stored order is positively oriented
    // (cxp_k_tets_orient), tsign = orientation of (a,b,c,d)
    double tsign = 1.0;
#define CXP_CSWAP(x, y) if (prio[v[x]] > prio[v[y]]) { const uint32_t tmp = v[x]; v[x] = v[y]; v[y] = tmp; tsign = -tsign; }
    CXP_CSWAP(0, 1) CXP_CSWAP(2, 3) CXP_CSWAP(0, 2) CXP_CSWAP(1, 3) CXP_CSWAP(1, 2)
#undef CXP_CSWAP
#pragma unroll
    for (int s = 0; s < 4; s++) tv[s] = pts[(size_t)v[s] * 4 + 3];
    double ts[4] = {tv[0], tv[1], tv[2], tv[3]};
#define CXP_DSWAP(x, y) if (ts[x] > ts[y]) { const double tmp = ts[x]; ts[x] = ts[y]; ts[y] = tmp; }
    CXP_DSWAP(0, 1) CXP_DSWAP(2, 3) CXP_DSWAP(0, 2) CXP_DSWAP(1, 3) CXP_DSWAP(1, 2)
#undef CXP_DSWAP
    // Everything below lives in named scalars, one set per edge, and the crossed edges are picked by select chains from a 6-bit set: with
    // small arrays indexed by a running count `m` (or by select chains over array elements, which the compiler folds back into an indexed
    // load) the arrays went to scratch memory -- 160 bytes per lane, 108 registers, 4 waves per SIMD, cxp_k_morph_emit 1.65 ms on config 4.
    // Same arithmetic, same order of the edges: scan order (a,b)(a,c)(a,d)(b,c)(b,d)(c,d) = edges 0..5.
    uint32_t n = 0;
    const double wx = tv[1] - tv[0], wy = tv[2] - tv[0], wz = tv[3] - tv[0];
#define CXP_EDGE(e, I, J)                                                                                                   \
    const bool cross##e = !(mid + 1e-5 < fmin(tv[I], tv[J]) || mid - 1e-5 > fmax(tv[I], tv[J])); /* morph_geometry.py:218 */ \
    const u64 sp##e = ((u64)v[I] << 32) | (u64)v[J];                                                                         \
    const bool zero##e = fabs(tv[I] - tv[J]) <= t_eps;                                           /* pentatopes.py:341-345 */  \
    const double den##e = tv[J] - tv[I];                                                                                     \
    const double lam##e = (den##e != 0.0) ? fmin(1.0, fmax(0.0, (mid - tv[I]) / den##e)) : 0.5;                              \
    const double px##e = ((I) == 1 ? 1.0 : 0.0) + lam##e * (((J) == 1 ? 1.0 : 0.0) - ((I) == 1 ? 1.0 : 0.0));                \
    const double py##e = ((I) == 2 ? 1.0 : 0.0) + lam##e * (((J) == 2 ? 1.0 : 0.0) - ((I) == 2 ? 1.0 : 0.0));                \
    const double pz##e = ((I) == 3 ? 1.0 : 0.0) + lam##e * (((J) == 3 ? 1.0 : 0.0) - ((I) == 3 ? 1.0 : 0.0));
#define CXP_PICK(name, k) ((k) == 5 ? name##5 : (k) == 4 ? name##4 : (k) == 3 ? name##3 : (k) == 2 ? name##2 : (k) == 1 ? name##1 : name##0)
#pragma unroll
    for (int g = 0; g < 3; g++) {
        if (!((ts[g + 1] - ts[g]) > 1e-4)) continue;               // morph_geometry.py:150
        const double mid = 0.5 * (ts[g + 1] + ts[g]);
        // the slice points in the tetrahedron's own affine frame: a = 0, b = e1, c = e2, d = e3
        CXP_EDGE(0, 0, 1) CXP_EDGE(1, 0, 2) CXP_EDGE(2, 0, 3) CXP_EDGE(3, 1, 2) CXP_EDGE(4, 1, 3) CXP_EDGE(5, 2, 3)
        const uint32_t cm = (cross0 ? 1u : 0u) | (cross1 ? 2u : 0u) | (cross2 ? 4u : 0u) | (cross3 ? 8u : 0u) | (cross4 ? 16u : 0u) | (cross5 ? 32u : 0u);
        // winding: all tetrahedra are oriented alike with respect to the field gradient, so the slice triangle whose
        // normal (inside the tetrahedron) points towards later times is wound alike everywhere -- a rule on the
        // order of the vertex times only, which bin_times and the tiny collapse do not disturb
        auto wound = [&](int i0, int i1, int i2) {
            const double x0 = CXP_PICK(px, i0), y0 = CXP_PICK(py, i0), z0 = CXP_PICK(pz, i0);
            const double ax = CXP_PICK(px, i1) - x0, ay = CXP_PICK(py, i1) - y0, az = CXP_PICK(pz, i1) - z0;
            const double bx = CXP_PICK(px, i2) - x0, by = CXP_PICK(py, i2) - y0, bz = CXP_PICK(pz, i2) - z0;
            const double det = (ay * bz - az * by) * wx + (az * bx - ax * bz) * wy + (ax * by - ay * bx) * wz;
            const u64 s0 = CXP_PICK(sp, i0), s1 = CXP_PICK(sp, i1), s2 = CXP_PICK(sp, i2);
            if (det * tsign >= 0.0) emit(s0, s1, s2); else emit(s0, s2, s1);
        };
        const int m = __popc(cm);
        const int e0 = (int)__ffs(cm) - 1;                          // the first crossed edge in scan order
        if (m == 3) {
            const uint32_t c1 = cm & (cm - 1u), c2 = c1 & (c1 - 1u);
            const int e1 = (int)__ffs(c1) - 1, e2 = (int)__ffs(c2) - 1;
            if (!(CXP_PICK(zero, e0) || CXP_PICK(zero, e1) || CXP_PICK(zero, e2))) { wound(e0, e1, e2); n++; }
        } else if (m == 4) {                                       // morph_geometry.py:176-186
            // p2 = the crossed edge without a vertex in common with the first one (the last such one in scan order)
            const u64 s0 = CXP_PICK(sp, e0);
            const uint32_t a0 = (uint32_t)(s0 >> 32), a1 = (uint32_t)s0;
            int p2 = -1;
#define CXP_DISJ(e)                                                                                          \
            {                                                                                                \
                const uint32_t b0 = (uint32_t)(sp##e >> 32), b1 = (uint32_t)sp##e;                            \
                if (cross##e && e != e0 && a0 != b0 && a0 != b1 && a1 != b0 && a1 != b1) p2 = e;             \
            }
            CXP_DISJ(0) CXP_DISJ(1) CXP_DISJ(2) CXP_DISJ(3) CXP_DISJ(4) CXP_DISJ(5)
#undef CXP_DISJ
            if (p2 >= 0) {
                const bool z02 = CXP_PICK(zero, e0) || CXP_PICK(zero, p2);
#define CXP_THIRD(e) if (cross##e && e != e0 && e != p2 && !(z02 || zero##e)) { wound(e0, p2, e); n++; }
                CXP_THIRD(0) CXP_THIRD(1) CXP_THIRD(2) CXP_THIRD(3) CXP_THIRD(4) CXP_THIRD(5)
#undef CXP_THIRD
            }
        }
    }
#undef CXP_EDGE
#undef CXP_PICK
    return n;
}

// Every tetrahedron of the 4-D march lies in the level set of the linear interpolant of ONE pentatope (Kuhn simplex
// of its hypercube, pentatopes.py:15-26).  Its four indices are put in the order that makes
// det[p1-p0, p2-p0, p3-p0, gradient] positive, with the points as the march interpolated them (before bin_times) and
// the gradient of that interpolant: along the axis added at step i of the pentatope's lattice path it is the
// difference of the two consecutive corner samples; the pentatope is the one whose path adds the axes in the order of
// decreasing fractional coordinate of the tetrahedron's centroid.
struct cxp_grid4 {
    const float* A;
    int n[4];
    double value;
};
__device__ __forceinline__ void cxp_crossing4(const cxp_grid4& G, uint32_t key, double x[4]) {
    const uint32_t lin = key >> 4, d = key & 15u;
    const uint32_t s3 = (uint32_t)G.n[3], s2 = s3 * (uint32_t)G.n[2], s1 = s2 * (uint32_t)G.n[1];
    uint32_t q[4];
    q[0] = lin / s1;
    uint32_t r = lin - q[0] * s1;
    q[1] = r / s2;
    r -= q[1] * s2;
    q[2] = r / s3;
    q[3] = r - q[2] * s3;
    const uint32_t lin2 = lin + ((d & 8u) ? s1 : 0u) + ((d & 4u) ? s2 : 0u) + ((d & 2u) ? s3 : 0u) + (d & 1u);
    const double f0 = (double)G.A[lin], f1 = (double)G.A[lin2];
    const bool owner_low = !(f0 > f1);
    const double flow = owner_low ? f0 : f1, fhigh = owner_low ? f1 : f0;
    double ratio = 0.5;
    const double den = 1.0 * (fhigh - flow);
    if (!(fabs(den) <= 1e-8)) ratio = (G.value - flow) / den;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const double db = (double)((d >> (3 - a)) & 1u);
        const double low = owner_low ? (double)q[a] : (double)q[a] + db, high = owner_low ? (double)q[a] + db : (double)q[a];
        x[a] = low + ratio * (high - low);
    }
}
__global__ void cxp_k_tets_orient(int32_t* tets, uint32_t nt, const uint32_t* keys, cxp_grid4 G) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    double p[4][4], c[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        cxp_crossing4(G, keys[(uint32_t)tets[(size_t)t * 4 + k]], p[k]);
#pragma unroll
        for (int a = 0; a < 4; a++) c[a] += 0.25 * p[k][a];
    }
    int base[4], ord[4] = {0, 1, 2, 3};
    double frac[4];
#pragma unroll
    for (int a = 0; a < 4; a++) {
        int i0 = (int)floor(c[a]);
        i0 = max(0, min(i0, G.n[a] - 2));
        base[a] = i0;
        frac[a] = c[a] - (double)i0;
    }
#pragma unroll
    for (int i = 1; i < 4; i++)
#pragma unroll
        for (int j = i; j > 0; j--)
            if (frac[ord[j]] > frac[ord[j - 1]]) { const int x = ord[j]; ord[j] = ord[j - 1]; ord[j - 1] = x; }
    int q[4] = {base[0], base[1], base[2], base[3]};
    const size_t s3 = (size_t)G.n[3], s2 = s3 * (size_t)G.n[2], s1 = s2 * (size_t)G.n[1];
    double prev = (double)G.A[q[0] * s1 + q[1] * s2 + q[2] * s3 + q[3]], g[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        q[ord[i]] += 1;
        const double cur = (double)G.A[q[0] * s1 + q[1] * s2 + q[2] * s3 + q[3]];
        g[ord[i]] = cur - prev;
        prev = cur;
    }
    // det of the rows (p1-p0, p2-p0, p3-p0, g), expanded along the last row
    double m[3][4];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int a = 0; a < 4; a++) m[k][a] = p[k + 1][a] - p[0][a];
    auto det3 = [&](int a, int b, int cc) {
        return m[0][a] * (m[1][b] * m[2][cc] - m[1][cc] * m[2][b]) - m[0][b] * (m[1][a] * m[2][cc] - m[1][cc] * m[2][a]) +
               m[0][cc] * (m[1][a] * m[2][b] - m[1][b] * m[2][a]);
    };
    const double det = -g[0] * det3(1, 2, 3) + g[1] * det3(0, 2, 3) - g[2] * det3(0, 1, 3) + g[3] * det3(0, 1, 2);
    if (det < 0.0) {
        const int32_t x = tets[(size_t)t * 4 + 2];
        tets[(size_t)t * 4 + 2] = tets[(size_t)t * 4 + 3];
        tets[(size_t)t * 4 + 3] = x;
    }
}
__global__ void cxp_k_morph_count(const int32_t* tets, uint32_t nt, const double* pts, const uint32_t* prio, const u64* mm, uint32_t* counts) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const double t_eps = 1e-7 * (cxd_from_orderable(mm[1]) - cxd_from_orderable(mm[0]));
    counts[t] = cxp_morph_slices(tets, t, pts, prio, t_eps, [](u64, u64, u64) {});
}
// (Measured and dropped: the workgroup's triangles put together in LDS and written out as consecutive words -- 0.81 -> 0.83 ms: the kernel is
// bound by its arithmetic and gathers at 128 registers, not by its stores.)
__global__ void cxp_k_morph_emit(const int32_t* tets, uint32_t nt, const double* pts, const uint32_t* prio, const u64* mm,
                                 const uint32_t* offsets, u64* pairs) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const double t_eps = 1e-7 * (cxd_from_orderable(mm[1]) - cxd_from_orderable(mm[0]));
    u64* out = pairs + (size_t)offsets[t] * 3;
    cxp_morph_slices(tets, t, pts, prio, t_eps, [&](u64 p0, u64 p1, u64 p2) { out[0] = p0; out[1] = p1; out[2] = p2; out += 3; });
}
// segments = distinct vertex pairs
// (slots by the first vertex of the pair, as in the 3-D edge table: vertex ids follow the march, so the triangles of a wave
// probe neighbouring lines; segment ids = slot order then follow the vertices too, which carries on into the edge table)
// A workgroup takes 1024 consecutive keys (the three pairs of ~340 neighbouring triangles: every segment shows up several times
// among them) and puts them through a set in LDS first; only the first of each key in the block goes on to the device-scope table,
// whose reads and compare-and-swaps are executed at the memory side of the fabric and bound this kernel.
#define CXP_SEG_KEYS 1024u
#define CXP_SEG_SLOTS 2048u
__global__ __launch_bounds__(256) void cxp_k_seg_insert(const u64* pairs, size_t n, u64* tkeys, u64 mask, u64 mult) {
    __shared__ u64 lset[CXP_SEG_SLOTS];
    for (uint32_t x = threadIdx.x; x < CXP_SEG_SLOTS; x += 256u) lset[x] = CXD_EMPTY;
    __syncthreads();
    const size_t b0 = (size_t)blockIdx.x * CXP_SEG_KEYS;
    u64 key[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        const size_t i = b0 + k * 256u + threadIdx.x;
        key[k] = (i < n) ? pairs[i] : CXD_EMPTY;
    }
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        if (key[k] == CXD_EMPTY) continue;
        uint32_t ls = (uint32_t)cxd_mix(key[k]) & (CXP_SEG_SLOTS - 1u);
        bool first = false;
        for (uint32_t probes = 0; probes < CXP_SEG_SLOTS; probes++) {      // (ends earlier: 1024 keys, 2048 slots)
            const u64 cur = atomicCAS((unsigned long long*)&lset[ls], (unsigned long long)CXD_EMPTY, (unsigned long long)key[k]);
            if (cur == CXD_EMPTY) { first = true; break; }
            if (cur == key[k]) break;
            ls = (ls + 1u) & (CXP_SEG_SLOTS - 1u);
        }
        if (!first) continue;
        u64 slot = cxp_edge_slot((uint32_t)(key[k] >> 32), (uint32_t)key[k], mask, mult);
        for (;;) {
            u64 cur = __hip_atomic_load(&tkeys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (see cxp_k_edge_lists)
            if (cur == CXD_EMPTY) cur = atomicCAS(&tkeys[slot], CXD_EMPTY, key[k]);
            if (cur == CXD_EMPTY || cur == key[k]) break;
            slot = (slot + 1) & mask;
        }
    }
}
// Segment ids = rank of the occupied slot, by ordered compaction without a flag or id word per SLOT (the table has 134 M slots on config 4
// for 12 M segments: flags + a full scan + ids for every slot were 1.5 GB written and 2 GB read, ~1 ms): a workgroup counts the occupied
// slots of its 4 096 (cxp_k_occ_count), one workgroup scans the block counts (cxp_k_scan_sums), and cxp_k_seg_write4 redoes the scan inside
// its block, lists the occupied slots in LDS and writes one record per list entry -- ids[slot] only for occupied slots (what
// cxp_k_tri_segments looks up), segments / midpoints / time ranges in id order, next to each other.
#define CXP_OCC_BLOCK 4096u
__device__ __forceinline__ uint32_t cxp_occ16(const u64* tkeys, size_t base, size_t n) {
    uint32_t m = 0;
    if (base + 16u <= n) {
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            const ulonglong2 w = *reinterpret_cast<const ulonglong2*>(tkeys + base + 2u * k);
            m |= (w.x != CXD_EMPTY ? 1u : 0u) << (2u * k);
            m |= (w.y != CXD_EMPTY ? 2u : 0u) << (2u * k);
        }
    } else {
        for (uint32_t k = 0; k < 16u && base + k < n; k++) m |= (tkeys[base + k] != CXD_EMPTY ? 1u : 0u) << k;
    }
    return m;
}
__global__ __launch_bounds__(256) void cxp_k_occ_count(const u64* tkeys, size_t n, uint32_t* count) {
    __shared__ uint32_t s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    uint32_t c = __popc(cxp_occ16(tkeys, (size_t)blockIdx.x * CXP_OCC_BLOCK + threadIdx.x * 16u, n));
    c = cxd_wave_add(c);
    if ((threadIdx.x & 63u) == 0 && c) atomicAdd(&s_n, c);
    __syncthreads();
    if (threadIdx.x == 0) count[blockIdx.x] = s_n;
}
__global__ __launch_bounds__(256) void cxp_k_seg_write4(const u64* tkeys, size_t n, const uint32_t* boff, const uint32_t* total, uint32_t nblocks,
                                                        const double* pts, uint32_t* ids, int32_t* segs, double* mid, double* stime) {
    __shared__ uint32_t s[256];
    __shared__ uint16_t list[CXP_OCC_BLOCK];
    const uint32_t first = boff[blockIdx.x];
    const uint32_t next = (blockIdx.x + 1u < nblocks) ? boff[blockIdx.x + 1u] : *total;
    if (next == first) return;
    const size_t base = (size_t)blockIdx.x * CXP_OCC_BLOCK;
    uint32_t m = cxp_occ16(tkeys, base + threadIdx.x * 16u, n);
    // exclusive prefix of the threads' counts (Hillis-Steele over 256), then the positions of the set bits
    const uint32_t cnt = __popc(m);
    s[threadIdx.x] = cnt;
    __syncthreads();
    for (uint32_t o = 1; o < 256; o <<= 1) {
        const uint32_t x = (threadIdx.x >= o) ? s[threadIdx.x - o] : 0u;
        __syncthreads();
        s[threadIdx.x] += x;
        __syncthreads();
    }
    uint32_t pos = s[threadIdx.x] - cnt;
    const uint32_t nl = s[255];
    while (m) {
        const uint32_t k = __ffs(m) - 1u;
        m &= m - 1u;
        list[pos++] = (uint16_t)(threadIdx.x * 16u + k);
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < nl; j += 256u) {
        const size_t slot = base + list[j];
        const u64 key = tkeys[slot];
        const uint32_t a = (uint32_t)(key >> 32), b = (uint32_t)key;
        const double4 pa = *reinterpret_cast<const double4*>(pts + (size_t)a * 4);
        const double4 pb = *reinterpret_cast<const double4*>(pts + (size_t)b * 4);
        const uint32_t sg = first + j;
        ids[slot] = sg;
        const bool swap = pa.w > pb.w;
        segs[(size_t)sg * 2] = (int32_t)(swap ? b : a); segs[(size_t)sg * 2 + 1] = (int32_t)(swap ? a : b);
        mid[(size_t)sg * 3] = swap ? 0.5 * (pb.x + pa.x) : 0.5 * (pa.x + pb.x);
        mid[(size_t)sg * 3 + 1] = swap ? 0.5 * (pb.y + pa.y) : 0.5 * (pa.y + pb.y);
        mid[(size_t)sg * 3 + 2] = swap ? 0.5 * (pb.z + pa.z) : 0.5 * (pa.z + pb.z);
        stime[(size_t)sg * 2] = swap ? pb.w : pa.w; stime[(size_t)sg * 2 + 1] = swap ? pa.w : pb.w;
    }
}
// triangles as segment-id triples + their time range (morph_geometry.py:69-89)
__global__ void cxp_k_tri_segments(const u64* pairs, uint32_t nt, const u64* tkeys, const uint32_t* ids, u64 mask, u64 mult, const double* stime,
                                   const u64* mm, int32_t* tris, double* ttime) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    double lo = cxd_from_orderable(mm[0]), hi = cxd_from_orderable(mm[1]);
    // the three keys, their three probes side by side, the three ids, the six times -- and only then the stores (one edge after the
    // other with its store at the end of each round, every load of the next round waited for that store: they may alias for all the
    // compiler knows)
    const u64 key[3] = {pairs[(size_t)t * 3], pairs[(size_t)t * 3 + 1], pairs[(size_t)t * 3 + 2]};
    u64 slot[3];
#pragma unroll
    for (int e = 0; e < 3; e++) slot[e] = cxp_edge_slot((uint32_t)(key[e] >> 32), (uint32_t)key[e], mask, mult);
    for (;;) {
        const u64 k0 = tkeys[slot[0]], k1 = tkeys[slot[1]], k2 = tkeys[slot[2]];
        const bool m0 = k0 == key[0], m1 = k1 == key[1], m2 = k2 == key[2];
        if (m0 && m1 && m2) break;
        if (!m0) slot[0] = (slot[0] + 1) & mask;
        if (!m1) slot[1] = (slot[1] + 1) & mask;
        if (!m2) slot[2] = (slot[2] + 1) & mask;
    }
    const uint32_t s0 = ids[slot[0]], s1 = ids[slot[1]], s2 = ids[slot[2]];
    const double a0 = stime[(size_t)s0 * 2], b0 = stime[(size_t)s0 * 2 + 1], a1 = stime[(size_t)s1 * 2], b1 = stime[(size_t)s1 * 2 + 1];
    const double a2 = stime[(size_t)s2 * 2], b2 = stime[(size_t)s2 * 2 + 1];
    lo = fmax(fmax(lo, a0), fmax(a1, a2));
    hi = fmin(fmin(hi, b0), fmin(b1, b2));
    tris[(size_t)t * 3] = (int32_t)s0; tris[(size_t)t * 3 + 1] = (int32_t)s1; tris[(size_t)t * 3 + 2] = (int32_t)s2;
    ttime[(size_t)t * 2] = lo; ttime[(size_t)t * 2 + 1] = hi;
}
// edge table with a linked list of the triangles on each edge (an "edge" = pair of segment ids).  A workgroup takes CXP_EL consecutive
// triangles: their visits of one edge are chained in LDS first (a table of keys with a head per slot, one LDS exchange per visit), and
// only the block's FIRST visitor of an edge -- the tail of that chain -- goes to the device-scope table: it finds or claims the key,
// swaps the block's local head in as the edge's new head and hangs the old head behind itself.  One device-scope exchange per (edge,
// block) instead of one per visit (triangle ids follow the march: most of an edge's triangles sit in one block); the reads and
// read-modify-writes at the memory side of the fabric are what this stage is bound by.  The order inside a list is of no consequence
// (cxp_k_edge_union_compat looks at every pair).  Measured and dropped (third session of round 4): key and head of a slot next to each other
// in ONE table (one line per probe, as the 3-D edge table has it) -- 2.99 -> 3.22 ms on config 4.
#define CXP_EL 512u
#define CXP_EL_PER (CXP_EL / 256u)
#define CXP_EL_SLOTS (4u * CXP_EL)
__global__ __launch_bounds__(256) void cxp_k_edge_lists(const int32_t* tri, uint32_t nt, u64* ekeys, u64* eheads, u64 mask, u64 mult, uint32_t* next) {
    __shared__ u64 lkey[CXP_EL_SLOTS];
    __shared__ uint32_t lhead[CXP_EL_SLOTS];
    for (uint32_t x = threadIdx.x; x < CXP_EL_SLOTS; x += 256u) { lkey[x] = CXD_EMPTY; lhead[x] = CXD_NONE; }
    __syncthreads();
    const uint32_t b0 = blockIdx.x * CXP_EL;
    u64 key_[CXP_EL_PER][3];
    uint16_t slot_[CXP_EL_PER][3];
    uint32_t tails = 0;       // bit 3 i + e: this visit is the block's first of its edge
#pragma unroll
    for (uint32_t i = 0; i < CXP_EL_PER; i++) {
        const uint32_t t = b0 + i * 256u + threadIdx.x;
        if (t >= nt) continue;
        const uint32_t v[3] = {(uint32_t)tri[(size_t)t * 3], (uint32_t)tri[(size_t)t * 3 + 1], (uint32_t)tri[(size_t)t * 3 + 2]};
#pragma unroll
        for (int e = 0; e < 3; e++) {
            const uint32_t p = v[e], q = v[(e + 1) % 3];
            const u64 key = ((u64)min(p, q) << 32) | (u64)max(p, q);
            key_[i][e] = key;
            uint32_t ls = (uint32_t)cxd_mix(key) & (CXP_EL_SLOTS - 1u);
            for (uint32_t probes = 0; probes < CXP_EL_SLOTS; probes++) {      // (ends earlier: 3 CXP_EL visits, 4 CXP_EL slots)
                const u64 cur = atomicCAS((unsigned long long*)&lkey[ls], (unsigned long long)CXD_EMPTY, (unsigned long long)key);
                if (cur == CXD_EMPTY || cur == key) break;
                ls = (ls + 1u) & (CXP_EL_SLOTS - 1u);
            }
            slot_[i][e] = (uint16_t)ls;
            const uint32_t me = t * 3u + (uint32_t)e;
            const uint32_t prev = atomicExch(&lhead[ls], me);
            if (prev == CXD_NONE) tails |= 1u << (3u * i + (uint32_t)e);
            else next[me] = prev;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t i = 0; i < CXP_EL_PER; i++) {
        const uint32_t t = b0 + i * 256u + threadIdx.x;
        if (t >= nt) continue;
#pragma unroll
        for (int e = 0; e < 3; e++) {
            if (!((tails >> (3u * i + (uint32_t)e)) & 1u)) continue;
            const u64 key = key_[i][e];
            u64 slot = cxp_edge_slot((uint32_t)(key >> 32), (uint32_t)key, mask, mult);
            for (;;) {
                // device-scope read first: every visitor of an edge but the first finds the key there and needs no read-modify-write
                u64 cur = __hip_atomic_load(&ekeys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (cur == CXD_EMPTY) cur = atomicCAS(&ekeys[slot], CXD_EMPTY, key);
                if (cur == CXD_EMPTY || cur == key) break;
                slot = (slot + 1) & mask;
            }
            const u64 old = atomicExch(&eheads[slot], (u64)lhead[slot_[i][e]]);      // the block's chain in front of what was there
            next[t * 3u + (uint32_t)e] = (old == CXD_EMPTY) ? CXD_NONE : (uint32_t)old;
        }
    }
}
// link every pair of time-compatible triangles on a common edge (morph_geometry.py:61-67, surface_geometry.py:117-128).
// Every visit walks the REST of its edge's list -- from the node behind its own to the end -- so each pair of nodes is looked at
// once, by the one nearer the head; no visit has to find the edge's slot in the table again.  (Until round 3 every visit probed the
// table for its edge and walked the whole list from the head, keeping the triangles with a smaller id: a random table read per
// visit and twice the hops.)
__global__ void cxp_k_edge_union_compat(uint32_t nt, const uint32_t* next, const double* ttime, u64* parent) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const double lo = ttime[(size_t)t * 2], hi = ttime[(size_t)t * 2 + 1];
    uint32_t it[3] = {next[t * 3u], next[t * 3u + 1u], next[t * 3u + 2u]};      // the three walks side by side
    while (it[0] != CXD_NONE || it[1] != CXD_NONE || it[2] != CXD_NONE) {
#pragma unroll
        for (int e = 0; e < 3; e++) {
            if (it[e] == CXD_NONE) continue;
            const uint32_t o = it[e] / 3u;
            const double l2 = fmax(lo, ttime[(size_t)o * 2]), h2 = fmin(hi, ttime[(size_t)o * 2 + 1]);
            it[e] = next[it[e]];
            if (l2 < h2 && o != t) cxp_union0(parent, t, o);   // connectivity only: the slices are wound alike (cxp_morph_slices); path halving (cxp_find0)
        }
    }
}


static int cxp_morph_sort_by_start(cx_ctx* ctx, cx_post_state* S, uint32_t nseg, uint32_t ntri, const u64* mm_host);
extern "C" int cx_morph_triangles(cx_ctx* ctx, int64_t* out_counts) {
    if (!ctx) return CX_ERR_INVALID;
    cx_state4* G = ctx->s4;
    if (!cxp_tets4d(ctx)) { ctx->err = "cx_morph_triangles: run cx_postprocess4d first"; return CX_ERR_STATE; }
    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_post_state* S = ctx->post;
    hipStream_t st = ctx->stream;
    const uint32_t nv = (uint32_t)S->nv_out, nt = (uint32_t)S->nt_out;   // vertices / surviving tetrahedra
    const double* pts = S->pts.as<const double>();
    const uint32_t* prio = S->prio.as<const uint32_t>();
    const int32_t* tets = S->tri_out.as<const int32_t>();
    uint32_t* misc = S->misc.as<uint32_t>();
    u64* mm = (u64*)(misc + CXP_M_MINMAX_T);
    int rc;
    int64_t counts[8] = {nv, 0, 0, 0, 0, 0, 0, 0};
    u64 h_mm[2] = {0, 0};      // min / max t of all points (MorphTriangles.min_value / max_value), orderable encodings
    S->ms_out = 0; S->mt_out = 0; S->msorted = false;
    if (nv && nt) {
        const u64 init[2] = {~0ULL, 0ULL};
        CX_HIP(ctx, hipMemcpyAsync(mm, init, sizeof(init), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(cxp_k_minmax_t, dim3(std::min(cx_blocks(nv), 2048u)), dim3(256), 0, st, pts, nv, mm);
        if ((rc = S->flags.grow(ctx, (size_t)(nt + 16) * sizeof(uint32_t)))) return rc;
        if ((rc = S->scan.grow(ctx, (size_t)(nt + 16) * sizeof(uint32_t)))) return rc;
        uint32_t* cnt = S->flags.as<uint32_t>();
        uint32_t* off = S->scan.as<uint32_t>();
        cxp_grid4 G4;
        G4.A = G->grid;
        for (int k = 0; k < 4; k++) G4.n[k] = (int)G->n[k];
        G4.value = G->value;
        // the march's table already emits every tetrahedron in that order (tools/gen_tables.py orient_tet: exact, and valid
        // where samples EQUAL the isovalue and the determinant below vanishes); CX_TETS_ORIENT=1 (debug) recomputes it from the data
        // (not on a slab assembly: its tetrahedra come from several grids, G->grid is only the last slab's)
        if (!G->post_assembled && cx_debug_knob("CX_TETS_ORIENT", 0))
            hipLaunchKernelGGL(cxp_k_tets_orient, dim3(cx_blocks(nt)), dim3(256), 0, st, S->tri_out.as<int32_t>(), nt, prio, G4);
        hipLaunchKernelGGL(cxp_k_morph_count, dim3(cx_blocks(nt)), dim3(256), 0, st, tets, nt, pts, prio, mm, cnt);
        if ((rc = cxp_scan(ctx, S, cnt, off, nt, misc + CXP_M_TOTAL0))) return rc;
        uint32_t ntri = 0;
        u64* h = h_mm;
        CX_HIP(ctx, hipMemcpyAsync(&ntri, misc + CXP_M_TOTAL0, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        CX_HIP(ctx, hipMemcpyAsync(h, mm, sizeof(h_mm), hipMemcpyDeviceToHost, st));
        CX_HIP(ctx, hipStreamSynchronize(st));
        S->me_off.clear();
        if (ntri) {
            if ((rc = S->mpairs.grow(ctx, (size_t)ntri * 3 * sizeof(u64)))) return rc;
            u64* pairs = S->mpairs.as<u64>();
            hipLaunchKernelGGL(cxp_k_morph_emit, dim3(cx_blocks(nt)), dim3(256), 0, st, tets, nt, pts, prio, mm, off, pairs);
            // ---- segments
            const size_t np = (size_t)ntri * 3;
            // (n keys of which a third or less are distinct -- every segment shows up in several triangles: the edge-table rule, 5/4 of the
            // bound, keeps the load below 0.8 in the worst case and near 0.25 here with half the slots to clear, flag and scan)
            const u64 ssz = cxp_edge_table_size(np);
            if ((rc = S->tkeys.grow(ctx, ssz * sizeof(u64)))) return rc;
            const uint32_t nob = cx_blocks(ssz, CXP_OCC_BLOCK);
            if ((rc = S->flags.grow(ctx, (size_t)(nob + 16) * sizeof(uint32_t)))) return rc;
            if ((rc = S->scan.grow(ctx, (size_t)(ssz + 16) * sizeof(uint32_t)))) return rc;
            u64* skeys = S->tkeys.as<u64>();
            uint32_t* boff = S->flags.as<uint32_t>();        // occupied slots per block of 4 096, then their exclusive scan
            uint32_t* sid = S->scan.as<uint32_t>();          // segment id per slot, written for occupied slots only
            cxp_fill64(st, skeys, (size_t)ssz, CXD_EMPTY);
            const u64 smult = std::max<u64>(1, ssz / std::max<u64>(1, (u64)nv));
            hipLaunchKernelGGL(cxp_k_seg_insert, dim3(cx_blocks(np, CXP_SEG_KEYS)), dim3(256), 0, st, pairs, np, skeys, ssz - 1, smult);
            hipLaunchKernelGGL(cxp_k_occ_count, dim3(nob), dim3(256), 0, st, (const u64*)skeys, (size_t)ssz, boff);
            cxp_scan_sums(st, boff, nob, misc + CXP_M_TOTAL1);
            uint32_t nseg = 0;
            CX_HIP(ctx, hipMemcpyAsync(&nseg, misc + CXP_M_TOTAL1, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            CX_HIP(ctx, hipStreamSynchronize(st));
            if ((rc = S->msegs.grow(ctx, (size_t)(nseg + 1) * 2 * sizeof(int32_t)))) return rc;
            if ((rc = S->mmid.grow(ctx, (size_t)(nseg + 1) * 3 * sizeof(double)))) return rc;
            if ((rc = S->mtime.grow(ctx, ((size_t)(nseg + 1) * 2 + (size_t)(ntri + 1) * 2) * sizeof(double)))) return rc;
            if ((rc = S->mtris.grow(ctx, (size_t)(ntri + 1) * 3 * sizeof(int32_t)))) return rc;
            int32_t* segs = S->msegs.as<int32_t>();
            double* mid = S->mmid.as<double>();
            double* stime = S->mtime.as<double>();
            double* ttime = stime + (size_t)(nseg + 1) * 2;
            int32_t* tris = S->mtris.as<int32_t>();
            hipLaunchKernelGGL(cxp_k_seg_write4, dim3(nob), dim3(256), 0, st, (const u64*)skeys, (size_t)ssz, (const uint32_t*)boff, (const uint32_t*)(misc + CXP_M_TOTAL1), nob,
                               pts, sid, segs, mid, stime);
            hipLaunchKernelGGL(cxp_k_tri_segments, dim3(cx_blocks(ntri)), dim3(256), 0, st, pairs, ntri, skeys, sid, ssz - 1, smult, stime, mm, tris, ttime);
            CX_HIP(ctx, hipStreamSynchronize(st));   // the segment table is reused below
            // ---- orientation on the segment midpoints, time-compatible neighbours only
            const u64 esz = cxp_edge_table_size((size_t)ntri * 3);
            const u64 emult4 = std::max<u64>(1, esz / std::max<u64>(1, (u64)nseg));
            if ((rc = S->tkeys.grow(ctx, esz * sizeof(u64)))) return rc;
            if ((rc = S->tvals.grow(ctx, esz * sizeof(u64)))) return rc;
            if ((rc = S->parent.grow(ctx, (size_t)ntri * sizeof(u64)))) return rc;
            if ((rc = S->mnext.grow(ctx, (size_t)ntri * 3 * sizeof(uint32_t)))) return rc;
            if ((rc = S->comp.grow(ctx, cxp_comp_bytes(ntri)))) return rc;
            u64* ekeys = S->tkeys.as<u64>();
            u64* eheads = S->tvals.as<u64>();
            u64* parent = S->parent.as<u64>();
            cxp_tables_taken(S);    // (the 3-D orientation's tables lived in S->parent and S->comp)
            uint32_t* next = S->mnext.as<uint32_t>();
            u64* comp = S->comp.as<u64>();    // the component tables (cxp_comp_view: laid out by cxp_orient_pick)
            cxp_fill64(st, ekeys, (size_t)esz, CXD_EMPTY);
            cxp_fill64(st, eheads, (size_t)esz, CXD_EMPTY);
            cxp_iota64(st, parent, ntri);
            hipLaunchKernelGGL(cxp_k_edge_lists, dim3(cx_blocks(ntri, CXP_EL)), dim3(256), 0, st, tris, ntri, ekeys, eheads, esz - 1, emult4, next);
            hipLaunchKernelGGL(cxp_k_edge_union_compat, dim3(cx_blocks(ntri)), dim3(256), 0, st, ntri, (const uint32_t*)next, (const double*)ttime, parent);
            // segment midpoints, no keys: the largest index breaks the tie.  (The list of possible start triangles sits where the edge lists'
            // `next` words were: free by now)
            uint32_t ncomp = 0;
            if ((rc = cxp_orient_pick(ctx, tris, ntri, mid, parent, comp, nullptr, nullptr, next, misc))) return rc;
            if ((rc = cxp_orient_decide(ctx, tris, ntri, mid, parent, comp, next, misc, true, &ncomp))) return rc;
            CX_HIP(ctx, hipStreamSynchronize(st));
            CX_HIP(ctx, hipGetLastError());
            S->ms_out = nseg; S->mt_out = ntri;
            counts[1] = nseg; counts[2] = ntri; counts[4] = ncomp;
        }
        memcpy(&counts[5], &h[0], 8); memcpy(&counts[6], &h[1], 8);   // orderable encodings, decoded by the host side
    }
    // Segments and triangles sorted by the bin of their start time: the surface at a time t is then a window of ids (cx_morph_eval_many).
    // AFTER the orientation: on sorted triangles the edge lists get a little shorter work (2.9 -> 2.7 ms) but the time-compatible unions
    // take 9.4 ms instead of 2.6 (measured on config 4: in march order the triangles of one edge follow each other within a few ids and a
    // list's nodes share cache lines; sorted by time they lie a layer's worth of ids apart).
    if (S->ms_out && S->mt_out && (rc = cxp_morph_sort_by_start(ctx, S, (uint32_t)S->ms_out, (uint32_t)S->mt_out, h_mm))) {
        S->ms_out = 0; S->mt_out = 0;
        return rc;
    }
    if (out_counts) memcpy(out_counts, counts, sizeof(counts));
    return CX_OK;
}

extern "C" int cx_morph_download(cx_ctx* ctx, double* points_xyzt, int32_t* segments, int32_t* triangles) {
    if (!ctx || !ctx->post) return CX_ERR_INVALID;
    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_post_state* S = ctx->post;
    void* d[3] = {(points_xyzt && S->nv_out) ? (void*)points_xyzt : nullptr, (segments && S->ms_out) ? (void*)segments : nullptr,
                  (triangles && S->mt_out) ? (void*)triangles : nullptr};
    const void* sp[3] = {S->pts.get(), S->msegs.get(), S->mtris.get()};
    const size_t nb[3] = {(size_t)S->nv_out * 4 * sizeof(double), (size_t)S->ms_out * 2 * sizeof(int32_t), (size_t)S->mt_out * 3 * sizeof(int32_t)};
    return cx_copy_to_host(ctx, 3, d, sp, nb);
}

// ---- stable sort of the morph triangles and their segments by the bin of their start time ----------------------------------------
// (the last step of cx_morph_triangles).  A morph triangle lives for a layer or two of the time axis, and ids follow the march, whose
// fastest axis is time: in id order the triangles that exist at one t are spread over ALL ids (nearly every block of 1 024 consecutive
// triangles exists at every t), and rounds 1-4 walked flag arrays as long as all triangles and all segments for every surface.  Sorted
// by start-time bin -- CXP_SB_BINS bins over the time range of all points, ids keeping their order inside a bin (stable: the
// neighbourhood the march gives the ids survives inside a time layer) -- the triangles that exist at t start inside the window of
// bins [bin(t - longest life) - 1, bin(t) + 1], a contiguous range of ids, and so do the segments they use.  The arrays the caller
// downloads (cx_morph_download) are the sorted ones: the order of morph triangles carries no meaning in the reference (a Python list
// filled from a dict, pentatopes.py:314-368), and the host-side MorphTriangles.triangles_at of the mirrored class sees the same order.
//
// Counting sort with no atomics: a wave takes CXP_SB_UNIT consecutive elements, counts them per bin in LDS (lanes of one bin add up
// among themselves: neighbouring triangles start at the same few times) and leaves the non-zero counts in a [bin][unit] matrix; an
// exclusive scan of that matrix in memory order is the position of every (bin, unit)'s first element; a second walk hands out ranks.
#define CXP_SB_BINS 256u
#define CXP_SB_UNIT 1024u
__device__ __forceinline__ uint32_t cxp_sb_bin(double x, double lo, double inv_width) {
    const double b = (x - lo) * inv_width;
    return b <= 0.0 ? 0u : (b >= (double)(CXP_SB_BINS - 1u) ? CXP_SB_BINS - 1u : (uint32_t)b);
}
// range = {start, end} per element (16 bytes, in order)
__global__ __launch_bounds__(256) void cxp_k_sb_hist(const double* range, uint32_t n, double lo, double inv_width, uint8_t* bins, uint32_t* counts,
                                                     uint32_t nunits, u64* maxdur) {
    __shared__ uint32_t h[4][CXP_SB_BINS];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    for (uint32_t x = lane; x < CXP_SB_BINS; x += 64u) h[w][x] = 0;
    __syncthreads();
    const uint32_t unit = blockIdx.x * 4u + w;
    double dur = 0.0;
    for (uint32_t r = 0; r < CXP_SB_UNIT / 64u; r++) {
        const size_t q = (size_t)unit * CXP_SB_UNIT + r * 64u + lane;
        const bool in = q < n;
        uint32_t bin = 0;
        if (in) {
            const double2 ab = *reinterpret_cast<const double2*>(range + q * 2);
            bin = cxp_sb_bin(ab.x, lo, inv_width);
            dur = fmax(dur, ab.y - ab.x);
            bins[q] = (uint8_t)bin;
        }
        uint64_t todo = __ballot(in);
        while (todo) {      // wave-uniform: one round per bin present among the 64
            const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
            const uint32_t bb = (uint32_t)__shfl((int)bin, (int)leader);
            const uint64_t same = __ballot(in && bin == bb) & todo;
            if (lane == leader) h[w][bb] += (uint32_t)__popcll(same);
            todo &= ~same;
        }
    }
    __syncthreads();
    if (unit < nunits)
        for (uint32_t x = lane; x < CXP_SB_BINS; x += 64u)
            if (h[w][x]) counts[(size_t)x * nunits + unit] = h[w][x];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dur = fmax(dur, __shfl_xor(dur, o));
    if (lane == 0 && dur > 0.0) cxd_max64(maxdur, cxd_orderable(dur));
}
__global__ __launch_bounds__(256) void cxp_k_sb_rank(const uint8_t* bins, uint32_t n, const uint32_t* offs, uint32_t nunits, uint32_t* rank) {
    __shared__ uint32_t h[4][CXP_SB_BINS];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    for (uint32_t x = lane; x < CXP_SB_BINS; x += 64u) h[w][x] = 0;
    __syncthreads();
    const uint32_t unit = blockIdx.x * 4u + w;
    uint32_t mine[CXP_SB_UNIT / 64u];
#pragma unroll
    for (uint32_t r = 0; r < CXP_SB_UNIT / 64u; r++) {
        const size_t q = (size_t)unit * CXP_SB_UNIT + r * 64u + lane;
        mine[r] = q < n ? (uint32_t)bins[q] : 0xFFFFFFFFu;
    }
    // which bins the unit holds (their cursors are the only ones loaded: a unit of neighbouring ids holds a few)
#pragma unroll
    for (uint32_t r = 0; r < CXP_SB_UNIT / 64u; r++) {
        const bool in = mine[r] != 0xFFFFFFFFu;
        uint64_t todo = __ballot(in);
        while (todo) {
            const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
            const uint32_t bb = (uint32_t)__shfl((int)mine[r], (int)leader);
            const uint64_t same = __ballot(in && mine[r] == bb) & todo;
            if (lane == leader) h[w][bb] = 1u;
            todo &= ~same;
        }
    }
    __syncthreads();
    if (unit < nunits)
        for (uint32_t x = lane; x < CXP_SB_BINS; x += 64u)
            if (h[w][x]) h[w][x] = offs[(size_t)x * nunits + unit];
    __syncthreads();
    volatile uint32_t* cur = h[w];
#pragma unroll
    for (uint32_t r = 0; r < CXP_SB_UNIT / 64u; r++) {
        const bool in = mine[r] != 0xFFFFFFFFu;
        uint64_t todo = __ballot(in);
        uint32_t my_rank = 0;
        while (todo) {
            const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
            const uint32_t bb = (uint32_t)__shfl((int)mine[r], (int)leader);
            const uint64_t same = __ballot(in && mine[r] == bb) & todo;
            const uint32_t base = cur[bb];
            if (in && mine[r] == bb) my_rank = base + (uint32_t)__popcll(same & ((1ULL << lane) - 1ULL));
            __builtin_amdgcn_wave_barrier();
            if (lane == leader) cur[bb] = base + (uint32_t)__popcll(same);
            __builtin_amdgcn_wave_barrier();
            todo &= ~same;
        }
        if (in) rank[(size_t)unit * CXP_SB_UNIT + r * 64u + lane] = my_rank;
    }
}
// first element of every bin (the scanned matrix at unit 0) + the total
__global__ void cxp_k_sb_starts(const uint32_t* offs, uint32_t nunits, uint32_t n, uint32_t* out) {
    const uint32_t b = threadIdx.x;
    if (b < CXP_SB_BINS) out[b] = offs[(size_t)b * nunits];
    if (b == CXP_SB_BINS) out[b] = n;
}
__global__ void cxp_k_sb_move_segs(const int32_t* segs, const double* stime, const double* mid, uint32_t ns, const uint32_t* rank, int32_t* segs2,
                                   double* stime2, double* mid2) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= ns) return;
    const int2 ab = *reinterpret_cast<const int2*>(segs + (size_t)s * 2);
    const double2 tt = *reinterpret_cast<const double2*>(stime + (size_t)s * 2);
    double m0 = 0.0, m1 = 0.0, m2 = 0.0;
    if (mid2) { m0 = mid[(size_t)s * 3]; m1 = mid[(size_t)s * 3 + 1]; m2 = mid[(size_t)s * 3 + 2]; }    // (the midpoints only while somebody still reads them)
    const uint32_t r = rank[s];
    *reinterpret_cast<int2*>(segs2 + (size_t)r * 2) = ab;
    *reinterpret_cast<double2*>(stime2 + (size_t)r * 2) = tt;
    if (mid2) { mid2[(size_t)r * 3] = m0; mid2[(size_t)r * 3 + 1] = m1; mid2[(size_t)r * 3 + 2] = m2; }
}
__global__ void cxp_k_sb_move_tris(const int32_t* tris, const double* ttime, uint32_t nt, const uint32_t* rank_t, const uint32_t* rank_s, int32_t* tris2,
                                   double* ttime2) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nt) return;
    const uint32_t a = (uint32_t)tris[(size_t)q * 3], b = (uint32_t)tris[(size_t)q * 3 + 1], c = (uint32_t)tris[(size_t)q * 3 + 2];
    const double2 tt = *reinterpret_cast<const double2*>(ttime + (size_t)q * 2);
    const uint32_t r = rank_t[q];
    const uint32_t na = rank_s[a], nb = rank_s[b], nc = rank_s[c];
    tris2[(size_t)r * 3] = (int32_t)na; tris2[(size_t)r * 3 + 1] = (int32_t)nb; tris2[(size_t)r * 3 + 2] = (int32_t)nc;
    *reinterpret_cast<double2*>(ttime2 + (size_t)r * 2) = tt;
}
static inline double cxp_host_from_orderable(u64 o) {
    const u64 b = (o >> 63) ? (o & 0x7FFFFFFFFFFFFFFFULL) : ~o;
    double d;
    memcpy(&d, &b, sizeof(d));
    return d;
}
// ranks of n elements by the bin of range[2 q]; bin starts (CXP_SB_BINS + 1) and the longest range[2 q + 1] - range[2 q] to the host.
// Scratch: S->mnext (bins), S->flags (count matrix), S->scan (its scan), S->misc words CXP_M_SB_STARTS.. (starts), CXP_M_MAXDUR (longest life).
static int cxp_sb_ranks(cx_ctx* ctx, cx_post_state* S, const double* range, uint32_t n, double lo, double inv_width, uint32_t* rank,
                        uint32_t* starts_host, double* maxdur_host) {
    int rc;
    hipStream_t st = ctx->stream;
    const uint32_t nunits = cx_blocks(n, CXP_SB_UNIT);
    const size_t cells = (size_t)CXP_SB_BINS * nunits;
    if (cells >= 0xFFFFFFFFull) { ctx->err = "cx_morph_triangles: too many morph triangles for the start-time sort"; return CX_ERR_INVALID; }
    if ((rc = S->mnext.grow(ctx, (size_t)n + 64))) return rc;
    if ((rc = S->flags.grow(ctx, (cells + 16) * sizeof(uint32_t)))) return rc;
    if ((rc = S->scan.grow(ctx, (cells + 16) * sizeof(uint32_t)))) return rc;
    uint8_t* bins = S->mnext.as<uint8_t>();
    uint32_t* counts = S->flags.as<uint32_t>();
    uint32_t* offs = S->scan.as<uint32_t>();
    uint32_t* misc = S->misc.as<uint32_t>();
    u64* maxdur = (u64*)(misc + CXP_M_MAXDUR);
    CX_HIP(ctx, hipMemsetAsync(counts, 0, cells * sizeof(uint32_t), st));
    CX_HIP(ctx, hipMemsetAsync(maxdur, 0, sizeof(u64), st));
    const uint32_t nblocks = cx_blocks(nunits, 4);
    hipLaunchKernelGGL(cxp_k_sb_hist, dim3(nblocks), dim3(256), 0, st, range, n, lo, inv_width, bins, counts, nunits, maxdur);
    if ((rc = cxp_scan(ctx, S, counts, offs, (uint32_t)cells, misc + CXP_M_SB_TOTAL))) return rc;
    hipLaunchKernelGGL(cxp_k_sb_rank, dim3(nblocks), dim3(256), 0, st, (const uint8_t*)bins, n, (const uint32_t*)offs, nunits, rank);
    hipLaunchKernelGGL(cxp_k_sb_starts, dim3(1), dim3(512), 0, st, (const uint32_t*)offs, nunits, n, misc + CXP_M_SB_STARTS);
    u64 md = 0;
    CX_HIP(ctx, hipMemcpyAsync(starts_host, misc + CXP_M_SB_STARTS, (CXP_SB_BINS + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    CX_HIP(ctx, hipMemcpyAsync(&md, maxdur, sizeof(md), hipMemcpyDeviceToHost, st));
    CX_HIP(ctx, hipStreamSynchronize(st));
    CX_HIP(ctx, hipGetLastError());
    *maxdur_host = md ? cxp_host_from_orderable(md) : 0.0;
    return CX_OK;
}
// mm_host = orderable min / max of the time of all points (misc words CXP_M_MINMAX_T, read by the caller)
static int cxp_morph_sort_by_start(cx_ctx* ctx, cx_post_state* S, uint32_t nseg, uint32_t ntri, const u64* mm_host) {
    int rc;
    hipStream_t st = ctx->stream;
    S->msorted = false;
    if (!nseg || !ntri) return CX_OK;
    const double lo = cxp_host_from_orderable(mm_host[0]), hi = cxp_host_from_orderable(mm_host[1]);
    const double inv_width = (hi > lo) ? (double)CXP_SB_BINS / (hi - lo) : 0.0;
    if ((rc = S->msegs2.grow(ctx, (size_t)(nseg + 1) * 2 * sizeof(int32_t)))) return rc;
    if ((rc = S->mtris2.grow(ctx, (size_t)(ntri + 1) * 3 * sizeof(int32_t)))) return rc;
    if ((rc = S->mtime2.grow(ctx, ((size_t)(nseg + 1) * 2 + (size_t)(ntri + 1) * 2) * sizeof(double)))) return rc;
    if ((rc = S->parent.grow(ctx, ((size_t)nseg + ntri + 64) * sizeof(uint32_t)))) return rc;
    uint32_t* rank_s = S->parent.as<uint32_t>();
    cxp_tables_taken(S);    // (the 3-D orientation's tables lived in S->parent)
    uint32_t* rank_t = rank_s + nseg + 16;
    const int32_t* segs = S->msegs.as<const int32_t>();
    const int32_t* tris = S->mtris.as<const int32_t>();
    const double* stime = S->mtime.as<const double>();
    const double* ttime = stime + (size_t)(nseg + 1) * 2;
    double* stime2 = S->mtime2.as<double>();
    double* ttime2 = stime2 + (size_t)(nseg + 1) * 2;
    if ((rc = cxp_sb_ranks(ctx, S, stime, nseg, lo, inv_width, rank_s, S->mbin_s, &S->ms_maxdur))) return rc;
    if ((rc = cxp_sb_ranks(ctx, S, ttime, ntri, lo, inv_width, rank_t, S->mbin_t, &S->mt_maxdur))) return rc;
    // (the segment midpoints are scratch of the orientation, which is over: they stay behind)
    hipLaunchKernelGGL(cxp_k_sb_move_segs, dim3(cx_blocks(nseg)), dim3(256), 0, st, segs, stime, (const double*)nullptr, nseg, (const uint32_t*)rank_s,
                       S->msegs2.as<int32_t>(), stime2, (double*)nullptr);
    hipLaunchKernelGGL(cxp_k_sb_move_tris, dim3(cx_blocks(ntri)), dim3(256), 0, st, tris, ttime, ntri, (const uint32_t*)rank_t, (const uint32_t*)rank_s,
                       S->mtris2.as<int32_t>(), ttime2);
    CX_HIP(ctx, hipStreamSynchronize(st));
    CX_HIP(ctx, hipGetLastError());
    std::swap(S->msegs, S->msegs2);
    std::swap(S->mtris, S->mtris2);
    std::swap(S->mtime, S->mtime2);
    S->mt_lo = lo;
    S->mt_inv_width = inv_width;
    S->msorted = true;
    return CX_OK;
}

// ---- B6: the surfaces at times t[0..n) from the morph triangles (misc/morph_triangles.js:26-140; MorphTriangles.triangles_at):
// a triangle is visible while t lies inside the intervals of all three of its segments (lo <= t <= hi with the intersection of their
// ranges, which cxp_k_tri_segments left per triangle); its corners are the points of its segments at t (linear interpolation, low t ->
// high t).  Points and triangles of a surface are compacted in index order (the order numpy.unique / boolean indexing give on the host).
//
// ALL the times of a call go through ONE set of launches (config 4's per-t isosurface stream: 64 surfaces).  Time i tests the window of
// triangle ids [tf, tf + tn) that can exist at t_i and flags inside the window of segment ids [sf, sf + sn) (see the sort above); the
// windows of all times lie one behind the other in the flag arrays, each padded to whole blocks of CXP_ME_BLOCK flags, and a block finds
// its time by bisection over the descriptors.  Ordered compaction without materialised scans: flags are bytes, a workgroup counts the
// flags of its block (first pass), one workgroup per (time, kind) turns the block counts into offsets, and the consumer kernels redo the
// scan INSIDE their block while they write.  The surfaces lie one behind the other in the two output arrays, tightly.
#define CXP_ME_BLOCK 4096u
struct cxp_me_desc {
    double t;
    uint32_t tf, tn, sf, sn;   // windows of triangle / segment ids
    uint32_t tb0, sb0;         // first block of the time's triangle flags / segment flags (blocks of CXP_ME_BLOCK, all times one behind the other)
};
__device__ __forceinline__ uint32_t cxp_me_time_of_tblock(const cxp_me_desc* D, uint32_t nd, uint32_t blk) {
    uint32_t lo = 0, hi = nd;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (D[mid].tb0 <= blk) lo = mid; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ uint32_t cxp_me_time_of_sblock(const cxp_me_desc* D, uint32_t nd, uint32_t blk) {
    uint32_t lo = 0, hi = nd;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (D[mid].sb0 <= blk) lo = mid; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ uint32_t cxp_block_excl_t(uint32_t t, uint32_t* s, uint32_t& block_total) {   // exclusive prefix of one number per thread, 256 threads
    s[threadIdx.x] = t;
    __syncthreads();
    for (uint32_t o = 1; o < 256; o <<= 1) {
        const uint32_t x = (threadIdx.x >= o) ? s[threadIdx.x - o] : 0u;
        __syncthreads();
        s[threadIdx.x] += x;
        __syncthreads();
    }
    block_total = s[255];
    const uint32_t r = s[threadIdx.x] - t;
    __syncthreads();
    return r;
}
// 16 flags (bytes, 0 / 1) as a bit mask; p is 16-byte aligned and the 16 bytes exist (the windows are padded to whole blocks)
__device__ __forceinline__ uint32_t cxp_flags16(const uint8_t* p) {
    const uint4 w = *reinterpret_cast<const uint4*>(p);
    const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
    uint32_t m = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++)
        m |= (((ww[k] & 1u) | ((ww[k] >> 7) & 2u) | ((ww[k] >> 14) & 4u) | ((ww[k] >> 21) & 8u))) << (4u * k);
    return m;
}
// the triangles of every window that exist at the window's time: a flag byte per window position (written for ALL positions of the
// padded window: nothing to clear) and the flags of their segments (set only; cleared by the kernel that consumes them).
// 16 workgroups of 256 per block of CXP_ME_BLOCK window positions.  err: a segment outside its window (cannot happen while the sort and
// the windows agree; checked because the write would land in another time's flags)
__global__ __launch_bounds__(256) void cxp_k_me_visible(const cxp_me_desc* D, uint32_t nd, const double* ttime, const int32_t* tris, uint8_t* tflag,
                                                        uint8_t* sused, uint32_t* err) {
    const uint32_t blk = blockIdx.x >> 4;
    const uint32_t i = cxp_me_time_of_tblock(D, nd, blk);
    const cxp_me_desc d = D[i];
    const uint32_t in_blk = (blockIdx.x & 15u) * 256u + threadIdx.x;
    const uint32_t x = (blk - d.tb0) * CXP_ME_BLOCK + in_blk;
    bool vis = false;
    if (x < d.tn) {
        const size_t q = (size_t)d.tf + x;
        const double2 r = *reinterpret_cast<const double2*>(ttime + q * 2);
        // [start, end): the viewer's active set (misc/morph_triangles.js:117-147, `triangle_max_t > min_t`).  Closed at the end, a surface
        // on a vertex time held both the slices that end there and those that start there.
        vis = r.x <= d.t && d.t < r.y;
        if (vis) {
            const uint32_t a = (uint32_t)tris[q * 3] - d.sf, b = (uint32_t)tris[q * 3 + 1] - d.sf, c = (uint32_t)tris[q * 3 + 2] - d.sf;
            if (a < d.sn && b < d.sn && c < d.sn) {
                uint8_t* su = sused + (size_t)d.sb0 * CXP_ME_BLOCK;
                su[a] = 1; su[b] = 1; su[c] = 1;
            } else {
                vis = false;
                *err = 1u;
            }
        }
    }
    tflag[(size_t)blk * CXP_ME_BLOCK + in_blk] = vis ? 1 : 0;
}
// block counts: workgroups [0, nsb) the segment flags, the rest the triangle flags
__global__ __launch_bounds__(256) void cxp_k_me_count16(const uint8_t* sused, uint32_t nsb, const uint8_t* tflag, uint32_t* scnt, uint32_t* tcnt) {
    __shared__ uint32_t s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const bool second = blockIdx.x >= nsb;
    const uint32_t blk = second ? blockIdx.x - nsb : blockIdx.x;
    const uint8_t* flags = second ? tflag : sused;
    uint32_t c = __popc(cxp_flags16(flags + (size_t)blk * CXP_ME_BLOCK + threadIdx.x * 16u));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o);
    if ((threadIdx.x & 63u) == 0 && c) atomicAdd(&s_n, c);
    __syncthreads();
    if (threadIdx.x == 0) (second ? tcnt : scnt)[blk] = s_n;
}
// one workgroup per (time, kind): its block counts -> exclusive offsets inside the time's surface (in place), the total -> totals[2 i + kind]
__global__ __launch_bounds__(256) void cxp_k_me_offsets(const cxp_me_desc* D, uint32_t nd, uint32_t* scnt, uint32_t* tcnt, uint32_t* totals, u64* bases) {
    __shared__ uint32_t s[256];
    const uint32_t i = blockIdx.x >> 1, kind = blockIdx.x & 1u;
    const cxp_me_desc d = D[i];
    const uint32_t b0 = kind ? d.tb0 : d.sb0;
    const uint32_t nb = (kind ? d.tn : d.sn) ? ((kind ? d.tn : d.sn) + CXP_ME_BLOCK - 1u) / CXP_ME_BLOCK : 0u;
    uint32_t* cnt = (kind ? tcnt : scnt) + b0;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nb; base += 256u) {     // block-uniform
        const uint32_t k = base + threadIdx.x;
        const uint32_t v = k < nb ? cnt[k] : 0u;
        uint32_t tot;
        const uint32_t e = cxp_block_excl_t(v, s, tot);
        if (k < nb) cnt[k] = carry + e;
        carry += tot;
    }
    if (threadIdx.x == 0) {
        totals[2u * i + kind] = carry;
        if (nd == 1u) bases[kind] = 0ull;      // (one surface: nothing before it, cxp_k_me_bases is not launched)
    }
}
// exclusive prefix of the totals over the times, both kinds (one workgroup; 64-bit: the sums of many surfaces may pass 2^32)
__global__ __launch_bounds__(256) void cxp_k_me_bases(const uint32_t* totals, uint32_t nd, u64* bases) {
    __shared__ u64 sp[256], st[256];
    u64 cp = 0, ct = 0;
    for (uint32_t base = 0; base < nd; base += 256u) {
        const uint32_t k = base + threadIdx.x;
        const u64 vp = k < nd ? totals[2u * k] : 0ull, vt = k < nd ? totals[2u * k + 1u] : 0ull;
        sp[threadIdx.x] = vp; st[threadIdx.x] = vt;
        __syncthreads();
        for (uint32_t o = 1; o < 256; o <<= 1) {
            const u64 xp = (threadIdx.x >= o) ? sp[threadIdx.x - o] : 0ull, xt = (threadIdx.x >= o) ? st[threadIdx.x - o] : 0ull;
            __syncthreads();
            sp[threadIdx.x] += xp; st[threadIdx.x] += xt;
            __syncthreads();
        }
        if (k < nd) { bases[2u * k] = cp + sp[threadIdx.x] - vp; bases[2u * k + 1u] = ct + st[threadIdx.x] - vt; }
        cp += sp[255]; ct += st[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) { bases[2u * nd] = cp; bases[2u * nd + 1u] = ct; }
}
// (A block whose count is zero leaves before it reads a flag.)  The consumers work in two steps: the positions of the block's set flags go
// into a list in LDS (the scan inside the block), then ONE THREAD PER LIST ENTRY does the work -- every lane busy, the gathers of a wave
// independent of each other, the stores of neighbouring lanes next to each other.  (First version: every thread walked the set bits of its
// own 16 flags, three of them on average, each round a chain of dependent gathers and a 24-byte store of its own: 0.67 + 0.71 ms for the 64
// surfaces of config 4.)
__device__ __forceinline__ uint32_t cxp_me_list(uint32_t m, uint16_t* list, uint32_t* s) {
    uint32_t tot;
    uint32_t pos = cxp_block_excl_t(__popc(m), s, tot);
    while (m) {
        const uint32_t k = __ffs(m) - 1u;
        m &= m - 1u;
        list[pos++] = (uint16_t)(threadIdx.x * 16u + k);
    }
    __syncthreads();
    return tot;
}
__global__ __launch_bounds__(256) void cxp_k_me_points(const cxp_me_desc* D, uint32_t nd, const double* P4, const int32_t* segs, uint8_t* sused,
                                                       const uint32_t* soff, const uint32_t* totals, const u64* bases, uint32_t* snew, double* out) {
    __shared__ uint32_t s[256];
    __shared__ uint16_t list[CXP_ME_BLOCK];
    const uint32_t blk = blockIdx.x;
    const uint32_t i = cxp_me_time_of_sblock(D, nd, blk);
    const cxp_me_desc d = D[i];
    const uint32_t nb = (d.sn + CXP_ME_BLOCK - 1u) / CXP_ME_BLOCK;
    const uint32_t rel = blk - d.sb0;
    if (rel >= nb) return;
    const uint32_t first = soff[blk];                                    // inside the surface
    const uint32_t next = (rel + 1u < nb) ? soff[blk + 1u] : totals[2u * i];
    if (next == first) return;
    const size_t fbase = (size_t)blk * CXP_ME_BLOCK;
    const uint32_t m = cxp_flags16(sused + fbase + threadIdx.x * 16u);
    if (m) *reinterpret_cast<uint4*>(sused + fbase + threadIdx.x * 16u) = make_uint4(0u, 0u, 0u, 0u);      // (the flags are all zero again when the call ends)
    const uint32_t n = cxp_me_list(m, list, s);
    const u64 gbase = bases[2u * i] + first;
    const double t = d.t;
    const size_t sg0 = (size_t)d.sf + (size_t)rel * CXP_ME_BLOCK;
    for (uint32_t j = threadIdx.x; j < n; j += 256u) {
        const uint32_t x = list[j];
        snew[fbase + x] = first + j;
        const int2 ab = *reinterpret_cast<const int2*>(segs + (sg0 + x) * 2);
        const double4 a = *reinterpret_cast<const double4*>(P4 + (size_t)ab.x * 4);
        const double4 b = *reinterpret_cast<const double4*>(P4 + (size_t)ab.y * 4);
        const double lo = a.w, hi = b.w;
        const double lam = (hi > lo) ? (t - lo) / (hi - lo) : 0.0;
        double* o = out + (size_t)(gbase + j) * 3;
        o[0] = a.x + lam * (b.x - a.x); o[1] = a.y + lam * (b.y - a.y); o[2] = a.z + lam * (b.z - a.z);
    }
}
__global__ __launch_bounds__(256) void cxp_k_me_tris(const cxp_me_desc* D, uint32_t nd, const int32_t* tris, const uint8_t* tflag, const uint32_t* toff,
                                                     const uint32_t* totals, const u64* bases, const uint32_t* snew, int32_t* out) {
    __shared__ uint32_t s[256];
    __shared__ uint16_t list[CXP_ME_BLOCK];
    const uint32_t blk = blockIdx.x;
    const uint32_t i = cxp_me_time_of_tblock(D, nd, blk);
    const cxp_me_desc d = D[i];
    const uint32_t nb = (d.tn + CXP_ME_BLOCK - 1u) / CXP_ME_BLOCK;
    const uint32_t rel = blk - d.tb0;
    if (rel >= nb) return;
    const uint32_t first = toff[blk];
    const uint32_t next = (rel + 1u < nb) ? toff[blk + 1u] : totals[2u * i + 1u];
    if (next == first) return;
    const uint32_t m = cxp_flags16(tflag + (size_t)blk * CXP_ME_BLOCK + threadIdx.x * 16u);
    const uint32_t n = cxp_me_list(m, list, s);
    const u64 gbase = bases[2u * i + 1u] + first;
    const uint32_t* sn_ = snew + (size_t)d.sb0 * CXP_ME_BLOCK;
    const size_t q0 = (size_t)d.tf + (size_t)rel * CXP_ME_BLOCK;
    for (uint32_t j = threadIdx.x; j < n; j += 256u) {
        const size_t q = q0 + list[j];
        const uint32_t sa = (uint32_t)tris[q * 3] - d.sf, sb = (uint32_t)tris[q * 3 + 1] - d.sf, sc = (uint32_t)tris[q * 3 + 2] - d.sf;
        const uint32_t a = sn_[sa], b = sn_[sb], c = sn_[sc];
        int32_t* o = out + (size_t)(gbase + j) * 3;
        o[0] = (int32_t)a; o[1] = (int32_t)b; o[2] = (int32_t)c;
    }
}
#define CXP_ME_MAX_TIMES 65536
#define CXP_ME_MAX_BYTES (96ull << 30)
extern "C" int cx_morph_eval_many(cx_ctx* ctx, const double* times, int32_t n_times, int64_t* out_counts) {
    if (!ctx || !ctx->post || n_times < 0 || (n_times && !times)) return CX_ERR_INVALID;
    if (n_times > CXP_ME_MAX_TIMES) { ctx->err = "cx_morph_eval_many: more than 65536 times in one call"; return CX_ERR_INVALID; }
    cx_post_state* S = ctx->post;
    CX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t ns = (uint32_t)S->ms_out, nt = (uint32_t)S->mt_out, nd = (uint32_t)n_times;
    S->me_off.assign((size_t)nd * 4, 0);
    if (out_counts) memset(out_counts, 0, (size_t)nd * 2 * sizeof(int64_t));
    if (!nd || !ns || !nt) return CX_OK;
    if (!S->msorted) { ctx->err = "cx_morph_eval: no sorted morph triangles (cx_morph_triangles first)"; return CX_ERR_STATE; }
    for (uint32_t i = 0; i < nd; i++)
        if (!(times[i] == times[i])) { ctx->err = "cx_morph_eval: a time is not a number"; return CX_ERR_INVALID; }
    int rc;
    // the windows: a triangle (segment) that exists at t starts in [t - longest life, t].  The bin of a start time is computed here exactly
    // as on the device (one subtraction, one product with the same factor: nothing to contract, the same double everywhere), and it is
    // monotone in its argument, so the bins of the two ends bound the window; the lower end gives way by 1e-9 of the time range for the
    // rounding of `end - start` and `t - longest life`.  (First version: a bin of slack on either side -- 8.4 bins tested per time on config 4
    // where 6.4 hold everything.)
    auto bin_of = [&](double x) {
        const double b = (x - S->mt_lo) * S->mt_inv_width;
        return b <= 0.0 ? 0u : (b >= (double)(CXP_SB_BINS - 1u) ? CXP_SB_BINS - 1u : (uint32_t)b);
    };
    const double give = S->mt_inv_width > 0.0 ? 1e-9 * ((double)CXP_SB_BINS / S->mt_inv_width) : 0.0;
    // (descriptors and totals of up to 1 151 times travel through pinned memory, so that neither copy is staged by the runtime; measured
    // on config 4: 7.8 ms for 64 single calls either way -- a call for ONE time is five dependent launches of 2-23 us each, 0.12 ms)
    if (!S->me_pinned && hipHostMalloc(&S->me_pinned, 49152) != hipSuccess) { S->me_pinned = nullptr; (void)hipGetLastError(); }
    const bool pin = S->me_pinned && (size_t)(nd + 1) * sizeof(cxp_me_desc) <= 36864 && ((size_t)2 * nd + 1) * sizeof(uint32_t) <= 12288;
    std::vector<cxp_me_desc> Dv(pin ? 0 : nd + 1);
    cxp_me_desc* D = pin ? (cxp_me_desc*)S->me_pinned : Dv.data();
    uint64_t tblocks = 0, sblocks = 0, pts_bound = 0, tri_bound = 0;
    for (uint32_t i = 0; i < nd; i++) {
        const double t = times[i];
        const uint32_t b_hi = bin_of(t);
        const uint32_t bt = bin_of(t - S->mt_maxdur - give), bs = bin_of(t - S->ms_maxdur - give);
        cxp_me_desc& d = D[i];
        d.t = t;
        d.tf = S->mbin_t[bt]; d.tn = S->mbin_t[b_hi + 1u] - d.tf;
        d.sf = S->mbin_s[bs]; d.sn = S->mbin_s[b_hi + 1u] - d.sf;
        d.tb0 = (uint32_t)tblocks; d.sb0 = (uint32_t)sblocks;
        tblocks += (d.tn + CXP_ME_BLOCK - 1u) / CXP_ME_BLOCK;
        sblocks += (d.sn + CXP_ME_BLOCK - 1u) / CXP_ME_BLOCK;
        pts_bound += std::min<uint64_t>(d.sn, 3ull * d.tn);
        tri_bound += d.tn;
    }
    D[nd].t = 0.0; D[nd].tf = D[nd].tn = D[nd].sf = D[nd].sn = 0; D[nd].tb0 = (uint32_t)tblocks; D[nd].sb0 = (uint32_t)sblocks;
    // the surfaces cannot hold more triangles than their windows, nor more points than the windows' segments (or three per triangle):
    // everything is reserved before anything is enqueued, so that the call runs to its end without the host in the middle
    const uint64_t bytes = (tblocks + sblocks) * (uint64_t)CXP_ME_BLOCK * 5ull + pts_bound * 24ull + tri_bound * 12ull;
    if (tblocks + sblocks >= (1ull << 20) * 16ull || bytes > CXP_ME_MAX_BYTES) {
        ctx->err = "cx_morph_eval_many: the windows of these times need more than 96 GB of work space: fewer times per call";
        return CX_ERR_NOMEM;
    }
    if (!tblocks || !sblocks) return CX_OK;       // every window is empty: every surface is
    const uint32_t ntb = (uint32_t)tblocks, nsb = (uint32_t)sblocks;
    {
        const size_t before = S->meflags.bytes();     // (not the address: a freed block often comes back at the same one, larger)
        if ((rc = S->meflags.grow(ctx, (size_t)sblocks * CXP_ME_BLOCK + 256))) return rc;
        if (S->meflags.bytes() != before) S->meflags_clean = false;
    }
    if ((rc = S->metflag.grow(ctx, (size_t)tblocks * CXP_ME_BLOCK + 256))) return rc;
    if ((rc = S->menew.grow(ctx, (size_t)sblocks * CXP_ME_BLOCK * sizeof(uint32_t) + 256))) return rc;
    if ((rc = S->mecnt.grow(ctx, ((size_t)tblocks + sblocks + 4ull * nd + 64) * sizeof(uint32_t) + (2ull * nd + 8) * sizeof(u64)))) return rc;
    if ((rc = S->medesc.grow(ctx, (size_t)(nd + 1) * sizeof(cxp_me_desc)))) return rc;
    if ((rc = S->me_pts.grow(ctx, (size_t)(pts_bound + 1) * 3 * sizeof(double)))) return rc;
    if ((rc = S->me_tri.grow(ctx, (size_t)(tri_bound + 1) * 3 * sizeof(int32_t)))) return rc;
    // (the segment flags are a buffer of their own, ALL of it zero between two calls: the next call's windows may be laid out differently)
    uint8_t* sused = S->meflags.as<uint8_t>();
    uint8_t* tflag = S->metflag.as<uint8_t>();
    uint32_t* snew = S->menew.as<uint32_t>();
    u64* bases = S->mecnt.as<u64>();                                   // 2 nd + 2 words of 64 bits first (alignment)
    uint32_t* scnt = (uint32_t*)(bases + 2ull * nd + 8);
    uint32_t* tcnt = scnt + nsb + 8;
    uint32_t* totals = tcnt + ntb + 8;
    uint32_t* err = totals + 2ull * nd;                              // (right behind the totals: one copy back for both)
    cxp_me_desc* Dd = S->medesc.as<cxp_me_desc>();
    const double* P4 = S->pts.as<const double>();
    const int32_t* segs = S->msegs.as<const int32_t>();
    const int32_t* tris = S->mtris.as<const int32_t>();
    const double* ttime = S->mtime.as<const double>() + (size_t)(ns + 1) * 2;   // behind the segments' ranges (cx_morph_triangles)
    // (the segment flags count as zeroed only while the last call ran to its end; they may have moved since: a larger call reserves anew)
    const bool clean = S->meflags_clean;
    S->meflags_clean = false;
    if (!clean) CX_HIP(ctx, hipMemsetAsync(sused, 0, S->meflags.bytes(), st));
    CX_HIP(ctx, hipMemcpyAsync(Dd, D, (size_t)(nd + 1) * sizeof(cxp_me_desc), hipMemcpyHostToDevice, st));
    CX_HIP(ctx, hipMemsetAsync(err, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(cxp_k_me_visible, dim3(ntb * 16u), dim3(256), 0, st, (const cxp_me_desc*)Dd, nd, ttime, tris, tflag, sused, err);
    hipLaunchKernelGGL(cxp_k_me_count16, dim3(nsb + ntb), dim3(256), 0, st, (const uint8_t*)sused, nsb, (const uint8_t*)tflag, scnt, tcnt);
    hipLaunchKernelGGL(cxp_k_me_offsets, dim3(2u * nd), dim3(256), 0, st, (const cxp_me_desc*)Dd, nd, scnt, tcnt, totals, bases);
    if (nd > 1u) hipLaunchKernelGGL(cxp_k_me_bases, dim3(1), dim3(256), 0, st, (const uint32_t*)totals, nd, bases);
    hipLaunchKernelGGL(cxp_k_me_points, dim3(nsb), dim3(256), 0, st, (const cxp_me_desc*)Dd, nd, P4, segs, sused, (const uint32_t*)scnt, (const uint32_t*)totals,
                       (const u64*)bases, snew, S->me_pts.as<double>());
    hipLaunchKernelGGL(cxp_k_me_tris, dim3(ntb), dim3(256), 0, st, (const cxp_me_desc*)Dd, nd, tris, (const uint8_t*)tflag, (const uint32_t*)tcnt,
                       (const uint32_t*)totals, (const u64*)bases, (const uint32_t*)snew, S->me_tri.as<int32_t>());
    std::vector<uint32_t> totv(pin ? 0 : (size_t)2 * nd + 1);
    uint32_t* tot = pin ? (uint32_t*)((char*)S->me_pinned + 36864) : totv.data();
    CX_HIP(ctx, hipMemcpyAsync(tot, totals, ((size_t)2 * nd + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    CX_HIP(ctx, hipStreamSynchronize(st));
    CX_HIP(ctx, hipGetLastError());
    if (tot[2 * nd]) { ctx->err = "cx_morph_eval: a visible triangle uses a segment outside its time's window (internal error)"; return CX_ERR_HIP; }
    S->meflags_clean = true;
    int64_t p0 = 0, t0 = 0;
    for (uint32_t i = 0; i < nd; i++) {
        S->me_off[4 * i] = p0; S->me_off[4 * i + 1] = tot[2 * i]; S->me_off[4 * i + 2] = t0; S->me_off[4 * i + 3] = tot[2 * i + 1];
        p0 += tot[2 * i]; t0 += tot[2 * i + 1];
        if (out_counts) { out_counts[2 * i] = tot[2 * i]; out_counts[2 * i + 1] = tot[2 * i + 1]; }
    }
    return CX_OK;
}
extern "C" int cx_morph_eval_many_download(cx_ctx* ctx, int32_t i, double* points_xyz, int32_t* triangles) {
    if (!ctx || !ctx->post) return CX_ERR_INVALID;
    cx_post_state* S = ctx->post;
    if (i < 0 || (size_t)i * 4 >= S->me_off.size()) { ctx->err = "cx_morph_eval_many_download: no such surface in the last call"; return CX_ERR_INVALID; }
    CX_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t* o = &S->me_off[(size_t)i * 4];
    void* d[2] = {(points_xyz && o[1]) ? (void*)points_xyz : nullptr, (triangles && o[3]) ? (void*)triangles : nullptr};
    const void* sp[2] = {o[1] ? (const void*)(S->me_pts.as<const double>() + (size_t)o[0] * 3) : nullptr,
                         o[3] ? (const void*)(S->me_tri.as<const int32_t>() + (size_t)o[2] * 3) : nullptr};
    const size_t nb[2] = {(size_t)o[1] * 3 * sizeof(double), (size_t)o[3] * 3 * sizeof(int32_t)};
    return cx_copy_to_host(ctx, 2, d, sp, nb);
}
// all surfaces of the last call in one transfer: points of surface 0, 1, ... one behind the other (sum of the point counts x 3 doubles),
// triangles likewise (indices local to their surface) -- one pipelined copy instead of two small ones per surface
extern "C" int cx_morph_eval_many_download_all(cx_ctx* ctx, double* points_xyz, int32_t* triangles) {
    if (!ctx || !ctx->post) return CX_ERR_INVALID;
    cx_post_state* S = ctx->post;
    CX_HIP(ctx, hipSetDevice(ctx->device));
    int64_t np_ = 0, nt_ = 0;
    for (size_t i = 0; i + 3 < S->me_off.size(); i += 4) { np_ += S->me_off[i + 1]; nt_ += S->me_off[i + 3]; }
    void* d[2] = {(points_xyz && np_) ? (void*)points_xyz : nullptr, (triangles && nt_) ? (void*)triangles : nullptr};
    const void* sp[2] = {S->me_pts.get(), S->me_tri.get()};
    const size_t nb[2] = {(size_t)np_ * 3 * sizeof(double), (size_t)nt_ * 3 * sizeof(int32_t)};
    return cx_copy_to_host(ctx, 2, d, sp, nb);
}
extern "C" int cx_morph_eval_many_device_ptrs(cx_ctx* ctx, int32_t i, void** points_xyz, void** triangles) {
    if (!ctx || !ctx->post) return CX_ERR_INVALID;
    cx_post_state* S = ctx->post;
    if (i < 0 || (size_t)i * 4 >= S->me_off.size()) { ctx->err = "cx_morph_eval_many_device_ptrs: no such surface in the last call"; return CX_ERR_INVALID; }
    const int64_t* o = &S->me_off[(size_t)i * 4];
    if (points_xyz) *points_xyz = o[1] ? (void*)(S->me_pts.as<double>() + (size_t)o[0] * 3) : nullptr;
    if (triangles) *triangles = o[3] ? (void*)(S->me_tri.as<int32_t>() + (size_t)o[2] * 3) : nullptr;
    return CX_OK;
}
extern "C" int cx_morph_eval(cx_ctx* ctx, double t, int64_t* out_counts) {
    return cx_morph_eval_many(ctx, &t, 1, out_counts);
}
extern "C" int cx_morph_eval_download(cx_ctx* ctx, double* points_xyz, int32_t* triangles) {
    if (!ctx || !ctx->post) return CX_ERR_INVALID;
    if (ctx->post->me_off.empty()) return CX_OK;      // nothing evaluated: nothing to copy
    return cx_morph_eval_many_download(ctx, 0, points_xyz, triangles);
}
