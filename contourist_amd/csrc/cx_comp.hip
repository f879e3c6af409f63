// cx_comp.hip -- connected components of the Level-1 mesh: labels, per-component measures, filtering.
//
// The orientation step of the post-pass (cx_post.hip, cxp_clean_orient) leaves, per output triangle, the root triangle of its
// component and per root the flip.  From these tables, on request and cached until the next post-pass:
//   cxc_k_roots + scan     component id = rank of the root among the roots (ascending root = ascending smallest triangle index)
//   cxc_k_labels           int32 per triangle, int32 per vertex (the smallest id among the triangles that use it)
//   cxc_k_measure          one lane per triangle: area, signed volume, area-weighted centroid moments, box, edge parity word
//   cxc_k_vertex_count     vertices per component (by vertex label)
//   cxc_k_finish           one lane per component: the cx_component record
//   cxc_k_keep_*           flags, two scans, order-preserving compaction of mesh and tables
// Sums are exact: every triangle's term is rounded ONCE to a multiple of 2^-q and added as an integer (within the wave first, then
// one set of integer atomics into a two-word accumulator per component), so a record is the same bit for bit in every launch
// order and whatever other components the mesh holds.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "cx_ctx.h"
#include "cx_dev.h"

// accumulator words per component
enum {
    CXC_W_NT = 0,       // triangles
    CXC_W_XOR = 1,      // XOR of the hashed undirected edges of every triangle: 0 when every edge is used an even number of times
    CXC_W_AREA = 2,     // 128-bit two's complement sums {low, high}: area, volume, three moments
    CXC_W_VOL = 4,
    CXC_W_MOM = 6,
    CXC_W_LO = 12,      // box: minima / maxima of the order-preserving integer image of the coordinates
    CXC_W_HI = 15,
    CXC_W_NV = 18,      // vertices
    CXC_W_OVER = 19,    // != 0: a term of this component was past the bound the grid 2^-q was chosen for (clamped; the sums are not exact)
    CXC_WORDS = 20
};

struct cx_comp_state {
    uint64_t gen_labels = ~0ULL, gen_table = ~0ULL;   // generation of the mesh (cx_level1_comp_view.gen) the labels / the table belong to
    bool table_world = false;
    double table_md[6] = {0, 0, 0, 1, 1, 1};
    double origin_q[4] = {0, 0, 0, 0};
    uint32_t nc = 0, nv = 0, nt = 0;
    cx_buf<uint32_t> tlab;                              // flags of the roots first, then the triangle labels (int32)
    cx_buf<uint32_t> tidx;                              // exclusive scan of the root flags
    cx_buf<uint32_t> vlab;                              // vertex labels (int32)
    cx_buf<uint32_t> sums;                              // block sums of the scans
    cx_buf<uint32_t> first;                             // root triangle of every component
    cx_buf<u64> acc;
    cx_buf<cx_component> table;
    cx_buf<uint32_t> misc;                              // totals of the scans
    // filtering
    cx_buf<uint32_t> tnew;
    cx_buf<uint32_t> vuse;
    cx_buf<uint32_t> vnew;
    cx_buf<uint8_t> keep;
};

void cx_comp_free(cx_ctx* ctx) {
    cx_comp_state* C = ctx->comp;
    if (!C) return;
    delete C;
    ctx->comp = nullptr;
}

// ---- device helpers -----------------------------------------------------------------------------------------------------------------
// term * 2^q as an integer; a term past the bound the scale was chosen for (|term| 2^q <= 2^54: vertices farther from the centre of the
// grid box than its diagonal, e.g. a caller's mesh that does not fit the corner it was handed over with) is clamped there and reported
__device__ __forceinline__ long long cxc_fixed(double scaled, bool& over) {
    const double lim = 18014398509481984.0;     // 2^54
    if (!(fabs(scaled) <= lim)) { over = true; scaled = scaled > 0.0 ? lim : (scaled < 0.0 ? -lim : 0.0); }
    return __double2ll_rn(scaled);
}

// ---- labels -------------------------------------------------------------------------------------------------------------------------
__global__ void cxc_k_roots(const u64* __restrict__ parent, uint32_t nt, uint32_t* __restrict__ flag) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    flag[t] = ((uint32_t)parent[t] == t) ? 1u : 0u;
}
__global__ void cxc_k_fill32(uint32_t* p, uint32_t n, uint32_t v) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}
// triangle label = rank of its root; vertex label = the smallest label among the triangles that use the vertex (two components may
// touch in one vertex without sharing an edge).  tlab may be the array the root flags were in: they are not read here.
__global__ void cxc_k_labels(const u64* __restrict__ parent, const uint32_t* __restrict__ idx, const int32_t* __restrict__ tri, uint32_t nt, uint32_t nv,
                             int32_t* tlab, int32_t* vlab, uint32_t* __restrict__ first) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const uint32_t root = (uint32_t)parent[t];
    const int32_t c = (int32_t)idx[root];
    tlab[t] = c;
    if (root == t) first[c] = t;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint32_t v = (uint32_t)tri[(size_t)t * 3 + k];
        if (v >= nv) continue;
        if (__hip_atomic_load(&vlab[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= c) continue;
        atomicMin(&vlab[v], c);
    }
}
__global__ void cxc_k_labels_unused(int32_t* vlab, uint32_t nv) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < nv && vlab[v] == 0x7FFFFFFF) vlab[v] = -1;
}

// ---- measures -----------------------------------------------------------------------------------------------------------------------
struct cxc_map {
    double m[3], d[3], o[3];   // world = grid * d + m (no fused multiply-add, as cxw_k_points maps them); o: the centre of the grid box, mapped
    double sa, sv, sm;         // 2^q of the area, the volume and the moments
    int world;
};
__global__ void cxc_k_acc_init(u64* acc, uint32_t nc) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc * (uint32_t)CXC_WORDS) return;
    const uint32_t w = i % (uint32_t)CXC_WORDS;
    acc[i] = (w >= (uint32_t)CXC_W_LO && w < (uint32_t)CXC_W_HI) ? ~0ULL : 0ULL;
}
#define CXC_SMALL_GROUP 4
__device__ __forceinline__ void cxc_lane_atomics(u64* w, long long ia, long long iv, long long im0, long long im1, long long im2, u64 ex,
                                                 u64 lo0, u64 lo1, u64 lo2, u64 hi0, u64 hi1, u64 hi2) {
    atomicAdd(&w[CXC_W_NT], 1ULL);
    atomicXor(&w[CXC_W_XOR], ex);
    cxd_add128(&w[CXC_W_AREA], ia); cxd_add128(&w[CXC_W_VOL], iv);
    cxd_add128(&w[CXC_W_MOM], im0); cxd_add128(&w[CXC_W_MOM + 2], im1); cxd_add128(&w[CXC_W_MOM + 4], im2);
    cxd_min64(&w[CXC_W_LO], lo0); cxd_min64(&w[CXC_W_LO + 1], lo1); cxd_min64(&w[CXC_W_LO + 2], lo2);
    cxd_max64(&w[CXC_W_HI], hi0); cxd_max64(&w[CXC_W_HI + 1], hi1); cxd_max64(&w[CXC_W_HI + 2], hi2);
}
// One lane per triangle in the order of tri_out.  The lanes of a wave that share a label reduce among themselves and ONE of them
// touches memory; nearly every wave of a real mesh holds one label (neighbouring triangles come from neighbouring cells), the others
// take one turn per label they hold.  All control flow around the cross-lane operations is wave-uniform.
__global__ __launch_bounds__(256) void cxc_k_measure(const int32_t* __restrict__ tri, const double* __restrict__ pts, const int32_t* __restrict__ tlab,
                                                     uint32_t nt, uint32_t nv, cxc_map M, u64* __restrict__ acc) {
#pragma clang fp contract(off)
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    bool active = t < nt;
    int32_t label = -1;
    bool over = false;
    long long ia = 0, iv = 0, im0 = 0, im1 = 0, im2 = 0;
    u64 ex = 0ULL, lo0 = ~0ULL, lo1 = ~0ULL, lo2 = ~0ULL, hi0 = 0ULL, hi1 = 0ULL, hi2 = 0ULL;
    if (active) {
        uint32_t v[3];
#pragma unroll
        for (int k = 0; k < 3; k++) v[k] = (uint32_t)tri[(size_t)t * 3 + k];
        active = v[0] < nv && v[1] < nv && v[2] < nv;      // (a mesh of the post-pass never fails this)
        if (active) {
            label = tlab[t];
            double p[3][3];
#pragma unroll
            for (int k = 0; k < 3; k++)
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    const double g = pts[(size_t)v[k] * 3 + a];
                    p[k][a] = M.world ? g * M.d[a] + M.m[a] : g;
                }
            lo0 = cxd_orderable(fmin(p[0][0], fmin(p[1][0], p[2][0]))); hi0 = cxd_orderable(fmax(p[0][0], fmax(p[1][0], p[2][0])));
            lo1 = cxd_orderable(fmin(p[0][1], fmin(p[1][1], p[2][1]))); hi1 = cxd_orderable(fmax(p[0][1], fmax(p[1][1], p[2][1])));
            lo2 = cxd_orderable(fmin(p[0][2], fmin(p[1][2], p[2][2]))); hi2 = cxd_orderable(fmax(p[0][2], fmax(p[1][2], p[2][2])));
            const double e1x = p[1][0] - p[0][0], e1y = p[1][1] - p[0][1], e1z = p[1][2] - p[0][2];
            const double e2x = p[2][0] - p[0][0], e2y = p[2][1] - p[0][1], e2z = p[2][2] - p[0][2];
            const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
            const double area = sqrt(nx * nx + ny * ny + nz * nz) / 2.0;
            const double ax = p[0][0] - M.o[0], ay = p[0][1] - M.o[1], az = p[0][2] - M.o[2];
            const double bx = p[1][0] - M.o[0], by = p[1][1] - M.o[1], bz = p[1][2] - M.o[2];
            const double cx = p[2][0] - M.o[0], cy = p[2][1] - M.o[1], cz = p[2][2] - M.o[2];
            const double det = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx);
            ia = cxc_fixed(area * M.sa, over);
            iv = cxc_fixed((det / 6.0) * M.sv, over);
            im0 = cxc_fixed((area * ((ax + bx + cx) / 3.0)) * M.sm, over);
            im1 = cxc_fixed((area * ((ay + by + cy) / 3.0)) * M.sm, over);
            im2 = cxc_fixed((area * ((az + bz + cz) / 3.0)) * M.sm, over);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const uint32_t a = v[k], b = v[(k + 1) % 3];
                ex ^= cxd_mix(((u64)(a < b ? a : b) << 32) | (u64)(a < b ? b : a));
            }
        }
    }
    if (active && over) atomicOr(&acc[(size_t)label * CXC_WORDS + CXC_W_OVER], 1ULL);       // (never, for a mesh inside its grid box)
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t rem = __ballot(active);
    while (rem != 0ULL) {                                   // wave-uniform
        const int leader = __ffsll((long long)rem) - 1;
        const int32_t k = __shfl(label, leader);
        const bool mine = active && label == k;
        const uint64_t grp = __ballot(mine);
        rem &= ~grp;
        if (__popcll(grp) <= CXC_SMALL_GROUP) {             // a few lanes of another component: their own atomics cost less than twelve butterflies
            if (mine) cxc_lane_atomics(acc + (size_t)k * CXC_WORDS, ia, iv, im0, im1, im2, ex, lo0, lo1, lo2, hi0, hi1, hi2);
            continue;
        }
        // (|term| * 2^q <= 2^54: the sum of 64 lanes stays inside 64 bits)
        const long long sa = cxd_wave_add(mine ? ia : 0LL), sv = cxd_wave_add(mine ? iv : 0LL);
        const long long s0 = cxd_wave_add(mine ? im0 : 0LL), s1 = cxd_wave_add(mine ? im1 : 0LL), s2 = cxd_wave_add(mine ? im2 : 0LL);
        const u64 sx = cxd_wave_xor(mine ? ex : 0ULL);
        const u64 l0 = cxd_wave_min(mine ? lo0 : ~0ULL), l1 = cxd_wave_min(mine ? lo1 : ~0ULL), l2 = cxd_wave_min(mine ? lo2 : ~0ULL);
        const u64 h0 = cxd_wave_max(mine ? hi0 : 0ULL), h1 = cxd_wave_max(mine ? hi1 : 0ULL), h2 = cxd_wave_max(mine ? hi2 : 0ULL);
        if ((int)lane == leader) {
            u64* w = acc + (size_t)k * CXC_WORDS;
            atomicAdd(&w[CXC_W_NT], (u64)__popcll(grp));
            if (sx) atomicXor(&w[CXC_W_XOR], sx);
            cxd_add128(&w[CXC_W_AREA], sa); cxd_add128(&w[CXC_W_VOL], sv);
            cxd_add128(&w[CXC_W_MOM], s0); cxd_add128(&w[CXC_W_MOM + 2], s1); cxd_add128(&w[CXC_W_MOM + 4], s2);
            cxd_min64(&w[CXC_W_LO], l0); cxd_min64(&w[CXC_W_LO + 1], l1); cxd_min64(&w[CXC_W_LO + 2], l2);
            cxd_max64(&w[CXC_W_HI], h0); cxd_max64(&w[CXC_W_HI + 1], h1); cxd_max64(&w[CXC_W_HI + 2], h2);
        }
    }
}
// vertices per component by vertex label, counted within the wave first
__global__ __launch_bounds__(256) void cxc_k_vertex_count(const int32_t* __restrict__ vlab, uint32_t nv, uint32_t nc, u64* __restrict__ acc) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t label = v < nv ? vlab[v] : -1;
    const bool active = label >= 0 && (uint32_t)label < nc;
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t rem = __ballot(active);
    while (rem != 0ULL) {
        const int leader = __ffsll((long long)rem) - 1;
        const int32_t k = __shfl(label, leader);
        const uint64_t grp = __ballot(active && label == k);
        rem &= ~grp;
        if ((int)lane == leader) atomicAdd(&acc[(size_t)k * CXC_WORDS + CXC_W_NV], (u64)__popcll(grp));
    }
}
__global__ void cxc_k_finish(const u64* __restrict__ acc, const uint32_t* __restrict__ first, const u64* __restrict__ cflip, uint32_t nc, cxc_map M,
                             int qa, int qv, int qm, cx_component* __restrict__ table) {
#pragma clang fp contract(off)
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nc) return;
    const u64* w = acc + (size_t)c * CXC_WORDS;
    cx_component r;
    r.triangles = (int64_t)w[CXC_W_NT];
    r.vertices = (int64_t)w[CXC_W_NV];
    r.area = cxd_to_double128(w[CXC_W_AREA], w[CXC_W_AREA + 1], qa);
    r.volume = cxd_to_double128(w[CXC_W_VOL], w[CXC_W_VOL + 1], qv);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double mom = cxd_to_double128(w[CXC_W_MOM + 2 * a], w[CXC_W_MOM + 2 * a + 1], qm);
        r.centroid[a] = r.area > 0.0 ? M.o[a] + mom / r.area : 0.0;
        r.bbox_lo[a] = cxd_from_orderable(w[CXC_W_LO + a]);
        r.bbox_hi[a] = cxd_from_orderable(w[CXC_W_HI + a]);
    }
    const uint32_t root = first[c];
    r.flipped = (int32_t)(cflip[root] & 1ULL);
    r.closed = w[CXC_W_XOR] == 0ULL ? 1 : 0;
    r.first_triangle = (int64_t)root;
    r.reserved[0] = w[CXC_W_OVER] ? 1.0 : 0.0;      // 1: a term was past the bound of the fixed-point grid, the three sums are not exact
    table[c] = r;
}

// ---- filtering ----------------------------------------------------------------------------------------------------------------------
__global__ void cxc_k_keep_flags(const int32_t* __restrict__ tlab, const uint8_t* __restrict__ keep, const int32_t* __restrict__ tri, uint32_t nt, uint32_t nv,
                                 uint32_t* __restrict__ tflag, uint32_t* vuse) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const uint32_t f = keep[tlab[t]] ? 1u : 0u;
    tflag[t] = f;
    if (!f) return;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint32_t v = (uint32_t)tri[(size_t)t * 3 + k];
        if (v < nv) vuse[v] = 1u;          // (every writer stores the same word)
    }
}
// kept triangles in their order, vertex indices renumbered; the tables of the orientation step follow: a component's root is its
// smallest triangle, which is kept with it and stays the smallest
__global__ void cxc_k_keep_tri(const int32_t* __restrict__ tri, const uint32_t* __restrict__ tflag, const uint32_t* __restrict__ tnew,
                               const uint32_t* __restrict__ vnew, const u64* __restrict__ parent, const u64* __restrict__ cflip, uint32_t nt, uint32_t nv,
                               int32_t* __restrict__ tri2, u64* __restrict__ parent2, u64* __restrict__ cflip2) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt || !tflag[t]) return;
    const uint32_t j = tnew[t];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint32_t v = (uint32_t)tri[(size_t)t * 3 + k];
        tri2[(size_t)j * 3 + k] = (int32_t)(v < nv ? vnew[v] : 0u);
    }
    const u64 w = parent[t];
    const uint32_t root = (uint32_t)w;
    parent2[j] = (w & 0xFFFFFFFF00000000ULL) | (u64)tnew[root];
    cflip2[j] = root == t ? cflip[t] : 0ULL;
}
__global__ void cxc_k_keep_vert(const double* __restrict__ pts, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vuse,
                                const uint32_t* __restrict__ vnew, uint32_t nv, double* __restrict__ pts2, uint32_t* __restrict__ keys2) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv || !vuse[v]) return;
    const uint32_t j = vnew[v];
#pragma unroll
    for (int a = 0; a < 3; a++) pts2[(size_t)j * 3 + a] = pts[(size_t)v * 3 + a];
    keys2[j] = keys[v];
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------

static int cxc_state(cx_ctx* ctx, cx_comp_state** out) {
    if (!ctx->comp) ctx->comp = new (std::nothrow) cx_comp_state();
    if (!ctx->comp) return CX_ERR_NOMEM;
    *out = ctx->comp;
    return ctx->comp->misc.grow(ctx, 16);
}

// labels of the current mesh (cached per generation of the mesh)
static int cxc_labels(cx_ctx* ctx, const char* who, cx_level1_comp_view* V, cx_comp_state** Cout) {
    CX_HIP(ctx, hipSetDevice(ctx->device));
    int rc = cx_level1_comp_view_get(ctx, who, V);
    if (rc) return rc;
    cx_comp_state* C;
    if ((rc = cxc_state(ctx, &C))) return rc;
    *Cout = C;
    if (C->gen_labels == V->gen) return CX_OK;
    C->gen_labels = ~0ULL; C->gen_table = ~0ULL;
    const uint32_t nv = V->nv, nt = V->nt;
    hipStream_t st = ctx->stream;
    uint32_t nc = 0;
    if ((rc = C->vlab.grow(ctx, (size_t)nv + 16))) return rc;
    if (nv) hipLaunchKernelGGL(cxc_k_fill32, cx_grid1(nv), dim3(256), 0, st, C->vlab, nv, nt ? 0x7FFFFFFFu : 0xFFFFFFFFu);
    if (nt) {
        if ((rc = C->tlab.grow(ctx, (size_t)nt + 16))) return rc;
        if ((rc = C->tidx.grow(ctx, (size_t)nt + 16))) return rc;
        if ((rc = C->sums.grow(ctx, (size_t)nt / 1024 + 16))) return rc;
        hipLaunchKernelGGL(cxc_k_roots, cx_grid1(nt), dim3(256), 0, st, V->parent, nt, C->tlab);
        if ((rc = cx_scan_u32(ctx, C->tlab, C->tidx, nt, C->sums, C->misc))) return rc;
        CX_HIP(ctx, hipMemcpyAsync(&nc, C->misc, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        CX_HIP(ctx, hipStreamSynchronize(st));
        if ((rc = C->first.grow(ctx, (size_t)nc + 16))) return rc;
        hipLaunchKernelGGL(cxc_k_labels, cx_grid1(nt), dim3(256), 0, st, V->parent, C->tidx, V->tri, nt, nv, C->tlab.as<int32_t>(), C->vlab.as<int32_t>(), C->first);
        hipLaunchKernelGGL(cxc_k_labels_unused, cx_grid1(nv), dim3(256), 0, st, C->vlab.as<int32_t>(), nv);
    }
    CX_HIP(ctx, hipGetLastError());
    C->nc = nc; C->nv = nv; C->nt = nt;
    C->gen_labels = V->gen;
    return CX_OK;
}

// what cx_topo.hip reads: the view, the labels of the current mesh (made here if need be) and the number of components
int cx_comp_labels_get(cx_ctx* ctx, const char* who, cx_level1_comp_view* V, const int32_t** tlab, const int32_t** vlab, uint32_t* nc) {
    cx_comp_state* C = nullptr;
    const int rc = cxc_labels(ctx, who, V, &C);
    if (rc) return rc;
    *tlab = C->tlab.as<const int32_t>(); *vlab = C->vlab.as<const int32_t>(); *nc = C->nc;
    return CX_OK;
}

static bool cxc_md_ok(const double* md) {
    if (!md) return true;
    for (int a = 0; a < 6; a++)
        if (!std::isfinite(md[a])) return false;
    return md[3] != 0.0 && md[4] != 0.0 && md[5] != 0.0;
}
// 2^q for terms bounded by `bound`: |term| * 2^q <= 2^54, so that the 64 lanes of a wave add up inside 64 bits
static int cxc_q(double bound) {
    int e = 0;
    (void)std::frexp(bound > 0.0 ? bound : 1.0, &e);      // bound <= 2^e
    return 54 - e;
}

extern "C" int cx_level1_components(cx_ctx* ctx, const double* mins_delta, int64_t* n_components, void** table_dev, double* origin3_and_q) {
    if (!ctx) return CX_ERR_INVALID;
    if (!cxc_md_ok(mins_delta)) { ctx->err = "cx_level1_components: mins and delta must be finite and delta non-zero"; return CX_ERR_INVALID; }
    cx_level1_comp_view V;
    cx_comp_state* C = nullptr;
    int rc = cxc_labels(ctx, "cx_level1_components", &V, &C);
    if (rc) return rc;
    const uint32_t nc = C->nc;
    const bool world = mins_delta != nullptr;
    const bool cached = C->gen_table == V.gen && C->table_world == world && (!world || !memcmp(C->table_md, mins_delta, 6 * sizeof(double)));
    if (!cached) {
        C->gen_table = ~0ULL;
        cxc_map M;
        double r2 = 0.0;
        for (int a = 0; a < 3; a++) {
            M.m[a] = world ? mins_delta[a] : 0.0;
            M.d[a] = world ? mins_delta[3 + a] : 1.0;
            M.o[a] = (V.corner[a] / 2.0) * M.d[a] + M.m[a];
            const double ext = V.corner[a] * std::fabs(M.d[a]);
            r2 += ext * ext;
        }
        M.world = world ? 1 : 0;
        // every vertex lies within R = the diagonal of the grid box of its centre (twice what the box itself needs: a sample array
        // with a rim around the reference's grid reaches past the box): edges <= 2R, area <= 2R^2, |det| / 6 <= R^3 / 6,
        // |area * (centroid - o)| <= 2R^3
        const double R = std::sqrt(r2);
        const int qa = cxc_q(2.0 * R * R), qv = cxc_q(R * R * R / 6.0), qm = cxc_q(2.0 * R * R * R);
        M.sa = std::ldexp(1.0, qa); M.sv = std::ldexp(1.0, qv); M.sm = std::ldexp(1.0, qm);
        for (int a = 0; a < 3; a++) C->origin_q[a] = M.o[a];
        C->origin_q[3] = (double)std::min(qa, std::min(qv, qm));
        if (nc) {
            hipStream_t st = ctx->stream;
            if ((rc = C->acc.grow(ctx, (size_t)nc * CXC_WORDS + 16))) return rc;
            if ((rc = C->table.grow(ctx, (size_t)nc + 1))) return rc;
            hipLaunchKernelGGL(cxc_k_acc_init, cx_grid1((size_t)nc * CXC_WORDS), dim3(256), 0, st, C->acc, nc);
            hipLaunchKernelGGL(cxc_k_measure, cx_grid1(V.nt), dim3(256), 0, st, V.tri, V.pts, C->tlab.as<const int32_t>(), V.nt, V.nv, M, C->acc);
            hipLaunchKernelGGL(cxc_k_vertex_count, cx_grid1(V.nv), dim3(256), 0, st, C->vlab.as<const int32_t>(), V.nv, nc, C->acc);
            hipLaunchKernelGGL(cxc_k_finish, cx_grid1(nc), dim3(256), 0, st, (const u64*)C->acc, (const uint32_t*)C->first, V.cflip, nc, M, qa, qv, qm, C->table);
            CX_HIP(ctx, hipGetLastError());
        }
        C->table_world = world;
        if (world) memcpy(C->table_md, mins_delta, 6 * sizeof(double));
        C->gen_table = V.gen;
    }
    if (n_components) *n_components = (int64_t)nc;
    if (table_dev) *table_dev = nc ? (void*)C->table : nullptr;
    if (origin3_and_q) memcpy(origin3_and_q, C->origin_q, 4 * sizeof(double));
    return CX_OK;
}

extern "C" int cx_level1_components_download(cx_ctx* ctx, const double* mins_delta, cx_component* out) {
    if (!ctx) return CX_ERR_INVALID;
    int64_t nc = 0;
    void* dev = nullptr;
    const int rc = cx_level1_components(ctx, mins_delta, &nc, &dev, nullptr);
    if (rc || !nc) return rc;
    if (!out) return CX_ERR_INVALID;
    return cx_copy_to_host1(ctx, out, dev, (size_t)nc * sizeof(cx_component));
}

extern "C" int cx_level1_component_labels(cx_ctx* ctx, void** tri_labels_dev, void** vert_labels_dev) {
    if (!ctx) return CX_ERR_INVALID;
    cx_level1_comp_view V;
    cx_comp_state* C = nullptr;
    const int rc = cxc_labels(ctx, "cx_level1_component_labels", &V, &C);
    if (rc) return rc;
    if (tri_labels_dev) *tri_labels_dev = V.nt ? C->tlab.get() : nullptr;
    if (vert_labels_dev) *vert_labels_dev = V.nv ? C->vlab.get() : nullptr;
    return CX_OK;
}

extern "C" int cx_level1_component_labels_download(cx_ctx* ctx, int32_t* tri_labels, int32_t* vert_labels) {
    if (!ctx) return CX_ERR_INVALID;
    cx_level1_comp_view V;
    cx_comp_state* C = nullptr;
    int rc = cxc_labels(ctx, "cx_level1_component_labels_download", &V, &C);
    if (rc) return rc;
    if (tri_labels && V.nt && (rc = cx_copy_to_host1(ctx, tri_labels, C->tlab, (size_t)V.nt * sizeof(int32_t)))) return rc;
    if (vert_labels && V.nv && (rc = cx_copy_to_host1(ctx, vert_labels, C->vlab, (size_t)V.nv * sizeof(int32_t)))) return rc;
    return CX_OK;
}

extern "C" int cx_level1_keep_components(cx_ctx* ctx, const uint8_t* keep, int64_t* out_counts) {
    if (!ctx) return CX_ERR_INVALID;
    cx_level1_comp_view V;
    cx_comp_state* C = nullptr;
    int rc = cxc_labels(ctx, "cx_level1_keep_components", &V, &C);
    if (rc) return rc;
    const uint32_t nc = C->nc, nv = V.nv, nt = V.nt;
    if (nc && !keep) return CX_ERR_INVALID;
    uint32_t kept = 0;
    for (uint32_t c = 0; c < nc; c++) kept += keep[c] ? 1u : 0u;
    uint32_t nv2 = nv, nt2 = nt;
    if (kept != nc) {      // (all ones: the mesh stays as it is, bit for bit)
        hipStream_t st = ctx->stream;
        cx_level1_comp_scratch X;
        if ((rc = cx_level1_comp_scratch_get(ctx, &X))) return rc;
        if ((rc = C->keep.grow(ctx, (size_t)nc + 16))) return rc;
        if ((rc = C->tnew.grow(ctx, (size_t)nt + 16))) return rc;
        if ((rc = C->vuse.grow(ctx, (size_t)nv + 16))) return rc;
        if ((rc = C->vnew.grow(ctx, (size_t)nv + 16))) return rc;
        if ((rc = C->sums.grow(ctx, (size_t)std::max(nt, nv) / 1024 + 16))) return rc;
        uint32_t* tflag = C->tidx;     // (the scan of the root flags has done its work once the labels stand)
        CX_HIP(ctx, hipMemcpyAsync(C->keep, keep, nc, hipMemcpyHostToDevice, st));
        CX_HIP(ctx, hipMemsetAsync(C->vuse, 0, (size_t)nv * sizeof(uint32_t), st));
        hipLaunchKernelGGL(cxc_k_keep_flags, cx_grid1(nt), dim3(256), 0, st, C->tlab.as<const int32_t>(), C->keep.get(), V.tri, nt, nv, tflag, C->vuse);
        if ((rc = cx_scan_u32(ctx, tflag, C->tnew, nt, C->sums, C->misc + 1))) return rc;
        if ((rc = cx_scan_u32(ctx, C->vuse, C->vnew, nv, C->sums, C->misc + 2))) return rc;
        uint32_t h[2] = {0, 0};
        CX_HIP(ctx, hipMemcpyAsync(h, C->misc + 1, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        CX_HIP(ctx, hipStreamSynchronize(st));      // (also: the caller's keep bytes are on the device)
        nt2 = h[0]; nv2 = h[1];
        if (nt2 > nt || nv2 > nv) { ctx->err = "cx_level1_keep_components: the scans do not add up"; return CX_ERR_HIP; }
        if (nt2) {
            hipLaunchKernelGGL(cxc_k_keep_tri, cx_grid1(nt), dim3(256), 0, st, V.tri, (const uint32_t*)tflag, (const uint32_t*)C->tnew, (const uint32_t*)C->vnew,
                               V.parent, V.cflip, nt, nv, X.tri, X.parent, X.cflip);
            hipLaunchKernelGGL(cxc_k_keep_vert, cx_grid1(nv), dim3(256), 0, st, V.pts, V.keys, (const uint32_t*)C->vuse, (const uint32_t*)C->vnew, nv, X.pts, X.keys);
        } else
            nv2 = 0;
        CX_HIP(ctx, hipGetLastError());
        if ((rc = cx_level1_comp_commit(ctx, nv2, nt2, C->vuse, C->vnew))) return rc;
        C->gen_labels = ~0ULL; C->gen_table = ~0ULL;
    }
    if (out_counts) { out_counts[0] = nv2; out_counts[1] = nt2; out_counts[4] = kept; }
    return CX_OK;
}
