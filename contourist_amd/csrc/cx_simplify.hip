// cx_simplify.hip -- simplification of the Level-1 mesh by vertex clustering (include/contourist_hip.h, section "simplification").
//
// A vertex belongs to the cluster (cell of a lattice of `cell3` anchored at grid coordinate 0, component label); a cluster becomes one
// vertex at the exact mean of its members.  Kernels, in the order they run:
//   cxs_k_cluster       one lane per vertex: key -> slot of an open-addressing table, the slot's smallest member (its FIRST member)
//   cxs_k_first_flags   v == first[slot(v)], then cx_scan_u32: new vertex i = the cluster with the i-th smallest first member
//   cxs_k_map           cluster id of every old vertex; prio[id] = first member
//   cxs_k_remap_tri     triangles through the map, alive = three distinct indices (counted: out_counts[7]; the dry run ends here)
//   cxs_k_accumulate    one lane per vertex: fixed-point coordinates (and normals) added exactly into the cluster's accumulators
//   cxs_k_finish        one lane per cluster: the mean, rounded once; the normalised normal sum
// then the shared tail of the post-pass (cx_level1_simplify_tail in cx_post.hip): duplicate removal, clean, compaction, orientation.
// The table only maps keys to slots; the sums go into DENSE accumulators indexed by the cluster id (80 bytes per cluster instead of
// per slot of a table twice the vertex count).  Level-1 vertex order follows the march's tiles, so the lanes of a wave share a few
// clusters: lanes with the first active lane's key reduce among themselves and one lane touches memory (the leader loop of
// cxc_k_measure); all control flow around the cross-lane operations is wave-uniform.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>

#include "cx_ctx.h"
#include "cx_dev.h"

#define CXS_SMALL_GROUP 4
// accumulator words per cluster: members, three 128-bit coordinate sums {low, high}, three 64-bit normal sums
enum { CXS_W_N = 0, CXS_W_POS = 1, CXS_W_NRM = 7, CXS_WORDS = 10 };

extern "C" int cx_level1_component_labels(cx_ctx* ctx, void** tri_labels_dev, void** vert_labels_dev);
extern "C" int cx_level1_normals(cx_ctx* ctx, const double* delta3, void** normals_dev);

struct cx_simplify_state {
    cx_buf<u64> tkeys;                                   // cluster table: keys
    cx_buf<uint32_t> tfirst;                             // per slot: the smallest member
    cx_buf<uint32_t> vslot;                              // per vertex: its slot (CXD_NONE: dropped)
    cx_buf<uint32_t> flag;                               // first-member flags
    cx_buf<uint32_t> idx;                                // their exclusive scan
    cx_buf<uint32_t> sums;                               // block sums of the scan
    cx_buf<u64> acc;
    cx_buf<uint32_t> misc;                               // [0] clusters, [1] triangles with three distinct indices, [2] clamped coordinates
};

void cx_simplify_free(cx_ctx* ctx) {
    cx_simplify_state* Z = ctx->simp;
    if (!Z) return;
    delete Z;
    ctx->simp = nullptr;
}

struct cxs_params {
    double cell[3];
    double lo[3], hi[3];       // the box the coordinates are clamped to: [-1, corner + 1]
    long long kmin[3];         // floor(-1 / cell): the first cell of the grid box
    long long kn[3];           // cells of the grid box per axis
    double scale;              // 2^q
    int q;
    int by_component;
};

// ---- device helpers -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 cxs_shfl64(u64 v, int lane) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, lane), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), lane);
    return ((u64)hi << 32) | lo;
}
// cell of a coordinate: floor(p / c), an IEEE division; a point outside the grid box counts to the box's nearest cell
__device__ __forceinline__ long long cxs_cell(double p, double c, long long kmin, long long kn) {
    const double k = floor(p / c) - (double)kmin;
    if (!(k > 0.0)) return 0;
    return k >= (double)kn ? kn - 1 : (long long)k;
}
__device__ __forceinline__ u64 cxs_key(const double* __restrict__ p, int32_t label, const cxs_params& P) {
    const long long k0 = cxs_cell(p[0], P.cell[0], P.kmin[0], P.kn[0]);
    const long long k1 = cxs_cell(p[1], P.cell[1], P.kmin[1], P.kn[1]);
    const long long k2 = cxs_cell(p[2], P.cell[2], P.kmin[2], P.kn[2]);
    const u64 lin = (u64)((k0 * P.kn[1] + k1) * P.kn[2] + k2);                 // < 2^31 (checked on the host)
    return ((u64)(P.by_component ? (uint32_t)label : 0u) << 31) | lin;
}

// ---- clusters -----------------------------------------------------------------------------------------------------------------------
__global__ void cxs_k_table_init(u64* __restrict__ tkeys, uint32_t* __restrict__ tfirst, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) { tkeys[i] = CXD_EMPTY; tfirst[i] = CXD_NONE; }
}
// One lane per vertex.  The lanes of a wave that share a key are served by ONE probe sequence and one minimum (the leader is the
// group's lowest lane, so its vertex is the group's smallest).
__global__ __launch_bounds__(256) void cxs_k_cluster(const double* __restrict__ pts, const int32_t* __restrict__ vlab, uint32_t nv, cxs_params P,
                                                     u64* tkeys, uint32_t* tfirst, u64 mask, uint32_t* __restrict__ vslot) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t label = v < nv ? vlab[v] : -1;
    const bool active = v < nv && label >= 0;
    const u64 key = active ? cxs_key(pts + (size_t)v * 3, label, P) : 0ULL;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t myslot = CXD_NONE;
    uint64_t rem = __ballot(active);
    while (rem != 0ULL) {                                   // wave-uniform
        const int leader = __ffsll((long long)rem) - 1;
        const u64 k = cxs_shfl64(key, leader);
        const bool mine = active && key == k;
        rem &= ~__ballot(mine);
        uint32_t slot = 0;
        if ((int)lane == leader) {
            u64 s = cxd_mix(k) & mask;
            for (;;) {
                u64 cur = __hip_atomic_load(&tkeys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (cur == CXD_EMPTY) cur = atomicCAS(&tkeys[s], CXD_EMPTY, k);
                if (cur == CXD_EMPTY || cur == k) break;
                s = (s + 1) & mask;
            }
            slot = (uint32_t)s;
            if (__hip_atomic_load(&tfirst[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > v) atomicMin(&tfirst[s], v);
        }
        slot = (uint32_t)__shfl((int)slot, leader);
        if (mine) myslot = slot;
    }
    if (v < nv) vslot[v] = myslot;
}
__global__ void cxs_k_first_flags(const uint32_t* __restrict__ vslot, const uint32_t* __restrict__ tfirst, uint32_t nv, uint32_t* __restrict__ flag) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const uint32_t s = vslot[v];
    flag[v] = (s != CXD_NONE && tfirst[s] == v) ? 1u : 0u;
}
__global__ void cxs_k_map(const uint32_t* __restrict__ vslot, const uint32_t* __restrict__ tfirst, const uint32_t* __restrict__ idx, uint32_t nv,
                          int32_t* __restrict__ map, uint32_t* __restrict__ prio) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const uint32_t s = vslot[v];
    if (s == CXD_NONE) { map[v] = -1; return; }
    const uint32_t f = tfirst[s];
    const uint32_t id = idx[f];
    map[v] = (int32_t)id;
    if (f == v) prio[id] = v;
}
// triangles through the map, in their order and winding; tprio3 = the old triangle index (of several triangles that become the same
// vertex set the smallest one stays); alive = three distinct clusters
__global__ __launch_bounds__(256) void cxs_k_remap_tri(const int32_t* __restrict__ tri, const int32_t* __restrict__ map, uint32_t nt, uint32_t nv,
                                                       int32_t* __restrict__ tri2, uint32_t* __restrict__ tprio3, uint8_t* __restrict__ alive, uint32_t* count) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = false;
    if (t < nt) {
        const uint32_t a = (uint32_t)tri[(size_t)t * 3], b = (uint32_t)tri[(size_t)t * 3 + 1], c = (uint32_t)tri[(size_t)t * 3 + 2];
        const int32_t ma = a < nv ? map[a] : -1, mb = b < nv ? map[b] : -1, mc = c < nv ? map[c] : -1;
        ok = ma >= 0 && mb >= 0 && mc >= 0 && ma != mb && ma != mc && mb != mc;
        tri2[(size_t)t * 3] = ok ? ma : 0; tri2[(size_t)t * 3 + 1] = ok ? mb : 0; tri2[(size_t)t * 3 + 2] = ok ? mc : 0;
        tprio3[(size_t)t * 3] = t; tprio3[(size_t)t * 3 + 1] = t; tprio3[(size_t)t * 3 + 2] = t;
        alive[t] = ok ? 1 : 0;
    }
    const uint64_t m = __ballot(ok);
    if ((threadIdx.x & 63u) == 0u && m) atomicAdd(count, (uint32_t)__popcll(m));
}

// ---- exact means --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void cxs_lane_atomics(u64* w, u64 n, long long x0, long long x1, long long x2, bool nrm, long long n0, long long n1, long long n2) {
    atomicAdd(&w[CXS_W_N], n);
    cxd_add128(&w[CXS_W_POS], x0); cxd_add128(&w[CXS_W_POS + 2], x1); cxd_add128(&w[CXS_W_POS + 4], x2);
    if (nrm) {
        if (n0) atomicAdd(&w[CXS_W_NRM], (u64)n0);
        if (n1) atomicAdd(&w[CXS_W_NRM + 1], (u64)n1);
        if (n2) atomicAdd(&w[CXS_W_NRM + 2], (u64)n2);
    }
}
// One lane per vertex: X = llrint(clamp(x) * 2^q) per coordinate (|X| < 2^52: 64 lanes add up inside 64 bits), llrint(n * 2^30) per
// normal component.  The lanes of a wave that share a cluster reduce among themselves and one of them issues the atomics; groups of
// CXS_SMALL_GROUP lanes or fewer issue their own (six butterflies cost more).
__global__ __launch_bounds__(256) void cxs_k_accumulate(const double* __restrict__ pts, const double* __restrict__ nrm, const int32_t* __restrict__ map,
                                                        uint32_t nv, cxs_params P, u64* __restrict__ acc, uint32_t* clamped) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t id = v < nv ? map[v] : -1;
    const bool active = id >= 0;
    long long X[3] = {0, 0, 0}, N[3] = {0, 0, 0};
    uint32_t nclamp = 0;
    if (active) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            double x = pts[(size_t)v * 3 + a];
            if (!(x >= P.lo[a])) { x = P.lo[a]; nclamp++; }
            else if (x > P.hi[a]) { x = P.hi[a]; nclamp++; }
            X[a] = __double2ll_rn(x * P.scale);
            if (nrm) {
                double n = nrm[(size_t)v * 3 + a];
                n = n >= -1.0 ? (n <= 1.0 ? n : 1.0) : -1.0;        // (a unit normal; NaN -> -1 cannot occur for one)
                N[a] = __double2ll_rn(n * 1073741824.0);
            }
        }
    }
    if (__ballot(nclamp != 0u) != 0ULL) {                   // (never, for a mesh inside its grid box)
        if (nclamp) atomicAdd(clamped, nclamp);
    }
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t rem = __ballot(active);
    while (rem != 0ULL) {                                   // wave-uniform
        const int leader = __ffsll((long long)rem) - 1;
        const int32_t k = __shfl(id, leader);
        const bool mine = active && id == k;
        const uint64_t grp = __ballot(mine);
        rem &= ~grp;
        if (__popcll(grp) <= CXS_SMALL_GROUP) {
            if (mine) cxs_lane_atomics(acc + (size_t)k * CXS_WORDS, 1ULL, X[0], X[1], X[2], nrm != nullptr, N[0], N[1], N[2]);
            continue;
        }
        const long long s0 = cxd_wave_add(mine ? X[0] : 0LL), s1 = cxd_wave_add(mine ? X[1] : 0LL), s2 = cxd_wave_add(mine ? X[2] : 0LL);
        long long m0 = 0, m1 = 0, m2 = 0;
        if (nrm) { m0 = cxd_wave_add(mine ? N[0] : 0LL); m1 = cxd_wave_add(mine ? N[1] : 0LL); m2 = cxd_wave_add(mine ? N[2] : 0LL); }   // (nrm: uniform)
        if ((int)lane == leader) cxs_lane_atomics(acc + (size_t)k * CXS_WORDS, (u64)__popcll(grp), s0, s1, s2, nrm != nullptr, m0, m1, m2);
    }
}
// one lane per cluster: double(sum) rounded once, / double(n), * 2^-q; the normal sum normalised in float64 ((0,0,0) for a zero sum)
__global__ void cxs_k_finish(const u64* __restrict__ acc, uint32_t ncl, cxs_params P, double* __restrict__ pts2, double* __restrict__ nrm2) {
#pragma clang fp contract(off)
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncl) return;
    const u64* w = acc + (size_t)c * CXS_WORDS;
    const double n = (double)w[CXS_W_N];
    const double inv = ldexp(1.0, -P.q);
#pragma unroll
    for (int a = 0; a < 3; a++) pts2[(size_t)c * 3 + a] = (cxd_to_double128(w[CXS_W_POS + 2 * a], w[CXS_W_POS + 2 * a + 1], 0) / n) * inv;
    if (nrm2) {
        const double x = (double)(long long)w[CXS_W_NRM], y = (double)(long long)w[CXS_W_NRM + 1], z = (double)(long long)w[CXS_W_NRM + 2];
        const double len = sqrt(x * x + y * y + z * z);
        nrm2[(size_t)c * 3] = len > 0.0 ? x / len : 0.0;
        nrm2[(size_t)c * 3 + 1] = len > 0.0 ? y / len : 0.0;
        nrm2[(size_t)c * 3 + 2] = len > 0.0 ? z / len : 0.0;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// cells of the grid box for `cell3`; false when the product reaches 2^31
static bool cxs_cells(const double corner[3], const double cell3[3], long long kmin[3], long long kn[3]) {
    double prod = 1.0;
    for (int a = 0; a < 3; a++) {
        const double lo = std::floor(-1.0 / cell3[a]), hi = std::floor((corner[a] + 1.0) / cell3[a]);
        const double n = hi - lo + 1.0;
        if (!(n >= 1.0) || !(n < 2147483648.0)) return false;
        kmin[a] = (long long)lo; kn[a] = (long long)n;
        prod *= n;
    }
    return prod < 2147483648.0;
}

extern "C" int cx_level1_simplify(cx_ctx* ctx, const double* cell3, uint32_t flags, int64_t* out_counts, double* q_out) {
    if (!ctx) return CX_ERR_INVALID;
    cx_level1_comp_view V;
    CX_HIP(ctx, hipSetDevice(ctx->device));
    int rc = cx_level1_comp_view_get(ctx, "cx_level1_simplify", &V);
    if (rc) return rc;
    if (!cell3 || (flags & ~15u)) { ctx->err = "cx_level1_simplify: three cell sizes and flags of CX_SIMPLIFY_* are needed"; return CX_ERR_INVALID; }
    for (int a = 0; a < 3; a++)
        if (!(cell3[a] > 0.0) || !std::isfinite(cell3[a])) { ctx->err = "cx_level1_simplify: the cell sizes must be positive and finite"; return CX_ERR_INVALID; }
    cxs_params P;
    double cmax = 0.0;
    for (int a = 0; a < 3; a++) {
        P.cell[a] = cell3[a];
        P.lo[a] = -1.0; P.hi[a] = V.corner[a] + 1.0;
        cmax = std::max(cmax, V.corner[a]);
    }
    if (!cxs_cells(V.corner, cell3, P.kmin, P.kn)) {
        // the smallest admissible uniform cell, by bisection (the count falls as the cell grows)
        double lo = 0.0, hi = cmax + 2.0;      // (one cell per axis and its two neighbours: admissible)
        for (int it = 0; it < 60; it++) {
            const double mid = 0.5 * (lo + hi), c3[3] = {mid, mid, mid};
            long long km[3], kn[3];
            if (mid > 0.0 && cxs_cells(V.corner, c3, km, kn)) hi = mid; else lo = mid;
        }
        char msg[256];
        snprintf(msg, sizeof(msg), "cx_level1_simplify: the cells of the grid box must number fewer than 2^31; the smallest admissible cell (all axes) is %.9g", hi);
        ctx->err = msg;
        return CX_ERR_INVALID;
    }
    {   // q = 52 - ceil(log2(max corner + 2)): |x| <= corner + 1 < 2^(52 - q)
        int e = 0;
        const double m = std::frexp(cmax + 2.0, &e);       // cmax + 2 = m 2^e, 0.5 <= m < 1
        P.q = 52 - (m == 0.5 ? e - 1 : e);
        P.scale = std::ldexp(1.0, P.q);
    }
    P.by_component = (flags & 2u) ? 0 : 1;
    const bool count_only = (flags & 4u) != 0u, want_normals = (flags & 8u) != 0u && !count_only;
    const uint32_t nv = V.nv, nt = V.nt;
    hipStream_t st = ctx->stream;
    if (!ctx->simp) ctx->simp = new (std::nothrow) cx_simplify_state();
    if (!ctx->simp) return CX_ERR_NOMEM;
    cx_simplify_state* Z = ctx->simp;
    cx_level1_simplify_io B;
    // the source's normals first: where they cannot be served nothing has been touched
    const double* nsrc = nullptr;
    if ((flags & 8u) != 0u) {
        const double* carried = nullptr;
        uint32_t nvc = 0;
        const int mode = cx_level1_carried_normals(ctx, &carried, &nvc);
        if (mode == 2) { ctx->err = "cx_level1_simplify: CX_SIMPLIFY_NORMALS on a mesh that was simplified without it: it carries no normals"; return CX_ERR_UNSUPPORTED; }
        if (mode == 1) nsrc = carried;
        else if (!count_only) {
            void* dev = nullptr;
            if ((rc = cx_level1_normals(ctx, nullptr, &dev))) return rc;
            nsrc = (const double*)dev;
        } else {
            cx_level1_view A;
            if ((rc = cx_level1_attr_view(ctx, "cx_level1_simplify", &A))) return rc;
        }
    }
    void *tl = nullptr, *vl = nullptr;
    if ((rc = cx_level1_component_labels(ctx, &tl, &vl))) return rc;
    if ((rc = cx_level1_simplify_bufs(ctx, want_normals, count_only, &B))) return rc;
    const u64 tsz = cx_table_size(nv);
    if ((rc = Z->misc.grow(ctx, 16))) return rc;
    if ((rc = Z->tkeys.grow(ctx, (size_t)tsz))) return rc;
    if ((rc = Z->tfirst.grow(ctx, (size_t)tsz))) return rc;
    if ((rc = Z->vslot.grow(ctx, (size_t)nv + 16))) return rc;
    if ((rc = Z->flag.grow(ctx, (size_t)nv + 16))) return rc;
    if ((rc = Z->idx.grow(ctx, (size_t)nv + 16))) return rc;
    if ((rc = Z->sums.grow(ctx, (size_t)nv / 1024 + 16))) return rc;
    CX_HIP(ctx, hipMemsetAsync(Z->misc, 0, 16 * sizeof(uint32_t), st));
    uint32_t ncl = 0, n3 = 0, nclamp = 0;
    if (nv) {
        hipLaunchKernelGGL(cxs_k_table_init, dim3(2048), dim3(256), 0, st, Z->tkeys, Z->tfirst, (size_t)tsz);
        hipLaunchKernelGGL(cxs_k_cluster, cx_grid1(nv), dim3(256), 0, st, V.pts, (const int32_t*)vl, nv, P, Z->tkeys, Z->tfirst, tsz - 1, Z->vslot);
        hipLaunchKernelGGL(cxs_k_first_flags, cx_grid1(nv), dim3(256), 0, st, (const uint32_t*)Z->vslot, (const uint32_t*)Z->tfirst, nv, Z->flag);
        if ((rc = cx_scan_u32(ctx, Z->flag, Z->idx, nv, Z->sums, Z->misc))) return rc;
        hipLaunchKernelGGL(cxs_k_map, cx_grid1(nv), dim3(256), 0, st, (const uint32_t*)Z->vslot, (const uint32_t*)Z->tfirst, (const uint32_t*)Z->idx, nv, B.map, B.prio);
        if (nt) hipLaunchKernelGGL(cxs_k_remap_tri, cx_grid1(nt), dim3(256), 0, st, V.tri, (const int32_t*)B.map, nt, nv, B.tri, B.tprio3, B.alive, Z->misc + 1);
        uint32_t h[2] = {0, 0};
        CX_HIP(ctx, hipMemcpyAsync(h, Z->misc, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        CX_HIP(ctx, hipStreamSynchronize(st));
        ncl = h[0]; n3 = h[1];
        if (ncl > nv || n3 > nt) { ctx->err = "cx_level1_simplify: the scans do not add up"; return CX_ERR_HIP; }
    }
    CX_HIP(ctx, hipGetLastError());
    if (q_out) *q_out = (double)P.q;
    if (count_only) {
        if (out_counts) { out_counts[6] = ncl; out_counts[7] = n3; }
        return CX_OK;
    }
    if (ncl) {
        if ((rc = Z->acc.grow(ctx, (size_t)ncl * CXS_WORDS + 16))) return rc;
        CX_HIP(ctx, hipMemsetAsync(Z->acc, 0, (size_t)ncl * CXS_WORDS * sizeof(u64), st));
        hipLaunchKernelGGL(cxs_k_accumulate, cx_grid1(nv), dim3(256), 0, st, V.pts, want_normals ? nsrc : (const double*)nullptr, (const int32_t*)B.map, nv, P, Z->acc,
                           Z->misc + 2);
        hipLaunchKernelGGL(cxs_k_finish, cx_grid1(ncl), dim3(256), 0, st, (const u64*)Z->acc, ncl, P, B.pts, want_normals ? B.nrm_new : (double*)nullptr);
        CX_HIP(ctx, hipMemcpyAsync(&nclamp, Z->misc + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        CX_HIP(ctx, hipGetLastError());
    }
    int64_t counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if ((rc = cx_level1_simplify_tail(ctx, nv, ncl, nt, !(flags & 1u), want_normals, counts))) return rc;      // (synchronises the stream)
    counts[5] = nclamp; counts[6] = ncl; counts[7] = n3;
    if (out_counts) memcpy(out_counts, counts, sizeof(counts));
    return CX_OK;
}

extern "C" int cx_level1_simplify_map(cx_ctx* ctx, void** new_index_of_old_vertex_dev) {
    if (!ctx || !new_index_of_old_vertex_dev) return CX_ERR_INVALID;
    const int32_t* map = nullptr;
    uint32_t n = 0;
    const int rc = cx_level1_simplify_map_get(ctx, &map, &n);
    if (rc) return rc;
    *new_index_of_old_vertex_dev = n ? (void*)map : nullptr;
    return CX_OK;
}

extern "C" int cx_level1_simplify_map_download(cx_ctx* ctx, int32_t* new_index_of_old_vertex) {
    if (!ctx) return CX_ERR_INVALID;
    const int32_t* map = nullptr;
    uint32_t n = 0;
    const int rc = cx_level1_simplify_map_get(ctx, &map, &n);
    if (rc || !n) return rc;
    if (!new_index_of_old_vertex) return CX_ERR_INVALID;
    CX_HIP(ctx, hipSetDevice(ctx->device));
    return cx_copy_to_host1(ctx, new_index_of_old_vertex, map, (size_t)n * sizeof(int32_t));
}
