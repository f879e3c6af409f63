// cx_post.hip -- the 3-D Level-1 post-pass on the device (surface-sized work): weld, tiny collapse, clean, compaction, orientation,
// sharded Level 1, smoothing; cx_surface_geometry on a caller's mesh; and the views through which cx_attr.hip, cx_comp.hip,
// cx_simplify.hip and cx_clip.hip read and write the Level-1 state.  The state itself and what the sibling files share: cx_post.h
// (cx_write.hip: mesh files, cx_post4d.hip: the 4-D post-pass, cx_morph.hip: morph triangles and the per-t stream).
//
// Reference semantics restated (paths relative to the reference checkout, contourist/...):
//   quantize_interpolations   tetrahedral.py:190-215      weld by bucket trunc(p * int(10000/corner))
//   remove_tiny_simplices     tetrahedral.py:353-375      drop tiny triangles, move their vertices together
//   extract_surface_geometry  tetrahedral.py:604-621      compact used vertices
//   clean_triangles           surface_geometry.py:14-50   drop zero-area triangles, merge their coincident vertices
//   orient_triangles          surface_geometry.py:52-140  per component: max-x start rule + edge flood fill
// Where the reference's result depends on Python set/dict order, a canonical choice is made (the
// member with the smallest priority -- edge id in the pipeline, index for a caller's mesh --
// represents a weld bucket / merge group; of triangles that become the same vertex set the one
// with the smallest sorted priority triple survives).  oracle/postpass.py restates the same choices.
//
// Building blocks: open-addressing hash tables (64-bit keys, atomicCAS), lock-free union-find
// (root = smallest priority; a parity bit per link carries the relative winding for the
// orientation flood fill), pointer jumping, a three-kernel exclusive scan.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "cx_post.h"
#include "cx_state4.h"

void cx_post_free(cx_ctx* ctx) {
    if (!ctx->post) return;
    cx_post_state* S = ctx->post;
    if (S->me_pinned) (void)hipHostFree(S->me_pinned);
    delete S;
    ctx->post = nullptr;
}

// ---- device helpers --------------------------------------------------------------------------------
__global__ void cxp_k_iota64(u64* a, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = (u64)i;
}
__global__ void cxp_k_fill64(u64* a, size_t n, u64 v) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) a[i] = v;
}
// pointer jumping with parity until every node points at its root
__global__ void cxp_k_jump(u64* parent, uint32_t n, uint32_t* changed) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u64 w = parent[i];
    uint32_t p = (uint32_t)w;
    if (p == i) return;
    bool moved = false;
#pragma unroll 1
    for (int hop = 0; hop < 3; hop++) {          // up to three hops per launch: fewer launches and host round trips
        const u64 wp = parent[p];
        const uint32_t pp = (uint32_t)wp;
        if (pp == p) break;
        w = ((((w >> 32) ^ (wp >> 32)) & 1ULL) << 32) | (u64)pp;
        p = pp;
        moved = true;
    }
    if (moved) {
        parent[i] = w;
        *changed = 1u;
    }
}

// ---- exclusive scan of u32 (n up to 2^32) ----------------------------------------------------------
#define CXP_SCAN_BLOCK 1024u
__global__ __launch_bounds__(256) void cxp_k_scan_blocks(const uint32_t* in, uint32_t* out, uint32_t* sums, uint32_t n) {
    __shared__ uint32_t s[256];
    const uint32_t base = blockIdx.x * CXP_SCAN_BLOCK + threadIdx.x * 4u;
    uint32_t v[4], t = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        v[k] = (base + k < n) ? in[base + k] : 0u;
        t += v[k];
    }
    s[threadIdx.x] = t;
    __syncthreads();
    for (uint32_t o = 1; o < 256; o <<= 1) {
        const uint32_t x = (threadIdx.x >= o) ? s[threadIdx.x - o] : 0u;
        __syncthreads();
        s[threadIdx.x] += x;
        __syncthreads();
    }
    uint32_t run = s[threadIdx.x] - t;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (base + k < n) out[base + k] = run;
        run += v[k];
    }
    if (threadIdx.x == 255) sums[blockIdx.x] = s[255];
}
// one workgroup turns the block sums into exclusive offsets: 16 consecutive sums per thread, 16384 per pass
#define CXP_SUMS_PER_THREAD 16u
__device__ __forceinline__ void cxp_scan_sums_body(uint32_t* sums, uint32_t nb, uint32_t* total, unsigned long long* total64);
// two arrays in one launch (cx_morph_eval: the block counts of the segments and of the triangles), a workgroup each
__global__ __launch_bounds__(1024) void cxp_k_scan_sums2(uint32_t* sums_a, uint32_t na, uint32_t* total_a, uint32_t* sums_b, uint32_t nb, uint32_t* total_b) {
    if (blockIdx.x == 0) cxp_scan_sums_body(sums_a, na, total_a, nullptr);
    else cxp_scan_sums_body(sums_b, nb, total_b, nullptr);
}
__global__ __launch_bounds__(1024) void cxp_k_scan_sums(uint32_t* sums, uint32_t nb, uint32_t* total, unsigned long long* total64) {
    cxp_scan_sums_body(sums, nb, total, total64);
}
__device__ __forceinline__ void cxp_scan_sums_body(uint32_t* sums, uint32_t nb, uint32_t* total, unsigned long long* total64) {
    __shared__ uint32_t s[1024];
    uint32_t carry = 0;
    unsigned long long wide = 0;   // the same total without the wrap at 2^32 (each pass adds less than 2^32)
    for (uint32_t base = 0; base < nb; base += 1024u * CXP_SUMS_PER_THREAD) {
        const uint32_t i0 = base + threadIdx.x * CXP_SUMS_PER_THREAD;
        uint32_t v[CXP_SUMS_PER_THREAD], t = 0;
#pragma unroll
        for (uint32_t k = 0; k < CXP_SUMS_PER_THREAD; k++) {
            v[k] = (i0 + k < nb) ? sums[i0 + k] : 0u;
            t += v[k];
        }
        s[threadIdx.x] = t;
        __syncthreads();
        for (uint32_t o = 1; o < 1024; o <<= 1) {
            const uint32_t x = (threadIdx.x >= o) ? s[threadIdx.x - o] : 0u;
            __syncthreads();
            s[threadIdx.x] += x;
            __syncthreads();
        }
        uint32_t run = carry + s[threadIdx.x] - t;
#pragma unroll
        for (uint32_t k = 0; k < CXP_SUMS_PER_THREAD; k++) {
            if (i0 + k < nb) sums[i0 + k] = run;
            run += v[k];
        }
        const uint32_t passtot = s[1023];
        __syncthreads();
        carry += passtot;
        wide += (unsigned long long)passtot;
    }
    if (threadIdx.x == 0) {
        *total = carry;
        if (total64) *total64 = wide;
    }
}
__global__ void cxp_k_scan_add(uint32_t* out, const uint32_t* sums, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] += sums[i / CXP_SCAN_BLOCK];
}

// ---- step kernels -------------------------------------------------------------------------------------
// float64 vertex coordinates exactly as the reference computes them (tetrahedral.py:471-487)
struct cxp_origin3 {
    double o[3];   // lattice coordinates of sample (0,0,0) in the whole volume (cx_set_origin), or zeros
};
template <int DT>   // the sample type of the grid (its samples convert to fp32, and so to float64, exactly)
__global__ void cxp_k_vertices_f64(const cx_grid_ref A, const double* __restrict__ A64, uint32_t n1, uint32_t n2, cx_fdiv dplane, cx_fdiv drow,
                                   double value, const cx_vrec* __restrict__ verts, uint32_t nv, double* pts, uint32_t* prio, cxp_origin3 org) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const uint32_t key = verts[v].x;
    const uint32_t lin = key >> 3, d = key & 7u;
    const uint32_t plane = n1 * n2;
    const uint32_t i = cx_div(lin, dplane);
    const uint32_t r = lin - i * plane;
    const uint32_t j = cx_div(r, drow);
    const uint32_t k = r - j * n2;
    const uint32_t lin2 = lin + ((d & 4u) ? plane : 0u) + ((d & 2u) ? n2 : 0u) + (d & 1u);
    const double f0 = A64 ? A64[lin] : (double)cx_sample<DT>(A, lin), f1 = A64 ? A64[lin2] : (double)cx_sample<DT>(A, lin2);
    const bool owner_low = !(f0 > f1);             // reference swaps when flow > fhigh
    const double flow = owner_low ? f0 : f1, fhigh = owner_low ? f1 : f0;
    double ratio = 0.5;
    const double den = 1.0 * (fhigh - flow);
    if (!(fabs(den) <= 1e-8)) ratio = (value - flow) / den;
    const double q[3] = {(double)i + org.o[0], (double)j + org.o[1], (double)k + org.o[2]};   // integers: exact
    const uint32_t db[3] = {(d >> 2) & 1u, (d >> 1) & 1u, d & 1u};
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double low = owner_low ? q[a] : q[a] + (double)db[a];
        const double high = owner_low ? q[a] + (double)db[a] : q[a];
        pts[(size_t)v * 3 + a] = low + ratio * (high - low);
    }
    prio[v] = key;
}
template <typename... Args>
static void cxp_launch_vertices_f64(dim3 grid, hipStream_t st, const cx_grid_ref& A, Args... args) {
#define CX_LAUNCH(DT) hipLaunchKernelGGL((cxp_k_vertices_f64<DT>), grid, dim3(256), 0, st, A, args...);
    CX_DISPATCH_DTYPE(A.dtype, CX_LAUNCH)
#undef CX_LAUNCH
}

__global__ void cxp_k_iota_prio(uint32_t* prio, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) prio[i] = i;
}

struct cxp_weld_params {
    double ex[3];
    double thr;   // > 0: vertices are crossings of the march (priority = edge id); those further than thr from both ends of their
                  // lattice edge cannot share a bucket with another crossing (see cxp_weld_alone)
};
// Crossings sit on edges of the Kuhn lattice (one per edge).  Two of them in one weld bucket are less than 1/ex apart in every
// axis.  Edges without a common end point stay at least 1/3 apart (max-norm; checked over all pairs of edge directions), edges
// with a common end point V run apart from it along some axis -- so one of the two crossings is within 1/ex of V and the other
// within 2/ex.  A crossing at least 2/ex from both ends of its edge is therefore ALONE in its bucket (ex >= 16): it is its own
// representative and does not have to go through the table (at 512^3: 4 of 5 vertices).
__device__ __forceinline__ bool cxp_weld_alone(const double* p, uint32_t key, const cxp_weld_params& W) {
    if (!(W.thr > 0.0)) return false;
    const uint32_t d = key & 7u;
    const double x = (d & 4u) ? p[0] : ((d & 2u) ? p[1] : p[2]);   // an axis the edge moves along
    const double u = x - floor(x);
    return u > W.thr && u < 1.0 - W.thr;
}
// weld bucket of a point: trunc(p * expander) per axis as the reference's astype(int) does it (tetrahedral.py:192-196),
// i.e. TOWARDS ZERO: on an array with a rim around the reference's grid the coordinates are the reference's own and
// may be negative, and (-1/ex, 0) shares bucket 0 with [0, 1/ex).  Biased by 2^20 per axis so the fields stay unsigned.
__device__ __forceinline__ u64 cxp_weld_key(const double* p, const cxp_weld_params& W) {
    const u64 q0 = (u64)((long long)(p[0] * W.ex[0]) + (1LL << 20));
    const u64 q1 = (u64)((long long)(p[1] * W.ex[1]) + (1LL << 20));
    const u64 q2 = (u64)((long long)(p[2] * W.ex[2]) + (1LL << 20));
    return (q0 << 42) | (q1 << 21) | q2;
}

// weld: bucket -> vertex with the LARGEST priority (= largest edge key).  The members of a bucket are crossings on the
// upward edges of one lattice point (truncation puts everything in [V, V + 1/expander)^3 together), so the largest key
// is the most diagonal edge -- the one the reference's "last inserted wins" (tetrahedral.py:198-203) picks most often,
// because an edge shared by fewer voxels is first met later (probe on the corner = 511 fixture: 56 of 112 buckets
// agree, against 15 of 112 for the smallest key; tiny-collapse counts then fall inside the reference's own band)
__global__ void cxp_k_weld_insert(const double* pts, const uint32_t* prio, uint32_t nv, cxp_weld_params W, u64* tkeys, u64* tvals,
                                  u64 mask, const uint8_t* vkeep) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    if (vkeep && !vkeep[v]) return;   // seeded selection: vertices of dropped components do not exist
    if (cxp_weld_alone(pts + (size_t)v * 3, prio[v], W)) return;
    const u64 key = cxp_weld_key(pts + (size_t)v * 3, W);
    u64 slot = cxd_mix(key) & mask;
    for (;;) {
        const u64 cur = atomicCAS(&tkeys[slot], CXD_EMPTY, key);
        if (cur == CXD_EMPTY || cur == key) break;
        slot = (slot + 1) & mask;
    }
    atomicMax(&tvals[slot], ((u64)prio[v] << 32) | (u64)v);
}
__global__ void cxp_k_weld_lookup(const double* pts, uint32_t nv, cxp_weld_params W, const u64* tkeys, const u64* tvals, u64 mask,
                                  uint32_t* rep, const uint8_t* vkeep, const uint32_t* prio) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    if (vkeep && !vkeep[v]) { rep[v] = v; return; }
    if (cxp_weld_alone(pts + (size_t)v * 3, prio[v], W)) { rep[v] = v; return; }
    const u64 key = cxp_weld_key(pts + (size_t)v * 3, W);
    u64 slot = cxd_mix(key) & mask;
    while (tkeys[slot] != key) slot = (slot + 1) & mask;
    rep[v] = (uint32_t)tvals[slot];
}

// remap triangles through `map` (optionally a union-find: map == nullptr), kill those with < 3 distinct vertices.
// involved (optional): flags the vertices something was merged INTO.  Two different triangles of the march can only become the
// same vertex set through a merge, and then both contain such a vertex: the dedupe that follows only has to look at triangles
// with a flagged vertex (a few per cent of a mesh) instead of putting all of them through its table of compare-and-swaps.
// ever (optional): the same flags, never cleared between the stages -- an edge of the march's mesh can only come to lie on more than
// two triangles through such a vertex (cxp_k_edges_block).
__global__ void cxp_k_remap(int32_t* tri, uint8_t* alive, uint32_t nt, const uint32_t* map, const u64* parent, uint8_t* involved = nullptr,
                            uint8_t* ever = nullptr) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt || !alive[t]) return;
    // the three indices, then the three look-ups, then the stores: written as one loop -- load, look up, store -- every load waited
    // for the store before it (they may alias as far as the compiler knows): seven round trips one after the other per triangle
    const uint32_t x[3] = {(uint32_t)tri[(size_t)t * 3], (uint32_t)tri[(size_t)t * 3 + 1], (uint32_t)tri[(size_t)t * 3 + 2]};
    uint32_t v[3];
    if (map) {
        v[0] = map[x[0]]; v[1] = map[x[1]]; v[2] = map[x[2]];
    } else {
        uint32_t par;
#pragma unroll
        for (int s = 0; s < 3; s++) v[s] = cxp_find(parent, x[s], par);
    }
#pragma unroll
    for (int s = 0; s < 3; s++) {
        if (v[s] != x[s]) {
            tri[(size_t)t * 3 + s] = (int32_t)v[s];
            if (involved) involved[v[s]] = 1;
            if (ever) ever[v[s]] = 1;
        }
    }
    if (v[0] == v[1] || v[0] == v[2] || v[1] == v[2]) alive[t] = 0;
}

// priority of a triangle = its sorted triple of ORIGINAL vertex priorities (compared lexicographically)
struct cxp_tri3 {
    uint32_t a, b, c;
};
__device__ __forceinline__ cxp_tri3 cxp_sorted3(uint32_t x, uint32_t y, uint32_t z) {
    if (x > y) { const uint32_t t = x; x = y; y = t; }
    if (y > z) { const uint32_t t = y; y = z; z = t; }
    if (x > y) { const uint32_t t = x; x = y; y = t; }
    cxp_tri3 r = {x, y, z};
    return r;
}
__device__ __forceinline__ bool cxp_less3(const cxp_tri3& p, const cxp_tri3& q) {
    if (p.a != q.a) return p.a < q.a;
    if (p.b != q.b) return p.b < q.b;
    return p.c < q.c;
}

// dedupe triangles that are the same vertex set: table slot holds the id of the current winner
__global__ void cxp_k_dedupe_insert(const int32_t* tri, const uint32_t* tprio3, const uint8_t* alive, uint32_t nt, u64* table,
                                    u64 mask, const uint8_t* involved = nullptr) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt || !alive[t]) return;
    if (involved && !(involved[tri[(size_t)t * 3]] | involved[tri[(size_t)t * 3 + 1]] | involved[tri[(size_t)t * 3 + 2]])) return;   // cannot have a twin
    const cxp_tri3 me = cxp_sorted3((uint32_t)tri[(size_t)t * 3], (uint32_t)tri[(size_t)t * 3 + 1], (uint32_t)tri[(size_t)t * 3 + 2]);
    const cxp_tri3 mp = {tprio3[(size_t)t * 3], tprio3[(size_t)t * 3 + 1], tprio3[(size_t)t * 3 + 2]};
    u64 slot = cxd_mix(((u64)me.a << 40) ^ ((u64)me.b << 20) ^ (u64)me.c ^ ((u64)me.c << 50)) & mask;
    for (;;) {
        u64 cur = atomicCAS(&table[slot], CXD_EMPTY, (u64)t);
        if (cur == CXD_EMPTY) return;
        for (;;) {   // slot occupied by triangle `cur`: same vertex set?
            const uint32_t o = (uint32_t)cur;
            const cxp_tri3 ot = cxp_sorted3((uint32_t)tri[(size_t)o * 3], (uint32_t)tri[(size_t)o * 3 + 1], (uint32_t)tri[(size_t)o * 3 + 2]);
            if (ot.a != me.a || ot.b != me.b || ot.c != me.c) break;   // different set: probe on
            const cxp_tri3 op = {tprio3[(size_t)o * 3], tprio3[(size_t)o * 3 + 1], tprio3[(size_t)o * 3 + 2]};
            if (!cxp_less3(mp, op)) return;                            // the resident wins
            const u64 seen = atomicCAS(&table[slot], cur, (u64)t);
            if (seen == cur) return;                                   // replaced it
            cur = seen;                                                // someone else got in: compare again
        }
        slot = (slot + 1) & mask;
    }
}
__global__ void cxp_k_dedupe_resolve(const int32_t* tri, uint8_t* alive, uint32_t nt, const u64* table, u64 mask, const uint8_t* involved = nullptr) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt || !alive[t]) return;
    if (involved && !(involved[tri[(size_t)t * 3]] | involved[tri[(size_t)t * 3 + 1]] | involved[tri[(size_t)t * 3 + 2]])) return;   // was not inserted
    const cxp_tri3 me = cxp_sorted3((uint32_t)tri[(size_t)t * 3], (uint32_t)tri[(size_t)t * 3 + 1], (uint32_t)tri[(size_t)t * 3 + 2]);
    u64 slot = cxd_mix(((u64)me.a << 40) ^ ((u64)me.b << 20) ^ (u64)me.c ^ ((u64)me.c << 50)) & mask;
    for (;;) {
        const uint32_t o = (uint32_t)table[slot];
        if (o == t) return;
        const cxp_tri3 ot = cxp_sorted3((uint32_t)tri[(size_t)o * 3], (uint32_t)tri[(size_t)o * 3 + 1], (uint32_t)tri[(size_t)o * 3 + 2]);
        if (ot.a == me.a && ot.b == me.b && ot.c == me.c) { alive[t] = 0; return; }
        slot = (slot + 1) & mask;
    }
}

// original priority triple of every triangle (sorted), taken before any remap
__global__ void cxp_k_tri_prio(const int32_t* tri, const uint32_t* prio, uint32_t nt, uint32_t* tprio3) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const cxp_tri3 p = cxp_sorted3(prio[tri[(size_t)t * 3]], prio[tri[(size_t)t * 3 + 1]], prio[tri[(size_t)t * 3 + 2]]);
    tprio3[(size_t)t * 3] = p.a; tprio3[(size_t)t * 3 + 1] = p.b; tprio3[(size_t)t * 3 + 2] = p.c;
}

__global__ __launch_bounds__(256) void cxp_k_count_alive(const uint8_t* alive, uint32_t nt, uint32_t* counter) {
    __shared__ uint32_t s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    uint32_t n = 0;
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < nt; t += gridDim.x * blockDim.x) n += alive[t] ? 1u : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += (uint32_t)__shfl_xor((int)n, o);
    if ((threadIdx.x & 63u) == 0 && n) atomicAdd(&s_n, n);
    __syncthreads();
    if (threadIdx.x == 0 && s_n) atomicAdd(counter, s_n);
}

// tiny triangles (tetrahedral.py:360-365): bbox * (1/corner) < epsilon on every axis
__global__ void cxp_k_tiny(const int32_t* tri, uint8_t* alive, uint32_t nt, const double* pts, double ic0, double ic1, double ic2,
                           double eps, u64* parent, const uint32_t* prio, uint8_t* moved) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt || !alive[t]) return;
    const uint32_t v0 = tri[(size_t)t * 3], v1 = tri[(size_t)t * 3 + 1], v2 = tri[(size_t)t * 3 + 2];
    const double ic[3] = {ic0, ic1, ic2};
    double worst = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double x0 = pts[(size_t)v0 * 3 + a], x1 = pts[(size_t)v1 * 3 + a], x2 = pts[(size_t)v2 * 3 + a];
        const double d = (fmax(x0, fmax(x1, x2)) - fmin(x0, fmin(x1, x2))) * ic[a];
        worst = fmax(worst, d);
    }
    if (worst < eps) {
        alive[t] = 0;
        cxp_union(parent, prio, v0, v1, 0);
        cxp_union(parent, prio, v0, v2, 0);
        moved[v0] = moved[v1] = moved[v2] = 1;
    }
}
// members of a tiny group take the coordinates of the group's root (tetrahedral.py:368-370, canonical root)
__global__ void cxp_k_move(double* pts, const double* pts_src, const u64* parent, const uint8_t* moved, uint32_t nv) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv || !moved[v]) return;
    uint32_t par;
    const uint32_t r = cxp_find(parent, v, par);
#pragma unroll
    for (int a = 0; a < 3; a++) pts[(size_t)v * 3 + a] = pts_src[(size_t)r * 3 + a];
}

// zero-area triangles (surface_geometry.py:33-43): drop, and merge their np.allclose vertex pairs
__global__ void cxp_k_degenerate(const int32_t* tri, uint8_t* alive, uint32_t nt, const double* pts, u64* parent, const uint32_t* prio) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt || !alive[t]) return;
    const uint32_t v[3] = {(uint32_t)tri[(size_t)t * 3], (uint32_t)tri[(size_t)t * 3 + 1], (uint32_t)tri[(size_t)t * 3 + 2]};
    double P[3][3];
#pragma unroll
    for (int s = 0; s < 3; s++)
#pragma unroll
        for (int a = 0; a < 3; a++) P[s][a] = pts[(size_t)v[s] * 3 + a];
    const double ux = P[0][0] - P[2][0], uy = P[0][1] - P[2][1], uz = P[0][2] - P[2][2];   // A - C
    const double wx = P[1][0] - P[2][0], wy = P[1][1] - P[2][1], wz = P[1][2] - P[2][2];   // B - C
    const double cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx;
    if (fabs(cx) <= 1e-8 && fabs(cy) <= 1e-8 && fabs(cz) <= 1e-8) {
        alive[t] = 0;
        const int pr[3][2] = {{0, 1}, {0, 2}, {1, 2}};
#pragma unroll
        for (int e = 0; e < 3; e++) {
            const int i = pr[e][0], j = pr[e][1];
            bool close = true;
#pragma unroll
            for (int a = 0; a < 3; a++) close = close && (fabs(P[i][a] - P[j][a]) <= 1e-8 + 1e-5 * fabs(P[j][a]));
            if (close) cxp_union(parent, prio, v[i], v[j], 0);
        }
    }
}

__global__ void cxp_k_alive_u32(const uint8_t* alive, uint32_t nt, uint32_t* out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < nt) out[t] = alive[t] ? 1u : 0u;
}
// ---- ordered compaction without materialised scans (Level 1 of the 3-D path, cx_morph_eval) -------------------------------------
// (keys: the priority = edge id of every surviving vertex travels with it; told: where a surviving triangle came from)
// Flags are bytes; a workgroup covers CXP_SCAN_BLOCK consecutive elements: first pass counts its flags (cxp_k_me_count), one
// workgroup turns the block counts into offsets (cxp_k_scan_sums2), the consumer kernels redo the scan INSIDE their block while they
// write.  (Until round 3: a full exclusive scan per array -- three kernels that read and write 4 bytes per element twice.)
__device__ __forceinline__ uint32_t cxp_block_excl4(const uint32_t v[4], uint32_t* s, uint32_t& block_total) {
    // exclusive prefix of this thread's 4 consecutive elements within the workgroup of 256 threads (s: 256 words of LDS)
    const uint32_t t = v[0] + v[1] + v[2] + v[3];
    s[threadIdx.x] = t;
    __syncthreads();
    for (uint32_t o = 1; o < 256; o <<= 1) {
        const uint32_t x = (threadIdx.x >= o) ? s[threadIdx.x - o] : 0u;
        __syncthreads();
        s[threadIdx.x] += x;
        __syncthreads();
    }
    block_total = s[255];
    return s[threadIdx.x] - t;
}
__global__ __launch_bounds__(256) void cxp_k_me_count(const uint8_t* flags, uint32_t n, uint32_t* count) {
    __shared__ uint32_t s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * CXP_SCAN_BLOCK + threadIdx.x * 4u;
    uint32_t c = 0;
    if (base + 3u < n) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(flags + base);   // 4 flags (0 / 1 each); base is a multiple of 4
        c = __popc(w & 0x01010101u);
    } else {
        for (uint32_t k = 0; k < 4 && base + k < n; k++) c += flags[base + k] ? 1u : 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o);
    if ((threadIdx.x & 63u) == 0 && c) atomicAdd(&s_n, c);
    __syncthreads();
    if (threadIdx.x == 0) count[blockIdx.x] = s_n;
}
__global__ void cxp_k_mark_used8(const int32_t* tri, const uint8_t* alive, uint32_t nt, uint8_t* used) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt || !alive[t]) return;
    const uint32_t a = (uint32_t)tri[(size_t)t * 3], b = (uint32_t)tri[(size_t)t * 3 + 1], c = (uint32_t)tri[(size_t)t * 3 + 2];   // all loads before the first store
    used[a] = 1; used[b] = 1; used[c] = 1;
}
// vertices in use -> their new ids (vnew, for the triangles) and their data in the compacted arrays
__global__ __launch_bounds__(256) void cxp_k_compact_pts_fused(const double* pts, const uint8_t* used, const uint32_t* voff, uint32_t nv, uint32_t* vnew,
                                                               double* out, const uint32_t* keys, uint32_t* keys_out, const uint8_t* ever, uint8_t* ever_out) {
    __shared__ uint32_t s[256];
    const uint32_t base = blockIdx.x * CXP_SCAN_BLOCK + threadIdx.x * 4u;
    uint32_t f[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) f[k] = (base + k < nv && used[base + k]) ? 1u : 0u;
    uint32_t tot;
    uint32_t id = voff[blockIdx.x] + cxp_block_excl4(f, s, tot);
    if (tot == 0u) return;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        if (!f[k]) continue;
        const uint32_t v = base + k;
        const double x = pts[(size_t)v * 3], y = pts[(size_t)v * 3 + 1], z = pts[(size_t)v * 3 + 2];
        const uint32_t key = keys_out ? keys[v] : 0u;
        const uint8_t e = ever_out ? ever[v] : (uint8_t)0;
        vnew[v] = id;
        out[(size_t)id * 3] = x; out[(size_t)id * 3 + 1] = y; out[(size_t)id * 3 + 2] = z;
        if (keys_out) keys_out[id] = key;
        if (ever_out) ever_out[id] = e;
        id++;
    }
}
__global__ __launch_bounds__(256) void cxp_k_compact_tri_fused(const int32_t* tri, const uint8_t* alive, const uint32_t* toff, const uint32_t* vnew, uint32_t nt,
                                                               int32_t* out, uint32_t* told) {
    __shared__ uint32_t s[256];
    const uint32_t base = blockIdx.x * CXP_SCAN_BLOCK + threadIdx.x * 4u;
    uint32_t f[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) f[k] = (base + k < nt && alive[base + k]) ? 1u : 0u;
    uint32_t tot;
    uint32_t id = toff[blockIdx.x] + cxp_block_excl4(f, s, tot);
    if (tot == 0u) return;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        if (!f[k]) continue;
        const uint32_t t = base + k;
        const uint32_t a = (uint32_t)tri[(size_t)t * 3], b = (uint32_t)tri[(size_t)t * 3 + 1], c = (uint32_t)tri[(size_t)t * 3 + 2];
        const uint32_t na = vnew[a], nb = vnew[b], nc = vnew[c];      // three look-ups in flight, then the stores
        out[(size_t)id * 3] = (int32_t)na; out[(size_t)id * 3 + 1] = (int32_t)nb; out[(size_t)id * 3 + 2] = (int32_t)nc;
        if (told) told[id] = t;
        id++;
    }
}

// ---- orientation ---------------------------------------------------------------------------------------
// edge table: key = (min vertex << 32) | max vertex, value = first triangle that inserted the edge.
// Every later triangle on that edge is linked to the first with the parity of their relative winding
// (surface_geometry.py:110-138: neighbours must run along the shared edge in opposite directions).
__device__ __forceinline__ uint32_t cxp_edge_dir(const int32_t* tri, uint32_t t, uint32_t lo, uint32_t hi) {
    // 1 if triangle t runs lo -> hi along its boundary cycle, 0 if hi -> lo
    const uint32_t a = tri[(size_t)t * 3], b = tri[(size_t)t * 3 + 1], c = tri[(size_t)t * 3 + 2];
    return ((a == lo && b == hi) || (b == lo && c == hi) || (c == lo && a == hi)) ? 1u : 0u;
}
__global__ void cxp_k_edges_claim(const int32_t* tri, uint32_t nt, u64* tab, u64 mask, u64 mult) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const uint32_t v[3] = {(uint32_t)tri[(size_t)t * 3], (uint32_t)tri[(size_t)t * 3 + 1], (uint32_t)tri[(size_t)t * 3 + 2]};
    for (int e = 0; e < 3; e++) {
        const uint32_t p = v[e], q = v[(e + 1) % 3];
        const uint32_t lo = min(p, q), hi = max(p, q);
        const u64 key = ((u64)lo << 32) | (u64)hi;
        u64 slot = cxp_edge_slot(lo, hi, mask, mult);
        for (;;) {
            // plain read first: the second visitor of an edge usually finds the key already there and needs no
            // read-modify-write (a stale EMPTY only costs the CAS it would have done anyway)
            u64 cur = __hip_atomic_load(&tab[2 * slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == CXD_EMPTY) cur = atomicCAS(&tab[2 * slot], CXD_EMPTY, key);
            if (cur == CXD_EMPTY) { __hip_atomic_store(&tab[2 * slot + 1], (u64)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
            if (cur == key) break;
            slot = (slot + 1) & mask;
        }
    }
}
// coherent == 0 (windings given by the caller, cx_surface_geometry): every visitor of an edge is united with the
// claimant with the parity of their relative winding, as the reference propagates it (surface_geometry.py:110-138).
// coherent != 0 (meshes of the march, which winds every triangle from low to high): two triangles that run along a
// shared edge in the same direction only occur where the weld has pinched sheets together along an edge shared by 3+
// triangles -- exactly the links that contradict each other (such an edge cannot have all of its triangles pairwise
// opposite).  United with their parities in one racing kernel, a contradictory union won somewhere and flipped a
// whole subtree: up to 4 % of the area of a 512^3 spherical shell came out wound the wrong way, differently from run
// to run.  So on these meshes a link only connects and never flips (parity 0; the neighbour's winding is not even
// read): both sides keep the march's winding -- a patch that hangs on a pinched edge still joins the component, as in
// the reference's traversal -- and the component is then turned as a whole by the max-x rule.
__global__ void cxp_k_edges_link(const int32_t* tri, uint32_t nt, const u64* tab, u64 mask, u64 mult, u64* parent, int coherent) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const uint32_t v[3] = {(uint32_t)tri[(size_t)t * 3], (uint32_t)tri[(size_t)t * 3 + 1], (uint32_t)tri[(size_t)t * 3 + 2]};
#pragma unroll
    for (int e = 0; e < 3; e++) {
        const uint32_t p = v[e], q = v[(e + 1) % 3];
        const uint32_t lo = min(p, q), hi = max(p, q);
        const u64 key = ((u64)lo << 32) | (u64)hi;
        u64 slot = cxp_edge_slot(lo, hi, mask, mult);
        while (tab[2 * slot] != key) slot = (slot + 1) & mask;   // every key was inserted by the claim kernel
        const uint32_t o = (uint32_t)tab[2 * slot + 1];
        if (o == t) continue;
        uint32_t rel = 0;
        if (!coherent) rel = (cxp_edge_dir(tri, t, lo, hi) == cxp_edge_dir(tri, o, lo, hi)) ? 1u : 0u;   // same direction = parity 1
        cxp_union(parent, nullptr, t, o, rel);
    }
}
// The same linking for the meshes of the march (coherent != 0: connectivity only) in two steps.  Triangle ids follow the march, so
// most edges join two triangles a few hundred ids apart: a workgroup takes CXP_LINK_BLOCK consecutive triangles, unites those
// whose partner lies in the same block in LDS (ds atomics instead of ~4 device-scope atomics per union, which are executed at
// the memory side of the fabric and bound the one-step kernel), writes the block's forest into the global parent words with
// plain stores -- nobody else touches them in this kernel -- and leaves the partners outside the block in `others` for the
// second kernel, which unites them with the global routine as before.  The roots are the smallest ids either way.
#ifndef CXP_LINK_BLOCK
#define CXP_LINK_BLOCK 2048u
#endif
#define CXP_LINK_PER_THREAD (CXP_LINK_BLOCK / 256u)
__device__ __forceinline__ uint32_t cxp_lfind(uint32_t* lp, uint32_t x) {
    for (;;) {
        const uint32_t p = ((volatile uint32_t*)lp)[x];
        if (p == x) return x;
        const uint32_t g = ((volatile uint32_t*)lp)[p];
        if (g != p) ((volatile uint32_t*)lp)[x] = g;   // path halving: only ever replaces a parent by an ancestor
        x = p;
    }
}
__global__ __launch_bounds__(256) void cxp_k_edges_link_local(const int32_t* tri, uint32_t nt, const u64* tab, u64 mask, u64 mult, u64* parent,
                                                              uint32_t* others) {
    __shared__ uint32_t lp[CXP_LINK_BLOCK];
    const uint32_t b0 = blockIdx.x * CXP_LINK_BLOCK;
    for (uint32_t x = threadIdx.x; x < CXP_LINK_BLOCK; x += 256u) lp[x] = x;
    __syncthreads();
#pragma unroll 1
    for (uint32_t i = 0; i < CXP_LINK_PER_THREAD; i++) {
        const uint32_t t = b0 + i * 256u + threadIdx.x;
        if (t >= nt) continue;
        const uint32_t v[3] = {(uint32_t)tri[(size_t)t * 3], (uint32_t)tri[(size_t)t * 3 + 1], (uint32_t)tri[(size_t)t * 3 + 2]};
#pragma unroll
        for (int e = 0; e < 3; e++) {
            const uint32_t p = v[e], q = v[(e + 1) % 3];
            const uint32_t lo = min(p, q), hi = max(p, q);
            const u64 key = ((u64)lo << 32) | (u64)hi;
            u64 slot = cxp_edge_slot(lo, hi, mask, mult);
            while (tab[2 * slot] != key) slot = (slot + 1) & mask;   // every key was inserted by the claim kernel
            const uint32_t o = (uint32_t)tab[2 * slot + 1];
            uint32_t far = CXD_NONE;
            if (o != t) {
                if (o - b0 < CXP_LINK_BLOCK) {          // partner in this block (o >= b0 by unsigned wrap-around)
                    uint32_t a = t - b0, b = o - b0;
                    for (;;) {
                        a = cxp_lfind(lp, a);
                        b = cxp_lfind(lp, b);
                        if (a == b) break;
                        const uint32_t win = min(a, b), lose = max(a, b);
                        if (atomicCAS(&lp[lose], lose, win) == lose) break;
                    }
                } else {
                    far = o;
                }
            }
            others[(size_t)t * 3 + e] = far;
        }
    }
    __syncthreads();
    for (uint32_t i = 0; i < CXP_LINK_PER_THREAD; i++) {
        const uint32_t x = i * 256u + threadIdx.x;
        if (b0 + x >= nt) continue;
        const uint32_t r = cxp_lfind(lp, x);
        if (r != x) parent[b0 + x] = (u64)(b0 + r);      // parity 0
    }
}
__global__ void cxp_k_edges_link_cross(uint32_t nt, const uint32_t* others, u64* parent) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
#pragma unroll
    for (int e = 0; e < 3; e++) {
        const uint32_t o = others[(size_t)t * 3 + e];
        if (o != CXD_NONE) cxp_union0(parent, t, o);
    }
}
// ---- the same linking for the MARCH'S OWN meshes, most of it in LDS ------------------------------------------------------
// An edge of the march's mesh lies on at most two triangles (a face of a tetrahedron has two sides), unless weld or clean-up
// merged something into one of its end points (`ever`).  Triangle ids follow the march: 86 % of the edges of the bench mesh join two
// triangles within the same 256 ids, 92 % within 1024 (tools/edge_locality.py).  A workgroup takes CXP_EB consecutive triangles and
// matches their edges in an LDS hash table; visitors of one edge are united in the block's LDS forest.  An edge found twice whose
// end points were never merged into is DONE and never sees the global table.  Only the rest goes through the device-scope table,
// one visit per block (the slot's taker): edges with one triangle in the block (the partner is in another block, or there is none)
// and edges with a flagged end point (their visitors in other blocks do the same, so three or more triangles on one edge still
// meet at the claimant, as in cxp_k_edges_link).  The table's compare-and-swaps (executed at the memory side) and the random
// 16-byte reads of the link step shrink to a sixth.  others[t] (one byte per triangle): bit e set = look edge e up in the second
// kernel, clear = settled here.
#ifndef CXP_EB
#define CXP_EB 512u
#endif
#define CXP_EB_PER (CXP_EB / 256u)      // triangles per thread
#define CXP_EB_SLOTS (4u * CXP_EB)       // > 3 * CXP_EB: an insert always finds a free slot
// (probe_limit / overflow: the global table is first sized for what usually reaches it -- a sixth of the edges -- and a probe
// sequence that long says it was too small for this mesh: the host repeats the stage with the table of the worst case)
__global__ __launch_bounds__(256) void cxp_k_edges_block(const int32_t* tri, uint32_t nt, const uint8_t* ever, u64* tab, u64 mask, u64 mult,
                                                         u64* parent, uint8_t* others, uint32_t probe_limit, uint32_t* overflow) {
    __shared__ u64 lkey[CXP_EB_SLOTS];
    __shared__ uint16_t lfirst[CXP_EB_SLOTS];
    __shared__ uint8_t lpair[CXP_EB_SLOTS];
    __shared__ uint32_t lp[CXP_EB];
    const uint32_t b0 = blockIdx.x * CXP_EB;
    for (uint32_t x = threadIdx.x; x < CXP_EB_SLOTS; x += 256u) { lkey[x] = CXD_EMPTY; lpair[x] = 0; }
    for (uint32_t x = threadIdx.x; x < CXP_EB; x += 256u) lp[x] = x;
    uint32_t lo_[CXP_EB_PER][3], hi_[CXP_EB_PER][3];
    uint32_t flag_[CXP_EB_PER][3];
    uint16_t slot_[CXP_EB_PER][3];
    // the triangles and the flags of their end points: all requested before anything is used
#pragma unroll
    for (uint32_t i = 0; i < CXP_EB_PER; i++) {
        const uint32_t t = min(b0 + i * 256u + threadIdx.x, nt - 1u);
        const uint32_t v[3] = {(uint32_t)tri[(size_t)t * 3], (uint32_t)tri[(size_t)t * 3 + 1], (uint32_t)tri[(size_t)t * 3 + 2]};
#pragma unroll
        for (int e = 0; e < 3; e++) {
            lo_[i][e] = min(v[e], v[(e + 1) % 3]);
            hi_[i][e] = max(v[e], v[(e + 1) % 3]);
        }
    }
#pragma unroll
    for (uint32_t i = 0; i < CXP_EB_PER; i++)
#pragma unroll
        for (int e = 0; e < 3; e++) flag_[i][e] = (uint32_t)ever[lo_[i][e]] | (uint32_t)ever[hi_[i][e]];
    __syncthreads();
    // pass 1: every edge visit finds or takes its slot; the taker leaves its triangle there
#pragma unroll
    for (uint32_t i = 0; i < CXP_EB_PER; i++) {
        const uint32_t lt = i * 256u + threadIdx.x;
        if (b0 + lt >= nt) continue;
#pragma unroll
        for (int e = 0; e < 3; e++) {
            const u64 key = ((u64)lo_[i][e] << 32) | (u64)hi_[i][e];
            uint32_t slot = (uint32_t)cxd_mix(key) & (CXP_EB_SLOTS - 1u);
            for (uint32_t probes = 0; probes < CXP_EB_SLOTS; probes++) {      // (always ends earlier: the table cannot fill up)
                const u64 cur = atomicCAS((unsigned long long*)&lkey[slot], (unsigned long long)CXD_EMPTY, (unsigned long long)key);
                if (cur == CXD_EMPTY) { lfirst[slot] = (uint16_t)lt; break; }
                if (cur == key) break;
                slot = (slot + 1u) & (CXP_EB_SLOTS - 1u);
            }
            slot_[i][e] = (uint16_t)slot;
        }
    }
    __syncthreads();
    // pass 2: the other visitors of a slot unite with the taker in the block's forest
#pragma unroll
    for (uint32_t i = 0; i < CXP_EB_PER; i++) {
        const uint32_t lt = i * 256u + threadIdx.x;
        if (b0 + lt >= nt) continue;
#pragma unroll
        for (int e = 0; e < 3; e++) {
            const uint32_t first = lfirst[slot_[i][e]];
            if (first == lt) continue;
            lpair[slot_[i][e]] = 1;
            uint32_t a = lt, b = first;
            for (;;) {
                a = cxp_lfind(lp, a);
                b = cxp_lfind(lp, b);
                if (a == b) break;
                const uint32_t win = min(a, b), lose = max(a, b);
                if (atomicCAS(&lp[lose], lose, win) == lose) break;
            }
        }
    }
    __syncthreads();
    // pass 3: what the block could not settle claims its place in the global table: an edge with one visitor here, and -- through
    // its taker alone, the block's other visitors are united with it already -- an edge with a flagged end point (its visitors in
    // OTHER blocks do the same and meet at the claimant)
#pragma unroll
    for (uint32_t i = 0; i < CXP_EB_PER; i++) {
        const uint32_t lt = i * 256u + threadIdx.x, t = b0 + lt;
        if (t >= nt) continue;
        uint32_t farbits = 0;      // bit e: edge e of this triangle went to the global table (one BYTE per triangle: the second kernel reads
                                   // nothing else of it -- as three 32-bit words this was 270 MB written and read back at 22.5 M triangles)
#pragma unroll
        for (int e = 0; e < 3; e++) {
            const uint32_t lo = lo_[i][e], hi = hi_[i][e];
            const bool taker = lfirst[slot_[i][e]] == lt;
            if (taker && (flag_[i][e] != 0u || !lpair[slot_[i][e]])) {
                farbits |= 1u << e;
                const u64 key = ((u64)lo << 32) | (u64)hi;
                u64 slot = cxp_edge_slot(lo, hi, mask, mult);
                for (uint32_t probes = 0;; probes++) {
                    if (probes >= probe_limit) { *overflow = 1u; break; }
                    u64 cur = __hip_atomic_load(&tab[2 * slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (cur == CXD_EMPTY) cur = atomicCAS(&tab[2 * slot], CXD_EMPTY, key);
                    if (cur == CXD_EMPTY) { __hip_atomic_store(&tab[2 * slot + 1], (u64)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
                    if (cur == key) break;
                    slot = (slot + 1) & mask;
                }
            }
        }
        others[t] = (uint8_t)farbits;
    }
    // the block's forest into the global parent words (nobody else touches them in this kernel); roots = smallest ids
    for (uint32_t x = threadIdx.x; x < CXP_EB; x += 256u) {
        if (b0 + x >= nt) continue;
        const uint32_t r = cxp_lfind(lp, x);
        if (r != x) parent[b0 + x] = (u64)(b0 + r);      // parity 0
    }
}
// second kernel: the visitors the first one sent to the global table unite with the edge's claimant
__global__ void cxp_k_edges_link_far(const int32_t* tri, uint32_t nt, const u64* tab, u64 mask, u64 mult, const uint8_t* others, u64* parent) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const uint32_t fb = others[t];
    if (!fb) return;
    const uint32_t v[3] = {(uint32_t)tri[(size_t)t * 3], (uint32_t)tri[(size_t)t * 3 + 1], (uint32_t)tri[(size_t)t * 3 + 2]};
#pragma unroll
    for (int e = 0; e < 3; e++) {
        if (!((fb >> e) & 1u)) continue;
        const uint32_t p = v[e], q = v[(e + 1) % 3];
        const uint32_t lo = min(p, q), hi = max(p, q);
        const u64 key = ((u64)lo << 32) | (u64)hi;
        u64 slot = cxp_edge_slot(lo, hi, mask, mult);
        while (tab[2 * slot] != key) slot = (slot + 1) & mask;   // every such key was inserted by the first kernel
        const uint32_t o = (uint32_t)tab[2 * slot + 1];
        if (o != t) cxp_union0(parent, t, o);
    }
}
// per component (root triangle): largest x over its vertices.  cls (sharded Level 1 only): per triangle, > 2 = a copy of a
// neighbour slab's triangle, which takes part in the components but not in the choice of the start triangle.
#define CXP_OWN(cls, t) (!(cls) || (cls)[t] <= 2u)
// Triangles are visited from the LAST to the first: the march numbers them by ascending x, so the first waves to run establish
// the maximum and everybody after them sees in a plain read that it has nothing to add (visited in ascending order every wave
// raises the maximum, and same-address atomics serialise).
__global__ void cxp_k_comp_maxx(const int32_t* tri, uint32_t nt, const double* pts, const u64* parent, u64* cmaxx, const uint8_t* cls) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t t = nt - 1u - idx;
    const bool have = idx < nt && CXP_OWN(cls, t);
    uint32_t root = 0;
    u64 m = 0;
    if (have) {
        root = (uint32_t)parent[t];
#pragma unroll
        for (int s = 0; s < 3; s++) m = max(m, cxd_orderable(pts[(size_t)tri[(size_t)t * 3 + s] * 3]));
    }
    cxp_wave_max64(cmaxx, root, m, have);
}
// The triangles that can hold the start triangle of their component: those with a vertex AT the component's largest x.  A handful
// per component (a face of the volume that the surface runs along: thousands) -- the four kernels below visit this list instead of
// every triangle.  One atomic per wave.
__global__ void cxp_k_comp_list(const int32_t* tri, uint32_t nt, const double* pts, const u64* parent, const u64* cmaxx, const uint8_t* cls,
                                uint32_t* list, uint32_t* nlist) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    bool hit = false;
    if (t < nt && CXP_OWN(cls, t)) {
        const u64 m = cmaxx[(uint32_t)parent[t]];
#pragma unroll
        for (int s = 0; s < 3; s++) hit = hit || cxd_orderable(pts[(size_t)tri[(size_t)t * 3 + s] * 3]) == m;
    }
    const uint64_t hits = __ballot(hit);
    if (hits == 0ULL) return;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t base = 0;
    if (lane == (uint32_t)(__ffsll((long long)hits) - 1)) base = atomicAdd(nlist, (uint32_t)__popcll(hits));
    base = (uint32_t)__shfl((int)base, __ffsll((long long)hits) - 1);
    if (hit) list[base + (uint32_t)__popcll(hits & ((1ULL << lane) - 1ULL))] = t;
}
// visit either every triangle (list == nullptr: one per thread) or the triangles of a list (grid-stride)
#define CXP_FOR_TRI(t)                                                                                                   \
    for (uint32_t i_ = blockIdx.x * blockDim.x + threadIdx.x, n_ = list ? *nlist : nt; i_ < n_; i_ += gridDim.x * blockDim.x) { \
        const uint32_t t = list ? list[i_] : i_;
#define CXP_END_FOR }
// among the vertices at that x: the one with the largest index in the reference (surface_geometry.py:79 max((x, index)), its
// numbering being its hash order); here the one with the largest EDGE ID, which does not depend on how the mesh is numbered or
// cut into slabs.  Packed (edge id << 32 | vertex).
__global__ void cxp_k_comp_maxv(const int32_t* tri, uint32_t nt, const double* pts, const u64* parent, const u64* cmaxx, u64* cmaxv,
                                const uint32_t* keys, const uint8_t* cls, const uint32_t* list, const uint32_t* nlist) {
    CXP_FOR_TRI(t)
        if (!CXP_OWN(cls, t)) continue;
        const uint32_t root = (uint32_t)parent[t];
        const u64 m = cmaxx[root];
#pragma unroll
        for (int s = 0; s < 3; s++) {
            const uint32_t v = tri[(size_t)t * 3 + s];
            if (cxd_orderable(pts[(size_t)v * 3]) == m) cxd_max64(&cmaxv[root], ((u64)(keys ? keys[v] : v) << 32) | (u64)v);
        }
    CXP_END_FOR
}
// among that vertex's triangles: the largest |cross(a-b, a-c)[0]| (surface_geometry.py:88-94); the packed
// word keeps the triangle id so that the next kernel can read its sign
__device__ __forceinline__ double cxp_dotx(const int32_t* tri, uint32_t t, const double* pts) {
    const uint32_t a = tri[(size_t)t * 3], b = tri[(size_t)t * 3 + 1], c = tri[(size_t)t * 3 + 2];
    const double aby = pts[(size_t)a * 3 + 1] - pts[(size_t)b * 3 + 1], abz = pts[(size_t)a * 3 + 2] - pts[(size_t)b * 3 + 2];
    const double acy = pts[(size_t)a * 3 + 1] - pts[(size_t)c * 3 + 1], acz = pts[(size_t)a * 3 + 2] - pts[(size_t)c * 3 + 2];
    return aby * acz - abz * acy;
}
__global__ void cxp_k_comp_start(const int32_t* tri, uint32_t nt, const double* pts, const u64* parent, const u64* cmaxv,
                                 u64* cbest, const uint8_t* cls, const uint32_t* list, const uint32_t* nlist) {
    CXP_FOR_TRI(t)
        if (!CXP_OWN(cls, t)) continue;
        const uint32_t root = (uint32_t)parent[t];
        const uint32_t vm = (uint32_t)cmaxv[root];
        if ((uint32_t)tri[(size_t)t * 3] != vm && (uint32_t)tri[(size_t)t * 3 + 1] != vm && (uint32_t)tri[(size_t)t * 3 + 2] != vm) continue;
        cxd_max64(&cbest[root], cxd_orderable(fabs(cxp_dotx(tri, t, pts))));
    CXP_END_FOR
}
__global__ void cxp_k_comp_pick(const int32_t* tri, uint32_t nt, const double* pts, const u64* parent, const u64* cmaxv,
                                const u64* cbest, uint32_t* cstart, const uint8_t* cls, const uint32_t* list, const uint32_t* nlist) {
    CXP_FOR_TRI(t)
        if (!CXP_OWN(cls, t)) continue;
        const uint32_t root = (uint32_t)parent[t];
        const uint32_t vm = (uint32_t)cmaxv[root];
        if ((uint32_t)tri[(size_t)t * 3] != vm && (uint32_t)tri[(size_t)t * 3 + 1] != vm && (uint32_t)tri[(size_t)t * 3 + 2] != vm) continue;
        if (cxd_orderable(fabs(cxp_dotx(tri, t, pts))) == cbest[root]) cxd_max32(&cstart[root], t);
    CXP_END_FOR
}
// the root's flip, so that the start triangle gets dotx > 0 (surface_geometry.py:99-103).  Decided in its own kernel,
// BEFORE any triangle is rewritten: cxp_k_orient reverses triangles in place, and reading the start triangle there
// raced with the thread that reverses it (a component came out partly wound one way and partly the other, rarely)
__global__ void cxp_k_comp_decide(const int32_t* tri, uint32_t nt, const double* pts, const u64* parent, const uint32_t* cstart, u64* cflip,
                                  const uint32_t* list, const uint32_t* nlist) {
    CXP_FOR_TRI(t)
        const u64 w = parent[t];
        const uint32_t root = (uint32_t)w;
        if (cstart[root] != t) continue;
        const uint32_t spar = (uint32_t)(w >> 32) & 1u;
        cflip[root] = (u64)((((cxp_dotx(tri, t, pts) < 0.0) ? 1u : 0u) ^ spar) & 1u);   // in the root's frame
    CXP_END_FOR
}
// final winding: triangle parity relative to the root, and the root's flip
__global__ void cxp_k_orient(int32_t* tri, uint32_t nt, const u64* parent, const u64* cflip, uint32_t* ncomp) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const u64 w = parent[t];
    const uint32_t root = (uint32_t)w, par = (uint32_t)(w >> 32) & 1u;
    if (root == t) atomicAdd(ncomp, 1u);
    if ((par ^ (uint32_t)cflip[root]) & 1u) {
        // reversed(orientation): (a,b,c) -> (c,b,a)
        const int32_t a = tri[(size_t)t * 3];
        tri[(size_t)t * 3] = tri[(size_t)t * 3 + 2];
        tri[(size_t)t * 3 + 2] = a;
    }
}

// ---- sharded Level 1: a slab marched together with two layers of its neighbours' cells ------------------
// Every triangle of the march lies in one cell; the smallest of its three edge ids belongs to an edge that starts in the
// cell's lower x face (a tetrahedron has no three crossing edges inside one face of the cube), so (id >> 3) / plane is the
// cell's layer.  Classes: 0 own, 1 / 2 own and next to the lower / upper neighbour, 3 / 4 first layer of the lower / upper
// neighbour (kept for the components), 255 second layer (only there so that weld, tiny collapse and clean-up of the first
// layer see everything they see in the undivided volume): dropped here.
struct cxp_shard {
    uint32_t plane;            // samples per x plane
    uint32_t own_lo, own_hi;   // own cell layers [own_lo, own_hi) of the local array
    uint32_t layers;           // cell layers of the local array
};
__global__ void cxp_k_shard_classify(const uint32_t* tprio3, uint8_t* alive, uint32_t nt, cxp_shard sh, cx_fdiv dplane, uint8_t* cls,
                                     uint32_t* counts) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    uint8_t c = 255;
    if (alive[t]) {
        const uint32_t layer = cx_div(tprio3[(size_t)t * 3] >> 3, dplane);
        if (layer >= sh.own_lo && layer < sh.own_hi) {
            c = 0;
            if (layer == sh.own_lo && sh.own_lo > 0u) c = 1;
            else if (layer + 1u == sh.own_hi && sh.own_hi < sh.layers) c = 2;
        } else if (layer + 1u == sh.own_lo) c = 3;
        else if (layer == sh.own_hi) c = 4;
        if (c == 255) alive[t] = 0;
        else if (c == 1) atomicAdd(&counts[0], 1u);
        else if (c == 4) atomicAdd(&counts[1], 1u);
    }
    cls[t] = c;
}
__global__ void cxp_k_shard_gather_cls(const uint8_t* cls, const uint32_t* told, uint32_t nt2, uint8_t* cls2) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < nt2) cls2[t] = cls[told[t]];
}
// What a rank and its LOWER neighbour must agree on: the neighbour holds copies of this rank's first layer of own triangles
// (its class 4), this rank holds the originals (class 1).  Both write (hash of the three ORIGINAL edge ids in the numbering of
// the whole volume, component label); sorted by the hash the two lists line up entry by entry, and the label pairs say which
// components are one.  (The copies on the other side -- classes 2 / 3 -- would say the same again: a link between two
// slabs' triangles is seen from both.)  Components with such a triangle are marked open.
__device__ __forceinline__ u64 cxp_triple_hash(u64 a, u64 b, u64 c) {
    u64 h = cxd_mix(a + 0x9E3779B97F4A7C15ULL);
    h = cxd_mix(h ^ (b + 0xC2B2AE3D27D4EB4FULL));
    return cxd_mix(h ^ (c + 0x165667B19E3779F9ULL));
}
__global__ void cxp_k_shard_boundary(const uint8_t* cls2, const uint32_t* told, const uint32_t* tprio3, const u64* parent, uint32_t nt2,
                                     u64 key_offset, uint32_t* counters, uint32_t cap1, uint32_t cap4, u64* hash1, uint32_t* label1,
                                     u64* hash4, uint32_t* label4, uint8_t* open) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt2) return;
    const uint32_t c = cls2[t];
    if (c != 1u && c != 4u) return;
    const uint32_t root = (uint32_t)parent[t];
    open[root] = 1;
    const uint32_t o = told[t];
    const u64 h = cxp_triple_hash((u64)tprio3[(size_t)o * 3] + key_offset, (u64)tprio3[(size_t)o * 3 + 1] + key_offset,
                                  (u64)tprio3[(size_t)o * 3 + 2] + key_offset);
    if (c == 1u) {
        const uint32_t at = atomicAdd(&counters[0], 1u);
        if (at < cap1) { hash1[at] = h; label1[at] = root; }
    } else {
        const uint32_t at = atomicAdd(&counters[1], 1u);
        if (at < cap4) { hash4[at] = h; label4[at] = root; }
    }
}
// the start-triangle candidate of every open component, from this slab's own triangles: (label, x of the max-x vertex, its
// edge id, |normal_x| of the start triangle, its sign, whether there is a candidate at all)
struct cxp_cand { double x, nx; uint32_t label, vkey, sign, has; };
__global__ void cxp_k_shard_candidates(const int32_t* tri2, const double* pts2, const uint32_t* keys2, const u64* parent, const uint8_t* open,
                                       uint32_t nt2, const u64* cmaxx, const u64* cmaxv, const uint32_t* cstart, uint32_t* counter,
                                       uint32_t cap, cxp_cand* out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt2 || (uint32_t)parent[t] != t || !open[t]) return;
    const uint32_t at = atomicAdd(counter, 1u);
    if (at >= cap) return;
    cxp_cand c;
    c.label = t; c.has = cmaxx[t] != 0 ? 1u : 0u; c.x = 0.0; c.nx = 0.0; c.vkey = 0; c.sign = 0;
    if (c.has) {
        const uint32_t vm = (uint32_t)cmaxv[t];
        const double d = cxp_dotx(tri2, cstart[t], pts2);
        c.x = pts2[(size_t)vm * 3]; c.vkey = keys2[vm]; c.nx = fabs(d); c.sign = d < 0.0 ? 1u : 0u;
    }
    out[at] = c;
}
__global__ void cxp_k_shard_set_flips(const uint32_t* labels, const uint8_t* flips, uint32_t n, uint32_t nt2, u64* cflip) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && labels[i] < nt2) cflip[labels[i]] = (u64)(flips[i] & 1u);
}
__global__ void cxp_k_shard_own_alive(const uint8_t* cls2, uint32_t nt2, uint8_t* alive) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < nt2) alive[t] = cls2[t] <= 2u ? 1 : 0;
}


// ---- host orchestration ----------------------------------------------------------------------------------
// the small kernels above for the other post-pass files (cx_post.h): a kernel is launched from the file that defines it
void cxp_iota64(hipStream_t st, u64* a, uint32_t n) {
    hipLaunchKernelGGL(cxp_k_iota64, dim3(cx_blocks(n)), dim3(256), 0, st, a, n);
}
void cxp_fill64(hipStream_t st, u64* a, size_t n, u64 v) {
    hipLaunchKernelGGL(cxp_k_fill64, dim3(2048), dim3(256), 0, st, a, n, v);
}
void cxp_count_alive(hipStream_t st, const uint8_t* alive, uint32_t nt, uint32_t* counter) {
    hipLaunchKernelGGL(cxp_k_count_alive, dim3(std::min(cx_blocks(nt), 1024u)), dim3(256), 0, st, alive, nt, counter);
}
void cxp_alive_u32(hipStream_t st, const uint8_t* alive, uint32_t nt, uint32_t* out) {
    hipLaunchKernelGGL(cxp_k_alive_u32, dim3(cx_blocks(nt)), dim3(256), 0, st, alive, nt, out);
}
void cxp_scan_sums(hipStream_t st, uint32_t* sums, uint32_t nb, uint32_t* total) {
    hipLaunchKernelGGL(cxp_k_scan_sums, dim3(1), dim3(1024), 0, st, sums, nb, total, (unsigned long long*)nullptr);
}

int cxp_scan(cx_ctx* ctx, cx_post_state* S, const uint32_t* in, uint32_t* out, uint32_t n, uint32_t* total_dev) {
    const uint32_t nb = cx_blocks(n, CXP_SCAN_BLOCK);
    int rc = S->blocksums.grow(ctx, (size_t)(nb + 1) * sizeof(uint32_t));
    if (rc) return rc;
    uint32_t* sums = S->blocksums.as<uint32_t>();
    hipLaunchKernelGGL(cxp_k_scan_blocks, dim3(nb ? nb : 1), dim3(256), 0, ctx->stream, in, out, sums, n);
    hipLaunchKernelGGL(cxp_k_scan_sums, dim3(1), dim3(1024), 0, ctx->stream, sums, nb, total_dev, (unsigned long long*)nullptr);
    hipLaunchKernelGGL(cxp_k_scan_add, dim3(cx_blocks(n)), dim3(256), 0, ctx->stream, out, sums, n);
    return CX_OK;
}

// exclusive scan for the other translation units (cx_contour2d.hip); sums_tmp holds n/1024 + 2 words
int cx_scan_u32(cx_ctx* ctx, const uint32_t* in, uint32_t* out, uint32_t n, uint32_t* sums_tmp, uint32_t* total_dev, unsigned long long* total64_dev) {
    const uint32_t nb = cx_blocks(n, CXP_SCAN_BLOCK);
    hipLaunchKernelGGL(cxp_k_scan_blocks, dim3(nb ? nb : 1), dim3(256), 0, ctx->stream, in, out, sums_tmp, n);
    hipLaunchKernelGGL(cxp_k_scan_sums, dim3(1), dim3(1024), 0, ctx->stream, sums_tmp, nb, total_dev, total64_dev);
    if (n) hipLaunchKernelGGL(cxp_k_scan_add, dim3(cx_blocks(n)), dim3(256), 0, ctx->stream, out, sums_tmp, n);
    return CX_OK;
}

static int cxp_flatten(cx_ctx* ctx, u64* parent, uint32_t n, uint32_t* changed_dev) {
    for (int it = 0; it < 64; it++) {
        CX_HIP(ctx, hipMemsetAsync(changed_dev, 0, sizeof(uint32_t), ctx->stream));
        hipLaunchKernelGGL(cxp_k_jump, dim3(cx_blocks(n)), dim3(256), 0, ctx->stream, parent, n, changed_dev);
        uint32_t changed = 0;
        CX_HIP(ctx, hipMemcpyAsync(&changed, changed_dev, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        CX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (!changed) return CX_OK;
    }
    ctx->err = "union-find did not flatten";
    return CX_ERR_HIP;
}

// The component orientation after the linking, in two halves (cx_post.h): the 3-D tail below and cx_morph_triangles (cx_morph.hip)
// run the same launches in the same order; the sharded Level 1 works between the halves.
int cxp_orient_pick(cx_ctx* ctx, const int32_t* tri, uint32_t nt, const double* pts, u64* parent, u64* comp, const uint32_t* keys,
                    const uint8_t* cls, uint32_t* clist, uint32_t* misc) {
    int rc;
    hipStream_t st = ctx->stream;
    const cxp_comp_tables C = cxp_comp_view(comp, nt);
    if ((rc = cxp_flatten(ctx, parent, nt, misc + CXP_M_CHANGED))) return rc;
    CX_HIP(ctx, hipMemsetAsync(comp, 0, cxp_comp_bytes(nt), st));
    CX_HIP(ctx, hipMemsetAsync(misc + CXP_M_NCOMP, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(cxp_k_comp_maxx, dim3(cx_blocks(nt)), dim3(256), 0, st, tri, nt, pts, parent, C.cmaxx, cls);
    // the four kernels that pick a component's start triangle visit the list of triangles AT the component's largest x (cxp_k_comp_list)
    const uint32_t* cn = misc + CXP_M_CLIST;
    const dim3 lgrid(std::min(cx_blocks(nt), 1024u));
    CX_HIP(ctx, hipMemsetAsync(misc + CXP_M_CLIST, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(cxp_k_comp_list, dim3(cx_blocks(nt)), dim3(256), 0, st, tri, nt, pts, parent, C.cmaxx, cls, clist, misc + CXP_M_CLIST);
    hipLaunchKernelGGL(cxp_k_comp_maxv, lgrid, dim3(256), 0, st, tri, nt, pts, parent, C.cmaxx, C.cmaxv, keys, cls, (const uint32_t*)clist, cn);
    hipLaunchKernelGGL(cxp_k_comp_start, lgrid, dim3(256), 0, st, tri, nt, pts, parent, C.cmaxv, C.cflip, cls, (const uint32_t*)clist, cn);
    hipLaunchKernelGGL(cxp_k_comp_pick, lgrid, dim3(256), 0, st, tri, nt, pts, parent, C.cmaxv, C.cflip, C.cstart, cls, (const uint32_t*)clist, cn);
    return CX_OK;
}
int cxp_orient_decide(cx_ctx* ctx, int32_t* tri, uint32_t nt, const double* pts, const u64* parent, u64* comp, const uint32_t* clist,
                      uint32_t* misc, bool wind, uint32_t* ncomp) {
    hipStream_t st = ctx->stream;
    const cxp_comp_tables C = cxp_comp_view(comp, nt);
    const uint32_t* cn = misc + CXP_M_CLIST;
    const dim3 lgrid(std::min(cx_blocks(nt), 1024u));
    hipLaunchKernelGGL(cxp_k_comp_decide, lgrid, dim3(256), 0, st, tri, nt, pts, parent, (const uint32_t*)C.cstart, C.cflip, clist, cn);
    if (wind) {
        hipLaunchKernelGGL(cxp_k_orient, dim3(cx_blocks(nt)), dim3(256), 0, st, tri, nt, parent, C.cflip, misc + CXP_M_NCOMP);
        CX_HIP(ctx, hipMemcpyAsync(ncomp, misc + CXP_M_NCOMP, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    return CX_OK;
}

// ---- the record of what the buffers hold (cx_post.h) ----------------------------------------------------------------------------------
void cxp_begin(cx_ctx* ctx, cx_post_state* S) {
    const uint64_t gen = S->rec.gen + 1;
    S->rec = cxp_record();
    S->rec.gen = gen;
    ctx->post_valid = false;
    if (ctx->s4) ctx->s4->post_valid = false;
}
int cxp_publish(cx_ctx* ctx, cx_post_state* S, cxp_record::holds_t holds, cxp_record::origin_t origin, const int64_t* counts, int64_t* out_counts) {
    S->rec.holds = holds;
    S->rec.origin = origin;
    if (holds == cxp_record::MESH3D) ctx->post_valid = true;
    if (holds == cxp_record::TETS4D) ctx->s4->post_valid = true;
    if (out_counts) memcpy(out_counts, counts, 8 * sizeof(int64_t));
    return CX_OK;
}
bool cxp_mesh3d(const cx_ctx* ctx) { return ctx->post && ctx->post_valid && ctx->post->rec.holds == cxp_record::MESH3D; }
bool cxp_tets4d(const cx_ctx* ctx) { return ctx->post && ctx->s4 && ctx->s4->post_valid && ctx->post->rec.holds == cxp_record::TETS4D; }

// the five buffers of the raw input mesh for nv vertices and nt triangles (S->raw).  weld: the whole post-pass follows (cxp_run3d): also
// the weld's representatives (rep) and the tiny collapse's union-find (parent), each at the place in the order it was always grown at
static int cxp_reserve_raw(cx_ctx* ctx, cx_post_state* S, size_t nv, size_t nt, bool weld = false) {
    int rc;
    if ((rc = S->pts.grow(ctx, (nv + 1) * 3 * sizeof(double)))) return rc;
    if ((rc = S->prio.grow(ctx, (nv + 1) * sizeof(uint32_t)))) return rc;
    if (weld && (rc = S->rep.grow(ctx, (nv + 1) * (sizeof(uint32_t) + 1)))) return rc;
    if ((rc = S->tri.grow(ctx, (nt + 1) * 3 * sizeof(int32_t) * 2))) return rc;   // triangles + priority triples
    if ((rc = S->alive.grow(ctx, nt + 16))) return rc;
    if (weld && (rc = S->parent.grow(ctx, (nv + 1) * sizeof(u64)))) return rc;
    if ((rc = S->parent2.grow(ctx, (nv + 1) * sizeof(u64)))) return rc;
    S->raw = {S->pts.as<double>(), S->prio.as<uint32_t>(), S->tri.as<int32_t>(), S->tri.as<uint32_t>() + (nt + 1) * 3, S->alive.as<uint8_t>(),
              S->parent2.as<u64>()};
    return CX_OK;
}

// triangles that became the same vertex set: the one with the smallest sorted priority triple survives (tsz slots of S->tkeys)
static void cxp_dedupe(cx_ctx* ctx, cx_post_state* S, const int32_t* tri, const uint32_t* tprio3, uint8_t* alive, uint32_t nt, u64 tsz, const uint8_t* involved) {
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(cxp_k_fill64, dim3(2048), dim3(256), 0, st, S->tkeys.as<u64>(), (size_t)tsz, CXD_EMPTY);
    hipLaunchKernelGGL(cxp_k_dedupe_insert, dim3(cx_blocks(nt)), dim3(256), 0, st, tri, tprio3, alive, nt, S->tkeys.as<u64>(), tsz - 1, involved);
    hipLaunchKernelGGL(cxp_k_dedupe_resolve, dim3(cx_blocks(nt)), dim3(256), 0, st, tri, alive, nt, S->tkeys.as<u64>(), tsz - 1, involved);
}

// Ordered compaction of the used vertices and living triangles of (pts, keys, tri, alive) into the buffers P / T / K, grown to the
// totals (byte flags in S->flags, per-block counts, the scan redone inside the two consumers; vnew in S->scan).  The totals come back
// in ONE copy of nwords words from CXP_M_TOTAL0 on: h[0] vertices, h[1] triangles, and h[2] = CXP_M_NCOMP for the caller that asks.
static int cxp_compact(cx_ctx* ctx, cx_post_state* S, const double* pts, const uint32_t* keys, const int32_t* tri, const uint8_t* alive, uint32_t nv,
                       uint32_t nt, cx_buf<uint8_t>& P, cx_buf<uint8_t>& T, cx_buf<uint8_t>& K, uint8_t* ever, uint32_t* told, int nwords,
                       uint32_t* h) {
    int rc;
    hipStream_t st = ctx->stream;
    uint32_t* misc = S->misc.as<uint32_t>();
    const uint32_t nbv = cx_blocks(nv, CXP_SCAN_BLOCK), nbt = cx_blocks(nt, CXP_SCAN_BLOCK);
    if ((rc = S->blocksums.grow(ctx, (size_t)(nbv + nbt + 16) * sizeof(uint32_t)))) return rc;
    uint8_t* used = S->flags.as<uint8_t>();
    uint32_t* vnew = S->scan.as<uint32_t>();
    uint32_t* voff = S->blocksums.as<uint32_t>();
    uint32_t* toff = voff + nbv + 8;
    for (int k = 0; k < nwords; k++) h[k] = 0;
    if (nt) {
        CX_HIP(ctx, hipMemsetAsync(used, 0, (size_t)nv, st));
        hipLaunchKernelGGL(cxp_k_mark_used8, dim3(cx_blocks(nt)), dim3(256), 0, st, tri, alive, nt, used);
        hipLaunchKernelGGL(cxp_k_me_count, dim3(nbv), dim3(256), 0, st, (const uint8_t*)used, nv, voff);
        hipLaunchKernelGGL(cxp_k_me_count, dim3(nbt), dim3(256), 0, st, alive, nt, toff);
        hipLaunchKernelGGL(cxp_k_scan_sums2, dim3(2), dim3(1024), 0, st, voff, nbv, misc + CXP_M_TOTAL0, toff, nbt, misc + CXP_M_TOTAL1);
        CX_HIP(ctx, hipMemcpyAsync(h, misc + CXP_M_TOTAL0, nwords * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        CX_HIP(ctx, hipStreamSynchronize(st));
    }
    if ((rc = P.grow(ctx, (size_t)(h[0] + 1) * 3 * sizeof(double)))) return rc;
    if ((rc = T.grow(ctx, (size_t)(h[1] + 1) * 3 * sizeof(int32_t)))) return rc;
    if ((rc = K.grow(ctx, (size_t)(h[0] + 1) * sizeof(uint32_t)))) return rc;
    if (h[1]) {
        hipLaunchKernelGGL(cxp_k_compact_pts_fused, dim3(nbv), dim3(256), 0, st, pts, (const uint8_t*)used, (const uint32_t*)voff, nv, vnew, P.as<double>(), keys,
                           K.as<uint32_t>(), (const uint8_t*)ever, ever ? ever + nv : nullptr);
        hipLaunchKernelGGL(cxp_k_compact_tri_fused, dim3(nbt), dim3(256), 0, st, tri, alive, (const uint32_t*)toff, (const uint32_t*)vnew, nt, T.as<int32_t>(), told);
    }
    return CX_OK;
}

// the boundary block of an open shard in S->bnd: hash1 u64[n1] | hash4 u64[n4] | candidates cxp_cand[n1 + n4] | label1 u32[n1] | label4 u32[n4]
struct cxp_bnd {
    u64 *hash1, *hash4;
    cxp_cand* cand;
    uint32_t *label1, *label4;
};
static size_t cxp_bnd_bytes(size_t n1, size_t n4) { return (n1 + n4 + 2) * (sizeof(u64) + sizeof(cxp_cand) + sizeof(uint32_t)) + 64; }
static cxp_bnd cxp_bnd_view(cx_post_state* S, size_t n1, size_t n4) {
    u64* hash1 = S->bnd.as<u64>();
    cxp_cand* cand = (cxp_cand*)(hash1 + n1 + n4);
    uint32_t* label1 = (uint32_t*)(cand + n1 + n4);
    return {hash1, hash1 + n1, cand, label1, label1 + n1};
}

// Shared tail: clean (optional) + compaction + orientation (optional) on the raw mesh S->raw (nv x 3 doubles, nt x 3 indices, alive
// bytes; prio = vertex priorities).  Results in S->pts_out / S->tri_out / S->keys_out, S->nv_out / S->nt_out.  The caller has called
// cxp_begin and publishes what comes out.
static int cxp_clean_orient(cx_ctx* ctx, cx_post_state* S, uint32_t nv, uint32_t nt, bool do_clean, bool do_orient, int64_t* out_counts, bool coherent,
                            uint8_t* involved = nullptr, const cxp_shard* shard = nullptr,
                            uint8_t* ever = nullptr) {   // ever != nullptr: the march's own mesh (cxp_k_edges_block); u8[nv] flags, room for nv more behind them
    int rc;
    double* pts = S->raw.pts;
    uint32_t* prio = S->raw.prio;
    int32_t* tri = S->raw.tri;
    uint32_t* tprio3 = S->raw.tprio3;
    uint8_t* alive = S->raw.alive;
    uint32_t* misc = S->misc.as<uint32_t>();
    hipStream_t st = ctx->stream;
    if (do_clean && nt) {
        u64* parent2 = S->raw.parent2;
        hipLaunchKernelGGL(cxp_k_iota64, dim3(cx_blocks(nv)), dim3(256), 0, st, parent2, nv);
        hipLaunchKernelGGL(cxp_k_degenerate, dim3(cx_blocks(nt)), dim3(256), 0, st, tri, alive, nt, pts, parent2, prio);
        if (involved) CX_HIP(ctx, hipMemsetAsync(involved, 0, nv, st));
        hipLaunchKernelGGL(cxp_k_remap, dim3(cx_blocks(nt)), dim3(256), 0, st, tri, alive, nt, (const uint32_t*)nullptr, parent2, involved, ever);
        // (with the filter only triangles next to a merge enter the table: 5/4 of the bound is plenty and half as much to clear)
        const u64 tsz = involved ? cxp_edge_table_size(nt) : cx_table_size(nt);
        if ((rc = S->tkeys.grow(ctx, tsz * sizeof(u64)))) return rc;
        cxp_dedupe(ctx, S, tri, tprio3, alive, nt, tsz, involved);
    }
    // ---- sharded: the second layer of the neighbours' cells has done its work (weld, tiny collapse and clean-up above saw it)
    uint8_t* cls = nullptr;
    uint32_t* told = nullptr;
    if (shard) {
        if ((rc = S->cls.grow(ctx, 3 * (size_t)nt + 64))) return rc;
        if ((rc = S->told.grow(ctx, ((size_t)nt + 16) * sizeof(uint32_t)))) return rc;
        cls = S->cls.as<uint8_t>();
        told = S->told.as<uint32_t>();
        CX_HIP(ctx, hipMemsetAsync(misc + CXP_M_SHARD_N, 0, 2 * sizeof(uint32_t), st));
        if (nt) hipLaunchKernelGGL(cxp_k_shard_classify, dim3(cx_blocks(nt)), dim3(256), 0, st, tprio3, alive, nt, *shard, cx_fdiv_make(shard->plane), cls, misc + CXP_M_SHARD_N);
    }
    // ---- compaction of used vertices and living triangles
    if ((rc = S->flags.grow(ctx, (size_t)(nv + nt + 16) * sizeof(uint32_t)))) return rc;      // (also: the list of possible start triangles below)
    if ((rc = S->scan.grow(ctx, (size_t)(nv + 16) * sizeof(uint32_t)))) return rc;
    uint32_t h[2];
    if ((rc = cxp_compact(ctx, S, pts, prio, tri, alive, nv, nt, S->pts_out, S->tri_out, S->keys_out, ever, told, 2, h))) return rc;
    const uint32_t nv2 = h[0], nt2 = h[1];
    double* pts2 = S->pts_out.as<double>();
    int32_t* tri2 = S->tri_out.as<int32_t>();
    uint32_t* keys2 = S->keys_out.as<uint32_t>();
    S->nv_out = nv2; S->nt_out = nt2;
    uint8_t* cls2 = nullptr;
    if (shard) {
        cls2 = cls + nt;
        if (nt2) hipLaunchKernelGGL(cxp_k_shard_gather_cls, dim3(cx_blocks(nt2)), dim3(256), 0, st, cls, told, nt2, cls2);
    }
    uint32_t ncomp = 0;
    if (do_orient && nt2) {
        // ---- orientation: edge table + parity union-find over triangles
        // (measured and dropped: clearing the table on a second stream while weld / tiny collapse / clean-up run -- no gain, the fill
        // takes from them what it saves)
        const u64 esz_full = cxp_edge_table_size((size_t)nt2 * 3);
        const bool blocks = ever && coherent && !cx_debug_knob("CX_LINK_GLOBAL", 0);
        // the march's own mesh: most edges are settled inside a block of triangles and never reach the table (cxp_k_edges_block): a
        // sixth of them for the bench mesh.  First attempt: one slot per TRIANGLE (a quarter of the worst case: 0.5 instead of 2 GB to
        // clear and to probe); a mesh that needs more says so and the stage is repeated with the full table.
        u64 esz = esz_full;
        if (blocks && !cx_debug_knob("CX_EDGE_TABLE_FULL", 0)) {
            esz = 1024;
            while (esz < (u64)nt2 + 16) esz <<= 1;
            if (cx_debug_knob("CX_EDGE_TABLE_TINY", 0)) esz = 1024;     // tests: force the repeat
            if (esz > esz_full) esz = esz_full;
        }
        if ((rc = S->parent.grow(ctx, (size_t)nt2 * sizeof(u64)))) return rc;
        if ((rc = S->comp.grow(ctx, cxp_comp_bytes(nt2)))) return rc;
        u64* parent = S->parent.as<u64>();
        const cxp_comp_tables C = cxp_comp_view(S->comp.as<u64>(), nt2);
        uint32_t* others = S->comp.as<uint32_t>();   // 12 of the 28 bytes per triangle that the component tables take below
        for (;;) {
            if ((rc = S->tkeys.grow(ctx, 2 * esz * sizeof(u64)))) return rc;
            u64* etab = S->tkeys.as<u64>();
            // (measured and dropped: clearing the table on a second stream while weld / tiny collapse / clean-up run -- no gain, the fill
            // takes from them what it saves)
            hipLaunchKernelGGL(cxp_k_fill64, dim3(2048), dim3(256), 0, st, etab, (size_t)(2 * esz), CXD_EMPTY);
            hipLaunchKernelGGL(cxp_k_iota64, dim3(cx_blocks(nt2)), dim3(256), 0, st, parent, nt2);
            const u64 emult = (blocks && esz != esz_full) ? 0 : std::max<u64>(1, esz / std::max<u64>(1, (u64)nv2));
            if (blocks) {
                CX_HIP(ctx, hipMemsetAsync(misc + CXP_M_OVER, 0, sizeof(uint32_t), st));
                hipLaunchKernelGGL(cxp_k_edges_block, dim3((nt2 + CXP_EB - 1u) / CXP_EB), dim3(256), 0, st, tri2, nt2, (const uint8_t*)(ever + nv), etab, esz - 1,
                                   emult, parent, (uint8_t*)others, esz == esz_full ? 0xFFFFFFFFu : 256u, misc + CXP_M_OVER);
                if (esz != esz_full) {
                    uint32_t over = 0;
                    CX_HIP(ctx, hipMemcpyAsync(&over, misc + CXP_M_OVER, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
                    CX_HIP(ctx, hipStreamSynchronize(st));
                    if (over) { esz = esz_full; continue; }
                }
                hipLaunchKernelGGL(cxp_k_edges_link_far, dim3(cx_blocks(nt2)), dim3(256), 0, st, tri2, nt2, etab, esz - 1, emult, (const uint8_t*)others, parent);
            } else {
                hipLaunchKernelGGL(cxp_k_edges_claim, dim3(cx_blocks(nt2)), dim3(256), 0, st, tri2, nt2, etab, esz - 1, emult);
                if (coherent && !cx_debug_knob("CX_LINK_ONE_STEP", 0)) {
                    hipLaunchKernelGGL(cxp_k_edges_link_local, dim3((nt2 + CXP_LINK_BLOCK - 1u) / CXP_LINK_BLOCK), dim3(256), 0, st, tri2, nt2, etab, esz - 1,
                                       emult, parent, others);
                    hipLaunchKernelGGL(cxp_k_edges_link_cross, dim3(cx_blocks(nt2)), dim3(256), 0, st, nt2, others, parent);
                } else
                    hipLaunchKernelGGL(cxp_k_edges_link, dim3(cx_blocks(nt2)), dim3(256), 0, st, tri2, nt2, etab, esz - 1, emult, parent, coherent ? 1 : 0);
            }
            break;
        }
        // (the scan / flag arrays of the compaction are free by now: the list of possible start triangles goes there)
        uint32_t* clist = S->flags.as<uint32_t>();
        if ((rc = cxp_orient_pick(ctx, tri2, nt2, pts2, parent, C.cmaxx, keys2, cls2, clist, misc))) return rc;
        if (shard) {
            // what the neighbours need: the triangles at the slab boundaries with their labels (they stay on the device), and the
            // start-triangle candidate of every component that reaches a neighbour.  Sizes follow the slab boundary, not the slab.
            uint32_t hb[2] = {0, 0};
            CX_HIP(ctx, hipMemcpyAsync(hb, misc + CXP_M_SHARD_N, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            CX_HIP(ctx, hipStreamSynchronize(st));
            const size_t n1 = hb[0], n4 = hb[1], nb = n1 + n4;
            if ((rc = S->bnd.grow(ctx, cxp_bnd_bytes(n1, n4)))) return rc;
            const cxp_bnd B = cxp_bnd_view(S, n1, n4);
            uint8_t* open = cls + 2 * (size_t)nt;
            CX_HIP(ctx, hipMemsetAsync(open, 0, nt2, st));
            CX_HIP(ctx, hipMemsetAsync(misc + CXP_M_BND_N, 0, 3 * sizeof(uint32_t), st));
            if (nb) {
                const u64 key_offset = ((u64)ctx->origin[0] * (u64)shard->plane) << 3;
                hipLaunchKernelGGL(cxp_k_shard_boundary, dim3(cx_blocks(nt2)), dim3(256), 0, st, cls2, told, tprio3, parent, nt2, key_offset, misc + CXP_M_BND_N,
                                   (uint32_t)n1, (uint32_t)n4, B.hash1, B.label1, B.hash4, B.label4, open);
                hipLaunchKernelGGL(cxp_k_shard_candidates, dim3(cx_blocks(nt2)), dim3(256), 0, st, tri2, pts2, keys2, parent, open, nt2, C.cmaxx, C.cmaxv,
                                   C.cstart, misc + CXP_M_BND_NCAND, (uint32_t)nb, B.cand);
            }
            uint32_t h2[3] = {0, 0, 0};
            CX_HIP(ctx, hipMemcpyAsync(h2, misc + CXP_M_BND_N, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            CX_HIP(ctx, hipStreamSynchronize(st));
            if (h2[0] != n1 || h2[1] != n4 || h2[2] > nb) { ctx->err = "sharded Level 1: boundary lists do not add up"; return CX_ERR_HIP; }
            S->shard.n1 = (uint32_t)n1; S->shard.n4 = (uint32_t)n4; S->shard.ncand = h2[2];
        }
        if ((rc = cxp_orient_decide(ctx, tri2, nt2, pts2, parent, C.cmaxx, clist, misc, !shard, &ncomp))) return rc;
        if (!shard) { S->rec.tables_live = true; S->rec.tables_nt = nt2; }
        CX_HIP(ctx, hipStreamSynchronize(st));
    } else if (shard) {
        S->shard.n1 = 0; S->shard.n4 = 0; S->shard.ncand = 0;
    }
    if (shard) { S->shard.nv2 = nv2; S->shard.nt2 = nt2; S->shard.nt_in = nt; }
    CX_HIP(ctx, hipGetLastError());
    if (out_counts) {
        out_counts[0] = nv2; out_counts[1] = nt2; out_counts[4] = ncomp;
    }
    return CX_OK;
}

// sharded Level 1, last step: the flips the ranks agreed on for the components that reach a neighbour replace the local
// decisions, every triangle is wound, and the copies of the neighbours' triangles leave the mesh
static int cxp_shard_finish(cx_ctx* ctx, cx_post_state* S, const uint32_t* labels, const uint8_t* flips, uint32_t n, int64_t* out_counts) {
    int rc;
    hipStream_t st = ctx->stream;
    uint32_t* misc = S->misc.as<uint32_t>();
    const uint32_t nv2 = S->shard.nv2, nt2 = S->shard.nt2;
    cxp_begin(ctx, S);      // (the open shard is over, however this ends)
    uint32_t h[3] = {0, 0, 0};       // vertices, triangles, components
    if (nt2) {
        u64* parent = S->parent.as<u64>();
        u64* cflip = cxp_comp_view(S->comp.as<u64>(), nt2).cflip;
        int32_t* tri2 = S->tri_out.as<int32_t>();
        const uint8_t* cls2 = S->cls.as<const uint8_t>() + S->shard.nt_in;
        if (n) {
            if ((rc = S->keys_tmp.grow(ctx, std::max((size_t)n * 5 + 64, (size_t)(nv2 + 1) * sizeof(uint32_t))))) return rc;
            uint32_t* dl = S->keys_tmp.as<uint32_t>();
            uint8_t* df = (uint8_t*)(dl + n);
            CX_HIP(ctx, hipMemcpyAsync(dl, labels, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            CX_HIP(ctx, hipMemcpyAsync(df, flips, (size_t)n, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(cxp_k_shard_set_flips, dim3(cx_blocks(n)), dim3(256), 0, st, dl, df, n, nt2, cflip);
        }
        CX_HIP(ctx, hipMemsetAsync(misc + CXP_M_NCOMP, 0, sizeof(uint32_t), st));
        hipLaunchKernelGGL(cxp_k_orient, dim3(cx_blocks(nt2)), dim3(256), 0, st, tri2, nt2, parent, cflip, misc + CXP_M_NCOMP);
        // own triangles and the vertices they use.  The march's own buffers are free by now: they take the final mesh on its way back
        // into the output buffers
        uint8_t* alive = S->alive.as<uint8_t>();
        hipLaunchKernelGGL(cxp_k_shard_own_alive, dim3(cx_blocks(nt2)), dim3(256), 0, st, cls2, nt2, alive);
        if ((rc = cxp_compact(ctx, S, S->pts_out.as<const double>(), S->keys_out.as<const uint32_t>(), tri2, alive, nv2, nt2, S->pts, S->tri, S->keys_tmp,
                              nullptr, nullptr, 3, h))) return rc;
        // back into the output buffers (every buffer keeps its size from call to call: nothing is reallocated for the next volume)
        if (h[1]) {
            CX_HIP(ctx, hipMemcpyAsync(S->pts_out.get(), S->pts.get(), (size_t)h[0] * 3 * sizeof(double), hipMemcpyDeviceToDevice, st));
            CX_HIP(ctx, hipMemcpyAsync(S->tri_out.get(), S->tri.get(), (size_t)h[1] * 3 * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
            CX_HIP(ctx, hipMemcpyAsync(S->keys_out.get(), S->keys_tmp.get(), (size_t)h[0] * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        }
        CX_HIP(ctx, hipStreamSynchronize(st));
    }
    S->nv_out = h[0]; S->nt_out = h[1];
    CX_HIP(ctx, hipGetLastError());
    const int64_t counts[8] = {h[0], h[1], 0, 0, h[2], 0, 0, 0};
    return cxp_publish(ctx, S, cxp_record::MESH3D, cxp_record::SHARD, counts, out_counts);
}

int cxp_state(cx_ctx* ctx, cx_post_state** out) {
    if (!ctx->post) ctx->post = new (std::nothrow) cx_post_state();
    if (!ctx->post) return CX_ERR_NOMEM;
    *out = ctx->post;
    // every post-pass rewrites the points the morph triangles of an earlier cx_morph_triangles index: those are gone (their segments would
    // point into the new points: cx_morph_eval on them read out of bounds)
    ctx->post->ms_out = 0; ctx->post->mt_out = 0; ctx->post->msorted = false; ctx->post->me_off.clear();
    return ctx->post->misc.grow(ctx, CXP_M_WORDS * sizeof(uint32_t));
}

// ---- smooth_interpolations(factor) (tetrahedral.py:329-351): every vertex that is part of a triangle moves by
// `factor` towards the mean of the vertices of its triangles (itself included, each neighbour once)
__global__ void cxp_k_unique_edges(const int32_t* tri, const uint8_t* alive, uint32_t nt, u64* ekeys, u64 mask) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt || !alive[t]) return;
    const uint32_t v[3] = {(uint32_t)tri[(size_t)t * 3], (uint32_t)tri[(size_t)t * 3 + 1], (uint32_t)tri[(size_t)t * 3 + 2]};
    for (int e = 0; e < 3; e++) {
        const uint32_t p = v[e], q = v[(e + 1) % 3];
        const u64 key = ((u64)min(p, q) << 32) | (u64)max(p, q);
        u64 slot = cxd_mix(key) & mask;
        for (;;) {
            u64 cur = __hip_atomic_load(&ekeys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the second visitor of an edge needs no read-modify-write
            if (cur == CXD_EMPTY) cur = atomicCAS(&ekeys[slot], CXD_EMPTY, key);
            if (cur == CXD_EMPTY || cur == key) break;
            slot = (slot + 1) & mask;
        }
    }
}
__global__ void cxp_k_smooth_accumulate(const u64* ekeys, size_t n, const double* pts, double* sum, uint32_t* cnt) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n || ekeys[i] == CXD_EMPTY) return;
    const uint32_t a = (uint32_t)(ekeys[i] >> 32), b = (uint32_t)ekeys[i];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        atomicAdd(&sum[(size_t)a * 3 + c], pts[(size_t)b * 3 + c]);
        atomicAdd(&sum[(size_t)b * 3 + c], pts[(size_t)a * 3 + c]);
    }
    atomicAdd(&cnt[a], 1u);
    atomicAdd(&cnt[b], 1u);
}
// The two kernels above in one, with the sums put together per workgroup first (default; the two-kernel form stays for comparison
// behind CX_SMOOTH_TWO_STEP): the thread whose compare-and-swap claimed an edge's slot accumulates that edge, right there -- in triangle
// order, where the triangles of a workgroup share their vertices --, into an LDS table keyed by vertex, and the workgroup adds every
// vertex of its table to the global sums ONCE.  (One device-scope add per edge, coordinate and direction -- eight per edge, 270 M on the
// 512^3 bench mesh -- took 12.1 of the 14.4 ms smoothing added to Level 1.)
#define CXP_SM_SLOTS 1024u
__global__ __launch_bounds__(256) void cxp_k_smooth_edges(const int32_t* tri, const uint8_t* alive, uint32_t nt, u64* ekeys, u64 mask, const double* pts,
                                                          double* sum, uint32_t* cnt) {
    __shared__ uint32_t lv[CXP_SM_SLOTS];
    __shared__ uint32_t lc[CXP_SM_SLOTS];
    __shared__ double ls[CXP_SM_SLOTS][3];
    for (uint32_t x = threadIdx.x; x < CXP_SM_SLOTS; x += 256u) { lv[x] = CXD_NONE; lc[x] = 0u; ls[x][0] = 0.0; ls[x][1] = 0.0; ls[x][2] = 0.0; }
    __syncthreads();
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < nt && alive[t]) {
        const uint32_t v[3] = {(uint32_t)tri[(size_t)t * 3], (uint32_t)tri[(size_t)t * 3 + 1], (uint32_t)tri[(size_t)t * 3 + 2]};
        auto add = [&](uint32_t to, uint32_t from) {      // the point `from` into the sums of vertex `to`
            uint32_t slot = (to * 0x9E3779B1u) >> 22;      // 10 bits
            for (;;) {
                const uint32_t cur = atomicCAS(&lv[slot], CXD_NONE, to);
                if (cur == CXD_NONE || cur == to) break;
                slot = (slot + 1u) & (CXP_SM_SLOTS - 1u);  // (at most 768 vertices per workgroup: a free slot is always found)
            }
            unsafeAtomicAdd(&ls[slot][0], pts[(size_t)from * 3]);
            unsafeAtomicAdd(&ls[slot][1], pts[(size_t)from * 3 + 1]);
            unsafeAtomicAdd(&ls[slot][2], pts[(size_t)from * 3 + 2]);
            atomicAdd(&lc[slot], 1u);
        };
        for (int e = 0; e < 3; e++) {
            const uint32_t p = v[e], q = v[(e + 1) % 3];
            const u64 key = ((u64)min(p, q) << 32) | (u64)max(p, q);
            u64 slot = cxd_mix(key) & mask;
            bool mine = false;
            for (;;) {
                u64 cur = __hip_atomic_load(&ekeys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the second visitor of an edge needs no read-modify-write
                if (cur == CXD_EMPTY) { cur = atomicCAS(&ekeys[slot], CXD_EMPTY, key); mine = cur == CXD_EMPTY; }
                if (cur == CXD_EMPTY || cur == key) break;
                slot = (slot + 1) & mask;
            }
            if (mine && p != q) { add(p, q); add(q, p); }
            else if (mine) { add(p, p); add(p, p); }        // (a degenerate edge: what the two-kernel form does with it)
        }
    }
    __syncthreads();
    for (uint32_t x = threadIdx.x; x < CXP_SM_SLOTS; x += 256u) {
        const uint32_t to = lv[x];
        if (to == CXD_NONE) continue;
        atomicAdd(&sum[(size_t)to * 3], ls[x][0]);
        atomicAdd(&sum[(size_t)to * 3 + 1], ls[x][1]);
        atomicAdd(&sum[(size_t)to * 3 + 2], ls[x][2]);
        atomicAdd(&cnt[to], lc[x]);
    }
}
__global__ void cxp_k_smooth_apply(double* pts, const double* sum, const uint32_t* cnt, uint32_t nv, double factor) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv || cnt[v] == 0u) return;
    const double inv = 1.0 / (double)(cnt[v] + 1u);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double p = pts[(size_t)v * 3 + c];
        const double avg = (sum[(size_t)v * 3 + c] + p) * inv;
        pts[(size_t)v * 3 + c] = p - factor * (p - avg);
    }
}

extern "C" int cx_postprocess3d_ex(cx_ctx* ctx, uint32_t flags, double smooth, int64_t* out_counts);

extern "C" int cx_postprocess3d(cx_ctx* ctx, uint32_t flags, int64_t* out_counts) {
    return cx_postprocess3d_ex(ctx, flags, 0.0, out_counts);
}

// The raw mesh from the current extraction: its vertices in float64 about the lattice origin org (priority = edge id), its triangles,
// and alive bytes for nt_alive triangles (a caller that appends triangles of its own asks for more than the extraction has).  The
// seeded selection's mask, where there is one, becomes the alive bytes and *vkeep the vertices' half of it.
static int cxp_raw_from_extraction(cx_ctx* ctx, cx_post_state* S, const cxp_origin3& org, uint32_t nt_alive, const uint8_t** vkeep) {
    const cx_params& P = ctx->last;
    const uint32_t nv = (uint32_t)ctx->counts.n_vertices, nt = (uint32_t)ctx->counts.n_triangles;
    hipStream_t st = ctx->stream;
    if (nv) cxp_launch_vertices_f64(dim3(cx_blocks(nv)), st, P.grid, ctx->grid64_valid ? ctx->grid64.get() : nullptr, P.n1, P.n2, P.div_plane, P.div_row, P.value,
                                    (const cx_vrec*)ctx->verts.get(), nv, S->raw.pts, S->raw.prio, org);
    if (nt) CX_HIP(ctx, hipMemcpyAsync(S->raw.tri, ctx->tris, (size_t)nt * 3 * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    if (ctx->keep_valid && vkeep) {   // cx_select_seeded3d: only the triangles (and vertices) of the selected components exist
        CX_HIP(ctx, hipMemcpyAsync(S->raw.alive, ctx->tri_keep, nt, hipMemcpyDeviceToDevice, st));
        *vkeep = ctx->tri_keep + nt;
    } else {
        CX_HIP(ctx, hipMemsetAsync(S->raw.alive, 1, nt_alive, st));
    }
    return CX_OK;
}
// the reference's `corner` (voxels per axis) of the resident array; an array with a margin around the reference's grid carries the
// reference's own corner in ctx->corner_ref (cx_set_reference_corner)
static void cxp_corner_of(const cx_ctx* ctx, double corner[3]) {
    const cx_params& P = ctx->last;
    const uint32_t n[3] = {P.n0, P.n1, P.n2};
    for (int a = 0; a < 3; a++) corner[a] = ctx->corner_ref[a] > 0 ? (double)ctx->corner_ref[a] : (double)(n[a] - 1);
}
// weld -> (smooth) -> tiny collapse -> clean -> orient on S->pts / S->prio / S->tri / S->alive (A6..A10)
// edge_crossings: the vertices are the march's own crossings with their edge ids as priorities (cx_postprocess3d*), not points
// handed over by a caller (cx_postprocess3d_mesh: refined points, slab meshes with global edge ids as ranks)
static int cxp_run3d(cx_ctx* ctx, cx_post_state* S, uint32_t nv, uint32_t nt, const double corner[3], const uint8_t* vkeep, bool do_clean,
                     double smooth, bool coherent, int64_t* counts, bool edge_crossings = false, const cxp_shard* shard = nullptr, bool march_mesh = false) {
    int rc;
    hipStream_t st = ctx->stream;
    double* pts = S->raw.pts;
    uint32_t* prio = S->raw.prio;
    uint32_t* rep = S->rep.as<uint32_t>();
    uint8_t* moved = (uint8_t*)(rep + nv + 1);
    int32_t* tri = S->raw.tri;
    uint32_t* tprio3 = S->raw.tprio3;
    uint8_t* alive = S->raw.alive;
    uint32_t* misc = S->misc.as<uint32_t>();
    uint8_t* ever = nullptr;      // the march's own crossings: which vertices weld or clean-up merge something into
    for (int a = 0; a < 3; a++) S->corner[a] = corner[a];
    // (march_mesh: a mesh the march emitted, handed back by the caller -- slabs assembled on the host, refined points --: an edge lies on
    // at most two triangles until something is merged into one of its ends, which is all the block linking needs; the weld shortcut needs
    // the crossings' own geometry and stays with edge_crossings)
    if (nv && nt && (edge_crossings || march_mesh) && coherent) {
        if ((rc = S->ever.grow(ctx, 2 * (size_t)nv + 64))) return rc;
        ever = S->ever.as<uint8_t>();
        CX_HIP(ctx, hipMemsetAsync(ever, 0, nv, st));
    }
    if (nv && nt) {
        hipLaunchKernelGGL(cxp_k_tri_prio, dim3(cx_blocks(nt)), dim3(256), 0, st, tri, prio, nt, tprio3);
        // ---- weld (tetrahedral.py:190-215): expander = int(10000 / corner)
        cxp_weld_params W;
        for (int a = 0; a < 3; a++) W.ex[a] = std::trunc((10000 * 1.0) / corner[a]);
        W.thr = 0.0;
        if (edge_crossings && !cx_debug_knob("CX_WELD_ALL", 0)) {
            const double exmin = std::min(W.ex[0], std::min(W.ex[1], W.ex[2]));
            if (exmin >= 16.0) W.thr = 2.0 / exmin + 1e-9;
        }
        // (W.thr > 0: four of five crossings are alone in their bucket and skip the table -- 5/4 of the bound instead of twice it)
        const u64 wsz = W.thr > 0.0 ? cxp_edge_table_size(nv) : cx_table_size(nv);
        if ((rc = S->tkeys.grow(ctx, std::max(wsz, cx_table_size(nt)) * sizeof(u64)))) return rc;
        if ((rc = S->tvals.grow(ctx, wsz * sizeof(u64)))) return rc;
        hipLaunchKernelGGL(cxp_k_fill64, dim3(2048), dim3(256), 0, st, S->tkeys.as<u64>(), (size_t)wsz, CXD_EMPTY);
        hipLaunchKernelGGL(cxp_k_fill64, dim3(2048), dim3(256), 0, st, S->tvals.as<u64>(), (size_t)wsz, (u64)0);
        hipLaunchKernelGGL(cxp_k_weld_insert, dim3(cx_blocks(nv)), dim3(256), 0, st, pts, prio, nv, W, S->tkeys.as<u64>(), S->tvals.as<u64>(), wsz - 1, vkeep);
        hipLaunchKernelGGL(cxp_k_weld_lookup, dim3(cx_blocks(nv)), dim3(256), 0, st, pts, nv, W, S->tkeys.as<u64>(), S->tvals.as<u64>(), wsz - 1, rep, vkeep, prio);
        // meshes of the march hold no triangle twice: only triangles with a vertex something was welded into can have a twin
        // (`moved` is free until the tiny collapse: it carries the flags)
        uint8_t* involved = (coherent && !cx_debug_knob("CX_DEDUPE_ALL", 0)) ? moved : nullptr;
        if (involved) CX_HIP(ctx, hipMemsetAsync(involved, 0, nv, st));
        hipLaunchKernelGGL(cxp_k_remap, dim3(cx_blocks(nt)), dim3(256), 0, st, tri, alive, nt, rep, (const u64*)nullptr, involved, ever);
        const u64 tsz = involved ? cxp_edge_table_size(nt) : cx_table_size(nt);
        cxp_dedupe(ctx, S, tri, tprio3, alive, nt, tsz, involved);
        CX_HIP(ctx, hipMemsetAsync(misc + CXP_M_WELD, 0, 2 * sizeof(uint32_t), st));
        hipLaunchKernelGGL(cxp_k_count_alive, dim3(std::min(cx_blocks(nt), 1024u)), dim3(256), 0, st, alive, nt, misc + CXP_M_WELD);
        if (smooth > 0.0) {
            // ---- smooth_interpolations (tetrahedral.py:547-550), between the weld and the tiny collapse
            const u64 esz = cx_table_size((size_t)nt * 3);
            if ((rc = S->tkeys.grow(ctx, esz * sizeof(u64)))) return rc;
            if ((rc = S->pts_out.grow(ctx, (size_t)(nv + 1) * 3 * sizeof(double)))) return rc;
            if ((rc = S->flags.grow(ctx, (size_t)(nv + nt + 16) * sizeof(uint32_t)))) return rc;
            double* sum = S->pts_out.as<double>();
            uint32_t* cnt = S->flags.as<uint32_t>();
            CX_HIP(ctx, hipMemsetAsync(sum, 0, (size_t)nv * 3 * sizeof(double), st));
            CX_HIP(ctx, hipMemsetAsync(cnt, 0, (size_t)nv * sizeof(uint32_t), st));
            hipLaunchKernelGGL(cxp_k_fill64, dim3(2048), dim3(256), 0, st, S->tkeys.as<u64>(), (size_t)esz, CXD_EMPTY);
            if (cx_debug_knob("CX_SMOOTH_TWO_STEP", 0)) {
                hipLaunchKernelGGL(cxp_k_unique_edges, dim3(cx_blocks(nt)), dim3(256), 0, st, tri, alive, nt, S->tkeys.as<u64>(), esz - 1);
                hipLaunchKernelGGL(cxp_k_smooth_accumulate, dim3(cx_blocks(esz)), dim3(256), 0, st, S->tkeys.as<const u64>(), (size_t)esz, pts, sum, cnt);
            } else {
                hipLaunchKernelGGL(cxp_k_smooth_edges, dim3(cx_blocks(nt)), dim3(256), 0, st, tri, alive, nt, S->tkeys.as<u64>(), esz - 1, (const double*)pts, sum, cnt);
            }
            hipLaunchKernelGGL(cxp_k_smooth_apply, dim3(cx_blocks(nv)), dim3(256), 0, st, pts, sum, cnt, nv, smooth);
        }
        // ---- tiny collapse (tetrahedral.py:353-375), epsilon = 1e-4, scaled by 1/corner
        u64* parent = S->parent.as<u64>();
        hipLaunchKernelGGL(cxp_k_iota64, dim3(cx_blocks(nv)), dim3(256), 0, st, parent, nv);
        CX_HIP(ctx, hipMemsetAsync(moved, 0, nv, st));
        hipLaunchKernelGGL(cxp_k_tiny, dim3(cx_blocks(nt)), dim3(256), 0, st, tri, alive, nt, pts, 1.0 / corner[0], 1.0 / corner[1],
                           1.0 / corner[2], 1e-4, parent, prio, moved);
        // roots keep their own coordinates, so moving members in place is race free
        hipLaunchKernelGGL(cxp_k_move, dim3(cx_blocks(nv)), dim3(256), 0, st, pts, pts, parent, moved, nv);
        hipLaunchKernelGGL(cxp_k_count_alive, dim3(std::min(cx_blocks(nt), 1024u)), dim3(256), 0, st, alive, nt, misc + CXP_M_TINY);
        uint32_t h[2];
        CX_HIP(ctx, hipMemcpyAsync(h, misc + CXP_M_WELD, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        CX_HIP(ctx, hipStreamSynchronize(st));
        counts[2] = h[0]; counts[3] = h[1];
    }
    // (`moved` is free again after cxp_k_move)
    return cxp_clean_orient(ctx, S, nv, nt, do_clean, true, counts, coherent,
                            (coherent && nv && nt && !cx_debug_knob("CX_DEDUPE_ALL", 0)) ? moved : nullptr, shard, ever);
}

extern "C" int cx_postprocess3d_ex(cx_ctx* ctx, uint32_t flags, double smooth, int64_t* out_counts) {
    if (!ctx) return CX_ERR_INVALID;
    if (!ctx->extracted) { ctx->err = "cx_postprocess3d: no valid extraction"; return CX_ERR_STATE; }
    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_post_state* S;
    int rc = cxp_state(ctx, &S);
    if (rc) return rc;
    const uint32_t nv = (uint32_t)ctx->counts.n_vertices, nt = (uint32_t)ctx->counts.n_triangles;
    int64_t counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    cxp_begin(ctx, S);
    if ((rc = cxp_reserve_raw(ctx, S, nv, nt, true))) return rc;
    const uint8_t* vkeep = nullptr;
    // an array with a rim of samples around the reference's grid starts at a NEGATIVE lattice point (cx_set_origin):
    // the post-pass then works in the reference's own lattice coordinates, so that the weld buckets truncate as the
    // reference's do (towards zero) and the Level-1 points come back in its coordinates.  Slabs (origin >= 0) stay local.
    cxp_origin3 org{{0.0, 0.0, 0.0}};
    if (ctx->origin[0] < 0 || ctx->origin[1] < 0 || ctx->origin[2] < 0)
        for (int a = 0; a < 3; a++) org.o[a] = (double)ctx->origin[a];
    if (nv && nt && (rc = cxp_raw_from_extraction(ctx, S, org, nt, &vkeep))) return rc;
    double corner[3];
    cxp_corner_of(ctx, corner);
    if ((rc = cxp_run3d(ctx, S, nv, nt, corner, vkeep, !(flags & 1u), smooth, true, counts, true))) return rc;   // the march winds every triangle low -> high
    return cxp_publish(ctx, S, cxp_record::MESH3D, cxp_record::GRID, counts, out_counts);
}

// ---- the capped mesh (cx_cap.hip, include/contourist_hip.h "rim caps"): the Level-0 mesh followed by the cap of cx_cap3d ---------------
// The input is filled as cx_postprocess3d_ex fills it, then the cap's vertices (the same float64 formula on their records {key, 0}: a
// lattice point, direction 0, interpolates between itself and itself) and triangles follow, and cxp_run3d runs on nv + cap, nt + cap.
// edge_crossings = true stands, for two reasons:
//   - cxp_weld_alone must treat a lattice-point vertex as NOT alone (a crossing within 1/ex of it shares its bucket).  It does: the
//     coordinate it looks at is an integer for a direction-0 key (every coordinate of a lattice point is), u = x - floor(x) = 0, and
//     u > thr fails for every thr > 0.  A crossing the cap made itself (the march had skipped it) is a crossing like the march's own.
//   - the block linking's premise, an edge on at most two triangles before anything is merged: a rim edge of the march's mesh lay on one
//     triangle and gets the one cap triangle of its face-triangle; an edge inside a face lies on the two cap triangles beside it; an edge
//     of the array's box lies on one cap triangle of each of its two faces; nothing else is added.
// The windings are coherent by construction (the cap is wound with the march), so coherent = true stands as well.
extern "C" int cx_postprocess3d_capped(cx_ctx* ctx, uint32_t flags, int64_t* out_counts) {
    if (!ctx) return CX_ERR_INVALID;
    if (!ctx->extracted) { ctx->err = "cx_postprocess3d_capped: no valid extraction"; return CX_ERR_STATE; }
    if (flags & ~1u) { ctx->err = "cx_postprocess3d_capped: unknown flag bits (only bit 0, no clean-up, is defined)"; return CX_ERR_INVALID; }
    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_cap_view K;
    int rc = cx_cap_view_get(ctx, "cx_postprocess3d_capped", &K);      // (refuses the routes no cap is built for; nothing is written before)
    if (rc) return rc;
    cx_post_state* S;
    if ((rc = cxp_state(ctx, &S))) return rc;
    const uint32_t nv0 = (uint32_t)ctx->counts.n_vertices, nt0 = (uint32_t)ctx->counts.n_triangles;
    const uint32_t nv = nv0 + K.ncv, nt = nt0 + K.nct;
    hipStream_t st = ctx->stream;
    int64_t counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    cxp_begin(ctx, S);
    if ((rc = cxp_reserve_raw(ctx, S, nv, nt, true))) return rc;
    const cx_params& P = ctx->last;
    // ON PURPOSE: the origin is zero and cx_set_reference_corner is ignored (unlike cx_postprocess3d_ex): the cap's lattice points are
    // those of the array that was marched, and the corner that of that array
    const cxp_origin3 org{{0.0, 0.0, 0.0}};
    if (nv && nt) {
        if ((rc = cxp_raw_from_extraction(ctx, S, org, nt, nullptr))) return rc;      // (alive bytes for the cap's triangles too)
        if (K.ncv) cxp_launch_vertices_f64(dim3(cx_blocks(K.ncv)), st, P.grid, ctx->grid64_valid ? ctx->grid64.get() : nullptr, P.n1, P.n2, P.div_plane, P.div_row,
                                           P.value, K.vrec, K.ncv, S->raw.pts + (size_t)nv0 * 3, S->raw.prio + nv0, org);
        if (K.nct) CX_HIP(ctx, hipMemcpyAsync(S->raw.tri + (size_t)nt0 * 3, K.tris, (size_t)K.nct * 3 * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    }
    const double corner[3] = {(double)(P.n0 - 1), (double)(P.n1 - 1), (double)(P.n2 - 1)};
    if ((rc = cxp_run3d(ctx, S, nv, nt, corner, nullptr, !(flags & 1u), 0.0, true, counts, true))) return rc;
    S->rec.capped = true;
    return cxp_publish(ctx, S, cxp_record::MESH3D, cxp_record::GRID, counts, out_counts);
}
bool cx_level1_capped(cx_ctx* ctx) { return cxp_mesh3d(ctx) && ctx->post->rec.capped; }

static bool cxp_shard_open(const cx_ctx* ctx) { return ctx->post && ctx->post->rec.holds == cxp_record::SHARD_OPEN; }
// ---- sharded Level 1 (the reference is one process: tetrahedral.py:190-215, 353-375, surface_geometry.py:14-140) ----
// The context holds the extraction of a slab that was marched TOGETHER with two layers of cells of each neighbour slab
// (cx_set_origin = where the local array starts in the whole volume, cx_set_reference_corner = the whole volume's corner).
// Weld buckets are narrower than a cell and never straddle an integer plane (tetrahedral.py:192-196), tiny and degenerate
// triangles chain around one lattice point: with two layers, everything this step decides about the slab's own cells and
// about the FIRST layer of its neighbours is what the undivided volume decides.  Components and the max-x rule are global:
// begin() labels the components of own + first-layer triangles and leaves, for the host to exchange, the first-layer and
// own-boundary triangles with their labels and one start-triangle candidate per component that reaches them (sizes follow the
// slab boundary); finish() takes the agreed flips for those components.  own_lo / own_hi: own cell layers of the local array.
extern "C" int cx_postprocess3d_shard_begin(cx_ctx* ctx, uint32_t flags, int64_t own_lo, int64_t own_hi, int64_t* out_counts,
                                            int64_t* n_own_lower, int64_t* n_upper_copies, int64_t* n_candidates) {
    if (!ctx || !n_own_lower || !n_upper_copies || !n_candidates) return CX_ERR_INVALID;
    if (!ctx->extracted) { ctx->err = "cx_postprocess3d_shard_begin: no valid extraction"; return CX_ERR_STATE; }
    const cx_params& P = ctx->last;
    if (own_lo < 0 || own_hi <= own_lo || own_hi > (int64_t)P.n0 - 1) { ctx->err = "cx_postprocess3d_shard_begin: own cell layers outside the local array"; return CX_ERR_INVALID; }
    if (ctx->keep_valid) { ctx->err = "cx_postprocess3d_shard_begin: not after a seeded selection"; return CX_ERR_STATE; }
    if (ctx->origin[0] < 0) { ctx->err = "cx_postprocess3d_shard_begin: the local array starts before the volume (cx_set_origin)"; return CX_ERR_STATE; }
    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_post_state* S;
    int rc = cxp_state(ctx, &S);
    if (rc) return rc;
    const uint32_t nv = (uint32_t)ctx->counts.n_vertices, nt = (uint32_t)ctx->counts.n_triangles;
    int64_t counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    cxp_begin(ctx, S);
    if ((rc = cxp_reserve_raw(ctx, S, nv, nt, true))) return rc;
    // coordinates of the WHOLE volume, added to the lattice points before the interpolation: bit for bit what the undivided
    // volume computes, so that the weld buckets truncate identically
    const cxp_origin3 org{{(double)ctx->origin[0], (double)ctx->origin[1], (double)ctx->origin[2]}};
    if (nv && nt && (rc = cxp_raw_from_extraction(ctx, S, org, nt, nullptr))) return rc;
    double corner[3];
    cxp_corner_of(ctx, corner);
    const cxp_shard sh{P.n1 * P.n2, (uint32_t)own_lo, (uint32_t)own_hi, P.n0 - 1};
    if ((rc = cxp_run3d(ctx, S, nv, nt, corner, nullptr, !(flags & 1u), 0.0, true, counts, true, &sh))) return rc;
    cxp_publish(ctx, S, cxp_record::SHARD_OPEN, cxp_record::SHARD, counts, out_counts);
    *n_own_lower = S->shard.n1;
    *n_upper_copies = S->shard.n4;
    *n_candidates = S->shard.ncand;
    return CX_OK;
}

// One of the two boundary lists of cx_postprocess3d_shard_begin: which = 1, this slab's own triangles next to its LOWER neighbour
// (n_own_lower entries); which = 4, its copies of the UPPER neighbour's first layer (n_upper_copies).  Per triangle a 64-bit hash
// of its three original edge ids in the numbering of the whole volume, and its component label here.  Rank r's list 4 and rank
// r+1's list 1 hold the same triangles: sorted by hash they pair up the labels.  hash / label: DEVICE OR HOST memory (the lists
// are meant to stay on the device: a torch tensor sorts and sends them).
extern "C" int cx_postprocess3d_shard_boundary(cx_ctx* ctx, int which, uint64_t* hash, uint32_t* label) {
    if (!ctx || (which != 1 && which != 4)) return CX_ERR_INVALID;
    if (!cxp_shard_open(ctx)) { ctx->err = "cx_postprocess3d_shard_boundary: call cx_postprocess3d_shard_begin first"; return CX_ERR_STATE; }
    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_post_state* S = ctx->post;
    const size_t n1 = S->shard.n1, n4 = S->shard.n4;
    const size_t n = which == 1 ? n1 : n4;
    if (!n) return CX_OK;
    if (!hash || !label) return CX_ERR_INVALID;
    const cxp_bnd B = cxp_bnd_view(S, n1, n4);
    CX_HIP(ctx, hipMemcpyAsync(hash, which == 1 ? B.hash1 : B.hash4, n * sizeof(u64), hipMemcpyDefault, ctx->stream));
    CX_HIP(ctx, hipMemcpyAsync(label, which == 1 ? B.label1 : B.label4, n * sizeof(uint32_t), hipMemcpyDefault, ctx->stream));
    CX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CX_OK;
}

// the start-triangle candidates of cx_postprocess3d_shard_begin (host arrays of n_candidates entries): per component that reaches
// a neighbour its label and, among this slab's OWN triangles (surface_geometry.py:79-103): x of the max-x vertex, that vertex's
// edge id (local: add (origin_x * n1 * n2) << 3 for the whole volume's), |normal_x| of the start triangle, 1 if its normal_x is
// negative; has = 0 if the component has no own triangle here.
extern "C" int cx_postprocess3d_shard_candidates(cx_ctx* ctx, uint32_t* cand_label, double* cand_x, uint32_t* cand_vertex_key, double* cand_nx,
                                                 uint8_t* cand_negative, uint8_t* cand_has) {
    if (!ctx) return CX_ERR_INVALID;
    if (!cxp_shard_open(ctx)) { ctx->err = "cx_postprocess3d_shard_candidates: call cx_postprocess3d_shard_begin first"; return CX_ERR_STATE; }
    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_post_state* S = ctx->post;
    const size_t nc = S->shard.ncand;
    if (!nc) return CX_OK;
    if (!cand_label || !cand_x || !cand_vertex_key || !cand_nx || !cand_negative || !cand_has) return CX_ERR_INVALID;
    const cxp_cand* cand = cxp_bnd_view(S, S->shard.n1, S->shard.n4).cand;
    std::vector<cxp_cand> h(nc);
    CX_HIP(ctx, hipMemcpyAsync(h.data(), cand, nc * sizeof(cxp_cand), hipMemcpyDeviceToHost, ctx->stream));
    CX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < nc; i++) {
        cand_label[i] = h[i].label; cand_x[i] = h[i].x; cand_vertex_key[i] = h[i].vkey; cand_nx[i] = h[i].nx;
        cand_negative[i] = (uint8_t)h[i].sign; cand_has[i] = (uint8_t)h[i].has;
    }
    return CX_OK;
}

// flips[i] (0 / 1) for component labels[i] of cx_postprocess3d_shard_candidates: the decision of the rank that holds the component's
// start triangle.  Components that reach no neighbour keep the local decision.  Afterwards cx_level1_download /
// cx_level1_download_keys / cx_level1_write hand out this slab's OWN triangles and the vertices they use, in the coordinates
// of the whole volume.  out_counts as cx_postprocess3d ([0] vertices, [1] triangles, [4] components seen locally).
extern "C" int cx_postprocess3d_shard_finish(cx_ctx* ctx, const uint32_t* labels, const uint8_t* flips, int64_t n, int64_t* out_counts) {
    if (!ctx || n < 0 || (n && (!labels || !flips))) return CX_ERR_INVALID;
    if (!cxp_shard_open(ctx)) { ctx->err = "cx_postprocess3d_shard_finish: call cx_postprocess3d_shard_begin first"; return CX_ERR_STATE; }
    if (n > (int64_t)ctx->post->shard.nt2) { ctx->err = "cx_postprocess3d_shard_finish: more labels than triangles"; return CX_ERR_INVALID; }
    CX_HIP(ctx, hipSetDevice(ctx->device));
    return cxp_shard_finish(ctx, ctx->post, labels, flips, (uint32_t)n, out_counts);
}

// edge id ((linear index of the lower lattice point << 3) | direction, local to the array that was marched) of every vertex of
// cx_level1_download, in its order: the identity of a Level-1 vertex across slabs and runs (the representative that survived
// weld, tiny collapse and clean-up)
extern "C" int cx_level1_download_keys(cx_ctx* ctx, uint32_t* keys) {
    if (!ctx || !keys) return CX_ERR_INVALID;
    if (!cxp_mesh3d(ctx)) { ctx->err = "cx_level1_download_keys: run cx_postprocess3d first"; return CX_ERR_STATE; }
    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_post_state* S = ctx->post;
    if (!S->nv_out) return CX_OK;
    return cx_copy_to_host1(ctx, keys, S->keys_out.get(), (size_t)S->nv_out * sizeof(uint32_t));
}

// float64 coordinates of the Level-0 vertices exactly as the reference interpolates them (tetrahedral.py:471-487) in the
// grid coordinates of the whole volume (the origin of cx_set_origin is added to the lattice points BEFORE the
// interpolation, so a slab yields bit for bit what the whole volume would), in the order of cx_level0_download -- what cx_postprocess3d works on, for callers that assemble the meshes of several slabs
extern "C" int cx_level0_points_f64(cx_ctx* ctx, double* points_xyz) {
    if (!ctx || !points_xyz) return CX_ERR_INVALID;
    if (!ctx->extracted) { ctx->err = "cx_level0_points_f64: no valid extraction"; return CX_ERR_STATE; }
    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_post_state* S;
    int rc = cxp_state(ctx, &S);
    if (rc) return rc;
    const uint32_t nv = (uint32_t)ctx->counts.n_vertices;
    if (!nv) return CX_OK;
    cxp_begin(ctx, S);         // (the points go where the post-pass starts from: the buffers no longer hold a Level-1 mesh)
    if ((rc = S->pts.grow(ctx, (size_t)(nv + 1) * 3 * sizeof(double)))) return rc;
    if ((rc = S->prio.grow(ctx, (size_t)(nv + 1) * sizeof(uint32_t)))) return rc;
    const cx_params& P = ctx->last;
    const cxp_origin3 org{{(double)ctx->origin[0], (double)ctx->origin[1], (double)ctx->origin[2]}};
    cxp_launch_vertices_f64(dim3(cx_blocks(nv)), ctx->stream, P.grid, ctx->grid64_valid ? ctx->grid64.get() : nullptr, P.n1, P.n2,
                       P.div_plane, P.div_row, P.value, ctx->verts.get(), nv, S->pts.as<double>(), S->prio.as<uint32_t>(), org);
    return cx_copy_to_host1(ctx, points_xyz, S->pts.get(), (size_t)nv * 3 * sizeof(double));
}

// Level 1 of a Level-0 mesh handed over by the caller, e.g. assembled from the slabs of several GPUs: vertices in
// ASCENDING EDGE-ID ORDER (their index is their priority) with the coordinates of cx_level0_points_f64 in the grid
// coordinates of the whole volume, triangles as indices wound as the march wound them.
extern "C" int cx_postprocess3d_mesh(cx_ctx* ctx, const double* points_xyz, int64_t nv64, const int32_t* tris, int64_t nt64, const int64_t* corner3,
                                     uint32_t flags, double smooth, int64_t* out_counts) {
    if (!ctx || !corner3 || nv64 < 0 || nt64 < 0 || (nv64 && !points_xyz) || (nt64 && !tris)) return CX_ERR_INVALID;
    if (nv64 >= 0x7FFFFFFFLL || nt64 >= 0x7FFFFFFFLL || corner3[0] < 1 || corner3[1] < 1 || corner3[2] < 1) {
        ctx->err = "cx_postprocess3d_mesh: corner >= 1 per axis and fewer than 2^31 vertices / triangles";
        return CX_ERR_INVALID;
    }
    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_post_state* S;
    int rc = cxp_state(ctx, &S);
    if (rc) return rc;
    const uint32_t nv = (uint32_t)nv64, nt = (uint32_t)nt64;
    {   // a bad index would be a fault on the device (smallest and largest index: a loop without an exit, which the compiler vectorises;
        // with the comparison and its return inside, 67 M iterations took their 10 ms one by one)
        int32_t lo = 0, hi = -1;
        for (int64_t n = 0; n < nt64 * 3; n++) { lo = tris[n] < lo ? tris[n] : lo; hi = tris[n] > hi ? tris[n] : hi; }
        if (lo < 0 || (int64_t)hi >= nv64) { ctx->err = "cx_postprocess3d_mesh: triangle index out of range"; return CX_ERR_INVALID; }
    }
    hipStream_t st = ctx->stream;
    int64_t counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    cxp_begin(ctx, S);         // (the input is good: from here on the resident mesh is gone)
    if ((rc = cxp_reserve_raw(ctx, S, nv, nt, true))) return rc;
    if (nv && nt) {
        CX_HIP(ctx, hipMemcpyAsync(S->pts.get(), points_xyz, (size_t)nv * 3 * sizeof(double), hipMemcpyHostToDevice, st));
        CX_HIP(ctx, hipMemcpyAsync(S->tri.get(), tris, (size_t)nt * 3 * sizeof(int32_t), hipMemcpyHostToDevice, st));
        CX_HIP(ctx, hipMemsetAsync(S->alive.get(), 1, nt, st));
        hipLaunchKernelGGL(cxp_k_iota_prio, dim3(cx_blocks(nv)), dim3(256), 0, st, S->prio.as<uint32_t>(), nv);
    }
    const double corner[3] = {(double)corner3[0], (double)corner3[1], (double)corner3[2]};
    if ((rc = cxp_run3d(ctx, S, nv, nt, corner, nullptr, !(flags & 1u), smooth, !(flags & 4u), counts, false, nullptr, (flags & 8u) != 0u))) return rc;
    return cxp_publish(ctx, S, cxp_record::MESH3D, cxp_record::CALLER_MESH, counts, out_counts);
}

extern "C" int cx_level1_download(cx_ctx* ctx, double* points_xyz, int32_t* tris) {
    if (!ctx) return CX_ERR_INVALID;
    if (!cxp_mesh3d(ctx)) { ctx->err = "cx_level1_download: run cx_postprocess3d first"; return CX_ERR_STATE; }
    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_post_state* S = ctx->post;
    void* d[2] = {(points_xyz && S->nv_out) ? (void*)points_xyz : nullptr, (tris && S->nt_out) ? (void*)tris : nullptr};
    const void* sp[2] = {S->pts_out.get(), S->tri_out.get()};
    const size_t nb[2] = {(size_t)S->nv_out * 3 * sizeof(double), (size_t)S->nt_out * 3 * sizeof(int32_t)};
    return cx_copy_to_host(ctx, 2, d, sp, nb);   // pinned, double-buffered, several host threads (cx_xfer.hip)
}

// device pointers of the Level-1 mesh: for consumers that live on the GPU (a torch tensor, a renderer's vertex buffer) the 541 MB
// download of a 512^3 mesh -- 60 % of the API path's time -- never has to happen.  Everything enqueued on the context's stream
// is complete when this returns.
extern "C" int cx_level1_device_ptrs(cx_ctx* ctx, void** points_xyz, void** tris, int64_t* n_vertices, int64_t* n_triangles) {
    if (!ctx) return CX_ERR_INVALID;
    if (!cxp_mesh3d(ctx)) { ctx->err = "cx_level1_device_ptrs: run cx_postprocess3d first"; return CX_ERR_STATE; }
    CX_HIP(ctx, hipSetDevice(ctx->device));
    CX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    cx_post_state* S = ctx->post;
    if (points_xyz) *points_xyz = S->nv_out ? S->pts_out.get() : nullptr;
    if (tris) *tris = S->nt_out ? S->tri_out.get() : nullptr;
    if (n_vertices) *n_vertices = (int64_t)S->nv_out;
    if (n_triangles) *n_triangles = (int64_t)S->nt_out;
    return CX_OK;
}

// ---- what the vertex attributes (cx_attr.hip) need from the Level-1 state ------------------------------------------------------------
// One byte per output vertex: the flip of the component its triangles belong to (cflip of the component's root, cxp_k_comp_decide).
// Every triangle of a component stores the same value, so the result does not depend on the launch order for a vertex whose
// triangles all lie in one component; plain byte stores, no atomics.
__global__ void cxp_k_vertex_flip(const int32_t* __restrict__ tri, uint32_t nt, const u64* __restrict__ parent, const u64* __restrict__ cflip,
                                  uint8_t* __restrict__ vflip) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const uint8_t f = (uint8_t)(cflip[(uint32_t)parent[t]] & 1u);
    if (!f) return;                       // (the bytes start at zero)
#pragma unroll
    for (int k = 0; k < 3; k++) vflip[(uint32_t)tri[(size_t)t * 3 + k]] = 1;
}
// what the two views answer without a 3-D mesh: CX_ERR_INVALID; where the 4-D post-pass's result lies in the buffers instead, CX_ERR_STATE
// with the view's text for tables that are gone (that pass took their memory)
static int cxp_no_mesh3d(cx_ctx* ctx, const char* who, const char* gone) {
    const bool tets = cxp_tets4d(ctx);
    ctx->err = std::string(who) + (tets ? gone : ": no Level-1 mesh (run cx_postprocess3d first)");
    return tets ? CX_ERR_STATE : CX_ERR_INVALID;
}
static const char CXP_ATTR_GONE[] = ": the orientation tables of the post-pass are gone (run cx_postprocess3d again)";
static const char CXP_COMP_GONE[] = ": the orientation tables of the post-pass are gone (a 4-D pass used their memory, or the post-pass ran without the orientation step): run cx_postprocess3d again";
int cx_level1_attr_view(cx_ctx* ctx, const char* who, cx_level1_view* out) {
    if (!cxp_mesh3d(ctx)) return cxp_no_mesh3d(ctx, who, CXP_ATTR_GONE);
    cx_post_state* S = ctx->post;
    if (S->rec.origin != cxp_record::GRID) {
        ctx->err = std::string(who) + (S->rec.origin == cxp_record::CLIPPED ? ": the vertices of a clipped mesh (cx_level1_clip_*) are not all edge crossings of the resident array"
                                       : S->rec.origin == cxp_record::SIMPLIFIED ? ": the vertices of a simplified mesh (cx_level1_simplify) are cluster means, not edge crossings of the resident array"
                                                     : ": the Level-1 vertices are not edge crossings of the resident array (a mesh handed to cx_postprocess3d_mesh, or a shard)");
        return CX_ERR_UNSUPPORTED;
    }
    const uint32_t nv = (uint32_t)S->nv_out, nt = (uint32_t)S->nt_out;
    if (nv && !S->rec.vflip_cached) {
        if (nt && !S->rec.tables_for(nt)) { ctx->err = std::string(who) + CXP_ATTR_GONE; return CX_ERR_STATE; }
        int rc;
        if ((rc = S->vflip.grow(ctx, (size_t)nv + 16))) return rc;
        CX_HIP(ctx, hipMemsetAsync(S->vflip.get(), 0, nv, ctx->stream));
        if (nt) {
            const u64* parent = S->parent.as<const u64>();
            const u64* cflip = cxp_comp_view(S->comp.as<u64>(), nt).cflip;
            hipLaunchKernelGGL(cxp_k_vertex_flip, dim3(cx_blocks(nt)), dim3(256), 0, ctx->stream, S->tri_out.as<const int32_t>(), nt, parent, cflip, S->vflip.as<uint8_t>());
            CX_HIP(ctx, hipGetLastError());
        }
        S->rec.vflip_cached = true;
    }
    out->keys = S->keys_out.as<const uint32_t>();
    out->vflip = S->vflip.as<const uint8_t>();
    out->nv = nv;
    return CX_OK;
}

// ---- what the components (cx_comp.hip) need from the Level-1 state --------------------------------------------------------------------
// The tables of the orientation step as they stand after cxp_k_orient: parent[t] = (parity << 32) | root, flattened, the root being the
// smallest triangle index of the component (every union keeps the smaller root); cflip[root] = the root's flip.  Nothing here needs
// edge ids, so the meshes of cx_postprocess3d_mesh are served too; a shard's components reach other ranks: CX_ERR_UNSUPPORTED.
// carried normals (cx_simplify.hip) of the vertices that stay, in their order: vnew[v] = new index (0xFFFFFFFF or use[v] == 0: gone)
__global__ void cxp_k_carry_normals(const double* __restrict__ in, const uint32_t* __restrict__ use, const uint32_t* __restrict__ vnew, uint32_t n,
                                    double* __restrict__ out) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n || (use && !use[v])) return;
    const uint32_t j = vnew[v];
    if (j == 0xFFFFFFFFu) return;
#pragma unroll
    for (int a = 0; a < 3; a++) out[(size_t)j * 3 + a] = in[(size_t)v * 3 + a];
}
int cx_level1_comp_view_get(cx_ctx* ctx, const char* who, cx_level1_comp_view* out) {
    if (!cxp_mesh3d(ctx)) return cxp_no_mesh3d(ctx, who, CXP_COMP_GONE);
    cx_post_state* S = ctx->post;
    if (S->rec.origin == cxp_record::SHARD) {
        ctx->err = std::string(who) + ": the components of a sharded Level-1 mesh reach other ranks (cx_postprocess3d_shard_*): not available";
        return CX_ERR_UNSUPPORTED;
    }
    const uint32_t nv = (uint32_t)S->nv_out, nt = (uint32_t)S->nt_out;
    if (nt && !S->rec.tables_for(nt)) {
        ctx->err = std::string(who) + CXP_COMP_GONE;
        return CX_ERR_STATE;
    }
    out->parent = S->parent.as<const u64>();
    out->cflip = nt ? cxp_comp_view(S->comp.as<u64>(), nt).cflip : nullptr;
    out->tri = S->tri_out.as<const int32_t>();
    out->pts = S->pts_out.as<const double>();
    out->keys = S->keys_out.as<const uint32_t>();
    out->nv = nv; out->nt = nt;
    for (int a = 0; a < 3; a++) out->corner[a] = S->corner[a];
    out->gen = S->rec.gen;
    return CX_OK;
}
// room for a filtered copy of the mesh and its tables in buffers the post-pass is done with (the march's points and triangles, the key
// scratch, the edge table), as cxp_shard_finish uses them: nothing is allocated once they have their size
int cx_level1_comp_scratch_get(cx_ctx* ctx, cx_level1_comp_scratch* out) {
    cx_post_state* S = ctx->post;
    const size_t nv = (size_t)S->nv_out, nt = (size_t)S->nt_out;
    int rc;
    if ((rc = S->pts.grow(ctx, (nv + 1) * 3 * sizeof(double)))) return rc;
    if ((rc = S->tri.grow(ctx, (nt + 1) * 3 * sizeof(int32_t)))) return rc;
    if ((rc = S->keys_tmp.grow(ctx, (nv + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = S->tkeys.grow(ctx, (nt + 1) * 2 * sizeof(u64)))) return rc;
    out->pts = S->pts.as<double>();
    out->tri = S->tri.as<int32_t>();
    out->keys = S->keys_tmp.as<uint32_t>();
    out->parent = S->tkeys.as<u64>();
    out->cflip = out->parent + nt + 1;
    return CX_OK;
}
// the filtered copy becomes the Level-1 mesh: every reader of the state (download, device pointers, keys, files, normals) serves it
int cx_level1_comp_commit(cx_ctx* ctx, uint32_t nv_new, uint32_t nt_new, const uint32_t* vuse, const uint32_t* vnew) {
    cx_post_state* S = ctx->post;
    hipStream_t st = ctx->stream;
    const cxp_record before = S->rec;
    cxp_begin(ctx, S);
    if (before.normals_carried && nv_new && S->nv_out) {       // the carried normals of a simplified mesh follow their vertices
        const int rcn = S->nrm[1 - S->nrm_cur].grow(ctx, ((size_t)nv_new + 1) * 3 * sizeof(double));
        if (rcn) return rcn;
        hipLaunchKernelGGL(cxp_k_carry_normals, dim3(cx_blocks((size_t)S->nv_out)), dim3(256), 0, st, S->nrm[S->nrm_cur].as<const double>(), vuse, vnew,
                           (uint32_t)S->nv_out, S->nrm[1 - S->nrm_cur].as<double>());
        S->nrm_cur = 1 - S->nrm_cur;
    }
    const size_t nt_old = (size_t)S->nt_out;
    const u64* parent_new = S->tkeys.as<const u64>();
    if (nv_new) {
        CX_HIP(ctx, hipMemcpyAsync(S->pts_out.get(), S->pts.get(), (size_t)nv_new * 3 * sizeof(double), hipMemcpyDeviceToDevice, st));
        CX_HIP(ctx, hipMemcpyAsync(S->keys_out.get(), S->keys_tmp.get(), (size_t)nv_new * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    }
    if (nt_new) {
        CX_HIP(ctx, hipMemcpyAsync(S->tri_out.get(), S->tri.get(), (size_t)nt_new * 3 * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        CX_HIP(ctx, hipMemcpyAsync(S->parent.get(), parent_new, (size_t)nt_new * sizeof(u64), hipMemcpyDeviceToDevice, st));
        CX_HIP(ctx, hipMemcpyAsync(cxp_comp_view(S->comp.as<u64>(), nt_new).cflip, parent_new + nt_old + 1, (size_t)nt_new * sizeof(u64), hipMemcpyDeviceToDevice, st));
    }
    CX_HIP(ctx, hipStreamSynchronize(st));
    S->nv_out = nv_new; S->nt_out = nt_new;
    // a filtered copy keeps where the mesh came from, its cap and its normals; its tables are the filtered ones; the vertex flips are
    // written again from them on the next request, and the map of an earlier simplification no longer fits
    S->rec.capped = before.capped; S->rec.normals_carried = before.normals_carried;
    S->rec.tables_live = before.tables_live; S->rec.tables_nt = nt_new;
    return cxp_publish(ctx, S, cxp_record::MESH3D, before.origin, nullptr, nullptr);
}

// ---- what the simplification (cx_simplify.hip) needs from the Level-1 state ------------------------------------------------------------
// The clusters' points, priorities (= first member, ascending with the cluster id), remapped triangles with their priorities (the old
// triangle index, three times) and alive bytes go into the buffers the post-pass starts from; cx_level1_simplify_tail then drops
// triangles that became the same vertex set and runs the shared tail (clean, compaction, orientation with the windings taken as
// coherent) on them, exactly the kernels cxp_run3d ends with.  Nothing is uploaded; nothing is allocated once the buffers have their size.
int cx_level1_simplify_bufs(cx_ctx* ctx, bool normals, bool dry_run, cx_level1_simplify_io* out) {
    cx_post_state* S = ctx->post;
    const size_t nv = (size_t)S->nv_out, nt = (size_t)S->nt_out;
    int rc;
    // (without S->parent: it holds the tables of the orientation step the mesh still needs if the call fails, and
    // without S->rep, which a dry run takes for the map below)
    if ((rc = cxp_reserve_raw(ctx, S, nv, nt))) return rc;
    // (a dry run leaves the map of the last simplification alone: its cluster ids go into the weld's scratch)
    if ((rc = (dry_run ? S->rep : S->smap).grow(ctx, (nv + 16) * sizeof(int32_t)))) return rc;
    if (normals && (rc = S->nrm_tmp.grow(ctx, (nv + 1) * 3 * sizeof(double)))) return rc;
    out->pts = S->raw.pts; out->prio = S->raw.prio; out->tri = S->raw.tri; out->tprio3 = S->raw.tprio3; out->alive = S->raw.alive;
    out->map = (dry_run ? S->rep : S->smap).as<int32_t>();
    out->nrm_new = normals ? S->nrm_tmp.as<double>() : nullptr;
    out->nrm_src = S->rec.normals_carried ? S->nrm[S->nrm_cur].as<const double>() : nullptr;
    out->simplified = S->rec.derived();
    if (!dry_run) S->rec.map_live = false;
    return CX_OK;
}
// new index of every OLD vertex: through the cluster, the vertex the clean-up merged the cluster into (if any), the compaction
__global__ void cxp_k_simplify_map(int32_t* map, uint32_t nv_old, uint32_t ncl, const u64* parent2, const uint32_t* vnew) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv_old) return;
    int32_t c = map[v];
    if (c < 0 || (uint32_t)c >= ncl) { map[v] = -1; return; }
    if (parent2) { uint32_t par; c = (int32_t)cxp_find(parent2, (uint32_t)c, par); }
    map[v] = (int32_t)vnew[c];       // (0xFFFFFFFF where no surviving triangle uses it)
}
int cx_level1_simplify_tail(cx_ctx* ctx, uint32_t nv_old, uint32_t ncl, uint32_t nt, bool do_clean, bool normals, int64_t* counts) {
    cx_post_state* S = ctx->post;
    hipStream_t st = ctx->stream;
    int rc;
    const int cur = S->nrm_cur;
    cxp_begin(ctx, S);      // (the raw mesh is written; from here on the outputs are: a failure leaves no mesh)
    if (nt && ncl) {
        const u64 tsz = cx_table_size(nt);
        if ((rc = S->tkeys.grow(ctx, tsz * sizeof(u64)))) return rc;
        cxp_dedupe(ctx, S, S->raw.tri, S->raw.tprio3, S->raw.alive, nt, tsz, nullptr);
    }
    // (the compaction writes the new id of every vertex in use: the others keep -1)
    if ((rc = S->scan.grow(ctx, ((size_t)ncl + 16) * sizeof(uint32_t)))) return rc;
    if (ncl) CX_HIP(ctx, hipMemsetAsync(S->scan.get(), 0xFF, (size_t)ncl * sizeof(uint32_t), st));
    if (normals && (rc = S->nrm[1 - cur].grow(ctx, ((size_t)ncl + 1) * 3 * sizeof(double)))) return rc;
    if ((rc = cxp_clean_orient(ctx, S, ncl, nt, do_clean, true, counts, true))) return rc;
    const uint32_t* vnew = S->scan.as<const uint32_t>();
    if (nv_old) hipLaunchKernelGGL(cxp_k_simplify_map, dim3(cx_blocks(nv_old)), dim3(256), 0, st, S->smap.as<int32_t>(), nv_old, ncl,
                                   (do_clean && nt) ? S->parent2.as<const u64>() : (const u64*)nullptr, vnew);
    if (normals && ncl && S->nv_out) {
        hipLaunchKernelGGL(cxp_k_carry_normals, dim3(cx_blocks(ncl)), dim3(256), 0, st, S->nrm_tmp.as<const double>(), (const uint32_t*)nullptr, vnew, ncl,
                           S->nrm[1 - cur].as<double>());
        S->nrm_cur = 1 - cur;
    }
    CX_HIP(ctx, hipGetLastError());
    CX_HIP(ctx, hipStreamSynchronize(st));
    S->rec.normals_carried = normals;
    S->rec.map_live = true; S->rec.map_n = nv_old;
    return cxp_publish(ctx, S, cxp_record::MESH3D, cxp_record::SIMPLIFIED, nullptr, nullptr);
}
// 0: the mesh is not a simplified one; 1: simplified, *nrm = its carried normals; 2: simplified without normals
int cx_level1_carried_normals(cx_ctx* ctx, const double** nrm, uint32_t* nv) {
    cx_post_state* S = ctx->post;
    if (!cxp_mesh3d(ctx) || !S->rec.derived()) return 0;
    *nv = (uint32_t)S->nv_out;
    *nrm = S->rec.normals_carried ? S->nrm[S->nrm_cur].as<const double>() : nullptr;
    return S->rec.normals_carried ? 1 : 2;
}
int cx_level1_simplify_map_get(cx_ctx* ctx, const int32_t** map, uint32_t* n) {
    cx_post_state* S = ctx->post;
    if (!cxp_mesh3d(ctx) || !S->rec.map_live) {
        ctx->err = "cx_level1_simplify_map: no simplification since the last post-pass or filter";
        return CX_ERR_STATE;
    }
    *map = S->smap.as<const int32_t>(); *n = S->rec.map_n;
    return CX_OK;
}

// ---- what the clip (cx_clip.hip) needs from the Level-1 state ---------------------------------------------------------------------------
// Siblings of the two simplify calls for a mesh that GROWS: nv_raw = the old vertices and the cut vertices, nt_raw = the triangles the
// clip emits (up to two per source triangle); every one of them is alive.  The buffers are the ones the post-pass starts from; the
// resident mesh (pts_out, tri_out, keys_out and the tables of the orientation step) is not touched before the tail.
int cx_level1_clip_bufs(cx_ctx* ctx, size_t nv_raw, size_t nt_raw, cx_level1_clip_io* out) {
    cx_post_state* S = ctx->post;
    int rc;
    if ((rc = cxp_reserve_raw(ctx, S, nv_raw, nt_raw))) return rc;
    out->pts = S->raw.pts; out->prio = S->raw.prio; out->tri = S->raw.tri; out->tprio3 = S->raw.tprio3; out->alive = S->raw.alive;
    return CX_OK;
}
// clean (optional), compaction, orientation with the windings taken as coherent: the kernels cxp_run3d ends with.  The result is a
// derived mesh in the sense of the simplification (its keys are not edge ids); it carries no normals until cx_level1_clip_normals.
int cx_level1_clip_tail(cx_ctx* ctx, uint32_t nv_raw, uint32_t nt_raw, bool do_clean, int64_t* counts) {
    cx_post_state* S = ctx->post;
    int rc;
    cxp_begin(ctx, S);
    if ((rc = cxp_clean_orient(ctx, S, nv_raw, nt_raw, do_clean, true, counts, true))) return rc;
    CX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return cxp_publish(ctx, S, cxp_record::MESH3D, cxp_record::CLIPPED, nullptr, nullptr);
}
// room for the normals the clipped mesh carries (one per vertex of it, written by the caller on the context's stream).  The clip reads
// its source's normals from the copy cx_level1_normals made (carried ones included), never from nrm[] itself, so the new ones take
// the current buffer: changing over to the other one, as the simplification and the component filter must, gave the second buffer its
// size only at the second clip, an allocation in the steady state of clip, post-pass, clip
int cx_level1_clip_normals(cx_ctx* ctx, double** out) {
    cx_post_state* S = ctx->post;
    const int cur = S->nrm_cur;
    const int rc = S->nrm[cur].grow(ctx, ((size_t)S->nv_out + 1) * 3 * sizeof(double));
    if (rc) return rc;
    *out = S->nrm[cur].as<double>();
    S->rec.normals_carried = true;
    return CX_OK;
}
// the generation of the Level-1 mesh (0: there is none): what another translation unit caches belongs to one value of it
uint64_t cx_level1_generation(cx_ctx* ctx) {
    cx_post_state* S = ctx->post;
    return cxp_mesh3d(ctx) ? S->rec.gen : 0;
}

// SurfaceGeometry(vertices, triangles) on a caller's mesh.  mode: 0 = orient only, 1 = clean + orient, 2 = clean only.
extern "C" int cx_surface_geometry(cx_ctx* ctx, double* points_xyz, int64_t* nv_io, int32_t* tris, int64_t* nt_io, int mode) {
    if (!ctx || !points_xyz || !tris || !nv_io || !nt_io || mode < 0 || mode > 2) return CX_ERR_INVALID;
    if (*nv_io < 0 || *nt_io < 0 || *nv_io > 0x7FFFFFF0LL || *nt_io > 0x7FFFFFF0LL) return CX_ERR_INVALID;
    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_post_state* S;
    int rc = cxp_state(ctx, &S);
    if (rc) return rc;
    const uint32_t nv = (uint32_t)*nv_io, nt = (uint32_t)*nt_io;
    for (int64_t n = 0; n < (int64_t)nt * 3; n++)
        if (tris[n] < 0 || tris[n] >= (int64_t)nv) { ctx->err = "cx_surface_geometry: triangle index out of range"; return CX_ERR_INVALID; }
    hipStream_t st = ctx->stream;
    cxp_begin(ctx, S);         // (nothing is published: the result goes back to the caller, the buffers hold no Level-1 mesh afterwards)
    if ((rc = cxp_reserve_raw(ctx, S, nv, nt))) return rc;
    int32_t* tri = S->raw.tri;
    uint32_t* tprio3 = S->raw.tprio3;
    if (nv) CX_HIP(ctx, hipMemcpyAsync(S->pts.get(), points_xyz, (size_t)nv * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    if (nt) CX_HIP(ctx, hipMemcpyAsync(tri, tris, (size_t)nt * 3 * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (nv) hipLaunchKernelGGL(cxp_k_iota_prio, dim3(cx_blocks(nv)), dim3(256), 0, st, S->prio.as<uint32_t>(), nv);
    if (nt) {
        CX_HIP(ctx, hipMemsetAsync(S->alive.get(), 1, nt, st));
        hipLaunchKernelGGL(cxp_k_tri_prio, dim3(cx_blocks(nt)), dim3(256), 0, st, tri, S->prio.as<const uint32_t>(), nt, tprio3);
        // a caller's triangle may repeat a vertex: such rows are not triangles (surface_geometry.py:63)
        hipLaunchKernelGGL(cxp_k_remap, dim3(cx_blocks(nt)), dim3(256), 0, st, tri, S->alive.as<uint8_t>(), nt, S->prio.as<const uint32_t>(),
                           (const u64*)nullptr);
    }
    int64_t counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if ((rc = cxp_clean_orient(ctx, S, nv, nt, mode != 0, mode != 2, counts, false))) return rc;   // caller's windings: arbitrary
    if (S->nv_out) CX_HIP(ctx, hipMemcpyAsync(points_xyz, S->pts_out.get(), (size_t)S->nv_out * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (S->nt_out) CX_HIP(ctx, hipMemcpyAsync(tris, S->tri_out.get(), (size_t)S->nt_out * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    CX_HIP(ctx, hipStreamSynchronize(st));
    *nv_io = S->nv_out; *nt_io = S->nt_out;
    return CX_OK;
}
