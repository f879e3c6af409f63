// cx_topo.hip -- topology of the Level-1 mesh: per component the Euler number, genus, boundary and non-manifold edge counts, and
// the boundary loops as ordered polylines (include/contourist_hip.h, "topology").  Everything is an integer: no floating point here.
//
// From the triangles, the labels of cx_comp.hip and the mesh view, on request and cached per generation of the mesh:
//   cxt_k_edges_insert     one lane per triangle: its three undirected edges {min, max} into an open-addressing table with a use count;
//                          the lane that claims a slot leaves its 3t+k there (the edge's representative)
//   cxt_k_edges_count      one lane per triangle: looks its edges up again; distinct edges (representatives), boundary edges (count 1)
//                          and non-manifold edges (representatives with count >= 3) per component, reduced within the wave first as
//                          cxc_k_measure does; the boundary mask and count per triangle for the compaction
//   cxt_k_vertices*        distinct vertices per component: by vertex label, plus the (label, vertex) pairs of corners whose triangle
//                          label is not the vertex label, made distinct through a second, small key table
//   cxt_k_compact          the boundary edges as a list in ascending 3t+k (cx_scan_u32 of the counts)
//   cxt_k_loop_*           union-find over that list through a (component, vertex) -> edge table; a set's root is its smallest list
//                          index, so ranking the roots numbers the loops in ascending smallest 3t+k
//   cxt_k_double           pointer doubling over the 2B directed edges ("darts") of the list: steps to the end of the walk that
//                          starts at the loop's smallest edge in its own direction; cxt_k_scatter places the simple loops' vertices
//   cxt_k_nonsimple        one wave walks the list in order and hands the edges of non-simple loops their rank within the loop
//   cxt_k_finish           one lane per component: the cx_topology record
#include <algorithm>
#include <cstring>
#include <new>
#include <string>

#include "cx_ctx.h"
#include "cx_dev.h"

#define CXT_END 0xFFFFFFFFu

// accumulator words per component
enum { CXT_W_F = 0, CXT_W_E = 1, CXT_W_BE = 2, CXT_W_NM = 3, CXT_W_V = 4, CXT_W_LOOPS = 5, CXT_W_NONSIMPLE = 6, CXT_WORDS = 8 };
// words of misc
enum { CXT_M_B = 0, CXT_M_L = 1, CXT_M_MISMATCH = 2, CXT_M_NONSIMPLE = 3, CXT_M_SCRATCH = 4, CXT_M_FAIL = 5, CXT_M_WORDS = 16 };

struct cx_topo_state {
    uint64_t gen = ~0ULL;                              // generation of the mesh (cx_level1_comp_view.gen) the results belong to
    uint32_t nc = 0, nl = 0, nb = 0;
    cx_buf<u64> ekeys;                                  // edge-use table: key (min << 32) | max, use count, 3t+k of the lane that claimed the slot
    cx_buf<uint32_t> ecnt, erep;
    cx_buf<uint8_t> bmask;                              // per triangle: which of its three edges are boundary edges
    cx_buf<uint32_t> bcnt, bpos;                        // their number and its exclusive scan
    cx_buf<uint32_t> sums, misc;
    cx_buf<u64> acc;
    cx_buf<cx_topology> table;
    cx_buf<u64> mkeys;                                  // (label << 32) | vertex of corners whose triangle label is not the vertex label
    // loops: per boundary edge of the list its 3t+k, tail, head, component, union-find parent, root, root flag, rank of the root, loop id
    cx_buf<uint32_t> bl, ea, eb, ec, parent, root, isroot, lidx, eloop;
    cx_buf<u64> vkeys;                                  // (component << 32) | vertex -> smallest / largest list index and number of boundary edges there
    cx_buf<uint32_t> vmin, vmax, vdeg;
    cx_buf<uint32_t> lcount, lfirst, cursor;
    cx_buf<cx_loop> loops;
    cx_buf<uint32_t> nxt[2], rnk[2];                    // pointer doubling over the darts, two copies each
    cx_buf<int32_t> lverts;
};

void cx_topo_free(cx_ctx* ctx) {
    cx_topo_state* T = ctx->topo;
    if (!T) return;
    delete T;
    ctx->topo = nullptr;
}

// ---- device helpers -----------------------------------------------------------------------------------------------------------------
// home slot in a table of cap < 2^32 slots (any size, not a power of two)
__device__ __forceinline__ uint32_t cxt_home(u64 key, uint32_t cap) { return (uint32_t)(((cxd_mix(key) >> 32) * (u64)cap) >> 32); }
// slot of key, claimed if it was not there (fresh: this lane claimed it); CXD_NONE when the table is full
__device__ __forceinline__ uint32_t cxt_insert(u64* keys, uint32_t cap, u64 key, bool& fresh) {
    uint32_t s = cxt_home(key, cap);
    fresh = false;
    for (uint32_t probe = 0; probe < cap; probe++) {
        u64 cur = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == CXD_EMPTY) {
            cur = atomicCAS(&keys[s], CXD_EMPTY, key);
            if (cur == CXD_EMPTY) { fresh = true; return s; }
        }
        if (cur == key) return s;
        s = s + 1u == cap ? 0u : s + 1u;
    }
    return CXD_NONE;
}
// slot of a key of a finished table; CXD_NONE when it is not there
__device__ __forceinline__ uint32_t cxt_find(const u64* __restrict__ keys, uint32_t cap, u64 key) {
    uint32_t s = cxt_home(key, cap);
    for (uint32_t probe = 0; probe < cap; probe++) {
        const u64 cur = keys[s];
        if (cur == key) return s;
        if (cur == CXD_EMPTY) return CXD_NONE;
        s = s + 1u == cap ? 0u : s + 1u;
    }
    return CXD_NONE;
}
__device__ __forceinline__ u64 cxt_edge_key(uint32_t a, uint32_t b) { return ((u64)(a < b ? a : b) << 32) | (u64)(a < b ? b : a); }
// union-find over list indices: a root points to itself, parents are smaller than their children, so a set's root is its smallest member.
// No path halving; every access to a parent word is a device-scope atomic (why: cx_dev.h, above cxd_uf_find)
__device__ __forceinline__ uint32_t cxt_root(uint32_t* parent, uint32_t x) {
    for (;;) {
        const uint32_t p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p >= x) return x;          // (p == x: a root; p > x never happens)
        x = p;
    }
}
__device__ __forceinline__ void cxt_union(uint32_t* parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = cxt_root(parent, a); b = cxt_root(parent, b);
        if (a == b) return;
        if (a < b) { const uint32_t w = a; a = b; b = w; }
        if (atomicCAS(&parent[a], a, b) == a) return;      // (a was still a root: it hangs below the smaller one now)
    }
}

// ---- edges --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cxt_k_edges_insert(const int32_t* __restrict__ tri, const int32_t* __restrict__ tlab, const int32_t* __restrict__ vlab,
                                                          uint32_t nt, uint32_t nv, u64* keys, uint32_t* cnt, uint32_t* rep, uint32_t cap, uint32_t* misc) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    uint32_t v[3];
#pragma unroll
    for (int k = 0; k < 3; k++) v[k] = (uint32_t)tri[(size_t)t * 3 + k];
    if (v[0] >= nv || v[1] >= nv || v[2] >= nv) return;      // (a mesh of the post-pass never fails this)
    const int32_t c = tlab[t];
    uint32_t mismatch = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        bool fresh;
        const uint32_t s = cxt_insert(keys, cap, cxt_edge_key(v[k], v[(k + 1) % 3]), fresh);
        if (s == CXD_NONE) { atomicOr(&misc[CXT_M_FAIL], 1u); continue; }
        if (fresh) rep[s] = t * 3u + (uint32_t)k;
        atomicAdd(&cnt[s], 1u);
        mismatch += vlab[v[k]] != c ? 1u : 0u;
    }
    if (mismatch) atomicAdd(&misc[CXT_M_MISMATCH], mismatch);     // (only where two components touch in a vertex)
}
// One lane per triangle.  The four small counts travel in one word (each at most 3 * 64 per wave); the lanes of a wave that share a
// label reduce among themselves and one of them issues the atomics.  Control flow around the cross-lane operations is wave-uniform.
__global__ __launch_bounds__(256) void cxt_k_edges_count(const int32_t* __restrict__ tri, const int32_t* __restrict__ tlab, uint32_t nt, uint32_t nv, uint32_t nc,
                                                         const u64* __restrict__ keys, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ rep,
                                                         uint32_t cap, uint8_t* __restrict__ bmask, uint32_t* __restrict__ bcnt, u64* __restrict__ acc,
                                                         uint32_t* misc) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    bool active = t < nt;
    int32_t label = -1;
    uint32_t packed = 0, mask = 0, nbnd = 0;       // packed: triangles | edges << 8 | boundary << 16 | non-manifold << 24
    if (active) {
        uint32_t v[3];
#pragma unroll
        for (int k = 0; k < 3; k++) v[k] = (uint32_t)tri[(size_t)t * 3 + k];
        label = tlab[t];
        active = v[0] < nv && v[1] < nv && v[2] < nv && label >= 0 && (uint32_t)label < nc;
        if (active) {
            packed = 1u;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const uint32_t s = cxt_find(keys, cap, cxt_edge_key(v[k], v[(k + 1) % 3]));
                if (s == CXD_NONE) { atomicOr(&misc[CXT_M_FAIL], 2u); continue; }
                const uint32_t uses = cnt[s];
                const bool first = rep[s] == t * 3u + (uint32_t)k;
                if (first) packed += 1u << 8;
                if (uses == 1u) { packed += 1u << 16; mask |= 1u << k; nbnd++; }
                if (first && uses >= 3u) packed += 1u << 24;
            }
        }
        bmask[t] = (uint8_t)mask;
        bcnt[t] = nbnd;
    }
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t rem = __ballot(active);
    while (rem != 0ULL) {                                   // wave-uniform
        const int leader = __ffsll((long long)rem) - 1;
        const int32_t k = __shfl(label, leader);
        const bool mine = active && label == k;
        const uint64_t grp = __ballot(mine);
        rem &= ~grp;
        const uint32_t sum = cxd_wave_add(mine ? packed : 0u);
        if ((int)lane == leader) {
            u64* w = acc + (size_t)k * CXT_WORDS;
            atomicAdd(&w[CXT_W_F], (u64)(sum & 255u));
            if ((sum >> 8) & 255u) atomicAdd(&w[CXT_W_E], (u64)((sum >> 8) & 255u));
            if ((sum >> 16) & 255u) atomicAdd(&w[CXT_W_BE], (u64)((sum >> 16) & 255u));
            if (sum >> 24) atomicAdd(&w[CXT_W_NM], (u64)(sum >> 24));
        }
    }
}

// ---- distinct vertices --------------------------------------------------------------------------------------------------------------
// every vertex once for its label (the smallest component that uses it), counted within the wave first
__global__ __launch_bounds__(256) void cxt_k_vertices(const int32_t* __restrict__ vlab, uint32_t nv, uint32_t nc, u64* __restrict__ acc) {
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
        if ((int)lane == leader) atomicAdd(&acc[(size_t)k * CXT_WORDS + CXT_W_V], (u64)__popcll(grp));
    }
}
// ... and once more for every OTHER component that uses it: the distinct (label, vertex) pairs of the corners whose triangle label is
// not the vertex label
__global__ __launch_bounds__(256) void cxt_k_vertices_shared(const int32_t* __restrict__ tri, const int32_t* __restrict__ tlab, const int32_t* __restrict__ vlab,
                                                             uint32_t nt, uint32_t nv, uint32_t nc, u64* keys, uint32_t cap, u64* __restrict__ acc, uint32_t* misc) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    uint32_t v[3];
#pragma unroll
    for (int k = 0; k < 3; k++) v[k] = (uint32_t)tri[(size_t)t * 3 + k];
    const int32_t c = tlab[t];
    if (v[0] >= nv || v[1] >= nv || v[2] >= nv || c < 0 || (uint32_t)c >= nc) return;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (vlab[v[k]] == c) continue;
        bool fresh;
        const uint32_t s = cxt_insert(keys, cap, ((u64)(uint32_t)c << 32) | (u64)v[k], fresh);
        if (s == CXD_NONE) { atomicOr(&misc[CXT_M_FAIL], 4u); continue; }
        if (fresh) atomicAdd(&acc[(size_t)c * CXT_WORDS + CXT_W_V], 1ULL);
    }
}

// ---- boundary edges and loops -------------------------------------------------------------------------------------------------------
__global__ void cxt_k_compact(const uint8_t* __restrict__ bmask, const uint32_t* __restrict__ bpos, uint32_t nt, uint32_t nb, uint32_t* __restrict__ bl) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const uint32_t m = bmask[t];
    if (!m) return;
    uint32_t p = bpos[t];
#pragma unroll
    for (int k = 0; k < 3; k++)
        if ((m >> k) & 1u) {
            if (p < nb) bl[p] = t * 3u + (uint32_t)k;
            p++;
        }
}
// per boundary edge i of the list: its ends and component, a set of its own, and its two ends into the (component, vertex) table
__global__ void cxt_k_loop_insert(const uint32_t* __restrict__ bl, const int32_t* __restrict__ tri, const int32_t* __restrict__ tlab, uint32_t nb,
                                  uint32_t* __restrict__ ea, uint32_t* __restrict__ eb, uint32_t* __restrict__ ec, uint32_t* __restrict__ parent,
                                  u64* vkeys, uint32_t* vmin, uint32_t* vmax, uint32_t* vdeg, uint32_t vcap, uint32_t* misc) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb) return;
    const uint32_t e = bl[i], t = e / 3u, k = e - 3u * t;
    const uint32_t a = (uint32_t)tri[(size_t)t * 3 + k], b = (uint32_t)tri[(size_t)t * 3 + (k + 1u) % 3u], c = (uint32_t)tlab[t];
    ea[i] = a; eb[i] = b; ec[i] = c;
    parent[i] = i;
#pragma unroll
    for (int end = 0; end < 2; end++) {
        bool fresh;
        const uint32_t s = cxt_insert(vkeys, vcap, ((u64)c << 32) | (u64)(end ? b : a), fresh);
        if (s == CXD_NONE) { atomicOr(&misc[CXT_M_FAIL], 8u); continue; }
        atomicMin(&vmin[s], i);
        atomicMax(&vmax[s], i);
        atomicAdd(&vdeg[s], 1u);
    }
}
// every boundary edge joins the set of the smallest edge at each of its ends: all the edges of one component at one vertex end up together
__global__ void cxt_k_loop_link(const uint32_t* __restrict__ ea, const uint32_t* __restrict__ eb, const uint32_t* __restrict__ ec, uint32_t nb,
                                const u64* __restrict__ vkeys, const uint32_t* __restrict__ vmin, uint32_t vcap, uint32_t* parent) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb) return;
#pragma unroll
    for (int end = 0; end < 2; end++) {
        const uint32_t s = cxt_find(vkeys, vcap, ((u64)ec[i] << 32) | (u64)(end ? eb[i] : ea[i]));
        if (s == CXD_NONE) continue;
        const uint32_t j = vmin[s];
        if (j < nb && j != i) cxt_union(parent, i, j);
    }
}
__global__ void cxt_k_loop_roots(uint32_t* parent, uint32_t nb, uint32_t* __restrict__ root, uint32_t* __restrict__ isroot) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb) return;
    const uint32_t r = cxt_root(parent, i);
    root[i] = r;
    isroot[i] = r == i ? 1u : 0u;
}
__global__ void cxt_k_loop_init(const uint32_t* __restrict__ isroot, const uint32_t* __restrict__ lidx, const uint32_t* __restrict__ ec, uint32_t nb, uint32_t nl,
                                cx_loop* __restrict__ loops) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb || !isroot[i]) return;
    const uint32_t l = lidx[i];
    if (l >= nl) return;
    cx_loop r;
    r.component = (int32_t)ec[i]; r.simple = 1; r.first = 0; r.count = 0;
    loops[l] = r;
}
// per boundary edge: its loop, the loop's edge count, whether its ends make the loop non-simple, and where its two darts lead.  Dart
// 2i leaves the tail of edge i along it, dart 2i+1 leaves the head; a dart's successor is the dart that leaves its far end along the
// OTHER boundary edge there.  The dart that would step onto dart 2 * root (the loop's smallest edge in its own direction) ends the walk.
__global__ void cxt_k_loop_edges(const uint32_t* __restrict__ ea, const uint32_t* __restrict__ eb, const uint32_t* __restrict__ ec, const uint32_t* __restrict__ root,
                                 const uint32_t* __restrict__ lidx, uint32_t nb, uint32_t nl, const u64* __restrict__ vkeys, const uint32_t* __restrict__ vmin,
                                 const uint32_t* __restrict__ vmax, const uint32_t* __restrict__ vdeg, uint32_t vcap, uint32_t* __restrict__ eloop,
                                 uint32_t* lcount, cx_loop* loops, uint32_t* __restrict__ nxt, uint32_t* __restrict__ rnk) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb) return;
    const uint32_t r = root[i], l = r < nb ? lidx[r] : CXD_NONE;
    eloop[i] = l;
    if (l >= nl) { nxt[2 * (size_t)i] = CXT_END; nxt[2 * (size_t)i + 1] = CXT_END; rnk[2 * (size_t)i] = 0; rnk[2 * (size_t)i + 1] = 0; return; }
    atomicAdd(&lcount[l], 1u);
    const uint32_t a = ea[i], b = eb[i], c = ec[i];
    bool simple = a != b;
#pragma unroll
    for (int dir = 0; dir < 2; dir++) {
        const uint32_t far = dir ? a : b;
        const uint32_t s = cxt_find(vkeys, vcap, ((u64)c << 32) | (u64)far);
        uint32_t to = 2u * i + (uint32_t)dir;          // (to itself: a walk that gets nowhere)
        if (s == CXD_NONE || vdeg[s] != 2u) simple = false;
        else {
            const uint32_t j = vmin[s] == i ? vmax[s] : vmin[s];
            if (j < nb) to = 2u * j + (ea[j] == far ? 0u : 1u);
        }
        nxt[2 * (size_t)i + dir] = to == 2u * r ? CXT_END : to;
        rnk[2 * (size_t)i + dir] = 1u;
    }
    if (!simple) loops[l].simple = 0;                  // (every writer stores the same word)
}
__global__ void cxt_k_loop_finish(const uint32_t* __restrict__ lcount, const uint32_t* __restrict__ lfirst, uint32_t nl, uint32_t nc, cx_loop* loops,
                                  u64* __restrict__ acc, uint32_t* misc) {
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= nl) return;
    loops[l].first = lfirst[l];
    loops[l].count = lcount[l];
    const uint32_t c = (uint32_t)loops[l].component;
    if (c >= nc) return;
    atomicAdd(&acc[(size_t)c * CXT_WORDS + CXT_W_LOOPS], 1ULL);
    if (!loops[l].simple) {
        atomicAdd(&acc[(size_t)c * CXT_WORDS + CXT_W_NONSIMPLE], 1ULL);
        atomicAdd(&misc[CXT_M_NONSIMPLE], 1u);
    }
}
// one round of pointer doubling: rnk = steps from the dart to nxt (the step onto the end counts)
__global__ void cxt_k_double(const uint32_t* __restrict__ nxt_in, const uint32_t* __restrict__ rnk_in, uint32_t nd, uint32_t* __restrict__ nxt_out,
                             uint32_t* __restrict__ rnk_out) {
    const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= nd) return;
    const uint32_t n = nxt_in[d];
    if (n == CXT_END || n >= nd) { nxt_out[d] = n; rnk_out[d] = rnk_in[d]; return; }
    nxt_out[d] = nxt_in[n];
    rnk_out[d] = rnk_in[d] + rnk_in[n];
}
// a dart of a simple loop that reached the end lies on the walk: it is `rnk` steps from the end, hence at place count - rnk
__global__ void cxt_k_scatter(const uint32_t* __restrict__ nxt, const uint32_t* __restrict__ rnk, const uint32_t* __restrict__ eloop, const uint32_t* __restrict__ ea,
                              const uint32_t* __restrict__ eb, const cx_loop* __restrict__ loops, uint32_t nb, uint32_t nl, int32_t* __restrict__ lverts) {
    const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = d >> 1;
    if (i >= nb) return;
    const uint32_t l = eloop[i];
    if (l >= nl || nxt[d] != CXT_END) return;
    const cx_loop L = loops[l];
    const uint32_t steps = rnk[d];
    if (!L.simple || steps == 0u || steps > L.count) return;
    const size_t at = (size_t)L.first + (L.count - steps);
    if (at < nb) lverts[at] = (int32_t)((d & 1u) ? eb[i] : ea[i]);
}
// the edges of non-simple loops in ascending 3t+k: ONE wave goes through the list in order; the lanes of a chunk that share a loop take
// consecutive places behind the loop's cursor.  Nothing to do (and nothing read) when every loop is simple.
__global__ __launch_bounds__(64) void cxt_k_nonsimple(const uint32_t* __restrict__ eloop, const uint32_t* __restrict__ ea, const cx_loop* __restrict__ loops,
                                                      uint32_t nb, uint32_t nl, uint32_t* cursor, const uint32_t* __restrict__ misc, int32_t* __restrict__ lverts) {
    if (misc[CXT_M_NONSIMPLE] == 0u) return;
    const uint32_t lane = threadIdx.x & 63u;
    for (u64 base = 0; base < (u64)nb; base += 64ULL) {      // wave-uniform
        const u64 i = base + lane;
        uint32_t l = CXD_NONE;
        bool active = i < (u64)nb;
        if (active) { l = eloop[i]; active = l < nl && loops[l].simple == 0; }
        uint64_t rem = __ballot(active);
        while (rem != 0ULL) {
            const int leader = __ffsll((long long)rem) - 1;
            const uint32_t k = (uint32_t)__shfl((int)l, leader);
            const bool mine = active && l == k;
            const uint64_t grp = __ballot(mine);
            rem &= ~grp;
            uint32_t start = 0;
            if ((int)lane == leader) start = atomicAdd(&cursor[k], (uint32_t)__popcll(grp));
            start = (uint32_t)__shfl((int)start, leader);
            if (mine) {
                const size_t at = (size_t)loops[k].first + start + (uint32_t)__popcll(grp & ((1ULL << lane) - 1ULL));
                if (at < nb) lverts[at] = (int32_t)ea[i];
            }
        }
    }
}

// ---- records ------------------------------------------------------------------------------------------------------------------------
__global__ void cxt_k_finish(const u64* __restrict__ acc, uint32_t nc, cx_topology* __restrict__ table) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nc) return;
    const u64* w = acc + (size_t)c * CXT_WORDS;
    cx_topology r;
    r.triangles = (int64_t)w[CXT_W_F];
    r.vertices = (int64_t)w[CXT_W_V];
    r.edges = (int64_t)w[CXT_W_E];
    r.boundary_edges = (int64_t)w[CXT_W_BE];
    r.nonmanifold_edges = (int64_t)w[CXT_W_NM];
    r.euler = r.vertices - r.edges + r.triangles;
    r.boundary_loops = (int32_t)w[CXT_W_LOOPS];
    const int64_t twice = 2 - r.euler - (int64_t)r.boundary_loops;
    r.genus = (r.nonmanifold_edges == 0 && twice >= 0 && (twice & 1) == 0 && twice / 2 <= 0x7FFFFFFF) ? (int32_t)(twice / 2) : -1;
    r.nonsimple_loops = (int32_t)w[CXT_W_NONSIMPLE];
    r.reserved = 0;
    table[c] = r;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------

static int cxt_fail_check(cx_ctx* ctx, const uint32_t* h) {
    if (!h[CXT_M_FAIL]) return CX_OK;
    ctx->err = "cx_level1_topology: a key table ran full or lost a key (bits " + std::to_string(h[CXT_M_FAIL]) + ")";
    return CX_ERR_HIP;
}

// the boundary loops of the current mesh, from the boundary list of nb edges
static int cxt_loops(cx_ctx* ctx, cx_topo_state* T, const cx_level1_comp_view& V, const int32_t* tlab, uint32_t nc, uint32_t nb, uint32_t* nl_out) {
    int rc;
    hipStream_t st = ctx->stream;
    const uint32_t nt = V.nt;
    const uint32_t vcap = 4u * nb + 64u;        // at most 2 nb keys: load <= 0.5 (nb < 2^30 here)
    if ((rc = T->bl.grow(ctx, (size_t)nb + 16))) return rc;
    if ((rc = T->ea.grow(ctx, (size_t)nb + 16))) return rc;
    if ((rc = T->eb.grow(ctx, (size_t)nb + 16))) return rc;
    if ((rc = T->ec.grow(ctx, (size_t)nb + 16))) return rc;
    if ((rc = T->parent.grow(ctx, (size_t)nb + 16))) return rc;
    if ((rc = T->root.grow(ctx, (size_t)nb + 16))) return rc;
    if ((rc = T->isroot.grow(ctx, (size_t)nb + 16))) return rc;
    if ((rc = T->lidx.grow(ctx, (size_t)nb + 16))) return rc;
    if ((rc = T->eloop.grow(ctx, (size_t)nb + 16))) return rc;
    if ((rc = T->lverts.grow(ctx, (size_t)nb + 16))) return rc;
    if ((rc = T->vkeys.grow(ctx, vcap))) return rc;
    if ((rc = T->vmin.grow(ctx, vcap))) return rc;
    if ((rc = T->vmax.grow(ctx, vcap))) return rc;
    if ((rc = T->vdeg.grow(ctx, vcap))) return rc;
    for (int b = 0; b < 2; b++) {
        if ((rc = T->nxt[b].grow(ctx, 2 * (size_t)nb + 16))) return rc;
        if ((rc = T->rnk[b].grow(ctx, 2 * (size_t)nb + 16))) return rc;
    }
    CX_HIP(ctx, hipMemsetAsync(T->vkeys, 0xFF, (size_t)vcap * sizeof(u64), st));
    CX_HIP(ctx, hipMemsetAsync(T->vmin, 0xFF, (size_t)vcap * sizeof(uint32_t), st));
    CX_HIP(ctx, hipMemsetAsync(T->vmax, 0, (size_t)vcap * sizeof(uint32_t), st));
    CX_HIP(ctx, hipMemsetAsync(T->vdeg, 0, (size_t)vcap * sizeof(uint32_t), st));
    CX_HIP(ctx, hipMemsetAsync(T->lverts, 0, (size_t)nb * sizeof(int32_t), st));
    hipLaunchKernelGGL(cxt_k_compact, cx_grid1(nt), dim3(256), 0, st, T->bmask.get(), (const uint32_t*)T->bpos, nt, nb, T->bl);
    hipLaunchKernelGGL(cxt_k_loop_insert, cx_grid1(nb), dim3(256), 0, st, (const uint32_t*)T->bl, V.tri, tlab, nb, T->ea, T->eb, T->ec, T->parent,
                       T->vkeys, T->vmin, T->vmax, T->vdeg, vcap, T->misc);
    hipLaunchKernelGGL(cxt_k_loop_link, cx_grid1(nb), dim3(256), 0, st, (const uint32_t*)T->ea, (const uint32_t*)T->eb, (const uint32_t*)T->ec, nb,
                       (const u64*)T->vkeys, (const uint32_t*)T->vmin, vcap, T->parent);
    hipLaunchKernelGGL(cxt_k_loop_roots, cx_grid1(nb), dim3(256), 0, st, T->parent, nb, T->root, T->isroot);
    if ((rc = cx_scan_u32(ctx, T->isroot, T->lidx, nb, T->sums, T->misc + CXT_M_L))) return rc;
    uint32_t h[CXT_M_WORDS];
    CX_HIP(ctx, hipMemcpyAsync(h, T->misc, sizeof(h), hipMemcpyDeviceToHost, st));
    CX_HIP(ctx, hipStreamSynchronize(st));
    if ((rc = cxt_fail_check(ctx, h))) return rc;
    const uint32_t nl = h[CXT_M_L];
    if (nl == 0 || nl > nb) { ctx->err = "cx_level1_boundary_loops: the loops do not add up"; return CX_ERR_HIP; }
    if ((rc = T->loops.grow(ctx, (size_t)nl + 16))) return rc;
    if ((rc = T->lcount.grow(ctx, (size_t)nl + 16))) return rc;
    if ((rc = T->lfirst.grow(ctx, (size_t)nl + 16))) return rc;
    if ((rc = T->cursor.grow(ctx, (size_t)nl + 16))) return rc;
    CX_HIP(ctx, hipMemsetAsync(T->lcount, 0, (size_t)nl * sizeof(uint32_t), st));
    CX_HIP(ctx, hipMemsetAsync(T->cursor, 0, (size_t)nl * sizeof(uint32_t), st));
    hipLaunchKernelGGL(cxt_k_loop_init, cx_grid1(nb), dim3(256), 0, st, (const uint32_t*)T->isroot, (const uint32_t*)T->lidx, (const uint32_t*)T->ec, nb, nl, T->loops);
    hipLaunchKernelGGL(cxt_k_loop_edges, cx_grid1(nb), dim3(256), 0, st, (const uint32_t*)T->ea, (const uint32_t*)T->eb, (const uint32_t*)T->ec,
                       (const uint32_t*)T->root, (const uint32_t*)T->lidx, nb, nl, (const u64*)T->vkeys, (const uint32_t*)T->vmin, (const uint32_t*)T->vmax,
                       (const uint32_t*)T->vdeg, vcap, T->eloop, T->lcount, T->loops, T->nxt[0], T->rnk[0]);
    if ((rc = cx_scan_u32(ctx, T->lcount, T->lfirst, nl, T->sums, T->misc + CXT_M_SCRATCH))) return rc;
    hipLaunchKernelGGL(cxt_k_loop_finish, cx_grid1(nl), dim3(256), 0, st, (const uint32_t*)T->lcount, (const uint32_t*)T->lfirst, nl, nc, T->loops, T->acc, T->misc);
    // the longest walk has nb steps: after r rounds a dart has looked 2^r steps ahead
    int rounds = 0;
    while (rounds < 32 && (1ULL << rounds) < (u64)nb) rounds++;
    int cur = 0;
    for (int r = 0; r < rounds; r++, cur ^= 1)
        hipLaunchKernelGGL(cxt_k_double, cx_grid1(2 * (size_t)nb), dim3(256), 0, st, (const uint32_t*)T->nxt[cur], (const uint32_t*)T->rnk[cur], 2u * nb,
                           T->nxt[cur ^ 1], T->rnk[cur ^ 1]);
    hipLaunchKernelGGL(cxt_k_scatter, cx_grid1(2 * (size_t)nb), dim3(256), 0, st, (const uint32_t*)T->nxt[cur], (const uint32_t*)T->rnk[cur], (const uint32_t*)T->eloop,
                       (const uint32_t*)T->ea, (const uint32_t*)T->eb, (const cx_loop*)T->loops, nb, nl, T->lverts);
    hipLaunchKernelGGL(cxt_k_nonsimple, dim3(1), dim3(64), 0, st, (const uint32_t*)T->eloop, (const uint32_t*)T->ea, (const cx_loop*)T->loops, nb, nl, T->cursor,
                       (const uint32_t*)T->misc, T->lverts);
    CX_HIP(ctx, hipGetLastError());
    *nl_out = nl;
    return CX_OK;
}

// table and loops of the current mesh (cached per generation of the mesh)
static int cxt_build(cx_ctx* ctx, const char* who, cx_topo_state** Tout) {
    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_level1_comp_view V;
    const int32_t *tlab = nullptr, *vlab = nullptr;
    uint32_t nc = 0;
    int rc = cx_comp_labels_get(ctx, who, &V, &tlab, &vlab, &nc);
    if (rc) return rc;
    if (!ctx->topo) ctx->topo = new (std::nothrow) cx_topo_state();
    if (!ctx->topo) return CX_ERR_NOMEM;
    cx_topo_state* T = ctx->topo;
    *Tout = T;
    if (T->gen == V.gen) return CX_OK;
    T->gen = ~0ULL;
    const uint32_t nt = V.nt, nv = V.nv;
    if (nt >= (1u << 30)) {
        ctx->err = std::string(who) + ": " + std::to_string(nt) + " triangles; the edge table (4 slots per triangle, 32-bit slot numbers and 3t+k) takes fewer than 2^30";
        return CX_ERR_UNSUPPORTED;
    }
    uint32_t nb = 0, nl = 0;
    if (nt && nc) {
        hipStream_t st = ctx->stream;
        // 3 nt keys at most (a mesh without a shared edge); a closed mesh has 1.5 nt: load 0.375 there, 0.75 at worst
        const uint32_t cap = 4u * nt + 64u;
        if ((rc = T->misc.grow(ctx, CXT_M_WORDS))) return rc;
        if ((rc = T->ekeys.grow(ctx, cap))) return rc;
        if ((rc = T->ecnt.grow(ctx, cap))) return rc;
        if ((rc = T->erep.grow(ctx, cap))) return rc;
        if ((rc = T->bmask.grow(ctx, (size_t)nt + 16))) return rc;
        if ((rc = T->bcnt.grow(ctx, (size_t)nt + 16))) return rc;
        if ((rc = T->bpos.grow(ctx, (size_t)nt + 16))) return rc;
        if ((rc = T->sums.grow(ctx, 3 * (size_t)nt / 1024 + 16))) return rc;
        if ((rc = T->acc.grow(ctx, (size_t)nc * CXT_WORDS + 16))) return rc;
        if ((rc = T->table.grow(ctx, (size_t)nc + 1))) return rc;
        CX_HIP(ctx, hipMemsetAsync(T->misc, 0, CXT_M_WORDS * sizeof(uint32_t), st));
        CX_HIP(ctx, hipMemsetAsync(T->ekeys, 0xFF, (size_t)cap * sizeof(u64), st));
        CX_HIP(ctx, hipMemsetAsync(T->ecnt, 0, (size_t)cap * sizeof(uint32_t), st));
        CX_HIP(ctx, hipMemsetAsync(T->acc, 0, (size_t)nc * CXT_WORDS * sizeof(u64), st));
        hipLaunchKernelGGL(cxt_k_edges_insert, cx_grid1(nt), dim3(256), 0, st, V.tri, tlab, vlab, nt, nv, T->ekeys, T->ecnt, T->erep, cap, T->misc);
        hipLaunchKernelGGL(cxt_k_edges_count, cx_grid1(nt), dim3(256), 0, st, V.tri, tlab, nt, nv, nc, (const u64*)T->ekeys, (const uint32_t*)T->ecnt,
                           (const uint32_t*)T->erep, cap, T->bmask, T->bcnt, T->acc, T->misc);
        hipLaunchKernelGGL(cxt_k_vertices, cx_grid1(nv), dim3(256), 0, st, vlab, nv, nc, T->acc);
        if ((rc = cx_scan_u32(ctx, T->bcnt, T->bpos, nt, T->sums, T->misc + CXT_M_B))) return rc;
        uint32_t h[CXT_M_WORDS];
        CX_HIP(ctx, hipMemcpyAsync(h, T->misc, sizeof(h), hipMemcpyDeviceToHost, st));
        CX_HIP(ctx, hipStreamSynchronize(st));
        if ((rc = cxt_fail_check(ctx, h))) return rc;
        nb = h[CXT_M_B];
        if (nb > 3u * nt) { ctx->err = std::string(who) + ": the boundary edges do not add up"; return CX_ERR_HIP; }
        const uint32_t shared = h[CXT_M_MISMATCH];
        if (shared) {
            const uint32_t mcap = 2u * std::min(shared, 3u * nt) + 64u;
            if ((rc = T->mkeys.grow(ctx, mcap))) return rc;
            CX_HIP(ctx, hipMemsetAsync(T->mkeys, 0xFF, (size_t)mcap * sizeof(u64), st));
            hipLaunchKernelGGL(cxt_k_vertices_shared, cx_grid1(nt), dim3(256), 0, st, V.tri, tlab, vlab, nt, nv, nc, T->mkeys, mcap, T->acc, T->misc);
        }
        if (nb >= (1u << 30)) {
            ctx->err = std::string(who) + ": " + std::to_string(nb) + " boundary edges; the loops (two darts per edge, 4 table slots per edge) take fewer than 2^30";
            return CX_ERR_UNSUPPORTED;
        }
        if (nb && (rc = cxt_loops(ctx, T, V, tlab, nc, nb, &nl))) return rc;
        hipLaunchKernelGGL(cxt_k_finish, cx_grid1(nc), dim3(256), 0, st, (const u64*)T->acc, nc, T->table);
        CX_HIP(ctx, hipMemcpyAsync(h, T->misc, sizeof(h), hipMemcpyDeviceToHost, st));
        CX_HIP(ctx, hipStreamSynchronize(st));
        CX_HIP(ctx, hipGetLastError());
        if ((rc = cxt_fail_check(ctx, h))) return rc;
    }
    T->nc = (nt && nc) ? nc : 0; T->nb = nb; T->nl = nl;
    T->gen = V.gen;
    return CX_OK;
}

extern "C" int cx_level1_topology(cx_ctx* ctx, int64_t* n_components, void** table_dev) {
    if (!ctx) return CX_ERR_INVALID;
    cx_topo_state* T = nullptr;
    const int rc = cxt_build(ctx, "cx_level1_topology", &T);
    if (rc) return rc;
    if (n_components) *n_components = (int64_t)T->nc;
    if (table_dev) *table_dev = T->nc ? (void*)T->table.get() : nullptr;
    return CX_OK;
}

extern "C" int cx_level1_topology_download(cx_ctx* ctx, cx_topology* out) {
    if (!ctx) return CX_ERR_INVALID;
    cx_topo_state* T = nullptr;
    const int rc = cxt_build(ctx, "cx_level1_topology_download", &T);
    if (rc || !T->nc) return rc;
    if (!out) return CX_ERR_INVALID;
    return cx_copy_to_host1(ctx, out, T->table, (size_t)T->nc * sizeof(cx_topology));
}

extern "C" int cx_level1_boundary_loops(cx_ctx* ctx, int64_t* n_loops, int64_t* n_boundary_edges, void** loops_dev, void** vertices_dev) {
    if (!ctx) return CX_ERR_INVALID;
    cx_topo_state* T = nullptr;
    const int rc = cxt_build(ctx, "cx_level1_boundary_loops", &T);
    if (rc) return rc;
    if (n_loops) *n_loops = (int64_t)T->nl;
    if (n_boundary_edges) *n_boundary_edges = (int64_t)T->nb;
    if (loops_dev) *loops_dev = T->nl ? (void*)T->loops.get() : nullptr;
    if (vertices_dev) *vertices_dev = T->nb ? (void*)T->lverts.get() : nullptr;
    return CX_OK;
}

extern "C" int cx_level1_boundary_loops_download(cx_ctx* ctx, cx_loop* loops, int32_t* vertices) {
    if (!ctx) return CX_ERR_INVALID;
    cx_topo_state* T = nullptr;
    int rc = cxt_build(ctx, "cx_level1_boundary_loops_download", &T);
    if (rc) return rc;
    if (loops && T->nl && (rc = cx_copy_to_host1(ctx, loops, T->loops, (size_t)T->nl * sizeof(cx_loop)))) return rc;
    if (vertices && T->nb && (rc = cx_copy_to_host1(ctx, vertices, T->lverts, (size_t)T->nb * sizeof(int32_t)))) return rc;
    return CX_OK;
}
