// cx_dev.h -- the device primitives that more than one translation unit needs, each defined once.
// Only __device__ __forceinline__ functions, typedefs and constants; a primitive that a second file needs moves here instead of
// being copied.
#pragma once
#include "cx_common.h"

typedef unsigned long long u64;
#define CXD_EMPTY 0xFFFFFFFFFFFFFFFFULL   // a free slot of a table of 64-bit keys
#define CXD_NONE 0xFFFFFFFFu              // no index

// 64-bit mixer (the finaliser of MurmurHash3): what every hash table here derives its home slot from
__device__ __forceinline__ u64 cxd_mix(u64 x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL;
    x ^= x >> 33;
    return x;
}
// total order on doubles as unsigned integers, and back
__device__ __forceinline__ u64 cxd_orderable(double x) {
    const u64 b = (u64)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}
__device__ __forceinline__ double cxd_from_orderable(u64 o) {
    const u64 b = (o >> 63) ? (o & 0x7FFFFFFFFFFFFFFFULL) : ~o;
    return __longlong_as_double((long long)b);
}

// The same for the floats of 32 and 16 bits, NaN included: -inf < negative < -0.0 < +0.0 < positive < +inf < every NaN (one key, all
// ones).  Unlike the keys of cx_pick.hip, which fold -0.0 onto +0.0, these have an inverse: a rank filter hands a sample back.
// `inf`: the bits of +infinity (0x7C00 half, 0x7F80 bfloat16); `qnan`: the canonical quiet NaN the NaN key stands for
__device__ __forceinline__ uint32_t cxd_orderable32(uint32_t u) {
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint32_t cxd_from_orderable32(uint32_t k) {
    if (k == 0xFFFFFFFFu) return 0x7FC00000u;
    return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
}
__device__ __forceinline__ uint32_t cxd_orderable16(uint32_t u, uint32_t inf) {
    if ((u & 0x7FFFu) > inf) return 0xFFFFu;
    return (u & 0x8000u) ? (~u & 0xFFFFu) : (u | 0x8000u);
}
__device__ __forceinline__ uint32_t cxd_from_orderable16(uint32_t k, uint32_t qnan) {
    if (k == 0xFFFFu) return qnan;
    return (k & 0x8000u) ? (k ^ 0x8000u) : (~k & 0xFFFFu);
}

// the key of a sample of any CX_DTYPE_* (its bits, zero-extended) in the key's own width, and back (cx_rank.hip, cx_recon.hip):
// integers by value with the sign bit flipped, floats by the functions above
__device__ __forceinline__ uint32_t cxd_sample_key(int32_t dtype, uint32_t raw) {
    switch (dtype) {
        case CX_DTYPE_U8: case CX_DTYPE_U16: return raw;
        case CX_DTYPE_I8: return raw ^ 0x80u;
        case CX_DTYPE_I16: return raw ^ 0x8000u;
        case CX_DTYPE_F16: return cxd_orderable16(raw, 0x7C00u);
        case CX_DTYPE_BF16: return cxd_orderable16(raw, 0x7F80u);
        default: return cxd_orderable32(raw);
    }
}
__device__ __forceinline__ uint32_t cxd_sample_unkey(int32_t dtype, uint32_t key) {
    switch (dtype) {
        case CX_DTYPE_U8: case CX_DTYPE_U16: return key;
        case CX_DTYPE_I8: return key ^ 0x80u;
        case CX_DTYPE_I16: return key ^ 0x8000u;
        case CX_DTYPE_F16: return cxd_from_orderable16(key, 0x7E00u);
        case CX_DTYPE_BF16: return cxd_from_orderable16(key, 0x7FC0u);
        default: return cxd_from_orderable32(key);
    }
}

// the boundary rule of the grid calls (cx_grid_resample3d, cx_grid_rank3d): the index read for j on an axis of n samples, -1 for cval
__device__ __forceinline__ int32_t cxd_boundary_src(int64_t j, int64_t n, int32_t mode) {
    if (j >= 0 && j < n) return (int32_t)j;
    if (mode == CX_FILTER_CONSTANT) return -1;
    if (mode == CX_FILTER_NEAREST) return j < 0 ? 0 : (int32_t)(n - 1);
    int64_t p = j % (2 * n);
    if (p < 0) p += 2 * n;
    return (int32_t)(p < n ? p : 2 * n - 1 - p);
}

// monotonic maximum / minimum with a plain read first: once the running extreme is established almost every caller
// sees that its value cannot move it and skips the atomic (same-address atomics serialise at ~88/us)
__device__ __forceinline__ void cxd_max64(u64* addr, u64 v) {
    if (__hip_atomic_load(addr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= v) return;
    atomicMax(addr, v);
}
__device__ __forceinline__ void cxd_min64(u64* addr, u64 v) {
    if (__hip_atomic_load(addr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= v) return;
    atomicMin(addr, v);
}
__device__ __forceinline__ void cxd_max32(uint32_t* addr, uint32_t v) {
    if (__hip_atomic_load(addr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= v) return;
    atomicMax(addr, v);
}

// butterflies over the 64 lanes of the wave: every lane ends with the result
__device__ __forceinline__ u64 cxd_shfl_xor64(u64 v, int o) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ uint32_t cxd_wave_add(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}
__device__ __forceinline__ long long cxd_wave_add(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (long long)cxd_shfl_xor64((u64)v, o);
    return v;
}
__device__ __forceinline__ u64 cxd_wave_xor(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v ^= cxd_shfl_xor64(v, o);
    return v;
}
__device__ __forceinline__ u64 cxd_wave_min(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u64 w = cxd_shfl_xor64(v, o); v = w < v ? w : v; }
    return v;
}
__device__ __forceinline__ u64 cxd_wave_max(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u64 w = cxd_shfl_xor64(v, o); v = w > v ? w : v; }
    return v;
}

// signed 64-bit value into a 128-bit two's complement accumulator {low, high}: the carry out of the low word follows from the value
// the atomic returns, so the sum is exact modulo 2^128 in any order
__device__ __forceinline__ void cxd_add128(u64* w, long long v) {
    if (v == 0) return;
    const u64 lo = (u64)v;
    u64 hi = v < 0 ? ~0ULL : 0ULL;
    const u64 old = atomicAdd(&w[0], lo);
    if (old + lo < old) hi += 1ULL;
    if (hi) atomicAdd(&w[1], hi);
}
// the 128-bit sum as a double, rounded once (the top 64 bits with a sticky bit), times 2^-q
__device__ __forceinline__ double cxd_to_double128(u64 lo, u64 hi, int q) {
    const bool neg = (hi >> 63) != 0ULL;
    if (neg) { lo = ~lo + 1ULL; hi = ~hi + (lo == 0ULL ? 1ULL : 0ULL); }
    double r;
    if (hi == 0ULL) r = ldexp((double)lo, -q);
    else {
        const int s = __clzll((long long)hi);
        u64 top = s ? ((hi << s) | (lo >> (64 - s))) : hi;
        const u64 rest = s ? (lo << s) : lo;
        if (rest) top |= 1ULL;
        r = ldexp((double)top, 64 - s - q);
    }
    return neg ? -r : r;
}

// ---- lock-free union-find -------------------------------------------------------------------------------------------------------------
// The rule for EVERY union-find in global memory here, whatever the width of its parent words (uint32_t below; the u64 words of
// cxp_find / cxp_union and cxp_find0 / cxp_union0 further down; cxt_root / cxt_union in cx_topo.hip): every access to a parent word
// inside the kernel that unites is a device-scope atomic, loads and path-shortening writes included.  The L2s of the 8 XCDs are not
// coherent with each other inside a kernel, and a version with plain loads and plain path-halving stores showed a rare wrong winding
// of one component (stale lines mixing with memory-side compare-and-swaps).
//
// Parents are ids, a root points to itself, the root of a set is its smallest id.  Path halving: on the way up a node is pointed at
// its grandparent by compare-and-swap, so a word only ever moves to an ancestor.
__device__ __forceinline__ uint32_t cxd_uf_find(uint32_t* parent, uint32_t x) {
    for (;;) {
        const uint32_t p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        const uint32_t g = __hip_atomic_load(&parent[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (g != p) atomicCAS(&parent[x], p, g);
        x = p;
    }
}
__device__ __forceinline__ void cxd_uf_union(uint32_t* parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = cxd_uf_find(parent, a);
        b = cxd_uf_find(parent, b);
        if (a == b) return;
        const uint32_t win = min(a, b), lose = max(a, b);
        if (atomicCAS(&parent[lose], lose, win) == lose) return;
    }
}
// find in a forest that one workgroup keeps in LDS (the block-local step of cx_seed.hip and cx_seed4.hip): its words are the
// workgroup's own, so plain loads see what the compare-and-swaps wrote
__device__ __forceinline__ uint32_t cxd_uf_find_lds(uint32_t* lp, uint32_t x) {
    for (;;) {
        const uint32_t p = lp[x];
        if (p == x) return x;
        const uint32_t g = lp[p];
        if (g != p) atomicCAS(&lp[x], p, g);
        x = p;
    }
}

// ---- the post-pass files' primitives (cx_post.hip, cx_post4d.hip, cx_morph.hip): a wave-wide maximum, union-find over u64 parent words,
// the slot of an edge in the edge tables.  They keep the prefix they had in cx_post.hip ----------------------------------------------
// monotonic maximum (cxd_max64) for a whole wave: when all its lanes share one key (component) they reduce among themselves and issue
// ONE atomic; a wave that straddles components falls back to one call per lane.  (With values that grow along
// the array -- vertices ordered by x -- the plain read alone does not help: every caller raises the maximum.)
// All lanes of the wave must call it; `active` masks the idle ones.
__device__ __forceinline__ void cxp_wave_max64(u64* table, uint32_t key, u64 v, bool active) {
    const uint64_t act = __ballot(active);
    if (act == 0ULL) return;
    const uint32_t k = (uint32_t)__shfl((int)key, __ffsll((long long)act) - 1);
    if (__ballot(active && key != k) != 0ULL) {   // wave-uniform
        if (active) cxd_max64(&table[key], v);
        return;
    }
    u64 m = active ? v : 0ULL;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)m, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(m >> 32), o);
        const u64 other = ((u64)hi << 32) | lo;
        m = other > m ? other : m;
    }
    if ((threadIdx.x & 63u) == 0u) cxd_max64(&table[k], m);
}

// union-find over 32-bit ids; parent word = (parity << 32) | parent id.  Root = smallest priority.
__device__ __forceinline__ uint32_t cxp_find(const u64* parent, uint32_t x, uint32_t& parity) {
    uint32_t par = 0;
    for (;;) {
        const u64 w = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t p = (uint32_t)w;
        if (p == x) break;
        par ^= (uint32_t)(w >> 32) & 1u;
        x = p;
    }
    parity = par;
    return x;
}
// link the sets of a and b; rel = parity between a and b (0: same winding class).
// Every access to the parent words is a device-scope atomic, loads included (why: cx_dev.h, above cxd_uf_find).
__device__ __forceinline__ void cxp_union(u64* parent, const uint32_t* prio, uint32_t a, uint32_t b, uint32_t rel) {
    for (;;) {
        uint32_t pa, pb;
        uint32_t ra = cxp_find(parent, a, pa), rb = cxp_find(parent, b, pb);
        if (ra == rb) return;
        const uint32_t ka = prio ? prio[ra] : ra, kb = prio ? prio[rb] : rb;
        const bool a_wins = (ka < kb) || (ka == kb && ra < rb);
        const uint32_t win = a_wins ? ra : rb, lose = a_wins ? rb : ra;
        const u64 expect = (u64)lose;                                  // still a root, parity 0
        const u64 desired = ((u64)((pa ^ pb ^ rel) & 1u) << 32) | (u64)win;
        if (atomicCAS(&parent[lose], expect, desired) == expect) return;
    }
}

// The same for forests without parities and priorities (connectivity only: the march's own meshes), with path HALVING: on the way
// up every node is pointed at its grandparent -- with a device-scope store, which is executed where the compare-and-swaps are, so
// the two cannot disagree (cx_dev.h, above cxd_uf_find) -- and only ever at an ancestor.  Most unions of a large component find both sides in one
// tree already; without the halving each of them walks the whole chain again (roots are the smallest ids, not the flattest trees).
__device__ __forceinline__ uint32_t cxp_find0(u64* parent, uint32_t x) {
    for (;;) {
        const uint32_t p = (uint32_t)__hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        const uint32_t g = (uint32_t)__hip_atomic_load(&parent[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (g == p) return p;
        __hip_atomic_store(&parent[x], (u64)g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = g;
    }
}
__device__ __forceinline__ void cxp_union0(u64* parent, uint32_t a, uint32_t b) {
    for (;;) {
        const uint32_t ra = cxp_find0(parent, a), rb = cxp_find0(parent, b);
        if (ra == rb) return;
        const uint32_t win = min(ra, rb), lose = max(ra, rb);
        if (atomicCAS(&parent[lose], (u64)lose, (u64)win) == (u64)lose) return;
        a = ra; b = rb;       // somebody else moved the loser: go on from the roots seen so far
    }
}

// edge table: slot s = (key at tab[2s], first triangle at tab[2s+1]) -- one cache line per probe.
// Slots are placed by the SMALLER vertex id (lo * mult + a few bits of the larger one): vertex ids follow the
// order of the march, so the triangles of a wave probe neighbouring lines instead of random ones.
// Device-scope atomics are executed at the memory side of the fabric (64 bytes of write traffic each, ~21 G/s for
// the whole chip: PMC TCC_ATOMIC / WRITE_SIZE), so they are what this stage is bound by: ONE read-modify-write per
// edge visit claims the key, the claimant publishes its triangle with a plain store (kernel 1); after the kernel
// boundary every other visitor finds the slot again with plain loads and links itself to the claimant (kernel 2).
// (mult == 0: plain hashing -- the small first table of cxp_k_edges_block, where the edges that arrive are the ones around merged
// vertices, clustered in space: rows per vertex ran into each other there, chains of hundreds of probes)
__device__ __forceinline__ u64 cxp_edge_slot(uint32_t lo, uint32_t hi, u64 mask, u64 mult) {
    if (mult == 0) return cxd_mix(((u64)lo << 32) | (u64)hi) & mask;
    return ((u64)lo * mult + (cxd_mix((u64)hi) % mult)) & mask;
}
