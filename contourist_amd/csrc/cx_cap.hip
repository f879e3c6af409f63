// cx_cap.hip -- caps of the isosurface where the rim of the array cuts it open (include/contourist_hip.h, section "rim caps").
//
// The six faces of the array are lattice planes, and the Kuhn tetrahedra cut each of them into the same two triangles per unit square
// (diagonal from the square's lower corner: direction 3 on an i-face, 5 on a j-face, 6 on a k-face).  The cross-section of the solid with
// a face is marching triangles on that face: its crossings ARE the Level-0 vertices of those lattice edges (found by edge id), its other
// corners are lattice points (key = linear index << 3 | 0).
//   cxc_k_signs<DT, AXIS>  the inside bit of every point of the two faces of one axis, one 64-bit word per wave (ballot).  i-faces are
//                          planes and j-faces rows of contiguous samples; on the k-faces a lane reads BOTH ends of its row, so the two
//                          lines a row touches are requested together
//   cxc_k_rim_count        one lane per Level-0 vertex record: does its lattice edge lie in a selected face?  (ballot, one atomic per wave)
//   cxc_k_rim_insert       those records into an open-addressing table {edge id -> vertex index} sized by that count
//   cxc_k_cases            one lane per face-triangle: three bit lookups -> the inside mask and the number of cap triangles; marks, in one
//                          byte per RIM point (a compact enumeration of the array's surface in ascending linear index), bit 0 = its
//                          lattice-point vertex is used, bit d = the crossing of its edge in direction d is used and the march has not emitted it
//   cxc_k_rim_counts       one lane per rim point: the bits of its byte (cx_scan_u32 turns them into the cap vertices' ranks: ascending key)
//   cxc_k_keys             one lane per rim point: the records {key, t = 0} of its cap vertices
//   cxc_k_emit             one lane per face-triangle: 0 / 1 / 2 triangles at their offsets
// Integer atomics only (compare-and-swap, or, add), no LDS: nothing depends on the order the lanes arrive in.
// The vertex records of the march are NOT ascending in edge id (waves and tiles finish in any order), hence a table and no binary search.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>

#include "cx_ctx.h"
#include "cx_dev.h"

#define CXC_BELOW 1u

// what the kernels know of the array and the request
struct cxc_geom {
    uint32_t n0, n1, n2, plane;
    uint32_t ring;          // rim points of a plane 0 < i < n0 - 1: its first and last row and the two ends of the rows between
    uint32_t faces;         // the 6-bit mask
    uint32_t reversed;      // bit f: the triangles of face f are emitted with their last two corners exchanged
    uint32_t item0[7];      // first face-triangle of every face (a face that is not selected has none); [6] all of them
    uint32_t word0[6];      // first sign word of every face
    cx_fdiv dsq[3];         // per axis: / squares per row of its faces
    cx_fdiv dplane, drow, dring;
};

struct cx_cap_state {
    cx_buf<u64> bits;              // inside words of the six faces
    cx_buf<u64> table;             // (edge id << 32) | Level-0 vertex index of the rim's crossings
    cx_buf<uint32_t> rmask;        // one byte per rim point, four to a word
    cx_buf<uint32_t> rcount, rbase;// per rim point: its cap vertices, and the first of them
    cx_buf<uint8_t> tcase;         // per face-triangle: the inside mask of its corners
    cx_buf<uint32_t> tcount, toff; // per face-triangle: its cap triangles, and the first of them
    cx_buf<uint32_t> sums, misc;   // scan scratch; [0] rim records [1] cap vertices [2] cap triangles [3] lattice-point vertices [4] missing crossings
    cx_buf<cx_vrec> vrec;          // the cap vertices {key, 0}: what the post-pass's vertex kernel reads
    cx_buf<uint32_t> keys;         // their keys alone: what cx_cap3d_download copies
    cx_buf<int32_t> tris;          // the cap triangles
    // the cap these hold: of which request (valid while ctx->cap_valid)
    uint32_t faces = 0, flags = 0;
    uint32_t nv0 = 0, nt0 = 0;     // the Level-0 mesh it continues
    uint32_t ncv = 0, nct = 0;
    int64_t counts[4] = {0, 0, 0, 0};
    hipEvent_t ev[2] = {nullptr, nullptr};
    double info[4] = {0, 0, 0, 0};
};

void cx_cap_free(cx_ctx* ctx) {
    cx_cap_state* Z = ctx->cap;
    if (!Z) return;
    for (int i = 0; i < 2; i++)
        if (Z->ev[i]) (void)hipEventDestroy(Z->ev[i]);
    delete Z;
    ctx->cap = nullptr;
    ctx->cap_valid = false;
}

// ---- device -------------------------------------------------------------------------------------------------------------------------
// the rim points in ascending linear index: plane 0 whole, of every plane between its first row, the two ends of its middle rows and
// its last row, plane n0 - 1 whole
__device__ __forceinline__ uint32_t cxc_rim(const cxc_geom& G, uint32_t i, uint32_t j, uint32_t k) {
    if (i == 0u) return j * G.n2 + k;
    if (i == G.n0 - 1u) return G.plane + (G.n0 - 2u) * G.ring + j * G.n2 + k;
    const uint32_t base = G.plane + (i - 1u) * G.ring;
    if (j == 0u) return base + k;
    if (j == G.n1 - 1u) return base + G.n2 + 2u * (G.n1 - 2u) + k;
    return base + G.n2 + 2u * (j - 1u) + (k ? 1u : 0u);
}
__device__ __forceinline__ uint32_t cxc_rim_lin(const cxc_geom& G, uint32_t r) {
    if (r < G.plane) return r;
    const uint32_t last = G.plane + (G.n0 - 2u) * G.ring;
    if (r >= last) return (G.n0 - 1u) * G.plane + (r - last);
    const uint32_t q = r - G.plane, ii = cx_div(q, G.dring), x = q - ii * G.ring;
    uint32_t j, k;
    if (x < G.n2) { j = 0u; k = x; }
    else if (x >= G.n2 + 2u * (G.n1 - 2u)) { j = G.n1 - 1u; k = x - G.n2 - 2u * (G.n1 - 2u); }
    else { const uint32_t y = x - G.n2; j = (y >> 1) + 1u; k = (y & 1u) ? G.n2 - 1u : 0u; }
    return (ii + 1u) * G.plane + j * G.n2 + k;
}
// (the arrays of cxc_geom and of a face-triangle are only ever indexed by compile-time constants: a run-time index would put them in
// scratch memory; what a run-time number picks goes through these selects)
__device__ __forceinline__ uint32_t cxc_sel6(const uint32_t (&a)[6], uint32_t f) {
    return f == 0u ? a[0] : (f == 1u ? a[1] : (f == 2u ? a[2] : (f == 3u ? a[3] : (f == 4u ? a[4] : a[5]))));
}
__device__ __forceinline__ uint32_t cxc_sel3(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t i) { return i == 0u ? x0 : (i == 1u ? x1 : x2); }
// a face-triangle: its face, its three corners (numbered counter-clockwise in the face's (u, w) plane: triangle 0 of the square at
// (a, b) is (a, b), (a+1, b), (a+1, b+1), triangle 1 is (a, b), (a+1, b+1), (a, b+1)) as rim points, their inside bits, and its three
// lattice edges (edge c joins corners c and (c+1) % 3): the id, and the rim point that owns it -- the end with the smaller linear index
struct cxc_tri {
    uint32_t face;
    uint32_t in;         // bit c: corner c is inside
    uint32_t rim[3];
    uint32_t ekey[3], eown[3];
};
__device__ __forceinline__ cxc_tri cxc_triangle(const cxc_geom& G, const u64* __restrict__ bits, uint32_t e) {
    cxc_tri T;
    // (item0 ascends; empty faces repeat their successor's)
    const uint32_t f = (e >= G.item0[1] ? 1u : 0u) + (e >= G.item0[2] ? 1u : 0u) + (e >= G.item0[3] ? 1u : 0u) + (e >= G.item0[4] ? 1u : 0u) + (e >= G.item0[5] ? 1u : 0u);
    const uint32_t first[6] = {G.item0[0], G.item0[1], G.item0[2], G.item0[3], G.item0[4], G.item0[5]};
    T.face = f;
    const uint32_t axis = f >> 1, local = e - cxc_sel6(first, f), tri = local & 1u, s = local >> 1;
    const uint32_t nw = axis == 2u ? G.n1 : G.n2;
    const uint32_t a = axis == 2u ? cx_div(s, G.dsq[2]) : cx_div(s, G.dsq[0]), b = s - a * (nw - 1u);      // (dsq[0] == dsq[1]: both / (n2 - 1))
    const uint32_t fixed = (f & 1u) ? (axis == 0u ? G.n0 : (axis == 1u ? G.n1 : G.n2)) - 1u : 0u;
    const uint32_t ca[3] = {a, a + 1u, a + 1u - tri}, cb[3] = {b, b + tri, b + 1u};
    const u64* __restrict__ W = bits + cxc_sel6(G.word0, f);
    uint32_t lin[3], p[3][3];
    T.in = 0u;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        p[c][0] = axis == 0u ? fixed : ca[c];
        p[c][1] = axis == 1u ? fixed : (axis == 0u ? ca[c] : cb[c]);
        p[c][2] = axis == 2u ? fixed : cb[c];
        lin[c] = p[c][0] * G.plane + p[c][1] * G.n2 + p[c][2];
        T.rim[c] = cxc_rim(G, p[c][0], p[c][1], p[c][2]);
        const uint32_t bit = ca[c] * nw + cb[c];
        T.in |= (uint32_t)((W[bit >> 6] >> (bit & 63u)) & 1ULL) << c;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int c1 = (c + 1) % 3;
        // (along an edge of a face-triangle no coordinate descends: each differs by 0 or 1)
        const uint32_t d = ((p[c][0] != p[c1][0]) ? 4u : 0u) | ((p[c][1] != p[c1][1]) ? 2u : 0u) | ((p[c][2] != p[c1][2]) ? 1u : 0u);
        T.ekey[c] = (min(lin[c], lin[c1]) << 3) | d;
        T.eown[c] = lin[c] < lin[c1] ? T.rim[c] : T.rim[c1];
    }
    return T;
}
// the Level-0 vertex on a rim edge, or CXD_NONE where the march has emitted none
__device__ __forceinline__ uint32_t cxc_find(const u64* __restrict__ table, u64 mask, uint32_t key) {
    u64 s = cxd_mix((u64)key) & mask;
    for (;;) {
        const u64 cur = table[s];
        if (cur == CXD_EMPTY) return CXD_NONE;
        if ((uint32_t)(cur >> 32) == key) return (uint32_t)cur;
        s = (s + 1) & mask;
    }
}

// One lane per point of a face of axis AXIS, both faces of the axis in one pass.
template <int DT, int AXIS>
__global__ __launch_bounds__(256) void cxc_k_signs(const cx_grid_ref A, cxc_geom G, float vcmp, int below, u64* __restrict__ bits) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t npts = AXIS == 0 ? G.plane : (AXIS == 1 ? G.n0 * G.n2 : G.n0 * G.n1);
    bool in0 = false, in1 = false;
    if (t < npts) {
        size_t l0, l1;
        if (AXIS == 0) { l0 = t; l1 = (size_t)(G.n0 - 1u) * G.plane + t; }
        else if (AXIS == 1) {
            const uint32_t i = cx_div(t, G.drow), k = t - i * G.n2;
            l0 = (size_t)i * G.plane + k; l1 = l0 + (size_t)(G.n1 - 1u) * G.n2;
        } else { l0 = (size_t)t * G.n2; l1 = l0 + (G.n2 - 1u); }       // (t = i * n1 + j: the row's first and last sample)
        const bool low0 = cx_sample<DT>(A, l0) < vcmp, low1 = cx_sample<DT>(A, l1) < vcmp;
        in0 = below ? low0 : !low0;
        in1 = below ? low1 : !low1;
    }
    const u64 m0 = __ballot(in0), m1 = __ballot(in1);
    if ((threadIdx.x & 63u) == 0u) {
        bits[G.word0[2 * AXIS] + (t >> 6)] = m0;
        bits[G.word0[2 * AXIS + 1] + (t >> 6)] = m1;
    }
}
// the lattice edge of a vertex record lies in a selected face
__device__ __forceinline__ bool cxc_on_rim(const cxc_geom& G, uint32_t key) {
    const uint32_t lin = key >> 3, d = key & 7u;
    const uint32_t i = cx_div(lin, G.dplane), r = lin - i * G.plane, j = cx_div(r, G.drow), k = r - j * G.n2;
    uint32_t on = 0u;
    if (!(d & 4u)) on |= (i == 0u ? 1u : 0u) | (i == G.n0 - 1u ? 2u : 0u);
    if (!(d & 2u)) on |= (j == 0u ? 4u : 0u) | (j == G.n1 - 1u ? 8u : 0u);
    if (!(d & 1u)) on |= (k == 0u ? 16u : 0u) | (k == G.n2 - 1u ? 32u : 0u);
    return (on & G.faces) != 0u;
}
__global__ __launch_bounds__(256) void cxc_k_rim_count(const cx_vrec* __restrict__ verts, uint32_t nv, cxc_geom G, uint32_t* count) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    const u64 m = __ballot(v < nv && cxc_on_rim(G, verts[v].x));
    if ((threadIdx.x & 63u) == 0u && m) atomicAdd(count, (uint32_t)__popcll(m));
}
__global__ void cxc_k_table_init(u64* __restrict__ table, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) table[i] = CXD_EMPTY;
}
// (an edge id occurs once among the records: a slot is claimed whole, key and index in one compare-and-swap)
__global__ __launch_bounds__(256) void cxc_k_rim_insert(const cx_vrec* __restrict__ verts, uint32_t nv, cxc_geom G, u64* table, u64 mask) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const uint32_t key = verts[v].x;
    if (!cxc_on_rim(G, key)) return;
    const u64 word = ((u64)key << 32) | (u64)v;
    u64 s = cxd_mix((u64)key) & mask;
    while (atomicCAS(&table[s], CXD_EMPTY, word) != CXD_EMPTY) s = (s + 1) & mask;
}
// One lane per face-triangle.
__global__ __launch_bounds__(256) void cxc_k_cases(cxc_geom G, const u64* __restrict__ bits, const u64* __restrict__ table, u64 mask, uint8_t* __restrict__ tcase,
                                                   uint32_t* __restrict__ tcount, uint32_t* rmask) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= G.item0[6]) return;
    const cxc_tri T = cxc_triangle(G, bits, e);
    const uint32_t m = (uint32_t)__popc(T.in);
    tcase[e] = (uint8_t)T.in;
    tcount[e] = m == 2u ? 2u : (m ? 1u : 0u);
    if (!m) return;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int c1 = (c + 1) % 3;
        if ((T.in >> c) & 1u) atomicOr(&rmask[T.rim[c] >> 2], 1u << (8u * (T.rim[c] & 3u)));
        if ((((T.in >> c) ^ (T.in >> c1)) & 1u) && cxc_find(table, mask, T.ekey[c]) == CXD_NONE)
            atomicOr(&rmask[T.eown[c] >> 2], (1u << (T.ekey[c] & 7u)) << (8u * (T.eown[c] & 3u)));
    }
}
__global__ __launch_bounds__(256) void cxc_k_rim_counts(const uint32_t* __restrict__ rmask, uint32_t nrim, uint32_t* __restrict__ rcount, uint32_t* counters) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t b = 0u;
    if (r < nrim) {
        b = (rmask[r >> 2] >> (8u * (r & 3u))) & 0xFFu;
        rcount[r] = (uint32_t)__popc(b);
    }
    const u64 ml = __ballot(b & 1u);
    const uint32_t miss = cxd_wave_add((uint32_t)__popc(b & 0xFEu));
    if ((threadIdx.x & 63u) == 0u) {
        if (ml) atomicAdd(counters + 3, (uint32_t)__popcll(ml));
        if (miss) atomicAdd(counters + 4, miss);
    }
}
__global__ __launch_bounds__(256) void cxc_k_keys(cxc_geom G, const uint32_t* __restrict__ rmask, const uint32_t* __restrict__ rbase, uint32_t nrim,
                                                  cx_vrec* __restrict__ vrec, uint32_t* __restrict__ keys) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrim) return;
    uint32_t b = (rmask[r >> 2] >> (8u * (r & 3u))) & 0xFFu;
    if (!b) return;
    const uint32_t lin = cxc_rim_lin(G, r);
    uint32_t o = rbase[r];
    while (b) {
        const uint32_t d = (uint32_t)__ffs((int)b) - 1u;
        b &= b - 1u;
        keys[o] = (lin << 3) | d;
        vrec[o++] = make_uint2((lin << 3) | d, 0u);
    }
}
// One lane per face-triangle.  One inside (corner i): (p_i, c(i,j), c(i,k)).  Two inside (i outside): (c(i,j), p_j, p_k) and
// (c(i,j), p_k, c(k,i)) -- the quad's diagonal runs from the crossing behind the outside corner to the corner before it, a rule of the
// triangle's own corner numbers.  A face with its bit in G.reversed exchanges the last two corners of every triangle.
__global__ __launch_bounds__(256) void cxc_k_emit(cxc_geom G, const u64* __restrict__ bits, const u64* __restrict__ table, u64 mask, const uint32_t* __restrict__ rmask,
                                                  const uint32_t* __restrict__ rbase, const uint32_t* __restrict__ toff, uint32_t nv0, int32_t* __restrict__ tris) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= G.item0[6]) return;
    const cxc_tri T = cxc_triangle(G, bits, e);
    const uint32_t m = (uint32_t)__popc(T.in);
    if (!m) return;
    // the vertex of every inside corner and of every edge with a crossing (edge c joins corners c and (c+1) % 3)
    uint32_t lat[3] = {0u, 0u, 0u}, crs[3] = {0u, 0u, 0u};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int c1 = (c + 1) % 3;
        if ((T.in >> c) & 1u) lat[c] = nv0 + rbase[T.rim[c]];
        if (((T.in >> c) ^ (T.in >> c1)) & 1u) {
            const uint32_t v = cxc_find(table, mask, T.ekey[c]);
            if (v != CXD_NONE) crs[c] = v;
            else {      // the cap's own: behind the owner's lattice-point vertex and its missing crossings of smaller direction
                const uint32_t r = T.eown[c], b = (rmask[r >> 2] >> (8u * (r & 3u))) & 0xFFu;
                crs[c] = nv0 + rbase[r] + (uint32_t)__popc(b & ((1u << (T.ekey[c] & 7u)) - 1u));
            }
        }
    }
    uint32_t r0[3] = {lat[0], lat[1], lat[2]}, r1[3] = {0u, 0u, 0u};
    if (m != 3u) {
        const uint32_t want = m == 1u ? 1u : 0u;      // the corner the rule rotates to the front: the inside one of one, the outside one of two
        const uint32_t i = ((T.in & 1u) == want) ? 0u : ((((T.in >> 1) & 1u) == want) ? 1u : 2u), j = (i + 1u) % 3u, k = (i + 2u) % 3u;
        const uint32_t ci = cxc_sel3(crs[0], crs[1], crs[2], i), ck = cxc_sel3(crs[0], crs[1], crs[2], k);      // c(i,j) and c(k,i)
        const uint32_t pk = cxc_sel3(lat[0], lat[1], lat[2], k);
        if (m == 1u) { r0[0] = cxc_sel3(lat[0], lat[1], lat[2], i); r0[1] = ci; r0[2] = ck; }
        else {
            r0[0] = ci; r0[1] = cxc_sel3(lat[0], lat[1], lat[2], j); r0[2] = pk;
            r1[0] = ci; r1[1] = pk; r1[2] = ck;
        }
    }
    const bool rev = ((G.reversed >> T.face) & 1u) != 0u;
    size_t o = (size_t)toff[e] * 3;
    tris[o] = (int32_t)r0[0]; tris[o + 1] = (int32_t)(rev ? r0[2] : r0[1]); tris[o + 2] = (int32_t)(rev ? r0[1] : r0[2]);
    if (m == 2u) {
        o += 3;
        tris[o] = (int32_t)r1[0]; tris[o + 1] = (int32_t)(rev ? r1[2] : r1[1]); tris[o + 2] = (int32_t)(rev ? r1[1] : r1[2]);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// The sizes of a request, in plain integer arithmetic (also what a stand-alone host program can check): rim points, face-triangles and
// sign words per face.  Every extent is at least 2 (cx_grid_upload) and the samples number at most 2^29, so all of it fits 32 bits.
struct cxc_sizes {
    uint32_t nrim, items, words;
};
static cxc_sizes cxc_fill_geom(cxc_geom& G, uint32_t n0, uint32_t n1, uint32_t n2, uint32_t faces, bool below) {
    memset(&G, 0, sizeof(G));
    G.n0 = n0; G.n1 = n1; G.n2 = n2; G.plane = n1 * n2;
    G.ring = 2u * n2 + 2u * (n1 - 2u);
    G.faces = faces;
    uint32_t items = 0, words = 0;
    for (uint32_t f = 0; f < 6u; f++) {
        const uint32_t axis = f >> 1, nu = axis == 0u ? n1 : n0, nw = axis == 2u ? n1 : n2;
        // the corners of a face-triangle run counter-clockwise around e_u x e_w = +i, -j, +k.  The march's normals point from f < value to
        // f >= value: into the solid of "above", out of the solid of "below"; the cap's must do the same, so "above" wants the normal that
        // points into the array (+axis on a low face, -axis on a high one) and "below" the other
        const bool natural_positive = axis != 1u, want_positive = below ? (f & 1u) != 0u : (f & 1u) == 0u;
        if (natural_positive != want_positive) G.reversed |= 1u << f;
        G.item0[f] = items;
        G.word0[f] = words;
        if ((faces >> f) & 1u) items += 2u * (nu - 1u) * (nw - 1u);
        words += cx_blocks((size_t)nu * nw) * 4u;      // (one word per wave of cxc_k_signs)
    }
    G.item0[6] = items;
    G.dsq[0] = cx_fdiv_make(n2 - 1u); G.dsq[1] = cx_fdiv_make(n2 - 1u); G.dsq[2] = cx_fdiv_make(n1 - 1u);
    G.dplane = cx_fdiv_make(G.plane); G.drow = cx_fdiv_make(n2); G.dring = cx_fdiv_make(G.ring);
    cxc_sizes Z;
    Z.nrim = 2u * G.plane + (n0 - 2u) * G.ring;
    Z.items = items; Z.words = words;
    return Z;
}

static int cxc_refuse(cx_ctx* ctx, const char* who, const char* why) {
    ctx->err = std::string(who) + ": " + why;
    return CX_ERR_UNSUPPORTED;
}
// what no cap is built for: checked before anything is written
static int cxc_route_checks(cx_ctx* ctx, const char* who) {
    if (!ctx->extracted || !ctx->grid.p) { ctx->err = std::string(who) + ": no valid extraction"; return CX_ERR_STATE; }
    if (ctx->keep_valid) return cxc_refuse(ctx, who, "a seeded selection is in force (its components end where the selection ends, not at the rim)");
    if (ctx->origin[0] < 0 || ctx->origin[1] < 0 || ctx->origin[2] < 0 || ctx->corner_ref[0] > 0 || ctx->corner_ref[1] > 0 || ctx->corner_ref[2] > 0)
        return cxc_refuse(ctx, who, "the array carries a margin (negative origin or a reference corner): its rim is not the grid's");
    if (ctx->origin[0] > 0 || ctx->origin[1] > 0 || ctx->origin[2] > 0)
        return cxc_refuse(ctx, who, "the array is a slab of a larger volume (cx_set_origin): its faces along the cut are not the volume's rim");
    return CX_OK;
}

extern "C" int cx_cap3d(cx_ctx* ctx, uint32_t faces, uint32_t flags, int64_t* counts4) {
    if (!ctx) return CX_ERR_INVALID;
    if (faces & ~0x3Fu) { ctx->err = "cx_cap3d: the face mask has six bits"; return CX_ERR_INVALID; }
    if (flags & ~CXC_BELOW) { ctx->err = "cx_cap3d: unknown flag bits (only CX_CAP_BELOW is defined)"; return CX_ERR_INVALID; }
    int rc = cxc_route_checks(ctx, "cx_cap3d");
    if (rc) return rc;
    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_counts C;
    if ((rc = cx_counts_get(ctx, &C))) return rc;
    if (C.n_vertices >= (1LL << 31) || C.n_triangles >= (1LL << 31)) return cxc_refuse(ctx, "cx_cap3d", "2^31 vertices or triangles or more");
    const uint32_t nv0 = (uint32_t)C.n_vertices, nt0 = (uint32_t)C.n_triangles;
    cx_cap_state* Z = ctx->cap;
    if (Z && ctx->cap_valid && Z->faces == faces && Z->flags == flags && Z->nv0 == nv0 && Z->nt0 == nt0) {   // the same request again
        if (counts4) memcpy(counts4, Z->counts, sizeof(Z->counts));
        return CX_OK;
    }
    if (!Z) ctx->cap = Z = new (std::nothrow) cx_cap_state();
    if (!Z) return CX_ERR_NOMEM;
    ctx->cap_valid = false;
    hipStream_t st = ctx->stream;
    for (int i = 0; i < 2; i++)
        if (!Z->ev[i]) CX_HIP(ctx, hipEventCreate(&Z->ev[i]));
    const cx_params& P = ctx->last;
    const bool below = (flags & CXC_BELOW) != 0u;
    cxc_geom G;
    const cxc_sizes S = cxc_fill_geom(G, P.n0, P.n1, P.n2, faces, below);
    if ((rc = Z->misc.grow(ctx, 16))) return rc;
    if ((rc = Z->bits.grow(ctx, (size_t)S.words + 16))) return rc;
    if ((rc = Z->rmask.grow(ctx, (size_t)S.nrim / 4 + 16))) return rc;
    if ((rc = Z->rcount.grow(ctx, (size_t)S.nrim + 16))) return rc;
    if ((rc = Z->rbase.grow(ctx, (size_t)S.nrim + 16))) return rc;
    if ((rc = Z->tcase.grow(ctx, (size_t)S.items + 16))) return rc;
    if ((rc = Z->tcount.grow(ctx, (size_t)S.items + 16))) return rc;
    if ((rc = Z->toff.grow(ctx, (size_t)S.items + 16))) return rc;
    if ((rc = Z->sums.grow(ctx, (size_t)std::max(S.items, S.nrim) / 1024 + 16))) return rc;
    CX_HIP(ctx, hipEventRecord(Z->ev[0], st));
    CX_HIP(ctx, hipMemsetAsync(Z->misc, 0, 16 * sizeof(uint32_t), st));
    uint32_t h[5] = {0, 0, 0, 0, 0};
    if (S.items) {
        CX_HIP(ctx, hipMemsetAsync(Z->rmask, 0, ((size_t)S.nrim / 4 + 1) * sizeof(uint32_t), st));
#define CX_LAUNCH(DT)                                                                                                                              \
        if (faces & 0x03u) hipLaunchKernelGGL((cxc_k_signs<DT, 0>), cx_grid1((size_t)G.plane), dim3(256), 0, st, P.grid, G, P.vcmp, below ? 1 : 0, Z->bits.get());    \
        if (faces & 0x0Cu) hipLaunchKernelGGL((cxc_k_signs<DT, 1>), cx_grid1((size_t)G.n0 * G.n2), dim3(256), 0, st, P.grid, G, P.vcmp, below ? 1 : 0, Z->bits.get()); \
        if (faces & 0x30u) hipLaunchKernelGGL((cxc_k_signs<DT, 2>), cx_grid1((size_t)G.n0 * G.n1), dim3(256), 0, st, P.grid, G, P.vcmp, below ? 1 : 0, Z->bits.get());
        CX_DISPATCH_DTYPE(P.grid.dtype, CX_LAUNCH)
#undef CX_LAUNCH
        hipLaunchKernelGGL(cxc_k_rim_count, cx_grid1(nv0), dim3(256), 0, st, (const cx_vrec*)ctx->verts.get(), nv0, G, Z->misc.get());
        CX_HIP(ctx, hipMemcpyAsync(h, Z->misc, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        CX_HIP(ctx, hipStreamSynchronize(st));
        CX_HIP(ctx, hipGetLastError());
        if (h[0] > nv0) { ctx->err = "cx_cap3d: more rim records than records"; return CX_ERR_HIP; }
        // the table holds the rim's crossings, not the mesh's: sized by their number
        const u64 tsz = cx_table_size(h[0]);
        if ((rc = Z->table.grow(ctx, (size_t)tsz))) return rc;
        hipLaunchKernelGGL(cxc_k_table_init, dim3((uint32_t)std::min<u64>(2048, (tsz + 255) / 256)), dim3(256), 0, st, Z->table.get(), (size_t)tsz);
        if (h[0]) hipLaunchKernelGGL(cxc_k_rim_insert, cx_grid1(nv0), dim3(256), 0, st, (const cx_vrec*)ctx->verts.get(), nv0, G, Z->table.get(), tsz - 1);
        hipLaunchKernelGGL(cxc_k_cases, cx_grid1(S.items), dim3(256), 0, st, G, (const u64*)Z->bits.get(), (const u64*)Z->table.get(), tsz - 1, Z->tcase.get(),
                           Z->tcount.get(), Z->rmask.get());
        hipLaunchKernelGGL(cxc_k_rim_counts, cx_grid1(S.nrim), dim3(256), 0, st, (const uint32_t*)Z->rmask.get(), S.nrim, Z->rcount.get(), Z->misc.get());
        if ((rc = cx_scan_u32(ctx, Z->rcount, Z->rbase, S.nrim, Z->sums, Z->misc + 1))) return rc;
        if ((rc = cx_scan_u32(ctx, Z->tcount, Z->toff, S.items, Z->sums, Z->misc + 2))) return rc;
        CX_HIP(ctx, hipMemcpyAsync(h, Z->misc, 5 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        CX_HIP(ctx, hipStreamSynchronize(st));
        CX_HIP(ctx, hipGetLastError());
        const uint32_t ncv = h[1], nct = h[2];
        if (ncv != h[3] + h[4] || ncv > 8u * S.nrim || nct > 2u * S.items) { ctx->err = "cx_cap3d: the scans do not add up"; return CX_ERR_HIP; }
        if ((u64)nv0 + ncv >= (1ULL << 31) || (u64)nt0 + nct >= (1ULL << 31)) return cxc_refuse(ctx, "cx_cap3d", "2^31 vertices or triangles or more with the cap");
        if ((rc = Z->vrec.grow(ctx, (size_t)ncv + 16))) return rc;
        if ((rc = Z->keys.grow(ctx, (size_t)ncv + 16))) return rc;
        if ((rc = Z->tris.grow(ctx, (size_t)nct * 3 + 16))) return rc;
        if (ncv) hipLaunchKernelGGL(cxc_k_keys, cx_grid1(S.nrim), dim3(256), 0, st, G, (const uint32_t*)Z->rmask.get(), (const uint32_t*)Z->rbase.get(), S.nrim, Z->vrec.get(), Z->keys.get());
        if (nct) hipLaunchKernelGGL(cxc_k_emit, cx_grid1(S.items), dim3(256), 0, st, G, (const u64*)Z->bits.get(), (const u64*)Z->table.get(), tsz - 1,
                                    (const uint32_t*)Z->rmask.get(), (const uint32_t*)Z->rbase.get(), (const uint32_t*)Z->toff.get(), nv0, Z->tris.get());
        CX_HIP(ctx, hipGetLastError());
        Z->info[2] = (double)tsz;
    }
    CX_HIP(ctx, hipEventRecord(Z->ev[1], st));
    CX_HIP(ctx, hipStreamSynchronize(st));
    float ms = 0.0f;
    CX_HIP(ctx, hipEventElapsedTime(&ms, Z->ev[0], Z->ev[1]));
    Z->info[0] = ms; Z->info[1] = h[0]; Z->info[3] = S.nrim;
    Z->faces = faces; Z->flags = flags; Z->nv0 = nv0; Z->nt0 = nt0;
    Z->ncv = h[1]; Z->nct = h[2];
    Z->counts[0] = h[3]; Z->counts[1] = h[2]; Z->counts[2] = h[4]; Z->counts[3] = (int64_t)h[0] + h[4];
    ctx->cap_valid = true;
    if (counts4) memcpy(counts4, Z->counts, sizeof(Z->counts));
    return CX_OK;
}

static int cxc_current(cx_ctx* ctx, const char* who, cx_cap_state** out) {
    if (!ctx->cap || !ctx->cap_valid) { ctx->err = std::string(who) + ": no cap of the current extraction (cx_cap3d comes after the extraction, level or seeded selection it caps)"; return CX_ERR_STATE; }
    *out = ctx->cap;
    return CX_OK;
}

extern "C" int cx_cap3d_download(cx_ctx* ctx, uint32_t* keys, int32_t* tris) {
    if (!ctx) return CX_ERR_INVALID;
    cx_cap_state* Z = nullptr;
    int rc = cxc_current(ctx, "cx_cap3d_download", &Z);
    if (rc) return rc;
    CX_HIP(ctx, hipSetDevice(ctx->device));
    if (keys && Z->ncv && (rc = cx_copy_to_host1(ctx, keys, Z->keys, (size_t)Z->ncv * sizeof(uint32_t)))) return rc;
    if (tris && Z->nct && (rc = cx_copy_to_host1(ctx, tris, Z->tris, (size_t)Z->nct * 3 * sizeof(int32_t)))) return rc;
    return CX_OK;
}

extern "C" int cx_cap3d_info(cx_ctx* ctx, double* info4) {
    if (!ctx || !info4) return CX_ERR_INVALID;
    cx_cap_state* Z = nullptr;
    const int rc = cxc_current(ctx, "cx_cap3d_info", &Z);
    if (rc) return rc;
    memcpy(info4, Z->info, sizeof(Z->info));
    return CX_OK;
}

int cx_cap_view_get(cx_ctx* ctx, const char* who, cx_cap_view* out) {
    cx_cap_state* Z = nullptr;
    int rc = cxc_current(ctx, who, &Z);       // (a cap that is gone is CX_ERR_STATE whatever took it; a valid one is no licence on a refused route)
    if (!rc) rc = cxc_route_checks(ctx, who);
    if (rc) return rc;
    if (Z->nv0 != (uint32_t)ctx->counts.n_vertices || Z->nt0 != (uint32_t)ctx->counts.n_triangles) { ctx->err = std::string(who) + ": the cap belongs to another extraction"; return CX_ERR_STATE; }
    out->vrec = Z->vrec; out->tris = Z->tris; out->ncv = Z->ncv; out->nct = Z->nct;
    return CX_OK;
}
