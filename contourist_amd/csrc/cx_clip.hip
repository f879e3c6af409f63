// cx_clip.hip -- clipping of the Level-1 mesh by a per-vertex scalar (include/contourist_hip.h, section "clipping").
//
// d[v] = s[v] - threshold (or its negative); a vertex is inside iff d is finite and >= 0.  Most triangles of a clipped mesh are wholly
// kept or wholly dropped, so the passes over all triangles read little and the work per cut edge is done on the cut band only:
//   cxk_k_classify      one lane per vertex: d[v]; two BIT masks, one word per wave (ballot): inside, and special (inside: d == 0;
//                       outside: d not finite) -- 2 bits per vertex that stay in L2 instead of three random doubles per triangle
//   cxk_k_cases         one lane per triangle: three bit lookups -> a case byte {cut edges, output triangles, rotation}, the counts of
//                       output triangles and cut corners (cx_scan_u32 turns them into offsets); one atomic per wave and counter
//   cxk_k_insert        cut triangles only: (lo << 32) | hi of every cut edge into an open-addressing table sized by the number of cut
//                       corners, atomicMin of the corner number 3t + k as the edge's representative; the corners are compacted
//   cxk_k_first         per compacted corner: is it its edge's representative?  cx_scan_u32 of the flags = the cut-vertex ranks (the
//                       compacted corners ascend with 3t + k)
//   cxk_k_cut_vertices  one lane per compacted corner, the representatives work: t, position, normal, the record {lo, hi, t}
//   cxk_k_old_vertices  the V old vertices in their order in front of the cut vertices
//   cxk_k_emit          one lane per source triangle: 0 / 1 / 2 triangles at their offsets; wholly kept triangles are a copy
// then the shared tail of the post-pass (cx_level1_clip_tail in cx_post.hip): clean, compaction, orientation; and
//   cxk_k_finish        one lane per OUTPUT vertex: the map record and the carried normal, found through the vertex's key
// Integer atomics only (compare-and-swap, minimum, add): nothing depends on the order the lanes arrive in.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>

#include "cx_ctx.h"
#include "cx_dev.h"

extern "C" int cx_level1_normals(cx_ctx* ctx, const double* delta3, void** normals_dev);

#define CXK_NO_CLEAN 1u
#define CXK_KEEP_BELOW 2u
#define CXK_NORMALS 4u
// case byte of a source triangle: bits 0-2 the cut edges (edge k joins corners k and (k+1)%3), bits 3-4 the output triangles, bits 5-6
// the corner the rule rotates to the front (the inside one of one, the outside one of two), bit 7: two corners inside
#define CXK_TWO_INSIDE 0x80u

struct cx_clip_state {
    cx_buf<double> sc;            // the caller's scalars when they came from the host
    cx_buf<double> d;             // d[v]
    cx_buf<u64> bits;             // inside words, then special words (one word per wave of cxk_k_classify)
    cx_buf<uint8_t> tcase;        // per source triangle: the case byte
    cx_buf<uint32_t> tout, tcut;  // per source triangle: output triangles / cut corners; tcut is then overwritten by the output offsets
    cx_buf<uint32_t> toffc;       // per source triangle: first compacted corner
    cx_buf<uint32_t> sums, misc;  // scan scratch; [0] cut corners [1] output triangles [2] cut triangles [3] non-finite triangles [4] d == 0 vertices [5] cut vertices
    cx_buf<u64> ekeys;            // edge table of the cut band: keys
    cx_buf<uint32_t> emin;        // per slot: the smallest corner number, then the cut vertex's rank
    cx_buf<uint32_t> cslot, ccorner, cflag, crank;   // per compacted corner
    cx_buf<int32_t> rec_lohi;     // per cut vertex
    cx_buf<double> rec_t, rec_n;
    cx_buf<int32_t> map_lohi;     // per OUTPUT vertex
    cx_buf<double> map_t;
    uint64_t map_gen = 0;         // generation of the Level-1 mesh the map belongs to (0: none)
    uint32_t map_n = 0;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    double info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool ran = false;
};

void cx_clip_free(cx_ctx* ctx) {
    cx_clip_state* Z = ctx->clip;
    if (!Z) return;
    for (int i = 0; i < 3; i++)
        if (Z->ev[i]) (void)hipEventDestroy(Z->ev[i]);
    delete Z;
    ctx->clip = nullptr;
}

// ---- device -------------------------------------------------------------------------------------------------------------------------
// bit 0: inside; bit 1: special (3: inside with d == 0; 2: d not finite)
__device__ __forceinline__ uint32_t cxk_code(const u64* __restrict__ inside, const u64* __restrict__ special, uint32_t v) {
    const uint32_t w = v >> 6, b = v & 63u;
    return (uint32_t)((inside[w] >> b) & 1ULL) | ((uint32_t)((special[w] >> b) & 1ULL) << 1);
}
// the case byte from the three codes (cc = c0 | c1 << 2 | c2 << 4); no triangle with a non-finite vertex gets here
__device__ __forceinline__ uint32_t cxk_case(uint32_t cc) {
    const uint32_t in0 = cc & 1u, in1 = (cc >> 2) & 1u, in2 = (cc >> 4) & 1u;
    const uint32_t nin = in0 + in1 + in2;
    if (nin == 3u) return 1u << 3;
    if (nin == 0u) return 0u;
    if (nin == 1u) {
        const uint32_t i = in0 ? 0u : (in1 ? 1u : 2u);
        if (((cc >> (2u * i)) & 3u) == 3u) return 0u;                 // both cut points ARE vertex i: (i, i, i)
        const uint32_t k = (i + 2u) % 3u;
        return (1u << i) | (1u << k) | (1u << 3) | (i << 5);
    }
    const uint32_t i = !in0 ? 0u : (!in1 ? 1u : 2u), j = (i + 1u) % 3u, k = (i + 2u) % 3u;
    const uint32_t m = ((((cc >> (2u * j)) & 3u) != 3u) ? (1u << i) : 0u) | ((((cc >> (2u * k)) & 3u) != 3u) ? (1u << k) : 0u);
    return m | ((uint32_t)__popc(m) << 3) | (i << 5) | CXK_TWO_INSIDE;
}

__global__ void cxk_k_table_init(u64* __restrict__ keys, uint32_t* __restrict__ vals, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) { keys[i] = CXD_EMPTY; vals[i] = CXD_NONE; }
}
// One lane per vertex.  PLANE: s = n0 x + n1 y + n2 z, every operation rounded once, left to right.
template <bool PLANE>
__global__ __launch_bounds__(256) void cxk_k_classify(const double* __restrict__ pts, const double* __restrict__ sc, uint32_t nv, double n0, double n1, double n2,
                                                      double thr, int below, double* __restrict__ d, u64* __restrict__ inside, u64* __restrict__ special,
                                                      uint32_t* nzero) {
#pragma clang fp contract(off)
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    bool in = false, sp = false;
    if (v < nv) {
        double s;
        if (PLANE) s = (n0 * pts[(size_t)v * 3] + n1 * pts[(size_t)v * 3 + 1]) + n2 * pts[(size_t)v * 3 + 2];
        else s = sc[v];
        const double dv = below ? thr - s : s - thr;
        d[v] = dv;
        const bool fin = __builtin_isfinite(dv);
        in = fin && dv >= 0.0;
        sp = !fin || dv == 0.0;
    }
    const u64 mi = __ballot(in), ms = __ballot(sp);
    if ((threadIdx.x & 63u) == 0u) {
        inside[v >> 6] = mi; special[v >> 6] = ms;
        const uint32_t nz = (uint32_t)__popcll(mi & ms);
        if (nz) atomicAdd(nzero, nz);
    }
}
// One lane per triangle: the case byte and the two counts.
__global__ __launch_bounds__(256) void cxk_k_cases(const int32_t* __restrict__ tri, uint32_t nt, uint32_t nv, const u64* __restrict__ inside,
                                                   const u64* __restrict__ special, uint8_t* __restrict__ tcase, uint32_t* __restrict__ tout,
                                                   uint32_t* __restrict__ tcut, uint32_t* counters) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    bool cut = false, bad = false;
    if (t < nt) {
        const uint32_t a = (uint32_t)tri[(size_t)t * 3], b = (uint32_t)tri[(size_t)t * 3 + 1], c = (uint32_t)tri[(size_t)t * 3 + 2];
        uint32_t cs = 0u;
        if (a < nv && b < nv && c < nv) {
            const uint32_t c0 = cxk_code(inside, special, a), c1 = cxk_code(inside, special, b), c2 = cxk_code(inside, special, c);
            bad = c0 == 2u || c1 == 2u || c2 == 2u;
            if (!bad) cs = cxk_case(c0 | (c1 << 2) | (c2 << 4));
        } else bad = true;                                  // (an index past the vertices: dropped with the non-finite ones)
        cut = (cs & 7u) != 0u;
        tcase[t] = (uint8_t)cs;
        tout[t] = (cs >> 3) & 3u;
        tcut[t] = (uint32_t)__popc(cs & 7u);
    }
    const u64 mc = __ballot(cut), mb = __ballot(bad);
    if ((threadIdx.x & 63u) == 0u) {
        if (mc) atomicAdd(counters + 2, (uint32_t)__popcll(mc));
        if (mb) atomicAdd(counters + 3, (uint32_t)__popcll(mb));
    }
}
// Cut triangles only: their cut edges into the table, the smallest corner number per edge, the compacted corners.
__global__ __launch_bounds__(256) void cxk_k_insert(const int32_t* __restrict__ tri, uint32_t nt, const uint8_t* __restrict__ tcase,
                                                    const uint32_t* __restrict__ toffc, u64* ekeys, uint32_t* emin, u64 mask,
                                                    uint32_t* __restrict__ cslot, uint32_t* __restrict__ ccorner) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const uint32_t m = tcase[t] & 7u;
    if (!m) return;
    const uint32_t a = (uint32_t)tri[(size_t)t * 3], b = (uint32_t)tri[(size_t)t * 3 + 1], c = (uint32_t)tri[(size_t)t * 3 + 2];
    uint32_t j = toffc[t];
#pragma unroll
    for (uint32_t e = 0; e < 3u; e++) {
        if (!((m >> e) & 1u)) continue;
        const uint32_t va = e == 0u ? a : (e == 1u ? b : c), vb = e == 0u ? b : (e == 1u ? c : a);
        const u64 key = ((u64)min(va, vb) << 32) | (u64)max(va, vb);
        u64 s = cxd_mix(key) & mask;
        for (;;) {
            u64 cur = __hip_atomic_load(&ekeys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == CXD_EMPTY) cur = atomicCAS(&ekeys[s], CXD_EMPTY, key);
            if (cur == CXD_EMPTY || cur == key) break;
            s = (s + 1) & mask;
        }
        const uint32_t corner = 3u * t + e;
        atomicMin(&emin[s], corner);
        cslot[j] = (uint32_t)s; ccorner[j] = corner;
        j++;
    }
}
__global__ void cxk_k_first(const uint32_t* __restrict__ cslot, const uint32_t* __restrict__ ccorner, const uint32_t* __restrict__ emin, uint32_t nc,
                            uint32_t* __restrict__ cflag) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nc) return;
    cflag[j] = emin[cslot[j]] == ccorner[j] ? 1u : 0u;
}
// One lane per compacted corner; the representative of an edge makes its cut vertex r: t = d[lo] / (d[lo] - d[hi]),
// p = p[lo] + t (p[hi] - p[lo]), n = normalize((1 - t) n[lo] + t n[hi]); the slot's word becomes r for cxk_k_emit.
__global__ __launch_bounds__(256) void cxk_k_cut_vertices(const uint32_t* __restrict__ cslot, const uint32_t* __restrict__ cflag, const uint32_t* __restrict__ crank,
                                                          uint32_t nc, const u64* __restrict__ ekeys, uint32_t* __restrict__ emin, const double* __restrict__ d,
                                                          const double* __restrict__ pts, const double* __restrict__ nrm, uint32_t nv, double* __restrict__ pts2,
                                                          uint32_t* __restrict__ prio, int32_t* __restrict__ rec_lohi, double* __restrict__ rec_t,
                                                          double* __restrict__ rec_n) {
#pragma clang fp contract(off)
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nc || !cflag[j]) return;
    const uint32_t s = cslot[j], r = crank[j];
    const u64 key = ekeys[s];
    const uint32_t lo = (uint32_t)(key >> 32), hi = (uint32_t)key;
    const double dl = d[lo], dh = d[hi];
    const double t = dl / (dl - dh);
    const size_t o = ((size_t)nv + r) * 3;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double pl = pts[(size_t)lo * 3 + a], ph = pts[(size_t)hi * 3 + a];
        pts2[o + a] = pl + t * (ph - pl);
    }
    prio[nv + r] = nv + r;
    rec_lohi[(size_t)r * 2] = (int32_t)lo; rec_lohi[(size_t)r * 2 + 1] = (int32_t)hi;
    rec_t[r] = t;
    if (nrm) {
        const double u = 1.0 - t;
        const double x = u * nrm[(size_t)lo * 3] + t * nrm[(size_t)hi * 3], y = u * nrm[(size_t)lo * 3 + 1] + t * nrm[(size_t)hi * 3 + 1],
                     z = u * nrm[(size_t)lo * 3 + 2] + t * nrm[(size_t)hi * 3 + 2];
        const double len = sqrt((x * x + y * y) + z * z);
        rec_n[(size_t)r * 3] = len > 0.0 ? x / len : 0.0;
        rec_n[(size_t)r * 3 + 1] = len > 0.0 ? y / len : 0.0;
        rec_n[(size_t)r * 3 + 2] = len > 0.0 ? z / len : 0.0;
    }
    emin[s] = r;
}
__global__ void cxk_k_old_vertices(const double* __restrict__ pts, uint32_t nv, double* __restrict__ pts2, uint32_t* __restrict__ prio) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
#pragma unroll
    for (int a = 0; a < 3; a++) pts2[(size_t)v * 3 + a] = pts[(size_t)v * 3 + a];
    prio[v] = v;
}
// One lane per source triangle.  One inside (corner i): (v_i, c(i,j), c(i,k)).  Two inside (i outside): (c(j,i), v_j, v_k) and
// (c(j,i), v_k, c(k,i)); c(a,b) is vertex a itself where d[a] == 0, and the triangle that would then name a vertex twice is not emitted.
__global__ __launch_bounds__(256) void cxk_k_emit(const int32_t* __restrict__ tri, uint32_t nt, uint32_t nv, const uint8_t* __restrict__ tcase,
                                                  const uint32_t* __restrict__ toffo, const uint32_t* __restrict__ toffc, const uint32_t* __restrict__ cslot,
                                                  const uint32_t* __restrict__ erank, int32_t* __restrict__ tri2, uint32_t* __restrict__ tprio3,
                                                  uint8_t* __restrict__ alive) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const uint32_t cs = tcase[t], nout = (cs >> 3) & 3u;
    if (!nout) return;
    const uint32_t a = (uint32_t)tri[(size_t)t * 3], b = (uint32_t)tri[(size_t)t * 3 + 1], c = (uint32_t)tri[(size_t)t * 3 + 2];
    const uint32_t m = cs & 7u;
    size_t o = toffo[t];
    uint32_t r0[3] = {a, b, c}, r1[3] = {0u, 0u, 0u};
    if (m) {
        const uint32_t i = (cs >> 5) & 3u, k = (i + 2u) % 3u;
        const uint32_t vi = i == 0u ? a : (i == 1u ? b : c), vj = i == 0u ? b : (i == 1u ? c : a), vk = i == 0u ? c : (i == 1u ? a : b);
        const uint32_t base = toffc[t];
        // the cut vertex on edge e is the rank its table slot holds; its compacted corner is the e-th set bit of m
        const uint32_t ci = ((m >> i) & 1u) ? nv + erank[cslot[base + (uint32_t)__popc(m & ((1u << i) - 1u))]] : vj;
        const uint32_t ck = ((m >> k) & 1u) ? nv + erank[cslot[base + (uint32_t)__popc(m & ((1u << k) - 1u))]] : vk;
        if (!(cs & CXK_TWO_INSIDE)) { r0[0] = vi; r0[1] = ci; r0[2] = ck; }
        else {
            const bool first = ((m >> i) & 1u) != 0u;
            r1[0] = ci; r1[1] = vk; r1[2] = ck;
            if (first) { r0[0] = ci; r0[1] = vj; r0[2] = vk; }
            else { r0[0] = r1[0]; r0[1] = r1[1]; r0[2] = r1[2]; }
        }
    }
    tri2[o * 3] = (int32_t)r0[0]; tri2[o * 3 + 1] = (int32_t)r0[1]; tri2[o * 3 + 2] = (int32_t)r0[2];
    tprio3[o * 3] = t; tprio3[o * 3 + 1] = t; tprio3[o * 3 + 2] = t;
    alive[o] = 1;
    if (nout == 2u) {
        o++;
        tri2[o * 3] = (int32_t)r1[0]; tri2[o * 3 + 1] = (int32_t)r1[1]; tri2[o * 3 + 2] = (int32_t)r1[2];
        tprio3[o * 3] = t; tprio3[o * 3 + 1] = t; tprio3[o * 3 + 2] = t;
        alive[o] = 1;
    }
}
// One lane per OUTPUT vertex: its key is its place in the list the tail was handed (old index, or V + r for cut vertex r).
__global__ void cxk_k_finish(const uint32_t* __restrict__ keys, uint32_t nv2, uint32_t nv_old, const int32_t* __restrict__ rec_lohi, const double* __restrict__ rec_t,
                             const double* __restrict__ rec_n, const double* __restrict__ nrm, int32_t* __restrict__ map_lohi, double* __restrict__ map_t,
                             double* __restrict__ nrm2) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv2) return;
    const uint32_t key = keys[v];
    if (key < nv_old) {
        map_lohi[(size_t)v * 2] = (int32_t)key; map_lohi[(size_t)v * 2 + 1] = (int32_t)key;
        map_t[v] = 0.0;
        if (nrm2) {
#pragma unroll
            for (int a = 0; a < 3; a++) nrm2[(size_t)v * 3 + a] = nrm[(size_t)key * 3 + a];
        }
    } else {
        const uint32_t r = key - nv_old;
        map_lohi[(size_t)v * 2] = rec_lohi[(size_t)r * 2]; map_lohi[(size_t)v * 2 + 1] = rec_lohi[(size_t)r * 2 + 1];
        map_t[v] = rec_t[r];
        if (nrm2) {
#pragma unroll
            for (int a = 0; a < 3; a++) nrm2[(size_t)v * 3 + a] = rec_n[(size_t)r * 3 + a];
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// plane3 != nullptr: the plane's normal (s is computed from the points); otherwise sc: V scalars, on the device when on_device
static int cxk_clip(cx_ctx* ctx, const char* who, const double* plane3, const double* sc, int on_device, double thr, uint32_t flags, int64_t* out_counts) {
    cx_level1_comp_view V;
    CX_HIP(ctx, hipSetDevice(ctx->device));
    int rc = cx_level1_comp_view_get(ctx, who, &V);
    if (rc) return rc;
    if (flags & ~7u) { ctx->err = std::string(who) + ": unknown flag bits (only CX_CLIP_NO_CLEAN, CX_CLIP_KEEP_BELOW and CX_CLIP_NORMALS are defined)"; return CX_ERR_INVALID; }
    const uint32_t nv = V.nv, nt = V.nt;
    if (!plane3 && !sc && nv) { ctx->err = std::string(who) + ": one scalar per vertex is needed"; return CX_ERR_INVALID; }
    if ((u64)nt >= (1ULL << 30)) { ctx->err = std::string(who) + ": 2^30 triangles or more (the corner number 3 t + k is a 32-bit word)"; return CX_ERR_UNSUPPORTED; }
    const bool want_normals = (flags & CXK_NORMALS) != 0u;
    // the source's normals first: where they cannot be served nothing has been touched
    const double* nsrc = nullptr;
    if (want_normals) {
        const double* carried = nullptr;
        uint32_t nvc = 0;
        if (cx_level1_carried_normals(ctx, &carried, &nvc) == 2) {
            ctx->err = std::string(who) + ": CX_CLIP_NORMALS on a derived mesh that carries no normals";
            return CX_ERR_UNSUPPORTED;
        }
        void* dev = nullptr;
        if ((rc = cx_level1_normals(ctx, nullptr, &dev))) return rc;
        nsrc = (const double*)dev;
    }
    if (!ctx->clip) ctx->clip = new (std::nothrow) cx_clip_state();
    if (!ctx->clip) return CX_ERR_NOMEM;
    cx_clip_state* Z = ctx->clip;
    hipStream_t st = ctx->stream;
    for (int i = 0; i < 3; i++)
        if (!Z->ev[i]) CX_HIP(ctx, hipEventCreate(&Z->ev[i]));
    if ((rc = Z->misc.grow(ctx, 16))) return rc;
    const size_t nwords = (size_t)cx_grid1(nv).x * 4u;
    if (nv) {
        if ((rc = Z->d.grow(ctx, (size_t)nv + 16))) return rc;
        if ((rc = Z->bits.grow(ctx, 2 * nwords))) return rc;
        if (!plane3 && !on_device) {
            if ((rc = Z->sc.grow(ctx, (size_t)nv + 16))) return rc;
            CX_HIP(ctx, hipMemcpyAsync(Z->sc, sc, (size_t)nv * sizeof(double), hipMemcpyHostToDevice, st));
            CX_HIP(ctx, hipStreamSynchronize(st));
            sc = Z->sc;
        }
    }
    if (nt) {
        if ((rc = Z->tcase.grow(ctx, (size_t)nt + 16))) return rc;
        if ((rc = Z->tout.grow(ctx, (size_t)nt + 16))) return rc;
        if ((rc = Z->tcut.grow(ctx, (size_t)nt + 16))) return rc;
        if ((rc = Z->toffc.grow(ctx, (size_t)nt + 16))) return rc;
        if ((rc = Z->sums.grow(ctx, (size_t)nt / 1024 + 16))) return rc;
    }
    CX_HIP(ctx, hipEventRecord(Z->ev[0], st));
    CX_HIP(ctx, hipMemsetAsync(Z->misc, 0, 16 * sizeof(uint32_t), st));
    u64* inside = Z->bits;
    u64* special = inside + nwords;
    uint32_t h[6] = {0, 0, 0, 0, 0, 0};
    u64 tsz = 0;
    if (nv) {
        if (plane3) hipLaunchKernelGGL((cxk_k_classify<true>), cx_grid1(nv), dim3(256), 0, st, V.pts, (const double*)nullptr, nv, plane3[0], plane3[1], plane3[2], thr,
                                       (flags & CXK_KEEP_BELOW) ? 1 : 0, Z->d, inside, special, Z->misc + 4);
        else hipLaunchKernelGGL((cxk_k_classify<false>), cx_grid1(nv), dim3(256), 0, st, V.pts, sc, nv, 0.0, 0.0, 0.0, thr, (flags & CXK_KEEP_BELOW) ? 1 : 0, Z->d,
                                inside, special, Z->misc + 4);
    }
    if (nv && nt) {
        hipLaunchKernelGGL(cxk_k_cases, cx_grid1(nt), dim3(256), 0, st, V.tri, nt, nv, (const u64*)inside, (const u64*)special, Z->tcase, Z->tout, Z->tcut, Z->misc);
        if ((rc = cx_scan_u32(ctx, Z->tcut, Z->toffc, nt, Z->sums, Z->misc))) return rc;
        if ((rc = cx_scan_u32(ctx, Z->tout, Z->tcut, nt, Z->sums, Z->misc + 1))) return rc;      // (tcut: the output offsets from here on)
    }
    CX_HIP(ctx, hipMemcpyAsync(h, Z->misc, 5 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    CX_HIP(ctx, hipStreamSynchronize(st));
    CX_HIP(ctx, hipGetLastError());
    const uint32_t nc = h[0], nto = h[1];
    if (nc > 2u * nt || nto > 2u * nt) { ctx->err = std::string(who) + ": the scans do not add up"; return CX_ERR_HIP; }
    uint32_t ncv = 0;
    if (nc) {
        // the table holds the cut band's edges, not the mesh's: sized by the cut corners
        tsz = cx_table_size(nc);
        if ((rc = Z->ekeys.grow(ctx, (size_t)tsz))) return rc;
        if ((rc = Z->emin.grow(ctx, (size_t)tsz))) return rc;
        if ((rc = Z->cslot.grow(ctx, (size_t)nc + 16))) return rc;
        if ((rc = Z->ccorner.grow(ctx, (size_t)nc + 16))) return rc;
        if ((rc = Z->cflag.grow(ctx, (size_t)nc + 16))) return rc;
        if ((rc = Z->crank.grow(ctx, (size_t)nc + 16))) return rc;
        if ((rc = Z->sums.grow(ctx, (size_t)(nc > nt ? nc : nt) / 1024 + 16))) return rc;
        hipLaunchKernelGGL(cxk_k_table_init, dim3((uint32_t)std::min<u64>(2048, (tsz + 255) / 256)), dim3(256), 0, st, Z->ekeys, Z->emin, (size_t)tsz);
        hipLaunchKernelGGL(cxk_k_insert, cx_grid1(nt), dim3(256), 0, st, V.tri, nt, (const uint8_t*)Z->tcase, (const uint32_t*)Z->toffc, Z->ekeys, Z->emin, tsz - 1,
                           Z->cslot, Z->ccorner);
        hipLaunchKernelGGL(cxk_k_first, cx_grid1(nc), dim3(256), 0, st, (const uint32_t*)Z->cslot, (const uint32_t*)Z->ccorner, (const uint32_t*)Z->emin, nc, Z->cflag);
        if ((rc = cx_scan_u32(ctx, Z->cflag, Z->crank, nc, Z->sums, Z->misc + 5))) return rc;
        CX_HIP(ctx, hipMemcpyAsync(&ncv, Z->misc + 5, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        CX_HIP(ctx, hipStreamSynchronize(st));
        CX_HIP(ctx, hipGetLastError());
        if (ncv > nc || !ncv) { ctx->err = std::string(who) + ": the cut vertices do not add up"; return CX_ERR_HIP; }
    }
    if ((u64)nv + ncv >= (1ULL << 31)) { ctx->err = std::string(who) + ": 2^31 vertices or more after the cut"; return CX_ERR_UNSUPPORTED; }
    const uint32_t nv_raw = nv + ncv;
    cx_level1_clip_io B;
    if ((rc = cx_level1_clip_bufs(ctx, nv_raw, nto, &B))) return rc;
    if (ncv) {
        if ((rc = Z->rec_lohi.grow(ctx, (size_t)ncv * 2 + 16))) return rc;
        if ((rc = Z->rec_t.grow(ctx, (size_t)ncv + 16))) return rc;
        if (want_normals && (rc = Z->rec_n.grow(ctx, (size_t)ncv * 3 + 16))) return rc;
    }
    if (nto) {
        hipLaunchKernelGGL(cxk_k_old_vertices, cx_grid1(nv), dim3(256), 0, st, V.pts, nv, B.pts, B.prio);
        if (ncv) hipLaunchKernelGGL(cxk_k_cut_vertices, cx_grid1(nc), dim3(256), 0, st, (const uint32_t*)Z->cslot, (const uint32_t*)Z->cflag, (const uint32_t*)Z->crank, nc,
                                    (const u64*)Z->ekeys, Z->emin, (const double*)Z->d, V.pts, want_normals ? nsrc : (const double*)nullptr, nv, B.pts, B.prio,
                                    Z->rec_lohi, Z->rec_t, want_normals ? Z->rec_n.get() : (double*)nullptr);
        hipLaunchKernelGGL(cxk_k_emit, cx_grid1(nt), dim3(256), 0, st, V.tri, nt, nv, (const uint8_t*)Z->tcase, (const uint32_t*)Z->tcut, (const uint32_t*)Z->toffc,
                           (const uint32_t*)Z->cslot, (const uint32_t*)Z->emin, B.tri, B.tprio3, B.alive);
    }
    CX_HIP(ctx, hipGetLastError());
    CX_HIP(ctx, hipEventRecord(Z->ev[1], st));
    // ---- the tail: from here on the mesh is the new one
    Z->map_gen = 0;
    int64_t counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if ((rc = cx_level1_clip_tail(ctx, nto ? nv_raw : 0u, nto, !(flags & CXK_NO_CLEAN), counts))) return rc;      // (synchronises the stream)
    const uint32_t nv2 = (uint32_t)counts[0];
    if (nv2) {
        if ((rc = cx_level1_comp_view_get(ctx, who, &V))) return rc;
        if ((rc = Z->map_lohi.grow(ctx, (size_t)nv2 * 2 + 16))) return rc;
        if ((rc = Z->map_t.grow(ctx, (size_t)nv2 + 16))) return rc;
    }
    double* nrm2 = nullptr;
    if (want_normals && (rc = cx_level1_clip_normals(ctx, &nrm2))) return rc;
    if (nv2) hipLaunchKernelGGL(cxk_k_finish, cx_grid1(nv2), dim3(256), 0, st, V.keys, nv2, nv, (const int32_t*)Z->rec_lohi, (const double*)Z->rec_t,
                                (const double*)Z->rec_n, nsrc, Z->map_lohi, Z->map_t, want_normals ? nrm2 : (double*)nullptr);
    CX_HIP(ctx, hipGetLastError());
    CX_HIP(ctx, hipEventRecord(Z->ev[2], st));
    CX_HIP(ctx, hipStreamSynchronize(st));
    Z->map_gen = cx_level1_generation(ctx); Z->map_n = nv2;
    float ms0 = 0.0f, ms1 = 0.0f;
    CX_HIP(ctx, hipEventElapsedTime(&ms0, Z->ev[0], Z->ev[1]));
    CX_HIP(ctx, hipEventElapsedTime(&ms1, Z->ev[1], Z->ev[2]));
    Z->info[0] = ms0; Z->info[1] = ms1; Z->info[2] = nc; Z->info[3] = (double)tsz; Z->info[4] = nv; Z->info[5] = nt; Z->info[6] = nv_raw; Z->info[7] = nto;
    Z->ran = true;
    counts[2] = ncv; counts[3] = h[2]; counts[5] = h[3]; counts[6] = h[4]; counts[7] = nto;
    if (out_counts) memcpy(out_counts, counts, sizeof(counts));
    return CX_OK;
}

extern "C" int cx_level1_clip_plane(cx_ctx* ctx, const double* plane4, uint32_t flags, int64_t* out_counts8) {
    if (!ctx) return CX_ERR_INVALID;
    if (!plane4) { ctx->err = "cx_level1_clip_plane: four doubles {n0, n1, n2, offset} are needed"; return CX_ERR_INVALID; }
    bool ok = std::isfinite(plane4[3]) && (plane4[0] != 0.0 || plane4[1] != 0.0 || plane4[2] != 0.0);
    for (int a = 0; a < 3; a++) ok = ok && std::isfinite(plane4[a]);
    if (!ok) { ctx->err = "cx_level1_clip_plane: the normal must be finite and not zero, the offset finite"; return CX_ERR_INVALID; }
    return cxk_clip(ctx, "cx_level1_clip_plane", plane4, nullptr, 0, plane4[3], flags, out_counts8);
}

extern "C" int cx_level1_clip_scalars(cx_ctx* ctx, const double* scalars, int on_device, double threshold, uint32_t flags, int64_t* out_counts8) {
    if (!ctx) return CX_ERR_INVALID;
    return cxk_clip(ctx, "cx_level1_clip_scalars", nullptr, scalars, on_device, threshold, flags, out_counts8);
}

static int cxk_map_get(cx_ctx* ctx, cx_clip_state** out) {
    cx_clip_state* Z = ctx->clip;
    if (!Z || !Z->map_gen || Z->map_gen != cx_level1_generation(ctx)) {
        ctx->err = "cx_level1_clip_map: no clip since the last post-pass, filter or simplification";
        return CX_ERR_STATE;
    }
    *out = Z;
    return CX_OK;
}

extern "C" int cx_level1_clip_map(cx_ctx* ctx, void** lo_hi_dev, void** t_dev) {
    if (!ctx) return CX_ERR_INVALID;
    cx_clip_state* Z = nullptr;
    const int rc = cxk_map_get(ctx, &Z);
    if (rc) return rc;
    if (lo_hi_dev) *lo_hi_dev = Z->map_n ? (void*)Z->map_lohi.get() : nullptr;
    if (t_dev) *t_dev = Z->map_n ? (void*)Z->map_t.get() : nullptr;
    return CX_OK;
}

extern "C" int cx_level1_clip_map_download(cx_ctx* ctx, int32_t* lo_hi, double* t) {
    if (!ctx) return CX_ERR_INVALID;
    cx_clip_state* Z = nullptr;
    int rc = cxk_map_get(ctx, &Z);
    if (rc || !Z->map_n) return rc;
    CX_HIP(ctx, hipSetDevice(ctx->device));
    if (lo_hi && (rc = cx_copy_to_host1(ctx, lo_hi, Z->map_lohi, (size_t)Z->map_n * 2 * sizeof(int32_t)))) return rc;
    if (t && (rc = cx_copy_to_host1(ctx, t, Z->map_t, (size_t)Z->map_n * sizeof(double)))) return rc;
    return CX_OK;
}

extern "C" int cx_level1_clip_info(cx_ctx* ctx, double* info8) {
    if (!ctx || !info8) return CX_ERR_INVALID;
    cx_clip_state* Z = ctx->clip;
    if (!Z || !Z->ran) { ctx->err = "cx_level1_clip_info: no clip has run on this context"; return CX_ERR_STATE; }
    memcpy(info8, Z->info, sizeof(Z->info));
    return CX_OK;
}
