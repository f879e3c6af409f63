// cx_slab4d.hip -- a 4-D volume of more than one extraction (2^28 samples), marched slab by slab along axis 0 and assembled on the device.
//
// Per slab the host binds planes i0 .. i1 (plus plane i1 as a halo unless the slab is the last), sets the origin (i0,0,0,0) -- the
// CPython-order 2-3 split then sees the whole volume's lattice -- and runs cx_extract4d; cx_slab4d_append then
//   1. sorts the slab's vertices together with the previous slab's halo vertices by edge id (LSD radix sort, 8 bits a pass, the
//      counting-sort layout of cxp_sb_ranks: a wave counts CXS_UNIT consecutive pairs per digit, the [digit][unit] matrix is scanned in
//      memory order, a second walk hands out stable ranks),
//   2. appends the owned vertices (lower lattice point below the halo plane) in ascending edge id, each once, with its global edge id
//      and its float64 crossing point interpolated in the whole volume's lattice -- the slab offset goes into the lattice coordinate
//      before interpolating, as cxp_k_vertices4_f64 does with an origin, so the points are those of a single extraction bit for bit,
//   3. resolves the previous slab's references to its halo vertices (they are this slab's plane-0 vertices; one the slab's own march
//      dropped -- an edge that only a hyper-voxel below the slab uses, samples EQUAL to the isovalue -- is taken from the halo list itself),
//   4. appends the slab's tetrahedra with assembly indices; a reference to one of its own halo vertices stays pending, -(1 + h).
// The march's table emits every tetrahedron oriented (tools/gen_tables.py orient_tet), and the append keeps the order of its four
// indices: the assembly is oriented as the single extraction is.  cx_slab4d_finish (cx_post4d.hip) runs the 4-D post-steps on it.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>

#include "cx_ctx.h"

#include "cx_post.h"
#include "cx_state4.h"

#define CXS_BINS 256u
#define CXS_UNIT 1024u        // pairs per wave and pass

void cx_slab4_free(cx_slab4*& A) {
    if (!A) return;
    delete A;
    A = nullptr;
}


// ---- kernels ---------------------------------------------------------------------------------------
// (edge id, source) pairs: the slab's own vertices (source = vertex index), then the previous slab's halo vertices (source = nv + h)
__global__ void cxs_k_pairs(const uint32_t* __restrict__ vkeys, uint32_t nv, const uint32_t* __restrict__ pend, uint32_t np, uint32_t* k,
                            uint32_t* v) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv + np) return;
    k[i] = i < nv ? vkeys[i] : pend[i - nv];
    v[i] = i;
}
// digit counts of one pass: wave w of the block takes unit blockIdx.x * 4 + w; hist[digit * nunits + unit] (every entry written)
__global__ __launch_bounds__(256) void cxs_k_hist(const uint32_t* __restrict__ k, uint32_t n, uint32_t shift, uint32_t nunits, uint32_t* hist) {
    __shared__ uint32_t h[4][CXS_BINS];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    for (uint32_t x = lane; x < CXS_BINS; x += 64u) h[w][x] = 0;
    __syncthreads();
    const uint32_t unit = blockIdx.x * 4u + w;
    for (uint32_t r = 0; r < CXS_UNIT / 64u; r++) {
        const size_t q = (size_t)unit * CXS_UNIT + r * 64u + lane;
        const bool in = q < n;
        const uint32_t d = in ? (k[q] >> shift) & 255u : 0u;
        uint64_t todo = __ballot(in);
        while (todo) {      // wave-uniform: one round per digit present among the 64
            const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
            const uint32_t dd = (uint32_t)__shfl((int)d, (int)leader);
            const uint64_t same = __ballot(in && d == dd) & todo;
            if (lane == leader) h[w][dd] += (uint32_t)__popcll(same);
            todo &= ~same;
        }
    }
    __syncthreads();
    if (unit < nunits)
        for (uint32_t x = lane; x < CXS_BINS; x += 64u) hist[(size_t)x * nunits + unit] = h[w][x];
}
// stable ranks from the scanned matrix (a cursor per digit of the unit in LDS) and the move of the pairs to them
__global__ __launch_bounds__(256) void cxs_k_scatter(const uint32_t* __restrict__ k, const uint32_t* __restrict__ v, uint32_t n, uint32_t shift,
                                                     const uint32_t* __restrict__ offs, uint32_t nunits, uint32_t* k2, uint32_t* v2) {
    __shared__ uint32_t h[4][CXS_BINS];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t unit = blockIdx.x * 4u + w;
    if (unit < nunits)
        for (uint32_t x = lane; x < CXS_BINS; x += 64u) h[w][x] = offs[(size_t)x * nunits + unit];
    __syncthreads();
    volatile uint32_t* cur = h[w];
    for (uint32_t r = 0; r < CXS_UNIT / 64u; r++) {
        const size_t q = (size_t)unit * CXS_UNIT + r * 64u + lane;
        const bool in = q < n;
        const uint32_t key = in ? k[q] : 0u, val = in ? v[q] : 0u;
        const uint32_t d = (key >> shift) & 255u;
        uint64_t todo = __ballot(in);
        uint32_t mine = 0;
        while (todo) {
            const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
            const uint32_t dd = (uint32_t)__shfl((int)d, (int)leader);
            const uint64_t same = __ballot(in && d == dd) & todo;
            const uint32_t base = cur[dd];
            if (in && d == dd) mine = base + (uint32_t)__popcll(same & ((1ULL << lane) - 1ULL));
            __builtin_amdgcn_wave_barrier();
            if (lane == leader) cur[dd] = base + (uint32_t)__popcll(same);
            __builtin_amdgcn_wave_barrier();
            todo &= ~same;
        }
        if (in) { k2[mine] = key; v2[mine] = val; }
    }
}
// on the sorted pairs: flag[i] = 1 for the first pair of every owned edge id (below `bound`); cnt[0] = pairs with an owned edge id
__global__ void cxs_k_mark(const uint32_t* __restrict__ K, uint32_t m, uint64_t bound, uint32_t* flag, uint32_t* cnt) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t key = K[i];
    const bool own = (uint64_t)key < bound;
    flag[i] = (own && (i == 0 || K[i - 1] != key)) ? 1u : 0u;
    if (own && (i + 1 == m || (uint64_t)K[i + 1] >= bound)) cnt[0] = i + 1;
}
struct cxs_place {
    const float* A;
    uint32_t n1, n2, n3;
    cx_fdiv d3, d2, d1;
    double value;
    int i0;                 // first plane of the slab in the whole volume
    uint64_t gofs;          // i0 * plane << 4: local edge id -> global edge id
    uint64_t bound;         // owned_planes * plane << 4: the first edge id of the halo plane
    uint32_t nv;            // the slab's own vertices (sources below nv)
    uint32_t base;          // assembled vertices before this slab
};
// float64 crossing point of a local edge id in the whole volume's lattice: cxp_k_vertices4_f64 with origin (i0,0,0,0), before bin_times
__device__ __forceinline__ void cxs_point(const cxs_place& P, uint32_t key, double x[4]) {
    const uint32_t lin = key >> 4, d = key & 15u;
    uint32_t q[4];
    q[0] = cx_div(lin, P.d3);
    uint32_t r = lin - q[0] * (P.n1 * P.n2 * P.n3);
    q[1] = cx_div(r, P.d2);
    r -= q[1] * (P.n2 * P.n3);
    q[2] = cx_div(r, P.d1);
    q[3] = r - q[2] * P.n3;
    const uint32_t lin2 = lin + ((d & 8u) ? P.n1 * P.n2 * P.n3 : 0u) + ((d & 4u) ? P.n2 * P.n3 : 0u) + ((d & 2u) ? P.n3 : 0u) + (d & 1u);
    const double f0 = (double)P.A[lin], f1 = (double)P.A[lin2];
    const bool owner_low = !(f0 > f1);
    const double flow = owner_low ? f0 : f1, fhigh = owner_low ? f1 : f0;
    double ratio = 0.5;
    const double den = 1.0 * (fhigh - flow);
    if (!(fabs(den) <= 1e-8)) ratio = (P.value - flow) / den;
    const uint32_t db[4] = {(d >> 3) & 1u, (d >> 2) & 1u, (d >> 1) & 1u, d & 1u};
    const int org[4] = {P.i0, 0, 0, 0};
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const double qa = (double)((int)q[a] + org[a]);
        const double low = owner_low ? qa : qa + (double)db[a];
        const double high = owner_low ? qa + (double)db[a] : qa;
        x[a] = low + ratio * (high - low);
    }
}
// every sorted pair: an owned edge id gets its assembly index (the first pair of the id writes the vertex); a halo edge id becomes
// pending entry h for the next slab
__global__ void cxs_k_place(const uint32_t* __restrict__ K, const uint32_t* __restrict__ V, const uint32_t* __restrict__ flag,
                            const uint32_t* __restrict__ pos, uint32_t m, const uint32_t* __restrict__ cnt, cxs_place P, uint64_t* keys,
                            double* pts, int32_t* vmap, int32_t* resolved, uint32_t* pend) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t key = K[i], src = V[i], hs = cnt[0];
    if (i < hs) {
        const uint32_t first = flag[i];
        const uint32_t idx = P.base + pos[i] + first - 1u;
        if (first) {
            double x[4];
            cxs_point(P, key, x);
            keys[idx] = P.gofs + (uint64_t)key;
            *reinterpret_cast<double2*>(pts + (size_t)idx * 4) = make_double2(x[0], x[1]);
            *reinterpret_cast<double2*>(pts + (size_t)idx * 4 + 2) = make_double2(x[2], x[3]);
        }
        if (src < P.nv) vmap[src] = (int32_t)idx;
        else resolved[src - P.nv] = (int32_t)idx;
    } else {
        const uint32_t h = i - hs;
        pend[h] = (uint32_t)((uint64_t)key - P.bound);
        if (src < P.nv) vmap[src] = -(int32_t)(h + 1u);
    }
}
__global__ void cxs_k_tets(const int32_t* __restrict__ tl, size_t n, const int32_t* __restrict__ vmap, int32_t* out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = vmap[tl[i]];
}
__global__ void cxs_k_resolve(int32_t* tets, size_t n, const int32_t* __restrict__ resolved) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t x = tets[i];
    if (x < 0) tets[i] = resolved[-(x + 1)];
}
__global__ void cxs_k_bad_refs(const int32_t* __restrict__ tets, size_t n, int32_t nv, uint32_t* bad) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t x = tets[i];
    if (x < 0 || x >= nv) atomicAdd(bad, 1u);
}

// ---- C ABI ------------------------------------------------------------------------------------------
extern "C" int cx_slab4d_begin(cx_ctx* ctx, const int64_t* whole_shape) {
    if (!ctx || !whole_shape) return CX_ERR_INVALID;
    for (int a = 0; a < 4; a++)
        if (whole_shape[a] < 2) { ctx->err = "cx_slab4d_begin: 4-D grid needs at least 2 samples per axis"; return CX_ERR_INVALID; }
    const int64_t plane = whole_shape[1] * whole_shape[2] * whole_shape[3];
    if (plane > (1LL << 27)) {
        ctx->err = "cx_slab4d_begin: a plane of more than 2^27 samples leaves no room for two planes per slab in one extraction";
        return CX_ERR_UNSUPPORTED;
    }
    CX_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->s4) ctx->s4 = new (std::nothrow) cx_state4();
    if (!ctx->s4) return CX_ERR_NOMEM;
    cx_state4* G = ctx->s4;
    if (!G->slab) G->slab = new (std::nothrow) cx_slab4();
    if (!G->slab) return CX_ERR_NOMEM;
    cx_slab4* A = G->slab;
    A->open = true;
    memcpy(A->whole, whole_shape, sizeof(A->whole));
    A->next_i0 = 0; A->nslabs = 0; A->value = 0.0;
    A->nv = 0; A->nt = 0; A->npend = 0; A->pend_t0 = 0;
    G->post_valid = false;       // the assembled result of an earlier finish (and any single post-pass) is gone
    G->post_assembled = false;
    return CX_OK;
}

extern "C" int cx_slab4d_append(cx_ctx* ctx, int64_t i0, int64_t owned_planes, int64_t* out_counts) {
    if (!ctx) return CX_ERR_INVALID;
    cx_state4* G = ctx->s4;
    cx_slab4* A = G ? G->slab : nullptr;
    if (!A || !A->open) { ctx->err = "cx_slab4d_append: no assembly open (cx_slab4d_begin)"; return CX_ERR_STATE; }
    if (!G->extracted) { ctx->err = "cx_slab4d_append: no valid 4-D extraction of the slab (cx_extract4d)"; return CX_ERR_STATE; }
    if (i0 != A->next_i0) {
        ctx->err = "cx_slab4d_append: slabs arrive in axis-0 order, the next one starts at plane " + std::to_string(A->next_i0);
        return CX_ERR_STATE;
    }
    const int64_t n0 = G->n[0];
    if (G->n[1] != A->whole[1] || G->n[2] != A->whole[2] || G->n[3] != A->whole[3] || i0 + n0 > A->whole[0]) {
        ctx->err = "cx_slab4d_append: the slab's grid is not a range of planes of the whole volume";
        return CX_ERR_INVALID;
    }
    if (G->origin[0] != i0 || G->origin[1] || G->origin[2] || G->origin[3]) {
        ctx->err = "cx_slab4d_append: march the slab with cx_set_origin4d(i0, 0, 0, 0)";
        return CX_ERR_INVALID;
    }
    if (!(owned_planes == n0 - 1 || owned_planes == n0) || owned_planes < 1 || (owned_planes == n0) != (i0 + n0 == A->whole[0])) {
        ctx->err = "cx_slab4d_append: every slab but the last carries exactly one halo plane, the last none";
        return CX_ERR_INVALID;
    }
    if (A->nslabs && !(G->value == A->value)) { ctx->err = "cx_slab4d_append: every slab is marched at the same isovalue"; return CX_ERR_INVALID; }
    CX_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t nvl = (uint32_t)G->counts.n_vertices, ntl = (uint32_t)G->counts.n_triangles, np = A->npend;
    const uint64_t m64 = (uint64_t)nvl + np;
    if ((uint64_t)A->nv + m64 >= (1ULL << 31) || (uint64_t)A->nt + ntl >= (1ULL << 31)) {
        ctx->err = "cx_slab4d_append: the assembly would pass 2^31 vertices or tetrahedra (int32 indices)";
        return CX_ERR_UNSUPPORTED;
    }
    const uint32_t m = (uint32_t)m64;
    const uint32_t n1 = (uint32_t)G->n[1], n2 = (uint32_t)G->n[2], n3 = (uint32_t)G->n[3];
    const uint64_t plane = (uint64_t)n1 * n2 * n3;
    const uint32_t nunits = cx_blocks(m, CXS_UNIT);
    const size_t cells = (size_t)CXS_BINS * nunits;
    int rc;
    // every reserve first (the assembly keeps its contents), pointers after
    if ((rc = A->keys.grow_keep(ctx, A->nv, (size_t)A->nv + m + 1))) return rc;
    if ((rc = A->pts.grow_keep(ctx, (size_t)A->nv * 4, ((size_t)A->nv + m + 1) * 4))) return rc;
    if ((rc = A->tets.grow_keep(ctx, (size_t)A->nt * 4, ((size_t)A->nt + ntl + 1) * 4))) return rc;
    if ((rc = A->pend.grow_keep(ctx, np, (size_t)m + 1))) return rc;
    if ((rc = A->ka.grow(ctx, (size_t)m + 64))) return rc;
    if ((rc = A->kb.grow(ctx, (size_t)m + 64))) return rc;
    if ((rc = A->va.grow(ctx, (size_t)m + 64))) return rc;
    if ((rc = A->vb.grow(ctx, (size_t)m + 64))) return rc;
    if ((rc = A->flag.grow(ctx, (size_t)m + 64))) return rc;
    if ((rc = A->pos.grow(ctx, (size_t)m + 64))) return rc;
    if ((rc = A->hist.grow(ctx, cells + 64))) return rc;
    if ((rc = A->offs.grow(ctx, cells + 64))) return rc;
    if ((rc = A->sums.grow(ctx, std::max(cells, (size_t)m) / 1024 + 64))) return rc;
    if ((rc = A->vmap.grow(ctx, (size_t)nvl + 1))) return rc;
    if ((rc = A->resolved.grow(ctx, (size_t)np + 1))) return rc;
    if ((rc = A->cnt.grow(ctx, (size_t)16))) return rc;
    hipStream_t st = ctx->stream;
    uint32_t h[2] = {0, 0};
    CX_HIP(ctx, hipMemsetAsync(A->cnt, 0, 16 * sizeof(uint32_t), st));
    if (m) {
        uint32_t *k = A->ka, *v = A->va, *k2 = A->kb, *v2 = A->vb;
        hipLaunchKernelGGL(cxs_k_pairs, dim3(cx_blocks(m)), dim3(256), 0, st, (const uint32_t*)G->vkeys, nvl, (const uint32_t*)A->pend, np, k, v);
        // as many 8-bit digits as the slab's edge ids have bits
        const uint64_t maxkey = (uint64_t)n0 * plane * 16u - 1u;
        int bits = 0;
        while (bits < 32 && (maxkey >> bits)) bits++;
        for (int shift = 0; shift < bits; shift += 8) {
            hipLaunchKernelGGL(cxs_k_hist, dim3(cx_blocks(nunits, 4)), dim3(256), 0, st, (const uint32_t*)k, m, (uint32_t)shift, nunits, A->hist);
            if ((rc = cx_scan_u32(ctx, A->hist, A->offs, (uint32_t)cells, A->sums, A->cnt + 2))) return rc;
            hipLaunchKernelGGL(cxs_k_scatter, dim3(cx_blocks(nunits, 4)), dim3(256), 0, st, (const uint32_t*)k, (const uint32_t*)v, m, (uint32_t)shift,
                               (const uint32_t*)A->offs, nunits, k2, v2);
            std::swap(k, k2);
            std::swap(v, v2);
        }
        const uint64_t bound = (uint64_t)owned_planes * plane * 16u;
        hipLaunchKernelGGL(cxs_k_mark, dim3(cx_blocks(m)), dim3(256), 0, st, (const uint32_t*)k, m, bound, A->flag, A->cnt);
        if ((rc = cx_scan_u32(ctx, A->flag, A->pos, m, A->sums, A->cnt + 1))) return rc;
        cxs_place P;
        P.A = G->grid; P.n1 = n1; P.n2 = n2; P.n3 = n3;
        P.d3 = cx_fdiv_make(n1 * n2 * n3); P.d2 = cx_fdiv_make(n2 * n3); P.d1 = cx_fdiv_make(n3);
        P.value = G->value; P.i0 = (int)i0;
        P.gofs = (uint64_t)i0 * plane * 16u;
        P.bound = bound; P.nv = nvl; P.base = A->nv;
        hipLaunchKernelGGL(cxs_k_place, dim3(cx_blocks(m)), dim3(256), 0, st, (const uint32_t*)k, (const uint32_t*)v, (const uint32_t*)A->flag,
                           (const uint32_t*)A->pos, m, (const uint32_t*)A->cnt, P, A->keys, A->pts, A->vmap, A->resolved, A->pend);
        CX_HIP(ctx, hipMemcpyAsync(h, A->cnt, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    // the previous slab's references to its halo plane, then this slab's tetrahedra
    const size_t prev = (size_t)(A->nt - A->pend_t0) * 4;
    if (np && prev)
        hipLaunchKernelGGL(cxs_k_resolve, dim3(cx_blocks(prev)), dim3(256), 0, st, A->tets + (size_t)A->pend_t0 * 4, prev, (const int32_t*)A->resolved);
    if (ntl)
        hipLaunchKernelGGL(cxs_k_tets, dim3(cx_blocks((size_t)ntl * 4)), dim3(256), 0, st, (const int32_t*)G->tets, (size_t)ntl * 4,
                           (const int32_t*)A->vmap, A->tets + (size_t)A->nt * 4);
    CX_HIP(ctx, hipGetLastError());
    CX_HIP(ctx, hipStreamSynchronize(st));
    const uint32_t hs = h[0], nnew = h[1];
    A->pend_t0 = A->nt;
    A->nt += ntl;
    A->nv += nnew;
    A->npend = m - hs;
    A->next_i0 = i0 + owned_planes;
    if (!A->nslabs) A->value = G->value;
    A->nslabs++;
    if (out_counts) {
        const int64_t c[8] = {(int64_t)A->nv, (int64_t)A->nt, (int64_t)nnew, (int64_t)ntl, (int64_t)A->npend, (int64_t)A->nslabs, 0, 0};
        memcpy(out_counts, c, sizeof(c));
    }
    return CX_OK;
}

// (cx_slab4d_finish) every slab appended, no reference pending, every index inside the assembly
int cx_slab4_check(cx_ctx* ctx, cx_slab4* A) {
    if (A->next_i0 != A->whole[0]) {
        ctx->err = "cx_slab4d_finish: the slabs cover planes 0 .. " + std::to_string(A->next_i0) + " of " + std::to_string(A->whole[0]);
        return CX_ERR_STATE;
    }
    if (A->npend) {
        ctx->err = "cx_slab4d_finish: " + std::to_string(A->npend) + " halo-plane vertices of the last slab have no slab after them";
        return CX_ERR_STATE;
    }
    if (!A->nt) return CX_OK;
    int rc;
    if ((rc = A->cnt.grow(ctx, (size_t)16))) return rc;
    uint32_t bad = 0;
    const size_t n = (size_t)A->nt * 4;
    CX_HIP(ctx, hipMemsetAsync(A->cnt + 4, 0, sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(cxs_k_bad_refs, dim3(cx_blocks(n)), dim3(256), 0, ctx->stream, (const int32_t*)A->tets, n, (int32_t)A->nv, A->cnt + 4);
    CX_HIP(ctx, hipMemcpyAsync(&bad, A->cnt + 4, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    CX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (bad) {
        ctx->err = "cx_slab4d_finish: " + std::to_string(bad) + " tetrahedron corners refer to no assembled vertex";
        return CX_ERR_STATE;
    }
    return CX_OK;
}

extern "C" int cx_slab4d_download_keys(cx_ctx* ctx, int64_t* keys) {
    if (!ctx || !keys) return CX_ERR_INVALID;
    cx_state4* G = ctx->s4;
    if (!cxp_tets4d(ctx) || !G->post_assembled || !G->slab) { ctx->err = "cx_slab4d_download_keys: run cx_slab4d_finish first"; return CX_ERR_STATE; }
    CX_HIP(ctx, hipSetDevice(ctx->device));
    if (!G->slab->nv) return CX_OK;
    return cx_copy_to_host1(ctx, keys, G->slab->keys, (size_t)G->slab->nv * sizeof(uint64_t));
}
