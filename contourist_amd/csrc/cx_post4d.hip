// cx_post4d.hip -- the 4-D post-pass on the device: cx_postprocess4d*, cx_slab4d_finish, cx_level1_4d_download.
//
// Reference semantics restated (paths relative to the reference checkout, contourist/...): the post-steps of
// GridContour4D.find_tetrahedra
//   bin_times(nbins=100)            pentatopes.py:162-169
//   drop_instant_tetrahedra(1e-7)   pentatopes.py:171-189
//   remove_tiny_simplices(1e-3)     tetrahedral.py:353-375 (called at pentatopes.py:125)
// The state, the parity union-find (cx_dev.h) and the scan are those of the 3-D post-pass (cx_post.h, cx_post.hip).
#include <algorithm>
#include <cstring>

#include "cx_post.h"
#include "cx_state4.h"

// float64 4-D vertex coordinates exactly as the reference interpolates them, with t snapped to its bin
__global__ void cxp_k_vertices4_f64(const float* __restrict__ A, uint32_t n1, uint32_t n2, uint32_t n3, cx_fdiv d3, cx_fdiv d2, cx_fdiv d1,
                                    double value, const uint32_t* __restrict__ vkeys, uint32_t nv, double min_interval, double* pts,
                                    uint32_t* prio, int o0, int o1, int o2, int o3) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const uint32_t key = vkeys[v];
    const uint32_t lin = key >> 4, d = key & 15u;
    uint32_t q[4];
    q[0] = cx_div(lin, d3);
    uint32_t r = lin - q[0] * (n1 * n2 * n3);
    q[1] = cx_div(r, d2);
    r -= q[1] * (n2 * n3);
    q[2] = cx_div(r, d1);
    q[3] = r - q[2] * n3;
    const uint32_t lin2 = lin + ((d & 8u) ? n1 * n2 * n3 : 0u) + ((d & 4u) ? n2 * n3 : 0u) + ((d & 2u) ? n3 : 0u) + (d & 1u);
    const double f0 = (double)A[lin], f1 = (double)A[lin2];
    const bool owner_low = !(f0 > f1);
    const double flow = owner_low ? f0 : f1, fhigh = owner_low ? f1 : f0;
    double ratio = 0.5;
    const double den = 1.0 * (fhigh - flow);
    if (!(fabs(den) <= 1e-8)) ratio = (value - flow) / den;
    const uint32_t db[4] = {(d >> 3) & 1u, (d >> 2) & 1u, (d >> 1) & 1u, d & 1u};
    const int org[4] = {o0, o1, o2, o3};   // (negative) origin of the array in the reference's lattice: the points are interpolated there
    double x[4];
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const double qa = (double)((int)q[a] + org[a]);
        const double low = owner_low ? qa : qa + (double)db[a];
        const double high = owner_low ? qa + (double)db[a] : qa;
        x[a] = low + ratio * (high - low);
    }
    // bin_times: bin = int(t / min_interval); t = bin * min_interval
    x[3] = (double)(long long)(x[3] / min_interval) * min_interval;
#pragma unroll
    for (int a = 0; a < 4; a++) pts[(size_t)v * 4 + a] = x[a];
    prio[v] = key;
}

// the same for points handed over by the caller (linear_interpolate=False: refined on the host with the caller's function,
// tetrahedral.py:488-505): only bin_times and the priority word
__global__ void cxp_k_vertices4_given(const uint32_t* __restrict__ vkeys, uint32_t nv, double min_interval, double* pts, uint32_t* prio) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const double t = pts[(size_t)v * 4 + 3];
    pts[(size_t)v * 4 + 3] = (double)(long long)(t / min_interval) * min_interval;
    prio[v] = vkeys[v];
}

__global__ void cxp_k_and_mask(uint8_t* alive, const uint8_t* keep, uint32_t n) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n && !keep[t]) alive[t] = 0;
}
__global__ void cxp_k_drop_instant(const int32_t* tets, uint8_t* alive, uint32_t nt, const double* pts, double eps) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    double lo = pts[(size_t)tets[(size_t)t * 4] * 4 + 3], hi = lo;
#pragma unroll
    for (int s = 1; s < 4; s++) {
        const double x = pts[(size_t)tets[(size_t)t * 4 + s] * 4 + 3];
        lo = fmin(lo, x); hi = fmax(hi, x);
    }
    alive[t] = ((hi - lo) < eps) ? 0 : 1;
}

__global__ void cxp_k_tiny4(const int32_t* tets, uint8_t* alive, uint32_t nt, const double* pts, double ic0, double ic1, double ic2,
                            double ic3, double eps, u64* parent, const uint32_t* prio, uint8_t* moved) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt || !alive[t]) return;
    const double ic[4] = {ic0, ic1, ic2, ic3};
    uint32_t v[4];
#pragma unroll
    for (int s = 0; s < 4; s++) v[s] = (uint32_t)tets[(size_t)t * 4 + s];
    double worst = 0.0;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        double lo = pts[(size_t)v[0] * 4 + a], hi = lo;
#pragma unroll
        for (int s = 1; s < 4; s++) {
            const double x = pts[(size_t)v[s] * 4 + a];
            lo = fmin(lo, x); hi = fmax(hi, x);
        }
        worst = fmax(worst, (hi - lo) * ic[a]);
    }
    if (worst < eps) {
        alive[t] = 0;
#pragma unroll
        for (int s = 1; s < 4; s++) cxp_union(parent, prio, v[0], v[s], 0);
#pragma unroll
        for (int s = 0; s < 4; s++) moved[v[s]] = 1;
    }
}
__global__ void cxp_k_move4(double* pts, const u64* parent, const uint8_t* moved, uint32_t nv) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv || !moved[v]) return;
    uint32_t par;
    const uint32_t r = cxp_find(parent, v, par);
    if (r == v) return;
#pragma unroll
    for (int a = 0; a < 4; a++) pts[(size_t)v * 4 + a] = pts[(size_t)r * 4 + a];
}
__global__ void cxp_k_compact_tets(const int32_t* tets, const uint8_t* alive, const uint32_t* tnew, uint32_t nt, int32_t* out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt || !alive[t]) return;
#pragma unroll
    for (int s = 0; s < 4; s++) out[(size_t)tnew[t] * 4 + s] = tets[(size_t)t * 4 + s];
}

extern "C" int cx_postprocess4d_points(cx_ctx* ctx, int32_t nbins, const double* points_xyzt, int64_t* out_counts);
extern "C" int cx_postprocess4d(cx_ctx* ctx, int32_t nbins, int64_t* out_counts) {
    return cx_postprocess4d_points(ctx, nbins, nullptr, out_counts);
}
// drop_instant, the seeded selection's mask (keep, or null), the tiny collapse and the compaction of the survivors into S->tri_out, on the
// points and priorities already in S->pts / S->prio (nv, nt > 0).  counts[2], [3]: tetrahedra after drop_instant / the tiny collapse
static int cxp_post4_tets(cx_ctx* ctx, cx_post_state* S, const int32_t* tets, uint32_t nv, uint32_t nt, const double corner[4], const uint8_t* keep,
                          int64_t* counts, uint32_t* nt2_out) {
    int rc;
    hipStream_t st = ctx->stream;
    double* pts = S->pts.as<double>();
    uint32_t* prio = S->prio.as<uint32_t>();
    uint8_t* moved = S->rep.as<uint8_t>();
    uint8_t* alive = S->alive.as<uint8_t>();
    u64* parent = S->parent.as<u64>();
    cxp_tables_taken(S);    // (the 3-D orientation's tables lived in S->parent)
    uint32_t* misc = S->misc.as<uint32_t>();
    hipLaunchKernelGGL(cxp_k_drop_instant, dim3(cx_blocks(nt)), dim3(256), 0, st, tets, alive, nt, pts, 1e-7);
    // cx_select_seeded4d: only the tetrahedra of the selected components exist
    if (keep) hipLaunchKernelGGL(cxp_k_and_mask, dim3(cx_blocks(nt)), dim3(256), 0, st, alive, keep, nt);
    CX_HIP(ctx, hipMemsetAsync(misc + CXP_M_WELD, 0, 2 * sizeof(uint32_t), st));
    cxp_count_alive(st, alive, nt, misc + CXP_M_WELD);
    cxp_iota64(st, parent, nv);
    CX_HIP(ctx, hipMemsetAsync(moved, 0, nv, st));
    hipLaunchKernelGGL(cxp_k_tiny4, dim3(cx_blocks(nt)), dim3(256), 0, st, tets, alive, nt, pts, 1.0 / corner[0], 1.0 / corner[1],
                       1.0 / corner[2], 1.0 / corner[3], 1e-3, parent, prio, moved);
    hipLaunchKernelGGL(cxp_k_move4, dim3(cx_blocks(nv)), dim3(256), 0, st, pts, parent, moved, nv);
    cxp_count_alive(st, alive, nt, misc + CXP_M_TINY);
    uint32_t* tflag = S->flags.as<uint32_t>();
    uint32_t* tnew = S->scan.as<uint32_t>();
    cxp_alive_u32(st, alive, nt, tflag);
    if ((rc = cxp_scan(ctx, S, tflag, tnew, nt, misc + CXP_M_TOTAL1))) return rc;
    uint32_t h[3];
    CX_HIP(ctx, hipMemcpyAsync(h, misc + CXP_M_WELD, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    CX_HIP(ctx, hipMemcpyAsync(h + 2, misc + CXP_M_TOTAL1, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    CX_HIP(ctx, hipStreamSynchronize(st));
    counts[2] = h[0]; counts[3] = h[1];
    const uint32_t nt2 = h[2];
    if ((rc = S->tri_out.grow(ctx, (size_t)(nt2 + 1) * 4 * sizeof(int32_t)))) return rc;
    hipLaunchKernelGGL(cxp_k_compact_tets, dim3(cx_blocks(nt)), dim3(256), 0, st, tets, alive, tnew, nt, S->tri_out.as<int32_t>());
    CX_HIP(ctx, hipGetLastError());
    *nt2_out = nt2;
    return CX_OK;
}
static int cxp_reserve4(cx_ctx* ctx, cx_post_state* S, uint32_t nv, uint32_t nt) {
    int rc;
    if ((rc = S->pts.grow(ctx, (size_t)(nv + 1) * 4 * sizeof(double)))) return rc;
    if ((rc = S->prio.grow(ctx, (size_t)(nv + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = S->rep.grow(ctx, (size_t)nv + 16))) return rc;
    if ((rc = S->alive.grow(ctx, (size_t)nt + 16))) return rc;
    if ((rc = S->parent.grow(ctx, (size_t)(nv + 1) * sizeof(u64)))) return rc;
    if ((rc = S->flags.grow(ctx, (size_t)(nt + 16) * sizeof(uint32_t)))) return rc;
    if ((rc = S->scan.grow(ctx, (size_t)(nt + 16) * sizeof(uint32_t)))) return rc;
    return CX_OK;
}
extern "C" int cx_postprocess4d_points(cx_ctx* ctx, int32_t nbins, const double* points_xyzt, int64_t* out_counts) {
    if (!ctx || nbins <= 0) return CX_ERR_INVALID;
    cx_state4* G = ctx->s4;
    if (!G || !G->extracted) { ctx->err = "cx_postprocess4d: no valid 4-D extraction"; return CX_ERR_STATE; }
    if (G->slab && G->slab->open) { ctx->err = "cx_postprocess4d: a slab assembly is open (cx_slab4d_finish post-processes it)"; return CX_ERR_STATE; }
    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_post_state* S;
    int rc = cxp_state(ctx, &S);
    if (rc) return rc;
    const uint32_t nv = (uint32_t)G->counts.n_vertices, nt = (uint32_t)G->counts.n_triangles;
    hipStream_t st = ctx->stream;
    cxp_begin(ctx, S);
    if ((rc = cxp_reserve4(ctx, S, nv, nt))) return rc;
    double* pts = S->pts.as<double>();
    uint32_t* prio = S->prio.as<uint32_t>();
    int64_t counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t nt2 = 0;
    G->post_assembled = false;
    if (nv && nt) {
        const uint32_t n1 = (uint32_t)G->n[1], n2 = (uint32_t)G->n[2], n3 = (uint32_t)G->n[3];
        // an array with a rim of samples around the reference's grid (negative origin, cx_set_origin4d): the reference's own
        // corner and lattice (scales of the tiny collapse, bin width, coordinates)
        int org[4];
        double corner[4];
        for (int a = 0; a < 4; a++) {
            org[a] = (G->origin[a] < 0) ? (int)G->origin[a] : 0;
            corner[a] = (double)(G->n[a] - 1 + 2 * org[a]);
        }
        const double min_interval = corner[3] * (1.0 / (double)nbins);
        if (points_xyzt) {   // the caller's points (in the reference's lattice), one per Level-0 vertex
            CX_HIP(ctx, hipMemcpyAsync(pts, points_xyzt, (size_t)nv * 4 * sizeof(double), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(cxp_k_vertices4_given, dim3(cx_blocks(nv)), dim3(256), 0, st, G->vkeys, nv, min_interval, pts, prio);
        } else
        hipLaunchKernelGGL(cxp_k_vertices4_f64, dim3(cx_blocks(nv)), dim3(256), 0, st, G->grid, n1, n2, n3, cx_fdiv_make(n1 * n2 * n3),
                           cx_fdiv_make(n2 * n3), cx_fdiv_make(n3), G->value, G->vkeys, nv, min_interval, pts, prio, org[0], org[1], org[2], org[3]);
        if ((rc = cxp_post4_tets(ctx, S, G->tets, nv, nt, corner, G->keep_valid ? (const uint8_t*)G->tet_keep : nullptr, counts, &nt2))) return rc;
    }
    S->nv_out = nv; S->nt_out = nt2;
    counts[0] = nv; counts[1] = nt2;
    return cxp_publish(ctx, S, cxp_record::TETS4D, cxp_record::GRID, counts, out_counts);
}

// ---- the same post-steps on a slab assembly (cx_slab4d.hip): the points were interpolated per slab in the whole volume's lattice, the
// priority of a vertex is its index (the assembly is in ascending global edge id, the order the edge ids give a single extraction)
__global__ void cxp_k_bin_times_iota(double* pts, uint32_t nv, double min_interval, uint32_t* prio) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const double t = pts[(size_t)v * 4 + 3];
    pts[(size_t)v * 4 + 3] = (double)(long long)(t / min_interval) * min_interval;
    prio[v] = v;
}
int cx_slab4_check(cx_ctx* ctx, cx_slab4* A);
extern "C" int cx_slab4d_finish(cx_ctx* ctx, int32_t nbins, int64_t* out_counts) {
    if (!ctx || nbins <= 0) return CX_ERR_INVALID;
    cx_state4* G = ctx->s4;
    cx_slab4* A = G ? G->slab : nullptr;
    if (!A || !A->open) { ctx->err = "cx_slab4d_finish: no assembly open (cx_slab4d_begin)"; return CX_ERR_STATE; }
    CX_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = cx_slab4_check(ctx, A))) return rc;
    cx_post_state* S;
    if ((rc = cxp_state(ctx, &S))) return rc;
    const uint32_t nv = A->nv, nt = A->nt;
    hipStream_t st = ctx->stream;
    cxp_begin(ctx, S);
    if ((rc = cxp_reserve4(ctx, S, nv, nt))) return rc;
    int64_t counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t nt2 = 0;
    if (nv && nt) {
        double corner[4];
        for (int a = 0; a < 4; a++) corner[a] = (double)(A->whole[a] - 1);
        const double min_interval = corner[3] * (1.0 / (double)nbins);
        CX_HIP(ctx, hipMemcpyAsync(S->pts.get(), A->pts, (size_t)nv * 4 * sizeof(double), hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(cxp_k_bin_times_iota, dim3(cx_blocks(nv)), dim3(256), 0, st, S->pts.as<double>(), nv, min_interval, S->prio.as<uint32_t>());
        if ((rc = cxp_post4_tets(ctx, S, A->tets, nv, nt, corner, nullptr, counts, &nt2))) return rc;
    }
    S->nv_out = nv; S->nt_out = nt2;
    counts[0] = nv; counts[1] = nt2;
    A->open = false;
    G->post_assembled = true;
    return cxp_publish(ctx, S, cxp_record::TETS4D, cxp_record::GRID, counts, out_counts);
}

extern "C" int cx_level1_4d_download(cx_ctx* ctx, double* points_xyzt, int32_t* tets) {
    if (!ctx) return CX_ERR_INVALID;
    if (!cxp_tets4d(ctx)) { ctx->err = "cx_level1_4d_download: run cx_postprocess4d first"; return CX_ERR_STATE; }
    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_post_state* S = ctx->post;
    void* d[2] = {(points_xyzt && S->nv_out) ? (void*)points_xyzt : nullptr, (tets && S->nt_out) ? (void*)tets : nullptr};
    const void* sp[2] = {S->pts.get(), S->tri_out.get()};
    const size_t nb[2] = {(size_t)S->nv_out * 4 * sizeof(double), (size_t)S->nt_out * 4 * sizeof(int32_t)};
    return cx_copy_to_host(ctx, 2, d, sp, nb);
}
