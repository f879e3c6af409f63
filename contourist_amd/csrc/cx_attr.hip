// cx_attr.hip -- vertex attributes of the 3-D isosurface: normals from the field's gradient and a second grid sampled at the
// vertices (include/contourist_hip.h, "vertex attributes").
//
// A vertex is a crossing of the lattice edge a -> b at fraction r.  The gradient G of the resident sample array at a lattice point
// follows numpy.gradient with its defaults: (f[p+e] - f[p-e]) / 2 inside, the one-sided first difference on the rim of the marched
// array.  Both are ONE difference of two samples times 0.5 or 1: the neighbour indices are clamped to the array and the scale
// follows from how many of them moved.  g = G(a) + r (G(b) - G(a)), divided per axis by the world spacing when one is handed
// over, n = s g / |g| and (0,0,0) when |g| == 0.
//   Level 0: a = q, b = q + d, r = the record's fp32 fraction, fp32, s = +1, float4 {nx, ny, nz, |g|} per vertex record.
//   Level 1: a / b / r = low point / high point / ratio exactly as cxp_k_vertices_f64 (cx_post.hip) computes them, float64,
//            s = -1 where the orientation step reversed the vertex's component.
// No atomics, no adjacency: every lane owns one vertex and writes one record.
//
// Curvature is the same kind of gather with a wider stencil.  The Hessian H of a lattice point is taken at the
// centre c = clamp(p, 1, n-2) per axis (a rim point takes the Hessian of its nearest interior point; every axis needs 3 samples):
//   H_aa = (f[c+e_a] - f[c]) - (f[c] - f[c-e_a]),   H_ab = ((f[c+e_a+e_b] - f[c+e_a-e_b]) - (f[c-e_a+e_b] - f[c-e_a-e_b])) * 0.25
// 19 samples, of which the 6 axis neighbours are the gradient's own inside the array.  g and H are lerped along the edge like the
// normal's g, divided by the world spacing (g_i / delta_i, H_ij / (delta_i delta_j)), and with n = g / |g|
//   mean = (tr H - n'Hn) / (2 |g|),   gauss = n' adj(H) n / |g|^2,   k1, k2 = mean +- sqrt(max(mean^2 - gauss, 0)),   k1 >= k2
// (a sphere whose field grows outwards: mean = +1/R, gauss = 1/R^2); four zeros when |g| == 0.
//   Level 0: fp32, float4 {mean, gauss, k1, k2} per vertex record.
//   Level 1: float64, double[4]; where the orientation step reversed the component, mean, k1, k2 change sign and k1, k2 swap.
#include <cmath>
#include <string>

#include "cx_ctx.h"

typedef float cxa_v4f __attribute__((ext_vector_type(4)));

struct cxa_dims {
    uint32_t n0, n1, n2, plane;
    cx_fdiv dplane, drow;
};

// offsets (in samples) to the clamped lower / upper neighbour of coordinate c on an axis of n samples with the given stride, and the
// scale of the difference: 0.5 when both neighbours exist, 1 on the rim (n >= 2, so one of them always does)
__device__ __forceinline__ void cxa_axis(uint32_t c, uint32_t n, uint32_t stride, uint32_t& lo, uint32_t& hi, bool& both) {
    lo = c ? stride : 0u;
    hi = (c + 1u < n) ? stride : 0u;
    both = lo != 0u && hi != 0u;
}

// fp32 gradient at lattice point (i, j, k) = sample `lin`: six loads, three in the point's own plane (the k neighbours share its
// 128-byte line or the next one, the j neighbours lie one row away); one rounding per component (the difference; the scale is exact)
template <int DT>
__device__ __forceinline__ void cxa_grad32(const cx_grid_ref& A, const cxa_dims& D, uint32_t lin, uint32_t i, uint32_t j, uint32_t k, float& gx,
                                           float& gy, float& gz) {
    uint32_t lo, hi;
    bool both;
    cxa_axis(k, D.n2, 1u, lo, hi, both);
    gz = (cx_sample<DT>(A, lin + hi) - cx_sample<DT>(A, lin - lo)) * (both ? 0.5f : 1.0f);
    cxa_axis(j, D.n1, D.n2, lo, hi, both);
    gy = (cx_sample<DT>(A, lin + hi) - cx_sample<DT>(A, lin - lo)) * (both ? 0.5f : 1.0f);
    cxa_axis(i, D.n0, D.plane, lo, hi, both);
    gx = (cx_sample<DT>(A, lin + hi) - cx_sample<DT>(A, lin - lo)) * (both ? 0.5f : 1.0f);
}

// ---- Level 0: one lane per vertex record, in record order (the 64 vertices of a wave sit in neighbouring cells, so the rows their
// twelve samples come from are a handful of lines shared by the whole wave).  Output: one nontemporal 16-byte store per lane.
template <int DT, bool WORLD>
__global__ __launch_bounds__(256) void cx_k_vertex_normals(const cx_grid_ref A, const cx_vrec* __restrict__ recs, cxa_v4f* __restrict__ out, uint32_t nv,
                                                           cxa_dims D, float d0, float d1, float d2) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= nv) return;
    const cx_vrec rec = recs[v];
    const uint32_t lin = rec.x >> 3, d = rec.x & 7u;
    const float t = __uint_as_float(rec.y);
    const uint32_t i = cx_div(lin, D.dplane);
    const uint32_t rem = lin - i * D.plane;
    const uint32_t j = cx_div(rem, D.drow);
    const uint32_t k = rem - j * D.n2;
    const uint32_t di = (d >> 2) & 1u, dj = (d >> 1) & 1u, dk = d & 1u;
    cxa_v4f o = {0.0f, 0.0f, 0.0f, 0.0f};
    if (i + di < D.n0 && j + dj < D.n1 && k + dk < D.n2) {      // (always, for a record of the march: nothing is read outside the array)
        float ax, ay, az, bx, by, bz;
        cxa_grad32<DT>(A, D, lin, i, j, k, ax, ay, az);
        cxa_grad32<DT>(A, D, lin + di * D.plane + dj * D.n2 + dk, i + di, j + dj, k + dk, bx, by, bz);
        float gx = fmaf(t, bx - ax, ax), gy = fmaf(t, by - ay, ay), gz = fmaf(t, bz - az, az);
        if (WORLD) { gx /= d0; gy /= d1; gz /= d2; }
        // scaled by a power of two (exact) so that the squares neither overflow nor vanish
        const float m = fmaxf(fabsf(gx), fmaxf(fabsf(gy), fabsf(gz)));
        if (m > 0.0f && m <= 3.0e38f) {
            int e;
            (void)frexpf(m, &e);
            const float sx = ldexpf(gx, -e), sy = ldexpf(gy, -e), sz = ldexpf(gz, -e);
            const float len = sqrtf(sx * sx + sy * sy + sz * sz);
            const float inv = 1.0f / len;
            o = cxa_v4f{sx * inv, sy * inv, sz * inv, ldexpf(len, e)};
        }
    }
    __builtin_nontemporal_store(o, out + v);
}

// ---- curvature, Level 0 ----------------------------------------------------------------------------------------------------------------
// The 19 samples of the Hessian's stencil around a centre, by name (no array: nothing here is indexed at run time).  c = the centre;
// xm / xp = centre -+ e_0 (a plane away), ym / yp = -+ e_1 (a row away), zm / zp = -+ e_2; xy_pm = centre + e_0 - e_1 and so on.
struct cxa_stencil {
    float c, xm, xp, ym, yp, zm, zp;
    float xy_mm, xy_mp, xy_pm, xy_pp, xz_mm, xz_mp, xz_pm, xz_pp, yz_mm, yz_mp, yz_pm, yz_pp;
};
// all 19 loads, issued before anything uses one of them; `lin` is a centre with every neighbour inside the array
template <int DT>
__device__ __forceinline__ cxa_stencil cxa_load_stencil(const cx_grid_ref& A, uint32_t lin, uint32_t plane, uint32_t row) {
    cxa_stencil S;
    S.c = cx_sample<DT>(A, lin);
    S.zm = cx_sample<DT>(A, lin - 1u);                 S.zp = cx_sample<DT>(A, lin + 1u);
    S.ym = cx_sample<DT>(A, lin - row);                S.yp = cx_sample<DT>(A, lin + row);
    S.yz_mm = cx_sample<DT>(A, lin - row - 1u);        S.yz_mp = cx_sample<DT>(A, lin - row + 1u);
    S.yz_pm = cx_sample<DT>(A, lin + row - 1u);        S.yz_pp = cx_sample<DT>(A, lin + row + 1u);
    S.xm = cx_sample<DT>(A, lin - plane);              S.xp = cx_sample<DT>(A, lin + plane);
    S.xz_mm = cx_sample<DT>(A, lin - plane - 1u);      S.xz_mp = cx_sample<DT>(A, lin - plane + 1u);
    S.xz_pm = cx_sample<DT>(A, lin + plane - 1u);      S.xz_pp = cx_sample<DT>(A, lin + plane + 1u);
    S.xy_mm = cx_sample<DT>(A, lin - plane - row);     S.xy_mp = cx_sample<DT>(A, lin - plane + row);
    S.xy_pm = cx_sample<DT>(A, lin + plane - row);     S.xy_pp = cx_sample<DT>(A, lin + plane + row);
    return S;
}
// gradient and Hessian of one lattice point: {gx, gy, gz} and {H00, H11, H22, H01, H02, H12}
struct cxa_jet32 {
    float gx, gy, gz, h00, h11, h22, h01, h02, h12;
};
// the Hessian in the order of evaluation the definition fixes: every difference of two samples is one rounding, the 0.25 is exact
__device__ __forceinline__ void cxa_hessian32(const cxa_stencil& S, cxa_jet32& J) {
    J.h00 = (S.xp - S.c) - (S.c - S.xm);
    J.h11 = (S.yp - S.c) - (S.c - S.ym);
    J.h22 = (S.zp - S.c) - (S.c - S.zm);
    J.h01 = ((S.xy_pp - S.xy_pm) - (S.xy_mp - S.xy_mm)) * 0.25f;
    J.h02 = ((S.xz_pp - S.xz_pm) - (S.xz_mp - S.xz_mm)) * 0.25f;
    J.h12 = ((S.yz_pp - S.yz_pm) - (S.yz_mp - S.yz_mm)) * 0.25f;
}
// a point with all its neighbours: plain strides, the gradient from the stencil's own axis samples (the bits of cxa_grad32: the
// same difference times 0.5)
template <int DT>
__device__ __forceinline__ cxa_jet32 cxa_jet_inside(const cx_grid_ref& A, const cxa_dims& D, uint32_t lin) {
    const cxa_stencil S = cxa_load_stencil<DT>(A, lin, D.plane, D.n2);
    cxa_jet32 J;
    J.gx = (S.xp - S.xm) * 0.5f; J.gy = (S.yp - S.ym) * 0.5f; J.gz = (S.zp - S.zm) * 0.5f;
    cxa_hessian32(S, J);
    return J;
}
// any point of an array with at least 3 samples per axis: the stencil around the clamped centre, the gradient by 9e's rule at the point
template <int DT>
__device__ __forceinline__ cxa_jet32 cxa_jet_clamped(const cx_grid_ref& A, const cxa_dims& D, uint32_t lin, uint32_t i, uint32_t j, uint32_t k) {
    const uint32_t ci = min(max(i, 1u), D.n0 - 2u), cj = min(max(j, 1u), D.n1 - 2u), ck = min(max(k, 1u), D.n2 - 2u);
    const cxa_stencil S = cxa_load_stencil<DT>(A, ci * D.plane + cj * D.n2 + ck, D.plane, D.n2);
    cxa_jet32 J;
    cxa_grad32<DT>(A, D, lin, i, j, k, J.gx, J.gy, J.gz);
    cxa_hessian32(S, J);
    return J;
}

// One lane per vertex record, as cx_k_vertex_normals.  A wave whose lanes all have both end points inside the array (every neighbour
// exists) takes the fast path: 2 x 19 loads at plain strides.  Any other wave (the vertices of a wave sit in neighbouring cells, so
// these are the waves along the array's rim) takes the clamped one, which gives an interior lane the same bits.  The samples the two
// stencils have in common depend on the lane's own d; picking them out would take a chain of selects per sample or an array indexed
// at run time, so they are asked for twice and the second request hits the line the first one brought in.
template <int DT, bool WORLD>
__global__ __launch_bounds__(256) void cx_k_vertex_curvature(const cx_grid_ref A, const cx_vrec* __restrict__ recs, cxa_v4f* __restrict__ out, uint32_t nv,
                                                             cxa_dims D, float d0, float d1, float d2) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= nv) return;
    const cx_vrec rec = recs[v];
    const uint32_t lin = rec.x >> 3, d = rec.x & 7u;
    const float t = __uint_as_float(rec.y);
    const uint32_t i = cx_div(lin, D.dplane);
    const uint32_t rem = lin - i * D.plane;
    const uint32_t j = cx_div(rem, D.drow);
    const uint32_t k = rem - j * D.n2;
    const uint32_t di = (d >> 2) & 1u, dj = (d >> 1) & 1u, dk = d & 1u;
    cxa_v4f o = {0.0f, 0.0f, 0.0f, 0.0f};
    const bool in_array = i + di < D.n0 && j + dj < D.n1 && k + dk < D.n2;      // (always, for a record of the march: nothing is read outside the array)
    const bool inside = i >= 1u && j >= 1u && k >= 1u && i + di + 1u < D.n0 && j + dj + 1u < D.n1 && k + dk + 1u < D.n2;
    const uint32_t lin2 = lin + di * D.plane + dj * D.n2 + dk;
    cxa_jet32 Ja, Jb;
    if (__all(inside)) {
        Ja = cxa_jet_inside<DT>(A, D, lin);
        Jb = cxa_jet_inside<DT>(A, D, lin2);
    } else if (in_array) {
        Ja = cxa_jet_clamped<DT>(A, D, lin, i, j, k);
        Jb = cxa_jet_clamped<DT>(A, D, lin2, i + di, j + dj, k + dk);
    } else {
        __builtin_nontemporal_store(o, out + v);
        return;
    }
    float gx = fmaf(t, Jb.gx - Ja.gx, Ja.gx), gy = fmaf(t, Jb.gy - Ja.gy, Ja.gy), gz = fmaf(t, Jb.gz - Ja.gz, Ja.gz);
    float h00 = fmaf(t, Jb.h00 - Ja.h00, Ja.h00), h11 = fmaf(t, Jb.h11 - Ja.h11, Ja.h11), h22 = fmaf(t, Jb.h22 - Ja.h22, Ja.h22);
    float h01 = fmaf(t, Jb.h01 - Ja.h01, Ja.h01), h02 = fmaf(t, Jb.h02 - Ja.h02, Ja.h02), h12 = fmaf(t, Jb.h12 - Ja.h12, Ja.h12);
    if (WORLD) {
        gx /= d0; gy /= d1; gz /= d2;
        h00 /= d0 * d0; h11 /= d1 * d1; h22 /= d2 * d2;
        h01 /= d0 * d1; h02 /= d0 * d2; h12 /= d1 * d2;
    }
    // scaled by a power of two (exact) so that the squares neither overflow nor vanish
    const float m = fmaxf(fabsf(gx), fmaxf(fabsf(gy), fabsf(gz)));
    if (m > 0.0f && m <= 3.0e38f) {
        int e;
        (void)frexpf(m, &e);
        const float sx = ldexpf(gx, -e), sy = ldexpf(gy, -e), sz = ldexpf(gz, -e);
        const float len = sqrtf(sx * sx + sy * sy + sz * sz);
        const float inv = 1.0f / len;
        const float nx = sx * inv, ny = sy * inv, nz = sz * inv;
        const float glen = ldexpf(len, e);
        const float nHn = nx * (h00 * nx + h01 * ny + h02 * nz) + ny * (h01 * nx + h11 * ny + h12 * nz) + nz * (h02 * nx + h12 * ny + h22 * nz);
        const float mean = ((h00 + h11 + h22) - nHn) / (2.0f * glen);
        // adj(H), symmetric
        const float a00 = h11 * h22 - h12 * h12, a11 = h00 * h22 - h02 * h02, a22 = h00 * h11 - h01 * h01;
        const float a01 = h02 * h12 - h01 * h22, a02 = h01 * h12 - h02 * h11, a12 = h01 * h02 - h00 * h12;
        const float nAn = nx * (a00 * nx + a01 * ny + a02 * nz) + ny * (a01 * nx + a11 * ny + a12 * nz) + nz * (a02 * nx + a12 * ny + a22 * nz);
        const float gauss = nAn / glen / glen;             // (two divisions: |g|^2 may overflow where |g| does not)
        const float root = sqrtf(fmaxf(mean * mean - gauss, 0.0f));
        o = cxa_v4f{mean, gauss, mean + root, mean - root};
    }
    __builtin_nontemporal_store(o, out + v);
}

// a second grid B at the same places: B(q) + t (B(q + d) - B(q)), two samples per vertex
template <int DTB>
__global__ __launch_bounds__(256) void cx_k_vertex_sample(const cx_grid_ref B, const cx_vrec* __restrict__ recs, float* __restrict__ out, uint32_t nv,
                                                          uint32_t n2, uint32_t plane, uint32_t nsamples) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= nv) return;
    const cx_vrec rec = recs[v];
    const uint32_t lin = rec.x >> 3, d = rec.x & 7u;
    const uint32_t lin2 = lin + ((d & 4u) ? plane : 0u) + ((d & 2u) ? n2 : 0u) + (d & 1u);
    float r = 0.0f;
    if (lin2 < nsamples) {
        const float b0 = cx_sample<DTB>(B, lin), b1 = cx_sample<DTB>(B, lin2);
        r = fmaf(__uint_as_float(rec.y), b1 - b0, b0);
    }
    __builtin_nontemporal_store(r, out + v);
}

// ---- Level 1: float64, one lane per Level-1 vertex, driven by the key array.  Not hot: clarity over tricks.
// The edge of every vertex once: {sample index of the low point a, of the high point b, ratio} as cxp_k_vertices_f64 has them
struct cxa_edge1 {
    uint32_t a, b;
    double r;
};
template <int DT>
__device__ __forceinline__ double cxa_sample64(const cx_grid_ref& A, const double* __restrict__ A64, uint32_t lin) {
    return A64 ? A64[lin] : (double)cx_sample<DT>(A, lin);
}
template <int DT>
__global__ void cx_k_level1_edges(const cx_grid_ref A, const double* __restrict__ A64, const uint32_t* __restrict__ keys, uint32_t nv, uint32_t n2,
                                  uint32_t plane, uint32_t nsamples, double value, cxa_edge1* __restrict__ out) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const uint32_t key = keys[v];
    const uint32_t lin = key >> 3, d = key & 7u;
    const uint32_t lin2 = lin + ((d & 4u) ? plane : 0u) + ((d & 2u) ? n2 : 0u) + (d & 1u);
    cxa_edge1 e = {0u, 0u, 0.5};
    if (lin2 < nsamples) {
        const double f0 = cxa_sample64<DT>(A, A64, lin), f1 = cxa_sample64<DT>(A, A64, lin2);
        const bool owner_low = !(f0 > f1);             // the reference swaps when flow > fhigh
        const double flow = owner_low ? f0 : f1, fhigh = owner_low ? f1 : f0;
        const double den = 1.0 * (fhigh - flow);
        if (!(fabs(den) <= 1e-8)) e.r = (value - flow) / den;
        e.a = owner_low ? lin : lin2;
        e.b = owner_low ? lin2 : lin;
    }
    out[v] = e;
}
template <int DT>
__device__ __forceinline__ void cxa_grad64(const cx_grid_ref& A, const double* __restrict__ A64, const cxa_dims& D, uint32_t lin, double g[3]) {
    const uint32_t i = cx_div(lin, D.dplane);
    const uint32_t rem = lin - i * D.plane;
    const uint32_t j = cx_div(rem, D.drow);
    const uint32_t k = rem - j * D.n2;
    uint32_t lo, hi;
    bool both;
    cxa_axis(i, D.n0, D.plane, lo, hi, both);
    g[0] = (cxa_sample64<DT>(A, A64, lin + hi) - cxa_sample64<DT>(A, A64, lin - lo)) * (both ? 0.5 : 1.0);
    cxa_axis(j, D.n1, D.n2, lo, hi, both);
    g[1] = (cxa_sample64<DT>(A, A64, lin + hi) - cxa_sample64<DT>(A, A64, lin - lo)) * (both ? 0.5 : 1.0);
    cxa_axis(k, D.n2, 1u, lo, hi, both);
    g[2] = (cxa_sample64<DT>(A, A64, lin + hi) - cxa_sample64<DT>(A, A64, lin - lo)) * (both ? 0.5 : 1.0);
}
template <int DT>
__global__ void cx_k_level1_normals(const cx_grid_ref A, const double* __restrict__ A64, const cxa_edge1* __restrict__ edges,
                                    const uint8_t* __restrict__ vflip, uint32_t nv, cxa_dims D, int world, double d0, double d1, double d2,
                                    double* __restrict__ out) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const cxa_edge1 e = edges[v];
    double ga[3], gb[3], g[3];
    cxa_grad64<DT>(A, A64, D, e.a, ga);
    cxa_grad64<DT>(A, A64, D, e.b, gb);
#pragma unroll
    for (int a = 0; a < 3; a++) g[a] = ga[a] + e.r * (gb[a] - ga[a]);
    if (world) { g[0] /= d0; g[1] /= d1; g[2] /= d2; }
    const double m = fmax(fabs(g[0]), fmax(fabs(g[1]), fabs(g[2])));
    double n[3] = {0.0, 0.0, 0.0};
    if (m > 0.0 && m <= 1.7e308) {
        int ex;
        (void)frexp(m, &ex);
        const double sx = ldexp(g[0], -ex), sy = ldexp(g[1], -ex), sz = ldexp(g[2], -ex);
        const double len = sqrt(sx * sx + sy * sy + sz * sz);
        const double s = vflip[v] ? -1.0 : 1.0;
        n[0] = s * sx / len; n[1] = s * sy / len; n[2] = s * sz / len;
    }
#pragma unroll
    for (int a = 0; a < 3; a++) out[(size_t)v * 3 + a] = n[a];
}
// curvature at Level 1: gradient and Hessian {H00, H11, H22, H01, H02, H12} of both end points in float64, the definition line by line
template <int DT>
__device__ __forceinline__ void cxa_hess64(const cx_grid_ref& A, const double* __restrict__ A64, const cxa_dims& D, uint32_t lin, double h[6]) {
    const uint32_t i = cx_div(lin, D.dplane);
    const uint32_t rem = lin - i * D.plane;
    const uint32_t j = cx_div(rem, D.drow);
    const uint32_t k = rem - j * D.n2;
    const uint32_t ci = min(max(i, 1u), D.n0 - 2u), cj = min(max(j, 1u), D.n1 - 2u), ck = min(max(k, 1u), D.n2 - 2u);
    const uint32_t c = ci * D.plane + cj * D.n2 + ck, e0 = D.plane, e1 = D.n2, e2 = 1u;
    const double fc = cxa_sample64<DT>(A, A64, c);
#define CXA_F(off) cxa_sample64<DT>(A, A64, c off)
    h[0] = (CXA_F(+ e0) - fc) - (fc - CXA_F(- e0));
    h[1] = (CXA_F(+ e1) - fc) - (fc - CXA_F(- e1));
    h[2] = (CXA_F(+ e2) - fc) - (fc - CXA_F(- e2));
    h[3] = ((CXA_F(+ e0 + e1) - CXA_F(+ e0 - e1)) - (CXA_F(- e0 + e1) - CXA_F(- e0 - e1))) * 0.25;
    h[4] = ((CXA_F(+ e0 + e2) - CXA_F(+ e0 - e2)) - (CXA_F(- e0 + e2) - CXA_F(- e0 - e2))) * 0.25;
    h[5] = ((CXA_F(+ e1 + e2) - CXA_F(+ e1 - e2)) - (CXA_F(- e1 + e2) - CXA_F(- e1 - e2))) * 0.25;
#undef CXA_F
}
template <int DT>
__global__ __launch_bounds__(256) void cx_k_level1_curvature(const cx_grid_ref A, const double* __restrict__ A64, const cxa_edge1* __restrict__ edges,
                                                             const uint8_t* __restrict__ vflip, uint32_t nv, uint32_t nsamples, cxa_dims D, int world,
                                                             double d0, double d1, double d2, double* __restrict__ out) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const cxa_edge1 e = edges[v];
    double mean = 0.0, gauss = 0.0, k1 = 0.0, k2 = 0.0;
    if (e.a < nsamples && e.b < nsamples) {
        double ga[3], gb[3], ha[6], hb[6], g[3], h[6];
        cxa_grad64<DT>(A, A64, D, e.a, ga);
        cxa_grad64<DT>(A, A64, D, e.b, gb);
        cxa_hess64<DT>(A, A64, D, e.a, ha);
        cxa_hess64<DT>(A, A64, D, e.b, hb);
#pragma unroll
        for (int a = 0; a < 3; a++) g[a] = ga[a] + e.r * (gb[a] - ga[a]);
#pragma unroll
        for (int a = 0; a < 6; a++) h[a] = ha[a] + e.r * (hb[a] - ha[a]);
        if (world) {
            g[0] /= d0; g[1] /= d1; g[2] /= d2;
            h[0] /= d0 * d0; h[1] /= d1 * d1; h[2] /= d2 * d2;
            h[3] /= d0 * d1; h[4] /= d0 * d2; h[5] /= d1 * d2;
        }
        const double m = fmax(fabs(g[0]), fmax(fabs(g[1]), fabs(g[2])));
        if (m > 0.0 && m <= 1.7e308) {
            int ex;
            (void)frexp(m, &ex);
            const double sx = ldexp(g[0], -ex), sy = ldexp(g[1], -ex), sz = ldexp(g[2], -ex);
            const double len = sqrt(sx * sx + sy * sy + sz * sz);
            const double nx = sx / len, ny = sy / len, nz = sz / len, glen = ldexp(len, ex);
            const double nHn = nx * (h[0] * nx + h[3] * ny + h[4] * nz) + ny * (h[3] * nx + h[1] * ny + h[5] * nz) + nz * (h[4] * nx + h[5] * ny + h[2] * nz);
            mean = ((h[0] + h[1] + h[2]) - nHn) / (2.0 * glen);
            const double a00 = h[1] * h[2] - h[5] * h[5], a11 = h[0] * h[2] - h[4] * h[4], a22 = h[0] * h[1] - h[3] * h[3];
            const double a01 = h[4] * h[5] - h[3] * h[2], a02 = h[3] * h[5] - h[4] * h[1], a12 = h[3] * h[4] - h[0] * h[5];
            const double nAn = nx * (a00 * nx + a01 * ny + a02 * nz) + ny * (a01 * nx + a11 * ny + a12 * nz) + nz * (a02 * nx + a12 * ny + a22 * nz);
            gauss = nAn / glen / glen;
            const double root = sqrt(fmax(mean * mean - gauss, 0.0));
            k1 = mean + root; k2 = mean - root;
            if (vflip[v]) {                      // the winding is the other way round: the signs change and the larger one is now -k2
                mean = -mean;
                const double t = k1;
                k1 = -k2; k2 = -t;
            }
        }
    }
    out[(size_t)v * 4] = mean; out[(size_t)v * 4 + 1] = gauss; out[(size_t)v * 4 + 2] = k1; out[(size_t)v * 4 + 3] = k2;
}
template <int DTB>
__global__ void cx_k_level1_sample(const cx_grid_ref B, const cxa_edge1* __restrict__ edges, uint32_t nv, double* __restrict__ out) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const cxa_edge1 e = edges[v];
    const double b0 = (double)cx_sample<DTB>(B, e.a), b1 = (double)cx_sample<DTB>(B, e.b);
    out[v] = b0 + e.r * (b1 - b0);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
static cxa_dims cxa_dims_of(const cx_ctx* ctx) {
    cxa_dims D;
    D.n0 = (uint32_t)ctx->n0; D.n1 = (uint32_t)ctx->n1; D.n2 = (uint32_t)ctx->n2;
    D.plane = D.n1 * D.n2;
    D.dplane = cx_fdiv_make(D.plane);
    D.drow = cx_fdiv_make(D.n2);
    return D;
}
static bool cxa_delta_ok(const double* delta3) {
    if (!delta3) return true;
    for (int a = 0; a < 3; a++)
        if (!(delta3[a] > 0.0) || !std::isfinite(delta3[a])) return false;
    return true;
}

// the second grid as the kernels read it: the caller's device pointer, or a copy of the host array in a buffer of the context
static int cxa_second_grid(cx_ctx* ctx, const char* who, const void* grid, int32_t dtype, int on_device, cx_grid_ref* out) {
    if (!grid || !cx_dtype_valid(dtype)) { ctx->err = std::string(who) + ": a grid of a CX_DTYPE_* sample type is needed"; return CX_ERR_INVALID; }
    if (on_device) { *out = {grid, dtype}; return CX_OK; }
    const size_t bytes = (size_t)(ctx->n0 * ctx->n1 * ctx->n2) * cx_dtype_size(dtype);
    const int rc = ctx->attr_grid.grow(ctx, bytes);
    if (rc) return rc;
    CX_HIP(ctx, hipMemcpyAsync(ctx->attr_grid, grid, bytes, hipMemcpyHostToDevice, ctx->stream));
    CX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the caller's array may go away when this returns
    *out = {ctx->attr_grid, dtype};
    return CX_OK;
}

// Level 0: the current extraction and its vertex count (one synchronisation the first time the counts are asked for)
static int cxa_level0(cx_ctx* ctx, const char* who, uint32_t* nv) {
    if (!ctx->extracted || !ctx->grid.p) { ctx->err = std::string(who) + ": no valid extraction"; return CX_ERR_INVALID; }
    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_counts c;
    const int rc = cx_counts_get(ctx, &c);
    if (rc) return rc;
    *nv = (uint32_t)c.n_vertices;
    return CX_OK;
}

extern "C" int cx_level0_normals(cx_ctx* ctx, const double* delta3, void** normals_dev) {
    if (!ctx) return CX_ERR_INVALID;
    if (!cxa_delta_ok(delta3)) return cx_fail(ctx, CX_ERR_INVALID, "cx_level0_normals: the spacing must be positive and finite");
    uint32_t nv = 0;
    int rc = cxa_level0(ctx, "cx_level0_normals", &nv);
    if (rc) return rc;
    if (normals_dev) *normals_dev = nullptr;
    if (!nv) return CX_OK;
    if (ctx->attr_n0.cap() < nv && (rc = ctx->attr_n0.grow(ctx, (size_t)nv + nv / 16u + 64u))) return rc;
    const cxa_dims D = cxa_dims_of(ctx);
    const float d0 = delta3 ? (float)delta3[0] : 1.0f, d1 = delta3 ? (float)delta3[1] : 1.0f, d2 = delta3 ? (float)delta3[2] : 1.0f;
    cxa_v4f* out = ctx->attr_n0.as<cxa_v4f>();
#define CX_LAUNCH(DT)                                                                                                                          \
    if (delta3) hipLaunchKernelGGL((cx_k_vertex_normals<DT, true>), dim3(cx_blocks(nv)), dim3(256), 0, ctx->stream, ctx->grid, ctx->verts, out, nv, D, d0, d1, d2); \
    else hipLaunchKernelGGL((cx_k_vertex_normals<DT, false>), dim3(cx_blocks(nv)), dim3(256), 0, ctx->stream, ctx->grid, ctx->verts, out, nv, D, d0, d1, d2);
    CX_DISPATCH_DTYPE(ctx->grid.dtype, CX_LAUNCH)
#undef CX_LAUNCH
    CX_HIP(ctx, hipGetLastError());
    if (normals_dev) *normals_dev = ctx->attr_n0;
    return CX_OK;
}

extern "C" int cx_level0_normals_download(cx_ctx* ctx, const double* delta3, float* normals_xyzg) {
    if (!ctx || !normals_xyzg) return CX_ERR_INVALID;
    void* dev = nullptr;
    const int rc = cx_level0_normals(ctx, delta3, &dev);
    if (rc || !dev) return rc;
    return cx_copy_to_host1(ctx, normals_xyzg, dev, (size_t)ctx->counts.n_vertices * sizeof(float4));
}

extern "C" int cx_level0_sample_grid(cx_ctx* ctx, const void* grid, int32_t dtype, int on_device, void** values_dev, float* values_host) {
    if (!ctx) return CX_ERR_INVALID;
    uint32_t nv = 0;
    int rc = cxa_level0(ctx, "cx_level0_sample_grid", &nv);
    if (rc) return rc;
    cx_grid_ref B;
    if ((rc = cxa_second_grid(ctx, "cx_level0_sample_grid", grid, dtype, on_device, &B))) return rc;
    if (values_dev) *values_dev = nullptr;
    if (!nv) return CX_OK;
    if (ctx->attr_v0.cap() < nv && (rc = ctx->attr_v0.grow(ctx, (size_t)nv + nv / 16u + 64u))) return rc;
    const uint32_t n2 = (uint32_t)ctx->n2, plane = (uint32_t)(ctx->n1 * ctx->n2), ns = (uint32_t)(ctx->n0 * ctx->n1 * ctx->n2);
#define CX_LAUNCH(DT) hipLaunchKernelGGL((cx_k_vertex_sample<DT>), dim3(cx_blocks(nv)), dim3(256), 0, ctx->stream, B, ctx->verts, ctx->attr_v0, nv, n2, plane, ns);
    CX_DISPATCH_DTYPE(dtype, CX_LAUNCH)
#undef CX_LAUNCH
    CX_HIP(ctx, hipGetLastError());
    if (values_dev) *values_dev = ctx->attr_v0;
    if (values_host) return cx_copy_to_host1(ctx, values_host, ctx->attr_v0, (size_t)nv * sizeof(float));
    return CX_OK;
}

// Level 1: the view of the post-pass and the edge {a, b, ratio} of every output vertex in ctx->attr_e1
static int cxa_level1(cx_ctx* ctx, const char* who, cx_level1_view* V) {
    CX_HIP(ctx, hipSetDevice(ctx->device));
    int rc = cx_level1_attr_view(ctx, who, V);
    if (rc) return rc;
    if (!ctx->extracted || !ctx->grid.p) { ctx->err = std::string(who) + ": no valid extraction"; return CX_ERR_INVALID; }
    if (!V->nv) return CX_OK;
    if (ctx->attr_e1.cap() < (size_t)V->nv * sizeof(cxa_edge1) &&
        (rc = ctx->attr_e1.grow(ctx, ((size_t)V->nv + V->nv / 16u + 64u) * sizeof(cxa_edge1)))) return rc;
    const uint32_t n2 = (uint32_t)ctx->n2, plane = (uint32_t)(ctx->n1 * ctx->n2), ns = (uint32_t)(ctx->n0 * ctx->n1 * ctx->n2);
    const double* A64 = ctx->grid64_valid ? ctx->grid64 : nullptr;
    cxa_edge1* edges = ctx->attr_e1.as<cxa_edge1>();
#define CX_LAUNCH(DT) hipLaunchKernelGGL((cx_k_level1_edges<DT>), dim3(cx_blocks(V->nv)), dim3(256), 0, ctx->stream, ctx->grid, A64, V->keys, V->nv, n2, plane, ns, ctx->last.value, edges);
    CX_DISPATCH_DTYPE(ctx->grid.dtype, CX_LAUNCH)
#undef CX_LAUNCH
    CX_HIP(ctx, hipGetLastError());
    return CX_OK;
}

// the normals a simplified mesh carries (cx_level1_simplify with CX_SIMPLIFY_NORMALS): N as it stands, or normalize(N / delta)
__global__ void cx_k_carried_normals(const double* __restrict__ N, uint32_t nv, int scaled, double d0, double d1, double d2, double* __restrict__ out) {
#pragma clang fp contract(off)
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    double x = N[(size_t)v * 3], y = N[(size_t)v * 3 + 1], z = N[(size_t)v * 3 + 2];
    if (scaled) {
        x = x / d0; y = y / d1; z = z / d2;
        const double len = sqrt(x * x + y * y + z * z);
        if (len > 0.0) { x = x / len; y = y / len; z = z / len; }
    }
    out[(size_t)v * 3] = x; out[(size_t)v * 3 + 1] = y; out[(size_t)v * 3 + 2] = z;
}
// 0: not a simplified mesh; 1: served (or failed: *rc); the normals are in ctx->attr_n1
static int cxa_carried(cx_ctx* ctx, const double* delta3, void** normals_dev, uint32_t* nv_out, int* rc) {
    const double* N = nullptr;
    uint32_t nv = 0;
    const int mode = cx_level1_carried_normals(ctx, &N, &nv);
    if (!mode) return 0;
    *rc = CX_OK;
    if (mode == 2) { *rc = cx_fail(ctx, CX_ERR_UNSUPPORTED, "cx_level1_normals: the mesh was simplified without CX_SIMPLIFY_NORMALS: it carries no normals"); return 1; }
    if (normals_dev) *normals_dev = nullptr;
    if (nv_out) *nv_out = nv;
    if (!nv) return 1;
    if (hipSetDevice(ctx->device) != hipSuccess) { *rc = cx_fail(ctx, CX_ERR_HIP, "cx_level1_normals: hipSetDevice"); return 1; }
    if (ctx->attr_n1.cap() < (size_t)nv * 3u && (*rc = ctx->attr_n1.grow(ctx, ((size_t)nv + nv / 16u + 64u) * 3u))) return 1;
    hipLaunchKernelGGL(cx_k_carried_normals, dim3(cx_blocks(nv)), dim3(256), 0, ctx->stream, N, nv, delta3 ? 1 : 0, delta3 ? delta3[0] : 1.0, delta3 ? delta3[1] : 1.0,
                       delta3 ? delta3[2] : 1.0, ctx->attr_n1);
    if (hipGetLastError() != hipSuccess) { *rc = cx_fail(ctx, CX_ERR_HIP, "cx_level1_normals: launch of the carried normals failed"); return 1; }
    if (normals_dev) *normals_dev = ctx->attr_n1;
    return 1;
}

extern "C" int cx_level1_normals(cx_ctx* ctx, const double* delta3, void** normals_dev) {
    if (!ctx) return CX_ERR_INVALID;
    if (!cxa_delta_ok(delta3)) return cx_fail(ctx, CX_ERR_INVALID, "cx_level1_normals: the spacing must be positive and finite");
    int rcc = CX_OK;
    if (cxa_carried(ctx, delta3, normals_dev, nullptr, &rcc)) return rcc;
    if (cx_level1_capped(ctx)) return cx_fail(ctx, CX_ERR_UNSUPPORTED, "cx_level1_normals: a capped mesh (cx_postprocess3d_capped) has a crease along the rim and no single normal there");
    cx_level1_view V;
    int rc = cxa_level1(ctx, "cx_level1_normals", &V);
    if (rc) return rc;
    if (normals_dev) *normals_dev = nullptr;
    if (!V.nv) return CX_OK;
    if (ctx->attr_n1.cap() < (size_t)V.nv * 3u && (rc = ctx->attr_n1.grow(ctx, ((size_t)V.nv + V.nv / 16u + 64u) * 3u))) return rc;
    const cxa_dims D = cxa_dims_of(ctx);
    const double* A64 = ctx->grid64_valid ? ctx->grid64 : nullptr;
    const cxa_edge1* edges = ctx->attr_e1.as<cxa_edge1>();
    const double d0 = delta3 ? delta3[0] : 1.0, d1 = delta3 ? delta3[1] : 1.0, d2 = delta3 ? delta3[2] : 1.0;
#define CX_LAUNCH(DT) hipLaunchKernelGGL((cx_k_level1_normals<DT>), dim3(cx_blocks(V.nv)), dim3(256), 0, ctx->stream, ctx->grid, A64, edges, V.vflip, V.nv, D, delta3 ? 1 : 0, d0, d1, d2, ctx->attr_n1);
    CX_DISPATCH_DTYPE(ctx->grid.dtype, CX_LAUNCH)
#undef CX_LAUNCH
    CX_HIP(ctx, hipGetLastError());
    if (normals_dev) *normals_dev = ctx->attr_n1;
    return CX_OK;
}

extern "C" int cx_level1_normals_download(cx_ctx* ctx, const double* delta3, double* normals_xyz) {
    if (!ctx || !normals_xyz) return CX_ERR_INVALID;
    void* dev = nullptr;
    const int rc = cx_level1_normals(ctx, delta3, &dev);
    if (rc || !dev) return rc;
    const double* carried = nullptr;
    uint32_t nvc = 0;
    if (cx_level1_carried_normals(ctx, &carried, &nvc) == 1) return cx_copy_to_host1(ctx, normals_xyz, dev, (size_t)nvc * 3u * sizeof(double));
    cx_level1_view V;
    const int rv = cx_level1_attr_view(ctx, "cx_level1_normals_download", &V);
    if (rv) return rv;
    return cx_copy_to_host1(ctx, normals_xyz, dev, (size_t)V.nv * 3u * sizeof(double));
}

extern "C" int cx_level1_sample_grid(cx_ctx* ctx, const void* grid, int32_t dtype, int on_device, void** values_dev, double* values_host) {
    if (!ctx) return CX_ERR_INVALID;
    cx_level1_view V;
    int rc = cxa_level1(ctx, "cx_level1_sample_grid", &V);
    if (rc) return rc;
    cx_grid_ref B;
    if ((rc = cxa_second_grid(ctx, "cx_level1_sample_grid", grid, dtype, on_device, &B))) return rc;
    if (values_dev) *values_dev = nullptr;
    if (!V.nv) return CX_OK;
    if (ctx->attr_v1.cap() < V.nv && (rc = ctx->attr_v1.grow(ctx, (size_t)V.nv + V.nv / 16u + 64u))) return rc;
    const cxa_edge1* edges = ctx->attr_e1.as<cxa_edge1>();
#define CX_LAUNCH(DT) hipLaunchKernelGGL((cx_k_level1_sample<DT>), dim3(cx_blocks(V.nv)), dim3(256), 0, ctx->stream, B, edges, V.nv, ctx->attr_v1);
    CX_DISPATCH_DTYPE(dtype, CX_LAUNCH)
#undef CX_LAUNCH
    CX_HIP(ctx, hipGetLastError());
    if (values_dev) *values_dev = ctx->attr_v1;
    if (values_host) return cx_copy_to_host1(ctx, values_host, ctx->attr_v1, (size_t)V.nv * sizeof(double));
    return CX_OK;
}

// ---- curvature: host side --------------------------------------------------------------------------------------------------------------
static int cxa_curvature_axes(cx_ctx* ctx, const char* who) {
    if (ctx->n0 >= 3 && ctx->n1 >= 3 && ctx->n2 >= 3) return CX_OK;
    ctx->err = std::string(who) + ": curvature needs at least 3 samples on every axis (the Hessian is a second difference)";
    return CX_ERR_UNSUPPORTED;
}

extern "C" int cx_level0_curvature(cx_ctx* ctx, const double* delta3, void** curv_dev) {
    if (!ctx) return CX_ERR_INVALID;
    if (!cxa_delta_ok(delta3)) return cx_fail(ctx, CX_ERR_INVALID, "cx_level0_curvature: the spacing must be positive and finite");
    uint32_t nv = 0;
    int rc = cxa_level0(ctx, "cx_level0_curvature", &nv);
    if (rc) return rc;
    if ((rc = cxa_curvature_axes(ctx, "cx_level0_curvature"))) return rc;
    if (curv_dev) *curv_dev = nullptr;
    if (!nv) return CX_OK;
    if (ctx->attr_c0.cap() < nv && (rc = ctx->attr_c0.grow(ctx, (size_t)nv + nv / 16u + 64u))) return rc;
    const cxa_dims D = cxa_dims_of(ctx);
    const float d0 = delta3 ? (float)delta3[0] : 1.0f, d1 = delta3 ? (float)delta3[1] : 1.0f, d2 = delta3 ? (float)delta3[2] : 1.0f;
    cxa_v4f* out = ctx->attr_c0.as<cxa_v4f>();
#define CX_LAUNCH(DT)                                                                                                                          \
    if (delta3) hipLaunchKernelGGL((cx_k_vertex_curvature<DT, true>), dim3(cx_blocks(nv)), dim3(256), 0, ctx->stream, ctx->grid, ctx->verts, out, nv, D, d0, d1, d2); \
    else hipLaunchKernelGGL((cx_k_vertex_curvature<DT, false>), dim3(cx_blocks(nv)), dim3(256), 0, ctx->stream, ctx->grid, ctx->verts, out, nv, D, d0, d1, d2);
    CX_DISPATCH_DTYPE(ctx->grid.dtype, CX_LAUNCH)
#undef CX_LAUNCH
    CX_HIP(ctx, hipGetLastError());
    if (curv_dev) *curv_dev = ctx->attr_c0;
    return CX_OK;
}

extern "C" int cx_level0_curvature_download(cx_ctx* ctx, const double* delta3, float* curv_mgk1k2) {
    if (!ctx || !curv_mgk1k2) return CX_ERR_INVALID;
    void* dev = nullptr;
    const int rc = cx_level0_curvature(ctx, delta3, &dev);
    if (rc || !dev) return rc;
    return cx_copy_to_host1(ctx, curv_mgk1k2, dev, (size_t)ctx->counts.n_vertices * sizeof(float4));
}

// (a simplified mesh is refused by cx_level1_attr_view: its vertices are cluster means, and no curvature is carried over)
extern "C" int cx_level1_curvature(cx_ctx* ctx, const double* delta3, void** curv_dev) {
    if (!ctx) return CX_ERR_INVALID;
    if (!cxa_delta_ok(delta3)) return cx_fail(ctx, CX_ERR_INVALID, "cx_level1_curvature: the spacing must be positive and finite");
    if (cx_level1_capped(ctx)) return cx_fail(ctx, CX_ERR_UNSUPPORTED, "cx_level1_curvature: a capped mesh (cx_postprocess3d_capped) has a crease along the rim and flat caps: no curvature of the field there");
    cx_level1_view V;
    int rc = cxa_level1(ctx, "cx_level1_curvature", &V);
    if (rc) return rc;
    if ((rc = cxa_curvature_axes(ctx, "cx_level1_curvature"))) return rc;
    if (curv_dev) *curv_dev = nullptr;
    if (!V.nv) return CX_OK;
    if (ctx->attr_c1.cap() < (size_t)V.nv * 4u && (rc = ctx->attr_c1.grow(ctx, ((size_t)V.nv + V.nv / 16u + 64u) * 4u))) return rc;
    const cxa_dims D = cxa_dims_of(ctx);
    const uint32_t ns = (uint32_t)(ctx->n0 * ctx->n1 * ctx->n2);
    const double* A64 = ctx->grid64_valid ? ctx->grid64 : nullptr;
    const cxa_edge1* edges = ctx->attr_e1.as<cxa_edge1>();
    const double d0 = delta3 ? delta3[0] : 1.0, d1 = delta3 ? delta3[1] : 1.0, d2 = delta3 ? delta3[2] : 1.0;
#define CX_LAUNCH(DT) hipLaunchKernelGGL((cx_k_level1_curvature<DT>), dim3(cx_blocks(V.nv)), dim3(256), 0, ctx->stream, ctx->grid, A64, edges, V.vflip, V.nv, ns, D, delta3 ? 1 : 0, d0, d1, d2, ctx->attr_c1);
    CX_DISPATCH_DTYPE(ctx->grid.dtype, CX_LAUNCH)
#undef CX_LAUNCH
    CX_HIP(ctx, hipGetLastError());
    if (curv_dev) *curv_dev = ctx->attr_c1;
    return CX_OK;
}

extern "C" int cx_level1_curvature_download(cx_ctx* ctx, const double* delta3, double* curv_mgk1k2) {
    if (!ctx || !curv_mgk1k2) return CX_ERR_INVALID;
    void* dev = nullptr;
    const int rc = cx_level1_curvature(ctx, delta3, &dev);
    if (rc || !dev) return rc;
    cx_level1_view V;
    const int rv = cx_level1_attr_view(ctx, "cx_level1_curvature_download", &V);
    if (rv) return rv;
    return cx_copy_to_host1(ctx, curv_mgk1k2, dev, (size_t)V.nv * 4u * sizeof(double));
}
