// cx_march3d.hip -- Level-0 kernels of the 3-D marching-tetrahedra voxel march for gfx950 (wave64).
//
// Lattice "cell" q = lattice point (i,j,k) seen as the lower corner of the voxel [q, q+1].
// A cell OWNS the 7 lattice edges q -> q+d, d = 4di+2dj+dk in 1..7, and (when all 8 corners are
// inside the array) the 6 Kuhn tetrahedra of its voxel.  Vertex id of an edge = (lin(q) << 3) | d.
//
// Staged pipeline (any grid with n2 >= 4) -- no atomics, no barriers between waves:
//   S1  cx_k_stream            one pass over the samples: sign bits packed per lane, active cells (sign
//                              change among the 8 corners) appended to a per-wave queue in global memory
//                              as packed entries; the queue is cut into batches of >= CX_BATCH_MIN cells
//                              with the vertex / triangle counts that precede them (from the packed words).
//   S2  cx_k_scan_list         exclusive scan of the per-wave totals -> output offsets, counters, a flat
//                              list of all batches and the batch each later wave's share of rounds starts in.
//   S3  cx_k_emit_vertices     the rounds of 64 queued cells dealt evenly to the waves: vertex records (one
//                              lane per vertex), one (first vertex, crossing mask) word per queue entry,
//                              8-byte cell records.  With P.records_only: 16-byte cell records and nothing else.
//   K2  cx_k_emit_triangles_q  one lane per cell record: expands the tetrahedra into index triples; the vertex
//                              indices of neighbour cells come from their queue entries' words.
// Every kernel has ONE body: the timing experiments that once lived here behind -D switches and flag bits are gone, their
// results are in the comments at the places they decided and in DESIGN.md section 4.  What can still be selected is whole,
// tested paths: on request (public flags) the fused kernel cx_k_emit_mesh (S3 + K2 in one pass) and the tile kernels of
// cx_tile3d.h; in a process started with CX_DEBUG=1, the fraction stream (CX_TQ: S1 hands the interpolation fractions to S3)
// and the entry-walking triangle kernel cx_k_emit_triangles_e (CX_K2_ENTRIES).  Macros behind #ifndef only give numbers.
// Rows shorter than 4 samples, or on request (CX_KERNEL_GENERIC): cx_k_classify_generic (one lane per cell, LDS queue, one
// reservation atomic per workgroup and counter -- same-address atomics saturate near 88/us on MI355X) followed by
// cx_k_emit_triangles, which walks 16-byte cell records and looks neighbours up in a table of one entry per sample.
//
// This file is the head and the host part of ONE translation unit: the tables, the tunables, then the device code stage by stage
// from headers that are included here and nowhere else (they are sections, not self-contained, and their order is the order of
// definition), then the launchers.
//   cx_emit3d.h     entry / record formats and the per-cell emit code all emitting kernels share
//   cx_generic3d.h  cx_k_classify_generic
//   cx_stream3d.h   S1, S2: cx_k_stream, cx_k_stream_levels, cx_k_scan_list, cx_k_scan_list_levels
//   cx_vertex3d.h   S3: cx_k_emit_vertices
//   cx_tri3d.h      CPython hash (cx_k_hash_xy), pattern tables, cx_k_emit_triangles, _q, _e
//   cx_fused3d.h    cx_k_cell_info, cx_k_hash_bytes, cx_k_emit_mesh
//   cx_tile3d.h     cx_k_tile_emit, cx_k_tile_boundary
// One unit, because the three tables below have external linkage in a library built without relocatable device code: a unit of its
// own per stage would need its own static copies, and static tables change the code of most kernels.
#include <cstdlib>

#include "cx_cell.h"
#include "cx_dev.h"

__device__ __constant__ uint8_t cx_d_tet_corners[6][4] = CX_TET_CORNERS_INIT;
__device__ __constant__ uint32_t cx_d_tet_tris[6][16][2] = CX_TET_TRIS_INIT;
__device__ __constant__ uint8_t cx_d_voxel_ntri[256] = CX_VOXEL_NTRI_INIT;

#ifndef CX_QCAP
#define CX_QCAP 1024u       // generic kernel: active cells a wave can queue in LDS before it flushes on its own
#endif
#ifndef CX_K1_MIN_WAVES
#define CX_K1_MIN_WAVES 3   // stream kernel: two sample planes in flight per wave
#endif
#ifndef CX_RJ
#define CX_RJ 4             // cell rows per wave in the stream kernel (a workgroup covers 4*CX_RJ rows)
#endif
#ifndef CX_S3_MIN_SHARE
#define CX_S3_MIN_SHARE 4u   // rounds a vertex-stage wave takes at least (small surfaces: fewer waves rather than waves that only start up)
#endif
#ifndef CX_BATCH_MIN
#define CX_BATCH_MIN 512u   // a streaming wave closes a batch once it holds this many cells (128..1024 measured: 512 best)
#endif

#include "cx_emit3d.h"
#include "cx_generic3d.h"
#include "cx_stream3d.h"
#include "cx_vertex3d.h"
#include "cx_tri3d.h"
#include "cx_fused3d.h"
#include "cx_tile3d.h"

// ---- launchers --------------------------------------------------------------------------------------
// a lane loads 4 samples of one row: fp32 grids need 4-byte aligned samples, narrow types take any address
bool cx_fast_classify_supported(const cx_params& P) {
    return cx_fast_classify_supported_dims(P.n2, P.grid);
}

bool cx_fast_classify_supported_dims(int64_t n2, const cx_grid_ref& grid) {
    return n2 >= 4 && (grid.dtype != CX_DTYPE_F32 || (reinterpret_cast<uintptr_t>(grid.p) & 3u) == 0u);
}
// the aligned stream kernel: n2 % 4 == 0 and every lane's 4 samples on a 4 x sizeof(T) boundary
static bool cx_stream_aligned(const cx_params& P) {
    return (P.n2 % 4u == 0u) && ((reinterpret_cast<uintptr_t>(P.grid.p) & (4u * cx_dtype_size(P.grid.dtype) - 1u)) == 0u);
}

cx_task cx_fast_task(uint32_t n0, uint32_t n1, uint32_t n2) {
    cx_task T;
    T.nks = (n2 + 255u) / 256u;
    T.njg = (n1 + 4u * CX_RJ - 1u) / (4u * CX_RJ);
    // planes per task: aim at ~3000 workgroups (12 per CU: measured best at 512^3), 2..64 planes each
    const uint32_t per_plane = T.nks * T.njg;
    const uint32_t target = cx_debug_knob("CX_TASKS", 3072u);
    uint32_t want_chunks = (target + per_plane - 1u) / per_plane;
    if (want_chunks < 1u) want_chunks = 1u;
    uint32_t ci = (n0 + want_chunks - 1u) / want_chunks;
    if (ci < 2u) ci = 2u;
    // thin slabs (one rank's share of a volume split over 8 GPUs): at least 4 planes per task -- with 2 every task streams 3 sample
    // planes for 2 planes of cells; 64 planes: 0.0446 -> 0.0426 ms per extraction two in flight
    if (ci < 4u && n0 > 8u && !cx_debug_knob("CX_TASKS", 0u)) ci = 4u;
    if (ci > CX_SWP - 1u) ci = CX_SWP - 1u;   // the sign words of ci + 1 planes are staged in LDS (and the entry format has 7 bits)
    T.ci = ci;
    T.nic = (n0 + ci - 1u) / ci;
    T.nblocks = T.nks * T.njg * T.nic;
    T.chunk = (T.nblocks + 7u) / 8u;
    T.wcap = CX_RJ * 256u * ci;
    T.bcap = T.wcap / CX_BATCH_MIN + 1u;
    T.bndcap = (256u + 2u * CX_RJ) * ci;     // per HALF tile
    T.div_nks = cx_fdiv_make(T.nks);
    T.div_njg = cx_fdiv_make(T.njg);
    return T;
}

void cx_launch_stream(const cx_params& P, const cx_task& T, hipStream_t s) {
    const bool aligned = cx_stream_aligned(P);
    const uint32_t ring = P.tq ? (uint32_t)(4u * 2u * (CX_RJ + 1u) * CX_PLW * sizeof(float)) : 0u;   // the staged sample planes (cx_stream_tile)
#define CX_LAUNCH(DT)                                                                                       \
    if (aligned) hipLaunchKernelGGL((cx_k_stream<true, DT>), dim3(T.chunk * 8u), dim3(256), ring, s, P, T);  \
    else hipLaunchKernelGGL((cx_k_stream<false, DT>), dim3(T.chunk * 8u), dim3(256), ring, s, P, T);
    CX_DISPATCH_DTYPE(P.grid.dtype, CX_LAUNCH)
#undef CX_LAUNCH
}

void cx_launch_stream_levels(const cx_params* host_params, const cx_task& T, uint32_t nlevels, hipStream_t s) {
    const cx_params& P0 = host_params[0];
    const bool aligned = cx_stream_aligned(P0);
    for (uint32_t l0 = 0; l0 < nlevels; l0 += CX_LEVELS_PER_LAUNCH) {      // more than 8 levels: another pass over the samples per 8
        const uint32_t n = std::min(CX_LEVELS_PER_LAUNCH, nlevels - l0);
        cx_params_pack pack;
        for (uint32_t k = 0; k < CX_LEVELS_PER_LAUNCH; k++) pack.p[k] = host_params[l0 + std::min(k, n - 1u)];
#define CX_LAUNCH(DT)                                                                                                    \
        if (aligned) hipLaunchKernelGGL((cx_k_stream_levels<true, DT>), dim3(T.chunk * 8u * n), dim3(256), 0, s, pack, T, n);   \
        else hipLaunchKernelGGL((cx_k_stream_levels<false, DT>), dim3(T.chunk * 8u * n), dim3(256), 0, s, pack, T, n);
        CX_DISPATCH_DTYPE(P0.grid.dtype, CX_LAUNCH)
#undef CX_LAUNCH
    }
}
void cx_launch_scan_levels(const cx_params* device_params, const cx_task& T, uint32_t nlevels, hipStream_t s) {
    const uint32_t nw = T.nblocks * 4u;
    hipLaunchKernelGGL(cx_k_scan_list_levels, dim3((nw + 255u) / 256u, nlevels), dim3(256), 0, s, device_params, T, nw);
}

void cx_launch_scan_waves(const cx_params& P, const cx_task& T, hipStream_t s) {
    const uint32_t nw = T.nblocks * 4u;
    hipLaunchKernelGGL(cx_k_scan_list, dim3((nw + 255u) / 256u), dim3(256), 0, s, P, T, nw);
}

// one wave per batch, grid-stride: the batch count lives on the device, so launch what fills the chip
// a few times over (256 CUs) and let every wave walk the list
static uint32_t cx_batch_grid(const cx_params& P, uint32_t per_cu) {
    const uint32_t g = cx_debug_knob("CX_BGRID", 256u * per_cu);
    const uint32_t most = (P.fcap + 3u) / 4u;
    return g < most ? g : most;
}
// the vertex stage launches what is resident at once (24.8 KB of LDS per workgroup: 6 per CU) and gives every wave the same
// number of rounds; small grids: no more waves than batches could be
static uint32_t cx_vertex_grid(const cx_params& P) {
    // workgroups of the vertex stage the device holds at once, asked of the runtime (a grid beyond that starts a second
    // generation of waves when the first is two thirds through: measured +40 % kernel time with 6 per CU launched, 5 resident)
    static const uint32_t resident = [] {
        int per_cu = 0, dev = 0;
        hipDeviceProp_t prop;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, cx_k_emit_vertices<true, CX_DTYPE_F32>, 256, 0) != hipSuccess || per_cu < 1) per_cu = 4;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess || prop.multiProcessorCount < 1) return 256u * (uint32_t)per_cu;
        return (uint32_t)prop.multiProcessorCount * (uint32_t)per_cu;
    }();
    const uint32_t g = cx_debug_knob("CX_BGRID", resident);
    const uint32_t most = (P.fcap + 3u) / 4u;
    return g < most ? g : most;
}
uint32_t cx_vertex_stage_waves(const cx_params& P) { return 4u * cx_vertex_grid(P); }
void cx_launch_emit_vertices(const cx_params& P, const cx_task& T, hipStream_t s) {
    // the stream of fractions (P.tq, an A/B switch of fp32 grids) is not instantiated for narrow types: enqueue_extract leaves it off
    if (P.tq) hipLaunchKernelGGL((cx_k_emit_vertices<true, CX_DTYPE_F32>), dim3(P.nvw / 4u), dim3(256), 0, s, P, T);
    else {
#define CX_LAUNCH(DT) hipLaunchKernelGGL((cx_k_emit_vertices<false, DT>), dim3(P.nvw / 4u), dim3(256), 0, s, P, T);
        CX_DISPATCH_DTYPE(P.grid.dtype, CX_LAUNCH)
#undef CX_LAUNCH
    }
}


void cx_launch_classify_generic(const cx_params& P, hipStream_t s) {
    // contiguous cell ranges per block: multiples of 256, at least 16384, about 2048 blocks
    uint32_t cpb = (P.nsamples + 2047u) / 2048u;
    cpb = (cpb + 255u) & ~255u;
    if (cpb < 16384u) cpb = 16384u;
    const uint32_t blocks = (P.nsamples + cpb - 1u) / cpb;
#define CX_LAUNCH(DT) hipLaunchKernelGGL((cx_k_classify_generic<DT>), dim3(blocks), dim3(256), 0, s, P, cpb);
    CX_DISPATCH_DTYPE(P.grid.dtype, CX_LAUNCH)
#undef CX_LAUNCH
}

void cx_launch_emit_triangles(const cx_params& P, const uint64_t* hash_xy, hipStream_t s) {
    // one lane per record, grid-stride: launch what fills the chip a few times over
    uint32_t g = cx_debug_knob("CX_TGRID", 256u * 8u);
    const uint32_t most = (P.ccap + 255u) / 256u;
    if (g > most) g = most;
    if ((int32_t)P.org2 < 0) hipLaunchKernelGGL(cx_k_emit_triangles<true>, dim3(g ? g : 1u), dim3(256), 0, s, P, hash_xy);
    else hipLaunchKernelGGL(cx_k_emit_triangles<false>, dim3(g ? g : 1u), dim3(256), 0, s, P, hash_xy);
}

void cx_launch_emit_mesh(const cx_params& P, const cx_task& T, hipStream_t s) {
    hipLaunchKernelGGL(cx_k_cell_info, dim3(cx_batch_grid(P, 8u)), dim3(256), 0, s, P, T);
    hipLaunchKernelGGL(cx_k_emit_mesh, dim3(cx_batch_grid(P, 8u)), dim3(256), 0, s, P, T);
}

void cx_launch_hash_bytes(uint8_t* table, const uint64_t* hash_xy, uint32_t n0, uint32_t n1, uint32_t n2, uint32_t org2, hipStream_t s) {
    const uint64_t n = (uint64_t)n0 * n1 * n2;
    hipLaunchKernelGGL(cx_k_hash_bytes, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, s, table, hash_xy, n0 * n1, n2, (int32_t)org2);
}

void cx_launch_emit_triangles_q(const cx_params& P, const cx_task& T, const uint64_t* hash_xy, hipStream_t s) {
    uint32_t g = cx_debug_knob("CX_TGRID", 256u * 8u);
    const uint32_t most = (P.ccap + 255u) / 256u;
    if (g > most) g = most;
    const dim3 grid(g ? g : 1u);
    const bool neg = (int32_t)P.org2 < 0;
    if (P.write_records == CX_RECORDS_SLIM) {
        if (neg) hipLaunchKernelGGL((cx_k_emit_triangles_q<true, true>), grid, dim3(256), 0, s, P, T, hash_xy);
        else hipLaunchKernelGGL((cx_k_emit_triangles_q<false, true>), grid, dim3(256), 0, s, P, T, hash_xy);
    } else {
        if (neg) hipLaunchKernelGGL((cx_k_emit_triangles_q<true, false>), grid, dim3(256), 0, s, P, T, hash_xy);
        else hipLaunchKernelGGL((cx_k_emit_triangles_q<false, false>), grid, dim3(256), 0, s, P, T, hash_xy);
    }
}

// ---- fp32 grid coordinates of the vertex records, on request (cx_level0_download, cx_level0_device_ptrs): {x, y, z, bits(edge id)}
// with the crossing at q + t*d, in the same fp32 arithmetic the vertex stage used while its records still carried xyz
__global__ __launch_bounds__(256) void cx_k_expand_verts(const cx_vrec* __restrict__ recs, float4* __restrict__ out, uint32_t n, uint32_t n2, uint32_t plane,
                                                         cx_fdiv dplane, cx_fdiv drow) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= n) return;
    const cx_vrec r = recs[v];
    const uint32_t lin = r.x >> 3, d = r.x & 7u;
    const uint32_t i = cx_div(lin, dplane);
    const uint32_t rem = lin - i * plane;
    const uint32_t j = cx_div(rem, drow);
    const uint32_t k = rem - j * n2;
    const float t = __uint_as_float(r.y);
    const float fi = (float)i, fj = (float)j, fk = (float)k;
    float4 o;
    o.x = (d & 4u) ? fi + t : fi;
    o.y = (d & 2u) ? fj + t : fj;
    o.z = (d & 1u) ? fk + t : fk;
    o.w = __uint_as_float(r.x);
    out[v] = o;
}
void cx_launch_expand_verts(const cx_vrec* recs, float4* out, uint32_t n, uint32_t n1, uint32_t n2, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(cx_k_expand_verts, dim3((n + 255u) / 256u), dim3(256), 0, s, recs, out, n, n2, n1 * n2, cx_fdiv_make(n1 * n2), cx_fdiv_make(n2));
}

// the triangle stage's grid: what is resident at once, as for the vertex stage (its own count: it runs fewer waves per SIMD)
static uint32_t cx_triangle_grid(const cx_params& P) {
    static const uint32_t resident = [] {
        int per_cu = 0, dev = 0;
        hipDeviceProp_t prop;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, cx_k_emit_triangles_e<false>, 256, 0) != hipSuccess || per_cu < 1) per_cu = 4;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess || prop.multiProcessorCount < 1) return 256u * (uint32_t)per_cu;
        return (uint32_t)prop.multiProcessorCount * (uint32_t)per_cu;
    }();
    const uint32_t g = cx_debug_knob("CX_TGRID_E", resident);
    const uint32_t most = (P.fcap + 3u) / 4u;
    return g < most ? g : most;
}
uint32_t cx_triangle_stage_waves(const cx_params& P) { return 4u * cx_triangle_grid(P); }
void cx_launch_emit_triangles_e(const cx_params& P, const cx_task& T, const uint64_t* hash_xy, hipStream_t s) {
    if ((int32_t)P.org2 < 0) hipLaunchKernelGGL(cx_k_emit_triangles_e<true>, dim3(P.nkw / 4u), dim3(256), 0, s, P, T, hash_xy);
    else hipLaunchKernelGGL(cx_k_emit_triangles_e<false>, dim3(P.nkw / 4u), dim3(256), 0, s, P, T, hash_xy);
}

void cx_launch_hash_xy(uint64_t* table, uint32_t n0, uint32_t n1, uint32_t org0, uint32_t org1, hipStream_t s) {
    const uint32_t n = n0 * n1;
    hipLaunchKernelGGL(cx_k_hash_xy, dim3((n + 255u) / 256u), dim3(256), 0, s, table, n0, n1, org0, org1);
}
