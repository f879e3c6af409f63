/*
 * contourist_hip.h -- C ABI of the MI355X (gfx950) isosurface extractor.
 *
 * The reference (AaronWatters/contourist) is pure Python and has no FFI; its boundary for this
 * path is a Python class API.  Each entry point below names the reference interface whose work
 * it replaces (paths relative to the reference checkout, contourist/...).  The Python host side
 * (contourist_amd/) mirrors the reference's classes 1:1 and calls these through ctypes; see
 * INTEGRATION.md for the stub a reference maintainer would add.
 *
 * Conventions: every function returns 0 (CX_OK) or a negative cx_status, never throws, keeps no
 * global state.  One cx_ctx == one device + one HIP stream; contexts are independent and a
 * context must not be used from two threads at once.  The caller owns every host buffer; the
 * library owns every device buffer it allocates until cx_ctx_destroy (an adopted grid pointer
 * stays the caller's).  Sample arrays are C-ordered fp32, A[n0][n1][n2], last axis fastest;
 * array axes (0,1,2) are the reference's (x,y,z).
 */
#ifndef CONTOURIST_HIP_H
#define CONTOURIST_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cx_ctx cx_ctx;

typedef enum {
    CX_OK = 0,
    CX_ERR_INVALID = -1,     /* bad argument */
    CX_ERR_HIP = -2,         /* a HIP runtime call failed; see cx_last_error */
    CX_ERR_NOMEM = -3,       /* device or host allocation failed */
    CX_ERR_STATE = -4,       /* call out of order (no grid, no extraction yet, ...) */
    CX_ERR_CAPACITY = -5,    /* output buffers too small; counts say what is needed */
    CX_ERR_UNSUPPORTED = -6  /* e.g. more than 2^29 samples in one grid (32-bit vertex ids) */
} cx_status;

/* flags of cx_extract3d */
#define CX_DIAG_CANONICAL 0u   /* 2-2 tetrahedron: quad split follows the tetrahedron's vertex order */
#define CX_DIAG_CPYTHON310 1u  /* quad split reproduces CPython 3.10 set iteration order, i.e. the
                                  reference as it runs today (tetrahedral.py:592-595) */
#define CX_KERNEL_GENERIC 0x100u /* force the shape-agnostic classify kernel (default: auto) */
#define CX_KERNEL_STAGED 0x200u  /* emit through the staged kernels (vertex stage + words per queue entry + triangle stage): the default */
#define CX_KERNEL_FUSED 0x400u   /* emit vertices and triangles in ONE kernel over the cell queues (vertex indices of neighbour
                                    cells found through the queues, no table per sample, no cell records); same mesh, same
                                    numbering.  An extraction with samples inside the reference's np.allclose tolerances whose
                                    rules drop vertices is sent through the staged kernels automatically */
#define CX_KERNEL_TILED 0x800u   /* emit vertices and triangles tile by tile (one workgroup per tile of the streaming pass, the
                                    neighbour cells' vertex indices kept in LDS; the voxels on a tile's last row / last sample
                                    column by a small second kernel): same mesh, same numbering, ~0.35 GB less HBM traffic per
                                    512^3 extraction.  Sent through the staged kernels automatically when a sample sits inside the
                                    reference's np.allclose tolerances or a tile holds more surface cells than the LDS words */

typedef struct {
    int64_t n_cells;         /* lattice cells with a sign change among their corners */
    int64_t n_vertices;      /* interpolated edge crossings == len(interpolated_contour_pairs) */
    int64_t n_triangles;     /* == len(simplex_sets) before quantize_interpolations */
    int64_t n_border_voxels; /* voxels with a sign change for which GridContour.border_voxel() is true */
} cx_counts;

/* ---- context --------------------------------------------------------------------------------- */
int cx_ctx_create(int device_id, cx_ctx** out);
int cx_ctx_destroy(cx_ctx* ctx);
const char* cx_last_error(cx_ctx* ctx);
/* run on an existing HIP stream (e.g. torch.cuda.current_stream().cuda_stream); NULL = own stream */
int cx_set_stream(cx_ctx* ctx, void* hip_stream);
int cx_synchronize(cx_ctx* ctx);

/* ---- the sampled field ------------------------------------------------------------------------
 * Replaces grid_field.FunctionGrid.materialize_array / grid_function (grid_field.py:34-44, 95-118):
 * the dense fp32 array the march reads instead of calling f(x,y,z) per corner per use. */
int cx_grid_upload(cx_ctx* ctx, const float* host, int64_t n0, int64_t n1, int64_t n2);
int cx_grid_adopt_device(cx_ctx* ctx, const void* device_ptr, int64_t n0, int64_t n1, int64_t n2);
/* float64 originals of the bound fp32 samples (same dimensions; NULL drops them).  The reference interpolates a
 * crossing on the float64 values of its callable (tetrahedral.py:471-487); with these bound, Level 1
 * (cx_postprocess3d, cx_level0_points_f64) does the same, so crossings next to a weld-bucket boundary
 * (surface_geometry.py:30-48) fall on the reference's side of it.  The march itself stays on fp32. */
int cx_grid_shadow_f64(cx_ctx* ctx, const double* host, int64_t n0, int64_t n1, int64_t n2);

/* Sample types of a 3-D grid.  Every one converts to fp32 exactly: the kernels load the narrow type, convert it to fp32 in
 * registers and run the fp32 march unchanged, so a grid of type T gives bit for bit the result of the same call on its fp32
 * copy.  cx_grid_upload / cx_grid_adopt_device bind CX_DTYPE_F32. */
#define CX_DTYPE_F32 0
#define CX_DTYPE_U8 1
#define CX_DTYPE_I8 2
#define CX_DTYPE_U16 3
#define CX_DTYPE_I16 4
#define CX_DTYPE_F16 5
#define CX_DTYPE_BF16 6
/* n0*n1*n2 samples of type `dtype` (a CX_DTYPE_*; CX_ERR_INVALID otherwise), copied into a buffer of the context of
 * n0*n1*n2*sizeof(T) bytes: no fp32 copy is made or held. */
int cx_grid_upload_typed(cx_ctx* ctx, const void* host, int32_t dtype, int64_t n0, int64_t n1, int64_t n2);
/* the same for samples already on the device (not copied; they must outlive their use).  Any alignment: rows of a multiple of
 * 4 samples on a 4*sizeof(T)-byte boundary take the aligned stream kernel. */
int cx_grid_adopt_device_typed(cx_ctx* ctx, const void* device_ptr, int32_t dtype, int64_t n0, int64_t n1, int64_t n2);
/* the bound grid's sample type, and the device bytes the context holds for it: 0 for an adopted grid, n*sizeof(T) otherwise.
 * CX_ERR_STATE without a grid.  Either pointer may be NULL.
 * What a typed grid (dtype != CX_DTYPE_F32) runs through: cx_extract3d* (CX_KERNEL_FUSED and CX_KERNEL_TILED are served by the
 * staged kernels: cx_level0_path reports 1), cx_extract3d_levels, cx_postprocess3d*, cx_level0_points_f64 and the seeded
 * selection.  cx_grid_shadow_f64 accepts any type.  The 4-D, 2-D and slab-step entry points have grids of their own (fp32). */
int cx_grid_info(cx_ctx* ctx, int32_t* dtype, int64_t* device_bytes);

/* the grid is a sub-block of a larger volume starting at lattice point (o0,o1,o2) (slab partitions).
 * Only CX_DIAG_CPYTHON310 depends on it: the reference's set order hashes ABSOLUTE lattice
 * coordinates (tetrahedral.py:567-575), so slabs must hash global coordinates to agree with the
 * undivided volume.  Edge ids stay local; the caller adds (o0*n1*n2 + ...) << 3.
 * Negative origins are allowed (|o| < 2^30): an array that carries a rim of samples around the reference's grid starts
 * at lattice point -1 (CPython's hash(-1) == -2 is reproduced).  cx_level0_points_f64 adds the origin as well. */
int cx_set_origin(cx_ctx* ctx, int64_t o0, int64_t o1, int64_t o2);

/* optional: pre-size the output buffers (cells / vertices / triangles); 0 keeps the default. */
int cx_reserve(cx_ctx* ctx, int64_t max_cells, int64_t max_vertices, int64_t max_triangles);

/* ---- Level 0: the voxel march -------------------------------------------------------------------
 * Replaces, for a dense grid, in one pass over the samples:
 *   FunctionGrid.find_contour_crossing_grid_segments   grid_field.py:64-84     (crossing edges)
 *   GridContour.find_initial_voxels/expand_voxels/border_voxel  tetrahedral.py:383-469 (active voxels)
 *   GridContour3d.enumerate_voxel_triangles / enumerate_tetrahedron_triangles  tetrahedral.py:554-595
 *   GridContour.add_simplex / interpolate_pair / contour_pair_interpolation    tetrahedral.py:176-188, 471-512
 * Result (device resident): 8-byte vertex records {uint32 edge id, fp32 t}: the crossing sits at q + t*d on the lattice edge
 * q -> q+d, edge id = (linear index of the owning lattice point q << 3) | direction(1..7, = 4di+2dj+dk), t = (v - f(q)) /
 * (f(q+d) - f(q)) -- what contour_pair_interpolation keeps per pair (tetrahedral.py:471-512: the pair and its ratio); and
 * triangles as int32 index triples wound so the normal points from f<value to f>=value.  Level 1 recomputes every point in
 * float64 from the grid and the id alone; fp32 grid coordinates {x, y, z, bits(edge id)} are expanded from the records on
 * request (cx_level0_download, cx_level0_device_ptrs).
 * cx_extract3d enqueues the kernels and returns the counts (one device->host copy);
 * the _async form only enqueues.  Returns CX_ERR_CAPACITY (with valid counts) if a buffer was too
 * small: call cx_reserve with the counts and extract again. */
int cx_extract3d(cx_ctx* ctx, double value, uint32_t flags, cx_counts* out);
int cx_extract3d_async(cx_ctx* ctx, double value, uint32_t flags);
int cx_counts_get(cx_ctx* ctx, cx_counts* out);
/* Several isovalues of ONE grid in one call (BASELINE config 5; the reference classifies against all sorted levels at once only
 * in 2-D, multiple_2d_contour.py:17-30, 48-59).  The pass over the samples runs once for all levels (the levels' workgroups
 * stream a tile side by side: it comes from HBM once); scan, vertex and triangle stages then run per level, so every level's
 * mesh is bit for bit the cx_extract3d mesh of that isovalue.  values: nlevels (1..64) isovalues in any order;
 * flags: CX_DIAG_CANONICAL / CX_DIAG_CPYTHON310; out_counts: nlevels entries (may be NULL).  Every level keeps its own
 * device buffers, sized to its surface.  Needs rows of at least 4 samples (CX_ERR_UNSUPPORTED otherwise).
 * cx_levels_select makes level `index` the context's current extraction: cx_level0_download, cx_level0_points_f64,
 * cx_postprocess3d*, cx_select_seeded3d* ... then act on that level (level 0 is selected on return).  The levels stay valid
 * until the next cx_extract3d* / cx_grid_* call on the context. */
int cx_extract3d_levels(cx_ctx* ctx, const double* values, int32_t nlevels, uint32_t flags, cx_counts* out_counts);
int cx_levels_select(cx_ctx* ctx, int32_t index);
/* which kernels produced the last extraction: 0 generic classify + triangle stage, 1 staged pipeline (stream, scan, vertex
 * stage, triangle stage), 2 stream, scan + fused emit kernel, 3 tile emit -- for measurement (bench.py names its kernels by
 * it).  A grid of a type other than CX_DTYPE_F32 never takes 2 or 3: those requests run the staged pipeline (1). */
int cx_level0_path(cx_ctx* ctx, int* path);
/* copy the Level-0 mesh to host: verts = n_vertices*4 floats, tris = n_triangles*3 int32 */
int cx_level0_download(cx_ctx* ctx, float* verts_xyzk, int32_t* tris);
/* device pointers of the Level-0 mesh (valid until the next extract / reserve / destroy / call of this function): the
 * vertex records expanded to float4 {x, y, z, bits(edge id)} (enqueued on the context's stream) and the index triples */
int cx_level0_device_ptrs(cx_ctx* ctx, void** verts_xyzk, void** tris);
/* device pointers of the Level-0 buffers as the march leaves them: n_vertices x {uint32 edge id, fp32 t}, n_triangles x 3
 * int32 (no copy, no kernel; valid until the next extract / reserve / destroy) */
int cx_level0_device_records(cx_ctx* ctx, void** vertex_records, void** tris);
/* the same to host memory: vertex_records = n_vertices x 2 uint32 {edge id, bits of the fp32 fraction t}, tris as above -- half the
 * bytes of cx_level0_download for a host that keeps (pair, ratio) as the reference does (tetrahedral.py:471-512) */
int cx_level0_download_records(cx_ctx* ctx, uint32_t* vertex_records, int32_t* tris);

/* ---- Level 1: mesh post-passes -------------------------------------------------------------------
 * Replaces GridContour.quantize_interpolations (tetrahedral.py:190-215), remove_tiny_simplices
 * (:353-375), GridContour3d.extract_surface_geometry (:604-621), SurfaceGeometry.clean_triangles
 * (surface_geometry.py:14-50) and SurfaceGeometry.orient_triangles (:52-140) on the device.
 * corner = grid_dimensions of the reference (= n-1 per axis).  flags bit 0: skip clean_triangles
 * (the reference's clean=False).  out_counts (8 x int64): [0] vertices, [1] triangles,
 * [2] triangles after weld, [3] triangles after tiny collapse, [4] connected components. */
int cx_postprocess3d(cx_ctx* ctx, uint32_t flags, int64_t* out_counts);
/* same with GridContour.smooth_interpolations(smooth) (tetrahedral.py:329-351, 547-550) between the weld and
 * the tiny collapse; 0 < smooth <= 1, smooth == 0 disables it */
int cx_postprocess3d_ex(cx_ctx* ctx, uint32_t flags, double smooth, int64_t* out_counts);
/* Seeded selection.  Replaces GridContour.find_initial_voxels / expand_voxels (tetrahedral.py:396-463): the
 * reference only enumerates the surface voxels it reaches breadth-first (26 neighbours) from its end point
 * pairs; the dense march finds every surface voxel, and this call restricts the NEXT cx_postprocess3d* calls
 * (until the next extraction) to the triangles of the voxel groups reached from the given pairs.
 * endpoints_ijk: n x 6 int32 lattice points (i0,j0,k0, i1,j1,k1) whose samples straddle the isovalue; they are
 * bisected and mapped to seed voxels exactly as the reference does.  out_counts (4 x int64): [0] seed voxels,
 * [1] voxel groups kept, [2] triangles kept, [3] rejected pairs (the reference asserts on those; CX_ERR_INVALID).
 * range_lo_hi: NULL, or 6 int32 (lo[3], hi[3]) = the reference's in_range box (tetrahedral.py:465-469) when the
 * sample array carries a margin around the reference's grid (the reference evaluates its callable outside the
 * grid for seed voxels on the rim; growth stays inside the box).
 * Not calling it keeps every component, as the reference's exhaustive search_for_endpoints() does. */
/* The Level-1 scales (weld buckets int(10000/corner), tiny-simplex extent 1/corner) use corner = n-1 per axis.
 * When the sample array carries a margin around the reference's grid, hand over the reference's own corner
 * (voxels per axis); 0 restores the default. */
int cx_set_reference_corner(cx_ctx* ctx, int64_t c0, int64_t c1, int64_t c2);
/* The one exchange step of a volume split into slabs along array axis 0 (no counterpart in the single-process reference; SURVEY
 * section 8e): rank r owns n_own planes and marches them with ONE halo plane, the first plane of rank r+1.  local_planes: device
 * buffer of (n_own + 1) * plane_samples floats (n_own on the last rank); sends plane 0 to rank-1 and receives plane n_own from
 * rank+1 in one RCCL group on the context's stream, so extractions enqueued afterwards are ordered behind it.  rccl_comm: the
 * caller's ncclComm_t; RCCL is not linked but looked up in the calling process (CX_ERR_UNSUPPORTED if there is none).
 * world == 1: nothing to do.  (The Python host uses torch.distributed for the same step: contourist_amd/distributed.py.) */
int cx_halo_exchange(cx_ctx* ctx, void* rccl_comm, int rank, int world, float* local_planes, int64_t n_own, int64_t plane_samples);
/* A communicator owned by the context, for hosts that have none to hand over: cx_rccl_unique_id on ONE rank (128 bytes,
 * ncclGetUniqueId), the bytes carried to every rank by the host's own means, cx_rccl_comm_init (ncclCommInitRank, collective)
 * on every rank; cx_halo_exchange with rccl_comm == NULL then uses it.  Only an RCCL copy ALREADY loaded in the process is
 * used (CX_ERR_UNSUPPORTED otherwise): a PyTorch host carries its own. */
int cx_rccl_unique_id(uint8_t* out128);
int cx_rccl_comm_init(cx_ctx* ctx, const uint8_t* id128, int rank, int world);
int cx_rccl_comm_destroy(cx_ctx* ctx);
/* CX_OK if this process can run the C-side exchange (an RCCL copy is loaded and exports what is needed), CX_ERR_UNSUPPORTED if not.
 * Local, no collective: the host asks every rank and agrees on the answers BEFORE the collective cx_rccl_comm_init, so that a
 * rank without RCCL cannot leave the others waiting inside ncclCommInitRank. */
int cx_rccl_available(void);
/* the contexts of one rank (several extractions in flight) share ONE communicator: `ctx` uses `owner`'s from now on (the owner
 * must outlive it and keeps the ownership; cx_rccl_comm_destroy on `ctx` only drops the reference).  Exchanges are issued by the
 * host's single thread in volume order, each on the calling context's stream. */
int cx_rccl_comm_share(cx_ctx* ctx, cx_ctx* owner);
/* One rank's whole step for one volume of a slab-partitioned stream of volumes, as ONE call: adopt the device buffer
 * (n_own planes of n1 x n2 samples, followed by room for the halo plane unless rank == world - 1), exchange the halo on the
 * context's stream with the context's own communicator, enqueue cx_extract3d_async behind it.  (A 64-plane slab of a 512^3
 * volume is ~50 us of GPU time: the host side of a step has to be cheaper than that.) */
int cx_slab_step(cx_ctx* ctx, float* local_planes, int64_t n_own, int64_t n1, int64_t n2, int rank, int world, double value, uint32_t flags);
/* Seeded selection (tetrahedral.py:396-463): restricts the post-passes, until the next extraction, to the triangles of the voxel
 * groups reached from the end points.  endpoints_ijk: n x 6 int32 lattice points (i0,j0,k0, i1,j1,k1) whose samples straddle the
 * isovalue; range_lo_hi: lo[3], hi[3] of the in_range box, lo <= voxel < hi, clamped to the array (NULL: the whole array).
 * out_counts (4 x int64): [0] seed voxels (slots looked at, with one thread per pair), [1] groups kept, [2] triangles kept,
 * [3] rejected pairs (CX_ERR_INVALID: the context is then without a selection).
 * Groups kept, here and in cx_select_seeded4d*: the number of connected groups (26 neighbours, 80 in 4-D) of surface voxels
 * INSIDE the box, connected inside the box, that the selection keeps.  A seed voxel outside the box is kept and lets the groups it
 * touches grow, but is itself no group.  With CX_SEED_ALL_IN_RANGE every group inside the box is kept, so that is their number,
 * whatever the end points. */
int cx_select_seeded3d(cx_ctx* ctx, const int32_t* endpoints_ijk, int64_t n, const int32_t* range_lo_hi, int64_t* out_counts);
/* flags CX_SEED_ALL_IN_RANGE: every voxel inside range_lo_hi is kept (the exhaustive search_for_endpoints() of the
 * reference, tetrahedral.py:74-81) and the end points only add the seed voxels OUTSIDE it: the reference does not
 * range-check the voxels it starts from (:396-441), so a surface that reaches the rim of the grid gets triangles in
 * the voxels one step outside, next to the crossing lattice segments on the rim. */
#define CX_SEED_ALL_IN_RANGE 1u
/* CX_SEED_PARALLEL: one thread per end point pair without the reference's shared `visited` set (what more than 65 536
 * pairs get anyway); each point then yields its own voxel or its first border neighbour */
#define CX_SEED_PARALLEL 2u
int cx_select_seeded3d_ex(cx_ctx* ctx, const int32_t* endpoints_ijk, int64_t n, const int32_t* range_lo_hi, uint32_t flags,
                          int64_t* out_counts);
/* the masks of the last selection on the host (n_triangles and n_vertices bytes; all ones without a selection): for
 * callers that refine the Level-0 mesh on the host before cx_postprocess3d_mesh -- linear_interpolate=False
 * re-evaluates the caller's function between the lattice points (tetrahedral.py:488-505) */
int cx_seeded_masks_download(cx_ctx* ctx, uint8_t* tri_keep, uint8_t* vert_keep);
/* how the last cx_select_seeded3d* / cx_select_seeded4d* call ran its end points: 0 = one after the other with the reference's
 * shared `visited` set (tetrahedral.py:396-441; up to 65 536 pairs in 3-D, 16 384 in 4-D), 1 = one thread per pair
 * (CX_SEED_PARALLEL, or more pairs than that): adjacent candidate voxels may then be picked differently where pairs collide */
int cx_seeded_mode(cx_ctx* ctx, int* mode);
/* Level 1 of a mesh assembled by the caller -- the way several GPUs share one volume: every rank marches its slab
 * (cx_extract3d), takes the float64 coordinates the reference would have interpolated (cx_level0_points_f64: nv*3
 * doubles in the order of cx_level0_download, in the grid coordinates of the whole volume = lattice point + origin of
 * cx_set_origin; tetrahedral.py:471-487) and its triangles, the owner of the result
 * concatenates them in ASCENDING GLOBAL EDGE-ID ORDER (ids are global by formula; the index of a vertex is then its
 * priority in the canonical choices) and runs the same weld / tiny collapse / clean / orient on them:
 * corner = voxels per axis of the WHOLE volume, coordinates in its grid coordinates, triangles wound as the march
 * wound them (flags bit 2 set: windings are arbitrary, propagate them like cx_surface_geometry); flags bit 0 as in
 * (flags bit 3 set: the triangles are ones the march emitted -- slab meshes assembled on the host, a Level-0 mesh with refined points --, i.e.
 * an edge lies on at most two of them until the post-pass merges something into one of its ends: the components are then linked block by
 * block in LDS as in cx_postprocess3d instead of through the full edge table; a mesh of any other origin must leave it clear)
 * cx_postprocess3d.  Results through cx_level1_download. */
int cx_level0_points_f64(cx_ctx* ctx, double* points_xyz);
int cx_postprocess3d_mesh(cx_ctx* ctx, const double* points_xyz, int64_t nv, const int32_t* tris, int64_t nt, const int64_t* corner3,
                          uint32_t flags, double smooth, int64_t* out_counts);
/* copy the Level-1 mesh to host: points = nv*3 doubles (grid coordinates), tris = nt*3 int32 */
int cx_level1_download(cx_ctx* ctx, double* points_xyz, int32_t* tris);
/* device pointers of the same mesh (no copy): points = n_vertices*3 doubles (grid coordinates), tris = n_triangles*3 int32, valid
 * until the next post-pass / extraction / destroy on the context; the context's stream is synchronised before they are handed out.
 * For consumers on the GPU: what get_points_and_triangles() returns (tetrahedral.py:83-87, 528-552) without the trip to the host. */
int cx_level1_device_ptrs(cx_ctx* ctx, void** points_xyz, void** tris, int64_t* n_vertices, int64_t* n_triangles);
/* edge id ((linear index of the lower lattice point << 3) | direction, local to the marched array) of every vertex of
 * cx_level1_download, in its order: the representative that survived weld, tiny collapse and clean-up -- the identity of a
 * Level-1 vertex across slabs (after cx_postprocess3d_mesh: the index of the input vertex). */
int cx_level1_download_keys(cx_ctx* ctx, uint32_t* keys);

/* ---- Level 1 sharded over slabs (the reference is one process: tetrahedral.py:190-215, 353-375,
 * surface_geometry.py:14-140).  The context holds the extraction of a slab marched together with TWO layers of cells of
 * each neighbour (cx_set_origin: where the local array starts in the whole volume; cx_set_reference_corner: the corner of
 * the whole volume).  begin: weld / tiny collapse / clean-up of everything local, components of the own and first-layer
 * triangles.  What the ranks must agree on follows the slab BOUNDARY: _boundary hands out (hash of the three original edge
 * ids in the whole volume's numbering, component label) for this slab's own triangles next to its lower neighbour
 * (which = 1) and for its copies of the upper neighbour's first layer (which = 4) -- rank r's list 4 and rank r+1's list 1
 * are the same triangles, sorted by hash they pair the labels up; hash / label may be DEVICE pointers.  _candidates: per
 * component that reaches a neighbour, the start-triangle candidate among the own triangles (surface_geometry.py:79-103).
 * finish: the agreed flip per such component; afterwards cx_level1_download / _keys / cx_level1_write hand out the slab's
 * OWN part of the mesh in whole-volume coordinates.  own_lo / own_hi: own cell layers [lo, hi) of the local array.
 * flags as cx_postprocess3d. */
int cx_postprocess3d_shard_begin(cx_ctx* ctx, uint32_t flags, int64_t own_lo, int64_t own_hi, int64_t* out_counts8,
                                 int64_t* n_own_lower, int64_t* n_upper_copies, int64_t* n_candidates);
int cx_postprocess3d_shard_boundary(cx_ctx* ctx, int which, uint64_t* hash, uint32_t* label);
int cx_postprocess3d_shard_candidates(cx_ctx* ctx, uint32_t* cand_label, double* cand_x, uint32_t* cand_vertex_key, double* cand_nx,
                                      uint8_t* cand_negative, uint8_t* cand_has);
int cx_postprocess3d_shard_finish(cx_ctx* ctx, const uint32_t* labels, const uint8_t* flips, int64_t n, int64_t* out_counts8);

/* Binary mesh file straight from the Level-1 device buffers -- the step right after get_points_and_triangles() for every caller
 * of the reference (html_demo.py:118-161), without materialising the mesh in the caller's address space: the file's records are
 * laid out on the device and streamed through pinned staging buffers.  format CX_FILE_PLY: binary little-endian PLY, float64
 * x y z per vertex, faces as uchar 3 + three int32 (what contourist_amd.mesh_io.write_ply writes from host arrays, byte for
 * byte); CX_FILE_GLTF_BIN: the .bin payload of a glTF 2.0 mesh, float32 positions followed by uint32 indices.
 * mins_delta: NULL (grid coordinates) or {min_x, min_y, min_z, delta_x, delta_y, delta_z} for FunctionGrid.from_grid_coordinates
 * (grid_field.py:89-93).  out_info (9 doubles, may be NULL): vertices, triangles, bytes written, min xyz, max xyz of the
 * positions as written (glTF accessor bounds; PLY: not computed).  Face order is the device's (the Python API sorts the rows). */
#define CX_FILE_PLY 0
#define CX_FILE_GLTF_BIN 1
/* the same with the unit normals of cx_level1_normals (world normals, delta = mins_delta[3..5], when mins_delta is given):
 * CX_FILE_PLY_NORMALS: double nx ny nz after x y z in every vertex record (contourist_amd.mesh_io.write_ply with normals, byte for
 * byte); CX_FILE_GLTF_BIN_NORMALS: float32 positions, float32 normals, uint32 indices.  out_info as for the other two. */
#define CX_FILE_PLY_NORMALS 2
#define CX_FILE_GLTF_BIN_NORMALS 3
int cx_level1_write(cx_ctx* ctx, int format, const char* path, const double* mins_delta, double* out_info);

/* ---- vertex attributes: normals from the field's gradient, and a second grid sampled at the vertices -------------------------------
 * What every consumer of the reference computes right after get_points_and_triangles (html_demo.py:91-92 asks three.js for
 * computeFaceNormals / computeVertexNormals).  A vertex is a crossing of the lattice edge a -> b at fraction r; the resident sample
 * array gives the gradient G at both ends by the rule of numpy.gradient with its defaults (central difference inside, the one-sided
 * first difference on the rim of the marched array, unit spacing), and
 *     g = G(a) + r * (G(b) - G(a));   g_axis /= delta3[axis] when delta3 != NULL (world spacing);   n = s * g / |g|, (0,0,0) when |g| == 0.
 * Level 0: a = the owning lattice point q, b = q + d, r = the fp32 fraction of the vertex record, fp32 arithmetic, s = +1 (the march
 * winds its triangles from f < value to f >= value: the gradient's side).  One float4 {nx, ny, nz, |g|} per vertex record, |g| the
 * length before normalisation.
 * Level 1: the vertices of cx_level1_download in its order, identified by cx_level1_download_keys; a, b, r = the low point, the high
 * point and the ratio of the float64 interpolation (on the float64 originals of cx_grid_shadow_f64 when bound; ratio 0.5 where the
 * two samples are within 1e-8), float64 throughout, three doubles per vertex.  s = -1 for the vertices of a component whose
 * triangles the orientation step reversed, +1 otherwise: a Level-1 normal agrees with the winding of its triangles.
 * A second grid B of the marched array's shape, of any CX_DTYPE_*, is sampled at the same places: B(a) + r * (B(b) - B(a)), fp32 at
 * Level 0, float64 at Level 1.  grid: host pointer (copied into a buffer of the context), or device pointer when on_device != 0.
 * values_dev / values_host: either may be NULL.
 * The kernels are enqueued on the context's stream; the device buffers belong to the context, are reused between calls and are valid
 * until the next call of the same function, extraction or post-pass.  CX_ERR_INVALID without an extraction (Level 0) or a post-pass
 * (Level 1).  CX_ERR_UNSUPPORTED where the Level-1 vertices are not edge crossings of the resident array: after
 * cx_postprocess3d_mesh (refined points, volumes assembled from slabs or ranks) and after cx_postprocess3d_shard_finish (the flips
 * come from other ranks and the rim planes belong to neighbours).  After cx_levels_select they act on the selected level; after a
 * seeded selection Level 0 covers every vertex record and Level 1 what the selection kept. */
int cx_level0_normals(cx_ctx* ctx, const double* delta3, void** normals_dev);
int cx_level0_normals_download(cx_ctx* ctx, const double* delta3, float* normals_xyzg);
int cx_level1_normals(cx_ctx* ctx, const double* delta3, void** normals_dev);
int cx_level1_normals_download(cx_ctx* ctx, const double* delta3, double* normals_xyz);
int cx_level0_sample_grid(cx_ctx* ctx, const void* grid, int32_t dtype, int on_device, void** values_dev, float* values_host);
int cx_level1_sample_grid(cx_ctx* ctx, const void* grid, int32_t dtype, int on_device, void** values_dev, double* values_host);

/* Curvature at the same vertices: how strongly the isosurface bends.  For an isosurface it is a closed formula in the field's
 * gradient and Hessian at the crossing, so it needs no mesh adjacency.  f is the resident sample array, p a lattice point.
 * Gradient G(p): the rule of the normals above (numpy.gradient with its defaults).
 * Hessian H(p): second differences at the centre c = clamp(p, 1, n-2) on every axis -- a rim point takes the Hessian of its
 * nearest interior point -- in this order of evaluation (the error bound of the tests rests on it):
 *     H_aa = (f[c+e_a] - f[c]) - (f[c] - f[c-e_a])
 *     H_ab = ((f[c+e_a+e_b] - f[c+e_a-e_b]) - (f[c-e_a+e_b] - f[c-e_a-e_b])) * 0.25   for a < b, H symmetric
 * 19 samples per lattice point; inside the array the 6 axis neighbours are the gradient's samples too.
 * At a vertex on the edge a -> b at fraction r (a, b, r per level exactly as the normals take them):
 *     g = G(a) + r (G(b) - G(a)),  H = H(a) + r (H(b) - H(a));   with delta3: g_i /= delta_i, H_ij /= delta_i delta_j;   n = g / |g|
 *     mean  = (tr H - n'Hn) / (2 |g|)
 *     gauss = n' adj(H) n / |g|^2
 *     k1, k2 = mean +- sqrt(max(mean^2 - gauss, 0)),  k1 >= k2
 * g is scaled by a power of two before it is squared, as for the normals; |g| == 0 gives four zeros.  Sign: a sphere whose field
 * grows outwards has mean = +1/R and gauss = 1/R^2.
 * Level 0: fp32, s = +1, one float4 {mean, gauss, k1, k2} per vertex record in record order.
 * Level 1: float64 (on the float64 shadow samples when bound), double[4] {mean, gauss, k1, k2} per vertex of cx_level1_download.
 * For a vertex whose component the orientation step reversed, mean, k1 and k2 change sign and k1, k2 swap, so that k1 >= k2 still
 * holds; gauss is unchanged.  Curvature then agrees with cx_level1_normals and the winding.
 * Stream, buffer lifetime, delta3 and the error codes are those of the normals (CX_ERR_INVALID without an extraction or a post-pass,
 * CX_ERR_UNSUPPORTED after cx_postprocess3d_mesh and the sharded post-pass; the selected level after cx_levels_select, the filtered
 * mesh after cx_level1_keep_components).  Also CX_ERR_UNSUPPORTED: an axis with fewer than 3 samples, and a mesh that came through
 * cx_level1_simplify (its vertices are cluster means, not crossings, and no curvature is carried over). */
int cx_level0_curvature(cx_ctx* ctx, const double* delta3, void** curv_dev);
int cx_level0_curvature_download(cx_ctx* ctx, const double* delta3, float* curv_mgk1k2);
int cx_level1_curvature(cx_ctx* ctx, const double* delta3, void** curv_dev);
int cx_level1_curvature_download(cx_ctx* ctx, const double* delta3, double* curv_mgk1k2);

/* ---- components of the Level-1 mesh: labels, per-component measures, filtering -------------------------------------------------------
 * What a caller does with an isosurface of noisy data right after extracting it: how many pieces, how big is each, is it closed, and
 * drop the specks / keep the largest few.  The orientation step of the post-pass already finds the components (the reference orients
 * every component on its own, surface_geometry.py:52-140); these calls read its tables, so the mesh never leaves the device.
 * Component      = a set of the orientation step: the triangles linked through shared edges.  Their number is out_counts[4] of
 *                  the post-pass that made the mesh.
 * Component id   c in 0 .. nc-1: the components in ascending order of their smallest triangle index in the order of
 *                  cx_level1_download.  It depends on the mesh only.
 * Triangle label int32[nt]: the id of the triangle's component.  Vertex label int32[nv]: the SMALLEST id among the components of
 *                  the triangles that use the vertex (two components may touch in a vertex without sharing an edge); -1 for a
 *                  vertex no triangle uses.
 * Measures, of the triangles as wound in the output (p0, p1, p2 = the rows of the triangle array), in world coordinates
 * w = grid * delta + mins when mins_delta (six doubles, as for cx_level1_write; mapped without fused multiply-add) is given, in
 * grid coordinates when it is NULL:
 *   triangles, vertices   counts (vertices by vertex label)
 *   area                  sum of |(p1-p0) x (p2-p0)| / 2
 *   volume                sum of det[p0-o, p1-o, p2-o] / 6, o = the centre of the WHOLE mesh's grid box (corner / 2, mapped like the
 *                         points; one o for all components, returned in origin3_and_q[0..2]).  Signed: positive for a closed
 *                         component wound outward, negative for one wound inward (the reference winds the outermost of nested
 *                         shells outward and every component by its own max-x rule).  For an open component it depends on o.
 *   centroid[3]           area-weighted mean of the triangle centroids ((0,0,0) for zero area)
 *   bbox_lo, bbox_hi      over the triangles' vertices
 *   flipped               1 = the orientation step reversed the component's root triangle (the s of cx_level1_normals)
 *   closed                1 = every undirected edge of the component is used by an even number of its triangles.  Decided from
 *                         the XOR of a 64-bit hash of the edges {min, max} of all its triangles: a false "closed" needs a 64-bit
 *                         hash collision; "open" is never wrong.
 *   first_triangle        the component's smallest triangle index
 * Reproducible: every triangle's term of the three sums (area, volume, centroid moments) is rounded once to a multiple of 2^-q' with
 * q' >= q = origin3_and_q[3], chosen from the grid box alone, and the integers are added exactly; a record is the same bit for bit in
 * every call, in every context, and whatever other components the mesh holds (cx_level1_keep_components leaves the kept records
 * unchanged).  |sum - exact sum of the terms| <= triangles * 2^-(q+1).  The grid is chosen for vertices that lie within the diagonal of
 * the grid box of its centre.  A term past that bound (a caller's mesh that does not fit the corner it was handed over with, a wrong
 * cx_set_reference_corner) is clamped and the record says so: reserved[0] == 1.0 means its three sums are not exact; 0.0 otherwise.
 * The table and the labels live in buffers of the context, are made on the first request and kept until the next post-pass or
 * cx_level1_keep_components; table_dev / the label pointers are valid until then (kernels are enqueued on the context's stream).
 * cx_level1_keep_components: keep[c] != 0 keeps component c (nc bytes on the host).  Triangles, vertices and keys keep their relative
 * order, components are renumbered in order; afterwards every reader of the Level-1 mesh -- cx_level1_download, _device_ptrs,
 * _download_keys, cx_level1_write, cx_level1_normals, cx_level1_sample_grid and these calls -- serves the filtered mesh.
 * (cx_surface_geometry works on arrays of the caller and is not affected.)  All ones leaves everything as it is; all zeros gives
 * an empty mesh.  out_counts: [0] vertices, [1] triangles, [4] components.  The sign of cx_level1_normals is read from the tables of the
 * FILTERED mesh: a vertex shared by two components with different flips (they touch in it without sharing an edge) takes the flip of a
 * component that is still there, which can differ from its sign before the filter; every other kept vertex keeps its normal bit for bit.
 * CX_ERR_INVALID without a Level-1 mesh; CX_ERR_UNSUPPORTED after cx_postprocess3d_shard_* (a shard's components reach other ranks);
 * CX_ERR_STATE when the tables of the orientation step are gone (a 4-D pass on the same context used their memory).  Meshes of
 * cx_postprocess3d_mesh are served: nothing here needs edge ids. */
typedef struct cx_component {            /* 128 bytes, plain data */
    int64_t triangles, vertices;
    double  area, volume, centroid[3], bbox_lo[3], bbox_hi[3];
    int32_t flipped, closed;
    int64_t first_triangle;              /* smallest triangle index (device order) */
    double  reserved[1];                 /* [0]: 1.0 when a term was past the bound of the sums' grid (see above), else 0.0 */
} cx_component;
int cx_level1_components(cx_ctx* ctx, const double* mins_delta, int64_t* n_components, void** table_dev, double* origin3_and_q);
int cx_level1_components_download(cx_ctx* ctx, const double* mins_delta, cx_component* out);
int cx_level1_component_labels(cx_ctx* ctx, void** tri_labels_dev, void** vert_labels_dev);
int cx_level1_component_labels_download(cx_ctx* ctx, int32_t* tri_labels, int32_t* vert_labels);
int cx_level1_keep_components(cx_ctx* ctx, const uint8_t* keep, int64_t* out_counts);

/* ---- topology of the Level-1 mesh: Euler number, genus, boundary loops -------------------------------------------------------------
 * What a caller asks right after cx_level1_components: is this piece a blob or riddled with handles, where has the array's rim cut
 * the surface open (the boundary curves as polylines, to cap, measure or show them), and can a simplified mesh still be trusted
 * (edges with three or more triangles).  All integers, counted exactly: no hash decides anything here.
 * Defined for ANY Level-1 mesh, whatever the multiplicity of its edges.  Input: the current unsharded Level-1 mesh -- triangles T in
 * device order -- and the triangle labels of cx_level1_component_labels.
 * Edge             an unordered pair {T[t][k], T[t][(k+1)%3]}; its multiplicity is the number of (t, k) that produce it.  All the
 *                  triangles on one edge belong to one component (the orientation step links every pair that shares an edge).
 * Per component c:
 *   triangles          F
 *   vertices           V, the number of DISTINCT vertex indices its triangles use.  A vertex two components share counts in both:
 *                      this is NOT cx_component.vertices, which counts every vertex once, for its smallest label.
 *   edges              E, its distinct edges
 *   boundary_edges     edges of multiplicity 1
 *   nonmanifold_edges  edges of multiplicity 3 or more
 *   euler              V - E + F
 *   boundary_loops     b, the number of its boundary loops; nonsimple_loops: those that are not simple
 *   genus              (2 - euler - b) / 2 when that is a non-negative integer and nonmanifold_edges == 0, otherwise -1.  It is the
 *                      genus proper only for an orientable 2-manifold with boundary: non-orientability is not detected (a Moebius
 *                      strip gives -1 only because 2 - euler - b is odd for it), nor are vertex pinches.
 * Boundary loop    a connected component of this graph: the nodes are the boundary edges of ONE mesh component, two nodes are linked
 *                  when the edges share a vertex.  A loop is simple when every vertex on it lies on exactly two of its edges (an
 *                  edge whose two ends are one vertex makes its loop non-simple).
 * Loop ids         0 .. L-1 over the whole mesh, in ascending order of the smallest 3*t + k among the loop's edges.
 * Loop vertices    one int32 array of length B, the total number of boundary edges, holds every loop's `count` entries from `first`
 *                  on, the loops in id order.  A simple loop is stored as its vertices in cyclic order: it starts at T[t][k] of its
 *                  smallest (t, k) and runs in that edge's direction, T[t][k] -> T[t][(k+1)%3].  A non-simple loop is stored as the
 *                  tail vertices T[t][k] of its edges in ascending 3*t + k.
 * The results live in buffers of the context, are made on the first request and cached per generation of the mesh: a new post-pass,
 * cx_level1_keep_components and cx_level1_simplify start a new one, after which they are rebuilt on request; the device pointers are
 * valid until then (kernels are enqueued on the context's stream).  An empty mesh has 0 components and 0 loops (null pointers).
 * Limits: fewer than 2^30 triangles (the edge table holds 4 slots of 16 bytes per triangle -- 64 bytes per triangle -- and 3*t + k
 * is a 32-bit word) and fewer than 2^30 boundary edges; CX_ERR_UNSUPPORTED with a message past them.
 * CX_ERR_INVALID without a Level-1 mesh; CX_ERR_UNSUPPORTED after cx_postprocess3d_shard_*; CX_ERR_STATE when the tables of the
 * orientation step are gone (see the components above).  Meshes of cx_postprocess3d_mesh are served.  Reproducible: every array is
 * the same byte for byte in every call and context. */
typedef struct cx_topology {             /* 64 bytes, plain data */
    int64_t triangles, vertices, edges, boundary_edges, nonmanifold_edges, euler;
    int32_t boundary_loops, genus;       /* genus -1: not defined, see above */
    int32_t nonsimple_loops, reserved;
} cx_topology;
typedef struct cx_loop {                 /* 16 bytes, plain data */
    int32_t component, simple;
    uint32_t first, count;               /* slice of the loop-vertex array */
} cx_loop;
int cx_level1_topology(cx_ctx* ctx, int64_t* n_components, void** table_dev);
int cx_level1_topology_download(cx_ctx* ctx, cx_topology* out);
int cx_level1_boundary_loops(cx_ctx* ctx, int64_t* n_loops, int64_t* n_boundary_edges, void** loops_dev, void** vertices_dev);
int cx_level1_boundary_loops_download(cx_ctx* ctx, cx_loop* loops, int32_t* vertices);

/* ---- simplification: vertex clustering of the Level-1 mesh on the device ---------------------------------------------------------
 * (The reference's flatten=True is serial LP decimation, a different algorithm with different output; it stays unsupported.)
 * Input: the current unsharded Level-1 mesh of the context -- points P (float64, grid coordinates), triangles T (device order) --
 * and the tables of the orientation step.  Parameters: cell3, three positive finite doubles in grid units, and flags.
 * Cluster of a vertex v:
 *   - its cell k_a = floor(P[v][a] / cell3[a]) per axis, an IEEE division as numpy.floor(p / c) computes it.  The lattice is anchored
 *     at grid coordinate 0; points on a sampled rim are negative, hence floor and not truncation.  The grid box has, per axis, the cells
 *     floor(-1 / cell_a) .. floor((corner_a + 1) / cell_a); a vertex outside of it (a caller's mesh that does not fit its corner)
 *     counts to the nearest cell of the box.
 *   - unless CX_SIMPLIFY_ACROSS_COMPONENTS is set the cluster is the pair (cell, vertex label of cx_level1_component_labels): two
 *     sheets that pass through one cell never fuse, and components cannot merge.
 *   - vertices with label -1 are dropped.
 *   - the number of cells of the grid box, per axis floor((corner_a + 1) / cell_a) - floor(-1 / cell_a) + 1, multiplied over the
 *     axes, must be below 2^31 ((label, linear cell) is one 64-bit table key): CX_ERR_INVALID otherwise, with a message that names
 *     the smallest admissible cell.
 * Position of a cluster: the mean of its members, computed exactly.  Each coordinate is clamped to [-1, corner_a + 1] (a clamped
 * coordinate is counted in out_counts[5]) and rounded once to X = llrint(x * 2^q), q = 52 - ceil(log2(max_a(corner_a) + 2)); q
 * comes from the grid box alone and is returned in *q_out.  The integers are added exactly (64-bit inside a wave, then a two-word
 * 128-bit accumulator per cluster); the result is double(sum), rounded once (to nearest, ties to even), / double(n), * 2^-q.
 * Order: new vertex i is the cluster with the i-th smallest first member, the first member being the cluster's smallest old vertex
 * index.  Surviving triangles keep their relative order and their winding.
 * Triangles: indices are remapped; a triangle with two equal indices is dropped; of several triangles with the same vertex set the
 * one with the smallest old index stays.  Unless CX_SIMPLIFY_NO_CLEAN (bit 0, with the meaning it has in cx_postprocess3d) is set,
 * the reference's clean_triangles rule (surface_geometry.py:14-50) then runs on the result with the kernels of the post-pass, on
 * the device buffers: nothing is uploaded, there is no weld and no tiny collapse.  The orientation step always runs, with the
 * windings taken as coherent (a component is turned as a whole by the max-x rule); afterwards cx_level1_components,
 * cx_level1_keep_components and their `flipped` work on the new mesh.  New vertices that no surviving triangle uses are compacted away.
 * Keys: cx_level1_download_keys gives the first member's old vertex index (the convention after cx_postprocess3d_mesh).  The keys
 * stop being edge ids: cx_level1_sample_grid answers CX_ERR_UNSUPPORTED after a simplification.
 * Carried normals (CX_SIMPLIFY_NORMALS): allowed only where cx_level1_normals is served for the source mesh (CX_ERR_UNSUPPORTED
 * elsewhere, the mesh untouched).  The grid-coordinate unit normals of the source (delta3 == NULL) are summed per cluster as
 * llrint(n * 2^30) integers, added exactly in 64 bits, then normalised in float64: N = s / sqrt(s.s), (0,0,0) for a zero sum.
 * After the call cx_level1_normals(delta3) serves N for delta3 == NULL and normalize(N / delta3) otherwise; so do
 * cx_level1_normals_download and the two _NORMALS file formats of cx_level1_write.  The component flip is not applied again (the
 * members' normals carry it; the orientation step's decision for the simplified mesh is reported by `flipped` as usual).
 * Simplifying a simplified mesh carries the carried normals on; cx_level1_keep_components keeps them with their vertices.  Without
 * the flag the normals calls answer CX_ERR_UNSUPPORTED after a simplification.
 * out_counts (8 x int64): [0] vertices, [1] triangles, [4] components, [5] clamped coordinates, [6] clusters, [7] triangles with
 * three distinct indices after the remap, before duplicate removal (an upper bound on [1]).  CX_SIMPLIFY_COUNT_ONLY is a dry run:
 * the mesh is untouched and only [6] and [7] are filled.
 * cx_level1_simplify_map: one int32 per vertex of the mesh BEFORE the call, its new index, -1 where the vertex went away (label -1,
 * or no surviving triangle uses its cluster; a cluster the clean rule merged into another maps to that one).  Valid until the next
 * post-pass, filter or simplification (CX_ERR_STATE then); callers use it to carry attributes of their own.
 * Errors and state: CX_ERR_INVALID without a Level-1 mesh or with bad cells; CX_ERR_UNSUPPORTED after cx_postprocess3d_shard_*;
 * CX_ERR_STATE when the tables of the orientation step are gone (a 4-D pass on the same context used their memory).  A call that
 * fails leaves the mesh as it was.  A successful call starts a new generation of the post state: cached component tables and
 * labels are rebuilt on request.  All buffers belong to the context and are reused.  Reproducible: every output array is the same
 * bit for bit in every call and context. */
#define CX_SIMPLIFY_NO_CLEAN           1u   /* bit 0, as cx_postprocess3d */
#define CX_SIMPLIFY_ACROSS_COMPONENTS  2u
#define CX_SIMPLIFY_COUNT_ONLY         4u   /* dry run: mesh untouched, only out_counts[6], [7] filled */
#define CX_SIMPLIFY_NORMALS            8u
int cx_level1_simplify(cx_ctx* ctx, const double* cell3, uint32_t flags, int64_t* out_counts8, double* q_out);
int cx_level1_simplify_map(cx_ctx* ctx, void** new_index_of_old_vertex_dev);
int cx_level1_simplify_map_download(cx_ctx* ctx, int32_t* new_index_of_old_vertex);

/* ---- clipping: cut the Level-1 mesh open by a plane or a per-vertex scalar, on the device ------------------------------------------
 * What a viewer or a measurement script does most often with an isosurface: keep the half in front of a plane, a region of interest,
 * or the part where a second volume is above a threshold.  cx_level1_keep_components only drops whole components; this cuts triangles.
 * (No counterpart in the reference.)
 * Input: the current unsharded Level-1 mesh (V vertices, T triangles in device order, every triangle with three distinct indices) and
 * one float64 scalar s[v] per vertex.  d[v] = s[v] - threshold, or threshold - s[v] with CX_CLIP_KEEP_BELOW.  A vertex is INSIDE iff
 * d[v] is finite and d[v] >= 0.
 *   - A triangle with a vertex whose d is not finite is dropped whole and counted (n_nonfinite).
 *   - Three vertices inside: the triangle is kept unchanged.  None inside: dropped.
 *   - One inside.  Rotate the corners, keeping the cyclic order, so that corner i is inside and j, k follow: one triangle
 *     (v_i, c(i,j), c(i,k)).
 *   - Two inside.  Rotate so that i is the outside corner: two triangles, (c(j,i), v_j, v_k) and (c(j,i), v_k, c(k,i)).  The diagonal
 *     is fixed by this rule and never looks at a neighbour.
 *   - c(a,b), with a inside and b outside: if d[a] == 0 it IS vertex a and no new vertex is made.  Otherwise it is the cut vertex of the
 *     undirected edge {lo, hi} = {min(a,b), max(a,b)}: one such vertex per mesh edge, shared by every triangle on that edge, at
 *         t = d[lo] / (d[lo] - d[hi]),   p = p[lo] + t * (p[hi] - p[lo])   per coordinate,
 *     every operation rounded once (no fused multiply-add), so numpy reproduces the bits.
 *   - Triangles left with two equal indices are dropped.
 * The vertex list handed to the tail is the V old vertices in their order, then the cut vertices, ordered by the smallest corner
 * number 3t+k among the triangle edges (edge k joins corners k and (k+1)%3) that cut that mesh edge.  The key of an old vertex is its
 * old index, the key of cut vertex r is V + r (cx_level1_download_keys).  Output triangles come in source-triangle order, the first of
 * a pair before the second; their priority triple is {t, t, t} of the source triangle, as the simplifier's.
 * Then comes the shared tail, exactly as after cx_level1_simplify: the reference's clean_triangles rule unless CX_CLIP_NO_CLEAN
 * (bit 0), compaction of the vertices in use, orientation with the windings taken as coherent.
 * CX_CLIP_NORMALS: an old vertex keeps its normal -- cx_level1_normals(delta3 == NULL) of the source, or its carried normals if the
 * source is itself a derived mesh; a cut vertex gets normalize((1 - t) * n[lo] + t * n[hi]), (0,0,0) for a zero sum, each operation
 * rounded once.  Allowed only where cx_level1_normals is served for the source (CX_ERR_UNSUPPORTED elsewhere, the mesh untouched).
 * The map has one record {lo, hi, t} per OUTPUT vertex, holding indices of the mesh before the call: lo == hi and t == 0 for a kept
 * vertex.  A caller carries any per-vertex attribute a of their own across the cut with it: (1 - t) * a[lo] + t * a[hi].
 * cx_level1_clip_plane: s = n0*x + n1*y + n2*z in grid coordinates, evaluated left to right with every operation rounded once;
 * plane4 = {n0, n1, n2, threshold}.  A zero or non-finite normal (or a non-finite threshold) gives CX_ERR_INVALID.
 * cx_level1_clip_scalars: the general entry; V doubles on the host, or on the device when on_device != 0 (the buffer
 * cx_level1_sample_grid returns may be handed over as it is).
 * out_counts (8 x int64): [0] vertices, [1] triangles, [2] cut vertices, [3] source triangles that were cut, [4] components,
 * [5] n_nonfinite (source triangles dropped for a non-finite d), [6] vertices with d == 0, [7] triangles handed to the tail (an upper
 * bound on [1]).
 * After a clip the mesh is a derived one in the sense of the simplification: cx_level1_normals serves the carried normals
 * (CX_ERR_UNSUPPORTED when the clip ran without CX_CLIP_NORMALS), cx_level1_sample_grid and cx_level1_curvature answer
 * CX_ERR_UNSUPPORTED, the simplify map is invalid.  The clip map is valid until the next post-pass, filter, simplification or clip
 * (CX_ERR_STATE then); its device pointers are (V', 2) int32 and (V',) float64.  Components, topology and boundary loops are
 * rebuilt on the next request; the boundary loops of a clipped closed surface are its cut curves.
 * Errors: CX_ERR_INVALID without a Level-1 mesh, with unknown flags or a bad plane; CX_ERR_UNSUPPORTED after
 * cx_postprocess3d_shard_*, for 2^30 triangles or more, and for CX_CLIP_NORMALS on a source without normals; CX_ERR_STATE when the
 * tables of the orientation step are gone.  A call that fails before the tail starts leaves the mesh bit for bit as it was.  All
 * buffers belong to the context (counted by cx_device_bytes) and are reused; the edge table is sized by the number of cut corners,
 * not by the mesh.  Reproducible: every output array is the same bit for bit in every call and context.
 * cx_level1_clip_info (measurement): of the last clip on this context, info8 = {ms of the clip kernels, ms of the tail with the
 * map, cut corners, slots of the edge table, V, T, vertices handed to the tail, triangles handed to the tail}, the times between
 * HIP events on the context's stream; CX_ERR_STATE when none has run. */
#define CX_CLIP_NO_CLEAN    1u   /* bit 0, as cx_postprocess3d */
#define CX_CLIP_KEEP_BELOW  2u
#define CX_CLIP_NORMALS     4u
int cx_level1_clip_plane(cx_ctx* ctx, const double* plane4, uint32_t flags, int64_t* out_counts8);
int cx_level1_clip_scalars(cx_ctx* ctx, const double* scalars, int on_device, double threshold, uint32_t flags, int64_t* out_counts8);
int cx_level1_clip_map(cx_ctx* ctx, void** lo_hi_dev, void** t_dev);
int cx_level1_clip_map_download(cx_ctx* ctx, int32_t* lo_hi, double* t);
int cx_level1_clip_info(cx_ctx* ctx, double* info8);

/* ---- rim caps: close the isosurface where the rim of the array cuts it open, on the device ------------------------------------------
 * A surface that runs into the edge of the sampled array ends there in boundary loops: its components are not closed, their signed
 * volume is no volume.  The cap is the cross-section of the solid with the selected faces of the array; march plus cap is a closed
 * mesh whose enclosed volume is that of {f >= value} (or {f < value}) under the march's own piecewise-linear interpolant.
 * (No counterpart in the reference.)
 * Input: the current extraction (resident grid of any CX_DTYPE_*, n0 x n1 x n2, isovalue v, nv Level-0 vertices {edge id, t}, nt
 * triangles), a 6-bit mask `faces` (bit 0: i = 0, bit 1: i = n0-1, bit 2: j = 0, bit 3: j = n1-1, bit 4: k = 0, bit 5: k = n2-1) and a
 * side: ABOVE caps where f >= v, BELOW (CX_CAP_BELOW) where f < v.
 *   - A lattice point is INSIDE iff !(f < v) for ABOVE and iff f < v for BELOW: the bit the march classifies with, read from the grid
 *     in its own type.
 *   - Face-triangles.  A face of axis a has the in-plane axes (u, w), u < w in the order i, j, k.  The Kuhn tetrahedra cut every unit
 *     square of it, lower corner (a, b) in (u, w), along the diagonal (a, b)-(a+1, b+1) (lattice direction 3 on an i-face, 5 on a j-face,
 *     6 on a k-face) into triangle 0 = {(a, b), (a+1, b), (a+1, b+1)} and triangle 1 = {(a, b), (a+1, b+1), (a, b+1)}, corners 0, 1, 2
 *     in that order.  The square's linear index in the face is a * (n_w - 1) + b.
 *   - Per face-triangle with m inside corners.  m = 0: nothing.  m = 3: one triangle (p_0, p_1, p_2) of lattice-point vertices.
 *     m = 1: rotate the corners, keeping the cyclic order, so that i is the inside one and j, k follow: (p_i, c(i,j), c(i,k)).
 *     m = 2: rotate so that i is the OUTSIDE one: (c(i,j), p_j, p_k) and (c(i,j), p_k, c(k,i)).  The quad's diagonal runs from the
 *     crossing behind the outside corner to the corner before it: a rule of the triangle's own corner numbers that never looks at a
 *     neighbour.
 *   - c(a,b) is the crossing of the lattice edge between corners a and b (their inside bits differ): the Level-0 vertex with that edge
 *     id, found by id, never made again.  Where the march has emitted none (it may skip a crossing under the reference's tolerance
 *     rules) the cap makes the vertex itself: key = the edge id, position by the float64 formula of the post-pass.  It is counted; the
 *     surface is already open there and the cap does not promise to close it.
 *   - A lattice-point vertex has key (linear index << 3) | 0 -- the direction field of an edge id takes 1..7, 0 is the lattice point
 *     itself --, position (i, j, k) exactly and t = 0.  A lattice point on two or three selected faces is ONE vertex.
 *   - Order.  The cap vertices follow the nv Level-0 vertices in ascending key.  The cap triangles follow the nt Level-0 triangles in
 *     the order (face number, square's linear index in the face, triangle 0 / 1, piece 0 / 1).
 *   - Winding.  The corners of a face-triangle run counter-clockwise in (u, w), around e_u x e_w = +i on an i-face, -j on a j-face, +k on
 *     a k-face.  The march's normals point from f < v to f >= v: into the solid of ABOVE, out of the solid of BELOW.  The cap is wound
 *     with it: ABOVE wants the normal that points into the array (+axis on the low face of an axis, -axis on the high one), BELOW the
 *     opposite; where that is not the counter-clockwise one the last two corners of every emitted triangle are exchanged (ABOVE:
 *     faces 1, 2, 5; BELOW: faces 0, 3, 4).  Every edge shared by a march triangle and a cap triangle, or by two cap triangles, is
 *     then traversed in opposite directions by the two.
 * cx_cap3d builds the cap of the current extraction.  counts4: [0] lattice-point vertices, [1] cap triangles, [2] crossings the march
 * had not emitted, [3] rim edges with a crossing.  Idempotent per (extraction, faces, side); the cap is gone with the next extraction,
 * grid call, cx_reserve, cx_levels_select or seeded selection (CX_ERR_STATE from the calls below then).
 * cx_cap3d_download: the raw cap: keys = [0] + [2] uint32, tris = [1] x 3 int32 indices into the Level-0 vertices followed by the
 * cap vertices.  Either pointer may be NULL.
 * cx_postprocess3d_capped: cx_postprocess3d (flags bit 0: no clean-up) on the Level-0 mesh followed by the current cap; out_counts as
 * cx_postprocess3d.  The result is a Level-1 mesh like any other for the downloads, components, topology, boundary loops, the
 * filter, the simplifier, the clip and the plain writers; cx_level1_download_keys returns edge ids and lattice-point keys, and
 * cx_level1_sample_grid samples a lattice-point vertex at its lattice point.  cx_level1_normals and cx_level1_curvature (and the
 * writers' formats with normals) answer CX_ERR_UNSUPPORTED: a crease runs along the rim and has no single normal.
 * Refused with CX_ERR_UNSUPPORTED and a message, before anything is written: a seeded selection in force, a negative origin or a
 * reference corner (arrays carrying a margin), a positive origin (a slab of a larger volume).  Smoothing, the sharded post-pass and
 * cx_postprocess3d_mesh take no cap.  CX_ERR_INVALID for unknown face or flag bits, CX_ERR_STATE without an extraction.
 * All buffers belong to the context (counted by cx_device_bytes) and are reused; the table of the rim's crossings is sized by their
 * number, not by the mesh.  Integer atomics only: every output is the same bit for bit in every call and context.
 * cx_cap3d_info (measurement): of the current cap, info4 = {ms of cx_cap3d between HIP events on the context's stream, Level-0
 * vertices on the selected faces, slots of the table, rim points}. */
#define CX_CAP_BELOW        1u
#define CX_CAP_ALL_FACES    63u
int cx_cap3d(cx_ctx* ctx, uint32_t faces, uint32_t flags, int64_t* counts4);
int cx_cap3d_download(cx_ctx* ctx, uint32_t* keys, int32_t* tris);
int cx_cap3d_info(cx_ctx* ctx, double* info4);
int cx_postprocess3d_capped(cx_ctx* ctx, uint32_t flags, int64_t* out_counts);

/* ---- choosing isovalues: exact order statistics of the samples, and the size of the surface at many candidate values ----------------
 * Replaces the host sort behind the reference's level pickers (Percentile2DContour / Linear2DContour, multiple_2d_contour.py:84-108:
 * np.sort of all samples, every (N / breakpoints)-th of them; min and max) and answers what the reference has no call for: how large
 * the isosurface is at each of a few hundred candidate values, without marching any of them.
 *
 * cx_samples_select: exact order statistics.
 *   samples  NULL: the bound 3-D grid in its own CX_DTYPE_* (dtype, on_device and n are ignored; CX_ERR_STATE without a grid).  Else n
 *            samples (1 <= n <= 2^31) of type `dtype`, on the device (on_device != 0: any pointer aligned to its own type, e.g. a slice
 *            of a larger array, a 2-D or 4-D array) or on the host (copied into scratch of the context).
 *   ranks    nranks (1..1024) zero-based ranks in any order, repeats allowed; a rank >= n is CX_ERR_INVALID.
 *   out_values[k] = the sample of rank ranks[k] in numpy's sort order of the samples as fp32 (every type converts to fp32 exactly):
 *            -inf < finite < +inf < NaN, NaN of either sign last, -0.0 and +0.0 equal (either may be returned).  That is
 *            np.sort(x.astype(np.float32), axis=None)[ranks[k]], NaN for NaN.  Exact: no sampling, no bins.
 *   out_n_nan  the number of NaN samples (may be NULL).  Minimum and maximum are ranks 0 and n - 1 - n_nan.
 *   Method: most-significant-digit radix select on order-preserving keys of the type's own width (8-bit types one pass over the
 *   samples, 16-bit types two, fp32 three of 12 / 10 / 10 bits); ranks that fall under different key prefixes are refined together, 12
 *   prefixes to a pass.  Counts are integers, summed in 64 bits.
 *
 * cx_level_spectrum3d: the per-level size curve of the bound grid (any CX_DTYPE_*, at least 2 samples per axis), one pass over the
 * samples for all levels.
 *   values   nlevels (1..4096) finite values of fp32 magnitude, any order, duplicates allowed; the outputs are in the order of `values`
 *            and any of them may be NULL.
 *   For a value v let vcmp and near_abs be what the march compares with (vcmp = the smallest fp32 >= v, -0.0 for 0; near_abs = the fp32
 *   above 2.2e-5 |v| + 4e-8).  A sample f is LOW iff f < vcmp; a NaN is never low.
 *   n_cells      lattice cells (all 8 corners inside the array) with a low and a non-low corner
 *   n_vertices   lattice edges with one low and one non-low end, an edge running from a lattice point to one of its 7 forward
 *                neighbours (di, dj, dk) != 0 inside the array: the edges of the 6 Kuhn tetrahedra
 *   n_triangles  over the 6 tetrahedra of every cell: 1 for a tetrahedron with 1 or 3 low corners, 2 for one with 2
 *   n_near       samples inside the march's tolerance screen: fabsf(f - vcmp) <= near_abs, evaluated in fp32
 *   Where n_near[l] == 0 they are the counts of cx_extract3d(values[l]): n_vertices and n_triangles are its n_vertices and
 *   n_triangles, n_cells is its n_border_voxels (the reference's len(surface_voxels)) -- and its n_cells wherever the surface stays
 *   off the upper faces of the array: the march also keeps a cell record for a lattice point of those faces that owns a crossing
 *   edge but no whole cell, so its n_cells lies between n_cells and n_cells + n_vertices here.  Enough to size cx_reserve, or to plot
 *   the curve and trust it.  Where n_near[l] > 0 the reference's np.allclose skips may make the march emit fewer.
 *   CX_ERR_STATE without a grid, CX_ERR_INVALID for a count outside 1..4096 or a value that is NaN, infinite or beyond fp32.
 * Both calls keep their own scratch in the context (counted by cx_device_bytes) and leave the current extraction, the selected level of
 * cx_extract3d_levels and the Level-1 state as they are.  Integer atomics only: every result is the same in every call. */
int cx_samples_select(cx_ctx* ctx, const void* samples, int32_t dtype, int on_device, int64_t n, const int64_t* ranks, int32_t nranks,
                      double* out_values, int64_t* out_n_nan);
int cx_level_spectrum3d(cx_ctx* ctx, const double* values, int32_t nlevels, int64_t* n_cells, int64_t* n_vertices, int64_t* n_triangles,
                        int64_t* n_near);

/* ---- preparing the volume: a separable filter with a stride per axis, on the device ----------------------------------------------
 * Smoothing (a Gaussian), binning (a block mean) and one step of a pyramid are all one operation: per axis a row of weights, an origin
 * and a stride.  The reference has no call for it; a caller ran scipy.ndimage on the host and uploaded again.
 *
 * cx_grid_filter3d
 *   samples  NULL: the bound 3-D grid in its own CX_DTYPE_* (dtype, on_device and the shape are ignored; CX_ERR_STATE without a grid).
 *            Else n0 n1 n2 samples of type `dtype` (every axis >= 1: a 2-D array goes in as 1 x n x m; at most 2^31 samples), on the
 *            device (any pointer aligned to its own type) or on the host (copied into scratch of the context).  The pointer
 *            cx_grid_filter3d_result handed out is a legal input (a pyramid on the device): that result is consumed, the new one
 *            takes its place.
 *   axes[a]  for axis a: n_weights fp32 weights (1..129), origin (0 .. n_weights-1) and stride (1 .. n_a).  weights == NULL or
 *            n_weights == 0: the axis is not filtered, only the stride applies (out[i] = in[i stride] as fp32, origin ignored).
 *   The passes run axis 2, then axis 1, then axis 0, each on the fp32 result of the one before.  Per axis, with n the length of the
 *   axis going in, the length coming out is m = ceil(n / stride) and
 *       out[i] = (float) sum over k = 0 .. n_weights-1 of (double)weights[k] * (double)in[src(i stride + k - origin)]
 *   summed in double with k ascending from +0.0 and rounded to fp32 once per pass.  (The product of two fp32 numbers is exact in double,
 *   so a fused multiply-add gives the same double as a multiply and an add: the bits do not depend on how the sum is compiled.)
 *   src is the boundary rule of `mode`: CX_FILTER_NEAREST clamps the index to [0, n-1]; CX_FILTER_REFLECT takes p = j mod 2n
 *   (non-negative) and reads p < n ? p : 2n-1-p, so a radius beyond the axis is legal; CX_FILTER_CONSTANT reads (float)cval outside.
 *   These are scipy.ndimage's 'nearest', 'reflect' and 'constant'.
 *   out_device  not NULL: m0 m1 m2 fp32 values are written there (device memory of the caller; CX_ERR_INVALID if it overlaps the
 *            input), and the context keeps no result.  NULL: the result goes into a buffer the context owns (counted by
 *            cx_device_bytes, reused by the next call) and stays pending until the next call or cx_grid_filter3d_bind.
 *   out_host    not NULL: also receives a copy.  out_shape (may be NULL) receives {m0, m1, m2}.
 *   CX_ERR_INVALID: an unknown mode or sample type, a NaN or infinite cval, n_weights, origin or stride outside their ranges, a shape
 *   outside its range.
 * cx_grid_filter3d_result: the pending result, device pointer and shape; CX_ERR_STATE when none is pending.
 * cx_grid_filter3d_bind: the pending result becomes the bound grid -- CX_DTYPE_F32, owned by the context, of the result's shape -- as
 *   if it had been uploaded: the float64 originals, the current extraction, the levels and the Level-1 state of the grid before are
 *   gone and the grid the context owned before is released.  No host copy of the filtered samples ever exists.  Afterwards nothing is
 *   pending (a second bind or a _result answers CX_ERR_STATE).  A result the march does not take (an axis shorter than 2, more than
 *   2^29 samples) is refused as an upload of that shape is, and stays pending.
 * Filtering without binding leaves the bound grid, the current extraction, the selected level of cx_extract3d_levels and the Level-1
 * state as they are.  No atomics: every call gives the same bits. */
#define CX_FILTER_NEAREST  0
#define CX_FILTER_REFLECT  1
#define CX_FILTER_CONSTANT 2
typedef struct cx_filter_axis { const float* weights; int32_t n_weights; int32_t origin; int32_t stride; } cx_filter_axis;
int cx_grid_filter3d(cx_ctx* ctx, const void* samples, int32_t dtype, int on_device, int64_t n0, int64_t n1, int64_t n2,
                     const cx_filter_axis axes[3], int32_t mode, double cval, void* out_device, float* out_host, int64_t out_shape[3]);
int cx_grid_filter3d_result(cx_ctx* ctx, void** out_device, int64_t out_shape[3]);
int cx_grid_filter3d_bind(cx_ctx* ctx);

/* ---- distance fields: the exact Euclidean distance transform of a thresholded volume, on the device ---------------------------------
 * What a caller with a segmented volume ran scipy.ndimage.distance_transform_edt for: a smooth field from a mask, offset surfaces,
 * dilation and erosion by a ball, thickness maps.  The reference has no call for it.
 *
 * cx_grid_distance3d
 *   samples  NULL: the bound 3-D grid in its own CX_DTYPE_* (dtype, on_device and the shape are ignored; CX_ERR_STATE without a grid).
 *            Else n0 n1 n2 samples of type `dtype` (every axis >= 1, at most 2^29 samples), on the device (any pointer aligned to its
 *            own type) or on the host (copied into scratch of the context).  The pointer cx_grid_distance3d_result handed out is a
 *            legal input (the second step of an opening or closing): that result is consumed, the new one takes its place.
 *   value    a sample f is LOW iff (double)f < value; a NaN is never low.  This is the march's own classification.
 *   sampling three doubles s0, s1, s2, each finite and > 0; NULL: 1, 1, 1.  w_a = s_a * s_a, rounded once, must be a normal double.
 *   side     CX_DIST_BELOW: the sites are the samples that are not low; the result is 0 there and the distance to the nearest site at
 *            the low samples (scipy's edt(f < value)).  CX_DIST_ABOVE: the sites are the low samples (edt(f >= value)).
 *            CX_DIST_SIGNED: above minus below; it has the sign of f - value, so marching it at 0 winds the surface as marching f at
 *            `value` does.
 *   The squared distance is a minimum per axis, last axis first, all in double, (a - b)^2 the exact integer converted to double (exact
 *   below 2^53), fl one IEEE rounding:
 *       g2[i,j,k] = min over the sites (i,j,k') of the row of fl(w2 (k-k')^2), +inf for a row without a site
 *       g1[i,j,k] = min over j' of fl(g2[i,j',k] + fl(w1 (j-j')^2))
 *       g0[i,j,k] = min over i' of fl(g1[i',j,k] + fl(w0 (i-i')^2))
 *   With unit sampling every value is an exact integer and g0 is the squared Euclidean distance to the nearest site.  With another
 *   sampling it is one well-defined double per sample: a minimum does not depend on the order of its candidates, and the kernels skip
 *   a candidate only where fl(w d^2) alone is not below the best so far.  A volume without a site gives +inf everywhere.
 *   out_kind CX_DIST_OUT_SQUARED_F64: g0 as doubles; with CX_DIST_SIGNED g0 of ABOVE minus g0 of BELOW (one of them is 0 everywhere).
 *            CX_DIST_OUT_F32: (float)sqrt(g0), the double square root correctly rounded, then rounded to fp32; with CX_DIST_SIGNED
 *            (float)(sqrt(gA) - sqrt(gB)).
 *            CX_DIST_OUT_MASK_U8: g0 <= radius2 ? 1 : 0 as uint8 (radius2 finite and >= 0; refused with CX_DIST_SIGNED).  The mask of
 *            BELOW is the dilation of {f >= value} by the ball of squared radius radius2, 1 minus the mask of ABOVE its erosion.
 *   out_device  not NULL: n0 n1 n2 values of the kind are written there (device memory of the caller, aligned to the kind's type;
 *            CX_ERR_INVALID if it overlaps the input), and the context keeps no result.  NULL: the result goes into a buffer the
 *            context owns (counted by cx_device_bytes, reused by the next call) and stays pending until the next cx_grid_distance3d
 *            or cx_grid_distance3d_bind.  The slot is the distance transform's own: cx_grid_filter3d and this call do not disturb
 *            each other's pending result.
 *   out_host    not NULL: also receives a copy.
 *   n_sites     (may be NULL) the number of sites, an exact count: samples that are not low (BELOW), low samples (ABOVE), the smaller
 *            of the two (SIGNED).  0 iff the distances are infinite.  The call returns after the stream has run it.
 *   CX_ERR_INVALID: a NaN or infinite value, a bad sampling, side, kind or radius2, an unknown sample type, a shape outside its range.
 * cx_grid_distance3d_result: the pending result: device pointer, shape, kind and n_sites; CX_ERR_STATE when none is pending.
 * cx_grid_distance3d_bind: the pending CX_DIST_OUT_F32 or CX_DIST_OUT_MASK_U8 result becomes the bound grid (CX_DTYPE_F32 / CX_DTYPE_U8),
 *   owned by the context, with every reset of an upload, as cx_grid_filter3d_bind does it.  Refused with CX_ERR_INVALID, the result
 *   left pending: a CX_DIST_OUT_SQUARED_F64 result, a result that holds an infinity (n_sites == 0), an axis shorter than 2.
 *   CX_ERR_STATE when nothing is pending.
 * A call without bind leaves the bound grid, the current extraction, the selected level, the Level-1 state and the cap as they are.
 * No atomics on floating-point values: every call gives the same bits.  tests/distance_ref.py restates all of it in numpy. */
#define CX_DIST_BELOW  0
#define CX_DIST_ABOVE  1
#define CX_DIST_SIGNED 2
#define CX_DIST_OUT_SQUARED_F64 0
#define CX_DIST_OUT_F32         1
#define CX_DIST_OUT_MASK_U8     2
int cx_grid_distance3d(cx_ctx* ctx, const void* samples, int32_t dtype, int on_device, int64_t n0, int64_t n1, int64_t n2,
                       double value, const double sampling[3], int32_t side, int32_t out_kind, double radius2,
                       void* out_device, void* out_host, int64_t* n_sites);
int cx_grid_distance3d_result(cx_ctx* ctx, void** out_device, int64_t out_shape[3], int32_t* out_kind, int64_t* n_sites);
int cx_grid_distance3d_bind(cx_ctx* ctx);

/* ---- labels: the connected components of a thresholded volume, on the device -----------------------------------------------------------
 * What a caller with a segmented volume ran scipy.ndimage.label for, and what follows from it: voxel counts, boxes and centroids per
 * component, "keep the largest object", "remove the specks", "fill the enclosed holes", "drop what touches the rim".  The reference has
 * no call for it.  (The components of the Level-1 MESH are another matter: a solid with a cavity is one voxel object and two surfaces.)
 *
 * cx_grid_label3d
 *   samples, dtype, on_device, n0 n1 n2: as in cx_grid_distance3d.  NULL: the bound 3-D grid in its own type (CX_ERR_STATE without one);
 *            else a host or device pointer of any CX_DTYPE_*, every axis >= 1, at most 2^29 samples.  The pointer
 *            cx_grid_label3d_select_result handed out is a legal input (CX_DTYPE_U8, on the device).
 *   value    a sample f is LOW iff (double)f < value; a NaN is never low.  This is the march's own classification.
 *   side     CX_LABEL_HIGH: the samples that are not low are labelled.  CX_LABEL_LOW: the low ones are.
 *   connectivity  1, 2 or 3: two labelled samples are neighbours when their index offsets are each in {-1, 0, 1} and differ from 0 on
 *            at most `connectivity` axes: 6, 18 or 26 neighbours, scipy's generate_binary_structure(3, connectivity).  Neighbours
 *            never wrap: the last sample of a row and the first of the next row are not neighbours, nor are those of two planes.
 *   The result: n0 n1 n2 int32 labels, 0 on the samples that are not labelled, else 1 .. K.  Components are numbered by the linear
 *   index (C order) of their first sample: component 1 holds the labelled sample with the smallest linear index, component c + 1 the
 *   smallest one that is in none of 1 .. c.  This is scipy.ndimage.label's own numbering, and it makes the labels a pure function of
 *   the inputs: no order of unions can show in them.
 *   out_device  not NULL: the labels are written there (device memory of the caller, aligned to 4; CX_ERR_INVALID if it overlaps the
 *            input), and the context keeps no result.  NULL: they go into a buffer the context owns (counted by cx_device_bytes, reused
 *            by the next call) and stay pending until the next cx_grid_label3d.  The slot is the labels' own: cx_grid_filter3d,
 *            cx_grid_distance3d and this call do not disturb each other's pending results.
 *   out_host    not NULL: also receives a copy.   n_components (may be NULL): K.  The call returns after the stream has run it.
 *   CX_ERR_INVALID: a NaN or infinite value, an unknown side, connectivity or sample type, a shape outside its range.
 * cx_grid_label3d_result: the pending labels: device pointer, shape, side, connectivity and K; CX_ERR_STATE when none are pending.
 * cx_grid_label3d_measures: one cx_label_component per component of the pending labels, record c - 1 for label c, computed on the
 *   first request.  Every field is an exact integer:
 *     voxels   the number of samples of the component          first    its smallest linear index
 *     sum[a]   the sum of its samples' indices along axis a (the centroid is sum / voxels)
 *     lo[a], hi[a]  the smallest and largest index along axis a (its box, both ends included)
 *     rim      bit 2a set: the component has a sample at index 0 of axis a; bit 2a + 1: one at index n_a - 1
 *     reserved 0
 *   CX_ERR_STATE when no labels are pending, CX_ERR_INVALID when capacity < K; K == 0 is served with any capacity.  Integer atomics
 *   only: two calls give the same bytes.
 * cx_grid_label3d_select: keep is n_keep == K + 1 host bytes indexed by label, keep[0] for the samples without one; the result is a
 *   uint8 mask, 1 where keep[label] != 0, written to out_device (memory of the caller; CX_ERR_INVALID if it overlaps the labels) or,
 *   out_device NULL, into a second buffer of the label state, where it stays pending until the next select or cx_grid_label3d_bind.
 *   out_host also receives a copy; n_voxels (may be NULL) the exact count of ones.  CX_ERR_STATE without pending labels,
 *   CX_ERR_INVALID for another n_keep.
 * cx_grid_label3d_select_result: the pending mask: device pointer, shape and count; CX_ERR_STATE when none is pending.  The pointer is a
 *   legal `samples` of cx_grid_distance3d and of cx_grid_label3d (CX_DTYPE_U8, on the device).
 * cx_grid_label3d_bind: the pending mask becomes the bound grid (CX_DTYPE_U8, owned by the context) with every reset of an upload, as
 *   cx_grid_distance3d_bind does it.  CX_ERR_INVALID, the mask left pending, for an axis shorter than 2; CX_ERR_STATE without a pending
 *   mask.  The labels stay pending: only a later cx_grid_label3d replaces them.
 * A call without bind leaves the bound grid, the current extraction, the selected level, the Level-1 state, the cap and the filter's
 * and the distance transform's pending results as they are.  tests/label_ref.py restates all of it in numpy. */
#define CX_LABEL_HIGH 0
#define CX_LABEL_LOW  1
typedef struct cx_label_component {
    int64_t voxels;
    int64_t first;
    int64_t sum[3];
    int32_t lo[3];
    int32_t hi[3];
    uint32_t rim;
    uint32_t reserved;
} cx_label_component;      /* 72 bytes */
int cx_grid_label3d(cx_ctx* ctx, const void* samples, int32_t dtype, int on_device, int64_t n0, int64_t n1, int64_t n2,
                    double value, int32_t side, int32_t connectivity, int32_t* out_device, int32_t* out_host, int64_t* n_components);
int cx_grid_label3d_result(cx_ctx* ctx, int32_t** labels_device, int64_t shape[3], int32_t* side, int32_t* connectivity, int64_t* n_components);
int cx_grid_label3d_measures(cx_ctx* ctx, cx_label_component* out_host, int64_t capacity);
int cx_grid_label3d_select(cx_ctx* ctx, const uint8_t* keep, int64_t n_keep, uint8_t* out_device, uint8_t* out_host, int64_t* n_voxels);
int cx_grid_label3d_select_result(cx_ctx* ctx, uint8_t** mask_device, int64_t shape[3], int64_t* n_voxels);
int cx_grid_label3d_bind(cx_ctx* ctx);

/* ---- resampling through an affine map: regrid, zoom, reslice, on the device ----------------------------------------------------------
 * What a caller ran scipy.ndimage.affine_transform or zoom for: a second volume on the marched volume's lattice, anisotropic voxels made
 * isotropic, a scan rotated into a registered frame, one oblique plane of samples.  The reference has no call for it.
 *
 * cx_grid_resample3d
 *   samples, dtype, on_device, n0 n1 n2: as in cx_grid_filter3d.  NULL: the bound 3-D grid in its own type (CX_ERR_STATE without one);
 *            else a host or device pointer of any CX_DTYPE_*, every axis >= 1, at most 2^31 samples.  The pointer
 *            cx_grid_resample3d_result handed out is a legal input: that result is consumed, the new one takes its place.
 *   matrix   9 doubles M[a][k] = matrix[3 a + k], offset 3 doubles, each finite and at most 2^20 in magnitude.  The matrix maps the
 *            OUTPUT index to the INPUT index (scipy.ndimage.affine_transform's convention).
 *   out_shape  m0 m1 m2, each >= 1, at most 2^31 samples in all.
 *   For the output index i0 i1 i2 the source coordinate on input axis a is
 *       c_a = ((offset[a] + M[a][0] i0) + M[a][1] i1) + M[a][2] i2
 *   in double, every product and every sum rounded on its own: no fused multiply-add (a product of two doubles is not exact, so
 *   contraction would change bits).  With the bound on the entries every floor of c fits an int64 and c - floor c is exact.
 *   src is the boundary rule of `mode` per index, as in cx_grid_filter3d: CX_FILTER_NEAREST clamps, CX_FILTER_REFLECT takes p = j mod 2n
 *   and reads p < n ? p : 2n-1-p, CX_FILTER_CONSTANT reads cval when any of the three indices is outside.  These are scipy's 'nearest',
 *   'reflect' and 'grid-constant' (scipy's plain 'constant' is another rule and is not offered).
 *   order 0  j_a = floor(c_a + 0.5); the output is the sample at src of j in the input's own type, its bytes copied (a mask or a label
 *            volume stays what it is).  cval must be a value of that type (CX_ERR_INVALID otherwise).
 *   order 1  trilinear: lo_a = floor(c_a), t_a = c_a - lo_a; the corner samples s[d0][d1][d2] at src of lo_a + d_a are widened to double
 *            (under CX_FILTER_CONSTANT the fill is (double)(float)cval); lerp(a, b, t) = (t == 0) ? a : a + t * (b - a), each operation
 *            rounded on its own; input axis 2 is reduced first (four lerps with t_2), then axis 1 (two), then axis 0 (one); the result
 *            is rounded to fp32 once.  The output is CX_DTYPE_F32.  With t == 0 the high corner does not enter, so an identity map
 *            reproduces infinite samples.
 *   n_outside  (may be NULL) the number of output samples with some c_a < 0 or c_a > n_a - 1: how much of the result is boundary rule
 *            and not data.  An exact integer, the same in every call.  The call returns after the stream has run it.
 *   out_device  not NULL: the m0 m1 m2 values are written there (device memory of the caller, aligned to the output type;
 *            CX_ERR_INVALID if it overlaps the input), and the context keeps no result.  NULL: the result goes into a buffer the context
 *            owns (counted by cx_device_bytes, reused by the next call) and stays pending until the next cx_grid_resample3d or
 *            cx_grid_resample3d_bind.  The slot is this call's own: cx_grid_filter3d, cx_grid_distance3d, cx_grid_label3d and this call
 *            do not disturb each other's pending results, and the pending pointer is a legal `samples` of all four.
 *   out_host    not NULL: also receives a copy.
 *   CX_ERR_INVALID: an unknown order, mode or sample type, a NaN or infinite cval, a matrix or offset entry that is not finite or
 *   exceeds 2^20 in magnitude, a shape outside its range.
 * cx_grid_resample3d_result: the pending result: device pointer, shape, its CX_DTYPE_* and n_outside; CX_ERR_STATE when none is pending.
 * cx_grid_resample3d_bind: the pending result becomes the bound grid -- CX_DTYPE_F32 for order 1, the input's own type for order 0, owned
 *   by the context -- with every reset of an upload, as cx_grid_filter3d_bind does it.  A result the march does not take (an axis
 *   shorter than 2, more than 2^29 samples) is refused as an upload of that shape is, and stays pending.  CX_ERR_STATE when nothing is
 *   pending.
 * A call without bind leaves the bound grid, the current extraction, the selected level and the Level-1 state as they are.  The only
 * atomic is the integer add of n_outside: every call gives the same bits.  tests/resample_ref.py restates all of it in numpy. */
int cx_grid_resample3d(cx_ctx* ctx, const void* samples, int32_t dtype, int on_device, int64_t n0, int64_t n1, int64_t n2,
                       const double matrix[9], const double offset[3], const int64_t out_shape[3],
                       int32_t order, int32_t mode, double cval, void* out_device, void* out_host, int64_t* n_outside);
int cx_grid_resample3d_result(cx_ctx* ctx, void** out_device, int64_t out_shape[3], int32_t* out_dtype, int64_t* n_outside);
int cx_grid_resample3d_bind(cx_ctx* ctx);

/* ---- rank filters: median, percentile, grey minimum and maximum of a volume, on the device ------------------------------------------
 * What a caller ran scipy.ndimage.median_filter, rank_filter, percentile_filter, minimum_filter or maximum_filter for: noise removed
 * with the edges kept before the threshold, the labelling and the distance transform see them; on a uint8 mask, the majority filter.
 * The reference has no call for it.
 *
 * cx_grid_rank3d
 *   samples, dtype, on_device, n0 n1 n2: as in cx_grid_resample3d.  NULL: the bound 3-D grid in its own type (CX_ERR_STATE without one);
 *            else a host or device pointer of any CX_DTYPE_*, aligned to its own type, every axis >= 1, at most 2^31 samples.  The
 *            pointer cx_grid_rank3d_result handed out is a legal input: that result is consumed, the new one takes its place.
 *   size     the footprint's box s0 s1 s2, each 1..7; origin o0 o1 o2, each 0 .. s_a - 1 (scipy's centre is s_a / 2; scipy's `origin`
 *            argument is o_a - s_a / 2).
 *   footprint  NULL: the whole box.  Else s0 s1 s2 bytes in C order on the host, non-zero = the offset belongs to the footprint.
 *            W = the number of offsets that belong to it (>= 1).
 *   rank     0 .. W - 1.
 *       window(i) = { in[src0(i0 + d0 - o0), src1(i1 + d1 - o1), src2(i2 + d2 - o2)] : d in the footprint }
 *       out[i]    = the element of window(i) at position `rank` in ascending order
 *   in the input's own type and shape.  The order is a total order on the samples' bits: integers by value; floats as
 *   -inf < negative finite < -0.0 < +0.0 < positive finite < +inf < NaN, every NaN, whatever its sign and payload, one largest element.
 *   A selected NaN comes out as the canonical quiet NaN of the type (0x7FC00000, 0x7E00 half, 0x7FC0 bfloat16); every other output is
 *   the bits of a sample (or of cval).  Equal elements have equal bits, so no tie rule is needed.  (The keys of cx_samples_select fold
 *   -0.0 onto +0.0 and have no inverse; these do not.)
 *   src is the boundary rule of `mode` per index, as in cx_grid_filter3d: CX_FILTER_NEAREST clamps, CX_FILTER_REFLECT takes p = j mod 2n
 *   and reads p < n ? p : 2n-1-p (a window wider than the axis is legal), under CX_FILTER_CONSTANT an element whose index is off the
 *   array on any axis is cval.  cval must be finite and a value of the sample type (CX_ERR_INVALID otherwise), in every mode.
 *   With origin = o - s / 2 this is scipy.ndimage.rank_filter(in, rank, footprint=..., mode='nearest' | 'reflect' | 'constant', cval=...,
 *   origin=...); rank W / 2 is median_filter, 0 and W - 1 are minimum_filter and maximum_filter.
 *   out_device  not NULL: the n0 n1 n2 values are written there (device memory of the caller, aligned to the sample type;
 *            CX_ERR_INVALID if it overlaps the input), and the context keeps no result.  NULL: the result goes into a buffer the context
 *            owns (counted by cx_device_bytes, reused by the next call) and stays pending until the next cx_grid_rank3d or
 *            cx_grid_rank3d_bind.  The slot is this call's own: cx_grid_filter3d, cx_grid_distance3d, cx_grid_label3d,
 *            cx_grid_resample3d and this call do not disturb each other's pending results, and the pending pointer is a legal `samples`
 *            of all five.
 *   out_host    not NULL: also receives a copy.  The call returns after the stream has run it.
 *   CX_ERR_INVALID: an unknown mode or sample type, a size outside 1..7, an origin outside 0 .. s - 1, an empty footprint, a rank
 *   outside 0 .. W - 1, a cval that is not finite or not a value of the sample type, a shape outside its range, an output that overlaps
 *   the input.
 * cx_grid_rank3d_result: the pending result: device pointer, shape and its CX_DTYPE_*; CX_ERR_STATE when none is pending.
 * cx_grid_rank3d_bind: the pending result becomes the bound grid in the input's own type, owned by the context, with every reset of an
 *   upload, as cx_grid_filter3d_bind does it.  A result the march does not take (an axis shorter than 2, more than 2^29 samples) is
 *   refused as an upload of that shape is, and stays pending.  Afterwards nothing is pending.  CX_ERR_STATE when nothing is pending.
 * A call without bind leaves the bound grid, the current extraction, the selected level and the Level-1 state as they are.  No
 * floating-point arithmetic and no atomics: every call gives the same bits.  tests/rank_ref.py restates all of it in numpy. */
int cx_grid_rank3d(cx_ctx* ctx, const void* samples, int32_t dtype, int on_device, int64_t n0, int64_t n1, int64_t n2,
                   const int32_t size[3], const int32_t origin[3], const uint8_t* footprint /* size[0]*size[1]*size[2] bytes, C order, host; NULL = full box */,
                   int32_t rank, int32_t mode, double cval, void* out_device, void* out_host);
int cx_grid_rank3d_result(cx_ctx* ctx, void** out_device, int64_t out_shape[3], int32_t* out_dtype);
int cx_grid_rank3d_bind(cx_ctx* ctx);

/* ---- reconstruction: grey morphological reconstruction of a volume, on the device ------------------------------------------------------
 * Reconstruction by dilation of a marker g under a mask f: the largest array R <= f that dominates min(g, f) and in which every sample
 * is reached from it by a path of neighbours along which R does not increase.  What a caller ran skimage.morphology.reconstruction,
 * h_maxima, local_maxima or scipy.ndimage.binary_propagation for: bumps shallower than h removed with the edges kept, the regional
 * maxima of a distance field as markers, grey fill-holes and grey clear-border.  The reference has no call for it.
 *
 * cx_grid_reconstruct3d
 *   mask, dtype, on_device, n0 n1 n2: as the samples of cx_grid_rank3d.  NULL: the bound 3-D grid in its own type (CX_ERR_STATE without
 *            one; the marker array is then on the device); else a host or device pointer of any CX_DTYPE_*, aligned to its own type,
 *            every axis >= 1, at most 2^31 samples (CX_ERR_UNSUPPORTED beyond).  The pointer cx_grid_reconstruct3d_result handed out
 *            is a legal input.
 *   Every comparison is made on the keys of the rank filters: integers by value; floats as -inf < negative finite < -0.0 < +0.0 <
 *   positive finite < +inf < NaN, every NaN one largest element that comes out as the canonical quiet NaN of the type.  The result is a
 *   minimum or maximum of values of the mask and the marker, in the samples' own type.
 *   method   CX_RECON_DILATION: the marker grows upward under the mask.  CX_RECON_EROSION: the dual: the smallest R >= f below
 *            max(g, f) in which every sample is reached by a path along which R does not decrease (the same on the complemented keys).
 *   connectivity  1, 2 or 3: 6, 18 or 26 neighbours, as in cx_grid_label3d.
 *   marker_kind
 *     CX_RECON_MARKER_ARRAY  `marker` is a second array of the mask's shape, type and residency (CX_ERR_INVALID when NULL), clamped into
 *            the mask: min(g, f) for dilation, max(g, f) for erosion.  stats->n_clamped counts the samples the clamp changed.
 *     CX_RECON_MARKER_SHIFT  marker = mask - h (dilation) or mask + h (erosion), h finite and > 0: h-maxima and h-minima.  Integer types:
 *            h an integer, the arithmetic saturates in the type.  Float types: (double)sample -+ h in float64, rounded once to the
 *            sample type (to nearest even); a NaN stays one.  No second array.
 *     CX_RECON_MARKER_STEP   marker = the sample's predecessor (dilation) or successor (erosion) in the order of the keys: integers
 *            v - 1 or v + 1, saturating; floats the next value of the type, -0.0 and +0.0 being neighbours, saturating at -inf (dilation)
 *            or +inf (erosion); the predecessor of NaN is +inf, its successor NaN.  With CX_RECON_OUT_CHANGED: the regional extrema.
 *     CX_RECON_MARKER_RIM    marker = mask on the faces of the array named by the 6 bits of `faces` (bit 0: i = 0, 1: i = n0-1, 2: j = 0,
 *            3: j = n1-1, 4: k = 0, 5: k = n2-1; 1..63), elsewhere the bottom (dilation) or the top (erosion) of the order of the
 *            keys, which does not survive: every sample is connected to the rim.  Grey clear-border and grey fill-holes.
 *   out_kind CX_RECON_OUT_VALUES: the reconstruction in the samples' own type.  CX_RECON_OUT_CHANGED: uint8, 1 where the key of the
 *            result differs from the key of the mask: the regional extrema, the support of the h-domes, what was filled or cleared.
 *            One case is defined apart: an integer array that is everywhere the extreme value of its type (the minimum for dilation,
 *            the maximum for erosion) has no predecessor to step to; under CX_RECON_MARKER_STEP it is one regional extremum and the
 *            CHANGED mask is all ones (n_changed stays the count of result != mask, 0).
 *   out_device, out_host  as in cx_grid_rank3d: a caller's device buffer (n0 n1 n2 samples, or bytes for CHANGED) may not overlap the
 *            mask or the marker (CX_ERR_INVALID) and leaves the context without a result; NULL: the result goes into a buffer the
 *            context owns and stays pending until the next cx_grid_reconstruct3d or cx_grid_reconstruct3d_bind, in a sixth slot:
 *            the pending results of cx_grid_filter3d, cx_grid_distance3d, cx_grid_label3d, cx_grid_resample3d and cx_grid_rank3d
 *            are not disturbed, and the pending pointer (CX_DTYPE_U8 for CHANGED) is a legal input of all of them.  out_host not
 *            NULL: also receives a copy.  The call returns after the stream has run it.
 *   stats    may be NULL.  n_changed: the samples where result != mask; n_clamped: see CX_RECON_MARKER_ARRAY.  Both exact and the same
 *            in every call.  rounds (kernel launches that visited a tile) and tile_visits are informational and may differ from call
 *            to call: tiles of one launch read each other's samples while they are written, which changes how soon a value arrives,
 *            never the result.
 *   CX_ERR_INVALID: an unknown method, marker kind, output kind, connectivity or sample type, faces outside 1..63 with
 *   CX_RECON_MARKER_RIM, an h that is not finite, not above 0 or (integer types) not an integer, a NULL marker with
 *   CX_RECON_MARKER_ARRAY, an axis below 1, an output that overlaps an input.  CX_ERR_UNSUPPORTED: more than 2^31 samples.
 *   CX_ERR_HIP with a message if tiles were still active after as many rounds as the array has samples (no correct run gets there).
 * cx_grid_reconstruct3d_result: the pending result: device pointer, shape, its CX_DTYPE_* and CX_RECON_OUT_*; CX_ERR_STATE when none is
 *   pending.
 * cx_grid_reconstruct3d_bind: the pending result becomes the bound grid (the samples' type, or CX_DTYPE_U8 for CHANGED), owned by the
 *   context, with every reset of an upload, as cx_grid_rank3d_bind does it.  A result the march does not take (an axis shorter than 2,
 *   more than 2^29 samples) is refused as an upload of that shape is, and stays pending.  CX_ERR_STATE when nothing is pending.
 * A call without bind leaves the bound grid, the current extraction, the selected level and the Level-1 state as they are.  The
 * result is the unique fixed point of v = min(f, max(v, neighbours of v)) above the clamped marker, so every call gives the same bits
 * whatever order the device works in.  tests/recon_ref.py restates all of it in numpy. */
#define CX_RECON_DILATION 0
#define CX_RECON_EROSION  1
#define CX_RECON_MARKER_ARRAY 0
#define CX_RECON_MARKER_SHIFT 1
#define CX_RECON_MARKER_STEP  2
#define CX_RECON_MARKER_RIM   3
#define CX_RECON_OUT_VALUES  0
#define CX_RECON_OUT_CHANGED 1
typedef struct cx_recon_stats { int64_t n_changed, n_clamped, rounds, tile_visits; } cx_recon_stats;
int cx_grid_reconstruct3d(cx_ctx* ctx, const void* mask, int32_t dtype, int on_device, int64_t n0, int64_t n1, int64_t n2,
                          const void* marker, int32_t marker_kind, double h, int32_t faces, int32_t method, int32_t connectivity,
                          int32_t out_kind, void* out_device, void* out_host, cx_recon_stats* stats);
int cx_grid_reconstruct3d_result(cx_ctx* ctx, void** out_device, int64_t out_shape[3], int32_t* out_dtype, int32_t* out_kind);
int cx_grid_reconstruct3d_bind(cx_ctx* ctx);

/* ---- watershed: marker-based watershed of a volume, on the device ----------------------------------------------------------------------
 * The labels of the markers flooded over a relief: Meyer's flooding with first-in first-out lakes, written as a path cost so that the
 * ties have one answer.  The last step of the chain threshold, distance field, h-maxima, regional maxima, labels: it splits grains,
 * cells or pores that touch.  What a caller ran skimage.segmentation.watershed or scipy.ndimage.watershed_ift for -- but their ties
 * differ from each other and from these, so neither is an equality oracle.
 *
 * cx_grid_watershed3d
 *   relief   the samples f: NULL = the bound grid (CX_ERR_STATE when none is bound); else n0 n1 n2 samples of CX_DTYPE_* `dtype` in device
 *            memory (on_device != 0) or host memory, every axis >= 1, at most 2^31 samples (CX_ERR_UNSUPPORTED beyond).
 *   markers  int32, the relief's shape, and where the relief is: device memory when the relief is on the device or the bound grid, host
 *            memory with a host relief.  A value above 0 is a label; everything else means "no marker".  One label may sit on many
 *            samples, connected or not.  CX_ERR_INVALID when NULL.
 *   region   NULL = every sample is inside; else uint8 of the same shape and residency, non-zero = inside.
 *   connectivity  1, 2 or 3: 6, 18 or 26 neighbours, as in cx_grid_label3d.
 *   direction  CX_WATERSHED_RISING floods from low values up.  CX_WATERSHED_FALLING is the dual: the same kernels on complemented keys,
 *            as CX_RECON_EROSION does it, so that a distance field is flooded from its maxima without being negated.
 *   Domain.  The samples that are inside the region and are not NaN (NaN is tested on the sample, before any complement).  A sample
 *            outside the domain always gets label 0.  A marker outside the domain is ignored and counted in n_ignored.
 *   Comparisons.  All on keys: the sample's bits mapped to an unsigned integer whose order is -inf < ... < -0.0 < +0.0 < ... < +inf for
 *            floats and the value's order for integers (the keys of cx_grid_rank3d); FALLING compares key ^ ones (of the key's width).
 *            No arithmetic is done on samples.
 *   Arrival cost.  A path is a sequence of neighbours inside the domain that starts on a marker sample s and passes through no other
 *            marker sample.  Its cost is a pair (P, d), built step by step: at s it is (key(s), 0); a step onto v from cost (P, d)
 *            gives (key(v), 0) if key(v) > P (a climb to a new level), else (P, d + 1) (staying in the lake at level P).  W(v) is the
 *            lexicographically least cost over all such paths to v, "unreached" when there is none.  P is the level at which the flood
 *            wets v, d the number of steps since that level was entered.  Equivalently W is the unique fixed point of
 *            W(v) = min over neighbours u of step(W(u), v) with the marker samples held at (key, 0); unique because a step strictly
 *            increases the pair.
 *   Labels.  A marker sample keeps its label.  Every other reached sample takes the label of ONE neighbour: the one with the least W,
 *            among neighbours of equal W the one with the smallest linear index in C order.  That neighbour's W is strictly below the
 *            sample's own, so the rule is well founded.  Unreached samples and samples outside the domain get 0.  The labels are a pure
 *            function of the inputs: the same bytes in every call, whatever order the device works in.  The index tie-break is a
 *            stated BIAS towards low indices on exact ties (a plateau between two markers at equal distance goes to the side whose
 *            samples come first in C order); it is what makes the answer unique, not a claim about the data.
 *   out_device, out_host  int32 labels.  A caller's device buffer (n0 n1 n2 int32, aligned to 4, else CX_ERR_INVALID) may not overlap
 *            a device input (CX_ERR_INVALID) and leaves the context without a result; NULL: the labels go into a buffer the context
 *            owns and stay pending until the next cx_grid_watershed3d, in a seventh slot of its own: the pending results of
 *            cx_grid_filter3d, cx_grid_distance3d, cx_grid_label3d (and its select), cx_grid_resample3d, cx_grid_rank3d and
 *            cx_grid_reconstruct3d are not disturbed, and their pending pointers are legal inputs here (labels as markers, a
 *            select mask as region, a distance field or reconstruction as relief).  This call's own pending result is a legal
 *            `markers` of the next call.  out_host not NULL: also receives a copy.  The call returns after the stream has run it.
 *   stats    may be NULL.  n_labelled: samples with a label above 0; n_unreached: samples INSIDE the domain that no path reaches;
 *            n_ignored: marker samples outside the domain; n_markers: marker samples inside it.  These four are exact and the same in
 *            every call.  rounds (kernel launches that visited a tile), tile_visits and jump_rounds (pointer-doubling passes that
 *            resolved the labels) are informational and may differ from call to call.
 *   No marker inside the domain is not an error: CX_OK, all labels 0.
 *   CX_ERR_INVALID: an unknown sample type, an axis below 1, NULL markers, a connectivity outside 1..3, an unknown direction, an output
 *   that overlaps an input, an out_device not aligned to 4.  CX_ERR_UNSUPPORTED: more than 2^31 samples.  CX_ERR_STATE: NULL relief
 *   with no grid bound.  CX_ERR_HIP with a message if tiles were still active after as many rounds as the array has samples, or the
 *   labels unresolved after 32 doubling passes (no correct run gets to either).
 * cx_grid_watershed3d_result: the pending labels: device pointer and shape; CX_ERR_STATE when nothing is pending.
 * There is no _bind: labels are not a grid to march.  A call leaves the bound grid, the current extraction, the selected level and the
 * Level-1 state as they are.  tests/watershed_ref.py restates all of it in numpy. */
#define CX_WATERSHED_RISING  0
#define CX_WATERSHED_FALLING 1
typedef struct cx_watershed_stats { int64_t n_labelled, n_unreached, n_ignored, n_markers, rounds, tile_visits, jump_rounds; } cx_watershed_stats;
int cx_grid_watershed3d(cx_ctx* ctx, const void* relief, int32_t dtype, int on_device, int64_t n0, int64_t n1, int64_t n2,
                        const int32_t* markers, const uint8_t* region, int32_t connectivity, int32_t direction,
                        void* out_device, void* out_host, cx_watershed_stats* stats);
int cx_grid_watershed3d_result(cx_ctx* ctx, void** out_device, int64_t out_shape[3]);

/* ---- regions: measures, cropped masks, contacts and relabelling of a labelled volume, on the device --------------------------------------
 * What follows a segmentation: per label its size, box, centroid and the extremes and sum of a second array (scipy.ndimage.find_objects,
 * sum, minimum_position, maximum_position), a mask of chosen labels cropped to a box that binds and marches (one surface per object at
 * the cost of its box, not of the volume), the pairs of labels that share a face, and a relabelling through a table
 * (skimage.segmentation.relabel_sequential, dropping, merging).  The reference has no call for it.
 *
 * Common to the four calls
 *   labels, on_device, n0 n1 n2: int32, aligned to 4, in device memory (on_device != 0) or host memory, every axis >= 1, at most 2^29
 *            samples (CX_ERR_INVALID otherwise, and for NULL).  Any label volume, whichever call made it: the pointers handed out by
 *            cx_grid_watershed3d_result and cx_grid_label3d_result are legal.  Device labels are read where they lie; host labels go
 *            up into a buffer of the state.  The context keeps no reference to the labels between calls.
 *   A label <= 0 is background; a negative label counts as 0 everywhere.
 *   Every count is an exact integer and every result a pure function of the inputs: two calls give the same bytes, with ONE stated
 *   exception, vsum of a float array (below).
 *
 * cx_grid_regions3d
 *   K = the largest label, found by a reduction; *k_max receives it, *n_negative the number of negative samples (either may be NULL).
 *   CX_ERR_UNSUPPORTED when K > CX_REGIONS_MAX_LABEL: the record table is K x 128 bytes on the device and on the host (2 GiB at the
 *   limit), and labels beyond it are no numbering of regions.  out_host NULL: K only.  Else CX_ERR_INVALID when capacity < K; K == 0 is
 *   served with any capacity.  Record c - 1 belongs to label c:
 *     shape    voxels, first, sum, lo, hi, rim as cx_grid_label3d_measures defines them
 *     n_nan    the samples of the label whose value is NaN
 *     min_at, max_at  the linear index of the smallest / largest value that is not NaN; among equal values the smallest index; -1: none
 *     vmin, vmax      those values, exactly (every sample type converts to double exactly); 0 when there is none
 *     isum     integer sample types: the exact sum of the values; float types: 0
 *     vsum     integer types: (double)isum; float types: the sum of the values that are not NaN, added up in double
 *   A label no sample carries has voxels 0, first -1, lo {0,0,0}, hi {-1,-1,-1}, min_at = max_at = -1 and everything else 0.
 *   values   NULL (the value fields are then those of a label without samples), or an array of the labels' shape of any CX_DTYPE_*
 *            values_dtype, in host or device memory (values_on_device) independently of the labels.
 *   Floats are ordered as cx_grid_rank3d orders them: -inf < ... < -0.0 < +0.0 < ... < +inf, NaN excluded and counted.  So vmin of
 *   {-0.0, +0.0} is -0.0.
 *   vsum of a float array is built with floating-point atomics, whose order differs from call to call: it is the ONLY field that may
 *   differ between two calls, and it satisfies |vsum - exact| <= (voxels - 1) * 2^-53 * sum |v|, the bound of a sum of doubles in any
 *   order (each sample converts to double exactly).
 * cx_grid_regions3d_select
 *   keep     n_keep host bytes indexed by label, keep[0] for the background; a label >= n_keep is not kept.
 *   box_lo, box_hi  an index box, both ends included; both NULL: the whole array.  pad: 0 .. 8.
 *   The result is the uint8 mask of the array extended by zeros, cropped to [box_lo - pad, box_hi + pad] and contiguous: shape
 *   box_hi - box_lo + 1 + 2 pad; inside the array keep[label] != 0, outside it 0.  out_shape, out_origin (= box_lo - pad, may be
 *   negative) and n_voxels (the exact count of ones) may be NULL.
 *   out_device  not NULL: the mask is written there (any alignment; CX_ERR_INVALID if it overlaps device labels), and the context keeps
 *            no result.  NULL: it goes into a buffer the context owns and stays pending until the next select or the bind, in an eighth
 *            slot of its own: the pending results of the seven other volume operations are not disturbed, and the pending pointer is a
 *            legal `samples` of them (CX_DTYPE_U8, on the device).  out_host not NULL: also receives a copy.
 *   CX_ERR_INVALID: a box that leaves the array, lo > hi, one end of the box without the other, a pad outside 0 .. 8.
 * cx_grid_regions3d_select_result: the pending mask: device pointer, shape, origin and count; CX_ERR_STATE when none is pending.
 * cx_grid_regions3d_bind: the pending mask becomes the bound grid (CX_DTYPE_U8, owned by the context) with every reset of an upload, as
 *   cx_grid_label3d_bind does it.  The origin is the caller's, as it is across uploads: passing the mask's origin to cx_set_origin,
 *   which takes negative origins, makes the march of the crop the march of the whole mask.  CX_ERR_INVALID, the mask left pending, for
 *   an axis shorter than 2; CX_ERR_STATE without a pending mask.
 * cx_grid_regions3d_map
 *   out[i] = map[label] for a label in [0, n_map), the negative ones counting as 0, and 0 for a label >= n_map.  map: n_map int32 on the
 *   host.  Relabelling, dropping small regions and merging regions are all this call.  out_device (aligned to 4) may BE the device
 *   labels (in place); any other overlap is CX_ERR_INVALID.  out_host also receives a copy; one of the two must be given.  Nothing stays
 *   pending.
 * cx_grid_regions3d_contacts
 *   One record per unordered pair a < b of distinct labels, 0 included as a partner, that are face neighbours somewhere; faces[x] = the
 *   number of sample pairs adjacent along axis x that carry {a, b}.  Neighbours never wrap across rows or planes.  Records are sorted by
 *   (a, b).  *n receives their number; out_host NULL: the number only; CX_ERR_INVALID when capacity < n.  Face contacts only.
 *   CX_ERR_UNSUPPORTED beyond 2^26 pairs.
 * A call without bind leaves the bound grid, the current extraction, the selected level, the Level-1 state and the seven other pending
 * results as they are.  tests/regions_ref.py restates all of it in numpy. */
#define CX_REGIONS_MAX_LABEL (1 << 24)
typedef struct cx_region {
    cx_label_component shape;
    int64_t n_nan;
    int64_t min_at, max_at;
    double  vmin, vmax;
    int64_t isum;
    double  vsum;
} cx_region;               /* 128 bytes */
typedef struct cx_region_contact { int32_t a, b; int64_t faces[3]; } cx_region_contact;      /* 32 bytes */
int cx_grid_regions3d(cx_ctx* ctx, const int32_t* labels, int on_device, int64_t n0, int64_t n1, int64_t n2,
                      const void* values, int32_t values_dtype, int values_on_device, cx_region* out_host, int64_t capacity,
                      int64_t* k_max, int64_t* n_negative);
int cx_grid_regions3d_select(cx_ctx* ctx, const int32_t* labels, int on_device, int64_t n0, int64_t n1, int64_t n2,
                             const uint8_t* keep, int64_t n_keep, const int64_t box_lo[3], const int64_t box_hi[3], int32_t pad,
                             uint8_t* out_device, uint8_t* out_host, int64_t out_shape[3], int64_t out_origin[3], int64_t* n_voxels);
int cx_grid_regions3d_select_result(cx_ctx* ctx, uint8_t** mask_device, int64_t shape[3], int64_t origin[3], int64_t* n_voxels);
int cx_grid_regions3d_bind(cx_ctx* ctx);
int cx_grid_regions3d_map(cx_ctx* ctx, const int32_t* labels, int on_device, int64_t n0, int64_t n1, int64_t n2,
                          const int32_t* map, int64_t n_map, int32_t* out_device, int32_t* out_host);
int cx_grid_regions3d_contacts(cx_ctx* ctx, const int32_t* labels, int on_device, int64_t n0, int64_t n1, int64_t n2,
                               cx_region_contact* out_host, int64_t capacity, int64_t* n);

/* ---- standalone SurfaceGeometry operator ---------------------------------------------------------
 * SurfaceGeometry(vertices, triangles).clean_triangles() / .orient_triangles()
 * (surface_geometry.py:6-12, 14-50, 52-140) on caller-supplied host arrays.
 * mode 0 = orient_triangles only, 1 = clean_triangles then orient_triangles, 2 = clean_triangles only.
 * Outputs are written in place: *nv / *nt are updated, points (nv*3 doubles) and tris (nt*3 int32)
 * are overwritten with the cleaned / oriented mesh (vertices compacted to those still in use). */
int cx_surface_geometry(cx_ctx* ctx, double* points_xyz, int64_t* nv, int32_t* tris, int64_t* nt,
                        int mode);

/* ---- 4-D: marching pentatopes ------------------------------------------------------------------------
 * Replaces, for a dense grid A[n0][n1][n2][n3] (last axis = t, fastest), GridContour4D's hyper-voxel
 * march: find_initial_voxels/expand_voxels/border_voxel with the 16-corner HYPERCUBE (pentatopes.py:94-95,
 * tetrahedral.py:383-469), enumerate_voxel_tetrahedra / enumerate_pentatope_tetrahedra
 * (pentatopes.py:216-291) and the edge interpolation (tetrahedral.py:471-512).
 * Result: vertex records float4 {x,y,z,t} in grid coordinates, edge ids
 * (linear index of the lower lattice point << 4) | direction (1..15 = 8di+4dj+2dk+dl), and
 * tetrahedra as 4 int32 vertex indices (cx_counts.n_triangles counts tetrahedra here).
 * CX_DIAG_CPYTHON310 reproduces the reference's 2-3 split (set order of 4-tuples, pentatopes.py:255-256).
 * cx_set_origin4d: lattice coordinates of sample [0,0,0,0] (>= -1024 per axis; they enter the set order only).  The kernels hash
 * lattice coordinates as 32-bit ints: with CX_DIAG_CPYTHON310 an origin that puts the array's last lattice point beyond 2^31 - 1
 * on some axis is refused by cx_extract4d (CX_ERR_UNSUPPORTED). */
int cx_grid4d_upload(cx_ctx* ctx, const float* host, int64_t n0, int64_t n1, int64_t n2, int64_t n3);
int cx_grid4d_adopt_device(cx_ctx* ctx, const void* device_ptr, int64_t n0, int64_t n1, int64_t n2, int64_t n3);
int cx_set_origin4d(cx_ctx* ctx, int64_t o0, int64_t o1, int64_t o2, int64_t o3);
int cx_extract4d(cx_ctx* ctx, double value, uint32_t flags, cx_counts* out);
/* The same march enqueued on the context's stream and not waited for (one volume after the other on two contexts, as
 * cx_extract3d_async / cx_counts_get for the 3-D path); cx_counts4d_get waits for it, validates the counters and, if a buffer was too
 * small, grows it and runs the march again synchronously.  CX_ERR_STATE without an extraction in flight. */
int cx_extract4d_async(cx_ctx* ctx, double value, uint32_t flags);
int cx_counts4d_get(cx_ctx* ctx, cx_counts* out);
/* Seeded selection in 4-D, the counterpart of cx_select_seeded3d: GridContour4D(corner, function, value, endpoints)
 * (pentatopes.py:92-100) grows from its end points with the methods it inherits (tetrahedral.py:396-463) over the 80
 * neighbours of pentatopes.py:32-39.  endpoints_ijkl: n x 8 int32 lattice points (i0,j0,k0,l0, i1,j1,k1,l1) whose
 * samples straddle the isovalue.  Call between cx_extract4d and cx_postprocess4d; restricts the post-pass (until the
 * next extraction) to the tetrahedra of the hyper-voxel groups reached.  out_counts (4 x int64): [0] seed voxels,
 * [1] groups kept (as defined at cx_select_seeded3d), [2] tetrahedra kept, [3] rejected pairs (CX_ERR_INVALID). */
int cx_select_seeded4d(cx_ctx* ctx, const int32_t* endpoints_ijkl, int64_t n, int64_t* out_counts);
/* The same with the reference's in_range box (tetrahedral.py:465-469) given explicitly: range_lo_hi = lo[4], hi[4] in array
 * coordinates, lo <= hyper-voxel < hi (NULL: the whole array).  For an array that carries a rim of samples around the reference's
 * grid (origin -1, cx_set_origin4d): the growth stays inside the grid, seed voxels in the rim are kept and grow one step into it
 * -- the reference does not range-check the voxels it starts from (tetrahedral.py:396-441, pentatopes.py:528-551).
 * flags: CX_SEED_ALL_IN_RANGE as for cx_select_seeded3d_ex (the exhaustive search on a surface that leaves the grid). */
int cx_select_seeded4d_ex(cx_ctx* ctx, const int32_t* endpoints_ijkl, int64_t n, const int32_t* range_lo_hi, uint32_t flags, int64_t* out_counts);
/* the selection as a mask over the Level-0 tetrahedra (n_tetrahedra bytes, 1 = kept) */
int cx_seeded4d_mask_download(cx_ctx* ctx, uint8_t* tet_keep);
int cx_level0_4d_download(cx_ctx* ctx, float* verts_xyzt, uint32_t* edge_ids, int32_t* tets);
/* GridContour4D.find_tetrahedra's post-steps on the device: bin_times(nbins) (pentatopes.py:162-169),
 * drop_instant_tetrahedra(1e-7) (:171-189), remove_tiny_simplices(1e-3) (tetrahedral.py:353-375).
 * out_counts (8 x int64): [0] vertices (unchanged numbering), [1] surviving tetrahedra,
 * [2] after drop_instant, [3] after the tiny collapse.  Download: points = nv*4 doubles, tets = nt*4 int32. */
int cx_postprocess4d(cx_ctx* ctx, int32_t nbins, int64_t* out_counts);
/* the same on points handed over by the caller: n_vertices * 4 doubles in the order of cx_level0_4d_download, in the reference's
 * lattice -- linear_interpolate=False re-evaluates the caller's function between the lattice points (tetrahedral.py:488-505),
 * which is Python; NULL = cx_postprocess4d */
int cx_postprocess4d_points(cx_ctx* ctx, int32_t nbins, const double* points_xyzt, int64_t* out_counts);
int cx_level1_4d_download(cx_ctx* ctx, double* points_xyzt, int32_t* tets);
/* GridContour4D.collect_morph_triangles (pentatopes.py:314-368) + MorphTriangles.orient_triangles
 * (morph_geometry.py:49-89) on the tetrahedra left by cx_postprocess4d: every tetrahedron is sliced at the
 * midpoints between its distinct vertex times into 1-2 triangles whose corners are SEGMENTS (pairs of 4-D
 * points, stored low t -> high t); triangles are oriented per connected component, propagating only between
 * triangles whose time ranges overlap.  out_counts (8 x int64): [0] points, [1] segments, [2] triangles,
 * [4] components.  Download: points nv*4 doubles, segments ns*2 int32 (point indices), triangles nt*3 int32
 * (segment indices). */
int cx_morph_triangles(cx_ctx* ctx, int64_t* out_counts);
int cx_morph_download(cx_ctx* ctx, double* points_xyzt, int32_t* segments, int32_t* triangles);
/* The surface at time t from the morph triangles of the last cx_morph_triangles: the consumer-side evaluation of
 * misc/morph_triangles.js:26-140 (a triangle is visible while t is inside the intervals of all three of its
 * segments; corners = points of the segments at t).  out_counts (2 x int64): [0] points, [1] triangles.
 * Download: points np*3 doubles, triangles nt*3 int32 (indices into those points, original triangle order). */
int cx_morph_eval(cx_ctx* ctx, double t, int64_t* out_counts);
int cx_morph_eval_download(cx_ctx* ctx, double* points_xyz, int32_t* triangles);
/* The same for n_times times in ONE set of launches -- the per-t isosurface stream the viewer plays frame by frame
 * (misc/morph_triangles.js:117-204 once per frame; here: all frames of a stream at once).  times: any order, repeats allowed.
 * out_counts (n_times x 2 x int64): per time [0] points, [1] triangles.  Surface i is exactly what cx_morph_eval(times[i]) returns
 * (same points, same index triples, same order); the surfaces lie one behind the other in device memory.
 * _download: surface i of the last call (points np*3 doubles, triangles nt*3 int32, indices local to the surface);
 * _device_ptrs: where surface i lies on the device (NULL for an empty one) -- valid until the next evaluation on this context.
 * cx_morph_triangles leaves segments and triangles sorted by their start time, so that the triangles (and segments) that exist at one
 * time are a window of ids: a call costs what its windows hold, not what the whole morph holds. */
int cx_morph_eval_many(cx_ctx* ctx, const double* times, int32_t n_times, int64_t* out_counts);
int cx_morph_eval_many_download(cx_ctx* ctx, int32_t i, double* points_xyz, int32_t* triangles);
int cx_morph_eval_many_device_ptrs(cx_ctx* ctx, int32_t i, void** points_xyz, void** triangles);
/* every surface of the last call in ONE transfer: the points of surface 0, 1, ... one behind the other (sum of the point counts x 3
 * doubles), the triangles likewise (indices local to their surface) */
int cx_morph_eval_many_download_all(cx_ctx* ctx, double* points_xyz, int32_t* triangles);

/* ---- 4-D volumes of more than 2^28 samples: marched slab by slab along axis 0, assembled on the device ----------------------------
 * One extraction addresses 2^28 samples (32-bit edge ids).  A larger volume is marched in slabs of whole planes, each with the next
 * plane as a halo (all but the last), and assembled into ONE mesh on the device:
 *     cx_slab4d_begin(ctx, whole_shape)                              whole_shape = {n0, n1, n2, n3} of the whole volume
 *     per slab, in axis-0 order:  bind planes i0 .. i1 (+ halo plane i1 unless last) with cx_grid4d_upload / _adopt_device,
 *                                 cx_set_origin4d(ctx, i0, 0, 0, 0), cx_extract4d, cx_slab4d_append(ctx, i0, i1 - i0, counts)
 *     cx_slab4d_finish(ctx, nbins, counts)                           the post-steps of cx_postprocess4d on the assembly
 * The append keeps the slab's OWNED vertices (lower lattice point below its halo plane) in ascending edge id, so the assembly is in
 * ascending GLOBAL edge id ((linear index in the whole volume << 4) | direction; cx_slab4d_download_keys) and a vertex's index is its
 * priority; points are float64 in the whole volume's lattice, bit for bit those of a single extraction.  Tetrahedra get assembly
 * indices; a reference to a halo-plane vertex is resolved by the next slab's append.  The march's table emits every tetrahedron
 * oriented, so the assembly is oriented as a single extraction is.  append out_counts (8 x int64): [0] assembled vertices, [1] assembled
 * tetrahedra, [2] this slab's new vertices, [3] its tetrahedra, [4] halo vertices pending, [5] slabs.  finish out_counts as
 * cx_postprocess4d's; afterwards cx_level1_4d_download, cx_morph_triangles (which then skips any data-driven orientation and does not
 * read the grid, only the last slab's by then), cx_morph_eval* work as after cx_postprocess4d.
 * CX_ERR_STATE: a slab out of order, cx_postprocess4d between begin and finish, finish with planes missing or references unresolved.
 * A later cx_extract4d, cx_postprocess4d or cx_slab4d_begin invalidates an assembled result, as a new post-pass does a single one. */
int cx_slab4d_begin(cx_ctx* ctx, const int64_t* whole_shape);
int cx_slab4d_append(cx_ctx* ctx, int64_t i0, int64_t owned_planes, int64_t* out_counts);
int cx_slab4d_finish(cx_ctx* ctx, int32_t nbins, int64_t* out_counts);
/* the global edge id of every assembled vertex (n_vertices int64, the order of the points) */
int cx_slab4d_download_keys(cx_ctx* ctx, int64_t* keys);

/* ---- 2-D contour lines at several isovalues ------------------------------------------------------
 * Replaces triangulated.Grid2DContour (search_grid :198-212, find_initial_contour_pairs :299-320,
 * expand_contour_pairs :322-331, get_contour_sequences :226-297; triangulated.py) for one sample array and ALL
 * isovalues of multiple_2d_contour.Multiple2DContourGrid.get_contours_dictionary (multiple_2d_contour.py:17-30,
 * level lookup by bisection as in classify_endpoint_values :48-59) in one pass over the samples.
 * samples: fp32 A[n][m] (host pointer, or device pointer when on_device != 0; array axes (0,1) are the reference's
 * (x,y)); values: ascending, distinct.  A sample equal to an isovalue counts as high.
 * seeds: nseeds x (i, j, role, level index) int32 -- the polylines grown from the pairs around lattice point (i,j)
 * as their low (role 0) or high (role 1) end are kept, exactly the reference's seeded growth; nseeds == 0: the seeds
 * of the reference's own grid search (every crossing axis edge that starts at i < n-1, j < m-1).
 * Limits: n*m <= 2^30 samples, at most 65535 values, fewer than 2^29 crossings (all levels together) per call
 * (CX_ERR_UNSUPPORTED otherwise: contour fewer levels per call).
 * mins_delta: {min_x, min_y, delta_x, delta_y} for FunctionGrid.from_grid_coordinates (grid_field.py:89-93), or NULL
 * for grid coordinates.
 * Output (cx_contour2d_download): points n_points x 2 float64, polyline by polyline; keys n_points int64 =
 * ((3*(i*m+j) + d) << 16) | level index for the crossing of the lattice edge from (i,j) in direction d (0: (1,0),
 * 1: (0,1), 2: (1,1)); chains: one cx_chain2d per polyline, ordered by their first crossing's id. */
#define CX2_ALL_CHAINS 1u   /* keep every polyline (no seeded growth) */
#define CX2_NO_DEDUPE 2u    /* keep points that are np.allclose to their predecessor (triangulated.py:268) */
#define CX2_SEARCH_SEEDS 4u /* with explicit seeds: add the seeds of the grid search too (multiple_2d_contour.py:39-41) */
typedef struct {
    uint32_t n_points;   /* points in the polylines returned */
    uint32_t n_chains;   /* polylines returned */
    uint32_t n_pairs;    /* crossings found on the whole lattice, all levels */
    uint32_t n_levels;
} cx_counts2d;
typedef struct {
    int32_t level;       /* index into values */
    int32_t closed;      /* the `closed` flag of get_contour_sequences */
    uint32_t first;      /* first point */
    uint32_t count;      /* number of points */
} cx_chain2d;
int cx_contour2d_extract(cx_ctx* ctx, const float* samples, int on_device, int64_t n, int64_t m, const double* values, int32_t nvalues,
                         const int32_t* seeds, int64_t nseeds, uint32_t flags, const double* mins_delta, cx_counts2d* out);
int cx_contour2d_download(cx_ctx* ctx, double* points_xy, int64_t* keys, cx_chain2d* chains);

/* ---- measurement ----------------------------------------------------------------------------------
 * When enabled, every extract records HIP events around its kernels on the context's stream (cx_timing_enable(ctx, 1)
 * creates the events of the next 256 extracts once per context; extracts beyond that go untimed until the next read).
 * cx_timing_read synchronises and returns the summed milliseconds since the last reset:
 * ms[0] classify + vertex stage (all of its kernels), ms[1] triangle emit kernel, ms[2] whole extract,
 * ms[3] stream kernel, ms[4] scan kernel, ms[5] cell / vertex emit kernel (staged pipeline; the generic
 * classify kernel is reported in ms[3]), ms[6..7] reserved.  *n = number of extracts accumulated. */
int cx_timing_enable(cx_ctx* ctx, int on);
int cx_timing_read(cx_ctx* ctx, double ms[8], int* n);
/* what a plain streaming READ of `bytes` bytes at device_ptr reaches on this device (16-byte loads, grid-stride; best of `reps`
 * launches on the context's stream, HIP events): the measured ceiling beside the 8 TB/s data-sheet figure that bench.py quotes
 * the stream kernel against ("also report measured stream-read BW on the box").  No counterpart in the reference. */
int cx_measure_read_bandwidth(cx_ctx* ctx, const void* device_ptr, int64_t bytes, int reps, double* out_GBps);

/* Device memory held in the library's growable buffers: bytes live now and hipMalloc calls made so far, of this context or -- with
 * ctx == NULL -- of the whole process (what is left after cx_ctx_destroy).  Either output may be NULL.  Buffers only ever grow, so
 * `allocations` standing still across a call says that the call allocated nothing.  No counterpart in the reference. */
int cx_device_bytes(cx_ctx* ctx, int64_t* live_bytes, int64_t* allocations);

/* diagnostics: per-wave s_memtime stamps of the stream kernel (4 words per wave: [0] start, [1] end; [2..3]
 * unused).  words > 0 allocates, host != NULL copies out, 0/NULL frees. */
int cx_debug_stamps(cx_ctx* ctx, int64_t words, unsigned long long* host);

/* library build info: "gfx950;<git describe or date>" */
const char* cx_version(void);

#ifdef __cplusplus
}
#endif
#endif
