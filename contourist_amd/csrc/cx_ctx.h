// cx_ctx.h -- the context object behind the C ABI (host side only).
#pragma once
#include <string>

#include "cx_common.h"

struct cx_post_state;  // Level-1 buffers (cx_post.hip)
struct cx_state4;       // 4-D march state (cx_api4d.hip)
struct cx_state2;       // 2-D contour lines (cx_contour2d.hip)
struct cx_levels_state; // several isovalues of one grid (cx_levels.hip)

struct cx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;      // stream in use
    hipStream_t own_stream = nullptr;  // stream created by the context
    std::string err;
    // sampled field
    cx_grid_ref grid = {nullptr, CX_DTYPE_F32};
    uint8_t* grid_owned = nullptr;     // the uploaded samples, any type (bytes)
    size_t grid_owned_bytes = 0;
    int64_t n0 = 0, n1 = 0, n2 = 0;
    double* grid64 = nullptr;          // float64 originals of the samples (cx_grid_shadow_f64): Level 1 interpolates on these
    size_t grid64_cap = 0;
    bool grid64_valid = false;
    // side tables of the march
    uint64_t* celltab = nullptr;
    size_t tables_for = 0;
    uint32_t* queue = nullptr;         // staged pipeline: per-wave queues, totals and offsets
    size_t queue_cap = 0;
    cx_wsum* wsum = nullptr;
    size_t wsum_cap = 0;
    cx_wbase* wbase = nullptr;
    size_t wbase_cap = 0;
    cx_brec* brec = nullptr;
    size_t brec_cap = 0;
    cx_bdesc* flat = nullptr;
    size_t flat_cap = 0;
    uint32_t* qa = nullptr;            // fused emit: queue positions / active cells per plane step and lane of the streaming waves
    size_t qa_cap = 0;
    uint32_t* info = nullptr;          // fused emit: per queue entry, first vertex of the cell in its wave | crossing mask
    size_t info_cap = 0;
    float* tq = nullptr;               // staged kernels: the stream kernel's interpolation fractions, one region per streaming wave (cx_params::tq)
    size_t tq_cap = 0;
    uint64_t* info64 = nullptr;        // staged kernels: per queue entry, (crossing mask << 32) | first vertex
    size_t info64_cap = 0;
    uint32_t* chunksum = nullptr;      // totals of every 256 streaming waves (cx_params::chunksum)
    size_t chunksum_cap = 0;
    uint32_t* rstart = nullptr;        // vertex stage: first batch of every wave's share of the rounds (cx_params::rstart)
    size_t rstart_cap = 0;
    uint32_t* kstart = nullptr;        // the same for the triangle stage (cx_params::kstart)
    size_t kstart_cap = 0;
    uint64_t* fj = nullptr;            // tile emit path: face words (cx_params::fj, fk), boundary records and their counts per tile
    size_t fj_cap = 0;
    uint64_t* fk = nullptr;
    size_t fk_cap = 0;
    uint4* bnd = nullptr;
    size_t bnd_cap = 0;
    uint32_t* bndn = nullptr;
    size_t bndn_cap = 0;
    uint32_t* torder = nullptr;
    size_t torder_cap = 0;
    uint8_t* hbytes = nullptr;         // fused emit: CPython set-order code per lattice point (valid for hash_xy's shape and origin)
    size_t hbytes_cap = 0;
    bool hbytes_valid = false;
    int64_t hbytes_n2 = 0, hbytes_o2 = 0;
    cx_task last_task = {};
    uint32_t last_flags = 0;
    int path = 0;                      // kernels of the last extraction: 0 generic, 1 staged, 2 fused, 3 tile emit
    bool records_valid = false;        // ctx->cells holds the cell records of the last extraction
    uint64_t* hash_xy = nullptr;       // CPython tuple-hash prefix per (i,j), for CX_DIAG_CPYTHON310
    size_t hash_xy_cap = 0;
    int64_t hash_xy_n0 = 0, hash_xy_n1 = 0, hash_xy_o0 = -1, hash_xy_o1 = -1;
    int64_t origin[3] = {0, 0, 0};
    int64_t corner_ref[3] = {0, 0, 0};   // > 0: the reference's corner for the Level-1 scales (cx_set_reference_corner)
    int64_t origin4[4] = {0, 0, 0, 0};
    cx_state4* s4 = nullptr;
    cx_state2* s2 = nullptr;
    cx_levels_state* lv = nullptr;
    int lv_current = -1;               // level of cx_extract3d_levels whose mesh the context's output buffers hold (-1: none)
    // Level-0 outputs
    cx_vrec* verts = nullptr;          // 8-byte vertex records {edge id, fp32 fraction}
    float4* verts_xyz = nullptr;       // {x, y, z, bits(edge id)} expanded from the records on request (cx_level0_expanded)
    size_t verts_xyz_cap = 0;
    uint4* cells = nullptr;
    int32_t* tris = nullptr;
    uint32_t vcap = 0, ccap = 0, tcap = 0;
    uint32_t* counters = nullptr;
    uint32_t* counters_host = nullptr;
    bool extracted = false;
    bool counts_fetched = false;       // ctx->counts holds the counters of the last 3-D extraction (cx_counts_get)
    cx_counts counts = {0, 0, 0, 0};
    cx_params last;
    // seeded selection (cx_select_seeded3d): triangle mask followed by vertex mask, valid until the next extraction
    uint8_t* tri_keep = nullptr;
    size_t keep_cap = 0;
    // scratch of cx_select_seeded3d_ex (bytes), kept between calls: map per sample, union-find, bitmap, flags, seeds, counters, end
    // points, visited set -- a selection allocated and freed them every time (0.8 of 2.9 ms on the 512^3 bench field)
    uint8_t* seed_buf[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t seed_cap[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int seed_mode = 0;      // how the last seeded selection (3-D or 4-D) ran its end points: 0 sequential (the reference's shared visited set), 1 one thread per pair
    bool keep_valid = false;
    // vertex attributes (cx_attr.hip), kept between calls: Level-0 normals float4 {nx, ny, nz, |g|}, Level-1 normals double[3], sampled
    // values (fp32 at Level 0, float64 at Level 1) and the device copy of a second grid handed over from the host
    float4* attr_n0 = nullptr;
    size_t attr_n0_cap = 0;
    double* attr_n1 = nullptr;
    size_t attr_n1_cap = 0;
    float* attr_v0 = nullptr;
    size_t attr_v0_cap = 0;
    double* attr_v1 = nullptr;
    size_t attr_v1_cap = 0;
    uint8_t* attr_e1 = nullptr;        // Level 1: per output vertex {sample index of the low point, of the high point, ratio} (16 bytes)
    size_t attr_e1_cap = 0;
    uint8_t* attr_grid = nullptr;
    size_t attr_grid_cap = 0;
    // components of the Level-1 mesh (cx_comp.hip): labels, accumulators and the table, kept between calls
    struct cx_comp_state* comp = nullptr;
    // vertex clustering of the Level-1 mesh (cx_simplify.hip): cluster table, accumulators, scans, kept between calls
    struct cx_simplify_state* simp = nullptr;
    // Level-1
    cx_post_state* post = nullptr;
    bool post_valid = false;
    unsigned long long* stamps = nullptr;   // diagnostic stamps (cx_debug_stamps)
    size_t stamps_words = 0;
    // the context's own RCCL communicator (cx_rccl_comm_init, cx_halo.hip), or null
    void* rccl_comm = nullptr;
    bool rccl_owned = true;              // false: the communicator belongs to another context of this rank (cx_rccl_comm_share)
    int rccl_rank = 0, rccl_world = 1;
    // device -> host copies of mesh-sized buffers (cx_xfer.hip): two pinned staging buffers and their events
    void* xfer_stage[2] = {nullptr, nullptr};
    hipEvent_t xfer_ev[2] = {nullptr, nullptr};
    // timing
    struct evset { hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}; };
    bool timing = false;
    int nevents = 0;
    evset events[256];
};

// THE place where a device buffer of a context is freed and allocated again.  A buffer is a (pointer, capacity) pair that always
// travels together through this function: a regrow branch cannot free a neighbour's pointer or leave a capacity describing a
// buffer that is gone (rounds 1 and 2 each had a stray hipFree in a hand-written regrow block).  Waits for the context's stream
// first (kernels enqueued on it may still use the old buffer).  `need` in elements; grows to exactly `need`.
template <typename T, typename C>
int cx_grow(cx_ctx* ctx, T*& ptr, C& cap, size_t need) {
    if ((size_t)cap >= need && ptr) return CX_OK;
    if (need == 0) return CX_OK;
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess && ptr) e = hipFree(ptr);
    ptr = nullptr; cap = 0;
    void* fresh = nullptr;
    if (e == hipSuccess) e = hipMalloc(&fresh, need * sizeof(T));
    if (e != hipSuccess) {
        ctx->err = std::string("device buffer (") + std::to_string(need * sizeof(T)) + " bytes): " + hipGetErrorString(e);
        return (e == hipErrorOutOfMemory) ? CX_ERR_NOMEM : CX_ERR_HIP;
    }
    ptr = static_cast<T*>(fresh);
    cap = (C)need;
    return CX_OK;
}
// The same for a buffer that is appended to (the slab assembly of cx_slab4d.hip): the first `used` elements move into the new buffer,
// which gets room for half as many again as before when that is more than `need` (a volume of many slabs grows it a few times, not
// once per slab).  Pointers into the old buffer are dead after the call: kernels get pointers taken after the last grow.
template <typename T>
int cx_grow_keep(cx_ctx* ctx, T*& ptr, size_t& cap, size_t used, size_t need) {
    if (cap >= need && ptr) return CX_OK;
    if (need == 0) return CX_OK;
    const size_t want = need > cap + cap / 2 ? need : cap + cap / 2;
    void* fresh = nullptr;
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = hipMalloc(&fresh, want * sizeof(T));
    if (e == hipSuccess && ptr && used) e = hipMemcpyAsync(fresh, ptr, used * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        if (fresh) (void)hipFree(fresh);
        ctx->err = std::string("device buffer (") + std::to_string(want * sizeof(T)) + " bytes): " + hipGetErrorString(e);
        return (e == hipErrorOutOfMemory) ? CX_ERR_NOMEM : CX_ERR_HIP;
    }
    if (ptr) (void)hipFree(ptr);
    ptr = static_cast<T*>(fresh);
    cap = want;
    return CX_OK;
}
template <typename T, typename C>
void cx_release(T*& ptr, C& cap) {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr; cap = 0;
}

// cx_api.hip
int cx_ensure_cell_records(cx_ctx* ctx);
int cx_ensure_hash_xy(cx_ctx* ctx, uint32_t flags);
int cx_level0_expanded(cx_ctx* ctx, float4** out);   // the records of the current extraction as float4 {x,y,z,id} (device, enqueued on the stream)
void cx_fill_value_params(cx_params& P, double value);
// cx_halo.hip
void cx_rccl_comm_free(cx_ctx* ctx);
// cx_xfer.hip
int cx_copy_to_host(cx_ctx* ctx, int nparts, void* const* dst, const void* const* src, const size_t* bytes);
int cx_copy_to_host1(cx_ctx* ctx, void* dst, const void* src, size_t bytes);
void cx_xfer_free(cx_ctx* ctx);
// cx_levels.hip
void cx_levels_free(cx_ctx* ctx);
void cx_levels_invalidate(cx_ctx* ctx);
// cx_post.hip
void cx_post_free(cx_ctx* ctx);
int cx_scan_u32(cx_ctx* ctx, const uint32_t* in, uint32_t* out, uint32_t n, uint32_t* sums_tmp, uint32_t* total_dev,
                unsigned long long* total64_dev = nullptr);   // total64: the total without the wrap at 2^32
// what cx_attr.hip reads of the Level-1 state: the edge id of every output vertex and one byte per vertex, 1 = the orientation step
// reversed the triangles of its component.  CX_ERR_INVALID without a post-pass, CX_ERR_UNSUPPORTED when the keys are not edge ids
// of the resident array (cx_postprocess3d_mesh, cx_postprocess3d_shard_*).  `who` names the caller in the error text.
struct cx_level1_view {
    const uint32_t* keys;
    const uint8_t* vflip;
    uint32_t nv;
};
int cx_level1_attr_view(cx_ctx* ctx, const char* who, cx_level1_view* out);
// what cx_comp.hip reads of the Level-1 state: the tables of the orientation step (parent word = (parity << 32) | root triangle, the
// root's flip in cflip[root]), the output mesh, the grid box of the post-pass and the generation of the mesh.  CX_ERR_INVALID without a
// post-pass, CX_ERR_UNSUPPORTED for a shard, CX_ERR_STATE when the tables are gone.  The scratch buffers take a filtered copy of the
// mesh (room for the whole of it); cx_level1_comp_commit makes that copy the Level-1 mesh.
struct cx_level1_comp_view {
    const unsigned long long* parent;
    const unsigned long long* cflip;
    const int32_t* tri;
    const double* pts;
    const uint32_t* keys;
    uint32_t nv, nt;
    double corner[3];
    uint64_t gen;
};
struct cx_level1_comp_scratch {
    double* pts;
    int32_t* tri;
    uint32_t* keys;
    unsigned long long* parent;
    unsigned long long* cflip;
};
int cx_level1_comp_view_get(cx_ctx* ctx, const char* who, cx_level1_comp_view* out);
int cx_level1_comp_scratch_get(cx_ctx* ctx, cx_level1_comp_scratch* out);
// (vuse / vnew: which vertices stay and their new indices, for what travels with the vertices -- the carried normals of a simplified mesh)
int cx_level1_comp_commit(cx_ctx* ctx, uint32_t nv_new, uint32_t nt_new, const uint32_t* vuse, const uint32_t* vnew);
// what cx_simplify.hip writes for the shared tail of the post-pass (clean, compaction, orientation), in buffers the post-pass starts
// from: the clusters' points, prio = first member, the remapped triangles, tprio3 = {old triangle index} x 3, alive bytes; map: one
// int32 per vertex of the mesh before (the cluster id; the tail turns it into the new vertex index); nrm_new: the clusters' normals;
// nrm_src: the carried normals of the mesh before when it is a simplified one itself
struct cx_level1_simplify_io {
    double* pts;
    uint32_t* prio;
    int32_t* tri;
    uint32_t* tprio3;
    uint8_t* alive;
    int32_t* map;
    double* nrm_new;
    const double* nrm_src;
    bool simplified;
};
int cx_level1_simplify_bufs(cx_ctx* ctx, bool normals, bool dry_run, cx_level1_simplify_io* out);   // dry_run: map is scratch, the last map stays
int cx_level1_simplify_tail(cx_ctx* ctx, uint32_t nv_old, uint32_t ncl, uint32_t nt, bool do_clean, bool normals, int64_t* counts);
int cx_level1_carried_normals(cx_ctx* ctx, const double** nrm, uint32_t* nv);
int cx_level1_simplify_map_get(cx_ctx* ctx, const int32_t** map, uint32_t* n);
// cx_attr.hip
void cx_attr_free(cx_ctx* ctx);
// cx_comp.hip
void cx_comp_free(cx_ctx* ctx);
// cx_simplify.hip
void cx_simplify_free(cx_ctx* ctx);
// cx_api4d.hip
void cx_state4_free(cx_ctx* ctx);
// cx_contour2d.hip
void cx_state2_free(cx_ctx* ctx);
