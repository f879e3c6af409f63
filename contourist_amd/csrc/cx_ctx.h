// cx_ctx.h -- the context object behind the C ABI (host side only).
#pragma once
#include <atomic>
#include <string>
#include <type_traits>
#include <utility>

#include "cx_common.h"

// A HIP call inside a function that returns a CX_* code: on failure the context keeps the call and the runtime's text, and the
// function returns CX_ERR_NOMEM or CX_ERR_HIP.
#define CX_HIP(ctx, call)                                                                        \
    do {                                                                                         \
        hipError_t e__ = (call);                                                                 \
        if (e__ != hipSuccess) {                                                                 \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e__);                     \
            return (e__ == hipErrorOutOfMemory) ? CX_ERR_NOMEM : CX_ERR_HIP;                      \
        }                                                                                        \
    } while (0)

// launch geometry: blocks of b threads for n items (none for n = 0); cx_grid1: at 256 threads, and one block where that is none
// (the kernel's own bound check idles it; a launch of zero blocks is an error)
static inline uint32_t cx_blocks(size_t n, uint32_t b = 256) { return (uint32_t)((n + b - 1) / b); }
static inline dim3 cx_grid1(size_t n) { return dim3(n ? cx_blocks(n) : 1u); }
// slots of an open-addressing table for n keys: a power of two, at most half full
static inline unsigned long long cx_table_size(size_t n) {
    unsigned long long s = 1024;
    while (s < 2 * (unsigned long long)n + 16) s <<= 1;
    return s;
}

// cval in the sample type, if it is a value of that type (cx_grid_resample3d at order 0, cx_grid_rank3d): its bits, zero-extended
static inline bool cx_dtype_value_bits(int32_t dtype, double cval, uint32_t& bits) {
    const float f = (float)cval;
    uint32_t fb;
    memcpy(&fb, &f, 4);
    switch (dtype) {
        case CX_DTYPE_U8: bits = (uint32_t)(uint8_t)cval; return cval >= 0.0 && cval <= 255.0 && (double)(uint8_t)cval == cval;
        case CX_DTYPE_I8: bits = (uint32_t)(uint8_t)(int8_t)cval; return cval >= -128.0 && cval <= 127.0 && (double)(int8_t)cval == cval;
        case CX_DTYPE_U16: bits = (uint32_t)(uint16_t)cval; return cval >= 0.0 && cval <= 65535.0 && (double)(uint16_t)cval == cval;
        case CX_DTYPE_I16: bits = (uint32_t)(uint16_t)(int16_t)cval; return cval >= -32768.0 && cval <= 32767.0 && (double)(int16_t)cval == cval;
        case CX_DTYPE_F16: {
            if (!(cval >= -65504.0 && cval <= 65504.0)) return false;
            const _Float16 h = (_Float16)cval;
            uint16_t hb;
            memcpy(&hb, &h, 2);
            bits = hb;
            return (double)h == cval;
        }
        case CX_DTYPE_BF16: bits = fb >> 16; return (double)f == cval && (fb & 0xFFFFu) == 0u;
        default: bits = fb; return (double)f == cval;
    }
}

struct cx_post_state;  // Level-1 buffers (cx_post.h)
struct cx_state4;       // 4-D march state (cx_api4d.hip)
struct cx_state2;       // 2-D contour lines (cx_contour2d.hip)
struct cx_levels_state; // several isovalues of one grid (cx_levels.hip)
struct cx_ctx;

// Device memory in use by one context (cx_ctx::tally) and by the whole process (cx_process_tally): bytes held by cx_bufs now and
// hipMalloc calls made so far.  Read through cx_device_bytes.
struct cx_tally { int64_t live_bytes = 0, allocations = 0; };
struct cx_process_tally_t { std::atomic<int64_t> live_bytes{0}, allocations{0}; };
inline cx_process_tally_t cx_process_tally;

// The one owner of growable device memory.  Capacity in elements of T.  Reads as a T* wherever a
// pointer is handed on; pointers taken from it are dead after the next grow.  Never give one static storage duration: its hipFree
// would run after the runtime has gone.
template <typename T>
class cx_buf {
public:
    cx_buf() = default;
    cx_buf(const cx_buf&) = delete;
    cx_buf& operator=(const cx_buf&) = delete;
    cx_buf(cx_buf&& o) noexcept : p_(o.p_), cap_(o.cap_), tally_(o.tally_) { o.p_ = nullptr; o.cap_ = 0; }
    cx_buf& operator=(cx_buf&& o) noexcept {
        if (this != &o) { release(); p_ = o.p_; cap_ = o.cap_; tally_ = o.tally_; o.p_ = nullptr; o.cap_ = 0; }
        return *this;
    }
    ~cx_buf() { release(); }

    operator T*() const { return p_; }
    T* get() const { return p_; }
    size_t cap() const { return cap_; }
    size_t bytes() const { return cap_ * sizeof(T); }
    template <typename U> U* as() const { return reinterpret_cast<U*>(p_); }   // a byte buffer read as another type

    int grow(cx_ctx* ctx, size_t need);
    int grow_keep(cx_ctx* ctx, size_t used, size_t need);
    void release() {
        if (p_) (void)hipFree(p_);
        forget();
    }

private:
    hipError_t alloc(cx_ctx* ctx, size_t n);
    static int fail(cx_ctx* ctx, size_t bytes, hipError_t e);
    void forget() {
        if (p_) { tally_->live_bytes -= (int64_t)bytes(); cx_process_tally.live_bytes -= (int64_t)bytes(); }
        p_ = nullptr; cap_ = 0;
    }
    T* p_ = nullptr;
    size_t cap_ = 0;
    cx_tally* tally_ = nullptr;   // of the context that allocated p_ (outlives its buffers)
};
static_assert(!std::is_copy_constructible<cx_buf<uint8_t>>::value && !std::is_copy_assignable<cx_buf<uint8_t>>::value, "cx_buf owns its memory");
static_assert(std::is_nothrow_move_constructible<cx_buf<uint8_t>>::value && std::is_nothrow_move_assignable<cx_buf<uint8_t>>::value, "cx_buf moves");

struct cx_ctx {
    cx_tally tally;                 // first: the buffers below count themselves out of it when the context goes
    int device = 0;
    hipStream_t stream = nullptr;      // stream in use
    hipStream_t own_stream = nullptr;  // stream created by the context
    std::string err;
    // sampled field
    cx_grid_ref grid = {nullptr, CX_DTYPE_F32};
    cx_buf<uint8_t> grid_owned;     // the uploaded samples, any type (bytes)
    int64_t n0 = 0, n1 = 0, n2 = 0;
    cx_buf<double> grid64;          // float64 originals of the samples (cx_grid_shadow_f64): Level 1 interpolates on these
    bool grid64_valid = false;
    // side tables of the march
    cx_buf<uint64_t> celltab;
    cx_buf<uint32_t> queue;         // staged pipeline: per-wave queues, totals and offsets
    cx_buf<cx_wsum> wsum;
    cx_buf<cx_wbase> wbase;
    cx_buf<cx_brec> brec;
    cx_buf<cx_bdesc> flat;
    cx_buf<uint32_t> qa;            // fused emit: queue positions / active cells per plane step and lane of the streaming waves
    cx_buf<uint32_t> info;          // fused emit: per queue entry, first vertex of the cell in its wave | crossing mask
    cx_buf<float> tq;               // staged kernels: the stream kernel's interpolation fractions, one region per streaming wave (cx_params::tq)
    cx_buf<uint64_t> info64;        // staged kernels: per queue entry, (crossing mask << 32) | first vertex
    cx_buf<uint32_t> chunksum;      // totals of every 256 streaming waves (cx_params::chunksum)
    cx_buf<uint2> cbase;           // slim cell records: {first triangle, first vertex} of every 64th record (cx_params::cbase)
    cx_buf<uint32_t> rstart;        // vertex stage: first batch of every wave's share of the rounds (cx_params::rstart)
    cx_buf<uint32_t> kstart;        // the same for the triangle stage (cx_params::kstart)
    cx_buf<uint64_t> fj;            // tile emit path: face words (cx_params::fj, fk), boundary records and their counts per tile
    cx_buf<uint64_t> fk;
    cx_buf<uint4> bnd;
    cx_buf<uint32_t> bndn;
    cx_buf<uint32_t> torder;
    cx_buf<uint8_t> hbytes;         // fused emit: CPython set-order code per lattice point (valid for hash_xy's shape and origin)
    bool hbytes_valid = false;
    int64_t hbytes_n2 = 0, hbytes_o2 = 0;
    cx_task last_task = {};
    uint32_t last_flags = 0;
    int path = 0;                      // kernels of the last extraction: 0 generic, 1 staged, 2 fused, 3 tile emit
    bool records_valid = false;        // ctx->cells holds the cell records of the last extraction
    cx_buf<uint64_t> hash_xy;       // CPython tuple-hash prefix per (i,j), for CX_DIAG_CPYTHON310
    int64_t hash_xy_n0 = 0, hash_xy_n1 = 0, hash_xy_o0 = -1, hash_xy_o1 = -1;
    int64_t origin[3] = {0, 0, 0};
    int64_t corner_ref[3] = {0, 0, 0};   // > 0: the reference's corner for the Level-1 scales (cx_set_reference_corner)
    int64_t origin4[4] = {0, 0, 0, 0};
    cx_state4* s4 = nullptr;
    cx_state2* s2 = nullptr;
    cx_levels_state* lv = nullptr;
    int lv_current = -1;               // level of cx_extract3d_levels whose mesh the context's output buffers hold (-1: none)
    // Level-0 outputs
    cx_buf<cx_vrec> verts;          // 8-byte vertex records {edge id, fp32 fraction}
    cx_buf<float4> verts_xyz;       // {x, y, z, bits(edge id)} expanded from the records on request (cx_level0_expanded)
    cx_buf<uint4> cells;
    cx_buf<int32_t> tris;           // three per triangle
    // the capacities as the kernels and the ABI count them (cx_params, cx_counts)
    uint32_t vcap() const { return (uint32_t)verts.cap(); }
    uint32_t ccap() const { return (uint32_t)cells.cap(); }
    uint32_t tcap() const { return (uint32_t)(tris.cap() / 3u); }
    cx_buf<uint32_t> counters;
    uint32_t* counters_host = nullptr;
    bool extracted = false;
    bool counts_fetched = false;       // ctx->counts holds the counters of the last 3-D extraction (cx_counts_get)
    cx_counts counts = {0, 0, 0, 0};
    cx_params last;
    // seeded selection (cx_select_seeded3d): triangle mask followed by vertex mask, valid until the next extraction
    cx_buf<uint8_t> tri_keep;
    // scratch of cx_select_seeded3d_ex (bytes), kept between calls: map per sample, union-find, bitmap, flags, seeds, counters, end
    // points, visited set -- a selection allocated and freed them every time (0.8 of 2.9 ms on the 512^3 bench field)
    cx_buf<uint8_t> seed_buf[8];
    int seed_mode = 0;      // how the last seeded selection (3-D or 4-D) ran its end points: 0 sequential (the reference's shared visited set), 1 one thread per pair
    bool keep_valid = false;
    // vertex attributes (cx_attr.hip), kept between calls: Level-0 normals float4 {nx, ny, nz, |g|}, Level-1 normals double[3], sampled
    // values (fp32 at Level 0, float64 at Level 1) and the device copy of a second grid handed over from the host
    cx_buf<float4> attr_n0;
    cx_buf<double> attr_n1;
    cx_buf<float> attr_v0;
    cx_buf<double> attr_v1;
    cx_buf<uint8_t> attr_e1;        // Level 1: per output vertex {sample index of the low point, of the high point, ratio} (16 bytes)
    cx_buf<uint8_t> attr_grid;
    cx_buf<float4> attr_c0;         // curvature: Level 0 float4 {mean, gauss, k1, k2}, Level 1 double[4] in the same order
    cx_buf<double> attr_c1;
    // components of the Level-1 mesh (cx_comp.hip): labels, accumulators and the table, kept between calls
    struct cx_comp_state* comp = nullptr;
    // vertex clustering of the Level-1 mesh (cx_simplify.hip): cluster table, accumulators, scans, kept between calls
    struct cx_simplify_state* simp = nullptr;
    // topology of the Level-1 mesh (cx_topo.hip): edge-use table, boundary loops and the table, kept between calls
    struct cx_topo_state* topo = nullptr;
    // clipping of the Level-1 mesh (cx_clip.hip): bit masks, counts, the edge table of the cut band, the map, kept between calls
    struct cx_clip_state* clip = nullptr;
    // rim caps of the current extraction (cx_cap.hip): sign words, the table of the rim's crossings, the cap itself, kept between calls.
    // cap_valid: they hold the cap of what the context's Level-0 buffers hold now (cleared wherever those change hands)
    struct cx_cap_state* cap = nullptr;
    bool cap_valid = false;
    // choosing isovalues (cx_pick.hip): histograms of the select, difference arrays and tables of the spectrum, the device copy of host
    // samples, kept between calls.  Scratch only: nothing here describes the current extraction
    struct cx_pick_state* pick = nullptr;
    // the whole-volume operations: filter, distance transform, components (the mask of cx_grid_label3d_select), resampling, rank filters,
    // reconstruction.  Each keeps a cx_slot of its own (cx_gridop.h: the device copy of host samples and the context's own result until
    // the operation's _bind makes it the bound grid) beside its scratch, so that none disturbs another's pending result.  Nothing here
    // describes the current extraction
    struct cx_filter_state* filt = nullptr;
    struct cx_dist_state* dist = nullptr;
    struct cx_label_state* label = nullptr;
    struct cx_resample_state* resample = nullptr;
    struct cx_rank_state* rank = nullptr;
    struct cx_recon_state* recon = nullptr;
    // the marker-based watershed (cx_watershed.hip): a seventh slot; its result is int32 labels, which are not a grid to bind
    struct cx_watershed_state* watershed = nullptr;
    // the regions of a labelled volume (cx_regions.hip): scratch, the device records and an eighth slot, the cropped mask of
    // cx_grid_regions3d_select.  The labels are an argument of every call: nothing here refers to them between calls
    struct cx_regions_state* regions = nullptr;
    // Level-1
    cx_post_state* post = nullptr;
    bool post_valid = false;
    cx_buf<unsigned long long> stamps;   // diagnostic stamps (cx_debug_stamps)
    // the context's own RCCL communicator (cx_rccl_comm_init, cx_halo.hip), or null
    void* rccl_comm = nullptr;
    bool rccl_owned = true;              // false: the communicator belongs to another context of this rank (cx_rccl_comm_share)
    int rccl_rank = 0, rccl_world = 1;
    // device -> host copies of mesh-sized buffers (cx_xfer.hip): two pinned staging buffers and their events
    void* xfer_stage[2] = {nullptr, nullptr};
    hipEvent_t xfer_ev[2] = {nullptr, nullptr};
    // timing
    // one set of five markers per timed extraction, all made by cx_timing_enable (never while extracting)
    struct evset { hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}; };
    bool timing = false;
    int nevents = 0;
    evset events[256];
};

// a refusal: the text into the context (where there is one), the code back to the caller
static inline int cx_fail(cx_ctx* ctx, int code, const char* msg) {
    if (ctx) ctx->err = msg;
    return code;
}

template <typename T>
int cx_buf<T>::fail(cx_ctx* ctx, size_t bytes, hipError_t e) {
    ctx->err = std::string("device buffer (") + std::to_string(bytes) + " bytes): " + hipGetErrorString(e);
    return (e == hipErrorOutOfMemory) ? CX_ERR_NOMEM : CX_ERR_HIP;
}
template <typename T>
hipError_t cx_buf<T>::alloc(cx_ctx* ctx, size_t n) {
    void* fresh = nullptr;
    const hipError_t e = hipMalloc(&fresh, n * sizeof(T));
    if (e != hipSuccess) return e;
    p_ = static_cast<T*>(fresh); cap_ = n; tally_ = &ctx->tally;
    tally_->live_bytes += (int64_t)bytes(); tally_->allocations++;
    cx_process_tally.live_bytes += (int64_t)bytes(); cx_process_tally.allocations++;
    return hipSuccess;
}
// Room for `need` elements, contents not kept: waits for the context's stream first (kernels enqueued on it may still use the old
// buffer), frees, allocates exactly `need`.
template <typename T>
int cx_buf<T>::grow(cx_ctx* ctx, size_t need) {
    if (cap_ >= need && p_) return CX_OK;
    if (need == 0) return CX_OK;
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess && p_) e = hipFree(p_);
    forget();
    if (e == hipSuccess) e = alloc(ctx, need);
    return e == hipSuccess ? CX_OK : fail(ctx, need * sizeof(T), e);
}
// The same for a buffer that is appended to (the slab assembly of cx_slab4d.hip): the first `used` elements move into the new buffer,
// which gets room for half as many again as before when that is more than `need` (a volume of many slabs grows it a few times, not
// once per slab).
template <typename T>
int cx_buf<T>::grow_keep(cx_ctx* ctx, size_t used, size_t need) {
    if (cap_ >= need && p_) return CX_OK;
    if (need == 0) return CX_OK;
    const size_t want = need > cap_ + cap_ / 2 ? need : cap_ + cap_ / 2;
    cx_buf fresh;
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = fresh.alloc(ctx, want);
    if (e == hipSuccess && p_ && used) e = hipMemcpyAsync(fresh.p_, p_, used * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, want * sizeof(T), e);
    *this = std::move(fresh);
    return CX_OK;
}

// cx_api.hip
// `buf` (n0 n1 n2 samples of `dtype`) becomes the bound grid, owned by the context: what cx_grid_upload_typed does once its samples are
// in place.  Everything that described the previous grid is reset, the previous owned grid is released; `buf` is left empty.  On a
// shape the march does not take nothing changes.
int cx_grid_bind_owned(cx_ctx* ctx, cx_buf<uint8_t>& buf, int32_t dtype, int64_t n0, int64_t n1, int64_t n2);
int cx_ensure_cell_records(cx_ctx* ctx);
int cx_ensure_hash_xy(cx_ctx* ctx, uint32_t flags);
int cx_level0_expanded(cx_ctx* ctx, float4** out);   // the records of the current extraction as float4 {x,y,z,id} (device, enqueued on the stream)
void cx_fill_value_params(cx_params& P, double value);
void cx_base_params(const cx_ctx* ctx, double value, uint32_t flags, cx_params& P);   // P zeroed, then the grid, its shape and origin, the value fields, the flags
struct cx_staged_sizes {      // what the staged pipeline's side tables hold for one extraction (elements, not bytes)
    size_t nw;                // streaming waves
    size_t need;              // queue entries: every wave's region of T.wcap
    size_t qa;                // queue words per (wave, plane step, lane)
    size_t chunk_words;       // totals of the scan's chunks of 256 waves
    size_t boundary;          // samples on three faces of the array
};
cx_staged_sizes cx_staged_sizes_of(const cx_ctx* ctx, const cx_task& T);
// cx_halo.hip
void cx_rccl_comm_free(cx_ctx* ctx);
// cx_xfer.hip
int cx_copy_to_host(cx_ctx* ctx, int nparts, void* const* dst, const void* const* src, const size_t* bytes);
int cx_copy_to_host1(cx_ctx* ctx, void* dst, const void* src, size_t bytes);
void cx_xfer_free(cx_ctx* ctx);
// cx_levels.hip
void cx_levels_free(cx_ctx* ctx);
void cx_levels_invalidate(cx_ctx* ctx);
void cx_levels_unselect(cx_ctx* ctx);
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
// what cx_clip.hip writes for the same tail: nv_raw points (the old vertices in their order, then the cut vertices), prio = the
// vertex's place in that list, nt_raw triangles with tprio3 = {source triangle} x 3, all of them alive
struct cx_level1_clip_io {
    double* pts;
    uint32_t* prio;
    int32_t* tri;
    uint32_t* tprio3;
    uint8_t* alive;
};
int cx_level1_clip_bufs(cx_ctx* ctx, size_t nv_raw, size_t nt_raw, cx_level1_clip_io* out);
int cx_level1_clip_tail(cx_ctx* ctx, uint32_t nv_raw, uint32_t nt_raw, bool do_clean, int64_t* counts);
int cx_level1_clip_normals(cx_ctx* ctx, double** out);
uint64_t cx_level1_generation(cx_ctx* ctx);
// cx_comp.hip
void cx_comp_free(cx_ctx* ctx);
int cx_comp_labels_get(cx_ctx* ctx, const char* who, cx_level1_comp_view* V, const int32_t** tlab, const int32_t** vlab, uint32_t* nc);
// cx_topo.hip
void cx_topo_free(cx_ctx* ctx);
// cx_simplify.hip
void cx_simplify_free(cx_ctx* ctx);
// cx_clip.hip
void cx_clip_free(cx_ctx* ctx);
// cx_cap.hip: the cap of the current extraction for the post-pass (cx_postprocess3d_capped): ncv vertex records {key, 0} in ascending
// key and nct index triples into the Level-0 vertices followed by them.  CX_ERR_STATE without a valid cap, CX_ERR_UNSUPPORTED on the
// routes no cap is built for.
void cx_cap_free(cx_ctx* ctx);
struct cx_cap_view {
    const cx_vrec* vrec;
    const int32_t* tris;
    uint32_t ncv, nct;
};
int cx_cap_view_get(cx_ctx* ctx, const char* who, cx_cap_view* out);
// cx_pick.hip
void cx_pick_free(cx_ctx* ctx);
// cx_filter.hip
void cx_filter_free(cx_ctx* ctx);
// cx_dist.hip
void cx_dist_free(cx_ctx* ctx);
// cx_label.hip
void cx_label_free(cx_ctx* ctx);
// cx_resample.hip
void cx_resample_free(cx_ctx* ctx);
// cx_rank.hip
void cx_rank_free(cx_ctx* ctx);
// cx_recon.hip
void cx_recon_free(cx_ctx* ctx);
// cx_watershed.hip
void cx_watershed_free(cx_ctx* ctx);
// cx_regions.hip
void cx_regions_free(cx_ctx* ctx);
bool cx_level1_capped(cx_ctx* ctx);   // cx_post.hip: the Level-1 mesh came out of cx_postprocess3d_capped (or is a filtered copy of one)
// cx_api4d.hip
void cx_state4_free(cx_ctx* ctx);
// cx_contour2d.hip
void cx_state2_free(cx_ctx* ctx);
