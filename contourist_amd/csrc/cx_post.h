// cx_post.h -- what the Level-1 post-pass files share (cx_post.hip, cx_write.hip, cx_post4d.hip, cx_morph.hip): the one state struct
// behind cx_ctx::post and the host helpers that more than one of them calls.  Host side only; private to those four files (and to
// cx_slab4d.hip for cxp_tets4d).
// A kernel is launched only from the translation unit that defines it: the few small kernels of cx_post.hip that the other files
// need are reached through the host functions at the end, which make the launch there.
#pragma once
#include <vector>

#include "cx_ctx.h"
#include "cx_dev.h"

// ---- what the buffers hold -----------------------------------------------------------------------------------------------------------
// ONE record says what pts / tri / pts_out / tri_out / keys_out and the orientation tables (parent, comp) hold.  The rule:
//   cxp_begin         every producer calls it before its first write into pts, tri, pts_out or tri_out (after the checks of its input
//                     that can still refuse the call: a refused call leaves the resident mesh alone).  Whatever was resident, 3-D or 4-D,
//                     is gone from then on; a producer that fails later leaves NOTHING resident.
//   cxp_publish       a producer's last step: what the buffers hold now and where it came from; hands the counts to the caller.
//   cxp_tables_taken  the memory of the orientation tables was used for something else.
//   cxp_mesh3d / cxp_tets4d   the two questions a reader asks.  No reader looks at the fields themselves before one of them said yes.
// ctx->post_valid and cx_state4::post_valid stay what the files outside the post-pass clear when the extraction under a result changes;
// here only cxp_begin and cxp_publish write them, and the two predicates read them.
struct cxp_record {
    enum holds_t : uint8_t { NOTHING, MESH3D, SHARD_OPEN, TETS4D };            // SHARD_OPEN: between cx_postprocess3d_shard_begin and _finish
    enum origin_t : uint8_t { GRID, CALLER_MESH, SHARD, SIMPLIFIED, CLIPPED };
    holds_t holds = NOTHING;
    // GRID: the keys are edge ids of the resident array (cx_postprocess3d*, and what cx_level1_keep_components leaves of such a mesh);
    // CALLER_MESH: cx_postprocess3d_mesh (the keys are the caller's indices); SHARD: cx_postprocess3d_shard_finish (its components reach
    // other ranks); SIMPLIFIED / CLIPPED: derived by cx_level1_simplify / cx_level1_clip_* (the keys are indices into the mesh before)
    origin_t origin = GRID;
    bool capped = false;             // out of cx_postprocess3d_capped, or a filtered copy of such a mesh: the keys are edge ids AND lattice points
                                     // (direction 0), a crease runs along the rim and no normal or curvature is served
    bool normals_carried = false;    // nrm[nrm_cur] holds one unit normal per vertex (a derived mesh that carries them)
    bool tables_live = false;        // parent / comp hold the component roots and flips of the orientation step for tables_nt triangles of tri_out
    uint32_t tables_nt = 0;
    bool vflip_cached = false;       // vflip: per output vertex, 1 = its component's triangles were reversed (filled on first request)
    bool map_live = false;           // smap: the new index of each of the map_n vertices of the mesh before the last simplification
    uint32_t map_n = 0;
    uint64_t gen = 0;                // counts the meshes the state has held: what cx_comp.hip and cx_topo.hip cache belongs to one value of it
    bool derived() const { return origin == SIMPLIFIED || origin == CLIPPED; }
    bool tables_for(uint32_t nt) const { return tables_live && tables_nt == nt; }
};

// ---- named layouts of the byte buffers ------------------------------------------------------------------------------------------------
// the raw input mesh of the 3-D post-pass as cxp_reserve_raw laid it out (valid until one of its buffers is grown for something else:
// from a producer's reserve to the end of its tail).  tprio3: the triangles' priority triples, behind the triangles in S->tri
struct cxp_raw {
    double* pts = nullptr;
    uint32_t* prio = nullptr;
    int32_t* tri = nullptr;
    uint32_t* tprio3 = nullptr;
    uint8_t* alive = nullptr;
    u64* parent2 = nullptr;
};
// the component tables of the orientation step for nt triangles: cmaxx u64[nt] | cflip (cbest until the flip is decided) u64[nt] |
// cmaxv u64[nt] | cstart u32[nt]
struct cxp_comp_tables {
    u64 *cmaxx, *cflip, *cmaxv;
    uint32_t* cstart;
};
static inline size_t cxp_comp_bytes(size_t nt) { return nt * (3 * sizeof(u64) + sizeof(uint32_t)); }
static inline cxp_comp_tables cxp_comp_view(u64* comp, size_t nt) { return {comp, comp + nt, comp + 2 * nt, (uint32_t*)(comp + 3 * nt)}; }
// the words of S->misc (u32).  Words that stand side by side are read back in one copy: TOTAL0..NCOMP, WELD..TINY, BND_N..BND_NCAND
enum : uint32_t {
    CXP_M_CHANGED = 0,        // the flag of the pointer jumping (cxp_flatten)
    CXP_M_TOTAL0 = 1,         // totals of a compaction or a scan: vertices (3-D), morph triangles
    CXP_M_TOTAL1 = 2,         //   triangles (3-D), tetrahedra (4-D), morph segments
    CXP_M_NCOMP = 3,          // components counted by the winding kernel
    CXP_M_WELD = 4,           // triangles alive after the weld (4-D: after drop_instant)
    CXP_M_TINY = 5,           //   and after the tiny collapse
    CXP_M_SHARD_N = 6,        // 6, 7: a shard's own triangles next to the lower neighbour, its copies of the upper neighbour's
    CXP_M_BND_N = 8,          // 8, 9: the same two as the boundary kernel wrote them
    CXP_M_BND_NCAND = 10,     //   and the open components (start-triangle candidates)
    CXP_M_CLIST = 11,         // length of the list of possible start triangles
    CXP_M_OVER = 12,          // the small edge table of the block linking overflowed
    CXP_M_MINMAX_T = 16,      // 16..19: orderable min / max of the time of all points, two u64 (cx_morph.hip)
    CXP_M_MAXDUR = 20,        // 20, 21: longest life of a morph triangle / segment, one u64
    CXP_M_SB_TOTAL = 22,      // total of the start-time sort's count matrix
    CXP_M_SB_STARTS = 32,     // 32..288: bin starts of the start-time sort (CXP_SB_BINS + 1 words)
    CXP_M_WORDS = 512
};

struct cx_post_state {
    cxp_record rec;
    cx_buf<uint8_t> pts, prio, rep, tri, alive, parent, parent2, tkeys, tvals, flags, scan, blocksums, pts_out, tri_out, comp, misc;
    cx_buf<uint8_t> keys_out, keys_tmp, told, cls, bnd;   // edge ids of the output vertices; sharded Level 1 (cx_postprocess3d_shard_*)
    cx_buf<uint8_t> ever;                                 // vertices something was ever merged into: u8[nv] before | u8[nv2] after the compaction
    cx_buf<uint8_t> vflip;                                // rec.vflip_cached (cx_attr.hip)
    cx_buf<uint8_t> nrm[2], nrm_tmp, smap;                // rec.normals_carried: nrm[nrm_cur]; rec.map_live: smap (cx_simplify.hip, cx_clip.hip)
    int nrm_cur = 0;
    cxp_raw raw;
    double corner[3] = {1.0, 1.0, 1.0};                   // the grid box the 3-D post-pass worked in
    int64_t nv_out = 0, nt_out = 0;                       // vertices and triangles (tetrahedra) of what rec.holds says is resident
    struct {                          // sizes of an open shard (rec.holds == SHARD_OPEN)
        uint32_t nv2 = 0, nt2 = 0;    // mesh of own + first-halo-layer triangles the labels refer to
        uint32_t nt_in = 0;           // triangles the post-pass started from (layout of S->cls)
        uint32_t n1 = 0, n4 = 0, ncand = 0;   // own triangles next to the lower neighbour, copies of the upper neighbour's, open components
    } shard;
    cx_buf<uint8_t> mpairs, msegs, mtris, mmid, mtime, mnext;   // morph triangles (4-D)
    // The morph triangles and their segments are kept SORTED by the bin of their start time (cxp_morph_sort_by_start, the last step of
    // cx_morph_triangles): the triangles that exist at a time t are then a window of ids, and so are their segments.
    cx_buf<uint8_t> msegs2, mtris2, mtime2;                     // the other halves of the double buffers the sort writes into
    cx_buf<uint8_t> meflags, metflag, menew, mecnt, medesc, me_pts, me_tri;   // cx_morph_eval_many: segment flag bytes (ALL zero between two calls) / triangle flag bytes / new point ids / block counts of the windows, per-time descriptors, outputs
    void* me_pinned = nullptr;                          // 48 KB of pinned host memory: descriptors up (36 KB), totals back (12 KB) without staging copies
    bool meflags_clean = false;                         // the segment flag bytes are all zero (the kernels that consume a flag clear it)
    uint32_t mbin_t[257] = {0}, mbin_s[257] = {0};      // first triangle / segment of every start-time bin (CXP_SB_BINS + 1 entries)
    double mt_lo = 0.0, mt_inv_width = 0.0;             // the bins: bin(x) = (x - mt_lo) * mt_inv_width, clamped (cxp_sb_bin)
    double mt_maxdur = 0.0, ms_maxdur = 0.0;            // longest life of a triangle / a segment
    bool msorted = false;
    std::vector<int64_t> me_off;                        // last cx_morph_eval_many: per time {first point, points, first triangle, triangles}
    int64_t ms_out = 0, mt_out = 0;
};

// the state of the context, made on first use; its misc words are reserved.  Every post-pass starts here (the morph triangles of an
// earlier cx_morph_triangles do not survive it)
int cxp_state(cx_ctx* ctx, cx_post_state** out);
void cxp_begin(cx_ctx* ctx, cx_post_state* S);
// counts: the eight counters of the call (copied to out_counts when that is given); returns CX_OK
int cxp_publish(cx_ctx* ctx, cx_post_state* S, cxp_record::holds_t holds, cxp_record::origin_t origin, const int64_t* counts, int64_t* out_counts);
static inline void cxp_tables_taken(cx_post_state* S) { S->rec.tables_live = false; S->rec.gen++; }   // (what cx_comp.hip cached of them is stale)
bool cxp_mesh3d(const cx_ctx* ctx);      // a 3-D Level-1 mesh is resident: pts_out, tri_out, keys_out, nv_out, nt_out
bool cxp_tets4d(const cx_ctx* ctx);      // the 4-D post-pass's points (pts) and tetrahedra (tri_out) are resident

// edge tables: n = 3 * triangles is an upper bound that only an open mesh without shared edges reaches; a closed
// mesh has half as many distinct edges.  5/4 of the bound keeps the worst case below a load of 0.8 and the usual
// case near 0.25-0.4 with half the footprint (the table is touched at random: footprint is what costs)
static inline u64 cxp_edge_table_size(size_t n) {
    u64 s = 1024;
    while (s < (5 * (u64)n) / 4 + 16) s <<= 1;
    return s;
}
// (measured and dropped: half that size for the meshes of the march, whose edges are nearly all shared by two triangles, with a
// repeat on overflow -- the fill gets 0.23 ms cheaper, the claim kernel 0.74 ms dearer: rows of 5 slots per vertex instead of 11
// run into each other)

// exclusive scan of n u32 on the context's stream (block sums in S->blocksums); the total goes to *total_dev
int cxp_scan(cx_ctx* ctx, cx_post_state* S, const uint32_t* in, uint32_t* out, uint32_t n, uint32_t* total_dev);

// Orientation of the components of a triangle mesh whose union-find (parent, one u64 per triangle) has been built; two halves, because
// the sharded Level 1 works between them.  comp: the component tables (cxp_comp_view, cxp_comp_bytes(nt) bytes).  keys: what breaks a
// tie between vertices at the largest x (null: the largest index); cls: the classes of a shard's triangles (null: all own); clist: room
// for nt u32; misc: the state's misc words (CXP_M_CHANGED, CXP_M_NCOMP, CXP_M_CLIST).
//   cxp_orient_pick     flattens parent and picks every component's start triangle (through cxp_k_comp_pick)
//   cxp_orient_decide   decides the flips (cbest); wind: also reverses the triangles of the flipped components and enqueues the copy of
//                       the component count into *ncomp -- valid after the caller's next synchronisation of the stream
int cxp_orient_pick(cx_ctx* ctx, const int32_t* tri, uint32_t nt, const double* pts, u64* parent, u64* comp, const uint32_t* keys,
                    const uint8_t* cls, uint32_t* clist, uint32_t* misc);
int cxp_orient_decide(cx_ctx* ctx, int32_t* tri, uint32_t nt, const double* pts, const u64* parent, u64* comp, const uint32_t* clist,
                      uint32_t* misc, bool wind, uint32_t* ncomp);

// launches of kernels that cx_post.hip defines, on stream st, with the grid and block every caller used
void cxp_iota64(hipStream_t st, u64* a, uint32_t n);                                              // a[i] = i
void cxp_fill64(hipStream_t st, u64* a, size_t n, u64 v);                                         // a[i] = v
void cxp_count_alive(hipStream_t st, const uint8_t* alive, uint32_t nt, uint32_t* counter);       // *counter += non-zero bytes
void cxp_alive_u32(hipStream_t st, const uint8_t* alive, uint32_t nt, uint32_t* out);             // out[t] = alive[t] != 0
void cxp_scan_sums(hipStream_t st, uint32_t* sums, uint32_t nb, uint32_t* total);                 // exclusive scan of block sums in place, one workgroup
