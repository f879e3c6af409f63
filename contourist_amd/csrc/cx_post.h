// cx_post.h -- what the Level-1 post-pass files share (cx_post.hip, cx_write.hip, cx_post4d.hip, cx_morph.hip): the one state struct
// behind cx_ctx::post and the host helpers that more than one of them calls.  Host side only; private to those four files.
// A kernel is launched only from the translation unit that defines it: the few small kernels of cx_post.hip that the other files
// need are reached through the host functions at the end, which make the launch there.
#pragma once
#include <vector>

#include "cx_ctx.h"
#include "cx_dev.h"

struct cx_post_state {
    cx_buf<uint8_t> pts, prio, rep, tri, alive, parent, parent2, tkeys, tvals, flags, scan, blocksums, pts_out, tri_out, comp, misc;
    cx_buf<uint8_t> keys_out, keys_tmp, told, cls, bnd;   // edge ids of the output vertices; sharded Level 1 (cx_postprocess3d_shard_*)
    cx_buf<uint8_t> ever;                                 // vertices something was ever merged into: u8[nv] before | u8[nv2] after the compaction
    bool keys_valid = false;
    // vertex attributes (cx_attr.hip).  keys_edge: keys_out holds edge ids of the resident array (cx_postprocess3d*, not a caller's mesh
    // and not a shard).  orient_live: S->parent / S->comp still hold the component roots and flips of the orientation step for the
    // orient_nt triangles of tri_out; vflip: per output vertex, 1 = its component's triangles were reversed (filled on first request)
    cx_buf<uint8_t> vflip;
    bool keys_edge = false, orient_live = false, vflip_valid = false;
    uint32_t orient_nt = 0;
    // components (cx_comp.hip).  shard_mesh: the mesh came out of cx_postprocess3d_shard_finish (its components reach other ranks);
    // corner: the grid box the 3-D post-pass worked in; gen: counts the meshes this state has held (every post-pass and every
    // cx_level1_keep_components make a new one): what cx_comp.hip caches belongs to one value of it
    bool shard_mesh = false;
    double corner[3] = {1.0, 1.0, 1.0};
    uint64_t gen = 0;
    // simplification (cx_simplify.hip).  simplified: the mesh came out of cx_level1_simplify (its keys are vertex indices of the mesh
    // before); carried: nrm[nrm_cur] holds one unit normal per vertex of it, carried over from the members of its clusters;
    // smap: new index of every vertex of the mesh before the last simplification
    cx_buf<uint8_t> nrm[2], nrm_tmp, smap;
    int nrm_cur = 0;
    bool simplified = false, carried = false, smap_valid = false;
    bool clipped = false;             // the derived mesh came out of cx_level1_clip_* (cx_clip.hip): old vertices and cut vertices
    uint32_t smap_n = 0;
    // rim caps (cx_cap.hip): the mesh of generation capped_gen came out of cx_postprocess3d_capped, or is a filtered copy of one: its keys
    // are edge ids AND lattice points (direction 0), a crease runs along its rim and no normal or curvature is served for it
    uint64_t capped_gen = 0;
    bool capped() const { return capped_gen != 0 && capped_gen == gen; }
    struct {
        bool open = false;            // between cx_postprocess3d_shard_begin and _finish
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
    int64_t nv_out = 0, nt_out = 0;
    int64_t ms_out = 0, mt_out = 0;
};

// the state of the context, made on first use; its misc words are reserved.  Every post-pass starts here (the morph triangles of an
// earlier cx_morph_triangles do not survive it)
int cxp_state(cx_ctx* ctx, cx_post_state** out);

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
// the sharded Level 1 works between them.  comp: the component tables, nt * (3 u64 + 1 u32) bytes laid out as
// cmaxx u64[nt] | cbest (the flip, once decided) u64[nt] | cmaxv u64[nt] | cstart u32[nt].  keys: what breaks a tie between vertices
// at the largest x (null: the largest index); cls: the classes of a shard's triangles (null: all own); clist: room for nt u32;
// misc: the state's misc words ([0] flatten flag, [3] component count, [11] list length).
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
