// cx_state4.h -- parameters and per-context state of the 4-D march (host side).
#pragma once
#include "cx_ctx.h"

struct cx_params4 {
    const float* grid;
    uint32_t n0, n1, n2, n3, nsamples;
    cx_fdiv div3, div2, div1;
    float vcmp, near_abs, vhi, vlo;
    double value, tol_value;
    uint32_t flags;
    uint32_t org[4];
    // where the vertices of a lattice cell are, without a table of one entry per sample (rounds 1-3: 8 bytes per sample, 1 GiB on config 4):
    // the cells of one bitmap word (32 cells of a row) sit next to each other in the queue, so
    //     queue position of cell (row, l) = items[row * nw3 + l / 32].x + popc(items[...].y & bits below l % 32)
    // and the cells kernel leaves (crossing mask << 32 | first vertex) per QUEUE ENTRY, densely
    uint2* items;              // [nrows * nw3] {queue position of the word's first active cell, the word's active cells}; written for words with one
    uint64_t* info;            // [qcap] per queue entry
    float4* verts;
    uint32_t* vkeys;
    uint4* cells;
    int32_t* tets;
    uint32_t vcap, ccap, tcap;
    uint32_t* counters;
    unsigned long long* counters_tb;   // (border voxels << 32) | tetrahedra: reserved by the cells kernel, in a cache line of its own
    const uint64_t* hash_xyz;
    const uint64_t* lut;
    uint32_t* queue;           // linear indices of the cells with a sign change among their corners
    uint32_t qcap;
    uint4* rounds;             // per 64 queue entries: first record, records, first tetrahedron, tetrahedra
    // sign bitmap: bit l%32 of word [row(i,j,k)][l/32] <=> sample < isovalue
    uint32_t* signbits;
    uint32_t nw3;              // words per row
    uint32_t nrows;            // n0*n1*n2
    cx_fdiv div_w, div_r2, div_r1;   // / nw3, / (n1*n2), / n2
};
#define CX4_CNT_QUEUE 6   // counter word: cells in the queue
void cx_launch_signbits4d(const cx_params4& P, hipStream_t s);
void cx_launch_classify4d(const cx_params4& P, hipStream_t s);
void cx_launch_emit_tets(const cx_params4& P, hipStream_t s);
void cx_launch_hash_xyz(uint64_t* table, uint32_t n0, uint32_t n1, uint32_t n2, const uint32_t org[4], hipStream_t s);
const uint64_t* cx_pent_lut_device();

// Assembly of a volume marched slab by slab along axis 0 (cx_slab4d_begin / _append / _finish; cx_slab4d.hip, cx_post4d.hip).  Slab
// i0 .. i1 is marched with origin (i0,0,0,0) and, unless it is the last, with plane i1 as a halo.  Its OWNED vertices (lower lattice
// point below the halo) are appended in ascending edge id, so the whole assembly is in ascending GLOBAL edge id; tetrahedra are
// appended with assembly indices, a reference to a halo vertex is held as -(1 + h) until the next append resolves entry h of `pend`.
// The four assembly buffers grow by cx_buf::grow_keep (which keeps their contents); kernels get pointers taken after the last grow.
struct cx_slab4 {
    bool open = false;              // between cx_slab4d_begin and cx_slab4d_finish
    int64_t whole[4] = {0, 0, 0, 0};
    int64_t next_i0 = 0;            // plane the next append starts at
    int64_t nslabs = 0;
    double value = 0.0;             // isovalue of the first slab (every slab must use it)
    uint32_t nv = 0, nt = 0;        // assembled vertices / tetrahedra
    uint32_t npend = 0;             // halo vertices of the last slab, resolved by the next append
    uint32_t pend_t0 = 0;           // first tetrahedron of the last slab (the only ones that may hold pending references)
    cx_buf<uint64_t> keys;          // [nv] global edge id ((linear index in the whole volume << 4) | direction)
    cx_buf<double> pts;             // [nv * 4] float64 crossing points in the whole volume's lattice (t not yet binned)
    cx_buf<int32_t> tets;           // [nt * 4]
    cx_buf<uint32_t> pend;          // [npend] the next slab's local edge ids of the last slab's halo vertices
    // scratch of one append: radix sort of (edge id, source) pairs, digit counts per unit, their scan, vertex map
    cx_buf<uint32_t> ka, kb, va, vb;
    cx_buf<uint32_t> hist, offs, sums, flag, pos;
    cx_buf<int32_t> vmap, resolved;
    cx_buf<uint32_t> cnt;           // [16] device counters
};
void cx_slab4_free(cx_slab4*& A);

struct cx_state4 {
    const float* grid = nullptr;     // the samples in use: grid_owned or an adopted array (not owned)
    cx_buf<float> grid_owned;
    int64_t n[4] = {0, 0, 0, 0};
    cx_buf<uint2> items;
    cx_buf<uint64_t> info;
    cx_buf<float4> verts;
    cx_buf<uint32_t> vkeys;          // one per vertex of `verts`
    cx_buf<uint4> cells;
    cx_buf<int32_t> tets;            // four per tetrahedron
    cx_buf<uint64_t> hash_xyz;
    cx_buf<uint32_t> queue;
    cx_buf<uint4> rounds;
    cx_buf<uint32_t> signbits;
    // the capacities as the kernels and the ABI count them (cx_params4, cx_counts)
    uint32_t vcap() const { return (uint32_t)verts.cap(); }
    uint32_t ccap() const { return (uint32_t)cells.cap(); }
    uint32_t tcap() const { return (uint32_t)(tets.cap() / 4u); }
    uint32_t qcap() const { return (uint32_t)queue.cap(); }
    int64_t hash_key[7] = {-1, -1, -1, -1, -1, -1, -1};
    int64_t origin[4] = {0, 0, 0, 0};
    bool extracted = false;
    bool post_valid = false;
    bool post_assembled = false;     // the post-pass result is a slab assembly's (cx_slab4d_finish): tetrahedra already oriented, G->grid not its own
    cx_slab4* slab = nullptr;
    bool pending = false;            // a cx_extract4d_async is enqueued, its counters not yet looked at (cx_counts4d_get)
    double pending_value = 0.0;
    uint32_t pending_flags = 0;
    double value = 0.0;
    cx_counts counts = {0, 0, 0, 0};
    // seeded selection (cx_select_seeded4d): mask over the Level-0 tetrahedra, valid until the next extraction
    cx_buf<uint8_t> tet_keep;
    bool keep_valid = false;
};
