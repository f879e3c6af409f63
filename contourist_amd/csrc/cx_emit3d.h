#pragma once
// cx_emit3d.h -- the PER-CELL EMIT code of the 3-D march: the formats of queue entries, info words and cell records, and what every
// emitting kernel runs per queued cell (cx_process_queue: the reference's tolerance rules cell by cell; cx_fast_geom, cx_vround /
// cx_emit_queue_fast and cx_tround / cx_emit_queue_t: rounds of 64 cells, one lane per vertex), the counts from the sign bits
// (cx_cnt) and the packed row masks of the stream kernel (cx_rowmask, cx_lmasks).  It defines no kernel; the vertex
// stage, the generic kernel, the fused kernel and the tile kernels call it.
// A section of the cx_march3d.hip translation unit: included only there, in this place, and not self-contained.  It is the first
// section: it relies on the tunables and the three device tables at the head of cx_march3d.hip (and on cx_cell.h, cx_dev.h).

// the word the vertex stage leaves per queue entry (staged pipeline): bits 0-31 first vertex of the cell, 32-39 crossing mask
// (bit d: the cell owns a crossing on its edge in direction d), 40-43 triangles of its voxel, 44-49 tetrahedra that emit nothing
// (the reference's tolerance skips; all six for a cell that is no voxel).  Everything the triangle stage needs about a cell besides
// its queue entry: it walks queue entries, not cell records (cx_k_emit_triangles_e).
__device__ __forceinline__ uint64_t cx_info_word(uint32_t vfirst, uint32_t emask, uint32_t ntri, uint32_t tetskip) {
    return (uint64_t)vfirst | ((uint64_t)((emask & 0xFFu) | ((ntri & 0xFu) << 8) | ((tetskip & 0x3Fu) << 12)) << 32);
}

// the record of one cell, at place `at` of the record array.  Full: 16 bytes {lin, word, first triangle, first vertex}.  Slim
// (P.write_records == CX_RECORDS_SLIM, the record-walking triangle kernel of the staged pipeline): 8 bytes {lin, word} in the front
// half of the same allocation; the two running numbers of every 64th record go to P.cbase, and the triangle kernel -- whose waves
// take 64 consecutive records from a multiple of 64 -- adds the prefixes of ntri and popc(emask) inside the group: records, vertices
// and triangles are all numbered along the flat batch list.
__device__ __forceinline__ void cx_store_cell_record(const cx_params& P, uint32_t at, uint32_t lin, uint32_t word, uint32_t tfirst, uint32_t vfirst) {
    if (P.write_records == CX_RECORDS_SLIM) {   // uniform
        reinterpret_cast<uint2*>(P.cells)[at] = make_uint2(lin, word);
        if ((at & 63u) == 0u) P.cbase[at >> 6] = make_uint2(tfirst, vfirst);
    } else {
        P.cells[at] = make_uint4(lin, word, tfirst, vfirst);
    }
}

// ---- per-cell path ------------------------------------------------------------------------------
struct cx_run {
    uint32_t v, t, c, b;   // running vertex / triangle / cell-record / border-voxel counts
    uint32_t s;            // count pass: owned crossings whose two samples differ by <= 1e-8 (the reference's ratio = 0.5 rule)
};

// one sweep over queued cells, re-reading their corners and applying the reference's tolerance rules
// exactly.  emit == false: only count into `run` (from zero); emit == true: `run` holds the bases and
// advances as vertex records and table entries (RECORDS: and cell records) are written.
#define CX_VSTAGE 256u   // vertex records a wave stages in LDS per batch of 64 cells (typical: ~200)
#define CX_VSTAGE_LDS 384u   // float4 slots per wave in the vertex stage's LDS (fast path: 2 x 448 slot words + 64 x 9 corner samples)
template <bool RECORDS, int DT, typename LinOf>
__device__ __forceinline__ void cx_process_queue(const cx_params& P, LinOf lin_of, uint32_t n, uint32_t lane,
                                                 bool emit, cx_run& run, cx_vrec* vstage, uint64_t* info = nullptr) {
    const uint32_t plane = P.n1 * P.n2;
    for (uint32_t b0 = 0; b0 < n; b0 += 64u) {
        const uint32_t idx = b0 + lane;
        const bool have = idx < n;
        const uint32_t lin = have ? lin_of(idx) : 0u;
        const uint32_t i = cx_div(lin, P.div_plane);
        const uint32_t r = lin - i * plane;
        const uint32_t j = cx_div(r, P.div_row);
        const uint32_t k = r - j * P.n2;
        float f[8];
        const uint32_t vm = cx_load_corners<DT>(P, lin, i, j, k, f);
        const uint32_t sm = cx_sign_mask(P, f);
        const uint32_t smv = sm & vm;
        const bool active = have && smv != 0u && smv != vm;
        cx_cell_info R;
        R.sm = sm; R.emask = 0; R.ntri = 0; R.tetskip = 0; R.border = 0;
        if (active) R = cx_classify_cell<DT>(P, f, vm, sm, i, j, k);
        const uint32_t nv = __popc(R.emask);
        const bool rec = active && (nv != 0u || R.ntri != 0u);
        uint32_t vtot, ttot;
        const uint32_t vpre = cx_wave_prefix_small<3>(nv, vtot);
        const uint32_t tpre = cx_wave_prefix_small<4>(R.ntri, ttot);
        const uint64_t recm = __ballot(rec);
        const uint32_t ctot = (uint32_t)__popcll(recm);
        const uint32_t btot = (uint32_t)__popcll(__ballot(R.border != 0u));
        if (!emit) {
            bool flat = false;   // a crossing the fp32 interpolation of the fast path must not take
#pragma unroll
            for (uint32_t d = 1; d < 8; d++) flat |= ((R.emask >> d) & 1u) && fabsf(f[d] - f[0]) <= 1.001e-8f;
            run.s += (uint32_t)__popcll(__ballot(flat));
        }
        if (emit) {
            const uint32_t vfirst = run.v + vpre;
            if (run.v + vtot <= P.vcap) {
                if (vtot <= CX_VSTAGE) {
                    // the wave's vertices of this batch are one contiguous run of the vertex array:
                    // stage them in LDS, then write full 16-byte-per-lane rows
                    if (nv) cx_emit_vertices(P, f, R.emask, lin, i, j, k, [&](uint32_t r2, const cx_vrec& rec4) { vstage[vpre + r2] = rec4; });
                    if (!P.records_only)
                        for (uint32_t o = lane; o < vtot; o += 64u) P.verts[run.v + o] = vstage[o];
                } else if (nv && !P.records_only) {
                    cx_emit_vertices(P, f, R.emask, lin, i, j, k, [&](uint32_t r2, const cx_vrec& rec4) { P.verts[vfirst + r2] = rec4; });
                }
                // (first vertex, crossing mask) of the cell for the triangle stage: per queue entry (staged pipeline), or in
                // the table of one entry per sample (generic classify kernel)
                if (info) { if (have && !P.records_only) info[idx] = cx_info_word(vfirst, R.emask, R.ntri, R.tetskip); }
                else if (nv && !P.records_only) P.celltab[lin] = ((uint64_t)R.emask << 32) | (uint64_t)vfirst;
            }
            if (RECORDS && (P.write_records || !info) && rec && run.c + ctot <= P.ccap) {
                cx_store_cell_record(P, run.c + cx_mbcnt(recm), lin, sm | (R.tetskip << 8) | (R.ntri << 16) | (R.emask << 24), run.t + tpre, vfirst);
            }
        }
        run.v += vtot; run.t += ttot; run.c += ctot; run.b += btot;
    }
}

// ---- packed queue entries of the staged pipeline (one u32 per active cell):
//   bits 0-9    corner signs as extracted from the packed plane words: bits 0,1 = corners 0,1;
//               bits 2,3 = corners 4,5; bits 6,7 = corners 2,3; bits 8,9 = corners 6,7
//   bits 10-14  position of the cell inside its lane's packed word (6*row + m)
//   bits 15-20  streaming lane (k = k0 + 4*lane + m)
//   bits 21-27  plane offset inside the task
// A wave waits for the loads it issued at the top of an iteration AFTER the iteration's stores, not before them (as rounds 1 and 2
// did -- a wait issued behind stores retires them too, `s_waitcnt vmcnt` counts loads and stores in issue order).
// tools/micro/mix_rate.hip settles it: 4 scattered gathers + 6 coalesced stores per iteration cost 1011 cycles per CU when the
// wave waits for the gathers before it stores and 662 when it stores first -- the stores of one iteration and the gathers of
// the next then travel together instead of one after the other.
#ifndef CX_VR
#define CX_VR 4u          // rounds of 64 vertices whose loads are issued together
#endif
struct cx_fast_geom {
    uint32_t pstart, j0, k0;
};
__device__ __forceinline__ void cx_decode_entry(const cx_params& P, const cx_fast_geom& G, uint32_t e, uint32_t& i,
                                                uint32_t& j, uint32_t& k) {
    const uint32_t bit = (e >> 10) & 31u;
    const uint32_t r = (bit * 11u) >> 6;   // bit / 6 for bit < 32
    i = G.pstart + ((e >> 21) & 127u);
    j = G.j0 + r;
    k = G.k0 + 4u * ((e >> 15) & 63u) + (bit - 6u * r);
}
__device__ __forceinline__ uint32_t cx_entry_lin(const cx_params& P, const cx_fast_geom& G, uint32_t e) {
    uint32_t i, j, k;
    cx_decode_entry(P, G, e, i, j, k);
    return (i * P.n1 + j) * P.n2 + k;
}
__device__ __forceinline__ uint32_t cx_entry_signs(uint32_t e) {
    return (e & 3u) | ((e >> 4) & 0xCu) | ((e << 2) & 0x30u) | ((e >> 2) & 0xC0u);
}
// validity mask of the 8 corners of cell (i,j,k)
__device__ __forceinline__ uint32_t cx_corner_valid(const cx_params& P, uint32_t i, uint32_t j, uint32_t k) {
    const bool vi = (i + 1u < P.n0), vj = (j + 1u < P.n1), vk = (k + 1u < P.n2);
    uint32_t vm = 1u | (vk ? 2u : 0u) | (vj ? 4u : 0u) | ((vj && vk) ? 8u : 0u);
    vm |= vi ? (vm << 4) : 0u;
    return vm;
}

// vertex records, per-cell table entries and cell records of n queued cells, common case (no sample of
// the streaming wave's region within the tolerance screen, so the corner signs decide everything): table
// entries and cell records one lane per CELL, vertices one lane per VERTEX (two sample loads, one division,
// one coalesced 16-byte store) -- no divergent per-direction loop.
// Vertex records and triangles are not read again by the pipeline: nontemporal stores keep them from sitting dirty
// in L2 / Infinity Cache until the NEXT extraction's stream kernel has to push them out (measured: stream kernel
// 0.148 -> 0.129 ms inside the pipeline, whole extraction -5 %).  Table entries and cell records are read by the
// triangle kernel right away and stay ordinary stores.
typedef float cx_v4f __attribute__((ext_vector_type(4)));
typedef uint32_t cx_v2u __attribute__((ext_vector_type(2)));
#define CX_STORE_VERT(ptr, val) __builtin_nontemporal_store(cx_v2u{(val).x, (val).y}, reinterpret_cast<cx_v2u*>(ptr))
// one round of 64 queued cells, as the vertex stage carries it from its front half (decode, prefix
// sums, slot table, corner loads issued) to its back half (interpolation, stores)
struct cx_vround {
    uint32_t e, lin, sm, emask, ntri, vpre, tpre, vtot, ttot, ctot, real_voxel, vk;
    uint64_t recm;
    cx_run base;                       // first vertex / triangle / record of the round
    float f[8];                        // the 8 corner samples of the lane's cell
    uint32_t e_next;                   // entries of the following round
};
#define CX_CORNER_ROW 9u               // dwords per cell in the LDS corner table (8 + 1: bank spread)
// A narrow sample type (DT != CX_DTYPE_F32) leaves the front half with its raw bits in R.f: they are converted to fp32 in
// cx_vround_pin, after the loads are complete, so that the gathers stay in flight meanwhile.  A (k, k+1) pair may start at any
// sample: it is one packed 2 x sizeof(T) load aligned to one sample (cx_t2), whose instructions the compiler picks for that alignment.
template <int DT>
__device__ __forceinline__ void cx_vround_front(const cx_params& P, const cx_fast_geom& G, const uint32_t* q, uint32_t n, uint32_t b0,
                                                uint32_t lane, uint32_t e, const cx_run& base, uint32_t* slot,
                                                const uint8_t* ntri_lut, cx_vround& R) {
    const uint32_t idx = b0 + lane;
    const bool have = idx < n;
    R.e = e;
    R.e_next = (idx + 64u < n) ? q[idx + 64u] : 0u;
    uint32_t i, j, k;
    cx_decode_entry(P, G, e, i, j, k);
    R.lin = (i * P.n1 + j) * P.n2 + k;
    R.sm = cx_entry_signs(e);
    // The samples the round's vertices interpolate between, loaded per CELL: the (k, k+1) pairs of the 4 (i,j) rows of
    // the voxel = 4 loads per lane whose addresses follow the queue order (runs along k inside a few rows).  One lane per
    // VERTEX loading its own two samples, as this stage did first, touched 2.7 x the cache lines: the vector L1 takes
    // about one line per 3-4 cycles per CU, and that -- not bytes -- bounds these kernels.
    // The loaded pairs stay untouched until the back half (cx_vround_corners): any arithmetic on them here would make the
    // wave wait for the gathers right where it issues them (`s_waitcnt vmcnt` in front of the first use) instead of
    // interpolating the previous round's vertices meanwhile.
    uint32_t vm = cx_corner_valid(P, i, j, k);
    R.vk = (vm >> 1) & 1u;
    const uint32_t lin0 = have ? R.lin : 0u;
    const uint32_t oi = (have && (vm & 0x10u)) ? P.n1 * P.n2 : 0u, oj = (have && (vm & 4u)) ? P.n2 : 0u;
    // at the array edge in k read the pair (k-1, k) instead and repeat k (as cx_load_corners does)
    const uint32_t at = (R.vk || !have) ? lin0 : lin0 - 1u;
    typedef typename cx_dt<DT>::bits B;
    const B* __restrict__ A = reinterpret_cast<const B*>(cx_grid_data<DT>(P.grid));
    const cx_pair<DT> p0 = *reinterpret_cast<const cx_pair<DT>*>(A + at);
    const cx_pair<DT> p1 = *reinterpret_cast<const cx_pair<DT>*>(A + at + oj);
    const cx_pair<DT> p2 = *reinterpret_cast<const cx_pair<DT>*>(A + at + oi);
    const cx_pair<DT> p3 = *reinterpret_cast<const cx_pair<DT>*>(A + at + oi + oj);
    R.f[0] = cx_dt<DT>::raw(p0.x); R.f[1] = cx_dt<DT>::raw(p0.y); R.f[2] = cx_dt<DT>::raw(p1.x); R.f[3] = cx_dt<DT>::raw(p1.y);
    R.f[4] = cx_dt<DT>::raw(p2.x); R.f[5] = cx_dt<DT>::raw(p2.y); R.f[6] = cx_dt<DT>::raw(p3.x); R.f[7] = cx_dt<DT>::raw(p3.y);
    if (!have) { vm = 0; R.vk = 1u; }
    R.real_voxel = (have && vm == 0xFFu) ? 1u : 0u;
    const uint32_t s0 = (R.sm & 1u) ? 0xFFu : 0u;
    R.emask = have ? (((R.sm ^ s0) & vm) & 0xFEu) : 0u;
    R.ntri = R.real_voxel ? (uint32_t)ntri_lut[R.sm] : 0u;
    const uint32_t nv = __popc(R.emask);
    R.vpre = cx_wave_prefix_small<3>(nv, R.vtot);
    R.tpre = cx_wave_prefix_small<4>(R.ntri, R.ttot);
    R.recm = __ballot((nv | R.ntri) != 0u);
    R.ctot = (uint32_t)__popcll(R.recm);
    R.base = base;
    // vertex o of this round (o = vpre + rank of d in emask) -> (cell lane, direction d)
#pragma unroll
    for (uint32_t d = 1; d < 8; d++)
        if ((R.emask >> d) & 1u) slot[R.vpre + __popc(R.emask & ((1u << d) - 1u))] = (lane << 3) | d;
    __builtin_amdgcn_wave_barrier();
}
// the loads issued by the front half have to be complete here
template <int DT>
__device__ __forceinline__ void cx_vround_pin(cx_vround& R) {
#pragma unroll
    for (uint32_t c = 0; c < 8; c++) asm volatile("" : "+v"(R.f[c]) :: "memory");
    asm volatile("" : "+v"(R.e_next) :: "memory");
    if constexpr (DT != CX_DTYPE_F32) {
#pragma unroll
        for (uint32_t c = 0; c < 8; c++) R.f[c] = cx_dt<DT>::cvt(__float_as_uint(R.f[c]));
    }
}
__device__ __forceinline__ cx_vrec cx_vertex_record(const cx_params& P, const cx_fast_geom& G, uint32_t e2, uint32_t d, float f0, float f1) {
    const uint32_t lin2 = cx_entry_lin(P, G, e2);
    // same arithmetic as cx_emit_vertices; |f1 - f0| > 1e-8 here (cx_k_stream keeps waves with flatter crossings off this path)
    const float t = cx_fraction((P.vhi - f0) + P.vlo, f1 - f0);
    return make_uint2((lin2 << 3) | d, __float_as_uint(t));
}

// vertex records, (first vertex, crossing mask) words and cell records of n queued cells, common case (no sample of
// the streaming wave's region within the tolerance screen, or none that changes anything: the corner signs decide
// everything): words and cell records one lane per CELL, vertices one lane per VERTEX (its two samples from the round's
// corner table in LDS, one division, one coalesced 16-byte store) -- no divergent per-direction loop.  Rounds of 64 cells
// are software-pipelined: the corner loads of round s+1 are issued, and waited for, before the stores of round s go
// out (`s_waitcnt vmcnt` retires loads and stores in issue order: a load behind a store waits for it).
// LDS per wave: two slot tables of 448 words (double buffered) and the corner table of 64 x CX_CORNER_ROW words.
// `first`: the cell the walk starts at (a multiple of 64; `run` holds what precedes it), `n`: where it ends -- a wave takes a
// range of a batch's rounds (cx_k_emit_vertices)
template <int DT>
__device__ __forceinline__ void cx_emit_queue_fast(const cx_params& P, const cx_fast_geom& G, const uint32_t* q, uint32_t first, uint32_t n,
                                                   uint32_t lane, cx_run run, uint32_t* slot2, const uint8_t* ntri_lut, uint64_t* info) {
    float* corners = reinterpret_cast<float*>(slot2 + 2u * 448u);
    cx_vround Ra, Rb;
    uint32_t e0 = (first + lane < n) ? q[first + lane] : 0u;
    asm volatile("" : "+v"(e0) :: "memory");
    cx_vround_front<DT>(P, G, q, n, first, lane, e0, run, slot2, ntri_lut, Ra);
    cx_vround_pin<DT>(Ra);
    uint32_t par = 0;
    for (uint32_t b0 = first; b0 < n; b0 += 64u) {
        const bool more = b0 + 64u < n;   // wave-uniform
        if (more) {
            cx_run nb = Ra.base;
            nb.v += Ra.vtot; nb.t += Ra.ttot; nb.c += Ra.ctot;
            cx_vround_front<DT>(P, G, q, n, b0 + 64u, lane, Ra.e_next, nb, slot2 + (par ^ 1u) * 448u, ntri_lut, Rb);
        }
        // back half of round b0: the corner samples of the 64 cells go to LDS ...
#pragma unroll
        for (uint32_t c = 0; c < 8; c++) corners[lane * CX_CORNER_ROW + c] = ((c & 1u) || Ra.vk) ? Ra.f[c] : Ra.f[c + 1u];   // no k+1: the pair is (k-1, k)
        __builtin_amdgcn_wave_barrier();
        const bool vroom = Ra.base.v + Ra.vtot <= P.vcap;   // wave-uniform
        const uint32_t* slot = slot2 + par * 448u;
        // ... the first CX_VR x 64 vertices are interpolated before the next round's loads are waited for ...
        cx_vrec rec4[CX_VR];
#pragma unroll
        for (uint32_t r = 0; r < CX_VR; r++) {
            rec4[r] = make_uint2(0u, 0u);
            if (64u * r >= Ra.vtot) continue;   // wave-uniform
            const uint32_t o = 64u * r + lane;
            const uint32_t sl = slot[(o < Ra.vtot) ? o : 0u];
            const uint32_t cell = sl >> 3, d = sl & 7u;
            const uint32_t e2 = (uint32_t)__shfl((int)Ra.e, (int)cell);
            rec4[r] = cx_vertex_record(P, G, e2, d, corners[cell * CX_CORNER_ROW], corners[cell * CX_CORNER_ROW + d]);
        }
        // ... then the stores
        if (vroom) {
#pragma unroll
            for (uint32_t r = 0; r < CX_VR; r++) {
                const uint32_t o = 64u * r + lane;
                if (o < Ra.vtot && !P.records_only) CX_STORE_VERT(&P.verts[Ra.base.v + o], rec4[r]);
            }
            for (uint32_t o0 = 64u * CX_VR; o0 < Ra.vtot; o0 += 64u) {   // more than CX_VR x 64 vertices: the rest one round at a time
                const uint32_t o = o0 + lane;
                const uint32_t sl = slot[(o < Ra.vtot) ? o : 0u];
                const uint32_t cell = sl >> 3, d = sl & 7u;
                const uint32_t e2 = (uint32_t)__shfl((int)Ra.e, (int)cell);
                const cx_vrec r4 = cx_vertex_record(P, G, e2, d, corners[cell * CX_CORNER_ROW], corners[cell * CX_CORNER_ROW + d]);
                if (o < Ra.vtot && !P.records_only) CX_STORE_VERT(&P.verts[Ra.base.v + o], r4);
            }
            // (first vertex, crossing mask) of every queued cell, one 8-byte word per queue entry: 512 contiguous bytes per round
            // (was: scattered into a table of one entry per sample -- a cache line per cell, written and later gathered)
            if (b0 + lane < n && !P.records_only)
                info[b0 + lane] = cx_info_word(Ra.base.v + Ra.vpre, Ra.emask, Ra.ntri, Ra.real_voxel ? 0u : 0x3Fu);
        }
        if (P.write_records && (Ra.emask | Ra.ntri) != 0u && Ra.base.c + Ra.ctot <= P.ccap) {
            cx_store_cell_record(P, Ra.base.c + cx_mbcnt(Ra.recm), Ra.lin, Ra.sm | ((Ra.real_voxel ? 0u : 0x3Fu) << 8) | (Ra.ntri << 16) | (Ra.emask << 24),
                                 Ra.base.t + Ra.tpre, Ra.base.v + Ra.vpre);
        }
        __builtin_amdgcn_wave_barrier();
        if (more) cx_vround_pin<DT>(Rb);   // the next round's samples are waited for AFTER this round's stores went out (the note above CX_VR)
        if (more) Ra = Rb;
        par ^= 1u;
    }
}

// The same walk with the interpolation fractions READ from the stream kernel's stream (P.tq) instead of computed from gathered
// samples: vertex n of a streaming wave has its fraction at tq[w * wcap + n], so a round's fractions are one coalesced run.  What
// is left of the vertex stage is bookkeeping: the prefix sums of a round, the slot table that turns "vertex o of the round" into
// (cell, direction), the edge id, and the stores.  `tq_wave`: the wave's region minus its first vertex (indexed by GLOBAL vertex).
struct cx_tround {
    uint32_t e, lin, sm, emask, ntri, vpre, tpre, vtot, ttot, ctot, real_voxel;
    uint64_t recm;
    cx_run base;
    uint32_t tv[CX_VR];                // fractions of the round's first CX_VR x 64 vertices, as loaded
    uint32_t e_next;
};
__device__ __forceinline__ void cx_tround_front(const cx_params& P, const cx_fast_geom& G, const uint32_t* q, uint32_t n, uint32_t b0,
                                                uint32_t lane, uint32_t e, const cx_run& base, uint32_t* slot, const uint8_t* ntri_lut,
                                                const uint32_t* tq_wave, cx_tround& R) {
    const uint32_t idx = b0 + lane;
    const bool have = idx < n;
    R.e = e;
    R.e_next = (idx + 64u < n) ? q[idx + 64u] : 0u;
    uint32_t i, j, k;
    cx_decode_entry(P, G, e, i, j, k);
    R.lin = (i * P.n1 + j) * P.n2 + k;
    R.sm = cx_entry_signs(e);
    const uint32_t vm = have ? cx_corner_valid(P, i, j, k) : 0u;
    R.real_voxel = (have && vm == 0xFFu) ? 1u : 0u;
    const uint32_t s0 = (R.sm & 1u) ? 0xFFu : 0u;
    R.emask = have ? (((R.sm ^ s0) & vm) & 0xFEu) : 0u;
    R.ntri = R.real_voxel ? (uint32_t)ntri_lut[R.sm] : 0u;
    const uint32_t nv = __popc(R.emask);
    R.vpre = cx_wave_prefix_small<3>(nv, R.vtot);
    R.tpre = cx_wave_prefix_small<4>(R.ntri, R.ttot);
    R.recm = __ballot((nv | R.ntri) != 0u);
    R.ctot = (uint32_t)__popcll(R.recm);
    R.base = base;
    // the round's fractions: requested here, used in the back half (no arithmetic on them in between: a use would wait for them here)
#pragma unroll
    for (uint32_t r = 0; r < CX_VR; r++) {
        const uint32_t o = 64u * r + lane;
        R.tv[r] = 0u;
        if (o < R.vtot) R.tv[r] = __builtin_nontemporal_load(tq_wave + base.v + o);
    }
#pragma unroll
    for (uint32_t d = 1; d < 8; d++)
        if ((R.emask >> d) & 1u) slot[R.vpre + __popc(R.emask & ((1u << d) - 1u))] = (lane << 3) | d;
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ void cx_tround_pin(cx_tround& R) {
#pragma unroll
    for (uint32_t r = 0; r < CX_VR; r++) asm volatile("" : "+v"(R.tv[r]) :: "memory");
    asm volatile("" : "+v"(R.e_next) :: "memory");
}
__device__ __forceinline__ void cx_emit_queue_t(const cx_params& P, const cx_fast_geom& G, const uint32_t* q, uint32_t first, uint32_t n,
                                                uint32_t lane, cx_run run, uint32_t* slot2, const uint8_t* ntri_lut, uint64_t* info,
                                                const uint32_t* tq_wave) {
    cx_tround Ra, Rb;
    uint32_t e0 = (first + lane < n) ? q[first + lane] : 0u;
    asm volatile("" : "+v"(e0) :: "memory");
    cx_tround_front(P, G, q, n, first, lane, e0, run, slot2, ntri_lut, tq_wave, Ra);
    cx_tround_pin(Ra);
    uint32_t par = 0;
    for (uint32_t b0 = first; b0 < n; b0 += 64u) {
        const bool more = b0 + 64u < n;   // wave-uniform
        if (more) {
            cx_run nb = Ra.base;
            nb.v += Ra.vtot; nb.t += Ra.ttot; nb.c += Ra.ctot;
            cx_tround_front(P, G, q, n, b0 + 64u, lane, Ra.e_next, nb, slot2 + (par ^ 1u) * 448u, ntri_lut, tq_wave, Rb);
        }
        const bool vroom = Ra.base.v + Ra.vtot <= P.vcap;   // wave-uniform
        const uint32_t* slot = slot2 + par * 448u;
        if (vroom) {
#pragma unroll
            for (uint32_t r = 0; r < CX_VR; r++) {
                if (64u * r >= Ra.vtot) continue;   // wave-uniform
                const uint32_t o = 64u * r + lane;
                const uint32_t sl = slot[(o < Ra.vtot) ? o : 0u];
                const uint32_t cell = sl >> 3, d = sl & 7u;
                const uint32_t e2 = (uint32_t)__shfl((int)Ra.e, (int)cell);
                const cx_vrec rec = make_uint2((cx_entry_lin(P, G, e2) << 3) | d, Ra.tv[r]);
                if (o < Ra.vtot && !P.records_only) CX_STORE_VERT(&P.verts[Ra.base.v + o], rec);
            }
            for (uint32_t o0 = 64u * CX_VR; o0 < Ra.vtot; o0 += 64u) {   // more than CX_VR x 64 vertices: the rest one round at a time
                const uint32_t o = o0 + lane;
                const uint32_t sl = slot[(o < Ra.vtot) ? o : 0u];
                const uint32_t cell = sl >> 3, d = sl & 7u;
                const uint32_t e2 = (uint32_t)__shfl((int)Ra.e, (int)cell);
                const uint32_t tb = (o < Ra.vtot) ? tq_wave[Ra.base.v + o] : 0u;
                const cx_vrec rec = make_uint2((cx_entry_lin(P, G, e2) << 3) | d, tb);
                if (o < Ra.vtot && !P.records_only) CX_STORE_VERT(&P.verts[Ra.base.v + o], rec);
            }
            if (b0 + lane < n && !P.records_only)
                info[b0 + lane] = cx_info_word(Ra.base.v + Ra.vpre, Ra.emask, Ra.ntri, Ra.real_voxel ? 0u : 0x3Fu);
        }
        if (P.write_records && (Ra.emask | Ra.ntri) != 0u && Ra.base.c + Ra.ctot <= P.ccap) {
            cx_store_cell_record(P, Ra.base.c + cx_mbcnt(Ra.recm), Ra.lin, Ra.sm | ((Ra.real_voxel ? 0u : 0x3Fu) << 8) | (Ra.ntri << 16) | (Ra.emask << 24),
                                 Ra.base.t + Ra.tpre, Ra.base.v + Ra.vpre);
        }
        __builtin_amdgcn_wave_barrier();
        if (more) cx_tround_pin(Rb);   // the next round's fractions are waited for AFTER this round's stores went out
        if (more) Ra = Rb;
        par ^= 1u;
    }
}

// vertex / triangle / record / border counts of an active cell from its sign mask alone -- exact
// unless a corner is within the reference's np.allclose tolerances of the isovalue (then phase B
// recounts exactly).
struct cx_cnt {
    uint32_t v, t, c, b;
};
__device__ __forceinline__ void cx_count_from_signs(uint32_t sm, uint32_t vm, cx_cnt& acc) {
    const uint32_t s0 = (sm & 1u) ? 0xFFu : 0u;
    const uint32_t nv = __popc(((sm ^ s0) & vm) & 0xFEu);
    const bool real_voxel = (vm == 0xFFu);
    const uint32_t nt = real_voxel ? cx_voxel_ntri(sm) : 0u;
    acc.v += nv;
    acc.t += nt;
    acc.c += (nv | nt) ? 1u : 0u;
    acc.b += real_voxel ? 1u : 0u;
}

// inclusive prefix sum over the wave with DPP row shifts / broadcasts (no LDS crossbar round trips)
__device__ __forceinline__ uint32_t cx_wave_incl_scan(uint32_t x, uint32_t lane) {
    (void)lane;
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, false);   // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, false);   // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, false);   // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, false);   // row_shr:8
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false);   // row_bcast:15 -> rows 1, 3
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false);   // row_bcast:31 -> rows 2, 3
    return x;
}

// FAST phase A bit layout: one u32 per lane and sample plane, 6 bits per sample row r (0..RJ):
//   bit 6r+m (m=0..3) : sample (row r, k = k0 + 4*lane + m) < isovalue
//   bit 6r+4          : the same for k+1 of m=3 (next lane's m=0, the halo sample, or a clamped repeat)
#define CX_ROWBITS 6u
constexpr uint32_t cx_rowmask(int rows, uint32_t bits) {
    uint32_t m = 0;
    for (int r = 0; r < rows; r++) m |= bits << (6 * r);
    return m;
}
#define CX_M0_MASK cx_rowmask(CX_RJ + 1, 1u)    // bit 6r+0, r = 0..RJ
#define CX_CELL_MASK cx_rowmask(CX_RJ, 0xFu)    // bits 6r+0..3, r = 0..RJ-1  (the 4*RJ cells of a lane)

// which of the 4*RJ cells of streaming lane `lane` of the wave tile at (k0, j0) exist (mr), have a k+1 neighbour inside
// the array (mk) and a j+1 neighbour (mj); bit layout of CX_CELL_MASK.  Used by the stream kernel and by the fused emit
// kernel, which recomputes the stream kernel's vertex numbering for cells of OTHER waves: one definition for both.
struct cx_lmasks {
    uint32_t mr, mk, mj;
};
__device__ __forceinline__ cx_lmasks cx_lane_masks(const cx_params& P, uint32_t k0, uint32_t j0, uint32_t lane) {
    const uint32_t kofs = k0 + 4u * lane;
    const bool lane_valid = kofs < P.n2;
    const uint32_t nvalid = lane_valid ? min(4u, P.n2 - kofs) : 0u;   // samples of the row this lane holds
    const uint32_t nrows = (j0 < P.n1) ? min((uint32_t)CX_RJ, P.n1 - j0) : 0u;
    const uint32_t last_lane = min(63u, (P.n2 - k0 - 1u) >> 2);       // lane that holds the last sample of the segment
    const bool halo_in = (k0 + 256u) < P.n2;                          // a sample right of this segment exists
    cx_lmasks M;
    M.mr = (nrows >= CX_RJ) ? CX_CELL_MASK : (CX_CELL_MASK & ((1u << (CX_ROWBITS * nrows)) - 1u));   // rows that exist
    M.mr &= cx_rowmask(CX_RJ, 1u) * ((1u << nvalid) - 1u);            // cells that exist in this lane
    if (!lane_valid) M.mr = 0;                                        // lanes right of the array own no cells
    M.mk = M.mr;
    if (lane == last_lane && !halo_in) M.mk &= ~(CX_M0_MASK << (nvalid - 1u));   // the last sample of the row has no k+1
    M.mj = 0;
#pragma unroll
    for (uint32_t r = 0; r < CX_RJ; r++)
        if (j0 + r + 1u < P.n1) M.mj |= 0xFu << (CX_ROWBITS * r);
    M.mj &= M.mr;
    return M;
}
// crossing words of a lane: bit b of x[d] set <=> the cell at bit b owns a crossing on its edge in direction d.
// A, B = packed sign words of the cell plane and of the plane above; mi = M.mr if that plane exists, else 0.
__device__ __forceinline__ void cx_cross_words(uint32_t A, uint32_t B, const cx_lmasks& M, uint32_t mi, uint32_t x[8]) {
    x[0] = 0;
    x[1] = (A ^ (A >> 1)) & M.mk;
    x[2] = (A ^ (A >> CX_ROWBITS)) & M.mj;
    x[3] = (A ^ (A >> (CX_ROWBITS + 1u))) & M.mk & M.mj;
    x[4] = (A ^ B) & mi;
    x[5] = (A ^ (B >> 1)) & M.mk & mi;
    x[6] = (A ^ (B >> CX_ROWBITS)) & M.mj & mi;
    x[7] = (A ^ (B >> (CX_ROWBITS + 1u))) & M.mk & M.mj & mi;
}
