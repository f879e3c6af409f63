#pragma once
// cx_fused3d.h -- the FUSED EMIT path of the 3-D march (on request): vertex records and triangles of a batch in one pass.
// Defines cx_k_cell_info, cx_k_hash_bytes and cx_k_emit_mesh.
// A section of the cx_march3d.hip translation unit: included only there, in this place, and not self-contained.  It relies on
// cx_emit3d.h (cx_fast_geom, the vertex rounds), cx_stream3d.h (the queues and P.qa) and cx_tri3d.h (cx_tri_lds, cx_tri_phase2,
// the hash rounds).

// =================================================================================================
// Fused emit: vertex records AND triangles of a batch in ONE pass over its queue entries.
//
// The staged kernels (cx_vertex3d.h, cx_tri3d.h) hand vertex indices from the vertex stage to the triangle stage through memory: a sparse
// 8-byte table entry per vertex-owning cell (scattered into a table of one entry per SAMPLE) plus a 16-byte record per
// active cell, and the triangle stage gathers up to six table entries per cell.  Here the hand-over is dense: a small
// kernel (cx_k_cell_info) writes ONE u32 per queue entry -- first vertex of the cell relative to its streaming wave and
// its crossing mask -- and the queue entry of ANY active lattice cell Y is found by arithmetic: the stream kernel left,
// per plane step and streaming lane, the queue position of the lane's first active cell and the 16-bit set of its active
// cells (P.qa), so position(Y) = qa >> 16 + popc(active cells below Y).  The six neighbour cells of a voxel that can own
// one of its edges live in the same lane word, the next lane, the next wave (rows) or the next task (planes):
// cx_nb_locate.  One wave per batch; rounds of 64 cells, software-pipelined like the vertex stage: everything round s+1
// loads is issued -- and waited for -- before the stores of round s go out.
// The CPython-order quad diagonals come from a byte per lattice point (cx_k_hash_bytes, built once per grid shape):
// the slot the point's tuple hash takes in an 8-slot set and the slot it moves to when that one is taken, which is all
// a two-element set's iteration order depends on.
// Only for extractions without a wave on the tolerance path (counters[CX_CNT_NEAR] == 0): there the reference's
// np.allclose rules drop vertices and triangles per cell (the host then runs the staged kernels instead).
// =================================================================================================
struct cx_geomx {          // wave-uniform: the streaming wave tile a batch belongs to
    uint32_t w, wave, nsteps;
};
// where cell X + c lives, X = (plane step ps, streaming lane ls, row r, sample m) of the tile:
// bits 0-5 lane, 6-9 cell in the lane (4r+m), 11 next k segment, 12 next row group, 13-19 plane step, 20 next plane chunk
__device__ __forceinline__ uint32_t cx_nb_locate(const cx_geomx& GX, uint32_t ps, uint32_t ls, uint32_t r, uint32_t m, uint32_t c) {
    uint32_t mY = m + (c & 1u), rY = r + ((c >> 1) & 1u), psY = ps + (c >> 2), laneY = ls;
    uint32_t kf = 0, jf = 0, pf = 0;
    if (mY == 4u) {
        mY = 0; laneY++;
        if (laneY == 64u) { laneY = 0; kf = 1; }
    }
    if (rY == (uint32_t)CX_RJ) { rY = 0; jf = 1; }
    if (psY == GX.nsteps) { psY = 0; pf = 1; }
    return laneY | ((4u * rY + mY) << 6) | (kf << 11) | (jf << 12) | (psY << 13) | (pf << 20);
}
// streaming wave that holds the cell of a location word
__device__ __forceinline__ uint32_t cx_nb_wave(const cx_geomx& GX, const cx_task& T, uint32_t loc) {
    uint32_t wY = GX.w;
    if ((loc >> 11) & 1u) wY += 4u;                                              // next block in k
    if ((loc >> 12) & 1u) wY += (GX.wave == 3u) ? (4u * T.nks - 3u) : 1u;        // next wave / next block in j
    if ((loc >> 20) & 1u) wY += 4u * T.nks * T.njg;                              // next chunk of planes
    return wY;
}

// ---- per queue entry: first vertex of the cell relative to its wave's first vertex (24 bits) | crossing mask >> 1 << 24
__global__ __launch_bounds__(256) void cx_k_cell_info(const cx_params P, const cx_task T) {
    if (P.counters[CX_CNT_NEAR] != 0u) return;
    const uint32_t nbatches = min(P.counters[CX_CNT_BATCHES], P.fcap);
    const uint32_t lane = cx_lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t stride = gridDim.x * 4u;
    for (uint32_t f = blockIdx.x * 4u + wave; f < nbatches; f += stride) {
        const cx_bdesc D = P.flat[f];
        const cx_tile tile = cx_tile_of(P, T, D.w >> 2, D.w & 3u);
        cx_fast_geom G;
        G.pstart = tile.p; G.j0 = tile.j0; G.k0 = tile.k0;
        const uint32_t* __restrict__ q = P.queue + D.qofs;
        uint32_t* __restrict__ info = P.info + D.qofs;
        uint32_t vrel = D.vbase - P.wbase[D.w].v;
        for (uint32_t b0 = 0; b0 < D.n; b0 += 64u) {
            const uint32_t idx = b0 + lane;
            const bool have = idx < D.n;
            const uint32_t e = have ? q[idx] : 0u;
            uint32_t i, j, k;
            cx_decode_entry(P, G, e, i, j, k);
            const uint32_t sm = cx_entry_signs(e);
            const uint32_t vm = cx_corner_valid(P, i, j, k);
            const uint32_t s0 = (sm & 1u) ? 0xFFu : 0u;
            const uint32_t emask = have ? (((sm ^ s0) & vm) & 0xFEu) : 0u;
            uint32_t vtot;
            const uint32_t vpre = cx_wave_prefix_small<3>(__popc(emask), vtot);
            if (have) info[idx] = (vrel + vpre) | (emask << 23);
            vrel += vtot;
        }
    }
}

// ---- CPython 3.10 set order of a lattice point, one byte: bits 0-2 = slot of hash((i,j,k)) in an 8-slot table, bits 3-5 =
// the first slot of its probe sequence that differs from it (what it takes when another element sits in its slot; the same
// slot again if 16 probes never leave it).  py_set2_swapped(h1, h2) == (t2 != s1 ? t2 < s1 : alt2 < s1) with s = slot(h1),
// t2 = slot(h2), alt2 = alternative of h2: the loop there stops at the first probe of h2 that differs from s1 == t2.
__global__ void cx_k_hash_bytes(uint8_t* __restrict__ table, const uint64_t* __restrict__ hash_xy, uint32_t nrows, uint32_t n2, int32_t org2) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t row = idx / n2;
    if (row >= nrows) return;
    const uint32_t k = idx - row * n2;
    const uint64_t h = py_finish3(py_round_signed(hash_xy[row], (int32_t)k + org2));
    const uint32_t s0 = (uint32_t)h & 7u;
    uint32_t s = s0;
    uint64_t perturb = h;
    for (int guard = 0; guard < 16 && s == s0; guard++) {
        perturb >>= 5;
        s = (uint32_t)((s * 5u + 1u + perturb) & 7u);
    }
    table[idx] = (uint8_t)(s0 | (s << 3));
}

struct cx_mesh_lds {
    cx_tri_lds tri;                // triangle stage tables (per wave) + the LUT
    uint32_t vslot[4][2][448];     // per wave, double buffered: vertex o of a round -> (cell lane << 3) | direction
    uint32_t vbt[4][8];            // per wave: wbase[].v of the 8 waves a neighbour cell can live in
    uint32_t qbt[4][8];            // per wave: first queue entry of those waves
    uint32_t qab[4][8];            // per wave: offset of their plane-step tables in P.qa
    uint8_t ntri[256];
};
// A round of 64 queued cells passes three stages, one per loop iteration of the wave:
//   stage 1 (round s+2)  decode, locate the neighbour cells, request the queue words of their lanes
//   stage 2 (round s+1)  queue words -> queue positions -> request the info words; prefix sums, vertex slot table, sample
//                        loads, set-order codes
//   stage 3 (round s)    interpolation, triangle expansion, stores
// Everything an iteration loads is waited for ONCE, after the arithmetic of stage 3 and before its stores (`s_waitcnt
// vmcnt` retires loads and stores in issue order, and the number of stores varies: a load waited for behind them would
// wait for all of them).
struct cx_mstage1 {
    uint32_t e, e_next;
    uint32_t nb[6];            // neighbour cells X + c, c = 1..6: (queue position of the lane's first cell << 16) | active cells below Y
    uint32_t nbw;              // 3 bits per neighbour: which of the 8 candidate waves; bit 18+c: neighbour c is wanted
};
struct cx_mround {
    uint32_t e, lin, sm, emask, ntri, vpre, tpre, vtot, ttot;
    uint32_t vbase, tbase;
    uint32_t e2[CX_VR], sl[CX_VR];
    float f0[CX_VR], f1[CX_VR];
    uint32_t nb[6];            // info words of the neighbour cells
    uint32_t nbw;
    uint32_t hb[4];            // set-order codes of the 8 corners, (k, k+1) pairs of the 4 (i,j) columns
};
__device__ __forceinline__ void cx_mesh_stage1(const cx_params& P, const cx_task& T, const cx_fast_geom& G, const cx_geomx& GX,
                                               const uint32_t* q, uint32_t n, uint32_t b0, uint32_t lane, uint32_t e,
                                               const uint8_t* ntri_lut, const uint32_t* qab, cx_mstage1& S) {
    const uint32_t idx = b0 + lane;
    const bool have = idx < n;
    S.e = e;
    S.e_next = (idx + 64u < n) ? q[idx + 64u] : 0u;
    uint32_t i, j, k;
    cx_decode_entry(P, G, e, i, j, k);
    const uint32_t sm = cx_entry_signs(e);
    const bool voxel = have && cx_corner_valid(P, i, j, k) == 0xFFu && ntri_lut[sm] != 0;   // emits triangles
    // the neighbour cells that own a crossing edge of this voxel: the queue word of their lane.  X + c sits in the same
    // lane word unless X is in the last sample column (m == 3: next lane, or lane 0 of the next k segment), the last row
    // (r == 3: next wave) or the last plane step (next task); `qab` holds the table offsets of the 8 waves that can be.
    const uint32_t ps = (e >> 21) & 127u, ls = (e >> 15) & 63u, bit = (e >> 10) & 31u;
    const uint32_t rr = (bit * 11u) >> 6, mm = bit - CX_ROWBITS * rr;
    const uint32_t m3 = (mm == 3u) ? 1u : 0u, r3 = (rr == (uint32_t)CX_RJ - 1u) ? 1u : 0u, pl = (ps + 1u == GX.nsteps) ? 1u : 0u;
    const uint32_t kfl = m3 & ((ls == 63u) ? 1u : 0u);
    const uint32_t lane_k[2] = {ls, m3 ? ((ls + 1u) & 63u) : ls};              // lane of X + dk
    const uint32_t cm[2] = {mm, (mm + 1u) & 3u};                               // sample column of X + dk
    const uint32_t cr[2] = {4u * rr, 4u * ((rr + 1u) & 3u)};                   // 4 * row of X + dj
    const uint32_t pofs[2] = {ps << 6, pl ? 0u : ((ps + 1u) << 6)};            // plane step of X + di, times 64
    S.nbw = 0;
#pragma unroll
    for (uint32_t c = 1; c < 7; c++) {
        const uint32_t dk = c & 1u, dj = (c >> 1) & 1u, di = c >> 2;
        const uint32_t sc = ((sm >> c) & 1u) ? 0xFFu : 0u;
        uint32_t sup = 0;   // corners that are strict supersets of c: the far ends of the voxel edges corner c owns
#pragma unroll
        for (uint32_t c2 = 0; c2 < 8; c2++) sup |= ((c2 & c) == c && c2 != c) ? (1u << c2) : 0u;
        S.nb[c - 1u] = 0;
        if (voxel && ((sm ^ sc) & sup) != 0u) {
            const uint32_t wsel = (dk ? kfl : 0u) | ((dj ? r3 : 0u) << 1) | ((di ? pl : 0u) << 2);
            const uint32_t qa = P.qa[qab[wsel] + pofs[di] + lane_k[dk]];
            // low 16 bits: the active cells below Y in its lane (their count completes the queue position)
            S.nb[c - 1u] = (qa & 0xFFFF0000u) | (qa & ((1u << (cr[dj] + cm[dk])) - 1u));
            S.nbw |= (wsel << (3u * (c - 1u))) | (1u << (18u + c));
        }
    }
}
__device__ __forceinline__ void cx_mesh_pin1(cx_mstage1& S) {
#pragma unroll
    for (uint32_t c = 0; c < 6; c++) asm volatile("" : "+v"(S.nb[c]) :: "memory");
    asm volatile("" : "+v"(S.e_next) :: "memory");
}
__device__ __forceinline__ void cx_mesh_stage2(const cx_params& P, const cx_task& T, const cx_fast_geom& G, const cx_mstage1& S,
                                               uint32_t n, uint32_t b0, uint32_t lane, uint32_t vbase, uint32_t tbase, uint32_t* slot,
                                               const uint8_t* ntri_lut, const uint32_t* qbt, cx_mround& R) {
    const float* __restrict__ A = cx_grid_data<CX_DTYPE_F32>(P.grid);   // fp32 grids only: enqueue_extract sends typed ones through the staged kernels
    const uint32_t plane = P.n1 * P.n2;
    const uint32_t idx = b0 + lane;
    const bool have = idx < n;
    const uint32_t e = S.e;
    R.e = e;
    // the queue words are back: queue positions of the neighbour cells -> their info words
    R.nbw = S.nbw;
#pragma unroll
    for (uint32_t c = 0; c < 6; c++) {
        const uint32_t w = S.nb[c];
        uint32_t infow = 0;
        if ((S.nbw >> (19u + c)) & 1u) infow = P.info[qbt[(S.nbw >> (3u * c)) & 7u] + (w >> 16) + __popc(w & 0xFFFFu)];
        R.nb[c] = infow;
    }
    uint32_t i, j, k;
    cx_decode_entry(P, G, e, i, j, k);
    R.lin = (i * P.n1 + j) * P.n2 + k;
    R.sm = cx_entry_signs(e);
    const uint32_t vm = cx_corner_valid(P, i, j, k);
    const bool real_voxel = have && vm == 0xFFu;
    const uint32_t s0 = (R.sm & 1u) ? 0xFFu : 0u;
    R.emask = have ? (((R.sm ^ s0) & vm) & 0xFEu) : 0u;
    R.ntri = real_voxel ? (uint32_t)ntri_lut[R.sm] : 0u;
    const uint32_t nv = __popc(R.emask);
    R.vpre = cx_wave_prefix_small<3>(nv, R.vtot);
    R.tpre = cx_wave_prefix_small<4>(R.ntri, R.ttot);
    R.vbase = vbase; R.tbase = tbase;
#pragma unroll
    for (uint32_t d = 1; d < 8; d++)
        if ((R.emask >> d) & 1u) slot[R.vpre + __popc(R.emask & ((1u << d) - 1u))] = (lane << 3) | d;
    __builtin_amdgcn_wave_barrier();
    // sample loads of the first CX_VR x 64 vertices
#pragma unroll
    for (uint32_t r = 0; r < CX_VR; r++) {
        R.sl[r] = 0; R.e2[r] = 0; R.f0[r] = 0.0f; R.f1[r] = 1.0f;
        if (64u * r >= R.vtot) continue;   // wave-uniform
        const uint32_t o = 64u * r + lane;
        R.sl[r] = slot[(o < R.vtot) ? o : 0u];
        R.e2[r] = (uint32_t)__shfl((int)e, (int)(R.sl[r] >> 3));
        const uint32_t d = R.sl[r] & 7u;
        const uint32_t lin2 = cx_entry_lin(P, G, R.e2[r]);
        R.f0[r] = A[lin2];
        R.f1[r] = A[lin2 + ((d & 4u) ? plane : 0u) + ((d & 2u) ? P.n2 : 0u) + (d & 1u)];
    }
    // CPython-order quad diagonals: the codes of the 8 corners, one 2-byte load per (i,j) column
    R.hb[0] = R.hb[1] = R.hb[2] = R.hb[3] = 0;
    if (P.hbytes && cx_need_hash(R.sm, 0u, R.ntri) != 0u) {   // only voxels: all 8 corners are inside the array
        const uint8_t* __restrict__ hb = P.hbytes + R.lin;
        uint16_t t0, t1, t2, t3;
        __builtin_memcpy(&t0, hb, 2); __builtin_memcpy(&t1, hb + P.n2, 2);
        __builtin_memcpy(&t2, hb + plane, 2); __builtin_memcpy(&t3, hb + plane + P.n2, 2);
        R.hb[0] = t0; R.hb[1] = t1; R.hb[2] = t2; R.hb[3] = t3;
    }
}
__device__ __forceinline__ void cx_mesh_pin2(cx_mround& R) {
#pragma unroll
    for (uint32_t r = 0; r < CX_VR; r++) asm volatile("" : "+v"(R.f0[r]), "+v"(R.f1[r]) :: "memory");
#pragma unroll
    for (uint32_t c = 0; c < 6; c++) asm volatile("" : "+v"(R.nb[c]) :: "memory");
    asm volatile("" : "+v"(R.hb[0]), "+v"(R.hb[1]), "+v"(R.hb[2]), "+v"(R.hb[3]) :: "memory");
}

// phase 1 of the triangle stage for the fused kernel: like cx_tri_phase1, with the quad diagonals from the corner codes
__device__ __forceinline__ uint32_t cx_mesh_phase1(const cx_params& P, cx_tri_lds& L, uint32_t lane, uint32_t wave, const cx_mround& R,
                                                   const uint32_t* vbt) {
    const uint32_t sm = R.sm, ntri = R.ntri;
    L.ve[wave][0][lane] = make_uint2(R.vbase + R.vpre, R.emask);
#pragma unroll
    for (uint32_t c = 1; c < 7; c++) {
        const uint32_t w = R.nb[c - 1u];
        const bool want = (R.nbw >> (18u + c)) & 1u;
        L.ve[wave][c][lane] = want ? make_uint2(vbt[(R.nbw >> (3u * (c - 1u))) & 7u] + (w & 0xFFFFFFu), (w >> 23) & 0xFEu) : make_uint2(0u, 0u);
    }
    uint32_t variants = 0;
    if (P.hbytes) {
        // code of corner c = byte (c & 1) of column c >> 1
#pragma unroll
        for (int t = 0; t < 6; t++) {
            const uint32_t pat = ((sm >> CX_TC[t][0]) & 1u) | (((sm >> CX_TC[t][1]) & 1u) << 1) |
                                 (((sm >> CX_TC[t][2]) & 1u) << 2) | (((sm >> CX_TC[t][3]) & 1u) << 3);
            if (__popc(pat) != 2) continue;
            uint32_t l0 = 0, l1 = 0, h0 = 0, h1 = 0;
            int nl = 0, nh = 0;
#pragma unroll
            for (int m = 0; m < 4; m++) {
                const uint32_t cc = CX_TC[t][m];
                const uint32_t code = (R.hb[cc >> 1] >> (8u * (cc & 1u))) & 0xFFu;
                if ((pat >> m) & 1u) { if (nl == 0) l0 = code; else l1 = code; nl++; }
                else { if (nh == 0) h0 = code; else h1 = code; nh++; }
            }
            if (cx_set2_swapped(l0, l1) != cx_set2_swapped(h0, h1)) variants |= 1u << t;
        }
    }
    L.u[wave].a.tfirst[lane] = R.tbase;   // triangle j of the round goes to tbase + j
    uint32_t pos = R.tpre;
#pragma unroll
    for (int t = 0; t < 6; t++) {
        const uint32_t pat = ((sm >> CX_TC[t][0]) & 1u) | (((sm >> CX_TC[t][1]) & 1u) << 1) |
                             (((sm >> CX_TC[t][2]) & 1u) << 2) | (((sm >> CX_TC[t][3]) & 1u) << 3);
        const uint32_t np = __popc(pat);
        const uint32_t nt = (ntri == 0u) ? 0u : ((np == 2u) ? 2u : (np & 1u));
        const uint32_t word = lane | (((uint32_t)t * 32u + pat * 2u + ((variants >> t) & 1u)) << 7);
        if (nt >= 1u) L.u[wave].a.slot[pos] = (uint16_t)word;
        if (nt == 2u) L.u[wave].a.slot[pos + 1u] = (uint16_t)(word | (1u << 6));
        pos += nt;
    }
    __builtin_amdgcn_wave_barrier();
    return R.ttot;
}

#ifndef CX_EM_MIN_WAVES
#define CX_EM_MIN_WAVES 1
#endif
__global__ __launch_bounds__(256, CX_EM_MIN_WAVES) void cx_k_emit_mesh(const cx_params P, const cx_task T) {
    __shared__ cx_mesh_lds L;
    if (P.counters[CX_CNT_NEAR] != 0u) return;   // a wave on the tolerance path: the host runs the staged kernels instead
    if (P.counters[CX_CNT_TRIS] > P.tcap || P.counters[CX_CNT_VERTS] > P.vcap) return;   // host re-runs with more room
    const uint32_t nbatches = min(P.counters[CX_CNT_BATCHES], P.fcap);
    if (blockIdx.x * 4u >= nbatches) return;
    cx_tri_lds_init(L.tri);
    L.ntri[threadIdx.x] = cx_d_voxel_ntri[threadIdx.x];
    __syncthreads();
    const float* __restrict__ A = cx_grid_data<CX_DTYPE_F32>(P.grid);   // fp32 grids only (as cx_mesh_stage2)
    const uint32_t plane = P.n1 * P.n2;
    const uint32_t lane = cx_lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nw = T.nblocks * 4u;
    const uint32_t stride = gridDim.x * 4u;
    uint32_t f = blockIdx.x * 4u + wave;
    if (f >= nbatches) return;
    cx_bdesc D = P.flat[f];
    for (;;) {   // waves are independent
        const uint32_t fn = f + stride;
        cx_bdesc Dn = D;
        if (fn < nbatches) Dn = P.flat[fn];   // next descriptor in flight while this batch is processed
        const cx_tile tile = cx_tile_of(P, T, D.w >> 2, D.w & 3u);
        cx_fast_geom G;
        G.pstart = tile.p; G.j0 = tile.j0; G.k0 = tile.k0;
        cx_geomx GX;
        GX.w = D.w; GX.wave = D.w & 3u; GX.nsteps = tile.ib - tile.p;
        // first vertex and first queue entry of the 8 streaming waves a neighbour cell can live in
        // (index: next k | next j << 1 | next chunk << 2)
        if (lane < 8u) {
            const uint32_t wY = min(cx_nb_wave(GX, T, ((lane & 1u) << 11) | (((lane >> 1) & 1u) << 12) | (((lane >> 2) & 1u) << 20)), nw - 1u);
            L.vbt[wave][lane] = P.wbase[wY].v;
            L.qbt[wave][lane] = wY * T.wcap;
            L.qab[wave][lane] = wY * (CX_SWP * 64u);
        }
        __builtin_amdgcn_wave_barrier();
        const uint32_t* __restrict__ q = P.queue + D.qofs;
        const uint32_t n = D.n;
        cx_mstage1 Sb, Sc;
        cx_mround Ra, Rb;
        uint32_t e0 = (lane < n) ? q[lane] : 0u;
        asm volatile("" : "+v"(e0) :: "memory");
        cx_mesh_stage1(P, T, G, GX, q, n, 0u, lane, e0, L.ntri, L.qab[wave], Sb);
        cx_mesh_pin1(Sb);
        cx_mesh_stage2(P, T, G, Sb, n, 0u, lane, D.vbase, D.tbase, L.vslot[wave][0], L.ntri, L.qbt[wave], Ra);
        if (64u < n) cx_mesh_stage1(P, T, G, GX, q, n, 64u, lane, Sb.e_next, L.ntri, L.qab[wave], Sc);
        cx_mesh_pin2(Ra);
        if (64u < n) { cx_mesh_pin1(Sc); Sb = Sc; }
        uint32_t par = 0;
        for (uint32_t b0 = 0; b0 < n; b0 += 64u) {
            const bool more1 = b0 + 64u < n, more2 = b0 + 128u < n;   // wave-uniform
            if (more2) cx_mesh_stage1(P, T, G, GX, q, n, b0 + 128u, lane, Sb.e_next, L.ntri, L.qab[wave], Sc);
            if (more1) cx_mesh_stage2(P, T, G, Sb, n, b0 + 64u, lane, Ra.vbase + Ra.vtot, Ra.tbase + Ra.ttot, L.vslot[wave][par ^ 1u],
                                      L.ntri, L.qbt[wave], Rb);
            // ---- stage 3 of round b0: what needs no store
            cx_vrec rec4[CX_VR];
#pragma unroll
            for (uint32_t r = 0; r < CX_VR; r++) rec4[r] = cx_vertex_record(P, G, Ra.e2[r], Ra.sl[r] & 7u, Ra.f0[r], Ra.f1[r]);
            const uint32_t ttot = cx_mesh_phase1(P, L.tri, lane, wave, Ra, L.vbt[wave]);
            if (more2) cx_mesh_pin1(Sc);
            if (more1) cx_mesh_pin2(Rb);
            // ---- the stores
            {
#pragma unroll
                for (uint32_t r = 0; r < CX_VR; r++) {
                    const uint32_t o = 64u * r + lane;
                    if (o < Ra.vtot) CX_STORE_VERT(&P.verts[Ra.vbase + o], rec4[r]);
                }
                const uint32_t* slot = L.vslot[wave][par];
                for (uint32_t o0 = 64u * CX_VR; o0 < Ra.vtot; o0 += 64u) {   // more than CX_VR x 64 vertices: the rest one round at a time
                    const uint32_t o = o0 + lane;
                    const uint32_t sl = slot[(o < Ra.vtot) ? o : 0u];
                    const uint32_t e2 = (uint32_t)__shfl((int)Ra.e, (int)(sl >> 3));
                    const uint32_t d = sl & 7u;
                    const uint32_t lin2 = cx_entry_lin(P, G, e2);
                    const float f0 = A[lin2];
                    const float f1 = A[lin2 + ((d & 4u) ? plane : 0u) + ((d & 2u) ? P.n2 : 0u) + (d & 1u)];
                    const cx_vrec r4 = cx_vertex_record(P, G, e2, d, f0, f1);
                    if (o < Ra.vtot) CX_STORE_VERT(&P.verts[Ra.vbase + o], r4);
                }
            }
            cx_tri_phase2(P, L.tri, lane, wave, ttot);
            __builtin_amdgcn_wave_barrier();
            if (more1) Ra = Rb;
            if (more2) Sb = Sc;
            par ^= 1u;
        }
        if (fn >= nbatches) break;
        f = fn;
        D = Dn;
    }
}
