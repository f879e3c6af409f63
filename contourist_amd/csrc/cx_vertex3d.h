#pragma once
// cx_vertex3d.h -- stage S3 of the staged 3-D march: vertex records, one info word per queue entry and the cell records.
// Defines cx_k_emit_vertices (and cx_skip_rounds, for a wave whose share of rounds starts inside a batch).
// A section of the cx_march3d.hip translation unit: included only there, in this place, and not self-contained.  It relies on
// cx_emit3d.h (cx_fast_geom, cx_emit_queue_fast, cx_emit_queue_t, cx_process_queue) and on the batch list cx_stream3d.h leaves.

// what `rounds` full rounds of 64 queued cells at the front of a batch hold (vertices, triangles, records), from the queue
// entries alone -- the same formulas as cx_vround_front.  A wave that starts inside a batch (below) adds this to the batch's bases.
__device__ __forceinline__ void cx_skip_rounds(const cx_params& P, const cx_fast_geom& G, const uint32_t* q, uint32_t rounds, uint32_t lane,
                                               const uint8_t* ntri_lut, cx_run& run) {
    uint32_t v = 0, t = 0, c = 0;
    for (uint32_t r = 0; r < rounds; r++) {
        const uint32_t e = q[r * 64u + lane];
        uint32_t i, j, k;
        cx_decode_entry(P, G, e, i, j, k);
        const uint32_t vm = cx_corner_valid(P, i, j, k);
        const uint32_t sm = cx_entry_signs(e);
        const uint32_t s0 = (sm & 1u) ? 0xFFu : 0u;
        const uint32_t nv = __popc(((sm ^ s0) & vm) & 0xFEu);
        const uint32_t nt = (vm == 0xFFu) ? (uint32_t)ntri_lut[sm] : 0u;
        v += nv; t += nt; c += (nv | nt) ? 1u : 0u;
    }
    run.v += cxd_wave_add(v); run.t += cxd_wave_add(t); run.c += cxd_wave_add(c);
}

// ---- S3: vertex records, (first vertex, crossing mask) words and cell records.  The ROUNDS of 64 queued cells of all batches
// are divided evenly among the waves of the grid (wave m: rounds [m q, m q + q) of the flat batch list; the scan kernel left the
// batch each share starts in, P.rstart): batches hold 1 to 24 rounds, and with whole batches dealt out to waves -- as this
// kernel did first -- it lasted as long as its unluckiest wave (25 rounds against a mean of 7) while the chip stood half empty
// for the last third of its time.  A wave that starts inside a batch counts what the rounds before hold (cx_skip_rounds).
// A batch on the tolerance path (per-cell path, counts not derivable from the signs) goes as a whole to the wave in whose
// share its first round falls.
#ifndef CX_S3_MIN_WAVES
#define CX_S3_MIN_WAVES 1
#endif
template <bool TQ, int DT>     // TQ: the interpolation fractions come from the stream kernel's stream (P.tq); else the samples are gathered here
__global__ __launch_bounds__(256, CX_S3_MIN_WAVES) void cx_k_emit_vertices(const cx_params P, const cx_task T) {
    __shared__ float4 s_vstage[4][CX_VSTAGE_LDS];
    __shared__ uint8_t s_ntri[256];
    s_ntri[threadIdx.x] = cx_d_voxel_ntri[threadIdx.x];
    __syncthreads();
    const uint32_t lane = cx_lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nbatches = min(P.counters[CX_CNT_BATCHES], P.fcap);
    const uint32_t rounds = P.counters[CX_CNT_ROUNDS];
    const uint32_t nvw = gridDim.x * 4u;     // == P.nvw
    const uint32_t share = max((rounds + nvw - 1u) / nvw, CX_S3_MIN_SHARE);
    const uint32_t lo = (blockIdx.x * 4u + wave) * share;
    if (lo >= rounds || nbatches == 0u) return;
    const uint32_t hi = min(rounds, lo + share);
    uint32_t f = P.rstart[blockIdx.x * 4u + wave];
    if (f >= nbatches) return;
    cx_bdesc D = P.flat[f];
    for (;;) {   // waves are independent
        const uint32_t fn = f + 1u;
        cx_bdesc Dn = D;
        if (fn < nbatches) Dn = P.flat[fn];   // next descriptor in flight while this batch is processed
        const uint32_t nrb = (D.n + 63u) >> 6;
        const uint32_t r0 = max(lo, D.rbase) - D.rbase, r1 = min(hi, D.rbase + nrb) - D.rbase;   // this wave's rounds of the batch
        cx_fast_geom G;
        G.pstart = D.p; G.j0 = D.j0; G.k0 = D.k0;
        const uint32_t* __restrict__ q = P.queue + D.qofs;
        cx_run run;
        run.v = D.vbase; run.t = D.tbase; run.c = D.cbase; run.b = 0;
        uint64_t* __restrict__ info = P.info64 + D.qofs;
        if (!D.near) {
            if (r0) cx_skip_rounds(P, G, q, r0, lane, s_ntri, run);
            if (TQ)        // the fractions come from the stream kernel (the pointer is the wave's region minus its first vertex: indexed by GLOBAL vertex)
                cx_emit_queue_t(P, G, q, r0 * 64u, min(D.n, r1 * 64u), lane, run, reinterpret_cast<uint32_t*>(s_vstage[wave]), s_ntri, info,
                                reinterpret_cast<const uint32_t*>(P.tq) + ((size_t)D.w * T.wcap) - __builtin_amdgcn_readfirstlane(P.wbase[D.w].v));
            else
                cx_emit_queue_fast<DT>(P, G, q, r0 * 64u, min(D.n, r1 * 64u), lane, run, reinterpret_cast<uint32_t*>(s_vstage[wave]), s_ntri, info);
        } else if (r0 == 0u) {
            cx_process_queue<true, DT>(P, [&](uint32_t x) { return cx_entry_lin(P, G, q[x]); }, D.n, lane, true, run, reinterpret_cast<cx_vrec*>(s_vstage[wave]), info);
        }
        if (D.rbase + nrb >= hi || fn >= nbatches) break;
        f = fn;
        D = Dn;
    }
}
