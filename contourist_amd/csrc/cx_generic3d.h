#pragma once
// cx_generic3d.h -- the GENERIC CLASSIFY kernel of the 3-D march, for rows shorter than 4 samples or on request (CX_KERNEL_GENERIC).
// Defines cx_k_classify_generic; its triangles come from cx_k_emit_triangles (cx_tri3d.h).
// A section of the cx_march3d.hip translation unit: included only there, in this place, and not self-contained.  It relies on
// cx_emit3d.h (cx_process_queue, cx_run, CX_VSTAGE) and on CX_QCAP at the head of cx_march3d.hip.

// =================================================================================================
// generic classify kernel (any shape / alignment): one lane per cell, wave-private LDS queue, the
// workgroup reserves output space with ONE atomic per counter, then emits (per-cell path).
// =================================================================================================
#ifndef CX_GEN_MIN_WAVES
#define CX_GEN_MIN_WAVES 6   // what its LDS admits; on its own the allocator takes 87 registers and five waves
#endif
template <int DT>
__global__ __launch_bounds__(256, CX_GEN_MIN_WAVES) void cx_k_classify_generic(const cx_params P, const uint32_t cells_per_block) {
    __shared__ uint32_t s_queue[4][CX_QCAP];
    __shared__ cx_vrec s_vstage[4][CX_VSTAGE];
    __shared__ uint32_t s_tot[4][4];
    __shared__ uint32_t s_base[4];
    const uint32_t lane = cx_lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t* q = s_queue[wave];
    uint32_t qn = 0;   // wave-uniform
    cx_cnt acc = {0, 0, 0, 0};   // per-lane counts of the queued cells (from sign masks)
    float dnear = 3.0e38f;       // per-lane: smallest |f - vcmp| among the corners of the queued cells
    const uint32_t plane = P.n1 * P.n2;
    uint32_t gbase = blockIdx.x * cells_per_block + wave * 64u;
    const uint32_t gend = min(blockIdx.x * cells_per_block + cells_per_block, P.nsamples);
    bool streaming = gbase < gend;
    for (;;) {
        // ---- phase A: stream until done or until the queue might not hold another step
        while (streaming && qn + 64u <= CX_QCAP) {
            const uint32_t lin = gbase + lane;
            const bool in = lin < gend;
            const uint32_t linc = in ? lin : (P.nsamples - 1u);
            const uint32_t i = cx_div(linc, P.div_plane);
            const uint32_t r = linc - i * plane;
            const uint32_t j = cx_div(r, P.div_row);
            const uint32_t k = r - j * P.n2;
            float f[8];
            const uint32_t vm = cx_load_corners<DT>(P, linc, i, j, k, f);
            const uint32_t sm = cx_sign_mask(P, f);
            const uint32_t smv = sm & vm;
            const bool active = in && smv != 0u && smv != vm;
            const uint64_t act = __ballot(active);
            if (active) {
                q[qn + cx_mbcnt(act)] = lin;
                cx_count_from_signs(sm, vm, acc);
#pragma unroll
                for (int c = 0; c < 8; c++) dnear = fminf(dnear, fabsf(f[c] - P.vcmp));
            }
            qn += (uint32_t)__popcll(act);
            gbase += 256u;
            streaming = gbase < gend;
        }
        // ---- phase B: count, reserve, emit.  The last round of a workgroup reserves once for all
        // four waves; a wave whose queue filled up early reserves for itself (dense surfaces only).
        const bool final_round = !streaming;
        cx_run run = {0, 0, 0, 0};
        auto lin_of = [&](uint32_t x) { return q[x]; };
        if (__ballot(dnear <= P.near_abs) != 0ULL) {   // wave-uniform: a sample inside the tolerance screen, count exactly
            cx_process_queue<true, DT>(P, lin_of, qn, lane, false, run, s_vstage[wave]);
        } else {
            run.v = cxd_wave_add(acc.v); run.t = cxd_wave_add(acc.t);
            run.c = cxd_wave_add(acc.c); run.b = cxd_wave_add(acc.b);
        }
        acc.v = acc.t = acc.c = acc.b = 0;
        dnear = 3.0e38f;
        if (final_round) {
            if (lane == 0) {
                s_tot[wave][0] = run.v; s_tot[wave][1] = run.t; s_tot[wave][2] = run.c; s_tot[wave][3] = run.b;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                const uint32_t v = s_tot[0][0] + s_tot[1][0] + s_tot[2][0] + s_tot[3][0];
                const uint32_t t = s_tot[0][1] + s_tot[1][1] + s_tot[2][1] + s_tot[3][1];
                const uint32_t c = s_tot[0][2] + s_tot[1][2] + s_tot[2][2] + s_tot[3][2];
                const uint32_t bb = s_tot[0][3] + s_tot[1][3] + s_tot[2][3] + s_tot[3][3];
                s_base[0] = v ? atomicAdd(&P.counters[CX_CNT_VERTS], v) : 0u;
                s_base[1] = t ? atomicAdd(&P.counters[CX_CNT_TRIS], t) : 0u;
                s_base[2] = c ? atomicAdd(&P.counters[CX_CNT_CELLS], c) : 0u;
                if (bb) atomicAdd(&P.counters[CX_CNT_BORDER], bb);
            }
            __syncthreads();
            run.v = s_base[0]; run.t = s_base[1]; run.c = s_base[2];
            for (uint32_t w = 0; w < wave; w++) {
                run.v += s_tot[w][0]; run.t += s_tot[w][1]; run.c += s_tot[w][2];
            }
        } else {
            cx_run base = {0, 0, 0, 0};
            if (lane == 0) {
                if (run.v) base.v = atomicAdd(&P.counters[CX_CNT_VERTS], run.v);
                if (run.t) base.t = atomicAdd(&P.counters[CX_CNT_TRIS], run.t);
                if (run.c) base.c = atomicAdd(&P.counters[CX_CNT_CELLS], run.c);
                if (run.b) atomicAdd(&P.counters[CX_CNT_BORDER], run.b);
            }
            run.v = __builtin_amdgcn_readfirstlane(base.v);
            run.t = __builtin_amdgcn_readfirstlane(base.t);
            run.c = __builtin_amdgcn_readfirstlane(base.c);
        }
        cx_process_queue<true, DT>(P, lin_of, qn, lane, true, run, s_vstage[wave]);
        qn = 0;
        if (final_round) break;
    }
}
