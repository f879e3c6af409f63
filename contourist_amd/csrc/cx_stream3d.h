#pragma once
// cx_stream3d.h -- stages S1 and S2 of the staged 3-D march: the one pass over the samples and the scan of what it queued.
// Defines cx_k_stream, its multi-level twin cx_k_stream_levels (both run cx_stream_tile), cx_k_scan_list and
// cx_k_scan_list_levels (both run cx_scan_list_chunk); also cx_task_of_block and cx_tile, which the later stages use.
// A section of the cx_march3d.hip translation unit: included only there, in this place, and not self-contained.  It relies on
// cx_emit3d.h (cx_cnt, the row masks, cx_lane_masks, cx_wave_incl_scan, cx_v2u) and on CX_RJ, CX_K1_MIN_WAVES and CX_BATCH_MIN at the
// head of cx_march3d.hip.

// =================================================================================================
// staged pipeline:  S1 stream -> S2 scan -> S3 vertices -> S4 triangles
// Every streaming wave owns a queue region in global memory (one u32 per cell of its task, written
// densely from the front) and a list of batch records; nothing waits for anything inside a kernel.
// =================================================================================================
// logical task of a workgroup: the hardware deals workgroups round-robin to the 8 XCDs, each with
// its own L2; give every XCD one contiguous range of tasks so that neighbours (which share halo
// rows and planes) run on the same XCD at about the same time.
__device__ __forceinline__ uint32_t cx_task_of_block(const cx_task& T) {
    return (blockIdx.x & 7u) * T.chunk + (blockIdx.x >> 3);
}
struct cx_tile {     // what a wave covers: planes [p, ib), rows j0.., samples k0 + 4*lane..
    uint32_t k0, j0, p, ib, nrows;
};
__device__ __forceinline__ cx_tile cx_tile_of(const cx_params& P, const cx_task& T, uint32_t b, uint32_t wave) {
    cx_tile t;
    const uint32_t ks = b % T.nks; b /= T.nks;
    const uint32_t jg = b % T.njg;
    const uint32_t ic = b / T.njg;
    t.k0 = ks * 256u;
    t.j0 = jg * (4u * CX_RJ) + wave * CX_RJ;
    t.p = ic * T.ci;
    t.ib = min(t.p + T.ci, P.n0);
    t.nrows = (t.j0 < P.n1) ? min((uint32_t)CX_RJ, P.n1 - t.j0) : 0u;
    return t;
}

// ---- S1: one pass over the samples.  Lanes hold 4 consecutive k-samples of RJ+1 rows (one 16-byte
// load per row and plane, two planes in flight); the 20 sign bits of a plane go into ONE u32 per lane,
// a cell's activity and the per-lane vertex / triangle / record counts come from bitwise ops on two
// such words for 16 cells at a time.
// Queue entries and batch records are staged in LDS and copied out in bulk: `s_waitcnt vmcnt` retires
// loads, stores and atomics in issue order, so a store issued between two plane loads would make the
// second wait for the store's round trip (measured: +45 % kernel time with one store per active step).
#define CX_SQ 512u      // queue entries a wave stages; a step adds at most 1024: more than CX_SQ go in two halves of the lanes (32 lanes hold at most 512 cells)
#define CX_PLW 260u     // floats per row of a staged sample plane: 256 samples of the segment + the one right of it (+ 3: bank spread)
#define CX_SBR 32u      // batch records a wave stages: all a wave can close (at most one per CX_BATCH_MIN cells of its (CX_SWP - 1) x 1024)
static_assert((CX_SWP - 1u) * 1024u / CX_BATCH_MIN + 1u <= CX_SBR, "a streaming wave can close more batches than its LDS stage holds");
static_assert(CX_SQ >= 512u, "half a wave's lanes queue up to 512 cells per step");
// ALIGNED: n2 % 4 == 0 and a 16-byte aligned grid (rows start on 16-byte boundaries, every lane holds 4 samples
// of one row).  Otherwise the 16-byte loads are only 4-byte aligned and the lane that holds the end of a row
// loads the row's last 4 samples and shifts them into place, repeating the last one (a clamped corner).
// DT: the sample type.  A narrow type keeps the same lane layout: a lane loads its 4 samples as ONE 4 x sizeof(T) load (aligned to
// 4 x sizeof(T) when ALIGNED, else to one sample: cx_row4) and the halo sample as its raw bits; they are converted to fp32 where the
// fp32 kernel reads them (plane_bits), so that the planes requested ahead stay in flight.  Everything after that is the fp32 code.
template <int DT> struct cx_row4 { typedef float4 v; typedef float h; };   // DT == CX_DTYPE_F32: the loads as they were
template <> struct cx_row4<CX_DTYPE_U8> { typedef uint32_t v; typedef uint32_t h; };
template <> struct cx_row4<CX_DTYPE_I8> { typedef uint32_t v; typedef uint32_t h; };
template <> struct cx_row4<CX_DTYPE_U16> { typedef cx_v2u v; typedef uint32_t h; };
template <> struct cx_row4<CX_DTYPE_I16> { typedef cx_v2u v; typedef uint32_t h; };
template <> struct cx_row4<CX_DTYPE_F16> { typedef cx_v2u v; typedef uint32_t h; };
template <> struct cx_row4<CX_DTYPE_BF16> { typedef cx_v2u v; typedef uint32_t h; };
template <typename V, size_t AL>
struct __attribute__((packed, aligned(AL))) cx_row4_ua { V v; };
template <int DT>
__device__ __forceinline__ void cx_row4_unpack(const typename cx_row4<DT>::v& w, float& x, float& y, float& z, float& t) {
    if constexpr (sizeof(typename cx_dt<DT>::T) == 1) {
        x = cx_dt<DT>::cvt(w); y = cx_dt<DT>::cvt(w >> 8); z = cx_dt<DT>::cvt(w >> 16); t = cx_dt<DT>::cvt(w >> 24);
    } else {
        x = cx_dt<DT>::cvt(w.x); y = cx_dt<DT>::cvt(w.x >> 16); z = cx_dt<DT>::cvt(w.y); t = cx_dt<DT>::cvt(w.y >> 16);
    }
}
template <bool ALIGNED, int DT>
__device__ __forceinline__ void cx_stream_tile(const cx_params& P, const cx_task& T, const uint32_t b) {
    __shared__ uint32_t s_q[4][CX_SQ];
    __shared__ uint32_t s_br[4][CX_SBR][5];
    // the two sample planes a step's cells lie between, per wave, row by row as the array has them ([CX_RJ + 1 rows][256 samples + the
    // one to the right]): what lets ONE LANE PER QUEUED CELL read its 8 corners, wherever the cell's streaming lane holds them in
    // registers -- the interpolation fractions of the crossings are computed HERE, where the samples already are, instead of being
    // gathered again from HBM by the vertex stage (round 4: those gathers pulled 274 MB of 128-byte lines per 512^3 extraction,
    // half of the grid, for 100 MB of vertex records)
    // (dynamic LDS: 41.6 KB per workgroup, asked for at launch only when the extraction hands fractions on -- without it the stream
    // kernel keeps its 11 KB and leaves the LDS of its CU to the other extraction's emit stages)
    extern __shared__ __attribute__((aligned(16))) float s_pl_dyn[];
    __shared__ uint32_t s_tot[4][8];
    __shared__ uint8_t s_ntri[256];      // triangles of a voxel by its corner sign mask
    if (b >= T.nblocks) return;
    s_ntri[threadIdx.x] = cx_d_voxel_ntri[threadIdx.x];
    if (b == 0u && threadIdx.x < 3u && P.torder) P.counters[CX_CNT_TCLS + threadIdx.x] = 0u;   // the scan kernel counts the tile kernel's work classes into these
    __syncthreads();
    const uint32_t lane = cx_lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t* q = s_q[wave];
    uint32_t ql = 0, qflushed = 0;      // wave-uniform: entries staged / already in global memory
    uint32_t nbl = 0, nbflushed = 0;    // the same for batch records
    const uint32_t w = b * 4u + wave;
    unsigned long long* stamp = P.stamps ? P.stamps + (size_t)w * 4u : nullptr;
    if (stamp && lane == 0) stamp[0] = __builtin_amdgcn_s_memtime();
    const cx_tile tile = cx_tile_of(P, T, b, wave);
    const uint32_t k0 = tile.k0, j0 = tile.j0, ib = tile.ib, nrows = tile.nrows;
    uint32_t p = tile.p;
    uint32_t* __restrict__ gq = P.queue + (size_t)w * T.wcap;
    cx_brec* __restrict__ brec = P.brec + (size_t)w * T.bcap;
    const typename cx_dt<DT>::bits* __restrict__ A = reinterpret_cast<const typename cx_dt<DT>::bits*>(cx_grid_data<DT>(P.grid));
    cx_cnt acc = {0, 0, 0, 0};   // per-lane counts of the cells queued since the last batch record (b: all)
    uint32_t qn = 0, qstart = 0, nb = 0;   // wave-uniform: queued cells, start of the open batch, closed batches
    uint32_t rv = 0, rt = 0, rc = 0;       // wave-uniform: vertices / triangles / records of the closed batches
    uint32_t nr = 0;                       // wave-uniform: rounds of 64 cells of the closed batches
    uint32_t tv = 0;                       // wave-uniform: fractions written to the wave's stream so far (== vertices of its cells)
    bool overflow_t = false;               // wave-uniform: the stream of fractions ran out of room
    float dnear = 3.0e38f;       // per-lane: smallest |f - vcmp| among the samples seen (tolerance screen)
    cx_fast_geom G;
    G.pstart = p; G.j0 = j0; G.k0 = k0;
    // P.qlimit: entries this wave's region holds.  A single extraction gives every wave room for all its cells (T.wcap); the levels of
    // cx_extract3d_levels share ONE pool, each with a slice of every wave's region -- a wave that finds more cells than its slice
    // holds stops storing them and raises the overflow flag (chunk slot 7): the host then gives that call full-size regions.
    bool overflow = false;
    // The counts of the queued cells (vertices, triangles, records, border voxels: what the batch records and the scan need) are only
    // ever used as sums over a batch, so they need not be taken step by step -- with ~30 cells per step half of the lanes of a
    // counting round stood idle.  Staged entries are counted in FULL rounds of 64 right before they leave the stage or a batch is
    // closed (the fraction stream P.tq works step by step and keeps the old form: one counting round per plane step).
    uint32_t qc = 0;                 // wave-uniform: staged entries already counted
    // all eight corners of every cell of this wave's tile inside the array: the validity mask is 0xFF (wave-uniform)
    const bool interior = (tile.ib < P.n0) && (j0 + (uint32_t)CX_RJ < P.n1) && (k0 + 256u < P.n2);
    auto count_pending = [&]() {
        __builtin_amdgcn_wave_barrier();
        for (uint32_t o0 = qc; o0 < ql; o0 += 64u) {       // wave-uniform
            const uint32_t o = o0 + lane;
            const bool have = o < ql;
            const uint32_t e = have ? q[o] : 0u;
            uint32_t vm = have ? 0xFFu : 0u;
            if (!interior) {
                uint32_t ci, cj, ck;
                cx_decode_entry(P, G, e, ci, cj, ck);
                vm = have ? cx_corner_valid(P, ci, cj, ck) : 0u;
            }
            const uint32_t sm = cx_entry_signs(e);
            const uint32_t s0 = (sm & 1u) ? 0xFFu : 0u;
            const uint32_t nv = __popc(((sm ^ s0) & vm) & 0xFEu);
            const bool real = (vm == 0xFFu);
            const uint32_t nt = real ? (uint32_t)s_ntri[sm] : 0u;
            acc.v += nv;
            acc.t += nt;
            acc.c += (nv | nt) ? 1u : 0u;
            acc.b += real ? 1u : 0u;
        }
        qc = ql;
    };
    auto flush_queue = [&]() {
        if (!P.tq) count_pending();
        __builtin_amdgcn_wave_barrier();
        if (qflushed + ql <= P.qlimit) {
            for (uint32_t o = lane; o < ql; o += 64u) gq[qflushed + o] = q[o];
            qflushed += ql;
        } else {
            overflow = true;
        }
        __builtin_amdgcn_wave_barrier();
        ql = 0; qc = 0;
    };
    auto flush_brec = [&]() {
        __builtin_amdgcn_wave_barrier();
        if (lane < nbl) {
            cx_brec R;
            R.qoff = s_br[wave][lane][0]; R.n = s_br[wave][lane][1]; R.vpre = s_br[wave][lane][2];
            R.tpre = s_br[wave][lane][3]; R.cpre = s_br[wave][lane][4]; R.near = 0; R.pad0 = 0; R.pad1 = 0;
            brec[nbflushed + lane] = R;
        }
        __builtin_amdgcn_wave_barrier();
        nbflushed += nbl;
        nbl = 0;
    };
    auto close_batch = [&]() {
        if (!P.tq) count_pending();
        const uint32_t bv = cxd_wave_add(acc.v), bt = cxd_wave_add(acc.t), bc = cxd_wave_add(acc.c);
        if (lane == 0) {
            s_br[wave][nbl][0] = qstart; s_br[wave][nbl][1] = qn - qstart; s_br[wave][nbl][2] = rv;
            s_br[wave][nbl][3] = rt; s_br[wave][nbl][4] = rc;
        }
        nbl++; nb++; rv += bv; rt += bt; rc += bc;
        nr += (qn - qstart + 63u) >> 6;
        qstart = qn;
        acc.v = acc.t = acc.c = 0;
    };
    if (nrows != 0u && p < ib) {
        const uint32_t kofs = k0 + 4u * lane;
        const bool lane_valid = kofs < P.n2;
        const uint32_t nvalid = lane_valid ? min(4u, P.n2 - kofs) : 0u;   // samples of the row this lane holds (ALIGNED: 4 or 0)
        const uint32_t kofs_c = (nvalid == 4u) ? kofs : (P.n2 - 4u);      // other lanes (re-)read the row's last 4 samples
        const uint32_t kshift = kofs - kofs_c;                            // ... and shift them into place (1..3; garbage for lanes off the row)
        const uint32_t last_lane = (uint32_t)__popcll(__ballot(lane_valid)) - 1u;
        const bool halo_in = (k0 + 256u) < P.n2;                  // a sample right of this segment exists
        // cells that exist / whose k+1 / j+1 neighbour exists (bit layout of CX_CELL_MASK)
        const cx_lmasks LM = cx_lane_masks(P, k0, j0, lane);
        const uint32_t mr = LM.mr, mk = LM.mk, mj = LM.mj;
        (void)mk; (void)mj;

        // one sample plane of this lane: RJ+1 rows x 4 consecutive k-samples, plus the sample right of the segment
        struct plane_raw {
            typename cx_row4<DT>::v v[CX_RJ + 1];
            typename cx_row4<DT>::h hv[CX_RJ + 1];
        };
        const uint32_t plane_last = min(ib, P.n0 - 1u);
        auto load_plane = [&](uint32_t pp, plane_raw& R) {
            const uint32_t pc = min(pp, plane_last);   // never beyond the last plane this task needs: a request past it re-reads that plane (a cache hit)
#pragma unroll
            for (int r = 0; r <= CX_RJ; r++) {
                const uint32_t jr = min(j0 + (uint32_t)r, P.n1 - 1u);   // rows beyond the array repeat the last row
                const uint32_t rowofs = (pc * P.n1 + jr) * P.n2;
                if constexpr (DT != CX_DTYPE_F32) {
                    typedef typename cx_row4<DT>::v V;
                    R.v[r] = reinterpret_cast<const cx_row4_ua<V, ALIGNED ? sizeof(V) : sizeof(*A)>*>(A + rowofs + kofs_c)->v;
                    R.hv[r] = A[rowofs + (halo_in ? k0 + 256u : 0u)];                // raw bits, wave-uniform address
                } else {
                R.v[r] = *reinterpret_cast<const float4*>(A + rowofs + kofs_c);      // lanes right of the array re-read its last 4 samples
                R.hv[r] = A[rowofs + (halo_in ? k0 + 256u : 0u)];                    // wave-uniform address
                }
            }
        };
        // sign bits of a loaded plane.  f < vcmp  <=>  sign bit of (f - vcmp)  (f == vcmp gives +0 -- also for f = -0.0 at isovalue 0:
        // the host passes that threshold as -0.0, cx_fill_value_params; NaN samples are not supported); the same differences feed the
        // tolerance screen (smallest |f - vcmp| seen)
        float (*ring)[CX_RJ + 1][CX_PLW] = reinterpret_cast<float (*)[CX_RJ + 1][CX_PLW]>(s_pl_dyn + (size_t)wave * (2u * (CX_RJ + 1u) * CX_PLW));
        const bool stage_t = P.tq != nullptr;      // wave-uniform: this extraction hands fractions on (else the vertex stage gathers samples)
        const bool stage_ring = stage_t;
        auto plane_bits = [&](const plane_raw& R, const uint32_t slot) -> uint32_t {
            // The sign bits are shifted in from the right, last row first: one v_alignbit_b32 per sample ({word, difference} >> 31 = the
            // word moved up by one with the sign bit of the difference behind it) instead of a shift and a shift-or; rows are
            // CX_ROWBITS apart: two more places after each row of four.  (The stream kernel is bound by its instructions.)
            uint32_t own = 0, halo = 0;
#pragma unroll
            for (int r = CX_RJ; r >= 0; r--) {
                float vx, vy, vz, vw_, hv;
                if constexpr (DT == CX_DTYPE_F32) {
                    vx = R.v[r].x; vy = R.v[r].y; vz = R.v[r].z; vw_ = R.v[r].w; hv = R.hv[r];
                } else {
                    cx_row4_unpack<DT>(R.v[r], vx, vy, vz, vw_);
                    hv = cx_dt<DT>::cvt(R.hv[r]);
                }
                const float vw = vw_;
                if (!ALIGNED) {   // lane at the end of the row: samples kofs.. of (n2-4 .. n2-1), the last one repeated
                    vx = (kshift == 1u) ? vy : ((kshift == 2u) ? vz : ((kshift == 3u) ? vw : vx));
                    vy = (kshift == 0u) ? vy : ((kshift == 1u) ? vz : vw);
                    vz = (kshift == 0u) ? vz : vw;
                }
                if (stage_ring) {   // the lane's four samples of row r, in place; the sample right of the segment behind them
                    *reinterpret_cast<float4*>(&ring[slot][r][4u * lane]) = make_float4(vx, vy, vz, vw);
                    if (lane == 0u) ring[slot][r][256] = hv;
                }
                const float dx = vx - P.vcmp, dy = vy - P.vcmp, dz = vz - P.vcmp, dw = vw - P.vcmp;
                const float dh = hv - P.vcmp;
                own <<= (CX_ROWBITS - 4u);                                     // the two unused places of the row above
                own = __builtin_amdgcn_alignbit(own, __float_as_uint(dw), 31);   // bit 3 of the row
                own = __builtin_amdgcn_alignbit(own, __float_as_uint(dz), 31);
                own = __builtin_amdgcn_alignbit(own, __float_as_uint(dy), 31);
                own = __builtin_amdgcn_alignbit(own, __float_as_uint(dx), 31);   // bit 0
                halo <<= (CX_ROWBITS - 1u);
                halo = __builtin_amdgcn_alignbit(halo, __float_as_uint(dh), 31);
                dnear = fminf(dnear, fminf(fminf(fabsf(dx), fabsf(dy)), fminf(fabsf(dz), fminf(fabsf(dw), fabsf(dh)))));
            }
            // k+1 neighbour of m=3: m=0 of the next lane; the last valid lane takes the halo sample or,
            // at the array edge, repeats its own m=3 (clamped corner)
            // lane l takes the word of lane l + 1 (DPP wave_shl:1, a VALU move; __shfl_down is a ds_bpermute: an LDS round trip per step)
            uint32_t nbr = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)own, 0x130, 0xF, 0xF, false) & CX_M0_MASK;
            if (lane == last_lane) nbr = halo_in ? halo : ((own >> 3) & CX_M0_MASK);
            return own | (nbr << 4);
        };

        // Sample planes p .. ib are needed (cell plane ib - 1 reads sample plane ib).  The prefetch runs past ib; those requests are
        // issued all the same -- a branch around them makes the compiler wait for ALL outstanding loads at the next use, which undoes
        // the prefetch (measured: 0.126 -> 0.138 ms) -- but re-read plane ib, a cache hit, instead of the neighbour task's plane ib + 1
        // (rounds 1 and 2: one plane in ci + 2, 6 % of the kernel's HBM reads).
        // One plane is in flight ahead of the one being worked on.  Two planes in flight ahead: 0.131 against 0.125 ms, 168 registers;
        // taken out (the kernel is not starved for samples).
        plane_raw rawA, rawB;
        load_plane(p, rawB);
        load_plane(p + 1u, rawA);
        uint32_t wprev = plane_bits(rawB, 0u);
        // one step: plane p+1 is in `cur` (loaded one step ago), plane p+2 is requested into `nxt`
        auto step = [&](const plane_raw& cur, plane_raw& nxt) {
            load_plane(p + 2u, nxt);
            const uint32_t wcur = plane_bits(cur, (p + 1u - G.pstart) & 1u);
            // per sample row: OR / AND over (k, k+1); then over rows (r, r+1); then over both planes
            const uint32_t op = wprev | (wprev >> 1), ap = wprev & (wprev >> 1);
            const uint32_t oc = wcur | (wcur >> 1), ac = wcur & (wcur >> 1);
            const uint32_t o = op | (op >> CX_ROWBITS) | oc | (oc >> CX_ROWBITS);
            const uint32_t a = ap & (ap >> CX_ROWBITS) & ac & (ac >> CX_ROWBITS);
            const uint32_t act0 = o & ~a & mr;
            if (__ballot(act0 != 0u) != 0ULL) {    // wave-uniform: some cell of this step has a sign change
                // exclusive prefix of the lanes' cell counts by DPP row shifts (9 instructions; five ballots with their mbcnt pairs: 35)
                const uint32_t cnt0 = __popc(act0);
                const uint32_t incl0 = cx_wave_incl_scan(cnt0, lane);
                const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl0, 63);
                const uint32_t pre = incl0 - cnt0;
                const uint32_t sidx = p - G.pstart;
                const uint32_t ebase = (lane << 15) | (sidx << 21);
                // where the lane's cells of this step sit in the wave's queue, and which they are (bit 4r+m): lets the triangle stage
                // find the queue entry of ANY active cell of the volume without a table per sample.  Straight to global memory, one
                // coalesced 256-byte store per step that queued cells (round 3 staged all steps' words in 17 KB of LDS and wrote them
                // out at the end, active or not; measured: the direct store is 3 % FASTER, and the LDS goes to the sample planes)
                if (P.qa) (P.qa + (size_t)w * (CX_SWP * 64u))[sidx * 64u + lane] =
                    ((qn + pre) << 16) | (act0 & 0xFu) | ((act0 >> 2) & 0xF0u) | ((act0 >> 4) & 0xF00u) | ((act0 >> 6) & 0xF000u);
                // The step's cells go through the entry stage in the order of the lanes; more than the stage holds (CX_SQ; up to 1024
                // on white noise) go in two halves of the lanes -- the order in the queue is the same either way.
                const uint32_t nhalf = (tot > CX_SQ) ? 2u : 1u;            // wave-uniform
                const uint32_t mid = (uint32_t)__builtin_amdgcn_readlane((int)pre, 32);   // cells of lanes 0..31
                const float* __restrict__ plo = &ring[sidx & 1u][0][0];          // sample plane p   (the cells' lower corners)
                const float* __restrict__ phi = &ring[(sidx + 1u) & 1u][0][0];   // sample plane p+1
                float* __restrict__ tqw = stage_t ? P.tq + (size_t)w * T.wcap : nullptr;
                for (uint32_t h = 0; h < nhalf; h++) {
                    const uint32_t cbase = (nhalf == 2u && h == 1u) ? mid : 0u;
                    const uint32_t ctot = (nhalf == 2u) ? (h == 0u ? mid : tot - mid) : tot;
                    if (ql + ctot > CX_SQ) flush_queue();   // wave-uniform
                    uint32_t act = (nhalf == 1u || (lane >> 5) == h) ? act0 : 0u;
                    uint32_t pos = ql + pre - cbase;
                    while (act) {
                        const uint32_t bit = __ffs(act) - 1u;
                        act &= act - 1u;
                        // corners (k,k+1) of rows (r,r+1): bits (bit, bit+1, bit+6, bit+7) of the two plane words
                        q[pos++] = ebase | (bit << 10) | ((wprev >> bit) & 0xC3u) | (((wcur >> bit) & 0xC3u) << 2);
                    }
                    // One lane per queued ENTRY: the counts of the cells just queued, with the vertex stage's own formulas
                    // (cx_vround_front), and -- with the samples of both planes in LDS -- the fraction t = (v - f(q)) / (f(q+d) - f(q))
                    // of every crossing the cell owns, written to the wave's stream of fractions in the order the vertex stage numbers
                    // the vertices (cell after cell, direction after direction).
                    __builtin_amdgcn_wave_barrier();
                    for (uint32_t o0 = 0; o0 < (stage_t ? ctot : 0u); o0 += 64u) {      // wave-uniform: without the fraction stream the cells are counted by count_pending
                        const uint32_t o = o0 + lane;
                        const bool have = o < ctot;
                        const uint32_t e = have ? q[ql + o] : 0u;
                        uint32_t ci, cj, ck;
                        cx_decode_entry(P, G, e, ci, cj, ck);
                        const uint32_t vm = have ? cx_corner_valid(P, ci, cj, ck) : 0u;
                        const uint32_t sm = cx_entry_signs(e);
                        const uint32_t s0 = (sm & 1u) ? 0xFFu : 0u;
                        const uint32_t emask = ((sm ^ s0) & vm) & 0xFEu;
                        const uint32_t nv = __popc(emask);
                        const bool real = (vm == 0xFFu);
                        const uint32_t nt = real ? (uint32_t)s_ntri[sm] : 0u;
                        acc.v += nv;
                        acc.t += nt;
                        acc.c += (nv | nt) ? 1u : 0u;
                        acc.b += real ? 1u : 0u;
                        if (stage_t) {      // wave-uniform
                            // corner c = 4 di + 2 dj + dk of the cell: plane di, row rr + dj, sample + dk.  All eight are requested at
                            // once, ahead of the prefix sums below (written as seven guarded loads, each crossing waited for its own
                            // LDS round trip: measured +43 us on the kernel), and all seven fractions are computed -- two
                            // instructions each -- whether the edge is crossed or not; only the stores are guarded.
                            const uint32_t bit = (e >> 10) & 31u;
                            const uint32_t rr = (bit * 11u) >> 6;
                            const uint32_t at = rr * CX_PLW + 4u * ((e >> 15) & 63u) + (bit - 6u * rr);
                            float f0 = plo[at], f1 = plo[at + 1u], f2 = plo[at + CX_PLW], f3 = plo[at + CX_PLW + 1u];
                            float f4 = phi[at], f5 = phi[at + 1u], f6 = phi[at + CX_PLW], f7 = phi[at + CX_PLW + 1u];
                            uint32_t vtot;
                            const uint32_t vpre = cx_wave_prefix_small<3>(nv, vtot);
                            if (tv + vtot <= P.tlimit) {    // wave-uniform
                                asm volatile("" : "+v"(f0), "+v"(f1), "+v"(f2), "+v"(f3), "+v"(f4), "+v"(f5), "+v"(f6), "+v"(f7));
                                const float num = (P.vhi - f0) + P.vlo;
                                const float t1 = cx_fraction(num, f1 - f0), t2 = cx_fraction(num, f2 - f0), t3 = cx_fraction(num, f3 - f0);
                                const float t4 = cx_fraction(num, f4 - f0), t5 = cx_fraction(num, f5 - f0), t6 = cx_fraction(num, f6 - f0);
                                const float t7 = cx_fraction(num, f7 - f0);
                                float* __restrict__ dst = tqw + tv + vpre;
                                if (emask & 0x02u) dst[0] = t1;
                                if (emask & 0x04u) dst[__popc(emask & 0x02u)] = t2;
                                if (emask & 0x08u) dst[__popc(emask & 0x06u)] = t3;
                                if (emask & 0x10u) dst[__popc(emask & 0x0Eu)] = t4;
                                if (emask & 0x20u) dst[__popc(emask & 0x1Eu)] = t5;
                                if (emask & 0x40u) dst[__popc(emask & 0x3Eu)] = t6;
                                if (emask & 0x80u) dst[__popc(emask & 0x7Eu)] = t7;
                            } else {
                                overflow_t = true;          // more crossings than the wave's region holds: its cells take the per-cell path downstream
                            }
                            tv += vtot;
                        }
                    }
                    ql += ctot;
                    qn += ctot;
                    __builtin_amdgcn_wave_barrier();
                }
                if (qn - qstart >= CX_BATCH_MIN) close_batch();
            }
            wprev = wcur;
            p++;
        };
        while (p < ib) {
            step(rawA, rawB);
            if (p >= ib) break;
            step(rawB, rawA);
        }
    }
    if (qn > qstart) close_batch();
    flush_queue();
    flush_brec();
    if (stamp && lane == 0) stamp[1] = __builtin_amdgcn_s_memtime();
    cx_run run;
    run.v = rv; run.t = rt; run.c = rc; run.b = cxd_wave_add(acc.b);
    const bool near = __ballot(dnear <= P.near_abs) != 0ULL;   // wave-uniform
    bool really_near = false;
    if (near && qn != 0u && !overflow) {
        // a sample inside the screen: the reference's tolerance rules may drop tetrahedra or vertices.
        // Count exactly (per-cell path over the wave's own queue; its stores are complete after the
        // fence) and hand the whole queue over as ONE batch that takes the per-cell path downstream.
        __threadfence();
        cx_run ex = {0, 0, 0, 0, 0};
        cx_process_queue<false, DT>(P, [&](uint32_t x) { return cx_entry_lin(P, G, __builtin_nontemporal_load(gq + x)); }, qn, lane, false, ex, nullptr);
        // The tolerance rules only ever REMOVE crossings and triangles from what the signs give.  Equal totals therefore
        // mean equal masks in every cell: the wave stays on the common path (its batches, its numbering), only the border
        // voxel count is the exact one.  Otherwise: ONE batch that takes the per-cell path downstream.
        really_near = !(ex.v == rv && ex.t == rt && ex.c == rc && ex.s == 0u);
        run.b = ex.b;
        if (really_near) { run.v = ex.v; run.t = ex.t; run.c = ex.c; }
    }
    // a wave whose stream of fractions ran out of room (more crossings than one per cell of its tile: white noise) hands its cells
    // to the per-cell path too -- which interpolates from the samples itself; its counts are the ones the signs gave
    if (overflow_t && qn != 0u && !overflow) really_near = true;
    if (really_near) {
        nb = 1;
        nr = (qn + 63u) >> 6;
        if (lane == 0) {
            cx_brec R;
            R.qoff = 0; R.n = qn; R.vpre = 0; R.tpre = 0; R.cpre = 0; R.near = 1; R.pad0 = 0; R.pad1 = 0;
            brec[0] = R;
        }
    }
    if (lane == 0) {
        cx_wsum S;
        S.nb = nb; S.v = run.v; S.t = run.t; S.c = run.c; S.b = run.b; S.nq = qn; S.near = really_near ? 1u : 0u; S.nr = nr;
        P.wsum[w] = S;
        s_tot[wave][0] = run.v; s_tot[wave][1] = run.t; s_tot[wave][2] = run.c; s_tot[wave][3] = run.b; s_tot[wave][4] = nb;
        s_tot[wave][5] = (really_near && qn != 0u) ? 1u : 0u;
        s_tot[wave][6] = nr;
        s_tot[wave][7] = overflow ? 1u : 0u;
    }
    // totals of every 256 waves (64 workgroups), so that the scan needs ONE round of loads for everything before its chunk
    // (the per-wave totals were just written by CUs all over the chip: each dependent round of loads from them costs ~2 us).
    // One atomic per workgroup and counter.
    __syncthreads();
    if (threadIdx.x < 8u) {
        const uint32_t sum = s_tot[0][threadIdx.x] + s_tot[1][threadIdx.x] + s_tot[2][threadIdx.x] + s_tot[3][threadIdx.x];
        uint32_t* cs = P.chunksum + (size_t)(b >> 6) * 8u;
        if (sum) atomicAdd(cs + threadIdx.x, sum);      // (slot 5: number of waves on the tolerance path; non-zero = flag; slot 6: rounds; slot 7: waves whose queue slice overflowed)
    }
}
template <bool ALIGNED, int DT>
__global__ __launch_bounds__(256, CX_K1_MIN_WAVES) void cx_k_stream(const cx_params P, const cx_task T) {
    cx_stream_tile<ALIGNED, DT>(P, T, cx_task_of_block(T));
}
// Several isovalues of ONE grid: the same pass, with workgroups numbered (tile, level), the level running fastest
// inside an XCD's sequence: the nlevels workgroups that stream one tile run next to each other on one XCD, so the tile comes
// from HBM once and from that XCD's L2 / the Infinity Cache for the other levels.  LP[level] = parameters of a level
// (isovalue, its queues and side tables).
// The parameters of up to CX_LEVELS_PER_LAUNCH levels travel BY VALUE as a kernel argument.  Read from a device array, as they were
// until the end of round 3, their pointers are generic as far as the compiler knows: loads and stores through them came out as FLAT
// instructions, which count on both memory counters -- every wait in the kernel was `vmcnt(0) lgkmcnt(0)`, the plane requested for the
// NEXT step was waited for together with the current one.  Pointers inside a kernel argument are known to be global: the waits are
// the counted ones of cx_k_stream again.  (It did not change the time -- 2.33 ms for 8 levels either way: the kernel is bound by its
// instructions, DESIGN section 10 -- but it is the code the single-level kernel runs.)
#define CX_LEVELS_PER_LAUNCH 8u
struct cx_params_pack {
    cx_params p[CX_LEVELS_PER_LAUNCH];
};
template <bool ALIGNED, int DT>
__global__ __launch_bounds__(256, CX_K1_MIN_WAVES) void cx_k_stream_levels(const cx_params_pack LP, const cx_task T, const uint32_t nlevels) {
    const uint32_t seq = blockIdx.x >> 3;                   // position in this XCD's sequence of workgroups
    const uint32_t tile_seq = seq / nlevels, level = seq - tile_seq * nlevels;
    cx_stream_tile<ALIGNED, DT>(LP.p[level], T, (blockIdx.x & 7u) * T.chunk + tile_seq);
}

// ---- S2 in one launch: workgroup g owns the streaming waves [256 g, 256 g + 256).  It sums the totals of ALL waves before its
// chunk itself (every thread reads one wave of each earlier chunk: g x 8 KB per workgroup out of L2 -- no partial sums to
// wait for, no second kernel, no atomics), scans its own 256 waves, and writes their output offsets and batch descriptors;
// the last workgroup, which has seen every wave, writes the counters.  (One workgroup scanning all 12 k waves of a 512^3
// grid was bound by what a single CU can pull: 22 us + 5 us for the list kernel.)
__device__ __forceinline__ void cx_scan_list_chunk(const cx_params& P, const cx_task& T, const uint32_t nw, const uint32_t g, const uint32_t nchunks) {
    __shared__ uint32_t s_part[4][8];    // per wave of the workgroup: totals of the earlier chunks (6), near | overflow << 1, rounds of ALL chunks
    __shared__ uint32_t s_own[4][6];     // per wave: inclusive totals of its 64 streaming waves
    const uint32_t tid = threadIdx.x, lane = cx_lane_id(), wave = tid >> 6;
    uint32_t acc[6] = {0, 0, 0, 0, 0, 0}, near_any = 0, rall = 0, over_any = 0;   // v, t, c, b, nb, nr
    for (uint32_t c = tid; c < nchunks; c += 256u) {     // thread c: the totals of chunk c (every workgroup looks at all of them: near flag, total rounds)
        const uint4 lo = *reinterpret_cast<const uint4*>(P.chunksum + (size_t)c * 8u);
        const uint4 hi = *reinterpret_cast<const uint4*>(P.chunksum + (size_t)c * 8u + 4u);
        if (c < g) { acc[0] += lo.x; acc[1] += lo.y; acc[2] += lo.z; acc[3] += lo.w; acc[4] += hi.x; acc[5] += hi.z; }
        near_any |= hi.y;
        rall += hi.z;
        over_any |= hi.w;
    }
    const uint32_t w = g * 256u + tid;
    cx_wsum S;
    S.nb = S.v = S.t = S.c = S.b = S.nq = S.near = S.nr = 0;
    if (w < nw) S = P.wsum[w];
    near_any |= (S.near != 0u && S.nq != 0u) ? 1u : 0u;
    const uint32_t x[6] = {S.v, S.t, S.c, S.b, S.nb, S.nr};
    uint32_t inc[6];
#pragma unroll
    for (int m = 0; m < 6; m++) {
        inc[m] = cx_wave_incl_scan(x[m], lane);
        const uint32_t before = cxd_wave_add(acc[m]);
        if (lane == 63u) { s_own[wave][m] = inc[m]; s_part[wave][m] = before; }
    }
    {
        const uint32_t nr = (__ballot(near_any != 0u) != 0ULL) ? 1u : 0u;
        const uint32_t ra = cxd_wave_add(rall);
        const uint32_t ov = (__ballot(over_any != 0u) != 0ULL) ? 1u : 0u;
        if (lane == 63u) { s_part[wave][6] = nr | (ov << 1); s_part[wave][7] = ra; }
    }
    __syncthreads();
    uint32_t ex[6];
#pragma unroll
    for (int m = 0; m < 6; m++) {
        uint32_t base = s_part[0][m] + s_part[1][m] + s_part[2][m] + s_part[3][m];
        for (uint32_t ww = 0; ww < wave; ww++) base += s_own[ww][m];
        ex[m] = base + inc[m] - x[m];
    }
    // the vertex stage divides the rounds of 64 queued cells evenly among its P.nvw waves: wave m takes rounds [m q, m q + q)
    const uint32_t rounds = s_part[0][7] + s_part[1][7] + s_part[2][7] + s_part[3][7];
    const uint32_t q = max((rounds + P.nvw - 1u) / P.nvw, CX_S3_MIN_SHARE);
    const uint32_t qk = max((rounds + P.nkw - 1u) / P.nkw, CX_S3_MIN_SHARE);
    if (w < nw) {
        cx_wbase B;
        B.v = ex[0]; B.t = ex[1]; B.c = ex[2]; B.boff = ex[4];
        P.wbase[w] = B;
        // the flat batch list: self-contained descriptors
        const cx_tile tile = cx_tile_of(P, T, w >> 2, w & 3u);
        uint32_t rb = ex[5];
        for (uint32_t i = 0; i < S.nb; i++) {
            if (ex[4] + i >= P.fcap) break;
            const cx_brec R = P.brec[(size_t)w * T.bcap + i];
            cx_bdesc D;
            D.w = w; D.qofs = w * T.wcap + R.qoff; D.n = R.n; D.near = R.near;
            D.vbase = ex[0] + R.vpre; D.tbase = ex[1] + R.tpre; D.cbase = ex[2] + R.cpre; D.rbase = rb;
            D.p = tile.p; D.j0 = tile.j0; D.k0 = tile.k0; D.nsteps = tile.ib - tile.p;
            P.flat[ex[4] + i] = D;
            // the waves whose share starts inside this batch
            const uint32_t nrb = (R.n + 63u) >> 6;
            for (uint32_t m = (rb + q - 1u) / q; m * q < rb + nrb; m++) P.rstart[m] = ex[4] + i;
            for (uint32_t m = (rb + qk - 1u) / qk; m * qk < rb + nrb; m++) P.kstart[m] = ex[4] + i;   // the same for the triangle stage's waves
            rb += nrb;
        }
    }
    if (P.torder) {
        // the tile kernel's order of work (cx_tile3d.h): half tiles (the queues of streaming waves 2m, 2m + 1) by class of queue
        // entries, most first -- with the tiles in launch order the kernel ended in a tail of its heaviest workgroups (60 of 245 us
        // at 512^3) -- and the empty ones in no list at all.  One reservation per workgroup and class.
        __shared__ uint32_t s_cls[3][4], s_clsbase[3];
        const uint32_t nqp = S.nq + (uint32_t)__shfl_down((int)S.nq, 1);        // even lanes: entries of the half tile
        const bool isht = !(tid & 1u) && w < nw;
        const uint32_t cls = !isht ? 4u : (nqp >= (P.tile_cap * 5u >> 3) ? 0u : (nqp >= (P.tile_cap * 5u >> 4) ? 1u : (nqp ? 2u : 3u)));
        uint32_t rank = 0;
#pragma unroll
        for (uint32_t c = 0; c < 3u; c++) {
            const uint64_t m = __ballot(cls == c);
            if (cls == c) rank = cx_mbcnt(m);
            if (lane == 0) s_cls[c][wave] = (uint32_t)__popcll(m);
        }
        __syncthreads();
        if (tid < 3u) {
            const uint32_t n = s_cls[tid][0] + s_cls[tid][1] + s_cls[tid][2] + s_cls[tid][3];
            s_clsbase[tid] = n ? atomicAdd(&P.counters[CX_CNT_TCLS + tid], n) : 0u;
        }
        __syncthreads();
        if (cls < 3u) {
            uint32_t at = s_clsbase[cls] + rank;
            for (uint32_t ww = 0; ww < wave; ww++) at += s_cls[cls][ww];
            P.torder[(size_t)cls * (nw >> 1) + at] = w >> 1;
        } else if (cls == 3u) {
            P.bndn[w >> 1] = 0u;          // nothing crosses this half tile: no boundary voxels
        }
    }
    if (g == nchunks - 1u && tid == 255u) {   // this thread's inclusive totals are the grand totals
        P.counters[CX_CNT_VERTS] = ex[0] + x[0]; P.counters[CX_CNT_TRIS] = ex[1] + x[1];
        P.counters[CX_CNT_CELLS] = ex[2] + x[2]; P.counters[CX_CNT_BORDER] = ex[3] + x[3];
        P.counters[CX_CNT_BATCHES] = ex[4] + x[4];
        P.counters[CX_CNT_ROUNDS] = rounds;
        const uint32_t fl = s_part[0][6] | s_part[1][6] | s_part[2][6] | s_part[3][6];
        P.counters[CX_CNT_NEAR] = fl & 1u;
        P.counters[CX_CNT_OVERFLOW] = (fl >> 1) & 1u;
        P.counters[CX_CNT_TILEOVF] = 0u;
    }
}
__global__ __launch_bounds__(256) void cx_k_scan_list(const cx_params P, const cx_task T, const uint32_t nw) {
    cx_scan_list_chunk(P, T, nw, blockIdx.x, gridDim.x);
}
__global__ __launch_bounds__(256) void cx_k_scan_list_levels(const cx_params* __restrict__ LP, const cx_task T, const uint32_t nw) {
    const cx_params P = LP[blockIdx.y];
    cx_scan_list_chunk(P, T, nw, blockIdx.x, gridDim.x);
}
