#pragma once
// cx_tri3d.h -- the TRIANGLE STAGE of the 3-D march: the CPython tuple hash and set order behind the quad diagonals, the pattern
// tables, the two phases every triangle-emitting kernel runs from LDS (cx_tri_lds*, cx_tri_in, cx_tri_phase1 / cx_tri_phase2).
// Defines cx_k_hash_xy and the three triangle kernels: cx_k_emit_triangles (generic pipeline: 16-byte records, neighbours from a
// table of one entry per sample), cx_k_emit_triangles_q (staged pipeline, the default: cell records, neighbours from their queue
// entries' words; cx_tri_qa) and cx_k_emit_triangles_e (CX_K2_ENTRIES: walks queue entries; cx_esrc, cx_eraw).
// A section of the cx_march3d.hip translation unit: included only there, in this place, and not self-contained.  It relies on
// cx_emit3d.h (the entry, info-word and record formats) and on what cx_stream3d.h writes (the queues and P.qa).

// ---- CPython 3.10 tuple hash + 8-slot set order, used only with
// CX_DIAG_CPYTHON310 to reproduce the quad diagonal the reference picks (tetrahedral.py:592-595).
// hash((x,y,z)) = finish(round(round(round(P5, x), y), z)); the first two rounds depend only on
// (x,y) and come from a table built once per grid shape (cx_k_hash_xy).
#define CX_PY_P1 11400714785074694791ULL
#define CX_PY_P2 14029467366897019727ULL
#define CX_PY_P5 2870177450012600261ULL
__device__ __forceinline__ uint64_t py_round(uint64_t acc, uint32_t x) {
    acc += (uint64_t)x * CX_PY_P2;
    acc = (acc << 31) | (acc >> 33);
    return acc * CX_PY_P1;
}
// the same round for a lattice coordinate that may be negative (an array with a rim of samples around the reference's
// grid has its origin at -1): CPython hashes a small int to itself, except hash(-1) == -2
__device__ __forceinline__ uint64_t py_round_signed(uint64_t acc, int32_t x) {
    const uint64_t lane = (x == -1) ? ~1ULL : (uint64_t)(int64_t)x;
    acc += lane * CX_PY_P2;
    acc = (acc << 31) | (acc >> 33);
    return acc * CX_PY_P1;
}
// the second half of py_round: acc already holds accumulator + lane * P2
__device__ __forceinline__ uint64_t py_round_tail(uint64_t acc) {
    acc = (acc << 31) | (acc >> 33);
    return acc * CX_PY_P1;
}
__device__ __forceinline__ uint64_t py_finish3(uint64_t acc) {
    acc += 3ULL ^ (CX_PY_P5 ^ 3527539ULL);
    return (acc == ~0ULL) ? 1546275796ULL : acc;
}
__global__ void cx_k_hash_xy(uint64_t* table, uint32_t n0, uint32_t n1, uint32_t org0, uint32_t org1) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n0 * n1) return;
    const uint32_t i = idx / n1, j = idx - i * n1;
    table[idx] = py_round_signed(py_round_signed(CX_PY_P5, (int32_t)i + (int32_t)org0), (int32_t)j + (int32_t)org1);
}
// does a 2-element set {first inserted h1, then h2} iterate h2 first?
__device__ __forceinline__ bool py_set2_swapped(uint64_t h1, uint64_t h2) {
    const uint32_t s1 = (uint32_t)h1 & 7u;
    uint32_t s2 = (uint32_t)h2 & 7u;
    uint64_t perturb = h2;
    for (int guard = 0; guard < 16 && s2 == s1; guard++) {
        perturb >>= 5;
        s2 = (uint32_t)((s2 * 5u + 1u + perturb) & 7u);
    }
    return s2 < s1;
}

// the same from the low 32 bits of the hashes (five probe steps fit); `unres`: still on one slot after five steps
__device__ __forceinline__ bool py_set2_swapped_lo(uint32_t h1, uint32_t h2, bool& unres) {
    const uint32_t s1 = h1 & 7u;
    uint32_t s2 = h2 & 7u;
    uint32_t perturb = h2;
    for (int guard = 0; guard < 5 && s2 == s1; guard++) {
        perturb >>= 5;
        s2 = (s2 * 5u + 1u + perturb) & 7u;
    }
    unres = (s2 == s1);
    return s2 < s1;
}

// The same decision from one byte per lattice point (cx_k_hash_bytes, built once per grid shape and origin): bits 0-2 = slot
// of hash((i,j,k)) in an 8-slot table, bits 3-5 = the first slot of its probe sequence that differs from it (what it takes
// when another element sits in its slot; the same slot again if 16 probes never leave it).
// py_set2_swapped(h1, h2) == (t2 != s1 ? t2 < s1 : alt2 < s1): the loop above stops at the first probe of h2 that differs
// from s1 == t2.  Second element iterates first?  (set built by inserting a then b)
__device__ __forceinline__ bool cx_set2_swapped(uint32_t ca, uint32_t cb) {
    const uint32_t sa = ca & 7u, tb = cb & 7u, ab = (cb >> 3) & 7u;
    return ((tb != sa) ? tb : ab) < sa;
}

// tet vertex m of tet t -> cube corner, as compile-time constants (same data as cx_d_tet_corners)
__device__ constexpr uint8_t CX_TC[6][4] = CX_TET_CORNERS_INIT;
#define CX_TC_MASK(t) ((1u << CX_TC[t][0]) | (1u << CX_TC[t][1]) | (1u << CX_TC[t][2]) | (1u << CX_TC[t][3]))

// =================================================================================================
// K2 triangles.  Phase 1, one lane per cell record: the (first vertex, crossing mask) pairs of the 7
// corners that can own an edge of the voxel go to LDS, and every triangle of the cell gets a slot word
// (cell lane, LUT entry, which of its 2 triangles, rank in the cell).  Phase 2, one lane per TRIANGLE:
// three (owner corner, direction) pairs from the LUT -> three vertex indices -> one 12-byte store,
// consecutive lanes writing consecutive triangles.  No divergent per-tetrahedron expansion.
// =================================================================================================
__device__ constexpr uint32_t CX_TRI_CD[6][16][2][2] = CX_TET_TRIS_CD_INIT;
#ifndef CX_VE_ROW
#define CX_VE_ROW 65
#endif
// what depends on the corner sign mask of a voxel alone, as tables (built at compile time from the tetrahedron list)
constexpr uint8_t CX_TCH[6][4] = CX_TET_CORNERS_INIT;
struct cx_pats_tab {
    uint32_t w[256][2];    // [sm]: x = 6 tetrahedron patterns x 4 bits (bit m: tet vertex m is low) | mask of the 2-2 tetrahedra << 24;
                           //       y = mask of the 1-3 / 3-1 tetrahedra | neighbour cells 1..6 that own a crossing edge of the voxel << 8
    uint16_t c22[6 * 16];  // [tet * 16 + pattern] of a 2-2 tetrahedron: cube corners of its low pair and of its high pair (tet
                           // vertex order = the reference's set insertion order), 3 bits each
};
constexpr cx_pats_tab cx_make_pats() {
    cx_pats_tab T{};
    for (uint32_t sm = 0; sm < 256u; sm++) {
        uint32_t pw = 0, m22 = 0, m1 = 0, want = 0;
        for (uint32_t t = 0; t < 6u; t++) {
            uint32_t pat = 0, np = 0;
            for (uint32_t m = 0; m < 4u; m++) {
                const uint32_t b = (sm >> CX_TCH[t][m]) & 1u;
                pat |= b << m;
                np += b;
            }
            pw |= pat << (4u * t);
            if (np == 2u) m22 |= 1u << t;
            if (np == 1u || np == 3u) m1 |= 1u << t;
        }
        for (uint32_t c = 1; c < 7u; c++) {
            // does corner c own a crossing edge of this voxel?  (a strict superset corner on the other side)
            const uint32_t sc = ((sm >> c) & 1u) ? 0xFFu : 0u;
            uint32_t sup = 0;
            for (uint32_t c2 = 0; c2 < 8u; c2++) sup |= ((c2 & c) == c && c2 != c) ? (1u << c2) : 0u;
            if (((sm ^ sc) & sup) != 0u) want |= 1u << c;
        }
        T.w[sm][0] = pw | (m22 << 24);
        T.w[sm][1] = m1 | (want << 8);
    }
    for (uint32_t t = 0; t < 6u; t++)
        for (uint32_t pat = 0; pat < 16u; pat++) {
            uint32_t lo[2] = {0, 0}, hi[2] = {0, 0}, nl = 0, nh = 0;
            for (uint32_t m = 0; m < 4u; m++) {
                if ((pat >> m) & 1u) { if (nl < 2u) lo[nl] = CX_TCH[t][m]; nl++; }
                else { if (nh < 2u) hi[nh] = CX_TCH[t][m]; nh++; }
            }
            T.c22[t * 16u + pat] = (uint16_t)((nl == 2u) ? (lo[0] | (lo[1] << 3) | (hi[0] << 6) | (hi[1] << 9)) : 0u);
        }
    return T;
}
__device__ constexpr cx_pats_tab CX_PATS = cx_make_pats();
union cx_tri_u {
    struct {
        uint16_t slot[12 * 64];  // one word per triangle
        uint32_t tfirst[64];     // first triangle index of each cell minus its rank in the wave
    } a;
    uint32_t hs[8][64];          // low words of the 8 corner hashes of each cell (dead before the slot words are written)
};
struct cx_tri_lds {
    static constexpr bool packed = false;
    uint2 ve[4][7][CX_VE_ROW];   // per wave: (first vertex, crossing mask) of corner c of each cell (rows padded: bank spread)
    cx_tri_u u[4];               // per wave
    uint16_t slot22[4][6 * 64];  // per wave: one word per 2-2 tetrahedron: cell lane | tet << 6 | pattern << 9
    uint32_t var[4][64];         // per wave: quad diagonal variants of each cell (bit t)
    uint32_t lut[6 * 16 * 2 * 2];
    uint2 pats[256];
    uint16_t c22[6 * 16];
};
// the same tables with ONE word per (corner, cell): first vertex relative to one of two bases (bits 0-22; bit 31 picks the base) |
// crossing mask << 23 -- the form the tile kernel keeps per queue entry in LDS (cx_tile3d.h): half the bytes, four workgroups per CU
struct cx_tri_lds_p {
    static constexpr bool packed = true;
    uint32_t ve[4][7][CX_VE_ROW];
    cx_tri_u u[4];
    uint16_t slot22[4][6 * 64];
    uint32_t var[4][64];
    uint32_t lut[6 * 16 * 2 * 2];
    uint2 pats[256];
    uint16_t c22[6 * 16];
    uint32_t vb[2];              // the two bases
};
template <typename LDS>
__device__ __forceinline__ void cx_tri_lds_init(LDS& L) {
    for (uint32_t x = threadIdx.x; x < 6 * 16 * 2 * 2; x += blockDim.x) L.lut[x] = (&CX_TRI_CD[0][0][0][0])[x];
    for (uint32_t x = threadIdx.x; x < 256u; x += blockDim.x) L.pats[x] = make_uint2(CX_PATS.w[x][0], CX_PATS.w[x][1]);
    for (uint32_t x = threadIdx.x; x < 96u; x += blockDim.x) L.c22[x] = CX_PATS.c22[x];
}
// slot word: bits 0-5 cell lane, 6 second triangle of the entry, 7-14 LUT entry (tet*32 + pattern*2 + variant)

// everything of one cell record that comes from memory.  The loads of record n+1 are issued before
// record n is expanded and are waited for BEFORE the triangle stores of record n are issued:
// `s_waitcnt vmcnt` retires loads and stores in issue order, so a load behind a store waits for the
// store's round trip as well.
struct cx_tri_in {
    uint4 rec;            // cell record (zero: no record)
    uint2 nb[6];          // table entries (first vertex, crossing mask) of corners 1..6
    uint64_t hxy[4];      // CPython hash prefixes of the 4 (i,j) columns of the voxel (CX_DIAG_CPYTHON310 without P.hbytes)
    uint32_t ck;          // k of the cell
    uint32_t hb[4];       // set-order codes of the 8 corners, (k, k+1) pairs of the 4 (i,j) columns (P.hbytes)
};
__device__ __forceinline__ uint32_t cx_need_hash(uint32_t sm, uint32_t tetskip, uint32_t ntri) {
    uint32_t need = 0;   // corners whose hash decides a quad diagonal
#pragma unroll
    for (int t = 0; t < 6; t++) {
        const uint32_t pat = ((sm >> CX_TC[t][0]) & 1u) | (((sm >> CX_TC[t][1]) & 1u) << 1) |
                             (((sm >> CX_TC[t][2]) & 1u) << 2) | (((sm >> CX_TC[t][3]) & 1u) << 3);
        if (ntri && !((tetskip >> t) & 1u) && __popc(pat) == 2) need |= CX_TC_MASK(t);
    }
    return need;
}
__device__ __forceinline__ void cx_tri_fetch(const cx_params& P, const uint64_t* __restrict__ hash_xy, const uint4& rec,
                                             cx_tri_in& I) {
    const uint32_t plane = P.n1 * P.n2;
    I.rec = rec;
    const uint32_t lin = rec.x, sm = rec.y & 0xFFu, tetskip = (rec.y >> 8) & 0x3Fu, ntri = (rec.y >> 16) & 0xFFu;
#pragma unroll
    for (uint32_t c = 1; c < 7; c++) {
        // does corner c own a crossing edge of this voxel?  (a strict superset corner on the other side)
        const uint32_t sc = ((sm >> c) & 1u) ? 0xFFu : 0u;
        uint32_t sup = 0;
#pragma unroll
        for (uint32_t c2 = 0; c2 < 8; c2++) sup |= ((c2 & c) == c && c2 != c) ? (1u << c2) : 0u;
        uint2 pr = make_uint2(0u, 0u);
        if (ntri && ((sm ^ sc) & sup) != 0u) {
            const uint32_t lc = lin + ((c & 4u) ? plane : 0u) + ((c & 2u) ? P.n2 : 0u) + (c & 1u);
            const uint64_t e = P.celltab[lc];
            pr = make_uint2((uint32_t)e, (uint32_t)(e >> 32));
        }
        I.nb[c - 1u] = pr;
    }
    I.ck = 0;
    I.hxy[0] = I.hxy[1] = I.hxy[2] = I.hxy[3] = 0;
    I.hb[0] = I.hb[1] = I.hb[2] = I.hb[3] = 0;
    if (P.hbytes) {
        if (cx_need_hash(sm, tetskip, ntri) != 0u) {   // only voxels: all 8 corners are inside the array
            const uint8_t* __restrict__ hb = P.hbytes + lin;
            uint16_t t0, t1, t2, t3;
            __builtin_memcpy(&t0, hb, 2); __builtin_memcpy(&t1, hb + P.n2, 2);
            __builtin_memcpy(&t2, hb + plane, 2); __builtin_memcpy(&t3, hb + plane + P.n2, 2);
            I.hb[0] = t0; I.hb[1] = t1; I.hb[2] = t2; I.hb[3] = t3;
        }
    } else if ((P.flags & CX_DIAG_CPYTHON310) && cx_need_hash(sm, tetskip, ntri) != 0u) {
        const uint32_t ci = cx_div(lin, P.div_plane);
        const uint32_t r = lin - ci * plane;
        const uint32_t cj = cx_div(r, P.div_row);
        I.ck = r - cj * P.n2;
        // hash prefixes of the 4 (i,j) columns of this voxel (clamped: pseudo cells never need them)
        const uint32_t i1 = min(ci + 1u, P.n0 - 1u), j1 = min(cj + 1u, P.n1 - 1u);
        I.hxy[0] = hash_xy[ci * P.n1 + cj]; I.hxy[1] = hash_xy[ci * P.n1 + j1];
        I.hxy[2] = hash_xy[i1 * P.n1 + cj]; I.hxy[3] = hash_xy[i1 * P.n1 + j1];
    }
}
// the loads behind I (and the next record) have to be complete here
__device__ __forceinline__ void cx_tri_pin(cx_tri_in& I, uint4& nxt) {
    asm volatile("" : "+v"(I.rec.x), "+v"(I.rec.y), "+v"(I.rec.z), "+v"(I.rec.w), "+v"(nxt.x), "+v"(nxt.y), "+v"(nxt.z), "+v"(nxt.w) :: "memory");
    asm volatile("" : "+v"(I.nb[0].x), "+v"(I.nb[0].y), "+v"(I.nb[1].x), "+v"(I.nb[1].y), "+v"(I.nb[2].x), "+v"(I.nb[2].y) :: "memory");
    asm volatile("" : "+v"(I.nb[3].x), "+v"(I.nb[3].y), "+v"(I.nb[4].x), "+v"(I.nb[4].y), "+v"(I.nb[5].x), "+v"(I.nb[5].y) :: "memory");
    asm volatile("" : "+v"(I.hxy[0]), "+v"(I.hxy[1]), "+v"(I.hxy[2]), "+v"(I.hxy[3]), "+v"(I.ck) :: "memory");
    asm volatile("" : "+v"(I.hb[0]), "+v"(I.hb[1]), "+v"(I.hb[2]), "+v"(I.hb[3]) :: "memory");
}

// phase 1 of one record per lane: LDS tables and slot words; returns the wave's triangle count
// NEG_ORIGIN: the array starts at a negative lattice point (rim of extra samples): signed hash lanes.  A kernel of its
// own, because the extra path costs the common one ~9 % when it is a run-time branch (registers, code size)
//
// The triangle kernels are bound by VALU issue, so everything that depends on the corner sign mask
// alone comes from a table (CX_PATS: the 6 tetrahedron patterns, which tetrahedra split 2-2 / 1-3, which neighbour cells own an
// edge of the voxel), and the CPython set order of the quad diagonals is decided one lane per 2-2 TETRAHEDRON instead of six
// predicated tetrahedra per cell lane: a voxel has 1.7 of them on average, so two rounds of 64 lanes replace six unrolled
// hash comparisons per lane.  The corner hashes (low words) of a round's cells go through LDS (hs), overlaying the slot
// words, which are written afterwards.
// SLIM: the wave's 64 lanes hold the slim records 64 g .. 64 g + 63 (cx_store_cell_record) and rec.z / rec.w the group's
// {first triangle, first vertex}: a record's own two numbers are those plus the prefixes of ntri and popc(emask) inside the wave
// (lanes behind the last record hold zeros, at the wave's end)
template <bool NEG_ORIGIN, bool SLIM = false, typename LDS>
__device__ __forceinline__ uint32_t cx_tri_phase1(const cx_params& P, LDS& L, uint32_t lane, uint32_t wave, const cx_tri_in& I) {
    const uint32_t sm = I.rec.y & 0xFFu, tetskip = (I.rec.y >> 8) & 0x3Fu, ntri = (I.rec.y >> 16) & 0xFFu;
    if constexpr (SLIM) {
        static_assert(!LDS::packed, "slim records: the record-walking kernel of the staged pipeline");
        uint32_t vtot;
        const uint32_t vpre = cx_wave_prefix_small<3>(__popc(I.rec.y >> 24), vtot);
        L.ve[wave][0][lane] = make_uint2(I.rec.w + vpre, I.rec.y >> 24);
#pragma unroll
        for (uint32_t c = 1; c < 7; c++) L.ve[wave][c][lane] = I.nb[c - 1u];
    } else if constexpr (LDS::packed) {     // rec.w and nb[].x carry the packed words as they are
        L.ve[wave][0][lane] = I.rec.w;
#pragma unroll
        for (uint32_t c = 1; c < 7; c++) L.ve[wave][c][lane] = I.nb[c - 1u].x;
    } else {
        L.ve[wave][0][lane] = make_uint2(I.rec.w, I.rec.y >> 24);
#pragma unroll
        for (uint32_t c = 1; c < 7; c++) L.ve[wave][c][lane] = I.nb[c - 1u];
    }
    const uint2 pw = L.pats[sm];                                  // x: 6 patterns x 4 bits | 2-2 mask << 24; y: 1-3 mask | wanted neighbours << 8
    const uint32_t em6 = ntri ? (~tetskip & 0x3Fu) : 0u;          // tetrahedra that emit
    const uint32_t m22 = (pw.x >> 24) & em6, m1 = pw.y & em6;
    // quad diagonal variants of the 2-2 tetrahedra (bit t of `variants`)
    uint32_t variants = 0;
    if (P.hbytes) {
        // code of corner c = byte (c & 1) of column c >> 1
#pragma unroll
        for (int t = 0; t < 6; t++) {
            const uint32_t pat = (pw.x >> (4 * t)) & 15u;
            if (!((m22 >> t) & 1u)) continue;
            uint32_t l0 = 0, l1 = 0, h0 = 0, h1 = 0;
            int nl = 0, nh = 0;
#pragma unroll
            for (int m = 0; m < 4; m++) {
                const uint32_t cc = CX_TC[t][m];
                const uint32_t code = (I.hb[cc >> 1] >> (8u * (cc & 1u))) & 0xFFu;
                if ((pat >> m) & 1u) { if (nl == 0) l0 = code; else l1 = code; nl++; }
                else { if (nh == 0) h0 = code; else h1 = code; nh++; }
            }
            if (cx_set2_swapped(l0, l1) != cx_set2_swapped(h0, h1)) variants |= 1u << t;
        }
    } else if ((P.flags & CX_DIAG_CPYTHON310) && __ballot(m22 != 0u) != 0ULL) {
        // (k + origin) * P2 of the tuple hash's last round for k and k + 1 (as CPython sees the lattice coordinate: hash(-1) == -2)
        uint64_t kp0, kp1;
        if (!NEG_ORIGIN) {
            kp0 = (uint64_t)(I.ck + P.org2) * CX_PY_P2;
            kp1 = kp0 + CX_PY_P2;
        } else {
            const int32_t v0 = (int32_t)I.ck + (int32_t)P.org2, v1 = v0 + 1;
            kp0 = ((v0 == -1) ? ~1ULL : (uint64_t)(int64_t)v0) * CX_PY_P2;
            kp1 = ((v1 == -1) ? ~1ULL : (uint64_t)(int64_t)v1) * CX_PY_P2;
        }
        bool exact;
        {
            // Fast form: only the LOW 32 bits of the corner hashes -- a probe step of the set order reads three bits five places
            // further up, so five steps fit.  A pair still on one slot after five steps, or a hash word of all ones (possibly
            // the hash CPython replaces by a constant), sends the whole wave through the 64-bit form below.
            bool bad = false;
            uint32_t (*hs)[64] = L.u[wave].hs;
#pragma unroll
            for (uint32_t c = 0; c < 8; c++) {
                const uint64_t sacc = I.hxy[c >> 1] + ((c & 1u) ? kp1 : kp0);
                const uint32_t rot = __builtin_amdgcn_alignbit((uint32_t)sacc, (uint32_t)(sacc >> 32), 1);   // low word of rotl64(s, 31)
                const uint32_t h = rot * (uint32_t)CX_PY_P1 + (uint32_t)(3ULL ^ (CX_PY_P5 ^ 3527539ULL));
                bad = bad || (h == 0xFFFFFFFFu);
                hs[c][lane] = h;
            }
            bad = bad && m22 != 0u;
            L.var[wave][lane] = 0u;
            uint32_t tot22;
            const uint32_t pre22 = cx_wave_prefix_small<3>(__popc(m22), tot22);
#pragma unroll
            for (uint32_t t = 0; t < 6; t++)
                if ((m22 >> t) & 1u)
                    L.slot22[wave][pre22 + __popc(m22 & ((1u << t) - 1u))] = (uint16_t)(lane | (t << 6) | (((pw.x >> (4u * t)) & 15u) << 9));
            __builtin_amdgcn_wave_barrier();
            for (uint32_t j0 = 0; j0 < tot22; j0 += 64u) {   // wave-uniform: one lane per 2-2 tetrahedron
                const uint32_t j = j0 + lane;
                const bool ok = j < tot22;
                const uint32_t w = L.slot22[wave][ok ? j : 0u];
                const uint32_t cell = w & 63u, t = (w >> 6) & 7u;
                const uint32_t cc = L.c22[(t << 4) | (w >> 9)];   // corners of the low pair and of the high pair, 3 bits each
                bool u1, u2;
                const bool a = py_set2_swapped_lo(hs[cc & 7u][cell], hs[(cc >> 3) & 7u][cell], u1);
                const bool b = py_set2_swapped_lo(hs[(cc >> 6) & 7u][cell], hs[(cc >> 9) & 7u][cell], u2);
                if (ok && a != b) atomicOr(&L.var[wave][cell], 1u << t);
                bad = bad || (ok && (u1 || u2));
            }
            __builtin_amdgcn_wave_barrier();
            variants = L.var[wave][lane];
            exact = __ballot(bad) != 0ULL;
        }
        if (exact) {
            variants = 0;
            uint64_t h[8];
#pragma unroll
            for (uint32_t c = 0; c < 8; c++) h[c] = py_finish3(py_round_tail(I.hxy[c >> 1] + ((c & 1u) ? kp1 : kp0)));
#pragma unroll
            for (int t = 0; t < 6; t++) {
                if (!((m22 >> t) & 1u)) continue;
                const uint32_t pat = (pw.x >> (4 * t)) & 15u;
                // low set and high set, each in insertion (tet vertex) order
                uint64_t hl0 = 0, hl1 = 0, hh0 = 0, hh1 = 0;
                int nl = 0, nh = 0;
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    const uint64_t hm = h[CX_TC[t][m]];
                    if ((pat >> m) & 1u) { if (nl == 0) hl0 = hm; else hl1 = hm; nl++; }
                    else { if (nh == 0) hh0 = hm; else hh1 = hm; nh++; }
                }
                if (py_set2_swapped(hl0, hl1) != py_set2_swapped(hh0, hh1)) variants |= 1u << t;
            }
        }
        __builtin_amdgcn_wave_barrier();   // hs is dead: the slot words below overlay it
    }
    // slot words of this cell's triangles, in tetrahedron order
    uint32_t ttot;
    const uint32_t tpre = cx_wave_prefix_small<4>(ntri, ttot);
    L.u[wave].a.tfirst[lane] = SLIM ? I.rec.z : I.rec.z - tpre;   // triangle j of the wave goes to tfirst[cell] + j
    uint32_t pos = tpre;
    uint16_t* slot = L.u[wave].a.slot;
#pragma unroll
    for (uint32_t t = 0; t < 6; t++) {
        const uint32_t two = (m22 >> t) & 1u, one = (m1 >> t) & 1u;
        const uint32_t word = lane | (t << 12) | (((pw.x >> (4u * t)) & 15u) << 8) | (((variants >> t) & 1u) << 7);
        if (two | one) slot[pos] = (uint16_t)word;
        if (two) slot[pos + 1u] = (uint16_t)(word | (1u << 6));
        pos += 2u * two + one;
    }
    __builtin_amdgcn_wave_barrier();
    return ttot;
}
// phase 2, one lane per triangle: stores only
template <typename LDS>
__device__ __forceinline__ void cx_tri_phase2(const cx_params& P, LDS& L, uint32_t lane, uint32_t wave, uint32_t ttot) {
    for (uint32_t j0 = 0; j0 < ttot; j0 += 64u) {   // wave-uniform
        const uint32_t j = j0 + lane;
        const bool ok = j < ttot;
        const uint32_t w = L.u[wave].a.slot[ok ? j : 0u];
        const uint32_t cell = w & 63u;
        const uint32_t tw = L.lut[((w >> 7) & 0xFFu) * 2u + ((w >> 6) & 1u)];
        int32_t vi[3];
#pragma unroll
        for (uint32_t sidx = 0; sidx < 3; sidx++) {
            const uint32_t cd = (tw >> (6u * sidx)) & 63u;
            if constexpr (LDS::packed) {
                const uint32_t wd = L.ve[wave][cd & 7u][cell];
                vi[sidx] = (int32_t)(L.vb[wd >> 31] + (wd & 0x7FFFFFu) + __popc(((wd >> 23) & 0xFEu) & ((1u << (cd >> 3)) - 1u)));
            } else {
                const uint2 pr = L.ve[wave][cd & 7u][cell];
                vi[sidx] = (int32_t)(pr.x + __popc(pr.y & ((1u << (cd >> 3)) - 1u)));
            }
        }
        if (ok) {
            // 32-bit wrap-around on purpose: tfirst = first - rank may be "negative" when the wave's cells come from
            // different reservations (generic path); the sum is the triangle index again
            int32_t* out = P.tris + (size_t)(uint32_t)(L.u[wave].a.tfirst[cell] + j) * 3u;
            typedef int32_t cx_v3i __attribute__((ext_vector_type(3)));
            __builtin_nontemporal_store(cx_v3i{vi[0], vi[1], vi[2]}, reinterpret_cast<cx_v3i*>(out));
        }
    }
    __builtin_amdgcn_wave_barrier();
}

// the cell records are read once: nontemporal loads (against plain loads: ~1.5 %, within noise)
__device__ __forceinline__ uint2 cx_load_record2(const uint2* p) {   // a slim record
    const cx_v2u v = __builtin_nontemporal_load(reinterpret_cast<const cx_v2u*>(p));
    return make_uint2(v.x, v.y);
}
__device__ __forceinline__ uint4 cx_load_record(const uint4* p) {
    typedef uint32_t cx_v4u __attribute__((ext_vector_type(4)));
    const cx_v4u v = __builtin_nontemporal_load(reinterpret_cast<const cx_v4u*>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}
// one lane per cell record; waves walk the record array grid-stride (the record count lives on the device)
#ifndef CX_K2_MIN_WAVES
#define CX_K2_MIN_WAVES 1
#endif
template <bool NEG_ORIGIN>
__global__ __launch_bounds__(256, CX_K2_MIN_WAVES) void cx_k_emit_triangles(const cx_params P, const uint64_t* __restrict__ hash_xy) {
    __shared__ cx_tri_lds L;
    const uint32_t ncells = min(P.counters[CX_CNT_CELLS], P.ccap);
    if (P.counters[CX_CNT_TRIS] > P.tcap || P.counters[CX_CNT_VERTS] > P.vcap) return;  // host re-runs with more room
    // (Records are taken in launch order.  Measured and dropped, third session of round 4: every XCD taking ONE contiguous eighth of each
    // stride -- workgroup b -> block (b % 8) * (grid / 8) + b / 8 --, so that the queue / info words of neighbour cells come from the XCD's
    // own L2 more often: 0.126 -> 0.136 ms, 0.330 -> 0.340-0.345 ms per step.)
    if (blockIdx.x * blockDim.x >= ncells) return;                 // whole block idle
    cx_tri_lds_init(L);
    __syncthreads();
    const uint32_t lane = cx_lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t stride = gridDim.x * blockDim.x;
    uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    const uint4 zero = make_uint4(0, 0, 0, 0);
    cx_tri_in Ia, Ib;
    cx_tri_fetch(P, hash_xy, (idx < ncells) ? cx_load_record(P.cells + idx) : zero, Ia);
    uint4 rec_b = (idx + stride < ncells) ? cx_load_record(P.cells + idx + stride) : zero;
    cx_tri_pin(Ia, rec_b);          // nothing is in flight when the loop is entered
    while (idx - lane < ncells) {   // wave-uniform
        const uint32_t nidx = idx + stride;
        cx_tri_fetch(P, hash_xy, rec_b, Ib);                                    // loads of the next record ...
        uint4 rec_c = (nidx + stride < ncells) ? cx_load_record(P.cells + nidx + stride) : zero;   // ... and the record after it
        const uint32_t ttot = cx_tri_phase1<NEG_ORIGIN>(P, L, lane, wave, Ia);
        cx_tri_pin(Ib, rec_c);                                                  // ... are back before the stores go out
        cx_tri_phase2(P, L, lane, wave, ttot);
        Ia = Ib;
        rec_b = rec_c;
        idx = nidx;
    }
}

// =================================================================================================
// K2 for the staged pipeline: the same triangle stage, but the (first vertex, crossing mask) pairs of the neighbour cells come
// from the vertex stage's word per QUEUE ENTRY (P.info64) instead of a table of one entry per sample.  The queue entry of
// any active lattice cell Y is found by arithmetic: the stream kernel left, per plane step and streaming lane, the queue
// position of the lane's first active cell and the 16-bit set of its active cells (P.qa), so
//     entry(Y) = wave(Y) * wcap + (qa >> 16) + popc(qa & cells below Y).
// Both tables are dense where they are used: a round of 64 records touches a few cache lines per lookup instead of one per
// cell and neighbour (the vector L1 handles about one line per 3-4 cycles per CU whatever the bytes asked for: these kernels
// are bound by the NUMBER of lines their gathers and scatters touch, not by bytes -- DESIGN.md section 4).
// Three records are in flight per lane: record s+2 has its queue words requested, record s+1 its info words, record s is
// expanded and stored.
// =================================================================================================
static_assert(CX_RJ == 4, "the wave / row arithmetic below assumes 4 rows per streaming wave");
struct cx_tri_qa {          // a record between its first stage (queue words requested) and its second
    uint4 rec;
    uint32_t qa[6];         // per neighbour cell X + c, c = 1..6: the queue word of its streaming lane and plane step, as loaded
    uint32_t geo;           // bits 0-5: neighbour c is wanted (bit c-1); 6: X + dk is in the next k block; 7: X + dj in the next wave;
                            // 8: X + di in the next chunk of planes; 9-10: row of X in its wave; 11-12: sample of X in its lane
    uint32_t w;             // streaming wave of the cell
    uint32_t ij, ck;        // (i * n1 + j) and k of the cell's lattice point
};
// byte-offset loads with a 32-bit offset from a uniform base (global_load with an SGPR base and a VGPR offset: no 64-bit
// address arithmetic per lane); the tables they read are smaller than 4 GiB
__device__ __forceinline__ uint32_t cx_ld_u32_at(const uint32_t* base, uint32_t byte_off) {
    return *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(base) + byte_off);
}
// a cell at lattice point (ci, cj, ck) = plane step ps of streaming wave w (row rr of its 4, lane ls, sample mm): request the queue
// words of the neighbour cells that own an edge of its voxel
__device__ __forceinline__ void cx_triq_issue(const cx_params& P, const cx_task& T, const cx_tri_lds& L, const uint4& rec, uint32_t w, uint32_t ci,
                                              uint32_t cj, uint32_t ck, uint32_t ps, uint32_t nsteps, cx_tri_qa& A) {
    A.rec = rec;
    const uint32_t sm = rec.y & 0xFFu, ntri = (rec.y >> 16) & 0xFFu;
    const uint32_t rr = cj & 3u, ls = (ck >> 2) & 63u, mm = ck & 3u;
    const uint32_t wv = w & 3u;
    A.w = w;
    const bool m3 = (mm == 3u), r3 = (rr == 3u), pl = (ps + 1u == nsteps);
    const bool kfl = m3 && ls == 63u;
    // neighbour cells that own a crossing edge of this voxel (bit c), from the table
    const uint32_t want = ntri ? ((L.pats[sm].y >> 9) & 0x3Fu) : 0u;
    A.geo = want | (kfl ? 64u : 0u) | (r3 ? 128u : 0u) | (pl ? 256u : 0u) | (rr << 9) | (mm << 11);
    A.ij = ci * P.n1 + cj; A.ck = ck;
    // word index of the queue word of X + c in P.qa = [wave][plane step][lane]: a sum of one term per axis.  The neighbour
    // is in the same lane word unless X is in the last sample column (next lane, or lane 0 of the next k block), the last
    // row (next wave, or the first wave of the next block in j) or the last plane step (the next chunk of planes)
    constexpr uint32_t WQ = CX_SWP * 64u;
    const uint32_t bk1 = kfl ? 4u * WQ : (m3 ? ls + 1u : ls);
    const uint32_t bj1 = r3 ? ((wv == 3u) ? (4u * T.nks - 3u) * WQ : WQ) : 0u;
    const uint32_t bp0 = ps << 6, bp1 = pl ? 4u * T.nks * T.njg * WQ : ((ps + 1u) << 6);
    const uint32_t base = A.w * WQ;
    const uint32_t B0 = base + bp0, B1 = base + bp1, B0j = B0 + bj1, B1j = B1 + bj1;
    const uint32_t idx[6] = {B0 + bk1, B0j + ls, B0j + bk1, B1 + ls, B1 + bk1, B1j + ls};
#pragma unroll
    for (uint32_t c = 0; c < 6; c++) {
        A.qa[c] = 0;
        if ((want >> c) & 1u) A.qa[c] = cx_ld_u32_at(P.qa, idx[c] << 2);
    }
}
// ... of a cell record (the record-walking kernel): the lattice point from its linear index
__device__ __forceinline__ void cx_triq_stage1(const cx_params& P, const cx_task& T, const cx_tri_lds& L, const uint4& rec,
                                               cx_tri_qa& A) {
    const uint32_t plane = P.n1 * P.n2;
    const uint32_t lin = rec.x;
    const uint32_t ci = cx_div(lin, P.div_plane);
    const uint32_t rem = lin - ci * plane;
    const uint32_t cj = cx_div(rem, P.div_row);
    const uint32_t ck = rem - cj * P.n2;
    // where the cell sits in the streaming layout
    const uint32_t ic = cx_div(ci, P.div_ci);
    const uint32_t ps = ci - ic * T.ci;
    const uint32_t nsteps = min(T.ci, P.n0 - ic * T.ci);
    const uint32_t w = 4u * ((ck >> 8) + T.nks * ((cj >> 4) + T.njg * ic)) + ((cj >> 2) & 3u);
    cx_triq_issue(P, T, L, rec, w, ci, cj, ck, ps, nsteps, A);
}
// ... of a queue entry e of streaming wave w with its info word iw (the entry-walking kernel): the tile from the wave's number,
// the position in the tile from the entry; tfirst = number of the cell's first triangle
__device__ __forceinline__ void cx_trie_stage1(const cx_params& P, const cx_task& T, const cx_tri_lds& L, uint32_t e, uint64_t iw, uint32_t w,
                                               uint32_t tfirst, cx_tri_qa& A) {
    const uint32_t b = w >> 2;
    const uint32_t t1 = cx_div(b, T.div_nks);
    const uint32_t ks = b - t1 * T.nks;
    const uint32_t ic = cx_div(t1, T.div_njg);
    const uint32_t jg = t1 - ic * T.njg;
    const uint32_t p = ic * T.ci;
    const uint32_t bit = (e >> 10) & 31u;
    const uint32_t rr = (bit * 11u) >> 6;
    const uint32_t ps = (e >> 21) & 127u;
    const uint32_t ci = p + ps, cj = jg * (4u * CX_RJ) + (w & 3u) * CX_RJ + rr, ck = ks * 256u + 4u * ((e >> 15) & 63u) + (bit - 6u * rr);
    const uint32_t hi = (uint32_t)(iw >> 32);
    // the cell's record as the later stages read it: {-, signs | tetskip << 8 | triangles << 16 | crossing mask << 24, first triangle, first vertex}
    const uint4 rec = make_uint4(0u, cx_entry_signs(e) | (((hi >> 12) & 0x3Fu) << 8) | (((hi >> 8) & 0xFu) << 16) | ((hi & 0xFFu) << 24), tfirst, (uint32_t)iw);
    cx_triq_issue(P, T, L, rec, w, ci, cj, ck, ps, min(T.ci, P.n0 - p), A);
}
__device__ __forceinline__ void cx_triq_pin1(cx_tri_qa& A, uint4& nxt) {
    asm volatile("" : "+v"(nxt.x), "+v"(nxt.y), "+v"(nxt.z), "+v"(nxt.w) :: "memory");
    asm volatile("" : "+v"(A.qa[0]), "+v"(A.qa[1]), "+v"(A.qa[2]), "+v"(A.qa[3]), "+v"(A.qa[4]), "+v"(A.qa[5]) :: "memory");
}
__device__ __forceinline__ void cx_triq_stage2(const cx_params& P, const cx_task& T, const uint64_t* __restrict__ hash_xy, const cx_tri_qa& A,
                                               cx_tri_in& I) {
    I.rec = A.rec;
    // queue entry of X + c = first entry of its wave + (queue position of its lane's first cell) + active cells of the lane below it
    const bool kfl = (A.geo >> 6) & 1u, r3 = (A.geo >> 7) & 1u, pl = (A.geo >> 8) & 1u;
    const uint32_t rr = (A.geo >> 9) & 3u, mm = (A.geo >> 11) & 3u;
    const uint32_t qk1 = kfl ? 4u * T.wcap : 0u;
    const uint32_t qj1 = r3 ? (((A.w & 3u) == 3u) ? (4u * T.nks - 3u) * T.wcap : T.wcap) : 0u;
    const uint32_t qp1 = pl ? 4u * T.nks * T.njg * T.wcap : 0u;
    const uint32_t Q0 = A.w * T.wcap, Q1 = Q0 + qp1, Q0j = Q0 + qj1, Q1j = Q1 + qj1;
    const uint32_t qb[6] = {Q0 + qk1, Q0j, Q0j + qk1, Q1, Q1 + qk1, Q1j};
    // bit of X + c in its lane's 16-bit set of active cells (bit 4r + m)
    const uint32_t b00 = 4u * rr + mm, b01 = 4u * rr + ((mm + 1u) & 3u), b10 = 4u * ((rr + 1u) & 3u) + mm, b11 = 4u * ((rr + 1u) & 3u) + ((mm + 1u) & 3u);
    const uint32_t bit[6] = {b01, b10, b11, b00, b01, b10};
#pragma unroll
    for (uint32_t c = 0; c < 6; c++) {
        uint2 pr = make_uint2(0u, 0u);
        if ((A.geo >> c) & 1u) {
            const uint32_t qa = A.qa[c];
            const uint32_t below = qa & ((1u << bit[c]) - 1u);     // bit[c] <= 15: only bits of the 16-bit set
            const uint32_t at = qb[c] + (qa >> 16) + __popc(below);
            const uint64_t e = P.info64[at];
            pr = make_uint2((uint32_t)e, (uint32_t)(e >> 32));   // (bits above the crossing mask ride along: phase 2 only looks below bit 8.  No arithmetic on the loaded word here -- it would put a wait behind every gather)
        }
        I.nb[c] = pr;
    }
    I.ck = A.ck;
    I.hb[0] = I.hb[1] = I.hb[2] = I.hb[3] = 0;
    I.hxy[0] = I.hxy[1] = I.hxy[2] = I.hxy[3] = 0;
    const uint32_t sm = A.rec.y & 0xFFu, tetskip = (A.rec.y >> 8) & 0x3Fu, ntri = (A.rec.y >> 16) & 0xFFu;
    if ((P.flags & CX_DIAG_CPYTHON310) && cx_need_hash(sm, tetskip, ntri) != 0u) {
        // only voxels get here (cj + 1 < n1, ci + 1 < n0): the prefixes of columns (i, j), (i, j+1) are neighbours in the
        // table, ONE 16-byte load per plane (8-byte aligned)
        struct __attribute__((packed, aligned(8))) u64x2 { uint64_t a, b; };
        const u64x2 p0 = *reinterpret_cast<const u64x2*>(hash_xy + A.ij);
        const u64x2 p1 = *reinterpret_cast<const u64x2*>(hash_xy + (A.ij + P.n1));
        I.hxy[0] = p0.a; I.hxy[1] = p0.b; I.hxy[2] = p1.a; I.hxy[3] = p1.b;
    }
}
__device__ __forceinline__ void cx_triq_pin2(cx_tri_in& I) {
    asm volatile("" : "+v"(I.hxy[0]), "+v"(I.hxy[1]), "+v"(I.hxy[2]), "+v"(I.hxy[3]) :: "memory");
    asm volatile("" : "+v"(I.nb[0].x), "+v"(I.nb[0].y), "+v"(I.nb[1].x), "+v"(I.nb[1].y), "+v"(I.nb[2].x), "+v"(I.nb[2].y) :: "memory");
    asm volatile("" : "+v"(I.nb[3].x), "+v"(I.nb[3].y), "+v"(I.nb[4].x), "+v"(I.nb[4].y), "+v"(I.nb[5].x), "+v"(I.nb[5].y) :: "memory");
}
#ifndef CX_K2Q_MIN_WAVES
#define CX_K2Q_MIN_WAVES 5   // 96 registers: one more wave per SIMD than the allocator takes on its own (98)
#endif
template <bool NEG_ORIGIN, bool SLIM>   // SLIM: 8-byte records + P.cbase (cx_store_cell_record); else the 16-byte records (cx_extract3d_levels)
__global__ __launch_bounds__(256, CX_K2Q_MIN_WAVES) void cx_k_emit_triangles_q(const cx_params P, const cx_task T, const uint64_t* __restrict__ hash_xy) {
    __shared__ cx_tri_lds L;
    const uint32_t ncells = min(P.counters[CX_CNT_CELLS], P.ccap);
    if (P.counters[CX_CNT_TRIS] > P.tcap || P.counters[CX_CNT_VERTS] > P.vcap) return;  // host re-runs with more room
    if (SLIM && P.counters[CX_CNT_CELLS] > P.ccap) return;   // ... here too: the last 64-group's records and its P.cbase slot may not all be there
    // (Records are taken in launch order.  Measured and dropped, third session of round 4: every XCD taking ONE contiguous eighth of each
    // stride -- workgroup b -> block (b % 8) * (grid / 8) + b / 8 --, so that the queue / info words of neighbour cells come from the XCD's
    // own L2 more often: 0.126 -> 0.136 ms, 0.330 -> 0.340-0.345 ms per step.)
    if (blockIdx.x * blockDim.x >= ncells) return;                 // whole block idle
    cx_tri_lds_init(L);
    __syncthreads();
    const uint32_t lane = cx_lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t stride = gridDim.x * blockDim.x;
    uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    const uint4 zero = make_uint4(0, 0, 0, 0);
    // A record is requested three steps before it is expanded -- UNCONDITIONALLY (from a clamped index) and without touching the
    // result: written as `(at < ncells) ? load : zero`, the load sat in a branch whose result the compiler copied into other
    // registers right behind it, i.e. every iteration began by waiting for the record it had just asked for.  Whether the record
    // exists is decided when it is used (`valid`).
    // Slim: the 8-byte record and, in its z / w, the {first triangle, first vertex} of its group of 64 -- one wave-uniform 8-byte load
    // per iteration (a wave's 64 records are one group: idx - lane is a multiple of 64), requested with the record
    auto record = [&](uint32_t at) {
        const uint32_t c = min(at, ncells - 1u);
        if constexpr (SLIM) {
            const uint2 r = cx_load_record2(reinterpret_cast<const uint2*>(P.cells) + c);
            const uint2 b = P.cbase[__builtin_amdgcn_readfirstlane(c >> 6)];
            return make_uint4(r.x, r.y, b.x, b.y);
        } else {
            return cx_load_record(P.cells + c);
        }
    };
    auto valid = [&](const uint4& r, uint32_t at) { return (at < ncells) ? r : zero; };
    // prologue: record idx through both stages, record idx + stride through the first, record idx + 2 stride loaded
    cx_tri_qa Ab, Ac;
    cx_tri_in Ia, Ib;
    uint4 rec_c = record(idx + 2u * stride);
    {
        uint4 r0 = record(idx), r1 = record(idx + stride);
        asm volatile("" : "+v"(r0.x), "+v"(r0.y), "+v"(r0.z), "+v"(r0.w), "+v"(r1.x), "+v"(r1.y), "+v"(r1.z), "+v"(r1.w) :: "memory");
        cx_triq_stage1(P, T, L, valid(r0, idx), Ac);
        cx_triq_stage1(P, T, L, valid(r1, idx + stride), Ab);
        cx_triq_pin1(Ac, rec_c);
        cx_triq_pin1(Ab, rec_c);
        cx_triq_stage2(P, T, hash_xy, Ac, Ia);
        cx_triq_pin2(Ia);
    }
    while (idx - lane < ncells) {   // wave-uniform
        const uint32_t nidx = idx + stride;
        uint4 rec_d = record(nidx + 2u * stride);          // the record three steps ahead
        cx_triq_stage1(P, T, L, valid(rec_c, nidx + stride), Ac);   // queue words of the record two steps ahead
        cx_triq_stage2(P, T, hash_xy, Ab, Ib);              // info words (and hash prefixes) of the next record
        const uint32_t ttot = cx_tri_phase1<NEG_ORIGIN, SLIM>(P, L, lane, wave, Ia);
        cx_tri_phase2(P, L, lane, wave, ttot);
        cx_triq_pin1(Ac, rec_d);                            // ... waited for after the stores went out
        cx_triq_pin2(Ib);
        Ia = Ib;
        Ab = Ac;
        rec_c = rec_d;
        idx = nidx;
    }
}

// =================================================================================================
// K2 walking QUEUE ENTRIES (cx_k_emit_triangles_e, the default of the staged pipeline from round 3 on).  The vertex stage no longer
// writes a 16-byte record per cell for this kernel to read back (128 MB of round trip at 512^3): everything a record held is in
// the cell's queue entry (signs, position in its streaming wave's tile) and in the word the vertex stage leaves per entry (first
// vertex, crossing mask, triangles, tolerance skips), and the number of a cell's first triangle follows from a running count --
// triangles are numbered along the flat batch list, cell after cell.
// Work division as in the vertex stage: wave m takes rounds [m q, m q + q) of the flat batch list (P.rstart: the batch its share
// starts in) and, where that is inside a batch, counts the triangles of the rounds before (info words; a batch on the tolerance
// path is not divided).  Unlike the vertex stage it PACKS its cells: a round of 64 lanes is filled across batch boundaries
// (up to four pieces), so only the last round of a wave's share is partial -- this kernel is bound by VALU issue per round.
// Three rounds are in flight per wave, as in the record-walking kernel: round s+3 has its entries and info words requested,
// round s+2 its queue words, round s+1 the neighbours' info words (and hash prefixes), round s is expanded and stored.
// =================================================================================================
// a descriptor of the flat batch list, its fields made wave-uniform for the compiler (the address is)
__device__ __forceinline__ cx_bdesc cx_desc_uniform(const cx_bdesc& D) {
    cx_bdesc U;
    U.w = __builtin_amdgcn_readfirstlane(D.w); U.qofs = __builtin_amdgcn_readfirstlane(D.qofs); U.n = __builtin_amdgcn_readfirstlane(D.n);
    U.vbase = 0; U.cbase = 0; U.p = 0; U.j0 = 0; U.k0 = 0; U.nsteps = 0;      // (not used by the triangle stage)
    U.tbase = __builtin_amdgcn_readfirstlane(D.tbase);
    U.near = __builtin_amdgcn_readfirstlane(D.near); U.rbase = __builtin_amdgcn_readfirstlane(D.rbase);
    return U;
}
struct cx_esrc {              // wave-uniform: where the next round's cells come from
    uint32_t f, nbatches, lo, hi; // current batch, batches in the list, the wave's share (rounds)
    uint32_t at, bend;        // entries [at, bend) of the current batch are still to be handed out
    uint32_t qofs, w;         // of the current batch
    uint32_t bend_round;      // round behind the current batch
    uint32_t tbase;           // first triangle of the current batch
    cx_bdesc next;            // descriptor f + 1, requested when batch f was entered (as loaded: made uniform when it is entered)
    bool done;
};
// entries [r0 * 64, end) of batch D belong to the wave whose share of rounds is [lo, hi): a batch on the tolerance path goes as a
// whole to the wave in whose share its first round falls.  Requests the descriptor after it.
__device__ __forceinline__ void cx_esrc_enter(const cx_params& P, cx_esrc& S, const cx_bdesc& Draw) {
    const cx_bdesc D = cx_desc_uniform(Draw);
    const uint32_t nrb = (D.n + 63u) >> 6;
    const uint32_t r0 = max(S.lo, D.rbase) - D.rbase, r1 = min(S.hi, D.rbase + nrb) - D.rbase;
    S.qofs = D.qofs; S.w = D.w; S.bend_round = D.rbase + nrb; S.tbase = D.tbase;
    if (D.near) { S.at = 0u; S.bend = (r0 == 0u) ? D.n : 0u; }
    else { S.at = r0 * 64u; S.bend = min(D.n, r1 * 64u); }
    if (S.f + 1u < S.nbatches) S.next = P.flat[S.f + 1u];
}
// the batch in hand is used up (or was not ours): on to the next one of the share, if any
__device__ __forceinline__ void cx_esrc_advance(const cx_params& P, cx_esrc& S) {
    while (S.at >= S.bend && !S.done) {
        if (S.bend_round >= S.hi || S.f + 1u >= S.nbatches) { S.done = true; break; }
        S.f++;
        cx_esrc_enter(P, S, S.next);
    }
}
struct cx_eraw {              // per lane: a cell of a round as it comes from memory
    uint32_t e, w;            // queue entry, streaming wave (0xFFFFFFFF: no cell in this lane)
    uint64_t iw;              // the vertex stage's word
};
// hand out the next (up to) 64 cells and request their entries and info words.  Four rounds in five come whole out of the batch
// in hand; the others take its tail and the head of the next batch (a next batch shorter than the gap leaves lanes empty).
__device__ __forceinline__ void cx_esrc_fetch(const cx_params& P, cx_esrc& S, uint32_t lane, cx_eraw& R) {
    R.w = 0xFFFFFFFFu; R.e = 0; R.iw = 0;
    if (S.done) return;                            // wave-uniform
    uint32_t at, w;
    bool have;
    if (S.at + 64u <= S.bend) {                    // wave-uniform
        at = S.qofs + S.at + lane; w = S.w; have = true;
        S.at += 64u;
    } else {
        const uint32_t c0 = S.bend - S.at, pos0 = S.qofs + S.at, w0 = S.w;
        S.at = S.bend;
        cx_esrc_advance(P, S);
        uint32_t c1 = 0, pos1 = 0, w1 = 0;
        if (!S.done) {
            c1 = min(S.bend - S.at, 64u - c0); pos1 = S.qofs + S.at; w1 = S.w;
            S.at += c1;
        }
        have = lane < c0 + c1;
        at = (lane < c0) ? pos0 + lane : pos1 + (lane - c0);
        w = (lane < c0) ? w0 : w1;
    }
    if (have) { R.w = w; R.e = P.queue[at]; R.iw = P.info64[at]; }
}
__device__ __forceinline__ void cx_eraw_pin(cx_eraw& R) { asm volatile("" : "+v"(R.e), "+v"(R.iw) :: "memory"); }

#ifndef CX_K2E_MIN_WAVES
#define CX_K2E_MIN_WAVES 4
#endif
template <bool NEG_ORIGIN>
__global__ __launch_bounds__(256, CX_K2E_MIN_WAVES) void cx_k_emit_triangles_e(const cx_params P, const cx_task T, const uint64_t* __restrict__ hash_xy) {
    __shared__ cx_tri_lds L;
    if (P.counters[CX_CNT_TRIS] > P.tcap || P.counters[CX_CNT_VERTS] > P.vcap) return;  // host re-runs with more room
    const uint32_t nbatches = min(P.counters[CX_CNT_BATCHES], P.fcap);
    const uint32_t rounds = P.counters[CX_CNT_ROUNDS];
    cx_tri_lds_init(L);
    __syncthreads();
    const uint32_t lane = cx_lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nkw = gridDim.x * 4u;     // == P.nkw
    const uint32_t share = max((rounds + nkw - 1u) / nkw, CX_S3_MIN_SHARE);
    const uint32_t lo = (blockIdx.x * 4u + wave) * share;
    if (lo >= rounds || nbatches == 0u) return;
    cx_esrc S;
    S.lo = lo; S.hi = min(rounds, lo + share); S.nbatches = nbatches; S.done = false;
    S.f = __builtin_amdgcn_readfirstlane(P.kstart[blockIdx.x * 4u + wave]);
    if (S.f >= nbatches) return;
    uint32_t run_t;      // number of the first triangle of the next round's first cell (wave-uniform)
    {
        const cx_bdesc D = P.flat[S.f];
        cx_esrc_enter(P, S, D);
        run_t = S.tbase;
        if (S.at) {   // the share starts inside this batch (never one on the tolerance path): the triangles of the cells before
            const uint64_t* __restrict__ iw = P.info64 + S.qofs;
            uint32_t t = 0;
            for (uint32_t x = lane; x < S.at; x += 64u) t += (uint32_t)(iw[x] >> 40) & 0xFu;
            run_t += cxd_wave_add(t);
        }
        if (S.at >= S.bend) {
            // the first batch of the share is on the tolerance path and belongs to the wave before: numbering is contiguous along
            // the list, so the first batch actually taken sets the count (it is taken from its first cell)
            cx_esrc_advance(P, S);
            if (S.done) return;
            run_t = S.tbase;
        }
    }
    // a round between its request and its first stage
    auto first_triangles = [&](const cx_eraw& R, uint32_t& tfirst) {
        // triangles are numbered cell after cell along the flat batch list
        const uint32_t nt = (R.w != 0xFFFFFFFFu) ? ((uint32_t)(R.iw >> 40) & 0xFu) : 0u;
        uint32_t ttot;
        const uint32_t tpre = cx_wave_prefix_small<4>(nt, ttot);
        tfirst = run_t + tpre;
        run_t += ttot;
    };
    cx_tri_qa Ab, Ac;
    cx_tri_in Ia, Ib;
    cx_eraw Rc, Rd;
    uint4 dummy = make_uint4(0, 0, 0, 0);
    auto stage1 = [&](const cx_eraw& R, cx_tri_qa& A) {
        uint32_t tfirst;
        first_triangles(R, tfirst);
        if (R.w != 0xFFFFFFFFu) cx_trie_stage1(P, T, L, R.e, R.iw, R.w, tfirst, A);
        else { A.rec = make_uint4(0, 0, 0, 0); A.geo = 0; A.w = 0; A.ij = 0; A.ck = 0; for (int c = 0; c < 6; c++) A.qa[c] = 0; }
    };
    // prologue: round 0 through both stages, round 1 through the first, round 2 requested
    {
        cx_eraw R0, R1;
        cx_esrc_fetch(P, S, lane, R0);
        cx_esrc_fetch(P, S, lane, R1);
        cx_esrc_fetch(P, S, lane, Rc);
        cx_eraw_pin(R0); cx_eraw_pin(R1);
        stage1(R0, Ac);
        stage1(R1, Ab);
        cx_triq_pin1(Ac, dummy);
        cx_triq_pin1(Ab, dummy);
        cx_triq_stage2(P, T, hash_xy, Ac, Ia);
        cx_triq_pin2(Ia);
        cx_eraw_pin(Rc);
    }
    // the loop ends when the round being expanded holds no cell: the source hands out full rounds until it is exhausted (only the
    // last one may be partial), then empty ones
    for (;;) {
        if (__ballot(Ia.rec.y != 0u) == 0ULL) break;         // (every queued cell has a sign change: its sign word is not 0)
        cx_esrc_fetch(P, S, lane, Rd);                   // entries and info words of the round three steps ahead
        stage1(Rc, Ac);                                      // queue words of the round two steps ahead
        cx_triq_stage2(P, T, hash_xy, Ab, Ib);               // info words (and hash prefixes) of the next round
        const uint32_t ttot = cx_tri_phase1<NEG_ORIGIN>(P, L, lane, wave, Ia);
        cx_tri_phase2(P, L, lane, wave, ttot);
        cx_triq_pin1(Ac, dummy); cx_triq_pin2(Ib); cx_eraw_pin(Rd);
        Ia = Ib;
        Ab = Ac;
        Rc = Rd;
    }
}
