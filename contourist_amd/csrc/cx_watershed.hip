// cx_watershed.hip -- marker-based watershed of a volume (include/contourist_hip.h, section "watershed"): every sample of the domain gets
// the label of the marker whose flood wets it first, by the arrival cost W = (P, d) of the header: P the level at which the flood
// reaches the sample, d the steps since that level was entered (Meyer's flooding with first-in first-out lakes, as a path cost).
//
// Nothing is computed but comparisons of keys and counts of steps.  Every sample becomes a key whose unsigned order is the header's
// order (cx_dev.h: cxd_sample_key), zero-extended to 32 bits; CX_WATERSHED_FALLING runs the same kernels on the keys complemented in
// their own width.  `words` holds one 64-bit word per sample, key << 32 | d:
//     CXW_OUTSIDE   (all ones)      the sample is outside the domain (outside the region, or NaN): never read as a source, never written
//     CXW_UNREACHED (all ones - 1)  inside the domain, no flood has arrived yet
//     anything else                 an arrival cost; a marker sample holds (key, 0) from cxw_k_init on
// d < 2^31 (a path has fewer steps than the array has samples, at most 2^31), so word + 1 never carries into the key and no cost
// collides with the two sentinels.  Two sentinels instead of one let the round kernel tell the domain from the word alone: it reads
// neither the region nor the NaN test again.
// The fixed point.  step(U, v) = (key(v), 0) if key(v) > U.P, else U + 1; W is the unique fixed point of
//     W(v) = min(W(v), min over the neighbours u of step(W(u), v))
// with the marker samples held at (key, 0).  (key(v), 0) is the least cost any path can bring to v, so holding the markers takes no
// flag: no step ever lowers them.
//
// A workgroup of 256 threads owns a tile of CXW_T0 x CXW_T1 x CXW_T2 = 8 x 8 x 64 samples (cxw_k_round).  It stages the words of the tile
// and a halo of one sample (10 x 10 x 66 x 8 B = 52,800 bytes, CXW_OUTSIDE outside the array) in LDS; a thread keeps the keys of its 16
// samples (lane = position on axis 2, 16 rows) in registers.  One sweep relaxes every sample of the tile once from all its 6, 18 or 26
// neighbours, in place, the rows ascending on even sweeps and descending on odd ones; threads read each other's words while they are
// written (see below).  Sweeps repeat until a workgroup-wide OR says that nothing moved, at most CXW_TILE + 1 times: a cost reaches a
// sample along a path of at most CXW_TILE steps inside the tile, and every sweep advances it by one step at least.  (A tile still
// moving at the bound -- no correct run gets there -- puts itself on the list again.)
//
// Rounds.  One launch per round over the list of active tiles; round 0 visits every tile.  A tile that lowered a sample writes its
// interior back with plain 8-byte stores and puts on the next round's list the neighbour tiles in whose halo a lowered sample lies (a
// flag word per tile and round parity, claimed by atomicExch, so a tile is listed once; one atomicAdd per visited tile appends the
// claims of a wave).  The host reads the counters after every CXW_BATCH launches and stops when the next list is empty.
//
// Why the order does not matter (section 9r's argument with the order reversed).  (1) Every word ever stored is
// at or above the true W of its sample and words only ever decrease: step is monotone in the neighbour's word, so an upper bound of
// W(u) steps to an upper bound of W(v), the marker words are exact, and an update is a minimum with the old word.  (2) A word is one
// aligned 8-byte access, in global memory and in LDS, which does not tear: a racing read returns some word that was stored, so some
// upper bound.  So a stale halo, or a stale read inside a sweep, can only leave a sample ABOVE its fixed point, never below it or at a
// wrong one.  (3) The neighbour that stored the lower word lowered a sample of its shell, so it lists this tile for the next round,
// whose launch boundary makes the word visible.  When no tile is listed every tile has seen the final halo and is at its fixed point:
// the whole array is at the fixed point, which is unique.  No workgroup waits for another: no grid barrier, no flag is polled, no
// kernel is persistent.
//
// Labels.  cxw_k_parent: a marker sample points to itself, every other reached sample to the neighbour with the least (W, index) -- the
// neighbours are visited in C order and replaced only by a strictly lower word -- and an unreached one holds CXW_NONE.  The pointers
// lie in the result buffer.  cxw_k_jump doubles them in place, parent[v] = parent[parent[v]]: a word only ever moves to an ancestor,
// a 4-byte read returns some ancestor, and parent[p] == p holds for roots only and for ever, so "a pass changed nothing" means every
// sample points at its root.  A chain has fewer than 2^31 links: at most CXW_JUMPS = 32 passes.  cxw_k_label writes markers[root].
//
// Every loop is bounded: the sweeps by CXW_TILE + 1, the rounds by the number of samples + 8 (not by the number of tiles: a winding
// corridor crosses the same tile face many times, but a path without repeats has fewer steps than the array has samples), the doubling
// passes by CXW_JUMPS.  Past a bound the call returns CX_ERR_HIP.
#include <cstring>
#include <new>
#include <utility>

#include "cx_dev.h"
#include "cx_gridop.h"

#define CXW_T0 8
#define CXW_T1 8
#define CXW_T2 64
#define CXW_H1 (CXW_T1 + 2)
#define CXW_H2 (CXW_T2 + 2)
#define CXW_TILE (CXW_T0 * CXW_T1 * CXW_T2)                         // 4096 samples
#define CXW_HALO ((CXW_T0 + 2) * CXW_H1 * CXW_H2)                   // 6600 words
#define CXW_PER_THREAD (CXW_TILE / 256)                             // 16 samples of a thread
#define CXW_BATCH 4u                                                // launches between two reads of the counters
#define CXW_GRID 4096u                                              // workgroups of a round whose list the host has not read
#define CXW_PASS_GRID 2048u                                         // workgroups of the per-sample passes (a counter add per wave)
#define CXW_JUMPS 32u                                               // doubling passes at most
#define CXW_OUTSIDE 0xFFFFFFFFFFFFFFFFULL
#define CXW_UNREACHED 0xFFFFFFFFFFFFFFFEULL
#define CXW_NONE 0xFFFFFFFFu

struct cxw_counters {          // 96 bytes, zeroed before every call
    uint32_t cnt[3];           // tiles on the list of round r: cnt[r % 3]
    uint32_t pad;
    uint32_t jump[3];          // pointers that doubling pass j moved: jump[j % 3]
    uint32_t pad2;
    u64 visits, rounds;        // tiles visited, launches that visited one
    u64 jump_rounds;           // doubling passes that ran
    u64 n_markers, n_ignored, n_labelled, n_unreached;
    u64 pad3;
};

struct cx_watershed_state : cx_slot {      // (`in`: a host relief; `result`: the labels, and the parent pointers before them)
    cx_buf<uint8_t> in2, in3;  // host markers, a host region
    cx_buf<u64> words;         // an arrival cost per sample
    cx_buf<uint32_t> work;     // two lists and two flag arrays of one word per tile
    cx_buf<uint8_t> counters;  // cxw_counters
    cx_buf<uint8_t> prev;      // the result of the call before, where that is an input of this call
};

void cx_watershed_free(cx_ctx* ctx) {
    delete ctx->watershed;
    ctx->watershed = nullptr;
}

struct cxw_args {
    const void* relief;
    const int32_t* markers;
    const uint8_t* region;               // or null
    u64* words;
    uint32_t* parent;                    // the result buffer
    uint32_t* list[2];
    uint32_t* flags[2];
    cxw_counters* C;
    int64_t n[3];
    uint32_t g[3], tiles;                // tiles per axis and in all
    int32_t dtype, conn, falling;
    uint32_t esize, ones;                // bytes of a sample, the all-ones key of that width
    uint32_t round, first;
};

__device__ __forceinline__ uint32_t cxw_raw(const void* p, uint32_t esize, size_t i) {
    if (esize == 1u) return static_cast<const uint8_t*>(p)[i];
    if (esize == 2u) return static_cast<const uint16_t*>(p)[i];
    return static_cast<const uint32_t*>(p)[i];
}
__device__ __forceinline__ bool cxw_is_float(int32_t dtype) { return dtype == CX_DTYPE_F32 || dtype == CX_DTYPE_F16 || dtype == CX_DTYPE_BF16; }

// the cost a neighbour's word U brings to a sample with working key k (kk = k << 32); a sentinel brings a sentinel
__device__ __forceinline__ u64 cxw_step(u64 U, uint32_t k, u64 kk) {
    if (U >= CXW_UNREACHED) return CXW_OUTSIDE;
    return k > (uint32_t)(U >> 32) ? kk : U + 1ULL;
}

// the domain and the markers: the first words, n_markers and n_ignored
__global__ __launch_bounds__(256) void cxw_k_init(const cxw_args A) {
    const size_t total = (size_t)A.n[0] * (size_t)A.n[1] * (size_t)A.n[2];
    const uint32_t flip = A.falling ? A.ones : 0u;
    const bool fl = cxw_is_float(A.dtype);
    long long n_markers = 0, n_ignored = 0;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < total; i += (size_t)gridDim.x * 256u) {
        const uint32_t key = cxd_sample_key(A.dtype, cxw_raw(A.relief, A.esize, i));
        const bool inside = (!A.region || A.region[i] != 0) && !(fl && key == A.ones);      // (NaN: on the sample, before the complement)
        const bool marked = A.markers[i] > 0;
        u64 w = inside ? CXW_UNREACHED : CXW_OUTSIDE;
        if (marked && inside) { w = (u64)(key ^ flip) << 32; n_markers++; }
        else if (marked) n_ignored++;
        A.words[i] = w;
    }
    n_markers = cxd_wave_add(n_markers);
    n_ignored = cxd_wave_add(n_ignored);
    if ((threadIdx.x & 63u) == 0u) {
        if (n_markers) atomicAdd(&A.C->n_markers, (u64)n_markers);
        if (n_ignored) atomicAdd(&A.C->n_ignored, (u64)n_ignored);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) A.C->cnt[0] = A.tiles;
}

extern __shared__ __align__(16) unsigned char cxw_smem[];

// where a sample of the tile lies on the tile's shell, per axis 0 = low face, 1 = inside, 2 = high face: bit (c0 3 + c1) 3 + c2
__device__ __forceinline__ uint32_t cxw_class(uint32_t d0, uint32_t d1, uint32_t d2) {
    const uint32_t c0 = d0 == 0u ? 0u : (d0 == CXW_T0 - 1u ? 2u : 1u), c1 = d1 == 0u ? 0u : (d1 == CXW_T1 - 1u ? 2u : 1u), c2 = d2 == 0u ? 0u : (d2 == CXW_T2 - 1u ? 2u : 1u);
    return 1u << ((c0 * 3u + c1) * 3u + c2);
}

// sample j of a thread: row (tid >> 6) + 4 j of the tile's 64 rows, position lane on axis 2.  Its word lowered from its CONN-neighbours
// in LDS; true if it moved
template <int CONN>
__device__ __forceinline__ bool cxw_relax(u64* V, uint32_t pos, uint32_t k) {
    const u64 kk = (u64)k << 32, old = V[pos];
    u64 best = old;
#pragma unroll
    for (int o0 = -1; o0 <= 1; o0++)
#pragma unroll
        for (int o1 = -1; o1 <= 1; o1++)
#pragma unroll
            for (int o2 = -1; o2 <= 1; o2++) {
                const int nz = (o0 != 0) + (o1 != 0) + (o2 != 0);
                if (nz == 0 || nz > CONN) continue;
                const u64 c = cxw_step(V[(int)pos + (o0 * CXW_H1 + o1) * CXW_H2 + o2], k, kk);
                best = c < best ? c : best;
            }
    if (best == old) return false;
    V[pos] = best;
    return true;
}

// one round: every tile of the list to its fixed point under the halo it finds
template <int CONN>
__global__ __launch_bounds__(256) void cxw_k_round(const cxw_args A) {
    uint32_t* head = reinterpret_cast<uint32_t*>(cxw_smem);      // [0]: the classes of the samples this visit lowered
    u64* V = reinterpret_cast<u64*>(cxw_smem + 16);              // words [10][10][66]
    u64* words = A.words;
    cxw_counters* C = A.C;
    const uint32_t r = A.round, n_active = min(C->cnt[r % 3u], A.tiles);      // (a tile is listed once: never more than all of them)
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t flip = A.falling ? A.ones : 0u;
    if (blockIdx.x == 0 && tid == 0) {
        C->cnt[(r + 2u) % 3u] = 0u;      // the list after the next one: nobody reads or appends to it in this launch
        C->visits += n_active;
        if (n_active) C->rounds += 1ull;
    }
    uint32_t* list_next = A.list[(r + 1u) & 1u];
    uint32_t* flags_next = A.flags[(r + 1u) & 1u];
    for (uint32_t it = blockIdx.x; it < n_active; it += gridDim.x) {
        const uint32_t tile = A.first ? it : A.list[r & 1u][it];
        if (tile >= A.tiles) continue;      // (never: the lists hold tile numbers)
        const uint32_t t2 = tile % A.g[2], t01 = tile / A.g[2], t1 = t01 % A.g[1], t0 = t01 / A.g[1];
        const int64_t b0 = (int64_t)t0 * CXW_T0, b1 = (int64_t)t1 * CXW_T1, b2 = (int64_t)t2 * CXW_T2;
        for (uint32_t e = tid; e < CXW_HALO; e += 256u) {
            const uint32_t row = e / CXW_H2, h2 = e - row * CXW_H2, h0 = row / CXW_H1, h1 = row - h0 * CXW_H1;
            const int64_t i0 = b0 + (int64_t)h0 - 1, i1 = b1 + (int64_t)h1 - 1, i2 = b2 + (int64_t)h2 - 1;
            u64 w = CXW_OUTSIDE;
            if (i0 >= 0 && i0 < A.n[0] && i1 >= 0 && i1 < A.n[1] && i2 >= 0 && i2 < A.n[2]) w = words[((size_t)i0 * (size_t)A.n[1] + (size_t)i1) * (size_t)A.n[2] + (size_t)i2];
            V[e] = w;
        }
        if (tid == 0) head[0] = 0u;
        __syncthreads();
        // the thread's 16 samples: their working keys, and which of them lie in the domain (what lies outside the array holds CXW_OUTSIDE)
        uint32_t key[CXW_PER_THREAD];
        uint32_t dom = 0u;
#pragma unroll
        for (int j = 0; j < CXW_PER_THREAD; j++) {
            const uint32_t d0 = (uint32_t)j >> 1, d1 = wave + 4u * ((uint32_t)j & 1u);
            key[j] = 0u;
            if (V[((d0 + 1u) * CXW_H1 + d1 + 1u) * CXW_H2 + lane + 1u] != CXW_OUTSIDE) {
                const size_t i = ((size_t)(b0 + d0) * (size_t)A.n[1] + (size_t)(b1 + d1)) * (size_t)A.n[2] + (size_t)(b2 + lane);
                key[j] = cxd_sample_key(A.dtype, cxw_raw(A.relief, A.esize, i)) ^ flip;
                dom |= 1u << j;
            }
        }
        uint32_t cls = 0u;
        int moving = __syncthreads_or(dom != 0u);      // a tile without a sample of the domain has nothing to sweep
        for (uint32_t sweep = 0; sweep <= CXW_TILE && moving; sweep++) {
            int ch = 0;
            if (!(sweep & 1u)) {
#pragma unroll
                for (int j = 0; j < CXW_PER_THREAD; j++) {
                    const uint32_t d0 = (uint32_t)j >> 1, d1 = wave + 4u * ((uint32_t)j & 1u);
                    if (((dom >> j) & 1u) && cxw_relax<CONN>(V, ((d0 + 1u) * CXW_H1 + d1 + 1u) * CXW_H2 + lane + 1u, key[j])) { ch = 1; cls |= cxw_class(d0, d1, lane); }
                }
            } else {
#pragma unroll
                for (int j = CXW_PER_THREAD - 1; j >= 0; j--) {
                    const uint32_t d0 = (uint32_t)j >> 1, d1 = wave + 4u * ((uint32_t)j & 1u);
                    if (((dom >> j) & 1u) && cxw_relax<CONN>(V, ((d0 + 1u) * CXW_H1 + d1 + 1u) * CXW_H2 + lane + 1u, key[j])) { ch = 1; cls |= cxw_class(d0, d1, lane); }
                }
            }
            moving = __syncthreads_or(ch);
        }
        if (cls) atomicOr(&head[0], cls);
        __syncthreads();
        const uint32_t lowered = head[0];
        if (lowered) {
            for (uint32_t e = tid; e < CXW_TILE; e += 256u) {
                const uint32_t d0 = e >> 9, d1 = (e >> 6) & 7u, d2 = e & 63u;
                const int64_t i0 = b0 + d0, i1 = b1 + d1, i2 = b2 + d2;
                if (i0 < A.n[0] && i1 < A.n[1] && i2 < A.n[2])
                    words[((size_t)i0 * (size_t)A.n[1] + (size_t)i1) * (size_t)A.n[2] + (size_t)i2] = V[((d0 + 1u) * CXW_H1 + d1 + 1u) * CXW_H2 + d2 + 1u];
            }
        }
        if (wave == 0u) {
            // lane j < 27 speaks for the tile at offset (j / 9 - 1, j / 3 % 3 - 1, j % 3 - 1): listed when a lowered sample lies in its halo
            bool want = false;
            uint32_t nt = 0u;
            if (lane < 27u) {
                const int o0 = (int)(lane / 9u) - 1, o1 = (int)((lane / 3u) % 3u) - 1, o2 = (int)(lane % 3u) - 1;
                const int nz = (o0 != 0) + (o1 != 0) + (o2 != 0);
                if (nz == 0) want = moving != 0;      // still moving at the sweep bound: this tile again
                else if (nz <= CONN) {
                    for (uint32_t c = 0; c < 27u; c++) {
                        const int s0 = (int)(c / 9u) - 1, s1 = (int)((c / 3u) % 3u) - 1, s2 = (int)(c % 3u) - 1;
                        if (((lowered >> c) & 1u) && (o0 == 0 || s0 == o0) && (o1 == 0 || s1 == o1) && (o2 == 0 || s2 == o2)) want = true;
                    }
                }
                const int64_t q0 = (int64_t)t0 + o0, q1 = (int64_t)t1 + o1, q2 = (int64_t)t2 + o2;
                if (q0 < 0 || q0 >= (int64_t)A.g[0] || q1 < 0 || q1 >= (int64_t)A.g[1] || q2 < 0 || q2 >= (int64_t)A.g[2]) want = false;
                else nt = (uint32_t)((q0 * (int64_t)A.g[1] + q1) * (int64_t)A.g[2] + q2);
            }
            const bool won = want && atomicExch(&flags_next[nt], 1u) == 0u;
            const uint64_t winners = __ballot(won);
            if (winners != 0ULL) {      // (wave-uniform)
                const int leader = __ffsll((long long)winners) - 1;
                uint32_t base = 0u;
                if ((int)lane == leader) base = atomicAdd(&C->cnt[(r + 1u) % 3u], (uint32_t)__popcll(winners));
                base = (uint32_t)__shfl((int)base, leader);
                const uint32_t pos = base + (uint32_t)__popcll(winners & ((1ULL << lane) - 1ULL));
                if (won && pos < A.tiles) list_next[pos] = nt;
            }
            if (!A.first && lane == 0u) A.flags[r & 1u][tile] = 0u;      // this round's claim on the tile is spent
        }
        __syncthreads();      // LDS is staged again
    }
}

// a marker sample points to itself, a reached one to its neighbour of least (W, index), an unreached one nowhere
__global__ __launch_bounds__(256) void cxw_k_parent(const cxw_args A) {
    const size_t total = (size_t)A.n[0] * (size_t)A.n[1] * (size_t)A.n[2], plane = (size_t)A.n[1] * (size_t)A.n[2];
    const u64* __restrict__ words = A.words;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < total; i += (size_t)gridDim.x * 256u) {
        const u64 w = words[i];
        uint32_t p = CXW_NONE;
        if (w < CXW_UNREACHED) {
            if (A.markers[i] > 0) p = (uint32_t)i;
            else {
                const int64_t i0 = (int64_t)(i / plane), rest = (int64_t)(i - (size_t)i0 * plane), i1 = rest / A.n[2], i2 = rest - i1 * A.n[2];
                u64 best = w;      // (the fixed point has a neighbour strictly below w)
                for (int o0 = -1; o0 <= 1; o0++)
                    for (int o1 = -1; o1 <= 1; o1++)
                        for (int o2 = -1; o2 <= 1; o2++) {      // ascending linear index: among equals the first one stays
                            const int nz = (o0 != 0) + (o1 != 0) + (o2 != 0);
                            const int64_t q0 = i0 + o0, q1 = i1 + o1, q2 = i2 + o2;
                            if (nz == 0 || nz > A.conn || q0 < 0 || q0 >= A.n[0] || q1 < 0 || q1 >= A.n[1] || q2 < 0 || q2 >= A.n[2]) continue;
                            const size_t q = ((size_t)q0 * (size_t)A.n[1] + (size_t)q1) * (size_t)A.n[2] + (size_t)q2;
                            const u64 u = words[q];
                            if (u < best) { best = u; p = (uint32_t)q; }
                        }
            }
        }
        A.parent[i] = p;
    }
}

// one doubling pass, in place; a pass after one that moved nothing does nothing
__global__ __launch_bounds__(256) void cxw_k_jump(const cxw_args A) {
    const size_t total = (size_t)A.n[0] * (size_t)A.n[1] * (size_t)A.n[2];
    cxw_counters* C = A.C;
    const uint32_t r = A.round;      // the pass modulo 3
    const bool idle = !A.first && C->jump[(r + 2u) % 3u] == 0u;      // (uniform over the launch: the pass before is complete)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        C->jump[(r + 1u) % 3u] = 0u;      // the next pass's count: nobody reads or adds to it in this launch (an idle pass leaves its own at 0)
        if (!idle) C->jump_rounds += 1ull;
    }
    if (idle) return;
    uint32_t* parent = A.parent;
    uint32_t moved = 0u;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < total; i += (size_t)gridDim.x * 256u) {
        const uint32_t p = parent[i];
        if (p == CXW_NONE || p == (uint32_t)i || (size_t)p >= total) continue;
        const uint32_t g = parent[p];
        if (g != p && g != CXW_NONE) { parent[i] = g; moved = 1u; }
    }
    if (__any(moved != 0u) && (threadIdx.x & 63u) == 0u) atomicAdd(&C->jump[r], 1u);
}

// the labels over the pointers, n_labelled and n_unreached
__global__ __launch_bounds__(256) void cxw_k_label(const cxw_args A) {
    const size_t total = (size_t)A.n[0] * (size_t)A.n[1] * (size_t)A.n[2];
    long long n_labelled = 0, n_unreached = 0;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < total; i += (size_t)gridDim.x * 256u) {
        const uint32_t p = A.parent[i];
        int32_t label = 0;
        if (p != CXW_NONE && (size_t)p < total) label = A.markers[p];
        if (label > 0) n_labelled++;
        else label = 0;
        if (A.words[i] == CXW_UNREACHED) n_unreached++;
        A.parent[i] = (uint32_t)label;
    }
    n_labelled = cxd_wave_add(n_labelled);
    n_unreached = cxd_wave_add(n_unreached);
    if ((threadIdx.x & 63u) == 0u) {
        if (n_labelled) atomicAdd(&A.C->n_labelled, (u64)n_labelled);
        if (n_unreached) atomicAdd(&A.C->n_unreached, (u64)n_unreached);
    }
}

static_assert(CXW_T2 == 64 && CXW_T0 * CXW_T1 == 4 * CXW_PER_THREAD && CXW_PER_THREAD <= 32, "a lane per sample of a row; the rows of a tile dealt to four waves");
static_assert(16u + CXW_HALO * 8u <= 65536u, "the LDS of a tile");
static_assert(sizeof(cxw_counters) == 96, "cxw_counters");

static void cxw_launch_round(const cxw_args& A, dim3 grid, hipStream_t st) {
    const size_t lds = 16u + CXW_HALO * sizeof(u64);      // 52,816 bytes: three workgroups per CU
    switch (A.conn) {
        case 1: hipLaunchKernelGGL(cxw_k_round<1>, grid, dim3(256), lds, st, A); break;
        case 2: hipLaunchKernelGGL(cxw_k_round<2>, grid, dim3(256), lds, st, A); break;
        default: hipLaunchKernelGGL(cxw_k_round<3>, grid, dim3(256), lds, st, A); break;
    }
}

extern "C" int cx_grid_watershed3d(cx_ctx* ctx, const void* relief, int32_t dtype, int on_device, int64_t n0, int64_t n1, int64_t n2,
                                   const int32_t* markers, const uint8_t* region, int32_t connectivity, int32_t direction,
                                   void* out_device, void* out_host, cx_watershed_stats* stats) {
    if (!ctx) return CX_ERR_INVALID;
    if (!markers) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_watershed3d: no markers given");
    if (connectivity < 1 || connectivity > 3) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_watershed3d: a connectivity of 1, 2 or 3");
    if (direction != CX_WATERSHED_RISING && direction != CX_WATERSHED_FALLING) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_watershed3d: unknown direction");
    if (((uintptr_t)out_device & 3u) != 0u) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_watershed3d: out_device must be aligned to 4 bytes");
    if (!relief && !ctx->grid.p) return cx_fail(ctx, CX_ERR_STATE, "cx_grid_watershed3d: no relief given and no grid bound");
    cx_source R;
    int rc = cx_source_resolve(ctx, "cx_grid_watershed3d", relief, dtype, on_device, n0, n1, n2, 31, &R, true);
    if (rc) return rc;
    dtype = R.dtype; n0 = R.n[0]; n1 = R.n[1]; n2 = R.n[2]; on_device = R.on_device;      // (markers and region live where the relief does)
    const size_t total = R.count, out_bytes = total * sizeof(int32_t);
    if (on_device && (cx_overlap(R.p, R.bytes, out_device, out_bytes) || cx_overlap(markers, out_bytes, out_device, out_bytes) || cx_overlap(region, total, out_device, out_bytes)))
        return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_watershed3d: the output overlaps an input");
    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_watershed_state* S = cx_state_of(ctx->watershed);
    if (!S) return CX_ERR_NOMEM;
    hipStream_t st = ctx->stream;
    // an input that lies in the result of the call before (its labels as this call's markers): that buffer steps aside into `prev`
    const void* relief_d = R.p;
    const void* markers_d = markers;
    const void* region_d = region;
    if (on_device) {
        S->step_aside(markers, out_bytes, S->prev);
        S->step_aside(R.p, R.bytes, S->prev);
        if (region) S->step_aside(region, total, S->prev);
    } else {
        if ((rc = cx_upload(ctx, S->in, R.p, R.bytes, &relief_d))) return rc;
        if ((rc = cx_upload(ctx, S->in2, markers, out_bytes, &markers_d))) return rc;
        if (region && (rc = cx_upload(ctx, S->in3, region, total, &region_d))) return rc;
    }
    const int64_t g0 = (n0 + CXW_T0 - 1) / CXW_T0, g1 = (n1 + CXW_T1 - 1) / CXW_T1, g2 = (n2 + CXW_T2 - 1) / CXW_T2;
    const size_t tiles = (size_t)g0 * (size_t)g1 * (size_t)g2;      // (<= 2^28: a tile holds eight samples at least, or the whole axis 0)
    void* out;
    if ((rc = S->open(ctx, out_device, out_bytes, &out))) return rc;
    if ((rc = S->words.grow(ctx, total))) return rc;
    if ((rc = S->work.grow(ctx, 4 * tiles))) return rc;
    if ((rc = S->counters.grow(ctx, sizeof(cxw_counters)))) return rc;
    cxw_args A;
    memset(&A, 0, sizeof(A));
    A.relief = relief_d; A.markers = static_cast<const int32_t*>(markers_d); A.region = static_cast<const uint8_t*>(region_d);
    A.words = S->words.get(); A.parent = static_cast<uint32_t*>(out);
    A.list[0] = S->work.get(); A.list[1] = A.list[0] + tiles;
    A.flags[0] = A.list[1] + tiles; A.flags[1] = A.flags[0] + tiles;
    A.C = S->counters.as<cxw_counters>();
    A.n[0] = n0; A.n[1] = n1; A.n[2] = n2;
    A.g[0] = (uint32_t)g0; A.g[1] = (uint32_t)g1; A.g[2] = (uint32_t)g2; A.tiles = (uint32_t)tiles;
    A.dtype = dtype; A.conn = connectivity; A.falling = direction == CX_WATERSHED_FALLING ? 1 : 0;
    A.esize = (uint32_t)cx_dtype_size(dtype);
    A.ones = A.esize == 1u ? 0xFFu : (A.esize == 2u ? 0xFFFFu : 0xFFFFFFFFu);
    CX_HIP(ctx, hipMemsetAsync(S->counters, 0, sizeof(cxw_counters), st));
    CX_HIP(ctx, hipMemsetAsync(A.flags[0], 0, 2 * tiles * sizeof(uint32_t), st));
    const dim3 pass_grid((uint32_t)((total + 255u) / 256u < CXW_PASS_GRID ? (total + 255u) / 256u : CXW_PASS_GRID));
    hipLaunchKernelGGL(cxw_k_init, pass_grid, dim3(256), 0, st, A);
    CX_HIP(ctx, hipGetLastError());
    // the rounds: CXW_BATCH launches, then one look at the counters.  Launches behind the last round that listed a tile find an empty list
    const unsigned long long bound = (unsigned long long)total + 8ull;
    cxw_counters hc;
    for (unsigned long long r = 0;;) {
        for (uint32_t j = 0; j < CXW_BATCH; j++, r++) {
            A.round = (uint32_t)(r % 6ull);      // (the kernel looks at the round modulo 2 and modulo 3)
            A.first = r == 0 ? 1u : 0u;
            cxw_launch_round(A, dim3((uint32_t)(r == 0 ? tiles : (tiles < CXW_GRID ? tiles : CXW_GRID))), st);
            CX_HIP(ctx, hipGetLastError());
        }
        CX_HIP(ctx, hipMemcpyAsync(&hc, S->counters, sizeof(hc), hipMemcpyDeviceToHost, st));
        CX_HIP(ctx, hipStreamSynchronize(st));
        if (hc.cnt[r % 3ull] == 0u) break;
        if (r >= bound) return cx_fail(ctx, CX_ERR_HIP, "cx_grid_watershed3d: tiles still active after as many rounds as the array has samples");
    }
    hipLaunchKernelGGL(cxw_k_parent, pass_grid, dim3(256), 0, st, A);
    CX_HIP(ctx, hipGetLastError());
    // the doubling passes, CXW_BATCH at a time: a pass behind one that moved nothing returns at once
    for (uint32_t j = 0;;) {
        for (uint32_t b = 0; b < CXW_BATCH; b++, j++) {
            A.round = j % 3u;
            A.first = j == 0 ? 1u : 0u;
            hipLaunchKernelGGL(cxw_k_jump, pass_grid, dim3(256), 0, st, A);
            CX_HIP(ctx, hipGetLastError());
        }
        CX_HIP(ctx, hipMemcpyAsync(&hc, S->counters, sizeof(hc), hipMemcpyDeviceToHost, st));
        CX_HIP(ctx, hipStreamSynchronize(st));
        if (hc.jump[(j + 2u) % 3u] == 0u) break;      // the last pass launched moved nothing
        if (j >= CXW_JUMPS) return cx_fail(ctx, CX_ERR_HIP, "cx_grid_watershed3d: labels unresolved after 32 doubling passes");
    }
    hipLaunchKernelGGL(cxw_k_label, pass_grid, dim3(256), 0, st, A);
    CX_HIP(ctx, hipGetLastError());
    CX_HIP(ctx, hipMemcpyAsync(&hc, S->counters, sizeof(hc), hipMemcpyDeviceToHost, st));
    if (out_host) CX_HIP(ctx, hipMemcpyAsync(out_host, out, out_bytes, hipMemcpyDeviceToHost, st));
    CX_HIP(ctx, hipStreamSynchronize(st));      // the caller's host memory is its own again
    if (stats) {
        stats->n_labelled = (int64_t)hc.n_labelled; stats->n_unreached = (int64_t)hc.n_unreached;
        stats->n_ignored = (int64_t)hc.n_ignored; stats->n_markers = (int64_t)hc.n_markers;
        stats->rounds = (int64_t)hc.rounds; stats->tile_visits = (int64_t)hc.visits; stats->jump_rounds = (int64_t)hc.jump_rounds;
    }
    if (!out_device) S->publish(n0, n1, n2);
    return CX_OK;
}

extern "C" int cx_grid_watershed3d_result(cx_ctx* ctx, void** out_device, int64_t out_shape[3]) {
    if (!ctx) return CX_ERR_INVALID;
    return cx_slot_result(ctx, ctx->watershed, "cx_grid_watershed3d_result: no result of cx_grid_watershed3d in the context", out_device, out_shape);
}
