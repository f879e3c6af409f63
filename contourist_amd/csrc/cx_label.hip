// cx_label.hip -- connected components of a thresholded volume (include/contourist_hip.h, section "labels"): cx_grid_label3d, its
// pending labels (cx_grid_label3d_result), their measures (cx_grid_label3d_measures), a mask chosen by label (cx_grid_label3d_select,
// cx_grid_label3d_select_result) and that mask as the bound grid (cx_grid_label3d_bind).
//
// The labels are a pure function of the samples: component c is the one whose smallest linear index is the c-th smallest among the
// components' smallest linear indices.  The union-find of cx_dev.h keeps the smallest index of a set as its root, so once every union
// has been made the roots ARE those smallest indices whatever the order of the unions was, and an exclusive scan of the root flags in
// linear order is the numbering.
//
// Runs, not voxels.  Lanes run along axis 2 and a wave owns a row:
//   cxl_k_rows<DT>  classifies in the sample's own type, one ballot per tile of 64 columns.  The ballot is kept (one bit per sample:
//                   everything after this kernel reads bits, not samples) and every labelled sample gets its first parent: the linear
//                   index of the start of its run in the row, carried across tile boundaries.  A run start is a root.
//   cxl_k_unite     per row and tile the ballots of the row and of each neighbour row that precedes it in C order (same plane j-1;
//                   previous plane j-1, j, j+1; as far as the connectivity admits them).  Where offsets of +-1 along axis 2 are admitted
//                   the neighbour's ballot counts dilated by one, the bits of the tiles beside it carried in.  ONE union per pair of
//                   (run of this row, run of the neighbour row) that touch: the lane at the first column of the contact issues it.
//                   Every access to a parent word in this kernel is a device-scope atomic (cxd_uf_find / cxd_uf_union, cx_dev.h).
//   cxl_k_flatten   every labelled sample points at its root; flag = the sample is a root.  cx_scan_u32 of the flags, in place.
//   cxl_k_relabel   label = rank of the root + 1, written over the parents: the labels buffer held the parents all along.
//   cxl_k_measure   on request.  A wave owns a row of LABELS at a time; a run is one label, its length is bit arithmetic on the ballot.
//                   The runs of a tile are added up per label among the lanes, the wave carries the sums of the label that holds the
//                   majority of what it has seen, and one lane issues integer atomics into a record per group or per wave.
//   cxl_k_select    mask = keep[label], 16 bytes per store where the output is aligned, one count per workgroup.
// Scratch beyond the input and the labels: 4 bytes per sample (flags / ranks) + 1 bit per sample (ballots) + 4 bytes per 1024 samples
// (the scan's block sums).  Integer atomics only: every call gives the same bytes.  DESIGN.md section 9o.
#include <cmath>
#include <cstring>
#include <new>
#include <string>

#include "cx_dev.h"
#include "cx_gridop.h"

#define CXL_WAVES 4u
#define CXL_SELECT_BLOCKS 2048u       // a lane walks its groups of 16 samples with the grid's stride; one count per workgroup
#define CXL_MEASURE_BLOCKS 1024u      // 4 blocks of 4 waves per compute unit: what every wave carries at its end goes to one record in the worst case

struct cx_label_state {
    cx_buf<uint32_t> labels;     // the context's own labels (the parents until cxl_k_relabel)
    cx_buf<uint32_t> rank;       // root flags, then their exclusive scan
    cx_buf<u64> bits;            // one ballot per row and tile
    cx_buf<uint32_t> sums;       // block sums of the scan
    cx_buf<u64> misc;            // [0] K (low word), [1] ones of the last select
    cx_buf<cx_label_component> records;
    cx_buf<uint8_t> keep;        // the caller's keep bytes
    cx_slot mask;                // the host samples of cx_grid_label3d, and the context's own mask (the result of cx_grid_label3d_select)
    int64_t shape[3] = {0, 0, 0};
    int32_t side = 0, connectivity = 0;
    int64_t k = 0;
    bool pending = false;        // `labels` holds the result of the last call
    bool measured = false;       // `records` describes them
    int64_t mask_voxels = 0;
};

void cx_label_free(cx_ctx* ctx) {
    delete ctx->label;
    ctx->label = nullptr;
}

struct cxl_rows_args {
    const void* in;
    uint32_t* parent;
    u64* bits;
    int64_t rows, n2, tiles;
    double value;
    int32_t side;
};

template <int DT>
__global__ __launch_bounds__(256) void cxl_k_rows(const cxl_rows_args A) {
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    const cx_grid_ref G = {A.in, DT};
    const u64 below_me = (1ull << lane) - 1ull;
    for (int64_t row = (int64_t)blockIdx.x * CXL_WAVES + wave; row < A.rows; row += (int64_t)gridDim.x * CXL_WAVES) {
        const size_t base = (size_t)row * (size_t)A.n2;
        int64_t carry = -1;      // the start of the run that reaches the end of the tile before, or none
        for (int64_t t = 0; t < A.tiles; t++) {
            const int64_t k = t * 64 + (int64_t)lane;
            const bool active = k < A.n2;
            const double f = (double)cx_sample<DT>(G, base + (size_t)(active ? k : A.n2 - 1));
            const bool low = f < A.value;
            const u64 m = __ballot(active && (A.side == CX_LABEL_LOW ? low : !low));
            const u64 gaps = ~m & below_me;      // the unlabelled samples of the tile below this lane
            int64_t start = gaps ? t * 64 + 64 - (int64_t)__builtin_clzll(gaps) : (carry >= 0 ? carry : t * 64);
            if (active) A.parent[base + (size_t)k] = ((m >> lane) & 1ull) ? (uint32_t)(base + (size_t)start) : CXD_NONE;
            if (lane == 0u) A.bits[(size_t)row * (size_t)A.tiles + (size_t)t] = m;
            if (m >> 63) {
                const u64 all_gaps = ~m;
                if (all_gaps) carry = t * 64 + 64 - (int64_t)__builtin_clzll(all_gaps);
                else if (carry < 0) carry = t * 64;
            } else carry = -1;
        }
    }
}

struct cxl_unite_args {
    uint32_t* parent;
    const u64* bits;
    int64_t n0, n1, n2, tiles;
    int32_t connectivity;
};

// the unions of one row with one neighbour row, one tile: m, q the ballots, m1 / q1 the ballots moved up by one column (the sample
// below each lane), q2 the neighbour's moved down by one (the sample above)
__device__ __forceinline__ void cxl_contacts(uint32_t* parent, uint32_t me, uint32_t other, uint32_t lane, bool dilated, u64 m, u64 m1, u64 q, u64 q1, u64 q2) {
    if (!dilated) {
        // contact at this column, and not already at the column below
        if (((m & q & ~(m1 & q1)) >> lane) & 1ull) cxd_uf_union(parent, me, other);
        return;
    }
    // a neighbour run S touches this row's run R where R meets S grown by one column; the lane at the first such column issues:
    //   S holds this column: first iff R starts here (else the column below is in R and within S grown)
    //   S starts at the next column: this column is the first
    //   S ends at the column below: first iff R starts here
    if (((m & q & ~m1) >> lane) & 1ull) cxd_uf_union(parent, me, other);
    if (((m & ~q & q2) >> lane) & 1ull) cxd_uf_union(parent, me, other + 1u);
    if (((m & ~q & q1 & ~m1) >> lane) & 1ull) cxd_uf_union(parent, me, other - 1u);
}

__global__ __launch_bounds__(256) void cxl_k_unite(const cxl_unite_args A) {
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    const int64_t rows = A.n0 * A.n1;
    for (int64_t row = (int64_t)blockIdx.x * CXL_WAVES + wave; row < rows; row += (int64_t)gridDim.x * CXL_WAVES) {
        const int64_t i = row / A.n1, j = row % A.n1;
        const u64* __restrict__ mine = A.bits + (size_t)row * (size_t)A.tiles;
        for (int64_t t = 0; t < A.tiles; t++) {
            const u64 m = mine[t];
            if (!m) continue;
            const u64 m1 = (m << 1) | (t > 0 ? mine[t - 1] >> 63 : 0ull);
            const uint32_t me = (uint32_t)((size_t)row * (size_t)A.n2 + (size_t)(t * 64) + lane);
#pragma unroll
            for (int nb = 0; nb < 4; nb++) {
                const int di = nb == 0 ? 0 : -1, dj = nb == 0 ? -1 : nb - 2;      // (0,-1) (-1,-1) (-1,0) (-1,+1)
                const int axes = (di != 0) + (dj != 0);
                if (axes > A.connectivity || i + di < 0 || j + dj < 0 || j + dj >= A.n1) continue;
                const int64_t nrow = row + di * A.n1 + dj;
                const u64* __restrict__ theirs = A.bits + (size_t)nrow * (size_t)A.tiles;
                const u64 q = theirs[t];
                const bool dilated = axes + 1 <= A.connectivity;
                u64 q1 = q << 1, q2 = q >> 1;
                if (t > 0) q1 |= theirs[t - 1] >> 63;
                if (dilated) {
                    if (t + 1 < A.tiles) q2 |= theirs[t + 1] << 63;
                    if (!((q | q1 | q2) & m)) continue;
                } else if (!(q & m)) continue;
                cxl_contacts(A.parent, me, (uint32_t)((size_t)nrow * (size_t)A.n2 + (size_t)(t * 64) + lane), lane, dilated, m, m1, q, q1, q2);
            }
        }
    }
}

// After the uniting kernel has ended its parent words are final and read with plain loads.  A sample's word is rewritten here while
// others may walk through it, but only ever to its root, which every path through it reaches anyway: an old value and the new one lead
// to the same place.  A root stays a root, so the flag does not depend on who is first.
__global__ __launch_bounds__(256) void cxl_k_flatten(uint32_t* parent, uint32_t* flag, uint32_t n) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        uint32_t x = parent[i];
        uint32_t root_flag = 0u;
        if (x != CXD_NONE) {
            root_flag = x == i ? 1u : 0u;
            for (;;) {
                const uint32_t p = parent[x];
                if (p == x) break;
                x = p;
            }
            parent[i] = x;
        }
        flag[i] = root_flag;
    }
}

__global__ __launch_bounds__(256) void cxl_k_relabel(uint32_t* labels, const uint32_t* __restrict__ rank, uint32_t n) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint32_t root = labels[i];
        labels[i] = root == CXD_NONE ? 0u : rank[root] + 1u;
    }
}

__global__ __launch_bounds__(256) void cxl_k_records_init(cx_label_component* rec, uint32_t k) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= k) return;
    cx_label_component r;
    r.voxels = 0; r.first = INT64_MAX;
    for (int a = 0; a < 3; a++) { r.sum[a] = 0; r.lo[a] = INT32_MAX; r.hi[a] = INT32_MIN; }
    r.rim = 0u;
    r.reserved = 0u;
    rec[c] = r;
}

// monotonic extremes with a plain look first (cxd_max64 and its kin, for the record's signed words)
__device__ __forceinline__ void cxl_min_i32(int32_t* addr, int32_t v) {
    if (__hip_atomic_load(addr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= v) return;
    atomicMin(addr, v);
}
__device__ __forceinline__ void cxl_max_i32(int32_t* addr, int32_t v) {
    if (__hip_atomic_load(addr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= v) return;
    atomicMax(addr, v);
}
__device__ __forceinline__ void cxl_min_i64(int64_t* addr, int64_t v) {
    if (__hip_atomic_load(addr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= v) return;
    atomicMin((long long*)addr, (long long)v);
}

struct cxl_measure_args {
    const uint32_t* labels;
    cx_label_component* rec;
    int64_t n0, n1, n2, tiles;
};

// what a wave has added up for one label and not yet put into the record: all of it wave-uniform
struct cxl_part {
    uint32_t label;      // 0: nothing
    int64_t voxels, first, sum[3];
    int32_t lo[3], hi[3];
    uint32_t rim;
};
// the samples of one label in one tile of row (i, j): `len` of them in columns s .. e, their columns summing to sk
__device__ __forceinline__ cxl_part cxl_part_of(const cxl_measure_args& A, uint32_t label, int64_t i, int64_t j, int64_t len, int64_t sk, int64_t s, int64_t e) {
    cxl_part P;
    P.label = label; P.voxels = len; P.first = (i * A.n1 + j) * A.n2 + s;
    P.sum[0] = i * len; P.sum[1] = j * len; P.sum[2] = sk;
    P.lo[0] = P.hi[0] = (int32_t)i; P.lo[1] = P.hi[1] = (int32_t)j; P.lo[2] = (int32_t)s; P.hi[2] = (int32_t)e;
    P.rim = (i == 0 ? 1u : 0u) | (i == A.n0 - 1 ? 2u : 0u) | (j == 0 ? 4u : 0u) | (j == A.n1 - 1 ? 8u : 0u) | (s == 0 ? 16u : 0u) | (e == A.n2 - 1 ? 32u : 0u);
    return P;
}
__device__ __forceinline__ void cxl_part_add(cxl_part& H, const cxl_part& P) {
    H.voxels += P.voxels;
    H.first = P.first < H.first ? P.first : H.first;
    for (int a = 0; a < 3; a++) {
        H.sum[a] += P.sum[a];
        H.lo[a] = P.lo[a] < H.lo[a] ? P.lo[a] : H.lo[a];
        H.hi[a] = P.hi[a] > H.hi[a] ? P.hi[a] : H.hi[a];
    }
    H.rim |= P.rim;
}
// into the record: one lane's integer atomics (the extremes and the rim bits look first)
__device__ __forceinline__ void cxl_part_flush(const cxl_measure_args& A, const cxl_part& P) {
    cx_label_component* r = A.rec + (P.label - 1u);
    atomicAdd((unsigned long long*)&r->voxels, (unsigned long long)P.voxels);
    for (int a = 0; a < 3; a++) {
        if (P.sum[a]) atomicAdd((unsigned long long*)&r->sum[a], (unsigned long long)P.sum[a]);
        cxl_min_i32(&r->lo[a], P.lo[a]);
        cxl_max_i32(&r->hi[a], P.hi[a]);
    }
    cxl_min_i64(&r->first, P.first);
    if (P.rim & ~__hip_atomic_load(&r->rim, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(&r->rim, P.rim);
}

// A wave owns a row of labels at a time and many rows in all.  Per tile the lanes at the starts of runs are grouped by label (all
// the runs of one label in the tile are added up among the lanes), and the group joins what the wave carries for ONE label, chosen by
// majority vote over the voxels seen (Boyer-Moore): a component that fills much of the volume is added up in registers and reaches its
// record once per wave, not once per run -- a record all runs added to directly takes same-address atomics at ~88 per microsecond.
// A group of another label goes to its record at once, from one lane.
__global__ __launch_bounds__(256) void cxl_k_measure(const cxl_measure_args A) {
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    const int64_t rows = A.n0 * A.n1;
    cxl_part H;
    H.label = 0u;
    int64_t votes = 0;
    for (int64_t row = (int64_t)blockIdx.x * CXL_WAVES + wave; row < rows; row += (int64_t)gridDim.x * CXL_WAVES) {
        const int64_t i = row / A.n1, j = row % A.n1;
        const uint32_t* __restrict__ L = A.labels + (size_t)row * (size_t)A.n2;
        for (int64_t t = 0; t < A.tiles; t++) {
            const int64_t k = t * 64 + (int64_t)lane;
            const uint32_t label = k < A.n2 ? L[k] : 0u;
            const u64 m = __ballot(label != 0u);
            if (!m) continue;
            // (two labelled samples side by side in a row are neighbours at every connectivity: a run has one label)
            const bool starts = ((m >> lane) & 1ull) && (lane == 0u || !((m >> (lane - 1u)) & 1ull));
            const u64 rest = ~(m >> lane);      // (zeros move in at the top: only lane 0 of a full tile sees none)
            const int64_t len = rest ? (int64_t)__builtin_ctzll(rest) : 64;
            const int64_t sk = len * k + len * (len - 1) / 2;
            u64 todo = __ballot(starts);
            while (todo) {
                const int leader = (int)__builtin_ctzll(todo);
                const uint32_t gl = (uint32_t)__shfl((int)label, leader);
                const bool mine = starts && label == gl;
                const u64 g = __ballot(mine);
                todo &= ~g;
                const int last = 63 - (int)__builtin_clzll(g);      // the group's runs ascend with the lane
                int64_t glen, gsk;
                if (g & (g - 1ull)) {
                    glen = (int64_t)cxd_wave_add(mine ? (uint32_t)len : 0u);
                    gsk = (int64_t)cxd_wave_add((long long)(mine ? sk : 0));
                } else {
                    glen = (int64_t)__shfl((int)len, leader);
                    gsk = ((int64_t)(uint32_t)__shfl((int)(uint32_t)((u64)sk >> 32), leader) << 32) | (int64_t)(uint32_t)__shfl((int)(uint32_t)(u64)sk, leader);
                }
                const int64_t e = t * 64 + last + (int64_t)__shfl((int)len, last) - 1;
                const cxl_part P = cxl_part_of(A, gl, i, j, glen, gsk, t * 64 + leader, e);
                if (H.label == gl) { cxl_part_add(H, P); votes += glen; }
                else if (votes >= glen) {
                    votes -= glen;
                    if (lane == 0u) cxl_part_flush(A, P);
                } else {
                    if (H.label && lane == 0u) cxl_part_flush(A, H);
                    H = P;
                    votes = glen;
                }
            }
        }
    }
    if (H.label && lane == 0u) cxl_part_flush(A, H);
}

struct cxl_select_args {
    const uint32_t* labels;
    const uint8_t* keep;
    uint8_t* out;
    u64* ones;
    size_t n, head, groups;      // `head` samples in front of the first 16-byte boundary of `out`, then `groups` of 16, then the rest
};

struct __attribute__((packed, aligned(4))) cxl_labels4 { uint32_t x, y, z, w; };

__global__ __launch_bounds__(256) void cxl_k_select(const cxl_select_args A) {
    uint32_t count = 0;
    const size_t tid = (size_t)blockIdx.x * 256u + threadIdx.x, step = (size_t)gridDim.x * 256u;
    for (size_t g = tid; g < A.groups; g += step) {
        const size_t at = A.head + g * 16u;
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const cxl_labels4 l4 = *reinterpret_cast<const cxl_labels4*>(A.labels + at + (size_t)(q * 4));      // (aligned to 4: one 16-byte load)
            const uint32_t l[4] = {l4.x, l4.y, l4.z, l4.w};
            uint32_t v = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const uint32_t one = A.keep[l[b]] ? 1u : 0u;
                v |= one << (8 * b);
                count += one;
            }
            w[q] = v;
        }
        *reinterpret_cast<uint4*>(A.out + at) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    // the samples in front of the first group and behind the last one: fewer than 32
    const size_t tail0 = A.head + A.groups * 16u, loose = A.head + (A.n - tail0);
    if (tid < loose) {
        const size_t at = tid < A.head ? tid : tail0 + (tid - A.head);
        const uint32_t one = A.keep[A.labels[at]] ? 1u : 0u;
        A.out[at] = (uint8_t)one;
        count += one;
    }
    // one add per workgroup (the launch has at most CXL_SELECT_BLOCKS of them: adds to one address run one after the other)
    __shared__ uint32_t per_wave[CXL_WAVES];
    count = cxd_wave_add(count);
    if ((threadIdx.x & 63u) == 0u) per_wave[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0u) {
        const uint32_t total = per_wave[0] + per_wave[1] + per_wave[2] + per_wave[3];
        if (total) atomicAdd(A.ones, (u64)total);
    }
}

static uint32_t cxl_grid_rows(int64_t rows) {
    const unsigned long long blocks = ((unsigned long long)rows + CXL_WAVES - 1u) / CXL_WAVES;
    return (uint32_t)(blocks < (1ull << 20) ? (blocks ? blocks : 1ull) : (1ull << 20));
}
static uint32_t cxl_grid_flat(size_t n) {
    const size_t blocks = (n + 255u) / 256u;
    return (uint32_t)(blocks < (1u << 20) ? (blocks ? blocks : 1u) : (1u << 20));
}

extern "C" int cx_grid_label3d(cx_ctx* ctx, const void* samples, int32_t dtype, int on_device, int64_t n0, int64_t n1, int64_t n2,
                               double value, int32_t side, int32_t connectivity, int32_t* out_device, int32_t* out_host, int64_t* n_components) {
    if (!ctx) return CX_ERR_INVALID;
    if (!std::isfinite(value)) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_label3d: value is NaN or infinite");
    if (side != CX_LABEL_HIGH && side != CX_LABEL_LOW) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_label3d: unknown side");
    if (connectivity < 1 || connectivity > 3) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_label3d: connectivity is 1, 2 or 3");
    cx_source S;
    int rc = cx_source_resolve(ctx, "cx_grid_label3d", samples, dtype, on_device, n0, n1, n2, 29, &S);
    if (rc) return rc;
    n0 = S.n[0]; n1 = S.n[1]; n2 = S.n[2];
    const size_t count = S.count, out_bytes = count * sizeof(int32_t);
    if (out_device && S.on_device && cx_overlap(S.p, S.bytes, out_device, out_bytes)) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_label3d: the output overlaps the input");
    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_label_state* L = cx_state_of(ctx->label);
    if (!L) return CX_ERR_NOMEM;
    hipStream_t st = ctx->stream;
    const void* dev = S.p;      // (the labels are no buffer a caller's samples can lie in: nothing steps aside)
    if (!S.on_device && (rc = cx_upload(ctx, L->mask.in, S.p, S.bytes, &dev))) return rc;
    L->pending = false;      // the labels of this call, or none: a caller's output leaves nothing to hand out or measure
    L->measured = false;
    uint32_t* parent = reinterpret_cast<uint32_t*>(out_device);
    if (!out_device) {
        if ((rc = L->labels.grow(ctx, count))) return rc;
        parent = L->labels.get();
    }
    const int64_t rows = n0 * n1, tiles = (n2 + 63) / 64;
    if ((rc = L->rank.grow(ctx, count)) || (rc = L->bits.grow(ctx, (size_t)(rows * tiles))) || (rc = L->sums.grow(ctx, count / 1024u + 2u)) ||
        (rc = L->misc.grow(ctx, 2)))
        return rc;
    cxl_rows_args R;
    memset(&R, 0, sizeof(R));
    R.in = dev; R.parent = parent; R.bits = L->bits.get();
    R.rows = rows; R.n2 = n2; R.tiles = tiles; R.value = value; R.side = side;
#define CX_LAUNCH(DT) hipLaunchKernelGGL((cxl_k_rows<DT>), dim3(cxl_grid_rows(rows)), dim3(256), 0, st, R);
    CX_DISPATCH_DTYPE(S.dtype, CX_LAUNCH)
#undef CX_LAUNCH
    CX_HIP(ctx, hipGetLastError());
    cxl_unite_args U;
    memset(&U, 0, sizeof(U));
    U.parent = parent; U.bits = L->bits.get(); U.n0 = n0; U.n1 = n1; U.n2 = n2; U.tiles = tiles; U.connectivity = connectivity;
    hipLaunchKernelGGL(cxl_k_unite, dim3(cxl_grid_rows(rows)), dim3(256), 0, st, U);
    CX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(cxl_k_flatten, dim3(cxl_grid_flat(count)), dim3(256), 0, st, parent, L->rank.get(), (uint32_t)count);
    CX_HIP(ctx, hipGetLastError());
    uint32_t* total = reinterpret_cast<uint32_t*>(L->misc.get());
    if ((rc = cx_scan_u32(ctx, L->rank, L->rank, (uint32_t)count, L->sums, total))) return rc;      // (in place: a thread reads its four words before it writes them)
    CX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(cxl_k_relabel, dim3(cxl_grid_flat(count)), dim3(256), 0, st, parent, (const uint32_t*)L->rank.get(), (uint32_t)count);
    CX_HIP(ctx, hipGetLastError());
    uint32_t k = 0;
    CX_HIP(ctx, hipMemcpyAsync(&k, total, sizeof(k), hipMemcpyDeviceToHost, st));
    if (out_host) CX_HIP(ctx, hipMemcpyAsync(out_host, parent, out_bytes, hipMemcpyDeviceToHost, st));
    CX_HIP(ctx, hipStreamSynchronize(st));      // K is the caller's, and its host memory is its own again
    if (!out_device) {
        L->shape[0] = n0; L->shape[1] = n1; L->shape[2] = n2;
        L->side = side; L->connectivity = connectivity; L->k = (int64_t)k; L->pending = true;
    }
    if (n_components) *n_components = (int64_t)k;
    return CX_OK;
}

extern "C" int cx_grid_label3d_result(cx_ctx* ctx, int32_t** labels_device, int64_t shape[3], int32_t* side, int32_t* connectivity, int64_t* n_components) {
    if (!ctx) return CX_ERR_INVALID;
    cx_label_state* L = ctx->label;
    if (!L || !L->pending) return cx_fail(ctx, CX_ERR_STATE, "cx_grid_label3d_result: no labels of cx_grid_label3d in the context");
    if (labels_device) *labels_device = reinterpret_cast<int32_t*>(L->labels.get());
    if (shape) { shape[0] = L->shape[0]; shape[1] = L->shape[1]; shape[2] = L->shape[2]; }
    if (side) *side = L->side;
    if (connectivity) *connectivity = L->connectivity;
    if (n_components) *n_components = L->k;
    return CX_OK;
}

extern "C" int cx_grid_label3d_measures(cx_ctx* ctx, cx_label_component* out_host, int64_t capacity) {
    if (!ctx) return CX_ERR_INVALID;
    cx_label_state* L = ctx->label;
    if (!L || !L->pending) return cx_fail(ctx, CX_ERR_STATE, "cx_grid_label3d_measures: no labels of cx_grid_label3d in the context");
    if (L->k == 0) return CX_OK;
    if (capacity < L->k || !out_host) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_label3d_measures: room for fewer records than there are components");
    CX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (!L->measured) {
        const int rc = L->records.grow(ctx, (size_t)L->k);
        if (rc) return rc;
        hipLaunchKernelGGL(cxl_k_records_init, cx_grid1((size_t)L->k), dim3(256), 0, st, L->records.get(), (uint32_t)L->k);
        CX_HIP(ctx, hipGetLastError());
        cxl_measure_args M;
        memset(&M, 0, sizeof(M));
        M.labels = L->labels.get(); M.rec = L->records.get();
        M.n0 = L->shape[0]; M.n1 = L->shape[1]; M.n2 = L->shape[2]; M.tiles = (M.n2 + 63) / 64;
        const uint32_t blocks = cxl_grid_rows(M.n0 * M.n1);      // many rows per wave: what a wave carries reaches the record once
        hipLaunchKernelGGL(cxl_k_measure, dim3(blocks < CXL_MEASURE_BLOCKS ? blocks : CXL_MEASURE_BLOCKS), dim3(256), 0, st, M);
        CX_HIP(ctx, hipGetLastError());
        L->measured = true;
    }
    CX_HIP(ctx, hipMemcpyAsync(out_host, L->records, (size_t)L->k * sizeof(cx_label_component), hipMemcpyDeviceToHost, st));
    CX_HIP(ctx, hipStreamSynchronize(st));
    return CX_OK;
}

extern "C" int cx_grid_label3d_select(cx_ctx* ctx, const uint8_t* keep, int64_t n_keep, uint8_t* out_device, uint8_t* out_host, int64_t* n_voxels) {
    if (!ctx) return CX_ERR_INVALID;
    cx_label_state* L = ctx->label;
    if (!L || !L->pending) return cx_fail(ctx, CX_ERR_STATE, "cx_grid_label3d_select: no labels of cx_grid_label3d in the context");
    if (!keep || n_keep != L->k + 1) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_label3d_select: one keep byte per label, 0 included");
    const size_t count = (size_t)(L->shape[0] * L->shape[1] * L->shape[2]);
    if (out_device && cx_overlap(L->labels.get(), count * sizeof(uint32_t), out_device, count)) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_label3d_select: the output overlaps the labels");
    CX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int rc;
    if ((rc = L->keep.grow(ctx, (size_t)n_keep))) return rc;
    CX_HIP(ctx, hipMemcpyAsync(L->keep, keep, (size_t)n_keep, hipMemcpyHostToDevice, st));
    void* opened;
    if ((rc = L->mask.open(ctx, out_device, count, &opened))) return rc;
    uint8_t* out = static_cast<uint8_t*>(opened);
    CX_HIP(ctx, hipMemsetAsync(L->misc.get() + 1, 0, sizeof(u64), st));
    cxl_select_args S;
    memset(&S, 0, sizeof(S));
    S.labels = L->labels.get(); S.keep = L->keep.get(); S.out = out; S.ones = L->misc.get() + 1; S.n = count;
    S.head = (size_t)((16u - ((uintptr_t)out & 15u)) & 15u);
    if (S.head > count) S.head = count;
    S.groups = (count - S.head) / 16u;
    const size_t threads = S.groups > 32u ? S.groups : 32u;      // (the loose samples are fewer than 32)
    const uint32_t blocks = cxl_grid_flat(threads);
    hipLaunchKernelGGL(cxl_k_select, dim3(blocks < CXL_SELECT_BLOCKS ? blocks : CXL_SELECT_BLOCKS), dim3(256), 0, st, S);
    CX_HIP(ctx, hipGetLastError());
    u64 ones = 0;
    CX_HIP(ctx, hipMemcpyAsync(&ones, L->misc.get() + 1, sizeof(ones), hipMemcpyDeviceToHost, st));
    if (out_host) CX_HIP(ctx, hipMemcpyAsync(out_host, out, count, hipMemcpyDeviceToHost, st));
    CX_HIP(ctx, hipStreamSynchronize(st));
    if (!out_device) { L->mask.publish(L->shape[0], L->shape[1], L->shape[2]); L->mask_voxels = (int64_t)ones; }
    if (n_voxels) *n_voxels = (int64_t)ones;
    return CX_OK;
}

extern "C" int cx_grid_label3d_select_result(cx_ctx* ctx, uint8_t** mask_device, int64_t shape[3], int64_t* n_voxels) {
    if (!ctx) return CX_ERR_INVALID;
    const cx_label_state* L = ctx->label;
    void* mask = nullptr;
    const int rc = cx_slot_result(ctx, L ? &L->mask : nullptr, "cx_grid_label3d_select_result: no mask of cx_grid_label3d_select in the context", &mask, shape);
    if (rc) return rc;
    if (mask_device) *mask_device = static_cast<uint8_t*>(mask);
    if (n_voxels) *n_voxels = L->mask_voxels;
    return CX_OK;
}

extern "C" int cx_grid_label3d_bind(cx_ctx* ctx) {
    if (!ctx) return CX_ERR_INVALID;
    return cx_slot_bind(ctx, ctx->label ? &ctx->label->mask : nullptr, "cx_grid_label3d_bind: no mask of cx_grid_label3d_select in the context", CX_DTYPE_U8);
}
