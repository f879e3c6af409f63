// cx_regions.hip -- the regions of a labelled volume (include/contourist_hip.h, section "regions"): one record per label with its
// shape measures and the extremes and sums of a second array (cx_grid_regions3d), a mask chosen by label and cropped to a box
// (cx_grid_regions3d_select, _select_result, _bind), a relabelling through a table (cx_grid_regions3d_map) and the face contacts
// between labels (cx_grid_regions3d_contacts).  The labels are any int32 volume, whichever call made it: every entry point takes them
// as an argument and the state keeps no reference to them.  A label <= 0 is background.
//
//   cxr_k_max        the largest label and the number of negative ones: one atomic of each per workgroup.
//   cxr_k_measure    a wave owns a row of labels and walks it in tiles of 64 columns, as cxl_k_measure does, but the lanes of a tile are
//                    grouped by EQUAL LABEL, not by runs: side by side two samples of a watershed carry different labels.  A group's
//                    partial is reduced across the wave and joins the one label the wave carries by majority vote (Boyer-Moore over the
//                    voxels seen), so that a region that fills much of the volume reaches its record once per wave.  At most
//                    CXR_GROUPS_MAX groups of a tile are reduced that way; in a tile with more labels than that (label noise) the lanes
//                    left over issue their own atomics, which then hardly collide.  Minimum and maximum are one 64-bit atomic each on
//                    a packed word (key << 32 | index, key << 32 | ~index): value, place and tie rule in one comparison.
//   cxr_k_finalize   the working records become cx_region: the packed words unpacked, the empty ones given their stated values.
//   cxr_k_select     one pass over the OUTPUT: the mask of the array extended by zeros, cropped to a box; 16 bytes per store where the
//                    output is aligned, one count per workgroup.
//   cxr_k_map        out = table[label], 16 bytes per load and store; in place is legal (a thread reads its samples before it writes).
//   cxr_k_contacts   a wave owns a row; every sample looks at its +1 neighbour along each axis.  The pairs of a tile are grouped by
//                    equal pair among the lanes (a contact face gives long runs of one pair), the first lane of a group adds the
//                    group's count to the pair's slot of an open-addressing table.  More than half full: the overflow flag, and the
//                    host doubles the table and runs again.
//   cxr_k_collect    the occupied slots, compacted in slot order (cx_scan_u32); the host sorts them by (a, b).
// Integer atomics everywhere but the float sum (vsum of a float array): everything else is the same bytes in every call.
// DESIGN.md section 9t.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>

#include "cx_dev.h"
#include "cx_gridop.h"

#define CXR_WAVES 4u
#define CXR_ROW_BLOCKS 1024u          // measure, contacts: many rows per wave, so that what a wave carries reaches its record once
#define CXR_FLAT_BLOCKS 2048u         // max, select, map: a lane walks its groups with the grid's stride
#define CXR_GROUPS_MAX 8              // measure: groups of a tile reduced across the wave; the lanes of further labels add for themselves
#define CXR_PAIR_GROUPS 6             // contacts: the same for the pairs of a tile and axis
#define CXR_TABLE_MIN 1024ull         // contacts: slots of the first table (512 pairs); doubled on overflow, never shrunk
#define CXR_TABLE_MAX (1ull << 27)    // 4 GiB of slots

struct cxr_pair_slot { u64 key, faces[3]; };      // key = a << 32 | b, CXD_EMPTY: free
static_assert(sizeof(cx_region) == 128 && sizeof(cx_region_contact) == 32 && sizeof(cxr_pair_slot) == 32, "the records of the header");

struct cx_regions_state {
    cx_slot mask;                  // `in`: host labels; `result`: the context's own mask (cx_grid_regions3d_select), pending until the bind
    cx_buf<uint8_t> values;        // host values
    cx_buf<uint8_t> mapped;        // the output of cx_grid_regions3d_map for device labels without out_device
    cx_buf<u64> misc;              // [0] largest label, [1] negative labels, [2] ones of the select, [3] slots in use, [4] overflow, [5] pairs
    cx_buf<cx_region> records;
    cx_buf<uint8_t> keep;
    cx_buf<int32_t> table;         // the caller's map
    cx_buf<cxr_pair_slot> pairs;   // the open-addressing table of the contacts
    cx_buf<uint32_t> rank, sums;   // occupied flags, their scan, its block sums
    cx_buf<cx_region_contact> found;
    int64_t origin[3] = {0, 0, 0};
    int64_t mask_voxels = 0;
};

void cx_regions_free(cx_ctx* ctx) {
    delete ctx->regions;
    ctx->regions = nullptr;
}

static uint32_t cxr_grid_rows(int64_t rows) {
    const unsigned long long blocks = ((unsigned long long)rows + CXR_WAVES - 1u) / CXR_WAVES;
    return (uint32_t)(blocks < CXR_ROW_BLOCKS ? (blocks ? blocks : 1ull) : CXR_ROW_BLOCKS);
}
static uint32_t cxr_grid_flat(size_t items) {
    const size_t blocks = (items + 255u) / 256u;
    return (uint32_t)(blocks < CXR_FLAT_BLOCKS ? (blocks ? blocks : 1u) : CXR_FLAT_BLOCKS);
}

// ---- the largest label ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cxr_k_max(const int32_t* __restrict__ labels, size_t n, u64* misc) {
    uint32_t top = 0u, negative = 0u;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) {
        const int32_t l = labels[i];
        if (l < 0) negative++;
        else top = (uint32_t)l > top ? (uint32_t)l : top;
    }
    __shared__ uint32_t tops[CXR_WAVES], negatives[CXR_WAVES];
    top = (uint32_t)cxd_wave_max((u64)top);
    negative = cxd_wave_add(negative);
    if ((threadIdx.x & 63u) == 0u) { tops[threadIdx.x >> 6] = top; negatives[threadIdx.x >> 6] = negative; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        for (uint32_t w = 1; w < CXR_WAVES; w++) { top = tops[w] > top ? tops[w] : top; negative += negatives[w]; }
        if (top) cxd_max64(&misc[0], (u64)top);
        if (negative) atomicAdd(&misc[1], (u64)negative);
    }
}

// ---- the records --------------------------------------------------------------------------------------------------------------------------
// While the measure kernel runs a record is a WORKING record: min_at and max_at hold the packed words of the two extremes (all ones and
// zero: none yet), first, lo and hi the identities of their minima and maxima.  cxr_k_finalize makes it the record of the header.
__global__ __launch_bounds__(256) void cxr_k_records_init(cx_region* rec, uint32_t k) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= k) return;
    cx_region r;
    memset(&r, 0, sizeof(r));
    r.shape.first = INT64_MAX;
    for (int a = 0; a < 3; a++) { r.shape.lo[a] = INT32_MAX; r.shape.hi[a] = INT32_MIN; }
    r.min_at = -1;      // (all ones)
    rec[c] = r;
}

template <int DT> struct cxr_kind { static constexpr bool is_float = DT == CX_DTYPE_F32 || DT == CX_DTYPE_F16 || DT == CX_DTYPE_BF16; };
// the bits of sample i, zero-extended; the key of a NaN; the bits as a double (exact for every sample type)
template <int DT>
__device__ __forceinline__ uint32_t cxr_raw(const void* values, size_t i) {
    if constexpr (DT == CX_DTYPE_F32) return __float_as_uint(static_cast<const float*>(values)[i]);
    else return (uint32_t)(typename cx_dt<DT>::bits) static_cast<const typename cx_dt<DT>::T*>(values)[i];
}
template <int DT>
__device__ __forceinline__ double cxr_double(uint32_t raw) {
    if constexpr (DT == CX_DTYPE_F32) return (double)__uint_as_float(raw);
    else return (double)cx_dt<DT>::cvt(raw);
}
__device__ __forceinline__ uint32_t cxr_nan_key(int32_t dtype) { return dtype == CX_DTYPE_F32 ? 0xFFFFFFFFu : 0xFFFFu; }
__device__ __forceinline__ double cxr_double_of(int32_t dtype, uint32_t raw) {
    switch (dtype) {
        case CX_DTYPE_U8: return cxr_double<CX_DTYPE_U8>(raw);
        case CX_DTYPE_I8: return cxr_double<CX_DTYPE_I8>(raw);
        case CX_DTYPE_U16: return cxr_double<CX_DTYPE_U16>(raw);
        case CX_DTYPE_I16: return cxr_double<CX_DTYPE_I16>(raw);
        case CX_DTYPE_F16: return cxr_double<CX_DTYPE_F16>(raw);
        case CX_DTYPE_BF16: return cxr_double<CX_DTYPE_BF16>(raw);
        default: return cxr_double<CX_DTYPE_F32>(raw);
    }
}

struct cxr_measure_args {
    const int32_t* labels;
    const void* values;
    cx_region* rec;
    int64_t n0, n1, n2, tiles;
    int32_t groups_max;      // CXR_GROUPS_MAX (a debug knob of the benchmark tool moves it)
};

// what a wave (or, in the many-labels case, a lane) has added up for one label and not yet put into the record
struct cxr_part {
    uint32_t label;      // 0: nothing
    int64_t voxels, first, sum[3];
    int32_t lo[3], hi[3];
    uint32_t rim;
    int64_t n_nan, isum;
    u64 minw, maxw;      // the packed extremes; all ones / zero: none
    double vsum;
};
// the samples of one label in one tile of row (i, j): `len` of them between the columns s and e, their columns summing to sk
__device__ __forceinline__ void cxr_part_shape(const cxr_measure_args& A, cxr_part& P, uint32_t label, int64_t i, int64_t j, int64_t len, int64_t sk, int64_t s, int64_t e) {
    P.label = label; P.voxels = len; P.first = (i * A.n1 + j) * A.n2 + s;
    P.sum[0] = i * len; P.sum[1] = j * len; P.sum[2] = sk;
    P.lo[0] = P.hi[0] = (int32_t)i; P.lo[1] = P.hi[1] = (int32_t)j; P.lo[2] = (int32_t)s; P.hi[2] = (int32_t)e;
    P.rim = (i == 0 ? 1u : 0u) | (i == A.n0 - 1 ? 2u : 0u) | (j == 0 ? 4u : 0u) | (j == A.n1 - 1 ? 8u : 0u) | (s == 0 ? 16u : 0u) | (e == A.n2 - 1 ? 32u : 0u);
}
__device__ __forceinline__ void cxr_part_add(cxr_part& H, const cxr_part& P) {
    H.voxels += P.voxels;
    H.first = P.first < H.first ? P.first : H.first;
    for (int a = 0; a < 3; a++) {
        H.sum[a] += P.sum[a];
        H.lo[a] = P.lo[a] < H.lo[a] ? P.lo[a] : H.lo[a];
        H.hi[a] = P.hi[a] > H.hi[a] ? P.hi[a] : H.hi[a];
    }
    H.rim |= P.rim;
    H.n_nan += P.n_nan; H.isum += P.isum; H.vsum += P.vsum;
    H.minw = P.minw < H.minw ? P.minw : H.minw;
    H.maxw = P.maxw > H.maxw ? P.maxw : H.maxw;
}
__device__ __forceinline__ void cxr_min_i32(int32_t* addr, int32_t v) {
    if (__hip_atomic_load(addr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= v) return;
    atomicMin(addr, v);
}
__device__ __forceinline__ void cxr_max_i32(int32_t* addr, int32_t v) {
    if (__hip_atomic_load(addr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= v) return;
    atomicMax(addr, v);
}
__device__ __forceinline__ void cxr_min_i64(int64_t* addr, int64_t v) {
    if (__hip_atomic_load(addr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= v) return;
    atomicMin((long long*)addr, (long long)v);
}
// into the working record: one lane's atomics (the extremes and the rim bits look first)
template <bool VAL, bool FLT>
__device__ __forceinline__ void cxr_part_flush(const cxr_measure_args& A, const cxr_part& P) {
    cx_region* r = A.rec + (P.label - 1u);
    atomicAdd((unsigned long long*)&r->shape.voxels, (unsigned long long)P.voxels);
    for (int a = 0; a < 3; a++) {
        if (P.sum[a]) atomicAdd((unsigned long long*)&r->shape.sum[a], (unsigned long long)P.sum[a]);
        cxr_min_i32(&r->shape.lo[a], P.lo[a]);
        cxr_max_i32(&r->shape.hi[a], P.hi[a]);
    }
    cxr_min_i64(&r->shape.first, P.first);
    if (P.rim & ~__hip_atomic_load(&r->shape.rim, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(&r->shape.rim, P.rim);
    if constexpr (VAL) {
        if (P.n_nan) atomicAdd((unsigned long long*)&r->n_nan, (unsigned long long)P.n_nan);
        if (P.minw != ~0ull) cxd_min64(reinterpret_cast<u64*>(&r->min_at), P.minw);
        if (P.maxw != 0ull) cxd_max64(reinterpret_cast<u64*>(&r->max_at), P.maxw);
        if constexpr (FLT) {
            if (P.maxw != 0ull) atomicAdd(&r->vsum, P.vsum);      // (some sample of the part is not NaN)
        } else if (P.isum) atomicAdd((unsigned long long*)&r->isum, (unsigned long long)P.isum);
    }
}
__device__ __forceinline__ double cxr_wave_add(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __longlong_as_double((long long)cxd_shfl_xor64((u64)__double_as_longlong(v), o));
    return v;
}

template <int DT, bool VAL>
__global__ __launch_bounds__(256) void cxr_k_measure(const cxr_measure_args A) {
    constexpr bool FLT = cxr_kind<DT>::is_float;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    const int64_t rows = A.n0 * A.n1;
    cxr_part H;
    memset(&H, 0, sizeof(H));
    int64_t votes = 0;
    for (int64_t row = (int64_t)blockIdx.x * CXR_WAVES + wave; row < rows; row += (int64_t)gridDim.x * CXR_WAVES) {
        const int64_t i = row / A.n1, j = row % A.n1;
        const size_t base = (size_t)row * (size_t)A.n2;
        for (int64_t t = 0; t < A.tiles; t++) {
            const int64_t k = t * 64 + (int64_t)lane;
            const int32_t read = k < A.n2 ? A.labels[base + (size_t)k] : 0;
            const uint32_t label = read > 0 ? (uint32_t)read : 0u;
            u64 todo = __ballot(label != 0u);
            if (!todo) continue;
            // this lane's sample: the packed words of its value, or none for a NaN
            const uint32_t at = (uint32_t)(base + (size_t)k);      // (below 2^29)
            bool nan = false;
            u64 minw = ~0ull, maxw = 0ull;
            long long iv = 0;
            double dv = 0.0;
            if constexpr (VAL) {
                if (label) {
                    const uint32_t raw = cxr_raw<DT>(A.values, base + (size_t)k);
                    const uint32_t key = cxd_sample_key(DT, raw);
                    nan = FLT && key == cxr_nan_key(DT);
                    if (!nan) {
                        minw = ((u64)key << 32) | (u64)at;
                        maxw = ((u64)key << 32) | (u64)(0xFFFFFFFFu - at);
                        if constexpr (FLT) dv = cxr_double<DT>(raw);
                        else iv = (long long)cxr_double<DT>(raw);
                    }
                }
            }
            for (int round = 0; todo && round < A.groups_max; round++) {
                const int leader = (int)__builtin_ctzll(todo);
                const uint32_t gl = (uint32_t)__shfl((int)label, leader);
                const bool mine = label == gl;
                const u64 g = __ballot(mine);
                todo &= ~g;
                const int64_t len = (int64_t)__builtin_popcountll(g);
                const int64_t s = t * 64 + (int64_t)__builtin_ctzll(g), e = t * 64 + 63 - (int64_t)__builtin_clzll(g);
                cxr_part P;
                memset(&P, 0, sizeof(P));
                cxr_part_shape(A, P, gl, i, j, len, t * 64 * len + (int64_t)cxd_wave_add(mine ? lane : 0u), s, e);
                P.minw = ~0ull;
                if constexpr (VAL) {
                    P.n_nan = (int64_t)__builtin_popcountll(__ballot(mine && nan));
                    P.minw = cxd_wave_min(mine ? minw : ~0ull);
                    P.maxw = cxd_wave_max(mine ? maxw : 0ull);
                    if constexpr (FLT) P.vsum = cxr_wave_add(mine ? dv : 0.0);
                    else P.isum = (int64_t)cxd_wave_add((long long)(mine ? iv : 0));
                }
                if (H.label == gl) { cxr_part_add(H, P); votes += len; }
                else if (votes >= len) {
                    votes -= len;
                    if (lane == 0u) cxr_part_flush<VAL, FLT>(A, P);
                } else {
                    if (H.label && lane == 0u) cxr_part_flush<VAL, FLT>(A, H);
                    H = P;
                    votes = len;
                }
            }
            // more labels in the tile than that: every lane left adds its own sample (distinct records, mostly)
            if ((todo >> lane) & 1ull) {
                cxr_part P;
                memset(&P, 0, sizeof(P));
                cxr_part_shape(A, P, label, i, j, 1, k, k, k);
                P.n_nan = nan ? 1 : 0; P.minw = minw; P.maxw = maxw; P.isum = iv; P.vsum = dv;
                cxr_part_flush<VAL, FLT>(A, P);
            }
        }
    }
    if (H.label && lane == 0u) cxr_part_flush<VAL, FLT>(A, H);
}

__global__ __launch_bounds__(256) void cxr_k_finalize(cx_region* rec, uint32_t k, int32_t dtype, int has_values) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= k) return;
    cx_region r = rec[c];
    const u64 minw = (u64)r.min_at, maxw = (u64)r.max_at;
    if (r.shape.voxels == 0) {
        r.shape.first = -1;
        for (int a = 0; a < 3; a++) { r.shape.lo[a] = 0; r.shape.hi[a] = -1; }
    }
    r.min_at = r.max_at = -1;
    r.vmin = r.vmax = 0.0;
    if (has_values && maxw != 0ull) {
        r.min_at = (int64_t)(uint32_t)minw;
        r.max_at = (int64_t)(0xFFFFFFFFu - (uint32_t)maxw);
        r.vmin = cxr_double_of(dtype, cxd_sample_unkey(dtype, (uint32_t)(minw >> 32)));
        r.vmax = cxr_double_of(dtype, cxd_sample_unkey(dtype, (uint32_t)(maxw >> 32)));
    }
    const bool is_float = dtype == CX_DTYPE_F32 || dtype == CX_DTYPE_F16 || dtype == CX_DTYPE_BF16;
    if (!has_values) { r.isum = 0; r.vsum = 0.0; }
    else if (!is_float) r.vsum = (double)r.isum;
    rec[c] = r;
}

// ---- select with crop -------------------------------------------------------------------------------------------------------------------
struct cxr_select_args {
    const int32_t* labels;
    const uint8_t* keep;
    uint8_t* out;
    u64* ones;
    int64_t n[3], m[3], org[3], n_keep;
    size_t total, head, groups;      // `head` bytes in front of the first 16-byte boundary of `out`, then `groups` of 16, then the rest
};
// output position (i, j, k) of the crop: keep[label] inside the array, 0 outside
__device__ __forceinline__ uint32_t cxr_select_at(const cxr_select_args& A, int64_t i, int64_t j, int64_t k) {
    const int64_t si = i + A.org[0], sj = j + A.org[1], sk = k + A.org[2];
    if (si < 0 || sj < 0 || sk < 0 || si >= A.n[0] || sj >= A.n[1] || sk >= A.n[2]) return 0u;
    const int32_t l = A.labels[((size_t)si * (size_t)A.n[1] + (size_t)sj) * (size_t)A.n[2] + (size_t)sk];
    const int64_t c = l > 0 ? (int64_t)l : 0;
    return c < A.n_keep && A.keep[c] ? 1u : 0u;
}
__global__ __launch_bounds__(256) void cxr_k_select(const cxr_select_args A) {
    uint32_t count = 0;
    const size_t tid = (size_t)blockIdx.x * 256u + threadIdx.x, step = (size_t)gridDim.x * 256u;
    for (size_t g = tid; g < A.groups; g += step) {
        const size_t at = A.head + g * 16u;
        int64_t k = (int64_t)(at % (size_t)A.m[2]);
        const size_t rowi = at / (size_t)A.m[2];
        int64_t j = (int64_t)(rowi % (size_t)A.m[1]), i = (int64_t)(rowi / (size_t)A.m[1]);
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int b = 0; b < 16; b++) {
            const uint32_t one = cxr_select_at(A, i, j, k);
            w[b >> 2] |= one << (8 * (b & 3));
            count += one;
            if (++k == A.m[2]) {
                k = 0;
                if (++j == A.m[1]) { j = 0; i++; }
            }
        }
        *reinterpret_cast<uint4*>(A.out + at) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    // the bytes in front of the first group and behind the last one: fewer than 32
    const size_t tail0 = A.head + A.groups * 16u, loose = A.head + (A.total - tail0);
    if (tid < loose) {
        const size_t at = tid < A.head ? tid : tail0 + (tid - A.head);
        const size_t rowi = at / (size_t)A.m[2];
        const uint32_t one = cxr_select_at(A, (int64_t)(rowi / (size_t)A.m[1]), (int64_t)(rowi % (size_t)A.m[1]), (int64_t)(at % (size_t)A.m[2]));
        A.out[at] = (uint8_t)one;
        count += one;
    }
    __shared__ uint32_t per_wave[CXR_WAVES];
    count = cxd_wave_add(count);
    if ((threadIdx.x & 63u) == 0u) per_wave[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0u) {
        const uint32_t total = per_wave[0] + per_wave[1] + per_wave[2] + per_wave[3];
        if (total) atomicAdd(A.ones, (u64)total);
    }
}

// ---- map ----------------------------------------------------------------------------------------------------------------------------------
struct cxr_map_args {
    const int32_t* labels;
    const int32_t* table;
    int32_t* out;
    int64_t n_map;
    size_t total, head, groups;      // in samples: `head` in front of the first 16-byte boundary of `out`, then `groups` of 4, then the rest
};
struct __attribute__((packed, aligned(4))) cxr_labels4 { int32_t x, y, z, w; };
__device__ __forceinline__ int32_t cxr_map_of(const cxr_map_args& A, int32_t l) {
    const int64_t c = l > 0 ? (int64_t)l : 0;
    return c < A.n_map ? A.table[c] : 0;
}
__global__ __launch_bounds__(256) void cxr_k_map(const cxr_map_args A) {
    const size_t tid = (size_t)blockIdx.x * 256u + threadIdx.x, step = (size_t)gridDim.x * 256u;
    for (size_t g = tid; g < A.groups; g += step) {
        const size_t at = A.head + g * 4u;
        const cxr_labels4 l = *reinterpret_cast<const cxr_labels4*>(A.labels + at);      // (aligned to 4: one 16-byte load)
        *reinterpret_cast<int4*>(A.out + at) = make_int4(cxr_map_of(A, l.x), cxr_map_of(A, l.y), cxr_map_of(A, l.z), cxr_map_of(A, l.w));
    }
    const size_t tail0 = A.head + A.groups * 4u, loose = A.head + (A.total - tail0);      // fewer than 8
    if (tid < loose) {
        const size_t at = tid < A.head ? tid : tail0 + (tid - A.head);
        A.out[at] = cxr_map_of(A, A.labels[at]);
    }
}

// ---- contacts -----------------------------------------------------------------------------------------------------------------------------
struct cxr_contact_args {
    const int32_t* labels;
    cxr_pair_slot* tab;
    u64* ctl;            // [0] slots in use, [1] overflow
    u64 mask;            // slots - 1
    int64_t n0, n1, n2, tiles;
};
__device__ __forceinline__ void cxr_pair_add(const cxr_contact_args& A, u64 key, int axis, u64 count) {
    u64 s = cxd_mix(key) & A.mask;
    for (u64 probes = 0; probes <= A.mask; probes++, s = (s + 1ull) & A.mask) {
        u64 seen = __hip_atomic_load(&A.tab[s].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seen == CXD_EMPTY) {
            seen = atomicCAS(&A.tab[s].key, CXD_EMPTY, key);
            if (seen == CXD_EMPTY) {
                seen = key;
                if ((atomicAdd(&A.ctl[0], 1ull) + 1ull) * 2ull > A.mask + 1ull) atomicMax(&A.ctl[1], 1ull);      // more than half full
            }
        }
        if (seen != key) continue;
        atomicAdd(&A.tab[s].faces[axis], count);
        return;
    }
    atomicMax(&A.ctl[1], 1ull);
}
__global__ __launch_bounds__(256) void cxr_k_pairs_init(cxr_pair_slot* tab, size_t slots) {
    for (size_t s = (size_t)blockIdx.x * 256u + threadIdx.x; s < slots; s += (size_t)gridDim.x * 256u) {
        cxr_pair_slot e;
        e.key = CXD_EMPTY; e.faces[0] = e.faces[1] = e.faces[2] = 0ull;
        tab[s] = e;
    }
}
__global__ __launch_bounds__(256) void cxr_k_contacts(const cxr_contact_args A) {
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    const int64_t rows = A.n0 * A.n1;
    for (int64_t row = (int64_t)blockIdx.x * CXR_WAVES + wave; row < rows; row += (int64_t)gridDim.x * CXR_WAVES) {
        if (__hip_atomic_load(&A.ctl[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;      // the table is too small: this run is thrown away
        const int64_t i = row / A.n1, j = row % A.n1;
        const size_t base = (size_t)row * (size_t)A.n2;
        for (int64_t t = 0; t < A.tiles; t++) {
            const int64_t k = t * 64 + (int64_t)lane;
            const bool active = k < A.n2;
            const int32_t read = active ? A.labels[base + (size_t)k] : 0;
            const uint32_t me = read > 0 ? (uint32_t)read : 0u;
#pragma unroll
            for (int axis = 0; axis < 3; axis++) {
                const bool has = active && (axis == 0 ? i + 1 < A.n0 : (axis == 1 ? j + 1 < A.n1 : k + 1 < A.n2));
                const size_t step = axis == 0 ? (size_t)(A.n1 * A.n2) : (axis == 1 ? (size_t)A.n2 : (size_t)1);
                const int32_t nread = has ? A.labels[base + (size_t)k + step] : read;
                const uint32_t other = nread > 0 ? (uint32_t)nread : 0u;
                const u64 key = me == other ? 0ull : (me < other ? ((u64)me << 32) | other : ((u64)other << 32) | me);      // (never 0 for a pair: b >= 1)
                u64 todo = __ballot(key != 0ull);
                for (int round = 0; todo && round < CXR_PAIR_GROUPS; round++) {
                    const int leader = (int)__builtin_ctzll(todo);
                    const u64 gk = ((u64)(uint32_t)__shfl((int)(uint32_t)(key >> 32), leader) << 32) | (u64)(uint32_t)__shfl((int)(uint32_t)key, leader);
                    const u64 g = __ballot(key == gk);
                    todo &= ~g;
                    if ((int)lane == leader) cxr_pair_add(A, gk, axis, (u64)__builtin_popcountll(g));
                }
                if ((todo >> lane) & 1ull) cxr_pair_add(A, key, axis, 1ull);
            }
        }
    }
}
__global__ __launch_bounds__(256) void cxr_k_occupied(const cxr_pair_slot* __restrict__ tab, uint32_t* flag, uint32_t slots) {
    for (uint32_t s = blockIdx.x * 256u + threadIdx.x; s < slots; s += gridDim.x * 256u) flag[s] = tab[s].key != CXD_EMPTY ? 1u : 0u;
}
__global__ __launch_bounds__(256) void cxr_k_collect(const cxr_pair_slot* __restrict__ tab, const uint32_t* __restrict__ rank, cx_region_contact* out, uint32_t slots) {
    for (uint32_t s = blockIdx.x * 256u + threadIdx.x; s < slots; s += gridDim.x * 256u) {
        const cxr_pair_slot e = tab[s];
        if (e.key == CXD_EMPTY) continue;
        cx_region_contact c;
        c.a = (int32_t)(uint32_t)(e.key >> 32); c.b = (int32_t)(uint32_t)e.key;
        c.faces[0] = (int64_t)e.faces[0]; c.faces[1] = (int64_t)e.faces[1]; c.faces[2] = (int64_t)e.faces[2];
        out[rank[s]] = c;
    }
}

// ---- the entry points ----------------------------------------------------------------------------------------------------------------------
// the labels of a call: int32, aligned to 4, every axis >= 1, at most 2^29 samples (the sample types of cx_source_resolve have no int32:
// its shape checks, restated)
static int cxr_labels(cx_ctx* ctx, const char* who, const int32_t* labels, int on_device, int64_t n0, int64_t n1, int64_t n2, cx_source* S) {
    auto refuse = [&](const char* what) { return cx_fail(ctx, CX_ERR_INVALID, (std::string(who) + ": " + what).c_str()); };
    if (!labels) return refuse("no labels given");
    if ((uintptr_t)labels & 3u) return refuse("labels must be aligned to 4 bytes");
    const int64_t lim = 1LL << 29;
    if (n0 < 1 || n1 < 1 || n2 < 1 || n0 > lim || n1 > lim || n2 > lim || n0 * n1 > lim || n0 * n1 * n2 > lim)
        return refuse("at least 1 sample per axis, at most 2^29 in all");
    S->p = labels; S->dtype = 0; S->on_device = on_device;
    S->n[0] = n0; S->n[1] = n1; S->n[2] = n2;
    S->count = (size_t)(n0 * n1 * n2); S->bytes = S->count * sizeof(int32_t);
    return CX_OK;
}
// the state, and the labels where the kernels read them
static int cxr_begin(cx_ctx* ctx, const cx_source& S, cx_regions_state** state, const int32_t** dev) {
    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_regions_state* R = cx_state_of(ctx->regions);
    if (!R) return CX_ERR_NOMEM;
    int rc;
    if ((rc = R->misc.grow(ctx, 8))) return rc;
    const void* p = nullptr;
    if ((rc = R->mask.stage(ctx, S, &p))) return rc;
    *state = R;
    *dev = static_cast<const int32_t*>(p);
    return CX_OK;
}

extern "C" int cx_grid_regions3d(cx_ctx* ctx, const int32_t* labels, int on_device, int64_t n0, int64_t n1, int64_t n2,
                                 const void* values, int32_t values_dtype, int values_on_device, cx_region* out_host, int64_t capacity,
                                 int64_t* k_max, int64_t* n_negative) {
    if (!ctx) return CX_ERR_INVALID;
    cx_source S, V;
    int rc = cxr_labels(ctx, "cx_grid_regions3d", labels, on_device, n0, n1, n2, &S);
    if (rc) return rc;
    if (values && (rc = cx_source_resolve(ctx, "cx_grid_regions3d (values)", values, values_dtype, values_on_device, n0, n1, n2, 29, &V))) return rc;
    cx_regions_state* R;
    const int32_t* dev;
    if ((rc = cxr_begin(ctx, S, &R, &dev))) return rc;
    hipStream_t st = ctx->stream;
    CX_HIP(ctx, hipMemsetAsync(R->misc.get(), 0, 2 * sizeof(u64), st));
    hipLaunchKernelGGL(cxr_k_max, dim3(cxr_grid_flat(S.count)), dim3(256), 0, st, dev, S.count, R->misc.get());
    CX_HIP(ctx, hipGetLastError());
    u64 top[2] = {0, 0};
    CX_HIP(ctx, hipMemcpyAsync(top, R->misc.get(), sizeof(top), hipMemcpyDeviceToHost, st));
    CX_HIP(ctx, hipStreamSynchronize(st));
    const int64_t k = (int64_t)top[0];
    if (k_max) *k_max = k;
    if (n_negative) *n_negative = (int64_t)top[1];
    if (k > CX_REGIONS_MAX_LABEL) return cx_fail(ctx, CX_ERR_UNSUPPORTED, "cx_grid_regions3d: a label above CX_REGIONS_MAX_LABEL");
    if (!out_host || k == 0) return CX_OK;
    if (capacity < k) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_regions3d: room for fewer records than the largest label");
    const void* vdev = nullptr;
    if (values) {
        vdev = V.p;
        if (!V.on_device && (rc = cx_upload(ctx, R->values, V.p, V.bytes, &vdev))) return rc;
    }
    if ((rc = R->records.grow(ctx, (size_t)k))) return rc;
    hipLaunchKernelGGL(cxr_k_records_init, cx_grid1((size_t)k), dim3(256), 0, st, R->records.get(), (uint32_t)k);
    CX_HIP(ctx, hipGetLastError());
    cxr_measure_args M;
    memset(&M, 0, sizeof(M));
    M.labels = dev; M.values = vdev; M.rec = R->records.get();
    M.n0 = n0; M.n1 = n1; M.n2 = n2; M.tiles = (n2 + 63) / 64;
    M.groups_max = (int32_t)cx_debug_knob("CX_REGIONS_GROUPS", CXR_GROUPS_MAX);      // (tools/bench_regions.py compares settings)
    const dim3 grid(cxr_grid_rows(n0 * n1));
    if (!values) hipLaunchKernelGGL((cxr_k_measure<CX_DTYPE_U8, false>), grid, dim3(256), 0, st, M);
    else {
#define CX_LAUNCH(DT) hipLaunchKernelGGL((cxr_k_measure<DT, true>), grid, dim3(256), 0, st, M);
        CX_DISPATCH_DTYPE(V.dtype, CX_LAUNCH)
#undef CX_LAUNCH
    }
    CX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(cxr_k_finalize, cx_grid1((size_t)k), dim3(256), 0, st, R->records.get(), (uint32_t)k, values ? V.dtype : 0, values ? 1 : 0);
    CX_HIP(ctx, hipGetLastError());
    CX_HIP(ctx, hipMemcpyAsync(out_host, R->records.get(), (size_t)k * sizeof(cx_region), hipMemcpyDeviceToHost, st));
    CX_HIP(ctx, hipStreamSynchronize(st));
    return CX_OK;
}

extern "C" int cx_grid_regions3d_select(cx_ctx* ctx, const int32_t* labels, int on_device, int64_t n0, int64_t n1, int64_t n2,
                                        const uint8_t* keep, int64_t n_keep, const int64_t box_lo[3], const int64_t box_hi[3], int32_t pad,
                                        uint8_t* out_device, uint8_t* out_host, int64_t out_shape[3], int64_t out_origin[3], int64_t* n_voxels) {
    if (!ctx) return CX_ERR_INVALID;
    cx_source S;
    int rc = cxr_labels(ctx, "cx_grid_regions3d_select", labels, on_device, n0, n1, n2, &S);
    if (rc) return rc;
    if (n_keep < 0 || (n_keep > 0 && !keep)) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_regions3d_select: n_keep keep bytes");
    if (pad < 0 || pad > 8) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_regions3d_select: a pad of 0 .. 8");
    if ((box_lo == nullptr) != (box_hi == nullptr)) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_regions3d_select: both ends of the box, or neither");
    int64_t m[3], org[3];
    for (int a = 0; a < 3; a++) {
        const int64_t lo = box_lo ? box_lo[a] : 0, hi = box_hi ? box_hi[a] : S.n[a] - 1;
        if (lo < 0 || hi >= S.n[a] || lo > hi) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_regions3d_select: the box lies inside the array, lo <= hi");
        m[a] = hi - lo + 1 + 2 * pad;
        org[a] = lo - pad;
    }
    const size_t total = (size_t)(m[0] * m[1] * m[2]);      // (at most (2^29 + 16)^... of one axis; the product stays far below 2^63)
    if (out_device && S.on_device && cx_overlap(S.p, S.bytes, out_device, total)) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_regions3d_select: the output overlaps the labels");
    cx_regions_state* R;
    const int32_t* dev;
    if ((rc = cxr_begin(ctx, S, &R, &dev))) return rc;
    hipStream_t st = ctx->stream;
    if ((rc = R->keep.grow(ctx, (size_t)(n_keep > 0 ? n_keep : 1)))) return rc;
    if (n_keep > 0) CX_HIP(ctx, hipMemcpyAsync(R->keep, keep, (size_t)n_keep, hipMemcpyHostToDevice, st));
    void* opened;
    if ((rc = R->mask.open(ctx, out_device, total, &opened))) return rc;
    uint8_t* out = static_cast<uint8_t*>(opened);
    CX_HIP(ctx, hipMemsetAsync(R->misc.get() + 2, 0, sizeof(u64), st));
    cxr_select_args A;
    memset(&A, 0, sizeof(A));
    A.labels = dev; A.keep = R->keep.get(); A.out = out; A.ones = R->misc.get() + 2; A.n_keep = n_keep; A.total = total;
    for (int a = 0; a < 3; a++) { A.n[a] = S.n[a]; A.m[a] = m[a]; A.org[a] = org[a]; }
    A.head = (size_t)((16u - ((uintptr_t)out & 15u)) & 15u);
    if (A.head > total) A.head = total;
    A.groups = (total - A.head) / 16u;
    hipLaunchKernelGGL(cxr_k_select, dim3(cxr_grid_flat(A.groups > 32u ? A.groups : 32u)), dim3(256), 0, st, A);      // (the loose bytes are fewer than 32)
    CX_HIP(ctx, hipGetLastError());
    u64 ones = 0;
    CX_HIP(ctx, hipMemcpyAsync(&ones, R->misc.get() + 2, sizeof(ones), hipMemcpyDeviceToHost, st));
    if (out_host) CX_HIP(ctx, hipMemcpyAsync(out_host, out, total, hipMemcpyDeviceToHost, st));
    CX_HIP(ctx, hipStreamSynchronize(st));
    if (!out_device) {
        R->mask.publish(m[0], m[1], m[2]);
        R->mask_voxels = (int64_t)ones;
        for (int a = 0; a < 3; a++) R->origin[a] = org[a];
    }
    for (int a = 0; a < 3; a++) {
        if (out_shape) out_shape[a] = m[a];
        if (out_origin) out_origin[a] = org[a];
    }
    if (n_voxels) *n_voxels = (int64_t)ones;
    return CX_OK;
}

extern "C" int cx_grid_regions3d_select_result(cx_ctx* ctx, uint8_t** mask_device, int64_t shape[3], int64_t origin[3], int64_t* n_voxels) {
    if (!ctx) return CX_ERR_INVALID;
    const cx_regions_state* R = ctx->regions;
    void* mask = nullptr;
    const int rc = cx_slot_result(ctx, R ? &R->mask : nullptr, "cx_grid_regions3d_select_result: no mask of cx_grid_regions3d_select in the context", &mask, shape);
    if (rc) return rc;
    if (mask_device) *mask_device = static_cast<uint8_t*>(mask);
    if (origin) { origin[0] = R->origin[0]; origin[1] = R->origin[1]; origin[2] = R->origin[2]; }
    if (n_voxels) *n_voxels = R->mask_voxels;
    return CX_OK;
}

extern "C" int cx_grid_regions3d_bind(cx_ctx* ctx) {
    if (!ctx) return CX_ERR_INVALID;
    return cx_slot_bind(ctx, ctx->regions ? &ctx->regions->mask : nullptr, "cx_grid_regions3d_bind: no mask of cx_grid_regions3d_select in the context", CX_DTYPE_U8);
}

extern "C" int cx_grid_regions3d_map(cx_ctx* ctx, const int32_t* labels, int on_device, int64_t n0, int64_t n1, int64_t n2,
                                     const int32_t* map, int64_t n_map, int32_t* out_device, int32_t* out_host) {
    if (!ctx) return CX_ERR_INVALID;
    cx_source S;
    int rc = cxr_labels(ctx, "cx_grid_regions3d_map", labels, on_device, n0, n1, n2, &S);
    if (rc) return rc;
    if (n_map < 0 || (n_map > 0 && !map)) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_regions3d_map: n_map entries of the map");
    if (!out_device && !out_host) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_regions3d_map: no output given");
    if ((uintptr_t)out_device & 3u) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_regions3d_map: out_device must be aligned to 4 bytes");
    if (out_device && S.on_device && (const void*)out_device != S.p && cx_overlap(S.p, S.bytes, out_device, S.bytes))
        return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_regions3d_map: the output overlaps the labels and is not the labels");
    cx_regions_state* R;
    const int32_t* dev;
    if ((rc = cxr_begin(ctx, S, &R, &dev))) return rc;
    hipStream_t st = ctx->stream;
    if ((rc = R->table.grow(ctx, (size_t)(n_map > 0 ? n_map : 1)))) return rc;
    if (n_map > 0) CX_HIP(ctx, hipMemcpyAsync(R->table, map, (size_t)n_map * sizeof(int32_t), hipMemcpyHostToDevice, st));
    int32_t* out = out_device;
    if (!out) {
        // for the host alone: the uploaded copy of host labels is mapped in place, device labels into a buffer of the state
        if (!S.on_device) out = const_cast<int32_t*>(dev);
        else {
            if ((rc = R->mapped.grow(ctx, S.bytes))) return rc;
            out = R->mapped.as<int32_t>();
        }
    }
    cxr_map_args A;
    memset(&A, 0, sizeof(A));
    A.labels = dev; A.table = R->table.get(); A.out = out; A.n_map = n_map; A.total = S.count;
    A.head = (size_t)(((16u - ((uintptr_t)out & 15u)) & 15u) / 4u);
    if (A.head > S.count) A.head = S.count;
    A.groups = (S.count - A.head) / 4u;
    hipLaunchKernelGGL(cxr_k_map, dim3(cxr_grid_flat(A.groups > 8u ? A.groups : 8u)), dim3(256), 0, st, A);      // (the loose samples are fewer than 8)
    CX_HIP(ctx, hipGetLastError());
    if (out_host) CX_HIP(ctx, hipMemcpyAsync(out_host, out, S.bytes, hipMemcpyDeviceToHost, st));
    CX_HIP(ctx, hipStreamSynchronize(st));
    return CX_OK;
}

extern "C" int cx_grid_regions3d_contacts(cx_ctx* ctx, const int32_t* labels, int on_device, int64_t n0, int64_t n1, int64_t n2,
                                          cx_region_contact* out_host, int64_t capacity, int64_t* n) {
    if (!ctx) return CX_ERR_INVALID;
    cx_source S;
    int rc = cxr_labels(ctx, "cx_grid_regions3d_contacts", labels, on_device, n0, n1, n2, &S);
    if (rc) return rc;
    cx_regions_state* R;
    const int32_t* dev;
    if ((rc = cxr_begin(ctx, S, &R, &dev))) return rc;
    hipStream_t st = ctx->stream;
    // the table of the call before is the first guess (a steady state allocates nothing and runs once)
    unsigned long long slots = CXR_TABLE_MIN;
    while (slots * 2ull <= (unsigned long long)R->pairs.cap()) slots *= 2ull;
    cxr_contact_args A;
    memset(&A, 0, sizeof(A));
    A.labels = dev; A.ctl = R->misc.get() + 3;
    A.n0 = n0; A.n1 = n1; A.n2 = n2; A.tiles = (n2 + 63) / 64;
    for (;; slots *= 2ull) {
        if (slots > CXR_TABLE_MAX) return cx_fail(ctx, CX_ERR_UNSUPPORTED, "cx_grid_regions3d_contacts: more pairs of labels than the largest table holds");
        if ((rc = R->pairs.grow(ctx, (size_t)slots))) return rc;
        A.tab = R->pairs.get(); A.mask = slots - 1ull;
        hipLaunchKernelGGL(cxr_k_pairs_init, dim3(cxr_grid_flat((size_t)slots)), dim3(256), 0, st, A.tab, (size_t)slots);
        CX_HIP(ctx, hipGetLastError());
        CX_HIP(ctx, hipMemsetAsync(A.ctl, 0, 2 * sizeof(u64), st));
        hipLaunchKernelGGL(cxr_k_contacts, dim3(cxr_grid_rows(n0 * n1)), dim3(256), 0, st, A);
        CX_HIP(ctx, hipGetLastError());
        u64 ctl[2] = {0, 0};
        CX_HIP(ctx, hipMemcpyAsync(ctl, A.ctl, sizeof(ctl), hipMemcpyDeviceToHost, st));
        CX_HIP(ctx, hipStreamSynchronize(st));
        if (!ctl[1]) break;
    }
    if ((rc = R->rank.grow(ctx, (size_t)slots)) || (rc = R->sums.grow(ctx, (size_t)slots / 1024u + 2u))) return rc;
    hipLaunchKernelGGL(cxr_k_occupied, dim3(cxr_grid_flat((size_t)slots)), dim3(256), 0, st, (const cxr_pair_slot*)A.tab, R->rank.get(), (uint32_t)slots);
    CX_HIP(ctx, hipGetLastError());
    uint32_t* total = reinterpret_cast<uint32_t*>(R->misc.get() + 5);
    if ((rc = cx_scan_u32(ctx, R->rank, R->rank, (uint32_t)slots, R->sums, total))) return rc;
    uint32_t found = 0;
    CX_HIP(ctx, hipMemcpyAsync(&found, total, sizeof(found), hipMemcpyDeviceToHost, st));
    CX_HIP(ctx, hipStreamSynchronize(st));
    if (n) *n = (int64_t)found;
    if (!out_host || found == 0u) return CX_OK;
    if (capacity < (int64_t)found) return cx_fail(ctx, CX_ERR_INVALID, "cx_grid_regions3d_contacts: room for fewer records than there are pairs");
    if ((rc = R->found.grow(ctx, (size_t)slots / 2u + 1u))) return rc;      // (what a table of this size can hold: the next call of this size allocates nothing)
    hipLaunchKernelGGL(cxr_k_collect, dim3(cxr_grid_flat((size_t)slots)), dim3(256), 0, st, (const cxr_pair_slot*)A.tab, (const uint32_t*)R->rank.get(), R->found.get(), (uint32_t)slots);
    CX_HIP(ctx, hipGetLastError());
    CX_HIP(ctx, hipMemcpyAsync(out_host, R->found.get(), (size_t)found * sizeof(cx_region_contact), hipMemcpyDeviceToHost, st));
    CX_HIP(ctx, hipStreamSynchronize(st));
    std::sort(out_host, out_host + found, [](const cx_region_contact& x, const cx_region_contact& y) { return x.a != y.a ? x.a < y.a : x.b < y.b; });
    return CX_OK;
}
