// cx_write.hip -- binary mesh files straight from the Level-1 device buffers (cx_level1_write).
//
// Reference semantics restated (paths relative to the reference checkout, contourist/...):
//   html_demo.py:118-161   positions, normals and faces as binary buffers: what every caller of the reference does next,
//                          here without the detour through Python arrays
// Reads the Level-1 state of cx_post.hip (cx_post.h) and nothing else of the post-pass.
#include <cstdio>
#include <string>

#include "cx_post.h"

// The file's records are laid out ON THE DEVICE, a chunk at a
// time (world coordinates = grid * delta + mins, rounded as numpy rounds them: no fused multiply-add), and streamed through two
// pinned staging buffers: the copy of chunk i+1 runs while chunk i is written to the file.
__global__ void cxw_k_points(const double* __restrict__ pts, uint32_t first, uint32_t n, double m0, double m1, double m2, double d0, double d1,
                             double d2, int as_f32, void* out) {
#pragma clang fp contract(off)   // grid * delta + mins with two roundings, as numpy computes it (a fused multiply-add differs in the last bit)
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* p = pts + (size_t)(first + i) * 3;
    const double x = p[0] * d0 + m0, y = p[1] * d1 + m1, z = p[2] * d2 + m2;
    if (as_f32) {
        float* o = reinterpret_cast<float*>(out) + (size_t)i * 3;
        o[0] = (float)x; o[1] = (float)y; o[2] = (float)z;
    } else {
        double* o = reinterpret_cast<double*>(out) + (size_t)i * 3;
        o[0] = x; o[1] = y; o[2] = z;
    }
}
// the same with the unit normal behind the position (CX_FILE_PLY_NORMALS: six doubles per vertex), and the normals alone as float32
// (the second section of CX_FILE_GLTF_BIN_NORMALS)
__global__ void cxw_k_points_normals(const double* __restrict__ pts, const double* __restrict__ nrm, uint32_t first, uint32_t n, double m0, double m1,
                                     double m2, double d0, double d1, double d2, double* out) {
#pragma clang fp contract(off)
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* p = pts + (size_t)(first + i) * 3;
    const double* q = nrm + (size_t)(first + i) * 3;
    double* o = out + (size_t)i * 6;
    o[0] = p[0] * d0 + m0; o[1] = p[1] * d1 + m1; o[2] = p[2] * d2 + m2;
    o[3] = q[0]; o[4] = q[1]; o[5] = q[2];
}
__global__ void cxw_k_normals_f32(const double* __restrict__ nrm, uint32_t first, uint32_t n, float* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* q = nrm + (size_t)(first + i) * 3;
    // (the rounded components of a float64 unit vector are 1 +- 1e-7 long)
    out[(size_t)i * 3] = (float)q[0]; out[(size_t)i * 3 + 1] = (float)q[1]; out[(size_t)i * 3 + 2] = (float)q[2];
}
// PLY faces: uchar 3 + three little-endian int32 = 13 bytes per triangle
__global__ void cxw_k_faces13(const int32_t* __restrict__ tri, uint32_t first, uint32_t n, uint8_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint8_t* o = out + (size_t)i * 13;
    o[0] = 3;
    for (int k = 0; k < 3; k++) {
        const uint32_t v = (uint32_t)tri[(size_t)(first + i) * 3 + k];
        o[1 + 4 * k] = (uint8_t)v; o[2 + 4 * k] = (uint8_t)(v >> 8); o[3 + 4 * k] = (uint8_t)(v >> 16); o[4 + 4 * k] = (uint8_t)(v >> 24);
    }
}
extern "C" int cx_level1_write(cx_ctx* ctx, int format, const char* path, const double* mins_delta, double* out_info) {
    if (!ctx || !path || (format != CX_FILE_PLY && format != CX_FILE_GLTF_BIN && format != CX_FILE_PLY_NORMALS && format != CX_FILE_GLTF_BIN_NORMALS)) return CX_ERR_INVALID;
    if (!cxp_mesh3d(ctx)) { ctx->err = "cx_level1_write: run cx_postprocess3d first"; return CX_ERR_STATE; }
    CX_HIP(ctx, hipSetDevice(ctx->device));
    cx_post_state* S = ctx->post;
    // the formats with normals: the unit normals of cx_level1_normals (world normals when a spacing is handed over), laid out like the positions
    const bool with_normals = format == CX_FILE_PLY_NORMALS || format == CX_FILE_GLTF_BIN_NORMALS;
    const double* nrm = nullptr;
    if (with_normals) {
        void* nd = nullptr;
        const int rcn = cx_level1_normals(ctx, mins_delta ? mins_delta + 3 : nullptr, &nd);
        if (rcn) return rcn;
        nrm = (const double*)nd;
        format = format == CX_FILE_PLY_NORMALS ? CX_FILE_PLY : CX_FILE_GLTF_BIN;
    }
    hipStream_t st = ctx->stream;
    const uint32_t nv = (uint32_t)S->nv_out, nt = (uint32_t)S->nt_out;
    double m[3] = {0, 0, 0}, d[3] = {1, 1, 1};
    if (mins_delta) for (int a = 0; a < 3; a++) { m[a] = mins_delta[a]; d[a] = mins_delta[3 + a]; }
    const uint32_t CHUNK = 1u << 20;                       // elements per chunk
    const size_t stage_bytes = (size_t)CHUNK * (with_normals ? 48u : 24u);   // the widest record: 3 doubles (6 with normals)
    cx_buf<uint8_t> dstage;
    uint8_t* hstage[2] = {nullptr, nullptr};
    FILE* f = fopen(path, "wb");
    if (!f) { ctx->err = std::string("cx_level1_write: cannot open ") + path; return CX_ERR_INVALID; }
    int rc = CX_OK;
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    size_t written = 0;
    do {
        hipError_t e;
#define CXW_TRY(call) if ((e = (call)) != hipSuccess) { ctx->err = std::string(#call) + ": " + hipGetErrorString(e); rc = (e == hipErrorOutOfMemory) ? CX_ERR_NOMEM : CX_ERR_HIP; break; }
        if ((rc = dstage.grow(ctx, 2 * stage_bytes))) break;
        CXW_TRY(hipHostMalloc(&hstage[0], stage_bytes));
        CXW_TRY(hipHostMalloc(&hstage[1], stage_bytes));
        if (format == CX_FILE_PLY) {
            char header[512];
            const int hl = snprintf(header, sizeof(header),
                                    "ply\nformat binary_little_endian 1.0\ncomment contourist_amd isosurface\nelement vertex %u\n"
                                    "property double x\nproperty double y\nproperty double z\n%s"
                                    "element face %u\nproperty list uchar int vertex_indices\nend_header\n", nv,
                                    with_normals ? "property double nx\nproperty double ny\nproperty double nz\n" : "", nt);
            if (fwrite(header, 1, (size_t)hl, f) != (size_t)hl) { rc = CX_ERR_INVALID; ctx->err = "cx_level1_write: write failed"; break; }
            written += (size_t)hl;
        }
        // section 0: points, section 1: faces / indices.  Chunk c of a section is prepared on the device into half c & 1 of
        // dstage and copied to hstage[c & 1]; the previous chunk is written to the file meanwhile.
        // (glTF with normals: a section 2 of float32 normals between the two; PLY with normals: six doubles per vertex in section 0)
        const int order3[3] = {0, 2, 1}, order2[3] = {0, 1, 1};
        const bool three = with_normals && format != CX_FILE_PLY;
        for (int si = 0; si < (three ? 3 : 2) && rc == CX_OK; si++) {
            const int section = three ? order3[si] : order2[si];
            const uint32_t count = section == 1 ? nt : nv;
            const size_t rec = section == 0 ? (format == CX_FILE_PLY ? (with_normals ? 48u : 24u) : 12u) : (section == 2 ? 12u : (format == CX_FILE_PLY ? 13u : 12u));
            size_t pending_bytes = 0;
            int pending = -1;
            for (uint32_t first = 0, c = 0; rc == CX_OK; first += CHUNK, c++) {
                const bool more = first < count;
                const uint32_t n = more ? std::min(CHUNK, count - first) : 0u;
                const int half = (int)(c & 1u);
                if (more) {
                    uint8_t* dst = dstage + (size_t)half * stage_bytes;
                    if (section == 0 && with_normals && format == CX_FILE_PLY)
                        hipLaunchKernelGGL(cxw_k_points_normals, dim3(cx_blocks(n)), dim3(256), 0, st, S->pts_out.as<const double>(), nrm, first, n, m[0], m[1], m[2],
                                           d[0], d[1], d[2], (double*)dst);
                    else if (section == 0)
                        hipLaunchKernelGGL(cxw_k_points, dim3(cx_blocks(n)), dim3(256), 0, st, S->pts_out.as<const double>(), first, n, m[0], m[1], m[2],
                                           d[0], d[1], d[2], format == CX_FILE_PLY ? 0 : 1, (void*)dst);
                    else if (section == 2)
                        hipLaunchKernelGGL(cxw_k_normals_f32, dim3(cx_blocks(n)), dim3(256), 0, st, nrm, first, n, (float*)dst);
                    else if (format == CX_FILE_PLY)
                        hipLaunchKernelGGL(cxw_k_faces13, dim3(cx_blocks(n)), dim3(256), 0, st, S->tri_out.as<const int32_t>(), first, n, dst);
                    const void* src = (section == 1 && format != CX_FILE_PLY) ? (const void*)(S->tri_out.as<const int32_t>() + (size_t)first * 3) : (const void*)dst;
                    e = hipMemcpyAsync(hstage[half], src, (size_t)n * rec, hipMemcpyDeviceToHost, st);
                    if (e != hipSuccess) { ctx->err = std::string("hipMemcpyAsync: ") + hipGetErrorString(e); rc = CX_ERR_HIP; break; }
                }
                if (pending >= 0) {   // the previous chunk is complete (synchronised below, last iteration); the one just enqueued copies meanwhile
                    if (fwrite(hstage[pending], 1, pending_bytes, f) != pending_bytes) { rc = CX_ERR_INVALID; ctx->err = "cx_level1_write: write failed"; break; }
                    written += pending_bytes;
                }
                if (!more) break;
                e = hipStreamSynchronize(st);
                if (e != hipSuccess) { ctx->err = std::string("hipStreamSynchronize: ") + hipGetErrorString(e); rc = CX_ERR_HIP; break; }
                if (section == 0) {   // bounds of the positions (glTF needs them in its JSON; reported for both formats)
                    if (format != CX_FILE_PLY) {
                        const float* q = reinterpret_cast<const float*>(hstage[half]);
                        for (uint32_t i = 0; i < n; i++)
                            for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], (double)q[3 * i + a]); hi[a] = std::max(hi[a], (double)q[3 * i + a]); }
                    } else {
                        const double* q = reinterpret_cast<const double*>(hstage[half]);
                        const size_t stride = with_normals ? 6u : 3u;
                        for (uint32_t i = 0; i < n; i++)
                            for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], q[stride * i + a]); hi[a] = std::max(hi[a], q[stride * i + a]); }
                    }
                }
                pending = half;
                pending_bytes = (size_t)n * rec;
            }
        }
#undef CXW_TRY
    } while (0);
    // a short write may only surface when the buffered bytes are flushed (disk full): check both, and leave no partial file
    if (fflush(f) != 0 && rc == CX_OK) { rc = CX_ERR_INVALID; ctx->err = "cx_level1_write: write failed (flush)"; }
    if (fclose(f) != 0 && rc == CX_OK) { rc = CX_ERR_INVALID; ctx->err = "cx_level1_write: write failed (close)"; }
    for (int k = 0; k < 2; k++)
        if (hstage[k]) (void)hipHostFree(hstage[k]);
    if (rc) { (void)remove(path); return rc; }
    if (out_info) {
        out_info[0] = (double)nv; out_info[1] = (double)nt; out_info[2] = (double)written;
        for (int a = 0; a < 3; a++) { out_info[3 + a] = nv ? lo[a] : 0.0; out_info[6 + a] = nv ? hi[a] : 0.0; }
    }
    return CX_OK;
}
