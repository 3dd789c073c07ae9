// Occupancy grid from the mesh, and what a ray needs of it: the conservative triangle-to-cell voxeliser (voxelize), the cube dilation of
// the byte grid (dilate), and per ray the span between its first and its last occupied cell (ray_spans).
// Built with -ffp-contract=off: every product, sum and quotient below rounds on its own, in the order written, so the numpy
// restatements (tests/test_occupancy_mesh_cpu.py) give the same bits; they are the definition, this file follows them line by line.
// No atomics.  The voxeliser only ever stores the byte 1 (as k_texel_mark / k_vc_seen do): racing stores write the same value, the
// caller zeroes the grid, several calls accumulate a union.  Every other output element has one writer.
#include "occ_tri.h"

#define OCM_BLK 256
#define OCM_CAP 2048          // blocks of a grid-stride launch: 8 per CU

// ---- voxeliser: one wave per triangle, the lanes stride over the candidate cells of its bounding box, x fastest --------------------
// The triangle index is wave-uniform, so the vertex loads are scalar loads and the set-up (normal, plane terms, nine edge terms) is done
// once per wave, outside the cell loop; per cell a lane evaluates the plane pair and nine edge functions of Schwarz and Seidel's
// conservative test on the inflated box.  Set-up and test are occ_tri.h's, shared with the cell triangle lists of meshhit.hip.
__global__ __launch_bounds__(OCM_BLK) void k_occ_voxelize(const float *__restrict__ vtx, const int64_t *__restrict__ faces, int64_t V, int64_t F, int G,
                                                          ocm3 lo, ocm3 inv, uint8_t *__restrict__ cells)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = __builtin_amdgcn_readfirstlane((int)(((int64_t)blockIdx.x * OCM_BLK + threadIdx.x) >> 6));
    const int64_t nwaves = ((int64_t)gridDim.x * OCM_BLK) >> 6;
    for (int64_t f = wave0; f < F; f += nwaves) {
        OccTri T;
        if (!occ_tri_setup(vtx, faces, V, f, G, lo, inv, T)) continue;
        for (int i = lane; i < T.total; i += 64) {
            int cx, cy, cz;
            occ_tri_candidate(T, i, cx, cy, cz);
            if (occ_tri_cell(T, cx, cy, cz)) cells[((int64_t)cz * G + cy) * G + cx] = 1;       // 0 <= c < G on the three axes by the set-up's clamps
        }
    }
}

extern "C" int32_t ctx_occ_voxelize(const float *vertices, const int64_t *faces, int64_t V, int64_t F, int32_t G, float lo_x, float lo_y, float lo_z,
                                    float inv_x, float inv_y, float inv_z, uint8_t *cells, ctx_stream_t stream)
{
    CTX_REQUIRE(vertices && faces && cells, "occ_voxelize: null pointer");
    CTX_REQUIRE(G >= 1 && G <= 256, "occ_voxelize: G=%d outside [1, 256]", (int)G);
    CTX_REQUIRE(V >= 1 && F >= 1, "occ_voxelize: V=%lld, F=%lld: want at least one vertex and one face", (long long)V, (long long)F);
    CTX_REQUIRE(V <= INT32_MAX && F <= INT32_MAX, "occ_voxelize: V=%lld, F=%lld: want both below 2^31", (long long)V, (long long)F);
    const ocm3 lo = {lo_x, lo_y, lo_z}, inv = {inv_x, inv_y, inv_z};
    hipLaunchKernelGGL(k_occ_voxelize, dim3(capped_blocks(F, OCM_BLK / 64, OCM_CAP)), dim3(OCM_BLK), 0, (hipStream_t)stream, vertices, faces, V, F,
                       (int)G, lo, inv, cells);
    CTX_CHECK_LAUNCH("occ_voxelize");
    return CTX_OK;
}

// ---- dilation: one pass per axis, dst[c] = any of src within +-k along that axis (clamped to the grid) -------------------------------
__global__ __launch_bounds__(OCM_BLK) void k_occ_dilate_axis(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int G, int k, int64_t stride,
                                                             int64_t n)
{
    for (int64_t c = (int64_t)blockIdx.x * OCM_BLK + threadIdx.x; c < n; c += (int64_t)gridDim.x * OCM_BLK) {
        const int a = (int)((c / stride) % G);
        const int j0 = a - k > 0 ? a - k : 0, j1 = a + k < G - 1 ? a + k : G - 1;
        uint8_t any = 0;
        for (int j = j0; j <= j1; ++j) any |= src[c + (int64_t)(j - a) * stride];          // same line and column: inside [0, n)
        dst[c] = any ? 1 : 0;
    }
}

extern "C" int32_t ctx_occ_dilate(const uint8_t *src, int32_t G, int32_t k, uint8_t *dst, uint8_t *ws, ctx_stream_t stream)
{
    CTX_REQUIRE(src && dst, "occ_dilate: null pointer");
    CTX_REQUIRE(G >= 1 && G <= 256, "occ_dilate: G=%d outside [1, 256]", (int)G);
    CTX_REQUIRE(k >= 0, "occ_dilate: k=%d: want k >= 0", (int)k);
    if (k > G) k = G;                                                 // the grid has G cells per axis: a wider cube reaches no further
    CTX_REQUIRE(src != dst, "occ_dilate: dst must not be src");
    CTX_REQUIRE(k == 0 || (ws && ws != src && ws != dst), "occ_dilate: k=%d needs a workspace of G^3 bytes that is neither src nor dst", (int)k);
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)G * G * G;
    const dim3 grid(capped_blocks(n, OCM_BLK, OCM_CAP)), blk(OCM_BLK);
    if (k == 0) {
        hipLaunchKernelGGL(k_occ_dilate_axis, grid, blk, 0, s, src, dst, (int)G, 0, (int64_t)1, n);              // the copy (non-zero -> 1)
    } else {
        hipLaunchKernelGGL(k_occ_dilate_axis, grid, blk, 0, s, src, dst, (int)G, (int)k, (int64_t)1, n);         // x
        hipLaunchKernelGGL(k_occ_dilate_axis, grid, blk, 0, s, (const uint8_t *)dst, ws, (int)G, (int)k, (int64_t)G, n);          // y
        hipLaunchKernelGGL(k_occ_dilate_axis, grid, blk, 0, s, (const uint8_t *)ws, dst, (int)G, (int)k, (int64_t)G * G, n);      // z
    }
    CTX_CHECK_LAUNCH("occ_dilate");
    return CTX_OK;
}

// ---- spans: one lane per ray; the cell walk is occ_walk (occ_walk.h), shared with the march kernels -------------------------------------
__global__ __launch_bounds__(OCM_BLK) void k_occ_ray_spans(const float *__restrict__ ro, const float *__restrict__ rd, int64_t R, float near, float far,
                                                           const uint8_t *__restrict__ cells, int G, ocm3 lo, ocm3 hi, ocm3 inv, ocm3 h,
                                                           float2 *__restrict__ span, uint8_t *__restrict__ hit)
{
    for (int64_t r = (int64_t)blockIdx.x * OCM_BLK + threadIdx.x; r < R; r += (int64_t)gridDim.x * OCM_BLK) {
        float s0 = near, s1 = far;
        bool found = false;
        occ_walk(ro[r * 3 + 0], ro[r * 3 + 1], ro[r * 3 + 2], rd[r * 3 + 0], rd[r * 3 + 1], rd[r * 3 + 2], near, far, cells, G, lo, hi, inv, h,
                 [&](bool occ, float tin, float tout) {
                     if (occ) {
                         if (!found) { s0 = tin; found = true; }
                         s1 = tout;
                     }
                 });
        span[r] = make_float2(s0, s1);
        hit[r] = found ? 1 : 0;
    }
}

extern "C" int32_t ctx_occ_ray_spans(const float *rays_o, const float *rays_d, int64_t R, float near, float far, const uint8_t *cells, int32_t G,
                                     float lo_x, float lo_y, float lo_z, float hi_x, float hi_y, float hi_z, float inv_x, float inv_y, float inv_z,
                                     float h_x, float h_y, float h_z, float *span, uint8_t *hit, ctx_stream_t stream)
{
    CTX_REQUIRE(rays_o && rays_d && cells && span && hit, "occ_ray_spans: null pointer");
    CTX_REQUIRE(G >= 1 && G <= 256, "occ_ray_spans: G=%d outside [1, 256]", (int)G);
    CTX_REQUIRE(R >= 1 && R <= INT32_MAX, "occ_ray_spans: R=%lld outside [1, 2^31)", (long long)R);
    CTX_REQUIRE(near < far && fabsf(near) < INFINITY && fabsf(far) < INFINITY, "occ_ray_spans: want finite near < far, got %g, %g", (double)near,
                (double)far);
    CTX_REQUIRE(((uintptr_t)span % 8) == 0, "occ_ray_spans: span must be 8-byte aligned");
    const ocm3 lo = {lo_x, lo_y, lo_z}, hi = {hi_x, hi_y, hi_z}, inv = {inv_x, inv_y, inv_z}, h = {h_x, h_y, h_z};
    hipLaunchKernelGGL(k_occ_ray_spans, dim3(capped_blocks(R, OCM_BLK, OCM_CAP)), dim3(OCM_BLK), 0, (hipStream_t)stream, rays_o, rays_d, R, near, far,
                       cells, (int)G, lo, hi, inv, h, (float2 *)span, hit);
    CTX_CHECK_LAUNCH("occ_ray_spans");
    return CTX_OK;
}
