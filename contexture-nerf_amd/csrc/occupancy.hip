// Occupancy grid of the ray path: which samples of a ray batch lie in occupied cells (mark), their points and the expansion of the
// field's compact output back to [R,S,4] (points / expand / collect), and the grid's own refresh (cell_points / update).
// Built with -ffp-contract=off: every product and sum below rounds on its own, in the order written, so a numpy restatement
// (tests/test_occupancy_cpu.py) and the torch expression `ro + rd * z` give the same bits.
// Streaming kernels, grid-stride, no atomics.  An element of `raw` has one writer per launch: ctx_occ_expand is two launches on one
// stream (fill, then the listed rows), so a listed row is stored twice, in stream order, with the same result on every run.
#include "common.h"

#define OCC_BLK 256
#define OCC_CAP 2048          // blocks of a grid-stride launch: 8 per CU

struct occ3 { float x, y, z; };

// mask byte of one sample: p = o + d*z, t = (p - lo)*inv, inside when 0 <= t < G on the three axes (false for NaN), then cells[(int)t]
__device__ __forceinline__ uint8_t occ_mark_one(occ3 o, occ3 d, float zv, const uint8_t *__restrict__ cells, int G, float Gf, occ3 lo, occ3 inv)
{
    const float px = o.x + d.x * zv, py = o.y + d.y * zv, pz = o.z + d.z * zv;
    const float tx = (px - lo.x) * inv.x, ty = (py - lo.y) * inv.y, tz = (pz - lo.z) * inv.z;
    const bool in = tx >= 0.f && tx < Gf && ty >= 0.f && ty < Gf && tz >= 0.f && tz < Gf;
    if (!in) return 0;
    const int cx = (int)tx, cy = (int)ty, cz = (int)tz;          // < G: t < (float)G and the conversion truncates
    return cells[((int64_t)cz * G + cy) * G + cx];
}

// S >= 64: one wave per ray.  The ray index is wave-uniform, so o / d are read once per wave (scalar loads); the lanes sweep the ray's
// samples, four per lane (16-byte z loads, 4-byte mask stores) when VEC (S % 4 == 0 and aligned bases), else one per lane.
template <bool VEC>
__global__ __launch_bounds__(OCC_BLK) void k_occ_mark_ray(const float *__restrict__ ro, const float *__restrict__ rd, const float *__restrict__ z,
                                                          int64_t R, int S, const uint8_t *__restrict__ cells, int G, occ3 lo, occ3 inv,
                                                          uint8_t *__restrict__ mask)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = __builtin_amdgcn_readfirstlane((int)(((int64_t)blockIdx.x * OCC_BLK + threadIdx.x) >> 6));
    const int64_t nwaves = ((int64_t)gridDim.x * OCC_BLK) >> 6;
    const float Gf = (float)G;
    for (int64_t r = wave0; r < R; r += nwaves) {
        const occ3 o = {ro[r * 3 + 0], ro[r * 3 + 1], ro[r * 3 + 2]};
        const occ3 d = {rd[r * 3 + 0], rd[r * 3 + 1], rd[r * 3 + 2]};
        const float *zr = z + r * S;
        uint8_t *mr = mask + r * S;
        if (VEC) {
            for (int s = lane * 4; s < S; s += 256) {             // S % 4 == 0: s + 3 < S
                const float4 zv = *reinterpret_cast<const float4 *>(zr + s);
                uchar4 m;
                m.x = occ_mark_one(o, d, zv.x, cells, G, Gf, lo, inv);
                m.y = occ_mark_one(o, d, zv.y, cells, G, Gf, lo, inv);
                m.z = occ_mark_one(o, d, zv.z, cells, G, Gf, lo, inv);
                m.w = occ_mark_one(o, d, zv.w, cells, G, Gf, lo, inv);
                *reinterpret_cast<uchar4 *>(mr + s) = m;
            }
        } else {
            for (int s = lane; s < S; s += 64) mr[s] = occ_mark_one(o, d, zr[s], cells, G, Gf, lo, inv);
        }
    }
}

// S < 64: one sample per lane over the flat [R*S] range
__global__ __launch_bounds__(OCC_BLK) void k_occ_mark_flat(const float *__restrict__ ro, const float *__restrict__ rd, const float *__restrict__ z,
                                                           int64_t total, int S, const uint8_t *__restrict__ cells, int G, occ3 lo, occ3 inv,
                                                           uint8_t *__restrict__ mask)
{
    const float Gf = (float)G;
    for (int64_t i = (int64_t)blockIdx.x * OCC_BLK + threadIdx.x; i < total; i += (int64_t)gridDim.x * OCC_BLK) {
        const int64_t r = i / S;
        const occ3 o = {ro[r * 3 + 0], ro[r * 3 + 1], ro[r * 3 + 2]};
        const occ3 d = {rd[r * 3 + 0], rd[r * 3 + 1], rd[r * 3 + 2]};
        mask[i] = occ_mark_one(o, d, z[i], cells, G, Gf, lo, inv);
    }
}

extern "C" int32_t ctx_occ_mark(const float *rays_o, const float *rays_d, const float *z_vals, int64_t R, int32_t S, const uint8_t *cells,
                                int32_t G, float lo_x, float lo_y, float lo_z, float inv_x, float inv_y, float inv_z, uint8_t *mask,
                                ctx_stream_t stream)
{
    CTX_REQUIRE(rays_o && rays_d && z_vals && cells && mask, "occ_mark: null pointer");
    CTX_REQUIRE(G >= 1 && G <= 256, "occ_mark: G=%d outside [1, 256]", (int)G);
    CTX_REQUIRE(R >= 1 && S >= 1, "occ_mark: R=%lld, S=%d: want at least one ray and one sample", (long long)R, (int)S);
    CTX_REQUIRE(R <= INT32_MAX / (int64_t)S, "occ_mark: R*S=%lld x %d does not fit the int32 sample indices (R*S < 2^31)", (long long)R, (int)S);
    hipStream_t s = (hipStream_t)stream;
    const occ3 lo = {lo_x, lo_y, lo_z}, inv = {inv_x, inv_y, inv_z};
    if (S >= 64) {
        const bool vec = (S % 4) == 0 && ((uintptr_t)z_vals % 16) == 0 && ((uintptr_t)mask % 4) == 0;
        const unsigned nb = capped_blocks(R, OCC_BLK / 64, OCC_CAP);
        CTX_BOOL_GO(vec, V, hipLaunchKernelGGL(k_occ_mark_ray<V>, dim3(nb), dim3(OCC_BLK), 0, s, rays_o, rays_d, z_vals, R, (int)S, cells,
                                               (int)G, lo, inv, mask));
    } else {
        const int64_t total = R * S;
        hipLaunchKernelGGL(k_occ_mark_flat, dim3(capped_blocks(total, OCC_BLK, OCC_CAP)), dim3(OCC_BLK), 0, s, rays_o, rays_d, z_vals, total,
                           (int)S, cells, (int)G, lo, inv, mask);
    }
    CTX_CHECK_LAUNCH("occ_mark");
    return CTX_OK;
}

// pts[k] = o + d*z of sample idx[k]: the expression of the mark kernel and of `ro + rd * z`, so the compact points carry the dense bits
__global__ __launch_bounds__(OCC_BLK) void k_occ_points(const float *__restrict__ ro, const float *__restrict__ rd, const float *__restrict__ z,
                                                        int64_t total, int S, const int32_t *__restrict__ idx, int64_t n, float *__restrict__ pts)
{
    for (int64_t k = (int64_t)blockIdx.x * OCC_BLK + threadIdx.x; k < n; k += (int64_t)gridDim.x * OCC_BLK) {
        const int64_t i = idx[k];
        if (i < 0 || i >= total) continue;
        const int64_t r = i / S;
        const float zv = z[i];
        pts[k * 3 + 0] = ro[r * 3 + 0] + rd[r * 3 + 0] * zv;
        pts[k * 3 + 1] = ro[r * 3 + 1] + rd[r * 3 + 1] * zv;
        pts[k * 3 + 2] = ro[r * 3 + 2] + rd[r * 3 + 2] * zv;
    }
}

extern "C" int32_t ctx_occ_points(const float *rays_o, const float *rays_d, const float *z_vals, int64_t R, int32_t S, const int32_t *idx,
                                  int64_t n, float *pts, ctx_stream_t stream)
{
    CTX_REQUIRE(rays_o && rays_d && z_vals && idx && pts, "occ_points: null pointer");
    CTX_REQUIRE(R >= 1 && S >= 1 && R <= INT32_MAX / (int64_t)S, "occ_points: R=%lld, S=%d: want 1 <= R*S < 2^31", (long long)R, (int)S);
    CTX_REQUIRE(n >= 1 && n <= R * S, "occ_points: n=%lld outside [1, R*S=%lld]", (long long)n, (long long)(R * S));
    hipLaunchKernelGGL(k_occ_points, dim3(capped_blocks(n, OCC_BLK, OCC_CAP)), dim3(OCC_BLK), 0, (hipStream_t)stream, rays_o, rays_d, z_vals,
                       R * S, (int)S, idx, n, pts);
    CTX_CHECK_LAUNCH("occ_points");
    return CTX_OK;
}

// the fill: zero colour, a density no noise lifts above zero, and finite
__global__ __launch_bounds__(OCC_BLK) void k_occ_fill(float4 *__restrict__ raw, int64_t total)
{
    const float4 fill = make_float4(0.f, 0.f, 0.f, -1e30f);
    for (int64_t i = (int64_t)blockIdx.x * OCC_BLK + threadIdx.x; i < total; i += (int64_t)gridDim.x * OCC_BLK) raw[i] = fill;
}

__global__ __launch_bounds__(OCC_BLK) void k_occ_scatter(const float4 *__restrict__ raw_c, const int32_t *__restrict__ idx, int64_t n, int64_t total,
                                                         float4 *__restrict__ raw)
{
    for (int64_t k = (int64_t)blockIdx.x * OCC_BLK + threadIdx.x; k < n; k += (int64_t)gridDim.x * OCC_BLK) {
        const int64_t i = idx[k];
        if (i >= 0 && i < total) raw[i] = raw_c[k];
    }
}

extern "C" int32_t ctx_occ_expand(const float *raw_c, const int32_t *idx, int64_t n, int64_t total, float *raw, ctx_stream_t stream)
{
    CTX_REQUIRE(raw, "occ_expand: null output");
    CTX_REQUIRE(total >= 1 && total <= INT32_MAX, "occ_expand: total=%lld outside [1, 2^31)", (long long)total);
    CTX_REQUIRE(n >= 0 && n <= total, "occ_expand: n=%lld outside [0, total=%lld]", (long long)n, (long long)total);
    CTX_REQUIRE(n == 0 || (raw_c && idx), "occ_expand: null list with n=%lld", (long long)n);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_occ_fill, dim3(capped_blocks(total, OCC_BLK, OCC_CAP)), dim3(OCC_BLK), 0, s, (float4 *)raw, total);
    if (n > 0)
        hipLaunchKernelGGL(k_occ_scatter, dim3(capped_blocks(n, OCC_BLK, OCC_CAP)), dim3(OCC_BLK), 0, s, (const float4 *)raw_c, idx, n, total,
                           (float4 *)raw);
    CTX_CHECK_LAUNCH("occ_expand");
    return CTX_OK;
}

// backward of the expansion: grad_c[k] = grad[idx[k]]; a skipped entry reads nothing and gets zero
__global__ __launch_bounds__(OCC_BLK) void k_occ_collect(const float4 *__restrict__ grad, const int32_t *__restrict__ idx, int64_t n, int64_t total,
                                                         float4 *__restrict__ grad_c)
{
    for (int64_t k = (int64_t)blockIdx.x * OCC_BLK + threadIdx.x; k < n; k += (int64_t)gridDim.x * OCC_BLK) {
        const int64_t i = idx[k];
        grad_c[k] = (i >= 0 && i < total) ? grad[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

extern "C" int32_t ctx_occ_collect(const float *grad, const int32_t *idx, int64_t n, int64_t total, float *grad_c, ctx_stream_t stream)
{
    CTX_REQUIRE(grad && idx && grad_c, "occ_collect: null pointer");
    CTX_REQUIRE(total >= 1 && total <= INT32_MAX, "occ_collect: total=%lld outside [1, 2^31)", (long long)total);
    CTX_REQUIRE(n >= 1 && n <= total, "occ_collect: n=%lld outside [1, total=%lld]", (long long)n, (long long)total);
    hipLaunchKernelGGL(k_occ_collect, dim3(capped_blocks(n, OCC_BLK, OCC_CAP)), dim3(OCC_BLK), 0, (hipStream_t)stream, (const float4 *)grad, idx, n,
                       total, (float4 *)grad_c);
    CTX_CHECK_LAUNCH("occ_collect");
    return CTX_OK;
}

// the point of cell c = (cz*G + cy)*G + cx the field is asked at: lo + ((float)c_axis + u)*h, u = 0.5 (the centre) or the given jitter
__global__ __launch_bounds__(OCC_BLK) void k_occ_cell_points(int G, occ3 lo, occ3 h, const float *__restrict__ u, float *__restrict__ pts)
{
    const int64_t n = (int64_t)G * G * G;
    for (int64_t c = (int64_t)blockIdx.x * OCC_BLK + threadIdx.x; c < n; c += (int64_t)gridDim.x * OCC_BLK) {
        const int cx = (int)(c % G), cy = (int)((c / G) % G), cz = (int)(c / ((int64_t)G * G));
        const float ux = u ? u[c * 3 + 0] : 0.5f, uy = u ? u[c * 3 + 1] : 0.5f, uz = u ? u[c * 3 + 2] : 0.5f;
        pts[c * 3 + 0] = lo.x + ((float)cx + ux) * h.x;
        pts[c * 3 + 1] = lo.y + ((float)cy + uy) * h.y;
        pts[c * 3 + 2] = lo.z + ((float)cz + uz) * h.z;
    }
}

extern "C" int32_t ctx_occ_cell_points(int32_t G, float lo_x, float lo_y, float lo_z, float h_x, float h_y, float h_z, const float *u, float *pts,
                                       ctx_stream_t stream)
{
    CTX_REQUIRE(pts, "occ_cell_points: null output");
    CTX_REQUIRE(G >= 1 && G <= 256, "occ_cell_points: G=%d outside [1, 256]", (int)G);
    const occ3 lo = {lo_x, lo_y, lo_z}, h = {h_x, h_y, h_z};
    hipLaunchKernelGGL(k_occ_cell_points, dim3(capped_blocks((int64_t)G * G * G, OCC_BLK, OCC_CAP)), dim3(OCC_BLK), 0, (hipStream_t)stream, (int)G,
                       lo, h, u, pts);
    CTX_CHECK_LAUNCH("occ_cell_points");
    return CTX_OK;
}

// dens = max(dens*decay, relu(raw.w)), cells = dens > thresh; a NaN density keeps dens (fmaxf drops it) and marks the cell occupied
__global__ __launch_bounds__(OCC_BLK) void k_occ_update(const float4 *__restrict__ raw, float *__restrict__ dens, uint8_t *__restrict__ cells, int64_t n,
                                                        float decay, float thresh)
{
    for (int64_t c = (int64_t)blockIdx.x * OCC_BLK + threadIdx.x; c < n; c += (int64_t)gridDim.x * OCC_BLK) {
        const float w = raw[c].w;
        const float sigma = w > 0.f ? w : 0.f;
        const float dn = fmaxf(dens[c] * decay, sigma);
        dens[c] = dn;
        cells[c] = (dn > thresh || w != w) ? 1 : 0;
    }
}

extern "C" int32_t ctx_occ_update(const float *raw, float *dens, uint8_t *cells, int64_t n, float decay, float thresh, ctx_stream_t stream)
{
    CTX_REQUIRE(raw && dens && cells, "occ_update: null pointer");
    CTX_REQUIRE(n >= 1 && n <= (int64_t)256 * 256 * 256, "occ_update: n=%lld outside [1, 256^3]", (long long)n);
    hipLaunchKernelGGL(k_occ_update, dim3(capped_blocks(n, OCC_BLK, OCC_CAP)), dim3(OCC_BLK), 0, (hipStream_t)stream, (const float4 *)raw, dens, cells,
                       n, decay, thresh);
    CTX_CHECK_LAUNCH("occ_update");
    return CTX_OK;
}
