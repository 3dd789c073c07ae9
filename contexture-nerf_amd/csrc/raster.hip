// Vertex preparation, the rasteriser and depth normalisation for gfx950.  HBM-bound integer+float32 work: no MFMA here.
// Compiled with -ffp-contract=off: every float op below is one IEEE binary32 op in source order,
// mirroring oracle/geometry_ref.c so face indices AND interpolated floats compare bit-exactly.
// Reference call sites replaced (include/ctx_nerf.h cites them per entry): src/models/render.py:112-157
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------------
// prepare_vertices: two tiny kernels (vertex transform, then per-face gather + normal).
__global__ void k_vertex_transform(const float *__restrict__ verts, const float *__restrict__ cam,
                                   const float *__restrict__ proj3, int V, float *__restrict__ vc,
                                   float *__restrict__ vi)
{
    int b = blockIdx.y;
    int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const float *M = cam + (size_t)b * 12;
    const float *p = verts + ((size_t)b * V + v) * 3;
    float x = p[0], y = p[1], z = p[2];
    float o[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float acc = x * M[0 * 3 + k];
        acc = acc + y * M[1 * 3 + k];
        acc = acc + z * M[2 * 3 + k];
        acc = acc + M[3 * 3 + k];
        o[k] = acc;
    }
    float *q = vc + ((size_t)b * V + v) * 3;
    q[0] = o[0]; q[1] = o[1]; q[2] = o[2];
    float px = o[0] * proj3[0], py = o[1] * proj3[1], pz = o[2] * proj3[2];
    vi[((size_t)b * V + v) * 2 + 0] = px / pz;
    vi[((size_t)b * V + v) * 2 + 1] = py / pz;
}

__global__ void k_face_gather(const float *__restrict__ vc, const float *__restrict__ vi,
                              const int64_t *__restrict__ faces, int V, int F,
                              float *__restrict__ fv_cam, float *__restrict__ fv_img,
                              float *__restrict__ fnorm)
{
    int b = blockIdx.y;
    int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    float p[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int64_t vid = faces[(size_t)f * 3 + k];
        const float *s = vc + ((size_t)b * V + vid) * 3;
        p[k][0] = s[0]; p[k][1] = s[1]; p[k][2] = s[2];
        float *d = fv_cam + (((size_t)b * F + f) * 3 + k) * 3;
        d[0] = p[k][0]; d[1] = p[k][1]; d[2] = p[k][2];
        const float *si = vi + ((size_t)b * V + vid) * 2;
        float *di = fv_img + (((size_t)b * F + f) * 3 + k) * 2;
        di[0] = si[0]; di[1] = si[1];
    }
    float e0x = p[1][0] - p[0][0], e0y = p[1][1] - p[0][1], e0z = p[1][2] - p[0][2];
    float e1x = p[2][0] - p[0][0], e1y = p[2][1] - p[0][1], e1z = p[2][2] - p[0][2];
    float nx = e0y * e1z - e0z * e1y;
    float ny = e0z * e1x - e0x * e1z;
    float nz = e0x * e1y - e0y * e1x;
    float len = sqrtf((nx * nx + ny * ny) + nz * nz);
    float d = len + 1e-10f;
    float *o = fnorm + ((size_t)b * F + f) * 3;
    o[0] = nx / d; o[1] = ny / d; o[2] = nz / d;
}

extern "C" int32_t ctx_prepare_vertices(const float *verts, const int64_t *faces, const float *cam,
                                        const float *proj3, int32_t B, int32_t V, int32_t F,
                                        float *fv_cam, float *fv_img, float *fnorm, void *ws,
                                        ctx_stream_t stream)
{
    CTX_REQUIRE(verts && faces && cam && proj3 && fv_cam && fv_img && fnorm && ws, "prepare_vertices: null pointer");
    CTX_REQUIRE(B > 0 && V > 0 && F > 0, "prepare_vertices: bad sizes B=%d V=%d F=%d", B, V, F);
    hipStream_t s = (hipStream_t)stream;
    float *vc = (float *)ws;
    float *vi = vc + (size_t)B * V * 3;
    hipLaunchKernelGGL(k_vertex_transform, dim3(cdiv(V, 256), B), dim3(256), 0, s, verts, cam, proj3, V, vc, vi);
    hipLaunchKernelGGL(k_face_gather, dim3(cdiv(F, 256), B), dim3(256), 0, s, vc, vi, faces, V, F, fv_cam, fv_img, fnorm);
    CTX_CHECK_LAUNCH("prepare_vertices");
    return CTX_OK;
}

// ------------------------------------------------------------------------------------------------
// Rasteriser.  Two kernels:
//   k_raster_bin : one workgroup per 64x64-pixel coarse tile scans all F faces (bbox vs tile) and
//                  appends surviving face ids to a per-tile list in the workspace.
//   k_raster     : one workgroup per 32x8 fine tile (one pixel per lane, 256 B of int64 indices per
//                  row) culls its coarse list to an LDS record list, then every pixel walks the
//                  LDS list.  Winner = max z, ties -> lowest face id (== "first face wins under a
//                  strict >" of the brute-force order), so list order is irrelevant.
#define COARSE 64
#define FT_W 32
#define FT_H 8

struct __attribute__((aligned(16))) FaceRec {   // 64 B, bbox first so it is one aligned 16-byte load
    float xmin, xmax, ymin, ymax;
    float ax, ay, bx, by, cx, cy;
    float z0, z1, z2;
    int id;
    int pad0, pad1;
};
static_assert(sizeof(FaceRec) == 64, "FaceRec must be 64 bytes");

__device__ __forceinline__ void load_face(const float *__restrict__ fxy, const float *__restrict__ fz,
                                          int zstride, float mult, FaceRec &r)
{
    r.ax = fxy[0] * mult; r.ay = fxy[1] * mult; r.bx = fxy[2] * mult;
    r.by = fxy[3] * mult; r.cx = fxy[4] * mult; r.cy = fxy[5] * mult;
    r.z0 = fz[0]; r.z1 = fz[zstride]; r.z2 = fz[2 * zstride];
    r.xmin = fminf(fminf(r.ax, r.bx), r.cx); r.xmax = fmaxf(fmaxf(r.ax, r.bx), r.cx);
    r.ymin = fminf(fminf(r.ay, r.by), r.cy); r.ymax = fmaxf(fmaxf(r.ay, r.by), r.cy);
}

__device__ __forceinline__ float pix_x(int i, int W, float mult) { return (mult / (float)W) * (float)(2 * i + 1 - W); }
__device__ __forceinline__ float pix_y(int j, int H, float mult) { return (mult / (float)H) * (float)(H - 2 * j - 1); }

// per-(view, face) record: scaled vertices, z, bbox — computed once, read as four 16-byte vectors afterwards
__global__ __launch_bounds__(256) void k_raster_setup(const float *__restrict__ fz, int zstride, const float *__restrict__ fxy,
                                                      int F, float mult, FaceRec *__restrict__ recs, float4 *__restrict__ bbox)
{
    int b = blockIdx.y;
    int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    FaceRec r;
    load_face(fxy + ((size_t)b * F + f) * 6, fz + ((size_t)b * F + f) * 3 * zstride, zstride, mult, r);
    r.id = f; r.pad0 = 0; r.pad1 = 0;
    recs[(size_t)b * F + f] = r;
    bbox[(size_t)b * F + f] = make_float4(r.xmin, r.xmax, r.ymin, r.ymax);   // compact copy: 16 B per face for the culls
}

// grid (coarse tiles, face-range groups, views): with few views a tile's face scan is cut into `gridDim.y` ranges so that the launch
// still has >= ~1000 workgroups; a group appends its survivors to the tile's list behind one global reservation per wave (the list
// order is then arbitrary: the fine kernel's winner rule does not depend on it).  `counts` is zeroed by the caller.
__global__ __launch_bounds__(256) void k_raster_bin(int H, int W, const float4 *__restrict__ bbox, int F, float mult,
                                                    int ntx, int nty, int *__restrict__ lists,
                                                    int *__restrict__ counts)
{
    int b = blockIdx.z;
    int tile = blockIdx.x;
    int tx = tile % ntx, ty = tile / ntx;
    int i0 = tx * COARSE, i1 = min(W, i0 + COARSE) - 1;
    int j0 = ty * COARSE, j1 = min(H, j0 + COARSE) - 1;
    float xlo = pix_x(i0, W, mult), xhi = pix_x(i1, W, mult);
    float yhi = pix_y(j0, H, mult), ylo = pix_y(j1, H, mult);
    int *list = lists + ((size_t)b * ntx * nty + tile) * F;
    int *cnt = counts + (size_t)b * ntx * nty + tile;
    const float4 *bbv = bbox + (size_t)b * F;
    const int per = ((F + (int)gridDim.y - 1) / (int)gridDim.y + 255) & ~255;
    const int fbeg = blockIdx.y * per, fend = min(F, fbeg + per);
    for (int f0 = fbeg; f0 < fend; f0 += 256) {
        int f = f0 + threadIdx.x;
        bool keep = false;
        if (f < fend) {
            const float4 bb = bbv[f];                             // xmin, xmax, ymin, ymax
            keep = !(xhi < bb.x || xlo >= bb.y || yhi < bb.z || ylo >= bb.w);
        }
        unsigned long long m = __ballot(keep);
        int lane = threadIdx.x & 63;
        int base = 0;
        if (lane == 0 && m) base = atomicAdd(cnt, __popcll(m));
        base = __shfl(base, 0, 64);
        if (keep) list[base + __popcll(m & ((1ull << lane) - 1))] = f;
    }
}

template <bool FUSED>
__global__ __launch_bounds__(256) void k_raster(int H, int W, const float *__restrict__ fz, int zstride,
                                                const FaceRec *__restrict__ recs, const float4 *__restrict__ bbox,
                                                const float *__restrict__ feat,
                                                int featB, int C, const float *__restrict__ fnorm, int F,
                                                float mult, float eps, int ntx, int nty,
                                                const int *__restrict__ lists, const int *__restrict__ counts,
                                                float *__restrict__ out, float *__restrict__ out_uv,
                                                int64_t *__restrict__ face_idx, float *__restrict__ normals)
{
    __shared__ __attribute__((aligned(16))) FaceRec s_rec[256];
    __shared__ int s_n;
    int b = blockIdx.z;
    int fi0 = blockIdx.x * FT_W, fj0 = blockIdx.y * FT_H;
    int lx = threadIdx.x % FT_W, ly = threadIdx.x / FT_W;
    int i = fi0 + lx, j = fj0 + ly;
    bool active = (i < W) && (j < H);
    int fi1 = min(W, fi0 + FT_W) - 1, fj1 = min(H, fj0 + FT_H) - 1;
    float txlo = pix_x(fi0, W, mult), txhi = pix_x(fi1, W, mult);
    float tyhi = pix_y(fj0, H, mult), tylo = pix_y(fj1, H, mult);
    float x0 = pix_x(i, W, mult), y0 = pix_y(j, H, mult);
    int ctile = (fj0 / COARSE) * ntx + (fi0 / COARSE);
    const int *list = lists + ((size_t)b * ntx * nty + ctile) * F;
    int n = counts[(size_t)b * ntx * nty + ctile];
    const FaceRec *rb = recs + (size_t)b * F;
    const float *zb = fz + (size_t)b * F * 3 * zstride;

    float best = -INFINITY, bw0 = 0.f, bw1 = 0.f, bw2 = 0.f;
    int bi = -1;
    for (int c0 = 0; c0 < n; c0 += 256) {
        __syncthreads();
        if (threadIdx.x == 0) s_n = 0;
        __syncthreads();
        int k = c0 + threadIdx.x;
        if (k < n) {
            int f = list[k];
            const float4 bb = bbox[(size_t)b * F + f];
            if (!(txhi < bb.x || txlo >= bb.y || tyhi < bb.z || tylo >= bb.w)) {
                int slot = atomicAdd(&s_n, 1);
                const float4 *src = (const float4 *)&rb[f];
                float4 *dst = (float4 *)&s_rec[slot];
                dst[0] = bb; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3];
            }
        }
        __syncthreads();
        int m = s_n;
        if (active) {
            for (int q = 0; q < m; ++q) {
                const FaceRec &r = s_rec[q];
                if (x0 < r.xmin || x0 >= r.xmax || y0 < r.ymin || y0 >= r.ymax) continue;
                float mm = r.bx - r.ax, p = r.by - r.ay, nn = r.cx - r.ax, qq = r.cy - r.ay;
                float s = x0 - r.ax, t = y0 - r.ay;
                float k1 = s * qq - nn * t;
                float k2 = mm * t - s * p;
                float k3 = mm * qq - nn * p;
                float den = k3 + eps;
                float w1 = k1 / den;
                float w2 = k2 / den;
                float w0 = (1.0f - w1) - w2;
                if (w0 < 0.0f || w1 < 0.0f || w2 < 0.0f) continue;
                float z = (w0 * r.z0 + w1 * r.z1) + w2 * r.z2;
                if (z > best || (z == best && r.id < bi)) {
                    best = z; bi = r.id; bw0 = w0; bw1 = w1; bw2 = w2;
                }
            }
        }
    }
    if (!active) return;
    size_t pix = ((size_t)b * H + j) * W + i;
    face_idx[pix] = (int64_t)bi;
    if (FUSED) {
        float d = 0.f, u = 0.f, v = 0.f;
        if (bi >= 0) {
            const float *zf = zb + (size_t)bi * 3 * zstride;
            d = (bw0 * zf[0] + bw1 * zf[zstride]) + bw2 * zf[2 * zstride];
            const float *ff = feat + ((size_t)(featB == 1 ? 0 : b) * F + bi) * 6;
            u = (bw0 * ff[0] + bw1 * ff[2]) + bw2 * ff[4];
            v = (bw0 * ff[1] + bw1 * ff[3]) + bw2 * ff[5];
        }
        out[pix] = d;
        out_uv[pix * 2 + 0] = u;
        out_uv[pix * 2 + 1] = v;
        if (normals) {
            int fnb = bi >= 0 ? bi : F - 1;   // python negative index: -1 -> last face
            const float *nf = fnorm + ((size_t)b * F + fnb) * 3;
            normals[pix * 3 + 0] = nf[0]; normals[pix * 3 + 1] = nf[1]; normals[pix * 3 + 2] = nf[2];
        }
    } else {
        for (int c = 0; c < C; ++c) {
            float val = 0.f;
            if (bi >= 0) {
                const float *ff = feat + ((size_t)(featB == 1 ? 0 : b) * F + bi) * 3 * C;
                val = (bw0 * ff[0 * C + c] + bw1 * ff[1 * C + c]) + bw2 * ff[2 * C + c];
            }
            out[pix * C + c] = val;
        }
    }
}

extern "C" int64_t ctx_rasterize_ws_bytes(int32_t H, int32_t W, int32_t B, int32_t F)
{
    int64_t nt = (int64_t)cdiv(W, COARSE) * cdiv(H, COARSE);
    return ((int64_t)B * nt * F + (int64_t)B * nt) * 4 + (int64_t)B * F * (64 + 16) + 512;
}

static int32_t raster_common(bool fused, int H, int W, const float *fz, int zstride, const float *fxy,
                             const float *feat, int featB, int C, const float *fnorm, int B, int F, float mult,
                             float eps, float *out, float *out_uv, int64_t *face_idx, float *normals, void *ws,
                             int64_t ws_bytes, hipStream_t s)
{
    CTX_REQUIRE(fz && fxy && feat && out && face_idx && ws, "rasterize: null pointer");
    CTX_REQUIRE(H > 0 && W > 0 && B > 0 && F > 0 && H <= 16384 && W <= 16384, "rasterize: bad sizes H=%d W=%d B=%d F=%d", H, W, B, F);
    CTX_REQUIRE(ws_bytes >= ctx_rasterize_ws_bytes(H, W, B, F), "rasterize: workspace too small (%lld < %lld)",
                (long long)ws_bytes, (long long)ctx_rasterize_ws_bytes(H, W, B, F));
    int ntx = cdiv(W, COARSE), nty = cdiv(H, COARSE);
    FaceRec *recs = (FaceRec *)(((uintptr_t)ws + 63) & ~(uintptr_t)63);
    float4 *bbox = (float4 *)(recs + (size_t)B * F);
    int *lists = (int *)(bbox + (size_t)B * F);
    int *counts = lists + (size_t)B * ntx * nty * F;
    hipLaunchKernelGGL(k_raster_setup, dim3(cdiv(F, 256), B), dim3(256), 0, s, fz, zstride, fxy, F, mult, recs, bbox);
    (void)hipMemsetAsync(counts, 0, (size_t)B * ntx * nty * sizeof(int), s);
    int G = cdiv(1024, ntx * nty * B);                          // face-range groups per tile: keep the bin launch >= ~1000 workgroups
    G = max(1, min(min(G, 8), cdiv(F, 256)));
    hipLaunchKernelGGL(k_raster_bin, dim3(ntx * nty, G, B), dim3(256), 0, s, H, W, bbox, F, mult, ntx, nty, lists, counts);
    dim3 grid(cdiv(W, FT_W), cdiv(H, FT_H), B);
    CTX_BOOL_GO(fused, FU, hipLaunchKernelGGL(k_raster<FU>, grid, dim3(256), 0, s, H, W, fz, zstride, recs, bbox, feat, featB, C, fnorm, F, mult,
                                              eps, ntx, nty, lists, counts, out, out_uv, face_idx, normals));
    CTX_CHECK_LAUNCH("rasterize");
    return CTX_OK;
}

extern "C" int32_t ctx_rasterize_fwd(int32_t H, int32_t W, const float *face_z, const float *face_xy,
                                     const float *feat, int32_t B, int32_t F, int32_t C, float multiplier,
                                     float eps, float *out, int64_t *face_idx, void *ws, int64_t ws_bytes,
                                     ctx_stream_t stream)
{
    CTX_REQUIRE(C >= 1 && C <= 64, "rasterize: C=%d unsupported", C);
    return raster_common(false, H, W, face_z, 1, face_xy, feat, B, C, nullptr, B, F, multiplier, eps, out, nullptr,
                         face_idx, nullptr, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int32_t ctx_rasterize_fused(int32_t H, int32_t W, const float *fv_cam, const float *face_xy,
                                       const float *uv_attr, int32_t Bu, const float *fnorm, int32_t B, int32_t F,
                                       float multiplier, float eps, float *depth, float *uv, int64_t *face_idx,
                                       float *normals, void *ws, int64_t ws_bytes, ctx_stream_t stream)
{
    CTX_REQUIRE(uv && (Bu == 1 || Bu == B), "rasterize_fused: uv null or Bu=%d not in {1,%d}", Bu, B);
    CTX_REQUIRE((normals == nullptr) || (fnorm != nullptr), "rasterize_fused: normals requested without fnorm");
    // z of vertex k of face f is fv_cam[b,f,k,2]: base +2, stride 3
    return raster_common(true, H, W, fv_cam + 2, 3, face_xy, uv_attr, Bu, 2, fnorm, B, F, multiplier, eps, depth, uv,
                         face_idx, normals, ws, ws_bytes, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------
// normalize_multiple_depth: partial min/max per (view, block) -> normalise.
#define ND_BLOCKS 256
__global__ __launch_bounds__(256) void k_depth_minmax(const float *__restrict__ d, int HW, float *__restrict__ part,
                                                      int *__restrict__ flags)
{
    int b = blockIdx.y;
    const float *p = d + (size_t)b * HW;
    float mn = INFINITY, mx = -INFINITY;
    int pos = 0, any = 0;
    const int n4 = HW >> 2;
    const float4 *p4 = (const float4 *)p;            // views start 16-B aligned when HW % 4 == 0 (else scalar path)
    if ((HW & 3) == 0) {
        for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += ND_BLOCKS * 256) {
            float4 v = p4[i];
            float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (e[j] > 0.f) pos = 1;
                if (e[j] != 0.f) { any = 1; mn = fminf(mn, e[j]); mx = fmaxf(mx, e[j]); }
            }
        }
    } else {
        for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += ND_BLOCKS * 256) {
            float v = p[i];
            if (v > 0.f) pos = 1;
            if (v != 0.f) { any = 1; mn = fminf(mn, v); mx = fmaxf(mx, v); }
        }
    }
    mn = wave_min(mn); mx = wave_max(mx);
    __shared__ float s_mn[4], s_mx[4];
    int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_mn[w] = mn; s_mx[w] = mx; }
    int bpos = __syncthreads_or(pos), bany = __syncthreads_or(any);
    if (threadIdx.x == 0) {
        mn = fminf(fminf(s_mn[0], s_mn[1]), fminf(s_mn[2], s_mn[3]));
        mx = fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
        part[((size_t)b * ND_BLOCKS + blockIdx.x) * 2 + 0] = mn;
        part[((size_t)b * ND_BLOCKS + blockIdx.x) * 2 + 1] = mx;
        // one flag word per block (no same-address atomics): bit0 = positive value seen, bit1 = non-zero seen
        flags[4 + b * ND_BLOCKS + blockIdx.x] = (bpos ? 1 : 0) | (bany ? 2 : 0);
    }
}

__global__ __launch_bounds__(256) void k_depth_apply(const float *__restrict__ d, int HW, const float *__restrict__ part,
                                                     const int *__restrict__ flags, float *__restrict__ out,
                                                     int *__restrict__ status)
{
    int b = blockIdx.y;
    float mn = part[((size_t)b * ND_BLOCKS + threadIdx.x) * 2 + 0];
    float mx = part[((size_t)b * ND_BLOCKS + threadIdx.x) * 2 + 1];
    mn = wave_min(mn); mx = wave_max(mx);
    __shared__ float s_mn[4], s_mx[4];
    int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_mn[w] = mn; s_mx[w] = mx; }
    __syncthreads();
    mn = fminf(fminf(s_mn[0], s_mn[1]), fminf(s_mn[2], s_mn[3]));
    mx = fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
    float range = mx - mn;
    if (status && b == 0 && blockIdx.x == 0) {
        int acc = 0;
        for (int i = threadIdx.x; i < (int)gridDim.y * ND_BLOCKS; i += 256) acc |= flags[4 + i];
        int any_pos = __syncthreads_or(acc & 1), any_nz = __syncthreads_or(acc & 2);   // returns "any non-zero", not the OR
        if (threadIdx.x == 0) status[0] = any_pos ? 1 : (any_nz ? 0 : 2);
    }
    const float *p = d + (size_t)b * HW;
    float *o = out + (size_t)b * HW;
    if ((HW & 3) == 0) {
        const int n4 = HW >> 2;
        for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
            float4 v = ((const float4 *)p)[i];
            float4 r;
            r.x = (v.x != 0.f) ? (v.x - mn) / range : v.x;
            r.y = (v.y != 0.f) ? (v.y - mn) / range : v.y;
            r.z = (v.z != 0.f) ? (v.z - mn) / range : v.z;
            r.w = (v.w != 0.f) ? (v.w - mn) / range : v.w;
            ((float4 *)o)[i] = r;
        }
    } else {
        for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
            float v = p[i];
            o[i] = (v != 0.f) ? (v - mn) / range : v;
        }
    }
}

extern "C" int64_t ctx_normalize_depth_ws_bytes(int32_t B) { return (int64_t)B * ND_BLOCKS * 3 * 4 + 64; }

extern "C" int32_t ctx_normalize_depth(const float *depth, int32_t B, int32_t HW, float *out, void *ws,
                                       int32_t *status, ctx_stream_t stream)
{
    CTX_REQUIRE(depth && out && ws && B > 0 && HW > 0, "normalize_depth: bad args");
    hipStream_t s = (hipStream_t)stream;
    int *flags = (int *)ws;                                   // [4 + B*ND_BLOCKS] ints, every word written by pass 1
    float *part = (float *)ws + 4 + (size_t)B * ND_BLOCKS;
    hipLaunchKernelGGL(k_depth_minmax, dim3(ND_BLOCKS, B), dim3(256), 0, s, depth, HW, part, flags);
    int nb = min(cdiv(HW, 1024), 1024);
    hipLaunchKernelGGL(k_depth_apply, dim3(nb, B), dim3(256), 0, s, depth, HW, part, flags, out, status);
    CTX_CHECK_LAUNCH("normalize_depth");
    return CTX_OK;
}
