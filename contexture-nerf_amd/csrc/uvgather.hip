// UV back-projection by texel-side GATHER: the other direction of uvscatter.hip's fixed mode.  Every atlas texel looks its own
// surface point up in every painted view, so there are no pinholes where the surface is magnified (neighbouring screen pixels
// landing more than a texel apart), nothing is written outside a chart, and there are neither atomics nor plan buffers.
//
// The texel map (texel_face, texel_bary: the UV triangles drawn at T x T with the identity as face features) names the face f
// and the barycentrics (b0, b1, b2) of every chart texel.  For view v, in binary32, in the order written, no contraction:
//   own pixel   f owns at least one pixel of face_idx[v] (k_ug_seen: plain byte stores of 1 into seen [B,F], as k_vc_seen);
//               back faces and sub-pixel faces drop out here.
//   projection  X = (b0*x0 + b1*x1) + b2*x2, Y likewise, from face_vertices_image[v,f]; px = ((X + 1)*W - 1)/2,
//               py = ((1 - Y)*H - 1)/2 (row 0 at Y = +1, the raster's rows); xn = floor(px + 0.5), yn = floor(py + 0.5);
//               (xn, yn) outside the image: nothing.
//   visibility  g = face_idx[v,yn,xn] must be RELATED to f: equal, or sharing a vertex id in `faces`.  An integer rule: no depth
//               tolerance.
//   colour      the four bilinear taps at (floor(px), floor(py)) + {0,1}^2 with k_texmap_fwd's weights and order (nw, ne, sw,
//               se); a tap counts when it is inside the image and its owner is related to f (an occluder in front of a
//               silhouette does not bleed in); colour_c = (sum w_k * values[v,tap_k,c]) / (sum w_k), IEEE division.  The
//               nearest pixel is a counted tap, so the divisor is >= 0.25.
//   weight      omega = weight[v,yn,xn] (nearest; 1 without a weight).  omega == 0, or a non-finite omega or colour: nothing.
//   sum         acc[c,p] += __float2ll_rn(ldexpf(colour_c * omega, frac)); acc[C,p] += __float2ll_rn(ldexpf(omega, frac)):
//               k_sb_direct's conversion, so dist.merge_atlas and ctx_fixed_to_float apply unchanged.
// One thread owns a texel, walks the B views with the C + 1 sums in registers and does one plain read-modify-write of acc:
// the result does not depend on grid, order or stream, and a texel outside every chart is never written.  A workgroup is a
// 16 x 16 texel tile (neighbouring texels read neighbouring pixels); a tile without a chart texel leaves at once.
#include "common.h"

#define UG_MAXC 4
#define UG_TS 16

__global__ __launch_bounds__(256) void k_ug_seen(const int64_t *__restrict__ face_idx, int64_t HW, int F, unsigned char *__restrict__ seen)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int v = blockIdx.y;
    if (p >= HW) return;
    const int64_t f = face_idx[(int64_t)v * HW + p];
    if (f >= 0 && f < F) seen[(int64_t)v * F + f] = 1;
}

// g is a face of the mesh and shares a vertex id with (or is) face f, whose vertex ids are a0..a2
__device__ __forceinline__ bool ug_related(const int64_t *__restrict__ faces, int F, int64_t f, int64_t a0, int64_t a1, int64_t a2, int64_t g)
{
    if (g < 0 || g >= F) return false;
    if (g == f) return true;
    const int64_t b0 = faces[g * 3 + 0], b1 = faces[g * 3 + 1], b2 = faces[g * 3 + 2];
    return b0 == a0 || b0 == a1 || b0 == a2 || b1 == a0 || b1 == a1 || b1 == a2 || b2 == a0 || b2 == a1 || b2 == a2;
}

template <int C>
__global__ __launch_bounds__(256) void k_uv_gather(const float *__restrict__ values, const float *__restrict__ weight, const int64_t *__restrict__ face_idx,
                                                   const float *__restrict__ fvi, const int64_t *__restrict__ faces,
                                                   const int64_t *__restrict__ texel_face, const float *__restrict__ texel_bary,
                                                   const unsigned char *__restrict__ seen, int B, int H, int W, int F, int T, int frac,
                                                   long long *__restrict__ acc)
{
    const int x = blockIdx.x * UG_TS + (threadIdx.x & (UG_TS - 1)), y = blockIdx.y * UG_TS + (threadIdx.x >> 4);
    const bool in = x < T && y < T;
    const size_t p = (size_t)y * T + x;
    int64_t f = in ? texel_face[p] : -1;
    if (f >= F) f = -1;
    if (!__syncthreads_or(f >= 0)) return;                      // about half the atlas belongs to no chart
    if (f < 0) return;
    const float b0 = texel_bary[p * 3 + 0], b1 = texel_bary[p * 3 + 1], b2 = texel_bary[p * 3 + 2];
    const int64_t a0 = faces[f * 3 + 0], a1 = faces[f * 3 + 1], a2 = faces[f * 3 + 2];
    const int64_t HW = (int64_t)H * W;
    const float fW = (float)W, fH = (float)H;
    long long sum[C + 1];
#pragma unroll
    for (int c = 0; c <= C; ++c) sum[c] = 0;
    bool touched = false;
    for (int v = 0; v < B; ++v) {
        if (!seen[(int64_t)v * F + f]) continue;
        const float2 *q = (const float2 *)(fvi + ((int64_t)v * F + f) * 6);
        const float2 q0 = q[0], q1 = q[1], q2 = q[2];
        const float X = (b0 * q0.x + b1 * q1.x) + b2 * q2.x, Y = (b0 * q0.y + b1 * q1.y) + b2 * q2.y;
        const float px = ((X + 1.0f) * fW - 1.0f) / 2.0f, py = ((1.0f - Y) * fH - 1.0f) / 2.0f;
        const float fxn = floorf(px + 0.5f), fyn = floorf(py + 0.5f);
        if (!(fxn >= 0.0f && fxn < fW && fyn >= 0.0f && fyn < fH)) continue;           // also refuses NaN
        const int xn = (int)fxn, yn = (int)fyn;
        const int64_t *idx = face_idx + (int64_t)v * HW;
        const int64_t pn = (int64_t)yn * W + xn;
        // every load of the view that does not hang on another: the nearest owner, its weight, the four tap owners
        const int x0 = (int)floorf(px), y0 = (int)floorf(py), x1 = x0 + 1, y1 = y0 + 1;   // px in [-0.5, W - 0.5) here
        const bool bx0 = x0 >= 0 && x0 < W, bx1 = x1 >= 0 && x1 < W, by0 = y0 >= 0 && y0 < H, by1 = y1 >= 0 && y1 < H;
        const bool tin[4] = {bx0 && by0, bx1 && by0, bx0 && by1, bx1 && by1};
        const int64_t tp[4] = {(int64_t)y0 * W + x0, (int64_t)y0 * W + x1, (int64_t)y1 * W + x0, (int64_t)y1 * W + x1};
        const int64_t g = idx[pn];
        const float om = weight ? weight[(int64_t)v * HW + pn] : 1.0f;
        int64_t tg[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) tg[k] = tin[k] ? idx[tp[k]] : -1;
        if (!ug_related(faces, F, f, a0, a1, a2, g)) continue;
        const float tw[4] = {((float)x1 - px) * ((float)y1 - py), (px - (float)x0) * ((float)y1 - py),
                             ((float)x1 - px) * (py - (float)y0), (px - (float)x0) * (py - (float)y0)};
        float s = 0.0f, num[C];
#pragma unroll
        for (int c = 0; c < C; ++c) num[c] = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!tin[k] || !ug_related(faces, F, f, a0, a1, a2, tg[k])) continue;
            const float *val = values + ((int64_t)v * HW + tp[k]) * C;
            s = s + tw[k];
#pragma unroll
            for (int c = 0; c < C; ++c) num[c] = num[c] + val[c] * tw[k];
        }
        bool ok = om != 0.0f && isfinite(om);
        float col[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            col[c] = num[c] / s;
            ok = ok && isfinite(col[c]);
        }
        if (!ok) continue;
#pragma unroll
        for (int c = 0; c < C; ++c) sum[c] += __float2ll_rn(ldexpf(col[c] * om, frac));
        sum[C] += __float2ll_rn(ldexpf(om, frac));
        touched = true;
    }
    if (!touched) return;
    const size_t TT = (size_t)T * T;
#pragma unroll
    for (int c = 0; c <= C; ++c) acc[c * TT + p] += sum[c];
}

extern "C" int64_t ctx_uv_gather_ws_bytes(int32_t B, int32_t F) { return (B < 1 || F < 1) ? -1 : (int64_t)B * F; }

extern "C" int32_t ctx_uv_gather_fixed(const float *values, const float *weight, const int64_t *face_idx, const float *face_vertices_image,
                                       const int64_t *faces, const int64_t *texel_face, const float *texel_bary, int32_t B, int32_t H, int32_t W,
                                       int32_t C, int32_t F, int32_t T, int32_t frac_bits, int64_t *acc, void *ws, int64_t ws_bytes, ctx_stream_t stream)
{
    CTX_REQUIRE(values && face_idx && face_vertices_image && faces && texel_face && texel_bary && acc && ws, "uv_gather_fixed: bad args");
    CTX_REQUIRE(B >= 1 && H >= 1 && W >= 1 && F >= 1 && T >= 1, "uv_gather_fixed: B=%d H=%d W=%d F=%d T=%d must be positive", B, H, W, F, T);
    CTX_REQUIRE(C >= 1 && C <= UG_MAXC, "uv_gather_fixed: C=%d outside [1, %d]", C, UG_MAXC);
    CTX_REQUIRE(frac_bits >= -64 && frac_bits <= 62, "uv_gather_fixed: frac_bits=%d outside [-64, 62]", frac_bits);
    CTX_REQUIRE(H <= (1 << 24) && W <= (1 << 24), "uv_gather_fixed: a %d x %d image is beyond exact float pixel indices", H, W);
    const int64_t HW = (int64_t)H * W;
    CTX_REQUIRE(cdiv64(HW, 256) <= 0x7fffffff && B <= 65535 && cdiv(T, UG_TS) <= 65535, "uv_gather_fixed: B=%d, %d x %d pixels or T=%d do not fit one grid", B, H, W, T);
    CTX_REQUIRE(ws_bytes >= ctx_uv_gather_ws_bytes(B, F), "uv_gather_fixed: workspace of %lld bytes, ctx_uv_gather_ws_bytes(%d, %d) = %lld",
                (long long)ws_bytes, B, F, (long long)ctx_uv_gather_ws_bytes(B, F));
    hipStream_t s = (hipStream_t)stream;
    unsigned char *seen = (unsigned char *)ws;
    if (hipMemsetAsync(seen, 0, (size_t)B * F, s) != hipSuccess) { ctx_set_error("uv_gather_fixed: memset failed"); return CTX_E_LAUNCH; }
    hipLaunchKernelGGL(k_ug_seen, dim3((unsigned)cdiv64(HW, 256), B), dim3(256), 0, s, face_idx, HW, F, seen);
    const dim3 grid(cdiv(T, UG_TS), cdiv(T, UG_TS));
#define UG_GO(C_) hipLaunchKernelGGL(k_uv_gather<C_>, grid, dim3(256), 0, s, values, weight, face_idx, face_vertices_image, faces, texel_face, texel_bary, \
                                     seen, B, H, W, F, T, frac_bits, (long long *)acc)
    switch (C) {
    case 1: UG_GO(1); break;
    case 2: UG_GO(2); break;
    case 3: UG_GO(3); break;
    default: UG_GO(4); break;
    }
#undef UG_GO
    CTX_CHECK_LAUNCH("uv_gather_fixed");
    return CTX_OK;
}
