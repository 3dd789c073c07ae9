// texture_mapping == grid_sample(bilinear|nearest, align_corners=False, padding 'border') for gfx950 (src/models/render.py:135):
// forward (planar and texel-interleaved), backward by float atomics, and the mark of the texels a raster reads.  Compiled with
// -ffp-contract=off and held to oracle/geometry_ref.c bit for bit; the tap is texel_taps.h's, which the binned scatter (uvscatter.hip)
// shares, so the lookup, its gradient and the active-texel list name the same texels.
#include "common.h"
#include "texel_taps.h"

#pragma clang fp contract(off)

__global__ __launch_bounds__(256) void k_texmap_fwd(const float *__restrict__ uv, const float *__restrict__ tex,
                                                    int64_t HW, int C, int T, int Bt, int mode,
                                                    const int64_t *__restrict__ mask_idx, float *__restrict__ out)
{
    int b = blockIdx.y;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += (int64_t)gridDim.x * 256) {
        size_t pix = (size_t)b * HW + i;
        float2 q = *(const float2 *)(uv + pix * 2);
        const float *tb = tex + (Bt == 1 ? 0 : (size_t)b * C * T * T);
        const TexelTaps t = texel_taps(q.x, q.y, T);
        float msk = 1.0f;
        if (mask_idx) msk = mask_idx[pix] > -1 ? 1.0f : 0.0f;
        float *o = out + pix * C;
        if (mode == 1) {
            int xn = (int)nearbyintf(t.ix), yn = (int)nearbyintf(t.iy);
            bool in = xn >= 0 && xn < T && yn >= 0 && yn < T;
            for (int c = 0; c < C; ++c) {
                float v = in ? tb[((size_t)c * T + yn) * T + xn] : 0.0f;
                o[c] = mask_idx ? v * msk : v;
            }
            continue;
        }
        for (int c = 0; c < C; ++c) {
            const float *tc = tb + (size_t)c * T * T;
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (t.in[k]) acc = acc + tc[(size_t)t.y(k) * T + t.x(k)] * t.w[k];
            o[c] = mask_idx ? acc * msk : acc;
        }
    }
}

__global__ __launch_bounds__(256) void k_texmap_bwd(const float *__restrict__ go, const float *__restrict__ uv,
                                                    int64_t HW, int C, int T, const int64_t *__restrict__ mask_idx,
                                                    float *__restrict__ gt)
{
    int b = blockIdx.y;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += (int64_t)gridDim.x * 256) {
        size_t pix = (size_t)b * HW + i;
        if (mask_idx && mask_idx[pix] < 0) continue;
        float2 q = *(const float2 *)(uv + pix * 2);
        const TexelTaps t = texel_taps(q.x, q.y, T);
        for (int c = 0; c < C; ++c) {
            float g = go[pix * C + c];
            float *tc = gt + (size_t)c * T * T;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (t.in[k]) atomicAdd(tc + (size_t)t.y(k) * T + t.x(k), g * t.w[k]);
        }
    }
}

// Texel-interleaved variant for C <= 4 and one shared texture: [C,T,T] is repacked once into [T,T,4] (16 bytes per
// texel) so a bilinear tap is ONE 16-byte gather instead of C 4-byte gathers; the per-channel arithmetic and its order are
// those of k_texmap_fwd (results are bit-identical).
__global__ __launch_bounds__(256) void k_tex_pack4(const float *__restrict__ tex, int C, int T, float4 *__restrict__ packed)
{
    const int64_t n = (int64_t)T * T;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        v.x = tex[i];
        if (C > 1) v.y = tex[n + i];
        if (C > 2) v.z = tex[2 * n + i];
        if (C > 3) v.w = tex[3 * n + i];
        packed[i] = v;
    }
}

__global__ __launch_bounds__(256) void k_texmap_fwd4(const float *__restrict__ uv, const float4 *__restrict__ tex, int64_t HW, int C,
                                                     int T, int mode, const int64_t *__restrict__ mask_idx, float *__restrict__ out)
{
    const int b = blockIdx.y;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += (int64_t)gridDim.x * 256) {
        const size_t pix = (size_t)b * HW + i;
        float2 q = *(const float2 *)(uv + pix * 2);
        const TexelTaps t = texel_taps(q.x, q.y, T);
        float msk = 1.0f;
        if (mask_idx) msk = mask_idx[pix] > -1 ? 1.0f : 0.0f;
        float r[4];
        if (mode == 1) {
            int xn = (int)nearbyintf(t.ix), yn = (int)nearbyintf(t.iy);
            bool in = xn >= 0 && xn < T && yn >= 0 && yn < T;
            float4 tn = in ? tex[(size_t)yn * T + xn] : make_float4(0.f, 0.f, 0.f, 0.f);
            r[0] = tn.x; r[1] = tn.y; r[2] = tn.z; r[3] = tn.w;
        } else {
            // unconditional gathers (x1, y1 clamped into the atlas), then the same guarded accumulation order as the planar kernel
            float a[4][4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 g = tex[(size_t)min(t.y(k), T - 1) * T + min(t.x(k), T - 1)];
                a[k][0] = g.x; a[k][1] = g.y; a[k][2] = g.z; a[k][3] = g.w;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float acc = 0.0f;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (t.in[k]) acc = acc + a[k][c] * t.w[k];
                r[c] = acc;
            }
        }
        float *o = out + pix * C;
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < C) o[c] = mask_idx ? r[c] * msk : r[c];
    }
}

extern "C" int32_t ctx_texture_pack4(const float *tex, int32_t C, int32_t T, float *packed, ctx_stream_t stream)
{
    CTX_REQUIRE(tex && packed && C >= 1 && C <= 4 && T > 0, "texture_pack4: bad args C=%d T=%d", C, T);
    int nb = min(cdiv(T * T, 256), 4096);
    hipLaunchKernelGGL(k_tex_pack4, dim3(nb), dim3(256), 0, (hipStream_t)stream, tex, C, T, (float4 *)packed);
    CTX_CHECK_LAUNCH("texture_pack4");
    return CTX_OK;
}

extern "C" int32_t ctx_texture_mapping_packed_fwd(const float *uv, const float *packed, int32_t B, int32_t HW, int32_t C, int32_t T,
                                                  int32_t mode, const int64_t *mask_idx, float *out, ctx_stream_t stream)
{
    CTX_REQUIRE(uv && packed && out, "texture_mapping_packed: null pointer");
    CTX_REQUIRE(B > 0 && HW > 0 && C >= 1 && C <= 4 && T > 0 && (mode == 0 || mode == 1), "texture_mapping_packed: bad args");
    int nb = min(cdiv(HW, 256), 4096);
    hipLaunchKernelGGL(k_texmap_fwd4, dim3(nb, B), dim3(256), 0, (hipStream_t)stream, uv, (const float4 *)packed, (int64_t)HW, C, T, mode,
                       mask_idx, out);
    CTX_CHECK_LAUNCH("texture_mapping_packed_fwd");
    return CTX_OK;
}

extern "C" int32_t ctx_texture_mapping_fwd(const float *uv, const float *tex, int32_t B, int32_t HW, int32_t C,
                                           int32_t T, int32_t Bt, int32_t mode, const int64_t *mask_idx, float *out,
                                           ctx_stream_t stream)
{
    CTX_REQUIRE(uv && tex && out, "texture_mapping: null pointer");
    CTX_REQUIRE(B > 0 && HW > 0 && C > 0 && T > 0 && (Bt == 1 || Bt == B) && (mode == 0 || mode == 1),
                "texture_mapping: bad args B=%d HW=%d C=%d T=%d Bt=%d mode=%d", B, HW, C, T, Bt, mode);
    int nb = min(cdiv(HW, 256), 4096);
    hipLaunchKernelGGL(k_texmap_fwd, dim3(nb, B), dim3(256), 0, (hipStream_t)stream, uv, tex, (int64_t)HW, C, T, Bt, mode, mask_idx, out);
    CTX_CHECK_LAUNCH("texture_mapping_fwd");
    return CTX_OK;
}

extern "C" int32_t ctx_texture_mapping_bwd(const float *grad_out, const float *uv, int32_t B, int32_t HW, int32_t C,
                                           int32_t T, const int64_t *mask_idx, float *grad_tex, ctx_stream_t stream)
{
    CTX_REQUIRE(grad_out && uv && grad_tex && B > 0 && HW > 0 && C > 0 && T > 0, "texture_mapping_bwd: bad args");
    int nb = min(cdiv(HW, 256), 4096);
    hipLaunchKernelGGL(k_texmap_bwd, dim3(nb, B), dim3(256), 0, (hipStream_t)stream, grad_out, uv, (int64_t)HW, C, T, mask_idx, grad_tex);
    CTX_CHECK_LAUNCH("texture_mapping_bwd");
    return CTX_OK;
}

// The texels a raster can read (the set get_texture_map_only_valid_areas, src/models/textured_mesh.py:303-347, restricts the field to,
// taken from the pixels instead of the charts): the four bilinear taps of every foreground pixel, with k_texmap_fwd's index
// arithmetic, whatever their weights.  Plain byte stores of 1 (as k_vc_seen): idempotent, so several rasters accumulate a union.
// A background pixel's uv may hold anything and is not read.
__global__ __launch_bounds__(256) void k_texel_mark(const float *__restrict__ uv, const int64_t *__restrict__ face_idx, int64_t HW, int T,
                                                    uint8_t *__restrict__ mask)
{
    int b = blockIdx.y;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += (int64_t)gridDim.x * 256) {
        size_t pix = (size_t)b * HW + i;
        if (face_idx[pix] < 0) continue;
        float2 q = *(const float2 *)(uv + pix * 2);
        const TexelTaps t = texel_taps(q.x, q.y, T);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (t.in[k]) mask[(size_t)t.y(k) * T + t.x(k)] = 1;
    }
}

extern "C" int32_t ctx_texel_active_mark(const float *uv, const int64_t *face_idx, int32_t B, int32_t H, int32_t W, int32_t T, uint8_t *mask,
                                         ctx_stream_t stream)
{
    CTX_REQUIRE(uv && face_idx && mask, "texel_active_mark: null pointer");
    CTX_REQUIRE(B > 0 && H > 0 && W > 0 && T >= 2, "texel_active_mark: bad sizes B=%d H=%d W=%d T=%d", B, H, W, T);
    const int64_t HW = (int64_t)H * W;
    hipLaunchKernelGGL(k_texel_mark, dim3(capped_blocks(HW, 256, 4096), B), dim3(256), 0, (hipStream_t)stream, uv, face_idx, HW, T, mask);
    CTX_CHECK_LAUNCH("texel_active_mark");
    return CTX_OK;
}
