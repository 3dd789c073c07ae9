// Camera rays and the unfused positional encoding for gfx950: the two small kernels of the NeRF-side API (get_rays, get_embedder)
// that no fused kernel covers.  Compiled with -ffp-contract=off: every float op is one IEEE binary32 op in source order, the
// order of oracle/nerf.py's embed and get_rays (run_nerf_helpers.py:15-65, 139-148).
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)

// Positional encoding (unfused form, kept for API parity with get_embedder; the MLP kernel fuses it).
__global__ __launch_bounds__(256) void k_embed(const float *__restrict__ x, int64_t N, int d, int L, float *__restrict__ out)
{
    int od = d * (1 + 2 * L);
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < N; n += (int64_t)gridDim.x * 256) {
        float *o = out + n * od;
        for (int c = 0; c < d; ++c) {
            float v = x[n * d + c];
            o[c] = v;
            float fr = 1.0f;
            for (int l = 0; l < L; ++l) {
                float a = v * fr;
                o[d + (2 * l) * d + c] = sinf(a);
                o[d + (2 * l + 1) * d + c] = cosf(a);
                fr = fr * 2.0f;
            }
        }
    }
}

extern "C" int32_t ctx_embed_fwd(const float *x, int64_t N, int32_t d, int32_t L, float *out, ctx_stream_t stream)
{
    CTX_REQUIRE(x && out && N > 0 && d > 0 && L >= 0, "embed: bad args");
    int nb = (int)((N + 255) / 256 < 4096 ? (N + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_embed, dim3(nb), dim3(256), 0, (hipStream_t)stream, x, N, d, L, out);
    CTX_CHECK_LAUNCH("embed");
    return CTX_OK;
}

// Camera rays.
__global__ __launch_bounds__(256) void k_get_rays(int H, int W, float fx, float fy, float cx, float cy,
                                                  const float *__restrict__ c2w, float *__restrict__ ro,
                                                  float *__restrict__ rd)
{
    int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= (int64_t)H * W) return;
    int j = (int)(n / W), i = (int)(n % W);
    float dx = ((float)i - cx) / fx, dy = -((float)j - cy) / fy, dz = -1.0f;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        // torch.sum(dirs[..., None, :] * c2w[:3,:3], -1): sequential left-to-right sum
        rd[n * 3 + r] = (dx * c2w[r * 4 + 0] + dy * c2w[r * 4 + 1]) + dz * c2w[r * 4 + 2];
        ro[n * 3 + r] = c2w[r * 4 + 3];
    }
}

extern "C" int32_t ctx_get_rays(int32_t H, int32_t W, float fx, float fy, float cx, float cy, const float *c2w,
                                float *rays_o, float *rays_d, ctx_stream_t stream)
{
    CTX_REQUIRE(c2w && rays_o && rays_d && H > 0 && W > 0, "get_rays: bad args");
    hipLaunchKernelGGL(k_get_rays, dim3((unsigned)cdiv64((int64_t)H * W, 256)), dim3(256), 0, (hipStream_t)stream,
                       H, W, fx, fy, cx, cy, c2w, rays_o, rays_d);
    CTX_CHECK_LAUNCH("get_rays");
    return CTX_OK;
}
