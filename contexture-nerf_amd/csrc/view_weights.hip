// View weights for gfx950 (src/training/trainer.py:155-249): per face the largest normal z over the views that see it, then per
// pixel "is this view the best one".  Floats are only compared and copied; the masks equal oracle/geometry_ref.c's exactly.
#include "common.h"

// max over pixels of fnz[b, face_idx[b,p]] per face == max over the views in which
// the face is visible, so phase 0 only marks (view, face) visibility (idempotent byte stores, no
// atomics) and then reduces B values per face.
__global__ __launch_bounds__(256) void k_vw_mark(const int64_t *__restrict__ face_idx, int64_t HW, int F,
                                                 uint8_t *__restrict__ vis)
{
    int b = blockIdx.y;
    const int64_t *p = face_idx + (size_t)b * HW;
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2; i < HW; i += (int64_t)gridDim.x * 512) {
        int64_t f0 = p[i];
        int64_t f1 = (i + 1 < HW) ? p[i + 1] : -1;
        if (f0 >= 0 && f0 < F) vis[(size_t)b * F + f0] = 1;      // a face id outside [0, F) must not become a stray store
        if (f1 >= 0 && f1 < F) vis[(size_t)b * F + f1] = 1;
    }
}

__global__ void k_vw_reduce(const uint8_t *__restrict__ vis, const float *__restrict__ fnz, int B, int F,
                            float *__restrict__ max_z)
{
    int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    float m = max_z[f];
    for (int b = 0; b < B; ++b)
        if (vis[(size_t)b * F + f]) {
            float z = fnz[(size_t)b * F + f];
            if (z > m) m = z;
        }
    max_z[f] = m;
}

__global__ __launch_bounds__(256) void k_vw_mask(const int64_t *__restrict__ face_idx, const float *__restrict__ fnz,
                                                 const float *__restrict__ max_z, int64_t HW, int F,
                                                 uint8_t *__restrict__ mask)
{
    int b = blockIdx.y;
    const int64_t *p = face_idx + (size_t)b * HW;
    uint8_t *o = mask + (size_t)b * HW;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += (int64_t)gridDim.x * 256) {
        int64_t f = p[i];
        uint8_t m = 1;
        if (f >= 0 && f < F) m = !(fnz[(size_t)b * F + f] < max_z[f]);
        o[i] = m;
    }
}

extern "C" int32_t ctx_view_weights_max(const int64_t *face_idx, const float *fnz, int32_t B, int32_t HW, int32_t F,
                                        float *max_z, void *vis_ws, ctx_stream_t stream)
{
    CTX_REQUIRE(face_idx && fnz && max_z && vis_ws && B > 0 && HW > 0 && F > 0, "view_weights_max: bad args");
    hipStream_t s = (hipStream_t)stream;
    (void)hipMemsetAsync(vis_ws, 0, (size_t)B * F, s);
    int nb = min(cdiv(HW, 512), 2048);
    hipLaunchKernelGGL(k_vw_mark, dim3(nb, B), dim3(256), 0, s, face_idx, (int64_t)HW, F, (uint8_t *)vis_ws);
    hipLaunchKernelGGL(k_vw_reduce, dim3(cdiv(F, 256)), dim3(256), 0, s, (const uint8_t *)vis_ws, fnz, B, F, max_z);
    CTX_CHECK_LAUNCH("view_weights_max");
    return CTX_OK;
}

extern "C" int32_t ctx_view_weights_mask(const int64_t *face_idx, const float *fnz, const float *max_z, int32_t B,
                                         int32_t HW, int32_t F, uint8_t *mask, ctx_stream_t stream)
{
    CTX_REQUIRE(face_idx && fnz && max_z && mask && B > 0 && HW > 0 && F > 0, "view_weights_mask: bad args");
    int nb = min(cdiv(HW, 256), 4096);
    hipLaunchKernelGGL(k_vw_mask, dim3(nb, B), dim3(256), 0, (hipStream_t)stream, face_idx, fnz, max_z, (int64_t)HW, F, mask);
    CTX_CHECK_LAUNCH("view_weights_mask");
    return CTX_OK;
}
