// Per-ray weighted sum of per-sample values on the marched sample lists: out[r, c] = sum_i w_i * v_{i,c} over the samples
// ray_off[r] .. ray_off[r+1] (the sequential restatement: tests/hashgrid_grad_rule.py).  It is what a
// torch.index_add_ of weights[:, None] * values by ray_id would give, without its float atomics: one wavefront per ray, lane s of chunk c
// holds sample ray_off[r] + 64c + s (ray_wave.h), every lane adds its products over the chunks in ascending order and one wave sum closes
// the ray.  Built with -ffp-contract=off: the product rounds before it is added.  No atomics; every output element has one writer, so
// two runs give the same bits.
#include "ray_wave.h"

template <int C>
__global__ __launch_bounds__(256) void k_weighted_sum_packed(const float *__restrict__ weights, const float *__restrict__ values,
                                                             const int64_t *__restrict__ ray_off, int64_t R, int64_t n, float *__restrict__ out)
{
    const ray_wave rw = ray_wave_here();
    const int lane = rw.lane;
    for (int64_t r = rw.first; r < R; r += rw.stride) {
        int64_t off;
        const int S = packed_count(ray_off, r, n, off);
        float part[C];
#pragma unroll
        for (int c = 0; c < C; ++c) part[c] = 0.f;
        for (int s = lane; s < S; s += 64) {                            // S <= INT32_MAX - 63: s + 64 stays an int
            const float w = weights[off + s];
            const float *v = values + (off + s) * C;
#pragma unroll
            for (int c = 0; c < C; ++c) part[c] = part[c] + w * v[c];
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float sum = wave_sum_dpp(part[c]);                    // an empty ray: zeros
            if (lane == 0) out[r * C + c] = sum;
        }
    }
}

extern "C" int32_t ctx_weighted_sum_packed(const float *weights, const float *values, const int64_t *ray_off, int64_t R, int64_t n, int32_t C,
                                           float *out, ctx_stream_t stream)
{
    CTX_REQUIRE(ray_off && out && R > 0, "weighted_sum_packed: bad args");
    CTX_REQUIRE(C >= 1 && C <= 4, "weighted_sum_packed: C=%d outside [1, 4]", C);
    CTX_REQUIRE(n >= 0 && n <= INT32_MAX, "weighted_sum_packed: n=%lld outside [0, 2^31)", (long long)n);
    CTX_REQUIRE(n == 0 || (weights && values), "weighted_sum_packed: null list with n=%lld", (long long)n);
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        if (hipMemsetAsync(out, 0, (size_t)R * C * sizeof(float), s) != hipSuccess) {
            ctx_set_error("weighted_sum_packed: memset failed");
            return CTX_E_LAUNCH;
        }
        return CTX_OK;
    }
    const dim3 grid(ray_blocks(R)), block(256);
    if (C == 1) hipLaunchKernelGGL(k_weighted_sum_packed<1>, grid, block, 0, s, weights, values, ray_off, R, n, out);
    else if (C == 2) hipLaunchKernelGGL(k_weighted_sum_packed<2>, grid, block, 0, s, weights, values, ray_off, R, n, out);
    else if (C == 3) hipLaunchKernelGGL(k_weighted_sum_packed<3>, grid, block, 0, s, weights, values, ray_off, R, n, out);
    else hipLaunchKernelGGL(k_weighted_sum_packed<4>, grid, block, 0, s, weights, values, ray_off, R, n, out);
    CTX_CHECK_LAUNCH("weighted_sum_packed");
    return CTX_OK;
}
