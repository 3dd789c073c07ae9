// One wavefront per ray, 256-thread blocks, grid-stride over the rays: the frame of the seven wave-per-ray kernels (composite.hip,
// distortion.hip, resample.hip).  Lane s of chunk c holds sample 64c + s of the wave's ray.
#pragma once
#include "wave_scan.h"

// for (int64_t r = rw.first; r < R; r += rw.stride)
struct ray_wave {
    int lane;
    int64_t first, stride;
};
__device__ __forceinline__ ray_wave ray_wave_here()
{
    return {(int)(threadIdx.x & 63), ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, ((int64_t)gridDim.x * 256) >> 6};
}

__device__ __forceinline__ float ray_norm(const float *__restrict__ rays_d, int64_t r)
{
    const float d0 = rays_d[r * 3 + 0], d1 = rays_d[r * 3 + 1], d2 = rays_d[r * 3 + 2];
    return sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
}

// Samples of ray r of a ragged list of n < 2^31 samples, off <- its first.  A ray_off outside the list reads nothing, nor does a ray whose
// 64 * chunks would leave an int: end - off <= INT32_MAX - 63, tested on the int (inside the list the difference is below 2^31).
__device__ __forceinline__ int packed_count(const int64_t *__restrict__ ray_off, int64_t r, int64_t n, int64_t &off)
{
    off = ray_off[r];
    const int64_t end = ray_off[r + 1];
    const int S = (off >= 0 && end >= off && end <= n) ? (int)(end - off) : 0;
    return S <= INT32_MAX - 63 ? S : 0;
}

static inline unsigned ray_blocks(int64_t R) { return capped_blocks(R, 4, 262144); }          // one ray per wave up to 1 M rays
