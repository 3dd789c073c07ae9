// What the 3-D hash-grid encoding (hashgrid.hip) and the 2-D texture field (hashtex.hip) share: the limits, the vector type of one table
// entry, and the control words and helper kernels of the integer accumulator of the table's gradient (DESIGN sections 4j, 4l).
#pragma once
#include "common.h"
#include <math.h>

#define HG_MAX_LEVELS 16
#define HG_BLOCK 256

template <int F> struct HgVec;
template <> struct HgVec<1> { typedef float type; };
template <> struct HgVec<2> { typedef float2 type; };
template <> struct HgVec<4> { typedef float4 type; };

// absmax: bits of max|g_emb| (the order of non-negative floats is the order of their bits; inf and NaN sort above every finite value);
// status: 0 = accumulate, 1 = all zero, 2 = a non-finite gradient poisons the table's gradient;  x: 2^x is the smallest power of two above m
struct HgCtl { uint32_t absmax; int32_t status; int32_t x; int32_t pad; };

static __global__ __launch_bounds__(HG_BLOCK) void k_hashgrid_absmax(const float *__restrict__ g, int64_t count, HgCtl *__restrict__ ctl)
{
    uint32_t m = 0;
    const int64_t stride = (int64_t)gridDim.x * HG_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * HG_BLOCK + threadIdx.x; i < count; i += stride) m = max(m, __float_as_uint(g[i]) & 0x7fffffffu);
    for (int o = 32; o; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
    __shared__ uint32_t s_m[HG_BLOCK / 64];
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {                        // one atomic per workgroup
        for (int k = 1; k < HG_BLOCK / 64; ++k) m = max(m, s_m[k]);
        if (m) atomicMax(&ctl->absmax, m);
    }
}

static __global__ void k_hashgrid_scale(HgCtl *ctl)
{
    const uint32_t b = ctl->absmax;
    int status = 0, x = 0;
    if (b == 0) status = 1;
    else if (b >= 0x7f800000u) status = 2;
    else if (b >> 23) x = (int)(b >> 23) - 126;    // m = 1.f * 2^(e - 127) < 2^(e - 126)
    else x = (31 - __clz((int)b)) - 148;           // subnormal: top bit p is worth 2^(p - 149)
    ctl->status = status;
    ctl->x = x;
}

// the exact power of two 2^e as a double, -1022 <= e <= 1023
__device__ __forceinline__ double hg_pow2(int e) { return __longlong_as_double((long long)(1023 + e) << 52); }

static __global__ __launch_bounds__(HG_BLOCK) void k_hashgrid_convert(const long long *__restrict__ acc, int64_t count, int E, const HgCtl *__restrict__ ctl,
                                                               float *__restrict__ g_table)
{
    const int status = ctl->status;
    const double inv = hg_pow2(ctl->x - E);
    const int64_t stride = (int64_t)gridDim.x * HG_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * HG_BLOCK + threadIdx.x; i < count; i += stride)
        g_table[i] = status == 2 ? __uint_as_float(0x7fc00000u) : (status == 1 ? 0.0f : (float)((double)acc[i] * inv));
}

static inline int64_t hg_align(int64_t x) { return (x + 255) & ~(int64_t)255; }

// E = 62 - ceil(log2(corners * n)), corners 8 (3-D) or 4 (2-D): an entry receives at most corners * n terms, each at most 2^E.  The
// accumulate, the convert and the table optimizer (adam.hip) must agree on it, so all three take it from here.
static inline int hg_acc_exponent(int64_t n, int corners)
{
    const int lc = corners == 8 ? 3 : 2;
    int c = lc;
    while (((int64_t)1 << (c - lc)) < n) ++c;
    return 62 - c;
}

