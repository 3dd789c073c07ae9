// Mask operators of the progressive paint loop (trainer.py: calculate_trimap, projection_weight, paint_progressive) and its atlas update.
// TEXTure (Richardson et al. 2023, sections 3.2-3.3) does the mask work with OpenCV on the host, one device-to-host round trip per view;
// here the masks never leave the device.  The rules are written out in include/ctx_nerf.h and restated in numpy in tests/trimap_rule.py.
//
//   ctx_mask_morph   k x k dilate (max) / erode (min), window clipped to the image        row pass -> ws, column pass -> dst
//   ctx_sep_filter   k-tap separable filter, reflect padding without the edge pixel        row pass -> ws, column pass -> dst
//   ctx_atlas_blend  acc <- acc blended with one view's contribution, per texel            one launch
//
// Both separable operators are ONE pair of kernels, templated on the operator: k_mo_rows (a block owns 4 rows x 256 columns; every row
// segment sits in LDS with its halo of k/2 on both sides; a lane makes 4 consecutive outputs and stores one dwordx4 where the row pitch
// and the base allow it) and k_mo_cols (a block owns 64 columns x 32 rows; the tile and its halo of k/2 rows sit in LDS as rows of 64
// floats, so a wave reads one LDS row per step without a bank conflict and global rows stay coalesced; a lane makes 8 outputs of one column).
// What lies outside the image is decided when the halo is staged: the operator's neutral element for min / max (the window is clipped),
// the reflected pixel for the filter.  The taps travel in the kernel arguments: no device copy, no host sync.
// One writer per element, no atomics; this file is built without FMA contraction (Makefile: EXACT), every float operation rounds on
// its own in the order written.
#include "common.h"
#include <math.h>

#define MO_MAXK 63
#define MO_R (MO_MAXK / 2)
#define MO_BLK 256
#define MO_RW 256                 // k_mo_rows: columns per block (64 lanes x 4)
#define MO_RH 4                   //            rows per block (one wave each)
#define MO_CW 64                  // k_mo_cols: columns per block (one lane each)
#define MO_CH 32                  //            rows per block (4 waves x 8)
#define MO_CPER (MO_CH / 4)

enum { MO_MAX = 0, MO_MIN = 1, MO_FILTER = 2 };

struct MoTaps {
    float w[MO_MAXK];
};

// source index of tap position i on an axis of n pixels: min / max skip what is outside (-1), the filter reflects without repeating the
// edge (-1 -> 1, n -> n - 2; one reflection reaches everything because k/2 <= n - 1).  A position the reflection cannot place belongs to
// an output beyond the image and is never read back.
template <int OP>
__device__ __forceinline__ int mo_source(int i, int n)
{
    if (OP == MO_FILTER) {
        if (i < 0) i = -i;
        if (i >= n) i = 2 * (n - 1) - i;
    }
    return (i >= 0 && i < n) ? i : -1;
}

template <int OP>
__device__ __forceinline__ float mo_neutral()
{
    return OP == MO_MAX ? -INFINITY : OP == MO_MIN ? INFINITY : 0.f;
}

// acc <- acc (op) tap j of the window, left to right
template <int OP>
__device__ __forceinline__ float mo_step(float acc, float v, float w, bool first)
{
    if (OP == MO_MAX) return fmaxf(acc, v);
    if (OP == MO_MIN) return fminf(acc, v);
    const float p = w * v;
    return first ? p : acc + p;
}

template <int OP>
__global__ __launch_bounds__(MO_BLK) void k_mo_rows(const float *__restrict__ src, int rows, int W, int k, MoTaps taps, int vec, float *__restrict__ dst)
{
    __shared__ float s[MO_RH][MO_RW + 2 * MO_R + 2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = k >> 1;
    const int ntx = (W + MO_RW - 1) / MO_RW;
    const int x0 = (int)(blockIdx.x % ntx) * MO_RW;
    const int64_t row = (int64_t)(blockIdx.x / ntx) * MO_RH + wv;
    if (row < rows) {
        const float *line = src + row * W;
        for (int j = lane; j < MO_RW + 2 * r; j += 64) {
            const int xs = mo_source<OP>(x0 - r + j, W);
            s[wv][j] = xs >= 0 ? line[xs] : mo_neutral<OP>();
        }
    }
    __syncthreads();
    if (row >= rows) return;
    const int lx = lane * 4, x = x0 + lx;
    if (x >= W) return;
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = mo_neutral<OP>();
    for (int j = 0; j < k; ++j) {
        const float w = OP == MO_FILTER ? taps.w[j] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = mo_step<OP>(o[i], s[wv][lx + i + j], w, j == 0);
    }
    float *out = dst + row * W + x;
    if (vec && x + 3 < W) {
        *(f32x4 *)out = f32x4{o[0], o[1], o[2], o[3]};
    } else {
        for (int i = 0; i < 4 && x + i < W; ++i) out[i] = o[i];
    }
}

template <int OP>
__global__ __launch_bounds__(MO_BLK) void k_mo_cols(const float *__restrict__ src, int H, int W, int k, MoTaps taps, float *__restrict__ dst)
{
    __shared__ float s[MO_CH + 2 * MO_R][MO_CW];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = k >> 1;
    const int ntx = (W + MO_CW - 1) / MO_CW, nty = (H + MO_CH - 1) / MO_CH;
    const int tx = (int)(blockIdx.x % ntx), ty = (int)((blockIdx.x / ntx) % nty);
    const int64_t n = blockIdx.x / ((int64_t)ntx * nty);
    const int x = tx * MO_CW + lane, y0 = ty * MO_CH;
    const float *img = src + n * H * W;
    for (int j = wv; j < MO_CH + 2 * r; j += 4) {
        const int ys = mo_source<OP>(y0 - r + j, H);
        s[j][lane] = (ys >= 0 && x < W) ? img[(int64_t)ys * W + x] : mo_neutral<OP>();
    }
    __syncthreads();
    if (x >= W) return;
    const int ly = wv * MO_CPER;
    float o[MO_CPER];
#pragma unroll
    for (int i = 0; i < MO_CPER; ++i) o[i] = mo_neutral<OP>();
    for (int j = 0; j < k; ++j) {
        const float w = OP == MO_FILTER ? taps.w[j] : 0.f;
#pragma unroll
        for (int i = 0; i < MO_CPER; ++i) o[i] = mo_step<OP>(o[i], s[ly + i + j][lane], w, j == 0);
    }
    float *out = dst + n * H * W;
#pragma unroll
    for (int i = 0; i < MO_CPER; ++i)
        if (y0 + ly + i < H) out[(int64_t)(y0 + ly + i) * W + x] = o[i];
}

template <int OP>
static void mo_launch(const float *src, int N, int H, int W, int k, const MoTaps &taps, float *dst, float *ws, hipStream_t s)
{
    const int rows = N * H;
    const int vec = (W % 4 == 0) && (((uintptr_t)ws & 15) == 0);
    const unsigned gr = (unsigned)(cdiv(W, MO_RW) * (int64_t)cdiv(rows, MO_RH));
    const unsigned gc = (unsigned)((int64_t)cdiv(W, MO_CW) * cdiv(H, MO_CH) * N);
    hipLaunchKernelGGL(k_mo_rows<OP>, dim3(gr), dim3(MO_BLK), 0, s, src, rows, W, k, taps, vec, ws);
    hipLaunchKernelGGL(k_mo_cols<OP>, dim3(gc), dim3(MO_BLK), 0, s, (const float *)ws, H, W, k, taps, dst);
}

#define MO_CHECK_COMMON(who)                                                                                                                      \
    CTX_REQUIRE(src && dst && ws, who ": null pointer");                                                                                          \
    CTX_REQUIRE(N >= 1 && H >= 1 && W >= 1 && (int64_t)N * H * W < (1ll << 31), who ": N=%d, H=%d, W=%d: want each >= 1 and N*H*W < 2^31", (int)N, \
                (int)H, (int)W);                                                                                                                  \
    CTX_REQUIRE(k >= 1 && k <= MO_MAXK && (k & 1), who ": k=%d: want an odd k in [1, %d]", (int)k, MO_MAXK);                                        \
    CTX_REQUIRE((const float *)dst != src, who ": dst must not be src");                                                                            \
    CTX_REQUIRE((const float *)ws != src && ws != dst, who ": the workspace of N*H*W floats must be neither src nor dst")

extern "C" int32_t ctx_mask_morph(const float *src, int32_t N, int32_t H, int32_t W, int32_t k, int32_t op, float *dst, float *ws, ctx_stream_t stream)
{
    MO_CHECK_COMMON("mask_morph");
    CTX_REQUIRE(op == MO_MAX || op == MO_MIN, "mask_morph: op=%d: want 0 (dilate) or 1 (erode)", (int)op);
    const MoTaps none = {};
    if (op == MO_MAX) mo_launch<MO_MAX>(src, N, H, W, k, none, dst, ws, (hipStream_t)stream);
    else mo_launch<MO_MIN>(src, N, H, W, k, none, dst, ws, (hipStream_t)stream);
    CTX_CHECK_LAUNCH("mask_morph");
    return CTX_OK;
}

extern "C" int32_t ctx_sep_filter(const float *src, int32_t N, int32_t H, int32_t W, const float *taps, int32_t k, float *dst, float *ws, ctx_stream_t stream)
{
    MO_CHECK_COMMON("sep_filter");
    CTX_REQUIRE(taps, "sep_filter: null pointer (taps)");
    CTX_REQUIRE(k / 2 <= (H < W ? H : W) - 1, "sep_filter: k=%d reflects further than a %d x %d image reaches: want k/2 <= min(H, W) - 1", (int)k, (int)H,
                (int)W);
    MoTaps t = {};
    for (int j = 0; j < k; ++j) t.w[j] = taps[j];
    mo_launch<MO_FILTER>(src, N, H, W, k, t, dst, ws, (hipStream_t)stream);
    CTX_CHECK_LAUNCH("sep_filter");
    return CTX_OK;
}

// ---- the progressive atlas update --------------------------------------------------------------------------------------------------
#define AB_ONE (1ll << 32)

__device__ __forceinline__ float ab_float(long long v) { return (float)ldexp((double)v, -32); }     // ctx_fixed_to_float's conversion
__device__ __forceinline__ long long ab_fixed(float v) { return __float2ll_rn(ldexpf(v, 32)); }     // k_sb_direct's conversion

__global__ __launch_bounds__(256) void k_atlas_blend(const long long *__restrict__ contrib, const long long *__restrict__ zsum, int64_t TT,
                                                     long long *__restrict__ acc, float *__restrict__ meta)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= TT) return;
    const long long w = contrib[3 * TT + p];
    if (w <= 0) return;
    const float wf = ab_float(w);
    const float m = fminf(1.f, wf);
    const float z = ab_float(zsum[p]) / wf;
    const long long aw = acc[3 * TT + p];
    const bool fresh = aw <= 0;
    const float awf = fresh ? 1.f : ab_float(aw), keep = 1.f - m;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float nw = ab_float(contrib[c * TT + p]) / wf;
        float out = nw;
        if (!fresh) {
            const float old = ab_float(acc[c * TT + p]) / awf;
            out = old * keep + nw * m;
        }
        acc[c * TT + p] = ab_fixed(out);
    }
    acc[3 * TT + p] = AB_ONE;
    meta[p] = fresh ? z : meta[p] * keep + z * m;
}

extern "C" int32_t ctx_atlas_blend(const int64_t *contrib, const int64_t *zsum, int32_t T, int64_t *acc, float *meta, ctx_stream_t stream)
{
    CTX_REQUIRE(contrib && zsum && acc && meta, "atlas_blend: null pointer");
    CTX_REQUIRE(T >= 1 && T <= 16384, "atlas_blend: T=%d outside [1, 16384]", (int)T);
    CTX_REQUIRE(contrib != acc && zsum != acc, "atlas_blend: acc must not be contrib or zsum");
    const int64_t TT = (int64_t)T * T;
    hipLaunchKernelGGL(k_atlas_blend, dim3((unsigned)cdiv64(TT, 256)), dim3(256), 0, (hipStream_t)stream, (const long long *)contrib, (const long long *)zsum, TT,
                       (long long *)acc, meta);
    CTX_CHECK_LAUNCH("atlas_blend");
    return CTX_OK;
}
