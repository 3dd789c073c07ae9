// Normalisation kernels of the UNet denoiser and the VAE (NHWC fp16 activations or the fp32 residual stream, fp32 statistics).
// HBM-bound: every access is a 16-byte (8 x f16) vector per lane.
//   GroupNorm(+SiLU)   diffusers ResnetBlock2D norm1/norm2, Transformer2DModel.norm, conv_norm_out: the two-pass form
//                      (k_gn_stats, k_gn_apply), the one-kernel form (k_gn_fused) and the backward (k_gnb_*)
//   LayerNorm          BasicTransformerBlock norm1/2/3: one wave per row(s) (k_layernorm) or 8 lanes per row (k_layernorm_g8)
// The other elementwise kernels of the engines live in elementwise.hip.
#include "common.h"
#include "kernels.h"
#include <math.h>

// ------------------------------------------------------------------------------------------------
// GroupNorm.  Both passes are latency-bound at the UNet's sizes (a 12 MB tensor is ~2 HBM latencies deep), so the
// structure is "every load of a thread in flight at once":
// Pass 1: grid (NS, B), block = C/8 chunk columns x PL pixel lanes (~1000 threads); a thread owns 8 channels and
// walks its split GN_U pixels at a time, each batch loaded before its first add; per-channel partials -> LDS -> per-group
// sums.  NS by sample size (16-32 for the UNet's tensors, 128 for the VAE's: see the launcher).
// Pass 2: grid (nb, B), block = C/8 chunk columns x >= 256/(C/8) pixel lanes; a thread keeps ONE column (scale / shift in
// registers), issues its GN_AU 16-byte loads first, then the block folds the NS split partials per (b, group) in a fixed
// order (deterministic: no float atomics anywhere in GroupNorm) while they fly.

// 8 consecutive channels of the input as they lie in memory: fp16 activations (16 bytes) or the fp32 residual stream (32 bytes).
// get(j) converts at use (4 VGPRs per chunk in flight as fp16, 8 as floats); widen() converts at load, for the kernels that
// read every value more than once.
struct Wide8 {
    float v[8];
    __device__ __forceinline__ float get(int j) const { return v[j]; }
};
template <bool X32> struct Raw8;
template <> struct Raw8<false> {
    f16x8 a;
    __device__ __forceinline__ float get(int j) const { return (float)a[j]; }
    __device__ __forceinline__ Wide8 widen() const
    {
        Wide8 r;
#pragma unroll
        for (int j = 0; j < 8; ++j) r.v[j] = (float)a[j];
        return r;
    }
};
template <> struct Raw8<true> {
    f32x4 a, b;
    __device__ __forceinline__ float get(int j) const { return j < 4 ? a[j] : b[j - 4]; }
    __device__ __forceinline__ Wide8 widen() const
    {
        Wide8 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) { r.v[j] = a[j]; r.v[4 + j] = b[j]; }
        return r;
    }
};
template <bool X32>
__device__ __forceinline__ Raw8<X32> ldraw(const void *base, size_t elem)
{
    Raw8<X32> r;
    if constexpr (X32) { r.a = *(const f32x4 *)((const float *)base + elem); r.b = *(const f32x4 *)((const float *)base + elem + 4); }
    else r.a = *(const f16x8 *)((const f16 *)base + elem);
    return r;
}

// Two-source input (x2 != null): the tensor is the channel concatenation [x ; x2] that nobody materialised: channels 0 .. Ca lie in
// x with pixel stride Ca, channels Ca .. C in x2 with pixel stride C - Ca (the up blocks' [hidden ; skip]).  A thread owns one
// 8-channel column, so it picks its source once; thread-to-channel mapping and summation order are those of the one-source form,
// which makes the result bit-identical to GroupNorm of the materialised concat.
struct GnSrc { const void *p; int cs, col; };         // source, its pixel stride, the column's first channel inside it
__device__ __forceinline__ GnSrc gn_src(const void *x, const void *x2, int Ca, int C, int ch)
{
    if (!x2) return {x, C, ch};
    return ch < Ca ? GnSrc{x, Ca, ch} : GnSrc{x2, C - Ca, ch - Ca};
}

// Statistics are accumulated about a per-(sample, group) pivot, the group's first channel at pixel 0 (from whichever source holds
// it): sum (x - pivot) and sum (x - pivot)^2.  var = sumsq/n - mean^2 of the raw values cancels to nothing once a group's mean is a few
// hundred of its sigmas away from zero; about a member of the group the two terms are of the variance's own size.  x - pivot is exact
// (fp16 input) or rounded once at the size of the difference, not of x.
template <bool X32>
__device__ __forceinline__ float gn_pivot(const void *x, const void *x2, int Ca, int C, int HW, int b, int ch)
{
    const GnSrc s = gn_src(x, x2, Ca, C, ch);
    const size_t e = (size_t)b * HW * s.cs + s.col;
    if constexpr (X32) return ((const float *)s.p)[e];
    else return (float)((const f16 *)s.p)[e];
}
// a thread's 8 channels ch0 .. ch0 + 8 (ch0 % 8 == 0): they lie in one group when a group is whole chunks, in at most two when it
// is wider than a chunk (the UNet's 10 .. 80 channels: two loads and a select, no branch per channel), else one load per group
template <bool X32>
__device__ __forceinline__ void gn_pivots(const void *x, const void *x2, int Ca, int C, int HW, int b, int ch0, int cg, float (&pv)[8])
{
    int first = ch0 / cg * cg, next = first + cg;          // the first channel of channel ch0's group, and of the group behind it
    float t = gn_pivot<X32>(x, x2, Ca, C, HW, b, first);
    if (cg % 8 == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) pv[j] = t;
    } else if (cg > 8) {
        const float t1 = gn_pivot<X32>(x, x2, Ca, C, HW, b, min(next, C - cg));     // next == C: no channel of this thread is behind it
#pragma unroll
        for (int j = 0; j < 8; ++j) pv[j] = ch0 + j >= next ? t1 : t;
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (ch0 + j >= next) { first = next; next += cg; t = gn_pivot<X32>(x, x2, Ca, C, HW, b, first); }
            pv[j] = t;
        }
    }
}

#define GN_MAX_GROUPS 64
#define GN_MAX_SPLITS CTX_GN_MAX_SLOTS
#define GN_MAX_C 4096
#define GN_U 4
#define GN_AU 6
#define GN_FOLD 8

template <bool X32>
__global__ __launch_bounds__(1024) void k_gn_stats(const void *__restrict__ x, const void *__restrict__ x2, int Ca, int HW, int C, int G,
                                                   int NS, int PL, float *__restrict__ part)
{
    extern __shared__ float s_part[];          // [PL][C][2]
    const int c8n = C / 8;
    const int b = blockIdx.y, sp = blockIdx.x;
    const int c8 = threadIdx.x % c8n, pl = threadIdx.x / c8n;
    const bool act = pl < PL;                  // blockDim.x is rounded up to whole waves: the lanes behind c8n * PL only help folding
    const int per = (HW + NS - 1) / NS;
    const int p0 = sp * per, p1 = min(HW, p0 + per);
    float s[8], q[8], pv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s[j] = 0.f; q[j] = 0.f; }
    gn_pivots<X32>(x, x2, Ca, C, HW, b, c8 * 8, C / G, pv);
    const GnSrc src = gn_src(x, x2, Ca, C, c8 * 8);
    const size_t base = ((size_t)b * HW) * src.cs + src.col;
    for (int p = p0 + pl; act && p < p1; p += PL * GN_U) {
        Wide8 v[GN_U];
#pragma unroll
        for (int u = 0; u < GN_U; ++u) v[u] = ldraw<X32>(src.p, base + (size_t)min(p + u * PL, p1 - 1) * src.cs).widen();   // unconditional
#pragma unroll
        for (int u = 0; u < GN_U; ++u) {
            const bool live = p + u * PL < p1;
#pragma unroll
            for (int j = 0; j < 8; ++j) { float f = live ? v[u].get(j) - pv[j] : 0.f; s[j] += f; q[j] += f * f; }
        }
    }
    if (act) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            s_part[((size_t)pl * C + c8 * 8 + j) * 2 + 0] = s[j];
            s_part[((size_t)pl * C + c8 * 8 + j) * 2 + 1] = q[j];
        }
    }
    __syncthreads();
    // fixed-order fold, two short steps.  A: (channel, slice a of the pixel lanes) -> s_ch[a][C]; B: 8 lanes per group
    // walk that group's na x cg cells, then a shuffle tree.
    float *s_ch = s_part + (size_t)PL * C * 2;
    const int na = max(1, (int)blockDim.x / C);
    for (int it = threadIdx.x; it < C * na; it += blockDim.x) {
        const int a = it / C, c = it - a * C;
        float ss = 0.f, qq = 0.f;
#pragma unroll 4
        for (int l = a; l < PL; l += na) {
            ss += s_part[((size_t)l * C + c) * 2 + 0];
            qq += s_part[((size_t)l * C + c) * 2 + 1];
        }
        s_ch[((size_t)a * C + c) * 2 + 0] = ss;
        s_ch[((size_t)a * C + c) * 2 + 1] = qq;
    }
    __syncthreads();
    const int cg = C / G, cells = na * cg;
    const int octs = (int)blockDim.x >> 3;               // whole 8-lane groups (blockDim.x is whole waves: octs >= 8)
    for (int g0 = 0; g0 < G; g0 += octs) {
        const int oc = (int)threadIdx.x >> 3, l = threadIdx.x & 7;
        const int g = oc < octs ? g0 + oc : G;
        float ss = 0.f, qq = 0.f;
        if (g < G)
            for (int k = l; k < cells; k += 8) {
                int a = k / cg, c = g * cg + (k - a * cg);
                ss += s_ch[((size_t)a * C + c) * 2 + 0];
                qq += s_ch[((size_t)a * C + c) * 2 + 1];
            }
#pragma unroll
        for (int o = 4; o > 0; o >>= 1) { ss += __shfl_xor(ss, o, 64); qq += __shfl_xor(qq, o, 64); }
        if (g < G && l == 0) {
            part[(((size_t)b * NS + sp) * G + g) * 2 + 0] = ss;
            part[(((size_t)b * NS + sp) * G + g) * 2 + 1] = qq;
        }
    }
}

// (mean, rstd) of n values from the sum and the sum of squares of their distances to `pivot` (0: of the values themselves, which is
// what a producer's epilogue can write)
__device__ __forceinline__ float2 gn_mean_rstd(float sum, float sumsq, float n, float eps, float pivot)
{
    const float m = sum / n;
    return make_float2(pivot + m, rsqrtf(fmaxf(sumsq / n - m * m, 0.f) + eps));
}
// y = x * sa + sh for a thread's 8 channels; mr(j) gives channel j's (mean, rstd)
template <class MR>
__device__ __forceinline__ void gn_scale_shift(MR mr, f16x8 ga, f16x8 be, float (&sa)[8], float (&sh)[8])
{
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float2 m = mr(j);
        sa[j] = m.y * (float)ga[j];
        sh[j] = (float)be[j] - m.x * sa[j];
    }
}
// one chunk: scale / shift, SiLU as x * rcp(1 + exp2(-log2(e) x)) when `silu`, one rounding, one 16-byte store
template <class V8>
__device__ __forceinline__ void gn_store(const V8 &v, const float (&sa)[8], const float (&sh)[8], int silu, f16 *dst)
{
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float t = v.get(j) * sa[j] + sh[j];
        if (silu) t = t * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * t));
        o[j] = (f16)t;
    }
    *(f16x8 *)dst = o;
}

// GN_AU = 6 chunks per thread measured best over the UNet's shapes (4 / 6 / 8 / 12: 6.7 / 5.8 / 6.4 / 7.7 us at 2304 x 640 x batch 2,
// 9.0 / 9.2 / 10.5 / 9.5 at 9216 x 320): with 12 a SIMD holds one wave whose ~1.7 us of SiLU arithmetic follows its loads instead of
// hiding under another wave's
// Pass 2.  Block = c8n chunk columns x PL pixel lanes (>= 256 threads); a thread owns ONE column of 8 channels, so its scale and shift
// live in 16 registers, and walks AU pixels of the block's contiguous pixel run, all AU 16-byte loads in flight before anything else
// (the fold of the split partials happens under them).  The form before this one let a thread's column vary with the chunk and
// fetched scale / shift from an LDS table: four ds_read_b128 per chunk at a 32-byte lane stride, i.e. bank-conflicted LDS reads of
// four times the payload — tools/probes/stream_probe.hip: a copy-shaped kernel goes from 3.9 to 8.8 us on 12 MB with exactly that
// table read added, and stays at 4.3 with the values in registers (SiLU and the index arithmetic cost nothing measurable).
template <bool X32>
__global__ __launch_bounds__(512) void k_gn_apply(const void *__restrict__ x, const void *__restrict__ x2, int Ca, const float *__restrict__ part,
                                                  const f16 *__restrict__ gamma, const f16 *__restrict__ beta, int HW, int C,
                                                  int G, int NS, int PL, int piv, float eps, int silu, f16 *__restrict__ y)
{
    // piv: the partials are k_gn_stats' (about the group's pivot, added back here); 0: a producer's (plain sums)
    constexpr int AU = GN_AU;
    __shared__ float s_mean[GN_MAX_GROUPS], s_rstd[GN_MAX_GROUPS];
    const int b = blockIdx.y;
    const int c8n = C / 8;
    const int c8 = threadIdx.x % c8n, pl = threadIdx.x / c8n;
    const int p0 = blockIdx.x * (PL * AU);
    const GnSrc src = gn_src(x, x2, Ca, C, c8 * 8);
    const size_t xb = (size_t)b * HW * src.cs + src.col;
    f16 *yb = y + (size_t)b * HW * C + c8 * 8;
    Raw8<X32> v[AU];
#pragma unroll
    for (int u = 0; u < AU; ++u) v[u] = ldraw<X32>(src.p, xb + (size_t)min(p0 + u * PL + pl, HW - 1) * src.cs);    // unconditional (clamped)
    const f16x8 ga = *(const f16x8 *)(gamma + c8 * 8), be = *(const f16x8 *)(beta + c8 * 8);
    if (threadIdx.x < 256) {
        const int lpg = min(256 / G, 64);                                   // lanes per group: a power of two inside one wave (G < 4: idle lanes)
        const int gi = threadIdx.x / lpg, l = threadIdx.x % lpg;
        const int g = min(gi, G - 1);
        const float pivot = piv ? gn_pivot<X32>(x, x2, Ca, C, HW, b, g * (C / G)) : 0.f;
        float s = 0.f, q = 0.f;
        for (int k0 = 0; k0 < NS; k0 += GN_FOLD * lpg) {                    // GN_FOLD independent loads per trip, fixed order
            float2 pv[GN_FOLD];
#pragma unroll
            for (int k = 0; k < GN_FOLD; ++k)
                pv[k] = *(const float2 *)(part + (((size_t)b * NS + min(k0 + k * lpg + l, NS - 1)) * G + g) * 2);
#pragma unroll
            for (int k = 0; k < GN_FOLD; ++k)
                if (k0 + k * lpg + l < NS) { s += pv[k].x; q += pv[k].y; }
        }
        for (int o = lpg >> 1; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); q += __shfl_xor(q, o, 64); }
        if (l == 0 && gi < G) {
            const float2 m = gn_mean_rstd(s, q, (float)HW * (float)(C / G), eps, pivot);
            s_mean[g] = m.x;
            s_rstd[g] = m.y;
        }
    }
    __syncthreads();
    const int cg = C / G;
    float sa[8], sh[8];
    gn_scale_shift([&](int j) { const int gg = (c8 * 8 + j) / cg; return make_float2(s_mean[gg], s_rstd[gg]); }, ga, be, sa, sh);
#pragma unroll
    for (int u = 0; u < AU; ++u) {
        const int p = p0 + u * PL + pl;
        if (p < HW) gn_store(v[u], sa, sh, silu, yb + (size_t)p * C);
    }
}

// Small-tensor GroupNorm in ONE kernel: when a group's channels are whole 16-byte chunks (C/G % 8 == 0) and one
// (batch, group) slab fits a workgroup's registers (<= GN_FT x GN_FU chunks), a workgroup loads its slab once, reduces
// it twice (the mean, then sum (x - mean)^2 over the same registers; fixed order: lane partials -> DPP wave sums -> 8 wave
// partials), and writes the normalised slab from registers.
// At the UNet's two deepest levels this replaces two latency-bound launches and one re-read of the tensor.
// SLAB: the input is a split-K convolution's fp32 slabs (GnSlabs) that no reduce launch has summed: a thread forms the fp16 value the
// reduce would have stored, in its operand order (slabs ascending, bias, bias2, row bias, one rounding: store4 of gemm_common.h), and
// normalises that, bit for bit what it would read from the reduced tensor.
#define GN_FT 512
#define GN_FU 12
__device__ __forceinline__ Wide8 gn_slab_chunk(const GnSlabs &sl, size_t m, int b, int C, int ch)
{
    const float *row = sl.part + m * C + ch;
    f32x4 lo = *(const f32x4 *)row, hi = *(const f32x4 *)(row + 4);
    for (int s = 1; s < sl.S; ++s) { lo += *(const f32x4 *)(row + s * sl.MN); hi += *(const f32x4 *)(row + s * sl.MN + 4); }
    Wide8 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) { r.v[j] = lo[j]; r.v[4 + j] = hi[j]; }
    if (sl.bias) { const f16x8 t = *(const f16x8 *)(sl.bias + ch);
#pragma unroll
        for (int j = 0; j < 8; ++j) r.v[j] += (float)t[j]; }
    if (sl.bias2) { const f16x8 t = *(const f16x8 *)(sl.bias2 + ch);
#pragma unroll
        for (int j = 0; j < 8; ++j) r.v[j] += (float)t[j]; }
    if (sl.rowbias) { const f16x8 t = *(const f16x8 *)(sl.rowbias + (size_t)b * sl.ldrb + ch);
#pragma unroll
        for (int j = 0; j < 8; ++j) r.v[j] += (float)t[j]; }
#pragma unroll
    for (int j = 0; j < 8; ++j) r.v[j] = (float)(f16)r.v[j];
    return r;
}
template <bool X32, bool SLAB = false>
__global__ __launch_bounds__(GN_FT) void k_gn_fused(const void *__restrict__ x, const void *__restrict__ x2, int Ca, const f16 *__restrict__ gamma,
                                                    const f16 *__restrict__ beta, int HW, int C, int G, int PLF, float eps, int silu,
                                                    f16 *__restrict__ y, GnSlabs sl)
{
    // threads = cpg chunk columns x PLF pixel lanes: a thread keeps one column, so gamma / beta are 16 registers (an LDS table read per
    // chunk at a 32-byte lane stride is bank-conflicted and was the slowest part of the apply kernels: tools/probes/stream_probe.hip)
    __shared__ float s_red[2][GN_FT / 64];
    const int g = blockIdx.x, b = blockIdx.y;
    const int cg = C / G, cpg = cg / 8;                // chunks per pixel in this group
    const int c = threadIdx.x % cpg, pl = threadIdx.x / cpg;
    const bool act = pl < PLF;                         // blockDim.x is rounded up to whole waves
    const GnSrc src = gn_src(x, x2, Ca, C, g * cg + c * 8);    // two sources: per column, so a group may straddle Ca
    const size_t xb = (size_t)b * HW * src.cs + src.col;
    f16 *yb = y + (size_t)b * HW * C + g * cg + c * 8;
    const f16x8 ga = *(const f16x8 *)(gamma + g * cg + c * 8), be = *(const f16x8 *)(beta + g * cg + c * 8);
    Wide8 v[GN_FU];
#pragma unroll
    for (int u = 0; u < GN_FU; ++u) {                                                                                     // unconditional (clamped), all in flight
        if constexpr (SLAB) v[u] = gn_slab_chunk(sl, (size_t)b * HW + min(pl + PLF * u, HW - 1), b, C, g * cg + c * 8);
        else v[u] = ldraw<X32>(src.p, xb + (size_t)min(pl + PLF * u, HW - 1) * src.cs).widen();
    }
    const int wave = threadIdx.x >> 6, nw = ((int)blockDim.x + 63) >> 6;
    const float n = (float)HW * (float)cg;
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < GN_FU; ++u)
        if (act && pl + PLF * u < HW) {
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[u].get(j);
        }
    s = wave_sum_dpp(s);
    if ((threadIdx.x & 63) == 0) s_red[0][wave] = s;
    __syncthreads();
    float ss = 0.f;
    for (int w = 0; w < nw; ++w) ss += s_red[0][w];
    const float mean = ss / n;
    float q = 0.f;
#pragma unroll
    for (int u = 0; u < GN_FU; ++u)
        if (act && pl + PLF * u < HW) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float d = v[u].get(j) - mean; q += d * d; }
        }
    q = wave_sum_dpp(q);
    if ((threadIdx.x & 63) == 0) s_red[1][wave] = q;
    __syncthreads();
    float qq = 0.f;
    for (int w = 0; w < nw; ++w) qq += s_red[1][w];
    const float2 m = make_float2(mean, rsqrtf(qq / n + eps));
    float sa[8], sh[8];
    gn_scale_shift([&](int) { return m; }, ga, be, sa, sh);
#pragma unroll
    for (int u = 0; u < GN_FU; ++u) {
        const int p = pl + PLF * u;
        if (act && p < HW) gn_store(v[u], sa, sh, silu, yb + (size_t)p * C);
    }
}

// what every GroupNorm launcher requires of a shape
static bool gn_shape_ok(int B, int HW, int C, int groups)
{
    return B > 0 && HW > 0 && groups > 0 && C % 8 == 0 && C % groups == 0 && groups <= GN_MAX_GROUPS && C <= GN_MAX_C && 256 % groups == 0 &&
           (256 / groups & (256 / groups - 1)) == 0;
}
// pixel lanes of the one-kernel form when the shape takes it (a group's channels are whole chunks and a (sample, group) slab fits
// a workgroup's registers), else 0: the two-pass form
static int gn_one_kernel_lanes(int HW, int C, int groups)
{
    static const int fuse = ctx_env_int("CTX_GN_FUSED", 1);
    const int cg = C / groups, cpg = cg / 8;
    const int plf = cg % 8 == 0 ? GN_FT / cpg : 0;
    return (fuse && plf > 0 && cpg <= GN_FT && (HW + plf - 1) / plf <= GN_FU) ? plf : 0;
}
// The launch plan: every number the GroupNorm launchers derive from a shape, in one place.  ctx_groupnorm_any launches exactly what
// gn_plan returns, and ctx_groupnorm_plan hands the same struct to the tests (tests/test_norm_cpu.py sweeps the accepted envelope).
//   one      1: the one-kernel form, grid (groups, B), `thr` threads = cpg chunk columns x `plf` pixel lanes rounded up to whole waves
//            0: the two-pass form.  Pass 1: grid (NS, B), `threads` = C/8 chunk columns x `PL` pixel lanes rounded up to whole waves
//               (a block of fewer than 8 threads would leave the fold without one whole 8-lane group), `lds` dynamic bytes
//               = (PL + na) * C * 2 floats, at most GN_LDS_OPTIN, which the launcher opts into.
//   apl, athreads, nb: pass 2 (also ctx_groupnorm_apply's): grid (nb, B), athreads = C/8 columns x apl pixel lanes in 256 .. 512 (the
//            fold of the partials uses the first 256), GN_AU pixels per lane.
struct GnPlan { int one, plf, thr, PL, threads, NS, na, lds, apl, athreads, nb; };
#define GN_LDS_OPTIN (96 * 1024)
static void gn_plan_apply(int HW, int C, GnPlan &p)
{
    const int c8n = C / 8;
    p.apl = (256 + c8n - 1) / c8n;
    p.athreads = c8n * p.apl;
    p.nb = (HW + p.apl * GN_AU - 1) / (p.apl * GN_AU);
}
// two != 0: two sources, the first Ca channels wide
static int gn_plan(int B, int HW, int C, int groups, int x32, int two, int Ca, GnPlan &p)
{
    p = GnPlan{};
    CTX_REQUIRE(gn_shape_ok(B, HW, C, groups), "groupnorm: unsupported B=%d HW=%d C=%d groups=%d", B, HW, C, groups);
    CTX_REQUIRE(!two || (Ca > 0 && Ca < C && Ca % 8 == 0), "groupnorm: two sources need 0 < Ca < C in whole 8-channel columns (Ca=%d C=%d)", Ca, C);
    gn_plan_apply(HW, C, p);
    if (const int plf = gn_one_kernel_lanes(HW, C, groups); plf) {      // either source count: the bits must not depend on it
        p.one = 1;
        p.plf = plf;
        p.thr = (C / groups / 8 * plf + 63) / 64 * 64;
        return CTX_OK;
    }
    const int c8n = C / 8;
    p.PL = min(max(1024 / c8n, 1), HW);                       // pixel lanes: ~1000 threads per block
    p.threads = (c8n * p.PL + 63) / 64 * 64;
    p.NS = min(GN_MAX_SPLITS, max(1, HW / p.PL));             // >= one pixel per lane per split
    {
        // Fat splits: a block's fold (two barriers, LDS walks, a shuffle tree) costs the same whatever it summed, and every apply block
        // re-reads all NS partials of its sample — but a 150 MB VAE tensor at batch 1 still needs all 128 of them to fill the chip.
        // ~384 KB of the sample per split, at least 64 stats blocks in all (measured, GroupNorm per evaluation: UNet batch 12 3.30 ms at
        // 128 splits / 2.13 at 16; batch 2 1.01 / 0.94 at 32; the VAE decoder's at 768^2 1.36 ms at 128 / 1.71 at 48).  CTX_GN_NS overrides.
        static const int ns_env = ctx_env_int("CTX_GN_NS", 0);
        const int64_t sample_bytes = (int64_t)HW * C * (x32 ? 4 : 2);
        const int by_size = (int)min((int64_t)GN_MAX_SPLITS, sample_bytes / (384 * 1024));
        const int want = ns_env > 0 ? ns_env : max(16, max(by_size, (64 + B - 1) / B));
        p.NS = min(p.NS, want);
    }
    p.na = max(1, p.threads / C);                             // k_gn_stats derives the same from blockDim.x
    p.lds = (p.PL + p.na) * C * 2 * (int)sizeof(float);
    CTX_REQUIRE(p.lds <= GN_LDS_OPTIN, "groupnorm: C=%d needs %d bytes of LDS", C, p.lds);
    return CTX_OK;
}

extern "C" int32_t ctx_groupnorm_plan(int32_t B, int32_t HW, int32_t C, int32_t groups, int32_t x32, int32_t Ca, int32_t *out)
{
    CTX_REQUIRE(out, "groupnorm plan: null pointer");
    GnPlan p;
    if (const int rc = gn_plan(B, HW, C, groups, x32, Ca != 0, Ca, p); rc != CTX_OK) return rc;
    const int v[12] = {p.one, p.plf, p.thr, p.PL, p.threads, p.NS, p.na, p.lds, p.apl, p.athreads, p.nb, GN_LDS_OPTIN};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
    return CTX_OK;
}

// pass 2 on NS partials per (sample, group): fat blocks (the per-block fold of the split partials is amortised), at least one batch each
static void gn_launch_apply(const GnPlan &p, const void *x, int x32, const void *x2, int Ca, const float *part, int NS, int piv, const void *gamma,
                            const void *beta, int B, int HW, int C, int groups, float eps, int silu, void *y, hipStream_t stream)
{
    CTX_BOOL_GO(x32, X, hipLaunchKernelGGL(k_gn_apply<X>, dim3(p.nb, B), dim3(p.athreads), 0, stream, x, x2, Ca, part, (const f16 *)gamma, (const f16 *)beta,
                                           HW, C, groups, NS, p.apl, piv, eps, silu, (f16 *)y));
}

extern "C" int64_t ctx_groupnorm_ws_bytes(int32_t B, int32_t groups)
{
    return ((int64_t)B * GN_MAX_SPLITS * groups * 2 + (int64_t)B * 2 * GN_MAX_C) * 4;
}

extern "C" int32_t ctx_groupnorm_f16(const void *x, const void *gamma, const void *beta, int32_t B, int32_t HW, int32_t C,
                                     int32_t groups, float eps, int32_t silu, void *y, void *stats_ws, ctx_stream_t stream)
{
    return ctx_groupnorm_any(x, 0, gamma, beta, B, HW, C, groups, eps, silu, y, stats_ws, (hipStream_t)stream);
}

// test seam of the fp32-input kernels (the engines reach them through the fp32 residual stream): x [B, HW, C] fp32
extern "C" int32_t ctx_groupnorm_f32in_f16(const float *x, const void *gamma, const void *beta, int32_t B, int32_t HW, int32_t C,
                                           int32_t groups, float eps, int32_t silu, void *y, void *stats_ws, ctx_stream_t stream)
{
    return ctx_groupnorm_any(x, 1, gamma, beta, B, HW, C, groups, eps, silu, y, stats_ws, (hipStream_t)stream);
}

// GroupNorm(+SiLU) of the channel concatenation [xa ; xb] read in place: xa [B, HW, Ca], xb [B, HW, C - Ca]; y [B, HW, C].
// Bit-identical to ctx_groupnorm_f16 of the materialised concat.
extern "C" int32_t ctx_groupnorm2_f16(const void *xa, const void *xb, int32_t Ca, const void *gamma, const void *beta, int32_t B, int32_t HW,
                                      int32_t C, int32_t groups, float eps, int32_t silu, void *y, void *stats_ws, ctx_stream_t stream)
{
    CTX_REQUIRE(xb, "groupnorm2: null pointer");
    return ctx_groupnorm_any(xa, 0, gamma, beta, B, HW, C, groups, eps, silu, y, stats_ws, (hipStream_t)stream, xb, Ca);
}

extern "C" int32_t ctx_groupnorm_apply_f16(const void *x, const void *part, int32_t slots, const void *gamma, const void *beta, int32_t B, int32_t HW,
                                           int32_t C, int32_t groups, float eps, int32_t silu, void *y, ctx_stream_t stream)
{
    return ctx_groupnorm_apply(x, (const float *)part, slots, gamma, beta, B, HW, C, groups, eps, silu, y, (hipStream_t)stream);
}

extern "C" int32_t ctx_groupnorm_slabs_f16(const void *part, int32_t splitk, const void *bias, const void *bias2, const void *rowbias, int32_t ldrb,
                                           const void *gamma, const void *beta, int32_t B, int32_t HW, int32_t C, int32_t groups, float eps,
                                           int32_t silu, void *y, ctx_stream_t stream)
{
    const GnSlabs sl = {(const float *)part, splitk, (size_t)B * HW * C, (const f16 *)bias, (const f16 *)bias2, (const f16 *)rowbias, ldrb};
    return ctx_groupnorm_slabs(sl, gamma, beta, B, HW, C, groups, eps, silu, y, (hipStream_t)stream);
}

// x32 != 0: the input is the fp32 residual stream (the output stays fp16: it is the next GEMM's operand)
int ctx_groupnorm_any(const void *x, int x32, const void *gamma, const void *beta, int B, int HW, int C, int groups, float eps, int silu,
                      void *y, void *stats_ws, hipStream_t stream, const void *x2, int Ca)
{
    CTX_REQUIRE(x && gamma && beta && y && stats_ws, "groupnorm: null pointer");
    GnPlan p;
    if (const int rc = gn_plan(B, HW, C, groups, x32, x2 != nullptr, Ca, p); rc != CTX_OK) return rc;
    if (p.one) {
        CTX_BOOL_GO(x32, X, hipLaunchKernelGGL(k_gn_fused<X>, dim3(groups, B), dim3(p.thr), 0, stream, x, x2, Ca, (const f16 *)gamma, (const f16 *)beta, HW, C,
                                               groups, p.plf, eps, silu, (f16 *)y, GnSlabs{}));
        CTX_CHECK_LAUNCH("groupnorm");
        return CTX_OK;
    }
    float *part = (float *)stats_ws;
    static bool attr = false;                                 // more than 64 KiB of dynamic LDS (C > 2048) needs the opt-in
    if (!attr) {
        hipError_t e = hipFuncSetAttribute((const void *)k_gn_stats<false>, hipFuncAttributeMaxDynamicSharedMemorySize, GN_LDS_OPTIN);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_gn_stats<true>, hipFuncAttributeMaxDynamicSharedMemorySize, GN_LDS_OPTIN);
        if (e != hipSuccess) {
            ctx_set_error("groupnorm: the LDS opt-in failed: %s", hipGetErrorString(e));
            return CTX_E_LAUNCH;
        }
        attr = true;
    }
    CTX_BOOL_GO(x32, X, hipLaunchKernelGGL(k_gn_stats<X>, dim3(p.NS, B), dim3(p.threads), (size_t)p.lds, stream, x, x2, Ca, HW, C, groups, p.NS, p.PL, part));
    gn_launch_apply(p, x, x32, x2, Ca, part, p.NS, 1, gamma, beta, B, HW, C, groups, eps, silu, y, stream);
    CTX_CHECK_LAUNCH("groupnorm");
    return CTX_OK;
}

int ctx_groupnorm_two_pass(int HW, int C, int groups) { return gn_one_kernel_lanes(HW, C, groups) == 0; }

// The apply half alone, on partials somebody else wrote (a GEMM / convolution epilogue or the split-K reduce: GemmArgs::gn_part):
// part[B][NS][groups][2], every slot of it written.
int ctx_groupnorm_apply(const void *x, const float *part, int NS, const void *gamma, const void *beta, int B, int HW, int C, int groups, float eps,
                        int silu, void *y, hipStream_t stream)
{
    CTX_REQUIRE(x && part && gamma && beta && y, "groupnorm apply: null pointer");
    CTX_REQUIRE(gn_shape_ok(B, HW, C, groups) && NS >= 1 && NS <= GN_MAX_SPLITS, "groupnorm apply: unsupported B=%d HW=%d C=%d groups=%d NS=%d", B, HW, C, groups, NS);
    GnPlan p{};
    gn_plan_apply(HW, C, p);
    gn_launch_apply(p, x, 0, nullptr, 0, part, NS, 0, gamma, beta, B, HW, C, groups, eps, silu, y, stream);
    CTX_CHECK_LAUNCH("groupnorm apply");
    return CTX_OK;
}

// One-kernel GroupNorm(+SiLU) of a split-K convolution's unreduced slabs (k_gn_fused's slab source); the shape must take the one-kernel form.
int ctx_groupnorm_slabs(const GnSlabs &sl, const void *gamma, const void *beta, int B, int HW, int C, int groups, float eps, int silu, void *y,
                        hipStream_t stream)
{
    CTX_REQUIRE(sl.part && sl.S >= 1 && gamma && beta && y, "groupnorm slabs: bad arguments");
    const int plf = gn_shape_ok(B, HW, C, groups) ? gn_one_kernel_lanes(HW, C, groups) : 0;
    CTX_REQUIRE(plf > 0 && (!sl.rowbias || sl.ldrb % 8 == 0), "groupnorm slabs: B=%d HW=%d C=%d groups=%d does not take the one-kernel form", B, HW, C, groups);
    const int thr = (C / groups / 8 * plf + 63) / 64 * 64;
    hipLaunchKernelGGL((k_gn_fused<false, true>), dim3(groups, B), dim3(thr), 0, stream, (const void *)nullptr, (const void *)nullptr, 0, (const f16 *)gamma,
                       (const f16 *)beta, HW, C, groups, plf, eps, silu, (f16 *)y, sl);
    CTX_CHECK_LAUNCH("groupnorm slabs");
    return CTX_OK;
}

// GroupNorm(+SiLU) backward, input gradient only (the VAE encoder's backward: the VAE is frozen): two reductions (statistics of
// x, then sum(du) and sum(du x^)) and one apply pass, all deterministic (fixed-order partial sums).
#define GNB_MAX_SPLITS 128

// MODE 0: per-group partial (sum (x - pivot), sum (x - pivot)^2) about the group's pivot (gn_pivot); MODE 1: partial (sum du, sum du x^) with du = dy silu'(u) gamma, u = gamma x^ + beta
// du = dy silu'(u) gamma for one element (u: the GroupNorm output before the SiLU)
__device__ __forceinline__ float gnb_du(float dy, float u, float gamma, int silu)
{
    if (silu) { const float sg = 1.0f / (1.0f + __expf(-u)); dy *= sg * (1.0f + u * (1.0f - sg)); }
    return dy * gamma;
}
template <int MODE>
__global__ __launch_bounds__(256) void k_gnb_reduce(const f16 *__restrict__ x, const f16 *__restrict__ dy, const f16 *__restrict__ gamma,
                                                    const f16 *__restrict__ beta, const float *__restrict__ mr, int HW, int C, int G, int NS,
                                                    int silu, float *__restrict__ part)
{
    extern __shared__ float sm[];                    // [PL][C][2] then [C][2]
    const int c8n = C / 8, PL = 256 / c8n;
    const int b = blockIdx.y, sp = blockIdx.x;
    const int c8 = threadIdx.x % c8n, pl = threadIdx.x / c8n;
    const int per = (HW + NS - 1) / NS, p0 = sp * per, p1 = min(HW, p0 + per), cg = C / G;
    float s[8], q[8], a[8], b0[8], ga[8], mu[8], rs[8], pv[8];
    if (MODE == 0) gn_pivots<false>(x, nullptr, 0, C, HW, b, c8 * 8, cg, pv);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        s[j] = 0.f; q[j] = 0.f;
        if (MODE == 1) {
            const int c = c8 * 8 + j, g = c / cg;
            mu[j] = mr[((size_t)b * G + g) * 2]; rs[j] = mr[((size_t)b * G + g) * 2 + 1];
            ga[j] = (float)gamma[c]; a[j] = rs[j] * ga[j]; b0[j] = (float)beta[c] - mu[j] * a[j];
        }
    }
    if (pl < PL)
        for (int p = p0 + pl; p < p1; p += PL) {
            const size_t off = ((size_t)b * HW + p) * C + c8 * 8;
            const f16x8 xv = *(const f16x8 *)(x + off);
            if (MODE == 0) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { float f = (float)xv[j] - pv[j]; s[j] += f; q[j] += f * f; }
            } else {
                const f16x8 dv = *(const f16x8 *)(dy + off);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float xf = (float)xv[j], du = gnb_du((float)dv[j], xf * a[j] + b0[j], ga[j], silu);
                    s[j] += du; q[j] += du * ((xf - mu[j]) * rs[j]);
                }
            }
        }
    if (pl < PL) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { sm[((size_t)pl * C + c8 * 8 + j) * 2] = s[j]; sm[((size_t)pl * C + c8 * 8 + j) * 2 + 1] = q[j]; }
    }
    __syncthreads();
    float *ch = sm + (size_t)PL * C * 2;
    for (int c = threadIdx.x; c < C; c += 256) {
        float ss = 0.f, qq = 0.f;
        for (int l = 0; l < PL; ++l) { ss += sm[((size_t)l * C + c) * 2]; qq += sm[((size_t)l * C + c) * 2 + 1]; }
        ch[c * 2] = ss; ch[c * 2 + 1] = qq;
    }
    __syncthreads();
    for (int g = threadIdx.x; g < G; g += 256) {
        float ss = 0.f, qq = 0.f;
        for (int c = g * cg; c < (g + 1) * cg; ++c) { ss += ch[c * 2]; qq += ch[c * 2 + 1]; }
        part[(((size_t)b * NS + sp) * G + g) * 2] = ss; part[(((size_t)b * NS + sp) * G + g) * 2 + 1] = qq;
    }
}
// MODE 0 -> (mean, rstd), the pivot of x's group added back; MODE 1 -> (sum du / n, sum du x^ / n)
template <int MODE>
__global__ void k_gnb_finalize(const float *__restrict__ part, const f16 *__restrict__ x, int HW, int C, int G, int NS, float n, float eps,
                               float *__restrict__ out)
{
    const int b = blockIdx.x;
    for (int g = threadIdx.x; g < G; g += blockDim.x) {
        float ss = 0.f, qq = 0.f;
        for (int k = 0; k < NS; ++k) { ss += part[(((size_t)b * NS + k) * G + g) * 2]; qq += part[(((size_t)b * NS + k) * G + g) * 2 + 1]; }
        if (MODE == 0) {
            const float2 m = gn_mean_rstd(ss, qq, n, eps, gn_pivot<false>(x, nullptr, 0, C, HW, b, g * (C / G)));
            out[((size_t)b * G + g) * 2] = m.x; out[((size_t)b * G + g) * 2 + 1] = m.y;
        } else { out[((size_t)b * G + g) * 2] = ss / n; out[((size_t)b * G + g) * 2 + 1] = qq / n; }
    }
}
// dx = rstd (du - c1 - x^ c2) (+ add)
__global__ __launch_bounds__(256) void k_gnb_apply(const f16 *__restrict__ x, const f16 *__restrict__ dy, const f16 *__restrict__ gamma,
                                                   const f16 *__restrict__ beta, const float *__restrict__ mr, const float *__restrict__ cc,
                                                   const f16 *__restrict__ add, int HW, int C, int G, int silu, f16 *__restrict__ dx)
{
    const int b = blockIdx.y, c8n = C / 8, cg = C / G;
    const size_t total = (size_t)HW * c8n;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c0 = (int)(i % c8n) * 8;
        const size_t off = (size_t)b * HW * C + i * 8;
        const f16x8 xv = *(const f16x8 *)(x + off), dv = *(const f16x8 *)(dy + off);
        f16x8 av = {0, 0, 0, 0, 0, 0, 0, 0};
        if (add) av = *(const f16x8 *)(add + off);
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = c0 + j, g = c / cg;
            const float mu = mr[((size_t)b * G + g) * 2], rs = mr[((size_t)b * G + g) * 2 + 1];
            const float c1 = cc[((size_t)b * G + g) * 2], c2 = cc[((size_t)b * G + g) * 2 + 1];
            const float ga = (float)gamma[c], xh = ((float)xv[j] - mu) * rs, u = xh * ga + (float)beta[c];
            o[j] = (f16)(rs * (gnb_du((float)dv[j], u, ga, silu) - c1 - xh * c2) + (float)av[j]);
        }
        *(f16x8 *)(dx + off) = o;
    }
}

extern "C" int64_t ctx_groupnorm_bwd_ws_bytes(int32_t B, int32_t groups)
{
    return ((int64_t)B * GNB_MAX_SPLITS * groups * 2 + (int64_t)B * groups * 4) * 4;
}

// dx = d(loss)/dx (+ add) of y = GroupNorm(x) (SiLU after it when `silu`), fp16 NHWC; ws: ctx_groupnorm_bwd_ws_bytes(B, groups)
extern "C" int32_t ctx_groupnorm_bwd_f16(const void *xv, const void *dyv, const void *gammav, const void *betav, const void *addv, int32_t B,
                                         int32_t HW, int32_t C, int32_t groups, float eps, int32_t silu, void *dxv, void *ws, ctx_stream_t stream)
{
    const f16 *x = (const f16 *)xv, *dy = (const f16 *)dyv, *gamma = (const f16 *)gammav, *beta = (const f16 *)betav, *add = (const f16 *)addv;
    f16 *dx = (f16 *)dxv;
    hipStream_t s = (hipStream_t)stream;
    CTX_REQUIRE(x && dy && gamma && beta && dx && ws, "groupnorm backward: null pointer");
    CTX_REQUIRE(B > 0 && HW > 0 && C >= 8 && groups > 0, "groupnorm backward: B=%d HW=%d C=%d groups=%d", B, HW, C, groups);
    const int G = groups, c8n = C / 8;
    CTX_REQUIRE(C % 8 == 0 && 256 % c8n == 0 && C % G == 0, "groupnorm backward: C=%d groups=%d is outside the kernel's envelope", C, G);
    const int PL = 256 / c8n;
    int NS = HW / (PL * 4); if (NS < 1) NS = 1; if (NS > GNB_MAX_SPLITS) NS = GNB_MAX_SPLITS;
    float *part = (float *)ws, *mr = part + (size_t)B * GNB_MAX_SPLITS * G * 2, *cc = mr + (size_t)B * G * 2;
    const size_t lds = ((size_t)PL * C * 2 + (size_t)C * 2) * sizeof(float);
    const float n = (float)HW * (float)(C / G);
    hipLaunchKernelGGL(k_gnb_reduce<0>, dim3(NS, B), dim3(256), lds, s, x, (const f16 *)nullptr, gamma, beta, (const float *)nullptr, HW, C, G, NS, silu, part);
    hipLaunchKernelGGL(k_gnb_finalize<0>, dim3(B), dim3(64), 0, s, part, x, HW, C, G, NS, n, eps, mr);
    hipLaunchKernelGGL(k_gnb_reduce<1>, dim3(NS, B), dim3(256), lds, s, x, dy, gamma, beta, mr, HW, C, G, NS, silu, part);
    hipLaunchKernelGGL(k_gnb_finalize<1>, dim3(B), dim3(64), 0, s, part, x, HW, C, G, NS, n, 0.f, cc);
    hipLaunchKernelGGL(k_gnb_apply, dim3(capped_blocks((int64_t)HW * c8n, 256, 2048), B), dim3(256), 0, s, x, dy, gamma, beta, mr, cc, add, HW, C, G, silu, dx);
    CTX_CHECK_LAUNCH("groupnorm backward");
    return CTX_OK;
}

// ------------------------------------------------------------------------------------------------
// LayerNorm over the last dim: one wave per LN_R rows at a time, up to 4 x 16-byte chunks per lane per row
// (C <= 2048); all LN_R rows' loads are issued before the first reduction.
// one element of a row, rounded once
__device__ __forceinline__ f16 ln_norm(float x, float mean, float rstd, f16 ga, f16 be) { return (f16)((x - mean) * rstd * (float)ga + (float)be); }
template <int KC, int R, bool X32>
__global__ __launch_bounds__(256) void k_layernorm(const void *__restrict__ x, const f16 *__restrict__ gamma,
                                                   const f16 *__restrict__ beta, int64_t rows, int C, float eps,
                                                   f16 *__restrict__ y)
{
    const int lane = threadIdx.x & 63;
    const int c8n = C / 8;
    const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int64_t row0 = wave * R;
    if (row0 >= rows) return;
    Wide8 v[R][KC];
#pragma unroll
    for (int rr = 0; rr < R; ++rr)
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            int c8 = lane + 64 * k;
            const int64_t rw = row0 + rr < rows ? row0 + rr : rows - 1;
            v[rr][k] = ldraw<X32>(x, (size_t)(rw * C + min(c8, c8n - 1) * 8)).widen();          // unconditional load, masked below
            if (c8 >= c8n) v[rr][k] = Wide8{};
        }
    f16x8 ga[KC], be[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        int c8 = lane + 64 * k;
        ga[k] = *(const f16x8 *)(gamma + min(c8, c8n - 1) * 8);
        be[k] = *(const f16x8 *)(beta + min(c8, c8n - 1) * 8);
    }
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
        if (row0 + rr >= rows) break;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < KC; ++k)
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[rr][k].get(j);                 // padded lanes hold zeros
        float mean = wave_sum_dpp(s) / (float)C;
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            int c8 = lane + 64 * k;
            if (c8 < c8n) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { float d = v[rr][k].get(j) - mean; q += d * d; }
            }
        }
        float rstd = rsqrtf(wave_sum_dpp(q) / (float)C + eps);
        f16 *yr = y + (row0 + rr) * C;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            int c8 = lane + 64 * k;
            if (c8 < c8n) {
                f16x8 o;
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = ln_norm(v[rr][k].get(j), mean, rstd, ga[k][j], be[k][j]);
                *(f16x8 *)(yr + c8 * 8) = o;
            }
        }
    }
}

// 8 lanes per row, KC 16-byte chunks per lane (C = 64 KC): every lane of the wave carries data (the one-wave-per-row form above leaves
// 24 of 64 lanes idle at C = 320 and 640), a lane's chunks k*8 + s make 128-byte runs with its 7 neighbours, and a wave keeps 8 rows x KC
// loads in flight.  The 8-lane sums are three DPP adds (sum8_dpp); same two-pass mean / variance and the same
// rounding points as k_layernorm, another summation order.
template <int KC>
__global__ __launch_bounds__(256) void k_layernorm_g8(const f16 *__restrict__ x, const f16 *__restrict__ gamma, const f16 *__restrict__ beta,
                                                      int64_t rows, float eps, f16 *__restrict__ y)
{
    constexpr int C = 64 * KC;
    const int lane = threadIdx.x & 63, s = lane & 7, rw = lane >> 3;
    const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int64_t row = wave * 8 + rw;
    const bool live = row < rows;                                   // uniform over the row's 8 lanes
    const f16 *xr = x + (live ? row : rows - 1) * C + s * 8;
    Raw8<false> v[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) v[k] = ldraw<false>(xr, k * 64);
    f16x8 ga[KC], be[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        ga[k] = *(const f16x8 *)(gamma + k * 64 + s * 8);
        be[k] = *(const f16x8 *)(beta + k * 64 + s * 8);
    }
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < KC; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) sum += v[k].get(j);
    const float mean = sum8_dpp(sum) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < KC; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float d = v[k].get(j) - mean; q += d * d; }
    const float rstd = rsqrtf(sum8_dpp(q) / (float)C + eps);
    if (!live) return;
    f16 *yr = y + row * C + s * 8;
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = ln_norm(v[k].get(j), mean, rstd, ga[k][j], be[k][j]);
        *(f16x8 *)(yr + k * 64) = o;
    }
}

extern "C" int32_t ctx_layernorm_f16(const void *x, const void *gamma, const void *beta, int64_t rows, int32_t C, float eps,
                                     void *y, ctx_stream_t stream)
{
    return ctx_layernorm_any(x, 0, gamma, beta, rows, C, eps, y, (hipStream_t)stream);
}

// test seam of the fp32-input kernels: x [rows, C] fp32
extern "C" int32_t ctx_layernorm_f32in_f16(const float *x, const void *gamma, const void *beta, int64_t rows, int32_t C, float eps,
                                           void *y, ctx_stream_t stream)
{
    return ctx_layernorm_any(x, 1, gamma, beta, rows, C, eps, y, (hipStream_t)stream);
}

// The launch plan.  g8 1: k_layernorm_g8<KC>, 8 lanes per row, 32 rows per block; 0: k_layernorm<KC, R>, a wave per R rows, 4 waves per block
struct LnPlan { int g8, KC, R; int64_t blocks; };
static int ln_plan(int64_t rows, int C, int x32, LnPlan &p)
{
    p = LnPlan{};
    CTX_REQUIRE(rows > 0 && C > 0 && C % 8 == 0 && C <= 2048, "layernorm: unsupported rows=%lld C=%d", (long long)rows, C);
    // fp16 input, C a multiple of 64 up to 640 (beyond that the one-wave-per-row form fills >= 83 % of its lanes and gamma / beta for 20
    // chunks per lane would not fit the registers): 8 lanes per row (CTX_LN_G8=0: the one-wave-per-row kernels)
    static const int g8 = ctx_env_int("CTX_LN_G8", 1);
    if (g8 && !x32 && C % 64 == 0 && C <= 640 && rows >= 64) {
        p.g8 = 1; p.KC = C / 64; p.R = 8;
        p.blocks = cdiv64(cdiv64(rows, 8), 4);
        return CTX_OK;
    }
    p.KC = (C / 8 + 63) / 64;                                 // 16-byte chunks per lane per row
    // rows per wave: ~4 loads in flight per lane, but keep >= ~2 waves per SIMD of work on the chip
    p.R = rows >= 8192 ? (p.KC == 1 ? 4 : p.KC == 2 ? 2 : 1) : 1;
    p.blocks = cdiv64(cdiv64(rows, p.R), 4);
    return CTX_OK;
}

extern "C" int32_t ctx_layernorm_plan(int64_t rows, int32_t C, int32_t x32, int64_t *out)
{
    CTX_REQUIRE(out, "layernorm plan: null pointer");
    LnPlan p;
    if (const int rc = ln_plan(rows, C, x32, p); rc != CTX_OK) return rc;
    out[0] = p.g8; out[1] = p.KC; out[2] = p.R; out[3] = p.blocks;
    return CTX_OK;
}

int ctx_layernorm_any(const void *x, int x32, const void *gamma, const void *beta, int64_t rows, int C, float eps, void *y, hipStream_t stream)
{
    CTX_REQUIRE(x && gamma && beta && y, "layernorm: null pointer");
    LnPlan p;
    if (const int rc = ln_plan(rows, C, x32, p); rc != CTX_OK) return rc;
    const unsigned nb = (unsigned)p.blocks;
    if (p.g8) {
#define LN_G8(KC_) case KC_: hipLaunchKernelGGL(k_layernorm_g8<KC_>, dim3(nb), dim3(256), 0, stream, (const f16 *)x, (const f16 *)gamma, (const f16 *)beta, rows, eps, (f16 *)y); break
        switch (p.KC) {
            LN_G8(1); LN_G8(2); LN_G8(3); LN_G8(4); LN_G8(5); LN_G8(6); LN_G8(7); LN_G8(8); LN_G8(9); LN_G8(10);
        }
#undef LN_G8
        CTX_CHECK_LAUNCH("layernorm");
        return CTX_OK;
    }
#define LN_GO(KC_, R_) CTX_BOOL_GO(x32, X, hipLaunchKernelGGL((k_layernorm<KC_, R_, X>), dim3(nb), dim3(256), 0, stream, x, \
                                                          (const f16 *)gamma, (const f16 *)beta, rows, C, eps, (f16 *)y))
    switch (p.KC * 8 + p.R) {
        case 1 * 8 + 4: LN_GO(1, 4); break;
        case 1 * 8 + 1: LN_GO(1, 1); break;
        case 2 * 8 + 2: LN_GO(2, 2); break;
        case 2 * 8 + 1: LN_GO(2, 1); break;
        case 3 * 8 + 1: LN_GO(3, 1); break;
        default: LN_GO(4, 1); break;
    }
#undef LN_GO
    CTX_CHECK_LAUNCH("layernorm");
    return CTX_OK;
}
