// Building blocks shared by the MFMA GEMM / convolution kernels (gemm.hip, gemm8.hip, gemm144.hip, conv_halo.hip) and, for the
// staging primitives and the host launch, attention.hip.  Device helpers are __forceinline__: a kernel that uses one compiles to
// the code it had when the helper was written out in place.  Each kernel keeps its own K loop, accumulator walk, LDS layout and
// bias preloading; what lives here is what must stay the same in all of them.
#pragma once
#include "common.h"
#include "kernels.h"
#include <hip/hip_ext.h>
#include <stdlib.h>

// ---- staging -------------------------------------------------------------------------------------------------------
// global_load_lds operands, and the page that out-of-range rows and convolution padding are fetched from (with step 0).
// `inline`, not `static`: a static device variable is made visible to the host, and every kernel then reads its address from the
// GOT instead of forming it pc-relative (an s_load and a wait in each kernel's prologue, and another register allocation).
typedef const __attribute__((address_space(1))) void *gptr_t;
typedef __attribute__((address_space(3))) void *lptr_t;
inline __device__ __attribute__((aligned(128))) f16 ctx_zero_page[64];

// 1-D grid cut into 8 contiguous runs, one per XCD (blocks b and b + 8 share an L2)
__device__ __forceinline__ int xcd_remap(int bid, int nwg)
{
    int q = nwg >> 3, r = nwg & 7, x = bid & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
}

// ---- tile decode ---------------------------------------------------------------------------------------------------
// Grid of tiles x K-slices, slice-major.  Inside a slice the tile order walks the operand that is re-read most (mfast:
// consecutive blocks share the weight panel; else the activation panel).  m0 / n0: origin of the bm x bn tile; kbeg / nk: this
// slice's K stages of `pkt` elements.
struct GemmTile { int slice, tile_m, tile_n, m0, n0, kbeg, nk; };
__device__ __forceinline__ GemmTile gemm_tile(const GemmArgs &a, int block, int pkt, int bm, int bn)
{
    const int ntiles = a.ntm * a.ntn;
    const int lin = xcd_remap(block, ntiles * a.splitk);
    GemmTile t;
    t.slice = lin / ntiles;
    const int bid = lin - t.slice * ntiles;
    t.tile_n = a.mfast ? bid / a.ntm : bid % a.ntn;
    t.tile_m = a.mfast ? bid % a.ntm : bid / a.ntn;
    t.m0 = t.tile_m * bm; t.n0 = t.tile_n * bn;
    const int nk_all = a.K / pkt;
    t.kbeg = (int)((long)nk_all * t.slice / a.splitk);
    t.nk = (int)((long)nk_all * (t.slice + 1) / a.splitk) - t.kbeg;
    return t;
}

// ---- im2col (NHWC, 3x3) --------------------------------------------------------------------------------------------
// output pixel m -> its input coordinate before the tap shift (oy, ox) and the offset of its image in X, plus the lane's chunk lc
__device__ __forceinline__ void conv_pixel(const GemmArgs &a, int m, int lc, int &oy, int &ox, int &off)
{
    const int hw = a.Ho * a.Wo;
    const int b = m / hw, p = m - b * hw;
    const int y = p / a.Wo, x = p - y * a.Wo;
    off = b * a.H * a.W * a.Cin + lc;
    oy = y * a.stride; ox = x * a.stride;
}
// the tap that K index k0 falls in: shift (with poff), first channel, and the extent of the (upsampled) input grid
struct ConvTap { int dy, dx, c0, Hv, Wv; };
__device__ __forceinline__ ConvTap conv_tap(const GemmArgs &a, int k0)
{
    const int tap = k0 / a.Cin;
    return {tap / 3 - 1 + a.poff, tap % 3 - 1 + a.poff, k0 - tap * a.Cin, a.H << a.ups, a.W << a.ups};
}
// Source of one pixel for that tap; `off` as conv_pixel gives it.  ok: in, the pixel's row exists; out,
// the tap reads the image (else the zero page: padding, or with ZINS the zero-inserted odd rows / columns of a.zins).
// `cen`: a K segment's pixel pointer, read instead of the image (the caller passes the centre tap then: ok = the row exists)
template <bool ZINS = false>
__device__ __forceinline__ const f16 *conv_tap_src(const GemmArgs &a, const ConvTap &t, int oy, int ox, int off, bool &ok, const f16 *cen = nullptr)
{
    const int iy = oy + t.dy, ix = ox + t.dx;
    ok = ok && iy >= 0 && iy < t.Hv && ix >= 0 && ix < t.Wv;
    if (ZINS) ok = ok && !(a.zins && ((iy | ix) & 1));
    const f16 *src = a.X + off + (((iy >> a.ups) * a.W + (ix >> a.ups)) * a.Cin) + t.c0;
    if (cen) src = cen;
    return ok ? src : ctx_zero_page;
}

// ---- phase form (GemmArgs::phase) ----------------------------------------------------------------------------------
// The kernels see a stride-1 convolution over the source grid (Ho = H, Wo = W, ups = 0) with 4 taps per pixel, and the M dimension is
// phase-major: ntm = 4 x the tiles of one phase's B H W rows, so a tile lies in one phase, which selects its weight matrix.
// ph: phase 2a + b; m0: the tile's first row inside the phase; M: rows per phase (the last tile of each phase is masked against it)
struct ConvPhase { int ph, pa, pb, m0, M; };
__device__ __forceinline__ ConvPhase conv_phase_tile(const GemmArgs &a, int tile_m, int bm)
{
    const int ntmp = a.ntm >> 2, ph = tile_m / ntmp;
    return {ph, ph >> 1, ph & 1, (tile_m - ph * ntmp) * bm, a.M >> 2};
}
// shift of tap t = 2u + v of phase parity p along one axis: p - 1 + (u | v)
__device__ __forceinline__ int conv_phase_dy(const ConvPhase &p, int t) { return p.pa - 1 + (t >> 1); }
__device__ __forceinline__ int conv_phase_dx(const ConvPhase &p, int t) { return p.pb - 1 + (t & 1); }
// conv_tap of the phase form: K index k0 falls in tap k0 / Cin of the 4
__device__ __forceinline__ ConvTap conv_phase_tap(const GemmArgs &a, const ConvPhase &p, int k0)
{
    const int tap = k0 / a.Cin;
    return {conv_phase_dy(p, tap), conv_phase_dx(p, tap), k0 - tap * a.Cin, a.H, a.W};
}
// row m of the phase (pixel (n, i, j) of the source grid) -> the row of output pixel (n, 2i + a, 2j + b); every epilogue and the split-K
// partials store through it, so the fp32 slabs are already in the output's order and the reduce kernel does not know the form
__device__ __forceinline__ int conv_phase_row(const GemmArgs &a, const ConvPhase &p, int m)
{
    const int hw = a.H * a.W, n = m / hw, r = m - n * hw, i = r / a.W, j = r - i * a.W;
    return ((n * 2 * a.H + 2 * i + p.pa) * 2 * a.W) + 2 * j + p.pb;
}

// K segments (GemmArgs::nseg): the source that the K stage starting at k0 reads.  src 0 .. 8: that tap of the 3x3 part; 9 / 10:
// segment 0 / 1.  c0: first channel inside the source, C: the source's channel count (C - c0 is what is left of it), so a split-K
// slice may start anywhere.  Weight rows of the 3x3 part are 9 Cin long whatever K is.
struct ConvSrc { int src, c0, C; };
__device__ __forceinline__ ConvSrc conv_stage_src(const GemmArgs &a, int k0)
{
    const int k9 = 9 * a.Cin;
    if (k0 < k9) { const int tap = k0 / a.Cin; return {tap, k0 - tap * a.Cin, a.Cin}; }
    const int k1 = k0 - k9;
    if (k1 < a.segC[0]) return {9, k1, a.segC[0]};
    return {10, k1 - a.segC[0], a.segC[1]};
}
// a segment's activation / weight source for output pixel m / feature n at the segment's channel c (the lane's chunk included);
// selects, not indexing: a run-time index into the by-value argument block would put it in scratch memory
// (element offsets fit 32 bits: the dispatcher checks M segC and N segLdw).  m / n / c here are the wave-uniform part (tile origin,
// the piece's first row, the stage's first channel): scalar arithmetic; the callers add the lane's own row and chunk.
__device__ __forceinline__ const f16 *conv_seg_x(const GemmArgs &a, int s, int m, int c)
{
    return (s ? a.segX[1] : a.segX[0]) + (unsigned)(m * (s ? a.segC[1] : a.segC[0]) + c);
}
__device__ __forceinline__ const f16 *conv_seg_w(const GemmArgs &a, int s, int n, int c)
{
    return (s ? a.segW[1] : a.segW[0]) + (unsigned)(n * (s ? a.segLdw[1] : a.segLdw[0]) + c);
}
// The segment switch runs once or twice per K loop.  Its per-lane arithmetic starts from a lane id taken through an empty volatile asm,
// so that none of it is hoisted out of the loop into registers that would stay live across every stage.  The K loops' pointers get
// no second definition either (that costs registers: the allocator keeps both): an activation pointer is still assigned in one
// place per kernel, from the tap's or the segment's source, and a weight pointer walks on in place by conv_seg_wjump().
__device__ __forceinline__ int conv_seg_lane(int lane)
{
    asm volatile("" : "+v"(lane));
    return lane;
}

// Weight pointers at a segment switch walk on from where they stand: in row n of the 3x3 matrix at K index k_issue (the end of the
// 3x3 part, or a slice's start inside a segment: `fresh`) or at the end of segment 0's row; the lane's chunk is already in them.
// -> bytes between the two matrices' origins (to the segment's channel c0) and the difference of the row strides (elements):
// row n's pointer advances by jump + n * dld * sizeof(f16).
struct ConvWJump { long jump; int dld; };
__device__ __forceinline__ ConvWJump conv_seg_wjump(const GemmArgs &a, int sg, int c0, int k_issue, bool fresh)
{
    const f16 *from = fresh ? a.Wt + k_issue : a.segW[0] + a.segC[0];
    const f16 *to = (sg ? a.segW[1] : a.segW[0]) + c0;
    return {(long)((const char *)to - (const char *)from), (sg ? a.segLdw[1] : a.segLdw[0]) - (fresh ? 9 * a.Cin : a.segLdw[0])};
}

// ---- epilogue ------------------------------------------------------------------------------------------------------
// exact-GELU (erf form) with a branch-free erf: Abramowitz-Stegun 7.1.26, |abs err| <= 1.5e-7 (far below fp16 resolution)
__device__ __forceinline__ float fast_erf(float x)
{
    float ax = __builtin_fabsf(x);
    float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * ax);
    float p = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f + t * (-1.453152027f + t * 1.061405429f))));
    float e = 1.0f - p * __builtin_amdgcn_exp2f(-1.4426950408889634f * ax * ax);
    return __builtin_copysignf(e, x);
}
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + fast_erf(x * 0.70710678118654752f)); }

// registers 4g .. 4g + 3 of a 32x32 accumulator: 4 consecutive features of the lane's row
__device__ __forceinline__ f32x4 acc4(const f32x16 &c, int g) { return (f32x4){c[4 * g], c[4 * g + 1], c[4 * g + 2], c[4 * g + 3]}; }
__device__ __forceinline__ f32x4 add4(f32x4 v, f16x4 b)
{
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += (float)b[e];
    return v;
}
__device__ __forceinline__ void add8(float (&v)[8], f16x8 b)
{
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] += (float)b[e];
}

// the tile's bias for features n ..: bias (+ bias2), summed in fp32
__device__ __forceinline__ f32x4 bias4(const GemmArgs &a, f32x4 v, int n)
{
    if (a.bias) v = add4(v, *(const f16x4 *)(a.bias + n));
    if (a.bias2) v = add4(v, *(const f16x4 *)(a.bias2 + n));
    return v;
}
__device__ __forceinline__ void bias8(const GemmArgs &a, float (&v)[8], int n)
{
    if (a.bias) add8(v, *(const f16x8 *)(a.bias + n));
    if (a.bias2) add8(v, *(const f16x8 *)(a.bias2 + n));
}

// The operand order of every epilogue: accumulator, bias (+ bias2), row bias, residual, one rounding.  The bias is the caller's (some
// kernels preload it per tile, some test a.bias per piece): store4 / store8 take v = accumulator + bias and do the rest.
// F32: honour a.res32 / a.out32 (fp32 residual stream); the kernels that never see those flags do not test them.
// store4: features nn .. nn + 3 of row m, whose row bias is row bidx.  -> the fp16 values as stored (zeros behind a.out32), for the
// callers that also sum them (GroupNorm partials)
template <bool F32 = false>
__device__ __forceinline__ f16x4 store4(const GemmArgs &a, f32x4 v, size_t m, int bidx, int nn)
{
    if (a.rowbias) v = add4(v, *(const f16x4 *)(a.rowbias + (size_t)bidx * a.ldrb + nn));
    if (a.residual) {
        if (F32 && a.res32) v += *(const f32x4 *)((const float *)a.residual + m * a.ldr + nn);
        else v = add4(v, *(const f16x4 *)(a.residual + m * a.ldr + nn));
    }
    if (F32 && a.out32) {
        *(f32x4 *)((float *)a.out + m * a.ldc + nn) = v;
        return (f16x4){0, 0, 0, 0};
    }
    f16x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (f16)v[e];
    *(f16x4 *)(a.out + m * a.ldc + nn) = o;
    return o;
}
// store8: features n .. n + 7 of row m (the row walk of the LDS-staged epilogues: 16 bytes of fp16 per lane)
template <bool F32 = false>
__device__ __forceinline__ f16x8 store8(const GemmArgs &a, float (&v)[8], int m, int n)
{
    if (a.rowbias) add8(v, *(const f16x8 *)(a.rowbias + (size_t)(m / a.rows_per_batch) * a.ldrb + n));
    if (a.residual) {
        if (F32 && a.res32) {
            const float *rp = (const float *)a.residual + (size_t)m * a.ldr + n;
            f32x4 b0 = *(const f32x4 *)rp, b1 = *(const f32x4 *)(rp + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[e] += b0[e]; v[4 + e] += b1[e]; }
        } else
            add8(v, *(const f16x8 *)(a.residual + (size_t)m * a.ldr + n));
    }
    if (F32 && a.out32) {
        float *op = (float *)a.out + (size_t)m * a.ldc + n;
        *(f32x4 *)op = (f32x4){v[0], v[1], v[2], v[3]}; *(f32x4 *)(op + 4) = (f32x4){v[4], v[5], v[6], v[7]};
        return (f16x8){0, 0, 0, 0, 0, 0, 0, 0};
    }
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (f16)v[e];
    *(f16x8 *)(a.out + (size_t)m * a.ldc + n) = o;
    return o;
}
// fp32 split-K partial: features nn .. nn + 3 of a row of the slice's [M][N] slab (masked along N)
__device__ __forceinline__ void store_part4(const GemmArgs &a, float *row, int nn, f32x4 v)
{
    if (nn < a.N) *(f32x4 *)(row + nn) = v;
}
// GEGLU: value x GELU(gate), both with their bias already added, rounded once
__device__ __forceinline__ f16 geglu(float xv, float gv) { return (f16)(xv * gelu_erf(gv)); }

// ---- host ----------------------------------------------------------------------------------------------------------
// 1: the weights are the larger operand (unique bytes: weights N*K, activations M*K; conv: M*Cin, the 9 taps re-read the same pixels)
static inline int ctx_gemm_mfast(const GemmArgs &a, bool conv)
{
    // (the phase form: four weight matrices of N x K, and the B H W source pixels that its M / 4 rows per phase share)
    const double wbytes = (double)a.N * a.K * (a.phase ? 4 : 1), xbytes = (double)(a.phase ? a.M / 4 : a.M) * (conv ? a.Cin : a.K);
    return wbytes > xbytes ? 1 : 0;
}
// Launch KERN; under profiling with the start / stop events of ctx_prof_events(klass, ...).  lds > 0: dynamic LDS, whose limit is
// raised on the kernel's first launch (one flag per KERN).
template <auto KERN, class Args>
static inline void ctx_launch(int klass, dim3 grid, dim3 block, size_t lds, hipStream_t s, const Args &a)
{
    static bool attr_done = false;
    if (lds && !attr_done) {
        (void)hipFuncSetAttribute((const void *)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_done = true;
    }
    if (ctx_prof_on()) {
        hipEvent_t e0, e1;
        ctx_prof_events(klass, &e0, &e1);
        hipExtLaunchKernelGGL(KERN, grid, block, lds, s, e0, e1, 0, a);
    } else
        hipLaunchKernelGGL(KERN, grid, block, lds, s, a);
}
