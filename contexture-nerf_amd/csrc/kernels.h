// Internal (non-ABI) host entry points shared between the translation units of libctxnerf.so.
#pragma once
#include "common.h"

struct GemmArgs {
    const f16 *X;
    const f16 *Wt;
    const f16 *bias;       // [N] or null (GEGLU: packed/interleaved order)
    const f16 *rowbias;    // [M/rows_per_batch, N] or null
    const f16 *residual;   // [M, ldr] or null
    f16 *out;
    int M, N, K;
    int ldc, ldr;
    int rows_per_batch;
    int ldrb;              // row stride of rowbias
    int epi;               // 0 plain, 1 GEGLU (out has N/2 columns)
    // conv
    int H, W, Cin, Ho, Wo, stride, ups;
    int poff;              // conv input-coordinate offset: 0 = symmetric padding 1; 1 = no top/left padding (diffusers' VAE
                           // Downsample2D: F.pad(x, (0,1,0,1)) then a stride-2 conv with padding 0)
    int res32, out32;      // 1: `residual` / `out` point at fp32 tensors (the fp32 residual-stream experiment; gemm.hip epilogues only)
    int zins;              // conv: 1 = with ups, the 2x grid is ZERO-INSERTED (odd rows / columns read the zero page) instead of
                           // nearest-upsampled: the input gradient of a stride-2 convolution (poff = -1 there); gemm.hip kernel only
    int phase;             // conv: 1 = the nearest x2 upsample + 3x3 convolution as four 2x2 convolutions over the SOURCE grid, one per output
                           // parity (a, b): Wt is the phase pack [4][N][2][2][Cin] (ctx_pack_conv3_phase_f16), K = 4 Cin, M = 4 B H W rows,
                           // phase-major; tap (u, v) of phase (a, b) reads source pixel (i + a - 1 + u, j + b - 1 + v) and row (n, i, j) of
                           // the phase goes to output pixel (n, 2i + a, 2j + b).  Bias only: no row bias, residual, K segments or GroupNorm
                           // partials.  The dispatcher turns the geometry into the kernels' (Ho = H, Wo = W, ups = 0) and checks the form.
    int ntm, ntn;
    int splitk;           // >1: grid.y = splitk, fp32 partials [splitk][M][N] go to `part`
    float *part;
    int pk;                // K-stage depth chosen by the launcher (32 or 64)
    int krot;              // 1: per-workgroup K rotation (spreads concurrent accesses to shared operand rows); 2: no rotation and no
                           // steady-state K loop (CTX_GEMM_STEADY=0, the A/B switch of gemm.hip's branch-free loop)
    int tile, use8;        // plan: tile id of gemm.hip (-1 = heuristic); use8: -1 heuristic, 0 gemm.hip, 1 gemm8.hip, 2 / 3 conv_halo.hip (128 / 64 features), 4 .. 8 gemm144.hip (6 waves; 15 waves lockstep; pipelined; barrier per two stages; 288 x 160 lockstep)
    int stage_epi;         // 1: epilogue staged through LDS (whole-line stores / residual reads)
    int mfast;             // 1: consecutive workgroups walk M first (share the weight panel in their XCD's L2)
    // conv, K segments: up to two centre-tap (1x1) products behind the 9 Cin part, each over another NHWC tensor of the output's pixel
    // grid with its own weights: out += segX[s] . segW[s]^T.  K = 9 Cin + segC[0] + segC[1]; stride 1, no upsample, poff 0 only.
    int nseg;              // 0 .. 2
    const f16 *segX[2];    // [M, segC[s]]: the channel count is the pixel stride
    const f16 *segW[2];    // [N] rows of segC[s] weights, row stride segLdw[s] (two column ranges of one [N][Ca + Cb] matrix)
    int segC[2], segLdw[2];
    const f16 *bias2;      // [N] or null: a second bias (the folded product's own), added in fp32 behind `bias`
    // GroupNorm partials request (gn_part null: none).  The kernel that rounds the output (a gemm144.hip tile, or the split-K reduce)
    // also writes the (sum x, sum x^2) of the fp16 values it stores, per (sample, slot, group), in k_gn_apply's layout
    // part[b][gn_ns][N / gn_cg][2]; every slot has exactly one writer.  The launcher fills gn_ns when it accepts and clears gn_part
    // when it declines (the caller then runs k_gn_stats as before).
    float *gn_part;
    int gn_cg, gn_hw;      // channels per group; pixels per sample (M = B gn_hw)
    int gn_ns;             // out: slots per sample
    int keep_slabs;        // 1 (with splitk > 1): no reduce launch; `out` is not written and the reader sums the fp32 slabs itself, in the
                           // reduce's operand order (k_gn_fused's slab source).  The dispatch fails if the launch did not split.
};
// slots per sample a GroupNorm partials buffer holds (ctx_groupnorm_ws_bytes is sized for it)
#define CTX_GN_MAX_SLOTS 128
#define CTX_GEMM_MAX_SEG 2

// the problem of a 3x3 convolution over x [B,H,W,Cin] in the given geometry (stride, x2 grid, poff, zins): output grid, GEMM extents and
// leading dimensions.  engine_conv3 and the test seam ctx_conv3x3_geom_f16 both fill their arguments here.
static inline void ctx_conv3_problem(GemmArgs &a, int B, int H, int W, int Cin, int Cout, int stride, int ups, int poff, int zins)
{
    a.Ho = ((H << ups) - 1) / stride + 1; a.Wo = ((W << ups) - 1) / stride + 1;
    a.M = B * a.Ho * a.Wo; a.N = Cout; a.K = 9 * Cin; a.ldc = Cout; a.ldr = Cout; a.rows_per_batch = a.Ho * a.Wo;
    a.H = H; a.W = W; a.Cin = Cin; a.stride = stride; a.ups = ups; a.poff = poff; a.zins = zins;
}

// the same upsampling problem (ups 1, stride 1, poff 0, no zins) in the phase form over the pack `wp`: M and the output stay what they were
static inline void ctx_conv3_phase(GemmArgs &a, const f16 *wp)
{
    a.phase = 1; a.Wt = wp; a.K = 4 * a.Cin;
}
// 1: this upsampling convolution has a phase form (the kernels that implement it stage 64 channels at a time)
static inline int ctx_conv3_phase_ok(int Cin, int Cout, int stride, int ups, int poff, int zins)
{
    return ups == 1 && stride == 1 && poff == 0 && !zins && Cin % 64 == 0 && Cout % 8 == 0;
}
// 1: at this shape (M output pixels) the per-shape table (tools/bench_upsample_phase.py) has the phase form slower than nine taps, and the
// engines keep the nine-tap form
static inline int ctx_conv3_phase_loses(int M, int Cout, int Cin) { return 0; }

int ctx_gemm_dispatch(GemmArgs &a, bool conv, hipStream_t s);
// 256x256 8-wave kernel (gemm8.hip): launches and returns 1 when the problem suits it, else 0
int ctx_gemm8_try(GemmArgs &a, bool conv, bool force, hipStream_t s);
// halo-staged 3x3 convolution (conv_halo.hip), ni = 1 | 2 (64 / 128 features per workgroup): 1 when launched
int ctx_conv_halo_try(GemmArgs &a, int ni, hipStream_t s);
// 144x160 kernel (gemm144.hip; plan value use8 = 4: 6 waves, 5: 15 waves): 1 when launched
int ctx_gemm144_try(GemmArgs &a, bool conv, int form, hipStream_t s);
// split-K factor the heuristic would use for this problem (1 = none); caller provides a.part = S*M*N floats
int ctx_gemm_pick_split(int M, int N, int K, int epi);
// fills a.splitk / a.tile / a.use8 for a fully described problem: the tuned table (gemm_tuned.h) first, heuristics otherwise
void ctx_gemm_plan(GemmArgs &a, bool conv);
// The engines' small ops (elementwise.hip, gemm.hip, unet.hip, vae.hip).  Each validates its arguments (CTX_E_ARG, nothing launched) and
// launches; include/ctx_nerf.h exports every one as a test seam under the name ctx_<op>_f16 / _f32 with the contract spelled out.
int ctx_gemv_core(const f16 *x, const f16 *w, const f16 *bias, int Bm, int N, int K, int silu_in, int silu_out, f16 *out, hipStream_t s);
int ctx_concat_core(const f16 *a, const f16 *b, int64_t M, int Ca, int Cb, f16 *y, hipStream_t s);
int ctx_transpose_v_core(const f16 *v, int B, int S, int ld, int heads, int Sp, f16 *vt, hipStream_t s);
int ctx_f32_to_f16_core(const float *x, int64_t n, f16 *y, hipStream_t s);
int ctx_time_embed_core(const float *t, int B, int dim, f16 *out, hipStream_t s);
int ctx_conv_in_core(const float *x, const f16 *w, const f16 *bias, int B, int Cin, int H, int W, int Cout, f16 *y, hipStream_t s);
int ctx_conv_out_core(const f16 *x, const f16 *w, const f16 *bias, int B, int H, int W, int C, int Cout, float *out, hipStream_t s);
int ctx_attention_core(const f16 *Q, const f16 *K, const f16 *V, int B, int Sq, int Skv, int heads, int q_stride,
                       int kv_stride, float scale, f16 *O, int o_stride, hipStream_t s);
extern "C" int64_t ctx_groupnorm_ws_bytes(int32_t B, int32_t groups);
// norms over the fp32 residual stream (x32 != 0) or fp16 activations; output fp16.  x2 != null: the input is the channel concatenation
// [x ; x2] read in place (x: channels 0 .. Ca with pixel stride Ca; x2: channels Ca .. C with pixel stride C - Ca; Ca % 8 == 0)
int ctx_groupnorm_any(const void *x, int x32, const void *gamma, const void *beta, int B, int HW, int C, int groups, float eps, int silu,
                      void *y, void *stats_ws, hipStream_t stream, const void *x2 = nullptr, int Ca = 0);
// 1: a GroupNorm of this shape, of one source or two, takes the two-pass form (k_gn_stats + k_gn_apply), 0: the one-kernel form
int ctx_groupnorm_two_pass(int HW, int C, int groups);
// the apply half of the two-pass form on partials part[B][NS][groups][2] that a producer wrote (GemmArgs::gn_part), fp16 input
int ctx_groupnorm_apply(const void *x, const float *part, int NS, const void *gamma, const void *beta, int B, int HW, int C, int groups, float eps,
                        int silu, void *y, hipStream_t stream);
// a split-K convolution's unreduced output (GemmArgs::keep_slabs): S fp32 slabs of [M][C] at stride MN, and the epilogue operands the
// reduce would have added; the one-kernel GroupNorm reads it in place of the reduced fp16 tensor, bit-identically
struct GnSlabs { const float *part; int S; size_t MN; const f16 *bias, *bias2, *rowbias; int ldrb; };
int ctx_groupnorm_slabs(const GnSlabs &sl, const void *gamma, const void *beta, int B, int HW, int C, int groups, float eps, int silu, void *y,
                        hipStream_t stream);
// GroupNorm(+SiLU) backward, input gradient only, fp16 NHWC: dx = d(loss)/dx (+ add); ws of ctx_groupnorm_bwd_ws_bytes(B, groups)
// (ctx_groupnorm_bwd_ws_bytes / ctx_groupnorm_bwd_f16: declared in include/ctx_nerf.h, the unit tests call them too)
int ctx_layernorm_any(const void *x, int x32, const void *gamma, const void *beta, int64_t rows, int C, float eps, void *y, hipStream_t stream);
int ctx_concat32_core(const float *a, const float *b, int64_t M, int Ca, int Cb, float *y, hipStream_t s);
int ctx_f16_to_f32_core(const f16 *x, int64_t n, float *y, hipStream_t s);
// ControlNet's few-channel 3x3 convolution (exactly one of x32 f32 NCHW / x16 f16 NHWC) and dst += scale * src over n f16 (n % 8 == 0)
int ctx_conv_small_core(const float *x32, const f16 *x16, const f16 *w, const f16 *bias, int B, int H, int W, int Cin, int Cout, int stride, int silu,
                        f16 *y, hipStream_t s);
int ctx_add_scaled_core(f16 *dst, const f16 *src, float scale, int64_t n, hipStream_t s);
// the VAE's 1x1 convolutions over a few channels -> f32 NCHW: x f32 NCHW with C <= 8, or (nhwc16) f16 NHWC with C <= 16
int ctx_pointwise_core(const void *x, const f16 *w, const f16 *b, int B, int C, int64_t HW, bool nhwc16, float *y, hipStream_t s);

// profiling hooks (api.cpp): when on, MFMA kernels are launched with hipExtLaunchKernelGGL start/stop events
bool ctx_prof_on(void);
void ctx_prof_events(int klass, hipEvent_t *a, hipEvent_t *b);
