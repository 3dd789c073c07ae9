// Elementwise and small-convolution kernels of the UNet / VAE engines (NHWC fp16 activations), everything that is not a norm,
// a GEMM or attention.  HBM-bound ones move a 16-byte (8 x f16) vector per lane.
//   k_geglu                      GEGLU of a separate projection (the GEMM epilogue form lives in gemm_common.h)
//   k_concat                     channel concat (skip connections), fp16 or, through ctx_concat32_core, the fp32 residual stream
//   k_transpose_v                per-head transpose [B, S, ld] -> [B, heads, 64, Sp] (the VAE's attention and its backward)
//   k_f32_to_f16, k_f16_to_f32   layout converters
//   k_time_embed                 sinusoidal timestep embedding
//   k_conv_in, k_conv_out        the 3x3 convolutions with <= 16 input / <= 4 output channels (NCHW fp32 outside, NHWC fp16 inside)
//   k_cfg_plms                   CFG + PLMS scheduler step (src/stable_diffusion_depth.py:428-430,514)
#include "common.h"
#include "kernels.h"
#include <math.h>

// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_geglu(const f16 *__restrict__ h, int64_t M, int C4, f16 *__restrict__ y)
{
    const int c8n = C4 / 8;
    const int64_t total = M * c8n;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int64_t m = i / c8n;
        int c8 = (int)(i % c8n);
        f16x8 a = *(const f16x8 *)(h + m * 2 * C4 + c8 * 8);
        f16x8 g = *(const f16x8 *)(h + m * 2 * C4 + C4 + c8 * 8);
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float gf = (float)g[j];
            o[j] = (f16)((float)a[j] * (0.5f * gf * (1.0f + erff(gf * 0.70710678118654752f))));
        }
        *(f16x8 *)(y + m * C4 + c8 * 8) = o;
    }
}

extern "C" int32_t ctx_geglu_f16(const void *h, int64_t M, int32_t C4, void *y, ctx_stream_t stream)
{
    CTX_REQUIRE(h && y && M > 0 && C4 % 8 == 0, "geglu: bad args");
    hipLaunchKernelGGL(k_geglu, dim3(capped_blocks(M * (C4 / 8), 256, 4096)), dim3(256), 0, (hipStream_t)stream, (const f16 *)h, M, C4, (f16 *)y);
    CTX_CHECK_LAUNCH("geglu");
    return CTX_OK;
}

// ------------------------------------------------------------------------------------------------
// Channel concat (NHWC): y[m, :Ca] = a[m], y[m, Ca:] = b[m].
__global__ __launch_bounds__(256) void k_concat(const f16 *__restrict__ a, const f16 *__restrict__ b, int64_t M, int Ca,
                                                int Cb, f16 *__restrict__ y)
{
    const int n8 = (Ca + Cb) / 8, a8 = Ca / 8;
    const int64_t total = M * n8;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int64_t m = i / n8;
        int c8 = (int)(i % n8);
        f16x8 v = c8 < a8 ? *(const f16x8 *)(a + m * Ca + c8 * 8) : *(const f16x8 *)(b + m * Cb + (c8 - a8) * 8);
        *(f16x8 *)(y + i * 8) = v;
    }
}

// same copy with 4-byte elements (the fp32 residual stream): channels counted in f16-equivalents of 2 x the float count
int ctx_concat32_core(const float *a, const float *b, int64_t M, int Ca, int Cb, float *y, hipStream_t s)
{
    return ctx_concat_core((const f16 *)a, (const f16 *)b, M, 2 * Ca, 2 * Cb, (f16 *)y, s);
}

int ctx_concat_core(const f16 *a, const f16 *b, int64_t M, int Ca, int Cb, f16 *y, hipStream_t s)
{
    CTX_REQUIRE(a && b && y && M > 0 && Ca > 0 && Cb > 0 && Ca % 8 == 0 && Cb % 8 == 0, "concat: unsupported M=%lld Ca=%d Cb=%d", (long long)M, Ca, Cb);
    hipLaunchKernelGGL(k_concat, dim3(capped_blocks(M * ((Ca + Cb) / 8), 256, 4096)), dim3(256), 0, s, a, b, M, Ca, Cb, y);
    CTX_CHECK_LAUNCH("concat");
    return CTX_OK;
}

// V [B, S, ld] (head slice at column h*64) -> Vt [B, heads, 64, Sp] (keys contiguous, zero padded to Sp): a plain transpose of
// 64 x 64 tiles through LDS.  The VAE's attention and its backward use it; the UNet's attention reads V untransposed.
__global__ __launch_bounds__(256) void k_transpose_v(const f16 *__restrict__ v, int S, int ld, int heads, int Sp, f16 *__restrict__ vt)
{
    __shared__ f16 tile[64][66];
    const int b = blockIdx.z, hd = blockIdx.y, s0 = blockIdx.x * 64;
    // load 64 keys x 64 d, 16 B per lane: thread t -> key t/8 + 32*i, chunk t%8
    for (int i = 0; i < 2; ++i) {
        int key = (threadIdx.x >> 3) + 32 * i, c = threadIdx.x & 7;
        f16x8 val = {0, 0, 0, 0, 0, 0, 0, 0};
        if (s0 + key < S) val = *(const f16x8 *)(v + ((size_t)b * S + s0 + key) * ld + hd * 64 + c * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) tile[key][c * 8 + j] = val[j];
    }
    __syncthreads();
    for (int i = 0; i < 2; ++i) {
        int d = (threadIdx.x >> 3) + 32 * i, c = threadIdx.x & 7;
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = tile[c * 8 + j][d];
        if (s0 + c * 8 < Sp) *(f16x8 *)(vt + (((size_t)b * heads + hd) * 64 + d) * Sp + s0 + c * 8) = o;
    }
}

int ctx_transpose_v_core(const f16 *v, int B, int S, int ld, int heads, int Sp, f16 *vt, hipStream_t s)
{
    CTX_REQUIRE(v && vt, "transpose_v: null pointer");
    // the kernel moves 16-byte pieces: 8 keys of a Vt row per store (a row must end on one), 8 columns of a V row per load
    CTX_REQUIRE(B > 0 && S > 0 && heads > 0 && Sp % 8 == 0 && Sp >= S && ld % 8 == 0 && ld >= heads * 64,
                "transpose_v: need Sp %% 8 == 0, Sp >= S, ld %% 8 == 0, ld >= 64 heads (B=%d S=%d ld=%d heads=%d Sp=%d)", B, S, ld, heads, Sp);
    hipLaunchKernelGGL(k_transpose_v, dim3(cdiv(Sp, 64), heads, B), dim3(256), 0, s, v, S, ld, heads, Sp, vt);
    CTX_CHECK_LAUNCH("transpose_v");
    return CTX_OK;
}

// ------------------------------------------------------------------------------------------------
// f32 -> f16 row-major copy (context embeddings).
__global__ __launch_bounds__(256) void k_f32_to_f16(const float *__restrict__ x, int64_t n, f16 *__restrict__ y)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) y[i] = (f16)x[i];
}
__global__ __launch_bounds__(256) void k_f16_to_f32(const f16 *__restrict__ x, int64_t n8, float *__restrict__ y)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
        const f16x8 v = *(const f16x8 *)(x + i * 8);
        f32x4 a = {(float)v[0], (float)v[1], (float)v[2], (float)v[3]}, b = {(float)v[4], (float)v[5], (float)v[6], (float)v[7]};
        *(f32x4 *)(y + i * 8) = a; *(f32x4 *)(y + i * 8 + 4) = b;
    }
}
int ctx_f16_to_f32_core(const f16 *x, int64_t n, float *y, hipStream_t s)
{
    CTX_REQUIRE(x && y && n > 0 && n % 8 == 0, "f16_to_f32: n=%lld is not a positive multiple of 8", (long long)n);
    hipLaunchKernelGGL(k_f16_to_f32, dim3(capped_blocks(n / 8, 256, 4096)), dim3(256), 0, s, x, n / 8, y);
    CTX_CHECK_LAUNCH("f16_to_f32");
    return CTX_OK;
}
int ctx_f32_to_f16_core(const float *x, int64_t n, f16 *y, hipStream_t s)
{
    CTX_REQUIRE(x && y && n > 0, "f32_to_f16: null pointer or n=%lld < 1", (long long)n);
    hipLaunchKernelGGL(k_f32_to_f16, dim3(capped_blocks(n, 256, 2048)), dim3(256), 0, s, x, n, y);
    CTX_CHECK_LAUNCH("f32_to_f16");
    return CTX_OK;
}

// Sinusoidal timestep embedding, diffusers get_timestep_embedding(flip_sin_to_cos=True, freq_shift=0):
// emb[b] = [cos(t*f_0..f_{h-1}), sin(t*f_0..)] with f_i = exp(-ln(10000) * i / h), h = dim/2.
__global__ void k_time_embed(const float *__restrict__ t, int B, int dim, f16 *__restrict__ out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    int half = dim / 2;
    if (i >= half) return;
    float fr = expf(-9.210340371976184f * (float)i / (float)half);
    float a = t[0] * fr;
    float c = cosf(a), sn = sinf(a);
    for (int b = 0; b < B; ++b) {
        out[(size_t)b * dim + i] = (f16)c;
        out[(size_t)b * dim + half + i] = (f16)sn;
    }
}
int ctx_time_embed_core(const float *t, int B, int dim, f16 *out, hipStream_t s)
{
    CTX_REQUIRE(t && out && B > 0 && dim >= 2 && dim % 2 == 0, "time_embed: unsupported B=%d dim=%d", B, dim);
    hipLaunchKernelGGL(k_time_embed, dim3(cdiv(dim / 2, 64)), dim3(64), 0, s, t, B, dim, out);
    CTX_CHECK_LAUNCH("time_embed");
    return CTX_OK;
}

// conv_in: sample [B,Cin,H,W] f32 NCHW (Cin <= 16) -> y [B,H,W,Cout] f16, 3x3 pad 1.  w packed [Cout][3][3][8 | 16] f16.
// One pixel per lane: its 9 x Cin inputs live in registers; the weights of this block's slice of output channels
// sit in LDS and are read as wave-wide broadcasts; grid.y splits the output channels.
#define CI_SPLIT 16
// CP = padded input channels of the weight pack [Cout][3][3][CP]: 8 (latents + depth, VAE) or 16 (the 9-channel inpainting UNet);
// CX = channels actually multiplied (the pack's zero padding is skipped).  The block's weight slice is converted to fp32 once
// when it is staged (the kernel is VALU-bound: one cvt per FMA otherwise).
template <int CP, int CX>
__global__ __launch_bounds__(256) void k_conv_in(const float *__restrict__ x, const f16 *__restrict__ w,
                                                 const f16 *__restrict__ bias, int B, int Cin, int H, int W, int Cout,
                                                 f16 *__restrict__ y)
{
    extern __shared__ __attribute__((aligned(16))) float s_w[];   // [o_per * 8][9][CX]
    constexpr int WR = 9 * CP, WX = 9 * CX;
    const int o8n = Cout / 8;
    const int o8_per = (o8n + CI_SPLIT - 1) / CI_SPLIT;
    const int o8_0 = blockIdx.y * o8_per, o8_1 = min(o8n, o8_0 + o8_per);
    const int no = (o8_1 - o8_0) * 8;
    for (int i = threadIdx.x; i < no * WX; i += 256) {
        const int o = i / WX, r = i - o * WX, t = r / CX, c = r - t * CX;
        s_w[i] = (float)w[(size_t)(o8_0 * 8 + o) * WR + t * CP + c];
    }
    __syncthreads();
    const int64_t npix = (int64_t)B * H * W;
    const int64_t pix0 = (int64_t)blockIdx.x * 256;
    const int64_t pix = pix0 + threadIdx.x;
    const bool live = pix < npix;
    const int64_t pq = live ? pix : npix - 1;
    int b = (int)(pq / (H * W)), p = (int)(pq % (H * W));
    int oy = p / W, ox = p % W;
    float in[9][CX];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        int iy = oy + t / 3 - 1, ix = ox + t % 3 - 1;
        bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
#pragma unroll
        for (int c = 0; c < CX; ++c)
            in[t][c] = (ok && c < Cin) ? (float)(f16)x[(((size_t)b * Cin + c) * H + iy) * W + ix] : 0.f;
    }
    // A lane's 8 channels are 16 bytes of a pixel row that is Cout x 2 bytes long: stored directly that is one 16-byte piece
    // per cache line and instruction (the kernel was bound by those stores: 53 us for 11.8 MB at 96^2 x 320).  Eight channel
    // groups at a time go through an LDS patch [256 pixels][64 channels] and leave as 128-byte row segments.
    f16 *patch = (f16 *)(s_w + no * WX);
    for (int g0 = o8_0; g0 < o8_1; g0 += 8) {
        const int ng = min(8, o8_1 - g0);
        for (int gi = 0; gi < ng; ++gi) {
            const int o8 = g0 + gi;
            f16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float *wr = s_w + ((o8 - o8_0) * 8 + j) * WX;
                float acc = (float)bias[o8 * 8 + j];
#pragma unroll
                for (int t = 0; t < 9; ++t)
#pragma unroll
                    for (int c = 0; c < CX; ++c) acc += in[t][c] * wr[t * CX + c];
                o[j] = (f16)acc;
            }
            *(f16x8 *)(patch + threadIdx.x * 72 + gi * 8) = o;      // row stride 72 f16 = 144 B: conflict-free 16-byte writes
        }
        __syncthreads();
        for (int ch = threadIdx.x; ch < 256 * ng; ch += 256) {
            const int px = ch / ng, gi = ch - px * ng;
            if (pix0 + px < npix) *(f16x8 *)(y + (pix0 + px) * Cout + (g0 + gi) * 8) = *(const f16x8 *)(patch + px * 72 + gi * 8);
        }
        __syncthreads();
    }
}
int ctx_conv_in_core(const float *x, const f16 *w, const f16 *bias, int B, int Cin, int H, int W, int Cout, f16 *y, hipStream_t s)
{
    CTX_REQUIRE(x && w && bias && y && Cout > 0 && Cout % 8 == 0, "conv_in: unsupported Cout=%d", Cout);
    // the widest instantiation multiplies 16 channels of a [Cout][3][3][16] pack: more would be dropped without a word
    CTX_REQUIRE(Cin >= 1 && Cin <= 16, "conv_in: need 1 <= Cin <= 16 (Cin=%d)", Cin);
    CTX_REQUIRE(B > 0 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 31), "conv_in: unsupported grid B=%d H=%d W=%d", B, H, W);
    int64_t npix = (int64_t)B * H * W;
    int o8_per = (Cout / 8 + CI_SPLIT - 1) / CI_SPLIT;
    const int cx = Cin <= 3 ? 3 : Cin <= 5 ? Cin : Cin <= 8 ? 8 : Cin == 9 ? 9 : 16;      // the CX of the instantiation chosen below
    CTX_REQUIRE((size_t)o8_per * 8 * 9 * cx * sizeof(float) + 256 * 72 * sizeof(f16) <= 64 * 1024,
                "conv_in: the weight slice of Cout=%d at Cin=%d does not fit the LDS", Cout, Cin);
    const dim3 grid((unsigned)cdiv64(npix, 256), CI_SPLIT);
#define CI_GO(CP_, CX_) hipLaunchKernelGGL((k_conv_in<CP_, CX_>), grid, dim3(256), (size_t)o8_per * 8 * 9 * CX_ * sizeof(float) + 256 * 72 * sizeof(f16), s, x, w, bias, B, Cin, H, W, Cout, y)
    if (Cin <= 3) CI_GO(8, 3);
    else if (Cin == 4) CI_GO(8, 4);
    else if (Cin == 5) CI_GO(8, 5);
    else if (Cin <= 8) CI_GO(8, 8);
    else if (Cin == 9) CI_GO(16, 9);
    else CI_GO(16, 16);
#undef CI_GO
    CTX_CHECK_LAUNCH("conv_in");
    return CTX_OK;
}

// conv_out: x [B,H,W,C] f16 (already GN+SiLU'd) -> out [B,Cout,H,W] f32 NCHW, Cout <= 4, 3x3 pad 1.
// w packed [Cout][3][3][C] f16, staged in LDS once per block.  One wave per output pixel: the 9 taps x C/8 16-byte chunks
// of the pixel's neighbourhood are one flat item list dealt over the 64 lanes (all lanes busy for any C), every load of a
// lane issued (unconditionally, clamped) before the first use; the Cout sums are DPP wave reductions.
// WF32: the staged weights are converted to fp32 once (the kernel is VALU-bound: 40 cvt per 32 FMA otherwise); used when the
// fp32 copy fits 64 KiB of LDS
template <int NU, bool WF32>
__global__ __launch_bounds__(256) void k_conv_out(const f16 *__restrict__ x, const f16 *__restrict__ w,
                                                  const f16 *__restrict__ bias, int B, int H, int W, int C, int Cout,
                                                  float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) char s_cw_raw[];    // [Cout][9][C] f16 or fp32
    f16 *s_cw = (f16 *)s_cw_raw;
    float *s_cf = (float *)s_cw_raw;
    const int nwt = Cout * 9 * C;
    if (WF32) {
        for (int i = threadIdx.x * 8; i < nwt; i += 256 * 8) {
            const f16x8 v = *(const f16x8 *)(w + i);
#pragma unroll
            for (int j = 0; j < 8; ++j) s_cf[i + j] = (float)v[j];
        }
    } else {
        for (int i = threadIdx.x * 8; i < nwt; i += 256 * 8) *(f16x8 *)(s_cw + i) = *(const f16x8 *)(w + i);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int c8n = C / 8, nitems = 9 * c8n;
    const int64_t npix = (int64_t)B * H * W;
    const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    int itap[NU], ic[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int i = min(lane + 64 * u, nitems - 1);
        itap[u] = i / c8n; ic[u] = (i - itap[u] * c8n) * 8;
    }
    // a wave walks its pixels with the NEXT pixel's loads issued before the current one is reduced (the kernel is bound by the
    // latency of those loads, not by the arithmetic: one pixel in flight per wave took 41 us at 96^2 x 320 channels)
    const int64_t pstep = ((int64_t)gridDim.x * 256) >> 6;
    f16x8 xn[NU];
    auto fetch = [&](int64_t pp_) {
        const int64_t q = pp_ < npix ? pp_ : npix - 1;
        const int b = (int)(q / (H * W)), p = (int)(q % (H * W));
        const int oy = p / W, ox = p % W;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int iy = oy + itap[u] / 3 - 1, ix = ox + itap[u] % 3 - 1;
            const int cy = min(max(iy, 0), H - 1), cx = min(max(ix, 0), W - 1);
            xn[u] = *(const f16x8 *)(x + (((size_t)b * H + cy) * W + cx) * C + ic[u]);
            if (lane + 64 * u >= nitems || iy != cy || ix != cx) xn[u] = zero8;
        }
    };
    int64_t pix = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (pix < npix) fetch(pix);
    for (; pix < npix; pix += pstep) {
        const int b = (int)(pix / (H * W)), p = (int)(pix % (H * W));
        const int oy = p / W, ox = p % W;
        f16x8 xv[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) xv[u] = xn[u];
        if (pix + pstep < npix) fetch(pix + pstep);
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            float xf[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) xf[j] = (float)xv[u][j];
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                if (o < Cout) {
                    if (WF32) {
                        const float *wr = s_cf + itap[u] * C + ic[u] + o * 9 * C;
                        const f32x4 w0 = *(const f32x4 *)wr, w1 = *(const f32x4 *)(wr + 4);
#pragma unroll
                        for (int j = 0; j < 4; ++j) { acc[o] += xf[j] * w0[j]; }
#pragma unroll
                        for (int j = 0; j < 4; ++j) { acc[o] += xf[4 + j] * w1[j]; }
                    } else {
                        const f16x8 wv = *(const f16x8 *)(s_cw + itap[u] * C + ic[u] + o * 9 * C);
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc[o] += xf[j] * (float)wv[j];
                    }
                }
            }
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            if (o < Cout) {
                float v = wave_sum_dpp(acc[o]);
                if (lane == 0) out[(((size_t)b * Cout + o) * H + oy) * W + ox] = v + (float)bias[o];
            }
        }
    }
}
int ctx_conv_out_core(const f16 *x, const f16 *w, const f16 *bias, int B, int H, int W, int C, int Cout, float *out, hipStream_t s)
{
    const int nitems = 9 * (C / 8);
    const size_t lds16 = (size_t)Cout * 9 * C * sizeof(f16);
    CTX_REQUIRE(x && w && bias && out, "conv_out: null pointer");
    CTX_REQUIRE(Cout >= 1 && Cout <= 4 && C >= 8 && C % 8 == 0 && nitems <= 64 * 12 && lds16 <= 64 * 1024, "conv_out: unsupported C=%d Cout=%d", C, Cout);
    CTX_REQUIRE(B > 0 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 31), "conv_out: unsupported grid B=%d H=%d W=%d", B, H, W);
    const unsigned nb = capped_blocks((int64_t)B * H * W, 4, 2048);       // every block stages the weights: keep them few and persistent
    const bool f32w = 2 * lds16 <= 64 * 1024;
    const size_t lds = f32w ? 2 * lds16 : lds16;
#define CO_GO(NU_) CTX_BOOL_GO(f32w, WF, hipLaunchKernelGGL((k_conv_out<NU_, WF>), dim3(nb), dim3(256), lds, s, x, w, bias, B, H, W, C, Cout, out))
    if (nitems <= 64 * 3) CO_GO(3);
    else if (nitems <= 64 * 6) CO_GO(6);
    else CO_GO(12);
#undef CO_GO
    CTX_CHECK_LAUNCH("conv_out");
    return CTX_OK;
}

// ------------------------------------------------------------------------------------------------
// CFG combine + PNDM/PLMS linear-multistep update, one pass over the latent.
__global__ __launch_bounds__(256) void k_cfg_plms(const float *__restrict__ eps_pair, int64_t n, float guidance,
                                                  float *__restrict__ ets, int head, float c0, float c1, float c2,
                                                  float c3, float sample_coeff, float eps_coeff, int mode,
                                                  float *__restrict__ cur, float *__restrict__ x)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float eu = eps_pair[i], et = eps_pair[n + i];
        float e = eu + guidance * (et - eu);
        float xs;
        float comb;
        if (mode == 1) {
            // second evaluation of the first PLMS step: average with the stored epsilon, restart from cur_sample
            comb = (e + ets[(size_t)head * n + i]) / 2.0f;
            xs = cur[i];
        } else {
            ets[(size_t)head * n + i] = e;
            float e1 = ets[(size_t)((head + 3) & 3) * n + i];
            float e2 = ets[(size_t)((head + 2) & 3) * n + i];
            float e3 = ets[(size_t)((head + 1) & 3) * n + i];
            comb = c0 * e;
            if (c1 != 0.f) comb += c1 * e1;
            if (c2 != 0.f) comb += c2 * e2;
            if (c3 != 0.f) comb += c3 * e3;
            xs = x[i];
            if (mode == 2) cur[i] = xs;      // first step: remember cur_sample
        }
        x[i] = sample_coeff * xs - eps_coeff * comb;
    }
}

extern "C" int32_t ctx_cfg_plms_step(const float *eps_pair, int64_t n, float guidance, float *ets, int32_t head,
                                     const float *coef4, float sample_coeff, float eps_coeff, int32_t mode,
                                     float *cur_sample_ws, float *x, ctx_stream_t stream)
{
    CTX_REQUIRE(eps_pair && ets && coef4 && x && n > 0 && head >= 0 && head < 4, "cfg_plms_step: bad args");
    CTX_REQUIRE(mode == 0 || cur_sample_ws, "cfg_plms_step: mode %d needs cur_sample_ws", mode);
    hipLaunchKernelGGL(k_cfg_plms, dim3(capped_blocks(n, 256, 2048)), dim3(256), 0, (hipStream_t)stream, eps_pair, n, guidance, ets, head,
                       coef4[0], coef4[1], coef4[2], coef4[3], sample_coeff, eps_coeff, mode, cur_sample_ws, x);
    CTX_CHECK_LAUNCH("cfg_plms_step");
    return CTX_OK;
}

// ---- test seams: each op above alone, through the host function the engines call (tests/engine_ops_rule.py) -----------------------
extern "C" int32_t ctx_concat_f16(const void *a, const void *b, int64_t M, int32_t Ca, int32_t Cb, void *y, ctx_stream_t stream)
{
    return ctx_concat_core((const f16 *)a, (const f16 *)b, M, Ca, Cb, (f16 *)y, (hipStream_t)stream);
}
extern "C" int32_t ctx_concat_f32(const float *a, const float *b, int64_t M, int32_t Ca, int32_t Cb, float *y, ctx_stream_t stream)
{
    CTX_REQUIRE(Ca > 0 && Cb > 0 && Ca <= (1 << 29) && Cb <= (1 << 29), "concat_f32: unsupported Ca=%d Cb=%d", Ca, Cb);
    return ctx_concat32_core(a, b, M, Ca, Cb, y, (hipStream_t)stream);
}
extern "C" int32_t ctx_transpose_v_f16(const void *v, int32_t B, int32_t S, int32_t ld, int32_t heads, int32_t Sp, void *vt, ctx_stream_t stream)
{
    CTX_REQUIRE(B <= 65535 && heads <= 65535, "transpose_v: B=%d / heads=%d exceed the grid", B, heads);
    return ctx_transpose_v_core((const f16 *)v, B, S, ld, heads, Sp, (f16 *)vt, (hipStream_t)stream);
}
extern "C" int32_t ctx_f32_to_f16(const float *x, int64_t n, void *y, ctx_stream_t stream)
{
    return ctx_f32_to_f16_core(x, n, (f16 *)y, (hipStream_t)stream);
}
extern "C" int32_t ctx_f16_to_f32(const void *x, int64_t n, float *y, ctx_stream_t stream)
{
    return ctx_f16_to_f32_core((const f16 *)x, n, y, (hipStream_t)stream);
}
extern "C" int32_t ctx_time_embed_f16(const float *t, int32_t B, int32_t dim, void *out, ctx_stream_t stream)
{
    return ctx_time_embed_core(t, B, dim, (f16 *)out, (hipStream_t)stream);
}
extern "C" int32_t ctx_conv_in_f16(const float *x, const void *w_pack, const void *bias, int32_t B, int32_t Cin, int32_t H, int32_t W, int32_t Cout,
                                   void *y, ctx_stream_t stream)
{
    return ctx_conv_in_core(x, (const f16 *)w_pack, (const f16 *)bias, B, Cin, H, W, Cout, (f16 *)y, (hipStream_t)stream);
}
extern "C" int32_t ctx_conv_out_f16(const void *x, const void *w, const void *bias, int32_t B, int32_t H, int32_t W, int32_t C, int32_t Cout,
                                    float *out, ctx_stream_t stream)
{
    return ctx_conv_out_core((const f16 *)x, (const f16 *)w, (const f16 *)bias, B, H, W, C, Cout, out, (hipStream_t)stream);
}
