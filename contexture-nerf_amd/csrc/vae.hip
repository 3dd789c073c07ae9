// VAE engine: diffusers `AutoencoderKL.decode` (post_quant_conv + Decoder) as used by
// StableDiffusion.decode_latents (src/stable_diffusion_depth.py:976-990): latents [B,4,h,w] -> image [B,3,8h,8w], and
// `AutoencoderKL.encode` (Encoder + quant_conv) behind StableDiffusion.encode_imgs (:971-975): image [B,3,8h,8w] ->
// moments [B,8,h,w] (mean | logvar of the latent distribution; sampling stays with the caller's RNG).
// Reuses the UNet's fp16 MFMA conv / GEMM and GroupNorm kernels; the single-head (dim 512) mid-block attention is run
// as two GEMMs around a row softmax (scores are materialised: it is one call per painted view, not per denoise step).
// Parameter names follow the diffusers AutoencoderKL state_dict ("decoder.up_blocks.2.resnets.0.conv1.weight", ...).
#include "engine.h"
#include <algorithm>

struct VRes { int cin, cout; size_t n1g, n1b, c1w, c1b, n2g, n2b, c2w, c2b, scw, scb; size_t c1wT = 0, c2wT = 0, scwT = 0; };
struct VAttn { size_t ng, nb, qkv, qkvb, ow, ob; size_t qkvT = 0, owT = 0; };

// what the decoder and the encoder both have around their level blocks: conv_in, the mid block (resnet, attention, resnet),
// conv_norm_out and conv_out
struct VHalf { size_t ciw, cib; VRes mid[2]; VAttn att; size_t cng, cnb, cow, cob; size_t cowT = 0; };

struct ctx_vae : Engine {
    ctx_vae_config_t cfg;
    VHalf dec, enc;
    size_t pqw, pqb, qw, qb;                  // post_quant_conv (before the decoder), quant_conv (after the encoder)
    std::vector<std::vector<VRes>> down;
    std::vector<size_t> dnw, dnb;
    std::vector<std::vector<VRes>> up;
    std::vector<size_t> upw, upb;
    std::vector<int> upc;
    int n_dec_params = 0;
    // encoder backward: transposed packs + the tape of the last training forward (pointers into the workspace)
    std::vector<size_t> dnwT;
    struct ResTape { const f16 *x, *h; };
    struct Tape {
        bool valid = false; int B = 0, H = 0, W = 0; size_t top = 0;
        const f16 *conv_in_out = nullptr;
        std::vector<ResTape> res;          // in forward order: down[i][j]..., mid0, mid1
        const f16 *attn_in = nullptr, *qkv = nullptr, *norm_out_in = nullptr;
    } tape;
    bool train = false;
};

static void vadd_bwd_conv3(ctx_vae *v, size_t &dstT, int cout, int cin, int pad)
{
    dstT = v->walloc((size_t)cin * 9 * pad);
    Param &q = v->params.back();
    q.kind2 = 1; q.dst2 = dstT; q.pad2 = pad;
}
static void vadd_bwd_mat(ctx_vae *v, size_t dstT, int ld, int col)
{
    Param &q = v->params.back();
    q.kind2 = 2; q.dst2 = dstT; q.ld2 = ld; q.col2 = col;
}

static void vadd_res(ctx_vae *v, const std::string &p, int cin, int cout, VRes &r, bool bwd = false)
{
    r.cin = cin; r.cout = cout;
    r.n1g = v->vec(p + ".norm1.weight", cin); r.n1b = v->vec(p + ".norm1.bias", cin);
    r.c1w = v->add(p + ".conv1.weight", {cout, cin, 3, 3}, 1, v->walloc((size_t)cout * cin * 9), cout, cin);
    if (bwd) vadd_bwd_conv3(v, r.c1wT, cout, cin, cout);
    r.c1b = v->vec(p + ".conv1.bias", cout);
    r.n2g = v->vec(p + ".norm2.weight", cout); r.n2b = v->vec(p + ".norm2.bias", cout);
    r.c2w = v->add(p + ".conv2.weight", {cout, cout, 3, 3}, 1, v->walloc((size_t)cout * cout * 9), cout, cout);
    if (bwd) vadd_bwd_conv3(v, r.c2wT, cout, cout, cout);
    r.c2b = v->vec(p + ".conv2.bias", cout);
    if (cin != cout) {
        r.scw = v->add(p + ".conv_shortcut.weight", {cout, cin, 1, 1}, 0, v->walloc((size_t)cout * cin));
        if (bwd) { r.scwT = v->walloc((size_t)cin * cout); vadd_bwd_mat(v, r.scwT, cout, 0); }
        r.scb = v->vec(p + ".conv_shortcut.bias", cout);
    } else r.scw = r.scb = 0;
}

static void vadd_attn(ctx_vae *v, const std::string &ap, int top, VAttn &a, bool bwd = false)
{
    a.ng = v->vec(ap + ".group_norm.weight", top); a.nb = v->vec(ap + ".group_norm.bias", top);
    a.qkv = v->walloc((size_t)3 * top * top); a.qkvb = v->walloc((size_t)3 * top);
    if (bwd) a.qkvT = v->walloc((size_t)3 * top * top);           // [top (in)][3 top (q | k | v out)]
    const char *qkv[3] = {"to_q", "to_k", "to_v"};
    for (int k = 0; k < 3; ++k) {
        v->add(ap + "." + qkv[k] + ".weight", {top, top}, 0, a.qkv + (size_t)k * top * top);
        if (bwd) vadd_bwd_mat(v, a.qkvT, 3 * top, k * top);
        v->add(ap + "." + qkv[k] + ".bias", {top}, 0, a.qkvb + (size_t)k * top);
    }
    a.ow = v->add(ap + ".to_out.0.weight", {top, top}, 0, v->walloc((size_t)top * top));
    if (bwd) { a.owT = v->walloc((size_t)top * top); vadd_bwd_mat(v, a.owT, top, 0); }
    a.ob = v->vec(ap + ".to_out.0.bias", top);
}

// the three pieces of a VHalf, in the order the table registers them (`p` = "decoder" / "encoder"; bwd: with the backward's packs)
static void vadd_conv_in(ctx_vae *v, const std::string &p, int cout, int cin, VHalf &h)
{
    h.ciw = v->add(p + ".conv_in.weight", {cout, cin, 3, 3}, 2, v->walloc((size_t)cout * 72), cout, cin);
    h.cib = v->vec(p + ".conv_in.bias", cout);
}
static void vadd_mid(ctx_vae *v, const std::string &p, int top, VHalf &h, bool bwd)
{
    vadd_res(v, p + ".mid_block.resnets.0", top, top, h.mid[0], bwd);
    vadd_attn(v, p + ".mid_block.attentions.0", top, h.att, bwd);
    vadd_res(v, p + ".mid_block.resnets.1", top, top, h.mid[1], bwd);
}
static void vadd_conv_out(ctx_vae *v, const std::string &p, int cin, int cout, VHalf &h, bool bwd)
{
    h.cng = v->vec(p + ".conv_norm_out.weight", cin); h.cnb = v->vec(p + ".conv_norm_out.bias", cin);
    h.cow = v->add(p + ".conv_out.weight", {cout, cin, 3, 3}, 1, v->walloc((size_t)cout * cin * 9), cout, cin);
    if (bwd) vadd_bwd_conv3(v, h.cowT, cout, cin, 64);              // its few output channels padded to one 64-deep K stage
    h.cob = v->vec(p + ".conv_out.bias", cout);
}

extern "C" ctx_vae_t *ctx_vae_create(const ctx_vae_config_t *cfg)
{
    if (!cfg || cfg->n_levels < 1 || cfg->n_levels > 4 || cfg->latent_channels > 8 || cfg->out_channels > 4 || cfg->groups > 64 ||
        cfg->layers_per_block < 1 || cfg->layers_per_block > 3) { ctx_set_error("vae_create: unsupported config"); return nullptr; }
    for (int i = 0; i < cfg->n_levels; ++i)
        if (cfg->block_out_channels[i] % 64 || cfg->block_out_channels[i] % cfg->groups) { ctx_set_error("vae_create: channels must be multiples of 64 and of groups"); return nullptr; }
    ctx_vae *v = new ctx_vae();
    v->tag = "vae";
    v->cfg = *cfg;
    const int n = cfg->n_levels, L = cfg->latent_channels;
    const int *ch = cfg->block_out_channels;
    const int top = ch[n - 1];
    v->pqw = v->add("post_quant_conv.weight", {L, L, 1, 1}, 0, v->walloc((size_t)L * L));
    v->pqb = v->vec("post_quant_conv.bias", L);
    vadd_conv_in(v, "decoder", top, L, v->dec);
    vadd_mid(v, "decoder", top, v->dec, false);
    v->up.resize(n); v->upw.assign(n, 0); v->upb.assign(n, 0); v->upc.assign(n, 0);
    int out = top;
    for (int i = 0; i < n; ++i) {
        int prev = out; out = ch[n - 1 - i];
        std::string p = "decoder.up_blocks." + std::to_string(i);
        v->up[i].resize(cfg->layers_per_block + 1);
        for (int j = 0; j <= cfg->layers_per_block; ++j) vadd_res(v, p + ".resnets." + std::to_string(j), j == 0 ? prev : out, out, v->up[i][j]);
        if (i != n - 1) {
            v->upc[i] = out;
            v->upw[i] = v->add(p + ".upsamplers.0.conv.weight", {out, out, 3, 3}, 1, v->walloc((size_t)out * out * 9), out, out);
            v->derive_phase();
            v->upb[i] = v->vec(p + ".upsamplers.0.conv.bias", out);
        }
    }
    vadd_conv_out(v, "decoder", ch[0], cfg->out_channels, v->dec, false);
    // ---- encoder (diffusers Encoder: conv_in, DownEncoderBlock2D x n, UNetMidBlock2D, GroupNorm-SiLU-conv_out) + quant_conv.
    // Registered after the decoder so a decoder-only checkpoint still fills a prefix of the table.
    v->n_dec_params = (int)v->params.size();
    vadd_conv_in(v, "encoder", ch[0], cfg->out_channels, v->enc);
    v->down.resize(n); v->dnw.assign(n, 0); v->dnb.assign(n, 0);
    int cur = ch[0];
    for (int i = 0; i < n; ++i) {
        std::string p = "encoder.down_blocks." + std::to_string(i);
        v->down[i].resize(cfg->layers_per_block);
        for (int j = 0; j < cfg->layers_per_block; ++j) { vadd_res(v, p + ".resnets." + std::to_string(j), j == 0 ? cur : ch[i], ch[i], v->down[i][j], true); }
        cur = ch[i];
        if (i != n - 1) {
            v->dnw[i] = v->add(p + ".downsamplers.0.conv.weight", {cur, cur, 3, 3}, 1, v->walloc((size_t)cur * cur * 9), cur, cur);
            v->dnwT.resize(n, 0);
            vadd_bwd_conv3(v, v->dnwT[i], cur, cur, cur);
            v->dnb[i] = v->vec(p + ".downsamplers.0.conv.bias", cur);
        }
    }
    vadd_mid(v, "encoder", top, v->enc, true);
    vadd_conv_out(v, "encoder", top, 2 * L, v->enc, true);
    v->qw = v->add("quant_conv.weight", {2 * L, 2 * L, 1, 1}, 0, v->walloc((size_t)4 * L * L));
    v->qb = v->vec("quant_conv.bias", 2 * L);
    return v;
}

extern "C" void ctx_vae_destroy(ctx_vae_t *v) { delete v; }
extern "C" int32_t ctx_vae_param_count(const ctx_vae_t *v) { return engine_param_count(v); }
/* the first ctx_vae_decoder_param_count entries are post_quant_conv + decoder, the rest encoder + quant_conv */
extern "C" int32_t ctx_vae_decoder_param_count(const ctx_vae_t *v) { return v ? v->n_dec_params : 0; }
extern "C" const char *ctx_vae_param_name(const ctx_vae_t *v, int32_t i) { return engine_param_name(v, i); }
extern "C" int32_t ctx_vae_param_shape(const ctx_vae_t *v, int32_t i, int64_t shape4[4]) { return engine_param_shape(v, i, shape4); }
extern "C" int64_t ctx_vae_weight_bytes(const ctx_vae_t *v) { return engine_weight_bytes(v); }
extern "C" int32_t ctx_vae_bind(ctx_vae_t *v, void *weights, void *workspace, int64_t workspace_bytes)
{
    return engine_bind(v, weights, workspace, workspace_bytes, "vae_bind");
}
extern "C" int64_t ctx_vae_derived_bytes(const ctx_vae_t *v) { return engine_derived_bytes(v); }
extern "C" int32_t ctx_vae_bind_derived(ctx_vae_t *v, void *derived, int64_t bytes) { return engine_bind_derived(v, derived, bytes, "vae_bind_derived"); }
extern "C" int32_t ctx_vae_set_param(ctx_vae_t *v, int32_t i, const float *src, ctx_stream_t stream)
{
    return engine_set_param(v, i, src, stream, "vae_set_param");
}

// 1x1 convolution over a few channels per pixel -> f32 NCHW.  NHWC16 false: f32 NCHW input, C <= 8 (post_quant_conv on the latents,
// 16 MACs per pixel); true: f16 NHWC input, C <= 16 (quant_conv over the 2L moment channels of the encoder's output)
template <bool NHWC16>
__global__ __launch_bounds__(256) void k_pointwise(const void *__restrict__ xv, const f16 *__restrict__ w, const f16 *__restrict__ b,
                                                   int B, int C, int64_t HW, float *__restrict__ y)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (int64_t)B * HW; i += (int64_t)gridDim.x * 256) {
        int bb = (int)(i / HW); int64_t p = i % HW;
        float in[NHWC16 ? 16 : 8];
        for (int c = 0; c < C; ++c) in[c] = NHWC16 ? (float)((const f16 *)xv)[i * C + c] : ((const float *)xv)[((int64_t)bb * C + c) * HW + p];
        for (int o = 0; o < C; ++o) {
            float acc = (float)b[o];
            for (int c = 0; c < C; ++c) acc += in[c] * (float)w[o * C + c];
            y[((int64_t)bb * C + o) * HW + p] = acc;
        }
    }
}

// the launch of either form, as the decoder / encoder graphs and the test seam ctx_pointwise_f32 make it
int ctx_pointwise_core(const void *x, const f16 *w, const f16 *b, int B, int C, int64_t HW, bool nhwc16, float *y, hipStream_t s)
{
    CTX_REQUIRE(x && w && b && y, "pointwise: null pointer");
    // the kernel keeps a pixel's channels in a register array of 8 (f32 NCHW input) or 16 (f16 NHWC input) floats
    CTX_REQUIRE(B > 0 && HW > 0 && C >= 1 && C <= (nhwc16 ? 16 : 8), "pointwise: need 1 <= C <= %d (B=%d C=%d HW=%lld)", nhwc16 ? 16 : 8, B, C, (long long)HW);
    CTX_BOOL_GO(nhwc16, NH, hipLaunchKernelGGL(k_pointwise<NH>, dim3((unsigned)cdiv64((int64_t)B * HW, 256)), dim3(256), 0, s, x, w, b, B, C, HW, y));
    CTX_CHECK_LAUNCH("pointwise");
    return CTX_OK;
}

// row softmax of f16 scores [rows, n] * scale -> f16 probabilities (fp32 math), one workgroup per row
__global__ __launch_bounds__(256) void k_softmax_rows(const f16 *__restrict__ s, int n, float scale_log2e, f16 *__restrict__ p)
{
    const f16 *row = s + (size_t)blockIdx.x * n;
    f16 *out = p + (size_t)blockIdx.x * n;
    __shared__ float red[4];
    float mx = -INFINITY;
    for (int i = threadIdx.x * 8; i < n; i += 2048) {
        f16x8 v = *(const f16x8 *)(row + i);
#pragma unroll
        for (int j = 0; j < 8; ++j) mx = fmaxf(mx, (float)v[j]);
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) * scale_log2e;
    __syncthreads();
    float sum = 0.f;
    for (int i = threadIdx.x * 8; i < n; i += 2048) {
        f16x8 v = *(const f16x8 *)(row + i);
#pragma unroll
        for (int j = 0; j < 8; ++j) sum += __builtin_amdgcn_exp2f((float)v[j] * scale_log2e - mx);
    }
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    float inv = 1.0f / ((red[0] + red[1]) + (red[2] + red[3]));
    for (int i = threadIdx.x * 8; i < n; i += 2048) {
        f16x8 v = *(const f16x8 *)(row + i);
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (f16)(__builtin_amdgcn_exp2f((float)v[j] * scale_log2e - mx) * inv);
        *(f16x8 *)(out + i) = o;
    }
}

#define VRUN(expr) ENGINE_RUN(v, expr)

// the shared conv builder on this engine's weight offsets
static void vconv(ctx_vae *v, const f16 *x, size_t w, size_t bias, const f16 *res, int B, int H, int W, int Cin, int Cout, f16 *out,
                  ConvGeom g = ConvGeom())
{
    engine_conv3(*v, x, v->W + w, v->W + bias, res, B, H, W, Cin, Cout, out, g);
}
static void vgn(ctx_vae *v, const f16 *x, size_t g, size_t b, int B, int HW, int C, int silu, f16 *y, void *stats)
{
    VRUN(ctx_groupnorm_f16(x, v->W + g, v->W + b, B, HW, C, v->cfg.groups, 1e-6f, silu, y, stats, v->s));
}
static void vres(ctx_vae *v, const VRes &r, const f16 *x, int B, int H, int W, f16 *out, void *stats)
{
    const size_t M = (size_t)B * H * W;
    f16 *hkeep = nullptr;
    if (v->train) {                                  // training forward: the two GroupNorm inputs (x, h) stay on the tape
        hkeep = v->allocH(M * r.cout);
        v->tape.res.push_back({x, hkeep});
    }
    size_t mark = v->top;
    f16 *t1 = v->allocH(M * r.cin);
    vgn(v, x, r.n1g, r.n1b, B, H * W, r.cin, 1, t1, stats);
    f16 *h = hkeep ? hkeep : v->allocH(M * r.cout);
    vconv(v, t1, r.c1w, r.c1b, nullptr, B, H, W, r.cin, r.cout, h);
    f16 *t2 = v->allocH(M * r.cout);
    vgn(v, h, r.n2g, r.n2b, B, H * W, r.cout, 1, t2, stats);
    const f16 *sc = x;
    if (r.cin != r.cout) {
        f16 *s2 = v->allocH(M * r.cout);
        engine_linear(*v, x, v->W + r.scw, v->W + r.scb, nullptr, (int)M, r.cout, r.cin, s2);
        sc = s2;
    }
    vconv(v, t2, r.c2w, r.c2b, sc, B, H, W, r.cout, r.cout, out);
    v->top = mark;
}

// one of q | k | v of a batch entry's rows of the fused projection (row stride 3 top) -> a dense [S, top] operand
static void vrows(ctx_vae *v, const f16 *src, int S, int top, f16 *dst)
{
    v->copy2d(dst, (size_t)top * 2, src, (size_t)3 * top * 2, (size_t)top * 2, S);
}
// k_softmax_rows takes its scale times log2(e) (it exponentiates with exp2)
static float softmax_scale_log2e(float scale) { return 1.4426950408889634f * scale; }
// probabilities pr = softmax(q k^T scale) [S, S] of dense q, k [S, top]; the scores sc are materialised
static void vprobs(ctx_vae *v, const f16 *qb, const f16 *kb, int S, int top, float scale_log2e, f16 *sc, f16 *pr)
{
    engine_linear(*v, qb, kb, nullptr, nullptr, S, S, top, sc);
    ENGINE_LAUNCH(v, k_softmax_rows, dim3(S), dim3(256), 0, sc, S, scale_log2e, pr);
}

// single-head attention of the mid block, dim = top: q,k,v GEMM -> per-batch scores GEMM -> softmax -> P.V GEMM -> out proj
// (+residual o); the result lands in x.
static void vattn(ctx_vae *v, const VAttn &at, const f16 *o, f16 *x, int B, int h, int w, int top, void *stats)
{
    const int S = h * w, M = B * S;
    if (S % 64) { v->rc = CTX_E_ARG; ctx_set_error("vae: latent h*w must be a multiple of 64 (got %d)", S); return; }
    f16 *qkeep = nullptr;
    if (v->train) { qkeep = v->allocH((size_t)M * 3 * top); v->tape.attn_in = o; v->tape.qkv = qkeep; }
    size_t mark = v->top;
    f16 *g = v->allocH((size_t)M * top);
    vgn(v, o, at.ng, at.nb, B, S, top, 0, g, stats);
    f16 *qkv = qkeep ? qkeep : v->allocH((size_t)M * 3 * top);
    engine_linear(*v, g, v->W + at.qkv, v->W + at.qkvb, nullptr, M, 3 * top, top, qkv);
    f16 *att = v->allocH((size_t)M * top);
    f16 *sc = v->allocH((size_t)S * S), *pr = v->allocH((size_t)S * S), *vt = v->allocH((size_t)top * S);
    f16 *qb = v->allocH((size_t)S * top), *kb = v->allocH((size_t)S * top);
    for (int b = 0; b < B; ++b) {
        const f16 *base = qkv ? qkv + (size_t)b * S * 3 * top : nullptr;
        vrows(v, base, S, top, qb);
        vrows(v, base ? base + top : nullptr, S, top, kb);
        VRUN(ctx_transpose_v_core(base + 2 * top, 1, S, 3 * top, top / 64, S, vt, v->s));     // V^T through the head-transpose kernel
        vprobs(v, qb, kb, S, top, softmax_scale_log2e(1.0f / sqrtf((float)top)), sc, pr);
        engine_linear(*v, pr, vt, nullptr, nullptr, S, top, S, att ? att + (size_t)b * S * top : nullptr);
    }
    f16 *o2 = v->allocH((size_t)M * top);
    engine_linear(*v, att, v->W + at.ow, v->W + at.ob, o, M, top, top, o2);
    v->copy(x, o2, (size_t)M * top * 2);             // o2 lives above the mark: copy down into x (its previous content is dead)
    v->top = mark;
}

// mid block of either half: resnet, attention, resnet.  in -> o -> x -> the returned buffer: o again, or (training forward: the
// attention's input stays on the tape, do not overwrite it) a new one
static f16 *vmid(ctx_vae *v, const VHalf &p, const f16 *in, f16 *o, f16 *x, int B, int h, int w, int top, void *stats)
{
    vres(v, p.mid[0], in, B, h, w, o, stats);
    vattn(v, p.att, o, x, B, h, w, top, stats);
    if (v->train) o = v->allocH((size_t)B * h * w * top);
    vres(v, p.mid[1], x, B, h, w, o, stats);
    return o;
}

static int vae_run(ctx_vae *v, const float *z, int B, int H, int W, float *img)
{
    const ctx_vae_config_t &c = v->cfg;
    const int n = c.n_levels, top = c.block_out_channels[n - 1], L = c.latent_channels;
    v->begin();
    void *stats = v->alloc((size_t)ctx_groupnorm_ws_bytes(B, c.groups));
    float *zq = (float *)v->alloc((size_t)B * L * H * W * 4);
    VRUN(ctx_pointwise_core(z, v->W + v->pqw, v->W + v->pqb, B, L, (int64_t)H * W, false, zq, v->s));
    int h = H, w = W;
    f16 *x = v->allocH((size_t)B * h * w * top);
    VRUN(ctx_conv_in_core(zq, v->W + v->dec.ciw, v->W + v->dec.cib, B, L, h, w, top, x, v->s));
    f16 *o = v->allocH((size_t)B * h * w * top);
    f16 *cur = vmid(v, v->dec, x, o, x, B, h, w, top, stats);     // the attention's output goes where conv_in's is dead by then
    int cc = top;
    for (int i = 0; i < n; ++i) {
        for (size_t j = 0; j < v->up[i].size(); ++j) {
            int cout = v->up[i][j].cout;
            f16 *nx = v->allocH((size_t)B * h * w * cout);
            vres(v, v->up[i][j], cur, B, h, w, nx, stats);
            cur = nx; cc = cout;
        }
        if (i != n - 1) {
            f16 *nx = v->allocH((size_t)B * (2 * h) * (2 * w) * cc);
            vconv(v, cur, v->upw[i], v->upb[i], nullptr, B, h, w, cc, cc, nx, ConvGeom{1, 1});         // nearest 2x upsample fused
            cur = nx; h *= 2; w *= 2;
        }
    }
    f16 *y = v->allocH((size_t)B * h * w * cc);
    vgn(v, cur, v->dec.cng, v->dec.cnb, B, h * w, cc, 1, y, stats);
    VRUN(ctx_conv_out_core(y, v->W + v->dec.cow, v->W + v->dec.cob, B, h, w, cc, c.out_channels, img, v->s));
    return engine_finish(v, "vae_decode");
}

extern "C" int64_t ctx_vae_workspace_bytes(const ctx_vae_t *cv, int32_t B, int32_t H, int32_t W)
{
    ctx_vae *v = const_cast<ctx_vae *>(cv);
    if (!v || B < 1 || H < 1 || W < 1 || (H * W) % 64) return -1;
    v->train = false;
    engine_dry_run(v, [&] { return vae_run(v, nullptr, B, H, W, nullptr); });
    return engine_workspace_need(v);
}

extern "C" int32_t ctx_vae_decode(ctx_vae_t *v, const float *latents, int32_t B, int32_t H, int32_t W, float *image, ctx_stream_t stream)
{
    CTX_REQUIRE(v && latents && image && v->W && v->ws, "vae_decode: null pointer / not bound");
    CTX_REQUIRE(B >= 1 && H >= 1 && W >= 1 && (H * W) % 64 == 0, "vae_decode: need h*w %% 64 == 0 (B=%d H=%d W=%d)", B, H, W);
    v->s = (hipStream_t)stream; v->dry = false; v->train = false;
    return vae_run(v, latents, B, H, W, image);
}

// image f32 NCHW [B,3,H,W] (H, W multiples of 2^(n-1)) -> moments f32 NCHW [B,2L,H>>(n-1),W>>(n-1)]
static int vae_encode_run(ctx_vae *v, const float *img, int B, int H, int W, float *moments)
{
    const ctx_vae_config_t &c = v->cfg;
    const int n = c.n_levels, top = c.block_out_channels[n - 1], L2 = 2 * c.latent_channels;
    v->begin();
    v->tape = ctx_vae::Tape();
    void *stats = v->alloc((size_t)ctx_groupnorm_ws_bytes(B, c.groups));
    int h = H, w = W, cc = c.block_out_channels[0];
    f16 *cur = v->allocH((size_t)B * h * w * cc);
    VRUN(ctx_conv_in_core(img, v->W + v->enc.ciw, v->W + v->enc.cib, B, c.out_channels, h, w, cc, cur, v->s));
    v->tape.conv_in_out = cur;
    for (int i = 0; i < n; ++i) {
        for (size_t j = 0; j < v->down[i].size(); ++j) {
            int cout = v->down[i][j].cout;
            f16 *nx = v->allocH((size_t)B * h * w * cout);
            vres(v, v->down[i][j], cur, B, h, w, nx, stats);
            cur = nx; cc = cout;
        }
        if (i != n - 1) {
            f16 *nx = v->allocH((size_t)B * (h / 2) * (w / 2) * cc);
            vconv(v, cur, v->dnw[i], v->dnb[i], nullptr, B, h, w, cc, cc, nx, ConvGeom{2, 0, 1});      // stride 2, padding (0,1,0,1)
            cur = nx; h /= 2; w /= 2;
        }
    }
    f16 *o = v->allocH((size_t)B * h * w * top), *x = v->allocH((size_t)B * h * w * top);
    o = vmid(v, v->enc, cur, o, x, B, h, w, top, stats);
    v->tape.norm_out_in = o;
    if (v->train) { v->tape.valid = !v->dry; v->tape.B = B; v->tape.H = H; v->tape.W = W; v->tape.top = v->top; }
    f16 *y = v->allocH((size_t)B * h * w * top);
    vgn(v, o, v->enc.cng, v->enc.cnb, B, h * w, top, 1, y, stats);
    f16 *m16 = v->allocH((size_t)B * h * w * L2);
    vconv(v, y, v->enc.cow, v->enc.cob, nullptr, B, h, w, top, L2, m16);
    VRUN(ctx_pointwise_core(m16, v->W + v->qw, v->W + v->qb, B, L2, (int64_t)h * w, true, moments, v->s));
    return engine_finish(v, "vae_encode");
}

static bool vae_encode_dims_ok(const ctx_vae *v, int B, int H, int W)
{
    const int f = 1 << (v->cfg.n_levels - 1);
    return B >= 1 && H >= f && W >= f && H % f == 0 && W % f == 0 && ((H / f) * (W / f)) % 64 == 0 && v->cfg.latent_channels * 2 % 8 == 0;
}

extern "C" int64_t ctx_vae_encode_workspace_bytes(const ctx_vae_t *cv, int32_t B, int32_t H, int32_t W)
{
    ctx_vae *v = const_cast<ctx_vae *>(cv);
    if (!v || !vae_encode_dims_ok(v, B, H, W)) return -1;
    v->train = false;
    engine_dry_run(v, [&] { return vae_encode_run(v, nullptr, B, H, W, nullptr); });
    return engine_workspace_need(v);
}

extern "C" int32_t ctx_vae_encode(ctx_vae_t *v, const float *image, int32_t B, int32_t H, int32_t W, float *moments, ctx_stream_t stream)
{
    CTX_REQUIRE(v && image && moments && v->W && v->ws, "vae_encode: null pointer / not bound");
    CTX_REQUIRE(vae_encode_dims_ok(v, B, H, W), "vae_encode: need H, W multiples of %d with (H/%d)*(W/%d) %% 64 == 0 and 2*latent_channels %% 8 == 0 (B=%d H=%d W=%d)",
                1 << (v->cfg.n_levels - 1), 1 << (v->cfg.n_levels - 1), 1 << (v->cfg.n_levels - 1), B, H, W);
    v->s = (hipStream_t)stream; v->dry = false; v->train = false;
    return vae_encode_run(v, image, B, H, W, moments);
}

// =====================================================================================================================
// Encoder backward (input gradients only: the VAE is frozen): the link that lets the reference's SDS loss reach the texture
// (`loss.backward()` through `vae.encode(rendered_grid)`, src/training/trainer.py:732, 866).  Every layer's data gradient runs on
// the forward's kernels: conv dgrad = the implicit-GEMM conv on the transposed / flipped weight pack (stride-2 downsamplers: the
// zero-inserted grid, GemmArgs.zins), linear dgrad = the GEMM on W^T, attention = the five products of softmax attention's
// backward as GEMMs around a row kernel (P is recomputed from the taped q, k), GroupNorm(+SiLU) = norm.hip's backward entry.
// Gradients are fp16 with a caller-chosen scale `gscale` (every op is linear in the gradient; the result is divided by it).
// dS = P * (dP - rowsum(dP * P)) * scale, one workgroup per row
__global__ __launch_bounds__(256) void k_softmax_bwd_rows(const f16 *__restrict__ P, const f16 *__restrict__ dP, int n, float scale, f16 *__restrict__ dS)
{
    const f16 *pr = P + (size_t)blockIdx.x * n, *dr = dP + (size_t)blockIdx.x * n;
    f16 *out = dS + (size_t)blockIdx.x * n;
    __shared__ float red[4];
    float dot = 0.f;
    for (int i = threadIdx.x * 8; i < n; i += 2048) {
        f16x8 a = *(const f16x8 *)(pr + i), b = *(const f16x8 *)(dr + i);
#pragma unroll
        for (int j = 0; j < 8; ++j) dot += (float)a[j] * (float)b[j];
    }
    dot = wave_sum(dot);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = dot;
    __syncthreads();
    dot = (red[0] + red[1]) + (red[2] + red[3]);
    for (int i = threadIdx.x * 8; i < n; i += 2048) {
        f16x8 a = *(const f16x8 *)(pr + i), b = *(const f16x8 *)(dr + i), o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (f16)((float)a[j] * ((float)b[j] - dot) * scale);
        *(f16x8 *)(out + i) = o;
    }
}

// quant_conv backward: g f32 NCHW [B,C,hw] -> d(m16) f16 NHWC padded to 64 channels, times gscale
__global__ __launch_bounds__(256) void k_quant_bwd(const float *__restrict__ g, const f16 *__restrict__ w, int B, int C, int64_t HW, float gscale,
                                                   f16 *__restrict__ d)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (int64_t)B * HW; i += (int64_t)gridDim.x * 256) {
        const int bb = (int)(i / HW); const int64_t p = i % HW;
        float in[16];
        for (int o = 0; o < C; ++o) in[o] = g[((int64_t)bb * C + o) * HW + p] * gscale;
        for (int c8 = 0; c8 < 8; ++c8) {
            f16x8 o8 = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int j = 0; j < 8; ++j) {
                const int c = c8 * 8 + j;
                if (c < C) { float acc = 0.f; for (int o = 0; o < C; ++o) acc += in[o] * (float)w[o * C + c]; o8[j] = (f16)acc; }
            }
            *(f16x8 *)(d + i * 64 + c8 * 8) = o8;
        }
    }
}

// conv_in backward: dy f16 NHWC [B,H,W,C] -> d(image) f32 NCHW [B,Cimg,H,W] / gscale; w = the forward pack [C][3][3][8]
__global__ __launch_bounds__(256) void k_conv_in_bwd(const f16 *__restrict__ dy, const f16 *__restrict__ w, int B, int H, int W, int C, int Cimg,
                                                     float inv_gscale, float *__restrict__ dimg)
{
    extern __shared__ float s_w[];                   // [9][Cimg(<=4)][C]
    for (int i = threadIdx.x; i < 9 * 4 * C; i += 256) {
        const int c = i % C, ci = (i / C) % 4, t = i / (4 * C);
        s_w[i] = ci < Cimg ? (float)w[((size_t)c * 9 + t) * 8 + ci] : 0.f;
    }
    __syncthreads();
    const int64_t npix = (int64_t)B * H * W;
    for (int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x; pix < npix; pix += (int64_t)gridDim.x * 256) {
        const int b = (int)(pix / ((int64_t)H * W)), p = (int)(pix % ((int64_t)H * W));
        const int iy = p / W, ix = p % W;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < 9; ++t) {
            // y[oy,ox] += x[oy+ky-1, ox+kx-1] w[ky,kx]  =>  dx[iy,ix] += dy[iy-ky+1, ix-kx+1] w[ky,kx]
            const int oy = iy - t / 3 + 1, ox = ix - t % 3 + 1;
            if (oy < 0 || oy >= H || ox < 0 || ox >= W) continue;
            const f16 *dp = dy + (((size_t)b * H + oy) * W + ox) * C;
            for (int c = 0; c < C; c += 8) {
                const f16x8 dv = *(const f16x8 *)(dp + c);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float d = (float)dv[j];
#pragma unroll
                    for (int ci = 0; ci < 4; ++ci) acc[ci] += d * s_w[(t * 4 + ci) * C + c + j];
                }
            }
        }
        for (int ci = 0; ci < Cimg; ++ci) dimg[(((size_t)b * Cimg + ci) * H + iy) * W + ix] = acc[ci] * inv_gscale;
    }
}

// launch geometry of the three kernels above: the engine's backward and the test seams at the end of this file both take it from here
static unsigned quant_bwd_blocks(int64_t npix) { return (unsigned)cdiv64(npix, 256); }
static unsigned conv_in_bwd_blocks(int64_t npix) { return (unsigned)std::min<int64_t>(cdiv64(npix, 256), 8192); }
static size_t conv_in_bwd_lds(int C) { return (size_t)9 * 4 * C * sizeof(float); }

// a data-gradient conv: the transposed / flipped pack by pointer, no bias
static void vconv_bwd(ctx_vae *v, const f16 *x, size_t wT, int B, int H, int W, int Cin, int Cout, f16 *out, ConvGeom g = ConvGeom())
{
    engine_conv3(*v, x, v->W + wT, nullptr, nullptr, B, H, W, Cin, Cout, out, g);
}
static void vgn_bwd(ctx_vae *v, const f16 *x, const f16 *dy, size_t g, size_t b, const f16 *add, int B, int HW, int C, int silu, f16 *dx, void *gws)
{
    VRUN(ctx_groupnorm_bwd_f16(x, dy, v->W + g, v->W + b, add, B, HW, C, v->cfg.groups, 1e-6f, silu, dx, gws, v->s));
}

// resnet backward: dout [M,cout] -> dx [M,cin] (dx may alias nothing the forward still needs)
static void vres_bwd(ctx_vae *v, const VRes &r, const ctx_vae::ResTape &tp, const f16 *dout, int B, int H, int W, f16 *dx, void *gws)
{
    const size_t M = (size_t)B * H * W;
    size_t mark = v->top;
    f16 *dt2 = v->allocH(M * r.cout);
    vconv_bwd(v, dout, r.c2wT, B, H, W, r.cout, r.cout, dt2);
    f16 *dh = v->allocH(M * r.cout);
    vgn_bwd(v, tp.h, dt2, r.n2g, r.n2b, nullptr, B, H * W, r.cout, 1, dh, gws);
    f16 *dt1 = dt2;                                   // dt2 is dead
    if (r.cin != r.cout) dt1 = v->allocH(M * r.cin);
    vconv_bwd(v, dh, r.c1wT, B, H, W, r.cout, r.cin, dt1);
    const f16 *dsc = dout;
    if (r.cin != r.cout) {
        f16 *s2 = v->allocH(M * r.cin);
        engine_linear(*v, dout, v->W + r.scwT, nullptr, nullptr, (int)M, r.cin, r.cout, s2);
        dsc = s2;
    }
    vgn_bwd(v, tp.x, dt1, r.n1g, r.n1b, dsc, B, H * W, r.cin, 1, dx, gws);
    v->top = mark;
}

// mid-block attention backward: x_out = o + proj(softmax(q k^T / sqrt(top)) v), q|k|v = gn(o) Wqkv^T + b
static void vattn_bwd(ctx_vae *v, const VAttn &at, const f16 *o, const f16 *qkv, const f16 *dx, f16 *d_o, int B, int h, int w, int top, void *gws)
{
    const int S = h * w, M = B * S;
    size_t mark = v->top;
    f16 *datt = v->allocH((size_t)M * top);
    engine_linear(*v, dx, v->W + at.owT, nullptr, nullptr, M, top, top, datt);
    f16 *dqkv = v->allocH((size_t)M * 3 * top);
    f16 *sc = v->allocH((size_t)S * S), *pr = v->allocH((size_t)S * S), *dp = v->allocH((size_t)S * S), *tr = v->allocH((size_t)S * S);
    f16 *qb = v->allocH((size_t)S * top), *kb = v->allocH((size_t)S * top), *vb = v->allocH((size_t)S * top), *tb = v->allocH((size_t)S * top);
    const float scale = 1.0f / sqrtf((float)top);
    for (int b = 0; b < B; ++b) {
        const f16 *base = qkv ? qkv + (size_t)b * S * 3 * top : nullptr;
        const f16 *da = datt ? datt + (size_t)b * S * top : nullptr;
        f16 *dq = dqkv ? dqkv + (size_t)b * S * 3 * top : nullptr;
        vrows(v, base, S, top, qb);
        vrows(v, base ? base + top : nullptr, S, top, kb);
        vrows(v, base ? base + 2 * top : nullptr, S, top, vb);
        vprobs(v, qb, kb, S, top, softmax_scale_log2e(scale), sc, pr);                               // P (recomputed)
        engine_linear(*v, da, vb, nullptr, nullptr, S, S, top, dp);                                 // dP = dAtt V^T
        // dV = P^T dAtt : X = P^T [S,S], Wt = dAtt^T [top,S]
        VRUN(ctx_transpose_v_core(pr, 1, S, S, S / 64, S, tr, v->s));
        VRUN(ctx_transpose_v_core(da, 1, S, top, top / 64, S, tb, v->s));
        engine_linear(*v, tr, tb, nullptr, nullptr, S, top, S, dq ? dq + 2 * top : nullptr, 3 * top);
        ENGINE_LAUNCH(v, k_softmax_bwd_rows, dim3(S), dim3(256), 0, pr, dp, S, scale, sc);          // dS -> sc
        // dQ = dS K : Wt = K^T [top,S]
        VRUN(ctx_transpose_v_core(kb, 1, S, top, top / 64, S, tb, v->s));
        engine_linear(*v, sc, tb, nullptr, nullptr, S, top, S, dq, 3 * top);
        // dK = dS^T Q : X = dS^T, Wt = Q^T
        VRUN(ctx_transpose_v_core(sc, 1, S, S, S / 64, S, tr, v->s));
        VRUN(ctx_transpose_v_core(qb, 1, S, top, top / 64, S, tb, v->s));
        engine_linear(*v, tr, tb, nullptr, nullptr, S, top, S, dq ? dq + top : nullptr, 3 * top);
    }
    f16 *dg = datt;                                    // datt is dead
    engine_linear(*v, dqkv, v->W + at.qkvT, nullptr, nullptr, M, top, 3 * top, dg);
    vgn_bwd(v, o, dg, at.ng, at.nb, dx, B, S, top, 0, d_o, gws);
    v->top = mark;
}

// continues the training forward's run: the arena from the tape's top, the FLOP count on top of the forward's
static int vae_encode_bwd_run(ctx_vae *v, const float *gmom, float gscale, float *dimg)
{
    const ctx_vae_config_t &c = v->cfg;
    const int n = c.n_levels, top = c.block_out_channels[n - 1], L2 = 2 * c.latent_channels;
    const int B = v->tape.B, H = v->tape.H, W = v->tape.W;
    int h = H >> (n - 1), w = W >> (n - 1);
    v->top = v->tape.top; v->rc = 0;
    void *gws = v->alloc((size_t)ctx_groupnorm_bwd_ws_bytes(B, c.groups));
    const size_t Ml = (size_t)B * h * w;
    f16 *dm = v->allocH(Ml * 64);
    ENGINE_LAUNCH(v, k_quant_bwd, dim3(quant_bwd_blocks((int64_t)Ml)), dim3(256), 0, gmom, v->W + v->qw, B, L2, (int64_t)h * w, gscale, dm);
    // two rotating gradient buffers sized for the largest activation of the encoder
    size_t big = 0;
    { int hh = H, ww = W; for (int i = 0; i < n; ++i) { big = std::max(big, (size_t)B * hh * ww * c.block_out_channels[i]); if (i != n - 1) { hh /= 2; ww /= 2; } } }
    f16 *ga = v->allocH(big), *gb = v->allocH(big);
    vconv_bwd(v, dm, v->enc.cowT, B, h, w, 64, top, ga);                                                       // conv_out dgrad -> dy [M,top]
    vgn_bwd(v, v->tape.norm_out_in, ga, v->enc.cng, v->enc.cnb, nullptr, B, h * w, top, 1, gb, gws);
    std::swap(ga, gb);                                                                                         // ga = current gradient
    int ri = (int)v->tape.res.size() - 1;
    auto tape_at = [&](int k) { return v->dry ? ctx_vae::ResTape{nullptr, nullptr} : v->tape.res[k]; };
    vres_bwd(v, v->enc.mid[1], tape_at(ri--), ga, B, h, w, gb, gws); std::swap(ga, gb);
    vattn_bwd(v, v->enc.att, v->tape.attn_in, v->tape.qkv, ga, gb, B, h, w, top, gws); std::swap(ga, gb);
    vres_bwd(v, v->enc.mid[0], tape_at(ri--), ga, B, h, w, gb, gws); std::swap(ga, gb);
    for (int i = n - 1; i >= 0; --i) {
        const int cc = c.block_out_channels[i];
        if (i != n - 1) {
            // downsampler backward: stride-2, pad (0,1,0,1) conv -> zero-inserted 2x grid, flipped weights, offset -2
            vconv_bwd(v, ga, v->dnwT[i], B, h, w, cc, cc, gb, ConvGeom{1, 1, -1, 1});
            std::swap(ga, gb); h *= 2; w *= 2;
        }
        for (int j = (int)v->down[i].size() - 1; j >= 0; --j) { vres_bwd(v, v->down[i][j], tape_at(ri--), ga, B, h, w, gb, gws); std::swap(ga, gb); }
    }
    const int C0 = c.block_out_channels[0];
    ENGINE_LAUNCH(v, k_conv_in_bwd, dim3(conv_in_bwd_blocks((int64_t)B * H * W)), dim3(256), conv_in_bwd_lds(C0),
                  ga, v->W + v->enc.ciw, B, H, W, C0, c.out_channels, 1.0f / gscale, dimg);
    return engine_finish(v, "vae_encode_bwd");
}

extern "C" int64_t ctx_vae_encode_train_workspace_bytes(const ctx_vae_t *cv, int32_t B, int32_t H, int32_t W)
{
    ctx_vae *v = const_cast<ctx_vae *>(cv);
    if (!v || !vae_encode_dims_ok(v, B, H, W)) return -1;
    v->train = true;
    engine_dry_run(v, [&] {                          // forward, then the backward on top of its tape: the peak is the larger of the two
        vae_encode_run(v, nullptr, B, H, W, nullptr);
        v->tape.B = B; v->tape.H = H; v->tape.W = W;
        return vae_encode_bwd_run(v, nullptr, 1.0f, nullptr);
    });
    v->train = false; v->tape.valid = false;
    return engine_workspace_need(v);
}

extern "C" int32_t ctx_vae_encode_train(ctx_vae_t *v, const float *image, int32_t B, int32_t H, int32_t W, float *moments, ctx_stream_t stream)
{
    CTX_REQUIRE(v && image && moments && v->W && v->ws, "vae_encode_train: null pointer / not bound");
    CTX_REQUIRE(vae_encode_dims_ok(v, B, H, W), "vae_encode_train: need H, W multiples of %d with (H/f)*(W/f) %% 64 == 0 (B=%d H=%d W=%d)",
                1 << (v->cfg.n_levels - 1), B, H, W);
    v->s = (hipStream_t)stream; v->dry = false; v->train = true;
    int rc = vae_encode_run(v, image, B, H, W, moments);
    v->train = false;
    if (rc) v->tape.valid = false;
    return rc;
}

extern "C" int32_t ctx_vae_encode_bwd(ctx_vae_t *v, const float *grad_moments, float gscale, float *grad_image, ctx_stream_t stream)
{
    CTX_REQUIRE(v && grad_moments && grad_image && v->W && v->ws, "vae_encode_bwd: null pointer / not bound");
    CTX_REQUIRE(v->tape.valid, "vae_encode_bwd: no tape (call ctx_vae_encode_train first; any other call on this handle drops the tape)");
    CTX_REQUIRE(gscale > 0.f, "vae_encode_bwd: gscale must be positive");
    v->s = (hipStream_t)stream; v->dry = false;
    int rc = vae_encode_bwd_run(v, grad_moments, gscale, grad_image);
    v->tape.valid = false;
    return rc;
}

/* GEMM and convolution FLOPs of the last run (a training forward's count carries on through its backward) */
extern "C" double ctx_vae_flops(const ctx_vae_t *v) { return v ? v->flops[0] : 0.0; }

// ---- test seams: the row kernels and the two ends of the encoder backward alone, launched as the engine launches them -------------
extern "C" int32_t ctx_softmax_rows_f16(const void *s, int32_t rows, int32_t n, float scale, void *p, ctx_stream_t stream)
{
    CTX_REQUIRE(s && p, "softmax_rows: null pointer");
    CTX_REQUIRE(rows > 0 && n > 0 && n % 8 == 0, "softmax_rows: need n %% 8 == 0 (rows=%d n=%d)", rows, n);
    hipLaunchKernelGGL(k_softmax_rows, dim3(rows), dim3(256), 0, (hipStream_t)stream, (const f16 *)s, n, softmax_scale_log2e(scale), (f16 *)p);
    CTX_CHECK_LAUNCH("softmax_rows");
    return CTX_OK;
}
extern "C" int32_t ctx_pointwise_f32(const void *x, const void *w, const void *b, int32_t B, int32_t C, int64_t HW, int32_t nhwc16, float *y,
                                     ctx_stream_t stream)
{
    CTX_REQUIRE((int64_t)B * HW <= 0xffffffffll * 256, "pointwise: B * HW exceeds the grid");
    return ctx_pointwise_core(x, (const f16 *)w, (const f16 *)b, B, C, HW, nhwc16 != 0, y, (hipStream_t)stream);
}
extern "C" int32_t ctx_softmax_bwd_rows_f16(const void *P, const void *dP, int32_t rows, int32_t n, float scale, void *dS, ctx_stream_t stream)
{
    CTX_REQUIRE(P && dP && dS, "softmax_bwd_rows: null pointer");
    CTX_REQUIRE(rows > 0 && n > 0 && n % 8 == 0, "softmax_bwd_rows: need n %% 8 == 0 (rows=%d n=%d)", rows, n);
    hipLaunchKernelGGL(k_softmax_bwd_rows, dim3(rows), dim3(256), 0, (hipStream_t)stream, (const f16 *)P, (const f16 *)dP, n, scale, (f16 *)dS);
    CTX_CHECK_LAUNCH("softmax_bwd_rows");
    return CTX_OK;
}
extern "C" int32_t ctx_quant_bwd_f16(const float *g, const void *w, int32_t B, int32_t C, int64_t HW, float gscale, void *d, ctx_stream_t stream)
{
    CTX_REQUIRE(g && w && d, "quant_bwd: null pointer");
    CTX_REQUIRE(B > 0 && HW > 0 && C > 0 && C <= 16 && (int64_t)B * HW < (1ll << 31), "quant_bwd: need 1 <= C <= 16 (B=%d C=%d HW=%lld)", B, C, (long long)HW);
    hipLaunchKernelGGL(k_quant_bwd, dim3(quant_bwd_blocks((int64_t)B * HW)), dim3(256), 0, (hipStream_t)stream, g, (const f16 *)w, B, C, HW, gscale, (f16 *)d);
    CTX_CHECK_LAUNCH("quant_bwd");
    return CTX_OK;
}
extern "C" int32_t ctx_conv_in_bwd_f16(const void *dy, const void *w_pack, int32_t B, int32_t H, int32_t W, int32_t C, int32_t Cimg, float inv_gscale,
                                       float *dimg, ctx_stream_t stream)
{
    CTX_REQUIRE(dy && w_pack && dimg, "conv_in_bwd: null pointer");
    CTX_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && Cimg >= 1 && Cimg <= 4 && conv_in_bwd_lds(C) <= 64 * 1024 &&
                    (int64_t)B * H * W * C < (1ll << 31),
                "conv_in_bwd: need C %% 8 == 0, C <= 448, 1 <= Cimg <= 4 (B=%d H=%d W=%d C=%d Cimg=%d)", B, H, W, C, Cimg);
    hipLaunchKernelGGL(k_conv_in_bwd, dim3(conv_in_bwd_blocks((int64_t)B * H * W)), dim3(256), conv_in_bwd_lds(C), (hipStream_t)stream, (const f16 *)dy,
                       (const f16 *)w_pack, B, H, W, C, Cimg, inv_gscale, dimg);
    CTX_CHECK_LAUNCH("conv_in_bwd");
    return CTX_OK;
}
