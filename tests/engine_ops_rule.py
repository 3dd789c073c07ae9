"""The definition of the engines' small ops, one by one: the kernels of the UNet / ControlNet / VAE graphs that are neither a GEMM,
attention nor a norm (elementwise.hip, k_gemv_f16 of gemm.hip, k_conv_small / k_add_scaled_f16 of unet.hip, k_pointwise of vae.hip, the
forward packs of engine.hip).  For every op: the float64 reference computed from the inputs as the kernel sees them (fp16-rounded where
the kernel rounds, conv_in's and conv_small's (f16)x of their f32 image included), the per-element error bound, and the cases, seeds and
input generators that the CPU and the GPU tests share.
Not a test module: tests/test_engine_ops_cpu.py and tests/test_engine_ops_gpu.py import it.

Where the bounds come from (u10 = 2^-10, u23 = 2^-23, u24 = 2^-24; S = the sum of the absolute values of an element's products plus
|bias|; a sequential or tree fp32 sum of n terms is off by at most gamma_n S <= n u24 S (1 + ..) <= n u23 S):
  conv_in, conv_small   fp16 output of an fp32 sum of n = 9 Cin + 1 terms: u10 |want| + n u23 S + u24 (u24: an fp16 subnormal result).
                        conv_small with SiLU: the whole bound times 1.1, SiLU's slope being at most 1.0998.
  conv_out, pointwise   fp32 output, n = 9 C + 1 or C + 1 terms: n u23 S.
  gemv                  fp16 output of a K-term fp32 sum, optional __expf SiLU on either side: f u10 S + u24 with S over
                        silu(x_k) w_nk when silu_in, f = 1.1 with silu_out (slope again; |silu(v)| <= |v| <= S) and 1 otherwise.  One
                        u11 S is the final rounding, the other covers the fp32 sum (K u24 <= u11 for K <= 8192, asserted in
                        gemv_ref) and __expf.
  add_scaled            u10 |want| + u24: one fp32 fused multiply-add, one fp16 rounding.
  time_embed            u10 + |t| 2^-21: the fp16 rounding of a value of at most 1, plus (slope of sin / cos <= 1) the error of the
                        fp32 argument t f_i, at most 8 fp32 ulps of it: f_i = expf(-ln(1e4) i / h) carries the roundings of the
                        constant, the product and the quotient in an exponent of at most 9.21, then expf's and the product's own.
                        The kernel embeds ONE timestep, t[0], and writes it to each of the B rows.
  transpose_v, concat_f16 / _f32, f16_to_f32, every pack   bit-equal (a pack to the round-to-nearest-even fp16 of the permuted tensor,
                        its padding columns exactly zero; transpose_v's keys S .. Sp exactly zero).
  f32_to_f16            bit-equal to torch's .half() (NaN: NaN-ness), on subnormals, halfway cases, values that round to inf and +-0.

The GEGLU packs (k_pack_geglu): source [2 C4 (, K)] holds the C4 value rows, then the C4 gate rows (diffusers' GEGLU chunks its
projection in that order).  Packed row p, in blocks of 64: blk = p / 64, w = p % 64; w < 32 takes value row 32 blk + w, w >= 32 takes
gate row C4 + 32 blk + (w - 32): 32 value rows, then their 32 gate rows, so that a 64-wide wave tile of the GEMM holds both halves.

What conv_out's listed cases reach: the weights are staged as fp32 when the fp32 copy fits 64 KiB of LDS, Cout C <= 1820, else as fp16.
Of the listed (C, Cout) only (512, 4) is past that, so NU = 12 is the one unroll that ever meets fp16 staging: NU = 3 / 6 need C <= 168 /
336, and Cout <= 4 keeps Cout C <= 1344 there.

Largest max error / bound seen on an MI355X, per op (the GPU tests print it for every case):
  conv_in 0.496   conv_small 0.485   add_scaled 0.500     the fp16 rounding alone is half of these bounds
  conv_out 0.003  pointwise 0.250    gemv 0.129 (0.129 / 0.092 at the UNet's own two shapes, both with the __expf SiLU)
  time_embed 0.249 (t = 1; 0.17 .. 0.20 at t = 500.5 and 999)
"""
import math
import torch
import torch.nn.functional as F

from vae_train_rule import ratio, assert_within, nhwc, nchw, f64, U10, U23, U24        # noqa: F401  (one definition of the gate)

f32, f16 = torch.float32, torch.float16
LN1E4 = math.log(10000.0)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    """the bit patterns of an f16 / f32 tensor, for bit-equality"""
    return t.contiguous().view(torch.int16 if t.dtype == f16 else torch.int32)


def silu64(v):
    return v * torch.sigmoid(v)


# ---- 3x3 convolutions -------------------------------------------------------------------------------------------------------------
def conv3_ref(x, w, bias, stride=1):
    """x [B,Cin,H,W], w [Cout,Cin,3,3], bias [Cout], all taken as float64 -> (want, S) [B,Cout,Ho,Wo]: padding 1, Ho = (H - 1) / stride + 1"""
    x, w, bias = x.to(f64), w.to(f64), bias.to(f64)
    return F.conv2d(x, w, bias, stride=stride, padding=1), F.conv2d(x.abs(), w.abs(), bias.abs(), stride=stride, padding=1)


def conv_weight(Cout, Cin, g):
    """f16 [Cout,Cin,3,3], randn / sqrt(9 Cin)"""
    return (torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5).half()


def pack_conv3_ref(w, pad=None):
    """[Cout,Cin,3,3] -> f16 [Cout][3][3][pad or Cin], channels last, exactly zero beyond Cin"""
    Cout, Cin = w.shape[:2]
    out = torch.zeros(Cout, 3, 3, pad or Cin, dtype=f16)
    out[..., :Cin] = w.half().permute(0, 2, 3, 1)
    return out


def conv_in_pad(Cin):
    return 16 if Cin > 8 else 8


# conv_in (B, Cin, H, W, Cout).  Cin 1 .. 16: the six instantiations <8,3> <8,4> <8,5> <8,8> <16,9> <16,16> and their masked c < Cin lanes.
# Cout 8: 15 idle grid.y slices; 320: o8_per = 3, a short last slice; 1152: o8_per = 9, the ng = 8 then 1 patch loop.  Grids: fewer than
# 256 pixels; a block spanning the batch boundary; all-border rows / columns; an exact multiple of 256.
CONV_IN_CASES = [
    (1, 1, 5, 7, 8), (2, 3, 9, 13, 64), (1, 4, 1, 300, 320), (1, 5, 300, 1, 512), (3, 7, 16, 16, 1152), (2, 8, 9, 13, 320),
    (1, 9, 5, 7, 512), (2, 12, 9, 13, 64), (1, 16, 5, 7, 320), (2, 16, 9, 13, 512), (1, 8, 5, 7, 1152),
]
CONV_IN_REFUSED = [(1, 17, 4, 4, 8), (1, 0, 4, 4, 8), (1, 32, 4, 4, 8)]


def conv_in_inputs(case):
    """-> x f32 [B,Cin,H,W] (not fp16-representable: the kernel's (f16)x is part of the op), w f16 [Cout,Cin,3,3], bias f16 [Cout]"""
    B, Cin, H, W, Cout = case
    g = gen(11000 + 131 * Cin + H * W + Cout)
    return torch.randn(B, Cin, H, W, generator=g), conv_weight(Cout, Cin, g), torch.randn(Cout, generator=g).half()


def conv_in_ref(x, w, bias):
    """-> (want, bound) NHWC [B,H,W,Cout]"""
    want, S = conv3_ref(x.half(), w, bias)
    return nhwc(want), nhwc(U10 * want.abs() + (9 * x.shape[1] + 1) * U23 * S + U24)


# conv_out (B, H, W, C, Cout).  C 8, 24, 128, 320, 512: 9, 27, 144, 360, 576 items, NU = 3, 3, 3, 6, 12 with masked lanes in each; the
# last grid has more than 8192 pixels: waves take a second, prefetched pixel.
CONV_OUT_CASES = [
    (1, 1, 1, 8, 1), (1, 3, 5, 24, 3), (2, 7, 9, 128, 4), (1, 1, 70, 320, 4), (1, 70, 1, 512, 4), (2, 7, 9, 512, 3), (1, 3, 5, 320, 1),
    (1, 92, 93, 16, 4),
]
CONV_OUT_REFUSED = [(1, 4, 4, 8, 0), (1, 4, 4, 8, 5), (1, 4, 4, 12, 4)]


def conv_out_inputs(case):
    """-> x f16 [B,C,H,W], w f16 [Cout,C,3,3], bias f16 [Cout]"""
    B, H, W, Cc, Cout = case
    g = gen(12000 + H * W + 7 * Cc + Cout)
    return torch.randn(B, Cc, H, W, generator=g).half(), conv_weight(Cout, Cc, g), torch.randn(Cout, generator=g).half()


def conv_out_ref(x, w, bias):
    """-> (want, bound) NCHW [B,Cout,H,W]"""
    want, S = conv3_ref(x, w, bias)
    return want, (9 * x.shape[1] + 1) * U23 * S


# conv_small: the layers of ControlNet's conditioning embedding (Cin, Cout, stride, f32 NCHW input?) on two grids; odd H / W at stride 2;
# (12, 16): an f16 input whose channel count is no multiple of 8 (the scalar loop)
CONV_SMALL_LAYERS = [(3, 16, 1, True), (16, 32, 2, False), (32, 96, 2, False), (96, 96, 1, False), (12, 16, 1, False)]
CONV_SMALL_GRIDS = [(1, 9, 13), (2, 8, 8)]
# (B, H, W, Cin, Cout, stride, from_f32, silu): every layer on both grids, SiLU on for one and off for the other
CONV_SMALL_CASES = [(B, H, W, ci, co, st, f32in, (li + gi) % 2)
                    for li, (ci, co, st, f32in) in enumerate(CONV_SMALL_LAYERS) for gi, (B, H, W) in enumerate(CONV_SMALL_GRIDS)]


def conv_small_inputs(case):
    """-> x [B,Cin,H,W] (f32 when from_f32, else f16), w f16 [Cout,Cin,3,3], bias f16"""
    B, H, W, Cin, Cout, stride, from_f32, silu = case
    g = gen(13000 + H * W + 5 * Cin + Cout)
    x = torch.randn(B, Cin, H, W, generator=g)
    return (x if from_f32 else x.half()), conv_weight(Cout, Cin, g), torch.randn(Cout, generator=g).half()


def conv_small_ref(x, w, bias, stride, silu):
    """-> (want, bound) NHWC [B,Ho,Wo,Cout]"""
    pre, S = conv3_ref(x.half(), w, bias, stride)
    want = silu64(pre) if silu else pre
    bound = U10 * want.abs() + (9 * x.shape[1] + 1) * U23 * S + U24
    return nhwc(want), nhwc(1.1 * bound if silu else bound)


# ---- pointwise (the VAE's quant / post-quant convolutions) ---------------------------------------------------------------------------
# (nhwc16, B, C, HW): f32 NCHW input with C in 4, 8; f16 NHWC input with C in 8, 16; HW around the 256-pixel block
POINTWISE_CASES = [(0, 1, 4, 1), (0, 2, 8, 255), (0, 1, 8, 257), (0, 2, 4, 257), (1, 1, 8, 1), (1, 2, 16, 255), (1, 1, 16, 257), (1, 2, 8, 257)]
POINTWISE_REFUSED = [(0, 1, 9, 8), (1, 1, 17, 8), (0, 1, 0, 8)]


def pointwise_inputs(case):
    """-> x [B,C,HW] (f32, or f16 for the NHWC form: the test transposes it), w f16 [C,C], b f16 [C]"""
    nh, B, Cc, HW = case
    g = gen(14000 + 1000 * nh + 17 * Cc + HW)
    x = torch.randn(B, Cc, HW, generator=g)
    return (x.half() if nh else x), (torch.randn(Cc, Cc, generator=g) / Cc ** 0.5).half(), torch.randn(Cc, generator=g).half()


def pointwise_ref(x, w, b):
    """-> (want, bound) [B,C,HW]: the f32 form reads x unrounded"""
    x, w, b = x.to(f64), w.to(f64), b.to(f64)
    want = torch.einsum("oc,bcp->bop", w, x) + b[None, :, None]
    S = torch.einsum("oc,bcp->bop", w.abs(), x.abs()) + b.abs()[None, :, None]
    return want, (x.shape[1] + 1) * U23 * S


# ---- gemv -----------------------------------------------------------------------------------------------------------------------------
# (Bm, N, K, silu_in, silu_out, bias).  K 2056: a second K block of one chunk; 320 / 1280: lanes past K clamped and masked; N odd: the
# wave's second feature clamped; Bm 5, 9: a second / third pass of four rows; (2, 1280, 320) and (2, 1280, 1280) are the UNet's own.
GEMV_CASES = [
    (1, 1, 8, 0, 0, True), (2, 2, 320, 0, 1, True), (4, 7, 1280, 1, 0, True), (5, 8, 2048, 1, 1, True), (9, 9, 2056, 0, 0, False),
    (2, 1280, 320, 0, 1, True), (2, 1280, 1280, 1, 1, True),
]
GEMV_REFUSED = [(1, 0, 8), (1, -3, 8), (0, 4, 8), (1, 4, 12), (1, 4, 0)]          # (Bm, N, K)


def gemv_inputs(case):
    """-> x f16 [Bm,K], w f16 [N,K] (randn / sqrt(K)), bias f16 [N] or None"""
    Bm, N, K, si, so, hb = case
    g = gen(15000 + 31 * Bm + 7 * N + K)
    x = torch.randn(Bm, K, generator=g).half()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).half()
    return x, w, (torch.randn(N, generator=g).half() if hb else None)


def gemv_ref(x, w, bias, silu_in, silu_out):
    """-> (want, bound) [Bm,N]"""
    K = x.shape[1]
    assert K * U24 <= 2.0 ** -11, "the bound's second u11 S covers the fp32 sum only up to K = 8192"
    a = silu64(x.to(f64)) if silu_in else x.to(f64)
    pre, S = a @ w.to(f64).T, a.abs() @ w.to(f64).abs().T
    if bias is not None:
        pre, S = pre + bias.to(f64), S + bias.to(f64).abs()
    return (silu64(pre) if silu_out else pre), (1.1 if silu_out else 1.0) * U10 * S + U24


# ---- add_scaled ---------------------------------------------------------------------------------------------------------------------
ADD_SCALED_CAP = 8 * 4096 * 256                                   # elements one sweep of the capped grid covers
ADD_SCALED_CASES = [(8, 1.0), (2048, 0.37), (2048, 0.0), (8, 0.37), (ADD_SCALED_CAP + 8, 0.37), (2048, 1.0)]
ADD_SCALED_REFUSED = [0, 12, -8]


def add_scaled_inputs(case):
    n, scale = case
    g = gen(16000 + n % 9973)
    return torch.randn(n, generator=g).half(), torch.randn(n, generator=g).half()


def add_scaled_ref(dst, src, scale):
    """scale as the kernel holds it, an fp32 number"""
    want = dst.to(f64) + float(torch.tensor(scale, dtype=f32)) * src.to(f64)
    return want, U10 * want.abs() + U24


# ---- time embedding -------------------------------------------------------------------------------------------------------------------
TIME_EMBED_CASES = [(1, 2, 0.0), (3, 64, 1.0), (1, 320, 500.5), (3, 322, 999.0), (1, 64, 999.0), (3, 320, 0.0), (1, 322, 1.0), (3, 2, 500.5)]   # (B, dim, t)
TIME_EMBED_REFUSED = [(1, 3), (1, 0), (0, 8)]                                                                      # (B, dim)


def time_embed_ref(B, dim, t):
    """diffusers' get_timestep_embedding(flip_sin_to_cos=True, freq_shift=0), downscale_freq_shift 0, in float64 -> (want, bound) [B,dim]"""
    h = dim // 2
    a = float(t) * torch.exp(-LN1E4 * torch.arange(h, dtype=f64) / h)
    want = torch.cat([torch.cos(a), torch.sin(a)]).expand(B, dim).contiguous()
    return want, torch.full_like(want, U10 + abs(float(t)) * 2.0 ** -21)


# ---- the bit-exact movers ---------------------------------------------------------------------------------------------------------------
# transpose_v (B, S, ld, heads, Sp, column offset): ld is the row length of the tensor V is a column slice of
TRANSPOSE_V_CASES = [(1, 64, 64, 1, 64, 0), (2, 100, 3 * 192, 3, 104, 2 * 192), (1, 100, 192, 3, 128, 0), (1, 130, 64, 1, 136, 0)]
TRANSPOSE_V_REFUSED = [(1, 100, 64, 1, 100, 0), (1, 100, 64, 1, 96, 0), (1, 64, 68, 1, 64, 0)]     # Sp % 8, Sp < S, ld % 8


def transpose_v_inputs(case):
    B, S, ld, heads, Sp, off = case
    return torch.randn(B, S, ld, generator=gen(17000 + S + ld)).half()


def transpose_v_ref(v, heads, Sp, off):
    """-> vt f16 [B,heads,64,Sp]: vt[b,h,d,s] = v[b,s,off + 64 h + d], exactly zero for s >= S"""
    B, S, _ = v.shape
    vt = torch.zeros(B, heads, 64, Sp, dtype=f16)
    vt[..., :S] = v[:, :, off:off + heads * 64].reshape(B, S, heads, 64).permute(0, 2, 3, 1)
    return vt


CONCAT_F16_CASES = [(1, 8, 8), (77, 320, 640), (300, 1280, 8)]          # (M, Ca, Cb)
CONCAT_F32_CASES = [(5, 4, 12), (77, 320, 640)]
CONCAT_REFUSED = [(4, 12, 8), (4, 8, 4), (0, 8, 8)]


def concat_inputs(case, dtype):
    M, Ca, Cb = case
    g = gen(18000 + M + Ca + Cb)
    return torch.randn(M, Ca, generator=g).to(dtype), torch.randn(M, Cb, generator=g).to(dtype)


F32_TO_F16_SIZES = [1, 1000, 2048 * 256 + 300]                         # one lane; a ragged block; past the grid cap of 2048 blocks
F16_TO_F32_SIZES = [8, 2048 + 8, 8 * 4096 * 256 + 8]                    # one lane; ragged; one vector past the grid cap of 4096 blocks


def f32_specials():
    """fp16 subnormals and their halfway points, halfway cases of the normal range (ties to even both ways), the overflow threshold,
    fp32 subnormals, +-0, +-inf, NaN"""
    p = [0.0, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20), 2.0 ** -24, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 3e-8, 6e-8, 1023.5 * 2.0 ** -24,
         2.0 ** -14, 2.0 ** -14 * (1 + 2.0 ** -11), 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -23, 1.0 + 2.0 ** -11 - 2.0 ** -24,
         2047.0, 2049.0, 2051.0, 65504.0, 65519.0, 65519.996, 65520.0, 65536.0, 1e5, 3e38, 1e-40, 1.4e-45, float("inf")]
    v = torch.tensor(p + [-a for a in p] + [float("nan")], dtype=f32)
    return v


def f32_to_f16_inputs(n):
    g = gen(19000 + n % 9973)
    x = torch.randn(n, generator=g) * torch.pow(2.0, torch.randint(-28, 18, (n,), generator=g).float())
    sp = f32_specials()
    k = min(n, sp.numel())
    x[:k] = sp[:k] if n >= sp.numel() else sp[-k:]
    return x


def f16_to_f32_inputs(n):
    """every fp16 bit pattern in turn (subnormals, infinities and NaNs among them)"""
    return (torch.arange(n, dtype=torch.int32) % 65536).to(torch.int16).view(f16)


def same_bits_or_nan(got, want):
    """bit-equal, except that a NaN only has to be a NaN"""
    nan = torch.isnan(want)
    return bool((torch.isnan(got) == nan).all()) and bool((bits(got)[~nan] == bits(want)[~nan]).all())


# ---- the forward packs -----------------------------------------------------------------------------------------------------------------
PK_COPY, PK_CONV3, PK_CONVIN, PK_GEGLU_W, PK_GEGLU_B = range(5)
# (kind, a, b): copy a x b elements; conv3 / conv_in Cout = a, Cin = b (conv_in pads 4, 5 -> 8 and 9 -> 16); GEGLU C4 = a, K = b
PACK_CASES = [(PK_COPY, 1000, 0), (PK_COPY, 77, 13), (PK_CONV3, 64, 64), (PK_CONV3, 8, 3), (PK_CONVIN, 16, 4), (PK_CONVIN, 16, 5), (PK_CONVIN, 24, 9),
              (PK_GEGLU_W, 64, 16), (PK_GEGLU_W, 320, 40), (PK_GEGLU_B, 64, 0), (PK_GEGLU_B, 320, 0)]
PACK_REFUSED = [(PK_CONVIN, 8, 17), (PK_CONVIN, 8, 0), (PK_GEGLU_W, 48, 8), (PK_GEGLU_B, 16, 0), (5, 8, 8), (-1, 8, 8)]


def pack_inputs(case):
    """-> the fp32 parameter in diffusers' layout"""
    kind, a, b = case
    g = gen(20000 + 100 * kind + a + b)
    shape = {PK_COPY: (a * max(b, 1),), PK_CONV3: (a, b, 3, 3), PK_CONVIN: (a, b, 3, 3), PK_GEGLU_W: (2 * a, b), PK_GEGLU_B: (2 * a,)}[kind]
    return torch.randn(*shape, generator=g)


def geglu_rows(C4):
    """source row of every packed row (the interleave stated in the module docstring)"""
    p = torch.arange(2 * C4)
    blk, w = p // 64, p % 64
    return torch.where(w < 32, blk * 32 + w, C4 + blk * 32 + (w - 32))


def pack_ref(case, src):
    """-> the f16 pack, flat"""
    kind, a, b = case
    if kind == PK_COPY:
        return src.half().reshape(-1)
    if kind in (PK_CONV3, PK_CONVIN):
        return pack_conv3_ref(src, conv_in_pad(b) if kind == PK_CONVIN else None).reshape(-1)
    return src[geglu_rows(a)].half().reshape(-1)
