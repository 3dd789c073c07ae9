"""The definition of the VAE encoder's training-path ops, one by one ("VAE encoder backward"): for every op the
float64 reference computed from the fp16-rounded inputs (through torch.autograd where a gradient is meant), the per-element error
bound, and the shapes, seeds and inputs that the CPU and the GPU tests share.
Not a test module: tests/test_vae_train_ops_cpu.py and tests/test_vae_train_ops_gpu.py import it.

Where the bounds come from (u16 = 2^-11, the unit roundoff of fp16; u32 = 2^-24):
  convolutions   the project's own conv gate, |err| <= 4e-3 + 3e-3 |want| (`_close(rtol=3e-3, atol=4e-3)` of test_conv3x3), with that
                 test's scaling: weights randn / sqrt(9 Cin) of the forward layer, unit activations and cotangents.
  GroupNorm bwd  dx = rstd (du - c1 - x^ c2) + add is rounded to fp16 once: u16 |dx| <= u16 T with T = rstd (|du| + |c1| + |x^ c2|) +
                 |add|.  The bound is 2^-10 T + 1e-7: the second u16 T is far more than the fp32 sums and __expf cost (~1e-6 T).
  softmax rows   p is rounded once (u16 p; 2^-25 absolute where p is an fp16 subnormal): 2^-10 p + 2^-24.  Backward
                 dS = scale P (dP - sum_j P_j dP_j): 2^-10 scale P (|dP| + sum_j |P_j dP_j|) + 2^-24, P the fp16 tensor the kernel is given.
  quant_bwd      fp16 output of a C-term fp32 sum: 2^-10 gscale sum_o |g_o w_oc|; the padded channels are exactly 0.
  conv_in_bwd    fp32 output of a 9C-term sequential fp32 sum: gamma_n <= n 2^-23 for n = 9C: 9C 2^-23 inv_gscale sum |dy w|.
  packs          bit-equal to the fp16 rounding (round to nearest even) of the permuted tensor, exactly zero in the pad columns."""
import torch
import torch.nn.functional as F

f64 = torch.float64
U10, U23, U24 = 2.0 ** -10, 2.0 ** -23, 2.0 ** -24
GN_EPS = 1e-6
GNB_MAX_SPLITS = 128


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def nhwc(t):
    """[B,C,H,W] -> contiguous [B,H,W,C]"""
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def ratio(got, want, bound):
    """max over the elements of |got - want| / bound (0 / 0 counts as 0, x / 0 as inf) and its flat index"""
    err = (got.to(f64) - want.to(f64)).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.to(f64).expand_as(err))
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    i = int(r.argmax())
    return float(r.flatten()[i]), i


def assert_within(got, want, bound, what):
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    assert torch.isfinite(got.to(f64)).all(), f"{what}: non-finite output"
    r, i = ratio(got, want, bound)
    print(f"{what}: max error / bound {r:.3f}")
    assert r <= 1.0, (f"{what}: element {i} is at {r:.3f} of its bound (got {float(got.flatten()[i]):.6g}, want "
                      f"{float(want.flatten()[i]):.6g}, bound {float(bound.expand_as(want).flatten()[i]):.3g})")


# ---- convolutions ---------------------------------------------------------------------------------------------------------------
def conv_bound(want):
    return 4e-3 + 3e-3 * want.abs()


# downsampler forward (stride 2, poff 1): (B, H, W, Cin, Cout)
DOWN_CASES = [(2, 16, 12, 64, 128), (1, 10, 14, 128, 64)]
# stride-1 dgrad: cotangent (B, H, W), forward Cout -> forward Cin, pad (the cotangent's channel count; > Cout: conv_out's case)
DGRAD1_CASES = [(2, 16, 12, 128, 64, 128), (1, 9, 13, 64, 128, 64), (2, 8, 8, 8, 64, 64)]
# stride-2 dgrad (ups 1, zins 1, poff -1): cotangent (B, h, w), forward Cout -> forward Cin; dx is (B, 2h, 2w, Cin)
DGRAD2_CASES = [(2, 8, 6, 128, 64), (1, 5, 7, 64, 64)]
# shapes whose (M, N, K, stride 2 | upsample) is a key of the tuned plan table (gemm_tuned.h), which knows neither poff nor zins: the
# planner hands these two geometries a UNet layer's tile and split-K factor (M 512, N 320, K 2880, stride 2; M 128, N 1280, K 11520, x2)
DOWN_PLAN_CASES = [(2, 32, 32, 320, 320)]
DGRAD2_PLAN_CASES = [(2, 4, 4, 1280, 1280)]


# stride 1 with poff 1 (rows and columns y .. y + 2: F.pad(x, (0,2,0,2)), no diffusers meaning): a geometry the halo-staged kernel
# does not have, at a shape it would otherwise take (H, W multiples of 16): (B, H, W, Cin, Cout)
OFFSET1_CASE = (1, 16, 16, 64, 64)


def offset1_inputs(case):
    B, H, W, Cin, Cout = case
    g = _gen(1500 + H * W + Cin)
    return torch.randn(B, Cin, H, W, generator=g).half(), conv_weight(Cout, Cin, 1501 + Cin).half(), torch.randn(Cout, generator=g).half()


def offset1_ref(x, w, bias):
    return F.conv2d(F.pad(x.to(f64), (0, 2, 0, 2)), w.to(f64), bias.to(f64))


def conv_weight(Cout, Cin, seed):
    """fp32 [Cout,Cin,3,3], randn / sqrt(9 Cin); the kernels see its fp16 rounding"""
    return torch.randn(Cout, Cin, 3, 3, generator=_gen(seed)) / (9 * Cin) ** 0.5


def down_inputs(case):
    B, H, W, Cin, Cout = case
    g = _gen(1000 + H * W + Cin)
    x = torch.randn(B, Cin, H, W, generator=g).half()
    w = conv_weight(Cout, Cin, 1001 + Cin).half()
    bias = torch.randn(Cout, generator=g).half()
    res = torch.randn(B, Cout, H // 2, W // 2, generator=g).half()
    return x, w, bias, res


def down_ref(x, w, bias, res=None):
    """diffusers' Downsample2D of the VAE: F.pad(x, (0,1,0,1)), stride-2 conv, no padding"""
    y = F.conv2d(F.pad(x.to(f64), (0, 1, 0, 1)), w.to(f64), bias.to(f64) if bias is not None else None, stride=2)
    return y + res.to(f64) if res is not None else y


def dgrad1_inputs(case):
    """-> dy [B,pad,H,W] f16 (channels >= Cout zero, as k_quant_bwd writes them), w fp32 [Cout,Cin,3,3]"""
    B, H, W, Cout, Cin, pad = case
    dy = torch.zeros(B, pad, H, W)
    dy[:, :Cout] = torch.randn(B, Cout, H, W, generator=_gen(2000 + H * W + Cout))
    return dy.half(), conv_weight(Cout, Cin, 2001 + Cout + Cin)


def dgrad1_ref(dy, w):
    """autograd of F.conv2d(x, w, padding=1) with respect to x; w rounded to fp16 as the pack rounds it"""
    Cout, Cin = w.shape[:2]
    B, _, H, W = dy.shape
    x = torch.zeros(B, Cin, H, W, dtype=f64, requires_grad=True)
    y = F.conv2d(x, w.half().to(f64), padding=1)
    return torch.autograd.grad(y, x, dy[:, :Cout].to(f64))[0]


def dgrad2_inputs(case):
    B, h, w_, Cout, Cin = case
    dy = torch.randn(B, Cout, h, w_, generator=_gen(3000 + h * w_ + Cout)).half()
    return dy, conv_weight(Cout, Cin, 3001 + Cout + Cin)


def dgrad2_ref(dy, w):
    """autograd of the padded stride-2 form with respect to x [B,Cin,2h,2w]"""
    Cout, Cin = w.shape[:2]
    B, _, h, w_ = dy.shape
    x = torch.zeros(B, Cin, 2 * h, 2 * w_, dtype=f64, requires_grad=True)
    y = F.conv2d(F.pad(x, (0, 1, 0, 1)), w.half().to(f64), stride=2)
    return torch.autograd.grad(y, x, dy.to(f64))[0]


# ---- weight packs -----------------------------------------------------------------------------------------------------------------
def pack_conv3_fwd(w):
    """forward layout [Cout][3][3][Cin] f16"""
    return w.half().permute(0, 2, 3, 1).contiguous()


def pack_conv3_dgrad_ref(w, pad):
    """[Cout,Cin,3,3] fp32 -> [Cin][t' = 3 (2 - ky) + (2 - kx)][pad] f16, zero beyond Cout"""
    Cout, Cin = w.shape[:2]
    out = torch.zeros(Cin, 9, pad, dtype=torch.float16)
    out[:, :, :Cout] = w.flip(2, 3).permute(1, 2, 3, 0).reshape(Cin, 9, Cout).half()
    return out


# (out, in) of the matrices; the fused q|k|v case packs three [out,in] blocks into one [in][3 out]
MAT_CASES = [(64, 128), (40, 24)]
QKV_CASE = (64, 128)


def mat_weight(out, in_, seed):
    return torch.randn(out, in_, generator=_gen(seed)) / in_ ** 0.5


def pack_mat_dgrad_ref(dst, w, col):
    """writes w^T (f16) into dst [in][ld] at columns col .. col + out; returns dst"""
    dst[:, col:col + w.shape[0]] = w.t().half()
    return dst


# ---- GroupNorm(+SiLU) backward ------------------------------------------------------------------------------------------------------
# (B, HW, C, G, silu, add, offset): x = randn * 2 + 0.5, or randn + 4 in the offset case
GN_CASES = [
    (2, 64, 64, 32, 1, False, False),       # C / G = 2
    (1, 4096, 128, 32, 1, True, False),     # 64 splits
    (3, 100, 512, 32, 0, True, False),      # ragged last split, 6 * 17 > 100
    (2, 37, 256, 32, 1, False, False),      # one split, HW not a multiple of the lanes
    (1, 289, 512, 32, 1, True, False),      # NS = 18, per = 17: the last split is empty
    (1, 2309, 512, 32, 1, False, False),    # split count capped at 128, ragged
    (2, 300, 8, 1, 1, False, False),        # one chunk column
    (2, 64, 64, 32, 1, True, True),         # offset: mean^2 / variance ~ 16
]
GN_REFUSED = (1, 16, 320, 32)               # B, HW, C, G: 256 % (C / 8) != 0


def gn_splits(HW, C):
    """the reduction's split geometry -> (NS, per): NS = HW / (PL * 4) in 1 .. 128 with PL = 256 / (C / 8) lanes; per = ceil(HW / NS)"""
    PL = 256 // (C // 8)
    NS = min(max(HW // (PL * 4), 1), GNB_MAX_SPLITS)
    return NS, (HW + NS - 1) // NS


def gn_inputs(case):
    """-> x, dy, add [B,HW,C] f16 (add None when unset), gamma, beta [C] f16.  Cotangents of order 0.5: no result is an fp16 subnormal"""
    B, HW, C, G, silu, add, offset = case
    g = _gen(4000 + HW + C + 7 * int(offset))
    x = torch.randn(B, HW, C, generator=g)
    x = (x + 4.0 if offset else x * 2.0 + 0.5).half()
    dy = (torch.randn(B, HW, C, generator=g) * 0.5).half()
    gamma = (torch.randn(C, generator=g) * 0.5 + 1.0).half()
    beta = (torch.randn(C, generator=g) * 0.5).half()
    a = (torch.randn(B, HW, C, generator=g) * 0.5).half() if add else None
    return x, dy, gamma, beta, a


def gn_bwd_terms(x, dy, gamma, beta, G, silu):
    """float64 closed form -> rstd [B,1,G,1], x^, du [B,HW,G,cg], c1, c2 [B,1,G,1]"""
    B, HW, C = x.shape
    xg = x.to(f64).reshape(B, HW, G, C // G)
    mean = xg.mean((1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(xg.var((1, 3), unbiased=False, keepdim=True) + GN_EPS)
    xh = (xg - mean) * rstd
    ga, be = gamma.to(f64).reshape(1, 1, G, -1), beta.to(f64).reshape(1, 1, G, -1)
    u = xh * ga + be
    du = dy.to(f64).reshape(B, HW, G, -1) * ga
    if silu:
        sg = torch.sigmoid(u)
        du = du * sg * (1.0 + u * (1.0 - sg))
    return rstd, xh, du, du.mean((1, 3), keepdim=True), (du * xh).mean((1, 3), keepdim=True)


def gn_bwd_ref(x, dy, gamma, beta, add, G, silu):
    """-> (want, bound) [B,HW,C] float64: want by autograd of F.group_norm (+ silu) (+ add), the bound from the closed form's terms"""
    B, HW, C = x.shape
    xx = x.to(f64).permute(0, 2, 1).contiguous().requires_grad_(True)              # [B,C,HW]
    y = F.group_norm(xx, G, gamma.to(f64), beta.to(f64), GN_EPS)
    if silu:
        y = F.silu(y)
    want = torch.autograd.grad(y, xx, dy.to(f64).permute(0, 2, 1))[0].permute(0, 2, 1)
    rstd, xh, du, c1, c2 = gn_bwd_terms(x, dy, gamma, beta, G, silu)
    t = (rstd * (du.abs() + c1.abs() + (xh * c2).abs())).reshape(B, HW, C)
    if add is not None:
        want = want + add.to(f64)
        t = t + add.to(f64).abs()
    return want, U10 * t + 1e-7


# ---- softmax rows -------------------------------------------------------------------------------------------------------------------
SOFTMAX_CASES = [(3, 64), (5, 384), (2, 2112), (1, 4096)]       # n = 2112: the second trip of the kernel's 2048-stride loop
SOFTMAX_SCALE = 0.5


def softmax_inputs(case):
    """-> scores s (randn * 4), probabilities P (the float64 softmax rounded to fp16: what the backward kernel is handed), dP; all f16"""
    rows, n = case
    g = _gen(5000 + rows + n)
    s = (torch.randn(rows, n, generator=g) * 4.0).half()
    P = torch.softmax(s.to(f64) * SOFTMAX_SCALE, -1).half()
    dP = torch.randn(rows, n, generator=g).half()
    return s, P, dP


def softmax_ref(s, scale):
    p = torch.softmax(s.to(f64) * scale, -1)
    return p, U10 * p + U24


def softmax_bwd_ref(P, dP, scale):
    p, d = P.to(f64), dP.to(f64)
    want = p * (d - (p * d).sum(-1, keepdim=True)) * scale
    return want, U10 * scale * p * (d.abs() + (p * d).abs().sum(-1, keepdim=True)) + U24


# ---- the two ends of the encoder backward ---------------------------------------------------------------------------------------------
QUANT_CASES = [(2, 8, 64), (1, 8, 300)]                         # (B, C, HW)
GSCALE = 64.0


def quant_inputs(case):
    """-> g f32 NCHW [B,C,HW], w f16 [C,C] (quant_conv.weight[o][c])"""
    B, C, HW = case
    g = _gen(6000 + C + HW)
    return torch.randn(B, C, HW, generator=g), (torch.randn(C, C, generator=g) / C ** 0.5).half()


def quant_bwd_ref(g, w, gscale):
    """-> (want, bound) [B*HW, 64]: d[p][c] = gscale sum_o g[o][p] w[o][c] for c < C, exactly 0 (bound 0) beyond"""
    B, C, HW = g.shape
    gg = g.to(f64).permute(0, 2, 1).reshape(B * HW, C)
    want, bound = torch.zeros(B * HW, 64, dtype=f64), torch.zeros(B * HW, 64, dtype=f64)
    want[:, :C] = gscale * gg @ w.to(f64)
    bound[:, :C] = U10 * gscale * gg.abs() @ w.to(f64).abs()
    return want, bound


CONV_IN_CASES = [(2, 16, 12, 64, 3), (1, 9, 13, 128, 3)]        # (B, H, W, C, Cimg)


def conv_in_inputs(case):
    """-> dy f16 [B,C,H,W], w f16 [C,Cimg,3,3] (conv_in.weight)"""
    B, H, W, C, Cimg = case
    g = _gen(7000 + H * W + C)
    return torch.randn(B, C, H, W, generator=g).half(), (torch.randn(C, Cimg, 3, 3, generator=g) / (9 * Cimg) ** 0.5).half()


def conv_in_pack(w):
    """the forward pack [C][3][3][8]: image channels last, zero-padded to 8"""
    C, Cimg = w.shape[:2]
    out = torch.zeros(C, 3, 3, 8, dtype=torch.float16)
    out[..., :Cimg] = w.permute(0, 2, 3, 1)
    return out


def conv_in_bwd_ref(dy, w, inv_gscale):
    """-> (want, bound) f64 NCHW [B,Cimg,H,W]: autograd of F.conv2d(img, w, padding=1) with respect to img, times inv_gscale"""
    B, C, H, W = dy.shape
    img = torch.zeros(B, w.shape[1], H, W, dtype=f64, requires_grad=True)
    want = torch.autograd.grad(F.conv2d(img, w.to(f64), padding=1), img, dy.to(f64))[0] * inv_gscale
    mag = F.conv_transpose2d(dy.to(f64).abs(), w.to(f64).abs(), padding=1)         # sum |dy w| over the terms of each element
    return want, 9 * C * U23 * inv_gscale * mag
