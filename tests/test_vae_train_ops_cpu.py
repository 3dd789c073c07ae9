"""CPU: the gates of tests/vae_train_rule.py can tell right from subtly wrong.  For every op of the VAE encoder's training path an
fp32 torch emulation of the kernel's formula with the kernel's rounding points (fp16 output, fp32 sums, sum and sum-of-squares
statistics) must lie inside the rule's bound on every input set the GPU test uses (tests/test_vae_train_ops_gpu.py imports the same
shapes and seeds), and each of the listed mutations of the emulation must fall outside it."""
import ctypes as C
import numpy as np
import pytest
import torch

import vae_train_rule as R

f32 = torch.float32


def _inside(got, want, bound, what):
    R.assert_within(got, want, bound, what)


def _outside(got, want, bound, what):
    r, _ = R.ratio(got, want, bound)
    print(f"{what}: max error / bound {r:.3g}")
    assert r > 1.0, f"{what}: the mutation stays inside the bound ({r:.3f}): the gate cannot see it"


# ---- emulations -----------------------------------------------------------------------------------------------------------------------
def emu_conv(x, wp, bias, res, stride, ups, poff, zins, zero_rows=True):
    """The implicit-GEMM convolution's addressing (conv_pixel / conv_tap / conv_tap_src of gemm_common.h) on x [B,H,W,C] f16 with
    weights wp [N][9][C] f16: output pixel (y, x) reads the virtual grid at (y stride + t / 3 - 1 + poff, x stride + t % 3 - 1 + poff);
    outside [0, H << ups) x [0, W << ups), and with zins at an odd row or column, it reads zero; else the source pixel is the
    coordinate >> ups.  fp32 sum, + bias + residual, one rounding.  zero_rows False: the mutation that forgets the odd rows."""
    B, H, W, Cc = x.shape
    Hv, Wv = H << ups, W << ups
    Ho, Wo = (Hv - 1) // stride + 1, (Wv - 1) // stride + 1
    N = wp.shape[0]
    xf = x.to(f32)
    acc = torch.zeros(B, Ho, Wo, N, dtype=f32)
    oy, ox = torch.arange(Ho) * stride, torch.arange(Wo) * stride
    for t in range(9):
        iy, ix = oy + t // 3 - 1 + poff, ox + t % 3 - 1 + poff
        oky, okx = (iy >= 0) & (iy < Hv), (ix >= 0) & (ix < Wv)
        if zins:
            okx &= (ix & 1) == 0
            if zero_rows:
                oky &= (iy & 1) == 0
        sy, sx = iy.clamp(0, Hv - 1) >> ups, ix.clamp(0, Wv - 1) >> ups
        patch = xf[:, sy][:, :, sx] * (oky[:, None] & okx[None, :]).to(f32)[None, :, :, None]
        acc += patch @ wp[:, t, :].to(f32).T
    if bias is not None:
        acc += bias.to(f32)
    if res is not None:
        acc += res.to(f32)
    return acc.half()


def emu_pack_conv3_T(w, pad, flip=True):
    """k_pack_conv3_T index by index: element i of [Cin][9][pad] <- s[((o Cin + c) 3 + ky) 3 + kx] with o = i % pad, t' = (i / pad) % 9,
    c = i / (9 pad), ky = 2 - t' / 3, kx = 2 - t' % 3.  flip False: the mutation that keeps the forward's tap order."""
    Cout, Cin = w.shape[:2]
    i = np.arange(Cin * 9 * pad)
    o, tp, c = i % pad, (i // pad) % 9, i // (pad * 9)
    ky, kx = (2 - tp // 3, 2 - tp % 3) if flip else (tp // 3, tp % 3)
    src = w.reshape(-1).numpy()[((np.minimum(o, Cout - 1) * Cin + c) * 3 + ky) * 3 + kx]
    return torch.from_numpy(np.where(o < Cout, src, np.float32(0)).astype(np.float16)).reshape(Cin, 9, pad)


def emu_pack_mat_T(dst, w, col):
    """k_pack_mat_T index by index: d[c ld + col + o] = s[i], c = i % in, o = i / in"""
    out, in_ = w.shape
    i = np.arange(out * in_)
    d = dst.reshape(-1).numpy()
    d[(i % in_) * dst.shape[1] + col + i // in_] = w.reshape(-1).numpy().astype(np.float16)
    return dst


def emu_gn_bwd(x, dy, gamma, beta, add, G, silu, mut=None):
    """k_gnb_reduce<0/1>, k_gnb_finalize and k_gnb_apply in fp32: statistics from (sum x, sum x^2) (the kernel sums about a pivot of the
    group, the same quantities in exact arithmetic: tests/norm_rule.py), du = dy silu'(u) gamma, c1 = sum du / n,
    c2 = sum du x^ / n, dx = (f16)(rstd (du - c1 - x^ c2) + add).  mut: 'no_c1' | 'c2_from_x' | 'skip_last' (every split of the two
    reductions stops one pixel early)."""
    B, HW, Cc = x.shape
    cg = Cc // G
    n = torch.tensor(float(HW) * float(cg), dtype=f32)
    keep = torch.ones(HW, dtype=f32)
    if mut == "skip_last":
        NS, per = R.gn_splits(HW, Cc)
        for sp in range(NS):
            p0, p1 = sp * per, min(HW, sp * per + per)
            if p1 > p0:
                keep[p1 - 1] = 0
    m = keep.reshape(1, HW, 1, 1)
    xf = x.to(f32).reshape(B, HW, G, cg)
    mean = (xf * m).sum((1, 3), keepdim=True) / n
    rstd = torch.rsqrt(((xf * xf * m).sum((1, 3), keepdim=True) / n - mean * mean).clamp_min(0) + f32_(R.GN_EPS))
    ga, be = gamma.to(f32).reshape(1, 1, G, cg), beta.to(f32).reshape(1, 1, G, cg)
    xh = (xf - mean) * rstd
    u = xh * ga + be
    du = dy.to(f32).reshape(B, HW, G, cg)
    if silu:
        sg = 1.0 / (1.0 + torch.exp(-u))
        du = du * (sg * (1.0 + u * (1.0 - sg)))
    du = du * ga
    c1 = (du * m).sum((1, 3), keepdim=True) / n
    c2 = (du * (xf if mut == "c2_from_x" else xh) * m).sum((1, 3), keepdim=True) / n
    if mut == "no_c1":
        c1 = torch.zeros_like(c1)
    out = (rstd * (du - c1 - xh * c2)).reshape(B, HW, Cc)
    if add is not None:
        out = out + add.to(f32)
    return out.half()


def f32_(v):
    return torch.tensor(v, dtype=f32)


def emu_softmax(s, scale):
    """k_softmax_rows: exp2((f32)s scale log2(e) - max), fp32 sum, times the reciprocal, one rounding"""
    sl = f32_(1.4426950408889634) * f32_(scale)
    a = s.to(f32) * sl
    e = torch.exp2(a - a.max(-1, keepdim=True).values)
    return (e * (1.0 / e.sum(-1, keepdim=True))).half()


def emu_softmax_bwd(P, dP, scale, rowsum=True):
    """k_softmax_bwd_rows: dS = (f16)(P (dP - sum_j P_j dP_j) scale) in fp32.  rowsum False: the mutation that drops the sum"""
    p, d = P.to(f32), dP.to(f32)
    dot = (p * d).sum(-1, keepdim=True) if rowsum else torch.zeros(p.shape[0], 1)
    return (p * (d - dot) * f32_(scale)).half()


def emu_quant_bwd(g, w, gscale):
    """k_quant_bwd: in_o = g_o gscale, d[p][c] = (f16) sum_o in_o w[o][c] in fp32, zero for c >= C; [B*HW, 64]"""
    B, Cc, HW = g.shape
    out = torch.zeros(B * HW, 64, dtype=torch.float16)
    out[:, :Cc] = ((g * f32_(gscale)).permute(0, 2, 1).reshape(B * HW, Cc) @ w.to(f32)).half()
    return out


def emu_conv_in_bwd(dy, wpack, Cimg, inv_gscale):
    """k_conv_in_bwd on the forward pack [C][3][3][8]: dimg[ci][iy][ix] = inv_gscale sum_t sum_c dy[c][iy - ky + 1][ix - kx + 1] w[c][t][ci]"""
    B, Cc, H, W = dy.shape
    d = torch.nn.functional.pad(dy.to(f32), (1, 1, 1, 1))
    acc = torch.zeros(B, Cimg, H, W, dtype=f32)
    wf = wpack.to(f32).reshape(Cc, 9, 8)
    for t in range(9):
        ky, kx = t // 3, t % 3
        sh = d[:, :, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W]                          # dy[iy - ky + 1, ix - kx + 1], zero outside
        acc += torch.einsum("bchw,ci->bihw", sh, wf[:, t, :Cimg])
    return acc * f32_(inv_gscale)


# ---- emulation inside the bound, on the GPU test's inputs ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.DOWN_CASES + R.DOWN_PLAN_CASES)
def test_downsample_forward_emulation_and_padding_side(case):
    x, w, bias, res = R.down_inputs(case)
    wp = R.pack_conv3_fwd(w).reshape(w.shape[0], 9, w.shape[1])
    for b, r in ((bias, res), (bias, None)):
        want = R.nhwc(R.down_ref(x, w, b, r))
        rr = R.nhwc(r) if r is not None else None
        _inside(emu_conv(R.nhwc(x), wp, b, rr, 2, 0, 1, 0), want, R.conv_bound(want), f"downsample {case} res={r is not None}")
        _outside(emu_conv(R.nhwc(x), wp, b, rr, 2, 0, 0, 0), want, R.conv_bound(want), f"downsample {case}, poff 0 in place of 1")


def test_stride1_offset_geometry_emulation():
    x, w, bias = R.offset1_inputs(R.OFFSET1_CASE)
    wp = R.pack_conv3_fwd(w).reshape(w.shape[0], 9, w.shape[1])
    want = R.nhwc(R.offset1_ref(x, w, bias))
    _inside(emu_conv(R.nhwc(x), wp, bias, None, 1, 0, 1, 0), want, R.conv_bound(want), f"stride 1, poff 1 {R.OFFSET1_CASE}")
    _outside(emu_conv(R.nhwc(x), wp, bias, None, 1, 0, 0, 0), want, R.conv_bound(want), f"stride 1 {R.OFFSET1_CASE}, poff 0 in place of 1")


@pytest.mark.parametrize("case", R.DGRAD1_CASES)
def test_dgrad_stride1_emulation_and_tap_flip(case):
    dy, w = R.dgrad1_inputs(case)
    pad = case[5]
    want = R.nhwc(R.dgrad1_ref(dy, w))
    wp = R.pack_conv3_dgrad_ref(w, pad)
    assert torch.equal(wp, emu_pack_conv3_T(w, pad))
    _inside(emu_conv(R.nhwc(dy), wp, None, None, 1, 0, 0, 0), want, R.conv_bound(want), f"dgrad stride 1 {case}")
    _outside(emu_conv(R.nhwc(dy), emu_pack_conv3_T(w, pad, flip=False), None, None, 1, 0, 0, 0), want, R.conv_bound(want),
             f"dgrad stride 1 {case}, taps not flipped")


@pytest.mark.parametrize("case", R.DGRAD2_CASES + R.DGRAD2_PLAN_CASES)
def test_dgrad_stride2_emulation_and_zero_insertion(case):
    dy, w = R.dgrad2_inputs(case)
    want = R.nhwc(R.dgrad2_ref(dy, w))
    wp = R.pack_conv3_dgrad_ref(w, w.shape[0])
    _inside(emu_conv(R.nhwc(dy), wp, None, None, 1, 1, -1, 1), want, R.conv_bound(want), f"dgrad stride 2 {case}")
    _outside(emu_conv(R.nhwc(dy), wp, None, None, 1, 1, -1, 1, zero_rows=False), want, R.conv_bound(want),
             f"dgrad stride 2 {case}, odd rows not zeroed")
    _outside(emu_conv(R.nhwc(dy), emu_pack_conv3_T(w, w.shape[0], flip=False), None, None, 1, 1, -1, 1), want, R.conv_bound(want),
             f"dgrad stride 2 {case}, taps not flipped")
    _outside(emu_conv(R.nhwc(dy), wp, None, None, 1, 1, 0, 1), want, R.conv_bound(want), f"dgrad stride 2 {case}, poff 0 in place of -1")


def test_pack_rules_match_the_kernels_index_formula():
    for case in R.DGRAD1_CASES:
        _, w = R.dgrad1_inputs(case)
        ref = R.pack_conv3_dgrad_ref(w, case[5])
        assert torch.equal(ref, emu_pack_conv3_T(w, case[5])) and not ref[:, :, case[3]:].any()
        assert not torch.equal(ref, emu_pack_conv3_T(w, case[5], flip=False))
    for k, (out, in_) in enumerate(R.MAT_CASES):
        w = R.mat_weight(out, in_, 8000 + k)
        a, b = torch.full((in_, out + 16), 7, dtype=torch.float16), torch.full((in_, out + 16), 7, dtype=torch.float16)
        assert torch.equal(R.pack_mat_dgrad_ref(a, w, 8), emu_pack_mat_T(b, w, 8))
        assert (a[:, :8] == 7).all() and (a[:, 8 + out:] == 7).all()             # the rest of the matrix is not written


@pytest.mark.parametrize("case", R.GN_CASES)
def test_groupnorm_backward_emulation_and_mutations(case):
    B, HW, Cc, G, silu, _, _ = case
    x, dy, gamma, beta, add = R.gn_inputs(case)
    want, bound = R.gn_bwd_ref(x, dy, gamma, beta, add, G, silu)
    # the closed form the bound's terms come from is the autograd result
    rstd, xh, du, c1, c2 = R.gn_bwd_terms(x, dy, gamma, beta, G, silu)
    closed = (rstd * (du - c1 - xh * c2)).reshape(B, HW, Cc) + (add.to(R.f64) if add is not None else 0)
    assert (closed - want).abs().max() < 1e-11
    what = f"groupnorm backward {case}"
    _inside(emu_gn_bwd(x, dy, gamma, beta, add, G, silu), want, bound, what)
    _outside(emu_gn_bwd(x, dy, gamma, beta, add, G, silu, "no_c1"), want, bound, what + ", c1 dropped")
    _outside(emu_gn_bwd(x, dy, gamma, beta, add, G, silu, "c2_from_x"), want, bound, what + ", c2 from x")
    _outside(emu_gn_bwd(x, dy, gamma, beta, add, G, silu, "skip_last"), want, bound, what + ", last pixel of a split skipped")


def test_groupnorm_split_geometry_of_the_cases():
    """the cases reach what their comments say: split counts, ragged and empty last splits, the cap"""
    assert R.gn_splits(64, 64) == (1, 64)
    assert R.gn_splits(4096, 128) == (64, 64)
    assert R.gn_splits(100, 512) == (6, 17) and 5 * 17 < 100 < 6 * 17
    assert R.gn_splits(37, 256) == (1, 37)
    assert R.gn_splits(289, 512) == (18, 17) and 17 * 17 == 289                   # split 17 starts at HW: empty
    assert R.gn_splits(2309, 512) == (128, 19) and 2309 % 19 != 0
    assert R.gn_splits(300, 8)[0] == 1
    _, HW, Cc, _ = R.GN_REFUSED
    assert Cc % 8 == 0 and 256 % (Cc // 8) != 0
    for case in R.GN_CASES:                                                        # no wanted value is an fp16 subnormal's neighbour
        x, dy, gamma, beta, add = R.gn_inputs(case)
        want, bound = R.gn_bwd_ref(x, dy, gamma, beta, add, case[3], case[4])
        assert (bound > 0).all() and torch.isfinite(want).all()


@pytest.mark.parametrize("case", R.SOFTMAX_CASES)
def test_softmax_rows_emulation_and_rowsum(case):
    s, P, dP = R.softmax_inputs(case)
    want, bound = R.softmax_ref(s, R.SOFTMAX_SCALE)
    got = emu_softmax(s, R.SOFTMAX_SCALE)
    _inside(got, want, bound, f"softmax rows {case}")
    assert (got.to(R.f64).sum(-1) - 1).abs().max() <= case[1] * 2.0 ** -11
    want, bound = R.softmax_bwd_ref(P, dP, R.SOFTMAX_SCALE)
    _inside(emu_softmax_bwd(P, dP, R.SOFTMAX_SCALE), want, bound, f"softmax backward {case}")
    _outside(emu_softmax_bwd(P, dP, R.SOFTMAX_SCALE, rowsum=False), want, bound, f"softmax backward {case}, rowsum dropped")


@pytest.mark.parametrize("case", R.QUANT_CASES)
def test_quant_bwd_emulation(case):
    g, w = R.quant_inputs(case)
    want, bound = R.quant_bwd_ref(g, w, R.GSCALE)
    got = emu_quant_bwd(g, w, R.GSCALE)
    _inside(got, want, bound, f"quant_bwd {case}")
    assert not got[:, case[1]:].any() and not bound[:, case[1]:].any()
    _outside(emu_quant_bwd(g, w.t().contiguous(), R.GSCALE), want, bound, f"quant_bwd {case}, weight not transposed")


@pytest.mark.parametrize("case", R.CONV_IN_CASES)
def test_conv_in_bwd_emulation(case):
    dy, w = R.conv_in_inputs(case)
    want, bound = R.conv_in_bwd_ref(dy, w, 1.0 / R.GSCALE)
    _inside(emu_conv_in_bwd(dy, R.conv_in_pack(w), case[4], 1.0 / R.GSCALE), want, bound, f"conv_in_bwd {case}")
    _outside(emu_conv_in_bwd(dy, R.conv_in_pack(w.flip(2, 3)), case[4], 1.0 / R.GSCALE), want, bound, f"conv_in_bwd {case}, taps flipped")


# ---- the seams refuse what they must, before anything is launched (no device needed: host buffers, never dereferenced) ---------------------
def test_seams_refuse_invalid_arguments_without_a_device():
    from contexture_nerf_amd import _lib as L
    lib = L.load()
    buf = (C.c_uint16 * 64)()
    p = C.cast(buf, C.c_void_p)
    E_ARG = -1
    for stride, ups, poff, zins, H, W in [(1, 0, 0, 1, 8, 8), (2, 0, 0, 1, 8, 8), (1, 1, 2, 0, 8, 8), (1, 0, -2, 0, 8, 8), (2, 0, 1, 0, 9, 8),
                                          (2, 0, 1, 0, 8, 7), (1, 1, -1, 2, 8, 8)]:
        assert lib.ctx_conv3x3_geom_f16(p, p, None, None, 1, H, W, 64, 64, stride, ups, poff, zins, None, 1, p, None) == E_ARG, (stride, ups, poff, zins)
        assert lib.ctx_last_error()
    assert lib.ctx_conv3x3_geom_f16(p, p, None, None, 1, 8, 8, 64, 64, 1, 0, 0, 0, p, 0, p, None) == E_ARG          # splitk 0
    assert lib.ctx_conv3x3_geom_f16(p, p, None, None, 1, 8, 8, 64, 64, 1, 0, 0, 0, p, 10, p, None) == E_ARG         # splitk > K / 64
    assert lib.ctx_groupnorm_bwd_f16(p, p, p, p, None, 1, 16, 320, 32, 1e-6, 1, p, p, None) == E_ARG
    assert lib.ctx_groupnorm_bwd_f16(p, p, p, p, None, 1, 16, 4, 1, 1e-6, 1, p, p, None) == E_ARG                    # C < 8
    assert lib.ctx_groupnorm_bwd_f16(p, p, p, p, None, 1, 16, 64, 24, 1e-6, 1, p, p, None) == E_ARG                  # C % groups
    assert lib.ctx_softmax_rows_f16(p, 1, 12, 1.0, p, None) == E_ARG
    assert lib.ctx_softmax_bwd_rows_f16(p, p, 1, 12, 1.0, p, None) == E_ARG
    assert lib.ctx_quant_bwd_f16(p, p, 1, 17, 64, 1.0, p, None) == E_ARG
    assert lib.ctx_conv_in_bwd_f16(p, p, 1, 8, 8, 64, 5, 1.0, p, None) == E_ARG
    assert lib.ctx_conv_in_bwd_f16(p, p, 1, 8, 8, 60, 3, 1.0, p, None) == E_ARG
    assert lib.ctx_pack_conv3_dgrad_f16(p, 16, 8, 8, p, None) == E_ARG                                               # pad < Cout
    assert lib.ctx_pack_mat_dgrad_f16(p, 16, 8, 20, 8, p, None) == E_ARG                                             # col + out > ld
    assert lib.ctx_groupnorm_bwd_ws_bytes(2, 32) == (2 * 128 * 32 * 2 + 2 * 32 * 4) * 4
