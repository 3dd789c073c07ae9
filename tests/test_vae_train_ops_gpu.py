"""GPU parity of the VAE encoder's training path, op by op, through the test seams of include/ctx_nerf.h: the downsampler's forward
geometry (stride 2, poff 1) and the two data-gradient geometries (default; ups 1, zins 1, poff -1) on every kernel the dispatcher can
route them to, the transposed / flipped weight packs, the GroupNorm(+SiLU) backward, the attention's row kernels and the two ends of
the encoder backward.  References, bounds, shapes and seeds: tests/vae_train_rule.py (float64 from the fp16-rounded inputs);
tests/test_vae_train_ops_cpu.py shows that those bounds reject the subtle mutations."""
import ctypes as C
import functools
import pytest
import torch

import vae_train_rule as R

pytestmark = pytest.mark.gpu

E_ARG = -1
TILES = list(range(28))
FORMS144 = [4, 5, 6, 7, 8]


def _lib():
    from contexture_nerf_amd import _lib as L
    return L, L.load()


def _last(lib):
    tile, use8 = C.c_int32(-7), C.c_int32(-7)
    lib.ctx_gemm_last_kernel(C.byref(tile), C.byref(use8))
    return tile.value, use8.value


def _conv(dev, x, w, bias, res, stride, ups, poff, zins, splitk=1, with_part=False):
    """x [B,H,W,Cin] f16, w [Cout,3,3,Cin] or [Cout,9,Cin] f16 (host) -> y [B,Ho,Wo,Cout] f16 (host) through ctx_conv3x3_geom_f16"""
    L, lib = _lib()
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    Ho, Wo = ((H << ups) - 1) // stride + 1, ((W << ups) - 1) // stride + 1
    xd, wd = x.contiguous().to(dev), w.contiguous().to(dev)
    bd = bias.to(dev) if bias is not None else None
    rd = res.contiguous().to(dev) if res is not None else None
    part = torch.empty((32 if splitk < 0 else splitk) * B * Ho * Wo * Cout, dtype=torch.float32, device=dev) if with_part else None
    y = torch.full((B, Ho, Wo, Cout), float("nan"), dtype=torch.float16, device=dev)
    L.check(lib.ctx_conv3x3_geom_f16(L.ptr(xd), L.ptr(wd), L.ptr(bd), L.ptr(rd), B, H, W, Cin, Cout, stride, ups, poff, zins, L.ptr(part),
                                     splitk, L.ptr(y), L.stream()))
    torch.cuda.synchronize()
    return y.cpu()


def _forced(lib, tile, use8):
    """what ran after a forced call: the forced kernel, or (it declined) a tile of gemm.hip"""
    t, u = _last(lib)
    if use8 == 0:
        assert (t, u) == (tile, 0), f"forced tile {tile}: tile {t} use8 {u} ran"
    else:
        assert (t, u) == (-1, use8) or (u == 0 and 0 <= t <= 27), f"forced use8 {use8}: tile {t} use8 {u} ran"
    return t, u


@functools.lru_cache(maxsize=None)
def _down(case):
    x, w, bias, res = R.down_inputs(case)
    return (R.nhwc(x), R.pack_conv3_fwd(w), bias, R.nhwc(res), R.nhwc(R.down_ref(x, w, bias, res)), R.nhwc(R.down_ref(x, w, bias, None)))


@pytest.mark.parametrize("case", R.DOWN_CASES)
def test_downsample_forward_on_every_kernel(dev, case):
    """stride 2 with poff 1 (diffusers pads (0,1,0,1)): the planner's choice, every tile of gemm.hip, gemm8.hip and the five forms of
    gemm144.hip, which carries its own copy of the tap arithmetic; bias + residual and bias alone."""
    L, lib = _lib()
    x, w, bias, res, want_r, want_b = _down(case)
    ran = set()
    try:
        for tile, use8 in [(None, None)] + [(t, 0) for t in TILES] + [(-1, 1)] + [(-1, f) for f in FORMS144]:
            if tile is None:
                lib.ctx_gemm_tune(-1, -1)
            else:
                lib.ctx_gemm_tune(tile, use8)
            for r, want in ((res, want_r), (None, want_b)):
                planned = tile is None
                y = _conv(dev, x, w, bias, r, 2, 0, 1, 0, splitk=-1 if planned else 1, with_part=planned)
                t, u = _last(lib) if planned else _forced(lib, tile, use8)
                ran.add((t, u))
                R.assert_within(y, want, R.conv_bound(want), f"downsample {case} forced ({tile}, {use8}) ran ({t}, {u}) res={r is not None}")
    finally:
        lib.ctx_gemm_tune(-1, -1)
    print("kernels that ran:", sorted(ran))


@functools.lru_cache(maxsize=None)
def _dgrad1(case):
    dy, w = R.dgrad1_inputs(case)
    return R.nhwc(dy), w, R.pack_conv3_dgrad_ref(w, case[5]), R.nhwc(R.dgrad1_ref(dy, w))


def _pack_conv3(dev, w, pad):
    L, lib = _lib()
    Cout, Cin = w.shape[:2]
    wd = w.contiguous().to(dev)
    dst = torch.full((Cin, 9, pad), 7.0, dtype=torch.float16, device=dev)
    L.check(lib.ctx_pack_conv3_dgrad_f16(L.ptr(wd), Cout, Cin, pad, L.ptr(dst), L.stream()))
    torch.cuda.synchronize()
    return dst.cpu()


@pytest.mark.parametrize("case", R.DGRAD1_CASES)
def test_dgrad_stride1_pack_then_default_geometry(dev, case):
    """ctx_pack_conv3_dgrad_f16 followed by the default geometry is the input gradient of the stride-1 convolution; the third case is
    conv_out's: 8 features packed with pad 64, the cotangent's channels >= 8 zero."""
    L, lib = _lib()
    dy, w, pack_want, want = _dgrad1(case)
    pack = _pack_conv3(dev, w, case[5])
    assert torch.equal(pack.view(torch.int16), pack_want.view(torch.int16)), f"dgrad pack {case} differs from the rule"
    for planned in (True, False):
        y = _conv(dev, dy, pack, None, None, 1, 0, 0, 0, splitk=-1 if planned else 1, with_part=planned)
        R.assert_within(y, want, R.conv_bound(want), f"dgrad stride 1 {case} planned={planned} ran {_last(lib)}")


@functools.lru_cache(maxsize=None)
def _dgrad2(case):
    dy, w = R.dgrad2_inputs(case)
    return R.nhwc(dy), R.pack_conv3_dgrad_ref(w, w.shape[0]), R.nhwc(R.dgrad2_ref(dy, w))


def _check_dgrad2(y, want, what):
    """the whole tensor, then every border row and column on its own so that a border error is named"""
    bound = R.conv_bound(want)
    for name, sl in (("top row", (slice(None), 0)), ("bottom row", (slice(None), -1)), ("left column", (slice(None), slice(None), 0)),
                     ("right column", (slice(None), slice(None), -1)), ("second row", (slice(None), 1)),
                     ("second column", (slice(None), slice(None), 1))):
        R.assert_within(y[sl], want[sl], bound[sl], f"{what}, {name}")
    R.assert_within(y, want, bound, what)


@pytest.mark.parametrize("case", R.DGRAD2_CASES)
def test_dgrad_stride2_zero_inserted_grid(dev, case):
    """ups 1, zins 1, poff -1 on the flipped pack is the input gradient of the padded stride-2 convolution: the planner's choice,
    every tile of gemm.hip, split-K 3; a forced gemm8 / conv_halo / gemm144 value is routed to gemm.hip, the only file with the
    zero-inserted addressing."""
    L, lib = _lib()
    dy, pack, want = _dgrad2(case)
    try:
        y = _conv(dev, dy, pack, None, None, 1, 1, -1, 1, splitk=-1, with_part=True)
        t, u = _last(lib)
        assert u == 0 and 0 <= t <= 27, f"planned zins convolution ran tile {t} use8 {u}"
        _check_dgrad2(y, want, f"dgrad stride 2 {case} planned, tile {t}")
        for tile in TILES:
            lib.ctx_gemm_tune(tile, 0)
            y = _conv(dev, dy, pack, None, None, 1, 1, -1, 1)
            _forced(lib, tile, 0)
            _check_dgrad2(y, want, f"dgrad stride 2 {case} tile {tile}")
        lib.ctx_gemm_tune(-1, -1)
        y = _conv(dev, dy, pack, None, None, 1, 1, -1, 1, splitk=3, with_part=True)
        _check_dgrad2(y, want, f"dgrad stride 2 {case} split-K 3, ran {_last(lib)}")
        for use8 in [1, 2, 3] + FORMS144:
            lib.ctx_gemm_tune(-1, use8)
            y = _conv(dev, dy, pack, None, None, 1, 1, -1, 1)
            t, u = _last(lib)
            assert u == 0 and 0 <= t <= 27, f"forced use8 {use8} on a zins convolution ran tile {t} use8 {u}: only gemm.hip has the addressing"
            _check_dgrad2(y, want, f"dgrad stride 2 {case} forced use8 {use8}, tile {t}")
    finally:
        lib.ctx_gemm_tune(-1, -1)


def test_planner_inherits_unet_table_entries(dev):
    """The tuned plan table is keyed on (M, N, K, stride 2, upsample) only, so a poff 1 or zins convolution of a UNet layer's extents
    runs that layer's plan (tile and split-K factor; a zins one always on gemm.hip): the result must be right whatever the plan is."""
    L, lib = _lib()
    for case in R.DOWN_PLAN_CASES:
        x, w, bias, res, want, _ = _down(case)
        y = _conv(dev, x, w, bias, res, 2, 0, 1, 0, splitk=-1, with_part=True)
        R.assert_within(y, want, R.conv_bound(want), f"downsample {case} planned, ran {_last(lib)}")
    for case in R.DGRAD2_PLAN_CASES:
        dy, pack, want = _dgrad2(case)
        y = _conv(dev, dy, pack, None, None, 1, 1, -1, 1, splitk=-1, with_part=True)
        t, u = _last(lib)
        assert u == 0 and 0 <= t <= 27, f"planned zins convolution ran tile {t} use8 {u}"
        _check_dgrad2(y, want, f"dgrad stride 2 {case} planned, tile {t}")


def test_halo_kernel_declines_an_offset_geometry(dev):
    """conv_halo.hip stages symmetric padding only: forced onto a stride-1 convolution with poff 1 at a shape it would take, it must
    decline (the call falls through to gemm.hip) and the result must be right; with poff 0 the same forcing does run it."""
    L, lib = _lib()
    x, w, bias = R.offset1_inputs(R.OFFSET1_CASE)
    want = R.nhwc(R.offset1_ref(x, w, bias))
    try:
        for use8 in (2, 3):
            lib.ctx_gemm_tune(-1, use8)
            y = _conv(dev, R.nhwc(x), R.pack_conv3_fwd(w), bias, None, 1, 0, 1, 0)
            t, u = _last(lib)
            assert u == 0 and 0 <= t <= 27, f"forced use8 {use8} with poff 1 ran tile {t} use8 {u}"
            R.assert_within(y, want, R.conv_bound(want), f"stride 1, poff 1 {R.OFFSET1_CASE} forced use8 {use8}, tile {t}")
            _conv(dev, R.nhwc(x), R.pack_conv3_fwd(w), bias, None, 1, 0, 0, 0)
            assert _last(lib) == (-1, use8), f"forced use8 {use8} with poff 0 ran {_last(lib)}"
    finally:
        lib.ctx_gemm_tune(-1, -1)


def test_invalid_geometries_are_refused_and_write_nothing(dev):
    L, lib = _lib()
    x = torch.randn(1, 9, 9, 64, device=dev).half()
    w = torch.randn(64, 3, 3, 64, device=dev).half()
    y = torch.full((1, 18, 18, 64), 3.0, dtype=torch.float16, device=dev)
    part = torch.empty(32 * 18 * 18 * 64, dtype=torch.float32, device=dev)
    # (H, W, stride, upsample, poff, zins, splitk)
    for H, W, stride, ups, poff, zins, splitk in [(8, 8, 1, 0, 0, 1, 1), (8, 8, 2, 0, 0, 1, 1), (8, 8, 2, 0, 1, 1, 1), (8, 8, 1, 1, 2, 0, 1),
                                                  (8, 8, 1, 1, -2, 1, 1), (9, 8, 2, 0, 1, 0, 1), (8, 9, 2, 0, 1, 0, 1), (9, 9, 1, 0, 1, 0, 1),
                                                  (8, 8, 2, 1, 0, 0, 1), (8, 8, 1, 1, -1, 2, 1), (8, 8, 1, 0, 0, 0, 0), (8, 8, 1, 0, 0, 0, 33)]:
        rc = lib.ctx_conv3x3_geom_f16(L.ptr(x), L.ptr(w), None, None, 1, H, W, 64, 64, stride, ups, poff, zins, L.ptr(part), splitk, L.ptr(y), L.stream())
        assert rc == E_ARG, f"H={H} W={W} stride={stride} ups={ups} poff={poff} zins={zins} splitk={splitk}: rc {rc}"
        assert lib.ctx_last_error()
    torch.cuda.synchronize()
    assert (y == 3.0).all(), "a refused call wrote to y"


def test_weight_packs_bit_for_bit(dev):
    """k_pack_conv3_T at every dgrad shape and k_pack_mat_T alone and as the fused q|k|v matrix, against the rule's permutation"""
    L, lib = _lib()
    for case in R.DGRAD1_CASES:
        _, w, want, _ = _dgrad1(case)
        got = _pack_conv3(dev, w, case[5])
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"conv pack {case}"
        assert not got[:, :, case[3]:].any(), f"conv pack {case}: the pad columns are not zero"
    for case in R.DGRAD2_CASES:
        w = R.dgrad2_inputs(case)[1]
        assert torch.equal(_pack_conv3(dev, w, w.shape[0]).view(torch.int16), R.pack_conv3_dgrad_ref(w, w.shape[0]).view(torch.int16)), f"conv pack {case}"
    for k, (out, in_) in enumerate(R.MAT_CASES):
        w = R.mat_weight(out, in_, 8000 + k)
        wd = w.to(dev)
        dst = torch.full((in_, out + 16), 7.0, dtype=torch.float16, device=dev)
        L.check(lib.ctx_pack_mat_dgrad_f16(L.ptr(wd), out, in_, out + 16, 8, L.ptr(dst), L.stream()))
        want = R.pack_mat_dgrad_ref(torch.full((in_, out + 16), 7.0, dtype=torch.float16), w, 8)
        assert torch.equal(dst.cpu().view(torch.int16), want.view(torch.int16)), f"matrix pack {(out, in_)}"
    out, in_ = R.QKV_CASE
    dst = torch.full((in_, 3 * out), 7.0, dtype=torch.float16, device=dev)
    want = torch.full((in_, 3 * out), 7.0, dtype=torch.float16)
    for blk in range(3):
        w = R.mat_weight(out, in_, 8100 + blk)
        wd = w.to(dev)
        L.check(lib.ctx_pack_mat_dgrad_f16(L.ptr(wd), out, in_, 3 * out, blk * out, L.ptr(dst), L.stream()))
        R.pack_mat_dgrad_ref(want, w, blk * out)
    assert torch.equal(dst.cpu().view(torch.int16), want.view(torch.int16)), "fused q|k|v matrix pack"
    assert not (want == 7.0).all(1).any()


def _gn_bwd(dev, x, dy, gamma, beta, add, G, silu, dx):
    L, lib = _lib()
    B, HW, Cc = x.shape
    ws = torch.full((lib.ctx_groupnorm_bwd_ws_bytes(B, G) // 4,), float("nan"), dtype=torch.float32, device=dev)   # nothing stale may be read
    rc = lib.ctx_groupnorm_bwd_f16(L.ptr(x), L.ptr(dy), L.ptr(gamma), L.ptr(beta), L.ptr(add), B, HW, Cc, G, R.GN_EPS, silu, L.ptr(dx), L.ptr(ws),
                                   L.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("case", R.GN_CASES)
def test_groupnorm_backward(dev, case):
    """k_gnb_reduce<0/1>, k_gnb_finalize<0/1> and k_gnb_apply against autograd in float64, at the split geometries the table of
    tests/vae_train_rule.py names; twice, bit-equal (fixed-order sums)."""
    L, lib = _lib()
    B, HW, Cc, G, silu, _, _ = case
    x, dy, gamma, beta, add = R.gn_inputs(case)
    want, bound = R.gn_bwd_ref(x, dy, gamma, beta, add, G, silu)
    d = [t.to(dev) if t is not None else None for t in (x, dy, gamma, beta, add)]
    outs = []
    for rep in range(2):
        dx = torch.full((B, HW, Cc), float("nan"), dtype=torch.float16, device=dev)
        L.check(_gn_bwd(dev, *d, G, silu, dx))
        outs.append(dx.cpu())
    R.assert_within(outs[0], want, bound, f"groupnorm backward {case}, splits {R.gn_splits(HW, Cc)}")
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), f"groupnorm backward {case}: two runs differ"


def test_groupnorm_backward_refuses_320_channels(dev):
    B, HW, Cc, G = R.GN_REFUSED
    x = torch.randn(B, HW, Cc, device=dev).half()
    g = torch.ones(Cc, dtype=torch.float16, device=dev)
    dx = torch.full((B, HW, Cc), 3.0, dtype=torch.float16, device=dev)
    assert _gn_bwd(dev, x, x, g, g, None, G, 1, dx) == E_ARG
    assert (dx == 3.0).all(), "a refused call wrote to dx"


@pytest.mark.parametrize("case", R.SOFTMAX_CASES)
def test_softmax_rows_forward_and_backward(dev, case):
    L, lib = _lib()
    rows, n = case
    s, P, dP = R.softmax_inputs(case)
    sd, Pd, dPd = s.to(dev), P.to(dev), dP.to(dev)               # held: a temporary's memory is reused by the next allocation
    p = torch.full((rows, n), float("nan"), dtype=torch.float16, device=dev)
    L.check(lib.ctx_softmax_rows_f16(L.ptr(sd), rows, n, R.SOFTMAX_SCALE, L.ptr(p), L.stream()))
    want, bound = R.softmax_ref(s, R.SOFTMAX_SCALE)
    R.assert_within(p.cpu(), want, bound, f"softmax rows {case}")
    dev_sum = (p.cpu().to(R.f64).sum(-1) - 1).abs().max()
    assert dev_sum <= n * 2.0 ** -11, f"softmax rows {case}: a row sums to 1 +- {dev_sum:.3e}"
    dS = torch.full((rows, n), float("nan"), dtype=torch.float16, device=dev)
    L.check(lib.ctx_softmax_bwd_rows_f16(L.ptr(Pd), L.ptr(dPd), rows, n, R.SOFTMAX_SCALE, L.ptr(dS), L.stream()))
    want, bound = R.softmax_bwd_ref(P, dP, R.SOFTMAX_SCALE)
    R.assert_within(dS.cpu(), want, bound, f"softmax backward {case}")


@pytest.mark.parametrize("case", R.QUANT_CASES)
def test_quant_bwd(dev, case):
    L, lib = _lib()
    B, Cc, HW = case
    g, w = R.quant_inputs(case)
    gd, wd = g.to(dev), w.to(dev)
    d = torch.full((B * HW, 64), float("nan"), dtype=torch.float16, device=dev)
    L.check(lib.ctx_quant_bwd_f16(L.ptr(gd), L.ptr(wd), B, Cc, HW, R.GSCALE, L.ptr(d), L.stream()))
    want, bound = R.quant_bwd_ref(g, w, R.GSCALE)
    got = d.cpu()
    assert (got[:, Cc:].view(torch.int16) == 0).all(), f"quant_bwd {case}: the padded channels are not +0"
    R.assert_within(got, want, bound, f"quant_bwd {case}")


@pytest.mark.parametrize("case", R.CONV_IN_CASES)
def test_conv_in_bwd(dev, case):
    L, lib = _lib()
    B, H, W, Cc, Cimg = case
    dy, w = R.conv_in_inputs(case)
    dyd, wd = R.nhwc(dy).to(dev), R.conv_in_pack(w).to(dev)
    dimg = torch.full((B, Cimg, H, W), float("nan"), dtype=torch.float32, device=dev)
    L.check(lib.ctx_conv_in_bwd_f16(L.ptr(dyd), L.ptr(wd), B, H, W, Cc, Cimg, 1.0 / R.GSCALE, L.ptr(dimg),
                                    L.stream()))
    want, bound = R.conv_in_bwd_ref(dy, w, 1.0 / R.GSCALE)
    R.assert_within(dimg.cpu(), want, bound, f"conv_in_bwd {case}")
