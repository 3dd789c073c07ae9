"""GPU parity of the engines' small ops, op by op, through the test seams of include/ctx_nerf.h: conv_in, conv_out, the time-embedding
GEMV, the timestep embedding, the per-head transpose, the concats, the converters, ControlNet's small convolution and residual
injection, the VAE's pointwise convolutions and the forward weight packs.  Each seam goes through the host function the engine calls.
References, bounds, cases and seeds: tests/engine_ops_rule.py (float64 from the inputs as the kernel sees them);
tests/test_engine_ops_cpu.py shows that those bounds reject the subtle mutations.  Every output buffer lies between two guard
regions of 0xA5 bytes that must come back unchanged."""
import ctypes as C
import math
import pytest
import torch

import engine_ops_rule as R

pytestmark = pytest.mark.gpu

E_ARG = -1
GUARD = 4096            # bytes on either side of an output
f16, f32 = torch.float16, torch.float32


def _lib():
    from contexture_nerf_amd import _lib as L
    return L, L.load()


class Out:
    """An output tensor of `shape` between two guards.  fill: the byte the tensor starts from: 0xFF (every f16 / f32 element a NaN:
    an element the kernel skips fails the finiteness check or the bit comparison) or 0xA5 (a refused call must leave it)."""

    def __init__(self, dev, shape, dtype, fill=0xFF):
        self.n = math.prod(shape) * torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full((2 * GUARD + self.n,), 0xA5, dtype=torch.uint8, device=dev)
        self.raw[GUARD:GUARD + self.n] = fill
        self.t = self.raw[GUARD:GUARD + self.n].view(dtype).view(shape)

    def cpu(self, what):
        torch.cuda.synchronize()
        raw = self.raw.cpu()
        assert (raw[:GUARD] == 0xA5).all(), f"{what}: wrote in front of its output"
        assert (raw[GUARD + self.n:] == 0xA5).all(), f"{what}: wrote behind its output"
        return self.t.cpu()

    def untouched(self, what):
        torch.cuda.synchronize()
        assert (self.raw.cpu() == 0xA5).all(), f"{what}: a refused call wrote to its output"


def _refused(lib, rc, needle, what):
    assert rc == E_ARG, f"{what}: returned {rc}, not CTX_E_ARG"
    msg = lib.ctx_last_error().decode()
    assert needle in msg, f"{what}: ctx_last_error says {msg!r}"


def _pack_fwd(dev, case, src):
    """the pack of `src` through ctx_pack_fwd_f16 -> flat f16 (host)"""
    L, lib = _lib()
    kind, a, b = case
    want = R.pack_ref(case, src)
    sd = src.contiguous().to(dev)
    out = Out(dev, (want.numel(),), f16)
    L.check(lib.ctx_pack_fwd_f16(L.ptr(sd), kind, a, b, L.ptr(out.t), L.stream()))
    return out.cpu(f"pack {case}"), want


# ---- convolutions -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CONV_IN_CASES)
def test_conv_in(dev, case):
    """k_conv_in<CP, CX> at every instantiation, the idle / short / looping grid.y slices and the ragged pixel blocks of the rule's table"""
    L, lib = _lib()
    B, Cin, H, W, Cout = case
    x, w, bias = R.conv_in_inputs(case)
    want, bound = R.conv_in_ref(x, w, bias)
    xd, wd, bd = x.to(dev), R.pack_conv3_ref(w, R.conv_in_pad(Cin)).to(dev), bias.to(dev)
    y = Out(dev, (B, H, W, Cout), f16)
    L.check(lib.ctx_conv_in_f16(L.ptr(xd), L.ptr(wd), L.ptr(bd), B, Cin, H, W, Cout, L.ptr(y.t), L.stream()))
    R.assert_within(y.cpu(f"conv_in {case}"), want, bound, f"conv_in {case}")


@pytest.mark.parametrize("case", R.CONV_OUT_CASES)
def test_conv_out(dev, case):
    """k_conv_out<NU, WF32>: the three unrolls with masked lanes, fp32- and fp16-staged weights, the second prefetched pixel of a wave"""
    L, lib = _lib()
    B, H, W, Cc, Cout = case
    x, w, bias = R.conv_out_inputs(case)
    want, bound = R.conv_out_ref(x, w, bias)
    xd, wd, bd = R.nhwc(x).to(dev), R.pack_conv3_ref(w).to(dev), bias.to(dev)
    y = Out(dev, (B, Cout, H, W), f32)
    L.check(lib.ctx_conv_out_f16(L.ptr(xd), L.ptr(wd), L.ptr(bd), B, H, W, Cc, Cout, L.ptr(y.t), L.stream()))
    R.assert_within(y.cpu(f"conv_out {case}"), want, bound, f"conv_out {case}")


@pytest.mark.parametrize("case", R.CONV_SMALL_CASES)
def test_conv_small(dev, case):
    """k_conv_small on the layers of ControlNet's conditioning embedding: f32 NCHW and f16 NHWC input, the 16-byte and the scalar channel
    loop, stride 1 and 2 on even and odd grids, with and without SiLU"""
    L, lib = _lib()
    B, H, W, Cin, Cout, stride, from_f32, silu = case
    x, w, bias = R.conv_small_inputs(case)
    want, bound = R.conv_small_ref(x, w, bias, stride, silu)
    xd = (x if from_f32 else R.nhwc(x)).contiguous().to(dev)
    wd, bd = R.pack_conv3_ref(w).to(dev), bias.to(dev)
    y = Out(dev, tuple(want.shape), f16)
    L.check(lib.ctx_conv_small_f16(L.ptr(xd if from_f32 else None), L.ptr(None if from_f32 else xd), L.ptr(wd), L.ptr(bd), B, H, W, Cin, Cout,
                                   stride, silu, L.ptr(y.t), L.stream()))
    R.assert_within(y.cpu(f"conv_small {case}"), want, bound, f"conv_small {case}")


@pytest.mark.parametrize("case", R.POINTWISE_CASES)
def test_pointwise(dev, case):
    L, lib = _lib()
    nh, B, Cc, HW = case
    x, w, b = R.pointwise_inputs(case)
    want, bound = R.pointwise_ref(x, w, b)
    xd = (x.permute(0, 2, 1) if nh else x).contiguous().to(dev)
    wd, bd = w.to(dev), b.to(dev)
    y = Out(dev, (B, Cc, HW), f32)
    L.check(lib.ctx_pointwise_f32(L.ptr(xd), L.ptr(wd), L.ptr(bd), B, Cc, HW, nh, L.ptr(y.t), L.stream()))
    R.assert_within(y.cpu(f"pointwise {case}"), want, bound, f"pointwise {case}")


# ---- the time-embedding path ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.GEMV_CASES)
def test_gemv(dev, case):
    """k_gemv_f16: one and several K blocks, the clamped and masked K tail, an odd N, one to three passes of four batch rows, SiLU on
    either side, no bias"""
    L, lib = _lib()
    Bm, N, K, si, so, _ = case
    x, w, bias = R.gemv_inputs(case)
    want, bound = R.gemv_ref(x, w, bias, si, so)
    xd, wd, bd = x.to(dev), w.to(dev), (bias.to(dev) if bias is not None else None)
    y = Out(dev, (Bm, N), f16)
    L.check(lib.ctx_gemv_f16(L.ptr(xd), L.ptr(wd), L.ptr(bd), Bm, N, K, si, so, L.ptr(y.t), L.stream()))
    R.assert_within(y.cpu(f"gemv {case}"), want, bound, f"gemv {case}")


@pytest.mark.parametrize("case", R.TIME_EMBED_CASES)
def test_time_embed(dev, case):
    L, lib = _lib()
    B, dim, t = case
    want, bound = R.time_embed_ref(B, dim, t)
    td = torch.tensor([t, -12345.0], dtype=f32, device=dev)          # one timestep: what follows it is not read
    y = Out(dev, (B, dim), f16)
    L.check(lib.ctx_time_embed_f16(L.ptr(td), B, dim, L.ptr(y.t), L.stream()))
    R.assert_within(y.cpu(f"time_embed {case}"), want, bound, f"time_embed {case}")


# ---- the bit-exact movers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.TRANSPOSE_V_CASES)
def test_transpose_v(dev, case):
    """k_transpose_v on a column slice of a wider row (the pointer the engine passes is base + column offset), S not a multiple of 64,
    Sp > S: the keys S .. Sp exactly +0"""
    L, lib = _lib()
    B, S, ld, heads, Sp, off = case
    v = R.transpose_v_inputs(case)
    want = R.transpose_v_ref(v, heads, Sp, off)
    vd = v.to(dev)
    vt = Out(dev, (B, heads, 64, Sp), f16)
    L.check(lib.ctx_transpose_v_f16(L.ptr(vd.view(-1)[off:]), B, S, ld, heads, Sp, L.ptr(vt.t), L.stream()))
    got = vt.cpu(f"transpose_v {case}")
    assert (R.bits(got[..., S:]) == 0).all(), f"transpose_v {case}: the padded keys are not +0"
    assert torch.equal(R.bits(got), R.bits(want)), f"transpose_v {case} differs from the rule"


def _concat(dev, case, dtype, fn):
    L, lib = _lib()
    M, Ca, Cb = case
    a, b = R.concat_inputs(case, dtype)
    both = torch.cat([a.reshape(-1), b.reshape(-1)]).to(dev)         # one allocation: the second source is a view at a non-zero offset
    y = Out(dev, (M, Ca + Cb), dtype)
    L.check(fn(lib)(L.ptr(both[:M * Ca]), L.ptr(both[M * Ca:]), M, Ca, Cb, L.ptr(y.t), L.stream()))
    assert torch.equal(R.bits(y.cpu(f"concat {case}")), R.bits(torch.cat([a, b], 1))), f"concat {dtype} {case} differs from torch.cat"


@pytest.mark.parametrize("case", R.CONCAT_F16_CASES)
def test_concat_f16(dev, case):
    _concat(dev, case, f16, lambda lib: lib.ctx_concat_f16)


@pytest.mark.parametrize("case", R.CONCAT_F32_CASES)
def test_concat_f32(dev, case):
    _concat(dev, case, f32, lambda lib: lib.ctx_concat_f32)


@pytest.mark.parametrize("n", R.F32_TO_F16_SIZES)
def test_f32_to_f16(dev, n):
    L, lib = _lib()
    x = R.f32_to_f16_inputs(n)
    xd = x.to(dev)
    y = Out(dev, (n,), f16, fill=0xA5)
    L.check(lib.ctx_f32_to_f16(L.ptr(xd), n, L.ptr(y.t), L.stream()))
    got, want = y.cpu(f"f32_to_f16 {n}"), x.half()
    assert R.same_bits_or_nan(got, want), f"f32_to_f16 n={n}: differs from torch's .half() at {(R.bits(got) != R.bits(want)).nonzero()[:8].flatten().tolist()}"


@pytest.mark.parametrize("n", R.F16_TO_F32_SIZES)
def test_f16_to_f32(dev, n):
    L, lib = _lib()
    x = R.f16_to_f32_inputs(n)
    xd = x.to(dev)
    y = Out(dev, (n,), f32, fill=0xA5)
    L.check(lib.ctx_f16_to_f32(L.ptr(xd), n, L.ptr(y.t), L.stream()))
    assert R.same_bits_or_nan(y.cpu(f"f16_to_f32 {n}"), x.float()), f"f16_to_f32 n={n}: differs from torch's .float()"


@pytest.mark.parametrize("case", R.ADD_SCALED_CASES)
def test_add_scaled(dev, case):
    """k_add_scaled_f16 in place; the largest case is one vector past what the capped grid covers in one sweep"""
    L, lib = _lib()
    n, scale = case
    dst, src = R.add_scaled_inputs(case)
    want, bound = R.add_scaled_ref(dst, src, scale)
    sd = src.to(dev)
    y = Out(dev, (n,), f16)
    y.t.copy_(dst.to(dev))
    L.check(lib.ctx_add_scaled_f16(L.ptr(y.t), L.ptr(sd), scale, n, L.stream()))
    R.assert_within(y.cpu(f"add_scaled {case}"), want, bound, f"add_scaled {case}")


@pytest.mark.parametrize("case", R.PACK_CASES)
def test_pack_fwd(dev, case):
    """k_pack_copy, k_pack_conv3 (also conv_in's padded rows: the padding exactly +0) and k_pack_geglu, with engine_set_param's grid"""
    got, want = _pack_fwd(dev, case, R.pack_inputs(case))
    assert torch.equal(R.bits(got), R.bits(want)), f"pack {case} differs from the rule"
    if case[0] == R.PK_CONVIN:
        assert (R.bits(got.reshape(case[1], 9, -1)[..., case[2]:]) == 0).all(), f"pack {case}: the padding channels are not +0"


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched(dev):
    """every argument check this op layer gained: CTX_E_ARG, a message that names the op, and not a byte of the output written"""
    L, lib = _lib()
    big = torch.zeros(1 << 16, dtype=f32, device=dev)              # any input: large enough for every shape below, were a check missing
    p, s = L.ptr(big), L.stream()
    null = L.ptr(None)

    def out():
        return Out(dev, (1 << 14,), f32, fill=0xA5)

    for B, Cin, H, W, Cout in R.CONV_IN_REFUSED:
        y = out()
        _refused(lib, lib.ctx_conv_in_f16(p, p, p, B, Cin, H, W, Cout, L.ptr(y.t), s), "conv_in", f"conv_in Cin={Cin}")
        y.untouched(f"conv_in Cin={Cin}")
    for B, H, W, Cc, Cout in R.CONV_OUT_REFUSED:
        y = out()
        _refused(lib, lib.ctx_conv_out_f16(p, p, p, B, H, W, Cc, Cout, L.ptr(y.t), s), "conv_out", f"conv_out C={Cc} Cout={Cout}")
        y.untouched(f"conv_out C={Cc} Cout={Cout}")
    for B, S, ld, heads, Sp, _ in R.TRANSPOSE_V_REFUSED:
        y = out()
        _refused(lib, lib.ctx_transpose_v_f16(p, B, S, ld, heads, Sp, L.ptr(y.t), s), "transpose_v", f"transpose_v S={S} ld={ld} Sp={Sp}")
        y.untouched(f"transpose_v S={S} ld={ld} Sp={Sp}")
    for Bm, N, K in R.GEMV_REFUSED:
        y = out()
        _refused(lib, lib.ctx_gemv_f16(p, p, p, Bm, N, K, 0, 0, L.ptr(y.t), s), "gemv", f"gemv Bm={Bm} N={N} K={K}")
        y.untouched(f"gemv Bm={Bm} N={N} K={K}")
    for args, what in (((p, null, 1, 4, 4, 8, 12, 1, 0), "Cout 12"), ((p, null, 1, 4, 4, 8, 8, 3, 0), "stride 3"), ((p, null, 1, 4, 4, 8, 8, 0, 0), "stride 0"),
                       ((p, p, 1, 4, 4, 8, 8, 1, 0), "both inputs"), ((null, null, 1, 4, 4, 8, 8, 1, 0), "no input")):
        y = out()
        x32, x16 = args[:2]
        _refused(lib, lib.ctx_conv_small_f16(x32, x16, p, p, *args[2:], L.ptr(y.t), s), "conv_small", f"conv_small {what}")
        y.untouched(f"conv_small {what}")
    for nh, B, Cc, HW in R.POINTWISE_REFUSED:
        y = out()
        _refused(lib, lib.ctx_pointwise_f32(p, p, p, B, Cc, HW, nh, L.ptr(y.t), s), "pointwise", f"pointwise nhwc16={nh} C={Cc}")
        y.untouched(f"pointwise nhwc16={nh} C={Cc}")
    for n in R.ADD_SCALED_REFUSED:
        y = out()
        _refused(lib, lib.ctx_add_scaled_f16(L.ptr(y.t), p, 1.0, n, s), "add_scaled", f"add_scaled n={n}")
        y.untouched(f"add_scaled n={n}")
    for M, Ca, Cb in R.CONCAT_REFUSED:
        y = out()
        _refused(lib, lib.ctx_concat_f16(p, p, M, Ca, Cb, L.ptr(y.t), s), "concat", f"concat M={M} Ca={Ca} Cb={Cb}")
        y.untouched(f"concat M={M} Ca={Ca} Cb={Cb}")
    for B, dim in R.TIME_EMBED_REFUSED:
        y = out()
        _refused(lib, lib.ctx_time_embed_f16(p, B, dim, L.ptr(y.t), s), "time_embed", f"time_embed B={B} dim={dim}")
        y.untouched(f"time_embed B={B} dim={dim}")
    for kind, a, b in R.PACK_REFUSED:
        y = out()
        _refused(lib, lib.ctx_pack_fwd_f16(p, kind, a, b, L.ptr(y.t), s), "pack", f"pack kind={kind} a={a} b={b}")
        y.untouched(f"pack kind={kind} a={a} b={b}")
    y = out()
    _refused(lib, lib.ctx_f16_to_f32(p, 12, L.ptr(y.t), s), "f16_to_f32", "f16_to_f32 n=12")
    _refused(lib, lib.ctx_f32_to_f16(p, 0, L.ptr(y.t), s), "f32_to_f16", "f32_to_f16 n=0")
    y.untouched("the converters")


# ---- the seams against the engine ---------------------------------------------------------------------------------------------------------
def test_conv_in_seam_equals_the_unets_first_tap(dev):
    """ctx_pack_fwd_f16 (conv_in pack) + ctx_conv_in_f16 on a tiny UNet's conv_in parameters == the first tap of ctx_unet_set_taps on
    that UNet's forward, bit for bit: the seam and the engine launch the same thing.  (fp16 stream: in the fp32 residual-stream mode
    the tap API records nothing.)"""
    from contexture_nerf_amd.unet import UNet2DConditionModel
    from oracle import unet_ref
    L, lib = _lib()
    cfg = unet_ref.tiny_config()
    torch.manual_seed(0)
    ref = unet_ref.randomize_affine(unet_ref.UNet2DConditionModelRef(cfg)).eval()
    sd = ref.state_dict()
    net = UNet2DConditionModel(cfg, device=dev, init=False)
    net.load_state_dict(sd)
    B, Cin, H, W = 2, cfg["in_channels"], 16, 16
    C0 = cfg["block_out_channels"][0]
    g = R.gen(21000)
    x, ctx = torch.randn(B, Cin, H, W, generator=g).to(dev), torch.randn(B, 7, cfg["cross_attention_dim"], generator=g).to(dev)
    cap = 1 << 22
    buf = torch.zeros(cap, dtype=f16, device=dev)
    L.check(lib.ctx_unet_set_taps(net._h, L.ptr(buf), cap))
    try:
        net(x, 481.0, ctx)
        torch.cuda.synchronize()
        off, rows, ch = C.c_int64(), C.c_int32(), C.c_int32()
        assert lib.ctx_unet_tap_count(net._h) > 0
        L.check(lib.ctx_unet_tap_info(net._h, 0, C.byref(off), C.byref(rows), C.byref(ch)))
    finally:
        L.check(lib.ctx_unet_set_taps(net._h, None, 0))
    assert (off.value, rows.value, ch.value) == (0, B * H * W, C0)
    tap = buf[:B * H * W * C0].cpu()
    w = sd["conv_in.weight"].float()
    pack, want_pack = _pack_fwd(dev, (R.PK_CONVIN, C0, Cin), w)
    assert torch.equal(R.bits(pack), R.bits(want_pack))
    wd, bd = pack.to(dev), sd["conv_in.bias"].half().to(dev)
    y = Out(dev, (B * H * W * C0,), f16)
    L.check(lib.ctx_conv_in_f16(L.ptr(x), L.ptr(wd), L.ptr(bd), B, Cin, H, W, C0, L.ptr(y.t), L.stream()))
    assert torch.equal(R.bits(y.cpu("conv_in of the tiny UNet")), R.bits(tap)), "the conv_in seam and the engine's conv_in differ"
