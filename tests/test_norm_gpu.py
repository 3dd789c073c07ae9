"""GPU: every launch form of the norm kernels (csrc/norm.hip) against the float64 references of tests/norm_rule.py, through its
comparator, on inputs whose groups sit at mean / sigma 0.25 .. 1000 (1e4 for the fp32 input), hold one constant and one with an
outlier column.  tests/test_norm_cpu.py asserts that the case lists reach every class of the launch plans.  Output buffers carry a
guard region that must come back untouched; the statistics workspace starts as NaN."""
import ctypes as C
import functools

import pytest
import torch

import norm_rule as R
import vae_train_rule as VR

pytestmark = pytest.mark.gpu

GUARD = 2048                    # fp16 elements behind every output
SENTINEL = 0x5A5A


def _lib():
    from contexture_nerf_amd import _lib as L
    return L, L.load()


class _Out:
    """an fp16 output of n elements with a guard region behind it"""

    def __init__(self, dev, shape):
        self.shape = tuple(shape)
        self.n = 1
        for s in self.shape:
            self.n *= s
        self.buf = torch.full((self.n + GUARD,), SENTINEL, dtype=torch.int16, device=dev)

    def ptr(self):
        L, _ = _lib()
        return L.ptr(self.buf)

    def result(self, what):
        torch.cuda.synchronize()
        assert bool((self.buf[self.n:] == SENTINEL).all()), f"{what}: wrote behind the output"
        return self.buf[:self.n].view(torch.float16).reshape(self.shape).cpu()


def _ws(dev, B, G):
    L, lib = _lib()
    return torch.full((lib.ctx_groupnorm_ws_bytes(B, G) // 4,), float("nan"), dtype=torch.float32, device=dev)


@functools.lru_cache(maxsize=None)
def _gn_case(B, HW, Cc, G, x32=False):
    x, names = R.gn_input(B, HW, Cc, G, R.KINDS32 if x32 else R.KINDS16, x32)
    gamma, beta = R.affine(Cc)
    return x, names, gamma, beta


def _report(got, want, bound, G, names, what):
    """prints the worst fraction of the bound per input kind, then asserts the whole tensor"""
    per = R.per_group_worst(got, want, bound, G)
    kinds = {}
    for b, row in enumerate(names):
        for g, k in enumerate(row):
            kinds[k] = max(kinds.get(k, 0.0), float(per[b, g]))
    print(f"{what}: " + ", ".join(f"{k} {v:.3f}" for k, v in kinds.items()))
    assert torch.isfinite(got.float()).all(), f"{what}: non-finite output"
    return R.assert_within(got, want, bound, what)


# ---- A. ctx_groupnorm_f16 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("silu", (0, 1))
@pytest.mark.parametrize("case", R.GN_CASES, ids=lambda c: "x".join(str(v) for v in c[:4]))
def test_groupnorm(dev, case, silu):
    L, lib = _lib()
    B, HW, Cc, G, tag = case
    x, names, gamma, beta = _gn_case(B, HW, Cc, G)
    want, bound = R.gn_ref(x, gamma, beta, G, R.GN_EPS, silu)
    y, ws = _Out(dev, (B, HW, Cc)), _ws(dev, B, G)
    xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
    L.check(lib.ctx_groupnorm_f16(L.ptr(xd), L.ptr(gd), L.ptr(bd), B, HW, Cc, G, R.GN_EPS, silu, y.ptr(), L.ptr(ws), L.stream()))
    _report(y.result(tag), want, bound, G, names, f"groupnorm {case[:4]} silu {silu} [{tag}]")


# ---- B. the fp32-input kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.GN32_CASES, ids=lambda c: "x".join(str(v) for v in c[:4]))
def test_groupnorm_f32_input(dev, case):
    L, lib = _lib()
    B, HW, Cc, G, tag = case
    x, names, gamma, beta = _gn_case(B, HW, Cc, G, True)
    assert x.dtype == torch.float32 and any("m1e4" in row for row in names)
    want, bound = R.gn_ref(x, gamma, beta, G, R.GN_EPS, 1)
    y, ws = _Out(dev, (B, HW, Cc)), _ws(dev, B, G)
    xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
    L.check(lib.ctx_groupnorm_f32in_f16(L.ptr(xd), L.ptr(gd), L.ptr(bd), B, HW, Cc, G, R.GN_EPS, 1, y.ptr(), L.ptr(ws), L.stream()))
    _report(y.result(tag), want, bound, G, names, f"groupnorm fp32 input {case[:4]} [{tag}]")


@pytest.mark.parametrize("case", R.LN32_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_layernorm_f32_input(dev, case):
    L, lib = _lib()
    rows, Cc, tag = case
    x, names = R.ln_input(rows, Cc, True)
    assert "m1e4" in names
    gamma, beta = R.affine(Cc)
    want, bound = R.ln_ref(x, gamma, beta)
    y = _Out(dev, (rows, Cc))
    xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
    L.check(lib.ctx_layernorm_f32in_f16(L.ptr(xd), L.ptr(gd), L.ptr(bd), rows, Cc, R.LN_EPS, y.ptr(), L.stream()))
    R.assert_within(y.result(tag), want, bound, f"layernorm fp32 input {rows} x {Cc} [{tag}]")


# ---- C. ctx_groupnorm2_f16 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("silu", (0, 1))
@pytest.mark.parametrize("case", R.GN2_CASES, ids=lambda c: "x".join(str(v) for v in c[:5]))
def test_groupnorm_two_sources(dev, case, silu):
    L, lib = _lib()
    B, HW, Cc, G, Ca, tag = case
    x, names, gamma, beta = _gn_case(B, HW, Cc, G)
    xa, xb = x[..., :Ca].contiguous(), x[..., Ca:].contiguous()
    want, bound = R.gn2_ref(xa, xb, gamma, beta, G, R.GN_EPS, silu)
    y2, y1, ws = _Out(dev, (B, HW, Cc)), _Out(dev, (B, HW, Cc)), _ws(dev, B, G)
    ad, bd_, xd, gd, bd = xa.to(dev), xb.to(dev), x.to(dev), gamma.to(dev), beta.to(dev)
    L.check(lib.ctx_groupnorm2_f16(L.ptr(ad), L.ptr(bd_), Ca, L.ptr(gd), L.ptr(bd), B, HW, Cc, G, R.GN_EPS, silu, y2.ptr(), L.ptr(ws), L.stream()))
    got = y2.result(tag)
    _report(got, want, bound, G, names, f"groupnorm2 {case[:5]} silu {silu} [{tag}]")
    ws.fill_(float("nan"))
    L.check(lib.ctx_groupnorm_f16(L.ptr(xd), L.ptr(gd), L.ptr(bd), B, HW, Cc, G, R.GN_EPS, silu, y1.ptr(), L.ptr(ws), L.stream()))
    assert torch.equal(got, y1.result(tag)), f"{tag}: not bit-identical to GroupNorm of the materialised concat"


# ---- D. ctx_groupnorm_apply_f16 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.APPLY_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_apply_on_hand_made_partials(dev, case):
    L, lib = _lib()
    B, HW, Cc, G, NS = case
    x, names = R.gn_input(B, HW, Cc, G, ("ordinary",))
    gamma, beta = R.affine(Cc)
    part = R.hand_partials(x, G, NS)
    want, bound = R.gn_ref(x, gamma, beta, G, R.GN_EPS, 1)
    y = _Out(dev, (B, HW, Cc))
    xd, pd, gd, bd = x.to(dev), part.to(dev), gamma.to(dev), beta.to(dev)
    L.check(lib.ctx_groupnorm_apply_f16(L.ptr(xd), L.ptr(pd), NS, L.ptr(gd), L.ptr(bd), B, HW, Cc, G, R.GN_EPS, 1, y.ptr(), L.stream()))
    R.assert_within(y.result("apply"), want, bound, f"apply {case}: {R.fold_trips(NS, G)} fold trip(s)")


# the producers of partials: (shape B, H, W, Cin, Cout; forced kernel of ctx_gemm_tune; split-K factor), both from
# tests/test_gn_epilogue_gpu.py's lists: the split-K reduce and the 144 x 160 tile's epilogue
PRODUCERS = [((2, 24, 24, 64, 640), (-1, 6), 2), ((2, 12, 12, 64, 320), (-1, 6), 1)]
PRODUCER_GROUPS = 32


def producer_apply(dev, shape, force, S, ratio, silu=1):
    """A convolution whose output groups sit at mean / sigma ~ ratio (unit-variance output, bias = ratio) writes the GroupNorm
    partials of its own output; the apply pass on them against float64 GroupNorm of that fp16 output.
    -> (the worst element as a fraction of its bound, slots)"""
    L, lib = _lib()
    B, H, W, Cin, Cout = shape
    G = PRODUCER_GROUPS
    g = torch.Generator().manual_seed(77 + H + Cout)
    x = torch.randn(B, H, W, Cin, generator=g).half().to(dev)
    w = (torch.randn(Cout, 3, 3, Cin, generator=g) / (9 * Cin) ** 0.5).half().to(dev)
    bias = torch.full((Cout,), float(ratio)).half().to(dev)
    gamma, beta = R.affine(Cout)
    gd, bd = gamma.to(dev), beta.to(dev)
    part = torch.empty(S * B * H * W * Cout, dtype=torch.float32, device=dev) if S > 1 else None
    ws = _ws(dev, B, G)
    conv, y = _Out(dev, (B, H * W, Cout)), _Out(dev, (B, H * W, Cout))
    slots = C.c_int32(-1)
    lib.ctx_gemm_tune(*force)
    try:
        L.check(lib.ctx_conv3x3_gn_f16(L.ptr(x), L.ptr(w), L.ptr(bias), None, None, None, B, H, W, Cin, Cout, L.ptr(part) if S > 1 else None, S, 0,
                                       G, L.ptr(ws), C.byref(slots), conv.ptr(), L.stream()))
    finally:
        lib.ctx_gemm_tune(-1, -1)
    assert slots.value > 0, f"{shape} forced {force} split {S}: the partials request was declined"
    cd = conv.buf[:conv.n].view(torch.float16)
    L.check(lib.ctx_groupnorm_apply_f16(L.ptr(cd), L.ptr(ws), slots.value, L.ptr(gd), L.ptr(bd), B, H * W, Cout, G, R.GN_EPS, silu, y.ptr(), L.stream()))
    xo = conv.result("conv")
    want, bound = R.gn_ref(xo, gamma, beta, G, R.GN_EPS, silu)
    return R.worst(y.result("apply"), want, bound)[0], slots.value


@pytest.mark.parametrize("shape,force,S", PRODUCERS, ids=["split-K reduce", "gemm144 epilogue"])
def test_apply_on_producer_partials(dev, shape, force, S):
    """mean / sigma ~ 16: the producers' plain (sum, sum of squares) is conditioned to a few tens (CTX_GN_EPI)"""
    r, slots = producer_apply(dev, shape, force, S, 16.0)
    print(f"apply on producer partials {shape} split {S}: {slots} slots, worst element / bound {r:.3f}")
    assert r <= 1.0


# ---- E. ctx_layernorm_f16 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.LN_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_layernorm(dev, case):
    L, lib = _lib()
    rows, Cc, tag = case
    x, names = R.ln_input(rows, Cc)
    gamma, beta = R.affine(Cc)
    want, bound = R.ln_ref(x, gamma, beta)
    y = _Out(dev, (rows, Cc))
    xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
    L.check(lib.ctx_layernorm_f16(L.ptr(xd), L.ptr(gd), L.ptr(bd), rows, Cc, R.LN_EPS, y.ptr(), L.stream()))
    R.assert_within(y.result(tag), want, bound, f"layernorm {rows} x {Cc} [{tag}]")


# ---- F. ctx_groupnorm_bwd_f16 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", R.BWD_RATIOS)
@pytest.mark.parametrize("case", R.BWD_CASES, ids=lambda c: "x".join(str(v) for v in c[:4]))
def test_groupnorm_backward(dev, case, ratio):
    L, lib = _lib()
    B, HW, Cc, G, silu, add = case
    x, dy, gamma, beta, a = R.bwd_inputs(case, ratio)
    want, bound = R.gn_bwd_ref(x, dy, gamma, beta, a, G, silu)
    dx = _Out(dev, (B, HW, Cc))
    ws = torch.full((lib.ctx_groupnorm_bwd_ws_bytes(B, G) // 4,), float("nan"), dtype=torch.float32, device=dev)
    xd, dyd, gd, bd = x.to(dev), dy.to(dev), gamma.to(dev), beta.to(dev)
    ad = a.to(dev) if a is not None else None
    L.check(lib.ctx_groupnorm_bwd_f16(L.ptr(xd), L.ptr(dyd), L.ptr(gd), L.ptr(bd), L.ptr(ad), B, HW, Cc, G, VR.GN_EPS, silu, dx.ptr(), L.ptr(ws),
                                      L.stream()))
    R.assert_within(dx.result("dx"), want, bound, f"groupnorm backward {case} mean/sigma {ratio}")
