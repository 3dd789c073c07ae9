"""GroupNorm statistics from the producer: the (sum, sum of squares) partials written by the 144 x 160 kernels' epilogue and by the
split-K reduce (GemmArgs::gn_part), the apply pass on them, the one-kernel GroupNorm over unreduced split-K slabs, and the engine
with and without them (CTX_GN_EPI)."""
import ctypes as C
import functools
import os
import subprocess
import sys
import tempfile

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 32


def _lib():
    from contexture_nerf_amd import _lib as L
    return L, L.load()


def _ran():
    L, lib = _lib()
    t, u = C.c_int32(-2), C.c_int32(-2)
    lib.ctx_gemm_last_kernel(C.byref(t), C.byref(u))
    return t.value, u.value


@functools.lru_cache(maxsize=None)
def _operands(B, H, W, Cin, Cout):
    """fp16 operands of one convolution (NHWC / [Cout][3][3][Cin]), on the CPU; made once per shape."""
    g = torch.Generator().manual_seed(B * H + W + Cin + Cout)
    return dict(x=torch.randn(B, H, W, Cin, generator=g).half(), w=(torch.randn(Cout, 3, 3, Cin, generator=g) / (9 * Cin) ** 0.5).half(),
                bias=torch.randn(Cout, generator=g).half(), bias2=torch.randn(Cout, generator=g).half(), rowb=torch.randn(B, Cout, generator=g).half(),
                res=torch.randn(B, H, W, Cout, generator=g).half(), gamma=(1 + 0.2 * torch.randn(Cout, generator=g)).half(),
                beta=(0.2 * torch.randn(Cout, generator=g)).half())


class _Conv:
    """One convolution's operands on the device and the calls the tests make on them."""

    def __init__(self, dev, shape, groups=G, max_split=1):
        self.shape, self.groups, self.dev = shape, groups, dev
        B, H, W, Cin, Cout = shape
        self.d = {k: v.to(dev) for k, v in _operands(*shape).items()}
        self.part = torch.empty(max_split * B * H * W * Cout, dtype=torch.float32, device=dev) if max_split > 1 else None
        L, lib = _lib()
        self.ws = torch.zeros(lib.ctx_groupnorm_ws_bytes(B, groups) // 4, dtype=torch.float32, device=dev)

    def run(self, request, S=1, keep=False, bias2=False, rowb=True, res=True):
        """-> (y [B,H,W,Cout], slots per sample written: 0 = no request or declined)"""
        L, lib = _lib()
        B, H, W, Cin, Cout = self.shape
        d = self.d
        y = torch.zeros(B, H, W, Cout, dtype=torch.float16, device=self.dev)
        slots = C.c_int32(-1)
        if request:
            self.ws.fill_(float("nan"))                    # a slot nobody writes shows
        L.check(lib.ctx_conv3x3_gn_f16(L.ptr(d["x"]), L.ptr(d["w"]), L.ptr(d["bias"]), L.ptr(d["bias2"]) if bias2 else None,
                                       L.ptr(d["rowb"]) if rowb else None, L.ptr(d["res"]) if res else None, B, H, W, Cin, Cout,
                                       L.ptr(self.part) if S > 1 else None, S, 1 if keep else 0, self.groups, L.ptr(self.ws) if request else None,
                                       C.byref(slots), None if keep else L.ptr(y), L.stream()))
        return y, slots.value

    def partials(self, slots):
        B, Cout = self.shape[0], self.shape[4]
        return self.ws[:B * slots * self.groups * 2].view(B, slots, self.groups, 2).clone()

    def groupnorm(self, y, silu, slots=0):
        """What the engine does behind the producer: the apply pass on its partials, or the whole GroupNorm after a decline."""
        L, lib = _lib()
        B, H, W, Cin, Cout = self.shape
        o = torch.zeros_like(y)
        if slots:
            L.check(lib.ctx_groupnorm_apply_f16(L.ptr(y), L.ptr(self.ws), slots, L.ptr(self.d["gamma"]), L.ptr(self.d["beta"]), B, H * W, Cout,
                                                self.groups, 1e-5, silu, L.ptr(o), L.stream()))
        else:
            ws = torch.empty(lib.ctx_groupnorm_ws_bytes(B, self.groups), dtype=torch.uint8, device=self.dev)
            L.check(lib.ctx_groupnorm_f16(L.ptr(y), L.ptr(self.d["gamma"]), L.ptr(self.d["beta"]), B, H * W, Cout, self.groups, 1e-5, silu,
                                          L.ptr(o), L.ptr(ws), L.stream()))
        return o


def _check_partials(t, y, part, slots, chain, what):
    """The slot partials, folded in slot order in fp32, against float64 sums of the kernel's own fp16 output: within
    chain * 2^-24 * sum|x| (resp. sum x^2), chain = the longest chain of fp32 additions behind one group's sum."""
    B, H, W, Cin, Cout = t.shape
    cg = Cout // t.groups
    assert torch.isfinite(part).all(), f"{what}: a slot was not written"
    acc = part[:, 0].clone()
    for s in range(1, slots):
        acc = acc + part[:, s]
    yd = y.double().view(B, H * W, t.groups, cg)
    s1, sa, s2 = yd.sum((1, 3)), yd.abs().sum((1, 3)), (yd * yd).sum((1, 3))
    e1, e2 = (acc[..., 0].double() - s1).abs(), (acc[..., 1].double() - s2).abs()
    u = chain * 2.0 ** -24
    print(f"{what}: chain {chain}, max |err sum| / bound {(e1 / (u * sa)).max().item():.3f}, max |err sumsq| / bound {(e2 / (u * s2)).max().item():.3f}")
    assert (e1 <= u * sa).all() and (e2 <= u * s2).all(), f"{what}: partials off the float64 sums"


def _chain144(cg, rows, slots):
    """gemm144.hip's staged epilogue: a thread adds its `rows` / 48 rows (the row walk: 3, or 6 on the 288-row tile), step A adds
    LPA = 8 pixel lanes, step B lets a lane add ceil(6 cg / 8) cells and the shuffle tree adds 3 levels; one rounding of each square;
    then this test's fold over the slots."""
    return rows // 48 + 8 + -(-6 * cg // 8) + 3 + 1 + slots


def _chain_reduce(cg, hw, B, Cout, slots):
    """k_splitk_reduce_gn (gemm.hip): a thread adds ceil(RB / PL) rows, the channel fold adds PL row lanes, a lane adds ceil(cg / 8)
    channels, the shuffle tree 3 levels; one rounding of each square; then this test's fold over the slots."""
    rb = hw // slots
    pl = min(rb, 1024 // (Cout // 4))
    return -(-rb // pl) + pl + -(-cg // 8) + 3 + 1 + slots


SHAPES = [(2, 12, 12, 64, 320),      # one tile per sample, two N tiles, 10-channel groups
          (2, 24, 24, 64, 640),      # four tiles per sample, 20-channel groups
          (2, 12, 12, 64, 1280)]     # 40-channel groups
CASES = [(s, u8) for s in SHAPES for u8 in (5, 6, 7)] + [((2, 24, 24, 64, 320), 8)]      # the 288-row form where 288 divides 576
_id = lambda c: "x".join(str(v) for v in c[0]) + f"-form{c[1]}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_partials_from_conv_epilogue(dev, case):
    """Bias + row bias + residual; the output equals the unrequested call's, the partials match the output's own sums, and five
    launches give the same partials (every slot has one writer and the fold order is fixed)."""
    L, lib = _lib()
    shape, use8 = case
    B, H, W, Cin, Cout = shape
    t = _Conv(dev, shape)
    rows = 288 if use8 == 8 else 144
    lib.ctx_gemm_tune(-1, use8)
    try:
        plain, none = t.run(False)
        assert _ran()[1] == use8 and none == 0
        y, slots = t.run(True)
        assert _ran()[1] == use8
        assert slots == H * W // rows, f"form {use8} on {shape}: {slots} slots"
        assert torch.equal(y, plain), "the request changed the convolution's output"
        part = t.partials(slots)
        _check_partials(t, y, part, slots, _chain144(Cout // G, rows, slots), f"conv {shape} form {use8}")
        for k in range(4):
            y2, s2 = t.run(True)
            assert s2 == slots and torch.equal(t.partials(slots), part), f"launch {k + 1}: partials differ from launch 0"
            assert torch.equal(y2, plain)
    finally:
        lib.ctx_gemm_tune(-1, -1)


# (shape, (tile, use8), groups): HW = 117 is no multiple of 144; N = 136 has a masked tail (17-channel groups); the 288-row tile spans
# both samples at HW = 144; a 64-column tile straddles 10-channel groups
DECLINES = [((1, 9, 13, 128, 320), (-1, 6), 32), ((2, 12, 12, 64, 136), (-1, 6), 8), ((2, 12, 12, 64, 320), (-1, 8), 32),
            ((2, 12, 12, 64, 320), (15, 0), 32)]


@pytest.mark.parametrize("shape,force,groups", DECLINES, ids=lambda v: "x".join(str(x) for x in v) if isinstance(v, tuple) else str(v))
def test_declined_requests(dev, shape, force, groups):
    L, lib = _lib()
    t = _Conv(dev, shape, groups)
    lib.ctx_gemm_tune(*force)
    try:
        plain, _ = t.run(False)
        y, slots = t.run(True)
        ran = _ran()
        assert ran == (force[0], 0) if force[0] >= 0 else ran[1] == force[1], f"forced {force}, ran {ran}"
        assert slots == 0, f"{shape} forced {force}: the request was honoured with {slots} slots"
        assert torch.equal(y, plain)
        for silu in (0, 1):
            assert torch.equal(t.groupnorm(y, silu, slots), t.groupnorm(plain, silu))
    finally:
        lib.ctx_gemm_tune(-1, -1)


@pytest.mark.parametrize("force", [(-1, 6), (15, 0)], ids=lambda f: f"tile{f[0]}use8{f[1]}")
@pytest.mark.parametrize("S", [2, 3])
def test_partials_from_splitk_reduce(dev, S, force):
    L, lib = _lib()
    shape = (2, 24, 24, 64, 640)
    B, H, W, Cin, Cout = shape
    t = _Conv(dev, shape, max_split=3)
    lib.ctx_gemm_tune(*force)
    try:
        plain, _ = t.run(False, S)
        y, slots = t.run(True, S)
        assert slots > 0 and (H * W) % slots == 0 and slots <= 128, f"split {S}: {slots} slots"
        assert torch.equal(y, plain), "the request changed the reduce's output"
        part = t.partials(slots)
        _check_partials(t, y, part, slots, _chain_reduce(Cout // G, H * W, B, Cout, slots), f"reduce split {S} forced {force}")
        for k in range(4):
            y2, s2 = t.run(True, S)
            assert s2 == slots and torch.equal(t.partials(slots), part), f"launch {k + 1}: partials differ from launch 0"
        for silu in (0, 1):
            _groupnorm_close(t, y, slots, silu, f"reduce split {S}")
    finally:
        lib.ctx_gemm_tune(-1, -1)


def _groupnorm_close(t, y, slots, silu, what):
    """The apply pass on the producer's partials against F.group_norm in fp32 of the producer's fp16 output, with test_groupnorm's
    bound (rtol 2e-3, atol 2e-3); prints how many elements differ from the two-kernel GroupNorm."""
    B, H, W, Cin, Cout = t.shape
    got = t.groupnorm(y, silu, slots)
    want = F.group_norm(y.float().view(B, H * W, Cout).permute(0, 2, 1), t.groups, t.d["gamma"].float(), t.d["beta"].float(), eps=1e-5)
    if silu:
        want = F.silu(want)
    want = want.permute(0, 2, 1).reshape(B, H, W, Cout)
    err = (got.float() - want).abs()
    bad = (err > 2e-3 + 2e-3 * want.abs()).sum().item()
    two = t.groupnorm(y, silu)
    print(f"{what} silu {silu}: {(got != two).sum().item()} of {got.numel()} elements differ from the two-kernel GroupNorm, max err {err.max().item():.3e}")
    assert bad == 0, f"{what}: {bad}/{got.numel()} off; max err {err.max():.4e}"


@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_groupnorm_on_producer_partials(dev, shape, silu):
    L, lib = _lib()
    t = _Conv(dev, shape)
    lib.ctx_gemm_tune(-1, 6)
    try:
        y, slots = t.run(True)
        assert slots > 0
        _groupnorm_close(t, y, slots, silu, f"groupnorm on partials {shape}")
    finally:
        lib.ctx_gemm_tune(-1, -1)


@pytest.mark.parametrize("extra", [False, True], ids=["bias", "bias+bias2+rowbias"])
@pytest.mark.parametrize("shape", [(2, 12, 12, 64, 1280), (2, 24, 24, 64, 1280)], ids=lambda s: "x".join(str(v) for v in s))
def test_groupnorm_from_slabs(dev, shape, extra):
    """The one-kernel GroupNorm over unreduced split-K slabs is bit-identical to the reduce followed by ctx_groupnorm_f16."""
    L, lib = _lib()
    B, H, W, Cin, Cout = shape
    t = _Conv(dev, shape, max_split=5)
    d = t.d
    for S in (2, 3, 5):
        y, _ = t.run(False, S, bias2=extra, rowb=extra, res=False)
        for silu in (0, 1):
            want = t.groupnorm(y, silu)
            t.run(False, S, keep=True, bias2=extra, rowb=extra, res=False)
            got = torch.zeros_like(y)
            L.check(lib.ctx_groupnorm_slabs_f16(L.ptr(t.part), S, L.ptr(d["bias"]), L.ptr(d["bias2"]) if extra else None,
                                                L.ptr(d["rowb"]) if extra else None, Cout, L.ptr(d["gamma"]), L.ptr(d["beta"]), B, H * W, Cout, G,
                                                1e-5, silu, L.ptr(got), L.stream()))
            assert torch.isfinite(got.float()).all()
            assert torch.equal(got, want), f"{shape} split {S} silu {silu}: {(got != want).sum().item()} elements differ"


_CHILD = r"""
import ctypes as C, sys, torch
sys.path.insert(0, sys.argv[1])
from contexture_nerf_amd.unet import UNet2DConditionModel
from oracle import unet_ref
cfg = unet_ref.tiny_config(ch=(64, 128, 256, 256), heads=(1, 2, 4, 4), ctx_dim=128)
torch.manual_seed(1)
ref = unet_ref.randomize_affine(unet_ref.UNet2DConditionModelRef(cfg)).eval()
dev = torch.device("cuda:0")
net = UNet2DConditionModel(cfg, device=dev, init=False)
net.load_state_dict(ref.state_dict())
g = torch.Generator().manual_seed(2)
x = torch.randn(2, 5, 16, 16, generator=g)
ctx = torch.randn(2, 77, cfg['cross_attention_dim'], generator=g)
got = net(x.to(dev), 981.0, ctx.to(dev))['sample'].float().cpu()
a, b = C.c_int64(-1), C.c_int64(-1)
assert net._lib.ctx_unet_gn_epilogue_counts(net._h, C.byref(a), C.byref(b)) == 0
with torch.no_grad():
    want = ref(x, torch.tensor(981.0), ctx)['sample']
torch.save({'got': got, 'want': want, 'from_producer': a.value, 'from_slabs': b.value}, sys.argv[2])
"""


def test_engine_gn_epilogue_switch(dev):
    """The tiny UNet (channels 64 / 128 / 256 / 256, 32 groups, latent 16, batch 2) in fresh child processes (the switch is read once).
    At these widths both parts occur: the 64- and 128-channel levels have 2- and 4-channel groups (two-pass GroupNorm) behind split-K
    convolutions, whose reduce writes the partials; the 256-channel levels have 8-channel groups (one-kernel GroupNorm) behind split-K
    conv1s.  CTX_GN_EPI = 0 is the graph without either; 3 (slabs only) moves no rounding point and must equal it bit for bit; the
    default (partials only: the slabs measured slower) and 1 (both) may be at most 1.10 x its relative L2 against the fp32 oracle (the
    statistics are summed in another order: the margin of tests/test_precision_cpu.py for decorrelated fp16 roundings)."""
    outs = {}
    with tempfile.TemporaryDirectory() as td:
        for mode in ("0", "3", "1", None):
            env = dict(os.environ)
            env.pop("CTX_GN_EPI", None)
            if mode is not None:
                env["CTX_GN_EPI"] = mode
            path = os.path.join(td, f"out_{mode}.pt")
            r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path], env=env, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            outs[mode] = torch.load(path)
    for mode, o in outs.items():
        print(f"CTX_GN_EPI={mode}: GroupNorms on producer partials {o['from_producer']}, on split-K slabs {o['from_slabs']}")
    assert (outs["0"]["from_producer"], outs["0"]["from_slabs"]) == (0, 0)
    assert outs["3"]["from_producer"] == 0 and outs["3"]["from_slabs"] > 0, "no conv1 kept its slabs at these widths"
    assert outs[None]["from_producer"] > 0 and outs[None]["from_slabs"] == 0, "no producer wrote partials at these widths"
    assert outs["1"]["from_producer"] == outs[None]["from_producer"] and outs["1"]["from_slabs"] == outs["3"]["from_slabs"]
    want = outs["0"]["want"]
    assert torch.equal(outs["3"]["got"], outs["0"]["got"]), "GroupNorm from slabs changed the engine's output"
    assert torch.equal(outs["1"]["got"], outs[None]["got"]), "GroupNorm from slabs changed the output behind the partials"
    rel = lambda t: ((t - want).norm() / want.norm()).item()
    r0, r1 = rel(outs["0"]["got"]), rel(outs[None]["got"])
    print(f"tiny UNet vs fp32 oracle: rel L2 with CTX_GN_EPI=0 {r0:.4e}, default {r1:.4e} (ratio {r1 / r0:.3f})")
    assert torch.isfinite(outs[None]["got"]).all()
    assert r1 <= 1.10 * r0, f"default {r1:.4e} vs {r0:.4e} with CTX_GN_EPI=0"
