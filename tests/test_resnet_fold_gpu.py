"""The resnet fold on the GPU: K segments of the implicit-GEMM convolution (the 1x1 shortcut inside conv2's K loop), GroupNorm
over two sources (the up blocks' [hidden ; skip] read in place) and the engine with and without them (CTX_RESNET_FOLD)."""
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
# (tile, use8) of ctx_gemm_tune: gemm.hip 128x128 32-deep, 64x64 64-deep and tile 27 (256x320; all three with the LDS-staged epilogue
# at these strides), gemm144.hip forms 5 .. 8, and the heuristic
FORMS = [(1, 0), (15, 0), (27, 0), (-1, 5), (-1, 6), (-1, 7), (-1, 8), (-1, -1)]
SPLITS = (1, 2, 3, 5)


def _lib():
    from contexture_nerf_amd import _lib as L
    return L, L.load()


def _check(got, want, what):
    """The bound of test_unet_gpu.test_conv3x3 (rtol 3e-3, atol 4e-3): one rounding of an fp32 sum."""
    got, want = got.float().cpu(), want.float()
    err = (got - want).abs()
    bad = (err > 4e-3 + 3e-3 * want.abs()).sum().item()
    assert bad == 0, f"{what}: {bad}/{got.numel()} off; max err {err.max():.4e}, rel L2 {(got - want).norm() / want.norm():.3e}"


@functools.lru_cache(maxsize=None)
def _problem(B, H, W, Cin, Cout, segs):
    """fp16-rounded operands (NHWC / [Cout][3][3][Cin] / W_sc [Cout][Ca + Cb]) and the fp32 pieces of the reference, on the CPU."""
    g = torch.Generator().manual_seed(B * H + Cin + Cout + sum(segs))
    x = torch.randn(B, Cin, H, W, generator=g).half()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5).half()
    csum = sum(segs)
    xs = [torch.randn(B, c, H, W, generator=g).half() for c in segs]
    wsc = (torch.randn(Cout, csum, generator=g) / csum ** 0.5).half()
    bias, bias2 = torch.randn(Cout, generator=g).half(), torch.randn(Cout, generator=g).half()
    rowb = torch.randn(B, Cout, generator=g).half()
    res = torch.randn(B, Cout, H, W, generator=g).half()
    conv = F.conv2d(x.float(), w.float(), None, padding=1)
    sc = F.conv2d(torch.cat([t.float() for t in xs], 1), wsc.float()[:, :, None, None])
    first = F.conv2d(xs[0].float(), wsc.float()[:, :segs[0], None, None])
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    return dict(x=nhwc(x), w=nhwc(w), xs=[nhwc(t) for t in xs], wsc=wsc, bias=bias, bias2=bias2, rowb=rowb, res=nhwc(res),
                conv=conv, sc=sc, first=first, res_nchw=res.float())


def _want(p, nseg=None, bias=True, bias2=True, rowb=True, res=True):
    w = p["conv"] + (p["first"] if nseg == 1 else p["sc"])
    if bias:
        w = w + p["bias"].float()[None, :, None, None]
    if bias2:
        w = w + p["bias2"].float()[None, :, None, None]
    if rowb:
        w = w + p["rowb"].float()[:, :, None, None]
    if res:
        w = w + p["res_nchw"]
    return w


class _Dev:
    """The problem's operands on the device, and the call."""

    def __init__(self, dev, p, shape, max_split=32):
        self.B, self.H, self.W, self.Cin, self.Cout, self.segs = shape
        self.d = {k: p[k].to(dev) for k in ("x", "w", "wsc", "bias", "bias2", "rowb", "res")}
        self.xs = [t.to(dev) for t in p["xs"]]
        self.part = torch.empty(max_split * self.B * self.H * self.W * self.Cout, dtype=torch.float32, device=dev)
        self.dev = dev

    def run(self, splitk=1, nseg=None, bias=True, bias2=True, rowb=True, res=True):
        L, lib = _lib()
        d, segs = self.d, self.segs
        nseg = len(segs) if nseg is None else nseg
        ld = sum(segs)
        y = torch.zeros(self.B, self.H, self.W, self.Cout, dtype=torch.float16, device=self.dev)
        wb = C.c_void_p(d["wsc"].data_ptr() + 2 * segs[0]) if nseg == 2 else None      # columns Ca .. Ca + Cb of the same matrix
        L.check(lib.ctx_conv3x3_seg_f16(L.ptr(d["x"]), L.ptr(d["w"]), L.ptr(d["bias"]) if bias else None, L.ptr(d["bias2"]) if bias2 else None,
                                        L.ptr(d["rowb"]) if rowb else None, L.ptr(d["res"]) if res else None, self.B, self.H, self.W,
                                        self.Cin, self.Cout, L.ptr(self.xs[0]), L.ptr(d["wsc"]), segs[0], ld,
                                        L.ptr(self.xs[1]) if nseg == 2 else None, wb, segs[1] if nseg == 2 else 0, ld,
                                        L.ptr(self.part) if splitk != 1 else None, splitk, L.ptr(y), L.stream()))
        return y.permute(0, 3, 1, 2)


# the (32, 96) segments are whole 32-deep stages only: the 64-deep tiles and gemm144.hip must hand the problem to a 32-deep tile
SHAPES = [(2, 12, 12, 64, 160, (64,)), (2, 12, 12, 64, 160, (64, 128)), (1, 9, 13, 128, 320, (128, 64)), (2, 24, 24, 320, 320, (320, 640)),
          (2, 12, 12, 64, 160, (32, 96))]


def _ran():
    """(tile, use8) of the kernel the last dispatch launched."""
    L, lib = _lib()
    t, u = C.c_int32(-2), C.c_int32(-2)
    lib.ctx_gemm_last_kernel(C.byref(t), C.byref(u))
    return t.value, u.value


def _assert_ran(shape, tile, use8, what):
    """The forced kernel ran; or, where it cannot take the segments (not whole 64-deep stages), a 32-deep tile of gemm.hip did."""
    rt, ru = _ran()
    seg64 = all(c % 64 == 0 for c in shape[5])
    if not seg64:
        assert ru == 0 and 0 <= rt < 10, f"{what}: ran tile {rt} use8 {ru}, expected a 32-deep tile of gemm.hip"
    elif use8 >= 4:
        assert ru == use8, f"{what}: ran tile {rt} use8 {ru}, expected gemm144 form {use8}"
    elif tile >= 0:
        assert (rt, ru) == (tile, 0), f"{what}: ran tile {rt} use8 {ru}, expected tile {tile}"


@pytest.mark.parametrize("tile,use8", FORMS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s[:5]) + "+" + "+".join(str(v) for v in s[5]))
def test_segmented_conv(dev, shape, tile, use8):
    """conv3x3 + the 1x1 products + both biases + row bias + residual against torch in fp32, every kernel form, split-K 1 / 2 / 3 / 5
    (and 4 / 6: with 64-deep stages the last shape's slices then start on the 3x3 | segment a and the a | b boundaries)."""
    L, lib = _lib()
    p = _problem(*shape)
    t = _Dev(dev, p, shape)
    want = _want(p)
    lib.ctx_gemm_tune(tile, use8)
    try:
        for S in SPLITS + (4, 6):
            _check(t.run(S), want, f"seg conv {shape} tile {tile} use8 {use8} split {S}")
            _assert_ran(shape, tile, use8, f"seg conv {shape} tile {tile} use8 {use8} split {S}")
        _check(t.run(-1), want, f"seg conv {shape} tile {tile} use8 {use8} planned split")
    finally:
        lib.ctx_gemm_tune(-1, -1)


@pytest.mark.parametrize("tile,use8", [(1, 0), (-1, 6), (-1, 8), (-1, -1)])
def test_segmented_conv_operands(dev, tile, use8):
    """One segment only of a two-segment problem; no bias; no second bias; no row bias; no residual; nothing but the products."""
    L, lib = _lib()
    shape = SHAPES[2]
    p = _problem(*shape)
    t = _Dev(dev, p, shape)
    lib.ctx_gemm_tune(tile, use8)
    try:
        for S in (1, 3):
            _check(t.run(S, nseg=1), _want(p, nseg=1), f"one segment, split {S}")
            for off in ("bias", "bias2", "rowb", "res"):
                kw = {off: False}
                _check(t.run(S, **kw), _want(p, **kw), f"no {off}, split {S}")
            none = dict(bias=False, bias2=False, rowb=False, res=False)
            _check(t.run(S, **none), _want(p, **none), f"products only, split {S}")
    finally:
        lib.ctx_gemm_tune(-1, -1)


@pytest.mark.parametrize("use8", [1, 2, 3])
def test_segmented_conv_declined_kernels(dev, use8):
    """gemm8.hip / conv_halo.hip forced: they decline a segmented problem, and the call still computes it through another kernel."""
    L, lib = _lib()
    shape = (2, 16, 16, 64, 128, (64, 128))                # 16-multiples: a shape conv_halo would take
    p = _problem(*shape)
    t = _Dev(dev, p, shape)
    lib.ctx_gemm_tune(-1, use8)
    try:
        for S in (1, 2):
            _check(t.run(S), _want(p), f"forced use8 {use8}, split {S}")
            assert _ran()[1] == 0, f"forced use8 {use8}: a kernel that does not take K segments ran ({_ran()})"
    finally:
        lib.ctx_gemm_tune(-1, -1)


def test_segmented_conv_repeat(dev):
    """One UNet-sized problem (B 2, 48 x 48, 640 <- 640 + (640, 320)): five launches per form and split, each within the bound and
    all five equal (a stage refilled before its readers are done shows as a launch that differs)."""
    L, lib = _lib()
    shape = (2, 48, 48, 640, 640, (640, 320))
    p = _problem(*shape)
    t = _Dev(dev, p, shape, max_split=max(SPLITS))
    want = _want(p)
    try:
        for tile, use8 in FORMS:
            lib.ctx_gemm_tune(tile, use8)
            for S in SPLITS:
                outs = [t.run(S).clone() for _ in range(5)]
                _assert_ran(shape, tile, use8, f"repeat tile {tile} use8 {use8} split {S}")
                torch.cuda.synchronize()
                for k, o in enumerate(outs):
                    _check(o, want, f"repeat tile {tile} use8 {use8} split {S} launch {k}")
                    assert torch.equal(o, outs[0]), f"repeat tile {tile} use8 {use8} split {S}: launch {k} differs from launch 0"
    finally:
        lib.ctx_gemm_tune(-1, -1)


@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("B,HW,Ca,Cb,G", [(2, 144, 1280, 1280, 32),     # one-kernel form, the boundary is a group boundary
                                           (2, 576, 1280, 640, 32),      # two-kernel form, a group straddles the boundary
                                           (2, 2304, 320, 320, 32),      # 20 channels per group
                                           (1, 100, 64, 32, 8)])
def test_groupnorm_two_sources(dev, B, HW, Ca, Cb, G, silu):
    """Bit-identical to the one-source GroupNorm of the materialised concat."""
    L, lib = _lib()
    g = torch.Generator().manual_seed(HW + Ca + Cb)
    Cc = Ca + Cb
    xa = (torch.randn(B, HW, Ca, generator=g) * 1.5 + 0.3).half().to(dev)
    xb = (torch.randn(B, HW, Cb, generator=g) * 0.7 - 0.2).half().to(dev)
    gamma, beta = torch.randn(Cc, generator=g).half().to(dev), torch.randn(Cc, generator=g).half().to(dev)
    ws = torch.empty(lib.ctx_groupnorm_ws_bytes(B, G), dtype=torch.uint8, device=dev)
    cat = torch.cat([xa, xb], 2).contiguous()
    y1 = torch.zeros(B, HW, Cc, dtype=torch.float16, device=dev)
    y2 = torch.ones(B, HW, Cc, dtype=torch.float16, device=dev)
    L.check(lib.ctx_groupnorm_f16(L.ptr(cat), L.ptr(gamma), L.ptr(beta), B, HW, Cc, G, 1e-5, silu, L.ptr(y1), L.ptr(ws), L.stream()))
    L.check(lib.ctx_groupnorm2_f16(L.ptr(xa), L.ptr(xb), Ca, L.ptr(gamma), L.ptr(beta), B, HW, Cc, G, 1e-5, silu, L.ptr(y2), L.ptr(ws),
                                   L.stream()))
    assert torch.isfinite(y1.float()).all()
    assert torch.equal(y1, y2)


_CHILD = r"""
import sys, torch
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
with torch.no_grad():
    want = ref(x, torch.tensor(981.0), ctx)['sample']
torch.save({'got': got, 'want': want}, sys.argv[2])
"""


def test_engine_fold_switch(dev):
    """The tiny UNet (channels 64 / 128 / 256 / 256, latent 16, batch 2) in fresh child processes (the switch is read once):
    CTX_RESNET_FOLD = 0 (the graph without either piece), 2 (concat read in place, shortcut not folded: bit-identical to 0) and the
    default.  Against the fp32 oracle the fold's relative L2 may be at most 1.10 x that of the path without it: it removes one fp16
    rounding per resnet, and 10 % covers the decorrelation of fp16 roundings (tests/test_precision_cpu.py)."""
    outs = {}
    with tempfile.TemporaryDirectory() as td:
        for mode in ("0", "2", None):
            env = dict(os.environ)
            env.pop("CTX_RESNET_FOLD", None)
            if mode is not None:
                env["CTX_RESNET_FOLD"] = mode
            path = os.path.join(td, f"out_{mode}.pt")
            r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path], env=env, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            outs[mode] = torch.load(path)
    want = outs["0"]["want"]
    assert torch.equal(outs["0"]["got"], outs["2"]["got"]), "concat in place changed the engine's output"
    rel = lambda t: ((t - want).norm() / want.norm()).item()
    r0, r1 = rel(outs["0"]["got"]), rel(outs[None]["got"])
    print(f"tiny UNet vs fp32 oracle: rel L2 without the fold {r0:.4e}, with the fold {r1:.4e} (ratio {r1 / r0:.3f})")
    assert torch.isfinite(outs[None]["got"]).all()
    assert r1 <= 1.10 * r0, f"fold {r1:.4e} vs {r0:.4e} without it"
