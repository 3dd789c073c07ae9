"""The upsampling convolution in its phase form (GemmArgs::phase): nearest x2 upsample + pad-1 3x3 convolution as
four 2x2 convolutions over the source grid, one per output parity, with the weights of ctx_pack_conv3_phase_f16.

References are torch on the CPU in fp32.  The convolution's reference is four F.conv2d over the padded source with the fp16 phase
weights (exactly the products the kernel forms), assembled with y[:, :, a::2, b::2]; each case also pins that reference against
F.conv2d(F.interpolate(x, 2, 'nearest'), w, padding=1) with the fp32 weights, to the distance that rounding the phase weights to
fp16 allows.  Kernel tolerance: rtol 3e-3, atol 4e-3 (fp16 output of an fp32 sum: what test_conv3x3 uses for the nine-tap form)."""
import ctypes as C
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

E_ARG = -1
RSETS = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}


def _lib():
    from contexture_nerf_amd import _lib as L
    return L, L.load()


def phase_pack_ref(w):
    """w f32 [Cout,Cin,3,3] -> f16 [4][Cout][2][2][Cin]: fp32 sums, ky ascending then kx ascending, left to right, rounded once."""
    Cout, Cin = w.shape[:2]
    out = torch.empty(4, Cout, 2, 2, Cin, dtype=torch.float16)
    for a in (0, 1):
        for b in (0, 1):
            for u in (0, 1):
                for v in (0, 1):
                    acc = None
                    for ky in RSETS[(a, u)]:
                        for kx in RSETS[(b, v)]:
                            t = w[:, :, ky, kx].float()
                            acc = t.clone() if acc is None else acc + t
                    out[2 * a + b, :, u, v, :] = acc.half()
    return out


def phase_conv_ref(x, wp, bias):
    """x f32 [B,Cin,H,W] (fp16 values), wp f16 [4][Cout][2][2][Cin] -> f32 [B,Cout,2H,2W]: four 2x2 convolutions over the padded source."""
    B, _, H, W = x.shape
    Cout = wp.shape[1]
    y = torch.empty(B, Cout, 2 * H, 2 * W)
    xp = F.pad(x, (1, 1, 1, 1))
    for a in (0, 1):
        for b in (0, 1):
            k = wp[2 * a + b].float().permute(0, 3, 1, 2).contiguous()           # [Cout,Cin,2,2]
            y[:, :, a::2, b::2] = F.conv2d(xp[:, :, a:a + H + 1, b:b + W + 1], k, bias)
    return y


def _close(got, want, what, rtol=3e-3, atol=4e-3):
    got, want = got.float().cpu(), want.float().cpu()
    err = (got - want).abs()
    bad = (err > atol + rtol * want.abs()).sum().item()
    rel = ((got - want).norm() / want.norm()).item()
    print(f"{what}: max err {err.max():.3e}, rel L2 {rel:.3e}")
    assert bad == 0, f"{what}: {bad}/{got.numel()} off; max err {err.max():.4e}, rel L2 {rel:.3e}"


_cases = {}


def _case(B, H, W, Cin, Cout):
    """Inputs and both references of one shape, computed once and shared (read-only) by the tests that use it."""
    key = (B, H, W, Cin, Cout)
    if key not in _cases:
        g = torch.Generator().manual_seed(B * H + W + Cin + Cout)
        x = torch.randn(B, Cin, H, W, generator=g).half()
        w = torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
        bias = torch.randn(Cout, generator=g).half()
        wp = phase_pack_ref(w)
        want = phase_conv_ref(x.float(), wp, None)
        # the reference itself: against the nine-tap definition with the fp32 weights.  The only difference is the rounding of the
        # phase weights to fp16 (relative 2^-11 each, independent): relative L2 ~ 2^-11 / sqrt(3) = 2.8e-4; 6e-4 is twice that.
        nine = F.conv2d(F.interpolate(x.float(), scale_factor=2.0, mode='nearest'), w, None, padding=1)
        rel = ((want - nine).norm() / nine.norm()).item()
        assert rel < 6e-4, f"phase reference vs nine-tap definition at {key}: rel L2 {rel:.3e}"
        _cases[key] = dict(x=x, w=w, bias=bias, wp=wp, want=want, rel_nine=rel)
    return _cases[key]


def _run(dev, B, H, W, Cin, Cout, with_bias, splitk=1, part_slices=0, rowbias=False, residual=False, no_pack=False):
    """-> (return code, y [B,Cout,2H,2W] on the device) of ctx_conv3x3_phase_f16 on the case's inputs."""
    L, lib = _lib()
    c = _case(B, H, W, Cin, Cout)
    xd = c['x'].permute(0, 2, 3, 1).contiguous().to(dev)
    wd = c['wp'].contiguous().to(dev)
    bd = c['bias'].to(dev)
    y = torch.zeros(B, 2 * H, 2 * W, Cout, dtype=torch.float16, device=dev)
    part = torch.empty(max(part_slices, 1) * y.numel(), dtype=torch.float32, device=dev) if part_slices else None
    rb = torch.zeros(B, Cout, dtype=torch.float16, device=dev) if rowbias else None
    rs = torch.zeros_like(y) if residual else None
    rc = lib.ctx_conv3x3_phase_f16(L.ptr(xd), None if no_pack else L.ptr(wd), L.ptr(bd) if with_bias else None, L.ptr(rb) if rowbias else None,
                                   L.ptr(rs) if residual else None, B, H, W, Cin, Cout, L.ptr(part) if part_slices else None, splitk,
                                   L.ptr(y), L.stream())
    torch.cuda.synchronize()
    return rc, y.permute(0, 3, 1, 2)


def _want(B, H, W, Cin, Cout, with_bias):
    c = _case(B, H, W, Cin, Cout)
    return c['want'] + c['bias'].float()[None, :, None, None] if with_bias else c['want']


@pytest.mark.parametrize("Cout,Cin", [(64, 64), (72, 128), (8, 64)])
def test_phase_pack(dev, Cout, Cin):
    L, lib = _lib()
    w = torch.randn(Cout, Cin, 3, 3, generator=torch.Generator().manual_seed(Cout + Cin))
    wd = w.to(dev)
    out = torch.zeros(4, Cout, 2, 2, Cin, dtype=torch.float16, device=dev)
    L.check(lib.ctx_pack_conv3_phase_f16(L.ptr(wd), Cout, Cin, L.ptr(out), L.stream()))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), phase_pack_ref(w))


SHAPES = [(1, 1, 1, 64, 64), (1, 2, 3, 64, 72), (2, 5, 7, 128, 160), (1, 9, 13, 128, 320), (2, 12, 12, 64, 320), (2, 24, 24, 320, 320)]


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("B,H,W,Cin,Cout", SHAPES)
def test_phase_conv(dev, B, H, W, Cin, Cout, with_bias):
    L, lib = _lib()
    rc, y = _run(dev, B, H, W, Cin, Cout, with_bias)
    L.check(rc)
    _close(y, _want(B, H, W, Cin, Cout, with_bias), f"phase conv {(B, H, W, Cin, Cout)} bias={with_bias}")


SPLIT = (2, 12, 12, 192, 160)


@pytest.mark.parametrize("splitk", [2, 3, 5, -1])
def test_phase_conv_splitk(dev, splitk):
    """K = 768 = 12 stages of 64, 3 per tap: 2 and 3 slices end on tap boundaries, 5 slices end inside taps; -1: the plan's own factor."""
    L, lib = _lib()
    rc, y = _run(dev, *SPLIT, True, splitk=splitk, part_slices=32 if splitk < 0 else splitk)
    L.check(rc)
    _close(y, _want(*SPLIT, True), f"phase conv split-K {splitk}")


# (tile, use8) of ctx_gemm_tune: the five forms of gemm144.hip (use8 4: 6 waves; 5, 6, 7: 15 waves; 8: 288 rows), every tile of gemm.hip,
# gemm8.hip and the two conv_halo.hip kernels
FORMS = [(-1, u) for u in (4, 5, 6, 7, 8)] + [(t, -1) for t in range(28)] + [(-1, 1), (-1, 2), (-1, 3)]


@pytest.mark.parametrize("tile,use8", FORMS)
@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 12, 12, 64, 320), (1, 9, 13, 128, 320)])
def test_phase_conv_every_form(dev, B, H, W, Cin, Cout, tile, use8):
    """Each forced form gives the right answer, or refuses with an error code and a message; none reads the pack as nine taps."""
    L, lib = _lib()
    lib.ctx_gemm_tune(tile, use8)
    try:
        rc, y = _run(dev, B, H, W, Cin, Cout, True)
        t, u = C.c_int32(-9), C.c_int32(-9)
        lib.ctx_gemm_last_kernel(C.byref(t), C.byref(u))
    finally:
        lib.ctx_gemm_tune(-1, -1)
    if rc != 0:
        msg = lib.ctx_last_error().decode()
        print(f"form (tile {tile}, use8 {use8}) refuses: {msg}")
        assert rc == E_ARG and "phase" in msg
        assert 1 <= use8 <= 3, "only gemm8.hip and conv_halo.hip are without the form"
        assert torch.count_nonzero(y).item() == 0, "a refused call wrote the output"
        return
    assert (t.value, u.value) == ((tile, 0) if tile >= 0 else (-1, use8)), f"ran tile {t.value} / use8 {u.value}"
    _close(y, _want(B, H, W, Cin, Cout, True), f"phase conv {(B, H, W, Cin, Cout)} tile {tile} use8 {use8}")


@pytest.mark.parametrize("what", ["rowbias", "residual", "no_pack"])
def test_phase_conv_refusals(dev, what):
    L, lib = _lib()
    rc, y = _run(dev, 2, 12, 12, 64, 320, True, **{what: True})
    assert rc == E_ARG and lib.ctx_last_error().decode()
    assert torch.count_nonzero(y).item() == 0, "a refused call launched"


def test_phase_conv_race_screen(dev):
    L, lib = _lib()
    for shape, kw in (((2, 24, 24, 320, 320), {}), (SPLIT, dict(splitk=5, part_slices=5))):
        outs = []
        for _ in range(3):
            rc, y = _run(dev, *shape, True, **kw)
            L.check(rc)
            outs.append(y.clone())
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), f"{shape}: launches differ"


def _rel(got, want):
    return ((got.float().cpu() - want).norm() / want.norm()).item()


def test_engine_unet_phase(dev):
    """The tiny UNet with the derived blob bound (phase form) and unbound (nine taps): both inside test_unet_vs_oracle's gates, the same
    launch counts and GroupNorm sources, and a clone_shared engine equal to its parent bit for bit."""
    from contexture_nerf_amd.unet import UNet2DConditionModel
    from oracle import unet_ref
    cfg = unet_ref.tiny_config()
    torch.manual_seed(1)
    ref = unet_ref.randomize_affine(unet_ref.UNet2DConditionModelRef(cfg)).eval()
    net = UNet2DConditionModel(cfg, device=dev, init=False)
    assert net._derived is not None and net._derived.numel() == net._lib.ctx_unet_derived_bytes(net._h) > 0
    net.load_state_dict(ref.state_dict())
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 5, 16, 16, generator=g)
    ctx = torch.randn(2, 7, cfg['cross_attention_dim'], generator=g)
    t = 981.0
    with torch.no_grad():
        want32 = ref(x, torch.tensor(t), ctx)['sample']
    want16 = unet_ref.forward_fp16_storage(ref, x, torch.tensor(t), ctx)['sample']
    floor = _rel(want16, want32)
    seen = {}
    for bound in (True, False):
        net.use_derived(bound)
        got = net(x.to(dev), t, ctx.to(dev))['sample'].clone()
        a, b = C.c_int64(-1), C.c_int64(-1)
        assert net._lib.ctx_unet_gn_epilogue_counts(net._h, C.byref(a), C.byref(b)) == 0
        fl = net.flops(2, 16, 16, 7)
        r16, r32 = _rel(got, want16), _rel(got, want32)
        print(f"tiny UNet, derived blob bound={bound}: rel L2 vs fp16-storage restatement {r16:.3e} | vs fp32 {r32:.3e} (floor {floor:.3e})")
        assert torch.isfinite(got).all()
        assert r16 < 1.6e-3 and r32 < 1.25 * floor + 2e-4
        seen[bound] = (got, a.value, b.value, fl)
    assert seen[True][1:3] == seen[False][1:3], "GroupNorm sources changed with the derived blob"
    assert seen[True][3] == seen[False][3], "launch / FLOP counts changed with the derived blob"
    assert not torch.equal(seen[True][0], seen[False][0]), "the phase form did not run (outputs are bit-identical)"
    net.use_derived(True)
    twin = net.clone_shared()
    assert twin._derived is net._derived
    assert torch.equal(twin(x.to(dev), t, ctx.to(dev))['sample'], seen[True][0])


def test_engine_vae_phase(dev):
    """The tiny VAE decoder, as test_engine_unet_phase (gate of test_vae_decode_vs_oracle: 3e-3)."""
    from contexture_nerf_amd.vae import AutoencoderKL
    from oracle import vae_ref, unet_ref
    cfg = dict(latent_channels=4, out_channels=3, block_out_channels=(64, 128), layers_per_block=1, groups=32)
    torch.manual_seed(3)
    ref = unet_ref.randomize_affine(vae_ref.AutoencoderKLDecodeRef(cfg)).eval()
    vae = AutoencoderKL(cfg, device=dev, init=False)
    assert vae._derived is not None and vae._derived.numel() == vae._lib.ctx_vae_derived_bytes(vae._h) > 0
    vae.load_state_dict(ref.state_dict())
    z = torch.randn(1, 4, 16, 8)
    with torch.no_grad():
        want = ref.decode(z)
    seen = {}
    for bound in (True, False):
        vae.use_derived(bound)
        got = vae.decode(z.to(dev)).sample.clone()
        r = _rel(got, want)
        print(f"tiny VAE decoder, derived blob bound={bound}: rel L2 vs fp32 = {r:.3e}")
        assert torch.isfinite(got).all() and r < 3e-3
        seen[bound] = (got, vae._lib.ctx_vae_flops(vae._h))
    assert seen[True][1] == seen[False][1], "FLOP count changed with the derived blob"
    assert not torch.equal(seen[True][0], seen[False][0]), "the phase form did not run (outputs are bit-identical)"
    vae.use_derived(True)
    twin = vae.clone_shared()
    assert twin._derived is vae._derived
    assert torch.equal(twin.decode(z.to(dev)).sample, seen[True][0])
