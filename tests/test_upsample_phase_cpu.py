"""The identity behind the upsampling convolution's phase form, in float64 on the CPU, and the derived blob's
size queries on engines that need no GPU."""
import pytest
import torch
import torch.nn.functional as F

RSETS = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}


@pytest.mark.parametrize("B,Cin,Cout,H,W", [(2, 64, 64, 6, 6), (1, 64, 72, 5, 7), (2, 128, 64, 1, 1), (1, 64, 64, 2, 3)])
def test_phase_identity_float64(B, Cin, Cout, H, W):
    """nearest x2 + pad-1 3x3 convolution == four 2x2 convolutions over the source with summed taps:
    wp[a,b][o][u][v][c] = sum_{ky in R(a,u)} sum_{kx in R(b,v)} w[o][c][ky][kx], y[n, 2i+a, 2j+b] = sum x[n, i+a-1+u, j+b-1+v] wp[a,b][u][v].
    In real arithmetic the two are equal; in float64 they differ by the order of ~Cin * 9 additions."""
    g = torch.Generator().manual_seed(B + Cin + Cout + H + W)
    x = torch.randn(B, Cin, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=torch.float64)
    bias = torch.randn(Cout, generator=g, dtype=torch.float64)
    want = F.conv2d(F.interpolate(x, scale_factor=2.0, mode='nearest'), w, bias, padding=1)
    xp = F.pad(x, (1, 1, 1, 1))
    got = torch.empty_like(want)
    for a in (0, 1):
        for b in (0, 1):
            k = torch.zeros(Cout, Cin, 2, 2, dtype=torch.float64)
            for u in (0, 1):
                for v in (0, 1):
                    for ky in RSETS[(a, u)]:
                        for kx in RSETS[(b, v)]:
                            k[:, :, u, v] += w[:, :, ky, kx]
            got[:, :, a::2, b::2] = F.conv2d(xp[:, :, a:a + H + 1, b:b + W + 1], k, bias)
    rel = ((got - want).norm() / want.norm()).item()
    print(f"phase identity {(B, Cin, Cout, H, W)}: relative difference {rel:.2e}")
    assert rel < 1e-14          # float64 round-off over <= 9 * 128 terms; a wrong tap set or shift is O(1)


def test_derived_bytes_and_pinned_weight_bytes():
    """The phase packs live in a blob of their own: 16 Cout Cin fp16 per upsampler (each rounded up to 128 elements) + 256 bytes;
    the weight blobs keep their pinned sizes (tests/test_abi_cpu.py)."""
    from contexture_nerf_amd.unet import UNet2DConditionModel, ControlNetModel, SD2_DEPTH
    from contexture_nerf_amd.vae import AutoencoderKL
    net = UNet2DConditionModel(SD2_DEPTH, device="cpu", init=False)
    cn = ControlNetModel(SD2_DEPTH, device="cpu", init=False)
    vae = AutoencoderKL(device="cpu", init=False)
    assert net._lib.ctx_unet_derived_bytes(net._h) == 2 * 16 * (1280 * 1280 + 1280 * 1280 + 640 * 640) + 256      # 117.96 MB
    assert cn._lib.ctx_unet_derived_bytes(cn._h) == 0                                                              # no upsamplers
    assert vae._lib.ctx_vae_derived_bytes(vae._h) == 2 * 16 * (512 * 512 + 512 * 512 + 256 * 256) + 256
    assert net._lib.ctx_unet_weight_bytes(net._h) == 1731858176
    assert cn._lib.ctx_unet_weight_bytes(cn._h) == 728486912
    assert vae._lib.ctx_vae_weight_bytes(vae._h) == 236137728
    # binding is refused where there is nothing to bind, and unbinding is always allowed
    assert cn._lib.ctx_unet_bind_derived(cn._h, None, 0) == 0
    assert net._lib.ctx_unet_bind_derived(net._h, None, 0) == 0
