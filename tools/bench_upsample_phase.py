#!/usr/bin/env python3
"""The upsampling convolutions as nine taps over the x2 grid against their phase form (four 2x2 convolutions over the source grid,
4 / 9 of the multiplies), each on its own plan: the three UNet upsamplers at latent 96^2 (batch 2 and the lockstep batch 12) and on
the Zero123++ grid (latent 120 x 80), and the VAE decoder's three at 768^2.  Device-timed back-to-back launches
(ctx_bench_gemm), bias only, random operands.  Usage: bench_upsample_phase.py [ITERS]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from contexture_nerf_amd import _lib as L

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 50
lib = L.load(); dev = torch.device('cuda:0')
# (what, B, H, W, C)
SHAPES = [("unet 96 b2", 2, 12, 12, 1280), ("unet 96 b2", 2, 24, 24, 1280), ("unet 96 b2", 2, 48, 48, 640),
          ("unet 96 b12", 12, 12, 12, 1280), ("unet 96 b12", 12, 24, 24, 1280), ("unet 96 b12", 12, 48, 48, 640),
          ("zero123++", 2, 15, 10, 1280), ("zero123++", 2, 30, 20, 1280), ("zero123++", 2, 60, 40, 640),
          ("vae 768", 1, 96, 96, 512), ("vae 768", 1, 192, 192, 512), ("vae 768", 1, 384, 384, 256)]
part = torch.empty(384 << 20, dtype=torch.uint8, device=dev)
print(f"{'layer':>12} {'B':>3} {'H':>4} {'W':>4} {'C':>5} {'M out':>8} {'nine-tap us':>12} {'phase us':>9} {'ratio':>6} {'phase TF/s (4/9 FLOP)':>22}")
tot9 = totp = 0.0
for what, B, H, W, Cc in SHAPES:
    g = torch.Generator(device=dev).manual_seed(H + Cc)
    M = 4 * B * H * W
    x = torch.randn(B, H, W, Cc, generator=g, device=dev).half()
    w9 = (torch.randn(Cc, 9 * Cc, generator=g, device=dev) / (9 * Cc) ** 0.5).half()
    wp = (torch.randn(4 * Cc, 4 * Cc, generator=g, device=dev) / (4 * Cc) ** 0.5).half()
    bias = torch.randn(Cc, generator=g, device=dev).half()
    y = torch.empty(M, Cc, dtype=torch.float16, device=dev)

    def run(wt, flags, K):
        ts = [lib.ctx_bench_gemm(L.ptr(x), L.ptr(wt), L.ptr(bias), None, M, Cc, K, L.ptr(y), B, H, W, Cc, flags, 0, L.ptr(part), -1, iters, L.stream())
              for _ in range(3)]
        if min(ts) <= 0:
            raise L.CtxError(lib.ctx_last_error().decode())
        return min(ts) * 1e3
    t9, tp = run(w9, 2, 9 * Cc), run(wp, 6, 4 * Cc)
    tot9 += t9; totp += tp
    print(f"{what:>12} {B:3d} {H:4d} {W:4d} {Cc:5d} {M:8d} {t9:12.1f} {tp:9.1f} {tp / t9:6.3f} {2.0 * M * Cc * 4 * Cc / tp / 1e6:22.1f}")
print(f"sum: nine-tap {tot9:.1f} us, phase {totp:.1f} us, ratio {totp / tot9:.3f}")
