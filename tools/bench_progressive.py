#!/usr/bin/env python3
"""Times the progressive paint loop (guide.paint_mode = 'progressive') and its kernels (csrc/maskops.hip).  One JSON object per line.

1. ctx_mask_morph (k = 19, dilate), ctx_sep_filter (k = 21) and ctx_atlas_blend (T = 1024) at the sizes of a 1200^2 render, device events
   over `--iters` calls, beside the time 8 TB/s would take for the bytes each call must move: the two separable operators read and
   write the image once per pass (4 x 4 x H x W bytes); the blend reads contrib, zsum, acc and meta and writes acc and meta in full at
   the worst (8 x (4 + 1 + 4 + 4) + 4 x 2 bytes per texel).
2. seconds per mesh of ConTEXTure.paint() on bench.py's mesh workload (bundled mesh, 1200^2 render, SD2-depth architecture at latent
   `--latent`, 50 PLMS steps, random-init weights), the same `--views` views in both modes: 'independent' as bench.py's mesh leg runs it
   (views_per_eval 6, the left-over view on its own) and 'progressive' (one view at a time, batch 2, plus one VAE encode per view).
Usage: python tools/bench_progressive.py [--latent 96] [--views 7] [--iters 200] [--skip-mesh]"""
import argparse
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from contexture_nerf_amd import kal

p = argparse.ArgumentParser()
p.add_argument("--latent", type=int, default=96)
p.add_argument("--views", type=int, default=7)
p.add_argument("--iters", type=int, default=200)
p.add_argument("--mesh-path", default="shapes/nascar.obj")
p.add_argument("--skip-mesh", action="store_true")
a = p.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_progressive: needs the GPU (a CPU run cannot give a time)")
dev = torch.device('cuda:0')
HBM = 8000.0   # GB/s spec


def timeit(fn, iters):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


G, T = 1200, 1024
g = torch.Generator().manual_seed(0)
mask = (torch.rand(1, 1, G, G, generator=g) < 0.4).float().to(dev)
taps = kal.gaussian_taps(21, 16.0)
contrib = torch.randint(0, 1 << 32, (4, T, T), generator=g).to(dev)
zsum = torch.randint(0, 1 << 32, (T, T), generator=g).to(dev)
acc = torch.randint(0, 1 << 32, (4, T, T), generator=g).to(dev)
meta = torch.rand(T, T, generator=g).to(dev)
cases = [
    ("ctx_mask_morph dilate k=19 @1200^2 (incl. two torch.empty)", lambda: kal.dilate(mask, 19), 4 * 4 * G * G),
    ("ctx_mask_morph erode k=5 @1200^2", lambda: kal.erode(mask, 5), 4 * 4 * G * G),
    ("ctx_mask_morph dilate k=63 @1200^2", lambda: kal.dilate(mask, 63), 4 * 4 * G * G),
    ("ctx_sep_filter k=21 @1200^2", lambda: kal.sep_filter(mask, taps), 4 * 4 * G * G),
    ("ctx_atlas_blend T=1024", lambda: kal.atlas_blend(contrib, zsum, acc, meta), (8 * 13 + 4 * 2) * T * T),
]
for name, fn, nbytes in cases:
    sec = timeit(fn, a.iters)
    print(json.dumps({"kernel": name, "us": round(sec * 1e6, 2), "bytes": nbytes, "hbm_floor_us": round(nbytes / (HBM * 1e9) * 1e6, 2)}), flush=True)

if not a.skip_mesh:
    from contexture_nerf_amd import config as CFG
    from contexture_nerf_amd.trainer import ConTEXTure
    from contexture_nerf_amd.stable_diffusion_depth import StableDiffusion
    cfg = CFG.TrainConfig()
    cfg.guide.text = "a photo of a car"
    cfg.guide.shape_path = a.mesh_path
    cfg.guide.guidance_scale = 10.0
    cfg.guide.sd_image_size = a.latent * 8
    cfg.guide.num_inference_steps = 50
    cfg.optim.views_in_flight, cfg.optim.views_per_eval = 3, 6
    sd = StableDiffusion(dev)
    tr = ConTEXTure(cfg, device=dev, diffusion=sd)
    tr.train_views = tr.train_views[:a.views]
    tr.text_z = sd.get_text_embeds([cfg.guide.text])
    for mode in ('independent', 'progressive', 'independent', 'progressive'):      # alternated: the first of each is its warm-up
        cfg.guide.paint_mode = mode
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        atlas, cov = tr.paint()
        torch.cuda.synchronize()
        print(json.dumps({"paint_mode": mode, "views": len(tr.train_views), "latent": a.latent, "sec_per_mesh": round(time.perf_counter() - t0, 3),
                          "atlas_coverage": round(float((cov > 0).float().mean()), 4)}), flush=True)
