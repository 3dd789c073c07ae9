#!/usr/bin/env python3
"""Times exposure compensation across painted views (guide.exposure_compensation; csrc/viewgain.hip) and appends ONE JSON line to
profiles/exposure_bench.jsonl.  Nothing here is gated.

1. ctx_view_pair_stats at V = 6, Tc = 256 and at V = 16, Tc = 512 (device events over `--iters` calls, after a warm-up), beside the time
   8 TB/s would take for the V * 4 * Tc^2 * 8 bytes it reads once.  The inputs are one random texture under per-view gains with a random
   70 % of the texels valid per view, so every pair of views overlaps: the most work the kernel can have per texel.
2. Seconds per mesh of ConTEXTure.paint() on spot with the switch off (the parent's paint_all) and on, alternated, `--repeats` times
   each after one warm-up of each: SD2-depth architecture at latent `--latent`, `--steps` PLMS steps, random-init weights.  The extra
   time is a few launches per view plus one host sync per mesh and does not depend on the denoising.
3. ConTEXTure.view_consistency() of the painted views (the switch on) without and with their gains.  With random-init weights the
   painted views are noise-like images: the figures show that the metric runs on gained views, not that real paints improve.
Usage: python tools/bench_exposure.py [--latent 64] [--steps 10] [--views 7] [--iters 200] [--repeats 3] [--skip-mesh]"""
import argparse
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from contexture_nerf_amd import kal

p = argparse.ArgumentParser()
p.add_argument("--latent", type=int, default=64)
p.add_argument("--steps", type=int, default=10)
p.add_argument("--views", type=int, default=7)
p.add_argument("--iters", type=int, default=200)
p.add_argument("--repeats", type=int, default=3)
p.add_argument("--grid", type=int, default=1200)
p.add_argument("--mesh-path", default="shapes/spot_triangulated.obj")
p.add_argument("--skip-mesh", action="store_true")
p.add_argument("--out", default=os.path.join(ROOT, "profiles", "exposure_bench.jsonl"))
a = p.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_exposure: needs the GPU (a CPU run cannot give a time)")
dev = torch.device('cuda:0')
HBM = 8000.0   # GB/s spec
rec = {"bench": "exposure", "kernel": [], "data": "synthetic (random-init engines)"}


def timeit(fn, iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


for V, Tc in ((6, 256), (16, 512)):
    g = torch.Generator().manual_seed(V)
    tex = torch.rand(1, 3, Tc, Tc, generator=g) * 0.4 + 0.2
    gains = torch.rand(V, 3, 1, 1, generator=g) * 0.6 + 0.7
    w = (torch.rand(V, 1, Tc, Tc, generator=g) < 0.7).to(torch.float64) * 2.0 ** 32
    A = torch.cat([(tex * gains).to(torch.float64) * w, w], dim=1).round().to(torch.int64).to(dev).contiguous()
    sec = timeit(lambda: kal.view_pair_stats(A), a.iters)
    count, _ = kal.view_pair_stats(A)
    nbytes = V * 4 * Tc * Tc * 8
    rec["kernel"].append({"V": V, "Tc": Tc, "us": round(sec * 1e6, 2), "bytes": nbytes, "hbm_floor_us": round(nbytes / (HBM * 1e9) * 1e6, 2),
                          "includes": "two torch.empty and two memsets per call", "pairs_with_overlap": int((count > 0).sum())})
    print(json.dumps(rec["kernel"][-1]), flush=True)

if not a.skip_mesh:
    from contexture_nerf_amd import config as CFG
    from contexture_nerf_amd.trainer import ConTEXTure
    from contexture_nerf_amd.stable_diffusion_depth import StableDiffusion
    cfg = CFG.TrainConfig()
    cfg.guide.text = "a photo of a cow"
    cfg.guide.shape_path = a.mesh_path
    cfg.guide.guidance_scale = 10.0
    cfg.guide.sd_image_size = a.latent * 8
    cfg.guide.num_inference_steps = a.steps
    cfg.render.train_grid_size = a.grid
    cfg.optim.views_in_flight, cfg.optim.views_per_eval = 3, 6
    sd = StableDiffusion(dev)
    tr = ConTEXTure(cfg, device=dev, diffusion=sd)
    tr.train_views = tr.train_views[:a.views]
    tr.text_z = sd.get_text_embeds([cfg.guide.text])
    times = {False: [], True: []}
    for k in range(2 * (a.repeats + 1)):                     # alternated; the first of each is its warm-up
        on = bool(k % 2)
        cfg.guide.exposure_compensation = on
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.paint()
        torch.cuda.synchronize()
        if k >= 2:
            times[on].append(time.perf_counter() - t0)
    off, on = float(np.median(times[False])), float(np.median(times[True]))
    rec["paint"] = {"mesh": os.path.basename(a.mesh_path), "views": len(tr.train_views), "latent": a.latent, "steps": a.steps, "render": a.grid,
                    "atlas": cfg.guide.texture_resolution, "exposure_resolution": cfg.guide.exposure_resolution,
                    "sec_per_mesh_off": round(off, 4), "sec_per_mesh_on": round(on, 4), "extra_ms": round((on - off) * 1e3, 2),
                    "all_off": [round(t, 4) for t in times[False]], "all_on": [round(t, 4) for t in times[True]]}
    print(json.dumps(rec["paint"]), flush=True)
    # the painted views of one more compensated paint (one rank: they finish in view order), without and with their gains
    views, finish = [], tr._paint_finish

    def finish_and_keep(ctx, rgb):
        out = finish(ctx, rgb)
        views.append(out[0])
        return out
    tr._paint_finish = finish_and_keep
    tr.paint()
    tr._paint_finish = finish
    gains = tr.view_gains.to(device=dev, dtype=torch.float32)
    views = torch.cat(views)
    gained = (views * gains[:, :, None, None]).clamp(0, 1)
    rec["view_consistency"] = {"without_gains": tr.view_consistency(images=views)['mean'], "with_gains": tr.view_consistency(images=gained)['mean'],
                               "gains": [[round(x, 4) for x in row] for row in tr.view_gains.tolist()],
                               "note": "random-init weights: noise-like views, no claim about real paints"}
    print(json.dumps(rec["view_consistency"]), flush=True)

os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "a") as fh:
    fh.write(json.dumps(rec) + "\n")
