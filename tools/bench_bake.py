#!/usr/bin/env python3
"""What baking a 3-D field into the UV atlas costs: spot with its own UVs, a T x T atlas, supersample 1 and 2, a
HashGridField at its defaults over a from_mesh(G = 128, dilate = 1) grid.  One process, device events, median after warm-up.

  1. ctx_texel_rays and ctx_bake_resolve on the chart list, each beside the HBM bytes it must move and the time 8 TB/s would take (the
     field is untrained, so the resolve runs with min_alpha = 0 and writes every entry);
  2. the whole bake_atlas, and its stages in turn: texel_rays, the march, the field on the marched points, the compositing, the resolve
     (host wall clock around a synchronize for the march, which reads its sample count back).

Appends one JSON line to profiles/bake_bench.jsonl.  Usage: python tools/bench_bake.py [atlas = 1024] [repetitions = 21]"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from contexture_nerf_amd import config as CFG, kal, run_nerf_helpers as rnh, volume_render as vr
from contexture_nerf_amd.hashgrid import HashGridField
from contexture_nerf_amd.trainer import ConTEXTure

T = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 21
G = 128
assert torch.cuda.is_available(), "bench_bake needs the GPU"
dev = torch.device("cuda:0")

cfg = CFG.TrainConfig()
cfg.guide.text = "a photo of a cow"
cfg.guide.shape_path = "shapes/spot_triangulated.obj"
cfg.guide.texture_resolution = T
tr = ConTEXTure(cfg, device=dev, diffusion=None)
mm = tr.mesh_model
verts, faces = mm.mesh.vertices.detach().contiguous(), mm.mesh.faces.contiguous()
face_uv = mm.face_attributes[0].detach().float().contiguous()
tface, tbary = mm.texel_map()
lo, hi = verts.min(0).values.cpu().numpy(), verts.max(0).values.cpu().numpy()
pad = 0.1 * float((hi - lo).max())
grid = vr.OccupancyGrid.from_mesh(verts, faces, G, lo - pad, hi + pad, dilate=1)
torch.manual_seed(0)
field = HashGridField.from_grid(grid).to(dev)
chart = kal.chart_texels(tface)
n = int(chart.numel())
shell = 1.5 * float(np.max(grid.h))
step = shell / 8.0


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); out = fn(); b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3, out


def median_us(fn, warm=3):
    ts = [timed(fn)[0] for _ in range(warm + reps)][warm:]
    return round(statistics.median(ts), 1)


def wall_us(fn, warm=3):
    ts = []
    for r in range(warm + reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return round(statistics.median(ts[warm:]), 1)


def with_floor(us, nbytes):
    return {"us": us, "hbm_bytes": int(nbytes), "floor_us_at_8TBps": round(nbytes / 8e6, 2)}


res = {"metric": "bake: texels to rays, the marched field, sub-samples to atlas sums",
       "case": {"mesh": "spot_triangulated", "atlas": T, "chart_texels": n, "G": G, "shell": round(shell, 6), "step": round(step, 6),
                "field": "HashGridField defaults", "repetitions": reps}, "supersample": {}}
with torch.no_grad():
    for s in (1, 2):
        R = n * s * s
        ro, rd, valid = kal.texel_rays(tface, tbary, face_uv, verts, faces, chart, s, shell)
        ray_off, _, t, dt, pts = grid.march(ro, rd, 0., 2 * shell, step)
        raw = field.forward_pts(pts).contiguous()
        rgb, _, alpha, _, _ = rnh.raw2outputs_packed(raw, t, dt, rd, ray_off)
        acc = torch.zeros(4, T, T, dtype=torch.int64, device=dev)
        # the field is untrained (its alpha stays under any useful cut), so the resolve is timed with min_alpha = 0: every entry is written
        covered = int((kal.bake_resolve(rgb, alpha, valid, chart, s, acc.clone(), min_alpha=0.0)[3] > 0).sum())
        # texel_rays: the list, per entry one texel_face, three barycentrics, three ids, nine vertex and (s > 1) six uv floats in; 25 bytes per row out
        in_bytes = n * (4 + 8 + 12 + 24 + 36 + (24 if s > 1 else 0))
        entry = {
            "rows": R, "samples": int(t.numel()), "covered": covered,
            "texel_rays": with_floor(median_us(lambda: kal.texel_rays(tface, tbary, face_uv, verts, faces, chart, s, shell)), in_bytes + R * 25),
            # resolve: 17 bytes per row in, the list, four int64 sums read and written per written texel
            "bake_resolve": with_floor(median_us(lambda: kal.bake_resolve(rgb, alpha, valid, chart, s, acc, min_alpha=0.0)), R * 17 + n * 4 + n * 64),
            "march_wall_us": wall_us(lambda: grid.march(ro, rd, 0., 2 * shell, step)),
            "field_us": median_us(lambda: field.forward_pts(pts)),
            "composite_us": median_us(lambda: rnh.raw2outputs_packed(raw, t, dt, rd, ray_off)),
            "bake_atlas_wall_us": wall_us(lambda: vr.bake_atlas(field, verts, faces, face_uv, tface, tbary, grid, supersample=s)),
        }
        res["supersample"][str(s)] = entry
res["floors"] = ("texel_rays: the inputs of every entry once (the s*s rows of an entry share them) and 25 bytes per row out; "
                 "bake_resolve: 17 bytes per row in, the list, the four int64 sums of a written texel read and written")
res["device"] = torch.cuda.get_device_name(0)
res["timer"] = "device events, median; *_wall_us: host clock around a synchronize, median"
line = json.dumps(res)
print(line)
with open(os.path.join(ROOT, "profiles", "bake_bench.jsonl"), "a") as f:
    f.write(line + "\n")
