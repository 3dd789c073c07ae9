#!/usr/bin/env python3
"""What marching the occupancy grid into ragged per-ray sample lists (march=step) costs and buys on the ray path, beside
the paths it is meant to replace: the mesh grid with 128 samples over near .. far, and mesh + clip.  Mesh, grid (G 128, dilate 1), camera,
box and field are those of tools/bench_occupancy_mesh.py.

  1. render_image at HW^2 rays and one train_step at 4096 rays for dense, mesh, mesh + clip and march in {h, h/2, h/4}, alternating in one
     process: n, samples per hit ray, the time, and the time the rule of section 4e predicts: n / (R * S) x dense + the march kernels + one sync;
  2. the train_step by stage (march, field forward, compositing, backward, optimizer) for each step, to see what does not scale with n;
  3. ctx_occ_march_count, ctx_occ_march_write, ctx_raymarch_packed_fwd and _bwd on their own, beside the bytes they must move and the time
     8 TB/s would take;
  4. the bytes a pass keeps alive between forward and backward (torch.cuda.memory_allocated around the forward).

Device events, median after warm-up.  Appends one JSON line to profiles/march_bench.jsonl.
Usage: python tools/bench_march.py [HW = 512] [S = 128] [render repetitions = 5] [step repetitions = 11]"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from contexture_nerf_amd import _lib as L, run_nerf_helpers as rnh, volume_render as vr

HW = int(sys.argv[1]) if len(sys.argv) > 1 else 512
S = int(sys.argv[2]) if len(sys.argv) > 2 else 128
reps_render = int(sys.argv[3]) if len(sys.argv) > 3 else 5
reps_step = int(sys.argv[4]) if len(sys.argv) > 4 else 11
assert torch.cuda.is_available(), "bench_march needs the GPU"
dev = torch.device('cuda:0')
lib = L.load()
torch.manual_seed(0)
G0, NEAR, FAR, RT = 128, 0.5, 2.5, 4096

m = np.load(os.path.join(ROOT, "shapes", "meshes.npz"))
verts = torch.tensor(m["spot_triangulated_v"], dtype=torch.float32, device=dev)
faces = torch.tensor(m["spot_triangulated_f"].astype(np.int64), device=dev)
verts = verts - verts.mean(dim=0)                                     # Mesh.normalize_mesh(target_scale=0.6, dy=0.25)
verts = verts / torch.max(torch.norm(verts, p=2, dim=1)) * 0.6
verts[:, 1] += 0.25
verts = verts.contiguous()
grid = vr.OccupancyGrid.from_mesh(verts, faces, G0, -1.0, 1.0, dilate=1)
H_CELL = float(grid.h[0])
STEPS = {"h": H_CELL, "h/2": H_CELL / 2, "h/4": H_CELL / 4}
field = rnh.NeRF2D(D=8, W=256, input_ch=63, output_ch=4, skips=[4]).to(dev)
with torch.no_grad():
    field.output_linear.bias[3] = 1.0
K = vr.pinhole(HW, HW)
c2w = torch.tensor([[1., 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1.5]], device=dev)
ro, rd = rnh.get_rays(HW, HW, K, c2w)
ro, rd = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()
R = ro.shape[0]
t_lin = torch.linspace(0., 1., S, device=dev)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); out = fn(); b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3, out


def alternate(fns, reps, warm=2):
    """Median microseconds of each of `fns`, run in turn so that all see the same clocks."""
    ts = [[] for _ in fns]
    for r in range(warm + reps):
        for k, fn in enumerate(fns):
            us, _ = timed(fn)
            if r >= warm:
                ts[k].append(us)
    return [round(statistics.median(x), 1) for x in ts]


def dense_selected(o, d, clip):
    """How many of the R x S samples of the mesh-grid path lie in occupied cells, with the dense or the clipped placement."""
    if clip:
        span, _ = grid.ray_spans(o, d, NEAR, FAR)
        z = (span[:, :1] * (1. - t_lin) + span[:, 1:] * t_lin).contiguous()
    else:
        z = (NEAR * (1. - t_lin) + FAR * t_lin).expand(o.shape[0], S).contiguous()
    return int(grid.select(o, d, z).numel())


def march_stats(o, d, step):
    ray_off = grid.march(o, d, NEAR, FAR, step)[0]
    cnt = ray_off[1:] - ray_off[:-1]
    hit = int((cnt > 0).sum())
    n = int(ray_off[-1])
    return {"n": n, "hit_rays": hit, "samples_per_hit_ray": round(n / max(hit, 1), 2), "max_per_ray": int(cnt.max())}


def march_only(o, d, step):
    return lambda: grid.march(o, d, NEAR, FAR, step)


res = {"metric": "ray path on ragged per-ray sample lists marched through the mesh grid (march=step) beside the mesh-grid path at S samples, "
                 "mesh + clip and the dense path of the same process",
       "case": {"mesh": "spot_triangulated", "scale": 0.6, "dy": 0.25, "G": G0, "dilate": 1, "cell": H_CELL, "box": [-1, 1],
                "camera_distance": 1.5, "fovy_deg": 60, "near_far": [NEAR, FAR], "samples": S, "field": {"D": 8, "W": 256},
                "occupied_cells": round(grid.fraction(), 4)}}

names = ("dense", "mesh", "mesh_clip") + tuple(f"march_{k}" for k in STEPS)
kws = (dict(), dict(occupancy=grid), dict(occupancy=grid, clip=True)) + tuple(dict(occupancy=grid, march=s) for s in STEPS.values())


def report(o, d, us, march_us):
    rays = o.shape[0]
    out = {"rays": rays, **{f"{n}_us": u for n, u in zip(names, us)}}
    out["mesh_selected"] = dense_selected(o, d, False)
    out["mesh_clip_selected"] = dense_selected(o, d, True)
    hit_clip = int(grid.ray_spans(o, d, NEAR, FAR)[1].sum())
    out["mesh_clip_selected_per_hit_ray"] = round(out["mesh_clip_selected"] / max(hit_clip, 1), 2)
    for (k, step), u, mu in zip(STEPS.items(), us[3:], march_us):
        st = march_stats(o, d, step)
        st["us"] = u
        st["march_us"] = mu                                           # count + scan + the sync + write
        st["predicted_us"] = round(st["n"] / (rays * S) * us[0] + mu, 1)
        st["vs_mesh"] = round(u / us[1], 4)
        st["vs_mesh_clip"] = round(u / us[2], 4)
        out[f"march_{k}"] = st
    return out


# ---- 1. render_image and train_step ---------------------------------------------------------------------------------------------------------
us = alternate([(lambda kw=kw: vr.render_image(field, HW, HW, K, c2w, NEAR, FAR, S, **kw)) for kw in kws], reps_render, warm=1)
march_us = alternate([march_only(ro, rd, s) for s in STEPS.values()], reps_render, warm=1)
res["render"] = {"repetitions": reps_render, **report(ro, rd, us, march_us)}

pick = torch.randint(0, R, (RT,), device=dev)
ro_t, rd_t = ro[pick].contiguous(), rd[pick].contiguous()
target = torch.rand(RT, 3, device=dev)
opt = torch.optim.Adam(field.parameters(), lr=5e-4)
us = alternate([(lambda kw=kw: vr.train_step(field, opt, ro_t, rd_t, target, NEAR, FAR, S, **kw)) for kw in kws], reps_step, warm=3)
march_us = alternate([march_only(ro_t, rd_t, s) for s in STEPS.values()], reps_step, warm=3)
res["train_step"] = {"repetitions": reps_step, **report(ro_t, rd_t, us, march_us)}

# ---- 2. the train_step by stage --------------------------------------------------------------------------------------------------------------
stages = {}
for k, step in STEPS.items():
    acc = {s: [] for s in ("march", "field_fwd", "composite_fwd", "loss", "backward", "optimizer")}
    for rep in range(3 + reps_step):
        opt.zero_grad(set_to_none=True)
        a, lists = timed(lambda: grid.march(ro_t, rd_t, NEAR, FAR, step, perturb=True))
        ray_off, ray_id, tt, dt, pts = lists
        b, raw = timed(lambda: field.forward_pts(pts))
        c, out = timed(lambda: rnh.raw2outputs_packed(raw, tt, dt, rd_t, ray_off))
        d_, loss = timed(lambda: rnh.img2mse(out[0], target))
        e, _ = timed(lambda: loss.backward())
        f, _ = timed(lambda: opt.step())
        if rep >= 3:
            for s, v in zip(acc, (a, b, c, d_, e, f)):
                acc[s].append(v)
    stages[f"march_{k}"] = {s: round(statistics.median(v), 1) for s, v in acc.items()}
    stages[f"march_{k}"]["n"] = int(tt.numel())
res["train_step_stages_us"] = stages

# ---- 3. the kernels alone ------------------------------------------------------------------------------------------------------------------------
ga = lambda step: (L.ptr(grid.cells), G0, *map(float, grid.lo), *map(float, grid.hi), *map(float, grid.inv), *map(float, grid.h), float(step))
kern = {}
keep = []
for k, step in STEPS.items():
    ray_off, ray_id, tt, dt, pts = grid.march(ro, rd, NEAR, FAR, step)
    n = int(tt.numel())
    count = torch.empty(R, dtype=torch.int32, device=dev)
    raw = torch.randn(n, 4, device=dev)
    outs = [torch.empty(R, 3, device=dev), torch.empty(R, device=dev), torch.empty(R, device=dev), torch.empty(n, device=dev), torch.empty(R, device=dev)]
    g_rgb, grad = torch.randn(R, 3, device=dev), torch.empty(n, 4, device=dev)
    keep.append((ray_off, ray_id, tt, dt, pts, count, raw, outs, g_rgb, grad))
    kern[f"march_count_{k}"] = (lambda step=step, count=count: L.check(lib.ctx_occ_march_count(L.ptr(ro), L.ptr(rd), R, NEAR, FAR, *ga(step),
                                                                                                  L.ptr(count), L.stream())), R * 28, n)
    kern[f"march_write_{k}"] = (lambda step=step, x=keep[-1], n=n: L.check(lib.ctx_occ_march_write(
        L.ptr(ro), L.ptr(rd), R, NEAR, FAR, *ga(step), L.ptr(x[0]), None, n, L.ptr(x[1]), L.ptr(x[2]), L.ptr(x[3]), L.ptr(x[4]), L.stream())),
        R * 40 + n * 24, n)
    kern[f"packed_fwd_{k}"] = (lambda x=keep[-1], n=n: L.check(lib.ctx_raymarch_packed_fwd(
        L.ptr(x[6]), L.ptr(x[2]), L.ptr(x[3]), L.ptr(rd), None, L.ptr(x[0]), R, n, 1, *[L.ptr(o) for o in x[7]], L.stream())),
        n * 28 + R * 52, n)
    kern[f"packed_bwd_{k}"] = (lambda x=keep[-1], n=n: L.check(lib.ctx_raymarch_packed_bwd(
        L.ptr(x[6]), L.ptr(x[2]), L.ptr(x[3]), L.ptr(rd), None, L.ptr(x[0]), R, n, 1, L.ptr(x[8]), None, None, None, None, L.ptr(x[9]),
        L.stream())), n * 40 + R * 40, n)
span, hit = torch.empty(R, 2, device=dev), torch.empty(R, dtype=torch.uint8, device=dev)
kern["ray_spans"] = (lambda: L.check(lib.ctx_occ_ray_spans(L.ptr(ro), L.ptr(rd), R, NEAR, FAR, *ga(1.0)[:-1], L.ptr(span), L.ptr(hit), L.stream())),
                     R * 33, 0)
us = alternate([k[0] for k in kern.values()], 21, warm=3)
res["kernels"] = {name: {"us": u, "bytes": b, "floor_us_at_8TBps": round(b / 8e6, 2), "n": n} for (name, (_, b, n)), u in zip(kern.items(), us)}
del keep, kern

# ---- 4. what a pass keeps alive between forward and backward ---------------------------------------------------------------------------------------
saved = {}
for name, kw in zip(names, kws):
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    out = rnh.render_rays(field, ro_t, rd_t, NEAR, FAR, S, perturb=1., white_bkgd=True, **kw)
    torch.cuda.synchronize()
    saved[name] = int(torch.cuda.memory_allocated() - before)
    del out
res["train_step"]["held_bytes_after_forward"] = saved

res["device"] = torch.cuda.get_device_name(0)
res["timer"] = "device events, median"
line = json.dumps(res)
print(line)
with open(os.path.join(ROOT, "profiles", "march_bench.jsonl"), "a") as f:
    f.write(line + "\n")
