#!/usr/bin/env python3
"""What a grid voxelised from the mesh (OccupancyGrid.from_mesh) and per-ray spans (render_rays(clip=True)) buy on the ray path, beside
the hand-made ball of tools/bench_occupancy.py.  Mesh: `spot` of shapes/meshes.npz, normalised as the trainer normalises it (centred,
largest vertex norm 0.6, lifted by 0.25); camera, box and sizes of bench_occupancy.py (pinhole at distance 1.5, fovy 60 deg, near / far
0.5 / 2.5, box [-1, 1]^3, field NeRF2D(63 -> 4, D 8, W 256)).

  1. the occupied share of cells, and of the render's samples, for the ball mask and for the mesh grid at G = 64, 128, 256 with dilate 0, 1, 2,
     without and with clip;
  2. render_image at HW^2 x S (default 512^2 x 128) and one train_step at 4096 x S for: dense, ball, mesh (G 128, dilate 1), mesh + clip,
     alternating in one process;
  3. ctx_occ_voxelize, ctx_occ_dilate and ctx_occ_ray_spans on their own, beside the bytes they must move and the time 8 TB/s would take;
  4. the voxeliser on a 12-triangle cube at G = 256: two triangles per face, each with up to G^2 cells to mark from one wave.

Device events, median after warm-up; the yardstick is the dense path of the same process.  Expectation to hold the figures against:
time = share of samples x dense + the select kernels + one sync per pass.  Appends one JSON line to profiles/occupancy_mesh_bench.jsonl.
Usage: python tools/bench_occupancy_mesh.py [HW = 512] [S = 128] [render repetitions = 5] [step repetitions = 11]"""
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
assert torch.cuda.is_available(), "bench_occupancy_mesh needs the GPU"
dev = torch.device('cuda:0')
lib = L.load()
torch.manual_seed(0)
G0, RADIUS, NEAR, FAR, RT = 128, 0.6, 0.5, 2.5, 4096

m = np.load(os.path.join(ROOT, "shapes", "meshes.npz"))
verts = torch.tensor(m["spot_triangulated_v"], dtype=torch.float32, device=dev)
faces = torch.tensor(m["spot_triangulated_f"].astype(np.int64), device=dev)
verts = verts - verts.mean(dim=0)                                     # Mesh.normalize_mesh(target_scale=0.6, dy=0.25)
verts = verts / torch.max(torch.norm(verts, p=2, dim=1)) * 0.6
verts[:, 1] += 0.25
verts = verts.contiguous()

c = (torch.arange(G0, device=dev, dtype=torch.float32) + 0.5) / G0 * 2 - 1
ball = vr.OccupancyGrid.from_mask((c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2) < RADIUS ** 2, -1.0, 1.0)
mesh_grid = vr.OccupancyGrid.from_mesh(verts, faces, G0, -1.0, 1.0, dilate=1)
field = rnh.NeRF2D(D=8, W=256, input_ch=63, output_ch=4, skips=[4]).to(dev)
with torch.no_grad():
    field.output_linear.bias[3] = 1.0
K = vr.pinhole(HW, HW)
c2w = torch.tensor([[1., 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1.5]], device=dev)
ro, rd = rnh.get_rays(HW, HW, K, c2w)
ro, rd = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()
R = ro.shape[0]
t = torch.linspace(0., 1., S, device=dev)


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


def sample_share(grid, o, d, clip):
    """The share of the samples of rays (o, d) the grid selects, with the dense or the clipped placement."""
    if clip:
        span, _ = grid.ray_spans(o, d, NEAR, FAR)
        z = (span[:, :1] * (1. - t) + span[:, 1:] * t).contiguous()
    else:
        z = (NEAR * (1. - t) + FAR * t).expand(o.shape[0], S).contiguous()
    return round(grid.select(o, d, z).numel() / (o.shape[0] * S), 4)


res = {"metric": "ray path with an occupancy grid voxelised from the mesh (from_mesh) and per-ray spans (clip=True); dense path and the ball "
                 "grid of the same process as yardsticks",
       "case": {"mesh": "spot_triangulated", "faces": int(faces.shape[0]), "scale": 0.6, "dy": 0.25, "box": [-1, 1], "camera_distance": 1.5,
                "fovy_deg": 60, "near_far": [NEAR, FAR], "samples": S, "ball_radius": RADIUS, "field": {"D": 8, "W": 256}}}

# ---- 1. shares ------------------------------------------------------------------------------------------------------------------------------
shares = {"ball_G128": {"cells": round(ball.fraction(), 4), "samples": sample_share(ball, ro, rd, False)}}
for G in (64, 128, 256):
    for dil in (0, 1, 2):
        g = vr.OccupancyGrid.from_mesh(verts, faces, G, -1.0, 1.0, dilate=dil)
        shares[f"mesh_G{G}_dilate{dil}"] = {"cells": round(g.fraction(), 4), "samples": sample_share(g, ro, rd, False),
                                            "samples_clip": sample_share(g, ro, rd, True)}
        del g
res["shares"] = shares

# ---- 2. render_image and train_step ------------------------------------------------------------------------------------------------------------
names = ("dense", "ball", "mesh", "mesh_clip")
kws = (dict(), dict(occupancy=ball), dict(occupancy=mesh_grid), dict(occupancy=mesh_grid, clip=True))
us = alternate([(lambda kw=kw: vr.render_image(field, HW, HW, K, c2w, NEAR, FAR, S, **kw)) for kw in kws], reps_render, warm=1)
res["render"] = {"rays": R, "repetitions": reps_render, **{f"{n}_us": u for n, u in zip(names, us)},
                 **{f"{n}_ratio": round(u / us[0], 4) for n, u in zip(names[1:], us[1:])}}

pick = torch.randint(0, R, (RT,), device=dev)
ro_t, rd_t = ro[pick].contiguous(), rd[pick].contiguous()
target = torch.rand(RT, 3, device=dev)
opt = torch.optim.Adam(field.parameters(), lr=5e-4)
us = alternate([(lambda kw=kw: vr.train_step(field, opt, ro_t, rd_t, target, NEAR, FAR, S, **kw)) for kw in kws], reps_step, warm=3)
res["train_step"] = {"rays": RT, "repetitions": reps_step, **{f"{n}_us": u for n, u in zip(names, us)},
                     **{f"{n}_ratio": round(u / us[0], 4) for n, u in zip(names[1:], us[1:])},
                     "sample_share": {"ball": sample_share(ball, ro_t, rd_t, False), "mesh": sample_share(mesh_grid, ro_t, rd_t, False),
                                      "mesh_clip": sample_share(mesh_grid, ro_t, rd_t, True)}}

# ---- 3. the three kernels alone ----------------------------------------------------------------------------------------------------------------
V, F = verts.shape[0], faces.shape[0]
n = G0 ** 3
cells, grown, ws = torch.zeros(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
span, hit = torch.empty(R, 2, device=dev), torch.empty(R, dtype=torch.uint8, device=dev)
gc = lambda g: (*map(float, g.lo), *map(float, g.inv))
vox = lambda: L.check(lib.ctx_occ_voxelize(L.ptr(verts), L.ptr(faces), V, F, G0, *gc(mesh_grid), L.ptr(cells), L.stream()))
vox()
marked = int(cells.count_nonzero())
kern = {
    "voxelize_spot_G128": (vox, F * 24 + V * 12 + marked),
    "dilate_G128_k1": (lambda: L.check(lib.ctx_occ_dilate(L.ptr(cells), G0, 1, L.ptr(grown), L.ptr(ws), L.stream())), 3 * 2 * n),
    "ray_spans_G128": (lambda: L.check(lib.ctx_occ_ray_spans(L.ptr(ro), L.ptr(rd), R, NEAR, FAR, L.ptr(mesh_grid.cells), G0, *map(float, mesh_grid.lo),
                                                             *map(float, mesh_grid.hi), *map(float, mesh_grid.inv), *map(float, mesh_grid.h),
                                                             L.ptr(span), L.ptr(hit), L.stream())), R * (24 + 8 + 1)),
}
# ---- 4. the worst balance: a cube of 12 triangles at G = 256 -------------------------------------------------------------------------------------
cube_v = torch.tensor([[x, y, z] for x in (-0.9, 0.9) for y in (-0.9, 0.9) for z in (-0.9, 0.9)], dtype=torch.float32, device=dev)
cube_f = torch.tensor([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]],
                      dtype=torch.int64, device=dev)
big = vr.OccupancyGrid(256, -1.0, 1.0, dev)
big.cells.zero_()
kern["voxelize_cube12_G256"] = (lambda: L.check(lib.ctx_occ_voxelize(L.ptr(cube_v), L.ptr(cube_f), 8, 12, 256, *gc(big), L.ptr(big.cells), L.stream())),
                                12 * 24 + 8 * 12)
us = alternate([k[0] for k in kern.values()], 21, warm=3)
res["kernels"] = {name: {"us": u, "bytes": b, "floor_us_at_8TBps": round(b / 8e6, 2)} for (name, (_, b)), u in zip(kern.items(), us)}
cube = res["kernels"]["voxelize_cube12_G256"]
cube["cells_marked"] = int(big.cells.count_nonzero())                 # one byte stored per marked cell
cube["bytes"] += cube["cells_marked"]
cube["floor_us_at_8TBps"] = round(cube["bytes"] / 8e6, 2)
res["kernels"]["voxelize_spot_G128"]["cells_marked"] = marked
res["device"] = torch.cuda.get_device_name(0)
res["timer"] = "device events, median"
line = json.dumps(res)
print(line)
with open(os.path.join(ROOT, "profiles", "occupancy_mesh_bench.jsonl"), "a") as f:
    f.write(line + "\n")
