#!/usr/bin/env python3
"""The ray / mesh intersector (volume_render.MeshTracer, csrc/meshhit.hip) on `spot` of shapes/meshes.npz, centred and scaled to a largest
vertex norm of 0.6, in the box [-1, 1]^3, under the Renderer pose elev 60 deg, azim 30 deg, radius 1.5 (volume_render.view_camera):

  1. build: MeshTracer(vertices, faces, G) for G = 32, 64, 128, host clock around the construction (it ends in its one host sync), and
     the list statistics (entries, mean and longest list over the cells that hold one);
  2. trace (nearest hit) and occluded (any hit) on HW^2 camera rays (default 512^2) at each G, in rays per second, beside
     ctx_occ_ray_spans on the same rays and the same grid: the same walk without triangles, hence a lower bound for the time;
  3. the share of pixels whose traced face equals the raster's face_idx for the same pose (kal.rasterize at HW^2): a reported number.
     Disagreements sit on silhouettes and on edges between faces, where the two tie rules differ.

Device events around each call, median after warm-up, the kernels of one G alternating so that all see the same clocks.  Appends one
JSON line to profiles/meshhit_bench.jsonl.  Usage: python tools/bench_meshhit.py [HW = 512] [repetitions = 21]"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from contexture_nerf_amd import _lib as L, kal, run_nerf_helpers as rnh, volume_render as vr

HW = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 21
assert torch.cuda.is_available(), "bench_meshhit needs the GPU"
dev = torch.device('cuda:0')
lib = L.load()
NEAR, FAR = 0.5, 2.5
ELEV, AZIM, RADIUS = np.pi / 3, np.pi / 6, 1.5

m = np.load(os.path.join(ROOT, "shapes", "meshes.npz"))
verts = torch.tensor(m["spot_triangulated_v"], dtype=torch.float32, device=dev)
faces = torch.tensor(m["spot_triangulated_f"].astype(np.int64), device=dev)
verts = verts - verts.mean(dim=0)
verts = (verts / torch.max(torch.norm(verts, p=2, dim=1)) * 0.6).contiguous()

K, c2w = vr.view_camera(ELEV, AZIM, RADIUS, 0.0, HW, HW)
ro, rd = rnh.get_rays(HW, HW, K, c2w.to(dev))
ro, rd = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()
R = ro.shape[0]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); out = fn(); b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3, out


def alternate(fns, reps, warm=3):
    """Median microseconds of each of `fns`, run in turn so that all see the same clocks."""
    ts = [[] for _ in fns]
    for r in range(warm + reps):
        for k, fn in enumerate(fns):
            us, _ = timed(fn)
            if r >= warm:
                ts[k].append(us)
    return [round(statistics.median(x), 1) for x in ts]


# the raster's view of the same pose
pos = torch.tensor([[RADIUS * np.sin(ELEV) * np.sin(AZIM), RADIUS * np.cos(ELEV), RADIUS * np.sin(ELEV) * np.cos(AZIM)]], dtype=torch.float32)
cam = kal.generate_transformation_matrix(pos, torch.zeros(1, 3), torch.tensor([[0.0, 1.0, 0.0]]))
f_cam, f_img, _ = kal.prepare_vertices(verts[None], faces, kal.generate_perspective_projection(np.pi / 3), camera_transform=cam.to(dev))
_, raster_face = kal.rasterize(HW, HW, f_cam[..., 2], f_img, f_cam[..., 2:3])
raster_face = raster_face.reshape(-1)

res = {"metric": "ray / mesh hits on the occupancy grid: build time, list statistics, trace / occluded rays per second beside ctx_occ_ray_spans "
                 "(the same walk without triangles), agreement of the traced face with the raster's face_idx",
       "case": {"mesh": "spot_triangulated", "faces": int(faces.shape[0]), "scale": 0.6, "box": [-1, 1], "pose": {"elev": ELEV, "azim": AZIM, "radius": RADIUS},
                "rays": R, "near_far": [NEAR, FAR], "repetitions": reps}, "grids": {}}
vr.MeshTracer(verts, faces, 32, -1.0, 1.0)                            # first launches load the code objects: not part of any build time
torch.cuda.synchronize()
for G in (32, 64, 128):
    builds = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tracer = vr.MeshTracer(verts, faces, G, -1.0, 1.0)
        torch.cuda.synchronize()
        builds.append((time.perf_counter() - t0) * 1e6)
    span, shit = torch.empty(R, 2, device=dev), torch.empty(R, dtype=torch.uint8, device=dev)
    spans = lambda: L.check(lib.ctx_occ_ray_spans(L.ptr(ro), L.ptr(rd), R, NEAR, FAR, L.ptr(tracer.cells), G, *map(float, tracer.lo), *map(float, tracer.hi),
                                                  *map(float, tracer.inv), *map(float, tracer.h), L.ptr(span), L.ptr(shit), L.stream()))
    us = alternate([lambda: tracer.trace(ro, rd, NEAR, FAR), lambda: tracer.occluded(ro, rd, NEAR, FAR), spans], reps)
    hit, _, face, _ = tracer.trace(ro, rd, NEAR, FAR)
    covered = (raster_face >= 0) | (hit != 0)
    res["grids"][f"G{G}"] = {"build_us_median_of_5": round(statistics.median(builds), 1), **tracer.stats(),
                             "trace_us": us[0], "occluded_us": us[1], "ray_spans_us": us[2],
                             "trace_Mrays_per_s": round(R / us[0], 1), "occluded_Mrays_per_s": round(R / us[1], 1),
                             "ray_spans_Mrays_per_s": round(R / us[2], 1), "trace_over_spans": round(us[0] / us[2], 2),
                             "hit_share": round(float(hit.float().mean()), 4),
                             "face_equals_raster_all_pixels": round(float((face == raster_face).float().mean()), 5),
                             "face_equals_raster_covered_pixels": round(float((face == raster_face)[covered].float().mean()), 5)}
res["device"] = torch.cuda.get_device_name(0)
res["timer"] = "device events, median; build: host clock around the constructor and a synchronise"
line = json.dumps(res)
print(line)
with open(os.path.join(ROOT, "profiles", "meshhit_bench.jsonl"), "a") as f:
    f.write(line + "\n")
