#!/usr/bin/env python3
"""The signed point / mesh query (MeshTracer.signed_distance, csrc/meshdist.hip), its tables (csrc/meshpn.hip) and MeshSolidField on `spot`
of shapes/meshes.npz, centred and scaled to a largest vertex norm of 0.6, in the box [-1, 1]^3, under the Renderer pose elev 60 deg,
azim 30 deg, radius 1.5 (the set-up of tools/bench_meshdist.py):

  1. signed_distance beside closest at G = 32, 64, 128 with max_dist = h on the marched sample points (tracer.occupancy(1), march = h / 2)
     of HW^2 camera rays (default 512^2), the two alternating, and the time of the table build (vertex -> face lists and the tables, with
     its one host sync) on a fresh tracer;
  2. fit_views at G = 64 on four views of the mesh in a procedural colour on white (traced, 128^2), the same iterations for the plain
     HashGridField (with mesh=tracer, mask_weight = 1, depth_weight = 0.1), MeshDensityField (the tent) and MeshSolidField (the ramp):
     the mean squared error of each field's render of the first view against its target, and of its acc against the traced silhouette;
  3. render_normals of the solid field at HW^2.

Device events around each call, median after warm-up, alternatives alternating so that all see the same clocks.  Nothing here is a gate.
Appends one JSON line to profiles/meshsdf_bench.jsonl.  Usage: python tools/bench_meshsdf.py [HW = 512] [repetitions = 11] [iters = 200]"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from contexture_nerf_amd import run_nerf_helpers as rnh, volume_render as vr
from contexture_nerf_amd.hashgrid import HashGridField

HW = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 11
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 200
assert torch.cuda.is_available(), "bench_meshsdf needs the GPU"
dev = torch.device('cuda:0')
NEAR, FAR = 0.5, 2.5
ELEV, AZIM, RADIUS = np.pi / 3, np.pi / 6, 1.5

m = np.load(os.path.join(ROOT, "shapes", "meshes.npz"))
verts = torch.tensor(m["spot_triangulated_v"], dtype=torch.float32, device=dev)
faces = torch.tensor(m["spot_triangulated_f"].astype(np.int64), device=dev)
verts = verts - verts.mean(dim=0)
verts = (verts / torch.max(torch.norm(verts, p=2, dim=1)) * 0.6).contiguous()


def camera_rays(elev, azim, hw):
    K, c2w = vr.view_camera(elev, azim, RADIUS, 0.0, hw, hw)
    ro, rd = rnh.get_rays(hw, hw, K, c2w.to(dev))
    return K, c2w.to(dev), ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()


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


def build_tables(tracer):
    tracer._pn = None
    return tracer.pseudonormals()


K, c2w, ro, rd = camera_rays(ELEV, AZIM, HW)
res = {"metric": "signed point / mesh query on marched sample points beside the unsigned one; the table build; fit_views of the plain, tent and "
                 "solid fields; render_normals of the solid field",
       "case": {"mesh": "spot_triangulated", "faces": int(faces.shape[0]), "scale": 0.6, "box": [-1, 1], "pose": {"elev": ELEV, "azim": AZIM, "radius": RADIUS},
                "camera_rays": ro.shape[0], "near_far": [NEAR, FAR], "repetitions": reps, "fit_iters": iters}, "grids": {}}
for G in (32, 64, 128):
    tracer = vr.MeshTracer(verts, faces, G, -1.0, 1.0)
    grid = tracer.occupancy(1)
    h = float(np.max(tracer.h))
    pts = grid.march(ro, rd, NEAR, FAR, h / 2)[4]
    n = pts.shape[0]
    us_tab = alternate([lambda: build_tables(tracer)], reps)[0]
    us = alternate([lambda: tracer.signed_distance(pts, h), lambda: tracer.closest(pts, h)], reps)
    found, sdist = tracer.signed_distance(pts, h)[:2]
    same = all(torch.equal(a, b) for a, b in zip((found, sdist.abs()), tracer.closest(pts, h)[:2]))
    res["grids"][f"G{G}"] = {**tracer.stats(), "topology": tracer.topology(), "points": n, "signed_us": us[0], "closest_us": us[1],
                             "ratio": round(us[0] / us[1], 3), "signed_Mpts_per_s": round(n / us[0], 1), "closest_Mpts_per_s": round(n / us[1], 1),
                             "table_build_us": us_tab, "found_share": round(float(found.float().mean()), 4),
                             "inside_share": round(float((sdist < 0).float().mean()), 4), "found_and_abs_equal_closest": bool(same)}

# ---- fit_views at G = 64: the plain field, the tent and the solid ----------------------------------------------------------------------------
G = 64
tracer = vr.MeshTracer(verts, faces, G, -1.0, 1.0)
grid = tracer.occupancy(1)
h = float(np.max(tracer.h))


def colour_of(p):
    return 0.5 + 0.5 * torch.sin(6.0 * p + torch.tensor([0.0, 2.0, 4.0], device=dev))


views, c2ws, sil = [], [], []
HV = 128
for elev, azim in ((np.pi / 3, np.pi / 6), (np.pi / 2, np.pi / 6 + np.pi / 2), (np.pi / 2.5, np.pi / 6 + np.pi), (2 * np.pi / 3, np.pi / 6 + 1.5 * np.pi)):
    Kv, c, o, d = camera_rays(elev, azim, HV)
    hit, t, _, _ = tracer.trace(o, d, NEAR, FAR)
    hitf = hit.float()[:, None]
    views.append((hitf * colour_of(o + d * t[:, None]) + (1 - hitf)).reshape(HV, HV, 3))
    c2ws.append(c); sil.append(hit.float())
views, c2ws = torch.stack(views), torch.stack(c2ws)


def new_field(kind):
    torch.manual_seed(1)
    inner = HashGridField.from_grid(grid, n_levels=8, n_features=2, log2_table=15, base_res=8, max_res=256).to(dev)
    if kind == "tent":
        return vr.MeshDensityField(inner, tracer)
    if kind == "solid":
        return vr.MeshSolidField(inner, tracer)
    with torch.no_grad():
        inner.mlp.output_linear.bias[3] = 1.0                          # a field that begins at zero density has no gradient
    return inner


fit = {}
for kind in ("plain", "tent", "solid"):
    field = new_field(kind)
    extra = dict(mesh=tracer, mask_weight=1.0, depth_weight=0.1) if kind == "plain" else {}
    hist = vr.fit_views(field, views, c2ws, Kv, NEAR, FAR, iters, rays_per_iter=4096, lr=1e-2, seed=0, white_bkgd=True, occupancy=grid,
                        occupancy_every=0, march=h / 2, **extra)
    img = vr.render_image(field, HV, HV, Kv, c2ws[0], NEAR, FAR, 0, white_bkgd=True, occupancy=grid, march=h / 2)
    fit[kind] = {"loss_first_five": round(float(np.mean(hist[:5])), 6), "loss_last_five": round(float(np.mean(hist[-5:])), 6),
                 "view0_mse_after": float(((img['rgb'] - views[0]) ** 2).mean()),
                 "view0_acc_mse_after": float(((img['acc'].reshape(-1) - sil[0]) ** 2).mean())}
res["fit_views_G64"] = {"views": 4, "size": HV, "iters": iters, "rays_per_iter": 4096, "lr": 1e-2, **fit,
                        "note": "the plain field's loss history includes its mask and depth terms; view0_mse_after is the image alone for all three; "
                                "view0_acc_mse_after is against the traced silhouette"}
solid = new_field("solid")
us_n = alternate([lambda: vr.render_normals(solid, HW, HW, K, c2w, NEAR, FAR, grid, h / 2)], max(3, reps // 3), warm=1)[0]
nrm = vr.render_normals(solid, HW, HW, K, c2w, NEAR, FAR, grid, h / 2)
res["render_normals_G64"] = {"size": HW, "us": us_n, "covered_share": round(float((nrm['acc'] > 0.5).float().mean()), 4),
                             "mean_z_normal_on_covered": round(float(nrm['z_normal'][nrm['acc'] > 0.5].mean()), 4)}
res["device"] = torch.cuda.get_device_name(0)
res["timer"] = "device events, median, alternating"
line = json.dumps(res)
print(line)
with open(os.path.join(ROOT, "profiles", "meshsdf_bench.jsonl"), "a") as f:
    f.write(line + "\n")
