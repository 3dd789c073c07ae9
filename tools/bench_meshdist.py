#!/usr/bin/env python3
"""The point / mesh query (MeshTracer.closest, csrc/meshdist.hip) and the mesh-anchored field on `spot` of shapes/meshes.npz, centred and
scaled to a largest vertex norm of 0.6, in the box [-1, 1]^3, under the Renderer pose elev 60 deg, azim 30 deg, radius 1.5:

  1. closest at G = 32, 64, 128 with max_dist = h on the marched sample points (tracer.occupancy(1), march = h / 2) of HW^2 camera rays
     (default 512^2) and of 4096 of them drawn at random, in points per second, beside tracer.trace on the same rays and beside a
     chunked brute-force evaluation in torch (every point against every triangle) on 16384 of the points: a sanity rate, and the largest
     difference of its distance from the kernel's where both find the mesh;
  2. train_step at G = 64 on 4096 rays, march = h / 2: MeshDensityField(HashGridField) beside the plain HashGridField with mesh=tracer,
     mask_weight = 1, depth_weight = 0.1, the two alternating;
  3. fit_views on four views of the mesh in a procedural colour on white (traced, 128^2), the same number of iterations for both: the mean
     squared error of each field's render of the first view against its target afterwards.

Device events around each call, median after warm-up, alternatives alternating so that all see the same clocks.  Nothing here is a gate.
Appends one JSON line to profiles/meshdist_bench.jsonl.  Usage: python tools/bench_meshdist.py [HW = 512] [repetitions = 11] [iters = 200]"""
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
assert torch.cuda.is_available(), "bench_meshdist needs the GPU"
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


def brute_force(pts, tri, r, chunk=2048):
    """Every point against every triangle in torch, float32: Ericson's regions as tests/meshdist_rule.py orders them -> (found, dist)."""
    v0, e1, e2 = tri[None, :, 0:3], tri[None, :, 4:7], tri[None, :, 8:11]
    found, dist = [], []
    for i in range(0, pts.shape[0], chunk):
        p = pts[i:i + chunk, None, :]
        ap = p - v0
        d1, d2 = (e1 * ap).sum(-1), (e2 * ap).sum(-1)
        bp = ap - e1
        d3, d4 = (e1 * bp).sum(-1), (e2 * bp).sum(-1)
        cp = ap - e2
        d5, d6 = (e1 * cp).sum(-1), (e2 * cp).sum(-1)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        den = 1.0 / (va + vb + vc)
        u, v = vb * den, vc * den
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        zero, one = torch.zeros_like(u), torch.ones_like(u)
        for cond, uu, vv in (((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), 1.0 - w, w), ((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, d2 / (d2 - d6)),
                             ((d6 >= 0) & (d5 <= d6), zero, one), ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1 / (d1 - d3), zero),
                             ((d3 >= 0) & (d4 <= d3), one, zero), ((d1 <= 0) & (d2 <= 0), zero, zero)):
            u, v = torch.where(cond, uu, u), torch.where(cond, vv, v)
        s = p - (v0 + e1 * u[..., None] + e2 * v[..., None])
        dd = torch.nan_to_num((s * s).sum(-1), nan=float('inf')).min(dim=1).values
        found.append(dd <= r * r); dist.append(dd.sqrt())
    return torch.cat(found), torch.cat(dist)


K, c2w, ro, rd = camera_rays(ELEV, AZIM, HW)
R = ro.shape[0]
gen = torch.Generator(device=dev).manual_seed(0)
batch = torch.randint(0, R, (4096,), device=dev, generator=gen)
ro_b, rd_b = ro[batch].contiguous(), rd[batch].contiguous()

res = {"metric": "point / mesh query on marched sample points: closest in points per second beside trace on the same rays and a brute-force torch "
                 "evaluation; train_step and fit_views of MeshDensityField(HashGridField) beside the plain field with the mask and depth terms",
       "case": {"mesh": "spot_triangulated", "faces": int(faces.shape[0]), "scale": 0.6, "box": [-1, 1], "pose": {"elev": ELEV, "azim": AZIM, "radius": RADIUS},
                "camera_rays": R, "training_rays": 4096, "near_far": [NEAR, FAR], "repetitions": reps, "fit_iters": iters}, "grids": {}}
for G in (32, 64, 128):
    tracer = vr.MeshTracer(verts, faces, G, -1.0, 1.0)
    grid = tracer.occupancy(1)
    h = float(np.max(tracer.h))
    row = {**tracer.stats()}
    for tag, o, d in (("camera", ro, rd), ("batch", ro_b, rd_b)):
        pts = grid.march(o, d, NEAR, FAR, h / 2)[4]
        n = pts.shape[0]
        us = alternate([lambda: tracer.closest(pts, h), lambda: tracer.trace(o, d, NEAR, FAR)], reps)
        found = tracer.closest(pts, h)[0]
        row[tag] = {"points": n, "closest_us": us[0], "closest_Mpts_per_s": round(n / us[0], 1), "trace_us": us[1],
                    "trace_Mrays_per_s": round(o.shape[0] / us[1], 1), "found_share": round(float(found.float().mean()), 4)}
        if tag == "camera":
            pick = torch.randperm(n, device=dev, generator=gen)[:16384]
            sub = pts[pick].contiguous()
            us_b = alternate([lambda: brute_force(sub, tracer.tri, h)], max(3, reps // 3), warm=1)[0]
            f_b, d_b = brute_force(sub, tracer.tri, h)
            f_k, d_k = tracer.closest(sub, h)[:2]
            both = f_b & (f_k != 0)
            row[tag].update({"brute_force_points": int(sub.shape[0]), "brute_force_us": us_b, "brute_force_Mpts_per_s": round(sub.shape[0] / us_b, 3),
                             "brute_force_found_differs": int((f_b != (f_k != 0)).sum()),
                             "brute_force_max_dist_diff": float((d_b[both] - d_k[both]).abs().max()) if bool(both.any()) else None})
    res["grids"][f"G{G}"] = row

# ---- train_step and fit_views at G = 64 ------------------------------------------------------------------------------------------------------
G = 64
tracer = vr.MeshTracer(verts, faces, G, -1.0, 1.0)
grid = tracer.occupancy(1)
h = float(np.max(tracer.h))


def colour_of(p):
    return 0.5 + 0.5 * torch.sin(6.0 * p + torch.tensor([0.0, 2.0, 4.0], device=dev))


views, c2ws = [], []
HV = 128
for elev, azim in ((np.pi / 3, np.pi / 6), (np.pi / 2, np.pi / 6 + np.pi / 2), (np.pi / 2.5, np.pi / 6 + np.pi), (2 * np.pi / 3, np.pi / 6 + 1.5 * np.pi)):
    Kv, c, o, d = camera_rays(elev, azim, HV)
    hit, t, _, _ = tracer.trace(o, d, NEAR, FAR)
    hitf = hit.float()[:, None]
    views.append((hitf * colour_of(o + d * t[:, None]) + (1 - hitf)).reshape(HV, HV, 3))
    c2ws.append(c)
views, c2ws = torch.stack(views), torch.stack(c2ws)


def new_field(anchored):
    torch.manual_seed(1)
    inner = HashGridField.from_grid(grid, n_levels=8, n_features=2, log2_table=15, base_res=8, max_res=256).to(dev)
    if anchored:
        return vr.MeshDensityField(inner, tracer)
    with torch.no_grad():
        inner.mlp.output_linear.bias[3] = 1.0                          # a field that begins at zero density has no gradient
    return inner


fields = {"anchored": new_field(True), "plain": new_field(False)}
opts = {k: torch.optim.Adam(f.parameters(), lr=1e-2) for k, f in fields.items()}
_, _, o128, d128 = camera_rays(ELEV, AZIM, HV)
pick = torch.randint(0, HV * HV, (4096,), device=dev, generator=gen)
o_t, d_t, tgt = o128[pick].contiguous(), d128[pick].contiguous(), views[0].reshape(-1, 3)[pick].contiguous()
kw = dict(occupancy=grid, march=h / 2, white_bkgd=True, generator=gen)
us = alternate([lambda: vr.train_step(fields["anchored"], opts["anchored"], o_t, d_t, tgt, NEAR, FAR, 0, **kw),
                lambda: vr.train_step(fields["plain"], opts["plain"], o_t, d_t, tgt, NEAR, FAR, 0, mesh=tracer, mask_weight=1.0, depth_weight=0.1, **kw)],
               reps)
res["train_step_G64"] = {"rays": 4096, "march": "h / 2", "mesh_density_field_us": us[0], "plain_with_mask_and_depth_us": us[1],
                         "ratio": round(us[0] / us[1], 3)}
fit = {}
for name, anchored in (("anchored", True), ("plain", False)):
    field = new_field(anchored)
    extra = {} if anchored else dict(mesh=tracer, mask_weight=1.0, depth_weight=0.1)
    hist = vr.fit_views(field, views, c2ws, Kv, NEAR, FAR, iters, rays_per_iter=4096, lr=1e-2, seed=0, white_bkgd=True, occupancy=grid,
                        occupancy_every=0, march=h / 2, **extra)
    img = vr.render_image(field, HV, HV, Kv, c2ws[0], NEAR, FAR, 0, white_bkgd=True, occupancy=grid, march=h / 2)
    fit[name] = {"loss_first_five": round(float(np.mean(hist[:5])), 6), "loss_last_five": round(float(np.mean(hist[-5:])), 6),
                 "view0_mse_after": float(((img['rgb'] - views[0]) ** 2).mean()),
                 "view0_acc_mse_after": float(((img['acc'].reshape(-1) - (views[0].reshape(-1, 3) != 1).any(1).float()) ** 2).mean())}
res["fit_views_G64"] = {"views": 4, "size": HV, "iters": iters, "rays_per_iter": 4096, "lr": 1e-2, **fit,
                        "note": "the plain field's loss history includes its mask and depth terms; view0_mse_after is the image alone for both"}
res["device"] = torch.cuda.get_device_name(0)
res["timer"] = "device events, median, alternating"
line = json.dumps(res)
print(line)
with open(os.path.join(ROOT, "profiles", "meshdist_bench.jsonl"), "a") as f:
    f.write(line + "\n")
