#!/usr/bin/env python3
"""What the importance-resampled second pass on the marched lists (resample=K) costs and buys, beside a shorter march
step.  Mesh, grid (G 128, dilate 1), camera, box and field are those of tools/bench_march.py.

  a. ctx_resample_packed alone at K in {8, 16, 32, 64} on the march = h lists, beside the bytes it must move (12 B per coarse sample, 16 B
     per ray and 24 B per hit ray read, 24 B per fine sample written with xi null), the time 8 TB/s would take, and the packed compositing
     launches on the same lists.  The count takes the coarse lists as read once, which is what the algorithm needs; the kernel reads them
     1 + ceil(K / 64) times in full (sweep one, then once per output chunk), from cache after the first;
  b. render_image at HW^2 rays for march = h with resample in {8, 16, 32} against plain march = h, h/2, h/4: time, n, n';
  c. one train_step at 4096 rays for the same variants, and the resampled ones by stage; the resample stage is timed as the host call
     (cumsum, the read-back of n', the draw, the launch), so what it has over the kernel alone is the second sync;
  d. the toy scene of section 4e (from_mesh(icosphere 0.6, G 16, dilate 1), `iters` iterations of fit_views, one seed): the loss over the
     first and last five iterations and the mean |depth / acc - analytic ray-sphere depth| over the rays that hit the sphere, for march = h/2
     and for march = h with resample = K, K chosen so that the points per hit ray are about equal.

Device events, variants alternating in one process, median after warm-up.  Appends one JSON line to profiles/resample_bench.jsonl.
Usage: python tools/bench_resample.py [HW = 512] [render repetitions = 5] [step repetitions = 11] [iters = 40]"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from contexture_nerf_amd import _lib as L, run_nerf_helpers as rnh, volume_render as vr

HW = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps_render = int(sys.argv[2]) if len(sys.argv) > 2 else 5
reps_step = int(sys.argv[3]) if len(sys.argv) > 3 else 11
ITERS = int(sys.argv[4]) if len(sys.argv) > 4 else 40
assert torch.cuda.is_available(), "bench_resample needs the GPU"
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
field = rnh.NeRF2D(D=8, W=256, input_ch=63, output_ch=4, skips=[4]).to(dev)
with torch.no_grad():
    field.output_linear.bias[3] = 1.0
K = vr.pinhole(HW, HW)
c2w = torch.tensor([[1., 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1.5]], device=dev)
ro, rd = rnh.get_rays(HW, HW, K, c2w)
ro, rd = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()
R = ro.shape[0]
KS_KERNEL, KS = (8, 16, 32, 64), (8, 16, 32)
VARIANTS = {"march_h": dict(march=H_CELL), "march_h/2": dict(march=H_CELL / 2), "march_h/4": dict(march=H_CELL / 4),
            **{f"march_h_resample_{k}": dict(march=H_CELL, resample=k) for k in KS}}


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


def counts(o, d, kw):
    """n, hit rays and n' of a variant on the rays o, d."""
    ray_off = grid.march(o, d, NEAR, FAR, kw["march"])[0]
    hit = int((ray_off[1:] > ray_off[:-1]).sum())
    n = int(ray_off[-1])
    n1 = hit * kw.get("resample", 0)
    return {"n": n, "hit_rays": hit, "n_fine": n1, "points_per_hit_ray": round((n + n1) / max(hit, 1), 2)}


res = {"metric": "importance resampling of the marched lists (resample=K on march=h) beside the plain march at h, h/2 and h/4",
       "case": {"mesh": "spot_triangulated", "scale": 0.6, "dy": 0.25, "G": G0, "dilate": 1, "cell": H_CELL, "box": [-1, 1],
                "camera_distance": 1.5, "fovy_deg": 60, "near_far": [NEAR, FAR], "field": {"D": 8, "W": 256}, "rays": R,
                "occupied_cells": round(grid.fraction(), 4)}}

# ---- a. the kernel alone ---------------------------------------------------------------------------------------------------------------------
ray_off, ray_id, tt, dt, pts, ts = grid.march(ro, rd, NEAR, FAR, H_CELL, starts=True)
n = int(tt.numel())
hit = int((ray_off[1:] > ray_off[:-1]).sum())
with torch.no_grad():
    w = rnh.raw2outputs_packed(field.forward_pts(pts), tt, dt, rd, ray_off)[3].contiguous()
kern, keep = {}, []
for k in KS_KERNEL:
    fine_off = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    fine_off[1:] = torch.cumsum(ray_off[1:] > ray_off[:-1], 0) * k
    n1 = hit * k
    outs = (torch.empty(n1, dtype=torch.int32, device=dev), torch.empty(n1, device=dev), torch.empty(n1, device=dev), torch.empty(n1, 3, device=dev))
    keep.append((fine_off, outs))
    kern[f"resample_K{k}"] = (lambda k=k, x=keep[-1], n1=n1: L.check(lib.ctx_resample_packed(
        L.ptr(w), L.ptr(ts), L.ptr(dt), L.ptr(ray_off), L.ptr(ro), L.ptr(rd), R, n, k, L.ptr(x[0]), None, n1, *[L.ptr(o) for o in x[1]],
        L.stream())), n * 12 + R * 16 + hit * 24 + n1 * 24, n1)
raw = torch.randn(n, 4, device=dev)
couts = [torch.empty(R, 3, device=dev), torch.empty(R, device=dev), torch.empty(R, device=dev), torch.empty(n, device=dev), torch.empty(R, device=dev)]
g_rgb, grad = torch.randn(R, 3, device=dev), torch.empty(n, 4, device=dev)
kern["packed_fwd_h"] = (lambda: L.check(lib.ctx_raymarch_packed_fwd(L.ptr(raw), L.ptr(tt), L.ptr(dt), L.ptr(rd), None, L.ptr(ray_off), R, n, 1,
                                                                     *[L.ptr(o) for o in couts], L.stream())), n * 28 + R * 52, n)
kern["packed_bwd_h"] = (lambda: L.check(lib.ctx_raymarch_packed_bwd(L.ptr(raw), L.ptr(tt), L.ptr(dt), L.ptr(rd), None, L.ptr(ray_off), R, n, 1,
                                                                     L.ptr(g_rgb), None, None, None, None, L.ptr(grad), L.stream())),
                        n * 40 + R * 40, n)
us = alternate([k[0] for k in kern.values()], 21, warm=3)
res["kernels"] = {"n": n, "hit_rays": hit, **{name: {"us": u, "bytes": b, "floor_us_at_8TBps": round(b / 8e6, 2), "elements": e}
                                              for (name, (_, b, e)), u in zip(kern.items(), us)}}
del keep, kern

# ---- b. render_image ---------------------------------------------------------------------------------------------------------------------------
us = alternate([(lambda kw=kw: vr.render_image(field, HW, HW, K, c2w, NEAR, FAR, 0, occupancy=grid, **kw)) for kw in VARIANTS.values()],
               reps_render, warm=1)
res["render"] = {"repetitions": reps_render, **{name: {"us": u, **counts(ro, rd, kw)} for (name, kw), u in zip(VARIANTS.items(), us)}}

# ---- c. train_step, whole and by stage -----------------------------------------------------------------------------------------------------------
pick = torch.randint(0, R, (RT,), device=dev)
ro_t, rd_t = ro[pick].contiguous(), rd[pick].contiguous()
target = torch.rand(RT, 3, device=dev)
opt = torch.optim.Adam(field.parameters(), lr=5e-4)
us = alternate([(lambda kw=kw: vr.train_step(field, opt, ro_t, rd_t, target, NEAR, FAR, 0, occupancy=grid, **kw)) for kw in VARIANTS.values()],
               reps_step, warm=3)
res["train_step"] = {"repetitions": reps_step, "rays": RT,
                     **{name: {"us": u, **counts(ro_t, rd_t, kw)} for (name, kw), u in zip(VARIANTS.items(), us)}}
stages = {}
for k in KS:
    acc = {s: [] for s in ("march", "field_fwd_coarse", "composite_coarse", "resample_with_sync", "field_fwd_fine", "composite_fine", "loss",
                           "backward", "optimizer")}
    for rep in range(3 + reps_step):
        opt.zero_grad(set_to_none=True)
        a, lists = timed(lambda: grid.march(ro_t, rd_t, NEAR, FAR, H_CELL, perturb=True, starts=True))
        b, raw0 = timed(lambda: field.forward_pts(lists[4]))
        c, out0 = timed(lambda: rnh.raw2outputs_packed(raw0, lists[2], lists[3], rd_t, lists[0]))
        d_, fine = timed(lambda: rnh.resample_packed(out0[3].detach(), lists[5], lists[3], lists[0], ro_t, rd_t, k, perturb=True))
        e, raw1 = timed(lambda: field.forward_pts(fine[4]))
        f, out1 = timed(lambda: rnh.raw2outputs_packed(raw1, fine[2], fine[3], rd_t, fine[0]))
        g, loss = timed(lambda: rnh.img2mse(out1[0], target) + rnh.img2mse(out0[0], target))
        h, _ = timed(lambda: loss.backward())
        i, _ = timed(lambda: opt.step())
        if rep >= 3:
            for s, v in zip(acc, (a, b, c, d_, e, f, g, h, i)):
                acc[s].append(v)
    stages[f"march_h_resample_{k}"] = {s: round(statistics.median(v), 1) for s, v in acc.items()}
    stages[f"march_h_resample_{k}"].update({"n": int(lists[2].numel()), "n_fine": int(fine[2].numel())})
res["train_step_stages_us"] = stages

# ---- d. the toy scene: loss and depth error at equal points per hit ray ------------------------------------------------------------------------------
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_occupancy_mesh_cpu as OM                                    # icosphere, ball_mask: the scene's definition
G, Hv, Wv, RADIUS = 16, 16, 16, 0.6


def toy_field(seed, sigma_bias=0.5):
    torch.manual_seed(seed)
    net = rnh.NeRF2D(D=8, W=64, input_ch=63, output_ch=4, skips=[4]).to(dev)
    with torch.no_grad():
        net.output_linear.bias[3] = sigma_bias
    return net


def shell():
    v, f = OM.icosphere(2, RADIUS)
    return vr.OccupancyGrid.from_mesh(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), G, -1.0, 1.0, dilate=1)


teacher_grid = vr.OccupancyGrid.from_mask(torch.from_numpy(OM.ball_mask(G, RADIUS)).to(dev), -1.0, 1.0)
teacher = toy_field(1, 8.0)
Kv = vr.pinhole(Hv, Wv)
c2ws = torch.tensor([[[1., 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1.5]], [[0., 0, 1, 1.5], [0, 1, 0, 0], [-1, 0, 0, 0]]], device=dev)
imgs = torch.stack([vr.render_image(teacher, Hv, Wv, Kv, c2ws[v], NEAR, FAR, 32, white_bkgd=True, occupancy=teacher_grid)['rgb'] for v in range(2)])
rays = [rnh.get_rays(Hv, Wv, Kv, c2ws[v]) for v in range(2)]
o_all = torch.stack([r[0] for r in rays]).reshape(-1, 3).contiguous()
d_all = torch.stack([r[1] for r in rays]).reshape(-1, 3).contiguous()
o64, d64 = o_all.double(), d_all.double()
qa, qb, qc = (d64 * d64).sum(-1), 2 * (o64 * d64).sum(-1), (o64 * o64).sum(-1) - RADIUS ** 2
disc = qb * qb - 4 * qa * qc
on_sphere = disc > 0
analytic = ((-qb - torch.sqrt(disc.clamp_min(0))) / (2 * qa))
h16 = float(shell().h[0])
g_ = shell()
c_h, c_h2 = (g_.march(o_all, d_all, NEAR, FAR, s)[0] for s in (h16, h16 / 2))
hit16 = int((c_h[1:] > c_h[:-1]).sum())
K_equal = max(1, round((int(c_h2[-1]) - int(c_h[-1])) / hit16))
toy = {"G": G, "views": 2, "HW": Hv, "iters": ITERS, "rays_per_iter": 256, "K_equal_points": K_equal,
       "points_per_hit_ray": {"march_h/2": round(int(c_h2[-1]) / hit16, 2), "march_h_resample": round(int(c_h[-1]) / hit16 + K_equal, 2)}}
for name, kw in (("march_h/2", dict(march=h16 / 2)), ("march_h_resample", dict(march=h16, resample=K_equal)), ("march_h", dict(march=h16))):
    student, g_ = toy_field(2), shell()
    hist = vr.fit_views(student, imgs, c2ws, Kv, NEAR, FAR, ITERS, rays_per_iter=256, seed=3, raw_noise_std=1., white_bkgd=True, occupancy=g_,
                        occupancy_every=0, **kw)
    with torch.no_grad():
        out = rnh.render_rays(student, o_all, d_all, NEAR, FAR, 0, white_bkgd=True, occupancy=g_, **kw)
    use = on_sphere & (out[2] > 1e-3)
    err = (out[4].double() / out[2].double() - analytic)[use].abs().mean()
    toy[name] = {"loss_first5": round(float(np.mean(hist[:5])), 5), "loss_last5": round(float(np.mean(hist[-5:])), 5),
                 "depth_over_acc_abs_err": round(float(err), 5), "rays_compared": int(use.sum()), "mean_acc": round(float(out[2][use].mean()), 4)}
res["toy_scene"] = toy

res["device"] = torch.cuda.get_device_name(0)
res["timer"] = "device events, median"
line = json.dumps(res)
print(line)
with open(os.path.join(ROOT, "profiles", "resample_bench.jsonl"), "a") as f:
    f.write(line + "\n")
