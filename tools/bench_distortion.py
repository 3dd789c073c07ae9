#!/usr/bin/env python3
"""What the distortion loss on the marched sample lists (distortion=) costs.  The setting is that of tools/bench_march.py:
spot, G 128, dilate 1, HW^2 rays, march in {h, h/2, h/4}.

  a. ctx_distortion_packed_fwd and _bwd alone, beside the bytes they must move (12 B per sample read + 4 B per ray written forward,
     12 + 4 B per sample backward) and the time 8 TB/s would take, and beside ctx_raymarch_packed_fwd / _bwd on the same lists;
  b. the same loss composed from torch ops on the packed lists (cumsum plus ray_id indexing), forward + backward: what the kernels replace;
  c. one train_step at 4096 rays with distortion 0 and 0.01.

One process, the variants alternate, device events, median after warm-up.  Appends one JSON line to profiles/distortion_bench.jsonl.
Usage: python tools/bench_distortion.py [HW = 512] [kernel repetitions = 21] [step repetitions = 11]"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from contexture_nerf_amd import _lib as L, run_nerf_helpers as rnh, volume_render as vr

HW = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps_kernel = int(sys.argv[2]) if len(sys.argv) > 2 else 21
reps_step = int(sys.argv[3]) if len(sys.argv) > 3 else 11
assert torch.cuda.is_available(), "bench_distortion needs the GPU"
dev = torch.device('cuda:0')
lib = L.load()
torch.manual_seed(0)
G0, NEAR, FAR, RT, LAMBDA = 128, 0.5, 2.5, 4096, 0.01

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


def torch_distortion(w, t, dt, d, ray_off, ray_id):
    """The prefix form from torch ops: one cumsum over all lists, made per-ray by subtracting its value at the ray's first sample."""
    nrm = torch.linalg.norm(d, dim=-1)[ray_id]
    first = ray_off[:-1][ray_id]
    x, dl = (t - t[first]) * nrm, dt * nrm
    wx = w * x
    cw, cv = torch.cumsum(w, 0), torch.cumsum(wx, 0)
    Wex, Vex = (cw - w) - (cw - w)[first], (cv - wx) - (cv - wx)[first]
    per = w * (2. * (x * Wex - Vex) + dl * w / 3.)
    return torch.zeros(d.shape[0], device=w.device).index_add_(0, ray_id, per)


res = {"metric": "distortion loss on the marched sample lists: the two HIP launches alone, the torch composition they replace, and train_step "
                 "with and without distortion=",
       "case": {"mesh": "spot_triangulated", "scale": 0.6, "dy": 0.25, "G": G0, "dilate": 1, "cell": H_CELL, "box": [-1, 1],
                "camera_distance": 1.5, "fovy_deg": 60, "near_far": [NEAR, FAR], "rays": R, "field": {"D": 8, "W": 256}, "lambda": LAMBDA}}

# ---- a. the kernels alone, b. the torch composition ---------------------------------------------------------------------------------------------
kern, keep, agree = {}, [], {}
for k, step in STEPS.items():
    ray_off, ray_id, tt, dt, pts = grid.march(ro, rd, NEAR, FAR, step)
    n = int(tt.numel())
    raw = torch.randn(n, 4, device=dev)
    outs = [torch.empty(R, 3, device=dev), torch.empty(R, device=dev), torch.empty(R, device=dev), torch.empty(n, device=dev), torch.empty(R, device=dev)]
    L.check(lib.ctx_raymarch_packed_fwd(L.ptr(raw), L.ptr(tt), L.ptr(dt), L.ptr(rd), None, L.ptr(ray_off), R, n, 1, *[L.ptr(o) for o in outs],
                                        L.stream()))
    w = outs[3]                                                         # real weights of a random field
    loss, g_loss, grad_w = torch.empty(R, device=dev), torch.full((R,), 1.0 / R, device=dev), torch.empty(n, device=dev)
    g_rgb, grad_raw = torch.randn(R, 3, device=dev), torch.empty(n, 4, device=dev)
    rid = ray_id.long()
    x = (ray_off, tt, dt, raw, outs, w, loss, g_loss, grad_w, g_rgb, grad_raw, rid)
    keep.append(x)
    kern[f"distortion_fwd_{k}"] = (lambda x=x, n=n: L.check(lib.ctx_distortion_packed_fwd(
        L.ptr(x[5]), L.ptr(x[1]), L.ptr(x[2]), L.ptr(rd), L.ptr(x[0]), R, n, L.ptr(x[6]), L.stream())), n * 12 + R * 4, n)
    kern[f"distortion_bwd_{k}"] = (lambda x=x, n=n: L.check(lib.ctx_distortion_packed_bwd(
        L.ptr(x[5]), L.ptr(x[1]), L.ptr(x[2]), L.ptr(rd), L.ptr(x[0]), R, n, L.ptr(x[7]), L.ptr(x[8]), L.stream())), n * 16, n)
    kern[f"packed_fwd_{k}"] = (lambda x=x, n=n: L.check(lib.ctx_raymarch_packed_fwd(
        L.ptr(x[3]), L.ptr(x[1]), L.ptr(x[2]), L.ptr(rd), None, L.ptr(x[0]), R, n, 1, *[L.ptr(o) for o in x[4]], L.stream())), n * 28 + R * 52, n)
    kern[f"packed_bwd_{k}"] = (lambda x=x, n=n: L.check(lib.ctx_raymarch_packed_bwd(
        L.ptr(x[3]), L.ptr(x[1]), L.ptr(x[2]), L.ptr(rd), None, L.ptr(x[0]), R, n, 1, L.ptr(x[9]), None, None, None, None, L.ptr(x[10]),
        L.stream())), n * 40 + R * 40, n)

    def host_pair(x=x):
        wg = x[5].detach().requires_grad_(True)
        rnh.distortion_loss(wg, x[1], x[2], rd, x[0]).mean().backward()
        return wg.grad

    def torch_pair(x=x):
        wg = x[5].detach().requires_grad_(True)
        torch_distortion(wg, x[1], x[2], rd, x[0], x[11]).mean().backward()
        return wg.grad
    kern[f"host_fwd_bwd_{k}"] = (host_pair, n * 28 + R * 8, n)
    kern[f"torch_fwd_bwd_{k}"] = (torch_pair, 0, n)
    a, b = host_pair(), torch_pair()
    agree[k] = float((a - b).abs().max() / a.abs().max())              # the two compositions compute one thing
us = alternate([v[0] for v in kern.values()], reps_kernel)
res["kernels"] = {name: {"us": u, "bytes": b, "floor_us_at_8TBps": round(b / 8e6, 2), "n": n} for (name, (_, b, n)), u in zip(kern.items(), us)}
res["torch_vs_hip_max_rel_grad_difference"] = agree
res["kernel_repetitions"] = reps_kernel
del keep, kern

# ---- c. train_step at 4096 rays ---------------------------------------------------------------------------------------------------------------------
pick = torch.randint(0, R, (RT,), device=dev)
ro_t, rd_t = ro[pick].contiguous(), rd[pick].contiguous()
target = torch.rand(RT, 3, device=dev)
opt = torch.optim.Adam(field.parameters(), lr=5e-4)
fns, names = [], []
for k, step in STEPS.items():
    for lam in (0., LAMBDA):
        fns.append(lambda step=step, lam=lam: vr.train_step(field, opt, ro_t, rd_t, target, NEAR, FAR, 128, occupancy=grid, march=step, distortion=lam))
        names.append(f"march_{k}_lambda_{lam:g}")
us = alternate(fns, reps_step)
res["train_step"] = {"rays": RT, "repetitions": reps_step, **{f"{n}_us": u for n, u in zip(names, us)},
                     **{f"march_{k}_added_us": round(us[2 * i + 1] - us[2 * i], 1) for i, k in enumerate(STEPS)}}

res["device"] = torch.cuda.get_device_name(0)
res["timer"] = "device events, median"
line = json.dumps(res)
print(line)
with open(os.path.join(ROOT, "profiles", "distortion_bench.jsonl"), "a") as f:
    f.write(line + "\n")
