#!/usr/bin/env python3
"""What render_rays(occupancy=) buys on the ray path: a ball mask of radius 0.6 at G = 128 over [-1, 1]^3, a pinhole camera at distance
1.5 (fovy 60 deg, near / far 0.5 / 2.5), the 3-D field NeRF2D(63 -> 4, D 8, W 256).

  1. render_image at HW^2 x S (default 512^2 x 128), dense against grid, alternating in one process;
  2. one train_step at 4096 rays x S, dense against grid, whole and split by stage as tools/bench_volume_train.py does (the grid path adds
     select = mark + compact + the host sync, points, expand and collect);
  3. the occupied fraction of the samples of both ray sets;
  4. mark, compact, points and expand on their own at HW^2 x S, beside the bytes they move and the time 8 TB/s would take for them;
  5. the saved-activation bytes of the training forward of both paths.

Device events, median after warm-up; the yardstick is the dense path of the same process.  Expectation to hold the figures against:
time = fraction x dense + the select kernels + one sync per pass.  Appends one JSON line to profiles/occupancy_bench.jsonl.
Usage: python tools/bench_occupancy.py [HW = 512] [S = 128] [render repetitions = 5] [step repetitions = 11]"""
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
assert torch.cuda.is_available(), "bench_occupancy needs the GPU"
dev = torch.device('cuda:0')
lib = L.load()
torch.manual_seed(0)
G, RADIUS, NEAR, FAR, RT = 128, 0.6, 0.5, 2.5, 4096

c = (torch.arange(G, device=dev, dtype=torch.float32) + 0.5) / G * 2 - 1
ball = (c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2) < RADIUS ** 2
grid = vr.OccupancyGrid.from_mask(ball, -1.0, 1.0)
field = rnh.NeRF2D(D=8, W=256, input_ch=63, output_ch=4, skips=[4]).to(dev)
with torch.no_grad():
    field.output_linear.bias[3] = 1.0
K = vr.pinhole(HW, HW)
c2w = torch.tensor([[1., 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1.5]], device=dev)


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
    return [round(statistics.median(t), 1) for t in ts]


res = {"metric": "ray path with an occupancy grid (render_rays(occupancy=)), dense path of the same process as yardstick",
       "case": {"grid": G, "mask": f"ball of radius {RADIUS}", "box": [-1, 1], "camera_distance": 1.5, "fovy_deg": 60, "near_far": [NEAR, FAR],
                "samples": S, "field": {"D": 8, "W": 256}}, "grid_fraction": round(grid.fraction(), 4)}

# ---- 1. render_image ------------------------------------------------------------------------------------------------------------------
dense_us, grid_us = alternate([lambda: vr.render_image(field, HW, HW, K, c2w, NEAR, FAR, S),
                               lambda: vr.render_image(field, HW, HW, K, c2w, NEAR, FAR, S, occupancy=grid)], reps_render, warm=1)
ro, rd = rnh.get_rays(HW, HW, K, c2w)
ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
R = ro.shape[0]
t = torch.linspace(0., 1., S, device=dev)
z = (NEAR * (1. - t) + FAR * t).expand(R, S).contiguous()
n_render = grid.select(ro, rd, z).numel()
res["render"] = {"rays": R, "dense_us": dense_us, "grid_us": grid_us, "ratio": round(grid_us / dense_us, 4),
                 "sample_fraction": round(n_render / (R * S), 4), "repetitions": reps_render}

# ---- 4. the select kernels alone at the render's size ---------------------------------------------------------------------------------
total = R * S
mask = torch.empty(total, dtype=torch.uint8, device=dev)
idx_buf = torch.empty(total, dtype=torch.int32, device=dev)
count = torch.empty(1, dtype=torch.int64, device=dev)
ws = torch.empty(lib.ctx_texel_compact_ws_bytes(total), dtype=torch.uint8, device=dev)
idx = grid.select(ro, rd, z)
n = idx.numel()
pts = torch.empty(n, 3, device=dev)
raw_c = torch.randn(n, 4, device=dev)
raw = torch.empty(total, 4, device=dev)
kern = {
    "mark": (lambda: L.check(lib.ctx_occ_mark(L.ptr(ro), L.ptr(rd), L.ptr(z), R, S, L.ptr(grid.cells), G, *map(float, grid.lo), *map(float, grid.inv),
                                              L.ptr(mask), L.stream())), total * 5 + R * 24),
    "compact": (lambda: L.check(lib.ctx_texel_compact(L.ptr(mask), total, L.ptr(idx_buf), L.ptr(count), L.ptr(ws), L.stream())), total * 2 + n * 4),
    "points": (lambda: L.check(lib.ctx_occ_points(L.ptr(ro), L.ptr(rd), L.ptr(z), R, S, L.ptr(idx), n, L.ptr(pts), L.stream())), n * (4 + 4 + 12)),
    "expand": (lambda: L.check(lib.ctx_occ_expand(L.ptr(raw_c), L.ptr(idx), n, total, L.ptr(raw), L.stream())), total * 16 + n * (16 + 4 + 16)),
}
us = alternate([k[0] for k in kern.values()], 21, warm=3)
res["select_kernels"] = {name: {"us": u, "bytes": b, "floor_us_at_8TBps": round(b / 8e6, 1)} for (name, (_, b)), u in zip(kern.items(), us)}
res["select_kernels"]["sum_us"] = round(sum(us), 1)
del mask, idx_buf, raw, raw_c, pts, idx, z, ws

# ---- 2. one training step at 4096 rays ------------------------------------------------------------------------------------------------
pick = torch.randint(0, R, (RT,), device=dev)
ro_t, rd_t = ro[pick].contiguous(), rd[pick].contiguous()
target = torch.rand(RT, 3, device=dev)
opt = torch.optim.Adam(field.parameters(), lr=5e-4)
step_dense, step_grid = alternate([lambda: vr.train_step(field, opt, ro_t, rd_t, target, NEAR, FAR, S),
                                   lambda: vr.train_step(field, opt, ro_t, rd_t, target, NEAR, FAR, S, occupancy=grid)], reps_step, warm=3)
zt = (NEAR * (1. - t) + FAR * t).expand(RT, S).contiguous()
n_step = grid.select(ro_t, rd_t, zt).numel()
res["train_step"] = {"rays": RT, "dense_us": step_dense, "grid_us": step_grid, "ratio": round(step_grid / step_dense, 4),
                     "sample_fraction": round(n_step / (RT * S), 4), "repetitions": reps_step}


def staged(with_grid):
    """One forward / backward with the graph cut at raw, so that the field's and the compositing's backward are timed apart."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(9)]
    field.zero_grad(set_to_none=True)
    ev[0].record()
    if with_grid:
        idx = grid.select(ro_t, rd_t, zt)
        ev[1].record()
        p = torch.empty(idx.numel(), 3, device=dev)
        L.check(lib.ctx_occ_points(L.ptr(ro_t), L.ptr(rd_t), L.ptr(zt), RT, S, L.ptr(idx), idx.numel(), L.ptr(p), L.stream()))
    else:
        ev[1].record()
        p = ro_t[:, None, :] + rd_t[:, None, :] * zt[:, :, None]
    ev[2].record()
    raw_f = field.forward_pts(p)
    ev[3].record()
    leaf = raw_f.detach().requires_grad_(True)
    full = rnh._OccExpandFn.apply(leaf, idx, RT * S).view(RT, S, 4) if with_grid else leaf
    ev[4].record()
    rgb = rnh.raw2outputs(full, zt, rd_t)[0]
    ev[5].record()
    g_rgb, = torch.autograd.grad(rnh.img2mse(rgb, target), rgb)
    ev[6].record()
    rgb.backward(g_rgb)                                                # compositing backward (+ collect on the grid path)
    ev[7].record()
    raw_f.backward(leaf.grad)
    ev[8].record()
    ev[8].synchronize()
    names = ("select_us", "points_us", "field_fwd_us", "expand_us", "composite_fwd_us", None, "composite_bwd_collect_us", "field_bwd_us")
    return {k: ev[i].elapsed_time(ev[i + 1]) * 1e3 for i, k in enumerate(names) if k}


for with_grid in (False, True):
    runs = [staged(with_grid) for _ in range(3 + reps_step)][3:]
    res["train_step"]["stages_grid" if with_grid else "stages_dense"] = {k: round(statistics.median(r[k] for r in runs), 1) for k in runs[0]}

# ---- 5. saved activations ---------------------------------------------------------------------------------------------------------------
saved = lambda m: int(lib.ctx_uvmlp_saved_bytes(m, field.D, field.W, field.input_ch))
res["saved_activation_bytes"] = {"dense": saved(RT * S), "grid": saved(n_step)}
res["device"] = torch.cuda.get_device_name(0)
res["timer"] = "device events, median"
line = json.dumps(res)
print(line)
with open(os.path.join(ROOT, "profiles", "occupancy_bench.jsonl"), "a") as f:
    f.write(line + "\n")
