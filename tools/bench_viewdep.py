#!/usr/bin/env python3
"""What view-dependent colour (hashgrid.ViewDependentField) costs on the marched ray path, beside the HashGridField it
extends, on the scene of tools/bench_hashgrid.py (spot, G 128, dilate 1, march = h) in one process.  A tool, not a gate.

  1. the four glue kernels of csrc/viewdep.hip on their own at the marched points of the HW^2 image and of 4096 training rays (E = 32,
     deg = 4), beside the HBM bytes they must move and the time 8 TB/s would take;
  2. render_image at HW^2 rays and one train_step at 4096 rays for both fields, alternating.

Device events, median after warm-up.  Appends one JSON line to profiles/viewdep_bench.jsonl.
Usage: python tools/bench_viewdep.py [HW = 512] [render repetitions = 5] [step repetitions = 11]"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from contexture_nerf_amd import _lib as L, run_nerf_helpers as rnh, volume_render as vr
from contexture_nerf_amd.hashgrid import HashGridField, ViewDependentField

HW = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps_render = int(sys.argv[2]) if len(sys.argv) > 2 else 5
reps_step = int(sys.argv[3]) if len(sys.argv) > 3 else 11
assert torch.cuda.is_available(), "bench_viewdep needs the GPU"
dev = torch.device('cuda:0')
lib = L.load()
torch.manual_seed(0)
G0, NEAR, FAR, RT, DEG = 128, 0.5, 2.5, 4096, 4

m = np.load(os.path.join(ROOT, "shapes", "meshes.npz"))
verts = torch.tensor(m["spot_triangulated_v"], dtype=torch.float32, device=dev)
faces = torch.tensor(m["spot_triangulated_f"].astype(np.int64), device=dev)
verts = verts - verts.mean(dim=0)                                     # Mesh.normalize_mesh(target_scale=0.6, dy=0.25)
verts = verts / torch.max(torch.norm(verts, p=2, dim=1)) * 0.6
verts[:, 1] += 0.25
verts = verts.contiguous()
grid = vr.OccupancyGrid.from_mesh(verts, faces, G0, -1.0, 1.0, dilate=1)
STEP = float(grid.h[0])
fields = {"hashgrid": HashGridField.from_grid(grid).to(dev), "view_dependent": ViewDependentField.from_grid(grid, sh_degree=DEG).to(dev)}
with torch.no_grad():
    for f in fields.values():
        f.mlp.output_linear.bias[3] = 1.0
    torch.nn.init.normal_(fields["view_dependent"].dir_mlp.output_linear.weight, std=0.1)
E = fields["view_dependent"].encoding.out_dim
KK = DEG * DEG
K = vr.pinhole(HW, HW)
c2w = torch.tensor([[1., 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1.5]], device=dev)
ro, rd = rnh.get_rays(HW, HW, K, c2w)
ro, rd = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()
R = ro.shape[0]
pick = torch.randint(0, R, (RT,), device=dev)
ro_t, rd_t = ro[pick].contiguous(), rd[pick].contiguous()
target = torch.rand(RT, 3, device=dev)


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


res = {"metric": "view-dependent colour (SH degree 4 into a 2 x 64 residual net) beside the position-only hash-grid field on the marched ray path",
       "case": {"mesh": "spot_triangulated", "G": G0, "dilate": 1, "march": STEP, "near_far": [NEAR, FAR], "image": HW, "train_rays": RT,
                "E": E, "sh_degree": DEG}}

# ---- 1. the kernels alone ------------------------------------------------------------------------------------------------------------
kern, keep = {}, []
for tag, (o, d) in (("image", (ro, rd)), ("train", (ro_t, rd_t))):
    _, ray_id, _, _, pts = grid.march(o, d, NEAR, FAR, STEP)
    n, Rn = int(pts.shape[0]), int(d.shape[0])
    emb, inp, g_emb = torch.randn(n, E, device=dev), torch.empty(n, E + KK, device=dev), torch.empty(n, E, device=dev)
    base, resid, raw, g_res = torch.randn(n, 4, device=dev), torch.randn(n, 3, device=dev), torch.empty(n, 4, device=dev), torch.empty(n, 3, device=dev)
    keep.append((ray_id, emb, inp, g_emb, base, resid, raw, g_res))
    s = L.stream
    kern[f"input_fwd_{tag}"] = (lambda e=emb, i=ray_id, d=d, x=inp, n=n, Rn=Rn: L.check(lib.ctx_viewdep_input_fwd(
        L.ptr(e), L.ptr(d), L.ptr(i), n, Rn, E, DEG, L.ptr(x), s())), n * (E * 4 + 4 + (E + KK) * 4), n)
    kern[f"input_bwd_{tag}"] = (lambda x=inp, g=g_emb, n=n: L.check(lib.ctx_viewdep_input_bwd(L.ptr(x), n, E, DEG, L.ptr(g), s())),
                                n * 2 * E * 4, n)
    kern[f"raw_fwd_{tag}"] = (lambda b=base, r=resid, x=raw, n=n: L.check(lib.ctx_viewdep_raw_fwd(L.ptr(b), L.ptr(r), n, L.ptr(x), s())),
                              n * (16 + 12 + 16), n)
    kern[f"raw_bwd_{tag}"] = (lambda b=base, g=g_res, n=n: L.check(lib.ctx_viewdep_raw_bwd(L.ptr(b), n, L.ptr(g), s())), n * (16 + 12), n)
us = alternate([k[0] for k in kern.values()], 21, warm=3)
res["kernels"] = {name: {"us": u, "n": n, "hbm_bytes": b, "floor_us_at_8TBps": round(b / 8e6, 2)} for (name, (_, b, n)), u in zip(kern.items(), us)}
del keep, kern

# ---- 2. render_image and train_step, both fields -------------------------------------------------------------------------------------
kw = dict(occupancy=grid, march=STEP)
names = list(fields)
us = alternate([(lambda f=f: vr.render_image(f, HW, HW, K, c2w, NEAR, FAR, 0, **kw)) for f in fields.values()], reps_render, warm=1)
res["render"] = {"rays": R, "n": int(grid.march(ro, rd, NEAR, FAR, STEP)[2].numel()), "repetitions": reps_render,
                 **{f"{k}_us": u for k, u in zip(names, us)}}
opts = {k: torch.optim.Adam(f.parameters(), lr=5e-4) for k, f in fields.items()}
us = alternate([(lambda k=k: vr.train_step(fields[k], opts[k], ro_t, rd_t, target, NEAR, FAR, 0, **kw)) for k in names], reps_step, warm=3)
res["train_step"] = {"rays": RT, "repetitions": reps_step, **{f"{k}_us": u for k, u in zip(names, us)}}

res["device"] = torch.cuda.get_device_name(0)
res["timer"] = "device events, median"
line = json.dumps(res)
print(line)
with open(os.path.join(ROOT, "profiles", "viewdep_bench.jsonl"), "a") as f:
    f.write(line + "\n")
