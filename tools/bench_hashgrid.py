#!/usr/bin/env python3
"""What the multiresolution hash-grid field (hashgrid.HashGridField) costs on the marched ray path, beside the 8 x 256
Fourier-feature field it replaces, on the scene of tools/bench_march.py (spot, G 128, dilate 1, march = h) in one process.

  1. the kernels on their own at the two ends of section 4g's tables (the marched points of the HW^2 image and of 4096 training rays):
     ctx_hashgrid_fwd, ctx_hashgrid_bwd whole and split into zero / accumulate / convert, and the grad_emb kernel (ctx_uvmlp_bwd_emb with
     and without the input gradient), beside the HBM bytes they must move and the time 8 TB/s would take; the achieved rate of the 64-bit
     integer adds (adds x 8 bytes / accumulate time);
  2. render_image at HW^2 rays and one train_step at 4096 rays for both fields, alternating;
  3. the train_step by stage (march, field forward, compositing, loss, backward, optimizer) for both fields;
  4. the bytes a pass keeps alive between forward and backward.

Device events, median after warm-up.  Appends one JSON line to profiles/hashgrid_bench.jsonl.
Usage: python tools/bench_hashgrid.py [HW = 512] [render repetitions = 5] [step repetitions = 11]"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ctypes as C
import numpy as np
import torch
from contexture_nerf_amd import _lib as L, run_nerf_helpers as rnh, volume_render as vr
from contexture_nerf_amd.hashgrid import HashGridField

HW = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps_render = int(sys.argv[2]) if len(sys.argv) > 2 else 5
reps_step = int(sys.argv[3]) if len(sys.argv) > 3 else 11
assert torch.cuda.is_available(), "bench_hashgrid needs the GPU"
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
STEP = float(grid.h[0])
fields = {"fourier_8x256": rnh.NeRF2D(D=8, W=256, input_ch=63, output_ch=4, skips=[4]).to(dev), "hashgrid": HashGridField.from_grid(grid).to(dev)}
with torch.no_grad():
    fields["fourier_8x256"].output_linear.bias[3] = 1.0
    fields["hashgrid"].mlp.output_linear.bias[3] = 1.0
hg = fields["hashgrid"]
enc, mlp = hg.encoding, hg.mlp
Lv, F, log2T = enc.n_levels, enc.n_features, enc.log2_table
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


res = {"metric": "hash-grid field (16 levels x 2 features, T = 2^19, MLP 2 x 64) beside the 8 x 256 Fourier field on the marched ray path",
       "case": {"mesh": "spot_triangulated", "G": G0, "dilate": 1, "march": STEP, "near_far": [NEAR, FAR], "image": HW, "train_rays": RT,
                "levels": Lv, "features": F, "log2_table": log2T, "res": enc.res.tolist(),
                "dense_levels": int(sum((int(r) + 1) ** 3 <= (1 << log2T) for r in enc.res))}}

# ---- 1. the kernels alone ------------------------------------------------------------------------------------------------------------
kern = {}
keep = []
table_bytes = Lv * (1 << log2T) * F * 4
ws = torch.empty(lib.ctx_hashgrid_bwd_ws_bytes(Lv, F, log2T), dtype=torch.uint8, device=dev)
g_table = torch.empty_like(enc.table)
for tag, (o, d) in (("image", (ro, rd)), ("train", (ro_t, rd_t))):
    pts = grid.march(o, d, NEAR, FAR, STEP)[4]
    n = int(pts.shape[0])
    W = Lv * F
    emb = torch.empty(n, W, device=dev)
    g_emb = torch.randn(n, W, device=dev) * 1e-3
    keep.append((pts, emb, g_emb))
    ga = enc._grid_args()
    kern[f"hashgrid_fwd_{tag}"] = (lambda p=pts, e=emb, n=n: L.check(lib.ctx_hashgrid_fwd(L.ptr(p), n, L.ptr(enc.table), *ga, L.ptr(e), L.stream())),
                                   n * 12 + n * W * 4 + table_bytes, n)
    for name, stages, nbytes in (("zero", 1, 2 * table_bytes), ("accumulate", 2, n * 12 + 2 * n * W * 4 + 2 * 2 * table_bytes),
                                 ("convert", 4, 2 * table_bytes + table_bytes), ("whole", 7, None)):
        kern[f"hashgrid_bwd_{name}_{tag}"] = (lambda p=pts, g=g_emb, n=n, st=stages: L.check(lib.ctx_hashgrid_bwd(
            L.ptr(p), n, L.ptr(g), *ga, st, L.ptr(ws), L.ptr(g_table), L.stream())), nbytes, n)
    # the MLP's backward with and without the input gradient: the difference is k_uvmlp_grad_emb
    blob = mlp.packed()
    saved = torch.empty(lib.ctx_uvmlp_saved_bytes(n, mlp.D, mlp.W, mlp.input_ch), dtype=torch.uint8, device=dev)
    raw = torch.empty(n, 4, device=dev)
    L.check(lib.ctx_uvmlp_fwd_emb(L.ptr(g_emb), n, L.ptr(blob), mlp.D, mlp.W, mlp.input_ch, 4, 0, L.ptr(raw), L.ptr(saved), L.stream()))
    bws = torch.empty(lib.ctx_uvmlp_bwd_ws_bytes(n, mlp.D, mlp.W), dtype=torch.uint8, device=dev)
    layers = list(mlp.pts_linears) + [mlp.output_linear]
    gws, gbs = [torch.empty_like(l.weight) for l in layers], [torch.empty_like(l.bias) for l in layers]
    gwp = (C.c_void_p * len(gws))(*[L.ptr(g).value for g in gws])
    gbp = (C.c_void_p * len(gbs))(*[L.ptr(g).value for g in gbs])
    g_raw, ge = torch.randn(n, 4, device=dev), torch.empty(n, W, device=dev)
    keep.append((blob, saved, raw, bws, gws, gbs, gwp, gbp, g_raw, ge))
    for name, out in (("mlp_bwd_without_grad_emb", None), ("mlp_bwd_with_grad_emb", ge)):
        kern[f"{name}_{tag}"] = (lambda x=keep[-1], n=n, out=out: L.check(lib.ctx_uvmlp_bwd_emb(
            L.ptr(x[8]), n, L.ptr(x[0]), mlp.D, mlp.W, mlp.input_ch, 4, 0, L.ptr(x[1]), L.ptr(x[3]), x[6], x[7], L.ptr(out), L.stream())), None, n)
us = alternate([k[0] for k in kern.values()], 21, warm=3)
res["kernels"] = {name: {"us": u, "n": n, **({} if b is None else {"hbm_bytes": b, "floor_us_at_8TBps": round(b / 8e6, 2)})}
                  for (name, (_, b, n)), u in zip(kern.items(), us)}
for tag in ("image", "train"):
    k = res["kernels"]
    n = k[f"hashgrid_fwd_{tag}"]["n"]
    adds = n * Lv * 8 * F
    k[f"hashgrid_bwd_accumulate_{tag}"]["int64_adds"] = adds
    k[f"hashgrid_bwd_accumulate_{tag}"]["add_rate_GBps"] = round(adds * 8 / k[f"hashgrid_bwd_accumulate_{tag}"]["us"] / 1e3, 1)
    ge_us = round(k[f"mlp_bwd_with_grad_emb_{tag}"]["us"] - k[f"mlp_bwd_without_grad_emb_{tag}"]["us"], 1)
    b = 2 * n * mlp.W * 4 + n * Lv * F * 4
    k[f"grad_emb_{tag}"] = {"us": ge_us, "n": n, "hbm_bytes": b, "floor_us_at_8TBps": round(b / 8e6, 2)}
del keep, kern

# ---- 2. render_image and train_step, both fields ------------------------------------------------------------------------------------------
kw = dict(occupancy=grid, march=STEP)
names = list(fields)
us = alternate([(lambda f=f: vr.render_image(f, HW, HW, K, c2w, NEAR, FAR, 0, **kw)) for f in fields.values()], reps_render, warm=1)
n_img = int(grid.march(ro, rd, NEAR, FAR, STEP)[2].numel())
res["render"] = {"rays": R, "n": n_img, "repetitions": reps_render, **{f"{k}_us": u for k, u in zip(names, us)}}
opts = {k: torch.optim.Adam(f.parameters(), lr=5e-4) for k, f in fields.items()}
us = alternate([(lambda k=k: vr.train_step(fields[k], opts[k], ro_t, rd_t, target, NEAR, FAR, 0, **kw)) for k in names], reps_step, warm=3)
res["train_step"] = {"rays": RT, "repetitions": reps_step, **{f"{k}_us": u for k, u in zip(names, us)}}

# ---- 3. the train_step by stage -----------------------------------------------------------------------------------------------------------------
stages = {}
for k, field in fields.items():
    acc = {s: [] for s in ("march", "field_fwd", "composite_fwd", "loss", "backward", "optimizer")}
    for rep in range(3 + reps_step):
        opts[k].zero_grad(set_to_none=True)
        a, lists = timed(lambda: grid.march(ro_t, rd_t, NEAR, FAR, STEP, perturb=True))
        ray_off, ray_id, tt, dt, pts = lists
        b, raw = timed(lambda: field.forward_pts(pts))
        c, out = timed(lambda: rnh.raw2outputs_packed(raw, tt, dt, rd_t, ray_off))
        d_, loss = timed(lambda: rnh.img2mse(out[0], target))
        e, _ = timed(lambda: loss.backward())
        f, _ = timed(lambda: opts[k].step())
        if rep >= 3:
            for s, v in zip(acc, (a, b, c, d_, e, f)):
                acc[s].append(v)
    stages[k] = {s: round(statistics.median(v), 1) for s, v in acc.items()}
    stages[k]["n"] = int(tt.numel())
res["train_step_stages_us"] = stages

# ---- 4. what a pass keeps alive between forward and backward ----------------------------------------------------------------------------------------
held = {}
for k, field in fields.items():
    (field.mlp if k == "hashgrid" else field)._saved_pool = None        # the pool the earlier sections left would hide the store
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    out = rnh.render_rays(field, ro_t, rd_t, NEAR, FAR, 0, perturb=1., white_bkgd=True, **kw)
    torch.cuda.synchronize()
    held[k] = int(torch.cuda.memory_allocated() - before)
    del out
res["train_step"]["held_bytes_after_forward"] = held
res["train_step"]["hashgrid_backward_scratch_bytes"] = int(ws.numel())

res["device"] = torch.cuda.get_device_name(0)
res["timer"] = "device events, median"
line = json.dumps(res)
print(line)
with open(os.path.join(ROOT, "profiles", "hashgrid_bench.jsonl"), "a") as f:
    f.write(line + "\n")
