#!/usr/bin/env python3
"""What the hash-grid field's gradient to the positions costs, on the scene of tools/bench_hashgrid.py (spot, G 128,
dilate 1, march = h; 16 levels x 2 features, T = 2^19, MLP 2 x 64) in one process, at the marched points of the HW^2 image and of 4096
training rays:

  1. ctx_hashgrid_bwd_pts in its two mappings, each forced (CTX_HASHGRID_PTS_LOOP=0: one thread per (point, level) with the scratch and
     the level sum, the default below 2^17 points; =1: one thread per point walking the levels, the default from there on) beside
     ctx_hashgrid_fwd, which issues the same gathers, in the same run, and beside the HBM bytes each must move (points, g_emb rows, the
     table once, g_pts, the scratch written and read) and the time 8 TB/s would take;
  2. the MLP's backward for the input gradient with and without its weight-gradient launches (ctx_uvmlp_bwd_emb with gws / gbs null);
  3. HashGridField.density_gradient beside forward_pts;
  4. ctx_weighted_sum_packed (C = 3) beside its byte floor;
  5. render_normals beside render_image at HW^2.

Device events, median of 21 after warm-up, the entries of a group run in turn.  Appends one JSON line to profiles/hashgrid_grad_bench.jsonl.
Usage: python tools/bench_hashgrid_grad.py [HW = 512] [render repetitions = 5]"""
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
assert torch.cuda.is_available(), "bench_hashgrid_grad needs the GPU"
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
field = HashGridField.from_grid(grid).to(dev)
with torch.no_grad():
    field.mlp.output_linear.bias[3] = 1.0
enc, mlp = field.encoding, field.mlp
Lv, F, log2T = enc.n_levels, enc.n_features, enc.log2_table
K = vr.pinhole(HW, HW)
c2w = torch.tensor([[1., 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1.5]], device=dev)
ro, rd = rnh.get_rays(HW, HW, K, c2w)
ro, rd = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()
R = ro.shape[0]
pick = torch.randint(0, R, (RT,), device=dev)
ro_t, rd_t = ro[pick].contiguous(), rd[pick].contiguous()


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


def with_floor(us, n, nbytes):
    return {"us": us, "n": n, "hbm_bytes": nbytes, "floor_us_at_8TBps": round(nbytes / 8e6, 2)}


res = {"metric": "hash-grid field: the gradient to the positions, density_gradient and render_normals (16 levels x 2 features, T = 2^19, MLP 2 x 64)",
       "case": {"mesh": "spot_triangulated", "G": G0, "dilate": 1, "march": STEP, "near_far": [NEAR, FAR], "image": HW, "train_rays": RT,
                "levels": Lv, "features": F, "log2_table": log2T, "res": enc.res.tolist()}}
table_bytes = Lv * (1 << log2T) * F * 4
Wd = Lv * F
ga = enc._grid_args()
kern, dens, wsum = {}, {}, {}
for tag, (o, d) in (("image", (ro, rd)), ("train", (ro_t, rd_t))):
    ray_off, ray_id, t, dt, pts = grid.march(o, d, NEAR, FAR, STEP)
    n = int(pts.shape[0])
    emb = torch.empty(n, Wd, device=dev)
    g_emb = torch.randn(n, Wd, device=dev) * 1e-3
    g_pts = torch.empty(n, 3, device=dev)
    ws = torch.empty(lib.ctx_hashgrid_bwd_pts_ws_bytes(n, Lv), dtype=torch.uint8, device=dev)

    def fwd(p=pts, e=emb, n=n):
        L.check(lib.ctx_hashgrid_fwd(L.ptr(p), n, L.ptr(enc.table), *ga, L.ptr(e), L.stream()))

    def bwd_pts(loop, p=pts, g=g_emb, n=n, w=ws, out=g_pts):
        os.environ["CTX_HASHGRID_PTS_LOOP"] = "1" if loop else "0"
        L.check(lib.ctx_hashgrid_bwd_pts(L.ptr(p), n, L.ptr(enc.table), L.ptr(g), *ga, L.ptr(w), L.ptr(out), L.stream()))

    # both mappings give the same bits before they are timed
    bwd_pts(False); a = g_pts.clone(); bwd_pts(True)
    assert torch.equal(a, g_pts), "the two mappings of ctx_hashgrid_bwd_pts differ"
    base = n * 12 + n * Wd * 4 + table_bytes
    us = alternate([fwd, lambda: bwd_pts(False), lambda: bwd_pts(True)], 21)
    kern[f"hashgrid_fwd_{tag}"] = with_floor(us[0], n, base)
    kern[f"hashgrid_bwd_pts_{tag}"] = with_floor(us[1], n, base + n * 12 + 2 * Lv * n * 12 + n * 12)     # + g_pts, the scratch out and in, pts again
    kern[f"hashgrid_bwd_pts_loop_{tag}"] = with_floor(us[2], n, base + n * 12)
    del os.environ["CTX_HASHGRID_PTS_LOOP"]                            # from here on the mapping the library picks by n

    # the MLP's backward for the input gradient, with and without the weight-gradient launches
    blob = mlp.packed()
    saved = torch.empty(lib.ctx_uvmlp_saved_bytes(n, mlp.D, mlp.W, mlp.input_ch), dtype=torch.uint8, device=dev)
    raw = torch.empty(n, 4, device=dev)
    L.check(lib.ctx_uvmlp_fwd_emb(L.ptr(g_emb), n, L.ptr(blob), mlp.D, mlp.W, mlp.input_ch, 4, 0, L.ptr(raw), L.ptr(saved), L.stream()))
    bws = torch.empty(lib.ctx_uvmlp_bwd_ws_bytes(n, mlp.D, mlp.W), dtype=torch.uint8, device=dev)
    layers = list(mlp.pts_linears) + [mlp.output_linear]
    gws, gbs = [torch.empty_like(l.weight) for l in layers], [torch.empty_like(l.bias) for l in layers]
    gwp = (C.c_void_p * len(gws))(*[L.ptr(g).value for g in gws])
    gbp = (C.c_void_p * len(gbs))(*[L.ptr(g).value for g in gbs])
    g_raw = torch.randn(n, 4, device=dev)
    ge = [torch.empty(n, Wd, device=dev) for _ in range(2)]

    def mlp_bwd(k, wp, bp, n=n, blob=blob, saved=saved, bws=bws, g_raw=g_raw, ge=ge):
        L.check(lib.ctx_uvmlp_bwd_emb(L.ptr(g_raw), n, L.ptr(blob), mlp.D, mlp.W, mlp.input_ch, 4, 0, L.ptr(saved), L.ptr(bws), wp, bp,
                                      L.ptr(ge[k]), L.stream()))

    us = alternate([lambda: mlp_bwd(0, gwp, gbp), lambda: mlp_bwd(1, None, None)], 21)
    assert torch.equal(ge[0], ge[1]), "grad_emb moved when the weight gradients were skipped"
    kern[f"mlp_bwd_emb_with_weight_grads_{tag}"] = {"us": us[0], "n": n}
    kern[f"mlp_bwd_emb_input_grad_only_{tag}"] = {"us": us[1], "n": n}

    us = alternate([lambda p=pts: field.forward_pts(p), lambda p=pts: field.density_gradient(p, return_raw=True)], 21)
    dens[tag] = {"n": n, "forward_pts_us": us[0], "density_gradient_us": us[1]}

    w = torch.rand(n, device=dev)
    v = torch.randn(n, 3, device=dev)
    Rr = o.shape[0]
    us = alternate([lambda w=w, v=v, ro_=ray_off: rnh.weighted_sum_packed(w, v, ro_)], 21)
    wsum[tag] = {"rays": Rr, **with_floor(us[0], n, n * 4 + n * 12 + (Rr + 1) * 8 + Rr * 12)}
    del emb, g_emb, g_pts, ws, saved, bws, ge, w, v
res["kernels"] = kern
res["density_gradient"] = dens
res["weighted_sum_packed_C3"] = wsum

with torch.no_grad():
    kw = dict(occupancy=grid, march=STEP)
    us = alternate([lambda: vr.render_image(field, HW, HW, K, c2w, NEAR, FAR, 0, **kw),
                    lambda: vr.render_normals(field, HW, HW, K, c2w, NEAR, FAR, **kw)], reps_render, warm=1)
res["render"] = {"rays": R, "n": kern["hashgrid_fwd_image"]["n"], "repetitions": reps_render, "render_image_us": us[0], "render_normals_us": us[1]}

res["device"] = torch.cuda.get_device_name(0)
res["timer"] = "device events, median"
line = json.dumps(res)
print(line)
with open(os.path.join(ROOT, "profiles", "hashgrid_grad_bench.jsonl"), "a") as f:
    f.write(line + "\n")
