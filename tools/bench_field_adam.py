#!/usr/bin/env python3
"""What the optimizer stage of a training step costs with optim.FieldAdam (csrc/adam.hip) beside torch.optim.Adam, at the
operating points of DESIGN 4j (HashGridField, 16 x 2^19 x 2, the marched points of 4096 rays through spot's shell) and 4l (HashGridTexture,
12 x 2^18 x 2, here on the whole 1024^2 atlas), and on one table of log2_table = 22.  One process, device events, median, the variants of a
group in turn.

  1. the optimizer stage alone over the field's parameters, with the table's gradient of one real backward: torch.optim.Adam,
     torch.optim.Adam(fused=True) where torch offers it, FieldAdam dense, FieldAdam sparse, FieldAdam deferred (`ctx_table_adam` on the
     integer sums + `ctx_adam_multi` on the MLP); beside them the zero pass and the convert pass of the accumulator, which the deferred
     step removes: the comparison is zero + convert + torch.optim.Adam against the deferred step;
  2. the two kernels on the table alone against their byte floors: ctx_adam_multi 28 * count dense and 4 * count + 28 * touched sparse,
     ctx_table_adam 8 * count + 32 * touched;
  3. train_step whole, fit_views' optimizer='torch' against 'fused' (4j's point only).

Appends one JSON line to profiles/field_adam_bench.jsonl.  Usage: python tools/bench_field_adam.py [repetitions = 21]"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import copy
import numpy as np
import torch
from contexture_nerf_amd import _lib as L, optim, run_nerf_helpers as rnh, volume_render as vr
from contexture_nerf_amd.hashgrid import HashGridField, HashGridTexture

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 21
assert torch.cuda.is_available(), "bench_field_adam needs the GPU"
dev = torch.device('cuda:0')
lib = L.load()
torch.manual_seed(0)
G0, NEAR, FAR, RT, ATLAS = 128, 0.5, 2.5, 4096, 1024
LR, TABLE_LR, BETAS, EPS = 5e-4, 1e-2, (0.9, 0.99), 1e-15


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def alternate(fns, warm=3):
    """Median microseconds of each of `fns` = (prepare or None, run), in turn so that all see the same clocks; prepare is not timed."""
    ts = [[] for _ in fns]
    for r in range(warm + reps):
        for k, (prep, fn) in enumerate(fns):
            if prep is not None:
                prep()
            us = timed(fn)
            if r >= warm:
                ts[k].append(us)
    return [round(statistics.median(x), 1) for x in ts]


def with_floor(us, nbytes):
    return {"us": us, "hbm_bytes": int(nbytes), "floor_us_at_8TBps": round(nbytes / 8e6, 2), "x_floor": round(us / (nbytes / 8e6), 2)}


def optimizer_stage(field, rows_of, g_emb):
    """The optimizer stage of `field` (encoding + mlp) for the table gradient of the backward on `rows_of(enc)` with g_emb."""
    enc = field.encoding
    table = enc.table
    count = table.numel()
    enc._workspace(dev, True)
    rows = rows_of(enc)
    g_table = torch.empty_like(table)
    enc._bwd_launch(rows, g_emb, 7, g_table)
    touched = int(torch.count_nonzero(g_table))
    mlp_params = list(field.mlp.parameters())
    mlp_count = sum(p.numel() for p in mlp_params)
    out = {"table_entries": count, "touched": touched, "touched_fraction": round(touched / count, 4), "rows": rows[-1], "mlp_parameters": mlp_count}

    def variant(make):
        f = copy.deepcopy(field)
        f.encoding.table.grad = g_table
        for p in f.mlp.parameters():
            p.grad = torch.randn_like(p) * 1e-3
        groups = [dict(params=[f.encoding.table], lr=TABLE_LR), dict(params=list(f.mlp.parameters()), lr=LR)]
        return f, make(groups)
    runs, names = [], []
    _f0, o = variant(lambda g: torch.optim.Adam(g, betas=BETAS, eps=EPS))
    names.append("torch_adam"); runs.append((None, o.step))
    try:
        _f1, o1 = variant(lambda g: torch.optim.Adam(g, betas=BETAS, eps=EPS, fused=True))
        o1.step()
        names.append("torch_adam_fused"); runs.append((None, o1.step))
    except Exception as e:                                            # this torch build has no fused Adam for the device
        out["torch_adam_fused"] = f"not offered: {type(e).__name__}"
    _f2, o2 = variant(lambda g: optim.FieldAdam(g, betas=BETAS, eps=EPS))
    names.append("field_adam_dense"); runs.append((None, o2.step))

    def sparse_groups(g):
        g[0]['sparse'] = True
        return optim.FieldAdam(g, betas=BETAS, eps=EPS)
    _f3, o3 = variant(sparse_groups)
    names.append("field_adam_sparse"); runs.append((None, o3.step))
    # deferred: the sums are put back before every step (not timed: the accumulate is the same work with either optimizer)
    f4, _unused = variant(lambda g: None)
    f4.encoding.table.grad = None
    o4 = optim.FieldAdam([dict(params=[f4.encoding.table], lr=TABLE_LR, sparse=True), dict(params=list(f4.mlp.parameters()), lr=LR)],
                         betas=BETAS, eps=EPS, encodings=[f4.encoding])
    e4 = f4.encoding
    e4._workspace(dev, True).zero_()
    rows4 = rows_of(e4)

    def refill():
        e4._bwd_launch(rows4, g_emb, 2, None)
        e4._pending, e4._ws_clean = rows4, False
    names.append("field_adam_deferred"); runs.append((refill, o4.step))
    # the two passes over the accumulator that the deferred step removes
    names.append("zero_pass"); runs.append((None, lambda: enc._bwd_launch(rows, g_emb, 1, None)))
    g_scratch = torch.empty_like(g_table)
    names.append("convert_pass"); runs.append((None, lambda: enc._bwd_launch(rows, g_emb, 4, g_scratch)))
    us = dict(zip(names, alternate(runs)))
    o4.release()
    out["optimizer_stage_us"] = us
    parent = round(us["zero_pass"] + us["convert_pass"] + us["torch_adam"], 1)
    out["parent_zero_convert_torch_adam_us"] = parent
    out["deferred_speedup_over_parent"] = round(parent / us["field_adam_deferred"], 2)
    # the kernels on the table alone, beside their floors
    p, m, v = (torch.randn(count, device=dev) * 1e-2 for _ in range(3))
    v.abs_()
    g = g_table.reshape(-1)
    ws = enc._bwd_ws

    def multi(sparse):
        optim.adam_multi([p], [m], [v], [g], TABLE_LR, BETAS, EPS, 5, sparse)

    def table_step():
        L.check(lib.ctx_table_adam(L.ptr(p), L.ptr(m), L.ptr(v), count, L.ptr(ws), rows[-1], enc._corners,
                                   *optim.coefficients(TABLE_LR, BETAS, EPS, 5), 1, L.stream()))
    enc._bwd_launch(rows, g_emb, 1, None)
    ku = alternate([(None, lambda: multi(False)), (None, lambda: multi(True)), (lambda: enc._bwd_launch(rows, g_emb, 2, None), table_step)])
    out["kernels"] = {"adam_multi_dense": with_floor(ku[0], 28 * count), "adam_multi_sparse": with_floor(ku[1], 4 * count + 28 * touched),
                      "table_adam": with_floor(ku[2], 8 * count + 32 * touched)}
    return out


res = {"metric": "the optimizer stage: optim.FieldAdam (HIP) beside torch.optim.Adam; deferred = the table's step from the integer sums",
       "case": {"repetitions": reps, "lr": LR, "table_lr": TABLE_LR, "betas": BETAS, "eps": EPS}}

# ---- DESIGN 4j's operating point --------------------------------------------------------------------------------------------------------
m = np.load(os.path.join(ROOT, "shapes", "meshes.npz"))
verts = torch.tensor(m["spot_triangulated_v"], dtype=torch.float32, device=dev)
faces = torch.tensor(m["spot_triangulated_f"].astype(np.int64), device=dev)
verts = verts - verts.mean(dim=0)                                     # Mesh.normalize_mesh(target_scale=0.6, dy=0.25)
verts = verts / torch.max(torch.norm(verts, p=2, dim=1)) * 0.6
verts[:, 1] += 0.25
grid = vr.OccupancyGrid.from_mesh(verts.contiguous(), faces, G0, -1.0, 1.0, dilate=1)
STEP = float(grid.h[0])
K = vr.pinhole(512, 512)
c2w = torch.tensor([[1., 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1.5]], device=dev)
ro, rd = rnh.get_rays(512, 512, K, c2w)
ro, rd = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()
pick = torch.randint(0, ro.shape[0], (RT,), device=dev)
ro_t, rd_t = ro[pick].contiguous(), rd[pick].contiguous()
target = torch.rand(RT, 3, device=dev)
field = HashGridField.from_grid(grid).to(dev)
with torch.no_grad():
    field.mlp.output_linear.bias[3] = 1.0

# the table's gradient of one real training backward: the g_emb the MLP hands down, on the marched points
seen = {}


def _keep(mod, inp, out):
    seen["pts"] = inp[0].detach().reshape(-1, 3).contiguous()
    out.register_hook(lambda g: seen.update(g_emb=g.detach().contiguous()))


hook = field.encoding.register_forward_hook(_keep)
out, _extras = rnh.render_rays(field, ro_t, rd_t, NEAR, FAR, 0, white_bkgd=True, perturb=1., return_extras=True, occupancy=grid, march=STEP)
rnh.img2mse(out[0], target).backward()
hook.remove()
field.zero_grad(set_to_none=True)
pts3, g_emb3 = seen["pts"], seen["g_emb"].reshape(-1, field.encoding.out_dim).contiguous()
res["hashgrid_3d"] = {"point": "DESIGN 4j: 4096 rays, spot's shell at G = 128, marched at h", "Lv_F_log2T": [16, 2, 19],
                      **optimizer_stage(field, lambda enc: (pts3, pts3.shape[0]), g_emb3)}

# train_step whole, 'torch' against 'fused'
kw = dict(occupancy=grid, march=STEP)
fa, fb = copy.deepcopy(field), copy.deepcopy(field)
oa, ob = vr.field_optimizer(fa, LR, 'torch', TABLE_LR), vr.field_optimizer(fb, LR, 'fused', TABLE_LR)
try:
    us = alternate([(None, lambda: vr.train_step(fa, oa, ro_t, rd_t, target, NEAR, FAR, 0, **kw)),
                    (None, lambda: vr.train_step(fb, ob, ro_t, rd_t, target, NEAR, FAR, 0, **kw))])
finally:
    ob.release()
res["train_step"] = {"rays": RT, "n": int(pts3.shape[0]), "torch_us": us[0], "fused_us": us[1], "speedup": round(us[0] / us[1], 2)}
del fa, fb, oa, ob

# ---- one table of log2_table = 22 at the same points ------------------------------------------------------------------------------------
big = HashGridField.from_grid(grid, log2_table=22).to(dev)
res["hashgrid_3d_log2T_22"] = {"Lv_F_log2T": [16, 2, 22], **optimizer_stage(big, lambda enc: (pts3, pts3.shape[0]), g_emb3)}
del big
torch.cuda.empty_cache()

# ---- DESIGN 4l's field, on the whole atlas ------------------------------------------------------------------------------------------------
tex = HashGridTexture().to(dev)
g_emb2 = torch.randn(ATLAS * ATLAS, tex.encoding.out_dim, device=dev) * 1e-3
res["hashgrid_2d"] = {"point": f"DESIGN 4l's field on the whole {ATLAS}^2 atlas (every texel a row; g_emb synthetic)", "Lv_F_log2T": [12, 2, 18],
                      **optimizer_stage(tex, lambda enc: (None, None, ATLAS, ATLAS * ATLAS), g_emb2)}

res["floors"] = ("adam_multi dense: p, m, v read and written and g read, 28 bytes per element; sparse: g read, 28 bytes per touched element; "
                 "table_adam: the int64 sum read, 8 bytes per element, and per touched element p, m, v read and written and the sum zeroed")
res["device"] = torch.cuda.get_device_name(0)
res["timer"] = "device events, median"
line = json.dumps(res)
print(line)
with open(os.path.join(ROOT, "profiles", "field_adam_bench.jsonl"), "a") as f:
    f.write(line + "\n")
