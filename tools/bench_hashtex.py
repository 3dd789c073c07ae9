#!/usr/bin/env python3
"""What the texture field costs as a hash grid (guide.texture_field = 'hashgrid') beside the 8 x 256 MLP it can replace,
at the reference's sizes: spot with its own UVs, the seven SDS poses at 1200^2, a 1024^2 atlas; the whole atlas and the texels the cached
raster can read (optim.field_texels = 'active').  One process, device events, median of 21 after warm-up, the entries of a group in turn.

  1. texture_map, training forward and forward + backward, for both fields; the backward gets a gradient on the texture that is zero off
     the list, as texture_mapping's backward hands it over;
  2. the new path by stage: encode (ctx_hashtex_fwd), the MLP's training forward and backward on the `emb` seam, the head forward and
     backward, and the table's backward by stage: zero, accumulate with and without the pre-sum (CTX_HASHTEX_PRESUM), convert;
  3. every kernel beside the HBM bytes it must move and the time 8 TB/s would take.

Appends one JSON line to profiles/hashtex_bench.jsonl.  Usage: python tools/bench_hashtex.py [atlas = 1024] [repetitions = 21]"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from contexture_nerf_amd import _lib as L, config as CFG, kal
from contexture_nerf_amd.trainer import ConTEXTure

T = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 21
assert torch.cuda.is_available(), "bench_hashtex needs the GPU"
dev = torch.device("cuda:0")
lib = L.load()


def trainer(field):
    cfg = CFG.TrainConfig()
    cfg.guide.text = "a photo of a cow"
    cfg.guide.shape_path = "shapes/spot_triangulated.obj"
    cfg.guide.texture_resolution = T
    cfg.guide.texture_field = field
    return ConTEXTure(cfg, device=dev, diffusion=None)


tr_mlp, tr_hash = trainer('mlp'), trainer('hashgrid')
with torch.no_grad():                                                  # the raster the SDS loop caches: its seven poses
    views = tr_mlp.train_views
    gray = torch.tensor([0.5, 0.5, 0.5], device=dev)
    allv = tr_mlp.mesh_model.render(theta=[v['theta'] for v in views], phi=[tr_mlp._offset_phi(v['phi']) for v in views],
                                    radius=[float(v['radius']) for v in views], background=gray)
    rc = allv['render_cache']
    texels, _ = kal.active_texels(rc['uv_features'].contiguous(), rc['face_idx'].contiguous(), T)
    del allv, rc
n_active = int(texels.numel())
fields = {"mlp": tr_mlp.texture_mlp, "hashgrid": tr_hash.texture_mlp}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); out = fn(); b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3, out


def alternate(fns, warm=3):
    """Median microseconds of each of `fns`, run in turn so that all see the same clocks."""
    ts = [[] for _ in fns]
    for r in range(warm + reps):
        for k, fn in enumerate(fns):
            us, _ = timed(fn)
            if r >= warm:
                ts[k].append(us)
    return [round(statistics.median(x), 1) for x in ts]


def with_floor(us, nbytes):
    return {"us": us, "hbm_bytes": int(nbytes), "floor_us_at_8TBps": round(nbytes / 8e6, 2)}


res = {"metric": "texture field: hash grid (12 levels x 2 features, T = 2^18, MLP 2 x 64) beside the 8 x 256 Fourier MLP",
       "case": {"mesh": "spot_triangulated", "atlas": T, "render": 1200, "views": len(views), "n_active": n_active,
                "active_fraction": round(n_active / float(T * T), 4), "repetitions": reps}}
enc, mlp = fields["hashgrid"].encoding, fields["hashgrid"].mlp
Lv, F, log2T, Wd = enc.n_levels, enc.n_features, enc.log2_table, enc.out_dim
res["case"].update(levels=Lv, features=F, log2_table=log2T, res=enc.res.tolist(),
                   dense_levels=[bool((int(r) + 1) ** 2 <= (1 << log2T)) for r in enc.res])
table_bytes = Lv * (1 << log2T) * F * 4

# ---- 1. texture_map of both fields ----------------------------------------------------------------------------------------------
g_tex = {"all": torch.randn(1, 3, T, T, device=dev) * 1e-3}
g_tex["active"] = torch.zeros(1, 3, T, T, device=dev)
g_tex["active"].view(3, -1)[:, texels.long()] = g_tex["all"].view(3, -1)[:, texels.long()]
tm = {}
for mode, tl in (("all", None), ("active", texels)):
    def fwd(name, tl=tl):
        return fields[name].texture_map(T, texels=tl)

    def fwd_bwd(name, tl=tl, g=g_tex[mode]):
        for p in fields[name].parameters():
            p.grad = None
        tex, _ = fields[name].texture_map(T, texels=tl)
        tex.backward(g)

    us = alternate([lambda: fwd_bwd("mlp"), lambda: fwd_bwd("hashgrid")])
    tm[mode] = {"rows": T * T if tl is None else n_active, "fwd_bwd_us": {"mlp": us[0], "hashgrid": us[1]}}
    with torch.no_grad():
        for f in fields.values():
            f._tex_cache = None
        us = alternate([lambda: (setattr(fields["mlp"], "_tex_cache", None), fwd("mlp")),
                        lambda: (setattr(fields["hashgrid"], "_tex_cache", None), fwd("hashgrid"))])
    tm[mode]["fwd_nograd_us"] = {"mlp": us[0], "hashgrid": us[1]}
res["texture_map"] = tm

# ---- 2. and 3. the new path by stage ----------------------------------------------------------------------------------------------
ga = enc._grid_args()
stages = {}
for mode, tl in (("all", None), ("active", texels)):
    n = T * T if tl is None else n_active
    idx_bytes = 0 if tl is None else n * 4
    emb = torch.empty(n, Wd, device=dev)
    g_emb = torch.randn(n, Wd, device=dev) * 1e-3
    g_table = torch.empty_like(enc.table)
    ws = torch.empty(lib.ctx_hashtex_bwd_ws_bytes(Lv, F, log2T), dtype=torch.uint8, device=dev)
    table = enc.table.detach()

    def encode():
        L.check(lib.ctx_hashtex_fwd(None, L.ptr(tl), n, T, L.ptr(table), *ga, L.ptr(emb), L.stream()))

    def bwd(stage, presum="1"):
        os.environ["CTX_HASHTEX_PRESUM"] = presum
        L.check(lib.ctx_hashtex_bwd(None, L.ptr(tl), n, T, L.ptr(g_emb), *ga, stage, L.ptr(ws), L.ptr(g_table), L.stream()))

    bwd(7, "1"); a = g_table.clone(); bwd(7, "0")
    assert torch.equal(a, g_table), "the pre-summed accumulate and the plain one differ"
    encode()
    emb_req = emb.clone().requires_grad_(True)
    raw = mlp.forward_features(emb).detach()
    g_raw = torch.randn_like(raw) * 1e-3
    tex = torch.empty(3, T * T, device=dev)
    g_rawo = torch.empty_like(raw)

    def mlp_fwd_bwd():
        for p in mlp.parameters():
            p.grad = None
        emb_req.grad = None
        mlp.forward_features(emb_req).backward(g_raw)

    def mlp_fwd():
        with torch.no_grad():
            mlp.forward_features(emb)

    def head_fwd():
        L.check(lib.ctx_texture_head_fwd(L.ptr(raw), L.ptr(tl), n, T * T, 3, L.ptr(tex), L.stream()))

    def head_bwd():
        L.check(lib.ctx_texture_head_bwd(L.ptr(g_tex[mode]), None, L.ptr(raw), L.ptr(tl), n, T * T, 3, L.ptr(g_rawo), L.stream()))

    bwd(1)
    us = alternate([encode, mlp_fwd, mlp_fwd_bwd, head_fwd, head_bwd, lambda: bwd(1), lambda: bwd(2, "1"), lambda: bwd(2, "0"), lambda: bwd(4)])
    del os.environ["CTX_HASHTEX_PRESUM"]
    terms = n * Lv * 4 * F
    stages[mode] = {
        "rows": n,
        "encode": with_floor(us[0], n * Wd * 4 + table_bytes + idx_bytes),
        "mlp_fwd_nograd": {"us": us[1]},
        "mlp_fwd_bwd_with_emb_grad": {"us": us[2]},
        "head_fwd": with_floor(us[3], n * 3 * 4 * 2 + idx_bytes),
        "head_bwd": with_floor(us[4], n * 3 * 4 * 3 + idx_bytes),
        "bwd_zero": with_floor(us[5], table_bytes * 2),
        "bwd_accumulate_presum": {**with_floor(us[6], 2 * n * Wd * 4 + table_bytes * 2 * 2 + 2 * idx_bytes), "terms": terms,
                                  "G_terms_per_s": round(terms / us[6] / 1e3, 2)},
        "bwd_accumulate_plain": {**with_floor(us[7], 2 * n * Wd * 4 + table_bytes * 2 * 2 + 2 * idx_bytes), "terms": terms,
                                 "G_terms_per_s": round(terms / us[7] / 1e3, 2)},
        "bwd_convert": with_floor(us[8], table_bytes * 3),
    }
    del emb, g_emb, g_table, ws, emb_req, raw, g_raw, tex, g_rawo
res["stages"] = stages
res["floors"] = ("encode: the emb rows out, the table once, the list; accumulate: g_emb twice (max, then terms), the int64 accumulator read "
                 "and written once, the list twice; zero: the accumulator; convert: the accumulator in, the float table out")
res["device"] = torch.cuda.get_device_name(0)
res["timer"] = "device events, median"
line = json.dumps(res)
print(line)
with open(os.path.join(ROOT, "profiles", "hashtex_bench.jsonl"), "a") as f:
    f.write(line + "\n")
