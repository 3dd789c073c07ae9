#!/usr/bin/env python3
"""What the mip-mapped lookup (guide.texture_interpolation_mode = 'mipmap') costs beside the bilinear one it replaces, at
the reference's sizes: spot with its own UVs, the seven SDS poses, a 1024^2 atlas, 4 levels; the raster at 1200^2 (the SDS loop's) and at
320^2 (a small render).  One process, device events, median of 21 after warm-up, the entries of a group in turn.

  build     ctx_mip_build with the chart mask as coverage (levels 1 .. L-1 and the counts)
  lod       ctx_face_uv_lod (the table of a raster; the product keeps it in the render cache)
  forward   ctx_texture_mapping_mip_fwd beside the bilinear forward (kal.texture_mapping, which packs the atlas and gathers 16 bytes per tap)
  backward  ctx_texture_mapping_mip_bwd with and without the pre-sum (CTX_TEXMIP_PRESUM) beside the binned bilinear backward on the same
            raster with its plan cached (kal.scatter_add_texture)

The mip lod of the 1200^2 raster is taken twice: as the raster gives it (mostly magnified against a 1024^2 atlas: lod 0) and with the SDS
loop's footprint scale of the 320^2 tile (1200 / 320), where the coarse levels are read.
Appends one JSON line to profiles/mipmap_bench.jsonl.  Usage: python tools/bench_mipmap.py [atlas = 1024] [levels = 4] [repetitions = 21]"""
import json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from contexture_nerf_amd import _lib as L, config as CFG, kal
from contexture_nerf_amd.trainer import ConTEXTure

T = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
LV = int(sys.argv[2]) if len(sys.argv) > 2 else 4
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 21
assert torch.cuda.is_available(), "bench_mipmap needs the GPU"
dev = torch.device("cuda:0")
lib = L.load()
C = 3

cfg = CFG.TrainConfig()
cfg.guide.text = "a photo of a cow"
cfg.guide.shape_path = "shapes/spot_triangulated.obj"
cfg.guide.texture_resolution = T
tr = ConTEXTure(cfg, device=dev, diffusion=None)
views = tr.train_views
mm = tr.mesh_model
coverage = mm.chart_mask().contiguous()
tex = torch.rand(1, C, T, T, device=dev)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def alternate(fns, warm=3):
    """Median microseconds of each of `fns`, run in turn so that all see the same clocks."""
    ts = [[] for _ in fns]
    for r in range(warm + reps):
        for k, fn in enumerate(fns):
            us = timed(fn)
            if r >= warm:
                ts[k].append(us)
    return [round(statistics.median(x), 1) for x in ts]


res = {"metric": "texture_mapping: the mip-mapped lookup and its backward beside the bilinear ones",
       "case": {"mesh": "spot_triangulated", "atlas": T, "levels": LV, "channels": C, "views": len(views), "repetitions": reps,
                "chart_fraction": round(float(coverage.float().mean()), 4)}}
try:
    res["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
except Exception:
    res["commit"] = None

pyr = torch.empty(lib.ctx_mip_levels_bytes(C, T, LV), dtype=torch.uint8, device=dev)
cc = torch.empty(lib.ctx_mip_cov_bytes(T, LV), dtype=torch.uint8, device=dev)
tex_c = tex[0].contiguous()


def build():
    L.check(lib.ctx_mip_build(L.ptr(tex_c), L.ptr(coverage), C, T, LV, L.ptr(pyr), L.ptr(cc), L.stream()))


build()
res["build_us"] = alternate([build])[0]

for G in (1200, 320):
    with torch.no_grad():
        allv = mm.render(theta=[v['theta'] for v in views], phi=[tr._offset_phi(v['phi']) for v in views],
                         radius=[float(v['radius']) for v in views], background=torch.tensor([0.5, 0.5, 0.5], device=dev), dims=(G, G))
    rc = allv['render_cache']
    uv, fi, fvi = rc['uv_features'].contiguous(), rc['face_idx'].contiguous(), rc['face_vertices_image'].contiguous()
    del allv
    B, HW, F = uv.shape[0], G * G, fvi.shape[1]
    out = torch.empty(B, G, G, C, device=dev)
    go = torch.randn(B, G, G, C, device=dev) * 1e-3
    g_mip = torch.empty(C, T, T, device=dev)
    g_bil = torch.zeros(C, T, T, device=dev)
    ws = torch.empty(lib.ctx_texture_mapping_mip_bwd_ws_bytes(C, T, LV), dtype=torch.uint8, device=dev)
    tex_b = tex.expand(B, -1, -1, -1)
    entry = {"pixels": B * HW, "foreground": int((fi >= 0).sum())}
    scales = {"raster": None}
    if G == 1200:
        scales["tile_320"] = [1.0] + [1200.0 / 320.0] * (B - 1)
    lod = None

    def lod_fn(scale=None):
        global lod
        lod = kal.face_uv_lod(fvi, mm.face_attributes, G, G, T, LV, scale=scale)

    def bil_fwd():
        with torch.no_grad():
            kal.texture_mapping(uv, tex_b, mode='bilinear', mask_idx=fi)

    def mip_fwd():
        L.check(lib.ctx_texture_mapping_mip_fwd(L.ptr(uv), L.ptr(tex_c), L.ptr(pyr), L.ptr(lod), L.ptr(fi), B, HW, F, C, T, LV, L.ptr(out), L.stream()))

    def bil_bwd():
        kal.scatter_add_texture(go, uv, fi, g_bil, reuse=True)

    def mip_bwd(presum):
        os.environ["CTX_TEXMIP_PRESUM"] = presum
        L.check(lib.ctx_texture_mapping_mip_bwd(L.ptr(go), L.ptr(uv), L.ptr(lod), L.ptr(fi), L.ptr(cc), B, HW, F, C, T, LV, L.ptr(ws), L.ptr(g_mip),
                                                L.stream()))

    for name, scale in scales.items():
        lod_fn(scale)
        fg_lod = lod.gather(1, fi.reshape(B, -1).clamp(min=0))[fi.reshape(B, -1) >= 0]
        e = {"lod_mean_over_foreground": round(float(fg_lod.mean()), 3), "lod_zero_fraction": round(float((fg_lod == 0).float().mean()), 3)}
        mip_bwd("1"); a = g_mip.clone(); mip_bwd("0")
        assert torch.equal(a, g_mip), "the pre-summed accumulate and the plain one differ"
        us = alternate([lambda: lod_fn(scale), bil_fwd, mip_fwd, bil_bwd, lambda: mip_bwd("1"), lambda: mip_bwd("0")])
        del os.environ["CTX_TEXMIP_PRESUM"]
        e.update(lod_us=us[0], fwd_us={"bilinear": us[1], "mipmap": us[2], "ratio": round(us[2] / us[1], 2)},
                 bwd_us={"bilinear_binned_cached_plan": us[3], "mipmap_presum": us[4], "mipmap_plain": us[5],
                         "ratio_presum": round(us[4] / us[3], 2), "ratio_plain": round(us[5] / us[3], 2)})
        entry[name] = e
    res[f"render_{G}"] = entry
    kal.clear_scatter_plans()
    del rc, uv, fi, fvi, out, go, g_mip, g_bil, ws

res["device"] = torch.cuda.get_device_name(0)
res["timer"] = "device events, median"
line = json.dumps(res)
print(line)
with open(os.path.join(ROOT, "profiles", "mipmap_bench.jsonl"), "a") as f:
    f.write(line + "\n")
