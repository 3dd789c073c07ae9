#!/usr/bin/env python3
"""Times ctx_atlas_fill (csrc/atlasfill.hip) at T = 1024 / 2048 / 4096 for three coverages: the spot case (seven poses at 1200^2
scattered with unit weights into the mesh's own UVs), a 1 %-random coverage, and the worst case of the row walk (one covered texel
in a corner, every texel a chart texel).  One JSON object per line, with the HBM floor of the bytes the call must move (read
coverage + chart + atlas, write filled + src) beside each time.  Usage: python tools/bench_atlas_fill.py [--sizes 1024,2048,4096]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from contexture_nerf_amd import kal, _lib as L
from contexture_nerf_amd.mesh import Mesh
from contexture_nerf_amd.render import Renderer
from contexture_nerf_amd.textured_mesh import uv_chart_mask

if not torch.cuda.is_available():
    raise SystemExit("bench_atlas_fill: needs the GPU (a CPU run cannot give a time)")
dev = torch.device('cuda:0')
lib = L.load()
HBM = 8000.0   # GB/s spec
C, PAD = 3, 8


def timeit(fn, iters):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def spot_case(T):
    mesh = Mesh(os.path.join(ROOT, 'shapes', 'spot_triangulated.obj'), dev).normalize_mesh(inplace=True, target_scale=0.6, dy=0.25)
    B, H = 7, 1200
    theta = torch.deg2rad(torch.tensor([60., 60, 60, 60, 110, 110, 110], device=dev))
    phi = torch.deg2rad(torch.tensor([0., 30, 150, 270, 90, 210, 330], device=dev))
    ren = Renderer(dev, dim=(H, H), interpolation_mode='bilinear')
    cam = ren.get_camera_from_multiple_view(theta, phi, torch.full((B,), 1.5, device=dev), 0.25)
    fvc, fvi, _ = kal.render.mesh.prepare_vertices(mesh.vertices[None].repeat(B, 1, 1), mesh.faces, ren.camera_projection, camera_transform=cam)
    face_uv = kal.ops.mesh.index_vertices_by_faces(mesh.vt.to(dev).unsqueeze(0), mesh.ft.to(dev).long())
    uv, idx = kal.render.mesh.rasterize(H, H, fvc[..., 2], fvi, face_uv.expand(B, -1, -1, -1).contiguous())
    acc = torch.zeros(1, T, T, dtype=torch.int64, device=dev)
    kal.scatter_fixed(torch.ones(B, H, H, 1, device=dev), uv.contiguous(), idx.contiguous(), acc)
    return kal.fixed_to_float(acc)[0].contiguous(), uv_chart_mask(face_uv, T)


def cases(T):
    g = torch.Generator().manual_seed(T)
    yield "spot (7 views @1200^2, own UVs)", *spot_case(T)
    cov = (torch.rand(T, T, generator=g) < 0.01).float().to(dev)
    chart = torch.ones(T, T, dtype=torch.uint8, device=dev)
    yield "random 1 % coverage, every texel in a chart", cov, chart
    one = torch.zeros(T, T, device=dev); one[T - 1, 0] = 1.0
    yield "one covered texel in a corner (worst case of the row walk: T LDS reads per texel)", one, chart


sizes = [1024, 2048, 4096]
for i, a in enumerate(sys.argv):
    if a == '--sizes':
        sizes = [int(s) for s in sys.argv[i + 1].split(',')]
for T in sizes:
    atlas = torch.rand(C, T, T, device=dev)
    ws = torch.empty(lib.ctx_atlas_fill_ws_bytes(T), dtype=torch.uint8, device=dev)
    filled = torch.empty_like(atlas)
    src = torch.empty(T, T, dtype=torch.int32, device=dev)
    for name, cov, chart in cases(T):
        call = lambda: L.check(lib.ctx_atlas_fill(L.ptr(atlas), L.ptr(cov), L.ptr(chart), C, T, PAD, L.ptr(filled), L.ptr(src), L.ptr(ws), ws.numel(), L.stream()))
        worst = name.startswith("one covered")
        sec = timeit(call, 3 if worst else 20)
        covered = cov > 0
        inchart = chart > 0
        bytes_ = T * T * (4 + 1 + C * 4 + C * 4 + 4)
        print(json.dumps({"kernel": "ctx_atlas_fill", "T": T, "C": C, "pad": PAD, "coverage": name, "us": round(sec * 1e6, 1),
                          "algorithmic_MB": round(bytes_ / 1e6, 2), "hbm_floor_us_8TBs": round(bytes_ / (HBM * 1e9) * 1e6, 2),
                          "frac_of_hbm_floor": round(bytes_ / (HBM * 1e9) / sec, 4),
                          "chart_texels": int(inchart.sum()), "stage_A_fills": int((inchart & ~covered).sum()),
                          "stage_B_fills": int(((src >= 0) & ~(inchart | covered)).sum())}), flush=True)
