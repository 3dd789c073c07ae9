#!/usr/bin/env python3
"""Times kal.view_consistency (csrc/viewconsist.hip) on six spot views at 1200^2 — forward (with and without the kept seen-vertex
map) and forward + backward — against the same quantity written in plain torch on the same GPU (`torch_port`: the loops of
src/training/trainer.py:429-531 with the raster's rows, the yardstick).  Median of 50 timed calls after 10 warm-up calls, one pair
of device events per call.  One JSON object per line; `hbm_fraction` counts one colour read per pair and side plus face_idx and
faces once (what an ideal kernel must move) against 8 TB/s.  Usage: python tools/bench_view_consistency.py [--size 1200]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from contexture_nerf_amd import kal
from contexture_nerf_amd.mesh import Mesh
from contexture_nerf_amd.render import Renderer

if not torch.cuda.is_available():
    raise SystemExit("bench_view_consistency: needs the GPU (a CPU run cannot give a time)")
dev = torch.device('cuda:0')
HBM = 8000.0   # GB/s spec
WARMUP, CALLS = 10, 50


def median_ms(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def torch_port(views, faces, face_idx, fvi):
    """The reference's loops (vertex table, visibility by unique, per-pair boolean indexing and gathers) with rows = 'image'; pairs
    whose source pixel is outside the image are dropped, as the kernel drops them."""
    V, C, h, w = views.shape
    nv = int(faces.max()) + 1
    table = torch.full((V, nv, 2), -1, dtype=torch.long, device=views.device)
    flat = faces.flatten()
    scale = torch.tensor([w, h], device=views.device, dtype=torch.float32)
    for i in range(V):
        c = fvi[i].reshape(-1, 2)
        c01 = torch.stack([(c[:, 0] + 1) / 2, (1 - c[:, 1]) / 2], 1)
        table[i, flat] = (c01 * scale).long()[:, [1, 0]]
    vis = torch.zeros((nv, V), dtype=torch.bool, device=views.device)
    for j in range(V):
        u = torch.unique(face_idx[j])
        u = u[u != -1]
        if u.numel() > 0:
            vis[faces[u].flatten(), j] = True
    terms = []
    for j in range(V):
        for i in range(V):
            if i == j:
                continue
            valid = face_idx[i] != -1
            if not torch.any(valid):
                continue
            pv = faces[face_idx[i][valid]]
            st = vis[:, j][pv]
            has = torch.any(st, dim=1)
            if not torch.any(has):
                continue
            first = torch.argmax(st[has].int(), dim=1)
            rep = pv[has][torch.arange(first.numel(), device=views.device), first]
            yx = table[j, rep]
            loc = valid.nonzero(as_tuple=False)[has]
            inside = (yx[:, 0] >= 0) & (yx[:, 0] < h) & (yx[:, 1] >= 0) & (yx[:, 1] < w)
            yx, loc = yx[inside], loc[inside]
            d = 1 - torch.abs(views[i][:, loc[:, 0], loc[:, 1]] - views[j][:, yx[:, 0], yx[:, 1]]).sum(dim=0) / C
            terms.append(d[d >= 0])
    allv = torch.cat(terms) if terms else torch.zeros(0, device=views.device)
    return torch.mean(allv) if allv.numel() > 0 else torch.tensor(0.0, device=views.device)


H = 1200
for i, a in enumerate(sys.argv):
    if a == '--size':
        H = int(sys.argv[i + 1])
V, C = 6, 3
mesh = Mesh(os.path.join(ROOT, 'shapes', 'spot_triangulated.obj'), dev).normalize_mesh(inplace=True, target_scale=0.6, dy=0.25)
theta = torch.deg2rad(torch.tensor([60., 60, 60, 110, 110, 110], device=dev))
phi = torch.deg2rad(torch.tensor([30., 150, 270, 90, 210, 330], device=dev))
ren = Renderer(dev, dim=(H, H), interpolation_mode='bilinear')
cam = ren.get_camera_from_multiple_view(theta, phi, torch.full((V,), 1.5, device=dev), 0.25)
fvc, fvi, _ = kal.render.mesh.prepare_vertices(mesh.vertices[None].repeat(V, 1, 1), mesh.faces, ren.camera_projection, camera_transform=cam)
_, idx = kal.render.mesh.rasterize(H, H, fvc[..., 2], fvi, fvc[..., 2:3].contiguous())
faces, idx, fvi = mesh.faces.contiguous(), idx.contiguous(), fvi.contiguous()
nv = int(mesh.vertices.shape[0])
views = torch.rand(V, C, H, H, generator=torch.Generator().manual_seed(0)).to(dev)

mean, st = kal.view_consistency(views, faces, idx, fvi, stats=True, n_vertices=nv)
N, fg = int(st['pair_count'].sum()), int((idx >= 0).sum())
ref = torch_port(views, faces, idx, fvi)
bytes_fwd = N * 2 * C * 4 + V * H * H * 8 + fg * 3 * 8
bytes_bwd = bytes_fwd + V * C * H * H * (4 + 4 + 4)              # + sign_count zeroed and read, grad_views written
seen = st['seen']
gviews = views.clone().requires_grad_(True)


def fwd_bwd(fn):
    def run():
        gviews.grad = None
        fn(gviews).backward()
    return run


rows = [("hip forward", lambda: kal.view_consistency(views, faces, idx, fvi, n_vertices=nv), bytes_fwd),
        ("hip forward, seen map kept", lambda: kal.view_consistency(views, faces, idx, fvi, seen=seen), bytes_fwd),
        ("hip forward + backward, seen map kept", fwd_bwd(lambda v: kal.view_consistency(v, faces, idx, fvi, seen=seen)), bytes_fwd + bytes_bwd),
        ("torch forward", lambda: torch_port(views, faces, idx, fvi), bytes_fwd),
        ("torch forward + backward", fwd_bwd(lambda v: torch_port(v, faces, idx, fvi)), bytes_fwd + bytes_bwd)]
for name, fn, nbytes in rows:
    med, best = median_ms(fn)
    print(json.dumps({"bench": "view_consistency", "what": name, "views": V, "size": H, "C": C, "pairs": N, "foreground_pixels": fg,
                      "median_ms": round(med, 4), "min_ms": round(best, 4), "calls": CALLS, "warmup": WARMUP,
                      "algorithmic_MB": round(nbytes / 1e6, 2), "hbm_fraction": round(nbytes / (HBM * 1e9) / (med * 1e-3), 4),
                      "mean_hip": float(mean), "mean_torch": float(ref)}), flush=True)
