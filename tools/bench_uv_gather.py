#!/usr/bin/env python3
"""Times the texel-side gather (ctx_uv_gather_fixed, csrc/uvgather.hip; the seen pass included) against the forward scatter
(kal.scatter_fixed with a kept plan and with the plan rebuilt every call) on the spot case: seven poses at 1200^2, C = 3 colours +
weight, T = 1024 / 2048 / 4096.  The three run in the same process, alternating, each call between two device events; the figure is
the median after warm-up.  Beside each time: the bytes the call must move (computed here from the shapes and the raster) and
their HBM floor at 8 TB/s.  Beyond the plan's limit (T > ctx_texmap_plan_max_res) both scatter lines are the plan-less kernel.
One JSON object per line, appended to profiles/uv_gather_bench.jsonl.
Usage: python tools/bench_uv_gather.py [--sizes 1024,2048,4096] [--reps 30]"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from contexture_nerf_amd import kal, _lib as L
from contexture_nerf_amd.mesh import Mesh
from contexture_nerf_amd.render import Renderer
from contexture_nerf_amd.textured_mesh import uv_texel_map

if not torch.cuda.is_available():
    raise SystemExit("bench_uv_gather: needs the GPU (a CPU run cannot give a time)")
dev = torch.device('cuda:0')
lib = L.load()
HBM = 8000.0   # GB/s spec
B, H, C = 7, 1200, 3
OUT = os.path.join(ROOT, 'profiles', 'uv_gather_bench.jsonl')

sizes, reps = [1024, 2048, 4096], 30
for i, a in enumerate(sys.argv):
    if a == '--sizes':
        sizes = [int(s) for s in sys.argv[i + 1].split(',')]
    if a == '--reps':
        reps = int(sys.argv[i + 1])

mesh = Mesh(os.path.join(ROOT, 'shapes', 'spot_triangulated.obj'), dev).normalize_mesh(inplace=True, target_scale=0.6, dy=0.25)
theta = torch.deg2rad(torch.tensor([60., 60, 60, 60, 110, 110, 110], device=dev))
phi = torch.deg2rad(torch.tensor([0., 30, 150, 270, 90, 210, 330], device=dev))
ren = Renderer(dev, dim=(H, H), interpolation_mode='bilinear')
cam = ren.get_camera_from_multiple_view(theta, phi, torch.full((B,), 1.5, device=dev), 0.25)
fvc, fvi, _ = kal.render.mesh.prepare_vertices(mesh.vertices[None].repeat(B, 1, 1), mesh.faces, ren.camera_projection, camera_transform=cam)
face_uv = kal.ops.mesh.index_vertices_by_faces(mesh.vt.to(dev).unsqueeze(0), mesh.ft.to(dev).long())
uv, idx = kal.render.mesh.rasterize(H, H, fvc[..., 2], fvi, face_uv.expand(B, -1, -1, -1).contiguous())
uv, idx, fvi, faces = uv.contiguous(), idx.contiguous(), fvi.contiguous(), mesh.faces.contiguous()
F = faces.shape[0]
g = torch.Generator().manual_seed(7)
rgb = torch.rand(B, H, H, C, generator=g).to(dev)
w = torch.rand(B, H, H, generator=g).to(dev)
go = torch.cat([rgb * w[..., None], w[..., None]], -1).contiguous()          # what project_back_scatter hands the scatter
n_pix, n_fg = B * H * H, int((idx >= 0).sum())


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3                                          # us


for T in sizes:
    tface, tbary = uv_texel_map(face_uv, T)
    chart = int((tface >= 0).sum())
    ws = torch.empty(lib.ctx_uv_gather_ws_bytes(B, F), dtype=torch.uint8, device=dev)
    acc_g = torch.zeros(C + 1, T, T, dtype=torch.int64, device=dev)
    acc_s = torch.zeros(C + 1, T, T, dtype=torch.int64, device=dev)
    p = (L.ptr(rgb), L.ptr(w), L.ptr(idx), L.ptr(fvi), L.ptr(faces), L.ptr(tface), L.ptr(tbary))
    calls = {
        "gather (seen pass + k_uv_gather)": lambda: L.check(lib.ctx_uv_gather_fixed(*p, B, H, H, C, F, T, kal.SCATTER_FRAC_BITS, L.ptr(acc_g), L.ptr(ws),
                                                                                    ws.numel(), L.stream())),
        "scatter, kept plan": lambda: kal.scatter_fixed(go, uv, idx, acc_s, reuse=True),
        "scatter, plan rebuilt": lambda: kal.scatter_fixed(go, uv, idx, acc_s, reuse=False),
    }
    kal.clear_scatter_plans()
    for fn in calls.values():                                                 # the coverage of one call each, then warm-up
        fn()
    torch.cuda.synchronize()
    g_cov, s_cov = acc_g[C] > 0, acc_s[C] > 0
    in_chart = tface >= 0
    stats = dict(chart_texels=chart, gather_empty=int((in_chart & ~g_cov).sum()), scatter_empty=int((in_chart & ~s_cov).sum()),
                 gather_outside_chart=int((g_cov & ~in_chart).sum()), scatter_outside_chart=int((s_cov & ~in_chart).sum()))
    touched_s = int(s_cov.sum())
    # bytes a call must move: the gather reads face_idx once for the seen pass, the owners / colours / weights of the foreground, the
    # texel map, and reads and writes acc on the chart; the scatter reads (go, uv, face_idx) of every pixel and reads and writes acc where it lands
    bytes_ = {
        "gather (seen pass + k_uv_gather)": n_pix * 8 + n_fg * (8 + C * 4 + 4) + B * F * (24 + 2) + T * T * (8 + 12) + chart * (C + 1) * 16,
        "scatter, kept plan": n_pix * 8 + n_fg * ((C + 1) * 4 + 8 + 4) + touched_s * (C + 1) * 16,
        "scatter, plan rebuilt": n_pix * 8 * 3 + n_fg * ((C + 1) * 4 + 8 * 3 + 4 * 2) + touched_s * (C + 1) * 16,
    }
    for _ in range(5):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(reps):                                                     # alternating: the three share whatever the host is doing
        for k, fn in calls.items():
            times[k].append(timed(fn))
    planned = kal.binned_fits(C + 1, T)
    with open(OUT, 'a') as fh:
        for k in calls:
            us = statistics.median(times[k])
            line = {"tool": "bench_uv_gather", "case": "spot, 7 views @1200^2, C=3 + weight", "T": T, "path": k,
                    "scatter_kernel": ("binned (plan)" if planned else "plan-less (int64 atomics)") if k.startswith("scatter") else None,
                    "us_median": round(us, 1), "us_min": round(min(times[k]), 1), "us_max": round(max(times[k]), 1), "reps": reps,
                    "must_move_MB": round(bytes_[k] / 1e6, 2), "hbm_floor_us_8TBs": round(bytes_[k] / (HBM * 1e9) * 1e6, 2),
                    "frac_of_hbm_floor": round(bytes_[k] / (HBM * 1e9) / (us * 1e-6), 4), **stats}
            print(json.dumps(line), flush=True)
            fh.write(json.dumps(line) + "\n")
