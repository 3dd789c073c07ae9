#!/usr/bin/env python3
"""What optim.field_texels = 'active' buys at the reference's sizes: spot with its own UVs, the seven SDS poses at 1200^2, a 1024^2 atlas,
the reference's field (D 8, W 256).

  1. n_active and the fraction of the atlas the cached raster can read (kal.active_texels);
  2. the field's training forward and its backward, dense and on the list, alternating in one process: device events, median after
     warm-up; the backward gets the gradient texture_mapping's backward would hand it (zero off the list) in both cases;
  3. the saved-activation bytes of either;
  4. one SDS iteration (paint_zero123plus, random-init engines) with the switch off / on / off, timed as tools/bench_sds_loop.py does.

The yardstick is the dense path in the same process.  Appends one JSON line to profiles/field_texels_bench.jsonl.
Usage: python tools/bench_field_texels.py [iterations per loop run = 10] [timed field repetitions = 15]"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from contexture_nerf_amd import _lib as L, config as CFG
from contexture_nerf_amd.trainer import ConTEXTure
from contexture_nerf_amd.stable_diffusion_depth import StableDiffusion

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 10
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 15
dev = torch.device("cuda:0")
cfg = CFG.TrainConfig()
cfg.guide.text = "a photo of a cow"
cfg.guide.shape_path = "shapes/spot_triangulated.obj"
cfg.guide.guidance_scale = 10.0
cfg.guide.sd_image_size = 512
sd = StableDiffusion(dev)
tr = ConTEXTure(cfg, device=dev, diffusion=sd)
tr.text_z = sd.get_text_embeds([cfg.guide.text])
tr.init_zero123plus()
T = int(cfg.guide.texture_resolution)


def loop_ms(mode):
    """-> (mean, min) ms per iteration of one paint_zero123plus run with optim.field_texels = mode, and its set-up record."""
    cfg.optim.field_texels = mode
    stamps = []

    def on_it(rec):
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
    log = tr.paint_zero123plus(iterations=iters + 3, on_iteration=on_it)
    per = [(b - a) * 1e3 for a, b in zip(stamps[2:-1], stamps[3:])]       # the first iterations size the workspaces
    assert all(r['loss'] == r['loss'] for r in log)
    return round(sum(per) / len(per), 2), round(min(per), 2), tr._sds_setup


loop = {}
loop['all_first'] = loop_ms('all')[:2]
ms, mn, setup = loop_ms('active')
loop['active'] = (ms, mn)
texels, n_active, fraction = setup['render_cache']['active_texels'], setup['n_active'], setup['active_fraction']
loop['all_again'] = loop_ms('all')[:2]

# ---- the field alone ------------------------------------------------------------------------------------------------------------
net = tr.texture_mlp
params = list(net.parameters())
g_tex = torch.zeros(3, T * T, device=dev)
g_tex[:, texels.long()] = torch.randn(3, n_active, device=dev) * 1e-6          # the magnitude of a mean-reduced loss's gradient
g_tex = g_tex.reshape(1, 3, T, T)


def once(listed):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    tex, _ = net.texture_map(T, texels=texels) if listed else net.texture_map(T)
    e[1].record()
    torch.autograd.grad(tex, params, g_tex)
    e[2].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])


times = {False: [], True: []}
for r in range(reps + 3):
    for listed in (False, True):                                               # alternating, so that both see the same clocks
        t = once(listed)
        if r >= 3:
            times[listed].append(t)
med = lambda listed, k: round(statistics.median(t[k] for t in times[listed]), 3)
lib = L.load()
saved = lambda n: int(lib.ctx_uvmlp_saved_bytes(n, net.D, net.W, net.input_ch))
out = {"metric": "texture field on the texels the cached raster reads (optim.field_texels), dense path of the same process as yardstick",
       "case": {"mesh": "spot_triangulated (own UVs)", "views": len(tr.train_views), "render": cfg.render.train_grid_size, "atlas": T,
                "field": {"D": net.D, "W": net.W}},
       "n_active": n_active, "active_fraction": round(fraction, 4),
       "field_ms": {"fwd_train_dense": med(False, 0), "fwd_train_active": med(True, 0), "bwd_dense": med(False, 1), "bwd_active": med(True, 1),
                    "repetitions": reps, "timer": "device events, median"},
       "ratio": {"fwd_train": round(med(True, 0) / med(False, 0), 3), "bwd": round(med(True, 1) / med(False, 1), 3)},
       "saved_activation_bytes": {"dense": saved(T * T), "active": saved(n_active)},
       "sds_iteration_ms": {"all_first": loop['all_first'][0], "active": loop['active'][0], "all_again": loop['all_again'][0],
                            "min": {"all_first": loop['all_first'][1], "active": loop['active'][1], "all_again": loop['all_again'][1]},
                            "iterations_timed": iters, "timer": "host clock around synchronised iterations, mean"},
       "device": torch.cuda.get_device_name(0), "data": "synthetic (random-init engines)"}
line = json.dumps(out)
print(line)
with open(os.path.join(ROOT, "profiles", "field_texels_bench.jsonl"), "a") as f:
    f.write(line + "\n")
