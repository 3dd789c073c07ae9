#!/usr/bin/env python3
"""Ray path, training side: (a) the compositing backward alone at HW^2 rays x S samples (default 512^2 x 128), against its
algorithmic bytes per sample — read 16 (raw) + 4 (z) + 4 (g_weights) + 4 (noise, when given), write 16 — and, for the same
inputs, the compositing forward; (b) one train_step at 4096 rays x S samples through NeRF2D(63 -> 4, W 256), split into field
forward, compositing forward, compositing backward and field backward.  Device events, median after warm-up.
Usage: bench_volume_train.py [HW] [S] [iters]"""
import sys, os, json, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, importlib
rnh = importlib.import_module('contexture_nerf_amd.run_nerf_helpers')
vr = importlib.import_module('contexture_nerf_amd.volume_render')
L = importlib.import_module('contexture_nerf_amd._lib')

HW = int(sys.argv[1]) if len(sys.argv) > 1 else 512
S = int(sys.argv[2]) if len(sys.argv) > 2 else 128
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 21
assert torch.cuda.is_available(), "bench_volume_train needs the GPU"
dev = torch.device('cuda:0')
lib = L.load()
torch.manual_seed(0)


def median_us(fn, n=iters, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


# ---- (a) the compositing kernels alone ------------------------------------------------------------
R = HW * HW
raw = torch.randn(R, S, 4, device=dev) * 2
z = torch.sort(torch.rand(R, S, device=dev) * 4 + 2, -1).values
d = torch.randn(R, 3, device=dev)
noise = torch.randn(R, S, device=dev)
g = [torch.randn(R, 3, device=dev), torch.randn(R, device=dev), torch.randn(R, device=dev), torch.randn(R, S, device=dev),
     torch.randn(R, device=dev)]
grad = torch.empty_like(raw)
outs = [torch.empty(R, 3, device=dev), torch.empty(R, device=dev), torch.empty(R, device=dev), torch.empty(R, S, device=dev),
        torch.empty(R, device=dev)]


def bwd(nz):
    L.check(lib.ctx_raymarch_composite_bwd(L.ptr(raw), L.ptr(z), L.ptr(d), L.ptr(nz), R, S, 0, L.ptr(g[0]), L.ptr(g[1]), L.ptr(g[2]),
                                           L.ptr(g[3]), L.ptr(g[4]), L.ptr(grad), L.stream()))


def fwd():
    L.check(lib.ctx_raymarch_composite_fwd(L.ptr(raw), L.ptr(z), L.ptr(d), R, S, 0, *[L.ptr(o) for o in outs], L.stream()))


res = {"rays": R, "samples": S}
for name, nz, per_sample in (("composite_bwd", None, 40), ("composite_bwd_noise", noise, 44)):
    us = median_us(lambda: bwd(nz))
    nbytes = R * S * per_sample
    res[name + "_us"] = round(us, 1)
    res[name + "_TBps"] = round(nbytes / us / 1e6, 2)
    res[name + "_frac_of_8TBps"] = round(nbytes / us / 1e6 / 8.0, 3)
us = median_us(fwd)
fwd_bytes = R * S * 5 * 4 + R * 12 + R * 5 * 4 + R * S * 4            # as tools/bench_volume.py counts the forward
res["composite_fwd_us"] = round(us, 1)
res["composite_fwd_frac_of_8TBps"] = round(fwd_bytes / us / 1e6 / 8.0, 3)
del raw, z, d, noise, g, grad, outs

# ---- (b) one training step at 4096 rays -----------------------------------------------------------
Rt = 4096
field = rnh.NeRF2D(D=8, W=256, input_ch=63, output_ch=4, skips=[4]).to(dev)
with torch.no_grad():
    field.output_linear.bias[3] = 1.0
opt = torch.optim.Adam(field.parameters(), lr=5e-4)
ro = torch.zeros(Rt, 3, device=dev) + torch.tensor([0., 0., 1.5], device=dev)
rd = torch.nn.functional.normalize(torch.randn(Rt, 3, device=dev) * 0.3 + torch.tensor([0., 0., -1.], device=dev), dim=-1)
target = torch.rand(Rt, 3, device=dev)
res["train_step_rays"] = Rt
res["train_step_us"] = round(median_us(lambda: vr.train_step(field, opt, ro, rd, target, 0.5, 2.5, S), n=11), 1)

ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
parts = {k: [] for k in ("field_fwd_us", "composite_fwd_us", "composite_bwd_us", "field_bwd_us")}
t = torch.linspace(0., 1., S, device=dev)
zt = (0.5 * (1. - t) + 2.5 * t).expand(Rt, S).contiguous()
pts = ro[:, None, :] + rd[:, None, :] * zt[:, :, None]
for i in range(3 + 11):
    field.zero_grad(set_to_none=True)
    ev[0].record()
    raw_t = field.forward_pts(pts)
    ev[1].record()
    leaf = raw_t.detach().requires_grad_(True)                      # cut the graph so the two backwards can be timed apart
    rgb = rnh.raw2outputs(leaf, zt, rd)[0]
    ev[2].record()
    loss = rnh.img2mse(rgb, target)
    g_rgb, = torch.autograd.grad(loss, rgb)
    ev[3].record()
    rgb.backward(g_rgb)
    ev[4].record()
    raw_t.backward(leaf.grad)
    ev[5].record()
    ev[5].synchronize()
    if i >= 3:
        parts["field_fwd_us"].append(ev[0].elapsed_time(ev[1]) * 1e3)
        parts["composite_fwd_us"].append(ev[1].elapsed_time(ev[2]) * 1e3)
        parts["composite_bwd_us"].append(ev[3].elapsed_time(ev[4]) * 1e3)
        parts["field_bwd_us"].append(ev[4].elapsed_time(ev[5]) * 1e3)
for k, v in parts.items():
    res["train_step_" + k] = round(statistics.median(v), 1)
print(json.dumps(res))
