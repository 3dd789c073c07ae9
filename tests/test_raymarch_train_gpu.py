"""GPU: the compositing backward (`ctx_raymarch_composite_bwd`), the density-noise forward, the autograd route of raw2outputs,
render_rays' training options and the training step of the 3-D field.  Yardstick: float64 CPU autograd of the plain-torch
restatement in test_raymarch_train_cpu.py, from the same float32 inputs."""
import ctypes as C
import functools
import numpy as np
import pytest
import torch

import test_raymarch_train_cpu as RM

pytestmark = pytest.mark.gpu

BOUND = 2e-4          # per ray, of the ray's largest reference gradient: the forward compositing's tolerance against its oracle


@functools.lru_cache(maxsize=None)
def _reference(R, S, white, which, with_noise=False):
    raw, z, d, noise = RM.make_case(R, S, seed=R * 1000 + S, with_noise=with_noise)
    grads = RM.make_grads(R, S, which, seed=S)
    want = RM.autograd_grad(raw, z, d, noise, white, grads)
    f32 = RM.autograd_grad(raw, z, d, noise, white, grads, dtype=torch.float32)
    return raw, z, d, noise, grads, want, f32


def _hip_grad(dev, raw, z, d, white, grads, noise=None):
    """grad_raw through raw2outputs' autograd route; absent gradients stay absent (null pointers in the kernel)."""
    from contexture_nerf_amd import run_nerf_helpers as rnh
    x = raw.detach().to(dev).requires_grad_(True)
    if noise is None:
        outs = rnh.raw2outputs(x, z.to(dev), d.to(dev), white_bkgd=white)
    else:
        outs = rnh._CompositeFn.apply(x, z.to(dev), d.to(dev), noise.to(dev), white)
    assert all(o.grad_fn is not None for o in outs)
    pairs = [(o, g.to(dev)) for o, g in zip(outs, grads) if g is not None]
    torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
    return x.grad.cpu()


@pytest.mark.parametrize("R,S", RM.SHAPES)
def test_backward_vs_float64_autograd(dev, R, S):
    """Every shape, both backgrounds, three gradient sets, with the opaque / acc == 0 / exact-zero rays of make_case.  The
    acc == 0 ray's reference leaves the disparity term out (g_disp = 0) while the kernel is handed g_disp != 0 there: it has to
    drop it, which also makes that ray's gradient finite."""
    worst, worst32 = 0.0, 0.0
    for white in (False, True):
        for which in RM.GRAD_SETS:
            raw, z, d, _, grads, want, f32 = _reference(R, S, white, which)
            got = _hip_grad(dev, raw, z, d, white, grads)
            assert torch.isfinite(got).all(), (R, S, white, which)
            ratio = RM.worst_ratio(got, want)
            worst, worst32 = max(worst, ratio), max(worst32, RM.worst_ratio(f32, want))
            assert ratio <= BOUND, (R, S, white, which, ratio)
    print(f"composite_bwd (R,S)=({R},{S}): worst |got-want|/max|want| per ray {worst:.3e}; float32 CPU autograd {worst32:.3e}")


@pytest.mark.parametrize("R,S", [(4, 65), (5, 33), (1, 1)])
def test_relu_mask_and_last_sample(dev, R, S):
    """grad_raw.w is exactly 0 wherever raw.w + noise <= 0 and finite elsewhere, on the last sample (dist = 1e10) too."""
    raw, z, d, noise = RM.make_case(R, S, seed=7 * R + S, with_noise=True)
    raw[0, -1, 3], noise[0, -1] = -0.5, 0.25                     # last sample masked ...
    if R > 3:
        raw[3, -1, 3], noise[3, -1] = 0.5, 0.25                  # ... and not masked
    grads = RM.make_grads(R, S, 'all', seed=S)
    for nz in (None, noise):
        got = _hip_grad(dev, raw, z, d, True, grads, noise=nz)
        pre = raw[..., 3] if nz is None else raw[..., 3] + nz
        assert torch.isfinite(got).all()
        assert (got[..., 3][pre <= 0] == 0).all()
        if S > 1:
            assert (got[..., 3][pre > 0] != 0).any()


def _abi_fwd(dev, raw, z, d, white, noise=None, use_noise_entry=False):
    from contexture_nerf_amd import _lib as L
    lib = L.load()
    R, S, _ = raw.shape
    outs = [torch.empty(R, 3, device=dev), torch.empty(R, device=dev), torch.empty(R, device=dev), torch.empty(R, S, device=dev),
            torch.empty(R, device=dev)]
    p = [L.ptr(o) for o in outs]
    if use_noise_entry:
        L.check(lib.ctx_raymarch_composite_fwd_noise(L.ptr(raw), L.ptr(z), L.ptr(d), L.ptr(noise), R, S, int(white), *p, L.stream()))
    else:
        L.check(lib.ctx_raymarch_composite_fwd(L.ptr(raw), L.ptr(z), L.ptr(d), R, S, int(white), *p, L.stream()))
    return outs


def _same(a, b):
    return all(torch.equal(torch.nan_to_num(x, nan=-7.0), torch.nan_to_num(y, nan=-7.0)) for x, y in zip(a, b))


@pytest.mark.parametrize("R,S", [(37, 128), (6, 257)])
def test_bits(dev, R, S):
    from contexture_nerf_amd import _lib as L, run_nerf_helpers as rnh
    raw, z, d, noise = [t.to(dev) for t in RM.make_case(R, S, seed=R + S, with_noise=True)]
    grads = RM.make_grads(R, S, 'all', seed=S)
    # backward: run to run and on a side stream; every element written (the buffer starts as NaN)
    g = [t.to(dev) for t in grads]
    lib = L.load()

    def bwd(nz):
        out = torch.full((R, S, 4), float('nan'), device=dev)
        L.check(lib.ctx_raymarch_composite_bwd(L.ptr(raw), L.ptr(z), L.ptr(d), L.ptr(nz), R, S, 1, L.ptr(g[0]), L.ptr(g[1]), L.ptr(g[2]),
                                               L.ptr(g[3]), L.ptr(g[4]), L.ptr(out), L.stream()))
        return out
    for nz in (None, noise):
        a, b = bwd(nz), bwd(nz)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            c = bwd(nz)
        side.synchronize()
        assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(a, c)
    x = raw.clone().requires_grad_(True)
    outs = rnh.raw2outputs(x, z, d, white_bkgd=True)
    torch.autograd.backward(list(outs), g)
    assert torch.equal(x.grad, bwd(None))                        # the autograd route is this call
    # forward: today's call without grad, the noise entry with and without noise
    direct = _abi_fwd(dev, raw, z, d, True)
    with torch.no_grad():
        assert _same(rnh.raw2outputs(raw.clone().requires_grad_(True), z, d, white_bkgd=True), direct)
    plain = rnh.raw2outputs(raw, z, d, white_bkgd=True)
    assert all(o.grad_fn is None for o in plain) and _same(plain, direct)
    assert _same([o.detach() for o in outs], direct)
    assert _same(_abi_fwd(dev, raw, z, d, True, None, use_noise_entry=True), direct)
    shifted = raw.clone()
    shifted[..., 3] += noise
    assert _same(_abi_fwd(dev, raw, z, d, True, noise, use_noise_entry=True), _abi_fwd(dev, shifted, z, d, True))


def test_noise_and_jitter(dev):
    from contexture_nerf_amd import run_nerf_helpers as rnh
    R, S = 5, 33
    raw, z, d, _ = RM.make_case(R, S, seed=11)
    np.random.seed(0)
    noise = torch.tensor(np.random.rand(R, S) * 1.0, dtype=torch.float32)
    grads = RM.make_grads(R, S, 'all', seed=S)
    x = raw.to(dev).requires_grad_(True)
    outs = rnh.raw2outputs(x, z.to(dev), d.to(dev), raw_noise_std=1, white_bkgd=True, pytest=True)
    want = RM.restate(raw.double(), z.double(), d.double(), noise.double(), True)
    for a, b in zip(outs, want):
        np.testing.assert_allclose(a.detach().cpu().numpy(), b.numpy(), rtol=2e-4, atol=2e-6)
    torch.autograd.backward(list(outs), [g.to(dev) for g in grads])
    ratio = RM.worst_ratio(x.grad.cpu(), RM.autograd_grad(raw, z, d, noise, True, grads))
    print(f"composite_bwd with noise (R,S)=({R},{S}): worst ratio {ratio:.3e}")
    assert ratio <= BOUND
    with torch.no_grad():                                         # the no-grad route takes the same noise
        assert _same(rnh.raw2outputs(raw.to(dev), z.to(dev), d.to(dev), raw_noise_std=1, white_bkgd=True, pytest=True),
                     [o.detach() for o in outs])
    # jitter: sorted, inside [near, far], repeatable under a fixed seed
    torch.manual_seed(3)
    field = rnh.NeRF2D(D=8, W=64, input_ch=63, output_ch=4, skips=[4]).to(dev)
    ro = torch.zeros(7, 3, device=dev) + torch.tensor([0., 0., 1.5], device=dev)
    rd = torch.nn.functional.normalize(torch.randn(7, 3, device=dev), dim=-1)
    runs = []
    for _ in range(2):
        torch.manual_seed(12)
        with torch.no_grad():
            out, extras = rnh.render_rays(field, ro, rd, 0.5, 2.5, 33, perturb=1., raw_noise_std=1., return_extras=True)
        runs.append((out, extras['z_vals']))
    zj = runs[0][1]
    assert (zj[:, 1:] >= zj[:, :-1]).all() and zj.min().item() >= 0.5 and zj.max().item() <= 2.5
    t = torch.linspace(0., 1., 33, device=dev)
    assert not torch.equal(zj, (0.5 * (1 - t) + 2.5 * t).expand(7, 33))
    assert torch.equal(runs[0][1], runs[1][1]) and _same(runs[0][0], runs[1][0])


def _embed(x, L=10):
    out = [x]
    for l in range(L):
        out += [torch.sin(x * 2.0 ** l), torch.cos(x * 2.0 ** l)]
    return torch.cat(out, -1)


def _torch_field(params, pts, skip=4):
    """NeRF2D.forward on the embedded points with plain torch ops; params = [w0, b0, ..., w_out, b_out]."""
    e = _embed(pts)
    h = e
    n = len(params) // 2 - 1
    for i in range(n):
        h = torch.relu(h @ params[2 * i].T + params[2 * i + 1])
        if i == skip:
            h = torch.cat([e, h], -1)
    return h @ params[-2].T + params[-1]


def _chain_reference(params32, ro, rd, zs, target, dtype):
    """Parameter gradients of the chain's loss by CPU autograd in `dtype`; zs = [z] or [z_coarse, z_all]."""
    ps = [p.to(dtype).requires_grad_(True) for p in params32]
    ro, rd, target = ro.to(dtype), rd.to(dtype), target.to(dtype)
    loss = 0.
    for k, z in enumerate(zs):
        z = z.to(dtype)
        pts = ro[:, None, :] + rd[:, None, :] * z[:, :, None]
        rgb, _, acc, _, _ = RM.restate(_torch_field(ps, pts), z, rd)
        loss = loss + ((rgb - target) ** 2).mean()
        if k == len(zs) - 1:
            loss = loss + 0.1 * acc.mean()
    loss.backward()
    return [p.grad for p in ps]


@pytest.mark.parametrize("N_importance", [0, 16])
def test_whole_chain_parameter_gradients(dev, N_importance):
    """field -> compositing -> loss = img2mse(rgb, target) + 0.1 acc.mean() (+ img2mse(rgb_coarse, target) when hierarchical):
    parameter gradients against float64 CPU autograd through a torch MLP with the same weights, a torch embedding and the
    restatement.  Per parameter tensor the relative L2 distance may be four times that of the float32 CPU run of the same
    reference (another summation order plus hardware transcendentals), and never has to be below 2e-4.  The sample positions are
    outside the gradient: the reference takes the merged z_vals of the HIP run (sample_pdf with det=True on both sides would
    differ by the rounding of the coarse weights)."""
    from contexture_nerf_amd import run_nerf_helpers as rnh
    torch.manual_seed(41)
    field = rnh.NeRF2D(D=8, W=64, input_ch=63, output_ch=4, skips=[4]).to(dev)
    g = torch.Generator().manual_seed(5)
    R, S = 96, 33
    ro = torch.tensor([0., 0., 1.5]) + 0.05 * torch.randn(R, 3, generator=g)
    rd = torch.nn.functional.normalize(torch.randn(R, 3, generator=g) * 0.3 + torch.tensor([0., 0., -1.]), dim=-1)
    target = torch.rand(R, 3, generator=g)
    out, extras = rnh.render_rays(field, ro.to(dev), rd.to(dev), 0.5, 2.5, S, N_importance=N_importance, return_extras=True)
    loss = rnh.img2mse(out[0], target.to(dev)) + 0.1 * out[2].mean()
    t = torch.linspace(0., 1., S)
    zs = [(0.5 * (1. - t) + 2.5 * t).expand(R, S)]
    if N_importance:
        loss = loss + rnh.img2mse(extras['rgb0'], target.to(dev))
        assert extras['z_vals'].shape == (R, S + N_importance)
        zs.append(extras['z_vals'].cpu())
    loss.backward()
    params = field._params()
    got = [p.grad.cpu() for p in params]
    p32 = [p.detach().cpu() for p in params]
    want = _chain_reference(p32, ro, rd, zs, target, torch.float64)
    f32 = _chain_reference(p32, ro, rd, zs, target, torch.float32)
    rel = lambda a, b: ((a.double() - b).norm() / b.norm()).item()
    rows = [(rel(a, w), rel(c, w)) for a, w, c in zip(got, want, f32)]
    print(f"chain N_importance={N_importance}: relative L2 per parameter tensor, HIP worst {max(r[0] for r in rows):.3e}, "
          f"float32 CPU worst {max(r[1] for r in rows):.3e}")
    for i, (a, c) in enumerate(rows):
        assert a <= max(4 * c, 2e-4), (i, a, c)


def _teacher_views(dev):
    from contexture_nerf_amd import run_nerf_helpers as rnh, volume_render as vr
    torch.manual_seed(8)
    teacher = rnh.NeRF2D(D=8, W=64, input_ch=63, output_ch=4, skips=[4]).to(dev)
    with torch.no_grad():
        teacher.output_linear.bias[3] = 3.0
    K = vr.pinhole(16, 16)
    c, s = np.cos(0.6), np.sin(0.6)
    c2ws = torch.tensor([[[1, 0, 0, 0.0], [0, 1, 0, 0.0], [0, 0, 1, 1.5]],
                         [[c, 0, s, 1.5 * s], [0, 1, 0, 0.0], [-s, 0, c, 1.5 * c]]], dtype=torch.float32, device=dev)
    images = torch.stack([vr.render_image(teacher, 16, 16, K, c2ws[v], 0.5, 2.5, 32)['rgb'] for v in range(2)])
    return images, c2ws, K


def test_fit_views_trains_and_repeats(dev):
    from contexture_nerf_amd import run_nerf_helpers as rnh, volume_render as vr
    images, c2ws, K = _teacher_views(dev)
    assert images.shape == (2, 16, 16, 3)
    hists = []
    for _ in range(2):
        torch.manual_seed(9)
        student = rnh.NeRF2D(D=8, W=64, input_ch=63, output_ch=4, skips=[4]).to(dev)
        hists.append(vr.fit_views(student, images, c2ws, K, 0.5, 2.5, iters=40, rays_per_iter=128, seed=0, N_samples=32))
    h = hists[0]
    assert len(h) == 40 and all(np.isfinite(v) for v in h)
    print(f"fit_views: first five {np.mean(h[:5]):.5f}, last five {np.mean(h[-5:]):.5f}")
    assert np.mean(h[-5:]) < np.mean(h[:5])
    assert hists[0] == hists[1]


def test_train_step_hierarchical(dev):
    """One hierarchical step: device scalars back, every parameter moved, coarse and fine pass both in the loss."""
    from contexture_nerf_amd import run_nerf_helpers as rnh, volume_render as vr
    images, c2ws, K = _teacher_views(dev)
    torch.manual_seed(10)
    student = rnh.NeRF2D(D=8, W=64, input_ch=63, output_ch=4, skips=[4]).to(dev)
    before = [p.detach().clone() for p in student.parameters()]
    ro, rd = rnh.get_rays(16, 16, K, c2ws[0])
    opt = torch.optim.Adam(student.parameters(), lr=5e-4)
    step = vr.train_step(student, opt, ro.reshape(-1, 3), rd.reshape(-1, 3), images[0].reshape(-1, 3), 0.5, 2.5, 16, N_importance=8,
                         raw_noise_std=1.0)
    assert step['loss'].is_cuda and step['loss'].shape == () and step['psnr'].shape == ()
    assert torch.isfinite(step['loss']) and torch.isfinite(step['psnr'])
    assert all(not torch.equal(a, b) for a, b in zip(before, student.parameters()))


def test_refusals(dev):
    from contexture_nerf_amd import _lib as L, run_nerf_helpers as rnh
    raw, z, d, _ = [None if t is None else t.to(dev) for t in RM.make_case(3, 8, seed=1)]
    with pytest.raises(L.CtxError, match="z_vals / rays_d"):
        rnh.raw2outputs(raw.clone().requires_grad_(True), z.clone().requires_grad_(True), d)
    with pytest.raises(L.CtxError, match="z_vals / rays_d"):
        rnh.raw2outputs(raw, z, d.clone().requires_grad_(True))
    S = 4097                                                      # one past the backward's cap
    raw, z, d, _ = [None if t is None else t.to(dev) for t in RM.make_case(2, S, seed=2)]
    x = raw.requires_grad_(True)
    rgb = rnh.raw2outputs(x, z, d)[0]                            # the forward has no cap
    with pytest.raises(L.CtxError, match="4096 samples per ray"):
        rgb.sum().backward()
    # the library's error text is per thread and backward() ran on autograd's: the entry itself, called from this thread
    lib, out = L.load(), torch.full((2, S, 4), 7.0, device=dev)
    rc = lib.ctx_raymarch_composite_bwd(L.ptr(raw), L.ptr(z), L.ptr(d), None, 2, S, 0, None, None, None, None, None, L.ptr(out), L.stream())
    assert rc != 0 and b"4096 samples per ray" in lib.ctx_last_error()
    assert (out == 7.0).all()                                     # refused before anything was launched
