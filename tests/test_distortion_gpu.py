"""GPU: the distortion kernels (ctx_distortion_packed_fwd / _bwd) against the float64 pairwise definition at the derived bounds, their
robustness, the chain raw -> raw2outputs_packed -> distortion_loss against float64 autograd, and training with distortion=.
Definitions: tests/distortion_rule.py, DESIGN section 4h."""
import numpy as np
import pytest
import torch

import distortion_rule as dr
import march_rule as mr
import test_occupancy_cpu as OC
import test_occupancy_mesh_cpu as OM
import test_occupancy_gpu as OG
from test_march_cpu import ragged_counts

pytestmark = pytest.mark.gpu
f32 = np.float32


def _abi(w, t, dt, d, ray_off, g_loss=None, n=None, grad_prefill=float('nan')):
    """The two ABI calls on device tensors -> (loss [R] and grad_w [n], both prefilled with NaN; grad_w None without g_loss)."""
    from contexture_nerf_amd import _lib as L
    lib = L.load()
    R, dev = d.shape[0], d.device
    n = w.shape[0] if n is None else n
    loss = torch.full((R,), float('nan'), device=dev)
    L.check(lib.ctx_distortion_packed_fwd(L.ptr(w), L.ptr(t), L.ptr(dt), L.ptr(d), L.ptr(ray_off), R, n, L.ptr(loss), L.stream()))
    if g_loss is None:
        return loss, None
    grad = torch.full((n,), grad_prefill, device=dev)
    L.check(lib.ctx_distortion_packed_bwd(L.ptr(w), L.ptr(t), L.ptr(dt), L.ptr(d), L.ptr(ray_off), R, n, L.ptr(g_loss),
                                          L.ptr(grad) if n else None, L.stream()))
    return loss, grad


# ---- 1. against float64 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", dr.NORMS)
def test_kernels_against_float64_on_ragged_lists(dev, norm):
    k = dr.NORMS.index(norm)
    case = dr.make_case(dr.COUNTS, seed=40 + k, norm=norm)
    g_loss = np.random.default_rng(50 + k).standard_normal(len(dr.COUNTS)).astype(f32)
    D = OG._dev(dev, *case, g_loss)
    loss, grad = _abi(*D)
    ray_off = case[4]
    own = np.zeros(len(case[0]), bool)
    for r in range(len(dr.COUNTS)):
        own[ray_off[r]:ray_off[r + 1]] = True
    assert own.all() and bool(torch.isfinite(grad).all()) and bool(torch.isfinite(loss).all())           # fully written over the NaN prefill
    rf, rg = dr.check(loss.cpu().numpy(), grad.cpu().numpy(), *case, g_loss)
    print(f"|d| = {norm}: largest error / bound, forward {rf:.4f}, gradient {rg:.4f}")
    assert bool((loss >= 0).all()) and bool((loss[torch.from_numpy(np.diff(ray_off) == 0).to(dev)] == 0).all())
    if norm == 0.0:
        assert bool((loss == 0).all()) and bool((grad == 0).all())                                       # a zero direction: exact zeros
        return
    if norm != 1.0:
        return
    # every ray launched alone gives the bits it has in the batch
    for r in range(len(dr.COUNTS)):
        s = slice(int(ray_off[r]), int(ray_off[r + 1]))
        one_off = torch.tensor([0, s.stop - s.start], dtype=torch.int64, device=dev)
        l1, g1 = _abi(D[0][s], D[1][s], D[2][s], D[3][r:r + 1], one_off, D[5][r:r + 1])
        assert torch.equal(l1, loss[r:r + 1]) and torch.equal(g1, grad[s]), r
    # a repeat and a side stream give equal bits
    again = _abi(*D)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _abi(*D)
    torch.cuda.current_stream().wait_stream(side)
    for got in (again, other):
        assert torch.equal(got[0], loss) and torch.equal(got[1], grad)


@pytest.mark.parametrize("R,S", [(1, 1), (3, 64), (4, 65), (2, 200)])
def test_rectangular_layout_through_the_host_entry(dev, R, S):
    from contexture_nerf_amd import run_nerf_helpers as rnh
    (w, z, d), packed = dr.make_rect_case(R, S, seed=R * 100 + S)
    g_loss = np.random.default_rng(S).standard_normal(R).astype(f32)
    W, Z, Dd, G = OG._dev(dev, w, z, d, g_loss)
    W.requires_grad_(True)
    loss = rnh.distortion_loss(W, Z, None, Dd)
    assert tuple(loss.shape) == (R,)
    (loss * G).sum().backward()
    assert tuple(W.grad.shape) == (R, S)
    dr.check(loss.detach().cpu().numpy(), W.grad.reshape(-1).cpu().numpy(), *packed, g_loss)
    with torch.no_grad():                                                            # the plain forward: the same bits, no graph
        plain = rnh.distortion_loss(W, Z, None, Dd)
    assert torch.equal(plain, loss.detach()) and not plain.requires_grad
    # the packed call on the same lists gives the same bits
    P = OG._dev(dev, *packed)
    assert torch.equal(rnh.distortion_loss(*P[:4], P[4]), plain)


# ---- 2. robustness -------------------------------------------------------------------------------------------------------------------------------
def test_empty_batches_give_zeros(dev):
    from contexture_nerf_amd import run_nerf_helpers as rnh
    R = 5
    d = torch.randn(R, 3, device=dev)
    zeros = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    g = torch.ones(R, device=dev)
    loss, grad = _abi(None, None, None, d, zeros, g, n=0)                           # n = 0: the lists may be null
    assert bool((loss == 0).all()) and grad.numel() == 0
    w, t, dt = torch.rand(9, device=dev), torch.linspace(1, 2, 9, device=dev), torch.full((9,), 0.1, device=dev)
    loss, grad = _abi(w, t, dt, d, zeros, g, grad_prefill=-5.0)                      # lists that no ray owns
    assert bool((loss == 0).all()) and bool((grad == -5.0).all())
    # a ray_off outside the lists reads nothing: the ray is taken as empty
    off = torch.tensor([0, 3, 10 ** 6, 6, -2, 9], dtype=torch.int64, device=dev)      # ray 0 holds 0..3; 1 overruns, 2 descends, 3 and 4 leave [0, n]
    loss, grad = _abi(w, t, dt, d, off, g, grad_prefill=-5.0)
    want = dr.distortion_np(*(x.cpu().numpy() for x in (w[:3], t[:3], dt[:3], d[:1])), np.int64([0, 3]))
    assert float(loss[0]) > 0 and bool((loss[1:] == 0).all()) and bool((grad[3:] == -5.0).all()) and bool(torch.isfinite(grad[:3]).all())
    assert np.allclose(loss[:1].cpu().numpy(), want[0], rtol=1e-5) and np.allclose(grad[:3].cpu().numpy(), want[1], rtol=1e-4, atol=1e-7)
    e = torch.empty(0, device=dev)
    host = rnh.distortion_loss(e.requires_grad_(True), e.detach(), e.detach(), d, zeros)
    assert bool((host == 0).all()) and tuple(host.shape) == (R,)


def test_a_nan_weight_poisons_its_own_ray_only(dev):
    case = list(dr.make_case([3, 70, 0, 5, 130], seed=7))
    case[3] = case[3].copy()
    case[3][3] = 0                                                                   # and one zero direction among the others
    g_loss = f32([1.5, -2.0, 1.0, 0.5, -1.0])
    clean = _abi(*OG._dev(dev, *case, g_loss))
    want = dr.oracle64(*case, g_loss)
    dr.check(clean[0].cpu().numpy(), clean[1].cpu().numpy(), *case, g_loss, want=want)
    assert float(clean[0][3]) == 0 and bool((clean[1][73:78] == 0).all())
    for at in (3, 3 + 40, 3 + 69):                                                   # the first sample, one inside the first chunk, one in the second
        bad = [a.copy() for a in case]
        bad[0][at] = np.nan
        loss, grad = _abi(*OG._dev(dev, *bad, g_loss))
        assert bool(torch.isnan(loss[1])) and bool(torch.isnan(grad[3:73]).all()), at
        keep = torch.tensor([0, 2, 3, 4], device=dev)
        assert torch.equal(loss[keep], clean[0][keep]) and torch.equal(grad[:3], clean[1][:3]) and torch.equal(grad[73:], clean[1][73:]), at


def test_gradients_go_to_the_weights_only(dev):
    from contexture_nerf_amd import _lib as L, run_nerf_helpers as rnh
    w, t, dt, d, ray_off = OG._dev(dev, *dr.make_case([3, 0, 5], seed=1))
    for k in (1, 2, 3):
        args = [w, t, dt, d]
        args[k] = args[k].clone().requires_grad_(True)
        with pytest.raises(L.CtxError, match="no gradient with respect to t / dt / rays_d"):
            rnh.distortion_loss(*args, ray_off)
    wg = w.clone().requires_grad_(True)
    loss = rnh.distortion_loss(wg, t, dt, d, ray_off)
    loss.sum().backward()
    assert bool(torch.isfinite(wg.grad).all()) and bool(wg.grad.any()) and t.grad is None and dt.grad is None and d.grad is None


# ---- 3. the chain: g_weights meets a real producer ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("white", (False, True))
@pytest.mark.parametrize("noise_std", (0.0, 1.0))
def test_chain_through_the_packed_compositing(dev, white, noise_std):
    from contexture_nerf_amd import run_nerf_helpers as rnh
    counts = ragged_counts(12, 3)
    raw, t, dt, d, ray_off, _ = mr.make_packed_case(counts, seed=31)
    Raw, T, DT, Dd, Off = (x.to(dev) for x in (raw, t, dt, d, ray_off))
    Raw.requires_grad_(True)
    rgb, _, _, w, _ = rnh.raw2outputs_packed(Raw, T, DT, Dd, Off, noise_std, white, torch.Generator(device=dev).manual_seed(13))
    dist = rnh.distortion_loss(w, T, DT, Dd, Off)
    (dist.mean() + rgb.sum()).backward()
    # the same chain in float64 torch, with the same noise
    noise = (torch.randn(raw.shape[0], device=dev, generator=torch.Generator(device=dev).manual_seed(13)) * noise_std).cpu() if noise_std > 0 else None
    x = raw.double().requires_grad_(True)
    rgb64, _, _, w64, _ = mr.restate_packed(x, t.double(), dt.double(), d.double(), ray_off, None if noise is None else noise.double(), white)
    dist64 = dr.pairwise64(w64, t, dt, d, ray_off)
    (dist64.mean() + rgb64.sum()).backward()
    fb, _ = dr.bounds(w64.detach().numpy(), t.numpy(), dt.numpy(), d.numpy(), ray_off.numpy())
    # the weights carry the compositing's own error, 2e-4 relative (its forward gate), and the loss is quadratic in them
    assert np.all(np.abs(dist.detach().cpu().numpy() - dist64.detach().numpy()) <= fb + 2 * 2e-4 * dist64.detach().numpy())
    assert float(dist64.detach().max()) > 1e-3 and bool(torch.isfinite(Raw.grad).all())
    ratio = mr.ray_ratio(Raw.grad.cpu(), x.grad, ray_off)
    assert ratio <= 2e-4, ratio
    # the distortion term is a visible part of the gradient: without it the same gate fails
    x2 = raw.double().requires_grad_(True)
    mr.restate_packed(x2, t.double(), dt.double(), d.double(), ray_off, None if noise is None else noise.double(), white)[0].sum().backward()
    assert mr.ray_ratio(Raw.grad.cpu(), x2.grad, ray_off) > 2e-4


# ---- 4. training -----------------------------------------------------------------------------------------------------------------------------------
G_TOY, HW, NEAR, FAR = 16, 16, 0.5, 2.5


@pytest.fixture(scope="module")
def toy(dev):
    """The toy scene of test_march_gpu.test_fit_views_marched: two views of a teacher ball, rendered once."""
    from contexture_nerf_amd import volume_render as vr
    teacher_grid = vr.OccupancyGrid.from_mask(torch.from_numpy(OM.ball_mask(G_TOY, 0.6)).to(dev), -1.0, 1.0)
    teacher = OG._field(dev, seed=1, sigma_bias=8.0)
    K = vr.pinhole(HW, HW)
    c2ws = torch.tensor([[[1., 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1.5]], [[0., 0, 1, 1.5], [0, 1, 0, 0], [-1, 0, 0, 0]]], device=dev)
    imgs = torch.stack([vr.render_image(teacher, HW, HW, K, c2ws[v], NEAR, FAR, 32, white_bkgd=True, occupancy=teacher_grid)['rgb'] for v in range(2)])
    return imgs, c2ws, K


def _shell_grid(dev):
    from contexture_nerf_amd import volume_render as vr
    v, f = OM.icosphere(2, 0.6)
    return vr.OccupancyGrid.from_mesh(*OG._dev(dev, v, f), G_TOY, -1.0, 1.0, dilate=1)


def _fit(dev, toy, marched=True, **kw):
    from contexture_nerf_amd import volume_render as vr
    imgs, c2ws, K = toy
    student = OG._field(dev, seed=2)
    grid = _shell_grid(dev) if marched else None
    hist = vr.fit_views(student, imgs, c2ws, K, NEAR, FAR, 40, rays_per_iter=256, seed=3, raw_noise_std=1., white_bkgd=True, occupancy=grid,
                        occupancy_every=0, march=float(grid.h[0]) / 2 if marched else None, N_samples=32, **kw)
    assert len(hist) == 40 and all(np.isfinite(hist))
    return hist, student


def _evaluate(dev, toy, student):
    """On a fixed ray batch (every pixel of both views, midpoint samples, no noise): the mean per-ray distortion and the photometric MSE."""
    from contexture_nerf_amd import run_nerf_helpers as rnh
    imgs, c2ws, K = toy
    rays = [rnh.get_rays(HW, HW, K, c2ws[v]) for v in range(2)]
    ro, rd = (torch.stack([r[k] for r in rays]).reshape(-1, 3).contiguous() for k in (0, 1))
    grid = _shell_grid(dev)
    with torch.no_grad():
        out, ex = rnh.render_rays_marched(student, ro, rd, NEAR, FAR, grid, float(grid.h[0]) / 2, white_bkgd=True, return_extras=True)
        dist = rnh.distortion_loss(out[3], ex['t'], ex['dt'], rd, ex['ray_off'])
    return float(dist.mean()), float(rnh.img2mse(out[0], imgs.reshape(-1, 3)))


def test_fit_views_with_distortion(dev, toy):
    """Measured on an MI355X (40 iterations of 256 rays, march = h/2): mean per-ray distortion of the final field
    0.08904 with lambda = 0 and 0.08389 with lambda = 0.01, ratio 0.942; photometric MSE 0.03291 and 0.03343.  The ratio is not below 0.5,
    so "lambda = 0.01 ends with lower distortion" is printed and not asserted: forty iterations move the density too little for an
    inequality that close to 1 to test anything but the seed."""
    plain, s_plain = _fit(dev, toy)
    zero, _ = _fit(dev, toy, distortion=0.)
    assert zero == plain                                                             # distortion=0. is not passing the argument
    a, s_a = _fit(dev, toy, distortion=0.01)
    b, _ = _fit(dev, toy, distortion=0.01)
    assert a == b and a != plain
    d0, m0 = _evaluate(dev, toy, s_plain)
    d1, m1 = _evaluate(dev, toy, s_a)
    print(f"toy scene after 40 iterations: mean per-ray distortion {d0:.6f} (lambda 0) -> {d1:.6f} (lambda 0.01), ratio {d1 / d0:.3f}; "
          f"photometric MSE {m0:.6f} -> {m1:.6f}")
    assert np.isfinite([d0, d1, m0, m1]).all() and d0 > 0 and d1 > 0
    # the dense path takes the fine pass's weights and z_vals
    c, _ = _fit(dev, toy, marched=False, distortion=0.01)
    e, _ = _fit(dev, toy, marched=False, distortion=0.01)
    f, _ = _fit(dev, toy, marched=False)
    assert c == e and c != f


def test_train_step_reports_the_distortion(dev, toy):
    from contexture_nerf_amd import volume_render as vr
    field = OG._field(dev, seed=2)
    grid = _shell_grid(dev)
    ro, rd, _ = OG._dev(dev, *OC.random_rays(np.random.default_rng(5), 64, 4))
    target = torch.rand(64, 3, device=dev)
    opt = torch.optim.Adam(field.parameters(), lr=1e-3)
    step = float(grid.h[0]) / 2
    for kw in (dict(occupancy=grid, march=step), dict(), dict(N_importance=8)):
        gen = torch.Generator(device=dev).manual_seed(1)
        off = vr.train_step(field, opt, ro, rd, target, NEAR, FAR, 32, generator=gen, **kw)
        assert sorted(off) == ['loss', 'psnr']
        before = [p.detach().clone() for p in field.parameters()]
        gen = torch.Generator(device=dev).manual_seed(1)
        on = vr.train_step(field, opt, ro, rd, target, NEAR, FAR, 32, generator=gen, distortion=0.01, **kw)
        assert sorted(on) == ['distortion', 'loss', 'psnr'] and on['distortion'].dim() == 0 and not on['distortion'].requires_grad
        assert bool(torch.isfinite(on['distortion'])) and float(on['distortion']) > 0 and bool(torch.isfinite(on['loss']))
        assert any(not torch.equal(a, b) for a, b in zip(before, field.parameters()))
    # an all-zeros grid: no sample, no graph: the parameters stay untouched and the distortion is 0
    empty = vr.OccupancyGrid.from_mask(torch.zeros(8, 8, 8, dtype=torch.bool, device=dev), -1.0, 1.0)
    before = [p.detach().clone() for p in field.parameters()]
    out = vr.train_step(field, opt, ro, rd, target, NEAR, FAR, 32, occupancy=empty, march=0.125, distortion=0.01)
    assert float(out['distortion']) == 0 and bool(torch.isfinite(out['loss']))
    assert all(torch.equal(a, b) for a, b in zip(before, field.parameters()))
