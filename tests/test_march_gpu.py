"""GPU: the march kernels against their numpy restatement (bit for bit), the packed compositing against the dense kernels (bit for bit on a
rectangular layout) and against float64 autograd on ragged lists, render_rays_marched as the composition of its pieces, the quadrature,
and training through it.  Definitions: tests/march_rule.py, DESIGN section 4g."""
import numpy as np
import pytest
import torch

import march_rule as mr
import test_occupancy_cpu as OC
import test_occupancy_mesh_cpu as OM
import test_occupancy_gpu as OG
from test_march_cpu import ragged_counts

pytestmark = pytest.mark.gpu
f32 = np.float32
NEAR, FAR = 0.5, 2.5


def _grid_args(grid, step):
    from contexture_nerf_amd import _lib as L
    return (L.ptr(grid.cells, torch.uint8, "cells"), grid.G, *map(float, grid.lo), *map(float, grid.hi), *map(float, grid.inv),
            *map(float, grid.h), float(step))


def _march_abi(grid, ro, rd, step, u=None, n_want=None):
    """ctx_occ_march_count, torch.cumsum, ctx_occ_march_write with a given u -> (count, ray_off, ray_id, t, dt, pts) device tensors."""
    from contexture_nerf_amd import _lib as L
    lib = L.load()
    R, dev = ro.shape[0], ro.device
    count = torch.full((R,), -7, dtype=torch.int32, device=dev)
    L.check(lib.ctx_occ_march_count(L.ptr(ro), L.ptr(rd), R, NEAR, FAR, *_grid_args(grid, step), L.ptr(count), L.stream()))
    ray_off = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    ray_off[1:] = torch.cumsum(count, 0, dtype=torch.int64)
    n = int(ray_off[-1].item())
    ray_id = torch.full((n,), -1, dtype=torch.int32, device=dev)
    t, dt, pts = (torch.full(s, float('nan'), device=dev) for s in ((n,), (n,), (n, 3)))
    L.check(lib.ctx_occ_march_write(L.ptr(ro), L.ptr(rd), R, NEAR, FAR, *_grid_args(grid, step), L.ptr(ray_off), L.ptr(u), n, L.ptr(ray_id),
                                    L.ptr(t), L.ptr(dt), L.ptr(pts), L.stream()))
    return count, ray_off, ray_id, t, dt, pts


# ---- 1. the march kernels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,G,cells,R,seed", mr.march_cases(), ids=[c[0] for c in mr.march_cases()])
def test_march_kernels_equal_the_restatement(dev, name, G, cells, R, seed):
    from contexture_nerf_amd import volume_render as vr
    ro, rd = OM.span_rays(np.random.default_rng(seed), R)
    grid = vr.OccupancyGrid.from_mask(torch.from_numpy(cells != 0).to(dev), -1.0, 1.0)
    d_ro, d_rd = OG._dev(dev, ro, rd)
    args = (ro, rd, NEAR, FAR, cells, grid.lo, grid.hi, grid.inv, grid.h)
    total = 0
    for step in mr.march_steps(G):
        want = mr.occ_march_np(*args, step)
        for given in (False, True):
            u = np.random.default_rng(seed + 5).random(len(want[3])).astype(f32) if given else None
            if given:
                want = mr.occ_march_np(*args, step, u=u)
            got = _march_abi(grid, d_ro, d_rd, step, None if u is None else torch.from_numpy(u).to(dev))
            for k, (g, w) in enumerate(zip(got, want[:6])):
                assert np.array_equal(g.cpu().numpy(), w), (step, given, ("count", "ray_off", "ray_id", "t", "dt", "pts")[k])
        total += len(want[3])
        # the host entry: the same lists, and the bound holds
        lists = grid.march(d_ro, d_rd, NEAR, FAR, step)
        want = mr.occ_march_np(*args, step)
        assert [x.dtype for x in lists] == [torch.int64, torch.int32, torch.float32, torch.float32, torch.float32]
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(lists, want[1:6]))
        assert int(want[0].max(initial=0)) <= grid.march_bound(step)
    if not cells.any():
        assert total == 0                                                            # all zeros: no sample anywhere
    if cells.all():
        assert total > 0                                                             # all ones: the box crossing
    # the span kernel, now on the shared walk, keeps its rule
    span, hit = grid.ray_spans(d_ro, d_rd, NEAR, FAR)
    want_span, want_hit = OM.occ_ray_spans_np(*args)
    assert np.array_equal(span.cpu().numpy(), want_span) and np.array_equal(hit.cpu().numpy(), want_hit != 0)


def test_march_run_clamps(dev):
    """The two clamps of k, fed straight to the ABI (the host refuses such steps): a step far below a run's length gives 4097 samples per
    run, and a quotient len / step that rounds to zero (a direction of 1e-20, a step of 3e38) gives one."""
    from contexture_nerf_amd import volume_render as vr
    G = 4
    cells = np.zeros((G, G, G), np.uint8)
    cells[1, 1, 0] = cells[1, 1, 3] = cells[2, 2, 2] = 1
    grid = vr.OccupancyGrid.from_mask(torch.from_numpy(cells != 0).to(dev), -1.0, 1.0)
    ro = f32([[-1.5, -0.25, -0.25], [0.25, 0.25, 0.25], [0.1, 0.2, 1.5]])
    rd = f32([[1.0, 0.0, 0.0], [1e-20, 0.0, 0.0], [0.0, 0.0, -1.0]])
    d_ro, d_rd = OG._dev(dev, ro, rd)
    for step, want_count in ((1e-6, [2 * 4097, 1, 4097]), (3e38, [2, 1, 1])):
        want = mr.occ_march_np(ro, rd, NEAR, FAR, cells, grid.lo, grid.hi, grid.inv, grid.h, step)
        assert want[0].tolist() == want_count, (step, want[0])
        got = _march_abi(grid, d_ro, d_rd, step)
        for k, (g, w) in enumerate(zip(got, want[:6])):
            assert np.array_equal(g.cpu().numpy(), w), (step, ("count", "ray_off", "ray_id", "t", "dt", "pts")[k])


def test_march_perturb_is_seeded_and_write_stays_inside_its_ray(dev):
    from contexture_nerf_amd import _lib as L, volume_render as vr
    G = 16
    grid = vr.OccupancyGrid.from_mask(torch.from_numpy(OM.ball_mask(G, 0.6)).to(dev), -1.0, 1.0)
    ro, rd, _ = OG._dev(dev, *OC.random_rays(np.random.default_rng(2), 70, 4))
    step = float(grid.h[0]) / 2
    a = grid.march(ro, rd, NEAR, FAR, step, perturb=True, generator=torch.Generator(device=dev).manual_seed(3))
    b = grid.march(ro, rd, NEAR, FAR, step, perturb=True, generator=torch.Generator(device=dev).manual_seed(3))
    mid = grid.march(ro, rd, NEAR, FAR, step)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(a[0], mid[0]) and torch.equal(a[3], mid[3])
    assert not torch.equal(a[2], mid[2]) and bool(((a[2] - mid[2]).abs() <= 0.5 * mid[3] * (1 + 1e-6)).all())
    n = a[2].numel()
    u = torch.rand(n, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    want = mr.occ_march_np(ro.cpu().numpy(), rd.cpu().numpy(), NEAR, FAR, grid.cells.cpu().numpy(), grid.lo, grid.hi, grid.inv, grid.h, step,
                           u=u.cpu().numpy())
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(a, want[1:6]))
    # offsets that give every ray one sample less than it computes: the write pass stops at its ray's end
    lib = L.load()
    short = torch.clamp(mid[0][1:] - mid[0][:-1] - 1, min=0)
    off = torch.zeros_like(mid[0])
    off[1:] = torch.cumsum(short, 0)
    m = int(off[-1].item())
    ray_id = torch.full((m + 8,), -1, dtype=torch.int32, device=dev)
    t, dt, pts = (torch.full(s, -5.0, device=dev) for s in ((m + 8,), (m + 8,), (m + 8, 3)))
    L.check(lib.ctx_occ_march_write(L.ptr(ro), L.ptr(rd), 70, NEAR, FAR, *_grid_args(grid, step), L.ptr(off), None, m, L.ptr(ray_id), L.ptr(t),
                                    L.ptr(dt), L.ptr(pts), L.stream()))
    assert bool((ray_id[m:] == -1).all()) and bool((t[m:] == -5.0).all()) and bool((pts[m:] == -5.0).all())
    assert torch.equal(ray_id[:m], torch.repeat_interleave(torch.arange(70, device=dev), short).to(torch.int32))
    for r in (0, 35, 69):                                                      # each ray holds the head of its own list
        k = int(short[r])
        assert torch.equal(t[int(off[r]):int(off[r]) + k], mid[2][int(mid[0][r]):int(mid[0][r]) + k])


# ---- 2. no tolerance: a rectangular layout gives the dense kernels' bits ---------------------------------------------------------------------
def _packed_abi(raw, t, dt, d, noise, ray_off, white, grads=None, prefill=None):
    from contexture_nerf_amd import _lib as L
    lib = L.load()
    R, n, dev = d.shape[0], raw.shape[0], d.device
    rgb, disp, acc, w, depth = (torch.full(s, 7.0, device=dev) for s in ((R, 3), (R,), (R,), (n,), (R,)))
    L.check(lib.ctx_raymarch_packed_fwd(L.ptr(raw), L.ptr(t), L.ptr(dt), L.ptr(d), L.ptr(noise), L.ptr(ray_off), R, n, int(white), L.ptr(rgb),
                                        L.ptr(disp), L.ptr(acc), L.ptr(w), L.ptr(depth), L.stream()))
    if grads is None:
        return (rgb, disp, acc, w, depth), None
    grad = torch.full((n, 4), float('nan') if prefill is None else prefill, device=dev)
    L.check(lib.ctx_raymarch_packed_bwd(L.ptr(raw), L.ptr(t), L.ptr(dt), L.ptr(d), L.ptr(noise), L.ptr(ray_off), R, n, int(white),
                                        *[L.ptr(g) for g in grads], L.ptr(grad), L.stream()))
    return (rgb, disp, acc, w, depth), grad


@pytest.mark.parametrize("R,S", [(5, 33), (3, 64), (4, 65), (2, 200), (1, 1)])
def test_packed_kernels_equal_the_dense_ones_on_a_rectangular_layout(dev, R, S):
    from contexture_nerf_amd import _lib as L, run_nerf_helpers as rnh
    from test_raymarch_train_cpu import make_case, make_grads
    lib = L.load()
    for white in (False, True):
        for with_noise in (False, True):
            raw, z, d, noise = [None if x is None else x.to(dev) for x in make_case(R, S, seed=R * 100 + S, with_noise=with_noise)]
            grads = [g.to(dev) for g in make_grads(R, S, 'all', seed=S)]
            want = rnh._composite_fwd(raw, z, d, noise, white)
            want_grad = torch.full((R, S, 4), float('nan'), device=dev)
            L.check(lib.ctx_raymarch_composite_bwd(L.ptr(raw), L.ptr(z), L.ptr(d), L.ptr(noise), R, S, int(white), *[L.ptr(g) for g in grads],
                                                   L.ptr(want_grad), L.stream()))
            dt = torch.cat([z[:, 1:] - z[:, :-1], torch.full((R, 1), 1e10, device=dev)], -1)
            ray_off = torch.arange(R + 1, device=dev, dtype=torch.int64) * S
            pgrads = [grads[0], grads[1], grads[2], grads[3].reshape(-1).contiguous(), grads[4]]
            got, got_grad = _packed_abi(raw.reshape(-1, 4), z.reshape(-1), dt.reshape(-1).contiguous(), d,
                                        None if noise is None else noise.reshape(-1), ray_off, white, pgrads)
            for k, (g, w) in enumerate(zip(got, want)):                 # as bit patterns: the 0 / 0 disparity of the acc == 0 ray included
                assert torch.equal(g.reshape(w.shape).view(torch.int32), w.view(torch.int32)), (white, with_noise, k)
            assert torch.equal(got_grad.reshape(R, S, 4), want_grad) and bool(torch.isfinite(got_grad).all()), (white, with_noise)


# ---- 3. ragged lists against float64 autograd of the formula --------------------------------------------------------------------------------
@pytest.mark.parametrize("white", (False, True))
@pytest.mark.parametrize("with_noise", (False, True))
def test_packed_kernels_on_ragged_lists(dev, white, with_noise):
    counts = ragged_counts(23, 4)
    R = len(counts)
    host = mr.make_packed_case(counts, seed=21, with_noise=with_noise)
    raw, t, dt, d, ray_off, noise = host
    hgrads = mr.make_packed_grads(R, raw.shape[0], seed=6)
    want = mr.restate_packed(raw.double(), t.double(), dt.double(), d.double(), ray_off, None if noise is None else noise.double(), white)
    want_grad = mr.packed_autograd_grad(raw, t, dt, d, ray_off, noise, white, hgrads)
    D = [None if x is None else x.to(dev) for x in host]
    dgrads = [g.to(dev) for g in hgrads]
    got, got_grad = _packed_abi(*D[:4], D[5], D[4], white, dgrads)                 # grad_raw prefilled with NaN
    for k, (g, w) in enumerate(zip(got, want)):
        assert torch.allclose(g.cpu().double(), w, rtol=2e-4, atol=2e-6, equal_nan=True), (k, (g.cpu().double() - w).abs().max())
    assert bool(torch.isfinite(got_grad).all())                                     # every row written
    ratio = mr.ray_ratio(got_grad.cpu(), want_grad, ray_off)
    assert ratio <= 2e-4, ratio
    pre = raw[:, 3] if noise is None else raw[:, 3] + noise
    assert bool((got_grad.cpu()[:, 3][pre <= 0] == 0).all())
    # the empty rays: acc = depth = 0, rgb 0 or white, disp 0/0
    for r in np.nonzero(counts == 0)[0]:
        assert float(got[2][r]) == 0 and float(got[4][r]) == 0 and bool(torch.isnan(got[1][r])) and bool((got[0][r] == (1.0 if white else 0.0)).all())
    assert counts[0] == 0 and counts[-1] == 0 and set(counts) == {0, 1, 2, 63, 64, 65, 130}
    # every ray launched alone gives the bits it has in the batch
    off = ray_off.tolist()
    for r in range(R):
        s = slice(off[r], off[r + 1])
        one_off = torch.tensor([0, off[r + 1] - off[r]], dtype=torch.int64, device=dev)
        g1 = [dgrads[0][r:r + 1], dgrads[1][r:r + 1], dgrads[2][r:r + 1], dgrads[3][s], dgrads[4][r:r + 1]]
        o1, gr1 = _packed_abi(D[0][s], D[1][s], D[2][s], D[3][r:r + 1], None if D[5] is None else D[5][s], one_off, white, g1)
        assert all(OG._eq(a, b) for a, b in zip(o1, (got[0][r:r + 1], got[1][r:r + 1], got[2][r:r + 1], got[3][s], got[4][r:r + 1]))), r
        assert torch.equal(gr1, got_grad[s]), r
    # absent upstream gradients are null pointers
    only_rgb = [dgrads[0], None, None, None, None]
    _, g_rgb = _packed_abi(*D[:4], D[5], D[4], white, only_rgb)
    want_rgb = mr.packed_autograd_grad(raw, t, dt, d, ray_off, noise, white, [hgrads[0], None, None, None, None])
    assert mr.ray_ratio(g_rgb.cpu(), want_rgb, ray_off) <= 2e-4


def test_packed_backward_poisons_a_ray_beyond_4096_samples(dev):
    counts = [3, 4097, 70, 0]
    host = mr.make_packed_case(counts, seed=8)
    raw, t, dt, d, ray_off, _ = [None if x is None else x.to(dev) for x in host]
    grads = [g.to(dev) for g in mr.make_packed_grads(4, raw.shape[0], seed=1)]
    out, grad = _packed_abi(raw, t, dt, d, None, ray_off, False, grads, prefill=0.0)
    assert bool(torch.isnan(grad[3:3 + 4097]).all())
    assert bool(torch.isfinite(out[0]).all())                                       # the forward has no such limit
    for r, s in ((0, slice(0, 3)), (2, slice(3 + 4097, 3 + 4097 + 70))):             # the neighbours: the bits each has alone
        g1 = [grads[0][r:r + 1], grads[1][r:r + 1], grads[2][r:r + 1], grads[3][s], grads[4][r:r + 1]]
        one_off = torch.tensor([0, s.stop - s.start], dtype=torch.int64, device=dev)
        _, alone = _packed_abi(raw[s], t[s], dt[s], d[r:r + 1], None, one_off, False, g1)
        assert torch.equal(alone, grad[s]) and bool(torch.isfinite(alone).all()) and bool(alone.any())


# ---- 4. render_rays_marched is the composition of its pieces ---------------------------------------------------------------------------------
def _shell_grid(dev, G=16):
    from contexture_nerf_amd import volume_render as vr
    v, f = OM.icosphere(2, 0.6)
    return vr.OccupancyGrid.from_mesh(*OG._dev(dev, v, f), G, -1.0, 1.0, dilate=1)


MARCHED_CASES = [(white, noise, perturb) for white in (False, True) for noise in (0.0, 1.0) for perturb in (0.0, 1.0)]


@pytest.mark.parametrize("white,noise,perturb", MARCHED_CASES)
def test_render_rays_marched_equals_the_composition(dev, white, noise, perturb):
    from contexture_nerf_amd import run_nerf_helpers as rnh
    field = OG._field(dev)
    grid = _shell_grid(dev)
    R = 41
    ro, rd, _ = OG._dev(dev, *OC.random_rays(np.random.default_rng(5), R, 4))
    step = float(grid.h[0]) / 2
    got, gx = rnh.render_rays(field, ro, rd, NEAR, FAR, 64, white_bkgd=white, perturb=perturb, raw_noise_std=noise, march=step,
                              occupancy=grid, generator=torch.Generator(device=dev).manual_seed(9), return_extras=True)
    got_grads = OG._backward_all(field, got, gx, seed=3)
    # the same chain from the restatement's lists
    gen = torch.Generator(device=dev).manual_seed(9)
    args = (ro.cpu().numpy(), rd.cpu().numpy(), NEAR, FAR, grid.cells.cpu().numpy(), grid.lo, grid.hi, grid.inv, grid.h, step)
    lists = mr.occ_march_np(*args)
    if perturb > 0:
        u = torch.rand(len(lists[3]), device=dev, generator=gen)
        lists = mr.occ_march_np(*args, u=u.cpu().numpy())
    ray_off, ray_id, t, dt, pts = OG._dev(dev, *lists[1:6])
    n = t.numel()
    assert 0 < n and 0 < int((lists[0] == 0).sum()) < R                             # rays that hit and rays that miss
    want = rnh.raw2outputs_packed(field.forward_pts(pts), t, dt, rd, ray_off, noise, white, gen)
    want_grads = OG._backward_all(field, want, {}, seed=3)
    assert sorted(gx) == ['dt', 'pts', 'ray_id', 'ray_off', 't'] and tuple(got[3].shape) == (n,)
    for key, w in zip(('ray_off', 'ray_id', 't', 'dt', 'pts'), (ray_off, ray_id, t, dt, pts)):
        assert torch.equal(gx[key], w), key
    for a, b in zip(got, want):
        assert OG._eq(a, b)
    assert len(got_grads) == 18
    for k, (a, b) in enumerate(zip(got_grads, want_grads)):
        assert torch.equal(a, b), f"parameter gradient {k}"
    assert any(bool(x.any()) for x in got_grads) and 0 < float(got[2].detach().max())
    miss = torch.from_numpy(lists[0] == 0).to(dev)
    assert bool((got[2].detach()[miss] == 0).all()) and bool((got[0].detach()[miss] == (1.0 if white else 0.0)).all())


def test_marched_repeat_and_side_stream_give_equal_bits(dev):
    from contexture_nerf_amd import run_nerf_helpers as rnh
    field = OG._field(dev)
    grid = _shell_grid(dev)
    ro, rd, _ = OG._dev(dev, *OC.random_rays(np.random.default_rng(8), 33, 4))

    def run():
        out, ex = rnh.render_rays_marched(field, ro, rd, NEAR, FAR, grid, float(grid.h[0]) / 2, white_bkgd=True, perturb=1., raw_noise_std=1.,
                                          generator=torch.Generator(device=dev).manual_seed(4), return_extras=True)
        return out, OG._backward_all(field, out, ex, seed=2)
    first = run()
    again = run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = run()
    torch.cuda.current_stream().wait_stream(side)
    for got in (again, other):
        assert all(OG._eq(a, b) for a, b in zip(got[0], first[0])) and all(torch.equal(a, b) for a, b in zip(got[1], first[1]))


def test_marched_with_an_empty_grid(dev):
    from contexture_nerf_amd import run_nerf_helpers as rnh, volume_render as vr
    field = OG._field(dev)
    grid = vr.OccupancyGrid.from_mask(torch.zeros(8, 8, 8, dtype=torch.bool, device=dev), -1.0, 1.0)
    R = 9
    ro, rd, _ = OG._dev(dev, *OC.random_rays(np.random.default_rng(1), R, 4))
    calls = []
    orig = field.forward_pts
    field.forward_pts = lambda pts: calls.append(1) or orig(pts)
    for white in (False, True):
        out, ex = rnh.render_rays_marched(field, ro, rd, NEAR, FAR, grid, 0.125, white_bkgd=white, return_extras=True)
        assert ex['t'].numel() == 0 and tuple(ex['pts'].shape) == (0, 3) and ex['ray_off'].tolist() == [0] * (R + 1)
        assert bool((out[2] == 0).all()) and bool((out[4] == 0).all()) and bool(torch.isnan(out[1]).all()) and out[3].numel() == 0
        assert bool((out[0] == (1.0 if white else 0.0)).all()) and not out[0].requires_grad
    before = [p.detach().clone() for p in field.parameters()]
    opt = torch.optim.Adam(field.parameters(), lr=1e-2)
    step = vr.train_step(field, opt, ro, rd, torch.rand(R, 3, device=dev), NEAR, FAR, 64, occupancy=grid, march=0.125)
    assert torch.isfinite(step['loss']) and torch.isfinite(step['psnr'])
    assert all(torch.equal(a, b) for a, b in zip(before, field.parameters())) and not calls          # untouched; the field never ran
    del field.forward_pts


# ---- 5. quadrature ------------------------------------------------------------------------------------------------------------------------------
class _ConstField:
    """forward_pts -> constant density and colour."""

    def __init__(self, sigma, dev):
        self.row = torch.tensor([0.3, -0.2, 0.9, sigma], device=dev)

    def forward_pts(self, pts):
        return self.row.expand(pts.shape[0], 4).contiguous()


def test_marched_quadrature_of_a_constant_density(dev):
    """Constant sigma0 inside the occupied cells: acc = 1 - exp(-sigma0 * occupied length).  The march tiles its runs exactly, so its acc
    is that of sum dt*|d| to the forward tolerance; the dense occupancy path at N_samples = 2048 marks a sample by its point and gives it
    the spacing dz, so it can misplace one dz per run boundary: 2 * runs * dz * |d| of length, times sigma0 of optical depth, and
    |d acc| <= |d tau|.  far = 4 puts every ray's last sample behind the ball (checked): the dense path gives that sample the 1e10
    distance, which the march by design does not."""
    from contexture_nerf_amd import run_nerf_helpers as rnh, volume_render as vr
    G, sigma0, R, S, far = 16, 3.0, 64, 2048, 4.0
    grid = vr.OccupancyGrid.from_mask(torch.from_numpy(OM.ball_mask(G, 0.6)).to(dev), -1.0, 1.0)
    ro, rd, _ = OG._dev(dev, *OC.random_rays(np.random.default_rng(12), R, 4, spread=0.5))
    field = _ConstField(sigma0, dev)
    step = float(grid.h[0]) / 2
    with torch.no_grad():
        out, ex = rnh.render_rays_marched(field, ro, rd, NEAR, far, grid, step, return_extras=True)
        dense = rnh.render_rays(field, ro, rd, NEAR, far, S, occupancy=grid)
    lists = mr.occ_march_np(ro.cpu().numpy(), rd.cpu().numpy(), NEAR, far, grid.cells.cpu().numpy(), grid.lo, grid.hi, grid.inv, grid.h, step)
    run_ray, _, run_b, k = lists[6]
    assert float(run_b.max()) < far - 0.1                                            # no run reaches the last dense sample
    runs = np.bincount(run_ray[k > 0], minlength=R)
    nrm = np.linalg.norm(rd.cpu().numpy().astype(np.float64), axis=-1)
    length = np.bincount(lists[2], weights=lists[4].astype(np.float64), minlength=R) * nrm
    want = 1.0 - np.exp(-sigma0 * length)
    acc = out[2].cpu().numpy().astype(np.float64)
    assert runs.max() >= 1 and (runs == 0).any() and 0.3 < want.max() < 0.999
    assert np.all(np.abs(acc - want) <= 2e-4 * np.abs(want) + 2e-6), np.abs(acc - want).max()
    dz = (far - NEAR) / (S - 1)
    tol = sigma0 * nrm * 2 * runs * dz
    dacc = dense[2].cpu().numpy().astype(np.float64)
    assert np.all(np.abs(acc - dacc) <= tol + 2e-4 * np.abs(want) + 2e-6), (np.abs(acc - dacc) - tol).max()
    # uniform spacing on the surface: every interval of a hit ray is at most one step of world length
    assert bool((ex['dt'] * torch.linalg.norm(rd, dim=-1)[ex['ray_id'].long()] <= step * (1 + 2.0 ** -20)).all())


# ---- 7. training through the march ---------------------------------------------------------------------------------------------------------------
def test_fit_views_marched(dev):
    """The toy scene of test_occupancy_mesh_gpu.test_fit_views_with_a_mesh_grid, with the student's samples marched at h/2."""
    from contexture_nerf_amd import volume_render as vr
    G, H, W, S = 16, 16, 16, 32
    teacher_grid = vr.OccupancyGrid.from_mask(torch.from_numpy(OM.ball_mask(G, 0.6)).to(dev), -1.0, 1.0)
    teacher = OG._field(dev, seed=1, sigma_bias=8.0)
    K = vr.pinhole(H, W)
    c2ws = torch.tensor([[[1., 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1.5]], [[0., 0, 1, 1.5], [0, 1, 0, 0], [-1, 0, 0, 0]]], device=dev)
    imgs = torch.stack([vr.render_image(teacher, H, W, K, c2ws[v], 0.5, 2.5, S, white_bkgd=True, occupancy=teacher_grid)['rgb'] for v in range(2)])

    def fit():
        student = OG._field(dev, seed=2)
        grid = _shell_grid(dev, G)
        before = grid.cells.clone()
        hist = vr.fit_views(student, imgs, c2ws, K, 0.5, 2.5, 40, rays_per_iter=256, seed=3, raw_noise_std=1., white_bkgd=True, occupancy=grid,
                            occupancy_every=0, march=float(grid.h[0]) / 2)
        assert torch.equal(grid.cells, before) and not bool(grid.dens.any()) and 0 < grid.fraction() < 1       # the grid is as it was
        return hist
    a, b = fit(), fit()
    print(f"fit_views marched at h/2: loss first 5 {np.mean(a[:5]):.4f}, last 5 {np.mean(a[-5:]):.4f}")
    assert len(a) == 40 and all(np.isfinite(a)) and a == b
    assert np.mean(a[-5:]) < np.mean(a[:5])


def test_render_image_marched(dev):
    from contexture_nerf_amd import run_nerf_helpers as rnh, volume_render as vr
    field = OG._field(dev, sigma_bias=8.0)
    v, f = OM.icosphere(2, 0.3)
    grid = vr.OccupancyGrid.from_mesh(*OG._dev(dev, v, f), 16, -1.0, 1.0, dilate=1)
    K = vr.pinhole(24, 24)
    c2w = torch.tensor([[1., 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1.5]], device=dev)
    step = float(grid.h[0]) / 2
    img = vr.render_image(field, 24, 24, K, c2w, NEAR, FAR, 0, white_bkgd=True, occupancy=grid, march=step)
    ro, rd = rnh.get_rays(24, 24, K, c2w)
    ray_off = grid.march(ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous(), NEAR, FAR, step)[0]
    empty = (ray_off[1:] == ray_off[:-1]).reshape(24, 24)
    assert tuple(img['rgb'].shape) == (24, 24, 3) and bool(torch.isfinite(img['rgb']).all())
    assert bool(empty[0, 0]) and not bool(empty[12, 12]) and float(img['acc'][12, 12]) > 0.5
    assert bool((img['acc'][empty] == 0).all()) and bool((img['rgb'][empty] == 1).all())
