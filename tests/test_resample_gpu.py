"""GPU: the resampling kernel (ctx_resample_packed) against the float64 CDF at the bounds the rule is held to, its stores, its bits alone /
repeated / on a side stream, render_rays_marched(resample=) as the composition of the public pieces, the quadrature and the concentration
of the fine pass, and training through it.  Definitions: tests/resample_rule.py, DESIGN section 4i."""
import numpy as np
import pytest
import torch

import resample_rule as rr
import test_occupancy_cpu as OC
import test_occupancy_mesh_cpu as OM
import test_occupancy_gpu as OG
from test_march_gpu import _shell_grid, _ConstField
from test_resample_cpu import _check_properties

pytestmark = pytest.mark.gpu
f32 = np.float32
NEAR, FAR = 0.5, 2.5
COUNTS = [0, 1, 2, 63, 64, 65, 130, 1, 5000, 1, 0]
MARGIN = 8


def _fine_off(counts, K):
    return np.concatenate([[0], np.cumsum(np.asarray(counts) > 0) * K]).astype(np.int64)


def _resample_abi(D, K, fine_off, xi=None, R=None):
    """ctx_resample_packed on the device lists D = (w, ts, dt, ray_off, ro, rd); the outputs carry MARGIN sentinel elements behind n' and
    are prefilled (ray_id -1, the rest NaN) -> (ray_id, t', dt', pts) with the margin."""
    from contexture_nerf_amd import _lib as L
    w, ts, dt, ray_off, ro, rd = D
    dev = w.device
    n1 = int(fine_off[-1].item())
    ray_id = torch.full((n1 + MARGIN,), -1, dtype=torch.int32, device=dev)
    t1, dt1, pts = (torch.full(s, float('nan'), device=dev) for s in ((n1 + MARGIN,), (n1 + MARGIN,), (n1 + MARGIN, 3)))
    L.check(L.load().ctx_resample_packed(L.ptr(w), L.ptr(ts), L.ptr(dt), L.ptr(ray_off), L.ptr(ro), L.ptr(rd), rd.shape[0] if R is None else R,
                                         w.shape[0], K, L.ptr(fine_off), L.ptr(xi), n1, L.ptr(ray_id), L.ptr(t1), L.ptr(dt1), L.ptr(pts),
                                         L.stream()))
    return ray_id, t1, dt1, pts


_HOST = {}


def _host_lists():
    if 'lists' not in _HOST:
        _HOST['lists'] = rr.make_lists(COUNTS, seed=31)
    return _HOST['lists']


# ---- 1. the kernel against the contract ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (1, 16, 64, 65, 130))
def test_kernel_meets_the_contract_and_writes_its_spans_only(dev, K):
    host = _host_lists()
    w, ts, dt, ray_off, ro, rd = host
    D = OG._dev(dev, *host)
    fine_off = _fine_off(COUNTS, K)
    n1 = int(fine_off[-1])
    assert n1 == K * 9                                                              # nine of the eleven rays hold samples
    for drawn in (False, True):
        xi = np.random.default_rng(K + 1).random(n1).astype(f32) if drawn else None
        got = _resample_abi(D, K, torch.from_numpy(fine_off).to(dev), None if xi is None else torch.from_numpy(xi).to(dev))
        ray_id, t1, dt1, pts = (g.cpu().numpy() for g in got)
        # every element of every hit ray's span written, the margin and nothing else untouched
        assert np.all(ray_id[n1:] == -1) and np.all(np.isnan(t1[n1:])) and np.all(np.isnan(dt1[n1:])) and np.all(np.isnan(pts[n1:]))
        ray_id, t1, dt1, pts = ray_id[:n1], t1[:n1], dt1[:n1], pts[:n1]
        _check_properties(w, ts, dt, ray_off, fine_off, ray_id, t1, dt1, K)            # finite, ray_id, inside an interval, order, dt' >= 0, sum
        assert np.array_equal(pts, (ro[ray_id] + rd[ray_id] * t1[:, None]).astype(f32))
        ra, rb, rB = rr.contract_ratios(w, ts, dt, ray_off, fine_off, t1, dt1, K, xi, 'wave')          # the kernel's order: the tight (b)
        print(f"kernel K={K} drawn={drawn}: largest error / bound (a) {ra:.3f}, (b) {rb:.3f}; (b) over (S+8) 2^-23 alone {rB:.2f}")
        assert ra <= 1.0 and rb <= 1.0, (ra, rb)


def test_bad_weights_count_as_their_clamped_values_on_the_device(dev):
    """NaN, negative, infinite and > 1 weights, in the first chunk, at a chunk edge and deep in the 5000-sample ray: the kernel gives the
    bits it gives for the clamped weights."""
    w, ts, dt, ray_off, ro, rd = _host_lists()
    bad = w.copy()
    off = ray_off.tolist()
    for r in (2, 4, 6, 8):                                                                # counts 2, 64, 130, 5000
        S = off[r + 1] - off[r]
        for j, v in ((0, np.nan), (S - 1, -3.0), (S // 2, np.inf), (S // 3, 7.5), (min(S - 1, 64), -np.inf), (min(S - 1, 63), np.nan)):
            bad[off[r] + j] = v
    want = rr.clamped(bad)
    assert np.isnan(bad).sum() >= 6 and np.all(np.isfinite(want)) and not np.array_equal(want, rr.clamped(w))
    K = 65
    fine_off = torch.from_numpy(_fine_off(COUNTS, K)).to(dev)
    D_bad = OG._dev(dev, bad, ts, dt, ray_off, ro, rd)
    D_ref = OG._dev(dev, want, ts, dt, ray_off, ro, rd)
    xi = torch.rand(int(fine_off[-1]), device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    for x in (None, xi):
        got, ref = _resample_abi(D_bad, K, fine_off, x), _resample_abi(D_ref, K, fine_off, x)
        n1 = int(fine_off[-1])
        assert all(torch.equal(a, b) for a, b in zip(got, ref) if a.dtype == torch.int32)
        assert all(torch.equal(a[:n1], b[:n1]) and bool(torch.isfinite(a[:n1]).all()) for a, b in zip(got[1:], ref[1:]))


def test_march_starts_are_t_minus_u_dt(dev):
    """march(starts=True): ts = t - u*dt with the u the march itself drew (a seeded generator regenerates it), 0.5 without jitter; the
    restatement gives the same bits; inside a run the next start is this start plus the width, to the rounding of the three binary32
    expressions that form them (a + (j+u)*dt, u*dt, the difference: four ulps of t)."""
    grid = _shell_grid(dev)
    ro, rd, _ = OG._dev(dev, *OC.random_rays(np.random.default_rng(8), 120, 4))
    step = float(grid.h[0]) / 2
    for perturb in (False, True):
        ray_off, ray_id, t, dt, pts, ts = grid.march(ro, rd, NEAR, FAR, step, perturb=perturb, starts=True,
                                                     generator=torch.Generator(device=dev).manual_seed(11))
        n = t.numel()
        assert n > 100
        u = torch.rand(n, device=dev, generator=torch.Generator(device=dev).manual_seed(11)) if perturb else None
        assert torch.equal(ts, t - (u if perturb else 0.5) * dt)
        assert np.array_equal(ts.cpu().numpy(), rr.starts_np(t.cpu().numpy(), dt.cpu().numpy(), None if u is None else u.cpu().numpy()))
        if perturb:
            assert not torch.equal(ts, t - 0.5 * dt)
        same_run = (ray_id[1:] == ray_id[:-1]) & (dt[1:] == dt[:-1])                   # neighbours of one run share its width
        gap = (ts[1:] - (ts[:-1] + dt[:-1])).abs()
        ulp = torch.from_numpy(np.spacing(t.cpu().numpy()[1:])).to(dev)
        near = same_run & (gap <= 0.25 * dt[1:])                                       # two runs of equal width are a gap apart, not ulps
        assert int(near.sum()) > n // 2 and bool((gap[near] <= 4 * ulp[near]).all()), float((gap[near] / ulp[near]).max())


# ---- 2. one summation order: alone, repeated, on a side stream --------------------------------------------------------------------------------
def test_every_ray_alone_repeat_and_side_stream_give_equal_bits(dev):
    host = _host_lists()
    D = OG._dev(dev, *host)
    w, ts, dt, ray_off, ro, rd = D
    K = 65
    fine_off = torch.from_numpy(_fine_off(COUNTS, K)).to(dev)
    n1 = int(fine_off[-1])
    xi = torch.rand(n1, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    first = _resample_abi(D, K, fine_off, xi)
    again = _resample_abi(D, K, fine_off, xi)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _resample_abi(D, K, fine_off, xi)
    torch.cuda.current_stream().wait_stream(side)
    for got in (again, other):
        assert all(OG._eq(a, b) for a, b in zip(got, first))
    off, foff = ray_off.tolist(), fine_off.tolist()
    for r, S in enumerate(COUNTS):
        if S == 0:
            continue
        s, o = slice(off[r], off[r + 1]), slice(foff[r], foff[r + 1])
        one = (w[s], ts[s], dt[s], torch.tensor([0, S], dtype=torch.int64, device=dev), ro[r:r + 1], rd[r:r + 1])
        alone = _resample_abi(one, K, torch.tensor([0, K], dtype=torch.int64, device=dev), xi[o].contiguous())
        assert bool((alone[0][:K] == 0).all())
        assert all(torch.equal(a[:K], b[o]) for a, b in zip(alone[1:], first[1:])), r


# ---- 3. a ray never stores past its fine span --------------------------------------------------------------------------------------------------
def test_a_short_fine_span_is_all_that_is_stored(dev):
    counts = [19, 70, 0, 5]
    host = rr.make_lists(counts, seed=5)
    D = OG._dev(dev, *host)
    K = 16
    full_off = torch.from_numpy(_fine_off(counts, K)).to(dev)
    full = _resample_abi(D, K, full_off)
    short = torch.tensor([0, 16, 16 + 9, 16 + 9, 16 + 9 + 16], dtype=torch.int64, device=dev)      # ray 1 owns 9 entries, not 16
    got = _resample_abi(D, K, short)
    m = int(short[-1])
    assert bool((got[0][m:] == -1).all()) and bool(torch.isnan(got[1][m:]).all()) and bool(torch.isnan(got[3][m:]).all())
    assert got[0][:m].tolist() == [0] * 16 + [1] * 9 + [3] * 16
    for a, b in zip(got[1:], full[1:]):
        assert torch.equal(a[:16], b[:16]) and torch.equal(a[16:25], b[16:25]) and torch.equal(a[25:41], b[32:48])      # the heads of their own lists
    # a last span shorter than K, ending where the lists end
    cut = torch.tensor([0, 16, 32, 32, 40], dtype=torch.int64, device=dev)                         # the last ray owns 8 entries up to n_fine = 40
    got = _resample_abi(D, K, cut)
    assert bool((got[0][40:] == -1).all()) and bool(torch.isnan(got[1][40:]).all()) and torch.equal(got[1][32:40], full[1][32:40])


# ---- 4. render_rays_marched(resample=) is the composition of the public pieces ----------------------------------------------------------------
RESAMPLED_CASES = [(white, noise, perturb) for white in (False, True) for noise in (0.0, 1.0) for perturb in (0.0, 1.0)]


def _mse_grads(field, out, rgb0, target):
    field.zero_grad(set_to_none=True)
    (((out[0] - target) ** 2).mean() + ((rgb0 - target) ** 2).mean()).backward()
    grads = [p.grad.clone() for p in field._params()]
    assert len(grads) == 18 and all(torch.isfinite(g).all() for g in grads)
    return grads


@pytest.mark.parametrize("white,noise,perturb", RESAMPLED_CASES)
def test_render_rays_marched_resampled_equals_the_composition(dev, white, noise, perturb):
    from contexture_nerf_amd import run_nerf_helpers as rnh
    field = OG._field(dev)
    grid = _shell_grid(dev)
    R, K = 300, 8
    ro, rd, _ = OG._dev(dev, *OC.random_rays(np.random.default_rng(5), R, 4))
    target = torch.rand(R, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    step = float(grid.h[0])
    got, gx = rnh.render_rays(field, ro, rd, NEAR, FAR, 64, white_bkgd=white, perturb=perturb, raw_noise_std=noise, march=step, occupancy=grid,
                              generator=torch.Generator(device=dev).manual_seed(9), return_extras=True, resample=K)
    got_grads = _mse_grads(field, got, gx['rgb0'], target)
    gen = torch.Generator(device=dev).manual_seed(9)
    ray_off, ray_id, t, dt, pts, ts = grid.march(ro, rd, NEAR, FAR, step, perturb=perturb > 0, generator=gen, starts=True)
    plain = grid.march(ro, rd, NEAR, FAR, step, perturb=perturb > 0, generator=torch.Generator(device=dev).manual_seed(9))
    assert len(plain) == 5 and all(torch.equal(a, b) for a, b in zip(plain, (ray_off, ray_id, t, dt, pts)))          # starts= changes no bit
    n = t.numel()
    hit = int((ray_off[1:] > ray_off[:-1]).sum())
    assert 0 < hit < R and n > 0
    coarse = rnh.raw2outputs_packed(field.forward_pts(pts), t, dt, rd, ray_off, noise, white, gen)
    fine = rnh.resample_packed(coarse[3].detach(), ts, dt, ray_off, ro, rd, K, perturb=perturb > 0, generator=gen)
    want = rnh.raw2outputs_packed(field.forward_pts(fine[4]), fine[2], fine[3], rd, fine[0], noise, white, gen)
    want_grads = _mse_grads(field, want, coarse[0], target)
    assert sorted(gx) == sorted(['ray_off', 'ray_id', 't', 'dt', 'pts', 'ray_off0', 'ray_id0', 't0', 'dt0', 'pts0', 'rgb0', 'disp0', 'acc0',
                                 'weights0', 'depth0'])
    assert tuple(got[3].shape) == (K * hit,) and fine[0][-1].item() == K * hit
    for key, w in zip(('ray_off', 'ray_id', 't', 'dt', 'pts'), fine):
        assert torch.equal(gx[key], w), key
    for key, w in zip(('ray_off0', 'ray_id0', 't0', 'dt0', 'pts0'), (ray_off, ray_id, t, dt, pts)):
        assert torch.equal(gx[key], w), key
    for key, w in zip(('rgb0', 'disp0', 'acc0', 'weights0', 'depth0'), coarse):
        assert OG._eq(gx[key], w), key
    for a, b in zip(got, want):
        assert OG._eq(a, b)
    for k, (a, b) in enumerate(zip(got_grads, want_grads)):
        assert torch.equal(a, b), f"parameter gradient {k}"
    assert any(bool(x.any()) for x in got_grads) and 0 < float(got[2].detach().max())
    if perturb > 0:                                                                                 # xi was drawn: not the midpoints
        mid = rnh.resample_packed(coarse[3].detach(), ts, dt, ray_off, ro, rd, K)
        assert torch.equal(mid[0], fine[0]) and not torch.equal(mid[2], fine[2])


# ---- 5. quadrature: the fine widths conserve the occupied length -------------------------------------------------------------------------------
def test_resampled_quadrature_of_a_constant_density(dev):
    """Constant sigma0 inside the occupied cells: the fine pass gives acc = 1 - exp(-sigma0 * sum dt * |d|) of the COARSE widths, because
    the fine widths tile the same occupied length; a wrong dt' shows here."""
    from contexture_nerf_amd import run_nerf_helpers as rnh, volume_render as vr
    G, sigma0, R, far = 16, 3.0, 64, 4.0
    grid = vr.OccupancyGrid.from_mask(torch.from_numpy(OM.ball_mask(G, 0.6)).to(dev), -1.0, 1.0)
    ro, rd, _ = OG._dev(dev, *OC.random_rays(np.random.default_rng(12), R, 4, spread=0.5))
    field = _ConstField(sigma0, dev)
    nrm = np.linalg.norm(rd.cpu().numpy().astype(np.float64), axis=-1)
    for K, perturb in ((8, 0.0), (70, 1.0)):
        with torch.no_grad():
            out, ex = rnh.render_rays_marched(field, ro, rd, NEAR, far, grid, float(grid.h[0]) / 2, perturb=perturb, return_extras=True, resample=K,
                                              generator=torch.Generator(device=dev).manual_seed(1))
        length = np.bincount(ex['ray_id0'].cpu().numpy(), weights=ex['dt0'].cpu().numpy().astype(np.float64), minlength=R) * nrm
        want = 1.0 - np.exp(-sigma0 * length)
        acc = out[2].cpu().numpy().astype(np.float64)
        assert (length == 0).any() and 0.3 < want.max() < 0.999
        assert np.all(np.abs(acc - want) <= 2e-4 * np.abs(want) + 2e-6), np.abs(acc - want).max()
        assert bool((out[2] == 0)[torch.from_numpy(length == 0).to(dev)].all())


# ---- 6. concentration: the fine samples go where the coarse weight is --------------------------------------------------------------------------
class _SlabField:
    """forward_pts -> a dense slab |z| < 0.06 across the rays, empty elsewhere."""

    def forward_pts(self, pts):
        raw = torch.zeros(pts.shape[0], 4, device=pts.device)
        raw[:, 3] = torch.where(pts[:, 2].abs() < 0.06, 200.0, -1.0)
        return raw


def test_fine_samples_concentrate_on_the_slab(dev):
    """The strata are equal in mass, so of a ray's K fine samples at least floor(K * (mass of the coarse intervals that carry the slab) / W)
    - 2 lie inside those intervals (they are neighbours in the list: one stretch of mass; one stratum is lost at each of its ends)."""
    from contexture_nerf_amd import run_nerf_helpers as rnh, volume_render as vr
    G, R, K = 16, 64, 32
    grid = vr.OccupancyGrid.from_mask(torch.from_numpy(OM.ball_mask(G, 0.6)).to(dev), -1.0, 1.0)
    ro, rd, _ = OG._dev(dev, *OC.random_rays(np.random.default_rng(12), R, 4, spread=0.5))
    with torch.no_grad():
        out, ex = rnh.render_rays_marched(_SlabField(), ro, rd, NEAR, 4.0, grid, float(grid.h[0]) / 2, return_extras=True, resample=K)
    off0, off1 = ex['ray_off0'].tolist(), ex['ray_off'].tolist()
    w0, t0, dt0 = (ex[k].detach().cpu().numpy() for k in ('weights0', 't0', 'dt0'))
    ts0 = (t0 - f32(0.5) * dt0).astype(f32)
    slab = np.abs(ex['pts0'].cpu().numpy()[:, 2]) < 0.06
    t1 = ex['t'].cpu().numpy()
    checked = 0
    for r in range(R):
        s, o = slice(off0[r], off0[r + 1]), slice(off1[r], off1[r + 1])
        if not slab[s].any():
            continue
        idx = np.nonzero(slab[s])[0]
        assert np.array_equal(idx, np.arange(idx[0], idx[-1] + 1))                                  # one stretch of the list
        m = rr.masses64(w0[s])
        share = m[idx].sum() / m.sum()
        inside = rr.in_coarse_interval(ts0[s][idx], dt0[s][idx], t1[o]).sum()
        assert inside >= int(np.floor(K * share)) - 2, (r, inside, share)
        checked += share > 0.9
    assert checked >= 8                                                                             # rays whose weight sits in the slab


# ---- 7. resample=0 is the present path ------------------------------------------------------------------------------------------------------------
def test_resample_zero_is_the_call_without_the_keyword(dev):
    from contexture_nerf_amd import run_nerf_helpers as rnh
    field = OG._field(dev)
    grid = _shell_grid(dev)
    ro, rd, _ = OG._dev(dev, *OC.random_rays(np.random.default_rng(8), 33, 4))
    kw = dict(white_bkgd=True, perturb=1., raw_noise_std=1., march=float(grid.h[0]) / 2, occupancy=grid, return_extras=True)
    a, ax = rnh.render_rays(field, ro, rd, NEAR, FAR, 64, generator=torch.Generator(device=dev).manual_seed(4), **kw)
    b, bx = rnh.render_rays(field, ro, rd, NEAR, FAR, 64, generator=torch.Generator(device=dev).manual_seed(4), resample=0, **kw)
    assert sorted(ax) == sorted(bx) == ['dt', 'pts', 'ray_id', 'ray_off', 't']
    assert all(OG._eq(x, y) for x, y in zip(a, b)) and all(torch.equal(ax[k], bx[k]) for k in ax)
    assert len(grid.march(ro, rd, NEAR, FAR, 0.1)) == 5 and len(grid.march(ro, rd, NEAR, FAR, 0.1, starts=True)) == 6


# ---- 8. an empty grid ---------------------------------------------------------------------------------------------------------------------------
def test_resampled_with_an_empty_grid(dev):
    from contexture_nerf_amd import run_nerf_helpers as rnh, volume_render as vr
    field = OG._field(dev)
    grid = vr.OccupancyGrid.from_mask(torch.zeros(8, 8, 8, dtype=torch.bool, device=dev), -1.0, 1.0)
    R = 9
    ro, rd, _ = OG._dev(dev, *OC.random_rays(np.random.default_rng(1), R, 4))
    calls = []
    orig = field.forward_pts
    field.forward_pts = lambda pts: calls.append(1) or orig(pts)
    for white in (False, True):
        out, ex = rnh.render_rays_marched(field, ro, rd, NEAR, FAR, grid, 0.125, white_bkgd=white, return_extras=True, resample=8)
        for sfx in ('', '0'):
            assert ex['t' + sfx].numel() == 0 and tuple(ex['pts' + sfx].shape) == (0, 3) and ex['ray_off' + sfx].tolist() == [0] * (R + 1)
        assert bool((out[2] == 0).all()) and bool((out[4] == 0).all()) and bool(torch.isnan(out[1]).all()) and out[3].numel() == 0
        assert bool((out[0] == (1.0 if white else 0.0)).all()) and not out[0].requires_grad and not ex['rgb0'].requires_grad
    before = [p.detach().clone() for p in field.parameters()]
    opt = torch.optim.Adam(field.parameters(), lr=1e-2)
    step = vr.train_step(field, opt, ro, rd, torch.rand(R, 3, device=dev), NEAR, FAR, 64, occupancy=grid, march=0.125, resample=8)
    assert torch.isfinite(step['loss']) and torch.isfinite(step['psnr'])
    assert all(torch.equal(a, b) for a, b in zip(before, field.parameters())) and not calls          # untouched; the field never ran
    del field.forward_pts


# ---- 9 .. 11. training and rendering through the fine pass ---------------------------------------------------------------------------------------
def test_train_step_resampled_with_distortion(dev):
    from contexture_nerf_amd import volume_render as vr
    field = OG._field(dev)
    grid = _shell_grid(dev)
    R = 128
    ro, rd, _ = OG._dev(dev, *OC.random_rays(np.random.default_rng(3), R, 4))
    before = [p.detach().clone() for p in field.parameters()]
    opt = torch.optim.Adam(field.parameters(), lr=1e-3)
    res = vr.train_step(field, opt, ro, rd, torch.rand(R, 3, device=dev), NEAR, FAR, 0, occupancy=grid, march=float(grid.h[0]), resample=8,
                        distortion=0.01, generator=torch.Generator(device=dev).manual_seed(2))
    assert sorted(res) == ['distortion', 'loss', 'psnr'] and all(bool(torch.isfinite(res[k])) for k in res)
    assert float(res['distortion']) > 0 and any(not torch.equal(a, b) for a, b in zip(before, field.parameters()))


def test_fit_views_resampled(dev):
    """The toy scene of test_march_gpu.test_fit_views_marched with the student marched at h and 8 fine samples per hit ray."""
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
                            occupancy_every=0, march=float(grid.h[0]), resample=8)
        assert torch.equal(grid.cells, before) and not bool(grid.dens.any()) and 0 < grid.fraction() < 1       # the grid is as it was
        return hist
    a, b = fit(), fit()
    print(f"fit_views marched at h, resample 8: loss first 5 {np.mean(a[:5]):.4f}, last 5 {np.mean(a[-5:]):.4f}")
    assert len(a) == 40 and all(np.isfinite(a)) and a == b
    assert np.mean(a[-5:]) < np.mean(a[:5])


def test_render_image_resampled(dev):
    from contexture_nerf_amd import run_nerf_helpers as rnh, volume_render as vr
    field = OG._field(dev, sigma_bias=8.0)
    v, f = OM.icosphere(2, 0.3)
    grid = vr.OccupancyGrid.from_mesh(*OG._dev(dev, v, f), 16, -1.0, 1.0, dilate=1)
    K = vr.pinhole(24, 24)
    c2w = torch.tensor([[1., 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1.5]], device=dev)
    step = float(grid.h[0])
    img = vr.render_image(field, 24, 24, K, c2w, NEAR, FAR, 0, white_bkgd=True, occupancy=grid, march=step, resample=16)
    ro, rd = rnh.get_rays(24, 24, K, c2w)
    with torch.no_grad():
        rgb, disp, acc, wts, depth = rnh.render_rays(field, ro.reshape(-1, 3), rd.reshape(-1, 3), NEAR, FAR, 0, white_bkgd=True, occupancy=grid,
                                                     march=step, resample=16)
    assert torch.equal(img['rgb'], rgb.reshape(24, 24, 3)) and torch.equal(img['acc'], acc.reshape(24, 24))
    assert torch.equal(img['depth'], depth.reshape(24, 24)) and OG._eq(img['disp'], disp.reshape(24, 24))
    plain = vr.render_image(field, 24, 24, K, c2w, NEAR, FAR, 0, white_bkgd=True, occupancy=grid, march=step)
    empty = plain['acc'] == 0
    assert bool(empty[0, 0]) and not bool(empty[12, 12]) and float(img['acc'][12, 12]) > 0.5 and wts.numel() == 16 * int((~empty).sum())
    assert bool((img['acc'][empty] == 0).all()) and bool((img['rgb'][empty] == 1).all()) and not torch.equal(img['rgb'], plain['rgb'])
