"""GPU: the occupancy grid voxelised from a mesh and the per-ray spans — ctx_occ_voxelize / ctx_occ_dilate / ctx_occ_ray_spans against the
numpy restatements of test_occupancy_mesh_cpu.py (array_equal), OccupancyGrid.from_mesh as their composition, and the bit contract of
render_rays(clip=True): it equals render_rays(z_vals=z) with z built in torch from the restatement's spans.  No tolerance in this file."""
import numpy as np
import pytest
import torch

import test_occupancy_cpu as OC
import test_occupancy_mesh_cpu as OM
import test_occupancy_gpu as OG

pytestmark = pytest.mark.gpu

f32 = np.float32


def _vox(dev, v, f, G, lo=-1.0, hi=1.0, cells=None):
    """ctx_occ_voxelize on the raw entry point -> (cells on the device, the restatement's cells)."""
    from contexture_nerf_amd import _lib as L
    lo3, inv, _ = OC.grid_consts(G, lo, hi)
    v, f = np.ascontiguousarray(v, f32).reshape(-1, 3), np.ascontiguousarray(f, np.int64).reshape(-1, 3)
    want = OM.occ_voxelize_np(v, f, G, lo3, inv, None if cells is None else cells.cpu().numpy().copy())
    t_v, t_f = OG._dev(dev, v, f)
    if cells is None:
        cells = torch.zeros(G, G, G, dtype=torch.uint8, device=dev)
    L.check(L.load().ctx_occ_voxelize(L.ptr(t_v, torch.float32), L.ptr(t_f, torch.int64), len(v), len(f), G, *map(float, lo3), *map(float, inv),
                                      L.ptr(cells, torch.uint8), L.stream()))
    return cells, want


# ---- the voxeliser ------------------------------------------------------------------------------------------------------------------------
def test_voxelize_hand_cases(dev):
    G = 8
    lo3, inv, h = OC.grid_consts(G, -1.0, 1.0)
    w = lambda g: (lo3 + np.asarray(g, f32) * h).astype(f32)
    line = w([[1.5, 1.5, 1.5], [2.5, 2.5, 1.5], [3.5, 3.5, 1.5]])
    bad = np.concatenate([line, f32([[np.nan, 0, 0], [np.inf, 0, 0]])])
    cases = [(w([[2.3, 5.2, 1.4], [2.7, 5.3, 1.5], [2.4, 5.8, 1.7]]), [[0, 1, 2]], G, 1),           # inside one cell
             (line, [[0, 1, 2]], G, 9), (line, [[1, 1, 1]], G, 1),                                    # degenerate: the candidates
             (bad, [[0, 1, 3]], G, 0), (bad, [[0, 4, 2]], G, 0), (bad, [[0, 1, 5]], G, 0), (bad, [[-1, 1, 2]], G, 0),
             (bad, [[0, 1, 5], [0, 1, 2], [3, 3, 3]], G, 9),                                          # the bad ones disturb no other
             (w([[2.2, 2.2, 3.0], [2.8, 2.2, 3.0], [2.2, 2.8, 3.0]]), [[0, 1, 2]], G, 2),             # on a cell face: both layers
             (w([[9.5, 1, 1], [10.5, 1, 2], [9.5, 2, 1]]), [[0, 1, 2]], G, 0),                        # outside the grid
             (f32([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0]]), [[0, 1, 2]], 1, 1),
             (f32([[-5, -5, 0], [5, -5, 0], [0, 7, 0]]), [[0, 1, 2]], 1, 1),
             (f32([[3, 0, 0], [3.5, 0, 0], [3, 0.5, 0]]), [[0, 1, 2]], 1, 0)]
    for k, (v, f, g, count) in enumerate(cases):
        got, want = _vox(dev, v, f, g)
        assert np.array_equal(got.cpu().numpy(), want) and int(want.sum()) == count, k


@pytest.mark.parametrize("G", [1, 4, 16, 64])
def test_voxelize_random_triangles_vs_restatement(dev, G):
    """300 triangles: 110 sub-cell, 100 several cells across, 20 reaching outside the grid (each has up to G^3 candidates), 70 lying
    exactly on a cell face."""
    rng = np.random.default_rng(100 + G)
    tri = np.concatenate([OM.random_triangles(rng, G, n, kind) for n, kind in zip((110, 100, 20, 70), OM.KINDS)])
    v, f = OM.triangles_to_mesh(tri, G)
    got, want = _vox(dev, v, f, G)
    assert np.array_equal(got.cpu().numpy(), want) and want.any()
    if G == 16:                                                      # one at a time: each kind alone, so no union hides a miss
        for k in range(0, 300, 15):
            got, want = _vox(dev, v, f[k:k + 1], G)
            assert np.array_equal(got.cpu().numpy(), want), k


def test_voxelize_spot(dev):
    v, f = OM.spot_mesh()
    got, want = _vox(dev, v, f, 64)
    assert np.array_equal(got.cpu().numpy(), want) and 0.003 < want.mean() < 0.05


def test_voxelize_face_counts_union_and_giant(dev):
    G = 16
    rng = np.random.default_rng(7)
    # F = 1, F below one block's four waves, and F = 8195: three more than the 2048 blocks x 4 waves of the capped launch
    for F in (1, 7, 8195):
        v, f = OM.triangles_to_mesh(OM.random_triangles(rng, G, F, "small"), G)
        got, want = _vox(dev, v, f, G)
        assert np.array_equal(got.cpu().numpy(), want), F
    # a second call accumulates the union, and clears nothing
    va, fa = OM.triangles_to_mesh(OM.random_triangles(rng, G, 5, "medium"), G)
    vb, fb = OM.triangles_to_mesh(OM.random_triangles(rng, G, 5, "on_face"), G)
    cells, want_a = _vox(dev, va, fa, G)
    cells[15, 15, 15] = 1
    cells, want_ab = _vox(dev, vb, fb, G, cells=cells)
    assert np.array_equal(cells.cpu().numpy(), want_ab) and want_ab[15, 15, 15] == 1 and np.all(want_ab >= want_a) and want_ab.sum() > want_a.sum() + 1
    # one giant triangle across a G = 64 grid: G^3 candidates for one wave, clipped to the grid on every side
    G = 64
    lo3, _, h = OC.grid_consts(G, -1.0, 1.0)
    v = (lo3 + f32([[-40.25, 10.5, -7.0], [130.0, 20.25, 50.5], [30.5, 90.0, 140.75]]) * h).astype(f32)
    got, want = _vox(dev, v, [[0, 1, 2]], G)
    assert np.array_equal(got.cpu().numpy(), want) and 2000 < want.sum() < 20000 and want[:, :, 0].any() and want[:, :, 63].any()


# ---- the dilation -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 5, 32])
def test_dilate_vs_restatement(dev, G):
    from contexture_nerf_amd import _lib as L
    lib = L.load()
    rng = np.random.default_rng(G)
    for density in (0.02, 0.5):
        cells = (rng.random((G, G, G)) < density).astype(np.uint8) * 5          # any non-zero byte is occupied
        cells[0, G - 1, G // 2] = 1
        src, = OG._dev(dev, cells)
        for k in (0, 1, 2, G):
            dst = torch.full((G, G, G), 7, dtype=torch.uint8, device=dev)
            ws = torch.full((G, G, G), 7, dtype=torch.uint8, device=dev)
            L.check(lib.ctx_occ_dilate(L.ptr(src), G, k, L.ptr(dst), L.ptr(ws) if k else None, L.stream()))
            assert np.array_equal(dst.cpu().numpy(), OM.occ_dilate_np(cells, k)), (density, k)
            assert np.array_equal(src.cpu().numpy(), cells)                       # the source is left alone
    grid_cells = (rng.random((G, G, G)) < 0.02).astype(np.uint8)
    from contexture_nerf_amd import volume_render as vr
    grid = vr.OccupancyGrid.from_mask(torch.from_numpy(grid_cells != 0).to(dev), -1.0, 1.0)
    grid.dilate(1)
    assert np.array_equal(grid.cells.cpu().numpy(), OM.occ_dilate_np(grid_cells, 1))


# ---- the spans ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 65, 300])
def test_ray_spans_vs_restatement(dev, R):
    from contexture_nerf_amd import volume_render as vr
    hits = 0
    for G, lo, hi in ((1, -1.0, 1.0), (4, -1.0, 1.0), (32, (-1.0, -0.5, -1.0), (1.0, 0.75, 0.5))):
        for density in (0.0, 0.05, 0.5, 1.0):
            rng = np.random.default_rng(1000 * R + G)
            ro, rd = OM.span_rays(rng, R)
            cells = (rng.random((G, G, G)) < density).astype(np.uint8)
            grid = vr.OccupancyGrid.from_mask(torch.from_numpy(cells != 0).to(dev), lo, hi)
            want_span, want_hit = OM.occ_ray_spans_np(ro, rd, 0.5, 2.5, cells, grid.lo, grid.hi, grid.inv, grid.h)
            span, hit = grid.ray_spans(*OG._dev(dev, ro, rd), 0.5, 2.5)
            assert span.dtype == torch.float32 and tuple(span.shape) == (R, 2) and hit.dtype == torch.bool
            assert np.array_equal(hit.cpu().numpy(), want_hit != 0), (G, density)
            assert np.array_equal(span.cpu().numpy(), want_span), (G, density)
            hits += int(want_hit.sum())
            if density == 0.0:
                assert not want_hit.any()
    assert hits > 0


# ---- from_mesh ------------------------------------------------------------------------------------------------------------------------------
def test_from_mesh_is_the_composition_and_thinner_than_the_ball(dev):
    from contexture_nerf_amd import volume_render as vr
    G = 32
    v, f = OM.icosphere(2, 0.6)
    lo3, inv, _ = OC.grid_consts(G, -1.0, 1.0)
    grid = vr.OccupancyGrid.from_mesh(*OG._dev(dev, v, f), G, -1.0, 1.0, dilate=1)
    surface = OM.occ_voxelize_np(v, f, G, lo3, inv)
    assert np.array_equal(grid.cells.cpu().numpy(), OM.occ_dilate_np(surface, 1)) and not bool(grid.dens.any())
    ball = vr.OccupancyGrid.from_mask(torch.from_numpy(OM.ball_mask(G, 0.6)).to(dev), -1.0, 1.0)
    ball.dilate(1)
    assert 0 < grid.fraction() < ball.fraction()
    # dilate=0 is the surface itself; voxelize on a grid unites with what is there
    bare = vr.OccupancyGrid.from_mesh(*OG._dev(dev, v, f), G, -1.0, 1.0, dilate=0)
    assert np.array_equal(bare.cells.cpu().numpy(), surface)
    ball.voxelize(*OG._dev(dev, v * f32(1.3), f), dilate=2)
    want = OM.occ_dilate_np(OM.ball_mask(G, 0.6).astype(np.uint8), 1) | OM.occ_dilate_np(OM.occ_voxelize_np(v * f32(1.3), f, G, lo3, inv), 2)
    assert np.array_equal(ball.cells.cpu().numpy(), want)


# ---- render_rays(clip=True) -------------------------------------------------------------------------------------------------------------------
def _shell_grid(dev, G=16):
    from contexture_nerf_amd import volume_render as vr
    v, f = OM.icosphere(2, 0.6)
    return vr.OccupancyGrid.from_mesh(*OG._dev(dev, v, f), G, -1.0, 1.0, dilate=1)


def _z_from_restatement(grid, ro, rd, near, far, S):
    span, hit = OM.occ_ray_spans_np(ro.cpu().numpy(), rd.cpu().numpy(), near, far, grid.cells.cpu().numpy(), grid.lo, grid.hi, grid.inv, grid.h)
    sp = torch.from_numpy(span).to(ro.device)
    t = torch.linspace(0., 1., steps=S, device=ro.device)
    return (sp[:, :1] * (1. - t) + sp[:, 1:] * t).contiguous(), span, hit


@pytest.mark.parametrize("N_importance", [0, 16])
def test_clip_equals_given_z_vals_from_the_restatement(dev, N_importance):
    from contexture_nerf_amd import run_nerf_helpers as rnh
    field = OG._field(dev)
    grid = _shell_grid(dev)
    R, S = 41, 64
    ro, rd, _ = OG._dev(dev, *OC.random_rays(np.random.default_rng(5), R, S))
    z, span, hit = _z_from_restatement(grid, ro, rd, 0.5, 2.5, S)
    assert 0 < hit.sum() < R and np.any(span[hit != 0, 1] - span[hit != 0, 0] < 1.0)          # rays that hit and rays that miss; narrowed spans
    kw = dict(perturb=0., N_importance=N_importance, return_extras=True, occupancy=grid)
    got, gx = rnh.render_rays(field, ro, rd, 0.5, 2.5, S, clip=True, **kw)
    got_grads = OG._backward_all(field, got, gx, seed=3)
    want, wx = rnh.render_rays(field, ro, rd, 0.5, 2.5, S, z_vals=z, **kw)
    want_grads = OG._backward_all(field, want, wx, seed=3)
    assert len(got) == 5 and tuple(got[3].shape) == (R, S + N_importance) and torch.equal(gx['z_vals'], wx['z_vals'])
    for a, b in zip(got, want):
        assert OG._eq(a, b)
    assert len(got_grads) == 18
    for k, (a, b) in enumerate(zip(got_grads, want_grads)):
        assert torch.equal(a, b), f"parameter gradient {k}"
    assert any(bool(x.any()) for x in got_grads) and 0 < float(got[2].detach().max())          # the case is not an empty one
    # clipping is visible: the unclipped samples of the same grid give another image
    plain = rnh.render_rays(field, ro, rd, 0.5, 2.5, S, perturb=0., N_importance=N_importance, occupancy=grid)
    assert not torch.equal(plain[0], got[0].detach())
    # a ray without a hit composites as empty space
    miss = torch.from_numpy(hit == 0).to(dev)
    assert bool((got[2].detach()[miss] == 0).all())


@pytest.mark.parametrize("N_importance", [0, 16])
def test_clip_with_an_all_ones_grid_over_everything_equals_no_clip(dev, N_importance):
    """The box -8 .. 8 holds [near, far] of every ray (|p| < 1.6 + 2.5 * |d|), so the slab clip leaves t_a = near and t_b = far and the
    walk, over occupied cells only, returns exactly (float32(near), float32(far)).  The z bits then agree with the dense expression
    near*(1-t) + far*t because torch multiplies a float32 tensor by a Python scalar in float32, and 0.5 and 2.5 are float32 numbers:
    span0*(1-t) + span1*t is the same three roundings per element."""
    from contexture_nerf_amd import run_nerf_helpers as rnh, volume_render as vr
    field = OG._field(dev)
    R, S = 41, 48
    ro, rd, _ = OG._dev(dev, *OC.random_rays(np.random.default_rng(6), R, S))
    grid = vr.OccupancyGrid(4, -8.0, 8.0, dev)
    span, hit = grid.ray_spans(ro, rd, 0.5, 2.5)
    assert bool(hit.all()) and bool((span == torch.tensor([0.5, 2.5], device=dev)).all())
    for perturb in (0., 1.):
        kw = dict(white_bkgd=True, perturb=perturb, raw_noise_std=1., N_importance=N_importance, return_extras=True, occupancy=grid)
        want, wx = rnh.render_rays(field, ro, rd, 0.5, 2.5, S, generator=torch.Generator(device=dev).manual_seed(1), **kw)
        got, gx = rnh.render_rays(field, ro, rd, 0.5, 2.5, S, generator=torch.Generator(device=dev).manual_seed(1), clip=True, **kw)
        assert all(OG._eq(a, b) for a, b in zip(got, want)) and torch.equal(gx['z_vals'], wx['z_vals'])


def test_clip_repeat_and_side_stream_give_equal_bits(dev):
    from contexture_nerf_amd import run_nerf_helpers as rnh
    field = OG._field(dev)
    grid = _shell_grid(dev)
    R, S = 33, 72
    ro, rd, _ = OG._dev(dev, *OC.random_rays(np.random.default_rng(8), R, S))

    def run():
        out, ex = rnh.render_rays(field, ro, rd, 0.5, 2.5, S, perturb=1., raw_noise_std=1., N_importance=16,
                                  generator=torch.Generator(device=dev).manual_seed(4), return_extras=True, occupancy=grid, clip=True)
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


# ---- fit_views with a static grid from the mesh ---------------------------------------------------------------------------------------------------
def test_fit_views_with_a_mesh_grid(dev):
    """The toy scene of test_occupancy_gpu.test_fit_views_with_a_grid: the teacher is a dense random field seen through a ball mask of
    radius 0.6.  The student's grid is the shell of the icosphere of that radius, static (occupancy_every=0), with clipped samples."""
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
        hist = vr.fit_views(student, imgs, c2ws, K, 0.5, 2.5, 40, rays_per_iter=256, seed=3, N_samples=S, N_importance=8, raw_noise_std=1.,
                            white_bkgd=True, occupancy=grid, occupancy_every=0, clip=True)
        assert torch.equal(grid.cells, before) and not bool(grid.dens.any()) and 0 < grid.fraction() < 1       # the grid is as it was
        return hist
    a, b = fit(), fit()
    print(f"fit_views with a mesh grid: loss first 5 {np.mean(a[:5]):.4f}, last 5 {np.mean(a[-5:]):.4f}")
    assert len(a) == 40 and all(np.isfinite(a)) and a == b
    assert np.mean(a[-5:]) < np.mean(a[:5])


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from contexture_nerf_amd import _lib as L, run_nerf_helpers as rnh, volume_render as vr
    lib = L.load()
    p = L.ptr
    err = lambda: lib.ctx_last_error().decode()
    G = 4
    v, f = OG._dev(dev, f32([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0]]), np.int64([[0, 1, 2]]))
    cells = torch.zeros(G, G, G, dtype=torch.uint8, device=dev)
    other, ws = torch.zeros_like(cells), torch.zeros_like(cells)
    ro, rd = OG._dev(dev, *OM.span_rays(np.random.default_rng(0), 4))
    span, hit = torch.zeros(4, 2, device=dev), torch.zeros(4, dtype=torch.uint8, device=dev)
    box = (-1.0, -1.0, -1.0, 2.0, 2.0, 2.0)
    box4 = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0, 0.5, 0.5, 0.5)
    for bad in (0, 257):
        assert lib.ctx_occ_voxelize(p(v), p(f), 3, 1, bad, *box, p(cells), L.stream()) != 0 and "outside [1, 256]" in err()
        assert lib.ctx_occ_dilate(p(cells), bad, 1, p(other), p(ws), L.stream()) != 0 and "outside [1, 256]" in err()
        assert lib.ctx_occ_ray_spans(p(ro), p(rd), 4, 0.5, 2.5, p(cells), bad, *box4, p(span), p(hit), L.stream()) != 0 and "outside [1, 256]" in err()
    assert lib.ctx_occ_voxelize(None, p(f), 3, 1, G, *box, p(cells), L.stream()) != 0 and "null" in err()
    assert lib.ctx_occ_voxelize(p(v), p(f), 3, 1, G, *box, None, L.stream()) != 0 and "null" in err()
    assert lib.ctx_occ_voxelize(p(v), p(f), 3, 0, G, *box, p(cells), L.stream()) != 0 and "at least one" in err()
    assert lib.ctx_occ_voxelize(p(v), p(f), 0, 1, G, *box, p(cells), L.stream()) != 0 and "at least one" in err()
    assert lib.ctx_occ_dilate(None, G, 1, p(other), p(ws), L.stream()) != 0 and "null" in err()
    assert lib.ctx_occ_dilate(p(cells), G, 1, p(cells), p(ws), L.stream()) != 0 and "must not be src" in err()
    assert lib.ctx_occ_dilate(p(cells), G, 1, p(other), None, L.stream()) != 0 and "workspace" in err()
    assert lib.ctx_occ_dilate(p(cells), G, 1, p(other), p(other), L.stream()) != 0 and "workspace" in err()
    assert lib.ctx_occ_dilate(p(cells), G, -1, p(other), p(ws), L.stream()) != 0 and "k >= 0" in err()
    assert lib.ctx_occ_ray_spans(p(ro), None, 4, 0.5, 2.5, p(cells), G, *box4, p(span), p(hit), L.stream()) != 0 and "null" in err()
    assert lib.ctx_occ_ray_spans(p(ro), p(rd), 0, 0.5, 2.5, p(cells), G, *box4, p(span), p(hit), L.stream()) != 0 and "outside [1, 2^31)" in err()
    for near, far in ((2.5, 0.5), (1.0, 1.0), (float('nan'), 1.0), (0.5, float('inf'))):
        assert lib.ctx_occ_ray_spans(p(ro), p(rd), 4, near, far, p(cells), G, *box4, p(span), p(hit), L.stream()) != 0 and "near < far" in err()
    assert not bool(cells.any()) and not bool(other.any()) and not bool(span.any())          # no refused call launched anything
    # the host side
    grid = vr.OccupancyGrid(G, -1.0, 1.0, dev)
    field = OG._field(dev)
    with pytest.raises(L.CtxError, match="clip=True needs an occupancy grid"):
        rnh.render_rays(field, ro, rd, 0.5, 2.5, 8, clip=True)
    with pytest.raises(L.CtxError, match="clip=True places the samples itself"):
        rnh.render_rays(field, ro, rd, 0.5, 2.5, 8, z_vals=torch.ones(4, 8, device=dev), occupancy=grid, clip=True)
    with pytest.raises(L.CtxError, match="device tensor"):
        vr.OccupancyGrid.from_mesh(v.cpu(), f.cpu(), G, -1.0, 1.0)
    with pytest.raises(L.CtxError, match=r"faces int64 \[F,3\]"):
        vr.OccupancyGrid.from_mesh(v, f.int(), G, -1.0, 1.0)
    with pytest.raises(L.CtxError, match=r"vertices float32 \[V,3\]"):
        grid.voxelize(v.double(), f)
    with pytest.raises(L.CtxError, match="no face"):
        vr.OccupancyGrid.from_mesh(v, f[:0], G, -1.0, 1.0)
    with pytest.raises(L.CtxError, match="dilate=-2"):
        vr.OccupancyGrid.from_mesh(v, f, G, -1.0, 1.0, dilate=-2)
    with pytest.raises(L.CtxError, match="near < far"):
        grid.ray_spans(ro, rd, 2.5, 0.5)
    with pytest.raises(L.CtxError, match="dtype"):
        grid.ray_spans(ro.double(), rd.double(), 0.5, 2.5)
    assert bool(grid.cells.all())                                                        # and the grid is as it was
