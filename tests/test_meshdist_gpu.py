"""GPU: the point / mesh query (csrc/meshdist.hip) against tests/meshdist_rule.py, and the two fields built on it.

1. ctx_mesh_closest_point on the raw entry point == the grid form of the rule, array_equal on found, dist, face and uv, outputs between
   guards and pre-filled: the CPU scenes at r = 0.5, 1.5 and 3 min(h), spot at G = 32, n in {1, 63, 65}, a batch past the capped launch
   against the same points in chunks, 1500 triangles in one cell, spoilt faces; n = 0 and the refusals;
2. MeshTracer.closest: dtypes, shapes, barycentrics, no gradient, refusals by name;
3. MeshDensityField: the tent bit for bit, colour untouched, no gradient to the density row, a view-dependent inner, fit_views repeats and
   falls, opaque walls;
4. AtlasField on a square with a linear ramp for an atlas.
No tolerance except AtlasField's colour (its docstring)."""
import numpy as np
import pytest
import torch

import meshdist_rule as R
import test_meshdist_cpu as MC
from test_engine_ops_gpu import Out

pytestmark = pytest.mark.gpu
f32 = np.float32
_TRACERS = {}


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def tracer_of(dev, name, mesh=None):
    """The MeshTracer of a CPU scene (or of `mesh` = (v, f) on that scene's grid), built once."""
    if name not in _TRACERS:
        from contexture_nerf_amd import volume_render as vr
        base = name.split("+")[0]
        if base == "spot":
            import test_meshhit_gpu as MH
            _TRACERS[name] = MH.scene(dev, "spot")[0]                 # one voxelisation of spot per session, on either side
        else:
            sc = MC.scene(base)
            v, f = (sc['v'], sc['f']) if mesh is None else mesh
            _TRACERS[name] = vr.MeshTracer(_t(dev, v), _t(dev, f), sc['G'], -1.0, 1.0)
    return _TRACERS[name]


def _raw(dev, tracer, pts, r, fill=0xFF):
    """ctx_mesh_closest_point on the raw entry point into guarded outputs pre-filled with 0xFF -> numpy (found, dist, face, uv)."""
    from contexture_nerf_amd import _lib as L
    n = len(pts)
    found, dist = Out(dev, (n,), torch.uint8, fill), Out(dev, (n,), torch.float32, fill)
    face, uv = Out(dev, (n,), torch.int32, fill), Out(dev, (n, 2), torch.float32, fill)
    p = _t(dev, pts)
    L.check(L.load().ctx_mesh_closest_point(L.ptr(p), n, float(r), tracer.G, *map(float, tracer.lo), *map(float, tracer.inv), L.ptr(tracer.cell_off),
                                            L.ptr(tracer.cell_tri), tracer.cell_tri.numel(), L.ptr(tracer.tri), tracer.tri.shape[0], L.ptr(found.t),
                                            L.ptr(dist.t), L.ptr(face.t), L.ptr(uv.t), L.stream()))
    return found.cpu("found").numpy(), dist.cpu("dist").numpy(), face.cpu("face").numpy(), uv.cpu("uv").numpy()


def _same(got, want, tag):
    for what, a, b in zip(MC.NAMES, got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (tag, what, a.dtype, b.dtype)
        assert np.array_equal(a, b), (tag, what, np.flatnonzero((a != b).reshape(len(a), -1).any(1))[:10])


# ---- 1. the raw entry point ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mult", MC.RADII)
@pytest.mark.parametrize("name", MC.SCENES)
def test_raw_vs_rule(dev, name, mult):
    """2300 points per case; r = 3 min(h) is the 7^3 block."""
    c = MC.case(name, mult)
    tracer = tracer_of(dev, name)
    assert np.array_equal(tracer.cell_tri.cpu().numpy(), MC.scene(name)['lists'][2])
    _same(_raw(dev, tracer, c['pts'], c['r']), c['grid'], (name, mult))
    assert 0 < c['grid'][0].sum() < len(c['pts'])


@pytest.mark.parametrize("n", [1, 63, 65])
def test_raw_small_batches(dev, n):
    c = MC.case("ico", 1.5)
    pick = np.arange(n) * 7 + 3
    _same(_raw(dev, tracer_of(dev, "ico"), c['pts'][pick], c['r']), [x[pick] for x in c['grid']], n)


def _spot_points(n, r, seed):
    v, _ = R.spot_mesh()
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    p = v[rng.integers(0, len(v), n)] + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0, 2 * r, (n, 1))
    return p.astype(f32)


def test_raw_spot(dev):
    import test_meshhit_gpu as MH
    tracer, v, f, lists, tri = MH.scene(dev, "spot")
    r = f32(1.5) * np.min(tracer.h)
    pts = _spot_points(4096, float(r), 5)
    want = R.closest_grid_np(pts, r, lists, tri, tracer.G, tracer.lo, tracer.inv)
    _same(_raw(dev, tracer, pts, r), want, "spot")
    assert 1000 < want[0].sum() < 4000 and len(set(want[2].tolist())) > 500


def test_large_batch_equals_chunks(dev):
    """n = 2048 * 256 + 3: three points more than one pass of the capped grid.  Against the same points in chunks, and the rule on 300."""
    import test_meshhit_gpu as MH
    tracer, v, f, lists, tri = MH.scene(dev, "spot")
    n = 2048 * 256 + 3
    r = f32(0.75) * np.min(tracer.h)
    pts = _spot_points(n, float(r), 6)
    p = _t(dev, pts)
    whole = tracer.closest(p, r)
    cut = [0, 1, 70000, 70001 + 256 * 1024, n]
    parts = [tracer.closest(p[a:b].contiguous(), r) for a, b in zip(cut[:-1], cut[1:])]
    for j in range(4):
        assert torch.equal(whole[j], torch.cat([q[j] for q in parts]))
    assert 0 < int(whole[0].sum()) < n
    pick = np.concatenate([np.arange(100), n // 2 + np.arange(100), n - 100 + np.arange(100)])
    want = R.closest_grid_np(pts[pick], r, lists, tri, tracer.G, tracer.lo, tracer.inv)
    assert np.array_equal(whole[0].cpu().numpy()[pick], want[0]) and np.array_equal(whole[1].cpu().numpy()[pick], want[1])
    assert np.array_equal(whole[2].cpu().numpy()[pick], want[2])


def test_long_list_in_one_cell(dev):
    """1500 sub-cell triangles inside one cell of a G = 4 grid: a list longer than a wave and longer than 1024."""
    from contexture_nerf_amd import volume_render as vr
    G = 4
    rng = np.random.default_rng(8)
    tri_grid = np.round((1.0 + rng.uniform(0.1, 0.9, (1500, 3, 3))) * 1024) / 1024
    v, f = R.triangles_to_mesh(tri_grid, G)
    lo, inv, h = R.grid_consts(G, -1.0, 1.0)
    lists, tri = R.mesh_cells_np(v, f, G, lo, inv), R.tri_records_np(v, f)
    assert lists[0].max() == 1500 and (lists[0] > 0).sum() == 1
    tracer = vr.MeshTracer(_t(dev, v), _t(dev, f), G, -1.0, 1.0)
    pts = (lo + rng.uniform(0.5, 2.5, (200, 3)) * h).astype(f32)     # in and around the cell (1, 1, 1)
    for mult in (0.5, 3.0):
        r = f32(mult) * h.min()
        want = R.closest_grid_np(pts, r, lists, tri, G, lo, inv)
        _same(_raw(dev, tracer, pts, r), want, ("long", mult))
        assert want[0].sum() > 50


def test_spoilt_faces_never_come_back(dev):
    v, f, bad = MC.broken_mesh()
    sc = MC.scene("tri4")
    tracer = tracer_of(dev, "tri4+broken", (v, f))
    c = MC.case("tri4", 1.5)
    centre = sc['v'][sc['f'][list(bad)]].mean(1)
    pts = np.concatenate([centre, c['pts'][:500]]).astype(f32)
    want = R.closest_grid_np(pts, c['r'], R.mesh_cells_np(v, f, sc['G'], sc['lo'], sc['inv']), R.tri_records_np(v, f), sc['G'], sc['lo'], sc['inv'])
    got = _raw(dev, tracer, pts, c['r'])
    _same(got, want, "spoilt")
    assert not set(got[2].tolist()) & set(bad) and got[0].sum() > 100
    # the whole lists of the unspoilt mesh with the spoilt records: the NaN records stop them; and list entries outside [0, F)
    from contexture_nerf_amd import _lib as L
    good = tracer_of(dev, "tri4")
    wild = sc['lists'][2].copy()
    wild[::7], wild[3::11] = -1, len(f)
    want = R.closest_grid_np(pts, c['r'], (sc['lists'][0], sc['lists'][1], wild), R.tri_records_np(v, f), sc['G'], sc['lo'], sc['inv'])

    class Mixed:
        G, lo, inv, cell_off, cell_tri, tri = good.G, good.lo, good.inv, good.cell_off, _t(dev, wild), tracer.tri
    got = _raw(dev, Mixed, pts, c['r'])
    _same(got, want, "stale lists")
    assert not set(got[2].tolist()) & set(bad)


def test_refusals_and_empty_batch(dev):
    from contexture_nerf_amd import _lib as L
    lib = L.load()
    tracer = tracer_of(dev, "ico")
    c = MC.case("ico", 1.5)
    pts = _t(dev, c['pts'][:4])
    found, dist = Out(dev, (4,), torch.uint8, 0xA5), Out(dev, (4,), torch.float32, 0xA5)
    face, uv = Out(dev, (4,), torch.int32, 0xA5), Out(dev, (4, 2), torch.float32, 0xA5)
    hmin = float(np.min(tracer.h))
    good = [L.ptr(pts), 4, float(c['r']), tracer.G, *map(float, tracer.lo), *map(float, tracer.inv), L.ptr(tracer.cell_off), L.ptr(tracer.cell_tri),
            tracer.cell_tri.numel(), L.ptr(tracer.tri), tracer.tri.shape[0], L.ptr(found.t), L.ptr(dist.t), L.ptr(face.t), L.ptr(uv.t), L.stream()]
    cases = [({k: None}, "null") for k in (0, 10, 11, 13, 15, 16, 17, 18)]
    cases += [({1: -1}, "n="), ({1: 2 ** 31}, "n="), ({12: -1}, "n_list="), ({12: 2 ** 31}, "n_list="), ({3: 0}, "outside [1, 256]"),
              ({3: 257}, "outside [1, 256]"), ({14: 0}, "F="), ({2: 0.0}, "radius > 0"), ({2: -1.0}, "radius > 0"), ({2: float('nan')}, "radius > 0"),
              ({2: float('inf')}, "radius > 0"), ({2: 3.01 * hmin}, "larger than 3 cells"), ({13: tracer.tri.data_ptr() + 4}, "aligned"),
              ({18: uv.t.data_ptr() + 4}, "aligned")]
    for change, needle in cases:
        a = list(good)
        for k, val in change.items():
            a[k] = val
        rc = lib.ctx_mesh_closest_point(*a)
        assert rc == -1 and needle.encode() in lib.ctx_last_error(), (change, rc, lib.ctx_last_error())
    a = list(good); a[1] = 0
    assert lib.ctx_mesh_closest_point(*a) == 0                          # n = 0 launches nothing
    a = list(good); a[1] = 0; a[0] = a[15] = None
    assert lib.ctx_mesh_closest_point(*a) == 0                          # and looks at no pointer
    for x in (found, dist, face, uv):
        x.untouched("mesh_closest_point")
    a = list(good); a[2] = 3.0 * hmin                                   # the limit itself passes
    assert lib.ctx_mesh_closest_point(*a) == 0
    assert found.cpu("found").max() <= 1


# ---- 2. MeshTracer.closest ------------------------------------------------------------------------------------------------------------------
def test_closest_wrapper(dev):
    from contexture_nerf_amd import _lib as L
    tracer = tracer_of(dev, "ico")
    c = MC.case("ico", 3.0)
    pts = _t(dev, c['pts'])
    found, dist, face, bary = tracer.closest(pts, c['r'])
    assert (found.dtype, dist.dtype, face.dtype, bary.dtype) == (torch.uint8, torch.float32, torch.int64, torch.float32)
    n = len(c['pts'])
    assert [tuple(x.shape) for x in (found, dist, face, bary)] == [(n,), (n,), (n,), (n, 3)]
    want = c['grid']
    assert np.array_equal(found.cpu().numpy(), want[0]) and np.array_equal(dist.cpu().numpy(), want[1]) and np.array_equal(face.cpu().numpy(), want[2])
    u, v = want[3][:, 0], want[3][:, 1]
    assert np.array_equal(bary.cpu().numpy(), np.stack([f32(1) - u - v, u, v], 1) * want[0][:, None].astype(f32))
    rows = bary.sum(1).cpu().numpy()
    assert np.all(rows[want[0] == 0] == 0) and np.all(np.abs(rows[want[0] == 1] - 1) < 1e-6) and not bary[found == 0].any()
    assert not any(x.requires_grad for x in (found, dist, face, bary))
    empty = tracer.closest(pts[:0], c['r'])
    assert [tuple(x.shape) for x in empty] == [(0,), (0,), (0,), (0, 3)] and empty[2].dtype == torch.int64
    with pytest.raises(L.CtxError, match="requires grad"):
        tracer.closest(pts.clone().requires_grad_(), c['r'])
    hmin = float(np.min(tracer.h))
    for bad in (0.0, -0.1, float('nan'), float('inf'), 3.01 * hmin):
        with pytest.raises(L.CtxError, match="max_dist"):
            tracer.closest(pts, bad)
    tracer.closest(pts[:8].contiguous(), 3 * np.min(tracer.h))
    with pytest.raises(L.CtxError, match=r"pts \[n,3\]"):
        tracer.closest(pts.reshape(-1), c['r'])
    with pytest.raises(L.CtxError, match="dtype"):
        tracer.closest(pts.double(), c['r'])
    with pytest.raises(L.CtxError, match="device tensor"):
        tracer.closest(pts.cpu(), c['r'])


# ---- 3. MeshDensityField --------------------------------------------------------------------------------------------------------------------
def _student(dev, tracer, seed=2):
    from contexture_nerf_amd import volume_render as vr
    from contexture_nerf_amd.hashgrid import HashGridField
    torch.manual_seed(seed)
    inner = HashGridField(tracer.lo, tracer.hi, n_levels=8, n_features=2, log2_table=12, base_res=4, max_res=64).to(dev)
    return vr.MeshDensityField(inner, tracer)


def test_density_is_the_tent_and_colour_is_inners(dev):
    from contexture_nerf_amd import _lib as L, volume_render as vr
    tracer = tracer_of(dev, "ico")
    field = _student(dev, tracer)
    width, peak = R.tent_defaults(tracer.h)
    assert field.width == width and field.peak == peak and float(peak) * float(width) == 16.0 and not field.view_dependent
    assert not hasattr(field, 'density_gradient')
    assert [id(p) for p in field.parameters()] == [id(p) for p in field.inner.parameters()] and field.inner in list(field.modules())
    c = MC.case("ico", 1.5)
    pts = _t(dev, c['pts'])
    raw = field.forward_pts(pts)
    base = field.inner.forward_pts(pts)
    found, dist, _, _ = tracer.closest(pts, width)
    want = R.tent_np(dist.cpu().numpy(), width, peak)
    assert raw.shape == (len(c['pts']), 4) and np.array_equal(raw[:, 3].detach().cpu().numpy(), want)
    assert torch.equal(raw[:, 3], float(peak) * (1.0 - dist / torch.full((), float(width), device=dev)).clamp_min(0.0))
    assert torch.equal(raw[:, :3], base[:, :3]) and not torch.equal(raw[:, 3], base[:, 3])
    dens = raw[:, 3].detach()
    assert bool((dens[found == 0] == 0).all()) and 0 < int((dens > 0).sum()) < len(c['pts']) and float(dens.max()) <= float(peak)
    assert raw.requires_grad and not field._tent(pts)[0].requires_grad
    shaped = field.forward_pts(pts[:2296].reshape(7, 328, 3))
    assert shaped.shape == (7, 328, 4) and torch.equal(shaped.reshape(-1, 4), raw[:2296])
    assert field.forward_pts(pts[:0]).shape == (0, 4)
    with pytest.raises(L.CtxError, match="width"):
        vr.MeshDensityField(field.inner, tracer, width=3.5 * float(width))
    with pytest.raises(L.CtxError, match="peak"):
        vr.MeshDensityField(field.inner, tracer, peak=0.0)
    with pytest.raises(L.CtxError, match="MeshTracer"):
        vr.MeshDensityField(field.inner, None)
    with pytest.raises(L.CtxError, match="density_gradient"):
        vr.render_normals(field, 8, 8, vr.pinhole(8, 8), torch.eye(4, device=dev)[:3], 0.5, 2.5, tracer.occupancy(1), 0.05)
    other = vr.MeshDensityField(field.inner, tracer, width=2 * float(width), peak=3.0)
    d2 = tracer.closest(pts, 2 * width)[1].cpu().numpy()
    assert np.array_equal(other.forward_pts(pts)[:, 3].detach().cpu().numpy(), R.tent_np(d2, 2 * width, 3.0))


def _camera(dev, H=24):
    from contexture_nerf_amd import run_nerf_helpers as rnh, volume_render as vr
    K = vr.pinhole(H, H)
    c2w = torch.tensor([[1., 0, 0, 0.1], [0, 1, 0, -0.05], [0, 0, 1, 2.0]], device=dev)
    ro, rd = rnh.get_rays(H, H, K, c2w)
    return ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()


def test_no_gradient_reaches_the_density_row(dev):
    from contexture_nerf_amd import run_nerf_helpers as rnh
    tracer = tracer_of(dev, "ico")
    field = _student(dev, tracer)
    grid = tracer.occupancy(1)
    ro, rd = _camera(dev)
    target = torch.rand(ro.shape[0], 3, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    rgb, _, acc, _, _ = rnh.render_rays_marched(field, ro, rd, 0.5, 3.5, grid, float(grid.h[0]) / 2)
    assert rgb.requires_grad and float(acc.detach().max()) > 0.5
    ((rgb - target) ** 2).mean().backward()
    out = field.inner.mlp.output_linear
    assert out.weight.grad.shape[0] == 4 and bool((out.weight.grad[3] == 0).all()) and float(out.bias.grad[3]) == 0.0
    assert all(float(out.weight.grad[k].abs().max()) > 0 and float(out.bias.grad[k]) != 0.0 for k in range(3))
    assert float(field.inner.encoding.table.grad.abs().max()) > 0


def test_view_dependent_inner_passes_through(dev):
    from contexture_nerf_amd import _lib as L, run_nerf_helpers as rnh, volume_render as vr
    from contexture_nerf_amd.hashgrid import ViewDependentField
    tracer = tracer_of(dev, "ico")
    torch.manual_seed(3)
    inner = ViewDependentField(tracer.lo, tracer.hi, n_levels=8, n_features=2, log2_table=12, base_res=4, max_res=64).to(dev)
    with torch.no_grad():
        inner.dir_mlp.output_linear.weight.normal_(0, 0.1)            # a residual that is not zero
    field = vr.MeshDensityField(inner, tracer)
    assert field.view_dependent
    grid = tracer.occupancy(1)
    ro, rd = _camera(dev)
    with torch.no_grad():
        out, ex = rnh.render_rays_marched(field, ro, rd, 0.5, 3.5, grid, float(grid.h[0]) / 2, return_extras=True)
        raw, res = field.forward_dirs(ex['pts'], rd, ex['ray_id'], return_residual=True)
        base, res0 = inner.forward_dirs(ex['pts'], rd, ex['ray_id'], return_residual=True)
        dist = tracer.closest(ex['pts'], field.width)[1]
    assert torch.equal(ex['residual'], res0) and torch.equal(res, res0) and float(res0.abs().max()) > 0
    assert torch.equal(raw[:, :3], base[:, :3]) and torch.equal(field.forward_dirs(ex['pts'], rd, ex['ray_id']), raw)
    assert np.array_equal(raw[:, 3].cpu().numpy(), R.tent_np(dist.cpu().numpy(), field.width, field.peak))
    assert float(out[2].max()) >= 1 - 2.0 ** -20
    with pytest.raises(L.CtxError, match="forward_dirs"):
        _student(dev, tracer).forward_dirs(ex['pts'], rd, ex['ray_id'])


def test_walls_are_opaque_and_empty_space_is_empty(dev):
    """acc >= 1 - 2^-20 on the rays the tracer hits at |cos| > 0.5 (peak * width = 16; the march at width / 2 loses at most
    peak * width / 32 of the optical thickness at each foot of the tent: e^-15 < 2^-20); acc == 0 exactly on the rays whose span misses
    the shell, and on the rays whose samples all lie a width or more from the surface."""
    from contexture_nerf_amd import run_nerf_helpers as rnh
    tracer = tracer_of(dev, "ico")
    field = _student(dev, tracer)
    grid = tracer.occupancy(1)
    ro, rd = _camera(dev, 48)
    with torch.no_grad():
        (rgb, _, acc, _, _), ex = rnh.render_rays_marched(field, ro, rd, 0.5, 3.5, grid, float(grid.h[0]) / 2, return_extras=True)
    hit, _, face, _ = tracer.trace(ro, rd, 0.5, 3.5)
    sc = MC.scene("ico")
    tri = _t(dev, sc['tri'])
    nrm = torch.cross(tri[:, 4:7], tri[:, 8:11], dim=1)
    nrm = nrm / nrm.norm(dim=1, keepdim=True)
    cos = ((rd / rd.norm(dim=1, keepdim=True)) * nrm[face.clamp_min(0)]).sum(1).abs()
    steep = (hit != 0) & (cos > 0.5)
    assert int(steep.sum()) > 200
    print(f"acc on {int(steep.sum())} steep hits: min 1 - {1 - float(acc[steep].double().min()):.3e}")
    assert float(acc[steep].min()) >= 1 - 2.0 ** -20
    _, spanned = grid.ray_spans(ro, rd, 0.5, 3.5)
    assert int((~spanned).sum()) > 200 and bool((acc[~spanned] == 0).all()) and bool((rgb[~spanned] == 0).all())
    dens = field.forward_pts(ex['pts'])[:, 3].detach()
    per_ray = torch.zeros(ro.shape[0], device=dev).index_add_(0, ex['ray_id'].long(), (dens > 0).float())
    clear = spanned & (per_ray == 0)
    assert int(clear.sum()) > 0 and bool((acc[clear] == 0).all())


def test_fit_views_repeats_and_falls(dev):
    """The toy scene: the teacher views of test_raymarch_train_gpu, the icosphere's shell at G = 16, a static grid, march = h / 2,
    40 iterations of 128 rays, 8 levels x 2 features, T = 2^12."""
    import test_raymarch_train_gpu as RT
    from contexture_nerf_amd import volume_render as vr
    images, c2ws, K = RT._teacher_views(dev)
    tracer = tracer_of(dev, "ico")
    grid = tracer.occupancy(1)
    runs = []
    for _ in range(2):
        field = _student(dev, tracer, seed=9)
        hist = vr.fit_views(field, images, c2ws, K, 0.5, 2.5, 40, rays_per_iter=128, lr=1e-2, seed=0, occupancy=grid, occupancy_every=0,
                            march=float(grid.h[0]) / 2)
        runs.append((hist, field.inner.encoding.table.detach().clone(), [p.detach().clone() for p in field.inner.mlp.parameters()]))
    h = runs[0][0]
    print(f"fit_views(MeshDensityField): first five {np.mean(h[:5]):.5f}, last five {np.mean(h[-5:]):.5f}")
    assert len(h) == 40 and all(np.isfinite(x) for x in h)
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1]) and all(torch.equal(a, b) for a, b in zip(runs[0][2], runs[1][2]))
    assert np.mean(h[-5:]) < np.mean(h[:5])


# ---- 4. AtlasField ----------------------------------------------------------------------------------------------------------------------------
ATLAS_MEASURED = 1.7e-7                  # the CPU chain against float64, the largest of four seeds of square_points
ATLAS_GATE = 4 * ATLAS_MEASURED          # 6.8e-7


def square_scene():
    """A unit square of two triangles in the plane z = 0 with its corners at uv (1/8, 1/8) .. (7/8, 7/8), and a T = 8 atlas that is a
    linear ramp: channel 0 = u, channel 1 = v, channel 2 = (u + v) / 2 at the texel centres, so that the bilinear sample at (u, v) is the
    ramp itself for 1/16 <= u, v <= 15/16."""
    v = f32([[-.5, -.5, 0], [.5, -.5, 0], [.5, .5, 0], [-.5, .5, 0]])
    f = np.int64([[0, 1, 2], [0, 2, 3]])
    vt = f32([[.125, .125], [.875, .125], [.875, .875], [.125, .875]])
    T = 8
    c = (np.arange(T, dtype=np.float64) + 0.5) / T
    u, w = np.meshgrid(c, 1.0 - c)                                    # row y of the atlas is v = 1 - (y + 0.5) / T
    atlas = np.stack([u, w, (u + w) / 2]).astype(f32)
    return v, f, vt[f], atlas


def square_points(n=1500, seed=4):
    rng = np.random.default_rng(seed)
    p = np.concatenate([rng.uniform(-0.6, 0.6, (n, 2)), rng.uniform(-0.2, 0.2, (n, 1))], 1)
    return p.astype(f32)


def atlas_colour_np(bary, face, face_uv, dtype=f32):
    """The ramp at uv = (b0 uv0 + b1 uv1) + b2 uv2 -> colour [n,3] = (u, v, (u + v) / 2)."""
    fuv = np.asarray(face_uv, dtype)[np.maximum(face, 0)]
    b = np.asarray(bary, dtype)
    uv = (b[:, 0:1] * fuv[:, 0] + b[:, 1:2] * fuv[:, 1]) + b[:, 2:3] * fuv[:, 2]
    return np.concatenate([uv, (uv[:, :1] + uv[:, 1:]) / dtype(2)], 1)


def test_atlas_field(dev):
    """sigmoid(logits) against the ramp at the rule's uv.  The tolerance: the same chain in torch on the CPU in float32 (uv from the
    barycentrics, grid_sample as texture_mapping defines it, clamp, logit, sigmoid) against the ramp in float64 differs by at most
    1.7e-7 (ATLAS_MEASURED; 1.3e-7 of it is the bilinear sample's) on these points; the gate is 4 x that, 6.8e-7 (last-bit effects of the bilinear weights and of logit / sigmoid near 1/8 and
    7/8; the factor covers another device's exp and log)."""
    from contexture_nerf_amd import volume_render as vr
    v, f, face_uv, atlas = square_scene()
    G = 16
    tracer = vr.MeshTracer(_t(dev, v), _t(dev, f), G, -1.0, 1.0)
    field = vr.AtlasField(tracer, _t(dev, face_uv), _t(dev, atlas))
    assert not list(field.parameters())
    width, peak = R.tent_defaults(tracer.h)
    pts = square_points()
    lo, inv, h = R.grid_consts(G, -1.0, 1.0)
    want = R.closest_grid_np(pts, width, R.mesh_cells_np(v, f, G, lo, inv), R.tri_records_np(v, f), G, lo, inv)
    raw = field.forward_pts(_t(dev, pts))
    assert raw.shape == (len(pts), 4) and raw.dtype == torch.float32 and not raw.requires_grad
    got = raw.cpu().numpy()
    hit = want[0] == 1
    assert 300 < hit.sum() < len(pts) - 300
    assert np.array_equal(got[:, 3], R.tent_np(want[1], width, peak))
    assert not got[~hit].any()                                        # a miss: colour logit 0, density 0
    u, w = want[3][:, 0], want[3][:, 1]
    bary = np.stack([f32(1) - u - w, u, w], 1)
    ramp = atlas_colour_np(bary, want[2], face_uv, np.float64)
    assert ramp[hit].min() >= 0.125 - 1e-6 and ramp[hit].max() <= 0.875 + 1e-6 and np.ptp(ramp[hit], 0).min() > 0.7
    err = np.abs(1.0 / (1.0 + np.exp(-got[hit, :3].astype(np.float64))) - ramp[hit]).max()
    print(f"AtlasField: max |sigmoid(logit) - ramp| = {err:.3e}, gate {ATLAS_GATE:.3e}")
    assert err <= ATLAS_GATE
    # the atlas-to-field direction: the square renders through the marched path in the ramp's colours
    from contexture_nerf_amd import run_nerf_helpers as rnh
    grid = tracer.occupancy(1)
    ro = torch.tensor([[-0.25, 0.25, 1.0], [0.25, -0.125, 1.0], [0.9, 0.9, 1.0]], device=dev)
    rd = torch.tensor([[0., 0, -1], [0., 0, -1], [0., 0, -1]], device=dev)
    rgb, _, acc, _, _ = rnh.render_rays_marched(field, ro, rd, 0.0, 2.0, grid, float(width) / 2)
    assert float(acc[:2].min()) >= 1 - 2.0 ** -20 and float(acc[2]) == 0.0
    uv_ray = (ro[:2, :2].cpu().numpy().astype(np.float64) + 0.5) * 0.75 + 0.125
    want_rgb = np.concatenate([uv_ray, uv_ray.sum(1, keepdims=True) / 2], 1)
    assert np.abs(rgb[:2].cpu().numpy() - want_rgb).max() < 1e-5
    assert field.forward_pts(_t(dev, pts[:0])).shape == (0, 4)
