"""GPU: the pseudonormal tables (csrc/meshpn.hip), the signed point / mesh query (csrc/meshdist.hip) and MeshSolidField (DESIGN section
4s) against tests/meshsdf_rule.py.

1. ctx_mesh_vertex_faces_* and ctx_mesh_pseudonormals on the raw entry points == the rule: the lists and rows 0 and 4-6 array_equal, rows
   1-3 (the only place a transcendental enters) within 4 x the CPU's float32-against-float64 figure; topology() == the rule;
2. ctx_mesh_signed_distance on the raw entry point, outputs between guards and pre-filled, == the grid form of the rule FED THE TABLES READ
   BACK FROM THE DEVICE, array_equal on all six outputs: the CPU scenes at three radii, spot, small batches, a batch past the capped
   launch against chunks, spoilt faces and wild lists, n = 0 and the refusals; found, |sdist|, face and uv == the unsigned kernel's;
3. MeshTracer.signed_distance: dtypes, shapes, barycentrics, |grad|, refusals by name;
4. MeshSolidField: the ramp and its gradient bit for bit, colour untouched, no gradient to the density row, a view-dependent inner, open
   meshes refused, the silhouette, the rendered normals, fit_views repeats and falls, OccupancyGrid.update, field_optimizer and bake_atlas
   take it as any field."""
import numpy as np
import pytest
import torch

import meshdist_rule as R
import meshsdf_rule as S
import test_meshdist_cpu as MC
import test_meshdist_gpu as MG
import test_meshsdf_cpu as SC
from test_engine_ops_gpu import Out

pytestmark = pytest.mark.gpu
f32 = np.float32
_t = MG._t
_DEVICE_TABLES = {}


def device_tables(dev, name, mesh=None):
    """-> (tracer, pn numpy [F,7,3] read back from the device), once per scene."""
    if name not in _DEVICE_TABLES:
        tracer = MG.tracer_of(dev, name, mesh)
        _DEVICE_TABLES[name] = (tracer, tracer.pseudonormals().cpu().numpy())
    return _DEVICE_TABLES[name]


def _raw(dev, tracer, pts, r, pn=None, fill=0xFF):
    """ctx_mesh_signed_distance on the raw entry point into guarded outputs pre-filled with 0xFF -> numpy, the six outputs."""
    from contexture_nerf_amd import _lib as L
    n = len(pts)
    outs = [Out(dev, shape, dtype, fill) for shape, dtype in (((n,), torch.uint8), ((n,), torch.float32), ((n,), torch.int32), ((n, 2), torch.float32),
                                                               ((n,), torch.uint8), ((n, 3), torch.float32))]
    p = _t(dev, pts)
    pn = tracer.pseudonormals() if pn is None else pn
    L.check(L.load().ctx_mesh_signed_distance(L.ptr(p), n, float(r), tracer.G, *map(float, tracer.lo), *map(float, tracer.inv), L.ptr(tracer.cell_off),
                                              L.ptr(tracer.cell_tri), tracer.cell_tri.numel(), L.ptr(tracer.tri), tracer.tri.shape[0], L.ptr(pn),
                                              pn.shape[0], *(L.ptr(o.t) for o in outs), L.stream()))
    return tuple(o.cpu(what).numpy() for o, what in zip(outs, SC.SIGNED_NAMES))


def _same(got, want, tag):
    for what, a, b in zip(SC.SIGNED_NAMES, got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (tag, what, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), (tag, what, np.flatnonzero((a != b).reshape(len(a), -1).any(1))[:10])


# ---- 1. the tables -------------------------------------------------------------------------------------------------------------------------
TABLE_MESHES = ("ico", "spot", "fan", "nonmanifold", "zero_area", "spoilt", "flipped", "cube", "spike")


def _table_mesh(name):
    return R.spot_mesh() if name == "spot" else SC.table_meshes()[name]


@pytest.mark.parametrize("name", TABLE_MESHES)
def test_tables_vs_rule(dev, name):
    """Rows 1-3 gate: 4 x the CPU's float32-against-float64 figure of the scene (test_meshsdf_cpu.TABLE_GATE), for the hand-made meshes
    the larger of the two (their rows are sums of no more terms); the factor covers the device's atan2f."""
    from contexture_nerf_amd import _lib as L, kal
    v, f = _table_mesh(name)
    V, F = len(v), len(f)
    fd = _t(dev, f)
    tri = kal.mesh_tri_records(_t(dev, v), fd)
    want_tri = R.tri_records_np(v, f)
    assert np.array_equal(tri.cpu().numpy(), want_tri, equal_nan=True)
    vf_off, vf_face = kal.mesh_vertex_faces(fd, V)
    ok = np.all((f >= 0) & (f < V), 1)
    ids, who = f[ok].reshape(-1), np.repeat(np.flatnonzero(ok), 3)
    order = np.lexsort((who, ids))
    assert vf_off.dtype == torch.int32 and vf_face.dtype == torch.int32
    assert np.array_equal(vf_off.cpu().numpy(), np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=V))]))
    assert np.array_equal(vf_face.cpu().numpy(), who[order])
    pn = Out(dev, (F, 7, 3), torch.float32)
    L.check(L.load().ctx_mesh_pseudonormals(L.ptr(fd), V, F, L.ptr(tri), L.ptr(vf_off), L.ptr(vf_face), vf_face.numel(), L.ptr(pn.t), L.stream()))
    got = pn.cpu("pn").numpy()
    want = S.pseudonormals_np(f, V, want_tri)
    exact = [0, 4, 5, 6]
    assert np.array_equal(got[:, exact], want[:, exact], equal_nan=True), np.flatnonzero((got[:, exact] != want[:, exact]).any((1, 2)))[:10]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    worst = float(np.nanmax(np.abs(got[:, 1:4] - want[:, 1:4]), initial=0.0))
    gate = SC.TABLE_GATE.get(name, max(SC.TABLE_GATE.values()))
    print(f"{name}: rows 1-3, device against the rule: max |diff| = {worst:.3e}, gate {gate:.3e}")
    assert worst <= gate
    if name == "spoilt":
        assert np.isnan(got[list(MC.broken_mesh()[2])]).all()
    if name == "zero_area":
        assert not got[12:, 0].any() and np.array_equal(got[:12, exact], S.pseudonormals_np(f[:12], 8, want_tri[:12])[:, exact])


def test_tracer_keeps_the_tables_and_counts_the_edges(dev):
    from contexture_nerf_amd import kal, volume_render as vr
    for name in ("ico", "fan", "nonmanifold", "flipped", "spoilt", "cube"):
        v, f = _table_mesh(name)
        tracer = vr.MeshTracer(_t(dev, v), _t(dev, f), 16, -1.0, 1.0)
        assert tracer.topology() == S.topology_np(f, len(v)), name
        assert all(isinstance(x, int) for x in tracer.topology().values())
    assert tracer._pn is None                                          # built lazily
    pn = tracer.pseudonormals()
    assert pn is tracer.pseudonormals() and pn.dtype == torch.float32 and tuple(pn.shape) == (12, 7, 3)
    vf = kal.mesh_vertex_faces(tracer.faces, 8)
    assert torch.equal(pn, kal.mesh_pseudonormals(tracer.faces, 8, tracer.tri, *vf))
    assert np.array_equal(pn.cpu().numpy()[:, 0], S.pseudonormals_np(f, 8, R.tri_records_np(v, f))[:, 0])


def test_table_refusals(dev):
    from contexture_nerf_amd import _lib as L, kal
    lib = L.load()
    v, f = SC.cube()
    fd = _t(dev, f)
    tri = kal.mesh_tri_records(_t(dev, v), fd)
    vf_off, vf_face = kal.mesh_vertex_faces(fd, 8)
    pn, count = Out(dev, (12, 7, 3), torch.float32, 0xA5), Out(dev, (8,), torch.int32, 0xA5)
    good = [L.ptr(fd), 8, 12, L.ptr(tri), L.ptr(vf_off), L.ptr(vf_face), vf_face.numel(), L.ptr(pn.t), L.stream()]
    for change, needle in [({0: None}, "null"), ({3: None}, "null"), ({4: None}, "null"), ({5: None}, "null"), ({7: None}, "null"), ({1: 0}, "V="),
                           ({1: 2 ** 31}, "V="), ({2: 0}, "F="), ({2: 2 ** 31}, "F="), ({6: -1}, "n_vf="), ({6: 37}, "n_vf="),
                           ({3: tri.data_ptr() + 4}, "aligned")]:
        a = list(good)
        for k, val in change.items():
            a[k] = val
        assert lib.ctx_mesh_pseudonormals(*a) == -1 and needle.encode() in lib.ctx_last_error(), (change, lib.ctx_last_error())
    for args, needle in [((None, 8, 12, L.ptr(count.t)), "null"), ((L.ptr(fd), 8, 12, None), "null"), ((L.ptr(fd), 0, 12, L.ptr(count.t)), "V="),
                         ((L.ptr(fd), 256 ** 3 + 1, 12, L.ptr(count.t)), "V="), ((L.ptr(fd), 8, 0, L.ptr(count.t)), "F="),
                         ((L.ptr(fd), 8, 2 ** 31 // 3 + 1, L.ptr(count.t)), "F=")]:
        assert lib.ctx_mesh_vertex_faces_count(*args, L.stream()) == -1 and needle.encode() in lib.ctx_last_error(), (args, lib.ctx_last_error())
    cursor = torch.zeros(8, dtype=torch.int32, device=dev)
    fill = [L.ptr(fd), 8, 12, L.ptr(vf_off), 36, L.ptr(cursor), L.ptr(count.t), L.ptr(pn.t), L.stream()]
    for change, needle in [({4: -1}, "n="), ({4: 37}, "n="), ({3: None}, "null"), ({5: None}, "null"), ({6: None}, "null"), ({7: None}, "null"),
                           ({7: count.t.data_ptr()}, "must not be")]:
        a = list(fill)
        for k, val in change.items():
            a[k] = val
        assert lib.ctx_mesh_vertex_faces_fill(*a) == -1 and needle.encode() in lib.ctx_last_error(), (change, lib.ctx_last_error())
    a = list(fill); a[4] = 0; a[3] = None
    assert lib.ctx_mesh_vertex_faces_fill(*a) == 0                       # n = 0 launches nothing and looks at no pointer
    pn.untouched("mesh_pseudonormals"), count.untouched("mesh_vertex_faces")
    with pytest.raises(L.CtxError, match="V="):
        kal.mesh_vertex_faces(fd, 0)
    with pytest.raises(L.CtxError, match="dtype"):
        kal.mesh_vertex_faces(fd.int(), 8)


# ---- 2. the raw entry point ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mult", MC.RADII)
@pytest.mark.parametrize("name", ["ico", "tri4"])
def test_raw_vs_rule(dev, name, mult):
    c, sc = MC.case(name, mult), MC.scene(name)
    tracer, pn = device_tables(dev, name)
    want = S.sign_step_np(c['pts'], c['r'], c['grid'], sc['tri'], pn)
    got = _raw(dev, tracer, c['pts'], c['r'])
    _same(got, want, (name, mult))
    found = want[0] == 1
    assert 0 < found.sum() < len(found) and (want[1] < 0).sum() > 50 and len(set(want[4][found].tolist())) >= 4
    # the unsigned kernel on the same points
    mine = tracer.signed_distance(_t(dev, c['pts']), c['r'])
    theirs = tracer.closest(_t(dev, c['pts']), c['r'])
    assert torch.equal(mine[0], theirs[0]) and torch.equal(mine[1].abs(), theirs[1]) and torch.equal(mine[2], theirs[2]) and torch.equal(mine[3], theirs[3])


@pytest.mark.parametrize("n", [1, 63, 65])
def test_raw_small_batches(dev, n):
    c, sc = MC.case("ico", 1.5), MC.scene("ico")
    tracer, pn = device_tables(dev, "ico")
    pick = np.arange(n) * 7 + 3
    want = S.sign_step_np(c['pts'][pick], c['r'], [x[pick] for x in c['grid']], sc['tri'], pn)
    _same(_raw(dev, tracer, c['pts'][pick], c['r']), want, n)


def test_raw_spot(dev):
    import test_meshhit_gpu as MH
    tracer, v, f, lists, tri = MH.scene(dev, "spot")
    pn = tracer.pseudonormals().cpu().numpy()
    r = f32(1.5) * np.min(tracer.h)
    pts = MG._spot_points(4096, float(r), 5)
    want = S.signed_grid_np(pts, r, lists, tri, pn, tracer.G, tracer.lo, tracer.inv)
    _same(_raw(dev, tracer, pts, r), want, "spot")
    found = want[0] == 1
    assert 1000 < found.sum() < 4000 and set(want[4][found].tolist()) == set(range(7)) and 200 < (want[1] < 0).sum() < found.sum() - 200
    wn = S.winding_number_np(pts[found], v, f)                         # and the device's sign is the truth's
    assert np.array_equal(want[1][found] < 0, wn > 0.5)
    mine, theirs = tracer.signed_distance(_t(dev, pts), r), tracer.closest(_t(dev, pts), r)
    assert torch.equal(mine[0], theirs[0]) and torch.equal(mine[1].abs(), theirs[1]) and torch.equal(mine[2], theirs[2]) and torch.equal(mine[3], theirs[3])


def test_large_batch_equals_chunks(dev):
    """n = 2048 * 256 + 3: three points more than one pass of the capped grid.  Against the same points in chunks, and the rule on 300."""
    import test_meshhit_gpu as MH
    from contexture_nerf_amd import kal
    tracer, v, f, lists, tri = MH.scene(dev, "spot")
    pn = tracer.pseudonormals()
    n = 2048 * 256 + 3
    r = f32(0.75) * np.min(tracer.h)
    pts = MG._spot_points(n, float(r), 6)
    p = _t(dev, pts)
    args = (r, tracer.G, tracer.lo, tracer.inv, tracer.cell_off, tracer.cell_tri, tracer.tri, pn)
    whole = kal.mesh_signed_distance(p, *args)
    cut = [0, 1, 70000, 70001 + 256 * 1024, n]
    parts = [kal.mesh_signed_distance(p[a:b].contiguous(), *args) for a, b in zip(cut[:-1], cut[1:])]
    for j in range(6):
        assert torch.equal(whole[j], torch.cat([q[j] for q in parts])), SC.SIGNED_NAMES[j]
    assert 0 < int(whole[0].sum()) < n and int((whole[1] < 0).sum()) > 1000
    pick = np.concatenate([np.arange(100), n // 2 + np.arange(100), n - 100 + np.arange(100)])
    want = S.signed_grid_np(pts[pick], r, lists, tri, pn.cpu().numpy(), tracer.G, tracer.lo, tracer.inv)
    _same([x.cpu().numpy()[pick] for x in whole], want, "large")


def test_spoilt_faces_and_wild_lists(dev):
    v, f, bad = MC.broken_mesh()
    sc, c = MC.scene("tri4"), MC.case("tri4", 1.5)
    tracer, pn = device_tables(dev, "tri4+broken", (v, f))
    assert np.isnan(pn[list(bad)]).all()
    centre = sc['v'][sc['f'][list(bad)]].mean(1)
    pts = np.concatenate([centre, c['pts'][:500]]).astype(f32)
    tri = R.tri_records_np(v, f)
    want = S.signed_grid_np(pts, c['r'], R.mesh_cells_np(v, f, sc['G'], sc['lo'], sc['inv']), tri, pn, sc['G'], sc['lo'], sc['inv'])
    got = _raw(dev, tracer, pts, c['r'])
    _same(got, want, "spoilt")
    assert not set(got[2].tolist()) & set(bad) and got[0].sum() > 100 and np.isfinite(got[1]).all() and np.isfinite(got[5]).all()
    good = MG.tracer_of(dev, "tri4")
    wild = sc['lists'][2].copy()
    wild[::7], wild[3::11] = -1, len(f)
    want = S.signed_grid_np(pts, c['r'], (sc['lists'][0], sc['lists'][1], wild), tri, pn, sc['G'], sc['lo'], sc['inv'])

    class Mixed:
        G, lo, inv, cell_off, cell_tri, tri = good.G, good.lo, good.inv, good.cell_off, _t(dev, wild), tracer.tri
    got = _raw(dev, Mixed, pts, c['r'], pn=tracer.pseudonormals())
    _same(got, want, "stale lists")
    assert not set(got[2].tolist()) & set(bad)


def test_refusals_and_empty_batch(dev):
    from contexture_nerf_amd import _lib as L
    lib = L.load()
    tracer, _ = device_tables(dev, "ico")
    pn = tracer.pseudonormals()
    c = MC.case("ico", 1.5)
    pts = _t(dev, c['pts'][:4])
    outs = [Out(dev, shape, dtype, 0xA5) for shape, dtype in (((4,), torch.uint8), ((4,), torch.float32), ((4,), torch.int32), ((4, 2), torch.float32),
                                                               ((4,), torch.uint8), ((4, 3), torch.float32))]
    hmin = float(np.min(tracer.h))
    good = [L.ptr(pts), 4, float(c['r']), tracer.G, *map(float, tracer.lo), *map(float, tracer.inv), L.ptr(tracer.cell_off), L.ptr(tracer.cell_tri),
            tracer.cell_tri.numel(), L.ptr(tracer.tri), tracer.tri.shape[0], L.ptr(pn), pn.shape[0], *(L.ptr(o.t) for o in outs), L.stream()]
    cases = [({k: None}, "null") for k in (0, 10, 11, 13, 15, 17, 18, 19, 20, 21, 22)]
    cases += [({1: -1}, "n="), ({1: 2 ** 31}, "n="), ({12: -1}, "n_list="), ({12: 2 ** 31}, "n_list="), ({3: 0}, "outside [1, 256]"),
              ({3: 257}, "outside [1, 256]"), ({14: 0}, "F="), ({2: 0.0}, "radius > 0"), ({2: -1.0}, "radius > 0"), ({2: float('nan')}, "radius > 0"),
              ({2: float('inf')}, "radius > 0"), ({2: 3.01 * hmin}, "larger than 3 cells"), ({13: tracer.tri.data_ptr() + 4}, "aligned"),
              ({20: outs[3].t.data_ptr() + 4}, "aligned"), ({16: pn.shape[0] - 1}, "short"), ({16: 0}, "short")]
    for change, needle in cases:
        a = list(good)
        for k, val in change.items():
            a[k] = val
        rc = lib.ctx_mesh_signed_distance(*a)
        assert rc == -1 and needle.encode() in lib.ctx_last_error() and b"mesh_signed_distance" in lib.ctx_last_error(), (change, rc, lib.ctx_last_error())
    a = list(good); a[1] = 0
    assert lib.ctx_mesh_signed_distance(*a) == 0                         # n = 0 launches nothing
    a = list(good); a[1] = 0; a[0] = a[15] = a[17] = None
    assert lib.ctx_mesh_signed_distance(*a) == 0                         # and looks at no pointer
    for x in outs:
        x.untouched("mesh_signed_distance")
    a = list(good); a[2] = 3.0 * hmin                                    # the limit itself passes
    assert lib.ctx_mesh_signed_distance(*a) == 0
    assert outs[0].cpu("found").max() <= 1 and outs[4].cpu("feature").max() <= 6


# ---- 3. MeshTracer.signed_distance ---------------------------------------------------------------------------------------------------------
def test_signed_distance_wrapper(dev):
    from contexture_nerf_amd import _lib as L
    tracer, pn = device_tables(dev, "ico")
    c, sc = MC.case("ico", 3.0), MC.scene("ico")
    pts = _t(dev, c['pts'])
    found, sdist, face, bary, grad = tracer.signed_distance(pts, c['r'])
    assert (found.dtype, sdist.dtype, face.dtype, bary.dtype, grad.dtype) == (torch.uint8, torch.float32, torch.int64, torch.float32, torch.float32)
    n = len(c['pts'])
    assert [tuple(x.shape) for x in (found, sdist, face, bary, grad)] == [(n,), (n,), (n,), (n, 3), (n, 3)]
    want = S.sign_step_np(c['pts'], c['r'], c['grid'], sc['tri'], pn)
    assert np.array_equal(found.cpu().numpy(), want[0]) and np.array_equal(sdist.cpu().numpy(), want[1]) and np.array_equal(face.cpu().numpy(), want[2])
    assert np.array_equal(grad.cpu().numpy(), want[5])
    u, v = want[3][:, 0], want[3][:, 1]
    assert np.array_equal(bary.cpu().numpy(), np.stack([f32(1) - u - v, u, v], 1) * want[0][:, None].astype(f32))
    norm = grad.double().norm(dim=1).cpu().numpy()
    assert np.abs(norm[want[0] == 1] - 1).max() <= 1e-6 and not grad[found == 0].any() and bool((sdist[found == 0] == float(c['r'])).all())
    wn = S.winding_number_np(c['pts'][want[0] == 1], sc['v'], sc['f'])
    assert np.array_equal(want[1][want[0] == 1] < 0, wn > 0.5)          # negative is inside
    assert not any(x.requires_grad for x in (found, sdist, face, bary, grad))
    empty = tracer.signed_distance(pts[:0], c['r'])
    assert [tuple(x.shape) for x in empty] == [(0,), (0,), (0,), (0, 3), (0, 3)] and empty[2].dtype == torch.int64
    with pytest.raises(L.CtxError, match="requires grad"):
        tracer.signed_distance(pts.clone().requires_grad_(), c['r'])
    hmin = float(np.min(tracer.h))
    for bad in (0.0, -0.1, float('nan'), float('inf'), 3.01 * hmin):
        with pytest.raises(L.CtxError, match="max_dist"):
            tracer.signed_distance(pts, bad)
    tracer.signed_distance(pts[:8].contiguous(), 3 * np.min(tracer.h))
    with pytest.raises(L.CtxError, match=r"pts \[n,3\]"):
        tracer.signed_distance(pts.reshape(-1), c['r'])
    with pytest.raises(L.CtxError, match="dtype"):
        tracer.signed_distance(pts.double(), c['r'])
    with pytest.raises(L.CtxError, match="device tensor"):
        tracer.signed_distance(pts.cpu(), c['r'])


# ---- 4. MeshSolidField ---------------------------------------------------------------------------------------------------------------------
def _student(dev, tracer, seed=2, cls="MeshSolidField"):
    from contexture_nerf_amd import volume_render as vr
    from contexture_nerf_amd.hashgrid import HashGridField
    torch.manual_seed(seed)
    inner = HashGridField(tracer.lo, tracer.hi, n_levels=8, n_features=2, log2_table=12, base_res=4, max_res=64).to(dev)
    return getattr(vr, cls)(inner, tracer)


def test_density_is_the_ramp_and_colour_is_inners(dev):
    from contexture_nerf_amd import _lib as L, volume_render as vr
    tracer, pn = device_tables(dev, "ico")
    field = _student(dev, tracer)
    width, peak = S.ramp_defaults(tracer.h)
    assert field.width == width and field.peak == peak and float(peak) * float(width) == 32.0 and not field.view_dependent
    assert [id(p) for p in field.parameters()] == [id(p) for p in field.inner.parameters()] and field.inner in list(field.modules())
    c, sc = MC.case("ico", 1.5), MC.scene("ico")
    pts = _t(dev, c['pts'])
    raw, base = field.forward_pts(pts), field.inner.forward_pts(pts)
    rule = S.signed_grid_np(c['pts'], width, sc['lists'], sc['tri'], pn, sc['G'], sc['lo'], sc['inv'])
    want = S.ramp_np(rule[1], width, peak)
    dens = raw[:, 3].detach()
    assert raw.shape == (len(c['pts']), 4) and np.array_equal(dens.cpu().numpy(), want)
    assert torch.equal(raw[:, :3], base[:, :3]) and not torch.equal(raw[:, 3], base[:, 3])
    sd = _t(dev, rule[1])
    assert bool((dens[sd >= 0] == 0).all()) and bool((dens[sd < 0] > 0).all()) and 100 < int((dens > 0).sum()) < len(c['pts']) - 100
    assert float(dens.max()) <= float(peak) and raw.requires_grad and not field._ramp(pts)[0].requires_grad
    shaped = field.forward_pts(pts[:2296].reshape(7, 328, 3))
    assert shaped.shape == (7, 328, 4) and torch.equal(shaped.reshape(-1, 4), raw[:2296])
    assert field.forward_pts(pts[:0]).shape == (0, 4)
    # the gradient, in any grad mode, with HashGridField's return convention
    want_g = S.ramp_gradient_np(rule[1], rule[5], width, peak)
    g = field.density_gradient(pts)
    with torch.no_grad():
        raw2, g2 = field.density_gradient(pts, return_raw=True)
    assert np.array_equal(g.cpu().numpy(), want_g) and torch.equal(g, g2) and torch.equal(raw2, raw.detach()) and not g.requires_grad
    on = (rule[1] < 0) & (rule[1] > -width)
    assert 100 < on.sum() and not want_g[~on].any() and np.abs(np.linalg.norm(want_g[on].astype(np.float64), axis=1) / (float(peak) / float(width)) - 1).max() < 1e-6
    assert field.density_gradient(pts[:6].reshape(2, 3, 3)).shape == (2, 3, 3) and field.density_gradient(pts[:0]).shape == (0, 3)
    for bad in (0, 2, True, 3.0):
        with pytest.raises(L.CtxError, match="channel"):
            field.density_gradient(pts, channel=bad)
    with pytest.raises(L.CtxError, match="width"):
        vr.MeshSolidField(field.inner, tracer, width=3.5 * float(width))
    with pytest.raises(L.CtxError, match="peak"):
        vr.MeshSolidField(field.inner, tracer, peak=0.0)
    with pytest.raises(L.CtxError, match="MeshTracer"):
        vr.MeshSolidField(field.inner, None)
    other = vr.MeshSolidField(field.inner, tracer, width=2 * float(width), peak=3.0)
    sd2 = tracer.signed_distance(pts, 2 * width)[1].cpu().numpy()
    assert np.array_equal(other.forward_pts(pts)[:, 3].detach().cpu().numpy(), S.ramp_np(sd2, 2 * width, 3.0))
    # MeshDensityField is what it was
    tent = vr.MeshDensityField(field.inner, tracer)
    assert not hasattr(tent, 'density_gradient')


def test_open_meshes_are_refused(dev):
    from contexture_nerf_amd import _lib as L, volume_render as vr
    inner = _student(dev, MG.tracer_of(dev, "ico")).inner
    for name in ("fan", "nonmanifold", "flipped"):
        v, f = SC.table_meshes()[name]
        tracer = vr.MeshTracer(_t(dev, v), _t(dev, f), 16, -1.0, 1.0)
        with pytest.raises(L.CtxError, match="not closed and consistently oriented"):
            vr.MeshSolidField(inner, tracer)
        field = vr.MeshSolidField(inner, tracer, allow_open=True)
        assert field.forward_pts(_t(dev, MC.case("ico", 1.5)['pts'][:64])).shape == (64, 4)


def test_no_gradient_reaches_the_density_row(dev):
    from contexture_nerf_amd import run_nerf_helpers as rnh
    tracer = MG.tracer_of(dev, "ico")
    field = _student(dev, tracer)
    grid = tracer.occupancy(1)
    ro, rd = MG._camera(dev)
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
    tracer = MG.tracer_of(dev, "ico")
    torch.manual_seed(3)
    inner = ViewDependentField(tracer.lo, tracer.hi, n_levels=8, n_features=2, log2_table=12, base_res=4, max_res=64).to(dev)
    with torch.no_grad():
        inner.dir_mlp.output_linear.weight.normal_(0, 0.1)            # a residual that is not zero
    field = vr.MeshSolidField(inner, tracer)
    assert field.view_dependent
    grid = tracer.occupancy(1)
    ro, rd = MG._camera(dev)
    with torch.no_grad():
        out, ex = rnh.render_rays_marched(field, ro, rd, 0.5, 3.5, grid, float(grid.h[0]) / 2, return_extras=True)
        raw, res = field.forward_dirs(ex['pts'], rd, ex['ray_id'], return_residual=True)
        base, res0 = inner.forward_dirs(ex['pts'], rd, ex['ray_id'], return_residual=True)
        sdist = tracer.signed_distance(ex['pts'], field.width)[1]
    assert torch.equal(ex['residual'], res0) and torch.equal(res, res0) and float(res0.abs().max()) > 0
    assert torch.equal(raw[:, :3], base[:, :3]) and torch.equal(field.forward_dirs(ex['pts'], rd, ex['ray_id']), raw)
    assert np.array_equal(raw[:, 3].cpu().numpy(), S.ramp_np(sdist.cpu().numpy(), field.width, field.peak))
    assert float(out[2].max()) >= 1 - 2.0 ** -20
    with pytest.raises(L.CtxError, match="forward_dirs"):
        _student(dev, tracer).forward_dirs(ex['pts'], rd, ex['ray_id'])


def test_the_silhouette_is_the_meshes(dev):
    """acc >= 1 - 2^-20 on the rays the tracer hits at |cos| > 0.5 (MeshSolidField's docstring: two walls of optical thickness >= 8 each);
    acc == 0 exactly on the rays the tracer misses whose samples all have sdist >= 0; acc < 1e-4 on every ray the tracer misses (a wrong
    sign can only occur within rounding of the surface, where the ramp is peak * 1e-6 / width at most); and the error of acc against the
    traced silhouette is strictly below the tent field's on the same rays (measured on an MI355X: 3.9e-3 against 1.1e-1; acc on the steep
    hits >= 1 - 6.0e-8, on the misses 0)."""
    from contexture_nerf_amd import run_nerf_helpers as rnh
    tracer = MG.tracer_of(dev, "ico")
    field, tent = _student(dev, tracer), _student(dev, tracer, cls="MeshDensityField")
    grid = tracer.occupancy(1)
    ro, rd = MG._camera(dev, 48)
    with torch.no_grad():
        (_, _, acc, _, _), ex = rnh.render_rays_marched(field, ro, rd, 0.5, 3.5, grid, float(grid.h[0]) / 2, return_extras=True)
        acc_tent = rnh.render_rays_marched(tent, ro, rd, 0.5, 3.5, grid, float(grid.h[0]) / 2)[2]
        sdist = tracer.signed_distance(ex['pts'], field.width)[1]
    hit, _, face, _ = tracer.trace(ro, rd, 0.5, 3.5)
    tri = _t(dev, MC.scene("ico")['tri'])
    nrm = torch.cross(tri[:, 4:7], tri[:, 8:11], dim=1)
    nrm = nrm / nrm.norm(dim=1, keepdim=True)
    cos = ((rd / rd.norm(dim=1, keepdim=True)) * nrm[face.clamp_min(0)]).sum(1).abs()
    steep, miss = (hit != 0) & (cos > 0.5), hit == 0
    assert int(steep.sum()) > 200 and int(miss.sum()) > 200
    print(f"acc on {int(steep.sum())} steep hits: min 1 - {1 - float(acc[steep].double().min()):.3e}; on {int(miss.sum())} misses: max {float(acc[miss].max()):.3e}")
    assert float(acc[steep].min()) >= 1 - 2.0 ** -20
    inside = torch.zeros(ro.shape[0], device=dev).index_add_(0, ex['ray_id'].long(), (sdist < 0).float())
    clear = miss & (inside == 0)
    assert int(clear.sum()) > 200 and bool((acc[clear] == 0).all())
    assert float(acc[miss].max()) < 1e-4
    mse, mse_tent = float(((acc - hit.float()) ** 2).mean()), float(((acc_tent - hit.float()) ** 2).mean())
    print(f"mean((acc - hit)^2): solid {mse:.4e}, tent {mse_tent:.4e}")
    assert mse < mse_tent
    # the device's acc against the rules composited in float64, on the device's own lists
    ref = SC.solid_render_np(48, ro.cpu().numpy(), rd.cpu().numpy(), (ex['ray_id'].cpu().numpy(), ex['dt'].cpu().numpy(), ex['pts'].cpu().numpy()))
    assert np.array_equal(ref['hit'], hit.cpu().numpy()) and np.abs(acc.cpu().numpy() - ref['acc']).max() < 1e-5


NORMAL_GATE = 4 * SC.NORMAL_MEASURED     # 9.2e-2: the CPU rule composited in float64 (test_meshsdf_cpu.test_solid_render_by_the_rules)
NORMAL_DEVICE = 5e-5


def test_rendered_normals_are_the_meshes(dev):
    """render_normals takes the field unchanged.  On rays that hit a face at |cos| > 0.5 with the three barycentrics above 0.2 the
    rendered normal is that face's unit normal up to NORMAL_GATE, 4 x the figure measured for the float32 rule composited in float64 on
    the CPU for the same camera: max |normal - face normal| = 2.2e-2.  That is no rounding figure: at |cos| near 0.5 a ray moves sideways
    by up to 1.7 x its depth, so the deeper samples of the ramp (a few per cent of the weight) have their nearest point on a
    neighbouring face of the icosphere, whose normal is some 10 degrees off.  What IS a rounding figure is the device against that same
    restatement on the device's own sample lists: NORMAL_DEVICE = 5e-5 bounds float32 compositing of at most 40 samples per ray (some
    ten rounded operations each, 2^-24 apiece, doubled by the normalisation); measured on an MI355X: 9.5e-8 on 387 rays."""
    from contexture_nerf_amd import volume_render as vr
    tracer = MG.tracer_of(dev, "ico")
    field = _student(dev, tracer)
    grid = tracer.occupancy(1)
    H = 48
    c2w = torch.tensor([[1., 0, 0, 0.1], [0, 1, 0, -0.05], [0, 0, 1, 2.0]], device=dev)
    out = vr.render_normals(field, H, H, vr.pinhole(H, H), c2w, 0.5, 3.5, grid, float(grid.h[0]) / 2)
    ro, rd = MG._camera(dev, H)
    samples = grid.march(ro, rd, 0.5, 3.5, float(grid.h[0]) / 2)
    ref = SC.solid_render_np(H, ro.cpu().numpy(), rd.cpu().numpy(), (samples[1].cpu().numpy(), samples[3].cpu().numpy(), samples[4].cpu().numpy()))
    cpu = SC.solid_render_np(H)
    flat = ref['flat']
    normal = out['normal'].reshape(-1, 3).cpu().numpy().astype(np.float64)
    dev_face = float(np.abs(normal[flat] - ref['face_normal'][flat]).max())
    cpu_face = float(np.abs(cpu['normal'][cpu['flat']] - cpu['face_normal'][cpu['flat']]).max())
    dev_ref = float(np.abs(normal[ref['steep']] - ref['normal'][ref['steep']]).max())
    print(f"normals on {int(flat.sum())} rays: device against the face {dev_face:.3e}, the CPU rule against the face {cpu_face:.3e} "
          f"(gate {NORMAL_GATE:.3e}); device against the rule in float64 on {int(ref['steep'].sum())} steep rays {dev_ref:.3e} (gate {NORMAL_DEVICE:.0e})")
    assert flat.sum() >= 40 and dev_face <= NORMAL_GATE and dev_ref <= NORMAL_DEVICE
    assert bool((out['z_normal'].reshape(-1)[_t(dev, flat)] > 0).all())
    assert np.abs(np.linalg.norm(normal[ref['steep']], axis=1) - 1).max() < 1e-5 and not normal[ref['acc'] == 0].any()


def test_fit_views_repeats_and_falls(dev):
    """The toy scene of test_meshdist_gpu.test_fit_views_repeats_and_falls, with the solid field; OccupancyGrid.update and field_optimizer
    take the field as any other."""
    import test_raymarch_train_gpu as RT
    from contexture_nerf_amd import volume_render as vr
    images, c2ws, K = RT._teacher_views(dev)
    tracer = MG.tracer_of(dev, "ico")
    grid = tracer.occupancy(1)
    runs = []
    for _ in range(2):
        field = _student(dev, tracer, seed=9)
        hist = vr.fit_views(field, images, c2ws, K, 0.5, 2.5, 40, rays_per_iter=128, lr=1e-2, seed=0, occupancy=grid, occupancy_every=0,
                            march=float(grid.h[0]) / 2)
        runs.append((hist, field.inner.encoding.table.detach().clone(), [p.detach().clone() for p in field.inner.mlp.parameters()]))
    h = runs[0][0]
    print(f"fit_views(MeshSolidField): first five {np.mean(h[:5]):.5f}, last five {np.mean(h[-5:]):.5f}")
    assert len(h) == 40 and all(np.isfinite(x) for x in h)
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1]) and all(torch.equal(a, b) for a, b in zip(runs[0][2], runs[1][2]))
    assert np.mean(h[-5:]) < np.mean(h[:5])
    vr.field_optimizer(field, 1e-2)
    live = tracer.occupancy(1)
    live.update(field, 0.5)
    assert 0 < float(live.fraction()) < float(grid.fraction()) + 1e-9


def test_bake_atlas_takes_the_field(dev, meshes):
    """bake_atlas marches from outside the surface through the wall: the solid field covers the chart as any opaque field does, and two
    bakes are equal.  The bake's default step, 1.5 h / 8, is below width / 2."""
    import test_bake_gpu as TB
    from contexture_nerf_amd import volume_render as vr
    from contexture_nerf_amd.hashgrid import HashGridField
    c = TB.spot_case(meshes, 32)
    ten = [_t(dev, c['v']), _t(dev, c['f']), _t(dev, c['uv']), _t(dev, c['tface']), _t(dev, c['tbary'])]
    tracer = vr.MeshTracer(ten[0], ten[1], 16, -1.0, 1.0)
    assert tracer.topology() == dict(boundary_edges=0, nonmanifold_edges=0, inconsistent_edges=0)
    torch.manual_seed(4)
    field = vr.MeshSolidField(HashGridField(tracer.lo, tracer.hi, n_levels=8, n_features=2, log2_table=12, base_res=4, max_res=64).to(dev), tracer)
    grid = tracer.occupancy(1)
    acc = vr.bake_atlas(field, *ten, grid, supersample=2)
    covered = int((acc[3] > 0).sum())
    print(f"bake_atlas(MeshSolidField): {covered} covered of {len(c['chart'])} chart texels")
    assert covered > 0.9 * len(c['chart']) and torch.equal(vr.bake_atlas(field, *ten, grid, supersample=2), acc)
