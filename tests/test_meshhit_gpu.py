"""GPU: the ray / mesh intersector (csrc/meshhit.hip) against tests/meshhit_rule.py, and its two uses.

1. lists: ctx_mesh_cells_count / _scan / _fill and ctx_mesh_tri_setup == the rule, array_equal: random triangles of the four kinds at
   G in {1, 4, 16}, spot at G = 32, F in {1, 7, 8195}, 1500 triangles in one cell, one giant triangle at G = 64; MeshTracer.occupancy;
2. hits: hit, face, t, uv == the rule, array_equal, outputs between guards and pre-filled; mode 1; own_face; a batch past the capped grid
   against the same rays in chunks; refusals;
3. bake_atlas(visibility=) on a square under a small wall;
4. train_step / fit_views(mesh=): weights 0 leave every bit, the reported terms are the formulas, the mask term falls.
No tolerance in this file."""
import numpy as np
import pytest
import torch

import meshhit_rule as MR
import test_uv_gather_cpu as UG
import test_occupancy_gpu as OG
from test_engine_ops_gpu import Out

pytestmark = pytest.mark.gpu
f32 = np.float32


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- 1. lists --------------------------------------------------------------------------------------------------------------------------
def _lists_equal(dev, v, f, G, lo=-1.0, hi=1.0):
    """kal.mesh_cell_lists and kal.mesh_tri_records against the rule -> the rule's (count, cell_off, cell_tri)."""
    from contexture_nerf_amd import kal
    v, f = np.ascontiguousarray(v, f32).reshape(-1, 3), np.ascontiguousarray(f, np.int64).reshape(-1, 3)
    lo3, inv, _ = MR.grid_consts(G, lo, hi)
    want = MR.mesh_cells_np(v, f, G, lo3, inv)
    got = kal.mesh_cell_lists(_t(dev, v), _t(dev, f), G, lo3, inv)
    for name, a, b in zip(("count", "cell_off", "cell_tri"), got, want):
        assert a.dtype == torch.int32 and np.array_equal(a.cpu().numpy(), b), (name, G, len(f))
    tri = kal.mesh_tri_records(_t(dev, v), _t(dev, f)).cpu().numpy()
    assert np.array_equal(tri, MR.tri_records_np(v, f), equal_nan=True)
    return want


@pytest.mark.parametrize("G", [1, 4, 16])
def test_lists_random_triangles_vs_rule(dev, G):
    """300 triangles: 110 sub-cell, 100 several cells across, 20 reaching outside the grid, 70 lying exactly on a cell face; then a few
    faces with an index out of range or a non-finite vertex among them."""
    rng = np.random.default_rng(200 + G)
    tri = np.concatenate([MR.random_triangles(rng, G, n, kind) for n, kind in zip((110, 100, 20, 70), MR.KINDS)])
    v, f = MR.triangles_to_mesh(tri, G)
    count, _, cell_tri = _lists_equal(dev, v, f, G)
    assert len(cell_tri) > 200 and count.sum() == len(cell_tri)
    v2, f2 = v.copy(), f.copy()
    v2[f2[5, 1]] = np.nan; v2[f2[17, 0], 2] = np.inf; f2[40, 2] = -1; f2[41, 0] = len(v2)
    _, _, cell_tri2 = _lists_equal(dev, v2, f2, G)
    assert not set(cell_tri2.tolist()) & {5, 17, 40, 41} and len(cell_tri2) < len(cell_tri)


def test_lists_spot(dev):
    v, f = MR.spot_mesh()
    count, _, cell_tri = _lists_equal(dev, v, f, 32)
    assert count.max() > 64 and len(cell_tri) > 10000                 # a list longer than one wave


def test_lists_face_counts_long_segment_and_giant(dev):
    G = 16
    rng = np.random.default_rng(8)
    # F = 1, F below one block's four waves, and F = 8195: three more than the 2048 blocks x 4 waves of the capped launch
    for F in (1, 7, 8195):
        v, f = MR.triangles_to_mesh(MR.random_triangles(rng, G, F, "small"), G)
        _lists_equal(dev, v, f, G)
    # 1500 sub-cell triangles inside one cell of a G = 4 grid: one segment longer than a wave and longer than 1024
    tri = 1.0 + rng.uniform(0.1, 0.9, (1500, 3, 3))
    v, f = MR.triangles_to_mesh(np.round(tri * 1024) / 1024, 4)
    count, _, cell_tri = _lists_equal(dev, v, f, 4)
    assert count.max() == 1500 and (count > 0).sum() == 1 and np.array_equal(cell_tri, np.arange(1500))
    # one giant triangle across a G = 64 grid: G^3 candidates for one wave
    G = 64
    lo3, _, h = MR.grid_consts(G, -1.0, 1.0)
    v = (lo3 + f32([[-40.25, 10.5, -7.0], [130.0, 20.25, 50.5], [30.5, 90.0, 140.75]]) * h).astype(f32)
    count, _, _ = _lists_equal(dev, v, [[0, 1, 2]], G)
    assert 2000 < count.sum() < 20000 and count.max() == 1


def test_tracer_occupancy_is_from_mesh(dev):
    from contexture_nerf_amd import volume_render as vr
    v, f = _t(dev, MR.icosphere(2, 0.6)[0]), _t(dev, MR.icosphere(2, 0.6)[1])
    box = (16, (-1.0, -0.75, -1.0), (1.0, 1.0, 0.875))
    tracer = vr.MeshTracer(v, f, *box)
    for dilate in (0, 1, 2):
        want = vr.OccupancyGrid.from_mesh(v, f, *box, dilate=dilate)
        got = tracer.occupancy(dilate)
        assert torch.equal(got.cells, want.cells) and got.cells.dtype == torch.uint8 and not bool(got.dens.any())
        assert got.G == want.G and all(np.array_equal(getattr(got, k), getattr(want, k)) for k in ("lo", "hi", "inv", "h"))
    st = tracer.stats()
    count = tracer.count.cpu().numpy()
    assert st == dict(entries=int(count.sum()), mean_list=float(count[count > 0].astype(np.float32).mean()), max_list=int(count.max()))


# ---- 2. hits ---------------------------------------------------------------------------------------------------------------------------
_SCENES = {}


def scene(dev, name):
    """(tracer, v, f, rule lists, rule tri) of the icosphere at G = 16 or spot at G = 32, built once."""
    if name not in _SCENES:
        from contexture_nerf_amd import volume_render as vr
        v, f = MR.icosphere(2, 0.6) if name == "ico" else MR.spot_mesh()
        G = 16 if name == "ico" else 32
        lo3, inv, _ = MR.grid_consts(G, -1.0, 1.0)
        _SCENES[name] = (vr.MeshTracer(_t(dev, v), _t(dev, f), G, -1.0, 1.0), v, f, MR.mesh_cells_np(v, f, G, lo3, inv), MR.tri_records_np(v, f))
    return _SCENES[name]


def _rule(sc, ro, rd, near, far, own=None, mode=0):
    tracer, v, f, lists, tri = sc
    return MR.mesh_hit_grid_np(ro, rd, near, far, lists, tri, f, tracer.G, tracer.lo, tracer.hi, tracer.inv, tracer.h, own_face=own, mode=mode)


def _raw_hit(dev, tracer, ro, rd, near, far, own=None, mode=0):
    """ctx_mesh_ray_hit on the raw entry point into guarded outputs pre-filled with 0xFF -> numpy (hit, t, face, uv)."""
    from contexture_nerf_amd import _lib as L
    R = len(ro)
    hit, t, face, uv = Out(dev, (R,), torch.uint8), Out(dev, (R,), torch.float32), Out(dev, (R,), torch.int32), Out(dev, (R, 2), torch.float32)
    ten = _t(dev, ro), _t(dev, rd)
    t_own = None if own is None else _t(dev, np.asarray(own, np.int64))
    L.check(L.load().ctx_mesh_ray_hit(L.ptr(ten[0]), L.ptr(ten[1]), R, near, far, L.ptr(tracer.cells), tracer.G, *map(float, tracer.lo),
                                      *map(float, tracer.hi), *map(float, tracer.inv), *map(float, tracer.h), L.ptr(tracer.cell_off),
                                      L.ptr(tracer.cell_tri), tracer.cell_tri.numel(), L.ptr(tracer.tri), L.ptr(tracer.faces), tracer.faces.shape[0],
                                      L.ptr(t_own), mode, L.ptr(hit.t), *((L.ptr(t.t), L.ptr(face.t), L.ptr(uv.t)) if mode == 0 else (None, None, None)),
                                      L.stream()))
    if mode == 1:                                                     # t, face and uv were not handed over
        return hit.cpu("hit").numpy(), None, None, None
    return hit.cpu("hit").numpy(), t.cpu("t").numpy(), face.cpu("face").numpy(), uv.cpu("uv").numpy()


def _camera_like_rays(seed, R):
    ro, rd = MR.span_rays(np.random.default_rng(seed), R)
    return ro, rd


@pytest.mark.parametrize("R", [1, 65, 300])
@pytest.mark.parametrize("name", ["ico", "spot"])
def test_hits_vs_rule(dev, name, R):
    sc = scene(dev, name)
    ro, rd = _camera_like_rays(1000 * R + len(name), R)
    hits = 0
    for near, far in ((0.5, 2.5), (0.0, 1.25)):
        want = _rule(sc, ro, rd, near, far)
        got = _raw_hit(dev, sc[0], ro, rd, near, far)
        for k, what in enumerate(("hit", "t", "face", "uv")):
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, near, far, np.flatnonzero((got[k] != want[k]).reshape(R, -1).any(1)))
        assert np.array_equal(_raw_hit(dev, sc[0], ro, rd, near, far, mode=1)[0], want[0])          # mode 1: the same flag, nothing else stored
        hits += int(want[0].sum())
    assert R == 1 or hits > 0
    if R == 300:
        assert 0 < want[0].sum() < R and not want[0][-9:][[8, 7, 2, 0]].any()          # NaN direction, a miss of the box, zero direction, looking away


def test_hits_from_inside_and_own_face(dev):
    """Rays that start on the surface of the icosphere, at the centroid of face r, along and against its normal: without own_face they
    meet their own triangle at t ~ 0; with it the ray along -n crosses the ball to the far wall and the one along +n misses."""
    sc = scene(dev, "ico")
    tracer, v, f = sc[0], sc[1], sc[2]
    c = v[f].mean(1).astype(f32)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n = (n * np.sign((n * c).sum(1, keepdims=True))).astype(f32)     # outward, whatever the winding
    ro, rd = np.concatenate([c, c]), np.concatenate([-n, n]).astype(f32) * f32(40)
    own = np.concatenate([np.arange(len(f)), np.arange(len(f))])
    own[3], own[7] = -1, len(f)                                        # two entries outside [0, F): nothing is skipped for them
    for near, far in ((0.0, 3.0), (-0.25, 0.5)):
        for o in (None, own):
            want = _rule(sc, ro, rd, near, far, own=o)
            got = _raw_hit(dev, tracer, ro, rd, near, far, own=o)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (near, far, o is None)
            assert np.array_equal(_raw_hit(dev, tracer, ro, rd, near, far, own=o, mode=1)[0], want[0])
    F = len(f)
    owned = np.setdiff1d(np.arange(F), [3, 7])
    hit, t, face, _ = _rule(sc, ro, rd, -0.25, 0.5, own=own)          # the far wall is beyond 0.5: only the rays without an own face hit
    assert not hit[owned].any() and not hit[F:].any()
    assert hit[[3, 7]].all() and face[[3, 7]].tolist() == [3, 7] and np.all(np.abs(t[[3, 7]]) < 1e-5)
    hit, t, face, _ = _rule(sc, ro, rd, 0.0, 3.0, own=own)
    assert hit[owned].all() and np.all(t[owned] > 0.5) and np.all(face[owned] != owned)          # the far wall, not the ray's own face
    assert not hit[F:].any()                                          # outward: nothing
    # the wrapper: int64 faces, barycentrics that sum to one on a hit and are zero on a miss
    h2, t2, f2, bary = tracer.trace(_t(dev, ro), _t(dev, rd), 0.0, 3.0, own_face=_t(dev, own))
    assert f2.dtype == torch.int64 and np.array_equal(f2.cpu().numpy(), face) and np.array_equal(h2.cpu().numpy(), hit) and np.array_equal(t2.cpu().numpy(), t)
    bary = bary.cpu().numpy()
    assert bary.shape == (2 * F, 3) and not bary[hit == 0].any() and np.all(np.abs(bary[hit == 1].sum(1) - 1) < 1e-6)
    occ = tracer.occluded(_t(dev, ro), _t(dev, rd), 0.0, 3.0, own_face=_t(dev, own))
    assert occ.dtype == torch.uint8 and np.array_equal(occ.cpu().numpy(), hit)


def test_hits_large_batch_equals_chunks(dev):
    """R = 2048 * 256 + 3: three rays more than one pass of the capped grid.  Against the same rays traced in chunks, and the rule on 300."""
    sc = scene(dev, "spot")
    tracer = sc[0]
    R = 2048 * 256 + 3
    rng = np.random.default_rng(11)
    base_o, base_d = MR.span_rays(rng, 4099)
    k = rng.integers(0, 4099, R)
    ro = (base_o[k] + rng.normal(0, 0.02, (R, 3))).astype(f32)
    rd = (base_d[k] + rng.normal(0, 0.02, (R, 3))).astype(f32)
    t_o, t_d = _t(dev, ro), _t(dev, rd)
    whole = tracer.trace(t_o, t_d, 0.5, 2.5)
    cut = [0, 1, 70000, 70001 + 256 * 1024, R]
    parts = [tracer.trace(t_o[a:b].contiguous(), t_d[a:b].contiguous(), 0.5, 2.5) for a, b in zip(cut[:-1], cut[1:])]
    for j in range(4):
        assert torch.equal(whole[j], torch.cat([p[j] for p in parts]))
    assert torch.equal(tracer.occluded(t_o, t_d, 0.5, 2.5), whole[0]) and 0 < int(whole[0].sum()) < R
    pick = np.concatenate([np.arange(100), R // 2 + np.arange(100), R - 100 + np.arange(100)])
    want = _rule(sc, ro[pick], rd[pick], 0.5, 2.5)
    assert np.array_equal(whole[0].cpu().numpy()[pick], want[0]) and np.array_equal(whole[1].cpu().numpy()[pick], want[1])
    assert np.array_equal(whole[2].cpu().numpy()[pick], want[2])


def test_hit_refusals_and_empty_batch(dev):
    from contexture_nerf_amd import _lib as L, volume_render as vr
    lib = L.load()
    tracer = scene(dev, "ico")[0]
    ro, rd = (_t(dev, x) for x in MR.span_rays(np.random.default_rng(0), 4))
    hit, t = Out(dev, (4,), torch.uint8, 0xA5), Out(dev, (4,), torch.float32, 0xA5)
    face, uv = Out(dev, (4,), torch.int32, 0xA5), Out(dev, (4, 2), torch.float32, 0xA5)
    box = [float(x) for k in ("lo", "hi", "inv", "h") for x in getattr(tracer, k)]
    good = [L.ptr(ro), L.ptr(rd), 4, 0.5, 2.5, L.ptr(tracer.cells), tracer.G, *box, L.ptr(tracer.cell_off), L.ptr(tracer.cell_tri),
            tracer.cell_tri.numel(), L.ptr(tracer.tri), L.ptr(tracer.faces), tracer.faces.shape[0], None, 0, L.ptr(hit.t), L.ptr(t.t), L.ptr(face.t),
            L.ptr(uv.t), L.stream()]
    cases = [({k: None}, "null") for k in (0, 1, 5, 19, 22, 23, 27, 28, 29, 30)]
    cases += [({2: -1}, "R="), ({6: 0}, "outside [1, 256]"), ({6: 257}, "outside [1, 256]"), ({26: 2}, "mode="), ({24: 0}, "F="), ({21: -1}, "n="),
              ({3: 2.5, 4: 0.5}, "near < far"), ({3: 1.0, 4: 1.0}, "near < far"), ({3: float('nan')}, "near < far"), ({4: float('inf')}, "near < far"),
              ({22: tracer.tri.data_ptr() + 4}, "aligned")]
    for change, needle in cases:
        a = list(good)
        for k, val in change.items():
            a[k] = val
        rc = lib.ctx_mesh_ray_hit(*a)
        assert rc != 0 and needle.encode() in lib.ctx_last_error(), (change, lib.ctx_last_error())
    a = list(good); a[2] = 0
    assert lib.ctx_mesh_ray_hit(*a) == 0                                # R = 0 launches nothing
    for x in (hit, t, face, uv):
        x.untouched("mesh_ray_hit")
    empty = tracer.trace(ro[:0], rd[:0], 0.5, 2.5)
    assert [tuple(x.shape) for x in empty] == [(0,), (0,), (0,), (0, 3)] and tuple(tracer.occluded(ro[:0], rd[:0], 0.5, 2.5).shape) == (0,)
    with pytest.raises(L.CtxError, match="near < far"):
        tracer.trace(ro, rd, 2.5, 0.5)
    with pytest.raises(L.CtxError, match="own_face"):
        tracer.trace(ro, rd, 0.5, 2.5, own_face=torch.zeros(3, dtype=torch.int64, device=dev))
    with pytest.raises(L.CtxError, match="dtype"):
        tracer.occluded(ro.double(), rd.double(), 0.5, 2.5)
    count = torch.zeros(8, dtype=torch.int32, device=dev)
    v, f = tracer.faces[:1].float().contiguous(), tracer.faces[:1]
    assert lib.ctx_mesh_cells_count(L.ptr(v), L.ptr(f), 3, 1, 0, -1., -1., -1., 1., 1., 1., L.ptr(count), L.stream()) != 0 and b"outside [1, 256]" in lib.ctx_last_error()
    assert lib.ctx_mesh_cells_count(L.ptr(v), L.ptr(f), 3, 0, 2, -1., -1., -1., 1., 1., 1., L.ptr(count), L.stream()) != 0 and b"at least one" in lib.ctx_last_error()
    assert lib.ctx_mesh_cells_scan(L.ptr(count), 0, L.ptr(count), L.ptr(count), L.stream()) != 0 and b"ncell=" in lib.ctx_last_error()
    assert lib.ctx_mesh_tri_setup(L.ptr(v), L.ptr(f), 3, 1, None, L.stream()) != 0 and b"null" in lib.ctx_last_error()
    with pytest.raises(L.CtxError, match="device tensor"):
        vr.MeshTracer(v.cpu(), f.cpu(), 4)


# ---- 3. bake with visibility --------------------------------------------------------------------------------------------------------------
class ConstantField:
    """One colour and one large density everywhere."""

    def forward_pts(self, pts):
        return torch.tensor([0.2, 0.5, 0.8, 1000.0], dtype=pts.dtype, device=pts.device).expand(pts.shape[0], 4).contiguous()


def test_bake_visibility_under_a_wall(dev):
    """A flat square (two triangles, its own atlas) and a small wall half a shell above part of it, with vertex ids of its own."""
    from contexture_nerf_amd import volume_render as vr
    T, G = 32, 16
    shell = 1.5 * 2.0 / G
    z = f32(0.5 * shell)
    v = f32([[-.5, -.5, 0], [.5, -.5, 0], [.5, .5, 0], [-.5, .5, 0], [.1, .1, z], [.4, .1, z], [.4, .4, z], [.1, .4, z]])
    f = np.int64([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]])
    vt = f32([[.05, .05], [.8, .05], [.8, .8], [.05, .8], [.85, .85], [.95, .85], [.95, .95], [.85, .95]])
    tface, tbary = UG.texel_map(vt, f, T)
    ground = (tface == 0) | (tface == 1)
    p = np.einsum('yxk,yxkc->yxc', tbary.astype(np.float64), v[f[np.clip(tface, 0, 3)]].astype(np.float64))          # the texel's surface point
    inside = ground & np.all((p[..., :2] > 0.1) & (p[..., :2] < 0.4), -1)
    margin = np.abs(p[..., :2, None] - np.float64([0.1, 0.4])).min((-1, -2))
    assert np.all(margin[ground] > 1e-3) and 30 < inside.sum() < ground.sum() / 4 and (tface >= 2).sum() > 4          # no texel sits on the wall's outline
    ten = [_t(dev, v), _t(dev, f), _t(dev, vt[f]), _t(dev, tface), _t(dev, tbary)]
    tracer = vr.MeshTracer(ten[0], ten[1], G, -1.0, 1.0)
    grid = tracer.occupancy(1)
    field = ConstantField()
    plain = vr.bake_atlas(field, *ten, grid, shell=shell, supersample=1)
    seen = vr.bake_atlas(field, *ten, grid, shell=shell, supersample=1, visibility=tracer)
    under = _t(dev, inside)
    assert bool((plain[3][under] > 0).all())                          # without visibility the covered texels carry the wall
    assert bool((seen[:, under] == 0).all())                          # with it they get nothing
    assert torch.equal(seen[:, ~under], plain[:, ~under]) and bool((seen[3][_t(dev, tface >= 0) & ~under] > 0).all())
    # sub-samples: a texel keeps what its unblocked sub-samples give; only texels with a blocked sub-sample change
    plain2 = vr.bake_atlas(field, *ten, grid, shell=shell, supersample=2)
    seen2 = vr.bake_atlas(field, *ten, grid, shell=shell, supersample=2, visibility=tracer)
    changed = (seen2 != plain2).any(0)
    near_wall = _t(dev, ground & np.all((p[..., :2] > 0.1 - 0.05) & (p[..., :2] < 0.4 + 0.05), -1))
    assert bool(changed.any()) and not bool((changed & ~near_wall).any())
    deep = _t(dev, ground & np.all((p[..., :2] > 0.15) & (p[..., :2] < 0.35), -1))
    assert bool((seen2[:, deep] == 0).all()) and bool(deep.any())


# ---- 4. training ------------------------------------------------------------------------------------------------------------------------------
def _ico_tracer(dev, G=16):
    from contexture_nerf_amd import volume_render as vr
    v, f = MR.icosphere(2, 0.6)
    return vr.MeshTracer(_t(dev, v), _t(dev, f), G, -1.0, 1.0)


def _batch(dev, R=96, seed=3):
    import test_occupancy_cpu as OC
    ro, rd, _ = OG._dev(dev, *OC.random_rays(np.random.default_rng(seed), R, 8))
    return ro, rd, torch.rand(R, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))


@pytest.mark.parametrize("marched", [False, True])
def test_train_step_with_zero_weights_is_todays_step(dev, marched):
    from contexture_nerf_amd import volume_render as vr
    tracer = _ico_tracer(dev)
    grid = tracer.occupancy(1)
    ro, rd, target = _batch(dev)
    kw = dict(occupancy=grid, march=float(grid.h[0]) / 2) if marched else dict(N_importance=8)
    params = []
    for extra in ({}, dict(mesh=tracer), dict(mesh=tracer, mask_weight=0.5, depth_weight=0.5)):
        field = OG._field(dev, seed=4)
        opt = torch.optim.Adam(field.parameters(), lr=1e-3)
        res = vr.train_step(field, opt, ro, rd, target, 0.5, 2.5, 32, raw_noise_std=1., generator=torch.Generator(device=dev).manual_seed(1), **kw, **extra)
        assert ('mask' in res) == ('mask_weight' in extra)
        params.append([p.detach().clone() for p in field.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(params[0], params[1]))
    assert any(not torch.equal(a, b) for a, b in zip(params[0], params[2]))             # and the terms, once weighted, do reach the parameters


@pytest.mark.parametrize("marched", [False, True])
def test_train_step_reports_the_formulas(dev, marched):
    from contexture_nerf_amd import run_nerf_helpers as rnh, volume_render as vr
    tracer = _ico_tracer(dev)
    grid = tracer.occupancy(1)
    ro, rd, target = _batch(dev, seed=5)
    kw = dict(occupancy=grid, march=float(grid.h[0]) / 2) if marched else dict(N_importance=8)
    field = OG._field(dev, seed=6, sigma_bias=4.0)
    out = [x.detach() for x in rnh.render_rays(field, ro, rd, 0.5, 2.5, 32, perturb=0., **kw)]          # with the graph, as the step renders
    img = rnh.img2mse(out[0], target)
    hit, t = tracer.trace(ro, rd, 0.5, 2.5)[:2]
    assert 0 < int(hit.sum()) < len(hit)
    hitf = hit.float()
    mask = ((out[2] - hitf) ** 2).mean()
    depth = (hitf * (out[4] - t) ** 2).sum() / hitf.sum().clamp(min=1.)
    opt = torch.optim.SGD(field.parameters(), lr=0.0)
    res = vr.train_step(field, opt, ro, rd, target, 0.5, 2.5, 32, perturb=0., mesh=tracer, mask_weight=0.25, depth_weight=2.0, **kw)
    assert torch.equal(res['mask'], mask) and torch.equal(res['depth'], depth) and float(mask) > 0 and float(depth) > 0
    if marched:                                                       # one pass: the loss is the image term plus the two weighted terms
        assert torch.equal(res['loss'], img + 0.25 * mask + 2.0 * depth)
    pair = vr.train_step(field, opt, ro, rd, target, 0.5, 2.5, 32, perturb=0., mesh=(hit, t), mask_weight=0.25, depth_weight=2.0, **kw)
    assert torch.equal(pair['loss'], res['loss']) and torch.equal(pair['mask'], mask)


def test_fit_views_mask_term_falls(dev):
    """40 iterations on the icosphere: the views are the tracer's own silhouettes (a flat colour on white), the student a small
    HashGridField marched through the shell grid."""
    from contexture_nerf_amd import run_nerf_helpers as rnh, volume_render as vr
    from contexture_nerf_amd.hashgrid import HashGridField
    tracer = _ico_tracer(dev)
    grid = tracer.occupancy(1)
    H = W = 24
    K = vr.pinhole(H, W)
    c2ws = torch.tensor([[[1., 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1.5]], [[0., 0, 1, 1.5], [0, 1, 0, 0], [-1, 0, 0, 0]]], device=dev)
    imgs = []
    for k in range(2):
        ro, rd = rnh.get_rays(H, W, K, c2ws[k])
        hit = tracer.occluded(ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous(), 0.5, 2.5).reshape(H, W, 1).float()
        imgs.append(hit * torch.tensor([0.8, 0.3, 0.2], device=dev) + (1 - hit))
    imgs = torch.stack(imgs)
    assert 0.1 < float((imgs[..., 1] < 0.5).float().mean()) < 0.9
    seen = []
    step = vr.train_step

    def spy(*a, **k):
        seen.append(step(*a, **k))
        return seen[-1]
    torch.manual_seed(2)
    student = HashGridField.from_grid(grid, n_levels=4, n_features=2, log2_table=10, base_res=4, max_res=32).to(dev)
    with torch.no_grad():
        student.mlp.output_linear.bias[3] = 1.0                       # some density to start from: a field that begins at zero has no gradient
    vr.train_step = spy
    try:
        hist = vr.fit_views(student, imgs, c2ws, K, 0.5, 2.5, 40, rays_per_iter=256, lr=1e-2, seed=3, white_bkgd=True, occupancy=grid, occupancy_every=0,
                            march=float(grid.h[0]) / 2, mesh=tracer, mask_weight=1.0, depth_weight=0.1)
    finally:
        vr.train_step = step
    masks = [float(s['mask']) for s in seen]
    print(f"fit_views(mesh=): mask first five {np.mean(masks[:5]):.4f}, last five {np.mean(masks[-5:]):.4f}; depth {float(seen[0]['depth']):.4f} -> "
          f"{float(seen[-1]['depth']):.4f}")
    assert len(hist) == 40 and all(np.isfinite(hist)) and all(np.isfinite(masks))
    assert np.mean(masks[-5:]) < np.mean(masks[:5])
