"""CPU: the ray / mesh intersector's rule (tests/meshhit_rule.py) and the host control flow around it.

1. lists: count > 0 is the voxeliser's grid, every segment ascends, the walk with the cell index is occ_ray_spans_np's walk;
2. the grid walk with its early stop against the same arithmetic over all triangles: equal on every ray, no exclusions;
3. against a float64 all-triangles reference, on the rays that neither graze a triangle nor pass within 1e-3 of an edge;
4. hand cases of the triangle test, the tie rule, near / far, own_face and the refused rays;
5. host: MeshTracer, train_step / fit_views(mesh=), bake_atlas(visibility=) with the device seams stubbed: the defaults pass nothing new
   down, the refusals fire."""
import types
import numpy as np
import pytest
import torch

import meshhit_rule as MR

f32 = np.float32


# ---- shared inputs: computed once, never modified ---------------------------------------------------------------------------------------
def _rays(seed, R, origin="outside"):
    """Rays towards the mesh: from a shell of radius 1.4 .. 1.7 around it aimed at points of the ball of radius 0.7 (`outside`), or
    from points inside the ball of radius 0.3 in every direction (`inside`), plus span_rays' special rays at the end."""
    rng = np.random.default_rng(seed)
    if origin == "outside":
        o = rng.normal(size=(R, 3)); o = o / np.linalg.norm(o, axis=1, keepdims=True) * rng.uniform(1.4, 1.7, (R, 1))
        aim = rng.normal(size=(R, 3)); aim = aim / np.linalg.norm(aim, axis=1, keepdims=True) * 0.7 * rng.uniform(0, 1, (R, 1)) ** (1 / 3)
        d = aim - o
        d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (R, 1))
    else:
        o = rng.normal(size=(R, 3)); o = o / np.linalg.norm(o, axis=1, keepdims=True) * 0.3 * rng.uniform(0, 1, (R, 1)) ** (1 / 3)
        d = rng.normal(size=(R, 3))
    ro, rd = o.astype(f32), d.astype(f32)
    so, sd = MR.span_rays(rng, 10)                                    # one ordinary ray, then the nine special ones
    ro[-9:], rd[-9:] = so[-9:], sd[-9:]
    return ro, rd


_CASES = {}


def case(name):
    """(v, f, G, lo3, hi3, inv, h, lists, tri, ro, rd, near, far) of a named case, built on first use and shared."""
    if name not in _CASES:
        mesh, G, origin, seed = {"ico8": ("ico", 8, "outside", 1), "ico16": ("ico", 16, "outside", 2), "ico8_in": ("ico", 8, "inside", 3),
                                 "ico16_in": ("ico", 16, "inside", 4), "spot32": ("spot", 32, "outside", 5)}[name]
        v, f = MR.icosphere(2, 0.6) if mesh == "ico" else MR.spot_mesh()
        lo3, inv, h = MR.grid_consts(G, -1.0, 1.0)
        hi3 = f32([1, 1, 1])
        lists = MR.mesh_cells_np(v, f, G, lo3, inv)
        ro, rd = _rays(seed, 1500, origin)
        near, far = (0.0, 4.0) if origin == "outside" else (0.0, 3.0)
        _CASES[name] = (v, f, G, lo3, hi3, inv, h, lists, MR.tri_records_np(v, f), ro, rd, near, far)
    return _CASES[name]


_GRID_HITS = {}


def grid_hits(name):
    if name not in _GRID_HITS:
        v, f, G, lo3, hi3, inv, h, lists, tri, ro, rd, near, far = case(name)
        st = {}
        _GRID_HITS[name] = MR.mesh_hit_grid_np(ro, rd, near, far, lists, tri, f, G, lo3, hi3, inv, h, stats=st) + (st,)
    return _GRID_HITS[name]


# ---- 1. lists ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ico8", "ico16", "spot32"])
def test_lists_are_the_voxelisers_cells_and_ascend(name):
    v, f, G, lo3, hi3, inv, h, (count, cell_off, cell_tri), tri, ro, rd, near, far = case(name)
    cells = MR.occ_voxelize_np(v, f, G, lo3, inv)
    assert count.dtype == np.int32 and cell_off.dtype == np.int32 and cell_tri.dtype == np.int32
    assert np.array_equal((count > 0).reshape(G, G, G), cells != 0)
    assert cell_off[0] == 0 and cell_off[-1] == len(cell_tri) == count.sum() and np.array_equal(np.diff(cell_off), count)
    inside = np.ones(len(cell_tri), bool); inside[cell_off[:-1][count > 0]] = False            # not the first entry of a segment
    assert np.all(np.diff(cell_tri.astype(np.int64))[inside[1:]] > 0)                         # strictly ascending within every segment
    assert cell_tri.min() >= 0 and cell_tri.max() < len(f) and len(np.unique(cell_tri)) == len(f)          # every face is listed somewhere
    occupied = count[count > 0]
    print(f"{name}: {len(cell_tri)} entries, mean list {occupied.mean():.1f}, max {occupied.max()}")


def test_lists_skip_bad_faces_and_records_are_nan_there():
    G = 4
    lo3, inv, _ = MR.grid_consts(G, -1.0, 1.0)
    v = f32([[0.1, 0.1, 0.1], [0.4, 0.1, 0.1], [0.1, 0.4, 0.1], [np.nan, 0, 0], [np.inf, 0, 0]])
    f = np.int64([[0, 1, 3], [0, 1, 2], [0, 4, 2], [-1, 1, 2], [0, 1, 5]])
    count, cell_off, cell_tri = MR.mesh_cells_np(v, f, G, lo3, inv)
    assert set(cell_tri.tolist()) == {1} and count.sum() == len(cell_tri) >= 1
    tri = MR.tri_records_np(v, f)
    assert tri.dtype == f32 and tri.shape == (5, 12)
    assert np.all(np.isnan(tri[[0, 2, 3, 4]])) and np.array_equal(tri[1], f32([0.1, 0.1, 0.1, 0, 0.4 - 0.1, 0, 0, 0, 0, 0.4 - 0.1, 0, 0]).astype(f32))
    assert np.array_equal(tri[1, 4:7], v[1] - v[0]) and np.array_equal(tri[1, 8:11], v[2] - v[0])


@pytest.mark.parametrize("name", ["ico8", "ico16_in", "spot32"])
def test_walk_with_cells_is_the_span_walk(name):
    v, f, G, lo3, hi3, inv, h, (count, _, _), tri, ro, rd, near, far = case(name)
    cells = (count > 0).reshape(G, G, G).astype(np.uint8)
    steps = MR.walk_cells_np(ro, rd, near, far, cells, lo3, hi3, inv, h)
    span, hit = MR.spans_from_cells_walk(steps, len(ro), near, far)
    want_span, want_hit = MR.occ_ray_spans_np(ro, rd, near, far, cells, lo3, hi3, inv, h)
    assert np.array_equal(span, want_span) and np.array_equal(hit, want_hit) and 0 < hit.sum() < len(ro)
    for occ, cell, _, _, visit in steps:
        assert np.all((cell >= 0) & (cell < G ** 3)) and np.array_equal(occ, visit & (cells.reshape(-1)[cell] != 0))


# ---- 2. grid walk with early stop == all triangles -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ico8", "ico16", "ico8_in", "ico16_in", "spot32"])
def test_grid_walk_equals_all_triangles(name):
    v, f, G, lo3, hi3, inv, h, lists, tri, ro, rd, near, far = case(name)
    hit, t, face, uv, st = grid_hits(name)
    a_hit, a_t, a_face, a_uv = MR.mesh_hit_all_np(ro, rd, near, far, tri, f)
    assert hit.dtype == np.uint8 and t.dtype == f32 and face.dtype == np.int32 and uv.dtype == f32 and uv.shape == (len(ro), 2)
    assert np.array_equal(hit, a_hit), np.flatnonzero(hit != a_hit)
    assert np.array_equal(face, a_face), np.flatnonzero(face != a_face)
    assert np.array_equal(t, a_t) and np.array_equal(uv, a_uv)
    assert 0.3 * len(ro) < hit.sum() < len(ro)                        # hits and misses
    assert np.all(t[hit == 0] == f32(far)) and np.all(face[hit == 0] == -1) and not uv[hit == 0].any()
    assert not hit[-9:][[8, 7, 2, 0]].any()                           # NaN direction, a miss of the box, zero direction, looking away
    assert st['tests'] < 0.25 * len(ro) * len(f)                      # the grid does prune
    # mode 1 (any) gives the same flag
    any_hit = MR.mesh_hit_grid_np(ro, rd, near, far, lists, tri, f, G, lo3, hi3, inv, h, mode=1)[0]
    assert np.array_equal(any_hit, hit)
    print(f"{name}: {int(hit.sum())} of {len(ro)} rays hit, {st['tests'] / len(ro):.1f} triangle tests per ray (all triangles: {len(f)})")


# ---- 3. against float64 over all triangles --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ico8", "ico16", "ico8_in", "ico16_in", "spot32"])
def test_grid_walk_vs_float64_reference(name):
    v, f, G, lo3, hi3, inv, h, lists, tri, ro, rd, near, far = case(name)
    hit, t, face, uv, _ = grid_hits(name)
    tri64 = MR.tri_records_np(v, f, np.float64)
    fin = np.all(np.isfinite(ro), 1) & np.all(np.isfinite(rd), 1)
    r64_hit, r64_t, r64_face, _ = MR.mesh_hit_all_np(np.where(fin[:, None], ro, 0), np.where(fin[:, None], rd, 0), near, far, tri64, f, dtype=np.float64)
    keep = MR.judged_rays_np(np.where(fin[:, None], ro, 0), np.where(fin[:, None], rd, 0), near, far, tri64) & fin
    excluded = 1.0 - keep.sum() / fin.sum()
    rel = np.abs(t[keep].astype(np.float64) - r64_t[keep]) / (1.0 + r64_t[keep])
    worst = rel[r64_hit[keep] != 0].max()
    print(f"{name}: excluded {excluded:.2%}, hit/face mismatches {int((hit[keep] != r64_hit[keep]).sum())}/{int((face[keep] != r64_face[keep]).sum())}, "
          f"largest |t - t64| / (1 + t64) = {worst:.2e}")
    assert excluded <= 0.05
    assert np.array_equal(hit[keep], r64_hit[keep]) and np.array_equal(face[keep], r64_face[keep])
    assert np.all(rel <= 4e-6)


# ---- 4. hand cases ---------------------------------------------------------------------------------------------------------------------------
def _scene(v, f, G=4):
    lo3, inv, h = MR.grid_consts(G, -1.0, 1.0)
    v, f = f32(v), np.int64(f)
    return dict(lists=MR.mesh_cells_np(v, f, G, lo3, inv), tri=MR.tri_records_np(v, f), faces=f, G=G, lo=lo3, hi=f32([1, 1, 1]), inv=inv, h=h)


def _hit(sc, o, d, near=0.0, far=4.0, own=None, mode=0):
    o, d = f32(o).reshape(-1, 3), f32(d).reshape(-1, 3)
    own = None if own is None else np.int64(own).reshape(-1)
    got = MR.mesh_hit_grid_np(o, d, near, far, sc['lists'], sc['tri'], sc['faces'], sc['G'], sc['lo'], sc['hi'], sc['inv'], sc['h'], own_face=own, mode=mode)
    want = MR.mesh_hit_all_np(o, d, near, far, sc['tri'], sc['faces'], own_face=own)
    if mode == 0:
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    else:
        assert np.array_equal(got[0], want[0])
    return got


# a square of two coplanar triangles in z = 0.25 sharing the edge (0,0)-(0.5,0.5), a fan of four around the vertex (0.25, -0.25), and a
# second square at z = -0.25 (same layout: faces 6, 7)
_V = [[0, 0, .25], [.5, 0, .25], [.5, .5, .25], [0, .5, .25],
      [.25, -.25, .25], [0, -.5, .25], [.5, -.5, .25], [.5, 0, .25], [0, 0, .25],
      [0, 0, -.25], [.5, 0, -.25], [.5, .5, -.25], [0, .5, -.25]]
_F = [[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7], [4, 7, 8], [4, 8, 5], [9, 10, 11], [9, 11, 12]]


def test_hand_cases_edges_vertices_and_ties():
    sc = _scene(_V, _F)
    down = [0, 0, -1]
    # through the shared edge of the coplanar faces 0 and 1: both accept with the same t, the lower id wins
    hit, t, face, uv = _hit(sc, [0.25, 0.25, 1.0], down)
    assert hit[0] == 1 and face[0] == 0 and t[0] == f32(0.75)
    ok = MR.tri_test_np(f32([0.25, 0.25, 1.0]), f32(down), sc['tri'][:2], 0.0, 4.0)[0]
    assert ok.tolist() == [True, True]
    # through the shared vertex of the fan 2..5: all four accept, face 2 is reported
    hit, t, face, uv = _hit(sc, [0.25, -0.25, 1.0], down)
    assert hit[0] == 1 and face[0] == 2 and t[0] == f32(0.75) and uv[0].tolist() == [0.0, 0.0]
    assert MR.tri_test_np(f32([0.25, -0.25, 1.0]), f32(down), sc['tri'][2:6], 0.0, 4.0)[0].all()
    # inside face 1 only
    hit, t, face, uv = _hit(sc, [0.125, 0.375, 1.0], down)
    assert hit[0] == 1 and face[0] == 1
    # a back face counts: from below, the lower square first, then (with near past it) the upper one from its back
    hit, t, face, _ = _hit(sc, [0.375, 0.125, -1.0], [0, 0, 1])
    assert hit[0] == 1 and face[0] == 6 and t[0] == f32(0.75)
    hit, t, face, _ = _hit(sc, [0.375, 0.125, -1.0], [0, 0, 1], near=1.0)
    assert hit[0] == 1 and face[0] == 0 and t[0] == f32(1.25)         # the hit before near is skipped and the next one is found
    # a hit beyond far is skipped: far between the two squares, then before both
    hit, t, face, _ = _hit(sc, [0.375, 0.125, 1.0], down, far=1.0)
    assert hit[0] == 1 and face[0] == 0
    hit, t, face, uv = _hit(sc, [0.375, 0.125, 1.0], down, far=0.5)
    assert hit[0] == 0 and t[0] == f32(0.5) and face[0] == -1 and not uv.any()
    # t == near and t == far are inside the range
    assert _hit(sc, [0.375, 0.125, 1.0], down, near=0.75, far=1.0)[2][0] == 0
    assert _hit(sc, [0.375, 0.125, 1.0], down, near=0.5, far=0.75)[2][0] == 0
    # a ray parallel to the squares, in the plane of the upper one: det = 0 for each of its triangles, a miss
    det = MR.tri_terms_np(f32([-0.9, 0.25, 0.25]), f32([1, 0, 0]), sc['tri'])[0]
    assert np.all(det == 0)
    assert _hit(sc, [-0.9, 0.25, 0.25], [1, 0, 0])[0][0] == 0
    # NaN and zero-direction rays, a NaN origin and a ray that misses the box are misses
    o = [[0.25, 0.25, 1.0], [0.25, 0.25, 0.5], [np.nan, 0.25, 1.0], [0.25, 3.0, 1.0]]
    d = [[np.nan, 0, -1], [0, 0, 0], [0, 0, -1], [0, 0, -1]]
    hit, t, face, uv = _hit(sc, o, d)
    assert not hit.any() and np.all(t == f32(4.0)) and np.all(face == -1) and not uv.any()
    # mode 1 reports the flag alone
    assert _hit(sc, [[0.25, 0.25, 1.0], [0.9, 0.9, 1.0]], [down, down], mode=1)[0].tolist() == [1, 0]


def test_hand_cases_own_face():
    sc = _scene(_V, _F)
    up = [0, 0, 1]
    # the origin on face 6 (the lower square), looking up at the upper square
    o = [0.375, 0.125, -0.25]
    hit, t, face, _ = _hit(sc, o, up)
    assert hit[0] == 1 and face[0] == 6 and t[0] == 0                 # without own_face the ray meets its own triangle at t = 0
    hit, t, face, _ = _hit(sc, o, up, own=[6])
    assert hit[0] == 1 and face[0] == 0 and t[0] == f32(0.5)           # with it, the next wall
    # a related neighbour is skipped too: on the shared edge of 6 and 7, own = 7 skips both (they share vertex ids 9 and 11)
    o = [0.25, 0.25, -0.25]
    assert _hit(sc, o, up)[2][0] == 6
    assert _hit(sc, o, up, own=[7])[2][0] == 0
    # faces 0 and 4 touch in space (vertices 0 and 8, 1 and 7 coincide) but share no vertex ID: not related, so own = 4 does not skip 0
    assert _hit(sc, [0.375, 0.125, 1.0], [0, 0, -1], own=[4])[2][0] == 0
    assert _hit(sc, [0.375, 0.125, 1.0], [0, 0, -1], own=[1])[2][0] == 6          # own = 1 skips 0 as well: the lower square is next
    # an own_face outside [0, F) skips nothing
    assert _hit(sc, [0.375, 0.125, 1.0], [0, 0, -1], own=[-1])[2][0] == 0
    assert _hit(sc, [0.375, 0.125, 1.0], [0, 0, -1], own=[99])[2][0] == 0
    # mode 1 honours own_face
    assert _hit(sc, [[0.375, 0.125, -0.25]] * 2, [up, up], far=0.25, own=[6, -1], mode=1)[0].tolist() == [0, 1]


# ---- 5. host ---------------------------------------------------------------------------------------------------------------------------------
class _Opt:
    def zero_grad(self, set_to_none=True):
        pass

    def step(self):
        pass


def _fake_render(seen):
    def render(field, ro, rd, near, far, N, **k):
        seen.append(k)
        R = ro.shape[0]
        w = torch.full((R, 3), 0.5, requires_grad=True)
        acc, depth = w[:, 0] * 1.0, w[:, 1] * 3.0
        return (w, w[:, 0], acc, w, depth), {}
    return render


class _Tracer:
    def __init__(self):
        self.calls = []

    def trace(self, ro, rd, near, far, own_face=None):
        self.calls.append(('trace', ro.shape[0], near, far))
        R = ro.shape[0]
        hit = (torch.arange(R) % 2).to(torch.uint8)
        return hit, torch.full((R,), 2.0), torch.zeros(R, dtype=torch.int64), torch.zeros(R, 3)

    def occluded(self, ro, rd, near, far, own_face=None):
        self.calls.append(('occluded', ro.shape[0], near, far, None if own_face is None else own_face.tolist()))
        return (torch.arange(ro.shape[0]) % 2).to(torch.uint8)


def test_train_step_mesh_terms_and_defaults(monkeypatch):
    from contexture_nerf_amd import _lib as L, volume_render as vr
    seen = []
    monkeypatch.setattr(vr.rnh, 'render_rays', _fake_render(seen))
    ro, rd, tgt = torch.zeros(4, 3), torch.ones(4, 3), torch.zeros(4, 3)
    # the defaults: no new key, nothing traced
    res = vr.train_step(None, _Opt(), ro, rd, tgt, 0.5, 2.5, 4)
    assert set(res) == {'loss', 'psnr'}
    tr = _Tracer()
    base = float(res['loss'])
    res = vr.train_step(None, _Opt(), ro, rd, tgt, 0.5, 2.5, 4, mesh=tr)               # a tracer with both weights 0: nothing new runs
    assert set(res) == {'loss', 'psnr'} and tr.calls == [] and float(res['loss']) == base
    res = vr.train_step(None, _Opt(), ro, rd, tgt, 0.5, 2.5, 4, mesh=tr, mask_weight=2.0, depth_weight=0.5)
    assert tr.calls == [('trace', 4, 0.5, 2.5)]
    # acc = 0.5 everywhere, hit = 0 1 0 1: mask = 0.25; depth = 1.5 against 2.0 on the two hit rays: 0.25
    assert float(res['mask']) == 0.25 and float(res['depth']) == 0.25
    assert abs(float(res['loss']) - (base + 2.0 * 0.25 + 0.5 * 0.25)) < 1e-6
    assert not res['mask'].requires_grad and not res['depth'].requires_grad
    # a traced pair in place of the tracer (what fit_views hands down): the same numbers, nothing traced
    pair = tr.trace(ro, rd, 0.5, 2.5)[:2]
    tr.calls.clear()
    res2 = vr.train_step(None, _Opt(), ro, rd, tgt, 0.5, 2.5, 4, mesh=pair, mask_weight=2.0, depth_weight=0.5)
    assert tr.calls == [] and float(res2['loss']) == float(res['loss'])
    # only one weight: both means are still reported
    res = vr.train_step(None, _Opt(), ro, rd, tgt, 0.5, 2.5, 4, mesh=tr, mask_weight=1.0)
    assert abs(float(res['loss']) - (base + 0.25)) < 1e-6 and float(res['depth']) == 0.25
    # no hit at all: the depth term is 0 / max(1, 0)
    none = (torch.zeros(4, dtype=torch.uint8), torch.full((4,), 2.5))
    res = vr.train_step(None, _Opt(), ro, rd, tgt, 0.5, 2.5, 4, mesh=none, depth_weight=1.0)
    assert float(res['depth']) == 0.0 and float(res['mask']) == 0.25
    # refusals, by name
    with pytest.raises(L.CtxError, match="mask_weight=1.0 needs mesh="):
        vr.train_step(None, _Opt(), ro, rd, tgt, 0.5, 2.5, 4, mask_weight=1.0)
    with pytest.raises(L.CtxError, match="depth_weight=0.5 needs mesh="):
        vr.train_step(None, _Opt(), ro, rd, tgt, 0.5, 2.5, 4, depth_weight=0.5)
    with pytest.raises(L.CtxError, match="mask_weight=-1"):
        vr.train_step(None, _Opt(), ro, rd, tgt, 0.5, 2.5, 4, mesh=tr, mask_weight=-1)
    with pytest.raises(L.CtxError, match="depth_weight=nan"):
        vr.train_step(None, _Opt(), ro, rd, tgt, 0.5, 2.5, 4, mesh=tr, depth_weight=float('nan'))
    with pytest.raises(L.CtxError, match=r"hit \[4\] and t \[4\]"):
        vr.train_step(None, _Opt(), ro, rd, tgt, 0.5, 2.5, 4, mesh=(torch.zeros(3, dtype=torch.uint8), torch.zeros(3)), mask_weight=1.0)


def test_fit_views_traces_once_and_indexes(monkeypatch):
    from contexture_nerf_amd import _lib as L, volume_render as vr
    seen = []
    monkeypatch.setattr(vr.rnh, 'get_rays', lambda H, W, K, c2w: (torch.zeros(H, W, 3), torch.ones(H, W, 3)))

    def step(*a, **k):
        seen.append(k)
        return {'loss': torch.tensor(1.0)}
    monkeypatch.setattr(vr, 'train_step', step)
    field = torch.nn.Linear(3, 4)
    args = (field, torch.zeros(2, 4, 4, 3), torch.zeros(2, 3, 4), vr.pinhole(4, 4), 0.5, 2.5, 3)
    vr.fit_views(*args, rays_per_iter=8)
    assert all('mesh' not in k and 'mask_weight' not in k and 'depth_weight' not in k for k in seen) and len(seen) == 3          # nothing new is handed down
    seen.clear()
    tr = _Tracer()
    vr.fit_views(*args, rays_per_iter=8, mesh=tr)                                          # weights 0: not traced, nothing handed down
    assert tr.calls == [] and all('mesh' not in k for k in seen)
    seen.clear()
    vr.fit_views(*args, rays_per_iter=8, mesh=tr, mask_weight=0.5, depth_weight=0.25)
    assert tr.calls == [('trace', 2 * 4 * 4, 0.5, 2.5)]                                    # all V*H*W rays, once, before the loop
    assert len(seen) == 3
    for k in seen:
        hit, t = k['mesh']
        assert hit.shape == (8,) and t.shape == (8,) and k['mask_weight'] == 0.5 and k['depth_weight'] == 0.25
    with pytest.raises(L.CtxError, match="mask_weight=0.5 needs mesh="):
        vr.fit_views(*args, rays_per_iter=8, mask_weight=0.5)


def test_bake_atlas_visibility_host_flow(monkeypatch):
    from contexture_nerf_amd import kal, volume_render as vr
    T, s = 4, 2
    texel_face = torch.full((T, T), -1, dtype=torch.int64)
    texel_face[1, 1], texel_face[2, 3] = 5, 7
    seen = {}
    monkeypatch.setattr(kal, 'chart_texels', lambda tf: torch.nonzero(tf.reshape(-1) >= 0).reshape(-1).to(torch.int32))
    monkeypatch.setattr(kal, 'texel_rays', lambda tf, tb, fuv, v, f, part, ss, shell: (torch.zeros(part.numel() * ss * ss, 3), torch.ones(part.numel() * ss * ss, 3),
                                                                                       torch.ones(part.numel() * ss * ss, dtype=torch.uint8)))
    monkeypatch.setattr(vr.rnh, 'render_rays_marched', lambda field, ro, rd, near, far, occ, step, **k: (torch.zeros(ro.shape[0], 3), None, torch.ones(ro.shape[0]), None, None))

    def resolve(rgb, alpha, valid, part, ss, acc, min_alpha=0.5):
        seen['valid'] = valid.clone()
    monkeypatch.setattr(kal, 'bake_resolve', resolve)
    grid = types.SimpleNamespace(h=f32([0.5, 0.5, 0.5]))
    args = (None, torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64), torch.zeros(1, 3, 2), texel_face, torch.zeros(T, T, 3), grid)
    vr.bake_atlas(*args, shell=0.25, supersample=s)
    assert seen['valid'].tolist() == [1] * 8                                              # the default: no visibility, valid as texel_rays gave it
    tr = _Tracer()
    vr.bake_atlas(*args, shell=0.25, supersample=s, visibility=tr)
    assert tr.calls == [('occluded', 8, 0.0, 0.25, [5] * 4 + [7] * 4)]                    # the texel's face, repeated per sub-sample
    assert seen['valid'].dtype == torch.uint8 and seen['valid'].tolist() == [1, 0] * 4    # valid &= ~blocked


def test_mesh_tracer_refusals_on_the_host():
    from contexture_nerf_amd import _lib as L, volume_render as vr
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64)
    with pytest.raises(L.CtxError, match="device tensor"):
        vr.MeshTracer(v, f, 4)
    with pytest.raises(L.CtxError, match=r"vertices float32 \[V,3\]"):
        vr.MeshTracer(v.double(), f, 4)
    with pytest.raises(L.CtxError, match=r"faces int64 \[F,3\]"):
        vr.MeshTracer(v, f.int(), 4)
    with pytest.raises(L.CtxError, match="no face"):
        vr.MeshTracer(v, f[:0], 4)
    with pytest.raises(L.CtxError, match=r"outside \[1, 256\]"):
        vr.MeshTracer(v, f, 0)
