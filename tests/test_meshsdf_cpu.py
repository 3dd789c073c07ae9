"""CPU: the signed point / mesh query's rule (tests/meshsdf_rule.py) against truth and against itself, and the meshes
the GPU tests share.

1. the sign of the binary32 rule == the float64 generalised winding number on the points of test_meshdist_cpu.draw_points;
2. a spike where the winning face's own normal gives the wrong sign and the pseudonormal the right one;
3. a cube with dyadic coordinates: hand-placed points in all seven feature classes, with exact sdist, feature and grad;
4. the tables: the order of the sums, float32 against float64, open / non-manifold / zero-area / spoilt faces;
5. topology by hand;
6. the grid form == the all-triangles form (the statement of test_grid_form_finds_what_all_triangles_find) on sdist, feature and grad;
7. the ramp and its gradient;
8. the marched render of the solid icosphere by the rules: the silhouette, and the figure behind the GPU test's gate on the normals."""
import numpy as np
import pytest

import meshdist_rule as R
import meshsdf_rule as S
import test_meshdist_cpu as MC

f32 = np.float32
SIGNED_NAMES = ("found", "sdist", "face", "uv", "feature", "grad")
_CACHE = {}


def tables(name, dtype=f32):
    """The rule's tables of a test_meshdist_cpu scene, computed once."""
    key = ("pn", name, dtype)
    if key not in _CACHE:
        sc = MC.scene(name)
        _CACHE[key] = S.pseudonormals_np(sc['f'], len(sc['v']), sc['tri'] if dtype is f32 else sc['tri64'], dtype)
    return _CACHE[key]


def signed_case(name, mult):
    """-> dict(grid, all): the two signed forms on MC.case(name, mult), computed once."""
    key = ("signed", name, mult)
    if key not in _CACHE:
        sc, c = MC.scene(name), MC.case(name, mult)
        pn = tables(name)
        _CACHE[key] = dict(grid=S.sign_step_np(c['pts'], c['r'], c['grid'], sc['tri'], pn), all=S.sign_step_np(c['pts'], c['r'], c['all'], sc['tri'], pn))
    return _CACHE[key]


# ---- the hand-made meshes ------------------------------------------------------------------------------------------------------------------
def cube():
    """The cube [-1/2, 1/2]^3, vertex id = x + 2 y + 4 z (bits), twelve faces wound outward; faces 0 and 1 are the top (z = +1/2):
    face 0 = (4, 5, 7): v0 = (-,-,+), e1 = (1, 0, 0), e2 = (1, 1, 0); face 1 = (4, 7, 6): e1 = (1, 1, 0), e2 = (0, 1, 0)."""
    v = f32([[x, y, z] for z in (-.5, .5) for y in (-.5, .5) for x in (-.5, .5)])
    f = np.int64([[4, 5, 7], [4, 7, 6], [0, 2, 3], [0, 3, 1], [0, 1, 5], [0, 5, 4], [2, 6, 7], [2, 7, 3], [0, 4, 6], [0, 6, 2], [1, 3, 7], [1, 7, 5]])
    return v, f


def spike():
    """A needle: the apex (0, 0, 1) over the square base (+-1/8, +-1/8, 0), six faces wound outward; face 0 is the side that faces -x."""
    v = f32([[0, 0, 1], [-.125, -.125, 0], [.125, -.125, 0], [.125, .125, 0], [-.125, .125, 0]])
    f = np.int64([[0, 4, 1], [0, 1, 2], [0, 2, 3], [0, 3, 4], [1, 4, 3], [1, 3, 2]])
    return v, f


def three_on_an_edge():
    """Three faces around the edge (0, 1): non-manifold."""
    v = f32([[0, 0, 0], [0.5, 0, 0], [0.25, 0.5, 0], [0.25, -0.25, 0.5], [0.25, -0.25, -0.5]])
    f = np.int64([[0, 1, 2], [1, 0, 3], [0, 1, 4]])
    return v, f


def flipped_ico(k=7):
    v, f = R.icosphere(2, 0.6)
    f = f.copy()
    f[k] = f[k][::-1]
    return v, f


def table_meshes():
    """name -> (v, f): the meshes the table tests run on, on either side: closed, open, non-manifold, with a zero-area face (a repeated
    id, and three collinear vertices), and with spoilt faces."""
    if "table_meshes" not in _CACHE:
        out = {"ico": (MC.scene("ico")['v'], MC.scene("ico")['f']), "cube": cube(), "spike": spike(), "fan": MC.fan_mesh(),
               "nonmanifold": three_on_an_edge(), "flipped": flipped_ico()}
        v, f = cube()
        v = np.concatenate([v, f32([[0, 0, 0.5]])])                   # the middle of the top's diagonal: (4, 8, 7) has no area
        out["zero_area"] = (v, np.concatenate([f, np.int64([[4, 8, 7], [5, 5, 7]])]))
        out["spoilt"] = MC.broken_mesh()[:2]
        _CACHE["table_meshes"] = out
    return _CACHE["table_meshes"]


def signed_volume(v, f):
    t = v[f].astype(np.float64)
    return float(np.einsum('nk,nk->n', t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6)


# ---- the marched render of the solid icosphere, restated (the GPU tests' reference for the silhouette and the normals) ---------------------
def camera_np(H):
    """The rays of test_meshdist_gpu._camera: nerf-pytorch's get_rays for K = pinhole(H, H) and a camera at (0.1, -0.05, 2) that looks
    down -z without rotation."""
    fl = f32((H / 2) / np.tan(np.pi / 6))
    i, j = np.meshgrid(np.arange(H, dtype=f32), np.arange(H, dtype=f32), indexing='xy')
    rd = np.stack([(i - f32(H / 2)) / fl, -(j - f32(H / 2)) / fl, -np.ones_like(i)], -1).reshape(-1, 3).astype(f32)
    return np.broadcast_to(f32([0.1, -0.05, 2.0]), rd.shape).copy(), rd


def solid_render_np(H=48, ro=None, rd=None, samples=None):
    """MeshSolidField on the icosphere through the marched path, by the rules: occ_march_np on the shell of occupancy(1) at the step
    h / 2 (or the caller's lists: samples = (ray_id, dt, pts)), signed_grid_np with the query radius width, ramp_np, ramp_gradient_np, and
    the compositing and the normals of render_normals in float64.  -> dict(acc, normal, hit, face, face_normal, steep, flat, ...):
    steep = rays the mesh is hit by at |cos| > 0.5, flat = those of them whose hit has its three barycentrics above 0.2."""
    import march_rule as MR
    import meshhit_rule as MH
    sc, pn = MC.scene("ico"), tables("ico")
    G, lo, inv, h = sc['G'], sc['lo'], sc['inv'], sc['h']
    lo3, hi3 = np.broadcast_to(f32(lo), (3,)), np.broadcast_to(f32(1.0), (3,))
    occ = (sc['lists'][0] > 0).reshape(G, G, G)
    pad = np.pad(occ, 1)
    cells = np.zeros_like(occ)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                cells |= pad[dz:dz + G, dy:dy + G, dx:dx + G]
    cells = cells.astype(np.uint8)
    if ro is None:
        ro, rd = camera_np(H)
    if samples is None:
        _, _, ray_id, _, dt, pts, _ = MR.occ_march_np(ro, rd, 0.5, 3.5, cells, lo3, hi3, inv, h, float(h[0]) / 2)
    else:
        ray_id, dt, pts = samples
    n_rays = len(ro)
    width, peak = S.ramp_defaults(h)
    sg = S.signed_grid_np(pts, width, sc['lists'], sc['tri'], pn, G, lo, inv)
    dens = S.ramp_np(sg[1], width, peak)
    g = S.ramp_gradient_np(sg[1], sg[5], width, peak).astype(np.float64)
    dist = dt.astype(np.float64) * np.linalg.norm(rd.astype(np.float64), axis=1)[ray_id]
    alpha = 1.0 - np.exp(-dens.astype(np.float64) * dist)
    lg = np.log(1.0 - alpha + 1e-10)
    c = np.cumsum(lg)
    first = np.zeros(n_rays + 1, np.int64)
    np.add.at(first, np.asarray(ray_id, np.int64) + 1, 1)
    first = np.cumsum(first)[:-1]                                     # the lists are grouped by ray, ascending
    before = np.concatenate([[0.0], c])[first]
    w = alpha * np.exp(c - lg - before[ray_id])
    acc = np.bincount(ray_id, weights=w, minlength=n_rays)
    n_i = -g / np.maximum(np.linalg.norm(g, axis=1, keepdims=True), 1e-12)
    N = np.stack([np.bincount(ray_id, weights=w * n_i[:, k], minlength=n_rays) for k in range(3)], 1)
    normal = N / np.maximum(np.linalg.norm(N, axis=1, keepdims=True), 1e-12)
    hit, _, face, uv = MH.mesh_hit_grid_np(ro, rd, 0.5, 3.5, sc['lists'], sc['tri'], sc['f'], G, lo3, hi3, inv, h)
    fn = np.cross(sc['tri64'][:, 4:7], sc['tri64'][:, 8:11])
    fn /= np.linalg.norm(fn, axis=1, keepdims=True)
    face_normal = fn[np.maximum(face, 0)]
    cos = np.abs(np.einsum('nk,nk->n', rd.astype(np.float64) / np.linalg.norm(rd.astype(np.float64), axis=1, keepdims=True), face_normal))
    steep = (hit == 1) & (cos > 0.5)
    flat = steep & (uv[:, 0] > 0.2) & (uv[:, 1] > 0.2) & (1 - uv[:, 0] - uv[:, 1] > 0.2)
    pos = np.bincount(ray_id, weights=(sg[1] < 0), minlength=n_rays)
    return dict(acc=acc, normal=normal, hit=hit, face=face, face_normal=face_normal, steep=steep, flat=flat, cells=cells, negative=pos,
                density=dens, sdist=sg[1], n=len(pts))


# ---- 1. the sign against the winding number ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ico", "spot"])
def test_sign_against_the_winding_number(name):
    """Measured: 0 wrong of 2300 in both scenes, in binary32 and in float64, with no point left out by the cut (the smallest float64
    distance is 6.3e-5 on the icosphere and 2.2e-5 on spot); 22 % / 39 % of the points have their nearest point on an edge or a vertex."""
    sc = MC.scene(name)
    assert S.topology_np(sc['f'], len(sc['v'])) == dict(boundary_edges=0, nonmanifold_edges=0, inconsistent_edges=0)
    assert signed_volume(sc['v'], sc['f']) > 0                        # wound outward
    pts = MC.draw_points(name, 1.5)
    wn = S.winding_number_np(pts, sc['v'], sc['f'])
    assert np.all(np.abs(wn - np.round(wn)) < 1e-9) and set(np.round(wn).astype(int)) == {0, 1}
    inside = wn > 0.5
    got32 = S.signed_all_np(pts, f32(1e6), sc['tri'], tables(name))
    got64 = S.signed_all_np(pts, f32(1e6), sc['tri64'], tables(name, np.float64), np.float64)
    assert got32[0].all() and got64[0].all()
    judged = np.abs(got64[1]) > 1e-6
    off_face = float((got32[4] != 0).mean())
    print(f"{name}: left out by the cut {int((~judged).sum())} of {len(pts)}; wrong: binary32 {int(((got32[1] < 0) != inside)[judged].sum())}, "
          f"float64 {int(((got64[1] < 0) != inside)[judged].sum())}; inside {int(inside.sum())}; off a face interior {off_face:.3f}")
    assert (~judged).mean() <= 0.005
    assert np.array_equal((got32[1] < 0)[judged], inside[judged]) and np.array_equal((got64[1] < 0)[judged], inside[judged])
    assert 300 < inside.sum() < len(pts) - 300 and off_face > 0.15
    assert np.array_equal(np.abs(got32[1]), R.closest_all_np(pts, f32(1e6), sc['tri'])[1])           # the distance is the unsigned one


# ---- 2. why the tables exist ---------------------------------------------------------------------------------------------------------------
def test_pseudonormals_are_needed():
    """Points beside the tip of a needle, outside it: the nearest point is the apex, the winner (the lowest face id among equal d2) is
    face 0, whose own normal looks towards -x: for a point on the +x side it says 'inside'.  The apex's pseudonormal points up."""
    v, f = spike()
    assert S.topology_np(f, len(v)) == dict(boundary_edges=0, nonmanifold_edges=0, inconsistent_edges=0) and signed_volume(v, f) > 0
    tri = R.tri_records_np(v, f)
    pn = S.pseudonormals_np(f, len(v), tri)
    pts = f32([[0.25, 0, 1.25], [0.25, 0.125, 1.125], [0.5, -0.25, 1.5]])
    assert np.all(S.winding_number_np(pts, v, f) < 1e-9)                                                # outside
    unsigned = R.closest_all_np(pts, f32(4), tri)
    right = S.sign_step_np(pts, f32(4), unsigned, tri, pn)
    wrong = S.sign_step_np(pts, f32(4), unsigned, tri, pn, face_normal_only=True)
    assert right[2].tolist() == [0, 0, 0] and right[4].tolist() == [1, 1, 1]                            # face 0, at its vertex v0: the apex
    assert np.all(wrong[1] < 0) and np.all(right[1] > 0) and np.array_equal(np.abs(wrong[1]), right[1])
    assert pn[0, 0, 0] < -0.9 and pn[0, 1, 2] > 0 and abs(pn[0, 1, 0]) < 1e-6 and abs(pn[0, 1, 1]) < 1e-6
    # an acute ridge: beside the edge apex - (1/8, -1/8, 0) shared by faces 1 and 2, nearest point on that edge
    p = f32([[0.5, -0.4375, 0.5]])
    u2 = R.closest_all_np(p, f32(4), tri)
    a, b = S.sign_step_np(p, f32(4), u2, tri, pn), S.sign_step_np(p, f32(4), u2, tri, pn, face_normal_only=True)
    assert a[4][0] in (4, 5, 6) and a[1][0] > 0 and S.winding_number_np(p, v, f)[0] < 1e-9
    print(f"ridge: face {a[2][0]}, feature {a[4][0]}, sdist by the pseudonormal {a[1][0]:+.4f}, by the face normal {b[1][0]:+.4f}")


# ---- 3. the cube ---------------------------------------------------------------------------------------------------------------------------
T3, T6, T8 = 1 / 3, 0.6, 0.8
CUBE_POINTS = [                          # point, face, feature, sdist, grad: dyadic offsets whose lengths are dyadic too (1-2-2, 3-4-5)
    ((0.25, -0.25, 0.75), 0, 0, 0.25, (0, 0, 1)),                                 # above the interior of face 0
    ((0.25, -0.25, 0.375), 0, 0, -0.125, (0, 0, 1)),                              # below it, inside
    ((0.25, -0.25, 0.5), 0, 0, 0.0, (0, 0, 1)),                                   # on it: outside, the face normal
    ((-0.5625, -0.625, 0.625), 0, 1, 0.1875, (-T3, -2 * T3, 2 * T3)),             # beyond v0 = vertex 4 by (-1, -2, 2) / 16
    ((0.5625, -0.625, 0.625), 0, 2, 0.1875, (T3, -2 * T3, 2 * T3)),               # beyond v0 + e1 = vertex 5
    ((0.625, 0.5625, 0.625), 0, 3, 0.1875, (2 * T3, T3, 2 * T3)),                 # beyond v0 + e2 = vertex 7
    ((0.125, -0.6875, 0.75), 0, 4, 0.3125, (0, -T6, T8)),                         # beside the cube edge along e1, by (-3, 4) / 16
    ((0.125, 0.125, 0.75), 0, 5, 0.25, (0, 0, 1)),                                # above the top's diagonal, the edge along e2 of face 0
    ((0.125, 0.125, 0.25), 0, 5, -0.25, (0, 0, 1)),                               # below the diagonal, inside
    ((0.6875, 0.125, 0.75), 0, 6, 0.3125, (T6, 0, T8)),                           # beside the cube edge opposite v0
    ((-0.125, 0.25, 0.625), 1, 0, 0.125, (0, 0, 1)),                              # above the interior of face 1
    ((-0.6875, 0.125, 0.75), 1, 5, 0.3125, (-T6, 0, T8)),                         # beside the edge along e2 of face 1
    ((0.125, 0.6875, 0.75), 1, 6, 0.3125, (0, T6, T8)),                           # beside the edge opposite v0 of face 1
    ((-0.5625, 0.625, 0.625), 1, 3, 0.1875, (-T3, 2 * T3, 2 * T3)),               # beyond v0 + e2 of face 1 = vertex 6
    ((0.0, 0.0, 0.0), 0, 5, -0.5, (0, 0, 1)),                                     # the centre: every face at 1/2, face 0 by its diagonal
]


def test_cube_by_hand():
    v, f = cube()
    assert S.topology_np(f, len(v)) == dict(boundary_edges=0, nonmanifold_edges=0, inconsistent_edges=0) and signed_volume(v, f) == 1.0
    tri = R.tri_records_np(v, f)
    pn = S.pseudonormals_np(f, len(v), tri)
    assert np.array_equal(pn[:, 0], f32([[0, 0, 1]] * 2 + [[0, 0, -1]] * 2 + [[0, -1, 0]] * 2 + [[0, 1, 0]] * 2 + [[-1, 0, 0]] * 2 + [[1, 0, 0]] * 2))
    assert np.array_equal(pn[0, 4:], f32([[0, -1, 1], [0, 0, 2], [1, 0, 1]]))                           # a cube edge, the diagonal, a cube edge
    corner = pn[0, 1] / np.linalg.norm(pn[0, 1])
    assert np.abs(corner - f32([-1, -1, 1]) / np.sqrt(3)).max() < 1e-6 and abs(np.linalg.norm(pn[0, 1]) - np.sqrt(3) * np.pi / 2) < 1e-5
    pts = f32([p for p, *_ in CUBE_POINTS])
    G = 4
    lo, inv, h = R.grid_consts(G, -1.0, 1.0)
    lists = R.mesh_cells_np(v, f, G, lo, inv)
    want_grad = np.stack([f32(g) for *_, g in CUBE_POINTS])
    for form in (S.signed_all_np(pts, f32(1.0), tri, pn), S.signed_grid_np(pts, f32(1.0), lists, tri, pn, G, lo, inv)):
        assert form[0].all() and all(x.dtype == t for x, t in zip(form, (np.uint8, f32, np.int32, f32, np.uint8, f32)))
        assert form[2].tolist() == [face for _, face, *_ in CUBE_POINTS] and form[4].tolist() == [feat for _, _, feat, *_ in CUBE_POINTS]
        assert np.array_equal(form[1], f32([d for _, _, _, d, _ in CUBE_POINTS])) and not np.signbit(form[1][2])
        assert np.array_equal(form[5], want_grad), form[5] - want_grad
    assert set(form[4].tolist()) == set(range(7))
    wn = S.winding_number_np(pts, v, f)
    off = np.abs(form[1]) > 0
    assert np.array_equal((form[1] < 0)[off], (wn > 0.5)[off])
    # on a vertex: d2 = 0, outside, and the gradient is the corner's pseudonormal, normalised
    at = S.signed_all_np(v[[4]], f32(1.0), tri, pn)
    assert at[1][0] == 0 and at[2][0] == 0 and at[4][0] == 1 and np.abs(at[5][0] - f32([-1, -1, 1]) / np.sqrt(3)).max() < 1e-6
    # a miss
    far = S.signed_grid_np(f32([[0.9, 0.9, 0.9], [np.nan, 0, 0]]), f32(0.25), lists, tri, pn, G, lo, inv)
    assert not far[0].any() and np.array_equal(far[1], f32([0.25, 0.25])) and np.all(far[2] == -1) and not far[3].any() and not far[4].any() \
        and not far[5].any()


# ---- 4. the tables -------------------------------------------------------------------------------------------------------------------------
TABLE_MEASURED = {"ico": 7.3e-7, "spot": 1.2e-6}        # max |pn32 - pn64| over the seven rows; rows 0 and 4-6 alone: 1.6e-7, 2.7e-7
TABLE_GATE = {k: 4 * x for k, x in TABLE_MEASURED.items()}                                             # 2.9e-6, 4.8e-6


@pytest.mark.parametrize("name", ["ico", "spot"])
def test_tables_against_float64(name):
    """Vertex rows have a length of up to 2 pi and are sums of about six terms, each an arctan2 times a unit vector: last-bit effects.
    The gate is 4 x the measured figure; the GPU test holds the device's rows 1-3 to the same gate (the factor covers its atan2f)."""
    pn, pn64 = tables(name), tables(name, np.float64)
    assert pn.dtype == f32 and pn64.dtype == np.float64 and pn.shape == (len(MC.scene(name)['f']), 7, 3)
    worst = float(np.abs(pn - pn64).max())
    print(f"{name}: tables, binary32 against float64: max |diff| = {worst:.3e} (rows 0, 4-6: {float(np.abs(pn - pn64)[:, [0, 4, 5, 6]].max()):.3e}), "
          f"gate {TABLE_GATE[name]:.3e}")
    assert worst <= TABLE_GATE[name]
    assert np.abs(np.linalg.norm(pn64[:, 0], axis=1) - 1).max() < 1e-12
    # on a closed surface every pseudonormal looks out of the same side as its face
    assert np.all(np.einsum('frk,fk->fr', pn64, pn64[:, 0]) > 0)


def test_the_order_of_the_sums_is_the_rule():
    """Visiting the faces in descending id changes last bits of the vertex rows (sums of six rounded terms), so the ascending order is
    part of the definition; the edge rows of a closed manifold mesh are sums of two terms, which commute."""
    sc = MC.scene("ico")
    F = len(sc['f'])
    pn = tables("ico")
    rev = S.pseudonormals_np(sc['f'], len(sc['v']), sc['tri'], order=np.arange(F)[::-1])
    assert np.array_equal(S.pseudonormals_np(sc['f'], len(sc['v']), sc['tri'], order=np.arange(F)), pn)
    assert np.array_equal(rev[:, 0], pn[:, 0]) and np.array_equal(rev[:, 4:], pn[:, 4:])
    differ = (rev[:, 1:4] != pn[:, 1:4]).any((1, 2))
    assert differ.sum() > F // 10 and np.abs(rev - pn).max() < 2e-6
    # three faces on one edge: the edge row is a sum of three terms, spelt out in ascending id
    v, f = three_on_an_edge()
    t = S.pseudonormals_np(f, len(v), R.tri_records_np(v, f))
    u = t[:, 0]
    assert np.array_equal(t[0, 4], (u[0] + u[1]) + u[2]) and np.array_equal(t[1, 4], t[0, 4]) and np.array_equal(t[2, 4], t[0, 4])
    assert np.array_equal(t[0, 5], u[0]) and np.array_equal(t[0, 6], u[0])                             # boundary edges: the one face's normal


def test_faces_that_do_not_count():
    meshes = table_meshes()
    v, f = meshes["zero_area"]
    pn = S.pseudonormals_np(f, len(v), R.tri_records_np(v, f))
    ref = S.pseudonormals_np(cube()[1], 8, R.tri_records_np(*cube()))
    assert np.array_equal(pn[:12], ref)                               # the two faces without area add nothing to any sum
    assert not pn[12:, 0].any() and np.array_equal(pn[12, 1], ref[0, 1]) and np.array_equal(pn[12, 3], ref[0, 3]) and not pn[12, 2].any()
    assert np.array_equal(pn[12, 5], ref[0, 5]) and not pn[13, 4].any()                                # (4, 7): the diagonal; (5, 5): nothing
    v, f = meshes["spoilt"]
    pn = S.pseudonormals_np(f, len(v), R.tri_records_np(v, f))
    bad = list(MC.broken_mesh()[2])
    assert np.isnan(pn[bad]).all() and np.isfinite(np.delete(pn, bad, 0)).all()
    v, f = meshes["fan"]
    pn = S.pseudonormals_np(f, len(v), R.tri_records_np(v, f))
    assert np.array_equal(pn[0, 4:], np.repeat(pn[0, :1], 3, 0))      # face 0 shares no edge: three boundary edges


# ---- 5. topology ---------------------------------------------------------------------------------------------------------------------------
def test_topology_by_hand():
    m = table_meshes()
    want = {"ico": (0, 0, 0), "cube": (0, 0, 0), "spike": (0, 0, 0), "fan": (7, 0, 0), "nonmanifold": (6, 1, 0), "flipped": (0, 0, 3)}
    for name, (b, n, i) in want.items():
        v, f = m[name]
        assert S.topology_np(f, len(v)) == dict(boundary_edges=b, nonmanifold_edges=n, inconsistent_edges=i), name
    v, f = m["spoilt"]                                                # the two faces with an id outside [0, V) are left out
    assert S.topology_np(f, len(v)) == S.topology_np(np.delete(f, [40, 41], 0), len(v))


# ---- 6. the two forms ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mult", MC.RADII)
@pytest.mark.parametrize("name", ["ico", "tri4"])
def test_grid_form_finds_what_all_triangles_find(name, mult):
    """test_meshdist_cpu's statement with its mask, on all six outputs.  The random triangles are no closed surface: their sign means
    nothing, and is the same number in both forms all the same."""
    c, s = MC.case(name, mult), signed_case(name, mult)
    n = len(c['pts'])
    judged = ~c['near_r'] & (c['in_box'] | (c['d_all'] > f32(1.01) * c['r']))
    for what, a, b in zip(SIGNED_NAMES, s['grid'], s['all']):
        assert a.dtype == b.dtype and np.array_equal(a[judged], b[judged], equal_nan=True), (what, np.flatnonzero(judged & (a != b).reshape(n, -1).any(1))[:10])
    for k in (0, 2, 3):
        assert np.array_equal(s['grid'][k], c['grid'][k])
    assert np.array_equal(np.abs(s['grid'][1]), c['grid'][1])
    found = s['grid'][0] == 1
    kinds = set(s['grid'][4][found].tolist())
    print(f"{name} r = {mult} min(h): features {sorted(kinds)}, inside {int((s['grid'][1] < 0).sum())}, outside {int((s['grid'][1][found] > 0).sum())}")
    assert len(kinds) >= 4 and (s['grid'][1] < 0).sum() > 50 and (s['grid'][1][found] > 0).sum() > 50      # the condition on the seeds
    norm = np.linalg.norm(s['grid'][5].astype(np.float64), axis=1)
    assert np.abs(norm[found & (s['grid'][1] != 0)] - 1).max() < 1e-6 and not s['grid'][5][~found].any() and not s['grid'][4][~found].any()


# ---- 7. the ramp ---------------------------------------------------------------------------------------------------------------------------
def test_ramp():
    for G in (16, 64, 12, 100):
        _, _, h = R.grid_consts(G, -1.0, 1.0)
        width, peak = S.ramp_defaults(h)
        assert width == h.max() and width.dtype == f32 and peak.dtype == f32
        if G in (16, 64):
            assert peak * width == f32(32)
        assert abs(float(peak) * float(width) - 32) <= 32 * 2.0 ** -23
        out = np.concatenate([width * f32([0, 2.0 ** -24, 0.5, 1, 3]), f32([np.inf])]).astype(f32)
        t = S.ramp_np(out, width, peak)
        assert t.dtype == f32 and not t.any()                         # exactly 0 on the surface, outside and on a miss (sdist = +width)
        t = S.ramp_np(-width * f32([2.0 ** -24, 0.25, 0.5, 1 - 2.0 ** -24, 1, 1.5, 3]), width, peak)
        assert np.all(t > 0) and np.all(np.diff(t[:5]) > 0) and np.all(t[4:] == peak)
        if G in (16, 64):
            assert np.array_equal(t[1:3], peak * f32([0.25, 0.5]))
        sd = -width * f32([0, 0.5, 1, 1.5, -0.5])
        g = S.ramp_gradient_np(sd, f32([[0, 0, 1]] * 5), width, peak)
        assert g.dtype == f32 and np.array_equal(g[:, 2], f32([0, -(peak / width), 0, 0, 0])) and not g[:, :2].any()


# ---- 8. the marched render by the rules ----------------------------------------------------------------------------------------------------
NORMAL_MEASURED = 2.3e-2                 # max |rendered normal - face normal| of solid_render_np(48) on its 54 flat rays: 2.217e-2


def test_solid_render_by_the_rules():
    """The restatement the GPU tests composite against, on its own camera: the silhouette is the mesh's (acc exactly 0 on every ray the
    mesh is not hit by, 1 on the steep hits), and the figure behind test_meshsdf_gpu's NORMAL_GATE.  It is no rounding figure: near
    |cos| = 0.5 a ray moves sideways by 1.7 x its depth, and the deeper samples of the wall have their nearest point on a neighbouring
    face of the icosphere, some ten degrees off."""
    out = solid_render_np(48)
    miss, steep, flat = out['hit'] == 0, out['steep'], out['flat']
    assert miss.sum() > 1500 and steep.sum() > 300 and flat.sum() >= 40
    assert not out['acc'][miss].any() and out['acc'][steep].min() >= 1 - 2.0 ** -20
    worst = float(np.abs(out['normal'][flat] - out['face_normal'][flat]).max())
    print(f"normals by the rules on {int(flat.sum())} rays: max |normal - face normal| = {worst:.3e}; mean((acc - hit)^2) = "
          f"{float(np.mean((out['acc'] - out['hit']) ** 2)):.3e}")
    assert 0.5 * NORMAL_MEASURED <= worst <= NORMAL_MEASURED
    assert np.all(np.einsum('nk,nk->n', out['normal'][steep], out['face_normal'][steep]) > 0.9)
