"""CPU: the point / mesh query's rule (tests/meshdist_rule.py) against itself and against float64, and the scenes and
points the GPU tests share.

1. the grid form == the all-triangles binary32 form, array_equal on found, face, dist and uv, where the all-triangles best distance is
   <= 0.99 r or > 1.01 r (the share in between is asserted to stay within 5 %) and, for a found point, where its nearest point lies inside
   the box: the random triangles reach out of the box, and a nearest point out there lies in no cell (meshdist_rule's docstring).  On the
   points left out for that reason the grid form, a minimum over fewer triangles, must give no smaller distance, and the same numbers
   wherever it names the same face;
2. the seven regions of a triangle by hand, a shared vertex, non-finite points, points beyond the box, faces that must never come back;
3. dist against the float64 all-triangles form;
4. the tent."""
import numpy as np
import pytest

import meshdist_rule as R

f32 = np.float32
RADII = (0.5, 1.5, 3.0)                  # in units of min(h)
SCENES = ("ico", "tri1", "tri4", "tri16")
_CACHE = {}


def scene(name):
    """-> dict(v, f, G, lo, inv, h, lists, tri, tri64), built once: icosphere(2, 0.6) at G = 16, or 300 random triangles of the four KINDS
    (110 small, 100 medium, 20 giant, 70 on a cell face) at the G the name carries; 'spot' at G = 32.  The box is [-1, 1]^3."""
    if name not in _CACHE:
        if name == "ico":
            (v, f), G = R.icosphere(2, 0.6), 16
        elif name == "spot":
            (v, f), G = R.spot_mesh(), 32
        else:
            G = int(name[3:])
            rng = np.random.default_rng(200 + G)
            tri = np.concatenate([R.random_triangles(rng, G, n, kind) for n, kind in zip((110, 100, 20, 70), R.KINDS)])
            v, f = R.triangles_to_mesh(tri, G)
        lo, inv, h = R.grid_consts(G, -1.0, 1.0)
        _CACHE[name] = dict(v=v, f=f, G=G, lo=lo, inv=inv, h=h, lists=R.mesh_cells_np(v, f, G, lo, inv), tri=R.tri_records_np(v, f),
                            tri64=R.tri_records_np(v, f, np.float64))
    return _CACHE[name]


def radius(sc, mult):
    return f32(mult) * np.min(sc['h'])


def draw_points(name, mult, n=2000, far=300):
    """n points within 2r of the surface (a uniform point of the mesh inside the box, moved by up to 2r in a uniform direction; three in
    four are then clamped to the box, where most nearest points lie inside it too), then `far` points uniform in the box grown by 3r."""
    sc = scene(name)
    r = float(radius(sc, mult))
    rng = np.random.default_rng(1000 * sc['G'] + int(10 * mult) + len(name))
    tri = sc['v'][sc['f']].astype(np.float64)
    k = rng.integers(0, len(tri), 40 * n)
    s = np.einsum('nk,nkc->nc', rng.dirichlet([1, 1, 1], 40 * n), tri[k])
    s = s[np.all(np.abs(s) <= 1, 1)][:n]
    assert len(s) == n
    d = rng.normal(size=(n, 3))
    p = s + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0, 2 * r, (n, 1))
    p[:3 * n // 4] = np.clip(p[:3 * n // 4], -1, 1)
    return np.concatenate([p, rng.uniform(-1 - 3 * r, 1 + 3 * r, (far, 3))]).astype(f32)


def case(name, mult):
    """-> dict(pts, r, grid, all, d_all, near_r, in_box) of one (scene, radius), computed once: the two forms on draw_points, the
    all-triangles best distance whatever r, which points lie within 1 % of r, and whose nearest point lies inside the box."""
    key = (name, mult)
    if key not in _CACHE:
        sc = scene(name)
        r, pts = radius(sc, mult), draw_points(name, mult)
        grid = R.closest_grid_np(pts, r, sc['lists'], sc['tri'], sc['G'], sc['lo'], sc['inv'])
        every = R.closest_all_np(pts, r, sc['tri'], return_d2=True)
        d_all = np.sqrt(every[4])
        free = R.closest_all_np(pts, f32(1e6), sc['tri'])                 # the nearest triangle whatever the radius
        _CACHE[key] = dict(pts=pts, r=r, grid=grid, all=every[:4], d_all=d_all, near_r=(d_all > f32(0.99) * r) & (d_all <= f32(1.01) * r),
                           in_box=R.closest_in_box(pts, free[2], free[3], sc['tri64'], -1.0, 1.0))
    return _CACHE[key]


NAMES = ("found", "dist", "face", "uv")


# ---- 1. the two forms -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mult", RADII)
@pytest.mark.parametrize("name", SCENES)
def test_grid_form_finds_what_all_triangles_find(name, mult):
    c = case(name, mult)
    grid, every, r = c['grid'], c['all'], c['r']
    n = len(c['pts'])
    near = float(c['near_r'].mean())
    judged = ~c['near_r'] & (c['in_box'] | (c['d_all'] > f32(1.01) * r))
    print(f"{name} r = {mult} min(h): within 1 % of r {near:.4f}, nearest point outside the box {float((~c['near_r'] & ~judged).mean()):.4f}, "
          f"found {int(every[0].sum())} of {n}")
    assert near <= 0.05                                               # the condition on the seeds
    assert judged.sum() >= n // 3 and every[0][judged].sum() >= n // 4 and (every[0][judged] == 0).sum() >= (50 if name == "ico" else 5)
    for what, a, b in zip(NAMES, grid, every):
        assert a.dtype == b.dtype and np.array_equal(a[judged], b[judged]), (what, np.flatnonzero(judged & (a != b).reshape(n, -1).any(1))[:10])
    # everywhere: the grid form is a minimum over fewer triangles with the same numbers per triangle
    assert not np.any(grid[0] & ~every[0]) and np.all(grid[1] >= every[1])
    same = (grid[2] == every[2]) & (grid[0] == 1)
    assert np.array_equal(grid[1][same], every[1][same]) and np.array_equal(grid[3][same], every[3][same])
    if name == "ico":                                                 # the whole mesh is inside the box: only the 1 % band is left out
        assert np.array_equal(judged, ~c['near_r'])


def test_order_of_cells_and_duplicates_do_not_matter():
    """A triangle listed in several cells gives the same numbers each time: reversing every cell's list and the face order of the ties
    leaves the answer (the minimum over (d2, face) has one value)."""
    sc, c = scene("tri4"), case("tri4", 1.5)
    count, cell_off, cell_tri = sc['lists']
    rev = cell_tri.copy()
    for a, b in zip(cell_off[:-1], cell_off[1:]):
        rev[a:b] = cell_tri[a:b][::-1]
    got = R.closest_grid_np(c['pts'], c['r'], (count, cell_off, rev), sc['tri'], sc['G'], sc['lo'], sc['inv'])
    assert all(np.array_equal(a, b) for a, b in zip(got, c['grid']))


# ---- 2. by hand ---------------------------------------------------------------------------------------------------------------------------------
V0, E1, E2 = f32([0.25, 0.25, 0.5]), f32([0.5, 0, 0]), f32([0, 0.5, 0])
REGIONS = [                              # offset from v0, expected (u, v), expected d2: all dyadic, every step exact
    ((-0.125, -0.125, 0.125), (0, 0), 3 * 0.125 ** 2),                # the vertex v0
    ((0.75, -0.125, 0.125), (1, 0), 0.25 ** 2 + 2 * 0.125 ** 2),      # the vertex v0 + e1
    ((0.25, -0.25, 0.125), (0.5, 0), 0.25 ** 2 + 0.125 ** 2),         # the middle of the edge along e1
    ((-0.125, 0.75, 0.125), (0, 1), 0.25 ** 2 + 2 * 0.125 ** 2),      # the vertex v0 + e2
    ((-0.25, 0.25, 0.125), (0, 0.5), 0.25 ** 2 + 0.125 ** 2),         # the middle of the edge along e2
    ((0.5, 0.5, 0.125), (0.5, 0.5), 2 * 0.25 ** 2 + 0.125 ** 2),      # the middle of the edge opposite v0
    ((0.125, 0.125, 0.25), (0.25, 0.25), 0.25 ** 2),                  # the interior: the foot of the perpendicular
]


def test_seven_regions_by_hand():
    v = np.stack([V0, V0 + E1, V0 + E2])
    f = np.int64([[0, 1, 2]])
    tri = R.tri_records_np(v, f)
    pts = np.stack([V0 + f32(off) for off, _, _ in REGIONS])
    ok, d2, u, w = R.closest_on_tri_np(pts, tri[0])
    assert ok.all()
    assert np.array_equal(np.stack([u, w], -1), f32([uv for _, uv, _ in REGIONS])) and np.array_equal(d2, f32([d for _, _, d in REGIONS]))
    G = 4
    lo, inv, h = R.grid_consts(G, -1.0, 1.0)
    lists = R.mesh_cells_np(v, f, G, lo, inv)
    for form in (R.closest_all_np(pts, f32(1.0), tri), R.closest_grid_np(pts, f32(1.0), lists, tri, G, lo, inv)):
        assert form[0].all() and not form[2].any()
        assert np.array_equal(form[3], f32([uv for _, uv, _ in REGIONS])) and np.array_equal(form[1], np.sqrt(f32([d for _, _, d in REGIONS])))
    # the same seven in float64
    ok, d2, u, w = R.closest_on_tri_np(pts, R.tri_records_np(v, f, np.float64)[0], np.float64)
    assert np.array_equal(np.stack([u, w], -1), np.float64([uv for _, uv, _ in REGIONS])) and d2.dtype == np.float64


def fan_mesh():
    """Five faces; faces 1 .. 4 share the vertex 0 at (0.25, 0.25, 0.25), as their first, second or third vertex; dyadic coordinates, so
    every edge vector and every nearest point is exact."""
    v = f32([[0.25, 0.25, 0.25], [0.75, 0.25, 0.25], [0.25, 0.75, 0.25], [-0.25, 0.25, 0.5], [0.25, -0.25, 0.5], [0.75, 0.75, -0.5], [0.5, 0.75, -0.5]])
    f = np.int64([[5, 6, 1], [1, 2, 0], [0, 2, 3], [4, 0, 3], [1, 0, 4]])
    return v, f


def test_shared_vertex_gives_zero_and_the_lowest_face():
    v, f = fan_mesh()
    G = 4
    lo, inv, h = R.grid_consts(G, -1.0, 1.0)
    tri, lists = R.tri_records_np(v, f), R.mesh_cells_np(v, f, G, lo, inv)
    pts = v[[0, 1]]                                                   # vertex 0: faces 1 .. 4; vertex 1: faces 0, 1, 4
    for form in (R.closest_all_np(pts, f32(0.25), tri), R.closest_grid_np(pts, f32(0.25), lists, tri, G, lo, inv)):
        assert form[0].tolist() == [1, 1] and form[1].tolist() == [0, 0] and form[2].tolist() == [1, 0]
        assert form[3].tolist() == [[0, 1], [0, 1]]                   # the third vertex of face 1, the third vertex of face 0


def test_non_finite_points_and_points_beyond_the_box_miss():
    sc = scene("ico")
    r = radius(sc, 1.5)
    bad = f32([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan], [3e38, 0, 0]])
    out = f32([[1 + 1.01 * r, 0, 0], [0, -1 - 1.01 * r, 0.3], [0.6, 0, 5], [-7, -7, -7]])
    edge = f32([[1 + 0.5 * r, 0, 0]])                                  # beyond the box but within r of it: a block, and nothing in it
    pts = np.concatenate([bad, out, edge])
    live = R.block_np(pts, r, sc['G'], sc['lo'], sc['inv'])[0]
    assert live.tolist() == [False] * 9 + [True]
    for form in (R.closest_grid_np(pts, r, sc['lists'], sc['tri'], sc['G'], sc['lo'], sc['inv']), R.closest_all_np(pts, r, sc['tri'])):
        assert not form[0].any() and np.array_equal(form[1], np.full(10, r, f32)) and np.all(form[2] == -1) and not form[3].any()
        assert form[0].dtype == np.uint8 and form[1].dtype == f32 and form[2].dtype == np.int32 and form[3].dtype == f32


def broken_mesh(name="tri4"):
    """The scene's mesh with four faces spoilt: a NaN vertex, an infinite coordinate, an index of -1, an index of V -> (v, f, bad ids)."""
    sc = scene(name)
    v, f = sc['v'].copy(), sc['f'].copy()
    v[f[5, 1]] = np.nan; v[f[17, 0], 2] = np.inf; f[40, 2] = -1; f[41, 0] = len(v)
    return v, f, (5, 17, 40, 41)


def test_spoilt_faces_never_come_back():
    sc = scene("tri4")
    v, f, bad = broken_mesh()
    tri, lists = R.tri_records_np(v, f), R.mesh_cells_np(v, f, sc['G'], sc['lo'], sc['inv'])
    assert np.isnan(tri[list(bad)]).all() and not set(lists[2].tolist()) & set(bad)
    r = radius(sc, 1.5)
    centre = sc['v'][sc['f'][list(bad)]].mean(1)                          # where the four faces were
    pts = np.concatenate([centre, np.clip(centre, -1, 1), draw_points("tri4", 1.5)[:500]]).astype(f32)
    before = R.closest_all_np(pts, r, sc['tri'])
    assert set(before[2][:8].tolist()) & set(bad)                         # unspoilt, they are the answer there
    stale = (sc['lists'][0], sc['lists'][1], sc['lists'][2])              # lists that still name the spoilt faces: the records stop them
    for form in (R.closest_all_np(pts, r, tri), R.closest_grid_np(pts, r, lists, tri, sc['G'], sc['lo'], sc['inv']),
                 R.closest_grid_np(pts, r, stale, tri, sc['G'], sc['lo'], sc['inv'])):
        assert not set(form[2].tolist()) & set(bad) and form[0].sum() > 100
    # a list entry outside [0, F) is skipped
    wild = lists[2].copy()
    wild[::7], wild[3::11] = -1, len(f)
    got = R.closest_grid_np(pts, r, (lists[0], lists[1], wild), tri, sc['G'], sc['lo'], sc['inv'])
    assert got[2].max() < len(f) and np.all((got[2] >= 0) == (got[0] == 1))


# ---- 3. against float64 -------------------------------------------------------------------------------------------------------------------------
DIST_MEASURED = {"ico": 4.4e-8, "tri1": 3.4e-4, "tri4": 2.5e-5, "tri16": 2.5e-7}       # max |dist32 - dist64| per scene, over the three radii
DIST_GATE = {k: 4 * x for k, x in DIST_MEASURED.items()}                                # 1.8e-7, 1.4e-3, 1.0e-4, 1.0e-6


@pytest.mark.parametrize("name", SCENES)
def test_dist_against_float64(name):
    """dist of the binary32 all-triangles form against the float64 one, per scene over the three radii.  Measured: the largest absolute
    difference is 4.4e-8 on the icosphere, 2.5e-7 / 2.5e-5 / 3.4e-4 on the random triangles at G = 16 / 4 / 1; the gate is 4 x that:
    1.8e-7, 1.0e-6, 1.0e-4, 1.4e-3.  On the icosphere (edges of 0.2) these are last-bit effects of a handful of float32 operations.  The
    random scenes are worse for a reason that has nothing to do with the last bit of dist: their worst points lie ON a triangle several
    box widths across (a clamped point on a cell face, an on_face or giant triangle in that plane), where the true distance is 0 and
    dist is the square root of what the cancellations in va, vb, vc leave of products of order extent^4; the 99th percentile stays below
    1e-6 in every scene.  The factor 4 covers other seeds.  found is compared outside the 1 % band around r, the face where float64
    does not see two faces within 1e-6 of each other."""
    worst = 0.0
    sc = scene(name)
    for mult in RADII:
        c = case(name, mult)
        ref = R.closest_all_np(c['pts'], c['r'], sc['tri64'], np.float64)
        got = c['all']
        clear = ~c['near_r']
        assert np.array_equal(got[0][clear], ref[0][clear])
        both = (got[0] == 1) & (ref[0] == 1)
        diff = np.abs(got[1][both].astype(np.float64) - ref[1][both])
        worst = max(worst, float(diff.max()))
        assert np.quantile(diff, 0.99) < 1e-6
        # the runner-up of float64: the best over the other faces
        ok, d2, _, _ = R.closest_on_tri_np(c['pts'][both][:, None, :], sc['tri64'][None], np.float64)
        d = np.sqrt(np.where(ok, d2, np.inf))
        d[np.arange(len(d)), ref[2][both]] = np.inf
        alone = d.min(1) - ref[1][both] > 1e-6
        assert alone.sum() > both.sum() // 4 and np.array_equal(got[2][both][alone], ref[2][both][alone])
        assert np.abs(got[3][both][alone] - ref[3][both][alone]).max() < 1e-3
    print(f"{name}: dist, binary32 against float64: max |diff| = {worst:.3e}, gate {DIST_GATE[name]:.3e}")
    assert worst <= DIST_GATE[name]


# ---- 4. the tent --------------------------------------------------------------------------------------------------------------------------------
def test_tent():
    for G in (16, 64, 12, 100):
        _, _, h = R.grid_consts(G, -1.0, 1.0)
        width, peak = R.tent_defaults(h)
        assert width == h.max() and width.dtype == f32 and peak.dtype == f32
        if G in (16, 64):
            assert peak * width == f32(16)                            # a power-of-two cell: exactly
        assert abs(float(peak) * float(width) - 16) <= 16 * 2.0 ** -23
        assert np.exp(-float(peak) * float(width)) < 2.0 ** -23       # the wall is opaque in float32
        dist = np.concatenate([width * f32([1, 1 + 2.0 ** -23, 1.5, 3, np.inf]), width * f32([0, 0.25, 0.5, 1 - 2.0 ** -24])]).astype(f32)
        t = R.tent_np(dist, width, peak)
        assert t.dtype == f32 and np.array_equal(t[:5], np.zeros(5, f32)) and not np.signbit(t[:5]).any()
        assert t[5] == peak and np.all(t[5:] > 0) and np.all(np.diff(t[5:]) < 0)
        if G in (16, 64):
            assert np.array_equal(t[5:8], peak * f32([1, 0.75, 0.5]))
    lo, inv, h = R.grid_consts(8, (-1.0, -1.0, -1.0), (1.0, 2.0, 1.0))
    assert R.tent_defaults(h)[0] == h[1] == f32(0.375)                # the largest edge
