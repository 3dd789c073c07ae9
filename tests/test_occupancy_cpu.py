"""CPU: the occupancy grid of the ray path (render_rays(occupancy=), volume_render.OccupancyGrid) — the definition of the selection,
of the grid's refresh and of its cell points, and the host control flow.

`occ_mark_np`, `occ_cell_points_np` and `occ_update_np` below ARE the rules csrc/occupancy.hip (ctx_occ_mark, ctx_occ_cell_points,
ctx_occ_update) is held to; tests/test_occupancy_gpu.py imports them from here and compares with array_equal.  All float arithmetic is
binary32 in the order written (numpy array operations round every product and sum on their own: no contraction).

1. the restatement against brute-force properties: an all-ones grid marks exactly the samples inside the box, an all-zeros grid none,
   a NaN point and a point on `hi` are outside, a point on `lo` is inside, the cell read is the one that holds the point;
2. the update rule on hand-made raw: decay, equality with the threshold is not occupied, NaN is occupied; the cell points;
3. host: construction refusals, host tensors, fit_views' update schedule and train_step's empty batch with the device seams stubbed."""
import types
import numpy as np
import pytest
import torch

f32 = np.float32


# ---- the numpy restatement ------------------------------------------------------------------------------------------------------
def grid_consts(G, lo, hi):
    """-> (lo [3], inv [3], h [3]) float32: inv = G / (hi - lo) and h = (hi - lo) / G, each computed once per axis in binary32."""
    lo = np.broadcast_to(np.asarray(lo, f32), (3,)).copy()
    hi = np.broadcast_to(np.asarray(hi, f32), (3,)).copy()
    ext = hi - lo
    return lo, f32(G) / ext, ext / f32(G)


def occ_points_np(ro, rd, z):
    """p = o + d*z [R,S,3]: one product, one sum per axis (what `rays_o[:, None] + rays_d[:, None] * z[..., None]` gives in torch)."""
    ro, rd, z = np.asarray(ro, f32), np.asarray(rd, f32), np.asarray(z, f32)
    with np.errstate(all='ignore'):
        return ro[:, None, :] + rd[:, None, :] * z[:, :, None]


def occ_mark_np(ro, rd, z, cells, lo, inv):
    """cells uint8 [G,G,G] indexed [cz,cy,cx] -> mask uint8 [R,S]: t = (p - lo)*inv; inside when 0 <= t < G on the three axes (false
    for NaN); then the byte of cell (int)t, else 0."""
    G = cells.shape[0]
    p = occ_points_np(ro, rd, z)
    with np.errstate(all='ignore'):
        t = (p - np.asarray(lo, f32)) * np.asarray(inv, f32)
        inside = np.all((t >= f32(0)) & (t < f32(G)), -1)
    c = t[inside].astype(np.int64)                       # truncation of a value in [0, G)
    mask = np.zeros(p.shape[:2], np.uint8)
    mask[inside] = cells[c[:, 2], c[:, 1], c[:, 0]]
    return mask


def occ_select_np(ro, rd, z, cells, lo, inv):
    """-> (idx int32 [n] ascending, pts float32 [n,3]): what OccupancyGrid.select and ctx_occ_points give."""
    mask = occ_mark_np(ro, rd, z, cells, lo, inv).reshape(-1)
    idx = np.flatnonzero(mask).astype(np.int32)
    return idx, occ_points_np(ro, rd, z).reshape(-1, 3)[idx]


def occ_cell_points_np(G, lo, h, u=None):
    """-> pts float32 [G^3,3], cell c = (cz*G + cy)*G + cx: per axis lo + ((float)c_axis + u)*h, u [G^3,3] or 0.5."""
    c = np.arange(G ** 3, dtype=np.int64)
    cax = np.stack([c % G, (c // G) % G, c // (G * G)], -1).astype(f32)
    u = np.full((G ** 3, 3), 0.5, f32) if u is None else np.asarray(u, f32)
    return np.asarray(lo, f32) + (cax + u) * np.asarray(h, f32)


def occ_update_np(raw, dens, decay, thresh):
    """raw [n,4], dens [n] -> (dens', cells uint8): sigma = raw.w > 0 ? raw.w : 0; dens' = fmaxf(dens*decay, sigma); cells = dens' > thresh;
    a NaN raw.w leaves sigma 0 and marks the cell."""
    w = np.asarray(raw, f32)[:, 3]
    with np.errstate(all='ignore'):
        sigma = np.where(w > f32(0), w, f32(0))
        dn = np.fmax(np.asarray(dens, f32) * f32(decay), sigma)
        cells = ((dn > f32(thresh)) | np.isnan(w)).astype(np.uint8)
    return dn.astype(f32), cells


def random_rays(rng, R, S, spread=1.0):
    """A pinhole-like batch around the origin: origins at distance 1.5, directions towards the box with `spread`, sorted depths."""
    ro = np.tile(f32([0.2, -0.1, 1.5]), (R, 1)) + rng.normal(0, 0.05, (R, 3)).astype(f32)
    rd = (f32([0, 0, -1]) + rng.normal(0, 0.4 * spread, (R, 3))).astype(f32)
    z = np.sort(rng.uniform(0.5, 2.5, (R, S)).astype(f32), -1)
    return ro, rd, z


# ---- 1. the selection rule -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,lo,hi", [(1, -1.0, 1.0), (4, -1.0, 1.0), (16, (-1.0, -0.5, 0.0), (1.0, 1.5, 4.0)), (128, -1.0, 1.0)])
def test_all_ones_marks_the_box_and_all_zeros_nothing(G, lo, hi):
    rng = np.random.default_rng(G)
    ro, rd, z = random_rays(rng, 37, 50)
    lo3, inv, _ = grid_consts(G, lo, hi)
    hi3 = np.broadcast_to(np.asarray(hi, f32), (3,))
    p = occ_points_np(ro, rd, z).astype(np.float64)
    in_box = np.all((p >= lo3) & (p < hi3), -1)                     # the box itself, no grid arithmetic
    assert 0 < in_box.sum() < in_box.size                           # rays enter and leave it
    assert np.array_equal(occ_mark_np(ro, rd, z, np.ones((G, G, G), np.uint8), lo3, inv) != 0, in_box)
    assert not occ_mark_np(ro, rd, z, np.zeros((G, G, G), np.uint8), lo3, inv).any()


def test_each_sample_reads_the_cell_that_holds_it():
    G = 8
    rng = np.random.default_rng(3)
    ro, rd, z = random_rays(rng, 21, 40)
    lo3, inv, h = grid_consts(G, -1.0, 1.0)
    cells = (rng.random((G, G, G)) < 0.5).astype(np.uint8)
    mask = occ_mark_np(ro, rd, z, cells, lo3, inv)
    p = occ_points_np(ro, rd, z).astype(np.float64)
    want = np.zeros_like(mask)
    for r in range(p.shape[0]):
        for s in range(p.shape[1]):
            c = np.floor((p[r, s] + 1.0) / 0.25).astype(int)        # h = 2 / 8, exact
            if np.all(c >= 0) and np.all(c < G):
                want[r, s] = cells[c[2], c[1], c[0]]
    assert np.array_equal(mask, want) and 0 < mask.sum() < mask.size
    idx, pts = occ_select_np(ro, rd, z, cells, lo3, inv)
    assert idx.dtype == np.int32 and np.all(np.diff(idx) > 0) and len(idx) == mask.sum()
    assert np.array_equal(pts, occ_points_np(ro, rd, z).reshape(-1, 3)[mask.reshape(-1) != 0])


def test_faces_and_nan():
    """On `lo` is inside (t = 0), on `hi` is outside (t = G: the extents here are powers of two, so (hi - lo)*inv is exactly G), a NaN
    coordinate is outside, and so is an infinite one."""
    G = 4
    lo3, inv, _ = grid_consts(G, (-1.0, -0.5, 0.0), (1.0, 1.5, 4.0))
    ones = np.ones((G, G, G), np.uint8)
    o = f32([[-1.0, -0.5, 0.0],          # the corner lo
             [1.0, 0.0, 1.0],            # on hi in x
             [0.0, 1.5, 1.0],            # on hi in y
             [0.0, 0.0, 4.0],            # on hi in z
             [0.0, 0.0, 0.0],            # on lo in z only
             [np.nan, 0.0, 1.0],
             [0.0, np.inf, 1.0],
             [np.nextafter(f32(-1.0), f32(-2.0)), 0.0, 1.0]])       # one ulp below lo
    d = np.zeros_like(o)
    z = np.ones((len(o), 1), f32)
    assert occ_mark_np(o, d, z, ones, lo3, inv).reshape(-1).tolist() == [1, 0, 0, 0, 1, 0, 0, 0]
    # a NaN direction or depth poisons its own ray only
    ro, rd, zz = random_rays(np.random.default_rng(0), 3, 9, spread=0.1)
    base = occ_mark_np(ro, rd, zz, ones, *grid_consts(G, -1.0, 1.0)[:2])
    rd2 = rd.copy(); rd2[1, 0] = np.nan
    got = occ_mark_np(ro, rd2, zz, ones, *grid_consts(G, -1.0, 1.0)[:2])
    assert base[1].any() and not got[1].any() and np.array_equal(got[[0, 2]], base[[0, 2]])


# ---- 2. the refresh --------------------------------------------------------------------------------------------------------------
def test_update_rule_on_hand_made_raw():
    w = f32([2.0, -3.0, 0.5, np.nan, 0.0, 0.25, np.inf])
    raw = np.zeros((len(w), 4), f32); raw[:, 3] = w
    dens = f32([0.0, 1.0, 1.0, 0.0, 0.5, 0.0, 0.0])
    dn, cells = occ_update_np(raw, dens, 0.5, 0.25)
    assert dn.dtype == f32 and cells.dtype == np.uint8
    assert dn.tolist() == [2.0, 0.5, 0.5, 0.0, 0.25, 0.25, np.inf]
    #                     new max; decayed; the larger of decayed and new; NaN: dens decays, cell stays; decayed to thresh: not occupied;
    #                     sigma == thresh: not occupied; +inf: occupied
    assert cells.tolist() == [1, 1, 1, 1, 0, 0, 1]
    # repeated refreshes from an empty field thin the grid out geometrically
    raw0 = np.zeros((1, 4), f32)
    d, steps = f32([1.0]), 0
    while occ_update_np(raw0, d, 0.95, 0.01)[1][0]:
        d = occ_update_np(raw0, d, 0.95, 0.01)[0]; steps += 1
    assert steps == 89                                               # 0.95^90 < 0.01 <= 0.95^89


@pytest.mark.parametrize("G", [1, 5, 32])
def test_cell_points_lie_in_their_cells(G):
    lo3, inv, h = grid_consts(G, (-1.0, -0.5, 0.0), (1.0, 1.5, 4.0))
    centres = occ_cell_points_np(G, lo3, h)
    assert centres.dtype == f32 and centres.shape == (G ** 3, 3)
    c = np.arange(G ** 3)
    want = np.stack([c % G, (c // G) % G, c // (G * G)], -1)
    assert np.array_equal(np.floor((centres - lo3) * inv).astype(np.int64), want)          # x is the fastest axis of the flat index
    u = np.random.default_rng(G).random((G ** 3, 3)).astype(f32)
    jit = occ_cell_points_np(G, lo3, h, u)
    assert np.all(np.abs(jit - centres) <= 0.5 * h + 1e-6) and not np.array_equal(jit, centres)
    # marking the cell points with a one-cell grid finds that cell and nothing else
    if G > 1:
        cells = np.zeros((G, G, G), np.uint8); cells[G // 2, 1, G - 1] = 1
        m = occ_mark_np(centres, np.zeros_like(centres), np.ones((G ** 3, 1), f32), cells, lo3, inv).reshape(-1)
        assert np.flatnonzero(m).tolist() == [((G // 2) * G + 1) * G + (G - 1)]


# ---- 3. host ----------------------------------------------------------------------------------------------------------------------
def test_grid_construction_and_refusals():
    from contexture_nerf_amd import _lib as L, volume_render as vr
    g = vr.OccupancyGrid(6, (-1.0, -0.5, 0.0), (1.0, 1.5, 4.0), 'cpu')
    lo3, inv, h = grid_consts(6, (-1.0, -0.5, 0.0), (1.0, 1.5, 4.0))
    assert np.array_equal(g.lo, lo3) and np.array_equal(g.inv, inv) and np.array_equal(g.h, h) and g.inv.dtype == f32
    assert g.cells.dtype == torch.uint8 and tuple(g.cells.shape) == (6, 6, 6) and bool(g.cells.all()) and not g.dens.any()
    assert g.fraction() == 1.0
    m = torch.zeros(4, 4, 4, dtype=torch.bool); m[1, 2, 3] = True
    gm = vr.OccupancyGrid.from_mask(m, -1.0, 1.0)
    assert gm.G == 4 and gm.fraction() == 1 / 64 and gm.cells[1, 2, 3] == 1 and gm.cells.dtype == torch.uint8
    for bad in (0, 257, -3):
        with pytest.raises(L.CtxError, match=r"outside \[1, 256\]"):
            vr.OccupancyGrid(bad, -1.0, 1.0, 'cpu')
    for lo, hi in ((1.0, 1.0), (1.0, -1.0), ((-1.0, 0.0, -1.0), (1.0, 0.0, 1.0)), (float('nan'), 1.0), (-1.0, float('inf'))):
        with pytest.raises(L.CtxError, match="lo < hi"):
            vr.OccupancyGrid(8, lo, hi, 'cpu')
    with pytest.raises(L.CtxError, match=r"\[G,G,G\]"):
        vr.OccupancyGrid.from_mask(torch.zeros(4, 4, 5, dtype=torch.bool), -1.0, 1.0)


def test_host_tensors_are_refused():
    from contexture_nerf_amd import _lib as L, volume_render as vr, run_nerf_helpers as rnh
    g = vr.OccupancyGrid(4, -1.0, 1.0, 'cpu')
    ro, rd, z = torch.zeros(2, 3), torch.ones(2, 3), torch.ones(2, 5)
    field = rnh.NeRF2D(D=2, W=64, input_ch=63, output_ch=4, skips=[0])
    with pytest.raises(L.CtxError, match="device tensor"):
        g.select(ro, rd, z)
    with pytest.raises(L.CtxError, match="device tensor"):
        g.cell_points()
    with pytest.raises(L.CtxError, match="device tensor"):
        g.update(field, 0.01)
    with pytest.raises(L.CtxError, match="device tensor"):
        rnh.render_rays(field, ro, rd, 0.5, 2.5, 5, occupancy=g)
    with pytest.raises(L.CtxError, match="device tensor"):
        rnh.field_on_occupied(field, g, ro, rd, z)
    with pytest.raises(L.CtxError, match="device tensor"):
        rnh._OccExpandFn.apply(torch.zeros(1, 4), torch.zeros(1, dtype=torch.int32), 4)
    opt = types.SimpleNamespace(zero_grad=lambda set_to_none=True: None, step=lambda: None)
    with pytest.raises(L.CtxError, match="device tensor"):
        vr.train_step(field, opt, ro, rd, torch.zeros(2, 3), 0.5, 2.5, 5, occupancy=g)
    with pytest.raises(L.CtxError, match="z_vals"):
        g.select(ro, rd, z.clone().requires_grad_(True))
    with pytest.raises(L.CtxError, match="z_vals"):
        rnh.render_rays(field, ro, rd, 0.5, 2.5, 5, z_vals=z.clone().requires_grad_(True), occupancy=g)


class _Recorder:
    """An OccupancyGrid stand-in: records before which iteration `update` ran."""

    def __init__(self, steps):
        self.steps, self.updates = steps, []

    def update(self, field, thresh, decay=0.95, generator=None):
        assert isinstance(generator, torch.Generator)               # the loop's own seeded generator
        self.updates.append((len(self.steps), thresh))


def _fit(monkeypatch, **kw):
    from contexture_nerf_amd import volume_render as vr
    steps = []
    monkeypatch.setattr(vr.rnh, 'get_rays', lambda H, W, K, c2w: (torch.zeros(H, W, 3), torch.ones(H, W, 3)))

    def fake_step(field, opt, ro, rd, target, near, far, N_samples, **k):
        steps.append(k.get('occupancy'))
        return {'loss': torch.tensor(float(len(steps))), 'psnr': torch.tensor(0.)}
    monkeypatch.setattr(vr, 'train_step', fake_step)
    field = torch.nn.Linear(3, 4)
    occ = _Recorder(steps) if kw.pop('with_grid', True) else None
    hist = vr.fit_views(field, torch.zeros(1, 4, 4, 3), torch.zeros(1, 3, 4), vr.pinhole(4, 4), 0.5, 2.5, kw.pop('iters'), rays_per_iter=8,
                        occupancy=occ, **kw)
    return hist, steps, occ


def test_fit_views_update_schedule(monkeypatch):
    hist, steps, occ = _fit(monkeypatch, iters=40, occupancy_warmup=10, occupancy_every=8, occupancy_thresh=0.5)
    assert hist == [float(i) for i in range(1, 41)] and all(s is occ for s in steps)
    assert occ.updates == [(10, 0.5), (18, 0.5), (26, 0.5), (34, 0.5)]
    _, _, occ = _fit(monkeypatch, iters=70)                                       # defaults: warm-up 32, every 16
    assert [u[0] for u in occ.updates] == [32, 48, 64] and occ.updates[0][1] == 0.01
    _, _, occ = _fit(monkeypatch, iters=20, occupancy_warmup=32)
    assert occ.updates == []                                                     # never past the warm-up
    _, _, occ = _fit(monkeypatch, iters=3, occupancy_warmup=0, occupancy_every=1)
    assert [u[0] for u in occ.updates] == [0, 1, 2]
    hist, steps, occ = _fit(monkeypatch, iters=5, with_grid=False)
    assert steps == [None] * 5 and len(hist) == 5


def test_train_step_without_an_occupied_sample_skips_the_step(monkeypatch):
    from contexture_nerf_amd import volume_render as vr
    calls = []
    opt = types.SimpleNamespace(zero_grad=lambda set_to_none=True: calls.append('zero'), step=lambda: calls.append('step'))
    w = torch.nn.Parameter(torch.ones(()))

    def fake_render(field, ro, rd, near, far, N, **k):
        rgb = torch.full((4, 3), 0.5) * (w if k['occupancy'] == 'some' else 1.0)
        return (rgb, None, None, None, None), {}
    monkeypatch.setattr(vr.rnh, 'render_rays', fake_render)
    tgt = torch.zeros(4, 3)
    out = vr.train_step(None, opt, None, None, tgt, 0.5, 2.5, 8, occupancy='none')
    assert calls == ['zero'] and float(out['loss']) == 0.25 and abs(float(out['psnr']) - 6.0206) < 1e-3
    out = vr.train_step(None, opt, None, None, tgt, 0.5, 2.5, 8, occupancy='some')
    assert calls == ['zero', 'zero', 'step'] and abs(float(w.grad) - 0.5) < 1e-6
    # the dense path is what it was: a loss without a graph is an error there, not a skipped step
    monkeypatch.setattr(vr.rnh, 'render_rays', lambda *a, **k: ((torch.full((4, 3), 0.5), None, None, None, None), {}))
    with pytest.raises(RuntimeError):
        vr.train_step(None, opt, None, None, tgt, 0.5, 2.5, 8)
