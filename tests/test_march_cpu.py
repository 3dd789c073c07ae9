"""CPU: the march rule against float64 dense sampling, the packed closed-form backward against float64 autograd, and
the host-side refusals and pass-through of `march=`.  The restatements live in tests/march_rule.py."""
import types
import numpy as np
import pytest
import torch

import march_rule as mr
from test_occupancy_cpu import grid_consts
from test_occupancy_mesh_cpu import occ_ray_spans_np, span_rays

f32 = np.float32
NEAR, FAR = 0.5, 2.5
NZ = 4096


def _dense_inside(ro, rd, cells, lo, hi):
    """float64 dense sampling at 4096 z per ray -> (z [NZ], inside bool [R,NZ], occupied bool [R,NZ]): the samples whose point lies in an
    occupied cell, `inside` only those at least 1e-3 of a cell from any cell boundary."""
    G = cells.shape[0]
    z = NEAR + (np.arange(NZ) + 0.5) * ((FAR - NEAR) / NZ)
    with np.errstate(all='ignore'):
        p = ro.astype(np.float64)[:, None, :] + rd.astype(np.float64)[:, None, :] * z[None, :, None]
        t = (p - lo) / (hi - lo) * G
        fl = np.floor(t)
        ingrid = np.all((fl >= 0) & (fl < G), -1)
        clear = ingrid & np.all((t - fl >= 1e-3) & (t - fl <= 1 - 1e-3), -1)
        c = np.where(ingrid[..., None], fl, 0).astype(int)
    occ = ingrid & (cells[c[..., 2], c[..., 1], c[..., 0]] != 0)
    return z, clear & occ, occ


@pytest.mark.parametrize("name,G,cells,R,seed", mr.march_cases(), ids=[c[0] for c in mr.march_cases()])
def test_march_rule_against_float64_dense_sampling(name, G, cells, R, seed):
    ro, rd = span_rays(np.random.default_rng(seed), R)
    lo3, inv, h = grid_consts(G, -1.0, 1.0)
    hi3 = f32([1, 1, 1])
    z, inside, occupied = _dense_inside(ro, rd, cells, -1.0, 1.0)
    dz = (FAR - NEAR) / NZ
    finite = np.all(np.isfinite(ro), -1) & np.all(np.isfinite(rd), -1)
    ta, tb, ok, steps = mr.occ_walk_np(ro, rd, NEAR, FAR, cells, lo3, hi3, inv, h)
    span, hit = mr.spans_from_walk(steps, R, NEAR, FAR)
    want_span, want_hit = occ_ray_spans_np(ro, rd, NEAR, FAR, cells, lo3, hi3, inv, h)
    assert np.array_equal(span, want_span) and np.array_equal(hit, want_hit)          # one walk: the span rule's bits
    nrm = np.where(finite, np.linalg.norm(np.where(finite[:, None], rd, 0).astype(np.float64), axis=-1), 0.0)
    for step in mr.march_steps(G):
        count, ray_off, ray_id, t, dt, pts, (run_ray, a, b, k) = mr.occ_march_np(ro, rd, NEAR, FAR, cells, lo3, hi3, inv, h, step)
        assert count.dtype == np.int32 and t.dtype == f32 and dt.dtype == f32 and pts.dtype == f32 and ray_id.dtype == np.int32
        assert ray_off[-1] == len(t) == count.sum() and np.all(count[~finite] == 0) and np.all(count[~ok] == 0)
        assert count.max(initial=0) <= mr.march_bound(G, -1.0, 1.0, step)
        assert np.array_equal(ray_id, np.repeat(np.arange(R), count).astype(np.int32))
        if not cells.any():
            assert len(t) == 0
        runs = np.bincount(run_ray[k > 0], minlength=R)
        t64, dt64 = t.astype(np.float64), dt.astype(np.float64)
        assert np.all(dt64 * nrm[ray_id] <= step * (1 + 2.0 ** -20))
        for r in range(R):
            s = slice(ray_off[r], ray_off[r + 1])
            lo_i, hi_i = t64[s] - 0.5 * dt64[s], t64[s] + 0.5 * dt64[s]
            zin = z[inside[r]]
            if nrm[r] == 0:                                     # a zero direction stays in its cell but has no world length: the rule
                assert count[r] == 0                            # (len > 0) gives it no sample, so there is no interval to lie in
            elif len(zin):
                assert count[r] > 0, (r, step)
                i = np.searchsorted(lo_i - 1e-4, zin, 'right') - 1
                assert np.all(i >= 0) and np.all(zin <= hi_i[i] + 1e-4), (r, step)
            if count[r]:
                slack = 2.0 ** -20 * np.maximum(1.0, np.abs(t64[s]))
                assert np.all(np.diff(t64[s]) > 0) and np.all(lo_i[1:] >= hi_i[:-1] - slack[1:]), (r, step)
                assert lo_i[0] >= ta[r] - slack[0] and hi_i[-1] <= tb[r] + slack[-1], (r, step)
            # sum dt * |d| = the float64 occupied length to within one step per run
            got = float(np.sum(dt64[s])) * nrm[r] if finite[r] else 0.0
            want = float(occupied[r].sum()) * dz * nrm[r] if finite[r] else 0.0
            assert abs(got - want) <= runs[r] * step, (r, step, got, want)
    # a given u moves the samples inside their intervals and nothing else
    step = mr.march_steps(G)[0]
    c0, off0, id0, t0, dt0, _, _ = mr.occ_march_np(ro, rd, NEAR, FAR, cells, lo3, hi3, inv, h, step)
    u = np.random.default_rng(seed + 1).random(len(t0)).astype(f32)
    c1, off1, id1, t1, dt1, p1, _ = mr.occ_march_np(ro, rd, NEAR, FAR, cells, lo3, hi3, inv, h, step, u=u)
    assert np.array_equal(c0, c1) and np.array_equal(dt0, dt1) and np.array_equal(id0, id1)
    assert np.all(np.abs(t1.astype(np.float64) - t0) <= 0.5 * dt0.astype(np.float64) * (1 + 1e-6) + 1e-7)
    assert np.array_equal(p1, (ro[id1] + rd[id1] * t1[:, None]).astype(f32))


def test_zero_length_empty_cell_closes_the_run():
    """A ray along a cell edge of a checkerboard: the walk meets empty cells of zero length between occupied ones; each closes the open
    run, so the two occupied cells are two runs with their own ceil."""
    G = 2
    lo3, inv, h = grid_consts(G, -1.0, 1.0)
    cells = np.zeros((G, G, G), np.uint8)
    cells[0, 0, 0] = cells[1, 1, 1] = 1
    ro, rd = f32([[-2.0, -2.0, -2.0]]), f32([[1.0, 1.0, 1.0]])                      # the diagonal: x, y and z exits tie at the centre
    _, _, _, steps = mr.occ_walk_np(ro, rd, 0.5, 4.0, cells, lo3, f32([1, 1, 1]), inv, h)
    ray, a, b = mr.occ_runs_np(steps, 1)
    assert len(ray) == 2 and b[0] == a[1] == f32(2.0) and a[0] == f32(1.0) and b[1] == f32(3.0)
    count, _, _, t, dt, _, _ = mr.occ_march_np(ro, rd, 0.5, 4.0, cells, lo3, f32([1, 1, 1]), inv, h, 1.0)
    assert count[0] == 4 and np.allclose(dt, 0.5)                                   # two runs of world length sqrt(3): ceil twice


COUNT_SET = (0, 1, 2, 63, 64, 65, 130)


def ragged_counts(R, seed):
    c = np.random.default_rng(seed).choice(COUNT_SET, R)
    c[:len(COUNT_SET)] = COUNT_SET[::-1][:R]                    # every count occurs
    c[0] = c[-1] = 0                                            # the first and the last ray are empty
    return c


@pytest.mark.parametrize("white", (False, True))
@pytest.mark.parametrize("with_noise", (False, True))
def test_packed_closed_form_matches_float64_autograd(white, with_noise):
    counts = ragged_counts(12, 3)
    raw, t, dt, d, ray_off, noise = mr.make_packed_case(counts, seed=11, with_noise=with_noise)
    full = mr.make_packed_grads(len(counts), raw.shape[0], seed=5)
    for keep in ((0, 1, 2, 3, 4), (0,), (3,)):
        grads = [g if i in keep else None for i, g in enumerate(full)]
        want = mr.packed_autograd_grad(raw, t, dt, d, ray_off, noise, white, grads)
        got = mr.packed_closed_form(raw, t, dt, d, ray_off, noise, white, grads)
        assert torch.isfinite(got).all()
        assert mr.ray_ratio(got, want, ray_off) <= 1e-12, (keep, mr.ray_ratio(got, want, ray_off))
        pre = raw[:, 3] if noise is None else raw[:, 3] + noise
        assert (got[:, 3][pre <= 0] == 0).all()
    # the empty rays of the formula
    rgb, disp, acc, w, depth = mr.restate_packed(raw.double(), t.double(), dt.double(), d.double(), ray_off, None, white)
    for r in (0, len(counts) - 1):
        assert acc[r] == 0 and depth[r] == 0 and torch.isnan(disp[r]) and (rgb[r] == (1.0 if white else 0.0)).all()


def test_packed_formula_is_the_dense_one_on_a_rectangular_layout():
    """ray_off = arange(R+1)*S, dt = cat(z[:,1:] - z[:,:-1], 1e10), t = z: the packed formula is nerf-pytorch's raw2outputs."""
    from test_raymarch_train_cpu import make_case, restate
    raw, z, d, _ = make_case(4, 33, seed=2)
    dt = torch.cat([z[:, 1:] - z[:, :-1], torch.full((4, 1), 1e10)], -1)
    got = mr.restate_packed(raw.reshape(-1, 4).double(), z.reshape(-1).double(), dt.reshape(-1).double(), d.double(), torch.arange(5) * 33)
    want = restate(raw.double(), z.double(), d.double())
    for g, w in zip(got, want):
        assert torch.allclose(g.reshape(w.shape), w, rtol=1e-12, atol=1e-14, equal_nan=True)


# ---- the host side --------------------------------------------------------------------------------------------------------------------------
def test_march_refusals_on_the_host():
    from contexture_nerf_amd import _lib as L, volume_render as vr, run_nerf_helpers as rnh
    ro, rd, z = torch.zeros(2, 3), torch.ones(2, 3), torch.ones(2, 5)
    field = rnh.NeRF2D(D=2, W=64, input_ch=63, output_ch=4, skips=[0])
    g = vr.OccupancyGrid(4, -1.0, 1.0, 'cpu')
    with pytest.raises(L.CtxError, match="march needs an occupancy grid"):
        rnh.render_rays(field, ro, rd, 0.5, 2.5, 5, march=0.1)
    with pytest.raises(L.CtxError, match="cannot be combined with pytest=True"):
        rnh.render_rays(field, ro, rd, 0.5, 2.5, 5, occupancy=g, pytest=True, march=0.1)
    with pytest.raises(L.CtxError, match="cannot be combined with clip=True"):
        rnh.render_rays(field, ro, rd, 0.5, 2.5, 5, occupancy=g, clip=True, march=0.1)
    with pytest.raises(L.CtxError, match="cannot be combined with N_importance > 0"):
        rnh.render_rays(field, ro, rd, 0.5, 2.5, 5, occupancy=g, N_importance=4, march=0.1)
    with pytest.raises(L.CtxError, match="cannot be combined with given z_vals"):
        rnh.render_rays(field, ro, rd, 0.5, 2.5, 5, occupancy=g, z_vals=z, march=0.1)
    with pytest.raises(L.CtxError, match="march needs an occupancy grid"):
        vr.train_step(field, torch.optim.SGD(field.parameters(), lr=0.1), ro, rd, torch.zeros(2, 3), 0.5, 2.5, 5, march=0.1)
    with pytest.raises(L.CtxError, match="march needs an occupancy grid"):
        rnh.render_rays_marched(field, ro, rd, 0.5, 2.5, None, 0.1)
    # a step whose bound exceeds what the compositing backward holds: refused before any pointer is taken
    step = 2 * np.sqrt(3) / 4096
    assert g.march_bound(step) > 4096 and g.march_bound(step) == mr.march_bound(4, -1.0, 1.0, step)
    with pytest.raises(L.CtxError, match="the compositing backward holds 4096"):
        g.march(ro, rd, 0.5, 2.5, step)
    big = vr.OccupancyGrid(128, -1.0, 1.0, 'cpu')
    h = 2.0 / 128
    assert [big.march_bound(h / k) <= 4096 for k in (1, 2, 4, 16, 32)] == [True, True, True, True, False]
    with pytest.raises(L.CtxError, match="finite world length > 0"):
        g.march(ro, rd, 0.5, 2.5, 0.0)
    with pytest.raises(L.CtxError, match="finite near < far"):
        g.march(ro, rd, 2.5, 0.5, 0.1)
    with pytest.raises(L.CtxError, match="device tensor"):                          # no CPU fallback
        g.march(ro, rd, 0.5, 2.5, 0.1)
    with pytest.raises(L.CtxError, match="device tensor"):
        rnh.raw2outputs_packed(torch.zeros(3, 4), torch.zeros(3), torch.zeros(3), rd, torch.tensor([0, 1, 3]))
    with pytest.raises(L.CtxError, match="t / dt / rays_d"):
        rnh.raw2outputs_packed(torch.zeros(3, 4), torch.zeros(3).requires_grad_(True), torch.zeros(3), rd, torch.tensor([0, 1, 3]))
    with pytest.raises(L.CtxError, match="t / dt / rays_d"):
        rnh.raw2outputs_packed(torch.zeros(3, 4), torch.zeros(3), torch.zeros(3).requires_grad_(True), rd, torch.tensor([0, 1, 3]))
    with pytest.raises(L.CtxError, match=r"ray_off \[R\+1\]"):
        rnh.raw2outputs_packed(torch.zeros(3, 4), torch.zeros(3), torch.zeros(3), rd, torch.tensor([0, 3]))


def test_march_passes_through_the_entry_points(monkeypatch):
    from contexture_nerf_amd import volume_render as vr
    seen = []

    def fake_render(field, ro, rd, near, far, N, **k):
        seen.append(k.get('march'))
        w = torch.ones(ro.shape[0], 3, requires_grad=True)
        return ((w, w[:, 0], w[:, 0], w, w[:, 0]), {}) if k.get('return_extras') else (w, w[:, 0], w[:, 0], w, w[:, 0])
    monkeypatch.setattr(vr.rnh, 'render_rays', fake_render)
    monkeypatch.setattr(vr.rnh, 'get_rays', lambda H, W, K, c2w: (torch.zeros(H, W, 3), torch.ones(H, W, 3)))
    opt = types.SimpleNamespace(zero_grad=lambda set_to_none=True: None, step=lambda: None)
    vr.render_image(None, 2, 2, vr.pinhole(2, 2), None, 0.5, 2.5, 4, occupancy='g', march=0.25)
    vr.render_image(None, 2, 2, vr.pinhole(2, 2), None, 0.5, 2.5, 4, occupancy='g')
    vr.train_step(None, opt, torch.zeros(4, 3), torch.ones(4, 3), torch.zeros(4, 3), 0.5, 2.5, 4, occupancy='g', march=0.125)
    vr.train_step(None, opt, torch.zeros(4, 3), torch.ones(4, 3), torch.zeros(4, 3), 0.5, 2.5, 4)
    assert seen == [0.25, None, 0.125, None]
    seen.clear()
    monkeypatch.setattr(vr, 'train_step', lambda *a, **k: seen.append(k.get('march')) or {'loss': torch.tensor(1.0)})
    vr.fit_views(torch.nn.Linear(3, 4), torch.zeros(1, 4, 4, 3), torch.zeros(1, 3, 4), vr.pinhole(4, 4), 0.5, 2.5, 3, rays_per_iter=8,
                 occupancy='g', occupancy_every=0, march=0.5)
    assert seen == [0.5] * 3
    seen.clear()
    def stop(*a, **k):
        seen.append(k.get('march'))
        raise KeyboardInterrupt
    monkeypatch.setattr(vr, 'render_image', stop)
    with pytest.raises(KeyboardInterrupt):
        vr.render_and_refine(None, None, None, 4, 4, None, occupancy='g', march=0.75)
    assert seen == [0.75]
