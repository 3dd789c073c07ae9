"""CPU: the resampling rule against the float64 CDF at the derived bounds, its order and conservation properties, and
the host-side refusals and pass-through of `resample=`.  The restatement lives in tests/resample_rule.py."""
import types
import numpy as np
import pytest
import torch

import resample_rule as rr

f32 = np.float32
S_SET = (1, 2, 19, 63, 64, 65, 130, 500, 4096)
K_SET = (1, 2, 16, 64, 65, 200)


def _grid_counts():
    """One ray per (S, weight shape, number of runs): make_lists cycles the shapes fastest, then the runs."""
    return [S for S in S_SET for _ in range(len(rr.SHAPES) * 3)]


_LISTS = {}


def _lists(key, counts, seed):
    if key not in _LISTS:
        _LISTS[key] = rr.make_lists(counts, seed)
    return _LISTS[key]


def _check_properties(w, ts, dt, ray_off, fine_off, ray_id, t1, dt1, K):
    assert t1.dtype == f32 and dt1.dtype == f32 and ray_id.dtype == np.int32
    assert np.all(np.isfinite(t1)) and np.all(np.isfinite(dt1)) and np.all(dt1 >= 0)
    hit = np.diff(ray_off) > 0
    assert np.array_equal(fine_off, np.concatenate([[0], np.cumsum(hit) * K]))
    assert np.array_equal(ray_id, np.repeat(np.arange(len(hit)), hit * K).astype(np.int32))
    for r in np.nonzero(hit)[0]:
        s, o = slice(ray_off[r], ray_off[r + 1]), slice(fine_off[r], fine_off[r + 1])
        S = ray_off[r + 1] - ray_off[r]
        assert np.all(rr.in_coarse_interval(ts[s], dt[s], t1[o])), r
        # ascending; at a joint of two intervals, whose ends are binary32 sums a + j*dt of their own, up to two ulps
        assert np.all(np.diff(t1[o].astype(np.float64)) >= -2 * np.spacing(t1[o][1:]).astype(np.float64)), r
        L = float(np.sum(dt[s].astype(np.float64)))
        assert abs(float(np.sum(dt1[o].astype(np.float64))) - L) <= (S + K) * 2.0 ** -23 * L, r


@pytest.mark.parametrize("order", ("seq", "wave"))
@pytest.mark.parametrize("drawn", (False, True))
@pytest.mark.parametrize("K", K_SET)
def test_rule_meets_the_contract_in_mass(K, drawn, order):
    counts = _grid_counts()
    w, ts, dt, ray_off, ro, rd = _lists('grid', counts, seed=17)
    xi = np.random.default_rng(K).random(len(counts) * K).astype(f32) if drawn else None
    fine_off, ray_id, t1, dt1, pts = rr.resample_np(w, ts, dt, ray_off, ro, rd, K, xi=xi, order=order)
    _check_properties(w, ts, dt, ray_off, fine_off, ray_id, t1, dt1, K)
    assert np.array_equal(pts, (ro[ray_id] + rd[ray_id] * t1[:, None]).astype(f32))
    ra, rb, rB = rr.contract_ratios(w, ts, dt, ray_off, fine_off, t1, dt1, K, xi, order)
    print(f"K={K} drawn={drawn} order={order}: largest error / bound (a) {ra:.3f}, (b) {rb:.3f}; (b) over (S+8) 2^-23 alone {rB:.2f}")
    assert ra <= 1.0 and rb <= 1.0, (ra, rb)


@pytest.mark.parametrize("order", ("seq", "wave"))
def test_rule_at_the_largest_K(order):
    counts = [1, 2, 19, 65, 0, 19, 2, 1, 65, 130, 19, 64]
    w, ts, dt, ray_off, ro, rd = _lists('small', counts, seed=23)
    K = rr.MAX_K
    xi = np.random.default_rng(4).random(int((np.array(counts) > 0).sum()) * K).astype(f32)
    for x in (None, xi):
        fine_off, ray_id, t1, dt1, _ = rr.resample_np(w, ts, dt, ray_off, ro, rd, K, xi=x, order=order)
        _check_properties(w, ts, dt, ray_off, fine_off, ray_id, t1, dt1, K)
        ra, rb, rB = rr.contract_ratios(w, ts, dt, ray_off, fine_off, t1, dt1, K, x, order)
        print(f"K={K} drawn={x is not None} order={order}: largest error / bound (a) {ra:.3f}, (b) {rb:.3f}; (b) over (S+8) 2^-23 alone {rB:.2f}")
        assert ra <= 1.0 and rb <= 1.0, (ra, rb)


@pytest.mark.parametrize("order", ("seq", "wave"))
def test_flat_weights_resample_uniformly_in_occupied_length(order):
    """Flat weights on intervals of one width: F_l is the straight line l / L, so every stratum has the width L / K to within twice the bound of (b) times L,
    B = (S+8) 2^-23 + (S+2) 2^-24, and sample k sits at the occupied length (k + 0.5) L / K to within the bound of (a) times L."""
    for S, K, runs in ((19, 16, 1), (130, 65, 1), (500, 200, 1), (64, 64, 1)):
        rng = np.random.default_rng(S)
        ts, dt = rr.make_intervals(rng, S, runs)
        w = np.full(S, 0.25, f32)
        off = np.array([0, S])
        _, _, t1, dt1, _ = rr.resample_np(w, ts, dt, off, np.zeros((1, 3), f32), np.ones((1, 3), f32), K, order=order)
        dt64 = dt.astype(np.float64)
        L = dt64.sum()
        B = (S + 8) * 2.0 ** -23 + (S + 2) * 2.0 ** -24
        assert np.all(np.abs(dt1.astype(np.float64) - L / K) <= 2 * B * L), np.abs(dt1 - L / K).max()
        i = np.clip(np.searchsorted(ts, t1, 'right') - 1, 0, S - 1)
        ell = np.concatenate([[0.0], np.cumsum(dt64)])[i] + np.clip(t1.astype(np.float64) - ts[i], 0, dt64[i])
        Ba = (S + 8) * 2.0 ** -23 + 2.0 ** -22 * (np.abs(t1) + dt[i]) / dt64[i] / S
        assert np.all(np.abs(ell / L - (np.arange(K) + 0.5) / K) <= Ba)


@pytest.mark.parametrize("order", ("seq", "wave"))
def test_a_single_heavy_interval_takes_its_share(order):
    """w_j = 1 in one interval and 0 elsewhere: m_j / W = (1 + 1e-5) / (1 + S * 1e-5) >= 1 / (1 + S * 1e-5) of the K strata's midpoints fall
    into interval j, less one for each of its two ends."""
    for S, K, j in ((19, 16, 7), (71, 64, 70), (130, 200, 64), (500, 65, 0), (4096, 200, 3000)):
        ts, dt = rr.make_intervals(np.random.default_rng(S + K), S, 2)
        w = np.zeros(S, f32)
        w[j] = 1
        _, _, t1, _, _ = rr.resample_np(w, ts, dt, np.array([0, S]), np.zeros((1, 3), f32), np.ones((1, 3), f32), K, order=order)
        inside = rr.in_coarse_interval(ts[j:j + 1], dt[j:j + 1], t1)
        assert inside.sum() >= int(np.floor(K / (1 + S * 1e-5))) - 1, (S, K, j, inside.sum())


def test_bad_weights_count_as_their_clamped_values():
    counts = [5, 64, 0, 130]
    w, ts, dt, ray_off, ro, rd = rr.make_lists(counts, seed=3)
    bad = w.copy()
    bad[[0, 70, 100]] = np.nan
    bad[[1, 6, 150]] = -3.0
    bad[[2, 68, 198]] = np.inf
    bad[[3, 71]] = 7.5
    bad[4] = -np.inf
    want = rr.clamped(bad)
    assert np.all(np.isfinite(want)) and want[0] == 0 and want[1] == 0 and want[2] == 1 and want[3] == 1 and want[4] == 0
    for order in ("seq", "wave"):
        got = rr.resample_np(bad, ts, dt, ray_off, ro, rd, 16, order=order)
        ref = rr.resample_np(want, ts, dt, ray_off, ro, rd, 16, order=order)
        assert all(np.array_equal(a, b) for a, b in zip(got, ref)) and all(np.all(np.isfinite(a)) for a in got[2:])


def test_running_maximum_and_min_are_identities_on_sequential_sums():
    """What makes the rule `l(u) = l_i + f*dt_i` with plain prefix sums: on sequential sums neither guard changes a bit."""
    rng = np.random.default_rng(9)
    for S in (19, 500, 4096):
        v = (rng.random(S) * rng.choice([1e-5, 1e-2, 1.0], S)).astype(f32)
        ex, inc, tot = rr.prefix(v, 'seq')
        assert np.array_equal(inc, np.cumsum(v, dtype=f32)) and tot == inc[-1]
        f = rng.random(S).astype(f32)
        f[::7] = 1
        assert np.all((ex + f * v).astype(f32) <= inc)
        # the kernel's order gives the same sums to within the summation error, and non-descending ones
        _, winc, wtot = rr.prefix(v, 'wave')
        assert np.all(np.diff(winc) >= 0) and wtot == winc[-1]
        assert np.all(np.abs(winc.astype(np.float64) - np.cumsum(v.astype(np.float64))) <= S * 2.0 ** -24 * float(v.sum()))


# ---- the host side --------------------------------------------------------------------------------------------------------------------------
def test_resample_refusals_on_the_host():
    from contexture_nerf_amd import _lib as L, volume_render as vr, run_nerf_helpers as rnh
    assert "ctx_resample_packed" in L.SIGNATURES
    ro, rd = torch.zeros(2, 3), torch.ones(2, 3)
    field = rnh.NeRF2D(D=2, W=64, input_ch=63, output_ch=4, skips=[0])
    g = vr.OccupancyGrid(4, -1.0, 1.0, 'cpu')
    with pytest.raises(L.CtxError, match="it needs march="):
        rnh.render_rays(field, ro, rd, 0.5, 2.5, 5, resample=8)
    with pytest.raises(L.CtxError, match="it needs march="):
        rnh.render_rays(field, ro, rd, 0.5, 2.5, 5, occupancy=g, resample=8)
    with pytest.raises(L.CtxError, match="it needs march="):
        vr.train_step(field, torch.optim.SGD(field.parameters(), lr=0.1), ro, rd, torch.zeros(2, 3), 0.5, 2.5, 5, resample=8)
    for bad in (0.5, -1, 4097, 8.0, True, None, "8"):
        with pytest.raises(L.CtxError, match="resample="):
            rnh.render_rays(field, ro, rd, 0.5, 2.5, 5, occupancy=g, march=0.1, resample=bad)
        with pytest.raises(L.CtxError, match="resample="):                         # before any pointer is taken: the CPU rays never get there
            rnh.render_rays_marched(field, ro, rd, 0.5, 2.5, g, 0.1, resample=bad)
    with pytest.raises(L.CtxError, match="march needs an occupancy grid"):
        rnh.render_rays(field, ro, rd, 0.5, 2.5, 5, march=0.1, resample=8)
    with pytest.raises(L.CtxError, match="cannot be combined with N_importance > 0"):   # the hierarchical pass of the lists is resample=, not this
        rnh.render_rays(field, ro, rd, 0.5, 2.5, 5, occupancy=g, N_importance=4, march=0.1, resample=8)
    w, ts, dt, off = torch.zeros(3), torch.zeros(3), torch.ones(3), torch.tensor([0, 1, 3])
    for bad in (0.5, -1, 0, 4097):
        with pytest.raises(L.CtxError, match=r"want an int in \[1, 4096\]"):
            rnh.resample_packed(w, ts, dt, off, ro, rd, bad)
    for k in range(3):
        args = [w, ts, dt]
        args[k] = args[k].clone().requires_grad_(True)
        with pytest.raises(L.CtxError, match="detach them"):
            rnh.resample_packed(*args, off, ro, rd, 8)
    with pytest.raises(L.CtxError, match=r"ray_off \[R\+1\]"):
        rnh.resample_packed(w, ts, dt, torch.tensor([0, 3]), ro, rd, 8)
    with pytest.raises(L.CtxError, match=r"ts \[n\]"):
        rnh.resample_packed(w, torch.zeros(4), dt, off, ro, rd, 8)
    with pytest.raises(L.CtxError, match="device tensor"):                          # no CPU fallback
        rnh.resample_packed(w, ts, dt, off, ro, rd, 8)
    with pytest.raises(L.CtxError, match="device tensor"):
        g.march(ro, rd, 0.5, 2.5, 0.1, starts=True)


def test_resample_passes_through_the_entry_points(monkeypatch):
    from contexture_nerf_amd import volume_render as vr, run_nerf_helpers as rnh
    seen = []

    def fake_marched(field, ro, rd, near, far, occupancy, step, **k):
        seen.append((step, k.get('resample')))
        return 'out'
    monkeypatch.setattr(rnh, 'render_rays_marched', fake_marched)
    assert rnh.render_rays(None, None, None, 0.5, 2.5, 4, occupancy='g', march=0.25, resample=8) == 'out'
    assert rnh.render_rays(None, None, None, 0.5, 2.5, 4, occupancy='g', march=0.25) == 'out'
    assert seen == [(0.25, 8), (0.25, 0)]
    seen.clear()

    def fake_render(field, ro, rd, near, far, N, **k):
        seen.append((k.get('march'), k.get('resample')))
        w = torch.ones(ro.shape[0], 3, requires_grad=True)
        return ((w, w[:, 0], w[:, 0], w, w[:, 0]), {}) if k.get('return_extras') else (w, w[:, 0], w[:, 0], w, w[:, 0])
    monkeypatch.setattr(vr.rnh, 'render_rays', fake_render)
    monkeypatch.setattr(vr.rnh, 'get_rays', lambda H, W, K, c2w: (torch.zeros(H, W, 3), torch.ones(H, W, 3)))
    opt = types.SimpleNamespace(zero_grad=lambda set_to_none=True: None, step=lambda: None)
    vr.render_image(None, 2, 2, vr.pinhole(2, 2), None, 0.5, 2.5, 4, occupancy='g', march=0.25, resample=16)
    vr.render_image(None, 2, 2, vr.pinhole(2, 2), None, 0.5, 2.5, 4, occupancy='g', march=0.25)
    vr.train_step(None, opt, torch.zeros(4, 3), torch.ones(4, 3), torch.zeros(4, 3), 0.5, 2.5, 4, occupancy='g', march=0.125, resample=32)
    vr.train_step(None, opt, torch.zeros(4, 3), torch.ones(4, 3), torch.zeros(4, 3), 0.5, 2.5, 4)
    assert seen == [(0.25, 16), (0.25, 0), (0.125, 32), (None, 0)]
    seen.clear()
    monkeypatch.setattr(vr, 'train_step', lambda *a, **k: seen.append((k.get('march'), k.get('resample'))) or {'loss': torch.tensor(1.0)})
    vr.fit_views(torch.nn.Linear(3, 4), torch.zeros(1, 4, 4, 3), torch.zeros(1, 3, 4), vr.pinhole(4, 4), 0.5, 2.5, 3, rays_per_iter=8,
                 occupancy='g', occupancy_every=0, march=0.5, resample=4)
    assert seen == [(0.5, 4)] * 3
    seen.clear()

    def stop(*a, **k):
        seen.append((k.get('march'), k.get('resample')))
        raise KeyboardInterrupt
    monkeypatch.setattr(vr, 'render_image', stop)
    with pytest.raises(KeyboardInterrupt):
        vr.render_and_refine(None, None, None, 4, 4, None, occupancy='g', march=0.75, resample=64)
    assert seen == [(0.75, 64)]
