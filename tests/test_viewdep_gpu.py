"""GPU: the view-dependent field (csrc/viewdep.hip, hashgrid.ViewDependentField).  The four glue kernels against
tests/sh_rule.py bit for bit, their refusals, the zero start, the density's independence of the direction, the whole chain against float64
autograd, training on views only a direction input can fit, the bake's two colours and the refusals by name."""
import ctypes as C
import numpy as np
import pytest
import torch

import hashgrid_rule as HG
import march_rule as mr
import sh_rule as SH
import test_occupancy_cpu as OC
import test_occupancy_mesh_cpu as OM
import test_occupancy_gpu as OG
from test_engine_ops_gpu import Out, E_ARG

pytestmark = pytest.mark.gpu
f32 = np.float32
NEAR, FAR = 0.5, 2.5
N_CASES = [1, 63, 64, 65, 300, 4097]
WIDTH_CASES = [(1, 1), (16, 4), (30, 3), (32, 4), (48, 4), (55, 3), (63, 1)]        # (E, deg): quad and scalar rows, the full width 64
SMALL = dict(n_levels=4, n_features=2, log2_table=8, base_res=2, max_res=16)       # _small_field of test_hashgrid_gpu.py


def _lib():
    from contexture_nerf_amd import _lib as L
    return L, L.load()


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _ray_ids(rng, n, R):
    """unsorted, with repeats, and with -1 and R among the entries"""
    ids = rng.integers(0, R, n).astype(np.int32)
    if n > 2:
        ids[rng.integers(0, n)] = -1
        ids[(int(np.argmin(ids)) + 1) % n] = R
    return ids


def _input_fwd(dev, emb_t, rd_t, id_t, n, R, E, deg):
    L, lib = _lib()
    out = Out(dev, (n, E + deg * deg), torch.float32)
    L.check(lib.ctx_viewdep_input_fwd(L.ptr(emb_t), L.ptr(rd_t), L.ptr(id_t), n, R, E, deg, L.ptr(out.t), L.stream()))
    return out


# ---- 5. the input row ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,deg", WIDTH_CASES)
def test_input_fwd_equals_the_rule(dev, E, deg):
    for n in N_CASES:
        for R in (1, 7):
            rng = np.random.default_rng(1000 * n + 10 * E + R)
            emb = rng.standard_normal((n, E)).astype(f32)
            rays_d = SH.mixed_directions(R, seed=n + R, zero=R > 1)
            ids = _ray_ids(rng, n, R)
            want = SH.input_np(emb, rays_d, ids, deg)
            emb_t, rd_t, id_t = _t(dev, emb), _t(dev, rays_d), _t(dev, ids)
            first = _input_fwd(dev, emb_t, rd_t, id_t, n, R, E, deg)
            got = first.cpu(f"input_fwd n={n} E={E} deg={deg} R={R}")
            assert bool(torch.isfinite(got).all()), (n, R)
            assert np.array_equal(got.numpy(), want), (n, R, int((got.numpy() != want).sum()))
            again = _input_fwd(dev, emb_t, rd_t, id_t, n, R, E, deg).cpu("input_fwd again")
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                other = _input_fwd(dev, emb_t, rd_t, id_t, n, R, E, deg)
            side.synchronize()
            assert torch.equal(again, got) and torch.equal(other.cpu("input_fwd side stream"), got)
    # emb as a view 4 bytes off the 16-byte grid: the scalar rows, the same bits
    assert (n, R) == (4097, 7)                                              # the last case's inputs and expectation
    buf = torch.zeros(n * E + 1, device=dev)
    off = buf[1:].view(n, E)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    off.copy_(emb_t)
    got = _input_fwd(dev, off, rd_t, id_t, n, R, E, deg).cpu("input_fwd off the 16-byte grid")
    assert np.array_equal(got.numpy(), want)


# ---- 6. the slices and the add -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,deg", WIDTH_CASES)
def test_input_bwd_equals_the_slice(dev, E, deg):
    L, lib = _lib()
    for n in N_CASES:
        g_inp = np.random.default_rng(n + E).standard_normal((n, E + deg * deg)).astype(f32)
        g = _t(dev, g_inp)
        out = Out(dev, (n, E), torch.float32)
        L.check(lib.ctx_viewdep_input_bwd(L.ptr(g), n, E, deg, L.ptr(out.t), L.stream()))
        got = out.cpu(f"input_bwd n={n} E={E} deg={deg}").numpy()
        assert np.array_equal(got, SH.input_bwd_np(g_inp, E)), n
    buf = torch.zeros(g.numel() + 1, device=dev)
    off = buf[1:].view_as(g)
    off.copy_(g)
    out = Out(dev, (n, E), torch.float32)
    L.check(lib.ctx_viewdep_input_bwd(L.ptr(off), n, E, deg, L.ptr(out.t), L.stream()))
    assert np.array_equal(out.cpu("input_bwd off the 16-byte grid").numpy(), SH.input_bwd_np(g_inp, E))


def test_raw_fwd_and_bwd_equal_the_rule(dev):
    L, lib = _lib()
    for n in N_CASES:
        rng = np.random.default_rng(n)
        base = (rng.standard_normal((n, 4)) * 3).astype(f32)
        res = (rng.standard_normal((n, 3)) * rng.choice([1e-6, 1.0, 100.0], (n, 1))).astype(f32)
        for shift in (0, 1):                                               # 1: every tensor 4 bytes off the 16-byte grid, the scalar rows
            def place(a):
                buf = torch.zeros(a.size + shift, device=dev)
                v = buf[shift:].view(a.shape)
                v.copy_(_t(dev, a))
                return v
            b, r = place(base), place(res)
            out = Out(dev, (n, 4), torch.float32)
            L.check(lib.ctx_viewdep_raw_fwd(L.ptr(b), L.ptr(r), n, L.ptr(out.t), L.stream()))
            got = out.cpu(f"raw_fwd n={n}").numpy()
            assert np.isfinite(got).all() and np.array_equal(got, SH.raw_np(base, res)), (n, shift)
            g = Out(dev, (n, 3), torch.float32)
            L.check(lib.ctx_viewdep_raw_bwd(L.ptr(b), n, L.ptr(g.t), L.stream()))
            assert np.array_equal(g.cpu(f"raw_bwd n={n}").numpy(), SH.raw_bwd_np(base)), (n, shift)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
def test_abi_refusals_leave_the_outputs_untouched(dev):
    L, lib = _lib()
    n, R, E, deg = 8, 3, 16, 4
    emb, rd, ids = torch.zeros(n, 64, device=dev), torch.ones(R, 3, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    g4 = torch.zeros(n, 4, device=dev)
    inp, g_emb = Out(dev, (n, 80), torch.float32, 0xA5), Out(dev, (n, 64), torch.float32, 0xA5)
    raw, g_res = Out(dev, (n, 4), torch.float32, 0xA5), Out(dev, (n, 3), torch.float32, 0xA5)
    s = L.stream()
    fwd = [L.ptr(emb), L.ptr(rd), L.ptr(ids), n, R, E, deg, L.ptr(inp.t), s]
    bwd = [L.ptr(emb), n, E, deg, L.ptr(g_emb.t), s]
    rf = [L.ptr(g4), L.ptr(g4), n, L.ptr(raw.t), s]
    rb = [L.ptr(g4), n, L.ptr(g_res.t), s]

    def refused(fn, good, change):
        a = list(good)
        for k, v in change.items():
            a[k] = v
        rc = fn(*a)
        assert rc == E_ARG and b"viewdep" in lib.ctx_last_error(), (fn.__name__, change, rc, lib.ctx_last_error())

    for ch in ({6: 0}, {6: 5}, {5: 49, 6: 4}, {5: 0}, {3: 0}, {3: -1}, {3: 1 << 31}, {4: 0}, {0: None}, {1: None}, {2: None}, {7: None}):
        refused(lib.ctx_viewdep_input_fwd, fwd, ch)
    for ch in ({3: 0}, {3: 5}, {2: 49, 3: 4}, {1: 0}, {0: None}, {4: None}):
        refused(lib.ctx_viewdep_input_bwd, bwd, ch)
    for ch in ({2: 0}, {2: 1 << 31}, {0: None}, {1: None}, {3: None}):
        refused(lib.ctx_viewdep_raw_fwd, rf, ch)
    for ch in ({1: 0}, {0: None}, {2: None}):
        refused(lib.ctx_viewdep_raw_bwd, rb, ch)
    for o, what in ((inp, "input_fwd"), (g_emb, "input_bwd"), (raw, "raw_fwd"), (g_res, "raw_bwd")):
        o.untouched(what)


# ---- the fields ----------------------------------------------------------------------------------------------------------------------
def _field_pair(dev, seed=0, **kw):
    """A ViewDependentField and a HashGridField with the same table and base parameters."""
    from contexture_nerf_amd.hashgrid import HashGridField, ViewDependentField
    torch.manual_seed(seed)
    plain = HashGridField(-1.0, 1.0, **SMALL).to(dev)
    with torch.no_grad():
        plain.encoding.table.copy_(torch.randn(plain.encoding.table.shape, generator=torch.Generator().manual_seed(seed + 1)) * 0.5)
        plain.mlp.output_linear.bias[3] = 1.0
    field = ViewDependentField(-1.0, 1.0, **SMALL, **kw).to(dev)
    with torch.no_grad():
        field.encoding.table.copy_(plain.encoding.table)
        for a, b in zip(field.mlp._params(), plain.mlp._params()):
            a.copy_(b)
    return field, plain


def _wake_direction_net(field, seed=3, scale=0.3):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        out = field.dir_mlp.output_linear
        out.weight.copy_(torch.randn(out.weight.shape, generator=g) * scale)
        out.bias.copy_(torch.randn(out.bias.shape, generator=g) * scale)


def _ball_grid(dev, G=8):
    from contexture_nerf_amd import volume_render as vr
    return vr.OccupancyGrid.from_mask(torch.from_numpy(OM.ball_mask(G, 0.6)).to(dev), -1.0, 1.0)


def _shell_grid(dev, G=16):
    from contexture_nerf_amd import volume_render as vr
    v, f = OM.icosphere(2, 0.6)
    return vr.OccupancyGrid.from_mesh(*OG._dev(dev, v, f), G, -1.0, 1.0, dilate=1)


FIRST_POSE = [[1, 0, 0, 0.0], [0, 1, 0, 0.0], [0, 0, 1, 1.5]]                       # _teacher_views' first pose


def _points_and_rays(dev, n=300, R=7, seed=11):
    rng = np.random.default_rng(seed)
    pts = _t(dev, rng.uniform(-1, 1, (n, 3)).astype(f32))
    rays_d = _t(dev, SH.mixed_directions(R, seed=seed, zero=False))
    ids = _t(dev, rng.integers(0, R, n).astype(np.int32))
    return pts, rays_d, ids


# ---- 8. the zero start ---------------------------------------------------------------------------------------------------------------
def test_zero_start_is_the_plain_field(dev):
    from contexture_nerf_amd import volume_render as vr
    field, plain = _field_pair(dev)
    pts, rays_d, ids = _points_and_rays(dev)
    with torch.no_grad():
        raw, res = field.forward_dirs(pts, rays_d, ids, return_residual=True)
        assert raw.grad_fn is None and field.mlp._saved_pool is None and field.dir_mlp._saved_pool is None      # no grad: nothing kept
        assert torch.equal(raw, plain.forward_pts(pts)) and torch.equal(raw, field.forward_pts(pts))
        assert tuple(res.shape) == (300, 3) and not bool(res.any())
    assert torch.equal(field.forward_dirs(pts, rays_d, ids).detach(), raw)          # with a graph: the same bits
    e_raw, e_res = field.forward_dirs(pts[:0], rays_d, ids[:0], return_residual=True)
    assert tuple(e_raw.shape) == (0, 4) and tuple(e_res.shape) == (0, 3)
    K, c2w, grid = vr.pinhole(16, 16), torch.tensor(FIRST_POSE, dtype=torch.float32, device=dev), _ball_grid(dev)
    step = float(grid.h[0]) / 2
    for resample in (0, 8):
        a = vr.render_image(field, 16, 16, K, c2w, NEAR, FAR, 0, occupancy=grid, march=step, resample=resample)
        b = vr.render_image(plain, 16, 16, K, c2w, NEAR, FAR, 0, occupancy=grid, march=step, resample=resample)
        assert float(a['acc'].max()) > 0
        assert all(torch.equal(a[k], b[k]) for k in ('rgb', 'acc', 'depth'))


# ---- 9. the density does not see the direction ---------------------------------------------------------------------------------------
def test_density_does_not_see_the_direction(dev):
    from contexture_nerf_amd import volume_render as vr
    field, plain = _field_pair(dev)
    _wake_direction_net(field)
    pts, rays_d, ids = _points_and_rays(dev)
    other = _t(dev, SH.mixed_directions(7, seed=99, zero=False))
    with torch.no_grad():
        a, b = field.forward_dirs(pts, rays_d, ids), field.forward_dirs(pts, other, ids)
        base = plain.forward_pts(pts)
        assert torch.equal(a[:, 3], b[:, 3]) and torch.equal(a[:, 3], base[:, 3])
        assert bool((a[:, :3] != b[:, :3]).any(dim=1).all())
        assert torch.equal(field.forward_pts(pts), base)
    grids = [_ball_grid(dev, 8), _ball_grid(dev, 8)]
    for g, f_ in zip(grids, (field, plain)):
        g.update(f_, 0.01, generator=torch.Generator(device=dev).manual_seed(4))
    assert torch.equal(grids[0].dens, grids[1].dens) and torch.equal(grids[0].cells, grids[1].cells) and bool(grids[0].dens.any())
    K, c2w, grid = vr.pinhole(16, 16), torch.tensor(FIRST_POSE, dtype=torch.float32, device=dev), _ball_grid(dev)
    n_a = vr.render_normals(field, 16, 16, K, c2w, NEAR, FAR, grid, float(grid.h[0]) / 2)
    n_b = vr.render_normals(plain, 16, 16, K, c2w, NEAR, FAR, grid, float(grid.h[0]) / 2)
    assert all(torch.equal(n_a[k], n_b[k]) for k in n_a) and bool(n_a['normal'].any())


# ---- 10. the whole chain -------------------------------------------------------------------------------------------------------------
def _field_tensors(field):
    return [field.encoding.table] + field.mlp._params() + field.dir_mlp._params()


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def _chain_reference(field, t32, passes, rd, target, dtype):
    """The gradients of img2mse(rgb, target) + 0.1 acc.mean() on the last pass (+ img2mse on an earlier, coarse one) + 0.05 mean(res^2) over
    the samples of every pass, by CPU autograd in `dtype` through the rule's cells, a torch MLP twice, the float64 SH rule as a constant
    and the compositing restatement.  passes: (pts, t, dt, ray_off, ray_id)."""
    enc = field.encoding
    ts = [x.clone().to(dtype).requires_grad_(True) for x in t32]
    rd_t, target = rd.to(dtype), target.to(dtype)
    loss, sq, count = 0., 0., 0
    for k, (pts, t, dt, ray_off, ray_id) in enumerate(passes):
        emb = HG.forward_torch(pts.numpy(), ts[0], enc.lo, enc.hi, enc.res, enc.log2_table, dtype=dtype)
        base = HG.mlp_torch(emb, ts[1:7], 0)
        sh = torch.from_numpy(SH.input_np(np.zeros((pts.shape[0], 0)), rd.numpy(), ray_id.numpy(), field.sh_degree, sh=SH.sh_f64)).to(dtype)
        res = HG.mlp_torch(torch.cat([emb, sh], 1), ts[7:13], 0)
        raw = torch.cat([base[:, :3] + res, base[:, 3:]], 1)
        rgb, _, acc, _, _ = mr.restate_packed(raw, t.to(dtype), dt.to(dtype), rd_t, ray_off)
        loss = loss + ((rgb - target) ** 2).mean()
        if k == len(passes) - 1:
            loss = loss + 0.1 * acc.mean()
        sq, count = sq + (res * res).sum(), count + res.numel()
    loss = loss + 0.05 * sq / count
    loss.backward()
    return [x.grad for x in ts]


@pytest.mark.parametrize("mode", ["marched", "resampled"])
def test_whole_chain_gradients_vs_float64(dev, mode):
    """forward_dirs with a non-zero direction net -> compositing -> loss: the gradients of the table and the twelve MLP tensors against
    float64 CPU autograd, at the criterion of test_hashgrid_gpu.test_whole_chain_gradients_vs_float64: per tensor the relative L2 distance
    may be four times that of the float32 CPU run of the same restatement and never has to be below 2e-4.  The sample lists are taken
    from the HIP run."""
    from contexture_nerf_amd import run_nerf_helpers as rnh
    field, _ = _field_pair(dev)
    _wake_direction_net(field)
    grid = _ball_grid(dev, 8)
    R = 96
    ro, rd, _ = OG._dev(dev, *OC.random_rays(np.random.default_rng(5), R, 4, spread=0.5))
    target = torch.rand(R, 3, generator=torch.Generator().manual_seed(2))
    step = float(grid.h[0]) / 2
    out, ex = rnh.render_rays(field, ro, rd, NEAR, FAR, 0, occupancy=grid, march=step, resample=8 if mode == "resampled" else 0,
                              return_extras=True)
    assert ex['t'].numel() > R and tuple(ex['residual'].shape) == (ex['t'].numel(), 3)
    passes = [tuple(ex[k].cpu() for k in ('pts', 't', 'dt', 'ray_off', 'ray_id'))]
    loss = rnh.img2mse(out[0], target.to(dev)) + 0.1 * out[2].mean()
    parts = [ex['residual']]
    if mode == "resampled":
        loss = loss + rnh.img2mse(ex['rgb0'], target.to(dev))
        passes.insert(0, tuple(ex[k].cpu() for k in ('pts0', 't0', 'dt0', 'ray_off0', 'ray_id0')))
        parts.insert(0, ex['residual0'])
    loss = loss + 0.05 * sum((p * p).sum() for p in parts) / sum(p.numel() for p in parts)
    loss.backward()
    tensors = _field_tensors(field)
    assert len(tensors) == 13
    got = [x.grad.cpu() for x in tensors]
    t32 = [x.detach().cpu() for x in tensors]
    want = _chain_reference(field, t32, passes, rd.cpu(), target, torch.float64)
    c32 = _chain_reference(field, t32, passes, rd.cpu(), target, torch.float32)
    rows = [(_rel(a, w), _rel(c, w)) for a, w, c in zip(got, want, c32)]
    print(f"view-dependent chain ({mode}): relative L2, table {rows[0][0]:.3e} (float32 CPU {rows[0][1]:.3e}), base MLP worst "
          f"{max(r[0] for r in rows[1:7]):.3e} (float32 CPU {max(r[1] for r in rows[1:7]):.3e}), direction MLP worst "
          f"{max(r[0] for r in rows[7:]):.3e} (float32 CPU {max(r[1] for r in rows[7:]):.3e})")
    for i, g in enumerate(got):
        assert bool(g.any()), i
    for i, (a, c) in enumerate(rows):
        assert a <= max(4 * c, 2e-4), (i, a, c)


# ---- 11. training on something only a direction input can fit ------------------------------------------------------------------------
def _direction_views(dev):
    """Four 16 x 16 views around the sphere of radius 0.6: a pixel whose ray hits it shows 0.5 + 0.4 * (its unit ray direction), every
    other pixel is white.  The same surface point has a different colour in every view that sees it."""
    from contexture_nerf_amd import run_nerf_helpers as rnh, volume_render as vr
    K = vr.pinhole(16, 16)
    first = np.asarray(FIRST_POSE, np.float64)
    c2ws = []
    for a in (0.0, np.pi / 2, np.pi, 3 * np.pi / 2):
        ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        c2ws.append(ry @ first)
    c2ws = torch.tensor(np.stack(c2ws), dtype=torch.float32, device=dev)
    images = []
    for v in range(4):
        ro, rd = rnh.get_rays(16, 16, K, c2ws[v])
        d = rd / rd.norm(dim=-1, keepdim=True)
        b = (ro * d).sum(-1)
        hit = (b * b - ((ro * ro).sum(-1) - 0.36) >= 0) & (b < 0)
        images.append(torch.where(hit[..., None], 0.5 + 0.4 * d, torch.ones_like(d)))
    images = torch.stack(images)
    assert 0.1 < float((images != 1).any(-1).float().mean()) < 0.9
    return images, c2ws, K


VIEW_FIT = dict(n_levels=8, n_features=2, log2_table=12, base_res=4, max_res=64)
# Measured on an MI355X: the new field's mean loss over the last five of the 60 iterations is r times the plain field's
# (0.000722 against 0.016577).  The gate is sqrt(r) = 0.209, the geometric midpoint between the measurement and "no better than the parent";
# the run repeats bit for bit, so the margin only has to absorb a change of compiler or runtime.
MEASURED_RATIO = 0.0436


def _fit(dev, cls, views, iters=60, optimizer='torch', **kw):
    from contexture_nerf_amd import volume_render as vr
    images, c2ws, K = views
    grid = _shell_grid(dev)
    torch.manual_seed(9)
    student = cls.from_grid(grid, **VIEW_FIT, **kw).to(dev)
    hist = vr.fit_views(student, images, c2ws, K, NEAR, FAR, iters=iters, rays_per_iter=128, lr=1e-2, seed=0, white_bkgd=True, occupancy=grid,
                        occupancy_every=0, march=float(grid.h[0]) / 2, optimizer=optimizer)
    return hist, student


def test_training_fits_what_only_a_direction_input_can(dev):
    from contexture_nerf_amd.hashgrid import HashGridField, ViewDependentField
    views = _direction_views(dev)
    plain, _ = _fit(dev, HashGridField, views)
    runs = [_fit(dev, ViewDependentField, views, sh_degree=4) for _ in range(2)]
    new = runs[0][0]
    assert len(new) == 60 and len(plain) == 60 and all(np.isfinite(v) for v in new + plain)
    r = float(np.mean(new[-5:]) / np.mean(plain[-5:]))
    print(f"direction-coloured sphere, last five of 60: ViewDependentField {np.mean(new[-5:]):.6f}, HashGridField {np.mean(plain[-5:]):.6f}, "
          f"ratio r = {r:.4f}")
    assert np.mean(new[-5:]) < np.mean(plain[-5:])
    assert r <= np.sqrt(MEASURED_RATIO), r
    assert runs[0][0] == runs[1][0]
    assert all(torch.equal(a, b) for a, b in zip(_field_tensors(runs[0][1]), _field_tensors(runs[1][1])))
    fused = [_fit(dev, ViewDependentField, views, iters=5, optimizer='fused', sh_degree=4) for _ in range(2)]
    assert len(fused[0][0]) == 5 and all(np.isfinite(v) for v in fused[0][0]) and fused[0][0] == fused[1][0]
    assert all(torch.equal(a, b) for a, b in zip(_field_tensors(fused[0][1]), _field_tensors(fused[1][1])))


def test_view_residual_term(dev):
    """train_step(view_residual=): the dict's 'view_residual' is the mean of res^2 over the samples of both passes, and the loss holds it."""
    from contexture_nerf_amd import run_nerf_helpers as rnh, volume_render as vr
    field, _ = _field_pair(dev)
    _wake_direction_net(field)
    grid = _ball_grid(dev, 8)
    ro, rd, _ = OG._dev(dev, *OC.random_rays(np.random.default_rng(5), 32, 4, spread=0.5))
    target = torch.rand(32, 3, device=dev)
    step = float(grid.h[0]) / 2
    with torch.no_grad():
        _, ex = rnh.render_rays(field, ro, rd, NEAR, FAR, 0, occupancy=grid, march=step, resample=4, perturb=0., return_extras=True)
        want = torch.cat([ex['residual0'], ex['residual']]).square().mean()
    opt = torch.optim.Adam(field.parameters(), lr=0.0)
    a = vr.train_step(field, opt, ro, rd, target, NEAR, FAR, 0, perturb=0., occupancy=grid, march=step, resample=4, view_residual=0.5)
    b = vr.train_step(field, opt, ro, rd, target, NEAR, FAR, 0, perturb=0., occupancy=grid, march=step, resample=4)
    assert float(want) > 0 and 'view_residual' not in b
    assert abs(float(a['view_residual']) - float(want)) <= 1e-5 * float(want)
    assert abs(float(a['loss']) - (float(b['loss']) + 0.5 * float(want))) <= 1e-5 * float(a['loss'])


# ---- 12. the bake --------------------------------------------------------------------------------------------------------------------
def test_bake_view_and_diffuse(dev):
    """The icosphere with an atlas of T = 64 whose texels each name a point of a face (supersample 1 reads nothing else of the map)."""
    from contexture_nerf_amd import volume_render as vr
    T = 64
    v, f = OM.icosphere(2, 0.6)
    F = f.shape[0]
    rng = np.random.default_rng(6)
    tface = np.full(T * T, -1, np.int64)
    tface[:10 * F] = np.arange(10 * F) % F
    tbary = np.zeros((T * T, 3), f32)
    tbary[:10 * F] = rng.dirichlet([2, 2, 2], 10 * F).astype(f32)
    face_uv = rng.random((F, 3, 2)).astype(f32)
    mesh = [_t(dev, v.astype(f32)), _t(dev, f.astype(np.int64)), _t(dev, face_uv), _t(dev, tface.reshape(T, T)), _t(dev, tbary.reshape(T, T, 3))]
    grid = _shell_grid(dev)
    field, plain = _field_pair(dev)
    with torch.no_grad():
        for f_ in (field, plain):
            f_.mlp.output_linear.bias[3] = 60.0                            # opaque inside the shell
    want = vr.bake_atlas(plain, *mesh, grid, supersample=1)
    covered = want[3] > 0
    assert int(covered.sum()) > 5 * F
    for colour in ('view', 'diffuse'):
        assert torch.equal(vr.bake_atlas(field, *mesh, grid, supersample=1, colour=colour), want)
        assert torch.equal(vr.bake_atlas(plain, *mesh, grid, supersample=1, colour=colour), want)
    with torch.no_grad():
        field.dir_mlp.output_linear.bias.fill_(2.0)
    assert torch.equal(vr.bake_atlas(field, *mesh, grid, supersample=1, colour='diffuse'), want)
    view = vr.bake_atlas(field, *mesh, grid, supersample=1, colour='view')
    assert torch.equal(view[3], want[3]) and not torch.equal(view, want)
    assert bool((view[:3, covered] > want[:3, covered]).all())


# ---- 13. refusals by name ------------------------------------------------------------------------------------------------------------
def test_refusals_by_name(dev):
    from contexture_nerf_amd import _lib as L, run_nerf_helpers as rnh, volume_render as vr
    from contexture_nerf_amd.hashgrid import ViewDependentField
    field, plain = _field_pair(dev)
    grid = _ball_grid(dev, 8)
    ro, rd, _ = OG._dev(dev, *OC.random_rays(np.random.default_rng(5), 8, 4))
    target = torch.rand(8, 3, device=dev)
    before = [p.detach().clone() for p in field.parameters()]
    opt = torch.optim.Adam(field.parameters(), lr=1e-2)
    with pytest.raises(L.CtxError, match="view-dependent field.*march="):
        rnh.render_rays(field, ro, rd, NEAR, FAR, 16)
    with pytest.raises(L.CtxError, match="view-dependent field.*march="):
        rnh.render_rays(field, ro, rd, NEAR, FAR, 16, occupancy=grid)
    with pytest.raises(L.CtxError, match="train_step.*view-dependent field.*march="):
        vr.train_step(field, opt, ro, rd, target, NEAR, FAR, 16)
    with pytest.raises(L.CtxError, match="view_residual"):
        vr.train_step(plain, torch.optim.Adam(plain.parameters(), lr=1e-2), ro, rd, target, NEAR, FAR, 0, occupancy=grid, march=0.125,
                      view_residual=0.1)
    assert all(torch.equal(a, b) for a, b in zip(before, field.parameters())) and all(p.grad is None for p in field.parameters())
    with pytest.raises(L.CtxError, match=r"60 \+ 9 = 69"):
        ViewDependentField(-1.0, 1.0, n_levels=15, n_features=4, log2_table=4, sh_degree=3)
    pts, rays_d, ids = _points_and_rays(dev, n=16)
    with pytest.raises(L.CtxError, match="rays_d"):
        field.forward_dirs(pts, rays_d.clone().requires_grad_(True), ids)
    with pytest.raises(L.CtxError, match="ray_id.*int32"):
        field.forward_dirs(pts, rays_d, ids.long())
    with pytest.raises(L.CtxError, match="rays_d.*float32"):
        field.forward_dirs(pts, rays_d.double(), ids)
    with pytest.raises(L.CtxError, match="ray_id"):
        field.forward_dirs(pts, rays_d, ids[:-1])
    with pytest.raises(L.CtxError, match="device tensor"):
        field.forward_dirs(pts, rays_d.cpu(), ids)
    with pytest.raises(L.CtxError, match="colour='specular'"):
        vr.bake_atlas(field, None, None, None, torch.zeros(4, 4, dtype=torch.int64, device=dev), None, grid, colour='specular')


def test_field_optimizer_groups(dev):
    """One table group and twelve MLP tensors, with either optimizer; a fused step moves all thirteen."""
    from contexture_nerf_amd import volume_render as vr
    field, _ = _field_pair(dev)
    opt = vr.field_optimizer(field, 1e-2, 'torch', table_lr=1e-1)
    assert [len(g['params']) for g in opt.param_groups] == [1, 12] and opt.param_groups[0]['params'][0] is field.encoding.table
    fused = vr.field_optimizer(field, 1e-2, 'fused')
    try:
        assert [len(g['params']) for g in fused.param_groups] == [1, 12]
    finally:
        fused.release()
