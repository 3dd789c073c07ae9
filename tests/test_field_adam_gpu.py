"""GPU: the field optimizer (csrc/adam.hip, contexture_nerf_amd/optim.py) against its rule (tests/adam_rule.py), the
table's step from the integer sums against the rule applied to stage 4's g_table, deferred against not deferred, and the caches."""
import ctypes as C
import functools
import numpy as np
import pytest
import torch

import adam_rule as AR
import hashgrid_rule as HG
import hashtex_rule as HT
import test_field_adam_cpu as AC

pytestmark = pytest.mark.gpu
f32 = np.float32
BETAS = AC.BETAS
LO, HI = HG.BOX_LO, HG.BOX_HI
COUNTS = [1, 63, 64, 65, 255, 256, 257, 1000, 4099]
# element offsets of (p, m, v, g) from a 16-byte boundary: the four on one offset take the 16-byte path behind a head, mixed ones the 4-byte path
OFFSETS = [(0, 0, 0, 0), (1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3), (0, 1, 2, 3), (0, 0, 0, 2)]


def make_case(count, seed):
    """p, m, v >= 0 and a gradient that holds +-0, subnormals, 1e30, inf and NaN where the count leaves room."""
    rng = np.random.default_rng(seed)
    p, m = rng.standard_normal(count).astype(f32), (rng.standard_normal(count) * 1e-3).astype(f32)
    v = (rng.standard_normal(count) ** 2 * 1e-6).astype(f32)
    g = (rng.standard_normal(count) * 3e-3).astype(f32)
    special = [0.0, -0.0, 1e-40, -3e-42, 1e30, np.inf, -np.inf, np.nan]
    pos = rng.permutation(count)
    for k, s in enumerate(special * 3):
        if k < count // 2:
            g[pos[k]] = f32(s)
    if count >= 16:
        g[8:16] = 0.0                                                 # two whole 16-byte groups of zeros somewhere
    return p, m, v, g


def on_device(dev, a, off):
    """A copy of a on the device that starts `off` elements behind a 16-byte boundary."""
    buf = torch.zeros(a.size + 8, device=dev)
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + a.size]
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4 * off and t.is_contiguous()
    return t


def same(a, b):
    """Equal values, NaN where NaN is wanted, and the sign of every zero."""
    ok = ~np.isnan(b)
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a)[ok], np.signbit(b)[ok])


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("t,eps", [(1, 1e-8), (1000, 1e-15), (1, 1e-15), (1000, 1e-8)])
def test_adam_multi_equals_the_rule(dev, sparse, t, eps):
    from contexture_nerf_amd import optim
    for count in COUNTS:
        case = make_case(count, seed=count)
        want = AR.adam_step(*case, 1e-2, BETAS, eps, t, sparse=sparse)
        for offs in OFFSETS:
            p, m, v, g = (on_device(dev, a, o) for a, o in zip(case, offs))
            optim.adam_multi([p], [m], [v], [g], 1e-2, BETAS, eps, t, sparse)
            for name, got, w in zip("pmv", (p, m, v), want):
                assert same(got.cpu().numpy(), w), (name, count, offs)
            assert np.array_equal(g.cpu().numpy(), case[3], equal_nan=True)


def test_sixteen_tensors_in_one_launch_and_seventeen_through_field_adam(dev):
    from contexture_nerf_amd import _lib as L, optim
    counts = COUNTS + [2, 5, 17, 4096, 4097, 8195, 20000]
    assert len(counts) == 16
    cases = [make_case(c, seed=100 + k) for k, c in enumerate(counts)]
    for sparse in (False, True):
        tensors = [[on_device(dev, a, (k + j) % 4 if k % 3 == 2 else k % 4) for j, a in enumerate(case)] for k, case in enumerate(cases)]
        optim.adam_multi(*[[ts[j] for ts in tensors] for j in range(4)], 5e-4, BETAS, 1e-8, 7, sparse)
        for k, (case, ts) in enumerate(zip(cases, tensors)):
            want = AR.adam_step(*case, 5e-4, BETAS, 1e-8, 7, sparse=sparse)
            assert all(same(got.cpu().numpy(), w) for got, w in zip(ts, want)), (k, counts[k], sparse)
    with pytest.raises(L.CtxError, match="n_tensors"):
        optim.adam_multi(*[[ts[j] for ts in tensors] + [tensors[0][j]] for j in range(4)], 5e-4, BETAS, 1e-8, 7, False)
    # 17 parameters: two launches; two steps, the second with moments and t = 2
    counts17 = counts + [300]
    cases = [make_case(c, seed=200 + k) for k, c in enumerate(counts17)]
    params = [torch.nn.Parameter(torch.from_numpy(c[0]).to(dev)) for c in cases]
    opt = optim.FieldAdam(params, lr=1e-2, betas=BETAS, eps=1e-15)
    want = [(c[0], np.zeros_like(c[0]), np.zeros_like(c[0])) for c in cases]
    for t in (1, 2):
        versions = [p._version for p in params]
        for p, c in zip(params, cases):
            p.grad = torch.from_numpy(c[3] * f32(t)).to(dev)
        opt.step()
        want = [AR.adam_step(*w, c[3] * f32(t), 1e-2, BETAS, 1e-15, t) for w, c in zip(want, cases)]
        assert all(p._version > v0 for p, v0 in zip(params, versions))
    for p, w in zip(params, want):
        st = opt.state[p]
        assert float(st['step']) == 2
        assert same(p.detach().cpu().numpy(), w[0]) and same(st['exp_avg'].cpu().numpy(), w[1]) and same(st['exp_avg_sq'].cpu().numpy(), w[2])
    # refusals that need the device
    with pytest.raises(L.CtxError, match="float32"):
        optim.FieldAdam([torch.nn.Parameter(torch.zeros(4, device=dev, dtype=torch.float64))])
    with pytest.raises(L.CtxError, match="contiguous"):
        optim.FieldAdam([torch.nn.Parameter(torch.zeros(4, 4, device=dev).t())])
    q = torch.nn.Parameter(torch.zeros(4, 4, device=dev))
    o2 = optim.FieldAdam([q])
    q.grad = torch.zeros(4, 4, device=dev).to_sparse()
    with pytest.raises(L.CtxError, match="sparse"):
        o2.step()


# ---- the table's step from the integer sums ---------------------------------------------------------------------------------------------
def _arr(a, ctype):
    a = np.ascontiguousarray(a, ctype)
    return a, a.ctypes.data_as(C.c_void_p)


class _Grid3D:
    corners = 8

    def __init__(self, dev, Lv, F, log2T):
        from contexture_nerf_amd import _lib as L
        self.dev, self.Lv, self.F, self.log2T = dev, Lv, F, log2T
        self.res = HG.resolutions(Lv, 2, 64)
        self.n = 300
        self.pts = torch.from_numpy(HG.case_points(self.n, LO, HI, self.res, seed=Lv)).to(dev)
        self.ws_bytes = L.load().ctx_hashgrid_bwd_ws_bytes(Lv, F, log2T)

    def bwd(self, g_emb, stages, ws, out):
        from contexture_nerf_amd import _lib as L
        (_r, rp), (_l, lp), (_h, hp) = _arr(self.res, np.int32), _arr(LO, f32), _arr(HI, f32)
        L.check(L.load().ctx_hashgrid_bwd(L.ptr(self.pts), self.n, L.ptr(g_emb), self.Lv, self.F, self.log2T, rp, lp, hp, stages, L.ptr(ws),
                                          L.ptr(out), L.stream()))


class _Grid2D(_Grid3D):
    corners = 4

    def __init__(self, dev, Lv, F, log2T):
        from contexture_nerf_amd import _lib as L
        self.dev, self.Lv, self.F, self.log2T = dev, Lv, F, log2T
        self.res = HT.resolutions(Lv, 2, 64)
        self.n = 300
        self.uv = torch.from_numpy(np.ascontiguousarray(HT.case_points(self.n, self.res, seed=5), f32)).to(dev)
        self.ws_bytes = L.load().ctx_hashtex_bwd_ws_bytes(Lv, F, log2T)

    def bwd(self, g_emb, stages, ws, out):
        from contexture_nerf_amd import _lib as L
        _r, rp = _arr(self.res, np.int32)
        L.check(L.load().ctx_hashtex_bwd(L.ptr(self.uv), None, self.n, 0, L.ptr(g_emb), self.Lv, self.F, self.log2T, rp, stages, L.ptr(ws),
                                         L.ptr(out), L.stream()))


def _table_adam(grid, state, ws, t, sparse, lr=1e-2, eps=1e-15):
    from contexture_nerf_amd import _lib as L, optim
    p, m, v = state
    L.check(L.load().ctx_table_adam(L.ptr(p), L.ptr(m), L.ptr(v), p.numel(), L.ptr(ws), grid.n, grid.corners,
                                    *optim.coefficients(lr, BETAS, eps, t), int(sparse), L.stream()))


@pytest.mark.parametrize("kind,Lv,F,log2T", [("3d", 4, 2, 6), ("3d", 3, 1, 5), ("3d", 2, 4, 4), ("2d", 4, 2, 6)])
def test_table_adam_equals_the_rule_on_stage_4(dev, kind, Lv, F, log2T):
    grid = (_Grid3D if kind == "3d" else _Grid2D)(dev, Lv, F, log2T)
    rng = np.random.default_rng(Lv * 10 + F)
    shape = (Lv, 1 << log2T, F)
    count = int(np.prod(shape))
    g_emb = torch.from_numpy((rng.standard_normal((grid.n, Lv * F)) * 3e-3).astype(f32)).to(dev)
    g_emb2 = torch.from_numpy(rng.standard_normal((grid.n, Lv * F)).astype(f32)).to(dev)
    p0, m0 = rng.standard_normal(count).astype(f32), (rng.standard_normal(count) * 1e-3).astype(f32)
    v0 = (rng.standard_normal(count) ** 2 * 1e-6).astype(f32)
    unused = torch.full(shape, 7.0, device=dev)

    def fresh(g):
        ws = torch.full((grid.ws_bytes,), 0xff, dtype=torch.uint8, device=dev)
        out = torch.full(shape, float('nan'), device=dev)
        grid.bwd(g, 7, ws, out)
        return out
    def garbage():
        """A workspace whose accumulator and control words, the bytes stage 1 clears, hold 0xff; the padding is zero."""
        ws = torch.zeros(grid.ws_bytes, dtype=torch.uint8, device=dev)
        ctl = (count * 8 + 255) // 256 * 256
        ws[:count * 8] = 0xff
        ws[ctl:ctl + 16] = 0xff
        return ws
    g_table = fresh(g_emb).cpu().numpy().reshape(-1)
    assert np.count_nonzero(g_table) > 0 and np.count_nonzero(g_table == 0) > 0 or log2T == 4
    for sparse in (True, False):
        ws = garbage()
        grid.bwd(g_emb, 3, ws, unused)                               # zero and accumulate: the sums stay in ws
        assert bool(ws.any()) and bool((unused == 7.0).all())
        state = [torch.from_numpy(a.copy()).to(dev) for a in (p0, m0, v0)]
        _table_adam(grid, state, ws, 3, sparse)
        want = AR.adam_step(p0, m0, v0, g_table, 1e-2, BETAS, 1e-15, 3, sparse=sparse)
        for name, got, w in zip("pmv", state, want):
            assert same(got.cpu().numpy(), w), (name, sparse)
        assert not bool(ws.any())                                    # the workspace is what stage 1 leaves
        # so stage 2 alone may follow, and its stage 4 equals a fresh backward
        out = torch.full(shape, float('nan'), device=dev)
        grid.bwd(g_emb2, 2, ws, unused)
        grid.bwd(g_emb2, 4, ws, out)
        assert torch.equal(out, fresh(g_emb2))
    # status 1: an all-zero g_emb moves nothing under sparse, and is the rule with g = 0 without it
    for sparse in (True, False):
        ws = torch.zeros(grid.ws_bytes, dtype=torch.uint8, device=dev)
        grid.bwd(torch.zeros_like(g_emb), 2, ws, unused)
        state = [torch.from_numpy(a.copy()).to(dev) for a in (p0, m0, v0)]
        _table_adam(grid, state, ws, 3, sparse)
        want = AR.adam_step(p0, m0, v0, np.zeros(count, f32), 1e-2, BETAS, 1e-15, 3, sparse=sparse)
        assert all(same(got.cpu().numpy(), w) for got, w in zip(state, want)) and not bool(ws.any())
        if sparse:
            assert all(np.array_equal(AR.bits(got.cpu().numpy()), AR.bits(a)) for got, a in zip(state, (p0, m0, v0)))
    # status 2: a NaN in g_emb turns the whole table into NaN, sparse or not
    bad = g_emb.clone()
    bad[17, 0] = float('nan')
    ws = torch.zeros(grid.ws_bytes, dtype=torch.uint8, device=dev)
    grid.bwd(bad, 2, ws, unused)
    state = [torch.from_numpy(a.copy()).to(dev) for a in (p0, m0, v0)]
    _table_adam(grid, state, ws, 3, True)
    assert all(bool(torch.isnan(s).all()) for s in state) and not bool(ws.any())


# ---- deferred equals not deferred -------------------------------------------------------------------------------------------------------
def _fit(dev, monkeypatch, deferred, resample, views):
    import test_hashgrid_gpu as TH
    from contexture_nerf_amd import volume_render as vr
    from contexture_nerf_amd.hashgrid import HashGridField
    images, c2ws, K = views
    made = []
    orig = vr.field_optimizer
    monkeypatch.setattr(vr, 'field_optimizer', lambda *a, **k: made.append(orig(*a, **k, deferred=deferred)) or made[-1])
    grid = TH._shell_grid(dev)
    torch.manual_seed(9)
    student = HashGridField.from_grid(grid, n_levels=8, n_features=2, log2_table=12, base_res=4, max_res=64).to(dev)
    hist = vr.fit_views(student, images, c2ws, K, TH.NEAR, TH.FAR, iters=8, rays_per_iter=128, lr=1e-3, seed=0, occupancy=grid,
                        occupancy_every=0, march=float(grid.h[0]) / 2, resample=resample, optimizer='fused', table_lr=1e-2)
    monkeypatch.setattr(vr, 'field_optimizer', orig)
    opt, = made
    assert not student.encoding._defer and student.encoding._pending is None           # released
    return hist, list(student.parameters()), [opt.state[p] for p in student.parameters()], opt


def _assert_same_run(a, b):
    assert a[0] == b[0] and len(a[0]) > 0 and all(np.isfinite(x) for x in a[0])
    assert len(a[1]) == len(b[1]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    for sa, sb in zip(a[2], b[2]):
        assert float(sa['step']) == float(sb['step']) > 0
        assert torch.equal(sa['exp_avg'], sb['exp_avg']) and torch.equal(sa['exp_avg_sq'], sb['exp_avg_sq'])


@pytest.mark.parametrize("resample", [0, 8])
def test_fit_views_deferred_equals_not_deferred(dev, monkeypatch, resample):
    """The toy scene of DESIGN 4j, 8 iterations of 128 marched rays; resample=8 calls the field twice per step: the flush path."""
    import test_raymarch_train_gpu as RT
    views = RT._teacher_views(dev)
    runs = [_fit(dev, monkeypatch, deferred, resample, views) for deferred in (True, False)]
    _assert_same_run(runs[0], runs[1])
    opt = runs[0][3]
    assert len(opt.param_groups) == 2 and opt.param_groups[0]['sparse'] and not opt.param_groups[1]['sparse']
    assert opt.param_groups[0]['lr'] == 1e-2 and opt.param_groups[1]['lr'] == 1e-3
    table = runs[0][1][0]
    assert table.grad is None or resample                                                # the table never had a float gradient
    moved = runs[0][2][0]['exp_avg_sq'] != 0
    assert 0 < int(moved.sum()) < moved.numel()                                          # sparse: untouched entries kept their zeros


def _texture_run(dev, deferred, texels, extra_backward=False):
    from contexture_nerf_amd import optim
    from contexture_nerf_amd.hashgrid import HashGridTexture
    torch.manual_seed(4)
    field = HashGridTexture(n_levels=4, n_features=2, log2_table=8, base_res=2, max_res=32).to(dev)
    target = torch.rand(1, 3, 16, 16, generator=torch.Generator().manual_seed(1)).to(dev)
    groups = [dict(params=[field.encoding.table], lr=1e-2, sparse=True), dict(params=list(field.mlp.parameters()), lr=1e-3)]
    opt = optim.FieldAdam(groups, betas=BETAS, eps=1e-15, encodings=[field.encoding] if deferred else ())
    hist = []
    try:
        for it in range(4):
            opt.zero_grad()
            if extra_backward and it == 1:
                (field.texture_map(16, texels)[0] * 3.0).sum().backward()                # a backward that no step consumes
                opt.zero_grad()
            tex, _raw = field.texture_map(16, texels)
            loss = ((tex - target) ** 2).sum()
            loss.backward()
            assert (field.encoding.table.grad is None) == deferred
            opt.step()
            hist.append(float(loss.detach()))
    finally:
        opt.release()
    params = list(field.parameters())
    return hist, params, [opt.state[p] for p in params], opt


@pytest.mark.parametrize("listed", [False, True])
def test_texture_map_deferred_equals_not_deferred(dev, listed):
    texels = torch.randperm(256, generator=torch.Generator().manual_seed(2))[:100].to(torch.int32).to(dev) if listed else None
    want = _texture_run(dev, False, texels)
    _assert_same_run(_texture_run(dev, True, texels), want)
    assert want[0][-1] < want[0][0]
    # a backward followed by zero_grad() and no step leaves the next steps unchanged, deferred or not
    _assert_same_run(_texture_run(dev, True, texels, extra_backward=True), want)
    _assert_same_run(_texture_run(dev, False, texels, extra_backward=True), want)


# ---- against torch on the device --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _float64_reference(lr, eps, scale):
    p0, grads = AC.fixed_problem(scale)
    return p0, grads, AC.torch_adam(p0, grads, lr, eps, torch.float64)


@pytest.mark.parametrize("lr,eps,scale", AC.CASES)
def test_field_adam_is_as_close_to_float64_as_torch_on_the_device(dev, lr, eps, scale):
    """Five steps, fixed gradients, no feedback through a field: the bound of the CPU test, float64 torch as the yardstick."""
    from contexture_nerf_amd import optim
    p0, grads, want = _float64_reference(lr, eps, scale)
    d_torch = AC.distance(AC.torch_adam(p0, grads, lr, eps, torch.float32, device=dev), p0, want)
    d_hip = AC.distance(AC.torch_adam(p0, grads, lr, eps, torch.float32, device=dev, make=optim.FieldAdam), p0, want)
    print(f"lr={lr} eps={eps} scale={scale}: FieldAdam {d_hip:.3e}, torch float32 on the device {d_torch:.3e}, ratio {d_hip / d_torch:.3f}")
    assert d_torch > 0 and d_hip <= 2 * d_torch


# ---- caches -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deferred", [False, True])
def test_step_invalidates_the_caches(dev, deferred):
    from contexture_nerf_amd import optim
    from contexture_nerf_amd.hashgrid import HashGridTexture
    torch.manual_seed(5)
    field = HashGridTexture(n_levels=4, n_features=2, log2_table=8, base_res=2, max_res=32).to(dev)
    with torch.no_grad():
        before = field.texture_map(16)[0].clone()
        assert field.texture_map(16)[0] is field.texture_map(16)[0]                      # cached
    blob = field.mlp._packed
    blob_version = field.mlp._packed_version
    assert blob is not None
    opt = optim.FieldAdam(field.parameters(), lr=1e-2, encodings=[field.encoding] if deferred else ())
    try:
        versions = [p._version for p in field.parameters()]
        (field.texture_map(16)[0] ** 2).sum().backward()
        opt.step()
        assert all(p._version > v for p, v in zip(field.parameters(), versions))         # every parameter was written and says so
    finally:
        opt.release()
    with torch.no_grad():
        after = field.texture_map(16)[0]
    assert not torch.equal(after, before)
    assert field.mlp._packed_version != blob_version                                     # the packed weights were rebuilt


# ---- defaults ---------------------------------------------------------------------------------------------------------------------------
def test_defaults_are_todays_and_table_lr_builds_two_groups(dev):
    import test_hashgrid_gpu as TH
    import test_raymarch_train_gpu as RT
    from contexture_nerf_amd import optim, volume_render as vr
    from contexture_nerf_amd.hashgrid import HashGridField
    from contexture_nerf_amd.run_nerf_helpers import NeRF2D
    images, c2ws, K = RT._teacher_views(dev)

    def run(**kw):
        grid = TH._shell_grid(dev)
        torch.manual_seed(9)
        student = HashGridField.from_grid(grid, n_levels=8, n_features=2, log2_table=12, base_res=4, max_res=64).to(dev)
        hist = vr.fit_views(student, images, c2ws, K, TH.NEAR, TH.FAR, iters=4, rays_per_iter=128, lr=1e-2, seed=0, occupancy=grid,
                            occupancy_every=0, march=float(grid.h[0]) / 2, **kw)
        return hist, list(student.parameters())
    a, b = run(), run(optimizer='torch', table_lr=None)
    assert a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    c = run(table_lr=1e-3)
    assert c[0][0] == a[0][0] and c[0] != a[0]                                           # another rate for the table: another run
    field = HashGridField.from_grid(TH._shell_grid(dev), n_levels=4, log2_table=8, base_res=4, max_res=32).to(dev)
    assert isinstance(vr.field_optimizer(field, 5e-4), torch.optim.Adam) and len(vr.field_optimizer(field, 5e-4).param_groups) == 1
    for name, cls in (('torch', torch.optim.Adam), ('fused', optim.FieldAdam)):
        opt = vr.field_optimizer(field, 5e-4, name, 1e-2)
        assert type(opt) is cls and len(opt.param_groups) == 2
        assert opt.param_groups[0]['params'][0] is field.encoding.table and len(opt.param_groups[0]['params']) == 1
        assert [g['lr'] for g in opt.param_groups] == [1e-2, 5e-4]
        assert sum(len(g['params']) for g in opt.param_groups) == len(list(field.parameters()))
        if name == 'fused':
            assert field.encoding._defer and opt.param_groups[0]['sparse'] and not opt.param_groups[1]['sparse']
            opt.release()
            assert not field.encoding._defer
    # a field without a table simply gets the HIP step
    mlp = NeRF2D(D=2, W=64, input_ch=63, output_ch=4, skips=[0]).to(dev)
    opt = vr.field_optimizer(mlp, 5e-4, 'fused')
    assert type(opt) is optim.FieldAdam and len(opt.param_groups) == 1 and not opt.param_groups[0]['sparse']
    with pytest.raises(Exception, match="optimizer"):
        vr.fit_views(mlp, images, c2ws, K, TH.NEAR, TH.FAR, iters=1, optimizer='adamw')


# ---- the SDS loop -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("texture_field", ["hashgrid", "mlp"])
def test_sds_loop_steps_with_fused_adam(dev, tmp_path, texture_field):
    """optim.fused_adam: two iterations of paint_zero123plus on the tiny product of test_hashtex_gpu; with the hash-grid field the table
    is deferred (no float gradient ever) and released when the loop ends."""
    import test_hashtex_gpu as TT
    from contexture_nerf_amd import config as CFG
    assert CFG.TrainConfig().optim.fused_adam is False
    tr = TT._tiny_trainer(dev, tmp_path, guide__texture_field=texture_field, optim__fused_adam=True, optim__field_texels='active')
    field = tr.texture_mlp
    before = [p.detach().clone() for p in field.parameters()]
    versions = [p._version for p in field.parameters()]
    log = tr.paint_zero123plus(iterations=2, tile=64)
    assert [r['i'] for r in log] == [0, 1] and all(np.isfinite(r['loss']) and np.isfinite(r['grad_norm']) and r['grad_norm'] > 0 for r in log)
    assert all(not torch.equal(a, b.detach()) for a, b in zip(before, field.parameters()))
    assert all(p._version > v for p, v in zip(field.parameters(), versions))
    assert all(bool(torch.isfinite(p).all()) for p in field.parameters())
    if texture_field == "hashgrid":
        enc = field.encoding
        assert enc.table.grad is None and not enc._defer and enc._pending is None
        assert not bool(enc._bwd_ws.any())                                               # the last step left the sums zeroed
