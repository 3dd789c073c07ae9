"""GPU: the hash-grid kernels against the rule (bit for bit), the `emb` seam of the MLP with its input gradient, the whole chain
field -> compositing -> loss against float64 autograd, and training through it.  Definitions: tests/hashgrid_rule.py, DESIGN section 4j."""
import ctypes as C
import functools
import numpy as np
import pytest
import torch

import hashgrid_rule as HG
import march_rule as mr
import test_occupancy_cpu as OC
import test_occupancy_mesh_cpu as OM
import test_occupancy_gpu as OG
import test_raymarch_train_cpu as RM

pytestmark = pytest.mark.gpu
f32 = np.float32
LO, HI = HG.BOX_LO, HG.BOX_HI
NEAR, FAR = 0.5, 2.5


def _arr(a, ctype):
    a = np.ascontiguousarray(a, ctype)
    return a, a.ctypes.data_as(C.c_void_p)


def _abi_fwd(dev, pts, table, res, log2T, lo=LO, hi=HI):
    from contexture_nerf_amd import _lib as L
    Lv, T, F = table.shape
    p, t = OG._dev(dev, pts, table)
    emb = torch.full((pts.shape[0], Lv * F), float('nan'), device=dev)
    (_r, rp), (_l, lp), (_h, hp) = _arr(res, np.int32), _arr(lo, f32), _arr(hi, f32)
    L.check(L.load().ctx_hashgrid_fwd(L.ptr(p), pts.shape[0], L.ptr(t), Lv, F, log2T, rp, lp, hp, L.ptr(emb), L.stream()))
    return emb.cpu().numpy()


def _abi_bwd(dev, pts, g_emb, res, log2T, F, lo=LO, hi=HI, ws=None):
    """-> g_table [Lv, T, F] as a device tensor; the buffer starts as NaN, the workspace as garbage (0xff)"""
    from contexture_nerf_amd import _lib as L
    lib = L.load()
    Lv = len(res)
    p, g = OG._dev(dev, pts, g_emb)
    out = torch.full((Lv, 1 << log2T, F), float('nan'), device=dev)
    if ws is None:
        ws = torch.full((lib.ctx_hashgrid_bwd_ws_bytes(Lv, F, log2T),), 0xff, dtype=torch.uint8, device=dev)
    (_r, rp), (_l, lp), (_h, hp) = _arr(res, np.int32), _arr(lo, f32), _arr(hi, f32)
    L.check(lib.ctx_hashgrid_bwd(L.ptr(p), pts.shape[0], L.ptr(g), Lv, F, log2T, rp, lp, hp, 7, L.ptr(ws), L.ptr(out), L.stream()))
    return out


@pytest.mark.parametrize("Lv,F,log2T", HG.GRID_CASES)
@pytest.mark.parametrize("max_res", [64, 512])
def test_kernels_equal_the_rule(dev, Lv, F, log2T, max_res):
    """Forward and backward, array_equal, on the anisotropic box: dense and hashed levels in one table, T = 16 where almost everything
    collides, points on faces, corners and nodes, outside the box, NaN and inf rows (case_points); n around the wave and block sizes."""
    res = HG.resolutions(Lv, 2, max_res)
    dense = [HG.is_dense(r, log2T) for r in res]
    if (Lv, log2T) in ((4, 6), (16, 12), (16, 10)):
        assert any(dense) and not all(dense)
    table = HG.case_table(Lv, F, log2T, seed=Lv + F)
    for n in HG.N_CASES:
        pts = HG.case_points(n, LO, HI, res, seed=n)
        got = _abi_fwd(dev, pts, table, res, log2T)
        assert np.array_equal(got, HG.forward_np(pts, table, LO, HI, res, log2T)), ("forward", n)
        g_emb = np.random.default_rng(n).standard_normal((n, Lv * F)).astype(f32) * f32(3e-3)
        gt = _abi_bwd(dev, pts, g_emb, res, log2T, F).cpu().numpy()
        assert np.array_equal(gt, HG.backward_np(pts, g_emb, LO, HI, res, log2T, F)), ("backward", n)


def test_node_count_beyond_32_bits(dev):
    """res = 2047: the level has 2048^3 = 2^33 nodes, a count that is 0 in 32 bits.  The level is hashed; a kernel that took the wrapped
    count for a dense level would index the table unmasked.  Forward and table backward, array_equal."""
    Lv, F, log2T, n, res = 1, 2, 12, 300, [2047]
    assert not HG.is_dense(res[0], log2T)
    table = HG.case_table(Lv, F, log2T, seed=5)
    pts = HG.case_points(n, LO, HI, res, seed=n)
    assert np.array_equal(_abi_fwd(dev, pts, table, res, log2T), HG.forward_np(pts, table, LO, HI, res, log2T))
    g_emb = np.random.default_rng(n).standard_normal((n, Lv * F)).astype(f32) * f32(3e-3)
    gt = _abi_bwd(dev, pts, g_emb, res, log2T, F).cpu().numpy()
    assert np.array_equal(gt, HG.backward_np(pts, g_emb, LO, HI, res, log2T, F))


def test_backward_contention_zero_nan_and_repeat(dev):
    Lv, F, log2T = 4, 2, 6
    res = HG.resolutions(Lv, 2, 64)
    rng = np.random.default_rng(3)
    # one point a thousand times: all adds land on eight entries per level
    pts = np.tile(f32([[0.3, 0.7, 0.5]]), (1000, 1))
    g_emb = rng.standard_normal((1000, Lv * F)).astype(f32)
    got = _abi_bwd(dev, pts, g_emb, res, log2T, F).cpu().numpy()
    assert np.array_equal(got, HG.backward_np(pts, g_emb, LO, HI, res, log2T, F))
    assert all(np.count_nonzero(got[l].any(-1)) <= 8 for l in range(Lv)) and got.any()
    # scales far from 1
    for scale in (1e-30, 1e20):
        gs = (g_emb * f32(scale)).astype(f32)
        assert np.array_equal(_abi_bwd(dev, pts, gs, res, log2T, F).cpu().numpy(), HG.backward_np(pts, gs, LO, HI, res, log2T, F))
    # all zero: zeros everywhere (the NaN prefill is gone); a NaN or an inf: NaN everywhere
    pts = HG.case_points(300, LO, HI, res, seed=1)
    g_emb = rng.standard_normal((300, Lv * F)).astype(f32)
    z = _abi_bwd(dev, pts, np.zeros_like(g_emb), res, log2T, F)
    assert not bool(z.any()) and bool(torch.isfinite(z).all())
    for bad in (np.nan, np.inf):
        gb = g_emb.copy()
        gb[123, 5] = bad
        assert bool(torch.isnan(_abi_bwd(dev, pts, gb, res, log2T, F)).all())
    # every element is written, five launches (one workspace, reused) and a side stream give the same bits
    from contexture_nerf_amd import _lib as L
    ws = torch.empty(L.load().ctx_hashgrid_bwd_ws_bytes(Lv, F, log2T), dtype=torch.uint8, device=dev)
    runs = [_abi_bwd(dev, pts, g_emb, res, log2T, F, ws=ws) for _ in range(5)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runs.append(_abi_bwd(dev, pts, g_emb, res, log2T, F))
    side.synchronize()
    assert bool(torch.isfinite(runs[0]).all()) and all(torch.equal(runs[0], r) for r in runs[1:])
    assert np.array_equal(runs[0].cpu().numpy(), HG.backward_np(pts, g_emb, LO, HI, res, log2T, F))


# ---- the MLP's input seam ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [64, 256])
def test_forward_features_is_forward_at_63_columns(dev, W):
    """One code path: on the 63-column embedding forward_features gives the bits of NeRF2D.forward, in the output and in every parameter
    gradient (and a finite input gradient on top)."""
    from contexture_nerf_amd.run_nerf_helpers import NeRF2D
    torch.manual_seed(3)
    net = NeRF2D(D=8, W=W, input_ch=63, output_ch=4, skips=[4]).to(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    emb = torch.randn(200, 63, device=dev, generator=g)
    g_raw = torch.randn(200, 4, device=dev, generator=g)
    outs, grads = [], []
    for fn, x in ((net.forward, emb), (net.forward_features, emb), (net.forward_features, emb.clone().requires_grad_(True))):
        net.zero_grad(set_to_none=True)
        raw = fn(x)
        raw.backward(g_raw)
        outs.append(raw.detach())
        grads.append([p.grad.clone() for p in net._params()])
        if x.requires_grad:
            assert x.grad.shape == (200, 63) and bool(torch.isfinite(x.grad).all()) and bool(x.grad.any())
    with torch.no_grad():
        outs.append(net.forward_features(emb))
    assert all(torch.equal(outs[0], o) for o in outs[1:])
    for other in grads[1:]:
        assert len(other) == 18 and all(torch.equal(a, b) for a, b in zip(grads[0], other))


@functools.lru_cache(maxsize=None)
def _mlp_reference(D, W, input_ch, skip, N):
    params = HG.make_params(D, W, input_ch, 4, skip, seed=D * 1000 + W + input_ch)
    g = torch.Generator().manual_seed(N)
    emb = torch.randn(N, input_ch, generator=g)
    g_raw = torch.randn(N, 4, generator=g)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        ps = [p.clone().to(dtype).requires_grad_(True) for p in params]        # clone: .to() of the same dtype is the tensor itself
        e = emb.clone().to(dtype).requires_grad_(True)
        raw = HG.mlp_torch(e, ps, skip)
        raw.backward(g_raw.to(dtype))
        ref[dtype] = (raw.detach(), [e.grad] + [p.grad for p in ps])
    return params, emb, g_raw, ref


def _load_params(net, params):
    with torch.no_grad():
        for p, v in zip(net._params(), params):
            p.copy_(v)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@pytest.mark.parametrize("D,W,input_ch,skip", [(2, 64, 32, 0), (2, 64, 1, 0), (3, 128, 64, 1), (8, 64, 63, 4)])
def test_input_and_parameter_gradients_vs_float64(dev, D, W, input_ch, skip):
    """grad_emb and the parameter gradients of forward_features against float64 CPU autograd of a torch MLP: per tensor the relative L2
    distance may be four times that of the float32 CPU run of the same reference and never has to be below 2e-4 (the criterion of
    test_raymarch_train_gpu.test_whole_chain_parameter_gradients); the forward at the texture field's rtol 1e-4, atol 2e-5."""
    from contexture_nerf_amd.run_nerf_helpers import NeRF2D
    net = NeRF2D(D=D, W=W, input_ch=input_ch, output_ch=4, skips=[skip]).to(dev)
    for N in (1, 64, 65, 200):
        params, emb, g_raw, ref = _mlp_reference(D, W, input_ch, skip, N)
        _load_params(net, params)
        net.zero_grad(set_to_none=True)
        e = emb.to(dev).requires_grad_(True)
        raw = net.forward_features(e)
        raw.backward(g_raw.to(dev))
        want_raw, want = ref[torch.float64]
        np.testing.assert_allclose(raw.detach().cpu().numpy(), want_raw.numpy(), rtol=1e-4, atol=2e-5)
        got = [e.grad.cpu()] + [p.grad.cpu() for p in net._params()]
        rows = [(_rel(a, w), _rel(c, w)) for a, w, c in zip(got, want, ref[torch.float32][1])]
        print(f"forward_features D={D} W={W} input_ch={input_ch} N={N}: relative L2, grad_emb {rows[0][0]:.3e} (float32 CPU {rows[0][1]:.3e}), "
              f"parameters worst {max(r[0] for r in rows[1:]):.3e} (float32 CPU {max(r[1] for r in rows[1:]):.3e})")
        for i, (a, c) in enumerate(rows):
            assert a <= max(4 * c, 2e-4), (N, i, a, c)
        # frozen parameters: the input gradient alone, the same bits
        for p in net.parameters():
            p.requires_grad_(False)
        e2 = emb.to(dev).requires_grad_(True)
        net.forward_features(e2).backward(g_raw.to(dev))
        assert torch.equal(e2.grad, e.grad)
        for p in net.parameters():
            p.requires_grad_(True)


# ---- the whole chain -----------------------------------------------------------------------------------------------------------------
def _small_field(dev, seed=0):
    from contexture_nerf_amd.hashgrid import HashGridField
    torch.manual_seed(seed)
    field = HashGridField(-1.0, 1.0, n_levels=4, n_features=2, log2_table=8, base_res=2, max_res=16).to(dev)
    with torch.no_grad():
        field.encoding.table.copy_(torch.randn(field.encoding.table.shape, generator=torch.Generator().manual_seed(seed + 1)) * 0.5)
        field.mlp.output_linear.bias[3] = 1.0
    return field


def _field_tensors(field):
    return [field.encoding.table] + field.mlp._params()


def _torch_field(field, tensors, pts, dtype):
    enc = field.encoding
    emb = HG.forward_torch(pts.reshape(-1, 3).numpy(), tensors[0], enc.lo, enc.hi, enc.res, enc.log2_table, dtype=dtype)
    return HG.mlp_torch(emb, tensors[1:], 0).reshape(*pts.shape[:-1], 4)


def _chain_reference(field, t32, passes, rd, target, dtype):
    """Gradients of img2mse(rgb, target) + 0.1 acc.mean() on the last pass (+ img2mse on an earlier, coarse one) by CPU autograd in `dtype`.
    passes: ('packed', pts, t, dt, ray_off) or ('dense', pts [R,S,3], z)."""
    ts = [x.clone().to(dtype).requires_grad_(True) for x in t32]
    rd, target = rd.to(dtype), target.to(dtype)
    loss = 0.
    for k, ps in enumerate(passes):
        raw = _torch_field(field, ts, ps[1], dtype)
        if ps[0] == 'packed':
            rgb, _, acc, _, _ = mr.restate_packed(raw, ps[2].to(dtype), ps[3].to(dtype), rd, ps[4])
        else:
            rgb, _, acc, _, _ = RM.restate(raw, ps[2].to(dtype), rd)
        loss = loss + ((rgb - target) ** 2).mean()
        if k == len(passes) - 1:
            loss = loss + 0.1 * acc.mean()
    loss.backward()
    return [x.grad for x in ts]


@pytest.mark.parametrize("mode", ["marched", "dense", "resampled"])
def test_whole_chain_gradients_vs_float64(dev, mode):
    """HashGridField -> compositing -> img2mse + 0.1 acc.mean(): the gradients of the table and of the six MLP tensors against float64 CPU
    autograd through a torch restatement (the rule's cells and weights, a torch MLP, the compositing restatements), at the criterion of
    test_raymarch_train_gpu.test_whole_chain_parameter_gradients.  The sample lists are outside the gradient: the reference takes those of
    the HIP run."""
    from contexture_nerf_amd import run_nerf_helpers as rnh, volume_render as vr
    field = _small_field(dev)
    grid = vr.OccupancyGrid.from_mask(torch.from_numpy(OM.ball_mask(8, 0.6)).to(dev), -1.0, 1.0)
    R = 96
    ro, rd, _ = OG._dev(dev, *OC.random_rays(np.random.default_rng(5), R, 4, spread=0.5))
    target = torch.rand(R, 3, generator=torch.Generator().manual_seed(2))
    step = float(grid.h[0]) / 2
    if mode == "dense":
        out, ex = rnh.render_rays(field, ro, rd, NEAR, FAR, 33, return_extras=True)
        z = ex['z_vals'].cpu()
        passes = [('dense', ro.cpu()[:, None, :] + rd.cpu()[:, None, :] * z[:, :, None], z)]
    else:
        out, ex = rnh.render_rays(field, ro, rd, NEAR, FAR, 0, occupancy=grid, march=step, resample=8 if mode == "resampled" else 0,
                                  return_extras=True)
        passes = [('packed', ex['pts'].cpu(), ex['t'].cpu(), ex['dt'].cpu(), ex['ray_off'].cpu())]
        assert ex['t'].numel() > R
    loss = rnh.img2mse(out[0], target.to(dev)) + 0.1 * out[2].mean()
    if mode == "resampled":
        loss = loss + rnh.img2mse(ex['rgb0'], target.to(dev))
        passes.insert(0, ('packed', ex['pts0'].cpu(), ex['t0'].cpu(), ex['dt0'].cpu(), ex['ray_off0'].cpu()))
    loss.backward()
    tensors = _field_tensors(field)
    assert len(tensors) == 7
    got = [x.grad.cpu() for x in tensors]
    t32 = [x.detach().cpu() for x in tensors]
    want = _chain_reference(field, t32, passes, rd.cpu(), target, torch.float64)
    c32 = _chain_reference(field, t32, passes, rd.cpu(), target, torch.float32)
    rows = [(_rel(a, w), _rel(c, w)) for a, w, c in zip(got, want, c32)]
    print(f"hash-grid chain ({mode}): relative L2, table {rows[0][0]:.3e} (float32 CPU {rows[0][1]:.3e}), MLP worst "
          f"{max(r[0] for r in rows[1:]):.3e} (float32 CPU {max(r[1] for r in rows[1:]):.3e})")
    assert bool(got[0].any())
    for i, (a, c) in enumerate(rows):
        assert a <= max(4 * c, 2e-4), (i, a, c)


# ---- training ------------------------------------------------------------------------------------------------------------------------
def _shell_grid(dev, G=16):
    from contexture_nerf_amd import volume_render as vr
    v, f = OM.icosphere(2, 0.6)
    return vr.OccupancyGrid.from_mesh(*OG._dev(dev, v, f), G, -1.0, 1.0, dilate=1)


def test_fit_views_trains_and_repeats(dev):
    """The toy scene of DESIGN 4g (the shell of the icosphere of radius 0.6 at G = 16, static, marched at h/2) on the teacher views of
    test_raymarch_train_gpu: the loss falls, the grid stays, and two runs give the same history and the same table bit for bit."""
    import test_raymarch_train_gpu as RT
    from contexture_nerf_amd import volume_render as vr
    from contexture_nerf_amd.hashgrid import HashGridField
    images, c2ws, K = RT._teacher_views(dev)
    runs = []
    for _ in range(2):
        grid = _shell_grid(dev)
        before = grid.cells.clone()
        torch.manual_seed(9)
        student = HashGridField.from_grid(grid, n_levels=8, n_features=2, log2_table=12, base_res=4, max_res=64).to(dev)
        hist = vr.fit_views(student, images, c2ws, K, NEAR, FAR, iters=40, rays_per_iter=128, lr=1e-2, seed=0, occupancy=grid, occupancy_every=0,
                            march=float(grid.h[0]) / 2)
        assert torch.equal(grid.cells, before) and not bool(grid.dens.any())
        runs.append((hist, student))
    h = runs[0][0]
    print(f"fit_views with a HashGridField: first five {np.mean(h[:5]):.5f}, last five {np.mean(h[-5:]):.5f}")
    assert len(h) == 40 and all(np.isfinite(v) for v in h)
    assert np.mean(h[-5:]) < np.mean(h[:5])
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1].encoding.table, runs[1][1].encoding.table)
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1].mlp._params(), runs[1][1].mlp._params()))
    # the field serves the grid's refresh and the image render as any field does
    student, grid = runs[0][1], _shell_grid(dev)
    grid.update(student, 0.01)
    assert bool(torch.isfinite(grid.dens).all()) and bool(grid.dens.any())
    img = vr.render_image(student, 16, 16, K, c2ws[0], NEAR, FAR, 0, occupancy=_shell_grid(dev), march=0.0625)
    assert tuple(img['rgb'].shape) == (16, 16, 3) and bool(torch.isfinite(img['rgb']).all()) and float(img['acc'].max()) > 0


def test_empty_grid_and_no_grad_leave_the_field_alone(dev):
    from contexture_nerf_amd import volume_render as vr
    field = _small_field(dev, seed=4)
    grid = vr.OccupancyGrid.from_mask(torch.zeros(8, 8, 8, dtype=torch.bool, device=dev), -1.0, 1.0)
    ro, rd, _ = OG._dev(dev, *OC.random_rays(np.random.default_rng(1), 9, 4))
    before = [p.detach().clone() for p in field.parameters()]
    opt = torch.optim.Adam(field.parameters(), lr=1e-2)
    step = vr.train_step(field, opt, ro, rd, torch.rand(9, 3, device=dev), NEAR, FAR, 64, occupancy=grid, march=0.125)
    assert torch.isfinite(step['loss'])
    assert len(before) == 7 and all(torch.equal(a, b) for a, b in zip(before, field.parameters()))
    # no grad: no graph, nothing kept; zero points: an empty result
    pts = torch.rand(65, 3, device=dev) * 2 - 1
    with torch.no_grad():
        raw = field.forward_pts(pts)
    assert raw.shape == (65, 4) and raw.grad_fn is None and field.mlp._saved_pool is None
    assert torch.equal(raw, field.forward_pts(pts).detach())
    assert field.forward_pts(pts[:0]).shape == (0, 4) and field.forward_pts(pts.reshape(5, 13, 3)).shape == (5, 13, 4)


def test_refusals(dev):
    from contexture_nerf_amd import _lib as L
    from contexture_nerf_amd.hashgrid import HashGridEncoding, HashGridField
    from contexture_nerf_amd.run_nerf_helpers import NeRF2D
    for kw in (dict(n_levels=17, n_features=4), dict(n_features=3), dict(log2_table=3), dict(log2_table=23)):
        with pytest.raises(L.CtxError):
            HashGridEncoding(-1.0, 1.0, **kw)
    for lo, hi in ((1.0, 1.0), ((0, 0, 0), (1, -1, 1)), (0.0, float('inf'))):
        with pytest.raises(L.CtxError, match="finite lo < hi"):
            HashGridField(lo, hi, log2_table=4)
    enc = HashGridEncoding(-1.0, 1.0, n_levels=2, log2_table=4).to(dev)
    with pytest.raises(L.CtxError, match="no gradient with respect to the positions"):
        enc(torch.zeros(4, 3, device=dev, requires_grad=True))
    with pytest.raises(L.CtxError, match="device tensor"):
        enc(torch.zeros(4, 3))
    with pytest.raises(L.CtxError, match=r"pts \[\.\.\., 3\]"):
        enc(torch.zeros(4, 2, device=dev))
    with pytest.raises(L.CtxError, match="input_ch=65"):
        NeRF2D(D=2, W=64, input_ch=65, output_ch=4, skips=[0]).to(dev).forward_features(torch.zeros(3, 65, device=dev))
    # the ABI refuses the same before any launch: the outputs keep their prefill
    lib = L.load()
    pts, table = torch.zeros(4, 3, device=dev), torch.zeros(2, 16, 2, device=dev)
    emb = torch.full((4, 4), 7.0, device=dev)
    (_r, rp), (_l, lp), (_h, hp) = _arr([2, 4], np.int32), _arr([0, 0, 0], f32), _arr([1, 1, 1], f32)
    for Lv, F, k in ((17, 4, 4), (2, 3, 4), (2, 2, 3), (2, 2, 23)):
        assert lib.ctx_hashgrid_fwd(L.ptr(pts), 4, L.ptr(table), Lv, F, k, rp, lp, hp, L.ptr(emb), L.stream()) != 0
        assert lib.ctx_hashgrid_bwd_ws_bytes(Lv, F, k) == -1
    (_h2, hp2) = _arr([1, 0, 1], f32)
    assert lib.ctx_hashgrid_fwd(L.ptr(pts), 4, L.ptr(table), 2, 2, 4, rp, lp, hp2, L.ptr(emb), L.stream()) != 0
    assert b"lo < hi" in lib.ctx_last_error()
    raw = torch.full((4, 4), 7.0, device=dev)
    blob = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    assert lib.ctx_uvmlp_fwd_emb(L.ptr(emb), 4, L.ptr(blob), 2, 64, 65, 4, 0, L.ptr(raw), None, L.stream()) != 0
    assert b"input_ch=65" in lib.ctx_last_error()
    assert bool((emb == 7.0).all()) and bool((raw == 7.0).all())
