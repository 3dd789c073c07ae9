"""GPU: the hash-grid encoding's gradient to the positions against its rule (bit for bit), the opt-in autograd path, density_gradient
against float64 autograd, the per-ray weighted sum, and render_normals' conventions and composition.
Definitions: tests/hashgrid_grad_rule.py, DESIGN section 4k."""
import ctypes as C
import functools
import numpy as np
import pytest
import torch

import hashgrid_rule as HG
import hashgrid_grad_rule as GR
import distortion_rule as DR
import test_occupancy_mesh_cpu as OM
import test_occupancy_gpu as OG

pytestmark = pytest.mark.gpu
f32 = np.float32
LO, HI = HG.BOX_LO, HG.BOX_HI
NEAR, FAR = 0.5, 2.5


def _arr(a, ctype):
    a = np.ascontiguousarray(a, ctype)
    return a, a.ctypes.data_as(C.c_void_p)


def _abi_bwd_pts(dev, pts, table, g_emb, res, log2T, lo, hi):
    """-> g_pts [n,3] as a device tensor; the output starts as NaN, the scratch as garbage (0xff)"""
    from contexture_nerf_amd import _lib as L
    lib = L.load()
    Lv, T, F = table.shape
    n = pts.shape[0]
    p, t, g = OG._dev(dev, pts, table, g_emb)
    out = torch.full((n, 3), float('nan'), device=dev)
    ws = torch.full((lib.ctx_hashgrid_bwd_pts_ws_bytes(n, Lv),), 0xff, dtype=torch.uint8, device=dev)
    (_r, rp), (_l, lp), (_h, hp) = _arr(res, np.int32), _arr(np.broadcast_to(f32(lo), (3,)), f32), _arr(np.broadcast_to(f32(hi), (3,)), f32)
    L.check(lib.ctx_hashgrid_bwd_pts(L.ptr(p), n, L.ptr(t), L.ptr(g), Lv, F, log2T, rp, lp, hp, L.ptr(ws), L.ptr(out), L.stream()))
    return out


@pytest.mark.parametrize("Lv,F,log2T", HG.GRID_CASES)
@pytest.mark.parametrize("box", [(LO, HI), (-1.0, 1.0)], ids=["anisotropic", "cube"])
def test_kernel_equals_the_rule(dev, Lv, F, log2T, box):
    """array_equal on dense and hashed levels, every F, n around the wave and block sizes, points on faces, corners and nodes, outside the
    box, NaN and inf rows (case_points); two runs give the same bits; the NaN prefill is gone."""
    lo, hi = box
    res = HG.resolutions(Lv, 2, 64)
    table = HG.case_table(Lv, F, log2T, seed=Lv + F)
    for n in HG.N_CASES:
        pts = HG.case_points(n, np.broadcast_to(f32(lo), (3,)), np.broadcast_to(f32(hi), (3,)), res, seed=n)
        g_emb = np.random.default_rng(n + 7).standard_normal((n, Lv * F)).astype(f32)
        got = _abi_bwd_pts(dev, pts, table, g_emb, res, log2T, lo, hi)
        again = _abi_bwd_pts(dev, pts, table, g_emb, res, log2T, lo, hi)
        assert torch.equal(got, again) and bool(torch.isfinite(got).all())
        want = GR.grad_pts_np(pts, table, g_emb, np.broadcast_to(f32(lo), (3,)), np.broadcast_to(f32(hi), (3,)), res, log2T)
        assert np.array_equal(got.cpu().numpy(), want), n
        assert want.any() or n == 1


def test_non_finite_inputs_reach_the_active_axes_only(dev):
    Lv, F, log2T, n = 4, 2, 6, 65
    res = HG.resolutions(Lv, 2, 64)
    pts = HG.case_points(n, LO, HI, res, seed=n)
    table = np.full((Lv, 1 << log2T, F), np.nan, f32)
    g_emb = np.full((n, Lv * F), np.inf, f32)
    got = _abi_bwd_pts(dev, pts, table, g_emb, res, log2T, LO, HI).cpu().numpy()
    act = GR.active_np(pts, LO, HI)
    assert act.any() and (~act).any()
    assert np.all(got[~act] == 0) and np.all(np.isnan(got[act]))


def test_abi_refusals(dev):
    """Each a refusal before any launch: the output keeps its prefill."""
    from contexture_nerf_amd import _lib as L
    lib = L.load()
    pts, table = torch.zeros(4, 3, device=dev), torch.zeros(2, 16, 2, device=dev)
    g_emb = torch.zeros(4, 4, device=dev)
    out = torch.full((4, 3), 7.0, device=dev)
    ws = torch.zeros(4096, dtype=torch.uint8, device=dev)
    (_r, rp), (_l, lp), (_h, hp) = _arr([2, 4], np.int32), _arr([0, 0, 0], f32), _arr([1, 1, 1], f32)

    def call(p=pts, n=4, t=table, g=g_emb, Lv=2, F=2, k=4, r=rp, lo=lp, hi=hp, w=ws, o=out):
        return lib.ctx_hashgrid_bwd_pts(L.ptr(p), n, L.ptr(t), L.ptr(g), Lv, F, k, r, lo, hi, L.ptr(w), L.ptr(o), L.stream())

    assert call() == 0 and bool((out == 0.0).all())                     # the accepted call, for contrast: zeros (a zero table)
    out.fill_(7.0)
    for kw in (dict(p=None), dict(t=None), dict(g=None), dict(w=None), dict(o=None), dict(r=None), dict(lo=None), dict(hi=None)):
        assert call(**kw) != 0, kw
        assert b"null" in lib.ctx_last_error()
    assert call(n=0) != 0 and b"n=0" in lib.ctx_last_error()
    assert call(n=1 << 31) != 0
    assert call(F=3) != 0 and b"F=3" in lib.ctx_last_error()
    # Lv * F > 64: with F in {1, 2, 4} and Lv <= 16 the product stops at 64, so the width is exceeded together with the level count
    assert call(Lv=17, F=4) != 0 and b"Lv=17" in lib.ctx_last_error()
    (_h2, hp2) = _arr([1, 0, 1], f32)
    assert call(hi=hp2) != 0 and b"lo < hi" in lib.ctx_last_error()
    with pytest.raises(L.CtxError):
        L.check(call(F=3))
    assert bool((out == 7.0).all())
    # a scratch that is too small cannot be seen by the callee: the size query refuses what the entry point refuses
    assert lib.ctx_hashgrid_bwd_pts_ws_bytes(4, 2) >= 2 * 4 * 3 * 4
    assert lib.ctx_hashgrid_bwd_pts_ws_bytes(300, 16) >= 16 * 300 * 3 * 4
    for n, Lv in ((0, 2), (-1, 2), (1 << 31, 2), (4, 0), (4, 17)):
        assert lib.ctx_hashgrid_bwd_pts_ws_bytes(n, Lv) == -1, (n, Lv)


def test_widest_accepted_embedding(dev):
    """Lv * F = 64, the edge of the envelope, runs and equals the rule."""
    Lv, F, log2T, n = 16, 4, 4, 65
    res = HG.resolutions(Lv, 2, 64)
    table = HG.case_table(Lv, F, log2T, seed=3)
    pts = HG.case_points(n, LO, HI, res, seed=n)
    g_emb = np.random.default_rng(1).standard_normal((n, Lv * F)).astype(f32)
    got = _abi_bwd_pts(dev, pts, table, g_emb, res, log2T, LO, HI)
    assert np.array_equal(got.cpu().numpy(), GR.grad_pts_np(pts, table, g_emb, LO, HI, res, log2T))


@pytest.mark.parametrize("forced", ["0", "1"])
def test_each_mapping_gives_the_rule_s_bits(dev, monkeypatch, forced):
    """CTX_HASHGRID_PTS_LOOP forces one of the two mappings (0: a thread per (point, level) and the scratch; 1: a thread per point over the
    levels): the rule's bits from both, on every grid case."""
    monkeypatch.setenv("CTX_HASHGRID_PTS_LOOP", forced)
    for Lv, F, log2T in HG.GRID_CASES:
        res = HG.resolutions(Lv, 2, 64)
        table = HG.case_table(Lv, F, log2T, seed=Lv + F)
        for n in (65, 300):
            pts = HG.case_points(n, LO, HI, res, seed=n)
            g_emb = np.random.default_rng(n + 7).standard_normal((n, Lv * F)).astype(f32)
            got = _abi_bwd_pts(dev, pts, table, g_emb, res, log2T, LO, HI)
            assert np.array_equal(got.cpu().numpy(), GR.grad_pts_np(pts, table, g_emb, LO, HI, res, log2T)), (Lv, F, n)


@pytest.mark.parametrize("n", [(1 << 17) - 1, 1 << 17])
def test_the_threshold_between_the_mappings(dev, monkeypatch, n):
    """Below 2^17 points the per-level mapping runs, from there on the per-point one: both sides of the threshold equal the rule and each
    other's forced run (Lv = 4, F = 2: the restatement of 131072 points stays quick)."""
    Lv, F, log2T = 4, 2, 6
    res = HG.resolutions(Lv, 2, 64)
    table = HG.case_table(Lv, F, log2T, seed=2)
    pts = HG.case_points(n, LO, HI, res, seed=3)
    g_emb = np.random.default_rng(4).standard_normal((n, Lv * F)).astype(f32)
    monkeypatch.delenv("CTX_HASHGRID_PTS_LOOP", raising=False)
    got = _abi_bwd_pts(dev, pts, table, g_emb, res, log2T, LO, HI)
    assert np.array_equal(got.cpu().numpy(), GR.grad_pts_np(pts, table, g_emb, LO, HI, res, log2T))
    for forced in ("0", "1"):
        monkeypatch.setenv("CTX_HASHGRID_PTS_LOOP", forced)
        assert torch.equal(_abi_bwd_pts(dev, pts, table, g_emb, res, log2T, LO, HI), got)


# ---- autograd --------------------------------------------------------------------------------------------------------------------------
def test_autograd_opt_in(dev):
    from contexture_nerf_amd import _lib as L
    from contexture_nerf_amd.hashgrid import HashGridEncoding, HashGridField
    Lv, F, log2T, n = 4, 2, 6, 300
    kw = dict(n_levels=Lv, n_features=F, log2_table=log2T, base_res=2, max_res=64)
    enc = HashGridEncoding(LO, HI, grad_pts=True, **kw).to(dev)
    res = HG.resolutions(Lv, 2, 64)
    assert np.array_equal(enc.res, res)
    table = HG.case_table(Lv, F, log2T, seed=1)
    with torch.no_grad():
        enc.table.copy_(torch.from_numpy(table))
    pts = HG.case_points(n, LO, HI, res, seed=n).reshape(5, -1, 3)                # a leading shape: the gradient takes pts's shape
    g = np.random.default_rng(2).standard_normal((pts.shape[0] * pts.shape[1], Lv * F)).astype(f32)
    g_t = torch.from_numpy(g).to(dev).reshape(5, -1, Lv * F)
    p = torch.from_numpy(pts).to(dev).requires_grad_(True)
    (enc(p) * g_t).sum().backward()
    assert p.grad.shape == p.shape
    assert np.array_equal(p.grad.cpu().numpy().reshape(-1, 3), GR.grad_pts_np(pts, table, g, LO, HI, res, log2T))
    with_pts = enc.table.grad.clone()
    enc.table.grad = None
    (enc(p.detach()) * g_t).sum().backward()
    assert torch.equal(enc.table.grad, with_pts) and bool(with_pts.any())
    # a frozen table: the positions' gradient alone, the same bits
    enc.table.requires_grad_(False)
    p2 = torch.from_numpy(pts).to(dev).requires_grad_(True)
    (enc(p2) * g_t).sum().backward()
    assert torch.equal(p2.grad, p.grad)
    # first order only
    enc.table.requires_grad_(True)
    p3 = torch.from_numpy(pts).to(dev).requires_grad_(True)
    gp, = torch.autograd.grad((enc(p3) * g_t).sum(), p3, create_graph=True)
    assert torch.equal(gp, p.grad)
    with pytest.raises(RuntimeError):
        gp.sum().backward()
    # the whole field, through the MLP's grad_emb link; from_grid hands the keyword on
    field = HashGridField(-1.0, 1.0, grad_pts=True, **kw).to(dev)
    q = (torch.rand(65, 3, device=dev) * 1.8 - 0.9).requires_grad_(True)
    field.forward_pts(q)[:, 3].sum().backward()
    assert q.grad.shape == (65, 3) and bool(torch.isfinite(q.grad).all()) and bool(q.grad.any())
    from contexture_nerf_amd import volume_render as vr
    grid = vr.OccupancyGrid(4, -1.0, 1.0, dev)
    assert HashGridField.from_grid(grid, grad_pts=True, **kw).encoding.grad_pts is True
    assert HashGridField.from_grid(grid, **kw).encoding.grad_pts is False


def test_default_still_refuses_positions_that_require_grad(dev):
    from contexture_nerf_amd import _lib as L
    from contexture_nerf_amd.hashgrid import HashGridEncoding
    enc = HashGridEncoding(-1.0, 1.0, n_levels=2, log2_table=4).to(dev)
    with pytest.raises(L.CtxError, match="no gradient with respect to the positions"):
        enc(torch.zeros(4, 3, device=dev, requires_grad=True))


# ---- density_gradient ------------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@functools.lru_cache(maxsize=None)
def _density_reference():
    """n = 300, Lv = 4, F = 2, T = 2^6, D = 2, W = 64 on the box -1 .. 1: d raw[:, 3] / d pts by CPU autograd through the differentiable
    restatement of the encoding and the torch MLP, in float64 and in float32."""
    Lv, F, log2T, n = 4, 2, 6, 300
    res = HG.resolutions(Lv, 2, 16)
    table = (HG.case_table(Lv, F, log2T, seed=5) * f32(0.5)).astype(f32)
    params = HG.make_params(2, 64, Lv * F, 4, 0, seed=11)
    pts = (np.random.default_rng(4).random((n, 3)) * 1.9 - 0.95).astype(f32)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        p = torch.from_numpy(pts).to(dtype).requires_grad_(True)
        emb = GR.forward_torch_pts(p, torch.from_numpy(table).to(dtype), -1.0, 1.0, res, log2T)
        raw = HG.mlp_torch(emb, [x.clone().to(dtype) for x in params], 0)
        raw[:, 3].sum().backward()
        ref[dtype] = (raw.detach(), p.grad)
    return res, table, params, pts, ref


def test_density_gradient_vs_float64(dev):
    """At most 4 x the relative L2 distance of the float32 CPU autograd run of the same reference to float64: the factor covers a different
    summation order along the MLP chain."""
    from contexture_nerf_amd.hashgrid import HashGridField
    res, table, params, pts, ref = _density_reference()
    fields = []
    for grad_pts in (False, True):
        field = HashGridField(-1.0, 1.0, n_levels=4, n_features=2, log2_table=6, base_res=2, max_res=16, D=2, W=64, grad_pts=grad_pts).to(dev)
        assert np.array_equal(field.encoding.res, res)
        with torch.no_grad():
            field.encoding.table.copy_(torch.from_numpy(table))
            for p, v in zip(field.mlp._params(), params):
                p.copy_(v)
        fields.append(field)
    field = fields[0]
    p = torch.from_numpy(pts).to(dev)
    raw, grad = field.density_gradient(p, return_raw=True)
    assert raw.shape == (300, 4) and grad.shape == (300, 3) and raw.grad_fn is None and grad.grad_fn is None
    assert all(x.grad is None for x in field.parameters())
    assert field.mlp._saved_pool is not None                                      # the activation pool is back
    want_raw, want = ref[torch.float64]
    got, cpu32 = _rel(grad.cpu(), want), _rel(ref[torch.float32][1], want)
    print(f"density_gradient: relative L2 to float64 {got:.3e} (float32 CPU autograd {cpu32:.3e})")
    np.testing.assert_allclose(raw.cpu().numpy(), want_raw.numpy(), rtol=1e-4, atol=2e-5)
    assert got <= 4 * cpu32, (got, cpu32)
    # the ambient grad mode, grad_pts, a leading shape and a pts that requires grad change no bit; forward_pts gives the same raw
    with torch.no_grad():
        assert torch.equal(field.density_gradient(p), grad)
    raw2, grad2 = fields[1].density_gradient(p.clone().requires_grad_(True).reshape(3, 100, 3), return_raw=True)
    assert torch.equal(grad2.reshape(-1, 3), grad) and torch.equal(raw2.reshape(-1, 4), raw)
    assert all(x.grad is None for x in fields[1].parameters())
    with torch.no_grad():
        assert torch.equal(field.forward_pts(p), raw)
    # autograd through the opt-in path arrives at the same bits
    q = p.clone().requires_grad_(True)
    fields[1].forward_pts(q)[:, 3].sum().backward()
    assert torch.equal(q.grad, grad)
    # other channels, and none
    g0 = field.density_gradient(p, channel=0)
    assert g0.shape == (300, 3) and not torch.equal(g0, grad)
    assert field.density_gradient(p[:0]).shape == (0, 3)
    from contexture_nerf_amd import _lib as L
    with pytest.raises(L.CtxError, match="channel"):
        field.density_gradient(p, channel=4)


# ---- the per-ray weighted sum -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", [1, 3, 4])
def test_weighted_sum_packed(dev, Cn):
    from contexture_nerf_amd import _lib as L, run_nerf_helpers as rnh
    w, v, ray_off = GR.weighted_sum_case(DR.COUNTS, Cn, seed=Cn)
    want, bnd = GR.weighted_sum_f64(w, v, ray_off)
    dw, dv, do = OG._dev(dev, w, v, ray_off)
    got = rnh.weighted_sum_packed(dw, dv, do)
    assert got.shape == (len(DR.COUNTS), Cn) and torch.equal(got, rnh.weighted_sum_packed(dw, dv, do))
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    print(f"weighted_sum_packed C={Cn}: worst error / bound {float((err[bnd > 0] / bnd[bnd > 0]).max()):.3f}")
    assert np.all(err <= bnd)
    empty = np.diff(ray_off) == 0
    assert empty.any() and bool((got[torch.from_numpy(empty).to(dev)] == 0).all())
    # quantised inputs: every product and every partial sum is exact, whatever the order
    w, v, ray_off = GR.weighted_sum_case(DR.COUNTS, Cn, seed=Cn + 10, quantised=True)
    got = rnh.weighted_sum_packed(*OG._dev(dev, w, v, ray_off))
    assert np.array_equal(got.cpu().numpy().astype(np.float64), GR.weighted_sum_f64(w, v, ray_off)[0])
    # no samples at all: zeros
    z = rnh.weighted_sum_packed(dw[:0], dv[:0], torch.zeros(4, dtype=torch.int64, device=dev))
    assert z.shape == (3, Cn) and not bool(z.any())


def test_weighted_sum_packed_refusals(dev):
    from contexture_nerf_amd import _lib as L, run_nerf_helpers as rnh
    w, v, ray_off = OG._dev(dev, *GR.weighted_sum_case([3, 0, 2], 5, seed=0))
    with pytest.raises(L.CtxError, match="C=5"):
        rnh.weighted_sum_packed(w, v, ray_off)
    out = torch.full((3, 5), 7.0, device=dev)
    assert L.load().ctx_weighted_sum_packed(L.ptr(w), L.ptr(v), L.ptr(ray_off), 3, 5, 5, L.ptr(out), L.stream()) != 0
    assert bool((out == 7.0).all())
    v3 = v[:, :3].contiguous()
    with pytest.raises(L.CtxError, match="no gradient"):
        rnh.weighted_sum_packed(w.clone().requires_grad_(True), v3, ray_off)
    with pytest.raises(L.CtxError, match="no gradient"):
        rnh.weighted_sum_packed(w, v3.clone().requires_grad_(True), ray_off)
    with pytest.raises(L.CtxError):
        rnh.weighted_sum_packed(w, v3[:4], ray_off)


# ---- render_normals ---------------------------------------------------------------------------------------------------------------------
class _BallField:
    """raw[:, 3] = k * (0.6^2 - |p|^2), a constant colour; the gradient is analytic: -2 k p."""
    k = 1000.0

    def density_gradient(self, pts, channel=3, return_raw=False):
        raw = torch.full((pts.shape[0], 4), 0.5, device=pts.device)
        raw[:, 3] = self.k * (0.36 - (pts * pts).sum(-1))
        g = -2.0 * self.k * pts
        return (raw, g) if return_raw else g


def _ball_grid(dev, G=16):
    from contexture_nerf_amd import volume_render as vr
    return vr.OccupancyGrid.from_mask(torch.from_numpy(OM.ball_mask(G, 0.6)).to(dev), -1.0, 1.0)


C2W_FRONT = [[1., 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1.5]]               # on +z, looking down -z at the origin
C2W_BACK = [[-1., 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, -1.5]]             # on -z, turned about y: looking down +z at the origin


def test_render_normals_conventions(dev):
    from contexture_nerf_amd import run_nerf_helpers as rnh, volume_render as vr
    grid = _ball_grid(dev)
    H = W = 16
    K = vr.pinhole(H, W)
    step = float(grid.h[0]) / 2
    outs = {}
    for name, c2w in (("front", C2W_FRONT), ("back", C2W_BACK)):
        c2w = torch.tensor(c2w, device=dev)
        out = vr.render_normals(_BallField(), H, W, K, c2w, NEAR, FAR, occupancy=grid, march=step)
        outs[name] = out
        assert out['normal'].shape == (H, W, 3) and all(out[k].shape == (H, W) for k in ('z_normal', 'acc', 'depth'))
        ro, rd = rnh.get_rays(H, W, K, c2w)
        fg = out['acc'] > 0.5
        assert int(fg.sum()) > 20
        nrm = out['normal'][fg]
        assert bool(((nrm.norm(dim=-1) - 1).abs() < 1e-5).all())
        assert bool((out['z_normal'][fg] > 0).all()) and bool((out['z_normal'] <= 1).all())
        p = ro[fg] + rd[fg] * out['depth'][fg][:, None]
        cos = (nrm * p / p.norm(dim=-1, keepdim=True)).sum(-1)
        print(f"render_normals ({name}): {int(fg.sum())} pixels with acc > 0.5, cosine to the radial direction min {float(cos.min()):.4f}, "
              f"z_normal min {float(out['z_normal'][fg].min()):.4f}")
        assert bool((cos >= 0.9).all())
        ray_off = grid.march(ro.reshape(-1, 3), rd.reshape(-1, 3), NEAR, FAR, step)[0]
        empty = (ray_off[1:] == ray_off[:-1]).reshape(H, W)
        assert bool(empty.any()) and bool((out['normal'][empty] == 0).all()) and bool((out['z_normal'][empty] == 0).all())
        assert bool((out['acc'][empty] == 0).all())
    # the centre pixel looks at the pole: the world normal flips with the camera, z_normal does not
    c = (H // 2, W // 2)
    assert float(outs["front"]['normal'][c][2]) > 0.9 and float(outs["back"]['normal'][c][2]) < -0.9
    assert float(outs["front"]['z_normal'][c]) > 0.9 and float(outs["back"]['z_normal'][c]) > 0.9
    # rows: a tile of the same image
    tile = vr.render_normals(_BallField(), H, W, K, torch.tensor(C2W_FRONT, device=dev), NEAR, FAR, occupancy=grid, march=step, rows=(4, 9))
    assert all(torch.equal(tile[k], outs["front"][k][4:9]) for k in tile)


def test_render_normals_composition(dev):
    """With a HashGridField: the chain march -> density_gradient -> raw2outputs_packed -> per-sample normals assembled in torch with a
    float64 per-ray sum.  With b the weighted sum's bound per channel, |N - N64| <= |b|, and x / |x| moves by at most 2 |dx| / |x|, so the
    normals agree within 2 |b| / |N64| plus the roundings of the normalisation and of the dot with the camera axis (8 * 2^-24)."""
    from contexture_nerf_amd import _lib as L, run_nerf_helpers as rnh, volume_render as vr
    from contexture_nerf_amd.hashgrid import HashGridField
    torch.manual_seed(0)
    field = HashGridField(-1.0, 1.0, n_levels=4, n_features=2, log2_table=8, base_res=2, max_res=16).to(dev)
    with torch.no_grad():
        field.encoding.table.copy_(torch.randn(field.encoding.table.shape, generator=torch.Generator().manual_seed(1)) * 0.5)
        field.mlp.output_linear.bias[3] = 1.0
    grid = _ball_grid(dev)
    H = W = 16
    K = vr.pinhole(H, W)
    c2w = torch.tensor(C2W_FRONT, device=dev)
    step = float(grid.h[0]) / 2
    out = vr.render_normals(field, H, W, K, c2w, NEAR, FAR, occupancy=grid, march=step)
    again = vr.render_normals(field, H, W, K, c2w, NEAR, FAR, occupancy=grid, march=step)
    assert all(torch.equal(out[k], again[k]) for k in out)
    assert all(x.grad is None for x in field.parameters())
    ro, rd = rnh.get_rays(H, W, K, c2w)
    ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
    ray_off, ray_id, t, dt, pts = grid.march(ro, rd, NEAR, FAR, step)
    raw, g = field.density_gradient(pts, return_raw=True)
    _, _, acc, wts, depth = rnh.raw2outputs_packed(raw, t, dt, rd, ray_off)
    assert torch.equal(out['acc'].reshape(-1), acc) and torch.equal(out['depth'].reshape(-1), depth)
    n_i = -g / g.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    _, bnd = GR.weighted_sum_f64(wts.cpu().numpy(), n_i.cpu().numpy(), ray_off.cpu().numpy())
    N64 = torch.zeros(H * W, 3, dtype=torch.float64).index_add_(0, ray_id.cpu().long(), wts.cpu().double()[:, None] * n_i.cpu().double())
    len64 = N64.norm(dim=-1, keepdim=True)
    want = N64 / len64.clamp_min(1e-12)
    tol = 2 * torch.from_numpy(bnd).norm(dim=-1) / len64[:, 0].clamp_min(1e-12) + 8 * 2.0 ** -24
    hit = len64[:, 0] > 1e-6
    assert int(hit.sum()) > 20
    err = (out['normal'].reshape(-1, 3).cpu().double() - want).norm(dim=-1)
    print(f"render_normals composition: {int(hit.sum())} rays, worst error / tolerance {float((err[hit] / tol[hit]).max()):.3f}")
    assert bool((err[hit] <= tol[hit]).all())
    want_z = (want * c2w[:3, 2].cpu().double()).sum(-1).clamp(0, 1)
    assert bool(((out['z_normal'].reshape(-1).cpu().double() - want_z).abs()[hit] <= tol[hit]).all())
    # a field without density_gradient is refused; so is the dense path
    with pytest.raises(L.CtxError, match="density_gradient"):
        vr.render_normals(rnh.NeRF2D(D=8, W=256, input_ch=63, output_ch=4, skips=[4]).to(dev), H, W, K, c2w, NEAR, FAR, occupancy=grid,
                          march=step)
    with pytest.raises(L.CtxError, match="marched path only"):
        vr.render_normals(field, H, W, K, c2w, NEAR, FAR, occupancy=None, march=step)
