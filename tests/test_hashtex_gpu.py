"""GPU: the texture field's 2-D hash grid (csrc/hashtex.hip) against its rule, bit for bit, in the three ways to name the rows; the
pre-summed accumulate against the plain one; the head; HashGridTexture.texture_map's gradients against float64 autograd; a fit against the
CPU restatement's; and the field inside the product.  Definitions: tests/hashtex_rule.py, DESIGN section 4l."""
import ctypes as C
import functools
import os
import numpy as np
import pytest
import torch

import hashgrid_rule as HG
import hashtex_rule as HT

pytestmark = pytest.mark.gpu
f32 = np.float32


def _dev(dev, a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


def _res_ptr(res):
    r = np.ascontiguousarray(res, np.int32)
    return r, r.ctypes.data_as(C.c_void_p)


def _abi_fwd(dev, table, res, log2T, uv=None, idx=None, grid=0):
    from contexture_nerf_amd import _lib as L
    Lv, T, F = table.shape
    u, i, t = _dev(dev, uv, f32), _dev(dev, idx, np.int32), _dev(dev, table, f32)
    n = uv.shape[0] if uv is not None else (len(idx) if idx is not None else grid * grid)
    emb = torch.full((n, Lv * F), float('nan'), device=dev)
    _r, rp = _res_ptr(res)
    L.check(L.load().ctx_hashtex_fwd(L.ptr(u), L.ptr(i), n, grid, L.ptr(t), Lv, F, log2T, rp, L.ptr(emb), L.stream()))
    return emb.cpu().numpy()


def _abi_bwd(dev, g_emb, res, log2T, F, uv=None, idx=None, grid=0, ws=None):
    """-> g_table [Lv, T, F] as a device tensor; the buffer starts as NaN, the workspace as garbage (0xff)"""
    from contexture_nerf_amd import _lib as L
    lib = L.load()
    Lv = len(res)
    u, i, g = _dev(dev, uv, f32), _dev(dev, idx, np.int32), _dev(dev, g_emb, f32)
    out = torch.full((Lv, 1 << log2T, F), float('nan'), device=dev)
    if ws is None:
        ws = torch.full((lib.ctx_hashtex_bwd_ws_bytes(Lv, F, log2T),), 0xff, dtype=torch.uint8, device=dev)
    _r, rp = _res_ptr(res)
    L.check(lib.ctx_hashtex_bwd(L.ptr(u), L.ptr(i), g_emb.shape[0], grid, L.ptr(g), Lv, F, log2T, rp, 7, L.ptr(ws), L.ptr(out), L.stream()))
    return out


class _presum:
    """CTX_HASHTEX_PRESUM for the calls inside: the library reads it per call"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("CTX_HASHTEX_PRESUM")
        os.environ["CTX_HASHTEX_PRESUM"] = self.value

    def __exit__(self, *a):
        if self.old is None:
            del os.environ["CTX_HASHTEX_PRESUM"]
        else:
            os.environ["CTX_HASHTEX_PRESUM"] = self.old


# ---- 1. the kernels are the rule -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lv,F,log2T", HT.TABLE_CASES)
@pytest.mark.parametrize("max_res", HT.MAX_RES_CASES)
def test_kernels_equal_the_rule(dev, Lv, F, log2T, max_res):
    """Forward and backward, array_equal: dense and hashed levels in one table, T = 16 where almost everything collides; points on 0 and
    1, on nodes, outside, NaN and inf rows, n around the wave and block sizes; whole atlases (33^2 rows cross the workgroup size, an odd
    grid takes both halves of the linspace rule); shuffled texel lists with an entry outside the atlas."""
    res = HT.resolutions(Lv, 2, max_res)
    dense = [HT.is_dense(r, log2T) for r in res]
    if Lv > 1 and (Lv == 4 or max_res == 256):
        assert any(dense) and not all(dense)                                    # the mixed cases
    else:
        assert all(dense)               # up to 16 the floor of the finest level is 15: 16^2 nodes fit 2^8 entries exactly, the boundary
    table = HT.case_table(Lv, F, log2T, seed=Lv + F)
    cases = [("points", n, dict(uv=HT.case_points(n, res, seed=n))) for n in HT.N_CASES]
    cases += [("atlas", g, dict(grid=g)) for g in HT.GRID_CASES]
    cases += [("list", k, dict(idx=HT.case_list(33, k, seed=k), grid=33)) for k in HT.LIST_SIZES]
    for mode, size, rows in cases:
        got = _abi_fwd(dev, table, res, log2T, **rows)
        assert np.array_equal(got, HT.forward_np(table, res, log2T, **rows)), ("forward", mode, size)
        g_emb = np.random.default_rng(size).standard_normal((got.shape[0], Lv * F)).astype(f32) * f32(3e-3)
        gt = _abi_bwd(dev, g_emb, res, log2T, F, **rows).cpu().numpy()
        assert np.array_equal(gt, HT.backward_np(g_emb, res, log2T, F, **rows)), ("backward", mode, size)


def test_node_count_beyond_32_bits(dev):
    """res = 65535: the level has 65536^2 = 2^32 nodes, a count that is 0 in 32 bits.  The level is hashed; a kernel that took the
    wrapped count for a dense level would index the table unmasked.  Forward and table backward on uv rows, array_equal."""
    Lv, F, log2T, n, res = 1, 2, 12, 300, [65535]
    assert not HT.is_dense(res[0], log2T)
    table = HT.case_table(Lv, F, log2T, seed=5)
    uv = HT.case_points(n, res, seed=n)
    assert np.array_equal(_abi_fwd(dev, table, res, log2T, uv=uv), HT.forward_np(table, res, log2T, uv=uv))
    g_emb = np.random.default_rng(n).standard_normal((n, Lv * F)).astype(f32) * f32(3e-3)
    gt = _abi_bwd(dev, g_emb, res, log2T, F, uv=uv).cpu().numpy()
    assert np.array_equal(gt, HT.backward_np(g_emb, res, log2T, F, uv=uv))


def test_row_modes_are_exclusive(dev):
    """An inconsistent combination is refused before any launch: the output keeps its prefill."""
    from contexture_nerf_amd import _lib as L
    lib = L.load()
    res, rp = _res_ptr([2, 4])
    table = torch.zeros(2, 16, 2, device=dev)
    uv = torch.zeros(9, 2, device=dev)
    idx = torch.zeros(9, dtype=torch.int32, device=dev)
    emb = torch.full((9, 4), 7.0, device=dev)

    def call(uv_, idx_, n, grid, Lv=2, F=2, log2T=4):
        return lib.ctx_hashtex_fwd(L.ptr(uv_), L.ptr(idx_), n, grid, L.ptr(table), Lv, F, log2T, rp, L.ptr(emb), L.stream())
    for args in ((uv, idx, 9, 0), (uv, None, 9, 3), (uv, idx, 9, 3), (None, None, 9, 0), (None, idx, 9, 1), (None, None, 8, 3),
                 (None, None, 0, 3), (None, idx, 0, 3), (None, None, 9, 46341)):
        with pytest.raises(L.CtxError):
            L.check(call(*args))
    for kw in (dict(Lv=0), dict(Lv=17), dict(F=3), dict(log2T=3), dict(log2T=23)):
        with pytest.raises(L.CtxError):
            L.check(call(uv, None, 9, 0, **kw))
    torch.cuda.synchronize()
    assert bool((emb == 7.0).all())
    assert lib.ctx_hashtex_bwd_ws_bytes(2, 2, 4) >= 2 * 16 * 2 * 8 + 16
    for bad in ((0, 2, 4), (17, 2, 4), (2, 3, 4), (2, 2, 3), (2, 2, 23), (16, 8, 4)):
        assert lib.ctx_hashtex_bwd_ws_bytes(*bad) == -1
    L.check(call(None, None, 9, 3))
    L.check(call(None, idx, 9, 3))
    L.check(call(uv, None, 9, 0))


# ---- 2. backward special cases -------------------------------------------------------------------------------------------------------
def test_backward_contention_presum_zero_nan_and_repeat(dev):
    Lv, F, log2T = 4, 2, 6
    res = HT.resolutions(Lv, 2, 64)
    rng = np.random.default_rng(3)
    # one point a thousand times: all adds land on four entries per level, every wave is one run
    uv = np.tile(f32([[0.3, 0.7]]), (1000, 1))
    g_emb = rng.standard_normal((1000, Lv * F)).astype(f32)
    got = _abi_bwd(dev, g_emb, res, log2T, F, uv=uv)
    assert np.array_equal(got.cpu().numpy(), HT.backward_np(g_emb, res, log2T, F, uv=uv))
    assert all(np.count_nonzero(got[l].cpu().numpy().any(-1)) <= 4 for l in range(Lv)) and bool(got.any())
    with _presum("0"):
        assert torch.equal(_abi_bwd(dev, g_emb, res, log2T, F, uv=uv), got)
    # scales far from 1
    for scale in (1e-30, 1e20):
        gs = (g_emb * f32(scale)).astype(f32)
        assert np.array_equal(_abi_bwd(dev, gs, res, log2T, F, uv=uv).cpu().numpy(), HT.backward_np(gs, res, log2T, F, uv=uv))
    # the whole 33 x 33 atlas on a single level of res 2: four cells, whole waves on one entry - the pre-sum's case
    one = np.array([2], np.int32)
    ga = rng.standard_normal((33 * 33, 2)).astype(f32)
    want = HT.backward_np(ga, one, 4, 2, grid=33)
    with _presum("1"):
        a = _abi_bwd(dev, ga, one, 4, 2, grid=33)
    with _presum("0"):
        b = _abi_bwd(dev, ga, one, 4, 2, grid=33)
    assert np.array_equal(a.cpu().numpy(), want) and torch.equal(a, b) and np.count_nonzero(want.any(-1)) == 9
    # a list in atlas order with entries outside it inside the runs: a dead lane ends a run and adds nothing
    idx = np.arange(33 * 33, dtype=np.int32)
    idx[5::7] = -1
    idx[100:164] = 33 * 33
    gl = rng.standard_normal((33 * 33, 2)).astype(f32)
    gl[5] = np.nan                                                       # a dead row's NaN does not poison
    want = HT.backward_np(gl, one, 4, 2, idx=idx, grid=33)
    a = _abi_bwd(dev, gl, one, 4, 2, idx=idx, grid=33)
    with _presum("0"):
        b = _abi_bwd(dev, gl, one, 4, 2, idx=idx, grid=33)
    assert np.all(np.isfinite(want)) and np.array_equal(a.cpu().numpy(), want) and torch.equal(a, b)
    # all zero: zeros everywhere (the NaN prefill is gone); a NaN or an inf: NaN everywhere
    uv = HT.case_points(300, res, seed=1)
    g_emb = rng.standard_normal((300, Lv * F)).astype(f32)
    z = _abi_bwd(dev, np.zeros_like(g_emb), res, log2T, F, uv=uv)
    assert not bool(z.any()) and bool(torch.isfinite(z).all())
    for bad in (np.nan, np.inf):
        gb = g_emb.copy()
        gb[123, 5] = bad
        assert bool(torch.isnan(_abi_bwd(dev, gb, res, log2T, F, uv=uv)).all())
    # every element is written, five launches (one workspace, reused) and a side stream give the same bits
    from contexture_nerf_amd import _lib as L
    ws = torch.empty(L.load().ctx_hashtex_bwd_ws_bytes(Lv, F, log2T), dtype=torch.uint8, device=dev)
    runs = [_abi_bwd(dev, g_emb, res, log2T, F, uv=uv, ws=ws) for _ in range(5)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runs.append(_abi_bwd(dev, g_emb, res, log2T, F, uv=uv))
    side.synchronize()
    assert bool(torch.isfinite(runs[0]).all()) and all(torch.equal(runs[0], r) for r in runs[1:])
    assert np.array_equal(runs[0].cpu().numpy(), HT.backward_np(g_emb, res, log2T, F, uv=uv))


# ---- 3. the head -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", [1, 3, 4])
def test_head_forward_and_backward(dev, C_):
    """tex within 4 * 2^-24 of (tanh64(raw) + 1) / 2: ocml's tanhf is within OpenCL's 5 ulp, 5 * 2^-24 for a value of at most 1, then the
    add's rounding (2^-24 below 2), all halved exactly.  grad_raw within |gt| * 0.5 * 13 * 2^-24 + 2^-24 * |grad_raw| of float64: y off by
    5 * 2^-24, y*y by twice that and a rounding (11), 1 - y*y by one more (12), the product with gt * 0.5 (exact) by one more (13), and the
    add to g_raw_in by one of the result's."""
    from contexture_nerf_amd import _lib as L
    lib = L.load()
    plane, u = 33 * 33, 2.0 ** -24
    rng = np.random.default_rng(C_)
    for idx in (None, HT.case_list(33, 500, seed=2), HT.case_list(33, 1, seed=1, bad=False)):
        n = plane if idx is None else len(idx)
        raw = (rng.standard_normal((n, C_)) * 3).astype(f32)
        raw[0, 0] = 0.0
        raw[n // 2, C_ - 1] = 40.0
        r, i = _dev(dev, raw), _dev(dev, idx, np.int32)
        tex = torch.full((C_, plane), -7.0, device=dev)
        L.check(lib.ctx_texture_head_fwd(L.ptr(r), L.ptr(i), n, plane, C_, L.ptr(tex), L.stream()))
        want = HT.head_f64(raw, idx, plane, fill=-7.0)
        got = tex.cpu().numpy().astype(np.float64)
        node, live = HT.rows_nodes(n, idx, plane)
        listed = np.zeros(plane, bool)
        listed[node[live]] = True
        assert np.array_equal(got[:, ~listed], want[:, ~listed])                  # the listed nodes only are written
        err = np.abs(got - want)[:, listed].max()
        print(f"head C={C_} n={n}: max |tex - float64| = {err / u:.2f} * 2^-24")
        assert err <= 4 * u and got[:, listed].min() >= 0 and got[:, listed].max() <= 1
        gt = rng.standard_normal((C_, plane)).astype(f32)
        gt[:, ~listed] = np.nan                                                  # the listed nodes only are read
        for g_in in (None, rng.standard_normal((n, C_)).astype(f32)):
            out = torch.full((n, C_), float('nan'), device=dev)
            gt_d, g_in_d = _dev(dev, gt), _dev(dev, g_in)                        # held: a temporary's memory would be handed out again
            L.check(lib.ctx_texture_head_bwd(L.ptr(gt_d), L.ptr(g_in_d), L.ptr(r), L.ptr(i), n, plane, C_, L.ptr(out), L.stream()))
            gtz = np.where(listed, gt, 0)
            want_g = HT.head_bwd_f64(gtz, g_in, raw, idx, plane)
            bound = np.where(live[:, None], np.abs(gtz[:, node].T), 0) * 0.5 * 13 * u + u * np.abs(want_g) + 1e-44
            got_g = out.cpu().numpy().astype(np.float64)
            assert np.all(np.isfinite(got_g)) and np.all(np.abs(got_g - want_g) <= bound)
            if idx is not None and not live.all():
                dead = np.nonzero(~live)[0]
                assert np.array_equal(got_g[dead], np.zeros((len(dead), C_)) if g_in is None else g_in[dead].astype(np.float64))
    for bad in (dict(C=0), dict(C=5), dict(n=5)):                                # refused before a launch
        with pytest.raises(L.CtxError):
            L.check(lib.ctx_texture_head_fwd(L.ptr(r), None, bad.get('n', plane), plane, bad.get('C', C_), L.ptr(tex), L.stream()))


# ---- 4. HashGridTexture.texture_map ------------------------------------------------------------------------------------------------
GRAD = dict(res=16, Lv=4, F=2, log2T=6, D=2, W=64, C=3)


@functools.lru_cache(maxsize=None)
def _texture_reference():
    """Table, MLP, texel list and upstream gradients, and per dtype the restatement's (tex, raw, gradients) for the whole atlas and the list"""
    c = GRAD
    res = HT.resolutions(c['Lv'], 2, c['res'])
    rng = np.random.default_rng(21)
    table = (rng.standard_normal((c['Lv'], 1 << c['log2T'], c['F'])) * 0.5).astype(f32)
    params = HG.make_params(c['D'], c['W'], c['Lv'] * c['F'], c['C'], 0, seed=21)
    texels = rng.permutation(c['res'] ** 2)[:100].astype(np.int32)
    g_tex = rng.standard_normal((c['C'], c['res'] ** 2)).astype(f32)
    g_raw = {None: rng.standard_normal((c['res'] ** 2, c['C'])).astype(f32), 'list': rng.standard_normal((100, c['C'])).astype(f32)}
    ref = {}
    for dtype in (torch.float64, torch.float32):
        for key, idx in ((None, None), ('list', texels)):
            t = torch.from_numpy(table).to(dtype).requires_grad_(True)
            ps = [p.clone().to(dtype).requires_grad_(True) for p in params]
            tex, raw = HT.texture_torch(t, ps, res, c['log2T'], c['res'], idx)
            ((tex * torch.from_numpy(g_tex).to(dtype)).sum() + (raw * torch.from_numpy(g_raw[key]).to(dtype)).sum()).backward()
            ref[dtype, key] = (tex.detach(), raw.detach(), [t.grad] + [p.grad for p in ps])
    return table, params, texels, g_tex, g_raw, ref


def _make_field(dev, table, params, **kw):
    from contexture_nerf_amd.hashgrid import HashGridTexture
    field = HashGridTexture(**kw).to(dev)
    with torch.no_grad():
        field.encoding.table.copy_(torch.from_numpy(np.asarray(table)))
        for p, v in zip(field.mlp._params(), params):
            p.copy_(v)
    return field


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def test_texture_map_gradients_vs_float64(dev):
    """The table and the six MLP tensors against float64 CPU autograd through the restatement: relative L2 at most 4 x that of the float32
    CPU autograd run of the same restatement (the bar of DESIGN section 4k: the factor covers a different summation order along the
    chain).  Listed texels carry the bits of the whole-atlas call; the no-grad atlas is cached until a parameter moves."""
    c = GRAD
    table, params, texels, g_tex, g_raw, ref = _texture_reference()
    field = _make_field(dev, table, params, n_levels=c['Lv'], n_features=c['F'], log2_table=c['log2T'], base_res=2, max_res=c['res'],
                        D=c['D'], W=c['W'], output_ch=c['C'])
    assert np.array_equal(field.encoding.res, HT.resolutions(c['Lv'], 2, c['res']))
    tl = torch.from_numpy(texels).to(dev)
    outs = {}
    names = ["table"] + [f"{k}{i}" for i in range(c['D'] + 1) for k in "wb"]
    for key, idx in ((None, None), ('list', tl)):
        field.zero_grad(set_to_none=True)
        tex, raw = field.texture_map(c['res'], texels=idx)
        assert tex.shape == (1, c['C'], c['res'], c['res']) and raw.shape == (g_raw[key].shape[0], c['C'])
        ((tex.reshape(c['C'], -1) * torch.from_numpy(g_tex).to(dev)).sum() + (raw * torch.from_numpy(g_raw[key]).to(dev)).sum()).backward()
        outs[key] = (tex.detach(), raw.detach())
        w_tex, w_raw, w_grads = ref[torch.float64, key]
        np.testing.assert_allclose(tex.detach().reshape(c['C'], -1).cpu().numpy(), w_tex.numpy(), rtol=0, atol=2e-5)
        np.testing.assert_allclose(raw.detach().cpu().numpy(), w_raw.numpy(), rtol=1e-4, atol=2e-5)
        grads = [field.encoding.table.grad] + [p.grad for p in field.mlp._params()]
        fails = []
        for name, g, w, w32 in zip(names, grads, w_grads, ref[torch.float32, key][2]):
            got, cpu32 = _rel(g.cpu(), w), _rel(w32, w)
            print(f"texture_map {'atlas' if key is None else 'list'} grad {name}: relative L2 to float64 {got:.3e} (float32 CPU autograd {cpu32:.3e})")
            if not got <= 4 * cpu32:
                fails.append((name, got, cpu32))
        assert not fails, fails
    # listed texels carry the bits of the whole-atlas call; off the list the texture is zero
    (tex_a, raw_a), (tex_l, raw_l) = outs[None], outs['list']
    flat_a, flat_l = tex_a.reshape(c['C'], -1), tex_l.reshape(c['C'], -1)
    assert torch.equal(flat_l[:, tl.long()], flat_a[:, tl.long()]) and torch.equal(raw_l, raw_a[tl.long()])
    off = torch.ones(c['res'] ** 2, dtype=torch.bool, device=dev)
    off[tl.long()] = False
    assert not bool(flat_l[:, off].any())
    # without grad: the same bits, and the same tensors until a step moves a parameter
    with torch.no_grad():
        t1, r1 = field.texture_map(c['res'])
        t2, r2 = field.texture_map(c['res'])
        assert t1 is t2 and r1 is r2 and torch.equal(t1, tex_a) and torch.equal(r1, raw_a)
        tl1, rl1 = field.texture_map(c['res'], texels=tl)
        assert torch.equal(tl1, tex_l) and torch.equal(rl1, raw_l)
        assert torch.equal(field.forward_uv(torch.from_numpy(HT.node_uv(c['res'], np.arange(c['res'] ** 2))).to(dev)), raw_a)
    opt = torch.optim.SGD(field.parameters(), lr=1e-3)
    opt.step()
    with torch.no_grad():
        t3, _ = field.texture_map(c['res'])
        assert t3 is not t1 and not torch.equal(t3, t1)
    # the list checks are NeRF2D's
    from contexture_nerf_amd import _lib as L
    for bad, msg in ((torch.zeros(0, dtype=torch.int32, device=dev), "empty"), (torch.tensor([0, 256], dtype=torch.int32, device=dev), "outside"),
                     (torch.tensor([-1], dtype=torch.int32, device=dev), "outside"), (torch.zeros(2, 2, dtype=torch.int32, device=dev), "1-D"),
                     (torch.zeros(3, dtype=torch.int64, device=dev), "dtype")):
        with pytest.raises(L.CtxError, match=msg):
            field.texture_map(c['res'], texels=bad)
    with pytest.raises(L.CtxError, match="no gradient with respect to uv"):
        field.forward_uv(torch.zeros(4, 2, device=dev, requires_grad=True))
    assert field.forward_uv(torch.zeros(0, 2, device=dev)).shape == (0, c['C'])
    assert field.encoding(torch.zeros(3, 0, 2, device=dev)).shape == (3, 0, c['Lv'] * c['F'])


# ---- 5. the fit ------------------------------------------------------------------------------------------------------------------------
def _fit_on_device(dev):
    c = HT.FIT
    table, params = HT.fit_initial()
    field = _make_field(dev, table, params, n_levels=c['Lv'], n_features=c['F'], log2_table=c['log2T'], base_res=c['base_res'],
                        max_res=c['max_res'], D=c['D'], W=c['W'], output_ch=c['C'])
    target = torch.from_numpy(HT.fit_target(c['grid'])).to(dev).reshape(1, c['C'], c['grid'], c['grid'])
    opt = HT.fit_optimizer(field.encoding.table, field.mlp._params())
    hist = []
    for _ in range(c['iters']):
        opt.zero_grad()
        tex, _ = field.texture_map(c['grid'])
        loss = ((tex - target) ** 2).mean()
        loss.backward()
        opt.step()
        hist.append(loss.detach())
    return field, torch.stack(hist)


def test_fit_matches_the_restatement_and_repeats(dev):
    """The schedule fixed in tests/test_hashtex_cpu.py: the device's mean loss over the last five iterations is at most 1.5 x the float64
    CPU restatement's (the margin covers float32 against float64 over 60 steps), and two runs are equal bit for bit."""
    import test_hashtex_cpu as TC
    h = TC.fit_history()
    cpu_first, cpu_last = float(np.mean(h[:5])), float(np.mean(h[-5:]))
    fa, ha = _fit_on_device(dev)
    fb, hb = _fit_on_device(dev)
    gpu = ha.cpu().numpy().astype(np.float64)
    gpu_first, gpu_last = float(gpu[:5].mean()), float(gpu[-5:].mean())
    print(f"fit: last-five mean loss on the device {gpu_last:.6e}, CPU float64 restatement {cpu_last:.6e} (first five: {gpu_first:.5f} / {cpu_first:.5f})")
    assert np.all(np.isfinite(gpu)) and gpu_last <= 1.5 * cpu_last
    assert torch.equal(ha, hb) and all(torch.equal(a, b) for a, b in zip(fa.parameters(), fb.parameters()))
    assert len(list(fa.parameters())) == 7


# ---- 6. the product ------------------------------------------------------------------------------------------------------------------
def _tiny_trainer(dev, tmp_path, **over):
    import test_pipeline_gpu as TP
    from contexture_nerf_amd import config as CFG
    from contexture_nerf_amd.trainer import ConTEXTure
    cfg = CFG.TrainConfig()
    cfg.guide.text = "a test mesh"; cfg.guide.shape_path = "shapes/spot_triangulated.obj"
    cfg.guide.texture_resolution = 128; cfg.guide.sd_image_size = 128; cfg.guide.num_inference_steps = 2
    cfg.render.train_grid_size = 192
    cfg.log.exp_root = tmp_path; cfg.log.exp_name = "hashtex"
    cfg.guide.hashgrid_levels = 6; cfg.guide.hashgrid_log2_table = 10
    for k, v in over.items():
        sect, name = k.split('__')
        setattr(getattr(cfg, sect), name, v)
    sd, _, _ = TP._tiny_sd(dev)
    tr = ConTEXTure(CFG.validate(cfg), device=dev, diffusion=sd)
    TP._tiny_zero123(dev, tr)
    return tr


def _render_shapes(tr):
    v = tr.train_views[1]
    with torch.no_grad():
        out = tr.mesh_model.render(theta=v['theta'], phi=tr._offset_phi(v['phi']), radius=float(v['radius']),
                                   background=torch.tensor([0.5, 0.5, 0.5], device=tr.device))
    return {k: (tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__) for k, x in out.items()}


@pytest.mark.parametrize("field_texels", ["all", "active"])
def test_product_paints_with_the_hashgrid_field(dev, tmp_path, field_texels):
    from contexture_nerf_amd.hashgrid import HashGridTexture
    tr = _tiny_trainer(dev, tmp_path, guide__texture_field='hashgrid', optim__field_texels=field_texels)
    field = tr.texture_mlp
    assert isinstance(field, HashGridTexture) and field.encoding.table.shape == (6, 1024, 2) and int(field.encoding.res[-1]) in (127, 128)
    table0 = field.encoding.table.detach().clone()
    mlp0 = [p.detach().clone() for p in field.mlp.parameters()]
    log = tr.paint_zero123plus(iterations=2, tile=64)
    assert [r['i'] for r in log] == [0, 1]
    assert all(np.isfinite(r['loss']) and np.isfinite(r['grad_norm']) and r['grad_norm'] > 0 for r in log)
    assert tr._sds_setup['field_texels'] == field_texels
    assert not torch.equal(table0, field.encoding.table.detach())
    assert any(not torch.equal(a, b.detach()) for a, b in zip(mlp0, field.mlp.parameters()))
    assert bool(torch.isfinite(field.encoding.table).all())
    if field_texels == "all":
        shapes = _render_shapes(tr)
        assert len(shapes) == 9
        mesh_dir = tr.cfg.log.exp_dir / 'mesh'                                    # the export of full_eval: no view was projected back here
        tr.export(mesh_dir) if getattr(tr, 'atlas', None) is not None else tr.mesh_model.export_mesh(str(mesh_dir))
        assert os.path.getsize(mesh_dir / 'albedo.png') > 0
        ref = _tiny_trainer(dev, tmp_path)                                       # the default config: the field is the MLP, same render
        from contexture_nerf_amd.run_nerf_helpers import NeRF2D
        assert isinstance(ref.texture_mlp, NeRF2D) and ref.cfg.guide.texture_field == 'mlp'
        assert _render_shapes(ref) == shapes
