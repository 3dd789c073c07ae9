"""GPU: the texture field on the texels the views sample — ctx_texel_active_mark / ctx_texel_compact against the numpy restatement of
tests/test_field_texels_cpu.py, the index-list mode of the field kernels (ctx_uvmlp_fwd_save_idx / ctx_uvmlp_bwd_idx) against the dense
path's bits and the float64 oracle, and the host layers above them (NeRF2D.texture_map(texels=), TexturedMeshModel.render with a list in
the cache, the SDS loop with optim.field_texels = 'active').

Tolerances.  Forward: bit equality (an MFMA row does not depend on its tile slot; the coordinates come from the grid mode's expression).
Parameter gradients against the dense path: 6e-5 of the dense tensor's largest entry — the two differ in summation grouping only (twice
the 3e-5 at which test_texture_field_backward_vs_oracle holds this kernel to float64 on uv lists); against the float64 oracle: the 2e-4
of test_texture_map_backward_and_fit (the device linspace's 1-ulp nodes, which both paths share)."""
import ctypes as C
import os
import numpy as np
import pytest
import torch

from oracle import nerf as onerf
from test_field_texels_cpu import active_texels_np, spot_raster
from test_geometry_gpu import _field_grads, _close

pytestmark = pytest.mark.gpu
DENSE_REL = 6e-5
ORACLE_REL = 2e-4


def _net(dev, W, seed=3, input_ch=42, output_ch=3):
    from contexture_nerf_amd import run_nerf_helpers as rnh
    torch.manual_seed(seed + W)
    return rnh.NeRF2D(D=8, W=W, input_ch=input_ch, output_ch=output_ch, skips=[4]).to(dev)


def _close_to_dense(got, dense, what):
    err = float((got - dense).abs().max()); scale = float(dense.abs().max())
    print(f"{what}: max |active - dense| {err:.3e}, max |dense| {scale:.3e}, ratio {err / max(scale, 1e-30):.2e}")
    assert err <= DENSE_REL * scale, f"{what}: {err:.3e} > {DENSE_REL} x {scale:.3e}"


# ---- mark and compact -----------------------------------------------------------------------------------------------------------
def _synthetic_raster(B, H, W, seed):
    """uv in [0, 1] with exact zeros and ones (the clamp makes x1 = T), NaN on the background; for B > 1 the last view is all background."""
    rng = np.random.default_rng(seed)
    uv = rng.random((B, H, W, 2)).astype(np.float32)
    edge = rng.random((B, H, W, 2))
    uv[edge < 0.05] = 0.0
    uv[edge > 0.95] = 1.0
    fi = rng.integers(-1, 5, (B, H, W)).astype(np.int64)
    fi[:, : H // 3] = -1
    if B > 1:
        fi[-1] = -1
    uv[fi < 0] = np.nan
    return uv, fi


@pytest.mark.parametrize("T", [64, 257])
@pytest.mark.parametrize("B,H,W", [(1, 37, 53), (3, 64, 64)])
def test_mark_and_compact_vs_restatement(dev, T, B, H, W):
    from contexture_nerf_amd import kal
    uv, fi = _synthetic_raster(B, H, W, seed=T + B)
    want, want_mask = active_texels_np(uv, fi, T)
    assert 0 < len(want) < T * T
    d_uv, d_fi = torch.tensor(uv, device=dev), torch.tensor(fi, device=dev)
    idx, mask = kal.active_texels(d_uv, d_fi, T)
    assert idx.dtype == torch.int32 and mask.dtype == torch.uint8
    assert np.array_equal(mask.cpu().numpy(), want_mask) and np.array_equal(idx.cpu().numpy(), want)
    # two calls into one mask: the union (of this raster and a second one)
    uv2, fi2 = _synthetic_raster(B, H, W, seed=1000 + T)
    both_want, _ = active_texels_np(uv2, fi2, T, want_mask.copy())
    both, mask2 = kal.active_texels(torch.tensor(uv2, device=dev), torch.tensor(fi2, device=dev), T, mask=mask)
    assert mask2 is mask and np.array_equal(both.cpu().numpy(), both_want) and len(both_want) >= len(want)
    # nothing foreground: count = 0
    none, m0 = kal.active_texels(d_uv, torch.full_like(d_fi, -1), T)
    assert none.numel() == 0 and none.dtype == torch.int32 and not bool(m0.any())
    # the same bits from a side stream
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        idx_s, mask_s = kal.active_texels(d_uv, d_fi, T)
    s.synchronize()
    assert torch.equal(idx_s, idx) and np.array_equal(mask_s.cpu().numpy(), want_mask)


def test_mark_and_compact_refusals(dev):
    from contexture_nerf_amd import _lib as L, kal
    lib = L.load()
    uv = torch.zeros(1, 4, 4, 2, device=dev); fi = torch.zeros(1, 4, 4, dtype=torch.int64, device=dev)
    mask = torch.zeros(8, 8, dtype=torch.uint8, device=dev)
    idx = torch.zeros(64, dtype=torch.int32, device=dev); cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.zeros(lib.ctx_texel_compact_ws_bytes(64), dtype=torch.uint8, device=dev)
    assert lib.ctx_texel_active_mark(None, L.ptr(fi), 1, 4, 4, 8, L.ptr(mask), L.stream()) != 0
    assert lib.ctx_texel_active_mark(L.ptr(uv), L.ptr(fi), 1, 4, 4, 8, None, L.stream()) != 0
    assert lib.ctx_texel_active_mark(L.ptr(uv), L.ptr(fi), 1, 4, 4, 1, L.ptr(mask), L.stream()) != 0          # T < 2
    assert lib.ctx_texel_compact_ws_bytes(0) == -1 and lib.ctx_texel_compact_ws_bytes(1 << 31) == -1
    assert lib.ctx_texel_compact(None, 64, L.ptr(idx), L.ptr(cnt), L.ptr(ws), L.stream()) != 0
    assert lib.ctx_texel_compact(L.ptr(mask), 64, L.ptr(idx), None, L.ptr(ws), L.stream()) != 0
    assert lib.ctx_texel_compact(L.ptr(mask), 1 << 31, L.ptr(idx), L.ptr(cnt), L.ptr(ws), L.stream()) != 0    # beyond one grid of int32 indices
    assert b"texel_compact" in lib.ctx_last_error()
    with pytest.raises(L.CtxError, match="dtype"):
        kal.active_texels(uv, fi.int(), 8)
    with pytest.raises(L.CtxError, match="face_idx"):
        kal.active_texels(uv, fi[:, :2], 8)
    torch.cuda.synchronize()
    assert not bool(mask.any()) and not bool(idx.any())                                                        # refused before any launch


# ---- index-list forward ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def raster(meshes):
    return spot_raster(meshes)                     # the oracle raster of two spot poses at 96 x 80, made once


def _lists(res, raster, dev):
    """name -> sorted int32 device list of distinct nodes of the res x res grid.  4 133 texels need res^2 >= 4 133: at res = 48 (2 304
    nodes) that list is 2 303 texels, one short of the whole grid."""
    n = res * res
    out = {'single': np.array([n // 2 + 7])}
    for k in (63, 65, 4133 if n >= 4133 else n - 1):
        out[f'random{k}'] = np.sort(np.random.default_rng(k).choice(n, k, replace=False))
    out['n%7<3'] = np.flatnonzero(np.arange(n) % 7 < 3)
    uv, fi = raster
    out['raster'] = active_texels_np(uv, fi, res)[0]
    assert 64 < len(out['raster']) < n
    return {k: torch.tensor(v.astype(np.int32), device=dev) for k, v in out.items()}


def _assert_listed_bits(net, res, idx, dense_tex, dense_raw, what):
    tex, raw = net.texture_map(res, texels=idx)
    li = idx.long()
    assert tuple(tex.shape) == (1, 3, res, res) and tuple(raw.shape) == (idx.numel(), 3), what
    assert torch.equal(raw, dense_raw[li]), f"{what}: raw differs from the dense rows"
    flat, dflat = tex.reshape(3, -1), dense_tex.reshape(3, -1)
    assert torch.equal(flat[:, li], dflat[:, li]), f"{what}: atlas differs at listed texels"
    off = torch.ones(res * res, dtype=torch.bool, device=idx.device); off[li] = False
    assert not bool(flat[:, off].any()), f"{what}: atlas written off the list"


@pytest.mark.parametrize("res", [48, 65])
@pytest.mark.parametrize("W", [64, 128, 256])
def test_index_forward_bits(dev, raster, W, res):
    net = _net(dev, W)
    lists = _lists(res, raster, dev)
    with torch.no_grad():
        dense_tex, dense_raw = net.texture_map(res)
        for name, idx in lists.items():
            _assert_listed_bits(net, res, idx, dense_tex, dense_raw, f"W={W} res={res} {name}")
    # the training forward (activations saved) writes the same outputs
    tex, raw = net.texture_map(res, texels=lists['raster'])
    assert tex.requires_grad and raw.requires_grad
    assert torch.equal(raw.detach(), dense_raw[lists['raster'].long()])
    if W == 256:                                                       # the default ran on the split-fp16 kernel; the exact-f32 one holds it too
        os.environ["CTX_UVMLP_EXACT_F32"] = "1"
        try:
            with torch.no_grad():
                net._tex_cache = None
                e_tex, e_raw = net.texture_map(res)
                assert not torch.equal(e_raw, dense_raw)               # really the other kernel
                for name, idx in lists.items():
                    _assert_listed_bits(net, res, idx, e_tex, e_raw, f"exact-f32 res={res} {name}")
        finally:
            os.environ.pop("CTX_UVMLP_EXACT_F32")
            net._tex_cache = None


def _loss_grads(net, res, idx, c_tex, c_raw):
    """autograd through texture_map: loss = <tex, c_tex> + <raw, c_raw> -> (tex, raw, 18 gradient tensors)."""
    net.zero_grad(set_to_none=True)
    tex, raw = net.texture_map(res) if idx is None else net.texture_map(res, texels=idx)
    ((tex * c_tex).sum() + (raw * c_raw).sum()).backward()
    gw, gb = _field_grads(net)
    return tex.detach(), raw.detach(), [g.clone() for g in gw + gb]


def test_identity_list_is_the_dense_path(dev):
    res = 48
    net = _net(dev, 256)
    g = torch.Generator().manual_seed(9)
    c_tex = torch.randn(1, 3, res, res, generator=g).to(dev)
    c_raw = (torch.randn(res * res, 3, generator=g) * 0.1).to(dev)
    d_tex, d_raw, d_g = _loss_grads(net, res, None, c_tex, c_raw)
    idx = torch.arange(res * res, dtype=torch.int32, device=dev)
    a_tex, a_raw, a_g = _loss_grads(net, res, idx, c_tex, c_raw)
    assert torch.equal(a_tex, d_tex) and torch.equal(a_raw, d_raw)
    assert len(a_g) == 18 and all(torch.equal(a, d) for a, d in zip(a_g, d_g))


# ---- index-list backward --------------------------------------------------------------------------------------------------------
def _bwd_abi_idx(net, idx, res, c_raw, c_tex):
    """training forward + backward of the list straight through the C-ABI -> (gws, gbs, saved activations [D,N,W])."""
    from contexture_nerf_amd import _lib as L
    lib = L.load()
    dev = idx.device
    N, D, W = idx.numel(), net.D, net.W
    blob = net.packed()
    raw = torch.empty(N, 3, device=dev)
    saved = torch.zeros(lib.ctx_uvmlp_saved_bytes(N, D, W, net.input_ch) // 4, device=dev)
    L.check(lib.ctx_uvmlp_fwd_save_idx(L.ptr(idx), N, res, L.ptr(blob), D, W, net.multires, 3, 4, L.ptr(raw), None, L.ptr(saved), L.stream()))
    ws_bytes, guard = lib.ctx_uvmlp_bwd_ws_bytes(N, D, W), 1 << 20
    ws = torch.full((ws_bytes + guard,), 0xA5, dtype=torch.uint8, device=dev)
    layers = list(net.pts_linears) + [net.output_linear]
    gws = [torch.empty_like(l.weight) for l in layers]
    gbs = [torch.empty_like(l.bias) for l in layers]
    gwp = (C.c_void_p * (D + 1))(*[L.ptr(t).value for t in gws])
    gbp = (C.c_void_p * (D + 1))(*[L.ptr(t).value for t in gbs])
    L.check(lib.ctx_uvmlp_bwd_idx(L.ptr(c_raw), L.ptr(c_tex), L.ptr(idx), res, L.ptr(raw), N, L.ptr(blob), D, W, net.multires, 3, 4,
                                  L.ptr(saved), L.ptr(ws), gwp, gbp, L.stream()))
    assert bool((ws[ws_bytes:] == 0xA5).all()), "the backward wrote past ctx_uvmlp_bwd_ws_bytes(len(idx))"
    return gws, gbs, saved[N * 48:N * 48 + D * N * W].reshape(D, N, W)


@pytest.mark.parametrize("W,res", [(256, 48), (64, 65), (128, 48)])
def test_index_backward_vs_oracle_and_dense(dev, raster, W, res):
    net = _net(dev, W)
    idx = _lists(res, raster, dev)['raster']
    li, n = idx.long(), idx.numel()
    g = torch.Generator().manual_seed(11 + res)
    c_tex = torch.zeros(3, res * res)
    c_tex[:, li.cpu()] = torch.randn(3, n, generator=g)                  # zero off the list, as texture_mapping's backward leaves it
    c_raw = torch.randn(n, 3, generator=g) * 0.1
    c_tex_d, c_raw_d = c_tex.reshape(1, 3, res, res).to(dev), c_raw.to(dev)
    _, _, a_g = _loss_grads(net, res, idx, c_tex_d, c_raw_d)
    # the C-ABI call gives the same bits, and so does a repeat
    hw, hb, acts = _bwd_abi_idx(net, idx, res, c_raw_d, c_tex.contiguous().to(dev))
    assert all(torch.equal(a, b) for a, b in zip(a_g, hw + hb)), "autograd seam != C-ABI"
    _, _, r_g = _loss_grads(net, res, idx, c_tex_d, c_raw_d)
    assert all(torch.equal(a, b) for a, b in zip(a_g, r_g)), "a repeat changed the gradients"
    # float64 oracle on the listed nodes, ReLU pattern from the saved activations
    acts = acts.cpu().numpy()
    ws = [l.weight.detach().cpu().numpy() for l in net.pts_linears]
    bs = [l.bias.detach().cpu().numpy() for l in net.pts_linears]
    e = onerf.embed(onerf.uv_grid(res))[li.cpu().numpy()]
    gws, gbs = onerf.nerf2d_backward(e, ws, bs, net.output_linear.weight.detach().cpu().numpy(), net.output_linear.bias.detach().cpu().numpy(),
                                     grad_raw=c_raw.numpy(), grad_tex=c_tex[:, li.cpu()].T.numpy(), masks=[acts[i] > 0 for i in range(8)])
    for i in range(9):
        _close(a_g[i], gws[i], ORACLE_REL, f'W={W} res={res} gw{i}')
        _close(a_g[9 + i], gbs[i], ORACLE_REL, f'W={W} res={res} gb{i}')
    # the dense path on the same inputs (grad_raw scattered to the listed rows, zero elsewhere): summation grouping only
    c_raw_full = torch.zeros(res * res, 3, device=dev); c_raw_full[li] = c_raw_d
    _, _, d_g = _loss_grads(net, res, None, c_tex_d, c_raw_full)
    for i, (a, d) in enumerate(zip(a_g, d_g)):
        _close_to_dense(a, d, f'W={W} res={res} ' + (f'gw{i}' if i < 9 else f'gb{i - 9}'))


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_index_entry_refusals(dev):
    from contexture_nerf_amd import _lib as L, run_nerf_helpers as rnh
    lib = L.load()
    net = _net(dev, 64)
    res = 8
    blob = net.packed()
    idx = torch.arange(10, dtype=torch.int32, device=dev)
    raw = torch.full((res * res + 1, 3), 7.0, device=dev)
    fwd = lambda p_idx, N, r: lib.ctx_uvmlp_fwd_save_idx(p_idx, N, r, L.ptr(blob), 8, 64, 10, 3, 4, L.ptr(raw), None, None, L.stream())
    assert fwd(None, 10, res) != 0 and b"null texel list" in lib.ctx_last_error()
    assert fwd(L.ptr(idx), 0, res) != 0
    assert fwd(L.ptr(idx), res * res + 1, res) != 0
    assert fwd(L.ptr(idx), 10, 1) != 0
    saved = torch.zeros(lib.ctx_uvmlp_saved_bytes(10, 8, 64, 42), dtype=torch.uint8, device=dev)
    ws = torch.zeros(lib.ctx_uvmlp_bwd_ws_bytes(10, 8, 64), dtype=torch.uint8, device=dev)
    layers = list(net.pts_linears) + [net.output_linear]
    gws = [torch.full_like(l.weight, 7.0) for l in layers]; gbs = [torch.full_like(l.bias, 7.0) for l in layers]
    gwp = (C.c_void_p * 9)(*[L.ptr(t).value for t in gws]); gbp = (C.c_void_p * 9)(*[L.ptr(t).value for t in gbs])
    bwd = lambda p_idx, N, r: lib.ctx_uvmlp_bwd_idx(L.ptr(raw), None, p_idx, r, L.ptr(raw), N, L.ptr(blob), 8, 64, 10, 3, 4, L.ptr(saved),
                                                    L.ptr(ws), gwp, gbp, L.stream())
    assert bwd(None, 10, res) != 0 and bwd(L.ptr(idx), 0, res) != 0 and bwd(L.ptr(idx), res * res + 1, res) != 0
    torch.cuda.synchronize()
    assert bool((raw == 7.0).all()) and all(bool((t == 7.0).all()) for t in gws + gbs)            # refused before any launch
    # the host wrapper: a host tensor, another dtype, an empty list, entries outside the atlas, the 3-D field
    with pytest.raises(L.CtxError, match="device tensor"):
        net.texture_map(res, texels=idx.cpu())
    with pytest.raises(L.CtxError, match="dtype"):
        net.texture_map(res, texels=idx.long())
    with pytest.raises(L.CtxError, match="empty"):
        net.texture_map(res, texels=idx[:0])
    with pytest.raises(L.CtxError, match="outside"):
        net.texture_map(res, texels=torch.tensor([0, res * res], dtype=torch.int32, device=dev))
    with pytest.raises(L.CtxError, match="outside"):
        net.texture_map(res, texels=torch.tensor([-1, 3], dtype=torch.int32, device=dev))
    field3 = _net(dev, 64, input_ch=63, output_ch=4)
    with pytest.raises(L.CtxError, match="dims=3"):
        field3.texture_map(res, texels=idx)


# ---- host layers on tiny engines ------------------------------------------------------------------------------------------------
def _trainer(dev, T, grid, **optim):
    from contexture_nerf_amd import config as CFG
    from contexture_nerf_amd.trainer import ConTEXTure
    from test_pipeline_gpu import _tiny_sd
    cfg = CFG.TrainConfig()
    cfg.guide.text = "a test mesh"; cfg.guide.shape_path = "shapes/spot_triangulated.obj"
    cfg.guide.texture_resolution = T; cfg.guide.sd_image_size = 128; cfg.guide.num_inference_steps = 2
    cfg.render.train_grid_size = grid; cfg.render.eval_grid_size = 96
    for k, v in optim.items():
        setattr(cfg.optim, k, v)
    sd, _, _ = _tiny_sd(dev)
    return ConTEXTure(cfg, device=dev, diffusion=sd)


def test_render_with_the_list_in_its_cache(dev):
    from contexture_nerf_amd import kal
    T = 64
    tr = _trainer(dev, T, 64)
    mm = tr.mesh_model
    mm.train()
    gray = torch.tensor([0.5, 0.5, 0.5], device=dev)
    views = tr.train_views[:3]
    with torch.no_grad():
        rc = mm.render(theta=[v['theta'] for v in views], phi=[tr._offset_phi(v['phi']) for v in views],
                       radius=[float(v['radius']) for v in views], background=gray)['render_cache']
    assert rc['face_idx'].shape == (3, 64, 64) and 'active_texels' not in rc
    idx, _ = kal.active_texels(rc['uv_features'].contiguous(), rc['face_idx'].contiguous(), T)
    assert 0 < idx.numel() < T * T
    params = list(tr.texture_mlp.parameters())

    def run(cache):
        for p in params:
            p.grad = None
        out = mm.render(render_cache=cache, background=gray)
        out['image'].sum().backward()
        return out, [p.grad.clone() for p in params]
    dense, d_g = run(rc)
    active, a_g = run(dict(rc, active_texels=idx))
    assert torch.equal(active['image'], dense['image']) and torch.equal(active['foreground'], dense['foreground'])
    assert active['render_cache']['active_texels'] is idx and 'active_texels' not in dense['render_cache']
    assert tuple(active['mlp_output'].shape) == (idx.numel(), 3) and tuple(dense['mlp_output'].shape) == (T * T, 3)
    for (name, _), a, d in zip(tr.texture_mlp.named_parameters(), a_g, d_g):
        _close_to_dense(a, d, f'render {name}')


def test_sds_loop_on_the_active_texels(dev):
    from test_pipeline_gpu import _tiny_zero123

    def run(mode):
        tr = _trainer(dev, 128, 192, field_texels=mode)
        _tiny_zero123(dev, tr)
        grads = []

        def keep(rec):
            if rec['i'] == 0:
                grads.extend(p.grad.detach().clone() for p in tr.texture_mlp.parameters())
        torch.manual_seed(1234)
        log = tr.paint_zero123plus(iterations=2, tile=64, on_iteration=keep)
        return tr, log, grads
    tr_d, log_d, g_d = run('all')
    tr_a, log_a, g_a = run('active')
    assert len(log_d) == len(log_a) == 2 and all(np.isfinite(r['loss']) for r in log_a)
    assert log_a[0]['loss'] == log_d[0]['loss']                                  # the rendered views keep their bits
    assert len(g_a) == len(g_d) == 18
    for (name, _), a, d in zip(tr_a.texture_mlp.named_parameters(), g_a, g_d):
        _close_to_dense(a, d, f'SDS iteration 0 {name}')
    s = tr_a._sds_setup
    assert s['field_texels'] == 'active' and 0 < s['active_fraction'] < 1 and s['n_active'] == s['render_cache']['active_texels'].numel()
    assert tr_d._sds_setup['field_texels'] == 'all' and 'active_texels' not in tr_d._sds_setup['render_cache']
    print(f"SDS loop: {s['n_active']} of {128 * 128} texels active ({s['active_fraction']:.3f})")
