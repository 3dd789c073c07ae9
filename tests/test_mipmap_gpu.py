"""GPU: mip-mapped texture sampling (csrc/texmip.hip) — the pyramid, the per-face level of detail, the trilinear forward
and the bit-reproducible backward against the numpy restatement tests/mipmap_rule.py (array_equal), the host surface in kal, and the
product path (Renderer, TexturedMeshModel.render, the SDS loop) in the 'mipmap' mode."""
import os

import numpy as np
import pytest
import torch

import mipmap_rule as MR

pytestmark = pytest.mark.gpu
f32 = np.float32


def _L():
    from contexture_nerf_amd import _lib
    return _lib


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _build(dev, tex, L, cov=None):
    """ctx_mip_build -> (pyr buffer, cov_count buffer, levels 1.. as numpy, counts 0.. as numpy)"""
    Lb = _L(); lib = Lb.load()
    C, T, _ = tex.shape
    d_tex = _t(tex, dev)
    pyr = torch.full((lib.ctx_mip_levels_bytes(C, T, L),), 0xff, dtype=torch.uint8, device=dev)
    cc = torch.full((lib.ctx_mip_cov_bytes(T, L),), 0xff, dtype=torch.uint8, device=dev)
    d_cov = None if cov is None else _t(cov, dev)
    Lb.check(lib.ctx_mip_build(Lb.ptr(d_tex), Lb.ptr(d_cov), C, T, L, Lb.ptr(pyr), Lb.ptr(cc), Lb.stream()))
    torch.cuda.synchronize()
    flt, cnt = pyr.view(torch.float32).cpu().numpy(), cc.cpu().numpy()
    levels, counts, off, coff = [], [cnt[:T * T].reshape(T, T)], 0, T * T
    for l in range(1, L):
        n = (T >> l) ** 2
        levels.append(flt[off:off + C * n].reshape(C, T >> l, T >> l)); off += C * n
        counts.append(cnt[coff:coff + n].reshape(T >> l, T >> l)); coff += n
    return d_tex, pyr, cc, levels, counts


# ---- the pyramid ----------------------------------------------------------------------------------------------------------------------
# T = 64, L = 5 and T = 8, L = 3: one pass; T = 48: a tile that is not full; T = 128, L = 7: the second pass reads level 5 and its counts
@pytest.mark.parametrize("C,T,L", [(1, 64, 5), (3, 64, 5), (4, 64, 5), (3, 8, 3), (2, 48, 4), (3, 128, 7), (1, 16, 1)])
@pytest.mark.parametrize("covered", [False, True])
def test_pyramid_equals_the_rule(dev, C, T, L, covered):
    tex = np.random.default_rng(T + C).standard_normal((C, T, T)).astype(f32)
    cov = MR.case_coverage(T, 5) if covered and T >= 16 else ((np.arange(T * T).reshape(T, T) % 3 != 0).astype(np.uint8) if covered else None)
    if covered and T == 8:
        cov[0:4, 0:4] = 0; cov[4:6, 6:8] = 0
    want_l, want_c = MR.pyramid(tex, L, cov)
    _, _, _, got_l, got_c = _build(dev, tex, L, cov)
    for l in range(1, L):
        assert np.array_equal(got_l[l - 1], want_l[l]), f"level {l}"
    for l in range(L):
        assert np.array_equal(got_c[l], want_c[l]), f"counts of level {l}"
    if covered and L >= 3:
        assert (want_c[1] == 0).any() and (want_c[2] == 0).any() and ((want_c[1] > 0) & (want_c[1] < 4)).any()


def test_mip_pyramid_returns_views_of_one_buffer_with_level_0_the_atlas(dev):
    from contexture_nerf_amd import kal
    tex = np.random.default_rng(0).uniform(0, 1, (3, 64, 64)).astype(f32)
    cov = MR.case_coverage(64, 1)
    d_tex = _t(tex, dev)
    lv = kal.mip_pyramid(d_tex, 5, coverage=_t(cov, dev))
    assert len(lv) == 5 and lv[0].data_ptr() == d_tex.data_ptr() and [tuple(x.shape) for x in lv] == [(3, 64 >> l, 64 >> l) for l in range(5)]
    base = lv[1].untyped_storage().data_ptr()
    assert all(x.untyped_storage().data_ptr() == base for x in lv[2:])
    for got, want in zip(lv, MR.pyramid(tex, 5, cov)[0]):
        assert np.array_equal(got.cpu().numpy(), want)


# ---- lod -------------------------------------------------------------------------------------------------------------------------------
def _lod_faces():
    """B = 2, twelve faces for H = 12, W = 20, T = 64, L = 4: a right triangle with legs of px pixels covering tu x tv texels"""
    H, W, T = 12, 20, 64

    def face(tx, ty, org=(-0.5, -0.25)):
        # legs of 4 pixels in NDC (8 / W, 8 / H) whose uv spans 4 * tx and 4 * ty texels
        p = np.array([org, (org[0] + 8.0 / W, org[1]), (org[0], org[1] + 8.0 / H)], f32)
        t = np.array([(0.25, 0.25), (0.25 + 4.0 * tx / T, 0.25), (0.25, 0.25 + 4.0 * ty / T)], f32)
        return p, t
    faces = [face(1, 1), face(2, 2), face(4, 4), face(100, 100), face(0.25, 0.5), face(6, 0.5), face(3, 3), face(1.5, 5), face(2, 2), face(2, 2),
             face(2.5, 2.5, (0.1, 0.3)), face(0.99, 1.01)]
    fvi = np.stack([f[0] for f in faces])[None].repeat(2, 0).copy()
    uva = np.stack([f[1] for f in faces])[None].repeat(2, 0).copy()
    fvi[:, 8, 2] = fvi[:, 8, 0] + (fvi[:, 8, 1] - fvi[:, 8, 0]) * f32(0.5)      # zero area
    fvi[0, 9, 1, 0] = np.nan                                                   # a NaN vertex, in view 0 only
    fvi[1] = fvi[1] * f32(0.5)                                                 # view 1 sees everything at half the size
    uva[1, :, :, 0] = uva[1, :, :, 0] * f32(1.25)
    return fvi, uva, H, W, T


@pytest.mark.parametrize("scale", [None, (1.0, 2.5)])
@pytest.mark.parametrize("batched_uv", [False, True])
def test_face_uv_lod_equals_the_rule(dev, scale, batched_uv):
    from contexture_nerf_amd import kal
    fvi, uva, H, W, T = _lod_faces()
    uva = uva if batched_uv else uva[:1]
    want = MR.lod_np(fvi, uva, H, W, T, 4, scale)
    got = kal.face_uv_lod(_t(fvi, dev), _t(uva, dev), H, W, T, 4, scale=scale).cpu().numpy()
    assert got.dtype == f32 and np.array_equal(got, want)
    if scale is None:
        # 1, 2 and 4 texels per pixel (2 / W is not a binary fraction: to a rounding), clamped, magnified, stretched along x only
        assert np.abs(want[0, :6] - f32([0, 1, 2, 3, 0, 2.5])).max() < 1e-6 and want[0, 3] == 3 and want[0, 4] == 0
        assert want[0, 8] == 0 and want[0, 9] == 0 and want[1, 9] > 0 and 0 < want[0, 11] < 0.02


# ---- forward ---------------------------------------------------------------------------------------------------------------------------
FB, FH, FW, FT, FL, FF = 2, 24, 40, 32, 4, 12


def _fwd(dev, tex, uv, lod, fi, L, cov=None):
    Lb = _L(); lib = Lb.load()
    C, T, _ = tex.shape
    B, HW = fi.shape
    d_tex, pyr, _, _, _ = _build(dev, tex, L, cov)
    out = torch.full((B, HW, C), float('nan'), device=dev)
    d_uv, d_lod, d_fi = _t(uv, dev), _t(lod, dev), _t(fi, dev)
    Lb.check(lib.ctx_texture_mapping_mip_fwd(Lb.ptr(d_uv), Lb.ptr(d_tex), Lb.ptr(pyr), Lb.ptr(d_lod), Lb.ptr(d_fi), B, HW, lod.shape[1], C, T, L,
                                             Lb.ptr(out), Lb.stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy(), lib.ctx_mip_status(Lb.ptr(pyr), C, T, L, Lb.stream())


@pytest.mark.parametrize("C", [1, 3, 4])
def test_forward_equals_the_rule_and_is_bilinear_where_the_lod_is_zero(dev, C):
    from contexture_nerf_amd import kal
    tex = np.random.default_rng(20 + C).uniform(0, 1, (C, FT, FT)).astype(f32)
    uv, fi = MR.case_raster(FB, FH, FW, FF, 21)
    lod = MR.case_lod_table(FB, FF, FL, 22)
    got, status = _fwd(dev, tex, uv, lod, fi, FL)
    assert status == 0 and np.array_equal(got, MR.forward(MR.pyramid(tex, FL)[0], uv, lod, fi))
    cov = MR.case_coverage(FT, 23)
    assert np.array_equal(_fwd(dev, tex, uv, lod, fi, FL, cov)[0], MR.forward(MR.pyramid(tex, FL, cov)[0], uv, lod, fi))
    junk = lod.copy(); junk[:, 6:10] = (np.nan, -3.0, 50.0, np.inf)              # kept inside [0, L-1], never an index
    assert np.array_equal(_fwd(dev, tex, uv, junk, fi, FL)[0], MR.forward(MR.pyramid(tex, FL)[0], uv, junk, fi))
    # lod 0 everywhere: mode='bilinear' with mask_idx, through the host surface
    d_uv, d_fi = _t(uv.reshape(FB, FH, FW, 2), dev), _t(fi.reshape(FB, FH, FW), dev)
    d_tex = _t(tex, dev)[None].expand(FB, -1, -1, -1)
    mip = kal.texture_mapping(d_uv, d_tex, mode='mipmap', mask_idx=d_fi, lod=torch.zeros(FB, FF, device=dev), levels=FL)
    assert torch.equal(mip, kal.texture_mapping(d_uv, d_tex, mode='bilinear', mask_idx=d_fi))
    mip = kal.texture_mapping(d_uv, d_tex, mode='mipmap', mask_idx=d_fi, lod=_t(lod, dev), levels=FL)
    assert np.array_equal(mip.cpu().numpy().reshape(FB, FH * FW, C), got)


# ---- backward --------------------------------------------------------------------------------------------------------------------------
def _bwd(dev, go, uv, lod, fi, T, L, cc=None, presum=None, poison=True):
    Lb = _L(); lib = Lb.load()
    B, HW, C = go.shape
    ws = torch.full((lib.ctx_texture_mapping_mip_bwd_ws_bytes(C, T, L),), 0xff if poison else 0, dtype=torch.uint8, device=dev)
    g = torch.full((C, T, T), float('nan'), device=dev)
    d = [_t(a, dev) for a in (go, uv, lod, fi)]
    old = os.environ.pop("CTX_TEXMIP_PRESUM", None)
    if presum is not None:
        os.environ["CTX_TEXMIP_PRESUM"] = str(presum)
    try:
        Lb.check(lib.ctx_texture_mapping_mip_bwd(*[Lb.ptr(a) for a in d], Lb.ptr(cc), B, HW, lod.shape[1], C, T, L, Lb.ptr(ws), Lb.ptr(g), Lb.stream()))
    finally:
        os.environ.pop("CTX_TEXMIP_PRESUM", None)
        if old is not None:
            os.environ["CTX_TEXMIP_PRESUM"] = old
    torch.cuda.synchronize()
    return g


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("covered", [False, True])
def test_backward_equals_the_rule_twice_and_without_the_presum(dev, C, covered):
    rng = np.random.default_rng(30 + C)
    uv, fi = MR.case_raster(FB, FH, FW, FF, 31)
    lod = MR.case_lod_table(FB, FF, FL, 32)
    go = (rng.standard_normal((FB, FH * FW, C)) * 3).astype(f32)
    cov = MR.case_coverage(FT, 33) if covered else None
    cc = _build(dev, np.zeros((C, FT, FT), f32), FL, cov)[2] if covered else None
    want = MR.backward_np(go, uv, lod, fi, FT, FL, MR.pyramid(np.zeros((C, FT, FT), f32), FL, cov)[1] if covered else None)
    a = _bwd(dev, go, uv, lod, fi, FT, FL, cc)
    assert np.array_equal(a.cpu().numpy(), want)
    assert torch.equal(a, _bwd(dev, go, uv, lod, fi, FT, FL, cc, poison=False))
    assert torch.equal(a, _bwd(dev, go, uv, lod, fi, FT, FL, cc, presum=0))
    if covered:
        assert np.all(a.cpu().numpy()[:, cov == 0] == 0) and np.any(a.cpu().numpy()[:, cov != 0] != 0)


def test_backward_of_4096_pixels_on_one_coarse_texel(dev):
    """Every pixel lands on the centre of texel (1, 1) of the coarsest level (side 4) with a gradient near the absmax: the longest runs the
    pre-sum meets and the most terms one entry of the accumulator can receive from this many pixels.  At lod 2.5 half of each term goes to
    the four level-2 texels under that texel, a quarter each."""
    T, L, n = 32, 4, 4096
    rng = np.random.default_rng(40)
    uv = np.empty((1, n, 2), f32)
    uv[0, :, 0] = 0.375; uv[0, :, 1] = 0.625          # the centre of texel (1, 1) of level 3: the other three taps weigh exactly 0
    fi = np.zeros((1, n), np.int64)
    go = rng.uniform(0.99, 1.0, (1, n, 3)).astype(f32)
    go[0, ::2, 1] *= -1
    for lodv in (3.0, 2.5):
        lod = np.array([[lodv]], f32)
        want = MR.backward_np(go, uv, lod, fi, T, L)
        a = _bwd(dev, go, uv, lod, fi, T, L)
        assert np.array_equal(a.cpu().numpy(), want)
        assert torch.equal(a, _bwd(dev, go, uv, lod, fi, T, L, presum=0))
        blk = want[:, 8:16, 8:16]
        assert np.all(blk == blk[:, :1, :1]) and abs(blk[0, 0, 0]) > 1


def test_backward_of_zero_is_zero_of_infinity_nan_and_autograd_takes_the_same_path(dev):
    from contexture_nerf_amd import kal
    C = 3
    uv, fi = MR.case_raster(FB, FH, FW, FF, 50)
    lod = MR.case_lod_table(FB, FF, FL, 51)
    go = np.zeros((FB, FH * FW, C), f32)
    assert torch.equal(_bwd(dev, go, uv, lod, fi, FT, FL), torch.zeros(C, FT, FT, device=dev))
    go[1, 7, 2] = np.inf
    assert bool(torch.isnan(_bwd(dev, go, uv, lod, fi, FT, FL)).all())
    # tex.grad of sum() is the C-ABI call on a gradient of ones, with and without a coverage plane
    tex = np.random.default_rng(52).uniform(0, 1, (C, FT, FT)).astype(f32)
    for cov in (None, MR.case_coverage(FT, 53)):
        d_tex = _t(tex, dev)[None].requires_grad_(True)
        out = kal.texture_mapping(_t(uv.reshape(FB, FH, FW, 2), dev), d_tex.expand(FB, -1, -1, -1), mode='mipmap', mask_idx=_t(fi.reshape(FB, FH, FW), dev),
                                  lod=_t(lod, dev), levels=FL, coverage=None if cov is None else _t(cov, dev))
        out.sum().backward()
        cc = None if cov is None else _build(dev, tex, FL, cov)[2]
        assert torch.equal(d_tex.grad[0], _bwd(dev, np.ones((FB, FH * FW, C), f32), uv, lod, fi, FT, FL, cc))


# ---- the stripe quad ---------------------------------------------------------------------------------------------------------------------
def test_stripes_through_the_raster_average_in_mipmap_and_alias_in_bilinear(dev):
    """The full-screen quad drawn by the rasteriser at 16 x 16 over the T = 64 stripe atlas: lod 2 on both faces.  Level 2 is 0.5 everywhere
    and the bilinear taps sit between two texels of 1, so the outputs are 0.5 and 1.0 up to the roundings of four weights, four products
    and four sums (at most 12 * 2^-24 relative: 1e-6); against the rule on the raster's own uv they are array_equal."""
    from contexture_nerf_amd import kal
    T, L, H, W = 64, 4, 16, 16
    fvi, uva = MR.quad_faces()
    d_fvi, d_uva = _t(fvi, dev), _t(uva, dev)
    fvc = torch.cat([d_fvi, torch.full((1, 2, 3, 1), -1.0, device=dev)], -1).contiguous()
    _, uv, fi, _ = kal.render.mesh.rasterize_fused(H, W, fvc, d_fvi, d_uva)
    assert bool((fi >= 0).all())
    lod = kal.face_uv_lod(d_fvi, d_uva, H, W, T, L)
    assert torch.equal(lod, torch.full((1, 2), 2.0, device=dev))
    tex = MR.stripes(T)
    d_tex = _t(tex, dev)[None]
    mip = kal.texture_mapping(uv, d_tex, mode='mipmap', mask_idx=fi, lod=lod, levels=L)
    bil = kal.texture_mapping(uv, d_tex, mode='bilinear', mask_idx=fi)
    assert float((mip - 0.5).abs().max()) <= 1e-6 and float((bil - 1.0).abs().max()) <= 1e-6
    want = MR.forward(MR.pyramid(tex, L)[0], uv.cpu().numpy().reshape(1, H * W, 2), lod.cpu().numpy(), fi.cpu().numpy().reshape(1, H * W))
    assert np.array_equal(mip.cpu().numpy().reshape(1, H * W, 1), want)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from contexture_nerf_amd import kal
    Lb = _L(); lib = Lb.load()
    for T, L in ((48, 6), (8, 4), (10, 3), (16, 0), (16, 17)):
        assert lib.ctx_mip_levels_bytes(3, T, L) == -1 and lib.ctx_texture_mapping_mip_bwd_ws_bytes(3, T, L) == -1
        with pytest.raises(Lb.CtxError, match="mip levels"):
            kal.mip_pyramid(torch.zeros(3, T, T, device=dev), L)
    assert lib.ctx_mip_levels_bytes(5, 16, 2) == -1
    with pytest.raises(Lb.CtxError, match="C=5"):
        kal.mip_pyramid(torch.zeros(5, 16, 16, device=dev), 2)
    uv, fi = MR.case_raster(FB, FH, FW, FF, 60)
    d_uv, d_fi, d_lod = _t(uv.reshape(FB, FH, FW, 2), dev), _t(fi.reshape(FB, FH, FW), dev), torch.zeros(FB, FF, device=dev)
    tex = torch.rand(1, 3, FT, FT, device=dev)
    with pytest.raises(Lb.CtxError, match="C=5"):
        kal.texture_mapping(d_uv, torch.rand(1, 5, FT, FT, device=dev), mode='mipmap', mask_idx=d_fi, lod=d_lod, levels=FL)
    with pytest.raises(Lb.CtxError, match="needs mask_idx"):
        kal.texture_mapping(d_uv, tex, mode='mipmap', mask_idx=d_fi, levels=FL)
    with pytest.raises(Lb.CtxError, match="needs mask_idx"):
        kal.texture_mapping(d_uv, tex, mode='mipmap', lod=d_lod, levels=FL)
    with pytest.raises(Lb.CtxError, match="mip levels"):
        kal.texture_mapping(d_uv, tex, mode='mipmap', mask_idx=d_fi, lod=d_lod, levels=6)
    with pytest.raises(Lb.CtxError, match="differ"):
        kal.texture_mapping(d_uv, torch.rand(FB, 3, FT, FT, device=dev), mode='mipmap', mask_idx=d_fi, lod=d_lod, levels=FL)
    same = tex.repeat(FB, 1, 1, 1)                                               # a materialised batch of equal textures is one atlas
    assert torch.equal(kal.texture_mapping(d_uv, same, mode='mipmap', mask_idx=d_fi, lod=d_lod, levels=FL),
                       kal.texture_mapping(d_uv, tex.expand(FB, -1, -1, -1), mode='mipmap', mask_idx=d_fi, lod=d_lod, levels=FL))
    # a face_idx outside the lod table is not read: its pixel is NaN, the pyramid's status is set, the gradient is NaN
    bad = fi.copy(); bad[1, 100] = FF; bad[0, 3] = 1 << 40
    texn = np.random.default_rng(61).uniform(0, 1, (3, FT, FT)).astype(f32)
    lod = MR.case_lod_table(FB, FF, FL, 62)
    got, status = _fwd(dev, texn, uv, lod, bad, FL)
    assert status == 1 and np.all(np.isnan(got[1, 100])) and np.all(np.isnan(got[0, 3]))
    ok = np.ones((FB, FH * FW), bool); ok[1, 100] = ok[0, 3] = False
    assert np.array_equal(got[ok], MR.forward(MR.pyramid(texn, FL)[0], uv, lod, fi)[ok])
    assert bool(torch.isnan(_bwd(dev, np.ones((FB, FH * FW, 3), f32), uv, lod, bad, FT, FL)).all())
    # the other modes do not look at the new arguments
    assert torch.equal(kal.texture_mapping(d_uv, tex, mode='bilinear', mask_idx=d_fi, lod=None, levels=99, coverage=None),
                       kal.texture_mapping(d_uv, tex, mode='bilinear', mask_idx=d_fi))


# ---- the product ---------------------------------------------------------------------------------------------------------------------------
def test_product_renders_and_trains_in_the_mipmap_mode(dev, tmp_path):
    from test_hashtex_gpu import _tiny_trainer
    tr = _tiny_trainer(dev, tmp_path, guide__texture_interpolation_mode='mipmap')
    mm = tr.mesh_model
    assert mm.renderer.interpolation_mode == 'mipmap' and mm.renderer.mip_levels == 4
    v = tr.train_views[1]
    gray = torch.tensor([0.5, 0.5, 0.5], device=dev)
    view = dict(theta=v['theta'], phi=tr._offset_phi(v['phi']), radius=float(v['radius']), background=gray)
    with torch.no_grad():
        out = mm.render(dims=(48, 48), **view)
        assert set(out) == {'image', 'mask', 'background', 'foreground', 'depth', 'normals', 'render_cache', 'texture_map', 'mlp_output'}
        assert out['image'].shape == (1, 3, 48, 48) and bool(torch.isfinite(out['image']).all())
        cache = out['render_cache']
        key, lod = cache['face_lod']
        assert key == (48, 48, 128, 4, None) and lod.shape == (1, mm.mesh.faces.shape[0]) and float(lod.max()) > 0
        again = mm.render(render_cache=cache, background=gray)
        assert again['render_cache']['face_lod'][1] is lod and torch.equal(again['image'], out['image'])
        scaled = mm.render(render_cache=cache, background=gray, mip_scale=[2.0])
        assert scaled['render_cache']['face_lod'][0] == (48, 48, 128, 4, (2.0,)) and not torch.equal(scaled['render_cache']['face_lod'][1], lod)
        mm.renderer.interpolation_mode = 'bilinear'
        try:
            plain = mm.render(dims=(48, 48), **view)
        finally:
            mm.renderer.interpolation_mode = 'mipmap'
        assert 'face_lod' not in plain['render_cache'] and not torch.equal(plain['image'], out['image'])
    before = [p.detach().clone() for p in tr.texture_mlp.parameters()]
    log = tr.paint_zero123plus(iterations=2, tile=64)
    assert [r['i'] for r in log] == [0, 1]
    assert all(np.isfinite(r['loss']) and np.isfinite(r['grad_norm']) and r['grad_norm'] > 0 for r in log)
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, tr.texture_mlp.parameters()))
    key = tr._sds_setup['render_cache']['face_lod'][0]
    assert key[:4] == (192, 192, 128, 4) and key[4][0] == 1.0 and len(key[4]) == len(tr.train_views) and all(s > 0 for s in key[4])


def test_default_mode_keeps_todays_cache(dev, tmp_path):
    from test_hashtex_gpu import _tiny_trainer
    tr = _tiny_trainer(dev, tmp_path)
    v = tr.train_views[1]
    with torch.no_grad():
        out = tr.mesh_model.render(theta=v['theta'], phi=tr._offset_phi(v['phi']), radius=float(v['radius']), dims=(48, 48),
                                   background=torch.tensor([0.5, 0.5, 0.5], device=dev))
    assert set(out['render_cache']) == {'camera_transform', 'uv_features', 'face_normals', 'face_idx', 'depth_map', 'raw_depth_map', 'face_vertices_image',
                                        'normals_image'}
