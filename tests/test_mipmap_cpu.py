"""CPU: mip-mapped texture sampling — the rule tests/mipmap_rule.py against independent statements of what it must
give, and the configuration.  No GPU: tests/test_mipmap_gpu.py holds the kernels to the same rule with array_equal.

1. the level of detail: the values of the full-screen quad, the faces that give 0, the clamp;
2. the forward at an integer lod against float64 grid_sample of the box-filtered atlas (bound 1e-5, the bilinear sampler's);
3. the backward: the forward's adjoint in float64 (1e-12 relative), and the float32 integer pyramid against it per texel;
4. the stripe image: 0.5 everywhere in mipmap mode, 1.0 in bilinear;
5. config: default, the new value, mip_levels against texture_resolution, the field_texels = 'active' refusal."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mipmap_rule as MR

f32 = np.float32


# ---- 1. lod --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,T,scale,want", [(16, 16, 16, None, 0.0), (16, 16, 32, None, 1.0), (16, 16, 64, None, 2.0), (16, 16, 48, None, 1.5),
                                              (12, 20, 64, None, 2.3333335), (16, 16, 16, 3.0, 1.5)])
def test_lod_of_the_full_screen_quad(H, W, T, scale, want):
    fvi, uva = MR.quad_faces()
    lod = MR.lod_np(fvi, uva, H, W, T, 4, None if scale is None else [scale])
    assert lod.dtype == f32 and lod.shape == (1, 2)
    assert np.array_equal(lod, np.full((1, 2), f32(want)))


def test_lod_is_zero_for_degenerate_nan_and_magnified_faces_and_clamps():
    fvi, uva = MR.quad_faces()
    fvi = np.repeat(fvi, 5, 1)[:, :5].copy(); uva = np.repeat(uva, 5, 1)[:, :5].copy()
    fvi[0, 0] = fvi[0, 1]; uva[0, 0] = uva[0, 1]
    fvi[0, 1, 2] = fvi[0, 1, 1]                          # zero area
    fvi[0, 2, 0, 0] = np.nan                             # a NaN vertex
    uva[0, 3] = uva[0, 3] * f32(0.01)                    # magnified: 0.16 texels per pixel
    uva[0, 4] = uva[0, 4] * f32(1000)                    # 1000 * 64 / 16 texels per pixel: clamps to L-1
    lod = MR.lod_np(fvi, uva, 16, 16, 64, 4)
    assert np.array_equal(lod[0], f32([2, 0, 0, 0, 3]))
    for L in (1, 2, 3):
        assert np.array_equal(MR.lod_np(*MR.quad_faces(), 16, 16, 64, L), np.full((1, 2), f32(min(2, L - 1))))
    e = np.array([[[[0, 0], [1e-30, 0], [0, 1e-30]]]], f32)          # det underflows to 0: lod 0; a huge Jacobian: r2 infinite, L-1
    assert MR.lod_np(e, MR.quad_faces()[1][:, :1], 16, 16, 64, 4)[0, 0] == 0
    e = np.array([[[[0, 0], [1e-15, 0], [0, 1e-15]]]], f32)
    assert MR.lod_np(e, MR.quad_faces()[1][:, :1] * f32(1e10), 16, 16, 64, 4)[0, 0] == 3


def test_levels_that_do_not_fit_are_refused_by_name():
    for T, L in ((48, 6), (8, 4), (10, 3), (16, 0), (16, 17)):
        with pytest.raises(ValueError, match="mip levels"):
            MR.check_levels(T, L)
    assert MR.check_levels(48, 4) == [48, 24, 12, 6] and MR.check_levels(8, 3) == [8, 4, 2]


# ---- the pyramid ----------------------------------------------------------------------------------------------------------------------
def test_pyramid_without_coverage_is_the_ordered_mean_and_with_coverage_averages_the_covered_children():
    rng = np.random.default_rng(0)
    tex = rng.standard_normal((3, 16, 16)).astype(f32)
    lv, cnt = MR.pyramid(tex, 4)
    a, b, c, d = tex[:, 0::2, 0::2], tex[:, 0::2, 1::2], tex[:, 1::2, 0::2], tex[:, 1::2, 1::2]
    assert np.array_equal(lv[1], (((a + b) + c) + d) / f32(4)) and all(np.all(n == 4) for n in cnt[1:])
    assert np.abs(lv[3].astype(np.float64) - tex.astype(np.float64).reshape(3, 2, 8, 2, 8).mean((2, 4))).max() < 1e-6
    cov = MR.case_coverage(16, 1)
    lv, cnt = MR.pyramid(tex, 4, cov)
    assert cnt[1][0, 0] == 0 and cnt[1][1, 1] == 0 and cnt[2][0, 0] == 0 and np.all(lv[2][:, 0, 0] == 0) and cnt[1][2, 4] == 0
    y, x = np.argwhere((cnt[1] > 0) & (cnt[1] < 4))[0]
    blk, cb = tex[:, 2 * y:2 * y + 2, 2 * x:2 * x + 2].astype(np.float64), cov[2 * y:2 * y + 2, 2 * x:2 * x + 2] != 0
    assert np.abs(lv[1][:, y, x] - (blk * cb).sum((1, 2)) / cb.sum()).max() < 1e-6
    poisoned = np.where(cov[None] != 0, tex, np.nan).astype(f32)                  # an uncovered texel is never read
    assert all(np.array_equal(p, q) for p, q in zip(MR.pyramid(poisoned, 4, cov)[0][1:], lv[1:]))


# ---- 2. forward ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l", [0, 1, 2, 3])
def test_forward_at_an_integer_lod_is_grid_sample_of_the_box_filtered_atlas(l):
    T, L, B, H, W, Fc = 32, 4, 2, 24, 40, 12
    rng = np.random.default_rng(2)
    tex = rng.uniform(0, 1, (3, T, T)).astype(f32)
    uv, fi = MR.case_raster(B, H, W, Fc, 3)
    lod = np.full((B, Fc), f32(l))
    out = MR.forward(MR.pyramid(tex, L)[0], uv, lod, fi)
    t64 = torch.from_numpy(tex.astype(np.float64))[None]
    pooled = F.avg_pool2d(t64, 2 ** l) if l else t64
    u64 = torch.from_numpy(uv.astype(np.float64))
    grid = torch.stack([u64[..., 0] * 2 - 1, (1 - u64[..., 1]) * 2 - 1], -1).reshape(B, H, W, 2)
    ref = F.grid_sample(pooled.expand(B, -1, -1, -1), grid, mode='bilinear', padding_mode='border', align_corners=False)
    ref = ref.permute(0, 2, 3, 1).reshape(B, H * W, 3).numpy() * (fi >= 0)[..., None]
    err = np.abs(out - ref).max()
    print(f"level {l}: max |rule - float64 grid_sample| = {err:.3e}")
    assert err < 1e-5
    assert np.all(out[fi < 0] == 0)


def test_forward_blends_linearly_and_is_bilinear_where_the_lod_is_zero():
    T, L, B, H, W, Fc = 32, 4, 2, 24, 40, 12
    tex = np.random.default_rng(4).uniform(0, 1, (3, T, T)).astype(f32)
    uv, fi = MR.case_raster(B, H, W, Fc, 5)
    lv = MR.pyramid(tex, L)[0]
    lod = MR.case_lod_table(B, Fc, L, 6)
    out, o64 = MR.forward(lv, uv, lod, fi), MR.forward(lv, uv, lod, fi, np.float64)
    assert np.abs(out - o64).max() < 1e-6
    _, l0, f = MR.pixel_levels(lod, fi, L)
    for l in range(L - 1):
        sel = (fi >= 0) & (l0 == l)
        lo = MR.forward(lv, uv, np.full((B, Fc), f32(l)), fi, np.float64)[sel]
        hi = MR.forward(lv, uv, np.full((B, Fc), f32(l + 1)), fi, np.float64)[sel]
        assert np.abs(o64[sel] - (lo * (1 - f[sel][:, None].astype(np.float64)) + hi * f[sel][:, None])).max() < 1e-12
    junk = np.array([[np.nan, -1.0, 99.0, np.inf, -np.inf, 0.0] * 2] * B, f32)     # a table kept inside [0, L-1]
    want = np.array([[0, 0, L - 1, L - 1, 0, 0] * 2] * B, f32)
    assert np.array_equal(MR.forward(lv, uv, junk, fi), MR.forward(lv, uv, want, fi))


# ---- 3. backward -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("covered", [False, True])
def test_backward_is_the_adjoint_and_the_integer_pyramid_keeps_the_bound(covered):
    """With a coverage plane stage B leaves the uncovered texels at 0 by definition, so the backward is the adjoint of the forward on
    the covered texels: <fwd(P tex), g> = <tex, bwd(g)> with P the projection onto them (P = 1 without a plane)."""
    T, L, B, H, W, Fc, C = 32, 4, 2, 24, 40, 12, 3
    rng = np.random.default_rng(7)
    tex = rng.standard_normal((C, T, T))
    uv, fi = MR.case_raster(B, H, W, Fc, 8)
    lod = MR.case_lod_table(B, Fc, L, 9)
    go = rng.standard_normal((B, H * W, C)).astype(f32)
    cov = MR.case_coverage(T, 10) if covered else None
    ptex = tex * (cov != 0)[None] if covered else tex
    lv, cnt = MR.pyramid(ptex, L, cov, np.float64)
    cnt = cnt if covered else None
    g64 = MR.backward_plain(go, uv, lod, fi, T, L, cnt)
    lhs, rhs = float((MR.forward(lv, uv, lod, fi, np.float64) * go).sum()), float((tex * g64).sum())
    scale = float((np.abs(tex) * MR.backward_plain(np.abs(go), uv, lod, fi, T, L, cnt)).sum())
    print(f"adjoint: {lhs!r} against {rhs!r}, relative {abs(lhs - rhs) / scale:.3e}")
    assert abs(lhs - rhs) <= 1e-12 * scale
    if covered:
        assert np.all(g64[:, cov == 0] == 0)
    # the float32 integer pyramid per texel: (8 + 2L) roundings of 2^-24 relative on A (the float64 backward of |g|): the weights, the
    # blend, the product, the convert and the L collapse steps; the quantisation totals at most 2^(61+x-2E) <= 2^-30 max|g| here
    g32 = MR.backward_np(go, uv, lod, fi, T, L, cnt)
    A = MR.backward_plain(np.abs(go), uv, lod, fi, T, L, cnt)
    bound = (8 + 2 * L) * 2.0 ** -24 * A + 2.0 ** -30 * float(np.abs(go).max())
    ratio = (np.abs(g32 - g64) / bound).max()
    print(f"float32 backward: max error / bound = {ratio:.3f}")
    assert g32.dtype == f32 and ratio <= 1.0


def test_backward_of_zero_is_zero_and_of_a_non_finite_gradient_is_nan():
    T, L = 8, 3
    uv, fi = MR.case_raster(1, 4, 4, 3, 11)
    lod = np.array([[0.0, 0.5, 2.0]], f32)
    go = np.zeros((1, 16, 2), f32)
    assert np.array_equal(MR.backward_np(go, uv, lod, fi, T, L), np.zeros((2, T, T), f32))
    go[0, 3, 1] = np.inf
    assert np.all(np.isnan(MR.backward_np(go, uv, lod, fi, T, L)))


# ---- 4. the stripes ----------------------------------------------------------------------------------------------------------------------
def test_stripes_alias_in_bilinear_and_average_in_mipmap():
    T, L, H, W = 64, 4, 16, 16
    fvi, uva = MR.quad_faces()
    uv, fi = MR.quad_raster(H, W)
    lod = MR.lod_np(fvi, uva, H, W, T, L)
    assert np.all(lod == 2)
    lv = MR.pyramid(MR.stripes(T), L)[0]
    assert np.array_equal(MR.forward(lv, uv, lod, fi), np.full((1, H * W, 1), f32(0.5)))
    assert np.array_equal(MR.forward(lv, uv, np.zeros_like(lod), fi), np.full((1, H * W, 1), f32(1.0)))


# ---- 5. config ---------------------------------------------------------------------------------------------------------------------------
def test_config_mipmap_mode_levels_and_the_active_texels_refusal():
    from contexture_nerf_amd import config as CFG
    assert CFG.TrainConfig().guide.texture_interpolation_mode == 'bilinear' and CFG.TrainConfig().guide.mip_levels == 4
    cfg = CFG.parse(argv=['--guide.texture_interpolation_mode=mipmap'])
    assert cfg.guide.texture_interpolation_mode == 'mipmap' and cfg.guide.mip_levels == 4
    assert CFG.parse(argv=['--guide.texture_interpolation_mode=mipmap', '--guide.mip_levels=6', '--guide.texture_resolution=96']).guide.mip_levels == 6
    for bad in (['--guide.mip_levels=7', '--guide.texture_resolution=96'], ['--guide.mip_levels=0'], ['--guide.mip_levels=11'],
                ['--guide.mip_levels=3', '--guide.texture_resolution=6']):
        with pytest.raises(ValueError, match="mip_levels"):
            CFG.parse(argv=['--guide.texture_interpolation_mode=mipmap'] + bad)
    assert CFG.parse(argv=['--guide.mip_levels=11']).guide.mip_levels == 11          # read in the mipmap mode only
    with pytest.raises(ValueError, match="field_texels"):
        CFG.parse(argv=['--guide.texture_interpolation_mode=mipmap', '--optim.field_texels=active'])
    with pytest.raises(ValueError, match="texture_interpolation_mode"):
        CFG.parse(argv=['--guide.texture_interpolation_mode=trilinear'])
