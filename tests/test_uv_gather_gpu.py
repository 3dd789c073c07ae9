"""GPU: the texel-side gather (csrc/uvgather.hip) against the numpy restatement of tests/test_uv_gather_cpu.py.  Every comparison
is array_equal on the int64 sums.

1. kernel == restatement on spot: T in {64, 257}, (H, W) in {(97, 131), (301, 257)}, B in {1, 2, 7}, C in {1, 3, 4}, weight null /
   0-1 mask / floats in [0, 1];
2. special cases: shape_scale 1.2 (part of the mesh outside the image), an all-background view, an all -1 texel map, non-finite colours;
3. full size once: T = 1024, 7 x 1200^2, with the empty-texel count the CPU test pins;
4. reproducibility: 3 + 4 views == one call; the same call twice and on a side stream;
5. TexturedMeshModel.texel_map / uv_texel_map against chart_mask (spot and a chart_atlas mesh) and against the restatement's map;
6. refusals: a sentinel-filled acc comes back untouched;
7. end to end on the tiny UNet: paint() with guide.projection = 'gather', complete_atlas, export."""
import os
import tempfile
import numpy as np
import pytest
import torch

import test_uv_gather_cpu as G

pytestmark = pytest.mark.gpu

_SCENES, _MAPS = {}, {}


def scene_of(meshes, H, W, shape_scale=0.6):
    key = (H, W, shape_scale)
    if key not in _SCENES:
        sc = G.spot_scene(meshes, H, W, shape_scale)
        rng = np.random.default_rng(H * 1000 + W)
        sc['values'] = rng.random((7, H, W, 4)).astype(np.float32)
        sc['mask'] = (rng.random((7, H, W)) < 0.7).astype(np.float32)
        sc['wfloat'] = rng.random((7, H, W)).astype(np.float32)
        _SCENES[key] = sc
    return _SCENES[key]


def map_of(meshes, T):
    if T not in _MAPS:
        _MAPS[T] = G.texel_map(meshes["spot_triangulated_vt"].astype(np.float32), meshes["spot_triangulated_ft"].astype(np.int64), T)
    return _MAPS[T]


def gpu_gather(dev, tface, tbary, sc, values, weight, views=slice(None), acc=None):
    from contexture_nerf_amd import kal
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device=dev)
    C, T = values.shape[-1], tface.shape[0]
    if acc is None:
        acc = torch.zeros(C + 1, T, T, dtype=torch.int64, device=dev)
    kal.gather_fixed(t(values[views]), None if weight is None else t(weight[views]), t(sc['face_idx'][views]), t(sc['fvi'][views]), t(sc['f']),
                     t(tface), t(tbary), acc)
    return acc


# ---- 1. kernel == restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 7])
@pytest.mark.parametrize("H,W", [(97, 131), (301, 257)])
@pytest.mark.parametrize("T", [64, 257])
def test_kernel_equals_restatement(dev, meshes, T, H, W, B):
    sc = scene_of(meshes, H, W)
    tface, tbary = map_of(meshes, T)
    v = slice(0, B)
    for C in (1, 3, 4):
        for wname in (None, 'mask', 'wfloat'):
            w = None if wname is None else sc[wname]
            vals = sc['values'][..., :C]
            want = G.uv_gather_fixed(tface, tbary, sc['f'], sc['fvi'][v], sc['face_idx'][v], vals[v], None if w is None else w[v])
            got = gpu_gather(dev, tface, tbary, sc, vals, w, v).cpu().numpy()
            assert (want[C] > 0).sum() > 100
            assert np.array_equal(got, want), f"C={C} weight={wname}: {int((got != want).sum())} sums differ"


# ---- 2. special cases ---------------------------------------------------------------------------------------------------------
def test_mesh_partly_outside_the_image(dev, meshes):
    H, W, T = 97, 131, 257
    sc = scene_of(meshes, H, W, 1.2)
    fvi = sc['fvi']
    assert np.abs(fvi).max() > 1.0 and (sc['face_idx'] >= 0).any()     # some of the mesh projects outside
    tface, tbary = map_of(meshes, T)
    want = G.uv_gather_fixed(tface, tbary, sc['f'], fvi, sc['face_idx'], sc['values'][..., :3], sc['wfloat'])
    got = gpu_gather(dev, tface, tbary, sc, sc['values'][..., :3], sc['wfloat']).cpu().numpy()
    assert np.array_equal(got, want) and (want[3] > 0).sum() > 100


def test_background_view_empty_map_and_non_finite_colours(dev, meshes):
    H, W, T = 97, 131, 257
    sc = dict(scene_of(meshes, H, W))
    tface, tbary = map_of(meshes, T)
    vals = sc['values'][..., :3].copy()
    sentinel = np.random.default_rng(5).integers(-1 << 40, 1 << 40, (4, T, T))
    # an all-background view
    idx = sc['face_idx'].copy(); idx[1] = -1
    sc_bg = dict(sc, face_idx=idx)
    want = G.uv_gather_fixed(tface, tbary, sc['f'], sc['fvi'], idx, vals, sc['mask'], acc=sentinel.copy())
    got = gpu_gather(dev, tface, tbary, sc_bg, vals, sc['mask'], acc=torch.tensor(sentinel, device=dev)).cpu().numpy()
    assert np.array_equal(got, want)
    only_bg = gpu_gather(dev, tface, tbary, sc_bg, vals, None, slice(1, 2), acc=torch.tensor(sentinel, device=dev)).cpu().numpy()
    assert np.array_equal(only_bg, sentinel)
    # an all -1 texel map
    none = gpu_gather(dev, np.full_like(tface, -1), tbary, sc, vals, None, acc=torch.tensor(sentinel, device=dev)).cpu().numpy()
    assert np.array_equal(none, sentinel)
    # non-finite colours and weights: the texels that would read them get nothing from that view
    fy, fx = np.nonzero(sc['face_idx'][0] >= 0)
    pick = np.random.default_rng(6).choice(len(fy), 40, replace=False)
    vals[0, fy[pick[:20]], fx[pick[:20]], 1] = np.inf
    vals[0, fy[pick[20:]], fx[pick[20:]], 2] = np.nan
    wf = sc['wfloat'].copy()
    wf[3, fy[pick[:5]], fx[pick[:5]]] = np.nan
    clean = G.uv_gather_fixed(tface, tbary, sc['f'], sc['fvi'], sc['face_idx'], sc['values'][..., :3], sc['wfloat'])
    want = G.uv_gather_fixed(tface, tbary, sc['f'], sc['fvi'], sc['face_idx'], vals, wf)
    got = gpu_gather(dev, tface, tbary, sc, vals, wf).cpu().numpy()
    assert np.array_equal(got, want) and (want[3] < clean[3]).any()


# ---- 3. full size, once -------------------------------------------------------------------------------------------------------
def test_full_size_spot(dev, meshes):
    H, T = 1200, 1024
    sc = G.spot_scene(meshes, H, H)
    vals = G.painted_views(sc, H, H)
    tface, tbary = G.texel_map(sc['vt'], sc['ft'], T)
    want = G.uv_gather_fixed(tface, tbary, sc['f'], sc['fvi'], sc['face_idx'], vals)
    got = gpu_gather(dev, tface, tbary, sc, vals, None).cpu().numpy()
    assert np.array_equal(got, want)
    empty = int(((tface >= 0) & (got[3] == 0)).sum())
    print(f"spot T={T} 7 x {H}^2: gather leaves {empty} chart texels empty (pinned {G.SPOT_GATHER_EMPTY}; the scatter {G.SPOT_SCATTER_EMPTY})")
    assert empty == G.SPOT_GATHER_EMPTY and not got[:, tface < 0].any()


# ---- 4. reproducibility -------------------------------------------------------------------------------------------------------
def test_split_twice_and_side_stream(dev, meshes):
    H, W, T = 301, 257, 257
    sc = scene_of(meshes, H, W)
    tface, tbary = map_of(meshes, T)
    vals = sc['values']
    one = gpu_gather(dev, tface, tbary, sc, vals, sc['wfloat'])
    part = gpu_gather(dev, tface, tbary, sc, vals, sc['wfloat'], slice(0, 3))
    part = gpu_gather(dev, tface, tbary, sc, vals, sc['wfloat'], slice(3, 7), acc=part)
    assert torch.equal(part, one)
    again = gpu_gather(dev, tface, tbary, sc, vals, sc['wfloat'])
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        other = gpu_gather(dev, tface, tbary, sc, vals, sc['wfloat'])
    side.synchronize()
    assert torch.equal(again, one) and torch.equal(other, one)


# ---- 5. the texel map ---------------------------------------------------------------------------------------------------------
def test_texel_map_spot_and_chart_atlas_mesh(dev, meshes):
    from contexture_nerf_amd import atlas as A
    from contexture_nerf_amd.textured_mesh import uv_chart_mask, uv_texel_map
    vt, ft = meshes["spot_triangulated_vt"].astype(np.float32), meshes["spot_triangulated_ft"].astype(np.int64)
    bvt, bft = A.chart_atlas(meshes["bunny_v"], meshes["bunny_f"], resolution=256)
    for name, (vt_, ft_), T in (("spot", (vt, ft), 257), ("bunny", (np.asarray(bvt, np.float32), np.asarray(bft, np.int64)), 256)):
        face_uv = torch.tensor(vt_[ft_][None], device=dev)
        tface, tbary = uv_texel_map(face_uv, T)
        assert tface.dtype == torch.int64 and tuple(tface.shape) == (T, T) and tbary.dtype == torch.float32 and tuple(tbary.shape) == (T, T, 3)
        assert tface.is_contiguous() and tbary.is_contiguous()
        assert torch.equal((tface >= 0).to(torch.uint8), uv_chart_mask(face_uv, T)) and int((tface >= 0).sum()) > 0.2 * T * T
        assert int(tface.max()) < ft_.shape[0]
        want_f, want_b = G.texel_map(vt_, ft_, T)
        assert np.array_equal(tface.cpu().numpy(), want_f)
        inside = want_f >= 0
        d = np.abs(tbary.cpu().numpy()[inside] - want_b[inside]).max()
        print(f"{name} T={T}: texel_bary differs from the oracle raster's by at most {d:.3e}")
        assert d <= 2.0 ** -20                                        # barycentrics in [0, 1]: a few binary32 roundings


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_acc_untouched(dev):
    from contexture_nerf_amd import kal, _lib as L
    T, H, W, F, B = 16, 12, 10, 5, 2
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=dev)
    sentinel = torch.full((4, T, T), 0x5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    good = dict(values=z(B, H, W, 3), weight=z(B, H, W), face_idx=z(B, H, W, dtype=torch.int64), face_vertices_image=z(B, F, 3, 2),
                faces=z(F, 3, dtype=torch.int64), texel_face=z(T, T, dtype=torch.int64), texel_bary=z(T, T, 3), acc=sentinel.clone())
    bad = [
        ("device tensor", dict(values=torch.zeros(B, H, W, 3))),
        ("device tensor", dict(acc=torch.zeros(4, T, T, dtype=torch.int64))),
        ("dtype", dict(face_idx=z(B, H, W, dtype=torch.int32))),
        ("dtype", dict(acc=z(4, T, T))),
        ("dtype", dict(texel_face=z(T, T, dtype=torch.int32))),
        ("contiguous", dict(values=z(B, H, W, 6)[..., ::2])),
        ("contiguous", dict(weight=z(B, H, 2 * W)[..., ::2])),
        ("weight", dict(weight=z(B, H, W + 1))),
        ("face_idx", dict(face_idx=z(B, W, H, dtype=torch.int64))),
        ("face_vertices_image", dict(face_vertices_image=z(B, F + 1, 3, 2))),
        ("texel_bary", dict(texel_bary=z(T, T, 2))),
        ("acc", dict(acc=sentinel.clone()[:3].contiguous())),
        ("C=5", dict(values=z(B, H, W, 5), acc=torch.full((6, T, T), 0x5A5A5A5A5A5A, dtype=torch.int64, device=dev))),
    ]
    for match, change in bad:
        args = dict(good, **change)
        keep = args['acc'].clone()
        with pytest.raises(L.CtxError, match=match):
            kal.gather_fixed(**args)
        torch.cuda.synchronize()
        assert torch.equal(args['acc'], keep), match
    assert torch.equal(good['acc'], sentinel)
    # a short workspace, straight at the entry point
    lib = L.load()
    n = lib.ctx_uv_gather_ws_bytes(B, F)
    assert n == B * F and lib.ctx_uv_gather_ws_bytes(0, F) == -1 and lib.ctx_uv_gather_ws_bytes(B, 0) == -1
    ws = torch.zeros(n, dtype=torch.uint8, device=dev)
    g = good
    rc = lib.ctx_uv_gather_fixed(L.ptr(g['values']), L.ptr(g['weight']), L.ptr(g['face_idx']), L.ptr(g['face_vertices_image']), L.ptr(g['faces']),
                                 L.ptr(g['texel_face']), L.ptr(g['texel_bary']), B, H, W, 3, F, T, 32, L.ptr(g['acc']), L.ptr(ws), n - 1, L.stream())
    assert rc != 0 and b"workspace" in lib.ctx_last_error()
    torch.cuda.synchronize()
    assert torch.equal(good['acc'], sentinel)
    kal.gather_fixed(**good)                                           # and the good call runs: zero weights add nothing
    torch.cuda.synchronize()
    assert torch.equal(good['acc'], sentinel)


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------
def test_paint_with_gather_end_to_end(dev):
    from PIL import Image
    from contexture_nerf_amd import config as CFG
    from contexture_nerf_amd.trainer import ConTEXTure
    from test_pipeline_gpu import _tiny_sd
    cfg = CFG.TrainConfig()
    cfg.guide.text = "a test mesh"
    cfg.guide.shape_path = "shapes/spot_triangulated.obj"
    cfg.guide.texture_resolution = 128
    cfg.guide.guidance_scale = 10.0
    cfg.guide.sd_image_size = 128
    cfg.guide.num_inference_steps = 2
    cfg.render.train_grid_size = 160
    sd, _, _ = _tiny_sd(dev)
    tr = ConTEXTure(cfg, device=dev, diffusion=sd)
    T = 128
    s_atlas, s_cov = tr.paint()                                       # the default: the scatter
    tr.cfg.guide.projection = 'gather'
    atlas, cov = tr.paint()
    again = tr.paint()
    assert torch.equal(again[0], atlas) and torch.equal(again[1], cov)
    chart = tr.mesh_model.chart_mask() > 0
    tface, tbary = tr.mesh_model.texel_map()
    assert tface is tr.mesh_model.texel_map()[0] and torch.equal(tface >= 0, chart)             # cached; the chart mask
    assert tuple(atlas.shape) == (3, T, T) and bool(torch.isfinite(atlas).all()) and bool(torch.isfinite(cov).all())
    covered = cov > 0
    assert not bool((covered & ~chart).any()) and bool(covered.any())                           # nothing outside the charts
    g_empty, s_empty = int((chart & ~covered).sum()), int((chart & ~(s_cov > 0)).sum())
    print(f"tiny paint T={T}, 160^2: empty chart texels scatter {s_empty}, gather {g_empty} of {int(chart.sum())}")
    tr.cfg.guide.atlas_fill = 'nearest'
    filled, src = tr.complete_atlas()
    assert bool((src[chart] >= 0).all()) and bool(torch.isfinite(filled).all())
    with tempfile.TemporaryDirectory() as td:
        png = np.asarray(Image.open(os.path.join(tr.export(os.path.join(td, 'gather')), 'albedo.png')).convert('RGB'))
    assert png.shape == (T, T, 3)
    tr.cfg.guide.projection, tr.cfg.guide.atlas_fill = 'scatter', 'none'                        # and back: the scatter's bits again
    b_atlas, b_cov = tr.paint()
    assert torch.equal(b_atlas, s_atlas) and torch.equal(b_cov, s_cov)
