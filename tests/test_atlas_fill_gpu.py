"""GPU: the atlas-completion kernels (csrc/atlasfill.hip) against the numpy restatement of tests/test_atlas_fill_cpu.py.
Every comparison is array_equal on integers or a bit copy of floats: no tolerance anywhere.

4. kal.nearest_seed vs the restatement (random masks, single seeds in the corners, all / no seeds, one row, one column,
   a checkerboard = every tie case), and T = 4096 against scipy's exact EDT;
5. kal.atlas_fill on the spot case produced through the product path (kal raster at 1200^2 for the seven poses, kal.scatter_fixed,
   fixed_to_float), pads 0 / 2 / 8, plus the property checks that do not need the restatement;
6. the chart mask against the row-flipped atlas.rasterize_uv_counts for spot and a chart_atlas mesh (bunny);
7. end to end on the tiny UNet: paint() with the switch on, complete_atlas, export."""
import os
import tempfile
import numpy as np
import pytest
import torch

import test_atlas_fill_cpu as R

pytestmark = pytest.mark.gpu


def _gpu_nearest(seed_np, dev):
    from contexture_nerf_amd import kal
    src, d2 = kal.nearest_seed(torch.from_numpy(seed_np.astype(np.uint8)).to(dev))
    torch.cuda.synchronize()
    assert src.dtype == torch.int32 and d2.dtype == torch.int32
    return src.cpu().numpy().astype(np.int64), d2.cpu().numpy().astype(np.int64)


def _check_nearest(seed, dev, what):
    s, d = _gpu_nearest(seed, dev)
    ws, wd = R.nearest_seed(seed)
    assert np.array_equal(d, wd), f"{what}: d2 differs at {int((d != wd).sum())} texels"
    assert np.array_equal(s, ws), f"{what}: src differs at {int((s != ws).sum())} texels"


# ---- 4. nearest_seed ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [64, 257, 1024])
@pytest.mark.parametrize("density", [1e-4, 0.01, 0.5])
def test_nearest_seed_random_masks(dev, T, density):
    rng = np.random.default_rng(int(T * 7 + density * 1e5))
    _check_nearest(rng.random((T, T)) < density, dev, f"random T={T} density={density}")


@pytest.mark.parametrize("T", [64, 257])
def test_nearest_seed_special_masks(dev, T):
    for pos in [(0, 0), (0, T - 1), (T - 1, 0), (T - 1, T - 1)]:
        seed = np.zeros((T, T), bool); seed[pos] = True
        _check_nearest(seed, dev, f"single seed {pos}")
    _check_nearest(np.ones((T, T), bool), dev, "all seeds")
    s, d = _gpu_nearest(np.zeros((T, T), bool), dev)
    assert (s == -1).all() and (d == -1).all()
    seed = np.zeros((T, T), bool); seed[T // 3] = True
    _check_nearest(seed, dev, "one full row")
    seed = np.zeros((T, T), bool); seed[:, 2 * T // 3] = True
    _check_nearest(seed, dev, "one full column")
    yy, xx = np.mgrid[0:T, 0:T]
    _check_nearest((yy + xx) % 2 == 0, dev, "checkerboard")
    _check_nearest(((yy % 5 == 0) & (xx % 7 == 0)), dev, "lattice (ties at larger distances)")


def test_nearest_seed_single_corner_seed_1024(dev):
    """The worst case of the row walk (T reads per texel)."""
    T = 1024
    seed = np.zeros((T, T), bool); seed[T - 1, 0] = True
    s, d = _gpu_nearest(seed, dev)
    yy, xx = np.mgrid[0:T, 0:T]
    assert (s == (T - 1) * T).all() and np.array_equal(d, (yy - (T - 1)) ** 2 + xx ** 2)


def test_nearest_seed_4096_vs_scipy_edt(dev):
    from scipy import ndimage
    T = 4096
    seed = np.random.default_rng(4096).random((T, T)) < 0.01
    s, d = _gpu_nearest(seed, dev)
    edt = ndimage.distance_transform_edt(~seed)
    assert np.array_equal(d, np.rint(edt ** 2).astype(np.int64))
    sy, sx = s // T, s % T
    yy, xx = np.mgrid[0:T, 0:T]
    assert seed[sy, sx].all() and np.array_equal((yy - sy) ** 2 + (xx - sx) ** 2, d)      # src is a seed at that d2


def test_entry_points_refuse_bad_arguments(dev):
    from contexture_nerf_amd import kal, _lib as L
    with pytest.raises(L.CtxError, match="device tensor"):
        kal.nearest_seed(torch.zeros(8, 8, dtype=torch.uint8))
    with pytest.raises(L.CtxError, match="dtype"):
        kal.nearest_seed(torch.zeros(8, 8, device=dev))
    with pytest.raises(L.CtxError, match="contiguous"):
        kal.nearest_seed(torch.zeros(8, 16, dtype=torch.uint8, device=dev)[:, ::2])
    a, c, m = torch.zeros(3, 8, 8, device=dev), torch.zeros(8, 8, device=dev), torch.zeros(8, 8, dtype=torch.uint8, device=dev)
    with pytest.raises(L.CtxError, match="pad"):
        kal.atlas_fill(a, c, m, -1)
    with pytest.raises(L.CtxError, match="coverage"):
        kal.atlas_fill(a, torch.zeros(8, 4, device=dev), m, 1)
    assert L.load().ctx_atlas_fill_ws_bytes(0) == -1 and L.load().ctx_atlas_fill_ws_bytes(4097) == -1


# ---- the spot case through the product path ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spot(dev, meshes):
    """atlas [3,T,T], coverage [T,T] (device) of the seven poses at 1200^2, T = 1024, unit weights, and the oracle's coverage."""
    from contexture_nerf_amd import kal
    from contexture_nerf_amd.textured_mesh import uv_chart_mask
    T, H = 1024, 1200
    v, f, vt, ft, cam, proj = R.spot_arrays(meshes)
    verts = torch.tensor(np.repeat(v[None], 7, 0), device=dev)
    g_cam, g_img, _ = kal.render.mesh.prepare_vertices(verts, torch.tensor(f, device=dev), torch.tensor(proj),
                                                       camera_transform=torch.tensor(cam, device=dev))
    face_uv = torch.tensor(vt[ft][None], device=dev)
    uv, idx = kal.render.mesh.rasterize(H, H, g_cam[..., 2], g_img, face_uv.expand(7, -1, -1, -1).contiguous())
    g = torch.Generator().manual_seed(11)
    values = torch.cat([torch.rand(7, H, H, 3, generator=g), torch.ones(7, H, H, 1)], -1).to(dev).contiguous()
    acc = torch.zeros(4, T, T, dtype=torch.int64, device=dev)
    kal.scatter_fixed(values, uv.contiguous(), idx.contiguous(), acc)
    contrib = kal.fixed_to_float(acc)
    coverage = contrib[3].contiguous()
    atlas = (contrib[:3] / coverage.clamp_min(1e-8)).contiguous()
    chart = uv_chart_mask(face_uv, T)
    torch.cuda.synchronize()
    o_acc, _, _ = R.spot_coverage_oracle(meshes, T, H)
    return dict(T=T, atlas=atlas, coverage=coverage, chart=chart, acc=acc, oracle_cov=o_acc[0] > 0, vt=vt, ft=ft)


def test_atlas_fill_spot_case(dev, spot):
    from contexture_nerf_amd import kal
    T = spot['T']
    atlas, coverage, chart = spot['atlas'], spot['coverage'], spot['chart']
    a_np, c_np, m_np = atlas.cpu().numpy(), coverage.cpu().numpy(), chart.cpu().numpy() > 0
    cov = c_np > 0
    # the input of this test is the case whose hole statistics the feature was specified on
    assert np.array_equal(cov, spot['oracle_cov']), "product coverage mask differs from the oracle's"
    holes = int((m_np & ~cov).sum())
    print(f"spot T={T}: chart texels {int(m_np.sum())} (numpy mask: {R.SPOT_CHART_TEXELS}), stage A fills {holes} "
          f"(specified: {R.SPOT_HOLE_TEXELS})")
    nearest = R.CachedNearest()
    ident = np.arange(T * T).reshape(T, T)
    _, dB = nearest(m_np | cov)
    a_before, c_before = atlas.clone(), coverage.clone()
    for pad in (0, 2, 8):
        filled, src = kal.atlas_fill(atlas, coverage, chart, pad)
        torch.cuda.synchronize()
        f_np, s_np = filled.cpu().numpy(), src.cpu().numpy().astype(np.int64)
        want_f, want_s = R.atlas_fill(a_np, c_np, m_np, pad, nearest=nearest)
        n_pad = int(((s_np >= 0) & ~(m_np | cov)).sum())
        print(f"  pad {pad}: stage B fills {n_pad} (specified: {R.SPOT_PAD_TEXELS.get(pad, 0)})")
        assert np.array_equal(s_np, want_s), f"pad {pad}: src differs at {int((s_np != want_s).sum())} texels"
        assert np.array_equal(f_np.view(np.uint32), want_f.view(np.uint32)), f"pad {pad}: filled differs"
        # properties that hold without the restatement
        assert np.array_equal(s_np[cov], ident[cov]) and np.array_equal(f_np[:, cov].view(np.uint32), a_np[:, cov].view(np.uint32))
        assert (s_np[m_np] >= 0).all()
        assert cov.reshape(-1)[s_np[s_np >= 0]].all()
        assert not (s_np[dB > pad * pad] >= 0).any()                            # nothing farther than pad from chart | covered
        flat, sf = a_np.reshape(3, -1), s_np.reshape(-1)
        gathered = np.where(sf >= 0, flat[:, np.maximum(sf, 0)], flat)
        assert np.array_equal(f_np.reshape(3, -1).view(np.uint32), gathered.view(np.uint32))
    assert torch.equal(atlas, a_before) and torch.equal(coverage, c_before)    # inputs are not modified
    # nothing covered: the atlas comes back as it is
    f0, s0 = kal.atlas_fill(atlas, torch.zeros_like(coverage), chart, 8)
    assert torch.equal(f0, atlas) and bool((s0 == -1).all())


# ---- 6. chart mask ----------------------------------------------------------------------------------------------------------
def _border_only(gpu_mask, np_mask):
    """Every texel where the two differ has a 4-neighbour of the other value in the numpy mask."""
    diff = gpu_mask != np_mask
    p = np.pad(np_mask, 1, mode='edge')
    other = (p[:-2, 1:-1] != np_mask) | (p[2:, 1:-1] != np_mask) | (p[1:-1, :-2] != np_mask) | (p[1:-1, 2:] != np_mask)
    return int(diff.sum()), bool((other | ~diff).all())


def test_chart_mask_spot_and_coverage_inside(dev, spot):
    T = spot['T']
    gpu = spot['chart'].cpu().numpy() > 0
    ref = R.numpy_chart_mask(spot['vt'], spot['ft'], T)
    n, ok = _border_only(gpu, ref)
    cov = spot['coverage'].cpu().numpy() > 0
    inside = float((cov & gpu).sum()) / float(cov.sum())
    flipped = float((cov & gpu[::-1]).sum()) / float(cov.sum())
    print(f"spot chart mask: {n} texels differ from the float64 mask; coverage inside the mask {inside:.3f} "
          f"(other row order: {flipped:.3f}); chart texels covered {float((cov & gpu).sum()) / float(gpu.sum()):.3f}")
    assert ok
    assert inside >= 0.9


def test_chart_mask_chart_atlas_mesh(dev, meshes):
    from contexture_nerf_amd import atlas as A
    from contexture_nerf_amd.textured_mesh import uv_chart_mask
    T = 512
    vt, ft = A.chart_atlas(meshes["bunny_v"], meshes["bunny_f"], resolution=T)
    gpu = uv_chart_mask(torch.tensor(np.asarray(vt, np.float32)[np.asarray(ft, np.int64)][None], device=dev), T).cpu().numpy() > 0
    ref = R.numpy_chart_mask(vt, ft, T)
    n, ok = _border_only(gpu, ref)
    print(f"bunny chart mask T={T}: {int(gpu.sum())} chart texels, {n} differ from the float64 mask")
    assert ok and gpu.sum() > 0.2 * T * T


# ---- 7. end to end ----------------------------------------------------------------------------------------------------------
def test_paint_complete_export_end_to_end(dev):
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
    atlas0, cov0 = tr.paint()
    assert tr.atlas_filled is None and tr.atlas_fill_src is None
    with tempfile.TemporaryDirectory() as td:
        png_off = np.asarray(Image.open(os.path.join(tr.export(os.path.join(td, 'off')), 'albedo.png')).convert('RGB'))
    runs = []
    for _ in range(2):
        tr.cfg.guide.atlas_fill = 'nearest'
        atlas1, cov1 = tr.paint()
        assert torch.equal(atlas1, atlas0) and torch.equal(cov1, cov0)           # the switch does not touch paint()'s results
        assert torch.equal(tr.atlas, atlas0) and torch.equal(tr.atlas_coverage, cov0)
        runs.append((tr.atlas_filled.clone(), tr.atlas_fill_src.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    chart = tr.mesh_model.chart_mask()
    assert chart is tr.mesh_model.chart_mask() and chart.shape == (T, T) and chart.dtype == torch.uint8      # cached
    m_np, c_np = chart.cpu().numpy() > 0, cov0.cpu().numpy()
    want_f, want_s = R.atlas_fill(atlas0.cpu().numpy(), c_np, m_np, cfg.guide.atlas_pad)
    f_np, s_np = tr.atlas_filled.cpu().numpy(), tr.atlas_fill_src.cpu().numpy().astype(np.int64)
    assert np.array_equal(s_np, want_s) and np.array_equal(f_np.view(np.uint32), want_f.view(np.uint32))
    covered = c_np > 0
    assert (m_np & ~covered).sum() > 0 and (s_np[m_np] >= 0).all()
    with tempfile.TemporaryDirectory() as td:
        png_on = np.asarray(Image.open(os.path.join(tr.export(os.path.join(td, 'on')), 'albedo.png')).convert('RGB'))
    assert png_on.shape == (T, T, 3)
    w = s_np >= 0
    assert np.array_equal(png_on[w], png_on[s_np[w] // T, s_np[w] % T])          # every chart texel shows a painted texel's colour
    assert np.array_equal(png_on[covered], png_off[covered]) and np.array_equal(png_on[~w], png_off[~w])
    to8 = (np.clip(atlas0.cpu().numpy(), 0, 1) * 255).astype(np.uint8).transpose(1, 2, 0)
    assert np.array_equal(png_on[covered], to8[covered])
    tr.cfg.guide.atlas_fill = 'none'                                              # and back: today's outputs again
    tr.paint()
    assert tr.atlas_filled is None
    with tempfile.TemporaryDirectory() as td:
        again = np.asarray(Image.open(os.path.join(tr.export(os.path.join(td, 'off2')), 'albedo.png')).convert('RGB'))
    assert np.array_equal(again, png_off)
