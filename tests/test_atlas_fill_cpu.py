"""CPU: atlas completion (hole fill + chart-edge padding) — its definition, config surface and host control flow.

The numpy restatement below IS the definition the HIP kernels (csrc/atlasfill.hip) are held to; tests/test_atlas_fill_gpu.py
imports it from here.  Everything is an integer or bit-copy comparison: no tolerance anywhere.

  nearest_seed(seed[T,T] bool) -> (src, d2): per texel the seed (sy, sx) minimising (d2, sy, sx) lexicographically,
      d2 = (y-sy)^2 + (x-sx)^2; src = sy*T + sx; no seed at all -> -1 everywhere.
  atlas_fill(atlas, coverage, chart, pad) -> (filled, src): stage A fills chart & ~covered from the nearest covered texel,
      stage B pads texels within `pad` of chart | covered from the nearest of those; src = the covered texel a colour came from.

1. the restatement against a brute-force all-pairs minimum on small masks, and against scipy's exact EDT at T = 1024 on the
   spot coverage (the oracle's raster + scatter of the seven Zero123PlusDataset poses);
2. config: guide.atlas_fill / guide.atlas_pad defaults, CLI parsing, a bad value raises, every committed YAML still loads;
3. ConTEXTure.complete_atlas / _painted_texture / export and MeshBatchPainter.paint_all with kal.atlas_fill stubbed by the
   restatement: switch off -> the albedo.png bytes of the earlier formula; switch on -> filled texels equal their source texel."""
import glob
import os
import types
import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the numpy restatement ------------------------------------------------------------------------------------------------
BIG = 1 << 28


def col_pass(seed):                                   # nearest seed row per column, tie -> smaller row, -1 if none
    T = seed.shape[0]; ys = np.arange(T)[:, None]
    up = np.maximum.accumulate(np.where(seed, ys, -BIG), 0)
    dn = np.minimum.accumulate(np.where(seed, ys, BIG)[::-1], 0)[::-1]
    ny = np.where((ys - up) <= (dn - ys), up, dn)
    return np.where((up > -BIG) | (dn < BIG), ny, -1)


def nearest_seed(seed):                               # exact; minimises (d2, sy, sx); T <= 2048 with these 11-bit fields
    T = seed.shape[0]; ny = col_pass(seed); xs = np.arange(T)
    src = np.full((T, T), -1, np.int64); d2o = np.full((T, T), -1, np.int64)
    dx2 = (xs[:, None] - xs[None, :]) ** 2
    for y in range(T):
        g = np.where(ny[y] >= 0, (ny[y] - y) ** 2, BIG).astype(np.int64)
        key = ((dx2 + g[None, :]) << 22) | (np.where(ny[y] >= 0, ny[y], 0)[None, :] << 11) | xs[None, :]
        k = key.min(1); d2 = k >> 22; ok = d2 < BIG
        src[y] = np.where(ok, ((k >> 11) & 2047) * T + (k & 2047), -1); d2o[y] = np.where(ok, d2, -1)
    return src, d2o


def atlas_fill(atlas, coverage, chart, pad, nearest=nearest_seed):
    C, T, _ = atlas.shape; cov = coverage > 0; chart = chart > 0
    ident = np.arange(T * T).reshape(T, T)
    if not cov.any():
        return atlas.copy(), np.full((T, T), -1, np.int64)
    sA, _ = nearest(cov)
    src = np.where(cov, ident, np.where(chart, sA, -1))
    if pad > 0:
        seedB = chart | cov
        sB, dB = nearest(seedB)
        take = ~seedB & (dB >= 0) & (dB <= pad * pad)
        src = np.where(take, src.reshape(-1)[np.where(take, sB, 0)], src)
    flat = atlas.reshape(C, -1)
    filled = np.where(src.reshape(-1) >= 0, flat[:, np.maximum(src.reshape(-1), 0)], flat).reshape(C, T, T)
    return filled, src


class CachedNearest:
    """nearest_seed memoised on the mask's bytes: the three pads of one case share their two transforms (5.6 s each at 1024)."""

    def __init__(self):
        self.memo = {}

    def __call__(self, seed):
        k = (seed.shape, np.packbits(seed).tobytes())
        if k not in self.memo:
            self.memo[k] = nearest_seed(seed)
        return self.memo[k]


def brute_nearest(seed):
    """All-pairs minimum of (d2, sy, sx): the definition, O(T^4)."""
    T = seed.shape[0]
    sy, sx = np.nonzero(seed)                          # row-major: ascending (sy, sx)
    src = np.full((T, T), -1, np.int64); d2o = np.full((T, T), -1, np.int64)
    if sy.size == 0:
        return src, d2o
    yy, xx = np.mgrid[0:T, 0:T]
    d = (yy[..., None] - sy) ** 2 + (xx[..., None] - sx) ** 2          # [T,T,S]
    k = d.argmin(-1)                                   # first minimum = smallest (sy, sx) among equal d2
    return sy[k] * T + sx[k], np.take_along_axis(d, k[..., None], -1)[..., 0]


# ---- the spot case of the issue, from the oracle --------------------------------------------------------------------------
SPOT_THETA = np.deg2rad(np.float32([60, 60, 60, 60, 110, 110, 110])).astype(np.float32)      # Zero123PlusDataset poses
SPOT_PHI = np.deg2rad(np.float32([0, 30, 150, 270, 90, 210, 330])).astype(np.float32)
SPOT_CHART_TEXELS, SPOT_HOLE_TEXELS = 515124, 41806                  # counted at T = 1024 when the feature was specified
SPOT_PAD_TEXELS = {2: 19182, 4: 39635, 8: 81667}


def spot_arrays(meshes):
    from oracle import geometry as og
    v = og.normalize_mesh(meshes["spot_triangulated_v"], 0.6, 0.25)
    f = meshes["spot_triangulated_f"].astype(np.int64)
    vt = meshes["spot_triangulated_vt"].astype(np.float32)
    ft = meshes["spot_triangulated_ft"].astype(np.int64)
    cam = og.get_camera_from_multiple_view(SPOT_THETA, SPOT_PHI, np.full(7, 1.5, np.float32), 0.25)
    proj = og.generate_perspective_projection(np.pi / 3)
    return v, f, vt, ft, cam, proj


def spot_coverage_oracle(meshes, T=1024, H=1200):
    """-> (acc [1,T,T] int64 of the unit-weight scatter, uv [7,H,H,2], face_idx [7,H,H]) from oracle/geometry.py."""
    from oracle import geometry as og
    v, f, vt, ft, cam, proj = spot_arrays(meshes)
    o_cam, o_img, _ = og.prepare_vertices(np.repeat(v[None], 7, 0), f, proj, cam)
    uva = np.repeat(vt[ft][None], 7, 0)
    uv, idx = og.rasterize(H, H, o_cam[..., 2], o_img, uva)
    acc = og.uv_scatter_fixed(np.ones((7, H, H, 1), np.float32), uv, idx, T)
    return acc, uv, idx


def numpy_chart_mask(vt, ft, T):
    """Texel centre inside a UV triangle, rows in the texel convention of the scatter (y = (1 - v) * T)."""
    from contexture_nerf_amd import atlas as A
    return (A.rasterize_uv_counts(np.asarray(vt, np.float64), np.asarray(ft, np.int64), T)[0] > 0)[::-1].copy()


# ---- 1. the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,density", [(37, 0.001), (37, 0.05), (48, 0.01), (48, 0.3), (64, 0.003), (64, 0.1)])
def test_restatement_vs_brute_force(T, density):
    rng = np.random.default_rng(T * 1000 + int(density * 1e4))
    seed = rng.random((T, T)) < density
    s, d = nearest_seed(seed)
    bs, bd = brute_nearest(seed)
    assert np.array_equal(s, bs) and np.array_equal(d, bd)


def test_restatement_single_seed_empty_and_ties():
    T = 48
    for pos in [(0, 0), (0, T - 1), (T - 1, 0), (T - 1, T - 1), (17, 30)]:
        seed = np.zeros((T, T), bool); seed[pos] = True
        s, d = nearest_seed(seed)
        yy, xx = np.mgrid[0:T, 0:T]
        assert (s == pos[0] * T + pos[1]).all() and np.array_equal(d, (yy - pos[0]) ** 2 + (xx - pos[1]) ** 2)
    s, d = nearest_seed(np.zeros((T, T), bool))
    assert (s == -1).all() and (d == -1).all()
    yy, xx = np.mgrid[0:T, 0:T]
    checker = (yy + xx) % 2 == 0                        # every non-seed has 2..4 seeds at d2 = 1: the tie rule decides
    s, d = nearest_seed(checker)
    bs, bd = brute_nearest(checker)
    assert np.array_equal(s, bs) and np.array_equal(d, bd)


def test_restatement_atlas_fill_properties():
    rng = np.random.default_rng(3)
    T = 40
    yy, xx = np.mgrid[0:T, 0:T]
    chart = ((yy - 12) ** 2 + (xx - 14) ** 2 < 81) | ((yy > 25) & (yy < 36) & (xx > 20) & (xx < 37))
    cov = (chart & (rng.random((T, T)) < 0.6)).astype(np.float32) * rng.random((T, T)).astype(np.float32)
    cov[2, 30] = 0.5                                    # covered outside every chart
    atlas = rng.random((3, T, T)).astype(np.float32)
    covered = cov > 0
    for pad in (0, 1, 3):
        filled, src = atlas_fill(atlas, cov, chart, pad)
        ident = np.arange(T * T).reshape(T, T)
        assert np.array_equal(src[covered], ident[covered]) and (src[chart] >= 0).all()
        assert covered.reshape(-1)[src[src >= 0]].all()
        flat = atlas.reshape(3, -1)
        assert np.array_equal(filled.reshape(3, -1)[:, src.reshape(-1) >= 0], flat[:, src.reshape(-1)[src.reshape(-1) >= 0]])
        assert np.array_equal(filled[:, src < 0], atlas[:, src < 0])
        _, dB = brute_nearest(chart | covered)
        assert np.array_equal(src >= 0, dB <= pad * pad)
        # stage A sources are the brute-force nearest covered texels
        bs, _ = brute_nearest(covered)
        assert np.array_equal(src[chart & ~covered], bs[chart & ~covered])
    f0, s0 = atlas_fill(atlas, np.zeros((T, T), np.float32), chart, 4)
    assert np.array_equal(f0, atlas) and (s0 == -1).all()


def test_restatement_vs_scipy_edt_on_spot_coverage(meshes):
    from scipy import ndimage
    T = 1024
    acc, _, _ = spot_coverage_oracle(meshes, T)
    cov = acc[0] > 0
    vt, ft = meshes["spot_triangulated_vt"], meshes["spot_triangulated_ft"]
    chart = numpy_chart_mask(vt, ft, T)
    holes = int((chart & ~cov).sum())
    print(f"spot T={T}: chart texels {int(chart.sum())}, uncovered chart texels {holes}, covered in chart "
          f"{float((cov & chart).sum()) / max(int(cov.sum()), 1):.3f}")
    src, d2 = nearest_seed(cov)
    edt = ndimage.distance_transform_edt(~cov)
    assert np.array_equal(d2, np.rint(edt ** 2).astype(np.int64))
    sy, sx = src // T, src % T
    yy, xx = np.mgrid[0:T, 0:T]
    assert cov[sy, sx].all() and np.array_equal((yy - sy) ** 2 + (xx - sx) ** 2, d2)


# ---- 2. config ------------------------------------------------------------------------------------------------------------
def test_config_fields_defaults_cli_and_validation(tmp_path):
    from contexture_nerf_amd import config as CFG
    cfg = CFG.TrainConfig()
    assert cfg.guide.atlas_fill == 'none' and cfg.guide.atlas_pad == 8
    cfg = CFG.parse(argv=['--guide.atlas_fill=nearest', '--guide.atlas_pad=3'])
    assert cfg.guide.atlas_fill == 'nearest' and cfg.guide.atlas_pad == 3 and isinstance(cfg.guide.atlas_pad, int)
    with pytest.raises(ValueError, match="atlas_fill"):
        CFG.parse(argv=['--guide.atlas_fill=pushpull'])
    with pytest.raises(ValueError, match="atlas_pad"):
        CFG.parse(argv=['--guide.atlas_pad=-1'])
    y = tmp_path / "c.yaml"
    y.write_text("guide:\n  atlas_fill: nearest\n  atlas_pad: 0\n")
    cfg = CFG.parse(argv=[f'--config_path={y}'])
    assert cfg.guide.atlas_fill == 'nearest' and cfg.guide.atlas_pad == 0
    y.write_text("guide:\n  atlas_fill: blur\n")
    with pytest.raises(ValueError, match="atlas_fill"):
        CFG.parse(argv=[f'--config_path={y}'])
    CFG.dump(cfg, tmp_path / "d.yaml")
    assert CFG.parse(argv=[f'--config_path={tmp_path / "d.yaml"}']).guide.atlas_pad == 0


def test_committed_yamls_still_load():
    from contexture_nerf_amd import config as CFG
    paths = sorted(glob.glob(os.path.join(ROOT, "configs", "**", "*.yaml"), recursive=True))
    assert len(paths) >= 10
    loaded = 0
    for p in paths:
        if os.path.basename(p) in ("beachball.yaml", "mickey.yaml"):           # refused for a key GuideConfig never had, as before
            with pytest.raises(KeyError, match="guidance_scale_crossattn"):
                CFG.parse(argv=[f'--config_path={p}'])
            continue
        cfg = CFG.parse(argv=[f'--config_path={p}'])
        assert cfg.guide.atlas_fill == 'none' and cfg.guide.atlas_pad == 8
        loaded += 1
    assert loaded >= 10


# ---- 3. host control flow with the kernel stubbed at the kal seam ------------------------------------------------------------
def _stub_atlas_fill(calls):
    def fill(atlas, coverage, chart, pad):
        calls.append(int(pad))
        f, s = atlas_fill(atlas.numpy(), coverage.numpy(), chart.numpy(), int(pad))
        return torch.from_numpy(f), torch.from_numpy(s.astype(np.int32))
    return fill


class _MeshModel:
    """What complete_atlas / export touch of TexturedMeshModel; export_mesh is the product's own."""

    def __init__(self, T, chart, base):
        self.texture_resolution = T
        self._chart, self._base = torch.from_numpy(chart.astype(np.uint8)), torch.from_numpy(base)[None]
        self.mesh = types.SimpleNamespace(vertices=torch.zeros(3, 3), faces=torch.tensor([[0, 1, 2]]))
        self.vt, self.ft = torch.tensor([[0.1, 0.1], [0.9, 0.1], [0.1, 0.9]]), torch.tensor([[0, 1, 2]])

    def chart_mask(self):
        return self._chart

    def get_texture_map(self):
        return self._base, None

    def export_mesh(self, path, texture=None):
        from contexture_nerf_amd.textured_mesh import TexturedMeshModel
        return TexturedMeshModel.export_mesh(self, path, texture=texture)


def _trainer(T=24, seed=0):
    from contexture_nerf_amd import config as CFG
    from contexture_nerf_amd.trainer import ConTEXTure
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:T, 0:T]
    chart = (yy - 11) ** 2 + (xx - 12) ** 2 < 64
    cov = (chart & (rng.random((T, T)) < 0.7)).astype(np.float32) * (0.25 + rng.random((T, T)).astype(np.float32))
    tr = ConTEXTure.__new__(ConTEXTure)
    tr.cfg = CFG.TrainConfig(); tr.cfg.guide.texture_resolution = T
    tr.group, tr.rank, tr.world, tr.device = None, 0, 1, torch.device('cpu')
    tr.mesh_model = _MeshModel(T, chart, rng.random((3, T, T)).astype(np.float32))
    tr.atlas, tr.atlas_coverage = torch.from_numpy(rng.random((3, T, T)).astype(np.float32)), torch.from_numpy(cov)
    return tr, chart, cov > 0


def _png_pixels(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert('RGB'))


def test_export_switch_off_writes_the_earlier_bytes(tmp_path):
    from contexture_nerf_amd.mesh import write_textured_obj
    tr, chart, covered = _trainer()
    base = tr.mesh_model.get_texture_map()[0]
    cov = (tr.atlas_coverage > 0)[None, None].to(base.dtype)
    want = base * (1 - cov) + tr.atlas[None, :3] * cov                         # the formula export() had before this feature
    colors = (want.permute(0, 2, 3, 1).contiguous().clamp(0, 1)[0] * 255).to(torch.uint8).numpy()
    write_textured_obj(str(tmp_path / "want"), np.zeros((3, 3)), np.array([[0, 1, 2]]), tr.mesh_model.vt.numpy(), tr.mesh_model.ft.numpy(), colors)
    assert getattr(tr, 'atlas_filled', None) is None
    p = tr.export(tmp_path / "got")
    assert open(os.path.join(p, 'albedo.png'), 'rb').read() == open(tmp_path / "want" / "albedo.png", 'rb').read()
    assert torch.equal(tr._painted_texture(base), want)


def test_complete_atlas_and_export_switch_on(tmp_path, monkeypatch):
    from contexture_nerf_amd import kal
    calls = []
    monkeypatch.setattr(kal, 'atlas_fill', _stub_atlas_fill(calls))
    tr, chart, covered = _trainer()
    tr.cfg.guide.atlas_fill, tr.cfg.guide.atlas_pad = 'nearest', 2
    atlas0, cov0 = tr.atlas.clone(), tr.atlas_coverage.clone()
    filled, src = tr.complete_atlas()
    assert calls == [2] and filled is tr.atlas_filled and src is tr.atlas_fill_src and src.dtype == torch.int32
    assert torch.equal(tr.atlas, atlas0) and torch.equal(tr.atlas_coverage, cov0)          # inputs are not modified
    want_f, want_s = atlas_fill(atlas0.numpy(), cov0.numpy(), chart, 2)
    assert np.array_equal(filled.numpy(), want_f) and np.array_equal(src.numpy(), want_s)
    off = tmp_path / "off"; on = tmp_path / "on"
    tr2, _, _ = _trainer()
    png_off = _png_pixels(os.path.join(tr2.export(off), 'albedo.png'))
    png_on = _png_pixels(os.path.join(tr.export(on), 'albedo.png'))
    T = chart.shape[0]
    s = src.numpy()
    holes = chart & ~covered
    assert holes.sum() > 10 and (s[chart] >= 0).all()
    sy, sx = s[holes] // T, s[holes] % T
    assert np.array_equal(png_on[holes], png_on[sy, sx])                       # a filled texel shows its source texel's colour
    assert np.array_equal(png_on[covered], png_off[covered])                   # painted texels as before
    assert np.array_equal(png_on[s < 0], png_off[s < 0])                        # beyond the padding: the texture field, as before
    assert not np.array_equal(png_on[holes], png_off[holes])
    tr.complete_atlas(pad=0)
    assert calls == [2, 0] and np.array_equal(tr.atlas_fill_src.numpy() >= 0, chart | covered)


def test_paint_all_calls_complete_atlas_only_when_switched_on(monkeypatch):
    import test_dist_product_cpu as P
    from contexture_nerf_amd import _lib as L, kal
    monkeypatch.setattr(L, 'load', lambda: P.FakeLib())
    monkeypatch.setattr(L, 'ptr', lambda t, dtype=None, name="tensor": t)
    monkeypatch.setattr(L, 'stream', lambda: None)
    monkeypatch.setattr(L, 'f32c', lambda t, device=None: t.to(torch.float32).contiguous())
    calls = []
    monkeypatch.setattr(kal, 'atlas_fill', _stub_atlas_fill(calls))
    chart = np.zeros((P.T, P.T), bool); chart[1:7, 1:6] = True
    res = {}
    for mode in ('none', 'nearest'):
        tr = P.make_trainer(0, 1, 3)
        tr.cfg.guide.atlas_fill, tr.cfg.guide.atlas_pad = mode, 1
        tr.mesh_model.chart_mask = lambda: torch.from_numpy(chart.astype(np.uint8))
        res[mode] = tr.paint() + (tr,)
    (a0, c0, t0), (a1, c1, t1) = res['none'], res['nearest']
    assert calls == [1]
    assert torch.equal(a0, a1) and torch.equal(c0, c1)                          # paint() returns what it returned before
    assert t0.atlas_filled is None and t0.atlas_fill_src is None
    want_f, want_s = atlas_fill(a1.numpy(), c1.numpy(), chart, 1)
    assert np.array_equal(t1.atlas_filled.numpy(), want_f) and np.array_equal(t1.atlas_fill_src.numpy(), want_s)
    assert torch.equal(t1.atlas, a1) and torch.equal(t1.atlas_coverage, c1)
    tr = P.make_trainer(0, 1, 1)
    tr.cfg.guide.atlas_fill = 'blur'
    with pytest.raises(ValueError, match="atlas_fill"):
        tr.paint()
