"""CPU: UV back-projection by texel-side gather — its definition, what it buys over the scatter, config surface and host control flow.

The numpy restatement `uv_gather_fixed` below IS the definition csrc/uvgather.hip is held to; tests/test_uv_gather_gpu.py imports it
from here and compares the int64 sums with array_equal.  All float arithmetic is binary32 in the order of the kernel (numpy array
operations round every product and sum on their own: no contraction).

  texel_map(vt, ft, T)      the UV triangles drawn at T x T by the oracle raster with the identity as face features
                            -> (texel_face [T,T] int64, texel_bary [T,T,3] f32); TexturedMeshModel.texel_map on the CPU.
  uv_gather_fixed(...)      per chart texel and view: own pixel, projection, related owner at the nearest pixel, bilinear colour over
                            the taps a related face owns, nearest weight, integer sum.

1. properties of the restatement (background view, empty texel map, constant colour, chart only, 3 + 4 split);
2. the spot case at T = 1024, 1200^2: empty chart texels against the scatter's (a condition), the counts pinned;
3. accuracy against the analytic truth at (1024, 1200^2) and (256, 301 x 257), relative to the scatter's;
4. config: guide.projection default, CLI, a bad value, the committed YAMLs;
5. host control flow with kal.gather_fixed / kal.scatter_fixed stubbed at the kal seam."""
import glob
import os
import numpy as np
import pytest
import torch

import test_atlas_fill_cpu as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
FRAC = 32


# ---- the numpy restatement ------------------------------------------------------------------------------------------------
def texel_map(vt, ft, T):
    from oracle import geometry as og
    xy = (np.asarray(vt, f32)[np.asarray(ft, np.int64)][None] * f32(2) - f32(1)).astype(f32)
    z = np.full(xy.shape[:3], -1.0, f32)
    eye = np.ascontiguousarray(np.broadcast_to(np.eye(3, dtype=f32), (1, xy.shape[1], 3, 3)))
    bary, idx = og.rasterize(T, T, z, xy, eye)
    return idx[0].copy(), bary[0].copy()


def _related(faces, f, g):
    """g is a face and equals f or shares a vertex id with it (elementwise over arrays of face ids)."""
    F = faces.shape[0]
    ok = (g >= 0) & (g < F)
    a, b = faces[f], faces[np.clip(g, 0, F - 1)]
    return ok & ((g == f) | (a[:, :, None] == b[:, None, :]).any((1, 2)))


def uv_gather_fixed(texel_face, texel_bary, faces, fvi, face_idx, values, weight=None, frac_bits=FRAC, acc=None):
    """-> acc [C+1,T,T] int64 (+= when given).  texel_face [T,T] i64, texel_bary [T,T,3] f32, faces [F,3] i64, fvi [B,F,3,2] f32,
    face_idx [B,H,W] i64, values [B,H,W,C] f32, weight [B,H,W] f32 | None."""
    T = texel_face.shape[0]
    B, H, W = face_idx.shape
    C, F = values.shape[-1], faces.shape[0]
    values, fvi = np.asarray(values, f32), np.asarray(fvi, f32)
    if acc is None:
        acc = np.zeros((C + 1, T, T), np.int64)
    ty, tx = np.nonzero((texel_face >= 0) & (texel_face < F))
    f_all, b_all = texel_face[ty, tx], np.asarray(texel_bary, f32)[ty, tx]
    one, two, half = f32(1), f32(2), f32(0.5)
    with np.errstate(all='ignore'):
        for v in range(B):
            idx = face_idx[v]
            own = np.zeros(F, bool)
            own[idx[(idx >= 0) & (idx < F)]] = True
            # 1. own pixel
            k = np.nonzero(own[f_all])[0]
            f, b = f_all[k], b_all[k]
            # 2. projection
            q = fvi[v][f]
            X = (b[:, 0] * q[:, 0, 0] + b[:, 1] * q[:, 1, 0]) + b[:, 2] * q[:, 2, 0]
            Y = (b[:, 0] * q[:, 0, 1] + b[:, 1] * q[:, 1, 1]) + b[:, 2] * q[:, 2, 1]
            px = ((X + one) * f32(W) - one) / two
            py = ((one - Y) * f32(H) - one) / two
            fxn, fyn = np.floor(px + half), np.floor(py + half)
            k2 = np.nonzero((fxn >= 0) & (fxn < W) & (fyn >= 0) & (fyn < H))[0]
            k, f, px, py = k[k2], f[k2], px[k2], py[k2]
            xn, yn = fxn[k2].astype(np.int64), fyn[k2].astype(np.int64)
            # 3. visibility
            k2 = np.nonzero(_related(faces, f, idx[yn, xn]))[0]
            k, f, px, py, xn, yn = k[k2], f[k2], px[k2], py[k2], xn[k2], yn[k2]
            # 4. colour
            x0, y0 = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
            x1, y1 = x0 + 1, y0 + 1
            fx0, fy0, fx1, fy1 = x0.astype(f32), y0.astype(f32), x1.astype(f32), y1.astype(f32)
            taps = ((x0, y0, (fx1 - px) * (fy1 - py)), (x1, y0, (px - fx0) * (fy1 - py)),
                    (x0, y1, (fx1 - px) * (py - fy0)), (x1, y1, (px - fx0) * (py - fy0)))
            s = np.zeros(len(k), f32)
            num = np.zeros((len(k), C), f32)
            for xs, ys, w in taps:
                inside = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
                xc, yc = np.clip(xs, 0, W - 1), np.clip(ys, 0, H - 1)
                cnt = inside & _related(faces, f, np.where(inside, idx[yc, xc], -1))
                s = np.where(cnt, s + w, s)
                num = np.where(cnt[:, None], num + values[v, yc, xc] * w[:, None], num)
            col = num / s[:, None]
            # 5. weight
            om = np.ones(len(k), f32) if weight is None else np.asarray(weight, f32)[v, yn, xn]
            k2 = np.nonzero((om != 0) & np.isfinite(om) & np.isfinite(col).all(1))[0]
            k, col, om = k[k2], col[k2], om[k2]
            # 6. sum
            for c in range(C):
                acc[c, ty[k], tx[k]] += np.rint(np.ldexp(col[:, c] * om, frac_bits).astype(np.float64)).astype(np.int64)
            acc[C, ty[k], tx[k]] += np.rint(np.ldexp(om, frac_bits).astype(np.float64)).astype(np.int64)
    return acc


# ---- the spot case ----------------------------------------------------------------------------------------------------------
def spot_scene(meshes, H, W, shape_scale=0.6):
    """The seven Zero123PlusDataset poses of spot from the oracle -> dict(v, f, vt, ft, fvi [7,F,3,2], face_idx [7,H,W], uv [7,H,W,2])."""
    from oracle import geometry as og
    v, f, vt, ft, cam, proj = R.spot_arrays(meshes)
    if shape_scale != 0.6:
        v = og.normalize_mesh(meshes["spot_triangulated_v"], shape_scale, 0.25)
    o_cam, o_img, _ = og.prepare_vertices(np.repeat(v[None], 7, 0), f, proj, cam)
    uv, idx = og.rasterize(H, W, o_cam[..., 2], o_img, np.repeat(vt[ft][None], 7, 0))
    return dict(v=v, f=f, vt=vt, ft=ft, fvi=o_img, face_idx=idx, uv=uv, z=o_cam[..., 2])


def position_colours(v):
    """Vertex colour = vertex position scaled per axis to [0, 1]."""
    lo, hi = v.min(0), v.max(0)
    return ((v - lo) / (hi - lo)).astype(f32)


def painted_views(scene, H, W, background=0.5):
    """The oracle raster of the vertex colours (perspective-correct, as any other face feature), background 0.5."""
    from oracle import geometry as og
    col = position_colours(scene['v'])
    img, idx = og.rasterize(H, W, scene['z'], scene['fvi'], np.repeat(col[scene['f']][None], scene['fvi'].shape[0], 0))
    return np.where((idx >= 0)[..., None], img, f32(background)).astype(f32)


def truth_atlas(scene, tface, tbary):
    col = position_colours(scene['v'])
    cf = col[scene['f']][np.clip(tface, 0, None)]                         # [T,T,3 corners,3]
    return (tbary[..., None].astype(np.float64) * cf).sum(2)              # [T,T,3]


def both_ways(scene, T, values):
    """-> (scatter acc, gather acc, texel_face, texel_bary): unit weight, C = 3 colours + weight."""
    from oracle import geometry as og
    tface, tbary = texel_map(scene['vt'], scene['ft'], T)
    ones = np.ones(values.shape[:3] + (1,), f32)
    sc = og.uv_scatter_fixed(np.concatenate([values, ones], -1), scene['uv'], scene['face_idx'], T)
    ga = uv_gather_fixed(tface, tbary, scene['f'], scene['fvi'], scene['face_idx'], values)
    return sc, ga, tface, tbary


def mean_abs_errors(sc, ga, truth):
    both = (sc[3] > 0) & (ga[3] > 0)
    es = np.abs(sc[:3, both].T / sc[3, both][:, None].astype(np.float64) - truth[both]).mean()
    eg = np.abs(ga[:3, both].T / ga[3, both][:, None].astype(np.float64) - truth[both]).mean()
    return float(es), float(eg), int(both.sum())


SPOT_SCATTER_EMPTY, SPOT_GATHER_EMPTY = 41807, 9026             # chart texels at T = 1024, seven poses at 1200^2, counted by the restatement
SPOT_ONLY_GATHER, SPOT_ONLY_SCATTER = 33251, 470                # scatter-empty & gather-covered; gather-empty & scatter-covered


@pytest.fixture(scope="module")
def spot_1024(meshes):
    H = 1200
    scene = spot_scene(meshes, H, H)
    values = painted_views(scene, H, H)
    return (scene, values) + both_ways(scene, 1024, values)


@pytest.fixture(scope="module")
def small(meshes):
    """T = 64, 97 x 131: the size of the property tests."""
    H, W, T = 97, 131, 64
    scene = spot_scene(meshes, H, W)
    tface, tbary = texel_map(scene['vt'], scene['ft'], T)
    return scene, painted_views(scene, H, W), tface, tbary


# ---- 1. properties ----------------------------------------------------------------------------------------------------------
def test_background_view_and_empty_texel_map_contribute_nothing(small):
    scene, values, tface, tbary = small
    rng = np.random.default_rng(0)
    sentinel = rng.integers(-1 << 40, 1 << 40, (4,) + tface.shape)
    bg = np.full_like(scene['face_idx'][:1], -1)
    acc = uv_gather_fixed(tface, tbary, scene['f'], scene['fvi'][:1], bg, values[:1], acc=sentinel.copy())
    assert np.array_equal(acc, sentinel)
    acc = uv_gather_fixed(np.full_like(tface, -1), tbary, scene['f'], scene['fvi'], scene['face_idx'], values, acc=sentinel.copy())
    assert np.array_equal(acc, sentinel)
    # a background view among painted ones adds nothing to them
    idx = scene['face_idx'].copy(); idx[2] = -1
    keep = [0, 1, 3, 4, 5, 6]
    a = uv_gather_fixed(tface, tbary, scene['f'], scene['fvi'], idx, values)
    b = uv_gather_fixed(tface, tbary, scene['f'], scene['fvi'][keep], idx[keep], values[keep])
    assert np.array_equal(a, b) and (a[3] > 0).any()


def test_constant_colour_chart_only_and_split(small):
    scene, values, tface, tbary = small
    rng = np.random.default_rng(1)
    mask = (rng.random(scene['face_idx'].shape) < 0.8).astype(f32)
    for w in (None, mask):
        acc = uv_gather_fixed(tface, tbary, scene['f'], scene['fvi'], scene['face_idx'], np.full_like(values, 0.5), w)
        touched = acc[3] != 0
        assert touched.sum() > 500 and not (touched & (tface < 0)).any()
        for c in range(3):                                            # a power of two commutes with every rounding
            assert np.array_equal(acc[c][touched], acc[3][touched] // 2) and not acc[c][~touched].any()
        assert (acc[3][touched] % (1 << FRAC) == 0).all() and acc[3].max() <= 7 << FRAC
    wf = rng.random(scene['face_idx'].shape).astype(f32)
    one = uv_gather_fixed(tface, tbary, scene['f'], scene['fvi'], scene['face_idx'], values, wf)
    assert not one[:, tface < 0].any()                                # no texel outside the chart is ever touched
    part = uv_gather_fixed(tface, tbary, scene['f'], scene['fvi'][:3], scene['face_idx'][:3], values[:3], wf[:3])
    part = uv_gather_fixed(tface, tbary, scene['f'], scene['fvi'][3:], scene['face_idx'][3:], values[3:], wf[3:], acc=part)
    assert np.array_equal(part, one)
    # colours stay inside the hull of the painted values: the taps' weights are normalised
    cov = one[3] > 0
    col = one[:3, cov] / one[3, cov].astype(np.float64)
    assert col.min() >= values.min() - 1e-6 and col.max() <= values.max() + 1e-6


def test_texel_map_is_the_chart_mask(meshes, small):
    scene, _, tface, tbary = small
    T = tface.shape[0]
    assert np.array_equal(tface >= 0, R.numpy_chart_mask(scene['vt'], scene['ft'], T))
    inside = tface >= 0
    assert np.abs(tbary[inside].sum(-1) - 1).max() < 1e-5 and tbary[inside].min() > -1e-5
    # the barycentrics reproduce the texel centre from the face's UV corners
    uvc = (tbary[inside][:, :, None] * scene['vt'][scene['ft']][tface[inside]]).sum(1)
    yy, xx = np.nonzero(inside)
    assert np.abs(uvc[:, 0] - (xx + 0.5) / T).max() < 1e-5 and np.abs(uvc[:, 1] - (1 - (yy + 0.5) / T)).max() < 1e-5


# ---- 2. / 3. the spot case ---------------------------------------------------------------------------------------------------
def test_spot_gather_leaves_far_fewer_empty_texels(spot_1024):
    scene, values, sc, ga, tface, tbary = spot_1024
    chart = tface >= 0
    s_cov, g_cov = sc[3] > 0, ga[3] > 0
    s_empty, g_empty = int((chart & ~s_cov).sum()), int((chart & ~g_cov).sum())
    only_g, only_s = int((chart & ~s_cov & g_cov).sum()), int((chart & s_cov & ~g_cov).sum())
    print(f"spot T=1024 1200^2: chart {int(chart.sum())}, scatter empty {s_empty}, gather empty {g_empty} ({g_empty / chart.sum():.4f}), "
          f"scatter-empty gather-covered {only_g}, gather-empty scatter-covered {only_s}, scatter outside chart {int((s_cov & ~chart).sum())}")
    assert g_empty <= 0.30 * s_empty
    assert not (g_cov & ~chart).any() and (s_cov & ~chart).any()       # the splat writes outside the charts, the gather never
    assert int(chart.sum()) == R.SPOT_CHART_TEXELS
    assert (s_empty, g_empty, only_g, only_s) == (SPOT_SCATTER_EMPTY, SPOT_GATHER_EMPTY, SPOT_ONLY_GATHER, SPOT_ONLY_SCATTER)


def test_spot_accuracy_at_1024(spot_1024):
    scene, values, sc, ga, tface, tbary = spot_1024
    es, eg, n = mean_abs_errors(sc, ga, truth_atlas(scene, tface, tbary))
    print(f"T=1024 1200^2: mean abs error scatter {es:.4e}, gather {eg:.4e} ({eg / es:.3f} x) on {n} texels")
    assert eg <= 1.25 * es


def test_spot_accuracy_at_256(meshes):
    H, W, T = 301, 257, 256
    scene = spot_scene(meshes, H, W)
    sc, ga, tface, tbary = both_ways(scene, T, painted_views(scene, H, W))
    es, eg, n = mean_abs_errors(sc, ga, truth_atlas(scene, tface, tbary))
    print(f"T=256 301x257: mean abs error scatter {es:.4e}, gather {eg:.4e} ({eg / es:.3f} x) on {n} texels")
    assert eg <= 1.0 * es


# ---- 4. config ---------------------------------------------------------------------------------------------------------------
def test_config_projection_default_cli_and_validation(tmp_path):
    from contexture_nerf_amd import config as CFG
    assert CFG.TrainConfig().guide.projection == 'scatter'
    assert CFG.parse(argv=[]).guide.projection == 'scatter'
    assert CFG.parse(argv=['--guide.projection=gather']).guide.projection == 'gather'
    with pytest.raises(ValueError, match="projection"):
        CFG.parse(argv=['--guide.projection=splat'])
    y = tmp_path / "c.yaml"
    y.write_text("guide:\n  projection: gather\n  atlas_fill: nearest\n")
    cfg = CFG.parse(argv=[f'--config_path={y}'])
    assert cfg.guide.projection == 'gather' and cfg.guide.atlas_fill == 'nearest'
    y.write_text("guide:\n  projection: both\n")
    with pytest.raises(ValueError, match="projection"):
        CFG.parse(argv=[f'--config_path={y}'])
    CFG.dump(cfg, tmp_path / "d.yaml")
    assert CFG.parse(argv=[f'--config_path={tmp_path / "d.yaml"}']).guide.projection == 'gather'


def test_committed_yamls_load_with_the_scatter():
    from contexture_nerf_amd import config as CFG
    paths = sorted(glob.glob(os.path.join(ROOT, "configs", "**", "*.yaml"), recursive=True))
    assert len(paths) == 12
    loaded = 0
    for p in paths:
        if os.path.basename(p) in ("beachball.yaml", "mickey.yaml"):           # refused for a key GuideConfig never had, as before
            with pytest.raises(KeyError, match="guidance_scale_crossattn"):
                CFG.parse(argv=[f'--config_path={p}'])
            continue
        assert CFG.parse(argv=[f'--config_path={p}']).guide.projection == 'scatter'
        loaded += 1
    assert loaded == 10


# ---- 5. host control flow with the kernels stubbed at the kal seam -----------------------------------------------------------
def _stub_kal(monkeypatch, calls):
    import test_dist_product_cpu as P
    from contexture_nerf_amd import _lib as L, kal
    monkeypatch.setattr(L, 'load', lambda: P.FakeLib())
    monkeypatch.setattr(L, 'ptr', lambda t, dtype=None, name="tensor": t)
    monkeypatch.setattr(L, 'stream', lambda: None)
    monkeypatch.setattr(L, 'f32c', lambda t, device=None: t.to(torch.float32).contiguous())

    def gather(values, weight, face_idx, fvi, faces, texel_face, texel_bary, acc, frac_bits=kal.SCATTER_FRAC_BITS):
        B, H, W, C = values.shape
        assert values.dtype == torch.float32 and values.is_contiguous() and C == 3
        assert weight.dtype == torch.float32 and tuple(weight.shape) == (B, H, W) == tuple(face_idx.shape)
        assert tuple(fvi.shape) == (B, faces.shape[0], 3, 2) and faces.dtype == torch.int64
        assert texel_face.dtype == torch.int64 and tuple(texel_bary.shape) == tuple(texel_face.shape) + (3,)
        assert acc.dtype == torch.int64 and tuple(acc.shape) == (4,) + tuple(texel_face.shape)
        calls.append(('gather', float(values.sum()), float(weight.sum())))
        acc[3] += (texel_face >= 0) * int(weight.sum())                 # a stand-in: coverage on the chart only
        acc[:3] += (texel_face >= 0) * 7
        return acc
    real_scatter = kal.scatter_fixed

    def scatter(values, uv, mask_idx, acc, frac_bits=kal.SCATTER_FRAC_BITS, reuse=False):
        calls.append(('scatter', float(values[..., :3].sum()), float(values[..., 3].sum())))
        return real_scatter(values, uv, mask_idx, acc, frac_bits, reuse)
    monkeypatch.setattr(kal, 'gather_fixed', gather)
    monkeypatch.setattr(kal, 'scatter_fixed', scatter)
    return P


def _gather_trainer(P, n_views, projection):
    tr = P.make_trainer(0, 1, n_views)
    tr.cfg.guide.projection = projection
    tface = torch.full((P.T, P.T), -1, dtype=torch.int64); tface[1:7, 1:6] = 3
    tr.mesh_model.texel_map = lambda: (tface, torch.full((P.T, P.T, 3), 1 / 3))
    prep = tr._paint_prepare

    def prep_with_fvi(data, image_size=None, num_inference_steps=None):
        kw, ctx = prep(data, image_size, num_inference_steps)
        ctx['render_cache']['face_vertices_image'] = torch.zeros(1, P.F, 3, 2)
        return kw, ctx
    tr._paint_prepare = prep_with_fvi
    return tr, tface


def test_paint_selects_the_projection(monkeypatch):
    calls = []
    P = _stub_kal(monkeypatch, calls)
    tr, tface = _gather_trainer(P, 3, 'gather')
    atlas, cov = tr.paint()
    assert [c[0] for c in calls] == ['gather'] * 3                       # once per painted item, the scatter never
    assert np.array_equal(cov.numpy() > 0, tface.numpy() >= 0)
    calls.clear()
    tr, _ = _gather_trainer(P, 3, 'scatter')
    a0, c0 = tr.paint()
    assert [c[0] for c in calls] == ['scatter'] * 3
    calls.clear()
    plain = P.make_trainer(0, 1, 3)                                       # a trainer as earlier builds made it: the same bits
    a1, c1 = plain.paint()
    assert [c[0] for c in calls] == ['scatter'] * 3 and torch.equal(a0, a1) and torch.equal(c0, c1)
    tr.cfg.guide.projection = 'splat'
    with pytest.raises(ValueError, match="projection"):
        tr.paint()


def test_project_back_selects_the_projection(monkeypatch):
    calls = []
    P = _stub_kal(monkeypatch, calls)
    from contexture_nerf_amd import kal
    monkeypatch.setattr(kal, 'fixed_to_float', lambda acc, frac_bits=32, out=None: (acc.double() * 2.0 ** -frac_bits).float())
    monkeypatch.setattr(kal.render.mesh, 'texture_mapping', lambda uv, tex, mode='bilinear', mask_idx=None: torch.zeros(uv.shape[:3] + (tex.shape[1],)))
    for mode in ('gather', 'scatter'):
        calls.clear()
        tr, _ = _gather_trainer(P, 1, mode)
        _, ctx = tr._paint_prepare(tr.train_views[0])
        out = tr.project_back(ctx['render_cache'], torch.zeros(3), ctx['rgb'], ctx['object_mask'], ctx['object_mask'])
        assert [c[0] for c in calls] == [mode] and tuple(out.shape) == (1, 3, P.H, P.W)
        assert calls[0][2] == float((ctx['object_mask'] > 0).sum())


def test_host_tensors_are_refused():
    from contexture_nerf_amd import _lib as L, kal
    T, H, W, F = 8, 6, 5, 4
    args = dict(values=torch.zeros(1, H, W, 3), weight=None, face_idx=torch.zeros(1, H, W, dtype=torch.int64),
                face_vertices_image=torch.zeros(1, F, 3, 2), faces=torch.zeros(F, 3, dtype=torch.int64),
                texel_face=torch.zeros(T, T, dtype=torch.int64), texel_bary=torch.zeros(T, T, 3), acc=torch.zeros(4, T, T, dtype=torch.int64))
    with pytest.raises(L.CtxError, match="device tensor"):
        kal.gather_fixed(**args)
