"""GPU: baking the 3-D field into the UV atlas (csrc/bake.hip) against tests/bake_rule.py.

1. ctx_texel_rays == the rule, array_equal, on spot: T in {32, 97}, s in 1..4, the whole chart, a list with -1, T*T and off-chart texels,
   a mesh with a face and a UV triangle without area, lengths 1 / 255 / 256 / 257; outputs between guards;
2. ctx_bake_resolve == the rule, array_equal on int64: NaN, +-inf, alpha just under and over the cut, an acc that holds sums;
3. refusals leave sentinel-filled outputs untouched;
4. bake_atlas against the float64 chain bake_rule + march_rule (rtol 2e-4; coverage equal); twice, side stream, chunks;
5. the round trip: a textured spot -> nine teacher views -> HashGridField by fit_views -> bake_field -> the baked mesh rendered again;
6. the trainer end to end: bake_field, complete_atlas, export; paint() untouched."""
import os
import tempfile
import numpy as np
import pytest
import torch

import bake_rule as B
import march_rule as mr
import test_atlas_fill_cpu as R
import test_uv_gather_cpu as G
from test_engine_ops_gpu import Out

pytestmark = pytest.mark.gpu
f32 = np.float32
SHELL = 0.03
_MAPS = {}


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def spot_case(meshes, T):
    """spot with its texel map at T, and a copy with one face and one UV triangle without area (both on the chart)."""
    if T not in _MAPS:
        v, f, vt, ft, _, _ = R.spot_arrays(meshes)
        tface, tbary = G.texel_map(vt, ft, T)
        chart = np.nonzero(tface.reshape(-1) >= 0)[0].astype(np.int32)
        off = np.nonzero(tface.reshape(-1) < 0)[0].astype(np.int32)
        fa, fb = int(tface.reshape(-1)[chart[len(chart) // 3]]), int(tface.reshape(-1)[chart[2 * len(chart) // 3]])
        assert fa != fb
        f2, uv2 = f.copy(), vt[ft].astype(f32).copy()
        f2[fa, 2] = f2[fa, 1]
        uv2[fb, 2] = uv2[fb, 1]
        _MAPS[T] = dict(v=v.astype(f32), f=f, uv=vt[ft].astype(f32), tface=tface, tbary=tbary, chart=chart, off=off, f_flat=f2, uv_flat=uv2)
    return _MAPS[T]


def gpu_rays(dev, c, faces, uv, idx, s, h=SHELL):
    """ctx_texel_rays into guarded, NaN-filled outputs -> numpy (o, d, valid)."""
    from contexture_nerf_amd import _lib as L
    lib = L.load()
    n = len(idx)
    R_ = n * s * s
    o, d, va = Out(dev, (R_, 3), torch.float32), Out(dev, (R_, 3), torch.float32), Out(dev, (R_,), torch.uint8)
    ten = [_t(dev, c['tface']), _t(dev, c['tbary']), _t(dev, uv), _t(dev, c['v']), _t(dev, faces), _t(dev, np.asarray(idx, np.int32))]
    T = c['tface'].shape[0]
    L.check(lib.ctx_texel_rays(*[L.ptr(x) for x in ten], n, T, faces.shape[0], c['v'].shape[0], s, h, L.ptr(o.t), L.ptr(d.t), L.ptr(va.t),
                               L.stream()))
    return o.cpu("rays_o").numpy(), d.cpu("rays_d").numpy(), va.cpu("valid").numpy()


# ---- 1. ctx_texel_rays ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2, 3, 4])
@pytest.mark.parametrize("T", [32, 97])
def test_texel_rays_equals_the_rule(dev, meshes, T, s):
    c = spot_case(meshes, T)
    chart, off = c['chart'], c['off']
    mixed = np.concatenate([chart[:125], [-1, T * T], off[:3], chart[125:250], off[-2:]]).astype(np.int32)
    assert len(mixed) == 257
    lists = [("chart", chart, c['f'], c['uv']), ("mixed", mixed, c['f'], c['uv']), ("flat", chart, c['f_flat'], c['uv_flat'])]
    lists += [(f"n={n}", chart[7:7 + n], c['f'], c['uv']) for n in (1, 255, 256, 257)]
    for name, idx, faces, uv in lists:
        want = B.texel_rays_np(c['tface'], c['tbary'], uv, c['v'], faces, idx, s, SHELL)
        got = gpu_rays(dev, c, faces, uv, idx, s)
        for k, what in enumerate(("rays_o", "rays_d", "valid")):
            assert np.array_equal(got[k], want[k]), (name, what, int((got[k] != want[k]).sum()))
        if name == "flat":
            assert 0 < int((want[2] == 0).sum()) < len(want[2])
        if name == "mixed":
            assert int((want[2].reshape(-1, s * s)[:, 0] == 0).sum()) == 7


def test_texel_rays_wrapper_and_shell(dev, meshes):
    from contexture_nerf_amd import kal
    c = spot_case(meshes, 32)
    args = [_t(dev, c['tface']), _t(dev, c['tbary']), _t(dev, c['uv']), _t(dev, c['v']), _t(dev, c['f'])]
    for h in (1e-3, 0.25):
        o, d, va = kal.texel_rays(*args, _t(dev, c['chart']), 2, h)
        want = B.texel_rays_np(c['tface'], c['tbary'], c['uv'], c['v'], c['f'], c['chart'], 2, h)
        assert np.array_equal(o.cpu().numpy(), want[0]) and np.array_equal(d.cpu().numpy(), want[1]) and np.array_equal(va.cpu().numpy(), want[2])
    assert torch.equal(kal.chart_texels(args[0]).cpu(), torch.from_numpy(c['chart']))
    o, d, va = kal.texel_rays(*args, _t(dev, c['chart'][:0]), 3, 0.1)
    assert o.shape == (0, 3) and va.shape == (0,)


# ---- 2. ctx_bake_resolve -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_bake_resolve_equals_the_rule(dev, s):
    from contexture_nerf_amd import kal
    T, ss = 40, s * s
    rng = np.random.default_rng(50 + s)
    written = dropped = 0
    for n in (1, 255, 256, 257, 1500):
        idx = rng.permutation(T * T)[:n].astype(np.int32)
        rgb = rng.random((n * ss, 3)).astype(f32)
        alpha = rng.random(n * ss).astype(f32)
        valid = (rng.random(n * ss) < 0.8).astype(np.uint8)
        near = rng.random(n) < 0.3                                     # entries whose mean alpha sits at the cut, a few ulps either way
        edge = (f32(0.5) + rng.integers(-2, 3, n).astype(f32) * f32(2.0 ** -24)).astype(f32)
        alpha.reshape(n, ss)[near] = edge[near, None]
        for bad in (np.nan, np.inf, -np.inf):
            rgb.reshape(-1)[rng.integers(0, rgb.size, max(1, n // 8))] = bad
            alpha[rng.integers(0, alpha.size, max(1, n // 16))] = bad
        start = rng.integers(-2 ** 40, 2 ** 40, (4, T, T)).astype(np.int64) if n % 2 else np.zeros((4, T, T), np.int64)
        want = B.bake_resolve_np(rgb, alpha, valid, idx, s, T, 0.5, acc=start.copy())
        acc = Out(dev, (4, T, T), torch.int64)
        acc.t.copy_(_t(dev, start))
        kal.bake_resolve(_t(dev, rgb), _t(dev, alpha), _t(dev, valid), _t(dev, idx), s, acc.t, min_alpha=0.5)
        got = acc.cpu("acc").numpy()
        assert np.array_equal(got, want), (n, int((got != want).sum()))
        cut = (want[3] == start[3]).reshape(-1)[idx]
        written, dropped = written + int((~cut).sum()), dropped + int(cut.sum())
    assert written > 500 and dropped > 100                              # the case set holds both: texels written, texels cut or empty


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(dev, meshes):
    from contexture_nerf_amd import _lib as L, kal
    lib = L.load()
    c = spot_case(meshes, 32)
    T, F, V, n = 32, c['f'].shape[0], c['v'].shape[0], 10
    ten = [_t(dev, c['tface']), _t(dev, c['tbary']), _t(dev, c['uv']), _t(dev, c['v']), _t(dev, c['f']), _t(dev, c['chart'][:n])]
    o, d, va = Out(dev, (n * 16, 3), torch.float32, 0xA5), Out(dev, (n * 16, 3), torch.float32, 0xA5), Out(dev, (n * 16,), torch.uint8, 0xA5)
    good = [L.ptr(x) for x in ten] + [n, T, F, V, 2, 0.05, L.ptr(o.t), L.ptr(d.t), L.ptr(va.t), L.stream()]
    cases = [({k: None}, "null") for k in (0, 1, 2, 3, 4, 5, 12, 13, 14)]
    cases += [({10: 0}, "supersample"), ({10: 5}, "supersample"), ({11: 0.0}, "shell"), ({11: -1.0}, "shell"), ({11: float('inf')}, "shell"),
              ({11: float('nan')}, "shell"), ({6: 1 << 27, 10: 4}, "2^31"), ({6: -1}, "2^31"), ({7: 0}, "T=")]
    for change, needle in cases:
        a = list(good)
        for k, val in change.items():
            a[k] = val
        rc = lib.ctx_texel_rays(*a)
        assert rc != 0 and needle.encode() in lib.ctx_last_error(), (change, lib.ctx_last_error())
    for x in (o, d, va):
        x.untouched("texel_rays")
    acc = Out(dev, (4, T, T), torch.int64, 0xA5)
    rgb, al, vd = torch.ones(n * 16, 3, device=dev), torch.ones(n * 16, device=dev), torch.ones(n * 16, dtype=torch.uint8, device=dev)
    good = [L.ptr(rgb), L.ptr(al), L.ptr(vd), ten[5].data_ptr(), n, 2, T, 0.5, 32, L.ptr(acc.t), L.stream()]
    cases = [({k: None}, "null") for k in (0, 1, 2, 3, 9)]
    cases += [({5: 0}, "supersample"), ({5: 5}, "supersample"), ({4: 1 << 27, 5: 4}, "2^31"), ({6: 0}, "T="), ({8: 63}, "frac_bits")]
    for change, needle in cases:
        a = list(good)
        for k, val in change.items():
            a[k] = val
        rc = lib.ctx_bake_resolve(*a)
        assert rc != 0 and needle.encode() in lib.ctx_last_error(), (change, lib.ctx_last_error())
    acc.untouched("bake_resolve")
    # the wrappers refuse shapes and dtypes before any launch
    for kw, match in ((dict(idx=ten[5].long()), "dtype"), (dict(idx=ten[5].cpu()), "device tensor"), (dict(supersample=5), "supersample"),
                      (dict(shell=0.0), "shell"), (dict(texel_bary=ten[1][:, :, :2].contiguous()), "texel_bary"),
                      (dict(face_uv=ten[2][:-1].contiguous()), "face_uv")):
        base = dict(texel_face=ten[0], texel_bary=ten[1], face_uv=ten[2], vertices=ten[3], faces=ten[4], idx=ten[5], supersample=2, shell=0.05)
        with pytest.raises(L.CtxError, match=match):
            kal.texel_rays(**dict(base, **kw))
    with pytest.raises(L.CtxError, match="alpha"):
        kal.bake_resolve(rgb[:40], al[:39], vd[:40], ten[5], 2, torch.zeros(4, T, T, dtype=torch.int64, device=dev))
    with pytest.raises(L.CtxError, match="acc"):
        kal.bake_resolve(rgb[:40], al[:40], vd[:40], ten[5], 2, torch.zeros(3, T, T, dtype=torch.int64, device=dev))


# ---- 4. the chain --------------------------------------------------------------------------------------------------------------------
class LinearField:
    """raw[:3] linear in the position, the density a large constant: plain torch, in the dtype of the points."""
    A = [[1.5, -0.7, 0.3], [0.2, 1.1, -0.9], [-0.6, 0.4, 1.3]]
    b = [0.1, -0.2, 0.3]
    sigma = 1000.0

    def forward_pts(self, pts):
        A, b = torch.tensor(self.A, dtype=pts.dtype, device=pts.device), torch.tensor(self.b, dtype=pts.dtype, device=pts.device)
        return torch.cat([pts @ A.T + b, torch.full_like(pts[:, :1], self.sigma)], 1)


def test_bake_atlas_against_the_float64_chain(dev, meshes):
    from contexture_nerf_amd import volume_render as vr
    T, s, Gn = 32, 2, 16
    c = spot_case(meshes, T)
    ten = [_t(dev, c['v']), _t(dev, c['f']), _t(dev, c['uv']), _t(dev, c['tface']), _t(dev, c['tbary'])]
    grid = vr.OccupancyGrid.from_mesh(ten[0], ten[1], Gn, -1.0, 1.0, dilate=1)
    field = LinearField()
    acc = vr.bake_atlas(field, *ten, grid, supersample=s)
    # the restatement: the rule's rays, the march's rule on them, the compositing formula in float64, the rule's resolve
    shell = 1.5 * float(np.max(grid.h))
    step = shell / 8.0
    ro, rd, valid = B.texel_rays_np(c['tface'], c['tbary'], c['uv'], c['v'], c['f'], c['chart'], s, shell)
    _, ray_off, _, t, dt, pts, _ = mr.occ_march_np(ro, rd, 0.0, 2.0 * shell, grid.cells.cpu().numpy(), grid.lo, grid.hi, grid.inv, grid.h, step)
    p64 = torch.from_numpy(pts).double()
    rgb, _, alpha, _, _ = mr.restate_packed(field.forward_pts(p64), torch.from_numpy(t).double(), torch.from_numpy(dt).double(),
                                           torch.from_numpy(rd).double(), ray_off)
    alpha = alpha.numpy()
    assert (np.abs(alpha - 0.5) > 0.4).all()                               # no ray near the cut: coverage cannot hang on a rounding
    m_alpha = alpha.reshape(-1, s * s).mean(1)
    assert (np.abs(m_alpha - 0.5) > 0.1).all()
    want = B.bake_resolve_np(rgb.numpy().astype(f32), alpha.astype(f32), valid, c['chart'], s, T, 0.5)
    got = acc.cpu().numpy()
    cov = want[3] > 0
    assert np.array_equal(got[3] > 0, cov) and 0.5 * len(c['chart']) < cov.sum() <= len(c['chart'])
    col_g = got[:3, cov].astype(np.float64) / got[3, cov]
    mean64 = (rgb.numpy().reshape(-1, s * s, 3).mean(1) / m_alpha[:, None])
    col_w = np.zeros((3, T * T)); col_w[:, c['chart']] = mean64.T
    col_w = col_w.reshape(3, T, T)[:, cov]
    rel = np.abs(col_g - col_w).max() / np.abs(col_w).max()
    print(f"bake_atlas vs the float64 chain: {cov.sum()} covered of {len(c['chart'])} chart texels, colour max rel {rel:.3e}")
    assert np.allclose(col_g, col_w, rtol=2e-4, atol=2e-6)               # the compositing's forward tolerance (tests/test_march_gpu.py)
    # reproducibility: twice, on a side stream, in several chunks
    again = vr.bake_atlas(field, *ten, grid, supersample=s)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        other = vr.bake_atlas(field, *ten, grid, supersample=s)
    side.synchronize()
    chunks = vr.bake_atlas(field, *ten, grid, supersample=s, rays_per_chunk=4 * 97)
    assert torch.equal(again, acc) and torch.equal(other, acc) and torch.equal(chunks, acc)


# ---- 5. the round trip ---------------------------------------------------------------------------------------------------------------
FIT_ITERS = 300          # recorded: the loss of the fit below falls by more than 10x within these


def _spot_trainer(dev, T, G_):
    from contexture_nerf_amd import config as CFG
    from contexture_nerf_amd.trainer import ConTEXTure
    cfg = CFG.TrainConfig()
    cfg.guide.text = "a test mesh"
    cfg.guide.shape_path = "shapes/spot_triangulated.obj"
    cfg.guide.texture_resolution = T
    cfg.render.train_grid_size = G_
    return ConTEXTure(cfg, device=dev, diffusion=None)


def _procedural_atlas(tr):
    """[1,3,T,T]: the colour of a chart texel is a smooth function of its 3-D surface point (no seams), padded outward past the charts."""
    from contexture_nerf_amd import kal
    mm = tr.mesh_model
    tface, tbary = mm.texel_map()
    corners = mm.mesh.vertices[mm.mesh.faces][tface.clamp_min(0)]                         # [T,T,3,3]
    P = (tbary[..., None] * corners).sum(2)
    col = 0.5 + 0.4 * torch.stack([torch.sin(5 * P[..., 0] + 2 * P[..., 1]), torch.sin(4 * P[..., 1] - 3 * P[..., 2] + 1),
                                   torch.sin(6 * P[..., 2] + 2 * P[..., 0] + 2)], 0)
    chart = (tface >= 0)
    filled, _ = kal.atlas_fill((col * chart).contiguous(), chart.float().contiguous(), mm.chart_mask(), 4)
    return filled[None].contiguous()


def _render(tr, tex, thetas, phis, radii, G_):
    mm = tr.mesh_model
    B_ = len(thetas)
    a = lambda x: torch.tensor(x, dtype=torch.float32, device=tr.device)
    img, mask, _, _, cache = mm.renderer.render_multiple_view_texture(
        mm.mesh.vertices[None].repeat(B_, 1, 1), mm.mesh.faces, mm.face_attributes, tex.expand(B_, -1, -1, -1).contiguous(), elev=a(thetas),
        azim=a(phis), radius=a(radii), look_at_height=mm.dy, dims=(G_, G_), background_type='white')
    return img.permute(0, 2, 3, 1).contiguous(), mask[:, 0] > 0, cache['face_idx']


def test_round_trip_through_a_hash_grid_field(dev):
    from contexture_nerf_amd import volume_render as vr
    from contexture_nerf_amd.hashgrid import HashGridField
    T, G_ = 128, 128
    tr = _spot_trainer(dev, T, G_)
    mm = tr.mesh_model
    tex = _procedural_atlas(tr)
    K, c2ws = tr.train_view_cameras(G_, G_)
    thetas = [float(v['theta']) for v in tr.train_views] + [0.35, np.pi - 0.35]
    phis = [tr._offset_phi(v['phi']) for v in tr.train_views] + [0.0, 0.0]
    radii = [float(v['radius']) for v in tr.train_views] + [1.5, 1.5]
    _, extra = vr.view_cameras(thetas[-2:], phis[-2:], radii[-2:], mm.dy, G_, G_)
    c2ws = torch.cat([c2ws, extra]).to(dev)
    teacher, fg, face_idx = _render(tr, tex, thetas, phis, radii, G_)
    verts, faces = mm.mesh.vertices.contiguous(), mm.mesh.faces.contiguous()
    lo, hi = verts.min(0).values.cpu().numpy(), verts.max(0).values.cpu().numpy()
    pad = 0.1 * float((hi - lo).max())                                     # the grid bake_field makes for itself: the field is trained where it is baked
    grid = vr.OccupancyGrid.from_mesh(verts, faces, 128, lo - pad, hi + pad, dilate=1)
    h = float(np.max(grid.h))
    torch.manual_seed(11)
    field = HashGridField.from_grid(grid, n_levels=8, log2_table=14).to(dev)
    hist = vr.fit_views(field, teacher, c2ws, K, 0.5, 2.5, FIT_ITERS, rays_per_iter=4096, lr=1e-2, seed=5, white_bkgd=True, occupancy=grid,
                        occupancy_every=0, march=h)
    first, last = float(np.mean(hist[:3])), float(np.mean(hist[-10:]))
    print(f"fit: {FIT_ITERS} iterations, loss {first:.5f} -> {last:.5f} ({first / last:.1f}x)")
    assert last * 10 <= first
    atlas, cov = tr.bake_field(field, supersample=2)
    tface, _ = mm.texel_map()
    chart = tface >= 0
    seen = torch.zeros(faces.shape[0], dtype=torch.bool, device=dev)
    seen[face_idx[face_idx >= 0]] = True                                   # a face the raster shows is front-facing in that view
    share_seen = float((chart & seen[tface.clamp_min(0)]).sum()) / float(chart.sum())
    share_cov = float(((cov > 0) & chart).sum()) / float(chart.sum())
    seen_chart = chart & seen[tface.clamp_min(0)]
    print(f"of the chart texels a teacher view shows, {float(((cov > 0) & seen_chart).sum()) / float(seen_chart.sum()):.4f} are covered")
    assert not bool(((cov > 0) & ~chart).any())
    tr.complete_atlas()
    baked_tex = tr._painted_texture(torch.zeros(1, 3, T, T, device=dev))
    baked, _, _ = _render(tr, baked_tex, thetas[:7], phis[:7], radii[:7], G_)
    own = torch.stack([vr.render_image(field, G_, G_, K, c2ws[v], 0.5, 2.5, 0, white_bkgd=True, occupancy=grid, march=h)['rgb'] for v in range(7)])
    m = fg[:7]
    A = float((baked - teacher[:7]).abs()[m].mean())
    Bv = float((own - teacher[:7]).abs()[m].mean())
    print(f"round trip: A (baked mesh vs teacher) {A:.5f}, B (field's own render vs teacher) {Bv:.5f}, A/B {A / Bv:.3f}; coverage {share_cov:.4f} "
          f"of the chart, front-facing in a teacher view {share_seen:.4f}")
    assert A <= 1.5 * Bv
    assert share_cov >= share_seen


# ---- 6. the trainer end to end -------------------------------------------------------------------------------------------------------
def test_trainer_bake_complete_export_and_paint_untouched(dev):
    from PIL import Image
    from contexture_nerf_amd import config as CFG
    from contexture_nerf_amd.trainer import ConTEXTure
    from test_pipeline_gpu import _tiny_sd
    T = 128

    def make():
        cfg = CFG.TrainConfig()
        cfg.guide.text = "a test mesh"
        cfg.guide.shape_path = "shapes/spot_triangulated.obj"
        cfg.guide.texture_resolution = T
        cfg.guide.guidance_scale = 10.0
        cfg.guide.sd_image_size = 128
        cfg.guide.num_inference_steps = 2
        cfg.render.train_grid_size = 160
        return ConTEXTure(cfg, device=dev, diffusion=_tiny_sd(dev)[0])
    plain, tr = make(), make()
    p_atlas, p_cov = plain.paint()                                          # a trainer that never bakes
    atlas, cov = tr.bake_field(LinearField(), G=64)
    chart = tr.mesh_model.chart_mask() > 0
    covered = cov > 0
    assert tuple(atlas.shape) == (3, T, T) and atlas is tr.atlas and cov is tr.atlas_coverage and tr.atlas_filled is None
    assert bool(covered.any()) and not bool((covered & ~chart).any()) and bool(torch.isfinite(atlas).all())
    assert float(covered.sum()) > 0.9 * float(chart.sum())
    filled, src = tr.complete_atlas()
    assert bool((src[chart] >= 0).all())
    with tempfile.TemporaryDirectory() as td:
        png = np.asarray(Image.open(os.path.join(tr.export(os.path.join(td, 'baked')), 'albedo.png')).convert('RGB'))
    want = (atlas.permute(1, 2, 0).clamp(0, 1) * 255).to(torch.uint8).cpu().numpy()
    c = covered.cpu().numpy()
    assert png.shape == (T, T, 3) and np.array_equal(png[c], want[c])
    K, c2ws = tr.train_view_cameras()
    assert tuple(c2ws.shape) == (len(tr.train_views), 3, 4) and K[0, 2] == (160 - 1) / 2
    t_atlas, t_cov = tr.paint()                                             # painting after a bake: the bits of the trainer that never baked
    assert torch.equal(t_atlas, p_atlas) and torch.equal(t_cov, p_cov)
