"""CPU: baking the 3-D field into the UV atlas — the camera of a Renderer pose, the properties of the two rules of
tests/bake_rule.py (the definitions csrc/bake.hip is held to), and the host control flow with the kernels stubbed.

1. view_camera: rays through the raster's pixel centres, for the seven train poses and three odd ones, two image shapes; cx = W/2 fails;
2. texel_rays_np against its float64 twin on spot at T = 64, s in 1..4, within a derived bound; |d| = 1; o + h d returns to the point;
   invalid entries; a UV triangle without area;
3. the bounds see five planted mistakes;
4. bake_resolve_np: half colour, the alpha cut, what is left out of the mean, two calls add;
5. bake_atlas / bake_field with kal.texel_rays, kal.bake_resolve and rnh.render_rays_marched stubbed.

The bounds of 2 (binary32, u = 2^-24; L = |e1| + |e2| the face's world edge lengths, vmax the largest |coordinate| of its vertices):
  barycentrics  The raster solves them from UV coordinates of magnitude <= 1 in its [-1, 1] frame: every edge function carries an absolute
                error of a few u times the UV edge lengths, divided by the UV area: eps_b <= 8 u (1 + cond T / 2), where
                cond = 2 (sum |UV edge components|) / (|D| T) is texel_points_f64's bound on sum_k |d b_k / d texel|, so cond T / 2 is the
                same quotient in UV units.  The 8 counts the roundings of the raster's edge function and quotient (its own restatement
                in tests/test_uv_gather_gpu.py meets the oracle within 2^-20 on barycentrics in [0, 1]).
  s > 1         the offset adds delta . g with |delta| <= 3/8 per axis and |g| summed <= cond / 2.  D = x1 y2 - x2 y1 cancels: its relative
                error is u kappa, kappa = (|x1 y2| + |x2 y1|) / |D| >= 1, and every g inherits it (plus 2 u of its own, plus the two
                products and the sum of the offset: 3 u): the barycentrics move by at most (3/8) cond (kappa + 5) u, b0' by as much again.
  point         sum b_k v_k with sum b_k = 1 up to 3 eps: |dx| <= eps_b' L + 6 u vmax (three products, two sums, and the defect of the sum
                of the barycentrics times |v0|), eps_b' the sum of the two terms above.
  A face whose bound exceeds 1e-4 of the mesh's extent (an ill-conditioned UV triangle: a sliver in the atlas) is left out; such faces
  may hold at most 1 % of the chart texels, which is asserted."""
import numpy as np
import pytest
import torch

import bake_rule as B
import test_atlas_fill_cpu as R

f32 = np.float32
U = 2.0 ** -24
T = 64
SHELL = 0.03


# ---- 1. the camera ---------------------------------------------------------------------------------------------------------------
POSES = [(float(t), float(p), 1.5) for t, p in zip(R.SPOT_THETA, R.SPOT_PHI)] + [(0.3, 5.9, 1.1), (2.8, 0.01, 2.5), (1.57, 3.14159, 0.9)]


def _raster_xy(pts, elev, azim, radius, dy):
    """World points [n,3] -> raster x, y through the renderer's own camera: kal.generate_transformation_matrix and
    kal.generate_perspective_projection, as prepare_vertices applies them (float64 here)."""
    from contexture_nerf_amd import kal
    from contexture_nerf_amd.render import Renderer
    M = Renderer.get_camera_from_view(torch.tensor(elev), torch.tensor(azim), radius, dy)[0].double().numpy()     # [4,3]
    proj = kal.generate_perspective_projection(np.pi / 3).double().numpy().reshape(3)
    cam = np.concatenate([pts, np.ones((len(pts), 1))], 1) @ M
    return cam[:, 0] * proj[0] / (cam[:, 2] * proj[2]), cam[:, 1] * proj[1] / (cam[:, 2] * proj[2])


@pytest.mark.parametrize("H,W", [(64, 64), (48, 80)])
def test_view_camera_rays_pass_through_the_raster_pixel_centres(H, W):
    from contexture_nerf_amd import volume_render as VR
    from oracle import nerf as on
    i, j = np.meshgrid(np.arange(W), np.arange(H), indexing='xy')
    want_x, want_y = ((2 * i + 1 - W) / W).reshape(-1), ((H - 2 * j - 1) / H).reshape(-1)
    Ks, c2ws = VR.view_cameras([p[0] for p in POSES], [p[1] for p in POSES], [p[2] for p in POSES], 0.25, H, W)
    assert tuple(c2ws.shape) == (len(POSES), 3, 4) and c2ws.dtype == torch.float32
    for v, (elev, azim, radius) in enumerate(POSES):
        K, c2w = VR.view_camera(elev, azim, radius, 0.25, H, W)
        assert K.dtype == np.float32 and tuple(c2w.shape) == (3, 4) and c2w.dtype == torch.float32
        assert torch.equal(c2w, c2ws[v]) and np.array_equal(K, Ks)
        Kr, cr = B.view_camera_np(elev, azim, radius, 0.25, H, W)
        assert np.array_equal(K, Kr) and np.abs(c2w.numpy() - cr).max() <= 4 * 2.0 ** -23 * radius
        ro, rd = on.get_rays(H, W, K, c2w.numpy())
        off = on.get_rays(H, W, np.array([[K[0, 0], 0, W / 2], [0, K[1, 1], (H - 1) / 2], [0, 0, 1]], f32), c2w.numpy())
        for t in (0.5, 2.0):
            x, y = _raster_xy((ro.astype(np.float64) + t * rd.astype(np.float64)).reshape(-1, 3), elev, azim, radius, 0.25)
            err = max(np.abs(x - want_x).max(), np.abs(y - want_y).max())
            assert err <= 1e-5, (v, t, err)
            xo, _ = _raster_xy((off[0].astype(np.float64) + t * off[1].astype(np.float64)).reshape(-1, 3), elev, azim, radius, 0.25)
            assert np.abs(xo - want_x).min() > 0.9 / W              # cx = W/2: every ray is half a pixel (1/W) off


# ---- 2. the rule on spot ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spot(meshes):
    import test_uv_gather_cpu as G
    v, f, vt, ft, _, _ = R.spot_arrays(meshes)
    tface, tbary = G.texel_map(vt, ft, T)
    idx = np.nonzero(tface.reshape(-1) >= 0)[0].astype(np.int32)
    return dict(v=v.astype(f32), f=f, face_uv=vt[ft].astype(f32), tface=tface, tbary=tbary, idx=idx)


def _bounds(sp, s):
    """Per row of the chart list: (point bound, normal bound, kept bool) as the module docstring derives them."""
    f = sp['tface'].reshape(-1)[sp['idx']]
    V = sp['v'].astype(np.float64)[sp['f'][f]]
    e1, e2 = V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]
    Lw = np.linalg.norm(e1, axis=1) + np.linalg.norm(e2, axis=1)
    vmax = np.abs(V).max((1, 2))
    uv = sp['face_uv'].astype(np.float64)[f]
    a, b = uv[:, 1] - uv[:, 0], uv[:, 2] - uv[:, 0]
    D = a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]
    with np.errstate(all='ignore'):
        cond = 2 * (np.abs(a).sum(1) + np.abs(b).sum(1)) / (np.abs(D) * T)
        kappa = (np.abs(a[:, 0] * b[:, 1]) + np.abs(b[:, 0] * a[:, 1])) / np.abs(D)
        eps = 8 * U * (1 + cond * T / 2)
        if s > 1:
            eps = eps + 2 * (3 / 8) * cond * (kappa + 5) * U
        point = eps * Lw + 6 * U * vmax
        c = np.cross(e1, e2)
        k3 = np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1) / np.linalg.norm(c, axis=1)
        normal = (8 * k3 + 4) * U                                 # six products and three differences cancel by k3; norm, sqrt, quotient
    extent = float(np.ptp(sp['v'], axis=0).max())
    kept = np.isfinite(point) & (point <= 1e-4 * extent)
    rep = lambda x: np.repeat(x, s * s)
    return rep(point), rep(normal), rep(kept), np.repeat(c / np.linalg.norm(c, axis=1, keepdims=True), s * s, 0)


def _errors(sp, s, **mistake):
    o, d, valid = B.texel_rays_np(sp['tface'], sp['tbary'], sp['face_uv'], sp['v'], sp['f'], sp['idx'], s, SHELL, **mistake)
    pts, _, ok = B.texel_points_f64(sp['tface'], sp['face_uv'], sp['v'], sp['f'], sp['idx'], s)
    back = o.astype(np.float64) + float(f32(SHELL)) * d.astype(np.float64)
    return o, d, valid, np.abs(back - pts).max(1), ok


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_rule_meets_its_float64_twin_on_spot(spot, s):
    o, d, valid, err, ok = _errors(spot, s)
    point, normal, kept, n64 = _bounds(spot, s)
    assert valid.all() and ok.all()
    left_out = 1.0 - kept.mean()
    assert left_out <= 0.01, f"{left_out:.4f} of the chart texels lie on faces the bound leaves out"
    # o + h d returns to the point: the point's bound plus the roundings of h*n, x + h*n and of this very sum in float64 of float32 terms
    ret = point + 4 * U * (np.abs(o).max(1) + SHELL)
    worst = (err[kept] / ret[kept]).max()
    print(f"s={s}: {kept.sum()} rows, max |o + h d - twin| = {err[kept].max():.3e}, worst ratio to its bound {worst:.3f}, left out {left_out:.4%}")
    assert worst <= 1.0
    ln = np.linalg.norm(d.astype(np.float64), axis=1)
    assert np.abs(ln - 1).max() <= 2 * 2.0 ** -23                   # |d| = 1 to 2 ulp
    dn = np.abs(d.astype(np.float64) + n64).max(1)                   # d = -(the face normal of prepare_vertices' orientation)
    assert (dn / normal).max() <= 1.0, (dn / normal).max()


def test_rule_orientation_is_kaolins_face_normal(spot, meshes):
    from oracle import geometry as og
    _, d, _ = B.texel_rays_np(spot['tface'], spot['tbary'], spot['face_uv'], spot['v'], spot['f'], spot['idx'], 1, SHELL)
    v, f, _, _, cam, proj = R.spot_arrays(meshes)
    _, _, fn = og.prepare_vertices(v[None], f, proj, cam[:1])          # face normals in the camera frame of the first pose
    face = spot['tface'].reshape(-1)[spot['idx']]
    d_cam = d.astype(np.float64) @ cam[0, :3].astype(np.float64)     # world -> camera, row vectors
    assert ((d_cam * fn[0][face]).sum(1) < -0.999).all()              # a question of sign: the other orientation gives +1


def test_invalid_entries_and_flat_triangles(spot):
    sp = spot
    F, V = sp['f'].shape[0], sp['v'].shape[0]
    off = np.nonzero(sp['tface'].reshape(-1) < 0)[0][:3].astype(np.int32)
    idx = np.concatenate([[-1, T * T, 2 ** 31 - 1], off, sp['idx'][:5]]).astype(np.int32)
    faces, vertices, face_uv = sp['f'].copy(), sp['v'].copy(), sp['face_uv'].copy()
    f3, f4 = (int(sp['tface'].reshape(-1)[sp['idx'][k]]) for k in (3, 4))
    faces[f3, 2] = faces[f3, 1]                                     # a face without area
    for s in (1, 3):
        o, d, valid = B.texel_rays_np(sp['tface'], sp['tbary'], face_uv, vertices, faces, idx, s, SHELL)
        valid = valid.reshape(len(idx), s * s)
        f_of = sp['tface'].reshape(-1)[sp['idx'][:5]]
        want = np.concatenate([np.zeros(6, bool), f_of != f3])
        assert np.array_equal(valid.all(1), want) and np.array_equal(valid.any(1), want)
        assert not o.reshape(len(idx), -1)[~want].any() and not d.reshape(len(idx), -1)[~want].any()
    bad = faces.copy(); bad[f4, 0] = V                              # a vertex id outside the mesh
    _, _, valid = B.texel_rays_np(sp['tface'], sp['tbary'], face_uv, vertices, bad, sp['idx'][:5], 2, SHELL)
    assert np.array_equal(valid.reshape(5, 4).all(1), ~np.isin(sp['tface'].reshape(-1)[sp['idx'][:5]], [f3, f4]))
    tf = sp['tface'].copy(); tf.reshape(-1)[sp['idx'][0]] = F       # a face id outside the mesh
    _, _, valid = B.texel_rays_np(tf, sp['tbary'], face_uv, vertices, sp['f'], sp['idx'][:2], 1, SHELL)
    assert valid.tolist() == [0, 1]
    # a UV triangle without area: the sub-samples collapse onto the centre, which is the s = 1 row
    f0 = int(sp['tface'].reshape(-1)[sp['idx'][0]])
    face_uv[f0, 2] = face_uv[f0, 1]
    o1, d1, _ = B.texel_rays_np(sp['tface'], sp['tbary'], face_uv, sp['v'], sp['f'], sp['idx'][:1], 1, SHELL)
    o3, d3, v3 = B.texel_rays_np(sp['tface'], sp['tbary'], face_uv, sp['v'], sp['f'], sp['idx'][:1], 3, SHELL)
    assert v3.all() and np.array_equal(o3, np.repeat(o1, 9, 0)) and np.array_equal(d3, np.repeat(d1, 9, 0))


# ---- 3. the bounds see mistakes --------------------------------------------------------------------------------------------------
def _sub(s):
    k = np.arange(s * s)
    return (k % s + 0.5) / s - 0.5, (k // s + 0.5) / s - 0.5


@pytest.mark.parametrize("name,mistake,affects", [
    ("v not flipped", dict(flip_v=False), lambda dx, dy: dy != 0),
    ("dy with the wrong sign", dict(dy_sign=-1.0), lambda dx, dy: dy != 0),
    ("barycentrics rotated by one", dict(rotate=1), lambda dx, dy: np.ones_like(dx, bool)),
    ("T - 1 in place of T", dict(T_edge=T - 1), lambda dx, dy: (dx != 0) | (dy != 0)),
])
def test_point_bound_rejects(spot, name, mistake, affects):
    for s in (2, 3):
        _, _, _, err, _ = _errors(spot, s, **mistake)
        point, _, kept, _ = _bounds(spot, s)
        o = B.texel_rays_np(spot['tface'], spot['tbary'], spot['face_uv'], spot['v'], spot['f'], spot['idx'], s, SHELL)[0]
        ret = point + 4 * U * (np.abs(o).max(1) + SHELL)
        can = np.tile(affects(*_sub(s)), len(spot['idx'])) & kept
        share = (err[can] > ret[can]).mean()
        print(f"{name}, s={s}: {share:.3f} of the {can.sum()} rows it can affect leave the bound")
        assert share > 0.5, (name, s, share)


def test_normal_bound_rejects_e2_cross_e1(spot):
    _, d, _, _, _ = _errors(spot, 1, swap_cross=True)
    _, normal, _, n64 = _bounds(spot, 1)
    assert (np.abs(d.astype(np.float64) + n64).max(1) > normal).mean() > 0.5


# ---- 4. the resolve --------------------------------------------------------------------------------------------------------------
def test_resolve_rule():
    Tt, s = 4, 2
    idx = np.array([5, 9, -1, 16, 2, 7], np.int32)
    n = len(idx)
    rgb = np.full((n, 4, 3), 0.5, f32); alpha = np.ones((n, 4), f32); valid = np.ones((n, 4), np.uint8)
    alpha[1] = [0.5, 0.5, 0.49, 0.5]                                # mean just under the cut
    valid[4, 1:] = 0; rgb[4, 1:] = 100.0                            # one sub-sample counts: m = 1
    alpha[5, 0] = np.nan; rgb[5, 1, 2] = np.inf; rgb[5, 2, 0] = -np.inf; valid[5, 3] = 0      # nothing counts: m = 0
    acc = B.bake_resolve_np(rgb.reshape(-1, 3), alpha.reshape(-1), valid.reshape(-1), idx, s, Tt, 0.5)
    flat = acc.reshape(4, -1)
    assert flat[3, 5] == 2 ** 32 and (flat[:3, 5] == flat[3, 5] // 2).all()
    assert flat[3, 2] == 2 ** 32 and (flat[:3, 2] == 2 ** 31).all()
    touched = np.zeros(16, bool); touched[[5, 2]] = True
    assert not flat[:, ~touched].any()
    alpha[1, 2] = 0.5                                               # now exactly at the cut: Ma >= min_alpha holds
    again = B.bake_resolve_np(rgb.reshape(-1, 3), alpha.reshape(-1), valid.reshape(-1), idx, s, Tt, 0.5, acc=acc.copy())
    assert again.reshape(4, -1)[3, 9] == 2 ** 31 and again.reshape(4, -1)[0, 9] == 2 ** 31
    assert (again.reshape(4, -1)[:, 5] == 2 * flat[:, 5]).all()      # two calls add
    # the mean is taken over what counts, left to right
    rgb2 = np.zeros((1, 4, 3), f32); rgb2[0, :, 0] = [0.1, 0.2, np.nan, 0.4]
    a2 = np.ones((1, 4), f32)
    got = B.bake_resolve_np(rgb2.reshape(-1, 3), a2.reshape(-1), np.ones(4, np.uint8), np.array([0], np.int32), 2, 1, 0.5)
    want = (f32(0.1) + f32(0.2) + f32(0.4)) / f32(3)
    assert got[0, 0, 0] == int(np.rint(np.float64(want) * 2.0 ** 32)) and got[3, 0, 0] == 2 ** 32


# ---- 5. host control flow --------------------------------------------------------------------------------------------------------
class _Grid:
    h = np.array([0.02, 0.04, 0.03], f32)


def _stub(monkeypatch, calls):
    from contexture_nerf_amd import _lib as L, kal, run_nerf_helpers as rnh
    monkeypatch.setattr(L, 'ptr', lambda t, dtype=None, name="tensor": t)

    def texel_rays(texel_face, texel_bary, face_uv, vertices, faces, idx, supersample, shell):
        R_ = idx.numel() * supersample ** 2
        calls.append(('rays', idx.clone(), supersample, shell))
        return torch.zeros(R_, 3), torch.zeros(R_, 3), torch.ones(R_, dtype=torch.uint8)

    def marched(field, ro, rd, near, far, occupancy, step, **kw):
        assert not kw and not torch.is_grad_enabled()
        calls.append(('march', ro.shape[0], near, far, step))
        R_ = ro.shape[0]
        return torch.full((R_, 3), 0.25), None, torch.ones(R_), None, None

    def resolve(rgb, alpha, valid, idx, supersample, acc, min_alpha=0.5, frac_bits=32):
        calls.append(('resolve', idx.clone(), supersample, min_alpha))
        flat = acc.view(4, -1)
        flat[:3, idx.long()] += 2 ** 30
        flat[3, idx.long()] += 2 ** 32
        return acc
    monkeypatch.setattr(kal, 'texel_rays', texel_rays)
    monkeypatch.setattr(kal, 'bake_resolve', resolve)
    monkeypatch.setattr(kal, 'chart_texels', lambda tf: torch.nonzero(tf.reshape(-1) >= 0).reshape(-1).to(torch.int32))
    monkeypatch.setattr(rnh, 'render_rays_marched', marched)


def test_bake_atlas_chunks_whole_texels_and_defaults(monkeypatch):
    from contexture_nerf_amd import _lib as L, volume_render as VR
    calls = []
    _stub(monkeypatch, calls)
    Tt = 6
    tface = torch.full((Tt, Tt), -1, dtype=torch.int64); tface[1:5, 1:4] = 2            # 12 chart texels
    args = (None, torch.zeros(3, 3), torch.zeros(4, 3, dtype=torch.int64), torch.zeros(4, 3, 2), tface, torch.zeros(Tt, Tt, 3))
    acc = VR.bake_atlas(*args, _Grid(), supersample=2, rays_per_chunk=22)              # 22 // 4 = 5 texels per chunk: 5 + 5 + 2
    rays = [c for c in calls if c[0] == 'rays']
    assert [c[1].numel() for c in rays] == [5, 5, 2]
    assert torch.equal(torch.cat([c[1] for c in rays]), torch.nonzero(tface.reshape(-1) >= 0).reshape(-1).to(torch.int32))
    shell = 1.5 * float(f32(0.04))
    assert all(c[3] == shell and c[2] == 2 for c in rays)
    assert [c[1:] for c in calls if c[0] == 'march'] == [(20, 0., 2.0 * shell, shell / 8.0), (20, 0., 2.0 * shell, shell / 8.0),
                                                          (8, 0., 2.0 * shell, shell / 8.0)]
    assert [c[0] for c in calls] == ['rays', 'march', 'resolve'] * 3
    assert acc.dtype == torch.int64 and tuple(acc.shape) == (4, Tt, Tt) and torch.equal(acc[3] > 0, tface >= 0)
    calls.clear()
    mine = torch.tensor([7, 8, 20], dtype=torch.int32)
    out = VR.bake_atlas(*args, _Grid(), step=0.01, shell=0.05, texels=mine, acc=acc, rays_per_chunk=1)       # never less than one texel
    assert out is acc and [c[1].tolist() for c in calls if c[0] == 'rays'] == [[7], [8], [20]]
    assert [c[1:] for c in calls if c[0] == 'march'] == [(1, 0., 0.1, 0.01)] * 3
    assert int(acc[3, 1, 1]) == 2 * 2 ** 32 and int(acc[3, 3, 2]) == 2 * 2 ** 32 and int(acc[3, 1, 3]) == 2 ** 32
    for bad, match in ((torch.tensor([7, 7], dtype=torch.int32), "twice"), (torch.tensor([36], dtype=torch.int32), "outside"),
                       (torch.tensor([-1], dtype=torch.int32), "outside"), (torch.zeros(2, 2, dtype=torch.int32), "1-D")):
        with pytest.raises(L.CtxError, match=match):
            VR.bake_atlas(*args, _Grid(), texels=bad)
    with pytest.raises(L.CtxError, match="occupancy"):
        VR.bake_atlas(*args, None)
    for kw, match in ((dict(supersample=5), "supersample"), (dict(supersample=0), "supersample"), (dict(shell=0.0), "shell"),
                      (dict(shell=float('inf')), "shell")):
        with pytest.raises(L.CtxError, match=match):
            VR.bake_atlas(*args, _Grid(), **kw)


def test_bake_field_sets_the_atlas_and_resets_the_fill(monkeypatch):
    import types
    import test_dist_product_cpu as P
    calls = []
    _stub(monkeypatch, calls)
    tr = P.make_trainer(0, 1, 3)
    tface = torch.full((P.T, P.T), -1, dtype=torch.int64); tface[1:7, 1:6] = 3
    tr.mesh_model.texel_map = lambda: (tface, torch.full((P.T, P.T, 3), 1 / 3))
    tr.mesh_model.face_attributes = torch.zeros(1, P.F, 3, 2)
    tr.mesh_model.renderer = types.SimpleNamespace(fovyangle=np.pi / 3)
    tr.atlas_filled, tr.atlas_fill_src = torch.ones(3, P.T, P.T), torch.zeros(P.T, P.T, dtype=torch.int32)
    atlas, cov = tr.bake_field(None, occupancy=_Grid())
    assert atlas is tr.atlas and cov is tr.atlas_coverage and tr.atlas_filled is None and tr.atlas_fill_src is None
    assert [c[2] for c in calls if c[0] == 'rays'] == [2]                                 # supersample defaults to 2
    assert torch.equal(cov > 0, tface >= 0) and torch.equal(atlas[:, tface >= 0], torch.full((3, 30), 0.25))
    assert tr.atlas_acc.dtype == torch.int64 and torch.equal(tr.atlas_acc[3] > 0, tface >= 0)
    filled = []
    tr.complete_atlas = lambda: filled.append(1)
    tr.cfg.guide.atlas_fill = 'nearest'
    tr.bake_field(None, occupancy=_Grid(), supersample=1)
    assert filled == [1]
    K, c2ws = tr.train_view_cameras(32, 48)
    assert tuple(c2ws.shape) == (3, 3, 4) and K[0, 2] == 23.5 and K[1, 2] == 15.5
    from contexture_nerf_amd import volume_render as VR
    want = VR.view_camera(1.0, tr._offset_phi(0.02), 1.5, tr.mesh_model.dy, 32, 48)[1]
    assert torch.equal(c2ws[2], want)
