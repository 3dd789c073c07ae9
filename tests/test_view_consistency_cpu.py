"""CPU: multi-view consistency (src/training/trainer.py:429-531) — its definition, the fixtures recorded from the reference, config
surface and the host's refusal of host tensors.

The numpy restatement below IS the definition the HIP kernels (csrc/viewconsist.hip) are held to; tests/test_view_consistency_gpu.py
imports it from here.  f32 per pair in the stated order, int64 sums, so the GPU comparison is array_equal.

  view_consistency(views [V,C,h,w] f32, faces [F,3], face_idx [V,h,w], fvi [V,F,3,2] f32, rows) ->
      dict(mean f32, pair_sum [V,V] i64 (units of 2^-32, [source, target]), pair_count [V,V] i64, n_outside, N, sign_count [V,C,h,w] i64)

Fixtures: tests/golden/view_consistency.npz, written by tests/golden/make_view_consistency_golden.py from the reference function
itself (spot, poses 1..6 of the seven Zero123PlusDataset poses, 160 squared).  Figures recorded there (and in DESIGN.md):
  case A (random colours)    N = 40559, mean 0.6662003, |mean_ref - mean_f64| = 2.27e-08; gradient: counts up to 71,
                             max |grad_ref / u - rint| = 2.20e-05, max |f32(count) * u - grad_ref| = 2.13e-05 u
  case B (position colours)  mean 0.7574 with the reference's rows, 0.9501 with the raster's rows (errors 2.68e-08 / 2.84e-08)

1. restatement vs the golden means (both cases, both row conventions), sum(pair_count) == N;
2. case A gradient: counts array_equal, values within twice the generator's own deviation;
3. case B: mean('image') > mean('reference');
4. synthetic inputs (coordinates x 1.5, colours x 3, one view all background, V = 1);
5. config; 6. kal.view_consistency on host tensors raises."""
import os
import zlib
import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "view_consistency.npz")
F32 = np.float32


# ---- the numpy restatement ------------------------------------------------------------------------------------------------
def seen_map(faces, face_idx, n_vertices):
    """[V, n_vertices] bool: vertex k is a corner of a face that owns at least one pixel of face_idx[j]."""
    V = face_idx.shape[0]
    seen = np.zeros((V, n_vertices), bool)
    for j in range(V):
        fs = np.unique(face_idx[j][face_idx[j] >= 0])
        seen[j, faces[fs].reshape(-1)] = True
    return seen


def source_pixel(coord, n, mirrored=False):
    """f32, in the stated order: trunc((((1 - Y) | (X + 1)) / 2) * n); inside exactly when -1 < a < n."""
    c = (F32(1) - coord) if mirrored else (coord + F32(1))
    a = (c / F32(2)) * F32(n)
    assert a.dtype == np.float32
    inside = (a > F32(-1)) & (a < F32(n))
    return np.where(inside, a, 0).astype(np.int64), inside


def view_consistency(views, faces, face_idx, fvi, rows='image', n_vertices=None, grad=True):
    views = np.ascontiguousarray(views, F32); fvi = np.asarray(fvi, F32)
    faces = np.asarray(faces, np.int64); face_idx = np.asarray(face_idx, np.int64)
    V, C, h, w = views.shape
    n_vertices = int(faces.max()) + 1 if n_vertices is None else n_vertices
    seen = seen_map(faces, face_idx, n_vertices)
    pair_sum = np.zeros((V, V), np.int64); pair_count = np.zeros((V, V), np.int64); n_outside = 0
    sign_count = np.zeros((V, C, h * w), np.int64)
    for i in range(V):
        ys, xs = np.nonzero(face_idx[i] >= 0)
        if ys.size == 0:
            continue
        f = face_idx[i, ys, xs]
        corners = faces[f]                                                   # [n, 3]
        t_all = views[i][:, ys, xs]                                          # [C, n]
        for j in range(V):
            if j == i:
                continue
            st = seen[j][corners]
            has = st.any(1)
            c = st.argmax(1)                                                 # first seen corner
            XY = fvi[j, f[has], c[has]]
            sx, inx = source_pixel(XY[:, 0], w)
            sy, iny = source_pixel(XY[:, 1], h, mirrored=(rows == 'image'))
            inside = inx & iny
            n_outside += int((~inside).sum())
            tp = (ys[has] * w + xs[has])[inside]
            sp = (sy * w + sx)[inside]
            t = t_all[:, has][:, inside]
            s = views[j].reshape(C, -1)[:, sp]
            a = np.abs(t[0] - s[0])
            for k in range(1, C):
                a = a + np.abs(t[k] - s[k])
            d = F32(1) - a / F32(C)
            assert d.dtype == np.float32
            ok = d >= 0
            pair_sum[j, i] = int(np.floor(d[ok].astype(np.float64) * 4294967296.0).astype(np.int64).sum())
            pair_count[j, i] = int(ok.sum())
            if grad:
                sg = np.sign(t[:, ok] - s[:, ok]).astype(np.int64)           # sign(0) = 0
                sign_count[i][:, tp[ok]] -= sg                               # target pixels are distinct within one (i, j)
                for k in range(C):
                    sign_count[j, k] += np.bincount(sp[ok], weights=sg[k], minlength=h * w).astype(np.int64)
    N = int(pair_count.sum()); S = int(pair_sum.sum())
    mean = F32(np.float64(S) / 4294967296.0 / np.float64(N)) if N > 0 else F32(0)
    return dict(mean=mean, pair_sum=pair_sum, pair_count=pair_count, n_outside=n_outside, N=N, sign_count=sign_count.reshape(V, C, h, w), seen=seen)


def grad_unit(N, C):
    """u = fl(fl(1 / N) / C): what one counted pair adds to an element of the gradient of the mean."""
    return (F32(1) / F32(N)) / F32(C) if N > 0 else F32(0)


def grad_from_counts(sign_count, N, C, g=1.0):
    return sign_count.astype(F32) * (grad_unit(N, C) * F32(g))


# ---- the spot cases of the fixtures, from the oracle --------------------------------------------------------------------------
def spot_case(meshes, H=160):
    """-> faces [F,3] i64, face_idx [6,H,H] i64, fvi [6,F,3,2] f32, position-coloured views [6,3,H,H] f32 (case B): poses 1..6 of
    test_atlas_fill_cpu.spot_arrays, rastered by oracle.geometry."""
    from oracle import geometry as og
    from test_atlas_fill_cpu import spot_arrays
    v, f, _, _, cam, proj = spot_arrays(meshes)
    cam = cam[1:7]
    o_cam, o_img, _ = og.prepare_vertices(np.repeat(v[None], 6, 0), f, proj, cam)
    lo, hi = v.min(0), v.max(0)
    col = ((v - lo) / (hi - lo)).astype(F32)[f]                              # [F,3,3] vertex position in [0, 1] per axis
    feat, idx = og.rasterize(H, H, o_cam[..., 2], o_img, np.repeat(col[None], 6, 0))
    views = np.where((idx >= 0)[..., None], feat, F32(0.5)).astype(F32).transpose(0, 3, 1, 2)
    return f, idx.astype(np.int64), o_img.astype(F32), np.ascontiguousarray(views)


def random_views(seed, V, C, h, w):
    return torch.rand(V, C, h, w, generator=torch.Generator().manual_seed(int(seed))).numpy()


@pytest.fixture(scope="module")
def gold():
    return load_golden()


def load_golden():
    """The fixture with fvi rebuilt from its per-vertex coordinates and case A's gradient unpacked."""
    z = np.load(GOLDEN)
    g = {k: z[k] for k in z.files}
    g['faces'] = g['faces'].astype(np.int64)
    g['face_idx'] = g['face_idx'].astype(np.int64)
    g['fvi'] = g['vertex_image'][:, g['faces']]                              # [V,F,3,2]
    V, h, w = g['face_idx'].shape
    grad = np.zeros(V * 3 * h * w, F32)
    grad[g['A_grad_index']] = g['A_grad_values']
    g['A_grad'] = grad.reshape(V, 3, h, w)
    g['A_views'] = random_views(g['A_seed'], V, 3, h, w)
    return g


def case_b_views(meshes, g):
    f, idx, fvi, views = spot_case(meshes, g['face_idx'].shape[1])
    assert np.array_equal(f, g['faces']) and np.array_equal(idx, g['face_idx']) and np.array_equal(fvi, g['fvi'])
    assert zlib.crc32(views.tobytes()) == int(g['B_views_crc32']), "case B's views are not the ones the fixture was recorded with"
    return views


# ---- 1. the restatement against the reference's recorded means ---------------------------------------------------------------
def _check_mean(tag, r, g, key):
    ref, err, N = F32(g[key + '_mean']), float(g[key + '_mean_err']), int(g[key + '_N'])
    allow = 2 * err + 2.0 ** -32
    print(f"{tag}: restatement {r['mean']:.9f}, reference {ref:.9f}, N {r['N']} / {N}, reference's own summation error {err:.3e}, allowed {allow:.3e}, "
          f"n_outside {r['n_outside']}")
    assert err <= 1e-6, "a stored summation error above 1e-6 is a different set of pairs, not rounding"
    assert r['N'] == N and r['n_outside'] == 0
    assert abs(float(r['mean']) - float(ref)) <= allow


def test_restatement_vs_reference_means(gold, meshes):
    g = gold
    rA = view_consistency(g['A_views'], g['faces'], g['face_idx'], g['fvi'], rows='reference', grad=False)
    _check_mean("case A, rows='reference'", rA, g, 'A_reference')
    vb = case_b_views(meshes, g)
    for rows in ('reference', 'image'):
        rB = view_consistency(vb, g['faces'], g['face_idx'], g['fvi'], rows=rows, grad=False)
        _check_mean(f"case B, rows={rows!r}", rB, g, 'B_' + rows)
    assert rA['pair_count'].trace() == 0 and rA['pair_sum'].trace() == 0                # the diagonal is empty


# ---- 2. case A gradient ---------------------------------------------------------------------------------------------------
def check_grad_against_reference(sign_count, grad, g):
    """The rule of the issue's test 2 for a (sign_count, grad = f32(sign_count) * u) pair against the reference's autograd gradient."""
    N = int(g['A_reference_N'])
    u = grad_unit(N, 3)
    ref = g['A_grad']
    ratio = ref.astype(np.float64) / np.float64(u)
    frac, dev = float(g['A_grad_frac_max']), float(g['A_grad_dev_max_u'])
    assert frac <= 0.01, "the fixture's integers are not unambiguous"
    assert np.array_equal(np.rint(ratio).astype(np.int64), np.asarray(sign_count, np.int64))
    got = np.abs(np.asarray(grad, np.float64) - ref.astype(np.float64)).max() / float(u)
    print(f"case A gradient: |count| max {np.abs(sign_count).max()}, max |f32(count) * u - grad_ref| = {got:.3e} u, generator's own {dev:.3e} u, allowed {2 * dev:.3e} u")
    assert got <= 2 * dev


def test_case_a_gradient_counts_and_values(gold):
    g = gold
    r = view_consistency(g['A_views'], g['faces'], g['face_idx'], g['fvi'], rows='reference')
    assert r['N'] == int(g['A_reference_N'])
    check_grad_against_reference(r['sign_count'], grad_from_counts(r['sign_count'], r['N'], 3), g)
    assert int(r['sign_count'].sum()) == 0                                              # every pair adds +s and -s


# ---- 3. the row-convention finding -------------------------------------------------------------------------------------------
def test_case_b_raster_rows_agree_better_than_reference_rows(gold, meshes):
    g = gold
    vb = case_b_views(meshes, g)
    m_ref = view_consistency(vb, g['faces'], g['face_idx'], g['fvi'], rows='reference', grad=False)['mean']
    m_img = view_consistency(vb, g['faces'], g['face_idx'], g['fvi'], rows='image', grad=False)['mean']
    print(f"case B (colour = surface position): mean with the raster's rows {m_img:.4f}, with the reference's rows {m_ref:.4f}; "
          f"recorded from the reference {float(g['B_image_mean']):.4f} / {float(g['B_reference_mean']):.4f}")
    assert m_img > m_ref
    assert float(g['B_image_mean']) > float(g['B_reference_mean'])


# ---- 4. synthetic inputs ---------------------------------------------------------------------------------------------------
def synthetic_cases(g):
    """name -> (views, faces, face_idx, fvi): the inputs of the issue's test 4, shared with the GPU test."""
    views, faces, idx, fvi = g['A_views'], g['faces'], g['face_idx'], g['fvi']
    blank = idx.copy(); blank[2] = -1
    return {
        'coords_x1.5': (views, faces, idx, (fvi * F32(1.5)).astype(F32)),
        'colours_x3': ((views * F32(3)).astype(F32), faces, idx, fvi),
        'one_view_background': (views, faces, blank, fvi),
        'single_view': (views[:1], faces, idx[:1], fvi[:1]),
    }


def test_synthetic_inputs(gold):
    g = gold
    base = view_consistency(g['A_views'], g['faces'], g['face_idx'], g['fvi'], rows='image', grad=False)
    cases = synthetic_cases(g)
    r = view_consistency(*cases['coords_x1.5'], rows='image')
    assert r['n_outside'] > 0 and 0 < r['N'] < base['N'] and int(r['sign_count'].sum()) == 0
    r3 = view_consistency(*cases['colours_x3'], rows='image', grad=False)
    assert 0 < r3['N'] < base['N'] and r3['n_outside'] == 0                            # pairs with d < 0 are dropped
    assert 0 <= r3['mean'] <= 1
    rb = view_consistency(*cases['one_view_background'], rows='image', n_vertices=int(g['faces'].max()) + 1)
    assert rb['pair_count'][2].sum() == 0 and rb['pair_count'][:, 2].sum() == 0 and 0 < rb['N'] < base['N']
    assert not rb['seen'][2].any() and not rb['sign_count'][2].any()
    r1 = view_consistency(*cases['single_view'], rows='image', n_vertices=int(g['faces'].max()) + 1)
    assert r1['mean'] == 0 and r1['N'] == 0 and not r1['pair_count'].any() and not r1['sign_count'].any() and r1['mean'].dtype == np.float32


def test_constant_images_agree_perfectly(gold):
    g = gold
    r = view_consistency(np.full_like(g['A_views'], 0.25), g['faces'], g['face_idx'], g['fvi'], rows='image')
    assert r['mean'] == 1 and r['N'] > 0 and not r['sign_count'].any()


# ---- 5. config ------------------------------------------------------------------------------------------------------------
def test_config_fields_defaults_cli_and_validation(tmp_path):
    from contexture_nerf_amd import config as CFG
    cfg = CFG.TrainConfig()
    assert cfg.optim.consistency_weight == 0.0 and isinstance(cfg.optim.consistency_weight, float)
    assert cfg.log.eval_consistency is False
    cfg = CFG.parse(argv=['--optim.consistency_weight=500', '--log.eval_consistency=true'])
    assert cfg.optim.consistency_weight == 500.0 and isinstance(cfg.optim.consistency_weight, float) and cfg.log.eval_consistency is True
    with pytest.raises(ValueError, match="consistency_weight"):
        CFG.parse(argv=['--optim.consistency_weight=-1'])
    y = tmp_path / "c.yaml"
    y.write_text("optim:\n  consistency_weight: -0.5\n")
    with pytest.raises(ValueError, match="consistency_weight"):
        CFG.parse(argv=[f'--config_path={y}'])
    y.write_text("optim:\n  consistency_weight: 2.5\nlog:\n  eval_consistency: true\n")
    cfg = CFG.parse(argv=[f'--config_path={y}'])
    assert cfg.optim.consistency_weight == 2.5 and cfg.log.eval_consistency is True
    CFG.dump(cfg, tmp_path / "d.yaml")
    assert CFG.parse(argv=[f'--config_path={tmp_path / "d.yaml"}']).optim.consistency_weight == 2.5


# ---- 6. no CPU fallback -----------------------------------------------------------------------------------------------------
def test_view_consistency_refuses_host_tensors():
    from contexture_nerf_amd import _lib as L, kal
    with pytest.raises(L.CtxError, match="device tensor"):
        kal.view_consistency(torch.zeros(2, 3, 8, 8), torch.zeros(1, 3, dtype=torch.int64), torch.zeros(2, 8, 8, dtype=torch.int64),
                             torch.zeros(2, 1, 3, 2))
    with pytest.raises(L.CtxError, match="rows"):
        kal.view_consistency(torch.zeros(2, 3, 8, 8), torch.zeros(1, 3, dtype=torch.int64), torch.zeros(2, 8, 8, dtype=torch.int64),
                             torch.zeros(2, 1, 3, 2), rows='flipped')
