"""GPU: the multi-view consistency kernels (csrc/viewconsist.hip) through the C-ABI against the numpy restatement of
tests/test_view_consistency_cpu.py — integer sums, so every comparison is array_equal / bit-equal — and the feature's host side:
ConTEXTure.view_consistency, optim.consistency_weight in the SDS loop, log.eval_consistency in full_eval."""
import json
import os
import numpy as np
import pytest
import torch

import test_view_consistency_cpu as VC

pytestmark = pytest.mark.gpu


def _dev(dev, views, faces, idx, fvi):
    return (torch.from_numpy(np.ascontiguousarray(views, np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(faces, np.int64)).to(dev),
            torch.from_numpy(np.ascontiguousarray(idx, np.int64)).to(dev), torch.from_numpy(np.ascontiguousarray(fvi, np.float32)).to(dev))


def _run(dev, args, rows, n_vertices, **kw):
    from contexture_nerf_amd import kal
    mean, st = kal.view_consistency(*_dev(dev, *args), rows=rows, stats=True, n_vertices=n_vertices, **kw)
    return mean, st


def _assert_forward(dev, tag, args, rows, n_vertices, want=None):
    want = VC.view_consistency(*args, rows=rows, n_vertices=n_vertices, grad=False) if want is None else want
    mean, st = _run(dev, args, rows, n_vertices)
    print(f"{tag} rows={rows}: mean {float(mean):.9f} (restatement {want['mean']:.9f}), N {want['N']}, n_outside {want['n_outside']}")
    assert np.array_equal(st['pair_sum'].cpu().numpy(), want['pair_sum']), tag
    assert np.array_equal(st['pair_count'].cpu().numpy(), want['pair_count']), tag
    assert int(st['n_outside']) == want['n_outside'], tag
    assert mean.dtype == torch.float32 and mean.dim() == 0
    assert mean.cpu().numpy().tobytes() == np.float32(want['mean']).tobytes(), tag
    assert np.array_equal(st['seen'].cpu().numpy() != 0, want['seen']), tag
    return want


def _sign_count(dev, args, rows, n_vertices, g=1.0):
    """ctx_view_consistency_bwd called directly: -> (sign_count [V,C,h,w] int32, grad_views) as numpy."""
    from contexture_nerf_amd import _lib as L
    lib = L.load()
    views, faces, idx, fvi = _dev(dev, *args)
    _, st = _run(dev, args, rows, n_vertices)
    V, C, h, w = views.shape
    sc = torch.empty(V, C, h, w, dtype=torch.int32, device=dev)
    grad = torch.empty_like(views)
    gt = torch.tensor([g], dtype=torch.float32, device=dev)
    L.check(lib.ctx_view_consistency_bwd(L.ptr(views), L.ptr(faces), L.ptr(idx), L.ptr(fvi), L.ptr(st['seen']), V, C, h, w, faces.shape[0], n_vertices,
                                         {'reference': 0, 'image': 1}[rows], L.ptr(st['pair_count']), L.ptr(gt), L.ptr(sc), L.ptr(grad), L.stream()))
    torch.cuda.synchronize()
    return sc.cpu().numpy(), grad.cpu().numpy()


def _autograd(dev, args, rows, n_vertices, g):
    from contexture_nerf_amd import kal
    views, faces, idx, fvi = _dev(dev, *args)
    views.requires_grad_(True)
    mean = kal.view_consistency(views, faces, idx, fvi, rows=rows, n_vertices=n_vertices)
    mean.backward(torch.tensor(float(g), device=dev))
    return views.grad.cpu().numpy()


@pytest.fixture(scope="module")
def gold():
    return VC.load_golden()


@pytest.fixture(scope="module")
def spot_gpu(dev, meshes):
    """size -> (faces, face_idx [6,H,H], fvi [6,F,3,2]) rastered by kal (the product's own raster), as numpy; memoised."""
    from contexture_nerf_amd import kal
    from oracle import geometry as og
    from test_atlas_fill_cpu import spot_arrays
    memo = {}

    def get(H):
        if H not in memo:
            v, f, _, _, cam, proj = spot_arrays(meshes)
            verts = torch.tensor(np.repeat(v[None], 6, 0), device=dev)
            g_cam, g_img, _ = kal.render.mesh.prepare_vertices(verts, torch.tensor(f, device=dev), torch.tensor(proj), camera_transform=torch.tensor(cam[1:7], device=dev))
            _, idx = kal.render.mesh.rasterize(H, H, g_cam[..., 2], g_img, g_cam[..., 2:3])
            memo[H] = (f, idx.cpu().numpy(), g_img.cpu().numpy())
        return memo[H]
    return get


@pytest.fixture(scope="module")
def big(spot_gpu):
    """The 1200-squared case and its restatement (the slow part), computed once per module."""
    f, idx, fvi = spot_gpu(1200)
    views = VC.random_views(7, 6, 3, 1200, 1200)
    args = (views, f, idx, fvi)
    return args, VC.view_consistency(*args, rows='image', n_vertices=int(f.max()) + 1, grad=True)


# ---- 7. forward against the restatement ------------------------------------------------------------------------------------
def test_forward_golden_cases(dev, gold, meshes):
    g = gold
    nV = int(g['faces'].max()) + 1
    vb = VC.case_b_views(meshes, g)
    for rows in ('reference', 'image'):
        _assert_forward(dev, "case A", (g['A_views'], g['faces'], g['face_idx'], g['fvi']), rows, nV)
        w = _assert_forward(dev, "case B", (vb, g['faces'], g['face_idx'], g['fvi']), rows, nV)
        assert abs(float(w['mean']) - float(g[f'B_{rows}_mean'])) <= 2 * float(g[f'B_{rows}_mean_err']) + 2.0 ** -32


@pytest.mark.parametrize("rows", ['reference', 'image'])
@pytest.mark.parametrize("C", [1, 3, 4])
def test_forward_spot_512_channels(dev, spot_gpu, rows, C):
    f, idx, fvi = spot_gpu(512)
    w = _assert_forward(dev, f"spot 512 C={C}", (VC.random_views(C, 6, C, 512, 512), f, idx, fvi), rows, int(f.max()) + 1)
    assert w['N'] > 100000


@pytest.mark.parametrize("V", [1, 2, 6, 16])
def test_forward_spot_512_view_counts(dev, spot_gpu, V):
    f, idx, fvi = spot_gpu(512)
    pick = np.arange(V) % 6                                                    # poses repeated
    w = _assert_forward(dev, f"spot 512 V={V}", (VC.random_views(100 + V, V, 3, 512, 512), f, idx[pick], fvi[pick]), 'image', int(f.max()) + 1)
    assert (w['N'] == 0) == (V == 1)


def test_forward_spot_1200(dev, big, spot_gpu):
    args, want = big
    nV = int(args[1].max()) + 1
    _assert_forward(dev, "spot 1200", args, 'image', nV, want=want)
    _assert_forward(dev, "spot 1200", args, 'reference', nV)


def test_forward_synthetic_inputs(dev, gold):
    nV = int(gold['faces'].max()) + 1
    for name, args in VC.synthetic_cases(gold).items():
        w = _assert_forward(dev, name, args, 'image', nV)
        if name == 'coords_x1.5':
            assert w['n_outside'] > 0
        if name == 'single_view':
            assert w['N'] == 0 and w['mean'] == 0


# ---- 8. backward ----------------------------------------------------------------------------------------------------------
def _assert_backward(dev, tag, args, rows, nV, want):
    C = args[0].shape[1]
    sc, g1 = _sign_count(dev, args, rows, nV, 1.0)
    assert np.array_equal(sc.astype(np.int64), want['sign_count']), tag
    for g in (1.0, -500.0):
        got = _autograd(dev, args, rows, nV, g)
        exp = VC.grad_from_counts(want['sign_count'], want['N'], C, g)
        assert got.dtype == np.float32 and got.tobytes() == exp.tobytes(), (tag, g)
    assert g1.tobytes() == VC.grad_from_counts(want['sign_count'], want['N'], C, 1.0).tobytes()
    print(f"{tag} rows={rows}: sign_count in [{sc.min()}, {sc.max()}], N {want['N']}")
    return sc, g1


def test_backward_counts_and_values(dev, gold, spot_gpu, big):
    g = gold
    nV = int(g['faces'].max()) + 1
    args = (g['A_views'], g['faces'], g['face_idx'], g['fvi'])
    want = VC.view_consistency(*args, rows='reference', n_vertices=nV)
    sc, grad = _assert_backward(dev, "case A", args, 'reference', nV, want)
    VC.check_grad_against_reference(sc, grad, g)                                 # the reference's autograd gradient, rule of the CPU test
    for name, a in VC.synthetic_cases(g).items():
        _assert_backward(dev, name, a, 'image', nV, VC.view_consistency(*a, rows='image', n_vertices=nV))
    f, idx, fvi = spot_gpu(512)
    for C in (1, 4):
        a = (VC.random_views(50 + C, 6, C, 512, 512), f, idx, fvi)
        _assert_backward(dev, f"spot 512 C={C}", a, 'image', int(f.max()) + 1, VC.view_consistency(*a, rows='image', n_vertices=int(f.max()) + 1))
    bargs, bwant = big
    _assert_backward(dev, "spot 1200", bargs, 'image', int(bargs[1].max()) + 1, bwant)


def test_backward_constant_images(dev, gold):
    g = gold
    nV = int(g['faces'].max()) + 1
    args = (np.full_like(g['A_views'], 0.25), g['faces'], g['face_idx'], g['fvi'])
    mean, st = _run(dev, args, 'image', nV)
    assert float(mean) == 1.0 and int(st['pair_count'].sum()) > 0
    assert not _autograd(dev, args, 'image', nV, 1.0).any()                      # sign(0) = 0


# ---- 9. determinism, streams, the kept seen map ------------------------------------------------------------------------------
def test_repeat_side_stream_and_kept_seen_map(dev, spot_gpu):
    from contexture_nerf_amd import kal
    f, idx, fvi = spot_gpu(512)
    nV = int(f.max()) + 1
    t = _dev(dev, VC.random_views(9, 6, 3, 512, 512), f, idx, fvi)

    def once(**kw):
        v = t[0].clone().requires_grad_(True)
        mean, st = kal.view_consistency(v, *t[1:], stats=True, n_vertices=nV, **kw)
        mean.backward()
        return mean.detach(), st, v.grad
    m0, s0, g0 = once()
    m1, s1, g1 = once()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m2, s2, g2 = once()
    side.synchronize()
    m3, s3, g3 = once(seen=s0['seen'])
    assert s3['seen'] is s0['seen']
    for m, s, g in ((m1, s1, g1), (m2, s2, g2), (m3, s3, g3)):
        assert torch.equal(m, m0) and torch.equal(g, g0) and torch.equal(s['pair_sum'], s0['pair_sum']) and torch.equal(s['pair_count'], s0['pair_count'])
        assert torch.equal(s['n_outside'], s0['n_outside']) and torch.equal(s['seen'], s0['seen'])
    with pytest.raises(kal.L.CtxError, match="contiguous"):
        kal.view_consistency(t[0].permute(0, 1, 3, 2), *t[1:], n_vertices=nV)
    with pytest.raises(kal.L.CtxError, match="dtype"):
        kal.view_consistency(t[0], t[1], t[2].int(), t[3], n_vertices=nV)


# ---- 10-12. the host side on tiny engines -------------------------------------------------------------------------------------
def _trainer(dev, tmp_path=None, **optim):
    from contexture_nerf_amd import config as CFG
    from contexture_nerf_amd.trainer import ConTEXTure
    from test_pipeline_gpu import _tiny_sd
    cfg = CFG.TrainConfig()
    cfg.guide.text = "a test mesh"; cfg.guide.shape_path = "shapes/spot_triangulated.obj"
    cfg.guide.texture_resolution = 128; cfg.guide.sd_image_size = 128; cfg.guide.num_inference_steps = 2
    cfg.render.train_grid_size = 192; cfg.render.eval_grid_size = 96
    if tmp_path is not None:
        cfg.log.exp_root = tmp_path; cfg.log.exp_name = "vc"; cfg.log.full_eval_size = 3
    for k, v in optim.items():
        setattr(cfg.optim, k, v)
    sd, _, _ = _tiny_sd(dev)
    return ConTEXTure(cfg, device=dev, diffusion=sd)


def _renders(tr, dev):
    views = tr.train_views
    out = tr.mesh_model.render(theta=[v['theta'] for v in views], phi=[tr._offset_phi(v['phi']) for v in views],
                               radius=[float(v['radius']) for v in views], background=torch.tensor([0.5, 0.5, 0.5], device=dev))
    return out['image'].detach().contiguous(), out['render_cache']


def test_trainer_view_consistency_entry(dev):
    from contexture_nerf_amd import kal
    tr = _trainer(dev)
    tr.paint()
    r = tr.view_consistency()
    V = len(tr.train_views)
    assert set(r) >= {'mean', 'pair_mean', 'pair_count', 'n_outside'} and isinstance(r['mean'], float) and isinstance(r['n_outside'], int)
    pm, pc = np.array(r['pair_mean']), np.array(r['pair_count'])
    assert pm.shape == (V, V) and pc.shape == (V, V) and not np.diag(pm).any() and not np.diag(pc).any()
    assert np.isfinite(pm).all() and (pm >= 0).all() and (pm <= 1).all() and pc.sum() > 0 and 0 <= r['mean'] <= 1
    with torch.no_grad():
        img, rc = _renders(tr, dev)
        direct = kal.view_consistency(img, tr.mesh_model.mesh.faces, rc['face_idx'], rc['face_vertices_image'])
    assert r['mean'] == float(direct)
    sub = tr.view_consistency(images=img[[1, 2, 4]], view_ids=[1, 2, 4], rows='reference')
    assert np.array(sub['pair_count']).shape == (3, 3) and sub['rows'] == 'reference'


def test_sds_loop_consistency_weight(dev, monkeypatch):
    from contexture_nerf_amd import kal
    from test_pipeline_gpu import _tiny_zero123
    real = kal.view_consistency

    def run(weight, spy=None):
        tr = _trainer(dev, consistency_weight=weight)
        _tiny_zero123(dev, tr)
        with monkeypatch.context() as mp:
            if spy is not None:
                mp.setattr(kal, 'view_consistency', spy)
            torch.manual_seed(1234)
            before = [p.detach().clone() for p in tr.texture_mlp.parameters()]
            log = tr.paint_zero123plus(iterations=3, tile=64)
        return log, before, [p.detach().clone() for p in tr.texture_mlp.parameters()]

    def boom(*a, **k):
        raise AssertionError("kal.view_consistency called with consistency_weight = 0")
    log_a, before_a, par_a = run(0.0, spy=boom)                                 # (a) never called
    assert len(log_a) == 3 and all('consistency' not in r for r in log_a)
    log_b, _, par_b = run(0.0)                                                   # (b) unpatched: the same records, float for float
    assert log_a == log_b
    assert all(torch.equal(a, b) for a, b in zip(par_a, par_b))
    calls = []

    def record(views, faces, face_idx, fvi, **kw):
        if not calls:
            calls.append((views.detach().clone(), faces, face_idx, fvi))
        return real(views, faces, face_idx, fvi, **kw)
    log_c, before_c, par_c = run(500.0, spy=record)                              # (c)
    assert all(torch.equal(a, c) for a, c in zip(before_a, before_c))          # the same start
    assert len(log_c) == 3 and all(np.isfinite(r['consistency']) and 0 <= r['consistency'] <= 1 for r in log_c)
    assert log_c[0]['loss'] == log_a[0]['loss']                                  # the record's loss stays the SDS term
    assert log_c[0]['grad_norm'] != log_a[0]['grad_norm']
    assert all(torch.isfinite(p).all() for p in par_c) and any(not torch.equal(a, c) for a, c in zip(par_a, par_c))
    views, faces, face_idx, fvi = calls[0]
    assert views.shape[0] == 6 and face_idx.shape == (6, 192, 192)
    assert log_c[0]['consistency'] == float(real(views, faces, face_idx, fvi))   # a direct call on iteration 0's renders
    print(f"SDS loop, weight 500: consistency {[r['consistency'] for r in log_c]}, grad_norm {log_c[0]['grad_norm']:.4e} against {log_a[0]['grad_norm']:.4e} without")


def test_full_eval_writes_consistency_only_when_asked(dev, tmp_path):
    tr = _trainer(dev, tmp_path / "off")
    tr.cfg.log.save_mesh = False
    tr.full_eval()
    assert not os.path.exists(tr.cfg.log.exp_dir / 'results' / 'view_consistency.json')
    tr = _trainer(dev, tmp_path / "on")
    tr.cfg.log.save_mesh = False
    tr.cfg.log.eval_consistency = True
    tr.full_eval()
    r = json.load(open(tr.cfg.log.exp_dir / 'results' / 'view_consistency.json'))
    assert np.isfinite(r['mean']) and 0 <= r['mean'] <= 1 and len(r['pair_count']) == len(tr.train_views)
