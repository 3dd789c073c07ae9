"""CPU: the rules of the progressive paint loop as tests/trimap_rule.py states them (morphology, taps and blur, trimap, checkerboard,
the atlas blend in integers), and the config surface of guide.paint_mode.  No GPU, no kernel: tests/test_trimap_gpu.py holds the
kernels and the trainer to these rules."""
import numpy as np
import pytest

import trimap_rule as R

F32 = np.float32
ONE = 1 << 32


# ---- morphology ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (37, 129)])
@pytest.mark.parametrize("k", [1, 3, 7, 19, 63])
def test_morph_equals_scipy(shape, k):
    """scipy's constant border at the operator's neutral element within [0,1] (0 for max, 1 for min) is the clipped window."""
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(k * 1000 + shape[1])
    for x in (rng.random(shape).astype(F32), (rng.random(shape) < 0.3).astype(F32)):
        assert np.array_equal(R.dilate(x, k), ndimage.maximum_filter(x, size=k, mode='constant', cval=0.0))
        assert np.array_equal(R.erode(x, k), ndimage.minimum_filter(x, size=k, mode='constant', cval=1.0))


def test_morph_hand_cases():
    x = np.zeros((9, 11), F32); x[0, 0] = 1
    want = np.zeros_like(x); want[:3, :3] = 1                      # a 5 x 5 square centred on the corner, clipped to 3 x 3
    assert np.array_equal(R.dilate(x, 5), want)
    y = np.random.default_rng(0).random((6, 8)).astype(F32)
    assert np.array_equal(R.dilate(y, 1), y) and np.array_equal(R.erode(y, 1), y)
    assert np.array_equal(R.dilate(y, 63), np.full_like(y, y.max())) and np.array_equal(R.erode(y, 63), np.full_like(y, y.min()))   # k > H, W
    assert np.array_equal(R.erode(np.ones((4, 4), F32), 7), np.ones((4, 4), F32))        # the border does not erode: outside takes no part
    batch = np.stack([y, 1 - y])
    assert np.array_equal(R.dilate(batch, 3)[1], R.dilate(1 - y, 3))


def test_opening_removes_specks_and_keeps_blocks():
    x = np.zeros((12, 12), F32)
    x[2, 2] = 1                                                     # a one-pixel speckle
    x[6:9, 5:8] = 1                                                 # a 3 x 3 block
    opened = R.dilate(R.erode(x, 3), 3)
    want = np.zeros_like(x); want[6:9, 5:8] = 1
    assert np.array_equal(opened, want)


# ---- taps and blur ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,sigma", [(1, 1.0), (3, 2.1333), (21, 16.0), (63, 16.0), (63, 0.5)])
def test_taps(k, sigma):
    t = R.gaussian_taps(k, sigma)
    assert t.dtype == F32 and t.shape == (k,) and (t >= 0).all() and np.array_equal(t, t[::-1])
    assert abs(float(t.astype(np.float64).sum()) - 1.0) <= k * 2.0 ** -24       # k roundings of half an ulp of a value <= 1
    assert t.argmax() == k // 2


def test_product_taps_are_the_rule():
    from contexture_nerf_amd import kal
    for k, sigma in [(1, 1.0), (3, 2.1333), (21, 16.0), (63, 7.0)]:
        assert np.array_equal(np.asarray(kal.gaussian_taps(k, sigma), F32), R.gaussian_taps(k, sigma))
    from contexture_nerf_amd._lib import CtxError
    with pytest.raises(CtxError, match="odd"):
        kal.gaussian_taps(4, 1.0)


@pytest.mark.parametrize("k", [1, 3, 21, 63])
def test_blur_of_a_constant_and_float64_twin(k):
    """Constant c: the exact result is c * (sum of taps)^2, and the taps sum to 1 within k 2^-24, so |exact - c| <= 2k 2^-24 c (first
    order); the float32 evaluation adds sep_filter_bound = 2k 2^-24 c.  Together 4k 2^-24 c, with 2^-20 c for the second-order terms."""
    H, W = 40, 70
    taps = R.gaussian_taps(k, 16.0 * 160 / 1200)
    c = F32(0.7)
    out = R.sep_filter(np.full((H, W), c, F32), taps)
    assert np.abs(out.astype(np.float64) - float(c)).max() <= (4 * k * 2.0 ** -24 + 2.0 ** -20) * float(c)
    x = (np.random.default_rng(k).random((2, H, W)) * 3 - 1).astype(F32)
    f32, f64 = R.sep_filter(x, taps), R.sep_filter(x, taps, np.float64)
    assert f32.dtype == F32
    assert np.abs(f32.astype(np.float64) - f64).max() <= R.sep_filter_bound(k, np.abs(x).max())
    # the twin is np.pad(mode='reflect') + a plain correlation: index -1 reads 1
    r = k // 2
    p = np.pad(x[0].astype(np.float64), r, mode='reflect')
    t64 = taps.astype(np.float64)
    rows = sum(t64[j] * p[:, j:j + W] for j in range(k))
    cols = sum(t64[j] * rows[j:j + H] for j in range(k))
    assert np.allclose(cols, f64[0], rtol=0, atol=1e-12)


def test_blur_refuses_a_window_wider_than_the_reflection():
    with pytest.raises(AssertionError):
        R.sep_filter(np.zeros((5, 40), F32), R.gaussian_taps(21, 3.0))          # k/2 = 10 > H - 1 = 4


# ---- trimap ---------------------------------------------------------------------------------------------------------------------------
def test_scaled_radii():
    from contexture_nerf_amd import trainer
    assert [R.scaled_k(k0, 1200) for k0 in (19, 7, 5, 25, 21)] == [19, 7, 5, 25, 21]
    assert trainer.TRIMAP_K0 == R.K0
    for G in (64, 160, 512, 1024, 1200, 2048):
        for k0 in R.K0.values():
            assert trainer.scaled_k(k0, G) == R.scaled_k(k0, G) and R.scaled_k(k0, G) % 2 == 1
    assert [R.scaled_k(k0, 160) for k0 in (19, 7, 5, 25, 21)] == [3, 1, 1, 5, 3]
    assert R.blur_sigma(1200) == 16.0


def _scene(G=1200 // 10):
    obj = np.zeros((G, G), F32); obj[20:100, 30:90] = 1
    return G, obj


def test_trimap_first_view_generates_the_object():
    G, obj = _scene()
    z = np.full((G, G), 0.8, F32)
    none = np.zeros((G, G), F32)
    update, generate, refine = R.calculate_trimap(obj, z, none, none, G)
    assert (generate[obj > 0] == 1).all() and (update[obj > 0] == 1).all() and (refine == 0).all()
    assert np.array_equal(generate, R.dilate(obj, R.scaled_k(19, G)))


def test_trimap_refine_and_keep():
    G, obj = _scene()
    painted = np.zeros((G, G), F32); painted[20:100, 30:90] = 1             # everything painted ...
    z_cache = np.full((G, G), 0.3, F32) * painted                          # ... at 0.3
    seen = np.full((G, G), 0.9, F32)
    update, generate, refine = R.calculate_trimap(obj, seen, painted, z_cache, G)
    assert (generate == 0).all() and (refine[obj > 0] == 1).all() and (refine[obj == 0] == 0).all()
    rim = R.erode(obj, R.scaled_k(7, G))
    assert np.array_equal(update, refine * (rim > 0))                       # refine, minus the object's rim
    seen = np.full((G, G), 0.4, F32)                                        # 0.4 is not 0.2 better than 0.3: keep
    update, generate, refine = R.calculate_trimap(obj, seen, painted, z_cache, G)
    assert (update == 0).all() and (generate == 0).all() and (refine == 0).all()
    # half painted: the unpainted half generates (and its dilation reaches into the painted half), the painted half is kept at 0.4
    painted[:, 60:] = 0
    z_cache = z_cache * painted
    update, generate, refine = R.calculate_trimap(obj, seen, painted, z_cache, G)
    r = R.scaled_radius(9, G)
    assert (generate[20:100, 60 - r:90] == 1).all() and (generate[20:100, 30:60 - r] == 0).all() and (refine == 0).all()
    assert np.array_equal(update, generate)


def test_checkerboard():
    G, S = 64, 128
    update = np.zeros((G, G), F32); update[8:56, 8:56] = 1
    generate = np.zeros((G, G), F32); generate[8:56, 8:30] = 1
    refine = np.zeros((G, G), F32); refine[8:56, 24:56] = 1
    m = R.checker_mask(update, refine, generate, S)
    gen_s, ref_s = R.nearest_resize(generate, S) > 0, R.nearest_resize(refine, S) > 0
    assert (m[gen_s] == 1).all()                                            # generate stays 1, also where it is refined too
    board = R.checker_board(S)
    only = ref_s & ~gen_s
    assert only.any() and np.array_equal(m[only], board[only])
    assert np.array_equal(m[~ref_s & ~gen_s], R.nearest_resize(update, S)[~ref_s & ~gen_s])
    c = S // 32
    assert board[0, 0] == 0 and board[0, c] == 1 and board[c, c] == 0 and board[c - 1, c - 1] == 0 and set(np.unique(board)) == {0.0, 1.0}
    assert np.array_equal(R.checker_board(512)[::8, ::8][:4, :4], np.float32([[0, 0, 1, 1], [0, 0, 1, 1], [1, 1, 0, 0], [1, 1, 0, 0]]))  # two latent pixels


def test_projection_weight_rule():
    G, obj = _scene()
    none = np.zeros((G, G), F32)
    z = np.full((G, G), 0.8, F32)
    update, _, _ = R.calculate_trimap(obj, z, none, none, G)
    w = R.projection_weight(obj, update, z, none, none, G)
    oe = R.erode(obj, R.scaled_k(5, G))
    assert (w[oe == 0] == 0).all() and w.max() <= 1 + 1e-6 and ((w == 0) | (w >= 0.5)).all()
    assert (w[40:80, 50:70] > 0.999).all()                                  # deep inside: the blur of ones
    painted = obj.copy()
    w2 = R.projection_weight(obj, update, z, painted, np.full((G, G), 0.9, F32), G)      # an earlier view was more frontal everywhere
    assert (w2 == 0).all()
    w3 = R.projection_weight(obj, update, z, painted, np.full((G, G), 0.9, F32), G, strict=False)
    assert np.array_equal(w3 > 0, (oe > 0) & (w3 > 0)) and w3[60, 60] > 0.999


# ---- the blend rule in integers -------------------------------------------------------------------------------------------------------
def _fixed(x):
    return np.rint(np.ldexp(np.asarray(x, np.float64), 32)).astype(np.int64)


def _blend_case(T=9, seed=0):
    rng = np.random.default_rng(seed)
    w = rng.random((T, T)) * 1.5                                            # weights below and above 1
    w[rng.random((T, T)) < 0.3] = 0
    w[0, 0] = -0.25                                                         # w <= 0: untouched
    if T > 1:
        w[0, 1] = 0
    rgb = rng.random((3, T, T))
    contrib = np.concatenate([_fixed(rgb * w), _fixed(w)[None]])
    zsum = _fixed(rng.random((T, T)) * w)
    acc = np.concatenate([_fixed(rng.random((3, T, T))), np.full((1, T, T), ONE, np.int64)])
    unpainted = rng.random((T, T)) < 0.4
    acc[:, unpainted] = 0
    meta = (rng.random((T, T)) * ~unpainted).astype(F32)
    return contrib, zsum, acc, meta, unpainted


def test_blend_rule_in_integers():
    contrib, zsum, acc, meta, unpainted = _blend_case()
    acc0, meta0, contrib0 = acc.copy(), meta.copy(), contrib.copy()
    out, mout = R.atlas_blend(contrib, zsum, acc, meta)
    assert np.array_equal(acc, acc0) and np.array_equal(meta, meta0) and np.array_equal(contrib, contrib0)      # inputs untouched
    miss = contrib[3] <= 0
    assert miss[0, 0] and miss[0, 1]
    assert np.array_equal(out[:, miss], acc[:, miss]) and np.array_equal(mout[miss].view(np.uint32), meta[miss].view(np.uint32))
    hit = ~miss
    assert (out[3][hit] == ONE).all()
    # an unpainted texel takes `new` fully, for any m
    with np.errstate(divide='ignore', invalid='ignore'):
        new = (np.ldexp(contrib[:3].astype(np.float64), -32).astype(F32) / np.ldexp(contrib[3].astype(np.float64), -32).astype(F32)).astype(F32)
    fresh = hit & unpainted
    assert fresh.any() and np.array_equal(out[:3][:, fresh], _fixed(new[:, fresh]))
    assert (np.ldexp(contrib[3][fresh].astype(np.float64), -32) < 1).any()                                      # ... also with m < 1
    # m = 1 replaces
    full = hit & ~unpainted & (contrib[3] >= ONE)
    assert full.any() and np.array_equal(out[:3][:, full], _fixed(new[:, full]))
    with np.errstate(divide='ignore', invalid='ignore'):
        z = (np.ldexp(zsum.astype(np.float64), -32).astype(F32) / np.ldexp(contrib[3].astype(np.float64), -32).astype(F32)).astype(F32)
    assert np.array_equal(mout[full], z[full]) and np.array_equal(mout[fresh], z[fresh])
    # in between: a convex combination, within the float32 rounding of the two products, the sum and the 2^-32 grid
    part = hit & ~unpainted & (contrib[3] < ONE)
    assert part.any()
    m = np.ldexp(contrib[3][part].astype(np.float64), -32)
    old = np.ldexp(acc[:3][:, part].astype(np.float64), -32)
    want = old * (1 - m) + new[:, part].astype(np.float64) * m
    assert np.abs(np.ldexp(out[:3][:, part].astype(np.float64), -32) - want).max() <= 4 * 2.0 ** -24
    # the atlas the rest of the pipeline reads: colours in [0, 1], coverage exactly 1 or 0
    cov = np.ldexp(out[3].astype(np.float64), -32)
    assert set(np.unique(cov[hit | ~unpainted])) == {1.0} and (cov[miss & unpainted] == 0).all()


# ---- config -----------------------------------------------------------------------------------------------------------------------------
def test_config_paint_mode():
    from contexture_nerf_amd import config as CFG
    cfg = CFG.TrainConfig()
    assert cfg.guide.paint_mode == 'independent' and CFG.validate(cfg) is cfg
    assert CFG.parse(argv=['--guide.paint_mode=progressive']).guide.paint_mode == 'progressive'
    with pytest.raises(ValueError, match="paint_mode"):
        CFG.parse(argv=['--guide.paint_mode=sequential'])
    assert cfg.guide.z_update_thr == 0.2 and cfg.guide.strict_projection is True


def test_default_mode_takes_the_batch_painter(monkeypatch):
    """paint() under the default mode builds MeshBatchPainter and touches nothing of the progressive loop."""
    from contexture_nerf_amd import config as CFG, trainer
    calls = []

    class Painter:
        def __init__(self, trainers, view_ids=None, group=None):
            calls.append(('init', list(view_ids)))

        def paint_all(self, image_size, steps):
            calls.append(('paint_all', image_size, steps))
            return [('atlas', 'cov')]

    monkeypatch.setattr(trainer, 'MeshBatchPainter', Painter)
    tr = trainer.ConTEXTure.__new__(trainer.ConTEXTure)
    tr.cfg, tr.train_views, tr.group, tr.world = CFG.TrainConfig(), [{}] * 3, None, 1
    for name in ('paint_progressive', 'begin_progressive', 'paint_view_progressive', 'calculate_trimap', 'projection_weight', 'checker_mask'):
        monkeypatch.setattr(trainer.ConTEXTure, name, lambda *a, **k: pytest.fail("the default mode reached the progressive loop"))
    assert tr.paint(64, 2) == ('atlas', 'cov')
    assert calls == [('init', [0, 1, 2]), ('paint_all', 64, 2)]
    assert not hasattr(tr, 'trimaps') and not hasattr(tr, 'atlas_meta')


def test_progressive_mode_dispatch_and_rank_refusal(monkeypatch):
    from contexture_nerf_amd import config as CFG, trainer
    tr = trainer.ConTEXTure.__new__(trainer.ConTEXTure)
    tr.cfg, tr.train_views, tr.group, tr.world = CFG.TrainConfig(), [{}] * 3, None, 2
    tr.cfg.guide.paint_mode = 'progressive'
    with pytest.raises(RuntimeError, match="2 ranks"):
        tr.paint()
    tr.cfg.guide.paint_mode = 'both'
    with pytest.raises(ValueError, match="paint_mode"):
        tr.paint()
    tr.cfg.guide.paint_mode = 'progressive'
    monkeypatch.setattr(trainer.ConTEXTure, 'paint_progressive', lambda self, a, b: ('progressive', a, b))
    assert tr.paint(96, 3) == ('progressive', 96, 3)
