"""CPU: exposure compensation across painted views, the rule (tests/exposure_rule.py) and the product's solve (kal.solve_view_gains).
(a) gains recovered from one texture seen under per-view gains; (b) groups of views without a common texel; (c) threshold exclusion,
counted by hand; (d) one view, clipping; (e) refusals by name; (f) world 2 over gloo: the statistics tensor after the all-reduce and the
gains on both ranks; (g) the config keys."""
import os
import sys
import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import exposure_rule as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_SPAN = float(np.log(1.3 / 0.7))


def _case(seed, V=4, Tc=16, keep=0.7):
    rng = np.random.default_rng(seed)
    texture = rng.uniform(0.2, 0.6, (3, Tc, Tc))
    gains = rng.uniform(0.7, 1.3, (V, 3))
    masks = rng.random((V, Tc, Tc)) < keep
    return texture, gains, masks, R.make_atlases(texture, gains, masks)


def _solve(count, colour_sum, **kw):
    from contexture_nerf_amd import kal
    g = kal.solve_view_gains(torch.from_numpy(count), torch.from_numpy(colour_sum), **kw)
    assert isinstance(g, torch.Tensor) and g.dtype == torch.float64 and g.device.type == 'cpu' and tuple(g.shape) == (count.shape[0], 3)
    assert np.array_equal(g.numpy(), R.solve_view_gains(count, colour_sum, **kw))          # the product restates the rule
    return g.numpy()


def _log_spread(product):
    """max over the channels of log(max over views / min over views)."""
    return float(np.log(product.max(axis=0) / product.min(axis=0)).max())


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_gains_are_recovered(seed):
    texture, true, masks, A = _case(seed)
    count, colour_sum = R.view_pair_stats(A)
    assert (count[np.triu_indices(4, 1)] > 0).all()                       # every pair overlaps
    assert np.array_equal(np.diag(count), masks.reshape(4, -1).sum(1))    # colours in [0.14, 0.78]: every texel of a mask is valid
    g0 = _solve(count, colour_sum, ridge=0.0)
    s0 = _log_spread(g0 * true)
    g1 = _solve(count, colour_sum, ridge=0.01)
    s1 = _log_spread(g1 * true)
    print(f"seed {seed}: log spread of gains * true gains: ridge 0 {s0:.3e}, ridge 0.01 {s1:.3e} (bound {0.01 * LOG_SPAN + 1e-5:.3e})")
    # colours >= 0.14 are quantised to 2^-24: 4.3e-7 relative per texel, so 1e-5 holds with room
    assert s0 <= np.log1p(1e-5)
    assert s1 <= 0.01 * LOG_SPAN + 1e-5


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------
def test_disconnected_groups_and_a_lone_view():
    rng = np.random.default_rng(3)
    V, Tc = 5, 16
    texture = rng.uniform(0.2, 0.6, (3, Tc, Tc))
    true = rng.uniform(0.7, 1.3, (V, 3))
    masks = np.zeros((V, Tc, Tc), bool)
    masks[0, :6], masks[1, 2:8] = True, True                              # group {0, 1}: rows 0..7
    masks[2, 8:13], masks[3, 10:14] = True, True                          # group {2, 3}: rows 8..13
    masks[4, 14:] = True                                                  # view 4 overlaps nobody
    count, colour_sum = R.view_pair_stats(R.make_atlases(texture, true, masks))
    assert count[0, 1] > 0 and count[2, 3] > 0 and count[:2, 2:].sum() == 0 and count[4, :4].sum() == 0 and count[4, 4] == 2 * Tc
    for ridge in (0.0, 0.01):
        g = _solve(count, colour_sum, ridge=ridge)
        p = g * true
        tol = np.log1p(1e-5) if ridge == 0 else 0.01 * LOG_SPAN + 1e-5
        assert _log_spread(p[:2]) <= tol and _log_spread(p[2:4]) <= tol
        assert (g[4] == 1.0).all()
    # ridge = 0: the minimum-norm solution centres each group's log gains on 0
    g = _solve(count, colour_sum, ridge=0.0)
    assert np.abs(np.log(g[:2]).sum(0)).max() <= 1e-12 and np.abs(np.log(g[2:4]).sum(0)).max() <= 1e-12


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------
def test_threshold_exclusion_by_hand():
    one = 2 ** 32
    A = np.zeros((2, 4, 2, 2), np.int64)
    A[:, 3] = one
    A[:, :3] = one // 2                                                   # both views 0.5 everywhere
    A[0, 1, 0, 1] = int(0.99 * one)                                       # view 0, texel (0,1): green above hi
    A[1, 2, 1, 0] = int(0.01 * one)                                       # view 1, texel (1,0): blue below lo
    A[1, 3, 1, 1] = 0                                                     # view 1, texel (1,1): empty
    A[1, :3, 1, 1] = 0
    count, colour_sum = R.view_pair_stats(A, 0.02, 0.98)
    assert count.tolist() == [[3, 1], [1, 2]]                             # view 0: 3 texels, view 1: 2, both: texel (0,0) only
    half = R.Q_ONE // 2
    assert colour_sum[0, 0].tolist() == [3 * half] * 3 and colour_sum[1, 1].tolist() == [2 * half] * 3
    assert colour_sum[0, 1].tolist() == [half] * 3 and colour_sum[1, 0].tolist() == [half] * 3
    # exactly at the thresholds a texel stays in
    lo, hi = np.float32(0.02), np.float32(0.98)
    B = np.zeros((1, 4, 2, 2), np.int64)
    B[0, 3] = one
    B[0, :3, 0, 0] = one // 2                                             # texel (0,0): 0.5; texel (0,1): colour 0, below lo
    for k, c in enumerate((lo, hi)):                                      # texels (1,0), (1,1): c == lo, c == hi exactly
        num = np.float64(c) * one
        assert num == np.rint(num)                                        # a float32 in (2^-8, 1) times 2^32 is an integer
        B[0, :3, 1, k] = int(num)
    cnt, _ = R.view_pair_stats(B, lo, hi)
    assert cnt.tolist() == [[3]]                                          # (0,1) is out; the other three are in
    cnt, _ = R.view_pair_stats(B, np.nextafter(lo, np.float32(1)), np.nextafter(hi, np.float32(0)))
    assert cnt.tolist() == [[1]]


# ---- (d) ----------------------------------------------------------------------------------------------------------------------------
def test_one_view_and_clipping():
    texture, true, masks, A = _case(5, V=1)
    count, colour_sum = R.view_pair_stats(A)
    for ridge in (0.0, 0.01):
        assert (_solve(count, colour_sum, ridge=ridge) == 1.0).all()
    texture = np.full((3, 8, 8), 0.3)
    true = np.array([[0.5, 0.5, 0.5], [2.0, 2.0, 2.0]])                  # a ratio of 4: the free solution is gains (2, 1/2)
    count, colour_sum = R.view_pair_stats(R.make_atlases(texture, true, np.ones((2, 8, 8), bool)))
    g = _solve(count, colour_sum, ridge=0.0, max_gain=4.0)
    assert np.abs(g[0] - 2.0).max() <= 1e-5 and np.abs(g[1] - 0.5).max() <= 1e-5
    g = _solve(count, colour_sum, ridge=0.0, max_gain=1.5)
    assert (g[0] == 1.5).all() and (g[1] == 1 / 1.5).all()
    assert (_solve(count, colour_sum, ridge=0.0, max_gain=1.0) == 1.0).all()


# ---- (e) ----------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from contexture_nerf_amd import _lib as L, kal
    count, colour_sum = R.view_pair_stats(_case(6)[3])
    with pytest.raises(L.CtxError, match="solve_view_gains: ridge"):
        kal.solve_view_gains(count, colour_sum, ridge=-0.1)
    with pytest.raises(L.CtxError, match="solve_view_gains: ridge"):
        kal.solve_view_gains(count, colour_sum, ridge=float('nan'))
    with pytest.raises(L.CtxError, match="solve_view_gains: max_gain"):
        kal.solve_view_gains(count, colour_sum, max_gain=0.99)
    with pytest.raises(L.CtxError, match=r"solve_view_gains: want count \[V,V\]"):
        kal.solve_view_gains(count, colour_sum[:, :, :2])
    z = lambda *s: torch.zeros(*s, dtype=torch.int64)
    with pytest.raises(L.CtxError, match=r"view_pair_stats: want atlases \[V,4,Tc,Tc\]"):
        kal.view_pair_stats(z(2, 3, 8, 8))
    with pytest.raises(L.CtxError, match=r"view_pair_stats: want atlases \[V,4,Tc,Tc\]"):
        kal.view_pair_stats(z(2, 4, 8, 4))
    with pytest.raises(L.CtxError, match=r"view_pair_stats: V=17 outside \[1, 16\]"):
        kal.view_pair_stats(z(17, 4, 2, 2))
    with pytest.raises(L.CtxError, match=r"view_pair_stats: V=0 outside \[1, 16\]"):
        kal.view_pair_stats(z(0, 4, 2, 2))
    with pytest.raises(L.CtxError, match=r"view_pair_stats: Tc=0 outside \[1, 4096\]"):
        kal.view_pair_stats(z(1, 4, 0, 0))
    for lo, hi in ((0.0, 0.98), (0.5, 0.5), (0.6, 0.5), (0.02, 1.01), (float('nan'), 0.9)):
        with pytest.raises(L.CtxError, match="view_pair_stats: lo="):
            kal.view_pair_stats(z(1, 4, 2, 2), lo, hi)
    with pytest.raises(L.CtxError, match="atlases: expected a device tensor"):      # inside the envelope: there is no CPU fallback
        kal.view_pair_stats(z(1, 4, 2, 2))


# ---- (f) ----------------------------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, tmp):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from contexture_nerf_amd import dist as D, kal
    import exposure_rule as R_
    r, w, dev = D.init(backend="gloo")
    assert (r, w) == (rank, world) and dev.type == "cpu"
    V = 5
    _, _, _, full = _case(7, V=V)                                         # same data on every rank
    mine = D.shard_views(V, rank, world)
    stats = torch.zeros(full.shape, dtype=torch.int64)
    stats[mine] = torch.from_numpy(full[mine])                            # each rank fills its own views' slices
    assert not torch.equal(stats, torch.from_numpy(full))
    D.all_reduce_sum_(stats)
    assert torch.equal(stats, torch.from_numpy(full))                     # == the 1-rank tensor
    count, colour_sum = R_.view_pair_stats(stats.numpy())
    gains = kal.solve_view_gains(count, colour_sum)
    torch.save(gains, os.path.join(tmp, f"gains{rank}.pt"))
    dist.destroy_process_group()


def test_world2_statistics_and_gains(tmp_path):
    port = 31500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    g0, g1 = (torch.load(tmp_path / f"gains{r}.pt", weights_only=True).numpy() for r in (0, 1))
    assert np.array_equal(g0, g1)
    one = R.solve_view_gains(*R.view_pair_stats(_case(7, V=5)[3]))
    assert np.array_equal(g0, one) and not (one == 1.0).all()


# ---- (g) ----------------------------------------------------------------------------------------------------------------------------
def test_config_keys():
    from contexture_nerf_amd import config as CFG
    cfg = CFG.parse(argv=[])
    g = cfg.guide
    assert (g.exposure_compensation, g.exposure_resolution, g.exposure_ridge, g.exposure_max_gain, g.exposure_z_min) == (False, 256, 0.01, 2.0, 0.25)
    cfg = CFG.parse(argv=["--guide.exposure_compensation=true", "--guide.exposure_resolution=64", "--guide.exposure_ridge=0"])
    assert cfg.guide.exposure_compensation is True and cfg.guide.exposure_resolution == 64 and cfg.guide.exposure_ridge == 0.0
    with pytest.raises(ValueError, match="exposure_compensation.*progressive"):
        CFG.parse(argv=["--guide.exposure_compensation=true", "--guide.paint_mode=progressive"])
    CFG.parse(argv=["--guide.paint_mode=progressive"])                    # the switch off: progressive stays legal
    for bad in ("--guide.exposure_resolution=0", "--guide.exposure_resolution=4097", "--guide.exposure_ridge=-1", "--guide.exposure_max_gain=0.5"):
        with pytest.raises(ValueError, match="guide.exposure_"):
            CFG.parse(argv=["--guide.exposure_compensation=true", bad])
