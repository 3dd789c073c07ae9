"""CPU: the rule of the texture field's 2-D hash grid (tests/hashtex_rule.py) against float64 - the interpolation, the
integer accumulator of the table's gradient and the mutations it must tell apart, the node uv against torch.linspace, the dense / hashed
classification, the config surface, the host refusals, and the schedule of the fit that tests/test_hashtex_gpu.py repeats on the device."""
import functools
import glob
import math
import os
import numpy as np
import pytest
import torch

import hashtex_rule as HT

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. forward ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lv,F,log2T", HT.TABLE_CASES)
@pytest.mark.parametrize("max_res", HT.MAX_RES_CASES)
def test_forward_vs_float64(Lv, F, log2T, max_res):
    """Within 8 * 2^-24 * sum_c |w_c t_c| per feature: w is exact (pos - i with i <= pos < i + 1 or the clamp), each 1 - w is one rounding,
    sx*sy one and * t_c one, so a corner carries at most 4; the 4-term sum adds at most 3; 7 in first order, 8 with room for the
    second-order terms.  All three ways to name the rows."""
    res = HT.resolutions(Lv, 2, max_res)
    table = HT.case_table(Lv, F, log2T, seed=Lv + F)
    worst = 0.0
    for kw in (dict(uv=HT.case_points(300, res, seed=Lv)), dict(grid=33), dict(idx=HT.case_list(33, 65, seed=3), grid=33)):
        got = HT.forward_np(table, res, log2T, **kw)
        want, mag = HT.forward_f64(table, res, log2T, **kw)
        assert got.dtype == f32 and got.shape == want.shape and np.all(np.isfinite(got))
        bound = 8 * 2.0 ** -24 * mag
        err = np.abs(got.astype(np.float64) - want)
        assert np.all(err <= bound)
        worst = max(worst, float((err[mag > 0] / bound[mag > 0]).max()))
    print(f"forward Lv={Lv} F={F} log2T={log2T} max_res={max_res}: worst share of the bound {worst:.3f}")
    assert 0 < worst <= 1
    bad = HT.case_list(33, 65, seed=3)
    assert not HT.forward_np(table, res, log2T, idx=bad, grid=33)[65 // 2].any()        # the out-of-range entry: a zero row


def test_node_returns_its_entry_and_wild_points_stay_in_range():
    res = np.array([2, 4, 8, 16], np.int32)
    table = HT.case_table(4, 2, 6, seed=1)
    rng = np.random.default_rng(2)
    for l, r in enumerate(res):
        g = rng.integers(0, r + 1, (40, 2))
        g[0], g[1] = (0, 0), (r, r)
        emb = HT.forward_np(table, res, 6, uv=(g / r).astype(f32))
        k = g[:, 0] + (r + 1) * g[:, 1] if HT.is_dense(r, 6) else HT.hash_index(g[:, 0], g[:, 1], 6).astype(np.int64)
        assert np.array_equal(emb[:, l * 2:(l + 1) * 2], table[l, k])
    bad = f32([[np.nan, np.nan], [np.inf, -np.inf], [1e30, -3e38], [-5, 7], [np.nan, 0.3]])
    for r in HT.resolutions(16, 2, 1 << 20):
        idx, w = HT.cell_np(bad, int(r), 8)
        assert idx.min() >= 0 and idx.max() < 256 and np.all(np.isfinite(w)) and w.min() >= 0 and w.max() <= 1
    assert np.array_equal(HT.forward_np(table, res, 6, uv=bad[:2]), HT.forward_np(table, res, 6, uv=f32([[0, 0], [1, 0]])))


# ---- 2. backward ---------------------------------------------------------------------------------------------------------------------
def _few_bits(x, bits):
    m, e = np.frexp(np.asarray(x, np.float64))
    return np.ldexp(np.rint(np.ldexp(m, bits)), e - bits).astype(f32)


def _autograd_f64(g_emb, res, log2T, F, **rows):
    table = torch.zeros(len(res), 1 << log2T, F, dtype=torch.float64, requires_grad=True)
    (HT.forward_torch(table, res, log2T, **rows) * torch.from_numpy(np.asarray(g_emb, np.float64))).sum().backward()
    return table.grad.numpy()


def _accumulator_bound(g_emb, res, log2T, F, uv):
    """Per entry: every term is rounded to a multiple of 2^(x-E), so it is off by at most 2^(x-E-1), and an entry receives one term per
    (row, corner) that addresses it.  The float64 reference adds the same terms with a relative error of 2^-53 per addition of partial
    sums that stay below the sum of the terms' magnitudes (the gradient of |g_emb|: the weights are not negative)."""
    n = g_emb.shape[0]
    x = math.frexp(float(np.abs(g_emb).max()))[1]
    E = 62 - HT.ceil_log2_4n(n)
    count = np.zeros((len(res), 1 << log2T))
    for l in range(len(res)):
        k, _ = HT.cell_np(uv, int(res[l]), log2T)
        np.add.at(count[l], k.reshape(-1), 1)
    return count[:, :, None] * (2.0 ** (x - E - 1) + 2.0 ** -53 * _autograd_f64(np.abs(g_emb), res, log2T, F, uv=uv))


@pytest.mark.parametrize("scale", [1.0, 1e-30, 1e20])
def test_integer_backward_vs_float64_autograd_and_mutations(scale):
    """The integer backward against float64 autograd through the torch restatement, before the final cast (as_double), on inputs whose
    float32 products are exact, as tests/test_hashgrid_cpu.py does for 3-D: the unit square with resolutions 2, 4, 8, 16 and coordinates
    k / 64 give corner weights of at most 8 bits, g_emb has 9.  What is left is the accumulator's own error, bounded per entry by
    (number of terms) * 2^(x-E-1); on these inputs it is far inside 2^-40 of the largest gradient too.  Three wrong rules leave that
    bound: u and v swapped, the dense index with the stride the third axis has in 3-D, and g_emb read with the level as the fast index."""
    n, Lv, F, log2T = 300, 4, 2, 6
    res = np.array([2, 4, 8, 16], np.int32)
    assert [HT.is_dense(r, log2T) for r in res] == [True, True, False, False]
    rng = np.random.default_rng(11)
    uv = (rng.integers(0, 65, (n, 2)) / 64).astype(f32)
    g_emb = _few_bits(rng.standard_normal((n, Lv * F)) * scale, 9)
    want = _autograd_f64(g_emb, res, log2T, F, uv=uv)
    bound = _accumulator_bound(g_emb, res, log2T, F, uv)
    got = HT.backward_np(g_emb, res, log2T, F, uv=uv, as_double=True)
    m = np.abs(want).max()
    assert m > 0 and np.all(np.abs(got - want) <= bound) and np.abs(got - want).max() <= 2.0 ** -40 * m
    assert np.array_equal(HT.backward_np(g_emb, res, log2T, F, uv=uv), got.astype(f32))
    for mutate in ('swap_axes', 'dense3d', 'colstride'):
        bad = HT.backward_np(g_emb, res, log2T, F, uv=uv, as_double=True, mutate=mutate)
        assert not np.all(np.abs(bad - want) <= bound), mutate


def test_the_exponent_of_the_accumulator_is_the_2d_one():
    """E = 62 - ceil(log2(4n)), one more than 3-D's: n rows on node (0, 0) of a one-cell level put one term each on entry 0.  One row
    carries m = 1 (x = 1); the others carry 0.75 * 2^(x-E), which the rule rounds to one unit each: off by 0.25 units per term, half
    the integer part of the bound.  With 3-D's E the same terms are 0.375 units and round to 0: off by 1.5 times that part, which the
    float64 reference's own share (a quarter of it here) does not cover."""
    n, res, log2T = 300, np.array([1], np.int32), 4
    E = 62 - HT.ceil_log2_4n(n)
    uv = np.zeros((n, 2), f32)
    g_emb = np.full((n, 1), 0.75 * 2.0 ** (1 - E), f32)
    g_emb[0] = 1.0
    want = _autograd_f64(g_emb, res, log2T, 1, uv=uv)
    bound = _accumulator_bound(g_emb, res, log2T, 1, uv)
    got = HT.backward_np(g_emb, res, log2T, 1, uv=uv, as_double=True)
    assert np.all(np.abs(got - want) <= bound) and abs(got[0, 0, 0] - want[0, 0, 0]) > 0.3 * bound[0, 0, 0]
    bad = HT.backward_np(g_emb, res, log2T, 1, uv=uv, as_double=True, mutate='E3d')
    assert abs(bad[0, 0, 0] - want[0, 0, 0]) > bound[0, 0, 0]


def test_backward_zero_nan_order_and_dead_rows():
    n, Lv, F, log2T = 65, 4, 2, 6
    res = HT.resolutions(Lv, 2, 64)
    uv = HT.case_points(n, res, seed=13)
    g = np.random.default_rng(6).standard_normal((n, Lv * F)).astype(f32)
    z = HT.backward_np(np.zeros_like(g), res, log2T, F, uv=uv)
    assert z.shape == (Lv, 1 << log2T, F) and not z.any()
    for bad in (np.nan, np.inf, -np.inf):
        gb = g.copy()
        gb[17, 3] = bad
        assert np.all(np.isnan(HT.backward_np(gb, res, log2T, F, uv=uv)))
    perm = np.random.default_rng(7).permutation(n)                      # the order of the rows does not matter
    assert np.array_equal(HT.backward_np(g, res, log2T, F, uv=uv), HT.backward_np(g[perm], res, log2T, F, uv=uv[perm]))
    # a list entry outside the atlas takes no part: neither its gradient nor its NaN, nor its magnitude in m
    idx = HT.case_list(33, 64, seed=5)
    dead = 32
    assert not 0 <= idx[dead] < 33 * 33
    live = np.delete(idx, dead)
    for v in (np.nan, 1e30, 0.0):
        gd = g.copy()
        gd[dead] = v
        got = HT.backward_np(gd, res, log2T, F, idx=idx, grid=33, as_double=True)
        ref = HT.backward_np(np.delete(g, dead, 0), res, log2T, F, idx=live, grid=33, as_double=True)
        assert np.all(np.isfinite(got)) and np.abs(got - ref).max() <= 2.0 ** -40 * np.abs(ref).max()   # n differs by one row: E may too
    # the whole atlas is the list of all nodes is the points at the nodes' uv
    ga = np.random.default_rng(8).standard_normal((64, Lv * F)).astype(f32)
    a = HT.backward_np(ga, res, log2T, F, grid=8)
    assert np.array_equal(a, HT.backward_np(ga, res, log2T, F, idx=np.arange(64), grid=8))
    assert np.array_equal(a, HT.backward_np(ga, res, log2T, F, uv=HT.node_uv(8, np.arange(64))))


# ---- 3. node uv and the classification ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [2, 3, 8, 33, 1024])
def test_node_uv_is_torch_linspace(g):
    lin = torch.linspace(0, 1, g).numpy()
    uv = HT.node_uv(g, np.arange(g * g) if g < 1024 else np.arange(g * g).reshape(g, g)[::37].reshape(-1))
    nodes = np.arange(g * g) if g < 1024 else np.arange(g * g).reshape(g, g)[::37].reshape(-1)
    assert uv.dtype == f32 and np.array_equal(uv[:, 0], lin[nodes % g]) and np.array_equal(uv[:, 1], lin[nodes // g])
    assert np.array_equal(HT.node_uv(g, np.arange(g))[:, 0], lin)                  # one whole row of the atlas, every size
    assert np.array_equal(HT.node_uv(g, np.arange(g) * g)[:, 1], lin)              # and one whole column


def test_dense_and_hashed_at_the_boundary():
    """(res + 1)^2 = T exactly is dense.  T = 64: res 6 and 7 are dense (49 and 64 nodes), res 8 is hashed (81)."""
    assert HT.is_dense(6, 6) and HT.is_dense(7, 6) and not HT.is_dense(8, 6)
    assert HT.is_dense(3, 4) and not HT.is_dense(4, 4) and HT.is_dense(2047, 22) and not HT.is_dense(2048, 22)
    for res in (6, 7, 8):
        g = np.stack(np.meshgrid(np.arange(res), np.arange(res), indexing='ij'), -1).reshape(-1, 2)
        idx, _ = HT.cell_np(((g + 0.5) / res).astype(f32), res, 6)
        nodes = {}
        clash = False
        for row, cell in zip(idx, g):
            for c in range(4):
                node = (cell[0] + (c & 1), cell[1] + ((c >> 1) & 1))
                want = node[0] + (res + 1) * node[1] if res < 8 else int(HT.hash_index(node[0], node[1], 6))
                assert int(row[c]) == want
                clash |= nodes.setdefault(int(row[c]), node) != node
        assert idx.max() < 64
        assert clash == (res == 8) and (res == 8 or len(nodes) == (res + 1) ** 2)   # dense: one index per node; 81 nodes cannot fit 64
    assert int(HT.hash_index(1, 0, 22)) == 1 and int(HT.hash_index(0, 1, 22)) == 2654435761 % (1 << 22)
    assert int(HT.hash_index(3, 5, 4)) == (3 ^ (5 * 2654435761 % 2 ** 32)) % 16


# ---- 4. config -----------------------------------------------------------------------------------------------------------------------
def test_config_texture_field_default_cli_and_validation(tmp_path):
    from contexture_nerf_amd import config as CFG
    cfg = CFG.TrainConfig()
    assert cfg.guide.texture_field == 'mlp' and CFG.parse(argv=[]).guide.texture_field == 'mlp'
    assert (cfg.guide.hashgrid_levels, cfg.guide.hashgrid_features, cfg.guide.hashgrid_log2_table, cfg.guide.hashgrid_base_res) == (12, 2, 18, 16)
    assert (cfg.optim.hashgrid_lr, cfg.optim.hashgrid_mlp_lr) == (1e-2, 1e-3)
    cfg = CFG.parse(argv=['--guide.texture_field=hashgrid', '--guide.hashgrid_levels=8', '--optim.hashgrid_lr=0.02'])
    assert cfg.guide.texture_field == 'hashgrid' and cfg.guide.hashgrid_levels == 8 and cfg.optim.hashgrid_lr == 0.02
    with pytest.raises(ValueError, match="texture_field"):
        CFG.parse(argv=['--guide.texture_field=voxels'])
    with pytest.raises(ValueError, match="hashgrid_lr"):
        CFG.parse(argv=['--optim.hashgrid_lr=0'])
    y = tmp_path / "c.yaml"
    y.write_text("guide:\n  texture_field: hashgrid\n")
    cfg = CFG.parse(argv=[f'--config_path={y}'])
    assert cfg.guide.texture_field == 'hashgrid'
    CFG.dump(cfg, tmp_path / "d.yaml")
    assert CFG.parse(argv=[f'--config_path={tmp_path / "d.yaml"}']).guide.texture_field == 'hashgrid'
    y.write_text("guide:\n  texture_field: grid\n")
    with pytest.raises(ValueError, match="texture_field"):
        CFG.parse(argv=[f'--config_path={y}'])


def test_committed_yamls_load_with_the_mlp():
    from contexture_nerf_amd import config as CFG
    paths = sorted(glob.glob(os.path.join(ROOT, "configs", "**", "*.yaml"), recursive=True))
    assert len(paths) == 12
    loaded = 0
    for p in paths:
        if os.path.basename(p) in ("beachball.yaml", "mickey.yaml"):           # refused for a key GuideConfig never had, as before
            with pytest.raises(KeyError, match="guidance_scale_crossattn"):
                CFG.parse(argv=[f'--config_path={p}'])
            continue
        assert CFG.parse(argv=[f'--config_path={p}']).guide.texture_field == 'mlp'
        loaded += 1
    assert loaded == 10


# ---- 5. host refusals ----------------------------------------------------------------------------------------------------------------
def test_host_refusals_need_no_device():
    from contexture_nerf_amd import _lib as L, hashgrid
    hashgrid.HashGridEncoding2D(n_levels=16, n_features=4, log2_table=8, base_res=2, max_res=8)      # 64 columns: the widest there is
    for kw, msg in ((dict(n_levels=17, n_features=4, log2_table=4), "n_levels"), (dict(n_features=3, log2_table=4), "1, 2 or 4"),
                    (dict(log2_table=3), r"outside \[4, 22\]"), (dict(log2_table=23), r"outside \[4, 22\]"),
                    (dict(log2_table=4, base_res=0), "base_res"), (dict(log2_table=4, base_res=32, max_res=16), "base_res"),
                    (dict(log2_table=4, n_levels=2.0), "want an int")):
        with pytest.raises(L.CtxError, match=msg):
            hashgrid.HashGridEncoding2D(**kw)
    enc = hashgrid.HashGridEncoding2D(n_levels=2, log2_table=4)
    assert enc.table.shape == (2, 16, 2) and 0 < enc.table.abs().max().item() <= 1e-4
    assert np.array_equal(enc.res, HT.resolutions(2, 16, 1024))
    with pytest.raises(L.CtxError, match="device tensor"):
        enc(torch.zeros(5, 2))                                          # a host tensor: there is no CPU fallback
    with pytest.raises(L.CtxError, match="device tensor"):
        enc.forward_texels(8)
    with pytest.raises(L.CtxError, match="no gradient with respect to uv"):
        enc(torch.zeros(5, 2, requires_grad=True))
    with pytest.raises(L.CtxError, match=r"uv \[\.\.\., 2\]"):
        enc(torch.zeros(5, 3))
    with pytest.raises(L.CtxError, match="res="):
        enc.forward_texels(1)
    tex = hashgrid.HashGridTexture(n_levels=2, log2_table=4, max_res=32)
    assert tex.mlp.input_ch == 4 and tex.mlp.skips == [0] and len(list(tex.parameters())) == 7
    with pytest.raises(L.CtxError, match="D=1"):
        hashgrid.HashGridTexture(n_levels=2, log2_table=4, D=1)
    for bad in (torch.zeros(4, dtype=torch.int32), torch.zeros(4), [0, 1]):      # a list is a 1-D int32 device tensor
        with pytest.raises(L.CtxError):
            tex.texture_map(8, texels=bad)


# ---- 6. the fit the GPU test repeats ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fit_history():
    return tuple(HT.fit_restatement())


def test_fit_schedule_converges_on_the_restatement():
    """The schedule of HT.FIT (instant-ngp's rates: Adam at 1e-2 on the table and 1e-3 on the MLP, 60 iterations, mean squared error on
    the 32 x 32 checker-plus-ramp) is chosen here: on the float64 restatement the mean loss of the last five iterations is at most 0.05
    of the mean of the first five."""
    c = HT.FIT
    res = HT.resolutions(c['Lv'], c['base_res'], c['max_res'])
    assert res[0] == 2 and res[-1] in (31, 32)                 # floor() of exp() in float64 may land one below, as in 3-D
    dense = [HT.is_dense(r, c['log2T']) for r in res]
    assert any(dense) and not all(dense)
    tgt = HT.fit_target(c['grid'])
    assert tgt.shape == (3, 32, 32) and tgt.min() >= 0.1 - 1e-6 and tgt.max() <= 0.9 + 1e-6
    h = fit_history()
    first, last = float(np.mean(h[:5])), float(np.mean(h[-5:]))
    print(f"fit on the CPU restatement: first five {first:.5f}, last five {last:.6f}, ratio {last / first:.4f}")
    assert len(h) == c['iters'] == 60 and all(np.isfinite(h)) and last <= 0.05 * first
