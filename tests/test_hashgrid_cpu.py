"""CPU: the hash-grid rule (tests/hashgrid_rule.py) against float64 - the interpolation, its continuity and node values,
the dense and hashed indices, the integer accumulator of the table's gradient, and the restated gradient of the MLP's input."""
import math
import numpy as np
import pytest
import torch

import hashgrid_rule as HG

f32 = np.float32
LO, HI = HG.BOX_LO, HG.BOX_HI


def _positive_table(Lv, F, log2T, seed):
    """values of order 1 and of one sign: every output is then of order 1 too, and a relative bound means something"""
    return (0.5 + np.random.default_rng(seed).random((Lv, 1 << log2T, F))).astype(f32)


@pytest.mark.parametrize("Lv,F,log2T", HG.GRID_CASES)
@pytest.mark.parametrize("max_res", [64, 512])
def test_forward_vs_float64(Lv, F, log2T, max_res):
    res = HG.resolutions(Lv, 2, max_res)
    pts = HG.case_points(300, LO, HI, res, seed=Lv)
    table = _positive_table(Lv, F, log2T, seed=F)
    got = HG.forward_np(pts, table, LO, HI, res, log2T)
    want = HG.forward_f64(pts, table, LO, HI, res, log2T)
    assert got.dtype == f32 and got.shape == (300, Lv * F) and np.all(np.isfinite(got))
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-9)


def test_resolutions():
    r = HG.resolutions(16, 16, 2048)
    assert r[0] == 16 and r[-1] in (2047, 2048) and np.all(np.diff(r) > 0) and r.dtype == np.int32
    assert HG.resolutions(1, 7, 99).tolist() == [7]
    r = HG.resolutions(4, 2, 16).tolist()                     # 2 * 2^l up to the rounding of exp(): floor may land one below
    assert r[0] == 2 and all(v in (2 << l, (2 << l) - 1) for l, v in enumerate(r))
    from contexture_nerf_amd import hashgrid
    for args in ((16, 16, 2048), (1, 7, 99), (4, 2, 64), (16, 2, 512)):
        assert np.array_equal(hashgrid.level_resolutions(*args), HG.resolutions(*args))


@pytest.mark.parametrize("log2T", [6, 12])
def test_continuous_across_cell_faces(log2T):
    """Two points one ulp apart on either side of a cell face: the values differ by no more than the slope allows, res * ulp(x) *
    (the largest difference between neighbouring entries <= 2 max|t|), plus the rounding of the sums (8 terms, 2^-23 max|t|)."""
    res = np.array([8], np.int32)
    table = HG.case_table(1, 2, log2T, seed=3)
    lo, hi = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    rng = np.random.default_rng(0)
    for k in range(1, 8):
        face = f32(k / 8)
        a = rng.random((50, 3)).astype(f32)
        b = a.copy()
        a[:, 0], b[:, 0] = np.nextafter(face, f32(0)), face
        ea, eb = (HG.forward_np(p, table, lo, hi, res, log2T) for p in (a, b))
        ia, _ = HG.positions_np(a, lo, hi, 8)
        ib, _ = HG.positions_np(b, lo, hi, 8)
        assert np.all(ia[:, 0] == k - 1) and np.all(ib[:, 0] == k)             # really on either side
        tmax = float(np.abs(table).max())
        bound = 8 * float(np.spacing(face)) * 2 * tmax + 8 * 2.0 ** -23 * tmax
        assert np.abs(ea - eb).max() <= bound, (k, np.abs(ea - eb).max(), bound)


@pytest.mark.parametrize("Lv,F,log2T", [(1, 1, 4), (4, 2, 12), (3, 4, 6)])
def test_node_returns_its_entry(Lv, F, log2T):
    """A point on a node (unit box, power-of-two resolutions: positions are exact) returns that node's entry exactly."""
    res = np.array([2, 4, 8, 16][:Lv], np.int32)
    table = HG.case_table(Lv, F, log2T, seed=1)
    lo, hi = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    rng = np.random.default_rng(2)
    for l in range(Lv):
        r = int(res[l])
        g = rng.integers(0, r + 1, (40, 3))
        g[0], g[1] = (0, 0, 0), (r, r, r)
        emb = HG.forward_np((g / r).astype(f32), table, lo, hi, res, log2T)
        if HG.is_dense(r, log2T):
            k = g[:, 0] + (r + 1) * (g[:, 1] + (r + 1) * g[:, 2])
        else:
            k = HG.hash_index(g[:, 0], g[:, 1], g[:, 2], log2T).astype(np.int64)
        assert np.array_equal(emb[:, l * F:(l + 1) * F], table[l, k])


def test_dense_levels_index_injectively():
    for res, log2T in ((1, 4), (2, 6), (3, 6), (15, 12), (7, 10)):
        assert HG.is_dense(res, log2T)
        g = np.stack(np.meshgrid(*[np.arange(res)] * 3, indexing='ij'), -1).reshape(-1, 3)
        pts = ((g + 0.5) / res).astype(f32)
        idx, _ = HG.cell_np(pts, (0, 0, 0), (1, 1, 1), res, log2T)
        nodes = {}
        for row, cell in zip(idx, g):
            for c in range(8):
                node = (cell[0] + (c & 1), cell[1] + ((c >> 1) & 1), cell[2] + ((c >> 2) & 1))
                assert nodes.setdefault(int(row[c]), node) == node                  # one node per index ...
        assert len(nodes) == (res + 1) ** 3 and max(nodes) < (1 << log2T)           # ... and one index per node
    assert not HG.is_dense(16, 12) and HG.is_dense(15, 12) and not HG.is_dense(2, 4)


def test_hash_by_hand():
    """(1, 0, 0) -> 1.  (0, 1, 0) -> 2654435761, no wrap.  (3, 5, 7): 5 * 2654435761 = 13272178805 wraps (three times 2^32 off) to
    387276917, 7 * 805459861 = 5638219027 wraps (once) to 1343251731, and 3 ^ 387276917 ^ 1343251731 = 1191511397."""
    assert int(HG.hash_index(1, 0, 0, 22)) == 1
    assert int(HG.hash_index(0, 1, 0, 22)) == 2654435761 % (1 << 22) == 3635633
    assert int(HG.hash_index(3, 5, 7, 22)) == 1191511397 % (1 << 22) == 329061
    assert int(HG.hash_index(3, 5, 7, 4)) == 1191511397 % 16 == 5


def test_wild_points_stay_in_range():
    res = HG.resolutions(16, 2, 512)
    bad = np.array([[np.nan, np.nan, np.nan], [np.inf, -np.inf, 0], [-np.inf, np.inf, np.nan], [1e30, -1e30, 3e38], [-5, 7, 0.5],
                    [np.nan, 0.3, np.inf]], f32)
    table = HG.case_table(16, 2, 12, seed=5)
    for l in range(16):
        idx, w = HG.cell_np(bad, LO, HI, int(res[l]), 12)
        assert idx.min() >= 0 and idx.max() < (1 << 12) and np.all(np.isfinite(w)) and w.min() >= 0 and w.max() <= 1
    assert np.all(np.isfinite(HG.forward_np(bad, table, LO, HI, res, 12)))
    # a NaN coordinate reads as lo, +inf as hi
    ref = np.array([[LO[0], LO[1], LO[2]], [HI[0], LO[1], 0]], f32)
    assert np.array_equal(HG.forward_np(bad[:2], table, LO, HI, res, 12), HG.forward_np(ref, table, LO, HI, res, 12))


def _few_bits(x, bits):
    """x rounded to `bits` bits of mantissa"""
    m, e = np.frexp(np.asarray(x, np.float64))
    return np.ldexp(np.rint(np.ldexp(m, bits)), e - bits).astype(f32)


@pytest.mark.parametrize("Lv,F,log2T", [(4, 2, 6), (4, 4, 10), (1, 1, 4)])
@pytest.mark.parametrize("scale", [1.0, 1e-30, 1e20])
def test_integer_backward_vs_float64_autograd(Lv, F, log2T, scale):
    """The integer backward against float64 autograd of the float64 forward, to 2^-40 of max|g_table|, at three scales of g_emb.
    Two roundings of the rule are not the accumulator's and are 2^-24 each, far above 2^-40: the float32 product w_c * g of every term,
    and the final cast of g_table to float32.  So the accumulator is compared before that cast (as_double), on inputs whose products
    are exact in float32: the unit box with resolutions 2, 4, 8, 16 and coordinates k / 64 give corner weights of at most 15 bits,
    and g_emb is rounded to 9 bits of mantissa.  Then float64 autograd and the integers must agree to the accumulator's own error,
    and the float32 result is the correct rounding of that.  test_integer_accumulator_to_2_pow_minus_40 covers arbitrary inputs."""
    n = 300
    lo, hi = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    res = np.array([2, 4, 8, 16][:Lv], np.int32)
    rng = np.random.default_rng(11)
    pts = (rng.integers(0, 65, (n, 3)) / 64).astype(f32)
    g_emb = _few_bits(rng.standard_normal((n, Lv * F)) * scale, 9)
    assert np.all(np.isfinite(g_emb)) and np.abs(g_emb).max() > 0
    got = HG.backward_np(pts, g_emb, lo, hi, res, log2T, F, as_double=True)
    table = torch.zeros(Lv, 1 << log2T, F, dtype=torch.float64, requires_grad=True)
    (HG.forward_torch(pts, table, lo, hi, res, log2T) * torch.from_numpy(g_emb.astype(np.float64))).sum().backward()
    want = table.grad.numpy()
    m = np.abs(want).max()
    assert m > 0 and np.abs(got - want).max() <= 2.0 ** -40 * m
    assert np.array_equal(HG.backward_np(pts, g_emb, lo, hi, res, log2T, F), got.astype(f32))


def test_integer_accumulator_to_2_pow_minus_40():
    """Arbitrary inputs: the integer sum times 2^(x-E), before the final float32 rounding, against the float64 sum of the same float32
    products (the rule's one rounding per term), to 2^-40 of max|g_table|; the same relative accuracy at 1e-30 and 1e+20.  Each term is
    rounded to a multiple of 2^(x-E) with E = 62 - 12 = 50 here, so 8 n = 2400 terms stay below 2^(x-39.7) even if every rounding went
    the same way, and max|g_table| is above 2^(x-1)."""
    n, Lv, F, log2T = 300, 4, 2, 6
    res = HG.resolutions(Lv, 2, 64)
    pts = HG.case_points(n, LO, HI, res, seed=12)
    for scale in (1.0, 1e-30, 1e20):
        g_emb = (np.random.default_rng(5).standard_normal((n, Lv * F)) * scale).astype(f32)
        x = math.frexp(float(np.abs(g_emb).max()))[1]
        E = 62 - HG.ceil_log2_8n(n)
        acc = np.zeros((Lv, 1 << log2T, F), np.int64)
        want = np.zeros(acc.shape)
        for l in range(Lv):
            idx, w = HG.cell_np(pts, LO, HI, int(res[l]), log2T)
            for c in range(8):
                prod = (w[:, c:c + 1] * g_emb[:, l * F:(l + 1) * F]).astype(np.float64)
                q = np.rint(np.ldexp(prod, E - x)).astype(np.int64)
                assert np.abs(q).max() <= 2 ** E
                for f in range(F):
                    np.add.at(acc[l, :, f], idx[:, c], q[:, f])
                    np.add.at(want[l, :, f], idx[:, c], prod[:, f])
        got = np.ldexp(acc.astype(np.float64), x - E)
        assert np.abs(got - want).max() <= 2.0 ** -40 * np.abs(want).max(), scale
        assert np.array_equal(got.astype(f32), HG.backward_np(pts, g_emb, LO, HI, res, log2T, F))


def test_backward_zero_nan_and_order():
    n, Lv, F, log2T = 65, 4, 2, 6
    res = HG.resolutions(Lv, 2, 64)
    pts = HG.case_points(n, LO, HI, res, seed=13)
    g = np.random.default_rng(6).standard_normal((n, Lv * F)).astype(f32)
    z = HG.backward_np(pts, np.zeros_like(g), LO, HI, res, log2T, F)
    assert z.shape == (Lv, 1 << log2T, F) and not z.any()
    for bad in (np.nan, np.inf, -np.inf):
        gb = g.copy()
        gb[17, 3] = bad
        assert np.all(np.isnan(HG.backward_np(pts, gb, LO, HI, res, log2T, F)))
    perm = np.random.default_rng(7).permutation(n)                      # the order of the points does not matter
    assert np.array_equal(HG.backward_np(pts, g, LO, HI, res, log2T, F), HG.backward_np(pts[perm], g[perm], LO, HI, res, log2T, F))


@pytest.mark.parametrize("D,W,input_ch,skip", [(2, 64, 32, 0), (3, 128, 64, 1), (8, 64, 63, 4)])
def test_grad_emb_formula_vs_autograd(D, W, input_ch, skip):
    N = 37
    params = HG.make_params(D, W, input_ch, 4, skip, seed=D, dtype=torch.float64)
    g = torch.Generator().manual_seed(1)
    emb = torch.randn(N, input_ch, generator=g, dtype=torch.float64).requires_grad_(True)
    g_raw = torch.randn(N, 4, generator=g, dtype=torch.float64)
    (HG.mlp_torch(emb, params, skip) * g_raw).sum().backward()
    dz = HG.mlp_dz_torch(emb.detach(), [p.clone().requires_grad_(True) for p in params], skip, g_raw)
    got = HG.grad_emb_formula(dz, params, skip, input_ch)
    assert (got - emb.grad).abs().max().item() <= 1e-12 * emb.grad.abs().max().item()


def test_host_refusals_need_no_device():
    from contexture_nerf_amd import _lib as L, hashgrid
    hashgrid.HashGridEncoding(LO, HI, n_levels=16, n_features=4, log2_table=8, base_res=2, max_res=8)   # 64 columns: the widest there is
    # n_levels * n_features > 64 needs more than 16 levels: it is the level count that is refused
    for kw, msg in ((dict(n_levels=17, n_features=4, log2_table=4), "n_levels"), (dict(n_features=3, log2_table=4), "1, 2 or 4"),
                    (dict(log2_table=3), r"outside \[4, 22\]"), (dict(log2_table=23), r"outside \[4, 22\]"),
                    (dict(n_levels=17, n_features=1, log2_table=4), "n_levels"), (dict(log2_table=4, base_res=0), "base_res")):
        with pytest.raises(L.CtxError, match=msg):
            hashgrid.HashGridEncoding(LO, HI, **kw)
    for lo, hi in (((0, 0, 0), (1, 0, 1)), (1.0, 1.0), ((0, 0, 0), (1, np.inf, 1)), ((np.nan, 0, 0), (1, 1, 1))):
        with pytest.raises(L.CtxError, match="finite lo < hi"):
            hashgrid.HashGridEncoding(lo, hi, n_levels=2, log2_table=4)
    enc = hashgrid.HashGridEncoding(LO, HI, n_levels=2, log2_table=4)
    assert enc.table.shape == (2, 16, 2) and enc.table.abs().max().item() <= 1e-4 and enc.table.abs().max().item() > 0
    with pytest.raises(L.CtxError, match="device tensor"):
        enc(torch.zeros(5, 3))                                          # a host tensor: there is no CPU fallback
