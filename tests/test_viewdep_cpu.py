"""CPU: the rule of the view-dependent field's glue (tests/sh_rule.py) checked against itself: the constants by
orthonormality on a quadrature of the sphere, the float32 rule against its float64 twin at a bound derived from the roundings, the row
properties, and the row rules on hand cases."""
import numpy as np
import pytest

import sh_rule as SH

f32 = np.float32


def test_orthonormality_pins_the_constants():
    """Real spherical harmonics are orthonormal on the sphere.  Degree 4 squared is a polynomial of degree 6: Gauss-Legendre (16) in
    cos(theta) and 32 uniform steps in phi integrate it exactly, so Y^T W Y = I to rounding.  A wrong constant or sign breaks it."""
    d, w = SH.sphere_quadrature(16, 32)
    assert abs(w.sum() - 4 * np.pi) < 1e-12
    Y = SH.sh_f64(d, 4)
    gram = Y.T @ (w[:, None] * Y)
    err = np.abs(gram - np.eye(16)).max()
    print(f"|Y^T W Y - I| max = {err:.2e}")
    assert err <= 1e-12


def test_float32_rule_against_its_twin():
    """|f32 - f64| <= 16 * 2^-24 * A per element, A the polynomial with every monomial in absolute value.  The 16: a normalised component
    carries about 2.5 units of 2^-24 (the three roundings of the sum of squares halved by the square root, the root, the division); a cubic
    monomial triples that and adds its own products and the constant's rounding, about 12 in all."""
    d = SH.mixed_directions(200001, seed=7)
    assert not d[-1].any()
    lengths = np.linalg.norm(d[:-1].astype(np.float64), axis=1)
    assert lengths.min() < 2e-3 and lengths.max() > 25
    got = SH.sh_np(d, 4).astype(np.float64)
    want, A = SH.sh_scale(d, 4)
    units = np.divide(np.abs(got - want), A * 2.0 ** -24, out=np.zeros_like(A), where=A > 0)
    print("worst error per column, in units of 2^-24 A:", np.round(units.max(0), 2).tolist())
    assert (np.abs(got - want) <= 16 * 2.0 ** -24 * A).all()


def test_row_properties():
    d = SH.mixed_directions(500, seed=3)
    full = SH.sh_np(d, 4)
    for deg in (1, 2, 3):
        assert np.array_equal(SH.sh_np(d, deg), full[:, :deg * deg])
        assert np.array_equal(SH.sh_f64(d, deg), SH.sh_f64(d, 4)[:, :deg * deg])
    zero = SH.sh_np(np.zeros((1, 3), f32), 4)[0]
    want = np.zeros(16, f32)
    want[0], want[6] = f32(SH.C0), f32(0) - f32(SH.C3B)
    assert np.array_equal(zero, want)
    assert np.array_equal(full[-1], want)                                     # mixed_directions ends with the zero direction
    # an out-of-range ray_id reads nothing and gives that same row, behind the untouched features
    emb = np.arange(12, dtype=f32).reshape(4, 3)
    rays_d = d[:2]
    inp = SH.input_np(emb, rays_d, np.int32([0, -1, 2, 1]), 4)
    assert inp.shape == (4, 19) and inp.dtype == f32
    assert np.array_equal(inp[:, :3], emb)
    assert np.array_equal(inp[1, 3:], want) and np.array_equal(inp[2, 3:], want)
    assert np.array_equal(inp[0, 3:], full[0]) and np.array_equal(inp[3, 3:], full[1])
    # the direction's length does not matter beyond rounding, its sign does on the odd bands
    a, b = SH.sh_f64(np.float64([[0.3, -0.5, 0.8]]), 4), SH.sh_f64(np.float64([[3.0, -5.0, 8.0]]), 4)
    assert np.allclose(a, b, rtol=0, atol=1e-15)
    m = SH.sh_f64(np.float64([[-0.3, 0.5, -0.8]]), 4)
    odd = np.r_[1:4, 9:16]
    assert np.allclose(m[:, odd], -a[:, odd], atol=1e-15) and np.allclose(np.delete(m, odd, 1), np.delete(a, odd, 1), atol=1e-15)


def test_known_values():
    """Along +z only the zonal harmonics are non-zero: sqrt((2l+1)/(4 pi)) for l = 0 .. 3."""
    y = SH.sh_f64(np.float64([[0, 0, 2.0]]), 4)[0]
    zonal = {0: 0, 2: 1, 6: 2, 12: 3}
    for k in range(16):
        want = np.sqrt((2 * zonal[k] + 1) / (4 * np.pi)) if k in zonal else 0.0
        assert abs(y[k] - want) < 1e-15, (k, y[k], want)


def test_row_rules_on_hand_cases():
    g_inp = np.arange(2 * 7, dtype=f32).reshape(2, 7)
    assert np.array_equal(SH.input_bwd_np(g_inp, 3), f32([[0, 1, 2], [7, 8, 9]]))
    base = f32([[1, 2, 3, 4], [0.1, 0.2, 0.3, -5]])
    res = f32([[10, 20, 30], [1e-9, -0.2, 1]])
    raw = SH.raw_np(base, res)
    assert raw.dtype == f32
    assert np.array_equal(raw, f32([[11, 22, 33, 4], [f32(0.1) + f32(1e-9), f32(0.2) + f32(-0.2), f32(0.3) + f32(1), -5]]))
    assert np.array_equal(raw[:, 3], base[:, 3]) and raw[1, 0] == f32(0.1)       # the add rounds in binary32
    g_raw = f32([[1, 2, 3, 4], [5, 6, 7, 8]])
    assert np.array_equal(SH.raw_bwd_np(g_raw), f32([[1, 2, 3], [5, 6, 7]]))
    assert SH.raw_np(base.astype(np.float64), res.astype(np.float64)).dtype == np.float64


def test_host_refusals_without_a_device():
    """What the constructor refuses by name needs no GPU."""
    from contexture_nerf_amd import _lib as L
    from contexture_nerf_amd.hashgrid import HashGridField, ViewDependentField
    with pytest.raises(L.CtxError, match=r"48 \+ 25|sh_degree"):
        ViewDependentField(-1.0, 1.0, n_levels=12, n_features=4, log2_table=4, sh_degree=5)
    with pytest.raises(L.CtxError, match=r"56 \+ 9 = 65"):
        ViewDependentField(-1.0, 1.0, n_levels=14, n_features=4, log2_table=4, sh_degree=3)
    with pytest.raises(L.CtxError, match="sh_degree"):
        ViewDependentField(-1.0, 1.0, n_levels=2, log2_table=4, sh_degree=0)
    field = ViewDependentField(-1.0, 1.0, n_levels=4, n_features=2, log2_table=4, base_res=2, max_res=8, sh_degree=4)
    assert isinstance(field, HashGridField) and field.view_dependent and field.dir_mlp.input_ch == 8 + 16 and field.dir_mlp.output_ch == 3
    assert not bool(field.dir_mlp.output_linear.weight.any()) and not bool(field.dir_mlp.output_linear.bias.any())
    assert len(list(field.parameters())) == 13
    assert not getattr(HashGridField(-1.0, 1.0, n_levels=2, log2_table=4), 'view_dependent', False)
