"""The view-dependent field's glue, restated: the real spherical harmonics of a ray's direction as the direction net's extra input
columns, and the sum of the base and the residual term (csrc/viewdep.hip).  This file is the definition.

The direction d = rays_d[r] is normalised as csrc/ray_wave.h's ray_norm does it: n = sqrtf((d0*d0 + d1*d1) + d2*d2), (x, y, z) = d / n where
n > 0 and (0, 0, 0) where it is not.  The K = deg^2 values, deg in 1..4, are the first K of the sixteen Cartesian polynomials below, every
operation rounding on its own in binary32 in the order written (no contraction); the constants are the float64 values rounded once.
`sh_np` is that rule, `sh_f64` its float64 twin (same inputs, every operation in binary64), `sh_scale` returns the twin together with A, the
same polynomials with every monomial taken in absolute value: the scale a rounding error of the float32 rule is measured in."""
import numpy as np

f32 = np.float32
MAX_DEG, MAX_WIDTH = 4, 64

C0 = 0.28209479177387814
C1 = 0.48860251190291987
C2 = 1.0925484305920792
C3 = 0.94617469575755997
C3B = 0.31539156525251999
C4 = 0.54627421529603959
C5 = 0.59004358992664352
C6 = 2.8906114426405538
C7 = 0.45704579946446572
C8 = 0.3731763325901154
C9 = 1.4453057213202769


def normalise(d, dtype):
    """d [R,3] -> (x, y, z) in dtype: d / |d| with the sum of squares in ray_norm's order, zeros where |d| is not > 0."""
    d = np.asarray(d).reshape(-1, 3).astype(dtype)
    d0, d1, d2 = d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(all='ignore'):
        n = np.sqrt((d0 * d0 + d1 * d1) + d2 * d2)
        ok = n > 0
        safe = np.where(ok, n, dtype(1))
        return [np.where(ok, c / safe, dtype(0)).astype(dtype) for c in (d0, d1, d2)]


def _columns(x, y, z, T, absolute=False):
    """The sixteen columns in the order of operations of the rule, in the type T of x, y, z; absolute: |monomial| everywhere."""
    c = lambda v: T(v)
    one, three, five = T(1), T(3), T(5)
    if absolute:
        x, y, z = np.abs(x), np.abs(y), np.abs(z)
        sub = lambda a, b: a + b
        neg = lambda v: T(v)
    else:
        sub = lambda a, b: a - b
        neg = lambda v: T(-v)
    xx, yy, zz = x * x, y * y, z * z
    cols = [np.full_like(x, c(C0)),
            neg(C1) * y, c(C1) * z, neg(C1) * x,
            c(C2) * (x * y), neg(C2) * (y * z), sub(c(C3) * zz, c(C3B)), neg(C2) * (x * z), c(C4) * sub(xx, yy),
            (c(C5) * y) * sub(yy, three * xx), (c(C6) * (x * y)) * z, (c(C7) * y) * sub(one, five * zz), (c(C8) * z) * sub(five * zz, three),
            (c(C7) * x) * sub(one, five * zz), (c(C9) * z) * sub(xx, yy), (c(C5) * x) * sub(three * yy, xx)]
    return np.stack(cols, 1)


def sh_np(d, deg):
    """The rule: d [R,3] float32 -> float32 [R, deg^2]."""
    assert 1 <= deg <= MAX_DEG
    with np.errstate(all='ignore'):
        out = _columns(*normalise(d, f32), f32)[:, :deg * deg]
    assert out.dtype == f32
    return out


def sh_f64(d, deg):
    """The twin: the same float32 directions, every operation in binary64 -> float64 [R, deg^2]."""
    assert 1 <= deg <= MAX_DEG
    with np.errstate(all='ignore'):
        return _columns(*normalise(d, np.float64), np.float64)[:, :deg * deg]


def sh_scale(d, deg):
    """-> (Y, A) float64 [R, deg^2]: the twin, and the same polynomials with every monomial in absolute value."""
    with np.errstate(all='ignore'):
        xyz = normalise(d, np.float64)
        return _columns(*xyz, np.float64)[:, :deg * deg], _columns(*xyz, np.float64, absolute=True)[:, :deg * deg]


def directions_of(rays_d, ray_id):
    """rays_d [R,3], ray_id int [n] -> float32 [n,3]: the listed rays' directions, (0,0,0) for an entry outside [0, R)."""
    rays_d = np.asarray(rays_d, f32).reshape(-1, 3)
    ray_id = np.asarray(ray_id).astype(np.int64)
    ok = (ray_id >= 0) & (ray_id < rays_d.shape[0])
    d = np.zeros((ray_id.shape[0], 3), f32)
    d[ok] = rays_d[ray_id[ok]]
    return d


def input_np(emb, rays_d, ray_id, deg, sh=sh_np):
    """inp [n, E + K] = [ emb[i] | SH(rays_d[ray_id[i]]) ]; an entry of ray_id outside [0, R) reads nothing and takes (0,0,0)."""
    emb = np.asarray(emb)
    y = sh(directions_of(rays_d, ray_id), deg)
    return np.concatenate([emb.astype(y.dtype), y], 1)


def input_bwd_np(g_inp, E):
    """g_emb [n, E] = g_inp[:, :E]."""
    return np.ascontiguousarray(np.asarray(g_inp)[:, :E])


def raw_np(base, res):
    """raw [n,4]: the colour channels base + res (one add each, in the arrays' type), the density base[:, 3]."""
    base, res = np.asarray(base), np.asarray(res)
    raw = base.copy()
    raw[:, :3] = base[:, :3] + res
    return raw


def raw_bwd_np(g_raw):
    """g_res [n,3] = g_raw[:, :3]; the gradient to base is g_raw itself."""
    return np.ascontiguousarray(np.asarray(g_raw)[:, :3])


def mixed_directions(n, seed, zero=True):
    """n random directions with lengths mixed over 1e-3, 1, 50 (and with zero, (0,0,0) as the last one) -> float32 [n,3]."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = (d * rng.choice([1e-3, 1.0, 50.0], size=(n, 1)) * rng.uniform(0.5, 2.0, size=(n, 1))).astype(f32)
    if zero:
        d[-1] = 0
    return d


def sphere_quadrature(n_theta=16, n_phi=32):
    """Gauss-Legendre in cos(theta) x uniform in phi -> (d float64 [n,3] unit, w float64 [n]) with sum(w) = 4 pi."""
    u, wu = np.polynomial.legendre.leggauss(n_theta)
    phi = (np.arange(n_phi) + 0.5) * (2 * np.pi / n_phi)
    s = np.sqrt(1 - u * u)
    d = np.stack([np.outer(s, np.cos(phi)), np.outer(s, np.sin(phi)), np.outer(u, np.ones_like(phi))], -1).reshape(-1, 3)
    w = np.outer(wu, np.full(n_phi, 2 * np.pi / n_phi)).reshape(-1)
    return d, w
