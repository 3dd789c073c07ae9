"""The definition of the field optimizer's step (csrc/adam.hip: ctx_adam_multi, ctx_table_adam), in numpy.
Per element, in binary32, every operation rounds once, in this order:

    host, in float64, then rounded to float:  b1, b2, o1 = 1 - b1, o2 = 1 - b2,
            c1 = lr / (1 - b1^t),  c2 = 1 / sqrt(1 - b2^t),  eps          (t = 1, 2, ...: the step count)
    if sparse and g == 0.0f (either sign):  p, m, v keep their bits
    else  m' = b1*m + o1*g ;  v' = b2*v + (o2*g)*g ;  d = sqrtf(v')*c2 + eps ;  p' = p - (c1*m') / d

A NaN or infinite g is not equal to zero: it propagates.  numpy's float32 multiply, add, divide and sqrt are the correctly rounded ones and
keep subnormals."""
import math
import numpy as np

f32 = np.float32


def coefficients(lr, betas, eps, t):
    """-> (b1, b2, o1, o2, c1, c2, eps) as float32, from Python floats (float64) and the step count t >= 1."""
    b1, b2 = float(betas[0]), float(betas[1])
    return (f32(b1), f32(b2), f32(1.0 - b1), f32(1.0 - b2), f32(float(lr) / (1.0 - b1 ** t)), f32(1.0 / math.sqrt(1.0 - b2 ** t)),
            f32(float(eps)))


def adam_step(p, m, v, g, lr, betas, eps, t, sparse=False):
    """One step on float32 arrays of one shape -> (p', m', v'), new arrays."""
    b1, b2, o1, o2, c1, c2, e = coefficients(lr, betas, eps, t)
    p, m, v, g = (np.ascontiguousarray(a, f32) for a in (p, m, v, g))
    with np.errstate(all='ignore'):
        m1 = b1 * m + o1 * g
        v1 = b2 * v + (o2 * g) * g
        d = np.sqrt(v1) * c2 + e
        p1 = p - (c1 * m1) / d
    assert p1.dtype == f32 and m1.dtype == f32 and v1.dtype == f32
    if sparse:
        keep = g == f32(0)
        p1, m1, v1 = np.where(keep, p, p1), np.where(keep, m, m1), np.where(keep, v, v1)
    return p1, m1, v1


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)
