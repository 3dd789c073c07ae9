"""CPU: the distortion rule (tests/distortion_rule.py).  The binary32 prefix form the HIP kernels implement, restated
sequentially in numpy, stays inside the derived error bounds of the float64 pairwise definition with |.|, and its closed-form gradient
inside those of float64 autograd of that definition; the rule's properties; the host entry's refusals."""
import inspect
import numpy as np
import pytest
import torch

import distortion_rule as dr

f32 = np.float32


@pytest.fixture(scope="module")
def cases():
    """One case per |d|, with its float64 oracle: computed once, shared, left unchanged."""
    out = {}
    for k, norm in enumerate(dr.NORMS):
        case = dr.make_case(dr.COUNTS, seed=40 + k, norm=norm)
        g_loss = np.random.default_rng(50 + k).standard_normal(len(dr.COUNTS)).astype(f32)
        out[norm] = (case, g_loss, dr.oracle64(*case, g_loss))
    return out


def test_the_cases_are_the_stated_ones():
    assert set(dr.COUNTS) == {0, 1, 2, 63, 64, 65, 130, 5000} and dr.COUNTS[0] == 0 and dr.COUNTS[-1] == 0
    k = dr.COUNTS.index(5000)
    assert dr.COUNTS[k - 1] == 1 and dr.COUNTS[k + 1] == 1
    w, t, dt, d, ray_off = dr.make_case(dr.COUNTS, seed=40, norm=3.0)
    assert w.dtype == f32 and 0 <= w.min() and w.max() < 1 and 0.5 <= t.min() and t.max() <= 4 and 0 < dt.min() and dt.max() <= 0.1011
    assert np.allclose(np.linalg.norm(d.astype(np.float64), axis=-1), 3.0, rtol=1e-6)
    a, b = ray_off[k], ray_off[k + 1]
    assert (np.diff(t[a:b]) == 0).sum() >= 900 and (np.diff(t[a:b]) > 0).sum() >= 3000               # ties and strict steps


@pytest.mark.parametrize("norm", dr.NORMS)
def test_binary32_rule_stays_inside_the_bounds(cases, norm):
    case, g_loss, want = cases[norm]
    loss, grad = dr.distortion_np(*case, g_loss)
    assert loss.dtype == f32 and grad.dtype == f32
    rf, rg = dr.check(loss, grad, *case, g_loss, want=want)
    print(f"|d| = {norm}: largest error / bound, forward {rf:.3f}, gradient {rg:.3f}")
    assert np.all(loss >= 0) and np.all(want[0] >= 0)
    ray_off = case[4]
    empty = np.diff(ray_off) == 0
    assert np.all(loss[empty] == 0)
    if norm == 0.0:
        assert np.all(loss == 0) and np.all(grad == 0)
    else:
        assert np.all(want[0][~empty] > 0)
    # a single-sample ray: L = w^2 delta / 3
    w, t, dt, d, _ = case
    fb, _ = dr.bounds(*case)
    nrm = np.linalg.norm(d.astype(np.float64), axis=-1)
    for r in np.nonzero(np.diff(ray_off) == 1)[0]:
        i = ray_off[r]
        assert abs(float(loss[r]) - float(w[i]) ** 2 * float(dt[i]) * nrm[r] / 3) <= fb[r]


def test_gradient_without_upstream_is_the_plain_derivative(cases):
    case = cases[1.0][0]
    loss, grad = dr.distortion_np(*case)
    dr.check(loss, grad, *case)


def test_shift_and_scale_invariance():
    w, t, dt, d, ray_off = dr.make_case(dr.COUNTS, seed=60, norm=1.0, quantised=True)
    loss, grad = dr.distortion_np(w, t, dt, d, ray_off)
    fb, gb = dr.bounds(w, t, dt, d, ray_off)
    # t -> t + c: exact on these inputs, so the centred differences keep their bits
    ts = t + f32(4)
    assert np.array_equal(ts.astype(np.float64), t.astype(np.float64) + 4)
    loss_s, grad_s = dr.distortion_np(w, ts, dt, d, ray_off)
    assert np.all(np.abs(loss_s.astype(np.float64) - loss) <= fb) and np.all(np.abs(grad_s.astype(np.float64) - grad) <= gb)
    # world lengths: |d| = 3 on (t, dt) is |d| = 1 on (3t, 3dt), and three times |d| = 1 on (t, dt): the scalings are exact on these inputs
    t3, dt3, d3 = t * f32(3), dt * f32(3), d * f32(3)
    for a, b in ((t3, t), (dt3, dt), (d3, d)):
        assert np.array_equal(a.astype(np.float64), b.astype(np.float64) * 3)
    loss_a, grad_a = dr.distortion_np(w, t, dt, d3, ray_off)
    loss_b, grad_b = dr.distortion_np(w, t3, dt3, d, ray_off)
    fb3, gb3 = dr.bounds(w, t, dt, d3, ray_off)
    assert np.allclose(fb3, 3 * fb, rtol=1e-12)
    assert np.all(np.abs(loss_a.astype(np.float64) - loss_b) <= fb3) and np.all(np.abs(grad_a.astype(np.float64) - grad_b) <= gb3)
    assert np.all(np.abs(loss_a.astype(np.float64) - 3 * loss.astype(np.float64)) <= fb3)


def test_rectangular_layout_against_the_oracle():
    for R, S in ((1, 1), (3, 64), (4, 65), (2, 200)):
        _, packed = dr.make_rect_case(R, S, seed=R * 100 + S)
        assert np.all(packed[2].reshape(R, S)[:, -1] == 0)                       # the unbounded last interval has no width
        dr.check(*dr.distortion_np(*packed), *packed)


def test_a_nan_weight_poisons_its_own_ray_only():
    case = list(dr.make_case([3, 70, 0, 5], seed=7))
    clean = dr.distortion_np(*case)
    case[0] = case[0].copy()
    case[0][3 + 40] = np.nan
    loss, grad = dr.distortion_np(*case)
    assert np.isnan(loss[1]) and np.all(np.isnan(grad[3:73]))
    assert np.array_equal(loss[[0, 2, 3]], clean[0][[0, 2, 3]]) and np.array_equal(grad[:3], clean[1][:3]) and np.array_equal(grad[73:], clean[1][73:])


def test_host_entry_refuses_what_it_cannot_do():
    from contexture_nerf_amd import _lib as L, run_nerf_helpers as rnh, volume_render as vr
    assert "ctx_distortion_packed_fwd" in L.SIGNATURES and "ctx_distortion_packed_bwd" in L.SIGNATURES
    w, t, dt, d, ray_off = (torch.from_numpy(a) for a in dr.make_case([3, 0, 5], seed=1))
    with pytest.raises(L.CtxError, match="device tensor"):                           # no CPU fallback
        rnh.distortion_loss(w, t, dt, d, ray_off)
    for k in (1, 2, 3):
        args = [w, t, dt, d]
        args[k] = args[k].clone().requires_grad_(True)
        with pytest.raises(L.CtxError, match="no gradient with respect to t / dt / rays_d"):
            rnh.distortion_loss(*args, ray_off)
    with pytest.raises(L.CtxError, match=r"want weights \[n\]"):
        rnh.distortion_loss(w, t[:-1], dt, d, ray_off)
    with pytest.raises(L.CtxError, match=r"without ray_off want weights \[R,S\]"):
        rnh.distortion_loss(w, t, None, d)
    for fn in (vr.train_step, vr.fit_views):
        assert inspect.signature(fn).parameters['distortion'].default == 0.
    with pytest.raises(L.CtxError, match="want a weight >= 0"):
        vr.train_step(None, None, d, d, d, 0.5, 2.5, 8, distortion=-1.)
