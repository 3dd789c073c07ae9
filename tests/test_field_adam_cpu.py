"""CPU: the field optimizer's rule (tests/adam_rule.py, the definition of csrc/adam.hip) against torch.optim.Adam, its sparse and
non-finite cases, FieldAdam's state and refusals, and the refusals of the two ABI entries (which happen before any launch)."""
import ctypes as C
import numpy as np
import pytest
import torch

import adam_rule as AR

f32 = np.float32
BETAS = (0.9, 0.99)
N = 200000
STEPS = 5
CASES = [(1e-2, 1e-8, 3e-3), (1e-2, 1e-15, 3e-3), (1e-5, 1e-15, 1e-6), (5e-4, 1e-8, 1.0)]      # (lr, eps, gradient scale)


def fixed_problem(scale, n=N, steps=STEPS, seed=0):
    """p0 [n] and `steps` fixed gradients [steps, n], float32."""
    rng = np.random.default_rng(seed)
    p0 = rng.standard_normal(n).astype(f32) * f32(0.1)
    grads = (rng.standard_normal((steps, n)) * scale).astype(f32)
    return p0, grads


def torch_adam(p0, grads, lr, eps, dtype, device='cpu', make=torch.optim.Adam):
    p = torch.nn.Parameter(torch.tensor(p0, device=device, dtype=dtype))      # a copy: p0 stays
    opt = make([p], lr=lr, betas=BETAS, eps=eps)
    for g in grads:
        p.grad = torch.tensor(g, device=device, dtype=dtype)
        opt.step()
    return p.detach().double().cpu().numpy()


def rule_adam(p0, grads, lr, eps):
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for t, g in enumerate(grads, 1):
        p, m, v = AR.adam_step(p, m, v, g, lr, BETAS, eps, t)
    return p.astype(np.float64)


def distance(p, p0, want):
    """Relative L2 of the travelled p - p0 against float64 torch."""
    d = want - p0.astype(np.float64)
    return float(np.linalg.norm((p - p0.astype(np.float64)) - d) / np.linalg.norm(d))


@pytest.mark.parametrize("lr,eps,scale", CASES)
def test_rule_is_as_close_to_float64_as_torch_float32(lr, eps, scale):
    """Five steps on fixed gradients: the rule's distance to float64 torch.optim.Adam is at most 2x that of float32 torch.optim.Adam on the
    CPU (both are a handful of roundings in another order; measured 0.86 - 1.00 at one and five steps, 1.35 - 1.56 at fifty)."""
    p0, grads = fixed_problem(scale)
    want = torch_adam(p0, grads, lr, eps, torch.float64)
    d_torch = distance(torch_adam(p0, grads, lr, eps, torch.float32), p0, want)
    d_rule = distance(rule_adam(p0, grads, lr, eps), p0, want)
    print(f"lr={lr} eps={eps} scale={scale}: rule {d_rule:.3e}, torch float32 {d_torch:.3e}, ratio {d_rule / d_torch:.3f}")
    assert d_torch > 0 and d_rule <= 2 * d_torch


def test_sparse_and_non_finite_semantics():
    rng = np.random.default_rng(1)
    n = 1000
    p, m, v = (rng.standard_normal(n).astype(f32) for _ in range(3))
    v = np.abs(v)
    g = rng.standard_normal(n).astype(f32)
    g[::3] = 0.0
    g[3::6] = -0.0
    zero = g == 0
    assert zero.sum() > 300 and np.signbit(g[zero]).any()
    for t in (1, 2, 7):
        p1, m1, v1 = AR.adam_step(p, m, v, g, 1e-2, BETAS, 1e-8, t, sparse=True)
        d1 = AR.adam_step(p, m, v, g, 1e-2, BETAS, 1e-8, t, sparse=False)
        for new, old, dense in zip((p1, m1, v1), (p, m, v), d1):
            assert np.array_equal(AR.bits(new)[zero], AR.bits(old)[zero])                   # kept bit for bit
            assert np.array_equal(AR.bits(new)[~zero], AR.bits(dense)[~zero])               # the rest steps with this t
        assert (p1[~zero] != p[~zero]).all()
    # t advances for the rest: the same gradient at another t moves p differently
    assert not np.array_equal(AR.adam_step(p, m, v, g, 1e-2, BETAS, 1e-8, 1, True)[0], AR.adam_step(p, m, v, g, 1e-2, BETAS, 1e-8, 2, True)[0])
    # dense, g = 0 and v = 0: m' = v' = 0, d = eps, the update is 0 / eps
    z = np.zeros(4, f32)
    for eps in (1e-8, 1e-15):
        p1, m1, v1 = AR.adam_step(p[:4], z, z, z, 1e-2, BETAS, eps, 1)
        assert np.array_equal(AR.bits(p1), AR.bits(p[:4])) and not m1.any() and not v1.any()
    # g = 1e30: v' overflows to inf, d = inf, the update is 0
    big = np.full(4, 1e30, f32)
    p1, m1, v1 = AR.adam_step(p[:4], z, z, big, 1e-2, BETAS, 1e-8, 1, sparse=True)
    assert np.isinf(v1).all() and np.isfinite(m1).all() and np.array_equal(AR.bits(p1), AR.bits(p[:4]))
    # NaN and inf are not zero: they propagate, also under sparse
    for bad in (np.nan, np.inf, -np.inf):
        p1, m1, v1 = AR.adam_step(p[:4], z, z, np.full(4, bad, f32), 1e-2, BETAS, 1e-8, 1, sparse=True)
        assert np.isnan(p1).all()


def test_coefficients_match_the_product():
    from contexture_nerf_amd import optim
    for lr, eps, t in ((1e-2, 1e-8, 1), (1e-5, 1e-15, 1000), (5e-4, 1e-8, 37)):
        got = [C.c_float(x).value for x in optim.coefficients(lr, BETAS, eps, t)]
        assert [float(x) for x in AR.coefficients(lr, BETAS, eps, t)] == got


def test_refusals_without_a_device():
    from contexture_nerf_amd import _lib as L, optim
    p = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(L.CtxError, match="device tensor"):
        optim.FieldAdam([p])
    for key, val in (("weight_decay", 0.1), ("amsgrad", True), ("maximize", True)):
        with pytest.raises(L.CtxError, match=key):
            optim.FieldAdam([dict(params=[torch.nn.Parameter(torch.zeros(1))], **{key: val})])
    with pytest.raises(L.CtxError, match="betas"):
        optim.FieldAdam([torch.nn.Parameter(torch.zeros(1))], betas=(1.0, 0.9))


def test_state_dict_round_trips_through_torch_adam():
    """The layout only, with states written by hand (a step needs the device): FieldAdam -> torch.optim.Adam -> FieldAdam."""
    from contexture_nerf_amd import optim
    ps = [torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(2, 3))]

    class OnHost(optim.FieldAdam):          # the device check is the one thing a CPU test cannot pass
        @staticmethod
        def _check_param(p):
            pass
    groups = lambda: [dict(params=[ps[0]], lr=1e-2, sparse=True), dict(params=[ps[1]], lr=1e-3, eps=1e-15)]
    a = OnHost(groups(), betas=BETAS)
    for p in ps:
        st = a._state(p)
        st['step'] += 3
        st['exp_avg'].copy_(torch.randn_like(p))
        st['exp_avg_sq'].copy_(torch.rand_like(p))
    sd = a.state_dict()
    t = torch.optim.Adam([dict(params=[ps[0]]), dict(params=[ps[1]])])
    t.load_state_dict(sd)
    assert [g['lr'] for g in t.param_groups] == [1e-2, 1e-3] and t.param_groups[1]['eps'] == 1e-15 and t.param_groups[0]['betas'] == BETAS
    for p in ps:
        p.grad = torch.ones_like(p)
    t.step()                                                        # torch accepts the state: step 4
    assert all(float(t.state[p]['step']) == 4 for p in ps)
    b = OnHost(groups(), betas=BETAS)
    b.load_state_dict(t.state_dict())
    assert [g['sparse'] for g in b.param_groups] == [True, False]
    for p in ps:
        assert float(b.state[p]['step']) == 4
        assert torch.equal(b.state[p]['exp_avg'], t.state[p]['exp_avg']) and torch.equal(b.state[p]['exp_avg_sq'], t.state[p]['exp_avg_sq'])
    # and from a torch.optim.Adam that never saw `sparse`
    t2 = torch.optim.Adam([dict(params=[ps[0]]), dict(params=[ps[1]])], betas=BETAS)
    t2.step()
    c = OnHost(groups(), betas=BETAS)
    c.load_state_dict(t2.state_dict())
    assert [g['sparse'] for g in c.param_groups] == [False, False]
    c._check_groups()


def test_abi_refuses_null_pointers_and_bad_counts():
    from contexture_nerf_amd import _lib as L
    lib = L.load()
    buf = (C.c_float * 64)()                                         # never read: every call below is refused before a launch
    a = C.addressof(buf)
    hyper = [float(x) for x in AR.coefficients(1e-2, BETAS, 1e-8, 1)]

    def multi(p, m, v, g, counts, n):
        arr = lambda xs: (C.c_void_p * 17)(*xs)
        return lib.ctx_adam_multi(arr(p), arr(m), arr(v), arr(g), (C.c_int64 * 17)(*counts), n, *hyper, 0, None)
    ok = [a] * 17
    assert multi(ok, ok, ok, ok, [4] * 17, 0) != 0 and b"n_tensors" in lib.ctx_last_error()
    assert multi(ok, ok, ok, ok, [4] * 17, 17) != 0 and b"n_tensors" in lib.ctx_last_error()
    assert multi(ok, ok, ok, ok, [4, 0] + [4] * 15, 2) != 0 and b"count" in lib.ctx_last_error()
    assert multi(ok, ok, ok, ok, [4, -3] + [4] * 15, 2) != 0 and b"count" in lib.ctx_last_error()
    for which in range(4):
        lists = [list(ok) for _ in range(4)]
        lists[which][1] = None
        assert multi(*lists, [4] * 17, 2) != 0 and b"null" in lib.ctx_last_error()
    assert lib.ctx_adam_multi(None, None, None, None, None, 1, *hyper, 0, None) != 0 and b"null" in lib.ctx_last_error()

    def table(p, m, v, count, ws, n, corners):
        return lib.ctx_table_adam(p, m, v, count, ws, n, corners, *hyper, 1, None)
    for args in ((None, a, a, 64, a, 10, 8), (a, None, a, 64, a, 10, 8), (a, a, None, 64, a, 10, 8), (a, a, a, 64, None, 10, 8)):
        assert table(*args) != 0 and b"null" in lib.ctx_last_error()
    for count in (0, -16, 8, 24):
        assert table(a, a, a, count, a, 10, 8) != 0 and b"count" in lib.ctx_last_error()
    for n in (0, -1, 1 << 31):
        assert table(a, a, a, 64, a, n, 8) != 0 and b"n=" in lib.ctx_last_error()
