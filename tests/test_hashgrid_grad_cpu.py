"""CPU: the rule of the hash-grid encoding's gradient to the positions (tests/hashgrid_grad_rule.py) against its float64
twin inside the derived bound, against float64 autograd through a differentiable restatement of the forward, on a linear ramp whose
gradient is known in closed form, and under mutations that the bound has to catch; the per-ray weighted sum inside its bound."""
import functools
import numpy as np
import pytest
import torch

import hashgrid_rule as HG
import hashgrid_grad_rule as GR
import distortion_rule as DR

f32 = np.float32
LO, HI = HG.BOX_LO, HG.BOX_HI


@functools.lru_cache(maxsize=None)
def _case(Lv, F, log2T, n):
    res = HG.resolutions(Lv, 2, 64)
    pts = HG.case_points(n, LO, HI, res, seed=n)
    table = HG.case_table(Lv, F, log2T, seed=Lv + F)
    g_emb = np.random.default_rng(n + 7).standard_normal((n, Lv * F)).astype(f32)
    want, mag = GR.grad_pts_f64(pts, table, g_emb, LO, HI, res, log2T)
    return res, pts, table, g_emb, want, mag


@pytest.mark.parametrize("Lv,F,log2T", HG.GRID_CASES)
def test_rule_within_the_bound_of_float64(Lv, F, log2T):
    worst = 0.0
    for n in HG.N_CASES:
        res, pts, table, g_emb, want, mag = _case(Lv, F, log2T, n)
        got = GR.grad_pts_np(pts, table, g_emb, LO, HI, res, log2T)
        assert got.dtype == f32 and got.shape == (n, 3)
        bnd = GR.bound(mag, Lv, F)
        pos = bnd > 0
        err = np.abs(got.astype(np.float64) - want)
        assert np.all(err[pos] <= bnd[pos]), (n, float((err[pos] / bnd[pos]).max()))
        assert np.all(err[~pos] == 0)
        if pos.any():
            worst = max(worst, float((err[pos] / bnd[pos]).max()))
        # exact zeros on every inactive axis (faces, outside, NaN, inf), finite everywhere: the inputs (table, g_emb) are
        off = ~GR.active_np(pts, LO, HI)
        assert np.all(got[off] == 0) and not np.any(np.signbit(got[off]))
        assert np.all(np.isfinite(got))
    print(f"hashgrid grad rule Lv={Lv} F={F} log2T={log2T}: worst binary32 error / bound {worst:.3f}")
    assert worst > 0


def test_inactive_axes_are_zero_whatever_the_inputs_hold():
    """NaN / inf in g_emb and in the table reach the active axes only."""
    Lv, F, log2T = 4, 2, 6
    res, pts, table, g_emb, _, _ = _case(Lv, F, log2T, 65)
    table, g_emb = np.full_like(table, np.nan), np.full_like(g_emb, np.inf)
    got = GR.grad_pts_np(pts, table, g_emb, LO, HI, res, log2T)
    act = GR.active_np(pts, LO, HI)
    assert act.any() and (~act).any()
    assert np.all(got[~act] == 0) and np.all(np.isnan(got[act]))
    special = pts[1:20:2]                                   # the rows case_points overwrites: corners, faces, outside, NaN, inf
    assert np.isnan(special).any() and np.isinf(special).any()


@pytest.mark.parametrize("Lv,F,log2T", HG.GRID_CASES)
def test_float64_twin_vs_autograd(Lv, F, log2T):
    """The formula against float64 autograd through clamp and the trilinear weights (cell detached): 1e-4 of the largest component on the
    strictly-inside axes (what is left is the binary32 rounding of the positions the twin starts from), and 0 = 0 strictly outside."""
    worst = 0.0
    for n in HG.N_CASES:
        res, pts, table, g_emb, want, _ = _case(Lv, F, log2T, n)
        rows = np.isfinite(pts).all(1)
        if not rows.any():
            continue
        p = torch.from_numpy(pts[rows].astype(np.float64)).requires_grad_(True)
        emb = GR.forward_torch_pts(p, torch.from_numpy(table.astype(np.float64)), LO, HI, res, log2T)
        (emb * torch.from_numpy(g_emb[rows].astype(np.float64))).sum().backward()
        auto = p.grad.numpy()
        inside, outside = GR.active_np(pts[rows], LO, HI), GR.outside_np(pts[rows], LO, HI)
        assert np.all(auto[outside] == 0) and np.all(want[rows][outside] == 0)
        if inside.any():
            rel = np.abs(want[rows][inside] - auto[inside]).max() / np.abs(auto[inside]).max()
            worst = max(worst, float(rel))
            assert rel <= 1e-4, (n, rel)
    print(f"hashgrid grad twin vs float64 autograd Lv={Lv} F={F} log2T={log2T}: worst {worst:.3e} of the largest component")


@pytest.mark.parametrize("lo,hi", [(LO, HI), (-1.0, 1.0)])
def test_linear_ramp_pins_the_scale(lo, hi):
    """One dense level, F = 1, entry = a * (gx + gy + gz) / res: emb = a * (x + y + z) in box coordinates, so d emb / d p = a / (hi - lo) on
    every axis, whatever the cell."""
    a, r, log2T = 3.0, 8, 10
    assert HG.is_dense(r, log2T)
    lo3, hi3 = np.broadcast_to(np.asarray(lo, f32), (3,)), np.broadcast_to(np.asarray(hi, f32), (3,))
    res = np.array([r], np.int32)
    table = np.zeros((1, 1 << log2T, 1), f32)
    g = np.arange(r + 1)
    node = g[None, None, :] + g[None, :, None] + g[:, None, None]                # [gz, gy, gx]
    table[0, :(r + 1) ** 3, 0] = (a * node / r).reshape(-1)                        # idx = gx + side * (gy + side * gz)
    rng = np.random.default_rng(0)
    pts = (lo3 + (0.01 + 0.98 * rng.random((200, 3))) * (hi3 - lo3)).astype(f32)
    g_emb = np.ones((200, 1), f32)
    got = GR.grad_pts_np(pts, table, g_emb, lo3, hi3, res, log2T)
    _, mag = GR.grad_pts_f64(pts, table, g_emb, lo3, hi3, res, log2T)
    want = np.broadcast_to(a / (hi3.astype(np.float64) - lo3), (200, 3))
    assert np.all(np.abs(got - want) <= GR.bound(mag, 1, 1))
    assert np.all(got > 0)


@pytest.mark.parametrize("mutate", GR.MUTATIONS)
def test_mutations_leave_the_bound(mutate):
    """The bound can fail: a wrong axis pair, a dropped sign, a scale without res and a wrong column stride each leave it on some case."""
    caught = 0
    for Lv, F, log2T in HG.GRID_CASES:
        for n in HG.N_CASES:
            res, pts, table, g_emb, want, mag = _case(Lv, F, log2T, n)
            got = GR.grad_pts_np(pts, table, g_emb, LO, HI, res, log2T, mutate=mutate)
            bnd = GR.bound(mag, Lv, F)
            caught += bool(np.any(np.abs(got - want) > bnd))
    assert caught >= 1, mutate


@pytest.mark.parametrize("C", [1, 3, 4])
def test_weighted_sum_within_the_bound_of_float64(C):
    w, v, ray_off = GR.weighted_sum_case(DR.COUNTS, C, seed=C)
    got = GR.weighted_sum_np(w, v, ray_off)
    want, bnd = GR.weighted_sum_f64(w, v, ray_off)
    assert got.dtype == f32 and got.shape == (len(DR.COUNTS), C)
    assert np.all(np.abs(got - want) <= bnd)
    empty = np.diff(ray_off) == 0
    assert empty.any() and np.all(got[empty] == 0)
    # quantised inputs: every product and partial sum is exact
    w, v, ray_off = GR.weighted_sum_case(DR.COUNTS, C, seed=C, quantised=True)
    assert np.array_equal(GR.weighted_sum_np(w, v, ray_off).astype(np.float64), GR.weighted_sum_f64(w, v, ray_off)[0])
