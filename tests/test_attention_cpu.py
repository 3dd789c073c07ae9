"""CPU: the error bound that tests/test_attention_gpu.py holds the attention kernel to (oracle/attention_ref.py) is reachable.

A plain fp32 emulation of the kernel's recurrence (64-key tiles, stale maximum per 32-row wave, P rounded to fp16, row sums of the
rounded P, fp16 output) must stay within 0.75 of `attention_bound` against float64 on every input family the GPU file uses.  This is
a condition on the bound, not a measurement of the kernel: a correct implementation of the contract has headroom under it."""
import pytest
import torch
from oracle import attention_ref as A

HEADROOM = 0.75


def _ratio(q, k, v, scale=0.125, lazy=8.0):
    want = A.attention_f64(q, k, v, scale)
    emu = A.attention_emulated(q, k, v, scale, lazy)
    assert torch.isfinite(emu.float()).all()
    err = (emu.double() - want).abs()
    return float((err / A.attention_bound(q, k, v, scale)).max()), float(err.norm() / want.norm())


def test_emulation_is_the_textbook_softmax_when_nothing_is_rounded():
    """The recurrence itself (tiles, stale maximum, rescale) against float64, at a key count that leaves a ragged tile: far below
    fp16 rounding apart from the fp16 P, so compare a variant whose P needs no rounding: one key."""
    q, k, v = A.random_qkv(2, 33, 1, 3, seed=1, planted=False)
    assert torch.equal(A.attention_emulated(q, k, v, 0.125), v[:, :1].expand(2, 33, 192))


def test_bound_is_reachable_on_the_grid():
    cases = sorted(set(A.grid_cases(0)) | set(A.grid_cases(1)))
    worst = {}
    for B, Sq, Skv, heads in cases:
        r, rel = _ratio(*A.random_qkv(B, Sq, Skv, heads, A.case_seed(B, Sq, Skv, heads)))
        worst[Skv] = max(worst.get(Skv, 0.0), r)
        assert r <= HEADROOM, f"B{B} Sq{Sq} Skv{Skv} heads{heads}: emulation at {r:.3f} of the bound"
    print("emulation / bound, worst per key count:", {s: round(r, 3) for s, r in worst.items()})


@pytest.mark.parametrize("B,Sq,Skv,heads,planted", [
    (2, 256, 256, 1, False), (1, 200, 200, 5, False), (2, 1024, 77, 2, False), (2, 96, 7, 1, False), (1, 2304, 2304, 5, False),   # tests/test_unet_gpu.py::test_attention
    (1, 129, 193, 3, True), (2, 129, 193, 3, True), (2, 129, 7, 3, True), (2, 129, 77, 3, True),                                # the layout cases
    (1, 1030, 1030, 2, True), (2, 1031, 1031, 5, True), (1, 257, 320, 3, True), (2, 40, 193, 1, True)])                         # default dispatch, identity
def test_bound_is_reachable_on_the_larger_shapes(B, Sq, Skv, heads, planted):
    seed = Sq + Skv if not planted else A.case_seed(B, Sq, Skv, heads)
    r, rel = _ratio(*A.random_qkv(B, Sq, Skv, heads, seed, planted=planted))
    print(f"B{B} Sq{Sq} Skv{Skv} heads{heads}: emulation / bound {r:.3f}, rel L2 {rel:.3e}")
    assert r <= HEADROOM


def test_bound_is_reachable_on_near_one_hot_rows():
    for B, Sq, Skv, heads in [(1, 129, 193, 3), (2, 33, 320, 1)]:
        q, k, v = A.sharp_qkv(B, Sq, Skv, heads, seed=11)
        s = (A._heads(q).double() @ A._heads(k).double().transpose(-1, -2) * 0.125).abs().max()
        r, rel = _ratio(q, k, v)
        print(f"near-one-hot Skv{Skv}: max |score*scale| {float(s):.1f}, emulation / bound {r:.3f}, rel L2 {rel:.3e}")
        assert 50.0 <= float(s) <= 90.0
        assert r <= HEADROOM


@pytest.mark.parametrize("lazy", [0.0, 8.0, 12.0])
def test_bound_is_reachable_with_a_creeping_maximum(lazy):
    q, k, v = A.creeping_qkv()
    r, rel = _ratio(q, k, v, lazy=lazy)
    print(f"creeping maximum, lazy {lazy}: emulation / bound {r:.3f}, rel L2 {rel:.3e}")
    assert r <= HEADROOM


def test_rescale_branch_inputs():
    """tests/test_unet_gpu.py::test_attention_rescale_branch's inputs."""
    g = torch.Generator().manual_seed(9)
    q = torch.randn(1, 256, 64, generator=g).half(); k = torch.randn(1, 256, 64, generator=g).half(); v = torch.randn(1, 256, 64, generator=g).half()
    k[0, 70] = q[0, 5] * 4; k[0, 200] = q[0, 37] * 6
    r, rel = _ratio(q, k, v)
    print(f"rescale branch: emulation / bound {r:.3f}")
    assert r <= HEADROOM


def test_lazy_and_eager_rescale_agree_within_the_bound():
    """The subtracted maximum is any per-row constant: lazy = 0 (the textbook recurrence) and lazy = 8 differ by rounding only, and
    they do differ where the maximum creeps."""
    for q, k, v in (A.creeping_qkv(), A.random_qkv(2, 129, 193, 3, 5), A.sharp_qkv(1, 129, 193, 3, seed=11)):
        e0 = A.attention_emulated(q, k, v, 0.125, 0.0).double()
        e8 = A.attention_emulated(q, k, v, 0.125, 8.0).double()
        r = float(((e0 - e8).abs() / A.attention_bound(q, k, v, 0.125)).max())
        print(f"lazy 0 vs 8: {r:.3f} of the bound")
        assert r <= 1.0
    q, k, v = A.creeping_qkv()
    assert not torch.equal(A.attention_emulated(q, k, v, 0.125, 0.0), A.attention_emulated(q, k, v, 0.125, 8.0))


def test_strided_views_give_the_same_reference():
    """The references take views: a packed [B*S, 3C] buffer gives what three separate tensors give."""
    q, k, v = A.random_qkv(2, 33, 33, 3, seed=2)
    qkv = torch.cat([q, k, v], -1)
    C = 192
    for fn in (lambda *a: A.attention_f64(*a, 0.125), lambda *a: A.attention_emulated(*a, 0.125), lambda *a: A.attention_bound(*a, 0.125)):
        assert torch.equal(fn(q, k, v), fn(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]))


def test_planted_keys_dominate():
    q, k, v = A.random_qkv(1, 129, 193, 3, seed=3)
    p = torch.softmax(A._heads(q).double() @ A._heads(k).double().transpose(-1, -2) * 0.125, -1)
    pairs = [((7 * n + 3) % 129, j) for n, j in enumerate(A.planted_positions(193))]
    assert [j for _, j in pairs] == [0, 63, 64, 192]
    for i, j in pairs:
        assert float(p[0, :, i, j].min()) > 0.99
    assert A.planted_positions(257) == [0, 63, 64, 256] and A.planted_positions(320) == [0, 63, 64, 319] and A.planted_positions(1) == [0]
