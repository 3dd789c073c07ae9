"""CPU: (1) the fp32 emulation of the K/V-split attention form (tests/attention_split_rule.py) keeps to 0.75 of attention_bound against
float64 on every input tests/test_attention_split_gpu.py uses, element by element and as a whole tensor, which is what makes that
file's gate (b) (rel L2 <= 1.5 x the emulation's) a sound one; (2) ctx_attention_plan, the function ctx_attention_core launches by,
gives the mid-size self-attention of a full device to the split form and leaves every other shape of the UNet where it was."""
import ctypes as C
import pytest
import torch
from oracle import attention_ref as A
import attention_split_rule as R

HEADROOM = 0.75


def _ratio(q, k, v, scale=0.125, lazy=8.0):
    want = A.attention_f64(q, k, v, scale)
    emu = R.split_emulated(q, k, v, scale, lazy)
    assert torch.isfinite(emu.float()).all()
    err = (emu.double() - want).abs()
    bound = A.attention_bound(q, k, v, scale)
    return float((err / bound).max()), float(err.norm() / bound.norm())


def test_split_emulation_is_the_plain_one_when_the_second_range_is_empty():
    for Skv in (1, 64):
        q, k, v = A.random_qkv(2, 33, Skv, 2, seed=Skv)
        assert R.split_point(Skv) == Skv
        assert torch.equal(R.split_emulated(q, k, v, 0.125), A.attention_emulated(q, k, v, 0.125))


def test_split_points():
    assert [R.split_point(s) for s in R.SKV] == [1, 64, 64, 64, 128, 192, 192, 256, 320]
    assert sorted({c[1] for c in R.grid_cases()}) == list(R.SQ) and sorted({c[2] for c in R.grid_cases()}) == list(R.SKV)
    assert {c[0] for c in R.grid_cases()} == {1, 2} and {c[3] for c in R.grid_cases()} == {1, 2}


def test_bound_is_reachable_on_the_grid():
    worst = {}
    for B, Sq, Skv, heads in R.grid_cases():
        r, whole = _ratio(*A.random_qkv(B, Sq, Skv, heads, A.case_seed(B, Sq, Skv, heads)))
        worst[Skv] = max(worst.get(Skv, 0.0), r)
        assert r <= HEADROOM and whole <= HEADROOM, f"B{B} Sq{Sq} Skv{Skv} heads{heads}: split emulation at {r:.3f} / {whole:.3f} of the bound"
    print("split emulation / bound, worst per key count:", {s: round(r, 3) for s, r in worst.items()})


@pytest.mark.parametrize("shape", [(2, 193, 448, 2), (2, 193, 193, 2), (2, 193, 321, 2), (2, 1152, 1152, 2), (1, 257, 320, 3)])
def test_bound_is_reachable_on_the_other_shapes(shape):
    r, whole = _ratio(*A.random_qkv(*shape, A.case_seed(*shape)))
    print(f"{shape}: split emulation / bound {r:.3f}, whole tensor {whole:.3f}")
    assert r <= HEADROOM and whole <= HEADROOM


def test_bound_is_reachable_with_a_dominant_key_in_one_range():
    q, k, v, pairs = R.dominant_qkv()
    r, whole = _ratio(q, k, v)
    assert r <= HEADROOM and whole <= HEADROOM
    emu = R.split_emulated(q, k, v, 0.125)
    for i, j in pairs:                                  # the other range weighs exactly nothing
        assert torch.equal(emu[:, i], v[:, j])


def test_bound_is_reachable_on_near_one_hot_rows():
    r, whole = _ratio(*A.sharp_qkv(1, 129, 193, 3, seed=11))
    assert r <= HEADROOM and whole <= HEADROOM


@pytest.mark.parametrize("lazy", [0.0, 8.0, 12.0])
def test_bound_is_reachable_with_a_creeping_maximum(lazy):
    r, whole = _ratio(*A.creeping_qkv(), lazy=lazy)
    print(f"creeping maximum, lazy {lazy}: split emulation / bound {r:.3f}, whole tensor {whole:.3f}")
    assert r <= HEADROOM and whole <= HEADROOM


# ---------------------------------------------------------------------------------------------------------------- the launch plan

def _plan(B, Sq, Skv, heads, n_cu=256):
    from contexture_nerf_amd import _lib as L
    lib = L.load()
    out = (C.c_int32 * 4)()
    L.check(lib.ctx_attention_plan(B, Sq, Skv, heads, n_cu, C.cast(out, C.c_void_p)))
    return list(out)


@pytest.fixture
def no_override():
    from contexture_nerf_amd import _lib as L
    L.load().ctx_attention_tune(-1, -1, -1, -1.0)
    yield
    L.load().ctx_attention_tune(-1, -1, -1, -1.0)


def _wave_tiles(B, Sq, Skv, heads, nw, ks, n_cu):
    """The model, restated: workgroups on the busiest CU x waves per SIMD x (tiles per wave + one for the split form's merge)."""
    wgs = -(-Sq // (32 * nw // ks)) * heads * B
    ntiles = -(-Skv // 64)
    return wgs, -(-wgs // n_cu) * (nw // 4) * (-(-ntiles // ks) + (1 if ks > 1 else 0))


UNET_SHAPES = [(2, 9216, 9216, 5), (2, 2304, 2304, 10), (2, 576, 576, 20), (2, 144, 144, 20),          # self-attention, 96^2 .. 12^2 latents
               (2, 9216, 77, 5), (2, 2304, 77, 10), (2, 576, 77, 20), (2, 144, 77, 20)]               # cross-attention


def test_plan_on_the_unet_shapes(no_override):
    assert _plan(2, 2304, 2304, 10) == [12, 2, 240, 57]             # 8 waves: 72, 4 waves: 72, split: 3 x (18 + 1)
    assert _plan(2, 9216, 9216, 5) == [4, 1, 720, 432]              # split: 2 x 3 x 73 = 438
    assert _plan(2, 576, 576, 20) == [4, 1, 200, 9]                 # split: 3 x 6
    for B in (1, 2, 12):
        for Sq, heads in ((9216, 5), (2304, 10), (576, 20), (144, 20)):
            assert _plan(B, Sq, 77, heads)[:2] == [4, 1], (B, Sq)
    assert _plan(12, 2304, 2304, 10)[:2] == [8, 1]                  # lockstep: 360 against 324 and 342, no form 1/8 ahead
    for shape in UNET_SHAPES:
        p = _plan(*shape)
        assert p[2:] == list(_wave_tiles(*shape, p[0], p[1], 256)), shape


def test_plan_keeps_the_base_form_on_a_tie_and_inside_the_margin(no_override):
    for n_cu in (64, 104, 256, 304):
        for B, Sq, Skv, heads in UNET_SHAPES + [(1, 2304, 2304, 10), (4, 2304, 2304, 10), (1, 1030, 1030, 2), (2, 4096, 4096, 8), (3, 1024, 1024, 16)]:
            base = (8, 1) if 1024 <= Sq < 4096 and Skv >= 1024 else (4, 1)
            cost = {f: _wave_tiles(B, Sq, Skv, heads, *f, n_cu)[1] for f in ((4, 1), (8, 1), (12, 2))}
            p = _plan(B, Sq, Skv, heads, n_cu)
            form = (p[0], p[1])
            assert p[3] == cost[form] == min(cost[form], cost[base])
            if form != base:                                        # left only for the cheapest form, and only beyond the margin
                assert cost[form] == min(cost.values()) and 8 * cost[form] < 7 * cost[base], (n_cu, B, Sq, Skv, heads, cost)
            else:
                assert all(8 * c >= 7 * cost[base] for c in cost.values()), (n_cu, B, Sq, Skv, heads, cost)
    # 2 x 10 heads x 2304^2 on 256 CUs: the 4- and the 8-wave form tie at 72; with the split form switched off the base (8) stays
    assert _wave_tiles(2, 2304, 2304, 10, 4, 1, 256)[1] == _wave_tiles(2, 2304, 2304, 10, 8, 1, 256)[1] == 72


def test_plan_follows_the_override_and_refuses_bad_arguments(no_override):
    from contexture_nerf_amd import _lib as L
    lib = L.load()
    for nw8, form in ((0, [4, 1]), (1, [8, 1]), (2, [12, 2])):
        lib.ctx_attention_tune(-1, nw8, -1, -1.0)
        for shape in UNET_SHAPES:
            assert _plan(*shape)[:2] == form
    lib.ctx_attention_tune(-1, -1, -1, -1.0)
    out = (C.c_int32 * 4)()
    po = C.cast(out, C.c_void_p)
    assert lib.ctx_attention_plan(2, 64, 64, 1, 256, None) != 0
    for bad in ((0, 64, 64, 1, 256), (2, 0, 64, 1, 256), (2, 64, 0, 1, 256), (2, 64, 64, 0, 256), (2, 64, 64, 1, 0)):
        assert lib.ctx_attention_plan(*bad, po) != 0, bad
