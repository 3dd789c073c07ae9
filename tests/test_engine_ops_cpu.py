"""CPU: the gates of tests/engine_ops_rule.py can tell right from subtly wrong.  The float64 references agree with torch's own ops and
with the kernels' index formulas written out; for every op an fp32 emulation with the kernel's rounding points (but not its layout) lies
inside the rule's bound on every case the GPU test runs (tests/test_engine_ops_gpu.py imports the same cases and seeds); and each of
the listed mutations of an emulation falls outside the bound on at least one of those cases."""
import functools
import math
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import engine_ops_rule as R

f32, f64 = torch.float32, torch.float64


def _inside(got, want, bound, what):
    R.assert_within(got, want, bound, what)


def _caught(ratios, what):
    """a mutation is caught when at least one listed case puts it outside the bound"""
    print(f"{what}: max error / bound per case {[f'{r:.3g}' for r in ratios]}")
    assert max(ratios) > 1.0, f"{what}: the mutation stays inside the bound on every case ({max(ratios):.3f}): the gate cannot see it"


def f32_(v):
    return torch.tensor(v, dtype=f32)


def emu_silu(v):
    """the kernels' v / (1 + __expf(-v)) in fp32"""
    return v / (1.0 + torch.exp(-v))


# ---- emulations -----------------------------------------------------------------------------------------------------------------------
def emu_conv3(x, w, bias, stride=1, silu=False, out=torch.float16, mut=None):
    """x [B,Cin,H,W] as the kernel holds it after its load (fp16 values), w f16 [Cout,Cin,3,3], bias f16: fp32 products and sum with the
    bias in the sum, SiLU in fp32, one rounding to `out`.  mut: 'transpose' (ky / kx swapped), 'replicate' (the border repeats the edge
    pixel instead of reading zero), 'no_bias', 'no_silu', 'drop_chunk' (the last 8 input channels are left out), 'row0' (every batch row
    reads row 0's image)."""
    xf, wf, bf = x.to(f32), w.to(f32), bias.to(f32)
    if mut == "transpose":
        wf = wf.transpose(2, 3)
    if mut == "drop_chunk":
        xf = xf.clone()
        xf[:, -8:] = 0
    if mut == "row0":
        xf = xf[:1].expand_as(xf)
    xp = F.pad(xf, (1, 1, 1, 1), mode="replicate" if mut == "replicate" else "constant")
    acc = F.conv2d(xp, wf, None if mut == "no_bias" else bf, stride=stride)
    if silu and mut != "no_silu":
        acc = emu_silu(acc)
    return acc.to(out)


def emu_pointwise(x, w, b, mut=None):
    xf = x.to(f32)
    if mut == "row0":
        xf = xf[:1].expand_as(xf)
    acc = torch.einsum("oc,bcp->bop", w.to(f32).T if mut == "transpose" else w.to(f32), xf)
    return acc if mut == "no_bias" else acc + b.to(f32)[None, :, None]


def emu_gemv(x, w, bias, silu_in, silu_out, mut=None):
    """k_gemv_f16: SiLU of the fp16 input in fp32, fp32 sum, + bias, SiLU, one rounding.  mut: 'no_silu_in', 'no_silu_out', 'no_bias',
    'drop_chunk' (the last 8 of K), 'row0' (every batch row is row 0), 'row4' (the rows of a later pass of four repeat the first pass)."""
    xf = x.to(f32)
    if mut == "row0":
        xf = xf[:1].expand_as(xf)
    if mut == "row4":
        xf = xf[torch.arange(xf.shape[0]) % 4]
    a = emu_silu(xf) if silu_in and mut != "no_silu_in" else xf
    wf = w.to(f32)
    if mut == "drop_chunk":
        a, wf = a[:, :-8], wf[:, :-8]
    acc = a @ wf.T
    if bias is not None and mut != "no_bias":
        acc = acc + bias.to(f32)
    if silu_out and mut != "no_silu_out":
        acc = emu_silu(acc)
    return acc.half()


def emu_add_scaled(dst, src, scale):
    """one fp32 fused multiply-add (exact in float64: 11 + 24 bits of product), one fp16 rounding"""
    return (dst.to(f64) + float(f32_(scale)) * src.to(f64)).to(f32).half()


def emu_time_embed(B, dim, t, swap=False):
    """k_time_embed in fp32: fr = expf(-9.2103..f * i / h), a = t fr, [cos a | sin a] rounded to fp16, the same row B times"""
    h = dim // 2
    fr = torch.exp(f32_(-9.210340371976184) * torch.arange(h, dtype=f32) / f32_(float(h)))
    a = f32_(t) * fr
    c, s = torch.cos(a), torch.sin(a)
    return torch.cat([s, c] if swap else [c, s]).half().expand(B, dim).contiguous()


def emu_transpose_v(v, heads, Sp, off, pad_value=0.0):
    """k_transpose_v tile by tile: 64 keys x 64 d, keys >= S read as zero, whole 8-key pieces stored below Sp"""
    B, S, ld = v.shape
    vt = torch.full((B, heads, 64, Sp), 7.0, dtype=torch.float16)
    for s0 in range(0, Sp, 64):
        tile = torch.full((B, 64, heads * 64), pad_value, dtype=torch.float16)
        n = max(0, min(64, S - s0))
        tile[:, :n] = v[:, s0:s0 + n, off:off + heads * 64]
        wdt = min(64, Sp - s0)
        vt[..., s0:s0 + wdt] = tile.reshape(B, 64, heads, 64).permute(0, 2, 3, 1)[..., :wdt]
    return vt


def emu_concat(a, b):
    """k_concat index by index over 8-element pieces: piece i -> row i / n8, piece i % n8 of [a | b]"""
    M, Ca = a.shape
    Cb = b.shape[1]
    n8, a8 = (Ca + Cb) // 8, Ca // 8
    i = np.arange(M * n8)
    m, c8 = i // n8, i % n8
    A, Bq = a.reshape(M, a8, 8).numpy(), b.reshape(M, Cb // 8, 8).numpy()
    out = np.where((c8 < a8)[:, None], A[m, np.minimum(c8, a8 - 1)], Bq[m, np.maximum(c8 - a8, 0)])
    return torch.from_numpy(out).reshape(M, Ca + Cb)


def emu_pack(case, src, mut=None):
    """k_pack_copy / k_pack_conv3 / k_pack_geglu index by index.  mut: 'tap_t' (tap index read as kx 3 + ky), 'pad' (the padding keeps
    the clamped channel's weight), 'halves' (GEGLU rows not interleaved)."""
    kind, a, b = case
    s = src.reshape(-1).numpy()
    if kind == R.PK_COPY:
        return torch.from_numpy(s.astype(np.float16))
    if kind in (R.PK_CONV3, R.PK_CONVIN):
        Cinp = R.conv_in_pad(b) if kind == R.PK_CONVIN else b
        i = np.arange(a * 9 * Cinp)
        c, tap, o = i % Cinp, (i // Cinp) % 9, i // (Cinp * 9)
        if mut == "tap_t":
            tap = (tap % 3) * 3 + tap // 3
        val = s[(o * b + np.minimum(c, b - 1)) * 9 + tap]
        return torch.from_numpy((val if mut == "pad" else np.where(c < b, val, np.float32(0))).astype(np.float16))
    kk = b if kind == R.PK_GEGLU_W else 1
    i = np.arange(2 * a * kk)
    k, p = i % kk, i // kk
    blk, w = p // 64, p % 64
    row = p if mut == "halves" else np.where(w < 32, blk * 32 + w, a + blk * 32 + (w - 32))
    return torch.from_numpy(s[row * kk + k].astype(np.float16))


# ---- the references against torch and against the index formulas ----------------------------------------------------------------------------
def test_conv_reference_is_the_kernels_tap_formula():
    """F.conv2d(padding=1) in float64 == sum over t of x[oy stride + t / 3 - 1][ox stride + t % 3 - 1] w[o][c][t / 3][t % 3], zero outside,
    which is what k_conv_in / k_conv_out / k_conv_small compute; on an odd grid, stride 1 and 2"""
    g = R.gen(1)
    x, w, bias = torch.randn(2, 5, 7, 9, generator=g, dtype=f64), torch.randn(6, 5, 3, 3, generator=g, dtype=f64), torch.randn(6, generator=g, dtype=f64)
    for stride in (1, 2):
        want, S = R.conv3_ref(x, w, bias, stride)
        Ho, Wo = (7 - 1) // stride + 1, (9 - 1) // stride + 1
        assert want.shape == (2, 6, Ho, Wo)
        acc, mag = bias.reshape(1, 6, 1, 1).expand(2, 6, Ho, Wo).clone(), bias.abs().reshape(1, 6, 1, 1).expand(2, 6, Ho, Wo).clone()
        for oy in range(Ho):
            for ox in range(Wo):
                for t in range(9):
                    iy, ix = oy * stride + t // 3 - 1, ox * stride + t % 3 - 1
                    if 0 <= iy < 7 and 0 <= ix < 9:
                        acc[:, :, oy, ox] += x[:, :, iy, ix] @ w[:, :, t // 3, t % 3].T
                        mag[:, :, oy, ox] += x[:, :, iy, ix].abs() @ w[:, :, t // 3, t % 3].abs().T
        assert (acc - want).abs().max() < 1e-12 and (mag - S).abs().max() < 1e-12


def test_gemv_and_pointwise_references_are_torchs_linear_silu_conv():
    for case in R.GEMV_CASES[:5]:
        x, w, bias = R.gemv_inputs(case)
        want, bound = R.gemv_ref(x, w, bias, case[3], case[4])
        a = F.silu(x.to(f64)) if case[3] else x.to(f64)
        y = F.linear(a, w.to(f64), bias.to(f64) if bias is not None else None)
        assert (want - (F.silu(y) if case[4] else y)).abs().max() < 1e-12
        assert (bound > 0).all()
    with pytest.raises(AssertionError):
        R.gemv_ref(torch.zeros(1, 8200).half(), torch.zeros(1, 8200).half(), None, 0, 0)
    for case in R.POINTWISE_CASES:
        x, w, b = R.pointwise_inputs(case)
        want, _ = R.pointwise_ref(x, w, b)
        assert (want - F.conv2d(x.to(f64)[..., None], w.to(f64)[:, :, None, None], b.to(f64))[..., 0]).abs().max() < 1e-12


def test_time_embed_reference_is_diffusers_formula():
    """get_timestep_embedding(timesteps, dim, flip_sin_to_cos=True, downscale_freq_shift=0) as diffusers writes it, in fp32"""
    for B, dim, t in R.TIME_EMBED_CASES:
        half = dim // 2
        exponent = -math.log(10000) * torch.arange(start=0, end=half, dtype=f32) / (half - 0)
        emb = torch.full((B,), t, dtype=f32)[:, None].float() * torch.exp(exponent)[None, :]
        emb = torch.cat([torch.sin(emb), torch.cos(emb)], dim=-1)
        emb = torch.cat([emb[:, half:], emb[:, :half]], dim=-1)                # flip_sin_to_cos
        want, bound = R.time_embed_ref(B, dim, t)
        assert want.shape == (B, dim)
        assert bool((bound == R.U10 + abs(t) * 2.0 ** -21).all())
        assert (emb - want).abs().max() <= abs(t) * 2.0 ** -21, "the fp32 formula is off by more than the bound's argument term"


def test_pack_references_are_the_index_formulas():
    for case in R.PACK_CASES:
        src = R.pack_inputs(case)
        assert torch.equal(R.bits(emu_pack(case, src)), R.bits(R.pack_ref(case, src))), f"pack {case}"
    w = R.pack_inputs((R.PK_CONVIN, 16, 5))
    p = R.pack_conv3_ref(w, 8)
    assert p.shape == (16, 3, 3, 8) and (R.bits(p[..., 5:]) == 0).all() and p[3, 1, 2, 4] == w[3, 4, 1, 2].half()
    rows = R.geglu_rows(64)
    assert rows[:32].tolist() == list(range(32)) and rows[32:64].tolist() == list(range(64, 96)) and rows[64:96].tolist() == list(range(32, 64))
    assert sorted(rows.tolist()) == list(range(128))


def test_mover_references_are_the_index_formulas():
    for case in R.TRANSPOSE_V_CASES:
        v = R.transpose_v_inputs(case)
        assert torch.equal(R.bits(emu_transpose_v(v, *case[3:])), R.bits(R.transpose_v_ref(v, *case[3:]))), f"transpose_v {case}"
    for case in R.CONCAT_F16_CASES:
        a, b = R.concat_inputs(case, torch.float16)
        assert torch.equal(R.bits(emu_concat(a, b)), R.bits(torch.cat([a, b], 1))), f"concat {case}"
    for case in R.CONCAT_F32_CASES:                                             # the alias: a float is two halves
        a, b = R.concat_inputs(case, f32)
        got = emu_concat(a.view(torch.float16), b.view(torch.float16)).view(f32)
        assert torch.equal(R.bits(got), R.bits(torch.cat([a, b], 1))), f"concat_f32 {case}"


def test_f32_to_f16_inputs_hold_the_edge_cases():
    x = R.f32_to_f16_inputs(1000)
    h = x.half()
    fin = torch.isfinite(x)
    assert torch.isnan(h).sum() == 1 and (torch.isinf(h) & fin).sum() >= 6                 # finite values that round to inf
    sub = (h != 0) & (h.abs() < 2.0 ** -14)
    assert sub.sum() >= 10 and ((h == 0) & (x != 0)).sum() >= 4                            # fp16 subnormals; underflow to zero
    assert (R.bits(h) == -32768).any() and (R.bits(h) == 0).any()                         # -0 and +0
    d = x.to(f64)
    lo = torch.nextafter(h, torch.full_like(h, -float("inf"))).to(f64)
    hi = torch.nextafter(h, torch.full_like(h, float("inf"))).to(f64)
    ok = fin & torch.isfinite(h) & torch.isfinite(lo) & torch.isfinite(hi)
    tie = ok & (((d - lo) == (h.to(f64) - d)) | ((hi - d) == (d - h.to(f64)))) & (d != h.to(f64))
    assert tie.sum() >= 8, "halfway cases"
    assert ((R.bits(h)[tie] & 1) == 0).all(), "torch's .half() rounds ties to even"
    y = R.f16_to_f32_inputs(65536 + 8)
    assert torch.isnan(y).sum() == 2046 and torch.isinf(y).sum() == 2


# ---- the emulations lie inside the bounds ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _conv_in(case):
    x, w, bias = R.conv_in_inputs(case)
    return (x.half(), w, bias) + R.conv_in_ref(x, w, bias)


@functools.lru_cache(maxsize=None)
def _conv_out(case):
    x, w, bias = R.conv_out_inputs(case)
    return (x, w, bias) + R.conv_out_ref(x, w, bias)


@functools.lru_cache(maxsize=None)
def _conv_small(case):
    x, w, bias = R.conv_small_inputs(case)
    return (x.half(), w, bias) + R.conv_small_ref(x, w, bias, case[5], case[7])


@pytest.mark.parametrize("case", R.CONV_IN_CASES)
def test_conv_in_emulation_inside(case):
    x, w, bias, want, bound = _conv_in(case)
    _inside(R.nhwc(emu_conv3(x, w, bias)), want, bound, f"conv_in {case}")


@pytest.mark.parametrize("case", R.CONV_OUT_CASES)
def test_conv_out_emulation_inside(case):
    x, w, bias, want, bound = _conv_out(case)
    _inside(emu_conv3(x, w, bias, out=f32), want, bound, f"conv_out {case}")


@pytest.mark.parametrize("case", R.CONV_SMALL_CASES)
def test_conv_small_emulation_inside(case):
    x, w, bias, want, bound = _conv_small(case)
    _inside(R.nhwc(emu_conv3(x, w, bias, stride=case[5], silu=bool(case[7]))), want, bound, f"conv_small {case}")


@pytest.mark.parametrize("case", R.POINTWISE_CASES)
def test_pointwise_emulation_inside(case):
    x, w, b = R.pointwise_inputs(case)
    _inside(emu_pointwise(x, w, b), *R.pointwise_ref(x, w, b), f"pointwise {case}")


@pytest.mark.parametrize("case", R.GEMV_CASES)
def test_gemv_emulation_inside(case):
    x, w, bias = R.gemv_inputs(case)
    _inside(emu_gemv(x, w, bias, case[3], case[4]), *R.gemv_ref(x, w, bias, case[3], case[4]), f"gemv {case}")


@pytest.mark.parametrize("case", R.ADD_SCALED_CASES)
def test_add_scaled_emulation_inside(case):
    dst, src = R.add_scaled_inputs(case)
    _inside(emu_add_scaled(dst, src, case[1]), *R.add_scaled_ref(dst, src, case[1]), f"add_scaled {case}")


@pytest.mark.parametrize("case", R.TIME_EMBED_CASES)
def test_time_embed_emulation_inside(case):
    _inside(emu_time_embed(*case), *R.time_embed_ref(*case), f"time_embed {case}")


# ---- the bounds reject the mutations -----------------------------------------------------------------------------------------------------
def _ratios(cases, fn):
    return [fn(c) for c in cases]


@pytest.mark.parametrize("mut", ["transpose", "replicate", "no_bias", "row0"])
def test_conv_in_bound_rejects(mut):
    def r(case):
        x, w, bias, want, bound = _conv_in(case)
        return R.ratio(R.nhwc(emu_conv3(x, w, bias, mut=mut)), want, bound)[0]
    _caught(_ratios(R.CONV_IN_CASES, r), f"conv_in, {mut}")


@pytest.mark.parametrize("mut", ["transpose", "replicate", "no_bias", "row0", "drop_chunk"])
def test_conv_out_bound_rejects(mut):
    def r(case):
        x, w, bias, want, bound = _conv_out(case)
        return R.ratio(emu_conv3(x, w, bias, out=f32, mut=mut), want, bound)[0]
    _caught(_ratios(R.CONV_OUT_CASES, r), f"conv_out, {mut}")


@pytest.mark.parametrize("mut", ["transpose", "replicate", "no_bias", "row0", "drop_chunk", "no_silu"])
def test_conv_small_bound_rejects(mut):
    def r(case):
        x, w, bias, want, bound = _conv_small(case)
        return R.ratio(R.nhwc(emu_conv3(x, w, bias, stride=case[5], silu=bool(case[7]), mut=mut)), want, bound)[0]
    _caught(_ratios(R.CONV_SMALL_CASES, r), f"conv_small, {mut}")


@pytest.mark.parametrize("mut", ["transpose", "no_bias", "row0"])
def test_pointwise_bound_rejects(mut):
    def r(case):
        x, w, b = R.pointwise_inputs(case)
        return R.ratio(emu_pointwise(x, w, b, mut=mut), *R.pointwise_ref(x, w, b))[0]
    _caught(_ratios(R.POINTWISE_CASES, r), f"pointwise, {mut}")


@pytest.mark.parametrize("mut", ["no_silu_in", "no_silu_out", "no_bias", "drop_chunk", "row0", "row4"])
def test_gemv_bound_rejects(mut):
    def r(case):
        x, w, bias = R.gemv_inputs(case)
        return R.ratio(emu_gemv(x, w, bias, case[3], case[4], mut=mut), *R.gemv_ref(x, w, bias, case[3], case[4]))[0]
    _caught(_ratios(R.GEMV_CASES, r), f"gemv, {mut}")


def test_gemv_drop_chunk_is_caught_at_every_k():
    """the K tail is where the kernel clamps and masks: the gate must see a dropped last chunk at each listed K, not at one of them"""
    for case in R.GEMV_CASES:
        x, w, bias = R.gemv_inputs(case)
        r = R.ratio(emu_gemv(x, w, bias, case[3], case[4], mut="drop_chunk"), *R.gemv_ref(x, w, bias, case[3], case[4]))[0]
        assert r > 1.0, f"gemv {case}: a dropped last chunk is at {r:.3f} of the bound"


def test_add_scaled_bound_rejects_a_dropped_scale_and_a_missed_tail():
    rs, rt = [], []
    for case in R.ADD_SCALED_CASES:
        dst, src = R.add_scaled_inputs(case)
        want, bound = R.add_scaled_ref(dst, src, case[1])
        rs.append(R.ratio(emu_add_scaled(dst, src, 1.0 if case[1] != 1.0 else 0.0), want, bound)[0])
        got = emu_add_scaled(dst, src, case[1])
        got[-8:] = dst[-8:]                                       # the last vector (past the capped grid's first sweep) left as it was
        rt.append(R.ratio(got, want, bound)[0])
    assert min(rs) > 1.0, rs
    _caught([rt[R.ADD_SCALED_CASES.index((R.ADD_SCALED_CAP + 8, 0.37))]], "add_scaled, the vector past the capped grid not written")


def test_time_embed_bound_rejects_swapped_halves():
    rs = [R.ratio(emu_time_embed(*c, swap=True), *R.time_embed_ref(*c))[0] for c in R.TIME_EMBED_CASES]
    print(rs)
    assert min(rs) > 1.0, "sin | cos for cos | sin must fail at every listed case"


def test_bit_equality_rejects_nonzero_padding_and_wrong_order():
    for case in R.TRANSPOSE_V_CASES:
        v = R.transpose_v_inputs(case)
        want = R.transpose_v_ref(v, *case[3:])
        if case[4] > case[1]:
            assert not torch.equal(R.bits(emu_transpose_v(v, *case[3:], pad_value=-0.0)), R.bits(want)), f"transpose_v {case}: -0 padding passes"
    for case in R.PACK_CASES:
        src = R.pack_inputs(case)
        want = R.bits(R.pack_ref(case, src))
        if case[0] in (R.PK_CONV3, R.PK_CONVIN):
            assert not torch.equal(R.bits(emu_pack(case, src, "tap_t")), want), f"pack {case}: transposed taps pass"
        if case[0] == R.PK_CONVIN:
            assert not torch.equal(R.bits(emu_pack(case, src, "pad")), want), f"pack {case}: non-zero padding passes"
        if case[0] in (R.PK_GEGLU_W, R.PK_GEGLU_B):
            assert not torch.equal(R.bits(emu_pack(case, src, "halves")), want), f"pack {case}: rows without the interleave pass"


# ---- the refusals need no device: a refused call returns before it touches one ------------------------------------------------------------
def test_refusals_return_e_arg_without_a_device():
    import ctypes as C
    from contexture_nerf_amd import _lib as L
    lib = L.load()
    buf = (C.c_char * 4096)()                                     # stands in for every pointer: a refused call reads none of them
    p, null = C.cast(buf, C.c_void_p), C.c_void_p(0)
    calls = [(lib.ctx_conv_in_f16(p, p, p, B, Cin, H, W, Cout, p, null), "conv_in") for B, Cin, H, W, Cout in R.CONV_IN_REFUSED]
    calls += [(lib.ctx_conv_out_f16(p, p, p, B, H, W, Cc, Cout, p, null), "conv_out") for B, H, W, Cc, Cout in R.CONV_OUT_REFUSED]
    calls += [(lib.ctx_transpose_v_f16(p, B, S, ld, heads, Sp, p, null), "transpose_v") for B, S, ld, heads, Sp, _ in R.TRANSPOSE_V_REFUSED]
    calls += [(lib.ctx_gemv_f16(p, p, p, Bm, N, K, 0, 0, p, null), "gemv") for Bm, N, K in R.GEMV_REFUSED]
    calls += [(lib.ctx_conv_small_f16(p, p, p, p, 1, 4, 4, 8, 8, 1, 0, p, null), "conv_small"), (lib.ctx_conv_small_f16(null, null, p, p, 1, 4, 4, 8, 8, 1, 0, p, null), "conv_small"),
              (lib.ctx_conv_small_f16(p, null, p, p, 1, 4, 4, 8, 12, 1, 0, p, null), "conv_small"), (lib.ctx_conv_small_f16(p, null, p, p, 1, 4, 4, 8, 8, 3, 0, p, null), "conv_small")]
    calls += [(lib.ctx_pointwise_f32(p, p, p, B, Cc, HW, nh, p, null), "pointwise") for nh, B, Cc, HW in R.POINTWISE_REFUSED]
    calls += [(lib.ctx_add_scaled_f16(p, p, 1.0, n, null), "add_scaled") for n in R.ADD_SCALED_REFUSED]
    calls += [(lib.ctx_concat_f16(p, p, M, Ca, Cb, p, null), "concat") for M, Ca, Cb in R.CONCAT_REFUSED]
    calls += [(lib.ctx_time_embed_f16(p, B, dim, p, null), "time_embed") for B, dim in R.TIME_EMBED_REFUSED]
    calls += [(lib.ctx_pack_fwd_f16(p, kind, a, b, p, null), "pack") for kind, a, b in R.PACK_REFUSED]
    calls += [(lib.ctx_f16_to_f32(p, 12, p, null), "f16_to_f32"), (lib.ctx_f32_to_f16(p, 0, p, null), "f32_to_f16")]
    assert all(rc == -1 for rc, _ in calls), [(rc, op) for rc, op in calls if rc != -1]
    assert lib.ctx_conv_in_f16(p, p, p, 1, 17, 4, 4, 8, p, null) == -1 and b"Cin" in lib.ctx_last_error()
    assert bytes(buf) == bytes(4096)
