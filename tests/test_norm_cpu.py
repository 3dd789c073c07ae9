"""CPU: the norm kernels' launch plans over the whole accepted envelope (ctx_groupnorm_plan / ctx_layernorm_plan: the functions the
launchers themselves call), the refusals, the comparator of tests/norm_rule.py judged by two fp32 emulations of the statistics, and
the class coverage of the GPU test's case lists (tests/test_norm_gpu.py imports the same lists)."""
import ctypes as C

import numpy as np
import pytest
import torch

import norm_rule as R

E_ARG = R.E_ARG
GROUPS = (1, 2, 4, 8, 16, 32, 64)
HWS = tuple(range(1, 41)) + (63, 64, 65, 143, 144, 145, 576, 577, 600, 612, 613, 1023, 1024, 1025, 2304, 6144, 6145, 9216, 16384, 36864, 589824)
BATCHES = (1, 2, 12)


@pytest.fixture(scope="module")
def lib():
    from contexture_nerf_amd import _lib as L
    return L.load()


def _covered_once(HW, apl, nb):
    """pixel p0 + u apl + pl of block blk (p0 = blk apl AU, u < AU, pl < apl), kept when < HW: every pixel exactly once"""
    run = apl * R.GN_AU
    if (nb - 1) * run >= HW or nb * run < HW:
        return False
    if HW > 4096:                                  # u apl + pl is a bijection onto 0 .. run: the two inequalities above are the whole claim
        return True
    blk, u, pl = np.meshgrid(np.arange(nb), np.arange(R.GN_AU), np.arange(apl), indexing="ij")
    p = (blk * run + u * apl + pl).ravel()
    return bool((np.bincount(p[p < HW], minlength=HW) == 1).all())


@pytest.mark.parametrize("x32", (0, 1))
def test_groupnorm_plan_over_the_envelope(lib, x32):
    out = (C.c_int32 * 12)()
    po = C.cast(out, C.c_void_p)
    plan = lib.ctx_groupnorm_plan
    n = two_pass = 0
    apply_seen = set()
    for Cc in range(8, 4097, 8):
        c8n = Cc // 8
        for G in GROUPS:
            if Cc % G:
                continue
            cg = Cc // G
            for HW in HWS:
                for B in BATCHES:
                    assert plan(B, HW, Cc, G, x32, 0, po) == 0, (B, HW, Cc, G)
                    one, plf, thr, PL, threads, NS, na, lds, apl, athreads, nb, optin = out
                    n += 1
                    what = (B, HW, Cc, G, x32, tuple(out))
                    if one:
                        assert cg % 8 == 0 and thr % 64 == 0 and cg // 8 * plf <= thr <= 512 and -(-HW // plf) <= R.GN_FU, what
                    else:
                        two_pass += 1
                        assert 8 <= threads <= 1024 and threads % 64 == 0 and threads >= c8n * PL and 1 <= PL <= HW, what
                        assert na == max(1, threads // Cc) and lds == (PL + na) * Cc * 8 and lds <= optin == 96 * 1024, what
                        assert 1 <= NS <= 128 and NS * -(-HW // NS) >= HW and NS * PL <= max(HW, PL), what
                    assert 256 <= athreads <= 512 and athreads == c8n * apl, what
                    if (HW, Cc) not in apply_seen:
                        apply_seen.add((HW, Cc))
                        assert _covered_once(HW, apl, nb), what
    print(f"x32={x32}: {n} shapes, {two_pass} of them two-pass")
    assert n > 100000 and two_pass > n // 4


def test_layernorm_plan_over_the_envelope(lib):
    out = (C.c_int64 * 4)()
    po = C.cast(out, C.c_void_p)
    seen = set()
    for Cc in range(8, 2049, 8):
        for rows in (1, 8, 63, 64, 65, 8191, 8192, 8197):
            for x32 in (0, 1):
                assert lib.ctx_layernorm_plan(rows, Cc, x32, po) == 0
                g8, KC, Rr, blocks = out
                what = (rows, Cc, x32, tuple(out))
                if g8:
                    assert not x32 and Cc == 64 * KC and 1 <= KC <= 10 and rows >= 64 and Rr == 8, what
                    assert blocks * 32 >= rows > (blocks - 1) * 32, what                       # 8 rows per wave, 4 waves per block
                else:
                    assert 1 <= KC <= 4 and KC * 64 * 8 >= Cc > (KC - 1) * 64 * 8 and (KC, Rr) in ((1, 1), (1, 4), (2, 1), (2, 2), (3, 1), (4, 1)), what
                    assert blocks * 4 * Rr >= rows > (blocks - 1) * 4 * Rr, what               # R rows per wave
                seen.add((g8, KC, Rr))
    assert len(seen) == 16


def test_seams_refuse_without_a_device(lib):
    buf = (C.c_uint16 * 64)()
    p = C.cast(buf, C.c_void_p)
    out = (C.c_int64 * 12)()
    po = C.cast(out, C.c_void_p)
    # (B, HW, C, G): C % 8, C % G, G = 3, G = 128, C = 4104, nothing to do
    for B, HW, Cc, G in [(1, 16, 12, 1), (1, 16, 64, 24), (1, 16, 48, 3), (1, 16, 256, 128), (1, 16, 4104, 8), (0, 16, 64, 8), (1, 0, 64, 8), (1, 16, 64, 0)]:
        assert lib.ctx_groupnorm_plan(B, HW, Cc, G, 0, 0, po) == E_ARG, (B, HW, Cc, G)
        assert lib.ctx_last_error()
        assert lib.ctx_groupnorm_f16(p, p, p, B, HW, Cc, G, 1e-5, 1, p, p, None) == E_ARG, (B, HW, Cc, G)
        assert lib.ctx_groupnorm_f32in_f16(p, p, p, B, HW, Cc, G, 1e-5, 1, p, p, None) == E_ARG, (B, HW, Cc, G)
        assert lib.ctx_groupnorm2_f16(p, p, 8, p, p, B, HW, Cc, G, 1e-5, 1, p, p, None) == E_ARG, (B, HW, Cc, G)
        assert lib.ctx_groupnorm_apply_f16(p, p, 4, p, p, B, HW, Cc, G, 1e-5, 1, p, None) == E_ARG, (B, HW, Cc, G)
    for Ca in (4, 12, 64, 72, -8):                                                             # Ca in whole columns inside 0 .. C
        assert lib.ctx_groupnorm_plan(1, 16, 64, 8, 0, Ca, po) == E_ARG, Ca
        assert lib.ctx_groupnorm2_f16(p, p, Ca, p, p, 1, 16, 64, 8, 1e-5, 1, p, p, None) == E_ARG, Ca
    assert lib.ctx_groupnorm2_f16(p, p, 0, p, p, 1, 16, 64, 8, 1e-5, 1, p, p, None) == E_ARG
    for slots in (0, 129):
        assert lib.ctx_groupnorm_apply_f16(p, p, slots, p, p, 1, 16, 64, 8, 1e-5, 1, p, None) == E_ARG
    for rows, Cc in [(4, 2056), (4, 12), (0, 64), (4, 0)]:
        assert lib.ctx_layernorm_plan(rows, Cc, 0, po) == E_ARG, (rows, Cc)
        assert lib.ctx_layernorm_f16(p, p, p, rows, Cc, 1e-5, p, None) == E_ARG, (rows, Cc)
        assert lib.ctx_layernorm_f32in_f16(p, p, p, rows, Cc, 1e-5, p, None) == E_ARG, (rows, Cc)
    assert lib.ctx_groupnorm_plan(1, 16, 64, 8, 0, 0, None) == E_ARG


def test_small_blocks_and_wide_tensors_are_planned_not_refused(lib):
    """The shapes that used to get a stats block of 3 .. 7 threads (its fold then never advanced) now get a whole wave, and the
    two-pass form beyond C = 2560 gets the LDS it asks for: the opt-in is sized from the plan."""
    for B, HW, Cc, G in [(1, 7, 8, 2), (1, 3, 8, 2), (1, 3, 16, 4), (1, 1, 32, 8), (1, 1, 56, 8)]:
        p = R.gn_plan(lib, B, HW, Cc, G)
        assert p and not p["one"] and (Cc // 8) * p["PL"] < 8 and p["threads"] == 64, (B, HW, Cc, G, p)
    for Cc in (2568, 2728, 3416, 4096):                                  # 3 pixel lanes up to c8n 341, then 2: c8n 427 is the first of them above 80 KiB
        p = R.gn_plan(lib, 1, 13, Cc, 1)
        assert p and not p["one"] and 80 * 1024 < p["lds"] <= p["lds_optin"], (Cc, p)


# ---- the comparator is neither blind nor unfair ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(2304, 20), (9216, 10)], ids=["n=2304x20", "n=9216x10"])
def judged(request):
    """one tensor per n whose groups are the input makers in turn; fp16 and fp32 input"""
    HW, cg = request.param
    out = {}
    for x32, kinds in ((False, R.KINDS16), (True, R.KINDS32)):
        G = len(kinds)
        x, names = R.gn_input(1, HW, cg * G, G, kinds, x32)
        gamma, beta = R.affine(cg * G)
        out[x32] = (x, names[0], gamma, beta, G)
    return out


@pytest.mark.parametrize("silu", (0, 1))
@pytest.mark.parametrize("x32", (False, True), ids=["f16", "f32"])
def test_comparator_accepts_two_pass_and_rejects_the_rest(judged, x32, silu):
    """Fair: fp32 arithmetic on two-pass fp32 statistics uses at most half of an element's bound in front of the output's rounding
    (a correctly rounded fp16 output alone can use all of the bound's first term, so the rounded emulation is held to 1), at every
    conditioning.  Not blind: rstd off by 2^-9 and sumsq/n - mean^2 on shifted groups are outside."""
    x, names, gamma, beta, G = judged[x32]
    want, bound = R.gn_ref(x, gamma, beta, G, R.GN_EPS, silu)
    two = R.per_group_worst(R.emu_gn(x, gamma, beta, G, R.GN_EPS, silu, "two_pass", round16=False), want, bound, G)[0]
    two16 = R.per_group_worst(R.emu_gn(x, gamma, beta, G, R.GN_EPS, silu, "two_pass"), want, bound, G)[0]
    one = R.per_group_worst(R.emu_gn(x, gamma, beta, G, R.GN_EPS, silu, "one_pass"), want, bound, G)[0]
    # float64 with rstd scaled by 1 + 2^-9, rounded to fp16
    B, HW, Cc = x.shape
    xg = x.double().reshape(B, HW, G, -1)
    mean = xg.mean((1, 3), keepdim=True)
    rstd = (1 + 2.0 ** -9) / torch.sqrt(xg.var((1, 3), unbiased=False, keepdim=True) + R.GN_EPS)
    y = (xg - mean) * rstd * gamma.double().reshape(1, 1, G, -1) + beta.double().reshape(1, 1, G, -1)
    if silu:
        y = y * torch.sigmoid(y)
    scaled = R.per_group_worst(y.reshape(B, HW, Cc).half(), want, bound, G)[0]
    for g, kind in enumerate(names):
        print(f"{kind:9s} two-pass {float(two[g]):.3f} (rounded {float(two16[g]):.3f})  one-pass {float(one[g]):.3g}  rstd (1 + 2^-9) {float(scaled[g]):.3f}")
        assert two[g] <= 0.5, f"{kind}: the two-pass fp32 emulation is at {float(two[g]):.3f} of the bound: the bound is unfair"
        assert two16[g] <= 1.0, f"{kind}: the rounded two-pass fp32 emulation is at {float(two16[g]):.3f} of the bound"
        if kind == "const":
            assert scaled[g] <= 1.0                                    # x^ = 0: no rstd can be seen
        else:
            assert scaled[g] > 1.0, f"{kind}: rstd off by 2^-9 stays inside the bound ({float(scaled[g]):.3f})"
        if kind in R.SHIFTED:
            assert one[g] > 1.0, f"{kind}: sumsq/n - mean^2 stays inside the bound ({float(one[g]):.3f})"


def test_layernorm_comparator_on_shifted_rows():
    """the same bound through ln_ref: a two-pass fp32 row is inside, rstd (1 + 2^-9) is outside"""
    x, names = R.ln_input(12, 320)
    gamma, beta = R.affine(320)
    want, bound = R.ln_ref(x, gamma, beta)
    emu = R.emu_gn(x.reshape(12, 1, 320), gamma, beta, 1, R.LN_EPS, 0, "two_pass", round16=False).reshape(12, 320)
    r = R.ratios(emu, want, bound).amax(1)
    assert (r <= 0.5).all(), r
    assert (R.ratios(emu.half(), want, bound) <= 1.0).all()
    xd = x.double()
    y = (xd - xd.mean(1, keepdim=True)) * (1 + 2.0 ** -9) / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + R.LN_EPS) * gamma.double() + beta.double()
    r = R.ratios(y.half(), want, bound).amax(1)
    assert all(v > 1.0 for v, k in zip(r, names) if k != "const"), r


def test_backward_bound_sees_wrong_statistics():
    """an fp32 emulation of the backward with two-pass statistics is inside the bound at every conditioning; with
    sumsq/n - mean^2 it is outside from mean / sigma 300 on"""
    f32 = torch.float32
    for case in R.BWD_CASES[:2]:
        B, HW, Cc, G, silu, add = case
        for ratio in R.BWD_RATIOS:
            x, dy, gamma, beta, a = R.bwd_inputs(case, ratio)
            want, bound = R.gn_bwd_ref(x, dy, gamma, beta, a, G, silu)
            res = {}
            for mode in ("two_pass", "one_pass"):
                xf = x.to(f32).reshape(B, HW, G, -1)
                st = [[R.emu_stats(xf[b, :, g].numpy(), mode) for g in range(G)] for b in range(B)]
                mean = torch.tensor([[float(m) for m, _ in row] for row in st], dtype=f32).reshape(B, 1, G, 1)
                rstd = torch.rsqrt(torch.tensor([[float(v) for _, v in row] for row in st], dtype=f32).reshape(B, 1, G, 1) + f32_(1e-6))
                ga, be = gamma.to(f32).reshape(1, 1, G, -1), beta.to(f32).reshape(1, 1, G, -1)
                xh = (xf - mean) * rstd
                u = xh * ga + be
                du = dy.to(f32).reshape(B, HW, G, -1)
                if silu:
                    sg = torch.sigmoid(u)
                    du = du * (sg * (1.0 + u * (1.0 - sg)))
                du = du * ga
                out = (rstd * (du - du.mean((1, 3), keepdim=True) - xh * (du * xh).mean((1, 3), keepdim=True))).reshape(B, HW, Cc)
                if a is not None:
                    out = out + a.to(f32)
                res[mode] = R.worst(out.half(), want, bound)[0]
            print(f"backward {case} mean/sigma {ratio}: two-pass {res['two_pass']:.3f}, one-pass {res['one_pass']:.3g}")
            assert res["two_pass"] <= 1.0
            if ratio >= 300:
                assert res["one_pass"] > 1.0


def f32_(v):
    return torch.tensor(v, dtype=torch.float32)


# ---- the GPU test's case lists hit every class the plan distinguishes ------------------------------------------------------------------
def test_case_lists_cover_every_class(lib):
    tags = set()
    for B, HW, Cc, G, _ in R.GN_CASES:
        tags |= R.gn_classes(R.gn_plan(lib, B, HW, Cc, G), B, HW, Cc, G)
    for B, HW, Cc, G, Ca, _ in R.GN2_CASES:
        tags |= R.gn_classes(R.gn_plan(lib, B, HW, Cc, G, 0, Ca), B, HW, Cc, G, Ca)
    for B, HW, Cc, G, NS in R.APPLY_CASES:
        tags.add(f"fold trips={R.fold_trips(NS, G)}")
    need = {f"one-kernel cpg={k}" for k in (1, 3, 5, 10, 16, 512)} | {"one-kernel at HW = 12 plf", "two-pass at HW = 12 plf + 1"}
    need |= {f"two-pass c8n={k}" for k in (1, 8, 40, 96, 200, 320, 512)} | {"na>1", "na=1", "NS=1", "ragged last split", "empty last split"}
    need |= {"want from B=1", "want from B=12"} | {f"two-pass cg={k}" for k in (1, 2, 4, 6, 10, 20, 60, 80)} | {f"G={k}" for k in (1, 2, 64)}
    need |= {f"fold trips={k}" for k in (1, 2, 4)} | {"two sources, aligned", "two sources, a group straddles Ca"}
    need |= {"stats block rounded up to whole waves", "fewer than 8 working stats lanes", "stats LDS above 80 KiB"}
    assert not need - tags, f"no case for {sorted(need - tags)}"
    for B, HW, Cc, G, _ in R.GN32_CASES:
        assert R.gn_plan(lib, B, HW, Cc, G, 1) is not None
    assert {bool(R.gn_plan(lib, B, HW, Cc, G, 1)["one"]) for B, HW, Cc, G, _ in R.GN32_CASES} == {True, False}

    tags = set()
    for rows, Cc, _ in R.LN_CASES:
        tags |= R.ln_classes(R.ln_plan(lib, rows, Cc), rows, Cc)
    need = {f"g8 KC={k}" for k in range(1, 11)} | {f"wave-per-row kc={k} R=1" for k in (1, 2, 3, 4)}
    need |= {"wave-per-row kc=1 R=4", "wave-per-row kc=2 R=2", "c8n not a multiple of 64", "one live row in the last wave"}
    assert not need - tags, f"no case for {sorted(need - tags)}"
    assert all(not R.ln_plan(lib, rows, Cc, 1)["g8"] for rows, Cc, _ in R.LN32_CASES)
