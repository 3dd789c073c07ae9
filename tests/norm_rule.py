"""The definition of the norm kernels (csrc/norm.hip): GroupNorm(+SiLU), GroupNorm of a two-source concat, LayerNorm and the
GroupNorm backward.  For each the float64 reference computed from the same fp16-rounded (or fp32) x, gamma and beta, the per-element
error bound, the input makers and the case lists that the CPU and the GPU tests share.
Not a test module: tests/test_norm_cpu.py and tests/test_norm_gpu.py import it.

The comparator (u16 = 2^-11, the unit roundoff of fp16).  With x^ = (x - mean64) rstd64, L = 1.1 (the largest slope of SiLU; 1 without
it) and xmax the largest |x| of the group (of the row, for LayerNorm):

    |y - y64| <= 2^-11 |y64| + L |gamma| (2^-12 |x^| + 2^-22 rstd64 xmax) + 1e-7

  2^-11 |y64|            the output's own fp16 rounding
  L |gamma| 2^-12 |x^|   a statistics error (relative error of rstd) of at most half of that rounding
  L |gamma| 2^-22 ...    the fp32 rounding of the mean and of x * sa + sh, which no fp32 scheme avoids: three or four roundings of
                         2^-24 at the size of rstd |x|.  The only term that matters for a constant group.

The backward.  dx = rstd (du - c1 - x^ c2) + add with u = gamma x^ + beta, du = dy silu'(u) gamma, c1 = mean du, c2 = mean du x^.  The
same two perturbations, rstd by the relative eps = 2^-12 and x^ by eta = eps |x^| + 2^-22 rstd xmax, pushed through the formula to
first order:
    |d u| <= |gamma| eta,  |d du| <= M |dy gamma| |d u| (M = max |silu''| = 0.5; 0 without SiLU),
    |d c1| <= mean |d du|,  |d c2| <= mean (|d du| |x^| + |du| eta),
    |dx - dx64| <= 2^-11 |dx64| + eps |dx64 - add| + rstd (|d du| + |d c1| + eta |c2| + |x^| |d c2|) + 2^-20 T + 1e-7
with T = rstd (|du| + |c1| + |x^ c2|) + |add|: the first term is the output's rounding, 2^-20 T the fp32 sums and __expf (as
tests/vae_train_rule.py counts them)."""
import numpy as np
import torch
import torch.nn.functional as F

import vae_train_rule as VR

f64 = torch.float64
U11, U12, U20, U22 = 2.0 ** -11, 2.0 ** -12, 2.0 ** -20, 2.0 ** -22
GN_EPS = 1e-5
LN_EPS = 1e-5
SILU_SLOPE = 1.1
GN_AU = 6                       # pixels per lane of the apply pass
GN_FU = 12                      # pixels per lane of the one-kernel form
GN_FOLD = 8                     # partial slots per lane and trip of the apply pass's fold

# ---- input makers -------------------------------------------------------------------------------------------------------------------
# kind -> (mean / sigma, sigma); 'const' and 'outlier' are made by hand below
KINDS = {"ordinary": (0.25, 2.0), "m30": (30.0, 1.0), "m300": (300.0, 1.0), "m1000": (1000.0, 1.0), "mneg1000": (-1000.0, 1.0),
         "m1e4": (1e4, 1.0)}
KINDS16 = ("ordinary", "m30", "m300", "m1000", "mneg1000", "const", "outlier")
KINDS32 = ("m1e4",) + KINDS16                          # first: the smallest fp32 case has four groups
SHIFTED = ("m300", "m1000", "mneg1000", "m1e4")        # where sumsq/n - mean^2 of the raw fp32 sums fails
CONST_VALUE = 7.25


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def group_kind(kinds, b, g, G):
    """groups of one sample get different kinds, and the samples start at different ones"""
    return kinds[(b * (G + 1) + g) % len(kinds)]


def make_group(kind, HW, cg, gen, odd):
    """one (sample, group) slab [HW, cg], float32, not yet rounded"""
    if kind == "const":
        return torch.full((HW, cg), CONST_VALUE)
    z = torch.randn(HW, cg, generator=gen)
    if kind == "outlier":                              # ordinary, one channel column 50 sigma away: the first or the last channel
        r, s = KINDS["ordinary"]
        v = z * s + r * s
        v[:, 0 if odd else cg - 1] += 50.0 * s
        return v
    r, s = KINDS[kind]
    return z * s + r * s


def gn_input(B, HW, C, G, kinds=KINDS16, x32=False, seed=0):
    """-> x [B,HW,C] f16 (f32 when x32), the kind of every (sample, group) [B][G]"""
    gen = _gen(9000 + seed + HW + 3 * C + 7 * G)
    cg = C // G
    x = torch.empty(B, HW, G, cg)
    names = [[group_kind(kinds, b, g, G) for g in range(G)] for b in range(B)]
    for b in range(B):
        for g in range(G):
            x[b, :, g] = make_group(names[b][g], HW, cg, gen, g & 1)
    x = x.reshape(B, HW, C)
    return (x if x32 else x.half()), names


def affine(C, seed=0):
    g = _gen(9500 + seed + C)
    return (torch.randn(C, generator=g) * 0.5 + 1.0).half(), (torch.randn(C, generator=g) * 0.5).half()


def ln_input(rows, C, x32=False, seed=0):
    """rows at mean / sigma 0.25, 30, 300, 1000, -1000 (, 1e4) in turn, one constant row"""
    kinds = tuple(k for k in (KINDS32 if x32 else KINDS16) if k != "outlier")
    gen = _gen(9700 + seed + C)
    x = torch.randn(rows, C, generator=gen)
    names = [kinds[r % len(kinds)] for r in range(rows)]
    scale = torch.tensor([0.0 if k == "const" else KINDS[k][1] for k in names])
    shift = torch.tensor([CONST_VALUE if k == "const" else KINDS[k][0] * KINDS[k][1] for k in names])
    x = x * scale[:, None] + shift[:, None]
    return (x if x32 else x.half()), names


# ---- float64 references and the comparator -------------------------------------------------------------------------------------------
def gn_ref(x, gamma, beta, G, eps=GN_EPS, silu=0):
    """x [B,HW,C] -> (y64, bound) [B,HW,C] float64"""
    B, HW, C = x.shape
    xg = x.to(f64).reshape(B, HW, G, C // G)
    mean = xg.mean((1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(xg.var((1, 3), unbiased=False, keepdim=True) + eps)
    xh = (xg - mean) * rstd
    ga, be = gamma.to(f64).reshape(1, 1, G, -1), beta.to(f64).reshape(1, 1, G, -1)
    y = xh * ga + be
    if silu:
        y = y * torch.sigmoid(y)
    L = SILU_SLOPE if silu else 1.0
    xmax = xg.abs().amax((1, 3), keepdim=True)
    bound = U11 * y.abs() + L * ga.abs() * (U12 * xh.abs() + U22 * rstd * xmax) + 1e-7
    return y.reshape(B, HW, C), bound.reshape(B, HW, C)


def gn2_ref(xa, xb, gamma, beta, G, eps=GN_EPS, silu=0):
    """GroupNorm of the channel concat [xa ; xb]"""
    return gn_ref(torch.cat([xa, xb], -1), gamma, beta, G, eps, silu)


def ln_ref(x, gamma, beta, eps=LN_EPS):
    """x [rows,C]: a row is one group of one pixel"""
    rows, C = x.shape
    y, b = gn_ref(x.reshape(rows, 1, C), gamma, beta, 1, eps, 0)
    return y.reshape(rows, C), b.reshape(rows, C)


def gn_bwd_ref(x, dy, gamma, beta, add, G, silu, eps=VR.GN_EPS):
    """-> (want, bound) [B,HW,C] float64; want by autograd (vae_train_rule.gn_bwd_ref's), the bound of this file's docstring"""
    B, HW, C = x.shape
    want, _ = VR.gn_bwd_ref(x, dy, gamma, beta, add, G, silu)
    rstd, xh, du, c1, c2 = VR.gn_bwd_terms(x, dy, gamma, beta, G, silu)
    ga = gamma.to(f64).reshape(1, 1, G, -1)
    xmax = x.to(f64).reshape(B, HW, G, -1).abs().amax((1, 3), keepdim=True)
    eta = U12 * xh.abs() + U22 * rstd * xmax
    d_du = (0.5 if silu else 0.0) * (dy.to(f64).reshape(B, HW, G, -1) * ga).abs() * ga.abs() * eta
    d_c1 = d_du.mean((1, 3), keepdim=True)
    d_c2 = (d_du * xh.abs() + du.abs() * eta).mean((1, 3), keepdim=True)
    a = add.to(f64) if add is not None else torch.zeros(B, HW, C, dtype=f64)
    T = (rstd * (du.abs() + c1.abs() + (xh * c2).abs())).reshape(B, HW, C) + a.abs()
    pert = (rstd * (d_du + d_c1 + eta * c2.abs() + xh.abs() * d_c2)).reshape(B, HW, C)
    return want, U11 * want.abs() + U12 * (want - a).abs() + pert + U20 * T + 1e-7


def ratios(got, want, bound):
    """|got - want| / bound per element (0 / 0 counts as 0, a non-finite value as inf)"""
    err = (got.to(f64) - want).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))


def worst(got, want, bound):
    """-> (the worst element as a fraction of its bound, its flat index)"""
    r = ratios(got, want, bound)
    i = int(r.argmax())
    return float(r.flatten()[i]), i


def per_group_worst(got, want, bound, G):
    """[B][G]: the worst fraction inside every (sample, group)"""
    B, HW, C = want.shape
    return ratios(got, want, bound).reshape(B, HW, G, C // G).amax((1, 3))


def assert_within(got, want, bound, what):
    assert tuple(got.shape) == tuple(want.shape), f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    r, i = worst(got, want, bound)
    print(f"{what}: worst element / bound {r:.3f}")
    assert r <= 1.0, (f"{what}: element {i} is at {r:.3f} of its bound (got {float(got.flatten()[i]):.6g}, want "
                      f"{float(want.flatten()[i]):.6g}, bound {float(bound.flatten()[i]):.3g})")
    return r


# ---- fp32 emulations of the statistics: they judge the comparator, not the kernels ----------------------------------------------------
def _sum32(v):
    """fp32 sum of a flat array as a kernel forms it: sequential chains of 24, then pairwise (numpy's float32 sum)"""
    v = np.asarray(v, np.float32).ravel()
    pad = (-len(v)) % 24
    v = np.concatenate([v, np.zeros(pad, np.float32)]).reshape(-1, 24)
    acc = np.zeros(len(v), np.float32)
    for k in range(24):
        acc = acc + v[:, k]
    return np.sum(acc, dtype=np.float32)


def emu_stats(v, mode):
    """(mean, rstd^-2 - eps) in fp32 of a flat array.  'two_pass': mean, then sum (x - mean)^2; 'one_pass': sumsq / n - mean^2"""
    v = np.asarray(v, np.float32).ravel()
    n = np.float32(len(v))
    mean = _sum32(v) / n
    if mode == "two_pass":
        d = v - mean
        return mean, _sum32(d * d) / n
    return mean, np.maximum(_sum32(v * v) / n - mean * mean, np.float32(0))


def emu_gn(x, gamma, beta, G, eps, silu, mode, round16=True):
    """GroupNorm(+SiLU) in fp32 with the kernels' rounding points: sa = rstd gamma, sh = beta - mean sa, y = (f16)act(x sa + sh);
    round16 False: the fp32 value in front of the last rounding"""
    B, HW, C = x.shape
    cg = C // G
    xf = x.float().numpy().reshape(B, HW, G, cg)
    ga, be = gamma.float().numpy().reshape(G, cg), beta.float().numpy().reshape(G, cg)
    out = np.empty_like(xf)
    for b in range(B):
        for g in range(G):
            mean, var = emu_stats(xf[b, :, g], mode)
            sa = (np.float32(1) / np.sqrt(var + np.float32(eps), dtype=np.float32)) * ga[g]
            # both are one fused multiply-add in the kernels (norm.hip is compiled with contraction on): the product of two floats is
            # exact in float64, so rounding the float64 sum once is the fma
            sh = (be[g].astype(np.float64) - np.float64(mean) * sa.astype(np.float64)).astype(np.float32)
            t = (xf[b, :, g].astype(np.float64) * sa.astype(np.float64) + sh.astype(np.float64)).astype(np.float32)
            if silu:
                with np.errstate(over="ignore"):                       # a wrong rstd makes t huge: exp -> inf, t / inf = -0
                    t = t / (np.float32(1) + np.exp(-t, dtype=np.float32))
            out[b, :, g] = t
    out = torch.from_numpy(out.reshape(B, HW, C))
    return out.half() if round16 else out


# ---- the launch plans as the tests read them (ctx_groupnorm_plan / ctx_layernorm_plan) -------------------------------------------------
GN_PLAN_FIELDS = ("one", "plf", "thr", "PL", "threads", "NS", "na", "lds", "apl", "athreads", "nb", "lds_optin")
E_ARG = -1


def gn_plan(lib, B, HW, C, G, x32=0, Ca=0):
    """-> dict of GN_PLAN_FIELDS, or None where the launcher refuses"""
    import ctypes
    out = (ctypes.c_int32 * 12)()
    rc = lib.ctx_groupnorm_plan(B, HW, C, G, x32, Ca, ctypes.cast(out, ctypes.c_void_p))
    if rc != 0:
        assert rc == E_ARG
        return None
    return dict(zip(GN_PLAN_FIELDS, out))


def ln_plan(lib, rows, C, x32=0):
    """-> dict g8, KC, R, blocks, or None"""
    import ctypes
    out = (ctypes.c_int64 * 4)()
    rc = lib.ctx_layernorm_plan(rows, C, x32, ctypes.cast(out, ctypes.c_void_p))
    if rc != 0:
        assert rc == E_ARG
        return None
    return dict(zip(("g8", "KC", "R", "blocks"), out))


def fold_trips(NS, G):
    """trips of k_gn_apply's fold of NS slots: 256 / G lanes per group (at most a wave), GN_FOLD slots per lane and trip"""
    lpg = min(256 // G, 64)
    return -(-NS // (GN_FOLD * lpg))


def gn_classes(p, B, HW, C, G, Ca=0):
    """the classes of the launch plan that one GroupNorm case is there for"""
    cg, c8n = C // G, C // 8
    tags = {f"G={G}"}
    if Ca:
        tags.add("two sources, aligned" if Ca % cg == 0 else "two sources, a group straddles Ca")
    if p["one"]:
        tags.add(f"one-kernel cpg={cg // 8}")
        if HW == GN_FU * p["plf"]:
            tags.add("one-kernel at HW = 12 plf")
        return tags
    tags |= {f"two-pass c8n={c8n}", f"two-pass cg={cg}", "na>1" if p["na"] > 1 else "na=1", f"fold trips={fold_trips(p['NS'], G)}"}
    if p["threads"] != c8n * p["PL"]:
        tags.add("stats block rounded up to whole waves")
    if c8n * p["PL"] < 8:
        tags.add("fewer than 8 working stats lanes")
    if p["lds"] > 80 * 1024:
        tags.add("stats LDS above 80 KiB")
    if cg % 8 == 0 and C // G // 8 <= 512 and HW == GN_FU * (512 // (cg // 8)) + 1:
        tags.add("two-pass at HW = 12 plf + 1")
    NS, per = p["NS"], -(-HW // p["NS"])
    if NS == 1:
        tags.add("NS=1")
    elif (NS - 1) * per >= HW:
        tags.add("empty last split")
    elif NS * per > HW:
        tags.add("ragged last split")
    if HW // p["PL"] > NS:                                         # the split count is `want`, not the pixels
        tags.add(f"want from B={B}")
    return tags


def ln_classes(p, rows, C):
    c8n = C // 8
    tags = {f"g8 KC={p['KC']}" if p["g8"] else f"wave-per-row kc={p['KC']} R={p['R']}"}
    if c8n % 64:
        tags.add("c8n not a multiple of 64")
    if rows % p["R"] == 1 and rows > 1:
        tags.add("one live row in the last wave")
    return tags


# ---- case lists ----------------------------------------------------------------------------------------------------------------------
# A. ctx_groupnorm_f16: (B, HW, C, G), what the case is there for
GN_CASES = [
    (2, 37, 64, 8, "one-kernel, one chunk per pixel"),
    (1, 2040, 48, 2, "one-kernel cpg 3 at HW = 12 plf"),
    (1, 2041, 48, 2, "the two-pass form one pixel later, cg 24"),
    (2, 100, 80, 2, "one-kernel cpg 5"),
    (1, 77, 160, 2, "one-kernel cpg 10"),
    (1, 50, 128, 1, "one-kernel cpg 16, G 1"),
    (1, 12, 4096, 1, "one-kernel cpg 512, one pixel lane"),
    (2, 5, 8, 2, "two-pass c8n 1, cg 4, NS 1: 5 working lanes in a block of 64"),
    (1, 1, 56, 8, "two-pass cg 7, one pixel: 7 working lanes"),
    (1, 8192, 64, 64, "two-pass c8n 8, cg 1, G 64, na 16, NS 64 from B = 1: two fold trips"),
    (2, 64, 64, 32, "two-pass cg 2"),
    (2, 37, 48, 8, "two-pass cg 6"),
    (2, 144, 320, 32, "two-pass c8n 40, cg 10, ragged last split"),
    (12, 430, 320, 32, "NS 16 from B = 12"),
    (1, 1650, 320, 32, "NS 64 from B = 1"),
    (1, 40, 768, 64, "two-pass c8n 96, cg 12"),
    (1, 30, 640, 32, "two-pass cg 20"),
    (1, 70, 120, 2, "two-pass cg 60"),
    (1, 613, 80, 1, "two-pass cg 80 at HW = 12 plf + 1"),
    (1, 13, 1600, 32, "two-pass c8n 200, cg 50"),
    (1, 13, 2560, 1, "two-pass c8n 320: 80 KiB of LDS, na 1"),
    (1, 13, 4096, 1, "two-pass c8n 512: 96 KiB of LDS, empty last split"),
]
# B. the fp32-input kernels, one case of every form
GN32_CASES = [(2, 37, 64, 8, "one-kernel"), (2, 144, 320, 32, "two-pass"), (2, 5, 8, 2, "two-pass, block rounded up")]
LN32_CASES = [(9, 320, "wave-per-row kc 1 (fp32 input never takes the 8-lane form)"), (3, 1032, "kc 3"), (8197, 72, "kc 1, R 4")]
# C. ctx_groupnorm2_f16: (B, HW, C, G, Ca)
GN2_CASES = [
    (2, 50, 128, 2, 64, "one-kernel, Ca on a group boundary"),
    (2, 50, 128, 2, 40, "one-kernel, a group straddles Ca"),
    (1, 40, 96, 8, 48, "two-pass cg 12, Ca on a group boundary"),
    (1, 40, 96, 8, 40, "two-pass cg 12, a group straddles Ca"),
]
# D. ctx_groupnorm_apply_f16 on hand-made partials: (B, HW, C, G, NS)
APPLY_CASES = [(2, 150, 64, G, NS) for G in (1, 64) for NS in (1, 7, 33, 128)]
# E. ctx_layernorm_f16: (rows, C)
LN_CASES = [(65, 64 * k, f"8 lanes per row, KC {k}, one live row in the last wave") for k in range(1, 11)] + [
    (63, 64, "fewer than 64 rows: wave-per-row kc 1"),
    (5, 72, "kc 1, c8n 9"),
    (8197, 72, "kc 1, R 4, one live row in the last wave"),
    (7, 520, "kc 2, c8n 65"),
    (8193, 520, "kc 2, R 2, one live row in the last wave"),
    (3, 1032, "kc 3"),
    (2, 1544, "kc 4, c8n 193"),
    (2, 2048, "kc 4, every lane full"),
]
# F. ctx_groupnorm_bwd_f16: three shapes of vae_train_rule.GN_CASES (B, HW, C, G, silu, add), x at these mean / sigma
BWD_CASES = [(2, 64, 64, 32, 1, False), (3, 100, 512, 32, 0, True), (1, 289, 512, 32, 1, True)]
BWD_RATIOS = (0.25, 300.0, 1000.0)


def bwd_inputs(case, ratio):
    """vae_train_rule.gn_inputs with x = randn + ratio (sigma 1), or randn * 2 + 0.5 for the ordinary 0.25"""
    B, HW, C, G, silu, add = case
    x, dy, gamma, beta, a = VR.gn_inputs((B, HW, C, G, silu, add, False))
    if ratio != 0.25:
        x = (torch.randn(B, HW, C, generator=_gen(9900 + HW + C)) + ratio).half()
    return x, dy, gamma, beta, a


def hand_partials(x, G, NS):
    """[B][NS][G][2] fp32: float64 (sum, sum of squares) of slot k's pixels k per .. (k + 1) per, per = ceil(HW / NS), rounded to fp32"""
    B, HW, C = x.shape
    per = -(-HW // NS)
    xg = x.to(f64).reshape(B, HW, G, C // G)
    part = torch.zeros(B, NS, G, 2, dtype=f64)
    for k in range(NS):
        sl = xg[:, k * per:min(HW, (k + 1) * per)]
        part[:, k, :, 0] = sl.sum((1, 3))
        part[:, k, :, 1] = (sl * sl).sum((1, 3))
    return part.float()
