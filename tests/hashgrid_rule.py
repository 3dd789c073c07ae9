"""The definition of the hash-grid encoding: numpy restatements in binary32 of `ctx_hashgrid_fwd` and of the integer
accumulator of `ctx_hashgrid_bwd`, the same forward in float64 / differentiable torch, the field's MLP in plain torch with the restated
`grad_emb` formula, and the inputs the CPU and the GPU tests share.
Not a test module: tests/test_hashgrid_cpu.py and tests/test_hashgrid_gpu.py import it."""
import math
import numpy as np
import torch

f32 = np.float32
P1, P2 = np.uint32(2654435761), np.uint32(805459861)


def resolutions(n_levels, base_res, max_res):
    """res[l] = floor(N_min * exp(l * ln(N_max / N_min) / (Lv - 1))) in float64 (N_min when Lv = 1): integers for the ABI."""
    if n_levels == 1:
        return np.array([int(base_res)], np.int32)
    b = math.log(max_res / base_res) / (n_levels - 1)
    return np.array([int(math.floor(base_res * math.exp(l * b))) for l in range(n_levels)], np.int32)


def is_dense(res, log2T):
    return (int(res) + 1) ** 3 <= (1 << log2T)


def hash_index(gx, gy, gz, log2T):
    """(gx ^ gy * 2654435761 ^ gz * 805459861) & (T - 1) in uint32 arithmetic with wrap."""
    gx, gy, gz = (np.asarray(g).astype(np.uint32) for g in (gx, gy, gz))
    with np.errstate(over='ignore'):
        return (gx ^ (gy * P1) ^ (gz * P2)) & np.uint32((1 << log2T) - 1)


def positions_np(pts, lo, hi, res):
    """(i int64 [n,3], pos float32 [n,3]) of one level, in binary32: x = (p - lo) / (hi - lo), clamped to [0, 1] by fmaxf / fminf (a NaN
    yields the other operand: 0), pos = x * (float)res, i = min((int)floorf(pos), res - 1)."""
    pts = np.asarray(pts, f32).reshape(-1, 3)
    lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
    with np.errstate(all='ignore'):
        x = (pts - lo) / (hi - lo)
        pos = np.fmin(np.fmax(x, f32(0)), f32(1)) * f32(res)
    return np.minimum(np.floor(pos).astype(np.int64), res - 1), pos


def cell_np(pts, lo, hi, res, log2T):
    """One level: (idx int64 [n,8], w float32 [n,8]) of the 8 corners c = cx + 2 cy + 4 cz, every operation binary32 in the kernel's order."""
    i, pos = positions_np(pts, lo, hi, res)
    w = pos - i.astype(f32)
    side = int(res) + 1
    idx = np.empty((i.shape[0], 8), np.int64)
    wc = np.empty((i.shape[0], 8), f32)
    one = f32(1)
    for c in range(8):
        b = (c & 1, (c >> 1) & 1, (c >> 2) & 1)
        g = [i[:, a] + b[a] for a in range(3)]
        if is_dense(res, log2T):
            idx[:, c] = g[0] + side * (g[1] + side * g[2])
        else:
            idx[:, c] = hash_index(g[0], g[1], g[2], log2T).astype(np.int64)
        s = [w[:, a] if b[a] else one - w[:, a] for a in range(3)]
        wc[:, c] = (s[0] * s[1]) * s[2]
    return idx, wc


def forward_np(pts, table, lo, hi, res, log2T):
    """emb float32 [n, Lv*F]: per feature the left-to-right sum over the corners of w_c * t_c, from 0."""
    table = np.asarray(table, f32)
    Lv, T, F = table.shape
    n = np.asarray(pts).reshape(-1, 3).shape[0]
    emb = np.zeros((n, Lv * F), f32)
    for l in range(Lv):
        idx, w = cell_np(pts, lo, hi, int(res[l]), log2T)
        acc = np.zeros((n, F), f32)
        for c in range(8):
            acc = acc + w[:, c:c + 1] * table[l, idx[:, c]]
        emb[:, l * F:(l + 1) * F] = acc
    return emb


def forward_f64(pts, table, lo, hi, res, log2T):
    """Float64 trilinear interpolation of the same table at the rule's binary32 positions: weights, products and sums in float64."""
    table = np.asarray(table, np.float64)
    Lv, T, F = table.shape
    n = np.asarray(pts).reshape(-1, 3).shape[0]
    emb = np.zeros((n, Lv * F))
    for l in range(Lv):
        r = int(res[l])
        i, pos = positions_np(pts, lo, hi, r)
        w = pos.astype(np.float64) - i
        for c in range(8):
            b = (c & 1, (c >> 1) & 1, (c >> 2) & 1)
            g = [i[:, a] + b[a] for a in range(3)]
            if is_dense(r, log2T):
                k = g[0] + (r + 1) * (g[1] + (r + 1) * g[2])
            else:
                k = hash_index(g[0], g[1], g[2], log2T).astype(np.int64)
            wc = np.prod([w[:, a] if b[a] else 1 - w[:, a] for a in range(3)], 0)
            emb[:, l * F:(l + 1) * F] += wc[:, None] * table[l, k]
    return emb


def ceil_log2_8n(n):
    c = 3
    while (1 << (c - 3)) < n:
        c += 1
    return c


def backward_np(pts, g_emb, lo, hi, res, log2T, F, as_double=False):
    """g_table float32 [Lv, T, F] by the integer accumulator: m = max|g_emb|, 2^x the smallest power of two above m, E = 62 - ceil(log2(8n));
    each float product w_c * g is scaled by 2^(E-x) in double, rounded to nearest even into int64 and added; g_table = (float)((double)acc *
    2^(x-E)).  m = 0: zeros; a non-finite g_emb: all NaN.  as_double=True returns the double before that last rounding to float32."""
    g_emb = np.asarray(g_emb, f32)
    n, Lv, T = g_emb.shape[0], len(res), 1 << log2T
    if not np.all(np.isfinite(g_emb)):
        return np.full((Lv, T, F), np.nan, f32)
    m = float(np.max(np.abs(g_emb))) if n else 0.0
    if m == 0.0:
        return np.zeros((Lv, T, F), f32)
    x = math.frexp(m)[1]                                       # m = f * 2^x, f in [0.5, 1): 2^(x-1) <= m < 2^x
    E = 62 - ceil_log2_8n(n)
    acc = np.zeros((Lv, T, F), np.int64)
    for l in range(Lv):
        idx, w = cell_np(pts, lo, hi, int(res[l]), log2T)
        for c in range(8):
            prod = w[:, c:c + 1] * g_emb[:, l * F:(l + 1) * F]                       # float32: one rounding
            q = np.rint(np.ldexp(prod.astype(np.float64), E - x)).astype(np.int64)   # rint: nearest even
            for f in range(F):
                np.add.at(acc[l, :, f], idx[:, c], q[:, f])
    out = np.ldexp(acc.astype(np.float64), x - E)
    return out if as_double else out.astype(f32)


def forward_torch(pts, table, lo, hi, res, log2T, dtype=torch.float64):
    """The forward as a torch expression differentiable in `table` (a torch tensor [Lv, T, F] of `dtype`): cells and weights from the
    binary32 rule, products and sums in `dtype`."""
    Lv, T, F = table.shape
    cols = []
    for l in range(Lv):
        idx, w = cell_np(pts, lo, hi, int(res[l]), log2T)
        idx_t, w_t = torch.from_numpy(idx), torch.from_numpy(w).to(dtype)
        cols.append((w_t[:, :, None] * table[l][idx_t]).sum(1))
    return torch.cat(cols, -1)


# ---- the field's MLP (NeRF2D with one skip) in plain torch, and the restated input gradient -----------------------------------
def mlp_torch(emb, params, skip):
    """params = [w0, b0, ..., w_D, b_D] in nn.Linear layout; layer skip + 1 reads cat([emb, h])."""
    D = len(params) // 2 - 1
    h = emb
    for i in range(D):
        h = torch.relu(torch.nn.functional.linear(h, params[2 * i], params[2 * i + 1]))
        if i == skip and i + 1 < D:
            h = torch.cat([emb, h], -1)
    return torch.nn.functional.linear(h, params[2 * D], params[2 * D + 1])


def mlp_dz_torch(emb, params, skip, g_raw):
    """dZ_i = d loss / d (pre-activation of hidden layer i) for loss = sum(raw * g_raw), by autograd."""
    D = len(params) // 2 - 1
    zs = []
    h = emb
    for i in range(D):
        z = torch.nn.functional.linear(h, params[2 * i], params[2 * i + 1])
        z.retain_grad()
        zs.append(z)
        h = torch.relu(z)
        if i == skip and i + 1 < D:
            h = torch.cat([emb, h], -1)
    raw = torch.nn.functional.linear(h, params[2 * D], params[2 * D + 1])
    (raw * g_raw).sum().backward()
    return [z.grad for z in zs]


def grad_emb_formula(dz, params, skip, input_ch):
    """grad_emb[n, e] = sum_j dz[0][n, j] W_0[j, e] + sum_j dz[skip+1][n, j] W_{skip+1}[j, e], e < input_ch."""
    return dz[0] @ params[0][:, :input_ch] + dz[skip + 1] @ params[2 * (skip + 1)][:, :input_ch]


def make_params(D, W, input_ch, output_ch, skip, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    ps = []
    for i in range(D):
        kin = input_ch if i == 0 else (W + input_ch if i == skip + 1 else W)
        ps += [torch.randn(W, kin, generator=g) * math.sqrt(2.0 / kin), torch.randn(W, generator=g) * 0.1]
    ps += [torch.randn(output_ch, W, generator=g) * math.sqrt(2.0 / W), torch.randn(output_ch, generator=g) * 0.1]
    return [p.to(dtype) for p in ps]


# ---- shared inputs -----------------------------------------------------------------------------------------------------------------
BOX_LO, BOX_HI = (-1.0, -0.5, 0.25), (1.0, 1.5, 0.75)          # anisotropic
GRID_CASES = [(1, 1, 4), (4, 2, 6), (16, 2, 12), (16, 4, 10)]   # (Lv, F, log2T)
N_CASES = [1, 63, 64, 65, 300]


def case_points(n, lo, hi, res, seed):
    """n points: uniform in a box 10 % larger than lo .. hi, then (as n allows) overwritten with the box corners and faces, nodes of the
    finest level, points outside, and NaN / inf rows."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
    ext = hi - lo
    p = (lo - 0.05 * ext + rng.random((n, 3)) * 1.1 * ext).astype(f32)
    r = int(res[-1])
    special = [lo, hi, np.array([lo[0], hi[1], 0.5 * (lo[2] + hi[2])], f32),
               (lo + ext * (np.array([1, 2, 1], f32) / f32(r))).astype(f32), (lo + ext * f32(0.5)).astype(f32),
               lo - 3 * ext, hi + 7 * ext, np.array([np.nan, 0, 0.5], f32), np.array([np.inf, -np.inf, np.nan], f32),
               np.array([0, np.inf, 0.5], f32)]
    for k, s in enumerate(special):
        if 2 * k + 1 < n:
            p[2 * k + 1] = s
    return p


def case_table(Lv, F, log2T, seed):
    return np.random.default_rng(seed).standard_normal((Lv, 1 << log2T, F)).astype(f32)
