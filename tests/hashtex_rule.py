"""The definition of the texture field's 2-D hash grid: numpy restatements in binary32 of `ctx_hashtex_fwd` and of the
integer accumulator of `ctx_hashtex_bwd`, the same forward in float64 / differentiable torch, the head in float64, the whole field
(cells, `hashgrid_rule.mlp_torch`, the tanh head) as a torch expression, and the inputs the CPU and the GPU tests share.
Not a test module: tests/test_hashtex_cpu.py and tests/test_hashtex_gpu.py import it."""
import math
import numpy as np
import torch

import hashgrid_rule as HG

f32 = np.float32
P1 = np.uint32(2654435761)
resolutions = HG.resolutions


def is_dense(res, log2T):
    return (int(res) + 1) ** 2 <= (1 << log2T)


def hash_index(gx, gy, log2T):
    """(gx ^ gy * 2654435761) & (T - 1) in uint32 arithmetic with wrap."""
    gx, gy = (np.asarray(g).astype(np.uint32) for g in (gx, gy))
    with np.errstate(over='ignore'):
        return (gx ^ (gy * P1)) & np.uint32((1 << log2T) - 1)


# ---- the three ways to name the rows -------------------------------------------------------------------------------------------------
def node_uv(grid, nodes):
    """uv float32 [n,2] of nodes i*grid + j of the grid x grid atlas: torch.linspace(0, 1, grid), in binary32: step = 1/(grid-1);
    u = j < grid/2 ? j*step : fmaf(-(grid-1-j), step, 1), v the same from i.  The second half is ONE rounding of 1 - (grid-1-j)*step: that is
    what torch.linspace gives and what `k_uvmlp_fwd`, which is compiled with contraction, computes from `1.0f - (float)(res-1-j) * step`.
    (The product of two binary32 numbers and, at these sizes, its difference from 1 are exact in float64, so the float64 expression rounded
    once is the fused operation.)"""
    nodes = np.asarray(nodes, np.int64)
    step = f32(1) / f32(grid - 1)

    def axis(k):
        fused = (1.0 - (grid - 1 - k).astype(np.float64) * np.float64(step)).astype(f32)
        return np.where(k < grid // 2, k.astype(f32) * step, fused).astype(f32)
    return np.stack([axis(nodes % grid), axis(nodes // grid)], -1)


def rows_uv(uv=None, idx=None, grid=0):
    """(uv float32 [n,2], live bool [n]) of the rows: points, the whole atlas (grid alone) or a texel list (idx, grid).  A list entry
    outside [0, grid^2) is not live: a zero row that takes no part in the backward."""
    if uv is not None:
        assert idx is None and grid == 0
        uv = np.asarray(uv, f32).reshape(-1, 2)
        return uv, np.ones(uv.shape[0], bool)
    assert grid >= 2
    if idx is None:
        return node_uv(grid, np.arange(grid * grid)), np.ones(grid * grid, bool)
    idx = np.asarray(idx, np.int64)
    live = (idx >= 0) & (idx < grid * grid)
    return node_uv(grid, np.where(live, idx, 0)), live


# ---- one level ---------------------------------------------------------------------------------------------------------------------------
def positions_np(uv, res):
    """(i int64 [n,2], pos float32 [n,2]) in binary32: x = fminf(fmaxf(p, 0), 1) (a NaN yields the other operand: 0), pos = x * (float)res,
    i = min((int)floorf(pos), res - 1)."""
    uv = np.asarray(uv, f32).reshape(-1, 2)
    with np.errstate(all='ignore'):
        pos = np.fmin(np.fmax(uv, f32(0)), f32(1)) * f32(res)
    return np.minimum(np.floor(pos).astype(np.int64), res - 1), pos


def cell_np(uv, res, log2T, mutate=None):
    """(idx int64 [n,4], w float32 [n,4]) of the 4 corners c = cx + 2 cy, every operation binary32 in the kernel's order.
    mutate: a deliberately wrong rule for the tests ('swap_axes', 'dense3d')."""
    uv = np.asarray(uv, f32).reshape(-1, 2)
    if mutate == 'swap_axes':
        uv = uv[:, ::-1]
    i, pos = positions_np(uv, res)
    w = pos - i.astype(f32)
    side = int(res) + 1
    idx = np.empty((i.shape[0], 4), np.int64)
    wc = np.empty((i.shape[0], 4), f32)
    one = f32(1)
    for c in range(4):
        b = (c & 1, (c >> 1) & 1)
        gx, gy = i[:, 0] + b[0], i[:, 1] + b[1]
        if is_dense(res, log2T):
            idx[:, c] = gx + side * gy if mutate != 'dense3d' else (gx + side * side * gy) & ((1 << log2T) - 1)
        else:
            idx[:, c] = hash_index(gx, gy, log2T).astype(np.int64)
        sx = w[:, 0] if b[0] else one - w[:, 0]
        sy = w[:, 1] if b[1] else one - w[:, 1]
        wc[:, c] = sx * sy
    return idx, wc


# ---- forward -------------------------------------------------------------------------------------------------------------------------------
def forward_np(table, res, log2T, uv=None, idx=None, grid=0):
    """emb float32 [n, Lv*F]: per feature the left-to-right sum over the corners of w_c * t_c, from 0; a row that is not live is zero."""
    table = np.asarray(table, f32)
    Lv, T, F = table.shape
    p, live = rows_uv(uv, idx, grid)
    n = p.shape[0]
    emb = np.zeros((n, Lv * F), f32)
    for l in range(Lv):
        k, w = cell_np(p, int(res[l]), log2T)
        acc = np.zeros((n, F), f32)
        for c in range(4):
            acc = acc + w[:, c:c + 1] * table[l, k[:, c]]
        emb[:, l * F:(l + 1) * F] = acc
    emb[~live] = 0
    return emb


def forward_f64(table, res, log2T, uv=None, idx=None, grid=0):
    """(emb, mag) in float64 at the rule's binary32 positions: weights, products and sums in float64; mag = sum_c |w_c t_c|, the scale of
    the rounding bound."""
    table = np.asarray(table, np.float64)
    Lv, T, F = table.shape
    p, live = rows_uv(uv, idx, grid)
    n = p.shape[0]
    emb, mag = np.zeros((n, Lv * F)), np.zeros((n, Lv * F))
    for l in range(Lv):
        r = int(res[l])
        i, pos = positions_np(p, r)
        w = pos.astype(np.float64) - i
        for c in range(4):
            b = (c & 1, (c >> 1) & 1)
            gx, gy = i[:, 0] + b[0], i[:, 1] + b[1]
            k = gx + (r + 1) * gy if is_dense(r, log2T) else hash_index(gx, gy, log2T).astype(np.int64)
            wc = (w[:, 0] if b[0] else 1 - w[:, 0]) * (w[:, 1] if b[1] else 1 - w[:, 1])
            term = wc[:, None] * table[l, k]
            emb[:, l * F:(l + 1) * F] += term
            mag[:, l * F:(l + 1) * F] += np.abs(term)
    emb[~live] = 0
    mag[~live] = 0
    return emb, mag


def forward_torch(table, res, log2T, uv=None, idx=None, grid=0, dtype=torch.float64):
    """The forward as a torch expression differentiable in `table` (a torch tensor [Lv, T, F] of `dtype`): cells and weights from the
    binary32 rule, products and sums in `dtype`."""
    p, live = rows_uv(uv, idx, grid)
    live_t = torch.from_numpy(live.astype(np.float64)).to(dtype)[:, None]
    cols = []
    for l in range(table.shape[0]):
        k, w = cell_np(p, int(res[l]), log2T)
        cols.append((torch.from_numpy(w).to(dtype)[:, :, None] * table[l][torch.from_numpy(k)]).sum(1) * live_t)
    return torch.cat(cols, -1)


# ---- backward to the table -------------------------------------------------------------------------------------------------------------
def ceil_log2_4n(n):
    c = 2
    while (1 << (c - 2)) < n:
        c += 1
    return c


def backward_np(g_emb, res, log2T, F, uv=None, idx=None, grid=0, as_double=False, mutate=None):
    """g_table float32 [Lv, T, F] by the integer accumulator: m = max|g_emb| over the live rows, 2^x the smallest power of two above m,
    E = 62 - ceil(log2(4n)); each float product w_c * g is scaled by 2^(E-x) in double, rounded to nearest even into int64 and added;
    g_table = (float)((double)acc * 2^(x-E)).  m = 0: zeros; a non-finite g_emb: all NaN.  as_double=True returns the double before that
    last rounding to float32.  mutate: a deliberately wrong rule for the tests ('swap_axes', 'dense3d', 'E3d', 'colstride')."""
    g_emb = np.asarray(g_emb, f32)
    p, live = rows_uv(uv, idx, grid)
    n, Lv, T = g_emb.shape[0], len(res), 1 << log2T
    assert p.shape[0] == n
    g_emb = g_emb[live]
    p = p[live]
    if not np.all(np.isfinite(g_emb)):
        return np.full((Lv, T, F), np.nan, f32)
    m = float(np.max(np.abs(g_emb))) if g_emb.size else 0.0
    if m == 0.0:
        return np.zeros((Lv, T, F), f32)
    x = math.frexp(m)[1]                                       # m = f * 2^x, f in [0.5, 1): 2^(x-1) <= m < 2^x
    E = 62 - (ceil_log2_4n(n) if mutate != 'E3d' else HG.ceil_log2_8n(n))
    acc = np.zeros((Lv, T, F), np.int64)
    for l in range(Lv):
        k, w = cell_np(p, int(res[l]), log2T, mutate)
        g = g_emb[:, l * F:(l + 1) * F] if mutate != 'colstride' else g_emb[:, l::Lv]
        for c in range(4):
            prod = w[:, c:c + 1] * g                                                 # float32: one rounding
            q = np.rint(np.ldexp(prod.astype(np.float64), E - x)).astype(np.int64)   # rint: nearest even
            for f in range(F):
                np.add.at(acc[l, :, f], k[:, c], q[:, f])
    out = np.ldexp(acc.astype(np.float64), x - E)
    return out if as_double else out.astype(f32)


# ---- the head --------------------------------------------------------------------------------------------------------------------------
def rows_nodes(n, idx, plane):
    """(node int64 [n], live bool [n]): node = row without a list."""
    if idx is None:
        return np.arange(n), np.ones(n, bool)
    idx = np.asarray(idx, np.int64)
    live = (idx >= 0) & (idx < plane)
    return np.where(live, idx, 0), live


def head_f64(raw, idx, plane, fill=0.0):
    """tex float64 [C, plane] = (tanh(raw) + 1) / 2 on the listed nodes, `fill` elsewhere."""
    raw = np.asarray(raw, np.float64)
    node, live = rows_nodes(raw.shape[0], idx, plane)
    tex = np.full((raw.shape[1], plane), fill, np.float64)
    tex[:, node[live]] = ((np.tanh(raw) + 1) / 2)[live].T
    return tex


def head_bwd_f64(grad_tex, g_raw_in, raw, idx, plane):
    """grad_raw float64 [n, C] = g_raw_in (or 0) + grad_tex[c, node] * 0.5 * (1 - tanh(raw)^2)."""
    raw = np.asarray(raw, np.float64)
    node, live = rows_nodes(raw.shape[0], idx, plane)
    out = np.zeros_like(raw) if g_raw_in is None else np.asarray(g_raw_in, np.float64).copy()
    y = np.tanh(raw)
    out += np.where(live[:, None], np.asarray(grad_tex, np.float64)[:, node].T * 0.5 * (1 - y * y), 0.0)
    return out


# ---- the whole field as a torch expression -----------------------------------------------------------------------------------------
def texture_torch(table, params, res, log2T, grid, idx=None):
    """(tex [C, grid^2] zero off the list, raw [n, C]) in the dtype of `table`: rule cells, the MLP (one skip after layer 0), the head."""
    emb = forward_torch(table, res, log2T, idx=idx, grid=grid, dtype=table.dtype)
    raw = HG.mlp_torch(emb, params, 0)
    y = (torch.tanh(raw) + 1) / 2
    if idx is None:
        return y.t(), raw
    node = torch.from_numpy(np.asarray(idx, np.int64))
    return torch.zeros(raw.shape[1], grid * grid, dtype=raw.dtype).index_copy(1, node, y.t()), raw


# ---- shared inputs ------------------------------------------------------------------------------------------------------------------------
TABLE_CASES = [(1, 1, 4), (4, 2, 6), (12, 2, 10), (16, 4, 8)]   # (Lv, F, log2T)
MAX_RES_CASES = [16, 256]
N_CASES = [1, 63, 64, 65, 300]
GRID_CASES = [2, 3, 8, 33]
LIST_SIZES = [1, 65, 500]


def case_points(n, res, seed):
    """n points: uniform in a square 10 % larger than the unit square, then (as n allows) overwritten with 0 and 1 on each axis, nodes of
    the finest level, points outside, and NaN / inf rows."""
    rng = np.random.default_rng(seed)
    p = (-0.05 + rng.random((n, 2)) * 1.1).astype(f32)
    r = int(res[-1])
    special = [f32([0, 0]), f32([1, 1]), f32([0, 1]), f32([1, 0.5]), f32([0.5, 0]), (f32([1, 2]) / f32(r)).astype(f32), f32([0.5, 0.5]),
               f32([-3, 8]), f32([np.nan, 0.5]), f32([np.inf, -np.inf]), f32([0.25, np.nan])]
    for k, s in enumerate(special):
        if 2 * k + 1 < n:
            p[2 * k + 1] = s
    return p


def case_list(grid, size, seed, bad=True):
    """A shuffled subset of the grid^2 nodes, int32 [size (+ 1)], with one out-of-range entry in the middle when bad."""
    rng = np.random.default_rng(seed)
    idx = rng.permutation(grid * grid)[:size].astype(np.int32)
    if bad:
        idx = np.insert(idx, size // 2, np.int32(grid * grid if seed % 2 else -1))
    return idx


def case_table(Lv, F, log2T, seed):
    return np.random.default_rng(seed).standard_normal((Lv, 1 << log2T, F)).astype(f32)


# ---- the fit: one schedule for the CPU restatement and the GPU field (chosen in tests/test_hashtex_cpu.py) ----------------------
FIT = dict(grid=32, Lv=4, F=2, log2T=8, base_res=2, max_res=32, D=2, W=64, C=3, iters=60, table_lr=1e-2, mlp_lr=1e-3,
           betas=(0.9, 0.99), eps=1e-15, seed=7)


def fit_target(grid=32):
    """[3, grid, grid] in [0.1, 0.9]: a 4 x 4-texel checker plus a ramp along u (red), along v (green) and along the diagonal (blue)."""
    i, j = np.meshgrid(np.arange(grid), np.arange(grid), indexing='ij')
    checker = (((i // 4) + (j // 4)) % 2).astype(np.float64)
    ramps = [j / (grid - 1), i / (grid - 1), (i + j) / (2 * grid - 2)]
    return np.stack([0.1 + 0.5 * r + 0.3 * checker for r in ramps]).astype(f32)


def fit_initial():
    """(table float32 [Lv, T, F] uniform in +-1e-4, params: the MLP's six tensors in nn.Linear layout)"""
    c = FIT
    rng = np.random.default_rng(c['seed'])
    table = ((rng.random((c['Lv'], 1 << c['log2T'], c['F'])) * 2 - 1) * 1e-4).astype(f32)
    return table, HG.make_params(c['D'], c['W'], c['Lv'] * c['F'], c['C'], 0, seed=c['seed'])


def fit_optimizer(table, params):
    c = FIT
    return torch.optim.Adam([dict(params=[table], lr=c['table_lr']), dict(params=list(params), lr=c['mlp_lr'])], betas=c['betas'], eps=c['eps'])


def fit_restatement(dtype=torch.float64):
    """The restatement fitted on the CPU -> the loss history (floats)."""
    c = FIT
    res = resolutions(c['Lv'], c['base_res'], c['max_res'])
    table, params = fit_initial()
    table = torch.from_numpy(table).to(dtype).requires_grad_(True)
    params = [p.clone().to(dtype).requires_grad_(True) for p in params]
    target = torch.from_numpy(fit_target(c['grid'])).to(dtype).reshape(c['C'], -1)
    opt = fit_optimizer(table, params)
    hist = []
    for _ in range(c['iters']):
        opt.zero_grad()
        tex, _ = texture_torch(table, params, res, c['log2T'], c['grid'])
        loss = ((tex - target) ** 2).mean()
        loss.backward()
        opt.step()
        hist.append(float(loss.detach()))
    return hist
