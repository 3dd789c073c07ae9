"""The definition of the hash-grid encoding's gradient to the positions: the numpy restatement in binary32 that
`ctx_hashgrid_bwd_pts` is array_equal to, the same formula in float64 with the magnitude its error bound scales with, the forward as a
torch expression differentiable in the positions, and the per-ray weighted sum of `ctx_weighted_sum_packed` restated sequentially.
Cells, weights, corner order and entry indices come from tests/hashgrid_rule.py.
Not a test module: tests/test_hashgrid_grad_cpu.py and tests/test_hashgrid_grad_gpu.py import it."""
import numpy as np
import torch

import hashgrid_rule as HG

f32 = np.float32
OTHERS = ((1, 2), (0, 2), (0, 1))                      # o1 < o2, the two other axes of axis a
MUTATIONS = ("swap_axes", "no_sign", "no_res", "stride")


def _box(lo, hi):
    """lo, hi as float32 [3]: a number or three per axis."""
    return tuple(np.broadcast_to(np.asarray(v, f32), (3,)).copy() for v in (lo, hi))


def active_np(pts, lo, hi):
    """bool [n,3]: x = (p - lo) / (hi - lo) in binary32, before the clamp, has x > 0 and x < 1.  False for NaN, +-inf and the box faces."""
    pts = np.asarray(pts, f32).reshape(-1, 3)
    lo, hi = _box(lo, hi)
    with np.errstate(all='ignore'):
        x = (pts - lo) / (hi - lo)
        return (x > 0) & (x < 1)


def outside_np(pts, lo, hi):
    """bool [n,3]: the axes strictly outside the box (finite or infinite x < 0 or x > 1)."""
    pts = np.asarray(pts, f32).reshape(-1, 3)
    lo, hi = _box(lo, hi)
    with np.errstate(all='ignore'):
        x = (pts - lo) / (hi - lo)
        return (x < 0) | (x > 1)


def _column(l, f, Lv, F, mutate):
    return f * Lv + l if mutate == "stride" else l * F + f


def grad_pts_np(pts, table, g_emb, lo, hi, res, log2T, mutate=None):
    """g_pts float32 [n,3], every operation binary32 in the kernel's order.  Per level l and axis a: s_a = (float)res / (hi_a - lo_a); per
    corner c ascending q_c = s_o1 * s_o2 with s_b = bit_b ? w_b : 1 - w_b, term = q_c * t_c[f], d_a[f] = d_a[f] +- term (+ where bit_a is set)
    from 0; gl_a = sum_f g_emb[n, l*F + f] * d_a[f] left to right from 0; g_pts[n, a] = sum_l gl_a * s_a ascending from 0; exactly 0 on an
    inactive axis.  mutate: one of MUTATIONS, a deliberately wrong variant for the test that the bound can fail."""
    pts = np.asarray(pts, f32).reshape(-1, 3)
    table, g_emb = np.asarray(table, f32), np.asarray(g_emb, f32)
    lo, hi = _box(lo, hi)
    Lv, T, F = table.shape
    n = pts.shape[0]
    ext = hi - lo
    one = f32(1)
    out = np.zeros((n, 3), f32)
    with np.errstate(all='ignore'):
        for l in range(Lv):
            r = int(res[l])
            i, pos = HG.positions_np(pts, lo, hi, r)
            w = pos - i.astype(f32)
            idx, _ = HG.cell_np(pts, lo, hi, r, log2T)
            s_axis = (one if mutate == "no_res" else f32(r)) / ext
            d = [np.zeros((n, F), f32) for _ in range(3)]
            for c in range(8):
                b = (c & 1, (c >> 1) & 1, (c >> 2) & 1)
                s = [w[:, a] if b[a] else one - w[:, a] for a in range(3)]
                t = table[l, idx[:, c]]
                for a in range(3):
                    o1, o2 = OTHERS[a]
                    if mutate == "swap_axes":
                        o1 = a
                    term = (s[o1] * s[o2])[:, None] * t
                    d[a] = d[a] + term if (b[a] or mutate == "no_sign") else d[a] - term
            for a in range(3):
                gl = np.zeros(n, f32)
                for f in range(F):
                    gl = gl + g_emb[:, _column(l, f, Lv, F, mutate)] * d[a][:, f]
                out[:, a] = out[:, a] + gl * s_axis[a]
    out[~active_np(pts, lo, hi)] = 0
    return out


def grad_pts_f64(pts, table, g_emb, lo, hi, res, log2T):
    """-> (g_pts float64 [n,3], mag float64 [n,3]): the same formula with float64 weights, products and sums at the rule's binary32 positions
    (cell and pos from positions_np, the box extent as the binary32 hi - lo), and mag = sum_l s_a sum_f |g| sum_c |q_c t_c|, what the error
    bound (Lv + F + 16) * 2^-24 * mag scales with.  Both 0 on inactive axes."""
    pts = np.asarray(pts, f32).reshape(-1, 3)
    lo, hi = _box(lo, hi)
    table, g_emb = np.asarray(table, np.float64), np.asarray(g_emb, np.float64)
    Lv, T, F = table.shape
    n = pts.shape[0]
    ext = (hi - lo).astype(np.float64)
    out, mag = np.zeros((n, 3)), np.zeros((n, 3))
    with np.errstate(all='ignore'):
        for l in range(Lv):
            r = int(res[l])
            i, pos = HG.positions_np(pts, lo, hi, r)
            w = pos.astype(np.float64) - i
            idx, _ = HG.cell_np(pts, lo, hi, r, log2T)
            g = g_emb[:, l * F:(l + 1) * F]
            for a in range(3):
                o1, o2 = OTHERS[a]
                d, m = np.zeros((n, F)), np.zeros((n, F))
                for c in range(8):
                    b = (c & 1, (c >> 1) & 1, (c >> 2) & 1)
                    q = (w[:, o1] if b[o1] else 1 - w[:, o1]) * (w[:, o2] if b[o2] else 1 - w[:, o2])
                    term = q[:, None] * table[l, idx[:, c]]
                    d = d + term if b[a] else d - term
                    m = m + np.abs(term)
                out[:, a] += (g * d).sum(1) * (r / ext[a])
                mag[:, a] += (np.abs(g) * m).sum(1) * (r / ext[a])
    off = ~active_np(pts, lo, hi)
    out[off] = 0
    mag[off] = 0
    return out, mag


def bound(mag, Lv, F):
    """(Lv + F + 16) * 2^-24 * mag: per level 8 products of two rounded factors and their 8-term sum, the F-term dot with g, the scaling
    by s_a and the Lv-term level sum, each operation within 2^-24 relative of its exact result."""
    return (Lv + F + 16) * 2.0 ** -24 * mag


def forward_torch_pts(pts, table, lo, hi, res, log2T):
    """emb [n, Lv*F] as a torch expression differentiable in pts (a torch tensor [n,3]; table a tensor [Lv, T, F] of the same dtype):
    x = clamp((p - lo) / (hi - lo), 0, 1), pos = x * res, w = pos - i with the cell i taken from the binary32 rule (floor detached), then the
    trilinear interpolation of the rule's entries.  The clamp's derivative is autograd's: 0 strictly outside the box."""
    Lv, T, F = table.shape
    p32 = pts.detach().numpy().astype(f32)
    lo32, hi32 = _box(lo, hi)
    lo_t = torch.from_numpy(lo32).to(pts.dtype)
    ext_t = torch.from_numpy(hi32 - lo32).to(pts.dtype)
    x = torch.clamp((pts - lo_t) / ext_t, 0.0, 1.0)
    cols = []
    for l in range(Lv):
        r = int(res[l])
        i, _ = HG.positions_np(p32, lo32, hi32, r)
        idx, _ = HG.cell_np(p32, lo32, hi32, r, log2T)
        w = x * r - torch.from_numpy(i).to(pts.dtype)
        acc = 0
        for c in range(8):
            b = (c & 1, (c >> 1) & 1, (c >> 2) & 1)
            wc = 1
            for a in range(3):
                wc = wc * (w[:, a] if b[a] else 1 - w[:, a])
            acc = acc + wc[:, None] * table[l][torch.from_numpy(idx[:, c])]
        cols.append(acc)
    return torch.cat(cols, -1)


# ---- the per-ray weighted sum --------------------------------------------------------------------------------------------------------
def weighted_sum_np(w, v, ray_off):
    """out float32 [R,C]: per ray and channel the left-to-right binary32 sum of the rounded products w_i * v_{i,c}, from 0 (np.cumsum
    accumulates sequentially); zeros for a ray without samples."""
    w, v = np.asarray(w, f32), np.asarray(v, f32)
    R = len(ray_off) - 1
    out = np.zeros((R, v.shape[1]), f32)
    for r in range(R):
        a, b = int(ray_off[r]), int(ray_off[r + 1])
        if b > a:
            out[r] = np.cumsum(w[a:b, None] * v[a:b], 0, dtype=f32)[-1]
    return out


def weighted_sum_f64(w, v, ray_off):
    """-> (out float64 [R,C], bound float64 [R,C]) with bound = (S + 8) * 2^-24 * sum_i |w_i v_{i,c}|: one rounding per product and at most
    S - 1 roundings along any summation order of S terms, with room for the wave sum's tree."""
    w, v = np.asarray(w, np.float64), np.asarray(v, np.float64)
    R = len(ray_off) - 1
    out, bnd = np.zeros((R, v.shape[1])), np.zeros((R, v.shape[1]))
    for r in range(R):
        a, b = int(ray_off[r]), int(ray_off[r + 1])
        prod = w[a:b, None] * v[a:b]
        out[r] = prod.sum(0)
        bnd[r] = (b - a + 8) * 2.0 ** -24 * np.abs(prod).sum(0)
    return out, bnd


def weighted_sum_case(counts, C, seed, quantised=False):
    """Ragged lists with the given per-ray counts: w in [0, 1), v in [-1, 1)^C -> (w [n], v [n,C], ray_off int64 [R+1]).  quantised=True puts
    both on multiples of 2^-5, so that every product and every partial sum of up to 2^13 of them is exact in binary32."""
    rng = np.random.default_rng(seed)
    ray_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n = int(ray_off[-1])
    w = rng.random(n).astype(f32)
    v = (rng.random((n, C)) * 2 - 1).astype(f32)
    if quantised:
        w, v = np.floor(w * 32) / f32(32), np.floor(v * 32) / f32(32)
    return w.astype(f32), v.astype(f32), ray_off
