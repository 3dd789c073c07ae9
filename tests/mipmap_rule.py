"""The definition of mip-mapped texture sampling: numpy restatements in binary32 of `ctx_mip_build`, `ctx_face_uv_lod`,
`ctx_texture_mapping_mip_fwd` and of the integer pyramid of `ctx_texture_mapping_mip_bwd`, the same forward and its plain adjoint in any
dtype (float64 for the bounds), and the inputs the CPU and the GPU tests share.  numpy array operations round every product, sum and
quotient on their own, in the order written.  Not a test module: tests/test_mipmap_cpu.py and tests/test_mipmap_gpu.py import it."""
import math
import numpy as np

f32 = np.float32


# ---- the pyramid -------------------------------------------------------------------------------------------------------------------------
def check_levels(T, L):
    """L levels of a T x T atlas: level l has side T >> l; T % 2^(L-1) == 0 and T >> (L-1) >= 2."""
    T, L = int(T), int(L)
    if not (1 <= L <= 16 and T >= 2 and T % (1 << (L - 1)) == 0 and (T >> (L - 1)) >= 2):
        raise ValueError(f"mip levels L={L} do not fit T={T}")
    return [T >> l for l in range(L)]


def pyramid(tex, L, coverage=None, dt=f32):
    """-> (levels: L arrays [C, T_l, T_l] of dt, level 0 = tex; counts: L arrays uint8 [T_l, T_l]: cov_0, then n_l).  The children of
    (y, x) are a = (2y, 2x), b = (2y, 2x+1), c = (2y+1, 2x), d = (2y+1, 2x+1); value = s / n, s = 0 then s = s + child over the covered
    children in that order; 0 where n = 0."""
    tex = np.asarray(tex, dt)
    C, T, _ = tex.shape
    check_levels(T, L)
    cov = np.ones((T, T), bool) if coverage is None else (np.asarray(coverage) != 0)
    levels, counts = [tex], [cov.astype(np.uint8)]
    for l in range(1, L):
        src = levels[-1]
        s = np.zeros((C, src.shape[1] // 2, src.shape[2] // 2), dt)
        n = np.zeros(s.shape[1:], np.int64)
        for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
            cc = cov[dy::2, dx::2]
            s = np.where(cc[None], s + src[:, dy::2, dx::2], s).astype(dt)
            n = n + cc
        with np.errstate(all='ignore'):
            v = np.where(n[None] > 0, s / np.maximum(n, 1).astype(dt)[None], dt(0)).astype(dt)
        levels.append(v)
        counts.append(n.astype(np.uint8))
        cov = n > 0
    return levels, counts


# ---- the level of detail of a (view, face) ----------------------------------------------------------------------------------------------
def lod_np(fvi, uva, H, W, T, L, scale=None):
    """lod float32 [B, F] of faces fvi [B, F, 3, 2] (NDC) with uv uva [Bu, F, 3, 2] (Bu = 1: batch 0 for every view); binary32 throughout."""
    fvi, uva = np.asarray(fvi, f32), np.asarray(uva, f32)
    check_levels(T, L)
    B, F = fvi.shape[:2]
    if uva.shape[0] == 1:
        uva = np.broadcast_to(uva, (B,) + uva.shape[1:])
    sb = np.ones(B, f32) if scale is None else np.asarray(scale, f32)
    with np.errstate(all='ignore'):
        e1, e2 = fvi[:, :, 1] - fvi[:, :, 0], fvi[:, :, 2] - fvi[:, :, 0]
        d1, d2 = uva[:, :, 1] - uva[:, :, 0], uva[:, :, 2] - uva[:, :, 0]
        det = e1[..., 0] * e2[..., 1] - e2[..., 0] * e1[..., 1]
        ok = (det != 0) & np.isfinite(det)
        ux = (d1[..., 0] * e2[..., 1] - d2[..., 0] * e1[..., 1]) / det
        uy = (d2[..., 0] * e1[..., 0] - d1[..., 0] * e2[..., 0]) / det
        vx = (d1[..., 1] * e2[..., 1] - d2[..., 1] * e1[..., 1]) / det
        vy = (d2[..., 1] * e1[..., 0] - d1[..., 1] * e2[..., 0]) / det
        ax = (((f32(2) / f32(W)) * f32(T)) * sb)[:, None]
        ay = (((f32(2) / f32(H)) * f32(T)) * sb)[:, None]
        r2 = np.fmax((ax * ax) * ((ux * ux) + (vx * vx)), (ay * ay) * ((uy * uy) + (vy * vy)))     # fmaxf: a NaN yields the other operand
        big = ok & (r2 > 1)                                                # false for magnification and for NaN
        rho = np.sqrt(np.where(big & np.isfinite(r2), r2, f32(1)).astype(f32))
        m, e = np.frexp(rho)                                               # rho = m * 2^e, m in [0.5, 1): ilogbf(rho) = e - 1, ldexpf(rho, -l0) = 2m
        l0 = e.astype(np.int64) - 1
        lod = l0.astype(f32) + (m.astype(f32) * f32(2) - f32(1))
        lod = np.where(l0 >= L - 1, f32(L - 1), lod)
        lod = np.where(np.isinf(r2), f32(L - 1), lod)
        lod = np.where(big, lod, f32(0))
    return lod.astype(f32)


# ---- a pixel's taps ----------------------------------------------------------------------------------------------------------------------
def taps(u, v, T, dt=f32):
    """texel_taps.h: (x0, y0 int64, w [n, 4] of dt for nw, ne, sw, se, inside bool [n, 4]).  ix, iy are binary32 whatever dt is; the weights
    are formed in dt from them."""
    u, v = np.asarray(u, f32), np.asarray(v, f32)

    def src_index(g):
        with np.errstate(all='ignore'):
            c = ((g + f32(1)) * f32(T) - f32(1)) / f32(2)
            return np.fmin(f32(T - 1), np.fmax(c, f32(0)))                 # fmaxf first: a NaN coordinate clamps to 0
    with np.errstate(all='ignore'):
        ix = src_index(u * f32(2) - f32(1))
        iy = src_index((f32(1) - v) * f32(2) - f32(1))
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    ixd, iyd = ix.astype(dt), iy.astype(dt)
    x1f, y1f, x0f, y0f = (x0 + 1).astype(dt), (y0 + 1).astype(dt), x0.astype(dt), y0.astype(dt)
    w = np.stack([(x1f - ixd) * (y1f - iyd), (ixd - x0f) * (y1f - iyd), (x1f - ixd) * (iyd - y0f), (ixd - x0f) * (iyd - y0f)], -1).astype(dt)
    bx1, by1 = x0 + 1 < T, y0 + 1 < T
    inside = np.stack([np.ones_like(bx1), bx1, by1, bx1 & by1], -1)
    return x0, y0, w, inside


def pixel_levels(lod, face_idx, L):
    """(fg bool, l0 int64, f float32) per pixel from the table lod [B, F] and face_idx [B, HW]; the lod is kept inside [0, L-1] (NaN -> 0)."""
    lod, face_idx = np.asarray(lod, f32), np.asarray(face_idx, np.int64)
    F = lod.shape[1]
    assert face_idx.max() < F, "a face_idx outside the table is the kernel's refusal, not the rule's business"
    fg = face_idx >= 0
    b = np.arange(lod.shape[0])[:, None]
    pl = np.fmin(np.fmax(lod[b, np.where(fg, face_idx, 0)], f32(0)), f32(L - 1))
    l0 = pl.astype(np.int64)
    return fg, l0, (pl - l0.astype(f32)).astype(f32)


def _level_tap(level, u, v, dt):
    """the bilinear tap of one level [C, Tl, Tl] at pixels u, v [n]: left-to-right sum over nw, ne, sw, se of texel * w, from 0 -> [n, C]"""
    C, Tl, _ = level.shape
    x0, y0, w, inside = taps(u, v, Tl, dt)
    acc = np.zeros((u.shape[0], C), dt)
    for k in range(4):
        xk, yk = np.minimum(x0 + (k & 1), Tl - 1), np.minimum(y0 + (k >> 1), Tl - 1)
        term = level[:, yk, xk].T * w[:, k:k + 1]
        acc = np.where(inside[:, k:k + 1], acc + term, acc).astype(dt)
    return acc


def forward(levels, uv, lod, face_idx, dt=f32):
    """out [B, HW, C] of dt: 0 on the background; s0 at level l0 = (int)lod; f > 0: s0*(1 - f) + s1*f with s1 at level l0 + 1."""
    uv = np.asarray(uv, f32)
    B, HW = uv.shape[0], uv.shape[1]
    L, C = len(levels), levels[0].shape[0]
    levels = [np.asarray(v, dt) for v in levels]
    fg, l0, f = pixel_levels(lod, face_idx, L)
    out = np.zeros((B * HW, C), dt)
    u, v, fgf, l0f, ff = uv[..., 0].reshape(-1), uv[..., 1].reshape(-1), fg.reshape(-1), l0.reshape(-1), f.reshape(-1)
    with np.errstate(all='ignore'):
        for l in range(L):
            sel = np.nonzero(fgf & (l0f == l))[0]
            if not sel.size:
                continue
            s0 = _level_tap(levels[l], u[sel], v[sel], dt)
            blend = ff[sel] > 0
            if blend.any():
                s1 = _level_tap(levels[l + 1], u[sel][blend], v[sel][blend], dt)
                fb = ff[sel][blend].astype(dt)[:, None]
                s0[blend] = s0[blend] * (dt(1) - fb) + s1 * fb
            out[sel] = s0
    return out.reshape(B, HW, C)


# ---- backward to the atlas ---------------------------------------------------------------------------------------------------------------
def _terms(go, uv, lod, face_idx, T, L, dt):
    """every term of stage A: yields (level, flat texel index [m], term [m, C] of dt), out-of-atlas taps and the background left out"""
    go, uv = np.asarray(go, dt), np.asarray(uv, f32)
    C = go.shape[-1]
    fg, l0, f = pixel_levels(lod, face_idx, L)
    g, u, v = go.reshape(-1, C), uv[..., 0].reshape(-1), uv[..., 1].reshape(-1)
    fgf, l0f, ff = fg.reshape(-1), l0.reshape(-1), f.reshape(-1)
    for hi in (0, 1):
        for l in range(L - hi):
            sel = np.nonzero(fgf & (l0f == l) & ((ff > 0) if hi else True))[0]
            if not sel.size:
                continue
            fs = ff[sel].astype(dt)[:, None]
            gl = np.where(fs > 0, g[sel] * (fs if hi else dt(1) - fs), g[sel]).astype(dt)
            Tl = T >> (l + hi)
            x0, y0, w, inside = taps(u[sel], v[sel], Tl, dt)
            for k in range(4):
                keep = inside[:, k]
                at = (y0 + (k >> 1)) * Tl + x0 + (k & 1)
                yield l + hi, at[keep], (w[:, k:k + 1] * gl)[keep].astype(dt)


def collapse(A, counts, dt=f32):
    """stage B: g0 = A_0 on the covered texels (0 elsewhere), Wt = 1, and for l = 1 .. L-1: Wt = Wt / n_l, g0 = g0 + A_l * Wt"""
    L, T = len(A), A[0].shape[-1]
    g0 = np.asarray(A[0], dt).copy()
    wt = np.ones((T, T), dt)
    yy, xx = np.mgrid[0:T, 0:T]
    covered = np.ones((T, T), bool) if counts is None else counts[0] != 0
    for l in range(1, L):
        n = np.full((T, T), 4, np.int64) if counts is None else counts[l][yy >> l, xx >> l].astype(np.int64)
        with np.errstate(all='ignore'):
            wt = (wt / np.maximum(n, 1).astype(dt)).astype(dt)
            g0 = (g0 + np.asarray(A[l], dt)[:, yy >> l, xx >> l] * wt[None]).astype(dt)
    return np.where(covered[None], g0, dt(0)).astype(dt)


def backward_plain(go, uv, lod, face_idx, T, L, counts=None, dt=np.float64):
    """the forward's adjoint in dt by plain sums (no integer accumulator): the reference of the bounds, grad_tex [C, T, T]"""
    C = np.asarray(go).shape[-1]
    A = [np.zeros((C, (T >> l) ** 2), dt) for l in range(L)]
    for l, at, term in _terms(go, uv, lod, face_idx, T, L, dt):
        for c in range(C):
            np.add.at(A[l][c], at, term[:, c])
    return collapse([a.reshape(C, T >> l, T >> l) for l, a in enumerate(A)], counts, dt)


def ceil_log2_4n(n):
    c = 2
    while (1 << (c - 2)) < n:
        c += 1
    return c


def backward_np(go, uv, lod, face_idx, T, L, counts=None):
    """grad_tex float32 [C, T, T] by the integer pyramid: m = max|go| over all of go, 2^x the smallest power of two above m,
    E = 62 - ceil(log2(4 B HW)); every float32 term is scaled by 2^(E-x) in double, rounded to nearest even into int64 and added;
    A_l = (float)((double)acc_l * 2^(x-E)), then `collapse`.  m = 0: zeros; a non-finite go: all NaN."""
    go = np.asarray(go, f32)
    C = go.shape[-1]
    if not np.all(np.isfinite(go)):
        return np.full((C, T, T), np.nan, f32)
    m = float(np.max(np.abs(go)))
    if m == 0.0:
        return np.zeros((C, T, T), f32)
    x = math.frexp(m)[1]
    E = 62 - ceil_log2_4n(go.shape[0] * go.shape[1])
    acc = [np.zeros((C, (T >> l) ** 2), np.int64) for l in range(L)]
    for l, at, term in _terms(go, uv, lod, face_idx, T, L, f32):
        q = np.rint(np.ldexp(term.astype(np.float64), E - x)).astype(np.int64)             # rint: nearest even
        for c in range(C):
            np.add.at(acc[l][c], at, q[:, c])
    A = [np.ldexp(a.astype(np.float64), x - E).astype(f32).reshape(C, T >> l, T >> l) for l, a in enumerate(acc)]
    return collapse(A, counts, f32)


# ---- shared inputs ---------------------------------------------------------------------------------------------------------------------
def quad_faces():
    """the full-screen quad with uv = the unit square, as two faces: (fvi [1, 2, 3, 2] NDC, uva [1, 2, 3, 2])"""
    p = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], f32)
    t = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], f32)
    tri = [[0, 1, 2], [0, 2, 3]]
    return p[tri][None], t[tri][None]


def quad_raster(H, W):
    """what the raster gives for `quad_faces`: uv [1, H*W, 2] at the pixel centres (v up), face_idx [1, H*W] (0 below the diagonal)"""
    j, i = np.mgrid[0:H, 0:W]
    u = ((2 * i + 1).astype(f32) / f32(2 * W)).astype(f32)
    v = (f32(1) - (2 * j + 1).astype(f32) / f32(2 * H)).astype(f32)
    fi = (v > u).astype(np.int64)
    return np.stack([u, v], -1).reshape(1, H * W, 2), fi.reshape(1, H * W)


def stripes(T=64):
    """[1, T, T]: texels with x % 4 in {1, 2} are 1, the rest 0"""
    x = np.arange(T)
    return np.broadcast_to(((x % 4 == 1) | (x % 4 == 2)).astype(f32)[None, None, :], (1, T, T)).copy()


def case_raster(B, H, W, F, seed):
    """uv [B, H*W, 2] with values below 0, above 1 and exactly 0 and 1; face_idx [B, H*W] random in [-1, F)"""
    rng = np.random.default_rng(seed)
    uv = rng.uniform(-0.1, 1.1, (B, H * W, 2)).astype(f32)
    uv[:, 0] = (0, 0); uv[:, 1] = (1, 1); uv[:, 2] = (0, 1); uv[:, 3] = (1, 0); uv[:, 4] = (-0.5, 2.0)
    return uv, rng.integers(-1, F, (B, H * W)).astype(np.int64)


def case_lod_table(B, F, L, seed):
    """lod [B, F]: 0, exact integers, L-1 and fractions"""
    rng = np.random.default_rng(seed)
    lod = rng.uniform(0, L - 1, (B, F)).astype(f32)
    lod[:, 0] = 0
    lod[:, 1] = L - 1
    lod[:, 2] = 1
    lod[:, 3] = np.nextafter(f32(1), f32(0))
    lod[:, 4] = min(2, L - 1)
    lod[:, 5] = 0.5
    return lod


def case_coverage(T, seed):
    """uint8 [T, T] with fully uncovered 2 x 2 and 4 x 4 blocks and partly covered ones"""
    rng = np.random.default_rng(seed)
    cov = (rng.uniform(size=(T, T)) < 0.7).astype(np.uint8)
    cov[0:4, 0:4] = 0
    cov[4:6, 8:10] = 0
    cov[T - 4:, T - 4:] = 0
    cov[8:12, 0:4] = 1
    return cov
