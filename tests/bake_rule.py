"""The definition of the bake: numpy restatements in binary32 of `ctx_texel_rays` and `ctx_bake_resolve`
(csrc/bake.hip), the host-only `view_camera` written out again, and a float64 twin of the texel point.  numpy array operations round
every product, sum, quotient and square root on their own, in the order written: no contraction.
Not a test module: tests/test_bake_cpu.py and tests/test_bake_gpu.py import it."""
import numpy as np

f32 = np.float32
FRAC = 32


# ---- view_camera -------------------------------------------------------------------------------------------------------------------------
def view_camera_np(elev, azim, radius, look_at_height, H, W, fovyangle=np.pi / 3):
    """-> (K float32 [3,3], c2w float32 [3,4]) of the Renderer pose: pos = r (sin e sin a, cos e, sin e cos a), looking at
    (0, look_at_height, 0) with up = +y; z = (pos - look_at)/|.|, x = up x z /|.|, y = z x x; c2w = [x y z | pos];
    fx = W / (2 tan(fov/2)), fy = H / (2 tan(fov/2)), cx = (W - 1)/2, cy = (H - 1)/2."""
    e, a, r = f32(elev), f32(azim), f32(radius)
    pos = np.array([r * np.sin(e) * np.sin(a), r * np.cos(e), r * np.sin(e) * np.cos(a)], f32)
    z = pos - np.array([0, look_at_height, 0], f32)
    z = z / np.linalg.norm(z)
    x = np.cross(np.array([0, 1, 0], f32), z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    c2w = np.stack([x, y, z, pos], 1).astype(f32)
    t = np.tan(fovyangle / 2.0)
    K = np.array([[W / (2 * t), 0, (W - 1) / 2], [0, H / (2 * t), (H - 1) / 2], [0, 0, 1]], f32)
    return K, c2w


# ---- ctx_texel_rays ----------------------------------------------------------------------------------------------------------------------
def texel_rays_np(texel_face, texel_bary, face_uv, vertices, faces, idx, s, h, flip_v=True, dy_sign=1.0, rotate=0, swap_cross=False, T_edge=None):
    """-> (rays_o f32 [n*s*s,3], rays_d f32 [n*s*s,3], valid u8 [n*s*s]); row j*s*s + a + s*b is list entry j, column offset a, row offset b.
    The rule of include/ctx_nerf.h (ctx_texel_rays), vectorised over the entries.
    The keyword switches after `h` are MISTAKES the CPU test plants to show that its bounds see them; the definition is the defaults."""
    texel_face = np.asarray(texel_face, np.int64)
    T = texel_face.shape[0]
    texel_bary = np.asarray(texel_bary, f32).reshape(T * T, 3)
    face_uv, vertices, faces = np.asarray(face_uv, f32), np.asarray(vertices, f32), np.asarray(faces, np.int64)
    F, V = faces.shape[0], vertices.shape[0]
    idx = np.asarray(idx, np.int32)
    n, s, ss = idx.shape[0], int(s), int(s) * int(s)
    h, fT = f32(h), f32(T if T_edge is None else T_edge)
    one, half = f32(1), f32(0.5)
    with np.errstate(all='ignore'):
        p = idx.astype(np.int64)
        ok = (p >= 0) & (p < T * T)
        p = np.where(ok, p, 0)
        f = texel_face.reshape(-1)[p]
        ok &= (f >= 0) & (f < F)
        f = np.where(ok, f, 0)
        vid = faces[f]
        ok &= ((vid >= 0) & (vid < V)).all(1)
        vid = np.where(ok[:, None], vid, 0)
        v0, v1, v2 = vertices[vid[:, 0]], vertices[vid[:, 1]], vertices[vid[:, 2]]
        e1, e2 = v1 - v0, v2 - v0
        if swap_cross:
            e1, e2 = e2, e1
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        l2 = (cx * cx + cy * cy) + cz * cz
        ok &= np.isfinite(l2) & (l2 > 0)
        ln = np.sqrt(l2)
        nrm = np.stack([cx / ln, cy / ln, cz / ln], 1)
        b = np.roll(texel_bary[p], rotate, axis=1)
        b0, b1, b2 = b[:, 0], b[:, 1], b[:, 2]
        if s > 1:
            uv = face_uv[f]
            x1, x2 = (uv[:, 1, 0] - uv[:, 0, 0]) * fT, (uv[:, 2, 0] - uv[:, 0, 0]) * fT
            if flip_v:
                y1, y2 = (uv[:, 0, 1] - uv[:, 1, 1]) * fT, (uv[:, 0, 1] - uv[:, 2, 1]) * fT
            else:
                y1, y2 = (uv[:, 1, 1] - uv[:, 0, 1]) * fT, (uv[:, 2, 1] - uv[:, 0, 1]) * fT
            D = x1 * y2 - x2 * y1
            flat = ~np.isfinite(D) | (D == 0)                  # a UV triangle without area: every sub-sample is the texel centre
            g1x, g1y, g2x, g2y = y2 / D, -x2 / D, -y1 / D, x1 / D
        o = np.zeros((n, ss, 3), f32)
        d = np.zeros((n, ss, 3), f32)
        valid = np.zeros((n, ss), np.uint8)
        for k in range(ss):
            a, bb = k % s, k // s
            if s > 1:
                dx = (f32(a) + half) / f32(s) - half
                dyy = f32(dy_sign) * ((f32(bb) + half) / f32(s) - half)
                c1 = b1 + (dx * g1x + dyy * g1y)
                c2 = b2 + (dx * g2x + dyy * g2y)
                c0 = (one - c1) - c2
                c0, c1, c2 = np.where(flat, b0, c0), np.where(flat, b1, c1), np.where(flat, b2, c2)
            else:
                c0, c1, c2 = b0, b1, b2
            x = (c0[:, None] * v0 + c1[:, None] * v1) + c2[:, None] * v2
            o[:, k] = np.where(ok[:, None], x + h * nrm, 0)
            d[:, k] = np.where(ok[:, None], -nrm, 0)
            valid[:, k] = ok
    return o.reshape(n * ss, 3), d.reshape(n * ss, 3), valid.reshape(n * ss)


def texel_points_f64(texel_face, face_uv, vertices, faces, idx, s):
    """The float64 twin of the texel point: (pts f64 [n*s*s,3], cond f64 [n*s*s], ok bool [n*s*s]).  Sub-sample (a, b) of texel (y, x) has
    u = (x + (a + 0.5)/s)/T, v = 1 - (y + (b + 0.5)/s)/T; its barycentrics are solved in the face's UV triangle and the point is
    sum b_k v_k.  cond = 2 (|e1.u| + |e1.v| + |e2.u| + |e2.v|) / (|D| T) with e_k the UV edges and D their cross product: a bound on the
    sum over the three corners of |d b_k / d texel|, the factor by which an error of one texel unit moves the barycentrics.  Rows of
    invalid entries (also a UV triangle without area) are zero, ok False."""
    texel_face = np.asarray(texel_face, np.int64)
    T = texel_face.shape[0]
    uvf, vertices, faces = np.asarray(face_uv, np.float64), np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    p = np.asarray(idx, np.int64)
    ok = (p >= 0) & (p < T * T)
    p = np.where(ok, p, 0)
    f = texel_face.reshape(-1)[p]
    ok &= (f >= 0) & (f < faces.shape[0])
    f = np.where(ok, f, 0)
    y, x = p // T, p % T
    a, b = np.arange(s * s) % s, np.arange(s * s) // s
    u = (x[:, None] + (a[None] + 0.5) / s) / T
    v = 1.0 - (y[:, None] + (b[None] + 0.5) / s) / T
    uv = uvf[f]
    e1, e2 = uv[:, 1] - uv[:, 0], uv[:, 2] - uv[:, 0]
    D = e1[:, 0] * e2[:, 1] - e2[:, 0] * e1[:, 1]
    ok &= D != 0
    Ds = np.where(D != 0, D, 1.0)[:, None]
    du, dv = u - uv[:, 0, 0][:, None], v - uv[:, 0, 1][:, None]
    b1 = (du * e2[:, 1][:, None] - dv * e2[:, 0][:, None]) / Ds
    b2 = (dv * e1[:, 0][:, None] - du * e1[:, 1][:, None]) / Ds
    b0 = 1.0 - b1 - b2
    V = vertices[faces[f]]                                                   # [n,3 corners,3]
    pts = b0[..., None] * V[:, None, 0] + b1[..., None] * V[:, None, 1] + b2[..., None] * V[:, None, 2]
    g = (np.abs(e2[:, 1]) + np.abs(e2[:, 0]) + np.abs(e1[:, 1]) + np.abs(e1[:, 0])) / np.abs(Ds[:, 0]) / T    # sum |d b_k / d texel|, k = 1, 2
    cond = np.repeat(2.0 * g[:, None], s * s, 1)                             # b0 moves by as much as b1 and b2 together
    okk = np.repeat(ok[:, None], s * s, 1)
    pts = np.where(okk[..., None], pts, 0.0)
    return pts.reshape(-1, 3), cond.reshape(-1), okk.reshape(-1)


# ---- ctx_bake_resolve --------------------------------------------------------------------------------------------------------------------
def bake_resolve_np(rgb, alpha, valid, idx, s, T, min_alpha, frac_bits=FRAC, acc=None):
    """-> acc int64 [4,T,T] (+= when given): the rule of include/ctx_nerf.h (ctx_bake_resolve), vectorised over the entries."""
    rgb, alpha, valid = np.asarray(rgb, f32), np.asarray(alpha, f32), np.asarray(valid, np.uint8)
    idx = np.asarray(idx, np.int32)
    n, ss = idx.shape[0], int(s) * int(s)
    rgb, alpha, valid = rgb.reshape(n, ss, 3), alpha.reshape(n, ss), valid.reshape(n, ss)
    if acc is None:
        acc = np.zeros((4, T, T), np.int64)
    flat = acc.reshape(4, T * T)
    with np.errstate(all='ignore'):
        S = np.zeros((n, 4), f32)
        m = np.zeros(n, np.int64)
        for k in range(ss):
            take = (valid[:, k] != 0) & np.isfinite(alpha[:, k]) & np.isfinite(rgb[:, k]).all(1)
            row = np.concatenate([rgb[:, k], alpha[:, k, None]], 1)
            S = np.where(take[:, None], S + row, S)
            m += take
        p = idx.astype(np.int64)
        M = S / np.maximum(m, 1).astype(f32)[:, None]
        write = (p >= 0) & (p < T * T) & (m > 0) & (M[:, 3] >= f32(min_alpha))
        q = np.rint(np.ldexp(M[write], frac_bits).astype(np.float64)).astype(np.int64)
        for c in range(4):
            flat[c, p[write]] += q[:, c]                     # the list holds distinct texels: no index repeats
    return acc
