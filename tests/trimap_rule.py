"""numpy restatements of the progressive paint loop's rules (include/ctx_nerf.h: ctx_mask_morph, ctx_sep_filter, ctx_atlas_blend;
trainer.py: calculate_trimap, checker_mask, projection_weight).  These ARE the definitions the kernels and the host logic are held to;
TEXTure's own source is not available to this project, the rules are written from the paper (Richardson et al. 2023, sections 3.2-3.3).
"""
import numpy as np

F32 = np.float32
ONE = 1 << 32


# ---- morphology: window clipped to the image --------------------------------------------------------------------------------
def _morph_axis(x, k, axis, dilate):
    r = k // 2
    fill = -np.inf if dilate else np.inf
    pad = [(0, 0)] * x.ndim
    pad[axis] = (r, r)
    p = np.pad(x, pad, mode='constant', constant_values=fill)
    win = np.lib.stride_tricks.sliding_window_view(p, k, axis=axis)
    return (win.max(-1) if dilate else win.min(-1)).astype(x.dtype)


def morph(x, k, op):
    """x float32 [..., H, W]; op 0 dilate (max) | 1 erode (min) over the k x k window INSIDE the image."""
    assert k % 2 == 1 and 1 <= k <= 63 and op in (0, 1)
    x = np.asarray(x, F32)
    return _morph_axis(_morph_axis(x, k, x.ndim - 1, op == 0), k, x.ndim - 2, op == 0)


def dilate(x, k):
    return morph(x, k, 0)


def erode(x, k):
    return morph(x, k, 1)


# ---- taps and the separable filter --------------------------------------------------------------------------------------------
def gaussian_taps(k, sigma):
    x = np.arange(-(k // 2), k // 2 + 1, dtype=np.float64)
    pdf = np.exp(-0.5 * (x / float(sigma)) ** 2)
    return (pdf / pdf.sum()).astype(F32)


def _filter_axis(x, taps, axis, dtype):
    k = len(taps)
    r = k // 2
    assert r <= x.shape[axis] - 1, "reflect padding needs k/2 <= n - 1"
    pad = [(0, 0)] * x.ndim
    pad[axis] = (r, r)
    p = np.pad(x.astype(dtype), pad, mode='reflect')
    n = x.shape[axis]
    acc = None
    for j in range(k):
        v = np.take(p, np.arange(j, j + n), axis=axis)
        prod = (dtype(taps[j]) * v).astype(dtype)
        acc = prod if acc is None else (acc + prod).astype(dtype)
    return acc


def sep_filter(x, taps, dtype=F32):
    """Rows, then columns; every output the taps summed left to right in `dtype` (float32: the kernel's bits; float64: its twin)."""
    x = np.asarray(x, F32)
    return _filter_axis(_filter_axis(x, taps, x.ndim - 1, dtype), taps, x.ndim - 2, dtype)


def sep_filter_bound(k, absmax):
    """|float32 restatement - float64 twin| <= 2k * 2^-24 * max|x| for taps that are non-negative and sum to 1 +- k 2^-24: each pass
    rounds k products and k - 1 sums of magnitude <= max|x| (1 + k 2^-24), half an ulp each: < k 2^-24 max|x| per pass to first order,
    and the second pass carries the first one's error through taps that sum to 1."""
    return 2 * k * 2.0 ** -24 * float(absmax)


# ---- radii scaled with the render grid ----------------------------------------------------------------------------------------------
K0 = dict(generate=19, rim=7, open=5, project=25, blur=21)


def scaled_radius(r0, G):
    return (2 * r0 * G + 1200) // 2400


def scaled_k(k0, G):
    return 2 * scaled_radius(k0 // 2, G) + 1


def blur_sigma(G):
    return 16.0 * G / 1200.0


# ---- trimap, checkerboard, projection weight ----------------------------------------------------------------------------------------
def calculate_trimap(object_mask, z_normals, painted, z_cache, G, z_update_thr=0.2):
    """all [G,G] float32 -> (update, generate, refine) float32 {0,1}."""
    obj, ptd = np.asarray(object_mask, F32) > 0, np.asarray(painted, F32) > 0
    z, zc = np.asarray(z_normals, F32), np.asarray(z_cache, F32)
    exact_generate = (obj & ~ptd).astype(F32)
    generate = dilate(exact_generate, scaled_k(K0['generate'], G))
    better = ((z > (zc + F32(z_update_thr)).astype(F32)) & ptd & obj).astype(F32)
    ko = scaled_k(K0['open'], G)
    refine = dilate(erode(better, ko), ko)
    update = np.maximum(generate, refine)
    rim = erode(obj.astype(F32), scaled_k(K0['rim'], G))
    update[(rim == 0) & (generate == 0)] = 0
    return update, generate, refine


def nearest_resize(x, S):
    """torch's F.interpolate(mode='nearest') for a square image: source index floor(i * n / S)."""
    n = x.shape[-1]
    idx = (np.arange(S) * n) // S
    return x[..., idx, :][..., :, idx]


def checker_board(S):
    c = max(1, S // 32)
    i = np.arange(S)
    return (((i[:, None] // c) + (i[None, :] // c)) % 2).astype(F32)


def checker_mask(update, refine, generate, S):
    out = nearest_resize(np.asarray(update, F32), S).copy()
    only = (nearest_resize(np.asarray(refine, F32), S) > 0) & ~(nearest_resize(np.asarray(generate, F32), S) > 0)
    out[only] = checker_board(S)[only]
    return out


def projection_weight(object_mask, update, z_normals, painted, z_cache, G, strict=True):
    obj = (np.asarray(object_mask, F32) > 0).astype(F32)
    oe = erode(obj, scaled_k(K0['open'], G))
    core = ((oe > 0) & (np.asarray(update, F32) > 0)).astype(F32)
    kb = scaled_k(K0['blur'], G)
    soft = sep_filter(dilate(core, scaled_k(K0['project'], G)), gaussian_taps(kb, blur_sigma(G)))
    soft[oe == 0] = 0
    if strict:
        soft[soft < F32(0.5)] = 0
        soft[(np.asarray(painted, F32) > 0) & (np.asarray(z_cache, F32) > np.asarray(z_normals, F32))] = 0
    return soft


# ---- the atlas update -------------------------------------------------------------------------------------------------------------
def _to_float(v):
    return np.ldexp(np.asarray(v, np.int64).astype(np.float64), -32).astype(F32)


def _to_fixed(v):
    return np.rint(np.ldexp(np.asarray(v, F32).astype(np.float64), 32)).astype(np.int64)


def atlas_blend(contrib, zsum, acc, meta):
    """contrib [4,T,T] i64, zsum [T,T] i64, acc [4,T,T] i64, meta [T,T] f32 -> (acc', meta'), inputs untouched."""
    contrib, zsum = np.asarray(contrib, np.int64), np.asarray(zsum, np.int64)
    acc, meta = np.array(acc, np.int64), np.array(meta, F32)
    w = contrib[3]
    hit = w > 0
    with np.errstate(divide='ignore', invalid='ignore'):
        wf = _to_float(w)
        m = np.minimum(F32(1), wf)
        keep = (F32(1) - m).astype(F32)
        z = (_to_float(zsum) / wf).astype(F32)
        fresh = acc[3] <= 0
        awf = np.where(fresh, F32(1), _to_float(acc[3])).astype(F32)
        for c in range(3):
            new = (_to_float(contrib[c]) / wf).astype(F32)
            old = (_to_float(acc[c]) / awf).astype(F32)
            mix = ((old * keep).astype(F32) + (new * m).astype(F32)).astype(F32)
            out = np.where(fresh, new, mix)
            acc[c] = np.where(hit, _to_fixed(np.where(hit, out, 0)), acc[c])
        zmix = ((meta * keep).astype(F32) + (z * m).astype(F32)).astype(F32)
        meta = np.where(hit, np.where(fresh, z, zmix), meta).astype(F32)
    acc[3] = np.where(hit, ONE, acc[3])
    return acc, meta
