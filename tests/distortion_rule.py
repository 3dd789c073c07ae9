"""The distortion loss on ragged per-ray sample lists, restated: the binary32 prefix form the HIP kernels implement,
sequentially in numpy, and the float64 pairwise definition with |.| it is judged against.  One definition for the CPU and the GPU tests.

Per ray, t ascending:  nrm = sqrtf((dx*dx + dy*dy) + dz*dz),  x_i = (t_i - t_0) * nrm,  delta_i = dt_i * nrm,
    L       = sum_i sum_j w_i w_j |x_i - x_j| + (1/3) sum_i w_i^2 delta_i
            = sum_i w_i * (2 * (x_i * W_<i - V_<i) + delta_i * w_i / 3)
    dL/dw_i = 2 * (x_i * (W_<i - W_>i) - (V_<i - V_>i)) + 2 * w_i * delta_i / 3
with W_<i = sum_{j<i} w_j, V_<i = sum_{j<i} w_j x_j and the suffix sums W_>i = W - W_<=i, V_>i = V - V_<=i."""
import numpy as np
import torch

f32 = np.float32
COUNTS = [0, 1, 2, 63, 64, 65, 130, 1, 5000, 1, 0]           # every chunk edge, a 5000-sample ray between two 1-sample rays, empty ends
NORMS = (1.0, 3.0, 0.0)


def ray_norm_np(d):
    d = d.astype(f32)
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(f32)


def _ray_np(w, t, dt, nrm):
    """One ray in binary32, every sum sequential (np.cumsum accumulates left to right) -> (L, dL/dw)."""
    x = (t - t[0]) * nrm
    dl = dt * nrm
    Win, Vin = np.cumsum(w, dtype=f32), np.cumsum(w * x, dtype=f32)
    Wex, Vex = np.concatenate([[f32(0)], Win[:-1]]), np.concatenate([[f32(0)], Vin[:-1]])
    terms = w * (f32(2) * (x * Wex - Vex) + (dl * w) / f32(3))
    g = f32(2) * (x * (Wex - (Win[-1] - Win)) - (Vex - (Vin[-1] - Vin))) + (f32(2) * (w * dl)) / f32(3)
    return np.cumsum(terms, dtype=f32)[-1], g.astype(f32)


def distortion_np(w, t, dt, d, ray_off, g_loss=None):
    """The rule on numpy arrays: -> (loss [R], grad_w [n]) in float32; grad_w = g_loss[r] * dL_r/dw (g_loss None: ones)."""
    w, t, dt = (np.asarray(a, f32) for a in (w, t, dt))
    nrm = ray_norm_np(np.asarray(d))
    R = len(nrm)
    gl = np.ones(R, f32) if g_loss is None else np.asarray(g_loss, f32)
    loss, grad = np.zeros(R, f32), np.zeros(len(w), f32)
    for r in range(R):
        a, b = int(ray_off[r]), int(ray_off[r + 1])
        if b > a:
            loss[r], g = _ray_np(w[a:b], t[a:b], dt[a:b], nrm[r])
            grad[a:b] = g * gl[r]
    return loss, grad


def pairwise64(w, t, dt, d, ray_off):
    """The definition in float64 torch: the pairwise double sum with |.|, differentiable in w -> loss [R]."""
    nrm = torch.sqrt((d.double() ** 2).sum(-1))
    out = []
    for r in range(d.shape[0]):
        a, b = int(ray_off[r]), int(ray_off[r + 1])
        x = (t[a:b].double() - (t[a].double() if b > a else 0.)) * nrm[r]
        A = (x[:, None] - x[None, :]).abs()
        out.append(w[a:b] @ (A @ w[a:b]) + (w[a:b] * w[a:b] * (dt[a:b].double() * nrm[r])).sum() / 3.)
    return torch.stack(out)


def oracle64(w, t, dt, d, ray_off, g_loss=None):
    """pairwise64 and its float64 autograd gradient of sum_r g_loss[r] * L_r -> (loss [R], grad_w [n]) as float64 numpy."""
    W = torch.as_tensor(np.asarray(w)).double().requires_grad_(True)
    T, DT, D = (torch.as_tensor(np.asarray(a)) for a in (t, dt, d))
    loss = pairwise64(W, T, DT, D, ray_off)
    gl = torch.ones_like(loss) if g_loss is None else torch.as_tensor(np.asarray(g_loss)).double()
    (loss * gl).sum().backward()
    return loss.detach().numpy(), W.grad.numpy()


def bounds(w, t, dt, d, ray_off, g_loss=None):
    """The derived error bounds, in float64 from the inputs: with S the ray's count, X = x_{S-1} + delta_{S-1} and
    W = sum w:  forward (S + 8) * 2^-22 * X * W^2 per ray [R],  gradient (S + 8) * 2^-21 * X * W * |g_loss| per sample [n].
    The derivation holds for rays whose every width fits the extent, delta_i <= X; a ray with an earlier width far above X (a tie ray of
    two whose first dt is a hundred times its second) has a delta term whose own rounding, 3u * w_i^2 * delta_i / 3, is not covered."""
    w, t, dt, d = (np.asarray(a, np.float64) for a in (w, t, dt, d))
    nrm = np.sqrt((d * d).sum(-1))
    R = len(nrm)
    gl = np.ones(R) if g_loss is None else np.abs(np.asarray(g_loss, np.float64))
    fb, gb = np.zeros(R), np.zeros(len(w))
    for r in range(R):
        a, b = int(ray_off[r]), int(ray_off[r + 1])
        if b > a:
            S, X, W = b - a, ((t[b - 1] - t[a]) + dt[b - 1]) * nrm[r], w[a:b].sum()
            fb[r] = (S + 8) * 2.0 ** -22 * X * W * W
            gb[a:b] = (S + 8) * 2.0 ** -21 * X * W * gl[r]
    return fb, gb


def make_case(counts, seed, norm=1.0, quantised=False):
    """Ragged lists with the given per-ray counts: w in [0,1) with sum w <= 1 per ray, t ascending in [0.5, 4] with ties (every fifth
    sample repeats its predecessor, and a ray of 2 is a tie), dt in (0, 0.1], d = a random direction of length `norm`.
    quantised=True puts t and dt on multiples of 2^-16 and d on multiples of 2^-10, so that t + 4 and a scaling by 3 are exact in
    binary32.  -> numpy (w, t, dt, d [R,3], ray_off int64 [R+1])."""
    rng = np.random.default_rng(seed)
    counts = [int(c) for c in counts]
    ray_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ws, ts = [], []
    for c in counts:
        w = rng.random(c)
        ws.append(w * (rng.random() / max(w.sum(), 1e-30)))
        t = np.sort(rng.random(c) * 3.5 + 0.5)
        t[4::5] = t[3::5][:len(t[4::5])]
        if c == 2:
            t[1] = t[0]
        ts.append(t)
    w, t = np.concatenate(ws).astype(f32), np.concatenate(ts).astype(f32)
    dt = (rng.random(len(w)) * 0.1 + 1e-3).astype(f32)
    d = rng.standard_normal((len(counts), 3))
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    if quantised:
        t, dt, d = np.round(t * 65536) / 65536, np.maximum(np.round(dt * 65536), 1) / 65536, np.round(d * 1024) / 1024
    d = (d * norm).astype(f32)
    for r in range(len(counts)):
        assert np.all(np.diff(t[ray_off[r]:ray_off[r + 1]]) >= 0) and w[ray_off[r]:ray_off[r + 1]].astype(np.float64).sum() <= 1.0
    return w, t.astype(f32), dt.astype(f32), d, ray_off


def make_rect_case(R, S, seed):
    """The rectangular layout of the dense path: weights [R,S], z_vals [R,S] ascending in [0.5, 4], d = randn [R,3] -> numpy (w, z, d) and the
    packed view of it (w [n], t [n], dt [n] with 0 for each ray's last sample, ray_off)."""
    rng = np.random.default_rng(seed)
    w = rng.random((R, S))
    w = (w * (rng.random((R, 1)) / w.sum(-1, keepdims=True))).astype(f32)
    z = np.sort(rng.random((R, S)) * 3.5 + 0.5, -1).astype(f32)
    d = rng.standard_normal((R, 3)).astype(f32)
    dt = np.concatenate([z[:, 1:] - z[:, :-1], np.zeros((R, 1), f32)], -1).astype(f32)
    return (w, z, d), (w.reshape(-1), z.reshape(-1), dt.reshape(-1), d, np.arange(R + 1, dtype=np.int64) * S)


def check(got_loss, got_grad, w, t, dt, d, ray_off, g_loss=None, want=None):
    """Assert the bounds against the float64 oracle (computed here, or the given (loss, grad)); -> the largest error / bound ratios."""
    want_loss, want_grad = oracle64(w, t, dt, d, ray_off, g_loss) if want is None else want
    fb, gb = bounds(w, t, dt, d, ray_off, g_loss)
    fe = np.abs(np.asarray(got_loss, np.float64) - want_loss)
    ge = np.abs(np.asarray(got_grad, np.float64) - want_grad)
    assert np.all(fe <= fb), ("forward", np.nonzero(fe > fb)[0][:5], (fe / np.maximum(fb, 1e-300)).max())
    assert np.all(ge <= gb), ("gradient", np.nonzero(ge > gb)[0][:5], (ge / np.maximum(gb, 1e-300)).max())
    nz = lambda e, b: float((e[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
    return nz(fe, fb), nz(ge, gb)
