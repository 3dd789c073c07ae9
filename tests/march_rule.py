"""The definition of the march: numpy restatements in binary32 of `ctx_occ_march_count` / `ctx_occ_march_write`, the
packed compositing formula in plain torch with its closed-form backward, and the inputs the CPU and the GPU tests share.
Not a test module: tests/test_march_cpu.py and tests/test_march_gpu.py import it."""
import numpy as np
import torch

f32 = np.float32
RUN_MAX = 4097           # samples of one run: one more than a ray may hold
RAY_MAX = 4096           # samples per ray the compositing backward holds


def occ_walk_np(ro, rd, near, far, cells, lo, hi, inv, h):
    """The walk of `ctx_occ_ray_spans`, vectorised over the rays -> (ta, tb, ok, steps) with steps a list of (visit bool [R], occ bool [R],
    t_in [R], t_out [R]) in walk order: `visit` marks the rays that look at a cell in that step, `occ` those whose cell is occupied.
    Finite check; clip: t_a = near, t_b = far, per axis with d != 0: t1 = (lo - o)/d, t2 = (hi - o)/d, t_a = max(t_a, min(t1, t2)),
    t_b = min(t_b, max(t1, t2)); with d == 0 the ray misses unless lo <= o <= hi; it misses unless t_a <= t_b.  Start cell per axis:
    (int)clamp(((o + d*t_a) - lo)*inv, 0, G - 1).  At every cell the exit parameter per axis is ((lo + (float)(c + (d > 0))*h) - o)/d (+inf
    for d == 0), te = the smallest, ties x, y, z; t_out = min(max(te, t_in), t_b) is the next cell's t_in.  The walk ends when te >= t_b,
    when the step along te's axis leaves the grid, or after 3G + 3 cells."""
    cells = np.asarray(cells)
    G = cells.shape[0]
    ro, rd = np.asarray(ro, f32).reshape(-1, 3), np.asarray(rd, f32).reshape(-1, 3)
    lo, hi, inv, h = (np.asarray(x, f32) for x in (lo, hi, inv, h))
    near, far = f32(near), f32(far)
    R = ro.shape[0]
    one, inf = f32(1), f32(np.inf)
    steps = []
    with np.errstate(all='ignore'):
        ok = np.all(np.isfinite(ro), -1) & np.all(np.isfinite(rd), -1)
        ta, tb = np.full(R, near, f32), np.full(R, far, f32)
        for k in range(3):
            o, d = ro[:, k], rd[:, k]
            zero = d == 0
            dd = np.where(zero, one, d)
            t1, t2 = (lo[k] - o) / dd, (hi[k] - o) / dd
            ta = np.where(zero, ta, np.maximum(ta, np.minimum(t1, t2)))
            tb = np.where(zero, tb, np.minimum(tb, np.maximum(t1, t2)))
            ok &= ~zero | ((o >= lo[k]) & (o <= hi[k]))
        ok &= ta <= tb
        c = []
        for k in range(3):
            t = ((ro[:, k] + rd[:, k] * ta) - lo[k]) * inv[k]
            t = np.minimum(np.maximum(t, f32(0)), f32(G - 1))
            c.append(np.where(ok, t, f32(0)).astype(np.int64))
        active, tin = ok.copy(), ta.copy()
        for _ in range(3 * G + 3):
            if not active.any():
                break
            ex = []
            for k in range(3):
                d = rd[:, k]
                zero = d == 0
                cf = (c[k] + (d > 0)).astype(f32)
                ex.append(np.where(zero, inf, ((lo[k] + cf * h[k]) - ro[:, k]) / np.where(zero, one, d)))
            ax, te = np.zeros(R, np.int64), ex[0]
            for k in (1, 2):
                m = ex[k] < te
                ax, te = np.where(m, k, ax), np.where(m, ex[k], te)
            tout = np.minimum(np.maximum(te, tin), tb)
            steps.append((active.copy(), active & (cells[c[2], c[1], c[0]] != 0), tin.copy(), tout.copy()))
            active = active & ~(te >= tb)
            for k in range(3):
                nxt = c[k] + np.where(rd[:, k] > 0, 1, -1)
                move = active & (ax == k)
                active = active & ~(move & ((nxt < 0) | (nxt > G - 1)))
                c[k] = np.where(move & active, nxt, c[k])
            tin = tout
    return ta, tb, ok, steps


def spans_from_walk(steps, R, near, far):
    """(span, hit) of `ctx_occ_ray_spans` from the steps of the walk: what tests/test_occupancy_mesh_cpu.occ_ray_spans_np returns."""
    s0, s1, found = np.full(R, f32(near), f32), np.full(R, f32(far), f32), np.zeros(R, bool)
    for _, occ, tin, tout in steps:
        s0 = np.where(occ & ~found, tin, s0)
        s1 = np.where(occ, tout, s1)
        found |= occ
    return np.stack([s0, s1], -1).astype(f32), found.astype(np.uint8)


def occ_runs_np(steps, R):
    """-> (ray int64 [m], a float32 [m], b float32 [m]): the runs of all rays, ordered by ray and, within a ray, in walk order.  A run is
    a maximal sequence of consecutive occupied cells: a = t_in of its first, b = t_out of its last; an empty cell closes the open run (also
    one of zero length), and so does the end of the walk."""
    open_, a, b = np.zeros(R, bool), np.zeros(R, f32), np.zeros(R, f32)
    rr, aa, bb = [], [], []

    def close(m):
        idx = np.nonzero(m)[0]
        rr.append(idx); aa.append(a[idx].copy()); bb.append(b[idx].copy())
    for visit, occ, tin, tout in steps:
        a = np.where(occ & ~open_, tin, a)
        b = np.where(occ, tout, b)
        closing = visit & ~occ & open_
        open_ = (open_ | occ) & ~closing
        close(closing)
    close(open_)
    ray, a, b = np.concatenate(rr), np.concatenate(aa), np.concatenate(bb)
    order = np.argsort(ray, kind='stable')                    # appended in walk order: stable keeps it inside a ray
    return ray[order], a[order], b[order]


def occ_march_np(ro, rd, near, far, cells, lo, hi, inv, h, step, u=None):
    """-> (count int32 [R], ray_off int64 [R+1], ray_id int32 [n], t [n], dt [n], pts [n,3], runs): the restatement of `ctx_occ_march_count`
    and `ctx_occ_march_write`.  Per closed run [a, b] of ray (o, d): nrm = sqrt((dx*dx + dy*dy) + dz*dz), len = (b - a)*nrm; no sample
    unless len > 0; else k = (int)min(max(ceil(len / step), 1), 4097), dt = (b - a) / (float)k, t_j = a + ((float)j + u)*dt for j < k with
    u = 0.5 or the caller's draw for that sample (u [n], indexed like the lists), p = o + d*t_j.  runs = (ray, a, b, k) of occ_runs_np."""
    ro, rd = np.asarray(ro, f32).reshape(-1, 3), np.asarray(rd, f32).reshape(-1, 3)
    R = ro.shape[0]
    step = f32(step)
    _, _, _, steps = occ_walk_np(ro, rd, near, far, cells, lo, hi, inv, h)
    ray, a, b = occ_runs_np(steps, R)
    with np.errstate(all='ignore'):
        d = rd[ray]
        nrm = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        ln = (b - a) * nrm
        k = np.where(ln > 0, np.minimum(np.maximum(np.ceil(ln / step), f32(1)), f32(RUN_MAX)), f32(0)).astype(np.int64)
        dt_run = (b - a) / np.maximum(k, 1).astype(f32)
    count = np.bincount(ray, weights=k, minlength=R).astype(np.int32)
    ray_off = np.concatenate([[0], np.cumsum(count.astype(np.int64))])
    n = int(ray_off[-1])
    run_of = np.repeat(np.arange(len(k)), k)
    first = np.concatenate([[0], np.cumsum(k)])[:-1]
    j = (np.arange(n) - first[run_of]).astype(f32)
    uu = f32(0.5) if u is None else np.asarray(u, f32)
    dt = dt_run[run_of].astype(f32)
    t = (a[run_of] + (j + uu) * dt).astype(f32)
    ray_id = ray[run_of].astype(np.int32)
    pts = (ro[ray_id] + rd[ray_id] * t[:, None]).astype(f32)
    return count, ray_off, ray_id, t, dt, pts, (ray, a, b, k)


def march_bound(G, lo, hi, step):
    """The bound of DESIGN section 4g on a ray's count: floor(D / step * (1 + 2^-15)) + (3G + 4) // 2 + 1, D the box diagonal."""
    lo = np.broadcast_to(np.asarray(lo, f32), (3,)).astype(np.float64)
    hi = np.broadcast_to(np.asarray(hi, f32), (3,)).astype(np.float64)
    D = float(np.sqrt(np.sum((hi - lo) ** 2)))
    return int(np.floor(D / float(step) * (1.0 + 2.0 ** -15))) + (3 * G + 4) // 2 + 1


# ---- inputs shared with the GPU tests ---------------------------------------------------------------------------------------------------
def march_cases():
    """(name, G, cells uint8 [G,G,G], R, seed): R in {1, 65, 300}, G in {1, 4, 32}, random masks of density 0.02 / 0.5, all ones, all
    zeros.  The rays come from test_occupancy_mesh_cpu.span_rays (axis-parallel rays, origins inside the box, misses, a NaN direction,
    an infinite origin, a zero direction)."""
    out = []
    for G in (1, 4, 32):
        for R in (1, 65, 300):
            rng = np.random.default_rng(100 * G + R)
            for dens in (0.02, 0.5):
                out.append((f"G{G}-R{R}-p{dens}", G, (rng.random((G, G, G)) < dens).astype(np.uint8), R, 7 * G + R))
        out.append((f"G{G}-ones", G, np.ones((G, G, G), np.uint8), 65, G))
        out.append((f"G{G}-zeros", G, np.zeros((G, G, G), np.uint8), 65, G + 1))
    return out


def march_steps(G, lo=-1.0, hi=1.0):
    """The steps of the case set: h/2, 3h, and one longer than the box diagonal."""
    h = (f32(hi) - f32(lo)) / f32(G)
    return [float(h / f32(2)), float(f32(3) * h), 4.0 * (hi - lo)]


# ---- the packed compositing formula ---------------------------------------------------------------------------------------------------------
def restate_packed(raw, t, dt, rays_d, ray_off, noise=None, white_bkgd=False):
    """raw2outputs on ragged lists in plain torch, in the dtype of `raw`: per ray the formula of nerf-pytorch with dist = dt * |d| (no 1e10
    distance).  A ray without samples: acc = depth = 0, rgb 0 or 1, disp = 0/0 (NaN).  -> (rgb, disp, acc, weights [n], depth)."""
    R = rays_d.shape[0]
    off = [int(x) for x in ray_off]
    nrm = torch.norm(rays_d, dim=-1)
    rgbs, accs, deps, ws = [], [], [], []
    for r in range(R):
        s = slice(off[r], off[r + 1])
        dist = dt[s] * nrm[r]
        sigma = raw[s, 3] if noise is None else raw[s, 3] + noise[s]
        alpha = 1. - torch.exp(-torch.relu(sigma) * dist)
        T = torch.cumprod(torch.cat([torch.ones_like(alpha[:1]), 1. - alpha + 1e-10], -1), -1)[:-1]
        w = alpha * T
        rgbs.append((w[:, None] * torch.sigmoid(raw[s, :3])).sum(0)); accs.append(w.sum()); deps.append((w * t[s]).sum()); ws.append(w)
    rgb, acc, depth = torch.stack(rgbs), torch.stack(accs), torch.stack(deps)
    disp = 1. / torch.max(1e-10 * torch.ones_like(depth), depth / acc)
    if white_bkgd:
        rgb = rgb + (1. - acc[:, None])
    return rgb, disp, acc, torch.cat(ws) if ws else raw[:, 3], depth


def packed_autograd_grad(raw, t, dt, d, ray_off, noise, white, grads, dtype=torch.float64):
    """d(sum_k <g_k, out_k>)/d raw by autograd of restate_packed in `dtype`; on a ray with acc == 0 the disp term is left out (as
    test_raymarch_train_cpu.autograd_grad does)."""
    c = lambda x: None if x is None else x.to(dtype)
    x = raw.detach().to(dtype, copy=True).requires_grad_(True)
    rgb, _, acc, w, depth = restate_packed(x, c(t), c(dt), c(d), ray_off, c(noise), white)
    g_rgb, g_disp, g_acc, g_w, g_depth = [c(g) for g in grads]
    loss = x.sum() * 0
    for g, o in ((g_rgb, rgb), (g_acc, acc), (g_w, w), (g_depth, depth)):
        if g is not None:
            loss = loss + (g * o).sum()
    if g_disp is not None:
        live = acc.detach() != 0
        disp = 1. / torch.clamp(depth[live] / acc[live], min=1e-10)
        loss = loss + (g_disp[live] * disp).sum()
    loss.backward()
    return x.grad


def packed_closed_form(raw, t, dt, d, ray_off, noise, white, grads):
    """The closed form `ctx_raymarch_packed_bwd` implements (DESIGN section 4d with dist = dt * |d|), float64 torch without autograd."""
    f = lambda x: None if x is None else x.double()
    raw, t, dt, d, noise = f(raw), f(t), f(dt), f(d), f(noise)
    R, n = d.shape[0], raw.shape[0]
    g_rgb, g_disp, g_acc, g_w, g_depth = [f(g) for g in grads]
    zero = lambda *s: torch.zeros(*s, dtype=torch.float64)
    g_rgb = zero(R, 3) if g_rgb is None else g_rgb
    g_disp = zero(R) if g_disp is None else g_disp
    g_acc = zero(R) if g_acc is None else g_acc
    g_w = zero(n) if g_w is None else g_w
    g_depth = zero(R) if g_depth is None else g_depth
    out = zero(n, 4)
    off = [int(x) for x in ray_off]
    for r in range(R):
        s = slice(off[r], off[r + 1])
        if off[r + 1] == off[r]:
            continue
        dist = dt[s] * d[r].norm()
        pre = raw[s, 3] if noise is None else raw[s, 3] + noise[s]
        e = torch.exp(-torch.relu(pre) * dist)
        alpha = 1. - e
        tt = 1. - alpha + 1e-10
        T = torch.cumprod(torch.cat([torch.ones(1, dtype=torch.float64), tt]), -1)[:-1]
        w = alpha * T
        c = torch.sigmoid(raw[s, :3])
        acc, depth = w.sum(), (w * t[s]).sum()
        q = depth / acc if acc != 0 else torch.tensor(0., dtype=torch.float64)
        hasq = bool(acc != 0) and bool(q > 1e-10)
        gq = -g_disp[r] / q ** 2 if hasq else torch.tensor(0., dtype=torch.float64)
        gd = g_depth[r] + (gq / acc if hasq else 0.)
        ga = g_acc[r] - (gq * depth / acc ** 2 if hasq else 0.) - (g_rgb[r].sum() if white else 0.)
        G = (g_rgb[r][None, :] * c).sum(-1) + gd * t[s] + ga + g_w[s]
        P = G * w
        X = torch.cat([torch.flip(torch.cumsum(torch.flip(P, [-1]), -1), [-1])[1:], zero(1)])
        out[s, :3] = w[:, None] * g_rgb[r][None, :] * c * (1. - c)
        out[s, 3] = torch.where(pre > 0, (G * T - X / tt) * dist * e, torch.zeros_like(pre))
    return out


def make_packed_case(counts, seed, with_noise=False):
    """Ragged lists with the given per-ray counts: raw = randn * 2, t ascending in [2, 6] per ray, dt in (0, 0.1], d = randn; the first
    ray with at least 3 samples is opaque mid-ray (raw.w = 1e4), the next has every raw.w < 0 (acc == 0)."""
    g = torch.Generator().manual_seed(seed)
    counts = [int(c) for c in counts]
    R, n = len(counts), sum(counts)
    ray_off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64)
    raw = torch.randn(n, 4, generator=g) * 2
    t = torch.cat([torch.sort(torch.rand(c, generator=g) * 4 + 2).values for c in counts]) if n else torch.zeros(0)
    dt = torch.rand(n, generator=g) * 0.1 + 1e-3
    d = torch.randn(R, 3, generator=g)
    noise = torch.randn(n, generator=g) if with_noise else None
    big = [r for r, c in enumerate(counts) if c >= 3]
    if big:
        raw[int(ray_off[big[0]]) + counts[big[0]] // 2, 3] = 1e4
    if len(big) > 1:
        s = slice(int(ray_off[big[1]]), int(ray_off[big[1] + 1]))
        raw[s, 3] = -raw[s, 3].abs() - 0.1
        if noise is not None:
            noise[s] = -noise[s].abs()
    return raw, t, dt, d, ray_off, noise


def make_packed_grads(R, n, seed):
    g = torch.Generator().manual_seed(2000 + seed)
    return [torch.randn(R, 3, generator=g), torch.randn(R, generator=g), torch.randn(R, generator=g), torch.randn(n, generator=g),
            torch.randn(R, generator=g)]


def ray_ratio(got, want, ray_off):
    """max over the non-empty rays of max|got - want| / max|want| on the ray's rows; a ray whose reference is all zero must match exactly."""
    worst = 0.0
    off = [int(x) for x in ray_off]
    for r in range(len(off) - 1):
        if off[r + 1] == off[r]:
            continue
        g, w = got[off[r]:off[r + 1]].double(), want[off[r]:off[r + 1]].double()
        err, ref = (g - w).abs().max().item(), w.abs().max().item()
        worst = max(worst, err / ref if ref > 0 else (0.0 if err == 0 else float('inf')))
    return worst
