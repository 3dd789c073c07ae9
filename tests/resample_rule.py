"""The definition of the importance resampling: a numpy restatement in binary32 of `ctx_resample_packed`, the float64
piecewise-linear CDF it is judged against, the derived bounds of the contract, and the generators of the test lists.

The rule, per ray with S coarse intervals (start ts_i, width dt_i, weight w_i) and K fine samples:
  m_i = min(max(w_i, 0), 1) + 1e-5 (NaN -> 0, +inf -> 1); C, l = exclusive prefix sums of m and dt, W, L their totals;
  at u: tau = u*W, i = the last interval with C_i <= tau, f = clamp((tau - C_i)/m_i, 0, 1);
  t'_k = ts_i + f*dt_i at u = (k + xi_k)/K;  dt'_k = l((k+1)/K) - l(k/K) with l(u) = min(l_i + f*dt_i, l_{i+1}), l(0) = 0, l(1) = L.
The prefix sums are made non-descending by a running maximum.  With order='seq' (plain sequential sums, the definition) the maximum and the
min in l(u) are identities: fl(l_i + fl(f*dt_i)) <= fl(l_i + dt_i) = l_{i+1}.  order='wave' adds in the kernel's order (64-lane chunks, a
4-level tree inside each 16-lane row, then the rows, chunks chained by a carried scalar), where both do work.  The two orders, and the
kernel, differ in the last bits and near a boundary in the chosen interval, so none is compared to another element-wise: the contract is
`contract_ratios`, stated in mass."""
import numpy as np

f32 = np.float32
FLOOR = f32(1e-5)
MAX_K = 4096


def masses(w):
    w = np.asarray(w, f32)
    with np.errstate(invalid='ignore'):
        c = np.where(w > 0, w, f32(0))
        c = np.where(c < 1, c, f32(1))
    return (c + FLOOR).astype(f32)


def clamped(w):
    """The weights the rule sees: NaN and negatives as 0, everything above 1 (+inf too) as 1."""
    w = np.asarray(w, f32)
    with np.errstate(invalid='ignore'):
        c = np.where(w > 0, w, f32(0))
        return np.where(c < 1, c, f32(1)).astype(f32)


def _wave_scan(v):
    """Inclusive sum of 64 binary32 values in the order of wave_scan<scan_sum> (row_shr 1, 2, 4, 8, row_bcast 15, row_bcast 31)."""
    x = v.astype(f32).copy()
    lane = np.arange(64)
    for s in (1, 2, 4, 8):
        has = (lane % 16) >= s
        y = x.copy()
        y[has] = x[has] + x[lane[has] - s]
        x = y
    x[16:32] = x[16:32] + x[15]
    x[48:64] = x[48:64] + x[47]
    x[32:64] = x[32:64] + x[31]
    return x


def prefix(v, order='seq'):
    """-> (exclusive [S], inclusive [S], total) non-descending binary32 prefix sums of v >= 0."""
    v = np.asarray(v, f32)
    S = len(v)
    if order == 'seq':
        inc = np.maximum.accumulate(np.cumsum(v, dtype=f32))
    else:
        inc = np.empty(S, f32)
        carry = f32(0)
        for c0 in range(0, S, 64):
            chunk = np.zeros(64, f32)
            k = min(64, S - c0)
            chunk[:k] = v[c0:c0 + k]
            full = np.maximum.accumulate((carry + _wave_scan(chunk)).astype(f32))
            inc[c0:c0 + k] = full[:k]
            carry = full[63]
    ex = np.concatenate([f32([0]), inc[:-1]])
    return ex, inc, inc[-1] if order == 'seq' else carry


def _invert(tau, Cex, m):
    i = np.clip(np.searchsorted(Cex, tau, 'right') - 1, 0, len(Cex) - 1)
    with np.errstate(invalid='ignore'):
        f = (tau - Cex[i]) / m[i]
        f = np.where(f > 0, f, f32(0))
        f = np.where(f < 1, f, f32(1)).astype(f32)
    return i, f


def resample_np(w, ts, dt, ray_off, ro, rd, K, xi=None, order='seq'):
    """-> (fine_off int64 [R+1], ray_id int32 [n'], t' [n'], dt' [n'], pts [n',3]); xi [n'] in [0,1) or None for 0.5."""
    w, ts, dt, ro, rd = (np.asarray(a, f32) for a in (w, ts, dt, ro, rd))
    R = len(ray_off) - 1
    count = np.diff(ray_off)
    fine_off = np.concatenate([[0], np.cumsum(count > 0) * K]).astype(np.int64)
    n1 = int(fine_off[-1])
    ray_id, t1, dt1, pts = np.empty(n1, np.int32), np.empty(n1, f32), np.empty(n1, f32), np.empty((n1, 3), f32)
    Kf = f32(K)
    for r in range(R):
        if count[r] == 0:
            continue
        s, o = slice(ray_off[r], ray_off[r + 1]), slice(fine_off[r], fine_off[r + 1])
        m = masses(w[s])
        Cex, _, W = prefix(m, order)
        Lex, Lin, Ltot = prefix(dt[s], order)
        k = np.arange(K).astype(f32)
        x = f32(0.5) if xi is None else np.asarray(xi, f32)[o]
        i, f = _invert(((k + x) / Kf) * W, Cex, m)
        t1[o] = ts[s][i] + f * dt[s][i]
        i, f = _invert((np.arange(K + 1).astype(f32) / Kf) * W, Cex, m)
        edge = np.minimum(Lex[i] + f * dt[s][i], Lin[i]).astype(f32)
        edge[0], edge[K] = f32(0), Ltot
        dt1[o] = edge[1:] - edge[:-1]
        ray_id[o] = r
        pts[o] = ro[r] + rd[r] * t1[o][:, None]
    return fine_off, ray_id, t1, dt1, pts


# ---- the float64 CDF and the contract -------------------------------------------------------------------------------------------------------
def masses64(w):
    return clamped(w).astype(np.float64) + np.float64(FLOOR)


def cdf(knots, width, m64, x):
    """The piecewise-linear CDF through the intervals [knots_i, knots_i + width_i] of mass m64_i, at x (float64): flat in a gap."""
    C = np.concatenate([[0.0], np.cumsum(m64)])
    i = np.clip(np.searchsorted(knots, x, 'right') - 1, 0, len(knots) - 1)
    with np.errstate(divide='ignore', invalid='ignore'):
        f = np.where(width[i] > 0, (x - knots[i]) / width[i], 1.0)
    return (C[i] + np.clip(f, 0.0, 1.0) * m64[i]) / C[-1], i


def _modulus(knots, width, m64, x, delta):
    """How far the CDF moves within delta of x, the larger side."""
    F = cdf(knots, width, m64, x)[0]
    return np.maximum(cdf(knots, width, m64, x + delta)[0] - F, F - cdf(knots, width, m64, x - delta)[0])


def prefix_depth(S, order):
    """The roundings a binary32 prefix of S terms has seen: S - 1 in a sequential sum; in the kernel's order six levels of the tree inside a
    chunk and one addition of the carry per chunk."""
    return S - 1 if order == 'seq' else min(S - 1, -(-S // 64) + 6)


def starts_np(t, dt, u=None):
    """The interval starts OccupancyGrid.march(starts=True) returns: ts = t - u*dt in binary32, u = 0.5 without jitter."""
    t, dt = np.asarray(t, f32), np.asarray(dt, f32)
    return (t - (f32(0.5) if u is None else np.asarray(u, f32)) * dt).astype(f32)


def contract_ratios(w, ts, dt, ray_off, fine_off, t1, dt1, K, xi=None, order='seq'):
    """The contract of DESIGN section 4i for every hit ray -> (largest error / bound of (a), of (b), largest error of (b) / B alone).
    (a) |F_t(t'_k) - (k + xi_k)/K| <= B + omega_t(t'_k, 2^-22 * (|t'_k| + dt_i))
    (b) |F_l(sum_{j<=k} dt'_j) - (k+1)/K| <= B + omega_l(., (depth + 3) * 2^-24 * L)
    with B = (S+8) * 2^-23, omega(x, delta) how far F moves within delta of x (delta * m_i / (dt_i * W) inside an interval) and depth =
    prefix_depth(S, order), the roundings in a prefix of dt: order='seq' for the sequential restatement, 'wave' for the kernel and the
    restatement in its order, which is held to the far smaller displacement."""
    ra = rb = rB = 0.0
    for r in range(len(ray_off) - 1):
        S = int(ray_off[r + 1] - ray_off[r])
        if S == 0:
            assert fine_off[r + 1] == fine_off[r]
            continue
        s, o = slice(ray_off[r], ray_off[r + 1]), slice(fine_off[r], fine_off[r + 1])
        assert fine_off[r + 1] - fine_off[r] == K
        m64, ts64, dt64 = masses64(w[s]), ts[s].astype(np.float64), dt[s].astype(np.float64)
        B = (S + 8) * 2.0 ** -23
        k = np.arange(K, dtype=np.float64)
        x = 0.5 if xi is None else np.asarray(xi)[o].astype(np.float64)
        tq = t1[o].astype(np.float64)
        F, i = cdf(ts64, dt64, m64, tq)
        bound = B + _modulus(ts64, dt64, m64, tq, 2.0 ** -22 * (np.abs(tq) + dt64[i]))
        ra = max(ra, float(np.max(np.abs(F - (k + x) / K) / bound)))
        l64 = np.concatenate([[0.0], np.cumsum(dt64)])
        cum = np.cumsum(dt1[o].astype(np.float64))
        F, _ = cdf(l64[:-1], dt64, m64, cum)
        bound = B + _modulus(l64[:-1], dt64, m64, cum, (prefix_depth(S, order) + 3) * 2.0 ** -24 * l64[-1])
        rb = max(rb, float(np.max(np.abs(F - (k + 1) / K) / bound)))
        rB = max(rB, float(np.max(np.abs(F - (k + 1) / K) / B)))
    return ra, rb, rB


# ---- test lists -----------------------------------------------------------------------------------------------------------------------------
SHAPES = ('peaky', 'flat', 'zero', 'random')


def make_weights(rng, S, shape):
    if shape == 'peaky':                                      # a narrow bump, as the weights of a surface
        c, sig = rng.uniform(0, S), rng.uniform(0.4, 2.0)
        w = 0.9 * np.exp(-0.5 * ((np.arange(S) + 0.5 - c) / sig) ** 2)
    elif shape == 'flat':
        w = np.full(S, 1.0 / S)
    elif shape == 'zero':
        w = np.zeros(S)
    else:
        w = rng.random(S) * (2.0 / S)
    return w.astype(f32)


def make_intervals(rng, S, runs):
    """S intervals in `runs` runs (fewer if S is smaller) separated by gaps, starting near t = 0.6 and spanning about 1.5 in all: inside a
    run the width is constant and ts_j = a + j*dt in binary32, as the march leaves them."""
    runs = max(1, min(runs, S))
    cuts = np.sort(rng.choice(np.arange(1, S), runs - 1, replace=False)) if runs > 1 else np.array([], int)
    sizes = np.diff(np.concatenate([[0], cuts, [S]]))
    ts, dt = [], []
    a = f32(rng.uniform(0.55, 0.7))
    for k in sizes:
        d = f32(rng.uniform(0.5, 1.0) * 1.5 / S)
        ts.append((a + np.arange(k).astype(f32) * d).astype(f32))
        dt.append(np.full(k, d, f32))
        a = f32(ts[-1][-1] + d + f32(rng.uniform(0.05, 0.2)))
    return np.concatenate(ts), np.concatenate(dt)


def make_lists(counts, seed, shapes=SHAPES, runs=(1, 2, 3)):
    """Ragged lists of the given per-ray counts: ray r takes shapes[r % len] and runs[r % len] -> (w, ts, dt, ray_off, ro, rd)."""
    rng = np.random.default_rng(seed)
    W, T, D = [], [], []
    for r, S in enumerate(counts):
        if S == 0:
            continue
        W.append(make_weights(rng, S, shapes[r % len(shapes)]))
        ts, dt = make_intervals(rng, S, runs[(r // len(shapes)) % len(runs)])
        T.append(ts)
        D.append(dt)
    ray_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    R = len(counts)
    ro = rng.uniform(-1, 1, (R, 3)).astype(f32)
    rd = rng.normal(size=(R, 3)).astype(f32)
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, f32)
    return cat(W), cat(T), cat(D), ray_off, ro, rd


def in_coarse_interval(ts, dt, t1, ulps=2):
    """Every t1 lies in a closed interval [ts_i, ts_i + dt_i] of the ray, widened by `ulps` binary32 ulps of |t1|."""
    ts64, dt64, x = ts.astype(np.float64), dt.astype(np.float64), t1.astype(np.float64)
    slack = ulps * np.spacing(np.abs(t1).astype(f32)).astype(np.float64)
    i = np.clip(np.searchsorted(ts64, x, 'right') - 1, 0, len(ts) - 1)
    ok = np.zeros(len(x), bool)
    for j in (np.maximum(i - 1, 0), i, np.minimum(i + 1, len(ts) - 1)):
        ok |= (x >= ts64[j] - slack) & (x <= ts64[j] + dt64[j] + slack)
    return ok
