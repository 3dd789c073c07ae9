"""The definition of exposure compensation across painted views, in numpy: the pair statistics (csrc/viewgain.hip must equal
`view_pair_stats` bit for bit) and the gain solve (kal.solve_view_gains restates `solve_view_gains`; it does not import this file).

Statistics.  A int64 [V,4,Tc,Tc]: per view the weighted colour sums and the weight sum of a back-projection, in units of 2^-32.
Per texel p, view v, channel ch: w = A[v,3,p]; c = float32(float64(A[v,ch,p]) / float64(w)); v is valid at p when w > 0 and
lo <= c <= hi (float32 comparisons) on all three channels; q = int64(rint(c * 2^24)) in float32 (exact product, half to even).
For every ordered pair (i, j), i == j included, with both views valid at p: count[i,j] += 1, colour_sum[i,j,ch] += q_i[ch].

Solve, per channel, N = count, S = colour_sum[..., ch]: d_ij = log(S_ij / N_ij) - log(S_ji / N_ij) for i < j with N_ij > 0, d_ji = -d_ij;
minimise sum_{i<j} N_ij (l_i + d_ij - l_j)^2 + ridge sum_i N_ii l_i^2 through its normal equations M l = b,
M_ii = sum_{j != i} N_ij + ridge N_ii, M_ij = -N_ij, b_i = -sum_{j != i} N_ij d_ij, solved by numpy.linalg.lstsq (minimum norm where
M is singular); gains = clip(exp(l), 1 / max_gain, max_gain)."""
import numpy as np

Q_ONE = 2 ** 24


def view_pair_stats(A, lo=0.02, hi=0.98):
    """-> (count int64 [V,V], colour_sum int64 [V,V,3])."""
    A = np.asarray(A)
    assert A.dtype == np.int64 and A.ndim == 4 and A.shape[1] == 4 and A.shape[2] == A.shape[3]
    V = A.shape[0]
    lo, hi = np.float32(lo), np.float32(hi)
    A = A.reshape(V, 4, -1)
    w = A[:, 3]
    has = w > 0
    c = (A[:, :3].astype(np.float64) / np.where(has, w, 1).astype(np.float64)[:, None]).astype(np.float32)
    valid = has & ((c >= lo) & (c <= hi)).all(axis=1)                                     # [V,P]
    q = np.rint(np.where(valid[:, None], c, np.float32(0)) * np.float32(Q_ONE)).astype(np.int64)   # [V,3,P]
    count = np.zeros((V, V), np.int64)
    colour_sum = np.zeros((V, V, 3), np.int64)
    for i in range(V):
        for j in range(V):
            both = valid[i] & valid[j]
            count[i, j] = int(both.sum())
            colour_sum[i, j] = q[i][:, both].sum(axis=1)
    return count, colour_sum


def solve_view_gains(count, colour_sum, ridge=0.01, max_gain=2.0):
    """-> gains float64 [V,3]."""
    N = np.asarray(count).astype(np.float64)
    S = np.asarray(colour_sum).astype(np.float64)
    V = N.shape[0]
    gains = np.ones((V, 3), np.float64)
    for ch in range(3):
        M = np.zeros((V, V), np.float64)
        b = np.zeros(V, np.float64)
        for i in range(V):
            M[i, i] = ridge * N[i, i]
            for j in range(V):
                if j == i or not N[i, j] > 0:
                    continue
                a, c = (i, j) if i < j else (j, i)
                d = np.log(S[a, c, ch] / N[a, c]) - np.log(S[c, a, ch] / N[a, c])          # d_ac, a < c
                d = d if i < j else -d
                M[i, i] += N[i, j]
                M[i, j] = -N[i, j]
                b[i] -= N[i, j] * d
        l = np.linalg.lstsq(M, b, rcond=None)[0]
        gains[:, ch] = np.clip(np.exp(l), 1.0 / max_gain, max_gain)
    return gains


def make_atlases(texture, gains, masks, weight=2 ** 32):
    """A [V,4,Tc,Tc] int64 of one texture [3,Tc,Tc] seen by V views with gains [V,3] on the texels of masks [V,Tc,Tc] (bool), every
    valid texel at the weight `weight` (an integer or an int64 array [V,Tc,Tc], units of 2^-32)."""
    texture, gains, masks = np.asarray(texture, np.float64), np.asarray(gains, np.float64), np.asarray(masks, bool)
    V, Tc = masks.shape[0], masks.shape[-1]
    w = np.broadcast_to(np.asarray(weight, np.int64), (V, Tc, Tc)) * masks
    A = np.zeros((V, 4, Tc, Tc), np.int64)
    A[:, 3] = w
    A[:, :3] = np.rint(texture[None] * gains[:, :, None, None] * w[:, None].astype(np.float64)).astype(np.int64)
    return A
