"""The definition of the ray / mesh intersector: numpy restatements in binary32 of the cell triangle lists
(`ctx_mesh_cells_count` / `_scan` / `_fill`), the triangle records (`ctx_mesh_tri_setup`) and the hit rule (`ctx_mesh_ray_hit`), in two
forms: the walk over the grid with its early stop, and the same arithmetic over all triangles.  csrc/meshhit.hip is held to the first form
with array_equal; the second says what the first must find.  Not a test module: tests/test_meshhit_cpu.py and tests/test_meshhit_gpu.py
import it.

The lists come from `occ_voxelize_np` face by face: (cell, face) is listed if and only if the voxeliser marks that cell for that face alone.
The walk here is `occ_ray_spans_np`'s, expression for expression, and also hands out the flat index of every cell it visits (which that
function keeps to itself); test_meshhit_cpu.py checks that the spans read off this walk are `occ_ray_spans_np`'s, bit for bit.
All float arithmetic is binary32 in the order written (numpy rounds every product, sum and quotient on its own)."""
import numpy as np

from test_occupancy_cpu import grid_consts                                                       # noqa: F401  (shared with the tests)
from test_occupancy_mesh_cpu import (occ_voxelize_np, occ_ray_spans_np, icosphere, spot_mesh, random_triangles, triangles_to_mesh,  # noqa: F401
                                     span_rays, KINDS)

f32 = np.float32
EPS = 2.0 ** -18                         # the slack of the barycentric test


# ---- lists ---------------------------------------------------------------------------------------------------------------------------
def mesh_cells_np(vertices, faces, G, lo, inv):
    """-> (count int32 [G^3], cell_off int32 [G^3 + 1], cell_tri int32 [n]): cell (cz*G + cy)*G + cx owns cell_off[c] .. cell_off[c+1] of
    cell_tri, the faces the voxeliser marks that cell for, ascending by face id."""
    v = np.asarray(vertices, f32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    cc, ff = [], []
    for i, tri in enumerate(faces):
        if np.any(tri < 0) or np.any(tri >= len(v)):
            continue
        c = np.flatnonzero(occ_voxelize_np(v[tri], [[0, 1, 2]], G, lo, inv).reshape(-1))          # the same three vertices, the same bits
        cc.append(c); ff.append(np.full(len(c), i, np.int64))
    cell = np.concatenate(cc) if cc else np.zeros(0, np.int64)
    face = np.concatenate(ff) if ff else np.zeros(0, np.int64)
    order = np.lexsort((face, cell))
    count = np.bincount(cell, minlength=G ** 3).astype(np.int32)
    cell_off = np.concatenate([[0], np.cumsum(count, dtype=np.int64)]).astype(np.int32)
    return count, cell_off, face[order].astype(np.int32)


def tri_records_np(vertices, faces, dtype=f32):
    """-> tri [F,12]: v0, e1 = v1 - v0, e2 = v2 - v0, each padded with a 0 to four numbers; twelve NaN for a face with an index outside
    [0, V) or a non-finite vertex.  dtype=float64 gives the reference's records (of the same binary32 vertices)."""
    v = np.asarray(vertices, f32).reshape(-1, 3).astype(dtype)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    rec = np.full((len(faces), 12), np.nan, dtype)
    ok = np.all((faces >= 0) & (faces < len(v)), 1)
    idx = np.flatnonzero(ok)
    with np.errstate(all='ignore'):
        p = v[faces[idx]]
        fin = np.all(np.isfinite(p), (1, 2))
        idx, p = idx[fin], p[fin]
        rec[idx] = 0
        rec[idx, 0:3], rec[idx, 4:7], rec[idx, 8:11] = p[:, 0], p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    return rec


# ---- the triangle test ---------------------------------------------------------------------------------------------------------------
def tri_terms_np(o, d, rec, dtype=f32):
    """-> (det, inv, u, v, t) of rays o, d [..., 3] against records rec [..., 12] (broadcast): p = d x e2, det = e1.p, inv = 1/det,
    s = o - v0, u = (s.p)*inv, q = s x e1, v = (d.q)*inv, t = (e2.q)*inv; dots are (ax*bx + ay*by) + az*bz."""
    o, d, rec = np.asarray(o, dtype), np.asarray(d, dtype), np.asarray(rec, dtype)
    ox, oy, oz, dx, dy, dz = o[..., 0], o[..., 1], o[..., 2], d[..., 0], d[..., 1], d[..., 2]
    v0x, v0y, v0z, e1x, e1y, e1z, e2x, e2y, e2z = (rec[..., k] for k in (0, 1, 2, 4, 5, 6, 8, 9, 10))
    with np.errstate(all='ignore'):
        px, py, pz = dy * e2z - dz * e2y, dz * e2x - dx * e2z, dx * e2y - dy * e2x
        det = (e1x * px + e1y * py) + e1z * pz
        inv = dtype(1) / det
        sx, sy, sz = ox - v0x, oy - v0y, oz - v0z
        u = ((sx * px + sy * py) + sz * pz) * inv
        qx, qy, qz = sy * e1z - sz * e1y, sz * e1x - sx * e1z, sx * e1y - sy * e1x
        v = ((dx * qx + dy * qy) + dz * qz) * inv
        t = ((e2x * qx + e2y * qy) + e2z * qz) * inv
    return det, inv, u, v, t


def tri_test_np(o, d, rec, near, far, dtype=f32):
    """-> (accepted bool, t, u, v).  Miss if det == 0, or if inv or t is not finite; accepted if and only if u >= -EPS, v >= -EPS,
    u + v <= 1 + EPS and near <= t <= far.  Two-sided."""
    det, inv, u, v, t = tri_terms_np(o, d, rec, dtype)
    eps, one = dtype(EPS), dtype(1)
    with np.errstate(all='ignore'):
        ok = (det != 0) & np.isfinite(inv) & np.isfinite(t)
        ok &= (u >= -eps) & (v >= -eps) & (u + v <= one + eps) & (t >= dtype(near)) & (t <= dtype(far))
    return ok, t, u, v


def related_np(faces, own, cand):
    """bool per pair: face cand[k] is own[k] or shares a vertex id with it in `faces` (the integer rule of csrc/uvgather.hip); an own
    outside [0, F) relates to nothing."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    own, cand = np.asarray(own, np.int64), np.asarray(cand, np.int64)
    valid = (own >= 0) & (own < len(faces))
    a, b = faces[np.where(valid, own, 0)], faces[cand]
    return valid & ((cand == own) | np.any(b[..., :, None] == a[..., None, :], (-1, -2)))


# ---- the same arithmetic over all triangles ----------------------------------------------------------------------------------------------
def mesh_hit_all_np(ro, rd, near, far, tri, faces, own_face=None, dtype=f32, chunk=128):
    """-> (hit uint8 [R], t [R], face int32 [R], uv [R,2]): every ray against every triangle; the lowest t, ties to the lower face id.
    A miss: hit = 0, t = far, face = -1, uv = 0."""
    ro, rd = np.asarray(ro, f32).reshape(-1, 3), np.asarray(rd, f32).reshape(-1, 3)
    R, F = len(ro), len(tri)
    hit, t_out = np.zeros(R, np.uint8), np.full(R, dtype(far), dtype)
    face, uv = np.full(R, -1, np.int32), np.zeros((R, 2), dtype)
    for r0 in range(0, R, chunk):
        sl = slice(r0, min(R, r0 + chunk))
        ok, t, u, v = tri_test_np(ro[sl, None, :], rd[sl, None, :], tri[None], near, far, dtype)
        if own_face is not None:
            own = np.asarray(own_face, np.int64)[sl]
            ok &= ~related_np(faces, np.broadcast_to(own[:, None], ok.shape), np.broadcast_to(np.arange(F)[None], ok.shape))
        tt = np.where(ok, t, dtype(np.inf))
        best = np.argmin(tt, 1)                                       # the first minimum: the lower face id on a tie
        rows = np.arange(ok.shape[0])
        got = ok[rows, best]
        hit[sl] = got
        t_out[sl] = np.where(got, t[rows, best], dtype(far))
        face[sl] = np.where(got, best, -1)
        uv[sl, 0], uv[sl, 1] = np.where(got, u[rows, best], 0), np.where(got, v[rows, best], 0)
    return hit, t_out, face, uv


# ---- the walk, with the cell index ---------------------------------------------------------------------------------------------------------
def walk_cells_np(ro, rd, near, far, cells, lo, hi, inv, h):
    """The walk of `occ_ray_spans_np`, vectorised over the rays -> steps, a list of (occ bool [R], cell int64 [R], t_in [R], t_out [R]) in
    walk order: `occ` marks the rays that look at an occupied cell in that step, `cell` = (cz*G + cy)*G + cx is the cell each ray looks at.
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
            steps.append((active & (cells[c[2], c[1], c[0]] != 0), (c[2] * G + c[1]) * G + c[0], tin.copy(), tout.copy(), active.copy()))
            active = active & ~(te >= tb)
            for k in range(3):
                nxt = c[k] + np.where(rd[:, k] > 0, 1, -1)
                move = active & (ax == k)
                active = active & ~(move & ((nxt < 0) | (nxt > G - 1)))
                c[k] = np.where(move & active, nxt, c[k])
            tin = tout
    return steps


def spans_from_cells_walk(steps, R, near, far):
    """(span, hit) of `occ_ray_spans_np` read off the steps of walk_cells_np."""
    s0, s1, found = np.full(R, f32(near), f32), np.full(R, f32(far), f32), np.zeros(R, bool)
    for occ, _, tin, tout, _ in steps:
        s0 = np.where(occ & ~found, tin, s0)
        s1 = np.where(occ, tout, s1)
        found |= occ
    return np.stack([s0, s1], -1).astype(f32), found.astype(np.uint8)


# ---- the grid form: what ctx_mesh_ray_hit computes ---------------------------------------------------------------------------------------
def mesh_hit_grid_np(ro, rd, near, far, lists, tri, faces, G, lo, hi, inv, h, own_face=None, mode=0, stats=None):
    """-> (hit uint8 [R], t float32 [R], face int32 [R], uv float32 [R,2]).  lists = (count, cell_off, cell_tri) of mesh_cells_np; the walk
    runs on cells = (count > 0).  In every occupied cell the listed triangles are tested (tri_test_np); own_face [R] (optional) skips the
    related ones (related_np).
    mode 0: per ray the best (t, face) is the lowest t, ties to the lower face id; a triangle seen in any cell counts with its t wherever
    that lies; after every cell of the walk the ray stops when best.t <= t_out of that cell.  A miss: hit = 0, t = far, face = -1, uv = 0.
    mode 1: the ray stops at its first accepted triangle; only hit means anything (the rest is returned as for a miss)."""
    count, cell_off, cell_tri = (np.asarray(x, np.int64) for x in lists)
    ro, rd = np.asarray(ro, f32).reshape(-1, 3), np.asarray(rd, f32).reshape(-1, 3)
    R = len(ro)
    cells = (count > 0).reshape(G, G, G).astype(np.uint8)
    found = np.zeros(R, bool)
    bt, bu, bv, bf = np.full(R, f32(far), f32), np.zeros(R, f32), np.zeros(R, f32), np.full(R, -1, np.int64)
    live = np.ones(R, bool)
    n_tests = 0
    for occ, cell, tin, tout, visit in walk_cells_np(ro, rd, near, far, cells, lo, hi, inv, h):
        idx = np.flatnonzero(live & occ)
        if idx.size:
            k0 = cell_off[cell[idx]]
            ln = cell_off[cell[idx] + 1] - k0
            rr = np.repeat(idx, ln)
            kk = np.repeat(k0 - (np.cumsum(ln) - ln), ln) + np.arange(int(ln.sum()))
            ff = cell_tri[kk]
            n_tests += len(ff)
            ok, t, u, v = tri_test_np(ro[rr], rd[rr], tri[ff], near, far)
            if own_face is not None:
                ok &= ~related_np(faces, np.asarray(own_face, np.int64)[rr], ff)
            rr, ff, t, u, v = rr[ok], ff[ok], t[ok], u[ok], v[ok]
            if mode == 1:
                found[rr] = True
            elif len(rr):
                order = np.lexsort((ff, t, rr))                        # per ray: lowest t first, then the lower face id
                rr, ff, t, u, v = rr[order], ff[order], t[order], u[order], v[order]
                first = np.concatenate([[True], rr[1:] != rr[:-1]])
                rr, ff, t, u, v = rr[first], ff[first], t[first], u[first], v[first]
                better = ~found[rr] | (t < bt[rr]) | ((t == bt[rr]) & (ff < bf[rr]))
                rr, ff, t, u, v = rr[better], ff[better], t[better], u[better], v[better]
                found[rr] = True
                bt[rr], bu[rr], bv[rr], bf[rr] = t, u, v, ff
        live &= ~(visit & found & ((mode == 1) | (bt <= tout)))
    if stats is not None:
        stats['tests'] = n_tests
    return found.astype(np.uint8), bt, bf.astype(np.int32), np.stack([bu, bv], -1)


# ---- which rays a float64 comparison may judge ----------------------------------------------------------------------------------------------
def judged_rays_np(ro, rd, near, far, tri64, edge=1e-3, graze=1e-2, chunk=128):
    """bool [R]: False for a ray that passes within `edge` (barycentric) of an edge of any triangle inside [near, far], or that meets a
    triangle at |det| / (|e1 x e2| |d|) < graze (float64 throughout): there the accept flag, or the choice among coplanar neighbours,
    hangs on the last bits."""
    ro, rd = np.asarray(ro, np.float64).reshape(-1, 3), np.asarray(rd, np.float64).reshape(-1, 3)
    keep = np.ones(len(ro), bool)
    e1, e2 = tri64[:, 4:7], tri64[:, 8:11]
    area = np.linalg.norm(np.cross(e1, e2), axis=1)
    with np.errstate(all='ignore'):
        for r0 in range(0, len(ro), chunk):
            sl = slice(r0, min(len(ro), r0 + chunk))
            det, inv, u, v, t = tri_terms_np(ro[sl, None, :], rd[sl, None, :], tri64[None], np.float64)
            in_t = (t >= near - edge) & (t <= far + edge)
            loose = (u >= -edge) & (v >= -edge) & (u + v <= 1 + edge) & in_t
            tight = (u >= edge) & (v >= edge) & (u + v <= 1 - edge)
            cosine = np.abs(det) / (area[None] * np.linalg.norm(rd[sl], axis=1)[:, None])
            keep[sl] &= ~np.any(loose & ~tight, 1) & ~np.any(loose & ~(cosine >= graze), 1)
    return keep
