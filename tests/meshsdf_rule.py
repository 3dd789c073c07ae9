"""The definition of the signed point / mesh query: numpy restatements in binary32, on top of tests/meshdist_rule.py,
of the pseudonormal tables (`ctx_mesh_pseudonormals`), of the feature code of the closest point on a triangle, of
`ctx_mesh_signed_distance` in grid form and in all-triangles form (the latter also in float64), of MeshSolidField's ramp and its gradient,
and a float64 generalised winding number as the independent truth for the sign.  Not a test module: tests/test_meshsdf_cpu.py and
tests/test_meshsdf_gpu.py import it.

The sign is that of (p - q) . N with q the nearest point and N the angle-weighted pseudonormal (Baerentzen & Aanaes 2005) of the feature
of the winning face on which q lies: the face, one of its three vertices or one of its three edges.  All float arithmetic is binary32 in
the order written; the only transcendental is the arctan2 of the vertex rows."""
import numpy as np

import meshdist_rule as R

f32 = np.float32
FEATURES = ("interior", "v0", "v0+e1", "v0+e2", "edge e1", "edge e2", "edge opposite v0")
EDGES = ((0, 1), (0, 2), (1, 2))         # rows 4, 5, 6: the corners each edge joins


# ---- the tables ----------------------------------------------------------------------------------------------------------------------------
def face_normals_np(tri, dtype=f32):
    """-> (u [F,3], counts bool [F]): row 0 of the table.  n = e1 x e2 with nx = e1y*e2z - e1z*e2y, ny = e1z*e2x - e1x*e2z,
    nz = e1x*e2y - e1y*e2x; nn = (nx*nx + ny*ny) + nz*nz; u = n / sqrt(nn) per component where 0 < nn < inf, 0 elsewhere, NaN for a
    record with a NaN.  A face counts in the sums if its u is finite and not (0, 0, 0)."""
    tri = np.asarray(tri, dtype)
    e1x, e1y, e1z, e2x, e2y, e2z = (tri[:, k] for k in (4, 5, 6, 8, 9, 10))
    with np.errstate(all='ignore'):
        nx, ny, nz = e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x
        nn = (nx * nx + ny * ny) + nz * nz
        ln = np.sqrt(nn)
        good = (nn > 0) & (nn < np.inf)
        u = np.stack([np.where(good, nx / ln, 0), np.where(good, ny / ln, 0), np.where(good, nz / ln, 0)], 1).astype(dtype)
        u[np.any(np.isnan(tri[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]]), 1)] = np.nan
        counts = np.all(np.isfinite(u), 1) & np.any(u != 0, 1)
    return u, counts


def corner_angles_np(tri, dtype=f32):
    """-> alpha [F,3]: the interior angle at each corner, arctan2(|a x b|, a . b) of the two edge vectors leaving it, taken from the
    record: at v0 a = e1, b = e2; at v1 a = -e1, b = e2 - e1; at v2 a = -e2, b = e1 - e2.  |c| = sqrt((cx*cx + cy*cy) + cz*cz)."""
    tri = np.asarray(tri, dtype)
    e1, e2 = tri[:, 4:7], tri[:, 8:11]
    out = np.zeros((len(tri), 3), dtype)
    with np.errstate(all='ignore'):
        for k, (a, b) in enumerate(((e1, e2), (-e1, e2 - e1), (-e2, e1 - e2))):
            ax, ay, az, bx, by, bz = a[:, 0], a[:, 1], a[:, 2], b[:, 0], b[:, 1], b[:, 2]
            cx, cy, cz = ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx
            out[:, k] = np.arctan2(np.sqrt((cx * cx + cy * cy) + cz * cz), (ax * bx + ay * by) + az * bz)
    return out


def _ordered_sums(key, face, vals, dtype):
    """Per distinct key the sum of vals [m,3] in ascending face id, starting from 0, one rounding per addition -> (keys, sums)."""
    order = np.lexsort((face, key))
    key, vals = key[order], vals[order]
    keys, start, inverse = np.unique(key, return_index=True, return_inverse=True)
    rank = np.arange(len(key)) - start[inverse]
    sums = np.zeros((len(keys), 3), dtype)
    for k in range(int(rank.max(initial=-1)) + 1):
        sel = rank == k                                               # every key at most once: a plain vector addition
        sums[inverse[sel]] = sums[inverse[sel]] + vals[sel]
    return keys, sums


def pseudonormals_np(faces, V, tri, dtype=f32, order=None):
    """-> pn [F,7,3] of faces int64 [F,3], V vertices and the records tri [F,12] (tri_records_np):
      row 0      the unit face normal u_f (face_normals_np);
      rows 1-3   at the vertex ids faces[f,0..2]: the sum over the counting faces g that hold that id at a corner, in ascending g, of
                 alpha_g * u_g per component (alpha_g the angle of g at that corner, corner_angles_np); acc = acc + alpha*u from 0;
      rows 4-6   for the edges (v0,v1), (v0,v2), (v1,v2): the sum of u_g over the counting faces g that hold the two ids at two
                 different corners, in ascending g.
    Vertex and edge rows are not normalised.  A face with a NaN record has seven NaN rows; a face that does not count (zero area)
    contributes to no sum, and its own rows 1-6 are the sums of the others.  order (a permutation of the face ids, for the tests) visits
    the faces in that order instead of ascending."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    tri = np.asarray(tri, dtype)
    F = len(faces)
    u, counts = face_normals_np(tri, dtype)
    alpha = corner_angles_np(tri, dtype)
    g = np.flatnonzero(counts)                                        # a counting face has a finite record, hence ids in [0, V)
    visit = np.arange(F) if order is None else np.argsort(np.asarray(order))
    pn = np.zeros((F, 7, 3), dtype)
    pn[:, 0] = u
    with np.errstate(all='ignore'):
        key = faces[g].reshape(-1)
        keys, sums = _ordered_sums(key, np.repeat(visit[g], 3), (alpha[g].reshape(-1, 1) * np.repeat(u[g], 3, 0)).astype(dtype), dtype)
        table = np.zeros((V, 3), dtype)
        table[keys] = sums
        ids = np.clip(faces, 0, V - 1)
        pn[:, 1:4] = table[ids]
        ek, ef = [], []
        for a, b in EDGES:
            lo, hi = np.minimum(faces[g, a], faces[g, b]), np.maximum(faces[g, a], faces[g, b])
            ek.append(lo * V + hi); ef.append(g)
        keys, sums = _ordered_sums(np.concatenate(ek), visit[np.concatenate(ef)], np.tile(u[g], (3, 1)), dtype)
        for j, (a, b) in enumerate(EDGES):
            lo, hi = np.minimum(ids[:, a], ids[:, b]), np.maximum(ids[:, a], ids[:, b])
            k = lo * V + hi
            pos = np.searchsorted(keys, k)
            has = (pos < len(keys)) & (keys[np.minimum(pos, max(len(keys) - 1, 0))] == k) if len(keys) else np.zeros(F, bool)
            pn[:, 4 + j] = np.where(has[:, None], sums[np.minimum(pos, max(len(keys) - 1, 0))] if len(keys) else 0, 0)
    pn[np.any(np.isnan(tri[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]]), 1)] = np.nan
    return pn


def topology_np(faces, V):
    """-> dict(boundary_edges, nonmanifold_edges, inconsistent_edges): undirected edges with one face, with more than two, and with two
    faces that traverse them in the same direction.  Faces with an id outside [0, V) are left out."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    faces = faces[np.all((faces >= 0) & (faces < V), 1)]
    a = np.concatenate([faces[:, 0], faces[:, 1], faces[:, 2]])
    b = np.concatenate([faces[:, 1], faces[:, 2], faces[:, 0]])
    und, cnt = np.unique(np.minimum(a, b) * V + np.maximum(a, b), return_counts=True)
    forward = np.bincount(np.searchsorted(und, np.minimum(a, b) * V + np.maximum(a, b)), weights=(a < b), minlength=len(und))
    two = cnt == 2
    return dict(boundary_edges=int((cnt == 1).sum()), nonmanifold_edges=int((cnt > 2).sum()),
                inconsistent_edges=int((two & (forward != 1)).sum()))


# ---- the feature code ----------------------------------------------------------------------------------------------------------------------
def feature_on_tri_np(p, rec, dtype=f32):
    """-> feature uint8 of the region of closest_on_tri_np that answers (the same d1 .. d6, va, vb, vc, the first region whose condition
    holds): 1 / 2 / 3 the vertices v0, v0 + e1, v0 + e2; 4 / 5 / 6 the edges along e1, along e2 and opposite v0; 0 the interior."""
    p, rec = np.asarray(p, dtype), np.asarray(rec, dtype)
    px, py, pz = p[..., 0], p[..., 1], p[..., 2]
    v0x, v0y, v0z, e1x, e1y, e1z, e2x, e2y, e2z = (rec[..., k] for k in (0, 1, 2, 4, 5, 6, 8, 9, 10))
    with np.errstate(all='ignore'):
        apx, apy, apz = px - v0x, py - v0y, pz - v0z
        d1 = (e1x * apx + e1y * apy) + e1z * apz
        d2 = (e2x * apx + e2y * apy) + e2z * apz
        bpx, bpy, bpz = apx - e1x, apy - e1y, apz - e1z
        d3 = (e1x * bpx + e1y * bpy) + e1z * bpz
        d4 = (e2x * bpx + e2y * bpy) + e2z * bpz
        vc = d1 * d4 - d3 * d2
        cpx, cpy, cpz = apx - e2x, apy - e2y, apz - e2z
        d5 = (e1x * cpx + e1y * cpy) + e1z * cpz
        d6 = (e2x * cpx + e2y * cpy) + e2z * cpz
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        feat = np.zeros(np.broadcast(d1, d2).shape, np.uint8)                                       # the regions, last to first
        feat = np.where((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), 6, feat)
        feat = np.where((vb <= 0) & (d2 >= 0) & (d6 <= 0), 5, feat)
        feat = np.where((d6 >= 0) & (d5 <= d6), 3, feat)
        feat = np.where((vc <= 0) & (d1 >= 0) & (d3 <= 0), 4, feat)
        feat = np.where((d3 >= 0) & (d4 <= d3), 2, feat)
        feat = np.where((d1 <= 0) & (d2 <= 0), 1, feat)
    return feat.astype(np.uint8)


# ---- the signed query ----------------------------------------------------------------------------------------------------------------------
def sign_step_np(pts, r, unsigned, tri, pn, dtype=f32, face_normal_only=False):
    """The step after the minimum.  unsigned = (found, dist, face, uv) of closest_grid_np / closest_all_np.  For a found point the winning
    face is evaluated once more (the same numbers as in the loop): feature = feature_on_tri_np; q = v0 + (e1*u + e2*v), s = p - q,
    d2 = (sx*sx + sy*sy) + sz*sz; N = pn[face, feature]; dot = (sx*Nx + sy*Ny) + sz*Nz; sgn = -1 if dot < 0 else +1 (zero and NaN are
    outside); sdist = sgn * sqrt(d2); grad = (sgn * s) / sqrt(d2) per component if d2 > 0, else N / sqrt((Nx*Nx + Ny*Ny) + Nz*Nz), or 0
    where that is not finite.  A miss: found = 0, sdist = +r, face = -1, uv = 0, feature = 0, grad = 0.
    -> (found uint8, sdist, face int32, uv, feature uint8, grad [n,3]).  face_normal_only (for the tests): N = pn[face, 0] whatever the
    feature, the sign a single face's normal would give."""
    found, dist, face, uv = unsigned
    pts = np.asarray(pts, f32).reshape(-1, 3).astype(dtype)
    tri, pn = np.asarray(tri, dtype), np.asarray(pn, dtype)
    n = len(pts)
    got = found == 1
    rec = tri[np.maximum(face, 0)]
    u, v = uv[:, 0].astype(dtype), uv[:, 1].astype(dtype)
    with np.errstate(all='ignore'):
        feat = np.where(got, feature_on_tri_np(pts, rec, dtype), 0).astype(np.uint8)
        q = [rec[:, k] + (rec[:, 4 + k] * u + rec[:, 8 + k] * v) for k in range(3)]
        sx, sy, sz = pts[:, 0] - q[0], pts[:, 1] - q[1], pts[:, 2] - q[2]
        dd = (sx * sx + sy * sy) + sz * sz
        N = pn[np.maximum(face, 0), 0 if face_normal_only else feat]
        dot = (sx * N[:, 0] + sy * N[:, 1]) + sz * N[:, 2]
        sgn = np.where(dot < 0, dtype(-1), dtype(1))
        d = np.sqrt(dd)
        sdist = np.where(got, sgn * d, dtype(f32(r))).astype(dtype)
        nl = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
        flat = N / nl[:, None]
        flat = np.where(np.isfinite(flat), flat, 0)
        grad = np.where((dd > 0)[:, None], (sgn[:, None] * np.stack([sx, sy, sz], 1)) / d[:, None], flat)
        grad = np.where(got[:, None], grad, 0).astype(dtype)
    return found, sdist, face, uv, feat, grad


def signed_grid_np(pts, r, lists, tri, pn, G, lo, inv):
    """What ctx_mesh_signed_distance computes: closest_grid_np, then sign_step_np."""
    return sign_step_np(pts, r, R.closest_grid_np(pts, r, lists, tri, G, lo, inv), tri, pn)


def signed_all_np(pts, r, tri, pn, dtype=f32):
    """The same over all triangles: closest_all_np, then sign_step_np; dtype=float64 with float64 records and tables is the reference."""
    return sign_step_np(pts, r, R.closest_all_np(pts, r, tri, dtype), tri, pn, dtype)


# ---- the ramp ------------------------------------------------------------------------------------------------------------------------------
def ramp_defaults(h):
    """-> (width, peak) float32 of MeshSolidField with width=None, peak=None: the largest cell edge and 32 / width."""
    width = f32(np.max(np.asarray(h, f32)))
    return width, f32(32) / width


def ramp_np(sdist, width, peak):
    """density = peak * min(1, max(0, -d)) with d = sdist / width, binary32, every operation rounding on its own."""
    sdist, width, peak = np.asarray(sdist, f32), f32(width), f32(peak)
    d = sdist / width
    return (peak * np.minimum(f32(1), np.maximum(f32(0), -d))).astype(f32)


def ramp_gradient_np(sdist, grad, width, peak):
    """d density / d p = (-(peak / width)) * grad where -width < sdist < 0, and 0 elsewhere; peak / width rounded once."""
    sdist, grad = np.asarray(sdist, f32), np.asarray(grad, f32)
    k = -(f32(peak) / f32(width))
    on = (sdist > -f32(width)) & (sdist < 0)
    return np.where(on[:, None], k * grad, f32(0)).astype(f32)


# ---- the independent truth for the sign ----------------------------------------------------------------------------------------------------
def winding_number_np(pts, vertices, faces, chunk=512):
    """Generalised winding number in float64 (Van Oosterom & Strackee's solid angle per triangle, summed, over 4 pi): 1 inside a closed
    mesh wound outward, 0 outside."""
    p = np.asarray(pts, np.float64).reshape(-1, 3)
    t = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    out = np.zeros(len(p))
    for i0 in range(0, len(p), chunk):
        a, b, c = (t[None, :, k] - p[i0:i0 + chunk, None] for k in range(3))
        la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (a, b, c))
        det = np.einsum('nfk,nfk->nf', a, np.cross(b, c))
        den = la * lb * lc + np.einsum('nfk,nfk->nf', a, b) * lc + np.einsum('nfk,nfk->nf', b, c) * la + np.einsum('nfk,nfk->nf', c, a) * lb
        out[i0:i0 + chunk] = (2 * np.arctan2(det, den)).sum(1) / (4 * np.pi)
    return out
