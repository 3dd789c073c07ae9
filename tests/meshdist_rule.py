"""The definition of the point / mesh query: numpy restatements in binary32 of the closest point on a triangle and of
`ctx_mesh_closest_point`, in two forms: the minimum over the triangles listed in the block of cells around the point (what the kernel
computes; csrc/meshdist.hip is held to it with array_equal), and the same arithmetic over all triangles, which says what the first must
find; the latter also in float64.  The tent of MeshDensityField / AtlasField is restated here too.  Not a test module:
tests/test_meshdist_cpu.py and tests/test_meshdist_gpu.py import it.

The lists and the triangle records are those of tests/meshhit_rule.py.  All float arithmetic is binary32 in the order written (numpy rounds
every product, sum and quotient on its own).

Where the two forms differ.  The voxeliser's cells are inflated by 2^-7 of a cell, so the cell that holds a triangle's closest point lists
that triangle: where the closest point of the all-triangles answer lies inside the box, the grid form finds the same triangle with the
same numbers, unless the distance is within rounding of r.  A closest point OUTSIDE the box lies in no cell: a triangle that reaches out of
the box is found with that distance only if one of the block's cells happens to list it.  The query answers for the mesh inside the box;
`closest_in_box` says which points a comparison of the two forms may judge."""
import numpy as np

from meshhit_rule import (mesh_cells_np, tri_records_np, grid_consts, icosphere, spot_mesh, random_triangles, triangles_to_mesh,  # noqa: F401
                          KINDS)

f32 = np.float32


# ---- point against triangle --------------------------------------------------------------------------------------------------------------
def closest_on_tri_np(p, rec, dtype=f32):
    """-> (ok bool, d2, u, v) of points p [..., 3] against records rec [..., 12] (broadcast): Ericson's closest point on a triangle, region
    by region, the first region whose condition holds.  Dots are (ax*bx + ay*by) + az*bz.
      ap = p - v0, d1 = e1.ap, d2 = e2.ap;                    d1 <= 0 and d2 <= 0                     -> (u, v) = (0, 0)
      bp = ap - e1, d3 = e1.bp, d4 = e2.bp;                   d3 >= 0 and d4 <= d3                    -> (1, 0)
      vc = d1*d4 - d3*d2;                                     vc <= 0 and d1 >= 0 and d3 <= 0         -> (d1/(d1 - d3), 0)
      cp = ap - e2, d5 = e1.cp, d6 = e2.cp;                   d6 >= 0 and d5 <= d6                    -> (0, 1)
      vb = d5*d2 - d1*d6;                                     vb <= 0 and d2 >= 0 and d6 <= 0         -> (0, d2/(d2 - d6))
      va = d3*d6 - d5*d4;                                     va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0
                                                              -> w = (d4 - d3)/((d4 - d3) + (d5 - d6)), (1 - w, w)
      otherwise den = 1/((va + vb) + vc)                                                              -> (vb*den, vc*den)
    then q = v0 + (e1*u + e2*v) per component, s = p - q, d2 = (sx*sx + sy*sy) + sz*sz.  ok is False for a record with a NaN and for a
    non-finite d2, u or v (the triangle is skipped)."""
    p, rec = np.asarray(p, dtype), np.asarray(rec, dtype)
    px, py, pz = p[..., 0], p[..., 1], p[..., 2]
    v0x, v0y, v0z, e1x, e1y, e1z, e2x, e2y, e2z = (rec[..., k] for k in (0, 1, 2, 4, 5, 6, 8, 9, 10))
    zero, one = dtype(0), dtype(1)
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
        den = one / ((va + vb) + vc)
        u, v = vb * den, vc * den                                                                  # the interior; the regions, last to first
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        m = (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)
        u, v = np.where(m, one - w, u), np.where(m, w, v)
        m = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        u, v = np.where(m, zero, u), np.where(m, d2 / (d2 - d6), v)
        m = (d6 >= 0) & (d5 <= d6)
        u, v = np.where(m, zero, u), np.where(m, one, v)
        m = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        u, v = np.where(m, d1 / (d1 - d3), u), np.where(m, zero, v)
        m = (d3 >= 0) & (d4 <= d3)
        u, v = np.where(m, one, u), np.where(m, zero, v)
        m = (d1 <= 0) & (d2 <= 0)
        u, v = np.where(m, zero, u), np.where(m, zero, v)
        qx, qy, qz = v0x + (e1x * u + e2x * v), v0y + (e1y * u + e2y * v), v0z + (e1z * u + e2z * v)
        sx, sy, sz = px - qx, py - qy, pz - qz
        dd = (sx * sx + sy * sy) + sz * sz
        ok = ~np.any(np.isnan(rec[..., [0, 1, 2, 4, 5, 6, 8, 9, 10]]), -1) & np.isfinite(dd) & np.isfinite(u) & np.isfinite(v)
    u, v, dd = (np.broadcast_to(x, ok.shape) for x in (u, v, dd))
    return ok, dd, u, v


def _miss(n, r, dtype=f32):
    return np.zeros(n, np.uint8), np.full(n, dtype(r), dtype), np.full(n, -1, np.int32), np.zeros((n, 2), dtype)


# ---- the same arithmetic over all triangles ----------------------------------------------------------------------------------------------
def closest_all_np(pts, r, tri, dtype=f32, chunk=256, return_d2=False):
    """-> (found uint8 [n], dist [n], face int32 [n], uv [n,2]): every point against every triangle; the minimum over (d2, face) in
    lexicographic order, accepted only if d2 <= r*r; dist = sqrt(d2).  A miss (also a non-finite point): found = 0, dist = r, face = -1,
    uv = 0.  dtype=float64 is the reference (records from tri_records_np(dtype=float64), r and the points as given in binary32).
    return_d2=True adds the best d2 [n] of every point, accepted or not (inf where no triangle counts)."""
    pts = np.asarray(pts, f32).reshape(-1, 3)
    tri = np.asarray(tri, dtype)
    n = len(pts)
    found, dist, face, uv = _miss(n, f32(r), dtype)
    best_d2 = np.full(n, np.inf, dtype)
    r = dtype(f32(r))
    rr = r * r
    with np.errstate(all='ignore'):
        for i0 in range(0, n, chunk):
            sl = slice(i0, min(n, i0 + chunk))
            ok, dd, u, v = closest_on_tri_np(pts[sl, None, :], tri[None], dtype)
            ok = ok & np.all(np.isfinite(pts[sl]), -1)[:, None]
            key = np.where(ok, dd, dtype(np.inf))
            best = np.argmin(key, 1)                                  # the first minimum: the lower face id on equal d2
            rows = np.arange(key.shape[0])
            best_d2[sl] = key[rows, best]
            got = ok[rows, best] & (dd[rows, best] <= rr)
            found[sl] = got
            dist[sl] = np.where(got, np.sqrt(dd[rows, best]), r)
            face[sl] = np.where(got, best, -1)
            uv[sl, 0], uv[sl, 1] = np.where(got, u[rows, best], 0), np.where(got, v[rows, best], 0)
    return (found, dist, face, uv, best_d2) if return_d2 else (found, dist, face, uv)


def closest_in_box(pts, face, uv, tri64, lo, hi):
    """bool [n]: the closest point v0 + e1*u + e2*v on `face` (float64 records) lies inside the box lo .. hi; False where face < 0."""
    tri64 = np.asarray(tri64, np.float64)
    rec = tri64[np.maximum(np.asarray(face, np.int64), 0)]
    uv = np.asarray(uv, np.float64)
    q = rec[:, 0:3] + rec[:, 4:7] * uv[:, :1] + rec[:, 8:11] * uv[:, 1:]
    with np.errstate(all='ignore'):
        return (np.asarray(face) >= 0) & np.all((q >= np.asarray(lo, np.float64)) & (q <= np.asarray(hi, np.float64)), -1)


# ---- the grid form: what ctx_mesh_closest_point computes ---------------------------------------------------------------------------------
def block_np(pts, r, G, lo, inv):
    """-> (live bool [n], a int64 [n,3], b int64 [n,3]): per axis a = floor(((p - r) - lo)*inv), b = floor(((p + r) - lo)*inv); a miss (not
    live) if p is not finite, or if on any axis b < 0 or a > G - 1; otherwise both clamped to [0, G - 1]."""
    pts = np.asarray(pts, f32).reshape(-1, 3)
    lo, inv, r = np.asarray(lo, f32), np.asarray(inv, f32), f32(r)
    with np.errstate(all='ignore'):
        a = np.floor(((pts - r) - lo) * inv)
        b = np.floor(((pts + r) - lo) * inv)
        live = np.all(np.isfinite(pts), -1) & ~np.any((b < 0) | (a > f32(G - 1)), -1)
        a = np.where(live[:, None], np.minimum(np.maximum(a, f32(0)), f32(G - 1)), 0).astype(np.int64)
        b = np.where(live[:, None], np.minimum(np.maximum(b, f32(0)), f32(G - 1)), 0).astype(np.int64)
    return live, a, b


def closest_grid_np(pts, r, lists, tri, G, lo, inv, stats=None):
    """-> (found uint8 [n], dist float32 [n], face int32 [n], uv float32 [n,2]).  lists = (count, cell_off, cell_tri) of mesh_cells_np, tri
    the records.  The block of block_np; the answer is the minimum, over every triangle listed in any cell of the block [a, b]^3, of
    (d2, face) in lexicographic order (closest_on_tri_np; a face id outside [0, F) is skipped), accepted only if d2 <= r*r;
    dist = sqrtf(d2).  A miss: found = 0, dist = r, face = -1, uv = 0.  No cell of the block is left out."""
    _, cell_off, cell_tri = (np.asarray(x, np.int64) for x in lists)
    pts = np.asarray(pts, f32).reshape(-1, 3)
    tri = np.asarray(tri, f32)
    n, F = len(pts), len(tri)
    r = f32(r)
    live, a, b = block_np(pts, r, G, lo, inv)
    bd, bf = np.full(n, f32(np.inf), f32), np.full(n, -1, np.int64)
    bu, bv = np.zeros(n, f32), np.zeros(n, f32)
    span = (b - a + 1) * live[:, None]
    n_tests = 0
    for dz in range(int(span[:, 2].max(initial=0))):
        for dy in range(int(span[:, 1].max(initial=0))):
            for dx in range(int(span[:, 0].max(initial=0))):
                idx = np.flatnonzero(live & (dx < span[:, 0]) & (dy < span[:, 1]) & (dz < span[:, 2]))
                if not idx.size:
                    continue
                cell = ((a[idx, 2] + dz) * G + (a[idx, 1] + dy)) * G + (a[idx, 0] + dx)
                k0 = cell_off[cell]
                ln = cell_off[cell + 1] - k0
                if not ln.sum():
                    continue
                pp = np.repeat(idx, ln)
                kk = np.repeat(k0 - (np.cumsum(ln) - ln), ln) + np.arange(int(ln.sum()))
                ff = cell_tri[kk]
                keep = (ff >= 0) & (ff < F)
                pp, ff = pp[keep], ff[keep]
                n_tests += len(ff)
                ok, dd, u, v = closest_on_tri_np(pts[pp], tri[ff])
                pp, ff, dd, u, v = pp[ok], ff[ok], dd[ok], u[ok], v[ok]
                if not len(pp):
                    continue
                order = np.lexsort((ff, dd, pp))                       # per point: the lowest d2 first, then the lower face id
                pp, ff, dd, u, v = pp[order], ff[order], dd[order], u[order], v[order]
                first = np.concatenate([[True], pp[1:] != pp[:-1]])
                pp, ff, dd, u, v = pp[first], ff[first], dd[first], u[first], v[first]
                better = (dd < bd[pp]) | ((dd == bd[pp]) & (ff < bf[pp]))      # bd starts at inf and an accepted d2 is finite
                pp, ff, dd, u, v = pp[better], ff[better], dd[better], u[better], v[better]
                bd[pp], bf[pp], bu[pp], bv[pp] = dd, ff, u, v
    if stats is not None:
        stats['tests'] = n_tests
    with np.errstate(all='ignore'):
        got = (bf >= 0) & (bd <= r * r)
        dist = np.where(got, np.sqrt(bd), r).astype(f32)
    return got.astype(np.uint8), dist, np.where(got, bf, -1).astype(np.int32), np.stack([np.where(got, bu, 0), np.where(got, bv, 0)], -1).astype(f32)


# ---- the tent ----------------------------------------------------------------------------------------------------------------------------------
def tent_defaults(h):
    """-> (width, peak) float32 of MeshDensityField / AtlasField with width=None, peak=None: the largest cell edge and 16 / width."""
    width = f32(np.max(np.asarray(h, f32)))
    return width, f32(16) / width


def tent_np(dist, width, peak):
    """density = peak * max(0, 1 - d) with d = dist / width, binary32, every operation rounding on its own."""
    dist, width, peak = np.asarray(dist, f32), f32(width), f32(peak)
    d = dist / width
    return (peak * np.maximum(f32(0), f32(1) - d)).astype(f32)
