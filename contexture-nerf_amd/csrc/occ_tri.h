// The conservative triangle-to-cell test of the mesh voxeliser, stated once: the per-triangle set-up (occ_tri_setup) and the per-cell test
// (occ_tri_cell), shared by the voxeliser (occupancy_mesh.hip: a byte per cell) and the cell triangle lists (meshhit.hip: a count and a
// list per cell).  (cell, face) is listed if and only if the voxeliser would store a 1 in that cell for that face alone: one predicate.
// Both files are built with -ffp-contract=off: every product, sum and quotient rounds on its own, in the order written, so the numpy
// restatement (tests/test_occupancy_mesh_cpu.py: occ_voxelize_np) gives the same bits; it is the definition.
#pragma once
#include "occ_walk.h"

#define OCM_E 0.0078125f      // 2^-7 of a cell: the inflation of the cell's box on every side
#define OCM_DELTA 1.015625f   // 1 + 2e, the side of the inflated box

// What the set-up leaves for the cell loop: the candidate box (first cell c0 and count cn per axis, total = their product <= 256^3) and the
// plane pair and nine edge functions of Schwarz and Seidel's test on the inflated box.  All values are uniform over the wave that owns the
// triangle (gfx950 has no scalar float arithmetic: they sit in vector registers).
struct OccTri {
    int c0[3], cn[3], total;
    bool degenerate;
    float n[3], d1, d2;
    float neu[9], nev[9], de[9];                                      // [plane * 3 + edge]; planes xy, yz, zx
};

// false: the face marks nothing (an index outside [0, V), a non-finite grid coordinate, or a bounding box that misses the grid)
__device__ __forceinline__ bool occ_tri_setup(const float *__restrict__ vtx, const int64_t *__restrict__ faces, int64_t V, int64_t f, int G, ocm3 lo,
                                              ocm3 inv, OccTri &T)
{
    const float Gm1 = (float)(G - 1);
    const int64_t i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) return false;
    float g[3][3];                                                    // g[vertex][axis], grid coordinates: the expression of ctx_occ_mark
    const int64_t iv[3] = {i0, i1, i2};
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        g[k][0] = (vtx[iv[k] * 3 + 0] - lo.x) * inv.x;
        g[k][1] = (vtx[iv[k] * 3 + 1] - lo.y) * inv.y;
        g[k][2] = (vtx[iv[k] * 3 + 2] - lo.z) * inv.z;
        fin = fin && ocm_finite(g[k][0]) && ocm_finite(g[k][1]) && ocm_finite(g[k][2]);
    }
    if (!fin) return false;
    bool empty = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float mn = fminf(fminf(g[0][a], g[1][a]), g[2][a]), mx = fmaxf(fmaxf(g[0][a], g[1][a]), g[2][a]);
        const float fa = floorf(mn - OCM_E), fb = floorf(mx + OCM_E);
        empty = empty || fb < 0.f || fa > Gm1;
        T.c0[a] = (int)fmaxf(fa, 0.f);                                // in [0, G - 1] unless empty (then unused)
        T.cn[a] = (int)fminf(fb, Gm1) - T.c0[a] + 1;
    }
    if (empty) return false;
    T.total = T.cn[0] * T.cn[1] * T.cn[2];                            // <= 256^3

    float ea[3], eb[3], e1[3], e2[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        ea[a] = g[1][a] - g[0][a]; eb[a] = g[2][a] - g[0][a];
        e1[a] = g[2][a] - g[1][a]; e2[a] = g[0][a] - g[2][a];
    }
    float *n = T.n;
    n[0] = ea[1] * eb[2] - ea[2] * eb[1];
    n[1] = ea[2] * eb[0] - ea[0] * eb[2];
    n[2] = ea[0] * eb[1] - ea[1] * eb[0];
    T.degenerate = n[0] == 0.f && n[1] == 0.f && n[2] == 0.f;
    float crit[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) crit[a] = n[a] > 0.f ? OCM_DELTA : 0.f;
    T.d1 = (n[0] * (crit[0] - g[0][0]) + n[1] * (crit[1] - g[0][1])) + n[2] * (crit[2] - g[0][2]);
    T.d2 = (n[0] * ((OCM_DELTA - crit[0]) - g[0][0]) + n[1] * ((OCM_DELTA - crit[1]) - g[0][1])) + n[2] * ((OCM_DELTA - crit[2]) - g[0][2]);
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
        const int u = pl, v = (pl + 1) % 3, w = (pl + 2) % 3;
#pragma unroll
        for (int ed = 0; ed < 3; ++ed) {
            const float eu = ed == 0 ? ea[u] : ed == 1 ? e1[u] : e2[u];
            const float ev = ed == 0 ? ea[v] : ed == 1 ? e1[v] : e2[v];
            const float a_u = n[w] >= 0.f ? -ev : ev, a_v = n[w] >= 0.f ? eu : -eu;
            T.neu[pl * 3 + ed] = a_u; T.nev[pl * 3 + ed] = a_v;
            T.de[pl * 3 + ed] = (-(a_u * g[ed][u] + a_v * g[ed][v]) + fmaxf(0.f, OCM_DELTA * a_u)) + fmaxf(0.f, OCM_DELTA * a_v);
        }
    }
    return true;
}

// candidate i of the box, x fastest -> its cell
__device__ __forceinline__ void occ_tri_candidate(const OccTri &T, int i, int &cx, int &cy, int &cz)
{
    const int ix = i % T.cn[0], t = i / T.cn[0];
    cx = T.c0[0] + ix; cy = T.c0[1] + t % T.cn[1]; cz = T.c0[2] + t / T.cn[1];
}

// the test of cell (cx, cy, cz), a candidate of T: the plane pair and the nine edge functions on the box with minimum corner c - e
__device__ __forceinline__ bool occ_tri_cell(const OccTri &T, int cx, int cy, int cz)
{
    if (T.degenerate) return true;
    const float p[3] = {(float)cx - OCM_E, (float)cy - OCM_E, (float)cz - OCM_E};
    const float npd = (T.n[0] * p[0] + T.n[1] * p[1]) + T.n[2] * p[2];
    const float s1 = npd + T.d1, s2 = npd + T.d2;
    bool ok = (s1 <= 0.f && s2 >= 0.f) || (s1 >= 0.f && s2 <= 0.f);
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
        const int u = pl, v = (pl + 1) % 3;
#pragma unroll
        for (int ed = 0; ed < 3; ++ed)
            ok = ok && ((T.neu[pl * 3 + ed] * p[u] + T.nev[pl * 3 + ed] * p[v]) + T.de[pl * 3 + ed]) >= 0.f;
    }
    return ok;
}
