// The cell walk of a ray through the occupancy grid, shared by the span kernel (occupancy_mesh.hip) and the march kernels (march.hip).
// Both files are built with -ffp-contract=off: every product, sum and quotient rounds on its own, in the order written.
#pragma once
#include "common.h"
#include <math.h>
#include <type_traits>

struct ocm3 { float x, y, z; };

__device__ __forceinline__ bool ocm_finite(float x) { return fabsf(x) < INFINITY; }          // false for NaN

// Finite check, slab clip to [t_a, t_b], start cell, then the walk: at every cell the exit parameters come afresh from the integer cell
// index (no running sum, no drift); te = the smallest, ties x, y, z; t_out = min(max(te, t_in), t_b) is the next cell's t_in.  Ends when
// te >= t_b, when the step leaves the grid, or after 3G + 3 cells.  visit(occupied, t_in, t_out) is called once per cell, in walk order;
// a ray that is non-finite or misses the box visits nothing.
// A visitor may also take the cell: visit(occupied, t_in, t_out, cell) with cell = (cz*G + cy)*G + cx, and such a visitor may return bool:
// true ends the walk after this cell (meshhit.hip stops at the cell that holds its nearest hit).  The three-argument visitors of the span
// and march kernels take the first branch below at compile time: their code is what it was.
template <class Visit>
__device__ __forceinline__ bool occ_walk_visit(Visit &visit, bool occ, float tin, float tout, int cell)
{
    if constexpr (std::is_invocable_v<Visit &, bool, float, float>) {
        visit(occ, tin, tout);
        return false;
    } else if constexpr (std::is_same_v<std::invoke_result_t<Visit &, bool, float, float, int>, bool>) {
        return visit(occ, tin, tout, cell);
    } else {
        visit(occ, tin, tout, cell);
        return false;
    }
}

template <class Visit>
__device__ __forceinline__ void occ_walk(float ox, float oy, float oz, float dx, float dy, float dz, float near, float far,
                                         const uint8_t *__restrict__ cells, int G, ocm3 lo, ocm3 hi, ocm3 inv, ocm3 h, Visit &&visit)
{
    const float Gm1 = (float)(G - 1);
    const int max_cells = 3 * G + 3;
    bool ok = ocm_finite(ox) && ocm_finite(oy) && ocm_finite(oz) && ocm_finite(dx) && ocm_finite(dy) && ocm_finite(dz);
    float ta = near, tb = far;
    if (ok) {                                                     // slab clip; a zero component compares the origin with its slab
        if (dx == 0.f) ok = ok && ox >= lo.x && ox <= hi.x;
        else { const float t1 = (lo.x - ox) / dx, t2 = (hi.x - ox) / dx; ta = fmaxf(ta, fminf(t1, t2)); tb = fminf(tb, fmaxf(t1, t2)); }
        if (dy == 0.f) ok = ok && oy >= lo.y && oy <= hi.y;
        else { const float t1 = (lo.y - oy) / dy, t2 = (hi.y - oy) / dy; ta = fmaxf(ta, fminf(t1, t2)); tb = fminf(tb, fmaxf(t1, t2)); }
        if (dz == 0.f) ok = ok && oz >= lo.z && oz <= hi.z;
        else { const float t1 = (lo.z - oz) / dz, t2 = (hi.z - oz) / dz; ta = fmaxf(ta, fminf(t1, t2)); tb = fminf(tb, fmaxf(t1, t2)); }
        ok = ok && ta <= tb;
    }
    if (!ok) return;
    int cx = (int)fminf(fmaxf(((ox + dx * ta) - lo.x) * inv.x, 0.f), Gm1);
    int cy = (int)fminf(fmaxf(((oy + dy * ta) - lo.y) * inv.y, 0.f), Gm1);
    int cz = (int)fminf(fmaxf(((oz + dz * ta) - lo.z) * inv.z, 0.f), Gm1);
    float tin = ta;
    for (int step = 0; step < max_cells; ++step) {
        const float ex = dx == 0.f ? INFINITY : ((lo.x + (float)(cx + (dx > 0.f ? 1 : 0)) * h.x) - ox) / dx;
        const float ey = dy == 0.f ? INFINITY : ((lo.y + (float)(cy + (dy > 0.f ? 1 : 0)) * h.y) - oy) / dy;
        const float ez = dz == 0.f ? INFINITY : ((lo.z + (float)(cz + (dz > 0.f ? 1 : 0)) * h.z) - oz) / dz;
        int ax = 0;
        float te = ex;
        if (ey < te) { ax = 1; te = ey; }
        if (ez < te) { ax = 2; te = ez; }
        const float tout = fminf(fmaxf(te, tin), tb);
        const int cell = (cz * G + cy) * G + cx;                           // 0 <= c < G: clamped at the start, checked at every step; < 2^24
        if (occ_walk_visit(visit, cells[cell] != 0, tin, tout, cell)) break;
        if (te >= tb) break;
        if (ax == 0) { cx += dx > 0.f ? 1 : -1; if (cx < 0 || cx > G - 1) break; }
        else if (ax == 1) { cy += dy > 0.f ? 1 : -1; if (cy < 0 || cy > G - 1) break; }
        else { cz += dz > 0.f ? 1 : -1; if (cz < 0 || cz > G - 1) break; }
        tin = tout;
    }
}
