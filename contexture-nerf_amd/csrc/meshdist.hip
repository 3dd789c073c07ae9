// How far a point is from the mesh, on which side of it, and where on it the nearest point lies: one kernel body, in an unsigned and a
// signed instantiation, over the per-cell triangle lists and the triangle records of meshhit.hip.  Built with -ffp-contract=off: every product, sum and quotient below rounds on its own, in the order written,
// and sqrtf and / are the correctly rounded ones, so the numpy restatement (tests/meshdist_rule.py, tests/meshsdf_rule.py for the signed form) gives the same bits; it is the
// definition, this file follows it line by line.
// One lane per point; a lane looks at every cell of its block [a, b]^3 and at every triangle listed there.  No cell is left out: a list
// says that a triangle touches the cell, not that its nearest point lies there (that point may be in a cell outside the grid), so the
// distance from the point to a cell bounds nothing that is listed in it.  The minimum over (d2, face) does not depend on the order of
// the visits, and a triangle listed in several cells gives the same numbers each time.
#include "occ_walk.h"

#define MD_BLK 256
#define MD_CAP 2048                      // blocks of a grid-stride launch: 8 per CU

// One point against one triangle record: Ericson's closest point, region by region.  The one body of both kernels; the unsigned kernel
// ignores feat and s, and the compiler drops them there.  feat: 0 the interior, 1 / 2 / 3 the vertices v0, v0 + e1, v0 + e2, 4 / 5 / 6 the
// edges along e1, along e2 and opposite v0: the row of the pseudonormal table (meshpn.hip) that belongs to the region.
struct MdTest { float u, v, dd, sx, sy, sz; int feat; };

__device__ __forceinline__ MdTest md_test(float px, float py, float pz, float4 v0, float4 e1, float4 e2)
{
    MdTest t;
    const float apx = px - v0.x, apy = py - v0.y, apz = pz - v0.z;
    const float d1 = (e1.x * apx + e1.y * apy) + e1.z * apz, d2 = (e2.x * apx + e2.y * apy) + e2.z * apz;
    const float bpx = apx - e1.x, bpy = apy - e1.y, bpz = apz - e1.z;
    const float d3 = (e1.x * bpx + e1.y * bpy) + e1.z * bpz, d4 = (e2.x * bpx + e2.y * bpy) + e2.z * bpz;
    const float cpx = apx - e2.x, cpy = apy - e2.y, cpz = apz - e2.z;
    const float d5 = (e1.x * cpx + e1.y * cpy) + e1.z * cpz, d6 = (e2.x * cpx + e2.y * cpy) + e2.z * cpz;
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    float u, v;
    if (d1 <= 0.f && d2 <= 0.f) { u = 0.f; v = 0.f; t.feat = 1; }                                   // the vertex v0
    else if (d3 >= 0.f && d4 <= d3) { u = 1.f; v = 0.f; t.feat = 2; }                               // the vertex v0 + e1
    else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) { u = d1 / (d1 - d3); v = 0.f; t.feat = 4; }      // the edge along e1
    else if (d6 >= 0.f && d5 <= d6) { u = 0.f; v = 1.f; t.feat = 3; }                               // the vertex v0 + e2
    else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) { u = 0.f; v = d2 / (d2 - d6); t.feat = 5; }      // the edge along e2
    else if (va <= 0.f && d4 - d3 >= 0.f && d5 - d6 >= 0.f) {                                       // the edge opposite v0
        const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        u = 1.0f - w; v = w; t.feat = 6;
    } else {                                                                                        // the interior
        const float den = 1.0f / ((va + vb) + vc);
        u = vb * den; v = vc * den; t.feat = 0;
    }
    const float qx = v0.x + (e1.x * u + e2.x * v), qy = v0.y + (e1.y * u + e2.y * v), qz = v0.z + (e1.z * u + e2.z * v);
    t.sx = px - qx; t.sy = py - qy; t.sz = pz - qz;
    t.dd = (t.sx * t.sx + t.sy * t.sy) + t.sz * t.sz;                 // a NaN anywhere in the record ends up here
    t.u = u; t.v = v;
    return t;
}

// SIGNED = false: ctx_mesh_closest_point.  SIGNED = true: ctx_mesh_signed_distance; the walk and the minimum are the same code, and after
// them the winning face is evaluated once more (the same bits as inside the loop, so its feature and s = p - q are those of the winning
// evaluation, and the loop carries nothing for them), one row of the pseudonormal table is fetched, and the sign, the feature and the
// gradient are stored beside the rest.
template <bool SIGNED>
__global__ __launch_bounds__(MD_BLK) void k_mesh_closest_point(const float *__restrict__ pts, int64_t n, float r, int G, ocm3 lo, ocm3 inv,
                                                               const int32_t *__restrict__ cell_off, const int32_t *__restrict__ cell_tri, int64_t n_list,
                                                               const float4 *__restrict__ tri, int F, const float *__restrict__ pn,
                                                               uint8_t *__restrict__ found, float *__restrict__ dist, int32_t *__restrict__ face,
                                                               float2 *__restrict__ uv, uint8_t *__restrict__ feature, float *__restrict__ grad)
{
    const float gmax = (float)(G - 1), rr = r * r;
    for (int64_t i = (int64_t)blockIdx.x * MD_BLK + threadIdx.x; i < n; i += (int64_t)gridDim.x * MD_BLK) {
        const float px = pts[i * 3 + 0], py = pts[i * 3 + 1], pz = pts[i * 3 + 2];
        const float ax = floorf(((px - r) - lo.x) * inv.x), ay = floorf(((py - r) - lo.y) * inv.y), az = floorf(((pz - r) - lo.z) * inv.z);
        const float bx = floorf(((px + r) - lo.x) * inv.x), by = floorf(((py + r) - lo.y) * inv.y), bz = floorf(((pz + r) - lo.z) * inv.z);
        bool live = ocm_finite(px) && ocm_finite(py) && ocm_finite(pz);
        live = live && !(bx < 0.f || by < 0.f || bz < 0.f || ax > gmax || ay > gmax || az > gmax);
        // fmaxf / fminf return the operand that is not a NaN: the six indices lie in [0, G - 1] whatever lo and inv hold
        const int x0 = (int)fminf(fmaxf(ax, 0.f), gmax), y0 = (int)fminf(fmaxf(ay, 0.f), gmax), z0 = (int)fminf(fmaxf(az, 0.f), gmax);
        const int x1 = (int)fminf(fmaxf(bx, 0.f), gmax), y1 = (int)fminf(fmaxf(by, 0.f), gmax), z1 = (int)fminf(fmaxf(bz, 0.f), gmax);
        float bd = INFINITY, bu = 0.f, bv = 0.f;
        int bf = -1;
        if (live) {
            for (int cz = z0; cz <= z1; ++cz)
                for (int cy = y0; cy <= y1; ++cy)
                    for (int cx = x0; cx <= x1; ++cx) {
                        const int cell = (cz * G + cy) * G + cx;
                        const int k0 = cell_off[cell], k1 = cell_off[cell + 1];
                        for (int k = k0 < 0 ? 0 : k0; k < k1 && k < n_list; ++k) {
                            const int f = cell_tri[k];
                            if (f < 0 || f >= F) continue;
                            const MdTest t = md_test(px, py, pz, tri[(int64_t)f * 3 + 0], tri[(int64_t)f * 3 + 1], tri[(int64_t)f * 3 + 2]);
                            if (!(ocm_finite(t.dd) && ocm_finite(t.u) && ocm_finite(t.v))) continue;
                            if (t.dd < bd || (t.dd == bd && f < bf)) { bd = t.dd; bu = t.u; bv = t.v; bf = f; }
                        }
                    }
        }
        const bool got = bf >= 0 && bd <= rr;
        found[i] = got ? 1 : 0;
        face[i] = got ? bf : -1;
        uv[i] = got ? make_float2(bu, bv) : make_float2(0.f, 0.f);
        if constexpr (!SIGNED) {
            dist[i] = got ? sqrtf(bd) : r;
        } else {
            float sd = r, gx = 0.f, gy = 0.f, gz = 0.f;
            int feat = 0;
            if (got) {                                                // 0 <= bf < F, 0 <= feat <= 6: the row lies inside pn [F,7,3]
                const MdTest t = md_test(px, py, pz, tri[(int64_t)bf * 3 + 0], tri[(int64_t)bf * 3 + 1], tri[(int64_t)bf * 3 + 2]);
                feat = t.feat;
                const float *N = pn + ((int64_t)bf * 7 + feat) * 3;
                const float Nx = N[0], Ny = N[1], Nz = N[2];
                const float dot = (t.sx * Nx + t.sy * Ny) + t.sz * Nz;
                const float sgn = dot < 0.f ? -1.0f : 1.0f;           // zero and NaN count as outside
                const float d = sqrtf(bd);
                sd = sgn * d;
                if (bd > 0.f) {
                    gx = (sgn * t.sx) / d; gy = (sgn * t.sy) / d; gz = (sgn * t.sz) / d;
                } else {                                              // on the surface: the pseudonormal's direction
                    const float nl = sqrtf((Nx * Nx + Ny * Ny) + Nz * Nz);
                    gx = Nx / nl; gy = Ny / nl; gz = Nz / nl;
                    gx = ocm_finite(gx) ? gx : 0.f; gy = ocm_finite(gy) ? gy : 0.f; gz = ocm_finite(gz) ? gz : 0.f;
                }
            }
            dist[i] = sd;
            feature[i] = (uint8_t)feat;
            grad[i * 3 + 0] = gx; grad[i * 3 + 1] = gy; grad[i * 3 + 2] = gz;
        }
    }
}

// the envelope both entry points share
static int32_t mesh_closest_args(const char *who, int64_t n, float r, int32_t G, float inv_x, float inv_y, float inv_z, int64_t n_list, int64_t F)
{
    CTX_REQUIRE(n >= 0 && n <= INT32_MAX, "%s: n=%lld outside [0, 2^31)", who, (long long)n);
    CTX_REQUIRE(n_list >= 0 && n_list <= INT32_MAX, "%s: n_list=%lld outside [0, 2^31)", who, (long long)n_list);
    CTX_REQUIRE(G >= 1 && G <= 256, "%s: G=%d outside [1, 256]", who, (int)G);
    CTX_REQUIRE(F >= 1 && F <= INT32_MAX, "%s: F=%lld outside [1, 2^31)", who, (long long)F);
    CTX_REQUIRE(fabsf(r) < INFINITY && r > 0.f, "%s: r=%g: want a finite radius > 0", who, (double)r);
    const float inv_max = fmaxf(fmaxf(inv_x, inv_y), inv_z), inv_min = fminf(fminf(inv_x, inv_y), inv_z);
    CTX_REQUIRE(inv_min > 0.f && fabsf(inv_max) < INFINITY, "%s: inv=(%g, %g, %g): want finite cells per unit length > 0", who, (double)inv_x,
                (double)inv_y, (double)inv_z);
    // h and inv are each rounded once from the box: 3 * min(h) itself must pass, hence the 2^-20
    CTX_REQUIRE((double)r * (double)inv_max <= 3.0 * (1.0 + 9.5367431640625e-07),
                "%s: r=%g is larger than 3 cells (3 min(h) = %g): the block would exceed 7^3 cells", who, (double)r, 3.0 / (double)inv_max);
    return CTX_OK;
}

extern "C" int32_t ctx_mesh_closest_point(const float *pts, int64_t n, float r, int32_t G, float lo_x, float lo_y, float lo_z, float inv_x, float inv_y,
                                          float inv_z, const int32_t *cell_off, const int32_t *cell_tri, int64_t n_list, const float *tri, int64_t F,
                                          uint8_t *found, float *dist, int32_t *face, float *uv, ctx_stream_t stream)
{
    if (int32_t rc = mesh_closest_args("mesh_closest_point", n, r, G, inv_x, inv_y, inv_z, n_list, F)) return rc;
    if (n == 0) return CTX_OK;
    CTX_REQUIRE(pts && cell_off && tri && found && dist && face && uv && (cell_tri || n_list == 0), "mesh_closest_point: null pointer");
    CTX_REQUIRE(((uintptr_t)tri % 16) == 0 && ((uintptr_t)uv % 8) == 0, "mesh_closest_point: tri must be 16-byte and uv 8-byte aligned");
    const ocm3 lo = {lo_x, lo_y, lo_z}, inv = {inv_x, inv_y, inv_z};
    hipLaunchKernelGGL(k_mesh_closest_point<false>, dim3(capped_blocks(n, MD_BLK, MD_CAP)), dim3(MD_BLK), 0, (hipStream_t)stream, pts, n, r, (int)G, lo,
                       inv, cell_off, cell_tri, n_list, (const float4 *)tri, (int)F, (const float *)nullptr, found, dist, face, (float2 *)uv,
                       (uint8_t *)nullptr, (float *)nullptr);
    CTX_CHECK_LAUNCH("mesh_closest_point");
    return CTX_OK;
}

extern "C" int32_t ctx_mesh_signed_distance(const float *pts, int64_t n, float r, int32_t G, float lo_x, float lo_y, float lo_z, float inv_x, float inv_y,
                                            float inv_z, const int32_t *cell_off, const int32_t *cell_tri, int64_t n_list, const float *tri, int64_t F,
                                            const float *pn, int64_t pn_faces, uint8_t *found, float *sdist, int32_t *face, float *uv, uint8_t *feature,
                                            float *grad, ctx_stream_t stream)
{
    if (int32_t rc = mesh_closest_args("mesh_signed_distance", n, r, G, inv_x, inv_y, inv_z, n_list, F)) return rc;
    CTX_REQUIRE(pn_faces >= F, "mesh_signed_distance: pn holds %lld faces, the records %lld: the table is short", (long long)pn_faces, (long long)F);
    if (n == 0) return CTX_OK;
    CTX_REQUIRE(pts && cell_off && tri && pn && found && sdist && face && uv && feature && grad && (cell_tri || n_list == 0),
                "mesh_signed_distance: null pointer");
    CTX_REQUIRE(((uintptr_t)tri % 16) == 0 && ((uintptr_t)uv % 8) == 0, "mesh_signed_distance: tri must be 16-byte and uv 8-byte aligned");
    const ocm3 lo = {lo_x, lo_y, lo_z}, inv = {inv_x, inv_y, inv_z};
    hipLaunchKernelGGL(k_mesh_closest_point<true>, dim3(capped_blocks(n, MD_BLK, MD_CAP)), dim3(MD_BLK), 0, (hipStream_t)stream, pts, n, r, (int)G, lo,
                       inv, cell_off, cell_tri, n_list, (const float4 *)tri, (int)F, pn, found, sdist, face, (float2 *)uv, feature, grad);
    CTX_CHECK_LAUNCH("mesh_signed_distance");
    return CTX_OK;
}
