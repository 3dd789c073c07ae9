// The angle-weighted pseudonormal tables of the mesh (Baerentzen & Aanaes 2005): per face its unit normal, the pseudonormals of its three
// vertices and of its three edges, the rows the signed query of meshdist.hip reads by (face, feature).  A set-up pass, not a hot path.
// Built with -ffp-contract=off: every product, sum and quotient below rounds on its own, in the order written, so the numpy restatement
// (tests/meshsdf_rule.py) gives the same bits for rows 0 and 4 .. 6; rows 1 .. 3 go through atan2f and agree to its last bits.
// Two launches: row 0 of every face, then one lane per (face, row 1 .. 6), which reads the row 0 of the faces around it.  Every sum runs
// over a vertex's incidence list, ascending by face id (ctx_mesh_vertex_faces_fill): no atomics, one writer per element, one value.
#include "occ_walk.h"

#define MP_BLK 256
#define MP_CAP 2048

__global__ __launch_bounds__(MP_BLK) void k_mesh_pn_face(const float4 *__restrict__ tri, int64_t F, float *__restrict__ pn)
{
    for (int64_t f = (int64_t)blockIdx.x * MP_BLK + threadIdx.x; f < F; f += (int64_t)gridDim.x * MP_BLK) {
        const float4 v0 = tri[f * 3 + 0], e1 = tri[f * 3 + 1], e2 = tri[f * 3 + 2];
        const float nx = e1.y * e2.z - e1.z * e2.y, ny = e1.z * e2.x - e1.x * e2.z, nz = e1.x * e2.y - e1.y * e2.x;
        const float nn = (nx * nx + ny * ny) + nz * nz;
        const float ln = sqrtf(nn);
        const bool good = nn > 0.f && nn < INFINITY;
        const bool spoilt = v0.x != v0.x || v0.y != v0.y || v0.z != v0.z || e1.x != e1.x || e1.y != e1.y || e1.z != e1.z || e2.x != e2.x ||
                            e2.y != e2.y || e2.z != e2.z;
        float *row = pn + f * 21;
        row[0] = spoilt ? NAN : (good ? nx / ln : 0.f);
        row[1] = spoilt ? NAN : (good ? ny / ln : 0.f);
        row[2] = spoilt ? NAN : (good ? nz / ln : 0.f);
    }
}

// the interior angle between the edge vectors a and b
__device__ __forceinline__ float mp_angle(float ax, float ay, float az, float bx, float by, float bz)
{
    const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    return atan2f(sqrtf((cx * cx + cy * cy) + cz * cz), (ax * bx + ay * by) + az * bz);
}

__global__ __launch_bounds__(MP_BLK) void k_mesh_pn_rows(const int64_t *__restrict__ faces, int64_t V, int64_t F, const float4 *__restrict__ tri,
                                                         const int32_t *__restrict__ vf_off, const int32_t *__restrict__ vf_face, int64_t n_vf,
                                                         float *__restrict__ pn)
{
    for (int64_t i = (int64_t)blockIdx.x * MP_BLK + threadIdx.x; i < F * 6; i += (int64_t)gridDim.x * MP_BLK) {
        const int64_t f = i / 6;
        const int row = 1 + (int)(i - f * 6);
        float *out = pn + f * 21 + row * 3;
        const float own = pn[f * 21];                                 // row 0 is NaN exactly for a spoilt record (the first launch)
        if (own != own) { out[0] = out[1] = out[2] = NAN; continue; }
        // a finite record has its three ids in [0, V); they are bounded all the same
        const int c0 = row <= 3 ? row - 1 : (row == 6 ? 1 : 0), c1 = row <= 3 ? -1 : (row == 4 ? 1 : 2);
        const int64_t w0 = faces[f * 3 + c0], w1 = c1 >= 0 ? faces[f * 3 + c1] : -1;
        float ax = 0.f, ay = 0.f, az = 0.f;
        if (w0 >= 0 && w0 < V) {
            const int k0 = vf_off[w0], k1 = vf_off[w0 + 1];
            for (int k = k0 < 0 ? 0 : k0; k < k1 && k < n_vf; ++k) {
                const int g = vf_face[k];
                if (g < 0 || g >= F) continue;
                const float ux = pn[(int64_t)g * 21 + 0], uy = pn[(int64_t)g * 21 + 1], uz = pn[(int64_t)g * 21 + 2];
                if (!(ocm_finite(ux) && ocm_finite(uy) && ocm_finite(uz)) || (ux == 0.f && uy == 0.f && uz == 0.f)) continue;   // does not count
                const int64_t g0 = faces[(int64_t)g * 3 + 0], g1 = faces[(int64_t)g * 3 + 1], g2 = faces[(int64_t)g * 3 + 2];
                if (row <= 3) {
                    const float4 e1 = tri[(int64_t)g * 3 + 1], e2 = tri[(int64_t)g * 3 + 2];
                    float al;
                    if (g0 == w0) al = mp_angle(e1.x, e1.y, e1.z, e2.x, e2.y, e2.z);
                    else if (g1 == w0) al = mp_angle(-e1.x, -e1.y, -e1.z, e2.x - e1.x, e2.y - e1.y, e2.z - e1.z);
                    else if (g2 == w0) al = mp_angle(-e2.x, -e2.y, -e2.z, e1.x - e2.x, e1.y - e2.y, e1.z - e2.z);
                    else continue;
                    ax = ax + al * ux; ay = ay + al * uy; az = az + al * uz;
                } else {
                    const bool both = (g0 == w0 && (g1 == w1 || g2 == w1)) || (g1 == w0 && (g0 == w1 || g2 == w1)) ||
                                      (g2 == w0 && (g0 == w1 || g1 == w1));
                    if (!both) continue;
                    ax = ax + ux; ay = ay + uy; az = az + uz;
                }
            }
        }
        out[0] = ax; out[1] = ay; out[2] = az;
    }
}

extern "C" int32_t ctx_mesh_pseudonormals(const int64_t *faces, int64_t V, int64_t F, const float *tri, const int32_t *vf_off, const int32_t *vf_face,
                                          int64_t n_vf, float *pn, ctx_stream_t stream)
{
    CTX_REQUIRE(V >= 1 && V <= INT32_MAX, "mesh_pseudonormals: V=%lld outside [1, 2^31)", (long long)V);
    CTX_REQUIRE(F >= 1 && F <= INT32_MAX / 21, "mesh_pseudonormals: F=%lld outside [1, 2^31 / 21)", (long long)F);
    CTX_REQUIRE(n_vf >= 0 && n_vf <= 3 * F, "mesh_pseudonormals: n_vf=%lld outside [0, 3 F]", (long long)n_vf);
    CTX_REQUIRE(faces && tri && vf_off && pn && (vf_face || n_vf == 0), "mesh_pseudonormals: null pointer");
    CTX_REQUIRE(((uintptr_t)tri % 16) == 0, "mesh_pseudonormals: tri must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mesh_pn_face, dim3(capped_blocks(F, MP_BLK, MP_CAP)), dim3(MP_BLK), 0, s, (const float4 *)tri, F, pn);
    hipLaunchKernelGGL(k_mesh_pn_rows, dim3(capped_blocks(F * 6, MP_BLK, MP_CAP)), dim3(MP_BLK), 0, s, faces, V, F, (const float4 *)tri, vf_off, vf_face,
                       n_vf, pn);
    CTX_CHECK_LAUNCH("mesh_pseudonormals");
    return CTX_OK;
}
