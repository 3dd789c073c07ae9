// Where a ray meets the mesh: per-cell triangle lists on the occupancy grid (count, scan, fill), the triangle records (tri_setup) and the
// hit kernel (ray_hit), which walks the grid with occ_walk and tests the triangles listed in the cells it visits.
// Built with -ffp-contract=off: every product, sum and quotient below rounds on its own, in the order written, so the numpy restatement
// (tests/meshhit_rule.py) gives the same bits; it is the definition, this file follows it line by line.
// The lists use one predicate, occ_tri.h's: (cell, face) is listed if and only if ctx_occ_voxelize would store a 1 in that cell for that
// face alone.  The counts are integer adds and every cell's segment is sorted by face id, so neither depends on scheduling.
#include "occ_tri.h"

#define MH_BLK 256
#define MH_CAP 2048                      // blocks of a grid-stride launch: 8 per CU
#define MH_EPS 3.814697265625e-06f       // 2^-18: the slack of the barycentric test

// ---- lists: one wave per triangle, the lanes stride over the candidate cells (the voxeliser's loop) ------------------------------------
// FILL = false: count[cell] += 1 per listed pair.  FILL = true: the pair takes the next free slot of its cell's segment (an atomic cursor;
// the arrival order is undone by k_mesh_cells_sort).  A slot outside the segment or outside [0, n) is never written, whatever the counts say.
template <bool FILL>
__global__ __launch_bounds__(MH_BLK) void k_mesh_cells(const float *__restrict__ vtx, const int64_t *__restrict__ faces, int64_t V, int64_t F, int G, ocm3 lo,
                                                       ocm3 inv, int32_t *__restrict__ count, const int32_t *__restrict__ cell_off, int64_t n,
                                                       int32_t *__restrict__ slots)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = __builtin_amdgcn_readfirstlane((int)(((int64_t)blockIdx.x * MH_BLK + threadIdx.x) >> 6));
    const int64_t nwaves = ((int64_t)gridDim.x * MH_BLK) >> 6;
    for (int64_t f = wave0; f < F; f += nwaves) {
        OccTri T;
        if (!occ_tri_setup(vtx, faces, V, f, G, lo, inv, T)) continue;
        for (int i = lane; i < T.total; i += 64) {
            int cx, cy, cz;
            occ_tri_candidate(T, i, cx, cy, cz);
            if (!occ_tri_cell(T, cx, cy, cz)) continue;
            const int cell = (cz * G + cy) * G + cx;                  // 0 <= c < G on the three axes by the set-up's clamps
            const int k = atomicAdd(&count[cell], 1);
            if (FILL) {
                const int64_t off = cell_off[cell], end = cell_off[cell + 1];
                if (off >= 0 && off + k < end && end <= n) slots[off + k] = (int32_t)f;
            }
        }
    }
}

// exclusive scan of count [ncell] -> cell_off [ncell + 1], total[0] = the sum.  One workgroup (k_fvm_scan's scheme): every thread sums a
// contiguous piece, one Hillis-Steele pass over the 1024 piece sums, then each thread writes its piece's prefixes.  Sums are int64; an
// offset beyond int32 is stored as INT32_MAX (the host refuses such a total before anything reads cell_off).
__global__ __launch_bounds__(1024) void k_mesh_cells_scan(const int32_t *__restrict__ count, int64_t ncell, int32_t *__restrict__ cell_off,
                                                          int64_t *__restrict__ total)
{
    __shared__ int64_t s[1024];
    const int64_t per = (ncell + 1023) / 1024;
    const int64_t i0 = (int64_t)threadIdx.x * per < ncell ? (int64_t)threadIdx.x * per : ncell, i1 = i0 + per < ncell ? i0 + per : ncell;
    int64_t sum = 0;
    for (int64_t i = i0; i < i1; ++i) sum += count[i];
    s[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int64_t t = threadIdx.x >= o ? s[threadIdx.x - o] : 0;
        __syncthreads();
        s[threadIdx.x] += t;
        __syncthreads();
    }
    int64_t run = s[threadIdx.x] - sum;
    for (int64_t i = i0; i < i1; ++i) { cell_off[i] = (int32_t)(run < INT32_MAX ? run : INT32_MAX); run += count[i]; }
    if (threadIdx.x == 1023) {
        cell_off[ncell] = (int32_t)(s[1023] < INT32_MAX ? s[1023] : INT32_MAX);
        total[0] = s[1023];
    }
}

// one wave per cell: entry i of the segment goes to its rank among the segment's entries (face ids of one cell are distinct; the index
// breaks a tie all the same, so the ranks are a permutation of 0 .. len-1 whatever the input).  Any length: the lanes stride over it.
__global__ __launch_bounds__(MH_BLK) void k_mesh_cells_sort(const int32_t *__restrict__ cell_off, int64_t ncell, int64_t n, const int32_t *__restrict__ slots,
                                                            int32_t *__restrict__ cell_tri)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = ((int64_t)blockIdx.x * MH_BLK + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * MH_BLK) >> 6;
    for (int64_t c = wave0; c < ncell; c += nwaves) {
        const int64_t off = cell_off[c], end = cell_off[c + 1];
        if (off < 0 || end > n || end <= off) continue;
        const int len = (int)(end - off);
        for (int i = lane; i < len; i += 64) {
            const int32_t v = slots[off + i];
            int rank = 0;
            for (int j = 0; j < len; ++j) {
                const int32_t w = slots[off + j];
                rank += (w < v || (w == v && j < i)) ? 1 : 0;
            }
            cell_tri[off + rank] = v;
        }
    }
}

static int32_t mesh_cells_args(const char *who, const void *vertices, const void *faces, int64_t V, int64_t F, int32_t G)
{
    CTX_REQUIRE(vertices && faces, "%s: null pointer", who);
    CTX_REQUIRE(G >= 1 && G <= 256, "%s: G=%d outside [1, 256]", who, (int)G);
    CTX_REQUIRE(V >= 1 && F >= 1, "%s: V=%lld, F=%lld: want at least one vertex and one face", who, (long long)V, (long long)F);
    CTX_REQUIRE(V <= INT32_MAX && F <= INT32_MAX, "%s: V=%lld, F=%lld: want both below 2^31", who, (long long)V, (long long)F);
    return CTX_OK;
}

extern "C" int32_t ctx_mesh_cells_count(const float *vertices, const int64_t *faces, int64_t V, int64_t F, int32_t G, float lo_x, float lo_y, float lo_z,
                                        float inv_x, float inv_y, float inv_z, int32_t *count, ctx_stream_t stream)
{
    if (int32_t rc = mesh_cells_args("mesh_cells_count", vertices, faces, V, F, G)) return rc;
    CTX_REQUIRE(count, "mesh_cells_count: null pointer");
    const ocm3 lo = {lo_x, lo_y, lo_z}, inv = {inv_x, inv_y, inv_z};
    hipStream_t s = (hipStream_t)stream;
    const int64_t ncell = (int64_t)G * G * G;
    if (hipMemsetAsync(count, 0, ncell * sizeof(int32_t), s) != hipSuccess) { ctx_set_error("mesh_cells_count: memset failed"); return CTX_E_LAUNCH; }
    hipLaunchKernelGGL(k_mesh_cells<false>, dim3(capped_blocks(F, MH_BLK / 64, MH_CAP)), dim3(MH_BLK), 0, s, vertices, faces, V, F, (int)G, lo, inv, count,
                       (const int32_t *)nullptr, (int64_t)0, (int32_t *)nullptr);
    CTX_CHECK_LAUNCH("mesh_cells_count");
    return CTX_OK;
}

extern "C" int32_t ctx_mesh_cells_scan(const int32_t *count, int64_t ncell, int32_t *cell_off, int64_t *total, ctx_stream_t stream)
{
    CTX_REQUIRE(count && cell_off && total, "mesh_cells_scan: null pointer");
    CTX_REQUIRE(ncell >= 1 && ncell <= (int64_t)256 * 256 * 256, "mesh_cells_scan: ncell=%lld outside [1, 256^3]", (long long)ncell);
    hipLaunchKernelGGL(k_mesh_cells_scan, dim3(1), dim3(1024), 0, (hipStream_t)stream, count, ncell, cell_off, total);
    CTX_CHECK_LAUNCH("mesh_cells_scan");
    return CTX_OK;
}

extern "C" int32_t ctx_mesh_cells_fill(const float *vertices, const int64_t *faces, int64_t V, int64_t F, int32_t G, float lo_x, float lo_y, float lo_z,
                                       float inv_x, float inv_y, float inv_z, const int32_t *cell_off, int64_t n, int32_t *cursor, int32_t *slots,
                                       int32_t *cell_tri, ctx_stream_t stream)
{
    if (int32_t rc = mesh_cells_args("mesh_cells_fill", vertices, faces, V, F, G)) return rc;
    CTX_REQUIRE(n >= 0 && n <= INT32_MAX, "mesh_cells_fill: n=%lld outside [0, 2^31)", (long long)n);
    if (n == 0) return CTX_OK;
    CTX_REQUIRE(cell_off && cursor && slots && cell_tri, "mesh_cells_fill: null pointer");
    CTX_REQUIRE(slots != cell_tri, "mesh_cells_fill: the workspace slots must not be cell_tri");
    const ocm3 lo = {lo_x, lo_y, lo_z}, inv = {inv_x, inv_y, inv_z};
    hipStream_t s = (hipStream_t)stream;
    const int64_t ncell = (int64_t)G * G * G;
    if (hipMemsetAsync(cursor, 0, ncell * sizeof(int32_t), s) != hipSuccess) { ctx_set_error("mesh_cells_fill: memset failed"); return CTX_E_LAUNCH; }
    hipLaunchKernelGGL(k_mesh_cells<true>, dim3(capped_blocks(F, MH_BLK / 64, MH_CAP)), dim3(MH_BLK), 0, s, vertices, faces, V, F, (int)G, lo, inv, cursor,
                       cell_off, n, slots);
    hipLaunchKernelGGL(k_mesh_cells_sort, dim3(capped_blocks(ncell, MH_BLK / 64, MH_CAP)), dim3(MH_BLK), 0, s, cell_off, ncell, n, (const int32_t *)slots,
                       cell_tri);
    CTX_CHECK_LAUNCH("mesh_cells_fill");
    return CTX_OK;
}

// ---- vertex -> face incidence lists (for the pseudonormal tables of meshpn.hip): count, the scan above, fill ----------------------------
// One lane per face.  A face whose three ids lie in [0, V) lists itself once per corner under that corner's vertex id; any other face is
// in no list.  FILL as for the cells: an atomic cursor into `slots`, and k_mesh_cells_sort puts every segment in ascending face id.
template <bool FILL>
__global__ __launch_bounds__(MH_BLK) void k_mesh_vertex_faces(const int64_t *__restrict__ faces, int64_t V, int64_t F, int32_t *__restrict__ count,
                                                              const int32_t *__restrict__ vf_off, int64_t n, int32_t *__restrict__ slots)
{
    for (int64_t f = (int64_t)blockIdx.x * MH_BLK + threadIdx.x; f < F; f += (int64_t)gridDim.x * MH_BLK) {
        const int64_t iv[3] = {faces[f * 3 + 0], faces[f * 3 + 1], faces[f * 3 + 2]};
        if (iv[0] < 0 || iv[0] >= V || iv[1] < 0 || iv[1] >= V || iv[2] < 0 || iv[2] >= V) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int k = atomicAdd(&count[iv[c]], 1);
            if (FILL) {
                const int64_t off = vf_off[iv[c]], end = vf_off[iv[c] + 1];
                if (off >= 0 && off + k < end && end <= n) slots[off + k] = (int32_t)f;
            }
        }
    }
}

static int32_t mesh_vertex_faces_args(const char *who, const void *faces, int64_t V, int64_t F)
{
    CTX_REQUIRE(faces, "%s: null pointer", who);
    CTX_REQUIRE(V >= 1 && V <= (int64_t)256 * 256 * 256, "%s: V=%lld outside [1, 256^3] (the scan's reach)", who, (long long)V);
    CTX_REQUIRE(F >= 1 && F <= INT32_MAX / 3, "%s: F=%lld outside [1, 2^31 / 3)", who, (long long)F);
    return CTX_OK;
}

extern "C" int32_t ctx_mesh_vertex_faces_count(const int64_t *faces, int64_t V, int64_t F, int32_t *count, ctx_stream_t stream)
{
    if (int32_t rc = mesh_vertex_faces_args("mesh_vertex_faces_count", faces, V, F)) return rc;
    CTX_REQUIRE(count, "mesh_vertex_faces_count: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(count, 0, V * sizeof(int32_t), s) != hipSuccess) { ctx_set_error("mesh_vertex_faces_count: memset failed"); return CTX_E_LAUNCH; }
    hipLaunchKernelGGL(k_mesh_vertex_faces<false>, dim3(capped_blocks(F, MH_BLK, MH_CAP)), dim3(MH_BLK), 0, s, faces, V, F, count,
                       (const int32_t *)nullptr, (int64_t)0, (int32_t *)nullptr);
    CTX_CHECK_LAUNCH("mesh_vertex_faces_count");
    return CTX_OK;
}

extern "C" int32_t ctx_mesh_vertex_faces_fill(const int64_t *faces, int64_t V, int64_t F, const int32_t *vf_off, int64_t n, int32_t *cursor,
                                              int32_t *slots, int32_t *vf_face, ctx_stream_t stream)
{
    if (int32_t rc = mesh_vertex_faces_args("mesh_vertex_faces_fill", faces, V, F)) return rc;
    CTX_REQUIRE(n >= 0 && n <= 3 * F, "mesh_vertex_faces_fill: n=%lld outside [0, 3 F]", (long long)n);
    if (n == 0) return CTX_OK;
    CTX_REQUIRE(vf_off && cursor && slots && vf_face, "mesh_vertex_faces_fill: null pointer");
    CTX_REQUIRE(slots != vf_face, "mesh_vertex_faces_fill: the workspace slots must not be vf_face");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(cursor, 0, V * sizeof(int32_t), s) != hipSuccess) { ctx_set_error("mesh_vertex_faces_fill: memset failed"); return CTX_E_LAUNCH; }
    hipLaunchKernelGGL(k_mesh_vertex_faces<true>, dim3(capped_blocks(F, MH_BLK, MH_CAP)), dim3(MH_BLK), 0, s, faces, V, F, cursor, vf_off, n, slots);
    hipLaunchKernelGGL(k_mesh_cells_sort, dim3(capped_blocks(V, MH_BLK / 64, MH_CAP)), dim3(MH_BLK), 0, s, vf_off, V, n, (const int32_t *)slots, vf_face);
    CTX_CHECK_LAUNCH("mesh_vertex_faces_fill");
    return CTX_OK;
}

// ---- triangle records: v0, e1 = v1 - v0, e2 = v2 - v0, each padded to four floats; NaN for a face the voxeliser would not take ----------
__global__ __launch_bounds__(MH_BLK) void k_mesh_tri_setup(const float *__restrict__ vtx, const int64_t *__restrict__ faces, int64_t V, int64_t F,
                                                           float4 *__restrict__ tri)
{
    for (int64_t f = (int64_t)blockIdx.x * MH_BLK + threadIdx.x; f < F; f += (int64_t)gridDim.x * MH_BLK) {
        const int64_t iv[3] = {faces[f * 3 + 0], faces[f * 3 + 1], faces[f * 3 + 2]};
        bool ok = true;
        float p[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            ok = ok && iv[k] >= 0 && iv[k] < V;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                p[k][a] = ok ? vtx[iv[k] * 3 + a] : NAN;
                ok = ok && ocm_finite(p[k][a]);
            }
        }
        if (ok) {
            tri[f * 3 + 0] = make_float4(p[0][0], p[0][1], p[0][2], 0.f);
            tri[f * 3 + 1] = make_float4(p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2], 0.f);
            tri[f * 3 + 2] = make_float4(p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2], 0.f);
        } else {
            tri[f * 3 + 0] = tri[f * 3 + 1] = tri[f * 3 + 2] = make_float4(NAN, NAN, NAN, NAN);
        }
    }
}

extern "C" int32_t ctx_mesh_tri_setup(const float *vertices, const int64_t *faces, int64_t V, int64_t F, float *tri, ctx_stream_t stream)
{
    CTX_REQUIRE(vertices && faces && tri, "mesh_tri_setup: null pointer");
    CTX_REQUIRE(V >= 1 && F >= 1, "mesh_tri_setup: V=%lld, F=%lld: want at least one vertex and one face", (long long)V, (long long)F);
    CTX_REQUIRE(V <= INT32_MAX && F <= INT32_MAX, "mesh_tri_setup: V=%lld, F=%lld: want both below 2^31", (long long)V, (long long)F);
    CTX_REQUIRE(((uintptr_t)tri % 16) == 0, "mesh_tri_setup: tri must be 16-byte aligned");
    hipLaunchKernelGGL(k_mesh_tri_setup, dim3(capped_blocks(F, MH_BLK, MH_CAP)), dim3(MH_BLK), 0, (hipStream_t)stream, vertices, faces, V, F, (float4 *)tri);
    CTX_CHECK_LAUNCH("mesh_tri_setup");
    return CTX_OK;
}

// ---- the hit kernel: one lane per ray, the cell walk is occ_walk with a visitor that takes the cell and may stop ------------------------
// ANY: stop at the first accepted triangle and store hit only.  OWN: skip the triangles related to own_face[r] (uvgather.hip's integer
// rule: the face itself, or one that shares a vertex id with it in `faces`).
template <bool ANY, bool OWN>
__global__ __launch_bounds__(MH_BLK) void k_mesh_ray_hit(const float *__restrict__ ro, const float *__restrict__ rd, int64_t R, float near, float far,
                                                         const uint8_t *__restrict__ cells, int G, ocm3 lo, ocm3 hi, ocm3 inv, ocm3 h,
                                                         const int32_t *__restrict__ cell_off, const int32_t *__restrict__ cell_tri, int64_t n,
                                                         const float4 *__restrict__ tri, const int64_t *__restrict__ faces, int F,
                                                         const int64_t *__restrict__ own_face, uint8_t *__restrict__ hit, float *__restrict__ t_hit,
                                                         int32_t *__restrict__ face_hit, float2 *__restrict__ uv_hit)
{
    for (int64_t r = (int64_t)blockIdx.x * MH_BLK + threadIdx.x; r < R; r += (int64_t)gridDim.x * MH_BLK) {
        const float ox = ro[r * 3 + 0], oy = ro[r * 3 + 1], oz = ro[r * 3 + 2], dx = rd[r * 3 + 0], dy = rd[r * 3 + 1], dz = rd[r * 3 + 2];
        int64_t own = -1, a0 = -1, a1 = -1, a2 = -1;
        if (OWN) {
            own = own_face[r];
            if (own >= 0 && own < F) { a0 = faces[own * 3 + 0]; a1 = faces[own * 3 + 1]; a2 = faces[own * 3 + 2]; }
            else own = -1;
        }
        bool found = false;
        float bt = far, bu = 0.f, bv = 0.f;
        int bf = -1;
        occ_walk(ox, oy, oz, dx, dy, dz, near, far, cells, G, lo, hi, inv, h, [&](bool occ, float tin, float tout, int cell) -> bool {
            if (occ) {
                const int k0 = cell_off[cell], k1 = cell_off[cell + 1];
                for (int k = k0 < 0 ? 0 : k0; k < k1 && k < n; ++k) {
                    const int f = cell_tri[k];
                    if (f < 0 || f >= F) continue;
                    if (OWN && own >= 0) {
                        if (f == own) continue;
                        const int64_t b0 = faces[(int64_t)f * 3 + 0], b1 = faces[(int64_t)f * 3 + 1], b2 = faces[(int64_t)f * 3 + 2];
                        if (b0 == a0 || b0 == a1 || b0 == a2 || b1 == a0 || b1 == a1 || b1 == a2 || b2 == a0 || b2 == a1 || b2 == a2) continue;
                    }
                    const float4 v0 = tri[(int64_t)f * 3 + 0], e1 = tri[(int64_t)f * 3 + 1], e2 = tri[(int64_t)f * 3 + 2];
                    const float px = dy * e2.z - dz * e2.y, py = dz * e2.x - dx * e2.z, pz = dx * e2.y - dy * e2.x;        // p = d x e2
                    const float det = (e1.x * px + e1.y * py) + e1.z * pz;
                    if (det == 0.f) continue;
                    const float idet = 1.0f / det;
                    if (!ocm_finite(idet)) continue;
                    const float sx = ox - v0.x, sy = oy - v0.y, sz = oz - v0.z;
                    const float u = ((sx * px + sy * py) + sz * pz) * idet;
                    const float qx = sy * e1.z - sz * e1.y, qy = sz * e1.x - sx * e1.z, qz = sx * e1.y - sy * e1.x;        // q = s x e1
                    const float v = ((dx * qx + dy * qy) + dz * qz) * idet;
                    const float t = ((e2.x * qx + e2.y * qy) + e2.z * qz) * idet;
                    if (!ocm_finite(t)) continue;
                    if (!(u >= -MH_EPS && v >= -MH_EPS && u + v <= 1.0f + MH_EPS && t >= near && t <= far)) continue;
                    if (ANY) { found = true; return true; }
                    if (!found || t < bt || (t == bt && f < bf)) { found = true; bt = t; bu = u; bv = v; bf = f; }
                }
            }
            return found && bt <= tout;
        });
        hit[r] = found ? 1 : 0;
        if (!ANY) {
            t_hit[r] = found ? bt : far;
            face_hit[r] = found ? bf : -1;
            uv_hit[r] = found ? make_float2(bu, bv) : make_float2(0.f, 0.f);
        }
    }
}

extern "C" int32_t ctx_mesh_ray_hit(const float *rays_o, const float *rays_d, int64_t R, float near, float far, const uint8_t *cells, int32_t G,
                                    float lo_x, float lo_y, float lo_z, float hi_x, float hi_y, float hi_z, float inv_x, float inv_y, float inv_z,
                                    float h_x, float h_y, float h_z, const int32_t *cell_off, const int32_t *cell_tri, int64_t n, const float *tri,
                                    const int64_t *faces, int64_t F, const int64_t *own_face, int32_t mode, uint8_t *hit, float *t, int32_t *face,
                                    float *uv, ctx_stream_t stream)
{
    CTX_REQUIRE(R >= 0 && R <= INT32_MAX, "mesh_ray_hit: R=%lld outside [0, 2^31)", (long long)R);
    CTX_REQUIRE(mode == 0 || mode == 1, "mesh_ray_hit: mode=%d: want 0 (nearest) or 1 (any)", (int)mode);
    CTX_REQUIRE(G >= 1 && G <= 256, "mesh_ray_hit: G=%d outside [1, 256]", (int)G);
    CTX_REQUIRE(F >= 1 && F <= INT32_MAX, "mesh_ray_hit: F=%lld outside [1, 2^31)", (long long)F);
    CTX_REQUIRE(n >= 0 && n <= INT32_MAX, "mesh_ray_hit: n=%lld outside [0, 2^31)", (long long)n);
    CTX_REQUIRE(near < far && fabsf(near) < INFINITY && fabsf(far) < INFINITY, "mesh_ray_hit: want finite near < far, got %g, %g", (double)near,
                (double)far);
    if (R == 0) return CTX_OK;
    CTX_REQUIRE(rays_o && rays_d && cells && cell_off && tri && faces && hit && (cell_tri || n == 0), "mesh_ray_hit: null pointer");
    CTX_REQUIRE(mode == 1 || (t && face && uv), "mesh_ray_hit: mode 0 (nearest) stores t, face and uv: null pointer");
    CTX_REQUIRE(((uintptr_t)tri % 16) == 0 && ((uintptr_t)uv % 8) == 0, "mesh_ray_hit: tri must be 16-byte and uv 8-byte aligned");
    const ocm3 lo = {lo_x, lo_y, lo_z}, hi = {hi_x, hi_y, hi_z}, inv = {inv_x, inv_y, inv_z}, h = {h_x, h_y, h_z};
    const dim3 grid(capped_blocks(R, MH_BLK, MH_CAP)), blk(MH_BLK);
    CTX_BOOL_GO(mode == 1, ANY, CTX_BOOL_GO(own_face != nullptr, OWN,
        hipLaunchKernelGGL((k_mesh_ray_hit<ANY, OWN>), grid, blk, 0, (hipStream_t)stream, rays_o, rays_d, R, near, far, cells, (int)G, lo, hi, inv, h,
                           cell_off, cell_tri, n, (const float4 *)tri, faces, (int)F, own_face, hit, t, face, (float2 *)uv)));
    CTX_CHECK_LAUNCH("mesh_ray_hit");
    return CTX_OK;
}
