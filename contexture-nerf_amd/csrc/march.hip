// Marching the occupancy grid into ragged per-ray sample lists: one lane per ray walks the grid (occ_walk, the walk of
// the span kernel) and places samples at a fixed world-space step inside its runs of occupied cells; two passes, march_count and
// march_write, with the host's exclusive scan of the counts between them.
// Built with -ffp-contract=off: every product, sum and quotient rounds on its own, in the order written, so the numpy restatement
// (tests/march_rule.py) gives the same bits; it is the definition.  No atomics; every output element has one writer.
#include "occ_walk.h"

#define MARCH_BLK 256
#define MARCH_CAP 2048          // blocks of a grid-stride launch: 8 per CU
#define MARCH_RUN_MAX 4097.f    // samples of one run: one more than a ray may hold, so a count stays an int32 whatever step is

// Samples of the closed run [a, b]: none unless its world length is > 0 (false for NaN), else k = ceil(len / step) in [1, 4097] of width dt.
__device__ __forceinline__ int march_run(float a, float b, float nrm, float step, float &dt)
{
    const float len = (b - a) * nrm;
    if (!(len > 0.f)) return 0;
    const int k = (int)fminf(fmaxf(ceilf(len / step), 1.f), MARCH_RUN_MAX);
    dt = (b - a) / (float)k;
    return k;
}

// The runs of ray r in walk order: a maximal sequence of consecutive occupied cells, closed by an empty cell (also one of zero length)
// or by the end of the walk.  emit(a, b) per closed run.
template <class Emit>
__device__ __forceinline__ void march_runs(const float *__restrict__ ro, const float *__restrict__ rd, int64_t r, float near, float far,
                                           const uint8_t *__restrict__ cells, int G, ocm3 lo, ocm3 hi, ocm3 inv, ocm3 h, Emit &&emit)
{
    bool open = false;
    float a = 0.f, b = 0.f;
    occ_walk(ro[r * 3 + 0], ro[r * 3 + 1], ro[r * 3 + 2], rd[r * 3 + 0], rd[r * 3 + 1], rd[r * 3 + 2], near, far, cells, G, lo, hi, inv, h,
             [&](bool occ, float tin, float tout) {
                 if (occ) {
                     if (!open) { a = tin; open = true; }
                     b = tout;
                 } else if (open) {
                     emit(a, b);
                     open = false;
                 }
             });
    if (open) emit(a, b);
}

__global__ __launch_bounds__(MARCH_BLK) void k_occ_march_count(const float *__restrict__ ro, const float *__restrict__ rd, int64_t R, float near,
                                                               float far, const uint8_t *__restrict__ cells, int G, ocm3 lo, ocm3 hi, ocm3 inv,
                                                               ocm3 h, float step, int32_t *__restrict__ count)
{
    for (int64_t r = (int64_t)blockIdx.x * MARCH_BLK + threadIdx.x; r < R; r += (int64_t)gridDim.x * MARCH_BLK) {
        const float dx = rd[r * 3 + 0], dy = rd[r * 3 + 1], dz = rd[r * 3 + 2];
        const float nrm = sqrtf((dx * dx + dy * dy) + dz * dz);
        int32_t c = 0;                                                // <= (3G + 3) * 4097 < 2^22
        march_runs(ro, rd, r, near, far, cells, G, lo, hi, inv, h, [&](float a, float b) {
            float dt;
            c += march_run(a, b, nrm, step, dt);
        });
        count[r] = c;
    }
}

// The same walk; ray r stores samples ray_off[r] .. ray_off[r+1] and never past that end (nor outside [0, n)), whatever it computes.
__global__ __launch_bounds__(MARCH_BLK) void k_occ_march_write(const float *__restrict__ ro, const float *__restrict__ rd, int64_t R, float near,
                                                               float far, const uint8_t *__restrict__ cells, int G, ocm3 lo, ocm3 hi, ocm3 inv,
                                                               ocm3 h, float step, const int64_t *__restrict__ ray_off, const float *__restrict__ u,
                                                               int64_t n, int32_t *__restrict__ ray_id, float *__restrict__ t, float *__restrict__ dts,
                                                               float *__restrict__ pts)
{
    for (int64_t r = (int64_t)blockIdx.x * MARCH_BLK + threadIdx.x; r < R; r += (int64_t)gridDim.x * MARCH_BLK) {
        int64_t pos = ray_off[r], end = ray_off[r + 1];
        if (pos < 0 || end > n) continue;
        if (pos >= end) continue;
        const float ox = ro[r * 3 + 0], oy = ro[r * 3 + 1], oz = ro[r * 3 + 2];
        const float dx = rd[r * 3 + 0], dy = rd[r * 3 + 1], dz = rd[r * 3 + 2];
        const float nrm = sqrtf((dx * dx + dy * dy) + dz * dz);
        march_runs(ro, rd, r, near, far, cells, G, lo, hi, inv, h, [&](float a, float b) {
            float dt;
            const int k = march_run(a, b, nrm, step, dt);
            for (int j = 0; j < k && pos < end; ++j, ++pos) {
                const float tj = a + ((float)j + (u ? u[pos] : 0.5f)) * dt;
                ray_id[pos] = (int32_t)r;
                t[pos] = tj;
                dts[pos] = dt;
                pts[pos * 3 + 0] = ox + dx * tj;                      // one product, one sum per axis: the bits of ctx_occ_points
                pts[pos * 3 + 1] = oy + dy * tj;
                pts[pos * 3 + 2] = oz + dz * tj;
            }
        });
    }
}

#define MARCH_REQUIRE_GRID(who)                                                                                                               \
    CTX_REQUIRE(G >= 1 && G <= 256, who ": G=%d outside [1, 256]", (int)G);                                                                   \
    CTX_REQUIRE(R >= 1 && R <= INT32_MAX, who ": R=%lld outside [1, 2^31)", (long long)R);                                                    \
    CTX_REQUIRE(near < far && fabsf(near) < INFINITY && fabsf(far) < INFINITY, who ": want finite near < far, got %g, %g", (double)near,      \
                (double)far);                                                                                                                 \
    CTX_REQUIRE(step > 0.f && step < INFINITY, who ": step=%g: want a finite world length > 0", (double)step)

extern "C" int32_t ctx_occ_march_count(const float *rays_o, const float *rays_d, int64_t R, float near, float far, const uint8_t *cells, int32_t G,
                                       float lo_x, float lo_y, float lo_z, float hi_x, float hi_y, float hi_z, float inv_x, float inv_y,
                                       float inv_z, float h_x, float h_y, float h_z, float step, int32_t *count, ctx_stream_t stream)
{
    CTX_REQUIRE(rays_o && rays_d && cells && count, "occ_march_count: null pointer");
    MARCH_REQUIRE_GRID("occ_march_count");
    const ocm3 lo = {lo_x, lo_y, lo_z}, hi = {hi_x, hi_y, hi_z}, inv = {inv_x, inv_y, inv_z}, h = {h_x, h_y, h_z};
    hipLaunchKernelGGL(k_occ_march_count, dim3(capped_blocks(R, MARCH_BLK, MARCH_CAP)), dim3(MARCH_BLK), 0, (hipStream_t)stream, rays_o, rays_d, R,
                       near, far, cells, (int)G, lo, hi, inv, h, step, count);
    CTX_CHECK_LAUNCH("occ_march_count");
    return CTX_OK;
}

extern "C" int32_t ctx_occ_march_write(const float *rays_o, const float *rays_d, int64_t R, float near, float far, const uint8_t *cells, int32_t G,
                                       float lo_x, float lo_y, float lo_z, float hi_x, float hi_y, float hi_z, float inv_x, float inv_y,
                                       float inv_z, float h_x, float h_y, float h_z, float step, const int64_t *ray_off, const float *u, int64_t n,
                                       int32_t *ray_id, float *t, float *dt, float *pts, ctx_stream_t stream)
{
    CTX_REQUIRE(rays_o && rays_d && cells && ray_off, "occ_march_write: null pointer");
    MARCH_REQUIRE_GRID("occ_march_write");
    CTX_REQUIRE(n >= 0 && n <= INT32_MAX, "occ_march_write: n=%lld outside [0, 2^31)", (long long)n);
    if (n == 0) return CTX_OK;
    CTX_REQUIRE(ray_id && t && dt && pts, "occ_march_write: null output with n=%lld", (long long)n);
    const ocm3 lo = {lo_x, lo_y, lo_z}, hi = {hi_x, hi_y, hi_z}, inv = {inv_x, inv_y, inv_z}, h = {h_x, h_y, h_z};
    hipLaunchKernelGGL(k_occ_march_write, dim3(capped_blocks(R, MARCH_BLK, MARCH_CAP)), dim3(MARCH_BLK), 0, (hipStream_t)stream, rays_o, rays_d, R,
                       near, far, cells, (int)G, lo, hi, inv, h, step, ray_off, u, n, ray_id, t, dt, pts);
    CTX_CHECK_LAUNCH("occ_march_write");
    return CTX_OK;
}
