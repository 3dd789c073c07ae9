// Marching the occupancy grid into ragged per-ray sample lists, and the compositing on such lists.
//   march_count / march_write: one lane per ray walks the grid (occ_walk, the walk of the span kernel) and places samples at a fixed
//     world-space step inside its runs of occupied cells; two passes with the host's exclusive scan of the counts between them.
//   raymarch_packed_fwd / _bwd: the dense compositing kernels with a per-ray sample count and a given distance (composite.h).
//   distortion_packed_fwd / _bwd: mip-NeRF 360's distortion loss of the weights on the same lists, by prefix sums.
// Built with -ffp-contract=off: every product, sum and quotient rounds on its own, in the order written, so the numpy restatement
// (tests/march_rule.py) gives the same bits; it is the definition.  No atomics; every output element has one writer.
#include "occ_walk.h"
#include "composite.h"

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

// ---- compositing on the lists: k_composite / k_composite_bwd with S = ray_off[r+1] - ray_off[r] and dist = dt * |d| -----------------------
// One wavefront per ray, lane s of chunk c holds sample ray_off[r] + 64c + s.  No sample gets the 1e10 distance: the background shows
// through what the runs leave.  Rays here hold a dozen or so samples, so most of a wave idles; a several-rays-per-wave form is follow-up.
__device__ __forceinline__ int packed_count(const int64_t *__restrict__ ray_off, int64_t r, int64_t n, int64_t &off)
{
    off = ray_off[r];
    const int64_t end = ray_off[r + 1];
    return (off >= 0 && end >= off && end <= n) ? (int)(end - off) : 0;          // n < 2^31; a ray_off outside the lists reads nothing
}

template <bool NOISE>
__global__ __launch_bounds__(256) void k_composite_packed(const float4 *__restrict__ raw, const float *__restrict__ tv, const float *__restrict__ dtv,
                                                          const float *__restrict__ rays_d, const float *__restrict__ noise,
                                                          const int64_t *__restrict__ ray_off, int64_t R, int64_t n, int white,
                                                          float *__restrict__ rgb, float *__restrict__ disp, float *__restrict__ acc,
                                                          float *__restrict__ weights, float *__restrict__ depth)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * 256) >> 6;
    for (int64_t r = wave; r < R; r += nwaves) {
        int64_t off;
        const int S = packed_count(ray_off, r, n, off);
        const int nch = (S + 63) >> 6;
        const float d0 = rays_d[r * 3 + 0], d1 = rays_d[r * 3 + 1], d2 = rays_d[r * 3 + 2];
        const float nrm = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
        float Tc = 1.0f, c0 = 0.f, c1 = 0.f, c2 = 0.f, dep = 0.f, a = 0.f;
        for (int ch = 0; ch < nch; ++ch) {
            const int s = ch * 64 + lane;
            const bool ok = s < S;
            const float4 q = ok ? raw[off + s] : make_float4(0.f, 0.f, 0.f, 0.f);
            const float zv = ok ? tv[off + s] : 0.f;
            const float dist = (ok ? dtv[off + s] : 0.f) * nrm;
            const float nz = (NOISE && ok) ? noise[off + s] : 0.f;
            float e, alpha, t, inc, exc;
            composite_rest<NOISE>(q.w, nz, dist, ok, e, alpha, t);
            composite_prefix(t, inc, exc);
            float w = alpha * (Tc * exc);
            if (weights && ok) weights[off + s] = w;
            c0 += w * composite_sigmoid(q.x);
            c1 += w * composite_sigmoid(q.y);
            c2 += w * composite_sigmoid(q.z);
            dep += w * zv;
            a += w;
            Tc = Tc * __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, inc), 63));
        }
        composite_finish(lane, r, white, c0, c1, c2, dep, a, rgb, disp, acc, depth);          // S = 0: acc = depth = 0, disp = 0 / 0
    }
}

template <bool NOISE>
__global__ __launch_bounds__(256) void k_composite_packed_bwd(const float4 *__restrict__ raw, const float *__restrict__ tv,
                                                              const float *__restrict__ dtv, const float *__restrict__ rays_d,
                                                              const float *__restrict__ noise, const int64_t *__restrict__ ray_off, int64_t R,
                                                              int64_t n, int white, const float *__restrict__ g_rgb, const float *__restrict__ g_disp,
                                                              const float *__restrict__ g_acc, const float *__restrict__ g_weights,
                                                              const float *__restrict__ g_depth, float4 *__restrict__ grad_raw)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * 256) >> 6;
    for (int64_t r = wave; r < R; r += nwaves) {
        int64_t off;
        const int S = packed_count(ray_off, r, n, off);
        if (S > COMPOSITE_BWD_MAX_S) {                                  // more chunks than the table holds: poisoned, not silently wrong
            const float bad = __builtin_nanf("");
            for (int s = lane; s < S; s += 64) grad_raw[off + s] = make_float4(bad, bad, bad, bad);
            continue;
        }
        const int nch = (S + 63) >> 6;
        const float d0 = rays_d[r * 3 + 0], d1 = rays_d[r * 3 + 1], d2 = rays_d[r * 3 + 2];
        const float nrm = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
        const float4 *rawr = raw + off;
        const float *zr = tv + off, *dr = dtv + off, *nr = NOISE ? noise + off : nullptr;
        float Tc = 1.0f, tcv = 1.0f, dep = 0.f, a = 0.f;
        for (int ch = 0; ch < nch; ++ch) {
            const int s = ch * 64 + lane;
            const bool ok = s < S;
            const float qw = ok ? rawr[s].w : 0.f;
            const float zv = ok ? zr[s] : 0.f;
            const float dist = (ok ? dr[s] : 0.f) * nrm;
            const float nz = (NOISE && ok) ? nr[s] : 0.f;
            float e, alpha, t, inc, exc;
            composite_rest<NOISE>(qw, nz, dist, ok, e, alpha, t);
            composite_prefix(t, inc, exc);
            if (lane == ch) tcv = Tc;
            float w = alpha * (Tc * exc);
            dep += w * zv;
            a += w;
            Tc = Tc * __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, inc), 63));
        }
        if (nch == 0) continue;                                         // an empty ray has no row of grad_raw
        const float sd = wave_sum_dpp(dep), sa = wave_sum_dpp(a);
        float g0, g1, g2, gd, ga;
        composite_bwd_upstream(r, white, sd, sa, g_rgb, g_disp, g_acc, g_depth, g0, g1, g2, gd, ga);
        float carry = 0.f;                                              // sum of G_k w_k over the chunks behind this one
        for (int ch = nch - 1; ch >= 0; --ch) {
            const int s = ch * 64 + lane;
            const bool ok = s < S;
            const float4 q = ok ? rawr[s] : make_float4(0.f, 0.f, 0.f, 0.f);
            const float zv = ok ? zr[s] : 0.f;
            const float dist = (ok ? dr[s] : 0.f) * nrm;
            const float nz = (NOISE && ok) ? nr[s] : 0.f;
            const float gw = (g_weights && ok) ? g_weights[off + s] : 0.f;
            float e, alpha, t, inc, exc;
            composite_rest<NOISE>(q.w, nz, dist, ok, e, alpha, t);
            composite_prefix(t, inc, exc);
            const float T = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, tcv), ch)) * exc;
            const float pre = NOISE ? q.w + nz : q.w;
            const float4 o = composite_bwd_sample(q, pre, zv, gw, ok, lane, dist, e, alpha, t, T, g0, g1, g2, gd, ga, carry);
            if (ok) grad_raw[off + s] = o;
        }
    }
}

static unsigned packed_blocks(int64_t R) { return capped_blocks(R, 4, 262144); }          // one ray per wave up to 1 M rays, as k_composite

extern "C" int32_t ctx_raymarch_packed_fwd(const float *raw, const float *t, const float *dt, const float *rays_d, const float *noise,
                                           const int64_t *ray_off, int64_t R, int64_t n, int32_t white_bkgd, float *rgb, float *disp, float *acc,
                                           float *weights, float *depth, ctx_stream_t stream)
{
    CTX_REQUIRE(rays_d && ray_off && rgb && disp && acc && depth && R > 0, "raymarch_packed: bad args");
    CTX_REQUIRE(n >= 0 && n <= INT32_MAX, "raymarch_packed: n=%lld outside [0, 2^31)", (long long)n);
    CTX_REQUIRE(n == 0 || (raw && t && dt), "raymarch_packed: null list with n=%lld", (long long)n);
    CTX_REQUIRE(((uintptr_t)raw % 16) == 0, "raymarch_packed: raw must be 16-byte aligned");
    CTX_BOOL_GO(noise != nullptr, NZ, hipLaunchKernelGGL(k_composite_packed<NZ>, dim3(packed_blocks(R)), dim3(256), 0, (hipStream_t)stream,
                                                         (const float4 *)raw, t, dt, rays_d, noise, ray_off, R, n, (int)white_bkgd, rgb, disp, acc,
                                                         weights, depth));
    CTX_CHECK_LAUNCH("raymarch_packed");
    return CTX_OK;
}

extern "C" int32_t ctx_raymarch_packed_bwd(const float *raw, const float *t, const float *dt, const float *rays_d, const float *noise,
                                           const int64_t *ray_off, int64_t R, int64_t n, int32_t white_bkgd, const float *g_rgb,
                                           const float *g_disp, const float *g_acc, const float *g_weights, const float *g_depth, float *grad_raw,
                                           ctx_stream_t stream)
{
    CTX_REQUIRE(rays_d && ray_off && R > 0, "raymarch_packed_bwd: bad args");
    CTX_REQUIRE(n >= 0 && n <= INT32_MAX, "raymarch_packed_bwd: n=%lld outside [0, 2^31)", (long long)n);
    if (n == 0) return CTX_OK;
    CTX_REQUIRE(raw && t && dt && grad_raw, "raymarch_packed_bwd: null list with n=%lld", (long long)n);
    CTX_REQUIRE(((uintptr_t)raw % 16) == 0 && ((uintptr_t)grad_raw % 16) == 0, "raymarch_packed_bwd: raw and grad_raw must be 16-byte aligned");
    CTX_BOOL_GO(noise != nullptr, NZ, hipLaunchKernelGGL(k_composite_packed_bwd<NZ>, dim3(packed_blocks(R)), dim3(256), 0, (hipStream_t)stream,
                                                         (const float4 *)raw, t, dt, rays_d, noise, ray_off, R, n, (int)white_bkgd, g_rgb, g_disp,
                                                         g_acc, g_weights, g_depth, (float4 *)grad_raw));
    CTX_CHECK_LAUNCH("raymarch_packed_bwd");
    return CTX_OK;
}

// ---- distortion loss on the lists (definition: tests/distortion_rule.py) -------------------------------------------------
// Per ray, with x_i = (t_i - t_0) * |d| and delta_i = dt_i * |d| in world lengths and t ascending (a precondition, not checked):
//   L = sum_i w_i * (2 * (x_i * W_<i - V_<i) + delta_i * w_i / 3),  W_<i = sum_{j<i} w_j,  V_<i = sum_{j<i} w_j x_j
//   dL/dw_i = 2 * (x_i * (W_<i - W_>i) - (V_<i - V_>i)) + 2 * w_i * delta_i / 3,  W_>i = W - W_<=i,  V_>i = V - V_<=i
// The layout is k_composite_packed's: one wavefront per ray, lane s of chunk c holds sample ray_off[r] + 64c + s.  The chunks are chained
// by two carried scalars (W, V), not by a chunk table, so there is no 4096-sample limit: a ray may hold any count below 2^31.
// One chunk of ray samples: the lane's w, x, delta (0 in a lane past the end) and the prefix sums of w and w * x, the carries included.
struct dist_chunk {
    float w, x, dl, Wex, Vex, Win, Vin;
};
__device__ __forceinline__ dist_chunk distortion_chunk(const float *__restrict__ wr, const float *__restrict__ tr, const float *__restrict__ dr,
                                                       int s, int S, float t0, float nrm, float &Wc, float &Vc)
{
    dist_chunk c;
    const bool ok = s < S;
    c.w = ok ? wr[s] : 0.f;
    c.x = ok ? (tr[s] - t0) * nrm : 0.f;
    c.dl = ok ? dr[s] * nrm : 0.f;
    float winc, wexc, vinc, vexc;
    composite_prefix_sum(c.w, winc, wexc);
    composite_prefix_sum(c.w * c.x, vinc, vexc);
    c.Wex = Wc + wexc; c.Win = Wc + winc;
    c.Vex = Vc + vexc; c.Vin = Vc + vinc;
    Wc = Wc + __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, winc), 63));
    Vc = Vc + __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, vinc), 63));
    return c;
}

__global__ __launch_bounds__(256) void k_distortion_packed(const float *__restrict__ weights, const float *__restrict__ tv,
                                                           const float *__restrict__ dtv, const float *__restrict__ rays_d,
                                                           const int64_t *__restrict__ ray_off, int64_t R, int64_t n, float *__restrict__ loss)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * 256) >> 6;
    for (int64_t r = wave; r < R; r += nwaves) {
        int64_t off;
        const int S = packed_count(ray_off, r, n, off);
        if (S == 0) {                                                   // an empty ray (most rays of a render): 0, without its direction
            if (lane == 0) loss[r] = 0.f;
            continue;
        }
        const int nch = (S + 63) >> 6;
        const float d0 = rays_d[r * 3 + 0], d1 = rays_d[r * 3 + 1], d2 = rays_d[r * 3 + 2];
        const float nrm = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
        const float t0 = tv[off];
        float Wc = 0.f, Vc = 0.f, part = 0.f;
        for (int ch = 0; ch < nch; ++ch) {
            const dist_chunk c = distortion_chunk(weights + off, tv + off, dtv + off, ch * 64 + lane, S, t0, nrm, Wc, Vc);
            part += c.w * (2.0f * (c.x * c.Wex - c.Vex) + (c.dl * c.w) / 3.0f);
        }
        const float sum = wave_sum_dpp(part);
        if (lane == 0) loss[r] = sum;
    }
}

__global__ __launch_bounds__(256) void k_distortion_packed_bwd(const float *__restrict__ weights, const float *__restrict__ tv,
                                                               const float *__restrict__ dtv, const float *__restrict__ rays_d,
                                                               const int64_t *__restrict__ ray_off, int64_t R, int64_t n,
                                                               const float *__restrict__ g_loss, float *__restrict__ grad_w)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * 256) >> 6;
    for (int64_t r = wave; r < R; r += nwaves) {
        int64_t off;
        const int S = packed_count(ray_off, r, n, off);
        if (S == 0) continue;                                           // an empty ray has no row of grad_w
        const int nch = (S + 63) >> 6;
        const float d0 = rays_d[r * 3 + 0], d1 = rays_d[r * 3 + 1], d2 = rays_d[r * 3 + 2];
        const float nrm = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
        const float t0 = tv[off], gl = g_loss[r];
        float Wt = 0.f, Vt = 0.f;                                       // sweep one: the totals, by the sums the prefixes are made of
        for (int ch = 0; ch < nch; ++ch) distortion_chunk(weights + off, tv + off, dtv + off, ch * 64 + lane, S, t0, nrm, Wt, Vt);
        float Wc = 0.f, Vc = 0.f;
        for (int ch = 0; ch < nch; ++ch) {
            const int s = ch * 64 + lane;
            const dist_chunk c = distortion_chunk(weights + off, tv + off, dtv + off, s, S, t0, nrm, Wc, Vc);
            const float g = 2.0f * (c.x * (c.Wex - (Wt - c.Win)) - (c.Vex - (Vt - c.Vin))) + (2.0f * (c.w * c.dl)) / 3.0f;
            if (s < S) grad_w[off + s] = g * gl;
        }
    }
}

extern "C" int32_t ctx_distortion_packed_fwd(const float *weights, const float *t, const float *dt, const float *rays_d, const int64_t *ray_off,
                                             int64_t R, int64_t n, float *loss, ctx_stream_t stream)
{
    CTX_REQUIRE(rays_d && ray_off && loss && R > 0, "distortion_packed: bad args");
    CTX_REQUIRE(n >= 0 && n <= INT32_MAX, "distortion_packed: n=%lld outside [0, 2^31)", (long long)n);
    CTX_REQUIRE(n == 0 || (weights && t && dt), "distortion_packed: null list with n=%lld", (long long)n);
    if (n == 0) {
        if (hipMemsetAsync(loss, 0, (size_t)R * sizeof(float), (hipStream_t)stream) != hipSuccess) {
            ctx_set_error("distortion_packed: memset failed");
            return CTX_E_LAUNCH;
        }
        return CTX_OK;
    }
    hipLaunchKernelGGL(k_distortion_packed, dim3(packed_blocks(R)), dim3(256), 0, (hipStream_t)stream, weights, t, dt, rays_d, ray_off, R, n, loss);
    CTX_CHECK_LAUNCH("distortion_packed");
    return CTX_OK;
}

extern "C" int32_t ctx_distortion_packed_bwd(const float *weights, const float *t, const float *dt, const float *rays_d, const int64_t *ray_off,
                                             int64_t R, int64_t n, const float *g_loss, float *grad_w, ctx_stream_t stream)
{
    CTX_REQUIRE(rays_d && ray_off && g_loss && R > 0, "distortion_packed_bwd: bad args");
    CTX_REQUIRE(n >= 0 && n <= INT32_MAX, "distortion_packed_bwd: n=%lld outside [0, 2^31)", (long long)n);
    if (n == 0) return CTX_OK;
    CTX_REQUIRE(weights && t && dt && grad_w, "distortion_packed_bwd: null list with n=%lld", (long long)n);
    hipLaunchKernelGGL(k_distortion_packed_bwd, dim3(packed_blocks(R)), dim3(256), 0, (hipStream_t)stream, weights, t, dt, rays_d, ray_off, R, n,
                       g_loss, grad_w);
    CTX_CHECK_LAUNCH("distortion_packed_bwd");
    return CTX_OK;
}
