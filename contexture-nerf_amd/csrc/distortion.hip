// mip-NeRF 360's distortion loss of the compositing weights on the marched sample lists, forward and backward, by prefix sums (DESIGN
// section 4h; definition: tests/distortion_rule.py).
// Per ray, with x_i = (t_i - t_0) * |d| and delta_i = dt_i * |d| in world lengths and t ascending (a precondition, not checked):
//   L = sum_i w_i * (2 * (x_i * W_<i - V_<i) + delta_i * w_i / 3),  W_<i = sum_{j<i} w_j,  V_<i = sum_{j<i} w_j x_j
//   dL/dw_i = 2 * (x_i * (W_<i - W_>i) - (V_<i - V_>i)) + 2 * w_i * delta_i / 3,  W_>i = W - W_<=i,  V_>i = V - V_<=i
// One wavefront per ray, lane s of chunk c holds sample ray_off[r] + 64c + s (ray_wave.h).  The chunks are chained
// by two carried scalars (W, V), not by a chunk table, so there is no 4096-sample limit: a ray may hold any count up to 2^31 - 64.
// Built with -ffp-contract=off: the numpy restatement gives the same bits.  No atomics; every output element has one writer.
#include "ray_wave.h"

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
    const float winc = wave_scan<scan_sum>(c.w), vinc = wave_scan<scan_sum>(c.w * c.x);
    c.Wex = Wc + wave_shr1(winc, 0.f); c.Win = Wc + winc;
    c.Vex = Vc + wave_shr1(vinc, 0.f); c.Vin = Vc + vinc;
    Wc = Wc + wave_lane(winc, 63);
    Vc = Vc + wave_lane(vinc, 63);
    return c;
}

__global__ __launch_bounds__(256) void k_distortion_packed(const float *__restrict__ weights, const float *__restrict__ tv,
                                                           const float *__restrict__ dtv, const float *__restrict__ rays_d,
                                                           const int64_t *__restrict__ ray_off, int64_t R, int64_t n, float *__restrict__ loss)
{
    const ray_wave rw = ray_wave_here();
    const int lane = rw.lane;
    for (int64_t r = rw.first; r < R; r += rw.stride) {
        int64_t off;
        const int S = packed_count(ray_off, r, n, off);
        if (S == 0) {                                                   // an empty ray (most rays of a render): 0, without its direction
            if (lane == 0) loss[r] = 0.f;
            continue;
        }
        const int nch = (S + 63) >> 6;
        const float nrm = ray_norm(rays_d, r);
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
    const ray_wave rw = ray_wave_here();
    const int lane = rw.lane;
    for (int64_t r = rw.first; r < R; r += rw.stride) {
        int64_t off;
        const int S = packed_count(ray_off, r, n, off);
        if (S == 0) continue;                                           // an empty ray has no row of grad_w
        const int nch = (S + 63) >> 6;
        const float nrm = ray_norm(rays_d, r);
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
    hipLaunchKernelGGL(k_distortion_packed, dim3(ray_blocks(R)), dim3(256), 0, (hipStream_t)stream, weights, t, dt, rays_d, ray_off, R, n, loss);
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
    hipLaunchKernelGGL(k_distortion_packed_bwd, dim3(ray_blocks(R)), dim3(256), 0, (hipStream_t)stream, weights, t, dt, rays_d, ray_off, R, n,
                       g_loss, grad_w);
    CTX_CHECK_LAUNCH("distortion_packed_bwd");
    return CTX_OK;
}
