// Volume-render compositing (nerf-pytorch raw2outputs) and its backward, on dense R x S samples and on the ragged per-ray lists of the
// march (DESIGN sections 4d, 4g).  One kernel body over the two ray layouts of composite.h: one wavefront per ray, lane s of chunk c holds
// sample 64c + s; the transmittance is an exclusive prefix product across the lanes, colour / depth / acc are wave sums.
// Built with -ffp-contract=off.  No atomics; every output element has one writer and one fixed summation order.
#include "composite.h"

template <class Layout, bool NOISE>
__global__ __launch_bounds__(256) void k_composite(const float4 *__restrict__ raw, const Layout L, const float *__restrict__ rays_d,
                                                   const float *__restrict__ noise, int64_t R, int white, float *__restrict__ rgb,
                                                   float *__restrict__ disp, float *__restrict__ acc, float *__restrict__ weights,
                                                   float *__restrict__ depth)
{
    const ray_wave rw = ray_wave_here();
    for (int64_t r = rw.first; r < R; r += rw.stride) {
        int64_t off;
        const int S = L.count(r, off);
        const int nch = (S + 63) >> 6;
        const float nrm = ray_norm(rays_d, r);
        composite_sums m;
        for (int ch = 0; ch < nch; ++ch) {
            const int s = ch * 64 + rw.lane;
            const bool ok = s < S;
            const float4 q = ok ? raw[off + s] : make_float4(0.f, 0.f, 0.f, 0.f);
            const float zv = ok ? L.depth[off + s] : 0.f;
            const float din = L.dist_in(off, s, S, ok, rw.lane);
            const float nz = (NOISE && ok) ? noise[off + s] : 0.f;
            composite_chunk<NOISE>(q, zv, nz, L.dist(zv, din, s, S, nrm), ok, weights, off + s, m);
        }
        composite_finish(rw.lane, r, white, m.c0, m.c1, m.c2, m.dep, m.a, rgb, disp, acc, depth);          // S = 0: acc = depth = 0, disp = 0 / 0
    }
}

// The dense forward as a software pipeline over the wave's flattened (ray, chunk) sequence: the next chunk's (or next ray's first) loads
// are issued before the current chunk is reduced, so HBM latency overlaps the shuffle chain.
template <bool NOISE>
__global__ __launch_bounds__(256) void k_composite_prefetch(const float4 *__restrict__ raw, const dense_rays L, const float *__restrict__ rays_d,
                                                            const float *__restrict__ noise, int64_t R, int white, float *__restrict__ rgb,
                                                            float *__restrict__ disp, float *__restrict__ acc, float *__restrict__ weights,
                                                            float *__restrict__ depth)
{
    const ray_wave rw = ray_wave_here();
    const int S = L.S, nch = (S + 63) >> 6;
    int64_t r = rw.first;
    int ch = 0;
    float4 q_n = make_float4(0.f, 0.f, 0.f, 0.f);
    float z_n = 0.f, zx_n = 0.f, nz_n = 0.f;
    auto fetch = [&](int64_t rr, int cc) {
        const int s = cc * 64 + rw.lane;
        const bool ok = rr < R && s < S;
        q_n = ok ? raw[rr * S + s] : make_float4(0.f, 0.f, 0.f, 0.f);
        z_n = ok ? L.depth[rr * S + s] : 0.f;
        zx_n = L.dist_in(rr * S, s, rr < R ? S : 0, ok, rw.lane);
        if (NOISE) nz_n = ok ? noise[rr * S + s] : 0.f;
    };
    if (r < R) fetch(r, 0);
    composite_sums m;
    float nrm = 0.f;
    while (r < R) {
        const float4 q = q_n;
        const float zv = z_n, zx = zx_n, nz = nz_n;
        const int s = ch * 64 + rw.lane;
        if (ch == 0) {
            nrm = ray_norm(rays_d, r);
            m = composite_sums();
        }
        int64_t rn = r;
        int cn = ch + 1;
        if (cn == nch) { cn = 0; rn = r + rw.stride; }
        fetch(rn, cn);
        composite_chunk<NOISE>(q, zv, nz, L.dist(zv, zx, s, S, nrm), s < S, weights, r * S + s, m);
        if (ch + 1 == nch) composite_finish(rw.lane, r, white, m.c0, m.c1, m.c2, m.dep, m.a, rgb, disp, acc, depth);
        r = rn; ch = cn;
    }
}

// Backward with respect to raw (closed form: DESIGN section 4d).  Two sweeps over the ray's 64-sample chunks.  Sweep 1 (front to back)
// re-runs the forward's alpha / transmittance sequence for acc and depth and leaves chunk c's entry transmittance in lane c of one
// register, which bounds a ray at 64 chunks.  Sweep 2 (back to front) recomputes the chunk, carries the suffix sum of G_k w_k over the
// chunks behind it and adds a true in-wave suffix scan, so a sample deep behind an opaque one keeps its relative accuracy.  Every row of
// grad_raw that belongs to a ray is written.
template <class Layout, bool NOISE>
__global__ __launch_bounds__(256) void k_composite_bwd(const float4 *__restrict__ raw, const Layout L, const float *__restrict__ rays_d,
                                                       const float *__restrict__ noise, int64_t R, int white, const float *__restrict__ g_rgb,
                                                       const float *__restrict__ g_disp, const float *__restrict__ g_acc,
                                                       const float *__restrict__ g_weights, const float *__restrict__ g_depth,
                                                       float4 *__restrict__ grad_raw)
{
    const ray_wave rw = ray_wave_here();
    const int lane = rw.lane;
    for (int64_t r = rw.first; r < R; r += rw.stride) {
        int64_t off;
        const int S = L.count(r, off);
        if (Layout::RAGGED && S == 0) continue;                         // an empty ray has no row of grad_raw
        if (Layout::RAGGED && S > COMPOSITE_BWD_MAX_S) {                // more chunks than the table holds: poisoned, not silently wrong
            const float bad = __builtin_nanf("");
            for (int s = lane; s < S; s += 64) grad_raw[off + s] = make_float4(bad, bad, bad, bad);
            continue;
        }
        const int nch = (S + 63) >> 6;
        const float nrm = ray_norm(rays_d, r);
        const float4 *rawr = raw + off;
        const float *zr = L.depth + off, *nr = NOISE ? noise + off : nullptr;
        float Tc = 1.0f, tcv = 1.0f, dep = 0.f, a = 0.f;
        for (int ch = 0; ch < nch; ++ch) {
            const int s = ch * 64 + lane;
            const bool ok = s < S;
            const float qw = ok ? rawr[s].w : 0.f;
            const float zv = ok ? zr[s] : 0.f;
            const float din = L.dist_in(off, s, S, ok, lane);
            const float nz = (NOISE && ok) ? nr[s] : 0.f;
            if (lane == ch) tcv = Tc;
            const float w = composite_weight<NOISE>(qw, nz, L.dist(zv, din, s, S, nrm), ok, Tc);
            dep += w * zv;
            a += w;
        }
        const float sd = wave_sum_dpp(dep), sa = wave_sum_dpp(a);
        float g0, g1, g2, gd, ga;
        composite_bwd_upstream(r, white, sd, sa, g_rgb, g_disp, g_acc, g_depth, g0, g1, g2, gd, ga);
        float carry = 0.f;                                              // sum of G_k w_k over the chunks behind this one
        for (int ch = nch - 1; ch >= 0; --ch) {
            const int s = ch * 64 + lane;
            const bool ok = s < S;
            const float4 q = ok ? rawr[s] : make_float4(0.f, 0.f, 0.f, 0.f);
            const float zv = ok ? zr[s] : 0.f;
            const float din = L.dist_in(off, s, S, ok, lane);
            const float nz = (NOISE && ok) ? nr[s] : 0.f;
            const float gw = (g_weights && ok) ? g_weights[off + s] : 0.f;
            const float dist = L.dist(zv, din, s, S, nrm);
            float e, alpha, t;
            composite_rest<NOISE>(q.w, nz, dist, ok, e, alpha, t);
            const float T = wave_lane(tcv, ch) * wave_shr1(wave_scan<scan_prod>(t), 1.0f);
            const float pre = NOISE ? q.w + nz : q.w;
            const float4 o = composite_bwd_sample(q, pre, zv, gw, ok, lane, dist, e, alpha, t, T, g0, g1, g2, gd, ga, carry);
            if (ok) grad_raw[off + s] = o;
        }
    }
}

// CTX_COMPOSITE_BLOCKS caps the grid of the dense forward and backward (default: one ray per wave up to 1 M rays: 136.8 us against 142.6 at
// 32768 blocks, 512^2 x 128)
static unsigned composite_blocks(int64_t R)
{
    static const int cap = ctx_env_int("CTX_COMPOSITE_BLOCKS", 262144);
    return capped_blocks(R, 4, cap);
}

extern "C" int32_t ctx_raymarch_composite_fwd_noise(const float *raw, const float *z_vals, const float *rays_d, const float *noise,
                                                    int64_t R, int32_t S, int32_t white_bkgd, float *rgb, float *disp, float *acc,
                                                    float *weights, float *depth, ctx_stream_t stream)
{
    CTX_REQUIRE(raw && z_vals && rays_d && rgb && disp && acc && depth && R > 0 && S > 0, "raymarch: bad args");
    const dense_rays L = {z_vals, (int)S};
    CTX_BOOL_GO(noise != nullptr, NZ, hipLaunchKernelGGL(k_composite_prefetch<NZ>, dim3(composite_blocks(R)), dim3(256), 0, (hipStream_t)stream,
                                                         (const float4 *)raw, L, rays_d, noise, R, (int)white_bkgd, rgb, disp, acc, weights, depth));
    CTX_CHECK_LAUNCH("raymarch_composite");
    return CTX_OK;
}

extern "C" int32_t ctx_raymarch_composite_fwd(const float *raw, const float *z_vals, const float *rays_d, int64_t R,
                                              int32_t S, int32_t white_bkgd, float *rgb, float *disp, float *acc,
                                              float *weights, float *depth, ctx_stream_t stream)
{
    return ctx_raymarch_composite_fwd_noise(raw, z_vals, rays_d, nullptr, R, S, white_bkgd, rgb, disp, acc, weights, depth, stream);
}

extern "C" int32_t ctx_raymarch_composite_bwd(const float *raw, const float *z_vals, const float *rays_d, const float *noise,
                                              int64_t R, int32_t S, int32_t white_bkgd, const float *g_rgb, const float *g_disp,
                                              const float *g_acc, const float *g_weights, const float *g_depth, float *grad_raw,
                                              ctx_stream_t stream)
{
    CTX_REQUIRE(raw && z_vals && rays_d && grad_raw && R > 0 && S > 0, "raymarch_bwd: bad args");
    CTX_REQUIRE(S <= COMPOSITE_BWD_MAX_S, "raymarch_bwd: S exceeds the 4096 samples per ray the backward supports");
    const dense_rays L = {z_vals, (int)S};
    CTX_BOOL_GO(noise != nullptr, NZ, hipLaunchKernelGGL((k_composite_bwd<dense_rays, NZ>), dim3(composite_blocks(R)), dim3(256), 0,
                                                         (hipStream_t)stream, (const float4 *)raw, L, rays_d, noise, R, (int)white_bkgd, g_rgb,
                                                         g_disp, g_acc, g_weights, g_depth, (float4 *)grad_raw));
    CTX_CHECK_LAUNCH("raymarch_composite_bwd");
    return CTX_OK;
}

extern "C" int32_t ctx_raymarch_packed_fwd(const float *raw, const float *t, const float *dt, const float *rays_d, const float *noise,
                                           const int64_t *ray_off, int64_t R, int64_t n, int32_t white_bkgd, float *rgb, float *disp, float *acc,
                                           float *weights, float *depth, ctx_stream_t stream)
{
    CTX_REQUIRE(rays_d && ray_off && rgb && disp && acc && depth && R > 0, "raymarch_packed: bad args");
    CTX_REQUIRE(n >= 0 && n <= INT32_MAX, "raymarch_packed: n=%lld outside [0, 2^31)", (long long)n);
    CTX_REQUIRE(n == 0 || (raw && t && dt), "raymarch_packed: null list with n=%lld", (long long)n);
    CTX_REQUIRE(((uintptr_t)raw % 16) == 0, "raymarch_packed: raw must be 16-byte aligned");
    const packed_rays L = {t, dt, ray_off, n};
    CTX_BOOL_GO(noise != nullptr, NZ, hipLaunchKernelGGL((k_composite<packed_rays, NZ>), dim3(ray_blocks(R)), dim3(256), 0, (hipStream_t)stream,
                                                         (const float4 *)raw, L, rays_d, noise, R, (int)white_bkgd, rgb, disp, acc, weights, depth));
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
    const packed_rays L = {t, dt, ray_off, n};
    CTX_BOOL_GO(noise != nullptr, NZ, hipLaunchKernelGGL((k_composite_bwd<packed_rays, NZ>), dim3(ray_blocks(R)), dim3(256), 0,
                                                         (hipStream_t)stream, (const float4 *)raw, L, rays_d, noise, R, (int)white_bkgd, g_rgb,
                                                         g_disp, g_acc, g_weights, g_depth, (float4 *)grad_raw));
    CTX_CHECK_LAUNCH("raymarch_packed_bwd");
    return CTX_OK;
}
