// Volume-render compositing, the per-sample and per-chunk pieces (kernels and entry points: composite.hip).  Everything here is written
// over a ray layout, dense or packed, so that a packed ray and a dense ray with the same distances give the same bits.
// One wavefront per ray, lane s of chunk c holds sample 64c + s (ray_wave.h).  Built without FMA contraction.
#pragma once
#include "ray_wave.h"

#define COMPOSITE_BWD_MAX_S 4096      // the backward keeps chunk c's entry transmittance in lane c of one register: 64 chunks

// Per-sample terms of nerf-pytorch raw2outputs after the distance, shared by the forward and the backward so both see the same bits.
// noise is added to the density before the ReLU.
template <bool NOISE>
__device__ __forceinline__ void composite_rest(float qw, float nz, float dist, bool ok, float &e, float &alpha, float &t)
{
    float pre = NOISE ? qw + nz : qw;
    float sigma = pre > 0.f ? pre : 0.f;
    e = __builtin_amdgcn_exp2f(-1.4426950408889634f * sigma * dist);
    alpha = ok ? 1.0f - e : 0.f;
    t = ok ? (1.0f - alpha) + 1e-10f : 1.0f;
}

__device__ __forceinline__ float composite_sigmoid(float x)
{
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}

// The two ray layouts.  Each says where ray r's samples start and how many there are (count), where a sample's depth lies (depth[i]) and
// what its distance to the next one is: dist_in is what that takes from memory, loaded with the sample, dist the arithmetic on it.  The
// distance is split in two so that k_composite_prefetch can issue the load a chunk ahead and do the arithmetic when it reduces the chunk;
// both take the union of what the two layouts need, so each ignores some arguments.
// RAGGED: a ray may be empty or hold more than COMPOSITE_BWD_MAX_S samples (the dense entry points refuse both).
struct dense_rays {                               // R x S samples, ray r at r * S; dist = z[s+1] - z[s], 1e10 on the last sample
    static constexpr bool RAGGED = false;
    const float *__restrict__ depth;
    int S;
    __device__ __forceinline__ int count(int64_t r, int64_t &off) const { off = r * S; return S; }
    // lane 63's next depth: the first depth of the following chunk (the other lanes take theirs from the lane above)
    __device__ __forceinline__ float dist_in(int64_t off, int s, int n, bool ok, int lane) const
    {
        return (lane == 63 && s + 1 < n) ? depth[off + s + 1] : 0.f;
    }
    __device__ __forceinline__ float dist(float zv, float zx, int s, int n, float nrm) const
    {
        const float zn = wave_shl1(zv, zx);
        return ((s + 1 < n) ? (zn - zv) : 1e10f) * nrm;
    }
};
struct packed_rays {                              // ray r holds samples ray_off[r] .. ray_off[r+1] of n; dist = dt * |d|, no 1e10 distance:
    static constexpr bool RAGGED = true;          // the background shows through what the runs leave
    const float *__restrict__ depth, *__restrict__ dt;
    const int64_t *__restrict__ ray_off;
    int64_t n;
    __device__ __forceinline__ int count(int64_t r, int64_t &off) const { return packed_count(ray_off, r, n, off); }
    __device__ __forceinline__ float dist_in(int64_t off, int s, int, bool ok, int) const { return ok ? dt[off + s] : 0.f; }
    __device__ __forceinline__ float dist(float, float dtv, int, int, float nrm) const { return dtv * nrm; }
};

// The sample's weight under its chunk's entry transmittance Tc (call it in every lane: it scans across the wave); Tc <- the next chunk's.
template <bool NOISE>
__device__ __forceinline__ float composite_weight(float qw, float nz, float dist, bool ok, float &Tc)
{
    float e, alpha, t;
    composite_rest<NOISE>(qw, nz, dist, ok, e, alpha, t);
    const float inc = wave_scan<scan_prod>(t);
    const float w = alpha * (Tc * wave_shr1(inc, 1.0f));
    Tc = Tc * wave_lane(inc, 63);
    return w;
}

// Forward, one chunk of a ray: the weight (stored when asked for) and the lane's share of the five sums.
struct composite_sums {
    float Tc = 1.0f, c0 = 0.f, c1 = 0.f, c2 = 0.f, dep = 0.f, a = 0.f;
};
template <bool NOISE>
__device__ __forceinline__ void composite_chunk(float4 q, float zv, float nz, float dist, bool ok, float *__restrict__ weights, int64_t i,
                                                composite_sums &m)
{
    const float w = composite_weight<NOISE>(q.w, nz, dist, ok, m.Tc);
    if (weights && ok) weights[i] = w;
    m.c0 += w * composite_sigmoid(q.x);
    m.c1 += w * composite_sigmoid(q.y);
    m.c2 += w * composite_sigmoid(q.z);
    m.dep += w * zv;
    m.a += w;
}

// The ray's outputs from the lanes' partial sums (wave-uniform call): the wave sums, the white background, disp = 1 / max(depth / acc, 1e-10)
// with the 0 / 0 of an empty ray passed through.
__device__ __forceinline__ void composite_finish(int lane, int64_t r, int white, float c0, float c1, float c2, float dep, float a,
                                                 float *__restrict__ rgb, float *__restrict__ disp, float *__restrict__ acc,
                                                 float *__restrict__ depth)
{
    float s0 = wave_sum_dpp(c0), s1 = wave_sum_dpp(c1), s2 = wave_sum_dpp(c2), sd = wave_sum_dpp(dep), sa = wave_sum_dpp(a);
    if (lane == 0) {
        if (white) { s0 += 1.0f - sa; s1 += 1.0f - sa; s2 += 1.0f - sa; }
        rgb[r * 3 + 0] = s0; rgb[r * 3 + 1] = s1; rgb[r * 3 + 2] = s2;
        depth[r] = sd; acc[r] = sa;
        float qd = sd / sa;
        float dv = 1.0f / (qd > 1e-10f ? qd : 1e-10f);
        disp[r] = (qd != qd) ? qd : dv;
    }
}

// Backward, per ray: the upstream gradients (each nullable = zero) folded into dL/drgb (g0, g1, g2) and the coefficients of depth (gd)
// and acc (ga) in dL/dw_s; sd, sa: the ray's recomputed depth and acc.
__device__ __forceinline__ void composite_bwd_upstream(int64_t r, int white, float sd, float sa, const float *__restrict__ g_rgb,
                                                       const float *__restrict__ g_disp, const float *__restrict__ g_acc,
                                                       const float *__restrict__ g_depth, float &g0, float &g1, float &g2, float &gd, float &ga)
{
    g0 = g_rgb ? g_rgb[r * 3 + 0] : 0.f; g1 = g_rgb ? g_rgb[r * 3 + 1] : 0.f; g2 = g_rgb ? g_rgb[r * 3 + 2] : 0.f;
    const float qd = sd / sa;
    const bool hasq = qd > 1e-10f;                                  // false on the acc == 0 ray (0 / 0): both gq terms drop
    const float gq = (hasq && g_disp) ? -g_disp[r] / (qd * qd) : 0.f;
    gd = (g_depth ? g_depth[r] : 0.f) + (hasq ? gq / sa : 0.f);
    ga = ((g_acc ? g_acc[r] : 0.f) - (hasq ? gq * sd / (sa * sa) : 0.f)) - (white ? (g0 + g1) + g2 : 0.f);
}

// Backward, per sample of the chunk being swept back to front (call it in every lane: it scans across the wave): the closed form of
// DESIGN section 4d.  q: the sample's raw, pre = q.w (+ noise), zv: its depth, gw: its upstream weight gradient, T: its transmittance;
// carry: the sum of G_k w_k over the chunks behind this one, updated.  -> the sample's row of grad_raw.
__device__ __forceinline__ float4 composite_bwd_sample(float4 q, float pre, float zv, float gw, bool ok, int lane, float dist, float e, float alpha,
                                                       float t, float T, float g0, float g1, float g2, float gd, float ga, float &carry)
{
    const float w = alpha * T;
    const float c0 = composite_sigmoid(q.x), c1 = composite_sigmoid(q.y), c2 = composite_sigmoid(q.z);
    const float G = ((((g0 * c0 + g1 * c1) + g2 * c2) + gd * zv) + ga) + gw;          // dL/dw_s
    const float suf = wave_suffix_sum(ok ? G * w : 0.f, lane);          // of G_k w_k over the lanes at and behind this one
    const float X = carry + wave_shl1(suf, 0.f);                         // exclusive: the inclusive sum of the next lane
    carry = carry + wave_lane(suf, 0);
    // dL/dalpha_s * dist_s * e_s with e_s folded in before the division: e / t <= 1 and dist * e stays finite at dist = 1e10
    const float da = (G * T) * (dist * e) - (X * (e * __builtin_amdgcn_rcpf(t))) * dist;
    float4 o;
    o.x = (w * g0) * (c0 * (1.0f - c0));
    o.y = (w * g1) * (c1 * (1.0f - c1));
    o.z = (w * g2) * (c2 * (1.0f - c2));
    o.w = pre > 0.f ? da : 0.f;                // the ReLU mask is a select: dist is 1e10 on the last sample
    return o;
}
