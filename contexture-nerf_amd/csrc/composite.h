// Volume-render compositing: everything that follows a sample's distance, shared by the dense kernels (geometry.hip: k_composite,
// k_composite_bwd) and the packed ones (march.hip), so that a packed ray and a dense ray with the same distances give the same bits.
// One wavefront per ray, lane s of chunk c holds sample 64c + s.  Both files are built without FMA contraction.
#pragma once
#include "common.h"

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

// inclusive prefix product over the 64 lanes on the DPP path (no LDS crossbar): Hillis-Steele inside the 16-lane
// rows (row_shr 1, 2, 4, 8; lanes without a source multiply by `old` = 1), then row_bcast 15 / 31 across rows;
// exc = inclusive shifted right by one lane (wave_shr:1; lane 0 keeps `old` = 1)
__device__ __forceinline__ void composite_prefix(float t, float &inc, float &exc)
{
    inc = t;
    const int one = 0x3f800000;
#define CTX_SCAN_STEP(ctrl, rmask) inc = inc * __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(one, __builtin_bit_cast(int, inc), ctrl, rmask, 0xf, false))
    CTX_SCAN_STEP(0x111, 0xf);
    CTX_SCAN_STEP(0x112, 0xf);
    CTX_SCAN_STEP(0x114, 0xf);
    CTX_SCAN_STEP(0x118, 0xf);
    CTX_SCAN_STEP(0x142, 0xa);                    // row_bcast:15 into rows 1 and 3
    CTX_SCAN_STEP(0x143, 0xc);                    // row_bcast:31 into rows 2 and 3
#undef CTX_SCAN_STEP
    exc = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(one, __builtin_bit_cast(int, inc), 0x138, 0xf, 0xf, false));
}

// inclusive prefix sum over the 64 lanes: the same DPP controls with `old` = 0, so lanes without a source and rows outside the mask add 0;
// exc = inclusive shifted right by one lane (lane 0 keeps 0).  Lane i adds its 16-lane row left to right in a 4-level tree, then the rows.
__device__ __forceinline__ void composite_prefix_sum(float v, float &inc, float &exc)
{
    inc = v;
#define CTX_SCAN_STEP(ctrl, rmask) inc = inc + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, inc), ctrl, rmask, 0xf, false))
    CTX_SCAN_STEP(0x111, 0xf);
    CTX_SCAN_STEP(0x112, 0xf);
    CTX_SCAN_STEP(0x114, 0xf);
    CTX_SCAN_STEP(0x118, 0xf);
    CTX_SCAN_STEP(0x142, 0xa);                    // row_bcast:15 into rows 1 and 3
    CTX_SCAN_STEP(0x143, 0xc);                    // row_bcast:31 into rows 2 and 3
#undef CTX_SCAN_STEP
    exc = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, inc), 0x138, 0xf, 0xf, false));
}

__device__ __forceinline__ float composite_sigmoid(float x)
{
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
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
    // inclusive suffix sum of G_k w_k over the lanes at and behind this one
    float suf = ok ? G * w : 0.f;
#define CTX_SUFFIX_STEP(ctrl) suf = suf + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, suf), ctrl, 0xf, 0xf, false))
    CTX_SUFFIX_STEP(0x101);                   // row_shl 1, 2, 4, 8: lanes without a source add `old` = 0
    CTX_SUFFIX_STEP(0x102);
    CTX_SUFFIX_STEP(0x104);
    CTX_SUFFIX_STEP(0x108);
#undef CTX_SUFFIX_STEP
    const int si = __builtin_bit_cast(int, suf);
    const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(si, 16)), r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(si, 32));
    const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(si, 48));
    const int row = lane >> 4;
    suf = suf + (row == 0 ? (r1 + (r2 + r3)) : row == 1 ? (r2 + r3) : row == 2 ? r3 : 0.f);
    // exclusive: the inclusive sum of the next lane (wave_shl:1; lane 63 keeps `old` = 0)
    const float X = carry + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, suf), 0x130, 0xf, 0xf, false));
    carry = carry + __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, suf), 0));
    // dL/dalpha_s * dist_s * e_s with e_s folded in before the division: e / t <= 1 and dist * e stays finite at dist = 1e10
    const float da = (G * T) * (dist * e) - (X * (e * __builtin_amdgcn_rcpf(t))) * dist;
    float4 o;
    o.x = (w * g0) * (c0 * (1.0f - c0));
    o.y = (w * g1) * (c1 * (1.0f - c1));
    o.z = (w * g2) * (c2 * (1.0f - c2));
    o.w = pre > 0.f ? da : 0.f;                // the ReLU mask is a select: dist is 1e10 on the last sample
    return o;
}
