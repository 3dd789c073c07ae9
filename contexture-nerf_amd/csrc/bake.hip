// Baking a 3-D field into the mesh's UV atlas: the two ends of the chain
//   texel list -> ctx_texel_rays -> occupancy.march + field + raw2outputs_packed (the ray path as it is) -> ctx_bake_resolve -> atlas sums.
// Both rules are written out in include/ctx_nerf.h; tests/bake_rule.py restates them in numpy and the kernels are array_equal to it
// (this file is built without contraction: every float operation rounds on its own, in the order written).
//
// k_texel_rays: one thread per output ROW (list entry j, sub-sample k): the loads of an entry hang on each other (texel -> face ->
// vertices), so each level is issued as a whole with clamped indices and the s*s lanes of an entry, neighbours in a wave, read the same
// addresses.  The job is bound by its stores, 25 bytes per row: a block of 256 rows owns 3072 contiguous bytes of rays_o and of rays_d
// and 256 of valid, stages them in LDS (stride-3 words: no bank conflict) and writes them as whole dwordx4 / dword vectors; only the
// last block of a call has a scalar tail.  One writer per element, no atomics.
// k_bake_resolve: one thread per list entry: s*s sub-samples summed left to right in registers, one plain read-modify-write of the four
// int64 sums of its texel (the list holds distinct texels).
#include "common.h"

#define BK_BLK 256

template <int S>
__global__ __launch_bounds__(BK_BLK) void k_texel_rays(const int64_t *__restrict__ texel_face, const float *__restrict__ texel_bary,
                                                       const float *__restrict__ face_uv, const float *__restrict__ vertices,
                                                       const int64_t *__restrict__ faces, const int32_t *__restrict__ idx, int64_t R, int T, int F,
                                                       int V, float h, float *__restrict__ rays_o, float *__restrict__ rays_d,
                                                       unsigned char *__restrict__ valid)
{
    constexpr int SS = S * S;
    __shared__ __attribute__((aligned(16))) float so[BK_BLK * 3];
    __shared__ __attribute__((aligned(16))) float sd[BK_BLK * 3];
    __shared__ __attribute__((aligned(16))) unsigned char sv[BK_BLK];
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * BK_BLK, r = base + t;
    float o[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, 0.0f};
    bool ok = false;
    if (r < R) {
        const int64_t j = r / SS;
        const int k = (int)(r - j * SS), a = k % S, b = k / S;
        // level 1: the texel
        int64_t p = idx[j];
        ok = p >= 0 && p < (int64_t)T * T;
        p = ok ? p : 0;
        // level 2: its face and barycentrics
        int64_t f = texel_face[p];
        const float s0 = texel_bary[p * 3 + 0], s1 = texel_bary[p * 3 + 1], s2 = texel_bary[p * 3 + 2];
        ok = ok && f >= 0 && f < F;
        f = ok ? f : 0;
        // level 3: the face's vertex ids and UV corners
        int64_t i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
        float2 q0 = make_float2(0.0f, 0.0f), q1 = q0, q2 = q0;
        if (S > 1) {
            const float2 *q = (const float2 *)(face_uv + f * 6);
            q0 = q[0]; q1 = q[1]; q2 = q[2];
        }
        ok = ok && i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V;
        i0 = ok ? i0 : 0; i1 = ok ? i1 : 0; i2 = ok ? i2 : 0;
        // level 4: the vertices
        float v0[3], v1[3], v2[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            v0[c] = vertices[i0 * 3 + c];
            v1[c] = vertices[i1 * 3 + c];
            v2[c] = vertices[i2 * 3 + c];
        }
        const float e1x = v1[0] - v0[0], e1y = v1[1] - v0[1], e1z = v1[2] - v0[2];
        const float e2x = v2[0] - v0[0], e2y = v2[1] - v0[1], e2z = v2[2] - v0[2];
        const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
        const float l2 = (cx * cx + cy * cy) + cz * cz;
        ok = ok && isfinite(l2) && l2 > 0.0f;
        const float ln = sqrtf(l2);
        const float n[3] = {cx / ln, cy / ln, cz / ln};
        float b0 = s0, b1 = s1, b2 = s2;
        if (S > 1) {
            const float fT = (float)T;
            const float x1 = (q1.x - q0.x) * fT, x2 = (q2.x - q0.x) * fT;
            const float y1 = (q0.y - q1.y) * fT, y2 = (q0.y - q2.y) * fT;          // row = (1 - v)*T - 1/2
            const float D = x1 * y2 - x2 * y1;
            if (isfinite(D) && D != 0.0f) {
                const float g1x = y2 / D, g1y = -x2 / D, g2x = -y1 / D, g2y = x1 / D;
                const float dx = ((float)a + 0.5f) / (float)S - 0.5f, dy = ((float)b + 0.5f) / (float)S - 0.5f;
                b1 = s1 + (dx * g1x + dy * g1y);
                b2 = s2 + (dx * g2x + dy * g2y);
                b0 = (1.0f - b1) - b2;
            }
        }
        if (ok) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float x = (b0 * v0[c] + b1 * v1[c]) + b2 * v2[c];
                o[c] = x + h * n[c];
                d[c] = -n[c];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        so[t * 3 + c] = o[c];
        sd[t * 3 + c] = d[c];
    }
    sv[t] = ok ? 1 : 0;
    __syncthreads();
    const int64_t left = R - base;
    const int rows = left < BK_BLK ? (int)left : BK_BLK;          // >= 1: the grid has no empty block
    const int words = rows * 3;
    float *go = rays_o + base * 3, *gd = rays_d + base * 3;       // 3072 bytes per block: 16-byte aligned with the base
    if (t * 4 + 4 <= words) {
        ((float4 *)go)[t] = ((const float4 *)so)[t];
        ((float4 *)gd)[t] = ((const float4 *)sd)[t];
    } else {
        for (int w = t * 4; w < words; ++w) {
            go[w] = so[w];
            gd[w] = sd[w];
        }
    }
    unsigned char *gv = valid + base;
    if (t * 4 + 4 <= rows) {
        ((uint32_t *)gv)[t] = ((const uint32_t *)sv)[t];
    } else {
        for (int w = t * 4; w < rows; ++w) gv[w] = sv[w];
    }
}

__global__ __launch_bounds__(BK_BLK) void k_bake_resolve(const float *__restrict__ rgb, const float *__restrict__ alpha,
                                                         const unsigned char *__restrict__ valid, const int32_t *__restrict__ idx, int64_t n, int ss,
                                                         int64_t TT, float min_alpha, int frac, long long *__restrict__ acc)
{
    const int64_t j = (int64_t)blockIdx.x * BK_BLK + threadIdx.x;
    if (j >= n) return;
    const int64_t p = idx[j];
    if (p < 0 || p >= TT) return;
    float S0 = 0.0f, S1 = 0.0f, S2 = 0.0f, Sa = 0.0f;
    int m = 0;
    for (int k = 0; k < ss; ++k) {
        const int64_t r = j * ss + k;
        const float c0 = rgb[r * 3 + 0], c1 = rgb[r * 3 + 1], c2 = rgb[r * 3 + 2], al = alpha[r];
        if (valid[r] && isfinite(al) && isfinite(c0) && isfinite(c1) && isfinite(c2)) {
            S0 = S0 + c0; S1 = S1 + c1; S2 = S2 + c2; Sa = Sa + al;
            ++m;
        }
    }
    if (m == 0) return;
    const float fm = (float)m;
    const float M0 = S0 / fm, M1 = S1 / fm, M2 = S2 / fm, Ma = Sa / fm;
    if (!(Ma >= min_alpha)) return;
    acc[0 * TT + p] += __float2ll_rn(ldexpf(M0, frac));
    acc[1 * TT + p] += __float2ll_rn(ldexpf(M1, frac));
    acc[2 * TT + p] += __float2ll_rn(ldexpf(M2, frac));
    acc[3 * TT + p] += __float2ll_rn(ldexpf(Ma, frac));
}

#define BK_REQUIRE_LIST(who)                                                                                                         \
    CTX_REQUIRE(s >= 1 && s <= 4, who ": supersample s=%d outside [1, 4]", s);                                                       \
    CTX_REQUIRE(T >= 1 && T <= 46340, who ": T=%d outside [1, 46340] (int32 texel indices)", T);                                     \
    CTX_REQUIRE(n >= 0 && n <= INT32_MAX && n * s * s <= INT32_MAX, who ": n=%lld entries x %d sub-samples: want 0 <= n*s*s < 2^31; split the list",   \
                (long long)n, s * s)

extern "C" int32_t ctx_texel_rays(const int64_t *texel_face, const float *texel_bary, const float *face_uv, const float *vertices,
                                  const int64_t *faces, const int32_t *idx, int64_t n, int32_t T, int32_t F, int32_t V, int32_t s, float h,
                                  float *rays_o, float *rays_d, uint8_t *valid, ctx_stream_t stream)
{
    CTX_REQUIRE(texel_face && texel_bary && face_uv && vertices && faces && idx && rays_o && rays_d && valid, "texel_rays: null pointer");
    BK_REQUIRE_LIST("texel_rays");
    CTX_REQUIRE(F >= 1 && V >= 1, "texel_rays: F=%d V=%d must be positive", F, V);
    CTX_REQUIRE(h > 0.0f && h <= 3.402823466e38f, "texel_rays: shell h=%g: want a finite world length > 0", (double)h);
    CTX_REQUIRE(((uintptr_t)rays_o & 15) == 0 && ((uintptr_t)rays_d & 15) == 0 && ((uintptr_t)valid & 3) == 0 && ((uintptr_t)face_uv & 7) == 0,
                "texel_rays: rays_o / rays_d want 16-byte, valid 4-byte and face_uv 8-byte alignment (whole-vector stores and loads)");
    const int64_t R = n * s * s;
    if (R == 0) return CTX_OK;
    const dim3 grid((unsigned)cdiv64(R, BK_BLK));
#define BK_GO(S_) hipLaunchKernelGGL(k_texel_rays<S_>, grid, dim3(BK_BLK), 0, (hipStream_t)stream, texel_face, texel_bary, face_uv, vertices, faces, idx, \
                                     R, T, F, V, h, rays_o, rays_d, valid)
    switch (s) {
    case 1: BK_GO(1); break;
    case 2: BK_GO(2); break;
    case 3: BK_GO(3); break;
    default: BK_GO(4); break;
    }
#undef BK_GO
    CTX_CHECK_LAUNCH("texel_rays");
    return CTX_OK;
}

extern "C" int32_t ctx_bake_resolve(const float *rgb, const float *alpha, const uint8_t *valid, const int32_t *idx, int64_t n, int32_t s, int32_t T,
                                    float min_alpha, int32_t frac_bits, int64_t *acc, ctx_stream_t stream)
{
    CTX_REQUIRE(rgb && alpha && valid && idx && acc, "bake_resolve: null pointer");
    BK_REQUIRE_LIST("bake_resolve");
    CTX_REQUIRE(frac_bits >= -64 && frac_bits <= 62, "bake_resolve: frac_bits=%d outside [-64, 62]", frac_bits);
    if (n == 0) return CTX_OK;
    hipLaunchKernelGGL(k_bake_resolve, dim3((unsigned)cdiv64(n, BK_BLK)), dim3(BK_BLK), 0, (hipStream_t)stream, rgb, alpha, valid, idx, n, s * s,
                       (int64_t)T * T, min_alpha, frac_bits, (long long *)acc);
    CTX_CHECK_LAUNCH("bake_resolve");
    return CTX_OK;
}
