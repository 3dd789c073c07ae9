// The glue of the view-dependent field (the rule: tests/sh_rule.py): the direction net's input row
// inp[i] = [ emb[i, 0:E] | SH(rays_d[ray_id[i]]) ] with the K = deg^2 real spherical harmonics of the ray's unit direction, its backward (a
// column slice), and raw = base + residual on the colour channels with its backward (another slice).  Four byte-rate kernels: one writer per
// element, every output element written, no atomics, no LDS, no host sync.  Built with -ffp-contract=off: every float operation of the
// harmonics rounds on its own in the order tests/sh_rule.py writes it.
// Work is cut into items, 256 per block and grid-stride round: in the two input kernels an item is one 16-byte quad (E % 4 == 0, K % 4 == 0
// and 16-byte-aligned rows) or one float of the copied columns, and one further item per row computes that row's harmonics once (one sqrtf,
// three divisions) and stores its K values; in the two raw kernels an item is four rows in whole quads, and the n % 4 last rows one by one.
#include "common.h"
#include <math.h>

#define VD_BLK 256
#define VD_MAX_WIDTH 64
static inline unsigned vd_blocks(int64_t items) { return capped_blocks(items, VD_BLK, 16384); }

// sh[0 .. DEG*DEG) of the direction d; a d whose length is not > 0 counts as (0, 0, 0)
template <int DEG>
__device__ __forceinline__ void vd_harmonics(float d0, float d1, float d2, float *sh)
{
    const float n = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);                        // ray_norm's expression (ray_wave.h)
    const bool ok = n > 0.0f;
    const float x = ok ? d0 / n : 0.0f, y = ok ? d1 / n : 0.0f, z = ok ? d2 / n : 0.0f;
    sh[0] = (float)0.28209479177387814;
    if constexpr (DEG >= 2) {
        sh[1] = (float)-0.48860251190291987 * y;
        sh[2] = (float)0.48860251190291987 * z;
        sh[3] = (float)-0.48860251190291987 * x;
    }
    if constexpr (DEG >= 3) {
        const float xx = x * x, yy = y * y, zz = z * z;
        sh[4] = (float)1.0925484305920792 * (x * y);
        sh[5] = (float)-1.0925484305920792 * (y * z);
        sh[6] = (float)0.94617469575755997 * zz - (float)0.31539156525251999;
        sh[7] = (float)-1.0925484305920792 * (x * z);
        sh[8] = (float)0.54627421529603959 * (xx - yy);
        if constexpr (DEG >= 4) {
            sh[9] = ((float)0.59004358992664352 * y) * (yy - 3.0f * xx);
            sh[10] = ((float)2.8906114426405538 * (x * y)) * z;
            sh[11] = ((float)0.45704579946446572 * y) * (1.0f - 5.0f * zz);
            sh[12] = ((float)0.3731763325901154 * z) * (5.0f * zz - 3.0f);
            sh[13] = ((float)0.45704579946446572 * x) * (1.0f - 5.0f * zz);
            sh[14] = ((float)1.4453057213202769 * z) * (xx - yy);
            sh[15] = ((float)0.59004358992664352 * x) * (3.0f * yy - xx);
        }
    }
}

// Item `it` of the grid-stride round that starts at item `base` (a multiple of VD_BLK, the same in the whole block) -> its row and its place
// j in [0, P) inside the row; P <= 65 items per row.  One 64-bit division per round on block-uniform values, a 32-bit one per item.
struct vd_item {
    int64_t row;
    int j;
};
__device__ __forceinline__ vd_item vd_locate(int64_t base, int P)
{
    const int64_t row0 = base / P;
    const unsigned local = (unsigned)(base - row0 * P) + threadIdx.x;             // < P + VD_BLK
    const unsigned r = local / (unsigned)P;
    return {row0 + r, (int)(local - r * (unsigned)P)};
}

// QUAD: P = E/4 + 1, items j < E/4 copy quad j of emb's row, item E/4 stores the K/4 quads of the harmonics.  Otherwise P = E + 1 in floats.
template <int DEG, bool QUAD>
__global__ __launch_bounds__(VD_BLK) void k_viewdep_input_fwd(const float *__restrict__ emb, const float *__restrict__ rays_d,
                                                              const int32_t *__restrict__ ray_id, int64_t n, int64_t R, int E,
                                                              float *__restrict__ inp)
{
    constexpr int K = DEG * DEG;
    const int Ec = QUAD ? E >> 2 : E, P = Ec + 1, Wd = E + K;
    const int64_t items = n * P;
    for (int64_t base = (int64_t)blockIdx.x * VD_BLK; base < items; base += (int64_t)gridDim.x * VD_BLK) {
        const vd_item it = vd_locate(base, P);
        if (it.row >= n) continue;
        float *dst = inp + it.row * Wd;
        if (it.j < Ec) {
            if (QUAD) ((float4 *)dst)[it.j] = ((const float4 *)(emb + it.row * E))[it.j];
            else dst[it.j] = emb[it.row * E + it.j];
            continue;
        }
        const int64_t r = ray_id[it.row];
        float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;
        if (r >= 0 && r < R) d0 = rays_d[r * 3 + 0], d1 = rays_d[r * 3 + 1], d2 = rays_d[r * 3 + 2];
        float sh[K];
        vd_harmonics<DEG>(d0, d1, d2, sh);
        if (QUAD) {
#pragma unroll
            for (int q = 0; q < K / 4; ++q) ((float4 *)(dst + E))[q] = make_float4(sh[4 * q], sh[4 * q + 1], sh[4 * q + 2], sh[4 * q + 3]);
        } else {
#pragma unroll
            for (int k = 0; k < K; ++k) dst[E + k] = sh[k];
        }
    }
}

// g_emb[i, 0:E] = g_inp[i, 0:E] out of rows Wd wide; QUAD: in 16-byte quads (E % 4 == 0, Wd % 4 == 0, aligned), P = E/4, else P = E
template <bool QUAD>
__global__ __launch_bounds__(VD_BLK) void k_viewdep_input_bwd(const float *__restrict__ g_inp, int64_t n, int E, int Wd, float *__restrict__ g_emb)
{
    const int P = QUAD ? E >> 2 : E;
    const int64_t items = n * P;
    for (int64_t base = (int64_t)blockIdx.x * VD_BLK; base < items; base += (int64_t)gridDim.x * VD_BLK) {
        const vd_item it = vd_locate(base, P);
        if (it.row >= n) continue;
        if (QUAD) ((float4 *)(g_emb + it.row * E))[it.j] = ((const float4 *)(g_inp + it.row * Wd))[it.j];
        else g_emb[it.row * E + it.j] = g_inp[it.row * Wd + it.j];
    }
}

// Items 0 .. n4-1 (n4 = n / 4 with QUAD, else 0) are four rows each: 4 quads of base, 3 of res, 4 of raw; the others one row each.
template <bool QUAD>
__global__ __launch_bounds__(VD_BLK) void k_viewdep_raw_fwd(const float *__restrict__ base, const float *__restrict__ res, int64_t n,
                                                            float *__restrict__ raw)
{
    const int64_t n4 = QUAD ? n >> 2 : 0, items = n4 + (n - 4 * n4);
    for (int64_t it = (int64_t)blockIdx.x * VD_BLK + threadIdx.x; it < items; it += (int64_t)gridDim.x * VD_BLK) {
        if (it < n4) {
            const float4 *b = (const float4 *)base + 4 * it, *r = (const float4 *)res + 3 * it;
            float4 *o = (float4 *)raw + 4 * it;
            const float4 b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3], r0 = r[0], r1 = r[1], r2 = r[2];
            o[0] = make_float4(b0.x + r0.x, b0.y + r0.y, b0.z + r0.z, b0.w);
            o[1] = make_float4(b1.x + r0.w, b1.y + r1.x, b1.z + r1.y, b1.w);
            o[2] = make_float4(b2.x + r1.z, b2.y + r1.w, b2.z + r2.x, b2.w);
            o[3] = make_float4(b3.x + r2.y, b3.y + r2.z, b3.z + r2.w, b3.w);
        } else {
            const int64_t i = 4 * n4 + (it - n4);
            raw[4 * i + 0] = base[4 * i + 0] + res[3 * i + 0];
            raw[4 * i + 1] = base[4 * i + 1] + res[3 * i + 1];
            raw[4 * i + 2] = base[4 * i + 2] + res[3 * i + 2];
            raw[4 * i + 3] = base[4 * i + 3];
        }
    }
}

template <bool QUAD>
__global__ __launch_bounds__(VD_BLK) void k_viewdep_raw_bwd(const float *__restrict__ g_raw, int64_t n, float *__restrict__ g_res)
{
    const int64_t n4 = QUAD ? n >> 2 : 0, items = n4 + (n - 4 * n4);
    for (int64_t it = (int64_t)blockIdx.x * VD_BLK + threadIdx.x; it < items; it += (int64_t)gridDim.x * VD_BLK) {
        if (it < n4) {
            const float4 *g = (const float4 *)g_raw + 4 * it;
            float4 *o = (float4 *)g_res + 3 * it;
            const float4 g0 = g[0], g1 = g[1], g2 = g[2], g3 = g[3];
            o[0] = make_float4(g0.x, g0.y, g0.z, g1.x);
            o[1] = make_float4(g1.y, g1.z, g2.x, g2.y);
            o[2] = make_float4(g2.z, g3.x, g3.y, g3.z);
        } else {
            const int64_t i = 4 * n4 + (it - n4);
            g_res[3 * i + 0] = g_raw[4 * i + 0];
            g_res[3 * i + 1] = g_raw[4 * i + 1];
            g_res[3 * i + 2] = g_raw[4 * i + 2];
        }
    }
}

static inline bool vd_aligned16(const void *a, const void *b, const void *c = nullptr)
{
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}
static inline bool vd_aligned4(const void *a, const void *b, const void *c = nullptr)
{
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 3) == 0;
}

#define VD_REQUIRE_ROWS(who)                                                                                                                  \
    CTX_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), who ": n=%lld outside [1, 2^31)", (long long)n)
#define VD_REQUIRE_WIDTH(who)                                                                                                                 \
    CTX_REQUIRE(deg >= 1 && deg <= 4, who ": deg=%d outside [1, 4]", deg);                                                                    \
    CTX_REQUIRE(E >= 1 && E + deg * deg <= VD_MAX_WIDTH, who ": E=%d with deg=%d: want 1 <= E and E + deg^2 <= %d, the MLP's input width", E, \
                deg, VD_MAX_WIDTH)

extern "C" int32_t ctx_viewdep_input_fwd(const float *emb, const float *rays_d, const int32_t *ray_id, int64_t n, int64_t R, int32_t E,
                                         int32_t deg, float *inp, ctx_stream_t stream)
{
    CTX_REQUIRE(emb && rays_d && ray_id && inp, "viewdep_input_fwd: null pointer");
    VD_REQUIRE_ROWS("viewdep_input_fwd");
    CTX_REQUIRE(R >= 1, "viewdep_input_fwd: R=%lld rays: want R >= 1", (long long)R);
    VD_REQUIRE_WIDTH("viewdep_input_fwd");
    CTX_REQUIRE(vd_aligned4(emb, rays_d, inp) && vd_aligned4(ray_id, inp), "viewdep_input_fwd: a pointer that is not 4-byte aligned");
    const int K = deg * deg;
    const bool quad = E % 4 == 0 && K % 4 == 0 && vd_aligned16(emb, inp);
    const dim3 grid(vd_blocks(n * ((quad ? E / 4 : E) + 1))), block(VD_BLK);
    hipStream_t s = (hipStream_t)stream;
#define VD_GO(D_, Q_) hipLaunchKernelGGL((k_viewdep_input_fwd<D_, Q_>), grid, block, 0, s, emb, rays_d, ray_id, n, R, E, inp)
    if (deg == 1) VD_GO(1, false);
    else if (deg == 3) VD_GO(3, false);
    else if (deg == 2) CTX_BOOL_GO(quad, Q, VD_GO(2, Q));
    else CTX_BOOL_GO(quad, Q, VD_GO(4, Q));
#undef VD_GO
    CTX_CHECK_LAUNCH("viewdep_input_fwd");
    return CTX_OK;
}

extern "C" int32_t ctx_viewdep_input_bwd(const float *g_inp, int64_t n, int32_t E, int32_t deg, float *g_emb, ctx_stream_t stream)
{
    CTX_REQUIRE(g_inp && g_emb, "viewdep_input_bwd: null pointer");
    VD_REQUIRE_ROWS("viewdep_input_bwd");
    VD_REQUIRE_WIDTH("viewdep_input_bwd");
    CTX_REQUIRE(vd_aligned4(g_inp, g_emb), "viewdep_input_bwd: a pointer that is not 4-byte aligned");
    const int Wd = E + deg * deg;
    const bool quad = E % 4 == 0 && Wd % 4 == 0 && vd_aligned16(g_inp, g_emb);
    const dim3 grid(vd_blocks(n * (quad ? E / 4 : E))), block(VD_BLK);
    CTX_BOOL_GO(quad, Q, hipLaunchKernelGGL(k_viewdep_input_bwd<Q>, grid, block, 0, (hipStream_t)stream, g_inp, n, E, Wd, g_emb));
    CTX_CHECK_LAUNCH("viewdep_input_bwd");
    return CTX_OK;
}

extern "C" int32_t ctx_viewdep_raw_fwd(const float *base, const float *res, int64_t n, float *raw, ctx_stream_t stream)
{
    CTX_REQUIRE(base && res && raw, "viewdep_raw_fwd: null pointer");
    VD_REQUIRE_ROWS("viewdep_raw_fwd");
    CTX_REQUIRE(vd_aligned4(base, res, raw), "viewdep_raw_fwd: a pointer that is not 4-byte aligned");
    const bool quad = vd_aligned16(base, res, raw);
    const dim3 grid(vd_blocks(quad ? n / 4 + n % 4 : n)), block(VD_BLK);
    CTX_BOOL_GO(quad, Q, hipLaunchKernelGGL(k_viewdep_raw_fwd<Q>, grid, block, 0, (hipStream_t)stream, base, res, n, raw));
    CTX_CHECK_LAUNCH("viewdep_raw_fwd");
    return CTX_OK;
}

extern "C" int32_t ctx_viewdep_raw_bwd(const float *g_raw, int64_t n, float *g_res, ctx_stream_t stream)
{
    CTX_REQUIRE(g_raw && g_res, "viewdep_raw_bwd: null pointer");
    VD_REQUIRE_ROWS("viewdep_raw_bwd");
    CTX_REQUIRE(vd_aligned4(g_raw, g_res), "viewdep_raw_bwd: a pointer that is not 4-byte aligned");
    const bool quad = vd_aligned16(g_raw, g_res);
    const dim3 grid(vd_blocks(quad ? n / 4 + n % 4 : n)), block(VD_BLK);
    CTX_BOOL_GO(quad, Q, hipLaunchKernelGGL(k_viewdep_raw_bwd<Q>, grid, block, 0, (hipStream_t)stream, g_raw, n, g_res));
    CTX_CHECK_LAUNCH("viewdep_raw_bwd");
    return CTX_OK;
}
