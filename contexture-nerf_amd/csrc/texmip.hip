// Mip-mapped texture_mapping for gfx950 (the call site is src/models/render.py:135; the reference samples the atlas with four texels
// however many lie under a pixel): the pyramid of the atlas, the level of detail of every (view, face), the trilinear forward and its
// bit-reproducible backward to the atlas.  The rule is tests/mipmap_rule.py; this file is built with
// -ffp-contract=off and is array_equal to it.
//
//   ctx_mip_build                : level l texel = (sum of its covered children a, b, c, d of level l-1, from 0, in that order) / n
//   ctx_face_uv_lod              : lod[b, f] from the constant screen-space Jacobian of the face's uv (k_raster interpolates uv affinely)
//   ctx_texture_mapping_mip_fwd  : out = s0 * (1 - f) + s1 * f, s0 and s1 the bilinear taps (texel_taps.h) at levels (int)lod and (int)lod + 1
//   ctx_texture_mapping_mip_bwd  : the terms w_k * g * (1 - f) and w'_k * g * f into the 64-bit integer pyramid of section 4j, then one
//                                  launch converts the levels and collapses them onto level 0 through the pyramid's weights 1 / n
//
// Levels 1 .. L-1 are planar: pyr = [C, T1, T1 | C, T2, T2 | ...] floats, then a 256-byte trailer whose first word is the sticky status
// (1: a forward met a face_idx outside the lod table; its pixel is NaN).  Level 0 is the caller's atlas and is never copied.
// cov_count = [T0^2 | T1^2 | ...] bytes: cov_0 (0 or 1), then n_l, the number of covered children of every texel of level l.
#include "hashgrid_common.h"
#include "texel_taps.h"

#pragma clang fp contract(off)

#define MIP_MAX_LEVELS 16
#define MIP_TILE 32                    // a 32 x 32 tile of the source level gives five levels in one pass through LDS
#define MIP_PASS 5

struct MipGeo {
    int64_t off[MIP_MAX_LEVELS + 1];   // texels of the levels before l, level 0 included: off[l] = sum over j < l of (T >> j)^2
    int T, L;
    __host__ __device__ int side(int l) const { return T >> l; }
    __host__ __device__ int64_t texels() const { return off[L]; }                          // of one channel, every level
    __host__ __device__ int64_t pyr_off(int l, int C) const { return (off[l] - off[1]) * C; }   // floats before level l >= 1 in pyr
};

static int32_t mip_check(const char *who, int32_t C, int32_t T, int32_t L, MipGeo &g)
{
    CTX_REQUIRE(C >= 1 && C <= 4, "%s: C=%d outside [1, 4]", who, C);
    CTX_REQUIRE(L >= 1 && L <= MIP_MAX_LEVELS, "%s: mip levels L=%d outside [1, %d]", who, L, MIP_MAX_LEVELS);
    CTX_REQUIRE(T >= 2 && T <= 16384, "%s: T=%d outside [2, 16384]", who, T);
    CTX_REQUIRE(T % (1 << (L - 1)) == 0 && (T >> (L - 1)) >= 2,
                "%s: mip levels L=%d do not fit T=%d (T must be a multiple of 2^(L-1) and the last level at least 2 x 2)", who, L, T);
    g.T = T; g.L = L;
    g.off[0] = 0;
    for (int l = 0; l < MIP_MAX_LEVELS; ++l) g.off[l + 1] = g.off[l] + (l < L ? (int64_t)(T >> l) * (T >> l) : 0);
    return CTX_OK;
}

static int64_t mip_pyr_floats(const MipGeo &g, int C) { return (g.off[g.L] - g.off[1]) * C; }
struct MipTrailer { int32_t bad; int32_t pad[63]; };
static MipTrailer *mip_trailer(float *pyr, const MipGeo &g, int C) { return (MipTrailer *)((char *)pyr + hg_align(mip_pyr_floats(g, C) * 4)); }

extern "C" int64_t ctx_mip_levels_bytes(int32_t C, int32_t T, int32_t L)
{
    MipGeo g;
    if (mip_check("mip_levels_bytes", C, T, L, g)) return -1;
    return hg_align(mip_pyr_floats(g, C) * 4) + (int64_t)sizeof(MipTrailer);
}

extern "C" int64_t ctx_mip_cov_bytes(int32_t T, int32_t L)
{
    MipGeo g;
    if (mip_check("mip_cov_bytes", 1, T, L, g)) return -1;
    return g.texels();
}

// ---- the pyramid ------------------------------------------------------------------------------------------------------------------
// One workgroup per 32 x 32 tile of level s and channel: levels s+1 .. s+nlev, every one from the level before it in LDS.  src is level
// s of this channel's plane ([Ts, Ts]); the coverage of level s is the caller's plane (s = 0; null: everything) or n_s > 0.
__global__ __launch_bounds__(256) void k_mip_build(const float *__restrict__ tex, const uint8_t *__restrict__ coverage, float *__restrict__ pyr,
                                                   uint8_t *__restrict__ cov_count, MipGeo g, int C, int s, int nlev)
{
    __shared__ float s_v[1024 + 256 + 64 + 16 + 4 + 1];
    __shared__ uint8_t s_c[1024 + 256 + 64 + 16 + 4 + 1];
    const int c = blockIdx.z, Ts = g.side(s);
    const float *src = s == 0 ? tex + (int64_t)c * Ts * Ts : pyr + g.pyr_off(s, C) + (int64_t)c * Ts * Ts;
    const uint8_t *scov = s == 0 ? coverage : cov_count + g.off[s];            // null only for s = 0 without a coverage plane
    const int y0 = blockIdx.y * MIP_TILE, x0 = blockIdx.x * MIP_TILE;
    for (int i = threadIdx.x; i < MIP_TILE * MIP_TILE; i += 256) {
        const int y = y0 + (i >> 5), x = x0 + (i & 31);
        const bool in = y < Ts && x < Ts;
        const bool cov = in && (scov ? scov[(int64_t)y * Ts + x] != 0 : true);
        s_v[i] = in ? src[(int64_t)y * Ts + x] : 0.0f;
        s_c[i] = cov ? 1 : 0;
        if (s == 0 && c == 0 && cov_count && in) cov_count[(int64_t)y * Ts + x] = cov ? 1 : 0;
    }
    int from = 0, side = MIP_TILE;                                             // the level before: its place in LDS and its side there
    for (int j = 1; j <= nlev; ++j) {
        __syncthreads();
        const int to = from + side * side, half = side >> 1, Tl = g.side(s + j);
        for (int i = threadIdx.x; i < half * half; i += 256) {
            const int ly = i / half, lx = i - ly * half;
            const int a = from + (2 * ly) * side + 2 * lx;
            float sum = 0.0f;
            int n = 0;
            if (s_c[a]) { sum = sum + s_v[a]; ++n; }
            if (s_c[a + 1]) { sum = sum + s_v[a + 1]; ++n; }
            if (s_c[a + side]) { sum = sum + s_v[a + side]; ++n; }
            if (s_c[a + side + 1]) { sum = sum + s_v[a + side + 1]; ++n; }
            const float v = n ? sum / (float)n : 0.0f;
            s_v[to + i] = v;
            s_c[to + i] = n ? 1 : 0;
            const int y = (y0 >> j) + ly, x = (x0 >> j) + lx;
            if (y < Tl && x < Tl) {
                pyr[g.pyr_off(s + j, C) + ((int64_t)c * Tl + y) * Tl + x] = v;
                if (c == 0 && cov_count) cov_count[g.off[s + j] + (int64_t)y * Tl + x] = (uint8_t)n;
            }
        }
        from = to; side = half;
    }
}

extern "C" int32_t ctx_mip_build(const float *tex, const uint8_t *coverage, int32_t C, int32_t T, int32_t L, float *pyr, uint8_t *cov_count,
                                 ctx_stream_t stream)
{
    MipGeo g;
    if (int32_t rc = mip_check("mip_build", C, T, L, g)) return rc;
    CTX_REQUIRE(tex && pyr, "mip_build: null pointer");
    CTX_REQUIRE(cov_count || (!coverage && L - 1 <= MIP_PASS),
                "mip_build: cov_count is needed with a coverage plane, and beyond %d levels (the later passes read the counts)", MIP_PASS + 1);
    hipStream_t st = (hipStream_t)stream;
    (void)hipMemsetAsync(mip_trailer(pyr, g, C), 0, sizeof(MipTrailer), st);
    if (L == 1 && cov_count) {                                                 // no level to reduce: cov_0 alone
        if (coverage) (void)hipMemcpyAsync(cov_count, coverage, (size_t)T * T, hipMemcpyDeviceToDevice, st);
        else (void)hipMemsetAsync(cov_count, 1, (size_t)T * T, st);
    }
    for (int s = 0; s < L - 1; s += MIP_PASS) {
        const int nlev = min(MIP_PASS, L - 1 - s), nt = cdiv(g.side(s), MIP_TILE);
        hipLaunchKernelGGL(k_mip_build, dim3(nt, nt, C), dim3(256), 0, st, tex, coverage, pyr, cov_count, g, C, s, nlev);
    }
    CTX_CHECK_LAUNCH("mip_build");
    return CTX_OK;
}

/* the sticky status of a pyramid: 1 when a forward met a face_idx outside its lod table (that pixel is NaN).  Synchronises the stream. */
extern "C" int32_t ctx_mip_status(const float *pyr, int32_t C, int32_t T, int32_t L, ctx_stream_t stream)
{
    MipGeo g;
    if (int32_t rc = mip_check("mip_status", C, T, L, g)) return rc;
    CTX_REQUIRE(pyr, "mip_status: null pointer");
    MipTrailer t;
    if (hipMemcpyAsync(&t, mip_trailer((float *)pyr, g, C), sizeof(t), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess) return CTX_E_LAUNCH;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return CTX_E_LAUNCH;
    return t.bad ? 1 : 0;
}

// ---- the level of detail of a (view, face) -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_face_uv_lod(const float *__restrict__ fvi, const float *__restrict__ uva, int Bu, int F, int H, int W, int T,
                                                     int L, const float *__restrict__ scale, float *__restrict__ lod)
{
    const int b = blockIdx.y, f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const float *p = fvi + ((int64_t)b * F + f) * 6, *t = uva + ((int64_t)(Bu == 1 ? 0 : b) * F + f) * 6;
    const float e1x = p[2] - p[0], e1y = p[3] - p[1], e2x = p[4] - p[0], e2y = p[5] - p[1];
    const float d1u = t[2] - t[0], d1v = t[3] - t[1], d2u = t[4] - t[0], d2v = t[5] - t[1];
    const float det = e1x * e2y - e2x * e1y;
    float out = 0.0f;
    if (det != 0.0f && isfinite(det)) {
        const float ux = (d1u * e2y - d2u * e1y) / det, uy = (d2u * e1x - d1u * e2x) / det;
        const float vx = (d1v * e2y - d2v * e1y) / det, vy = (d2v * e1x - d1v * e2x) / det;
        const float sb = scale ? scale[b] : 1.0f;
        const float ax = ((2.0f / (float)W) * (float)T) * sb, ay = ((2.0f / (float)H) * (float)T) * sb;
        const float r2 = fmaxf((ax * ax) * ((ux * ux) + (vx * vx)), (ay * ay) * ((uy * uy) + (vy * vy)));
        if (r2 > 1.0f) {                                                       // false for magnification and for NaN
            if (isinf(r2)) out = (float)(L - 1);
            else {
                const uint32_t bits = __float_as_uint(sqrtf(r2));              // rho >= 1: a normal number
                const int l0 = (int)(bits >> 23) - 127;                        // ilogbf(rho)
                const float m = __uint_as_float((bits & 0x007fffffu) | 0x3f800000u);   // ldexpf(rho, -l0), in [1, 2)
                out = l0 >= L - 1 ? (float)(L - 1) : (float)l0 + (m - 1.0f);
            }
        }
    }
    lod[(int64_t)b * F + f] = out;
}

extern "C" int32_t ctx_face_uv_lod(const float *fvi, const float *uva, int32_t Bu, int32_t B, int32_t F, int32_t H, int32_t W, int32_t T, int32_t L,
                                   const float *scale, float *lod, ctx_stream_t stream)
{
    MipGeo g;
    if (int32_t rc = mip_check("face_uv_lod", 1, T, L, g)) return rc;
    CTX_REQUIRE(fvi && uva && lod, "face_uv_lod: null pointer");
    CTX_REQUIRE(B >= 1 && B <= 65535 && F >= 1 && H >= 1 && W >= 1 && (Bu == 1 || Bu == B), "face_uv_lod: bad sizes B=%d F=%d H=%d W=%d Bu=%d", B, F, H, W,
                Bu);
    hipLaunchKernelGGL(k_face_uv_lod, dim3(cdiv(F, 256), B), dim3(256), 0, (hipStream_t)stream, fvi, uva, Bu, F, H, W, T, L, scale, lod);
    CTX_CHECK_LAUNCH("face_uv_lod");
    return CTX_OK;
}

// ---- a pixel's two levels --------------------------------------------------------------------------------------------------------------
// lod of a table entry, kept inside [0, L-1] whatever the table holds (fmaxf first: a NaN becomes 0): l0 = (int)lod, f = lod - l0, and
// f > 0 only below the last level
struct MipLod { int l0; float f; };
__device__ __forceinline__ MipLod mip_lod(float lod, int L)
{
    lod = fminf(fmaxf(lod, 0.0f), (float)(L - 1));
    MipLod m;
    m.l0 = (int)lod;
    m.f = lod - (float)m.l0;
    return m;
}

// the bilinear tap of one level, channel by channel, in k_texmap_fwd's order
template <int C>
__device__ __forceinline__ void mip_tap(const float *__restrict__ lv, int Tl, const TexelTaps &t, float (&r)[C])
{
    float a[4][C];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t at = (int64_t)min(t.y(k), Tl - 1) * Tl + min(t.x(k), Tl - 1);      // x1, y1 clamped into the level: the four gathers in flight
#pragma unroll
        for (int c = 0; c < C; ++c) a[k][c] = lv[(int64_t)c * Tl * Tl + at];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (t.in[k]) acc = acc + a[k][c] * t.w[k];
        r[c] = acc;
    }
}

template <int C>
__global__ __launch_bounds__(256) void k_texmip_fwd(const float *__restrict__ uv, const float *__restrict__ tex, const float *__restrict__ pyr,
                                                    const float *__restrict__ lod, const int64_t *__restrict__ face_idx, int64_t HW, int F, MipGeo g,
                                                    int32_t *__restrict__ bad, float *__restrict__ out)
{
    const int b = blockIdx.y;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += (int64_t)gridDim.x * 256) {
        const int64_t pix = (int64_t)b * HW + i;
        const int64_t fi = face_idx[pix];
        float r[C];
#pragma unroll
        for (int c = 0; c < C; ++c) r[c] = 0.0f;
        if (fi >= F) {                                                         // outside the table: never read, the pixel says so
            *bad = 1;
#pragma unroll
            for (int c = 0; c < C; ++c) r[c] = __uint_as_float(0x7fc00000u);
        } else if (fi >= 0) {
            const float2 q = *(const float2 *)(uv + pix * 2);
            const MipLod m = mip_lod(lod[(int64_t)b * F + fi], g.L);
            const int T0 = g.side(m.l0);
            mip_tap<C>(m.l0 == 0 ? tex : pyr + g.pyr_off(m.l0, C), T0, texel_taps(q.x, q.y, T0), r);
            if (m.f > 0.0f) {
                float r1[C];
                const int T1 = g.side(m.l0 + 1);
                mip_tap<C>(pyr + g.pyr_off(m.l0 + 1, C), T1, texel_taps(q.x, q.y, T1), r1);
#pragma unroll
                for (int c = 0; c < C; ++c) r[c] = r[c] * (1.0f - m.f) + r1[c] * m.f;
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) out[pix * C + c] = r[c];
    }
}

#define MIP_LAUNCH_C(kernel, C, ...)                                  \
    do {                                                              \
        if (C == 1) hipLaunchKernelGGL(kernel<1>, __VA_ARGS__);       \
        else if (C == 2) hipLaunchKernelGGL(kernel<2>, __VA_ARGS__);  \
        else if (C == 3) hipLaunchKernelGGL(kernel<3>, __VA_ARGS__);  \
        else hipLaunchKernelGGL(kernel<4>, __VA_ARGS__);              \
    } while (0)

static int32_t mip_check_raster(const char *who, int32_t B, int32_t HW, int32_t F)
{
    CTX_REQUIRE(B >= 1 && B <= 65535 && HW >= 1 && F >= 1, "%s: bad sizes B=%d HW=%d F=%d", who, B, HW, F);
    return CTX_OK;
}

extern "C" int32_t ctx_texture_mapping_mip_fwd(const float *uv, const float *tex, float *pyr, const float *lod, const int64_t *face_idx, int32_t B,
                                               int32_t HW, int32_t F, int32_t C, int32_t T, int32_t L, float *out, ctx_stream_t stream)
{
    MipGeo g;
    if (int32_t rc = mip_check("texture_mapping_mip_fwd", C, T, L, g)) return rc;
    if (int32_t rc = mip_check_raster("texture_mapping_mip_fwd", B, HW, F)) return rc;
    CTX_REQUIRE(uv && tex && pyr && lod && face_idx && out, "texture_mapping_mip_fwd: null pointer (mode 'mipmap' needs the lod table and face_idx)");
    MIP_LAUNCH_C(k_texmip_fwd, C, dim3(capped_blocks(HW, 256, 4096), B), dim3(256), 0, (hipStream_t)stream, uv, tex, (const float *)pyr, lod, face_idx,
                 (int64_t)HW, F, g, &mip_trailer(pyr, g, C)->bad, out);
    CTX_CHECK_LAUNCH("texture_mapping_mip_fwd");
    return CTX_OK;
}

// ---- backward to the atlas ---------------------------------------------------------------------------------------------------------
// Stage A.  One thread per pixel, so the lanes of a wave are neighbours on the screen and, under minification, address the same coarse
// texel: hg_presum_runs adds the terms of such a run into its first lane.  acc = [level 0: C, T, T | level 1: C, T1, T1 | ...]; ctl->pad
// is the sticky word of the call (a face_idx outside the table poisons the gradient, as a non-finite grad_out does).
template <int C>
__global__ __launch_bounds__(HG_BLOCK) void k_texmip_bwd(const float *__restrict__ go, const float *__restrict__ uv, const float *__restrict__ lod,
                                                         const int64_t *__restrict__ face_idx, int64_t HW, int F, MipGeo g, int E, int presum,
                                                         HgCtl *__restrict__ ctl, unsigned long long *__restrict__ acc)
{
    if (ctl->status != 0) return;                                              // uniform over the grid
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * HG_BLOCK + threadIdx.x, pix = (int64_t)b * HW + i;
    const int64_t fi = i < HW ? face_idx[pix] : -1;
    if (fi >= F) ctl->pad = 1;
    const bool fg = fi >= 0 && fi < F;                                         // a lane without a pixel stays for the shuffles, with terms of 0
    float2 q2 = make_float2(0.0f, 0.0f);
    MipLod m = {0, 0.0f};
    float gc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) gc[c] = 0.0f;
    if (fg) {
        q2 = *(const float2 *)(uv + pix * 2);
        m = mip_lod(lod[(int64_t)b * F + fi], g.L);
#pragma unroll
        for (int c = 0; c < C; ++c) gc[c] = go[pix * C + c];
    }
    const double scale = hg_pow2(E - ctl->x);
#pragma unroll
    for (int hi = 0; hi < 2; ++hi) {
        const bool on = fg && (hi == 0 || m.f > 0.0f);
        if (hi == 1 && !__any(on)) break;                                      // uniform over the wave
        const int l = on ? m.l0 + hi : 0, Tl = g.side(l);
        const TexelTaps t = texel_taps(q2.x, q2.y, Tl);
        float gl[C];
#pragma unroll
        for (int c = 0; c < C; ++c) gl[c] = m.f > 0.0f ? gc[c] * (hi ? m.f : 1.0f - m.f) : gc[c];
        unsigned long long *al = acc + g.off[l] * C;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool live = on && t.in[k];
            const int64_t at = (int64_t)min(t.y(k), Tl - 1) * Tl + min(t.x(k), Tl - 1);
            long long qq[C];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float prod = t.w[k] * gl[c];                             // one rounding
                qq[c] = live ? __double2ll_rn((double)prod * scale) : 0;       // |prod| < 2^x: |q| <= 2^E, exact scaling, nearest even
            }
            const bool issue = presum ? hg_presum_runs<C>((uint32_t)(g.off[l] + at), live, lane, qq) : live;
            if (issue) {
#pragma unroll
                for (int c = 0; c < C; ++c)
                    if (qq[c]) atomicAdd(al + (int64_t)c * Tl * Tl + at, (unsigned long long)qq[c]);
            }
        }
    }
}

// Stage B.  One thread per level-0 texel and channel: the levels converted, then collapsed onto level 0 in ascending order.
__global__ __launch_bounds__(HG_BLOCK) void k_texmip_collapse(const long long *__restrict__ acc, const uint8_t *__restrict__ cov_count, MipGeo g, int C, int E,
                                                              const HgCtl *__restrict__ ctl, float *__restrict__ gt)
{
    const int status = ctl->pad ? 2 : ctl->status;
    const double inv = hg_pow2(ctl->x - E);
    const int T = g.T;
    const int64_t plane = (int64_t)T * T, count = plane * C, stride = (int64_t)gridDim.x * HG_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * HG_BLOCK + threadIdx.x; i < count; i += stride) {
        if (status) { gt[i] = status == 2 ? __uint_as_float(0x7fc00000u) : 0.0f; continue; }
        const int c = (int)(i / plane);
        const int64_t r = i - c * plane;
        const int y = (int)(r / T), x = (int)(r - (int64_t)y * T);
        float g0 = 0.0f;
        if (!cov_count || cov_count[r]) {
            g0 = (float)((double)acc[i] * inv);
            float wt = 1.0f;
            for (int l = 1; l < g.L; ++l) {
                const int Tl = g.side(l);
                const int64_t at = (int64_t)(y >> l) * Tl + (x >> l);
                wt = wt / (float)(cov_count ? (int)cov_count[g.off[l] + at] : 4);
                g0 = g0 + (float)((double)acc[g.off[l] * C + (int64_t)c * Tl * Tl + at] * inv) * wt;
            }
        }
        gt[i] = g0;
    }
}

extern "C" int64_t ctx_texture_mapping_mip_bwd_ws_bytes(int32_t C, int32_t T, int32_t L)
{
    MipGeo g;
    if (mip_check("texture_mapping_mip_bwd_ws_bytes", C, T, L, g)) return -1;
    return hg_align(g.texels() * C * 8) + 256;
}

extern "C" int32_t ctx_texture_mapping_mip_bwd(const float *grad_out, const float *uv, const float *lod, const int64_t *face_idx, const uint8_t *cov_count,
                                               int32_t B, int32_t HW, int32_t F, int32_t C, int32_t T, int32_t L, void *ws, float *grad_tex,
                                               ctx_stream_t stream)
{
    MipGeo g;
    if (int32_t rc = mip_check("texture_mapping_mip_bwd", C, T, L, g)) return rc;
    if (int32_t rc = mip_check_raster("texture_mapping_mip_bwd", B, HW, F)) return rc;
    CTX_REQUIRE(grad_out && uv && lod && face_idx && ws && grad_tex, "texture_mapping_mip_bwd: null pointer");
    const int presum = ctx_env_int("CTX_TEXMIP_PRESUM", 1) != 0;               // read per call: a tool times both forms in one process
    hipStream_t s = (hipStream_t)stream;
    const int64_t count = g.texels() * C, n = (int64_t)B * HW;
    unsigned long long *acc = (unsigned long long *)ws;
    HgCtl *ctl = (HgCtl *)((char *)ws + hg_align(count * 8));
    const int E = hg_acc_exponent(n, 4);
    (void)hipMemsetAsync(acc, 0, count * 8, s);
    (void)hipMemsetAsync(ctl, 0, sizeof(HgCtl), s);
    hipLaunchKernelGGL(k_hashgrid_absmax, dim3(capped_blocks(n * C, HG_BLOCK * 4, 1024)), dim3(HG_BLOCK), 0, s, grad_out, n * C, ctl);
    hipLaunchKernelGGL(k_hashgrid_scale, dim3(1), dim3(1), 0, s, ctl);
    MIP_LAUNCH_C(k_texmip_bwd, C, dim3((unsigned)cdiv64(HW, HG_BLOCK), B), dim3(HG_BLOCK), 0, s, grad_out, uv, lod, face_idx, (int64_t)HW, F, g, E, presum,
                 ctl, acc);
    hipLaunchKernelGGL(k_texmip_collapse, dim3(capped_blocks((int64_t)T * T * C, HG_BLOCK, 4096)), dim3(HG_BLOCK), 0, s, (const long long *)acc, cov_count, g,
                       C, E, ctl, grad_tex);
    CTX_CHECK_LAUNCH("texture_mapping_mip_bwd");
    return CTX_OK;
}
