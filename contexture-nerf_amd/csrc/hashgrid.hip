// Multiresolution hash-grid encoding (instant-ngp): xyz -> Lv levels x F trainable features, trilinear in each level's grid.
// The rule is tests/hashgrid_rule.py; this file is built with -ffp-contract=off and is array_equal to it.
//
//   ctx_hashgrid_fwd : emb[n, l*F + f] = sum over the 8 corners of the point's cell at level l of w_c * table[l, idx_c, f]
//   ctx_hashgrid_bwd : g_table[l, idx_c, f] += w_c * g_emb[n, l*F + f], summed as 64-bit integers (a fixed-point accumulator scaled from
//                      max|g_emb|), so the result does not depend on the order the adds arrive in: bit-reproducible
//
//   ctx_hashgrid_bwd_pts : g_pts[n, a] = sum over the levels of (sum_f g_emb[n, l*F + f] * d emb[n, l*F + f] / d w_a) * res[l] / (hi_a - lo_a):
//                      the derivative of the trilinear interpolation in the cell the forward assigns the point to, 0 on an axis
//                      that is not strictly inside the box (the rule: tests/hashgrid_grad_rule.py).  No atomics.
//
// Mapping of all three: one thread per (point, level), blockIdx.y = level.  Workgroups are dispatched x-fastest, so the chip works on
// one level at a time and that level's T*F*4 (forward, backward to the positions) or T*F*8 (backward to the table) bytes stay hot in
// L2 - instant-ngp's mapping.  A thread gathers (adds to) 8 entries of F floats (F int64) and stores (loads) its F floats of the
// point's row; the backward to the positions stores its three per-level partials to a scratch [Lv, n, 3], which a second kernel (one
// thread per point) adds in ascending level order.  From 2^17 points on it runs as one thread per point over the levels instead.
// The positions' gradient is first order only and opt-in on the host.  No transcendental runs here: the level resolutions are integers
// computed on the host.
#include "hashgrid_common.h"

// the table, and the box that maps a position to unit coordinates
struct HgGrid : HgTable {
    float lo[3], hi[3];
};

// what every entry point accepts
static int32_t hg_check(const char *who, int32_t Lv, int32_t F, int32_t log2T, const int32_t *res, const float *lo, const float *hi, HgGrid &g)
{
    CTX_REQUIRE(res && lo && hi, "%s: null res / lo / hi", who);
    if (int32_t rc = hg_check_table(who, Lv, F, log2T, res, g)) return rc;
    for (int a = 0; a < 3; ++a) {
        CTX_REQUIRE(isfinite(lo[a]) && isfinite(hi[a]) && lo[a] < hi[a], "%s: box axis %d: want finite lo < hi (lo=%g hi=%g)", who, a, lo[a], hi[a]);
        g.lo[a] = lo[a]; g.hi[a] = hi[a];
    }
    return CTX_OK;
}

// point n on level l: its unit coordinates in the box, axis by axis; every row is live
__device__ __forceinline__ HgAxes<3> hg_axes(const float *__restrict__ pts, int64_t n, const HgGrid &g, int l)
{
    float x[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) x[a] = (pts[n * 3 + a] - g.lo[a]) / (g.hi[a] - g.lo[a]);
    return hg_axes<3>(x, g.res[l]);
}

template <int F>
__global__ __launch_bounds__(HG_BLOCK) void k_hashgrid_fwd(const float *__restrict__ pts, int64_t n, const float *__restrict__ table, HgGrid g,
                                                           float *__restrict__ emb)
{
    typedef typename HgVec<F>::type V;
    const int l = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * HG_BLOCK + threadIdx.x;
    if (p >= n) return;
    float o[F];
    hg_interpolate<3, F>(hg_axes(pts, p, g, l), g, l, table, o);
    *(V *)(emb + hg_row<F>(p, g, l)) = *(const V *)o;
}

extern "C" int32_t ctx_hashgrid_fwd(const float *pts, int64_t n, const float *table, int32_t Lv, int32_t F, int32_t log2T, const int32_t *res,
                                    const float *lo, const float *hi, float *emb, ctx_stream_t stream)
{
    HgGrid g;
    if (int32_t rc = hg_check("hashgrid_fwd", Lv, F, log2T, res, lo, hi, g)) return rc;
    CTX_REQUIRE(pts && table && emb, "hashgrid_fwd: null pointer");
    CTX_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "hashgrid_fwd: n=%lld outside [1, 2^31)", (long long)n);
    HG_LAUNCH_F(k_hashgrid_fwd, F, dim3((unsigned)cdiv64(n, HG_BLOCK), Lv), dim3(HG_BLOCK), 0, (hipStream_t)stream, pts, n, table, g, emb);
    CTX_CHECK_LAUNCH("hashgrid_fwd");
    return CTX_OK;
}

// ---- backward to the table -------------------------------------------------------------------------------------------------------
// the accumulator, its helper kernels and the host driver are in hashgrid_common.h.  Points arrive unordered: every lane adds its own terms
template <int F>
__global__ __launch_bounds__(HG_BLOCK) void k_hashgrid_bwd(const float *__restrict__ pts, int64_t n, const float *__restrict__ g_emb, HgGrid g, int E,
                                                           const HgCtl *__restrict__ ctl, unsigned long long *__restrict__ acc)
{
    typedef typename HgVec<F>::type V;
    if (ctl->status != 0) return;
    const int l = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * HG_BLOCK + threadIdx.x;
    if (p >= n) return;
    float ge[F];
    *(V *)ge = *(const V *)(g_emb + hg_row<F>(p, g, l));
    hg_accumulate<3, F>(hg_cell(hg_axes(pts, p, g, l), g.res[l], g.log2T), ge, hg_pow2(E - ctl->x), acc + ((int64_t)l << g.log2T) * F,
                        [](uint32_t, const long long (&)[F]) { return true; });
}

extern "C" int64_t ctx_hashgrid_bwd_ws_bytes(int32_t Lv, int32_t F, int32_t log2T)
{
    return hg_table_bwd_ws_bytes("hashgrid_bwd_ws_bytes", Lv, F, log2T);
}

extern "C" int32_t ctx_hashgrid_bwd(const float *pts, int64_t n, const float *g_emb, int32_t Lv, int32_t F, int32_t log2T, const int32_t *res,
                                    const float *lo, const float *hi, int32_t stages, void *ws, float *g_table, ctx_stream_t stream)
{
    HgGrid g;
    if (int32_t rc = hg_check("hashgrid_bwd", Lv, F, log2T, res, lo, hi, g)) return rc;
    CTX_REQUIRE(pts && g_emb && ws && g_table, "hashgrid_bwd: null pointer");
    CTX_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "hashgrid_bwd: n=%lld outside [1, 2^31)", (long long)n);
    hipStream_t s = (hipStream_t)stream;
    return hg_table_bwd<3>(
        "hashgrid_bwd", n, g, F, stages, ws, g_table, s,
        [&](dim3 blocks, HgCtl *ctl) { hipLaunchKernelGGL(k_hashgrid_absmax, blocks, dim3(HG_BLOCK), 0, s, g_emb, n * Lv * F, ctl); },
        [&](dim3 grid, int E, const HgCtl *ctl, unsigned long long *acc) {
            HG_LAUNCH_F(k_hashgrid_bwd, F, grid, dim3(HG_BLOCK), 0, s, pts, n, g_emb, g, E, ctl, acc);
        });
}

// ---- backward to the positions ---------------------------------------------------------------------------------------------------
// One level's three partials gl_a * s_a of a point.  d_a[f] = d emb[f] / d w_a: per corner, ascending, the product of the two other
// axes' factors times the entry, added where the corner's bit on axis a is set and subtracted where it is not.
template <int F>
__device__ __forceinline__ void hg_level_grad(const float *__restrict__ pts, int64_t p, const float *__restrict__ table,
                                              const float *__restrict__ g_emb, const HgGrid &g, int l, float out[3])
{
    typedef typename HgVec<F>::type V;
    const HgAxes<3> ax = hg_axes(pts, p, g, l);
    const HgCell<3> c = hg_cell(ax, g.res[l], g.log2T);
    const float *tl = table + ((int64_t)l << g.log2T) * F;
    float t[8][F];
#pragma unroll
    for (int k = 0; k < 8; ++k) *(V *)t[k] = *(const V *)(tl + (int64_t)c.idx[k] * F);   // the 8 gathers in flight together
    float ge[F];
    *(V *)ge = *(const V *)(g_emb + hg_row<F>(p, g, l));
    float d[3][F];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int f = 0; f < F; ++f) d[a][f] = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int bit[3] = {k & 1, (k >> 1) & 1, (k >> 2) & 1};
        float s[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) s[a] = bit[a] ? ax.w[a] : 1.0f - ax.w[a];
        const float q[3] = {s[1] * s[2], s[0] * s[2], s[0] * s[1]};
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int f = 0; f < F; ++f) {
                const float term = q[a] * t[k][f];
                d[a][f] = bit[a] ? d[a][f] + term : d[a][f] - term;
            }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float gl = 0.0f;
#pragma unroll
        for (int f = 0; f < F; ++f) gl = gl + ge[f] * d[a][f];
        out[a] = gl * ((float)g.res[l] / (g.hi[a] - g.lo[a]));
    }
}

template <int F>
__global__ __launch_bounds__(HG_BLOCK) void k_hashgrid_bwd_pts(const float *__restrict__ pts, int64_t n, const float *__restrict__ table,
                                                               const float *__restrict__ g_emb, HgGrid g, float *__restrict__ part)
{
    const int l = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * HG_BLOCK + threadIdx.x;
    if (p >= n) return;
    float o[3];
    hg_level_grad<F>(pts, p, table, g_emb, g, l, o);
    float *dst = part + ((int64_t)l * n + p) * 3;
    dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
}

// g_pts[p, a] = the partials of the levels added in ascending order from 0, or exactly 0 on an inactive axis whatever the partials hold
__global__ __launch_bounds__(HG_BLOCK) void k_hashgrid_bwd_pts_sum(const float *__restrict__ pts, int64_t n, HgGrid g, const float *__restrict__ part,
                                                                   float *__restrict__ g_pts)
{
    const int64_t p = (int64_t)blockIdx.x * HG_BLOCK + threadIdx.x;
    if (p >= n) return;
    const HgAxes<3> ax = hg_axes(pts, p, g, 0);                                              // the active flags do not depend on the level
    float s[3] = {0.0f, 0.0f, 0.0f};
    for (int l = 0; l < g.Lv; ++l) {
        const float *src = part + ((int64_t)l * n + p) * 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) s[a] = s[a] + src[a];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) g_pts[p * 3 + a] = ax.active[a] ? s[a] : 0.0f;
}

// The mapping for many points (n >= HG_PTS_LOOP_MIN_N; CTX_HASHGRID_PTS_LOOP=0|1 forces one of the two): one thread per
// point walks the levels in ascending order, so there is no scratch traffic and no second kernel, and the same bits.  With few points it
// leaves most of the chip idle and the per-level mapping wins; from about 10^5 points on the scratch's 24 Lv n bytes cost more.
#define HG_PTS_LOOP_MIN_N (1 << 17)
template <int F>
__global__ __launch_bounds__(HG_BLOCK) void k_hashgrid_bwd_pts_loop(const float *__restrict__ pts, int64_t n, const float *__restrict__ table,
                                                                    const float *__restrict__ g_emb, HgGrid g, float *__restrict__ g_pts)
{
    const int64_t p = (int64_t)blockIdx.x * HG_BLOCK + threadIdx.x;
    if (p >= n) return;
    const HgAxes<3> ax = hg_axes(pts, p, g, 0);
    float s[3] = {0.0f, 0.0f, 0.0f};
    for (int l = 0; l < g.Lv; ++l) {
        float o[3];
        hg_level_grad<F>(pts, p, table, g_emb, g, l, o);
#pragma unroll
        for (int a = 0; a < 3; ++a) s[a] = s[a] + o[a];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) g_pts[p * 3 + a] = ax.active[a] ? s[a] : 0.0f;
}

extern "C" int64_t ctx_hashgrid_bwd_pts_ws_bytes(int64_t n, int32_t Lv)
{
    if (n < 1 || n >= ((int64_t)1 << 31) || Lv < 1 || Lv > HG_MAX_LEVELS) return -1;
    return hg_align((int64_t)Lv * n * 3 * 4);                   // the per-level partials [Lv, n, 3], whichever mapping runs
}

extern "C" int32_t ctx_hashgrid_bwd_pts(const float *pts, int64_t n, const float *table, const float *g_emb, int32_t Lv, int32_t F, int32_t log2T,
                                        const int32_t *res, const float *lo, const float *hi, void *ws, float *g_pts, ctx_stream_t stream)
{
    HgGrid g;
    if (int32_t rc = hg_check("hashgrid_bwd_pts", Lv, F, log2T, res, lo, hi, g)) return rc;
    CTX_REQUIRE(pts && table && g_emb && ws && g_pts, "hashgrid_bwd_pts: null pointer");
    CTX_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "hashgrid_bwd_pts: n=%lld outside [1, 2^31)", (long long)n);
    float *part = (float *)ws;
    hipStream_t s = (hipStream_t)stream;
    const int forced = ctx_env_int("CTX_HASHGRID_PTS_LOOP", -1);  // read per call: a tool measures both mappings in one process
    if (forced < 0 ? n >= HG_PTS_LOOP_MIN_N : forced != 0) {
        HG_LAUNCH_F(k_hashgrid_bwd_pts_loop, F, dim3((unsigned)cdiv64(n, HG_BLOCK)), dim3(HG_BLOCK), 0, s, pts, n, table, g_emb, g, g_pts);
        CTX_CHECK_LAUNCH("hashgrid_bwd_pts");
        return CTX_OK;
    }
    HG_LAUNCH_F(k_hashgrid_bwd_pts, F, dim3((unsigned)cdiv64(n, HG_BLOCK), Lv), dim3(HG_BLOCK), 0, s, pts, n, table, g_emb, g, part);
    hipLaunchKernelGGL(k_hashgrid_bwd_pts_sum, dim3((unsigned)cdiv64(n, HG_BLOCK)), dim3(HG_BLOCK), 0, s, pts, n, g, (const float *)part, g_pts);
    CTX_CHECK_LAUNCH("hashgrid_bwd_pts");
    return CTX_OK;
}
