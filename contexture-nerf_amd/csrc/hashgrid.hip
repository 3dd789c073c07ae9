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

struct HgGrid {
    float lo[3], hi[3];
    int res[HG_MAX_LEVELS];
    int Lv, log2T;
};

// what every entry point accepts
static int32_t hg_check(const char *who, int32_t Lv, int32_t F, int32_t log2T, const int32_t *res, const float *lo, const float *hi, HgGrid &g)
{
    CTX_REQUIRE(res && lo && hi, "%s: null res / lo / hi", who);
    CTX_REQUIRE(Lv >= 1 && Lv <= HG_MAX_LEVELS, "%s: Lv=%d outside [1, %d]", who, Lv, HG_MAX_LEVELS);
    CTX_REQUIRE(F == 1 || F == 2 || F == 4, "%s: F=%d (1, 2 or 4 features per entry)", who, F);
    CTX_REQUIRE(Lv * F <= 64, "%s: Lv*F=%d above 64, the width of the field's embedding", who, Lv * F);
    CTX_REQUIRE(log2T >= 4 && log2T <= 22, "%s: log2T=%d outside [4, 22]", who, log2T);
    for (int a = 0; a < 3; ++a) {
        CTX_REQUIRE(isfinite(lo[a]) && isfinite(hi[a]) && lo[a] < hi[a], "%s: box axis %d: want finite lo < hi (lo=%g hi=%g)", who, a, lo[a], hi[a]);
        g.lo[a] = lo[a]; g.hi[a] = hi[a];
    }
    for (int l = 0; l < Lv; ++l) {
        CTX_REQUIRE(res[l] >= 1 && res[l] <= (1 << 20), "%s: res[%d]=%d outside [1, 2^20]", who, l, res[l]);
        g.res[l] = res[l];
    }
    g.Lv = Lv; g.log2T = log2T;
    return CTX_OK;
}

// A point on one level, axis by axis: cell i, weight w inside it, and whether the axis is active, i.e. strictly inside the box before the
// clamp (x > 0 && x < 1: false for NaN, +-inf and the faces).  NaN clamps to 0, so every index is in range.
struct HgAxes { int i[3]; float w[3]; bool active[3]; };
__device__ __forceinline__ HgAxes hg_axes(const float *__restrict__ pts, int64_t n, const HgGrid &g, int l)
{
    const int res = g.res[l];
    HgAxes ax;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float x = (pts[n * 3 + a] - g.lo[a]) / (g.hi[a] - g.lo[a]);
        ax.active[a] = x > 0.0f && x < 1.0f;
        x = fminf(fmaxf(x, 0.0f), 1.0f);
        const float pos = x * (float)res;
        ax.i[a] = min((int)floorf(pos), res - 1);
        ax.w[a] = pos - (float)ax.i[a];
    }
    return ax;
}

// A point's cell at one level: entry index and weight of the 8 corners, c = cx + 2 cy + 4 cz.
struct HgCell { uint32_t idx[8]; float w[8]; };
__device__ __forceinline__ HgCell hg_cell(const HgAxes &ax, const HgGrid &g, int l)
{
    const int res = g.res[l];
    const uint32_t T = 1u << g.log2T;
    const int64_t side = (int64_t)res + 1;
    const bool dense = side * side * side <= (int64_t)T;
    HgCell c;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int bx = k & 1, by = (k >> 1) & 1, bz = (k >> 2) & 1;
        const uint32_t gx = (uint32_t)(ax.i[0] + bx), gy = (uint32_t)(ax.i[1] + by), gz = (uint32_t)(ax.i[2] + bz);
        c.idx[k] = dense ? gx + (uint32_t)side * (gy + (uint32_t)side * gz) : ((gx ^ (gy * 2654435761u) ^ (gz * 805459861u)) & (T - 1));
        const float sx = bx ? ax.w[0] : 1.0f - ax.w[0], sy = by ? ax.w[1] : 1.0f - ax.w[1], sz = bz ? ax.w[2] : 1.0f - ax.w[2];
        c.w[k] = (sx * sy) * sz;
    }
    return c;
}
__device__ __forceinline__ HgCell hg_cell(const float *__restrict__ pts, int64_t n, const HgGrid &g, int l)
{
    return hg_cell(hg_axes(pts, n, g, l), g, l);
}

template <int F>
__global__ __launch_bounds__(HG_BLOCK) void k_hashgrid_fwd(const float *__restrict__ pts, int64_t n, const float *__restrict__ table, HgGrid g,
                                                           float *__restrict__ emb)
{
    typedef typename HgVec<F>::type V;
    const int l = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * HG_BLOCK + threadIdx.x;
    if (p >= n) return;
    const HgCell c = hg_cell(pts, p, g, l);
    const float *tl = table + ((int64_t)l << g.log2T) * F;
    float t[8][F];
#pragma unroll
    for (int k = 0; k < 8; ++k) *(V *)t[k] = *(const V *)(tl + (int64_t)c.idx[k] * F);   // the 8 gathers in flight together
    float o[F];
#pragma unroll
    for (int f = 0; f < F; ++f) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) s = s + c.w[k] * t[k][f];
        o[f] = s;
    }
    *(V *)(emb + p * ((int64_t)g.Lv * F) + l * F) = *(const V *)o;
}

extern "C" int32_t ctx_hashgrid_fwd(const float *pts, int64_t n, const float *table, int32_t Lv, int32_t F, int32_t log2T, const int32_t *res,
                                    const float *lo, const float *hi, float *emb, ctx_stream_t stream)
{
    HgGrid g;
    if (int32_t rc = hg_check("hashgrid_fwd", Lv, F, log2T, res, lo, hi, g)) return rc;
    CTX_REQUIRE(pts && table && emb, "hashgrid_fwd: null pointer");
    CTX_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "hashgrid_fwd: n=%lld outside [1, 2^31)", (long long)n);
    const dim3 grid((unsigned)cdiv64(n, HG_BLOCK), Lv);
    hipStream_t s = (hipStream_t)stream;
    if (F == 1) hipLaunchKernelGGL(k_hashgrid_fwd<1>, grid, dim3(HG_BLOCK), 0, s, pts, n, table, g, emb);
    else if (F == 2) hipLaunchKernelGGL(k_hashgrid_fwd<2>, grid, dim3(HG_BLOCK), 0, s, pts, n, table, g, emb);
    else hipLaunchKernelGGL(k_hashgrid_fwd<4>, grid, dim3(HG_BLOCK), 0, s, pts, n, table, g, emb);
    CTX_CHECK_LAUNCH("hashgrid_fwd");
    return CTX_OK;
}

// ---- backward to the table -------------------------------------------------------------------------------------------------------
// HgCtl, the absmax / scale / convert kernels and hg_pow2 are in hashgrid_common.h: the 2-D texture field (hashtex.hip) uses them too
template <int F>
__global__ __launch_bounds__(HG_BLOCK) void k_hashgrid_bwd(const float *__restrict__ pts, int64_t n, const float *__restrict__ g_emb, HgGrid g, int E,
                                                           const HgCtl *__restrict__ ctl, unsigned long long *__restrict__ acc)
{
    typedef typename HgVec<F>::type V;
    if (ctl->status != 0) return;
    const int l = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * HG_BLOCK + threadIdx.x;
    if (p >= n) return;
    const double scale = hg_pow2(E - ctl->x);
    float ge[F];
    *(V *)ge = *(const V *)(g_emb + p * ((int64_t)g.Lv * F) + l * F);
    const HgCell c = hg_cell(pts, p, g, l);
    unsigned long long *al = acc + ((int64_t)l << g.log2T) * F;
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const float prod = c.w[k] * ge[f];                                  // one rounding
            const long long q = __double2ll_rn((double)prod * scale);           // |prod| < 2^x: |q| <= 2^E, exact scaling, nearest even
            if (q) atomicAdd(al + (int64_t)c.idx[k] * F + f, (unsigned long long)q);
        }
}

extern "C" int64_t ctx_hashgrid_bwd_ws_bytes(int32_t Lv, int32_t F, int32_t log2T)
{
    if (Lv < 1 || Lv > HG_MAX_LEVELS || !(F == 1 || F == 2 || F == 4) || Lv * F > 64 || log2T < 4 || log2T > 22) return -1;
    return hg_align(((int64_t)Lv << log2T) * F * 8) + 256;      // the int64 accumulator [Lv, T, F], then the control words
}

extern "C" int32_t ctx_hashgrid_bwd(const float *pts, int64_t n, const float *g_emb, int32_t Lv, int32_t F, int32_t log2T, const int32_t *res,
                                    const float *lo, const float *hi, int32_t stages, void *ws, float *g_table, ctx_stream_t stream)
{
    HgGrid g;
    if (int32_t rc = hg_check("hashgrid_bwd", Lv, F, log2T, res, lo, hi, g)) return rc;
    CTX_REQUIRE(pts && g_emb && ws && g_table, "hashgrid_bwd: null pointer");
    CTX_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "hashgrid_bwd: n=%lld outside [1, 2^31)", (long long)n);
    CTX_REQUIRE(stages >= 1 && stages <= 7, "hashgrid_bwd: stages=%d (bits: 1 zero, 2 accumulate, 4 convert; 7 is the backward)", stages);
    const int64_t count = ((int64_t)Lv << log2T) * F;
    unsigned long long *acc = (unsigned long long *)ws;
    HgCtl *ctl = (HgCtl *)((char *)ws + hg_align(count * 8));
    const int E = hg_acc_exponent(n, 8);
    hipStream_t s = (hipStream_t)stream;
    if (stages & 1) {
        (void)hipMemsetAsync(acc, 0, count * 8, s);
        (void)hipMemsetAsync(ctl, 0, sizeof(HgCtl), s);
    }
    if (stages & 2) {
        hipLaunchKernelGGL(k_hashgrid_absmax, dim3(capped_blocks(n * Lv * F, HG_BLOCK * 4, 1024)), dim3(HG_BLOCK), 0, s, g_emb, n * Lv * F, ctl);
        hipLaunchKernelGGL(k_hashgrid_scale, dim3(1), dim3(1), 0, s, ctl);
        const dim3 grid((unsigned)cdiv64(n, HG_BLOCK), Lv);
        if (F == 1) hipLaunchKernelGGL(k_hashgrid_bwd<1>, grid, dim3(HG_BLOCK), 0, s, pts, n, g_emb, g, E, ctl, acc);
        else if (F == 2) hipLaunchKernelGGL(k_hashgrid_bwd<2>, grid, dim3(HG_BLOCK), 0, s, pts, n, g_emb, g, E, ctl, acc);
        else hipLaunchKernelGGL(k_hashgrid_bwd<4>, grid, dim3(HG_BLOCK), 0, s, pts, n, g_emb, g, E, ctl, acc);
    }
    if (stages & 4)
        hipLaunchKernelGGL(k_hashgrid_convert, dim3(capped_blocks(count, HG_BLOCK * 4, 4096)), dim3(HG_BLOCK), 0, s, (const long long *)acc, count, E,
                           ctl, g_table);
    CTX_CHECK_LAUNCH("hashgrid_bwd");
    return CTX_OK;
}

// ---- backward to the positions ---------------------------------------------------------------------------------------------------
// One level's three partials gl_a * s_a of a point.  d_a[f] = d emb[f] / d w_a: per corner, ascending, the product of the two other
// axes' factors times the entry, added where the corner's bit on axis a is set and subtracted where it is not.
template <int F>
__device__ __forceinline__ void hg_level_grad(const float *__restrict__ pts, int64_t p, const float *__restrict__ table,
                                              const float *__restrict__ g_emb, const HgGrid &g, int l, float out[3])
{
    typedef typename HgVec<F>::type V;
    const HgAxes ax = hg_axes(pts, p, g, l);
    const HgCell c = hg_cell(ax, g, l);
    const float *tl = table + ((int64_t)l << g.log2T) * F;
    float t[8][F];
#pragma unroll
    for (int k = 0; k < 8; ++k) *(V *)t[k] = *(const V *)(tl + (int64_t)c.idx[k] * F);   // the 8 gathers in flight together
    float ge[F];
    *(V *)ge = *(const V *)(g_emb + p * ((int64_t)g.Lv * F) + l * F);
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
    const HgAxes ax = hg_axes(pts, p, g, 0);                                              // the active flags do not depend on the level
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
    const HgAxes ax = hg_axes(pts, p, g, 0);
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
        const dim3 grid1((unsigned)cdiv64(n, HG_BLOCK));
        if (F == 1) hipLaunchKernelGGL(k_hashgrid_bwd_pts_loop<1>, grid1, dim3(HG_BLOCK), 0, s, pts, n, table, g_emb, g, g_pts);
        else if (F == 2) hipLaunchKernelGGL(k_hashgrid_bwd_pts_loop<2>, grid1, dim3(HG_BLOCK), 0, s, pts, n, table, g_emb, g, g_pts);
        else hipLaunchKernelGGL(k_hashgrid_bwd_pts_loop<4>, grid1, dim3(HG_BLOCK), 0, s, pts, n, table, g_emb, g, g_pts);
        CTX_CHECK_LAUNCH("hashgrid_bwd_pts");
        return CTX_OK;
    }
    const dim3 grid((unsigned)cdiv64(n, HG_BLOCK), Lv);
    if (F == 1) hipLaunchKernelGGL(k_hashgrid_bwd_pts<1>, grid, dim3(HG_BLOCK), 0, s, pts, n, table, g_emb, g, part);
    else if (F == 2) hipLaunchKernelGGL(k_hashgrid_bwd_pts<2>, grid, dim3(HG_BLOCK), 0, s, pts, n, table, g_emb, g, part);
    else hipLaunchKernelGGL(k_hashgrid_bwd_pts<4>, grid, dim3(HG_BLOCK), 0, s, pts, n, table, g_emb, g, part);
    hipLaunchKernelGGL(k_hashgrid_bwd_pts_sum, dim3((unsigned)cdiv64(n, HG_BLOCK)), dim3(HG_BLOCK), 0, s, pts, n, g, (const float *)part, g_pts);
    CTX_CHECK_LAUNCH("hashgrid_bwd_pts");
    return CTX_OK;
}
