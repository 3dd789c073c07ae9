// The texture field as a 2-D hash grid over the unit UV square (instant-ngp's gigapixel-image case): uv -> Lv levels x F trainable
// features, bilinear in each level's grid, and the (tanh + 1) / 2 head that turns the MLP's output into the atlas.
// The rule is tests/hashtex_rule.py; this file is built with -ffp-contract=off and is array_equal to it.
//
//   ctx_hashtex_fwd      : emb[r, l*F + f] = sum over the 4 corners of the row's cell at level l of w_c * table[l, idx_c, f]
//   ctx_hashtex_bwd      : g_table[l, idx_c, f] += w_c * g_emb[r, l*F + f] in the 64-bit integer accumulator of section 4j (bit-reproducible)
//   ctx_texture_head_fwd : tex[c, node] = (tanhf(raw[r, c]) + 1) / 2
//   ctx_texture_head_bwd : grad_raw[r, c] = g_raw_in[r, c] + grad_tex[c, node] * 0.5 * (1 - tanhf(raw[r, c])^2)
//
// A row is a point uv[r], node r of the grid x grid atlas, or node idx[r] of it (a texel list); a node's uv is torch.linspace(0, 1, grid)
// as uvmlp.hip computes it.  Mapping of the encode, forward and backward: one thread per (row, level), blockIdx.y = level, as in
// hashgrid.hip.  In atlas order neighbouring lanes fall into one cell of a coarse level, so the accumulate kernel first adds the terms of
// every run of adjacent lanes that address the same entry (a segmented wave scan; the terms are integers, the sum does not depend on
// its order) and only the run's first lane issues the atomic.  CTX_HASHTEX_PRESUM=0 turns that off.
#include "hashgrid_common.h"

// how the rows are named: uv [n,2], or nodes of the grid x grid atlas (idx null: node = row)
struct HtRows {
    const float *uv;
    const int32_t *idx;
    int grid;
};

static int32_t ht_check(const char *who, const float *uv, const int32_t *idx, int64_t n, int32_t grid, int32_t Lv, int32_t F, int32_t log2T,
                        const int32_t *res, HgTable &g, HtRows &rows)
{
    CTX_REQUIRE(res, "%s: null res", who);
    if (int32_t rc = hg_check_table(who, Lv, F, log2T, res, g)) return rc;
    CTX_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "%s: n=%lld outside [1, 2^31)", who, (long long)n);
    if (uv) {
        CTX_REQUIRE(!idx && grid == 0, "%s: points (uv) exclude a texel list and a grid (idx=%p, grid=%d)", who, (const void *)idx, grid);
    } else {
        CTX_REQUIRE(grid >= 2 && grid <= 46340, "%s: without uv the rows are nodes of a grid x grid atlas, 2 <= grid <= 46340 (grid=%d)", who, grid);
        CTX_REQUIRE(idx || n == (int64_t)grid * grid, "%s: whole atlas: n=%lld is not grid^2=%lld", who, (long long)n, (long long)grid * grid);
    }
    rows.uv = uv; rows.idx = idx; rows.grid = grid;
    return CTX_OK;
}

// The row's point x = (u, v), already unit coordinates.  false: a list entry outside the atlas (a zero row that takes no part in the backward).
__device__ __forceinline__ bool ht_point(const HtRows &rows, int64_t r, float (&x)[2])
{
    if (rows.uv) {
        x[0] = rows.uv[r * 2 + 0];
        x[1] = rows.uv[r * 2 + 1];
        return true;
    }
    const int grid = rows.grid;
    int64_t node = r;
    if (rows.idx) {
        node = rows.idx[r];
        if (node < 0 || node >= (int64_t)grid * grid) return false;
    }
    // torch.linspace(0,1,grid): start + i*step for the first half, end - (grid-1-i)*step after, the latter in one rounding: uvmlp.hip is
    // built with contraction and fuses its `1.0f - (float)(res-1-j) * step`; this file is not, so the fused operation is written out
    const int i = (int)(node / grid), j = (int)(node % grid);
    const float step = 1.0f / (float)(grid - 1);
    x[0] = (j < grid / 2) ? (float)j * step : fmaf(-(float)(grid - 1 - j), step, 1.0f);
    x[1] = (i < grid / 2) ? (float)i * step : fmaf(-(float)(grid - 1 - i), step, 1.0f);
    return true;
}

template <int F>
__global__ __launch_bounds__(HG_BLOCK) void k_hashtex_fwd(HtRows rows, int64_t n, const float *__restrict__ table, HgTable g, float *__restrict__ emb)
{
    typedef typename HgVec<F>::type V;
    const int l = blockIdx.y;
    const int64_t r = (int64_t)blockIdx.x * HG_BLOCK + threadIdx.x;
    if (r >= n) return;
    float o[F];
#pragma unroll
    for (int f = 0; f < F; ++f) o[f] = 0.0f;
    float x[2];
    if (ht_point(rows, r, x)) hg_interpolate<2, F>(hg_axes<2>(x, g.res[l]), g, l, table, o);
    *(V *)(emb + hg_row<F>(r, g, l)) = *(const V *)o;
}

extern "C" int32_t ctx_hashtex_fwd(const float *uv, const int32_t *idx, int64_t n, int32_t grid, const float *table, int32_t Lv, int32_t F,
                                   int32_t log2T, const int32_t *res, float *emb, ctx_stream_t stream)
{
    HgTable g;
    HtRows rows;
    if (int32_t rc = ht_check("hashtex_fwd", uv, idx, n, grid, Lv, F, log2T, res, g, rows)) return rc;
    CTX_REQUIRE(table && emb, "hashtex_fwd: null pointer");
    HG_LAUNCH_F(k_hashtex_fwd, F, dim3((unsigned)cdiv64(n, HG_BLOCK), Lv), dim3(HG_BLOCK), 0, (hipStream_t)stream, rows, n, table, g, emb);
    CTX_CHECK_LAUNCH("hashtex_fwd");
    return CTX_OK;
}

// ---- backward to the table -------------------------------------------------------------------------------------------------------
// max|g_emb| over the rows of a texel list that name a node of the atlas (the other rows take no part); width = Lv*F columns per row
__global__ __launch_bounds__(HG_BLOCK) void k_hashtex_absmax_list(const float *__restrict__ g, int64_t count, int width, const int32_t *__restrict__ idx,
                                                                  int64_t plane, HgCtl *__restrict__ ctl)
{
    uint32_t m = 0;
    const int64_t stride = (int64_t)gridDim.x * HG_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * HG_BLOCK + threadIdx.x; i < count; i += stride) {
        const int64_t node = idx[i / width];
        if (node >= 0 && node < plane) m = max(m, __float_as_uint(g[i]) & 0x7fffffffu);
    }
    hg_absmax_commit(m, ctl);
}

template <int F>
__global__ __launch_bounds__(HG_BLOCK) void k_hashtex_bwd(HtRows rows, int64_t n, const float *__restrict__ g_emb, HgTable g, int E, int presum,
                                                          const HgCtl *__restrict__ ctl, unsigned long long *__restrict__ acc)
{
    typedef typename HgVec<F>::type V;
    if (ctl->status != 0) return;                  // uniform over the grid
    const int l = blockIdx.y;
    const int64_t r = (int64_t)blockIdx.x * HG_BLOCK + threadIdx.x;
    float x[2] = {0.0f, 0.0f};
    const bool live = r < n && ht_point(rows, r, x);        // a lane that is not live stays for the shuffles, with terms of 0 and a key of its own
    float ge[F];
#pragma unroll
    for (int f = 0; f < F; ++f) ge[f] = 0.0f;               // times the finite weights of the point (0, 0): every term of such a lane is 0
    if (live) *(V *)ge = *(const V *)(g_emb + hg_row<F>(r, g, l));
    const int lane = threadIdx.x & 63;
    hg_accumulate<2, F>(hg_cell(hg_axes<2>(x, g.res[l]), g.res[l], g.log2T), ge, hg_pow2(E - ctl->x), acc + ((int64_t)l << g.log2T) * F,
                        [&](uint32_t entry, long long (&q)[F]) {
        return presum ? hg_presum_runs<F>(entry, live, lane, q) : live;          // the segmented wave scan of hashgrid_common.h
    });
}

extern "C" int64_t ctx_hashtex_bwd_ws_bytes(int32_t Lv, int32_t F, int32_t log2T)
{
    return hg_table_bwd_ws_bytes("hashtex_bwd_ws_bytes", Lv, F, log2T);
}

extern "C" int32_t ctx_hashtex_bwd(const float *uv, const int32_t *idx, int64_t n, int32_t grid, const float *g_emb, int32_t Lv, int32_t F,
                                   int32_t log2T, const int32_t *res, int32_t stages, void *ws, float *g_table, ctx_stream_t stream)
{
    HgTable g;
    HtRows rows;
    if (int32_t rc = ht_check("hashtex_bwd", uv, idx, n, grid, Lv, F, log2T, res, g, rows)) return rc;
    CTX_REQUIRE(g_emb && ws && g_table, "hashtex_bwd: null pointer");
    const int presum = ctx_env_int("CTX_HASHTEX_PRESUM", 1) != 0;   // read per call: a tool times both forms in one process
    hipStream_t s = (hipStream_t)stream;
    return hg_table_bwd<2>(
        "hashtex_bwd", n, g, F, stages, ws, g_table, s,
        [&](dim3 blocks, HgCtl *ctl) {
            if (idx) hipLaunchKernelGGL(k_hashtex_absmax_list, blocks, dim3(HG_BLOCK), 0, s, g_emb, n * Lv * F, Lv * F, idx, (int64_t)grid * grid, ctl);
            else hipLaunchKernelGGL(k_hashgrid_absmax, blocks, dim3(HG_BLOCK), 0, s, g_emb, n * Lv * F, ctl);
        },
        [&](dim3 blocks, int E, const HgCtl *ctl, unsigned long long *acc) {
            HG_LAUNCH_F(k_hashtex_bwd, F, blocks, dim3(HG_BLOCK), 0, s, rows, n, g_emb, g, E, presum, ctl, acc);
        });
}

// ---- the head: raw -> atlas ----------------------------------------------------------------------------------------------------------
// node of row r: r itself, or idx[r]; -1 for a list entry outside the plane (nothing is written or read for it)
__device__ __forceinline__ int64_t ht_node(const int32_t *__restrict__ idx, int64_t r, int64_t plane)
{
    if (!idx) return r;
    const int64_t node = idx[r];
    return node >= 0 && node < plane ? node : -1;
}

__global__ __launch_bounds__(HG_BLOCK) void k_texture_head_fwd(const float *__restrict__ raw, const int32_t *__restrict__ idx, int64_t n, int64_t plane,
                                                               int C, float *__restrict__ tex)
{
    const int64_t r = (int64_t)blockIdx.x * HG_BLOCK + threadIdx.x;
    if (r >= n) return;
    const int64_t node = ht_node(idx, r, plane);
    if (node < 0) return;
    for (int c = 0; c < C; ++c) tex[(int64_t)c * plane + node] = (tanhf(raw[r * C + c]) + 1.0f) / 2.0f;
}

__global__ __launch_bounds__(HG_BLOCK) void k_texture_head_bwd(const float *__restrict__ grad_tex, const float *__restrict__ g_raw_in,
                                                               const float *__restrict__ raw, const int32_t *__restrict__ idx, int64_t n, int64_t plane,
                                                               int C, float *__restrict__ grad_raw)
{
    const int64_t r = (int64_t)blockIdx.x * HG_BLOCK + threadIdx.x;
    if (r >= n) return;
    const int64_t node = ht_node(idx, r, plane);
    for (int c = 0; c < C; ++c) {
        float v = g_raw_in ? g_raw_in[r * C + c] : 0.0f;
        if (node >= 0) {
            const float y = tanhf(raw[r * C + c]);
            v += grad_tex[(int64_t)c * plane + node] * 0.5f * (1.0f - y * y);
        }
        grad_raw[r * C + c] = v;
    }
}

static int32_t head_check(const char *who, const int32_t *idx, int64_t n, int64_t plane, int32_t C)
{
    CTX_REQUIRE(C >= 1 && C <= 4, "%s: C=%d outside [1, 4]", who, C);
    CTX_REQUIRE(plane >= 1 && plane < ((int64_t)1 << 31), "%s: plane=%lld outside [1, 2^31)", who, (long long)plane);
    CTX_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "%s: n=%lld outside [1, 2^31)", who, (long long)n);
    CTX_REQUIRE(idx || n == plane, "%s: without a texel list every node is a row: n=%lld, plane=%lld", who, (long long)n, (long long)plane);
    return CTX_OK;
}

extern "C" int32_t ctx_texture_head_fwd(const float *raw, const int32_t *idx, int64_t n, int64_t plane, int32_t C, float *tex_chw,
                                        ctx_stream_t stream)
{
    if (int32_t rc = head_check("texture_head_fwd", idx, n, plane, C)) return rc;
    CTX_REQUIRE(raw && tex_chw, "texture_head_fwd: null pointer");
    hipLaunchKernelGGL(k_texture_head_fwd, dim3((unsigned)cdiv64(n, HG_BLOCK)), dim3(HG_BLOCK), 0, (hipStream_t)stream, raw, idx, n, plane, C, tex_chw);
    CTX_CHECK_LAUNCH("texture_head_fwd");
    return CTX_OK;
}

extern "C" int32_t ctx_texture_head_bwd(const float *grad_tex, const float *g_raw_in, const float *raw, const int32_t *idx, int64_t n,
                                        int64_t plane, int32_t C, float *grad_raw, ctx_stream_t stream)
{
    if (int32_t rc = head_check("texture_head_bwd", idx, n, plane, C)) return rc;
    CTX_REQUIRE(grad_tex && raw && grad_raw, "texture_head_bwd: null pointer");
    hipLaunchKernelGGL(k_texture_head_bwd, dim3((unsigned)cdiv64(n, HG_BLOCK)), dim3(HG_BLOCK), 0, (hipStream_t)stream, grad_tex, g_raw_in, raw, idx,
                       n, plane, C, grad_raw);
    CTX_CHECK_LAUNCH("texture_head_bwd");
    return CTX_OK;
}
