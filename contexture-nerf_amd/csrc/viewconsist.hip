// Multi-view consistency (src/training/trainer.py:429-531, the reward of :856-863 that upstream switched off): how well the V
// rendered views agree where they show the same surface, as ONE number with a gradient with respect to the views.
//
//   vertex k is SEEN in view j      when it is a corner of a face that owns at least one pixel of face_idx[j].
//   pair (source j, target i, y, x) f = face_idx[i, y, x] >= 0, j != i, c = the first corner of faces[f] seen in j (none: no pair);
//                                   (X, Y) = face_vertices_image[j, f, c]; sx = trunc(((X + 1) / 2) * w);
//                                   sy = trunc(((Y + 1) / 2) * h) (rows = 0, upstream's rows) | trunc(((1 - Y) / 2) * h) (rows = 1, the
//                                   raster's rows: row 0 at Y = +1).  (sy, sx) outside the image: not gathered, counted in n_outside.
//   d = 1 - (|t0 - s0| + |t1 - s1| + ...) / C   f32, left to right, no contraction, IEEE division; the pair counts when d >= 0.
//   pair_sum[j, i] += floor(d * 2^32), pair_count[j, i] += 1; mean = sum(pair_sum) / 2^32 / sum(pair_count) in f64, rounded to f32 once.
//   backward: sign_count[i, c, y, x] -= sign(t_c - s_c), sign_count[j, c, sy, sx] += sign(t_c - s_c) per counted pair (int32);
//             grad_views = float(sign_count) * (u * g), u = (1 / float(N)) / C, N = sum(pair_count).
//
// Every sum is an integer sum (as uvscatter.hip's fixed mode), so no result depends on grid, block order or stream.
//   k_vc_seen   one thread per pixel of every view: plain byte stores of 1 into seen [V, n_vertices].
//   k_vc_pairs  one thread per target pixel (blockIdx.y = target view), a loop over the sources.  Forward: per source the wave adds its
//               counts by ballot and its sums by shuffles, lane 0 adds them to the block's LDS cells, and after the barrier one 64-bit
//               global atomic goes out per non-empty cell.  Backward: the target's signs are summed in registers and added once;
//               source signs go out as 32-bit integer atomics.
//   k_vc_mean / k_vc_scale   the one f64 division; the elementwise scaling of sign_count into grad_views.
#include "common.h"

#define VC_MAXV 16
#define VC_MAXC 4
#define VC_BLOCK 256

__global__ __launch_bounds__(VC_BLOCK) void k_vc_seen(const int64_t *faces, const int64_t *face_idx, int V, int64_t HW, int F, int nV, unsigned char *seen)
{
    const int64_t p = (int64_t)blockIdx.x * VC_BLOCK + threadIdx.x;
    const int j = blockIdx.y;
    if (p >= HW) return;
    const int64_t f = face_idx[(int64_t)j * HW + p];
    if (f < 0 || f >= F) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int64_t v = faces[f * 3 + c];
        if (v >= 0 && v < nV) seen[(int64_t)j * nV + v] = 1;
    }
}

__device__ __forceinline__ unsigned long long vc_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// image coordinate in [-1, 1] -> pixel index; false when it falls outside [0, n).  trunc(a) is in [0, n-1] exactly when -1 < a < n.
__device__ __forceinline__ bool vc_pixel(float coord01, int n, int *out)
{
    const float a = coord01 * (float)n;
    const bool in = a > -1.0f && a < (float)n;
    *out = in ? (int)a : 0;
    return in;
}

template <bool BWD>
__global__ __launch_bounds__(VC_BLOCK) void k_vc_pairs(const float *views, const int64_t *faces, const int64_t *face_idx, const float *fvi,
                                                       const unsigned char *seen, int V, int C, int h, int w, int F, int nV, int rows,
                                                       unsigned long long *pair_sum, unsigned long long *pair_count, unsigned long long *n_outside,
                                                       int *sign_count)
{
    __shared__ unsigned long long s_sum[VC_MAXV], s_cnt[VC_MAXV];
    __shared__ unsigned int s_out;
    const int64_t HW = (int64_t)h * w;
    const int64_t p = (int64_t)blockIdx.x * VC_BLOCK + threadIdx.x;
    const int i = blockIdx.y;
    const int lane = threadIdx.x & 63;
    if (!BWD) {
        if (threadIdx.x < VC_MAXV) { s_sum[threadIdx.x] = 0; s_cnt[threadIdx.x] = 0; }
        if (threadIdx.x == 0) s_out = 0;
        __syncthreads();
    }
    int64_t f = -1;
    if (p < HW) {
        f = face_idx[(int64_t)i * HW + p];
        if (f >= F) f = -1;
    }
    const bool fg = f >= 0;
    int64_t vid[3] = {-1, -1, -1};
    float t[VC_MAXC] = {0.f, 0.f, 0.f, 0.f};
    if (fg) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int64_t v = faces[f * 3 + c];
            vid[c] = (v >= 0 && v < nV) ? v : -1;
        }
#pragma unroll
        for (int c = 0; c < VC_MAXC; ++c)
            if (c < C) t[c] = views[((int64_t)i * C + c) * HW + p];
    }
    const float fC = (float)C;
    int acc[VC_MAXC] = {0, 0, 0, 0};
    for (int j = 0; j < V; ++j) {                       // uniform over the block: every lane takes part in the wave sums
        if (j == i) continue;
        bool pair = false, outside = false;
        unsigned long long q = 0;
        if (fg) {
            const unsigned char *sj = seen + (int64_t)j * nV;
            int corner = -1;
            if (vid[0] >= 0 && sj[vid[0]]) corner = 0;
            else if (vid[1] >= 0 && sj[vid[1]]) corner = 1;
            else if (vid[2] >= 0 && sj[vid[2]]) corner = 2;
            if (corner >= 0) {
                const float2 xy = *(const float2 *)(fvi + (((int64_t)j * F + f) * 3 + corner) * 2);
                int sx, sy;
                const bool inx = vc_pixel((xy.x + 1.0f) / 2.0f, w, &sx);
                const bool iny = vc_pixel((rows == 0 ? (xy.y + 1.0f) : (1.0f - xy.y)) / 2.0f, h, &sy);
                if (inx && iny) {
                    const int64_t sp = (int64_t)sy * w + sx;
                    float s[VC_MAXC] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int c = 0; c < VC_MAXC; ++c)
                        if (c < C) s[c] = views[((int64_t)j * C + c) * HW + sp];
                    float a = fabsf(t[0] - s[0]);
#pragma unroll
                    for (int c = 1; c < VC_MAXC; ++c)
                        if (c < C) a = a + fabsf(t[c] - s[c]);
                    const float d = 1.0f - a / fC;
                    pair = d >= 0.0f;
                    if (pair) {
                        if (BWD) {
#pragma unroll
                            for (int c = 0; c < VC_MAXC; ++c) {
                                if (c < C) {
                                    const int sg = (t[c] > s[c]) - (t[c] < s[c]);
                                    acc[c] -= sg;
                                    if (sg != 0) atomicAdd(sign_count + ((int64_t)j * C + c) * HW + sp, sg);
                                }
                            }
                        } else {
                            q = (unsigned long long)((double)d * 4294967296.0);      // d in [0, 1]: exact in f64, truncation = floor
                        }
                    }
                } else {
                    outside = true;
                }
            }
        }
        if (!BWD) {
            const unsigned long long mp = __ballot(pair), mo = __ballot(outside);
            if (mp) {
                const unsigned long long ws = vc_wave_sum(q);
                if (lane == 0) {
                    atomicAdd(&s_sum[j], ws);
                    atomicAdd(&s_cnt[j], (unsigned long long)__popcll(mp));
                }
            }
            if (mo && lane == 0) atomicAdd(&s_out, (unsigned int)__popcll(mo));
        }
    }
    if (BWD) {
        if (fg) {
#pragma unroll
            for (int c = 0; c < VC_MAXC; ++c)
                if (c < C && acc[c] != 0) atomicAdd(sign_count + ((int64_t)i * C + c) * HW + p, acc[c]);
        }
    } else {
        __syncthreads();
        if (threadIdx.x < V && s_cnt[threadIdx.x]) {
            atomicAdd(pair_sum + threadIdx.x * V + i, s_sum[threadIdx.x]);
            atomicAdd(pair_count + threadIdx.x * V + i, s_cnt[threadIdx.x]);
        }
        if (threadIdx.x == 64 && s_out) atomicAdd(n_outside, (unsigned long long)s_out);
    }
}

__global__ void k_vc_mean(const int64_t *pair_sum, const int64_t *pair_count, int VV, float *mean)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int64_t S = 0, N = 0;
    for (int k = 0; k < VV; ++k) { S += pair_sum[k]; N += pair_count[k]; }
    *mean = N > 0 ? (float)((double)S / 4294967296.0 / (double)N) : 0.0f;
}

__global__ __launch_bounds__(VC_BLOCK) void k_vc_scale(const int *sign_count, int64_t n, const int64_t *pair_count, int VV, int C, const float *g, float *grad)
{
    int64_t N = 0;
    for (int k = 0; k < VV; ++k) N += pair_count[k];
    const float u = N > 0 ? (1.0f / (float)N) / (float)C : 0.0f;
    const float ug = u * g[0];
    const int64_t stride = (int64_t)gridDim.x * VC_BLOCK;
    for (int64_t e = (int64_t)blockIdx.x * VC_BLOCK + threadIdx.x; e < n; e += stride) grad[e] = (float)sign_count[e] * ug;
}

extern "C" int64_t ctx_view_consistency_ws_bytes(int32_t V, int32_t n_vertices)
{
    if (V < 1 || V > VC_MAXV || n_vertices < 1) return -1;
    return (int64_t)V * n_vertices;
}

static int vc_check(const char *who, int V, int C, int h, int w, int F, int nV, int rows)
{
    CTX_REQUIRE(V >= 1 && V <= VC_MAXV, "%s: V=%d outside [1, %d]", who, V, VC_MAXV);
    CTX_REQUIRE(C >= 1 && C <= VC_MAXC, "%s: C=%d outside [1, %d]", who, C, VC_MAXC);
    CTX_REQUIRE(rows == 0 || rows == 1, "%s: rows=%d, expected 0 (reference) or 1 (image)", who, rows);
    CTX_REQUIRE(h >= 1 && w >= 1 && F >= 1 && nV >= 1, "%s: h=%d w=%d F=%d n_vertices=%d must be positive", who, h, w, F, nV);
    CTX_REQUIRE(cdiv64((int64_t)h * w, VC_BLOCK) <= 0x7fffffff, "%s: %d x %d pixels do not fit one grid", who, h, w);
    return CTX_OK;
}

extern "C" int32_t ctx_view_consistency_fwd(const float *views, const int64_t *faces, const int64_t *face_idx, const float *face_vertices_image,
                                            int32_t V, int32_t C, int32_t h, int32_t w, int32_t F, int32_t n_vertices, int32_t rows, int32_t build_seen,
                                            uint8_t *seen, int64_t seen_bytes, int64_t *pair_sum, int64_t *pair_count, int64_t *n_outside, float *mean,
                                            ctx_stream_t stream)
{
    CTX_REQUIRE(views && faces && face_idx && face_vertices_image && seen && pair_sum && pair_count && n_outside && mean, "view_consistency_fwd: bad args");
    if (int rc = vc_check("view_consistency_fwd", V, C, h, w, F, n_vertices, rows)) return rc;
    CTX_REQUIRE(seen_bytes >= ctx_view_consistency_ws_bytes(V, n_vertices), "view_consistency_fwd: seen map of %lld bytes, ctx_view_consistency_ws_bytes(%d, %d) = %lld",
                (long long)seen_bytes, V, n_vertices, (long long)ctx_view_consistency_ws_bytes(V, n_vertices));
    hipStream_t s = (hipStream_t)stream;
    const int64_t HW = (int64_t)h * w;
    const dim3 grid((unsigned)cdiv64(HW, VC_BLOCK), V);
    if (build_seen) {
        if (hipMemsetAsync(seen, 0, (size_t)V * n_vertices, s) != hipSuccess) { ctx_set_error("view_consistency_fwd: memset failed"); return CTX_E_LAUNCH; }
        hipLaunchKernelGGL(k_vc_seen, grid, dim3(VC_BLOCK), 0, s, faces, face_idx, V, HW, F, n_vertices, seen);
    }
    if (hipMemsetAsync(pair_sum, 0, sizeof(int64_t) * V * V, s) != hipSuccess || hipMemsetAsync(pair_count, 0, sizeof(int64_t) * V * V, s) != hipSuccess ||
        hipMemsetAsync(n_outside, 0, sizeof(int64_t), s) != hipSuccess) {
        ctx_set_error("view_consistency_fwd: memset failed");
        return CTX_E_LAUNCH;
    }
    hipLaunchKernelGGL(k_vc_pairs<false>, grid, dim3(VC_BLOCK), 0, s, views, faces, face_idx, face_vertices_image, seen, V, C, h, w, F, n_vertices, rows,
                       (unsigned long long *)pair_sum, (unsigned long long *)pair_count, (unsigned long long *)n_outside, (int *)nullptr);
    hipLaunchKernelGGL(k_vc_mean, dim3(1), dim3(64), 0, s, pair_sum, pair_count, V * V, mean);
    CTX_CHECK_LAUNCH("view_consistency_fwd");
    return CTX_OK;
}

extern "C" int32_t ctx_view_consistency_bwd(const float *views, const int64_t *faces, const int64_t *face_idx, const float *face_vertices_image,
                                            const uint8_t *seen, int32_t V, int32_t C, int32_t h, int32_t w, int32_t F, int32_t n_vertices, int32_t rows,
                                            const int64_t *pair_count, const float *grad_mean, int32_t *sign_count, float *grad_views, ctx_stream_t stream)
{
    CTX_REQUIRE(views && faces && face_idx && face_vertices_image && seen && pair_count && grad_mean && sign_count && grad_views, "view_consistency_bwd: bad args");
    if (int rc = vc_check("view_consistency_bwd", V, C, h, w, F, n_vertices, rows)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int64_t HW = (int64_t)h * w, n = (int64_t)V * C * HW;
    if (hipMemsetAsync(sign_count, 0, sizeof(int32_t) * (size_t)n, s) != hipSuccess) { ctx_set_error("view_consistency_bwd: memset failed"); return CTX_E_LAUNCH; }
    hipLaunchKernelGGL(k_vc_pairs<true>, dim3((unsigned)cdiv64(HW, VC_BLOCK), V), dim3(VC_BLOCK), 0, s, views, faces, face_idx, face_vertices_image, seen, V, C, h, w, F,
                       n_vertices, rows, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (unsigned long long *)nullptr, sign_count);
    hipLaunchKernelGGL(k_vc_scale, dim3((unsigned)(cdiv64(n, VC_BLOCK) < 2048 ? cdiv64(n, VC_BLOCK) : 2048)), dim3(VC_BLOCK), 0, s, sign_count, n, pair_count, V * V, C, grad_mean, grad_views);
    CTX_CHECK_LAUNCH("view_consistency_bwd");
    return CTX_OK;
}
