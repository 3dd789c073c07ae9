// Exposure compensation across painted views (Brown & Lowe 2007, gain compensation): the pair statistics the per-view gains are solved from.
//
//   atlases [V,4,Tc,Tc] int64: per view the weighted colour sums (channels 0..2) and the weight sum (channel 3) of a low-resolution
//   back-projection, in units of 2^-32 (what ctx_uv_scatter_fixed leaves).  Per texel p, view v, channel ch:
//     w = A[v,3,p];  c = float32(float64(A[v,ch,p]) / float64(w))              one f64 division, one rounding to f32
//     v is VALID at p when w > 0 and lo <= c <= hi on all three channels          (black and saturated texels follow no gain model)
//     q = int64(rintf(c * 2^24))                                                  c * 2^24 is exact; rintf rounds half to even; q <= 2^24
//   For every ordered pair (i, j), i == j included, with both views valid at p:  count[i,j] += 1, colour_sum[i,j,ch] += q_i[ch].
//   colour_sum[i,j] is view i's colour summed over its overlap with view j; the diagonal holds each view's own valid texels.
//   tests/exposure_rule.py states the same in numpy; the kernel equals it bit for bit.
//
// Every sum is an integer sum (as viewconsist.hip, uvscatter.hip's fixed mode): no result depends on grid, texel order or stream, and
// every rank of a job computes the same statistics from the same all-reduced atlases.
//   k_view_pair_stats  one lane per texel, a wave walks the atlas in steps of the grid.  The lane keeps its texel's validity bits of all
//                      views; per view i the wave forms q_i once, and per j the ballot of (valid_i & valid_j) gives the count by popcount
//                      and three DPP wave sums give the colour sums (a wave sum of 64 values <= 2^24 fits 32 bits).  Lanes 0..3 add the
//                      four wave totals to the block's LDS cells (64-bit), and after the barrier one 64-bit global atomic goes out per
//                      non-empty cell.  No float atomics.
#include "common.h"

#define VG_MAXV 16
#define VG_BLOCK 256
#define VG_MAX_BLOCKS 1024
#define VG_MAX_TC 4096

// sum over the 64 lanes of a wave, in every lane (the DPP pattern of common.h's wave_sum_dpp, on integers: any order gives the same bits)
__device__ __forceinline__ unsigned vg_wave_sum(unsigned x)
{
    int v = (int)x;
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, true);    // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, true);    // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, true);   // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, true);   // row_mirror
    return (unsigned)(__builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16)) +
           (unsigned)(__builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48));
}

// colour of view v at texel p and whether the view is valid there
__device__ __forceinline__ bool vg_colour(const int64_t *A, int v, int64_t P, int64_t p, bool in, float lo, float hi, float c[3])
{
    c[0] = c[1] = c[2] = 0.0f;
    if (!in) return false;
    const int64_t *a = A + (int64_t)v * 4 * P + p;
    const int64_t w = a[3 * P];
    if (w <= 0) return false;
    const double dw = (double)w;
    bool ok = true;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        c[ch] = (float)((double)a[ch * P] / dw);
        ok = ok && c[ch] >= lo && c[ch] <= hi;
    }
    return ok;
}

__global__ __launch_bounds__(VG_BLOCK) void k_view_pair_stats(const int64_t *A, int V, int64_t P, float lo, float hi, unsigned long long *count,
                                                              unsigned long long *colour_sum)
{
    __shared__ unsigned long long s_acc[VG_MAXV * VG_MAXV * 4];      // per pair: count, colour sums of the three channels
    const int cells = V * V * 4;
    for (int k = threadIdx.x; k < cells; k += VG_BLOCK) s_acc[k] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * VG_BLOCK;
    // `base` is uniform over the wave: every lane takes part in the ballots and the wave sums, a lane past the end holds no valid view
    for (int64_t base = (int64_t)blockIdx.x * VG_BLOCK + (threadIdx.x & ~63); base < P; base += stride) {
        const int64_t p = base + lane;
        const bool in = p < P;
        float c[3];
        unsigned valid = 0;
        for (int v = 0; v < V; ++v) valid |= (vg_colour(A, v, P, p, in, lo, hi, c) ? 1u : 0u) << v;
        for (int i = 0; i < V; ++i) {
            const bool vi = (valid >> i) & 1u;
            if (!__ballot(vi)) continue;
            vg_colour(A, i, P, p, in, lo, hi, c);                    // the second read of view i comes from the cache
            unsigned q[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) q[ch] = vi ? (unsigned)(int)rintf(c[ch] * 16777216.0f) : 0u;
            for (int j = 0; j < V; ++j) {
                const bool both = vi && ((valid >> j) & 1u);
                const unsigned long long m = __ballot(both);
                if (!m) continue;
                const unsigned s0 = vg_wave_sum(both ? q[0] : 0u), s1 = vg_wave_sum(both ? q[1] : 0u), s2 = vg_wave_sum(both ? q[2] : 0u);
                if (lane < 4) {
                    const unsigned t = lane == 0 ? (unsigned)__popcll(m) : lane == 1 ? s0 : lane == 2 ? s1 : s2;
                    atomicAdd(&s_acc[(i * V + j) * 4 + lane], (unsigned long long)t);
                }
            }
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < cells; k += VG_BLOCK) {
        const unsigned long long a = s_acc[k];
        if (!a) continue;
        const int pair = k >> 2, f = k & 3;
        atomicAdd(f == 0 ? count + pair : colour_sum + pair * 3 + (f - 1), a);
    }
}

extern "C" int32_t ctx_view_pair_stats(const int64_t *atlases, int32_t V, int32_t Tc, float lo, float hi, int64_t *count, int64_t *colour_sum,
                                       ctx_stream_t stream)
{
    CTX_REQUIRE(atlases && count && colour_sum, "view_pair_stats: bad args");
    CTX_REQUIRE(V >= 1 && V <= VG_MAXV, "view_pair_stats: V=%d outside [1, %d]", V, VG_MAXV);
    CTX_REQUIRE(Tc >= 1 && Tc <= VG_MAX_TC, "view_pair_stats: Tc=%d outside [1, %d]", Tc, VG_MAX_TC);
    CTX_REQUIRE(lo > 0.0f && lo < hi && hi <= 1.0f, "view_pair_stats: lo=%g hi=%g, expected 0 < lo < hi <= 1", (double)lo, (double)hi);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(count, 0, sizeof(int64_t) * V * V, s) != hipSuccess || hipMemsetAsync(colour_sum, 0, sizeof(int64_t) * V * V * 3, s) != hipSuccess) {
        ctx_set_error("view_pair_stats: memset failed");
        return CTX_E_LAUNCH;
    }
    const int64_t P = (int64_t)Tc * Tc;
    hipLaunchKernelGGL(k_view_pair_stats, dim3(capped_blocks(P, VG_BLOCK, VG_MAX_BLOCKS)), dim3(VG_BLOCK), 0, s, atlases, V, P, lo, hi,
                       (unsigned long long *)count, (unsigned long long *)colour_sum);
    CTX_CHECK_LAUNCH("view_pair_stats");
    return CTX_OK;
}
