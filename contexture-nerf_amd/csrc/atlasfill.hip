// Atlas completion: every uncovered chart texel of the merged atlas takes the colour of its NEAREST covered texel, then the charts
// are padded outward by `pad` texels.  It completes the forward scatter of uvscatter.hip (call contract src/training/trainer.py:1076-1090,
// whose upstream project_back has no body): texels no screen pixel reaches would otherwise ship with the untrained texture field's
// colour.  Colours are copied, never computed: the whole result is defined by an integer source map.
//
//   nearest seed of texel (y, x) = the seed (sy, sx) that minimises (d2, sy, sx) lexicographically, d2 = (y-sy)^2 + (x-sx)^2.
//
// The transform is separable and exact in integers:
//   k_af_cols   ny[y][x] = row of the nearest seed in column x (tie -> the smaller row), AF_NONE when the column has none.
//               A workgroup owns 64 columns (one lane each, coalesced rows); its 16 waves each sweep one band of rows down
//               (last seed at or above), exchange the band summaries through LDS, then sweep the band up.
//   k_af_rows   one workgroup per row: ny of the row in LDS; a lane minimises (x-x')^2 + (ny[x']-y)^2 over x' by walking outward
//               from its own x (x-1, x+1, x-2, ...) until dx^2 > best d2.  Lanes of a wave read consecutive LDS words, and the walk is
//               as long as the answer is far.  The candidate key is (d2 << 24 | sy << 12 | sx), so one 64-bit min carries the
//               tie rule; a candidate with dx^2 == best d2 can still win on (sy, sx), hence the strict '>' of the exit.
//               Worst case (one seed in a corner): T LDS reads per texel.  With no seed at all nothing walks (the row's ny says so).
// AF_NONE = -16384 makes (ny - y)^2 >= 2^28 for every y < 4096 without a branch: a result with d2 >= 2^28 means "no seed".
//
// ctx_atlas_fill = stage A (seeds: coverage > 0; evaluated on chart | covered texels only) into a workspace map, then stage B
// (seeds: chart | covered; walk limited to pad) composed with it, the colour gather in the same launch.  No float arithmetic, no
// atomics, no data-dependent allocation; plain vector stores.
#include "common.h"

#define AF_NONE (-16384)
#define AF_BIG (1u << 28)
#define AF_MAXT 4096
#define AF_SEGS 16

enum { AF_SEED_U8 = 0, AF_SEED_COV = 1, AF_SEED_CHART_OR_COV = 2 };
enum { AF_NEAREST = 0, AF_STAGE_A = 1, AF_STAGE_B = 2 };

template <int SEED>
__device__ __forceinline__ bool af_is_seed(const unsigned char *m, const float *cov, int p)
{
    if (SEED == AF_SEED_U8) return m[p] != 0;
    if (SEED == AF_SEED_COV) return cov[p] > 0.f;
    return m[p] != 0 || cov[p] > 0.f;
}

template <int SEED>
__global__ __launch_bounds__(64 * AF_SEGS) void k_af_cols(const unsigned char *m, const float *cov, int T, short *ny)
{
    __shared__ short s_last[AF_SEGS][64], s_first[AF_SEGS][64];
    const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
    const int x = blockIdx.x * 64 + lane;
    const int L = (T + AF_SEGS - 1) / AF_SEGS;
    const int y0 = min(T, seg * L), y1 = min(T, y0 + L);
    int last = AF_NONE, first = AF_NONE;
    if (x < T) {
        for (int y = y0; y < y1; ++y) {
            const int p = y * T + x;
            if (af_is_seed<SEED>(m, cov, p)) {
                last = y;
                if (first < 0) first = y;
            }
            ny[p] = (short)last;
        }
    }
    s_last[seg][lane] = (short)last;
    s_first[seg][lane] = (short)first;
    __syncthreads();                                   // waits for the LDS stores (lgkmcnt) before the barrier, unlike ctx_barrier()
    if (x >= T) return;
    int up_in = AF_NONE, dn = 1 << 20;
    for (int s = 0; s < seg; ++s) {
        const int v = s_last[s][lane];
        if (v >= 0) up_in = v;
    }
    for (int s = AF_SEGS - 1; s > seg; --s) {
        const int v = s_first[s][lane];
        if (v >= 0) dn = v;
    }
    for (int y = y1 - 1; y >= y0; --y) {
        const int p = y * T + x;
        int up = ny[p];
        if (up < 0) up = up_in;
        if (up == y) dn = y;
        const bool has_up = up >= 0, has_dn = dn < (1 << 20);
        const int r = (has_up && (!has_dn || y - up <= dn - y)) ? up : (has_dn ? dn : AF_NONE);
        ny[p] = (short)r;
    }
}

__device__ __forceinline__ unsigned long long af_key(const int *s_ny, int xc, int x, int y)
{
    const int n = s_ny[xc];
    const int dx = xc - x, dy = n - y;
    const unsigned d2 = (unsigned)(dx * dx) + (unsigned)(dy * dy);
    return ((unsigned long long)d2 << 24) | (unsigned)((n & 0xfff) << 12) | (unsigned)xc;
}

template <int MODE>
__global__ __launch_bounds__(256) void k_af_rows(const short *ny, int T, const unsigned char *chart, const float *cov, int pad, int *src, int *d2out,
                                                 const int *src_a, const float *atlas, float *filled, int C)
{
    extern __shared__ int s_ny[];
    const int y = blockIdx.x;
    int any = 0;
    for (int x = threadIdx.x; x < T; x += 256) {
        const int n = ny[y * T + x];
        s_ny[x] = n;
        any |= n >= 0;
    }
    // barrier (with the wait for the LDS stores above) + "is there a seed at all": every column's ny is valid or none for the whole
    // column, so a row without a valid ny means no seed anywhere, and no texel walks its row for an answer that is -1
    const bool has_seed = __syncthreads_or(any) != 0;
    for (int x = threadIdx.x; x < T; x += 256) {
        const int p = y * T + x;
        bool walk = has_seed;
        if (MODE == AF_STAGE_A) walk = walk && (chart[p] != 0 || cov[p] > 0.f);
        unsigned long long key = af_key(s_ny, x, x, y);
        if (walk) {
            const int rmax = MODE == AF_STAGE_B ? min(pad, T - 1) : T - 1;
            for (int r = 1; r <= rmax; ++r) {
                if ((unsigned long long)(r * r) > (key >> 24)) break;
                const int xl = x - r, xr = x + r;
                if (xl < 0 && xr >= T) break;
                if (xl >= 0) key = min(key, af_key(s_ny, xl, x, y));
                if (xr < T) key = min(key, af_key(s_ny, xr, x, y));
            }
        }
        const unsigned d2 = (unsigned)(key >> 24);
        const bool found = walk && d2 < AF_BIG;
        const int q = (int)((key >> 12) & 0xfff) * T + (int)(key & 0xfff);
        if (MODE == AF_NEAREST) {
            src[p] = found ? q : -1;
            d2out[p] = found ? (int)d2 : -1;
        } else if (MODE == AF_STAGE_A) {
            src[p] = found ? q : -1;
        } else {
            const int s = (found && d2 <= (unsigned)(pad * pad)) ? src_a[q] : -1;
            src[p] = s;
            const size_t from = s >= 0 ? (size_t)s : (size_t)p, TT = (size_t)T * T;
            for (int c = 0; c < C; ++c) filled[c * TT + p] = atlas[c * TT + from];
        }
    }
}

extern "C" int64_t ctx_atlas_fill_ws_bytes(int32_t T) { return (T < 1 || T > AF_MAXT) ? -1 : (int64_t)T * T * 6 + 256; }

static short *af_ny(void *ws) { return (short *)ws; }
static int *af_src_a(void *ws, int T) { return (int *)((char *)ws + (((size_t)T * T * 2 + 255) / 256) * 256); }

extern "C" int32_t ctx_nearest_seed(const uint8_t *seed, int32_t T, int32_t *src, int32_t *d2, void *ws, int64_t ws_bytes, ctx_stream_t stream)
{
    CTX_REQUIRE(seed && src && d2 && ws, "nearest_seed: bad args");
    CTX_REQUIRE(T >= 1 && T <= AF_MAXT, "nearest_seed: T=%d outside [1, %d]", T, AF_MAXT);
    CTX_REQUIRE(ws_bytes >= ctx_atlas_fill_ws_bytes(T), "nearest_seed: workspace of %lld bytes, ctx_atlas_fill_ws_bytes(%d) = %lld", (long long)ws_bytes, T,
                (long long)ctx_atlas_fill_ws_bytes(T));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_af_cols<AF_SEED_U8>, dim3(cdiv(T, 64)), dim3(64 * AF_SEGS), 0, s, seed, (const float *)nullptr, T, af_ny(ws));
    hipLaunchKernelGGL(k_af_rows<AF_NEAREST>, dim3(T), dim3(256), (size_t)T * 4, s, af_ny(ws), T, (const unsigned char *)nullptr, (const float *)nullptr, 0, src, d2,
                       (const int *)nullptr, (const float *)nullptr, (float *)nullptr, 0);
    CTX_CHECK_LAUNCH("nearest_seed");
    return CTX_OK;
}

extern "C" int32_t ctx_atlas_fill(const float *atlas, const float *coverage, const uint8_t *chart, int32_t C, int32_t T, int32_t pad, float *filled, int32_t *src,
                                  void *ws, int64_t ws_bytes, ctx_stream_t stream)
{
    CTX_REQUIRE(atlas && coverage && chart && filled && src && ws && filled != atlas, "atlas_fill: bad args");
    CTX_REQUIRE(T >= 1 && T <= AF_MAXT, "atlas_fill: T=%d outside [1, %d]", T, AF_MAXT);
    CTX_REQUIRE(C >= 1 && C <= 64, "atlas_fill: C=%d outside [1, 64]", C);
    CTX_REQUIRE(pad >= 0 && pad <= AF_MAXT, "atlas_fill: pad=%d outside [0, %d]", pad, AF_MAXT);
    CTX_REQUIRE(ws_bytes >= ctx_atlas_fill_ws_bytes(T), "atlas_fill: workspace of %lld bytes, ctx_atlas_fill_ws_bytes(%d) = %lld", (long long)ws_bytes, T,
                (long long)ctx_atlas_fill_ws_bytes(T));
    hipStream_t s = (hipStream_t)stream;
    short *ny = af_ny(ws);
    int *src_a = af_src_a(ws, T);
    const dim3 gc(cdiv(T, 64)), bc(64 * AF_SEGS);
    // stage A: nearest covered texel of every chart | covered texel
    hipLaunchKernelGGL(k_af_cols<AF_SEED_COV>, gc, bc, 0, s, (const unsigned char *)nullptr, coverage, T, ny);
    hipLaunchKernelGGL(k_af_rows<AF_STAGE_A>, dim3(T), dim3(256), (size_t)T * 4, s, ny, T, chart, coverage, 0, src_a, (int *)nullptr, (const int *)nullptr,
                       (const float *)nullptr, (float *)nullptr, 0);
    // stage B: nearest chart | covered texel within pad, composed with stage A, and the colour gather
    hipLaunchKernelGGL(k_af_cols<AF_SEED_CHART_OR_COV>, gc, bc, 0, s, chart, coverage, T, ny);
    hipLaunchKernelGGL(k_af_rows<AF_STAGE_B>, dim3(T), dim3(256), (size_t)T * 4, s, ny, T, chart, coverage, pad, src, (int *)nullptr, src_a, atlas, filled, C);
    CTX_CHECK_LAUNCH("atlas_fill");
    return CTX_OK;
}
