// Importance resampling of the marched sample lists (definition: tests/resample_rule.py): every hit ray gets K fine
// samples placed by the inverse CDF of its own coarse weights, and K fine widths that tile its occupied length.
// One wavefront per ray, grid-stride (ray_wave.h); lane s of coarse chunk c holds interval
// ray_off[r] + 64c + s, lane k of output chunk q owns fine sample fine_off[r] + 64q + k.  Sweep one takes the totals W (mass) and L (occupied
// length) by chunked prefix sums chained by two carried scalars, so any S <= 2^31 - 64 works without a chunk table (the chunk and sample
// indices are int).  Sweep two, per output chunk, walks the coarse chunks again with the same sums; a lane whose target falls into the chunk's mass range finds its interval by a six-step
// lane-indexed search on the chunk's exclusive sums (ds_bpermute, no LDS allocation) and fetches that lane's C, l, m, ts, dt.
// Built with -ffp-contract=off.  No atomics; every output element has one writer.
#include "ray_wave.h"

#define RESAMPLE_MAX_K 4096           // the fine lists are composited too: what the compositing backward holds per ray (COMPOSITE_BWD_MAX_S)

__device__ __forceinline__ float resample_lane(float v, int src)          // v of lane src (all 64 lanes active at every call site)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src << 2, __builtin_bit_cast(int, v)));
}

// non-descending prefix sums of v >= 0 continued from carry: in = max over the lanes up to this one of carry + (inclusive sum), ex = the
// lane before's `in` (lane 0: carry); carry <- lane 63's `in`.  A tree-ordered prefix sum of non-negative terms can step down by an ulp
// between neighbouring lanes; the prefix maximum makes it non-descending, which the search, the order of t' and dt' >= 0 rest on.  On
// sequential sums (the restatement) it is the identity.
__device__ __forceinline__ void resample_prefix(float v, float &carry, float &ex, float &in)
{
    in = wave_scan<scan_max>(carry + wave_scan<scan_sum>(v));
    ex = wave_shr1(in, carry);
    carry = wave_lane(in, 63);
}

// One chunk of coarse intervals: the lane's mass m = min(max(w, 0), 1) + 1e-5 (a NaN weight counts as 0, +inf as 1), start and width (all 0
// in a lane past the end), and the prefix sums of m (C) and dt (l), the carries included.
struct resample_chunk_t {
    float m, ts, dt, Cex, Cin, Lex, Lin;
};
__device__ __forceinline__ resample_chunk_t resample_chunk(const float *__restrict__ wr, const float *__restrict__ sr, const float *__restrict__ dr,
                                                           int s, int S, float &Cc, float &Lc)
{
    resample_chunk_t c;
    const bool ok = s < S;
    float w = ok ? wr[s] : 0.f;
    w = w > 0.f ? w : 0.f;
    w = w < 1.f ? w : 1.f;
    c.m = ok ? w + 1e-5f : 0.f;
    c.ts = ok ? sr[s] : 0.f;
    c.dt = ok ? dr[s] : 0.f;
    resample_prefix(c.m, Cc, c.Cex, c.Cin);
    resample_prefix(c.dt, Lc, c.Lex, c.Lin);
    return c;
}

// The last of the chunk's cnt intervals with C <= tau (interval 0 if none): six lane-indexed steps on the non-descending exclusive sums.
__device__ __forceinline__ int resample_find(float Cex, int cnt, float tau)
{
    int lo = 0;
#pragma unroll
    for (int b = 32; b; b >>= 1) {
        const int c = lo + b;                                           // <= 63
        const float v = resample_lane(Cex, c);
        if (c < cnt && v <= tau) lo = c;
    }
    return lo;
}

// f = clamp((tau - C_i) / m_i, 0, 1) in the interval i the search found; a NaN quotient counts as 0
__device__ __forceinline__ float resample_frac(const resample_chunk_t &c, int i, float tau)
{
    float f = (tau - resample_lane(c.Cex, i)) / resample_lane(c.m, i);
    f = f > 0.f ? f : 0.f;
    return f < 1.f ? f : 1.f;
}

__global__ __launch_bounds__(256) void k_resample_packed(const float *__restrict__ weights, const float *__restrict__ tsv,
                                                         const float *__restrict__ dtv, const int64_t *__restrict__ ray_off,
                                                         const float *__restrict__ ro, const float *__restrict__ rd, int64_t R, int64_t n, int K,
                                                         const int64_t *__restrict__ fine_off, const float *__restrict__ xi, int64_t n_fine,
                                                         int32_t *__restrict__ ray_id, float *__restrict__ t_out, float *__restrict__ dt_out,
                                                         float *__restrict__ pts)
{
    const ray_wave rw = ray_wave_here();
    const int lane = rw.lane;
    const float Kf = (float)K;
    for (int64_t r = rw.first; r < R; r += rw.stride) {
        int64_t off;
        const int S = packed_count(ray_off, r, n, off);
        if (S == 0) continue;                                           // an empty ray (most rays of a render): nothing, without its origin
        const int64_t foff = fine_off[r];
        const int64_t fend = fine_off[r + 1] < n_fine ? fine_off[r + 1] : n_fine;
        const int nch = (S + 63) >> 6;
        const float *wr = weights + off, *sr = tsv + off, *dr = dtv + off;
        float W = 0.f, Ltot = 0.f;                                      // sweep one: the totals, by the sums the prefixes are made of
        for (int ch = 0; ch < nch; ++ch) resample_chunk(wr, sr, dr, ch * 64 + lane, S, W, Ltot);
        const float ox = ro[r * 3 + 0], oy = ro[r * 3 + 1], oz = ro[r * 3 + 2];
        const float dx = rd[r * 3 + 0], dy = rd[r * 3 + 1], dz = rd[r * 3 + 2];
        for (int q = 0; q * 64 < K; ++q) {
            const int k = q * 64 + lane;
            const int64_t pos = foff + k;
            const bool store = k < K && pos >= 0 && pos < fend;         // inside the ray's fine span, inside the lists, at most K entries
            const float x = (xi && store) ? xi[pos] : 0.5f;
            // the three targets in mass: the sample and the two edges of its stratum (lane k's upper edge is lane k+1's lower edge: same bits)
            const float tau_s = (((float)k + x) / Kf) * W;
            const float tau_a = ((float)k / Kf) * W, tau_b = ((float)(k + 1) / Kf) * W;
            float tq = 0.f, la = 0.f, lb = 0.f;
            float Cc = 0.f, Lc = 0.f;
            for (int ch = 0; ch < nch; ++ch) {
                const float C0 = Cc;
                const resample_chunk_t c = resample_chunk(wr, sr, dr, ch * 64 + lane, S, Cc, Lc);
                const bool last = ch == nch - 1;
                // the chunk holds a target that lies in [its first C, the next chunk's first C); the last chunk takes all that is left
                // (a lane past K owns no sample: it takes part in the permutes and asks for nothing)
                const bool in_s = k < K && tau_s >= C0 && (last || tau_s < Cc);
                const bool in_a = k < K && tau_a >= C0 && (last || tau_a < Cc);
                const bool in_b = k < K && tau_b >= C0 && (last || tau_b < Cc);
                if (__builtin_amdgcn_ballot_w64(in_s || in_a || in_b) == 0) continue;          // wave-uniform: no lane of this output chunk lands here
                const int cnt = S - ch * 64 < 64 ? S - ch * 64 : 64;
                {
                    const int i = resample_find(c.Cex, cnt, tau_s);
                    const float f = resample_frac(c, i, tau_s);
                    const float v = resample_lane(c.ts, i) + f * resample_lane(c.dt, i);
                    if (in_s) tq = v;
                }
                {
                    const int i = resample_find(c.Cex, cnt, tau_a);
                    const float f = resample_frac(c, i, tau_a);
                    const float v = resample_lane(c.Lex, i) + f * resample_lane(c.dt, i), top = resample_lane(c.Lin, i);
                    if (in_a) la = v < top ? v : top;                   // l(u) stays below the next interval's l: non-descending in u
                }
                {
                    const int i = resample_find(c.Cex, cnt, tau_b);
                    const float f = resample_frac(c, i, tau_b);
                    const float v = resample_lane(c.Lex, i) + f * resample_lane(c.dt, i), top = resample_lane(c.Lin, i);
                    if (in_b) lb = v < top ? v : top;
                }
            }
            if (k == 0) la = 0.f;                                       // the ends are pinned: l(0) = 0, l(1) = L
            if (k + 1 >= K) lb = Ltot;
            if (store) {
                ray_id[pos] = (int32_t)r;
                t_out[pos] = tq;
                dt_out[pos] = lb - la;
                pts[pos * 3 + 0] = ox + dx * tq;                        // one product, one sum per axis: the bits of ctx_occ_points
                pts[pos * 3 + 1] = oy + dy * tq;
                pts[pos * 3 + 2] = oz + dz * tq;
            }
        }
    }
}

extern "C" int32_t ctx_resample_packed(const float *weights, const float *ts, const float *dt, const int64_t *ray_off, const float *rays_o,
                                       const float *rays_d, int64_t R, int64_t n, int32_t K, const int64_t *fine_off, const float *xi,
                                       int64_t n_fine, int32_t *ray_id_out, float *t_out, float *dt_out, float *pts_out, ctx_stream_t stream)
{
    CTX_REQUIRE(R >= 1 && R <= INT32_MAX, "resample_packed: R=%lld outside [1, 2^31)", (long long)R);
    CTX_REQUIRE(K >= 1 && K <= RESAMPLE_MAX_K, "resample_packed: K=%d outside [1, %d]", (int)K, RESAMPLE_MAX_K);
    CTX_REQUIRE(n >= 0 && n <= INT32_MAX, "resample_packed: n=%lld outside [0, 2^31)", (long long)n);
    CTX_REQUIRE(n_fine >= 0 && n_fine <= INT32_MAX, "resample_packed: n_fine=%lld outside [0, 2^31)", (long long)n_fine);
    if (n == 0 || n_fine == 0) return CTX_OK;
    CTX_REQUIRE(weights && ts && dt && ray_off && rays_o && rays_d && fine_off, "resample_packed: null input with n=%lld", (long long)n);
    CTX_REQUIRE(ray_id_out && t_out && dt_out && pts_out, "resample_packed: null output with n_fine=%lld", (long long)n_fine);
    hipLaunchKernelGGL(k_resample_packed, dim3(ray_blocks(R)), dim3(256), 0, (hipStream_t)stream, weights, ts, dt, ray_off, rays_o,
                       rays_d, R, n, (int)K, fine_off, xi, n_fine, ray_id_out, t_out, dt_out, pts_out);
    CTX_CHECK_LAUNCH("resample_packed");
    return CTX_OK;
}
