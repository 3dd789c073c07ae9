// The one definition of a hash-grid level for DIM = 3 (the field of the ray path, hashgrid.hip) and DIM = 2 (the texture field, hashtex.hip):
// the limits and the parameter check, a point's cell, the forward's interpolation, the integer accumulator of the table's gradient with
// its control words, helper kernels and host driver, and the launch by feature count (DESIGN sections 4j, 4l).  How a row becomes a unit
// coordinate, and what a file does around these bodies, stays with the file.
#pragma once
#include "common.h"
#include <math.h>

#define HG_MAX_LEVELS 16
#define HG_BLOCK 256

template <int F> struct HgVec;
template <> struct HgVec<1> { typedef float type; };
template <> struct HgVec<2> { typedef float2 type; };
template <> struct HgVec<4> { typedef float4 type; };

// launches kernel<F> for the run-time F in {1, 2, 4}; the rest is hipLaunchKernelGGL's argument list
#define HG_LAUNCH_F(kernel, F, ...)                                                          \
    do {                                                                                     \
        if (F == 1) hipLaunchKernelGGL(kernel<1>, __VA_ARGS__);                              \
        else if (F == 2) hipLaunchKernelGGL(kernel<2>, __VA_ARGS__);                         \
        else hipLaunchKernelGGL(kernel<4>, __VA_ARGS__);                                     \
    } while (0)

// The table [Lv, T = 2^log2T, F] and the cells per axis of its levels.
struct HgTable {
    int res[HG_MAX_LEVELS];
    int Lv, log2T;
};

// what every entry point accepts of a table; res is null where only the sizes are asked about (the workspace queries)
static int32_t hg_check_table(const char *who, int32_t Lv, int32_t F, int32_t log2T, const int32_t *res, HgTable &g)
{
    CTX_REQUIRE(Lv >= 1 && Lv <= HG_MAX_LEVELS, "%s: Lv=%d outside [1, %d]", who, Lv, HG_MAX_LEVELS);
    CTX_REQUIRE(F == 1 || F == 2 || F == 4, "%s: F=%d (1, 2 or 4 features per entry)", who, F);
    CTX_REQUIRE(Lv * F <= 64, "%s: Lv*F=%d above 64, the width of the field's embedding", who, Lv * F);
    CTX_REQUIRE(log2T >= 4 && log2T <= 22, "%s: log2T=%d outside [4, 22]", who, log2T);
    for (int l = 0; res && l < Lv; ++l) {
        CTX_REQUIRE(res[l] >= 1 && res[l] <= (1 << 20), "%s: res[%d]=%d outside [1, 2^20]", who, l, res[l]);
        g.res[l] = res[l];
    }
    g.Lv = Lv; g.log2T = log2T;
    return CTX_OK;
}

// ---- a point's cell ------------------------------------------------------------------------------------------------------------------
// A point on one level, axis by axis, from its unit coordinates x: cell i, weight w inside it, and whether the axis is active, i.e. strictly
// inside the box before the clamp (x > 0 && x < 1: false for NaN, +-inf and the faces).  NaN clamps to 0, so every index is in range.
template <int DIM> struct HgAxes { int i[DIM]; float w[DIM]; bool active[DIM]; };
template <int DIM>
__device__ __forceinline__ HgAxes<DIM> hg_axes(const float (&x)[DIM], int res)
{
    HgAxes<DIM> ax;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        ax.active[a] = x[a] > 0.0f && x[a] < 1.0f;
        const float pos = fminf(fmaxf(x[a], 0.0f), 1.0f) * (float)res;
        ax.i[a] = min((int)floorf(pos), res - 1);
        ax.w[a] = pos - (float)ax.i[a];
    }
    return ax;
}

// The cell: entry index and weight of its 2^DIM corners, c = cx + 2 cy (+ 4 cz).  A level whose (res + 1)^DIM nodes fit the table indexes
// it directly, a finer one by instant-ngp's hash.  The node count is 64-bit: res reaches 2^20, and a count that wrapped (res = 2047 in
// 3-D, 65535 in 2-D) would pass for dense and index the table unmasked.  The weight is the product of the axes' factors, left to right.
template <int DIM> struct HgCell { uint32_t idx[1 << DIM]; float w[1 << DIM]; };
template <int DIM>
__device__ __forceinline__ HgCell<DIM> hg_cell(const HgAxes<DIM> &ax, int res, int log2T)
{
    static_assert(DIM == 2 || DIM == 3, "hash-grid levels are 2-D or 3-D");
    const uint32_t prime[3] = {1u, 2654435761u, 805459861u};
    const uint32_t T = 1u << log2T;
    const int64_t side = (int64_t)res + 1;
    int64_t nodes = side;
#pragma unroll
    for (int a = 1; a < DIM; ++a) nodes *= side;
    const bool dense = nodes <= (int64_t)T;
    HgCell<DIM> c;
#pragma unroll
    for (int k = 0; k < (1 << DIM); ++k) {
        float w = 1.0f;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            const float s = (k >> a) & 1 ? ax.w[a] : 1.0f - ax.w[a];
            w = a ? w * s : s;
        }
        c.w[k] = w;
    }
    if (dense) {                                                                // uniform over the workgroup: one branch per level
#pragma unroll
        for (int k = 0; k < (1 << DIM); ++k) {
            uint32_t idx = 0;
#pragma unroll
            for (int a = DIM - 1; a >= 0; --a) idx = (uint32_t)(ax.i[a] + ((k >> a) & 1)) + (uint32_t)side * idx;   // Horner: gx + side * (gy + side * gz)
            c.idx[k] = idx;
        }
    } else {
#pragma unroll
        for (int k = 0; k < (1 << DIM); ++k) {
            uint32_t idx = 0;
#pragma unroll
            for (int a = 0; a < DIM; ++a) idx ^= (uint32_t)(ax.i[a] + ((k >> a) & 1)) * prime[a];
            c.idx[k] = idx & (T - 1);
        }
    }
    return c;
}

// where row r keeps its F floats of level l in emb or g_emb [n, Lv*F]
template <int F>
__device__ __forceinline__ int64_t hg_row(int64_t r, const HgTable &g, int l) { return r * ((int64_t)g.Lv * F) + l * F; }

// The forward of one (row, level): o[f] = sum over the corners, ascending from 0, of w_c * table[l, idx_c, f]
template <int DIM, int F>
__device__ __forceinline__ void hg_interpolate(const HgAxes<DIM> &ax, const HgTable &g, int l, const float *__restrict__ table, float (&o)[F])
{
    typedef typename HgVec<F>::type V;
    const HgCell<DIM> c = hg_cell(ax, g.res[l], g.log2T);
    const float *tl = table + ((int64_t)l << g.log2T) * F;
    float t[1 << DIM][F];
#pragma unroll
    for (int k = 0; k < (1 << DIM); ++k) *(V *)t[k] = *(const V *)(tl + (int64_t)c.idx[k] * F);   // the 2^DIM gathers in flight together
#pragma unroll
    for (int f = 0; f < F; ++f) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < (1 << DIM); ++k) s = s + c.w[k] * t[k][f];
        o[f] = s;
    }
}

// ---- the integer accumulator of the table's gradient ---------------------------------------------------------------------------------
// absmax: bits of max|g_emb| (the order of non-negative floats is the order of their bits; inf and NaN sort above every finite value);
// status: 0 = accumulate, 1 = all zero, 2 = a non-finite gradient poisons the table's gradient;  x: 2^x is the smallest power of two above m
struct HgCtl { uint32_t absmax; int32_t status; int32_t x; int32_t pad; };

// every thread of the workgroup brings its m: the wave's, then the workgroup's maximum, and one atomic per workgroup
__device__ __forceinline__ void hg_absmax_commit(uint32_t m, HgCtl *__restrict__ ctl)
{
    for (int o = 32; o; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
    __shared__ uint32_t s_m[HG_BLOCK / 64];
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < HG_BLOCK / 64; ++k) m = max(m, s_m[k]);
        if (m) atomicMax(&ctl->absmax, m);
    }
}

static __global__ __launch_bounds__(HG_BLOCK) void k_hashgrid_absmax(const float *__restrict__ g, int64_t count, HgCtl *__restrict__ ctl)
{
    uint32_t m = 0;
    const int64_t stride = (int64_t)gridDim.x * HG_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * HG_BLOCK + threadIdx.x; i < count; i += stride) m = max(m, __float_as_uint(g[i]) & 0x7fffffffu);
    hg_absmax_commit(m, ctl);
}

static __global__ void k_hashgrid_scale(HgCtl *ctl)
{
    const uint32_t b = ctl->absmax;
    int status = 0, x = 0;
    if (b == 0) status = 1;
    else if (b >= 0x7f800000u) status = 2;
    else if (b >> 23) x = (int)(b >> 23) - 126;    // m = 1.f * 2^(e - 127) < 2^(e - 126)
    else x = (31 - __clz((int)b)) - 148;           // subnormal: top bit p is worth 2^(p - 149)
    ctl->status = status;
    ctl->x = x;
}

// the exact power of two 2^e as a double, -1022 <= e <= 1023
__device__ __forceinline__ double hg_pow2(int e) { return __longlong_as_double((long long)(1023 + e) << 52); }

// The backward of one (row, level) into al = the level's accumulator [T, F]: per corner the F terms w_c * ge[f] scaled to integers; then
// keep(idx_c, q), which may merge the terms of lanes that address the same entry into one lane's q, says whether this lane adds its q.
template <int DIM, int F, class Keep>
__device__ __forceinline__ void hg_accumulate(const HgCell<DIM> &c, const float (&ge)[F], double scale, unsigned long long *__restrict__ al, Keep keep)
{
#pragma unroll
    for (int k = 0; k < (1 << DIM); ++k) {
        long long q[F];
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const float prod = c.w[k] * ge[f];                                  // one rounding
            q[f] = __double2ll_rn((double)prod * scale);                        // |prod| < 2^x: |q| <= 2^E, exact scaling, nearest even
        }
        if (keep(c.idx[k], q)) {
#pragma unroll
            for (int f = 0; f < F; ++f)
                if (q[f]) atomicAdd(al + (int64_t)c.idx[k] * F + f, (unsigned long long)q[f]);
        }
    }
}

// Every lane of the wave calls this.  Lanes lane .. end-1 form the run this lane belongs to (adjacent lanes with one key); returns the sum
// of q over lane .. end-1, which in the run's first lane is the run's total: a segmented suffix scan in six shuffle steps.
__device__ __forceinline__ long long hg_run_sum(long long q, int lane, int end)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long other = __shfl_down(q, d, 64);
        if (lane + d < end) q += other;
    }
    return q;
}

// The pre-sum of a wave's terms (hashtex.hip, texmip.hip): every lane of the wave calls this with the entry it addresses and its F terms.
// The terms of every run of adjacent live lanes that address one entry are added into the run's first lane (integers: the sum does not
// depend on its order); returns whether this lane issues the atomics.  A lane that is not live keeps a key of its own (no entry has the
// index 2^32 - 1) and issues nothing.
template <int F>
__device__ __forceinline__ bool hg_presum_runs(uint32_t entry, bool live, int lane, long long (&q)[F])
{
    const uint32_t key = live ? entry : 0xffffffffu;
    const uint32_t prev = (uint32_t)__shfl_up((int)key, 1, 64);
    const bool first = lane == 0 || prev != key || !live;
    const unsigned long long heads = __ballot(first);
    if (heads != ~0ull) {                                                   // uniform: some run is longer than one lane
        const unsigned long long after = lane == 63 ? 0ull : heads >> (lane + 1);
        const int end = after ? lane + 1 + __ffsll((long long)after) - 1 : 64;
#pragma unroll
        for (int f = 0; f < F; ++f) q[f] = hg_run_sum(q[f], lane, end);
    }
    return live && first;
}

static __global__ __launch_bounds__(HG_BLOCK) void k_hashgrid_convert(const long long *__restrict__ acc, int64_t count, int E, const HgCtl *__restrict__ ctl,
                                                               float *__restrict__ g_table)
{
    const int status = ctl->status;
    const double inv = hg_pow2(ctl->x - E);
    const int64_t stride = (int64_t)gridDim.x * HG_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * HG_BLOCK + threadIdx.x; i < count; i += stride)
        g_table[i] = status == 2 ? __uint_as_float(0x7fc00000u) : (status == 1 ? 0.0f : (float)((double)acc[i] * inv));
}

static inline int64_t hg_align(int64_t x) { return (x + 255) & ~(int64_t)255; }

// E = 62 - ceil(log2(corners * n)), corners 8 (3-D) or 4 (2-D): an entry receives at most corners * n terms, each at most 2^E.  The
// accumulate, the convert and the table optimizer (adam.hip) must agree on it, so all three take it from here.
static inline int hg_acc_exponent(int64_t n, int corners)
{
    const int lc = corners == 8 ? 3 : 2;
    int c = lc;
    while (((int64_t)1 << (c - lc)) < n) ++c;
    return 62 - c;
}

// the backward's workspace: the int64 accumulator [Lv, T, F], then the control words; -1: refused
static int64_t hg_table_bwd_ws_bytes(const char *who, int32_t Lv, int32_t F, int32_t log2T)
{
    HgTable g;
    if (hg_check_table(who, Lv, F, log2T, nullptr, g)) return -1;
    return hg_align(((int64_t)Lv << log2T) * F * 8) + 256;
}

// The table's backward of a checked call on n rows, by stages (bits: 1 zero, 2 accumulate, 4 convert).  absmax(blocks, ctl) launches the
// reduction of max|g_emb| over the rows that take part, accumulate(grid, E, ctl, acc) the file's kernel around hg_accumulate<DIM, F>.
template <int DIM, class Absmax, class Accumulate>
static int32_t hg_table_bwd(const char *who, int64_t n, const HgTable &g, int32_t F, int32_t stages, void *ws, float *g_table, hipStream_t s, Absmax absmax,
                            Accumulate accumulate)
{
    CTX_REQUIRE(stages >= 1 && stages <= 7, "%s: stages=%d (bits: 1 zero, 2 accumulate, 4 convert; 7 is the backward)", who, stages);
    const int64_t count = ((int64_t)g.Lv << g.log2T) * F;
    unsigned long long *acc = (unsigned long long *)ws;
    HgCtl *ctl = (HgCtl *)((char *)ws + hg_align(count * 8));
    const int E = hg_acc_exponent(n, 1 << DIM);
    if (stages & 1) {
        (void)hipMemsetAsync(acc, 0, count * 8, s);
        (void)hipMemsetAsync(ctl, 0, sizeof(HgCtl), s);
    }
    if (stages & 2) {
        absmax(dim3(capped_blocks(n * g.Lv * F, HG_BLOCK * 4, 1024)), ctl);
        hipLaunchKernelGGL(k_hashgrid_scale, dim3(1), dim3(1), 0, s, ctl);
        accumulate(dim3((unsigned)cdiv64(n, HG_BLOCK), g.Lv), E, ctl, acc);
    }
    if (stages & 4)
        hipLaunchKernelGGL(k_hashgrid_convert, dim3(capped_blocks(count, HG_BLOCK * 4, 4096)), dim3(HG_BLOCK), 0, s, (const long long *)acc, count, E,
                           ctl, g_table);
    CTX_CHECK_LAUNCH(who);
    return CTX_OK;
}
