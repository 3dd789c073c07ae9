// The field optimizer (the rule: tests/adam_rule.py).  Built without FMA contraction: every float operation rounds on
// its own, in source order.
//   ctx_adam_multi : Adam in place on up to 16 float tensors in one launch; the tensor table travels in the kernel's arguments
//   ctx_table_adam : the step of a hash table read straight from the 64-bit integer sums of its gradient (hashgrid.hip, hashtex.hip), which
//                    it leaves zeroed: no float g_table, no zero pass and no convert pass
// Both are streaming kernels: 16 bytes per lane and access, a grid-stride loop over at most ADAM_MAX_BLOCKS workgroups, one writer per
// element, no atomics.  With `sparse` an element whose gradient is exactly zero is left alone, and a run of four such elements costs
// the read of its gradient only.
#include "hashgrid_common.h"

#define ADAM_BLOCK 256
#define ADAM_MAX_TENSORS 16
#define ADAM_CHUNK (ADAM_BLOCK * 4 * 4)        // elements per workgroup turn: four 16-byte accesses per lane and array
#define ADAM_MAX_BLOCKS 2048

struct AdamHyper { float b1, b2, o1, o2, c1, c2, eps; int sparse; };

// head: elements before the first 16-byte boundary (0 .. 3, at most count), or -1: the four pointers disagree, 4-byte accesses throughout
struct AdamTensors {
    float *p[ADAM_MAX_TENSORS], *m[ADAM_MAX_TENSORS], *v[ADAM_MAX_TENSORS];
    const float *g[ADAM_MAX_TENSORS];
    int64_t count[ADAM_MAX_TENSORS];
    int64_t chunk0[ADAM_MAX_TENSORS + 1];      // first chunk of tensor k in the launch's list of chunks
    int32_t head[ADAM_MAX_TENSORS];
    int32_t n;
};

__device__ __forceinline__ void adam_rule(float &p, float &m, float &v, float g, const AdamHyper &h)
{
    m = h.b1 * m + h.o1 * g;
    v = h.b2 * v + (h.o2 * g) * g;
    // sqrtf and / are the correctly rounded ones in this build (hipcc's default, -fhip-fp32-correctly-rounded-divide-sqrt); the __fsqrt_rn
    // intrinsic is not: without OCML's rounded operations it is the native 1-ulp square root
    const float d = sqrtf(v) * h.c2 + h.eps;
    p = p - (h.c1 * m) / d;
}

__device__ __forceinline__ void adam_scalar(float *__restrict__ p, float *__restrict__ m, float *__restrict__ v, float g, int64_t i, const AdamHyper &h)
{
    if (h.sparse && g == 0.0f) return;
    float pi = p[i], mi = m[i], vi = v[i];
    adam_rule(pi, mi, vi, g, h);
    p[i] = pi, m[i] = mi, v[i] = vi;
}

// four elements at a 16-byte boundary of all three arrays; an element with a zero gradient under `sparse` is written back with the bits read
__device__ __forceinline__ void adam_vec4(float *__restrict__ p, float *__restrict__ m, float *__restrict__ v, const float g[4], int64_t i, const AdamHyper &h)
{
    if (h.sparse && g[0] == 0.0f && g[1] == 0.0f && g[2] == 0.0f && g[3] == 0.0f) return;
    float4 p4 = *(const float4 *)(p + i), m4 = *(const float4 *)(m + i), v4 = *(const float4 *)(v + i);
    float *pe = (float *)&p4, *me = (float *)&m4, *ve = (float *)&v4;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (!(h.sparse && g[k] == 0.0f)) adam_rule(pe[k], me[k], ve[k], g[k], h);
    *(float4 *)(p + i) = p4, *(float4 *)(m + i) = m4, *(float4 *)(v + i) = v4;
}

__global__ __launch_bounds__(ADAM_BLOCK) void k_adam_multi(const AdamTensors T, const AdamHyper h)
{
    const int64_t total = T.chunk0[T.n];
    for (int64_t c = blockIdx.x; c < total; c += gridDim.x) {
        int k = 0;
        while (k + 1 < T.n && c >= T.chunk0[k + 1]) ++k;           // workgroup-uniform: at most 15 scalar compares
        float *__restrict__ p = T.p[k], *__restrict__ m = T.m[k], *__restrict__ v = T.v[k];
        const float *__restrict__ g = T.g[k];
        const int64_t count = T.count[k], lc = c - T.chunk0[k];
        const int head = T.head[k];
        if (head < 0) {                                            // 4-byte accesses, adjacent lanes on adjacent elements
            const int64_t e0 = lc * ADAM_CHUNK, e1 = min(count, e0 + ADAM_CHUNK);
            for (int64_t i = e0 + threadIdx.x; i < e1; i += ADAM_BLOCK) adam_scalar(p, m, v, g[i], i, h);
            continue;
        }
        if (lc == 0 && (int)threadIdx.x < head) adam_scalar(p, m, v, g[threadIdx.x], threadIdx.x, h);
        // chunk lc covers the elements head + lc * CHUNK ... of the aligned body; the last float4 may run past count: that is the tail
        const int64_t e0 = head + lc * ADAM_CHUNK, e1 = min(count, e0 + ADAM_CHUNK);
        for (int64_t i = e0 + (int64_t)threadIdx.x * 4; i < e1; i += ADAM_BLOCK * 4) {
            if (i + 4 <= e1) {
                const float4 g4 = *(const float4 *)(g + i);
                adam_vec4(p, m, v, (const float *)&g4, i, h);
            } else {
                for (int64_t j = i; j < e1; ++j) adam_scalar(p, m, v, g[j], j, h);
            }
        }
    }
}

extern "C" int32_t ctx_adam_multi(const void *const *p, const void *const *m, const void *const *v, const void *const *g, const int64_t *counts,
                                  int32_t n_tensors, float b1, float b2, float o1, float o2, float c1, float c2, float eps, int32_t sparse,
                                  ctx_stream_t stream)
{
    CTX_REQUIRE(n_tensors >= 1 && n_tensors <= ADAM_MAX_TENSORS, "adam_multi: n_tensors=%d outside [1, %d]", n_tensors, ADAM_MAX_TENSORS);
    CTX_REQUIRE(p && m && v && g && counts, "adam_multi: null pointer");
    AdamTensors T;
    T.n = n_tensors;
    T.chunk0[0] = 0;
    for (int k = 0; k < n_tensors; ++k) {
        CTX_REQUIRE(p[k] && m[k] && v[k] && g[k], "adam_multi: tensor %d: null pointer", k);
        CTX_REQUIRE(counts[k] >= 1, "adam_multi: tensor %d: count=%lld, want >= 1", k, (long long)counts[k]);
        const uintptr_t a = (uintptr_t)p[k], b = (uintptr_t)m[k], c = (uintptr_t)v[k], d = (uintptr_t)g[k];
        CTX_REQUIRE(((a | b | c | d) & 3) == 0, "adam_multi: tensor %d: a float pointer that is not 4-byte aligned", k);
        T.p[k] = (float *)p[k], T.m[k] = (float *)m[k], T.v[k] = (float *)v[k], T.g[k] = (const float *)g[k];
        T.count[k] = counts[k];
        int64_t body = counts[k];
        if ((a & 15) == (b & 15) && (a & 15) == (c & 15) && (a & 15) == (d & 15)) {
            const int64_t head = (int64_t)(((16 - (a & 15)) & 15) >> 2);
            T.head[k] = (int32_t)(head < counts[k] ? head : counts[k]);
            body -= T.head[k];
        } else {
            T.head[k] = -1;
        }
        const int64_t chunks = cdiv64(body, ADAM_CHUNK);
        T.chunk0[k + 1] = T.chunk0[k] + (chunks > 0 ? chunks : 1);          // a tensor that is all head still gets its chunk
    }
    for (int k = n_tensors; k < ADAM_MAX_TENSORS; ++k) {
        T.p[k] = T.m[k] = T.v[k] = nullptr, T.g[k] = nullptr;
        T.count[k] = 0, T.head[k] = 0, T.chunk0[k + 1] = T.chunk0[n_tensors];
    }
    const AdamHyper h = {b1, b2, o1, o2, c1, c2, eps, sparse != 0};
    hipLaunchKernelGGL(k_adam_multi, dim3(capped_blocks(T.chunk0[n_tensors], 1, ADAM_MAX_BLOCKS)), dim3(ADAM_BLOCK), 0, (hipStream_t)stream, T, h);
    CTX_CHECK_LAUNCH("adam_multi");
    return CTX_OK;
}

// ---- the table's step from its integer sums ------------------------------------------------------------------------------------------
// count is a multiple of 16 (Lv * 2^log2T * F, log2T >= 4) and p, m, v, acc are 16-byte aligned: whole float4 / two longlong2 per lane
__global__ __launch_bounds__(ADAM_BLOCK) void k_table_adam(float *__restrict__ p, float *__restrict__ m, float *__restrict__ v, int64_t count,
                                                           long long *__restrict__ acc, const HgCtl *__restrict__ ctl, int E, const AdamHyper h)
{
    const int status = ctl->status;
    const double inv = hg_pow2(ctl->x - E);
    const int64_t stride = (int64_t)gridDim.x * ADAM_BLOCK * 4;
    for (int64_t i = ((int64_t)blockIdx.x * ADAM_BLOCK + threadIdx.x) * 4; i < count; i += stride) {
        const longlong2 a01 = *(const longlong2 *)(acc + i), a23 = *(const longlong2 *)(acc + i + 2);
        const long long a[4] = {a01.x, a01.y, a23.x, a23.y};
        if (a01.x | a01.y) *(longlong2 *)(acc + i) = make_longlong2(0, 0);
        if (a23.x | a23.y) *(longlong2 *)(acc + i + 2) = make_longlong2(0, 0);
        float g[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)                                // k_hashgrid_convert's expression
            g[k] = status == 2 ? __uint_as_float(0x7fc00000u) : (status == 1 ? 0.0f : (float)((double)a[k] * inv));
        adam_vec4(p, m, v, g, i, h);
    }
}

extern "C" int32_t ctx_table_adam(float *p, float *m, float *v, int64_t count, void *ws, int64_t n, int32_t corners, float b1, float b2, float o1,
                                  float o2, float c1, float c2, float eps, int32_t sparse, ctx_stream_t stream)
{
    CTX_REQUIRE(p && m && v && ws, "table_adam: null pointer");
    CTX_REQUIRE(count >= 16 && count % 16 == 0 && count <= ((int64_t)HG_MAX_LEVELS << 22) * 4,
                "table_adam: count=%lld is not the size of a hash table (Lv * 2^log2T * F, log2T >= 4)", (long long)count);
    CTX_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "table_adam: n=%lld outside [1, 2^31)", (long long)n);
    CTX_REQUIRE(corners == 8 || corners == 4, "table_adam: corners=%d, want 8 (ctx_hashgrid_bwd) or 4 (ctx_hashtex_bwd)", corners);
    CTX_REQUIRE((((uintptr_t)p | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ws) & 15) == 0, "table_adam: p, m, v and ws must be 16-byte aligned");
    long long *acc = (long long *)ws;
    HgCtl *ctl = (HgCtl *)((char *)ws + hg_align(count * 8));
    const int E = hg_acc_exponent(n, corners);
    const AdamHyper h = {b1, b2, o1, o2, c1, c2, eps, sparse != 0};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_table_adam, dim3(capped_blocks(count, ADAM_BLOCK * 4, ADAM_MAX_BLOCKS)), dim3(ADAM_BLOCK), 0, s, p, m, v, count, acc,
                       (const HgCtl *)ctl, E, h);
    (void)hipMemsetAsync(ctl, 0, sizeof(HgCtl), s);
    CTX_CHECK_LAUNCH("table_adam");
    return CTX_OK;
}
