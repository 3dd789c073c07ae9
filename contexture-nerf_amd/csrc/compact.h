// Ordered stream compaction (count -> scan -> write) of n items in blocks of CMP_BLK, stated once: a use (compact.hip, the one
// translation unit that includes this) supplies the item type In, a predicate keep(item) and an emit step emit(i, item, rank); ranks
// ascend with i.  Integer work only: the output does not depend on how blocks or waves are scheduled.
#pragma once
#include "common.h"

#define CMP_BLK 1024

// workspace of a compaction of n items: base i64[nblk] | counts i32[nblk], and 64 spare bytes
struct CompactWs { int64_t nblk, bytes; int64_t *base; int *counts; };
static inline CompactWs compact_ws(int64_t n, void *ws = nullptr)
{
    const int64_t nblk = cdiv64(n, CMP_BLK);
    return {nblk, nblk * 4 + nblk * 8 + 64, (int64_t *)ws, (int *)((int64_t *)ws + nblk)};
}

// the two block-level steps: counts[block] = the block's kept items; rank of a kept item in the output
__device__ __forceinline__ void cmp_block_count(bool v, int *__restrict__ counts)
{
    unsigned long long m = __ballot(v);
    __shared__ int s[CMP_BLK / 64];
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int k = 0; k < CMP_BLK / 64; ++k) t += s[k];
        counts[blockIdx.x] = t;
    }
}
__device__ __forceinline__ int64_t cmp_block_rank(bool v, const int64_t *__restrict__ base)
{
    unsigned long long m = __ballot(v);
    __shared__ int s[CMP_BLK / 64];
    int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) s[w] = __popcll(m);
    __syncthreads();
    int off = 0;
    for (int k = 0; k < w; ++k) off += s[k];
    return base[blockIdx.x] + off + __popcll(m & ((1ull << lane) - 1));
}

template <class In, class Keep>
__global__ __launch_bounds__(CMP_BLK) void k_compact_count(const In *__restrict__ in, int64_t n, Keep keep, int *__restrict__ counts)
{
    int64_t i = (int64_t)blockIdx.x * CMP_BLK + threadIdx.x;
    cmp_block_count(i < n && keep(in[i]), counts);
}

__global__ __launch_bounds__(1024) void k_fvm_scan(int *__restrict__ counts, int64_t nblk, int64_t *__restrict__ base,
                                                   int64_t *__restrict__ n_rows)
{
    // single workgroup: every thread sums one contiguous segment, one Hillis-Steele pass over the 1024 segment sums,
    // then each thread writes its segment's exclusive prefix
    __shared__ int64_t s[1024];
    const int64_t per = (nblk + 1023) / 1024;
    const int64_t i0 = (int64_t)threadIdx.x * per, i1 = i0 + per < nblk ? i0 + per : nblk;
    int64_t sum = 0;
    for (int64_t i = i0; i < i1; ++i) sum += counts[i];
    s[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        int64_t t = threadIdx.x >= o ? s[threadIdx.x - o] : 0;
        __syncthreads();
        s[threadIdx.x] += t;
        __syncthreads();
    }
    int64_t run = s[threadIdx.x] - sum;
    for (int64_t i = i0; i < i1; ++i) { base[i] = run; run += counts[i]; }
    if (threadIdx.x == 1023) n_rows[0] = s[1023];
}

template <class In, class Keep, class Emit>
__global__ __launch_bounds__(CMP_BLK) void k_compact_write(const In *__restrict__ in, int64_t n, Keep keep, const int64_t *__restrict__ base,
                                                           Emit emit)
{
    int64_t i = (int64_t)blockIdx.x * CMP_BLK + threadIdx.x;
    In item = i < n ? in[i] : In();
    bool v = i < n && keep(item);
    int64_t r = cmp_block_rank(v, base);
    if (v) emit(i, item, r);
}

// n_out[0] = the number kept
template <class In, class Keep, class Emit>
static int32_t compact_run(const char *name, const In *in, int64_t n, Keep keep, Emit emit, int64_t *n_out, void *ws, hipStream_t s)
{
    const CompactWs c = compact_ws(n, ws);
    hipLaunchKernelGGL((k_compact_count<In, Keep>), dim3((unsigned)c.nblk), dim3(CMP_BLK), 0, s, in, n, keep, c.counts);
    hipLaunchKernelGGL(k_fvm_scan, dim3(1), dim3(1024), 0, s, c.counts, c.nblk, c.base, n_out);
    hipLaunchKernelGGL((k_compact_write<In, Keep, Emit>), dim3((unsigned)c.nblk), dim3(CMP_BLK), 0, s, in, n, keep, c.base, emit);
    CTX_CHECK_LAUNCH(name);
    return CTX_OK;
}
