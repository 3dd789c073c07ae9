// Flash-style fused attention  O = softmax(Q K^T * scale) V  for the UNet transformer blocks
// (diffusers Attention / AttnProcessor2_0 under src/stable_diffusion_depth.py:422), head_dim 64, fp16
// operands, fp32 scores / running max / running sum / output accumulator.
//
// 4 waves per workgroup, 32 query rows per wave; K/V tiles of 64 keys staged through LDS and shared
// by the 4 waves.  Scores are computed TRANSPOSED (S^T = K . Q^T: K rows are the MFMA A operand, Q
// the B operand) so each lane owns one query column: the softmax row reductions are in-register plus a
// single cross-half shuffle, and the exponentiated tile, converted to f16 in place, is already the B
// operand of the second product O^T = V^T . P^T (no LDS round trip for P).  V arrives pre-transposed
// ([B, heads, 64, Skv_pad], keys contiguous) so its fragment is two 8-byte LDS reads.
#include "gemm_common.h"
#include <math.h>
#include <type_traits>

#define AT_KB 64                // keys per tile
#define AT_KROW 72              // f16 per K row in LDS (144 B: conflict-free ds_read_b128)
#define AT_VROW 68              // f16 per V^T row in LDS (136 B: conflict-free ds_read_b64)


struct AttnArgs {
    const f16 *Q, *K, *V;
    f16 *O;
    int Sq, Skv, heads;
    int q_stride, kv_stride, o_stride;
    float scale_log2e;
    float lazy;            // log2 units a row's maximum may run ahead of the subtracted one before the accumulators are rescaled (0: never)
};

// ------------------------------------------------------------------------------------------------
// LDS-DMA variant (default): K and V^T tiles arrive by global_load_lds into a ring of AT_NS stages (1 KiB pieces of
// 8 rows x 128 B, chunk swizzle c ^ ((row>>1)&7) on the source address and on the fragment reads), prefetch distance
// AT_NS-1 tiles, one raw s_barrier + counted vmcnt per tile — the same pipeline as k_gemm_pipe.


// One 64-key tile of the online-softmax recurrence for this wave's 32 queries (MASK only for the last, ragged tile).
// V stays [key][d] in LDS exactly as it lies in memory (no transpose pass): the PV product's A operand (V^T: row d,
// 8 keys) comes from two transposing reads ds_read_b64_tr_b16, each a 4-key x 16-d block per 16-lane group: lane
// (q = (l&15)>>2, p = l&3) points at key row q, d columns 4p..4p+3 and receives d column l&15 of the 4 keys — exactly
// the keys 4h + (0..3) (then 8 + 4h + (0..3)) that element j of the P fragment holds.  The 16-byte chunk index of the V
// image is XORed with 4 on key rows 2, 3 (mod 4), which spreads the four rows of a block over all 64 banks.
// The row sums l = sum_k p ride on the matrix pipe: one extra MFMA per k-step with an all-ones A operand accumulates, in
// every row of `ls`, the sum of exactly the fp16-rounded P the PV product uses; the VALU is this kernel's critical resource.
typedef short at_s16x4 __attribute__((__vector_size__(4 * sizeof(short))));
__device__ __forceinline__ f16x4 at_tr16(const f16 *p)
{
    at_s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) at_s16x4 *)p);
    return __builtin_bit_cast(f16x4, v);
}
struct AtNoIssue { __device__ __forceinline__ void operator()(int) const {} };
// NISSUE > 0: `iss(i)` launches DMA piece i of a later tile right behind the i-th QK MFMA.  The four waves of a workgroup leave the
// tile's barrier together, and 16 KB of global_load_lds issued in one burst queue at the CU's one vector-memory port: timestamps
// taken inside the loop (s_memtime around each section, round 3) showed ~10 % of a wave's tile period stalled at the issue of
// its 4 pieces.
template <bool MASK, int NISSUE = 0, class Issue = AtNoIssue>
__device__ __forceinline__ void attn_tile(const f16 *__restrict__ Ks, const f16 *__restrict__ Vs, int k0, int Skv, int r, int h,
                                          int swz, int vlane, int vfq, int xidx, float c, const f16x8 (&qf)[4], f32x16 (&o)[2], f32x16 &ls,
                                          float &m_run, float lazy, Issue iss = Issue())
{
    f32x16 s[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int q = 0; q < 16; ++q) s[kb][q] = 0.f;
        const f16 *kr = Ks + (kb * 32 + r) * 64;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            f16x8 kf = *(const f16x8 *)(kr + ((2 * ks + h) ^ swz) * 8);
            s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[ks], s[kb], 0, 0, 0);
            if (kb * 4 + ks < NISSUE) iss(kb * 4 + ks);
        }
    }
    if (MASK) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                int key = k0 + kb * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
                if (key >= Skv) s[kb][q] = -INFINITY;
            }
    }
    // 32 scores -> three-input maxima in two chains (v_max3_f32), then the other half's lane
    float mxa = fmaxf(s[0][0], s[0][1]), mxb = fmaxf(s[1][0], s[1][1]);
#pragma unroll
    for (int q = 2; q < 16; q += 2) {
        mxa = __builtin_fmaxf(__builtin_fmaxf(mxa, s[0][q]), s[0][q + 1]);
        mxb = __builtin_fmaxf(__builtin_fmaxf(mxb, s[1][q]), s[1][q + 1]);
    }
    float mx = fmaxf(mxa, mxb);
    // xidx = 4 * (lane ^ 32), formed once by the caller (__shfl_xor rebuilds it with a compare, a select and a shift per tile)
    mx = fmaxf(mx, __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(xidx, __builtin_bit_cast(int, mx)))) * c;
    // The subtracted maximum is any per-row constant: it follows the true running maximum only when some row of the wave has moved by
    // more than `lazy` (P then stays <= 2^lazy, exact in fp16's range), which skips most of the 33-multiply rescales of O and l
    // (lazy = 0: every change, the textbook recurrence; first tile: m_run = -inf always moves)
    const float m_cand = fmaxf(m_run, mx);
    const bool move = __any(m_cand > m_run + lazy);
    const float m_new = move ? m_cand : m_run;
    // s * c - m_new two scores per instruction (v_pk_fma_f32: the same fused operation per element), then the exponentials
    typedef float at_f2 __attribute__((ext_vector_type(2)));
    const at_f2 c2 = {c, c}, nm2 = {-m_new, -m_new};
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int q = 0; q < 16; q += 2) {
            const at_f2 t = __builtin_elementwise_fma((at_f2){s[kb][q], s[kb][q + 1]}, c2, nm2);
            s[kb][q] = __builtin_amdgcn_exp2f(t[0]);
            s[kb][q + 1] = __builtin_amdgcn_exp2f(t[1]);
        }
    // rescale only when some row's max moved (wave-uniform branch).  The multiplies are inline asm with tied operands:
    // written as C++ the compiler multiplies out of place and then copies all 48 accumulator registers on the
    // fall-through path of every tile, which costs more than multiplying unconditionally.
    if (move) {
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);      // 0 on the first tile (m_run = -inf)
        // s_nop: alpha comes straight from v_exp_f32 (transcendental -> VALU use needs a wait state hipcc cannot see into)
        asm volatile("s_nop 1\n\tv_mul_f32 %0, %0, %1" : "+v"(ls[0]) : "v"(alpha));
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
            for (int q = 0; q < 16; ++q) asm volatile("v_mul_f32 %0, %0, %1" : "+v"(o[d][q]) : "v"(alpha));
    }
    m_run = m_new;
    const f16x8 ones = {1, 1, 1, 1, 1, 1, 1, 1};
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            f16x8 pf;
#pragma unroll
            for (int j = 0; j < 8; ++j) pf[j] = (f16)s[kb][8 * st + j];
            const f16 *vk = Vs + (32 * kb + 16 * st + 4 * h) * 64 + vlane;       // key block of this lane half
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                const int co = ((4 * d) ^ vfq) * 8;                              // d block, swizzled with the lane's key row
                f16x4 v0 = at_tr16(vk + co), v1 = at_tr16(vk + 8 * 64 + co);
                f16x8 vf = __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
                o[d] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, o[d], 0, 0, 0);
            }
            ls = __builtin_amdgcn_mfma_f32_32x32x16_f16(ones, pf, ls, 0, 0, 0);
        }
}

// NW waves per workgroup (32 queries each): 4 = 128 queries, 8 = 256 queries per staged K/V tile (half the L2 -> LDS bytes per
// FLOP: the staging path is this chip's scarce resource, ~28 B/clk per CU, and three 4-wave workgroups per CU ask ~20 of it)
//
// KS = 2 (12 waves: 6 query blocks x 2 key ranges) splits the tiles of a launch between two wave groups of one workgroup: group 0
// runs tiles [0, ceil(ntiles/2)), group 1 the rest, each through a ring, an issue counter and a counted vmcnt of its own, and the two
// partial (o, l, m) of a query block meet in LDS behind the last tile.  The unit of work per wave halves, which is what balances the
// mid-size self-attention over the SIMDs (attn_plan).  gfx950 has no named barriers, so the groups share the one workgroup barrier:
// every wave meets it once per tile trip of the longer range; the group with fewer tiles meets the ones it has no tile for bare.
template <int AT_NS, int NW, bool SPREAD = true, int KS = 1>
__global__ __launch_bounds__(64 * NW, NW == 8 ? 4 : NW == 12 ? 3 : 1) void k_attention_dma(AttnArgs a)
{
    constexpr int NQ = NW / KS;                      // query blocks of 32 per workgroup = waves per key range
    constexpr int STAGE = 2 * 64 * 64;               // f16 per stage: K [64][64] then V [64][64]
    constexpr int G = (16 + NQ - 1) / NQ;            // DMA pieces per wave per tile: the tile is 8 + 8 pieces of 1 KiB
    static_assert(NW == NQ * KS && (KS == 1 ? 16 % NQ == 0 : NQ * 34 * 64 * 4 <= KS * 2 * STAGE * 2), "attention: workgroup shape");
    __shared__ __attribute__((aligned(16))) f16 ring[KS * AT_NS * STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform by construction: SGPR, scalar branches
    const int half = KS == 1 ? 0 : (wave >= NQ ? 1 : 0), qw = wave - half * NQ;
    const int r = lane & 31, h = lane >> 5;
    const int b = blockIdx.z, hd = blockIdx.y;
    const int q0 = blockIdx.x * (32 * NQ) + qw * 32;
    const int qrow = q0 + r;
    const bool qok = qrow < a.Sq;

    f16x8 qf[4];
    const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    {
        const f16 *qp = a.Q + ((size_t)b * a.Sq + (qok ? qrow : 0)) * a.q_stride + hd * 64 + 8 * h;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = qok ? *(const f16x8 *)(qp + ks * 16) : zero8;
    }
    f32x16 o[2];
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int q = 0; q < 16; ++q) o[d][q] = 0.f;
    f32x16 ls;
#pragma unroll
    for (int q = 0; q < 16; ++q) ls[q] = 0.f;
    float m_run = -INFINITY;

    // this wave's tiles [tb, tb + n) of the launch's ntiles (nf of them full: only the launch's last tile can be ragged)
    const int ntiles = (a.Skv + AT_KB - 1) / AT_KB;
    const int nmax = (ntiles + KS - 1) / KS;
    const int tb = half * nmax, n = half ? ntiles - nmax : nmax;
    const int nf = max(min(tb + n, a.Skv / AT_KB) - tb, 0);
    f16 *const ringh = ring + half * (AT_NS * STAGE);
    // issue-side state: slot j of this wave moves piece qw + NQ*j of the tile's 16 (0 .. 7 of K, 8 .. 15 of V; with 6 waves the last two
    // have no third piece and move their first again: same bytes to the same place, and vmcnt counts G per tile in every wave).  The
    // source is a wave-uniform pointer, advanced by a scalar add per tile, plus a 32-bit lane offset that never changes.
    const int lr = lane >> 3, pc = lane & 7;
    const char *dsrc[G];
    uint32_t doff[G];
    int drow[G], dlds[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
        const int p = (KS > 1 && qw + NQ * j >= 16) ? qw : qw + NQ * j;
        const bool isv = KS == 1 ? j >= G / 2 : p >= 8;
        const int row = 8 * (p & 7) + lr;
        const int lc = isv ? pc ^ (((row >> 1) & 1) << 2) : pc ^ ((row >> 1) & 7);
        drow[j] = row;
        doff[j] = ((uint32_t)row * (uint32_t)a.kv_stride + lc * 8) * 2;                      // < 2^32: ctx_attention_f16 bounds kv_stride
        dlds[j] = (isv ? 64 * 64 : 0) + (p & 7) * 512;
        dsrc[j] = (const char *)((isv ? a.V : a.K) + ((size_t)b * a.Skv + (size_t)tb * AT_KB) * a.kv_stride + hd * 64);
    }
    const size_t tile_bytes = (size_t)AT_KB * a.kv_stride * 2;
    int issued = 0;
    // piece j of tile tb + `issued`; the caller bumps `issued` after the last one.  FULL: the tile is known to be a full one (the steady
    // loop); otherwise rows behind the last key come from the zero page
    auto issue_piece = [&](int buf, int j, auto full) {
        // the empty asms pin the base in SGPRs and the offset in one VGPR as values of their own, next to the load: left to itself
        // hipcc widens the offset outside the loop and pays a 64-bit vector add per piece, where global_load_lds takes a scalar base
        // and a 32-bit lane offset as they are
        asm volatile("" : "+s"(dsrc[j]), "+v"(doff[j]));
        const char *src = dsrc[j] + (size_t)doff[j];
        if (!decltype(full)::value && (tb + issued) * AT_KB + drow[j] >= a.Skv) src = (const char *)ctx_zero_page;
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(ringh + buf * STAGE + dlds[j]), 16, 0, 0);
        dsrc[j] += tile_bytes;
    };
    auto issue = [&](int buf, auto full) {
#pragma unroll
        for (int j = 0; j < G; ++j) issue_piece(buf, j, full);
        ++issued;
    };
    constexpr std::true_type FULL{};
    constexpr std::false_type ANY{};
#pragma unroll
    for (int p = 0; p < AT_NS - 1; ++p)
        if (p < n) issue(p, ANY);

    const int swz = (r >> 1) & 7;
    // V reads: lane (q = (l&15)>>2, p = l&3, a = (l>>4)&1) -> key row q, d columns 16a + 4p.. of a 32-d block
    const int vq = (lane & 15) >> 2, vfq = ((vq >> 1) & 1) << 2;
    const int vlane = vq * 64 + (((2 * ((lane >> 4) & 1) + ((lane & 3) >> 1)) ^ 0) * 8) + (lane & 1) * 4;
    const int xidx = (lane ^ 32) << 2;               // ds_bpermute address of the lane that holds the other 16 keys of this query
    const float c = a.scale_log2e;
    // one copy of the tile body in the loop (runtime ring slot): full tiles first, the ragged tile peeled off the end, so
    // the accumulators keep one fixed register block (unrolled / two-variant bodies made hipcc shuffle all 48 of them)
    int slot = 0;
    int t = 0;
    // steady tiles: the tile AT_NS-1 ahead is a full one still to be issued, so exactly AT_NS-2 newer tiles are in flight at the wait
    // and the issue needs no row test (no wave-uniform branches in the body; a ragged tile is issued from the drain loop)
    for (; t + AT_NS - 1 < nf; ++t) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((AT_NS - 2) * G) : "memory");
        __builtin_amdgcn_sched_barrier(0);
        ctx_barrier();
        const int ibuf = slot == 0 ? AT_NS - 1 : slot - 1;
        const f16 *Ks = ringh + slot * STAGE;
        if (SPREAD) {
            attn_tile<false, G>(Ks, Ks + 64 * 64, (tb + t) * AT_KB, a.Skv, r, h, swz, vlane, vfq, xidx, c, qf, o, ls, m_run, a.lazy,
                                [&](int idx) { issue_piece(ibuf, idx, FULL); });
            ++issued;
        } else {
            issue(ibuf, FULL);
            attn_tile<false>(Ks, Ks + 64 * 64, (tb + t) * AT_KB, a.Skv, r, h, swz, vlane, vfq, xidx, c, qf, o, ls, m_run, a.lazy);
        }
        slot = slot + 1 == AT_NS ? 0 : slot + 1;
    }
    for (; t < nf; ++t) {
        const int newer = issued - 1 - t;
        if (AT_NS >= 4 && newer >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * G) : "memory");
        else if (newer >= 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // tile t-1's slot is refilled right after the barrier and the barrier does not wait for LDS reads in flight: the tile's
        // MFMAs (which wait for their K / V fragments) must all stay above it
        __builtin_amdgcn_sched_barrier(0);
        ctx_barrier();
        if (issued < n) issue(slot == 0 ? AT_NS - 1 : slot - 1, ANY);          // the ragged tile, into the slot tile t-1 used
        const f16 *Ks = ringh + slot * STAGE;
        attn_tile<false>(Ks, Ks + 64 * 64, (tb + t) * AT_KB, a.Skv, r, h, swz, vlane, vfq, xidx, c, qf, o, ls, m_run, a.lazy);
        slot = slot + 1 == AT_NS ? 0 : slot + 1;
    }
    if (nf < n) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ctx_barrier();
        const f16 *Ks = ringh + slot * STAGE;
        attn_tile<true>(Ks, Ks + 64 * 64, (tb + nf) * AT_KB, a.Skv, r, h, swz, vlane, vfq, xidx, c, qf, o, ls, m_run, a.lazy);
    }
    if (KS > 1) {
        for (int i = n; i < nmax; ++i) ctx_barrier();                           // the trips of the longer key range this one has no tile for
        // Merge: group 1 parks (o, l, m) of its 32 queries in the dead rings as [query block][value][lane]; the group-0 wave of the same
        // block folds them into its own in fp32, always as own * 2^(m0 - m) + parked * 2^(m1 - m).  A range without tiles parks
        // m = -inf, l = 0, o = 0 and weighs exactly nothing (m0 is finite: group 0 always has a tile with a key in it).
        float *mg = (float *)ring + qw * (34 * 64) + lane;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                      // this wave's K / V fragment reads have landed,
        ctx_barrier();                                                          // every wave's have: the rings are dead
        if (half) {
#pragma unroll
            for (int d = 0; d < 2; ++d)
#pragma unroll
                for (int q = 0; q < 16; ++q) mg[(16 * d + q) * 64] = o[d][q];
            mg[32 * 64] = ls[0];
            mg[33 * 64] = m_run;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        ctx_barrier();
        if (half) return;
        const float m1 = mg[33 * 64], m = fmaxf(m_run, m1);
        const float a0 = __builtin_amdgcn_exp2f(m_run - m), a1 = m1 == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m1 - m);
        ls[0] = ls[0] * a0 + mg[32 * 64] * a1;
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
            for (int q = 0; q < 16; ++q) o[d][q] = o[d][q] * a0 + mg[(16 * d + q) * 64] * a1;
    }
    if (qok) {
        float inv = 1.0f / ls[0];
        f16 *op = a.O + ((size_t)b * a.Sq + qrow) * a.o_stride + hd * 64;
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f16x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = (f16)(o[d][4 * g + j] * inv);
                *(f16x4 *)(op + d * 32 + 8 * g + 4 * h) = v;
            }
    }
}

template <int NS, int NW, bool SPREAD = true, int KS = 1>
static void attn_launch(const AttnArgs &a, int B, bool report, hipStream_t s)
{
    constexpr auto kern = k_attention_dma<NS, NW, SPREAD, KS>;
    if (report) {
        int nb = 0;
        hipFuncAttributes fa;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, 64 * NW, 0);
        (void)hipFuncGetAttributes(&fa, (const void *)kern);
        fprintf(stderr, "[ctx] attention: %d blocks/CU by the occupancy API, %d VGPRs, %zu B static LDS\n", nb, fa.numRegs, fa.sharedSizeBytes);
    }
    ctx_launch<kern>(1, dim3(cdiv(a.Sq, 32 * NW / KS), a.heads, B), dim3(64 * NW), 0, s, a);
}

// Which workgroup form a launch takes, by how it balances over the SIMDs.  MFMA and VALU work of different waves on one SIMD do not
// overlap: a SIMD retires about one wave-tile (32 queries x 64 keys) per fixed number of clocks whatever its occupancy,
// so a launch takes as long as its busiest SIMD has wave-tiles.  The dispatcher spreads workgroups evenly over the CUs, in rounds once
// registers and LDS admit no more (3 four-wave, 2 eight-wave, 1 split workgroup per CU: the cap drops out of the count), so the busiest
// CU runs ceil(workgroups / CUs) of them, each putting NW/4 waves on every SIMD.  The split form pays its merge (33 multiply-adds per
// lane, two barriers, an LDS round trip) as one more tile per wave.  Today's form (`base`: 8 waves for the mid-size self-attention, else
// 4) is left only for a form the model puts more than 1/8 ahead: at equal counts the forms still differ by ~7 % in what the model does
// not see (72 against 77 us at 72 wave-tiles each, staging traffic per FLOP), and a tie keeps the base.
//   2 x 10 heads x 2304^2: 4 waves 2 x 36 = 72, 8 waves 2 x 36 = 72, split 3 x 19 = 57 -> split
//   2 x  5 heads x 9216^2: 4 waves 3 x 144 = 432, split 2 x 3 x 73 = 438 -> 4 waves;  2 x 20 x 576^2: 9 against 3 x 6 = 18 -> 4 waves
//   77 keys: two tiles a wave against 3 x (1 + 1) -> 4 waves;  12 x 10 x 2304^2: 8 waves 360, 4 waves 324 (10 % ahead) -> stays
struct AttnPlan { int nw, ks, wgs, cost; };
static AttnPlan attn_plan(int B, int Sq, int Skv, int heads, int n_cu, int nw8)
{
    const int ntiles = cdiv(Skv, AT_KB);
    auto form = [&](int nw, int ks) {
        AttnPlan p = {nw, ks, cdiv(Sq, 32 * nw / ks) * heads * B, 0};
        const int64_t cost = (int64_t)cdiv(p.wgs, n_cu) * (nw / 4) * (cdiv(ntiles, ks) + (ks > 1 ? 1 : 0));
        p.cost = (int)(cost < INT32_MAX ? cost : INT32_MAX);
        return p;
    };
    const AttnPlan f4 = form(4, 1), f8 = form(8, 1), f12 = form(12, 2);
    if (nw8 >= 0) return nw8 == 2 ? f12 : nw8 == 1 ? f8 : f4;
    const bool w8 = Sq >= 1024 && Sq < 4096 && Skv >= 1024;
    AttnPlan best = w8 ? f8 : f4;
    const int64_t bar = (int64_t)best.cost * 7;                                 // 8 * cost < 7 * base: more than 1/8 ahead
    for (const AttnPlan &p : {f4, f8, f12})
        if ((int64_t)p.cost * 8 < bar && p.cost < best.cost) best = p;
    return best;
}
static int attn_cu_count()
{
    static const int n = [] {
        int dev = 0, cu = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cu <= 0) cu = 256;
        return cu;
    }();
    return n;
}

// Kernel selection (A/B switches): the environment seeds it once per process, ctx_attention_tune overrides it while set.
//   ns      CTX_ATTN_NS      ring depth 2 | 3 | 4 (default 3; anything else runs 3)
//   nw8     CTX_ATTN_NW8     0 always the 4-wave workgroups, 1 always the 8-wave ones, 2 always the K/V-split ones, -1 by attn_plan
//   spread  CTX_ATTN_SPREAD  0: all DMA pieces of a tile right after the barrier
//   lazy    CTX_ATTN_LAZY    rescale threshold in log2 units (default 8 = a factor 256; 0 = rescale on every change; 0 .. 12)
struct AttnTune { int ns, nw8, spread; float lazy; };
static AttnTune g_attn_force = {-1, -1, -1, -1.f};          // -1 / negative lazy: what the environment or the default says
static const AttnTune &attn_tune_env()
{
    static const AttnTune env = [] {
        AttnTune t;
        t.ns = ctx_env_int("CTX_ATTN_NS", 3);
        t.nw8 = ctx_env_int("CTX_ATTN_NW8", -1);
        t.spread = ctx_env_int("CTX_ATTN_SPREAD", 1);
        const char *e = getenv("CTX_ATTN_LAZY");
        t.lazy = e ? (float)atof(e) : 8.0f;
        if (!(t.lazy >= 0.f && t.lazy <= 12.f)) t.lazy = 8.0f;
        return t;
    }();
    return env;
}

extern "C" void ctx_attention_tune(int32_t ns, int32_t nw8, int32_t spread, float lazy)
{
    g_attn_force.ns = ns; g_attn_force.nw8 = nw8; g_attn_force.spread = spread; g_attn_force.lazy = lazy;
}
static int attn_nw8() { return g_attn_force.nw8 >= 0 ? g_attn_force.nw8 : attn_tune_env().nw8; }

// What ctx_attention_core launches for a shape on a device of n_cu CUs under the switches in force: waves per workgroup, key ranges
// per workgroup, workgroups, and the model's wave-tiles on the busiest SIMD (attn_plan).  Host only.
extern "C" int32_t ctx_attention_plan(int32_t B, int32_t Sq, int32_t Skv, int32_t heads, int32_t n_cu, int32_t *out)
{
    CTX_REQUIRE(out && B > 0 && Sq > 0 && Skv > 0 && heads > 0 && n_cu > 0, "attention plan: bad arguments");
    const AttnPlan p = attn_plan(B, Sq, Skv, heads, n_cu, attn_nw8());
    out[0] = p.nw; out[1] = p.ks; out[2] = p.wgs; out[3] = p.cost;
    return CTX_OK;
}

int ctx_attention_core(const f16 *Q, const f16 *K, const f16 *V, int B, int Sq, int Skv, int heads, int q_stride,
                       int kv_stride, float scale, f16 *O, int o_stride, hipStream_t s)
{
    AttnArgs a;
    a.Q = Q; a.K = K; a.V = V; a.O = O; a.Sq = Sq; a.Skv = Skv; a.heads = heads;
    a.q_stride = q_stride; a.kv_stride = kv_stride; a.o_stride = o_stride;
    a.scale_log2e = scale * 1.4426950408889634f;
    const AttnTune &tu = attn_tune_env();
    const float lazy = g_attn_force.lazy >= 0.f ? g_attn_force.lazy : tu.lazy;
    a.lazy = lazy >= 0.f && lazy <= 12.f ? lazy : 8.0f;
    const int ns = g_attn_force.ns >= 0 ? g_attn_force.ns : tu.ns;
    // 8-wave workgroups (two per CU at 128 VGPRs) measured against three 4-wave ones (148 VGPRs): 72 vs 77 us at 2304 tokens
    // x 10 heads, 411 vs 371 us at 9216 x 5 (CTX_ATTN_NW8: 0 always 4 waves, 1 always 8, 2 always the K/V split, else attn_plan)
    const AttnPlan plan = attn_plan(B, Sq, Skv, heads, attn_cu_count(), attn_nw8());
    const int spread = g_attn_force.spread >= 0 ? g_attn_force.spread : tu.spread;
    static int dbg = -1;                                            // CTX_ATTN_DEBUG: the first launch reports its kernel's occupancy
    bool report = false;
    if (dbg < 0) { dbg = ctx_env_int("CTX_ATTN_DEBUG", 0); report = dbg != 0; }
    if (plan.ks == 2) {
        if (ns == 2) attn_launch<2, 12, true, 2>(a, B, report, s); else if (ns == 4) attn_launch<4, 12, true, 2>(a, B, report, s);
        else if (spread) attn_launch<3, 12, true, 2>(a, B, report, s); else attn_launch<3, 12, false, 2>(a, B, report, s);
    } else if (plan.nw == 8) {
        if (ns == 2) attn_launch<2, 8>(a, B, report, s); else if (ns == 4) attn_launch<4, 8>(a, B, report, s);
        else if (spread) attn_launch<3, 8>(a, B, report, s); else attn_launch<3, 8, false>(a, B, report, s);
    } else {
        if (ns == 2) attn_launch<2, 4>(a, B, report, s); else if (ns == 4) attn_launch<4, 4>(a, B, report, s);
        else if (spread) attn_launch<3, 4>(a, B, report, s); else attn_launch<3, 4, false>(a, B, report, s);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        ctx_set_error("attention launch failed: %s", hipGetErrorString(e));
        return CTX_E_LAUNCH;
    }
    return CTX_OK;
}

extern "C" int64_t ctx_attention_ws_bytes(int32_t B, int32_t Skv, int32_t heads)
{
    (void)B; (void)Skv; (void)heads;
    return 256;                                   // no workspace is needed any more (V is consumed untransposed); kept for callers
}

extern "C" int32_t ctx_attention_f16(const void *Q, const void *K, const void *V, int32_t B, int32_t Sq, int32_t Skv,
                                     int32_t heads, int32_t q_stride, int32_t kv_stride, float scale, void *O,
                                     int32_t o_stride, void *vt_ws, ctx_stream_t stream)
{
    (void)vt_ws;
    CTX_REQUIRE(Q && K && V && O, "attention: null pointer");
    CTX_REQUIRE(B > 0 && Sq > 0 && Skv > 0 && heads > 0 && q_stride % 8 == 0 && kv_stride % 8 == 0 && o_stride % 4 == 0 &&
                    q_stride >= heads * 64 && kv_stride >= heads * 64 && o_stride >= heads * 64,
                "attention: bad strides/sizes (head_dim is fixed at 64)");
    // the DMA source of a lane is a tile's base plus a 32-bit byte offset of up to 63 rows
    CTX_REQUIRE(kv_stride < (1 << 24), "attention: kv_stride %d is beyond the 2^24 elements the tile addressing holds", kv_stride);
    return ctx_attention_core((const f16 *)Q, (const f16 *)K, (const f16 *)V, B, Sq, Skv, heads, q_stride, kv_stride, scale, (f16 *)O,
                              o_stride, (hipStream_t)stream);
}
