// fp16 MFMA GEMM / implicit-GEMM 3x3 convolution for the UNet denoiser (gfx950), small and medium tiles.
//
//   out[M,N] = X[M,K] . Wt[N,K]^T  (+bias[N]) (+rowbias[row/rows_per_batch, N]) (+residual[M,N])
//
// Replaces the cuDNN/cuBLAS conv2d / linear calls under diffusers' UNet2DConditionModel
// (reference call site src/stable_diffusion_depth.py:422-423).  fp16 operands, fp32 accumulate.
//
// One kernel template, k_gemm_pipe<WM, WN, MI, NI, CONV, NS, PKT>: WM x WN waves, each owning MI x NI accumulators of
// v_mfma_f32_32x32x16_f16.  The WEIGHT fragment is the A operand and the ACTIVATION fragment the B operand, so a lane
// owns one output row (token / pixel) and its registers walk the features.  Operand tiles go global -> LDS by
// global_load_lds_dwordx4 into a ring of NS K-stages (PKT deep), one raw s_barrier per stage and a counted vmcnt so the
// newer stages stay in flight.  What limits these layers is how many bytes per clock a CU can stage (about 1 KiB per
// ~120 cycles per issuing wave, ~30 B/clk per CU), not the matrix pipe: the tile list below trades flop per staged
// byte (big tiles) against waves that issue (small problems want 4-8 waves even on a 64x64 tile).  The conv variant
// only changes the activation address generator (im2col on the fly, NHWC, zero padding by pointing at a zero page,
// optional fused nearest x2 upsample and stride 2).  The large layers go to gemm8.hip (256x256, 8 staggered waves).
#include "gemm_common.h"

// Direct epilogue (GEGLU, or when strides are not 16-byte friendly): lane owns row m, registers walk n.
// PH (both epilogues): the phase form; rows are masked against the phase's row count and stored through conv_phase_row
template <int MI, int NI, bool PH = false>
__device__ __forceinline__ void gemm_epilogue(const GemmArgs &a, f32x16 (&acc)[MI][NI], int mw, int nw, int r, int h, const ConvPhase &ph)
{
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        int m = mw + mi * 32 + r;
        if (m >= ph.M) continue;
        const int mo = PH ? conv_phase_row(a, ph, m) : m;
        int bidx = a.rowbias ? m / a.rows_per_batch : 0;
        if (a.epi == 1) {
            if constexpr (NI == 2) {
                // GEGLU: ni=0 -> value half, ni=1 -> gate half of the same 32 features (packed weight order)
                int fbase = nw / 2;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    int nn = nw + 8 * g + 4 * h;       // packed column of the value half
                    if (nn >= a.N) continue;
                    f16x4 o;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float xv = acc[mi][0][4 * g + j], gv = acc[mi][1][4 * g + j];
                        if (a.bias) { xv += (float)a.bias[nn + j]; gv += (float)a.bias[nn + 32 + j]; }
                        o[j] = geglu(xv, gv);
                    }
                    *(f16x4 *)(a.out + (size_t)m * a.ldc + fbase + 8 * g + 4 * h) = o;
                }
            }
        } else {
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    int nn = nw + ni * 32 + 8 * g + 4 * h;
                    if (nn >= a.N) continue;
                    f32x4 v = acc4(acc[mi][ni], g);
                    store4<true>(a, bias4(a, v, nn), mo, bidx, nn);
                }
        }
    }
}

// Epilogue through LDS: the accumulator layout gives every lane one token row and 4-feature pieces, i.e. 8-byte
// accesses scattered over 32 cache lines per wave instruction, for the store AND for the residual read.  Each wave
// instead parks 32 rows x (32 NI) features of fp32 in its own LDS patch (row stride 32 NI + 4 floats: conflict-free
// ds_write_b128) and walks it back in whole rows: bias / row bias / residual / output all move as 64- or 128-byte
// row segments, 16 bytes per lane, and the sum is still rounded to fp16 exactly once.
template <int MI, int NI, bool PH = false>
__device__ __forceinline__ void gemm_epilogue_staged(const GemmArgs &a, f32x16 (&acc)[MI][NI], int mw, int nw, int r, int h,
                                                     float *stage, int lane, const ConvPhase &ph)
{
    constexpr int RS = 32 * NI + 4;                    // patch row stride (floats)
    constexpr int LPR = 4 * NI;                        // lanes per row (8 features each)
    constexpr int RPP = 64 / LPR;                      // rows per pass
    const int prow = lane / LPR, c8 = (lane % LPR) * 8;
    const int n = nw + c8;
    f16x8 bs = {0, 0, 0, 0, 0, 0, 0, 0};
    if (a.bias && n < a.N) bs = *(const f16x8 *)(a.bias + n);
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *(f32x4 *)(stage + r * RS + ni * 32 + 8 * g + 4 * h) = acc4(acc[mi][ni], g);
#pragma unroll
        for (int p = 0; p < 32 / RPP; ++p) {
            const int row = RPP * p + prow;
            const int m = mw + mi * 32 + row;
            f32x4 v0 = *(const f32x4 *)(stage + row * RS + c8), v1 = *(const f32x4 *)(stage + row * RS + c8 + 4);
            if (m < ph.M && n < a.N) {
                float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                add8(v, bs);
                if (a.bias2) add8(v, *(const f16x8 *)(a.bias2 + n));
                store8<true>(a, v, PH ? conv_phase_row(a, ph, m) : m, n);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Pipelined LDS-DMA variant: K-stages of 32, ring of NS stages, prefetch distance NS-1, ONE raw s_barrier per
// stage and a counted s_waitcnt vmcnt so the newer stages' DMA stays in flight across the barrier.
//   iteration kt:  vmcnt((NS-2)*G)  -> this wave's pieces of stage kt have landed
//                  s_barrier        -> everybody's pieces landed AND everybody finished stage kt-1
//                  issue stage kt+NS-1 into the buffer stage kt-1 used
//                  8 x MFMA on stage kt
// 64-byte LDS rows ([rows][32 f16]), chunk swizzle c ^ ((row>>2)&3) applied on the DMA source address and on the
// fragment read (conflict-free ds_read_b128 under the 64-bank / 16-lane-group rule).
// PH: the upsample's phase form (GemmArgs::phase): 4 taps with the shifts of the tile's phase, that phase's weight matrix, and the row
// remap in the epilogues; the other instantiations compile to what they were
template <int WM, int WN, int MI, int NI, bool CONV, int NS, int PKT, bool PH = false>
__global__ __launch_bounds__(64 * WM * WN) void k_gemm_pipe(GemmArgs a)
{
    constexpr int BM = 32 * MI * WM, BN = 32 * NI * WN, NW = WM * WN;
    constexpr int RP = 512 / PKT;                   // rows per 1-KiB DMA piece (16 x 64 B or 8 x 128 B)
    constexpr int LPR = PKT / 8;                    // lanes (16-B chunks) per row
    constexpr int XI = BM / (RP * NW), WI = BN / (RP * NW);   // DMA pieces per wave per stage
    static_assert(XI >= 1 && WI >= 1, "tile too small for the wave count");
    constexpr int G = XI + WI;
    constexpr int STAGE = (BM + BN) * PKT;           // f16 per stage
    extern __shared__ __attribute__((aligned(16))) f16 smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform by construction: SGPR, scalar branches
    const int r = lane & 31, h = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
    // 1-D grid of tiles x K-slices, slice-major, cut into 8 contiguous runs (one per XCD: blocks b and b+8 share an L2):
    // an XCD then streams ~1/8 of the K range of both operands.  Inside a slice the tile order walks the operand that is
    // re-read most (mfast: consecutive blocks share the weight panel; else the activation panel).
    const GemmTile t = gemm_tile(a, blockIdx.x, PKT, BM, BN);
    static_assert(!PH || CONV, "the phase form is a convolution");
    const ConvPhase ph = PH ? conv_phase_tile(a, t.tile_m, BM) : ConvPhase{0, 0, 0, t.m0, a.M};
    const int slice = t.slice, tile_m = t.tile_m, tile_n = t.tile_n, m0 = ph.m0, n0 = t.n0, kbeg = t.kbeg, nk = t.nk;
    const int ldw = CONV ? (PH ? 4 : 9) * a.Cin : a.K;             // weight row stride
    const f16 *const Wt = PH ? a.Wt + (size_t)ph.ph * a.N * ldw : a.Wt;
    const int lr = lane / LPR, pc = lane % LPR;        // row within the piece's 16 rows, physical 16-B chunk

    // ---- issue-side state: one running source pointer per DMA piece (advanced by a fixed step per stage; rows that
    // are out of range / conv padding point at a zero page with step 0), so a stage costs G loads + G pointer adds
    const f16 *xp[XI], *wp[WI];
    int xst[XI], wst[WI];
    int xoff[XI], xoy[XI], xox[XI];
    bool xok[XI];
#pragma unroll
    for (int i = 0; i < XI; ++i) {
        int row = RP * (wave + NW * i) + lr;
        int m = m0 + row;
        const int lc = (pc ^ (PKT == 32 ? ((row >> 2) & 3) : ((row >> 1) & 7))) * 8;
        xok[i] = m < ph.M;
        if (CONV) {
            conv_pixel(a, m, lc, xoy[i], xox[i], xoff[i]);
            xp[i] = ctx_zero_page; xst[i] = 0;
        } else {
            xoff[i] = 0; xoy[i] = 0; xox[i] = 0;
            xp[i] = xok[i] ? a.X + (size_t)m * a.K + kbeg * PKT + lc : ctx_zero_page;
            xst[i] = xok[i] ? PKT : 0;
        }
    }
#pragma unroll
    for (int i = 0; i < WI; ++i) {
        int row = RP * (wave + NW * i) + lr;
        bool ok = (n0 + row) < a.N;
        wp[i] = ok ? Wt + (size_t)(n0 + row) * ldw + kbeg * PKT + ((pc ^ (PKT == 32 ? ((row >> 2) & 3) : ((row >> 1) & 7))) * 8) : ctx_zero_page;
        wst[i] = ok ? PKT : 0;
    }
    // K rotation: workgroups that stream the same weight rows (same tile_n) or the same activation rows (same tile_m)
    // start at different K offsets and wrap, so at any instant they hit different cache lines / L2 channels.
    const int k_lo = kbeg * PKT, k_hi = (kbeg + nk) * PKT;
    // (never with K segments: the wrap below steps back inside ONE weight matrix)
    const int rot = a.krot == 1 && !a.nseg ? (int)(((unsigned)tile_m * 13u + (unsigned)tile_n * 5u) % (unsigned)nk) : 0;
    int k_issue = k_lo + rot * PKT, issued = 0, tap_left = 0;
    if (!CONV) {
#pragma unroll
        for (int i = 0; i < XI; ++i) xp[i] += (xst[i] ? rot * PKT : 0);
    }
#pragma unroll
    for (int i = 0; i < WI; ++i) wp[i] += (wst[i] ? rot * PKT : 0);

    auto retap = [&]() {                            // CONV: new 3x3 tap -> recompute the activation pointers
        // ... or a K segment: its tensor has the output's pixel grid, so the lane's pixel is row m of it, read as a centre tap
        const bool seg = a.nseg && k_issue >= 9 * a.Cin;
        const ConvSrc cs = conv_stage_src(a, k_issue);
        const int sg = cs.src - 9;
        const ConvTap tap = PH ? conv_phase_tap(a, ph, k_issue) : conv_tap(a, seg ? 4 * a.Cin : k_issue);
        unsigned lox = 0;
        if (seg) {
            // a piece's rows start at a multiple of RP and the wave count is even wherever a stage is 64 deep, so the lane's
            // swizzled chunk is that of its row in piece 0 for every piece: one per-lane offset for all of them
            static_assert(PKT == 32 || NW % 2 == 0, "the chunk swizzle must not depend on the piece");
            const int ln = conv_seg_lane(lane), lr = ln / LPR, row0 = RP * wave + lr;
            lox = (unsigned)(lr * cs.C + ((ln % LPR) ^ (PKT == 32 ? ((row0 >> 2) & 3) : ((row0 >> 1) & 7))) * 8);
            const ConvWJump wj = conv_seg_wjump(a, sg, cs.c0, k_issue, sg == 0 || issued == 0);
#pragma unroll
            for (int i = 0; i < WI; ++i) {
                const long step = wj.jump + ((long)(n0 + RP * (wave + NW * i)) * wj.dld + lr * wj.dld) * (long)sizeof(f16);
                wp[i] = (const f16 *)((const char *)wp[i] + (wst[i] ? step : 0));
            }
        }
#pragma unroll
        for (int i = 0; i < XI; ++i) {
            bool ok = xok[i];
            xp[i] = conv_tap_src<true>(a, tap, xoy[i], xox[i], xoff[i], ok, seg ? conv_seg_x(a, sg, m0 + RP * (wave + NW * i), cs.c0) + lox : nullptr);
            xst[i] = ok ? PKT : 0;
        }
        tap_left = (cs.C - cs.c0) / PKT;
    };
    auto issue = [&](int buf) {
        if (k_issue == k_hi) {                       // wrap of the rotated K range
            k_issue = k_lo;
            const int span = k_hi - k_lo;
            if (!CONV) {
#pragma unroll
                for (int i = 0; i < XI; ++i) xp[i] -= (xst[i] ? span : 0);
            }
#pragma unroll
            for (int i = 0; i < WI; ++i) wp[i] -= (wst[i] ? span : 0);
            tap_left = 0;
        }
        if (CONV) {
            if (tap_left == 0) retap();
            --tap_left;
        }
        f16 *Xs = smem + buf * STAGE;
        f16 *Ws = Xs + BM * PKT;
#pragma unroll
        for (int i = 0; i < XI; ++i) {
            __builtin_amdgcn_global_load_lds((gptr_t)xp[i], (lptr_t)(Xs + (wave + NW * i) * 512), 16, 0, 0);
            xp[i] += xst[i];
        }
#pragma unroll
        for (int i = 0; i < WI; ++i) {
            __builtin_amdgcn_global_load_lds((gptr_t)wp[i], (lptr_t)(Ws + (wave + NW * i) * 512), 16, 0, 0);
            wp[i] += wst[i];
        }
        k_issue += PKT;
        ++issued;
    };

    f32x16 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

#pragma unroll
    for (int p = 0; p < NS - 1; ++p)
        if (p < nk) issue(p);
    const int swz = PKT == 32 ? ((r >> 2) & 3) : ((r >> 1) & 7);
    const int xrow = (wm * 32 * MI + r) * PKT, wrow = BM * PKT + (wn * 32 * NI + r) * PKT;
    int kt = 0;
    // steady groups of NS stages: every stage of the group still issues a stage NS-1 ahead, so exactly NS-2 newer stages are in
    // flight at each wait — none of the wave-uniform branches of the general form below (about ten s_cbranch per stage in the ISA)
    for (; a.krot == 0 && kt + 2 * NS - 2 < nk; kt += NS) {
#pragma unroll
        for (int u = 0; u < NS; ++u) {
            // lgkmcnt(0): the barrier does not wait for LDS reads in flight, and the stage issued right after it lands in the
            // buffer the previous stage's fragments were read from (hipcc sinks those reads' MFMAs below the barrier when it can)
            asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((NS - 2) * G) : "memory");
            ctx_barrier();
            issue((u + NS - 1) % NS);
            const f16 *sb = smem + u * STAGE;
#pragma unroll
            for (int ks = 0; ks < PKT / 16; ++ks) {
                const int pch = ((2 * ks + h) ^ swz) * 8;
                f16x8 xf[MI], wf[NI];
#pragma unroll
                for (int i = 0; i < MI; ++i) xf[i] = *(const f16x8 *)(sb + xrow + i * 32 * PKT + pch);
#pragma unroll
                for (int j = 0; j < NI; ++j) wf[j] = *(const f16x8 *)(sb + wrow + j * 32 * PKT + pch);
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[j], xf[i], acc[i][j], 0, 0, 0);
            }
        }
    }
    for (; kt < nk; kt += NS) {
#pragma unroll
        for (int u = 0; u < NS; ++u) {
            if (kt + u < nk) {
                // pieces still allowed in flight after this wait: those of the (up to NS-2) newer issued stages
                int newer = issued - 1 - (kt + u);
                if (NS >= 8 && newer >= 6) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(6 * G) : "memory");
                else if (NS >= 7 && newer >= 5) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(5 * G) : "memory");
                else if (NS >= 6 && newer >= 4) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * G) : "memory");
                else if (NS >= 5 && newer >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * G) : "memory");
                else if (NS >= 4 && newer >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * G) : "memory");
                else if (newer >= 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G) : "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // see the steady loop
                ctx_barrier();
                if (issued < nk) issue((u + NS - 1) % NS);
                const f16 *sb = smem + u * STAGE;
#pragma unroll
                for (int ks = 0; ks < PKT / 16; ++ks) {
                    const int pch = ((2 * ks + h) ^ swz) * 8;
                    f16x8 xf[MI], wf[NI];
#pragma unroll
                    for (int i = 0; i < MI; ++i) xf[i] = *(const f16x8 *)(sb + xrow + i * 32 * PKT + pch);
#pragma unroll
                    for (int j = 0; j < NI; ++j) wf[j] = *(const f16x8 *)(sb + wrow + j * 32 * PKT + pch);
#pragma unroll
                    for (int i = 0; i < MI; ++i)
#pragma unroll
                        for (int j = 0; j < NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[j], xf[i], acc[i][j], 0, 0, 0);
                }
            }
        }
    }
    if (a.splitk > 1) {
        float *pb = a.part + (size_t)slice * a.M * a.N;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            int m = m0 + wm * 32 * MI + mi * 32 + r;
            if (m >= ph.M) continue;
            const int mo = PH ? conv_phase_row(a, ph, m) : m;
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    store_part4(a, pb + (size_t)mo * a.N, n0 + wn * 32 * NI + ni * 32 + 8 * g + 4 * h, acc4(acc[mi][ni], g));
        }
        return;
    }
    if (a.epi == 0 && a.stage_epi) {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        ctx_barrier();                 // every wave is done reading the ring
        gemm_epilogue_staged<MI, NI, PH>(a, acc, m0 + wm * 32 * MI, n0 + wn * 32 * NI, r, h, (float *)smem + wave * (32 * (32 * NI + 4)), lane, ph);
        return;
    }
    gemm_epilogue<MI, NI, PH>(a, acc, m0 + wm * 32 * MI, n0 + wn * 32 * NI, r, h, ph);
}

// Split-K second pass: out = sum_s part[s] (+bias)(+rowbias)(+residual) -> f16.  Fixed summation order.
__global__ __launch_bounds__(256) void k_splitk_reduce(GemmArgs a)
{
    const int n4 = a.N / 4;
    const size_t total = (size_t)a.M * n4, MN = (size_t)a.M * a.N;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        int m = (int)(i / n4), nn = (int)(i % n4) * 4;
        f32x4 v = *(const f32x4 *)(a.part + (size_t)m * a.N + nn);
        for (int sidx = 1; sidx < a.splitk; ++sidx) {
            f32x4 p = *(const f32x4 *)(a.part + sidx * MN + (size_t)m * a.N + nn);
            v += p;
        }
        v = bias4(a, v, nn);
        store4<true>(a, v, m, a.rowbias ? m / a.rows_per_batch : 0, nn);
    }
}

// The same second pass with a GroupNorm partials request (GemmArgs::gn_part): grid (slots, samples), a block owns RB whole rows of one
// sample and a thread one 4-feature column of them (c4n columns x PL row lanes; blockDim is rounded up to whole waves), so that it can
// sum the fp16 values it stores.  Operand order and rounding are k_splitk_reduce's: the output is bit-identical.  Fold, fixed order:
// thread sums [PL][4][c4n] -> channel sums [N] -> 8 lanes per group and a shuffle tree -> part[b][slot][g].
__global__ __launch_bounds__(1024) void k_splitk_reduce_gn(GemmArgs a, int RB, int PL)
{
    extern __shared__ float2 s_gn[];                               // [PL][4][c4n], then [N]
    const int c4n = a.N / 4, tid = threadIdx.x;
    const int c4 = tid % c4n, pl = tid / c4n, nn = c4 * 4;
    const int b = blockIdx.y, slot = blockIdx.x;
    const size_t MN = (size_t)a.M * a.N;
    float gs[4] = {0.f, 0.f, 0.f, 0.f}, gq[4] = {0.f, 0.f, 0.f, 0.f};
    if (pl < PL) {
        for (int r = pl; r < RB; r += PL) {
            const int m = b * a.gn_hw + slot * RB + r;
            f32x4 v = *(const f32x4 *)(a.part + (size_t)m * a.N + nn);
            for (int sidx = 1; sidx < a.splitk; ++sidx) {
                f32x4 p = *(const f32x4 *)(a.part + sidx * MN + (size_t)m * a.N + nn);
                v += p;
            }
            v = bias4(a, v, nn);
            const f16x4 o = store4<true>(a, v, m, a.rowbias ? m / a.rows_per_batch : 0, nn);
#pragma unroll
            for (int j = 0; j < 4; ++j) { const float f = (float)o[j]; gs[j] += f; gq[j] += f * f; }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) s_gn[(pl * 4 + j) * c4n + c4] = make_float2(gs[j], gq[j]);
    }
    __syncthreads();
    float2 *s_ch = s_gn + PL * 4 * c4n;
    for (int c = tid; c < a.N; c += blockDim.x) {
        const int cell = (c & 3) * c4n + (c >> 2);
        float ss = 0.f, qq = 0.f;
        for (int l = 0; l < PL; ++l) { const float2 t = s_gn[l * 4 * c4n + cell]; ss += t.x; qq += t.y; }
        s_ch[c] = make_float2(ss, qq);
    }
    __syncthreads();
    const int cg = a.gn_cg, G = a.N / cg, octs = (int)blockDim.x >> 3;
    for (int g0 = 0; g0 < G; g0 += octs) {
        const int g = g0 + (tid >> 3), l8 = tid & 7;
        float ss = 0.f, qq = 0.f;
        if (g < G)
            for (int k = l8; k < cg; k += 8) { const float2 t = s_ch[g * cg + k]; ss += t.x; qq += t.y; }
#pragma unroll
        for (int o = 4; o > 0; o >>= 1) { ss += __shfl_xor(ss, o, 64); qq += __shfl_xor(qq, o, 64); }
        if (g < G && l8 == 0) *(float2 *)(a.gn_part + (((size_t)b * a.gn_ns + slot) * G + g) * 2) = make_float2(ss, qq);
    }
}

// tile ids (CTX_GEMM_TILE / ctx_gemm_tune): WM x WN waves of MI x NI 32x32 blocks
//   0: 256x128 8w   1: 128x128 4w   2: 256x64 4w   3: 128x64 2w   4: 64x64 1w
//   5: 64x64 4w (32x32 per wave)   6: 64x64 2w (64x32)   7: 128x128 8w (32x64)   8: 64x128 4w (32x64)   9: 128x64 4w (64x32)
//   10-18: 64-deep K stages, ring of 3: 256x128 16w (32x64) | 256x128 16w (64x32) | 256x128 8w | 128x128 16w (32x32) | 128x128 8w |
//          64x64 4w | 64x128 4w | 128x64 4w | 128x128 4w;  19-22: ring of 2: 64x64 4w | 128x128 8w | 128x128 16w | 128x128 4w
//   23-26: deep rings: 64x64 4w x6 | 64x128 4w x5 | 128x128 8w x4 | 128x64 4w x5;  27: 256x320 8w (64x160), ring of 2
static int g_force_tile = -1, g_force_gemm8 = -1;
static int g_last_tile = -1, g_last_use8 = -1;      // what the last dispatch launched (ctx_gemm_last_kernel)
extern "C" void ctx_gemm_tune(int32_t tile, int32_t gemm8)
{
    g_force_tile = tile;            // -1: heuristic
    g_force_gemm8 = gemm8;          // -1: heuristic, 0: never, 1: always when applicable
}

template <int WM, int WN, int MI, int NI, bool CONV, int NS = 4, int PKT = 32, bool PH = false>
static void launch_gemm(GemmArgs &a, hipStream_t s)
{
    constexpr int BM = 32 * MI * WM, BN = 32 * NI * WN;
    a.ntm = PH ? 4 * cdiv(a.M / 4, BM) : cdiv(a.M, BM);              // phase form: whole tiles per phase
    a.ntn = cdiv(a.N, BN);
    if (a.splitk < 1 || !a.part) a.splitk = 1;
    static const int mfast = ctx_env_int("CTX_GEMM_MFAST", -1);
    a.mfast = mfast >= 0 ? mfast : ctx_gemm_mfast(a, CONV);
    static const int stg = ctx_env_int("CTX_GEMM_STAGE_EPI", 1);
    a.stage_epi = stg && (a.ldc % 8 == 0) && (!a.residual || a.ldr % 8 == 0) && (!a.rowbias || a.ldrb % 8 == 0) &&
                  (size_t)WM * WN * 32 * (32 * NI + 4) * sizeof(float) <= 160 * 1024;       // the per-wave fp32 patch must fit the LDS
    static const int steady = ctx_env_int("CTX_GEMM_STEADY", 1);
    a.pk = PKT; a.krot = steady ? 0 : 2;                 // krot = 2: no rotation, general K loop only (A/B switch of the steady loop)
    constexpr int NT = 64 * WM * WN;
    constexpr size_t ring = (size_t)NS * (BM + BN) * PKT * sizeof(f16);
    constexpr size_t patch = (size_t)WM * WN * 32 * (32 * NI + 4) * sizeof(float);
    constexpr size_t lds = (ring > patch || patch > 160 * 1024) ? ring : patch;
    ctx_launch<k_gemm_pipe<WM, WN, MI, NI, CONV, NS, PKT, PH>>(0, dim3(a.ntm * a.ntn * a.splitk), dim3(NT), lds, s, a);
}

static void launch_reduce(GemmArgs &a, hipStream_t s)
{
    if (a.gn_part) {
        // rows per block: the smallest divisor of the sample that leaves <= CTX_GN_MAX_SLOTS slots and ~256 blocks in all
        const int c4n = a.N / 4, hw = a.gn_hw;
        bool ok = !a.res32 && !a.out32 && a.N % 4 == 0 && c4n <= 1024 && hw > 0 && a.M % hw == 0 && a.gn_cg >= 1 && a.N % a.gn_cg == 0 && a.ldc == a.N;
        if (ok) {
            const int B = a.M / hw, want = B >= 2 ? (CTX_GN_MAX_SLOTS < cdiv(256, B) ? CTX_GN_MAX_SLOTS : cdiv(256, B)) : CTX_GN_MAX_SLOTS;
            int rb = cdiv(hw, want);
            while (hw % rb) ++rb;
            const int pl = rb < 1024 / c4n ? rb : 1024 / c4n, threads = cdiv(c4n * pl, 64) * 64;
            a.gn_ns = hw / rb;
            const size_t lds = ((size_t)pl * 4 * c4n + a.N) * sizeof(float2);
            static bool attr = false;
            if (!attr) { (void)hipFuncSetAttribute((const void *)k_splitk_reduce_gn, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024); attr = true; }
            if (ctx_prof_on()) {
                hipEvent_t e0, e1;
                ctx_prof_events(0, &e0, &e1);
                hipExtLaunchKernelGGL(k_splitk_reduce_gn, dim3(a.gn_ns, B), dim3(threads), lds, s, e0, e1, 0, a, rb, pl);
            } else
                hipLaunchKernelGGL(k_splitk_reduce_gn, dim3(a.gn_ns, B), dim3(threads), lds, s, a, rb, pl);
            return;
        }
        a.gn_part = nullptr;                                       // declined: the plain reduce below
    }
    size_t total = (size_t)a.M * (a.N / 4);
    unsigned nb = (unsigned)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    ctx_launch<k_splitk_reduce>(0, dim3(nb), dim3(256), 0, s, a);
}

int ctx_gemm_pick_split(int M, int N, int K, int epi)
{
    static const int en = ctx_env_int("CTX_SPLITK", 1);
    if (!en || epi != 0 || N % 4) return 1;
    bool wide = (N % 128 == 0);
    int tiles = wide ? cdiv(M, 128) * cdiv(N, 128) : cdiv(M, 256) * cdiv(N, 64);
    if (tiles >= 200) return 1;
    if (K < 2048 && tiles > 48) return 1;      // short-K problems: the slab round trip + extra launch costs more than it buys
    int S = 640 / tiles;                       // aim at ~2.5 workgroups per CU
    int maxS = (K / 32) / 8;                   // keep >= 8 stages per split
    if (S > maxS) S = maxS;
    if (S > 32) S = 32;
    return S < 2 ? 1 : S;
}

#include "gemm_tuned.h"
#include "gemm_tuned_phase.h"
void ctx_gemm_plan(GemmArgs &a, bool conv)
{
    a.tile = -1; a.use8 = -1;
    static const int use_table = ctx_env_int("CTX_GEMM_TUNED", 1);
    if (use_table) {
        const int flags = conv ? ((a.stride == 2 ? 1 : 0) | (a.ups ? 2 : 0) | (a.phase ? 4 : 0)) : 0;
        auto match = [&](const TunedGemm &t) { return t.conv == (conv ? 1 : 0) && t.M == a.M && t.N == a.N && t.K == a.K && t.flags == flags && t.epi == a.epi; };
        for (const TunedGemm &t : g_tuned)
            if (match(t)) {
                a.tile = t.tile; a.use8 = t.use8; a.splitk = t.splitk;
                return;
            }
        for (const TunedGemm &t : g_tuned_phase)                    // the phase form's rows (flag bit 2) have a table of their own
            if (match(t)) {
                a.tile = t.tile; a.use8 = t.use8; a.splitk = t.splitk;
                return;
            }
    }
    // shapes outside the table: the rules the plan search kept producing (tools/tune_gemm.py, latents 96 / 64 / 32)
    if (a.K % 64 == 0 && (!conv || a.Cin % 64 == 0)) {
        const double MN = (double)a.M * a.N;
        // Large plain-epilogue problems (other lockstep batch sizes than the tuned 2 and 12, other latent sizes): the 144 x 160 kernel
        // family of gemm144.hip where it has enough tiles to fill the chip and <= 10 % masked waste along N — the 288-row form from ~512
        // tiles on, the software-pipelined 144-row form from ~220 (what the plan search chose for such shapes at batch 2 / 12).
        static const int heur144 = ctx_env_int("CTX_GEMM_HEUR144", 1);    // 0: the r2 rules only (A/B)
        if (heur144 && a.epi == 0 && a.N % 8 == 0 && !a.zins && !a.res32 && !a.out32) {
            const int nt = cdiv(a.N, 160);
            const double fill = (double)a.N / (160.0 * nt);
            if (fill >= 0.9) {                                  // the UNet's widths (multiples of 160); the VAE's 128 / 256 / 512 would mask a fifth of every tile (measured: the SDS loop's VAE passes lose 1.5 ms)
                if (cdiv(a.M, 288) * nt >= 512) { a.tile = -1; a.use8 = 8; a.splitk = 1; return; }
                if (cdiv(a.M, 144) * nt >= 220) { a.tile = -1; a.use8 = 6; a.splitk = 1; return; }
            }
        }
        int tile, bm, bn;
        if (MN >= 5.0e6) { tile = a.epi == 1 ? 10 : (conv ? 12 : 11); bm = 256; bn = 128; }          // 256x128, 8 / 16 waves
        else if ((MN >= 2.5e6 && a.K >= 960) || (conv && MN >= 1.2e6 && a.K >= 5760)) { tile = 14; bm = 128; bn = 128; }
        else if (a.epi == 1) { tile = 16; bm = 64; bn = 128; }                                        // GEGLU needs 64-wide wave tiles
        else { tile = 15; bm = 64; bn = 64; }                                                         // 64x64, 4 waves
        const int tiles = cdiv(a.M, bm) * cdiv(a.N, bn);
        int S = 1;
        if (a.epi == 0 && a.N % 4 == 0) {
            S = 320 / tiles;                                   // ~1.25 workgroups per CU
            const int maxS = a.K / 64 / 4;                     // >= 4 stages per slice
            if (S > maxS) S = maxS;
            if (S > 12) S = 12;
            if (S < 1) S = 1;
        }
        a.tile = tile; a.splitk = S;
        a.use8 = (a.epi == 1 && MN >= 1.0e7) ? -1 : 0;        // the 256x256 kernel only where its own heuristic wants it
        return;
    }
    a.splitk = ctx_gemm_pick_split(a.M, a.N, a.K, a.epi);
}

// Tile choice: the largest tile (most flops per staged byte) that still gives the chip >= ~1.5 workgroups per CU once
// split-K is counted; small problems fall through to tiles with more waves per staged byte.
int ctx_gemm_dispatch(GemmArgs &a, bool conv, hipStream_t s)
{
    bool seg64 = true;                                                       // every K segment is whole 64-deep stages
    if (a.nseg) {
        int kseg = 0;
        bool ok = conv && a.nseg <= CTX_GEMM_MAX_SEG && a.stride == 1 && !a.ups && !a.poff && !a.zins && a.epi == 0;
        for (int i = 0; ok && i < a.nseg; ++i) {
            ok = a.segX[i] && a.segW[i] && a.segC[i] > 0 && a.segC[i] % 32 == 0 && a.segLdw[i] % 8 == 0;
            ok = ok && (int64_t)a.M * a.segC[i] < (1ll << 31) && (int64_t)a.N * a.segLdw[i] < (1ll << 31);
            seg64 = seg64 && a.segC[i] % 64 == 0;
            kseg += a.segC[i];
        }
        if (!ok || a.K != 9 * a.Cin + kseg) {
            ctx_set_error("gemm: K segments need a stride-1 3x3 convolution without upsample and channel counts in multiples of 32");
            return CTX_E_ARG;
        }
    }
    const bool only_pipe = a.zins || a.res32 || a.out32;                     // features of this file's kernel only
    if (only_pipe) a.use8 = 0;
    int want8 = only_pipe ? 0 : (g_force_gemm8 >= 0 ? g_force_gemm8 : a.use8);                // -1: gemm8's own heuristic
    if (a.phase) {
        // The phase form of an upsampling convolution (GemmArgs::phase): bias only, and only the kernels that implement it (gemm144.hip
        // and this file's tiles).  Any other kernel would read the four 2x2 matrices as one nine-tap matrix: a request for one is an error.
        const bool ok = conv && a.Wt && a.ups == 1 && a.stride == 1 && !a.poff && !a.zins && a.epi == 0 && !a.res32 && !a.out32 && !a.rowbias &&
                        !a.residual && !a.nseg && !a.bias2 && !a.gn_part && !a.keep_slabs && a.Cin % 64 == 0 && a.K == 4 * a.Cin && a.M % 4 == 0;
        if (!ok) {
            ctx_set_error("gemm: the phase form takes an upsampling convolution (stride 1, Cin %% 64 == 0) over its phase pack with a bias only");
            return CTX_E_ARG;
        }
        const bool tile_first = g_force_tile >= 0 || (g_force_gemm8 < 0 && a.tile >= 0);      // (want_tile >= 0 below)
        if (!tile_first && want8 >= 1 && want8 <= 3) {
            ctx_set_error("gemm: kernel %d (gemm8.hip / conv_halo.hip) does not implement the phase form", want8);
            return CTX_E_ARG;
        }
        if (want8 < 0) want8 = 0;                                            // gemm8.hip's own heuristic never sees the form
        a.Ho = a.H; a.Wo = a.W; a.ups = 0; a.rows_per_batch = a.H * a.W;    // what the kernels walk: the source grid, stride 1
    }
    const int want_tile = g_force_tile >= 0 ? g_force_tile : (g_force_gemm8 >= 0 ? -1 : a.tile);
    // the kernels of the other files first (each *_try launches and returns 1 when the problem suits it), else this file's tiles
    const bool launched = want_tile < 0 && ((want8 >= 4 && want8 <= 8 && ctx_gemm144_try(a, conv, want8 - 4, s)) ||
                                            (conv && (want8 == 2 || want8 == 3) && ctx_conv_halo_try(a, want8 == 2 ? 2 : 1, s)) ||
                                            (want8 != 0 && want8 < 2 && ctx_gemm8_try(a, conv, want8 == 1, s)));
    g_last_use8 = launched ? (want8 < 0 ? 1 : want8) : 0; g_last_tile = -1;     // want8 -1: only gemm8's own heuristic launches
    if (!launched) {
        static const int big = ctx_env_int("CTX_GEMM_BIG", 1);
        const int S = a.splitk > 1 && a.part ? a.splitk : 1;
        auto wgs = [&](int bm, int bn) { return cdiv(a.M, bm) * cdiv(a.N, bn) * S; };
        const bool n128 = (a.N % 128 == 0);
        int pick;
        static const int bigk = ctx_env_int("CTX_GEMM_BIGK", 1024);
        if (big && a.M >= 8192 && a.N >= 256 && a.K >= bigk) pick = 0;                 // 256x128, 8 waves
        else if (n128 && wgs(128, 128) >= 384) pick = 1;                               // 128x128
        else if (!n128 && wgs(256, 64) >= 384) pick = 2;                               // 256x64
        else if (wgs(128, 64) >= 320) pick = 3;                                        // 128x64, 2 waves
        else if (S > 1) pick = n128 ? 1 : 2;                                           // split-K already spreads it
        else pick = 4;                                                                 // 64x64, 1 wave
        static const int force = ctx_env_int("CTX_GEMM_TILE", -1);
        if (force >= 0) pick = force;
        if (want_tile >= 0) pick = want_tile;
        if (a.epi == 1 && (pick == 5 || pick == 6 || pick == 9 || pick == 11 || pick == 13 || pick == 15 || pick == 17 || pick == 19 || pick == 21 || pick == 23 || pick == 26 || pick == 27)) pick = 1;   // GEGLU needs 64-wide wave tiles
        if (pick >= 10 && (a.K % 64 != 0 || (conv && a.Cin % 64 != 0) || !seg64)) pick = 1;   // 64-deep stages
#define CTX_LAUNCH(WM_, WN_, MI_, NI_) do { if (a.phase) launch_gemm<WM_, WN_, MI_, NI_, true, 4, 32, true>(a, s); else if (conv) launch_gemm<WM_, WN_, MI_, NI_, true>(a, s); else launch_gemm<WM_, WN_, MI_, NI_, false>(a, s); } while (0)
        g_last_tile = pick;
        switch (pick) {
        case 0: CTX_LAUNCH(4, 2, 2, 2); break;
        case 1: CTX_LAUNCH(2, 2, 2, 2); break;
        case 2: CTX_LAUNCH(4, 1, 2, 2); break;
        case 3: CTX_LAUNCH(2, 1, 2, 2); break;
        case 4: CTX_LAUNCH(1, 1, 2, 2); break;
        case 5: CTX_LAUNCH(2, 2, 1, 1); break;
        case 6: CTX_LAUNCH(1, 2, 2, 1); break;
        case 7: CTX_LAUNCH(4, 2, 1, 2); break;
        case 8: CTX_LAUNCH(2, 2, 1, 2); break;
        case 9: CTX_LAUNCH(2, 2, 2, 1); break;
#define CTX_LAUNCH64(WM_, WN_, MI_, NI_) do { if (a.phase) launch_gemm<WM_, WN_, MI_, NI_, true, 3, 64, true>(a, s); else if (conv) launch_gemm<WM_, WN_, MI_, NI_, true, 3, 64>(a, s); else launch_gemm<WM_, WN_, MI_, NI_, false, 3, 64>(a, s); } while (0)
        case 10: CTX_LAUNCH64(8, 2, 1, 2); break;     // 256x128, 16 waves (32x64), 64-deep stages
        case 11: CTX_LAUNCH64(4, 4, 2, 1); break;     // 256x128, 16 waves (64x32)
        case 12: CTX_LAUNCH64(4, 2, 2, 2); break;     // 256x128, 8 waves
        case 13: CTX_LAUNCH64(4, 4, 1, 1); break;     // 128x128, 16 waves (32x32)
        case 14: CTX_LAUNCH64(4, 2, 1, 2); break;     // 128x128, 8 waves (32x64)
        case 15: CTX_LAUNCH64(2, 2, 1, 1); break;     // 64x64, 4 waves (32x32)
        case 16: CTX_LAUNCH64(2, 2, 1, 2); break;     // 64x128, 4 waves (32x64)
        case 17: CTX_LAUNCH64(2, 2, 2, 1); break;     // 128x64, 4 waves (64x32)
        case 18: CTX_LAUNCH64(2, 2, 2, 2); break;     // 128x128, 4 waves
#define CTX_LAUNCH64N2(WM_, WN_, MI_, NI_) do { if (a.phase) launch_gemm<WM_, WN_, MI_, NI_, true, 2, 64, true>(a, s); else if (conv) launch_gemm<WM_, WN_, MI_, NI_, true, 2, 64>(a, s); else launch_gemm<WM_, WN_, MI_, NI_, false, 2, 64>(a, s); } while (0)
        case 19: CTX_LAUNCH64N2(2, 2, 1, 1); break;   // ring of 2 (half the LDS, more workgroups per CU): 64x64, 4 waves
        case 20: CTX_LAUNCH64N2(4, 2, 1, 2); break;   // 128x128, 8 waves
        case 21: CTX_LAUNCH64N2(4, 4, 1, 1); break;   // 128x128, 16 waves
        case 22: CTX_LAUNCH64N2(2, 2, 2, 2); break;   // 128x128, 4 waves
        // deep rings (one workgroup per CU, 4-5 stages in flight) for the weight-streaming layers of the two deepest levels,
        // whose few workgroups wait on HBM latency rather than on staging bandwidth
#define CTX_LAUNCH64NS(NS_, WM_, WN_, MI_, NI_) do { if (a.phase) launch_gemm<WM_, WN_, MI_, NI_, true, NS_, 64, true>(a, s); else if (conv) launch_gemm<WM_, WN_, MI_, NI_, true, NS_, 64>(a, s); else launch_gemm<WM_, WN_, MI_, NI_, false, NS_, 64>(a, s); } while (0)
        case 23: CTX_LAUNCH64NS(6, 2, 2, 1, 1); break;   // 64x64, 4 waves, ring of 6
        case 24: CTX_LAUNCH64NS(5, 2, 2, 1, 2); break;   // 64x128, 4 waves, ring of 5
        case 25: CTX_LAUNCH64NS(4, 4, 2, 1, 2); break;   // 128x128, 8 waves, ring of 4
        case 26: CTX_LAUNCH64NS(5, 2, 2, 2, 1); break;   // 128x64, 4 waves, ring of 5
        default: CTX_LAUNCH64N2(4, 2, 2, 5); break;      // 27: 256x320, 8 waves (64x160 each), ring of 2: 142 FLOP per staged byte (the lockstep batch)
#undef CTX_LAUNCH64NS
#undef CTX_LAUNCH64N2
#undef CTX_LAUNCH64
        }
#undef CTX_LAUNCH
    }
    // a GroupNorm partials request: served by a gemm144.hip tile's epilogue (it accepted or cleared the request itself) or, behind
    // split-K, by the reduce; no other tile takes it
    if (a.gn_part && a.splitk <= 1 && !(launched && want8 >= 4)) a.gn_part = nullptr;
    if (a.keep_slabs && a.splitk <= 1) {
        ctx_set_error("gemm: the slabs were to be kept but the launch did not split K");
        return CTX_E_STATE;
    }
    if (a.splitk > 1 && !a.keep_slabs) launch_reduce(a, s);                  // every kernel above leaves fp32 partials then
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        ctx_set_error("gemm launch failed: %s", hipGetErrorString(e));
        return CTX_E_LAUNCH;
    }
    return CTX_OK;
}

// Which kernel the last GEMM / conv dispatch of this process launched: *use8 as ctx_gemm_tune's second argument (0 = a tile of
// gemm.hip, whose id goes to *tile; else *tile = -1).  For tests of the forcing and of the fall-through when a kernel declines.
extern "C" void ctx_gemm_last_kernel(int32_t *tile, int32_t *use8)
{
    if (tile) *tile = g_last_tile;
    if (use8) *use8 = g_last_use8;
}

extern "C" int32_t ctx_gemm_f16(const void *A, const void *Wt, const void *bias, const void *residual, int32_t M,
                                int32_t N, int32_t K, void *C, ctx_stream_t stream)
{
    CTX_REQUIRE(A && Wt && C, "gemm: null pointer");
    CTX_REQUIRE(M > 0 && N > 0 && K > 0 && K % 64 == 0 && N % 8 == 0, "gemm: need K%%64==0, N%%8==0 (M=%d N=%d K=%d)", M, N, K);
    CTX_REQUIRE((int64_t)M * K < (1ll << 31) && (int64_t)N * K < (1ll << 31), "gemm: operand too large for 32-bit offsets");
    GemmArgs a = {};
    a.X = (const f16 *)A; a.Wt = (const f16 *)Wt; a.bias = (const f16 *)bias; a.residual = (const f16 *)residual;
    a.out = (f16 *)C; a.M = M; a.N = N; a.K = K; a.ldc = N; a.ldr = N; a.rows_per_batch = 1; a.ldrb = N; a.epi = 0;
    a.tile = -1; a.use8 = -1;
    return ctx_gemm_dispatch(a, false, (hipStream_t)stream);
}

extern "C" int32_t ctx_conv3x3_f16(const void *x, const void *w, const void *bias, const void *rowbias,
                                   const void *residual, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                                   int32_t stride, int32_t upsample, void *y, ctx_stream_t stream)
{
    CTX_REQUIRE(x && w && y, "conv3x3: null pointer");
    CTX_REQUIRE(B > 0 && H > 0 && W > 0 && Cin % 64 == 0 && Cout % 8 == 0 && (stride == 1 || stride == 2) &&
                    (upsample == 0 || upsample == 1) && !(upsample && stride == 2),
                "conv3x3: need Cin%%64==0, Cout%%8==0, stride 1|2 (B=%d H=%d W=%d Cin=%d Cout=%d s=%d up=%d)", B, H, W, Cin, Cout, stride, upsample);
    GemmArgs a = {};
    int Hv = H << upsample, Wv = W << upsample;
    a.Ho = (Hv + 2 - 3) / stride + 1; a.Wo = (Wv + 2 - 3) / stride + 1;
    a.X = (const f16 *)x; a.Wt = (const f16 *)w; a.bias = (const f16 *)bias; a.rowbias = (const f16 *)rowbias;
    a.residual = (const f16 *)residual; a.out = (f16 *)y;
    a.M = B * a.Ho * a.Wo; a.N = Cout; a.K = 9 * Cin; a.ldc = Cout; a.ldr = Cout; a.rows_per_batch = a.Ho * a.Wo; a.ldrb = Cout; a.epi = 0;
    a.H = H; a.W = W; a.Cin = Cin; a.stride = stride; a.ups = upsample;
    a.tile = -1; a.use8 = -1;
    CTX_REQUIRE((int64_t)B * H * W * Cin < (1ll << 31) && (int64_t)Cout * a.K < (1ll << 31), "conv3x3: tensor too large for 32-bit offsets");
    return ctx_gemm_dispatch(a, true, (hipStream_t)stream);
}

// The resnet's second convolution with its 1x1 shortcut folded in as K segments (diffusers ResnetBlock2D.forward:
// conv_shortcut(input_tensor) + conv2(hidden_states); reference call site src/stable_diffusion_depth.py:422-423):
//   y = conv3x3(x; w) + xa wa^T (+ xb wb^T) + bias (+ bias2) (+ rowbias) (+ residual), fp32 sum, one rounding.
// xa / xb: [B, H, W, Ca / Cb] on x's pixel grid; wa / wb: [Cout] rows of Ca / Cb weights, row strides ldwa / ldwb; xb null = one segment.
// splitk: 1 none, > 1 that many slices, < 0 what the engine would plan for the 3x3 part; `part` holds splitk * M * Cout floats (with
// splitk < 0: 32 * M * Cout) or is null (no split).  Honours ctx_gemm_tune.
extern "C" int32_t ctx_conv3x3_seg_f16(const void *x, const void *w, const void *bias, const void *bias2, const void *rowbias,
                                       const void *residual, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, const void *xa,
                                       const void *wa, int32_t Ca, int32_t ldwa, const void *xb, const void *wb, int32_t Cb, int32_t ldwb,
                                       void *part, int32_t splitk, void *y, ctx_stream_t stream)
{
    CTX_REQUIRE(x && w && y && xa && wa, "conv3x3_seg: null pointer");
    CTX_REQUIRE(B > 0 && H > 0 && W > 0 && Cin % 32 == 0 && Cout % 8 == 0, "conv3x3_seg: need Cin%%32==0, Cout%%8==0 (Cin=%d Cout=%d)", Cin, Cout);
    GemmArgs a = {};
    a.Ho = H; a.Wo = W;
    a.X = (const f16 *)x; a.Wt = (const f16 *)w; a.bias = (const f16 *)bias; a.bias2 = (const f16 *)bias2; a.rowbias = (const f16 *)rowbias;
    a.residual = (const f16 *)residual; a.out = (f16 *)y;
    a.M = B * H * W; a.N = Cout; a.K = 9 * Cin; a.ldc = Cout; a.ldr = Cout; a.rows_per_batch = H * W; a.ldrb = Cout;
    a.H = H; a.W = W; a.Cin = Cin; a.stride = 1;
    a.tile = -1; a.use8 = -1;
    if (splitk < 0 && part) ctx_gemm_plan(a, true); else a.splitk = splitk;      // the plan of the 3x3 part's shape
    a.part = (float *)part;
    a.nseg = xb ? 2 : 1;
    a.segX[0] = (const f16 *)xa; a.segW[0] = (const f16 *)wa; a.segC[0] = Ca; a.segLdw[0] = ldwa;
    a.segX[1] = (const f16 *)xb; a.segW[1] = (const f16 *)wb; a.segC[1] = xb ? Cb : 0; a.segLdw[1] = ldwb;
    a.K += a.segC[0] + a.segC[1];
    CTX_REQUIRE((int64_t)a.M * (Cin > Ca + Cb ? Cin : Ca + Cb) < (1ll << 31) && (int64_t)Cout * a.K < (1ll << 31), "conv3x3_seg: tensor too large for 32-bit offsets");
    return ctx_gemm_dispatch(a, true, (hipStream_t)stream);
}

// A 3x3 convolution in any geometry the engines use (test seam): GemmArgs as engine_conv3 fills them, so the VAE's downsampler
// forward (stride 2, poff 1: diffusers' F.pad(x, (0,1,0,1))) and its input gradient (upsample 1, zins 1, poff -1: the zero-inserted
// grid) can be run one kernel at a time.  splitk / part as ctx_conv3x3_seg_f16 (no part: no split).  Honours ctx_gemm_tune.
extern "C" int32_t ctx_conv3x3_geom_f16(const void *x, const void *w, const void *bias, const void *residual, int32_t B, int32_t H, int32_t W,
                                        int32_t Cin, int32_t Cout, int32_t stride, int32_t upsample, int32_t poff, int32_t zins, void *part,
                                        int32_t splitk, void *y, ctx_stream_t stream)
{
    CTX_REQUIRE(x && w && y, "conv3x3_geom: null pointer");
    CTX_REQUIRE(B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && Cin % 64 == 0 && Cout % 8 == 0 && (stride == 1 || stride == 2) &&
                    (upsample == 0 || upsample == 1) && !(upsample && stride == 2),
                "conv3x3_geom: need Cin%%64==0, Cout%%8==0, stride 1|2 (B=%d H=%d W=%d Cin=%d Cout=%d s=%d up=%d)", B, H, W, Cin, Cout, stride, upsample);
    CTX_REQUIRE(zins == 0 || (zins == 1 && upsample == 1 && stride == 1), "conv3x3_geom: the zero-inserted grid needs upsample 1 and stride 1");
    CTX_REQUIRE(poff >= -1 && poff <= 1, "conv3x3_geom: poff %d is outside -1 .. 1", poff);
    CTX_REQUIRE(poff != 1 || (H % 2 == 0 && W % 2 == 0), "conv3x3_geom: poff 1 (padding on the bottom / right only) needs even H and W (H=%d W=%d)", H, W);
    CTX_REQUIRE(splitk != 0 && splitk <= 32 && (splitk <= 1 || splitk <= 9 * Cin / 64), "conv3x3_geom: splitk %d (1 .. min(32, K / 64), or < 0 for the plan)", splitk);
    GemmArgs a = {};
    ctx_conv3_problem(a, B, H, W, Cin, Cout, stride, upsample, poff, zins);
    a.X = (const f16 *)x; a.Wt = (const f16 *)w; a.bias = (const f16 *)bias; a.residual = (const f16 *)residual; a.out = (f16 *)y;
    a.ldrb = Cout;
    a.tile = -1; a.use8 = -1;
    CTX_REQUIRE((int64_t)B * H * W * Cin < (1ll << 31) && (int64_t)Cout * a.K < (1ll << 31) && (int64_t)B * a.Ho * a.Wo * Cout < (1ll << 31),
                "conv3x3_geom: tensor too large for 32-bit offsets");
    if (splitk < 0 && part) ctx_gemm_plan(a, true); else a.splitk = part && splitk > 1 ? splitk : 1;
    a.part = (float *)part;
    return ctx_gemm_dispatch(a, true, (hipStream_t)stream);
}

// The upsampling convolution in its phase form (test seam; GemmArgs::phase): nearest x2 upsample of x [B,H,W,Cin] and a pad-1 3x3
// convolution, computed as four 2x2 convolutions over x with the pack wp [4][Cout][2][2][Cin] of ctx_pack_conv3_phase_f16 -> y
// [B,2H,2W,Cout].  The form takes a bias only: rowbias / residual are here to be refused (CTX_E_ARG, nothing launched), as is a null
// pack.  splitk / part as ctx_conv3x3_geom_f16 (splitk <= min(32, 4 Cin / 64)).  Honours ctx_gemm_tune; a forced kernel without the form fails.
extern "C" int32_t ctx_conv3x3_phase_f16(const void *x, const void *wp, const void *bias, const void *rowbias, const void *residual, int32_t B,
                                         int32_t H, int32_t W, int32_t Cin, int32_t Cout, void *part, int32_t splitk, void *y, ctx_stream_t stream)
{
    CTX_REQUIRE(x && y, "conv3x3_phase: null pointer");
    CTX_REQUIRE(wp, "conv3x3_phase: no phase pack (ctx_pack_conv3_phase_f16 writes it)");
    CTX_REQUIRE(!rowbias && !residual, "conv3x3_phase: the phase form takes a bias only, no row bias or residual");
    CTX_REQUIRE(B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && Cin % 64 == 0 && Cout % 8 == 0,
                "conv3x3_phase: need Cin%%64==0, Cout%%8==0 (B=%d H=%d W=%d Cin=%d Cout=%d)", B, H, W, Cin, Cout);
    CTX_REQUIRE(splitk != 0 && splitk <= 32 && (splitk <= 1 || splitk <= 4 * Cin / 64), "conv3x3_phase: splitk %d (1 .. min(32, K / 64), or < 0 for the plan)", splitk);
    GemmArgs a = {};
    ctx_conv3_problem(a, B, H, W, Cin, Cout, 1, 1, 0, 0);
    ctx_conv3_phase(a, (const f16 *)wp);
    a.X = (const f16 *)x; a.bias = (const f16 *)bias; a.out = (f16 *)y;
    a.ldrb = Cout;
    a.tile = -1; a.use8 = -1;
    CTX_REQUIRE((int64_t)B * H * W * Cin < (1ll << 31) && (int64_t)4 * Cout * a.K < (1ll << 31) && (int64_t)a.M * Cout < (1ll << 31),
                "conv3x3_phase: tensor too large for 32-bit offsets");
    if (splitk < 0 && part) ctx_gemm_plan(a, true); else a.splitk = part && splitk > 1 ? splitk : 1;
    a.part = (float *)part;
    return ctx_gemm_dispatch(a, true, (hipStream_t)stream);
}

// The resnet's first convolution as the engine runs it in front of norm2 (diffusers ResnetBlock2D.forward: conv1, + time embedding,
// norm2; reference call site src/stable_diffusion_depth.py:422-423): a stride-1 conv3x3 with either
//   gn_part != null: a request for the partials of GroupNorm(groups) over its output (GemmArgs::gn_part); *slots = slots per sample
//                    that were written (ctx_groupnorm_apply_f16 takes them), 0 = the launched kernel declined; or
//   keep_slabs != 0: split-K without the reduce launch; y is not written (may be null) and ctx_groupnorm_slabs_f16 reads `part`
//                    (*slots, when given, = the split factor that ran).
// splitk / part as ctx_conv3x3_seg_f16.  Honours ctx_gemm_tune.
extern "C" int32_t ctx_conv3x3_gn_f16(const void *x, const void *w, const void *bias, const void *bias2, const void *rowbias, const void *residual,
                                      int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, void *part, int32_t splitk, int32_t keep_slabs,
                                      int32_t groups, void *gn_part, int32_t *slots, void *y, ctx_stream_t stream)
{
    CTX_REQUIRE(x && w && (y || keep_slabs), "conv3x3_gn: null pointer");
    CTX_REQUIRE(B > 0 && H > 0 && W > 0 && Cin % 64 == 0 && Cout % 8 == 0 && splitk != 0, "conv3x3_gn: need Cin%%64==0, Cout%%8==0 (Cin=%d Cout=%d)", Cin, Cout);
    CTX_REQUIRE(!gn_part || (slots && groups > 0 && Cout % groups == 0 && !keep_slabs), "conv3x3_gn: a partials request needs slots, groups dividing Cout, and no kept slabs");
    CTX_REQUIRE(!keep_slabs || (part && (splitk > 1 || splitk < 0)), "conv3x3_gn: kept slabs need split-K");
    GemmArgs a = {};
    a.Ho = H; a.Wo = W;
    a.X = (const f16 *)x; a.Wt = (const f16 *)w; a.bias = (const f16 *)bias; a.bias2 = (const f16 *)bias2; a.rowbias = (const f16 *)rowbias;
    a.residual = (const f16 *)residual; a.out = (f16 *)y;
    a.M = B * H * W; a.N = Cout; a.K = 9 * Cin; a.ldc = Cout; a.ldr = Cout; a.rows_per_batch = H * W; a.ldrb = Cout;
    a.H = H; a.W = W; a.Cin = Cin; a.stride = 1;
    a.tile = -1; a.use8 = -1;
    if (splitk < 0 && part) ctx_gemm_plan(a, true); else a.splitk = part ? splitk : 1;      // < 0: the engine's plan (kernel and split)
    a.part = (float *)part; a.keep_slabs = keep_slabs ? 1 : 0;
    if (gn_part) { a.gn_part = (float *)gn_part; a.gn_cg = Cout / groups; a.gn_hw = H * W; }
    CTX_REQUIRE((int64_t)a.M * Cin < (1ll << 31) && (int64_t)Cout * a.K < (1ll << 31), "conv3x3_gn: tensor too large for 32-bit offsets");
    const int rc = ctx_gemm_dispatch(a, true, (hipStream_t)stream);
    if (slots) *slots = rc != CTX_OK ? 0 : keep_slabs ? a.splitk : a.gn_part ? a.gn_ns : 0;
    return rc;
}

// ------------------------------------------------------------------------------------------------
// Small-M path (time embedding MLP, per-resnet temb projections; M = CFG batch = 2): weight-streaming
// GEMV, one wave per output feature, 16-byte loads along K, fp32 accumulate.
//   out[b,n] = act( sum_k x[b,k] * w[n,k] + bias[n] ),  x optionally SiLU'd on load.
// Two output features per wave and up to GV_U 16-byte chunks per lane per feature, all loaded before the first FMA: the
// time_emb_proj GEMV streams 52 MB of weights per UNet evaluation and is bound by the bytes it keeps in flight.
#define GV_U 4
__global__ __launch_bounds__(256) void k_gemv_f16(const f16 *__restrict__ x, const f16 *__restrict__ w,
                                                  const f16 *__restrict__ bias, int Bm, int N, int K, int silu_in,
                                                  int silu_out, f16 *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int n0 = ((blockIdx.x * 256 + threadIdx.x) >> 6) * 2;
    if (n0 >= N) return;
    const int n1 = n0 + 1 < N ? n0 + 1 : n0;
    float acc[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k0 = 0; k0 < K; k0 += 512 * GV_U) {
        f16x8 wv[2][GV_U];
#pragma unroll
        for (int u = 0; u < GV_U; ++u) {
            const int k = k0 + u * 512 + lane * 8;
            const int kc = k < K ? k : K - 8;                              // unconditional (clamped) loads, masked below
            wv[0][u] = *(const f16x8 *)(w + (size_t)n0 * K + kc);
            wv[1][u] = *(const f16x8 *)(w + (size_t)n1 * K + kc);
        }
#pragma unroll
        for (int u = 0; u < GV_U; ++u) {
            const int k = k0 + u * 512 + lane * 8;
            if (k >= K) { wv[0][u] = zero8; wv[1][u] = zero8; }
            const int kc = k < K ? k : K - 8;
            for (int b = 0; b < Bm; ++b) {
                f16x8 xv = *(const f16x8 *)(x + (size_t)b * K + kc);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float xf = (float)xv[j];
                    if (silu_in) xf = xf / (1.0f + __expf(-xf));
                    acc[0][b] += xf * (float)wv[0][u][j];
                    acc[1][b] += xf * (float)wv[1][u][j];
                }
            }
        }
    }
    for (int r = 0; r < 2; ++r) {
        const int n = n0 + r;
        for (int b = 0; b < Bm; ++b) {
            float v = wave_sum(acc[r][b]);
            if (lane == 0 && n < N) {
                if (bias) v += (float)bias[n];
                if (silu_out) v = v / (1.0f + __expf(-v));
                out[(size_t)b * N + n] = (f16)v;
            }
        }
    }
}

int ctx_gemv_core(const f16 *x, const f16 *w, const f16 *bias, int Bm, int N, int K, int silu_in, int silu_out, f16 *out,
                 hipStream_t s)
{
    if (!x || !w || !out || Bm < 1 || N < 1 || K % 8 != 0 || K < 8) {
        ctx_set_error("gemv: null pointer, or Bm=%d (>=1) N=%d (>=1) K=%d (%%8)", Bm, N, K);
        return CTX_E_ARG;
    }
    for (int b0 = 0; b0 < Bm; b0 += 4) {                       // four rows per pass over the weights
        const int nb = Bm - b0 < 4 ? Bm - b0 : 4;
        hipLaunchKernelGGL(k_gemv_f16, dim3(cdiv(N, 8)), dim3(256), 0, s, x + (size_t)b0 * K, w, bias, nb, N, K, silu_in, silu_out,
                           out + (size_t)b0 * N);
    }
    return CTX_OK;
}
// test seam (tests/engine_ops_rule.py): the GEMV alone, through the host function the UNet engine calls
extern "C" int32_t ctx_gemv_f16(const void *x, const void *w, const void *bias, int32_t Bm, int32_t N, int32_t K, int32_t silu_in, int32_t silu_out,
                                void *out, ctx_stream_t stream)
{
    const int rc = ctx_gemv_core((const f16 *)x, (const f16 *)w, (const f16 *)bias, Bm, N, K, silu_in, silu_out, (f16 *)out, (hipStream_t)stream);
    if (rc != CTX_OK) return rc;
    CTX_CHECK_LAUNCH("gemv");
    return CTX_OK;
}

// ------------------------------------------------------------------------------------------------
// Device-timed repeat launcher for tools/bench_gemm.py (the Python call overhead of ~10 us per launch hides the
// real duration of the small layers).  Returns the average milliseconds per launch, or a negative error code.
extern "C" float ctx_bench_gemm(const void *A, const void *Wt, const void *bias, const void *residual, int32_t M, int32_t N,
                                int32_t K, void *C, int32_t conv_B, int32_t conv_H, int32_t conv_W, int32_t conv_Cin,
                                int32_t conv_flags, int32_t epi, void *part, int32_t splitk, int32_t iters, ctx_stream_t stream)
{
    hipStream_t s = (hipStream_t)stream;
    GemmArgs a = {};
    a.X = (const f16 *)A; a.Wt = (const f16 *)Wt; a.bias = (const f16 *)bias; a.residual = (const f16 *)residual; a.out = (f16 *)C;
    bool conv = conv_B > 0;
    if (conv) {
        a.stride = (conv_flags & 1) ? 2 : 1; a.ups = (conv_flags & 2) ? 1 : 0;
        int Hv = conv_H << a.ups, Wv = conv_W << a.ups;
        a.H = conv_H; a.W = conv_W; a.Cin = conv_Cin; a.Ho = (Hv - 1) / a.stride + 1; a.Wo = (Wv - 1) / a.stride + 1;
        a.M = conv_B * a.Ho * a.Wo; a.N = N; a.K = 9 * conv_Cin; a.rows_per_batch = a.Ho * a.Wo;
        if (conv_flags & 4) ctx_conv3_phase(a, a.Wt);      // bit 2 (with bit 1): the phase form; Wt is then the phase pack (no residual)
    } else {
        a.M = M; a.N = N; a.K = K; a.rows_per_batch = 1;
    }
    a.epi = epi;
    a.ldc = epi == 1 ? a.N / 2 : a.N; a.ldr = a.N; a.ldrb = a.N;
    a.tile = -1; a.use8 = -1;
    if (splitk < 0) {                                       // what the UNet executor would choose
        if (part) { ctx_gemm_plan(a, conv); splitk = a.splitk; } else splitk = 1;
    }
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    for (int i = 0; i < iters + 2; ++i) {
        if (i == 2) (void)hipEventRecord(e0, s);
        GemmArgs b = a;
        b.splitk = splitk; b.part = (float *)part;
        int rc = ctx_gemm_dispatch(b, conv, s);
        if (rc) return (float)rc;
    }
    (void)hipEventRecord(e1, s);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return ms / iters;
}
