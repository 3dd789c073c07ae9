// 144x160x64 fp16 MFMA GEMM / implicit-GEMM 3x3 convolution (gfx950): the tile that divides the UNet evenly over 256 CUs.
//
//   out[M,N] = X[M,K] . Wt[N,K]^T  (+bias)(+rowbias)(+residual) | fp32 split-K partials
//
// Replaces the cuBLAS / cuDNN calls under diffusers' UNet2DConditionModel (reference call site
// src/stable_diffusion_depth.py:422-423).  Why this shape: at the reference's 768^2 image (latent 96^2, CFG batch 2) the four
// UNet levels have M = 18432 / 4608 / 1152 / 288 tokens and N = 320 k features.  18432 x 320 outputs are exactly 256 tiles of
// 144 x 160 (one per CU, nothing masked), and the deeper levels are 128 / 64 / 16 such tiles: split-K by 2 / 4 / 16 gives 256
// workgroups again.  The 128- and 256-wide tiles of gemm.hip / gemm8.hip leave 16-30 % of the CUs idle or of the tile masked
// on these shapes (N = 320 is 2.5 tiles of 128), and their time is set by the bytes a CU stages per K step.
//
// Structure: WM x WN waves over the tile's 9 x 10 blocks of 16 x 16: 3 x 2 (wave tile 48 tokens x 80 features, 15 accumulators
// of v_mfma_f32_16x16x32_f16) or 3 x 5 (48 x 32, 6 accumulators, 15 waves: 4 / 4 / 4 / 3 per SIMD); weights = A operand,
// activations = B operand, so a lane owns one token and 4 consecutive features per accumulator.  Operand tiles go global -> LDS
// by global_load_lds_dwordx4 in 1-KiB pieces (8 rows x 128 B; 18 activation + 20 weight pieces per 64-deep K stage, dealt
// round-robin to the waves: a wave has SL or SL - 1 of them and waits with its own immediate vmcnt count), ring of 3 stages,
// one raw s_barrier per stage.
// LDS image and fragment reads as gemm8.hip (16-byte chunk index XORed with (row>>1)&7 on the DMA source and on the read).
#include "gemm_common.h"
#include <type_traits>

#define G144_BM 144
#define G144_BN 160
#define G144_STAGE ((G144_BM + G144_BN) * 64)      // f16 per stage

// UPS 1: the convolution has the fused nearest x2 upsample over nine taps (generic per-tap address arithmetic); 0: a tap is one scalar
// offset from the lane's centre-tap pointer and a bit of a 9-bit in-bounds mask; 2: the upsample's phase form (GemmArgs::phase), which
// is the fast path again with 4 taps, the shifts of the tile's phase and a row remap in the epilogues
// BMB: token rows of the tile in 16-row blocks: 9 (144 x 160) or 18 (288 x 160: 103 instead of 76 FLOP per staged byte, for problems
// with >= ~512 such tiles, i.e. the lockstep batch; its 56 KB stages leave room for a ring of 2 only, so it runs the lockstep schedule)
// GNP: the GroupNorm partials request (GemmArgs::gn_part) is honoured in the LDS-staged epilogue; instantiated for the 15-wave forms
// only, and the kernels without it compile to what they were
template <int WM, int WN, bool CONV, int NS, int VAR, int UPS = 0, int BMB = 9, bool GNP = false>
__global__ __launch_bounds__(64 * WM * WN) void k_gemm144(GemmArgs a)
{
    constexpr int NW = WM * WN, MI = BMB / WM, NI = 10 / WN;        // waves; 16x16 blocks per wave along tokens / features
    constexpr int BM = 16 * BMB, NPX = BM / 8;                      // tile rows; activation pieces (8 rows x 128 B each)
    constexpr int NP = NPX + 20;                                    // DMA pieces per stage: activation + 20 weight
    constexpr int STAGE = (BM + G144_BN) * 64;                      // f16 per stage
    static_assert(NPX % 2 == 0, "the K segments' chunk swizzle takes a weight piece's parity from its slot");
    static_assert(BMB % WM == 0 && (BMB == 9 || (BMB == 18 && VAR == 0)), "288-row tiles: lockstep schedule only");
    constexpr int SL = (NP + NW - 1) / NW;                          // piece slots per wave (the last one empty on some waves)
    static_assert(9 % WM == 0 && 10 % WN == 0, "wave grid must divide 9 x 10 blocks");
    extern __shared__ __attribute__((aligned(16))) f16 smem[];     // [NS][144 X rows | 160 W rows][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform by construction: SGPR, scalar branches
    const int wm = wave / WN, wn = wave % WN;
    const int r16 = lane & 15, kg = lane >> 4;

    const GemmTile tl = gemm_tile(a, blockIdx.x, 64, BM, G144_BN);
    constexpr bool PH = UPS == 2;
    static_assert(!PH || (CONV && !GNP), "the phase form is a convolution without GroupNorm partials");
    const ConvPhase ph = PH ? conv_phase_tile(a, tl.tile_m, BM) : ConvPhase{0, 0, 0, tl.m0, a.M};
    const int slice = tl.slice, m0 = ph.m0, n0 = tl.n0, kbeg = tl.kbeg, nk = tl.nk;
    const int ldw = CONV ? (PH ? 4 : 9) * a.Cin : a.K;             // weight row stride
    const f16 *const Wt = PH ? a.Wt + (size_t)ph.ph * a.N * ldw : a.Wt;

    // ---- DMA state: piece p = wave + NW i of the stage image; p < 18 activation rows 8p.., else weight rows 8(p-18).. -----
    const int prow = lane >> 3, pc = lane & 7;
    constexpr bool FAST = CONV && UPS != 1;
    constexpr int NTAP = PH ? 4 : 9;
    const f16 *pp[SL], *xcen[SL];
    int pst[SL], xoff[SL], xoy[SL], xox[SL], xlc[SL], xval[SL];
    bool xok[SL];
    const f16 *const zp = ctx_zero_page;
    const bool full = wave + NW * (SL - 1) < NP;                    // this wave uses its last slot
#pragma unroll
    for (int i = 0; i < SL; ++i) {
        const int p = wave + NW * i;
        const bool isx = p < NPX, live = p < NP;
        const int s = isx ? 8 * p + prow : 8 * (p - NPX) + prow;     // row inside the activation / weight tile
        xlc[i] = (pc ^ ((s >> 1) & 7)) * 8;
        xoff[i] = 0; xoy[i] = 0; xox[i] = 0;
        if (isx) {
            const int m = m0 + s;
            xok[i] = m < ph.M;
            if (CONV) {
                conv_pixel(a, xok[i] ? m : 0, xlc[i], xoy[i], xox[i], xoff[i]);
                pp[i] = zp; pst[i] = 0;
                if (FAST) {
                    xcen[i] = a.X + (size_t)xoff[i] + (size_t)(xoy[i] * a.W + xox[i]) * a.Cin;
                    int v = 0;
#pragma unroll
                    for (int t = 0; t < NTAP; ++t) {
                        const int iy = xoy[i] + (PH ? conv_phase_dy(ph, t) : t / 3 - 1 + a.poff), ix = xox[i] + (PH ? conv_phase_dx(ph, t) : t % 3 - 1 + a.poff);
                        if (xok[i] && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v |= 1 << t;
                    }
                    xval[i] = v;
                }
            } else {
                pp[i] = xok[i] ? a.X + (size_t)m * a.K + (size_t)kbeg * 64 + xlc[i] : ctx_zero_page;
                pst[i] = xok[i] ? 64 : 0;
            }
        } else {
            const bool ok = live && (n0 + s) < a.N;
            xok[i] = ok;
            pp[i] = ok ? Wt + (size_t)(n0 + s) * ldw + (size_t)kbeg * 64 + xlc[i] : ctx_zero_page;
            pst[i] = ok ? 64 : 0;
        }
    }

    int k_issue = kbeg * 64, issued = 0, tap_left = 0;
    // FAST: source (tap 0 .. 8, K segment 9 / 10), its channel count and the first channel of the next stage
    int cur_tap = 0, cur_c0 = 0, cur_C = a.Cin;
    if (CONV) { const ConvSrc cs = conv_stage_src(a, kbeg * 64); cur_tap = cs.src; cur_c0 = cs.c0; cur_C = cs.C; }
    auto retap = [&]() {                                            // CONV: new 3x3 tap -> recompute the activation pointers
        if (FAST) {
            // A K segment (cur_tap 9 / 10): its tensor has the output's pixel grid, so the lane's pixel is row m of it and the segment
            // is walked as a centre tap of that tensor; its weights are another matrix, so the weight pointers are formed anew.
            // (Nothing behind a segment reads the earlier sources again.)  One assignment to pp[] serves taps and segments: a second
            // definition of the pointers costs the kernel registers it does not have.  xcen[] itself is left as it is (a temporary per
            // slot takes the segment's pointer): overwriting it put the array in scratch memory with this compiler.  The 288-row form
            // now uses exactly 128 VGPRs, the limit of a 15-wave workgroup: it has no register left for the next change
            // (`make resources` prints every kernel's registers and scratch).
            const bool seg = cur_tap >= 9;
            const int sg = cur_tap - 9, tap = seg ? 4 : cur_tap;    // bit 4 of xval: the row exists
            if (seg) cur_C = sg ? a.segC[1] : a.segC[0];
            const int dy = PH ? conv_phase_dy(ph, tap) : tap / 3 - 1 + a.poff, dx = PH ? conv_phase_dx(ph, tap) : tap - (tap / 3) * 3 - 1 + a.poff;
            const int soff = seg ? cur_c0 : (dy * a.W + dx) * a.Cin + cur_c0;     // scalar: the same for every lane
            // the weight pointers walk on from where they stand, in place
            ConvWJump wj = {0, 0};
            if (seg) wj = conv_seg_wjump(a, sg, cur_c0, k_issue, sg == 0 || issued == 0);
#pragma unroll
            for (int i = 0; i < SL; ++i) {
                const int p = wave + NW * i;
                // lane's share of a segment offset: its row inside the 8-row piece times the row stride plus its swizzled chunk
                // (NPX is even: a weight piece's rows have p's parity)
                if (p >= NPX) {
                    if (seg) {
                        const int prow = conv_seg_lane(lane) >> 3;
                        const long step = wj.jump + ((long)(n0 + 8 * (p - NPX)) * wj.dld + prow * wj.dld) * (long)sizeof(f16);
                        pp[i] = (const f16 *)((const char *)pp[i] + (pst[i] ? step : 0));
                    }
                    continue;
                }
                const f16 *cen = xcen[i];
                if (seg) {
                    const int ln = conv_seg_lane(lane), prow = ln >> 3;
                    cen = conv_seg_x(a, sg, m0 + 8 * p, 0) + (unsigned)(prow * cur_C + (((ln & 7) ^ (prow >> 1) ^ ((p & 1) << 2)) << 3));
                }
                const bool v = (xval[i] >> tap) & 1;
                pp[i] = v ? cen + soff : zp;
                pst[i] = v ? 64 : 0;
            }
            tap_left = (cur_C - cur_c0) >> 6;
            return;
        }
        const ConvTap tap = conv_tap(a, k_issue);
#pragma unroll
        for (int i = 0; i < SL; ++i) {
            if (wave + NW * i >= NPX) continue;
            bool ok = xok[i];
            pp[i] = conv_tap_src(a, tap, xoy[i], xox[i], xoff[i], ok);
            pst[i] = ok ? 64 : 0;
        }
        tap_left = (a.Cin - tap.c0) / 64;
    };
    auto issue_begin = [&]() {
        if (CONV) {
            if (tap_left == 0) retap();
            --tap_left;
        }
    };
    auto issue_slot = [&](int buf, int i) {
        const int p = wave + NW * i;
        if (p < NP) {
            __builtin_amdgcn_global_load_lds((gptr_t)pp[i], (lptr_t)(smem + buf * STAGE + p * 512), 16, 0, 0);
            pp[i] += pst[i];
        }
    };
    auto issue_end = [&]() {
        k_issue += 64; ++issued;
        if (FAST) { cur_c0 += 64; if (cur_c0 == cur_C) { cur_c0 = 0; ++cur_tap; } }
    };
    auto issue = [&](int buf) {
        issue_begin();
#pragma unroll
        for (int i = 0; i < SL; ++i) issue_slot(buf, i);
        issue_end();
    };

    f32x4 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int swz = (r16 >> 1) & 7;
    const int ck[2] = {(kg ^ swz) * 8, ((4 + kg) ^ swz) * 8};
    const int xrow = (wm * 16 * MI + r16) * 64, wrow = BM * 64 + (wn * 16 * NI + r16) * 64;

#pragma unroll
    for (int p = 0; p < NS - 1; ++p)
        if (p < nk) issue(p);
    // wait until this wave's pieces of every stage but the `newer` most recent ones have landed
    auto wait_newer = [&](int newer) {
        if (newer >= 2) {
            if (full) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * SL) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (SL - 1)) : "memory");
        } else if (newer >= 1) {
            if (full) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(SL) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(SL - 1) : "memory");
        } else
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };
    int buf = 0;
    if constexpr (VAR == 0 && BMB == 18) {
        // lockstep with the stage's own work interleaved (the 288-row tile: ring of 2, so nothing of the NEXT stage can be touched
        // early): k 0..31 fragments first, then one DMA piece of the next stage behind each MFMA row instead of a burst of four at the
        // barrier (the vector-memory port queues them: the attention kernel's time stamps), and the k 32..63
        // fragments read under the first half's MFMAs.
        f16x8 xa[MI], wa[NI], wb[NI];                               // the k 32..63 token fragments reuse xa row by row (128 VGPRs at 15 waves)
        auto mrow = [&](const f16x8 &xf, const f16x8 (&wf)[NI], int i) {
#pragma unroll
            for (int j = 0; j < NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[j], xf, acc[i][j], 0, 0, 0);
        };
        static_assert(BMB != 18 || SL <= MI, "one DMA piece per MFMA row");
        for (int kt = 0; kt < nk; ++kt) {
            wait_newer(issued - 1 - kt);                            // this wave's pieces of stage kt
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            ctx_barrier();
            const bool go = issued < nk;
            const int pb = buf == 0 ? NS - 1 : buf - 1;
            const f16 *sb = smem + buf * STAGE;
#pragma unroll
            for (int i = 0; i < MI; ++i) xa[i] = *(const f16x8 *)(sb + xrow + i * 1024 + ck[0]);
#pragma unroll
            for (int j = 0; j < NI; ++j) wa[j] = *(const f16x8 *)(sb + wrow + j * 1024 + ck[0]);
            if (go) issue_begin();
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                mrow(xa[i], wa, i);
                __builtin_amdgcn_sched_barrier(0);
                xa[i] = *(const f16x8 *)(sb + xrow + i * 1024 + ck[1]);       // the row just consumed takes its second half
                if (i == 0) {
#pragma unroll
                    for (int j = 0; j < NI; ++j) wb[j] = *(const f16x8 *)(sb + wrow + j * 1024 + ck[1]);
                }
                if (go && i < SL) issue_slot(pb, i);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (go) issue_end();
#pragma unroll
            for (int i = 0; i < MI; ++i) mrow(xa[i], wb, i);
            buf = buf == NS - 1 ? 0 : buf + 1;
        }
    } else if constexpr (VAR == 0) {
        // lockstep schedule: one barrier per stage, every wave issues, reads and multiplies in the same order
        for (int kt = 0; kt < nk; ++kt) {
            wait_newer(issued - 1 - kt);                            // this wave's pieces of stage kt
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // the barrier does not wait for LDS reads in flight (stage kt-1's)
            ctx_barrier();                                          // everybody's pieces landed AND everybody finished stage kt-1
            if (issued < nk) issue(buf == 0 ? NS - 1 : buf - 1);   // into the buffer stage kt-1 used
            const f16 *sb = smem + buf * STAGE;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                f16x8 xf[MI], wf[NI];
#pragma unroll
                for (int i = 0; i < MI; ++i) xf[i] = *(const f16x8 *)(sb + xrow + i * 1024 + ck[ks]);
#pragma unroll
                for (int j = 0; j < NI; ++j) wf[j] = *(const f16x8 *)(sb + wrow + j * 1024 + ck[ks]);
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[j], xf[i], acc[i][j], 0, 0, 0);
            }
            buf = buf == NS - 1 ? 0 : buf + 1;
        }
    } else if constexpr (VAR == 2) {
        // One barrier per TWO stages (ring of 4 = two pairs of buffers): PMC on the forms above has the waves 42 % of their time at
        // s_waitcnt / s_barrier with 15 waves meeting every 64 K elements.  Iteration j: the pair's pieces have landed (vmcnt(0):
        // they were issued one whole iteration ago), barrier, the next pair's pieces go into the buffers pair j-1 just left, one
        // after each MFMA row, and the four k-32 quarters of the pair are multiplied with the next quarter's fragments read under
        // the current quarter's MFMAs.
        static_assert(VAR != 2 || NS == 4, "written for a ring of 4");
        f16x8 xa[MI], wa[NI], xb[MI], wb[NI];
        auto rd = [&](f16x8 (&xf)[MI], f16x8 (&wf)[NI], const f16 *sb, int ks) {
#pragma unroll
            for (int i = 0; i < MI; ++i) xf[i] = *(const f16x8 *)(sb + xrow + i * 1024 + ck[ks]);
#pragma unroll
            for (int j = 0; j < NI; ++j) wf[j] = *(const f16x8 *)(sb + wrow + j * 1024 + ck[ks]);
        };
        auto mrow = [&](const f16x8 &xf, const f16x8 (&wf)[NI], int i) {
#pragma unroll
            for (int j = 0; j < NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[j], xf, acc[i][j], 0, 0, 0);
        };
        static_assert(SL <= MI, "one DMA piece per MFMA row of a quarter");
        if (issued < nk) issue(issued & 3);                         // stage 3 (0 .. 2 went above): the prologue holds two whole pairs
        // `steady`: a whole pair with both of the next pair's stages still to issue: no wave-uniform branches in the body
        auto pair = [&](int k0, auto steady) {
            constexpr bool ST = decltype(steady)::value;
            const int b0 = k0 & 3;                                  // buffers of this pair: b0, b0 + 1
            const bool two = ST || k0 + 1 < nk;
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            ctx_barrier();                           // pair landed for everybody; the previous pair's buffers are free
            // quarter q of the pair: buffer b0 + (q >> 1), k half q & 1
            rd(xa, wa, smem + b0 * STAGE, 0);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (q >= 2 && !two) break;
                const bool even = (q & 1) == 0;
                if (q + 1 < (two ? 4 : 2)) {
                    const f16 *sn = smem + (b0 + ((q + 1) >> 1)) * STAGE;
                    if (even) rd(xb, wb, sn, (q + 1) & 1); else rd(xa, wa, sn, (q + 1) & 1);
                }
                // the next pair's two stages go into the buffers of the previous pair, one stage per even quarter
                const bool dma = even && (ST || (issued < nk && issued <= k0 + 3));
                if (dma) issue_begin();
#pragma unroll
                for (int i = 0; i < MI; ++i) {
                    if (even) mrow(xa[i], wa, i); else mrow(xb[i], wb, i);
                    __builtin_amdgcn_sched_barrier(0);
                    if (dma && i < SL) issue_slot(issued & 3, i);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (dma) issue_end();
            }
        };
        using T1 = std::integral_constant<bool, true>;
        using T0 = std::integral_constant<bool, false>;
        int k0 = 0;
        if (k0 < nk) { pair(k0, T0{}); k0 += 2; }                   // pair 0: the next pair was issued by the prologue
        for (; k0 + 3 < nk; k0 += 2) pair(k0, T1{});                // stages k0 + 2, k0 + 3 exist and are issued here
        for (; k0 < nk; k0 += 2) pair(k0, T0{});
    } else {
        // Software-pipelined schedule (ring of 4).  Measured on the lockstep schedule (each leg removed in turn): a 64-deep stage
        // costs ~1670 clk, of which DMA, fragment reads and MFMA each expose ~400 and ~390 are fixed: after the barrier every wave
        // first issues its DMA pieces, then waits for the fragment reads it has just issued, and only then multiplies.  Here the
        // first half of a stage's fragments (k 0..31) is read during the PREVIOUS stage's last MFMAs, so after the barrier the
        // MFMAs start at once, and the DMA pieces and the remaining reads ride between them:
        //   iteration kt:  vmcnt: own pieces of stage kt+1 landed;  lgkmcnt(0): half-fragments A of stage kt are in registers
        //                  s_barrier  -> everybody's pieces of kt+1 landed, everybody is done reading buffer kt-1
        //                  MFMA(A) x MI rows, one DMA piece of stage kt+3 (into buffer kt-1) after each row, read B (k 32..63)
        //                  MFMA(B), read A' (stage kt+1, k 0..31) under them
        // (Tried first on this tile and dropped, both neutral: two wave groups one barrier apart as in gemm8.hip; whole-stage
        // register double buffering, which spills at 128 VGPRs.)
        static_assert(VAR == 0 || NS == 4, "written for a ring of 4");
        wait_newer(issued - 1);                                     // stage 0 (stages 1, 2 may fly)
        ctx_barrier();
        f16x8 xp_[MI], wp_[NI], xq[MI], wq[NI], xb[MI], wb[NI];
        auto rd = [&](f16x8 (&xf)[MI], f16x8 (&wf)[NI], const f16 *sb, int ks) {
#pragma unroll
            for (int i = 0; i < MI; ++i) xf[i] = *(const f16x8 *)(sb + xrow + i * 1024 + ck[ks]);
#pragma unroll
            for (int j = 0; j < NI; ++j) wf[j] = *(const f16x8 *)(sb + wrow + j * 1024 + ck[ks]);
        };
        auto mrow = [&](const f16x8 &xf, const f16x8 (&wf)[NI], int i) {
#pragma unroll
            for (int j = 0; j < NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[j], xf, acc[i][j], 0, 0, 0);
        };
        rd(xp_, wp_, smem, 0);
        // cur = half-fragments A of this stage (loaded), nxt = where the next stage's go
        // `steady` (a std::integral_constant): the loop's middle, where a stage is still to be issued (go), a next stage exists
        // (more) and exactly one newer stage is in flight at the wait — none of the wave-uniform branches those conditions cost
        // in the general form (ten s_cbranch per stage in the ISA), only the wave's own piece count remains
        auto stage = [&](f16x8 (&xc)[MI], f16x8 (&wc)[NI], f16x8 (&xn)[MI], f16x8 (&wn_)[NI], int kt, auto steady) {
            constexpr bool ST = decltype(steady)::value;
            if (ST) {
                if (full) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(SL) : "memory");
                else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(SL - 1) : "memory");
            } else
                wait_newer(issued - 1 - (kt + 1));                  // own pieces of stage kt+1
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // A of this stage has arrived; nothing of stage kt-1 is pending
            ctx_barrier();
            const bool go = ST || issued < nk;
            const int pb = buf == 0 ? NS - 1 : buf - 1;             // buffer of stage kt-1: takes stage kt+3
            const int nb_ = buf == NS - 1 ? 0 : buf + 1;
            const f16 *sc = smem + buf * STAGE, *sn = smem + nb_ * STAGE;
            const bool more = ST || kt + 1 < nk;
            if (go) issue_begin();
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                mrow(xc[i], wc, i);
                __builtin_amdgcn_sched_barrier(0);
                if (i == 0) rd(xb, wb, sc, 1);
                if (go && i < SL) issue_slot(pb, i);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (go) {
#pragma unroll
                for (int i = MI; i < SL; ++i) issue_slot(pb, i);
                issue_end();
            }
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                mrow(xb[i], wb, i);
                if (i == 0) {
                    __builtin_amdgcn_sched_barrier(0);
                    if (more) rd(xn, wn_, sn, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            buf = nb_;
        };
        using T1 = std::integral_constant<bool, true>;
        using T0 = std::integral_constant<bool, false>;
        int kt = 0;
        // steady pairs: stages kt and kt+1 both issue a stage (kt + 4 < nk) ...
        for (; kt + 4 < nk; kt += 2) {
            stage(xp_, wp_, xq, wq, kt, T1{});
            stage(xq, wq, xp_, wp_, kt + 1, T1{});
        }
        // ... then the last (up to four) stages in the general form
        for (; kt + 1 < nk; kt += 2) {
            stage(xp_, wp_, xq, wq, kt, T0{});
            stage(xq, wq, xp_, wp_, kt + 1, T0{});
        }
        if (kt < nk) stage(xp_, wp_, xq, wq, kt, T0{});
    }

    // ---- epilogue: lane owns token m (column r16 of each 16x16 block), registers walk 4 consecutive features --------------
    const int mb = m0 + wm * 16 * MI, nb = n0 + wn * 16 * NI;
    if (a.splitk > 1) {
        float *pb = a.part + (size_t)slice * a.M * a.N;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int m = mb + 16 * i + r16;
            if (m >= ph.M) continue;
            const int mo = PH ? conv_phase_row(a, ph, m) : m;
#pragma unroll
            for (int j = 0; j < NI; ++j) store_part4(a, pb + (size_t)mo * a.N, nb + 16 * j + 4 * kg, acc[i][j]);
        }
        return;
    }
    if (a.stage_epi) {
        // Through LDS: the accumulator layout gives a lane one token and 4 features, i.e. 8-byte accesses in 32-byte runs over 16
        // rows per wave instruction, for the store AND for the residual read.  The tile is parked as fp32 [144][164] in the (now
        // idle) ring and walked back in whole rows: 16 bytes of fp16 per lane, 320-byte row segments, one rounding to fp16.
        constexpr int RS = G144_BN + 4;
        float *tile = (float *)smem;
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        ctx_barrier();                               // every wave is done with the ring
        constexpr int NT = 64 * NW, CPR = G144_BN / 8;              // chunks of 8 features per row
        // GNP: NT is a whole number of rows of chunks, so a thread keeps its 8-channel column over every pass of the walk below and
        // sums what it stores (the values as rounded to fp16: what k_gn_apply will read); nothing is masked (the launcher checks)
        static_assert(!GNP || (NT % CPR == 0 && NT % G144_BN == 0 && (NT / CPR) % (NT / G144_BN) == 0), "GroupNorm partials: whole chunk rows per pass");
        float gs[8], gq[8];
        if constexpr (GNP) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { gs[j] = 0.f; gq[j] = 0.f; }
        }
        // 144 rows at a time (the 288-row tile takes two passes through the same patch)
#pragma unroll
        for (int half = 0; half < BMB / 9; ++half) {
            if (half) __syncthreads();                              // the previous pass has been read out
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                const int blk = wm * MI + i;                        // 16-row block of the tile
                if (blk / 9 != half) continue;
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    *(f32x4 *)(tile + ((blk - 9 * half) * 16 + r16) * RS + wn * 16 * NI + 16 * j + 4 * kg) = acc[i][j];
            }
            __syncthreads();
            for (int ch = tid; ch < 144 * CPR; ch += NT) {
                const int row = ch / CPR, c8 = (ch - row * CPR) * 8;
                const int m = m0 + 144 * half + row, n = n0 + c8;
                if (m >= ph.M || n >= a.N) continue;
                const f32x4 v0 = *(const f32x4 *)(tile + row * RS + c8), v1 = *(const f32x4 *)(tile + row * RS + c8 + 4);
                float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                bias8(a, v, n);
                const f16x8 o = store8(a, v, PH ? conv_phase_row(a, ph, m) : m, n);
                if constexpr (GNP) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) { const float f = (float)o[j]; gs[j] += f; gq[j] += f * f; }
                }
            }
        }
        if constexpr (GNP) {
            // Fold to one (sum, sum of squares) per group of the tile, in a fixed order, through the patch's LDS (read out by now):
            // thread sums [PLN pixel lanes][8][CPR] (8-byte cells, consecutive lanes consecutive cells) -> A: channel sums over NA
            // slices of the pixel lanes [NA][160] -> B: 8 lanes walk a group's NA x cg cells, then a shuffle tree (as k_gn_stats).
            constexpr int PLN = NT / CPR, NA = NT / G144_BN, LPA = PLN / NA;
            float2 *sp = (float2 *)smem, *sc = sp + PLN * 8 * CPR;
            const int c8 = tid % CPR, pl = tid / CPR;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            ctx_barrier();                                          // everybody has read the patch out
#pragma unroll
            for (int j = 0; j < 8; ++j) sp[(pl * 8 + j) * CPR + c8] = make_float2(gs[j], gq[j]);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            ctx_barrier();
            {
                const int sl = tid / G144_BN, ci = tid - sl * G144_BN;      // cell ci = j * CPR + c8 of a pixel lane: channel c8 * 8 + j
                float ss = 0.f, qq = 0.f;
#pragma unroll
                for (int l = 0; l < LPA; ++l) { const float2 t = sp[(sl * LPA + l) * G144_BN + ci]; ss += t.x; qq += t.y; }
                sc[sl * G144_BN + (ci % CPR) * 8 + ci / CPR] = make_float2(ss, qq);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            ctx_barrier();
            const int cg = a.gn_cg, ng = G144_BN / cg, cells = NA * cg;
            const int oc = tid >> 3, l8 = tid & 7;                  // NT / 8 = 120 octets >= the tile's groups (cg >= 2)
            float ss = 0.f, qq = 0.f;
            if (oc < ng)
                for (int k = l8; k < cells; k += 8) {
                    const int sl = k / cg;
                    const float2 t = sc[sl * G144_BN + oc * cg + (k - sl * cg)];
                    ss += t.x; qq += t.y;
                }
#pragma unroll
            for (int o = 4; o > 0; o >>= 1) { ss += __shfl_xor(ss, o, 64); qq += __shfl_xor(qq, o, 64); }
            if (oc < ng && l8 == 0) {
                const int b = m0 / a.gn_hw, slot = (m0 - b * a.gn_hw) / BM;
                *(float2 *)(a.gn_part + (((size_t)b * a.gn_ns + slot) * (a.N / cg) + n0 / cg + oc) * 2) = make_float2(ss, qq);
            }
        }
        return;
    }
    f16x4 bs[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int nn = nb + 16 * j + 4 * kg;
        bs[j] = (a.bias && nn < a.N) ? *(const f16x4 *)(a.bias + nn) : (f16x4){0, 0, 0, 0};
    }
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        const int m = mb + 16 * i + r16;
        if (m >= ph.M) continue;
        const int bidx = a.rowbias ? m / a.rows_per_batch : 0;
        const int mo = PH ? conv_phase_row(a, ph, m) : m;
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int nn = nb + 16 * j + 4 * kg;
            if (nn >= a.N) continue;
            f32x4 v = add4(acc[i][j], bs[j]);
            if (a.bias2) v = add4(v, *(const f16x4 *)(a.bias2 + nn));
            store4(a, v, mo, bidx, nn);
        }
    }
}

// Launch when the problem fits (returns 1): K a multiple of 64 (conv: Cin too), plain epilogue, fp16 in and out.
// form 0: 6 waves (3 x 2, wave tile 48 x 80); 1: 15 waves (3 x 5, wave tile 48 x 32), lockstep; 2: 15 waves, ring of 4, software-pipelined
// (MFMAs first, DMA and reads between them); 3: 15 waves, one barrier per two stages; 4: 288 x 160 tile, 15 waves, lockstep, ring of 2.
int ctx_gemm144_try(GemmArgs &a, bool conv, int form, hipStream_t s)
{
    if (a.K % 64 != 0 || (conv && a.Cin % 64 != 0) || a.N % 4 != 0 || a.epi != 0 || a.res32 || a.out32 || a.zins) return 0;
    for (int i = 0; i < a.nseg; ++i)
        if (a.segC[i] % 64 != 0 || a.segLdw[i] % 64 != 0) return 0;  // K segments in whole stages, weight rows in whole swizzle periods
    if (a.ldc % 4 != 0 || (a.residual && a.ldr % 4 != 0) || (a.rowbias && a.ldrb % 4 != 0)) return 0;
    const int bm = form == 4 ? 288 : G144_BM;
    a.ntm = a.phase ? 4 * cdiv(a.M / 4, bm) : cdiv(a.M, bm);       // phase form: whole tiles per phase
    a.ntn = cdiv(a.N, G144_BN);
    int S = (a.splitk > 1 && a.part) ? a.splitk : 1;
    if (S > a.K / 64) S = a.K / 64;
    a.splitk = S;
    a.mfast = ctx_gemm_mfast(a, conv);
    static const int stg = ctx_env_int("CTX_G144_STAGE", 1);
    a.stage_epi = stg && form != 0 && a.N % 8 == 0 && a.ldc % 8 == 0 && (!a.residual || a.ldr % 8 == 0) && (!a.rowbias || a.ldrb % 8 == 0);
    const dim3 grid(a.ntm * a.ntn * S);
    // GroupNorm partials: a tile lies inside one sample and holds whole groups, nothing is masked, and the rows are walked through
    // LDS (the 15-wave forms).  With split-K the request is the reduce kernel's (gemm.hip); otherwise a request this tile cannot
    // serve is cleared: the caller sees the decline.
    bool gnp = false;
    if (a.gn_part && S == 1) {
        gnp = a.stage_epi && !(conv && a.ups) && a.gn_hw > 0 && a.gn_cg >= 2 && a.M % a.gn_hw == 0 && a.gn_hw % bm == 0 && a.gn_hw / bm <= CTX_GN_MAX_SLOTS &&
              a.N % G144_BN == 0 && G144_BN % a.gn_cg == 0 && a.ldc == a.N;
        if (gnp) a.gn_ns = a.gn_hw / bm; else a.gn_part = nullptr;
    }
    // threads, ring depth, then the kernel's template arguments
#define G144_GO(NT_, NS_, ...) ctx_launch<k_gemm144<__VA_ARGS__>>(0, grid, dim3(NT_), (size_t)NS_ * (bm + G144_BN) * 64 * sizeof(f16), s, a)
    const int ups = !conv ? 0 : a.phase ? 2 : a.ups ? 1 : 0;        // the kernels' UPS
    if (gnp) {                                                       // the same forms with the partials in the epilogue
        switch (form) {
        case 4: if (conv) G144_GO(960, 2, 3, 5, true, 2, 0, 0, 18, true); else G144_GO(960, 2, 3, 5, false, 2, 0, 0, 18, true); break;
        case 1: if (conv) G144_GO(960, 3, 3, 5, true, 3, 0, 0, 9, true); else G144_GO(960, 3, 3, 5, false, 3, 0, 0, 9, true); break;
        case 2: if (conv) G144_GO(960, 4, 3, 5, true, 4, 1, 0, 9, true); else G144_GO(960, 4, 3, 5, false, 4, 1, 0, 9, true); break;
        default: if (conv) G144_GO(960, 4, 3, 5, true, 4, 2, 0, 9, true); else G144_GO(960, 4, 3, 5, false, 4, 2, 0, 9, true); break;
        }
        return 1;
    }
    switch (form) {
    case 4:                                                          // 288 x 160, 15 waves, lockstep, ring of 2
        if (!conv) G144_GO(960, 2, 3, 5, false, 2, 0, 0, 18);
        else if (ups == 2) G144_GO(960, 2, 3, 5, true, 2, 0, 2, 18);
        else if (ups) G144_GO(960, 2, 3, 5, true, 2, 0, 1, 18); else G144_GO(960, 2, 3, 5, true, 2, 0, 0, 18);
        break;
    case 1:
        if (!conv) G144_GO(960, 3, 3, 5, false, 3, 0);
        else if (ups == 2) G144_GO(960, 3, 3, 5, true, 3, 0, 2);
        else if (ups) G144_GO(960, 3, 3, 5, true, 3, 0, 1); else G144_GO(960, 3, 3, 5, true, 3, 0);
        break;
    case 2:
        if (!conv) G144_GO(960, 4, 3, 5, false, 4, 1);
        else if (ups == 2) G144_GO(960, 4, 3, 5, true, 4, 1, 2);
        else if (ups) G144_GO(960, 4, 3, 5, true, 4, 1, 1); else G144_GO(960, 4, 3, 5, true, 4, 1);
        break;
    case 3:
        if (!conv) G144_GO(960, 4, 3, 5, false, 4, 2);
        else if (ups == 2) G144_GO(960, 4, 3, 5, true, 4, 2, 2);
        else if (ups) G144_GO(960, 4, 3, 5, true, 4, 2, 1); else G144_GO(960, 4, 3, 5, true, 4, 2);
        break;
    default:
        if (!conv) G144_GO(384, 3, 3, 2, false, 3, 0);
        else if (ups == 2) G144_GO(384, 3, 3, 2, true, 3, 0, 2);
        else if (ups) G144_GO(384, 3, 3, 2, true, 3, 0, 1); else G144_GO(384, 3, 3, 2, true, 3, 0);
        break;
    }
#undef G144_GO
    return 1;
}
