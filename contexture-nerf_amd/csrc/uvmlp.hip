// Fused texture field:  uv -> Fourier embed -> NeRF2D MLP -> raw rgb (-> (tanh+1)/2 atlas).
// Replaces get_embedder + NeRF2D.forward (src/run_nerf_helpers.py:15-135) as called from
// TexturedMeshModel.get_texture_map (src/models/textured_mesh.py:266-301).
//
// The reference computes this in fp32.  Two matrix pipes carry the contraction at that accuracy:
//   * the reference's own 2-D texture field (W = 256, 48-wide embedding) runs by default on the 16-bit pipe with SPLIT
//     operands (k_uvmlp_fwd16 / k_uvmlp_dgrad16: every operand is two fp16 numbers, 22 bits of mantissa);
//   * every other shape, the weight gradients, and everything under CTX_UVMLP_EXACT_F32=1 run on the exact-f32 pipe
//     (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain, 157 TFLOP/s peak on MI355X).
// ctx_uvmlp_fwd_emb / ctx_uvmlp_bwd_emb take a precomputed embedding of any width up to 64 (the hash-grid field) through the same
// exact-f32 kernels and add the gradient to that embedding (k_uvmlp_grad_emb, after the dZ chain).
//
// In all four chain kernels one workgroup = 64 texels x W hidden units; wave w owns hidden columns [64w, 64w+64) as 2x2
// accumulator tiles of 32x32.  Activations never leave the CU: the f32 kernels keep them in LDS as act[64][STRIDE] floats
// with the (zero-padded to 48) embedding in columns [0,48) and the hidden vector in [48,48+W); the skip layer simply reads
// columns [0,48+W).  The split kernels keep the same columns as two fp16 planes.  Weights are pre-packed so a lane's
// k-steps of one k-block are one 16-byte global load (L2-resident: 1.9 MB).
//
// Shared device pieces, each written once below and used by the kernels named:
//   uvm_split / uvm_join          hi / lo operands            pack16 kernels, fwd16, dgrad16
//   uvm_acc_row / uvm_relu_bit    accumulator element -> (row, ReLU bit)   all chain kernels, wgrad's slab store
//   uvm_stage_planes              a wave's packed outputs -> hi / lo planes   fwd16, dgrad16
//   uvm_kloop_f32                 f32-pipe K-loop             fwd (all three uses), dgrad
//   uvm_kloop_split               split-fp16 K-loop           fwd16, dgrad16
//   uvm_point / uvm_embed_col     Fourier embedding           fwd, fwd16
//   UvmList / uvm_node            texel list: compact row -> atlas node   uvm_point, uvm_store_out, uvm_draw_tile, k_uvm_absmax
//   uvm_store_out                 raw / tex store             fwd, fwd16
//   UvmOutGrad + uvm_draw_tile / uvm_bwd_out_layer / uvm_fold_out_grad   draw tile, backward output layer, gwo / gbo fold   dgrad, dgrad16
//   uvm_frag / uvm_src_k          fragment decode of the packed weights   the four pack kernels
#include "common.h"
#include <math.h>
#include <stdlib.h>
#include <type_traits>

#define UVM_MAX_LAYERS 16
#define UVM_EPAD 48       // padded embedding width of the 2-D field (42 -> 48)
#define UVM_EPAD3 64      // ... of the 3-D field (63 -> 64); the plan carries the one in use
#define UVM_TM 64         // texels per workgroup
#define UVM16_TM 64       // ... of the split-fp16 kernels
// The saved ReLU masks are [layer][64-texel tile][thread] u64 and are indexed by blockIdx / tile in every chain kernel, f32 or split.
static_assert(UVM16_TM == UVM_TM, "forward and backward, f32 and split, index the saved ReLU masks by the same 64-texel tile");

// Weight fragments of the NEXT k-block are fetched while the current one feeds the matrix pipe.  hipcc re-materialises a plain
// C++ prefetch (it proves the carried value equals a load of this iteration's address and re-loads it at the loop top), so the
// prefetched block index is laundered through an empty asm: the value then has to be carried in registers.  The K loops
// are unrolled by two over two register sets so that carrying costs no copies.
__device__ __forceinline__ int uvm_opaque(int k)
{
    asm volatile("" : "+s"(k));
    return k;
}

// ---- split operands: x = hi + lo * 2^-11 with hi = rn16(x), lo = rn16((x - hi) * 2^11): 22 bits of mantissa in two fp16 numbers ----
#define UVM_LO_SCALE 2048.0f            // 2^11
#define UVM_LO_INV (1.0f / 2048.0f)
__device__ __forceinline__ void uvm_split(float v, f16 &hi, f16 &lo)
{
    const f16 a = (f16)v;
    hi = a;
    lo = (f16)((v - (float)a) * UVM_LO_SCALE);
}
__device__ __forceinline__ float uvm_join(f16 hi, f16 lo) { return (float)hi + (float)lo * UVM_LO_INV; }
__device__ __forceinline__ void uvm_split4(const float (&v)[4], f16x4 &hi, f16x4 &lo)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) { f16 a, b; uvm_split(v[j], a, b); hi[j] = a; lo[j] = b; }
}
__device__ __forceinline__ float4 uvm_join4(const f16 *hi, const f16 *lo)   // four consecutive (8-byte aligned) elements of both planes
{
    const f16x4 vh = *(const f16x4 *)hi, vl = *(const f16x4 *)lo;
    return make_float4(uvm_join(vh[0], vl[0]), uvm_join(vh[1], vl[1]), uvm_join(vh[2], vl[2]), uvm_join(vh[3], vl[3]));
}
__device__ __forceinline__ uint32_t uvm_split_packed(float v)               // hi | lo << 16: one register until the planes may be written
{
    f16 hi, lo;
    uvm_split(v, hi, lo);
    return (uint32_t)__builtin_bit_cast(unsigned short, hi) | ((uint32_t)__builtin_bit_cast(unsigned short, lo) << 16);
}

// ---- accumulator layout of the 32x32 MFMAs: element q of lane (r, h) of the tile whose first row is row0 (32 mb within a wave's 2 x 2
// tiles (mb, nb)) sits at column nb*32 + r and this row ----
__device__ __forceinline__ int uvm_acc_row(int row0, int q, int h) { return row0 + (q & 3) + 8 * (q >> 2) + 4 * h; }
// ... and its ReLU pattern is this bit of the lane's u64 (what the forward saves is what the backward chain's tiles read)
__device__ __forceinline__ int uvm_relu_bit(int nb, int mb, int q) { return (nb * 2 + mb) * 16 + q; }

// a wave's outputs outv[nb][mb][q] (hi | lo << 16) to columns COL0 + [64 wave, 64 wave + 64) of the two planes; STRIDE in halves
template <int STRIDE, int COL0>
__device__ __forceinline__ void uvm_stage_planes(f16 *phi, f16 *plo, const uint32_t (&outv)[2][2][16], int wave, int r, int h)
{
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const int col = wave * 64 + nb * 32 + r;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int o = uvm_acc_row(mb * 32, q, h) * STRIDE + COL0 + col;
                ((unsigned short *)phi)[o] = (unsigned short)(outv[nb][mb][q] & 0xffffu);
                ((unsigned short *)plo)[o] = (unsigned short)(outv[nb][mb][q] >> 16);
            }
    }
}

__device__ __forceinline__ void uvm_zero(f32x16 &a)
{
#pragma unroll
    for (int q = 0; q < 16; ++q) a[q] = 0.f;
}

// ---- K-loop of the f32 pipe: acc[mb][nb] += A[rows 32 mb ..][k] . B[k][cols 32 nb ..] over k-blocks [kb0, kb1) (an even count) ----
// wp: the lane's float4 of the layer's k-block 0, column block 2 wave (KBS float4 per k-block, the second column block 64 further);
// arow0 / arow1: the lane's LDS rows r and r + 32 at the column of k-block 0 (+ 4h), so k-block kb is read at + 8 kb.
template <int W>
__device__ __forceinline__ void uvm_kloop_f32(f32x16 (&acc)[2][2], const float4 *wp, const float *arow0, const float *arow1, int kb0, int kb1)
{
    constexpr size_t KBS = (size_t)(W / 32) * 64;   // float4 per k-block
    auto kstep = [&](int kb, const float4 &b0, const float4 &b1) {
        float4 a0 = *(const float4 *)(arow0 + kb * 8);
        float4 a1 = *(const float4 *)(arow1 + kb * 8);
        const float av0[4] = {a0.x, a0.y, a0.z, a0.w}, av1[4] = {a1.x, a1.y, a1.z, a1.w};
        const float bv0[4] = {b0.x, b0.y, b0.z, b0.w}, bv1[4] = {b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0[j], bv0[j], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0[j], bv1[j], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1[j], bv0[j], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1[j], bv1[j], acc[1][1], 0, 0, 0);
        }
    };
    const float4 *p0 = wp + (size_t)kb0 * KBS;
    float4 wa0 = p0[0], wa1 = p0[64], wb0, wb1;
    for (int kb = kb0; kb < kb1; kb += 2) {          // every k-block range here has an even length
        const float4 *pb = wp + (size_t)uvm_opaque(kb + 1) * KBS;
        wb0 = pb[0]; wb1 = pb[64];
        __builtin_amdgcn_sched_barrier(0);           // keep the prefetch above the MFMAs it hides under
        kstep(kb, wa0, wa1);
        const float4 *pa = wp + (size_t)uvm_opaque(kb + 2 < kb1 ? kb + 2 : kb) * KBS;
        wa0 = pa[0]; wa1 = pa[64];
        __builtin_amdgcn_sched_barrier(0);
        kstep(kb + 1, wb0, wb1);
    }
}

// ---- K-loop of the split pipe: one 32-column block of the wave against its two 32-row blocks, nkb 16-deep k-steps ----
// A product a.w = ah.wh + 2^-11 (ah.wl + al.wh) + 2^-22 al.wl: the first three terms are three v_mfma_f32_32x32x16_f16 passes into TWO
// fp32 accumulator sets (acc: main, acx: cross, to be joined as acc + acx * 2^-11), the last (relative 2^-22) is dropped.
// wbase: the lane's 8 halves of weight block (k-step 0, this column block): block (kb, nbg) at ((kb * 8 + nbg) * 1024) halves, hi[64][8]
// then lo[64][8].  ah_base / al_base: the lane's row r at the column of k-step 0 (+ 8h) in the hi / lo plane; STRIDE in halves.
template <int STRIDE>
__device__ __forceinline__ void uvm_kloop_split(f32x16 (&acc_io)[2], f32x16 (&acx_io)[2], const f16 *wbase, const f16 *ah_base, const f16 *al_base, int nkb)
{
    // The loop runs on local copies declared before the operand sets and hands them back at the end.  Inlined, that is no code at all,
    // but it is the order the register allocator then sees them in: with the caller's arrays used directly, k_uvmlp_fwd16 comes out with
    // 20 bytes/lane of scratch and 64 accumulator copies behind its odd tail; this way it has neither.
    f32x16 acc[2] = {acc_io[0], acc_io[1]}, acx[2] = {acx_io[0], acx_io[1]};
    f16x8 b0h, b0l, b1h, b1l, b2h, b2l;    // k-steps kb, kb+1, kb+2: two steps of prefetch (one wave per SIMD hides nothing)
    auto load_b = [&](int kb, f16x8 &xh, f16x8 &xl) {
        const f16 *p = wbase + (size_t)uvm_opaque(kb < nkb ? kb : nkb - 1) * 8 * 1024;
        xh = *(const f16x8 *)(p); xl = *(const f16x8 *)(p + 512);
    };
    load_b(0, b0h, b0l); load_b(1, b1h, b1l);
    f16x8 ah[2], al[2], nah[2], nal[2];
    auto load_a = [&](int kb, f16x8 (&xh)[2], f16x8 (&xl)[2]) {
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            xh[mb] = *(const f16x8 *)(ah_base + mb * 32 * STRIDE + kb * 16);
            xl[mb] = *(const f16x8 *)(al_base + mb * 32 * STRIDE + kb * 16);
        }
    };
    load_a(0, ah, al);
    // One k-step: the next step's activation fragments (LDS) and the weights two steps ahead (L2) are requested before this
    // step's MFMAs issue — with one wave per SIMD nothing else covers their latency.  The loop walks two steps per trip over
    // the two activation register sets (no copies); only the three small weight sets rotate.
    auto step = [&](int kb, f16x8 (&ch)[2], f16x8 (&cl)[2], f16x8 (&nh)[2], f16x8 (&nl)[2]) {
        load_b(kb + 2, b2h, b2l);
        load_a(kb + 1 < nkb ? kb + 1 : kb, nh, nl);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            acc[mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch[mb], b0h, acc[mb], 0, 0, 0);
            acx[mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch[mb], b0l, acx[mb], 0, 0, 0);
            acx[mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cl[mb], b0h, acx[mb], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        b0h = b1h; b0l = b1l; b1h = b2h; b1l = b2l;
    };
    int kb = 0;
    for (; kb + 2 <= nkb; kb += 2) {
        step(kb, ah, al, nah, nal);
        step(kb + 1, nah, nal, ah, al);
    }
    if (kb < nkb) step(kb, ah, al, nah, nal);       // K = 48 and 304 are an odd number of 16-deep steps; a constant even nkb has no tail
    acc_io[0] = acc[0]; acc_io[1] = acc[1]; acx_io[0] = acx[0]; acx_io[1] = acx[1];
}

struct UvmLayer {
    int col0;       // first LDS column read
    int kp;         // padded K (multiple of 8)
    int64_t w_off;  // float offset of packed weights
    int64_t b_off;  // float offset of bias
};
struct UvmPlan {
    int n_hidden;            // D
    int W;
    int in_ch;               // dims*(1+2L)
    int epad;                // in_ch padded: 48 or 64
    int dims;                // input dimensionality (2: uv, 3: xyz); set by the forward entry
    int out_ch;
    int64_t out_w_off, out_b_off;
    UvmLayer layer[UVM_MAX_LAYERS];
    int64_t wt_off[UVM_MAX_LAYERS];   // layer i >= 1: W_i[:, hidden part]^T packed as an MFMA B operand (backward chain)
    int64_t w16_off[UVM_MAX_LAYERS];  // layer i: the same weights as two fp16 planes (hi, lo x 2^11) in 32x32x16 B-fragment order, or -1
    int64_t wt16_off[UVM_MAX_LAYERS]; // layer i >= 1: wt_off's operand as two fp16 planes (backward chain of k_uvmlp_dgrad16), or -1
};

// the shapes every entry point accepts: the widths are the ones uvm_dispatch has kernels for (one wave per 64 hidden columns as 1, 2 or
// 4 waves; there is no 3-wave form, so W = 192 is refused like any other width)
static inline bool uvm_envelope(int D, int W, int input_ch = 1 /* where the answer does not depend on it */)
{
    return D >= 1 && D <= UVM_MAX_LAYERS && (W == 64 || W == 128 || W == 256) && input_ch >= 1 && input_ch <= UVM_EPAD3;
}
static inline int uvm_epad(int input_ch) { return input_ch <= UVM_EPAD ? UVM_EPAD : UVM_EPAD3; }

static int uvm_build_plan(int D, int W, int input_ch, int output_ch, int skip, UvmPlan &p, int64_t &total)
{
    if (!uvm_envelope(D, W, input_ch) || output_ch < 1 || output_ch > 4) return -1;
    const int EP = uvm_epad(input_ch);
    p.n_hidden = D; p.W = W; p.in_ch = input_ch; p.out_ch = output_ch; p.epad = EP; p.dims = 2;
    int64_t off = 0;
    for (int i = 0; i < D; ++i) {
        UvmLayer &l = p.layer[i];
        if (i == 0) { l.col0 = 0; l.kp = EP; }
        else if (i == skip + 1) { l.col0 = 0; l.kp = EP + W; }
        else { l.col0 = EP; l.kp = W; }
        l.w_off = off; off += (int64_t)l.kp * W;
        l.b_off = off; off += W;
    }
    p.out_w_off = off; off += (int64_t)output_ch * W;
    p.out_b_off = off; off += 4;
    p.wt_off[0] = -1;
    for (int i = 1; i < D; ++i) { p.wt_off[i] = off; off += (int64_t)W * W; }
    // split-fp16 copies for the fast forward (k_uvmlp_fwd16): kp x W elements x (2 + 2) bytes = kp x W floats of space
    for (int i = 0; i < D; ++i) {
        if (W == 256 && EP == UVM_EPAD && p.layer[i].kp % 16 == 0) { p.w16_off[i] = off; off += (int64_t)p.layer[i].kp * W; }
        else p.w16_off[i] = -1;
    }
    for (int i = 0; i < D; ++i) {
        if (i >= 1 && W == 256 && EP == UVM_EPAD) { p.wt16_off[i] = off; off += (int64_t)W * W; }
        else p.wt16_off[i] = -1;
    }
    total = off;
    return 0;
}

// The split-fp16 kernels serve the reference's texture field (2-D, W = 256, 48-wide embedding) unless the exact-f32 pipe is asked for.
// The environment is read on every call: the switch may be flipped inside one process.
static bool uvm_use_split16(const UvmPlan &p, int dims, bool backward)
{
    const char *ex = getenv("CTX_UVMLP_EXACT_F32");
    bool fast = dims == 2 && p.W == 256 && p.epad == UVM_EPAD && !(ex && ex[0] == '1');
    for (int i = backward ? 1 : 0; i < p.n_hidden && fast; ++i) fast = (backward ? p.wt16_off[i] : p.w16_off[i]) >= 0;
    return fast;
}

// (W, EP) of a plan as compile-time constants: f(integral_constant<W>, integral_constant<EP>)
template <int V> using uvm_c = std::integral_constant<int, V>;
// The widths are uvm_envelope's, one branch each.  Any other width is unreachable here (every caller has built its plan, and
// uvm_build_plan starts with uvm_envelope); should the gate ever be widened without a kernel, nothing is launched and the caller
// reports the false return as an error instead of running another width's kernel on the blob.
template <class F> static bool uvm_dispatch(int W, int EP, F f)
{
    auto with_w = [&](auto w) { if (EP == UVM_EPAD) f(w, uvm_c<UVM_EPAD>{}); else f(w, uvm_c<UVM_EPAD3>{}); };
    if (W == 256) with_w(uvm_c<256>{});
    else if (W == 128) with_w(uvm_c<128>{});
    else if (W == 64) with_w(uvm_c<64>{});
    else return false;
    return true;
}
#define UVM_DISPATCHED(ok, who) CTX_REQUIRE(ok, "%s: no kernel for W=%d (unreachable behind uvm_envelope)", who, W)

extern "C" int64_t ctx_uvmlp_packed_bytes(int32_t D, int32_t W, int32_t input_ch, int32_t output_ch, int32_t skip)
{
    UvmPlan p; int64_t total = 0;
    if (uvm_build_plan(D, W, input_ch, output_ch, skip, p, total)) return -1;
    return total * 4;
}

// ---- packed weights: B fragments of the 32x32 MFMAs, J values per lane and k-block (4: x2_f32 in four steps, 8: x16_f16) ----
// Element idx of a packed layer = (block (kb, nb), lane (r, h), j): position k = kb*2J + J*h + j along the contraction, n = nb*32 + r across.
struct UvmFrag { int64_t blk; int lane, j, k, n; };
template <int J>
__device__ __forceinline__ UvmFrag uvm_frag(int64_t idx, int W)
{
    UvmFrag f;
    f.j = idx & (J - 1);
    f.lane = ((uint64_t)idx / J) & 63;
    f.blk = (uint64_t)idx / (64 * J);
    const int nb = f.blk % (W / 32), kb = f.blk / (W / 32);
    f.k = kb * 2 * J + J * (f.lane >> 5) + f.j;
    f.n = nb * 32 + (f.lane & 31);
    return f;
}
// padded LDS column k -> column of the nn.Linear weight (or -1: zero).  mode 0: first layer (embedding, padded to epad);
// 1: skip layer (padded embedding, then the hidden vector); 2: plain hidden layer
__device__ __forceinline__ int uvm_src_k(int mode, int k, int in_ch, int epad)
{
    if (mode == 2) return k;
    if (mode == 0) return k < in_ch ? k : -1;
    return k < in_ch ? k : (k < epad ? -1 : k - epad + in_ch);
}
__device__ __forceinline__ float uvm_src_w(const float *w, int kin, int n, int src_k) { return (src_k >= 0 && src_k < kin) ? w[(int64_t)n * kin + src_k] : 0.0f; }
// a split element to block f.blk = hi[64 lanes][8] then lo[64 lanes][8]: one 16-byte load per lane and plane
__device__ __forceinline__ void uvm_put16(f16 *dw, const UvmFrag &f, float v)
{
    f16 hi, lo;
    uvm_split(v, hi, lo);
    dw[f.blk * 1024 + f.lane * 8 + f.j] = hi;
    dw[f.blk * 1024 + 512 + f.lane * 8 + f.j] = lo;
}

// src: nn.Linear weight [W][kin]; dst packed [(kb*(W/32)+nb)*64+lane][4] with
// lane=(r,h): value j = weight[nb*32+r][map(kb*8+4h+j)].
__global__ void k_uvm_pack(const float *__restrict__ w, const float *__restrict__ b, int W, int kin, int kp,
                           int in_ch, int epad, int mode, float *__restrict__ dw, float *__restrict__ db)
{
    int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < (int64_t)kp * W) {
        const UvmFrag f = uvm_frag<4>(idx, W);
        dw[idx] = uvm_src_w(w, kin, f.n, uvm_src_k(mode, f.k, in_ch, epad));
    }
    if (idx < W) db[idx] = b[idx];
}

// Backward-chain operand: dA_{i-1}[t][k] = sum_n dZ_i[t][n] * w[n][off + k]  ->  B[n][k]; packed like k_uvm_pack with the
// contraction index n in the place of k:  dst[(kb*(W/32)+nb)*64+lane][j] = w[kb*8+4h+j][off + nb*32 + r].
__global__ void k_uvm_pack_t(const float *__restrict__ w, int W, int kin, int off, float *__restrict__ dw)
{
    int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)W * W) return;
    const UvmFrag f = uvm_frag<4>(idx, W);
    dw[idx] = w[(int64_t)f.k * kin + off + f.n];
}

// fp16 split of the layer weights for k_uvmlp_fwd16: lane (r, h) element j = w[nb*32 + r][map(kb*16 + 8h + j)]
// — the B fragment of v_mfma_f32_32x32x16_f16.
__global__ void k_uvm_pack16(const float *__restrict__ w, int W, int kin, int kp, int in_ch, int epad, int mode, f16 *__restrict__ dw)
{
    int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)kp * W) return;
    const UvmFrag f = uvm_frag<8>(idx, W);
    uvm_put16(dw, f, uvm_src_w(w, kin, f.n, uvm_src_k(mode, f.k, in_ch, epad)));
}

// backward-chain operand of k_uvmlp_dgrad16: block (kb over the contraction index n, nb over the output column k),
// lane (r, h) element j = w[kb*16 + 8h + j][off + nb*32 + r]
__global__ void k_uvm_pack16_t(const float *__restrict__ w, int W, int kin, int off, f16 *__restrict__ dw)
{
    int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)W * W) return;
    const UvmFrag f = uvm_frag<8>(idx, W);
    uvm_put16(dw, f, w[(int64_t)f.k * kin + off + f.n]);
}

__global__ void k_uvm_pack_out(const float *__restrict__ w, const float *__restrict__ b, int W, int out_ch,
                               float *__restrict__ dw, float *__restrict__ db)
{
    int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < out_ch * W) dw[idx] = w[idx];
    if (idx < 4) db[idx] = idx < out_ch ? b[idx] : 0.0f;
}

extern "C" int32_t ctx_uvmlp_pack(const float *const *ws, const float *const *bs, int32_t D, int32_t W,
                                  int32_t input_ch, int32_t output_ch, int32_t skip, void *packed, ctx_stream_t stream)
{
    UvmPlan p; int64_t total = 0;
    CTX_REQUIRE(ws && bs && packed, "uvmlp_pack: null pointer");
    CTX_REQUIRE(uvm_build_plan(D, W, input_ch, output_ch, skip, p, total) == 0,
                "uvmlp_pack: unsupported D=%d W=%d input_ch=%d output_ch=%d", D, W, input_ch, output_ch);
    float *dst = (float *)packed;
    hipStream_t s = (hipStream_t)stream;
    for (int i = 0; i < D; ++i) {
        int mode = i == 0 ? 0 : (i == skip + 1 ? 1 : 2);
        int kin = i == 0 ? input_ch : (i == skip + 1 ? input_ch + W : W);
        int64_t n = (int64_t)p.layer[i].kp * W;
        hipLaunchKernelGGL(k_uvm_pack, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, s, ws[i], bs[i], W, kin, p.layer[i].kp,
                           input_ch, p.epad, mode, dst + p.layer[i].w_off, dst + p.layer[i].b_off);
        if (i >= 1)
            hipLaunchKernelGGL(k_uvm_pack_t, dim3((unsigned)cdiv64((int64_t)W * W, 256)), dim3(256), 0, s, ws[i], W, kin,
                               i == skip + 1 ? input_ch : 0, dst + p.wt_off[i]);
        if (p.wt16_off[i] >= 0)
            hipLaunchKernelGGL(k_uvm_pack16_t, dim3((unsigned)cdiv64((int64_t)W * W, 256)), dim3(256), 0, s, ws[i], W, kin, i == skip + 1 ? input_ch : 0,
                               (f16 *)(dst + p.wt16_off[i]));
        if (p.w16_off[i] >= 0)
            hipLaunchKernelGGL(k_uvm_pack16, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, s, ws[i], W, kin, p.layer[i].kp, input_ch, p.epad, mode,
                               (f16 *)(dst + p.w16_off[i]));
    }
    hipLaunchKernelGGL(k_uvm_pack_out, dim3(cdiv(output_ch * W, 256)), dim3(256), 0, s, ws[D], bs[D], W, output_ch,
                       dst + p.out_w_off, dst + p.out_b_off);
    CTX_CHECK_LAUNCH("uvmlp_pack");
    return CTX_OK;
}

// ---- Fourier embedding: uvm_point yields a texel's coordinates, uvm_embed_col column e of its embedding ----
struct UvmPoint { float x0, x1, x2; };
// Texel list (get_texture_map_only_valid_areas, src/models/textured_mesh.py:303-347): row n of the launch is node idx[n] of the
// res x res grid.  raw, the saved activations and dZ stay compact ([N] rows); only the atlas planes ([out_ch][plane], plane = res^2)
// are addressed through the list.  idx == nullptr: row n is its own node and plane == N (every other point source).
struct UvmList { const int *idx; int64_t plane; };
// the atlas node of row n < N, or -1 for a list entry outside the grid (never stored to, never read from)
__device__ __forceinline__ int64_t uvm_node(const UvmList &list, int64_t n)
{
    if (!list.idx) return n;
    const int64_t t = list.idx[n];
    return (t >= 0 && t < list.plane) ? t : -1;
}
// row n of uv (d = 2) / xyz (d = 3), or node n (listed: node idx[n]) of the res x res atlas grid; zero past N and on the `emb` seam
__device__ __forceinline__ UvmPoint uvm_point(const float *__restrict__ uv, const float *__restrict__ emb, const UvmList &list, int64_t n, int64_t N,
                                              int res, int d)
{
    UvmPoint p = {0.f, 0.f, 0.f};
    if (n < N && !emb) {
        if (uv) { p.x0 = uv[n * d + 0]; p.x1 = uv[n * d + 1]; if (d > 2) p.x2 = uv[n * d + 2]; }
        else {
            // torch.linspace(0,1,res): start + i*step for the first half, end - (res-1-i)*step after
            if (list.idx) { n = uvm_node(list, n); if (n < 0) return p; }
            int i = (int)(n / res), j = (int)(n % res);
            float step = 1.0f / (float)(res - 1);
            p.x0 = (j < res / 2) ? (float)j * step : 1.0f - (float)(res - 1 - j) * step;
            p.x1 = (i < res / 2) ? (float)i * step : 1.0f - (float)(res - 1 - i) * step;
        }
    }
    return p;
}
// column e of [x, sin(2^l x) (d), cos(2^l x) (d) per frequency l < L], zero from in_ch on; `emb` given: that row of it instead
__device__ __forceinline__ float uvm_embed_col(const UvmPoint &p, const float *__restrict__ emb, int64_t n, int64_t N, int e, int d, int L, int in_ch)
{
    float val = 0.f;
    if (emb) val = (e < in_ch && n < N) ? emb[n * in_ch + e] : 0.f;
    else if (e < d) val = e == 0 ? p.x0 : (e == 1 ? p.x1 : p.x2);
    else if (e < d * (1 + 2 * L)) {
        int l = (e - d) / (2 * d), q = (e - d) % (2 * d);
        int c = q % d;
        float a = (c == 0 ? p.x0 : (c == 1 ? p.x1 : p.x2)) * (float)(1 << l);
        val = (q >= d) ? cosf(a) : sinf(a);
    }
    return val;
}

// the forward output layer's result s[c] (before the bias) of texel n < N: raw [N][out_ch] and, for the atlas, (tanh + 1) / 2 at the
// row's node of [out_ch][plane]
__device__ __forceinline__ void uvm_store_out(const float (&s)[4], const float *__restrict__ packed, const UvmPlan &plan, float *__restrict__ raw,
                                              float *__restrict__ tex, const UvmList &list, int64_t n)
{
    const int64_t node = uvm_node(list, n);
    for (int c = 0; c < plan.out_ch; ++c) {
        float v = s[c] + packed[plan.out_b_off + c];
        raw[n * plan.out_ch + c] = v;
        if (tex && node >= 0) tex[(int64_t)c * list.plane + node] = (tanhf(v) + 1.0f) / 2.0f;
    }
}

template <int W, int EP>
__global__ __launch_bounds__(W) void k_uvmlp_fwd(const float *__restrict__ uv, const float *__restrict__ emb, UvmList list, int64_t N, int res, int L,
                                                 const float *__restrict__ packed, UvmPlan plan,
                                                 float *__restrict__ raw, float *__restrict__ tex, float *__restrict__ saved)
{
    // 2-D field (EP = 48): embedding in columns [0,48), hidden vector in [48,48+W), 78.8 KB -> two workgroups per CU.
    // 3-D field (EP = 64): that layout would be 82.9 KB (one workgroup per CU), so the hidden vector overlays the embedding
    // ([0,W), 66.6 KB) and the skip layer re-creates the embedding in place after its hidden-part k-blocks.
    constexpr bool RC = EP > UVM_EPAD;
    constexpr int HOFF = RC ? 0 : EP;
    constexpr int STRIDE = HOFF + W + 4;   // 308 / 260 for W=256: 4 x odd -> conflict-free ds_read_b128 rows
    static_assert((STRIDE / 4) % 2 == 1, "row stride must be 4 x odd");
    static_assert(W >= EP || !RC, "the overlay needs W >= 64");
    extern __shared__ __attribute__((aligned(16))) float act[];   // [UVM_TM][STRIDE]
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int64_t n0 = (int64_t)blockIdx.x * UVM_TM;

    // ---- Fourier embedding into columns [0,EP): one texel per lane, the waves share the columns ----
    auto put_embedding = [&]() {
        int row = tid & 63;
        int64_t n = n0 + row;
        const UvmPoint pt = uvm_point(uv, emb, list, n, N, res, plan.dims);
        for (int e = wave; e < EP; e += W / 64) act[row * STRIDE + e] = uvm_embed_col(pt, emb, n, N, e, plan.dims, L, plan.in_ch);
    };
    put_embedding();
    __syncthreads();
    if (saved) {   // training: keep the (padded) embedding for the weight gradients of layer 0 and the skip layer
        for (int i = tid; i < UVM_TM * (EP / 4); i += W) {
            int row = i / (EP / 4), c4 = i % (EP / 4);
            if (n0 + row < N) *(float4 *)(saved + (n0 + row) * EP + c4 * 4) = *(const float4 *)(act + row * STRIDE + c4 * 4);
        }
    }

    // ---- hidden layers on the f32 matrix pipe --------------------------------------------------
    for (int li = 0; li < plan.n_hidden; ++li) {
        const UvmLayer ly = plan.layer[li];
        f32x16 acc[2][2];
        uvm_zero(acc[0][0]); uvm_zero(acc[0][1]); uvm_zero(acc[1][0]); uvm_zero(acc[1][1]);
        const float4 *wp = (const float4 *)(packed + ly.w_off) + ((size_t)(wave * 2) * 64 + lane);
        // k-blocks [kb0, kb1) of the layer's packed weights against LDS columns lc0 + 8 (kb - kb0) ...
        auto run_k = [&](int kb0, int kb1, int lc0) {
            const float *arow0 = act + r * STRIDE + lc0 + 4 * h - kb0 * 8;
            uvm_kloop_f32<W>(acc, wp, arow0, arow0 + 32 * STRIDE, kb0, kb1);
        };
        if (!RC) run_k(0, ly.kp / 8, ly.col0);
        else if (ly.kp == EP + W) {                          // skip layer of the overlaid layout: hidden part, then embedding
            run_k(EP / 8, (EP + W) / 8, 0);
            __syncthreads();
            put_embedding();
            __syncthreads();
            run_k(0, EP / 8, 0);
        } else run_k(0, ly.kp / 8, 0);
        __syncthreads();   // everyone has finished reading this layer's input
        const float *bias = packed + ly.b_off;
        unsigned long long relu_bits = 0;   // bit uvm_relu_bit(nb, mb, q) of this lane: its accumulator element is > 0
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            int col = wave * 64 + nb * 32 + r;
            float bv = bias[col];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    float v = acc[mb][nb][q] + bv;
                    relu_bits |= (unsigned long long)(v > 0.f) << uvm_relu_bit(nb, mb, q);
                    act[uvm_acc_row(mb * 32, q, h) * STRIDE + HOFF + col] = v > 0.f ? v : 0.f;
                }
        }
        if (saved) {   // the ReLU pattern in the accumulator layout the backward chain's tiles have: [layer][tile][thread] u64
            unsigned long long *mk = (unsigned long long *)(saved + N * (int64_t)(EP + plan.n_hidden * W));
            mk[((int64_t)li * gridDim.x + blockIdx.x) * W + tid] = relu_bits;
        }
        __syncthreads();
        if (saved) {   // post-ReLU activations [layer][texel][W], whole rows per texel
            float *dst = saved + N * EP + (int64_t)li * N * W;
            for (int i = tid; i < UVM_TM * (W / 4); i += W) {
                int row = i / (W / 4), c4 = i % (W / 4);
                if (n0 + row < N) *(float4 *)(dst + (n0 + row) * W + c4 * 4) = *(const float4 *)(act + row * STRIDE + HOFF + c4 * 4);
            }
        }
    }

    // ---- output layer (W -> out_ch <= 4) on the VALU, 4 lanes per texel ------------------------
    {
        constexpr int PARTS = W / 64;            // threads per texel
        int row = tid / PARTS, part = tid % PARTS;
        const float *a = act + row * STRIDE + HOFF + part * 64;
        const float *ow = packed + plan.out_w_off + part * 64;
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < 64; ++k) {
            float x = a[k];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < plan.out_ch) s[c] += x * ow[c * W + k];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
            for (int o = 1; o < PARTS; o <<= 1) s[c] += __shfl_xor(s[c], o, 64);
        if (part == 0 && n0 + row < N) uvm_store_out(s, packed, plan, raw, tex, list, n0 + row);
    }
}


// =====================================================================================================================
// Fast forward of the 2-D texture field (W = 256): the same network on the 16-bit matrix pipe with SPLIT operands.
// Every activation and weight is carried as two fp16 numbers (uvm_split): 22 bits of mantissa, i.e. fp32-grade operands; the product
// is three v_mfma_f32_32x32x16_f16 passes into two fp32 accumulator sets (uvm_kloop_split).  Per 16-deep k-step that is 3 x 32 cycles
// against 8 x 64 for v_mfma_f32_32x32x2_f32: 5.3x the matrix rate at the f32 path's accuracy (measured against the reference's vectors
// at the same tolerances; CTX_UVMLP_EXACT_F32=1 selects the exact-f32 kernel).
// One workgroup = 64 texels, 4 waves, two workgroups per CU; wave w owns hidden columns [64w, 64w+64) as 2 x 2 accumulator tiles of
// 32 x 32 (x 2 sets), one 32-column block at a time.  Activations live in LDS as two fp16 planes, [64][hi 312 | lo 312 | pad 8].
// `saved` gets what k_uvmlp_fwd leaves (embedding, post-ReLU activations as hi + lo * 2^-11, ReLU bit masks per 64-texel tile).
#define UVM16_LO 312              // halves: a row's lo plane sits this far behind its hi plane (48 + 256 + 8)
#define UVM16_STRIDE 632          // halves per row PAIR (hi | lo): 1264 bytes = 16 x odd -> conflict-free ds_read_b128 over 16 rows, and
                                  // the lo plane within the 16-bit immediate offset of every DS access to the hi plane
__global__ __launch_bounds__(256, 2) void k_uvmlp_fwd16(const float *__restrict__ uv, const float *__restrict__ emb, UvmList list, int64_t N, int res, int L,
                                                     const float *__restrict__ packed, UvmPlan plan,
                                                     float *__restrict__ raw, float *__restrict__ tex, float *__restrict__ saved)
{
    constexpr int W = 256, EP = UVM_EPAD, STRIDE = UVM16_STRIDE;
    extern __shared__ __attribute__((aligned(16))) f16 pl[];      // [64 rows][hi 312 | lo 312 | pad 8] halves
    f16 *phi = pl, *plo = pl + UVM16_LO;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int64_t n0 = (int64_t)blockIdx.x * UVM16_TM;

    // ---- Fourier embedding into columns [0,48): four threads per texel, 12 columns each ------------------------------
    {
        const int row = tid >> 2, quarter = tid & 3;
        const int64_t n = n0 + row;
        const UvmPoint pt = uvm_point(uv, emb, list, n, N, res, plan.dims);
        for (int e = quarter * (EP / 4); e < (quarter + 1) * (EP / 4); ++e)
            uvm_split(uvm_embed_col(pt, emb, n, N, e, plan.dims, L, plan.in_ch), phi[row * STRIDE + e], plo[row * STRIDE + e]);
    }
    __syncthreads();
    if (saved) {
        for (int i = tid; i < UVM16_TM * EP; i += 256) {
            int row = i / EP, c = i % EP;
            if (n0 + row < N) saved[(n0 + row) * EP + c] = uvm_join(phi[row * STRIDE + c], plo[row * STRIDE + c]);
        }
    }

    for (int li = 0; li < plan.n_hidden; ++li) {
        const UvmLayer ly = plan.layer[li];
        const int nkb = ly.kp / 16;
        const f16 *ah_base = phi + r * STRIDE + ly.col0 + 8 * h;
        const f16 *al_base = plo + r * STRIDE + ly.col0 + 8 * h;
        const float *bias = packed + ly.b_off;
        unsigned long long bits0 = 0;              // ReLU pattern of the tile, in k_uvmlp_fwd's bit layout
        uint32_t outv[2][2][16];                   // this layer's outputs (hi | lo << 16) wait in registers until every wave has read its inputs
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {           // the wave's two 32-column blocks one after the other: 64 accumulator registers
            f32x16 acc[2], acx[2];
            uvm_zero(acc[0]); uvm_zero(acx[0]); uvm_zero(acc[1]); uvm_zero(acx[1]);
            const f16 *wbase = (const f16 *)(packed + plan.w16_off[li]) + (size_t)(wave * 2 + nb) * 1024 + lane * 8;
            uvm_kloop_split<STRIDE>(acc, acx, wbase, ah_base, al_base, nkb);
            const float bv = bias[wave * 64 + nb * 32 + r];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const float v = acc[mb][q] + acx[mb][q] * UVM_LO_INV + bv;
                    bits0 |= (unsigned long long)(v > 0.f) << uvm_relu_bit(nb, mb, q);
                    outv[nb][mb][q] = uvm_split_packed(v > 0.f ? v : 0.f);
                }
        }
        __syncthreads();                       // everyone has finished reading this layer's input
        uvm_stage_planes<STRIDE, EP>(phi, plo, outv, wave, r, h);
        if (saved) {
            unsigned long long *mk = (unsigned long long *)(saved + N * (int64_t)(EP + plan.n_hidden * W));
            mk[((int64_t)li * gridDim.x + blockIdx.x) * W + tid] = bits0;
        }
        __syncthreads();
        if (saved) {   // post-ReLU activations [layer][texel][W] as the value the next layer consumes (hi + lo 2^-11)
            float *dst = saved + N * EP + (int64_t)li * N * W;
            for (int i = tid; i < UVM16_TM * (W / 4); i += 256) {
                const int row = i / (W / 4), c4 = i % (W / 4);
                if (n0 + row < N) *(float4 *)(dst + (n0 + row) * W + c4 * 4) = uvm_join4(phi + row * STRIDE + EP + c4 * 4, plo + row * STRIDE + EP + c4 * 4);
            }
        }
    }

    // ---- output layer (256 -> out_ch <= 4) on the VALU, 4 threads per texel ------------------------------------------
    {
        const int row = tid >> 2, part = tid & 3;
        const float *ow = packed + plan.out_w_off + part * 64;
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < 64; k += 8) {
            const f16x8 vh = *(const f16x8 *)(phi + row * STRIDE + EP + part * 64 + k), vl = *(const f16x8 *)(plo + row * STRIDE + EP + part * 64 + k);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float x = uvm_join(vh[j], vl[j]);
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (c < plan.out_ch) s[c] += x * ow[c * W + k + j];
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) { s[c] += __shfl_xor(s[c], 1, 64); s[c] += __shfl_xor(s[c], 2, 64); }
        if (part == 0 && n0 + row < N) uvm_store_out(s, packed, plan, raw, tex, list, n0 + row);
    }
}

extern "C" int64_t ctx_uvmlp_saved_bytes(int64_t N, int32_t D, int32_t W, int32_t input_ch)
{
    if (N <= 0 || !uvm_envelope(D, W, input_ch)) return -1;
    return N * (int64_t)(uvm_epad(input_ch) + D * W) * 4 + (int64_t)D * cdiv64(N, UVM_TM) * W * 8;   // + ReLU bit masks
}

// what the list entry points (2-D field only: they take no dims) refuse; the list's values are the caller's to keep inside [0, res^2) (an entry outside is skipped)
static int32_t uvm_check_list(const char *who, const int32_t *idx, int64_t N, int32_t res)
{
    CTX_REQUIRE(idx, "%s: null texel list", who);
    CTX_REQUIRE(res >= 2 && N >= 1 && N <= (int64_t)res * res, "%s: need res >= 2 and 1 <= N <= res*res (N=%lld res=%d)", who, (long long)N, res);
    return CTX_OK;
}

// idx == nullptr: the points are uv / emb / the whole grid and the atlas plane is N long
// input_ch: the embedding's width, dims * (1 + 2L) where the kernel computes it; any width in [1, 64] on the `emb` seam
static int32_t uvm_fwd(const float *uv, const float *emb, const int32_t *idx, int64_t N, int32_t res, const void *packed, int32_t D, int32_t W,
                       int32_t dims, int32_t L, int32_t input_ch, int32_t output_ch, int32_t skip, float *raw, float *tex_chw, void *saved_v,
                       ctx_stream_t stream)
{
    float *saved = (float *)saved_v;
    UvmPlan p; int64_t total = 0;
    const UvmList list = {idx, idx ? (int64_t)res * res : N};
    CTX_REQUIRE(packed && raw && N > 0, "uvmlp_fwd: bad args");
    CTX_REQUIRE(dims == 2 || dims == 3, "uvmlp_fwd: dims=%d (2: uv, 3: xyz)", dims);
    CTX_REQUIRE(uv || emb || idx || (dims == 2 && res > 1 && (int64_t)res * res == N),
                "uvmlp_fwd: no inputs needs dims == 2 and N == res*res (N=%lld res=%d)", (long long)N, res);
    CTX_REQUIRE(uvm_build_plan(D, W, input_ch, output_ch, skip, p, total) == 0,
                "uvmlp_fwd: unsupported D=%d W=%d dims=%d L=%d input_ch=%d output_ch=%d", D, W, dims, L, input_ch, output_ch);
    p.dims = dims;
    hipStream_t s = (hipStream_t)stream;
    const float *pk = (const float *)packed;
    if (uvm_use_split16(p, dims, false)) {
        const size_t lds16 = (size_t)UVM16_TM * UVM16_STRIDE * sizeof(f16);
        (void)hipFuncSetAttribute((const void *)k_uvmlp_fwd16, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds16);
        hipLaunchKernelGGL(k_uvmlp_fwd16, dim3((unsigned)cdiv64(N, UVM16_TM)), dim3(256), lds16, s, uv, emb, list, N, res, L, pk, p, raw, tex_chw, saved);
        CTX_CHECK_LAUNCH("uvmlp_fwd16");
        return CTX_OK;
    }
    const bool known = uvm_dispatch(W, p.epad, [&](auto w, auto ep) {
        constexpr int WW = decltype(w)::value, EE = decltype(ep)::value;
        const size_t lds = (size_t)UVM_TM * ((EE == UVM_EPAD ? UVM_EPAD : 0) + WW + 4) * 4;   // the 3-D layout overlays the embedding
        (void)hipFuncSetAttribute((const void *)k_uvmlp_fwd<WW, EE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((k_uvmlp_fwd<WW, EE>), dim3((unsigned)cdiv64(N, UVM_TM)), dim3(WW), lds, s, uv, emb, list, N, res, L, pk, p, raw, tex_chw, saved);
    });
    UVM_DISPATCHED(known, "uvmlp_fwd");
    CTX_CHECK_LAUNCH("uvmlp_fwd");
    return CTX_OK;
}

extern "C" int32_t ctx_uvmlp_fwd_save(const float *uv, const float *emb, int64_t N, int32_t res, const void *packed, int32_t D, int32_t W,
                                      int32_t dims, int32_t L, int32_t output_ch, int32_t skip, float *raw, float *tex_chw, void *saved,
                                      ctx_stream_t stream)
{
    return uvm_fwd(uv, emb, nullptr, N, res, packed, D, W, dims, L, dims * (1 + 2 * L), output_ch, skip, raw, tex_chw, saved, stream);
}

extern "C" int32_t ctx_uvmlp_fwd_save_idx(const int32_t *idx, int64_t N, int32_t res, const void *packed, int32_t D, int32_t W, int32_t L,
                                          int32_t output_ch, int32_t skip, float *raw, float *tex_chw, void *saved, ctx_stream_t stream)
{
    if (int32_t rc = uvm_check_list("uvmlp_fwd_save_idx", idx, N, res)) return rc;
    return uvm_fwd(nullptr, nullptr, idx, N, res, packed, D, W, 2, L, 2 * (1 + 2 * L), output_ch, skip, raw, tex_chw, saved, stream);
}

extern "C" int32_t ctx_uvmlp_fwd(const float *uv, const float *emb, int64_t N, int32_t res, const void *packed, int32_t D, int32_t W,
                                 int32_t L, int32_t output_ch, int32_t skip, float *raw, float *tex_chw,
                                 ctx_stream_t stream)
{
    return uvm_fwd(uv, emb, nullptr, N, res, packed, D, W, 2, L, 2 * (1 + 2 * L), output_ch, skip, raw, tex_chw, nullptr, stream);
}

// The `emb` seam on its own: a precomputed embedding of any width input_ch in [1, 64] (the hash-grid field's Lv * F features).  dims = 3 keeps it
// on the exact-f32 chain whatever W is; with input_ch = 63 it is the launch ctx_uvmlp_fwd_save(emb, dims = 3, L = 10) makes.
extern "C" int32_t ctx_uvmlp_fwd_emb(const float *emb, int64_t N, const void *packed, int32_t D, int32_t W, int32_t input_ch, int32_t output_ch,
                                     int32_t skip, float *raw, void *saved, ctx_stream_t stream)
{
    CTX_REQUIRE(emb, "uvmlp_fwd_emb: null embedding");
    CTX_REQUIRE(input_ch >= 1 && input_ch <= UVM_EPAD3, "uvmlp_fwd_emb: input_ch=%d outside [1, %d]", input_ch, UVM_EPAD3);
    return uvm_fwd(nullptr, emb, nullptr, N, 0, packed, D, W, 3, 0, input_ch, output_ch, skip, raw, nullptr, saved, stream);
}

// =====================================================================================================================
// Backward of the texture field (autograd of NeRF2D.forward, src/run_nerf_helpers.py:106-135, as driven by the SDS loop
// src/training/trainer.py:644-907: atlas gradient -> tanh -> MLP -> parameter gradients; uv is not trainable).
//
// Two phases, both on the exact-f32 matrix pipe:
//   k_uvmlp_dgrad : per 64-texel tile, the chain dA_7 = draw . Wout; dZ_i = dA_i * (A_i > 0); dA_{i-1} = dZ_i . W_i[:, hidden]
//                   with dA resident in LDS; every dZ_i goes to HBM [layer][texel][W] (whole rows), and the output layer's
//                   weight / bias gradients are accumulated on the VALU on the way.
//   k_uvmlp_wgrad : dW_i = dZ_i^T . In_i as a split-K GEMM over the texels: a workgroup owns the whole W x cols gradient
//                   in registers (256 accumulator VGPRs per lane for 256 x 256) and walks its texel range two texels per
//                   MFMA k-step; both operands are texel-major, so a lane's operand is ONE dword of a 128-byte row segment
//                   straight from global memory (no LDS, no transposes).  db_i = column sums of dZ_i ride along.
//                   Partial gradients land in per-workgroup slabs and are summed in a fixed order (deterministic).
// =====================================================================================================================
#define UVM_WG_GROUPS 256       // workgroups (= texel ranges) of the weight-gradient GEMMs
#define UVM_WG_GROUPS_EMB 768   // the 48-column embedding gradients run 3 workgroups per CU
#define UVM_DGRAD_GRID 512      // persistent dgrad workgroups (2 per CU)

// ---- what the two dZ-chain kernels share around their K-loops.  W threads; thread (rg, c4) = (row group of 4, float4 column) of a W-wide row ----
struct UvmOutGrad {      // a thread's share of the output layer
    float wo[4][4];      // Wout[c][4 c4 + j] (zero from out_ch on)
    float gwo[4][4];     // the gradient of those weights, summed over the thread's rows
    float gbo;           // the gradient of the bias of channel tid & 3, summed over the thread's draw elements
};
template <int W>
__device__ __forceinline__ void uvm_out_grad_init(UvmOutGrad &og, const float *__restrict__ packed, const UvmPlan &plan, int c4)
{
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            og.wo[c][j] = c < plan.out_ch ? packed[plan.out_w_off + c * W + c4 * 4 + j] : 0.f;
            og.gwo[c][j] = 0.f;
        }
    og.gbo = 0.f;
}
// d loss / d raw of the tile's 64 texels -> dr[64][4]: grad_raw (compact rows) + grad_tex (at the rows' nodes) . d((tanh + 1) / 2)
template <int W>
__device__ __forceinline__ void uvm_draw_tile(float *dr, UvmOutGrad &og, const float *__restrict__ grad_raw, const float *__restrict__ grad_tex,
                                              const float *__restrict__ raw, const UvmList &list, int64_t N, int64_t n0, int out_ch, int tid)
{
    for (int i = tid; i < UVM_TM * 4; i += W) {
        int t = i >> 2, c = i & 3;
        int64_t n = n0 + t;
        float v = 0.f;
        if (n < N && c < out_ch) {
            if (grad_raw) v = grad_raw[n * out_ch + c];
            const int64_t node = grad_tex ? uvm_node(list, n) : -1;
            if (node >= 0) {
                float y = tanhf(raw[n * out_ch + c]);
                v += grad_tex[(int64_t)c * list.plane + node] * 0.5f * (1.0f - y * y);
            }
        }
        dr[i] = v;
        og.gbo += v;
    }
}
// output layer on the VALU (f32): dA = draw . Wout, dWout += draw^T . A, dZ = dA * (A > 0) -> HBM; put(t, o) leaves the thread's four
// columns o[0..3] of row t in LDS in the form the chain's K-loop reads
template <int W, class Put>
__device__ __forceinline__ void uvm_bwd_out_layer(UvmOutGrad &og, const float *dr, const float *__restrict__ a_top, float *__restrict__ dz_top,
                                                  int64_t N, int64_t n0, int rg, int c4, Put put)
{
#pragma unroll 4
    for (int p = 0; p < UVM_TM / 4; ++p) {
        int t = p * 4 + rg;
        int64_t n = n0 + t;
        int64_t nc = n < N ? n : N - 1;
        float4 a = *(const float4 *)(a_top + nc * W + c4 * 4);
        float4 d = *(const float4 *)(dr + t * 4);
        const float av[4] = {a.x, a.y, a.z, a.w}, dv[4] = {d.x, d.y, d.z, d.w};
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float da = dv[0] * og.wo[0][j];
            da = fmaf(dv[1], og.wo[1][j], da);
            da = fmaf(dv[2], og.wo[2][j], da);
            da = fmaf(dv[3], og.wo[3][j], da);
            o[j] = av[j] > 0.f ? da : 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) og.gwo[c][j] = fmaf(dv[c], av[j], og.gwo[c][j]);
        }
        put(t, o);
        if (n < N) *(float4 *)(dz_top + n * W + c4 * 4) = make_float4(o[0], o[1], o[2], o[3]);
    }
}
// output-layer gradients of this workgroup: fold the 4 row groups through gf[16][W], one partial row per channel; dr is scratch for the bias
template <int W>
__device__ __forceinline__ void uvm_fold_out_grad(const UvmOutGrad &og, float *gf, float *dr, float *__restrict__ part_w /*[grid][4][W]*/,
                                                  float *__restrict__ part_b /*[grid][4]*/, int tid, int rg, int c4)
{
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) gf[(rg * 4 + c) * W + c4 * 4 + j] = og.gwo[c][j];
    __syncthreads();
    for (int c = 0; c < 4; ++c) {
        float s = gf[(0 * 4 + c) * W + tid];
        s += gf[(1 * 4 + c) * W + tid];
        s += gf[(2 * 4 + c) * W + tid];
        s += gf[(3 * 4 + c) * W + tid];
        part_w[((int64_t)blockIdx.x * 4 + c) * W + tid] = s;
    }
    dr[tid] = og.gbo;
    __syncthreads();
    if (tid < 4) {
        float s = 0.f;
        for (int i = tid; i < W; i += 4) s += dr[i];
        part_b[(int64_t)blockIdx.x * 4 + tid] = s;
    }
}

template <int W>
__global__ __launch_bounds__(W, 2) void k_uvmlp_dgrad(const float *__restrict__ grad_raw, const float *__restrict__ grad_tex,
                                                   const float *__restrict__ raw, UvmList list, int64_t N, const float *__restrict__ packed,
                                                   UvmPlan plan, const float *__restrict__ saved, float *__restrict__ dz,
                                                   float *__restrict__ part_w /*[grid][4][W]*/, float *__restrict__ part_b /*[grid][4]*/)
{
    constexpr int STRIDE = W + 4;               // 4 x odd
    constexpr int C4N = W / 4;                  // float4 per row; W threads -> 4 rows per pass, 16 passes per tile
    extern __shared__ __attribute__((aligned(16))) float g[];   // [64][STRIDE] dA / dZ, then dr[64][4]
    float *dr = g + UVM_TM * STRIDE;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int c4 = tid % C4N, rg = tid / C4N;
    const int D = plan.n_hidden;
    const float *acts = saved + N * plan.epad;
    const unsigned long long *masks = (const unsigned long long *)(saved + N * (int64_t)(plan.epad + D * W));
    UvmOutGrad og;
    uvm_out_grad_init<W>(og, packed, plan, c4);

    const int64_t ntiles = (N + UVM_TM - 1) / UVM_TM;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t n0 = tile * UVM_TM;
        uvm_draw_tile<W>(dr, og, grad_raw, grad_tex, raw, list, N, n0, plan.out_ch, tid);
        __syncthreads();
        uvm_bwd_out_layer<W>(og, dr, acts + (int64_t)(D - 1) * N * W, dz + (int64_t)(D - 1) * N * W, N, n0, rg, c4,
                             [&](int t, const float (&o)[4]) { *(float4 *)(g + t * STRIDE + c4 * 4) = make_float4(o[0], o[1], o[2], o[3]); });
        __syncthreads();
        // ---- hidden layers, last to second ------------------------------------------------------
        for (int li = D - 1; li >= 1; --li) {
            float *dz_prev = dz + (int64_t)(li - 1) * N * W;
            const unsigned long long relu_bits = masks[((int64_t)(li - 1) * ntiles + tile) * W + tid];
            f32x16 acc[2][2];
            uvm_zero(acc[0][0]); uvm_zero(acc[0][1]); uvm_zero(acc[1][0]); uvm_zero(acc[1][1]);
            const float4 *wp = (const float4 *)(packed + plan.wt_off[li]) + ((size_t)(wave * 2) * 64 + lane);
            const float *arow0 = g + r * STRIDE + 4 * h;
            uvm_kloop_f32<W>(acc, wp, arow0, arow0 + 32 * STRIDE, 0, W / 8);
            __syncthreads();                     // all fragment reads of dZ_li (and the row copies of it below) are done
            // dZ_{li-1} = dA_{li-1} * relu'(layer li-1): the forward left the pattern in this very accumulator layout
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                int col = wave * 64 + nb * 32 + r;
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        bool on = (relu_bits >> uvm_relu_bit(nb, mb, q)) & 1ull;
                        g[uvm_acc_row(mb * 32, q, h) * STRIDE + col] = on ? acc[mb][nb][q] : 0.f;
                    }
            }
            __syncthreads();
            // whole rows of dZ_{li-1} to HBM; the next layer's fragment reads of g run alongside (both only read)
#pragma unroll 4
            for (int p = 0; p < UVM_TM / 4; ++p) {
                int t = p * 4 + rg;
                int64_t n = n0 + t;
                if (n < N) *(float4 *)(dz_prev + n * W + c4 * 4) = *(const float4 *)(g + t * STRIDE + c4 * 4);
            }
        }
        __syncthreads();                         // the last row copies read g before the next tile overwrites it
    }
    uvm_fold_out_grad<W>(og, g, dr, part_w, part_b, tid, rg, c4);
}

// ---- the dZ chain on the 16-bit matrix pipe with split operands (the backward twin of k_uvmlp_fwd16) ---------------------------------
// Same phases and outputs as k_uvmlp_dgrad<256>; the chain's GEMMs dA_{i-1} = dZ_i . W_i[:, hidden] run as three v_mfma_f32_32x32x16_f16
// passes over (hi, lo) planes of dZ (LDS) and of the weights (L2).  Gradients have no natural scale (1e-8 under a mean-reduced loss):
// every op of the chain is linear, so the tile's draw is multiplied by 2^e with e from a device reduction of max|grad| (the largest
// draw lands near 16: room for a 4 000-fold growth through the layers before fp16 overflows, 2^-35 of the maximum still resolved), and
// dZ goes to HBM multiplied by 2^-e (exact).
struct UvmCtl { uint32_t absmax_raw, absmax_tex; int32_t e; int32_t pad; };
// a: grad_raw, na elements; b: grad_tex [out_ch][plane], nb_ = out_ch * N elements of it: all of it, or the listed nodes of every plane
__global__ __launch_bounds__(256) void k_uvm_absmax(const float *__restrict__ a, int64_t na, const float *__restrict__ b, int64_t nb_, UvmList list, int64_t N,
                                                    UvmCtl *__restrict__ ctl)
{
    uint32_t ma = 0, mb = 0;
    const int64_t stride = (int64_t)gridDim.x * 256, i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a) for (int64_t i = i0; i < na; i += stride) ma = max(ma, __float_as_uint(a[i]) & 0x7fffffffu);
    if (b && !list.idx) for (int64_t i = i0; i < nb_; i += stride) mb = max(mb, __float_as_uint(b[i]) & 0x7fffffffu);
    if (b && list.idx)
        for (int64_t i = i0; i < nb_; i += stride) {
            const int64_t node = uvm_node(list, i % N);
            if (node >= 0) mb = max(mb, __float_as_uint(b[(i / N) * list.plane + node]) & 0x7fffffffu);
        }
    for (int o = 32; o; o >>= 1) { ma = max(ma, (uint32_t)__shfl_xor((int)ma, o)); mb = max(mb, (uint32_t)__shfl_xor((int)mb, o)); }
    __shared__ uint32_t s_m[2][4];                 // one atomic pair per workgroup (atomics on one address serialise)
    if ((threadIdx.x & 63) == 0) { s_m[0][threadIdx.x >> 6] = ma; s_m[1][threadIdx.x >> 6] = mb; }
    __syncthreads();
    if (threadIdx.x == 0) {
        ma = max(max(s_m[0][0], s_m[0][1]), max(s_m[0][2], s_m[0][3]));
        mb = max(max(s_m[1][0], s_m[1][1]), max(s_m[1][2], s_m[1][3]));
        if (ma) atomicMax(&ctl->absmax_raw, ma);
        if (mb) atomicMax(&ctl->absmax_tex, mb);
    }
}
__global__ void k_uvm_scale(UvmCtl *ctl)
{
    // |draw| <= |grad_raw| + 0.5 |grad_tex| (tanh' <= 1); non-finite or zero gradients: no scaling (they propagate as they are)
    const float bound = __uint_as_float(ctl->absmax_raw) + 0.5f * __uint_as_float(ctl->absmax_tex);
    int e = 0;
    if (bound > 0.f && bound < INFINITY) { int x; (void)frexpf(bound, &x); e = 4 - x; }
    ctl->e = e;
}

#define UVM16B_LO 264             // halves: dZ's lo plane behind its hi plane (256 + 8)
#define UVM16B_STRIDE 536         // halves per row pair: 1072 bytes = 16 x odd
__global__ __launch_bounds__(256, 2) void k_uvmlp_dgrad16(const float *__restrict__ grad_raw, const float *__restrict__ grad_tex,
                                                          const float *__restrict__ raw, UvmList list, int64_t N, const float *__restrict__ packed,
                                                          UvmPlan plan, const float *__restrict__ saved, float *__restrict__ dz,
                                                          float *__restrict__ part_w, float *__restrict__ part_b, const UvmCtl *__restrict__ ctl)
{
    constexpr int W = 256, STRIDE = UVM16B_STRIDE, C4N = W / 4;
    extern __shared__ __attribute__((aligned(16))) f16 gp[];       // [64][hi 264 | lo 264 | 8] halves, then dr[64][4] floats
    f16 *ghi = gp, *glo = gp + UVM16B_LO;
    float *dr = (float *)(gp + UVM_TM * STRIDE);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int c4 = tid % C4N, rg = tid / C4N;
    const int D = plan.n_hidden;
    const float *acts = saved + N * plan.epad;
    const unsigned long long *masks = (const unsigned long long *)(saved + N * (int64_t)(plan.epad + D * W));
    const int e = ctl->e;
    UvmOutGrad og;
    uvm_out_grad_init<W>(og, packed, plan, c4);

    const int64_t ntiles = (N + UVM_TM - 1) / UVM_TM;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t n0 = tile * UVM_TM;
        uvm_draw_tile<W>(dr, og, grad_raw, grad_tex, raw, list, N, n0, plan.out_ch, tid);
        __syncthreads();
        // dZ of the output layer goes to HBM as it is, to LDS scaled and split
        uvm_bwd_out_layer<W>(og, dr, acts + (int64_t)(D - 1) * N * W, dz + (int64_t)(D - 1) * N * W, N, n0, rg, c4,
                             [&](int t, const float (&o)[4]) {
                                 const float sv[4] = {ldexpf(o[0], e), ldexpf(o[1], e), ldexpf(o[2], e), ldexpf(o[3], e)};
                                 f16x4 oh, ol;
                                 uvm_split4(sv, oh, ol);
                                 *(f16x4 *)(ghi + t * STRIDE + c4 * 4) = oh;
                                 *(f16x4 *)(glo + t * STRIDE + c4 * 4) = ol;
                             });
        __syncthreads();
        // ---- hidden layers, last to second ------------------------------------------------------------------------------
        for (int li = D - 1; li >= 1; --li) {
            float *dz_prev = dz + (int64_t)(li - 1) * N * W;
            const unsigned long long relu_bits = masks[((int64_t)(li - 1) * ntiles + tile) * W + tid];
            const f16 *ah_base = ghi + r * STRIDE + 8 * h, *al_base = glo + r * STRIDE + 8 * h;
            uint32_t outv[2][2][16];
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                f32x16 acc[2], acx[2];
                uvm_zero(acc[0]); uvm_zero(acx[0]); uvm_zero(acc[1]); uvm_zero(acx[1]);
                const f16 *wbase = (const f16 *)(packed + plan.wt16_off[li]) + (size_t)(wave * 2 + nb) * 1024 + lane * 8;
                uvm_kloop_split<STRIDE>(acc, acx, wbase, ah_base, al_base, W / 16);   // a constant, even count: no tail
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const bool on = (relu_bits >> uvm_relu_bit(nb, mb, q)) & 1ull;
                        outv[nb][mb][q] = uvm_split_packed(on ? acc[mb][q] + acx[mb][q] * UVM_LO_INV : 0.f);
                    }
            }
            __syncthreads();                     // all fragment reads of dZ_li (and the row copies of it below) are done
            uvm_stage_planes<STRIDE, 0>(ghi, glo, outv, wave, r, h);
            __syncthreads();
            // whole rows of dZ_{li-1} to HBM, unscaled; the next layer's fragment reads run alongside (both only read)
#pragma unroll 4
            for (int p = 0; p < UVM_TM / 4; ++p) {
                int t = p * 4 + rg;
                int64_t n = n0 + t;
                if (n < N) {
                    const float4 v = uvm_join4(ghi + t * STRIDE + c4 * 4, glo + t * STRIDE + c4 * 4);
                    *(float4 *)(dz_prev + n * W + c4 * 4) = make_float4(ldexpf(v.x, -e), ldexpf(v.y, -e), ldexpf(v.z, -e), ldexpf(v.w, -e));
                }
            }
        }
        __syncthreads();                         // the last row copies read the planes before the next tile overwrites them
    }
    uvm_fold_out_grad<W>(og, (float *)gp /* 16 x 256 floats */, dr, part_w, part_b, tid, rg, c4);
}

// dW[rows x cols] = dZ^T . In over the texel range of this workgroup.  Waves WR x WC, wave tile (32 NI) x (32 NJ).
// Row strides are compile-time (LDZ = W = rows, LDIN = W or 48) so the operand loads of a whole k-step group hang off two
// running pointers with immediate offsets; only the last, ragged texel range takes the bounds-checked path.
template <int WR, int WC, int NI, int NJ, int LDZ, int LDIN, int INCOLS>
__global__ __launch_bounds__(64 * WR * WC)
void k_uvmlp_wgrad(const float *__restrict__ dz, const float *__restrict__ in, int64_t N, int64_t chunk, float *__restrict__ slab,
                   float *__restrict__ bslab)
{
    constexpr int ROWS = WR * NI * 32, COLS = WC * NJ * 32;
    static_assert(ROWS == LDZ && COLS >= INCOLS, "workgroup owns the whole gradient");
    constexpr int U = 4;                         // k-steps (2 texels each) per buffer
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wr = wave / WC, wc = wave % WC;
    const int row0 = wr * NI * 32, col0 = wc * NJ * 32;
    const int64_t t_begin = (int64_t)blockIdx.x * chunk;
    const int64_t t_end = t_begin + chunk < N ? t_begin + chunk : N;

    f32x16 acc[NI][NJ];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
    float bs[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) bs[i] = 0.f;
    int bcol[NJ]; bool bok[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        int cc = col0 + j * 32 + r;
        bok[j] = cc < INCOLS;
        bcol[j] = bok[j] ? cc : INCOLS - 1;
    }
    float a0[U][NI], b0[U][NJ], a1[U][NI], b1[U][NJ];
    auto mma = [&](const float (&a)[U][NI], const float (&b)[U][NJ]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int i = 0; i < NI; ++i) {
#pragma unroll
                for (int j = 0; j < NJ; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][i], b[u][j], acc[i][j], 0, 0, 0);
                bs[i] += a[u][i];
            }
        }
    };
    if (t_begin + chunk <= N) {
        // ---- whole range: no bounds checks.  Three operand buffers of U k-steps: while buffer p feeds the matrix pipe, the
        // buffer consumed one phase ago is refilled (8 loads after each k-step's 16 MFMAs) and is used one phase later, so a
        // whole phase (U x 1024 MFMA cycles) covers the memory latency and the waits are vmcnt(one buffer), never 0.
        const float *zp = dz + (t_begin + h) * LDZ + row0 + r;
        const float *ip = in + (t_begin + h) * LDIN;
        float a2[U][NI], b2[U][NJ];
        auto load_step = [&](int u, float (&a)[U][NI], float (&b)[U][NJ]) {
#pragma unroll
            for (int i = 0; i < NI; ++i) a[u][i] = zp[u * 2 * LDZ + i * 32];
#pragma unroll
            for (int j = 0; j < NJ; ++j) b[u][j] = ip[u * 2 * LDIN + bcol[j]];
        };
        auto phase = [&](const float (&a)[U][NI], const float (&b)[U][NJ], float (&na)[U][NI], float (&nb)[U][NJ]) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float bv[NJ];
#pragma unroll
                for (int j = 0; j < NJ; ++j) bv[j] = (INCOLS == COLS || bok[j]) ? b[u][j] : 0.f;
#pragma unroll
                for (int i = 0; i < NI; ++i) {
#pragma unroll
                    for (int j = 0; j < NJ; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][i], bv[j], acc[i][j], 0, 0, 0);
                    bs[i] += a[u][i];
                }
                load_step(u, na, nb);
                __builtin_amdgcn_sched_barrier(0);
            }
            zp += 2 * U * LDZ; ip += 2 * U * LDIN;
        };
        // prologue: buffers 0 and 1; zp / ip then point at the rows of the buffer to refill next
#pragma unroll
        for (int u = 0; u < U; ++u) load_step(u, a0, b0);
        zp += 2 * U * LDZ; ip += 2 * U * LDIN;
#pragma unroll
        for (int u = 0; u < U; ++u) load_step(u, a1, b1);
        zp += 2 * U * LDZ; ip += 2 * U * LDIN;
        __builtin_amdgcn_sched_barrier(0);
        // chunk is a multiple of 3 buffers (48 texels); the refills of the last two phases read (in-bounds or next-range)
        // rows that are never used: keep them in bounds by stepping back at the end
        const int rounds = (int)(chunk / (6 * U));
        const float *zlast = dz + (N - 2 * U + h) * LDZ + row0 + r;     // last whole buffer of the array
        const float *ilast = in + (N - 2 * U + h) * LDIN;
        for (int it = 0; it < rounds; ++it) {
            const bool tail = it + 1 == rounds;
            phase(a0, b0, a2, b2);
            if (tail) { zp = zlast; ip = ilast; }
            phase(a1, b1, a0, b0);
            if (tail) { zp = zlast; ip = ilast; }
            phase(a2, b2, a1, b1);
        }
    } else {
        auto fetch = [&](int64_t t, float (&a)[U][NI], float (&b)[U][NJ]) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                int64_t tt = t + 2 * u + h;
                bool ok = tt < t_end;
                int64_t tc = tt < N ? tt : N - 1;
                const float *zp = dz + tc * LDZ + row0 + r;
                const float *ip = in + tc * LDIN;
#pragma unroll
                for (int i = 0; i < NI; ++i) { float v = zp[i * 32]; a[u][i] = ok ? v : 0.f; }
#pragma unroll
                for (int j = 0; j < NJ; ++j) { float v = ip[bcol[j]]; b[u][j] = bok[j] ? v : 0.f; }
            }
        };
        fetch(t_begin, a0, b0);
        for (int64_t t = t_begin; t < t_end; t += 4 * U) {
            fetch(t + 2 * U, a1, b1);            // past-the-end fetches are clamped and zeroed
            mma(a0, b0);
            fetch(t + 4 * U, a0, b0);
            mma(a1, b1);
        }
    }
    float *sl = slab + (int64_t)blockIdx.x * ROWS * COLS;
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                int n = uvm_acc_row(row0 + i * 32, q, h);
                sl[n * COLS + col0 + j * 32 + r] = acc[i][j][q];
            }
    if (wc == 0 && bslab) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            float v = bs[i] + __shfl_xor(bs[i], 32, 64);
            if (h == 0) bslab[(int64_t)blockIdx.x * ROWS + row0 + i * 32 + r] = v;
        }
    }
}

// out[n][col_off + k] = sum_g slab[g][n][k]  (fixed order), k < out_cols.  One thread per (4 columns, quarter of the groups):
// 16-byte loads, the four quarters folded through LDS in a fixed order.  cols_pad % 4 == 0.
__global__ __launch_bounds__(256) void k_uvm_reduce(const float *__restrict__ slab, int G, int64_t stride, int rows, int cols_pad,
                                                    int out_cols, float *__restrict__ out, int ld_out, int col_off)
{
    __shared__ float4 part[4][64];
    const int q = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int idx4 = blockIdx.x * 64 + l;                    // float4 index within rows x cols_pad
    const int total4 = rows * cols_pad / 4;
    const int gq = (G + 3) / 4;
    const int g0 = q * gq, g1 = (g0 + gq < G ? g0 + gq : G);
    float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
    if (idx4 < total4) {
        const float4 *p = (const float4 *)slab + idx4;
        const int64_t st4 = stride / 4;
        int gi = g0;
        for (; gi + 2 <= g1; gi += 2) {
            float4 a = p[gi * st4], b = p[(gi + 1) * st4];
            s0.x += a.x; s0.y += a.y; s0.z += a.z; s0.w += a.w;
            s1.x += b.x; s1.y += b.y; s1.z += b.z; s1.w += b.w;
        }
        if (gi < g1) { float4 a = p[gi * st4]; s0.x += a.x; s0.y += a.y; s0.z += a.z; s0.w += a.w; }
    }
    part[q][l] = make_float4(s0.x + s1.x, s0.y + s1.y, s0.z + s1.z, s0.w + s1.w);
    __syncthreads();
    if (q == 0 && idx4 < total4) {
        float4 a = part[0][l], b = part[1][l], c = part[2][l], d = part[3][l];
        const float v[4] = {(a.x + b.x) + (c.x + d.x), (a.y + b.y) + (c.y + d.y), (a.z + b.z) + (c.z + d.z), (a.w + b.w) + (c.w + d.w)};
        const int n = idx4 * 4 / cols_pad, k = idx4 * 4 % cols_pad;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (k + j < out_cols) out[(int64_t)n * ld_out + col_off + k + j] = v[j];
    }
}

// ---- gradient of the `emb` seam: grad_emb[n][e] = sum_j dZ_0[n][j] W_0[j][e] + sum_j dZ_s[n][j] W_s[j][e], s = skip + 1, e < in_ch --------
// (the skip layer's first in_ch weight columns are its embedding part).  Reads the dZ rows k_uvmlp_dgrad left in the workspace and the
// forward's packed weights (k_uvm_pack's fragment order: element (j, k) of a layer sits in block (k / 8, j / 32), lane (j % 32) + 32 (k % 8 / 4),
// slot k % 4; both layers hold the padded embedding in k < epad).  One workgroup = 64 points x 64 columns as a register-tiled product on the
// VALU: thread (pg, eg) owns points 4 pg .. 4 pg + 3 and columns 4 eg .. 4 eg + 3, and walks K = 2 W in chunks of 64 staged through LDS.
// HBM floor: the 2 N W 4 bytes of dZ it reads (+ N in_ch 4 written).
#define UVM_GE_LD 68      // floats per staged row: 16-byte aligned, 4 x odd
__global__ __launch_bounds__(256) void k_uvmlp_grad_emb(const float *__restrict__ dz0, const float *__restrict__ dzs, int64_t N, int W,
                                                        const float *__restrict__ w0, const float *__restrict__ wsk, int in_ch, int epad,
                                                        float *__restrict__ grad_emb)
{
    __shared__ __attribute__((aligned(16))) float dzt[UVM_TM * UVM_GE_LD];   // [point][j]
    __shared__ __attribute__((aligned(16))) float wt[64 * UVM_GE_LD];        // [j][e]
    const int tid = threadIdx.x, eg = tid & 15, pg = tid >> 4;
    const int64_t n0 = (int64_t)blockIdx.x * UVM_TM;
    const bool live = eg * 4 < in_ch;
    float acc[4][4] = {};
    for (int src = 0; src < 2; ++src) {
        const float *dz = src ? dzs : dz0;
        const float *wp = src ? wsk : w0;
        for (int jc = 0; jc < W / 64; ++jc) {
            __syncthreads();                       // the previous chunk has been consumed
            for (int q = tid; q < UVM_TM * 16; q += 256) {
                const int row = q >> 4, c4 = q & 15;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (n0 + row < N) v = *(const float4 *)(dz + (n0 + row) * W + jc * 64 + c4 * 4);
                *(float4 *)(dzt + row * UVM_GE_LD + c4 * 4) = v;
            }
            for (int q = tid; q < 1024; q += 256) {
                const int lane = q & 63, nbl = (q >> 6) & 1, kb = q >> 7;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (kb * 8 < epad) v = *(const float4 *)(wp + (((int64_t)kb * (W / 32) + jc * 2 + nbl) * 64 + lane) * 4);
                *(float4 *)(wt + (nbl * 32 + (lane & 31)) * UVM_GE_LD + kb * 8 + 4 * (lane >> 5)) = v;
            }
            __syncthreads();
            if (live) {
#pragma unroll 8
                for (int j = 0; j < 64; ++j) {
                    const float4 b = *(const float4 *)(wt + j * UVM_GE_LD + eg * 4);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float a = dzt[(pg * 4 + i) * UVM_GE_LD + j];
                        acc[i][0] += a * b.x; acc[i][1] += a * b.y; acc[i][2] += a * b.z; acc[i][3] += a * b.w;
                    }
                }
            }
        }
    }
    if (live)
        for (int i = 0; i < 4; ++i) {
            const int64_t n = n0 + pg * 4 + i;
            if (n < N)
                for (int c = 0; c < 4; ++c)
                    if (eg * 4 + c < in_ch) grad_emb[n * in_ch + eg * 4 + c] = acc[i][c];
        }
}

static inline int64_t uvm_align(int64_t x) { return (x + 255) & ~(int64_t)255; }

// The backward's workspace: byte offsets of its parts and the total.  ctx_uvmlp_bwd_ws_bytes and ctx_uvmlp_bwd both take it from here.
struct UvmWs { int64_t dz, slab, bslab, part_w, part_b, ctl, bytes; };
static UvmWs uvm_ws_layout(int64_t N, int D, int W)
{
    UvmWs l;
    int64_t off = 0;
    auto carve = [&](int64_t bytes) { const int64_t at = off; off += uvm_align(bytes); return at; };
    // every workgroup of a weight-gradient launch owns one slab: up to UVM_WG_GROUPS of W x max(W, 64) floats (hidden part),
    // up to UVM_WG_GROUPS_EMB of W x 64 (embedding part, whichever its padded width)
    const int64_t slab_hid = (int64_t)UVM_WG_GROUPS * W * (W > 64 ? W : 64), slab_emb = (int64_t)UVM_WG_GROUPS_EMB * W * 64;
    l.dz = carve((int64_t)D * N * W * 4);                              // dZ [layer][texel][W]
    l.slab = carve((slab_hid > slab_emb ? slab_hid : slab_emb) * 4);   // weight-gradient slabs
    l.bslab = carve((int64_t)UVM_WG_GROUPS_EMB * W * 4);               // bias slabs
    l.part_w = carve((int64_t)UVM_DGRAD_GRID * 4 * W * 4);             // output-layer weight partials
    l.part_b = carve((int64_t)UVM_DGRAD_GRID * 4 * 4);                 // output-layer bias partials
    l.ctl = carve(256);                                                // control words of the split-fp16 chain (gradient scale)
    l.bytes = off;
    return l;
}

extern "C" int64_t ctx_uvmlp_bwd_ws_bytes(int64_t N, int32_t D, int32_t W)
{
    if (N <= 0 || !uvm_envelope(D, W)) return -1;
    return uvm_ws_layout(N, D, W).bytes;
}

template <int WR, int WC, int NI, int NJ, int LDZ, int LDIN, int INCOLS>
static void uvm_launch_wgrad(int G, const float *dz, const float *in, int64_t N, int64_t chunk, float *slab, float *bslab, hipStream_t s)
{
    hipLaunchKernelGGL((k_uvmlp_wgrad<WR, WC, NI, NJ, LDZ, LDIN, INCOLS>), dim3(G), dim3(64 * WR * WC), 0, s, dz, in, N, chunk, slab,
                       bslab);
}

// idx == nullptr: grad_tex is [output_ch][N]; else [output_ch][res^2], read at the listed nodes
static int32_t uvm_bwd(const float *grad_raw, const float *grad_tex, const int32_t *idx, int32_t res, const float *raw, int64_t N, const void *packed,
                       int32_t D, int32_t W, int32_t dims, int32_t L, int32_t input_ch, int32_t output_ch, int32_t skip, const void *saved_v,
                       void *ws, float *const *gws, float *const *gbs, float *grad_emb, ctx_stream_t stream)
{
    UvmPlan p; int64_t total = 0;
    const UvmList list = {idx, idx ? (int64_t)res * res : N};
    // gws and gbs both null with a grad_emb: the input gradient alone (the dZ chain and k_uvmlp_grad_emb), no weight-gradient launch
    const bool want_w = gws || gbs || !grad_emb;
    CTX_REQUIRE(packed && saved_v && ws && (!want_w || (gws && gbs)) && N > 0, "uvmlp_bwd: bad args");
    CTX_REQUIRE(grad_raw || grad_tex, "uvmlp_bwd: need grad_raw and / or grad_tex");
    CTX_REQUIRE(!grad_tex || raw, "uvmlp_bwd: grad_tex needs raw (the tanh argument)");
    CTX_REQUIRE(dims == 2 || dims == 3, "uvmlp_bwd: dims=%d (2: uv, 3: xyz)", dims);
    CTX_REQUIRE(uvm_build_plan(D, W, input_ch, output_ch, skip, p, total) == 0,
                "uvmlp_bwd: unsupported D=%d W=%d dims=%d L=%d input_ch=%d output_ch=%d", D, W, dims, L, input_ch, output_ch);
    p.dims = dims;
    CTX_REQUIRE(skip >= 0 && skip + 1 < D, "uvmlp_bwd: skip=%d outside [0, D-2]", skip);
    for (int i = 0; want_w && i <= D; ++i) CTX_REQUIRE(gws[i] && gbs[i], "uvmlp_bwd: null gradient pointer for layer %d", i);
    hipStream_t s = (hipStream_t)stream;
    const float *pk = (const float *)packed;
    const float *saved = (const float *)saved_v;
    const UvmWs l = uvm_ws_layout(N, D, W);
    char *const base = (char *)ws;
    float *dz = (float *)(base + l.dz), *slab = (float *)(base + l.slab), *bslab = (float *)(base + l.bslab);
    float *part_w = (float *)(base + l.part_w), *part_b = (float *)(base + l.part_b);
    UvmCtl *ctl = (UvmCtl *)(base + l.ctl);

    // ---- phase 1: the dZ chain ----
    int64_t ntiles = cdiv64(N, UVM_TM);
    int dg = (int)(ntiles < UVM_DGRAD_GRID ? ntiles : UVM_DGRAD_GRID);
    if (uvm_use_split16(p, dims, true)) {
        // split-fp16 chain: scale from max|grad| on the device, then the same phases as the f32 kernel
        (void)hipMemsetAsync(ctl, 0, sizeof(UvmCtl), s);
        hipLaunchKernelGGL(k_uvm_absmax, dim3(512), dim3(256), 0, s, grad_raw, grad_raw ? N * output_ch : 0, grad_tex, grad_tex ? N * output_ch : 0, list, N, ctl);
        hipLaunchKernelGGL(k_uvm_scale, dim3(1), dim3(1), 0, s, ctl);
        const size_t lds16 = (size_t)UVM_TM * UVM16B_STRIDE * sizeof(f16) + UVM_TM * 4 * 4;
        (void)hipFuncSetAttribute((const void *)k_uvmlp_dgrad16, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds16);
        hipLaunchKernelGGL(k_uvmlp_dgrad16, dim3(dg), dim3(256), lds16, s, grad_raw, grad_tex, raw, list, N, pk, p, saved, dz, part_w, part_b, ctl);
    } else {
        const bool known = uvm_dispatch(W, p.epad, [&](auto w, auto) {
            constexpr int WW = decltype(w)::value;
            const size_t lds = (size_t)(UVM_TM * (WW + 4) + UVM_TM * 4) * 4;
            (void)hipFuncSetAttribute((const void *)k_uvmlp_dgrad<WW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(k_uvmlp_dgrad<WW>, dim3(dg), dim3(WW), lds, s, grad_raw, grad_tex, raw, list, N, pk, p, saved, dz, part_w, part_b);
        });
        UVM_DISPATCHED(known, "uvmlp_dgrad");
    }
    CTX_CHECK_LAUNCH("uvmlp_dgrad");
    if (want_w) {
        hipLaunchKernelGGL(k_uvm_reduce, dim3(cdiv(output_ch * W / 4, 64)), dim3(256), 0, s, part_w, dg, (int64_t)4 * W, output_ch, W, W,
                           gws[D], W, 0);
        hipLaunchKernelGGL(k_uvm_reduce, dim3(1), dim3(256), 0, s, part_b, dg, (int64_t)4, 1, 4, output_ch, gbs[D], 4, 0);
        CTX_CHECK_LAUNCH("uvmlp_reduce_out");
    }

    // ---- phase 2: weight / bias gradients ----
    int64_t chunk = cdiv64(N, UVM_WG_GROUPS);
    chunk = (chunk + 47) / 48 * 48;              // whole rounds of both loop forms (3 buffers x 4 k-steps x 2 texels; 16)
    int G = (int)cdiv64(N, chunk);
    int64_t chunk_e = cdiv64(N, UVM_WG_GROUPS_EMB);
    chunk_e = (chunk_e + 47) / 48 * 48;
    int Ge = (int)cdiv64(N, chunk_e);
    const float *emb = saved;
    const float *acts = saved + N * p.epad;
    const char *wg8_env = getenv("CTX_UVM_WG8");   // read on every call, like CTX_UVMLP_EXACT_F32: the switch may be flipped inside one process
    const int wg8 = wg8_env ? atoi(wg8_env) : 0;
    for (int li = D - 1; want_w && li >= 0; --li) {
        const float *dzl = dz + (int64_t)li * N * W;
        const int kin = li == 0 ? input_ch : (li == skip + 1 ? input_ch + W : W);
        const bool has_emb = li == 0 || li == skip + 1;
        const bool has_hid = li != 0;
        if (has_hid) {
            const float *in = acts + (int64_t)(li - 1) * N * W;
            const bool known = uvm_dispatch(W, p.epad, [&](auto w, auto) {
                constexpr int WW = decltype(w)::value;
                if (WW == 256 && wg8) uvm_launch_wgrad<2, 4, 4, 2, 256, 256, 256>(G, dzl, in, N, chunk, slab, bslab, s);
                else uvm_launch_wgrad<2, 2, WW / 64, WW / 64, WW, WW, WW>(G, dzl, in, N, chunk, slab, bslab, s);
            });
            UVM_DISPATCHED(known, "uvmlp_wgrad");
            CTX_CHECK_LAUNCH("uvmlp_wgrad");
            hipLaunchKernelGGL(k_uvm_reduce, dim3(cdiv(W * W / 4, 64)), dim3(256), 0, s, slab, G, (int64_t)W * W, W, W, W, gws[li], kin,
                               has_emb ? input_ch : 0);
            hipLaunchKernelGGL(k_uvm_reduce, dim3(cdiv(W / 4, 64)), dim3(256), 0, s, bslab, G, (int64_t)W, 1, W, W, gbs[li], W, 0);
        }
        if (has_emb) {
            float *bsl = has_hid ? nullptr : bslab;
            const bool known = uvm_dispatch(W, p.epad, [&](auto w, auto ep) {
                constexpr int WW = decltype(w)::value, EE = decltype(ep)::value;
                uvm_launch_wgrad<WW / 64, 1, 2, 2, WW, EE, EE>(Ge, dzl, emb, N, chunk_e, slab, bsl, s);
            });
            UVM_DISPATCHED(known, "uvmlp_wgrad_emb");
            CTX_CHECK_LAUNCH("uvmlp_wgrad_emb");
            hipLaunchKernelGGL(k_uvm_reduce, dim3(cdiv(W * 64 / 4, 64)), dim3(256), 0, s, slab, Ge, (int64_t)W * 64, W, 64, input_ch, gws[li], kin, 0);
            if (!has_hid)
                hipLaunchKernelGGL(k_uvm_reduce, dim3(cdiv(W / 4, 64)), dim3(256), 0, s, bslab, Ge, (int64_t)W, 1, W, W, gbs[li], W, 0);
        }
        CTX_CHECK_LAUNCH("uvmlp_wgrad_reduce");
    }
    if (grad_emb) {   // the input gradient, from the dZ rows of the two layers that read the embedding
        hipLaunchKernelGGL(k_uvmlp_grad_emb, dim3((unsigned)ntiles), dim3(256), 0, s, dz, dz + (int64_t)(skip + 1) * N * W, N, W, pk + p.layer[0].w_off,
                           pk + p.layer[skip + 1].w_off, input_ch, p.epad, grad_emb);
        CTX_CHECK_LAUNCH("uvmlp_grad_emb");
    }
    return CTX_OK;
}

extern "C" int32_t ctx_uvmlp_bwd(const float *grad_raw, const float *grad_tex, const float *raw, int64_t N, const void *packed,
                                 int32_t D, int32_t W, int32_t dims, int32_t L, int32_t output_ch, int32_t skip, const void *saved, void *ws,
                                 float *const *gws, float *const *gbs, ctx_stream_t stream)
{
    return uvm_bwd(grad_raw, grad_tex, nullptr, 0, raw, N, packed, D, W, dims, L, dims * (1 + 2 * L), output_ch, skip, saved, ws, gws, gbs, nullptr, stream);
}

extern "C" int32_t ctx_uvmlp_bwd_idx(const float *grad_raw, const float *grad_tex, const int32_t *idx, int32_t res, const float *raw, int64_t N,
                                     const void *packed, int32_t D, int32_t W, int32_t L, int32_t output_ch, int32_t skip, const void *saved,
                                     void *ws, float *const *gws, float *const *gbs, ctx_stream_t stream)
{
    if (int32_t rc = uvm_check_list("uvmlp_bwd_idx", idx, N, res)) return rc;
    return uvm_bwd(grad_raw, grad_tex, idx, res, raw, N, packed, D, W, 2, L, 2 * (1 + 2 * L), output_ch, skip, saved, ws, gws, gbs, nullptr, stream);
}

// ctx_uvmlp_bwd of the `emb` seam (ctx_uvmlp_fwd_emb's `saved`), with the gradient to the embedding: grad_emb [N][input_ch], nullptr skips it
extern "C" int32_t ctx_uvmlp_bwd_emb(const float *grad_raw, int64_t N, const void *packed, int32_t D, int32_t W, int32_t input_ch, int32_t output_ch,
                                     int32_t skip, const void *saved, void *ws, float *const *gws, float *const *gbs, float *grad_emb,
                                     ctx_stream_t stream)
{
    CTX_REQUIRE(grad_raw, "uvmlp_bwd_emb: null grad_raw");
    CTX_REQUIRE(input_ch >= 1 && input_ch <= UVM_EPAD3, "uvmlp_bwd_emb: input_ch=%d outside [1, %d]", input_ch, UVM_EPAD3);
    return uvm_bwd(grad_raw, nullptr, nullptr, 0, nullptr, N, packed, D, W, 3, 0, input_ch, output_ch, skip, saved, ws, gws, gbs, grad_emb, stream);
}
