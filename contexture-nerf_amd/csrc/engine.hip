// Engine core (engine.h): table accessors, bind, the parameter repack kernels, the linear / conv builders over the GEMM launch
// sequence and the tail of a run.
#include "engine.h"

int32_t engine_param_count(const Engine *e) { return e ? (int32_t)e->params.size() : 0; }
const char *engine_param_name(const Engine *e, int32_t i)
{
    return (e && i >= 0 && i < (int)e->params.size()) ? e->params[i].name.c_str() : "";
}
int32_t engine_param_shape(const Engine *e, int32_t i, int64_t shape4[4])
{
    if (!e || i < 0 || i >= (int)e->params.size()) return 0;
    for (int k = 0; k < 4; ++k) shape4[k] = e->params[i].shape[k];
    return e->params[i].ndim;
}
int64_t engine_weight_bytes(const Engine *e) { return e ? (int64_t)e->wtop * 2 + 256 : 0; }

int32_t engine_bind(Engine *e, void *weights, void *workspace, int64_t workspace_bytes, const char *who)
{
    CTX_REQUIRE(e && weights && workspace && workspace_bytes > 0, "%s: bad args", who);
    CTX_REQUIRE(((uintptr_t)weights & 255) == 0 && ((uintptr_t)workspace & 255) == 0, "%s: blobs must be 256-byte aligned", who);
    e->W = (f16 *)weights; e->ws = (char *)workspace; e->ws_cap = (size_t)workspace_bytes;
    return CTX_OK;
}

int64_t engine_derived_bytes(const Engine *e) { return e && e->dtop ? (int64_t)e->dtop * 2 + 256 : 0; }
int32_t engine_bind_derived(Engine *e, void *derived, int64_t bytes, const char *who)
{
    CTX_REQUIRE(e, "%s: bad args", who);
    if (!derived) { e->D = nullptr; return CTX_OK; }
    CTX_REQUIRE(e->dtop > 0, "%s: this engine derives nothing", who);
    CTX_REQUIRE(bytes >= engine_derived_bytes(e) && ((uintptr_t)derived & 255) == 0, "%s: the derived blob needs %lld bytes, 256-byte aligned", who,
                (long long)engine_derived_bytes(e));
    e->D = (f16 *)derived;
    return CTX_OK;
}

// one GEMM / implicit-GEMM conv of a fully described problem: plan, split-K scratch above the arena mark, dispatch, release
// phase: the phase pack of an upsampling convolution; the op is counted as the nine-tap convolution it stands for and runs the phase form
static void engine_gemm(Engine &e, GemmArgs &a, bool conv, const ConvSegs *segs = nullptr, const GnReq *gn = nullptr, GnSlabs *slabs = nullptr,
                        const f16 *phase = nullptr)
{
    e.note(0, 2.0 * a.M * a.N * a.K);
    size_t mark = e.top;
    if (phase) ctx_conv3_phase(a, phase);
    ctx_gemm_plan(a, conv);                               // a segmented convolution runs the plan of its 3x3 part's shape
    if (segs && segs->n) {
        int kseg = 0;
        a.nseg = segs->n; a.bias2 = segs->bias2;
        for (int i = 0; i < segs->n; ++i) {
            a.segX[i] = segs->x[i]; a.segW[i] = segs->w[i]; a.segC[i] = segs->C[i]; a.segLdw[i] = segs->ldw[i];
            kseg += segs->C[i];
        }
        a.K += kseg;
        e.note(0, 2.0 * a.M * a.N * kseg);
    }
    if (a.zins) a.use8 = 0;        // the zero-inserted grid is an addressing mode of gemm.hip only
    if (a.splitk > 1) a.part = (float *)e.alloc((size_t)a.splitk * a.M * a.N * 4);
    if (gn && gn->part && gn->groups > 0 && a.N % gn->groups == 0) { a.gn_part = gn->part; a.gn_cg = a.N / gn->groups; a.gn_hw = gn->HW; }
    if (slabs) {
        a.keep_slabs = 1;
        *slabs = GnSlabs{a.part, a.splitk, (size_t)a.M * a.N, a.bias, a.bias2, a.rowbias, a.ldrb};
    }
    ENGINE_RUN(&e, ctx_gemm_dispatch(a, conv, e.s));
    if (e.live() && a.gn_part) e.gn_tag = Engine::GnTag{a.out, a.M / a.gn_hw, a.gn_hw, a.N, gn->groups, a.gn_ns};
    if (!slabs) e.top = mark;
}

int engine_conv3_split(int B, int H, int W, int Cin, int Cout)
{
    GemmArgs a = {};
    a.Ho = H; a.Wo = W; a.M = B * H * W; a.N = Cout; a.K = 9 * Cin; a.H = H; a.W = W; a.Cin = Cin; a.stride = 1;
    ctx_gemm_plan(a, true);
    return (a.splitk > 1 && a.splitk <= a.K / 64) ? a.splitk : 1;       // (gemm144.hip clips the factor to K / 64)
}

void engine_linear(Engine &e, const f16 *X, const f16 *Wt, const f16 *bias, const void *res, int M, int N, int K, void *out, int ldc, int epi,
                   bool res32, bool out32, const GnReq *gn)
{
    GemmArgs a = {};
    a.X = X; a.Wt = Wt; a.bias = bias; a.residual = (const f16 *)res; a.out = (f16 *)out;
    a.M = M; a.N = N; a.K = K; a.ldc = ldc ? ldc : epi == 1 ? N / 2 : N; a.ldr = N; a.rows_per_batch = 1; a.ldrb = N; a.epi = epi;
    a.res32 = res32; a.out32 = out32;
    engine_gemm(e, a, false, nullptr, gn);
}

void engine_conv3(Engine &e, const f16 *x, const f16 *Wt, const f16 *bias, const void *res, int B, int H, int W, int Cin, int Cout, void *out,
                  ConvGeom g, const f16 *rowbias, int ldrb, bool res32, bool out32, const ConvSegs *segs, const GnReq *gn, GnSlabs *slabs)
{
    GemmArgs a = {};
    ctx_conv3_problem(a, B, H, W, Cin, Cout, g.stride, g.ups, g.poff, g.zins);
    a.X = x; a.Wt = Wt; a.bias = bias; a.rowbias = rowbias; a.residual = (const f16 *)res; a.out = (f16 *)out;
    a.ldrb = ldrb;
    a.res32 = res32; a.out32 = out32;
    // An upsampler whose phase pack is bound runs the phase form (4 / 9 of the multiplies); it takes a bias only.  Which form runs is
    // a function of the problem and of what is bound, never of a measurement.
    const f16 *phase = nullptr;
    if (g.ups && ctx_conv3_phase_ok(Cin, Cout, g.stride, g.ups, g.poff, g.zins) && !res && !rowbias && !segs && !gn && !slabs && !res32 && !out32 &&
        !ctx_conv3_phase_loses(a.M, Cout, Cin))
        phase = e.phase_pack(Wt);
    engine_gemm(e, a, true, segs, gn, slabs, phase);
}

int engine_finish(Engine *e, const char *who)
{
    if (e->live()) CTX_CHECK_LAUNCH(who);
    return e->rc;
}

// ---- parameter repack kernels ----------------------------------------------------------------------
__global__ void k_pack_copy(const float *__restrict__ s, int64_t n, f16 *__restrict__ d)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) d[i] = (f16)s[i];
}
// [Cout,Cin,3,3] -> [Cout][3][3][Cinp] (Cinp = Cin, or 8 for conv_in)
__global__ void k_pack_conv3(const float *__restrict__ s, int Cout, int Cin, int Cinp, f16 *__restrict__ d)
{
    int64_t n = (int64_t)Cout * 9 * Cinp;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        int c = (int)(i % Cinp);
        int tap = (int)((i / Cinp) % 9);
        int o = (int)(i / ((int64_t)Cinp * 9));
        d[i] = c < Cin ? (f16)s[((int64_t)o * Cin + c) * 9 + tap] : (f16)0.f;
    }
}
// the phase pack of an upsampler's conv3 (GemmArgs::phase): [Cout,Cin,3,3] -> [4 phases (a, b)][Cout][2 u][2 v][Cin], where tap (u, v)
// of phase (a, b) is the sum of the source taps ky in R(a, u), kx in R(b, v), R(0,0) = {0}, R(0,1) = {1,2}, R(1,0) = {0,1}, R(1,1) = {2}:
// fp32, added left to right with ky ascending, then kx ascending, rounded once
__global__ void k_pack_conv3_phase(const float *__restrict__ s, int Cout, int Cin, f16 *__restrict__ d)
{
    const int64_t per = (int64_t)Cout * 4 * Cin, n = 4 * per;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % Cin), t = (int)((i / Cin) % 4), o = (int)((i / ((int64_t)Cin * 4)) % Cout), ph = (int)(i / per);
        const int pa = ph >> 1, pb = ph & 1, u = t >> 1, v = t & 1;
        const int ky0 = pa == 0 ? (u ? 1 : 0) : (u ? 2 : 0), ky1 = pa == 0 ? (u ? 2 : 0) : (u ? 2 : 1);
        const int kx0 = pb == 0 ? (v ? 1 : 0) : (v ? 2 : 0), kx1 = pb == 0 ? (v ? 2 : 0) : (v ? 2 : 1);
        const float *w = s + ((int64_t)o * Cin + c) * 9;
        float acc = 0.f;
        bool first = true;
        for (int ky = ky0; ky <= ky1; ++ky)
            for (int kx = kx0; kx <= kx1; ++kx) {
                const float x = w[ky * 3 + kx];
                acc = first ? x : acc + x;
                first = false;
            }
        d[i] = (f16)acc;
    }
}
// GEGLU rows: packed row p (of 2*C4) <- source row  (w<32 ? blk*32+w : C4 + blk*32 + w-32), blk=p/64, w=p%64
__global__ void k_pack_geglu(const float *__restrict__ s, int C4, int K, f16 *__restrict__ d)
{
    int64_t n = (int64_t)2 * C4 * (K > 0 ? K : 1);
    int kk = K > 0 ? K : 1;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        int k = (int)(i % kk);
        int p = (int)(i / kk);
        int blk = p / 64, w = p % 64;
        int src = w < 32 ? blk * 32 + w : C4 + blk * 32 + (w - 32);
        d[i] = (f16)s[(int64_t)src * kk + k];
    }
}
// backward packs: conv3 [Cout,Cin,3,3] -> [Cin][t' = 3 (2-ky) + (2-kx)][pad] (zero beyond Cout); matrix [out,in] -> [in][ld] at column col
__global__ void k_pack_conv3_T(const float *__restrict__ s, int Cout, int Cin, int pad, f16 *__restrict__ d)
{
    int64_t n = (int64_t)Cin * 9 * pad;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        int o = (int)(i % pad), tp = (int)((i / pad) % 9), c = (int)(i / ((int64_t)pad * 9));
        int ky = 2 - tp / 3, kx = 2 - tp % 3;
        d[i] = o < Cout ? (f16)s[(((int64_t)o * Cin + c) * 3 + ky) * 3 + kx] : (f16)0.f;
    }
}
__global__ void k_pack_mat_T(const float *__restrict__ s, int out, int in, int ld, int col, f16 *__restrict__ d)
{
    int64_t n = (int64_t)out * in;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        int c = (int)(i % in), o = (int)(i / in);
        d[(int64_t)c * ld + col + o] = (f16)s[i];
    }
}

// grid of a repack launch over a parameter of n source elements (grid-stride kernels)
static unsigned pack_blocks(int64_t n)
{
    const int64_t nbk = cdiv64(n, 256);
    return (unsigned)(nbk > 4096 ? 4096 : nbk);
}

// The forward pack of one parameter of n source elements: kind and its dims a, b as the parameter table holds them (PK_CONV3 /
// PK_CONVIN: Cout, Cin; PK_GEGLU_W: C4, K; PK_GEGLU_B: C4).  engine_set_param and the test seam ctx_pack_fwd_f16 launch through here.
int engine_pack_fwd(int kind, const float *src, int64_t n, int a, int b, f16 *d, hipStream_t s, const char *who)
{
    CTX_REQUIRE(src && d && n > 0, "%s: pack: null pointer or empty parameter", who);
    const unsigned nb = pack_blocks(n);
    switch (kind) {
    case PK_COPY: hipLaunchKernelGGL(k_pack_copy, dim3(nb), dim3(256), 0, s, src, n, d); break;
    case PK_CONV3:
        CTX_REQUIRE(a > 0 && b > 0 && n == (int64_t)a * b * 9, "%s: conv3 pack of %lld elements is not [%d,%d,3,3]", who, (long long)n, a, b);
        hipLaunchKernelGGL(k_pack_conv3, dim3(nb), dim3(256), 0, s, src, a, b, b, d); break;
    case PK_CONVIN:
        // rows of 8 or 16 channels: a 17th would land in the next row, and conv_in multiplies at most 16
        CTX_REQUIRE(a > 0 && b >= 1 && b <= 16 && n == (int64_t)a * b * 9, "%s: conv_in pack needs 1 <= Cin <= 16 and [%d,%d,3,3] = %lld elements", who, a, b, (long long)n);
        hipLaunchKernelGGL(k_pack_conv3, dim3(nb), dim3(256), 0, s, src, a, b, b > 8 ? 16 : 8, d); break;
    case PK_GEGLU_W:
        CTX_REQUIRE(a > 0 && a % 32 == 0 && b > 0 && n == (int64_t)2 * a * b, "%s: GEGLU weight pack needs C4 %% 32 == 0 and [2 * %d, %d] = %lld elements", who, a, b, (long long)n);
        hipLaunchKernelGGL(k_pack_geglu, dim3(nb), dim3(256), 0, s, src, a, b, d); break;
    case PK_GEGLU_B:
        CTX_REQUIRE(a > 0 && a % 32 == 0 && n == (int64_t)2 * a, "%s: GEGLU bias pack needs C4 %% 32 == 0 and 2 * %d = %lld elements", who, a, (long long)n);
        hipLaunchKernelGGL(k_pack_geglu, dim3(nb), dim3(256), 0, s, src, a, 0, d); break;
    default: ctx_set_error("%s: unknown pack kind %d", who, kind); return CTX_E_ARG;
    }
    return CTX_OK;
}

int32_t engine_set_param(Engine *e, int32_t i, const float *src, ctx_stream_t stream, const char *who)
{
    CTX_REQUIRE(e && e->W && src && i >= 0 && i < (int)e->params.size(), "%s: bad args / not bound", who);
    const Param &p = e->params[i];
    hipStream_t s = (hipStream_t)stream;
    int64_t n = 1;
    for (int k = 0; k < p.ndim; ++k) n *= p.shape[k];
    f16 *d = e->W + p.dst;
    const unsigned nb = pack_blocks(n);
    const int rc = engine_pack_fwd(p.kind, src, n, p.a, p.b, d, s, who);
    if (rc != CTX_OK) return rc;
    if (p.kind2 == 1) hipLaunchKernelGGL(k_pack_conv3_T, dim3(nb), dim3(256), 0, s, src, p.a, p.b, p.pad2, e->W + p.dst2);
    else if (p.kind2 == 2) hipLaunchKernelGGL(k_pack_mat_T, dim3(nb), dim3(256), 0, s, src, (int)p.shape[0], (int)p.shape[1], p.ld2, p.col2, e->W + p.dst2);
    if (p.kind3 == 1 && e->D) hipLaunchKernelGGL(k_pack_conv3_phase, dim3(pack_blocks(16 * n / 9)), dim3(256), 0, s, src, p.a, p.b, e->D + p.dst3);
    CTX_CHECK_LAUNCH(who);
    return CTX_OK;
}

// ---- test seams: the forward packs and the two backward packs alone, with engine_set_param's launch geometry -----------------------------
extern "C" int32_t ctx_pack_fwd_f16(const float *src, int32_t kind, int32_t a, int32_t b, void *dst, ctx_stream_t stream)
{
    CTX_REQUIRE(kind >= PK_COPY && kind <= PK_GEGLU_B && a > 0 && b >= 0, "pack_fwd: kind %d with a=%d b=%d", kind, a, b);
    const int64_t n = kind == PK_COPY ? (int64_t)a * (b > 0 ? b : 1) : kind == PK_GEGLU_W ? (int64_t)2 * a * b : kind == PK_GEGLU_B ? (int64_t)2 * a
                                                                                                               : (int64_t)a * b * 9;
    const int rc = engine_pack_fwd(kind, src, n, a, b, (f16 *)dst, (hipStream_t)stream, "pack_fwd");
    if (rc != CTX_OK) return rc;
    CTX_CHECK_LAUNCH("pack_fwd");
    return CTX_OK;
}
// the phase pack alone (k_pack_conv3_phase), with engine_set_param's launch geometry; dst holds 16 Cout Cin f16
extern "C" int32_t ctx_pack_conv3_phase_f16(const float *src, int32_t Cout, int32_t Cin, void *dst, ctx_stream_t stream)
{
    CTX_REQUIRE(src && dst, "pack_conv3_phase: null pointer");
    CTX_REQUIRE(Cout > 0 && Cin > 0 && (int64_t)16 * Cout * Cin < (1ll << 31), "pack_conv3_phase: need Cout, Cin > 0 and 16 Cout Cin < 2^31 (Cout=%d Cin=%d)", Cout, Cin);
    hipLaunchKernelGGL(k_pack_conv3_phase, dim3(pack_blocks((int64_t)16 * Cout * Cin)), dim3(256), 0, (hipStream_t)stream, src, Cout, Cin, (f16 *)dst);
    CTX_CHECK_LAUNCH("pack_conv3_phase");
    return CTX_OK;
}
extern "C" int32_t ctx_pack_conv3_dgrad_f16(const float *src, int32_t Cout, int32_t Cin, int32_t pad, void *dst, ctx_stream_t stream)
{
    CTX_REQUIRE(src && dst, "pack_conv3_dgrad: null pointer");
    CTX_REQUIRE(Cout > 0 && Cin > 0 && pad >= Cout && (int64_t)Cin * 9 * pad < (1ll << 31), "pack_conv3_dgrad: need 0 < Cout <= pad (Cout=%d Cin=%d pad=%d)", Cout, Cin, pad);
    hipLaunchKernelGGL(k_pack_conv3_T, dim3(pack_blocks((int64_t)Cout * Cin * 9)), dim3(256), 0, (hipStream_t)stream, src, Cout, Cin, pad, (f16 *)dst);
    CTX_CHECK_LAUNCH("pack_conv3_dgrad");
    return CTX_OK;
}
extern "C" int32_t ctx_pack_mat_dgrad_f16(const float *src, int32_t out, int32_t in, int32_t ld, int32_t col, void *dst, ctx_stream_t stream)
{
    CTX_REQUIRE(src && dst, "pack_mat_dgrad: null pointer");
    CTX_REQUIRE(out > 0 && in > 0 && col >= 0 && (int64_t)col + out <= ld && (int64_t)in * ld < (1ll << 31),
                "pack_mat_dgrad: columns col .. col + out must lie inside ld (out=%d in=%d ld=%d col=%d)", out, in, ld, col);
    hipLaunchKernelGGL(k_pack_mat_T, dim3(pack_blocks((int64_t)out * in)), dim3(256), 0, (hipStream_t)stream, src, out, in, ld, col, (f16 *)dst);
    CTX_CHECK_LAUNCH("pack_mat_dgrad");
    return CTX_OK;
}
