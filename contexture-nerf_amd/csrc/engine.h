// Engine core shared by the UNet / ControlNet engine (unet.hip) and the VAE engine (vae.hip): the parameter table over one
// fp16 weight blob, the workspace arena (bump allocator with mark/release; sized by a dry run of the same code path), the
// fp32 -> fp16 parameter repack, and the op layer the two graphs are written in: guarded launches and copies, the linear /
// 3x3-conv builders over the GEMM launch sequence, FLOP / launch accounting, the dry run behind every size query and the
// error tail.  `struct ctx_unet : Engine`, `struct ctx_vae : Engine`; nothing here asks which of the two it serves.
//
// A run keeps its first error (a workspace overflow in alloc(), a kernel entry's refusal) in `rc`, and from then on launches and
// copies nothing: a graph launches and copies only through ENGINE_RUN / ENGINE_LAUNCH / copy() / copy2d(), which do nothing on a
// dry run or once rc != 0.  (After an overflow alloc() hands out the workspace base: a pointer that must never reach a kernel.)
#pragma once
#include "common.h"
#include "kernels.h"
#include <string>
#include <vector>

enum PackKind { PK_COPY = 0, PK_CONV3 = 1, PK_CONVIN = 2, PK_GEGLU_W = 3, PK_GEGLU_B = 4 };

struct Param {
    std::string name;
    int ndim;
    int64_t shape[4];
    int kind;
    size_t dst;      // element offset into the fp16 weight blob
    int a, b;        // kind-specific dims
    // second pack for the VAE encoder's backward (input gradients): kind2 1 = conv3 [Cout,Cin,3,3] -> [Cin][2-ky][2-kx][pad2 >= Cout]
    // (the data-gradient of a 3x3 convolution is a 3x3 convolution with this matrix), 2 = [out,in] -> [in][ld2] at column col2
    int kind2 = 0; size_t dst2 = 0; int pad2 = 0, ld2 = 0, col2 = 0;
    // pack derived from the parameter, in the derived blob (Engine::D): kind3 1 = the phase pack of an upsampler's conv3
    // [Cout,Cin,3,3] -> [4][Cout][2][2][Cin] (GemmArgs::phase), 16 Cout Cin elements at dst3
    int kind3 = 0; size_t dst3 = 0;
};

struct Engine {
    const char *tag = "";      // engine name in error messages
    std::vector<Param> params;
    size_t wtop = 0;           // elements
    // The derived blob: packs that are functions of parameters but have no place in the weight blob, whose size is part of the ABI.
    // Optional: an engine with none bound (D null) runs every layer from the weight blob alone.  dtop: elements.
    size_t dtop = 0;
    f16 *D = nullptr;
    // bound memory
    f16 *W = nullptr;
    char *ws = nullptr;
    size_t ws_cap = 0;
    // arena state
    size_t top = 0, peak = 0;
    bool dry = false;
    hipStream_t s = nullptr;
    int rc = 0;
    // accounting of the current run by kernel class: 0 GEMM / conv, 1 attention, 2 everything else (a dry run counts the same)
    int64_t launches[3] = {0, 0, 0};
    double flops[3] = {0, 0, 0};

    // GroupNorm partials that a producer's epilogue has written (engine_linear / engine_conv3 with a GnReq): the tensor they belong to
    // and its GroupNorm shape.  A graph's GroupNorm op takes them only for exactly this tensor and shape, and every GroupNorm op
    // clears the tag, so partials never outlive the next GroupNorm.  Counters of the current run: GroupNorms that ran on a
    // producer's partials / that read split-K slabs in place of a reduced tensor.
    struct GnTag { const void *x = nullptr; int B = 0, HW = 0, C = 0, groups = 0, NS = 0; } gn_tag;
    int64_t gn_from_producer = 0, gn_from_slabs = 0;

    size_t walloc(size_t n) { size_t o = wtop; wtop += (n + 127) / 128 * 128; return o; }
    size_t add(const std::string &name, std::vector<int64_t> shp, int kind, size_t dst, int a = 0, int b = 0)
    {
        Param p; p.name = name; p.ndim = (int)shp.size(); p.kind = kind; p.dst = dst; p.a = a; p.b = b;
        for (int i = 0; i < 4; ++i) p.shape[i] = i < p.ndim ? shp[i] : 1;
        params.push_back(p);
        return dst;
    }
    // the parameter added last is an upsampler's conv3 [Cout,Cin,3,3]: reserve its phase pack in the derived blob (where the form exists)
    void derive_phase()
    {
        Param &p = params.back();
        if (!ctx_conv3_phase_ok(p.b, p.a, 1, 1, 0, 0)) return;
        p.kind3 = 1; p.dst3 = dtop; dtop += ((size_t)16 * p.a * p.b + 127) / 128 * 128;
    }
    // the phase pack of the conv3 weights at Wt, or null: none bound, or the layer has none
    const f16 *phase_pack(const f16 *Wt) const
    {
        if (!D || !W) return nullptr;
        for (const Param &p : params)
            if (p.kind3 == 1 && W + p.dst == Wt) return D + p.dst3;
        return nullptr;
    }
    size_t vec(const std::string &name, int n) { return add(name, {n}, PK_COPY, walloc(n)); }
    size_t lin(const std::string &name, int out, int in) { return add(name, {out, in}, PK_COPY, walloc((size_t)out * in)); }

    void *alloc(size_t bytes)
    {
        size_t o = (top + 255) / 256 * 256;
        top = o + bytes;
        if (top > peak) peak = top;
        if (!dry && top > ws_cap) { rc = CTX_E_STATE; ctx_set_error("%s: workspace too small (%zu > %zu)", tag, top, ws_cap); return ws; }
        return dry ? nullptr : (void *)(ws + o);
    }
    f16 *allocH(size_t n) { return (f16 *)alloc(n * 2); }

    void begin()                                               // a run from an empty arena
    {
        top = 0; peak = 0; rc = 0; gn_tag = GnTag(); gn_from_producer = 0; gn_from_slabs = 0;
        for (int k = 0; k < 3; ++k) { launches[k] = 0; flops[k] = 0; }
    }
    void note(int klass, double fl, int n = 1) { launches[klass] += n; flops[klass] += fl; }
    bool live() const { return !dry && rc == 0; }
    // device-to-device copies on the run's stream
    void copy(void *dst, const void *src, size_t bytes) { if (live()) (void)hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s); }
    void copy2d(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t rows)
    { if (live()) (void)hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, hipMemcpyDeviceToDevice, s); }
};

// a kernel entry that returns a code / a bare kernel on the run's stream: skipped on a dry run or after an error; the first error code is kept
#define ENGINE_RUN(e, expr) do { if ((e)->live()) { int r__ = (expr); if (r__ != 0) (e)->rc = r__; } } while (0)
#define ENGINE_LAUNCH(e, kernel, grid, block, lds, ...) do { if ((e)->live()) hipLaunchKernelGGL(kernel, grid, block, lds, (e)->s, __VA_ARGS__); } while (0)

// A request that the producer of `out` also write the GroupNorm partials of a following GroupNorm(groups) over samples of HW rows, into
// `part` (ctx_groupnorm_ws_bytes).  Honoured (a live run only): e.gn_tag names `out`; declined: the tag stays empty and the GroupNorm
// op computes its statistics itself.
struct GnReq { float *part = nullptr; int groups = 0, HW = 0; };
// out[M, ldc] = X[M,K] Wt[N,K]^T (+ bias[N]) (+ res[M,N]); ldc 0 = dense; epi 1 = GEGLU (out has N/2 columns); res32 / out32: res / out are fp32
void engine_linear(Engine &e, const f16 *X, const f16 *Wt, const f16 *bias, const void *res, int M, int N, int K, void *out, int ldc = 0,
                   int epi = 0, bool res32 = false, bool out32 = false, const GnReq *gn = nullptr);
// a 3x3 convolution's geometry beyond "stride 1, padding 1" (GemmArgs has each meaning); Ho = ((H << ups) - 1) / stride + 1, Wo alike
struct ConvGeom { int stride = 1, ups = 0, poff = 0, zins = 0; };
// K segments of a convolution (GemmArgs::nseg): n 1x1 products over tensors x[s] [B,H,W,C[s]] of the output's pixel grid, weights
// w[s] [Cout] rows of C[s] at row stride ldw[s], and their bias; folded into the convolution's K loop (default geometry only)
struct ConvSegs { int n = 0; const f16 *x[2] = {nullptr, nullptr}; const f16 *w[2] = {nullptr, nullptr}; int C[2] = {0, 0}, ldw[2] = {0, 0}; const f16 *bias2 = nullptr; };
// out[B,Ho,Wo,Cout] = conv3x3(x[B,H,W,Cin]; Wt[Cout][3][3][Cin]) (+ bias[Cout]) (+ rowbias[b * ldrb ..]) (+ res) (+ segments); NHWC.
// The segments' product is counted as a class-0 op of its own (the 1x1 convolution it stands for).
void engine_conv3(Engine &e, const f16 *x, const f16 *Wt, const f16 *bias, const void *res, int B, int H, int W, int Cin, int Cout, void *out,
                  ConvGeom g = ConvGeom(), const f16 *rowbias = nullptr, int ldrb = 0, bool res32 = false, bool out32 = false,
                  const ConvSegs *segs = nullptr, const GnReq *gn = nullptr, GnSlabs *slabs = nullptr);
// Split-K factor that engine_conv3 will run this stride-1 convolution with when asked to keep its slabs (1: it does not split).
// slabs != null in engine_conv3: the reduce launch is skipped, `out` is not written (pass null) and *slabs describes the fp32 slabs,
// which stay allocated above the caller's arena mark; only where this function returns > 1.
int engine_conv3_split(int B, int H, int W, int Cin, int Cout);

// `run` as a dry run: nothing is launched, the arena only measures (e.peak), the counters count; -> the run's return code
template <class F> int engine_dry_run(Engine *e, F run)
{
    const bool was = e->dry;
    e->dry = true; const int rc = run(); e->dry = was;
    return rc;
}
inline int64_t engine_workspace_need(const Engine *e) { return (int64_t)e->peak + 4096; }
// tail of a run: a launch error of the runtime, else the run's first error (`who` is the entry point's name in the message)
int engine_finish(Engine *e, const char *who);

// bodies of the ctx_<engine>_param_count / _param_name / _param_shape / _weight_bytes / _bind / _set_param entry points
// (`who` is the entry point's name in error messages)
int32_t engine_param_count(const Engine *e);
const char *engine_param_name(const Engine *e, int32_t i);
int32_t engine_param_shape(const Engine *e, int32_t i, int64_t shape4[4]);
int64_t engine_weight_bytes(const Engine *e);
int32_t engine_bind(Engine *e, void *weights, void *workspace, int64_t workspace_bytes, const char *who);
int32_t engine_set_param(Engine *e, int32_t i, const float *src, ctx_stream_t stream, const char *who);
// bodies of ctx_<engine>_derived_bytes / _bind_derived: the derived blob's size (0: the engine derives nothing) and its binding (null unbinds).
// Parameters set while it is bound fill it; bind it before loading weights, or share a filled one between engines over the same weights.
int64_t engine_derived_bytes(const Engine *e);
int32_t engine_bind_derived(Engine *e, void *derived, int64_t bytes, const char *who);
// the forward pack of one parameter alone (kind: PackKind; a, b: its dims in the table; n source elements); no launch check of its own
int engine_pack_fwd(int kind, const float *src, int64_t n, int a, int b, f16 *d, hipStream_t s, const char *who);
