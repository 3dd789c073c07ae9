// Engine core shared by the UNet / ControlNet engine (unet.hip) and the VAE engine (vae.hip): the parameter table over one
// fp16 weight blob, the workspace arena (bump allocator with mark/release; sized by a dry run of the same code path), the
// GEMM / conv launch sequence and the fp32 -> fp16 parameter repack.  `struct ctx_unet : Engine`, `struct ctx_vae : Engine`;
// nothing here asks which of the two it serves.
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
};

struct Engine {
    const char *tag = "";      // engine name in error messages
    std::vector<Param> params;
    size_t wtop = 0;           // elements
    // bound memory
    f16 *W = nullptr;
    char *ws = nullptr;
    size_t ws_cap = 0;
    // arena state
    size_t top = 0, peak = 0;
    bool dry = false;
    hipStream_t s = nullptr;
    int rc = 0;

    size_t walloc(size_t n) { size_t o = wtop; wtop += (n + 127) / 128 * 128; return o; }
    size_t add(const std::string &name, std::vector<int64_t> shp, int kind, size_t dst, int a = 0, int b = 0)
    {
        Param p; p.name = name; p.ndim = (int)shp.size(); p.kind = kind; p.dst = dst; p.a = a; p.b = b;
        for (int i = 0; i < 4; ++i) p.shape[i] = i < p.ndim ? shp[i] : 1;
        params.push_back(p);
        return dst;
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
};

// skip launches on a dry run or after an error, keep the first error code
#define ENGINE_RUN(e, expr) do { if (!(e)->dry && (e)->rc == 0) { int r__ = (expr); if (r__ != 0) (e)->rc = r__; } } while (0)

// one GEMM / implicit-GEMM conv of a fully described problem: plan, split-K scratch above the arena mark, dispatch, release
void engine_gemm(Engine &e, GemmArgs &a, bool conv);

// bodies of the ctx_<engine>_param_count / _param_name / _param_shape / _weight_bytes / _bind / _set_param entry points
// (`who` is the entry point's name in error messages)
int32_t engine_param_count(const Engine *e);
const char *engine_param_name(const Engine *e, int32_t i);
int32_t engine_param_shape(const Engine *e, int32_t i, int64_t shape4[4]);
int64_t engine_weight_bytes(const Engine *e);
int32_t engine_bind(Engine *e, void *weights, void *workspace, int64_t workspace_bytes, const char *who);
int32_t engine_set_param(Engine *e, int32_t i, const float *src, ctx_stream_t stream, const char *who);
