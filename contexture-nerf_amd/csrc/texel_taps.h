// The bilinear tap of grid_sample(align_corners=False, padding 'border') on a T x T atlas, stated once for every kernel that reads,
// scatters into, marks or bins by it (texmap.hip, uvscatter.hip): they agree on a pixel's texels and weights because this is all
// there is.  Every file that includes this is built with -ffp-contract=off: each product, sum and quotient below rounds on its
// own, in the order written (oracle/geometry_ref.c and tests/test_field_texels_cpu.py state the same arithmetic).
#pragma once
#include "common.h"
#include <math.h>

struct TexelTaps {
    float ix, iy;           // source coordinates after the border clamp (the nearest mode rounds these)
    int x0, y0, x1, y1;     // the 2 x 2 footprint
    float w[4];             // weights of the taps nw (x0,y0), ne (x1,y0), sw (x0,y1), se (x1,y1)
    bool in[4];             // tap k lies inside the atlas
    __device__ __forceinline__ int x(int k) const { return (k & 1) ? x1 : x0; }
    __device__ __forceinline__ int y(int k) const { return (k & 2) ? y1 : y0; }
};

// (u, v) in texture space, v up.  A user of the integers or of ix, iy alone calls this too: the compiler drops what it does not read.
__device__ __forceinline__ TexelTaps texel_taps(float u, float v, int T)
{
    auto src_index = [](float g, int size) {
        float c = ((g + 1.0f) * (float)size - 1.0f) / 2.0f;
        return fminf((float)(size - 1), fmaxf(c, 0.0f));            // fmaxf first: a NaN coordinate clamps to 0
    };
    TexelTaps t;
    t.ix = src_index(u * 2.0f - 1.0f, T);
    t.iy = src_index((1.0f - v) * 2.0f - 1.0f, T);
    t.x0 = (int)floorf(t.ix); t.y0 = (int)floorf(t.iy); t.x1 = t.x0 + 1; t.y1 = t.y0 + 1;
    t.w[0] = ((float)t.x1 - t.ix) * ((float)t.y1 - t.iy);
    t.w[1] = (t.ix - (float)t.x0) * ((float)t.y1 - t.iy);
    t.w[2] = ((float)t.x1 - t.ix) * (t.iy - (float)t.y0);
    t.w[3] = (t.ix - (float)t.x0) * (t.iy - (float)t.y0);
    // The clamp leaves 0 <= ix, iy <= T-1 (T-1 is exact in binary32 for any atlas that fits memory), so 0 <= x0, y0 <= T-1 and
    // 1 <= x1, y1 <= T: of the four bound tests per axis of the general grid_sample only x1 < T and y1 < T can fail.
    const bool bx1 = t.x1 < T, by1 = t.y1 < T;
    t.in[0] = true; t.in[1] = bx1; t.in[2] = by1; t.in[3] = bx1 && by1;
    return t;
}
