// Scans and single-lane moves across the 64 lanes of a wavefront on the DPP path (no LDS crossbar), for the wave-per-ray kernels
// (composite.hip, distortion.hip, resample.hip).  The order of the steps inside a scan is part of every result built on it:
// tests/resample_rule.py restates it lane by lane.
#pragma once
#include "common.h"

// v moved across the lanes by the DPP control CTRL, into the 16-lane rows of the mask ROWS; a lane without a source, or in a row outside
// the mask, gets `old`
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ float wave_dpp(float old, float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v), CTRL, ROWS, 0xf, false));
}

__device__ __forceinline__ float wave_shr1(float v, float fill) { return wave_dpp<0x138>(fill, v); }          // lane i <- lane i - 1; lane 0 <- fill
__device__ __forceinline__ float wave_shl1(float v, float fill) { return wave_dpp<0x130>(fill, v); }          // lane i <- lane i + 1; lane 63 <- fill
__device__ __forceinline__ float wave_lane(float v, int k)                                                    // v of lane k (k wave-uniform)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), k));
}

// The operations of wave_scan: a lane without a source combines with the identity.
struct scan_prod {
    static constexpr float identity = 1.0f;
    static __device__ __forceinline__ float op(float a, float b) { return a * b; }
};
struct scan_sum {
    static constexpr float identity = 0.f;
    static __device__ __forceinline__ float op(float a, float b) { return a + b; }
};
struct scan_max {                                 // of values >= 0
    static constexpr float identity = 0.f;
    static __device__ __forceinline__ float op(float a, float b) { return fmaxf(a, b); }
};

// Inclusive scan over the 64 lanes: Hillis-Steele inside the 16-lane rows (row_shr 1, 2, 4, 8), then row_bcast 15 into rows 1 and 3 and
// row_bcast 31 into rows 2 and 3.  Lane i combines its row left to right in a 4-level tree, then the rows.
template <class Op>
__device__ __forceinline__ float wave_scan(float v)
{
    v = Op::op(v, wave_dpp<0x111>(Op::identity, v));
    v = Op::op(v, wave_dpp<0x112>(Op::identity, v));
    v = Op::op(v, wave_dpp<0x114>(Op::identity, v));
    v = Op::op(v, wave_dpp<0x118>(Op::identity, v));
    v = Op::op(v, wave_dpp<0x142, 0xa>(Op::identity, v));
    v = Op::op(v, wave_dpp<0x143, 0xc>(Op::identity, v));
    return v;
}

// Inclusive suffix sum (lane i: the sum over the lanes at and behind it): row_shl 1, 2, 4, 8 inside the rows, then the totals of the rows
// behind a row (lanes 16, 32, 48) by lane reads.  A true suffix scan, not total - prefix: a small term behind a large one keeps its bits.
__device__ __forceinline__ float wave_suffix_sum(float v, int lane)
{
    v = v + wave_dpp<0x101>(0.f, v);
    v = v + wave_dpp<0x102>(0.f, v);
    v = v + wave_dpp<0x104>(0.f, v);
    v = v + wave_dpp<0x108>(0.f, v);
    const float r1 = wave_lane(v, 16), r2 = wave_lane(v, 32), r3 = wave_lane(v, 48);
    const int row = lane >> 4;
    return v + (row == 0 ? (r1 + (r2 + r3)) : row == 1 ? (r2 + r3) : row == 2 ? r3 : 0.f);
}
