// The two ordered compactions of the library, both instances of compact.h: create_face_view_map (src/training/trainer.py:155-249:
// the covered pixels of a raster as rows (face, view, y, x), in pixel order) and the active-texel list.  Integer work, held to
// equality with oracle/geometry_ref.c and tests/test_field_texels_cpu.py element for element.
#include "compact.h"

// create_face_view_map: a pixel is kept when a face covers it
struct FaceCovers { __device__ bool operator()(int64_t f) const { return f >= 0; } };
struct FaceViewRow {
    int64_t HW; int W; int64_t *rows;
    __device__ void operator()(int64_t i, int64_t f, int64_t r) const
    {
        int64_t view = i / HW, pix = i % HW;
        int64_t *o = rows + r * 4;
        o[0] = f; o[1] = view; o[2] = pix / W; o[3] = pix % W;
    }
};

extern "C" int64_t ctx_face_view_map_ws_bytes(int32_t B, int32_t H, int32_t W) { return compact_ws((int64_t)B * H * W).bytes; }

extern "C" int32_t ctx_face_view_map(const int64_t *face_idx, int32_t B, int32_t H, int32_t W, int64_t *rows,
                                     int64_t *n_rows, void *ws, ctx_stream_t stream)
{
    CTX_REQUIRE(face_idx && rows && n_rows && ws && B > 0 && H > 0 && W > 0, "face_view_map: bad args");
    return compact_run("face_view_map", face_idx, (int64_t)B * H * W, FaceCovers{}, FaceViewRow{(int64_t)H * W, W, rows}, n_rows, ws,
                       (hipStream_t)stream);
}

// The same compaction of a byte mask (ctx_texel_active_mark's): idx_out[0:count] = the flat indices of its non-zero bytes, ascending.
struct ByteSet { __device__ bool operator()(uint8_t b) const { return b != 0; } };
struct TexelIndex { int32_t *idx_out; __device__ void operator()(int64_t i, uint8_t, int64_t r) const { idx_out[r] = (int32_t)i; } };

extern "C" int64_t ctx_texel_compact_ws_bytes(int64_t n)
{
    if (n < 1 || n > INT32_MAX) return -1;       // the indices are int32; one block per CMP_BLK bytes stays far inside one grid
    return compact_ws(n).bytes;
}

extern "C" int32_t ctx_texel_compact(const uint8_t *mask, int64_t n, int32_t *idx_out, int64_t *count_out, void *ws, ctx_stream_t stream)
{
    CTX_REQUIRE(mask && idx_out && count_out && ws, "texel_compact: null pointer");
    CTX_REQUIRE(n >= 1 && n <= INT32_MAX, "texel_compact: n=%lld outside [1, 2^31)", (long long)n);
    return compact_run("texel_compact", mask, n, ByteSet{}, TexelIndex{idx_out}, count_out, ws, (hipStream_t)stream);
}
