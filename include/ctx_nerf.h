/*
 * ctx_nerf.h — C-ABI of libctxnerf.so: the MI355X (gfx950) hot path of ConTEXTure's per-view
 * texture-painting loop.
 *
 * The reference (zaiisao/ConTEXTure-NeRF) has no FFI of its own: its hot ops live in third-party
 * Python packages (kaolin, torch-scatter, diffusers).  Each entry point below replaces the
 * third-party call the reference makes at the cited file:line; the Python shims in
 * contexture-nerf_amd/ keep those call signatures (INTEGRATION.md shows the ctypes binding).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous row-major memory owned by the caller
 *     (PyTorch allocates; the library never frees or retains it beyond the call, except the
 *     weight/workspace blobs explicitly bound to a ctx_unet_t);
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing syncs;
 *   - return 0 = OK, negative = error (CTX_E_*); ctx_last_error() gives a thread-local message;
 *   - int64 face indices follow the reference's dtype (kaolin returns int64, -1 = background).
 */
#ifndef CTX_NERF_H
#define CTX_NERF_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CTX_OK 0
#define CTX_E_ARG (-1)      /* bad shape / null pointer / unsupported size */
#define CTX_E_LAUNCH (-2)   /* hipGetLastError() after launch */
#define CTX_E_STATE (-3)    /* handle not bound / wrong phase */

typedef void *ctx_stream_t;

int32_t ctx_version(void);
const char *ctx_last_error(void);
/* Device check used by the Python loader: 0 when a gfx950 device is current. */
int32_t ctx_device_check(void);

/* ---- raster path ------------------------------------------------------------------------- */
/* kal.render.mesh.prepare_vertices  (src/models/render.py:112-113; textured_mesh.py:167-168)
   verts[B,V,3] faces[F,3] cam[B,4,3] proj3[3] -> fv_cam[B,F,3,3] fv_img[B,F,3,2] fnorm[B,F,3] */
int32_t ctx_prepare_vertices(const float *verts, const int64_t *faces, const float *cam,
                             const float *proj3, int32_t B, int32_t V, int32_t F,
                             float *fv_cam, float *fv_img, float *fnorm,
                             void *ws /* B*V*5 floats */, ctx_stream_t stream);

/* Scratch for the per-coarse-tile face lists of the two rasterise entry points. */
int64_t ctx_rasterize_ws_bytes(int32_t H, int32_t W, int32_t B, int32_t F);
/* kal.render.mesh.rasterize  (src/models/render.py:115-120; textured_mesh.py:170-175)
   face_z[B,F,3] face_xy[B,F,3,2] feat[B,F,3,C] -> out[B,H,W,C] face_idx[B,H,W]  (C <= 64) */
int32_t ctx_rasterize_fwd(int32_t H, int32_t W, const float *face_z, const float *face_xy,
                          const float *feat, int32_t B, int32_t F, int32_t C,
                          float multiplier, float eps, float *out, int64_t *face_idx,
                          void *ws, int64_t ws_bytes, ctx_stream_t stream);

/* The reference rasterises twice per render (depth pass, then UV pass: render.py:115 and :119).
   Fused single pass: depth[B,H,W] (feature = z), uv[B,H,W,2], face_idx[B,H,W], and optionally the
   gathered face normals normals[B,H,W,3] (render.py:150-157; background reads the LAST face).
   fv_cam[B,F,3,3] supplies z (= fv_cam[...,2]); uv_attr[Bu,F,3,2] with Bu in {1,B}. */
int32_t ctx_rasterize_fused(int32_t H, int32_t W, const float *fv_cam, const float *face_xy,
                            const float *uv_attr, int32_t Bu, const float *fnorm /*nullable*/,
                            int32_t B, int32_t F, float multiplier, float eps,
                            float *depth, float *uv, int64_t *face_idx, float *normals /*nullable*/,
                            void *ws, int64_t ws_bytes, ctx_stream_t stream);

/* Renderer.normalize_multiple_depth (src/models/render.py:48-74).  ws: ctx_normalize_depth_ws_bytes(B).
   status[0] (device int32, nullable): 0 ok, 1 positive depth present, 2 all-zero (the reference's
   two asserts, render.py:49-50). */
int64_t ctx_normalize_depth_ws_bytes(int32_t B);
int32_t ctx_normalize_depth(const float *depth, int32_t B, int32_t HW, float *out,
                            void *ws, int32_t *status, ctx_stream_t stream);

/* kal.render.mesh.texture_mapping (src/models/render.py:135) == grid_sample(align_corners=False,
   padding 'border'); tex[Bt,C,T,T] with Bt in {1,B}; mode 0 bilinear, 1 nearest; out[B,HW,C].
   mask_idx (nullable, int64[B,HW]): when given, out *= (face_idx > -1)   (render.py:133,141). */
int32_t ctx_texture_mapping_fwd(const float *uv, const float *tex, int32_t B, int32_t HW,
                                int32_t C, int32_t T, int32_t Bt, int32_t mode,
                                const int64_t *mask_idx, float *out, ctx_stream_t stream);
/* autograd of the above w.r.t. the (expanded) atlas: grad_tex[C,T,T] += ...  (caller zeroes). */
int32_t ctx_texture_mapping_bwd(const float *grad_out, const float *uv, int32_t B, int32_t HW,
                                int32_t C, int32_t T, const int64_t *mask_idx, float *grad_tex,
                                ctx_stream_t stream);
/* The same scatter without global float atomics (uvscatter.hip): pixels are binned by 32 x 32-texel atlas tile once per raster
   (`plan`: depends on uv / mask_idx only, reusable by every backward of the SDS loop), then one workgroup per tile accumulates
   its pixel list in LDS as fixed-point int64 sums and writes each texel once.  Bit-reproducible (integer sums do not depend
   on arrival order); C <= 4, B*HW < 2^32, T <= ctx_texmap_plan_max_res().  grad_tex [C,T,T] is added to (as above).
   The fixed-point unit is chosen per call from max|grad_out| (2^-E of the largest tap, E = 62 - ceil(log2(B*HW))), so gradients of
   any magnitude keep the same relative resolution; a non-finite grad_out, or a (uv, mask_idx) that no longer matches the plan's
   sampled checksum, turns the whole of grad_tex into NaN (and ctx_texmap_plan_stale() reports the latter).
   ws: ctx_texture_mapping_bwd_binned_ws_bytes. */
int64_t ctx_texmap_bwd_plan_bytes(int32_t B, int32_t HW, int32_t T);
int32_t ctx_texmap_plan_max_res(void);
int32_t ctx_texmap_bwd_plan(const float *uv, const int64_t *mask_idx, int32_t B, int32_t HW, int32_t T, void *plan, ctx_stream_t stream);
int32_t ctx_texmap_plan_stale(const void *plan, ctx_stream_t stream);
int64_t ctx_texture_mapping_bwd_binned_ws_bytes(int32_t C, int32_t T);
int32_t ctx_texture_mapping_bwd_binned(const float *grad_out, const float *uv, const int64_t *mask_idx, int32_t B, int32_t HW, int32_t C, int32_t T,
                                       const void *plan, void *ws, float *grad_tex, ctx_stream_t stream);

/* UV back-projection of painted views (north_star "torch-scatter UV back-projection"; call contract src/training/trainer.py:1076-1090)
   as INTEGER sums: acc [C,T,T] int64 += round(values * bilinear weight * 2^frac_bits) at the 4 texels of every unmasked pixel.
   The caller owns acc across calls and ranks: view shards are all-reduced (SUM, int64) and converted once by ctx_fixed_to_float,
   so the N-rank atlas equals the 1-rank atlas bit for bit.  Requires |values| * B*HW * 2^frac_bits < 2^63.
   plan: as above, or NULL (any T, any C: one global int64 atomic per tap). */
int32_t ctx_uv_scatter_fixed(const float *values, const float *uv, const int64_t *mask_idx, int32_t B, int32_t HW, int32_t C, int32_t T,
                             const void *plan, int32_t frac_bits, int64_t *acc, ctx_stream_t stream);
int32_t ctx_fixed_to_float(const int64_t *acc, int64_t n, int32_t frac_bits, int32_t accumulate, float *out, ctx_stream_t stream);

/* The same back-projection as a texel-side GATHER (uvgather.hip): every chart texel looks its own surface point up in every view,
   so a magnified surface leaves no pinholes and nothing is written outside a chart.  No atomics, no plan.
   texel_face [T,T] i64 (-1 = no chart) and texel_bary [T,T,3] f32: the UV triangles drawn at T x T with the identity as face
   features.  faces [F,3] i64, face_vertices_image [B,F,3,2] f32, face_idx [B,H,W] i64 (-1 = background), values [B,H,W,C] f32
   (NHWC, colour only), weight [B,H,W] f32 or NULL (= 1), acc [C+1,T,T] int64 in units of 2^-frac_bits, 1 <= C <= 4.
   For texel p with f = texel_face[p] >= 0, barycentrics (b0,b1,b2) and view v, in binary32 in the order written:
     f must own a pixel of face_idx[v];  X = (b0*x0 + b1*x1) + b2*x2, Y likewise, from face_vertices_image[v,f];
     px = ((X + 1)*W - 1)/2, py = ((1 - Y)*H - 1)/2;  xn = floor(px + 0.5), yn = floor(py + 0.5), inside the image;
     g = face_idx[v,yn,xn] must be related to f (equal, or sharing a vertex id in faces);
     colour_c = (sum w_k * values[v,tap_k,c]) / (sum w_k) over the bilinear taps at (floor(px), floor(py)) + {0,1}^2 (weights
     and order of ctx_texture_mapping_fwd: nw, ne, sw, se) that are inside the image and whose owner is related to f;
     omega = weight[v,yn,xn]; omega == 0 or a non-finite omega or colour: no contribution;
     acc[c,p] += rint(colour_c * omega * 2^frac_bits), acc[C,p] += rint(omega * 2^frac_bits)   (the conversion of the scatter).
   One thread owns a texel: integer sums, one plain read-modify-write, independent of grid, order and stream; texels outside
   every chart are never written.  ws: ctx_uv_gather_ws_bytes(B, F) bytes (the [B,F] map of faces that own a pixel). */
int64_t ctx_uv_gather_ws_bytes(int32_t B, int32_t F);
int32_t ctx_uv_gather_fixed(const float *values, const float *weight, const int64_t *face_idx, const float *face_vertices_image,
                            const int64_t *faces, const int64_t *texel_face, const float *texel_bary, int32_t B, int32_t H, int32_t W,
                            int32_t C, int32_t F, int32_t T, int32_t frac_bits, int64_t *acc, void *ws, int64_t ws_bytes, ctx_stream_t stream);

/* Atlas completion (atlasfill.hip): the step after the scatter above. The scatter is a forward one, so texels no screen pixel
   reaches stay empty; the call site it completes is src/training/trainer.py:1076-1090 (project_back, which has no body upstream).
   Colours are copied, never computed, so the result is defined by an integer source map:
     nearest seed of texel (y, x) = the seed (sy, sx) minimising (d2, sy, sx) lexicographically, d2 = (y-sy)^2 + (x-sx)^2 (exact).
   ctx_nearest_seed: seed [T,T] u8 (non-zero = seed) -> src [T,T] int32 = sy*T + sx and d2 [T,T] int32; a seed maps to itself with
   d2 = 0; with no seed at all src = d2 = -1 everywhere.
   ctx_atlas_fill: atlas [C,T,T] f32, coverage [T,T] f32, chart [T,T] u8, pad >= 0 -> filled [C,T,T] f32, src [T,T] int32 (outputs and ws must not overlap
   the inputs or each other).
     stage A  seeds = coverage > 0: every texel with chart & ~seed takes the colour of its nearest seed (no distance limit);
     stage B  seeds = chart | coverage > 0: every other texel whose nearest stage-B seed has d2 <= pad*pad takes that seed's
              stage-A colour (pad = 0 skips it).
   src[p] = flat index of the COVERED texel whose colour p ends up with (p itself when covered), -1 = untouched, so
   filled[c][p] == atlas[c][src[p]] bit for bit where src[p] >= 0 and filled[c][p] == atlas[c][p] elsewhere.  Nothing covered:
   filled == atlas, src == -1.  1 <= T <= 4096 (d2 < 2^25).  ws: ctx_atlas_fill_ws_bytes(T) bytes, for either entry. */
int64_t ctx_atlas_fill_ws_bytes(int32_t T);
int32_t ctx_nearest_seed(const uint8_t *seed, int32_t T, int32_t *src, int32_t *d2, void *ws, int64_t ws_bytes, ctx_stream_t stream);
int32_t ctx_atlas_fill(const float *atlas, const float *coverage, const uint8_t *chart, int32_t C, int32_t T, int32_t pad, float *filled, int32_t *src,
                       void *ws, int64_t ws_bytes, ctx_stream_t stream);

/* ---- mask operators and the atlas update of the progressive paint loop (maskops.hip; guide.paint_mode = 'progressive') ----
   TEXTure (Richardson et al. 2023, sections 3.2-3.3) builds its generate / refine / keep trimap and its projection weight from mask
   morphology and a Gaussian blur done on the host; these are the same operators on the device.  Images are f32 [N,H,W], N*H*W < 2^31.
   Every entry refuses bad arguments BEFORE any launch and leaves its outputs untouched then; one writer per element, no atomics,
   no host sync.  src, dst and ws (N*H*W floats) are pairwise distinct.
   ctx_mask_morph: dst[n,y,x] = max (op 0, dilate) or min (op 1, erode) of src[n,y',x'] over |y'-y| <= k/2, |x'-x| <= k/2 INSIDE the
     image: pixels outside take no part (OpenCV's default border of both operators).  k odd in [1, 63], and it may exceed H or W;
     values are any finite floats (soft masks too).  Separable: the row pass writes ws, the column pass dst.
   ctx_sep_filter: taps = HOST array of k floats, k odd in [1, 63], k/2 <= min(H, W) - 1.  r = k/2, R(i, n) = -i for i < 0,
     2(n-1) - i for i >= n, i otherwise (reflection that does not repeat the edge: index -1 reads 1):
       ws[n,y,x]  = sum_j taps[j] * src[n, y, R(x - r + j, W)],   dst[n,y,x] = sum_j taps[j] * ws[n, R(y - r + j, H), x],
     each sum in binary32 from j = 0 upwards: s = taps[0]*v_0, then s = s + taps[j]*v_j (product and sum round on their own). */
int32_t ctx_mask_morph(const float *src, int32_t N, int32_t H, int32_t W, int32_t k, int32_t op, float *dst, float *ws, ctx_stream_t stream);
int32_t ctx_sep_filter(const float *src, int32_t N, int32_t H, int32_t W, const float *taps, int32_t k, float *dst, float *ws, ctx_stream_t stream);
/* ctx_atlas_blend: the progressive replacement for plain summation of view contributions, in the atlas's own 2^-32 currency.
   contrib [4,T,T] i64 (one view's colour * weight sums and its weight sum, as ctx_uv_scatter_fixed / ctx_uv_gather_fixed leave them),
   zsum [T,T] i64 (the same view's z-normal * weight sum), acc [4,T,T] i64 (the running atlas), meta [T,T] f32 (the z-normal each
   texel was painted at).  F(v) = (float)ldexp((double)v, -32) (ctx_fixed_to_float's conversion).  Per texel, in binary32 in the order written:
     w = contrib[3];  w <= 0: nothing changes.  wf = F(w), m = min(1, wf), new_c = F(contrib[c]) / wf, z = F(zsum) / wf;
     acc[3] <= 0 (never painted): out_c = new_c, meta = z;
     else old_c = F(acc[c]) / F(acc[3]):  out_c = old_c*(1 - m) + new_c*m,  meta = meta*(1 - m) + z*m;
     acc[c] = rint(out_c * 2^32) (the conversion of the scatter), acc[3] = 2^32.
   acc stays a sum image, so ctx_fixed_to_float and everything after the atlas merge apply unchanged.  1 <= T <= 16384. */
int32_t ctx_atlas_blend(const int64_t *contrib, const int64_t *zsum, int32_t T, int64_t *acc, float *meta, ctx_stream_t stream);

/* ---- multi-view consistency (src/training/trainer.py:429-531; the reward of :856-863, switched off upstream) ------- */
/* views [V,C,h,w] f32, faces [F,3] i64, face_idx [V,h,w] i64 (-1 = background), face_vertices_image [V,F,3,2] f32 in [-1, 1].
   Vertex k is seen in view j when it is a corner of a face owning a pixel of face_idx[j].  For target view i, pixel (y, x) with
   f = face_idx[i,y,x] >= 0 and source j != i: c = first corner of faces[f] seen in j (none: no pair), (X, Y) = face_vertices_image[j,f,c],
   sx = trunc(((X + 1) / 2) * w), sy = trunc(((Y + 1) / 2) * h) for rows = 0 (upstream's rows) or trunc(((1 - Y) / 2) * h) for rows = 1
   (the raster's rows).  (sy, sx) outside the image: counted in n_outside, nothing else.  d = 1 - (|t0 - s0| + |t1 - s1| + ..) / C in f32,
   t = views[i,:,y,x], s = views[j,:,sy,sx]; the pair counts when d >= 0: pair_sum[j,i] += floor(d * 2^32), pair_count[j,i] += 1 (both
   [V,V] i64, written, not accumulated).  mean = sum(pair_sum) / 2^32 / sum(pair_count) in f64 rounded to f32; 0 when nothing counts.
   Integer sums: the results do not depend on the launch geometry or the stream.  1 <= V <= 16, 1 <= C <= 4.
   seen [V, n_vertices] u8 of ctx_view_consistency_ws_bytes(V, n_vertices) bytes: built when build_seen != 0, else read as a
   previous call on the same face_idx left it (trainer.py:429-531 rebuilds it on every call). */
int64_t ctx_view_consistency_ws_bytes(int32_t V, int32_t n_vertices);
int32_t ctx_view_consistency_fwd(const float *views, const int64_t *faces, const int64_t *face_idx, const float *face_vertices_image,
                                 int32_t V, int32_t C, int32_t h, int32_t w, int32_t F, int32_t n_vertices, int32_t rows, int32_t build_seen,
                                 uint8_t *seen, int64_t seen_bytes, int64_t *pair_sum, int64_t *pair_count, int64_t *n_outside, float *mean,
                                 ctx_stream_t stream);
/* Gradient of that mean (trainer.py:429-531 under autograd) with respect to views: per counted pair sign_count[i,c,y,x] -= sign(t_c - s_c)
   and sign_count[j,c,sy,sx] += sign(t_c - s_c), sign(0) = 0; sign_count [V,C,h,w] i32 (written); then
   grad_views = float(sign_count) * (u * grad_mean[0]), u = (1 / float(N)) / C, N = sum(pair_count) of the forward.  pair_count and
   grad_mean are device memory: no host sync. */
int32_t ctx_view_consistency_bwd(const float *views, const int64_t *faces, const int64_t *face_idx, const float *face_vertices_image,
                                 const uint8_t *seen, int32_t V, int32_t C, int32_t h, int32_t w, int32_t F, int32_t n_vertices, int32_t rows,
                                 const int64_t *pair_count, const float *grad_mean, int32_t *sign_count, float *grad_views, ctx_stream_t stream);

/* ---- exposure compensation across painted views: the pair statistics the per-view gains are solved from ------- */
/* atlases [V,4,Tc,Tc] i64: per view the weighted colour sums and the weight sum of a low-resolution back-projection in units of 2^-32
   (ctx_uv_scatter_fixed).  Per texel p, view v, channel ch: w = A[v,3,p], c = float32(float64(A[v,ch,p]) / float64(w)); v is valid at p
   when w > 0 and lo <= c <= hi on all three channels; q = int64(rintf(c * 2^24)).  For every ordered pair (i, j), i == j included, with
   both views valid at p: count[i,j] += 1 and colour_sum[i,j,ch] += q_i[ch] (count [V,V] i64, colour_sum [V,V,3] i64; written, not
   accumulated).  Integer sums: the results do not depend on the launch geometry or the texel order.  1 <= V <= 16, 1 <= Tc <= 4096,
   0 < lo < hi <= 1.  No host sync. */
int32_t ctx_view_pair_stats(const int64_t *atlases, int32_t V, int32_t Tc, float lo, float hi, int64_t *count, int64_t *colour_sum,
                            ctx_stream_t stream);

/* Texel-interleaved forward for C <= 4 and one texture shared by the batch (the reference's texture_img.expand(B, ...),
   render.py:133-135): ctx_texture_pack4 repacks [C,T,T] into [T,T,4] once, ctx_texture_mapping_packed_fwd then gathers one
   16-byte texel per bilinear tap.  Results are bit-identical to ctx_texture_mapping_fwd. */
int32_t ctx_texture_pack4(const float *tex, int32_t C, int32_t T, float *packed, ctx_stream_t stream);
int32_t ctx_texture_mapping_packed_fwd(const float *uv, const float *packed, int32_t B, int32_t HW, int32_t C, int32_t T,
                                       int32_t mode, const int64_t *mask_idx, float *out, ctx_stream_t stream);

/* ---- view weights: torch_scatter.scatter_max seam (src/training/trainer.py:213-249) ------- */
/* phase 0: max_z[f] = max(max_z[f], fnz[b,f]) over pixels of the B local views showing f.
   Caller pre-fills max_z with -inf; between the phases a multi-GPU caller all-reduces(MAX). */
int32_t ctx_view_weights_max(const int64_t *face_idx, const float *fnz, int32_t B, int32_t HW,
                             int32_t F, float *max_z, void *vis_ws /* B*F bytes */, ctx_stream_t stream);
/* phase 1: mask[b,p] = !(fnz[b,f] < max_z[f]) for f>=0, 1 for background. */
int32_t ctx_view_weights_mask(const int64_t *face_idx, const float *fnz, const float *max_z,
                              int32_t B, int32_t HW, int32_t F, uint8_t *mask, ctx_stream_t stream);
/* ConTEXTure.create_face_view_map (trainer.py:155-211): rows (face,view,i,j) of valid pixels in
   (view, row, col) order.  ws: ctx_face_view_map_ws_bytes.  n_rows: device int64[1]. */
int64_t ctx_face_view_map_ws_bytes(int32_t B, int32_t H, int32_t W);
int32_t ctx_face_view_map(const int64_t *face_idx, int32_t B, int32_t H, int32_t W,
                          int64_t *rows /*[B*H*W,4] capacity*/, int64_t *n_rows, void *ws,
                          ctx_stream_t stream);

/* ---- texture field: get_embedder / NeRF2D (src/run_nerf_helpers.py:15-135) ---------------- */
/* embed(x[N,d]) -> [N, d*(1+2L)], order [x, sin(2^0 x), cos(2^0 x), sin(2^1 x), ...]. */
int32_t ctx_embed_fwd(const float *x, int64_t N, int32_t d, int32_t L, float *out, ctx_stream_t stream);
/* The envelope of every ctx_uvmlp_* entry point: 1 <= D <= 16 hidden layers, W in {64, 128, 256} (no other width: W = 192 is refused),
   1 <= input_ch <= 64 (dims * (1 + 2L) with dims in {2, 3} where an entry takes dims / L; the embedding is padded to EP = 48 for
   input_ch <= 48, else to 64), 1 <= output_ch <= 4, N >= 1.  Outside it the three size queries return -1 and every other entry
   returns CTX_E_ARG before it launches anything.
   skip: the hidden layer after which the embedding is concatenated again, i.e. layer skip + 1 reads [embedding, hidden].  A skip
   outside [0, D-2] means NO skip layer to ctx_uvmlp_packed_bytes, ctx_uvmlp_pack and the forward entries (every hidden layer after the
   first reads the hidden vector alone; ws[i] is then [W, W] for every 1 <= i < D), and is refused (CTX_E_ARG, nothing launched) by the
   three backward entries ctx_uvmlp_bwd, ctx_uvmlp_bwd_idx and ctx_uvmlp_bwd_emb; so D = 1 is forward only. */
/* Bytes of the packed-weight blob for NeRF2D(D,W,input_ch,output_ch,skip); never less than the parameters' 4 bytes each, and
   non-decreasing in D. */
int64_t ctx_uvmlp_packed_bytes(int32_t D, int32_t W, int32_t input_ch, int32_t output_ch, int32_t skip);
/* Pack nn.Linear weights: ws[i] -> device float [out_i,in_i], bs[i] -> device float [out_i];
   index D is output_linear. */
int32_t ctx_uvmlp_pack(const float *const *ws, const float *const *bs, int32_t D, int32_t W,
                       int32_t input_ch, int32_t output_ch, int32_t skip, void *packed,
                       ctx_stream_t stream);
/* Fused  embed(uv) -> NeRF2D -> raw[N,3]  (+ optional tex_chw[3,N] = (tanh(raw)+1)/2 laid out as the
   [1,3,res,res] atlas of textured_mesh.py:298-301).  uv nullable: then uv = the res x res 'xy'
   meshgrid of linspace(0,1,res) (textured_mesh.py:269-273), N = res*res. */
/* emb (nullable): precomputed embedding [N, 2*(1+2L)] as returned by embed(); when given it is
   loaded instead of being recomputed from uv (keeps the NeRF2D.forward(embedded) seam). */
int32_t ctx_uvmlp_fwd(const float *uv /*nullable*/, const float *emb /*nullable*/, int64_t N, int32_t res, const void *packed,
                      int32_t D, int32_t W, int32_t L, int32_t output_ch, int32_t skip,
                      float *raw, float *tex_chw /*nullable*/, ctx_stream_t stream);

/* General / training forward.  dims = 2 (uv, as ctx_uvmlp_fwd) or 3 (xyz sample points of the ray path: the reference's
   NeRF2D defaults, input_ch = 3*(1+2L) <= 64, output_ch = 4 = rgb + sigma); `uv` is then the [N,dims] point list.
   saved (nullable: plain forward) keeps what the backward needs (ctx_uvmlp_saved_bytes(N,D,W,input_ch) bytes: the padded
   embedding [N,EP], the post-ReLU activations [D,N,W] fp32 and the ReLU pattern as bit masks [D, ceil(N/64), W] u64:
   N*(EP + D*W)*4 + D*ceil(N/64)*W*8). */
int64_t ctx_uvmlp_saved_bytes(int64_t N, int32_t D, int32_t W, int32_t input_ch);
int32_t ctx_uvmlp_fwd_save(const float *uv /*nullable*/, const float *emb /*nullable*/, int64_t N, int32_t res, const void *packed,
                           int32_t D, int32_t W, int32_t dims, int32_t L, int32_t output_ch, int32_t skip,
                           float *raw, float *tex_chw /*nullable*/, void *saved /*nullable: plain forward*/, ctx_stream_t stream);
/* Backward of NeRF2D.forward (autograd of src/run_nerf_helpers.py:106-135; the SDS loop src/training/trainer.py:644-907
   drives it with the atlas gradient).  Upstream gradient: grad_raw [N,output_ch] (d loss / d mlp_output) and / or
   grad_tex [output_ch,N] (d loss / d texture atlas of textured_mesh.py:298-301; the (tanh+1)/2 is differentiated
   here from `raw`).  Writes (not accumulates) d loss / d weight into gws[i] ([out_i,in_i], nn.Linear layout) and
   d loss / d bias into gbs[i], i = 0..D-1 hidden, D = output_linear (host arrays of device pointers).
   ws: ctx_uvmlp_bwd_ws_bytes(N,D,W) bytes of scratch.  Deterministic (fixed-order partial sums). */
int64_t ctx_uvmlp_bwd_ws_bytes(int64_t N, int32_t D, int32_t W);
int32_t ctx_uvmlp_bwd(const float *grad_raw /*nullable*/, const float *grad_tex /*nullable*/, const float *raw /*nullable w/o grad_tex*/,
                      int64_t N, const void *packed, int32_t D, int32_t W, int32_t dims, int32_t L, int32_t output_ch, int32_t skip,
                      const void *saved, void *ws, float *const *gws, float *const *gbs, ctx_stream_t stream);

/* The `emb` seam on its own, with the gradient to the embedding (the hash-grid field): ctx_uvmlp_fwd_save / ctx_uvmlp_bwd
   with the embedding's width given instead of derived from (dims, L): emb [N, input_ch], 1 <= input_ch <= 64, raw [N, output_ch], no atlas.
   Always the exact-f32 chain; with input_ch = 63 the launches, and so the bits, are those of ctx_uvmlp_fwd_save(emb, dims = 3, L = 10) /
   ctx_uvmlp_bwd.  saved (nullable: plain forward): ctx_uvmlp_saved_bytes(N, D, W, input_ch); ws: ctx_uvmlp_bwd_ws_bytes(N, D, W).
   grad_emb [N, input_ch] (nullable: skipped) = dZ_0 . W_0 + dZ_{skip+1} . W_{skip+1}[:, :input_ch], one kernel after the dZ chain that
   reads the dZ rows the chain left in ws.  gws and gbs both null with a grad_emb: the input gradient alone, no weight-gradient launch, the
   same bits in grad_emb.  Deterministic. */
int32_t ctx_uvmlp_fwd_emb(const float *emb, int64_t N, const void *packed, int32_t D, int32_t W, int32_t input_ch, int32_t output_ch,
                          int32_t skip, float *raw, void *saved /*nullable*/, ctx_stream_t stream);
int32_t ctx_uvmlp_bwd_emb(const float *grad_raw, int64_t N, const void *packed, int32_t D, int32_t W, int32_t input_ch, int32_t output_ch,
                          int32_t skip, const void *saved, void *ws, float *const *gws, float *const *gbs, float *grad_emb /*nullable*/,
                          ctx_stream_t stream);

/* ---- texture field on the texels the views sample (TexturedMeshModel.get_texture_map_only_valid_areas,
   src/models/textured_mesh.py:303-347, queries the MLP on chosen texels only; here the choice is what a cached raster can read) ---- */
/* The active set of a raster, in binary32 in the order ctx_texture_mapping_fwd / _bwd use: for every pixel of uv [B,H,W,2] with
   face_idx[b,y,x] >= 0:  ix = src_index(u*2 - 1, T), iy = src_index((1 - v)*2 - 1, T) with src_index(g, T) =
   min(T - 1, max(((g + 1)*T - 1)/2, 0));  x0 = (int)floorf(ix), y0 = (int)floorf(iy), x1 = x0 + 1, y1 = y0 + 1;  each of the four
   (y, x) with 0 <= x < T and 0 <= y < T is active, whatever its bilinear weight.  Background pixels mark nothing and their uv is
   not read.  mask_u8 [T,T]: plain byte stores of 1, never cleared — the caller zeroes it, several calls accumulate a union.  T >= 2. */
int32_t ctx_texel_active_mark(const float *uv, const int64_t *face_idx, int32_t B, int32_t H, int32_t W, int32_t T, uint8_t *mask_u8,
                              ctx_stream_t stream);
/* Ordered compaction of such a mask (count, scan, write, as ctx_face_view_map): idx_out[0:count_out[0]] = the flat indices y*T + x
   of the n bytes that are non-zero, ascending; the rest of idx_out [n] is not written.  count_out: device int64[1].
   1 <= n < 2^31.  ws: ctx_texel_compact_ws_bytes(n) bytes (-1: n refused). */
int64_t ctx_texel_compact_ws_bytes(int64_t n);
int32_t ctx_texel_compact(const uint8_t *mask, int64_t n, int32_t *idx_out, int64_t *count_out, void *ws, ctx_stream_t stream);
/* ctx_uvmlp_fwd_save / ctx_uvmlp_bwd of the 2-D field on a list idx int32 [N] of nodes of the res x res grid (distinct, each in
   [0, res^2); 1 <= N <= res^2, res >= 2).  Row n of the launch is node idx[n]: its coordinates come from the grid mode's linspace
   expression, so they carry that mode's bits, and so do raw and the atlas value of a listed texel.  raw [N,output_ch], saved
   (ctx_uvmlp_saved_bytes(N, ...)) and the backward's scratch (ctx_uvmlp_bwd_ws_bytes(N, ...)) are compact; tex_chw and grad_tex
   are whole atlases [output_ch, res^2]: tex_chw is written at the listed texels only (the caller fills the rest), grad_tex is
   read at the listed texels only.  A list entry outside the grid is skipped (nothing stored, nothing read). */
int32_t ctx_uvmlp_fwd_save_idx(const int32_t *idx, int64_t N, int32_t res, const void *packed, int32_t D, int32_t W, int32_t L,
                               int32_t output_ch, int32_t skip, float *raw, float *tex_chw /*nullable*/, void *saved /*nullable*/,
                               ctx_stream_t stream);
int32_t ctx_uvmlp_bwd_idx(const float *grad_raw /*nullable*/, const float *grad_tex /*nullable*/, const int32_t *idx, int32_t res,
                          const float *raw /*nullable w/o grad_tex*/, int64_t N, const void *packed, int32_t D, int32_t W, int32_t L,
                          int32_t output_ch, int32_t skip, const void *saved, void *ws, float *const *gws, float *const *gbs,
                          ctx_stream_t stream);

/* ---- ray path (north_star; dead/absent in the reference) ------------------------ */
/* get_rays (run_nerf_helpers.py:139-148): K row-major [3,3] host floats passed by value fields. */
int32_t ctx_get_rays(int32_t H, int32_t W, float fx, float fy, float cx, float cy,
                     const float *c2w /*[3,4] device*/, float *rays_o, float *rays_d, ctx_stream_t stream);
/* nerf-pytorch raw2outputs: raw[R,S,4] z[R,S] rays_d[R,3] -> rgb[R,3] disp[R] acc[R]
   weights[R,S] (nullable) depth[R]. */
int32_t ctx_raymarch_composite_fwd(const float *raw, const float *z_vals, const float *rays_d,
                                   int64_t R, int32_t S, int32_t white_bkgd, float *rgb, float *disp,
                                   float *acc, float *weights, float *depth, ctx_stream_t stream);
/* The same with nerf-pytorch's density noise: sigma = relu(raw.w + noise), noise[R,S] (nullable: then this is
   ctx_raymarch_composite_fwd bit for bit; with noise it equals that call on raw with the noise added to .w). */
int32_t ctx_raymarch_composite_fwd_noise(const float *raw, const float *z_vals, const float *rays_d,
                                         const float *noise /*nullable*/, int64_t R, int32_t S, int32_t white_bkgd,
                                         float *rgb, float *disp, float *acc, float *weights /*nullable*/, float *depth,
                                         ctx_stream_t stream);
/* Backward of the compositing with respect to raw: grad_raw[R,S,4] = d loss / d raw, every element written.  The
   upstream gradients g_rgb[R,3] g_disp[R] g_acc[R] g_weights[R,S] g_depth[R] are each nullable (= zero).  alpha,
   transmittance, acc and depth are recomputed from the inputs with the forward's instruction sequence: nothing is
   carried over from the forward.  On a ray with acc == 0 the disparity terms are dropped (finite result); grad_raw.w
   is exactly 0 where raw.w + noise <= 0.  S <= 4096, larger S is refused with a message.  No gradient with respect
   to z_vals or rays_d.  Deterministic (no atomics, fixed summation order). */
int32_t ctx_raymarch_composite_bwd(const float *raw, const float *z_vals, const float *rays_d,
                                   const float *noise /*nullable*/, int64_t R, int32_t S, int32_t white_bkgd,
                                   const float *g_rgb, const float *g_disp, const float *g_acc, const float *g_weights,
                                   const float *g_depth, float *grad_raw, ctx_stream_t stream);

/* ---- occupancy grid of the ray path: evaluate the field only on the samples that lie in occupied cells ---- */
/* The grid: cells uint8 [G,G,G] (flat index (cz*G + cy)*G + cx, 1 = occupied) and dens float32 [G,G,G] over the box lo .. hi,
   1 <= G <= 256.  The host computes inv = G / (hi - lo) and h = (hi - lo) / G once per axis in binary32 and passes them by value.
   All arithmetic below is binary32 in the order written (no contraction).
   ctx_occ_mark: for every sample of z_vals [R,S]: p = o + d*z (one product, one sum per axis: the bits of the torch expression
   rays_o + rays_d * z), t = (p - lo)*inv; the sample is inside when t >= 0 && t < G on the three axes (false for NaN); then
   mask = cells[(int)t], else 0.  Every byte of mask [R*S] is written.  1 <= R*S < 2^31 (the rule of ctx_texel_compact, which turns the
   mask into the ascending list idx). */
int32_t ctx_occ_mark(const float *rays_o, const float *rays_d, const float *z_vals, int64_t R, int32_t S, const uint8_t *cells,
                     int32_t G, float lo_x, float lo_y, float lo_z, float inv_x, float inv_y, float inv_z, uint8_t *mask,
                     ctx_stream_t stream);
/* pts [n,3]: row k = o + d*z of sample idx[k] (ray idx[k] / S), the same expression.  1 <= n <= R*S. */
int32_t ctx_occ_points(const float *rays_o, const float *rays_d, const float *z_vals, int64_t R, int32_t S, const int32_t *idx,
                       int64_t n, float *pts, ctx_stream_t stream);
/* raw [total,4]: row idx[k] = raw_c[k], every other row the fill (0, 0, 0, -1e30f): zero density after the compositing's ReLU, with
   density noise too, and finite.  n = 0 is legal (all fill; raw_c and idx may be null).  Two launches: the fill, then the listed rows. */
int32_t ctx_occ_expand(const float *raw_c, const int32_t *idx, int64_t n, int64_t total, float *raw, ctx_stream_t stream);
/* Backward of ctx_occ_expand: grad_c [n,4], row k = grad[idx[k]].  n >= 1.
   In these three list kernels an idx entry outside [0, total) is skipped: nothing is read or stored through it (ctx_occ_points and
   ctx_occ_expand leave its row alone, ctx_occ_collect writes zeros to it). */
int32_t ctx_occ_collect(const float *grad, const int32_t *idx, int64_t n, int64_t total, float *grad_c, ctx_stream_t stream);
/* pts [G^3,3]: the point of cell c the field is asked at, per axis lo + ((float)c_axis + u)*h with u [G^3,3] in [0,1) (nullable: 0.5). */
int32_t ctx_occ_cell_points(int32_t G, float lo_x, float lo_y, float lo_z, float h_x, float h_y, float h_z,
                            const float *u /*nullable*/, float *pts, ctx_stream_t stream);
/* The refresh from raw [n,4] = the field on those points (n = G^3): sigma = raw.w > 0 ? raw.w : 0, dens = fmaxf(dens*decay, sigma),
   cells = dens > thresh (equality is not occupied).  A NaN raw.w leaves sigma 0 and marks the cell occupied. */
int32_t ctx_occ_update(const float *raw, float *dens, uint8_t *cells, int64_t n, float decay, float thresh, ctx_stream_t stream);

/* ---- occupancy grid from the mesh, and the span of occupied cells along a ray (definitions: tests/test_occupancy_mesh_cpu.py) ---- */
/* ctx_occ_voxelize: stores the byte 1 into every cell a triangle of the mesh touches; never clears (the caller zeroes cells; calls
   accumulate a union); plain byte stores, no atomics.  vertices float32 [V,3] in the frame of the box, faces int64 [F,3].  Binary32 in
   the order written: g = (v - lo)*inv per vertex (the expression of ctx_occ_mark), so cell c is the cube [c, c+1]^3; the test runs on
   the cube inflated by e = 2^-7 of a cell on every side (minimum corner p = c - e, side D = 1 + 2e), which makes the binary32 result a
   superset of the exact overlap and lets a triangle on a cell face mark both layers.  Candidates per axis: max(0, floor(min - e)) ..
   min(G - 1, floor(max + e)) of the triangle's bounding box.  A triangle with a face index outside [0, V) or a non-finite grid
   coordinate marks nothing.  Test (Schwarz and Seidel 2010): n = (g1 - g0) x (g2 - g0); n == 0: every candidate is marked.  Plane:
   crit = D where n > 0 else 0 per axis, d1 = n.(crit - g0), d2 = n.((D - crit) - g0), s1 = n.p + d1, s2 = n.p + d2, passes when s1 and
   s2 do not have the same strict sign (s1*s2 <= 0, written with comparisons).  Edges: for the planes xy, yz, zx and the edges
   e_i = g_{i+1} - g_i: ne = (-e.v, e.u), negated when n's third component there is < 0; de = -(ne.g_i) + max(0, D*ne.u) + max(0, D*ne.v);
   passes when ne.p + de >= 0.  Dots sum left to right.  1 <= G <= 256, 1 <= V, F < 2^31. */
int32_t ctx_occ_voxelize(const float *vertices, const int64_t *faces, int64_t V, int64_t F, int32_t G, float lo_x, float lo_y, float lo_z,
                         float inv_x, float inv_y, float inv_z, uint8_t *cells, ctx_stream_t stream);
/* Cube (Chebyshev) dilation: dst[c] = 1 when any cell of src within k on the three axes is non-zero, else 0.  Separable: x (src -> dst),
   y (dst -> ws), z (ws -> dst), each a running maximum over +-k clamped to the grid.  k >= 0 (above G - 1 it reaches no further); k = 0 copies (non-zero -> 1) and takes
   no workspace.  src, dst and ws [G^3] bytes, pairwise distinct. */
int32_t ctx_occ_dilate(const uint8_t *src, int32_t G, int32_t k, uint8_t *dst, uint8_t *ws /*nullable for k = 0*/, ctx_stream_t stream);
/* span [R,2], hit [R]: where the ray o + d*t enters its first and leaves its last occupied cell within [near, far] clipped to the box;
   (near, far) and hit = 0 for a ray without one.  One lane per ray, binary32 in the order written.  A non-finite o or d: no hit.
   Clip: t_a = near, t_b = far; per axis with d != 0: t1 = (lo - o)/d, t2 = (hi - o)/d, t_a = max(t_a, min(t1, t2)), t_b = min(t_b,
   max(t1, t2)); with d == 0 the ray misses unless lo <= o <= hi; it misses unless t_a <= t_b.  Start cell per axis:
   (int)clamp(((o + d*t_a) - lo)*inv, 0, G - 1).  Walk: at every cell the exit parameter per axis is ((lo + (float)(c + (d > 0))*h) - o)/d
   from the integer cell index (+inf for d == 0; no running sum, no drift); te = the smallest, ties to x before y before z; the cell is
   left at t_out = min(max(te, t_in), t_b), the next cell's t_in (the first one's is t_a); an occupied cell sets span1 = t_out and, if it
   is the first, span0 = t_in.  The walk ends when te >= t_b, when the step along te's axis leaves the grid, or after 3G + 3 cells.
   Finite near < far; 1 <= R < 2^31; span 8-byte aligned. */
int32_t ctx_occ_ray_spans(const float *rays_o, const float *rays_d, int64_t R, float near, float far, const uint8_t *cells, int32_t G,
                          float lo_x, float lo_y, float lo_z, float hi_x, float hi_y, float hi_z, float inv_x, float inv_y, float inv_z,
                          float h_x, float h_y, float h_z, float *span, uint8_t *hit, ctx_stream_t stream);

/* ---- where a ray meets the mesh: cell triangle lists on the grid, and the hit kernel (definition: tests/meshhit_rule.py) ---- */
/* count int32 [G^3] (index (cz*G + cy)*G + cx): how many faces list themselves in each cell.  (cell, face) is listed if and only if
   ctx_occ_voxelize would store a 1 in that cell for that face alone (one predicate, one device function), so count > 0 is the voxeliser's
   grid.  The call zeroes count, then adds with integer atomics: the counts do not depend on scheduling.  Arguments as ctx_occ_voxelize. */
int32_t ctx_mesh_cells_count(const float *vertices, const int64_t *faces, int64_t V, int64_t F, int32_t G, float lo_x, float lo_y, float lo_z,
                             float inv_x, float inv_y, float inv_z, int32_t *count, ctx_stream_t stream);
/* cell_off int32 [ncell + 1]: the exclusive scan of count [ncell]; total[0] (int64) = the sum, which the caller reads back and refuses at
   2^31 or more (an offset beyond int32 is stored as INT32_MAX).  1 <= ncell <= 256^3. */
int32_t ctx_mesh_cells_scan(const int32_t *count, int64_t ncell, int32_t *cell_off, int64_t *total, ctx_stream_t stream);
/* cell_tri int32 [n], n = cell_off[G^3]: cell c owns cell_off[c] .. cell_off[c+1], the faces listed in it, ASCENDING by face id: the array
   has one value whatever the arrival order (an atomic cursor per cell into `slots`, then a rank sort of every segment into cell_tri; any
   segment length).  cursor int32 [G^3] and slots int32 [n] are workspaces (cursor is zeroed here); nothing is stored outside a cell's
   segment or outside [0, n).  n = 0 launches nothing.  The mesh and the grid must be those of the count. */
int32_t ctx_mesh_cells_fill(const float *vertices, const int64_t *faces, int64_t V, int64_t F, int32_t G, float lo_x, float lo_y, float lo_z,
                            float inv_x, float inv_y, float inv_z, const int32_t *cell_off, int64_t n, int32_t *cursor, int32_t *slots,
                            int32_t *cell_tri, ctx_stream_t stream);
/* tri float32 [F,12], 16-byte aligned: per face v0, e1 = v1 - v0, e2 = v2 - v0, each padded with a 0 to four floats, so the hit kernel
   loads three whole vectors and never chases faces -> vertices.  A face with an index outside [0, V) or a non-finite vertex gets twelve
   NaN (and is in no list: it marks nothing in the voxeliser either). */
int32_t ctx_mesh_tri_setup(const float *vertices, const int64_t *faces, int64_t V, int64_t F, float *tri, ctx_stream_t stream);
/* hit u8 [R], t [R], face int32 [R], uv [R,2]: where the ray o + d*t first meets the mesh within [near, far].  One lane per ray, binary32
   in the order written.  The walk is that of ctx_occ_ray_spans on cells = (count > 0) (one device function); in every occupied cell the
   triangles cell_tri[cell_off[c] .. cell_off[c+1]) are tested in list order.
   Test of a triangle (v0, e1, e2), dots summed (ax*bx + ay*by) + az*bz: p = d x e2, det = e1.p, inv = 1/det, s = o - v0, u = (s.p)*inv,
   q = s x e1, v = (d.q)*inv, t = (e2.q)*inv.  Miss if det == 0, or if inv or t is not finite.  Accepted if and only if u >= -EPS,
   v >= -EPS, u + v <= 1 + EPS and near <= t <= far, with EPS = 2^-18.  Two-sided: back faces count.
   mode 0 (nearest): the best (t, face) is the lowest t, ties to the lower face id; a triangle seen in any cell counts with its t wherever
   that t lies; after every cell the walk stops when best.t <= t_out of that cell (the lists are conservative, so no later cell holds a
   nearer hit).  A miss stores hit = 0, t = far, face = -1, uv = 0.  mode 1 (any): stops at the first accepted triangle; only hit is
   stored (t, face, uv may be null) and it equals mode 0's.
   own_face int64 [R] (nullable): for an entry in [0, F) the triangles that are that face or share a vertex id with it in faces [F,3] are
   skipped (the integer "related" rule of ctx_uv_gather_fixed): a ray leaving a surface point is blinded neither by its own face nor by
   one adjacent across a crease.  Non-finite rays, a zero direction and rays that miss the box are misses.  R = 0 launches nothing.
   Finite near < far; 0 <= R < 2^31; 1 <= F < 2^31; 0 <= n < 2^31; tri 16-byte and uv 8-byte aligned.  Entries of cell_off and cell_tri
   that point outside [0, n) or [0, F) are skipped. */
int32_t ctx_mesh_ray_hit(const float *rays_o, const float *rays_d, int64_t R, float near, float far, const uint8_t *cells, int32_t G,
                         float lo_x, float lo_y, float lo_z, float hi_x, float hi_y, float hi_z, float inv_x, float inv_y, float inv_z,
                         float h_x, float h_y, float h_z, const int32_t *cell_off, const int32_t *cell_tri, int64_t n, const float *tri,
                         const int64_t *faces, int64_t F, const int64_t *own_face /*nullable*/, int32_t mode, uint8_t *hit,
                         float *t /*nullable for mode 1*/, int32_t *face /*nullable for mode 1*/, float *uv /*nullable for mode 1*/,
                         ctx_stream_t stream);
/* found u8 [n], dist [n], face int32 [n], uv [n,2]: the nearest point of the mesh to each of pts [n,3] within the radius r (definition:
   tests/meshdist_rule.py).  One lane per point, binary32 in the order written; cell_off, cell_tri and tri are those of the calls above.
   Block: per axis a = floorf(((p - r) - lo)*inv), b = floorf(((p + r) - lo)*inv).  A miss if p is not finite, or if on any axis b < 0 or
   a > G - 1; otherwise both are clamped to [0, G - 1] and every triangle listed in any cell of [a, b]^3 is looked at (no cell is left
   out; a triangle listed in several cells gives the same numbers each time).
   Point against a triangle (v0, e1, e2), Ericson's closest point region by region, dots summed (ax*bx + ay*by) + az*bz:
     ap = p - v0, d1 = e1.ap, d2 = e2.ap;   d1 <= 0 and d2 <= 0 -> (u, v) = (0, 0)
     bp = ap - e1, d3 = e1.bp, d4 = e2.bp;  d3 >= 0 and d4 <= d3 -> (1, 0)
     vc = d1*d4 - d3*d2;                    vc <= 0 and d1 >= 0 and d3 <= 0 -> (d1/(d1 - d3), 0)
     cp = ap - e2, d5 = e1.cp, d6 = e2.cp;  d6 >= 0 and d5 <= d6 -> (0, 1)
     vb = d5*d2 - d1*d6;                    vb <= 0 and d2 >= 0 and d6 <= 0 -> (0, d2/(d2 - d6))
     va = d3*d6 - d5*d4;                    va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0 -> w = (d4 - d3)/((d4 - d3) + (d5 - d6)), (1 - w, w)
     otherwise den = 1/((va + vb) + vc) -> (vb*den, vc*den)
   then q = v0 + (e1*u + e2*v) per component, s = p - q, d2 = (sx*sx + sy*sy) + sz*sz.  A record with a NaN, or a non-finite d2, u or v,
   is skipped.  The answer is the minimum over (d2, face) in lexicographic order (the lower face id on equal d2), accepted only if
   d2 <= r*r: found = 1, dist = sqrtf(d2), face, uv; the nearest point is v0 + u e1 + v e2 of that face.  A miss stores found = 0,
   dist = r, face = -1, uv = 0.  The nearest point of a triangle that lies outside the box is in no cell: the answer is for the mesh
   inside the box.  n = 0 launches nothing.
   0 <= n < 2^31; 0 <= n_list < 2^31; 1 <= G <= 256; 1 <= F < 2^31; r finite, > 0 and at most 3 min(h) (a block of at most 7^3 cells);
   tri 16-byte and uv 8-byte aligned.  Entries of cell_off and cell_tri that point outside [0, n_list) or [0, F) are skipped. */
int32_t ctx_mesh_closest_point(const float *pts, int64_t n, float r, int32_t G, float lo_x, float lo_y, float lo_z, float inv_x, float inv_y,
                               float inv_z, const int32_t *cell_off, const int32_t *cell_tri, int64_t n_list, const float *tri, int64_t F,
                               uint8_t *found, float *dist, int32_t *face, float *uv, ctx_stream_t stream);

/* ---- on which side of the mesh a point lies: pseudonormal tables and the signed query (definition: tests/meshsdf_rule.py) ---- */
/* count int32 [V]: how many corners of faces [F,3] name each vertex id.  Only a face whose three ids lie in [0, V) is counted, once per
   corner.  The call zeroes count, then adds with integer atomics.  Its exclusive scan is ctx_mesh_cells_scan with ncell = V, which sets
   the envelope: 1 <= V <= 256^3; 1 <= F < 2^31 / 3. */
int32_t ctx_mesh_vertex_faces_count(const int64_t *faces, int64_t V, int64_t F, int32_t *count, ctx_stream_t stream);
/* vf_face int32 [n], n = vf_off[V]: vertex w owns vf_off[w] .. vf_off[w+1], the faces that name it at a corner, ASCENDING by face id (a
   face that names it twice is listed twice): one value whatever the arrival order, as ctx_mesh_cells_fill (the same cursor, slots and
   rank sort).  cursor int32 [V] and slots int32 [n] are workspaces; nothing is stored outside a segment or outside [0, n).  n = 0
   launches nothing; 0 <= n <= 3 F. */
int32_t ctx_mesh_vertex_faces_fill(const int64_t *faces, int64_t V, int64_t F, const int32_t *vf_off, int64_t n, int32_t *cursor, int32_t *slots,
                                   int32_t *vf_face, ctx_stream_t stream);
/* pn float32 [F,7,3]: the angle-weighted pseudonormals (Baerentzen & Aanaes 2005) of every face's seven features, in the order of the
   signed query's feature code.  Binary32 in the order written, dots summed (ax*bx + ay*by) + az*bz.  tri is ctx_mesh_tri_setup's.
   Row 0, the face: n = e1 x e2 (nx = e1y*e2z - e1z*e2y, ny = e1z*e2x - e1x*e2z, nz = e1x*e2y - e1y*e2x), nn = n.n, u = n / sqrtf(nn) per
     component if 0 < nn < inf, else 0 (a zero-area face).  A face COUNTS in the sums below if its u is finite and not (0, 0, 0).
   Rows 1-3, the vertices faces[f,0..2]: the sum, over the counting faces g in that vertex id's list, ascending g, of alpha*u_g per
     component (acc = acc + alpha*u from 0), alpha = atan2f(|a x b|, a.b) the angle of g at the first corner that names the id: at v0
     a = e1, b = e2; at v1 a = -e1, b = e2 - e1; at v2 a = -e2, b = e1 - e2.
   Rows 4-6, the edges (v0,v1), (v0,v2), (v1,v2): the sum of u_g over the counting faces g, in the list of the edge's first vertex,
     ascending g, that name the two ids at two different corners.  A boundary edge gets its one face's normal, a non-manifold edge the sum
     of all its faces.
   Rows 1-6 are not normalised.  A face whose record holds a NaN (an id outside [0, V), a non-finite vertex) has seven NaN rows and
   counts nowhere.  No atomics; every element has one writer and one value.  Entries of vf_off and vf_face that point outside
   [0, n_vf) or [0, F) are skipped.  1 <= V < 2^31; 1 <= F < 2^31 / 21; 0 <= n_vf <= 3 F; tri 16-byte aligned. */
int32_t ctx_mesh_pseudonormals(const int64_t *faces, int64_t V, int64_t F, const float *tri, const int32_t *vf_off, const int32_t *vf_face,
                               int64_t n_vf, float *pn, ctx_stream_t stream);
/* found u8 [n], sdist [n], face int32 [n], uv [n,2], feature u8 [n], grad [n,3]: ctx_mesh_closest_point's block walk, triangle arithmetic
   and minimum over (d2, face), the same code and the same bits, and then: the winning face is evaluated once more, which gives the same
   u, v, s = p - q and d2 as inside the loop, and feature = the region that answers: 0 the interior; 1 / 2 / 3 the vertices v0, v0 + e1,
   v0 + e2; 4 / 5 / 6 the edges along e1, along e2 and opposite v0.  N = pn[face, feature] (pn [pn_faces,7,3] of
   ctx_mesh_pseudonormals), dot = (sx*Nx + sy*Ny) + sz*Nz, sgn = -1 if dot < 0 else +1: zero, NaN and d2 = 0 count as outside.
   sdist = sgn * sqrtf(d2); grad = (sgn*s) / sqrtf(d2) per component if d2 > 0, else N / sqrtf((Nx*Nx + Ny*Ny) + Nz*Nz) per component, or
   0 where that is not finite.  A miss stores found = 0, sdist = +r, face = -1, uv = 0, feature = 0, grad = 0.
   Negative means inside only for a closed, consistently oriented mesh wound outward; an inward-wound mesh inverts the sign, and an open
   or non-manifold one has no inside.  Envelope, alignment and refusals as ctx_mesh_closest_point; pn_faces >= F. */
int32_t ctx_mesh_signed_distance(const float *pts, int64_t n, float r, int32_t G, float lo_x, float lo_y, float lo_z, float inv_x, float inv_y,
                                 float inv_z, const int32_t *cell_off, const int32_t *cell_tri, int64_t n_list, const float *tri, int64_t F,
                                 const float *pn, int64_t pn_faces, uint8_t *found, float *sdist, int32_t *face, float *uv, uint8_t *feature,
                                 float *grad, ctx_stream_t stream);

/* ---- marching the grid into ragged per-ray sample lists, and the compositing on them (definition: tests/march_rule.py) ---- */
/* count [R]: how many samples the march places on each ray.  The finite check, the clip, the start cell and the walk are those of
   ctx_occ_ray_spans, expression for expression (one device function).  A run is a maximal sequence of consecutive occupied cells of the
   walk: a = t_in of its first cell, b = t_out of its last; an empty cell closes the open run (also an empty cell of zero length between two
   occupied ones), and so do the end of the walk and a step that leaves the grid.  step > 0 is a WORLD length.  A closed run [a, b]:
   nrm = sqrtf((dx*dx + dy*dy) + dz*dz), len = (b - a)*nrm; no sample unless len > 0 (false for NaN); else
   k = (int)min(max(ceilf(len / step), 1), 4097), dt = (b - a) / (float)k, and sample j = 0 .. k-1 sits at t_j = a + ((float)j + u)*dt with
   interval width dt: the intervals tile the run.  count = the sum of k over the ray's runs; 0 for a ray that is non-finite, misses the box
   or meets no occupied cell.  Binary32 in the order written; sqrtf and / correctly rounded.  Arguments as ctx_occ_ray_spans. */
int32_t ctx_occ_march_count(const float *rays_o, const float *rays_d, int64_t R, float near, float far, const uint8_t *cells, int32_t G,
                            float lo_x, float lo_y, float lo_z, float hi_x, float hi_y, float hi_z, float inv_x, float inv_y, float inv_z,
                            float h_x, float h_y, float h_z, float step, int32_t *count, ctx_stream_t stream);
/* The same walk, writing the lists: ray r stores its samples, in walk order (ascending t), at ray_off[r] .. ray_off[r+1] of ray_id int32 [n],
   t [n], dt [n] and pts [n,3] with p = o + d*t_j (one product, one sum per axis: the bits of ctx_occ_points).  ray_off int64 [R+1] is the
   exclusive scan of count, n = ray_off[R] < 2^31.  u [n] (nullable: 0.5, the midpoints) holds one draw in [0,1) per sample.  A ray never
   stores past ray_off[r+1] nor outside [0, n), whatever it computes; n = 0 is legal (nothing is launched, the lists may be null). */
int32_t ctx_occ_march_write(const float *rays_o, const float *rays_d, int64_t R, float near, float far, const uint8_t *cells, int32_t G,
                            float lo_x, float lo_y, float lo_z, float hi_x, float hi_y, float hi_z, float inv_x, float inv_y, float inv_z,
                            float h_x, float h_y, float h_z, float step, const int64_t *ray_off, const float *u /*nullable*/, int64_t n,
                            int32_t *ray_id, float *t, float *dt, float *pts, ctx_stream_t stream);
/* ctx_raymarch_composite_fwd_noise on ragged lists: ray r holds the samples ray_off[r] .. ray_off[r+1] of raw [n,4], t [n], dt [n]
   (noise [n] nullable), and sample s has the distance dist = dt_s * |rays_d| in place of (z_{s+1} - z_s) * |rays_d|: no sample gets the
   1e10 distance, the background shows through what the lists leave.  Everything after dist is the dense kernel's code, so a rectangular
   layout (ray_off = r*S, dt = z_{s+1} - z_s with 1e10 last) gives the dense kernel's bits.  depth = sum w*t.  A ray without samples:
   acc = depth = 0, rgb 0 (1 with white_bkgd), disp = 0/0 as the dense kernel gives a ray of zero density.  weights [n] nullable.
   0 <= n < 2^31; a ray whose ray_off leaves [0, n] or descends is taken as empty. */
int32_t ctx_raymarch_packed_fwd(const float *raw, const float *t, const float *dt, const float *rays_d, const float *noise /*nullable*/,
                                const int64_t *ray_off, int64_t R, int64_t n, int32_t white_bkgd, float *rgb, float *disp, float *acc,
                                float *weights /*nullable*/, float *depth, ctx_stream_t stream);
/* Backward with respect to raw, the closed form of ctx_raymarch_composite_bwd on the lists: grad_raw [n,4], every row of every ray
   written, nothing for a ray without samples; upstream gradients each nullable (g_weights [n]).  No atomics, one summation order.  A ray
   with more than 4096 samples (which the march never makes: only a caller's own ray_off can) gets NaN in its rows; other rays are
   unaffected.  No gradient with respect to t, dt or rays_d. */
int32_t ctx_raymarch_packed_bwd(const float *raw, const float *t, const float *dt, const float *rays_d, const float *noise /*nullable*/,
                                const int64_t *ray_off, int64_t R, int64_t n, int32_t white_bkgd, const float *g_rgb, const float *g_disp,
                                const float *g_acc, const float *g_weights, const float *g_depth, float *grad_raw, ctx_stream_t stream);
/* mip-NeRF 360's distortion loss of the weights on the same lists (definition: tests/distortion_rule.py).  With |d| = the norm of ray r's
   direction as the compositing forms it, x_i = (t_i - t_0) * |d| and delta_i = dt_i * |d| (world lengths, centred on the ray's first sample):
   loss[r] = sum_i sum_j w_i w_j |x_i - x_j| + (1/3) sum_i w_i^2 delta_i, evaluated by prefix sums as
   sum_i w_i * (2 * (x_i * W_<i - V_<i) + delta_i * w_i / 3) with W_<i = sum_{j<i} w_j, V_<i = sum_{j<i} w_j x_j: t ascending inside a ray is a
   precondition and is not checked.  loss [R]: every element written, 0 for a ray without samples and for a zero direction; a non-finite
   weight poisons its own ray only.  n = 0 zero-fills loss (the lists may be null).  ray_off as ctx_raymarch_packed_fwd.  The chunks of a
   ray are chained by two carried scalars, so there is no 4096-sample limit. */
int32_t ctx_distortion_packed_fwd(const float *weights, const float *t, const float *dt, const float *rays_d, const int64_t *ray_off, int64_t R,
                                  int64_t n, float *loss, ctx_stream_t stream);
/* Backward with respect to weights: grad_w[i] = g_loss[r] * (2 * (x_i * (W_<i - W_>i) - (V_<i - V_>i)) + 2 * w_i * delta_i / 3) with the
   suffix sums taken as total minus inclusive prefix.  grad_w [n]: every row of every ray written, nothing for a ray without samples.
   Recomputed from the inputs, nothing saved; no atomics, one summation order; no 4096-sample limit.  No gradient with respect to t, dt
   or rays_d. */
int32_t ctx_distortion_packed_bwd(const float *weights, const float *t, const float *dt, const float *rays_d, const int64_t *ray_off, int64_t R,
                                  int64_t n, const float *g_loss, float *grad_w, ctx_stream_t stream);

/* Importance resampling of the same lists (definition: tests/resample_rule.py).  Ray r's S = ray_off[r+1] - ray_off[r]
   coarse samples arrive as interval start ts [n], width dt [n] >= 0 and weight weights [n]; it gets the K fine samples fine_off[r] ..
   fine_off[r+1] (fine_off int64 [R+1] = K * the exclusive scan of S > 0; n_fine = fine_off[R]).  Mass m_i = min(max(w_i, 0), 1) + 1e-5 (a NaN
   weight counts as 0, +inf as 1); C, l = the exclusive prefix sums of m and dt, W, L their totals.  At u in [0, 1]: tau = u*W, i = the last
   interval with C_i <= tau, f = clamp((tau - C_i)/m_i, 0, 1).  Fine sample k < K: u = ((float)k + xi_k)/(float)K with xi [n_fine]
   (nullable: 0.5) one draw in [0, 1) per fine sample; t' = ts_i + f*dt_i (always inside a coarse interval, never in a gap between runs);
   dt' = l((k+1)/K) - l(k/K) with l(u) = min(l_i + f*dt_i, l_{i+1}), l(0) = 0 and l(1) = L, so the widths are >= 0 and tile the ray's
   occupied length; p = o + d*t' (the bits of ctx_occ_points); ray_id = r.  The prefix sums are made non-descending by a running maximum
   (the identity on sequential sums).  Every element of a hit ray's fine span is written, nothing for a ray without samples; whatever a
   ray computes it stores only inside [fine_off[r], fine_off[r+1]) and [0, n_fine), at most K entries.  No atomics, one summation order;
   any S <= 2^31 - 64 (a longer ray is taken as empty).  1 <= K <= 4096 (what the compositing backward holds); n = 0 or n_fine = 0 launches nothing (the lists may be null). */
int32_t ctx_resample_packed(const float *weights, const float *ts, const float *dt, const int64_t *ray_off, const float *rays_o,
                            const float *rays_d, int64_t R, int64_t n, int32_t K, const int64_t *fine_off, const float *xi /*nullable*/,
                            int64_t n_fine, int32_t *ray_id_out, float *t_out, float *dt_out, float *pts_out, ctx_stream_t stream);

/* ---- multiresolution hash-grid encoding (instant-ngp; definition: tests/hashgrid_rule.py) ---- */
/* pts [n,3] in the box lo .. hi (host float[3] each, finite, lo < hi) -> emb [n, Lv*F].  table float32 [Lv, T, F], T = 2^log2T, 4 <= log2T <= 22;
   1 <= Lv <= 16, F in {1, 2, 4}, Lv*F <= 64; res int32 [Lv] (host), 1 <= res[l] <= 2^20, computed by the caller in float64.  Per level and
   axis, in binary32 in this order: x = (p - lo)/(hi - lo), x = fminf(fmaxf(x, 0), 1) (NaN -> 0: every index is in range), pos = x*(float)res,
   i = min((int)floorf(pos), res - 1), w = pos - (float)i.  Corner c = cx + 2 cy + 4 cz at node g = i + bit: idx = gx + (res+1)*(gy + (res+1)*gz)
   where (res+1)^3 <= T (dense level), else (gx ^ gy*2654435761u ^ gz*805459861u) & (T - 1) in uint32; weight (sx*sy)*sz with s = bit ? w : 1 - w;
   emb[n, l*F + f] = the left-to-right sum over c ascending of w_c * table[l, idx_c, f], starting from 0.  1 <= n < 2^31. */
int32_t ctx_hashgrid_fwd(const float *pts, int64_t n, const float *table, int32_t Lv, int32_t F, int32_t log2T, const int32_t *res,
                         const float *lo, const float *hi, float *emb, ctx_stream_t stream);
/* The gradient to the table, g_table [Lv, T, F], every element written (the positions' gradient: ctx_hashgrid_bwd_pts).  An integer accumulator, so the result does not
   depend on the order of the adds: m = max|g_emb|, 2^x the smallest power of two above m, E = 62 - ceil(log2(8n)); every contribution
   w_c * g_emb[n, l*F + f] (one float rounding) is scaled by 2^(E-x) in double (exact), rounded to nearest even into int64 and added to
   acc[l, idx_c, f] with a 64-bit integer atomic; g_table = (float)((double)acc * 2^(x-E)).  m = 0 writes zeros; a non-finite g_emb turns all
   of g_table into NaN.  ws: ctx_hashgrid_bwd_ws_bytes(Lv, F, log2T) bytes (-1: refused): the accumulator and the control words.
   stages: bits 1 = zero the accumulator, 2 = reduce m and accumulate, 4 = convert; 7 is the backward, the parts exist to be timed apart. */
int64_t ctx_hashgrid_bwd_ws_bytes(int32_t Lv, int32_t F, int32_t log2T);
int32_t ctx_hashgrid_bwd(const float *pts, int64_t n, const float *g_emb, int32_t Lv, int32_t F, int32_t log2T, const int32_t *res,
                         const float *lo, const float *hi, int32_t stages, void *ws, float *g_table, ctx_stream_t stream);
/* The gradient to the positions, g_pts [n,3], every element written (definition: tests/hashgrid_grad_rule.py).  Per
   point, axis a and level, in binary32 in this order: the axis is active iff x_a = (p_a - lo_a)/(hi_a - lo_a), before the clamp, has
   x_a > 0 && x_a < 1; cell, weights w, corner order and entries t_c are the forward's; s_a = (float)res[l] / (hi_a - lo_a); with o1 < o2 the
   two other axes, per corner c ascending q_c = s_o1 * s_o2 (s_b = bit_b ? w_b : 1 - w_b), term = q_c * t_c[f], d_a[f] = bit_a ? d_a[f] + term :
   d_a[f] - term from 0; gl_a = sum_f g_emb[n, l*F + f] * d_a[f] left to right from 0; g_pts[n, a] = sum_l (gl_a * s_a), levels ascending from 0.
   An inactive axis (NaN, +-inf, on or outside the box faces) gets exactly 0.0f whatever g_emb and the table hold; on an active axis their
   non-finite values propagate.  The derivative is that of the cell the forward assigns the point to: one-sided on cell faces.  First
   order only.  No atomics, one writer per element.  ws: ctx_hashgrid_bwd_pts_ws_bytes(n, Lv) bytes (-1 outside 1 <= n < 2^31, 1 <= Lv <= 16):
   the per-level partials [Lv, n, 3].  The envelope and the refusals are the forward's. */
int64_t ctx_hashgrid_bwd_pts_ws_bytes(int64_t n, int32_t Lv);
int32_t ctx_hashgrid_bwd_pts(const float *pts, int64_t n, const float *table, const float *g_emb, int32_t Lv, int32_t F, int32_t log2T,
                             const int32_t *res, const float *lo, const float *hi, void *ws, float *g_pts /*[n,3]*/, ctx_stream_t stream);

/* ---- the texture field as a 2-D hash grid over the unit UV square (definition: tests/hashtex_rule.py) ---- */
/* n rows -> emb [n, Lv*F].  Exactly one way of naming the rows: uv [n,2] (idx null, grid 0); the whole atlas (uv, idx null; grid >= 2,
   n = grid^2, row r is node r); a texel list (uv null; idx int32 [n], row r is node idx[r] of the grid x grid atlas; an entry outside
   [0, grid^2) gives a zero row).  Any other combination is refused before a launch.  Node i*grid + j has u = j < grid/2 ? (float)j*step :
   fmaf(-(float)(grid-1-j), step, 1.0f) with step = 1.0f/(float)(grid-1), v likewise from i: torch.linspace(0, 1, grid), as ctx_uvmlp_fwd.
   table float32 [Lv, T, F], T = 2^log2T, 4 <= log2T <= 22; 1 <= Lv <= 16, F in {1, 2, 4}, Lv*F <= 64; res int32 [Lv] (host), 1 <= res[l] <= 2^20.
   Per level and axis a (0: u, 1: v), in binary32 in this order: x = fminf(fmaxf(p_a, 0), 1) (NaN -> 0), pos = x*(float)res,
   i = min((int)floorf(pos), res - 1), w = pos - (float)i.  Corner c = cx + 2 cy at node g = i + bit: idx = gx + (res+1)*gy where
   (res+1)^2 <= T (dense level), else (gx ^ gy*2654435761u) & (T - 1) in uint32; weight sx*sy with s = bit ? w : 1 - w;
   emb[r, l*F + f] = the left-to-right sum over c ascending of w_c * table[l, idx_c, f], starting from 0.  1 <= n < 2^31, grid <= 46340. */
int32_t ctx_hashtex_fwd(const float *uv /*nullable*/, const int32_t *idx /*nullable*/, int64_t n, int32_t grid, const float *table, int32_t Lv,
                        int32_t F, int32_t log2T, const int32_t *res, float *emb, ctx_stream_t stream);
/* The gradient to the table, g_table [Lv, T, F], every element written; there is no gradient to uv.  The integer accumulator of
   ctx_hashgrid_bwd with 4 corners: m = max|g_emb| over the rows that take part (all but the out-of-range entries of a list), 2^x the
   smallest power of two above m, E = 62 - ceil(log2(4n)); every w_c * g_emb[r, l*F + f] (one float rounding) is scaled by 2^(E-x) in
   double, rounded to nearest even into int64 and added; g_table = (float)((double)acc * 2^(x-E)).  m = 0 writes zeros; a non-finite
   g_emb turns all of g_table into NaN.  Adjacent lanes of a wave that address one entry add their integers before one atomic is issued
   (CTX_HASHTEX_PRESUM=0, read per call: one atomic per term); the bits are the same.  ws: ctx_hashtex_bwd_ws_bytes(Lv, F, log2T)
   bytes (-1: refused).  stages: bits 1 = zero the accumulator, 2 = reduce m and accumulate, 4 = convert; 7 is the backward. */
int64_t ctx_hashtex_bwd_ws_bytes(int32_t Lv, int32_t F, int32_t log2T);
int32_t ctx_hashtex_bwd(const float *uv /*nullable*/, const int32_t *idx /*nullable*/, int64_t n, int32_t grid, const float *g_emb, int32_t Lv,
                        int32_t F, int32_t log2T, const int32_t *res, int32_t stages, void *ws, float *g_table, ctx_stream_t stream);
/* The texture field's head.  raw [n, C], 1 <= C <= 4; node of row r = r (idx null; then n = plane) or idx[r] (int32 [n], distinct nodes;
   an entry outside [0, plane) is skipped).  tex_chw [C, plane]: tex[c, node] = (tanhf(raw[r,c]) + 1.0f) / 2.0f, the listed nodes only are
   written.  Backward: grad_raw[r,c] = (g_raw_in[r,c], nullable: 0) + grad_tex[c, node] * 0.5f * (1.0f - y*y), y = tanhf(raw[r,c]); every
   element of grad_raw [n, C] is written, the listed nodes only are read.  One writer per element, no atomics.  1 <= n, plane < 2^31. */
int32_t ctx_texture_head_fwd(const float *raw, const int32_t *idx /*nullable*/, int64_t n, int64_t plane, int32_t C, float *tex_chw,
                             ctx_stream_t stream);
int32_t ctx_texture_head_bwd(const float *grad_tex, const float *g_raw_in /*nullable*/, const float *raw, const int32_t *idx /*nullable*/,
                             int64_t n, int64_t plane, int32_t C, float *grad_raw, ctx_stream_t stream);

/* ---- mip-mapped texture_mapping (texmip.hip; definition: tests/mipmap_rule.py; the call site is
   src/models/render.py:135, where the reference samples the atlas with four texels whatever the pixel's footprint) ----
   The atlas tex [C, T, T], 1 <= C <= 4, is level 0; level l has side T >> l; L levels need T % 2^(L-1) == 0 and T >> (L-1) >= 2
   (1 <= L <= 16, 2 <= T <= 16384; anything else is refused).  Everything is binary32, every operation rounding on its own.
   pyr: ctx_mip_levels_bytes(C, T, L) bytes (-1: refused): levels 1 .. L-1, planar [C, T_l, T_l] one after the other, and a 256-byte
   trailer with the pyramid's sticky status.  cov_count: ctx_mip_cov_bytes(T, L) bytes = sum of T_l^2: cov_0 (0 / 1), then n_l.
   ctx_mip_build writes levels 1 .. L-1 (level 0 stays the caller's atlas) and, where cov_count is given, the counts: the children of
   texel (y, x) are a = (2y, 2x), b = (2y, 2x+1), c = (2y+1, 2x), d = (2y+1, 2x+1); cov_0 = coverage != 0 (coverage uint8 [T, T], null:
   everything); n = the covered children, cov_l = n > 0, value = s / (float)n with s = 0 then s = s + child over the covered children in
   that order, 0 where n = 0.  A 32 x 32 tile of a level gives the next five in one launch.  cov_count is required with a coverage plane
   and for L > 6.  ctx_mip_status: 1 after a forward on this pyramid met a face_idx outside its lod table (synchronises the stream). */
int64_t ctx_mip_levels_bytes(int32_t C, int32_t T, int32_t L);
int64_t ctx_mip_cov_bytes(int32_t T, int32_t L);
int32_t ctx_mip_build(const float *tex, const uint8_t *coverage /*nullable*/, int32_t C, int32_t T, int32_t L, float *pyr,
                      uint8_t *cov_count /*nullable*/, ctx_stream_t stream);
int32_t ctx_mip_status(const float *pyr, int32_t C, int32_t T, int32_t L, ctx_stream_t stream);
/* lod [B, F] of the faces fvi [B, F, 3, 2] (NDC, prepare_vertices' face_vertices_image) with uv uva [Bu, F, 3, 2], Bu in {1, B}:
   e = p1 - p0, p2 - p0, d = t1 - t0, t2 - t0; det = e1x*e2y - e2x*e1y (0 or not finite: lod 0); ux = (d1u*e2y - d2u*e1y)/det,
   uy = (d2u*e1x - d1u*e2x)/det, vx, vy likewise; ax = ((2/W)*T)*s_b, ay = ((2/H)*T)*s_b (scale float [B], null: 1);
   r2 = fmaxf((ax*ax)*((ux*ux)+(vx*vx)), (ay*ay)*((uy*uy)+(vy*vy))); !(r2 > 1): 0; infinite: L-1; rho = sqrtf(r2), l0 = ilogbf(rho);
   l0 >= L-1: L-1; else (float)l0 + (ldexpf(rho, -l0) - 1.0f): the blend is linear in the footprint's width. */
int32_t ctx_face_uv_lod(const float *fvi, const float *uva, int32_t Bu, int32_t B, int32_t F, int32_t H, int32_t W, int32_t T, int32_t L,
                        const float *scale /*nullable*/, float *lod, ctx_stream_t stream);
/* out [B, HW, C]: 0 where face_idx [B, HW] (int64) < 0; else lod = fminf(fmaxf(table[b, face_idx], 0), L-1), l0 = (int)lod,
   f = lod - (float)l0, s0 = the bilinear tap of ctx_texture_mapping_fwd at level l0 (side T >> l0, same clamp, same order); f > 0:
   out = s0*(1.0f - f) + s1*f with s1 the tap at level l0 + 1, else out = s0.  One shared atlas.  A face_idx >= F reads nothing: its
   pixel is NaN and the pyramid's status becomes 1 (ctx_mip_status). */
int32_t ctx_texture_mapping_mip_fwd(const float *uv, const float *tex, float *pyr, const float *lod, const int64_t *face_idx, int32_t B, int32_t HW,
                                    int32_t F, int32_t C, int32_t T, int32_t L, float *out, ctx_stream_t stream);
/* grad_tex [C, T, T], every element written.  Stage A: per foreground pixel and channel g = grad_out; f > 0: gl = g*(1.0f - f),
   gh = g*f, else gl = g; the terms w_k*gl (level l0) and w'_k*gh (level l0 + 1) of the taps inside the level go into a 64-bit integer
   pyramid by ctx_hashtex_bwd's scheme (x from max|grad_out| over all of it, E = 62 - ceil(log2(4*B*HW))).  Stage B, one launch:
   A_l = (float)((double)acc_l * 2^(x-E)); an uncovered texel gets 0, else g0 = A_0[y, x], Wt = 1.0f, and for l = 1 .. L-1:
   Wt = Wt / (float)n_l(y >> l, x >> l), g0 = g0 + A_l[y >> l, x >> l]*Wt (cov_count null: everything covered, n = 4).
   An all-zero grad_out gives zeros; a non-finite one, or a face_idx >= F, NaN.  Adjacent lanes that address one texel add their
   integers before one atomic (CTX_TEXMIP_PRESUM=0, read per call, turns that off; same bits).  ws: ..._ws_bytes(C, T, L) bytes. */
int64_t ctx_texture_mapping_mip_bwd_ws_bytes(int32_t C, int32_t T, int32_t L);
int32_t ctx_texture_mapping_mip_bwd(const float *grad_out, const float *uv, const float *lod, const int64_t *face_idx,
                                    const uint8_t *cov_count /*nullable*/, int32_t B, int32_t HW, int32_t F, int32_t C, int32_t T, int32_t L,
                                    void *ws, float *grad_tex, ctx_stream_t stream);

/* ---- the field optimizer: Adam in place (adam.hip; definition: tests/adam_rule.py) ---- */
/* Per element, in binary32, every operation rounding once, in this order (b1, b2, o1 = 1 - b1, o2 = 1 - b2, c1 = lr / (1 - b1^t),
   c2 = 1 / sqrt(1 - b2^t), eps: computed by the caller in float64 and rounded to float; t = 1, 2, ... counts the steps):
     if sparse and g == 0.0f (either sign): p, m, v keep their bits
     else m' = b1*m + o1*g;  v' = b2*v + (o2*g)*g;  d = sqrtf(v')*c2 + eps;  p' = p - (c1*m') / d
   with the correctly rounded division and square root.  A NaN or infinite g is not zero and propagates.  No weight decay, no amsgrad.
   ctx_adam_multi: one launch over n_tensors (1 .. 16) tensors that share the seven floats.  p, m, v, g: host arrays of n_tensors device
   pointers, counts: host int64 [n_tensors], every count >= 1; they travel in the kernel's arguments, nothing is copied to the device.
   Tensors are contiguous float32 and need 4-byte alignment only: a tensor whose four pointers sit at the same offset from a 16-byte
   boundary moves in 16-byte accesses behind a scalar head and before a scalar tail, any other in 4-byte accesses.  p, m, v are updated
   in place, g is read; the tensors must not overlap.  A null pointer, a count < 1 or n_tensors outside [1, 16] is refused before any
   launch.  One writer per element, no atomics. */
int32_t ctx_adam_multi(const void *const *p, const void *const *m, const void *const *v, const void *const *g, const int64_t *counts,
                       int32_t n_tensors, float b1, float b2, float o1, float o2, float c1, float c2, float eps, int32_t sparse,
                       ctx_stream_t stream);
/* The step of a hash table straight from the integer accumulator that stage 2 of ctx_hashgrid_bwd (corners = 8) or ctx_hashtex_bwd
   (corners = 4) left in ws: p, m, v float32 [count], 16-byte aligned, count the table's Lv * T * F elements; ws that call's workspace
   (count int64 sums, then the control words), n that call's n, from which E is derived as there.  Per element g = NaN for a non-finite
   g_emb, 0 for an all-zero one, else (float)((double)acc * 2^(x-E)): the bits of g_table from stage 4; then the rule above.  Every
   accumulator word that was not 0 is set to 0 and the control words are cleared behind the kernel on the stream: the workspace is left
   as stage 1 leaves it.  One writer per element, no atomics. */
int32_t ctx_table_adam(float *p, float *m, float *v, int64_t count, void *ws, int64_t n, int32_t corners, float b1, float b2, float o1,
                       float o2, float c1, float c2, float eps, int32_t sparse, ctx_stream_t stream);

/* ---- per-ray weighted sum on the marched lists ---- */
/* out[r, c] = sum_i weights[i] * values[i, c] over ray r's samples ray_off[r] .. ray_off[r+1]; weights [n], values [n,C], 1 <= C <= 4,
   out [R,C], every element written, zeros for a ray without samples.  One wavefront per ray: lane partials over the chunks in ascending
   order, then one wave sum; no atomics, so two runs give the same bits.  ray_off as ctx_raymarch_packed_fwd; n = 0 zero-fills out (the
   lists may be null) and launches no kernel. */
int32_t ctx_weighted_sum_packed(const float *weights, const float *values, const int64_t *ray_off, int64_t R, int64_t n, int32_t C,
                                float *out, ctx_stream_t stream);

/* ---- baking the 3-D field into the UV atlas (bake.hip) ---- */
/* ctx_texel_rays: texels to rays.  texel_face [T,T] i64 and texel_bary [T,T,3] f32 as ctx_uv_gather_fixed takes them, face_uv [F,3,2] f32
   (vt[ft]), vertices [V,3] f32, faces [F,3] i64, idx int32 [n] a texel list, supersample 1 <= s <= 4, shell h a finite world length > 0.
   -> rays_o [n*s*s,3], rays_d [n*s*s,3], valid u8 [n*s*s]; EVERY element is written.  Row j*s*s + k with k = a + s*b is list entry j,
   column offset a, row offset b.  Per entry, in binary32 in the order written, no contraction:
     p = idx[j] outside [0, T*T), f = texel_face[p] outside [0, F) or a vertex id of faces[f] outside [0, V): the s*s rows get valid = 0
       and zeros;
     e1 = v1 - v0, e2 = v2 - v0, c = e1 x e2 (each component two products and one difference: cx = e1y*e2z - e1z*e2y, ...),
       l2 = (cx*cx + cy*cy) + cz*cz; l2 not finite or not > 0: invalid as above; n = c / sqrtf(l2) (IEEE sqrt and division): the face
       normal of ctx_prepare_vertices' orientation;
     s == 1: (b0, b1, b2) = texel_bary[p] as stored;
     s > 1:  dx = ((float)a + 0.5f)/(float)s - 0.5f, dy likewise from b (texel units along +column and +row);
       x1 = (u1 - u0)*(float)T, x2 = (u2 - u0)*(float)T, y1 = (v0 - v1)*(float)T, y2 = (v0 - v2)*(float)T   (row = (1 - v)*T - 1/2);
       D = x1*y2 - x2*y1;  g1x = y2/D, g1y = -x2/D, g2x = -y1/D, g2y = x1/D;
       b1' = b1 + (dx*g1x + dy*g1y), b2' = b2 + (dx*g2x + dy*g2y), b0' = (1.0f - b1') - b2';
       D not finite or zero: every sub-sample takes the stored (b0, b1, b2).  A sub-sample outside the triangle keeps its extrapolated
       barycentrics (the point stays on the face's plane);
     per axis x = (b0*v0 + b1*v1) + b2*v2, o = x + h*n, d = -n, valid = 1.
   One thread per row, whole-vector stores through LDS, one writer per element, no atomics.  0 <= n, n*s*s < 2^31, 1 <= T <= 46340;
   rays_o and rays_d 16-byte, valid 4-byte, face_uv 8-byte aligned.  n = 0 launches nothing.  A refused call leaves the outputs untouched.
   ctx_bake_resolve: composited sub-samples to atlas sums.  rgb [n*s*s,3] (sum w_i c_i of ctx_raymarch_packed_fwd without white
   background), alpha [n*s*s] (its acc), valid u8 [n*s*s], idx and s as above, acc int64 [4,T,T] in units of 2^-frac_bits, ADDED to.
   Per entry with p = idx[j] inside [0, T*T): over k ascending a sub-sample counts when valid != 0 and its alpha and three colours are
   finite: Sc = Sc + rgb[k,c], Sa = Sa + alpha[k], m += 1 (from 0, left to right).  m == 0: nothing.  Mc = Sc/(float)m, Ma = Sa/(float)m;
   unless Ma >= min_alpha: nothing.  acc[c,p] += rint(Mc * 2^frac_bits), acc[3,p] += rint(Ma * 2^frac_bits): the conversion of
   ctx_uv_scatter_fixed (__float2ll_rn(ldexpf(., frac_bits)); |M| * 2^frac_bits < 2^63), so ctx_fixed_to_float gives acc[:3]/acc[3] the
   un-premultiplied colour and acc[3] > 0 the coverage.  The list must hold DISTINCT texels: one thread per entry does a plain
   read-modify-write, no atomics.  -64 <= frac_bits <= 62. */
int32_t ctx_texel_rays(const int64_t *texel_face, const float *texel_bary, const float *face_uv, const float *vertices, const int64_t *faces,
                       const int32_t *idx, int64_t n, int32_t T, int32_t F, int32_t V, int32_t s, float h, float *rays_o, float *rays_d,
                       uint8_t *valid, ctx_stream_t stream);
int32_t ctx_bake_resolve(const float *rgb, const float *alpha, const uint8_t *valid, const int32_t *idx, int64_t n, int32_t s, int32_t T,
                         float min_alpha, int32_t frac_bits, int64_t *acc, ctx_stream_t stream);

/* ---- the view-dependent field's glue (viewdep.hip; definition: tests/sh_rule.py) ---- */
/* The direction net's input row and the sum of the base and the residual term.  K = deg^2, 1 <= deg <= 4.
   SH(d), d = rays_d[r]: n = sqrtf((d0*d0 + d1*d1) + d2*d2); (x,y,z) = d / n where n > 0 and (0,0,0) where it is not; then, every operation
   rounding on its own in binary32 in the order written (no contraction), the constants being the float64 values rounded once:
      0:  0.28209479177387814
      1: -0.48860251190291987*y      2: 0.48860251190291987*z      3: -0.48860251190291987*x
      4:  1.0925484305920792*(x*y)   5: -1.0925484305920792*(y*z)  6: 0.94617469575755997*(z*z) - 0.31539156525251999
      7: -1.0925484305920792*(x*z)   8: 0.54627421529603959*(x*x - y*y)
      9:  0.59004358992664352*y*(y*y - 3*(x*x))      10: 2.8906114426405538*(x*y)*z
     11:  0.45704579946446572*y*(1 - 5*(z*z))        12: 0.3731763325901154*z*(5*(z*z) - 3)
     13:  0.45704579946446572*x*(1 - 5*(z*z))        14: 1.4453057213202769*z*(x*x - y*y)
     15:  0.59004358992664352*x*(3*(y*y) - x*x)
   of which degree deg is the first K.
   ctx_viewdep_input_fwd: inp[i] = [ emb[i, 0:E] | SH(rays_d[ray_id[i]]) ], inp [n, E+K]; emb [n,E], rays_d [R,3], ray_id int32 [n]; an
     entry of ray_id outside [0, R) reads nothing and takes the direction (0,0,0).
   ctx_viewdep_input_bwd: g_emb[i] = g_inp[i, 0:E]; g_inp [n, E+K], g_emb [n,E].  The directions have no gradient.
   ctx_viewdep_raw_fwd:   raw[i,c] = base[i,c] + res[i,c] for c < 3 (one binary32 add), raw[i,3] = base[i,3]; base, raw [n,4], res [n,3].
   ctx_viewdep_raw_bwd:   g_res[i] = g_raw[i, 0:3]; g_raw [n,4], g_res [n,3].  The gradient to base is g_raw itself.
   Every output element is written; one writer per element, no atomics, no LDS, no host sync.  Tensors are contiguous and need 4-byte
   alignment only: rows move in 16-byte accesses where the widths (E % 4 == 0 and K % 4 == 0; (E+K) % 4 == 0 for the backward) and the
   base pointers (16-byte aligned) allow, in 4-byte accesses otherwise.  1 <= n < 2^31, R >= 1, 1 <= E, E + K <= 64.  Outside that, or with
   a null pointer, a call returns CTX_E_ARG before any launch and leaves the outputs untouched. */
int32_t ctx_viewdep_input_fwd(const float *emb, const float *rays_d, const int32_t *ray_id, int64_t n, int64_t R, int32_t E, int32_t deg,
                              float *inp, ctx_stream_t stream);
int32_t ctx_viewdep_input_bwd(const float *g_inp, int64_t n, int32_t E, int32_t deg, float *g_emb, ctx_stream_t stream);
int32_t ctx_viewdep_raw_fwd(const float *base, const float *res, int64_t n, float *raw, ctx_stream_t stream);
int32_t ctx_viewdep_raw_bwd(const float *g_raw, int64_t n, float *g_res, ctx_stream_t stream);

/* ---- UNet denoise engine (src/stable_diffusion_depth.py:422-430,514) ----------------------- */
typedef struct ctx_unet ctx_unet_t;
typedef struct {
    int32_t in_channels, out_channels;
    int32_t n_levels;            /* <= 4 */
    int32_t block_out_channels[4];
    int32_t heads[4];
    int32_t down_attn[4], up_attn[4];
    int32_t layers_per_block;
    int32_t cross_attention_dim;
    int32_t groups;
    float norm_eps;
} ctx_unet_config_t;

ctx_unet_t *ctx_unet_create(const ctx_unet_config_t *cfg);
void ctx_unet_destroy(ctx_unet_t *u);
/* Parameter table in diffusers state_dict naming ("down_blocks.0.resnets.0.conv1.weight", ...). */
int32_t ctx_unet_param_count(const ctx_unet_t *u);
const char *ctx_unet_param_name(const ctx_unet_t *u, int32_t i);
int32_t ctx_unet_param_shape(const ctx_unet_t *u, int32_t i, int64_t shape4[4]); /* returns ndim */
int64_t ctx_unet_weight_bytes(const ctx_unet_t *u);
int64_t ctx_unet_workspace_bytes(const ctx_unet_t *u, int32_t B, int32_t H, int32_t W, int32_t ctx_len);
/* Bind caller-allocated blobs (256-B aligned). */
int32_t ctx_unet_bind(ctx_unet_t *u, void *weights, void *workspace, int64_t workspace_bytes);
/* The derived blob: packs that are functions of parameters and live outside the weight blob (the phase packs of the upsamplers'
   convolutions, ctx_conv3x3_phase_f16).  ctx_unet_derived_bytes: its size (0: this engine derives nothing, e.g. a ControlNet);
   ctx_unet_bind_derived: bind it (256-B aligned, >= that size; NULL unbinds).  Optional: with none bound the upsamplers run as
   nine-tap convolutions over the x2 grid.  ctx_unet_set_param fills it for the parameters set while it is bound, so bind it
   before loading; engines over the same weight blob may share one. */
int64_t ctx_unet_derived_bytes(const ctx_unet_t *u);
int32_t ctx_unet_bind_derived(ctx_unet_t *u, void *derived, int64_t bytes);
/* Convert + repack parameter i from fp32 [diffusers layout] into the fp16 weight blob. */
int32_t ctx_unet_set_param(ctx_unet_t *u, int32_t i, const float *src, ctx_stream_t stream);
/* sample[B,Cin,H,W] f32 NCHW, timestep: device float[1] (graph-replay friendly), ctx[B,L,D] f32
   -> out[B,Cout,H,W] f32 NCHW.  Computes in fp16 with fp32 accumulation/statistics. */
int32_t ctx_unet_forward(ctx_unet_t *u, const float *sample, const float *timestep, const float *ctx,
                         int32_t B, int32_t H, int32_t W, int32_t ctx_len, float *out, ctx_stream_t stream);
/* Reference-only self-attention (Zero123++'s RefOnlyNoisedUNet / ReferenceOnlyAttnProc; the reference keeps the spec in
   src/zero123plus.py:127-237 and drives it from src/training/trainer.py:644-907).
   mode 1 ('w'): an ordinary forward over the noised condition latent that also parks every attn1 input (the LayerNorm-1 output,
                 [B, tokens, C] fp16 per layer) in `bank` (ctx_unet_ref_bank_bytes(u, B, H, W) bytes).
   mode 2 ('r'): forward whose attn1 layers use [own tokens ; parked tokens] as the K/V source for the batch rows >= ref_row0
                 (is_cfg_guidance => ref_row0 = 1: the unconditional row attends without the reference); row b reads the parked
                 row b - ref_row0, so the 'w' pass must have had B - ref_row0 rows.  The bank layout is private to the engine
                 that wrote it.  Workspace: ctx_unet_workspace_bytes_ref (for mode 2 call it after the 'w' pass). */
int64_t ctx_unet_ref_bank_bytes(const ctx_unet_t *u, int32_t B, int32_t H, int32_t W);
int64_t ctx_unet_workspace_bytes_ref(const ctx_unet_t *u, int32_t B, int32_t H, int32_t W, int32_t ctx_len, int32_t mode,
                                     int32_t ref_row0);
int32_t ctx_unet_forward_ref(ctx_unet_t *u, const float *sample, const float *timestep, const float *ctx,
                             int32_t B, int32_t H, int32_t W, int32_t ctx_len, int32_t mode, void *bank, int32_t ref_row0,
                             float *out, ctx_stream_t stream);
/* ControlNet (diffusers ControlNetModel.from_unet; Zero123++'s DepthControlUNet, spec in src/zero123plus.py:260-298, loaded at
   src/training/trainer.py:302-304): an engine with the UNet's conv_in / time embedding / down blocks / mid block, the
   conditioning-image embedding (channels 16-32-96-256, three stride-2 steps: the image is 8x the latent grid) and the 1x1 zero
   convolutions.  ctx_controlnet_forward writes the residuals (one per skip tensor, then the mid block; fp16, engine layout,
   ctx_controlnet_residual_bytes) — UNSCALED; ctx_unet_set_residuals hands them to a UNet engine of the same configuration, which
   adds `scale` x residual to its skip tensors and mid-block output in the following forwards (NULL switches it off).
   Parameter names are diffusers' ControlNetModel state_dict keys; the size / bind / set_param / destroy calls are ctx_unet_*. */
ctx_unet_t *ctx_controlnet_create(const ctx_unet_config_t *cfg, int32_t cond_channels);
int64_t ctx_controlnet_residual_bytes(const ctx_unet_t *cn, int32_t B, int32_t H, int32_t W);
/* cond_cache (nullable; ctx_controlnet_cond_cache_bytes): holds the output of the embedding's few-channel layers, which depends
   only on the conditioning image; pass cache_valid = 1 while the image is unchanged (every denoise step after the first). */
int64_t ctx_controlnet_cond_cache_bytes(const ctx_unet_t *cn, int32_t B, int32_t H, int32_t W);
int32_t ctx_controlnet_forward(ctx_unet_t *cn, const float *sample, const float *timestep, const float *ctx,
                               const float *cond /*[B,cond_channels,8H,8W] f32 NCHW*/, void *cond_cache, int32_t cache_valid,
                               int32_t B, int32_t H, int32_t W, int32_t ctx_len, void *residuals, ctx_stream_t stream);
int32_t ctx_unet_set_residuals(ctx_unet_t *u, const void *residuals /*nullable*/, float scale);
/* Per-kernel accounting of the last forward: number of launches and algorithmic FLOPs by class
   (0 gemm/conv MFMA, 1 attention MFMA, 2 other). */
/* Precision experiment: on != 0 keeps the UNet's residual stream (block outputs, skip tensors, the transformer blocks' running
   sums) in fp32; operands, weights and everything else stay as they are.  Plain forward only (not the ControlNet / reference-only
   passes).  The workspace grows: query ctx_unet_workspace_bytes again after switching. */
int32_t ctx_unet_set_residual_fp32(ctx_unet_t *u, int32_t on);
int32_t ctx_unet_stats(const ctx_unet_t *u, int32_t klass, int64_t *launches, double *flops);
/* GroupNorms of the last forward that ran without a statistics launch on partials from their producer's epilogue, and GroupNorms
   that read a split-K convolution's slabs in place of a reduced tensor (CTX_GN_EPI; no reference counterpart). */
int32_t ctx_unet_gn_epilogue_counts(const ctx_unet_t *u, int64_t *from_producer, int64_t *from_slabs);
/* Measurement aid (tools/precision_attribution.py; no reference counterpart): buf (fp16 device memory of `capacity` elements, NULL =
   off) receives a copy of every block's output (fp16 NHWC [rows, channels]) of the following plain forwards, in execution order:
   conv_in; per down level resnet (, transformer) x layers, downsampler; mid resnet, transformer, resnet; per up level resnet
   (, transformer) x (layers + 1), upsampler.  ctx_unet_tap_count / ctx_unet_tap_info describe the last forward's taps. */
int32_t ctx_unet_set_taps(ctx_unet_t *u, void *buf, int64_t capacity);
int32_t ctx_unet_tap_count(const ctx_unet_t *u);
int32_t ctx_unet_tap_info(const ctx_unet_t *u, int32_t i, int64_t *offset, int32_t *rows, int32_t *channels);

/* ---- VAE decoder (src/stable_diffusion_depth.py:976-990 decode_latents -> diffusers AutoencoderKL.decode) ---------- */
typedef struct ctx_vae ctx_vae_t;
typedef struct {
    int32_t latent_channels, out_channels;
    int32_t n_levels;                 /* <= 4 */
    int32_t block_out_channels[4];    /* encoder order, e.g. 128,256,512,512 */
    int32_t layers_per_block;
    int32_t groups;
} ctx_vae_config_t;
ctx_vae_t *ctx_vae_create(const ctx_vae_config_t *cfg);
void ctx_vae_destroy(ctx_vae_t *v);
int32_t ctx_vae_param_count(const ctx_vae_t *v);
const char *ctx_vae_param_name(const ctx_vae_t *v, int32_t i);      /* diffusers AutoencoderKL state_dict keys */
int32_t ctx_vae_param_shape(const ctx_vae_t *v, int32_t i, int64_t shape4[4]);
int64_t ctx_vae_weight_bytes(const ctx_vae_t *v);
int64_t ctx_vae_workspace_bytes(const ctx_vae_t *v, int32_t B, int32_t H, int32_t W);
int32_t ctx_vae_bind(ctx_vae_t *v, void *weights, void *workspace, int64_t workspace_bytes);
/* the derived blob of the decoder's upsamplers, as ctx_unet_derived_bytes / ctx_unet_bind_derived */
int64_t ctx_vae_derived_bytes(const ctx_vae_t *v);
int32_t ctx_vae_bind_derived(ctx_vae_t *v, void *derived, int64_t bytes);
int32_t ctx_vae_set_param(ctx_vae_t *v, int32_t i, const float *src, ctx_stream_t stream);
/* latents [B,L,H,W] f32 (already divided by the 0.18215 scaling factor) -> image [B,3,8H,8W] f32 */
int32_t ctx_vae_decode(ctx_vae_t *v, const float *latents, int32_t B, int32_t H, int32_t W, float *image, ctx_stream_t stream);
/* AutoencoderKL.encode behind StableDiffusion.encode_imgs (src/stable_diffusion_depth.py:971-975): image f32 NCHW
   [B,3,H,W] (the caller applies 2x-1) -> moments f32 NCHW [B, 2*latent_channels, H/8, W/8] = quant_conv(Encoder(x)):
   mean | logvar of DiagonalGaussianDistribution; `.sample()` (mean + exp(0.5 clamp(logvar,-30,20)) * randn) and the
   0.18215 factor stay with the caller so that the noise comes from the caller's RNG stream.
   The parameter table lists post_quant_conv + decoder first (ctx_vae_decoder_param_count entries), then encoder + quant_conv. */
int32_t ctx_vae_decoder_param_count(const ctx_vae_t *v);
int64_t ctx_vae_encode_workspace_bytes(const ctx_vae_t *v, int32_t B, int32_t H, int32_t W);
int32_t ctx_vae_encode(ctx_vae_t *v, const float *image, int32_t B, int32_t H, int32_t W, float *moments, ctx_stream_t stream);
double ctx_vae_flops(const ctx_vae_t *v);     /* algorithmic FLOPs of the last decode / encode / dry run */
/* Autograd of `vae.encode` in the reference's SDS loop (`loss.backward()` reaches the texture through
   `vae.encode(rendered_grid_clean)`, src/training/trainer.py:732, 866; torch autograd over diffusers' Encoder there).
   ctx_vae_encode_train = ctx_vae_encode that keeps what the backward needs (every GroupNorm input and the attention's q|k|v)
   in the bound workspace; ctx_vae_encode_bwd consumes that tape once: grad_moments f32 NCHW [B, 2L, H/8, W/8] ->
   grad_image f32 NCHW [B,3,H,W] (input gradients only: the VAE's parameters are frozen on this path).  Internally the
   gradients are fp16 times `gscale` (choose it so that gscale * max|grad_moments| is O(1..100)); the result is exact in gscale.
   Any other call on the handle between the two drops the tape (ctx_vae_encode_bwd then fails with CTX_E_ARG). */
int64_t ctx_vae_encode_train_workspace_bytes(const ctx_vae_t *v, int32_t B, int32_t H, int32_t W);
int32_t ctx_vae_encode_train(ctx_vae_t *v, const float *image, int32_t B, int32_t H, int32_t W, float *moments, ctx_stream_t stream);
int32_t ctx_vae_encode_bwd(ctx_vae_t *v, const float *grad_moments, float gscale, float *grad_image, ctx_stream_t stream);

/* Building blocks, exported for unit parity tests (fp16 tensors passed as uint16 bit patterns). */
/* C[M,N] = A[M,K] @ Wt[N,K]^T (+bias[N]) (+residual[M,N]); K%64==0, N%8==0. */
int32_t ctx_gemm_f16(const void *A, const void *Wt, const void *bias, const void *residual,
                     int32_t M, int32_t N, int32_t K, void *C, ctx_stream_t stream);
/* x[B,H,W,Cin] (NHWC f16) * w[Cout,3,3,Cin] stride s pad 1 (+bias) (+rowbias[B,Cout]) (+res) -> [B,Ho,Wo,Cout];
   upsample=1: nearest x2 of x first (Upsample2D). */
int32_t ctx_conv3x3_f16(const void *x, const void *w, const void *bias, const void *rowbias,
                        const void *residual, int32_t B, int32_t H, int32_t W, int32_t Cin,
                        int32_t Cout, int32_t stride, int32_t upsample, void *y, ctx_stream_t stream);
/* The same stride-1 convolution with up to two K segments behind its 9 Cin part: centre-tap (1x1) products over tensors xa / xb
   [B,H,W,Ca / Cb] of the same pixel grid, weights wa / wb [Cout] rows of Ca / Cb at row strides ldwa / ldwb (xb NULL: one segment):
   y = conv3x3(x; w) + xa wa^T + xb wb^T + bias + bias2 (+rowbias) (+residual), summed in fp32 and rounded once.  This is
   ResnetBlock2D's conv_shortcut(input_tensor) + conv2(hidden_states) under diffusers' UNet2DConditionModel (reference call site
   src/stable_diffusion_depth.py:422-423) with the up blocks' torch.cat([hidden_states, skip]) read in place.  Channel counts in
   multiples of 32.  splitk: 1 none, > 1 that many K slices, < 0 the engine's plan for the 3x3 part; part: splitk * M * Cout floats
   (32 * M * Cout with splitk < 0) or NULL (no split). */
int32_t ctx_conv3x3_seg_f16(const void *x, const void *w, const void *bias, const void *bias2, const void *rowbias,
                            const void *residual, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                            const void *xa, const void *wa, int32_t Ca, int32_t ldwa, const void *xb, const void *wb,
                            int32_t Cb, int32_t ldwb, void *part, int32_t splitk, void *y, ctx_stream_t stream);
/* The resnet's conv1 as the UNet engine runs it in front of norm2 (ResnetBlock2D.forward: conv1, + time embedding, norm2, under
   diffusers' UNet2DConditionModel; reference call site src/stable_diffusion_depth.py:422-423): stride-1 conv3x3 + bias + bias2
   (+rowbias) (+residual), and one of
     gn_part != NULL: the kernel that rounds the output also writes the (sum, sum of squares) partials of GroupNorm(groups) over it
       into gn_part (ctx_groupnorm_ws_bytes(B, groups)); *slots = slots per sample written, for ctx_groupnorm_apply_f16, or 0 when
       the launched kernel declined the request (y is the same either way);
     keep_slabs != 0 (needs splitk > 1): the split-K reduce is not launched; y is not written (may be NULL) and part holds the splitk
       fp32 slabs [B*H*W][Cout] for ctx_groupnorm_slabs_f16 (*slots, when given, = the split factor that ran).
   splitk and part as ctx_conv3x3_seg_f16 (< 0: the engine's plan, kernel and split).  Honours ctx_gemm_tune. */
int32_t ctx_conv3x3_gn_f16(const void *x, const void *w, const void *bias, const void *bias2, const void *rowbias,
                           const void *residual, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, void *part,
                           int32_t splitk, int32_t keep_slabs, int32_t groups, void *gn_part, int32_t *slots, void *y,
                           ctx_stream_t stream);
/* The kernel that the last GEMM / convolution dispatch launched, in ctx_gemm_tune's terms (use8 0: gemm.hip's tile *tile): lets a test
   of the cuBLAS / cuDNN replacements under UNet2DConditionModel (reference call site src/stable_diffusion_depth.py:422-423) see
   that a forced kernel ran, or that the call fell through to another one when it declined. */
void ctx_gemm_last_kernel(int32_t *tile, int32_t *use8);
/* ---- test-only seams of the VAE encoder's training path (ctx_vae_encode_train / ctx_vae_encode_bwd: autograd of `vae.encode`,
   src/training/trainer.py:732, 866).  Each validates and then launches what the engine launches; tests/vae_train_rule.py holds the
   float64 references and the error bounds.  Not for product code. ---- */
/* A 3x3 convolution in any geometry the engines use, GemmArgs filled as the engines fill them: Ho = ((H << upsample) - 1) / stride + 1.
   poff: input-coordinate offset, 0 = symmetric padding 1; 1 = padding on the bottom / right only (diffusers' Downsample2D of the VAE:
   F.pad(x, (0,1,0,1)) and a stride-2 conv; needs even H and W).  zins = 1 (needs upsample 1, stride 1): the x2 grid is zero-inserted,
   not nearest-upsampled; with poff -1 and the pack of ctx_pack_conv3_dgrad_f16 this is that downsampler's input gradient.
   w [Cout][3][3][Cin]; splitk / part as ctx_conv3x3_seg_f16 (part NULL: no split; splitk <= min(32, 9 Cin / 64)).  Honours
   ctx_gemm_tune.  CTX_E_ARG, nothing launched: zins without upsample 1 and stride 1, poff outside -1 .. 1, poff 1 with odd H or W. */
int32_t ctx_conv3x3_geom_f16(const void *x, const void *w, const void *bias, const void *residual, int32_t B, int32_t H, int32_t W,
                             int32_t Cin, int32_t Cout, int32_t stride, int32_t upsample, int32_t poff, int32_t zins, void *part,
                             int32_t splitk, void *y, ctx_stream_t stream);
/* The phase form of the upsampling convolution: nearest x2 upsample of x [B,H,W,Cin] followed by a pad-1 3x3 convolution, computed
   as four 2x2 convolutions over x, one per output parity (a, b): y[n, 2i+a, 2j+b, o] = bias[o] + sum_{u,v,c} x[n, i+a-1+u, j+b-1+v, c]
   wp[a,b][o][u][v][c] (x reads 0 outside the grid); 4 / 9 of the nine-tap form's multiplies.
   ctx_pack_conv3_phase_f16: w f32 [Cout,Cin,3,3] -> wp f16 [4 phases (0,0),(0,1),(1,0),(1,1)][Cout][2][2][Cin]; tap (u, v) of phase
     (a, b) is the sum over ky in R(a,u), kx in R(b,v), R(0,0) = {0}, R(0,1) = {1,2}, R(1,0) = {0,1}, R(1,1) = {2}, in fp32, added
     left to right with ky ascending, then kx ascending, rounded once.
   ctx_conv3x3_phase_f16: y f16 [B,2H,2W,Cout]; Cin % 64 == 0, Cout % 8 == 0.  Bias only: a rowbias, a residual or a NULL pack is
     CTX_E_ARG with nothing launched.  splitk / part as ctx_conv3x3_geom_f16 (splitk <= min(32, 4 Cin / 64)).  Honours ctx_gemm_tune;
     a forced kernel that does not implement the form (gemm8.hip, conv_halo.hip) fails with CTX_E_ARG. */
int32_t ctx_pack_conv3_phase_f16(const float *src, int32_t Cout, int32_t Cin, void *dst, ctx_stream_t stream);
int32_t ctx_conv3x3_phase_f16(const void *x, const void *wp, const void *bias, const void *rowbias, const void *residual, int32_t B,
                              int32_t H, int32_t W, int32_t Cin, int32_t Cout, void *part, int32_t splitk, void *y, ctx_stream_t stream);
/* The weight packs of the data gradients, as ctx_vae_set_param writes them next to the forward packs.
   conv: src f32 [Cout,Cin,3,3] -> dst f16 [Cin][t' = 3 (2 - ky) + (2 - kx)][pad], zero in the columns Cout .. pad (pad >= Cout): the
   weights [N = Cin][3][3][K-channels = pad] of the convolution that maps a cotangent of pad channels to the input gradient.
   matrix: src f32 [out,in] -> dst f16 [in][ld] at columns col .. col + out (the rest of dst is not written). */
int32_t ctx_pack_conv3_dgrad_f16(const float *src, int32_t Cout, int32_t Cin, int32_t pad, void *dst, ctx_stream_t stream);
int32_t ctx_pack_mat_dgrad_f16(const float *src, int32_t out, int32_t in, int32_t ld, int32_t col, void *dst, ctx_stream_t stream);
/* GroupNorm(+SiLU) backward, input gradient only, NHWC f16: dx = d loss / d x (+ add, nullable) of y = GroupNorm(x) (SiLU behind it
   when silu) for the cotangent dy.  Deterministic.  ws: ctx_groupnorm_bwd_ws_bytes(B, groups).  C % 8 == 0, 256 % (C / 8) == 0,
   C % groups == 0, else CTX_E_ARG. */
int64_t ctx_groupnorm_bwd_ws_bytes(int32_t B, int32_t groups);
int32_t ctx_groupnorm_bwd_f16(const void *x, const void *dy, const void *gamma, const void *beta, const void *add, int32_t B, int32_t HW,
                              int32_t C, int32_t groups, float eps, int32_t silu, void *dx, void *ws, ctx_stream_t stream);
/* The row kernels of the mid-block attention: p = softmax(s * scale) over rows of n f16 scores, and its backward
   dS = P * (dP - sum_j P_j dP_j) * scale.  n % 8 == 0. */
int32_t ctx_softmax_rows_f16(const void *s, int32_t rows, int32_t n, float scale, void *p, ctx_stream_t stream);
int32_t ctx_softmax_bwd_rows_f16(const void *P, const void *dP, int32_t rows, int32_t n, float scale, void *dS, ctx_stream_t stream);
/* The two ends of the encoder backward.  quant_conv: g f32 NCHW [B,C,HW], w f16 [C,C] -> d f16 NHWC [B*HW,64] =
   gscale * sum_o g_o w[o][c], zero in the channels C .. 64 (C <= 16).  conv_in: dy f16 NHWC [B,H,W,C], w_pack f16 [C][3][3][8] (the
   forward pack, image channels padded to 8) -> dimg f32 NCHW [B,Cimg,H,W] = inv_gscale * the input gradient (Cimg <= 4, C <= 448). */
int32_t ctx_quant_bwd_f16(const float *g, const void *w, int32_t B, int32_t C, int64_t HW, float gscale, void *d, ctx_stream_t stream);
int32_t ctx_conv_in_bwd_f16(const void *dy, const void *w_pack, int32_t B, int32_t H, int32_t W, int32_t C, int32_t Cimg, float inv_gscale,
                            float *dimg, ctx_stream_t stream);
/* ---- test-only seams of the engines' small ops: what the UNet / ControlNet / VAE graphs launch besides GEMMs, attention and norms
   (diffusers' UNet2DConditionModel, ControlNetModel and AutoencoderKL under src/stable_diffusion_depth.py:422-423 and
   src/training/trainer.py:732).  Each goes through the host function the engine calls: same checks, same grid, same template
   choice.  A refused call returns CTX_E_ARG and launches nothing.  tests/engine_ops_rule.py holds the float64 references and the
   error bounds.  Not for product code. ---- */
/* conv_in: x f32 NCHW [B,Cin,H,W], each value rounded to f16 on load; w_pack f16 [Cout][3][3][8] (Cin <= 8) or [Cout][3][3][16], the
   channels Cin .. 8 | 16 of a row finite (the pack writes zeros; some are multiplied by a zero input); bias f16 [Cout] -> y f16 NHWC [B,H,W,Cout]; 3x3, padding 1, fp32 sum (bias first).
   1 <= Cin <= 16, Cout % 8 == 0, and the weight slice of Cout / 16 features must fit the LDS (Cout <= 1152 at Cin <= 8). */
int32_t ctx_conv_in_f16(const float *x, const void *w_pack, const void *bias, int32_t B, int32_t Cin, int32_t H, int32_t W, int32_t Cout,
                        void *y, ctx_stream_t stream);
/* conv_out: x f16 NHWC [B,H,W,C], w f16 [Cout][3][3][C], bias f16 [Cout] -> out f32 NCHW [B,Cout,H,W]; 3x3, padding 1, fp32 sum over the
   64 lanes of a wave, bias last.  1 <= Cout <= 4, C % 8 == 0, 8 <= C <= 680, Cout * C <= 3640. */
int32_t ctx_conv_out_f16(const void *x, const void *w, const void *bias, int32_t B, int32_t H, int32_t W, int32_t C, int32_t Cout,
                         float *out, ctx_stream_t stream);
/* GEMV of the time-embedding MLP: out[b][n] = act(sum_k in(x[b][k]) w[n][k] + bias[n]), f16 in and out, fp32 sum; in = SiLU when
   silu_in, act = SiLU when silu_out; bias nullable.  Bm >= 1 (four rows per pass over w), N >= 1, K % 8 == 0, K >= 8. */
int32_t ctx_gemv_f16(const void *x, const void *w, const void *bias, int32_t Bm, int32_t N, int32_t K, int32_t silu_in, int32_t silu_out,
                     void *out, ctx_stream_t stream);
/* diffusers' get_timestep_embedding(flip_sin_to_cos=True, freq_shift=0) of the ONE timestep t[0] (device f32), written to each of
   the B rows: out f16 [B][dim] = [cos(t f_i) | sin(t f_i)], f_i = exp(-ln(10000) i / (dim / 2)).  dim even, >= 2. */
int32_t ctx_time_embed_f16(const float *t, int32_t B, int32_t dim, void *out, ctx_stream_t stream);
/* Per-head transpose: v f16 [B,S,ld] (head h at columns 64 h .. 64 h + 64; pass v + column offset for a slice of a wider row) ->
   vt f16 [B,heads,64,Sp], keys contiguous, exactly zero in the keys S .. Sp.  Sp % 8 == 0, Sp >= S, ld % 8 == 0, ld >= 64 heads. */
int32_t ctx_transpose_v_f16(const void *v, int32_t B, int32_t S, int32_t ld, int32_t heads, int32_t Sp, void *vt, ctx_stream_t stream);
/* Channel concat of NHWC rows: y[m] = [a[m] (Ca) | b[m] (Cb)] for m < M; f16 with Ca, Cb % 8 == 0; f32 (the fp32 residual stream: the
   same kernel, a float counted as two halves) with Ca, Cb % 4 == 0. */
int32_t ctx_concat_f16(const void *a, const void *b, int64_t M, int32_t Ca, int32_t Cb, void *y, ctx_stream_t stream);
int32_t ctx_concat_f32(const float *a, const float *b, int64_t M, int32_t Ca, int32_t Cb, float *y, ctx_stream_t stream);
/* The converters: y = (f16)x, round to nearest even, n >= 1; y = (f32)x, n % 8 == 0. */
int32_t ctx_f32_to_f16(const float *x, int64_t n, void *y, ctx_stream_t stream);
int32_t ctx_f16_to_f32(const void *x, int64_t n, float *y, ctx_stream_t stream);
/* ControlNet's conditioning-embedding convolution: 3x3, padding 1, stride 1 | 2 (Ho = (H - 1) / stride + 1); input either x32 f32 NCHW
   [B,Cin,H,W] (rounded to f16 on load) or x16 f16 NHWC [B,H,W,Cin], exactly one of them non-null; w f16 [Cout][3][3][Cin], bias f16
   [Cout] -> y f16 NHWC [B,Ho,Wo,Cout] = (f16)act(sum), act = SiLU when silu.  Cout % 8 == 0. */
int32_t ctx_conv_small_f16(const float *x32, const void *x16, const void *w, const void *bias, int32_t B, int32_t H, int32_t W, int32_t Cin,
                           int32_t Cout, int32_t stride, int32_t silu, void *y, ctx_stream_t stream);
/* ControlNet's residual injection: dst = (f16)(dst + scale * src) over n f16, fp32 arithmetic.  n % 8 == 0, n >= 8. */
int32_t ctx_add_scaled_f16(void *dst, const void *src, float scale, int64_t n, ctx_stream_t stream);
/* The VAE's 1x1 convolutions over a few channels: y f32 NCHW [B,C,HW] = w[o][c] x + b[o], w f16 [C][C], b f16 [C], fp32 sum (bias
   first).  nhwc16 0: x f32 NCHW [B,C,HW], C <= 8 (post_quant_conv); 1: x f16 NHWC [B,HW,C], C <= 16 (quant_conv). */
int32_t ctx_pointwise_f32(const void *x, const void *w, const void *b, int32_t B, int32_t C, int64_t HW, int32_t nhwc16, float *y,
                          ctx_stream_t stream);
/* The forward weight packs of ctx_unet_set_param / ctx_vae_set_param, src f32 -> dst f16 (round to nearest even).  kind
   0 copy: a * max(b, 1) elements in order;
   1 conv3: [a = Cout, b = Cin, 3, 3] -> [Cout][ky][kx][Cin];
   2 conv_in: the same with the rows padded to 8 (Cin <= 8) or 16 channels, the padding exactly zero; 1 <= Cin <= 16;
   3 GEGLU weight [2 a, b] (a = C4 value rows, then C4 gate rows; b = K) and 4 GEGLU bias [2 a]: packed row p takes source row
     32 (p / 64) + p % 64 when p % 64 < 32 (a value row) and C4 + 32 (p / 64) + p % 64 - 32 otherwise (its gate row): blocks of 32
     value rows and their 32 gate rows alternate.  C4 % 32 == 0. */
int32_t ctx_pack_fwd_f16(const float *src, int32_t kind, int32_t a, int32_t b, void *dst, ctx_stream_t stream);
/* GroupNorm(+SiLU) over NHWC f16; stats_ws: ctx_groupnorm_ws_bytes(B, groups). */
int64_t ctx_groupnorm_ws_bytes(int32_t B, int32_t groups);
int32_t ctx_groupnorm_f16(const void *x, const void *gamma, const void *beta, int32_t B, int32_t HW,
                          int32_t C, int32_t groups, float eps, int32_t silu, void *y, void *stats_ws,
                          ctx_stream_t stream);
/* GroupNorm(+SiLU) of the channel concatenation [xa ; xb] (xa [B,HW,Ca], xb [B,HW,C-Ca], Ca % 8 == 0) read in place: norm1 of
   the up blocks' ResnetBlock2D over torch.cat([hidden_states, res_hidden_states], dim=1) under diffusers' UNet2DConditionModel
   (reference call site src/stable_diffusion_depth.py:422-423).  Bit-identical to ctx_groupnorm_f16 of the concatenated tensor. */
int32_t ctx_groupnorm2_f16(const void *xa, const void *xb, int32_t Ca, const void *gamma, const void *beta, int32_t B,
                           int32_t HW, int32_t C, int32_t groups, float eps, int32_t silu, void *y, void *stats_ws,
                           ctx_stream_t stream);
/* The second pass of GroupNorm(+SiLU) alone, on partials part[B][slots][groups][2] that the producer of x wrote
   (ctx_conv3x3_gn_f16 with gn_part); same reference call site as ctx_groupnorm2_f16. */
int32_t ctx_groupnorm_apply_f16(const void *x, const void *part, int32_t slots, const void *gamma, const void *beta, int32_t B,
                                int32_t HW, int32_t C, int32_t groups, float eps, int32_t silu, void *y, ctx_stream_t stream);
/* One-kernel GroupNorm(+SiLU) of a split-K convolution's unreduced output (ctx_conv3x3_gn_f16 with keep_slabs): the value it
   normalises is (f16)(sum_s slab_s + bias + bias2 + rowbias[b]) in the reduce kernel's operand order, so the result is bit-identical
   to the reduce followed by ctx_groupnorm_f16.  The shape must take the one-kernel form (C / groups a multiple of 8, small HW);
   same reference call site as ctx_groupnorm2_f16. */
int32_t ctx_groupnorm_slabs_f16(const void *part, int32_t splitk, const void *bias, const void *bias2, const void *rowbias,
                                int32_t ldrb, const void *gamma, const void *beta, int32_t B, int32_t HW, int32_t C,
                                int32_t groups, float eps, int32_t silu, void *y, ctx_stream_t stream);
int32_t ctx_layernorm_f16(const void *x, const void *gamma, const void *beta, int64_t rows, int32_t C,
                          float eps, void *y, ctx_stream_t stream);
/* ---- test-only seams of the norm kernels (GroupNorm / LayerNorm of diffusers' UNet2DConditionModel and AutoencoderKL under
   src/stable_diffusion_depth.py:422-423).  tests/norm_rule.py holds the float64 references and the error bound.  Not for product code. ----
   The launch plans, host only: what ctx_groupnorm_f16 / ctx_groupnorm2_f16 (Ca != 0: two sources, the first Ca channels wide) /
   ctx_groupnorm_f32in_f16 (x32) would launch for a shape, from the function the launcher itself calls; CTX_E_ARG where it refuses.
   groupnorm out[12]: one (1 the one-kernel form, 0 the two-pass form), plf, thr (one-kernel: pixel lanes, block), PL, threads, NS,
     na, lds (pass 1: pixel lanes, block, splits, fold slices, dynamic LDS bytes), apl, athreads, nb (pass 2, also
     ctx_groupnorm_apply_f16's: pixel lanes, block, blocks per sample at 6 pixels per lane), the LDS bytes pass 1 opts into.
   layernorm out[4]: g8 (1: 8 lanes per row, else a wave per R rows), KC (16-byte chunks per lane per row), R, blocks of 256 threads. */
int32_t ctx_groupnorm_plan(int32_t B, int32_t HW, int32_t C, int32_t groups, int32_t x32, int32_t Ca, int32_t *out);
int32_t ctx_layernorm_plan(int64_t rows, int32_t C, int32_t x32, int64_t *out);
/* ctx_groupnorm_f16 and ctx_layernorm_f16 with x in fp32 (the kernels behind ctx_unet_set_residual_fp32); y stays f16. */
int32_t ctx_groupnorm_f32in_f16(const float *x, const void *gamma, const void *beta, int32_t B, int32_t HW, int32_t C,
                                int32_t groups, float eps, int32_t silu, void *y, void *stats_ws, ctx_stream_t stream);
int32_t ctx_layernorm_f32in_f16(const float *x, const void *gamma, const void *beta, int64_t rows, int32_t C, float eps,
                                void *y, ctx_stream_t stream);
/* softmax(Q K^T * scale) V; Q[B,Sq,heads*64], K[B,Skv,heads*64], V likewise (f16) -> O[B,Sq,heads*64];
   row strides in elements.  vt_ws: unused since V is consumed untransposed (ds_read_b64_tr_b16); may be null, ctx_attention_ws_bytes() returns a token size. */
int64_t ctx_attention_ws_bytes(int32_t B, int32_t Skv, int32_t heads);
int32_t ctx_attention_f16(const void *Q, const void *K, const void *V, int32_t B, int32_t Sq, int32_t Skv,
                          int32_t heads, int32_t q_stride, int32_t kv_stride, float scale, void *O,
                          int32_t o_stride, void *vt_ws, ctx_stream_t stream);
/* GEGLU: y[M,C4] = h[:, :C4] * gelu(h[:, C4:])  for h[M,2*C4] f16. */
int32_t ctx_geglu_f16(const void *h, int64_t M, int32_t C4, void *y, ctx_stream_t stream);

/* CFG combine + PNDM/PLMS update fused (stable_diffusion_depth.py:428-430,514; diffusers PNDMScheduler
   step_plms with skip_prk_steps).  eps_pair[2,n] (uncond, text); ets[4,n] history ring (newest at
   slot `head`); coef4 = HOST float[4] linear-multistep weights for (e_t, e_t-1, e_t-2, e_t-3) after insertion;
   sample_coeff, eps_coeff from _get_prev_sample; x[n] updated in place; also writes the blended
   epsilon into ets[head]. mode 0: normal; 1: second call of the first step (average with ets[head],
   use cur_sample_ws as x). */
int32_t ctx_cfg_plms_step(const float *eps_pair, int64_t n, float guidance, float *ets, int32_t head,
                          const float *coef4, float sample_coeff, float eps_coeff, int32_t mode,
                          float *cur_sample_ws, float *x, ctx_stream_t stream);

/* Live per-kernel timing for bench.py's roofline: between begin and end every MFMA kernel launch (class 0 =
   GEMM / implicit-GEMM conv, class 1 = attention) is bracketed by dispatch-tight HIP events on ITS stream;
   end() synchronises them and returns the summed kernel time and the launch count of one class. */
int32_t ctx_profile_begin(void);
int32_t ctx_profile_end(int32_t klass, double *total_ms /*host*/, int64_t *count /*host*/);

/* Benchmark support (tools/bench_gemm.py): `iters` back-to-back launches timed on the device; conv_B > 0 selects the
   implicit-GEMM conv (N = Cout, input [conv_B, conv_H, conv_W, conv_Cin]; conv_flags bit 0: stride 2, bit 1: fused nearest
   x2 upsample, bit 2 (with bit 1): the upsample's phase form, Wt then being the phase pack and residual NULL).  epi 1: GEGLU epilogue.  splitk < 0: the UNet executor's own choice (needs `part`).  Returns average ms
   per launch (< 0: error). */
float ctx_bench_gemm(const void *A, const void *Wt, const void *bias, const void *residual, int32_t M, int32_t N, int32_t K,
                     void *C, int32_t conv_B, int32_t conv_H, int32_t conv_W, int32_t conv_Cin, int32_t conv_flags, int32_t epi,
                     void *part, int32_t splitk, int32_t iters, ctx_stream_t stream);

/* Tuning support (tools/tune_gemm.py): force the tile id of gemm.hip (-1 = planner's choice) and the 256x256 kernel of
   gemm8.hip (-1 planner, 0 never, 1 whenever applicable) for every following GEMM / conv launch of this process. */
void ctx_gemm_tune(int32_t tile, int32_t gemm8);

/* Tuning / test support (tests/test_attention_gpu.py, tools/bench_attn.py): select the attention kernel for every following
   launch of this process instead of CTX_ATTN_NS (2 | 3 | 4), CTX_ATTN_NW8 (0: always 4-wave workgroups, 1: always 8-wave ones,
   2: always the 12-wave K/V-split ones), CTX_ATTN_SPREAD (0 | 1) and CTX_ATTN_LAZY (0 .. 12).  -1 (a negative lazy) = what the
   environment or the default says; for nw8 the default is the balance model ctx_attention_plan reports. */
void ctx_attention_tune(int32_t ns, int32_t nw8, int32_t spread, float lazy);
/* Test-only seam, host only: what ctx_attention_f16 launches for a shape on a device of n_cu compute units under the switches in
   force.  out[4]: waves per workgroup (4 | 8 | 12), key ranges per workgroup (1 | 2), workgroups, and the model's wave-tiles
   (32 queries x 64 keys, the split form's merge counted as one) on the busiest SIMD. */
int32_t ctx_attention_plan(int32_t B, int32_t Sq, int32_t Skv, int32_t heads, int32_t n_cu, int32_t *out);

/* Unit-test support: one 32x32 tile through the MFMA fragment maps the kernels assume.
   which 0: f16 32x32x16 (A[32][16], Bt[32][16]); 1: f32 32x32x2 (A[32][2], Bt[32][2]); C[32][32] f32.
   which 2: the transposing LDS read ds_read_b64_tr_b16 on an f16 tile A[8][32]; C[64 lanes][4] f32 (Bt unused but non-null). */
int32_t ctx_probe_mfma(int32_t which, const void *A, const void *Bt, float *C, ctx_stream_t stream);

/* Measurement support (tools/probe_stage.py): bytes per second one workgroup per CU stages out of L2 by LDS-DMA (mode 0), by
   16-byte register loads (mode 1) or by both (mode 2); `waves` waves per workgroup, `u` (4 | 8) KiB in flight per wave.
   src >= 2 MiB of device memory, sink >= 4 bytes.  Returns the milliseconds of `iters` turns, negative on error. */
float ctx_probe_stage(int32_t mode, int32_t waves, int32_t u, int32_t iters, int32_t shared_region, const void *src, void *sink,
                      ctx_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
