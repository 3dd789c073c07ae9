"""Drop-in for the slice of `kaolin` (0.15.0) the reference calls — same attribute paths, argument
order and return layouts, backed by libctxnerf.so on gfx950:

    kal.render.camera.generate_perspective_projection   src/models/render.py:11
    kal.render.camera.generate_transformation_matrix    src/models/render.py:31,45
    kal.render.mesh.prepare_vertices                    src/models/render.py:112; textured_mesh.py:167
    kal.render.mesh.rasterize                           src/models/render.py:115,119; textured_mesh.py:170,174
    kal.render.mesh.texture_mapping                     src/models/render.py:135
    kal.ops.mesh.index_vertices_by_faces                src/models/textured_mesh.py:149
    kal.io.obj.import_mesh                              src/models/mesh.py:12-14

plus `kal.render.mesh.rasterize_fused`, the single-pass depth+uv+index(+normals) raster the renderer
uses instead of the reference's two passes.  Camera helpers are host-side torch (tiny).
"""
import math
import types
import torch
from . import _lib as L


# ---- camera ------------------------------------------------------------------------------------
def generate_perspective_projection(fovyangle, ratio=1.0, dtype=torch.float):
    tanfov = math.tan(fovyangle / 2.0)
    return torch.tensor([[1.0 / (ratio * tanfov)], [1.0 / tanfov], [-1]], dtype=dtype)


def generate_transformation_matrix(camera_position, look_at, camera_up_direction):
    z_axis = camera_position - look_at
    z_axis = z_axis / z_axis.norm(dim=1, keepdim=True)
    x_axis = torch.cross(camera_up_direction, z_axis, dim=1)
    x_axis = x_axis / x_axis.norm(dim=1, keepdim=True)
    y_axis = torch.cross(z_axis, x_axis, dim=1)
    rot_part = torch.stack([x_axis, y_axis, z_axis], dim=2)
    trans_part = -camera_position.unsqueeze(1) @ rot_part
    return torch.cat([rot_part, trans_part], dim=1)


# ---- mesh ops ----------------------------------------------------------------------------------
def index_vertices_by_faces(vertices_features, faces):
    return vertices_features[:, faces.long()]


def prepare_vertices(vertices, faces, camera_proj, camera_rot=None, camera_trans=None, camera_transform=None):
    if camera_transform is None:
        raise L.CtxError("prepare_vertices: only the camera_transform form used by the reference is implemented")
    lib = L.load()
    dev = vertices.device
    verts = L.f32c(vertices)
    faces = faces.to(device=dev, dtype=torch.int64).contiguous()
    cam = L.f32c(camera_transform, dev)
    proj = L.f32c(camera_proj.reshape(3), dev)
    B, V, _ = verts.shape
    F = faces.shape[0]
    fv_cam = torch.empty(B, F, 3, 3, device=dev)
    fv_img = torch.empty(B, F, 3, 2, device=dev)
    fnorm = torch.empty(B, F, 3, device=dev)
    ws = torch.empty(B * V * 5, device=dev)
    L.check(lib.ctx_prepare_vertices(L.ptr(verts, torch.float32, "vertices"), L.ptr(faces, torch.int64, "faces"),
                                     L.ptr(cam), L.ptr(proj), B, V, F, L.ptr(fv_cam), L.ptr(fv_img), L.ptr(fnorm),
                                     L.ptr(ws), L.stream()))
    return fv_cam, fv_img, fnorm


def _raster_ws(H, W, B, F, dev):
    n = L.load().ctx_rasterize_ws_bytes(H, W, B, F)
    return torch.empty(n, dtype=torch.uint8, device=dev), n


def rasterize(height, width, face_vertices_z, face_vertices_image, face_features, valid_faces=None,
              multiplier=None, eps=None, backend='cuda'):
    """-> (interpolated_features [B,H,W,C] f32, face_idx [B,H,W] i64, -1 = background)."""
    if valid_faces is not None:
        raise L.CtxError("rasterize: valid_faces is not used by the reference and is not implemented")
    multiplier = 1000.0 if multiplier is None else float(multiplier)
    eps = 1e-8 if eps is None else float(eps)
    lib = L.load()
    dev = face_vertices_z.device
    fz, fxy, feat = L.f32c(face_vertices_z), L.f32c(face_vertices_image), L.f32c(face_features)
    B, F, _ = fz.shape
    C = feat.shape[-1]
    out = torch.empty(B, height, width, C, device=dev)
    idx = torch.empty(B, height, width, dtype=torch.int64, device=dev)
    ws, n = _raster_ws(height, width, B, F, dev)
    L.check(lib.ctx_rasterize_fwd(height, width, L.ptr(fz, torch.float32, "face_vertices_z"), L.ptr(fxy), L.ptr(feat),
                                  B, F, C, multiplier, eps, L.ptr(out), L.ptr(idx), L.ptr(ws), n, L.stream()))
    return out, idx


def rasterize_fused(height, width, face_vertices_camera, face_vertices_image, uv_face_attr, face_normals=None,
                    multiplier=1000.0, eps=1e-8):
    """One pass for what the reference does in two (render.py:115-120):
    -> depth [B,H,W,1], uv [B,H,W,2], face_idx [B,H,W] i64, normals [B,H,W,3] | None."""
    lib = L.load()
    dev = face_vertices_camera.device
    fvc, fxy, uva = L.f32c(face_vertices_camera), L.f32c(face_vertices_image), L.f32c(uv_face_attr)
    B, F = fvc.shape[0], fvc.shape[1]
    Bu = uva.shape[0]
    depth = torch.empty(B, height, width, 1, device=dev)
    uv = torch.empty(B, height, width, 2, device=dev)
    idx = torch.empty(B, height, width, dtype=torch.int64, device=dev)
    fn = L.f32c(face_normals) if face_normals is not None else None
    normals = torch.empty(B, height, width, 3, device=dev) if fn is not None else None
    ws, n = _raster_ws(height, width, B, F, dev)
    L.check(lib.ctx_rasterize_fused(height, width, L.ptr(fvc), L.ptr(fxy), L.ptr(uva), Bu, L.ptr(fn), B, F,
                                    float(multiplier), float(eps), L.ptr(depth), L.ptr(uv), L.ptr(idx), L.ptr(normals),
                                    L.ptr(ws), n, L.stream()))
    return depth, uv, idx, normals


# ---- UV scatter: plans ------------------------------------------------------------------------------
# A plan (binning of a raster by atlas tile, uvscatter.hip) depends on (uv, mask) only.  Plans are cached ONLY when the caller
# says the raster will come back (`reuse=True`: the SDS loop's render_cache); one-shot scatters build theirs and drop it.  The
# cache is keyed by the tensors' addresses and versions, holds the tensors alive, is capped in bytes, and every scatter re-checks
# a sampled checksum of (uv, mask) on the device: a raster rewritten behind the key poisons the result with NaN instead of
# silently scattering along the old lists.
_PLANS = {}
PLAN_CACHE_BYTES = 768 << 20


def clear_scatter_plans():
    """Drop every cached scatter plan (and the rasters they keep alive)."""
    _PLANS.clear()


def _plan_bytes(ent):
    return sum(t.numel() * t.element_size() for t in ent if t is not None)


def binned_fits(C, T):
    """True when the tile-binned scatter can take this atlas: C <= 4 and T within the plan's LDS histogram (2272)."""
    return C <= 4 and T <= L.load().ctx_texmap_plan_max_res()


def scatter_plan(uv, mask_idx, T, reuse=False):
    """-> plan buffer for (uv [B,..,2] f32 contiguous, mask_idx | None, T)."""
    lib = L.load()
    B = uv.shape[0]
    HW = uv[0].numel() // 2
    key = (uv.data_ptr(), uv._version, None if mask_idx is None else (mask_idx.data_ptr(), mask_idx._version), B, HW, T)
    ent = _PLANS.get(key) if reuse else None
    if ent is not None:
        return ent[0]
    nbytes = lib.ctx_texmap_bwd_plan_bytes(B, HW, T)
    if nbytes < 0:
        raise L.CtxError(f"scatter_plan: B*HW = {B * HW} pixels do not fit the binned path")
    plan = torch.empty(nbytes, dtype=torch.uint8, device=uv.device)
    L.check(lib.ctx_texmap_bwd_plan(L.ptr(uv, torch.float32, "uv"), L.ptr(mask_idx), B, HW, T, L.ptr(plan), L.stream()))
    if reuse:
        ent = (plan, uv, mask_idx)                    # keep uv / mask alive: the key is their address
        if _plan_bytes(ent) <= PLAN_CACHE_BYTES:
            while _PLANS and sum(_plan_bytes(e) for e in _PLANS.values()) + _plan_bytes(ent) > PLAN_CACHE_BYTES:
                _PLANS.pop(next(iter(_PLANS)))
            _PLANS[key] = ent
    return plan


def scatter_add_texture(go, uv, mask_idx, grad_tex, binned=None, reuse=False):
    """grad_tex [C,T,T] += bilinear scatter of go [B,H,W,C] (or [B,HW,C]) at uv — the backward of texture_mapping.  Large rasters
    (>= 64k pixels, C <= 4, T within the plan's limit) go through the binned, atomics-free path of uvscatter.hip, whose fixed-point
    unit follows max|go| of the call; otherwise the float-atomics kernel.  reuse: keep the plan for the next call on this raster."""
    lib = L.load()
    B = uv.shape[0]
    HW = uv[0].numel() // 2
    C, T = grad_tex.shape[0], grad_tex.shape[-1]
    use = (B * HW >= 65536 and binned_fits(C, T)) if binned is None else binned
    if not use:
        L.check(lib.ctx_texture_mapping_bwd(L.ptr(go, torch.float32, "grad_out"), L.ptr(uv, torch.float32, "uv"), B, HW, C, T,
                                            L.ptr(mask_idx), L.ptr(grad_tex, torch.float32, "grad_tex"), L.stream()))
        return grad_tex
    plan = scatter_plan(uv, mask_idx, T, reuse=reuse)
    ws = torch.empty(lib.ctx_texture_mapping_bwd_binned_ws_bytes(C, T), dtype=torch.uint8, device=uv.device)
    L.check(lib.ctx_texture_mapping_bwd_binned(L.ptr(go, torch.float32, "grad_out"), L.ptr(uv, torch.float32, "uv"), L.ptr(mask_idx), B, HW, C, T,
                                               L.ptr(plan), L.ptr(ws), L.ptr(grad_tex, torch.float32, "grad_tex"), L.stream()))
    return grad_tex


SCATTER_FRAC_BITS = 32          # unit of the painted-view accumulators: 2^-32 (values are colours x weights in [0, 1])


def scatter_fixed(values, uv, mask_idx, acc, frac_bits=SCATTER_FRAC_BITS, reuse=False):
    """acc [C,T,T] int64 += round(values * bilinear weight * 2^frac_bits): the UV back-projection of painted views as integer
    sums (order-free, so view shards on different ranks add up to the same bits).  Any raster size; atlases beyond the plan's
    limit (or C > 4) take the plan-less kernel (one int64 atomic per tap)."""
    lib = L.load()
    B = uv.shape[0]
    HW = uv[0].numel() // 2
    C, T = acc.shape[0], acc.shape[-1]
    plan = scatter_plan(uv, mask_idx, T, reuse=reuse) if binned_fits(C, T) else None
    L.check(lib.ctx_uv_scatter_fixed(L.ptr(values, torch.float32, "values"), L.ptr(uv, torch.float32, "uv"), L.ptr(mask_idx), B, HW, C, T,
                                     L.ptr(plan), int(frac_bits), L.ptr(acc, torch.int64, "acc"), L.stream()))
    return acc


def gather_fixed(values, weight, face_idx, face_vertices_image, faces, texel_face, texel_bary, acc, frac_bits=SCATTER_FRAC_BITS):
    """acc [C+1,T,T] int64 += the texel-side gather of painted views (uvgather.hip): every chart texel of (texel_face [T,T] i64,
    texel_bary [T,T,3] f32: TexturedMeshModel.texel_map) projects its surface point into every view of face_idx [B,H,W] i64 /
    face_vertices_image [B,F,3,2] f32, takes the bilinear colour of values [B,H,W,C] f32 there if its face (or one sharing a
    vertex in faces [F,3] i64) owns the pixel, and adds round(colour * w * 2^frac_bits) to acc[:C] and round(w * 2^frac_bits)
    to acc[C]; w = weight [B,H,W] f32 at the nearest pixel, or 1 for weight = None.  Integer sums, as scatter_fixed."""
    lib = L.load()
    p = (L.ptr(values, torch.float32, "values"), L.ptr(weight, torch.float32, "weight"), L.ptr(face_idx, torch.int64, "face_idx"),
         L.ptr(face_vertices_image, torch.float32, "face_vertices_image"), L.ptr(faces, torch.int64, "faces"),
         L.ptr(texel_face, torch.int64, "texel_face"), L.ptr(texel_bary, torch.float32, "texel_bary"))
    p_acc = L.ptr(acc, torch.int64, "acc")
    if values.dim() != 4 or face_idx.dim() != 3 or faces.dim() != 2 or faces.shape[1] != 3 or texel_face.dim() != 2 or acc.dim() != 3:
        raise L.CtxError(f"gather_fixed: want values [B,H,W,C], face_idx [B,H,W], faces [F,3], texel_face [T,T], acc [C+1,T,T]; got "
                         f"{tuple(values.shape)}, {tuple(face_idx.shape)}, {tuple(faces.shape)}, {tuple(texel_face.shape)}, {tuple(acc.shape)}")
    B, H, W, C = values.shape
    F, T = faces.shape[0], texel_face.shape[0]
    want = dict(face_idx=(B, H, W), face_vertices_image=(B, F, 3, 2), texel_face=(T, T), texel_bary=(T, T, 3), acc=(C + 1, T, T))
    got = dict(face_idx=face_idx, face_vertices_image=face_vertices_image, texel_face=texel_face, texel_bary=texel_bary, acc=acc)
    if weight is not None:
        want['weight'], got['weight'] = (B, H, W), weight
    for k, shp in want.items():
        if tuple(got[k].shape) != shp:
            raise L.CtxError(f"gather_fixed: {k} is {tuple(got[k].shape)}, expected {shp} (values {tuple(values.shape)}, faces {tuple(faces.shape)})")
    n = lib.ctx_uv_gather_ws_bytes(B, F)
    if n < 0:
        raise L.CtxError(f"gather_fixed: B={B} or F={F} < 1")
    ws = torch.empty(n, dtype=torch.uint8, device=values.device)
    L.check(lib.ctx_uv_gather_fixed(*p, B, H, W, C, F, T, int(frac_bits), p_acc, L.ptr(ws), n, L.stream()))
    return acc


def fixed_to_float(acc, frac_bits=SCATTER_FRAC_BITS, out=None):
    """int64 sums in units of 2^-frac_bits -> float32 (one rounding per texel)."""
    lib = L.load()
    if out is None:
        out = torch.empty(acc.shape, dtype=torch.float32, device=acc.device)
    L.check(lib.ctx_fixed_to_float(L.ptr(acc, torch.int64, "acc"), acc.numel(), int(frac_bits), 0, L.ptr(out, torch.float32, "out"), L.stream()))
    return out


def _check_bake_list(who, idx, s):
    L.ptr(idx, torch.int32, "idx")
    if idx.dim() != 1:
        raise L.CtxError(f"{who}: idx must be a 1-D int32 texel list, got shape {tuple(idx.shape)}")
    if int(s) != s or not 1 <= s <= 4:
        raise L.CtxError(f"{who}: supersample={s}: want a whole number in [1, 4]")
    if idx.numel() * int(s) ** 2 >= 2 ** 31:
        raise L.CtxError(f"{who}: {idx.numel()} entries x {int(s) ** 2} sub-samples: want fewer than 2^31 rows; split the list")
    return idx.numel(), int(s)


def texel_rays(texel_face, texel_bary, face_uv, vertices, faces, idx, supersample, shell):
    """-> (rays_o [n*s*s,3] f32, rays_d [n*s*s,3] f32, valid [n*s*s] u8): per texel of the list idx int32 [n] and sub-sample k = a + s*b
    (row j*s*s + k) a ray that starts `shell` outside the surface point of the sub-sample and runs down the face normal (bake.hip; the
    rule is written out at ctx_texel_rays).  texel_face [T,T] i64 and texel_bary [T,T,3] f32: TexturedMeshModel.texel_map; face_uv
    [F,3,2] f32 (vt[ft]); vertices [V,3] f32; faces [F,3] i64.  Rows of an entry that names no texel, no face or a face without area are
    zero with valid = 0.  No host sync."""
    lib = L.load()
    p = (L.ptr(texel_face, torch.int64, "texel_face"), L.ptr(texel_bary, torch.float32, "texel_bary"), L.ptr(face_uv, torch.float32, "face_uv"),
         L.ptr(vertices, torch.float32, "vertices"), L.ptr(faces, torch.int64, "faces"))
    n, s = _check_bake_list("texel_rays", idx, supersample)
    if texel_face.dim() != 2 or texel_face.shape[0] != texel_face.shape[1] or faces.dim() != 2 or faces.shape[1] != 3 or vertices.dim() != 2 \
            or vertices.shape[1] != 3:
        raise L.CtxError(f"texel_rays: want texel_face [T,T], vertices [V,3], faces [F,3]; got {tuple(texel_face.shape)}, "
                         f"{tuple(vertices.shape)}, {tuple(faces.shape)}")
    T, F, V = texel_face.shape[0], faces.shape[0], vertices.shape[0]
    for k, t, shp in (("texel_bary", texel_bary, (T, T, 3)), ("face_uv", face_uv, (F, 3, 2))):
        if tuple(t.shape) != shp:
            raise L.CtxError(f"texel_rays: {k} is {tuple(t.shape)}, expected {shp} (texel_face {tuple(texel_face.shape)}, faces {tuple(faces.shape)})")
    shell = float(shell)
    if not (shell > 0 and math.isfinite(shell)):
        raise L.CtxError(f"texel_rays: shell={shell}: want a finite world length > 0")
    dev = idx.device
    ro, rd = torch.empty(n * s * s, 3, device=dev), torch.empty(n * s * s, 3, device=dev)
    valid = torch.empty(n * s * s, dtype=torch.uint8, device=dev)
    if n == 0:                                        # an empty list: empty outputs (a tensor without elements has no address to hand on)
        return ro, rd, valid
    L.check(lib.ctx_texel_rays(*p, L.ptr(idx), n, T, F, V, s, shell, L.ptr(ro), L.ptr(rd), L.ptr(valid), L.stream()))
    return ro, rd, valid


def bake_resolve(rgb, alpha, valid, idx, supersample, acc, min_alpha=0.5, frac_bits=SCATTER_FRAC_BITS):
    """acc [4,T,T] int64 += per texel of the list idx int32 [n] (DISTINCT texels; not looked at here) the mean over its valid, finite
    sub-samples of rgb [n*s*s,3] and alpha [n*s*s] in units of 2^-frac_bits, where that mean alpha >= min_alpha (bake.hip; the rule is
    written out at ctx_bake_resolve).  rgb is premultiplied (sum w_i c_i), so acc[:3]/acc[3] is the colour and acc[3] > 0 the coverage."""
    lib = L.load()
    p = (L.ptr(rgb, torch.float32, "rgb"), L.ptr(alpha, torch.float32, "alpha"), L.ptr(valid, torch.uint8, "valid"))
    p_acc = L.ptr(acc, torch.int64, "acc")
    n, s = _check_bake_list("bake_resolve", idx, supersample)
    if acc.dim() != 3 or acc.shape[0] != 4 or acc.shape[1] != acc.shape[2]:
        raise L.CtxError(f"bake_resolve: acc is {tuple(acc.shape)}, expected [4,T,T]")
    R = n * s * s
    for k, t, shp in (("rgb", rgb, (R, 3)), ("alpha", alpha, (R,)), ("valid", valid, (R,))):
        if tuple(t.shape) != shp:
            raise L.CtxError(f"bake_resolve: {k} is {tuple(t.shape)}, expected {shp} ({n} entries x {s * s} sub-samples)")
    if n == 0:
        return acc
    L.check(lib.ctx_bake_resolve(*p, L.ptr(idx), n, s, acc.shape[1], float(min_alpha), int(frac_bits), p_acc, L.stream()))
    return acc


def chart_texels(texel_face):
    """-> idx int32 [n], ascending: the chart texels y*T + x of texel_face [T,T] i64 (texel_face >= 0), by the ordered compaction
    ctx_texel_compact.  A set-up call: it reads n back, which SYNCS the host."""
    lib = L.load()
    L.ptr(texel_face, torch.int64, "texel_face")
    n_tex = texel_face.numel()
    n_ws = lib.ctx_texel_compact_ws_bytes(n_tex)
    if n_ws < 0:
        raise L.CtxError(f"chart_texels: {n_tex} texels: want 1 <= T*T < 2^31")
    mask = (texel_face >= 0).to(torch.uint8).contiguous()
    ws = torch.empty(n_ws, dtype=torch.uint8, device=mask.device)
    idx = torch.empty(n_tex, dtype=torch.int32, device=mask.device)
    count = torch.empty(1, dtype=torch.int64, device=mask.device)
    L.check(lib.ctx_texel_compact(L.ptr(mask), n_tex, L.ptr(idx), L.ptr(count), L.ptr(ws), L.stream()))
    return idx[:int(count.item())].clone()


# ---- ray / mesh hits on the occupancy grid (csrc/meshhit.hip; the rule is written out at ctx_mesh_ray_hit) --------
def mesh_cell_lists(vertices, faces, G, lo, inv):
    """-> (count int32 [G^3], cell_off int32 [G^3 + 1], cell_tri int32 [n]): per cell of the grid the faces the voxeliser marks it for,
    ascending by face id (ctx_mesh_cells_count, the exclusive scan, ctx_mesh_cells_fill).  vertices float32 [V,3] and faces int64 [F,3]
    are device tensors; lo, inv: three floats each, the grid's.  A set-up call: it reads n back, which SYNCS the host, once."""
    lib = L.load()
    p_v, p_f = L.ptr(vertices, torch.float32, "vertices"), L.ptr(faces, torch.int64, "faces")
    V, F, G = vertices.shape[0], faces.shape[0], int(G)
    if not 1 <= G <= 256:
        raise L.CtxError(f"mesh_cell_lists: G={G} outside [1, 256]")
    dev, ncell = vertices.device, G ** 3
    box = (*map(float, lo), *map(float, inv))
    count = torch.empty(ncell, dtype=torch.int32, device=dev)
    L.check(lib.ctx_mesh_cells_count(p_v, p_f, V, F, G, *box, L.ptr(count), L.stream()))
    cell_off = torch.empty(ncell + 1, dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    L.check(lib.ctx_mesh_cells_scan(L.ptr(count), ncell, L.ptr(cell_off), L.ptr(total), L.stream()))
    n = int(total.item())                                                                  # the one host sync
    if n >= 2 ** 31:
        raise L.CtxError(f"mesh_cell_lists: {n} (cell, face) entries for {F} faces at G={G}: want fewer than 2^31; use a coarser grid")
    cell_tri = torch.empty(n, dtype=torch.int32, device=dev)
    if n:
        cursor, slots = torch.empty(ncell, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        L.check(lib.ctx_mesh_cells_fill(p_v, p_f, V, F, G, *box, L.ptr(cell_off), n, L.ptr(cursor), L.ptr(slots), L.ptr(cell_tri), L.stream()))
    return count, cell_off, cell_tri


def mesh_tri_records(vertices, faces):
    """-> tri float32 [F,12]: per face v0, e1 = v1 - v0, e2 = v2 - v0, each padded to four floats (ctx_mesh_tri_setup); NaN for a face
    with an index outside [0, V) or a non-finite vertex.  No host sync."""
    p_v, p_f = L.ptr(vertices, torch.float32, "vertices"), L.ptr(faces, torch.int64, "faces")
    tri = torch.empty(faces.shape[0], 12, dtype=torch.float32, device=vertices.device)
    L.check(L.load().ctx_mesh_tri_setup(p_v, p_f, vertices.shape[0], faces.shape[0], L.ptr(tri), L.stream()))
    return tri


def mesh_ray_hit(rays_o, rays_d, near, far, cells, G, lo, hi, inv, h, cell_off, cell_tri, tri, faces, own_face=None, any_hit=False):
    """ctx_mesh_ray_hit -> (hit u8 [R], t f32 [R], face i32 [R], uv f32 [R,2]), or hit alone with any_hit=True (mode 1).  rays_o, rays_d
    float32 [R,3]; own_face int64 [R] or None.  R = 0 gives empty tensors.  No host sync."""
    p_o, p_d = L.ptr(rays_o, torch.float32, "rays_o"), L.ptr(rays_d, torch.float32, "rays_d")
    if rays_o.dim() != 2 or rays_o.shape[1] != 3 or rays_d.shape != rays_o.shape:
        raise L.CtxError(f"mesh_ray_hit: want rays_o, rays_d [R,3]; got {tuple(rays_o.shape)}, {tuple(rays_d.shape)}")
    R, dev = rays_o.shape[0], rays_o.device
    p_own = L.ptr(own_face, torch.int64, "own_face")
    if own_face is not None and tuple(own_face.shape) != (R,):
        raise L.CtxError(f"mesh_ray_hit: own_face is {tuple(own_face.shape)}, expected {(R,)}")
    hit = torch.empty(R, dtype=torch.uint8, device=dev)
    out = () if any_hit else (torch.empty(R, dtype=torch.float32, device=dev), torch.empty(R, dtype=torch.int32, device=dev),
                              torch.empty(R, 2, dtype=torch.float32, device=dev))
    if R:
        L.check(L.load().ctx_mesh_ray_hit(p_o, p_d, R, float(near), float(far), L.ptr(cells, torch.uint8, "cells"), int(G), *map(float, lo),
                                          *map(float, hi), *map(float, inv), *map(float, h), L.ptr(cell_off, torch.int32, "cell_off"),
                                          L.ptr(cell_tri, torch.int32, "cell_tri") if cell_tri.numel() else None, cell_tri.numel(),
                                          L.ptr(tri, torch.float32, "tri"), L.ptr(faces, torch.int64, "faces"), faces.shape[0], p_own,
                                          1 if any_hit else 0, L.ptr(hit), *(L.ptr(x) for x in out), *([None] * (3 - len(out))), L.stream()))
    return hit if any_hit else (hit, *out)


def mesh_closest_point(pts, r, G, lo, inv, cell_off, cell_tri, tri):
    """ctx_mesh_closest_point -> (found u8 [n], dist f32 [n], face i32 [n], uv f32 [n,2]): the nearest point of the mesh within r of each of
    pts float32 [n,3] (csrc/meshdist.hip; the rule is written out at the entry point).  A miss: found = 0, dist = r, face = -1, uv = 0.
    n = 0 gives empty tensors.  No host sync."""
    p_p = L.ptr(pts, torch.float32, "pts")
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise L.CtxError(f"mesh_closest_point: want pts [n,3]; got {tuple(pts.shape)}")
    n, dev = pts.shape[0], pts.device
    found = torch.empty(n, dtype=torch.uint8, device=dev)
    dist, face = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    uv = torch.empty(n, 2, dtype=torch.float32, device=dev)
    if n:
        L.check(L.load().ctx_mesh_closest_point(p_p, n, float(r), int(G), *map(float, lo), *map(float, inv), L.ptr(cell_off, torch.int32, "cell_off"),
                                                L.ptr(cell_tri, torch.int32, "cell_tri") if cell_tri.numel() else None, cell_tri.numel(),
                                                L.ptr(tri, torch.float32, "tri"), tri.shape[0], L.ptr(found), L.ptr(dist), L.ptr(face), L.ptr(uv),
                                                L.stream()))
    return found, dist, face, uv


def mesh_vertex_faces(faces, V):
    """-> (vf_off int32 [V + 1], vf_face int32 [n]): per vertex id the faces of faces int64 [F,3] that name it at a corner, ascending by
    face id (ctx_mesh_vertex_faces_count, the exclusive scan ctx_mesh_cells_scan, ctx_mesh_vertex_faces_fill); a face with an id outside
    [0, V) is in no list.  A set-up call: it reads n back, which SYNCS the host, once."""
    lib = L.load()
    p_f = L.ptr(faces, torch.int64, "faces")
    V, F = int(V), faces.shape[0]
    if faces.dim() != 2 or faces.shape[1] != 3 or F < 1:
        raise L.CtxError(f"mesh_vertex_faces: want faces [F,3] with F >= 1; got {tuple(faces.shape)}")
    if not 1 <= V <= 256 ** 3 or F >= 2 ** 31 // 3:
        raise L.CtxError(f"mesh_vertex_faces: V={V}, F={F}: want 1 <= V <= 256^3 and F < 2^31 / 3")
    dev = faces.device
    count = torch.empty(V, dtype=torch.int32, device=dev)
    L.check(lib.ctx_mesh_vertex_faces_count(p_f, V, F, L.ptr(count), L.stream()))
    vf_off = torch.empty(V + 1, dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    L.check(lib.ctx_mesh_cells_scan(L.ptr(count), V, L.ptr(vf_off), L.ptr(total), L.stream()))
    n = int(total.item())                                                                  # the one host sync
    vf_face = torch.empty(n, dtype=torch.int32, device=dev)
    if n:
        cursor, slots = torch.empty(V, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        L.check(lib.ctx_mesh_vertex_faces_fill(p_f, V, F, L.ptr(vf_off), n, L.ptr(cursor), L.ptr(slots), L.ptr(vf_face), L.stream()))
    return vf_off, vf_face


def mesh_pseudonormals(faces, V, tri, vf_off, vf_face):
    """ctx_mesh_pseudonormals -> pn float32 [F,7,3]: per face its unit normal (row 0), the angle-weighted pseudonormals of its three
    vertices (rows 1-3) and the pseudonormals of its edges (v0,v1), (v0,v2), (v1,v2) (rows 4-6), not normalised (csrc/meshpn.hip; the
    rule is written out at the entry point).  tri: mesh_tri_records; vf_off, vf_face: mesh_vertex_faces.  No host sync."""
    p_f = L.ptr(faces, torch.int64, "faces")
    V, F = int(V), faces.shape[0]
    if tuple(tri.shape) != (F, 12) or tuple(vf_off.shape) != (V + 1,):
        raise L.CtxError(f"mesh_pseudonormals: want tri [{F},12] and vf_off [{V + 1}]; got {tuple(tri.shape)}, {tuple(vf_off.shape)}")
    pn = torch.empty(F, 7, 3, dtype=torch.float32, device=faces.device)
    L.check(L.load().ctx_mesh_pseudonormals(p_f, V, F, L.ptr(tri, torch.float32, "tri"), L.ptr(vf_off, torch.int32, "vf_off"),
                                            L.ptr(vf_face, torch.int32, "vf_face") if vf_face.numel() else None, vf_face.numel(), L.ptr(pn),
                                            L.stream()))
    return pn


def mesh_signed_distance(pts, r, G, lo, inv, cell_off, cell_tri, tri, pn):
    """ctx_mesh_signed_distance -> (found u8 [n], sdist f32 [n], face i32 [n], uv f32 [n,2], feature u8 [n], grad f32 [n,3]):
    mesh_closest_point with the sign of (p - q) . pn[face, feature] on the distance, the feature of the winning face on which the nearest
    point lies, and the unit direction grad = d sdist / d p (csrc/meshdist.hip; the rule is written out at the entry point).  A miss:
    found = 0, sdist = +r, face = -1, uv = 0, feature = 0, grad = 0.  n = 0 gives empty tensors.  No host sync."""
    p_p = L.ptr(pts, torch.float32, "pts")
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise L.CtxError(f"mesh_signed_distance: want pts [n,3]; got {tuple(pts.shape)}")
    if pn.dim() != 3 or tuple(pn.shape[1:]) != (7, 3) or pn.shape[0] < tri.shape[0]:
        raise L.CtxError(f"mesh_signed_distance: want pn [F,7,3] with F >= {tri.shape[0]}; got {tuple(pn.shape)}")
    n, dev = pts.shape[0], pts.device
    found, feature = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    sdist, face = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    uv, grad = torch.empty(n, 2, dtype=torch.float32, device=dev), torch.empty(n, 3, dtype=torch.float32, device=dev)
    if n:
        L.check(L.load().ctx_mesh_signed_distance(p_p, n, float(r), int(G), *map(float, lo), *map(float, inv), L.ptr(cell_off, torch.int32, "cell_off"),
                                                  L.ptr(cell_tri, torch.int32, "cell_tri") if cell_tri.numel() else None, cell_tri.numel(),
                                                  L.ptr(tri, torch.float32, "tri"), tri.shape[0], L.ptr(pn, torch.float32, "pn"), pn.shape[0],
                                                  L.ptr(found), L.ptr(sdist), L.ptr(face), L.ptr(uv), L.ptr(feature), L.ptr(grad), L.stream()))
    return found, sdist, face, uv, feature, grad


def _fill_ws(lib, T, device):
    n = lib.ctx_atlas_fill_ws_bytes(T)
    if n < 0:
        raise L.CtxError(f"atlas fill: T={T} outside [1, 4096]")
    return torch.empty(n, dtype=torch.uint8, device=device), n


def nearest_seed(seed):
    """seed [T,T] uint8 (non-zero = seed) -> (src [T,T] int32, d2 [T,T] int32): per texel the seed minimising (d2, sy, sx), exact
    integer Euclidean; src = sy*T + sx; both -1 everywhere when there is no seed."""
    lib = L.load()
    if seed.dim() != 2 or seed.shape[0] != seed.shape[1]:
        raise L.CtxError(f"nearest_seed: seed must be [T,T], got {tuple(seed.shape)}")
    T = seed.shape[0]
    p_seed = L.ptr(seed, torch.uint8, "seed")
    ws, n = _fill_ws(lib, T, seed.device)
    src = torch.empty(T, T, dtype=torch.int32, device=seed.device)
    d2 = torch.empty(T, T, dtype=torch.int32, device=seed.device)
    L.check(lib.ctx_nearest_seed(p_seed, T, L.ptr(src), L.ptr(d2), L.ptr(ws), n, L.stream()))
    return src, d2


def atlas_fill(atlas, coverage, chart, pad):
    """Atlas completion: (filled [C,T,T] f32, src [T,T] int32).  Uncovered chart texels take the colour of their nearest covered
    texel, then texels within `pad` of chart | covered take the colour of the nearest of those; src is the flat index of the
    covered texel a colour was copied from (-1 = untouched).  atlas [C,T,T] f32, coverage [T,T] f32, chart [T,T] uint8."""
    lib = L.load()
    if atlas.dim() != 3 or atlas.shape[1] != atlas.shape[2] or tuple(coverage.shape) != tuple(atlas.shape[1:]) or tuple(chart.shape) != tuple(atlas.shape[1:]):
        raise L.CtxError(f"atlas_fill: want atlas [C,T,T], coverage [T,T], chart [T,T]; got {tuple(atlas.shape)}, {tuple(coverage.shape)}, {tuple(chart.shape)}")
    C, T = atlas.shape[0], atlas.shape[1]
    p_atlas, p_cov, p_chart = L.ptr(atlas, torch.float32, "atlas"), L.ptr(coverage, torch.float32, "coverage"), L.ptr(chart, torch.uint8, "chart")
    ws, n = _fill_ws(lib, T, atlas.device)
    filled = torch.empty_like(atlas)
    src = torch.empty(T, T, dtype=torch.int32, device=atlas.device)
    L.check(lib.ctx_atlas_fill(p_atlas, p_cov, p_chart, C, T, int(pad), L.ptr(filled), L.ptr(src), L.ptr(ws), n, L.stream()))
    return filled, src


# ---- mask operators of the progressive paint loop (csrc/maskops.hip) ---------------------------------------
MORPH_OPS = {'dilate': 0, 'erode': 1}
MASK_MAX_K = 63


def _mask_image(who, src):
    """src float32 [..., H, W] (device, contiguous) -> (pointer, N, H, W)."""
    p = L.ptr(src, torch.float32, "src")
    if src.dim() < 2 or src.numel() == 0:
        raise L.CtxError(f"{who}: want a non-empty float32 image [..., H, W], got {tuple(src.shape)}")
    H, W = int(src.shape[-2]), int(src.shape[-1])
    return p, src.numel() // (H * W), H, W


def mask_morph(src, k, op):
    """k x k dilation (op 'dilate': max) or erosion ('erode': min) of float32 images [..., H, W], the window clipped to the image (pixels
    outside take no part: OpenCV's default border of both).  k odd in [1, 63]; it may exceed H or W.  Any finite values: soft masks too.
    -> a new tensor of src's shape; src is not modified.  No host sync."""
    if op not in MORPH_OPS:
        raise L.CtxError(f"mask_morph: op={op!r}: expected one of {tuple(MORPH_OPS)}")
    p, N, H, W = _mask_image("mask_morph", src)
    dst, ws = torch.empty_like(src), torch.empty_like(src)
    L.check(L.load().ctx_mask_morph(p, N, H, W, int(k), MORPH_OPS[op], L.ptr(dst), L.ptr(ws), L.stream()))
    return dst


def dilate(src, k):
    return mask_morph(src, k, 'dilate')


def erode(src, k):
    return mask_morph(src, k, 'erode')


def gaussian_taps(k, sigma):
    """The k taps of torchvision's gaussian_blur kernel: exp(-0.5 (x / sigma)^2) at the integer offsets x = -(k//2) .. k//2, normalised to
    sum 1 in float64, then rounded to float32.  -> list of k Python floats (each exactly a float32)."""
    k, sigma = int(k), float(sigma)
    if k < 1 or k % 2 == 0 or not (sigma > 0 and math.isfinite(sigma)):
        raise L.CtxError(f"gaussian_taps: k={k}, sigma={sigma}: want an odd k >= 1 and a finite sigma > 0")
    x = torch.arange(-(k // 2), k // 2 + 1, dtype=torch.float64)
    pdf = torch.exp(-0.5 * (x / sigma) ** 2)
    return (pdf / pdf.sum()).to(torch.float32).tolist()


def sep_filter(src, taps):
    """Separable k-tap filter of float32 images [..., H, W]: the taps along the rows, then along the columns, reflect padding that does
    not repeat the edge (index -1 reads 1), every output the taps summed left to right in binary32.  taps: k host floats, k odd in
    [1, 63], k // 2 <= min(H, W) - 1.  -> a new tensor; no host sync (the taps travel with the launch)."""
    p, N, H, W = _mask_image("sep_filter", src)
    taps = [float(t) for t in taps]
    k = len(taps)
    if k < 1 or k > MASK_MAX_K or k % 2 == 0:
        raise L.CtxError(f"sep_filter: {k} taps: want an odd count in [1, {MASK_MAX_K}]")
    dst, ws = torch.empty_like(src), torch.empty_like(src)
    L.check(L.load().ctx_sep_filter(p, N, H, W, (L.C.c_float * k)(*taps), k, L.ptr(dst), L.ptr(ws), L.stream()))
    return dst


def gaussian_blur(src, k, sigma):
    return sep_filter(src, gaussian_taps(k, sigma))


def atlas_blend(contrib, zsum, acc, meta):
    """The progressive atlas update (ctx_atlas_blend; the rule is written out there): acc [4,T,T] int64 and meta [T,T] float32 take one
    view's contribution contrib [4,T,T] int64 / zsum [T,T] int64 (sums in units of 2^-32, as scatter_fixed / gather_fixed leave them),
    IN PLACE.  A texel the view gave no weight keeps its bits; a painted one ends with acc[3] = 2^32.  -> (acc, meta)."""
    p = (L.ptr(contrib, torch.int64, "contrib"), L.ptr(zsum, torch.int64, "zsum"))
    p_acc, p_meta = L.ptr(acc, torch.int64, "acc"), L.ptr(meta, torch.float32, "meta")
    if acc.dim() != 3 or acc.shape[0] != 4 or acc.shape[1] != acc.shape[2]:
        raise L.CtxError(f"atlas_blend: acc is {tuple(acc.shape)}, expected [4,T,T]")
    T = int(acc.shape[1])
    for name, t, shp in (("contrib", contrib, (4, T, T)), ("zsum", zsum, (T, T)), ("meta", meta, (T, T))):
        if tuple(t.shape) != shp:
            raise L.CtxError(f"atlas_blend: {name} is {tuple(t.shape)}, expected {shp}")
    L.check(L.load().ctx_atlas_blend(*p, T, p_acc, p_meta, L.stream()))
    return acc, meta


# ---- multi-view consistency (src/training/trainer.py:429-531) ------------------------------------------
VIEW_ROWS = {'reference': 0, 'image': 1}      # 'reference': upstream's rows (row 0 at Y = -1); 'image': the raster's (row 0 at Y = +1)


def _vc_args(views, faces, face_idx, fvi):
    p = (L.ptr(views, torch.float32, "views"), L.ptr(faces, torch.int64, "faces"), L.ptr(face_idx, torch.int64, "face_idx"),
         L.ptr(fvi, torch.float32, "face_vertices_image"))
    if views.dim() != 4 or face_idx.dim() != 3 or faces.dim() != 2 or faces.shape[1] != 3 or fvi.dim() != 4:
        raise L.CtxError(f"view_consistency: want views [V,C,h,w], faces [F,3], face_idx [V,h,w], face_vertices_image [V,F,3,2]; got "
                         f"{tuple(views.shape)}, {tuple(faces.shape)}, {tuple(face_idx.shape)}, {tuple(fvi.shape)}")
    V, C, h, w = views.shape
    F = faces.shape[0]
    if tuple(face_idx.shape) != (V, h, w) or tuple(fvi.shape) != (V, F, 3, 2):
        raise L.CtxError(f"view_consistency: face_idx {tuple(face_idx.shape)} / face_vertices_image {tuple(fvi.shape)} do not match views "
                         f"{tuple(views.shape)} and faces {tuple(faces.shape)}")
    return p, (V, C, h, w, F)


class _ViewConsistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, views, faces, face_idx, fvi, rows, seen, build):
        lib = L.load()
        (p_views, p_faces, p_idx, p_fvi), (V, C, h, w, F) = _vc_args(views, faces, face_idx, fvi)
        dev = views.device
        n_vertices = seen.shape[1]
        pair_sum = torch.empty(V, V, dtype=torch.int64, device=dev)
        pair_count = torch.empty(V, V, dtype=torch.int64, device=dev)
        n_outside = torch.empty((), dtype=torch.int64, device=dev)
        mean = torch.empty((), dtype=torch.float32, device=dev)
        L.check(lib.ctx_view_consistency_fwd(p_views, p_faces, p_idx, p_fvi, V, C, h, w, F, n_vertices, rows, int(build),
                                             L.ptr(seen, torch.uint8, "seen"), seen.numel(), L.ptr(pair_sum), L.ptr(pair_count), L.ptr(n_outside),
                                             L.ptr(mean), L.stream()))
        ctx.save_for_backward(views, faces, face_idx, fvi, seen, pair_count)
        ctx.meta = (V, C, h, w, F, n_vertices, rows)
        ctx.mark_non_differentiable(pair_sum, pair_count, n_outside)
        return mean, pair_sum, pair_count, n_outside

    @staticmethod
    def backward(ctx, g, *unused):
        views, faces, face_idx, fvi, seen, pair_count = ctx.saved_tensors
        V, C, h, w, F, n_vertices, rows = ctx.meta
        lib = L.load()
        g = L.f32c(g)
        sign_count = torch.empty(views.shape, dtype=torch.int32, device=views.device)
        grad = torch.empty_like(views)
        L.check(lib.ctx_view_consistency_bwd(L.ptr(views), L.ptr(faces), L.ptr(face_idx), L.ptr(fvi), L.ptr(seen), V, C, h, w, F, n_vertices, rows,
                                             L.ptr(pair_count), L.ptr(g, torch.float32, "grad_mean"), L.ptr(sign_count), L.ptr(grad), L.stream()))
        return grad, None, None, None, None, None, None


def view_consistency(views, faces, face_idx, face_vertices_image, rows='image', seen=None, stats=False, n_vertices=None):
    """Mean colour agreement of V rendered views over the pixels that show a shared vertex (trainer.py:429-531): a f32 device
    scalar, differentiable with respect to `views`, no host sync.  views [V,C,h,w] f32, faces [F,3] i64, face_idx [V,h,w] i64
    (-1 = background), face_vertices_image [V,F,3,2] f32.  rows: 'image' looks the source pixel up in the raster's row convention,
    'reference' in upstream's (vertically mirrored) one.  seen [V, n_vertices] u8: the seen-vertex map a previous call on the SAME
    raster returned (stats['seen']); it depends on faces and face_idx only, so the SDS loop builds it once.  n_vertices: the mesh's
    vertex count; without it (and without `seen`) it is read from faces.max(), which syncs.  stats=True: -> (mean, dict(pair_sum
    [V,V] i64 in units of 2^-32 indexed [source, target], pair_count [V,V] i64, n_outside i64, seen))."""
    if rows not in VIEW_ROWS:
        raise L.CtxError(f"view_consistency: rows={rows!r}, expected one of {tuple(VIEW_ROWS)}")
    (_, (V, C, h, w, F)) = _vc_args(views, faces, face_idx, face_vertices_image)
    build = seen is None
    if build:
        n_vertices = int(faces.max()) + 1 if n_vertices is None else int(n_vertices)
        if L.load().ctx_view_consistency_ws_bytes(V, n_vertices) < 0:
            raise L.CtxError(f"view_consistency: V={V} outside [1, 16] or n_vertices={n_vertices} < 1")
        seen = torch.empty(V, n_vertices, dtype=torch.uint8, device=views.device)
    else:
        L.ptr(seen, torch.uint8, "seen")
        if seen.dim() != 2 or seen.shape[0] != V:
            raise L.CtxError(f"view_consistency: seen must be [V={V}, n_vertices] uint8, got {tuple(seen.shape)}")
    mean, pair_sum, pair_count, n_outside = _ViewConsistency.apply(views, faces, face_idx, face_vertices_image, VIEW_ROWS[rows], seen, build)
    if stats:
        return mean, dict(pair_sum=pair_sum, pair_count=pair_count, n_outside=n_outside, seen=seen)
    return mean


# ---- exposure compensation across painted views (gain compensation, Brown & Lowe 2007) ----------------------------------
VIEW_GAIN_MAX_VIEWS, VIEW_GAIN_MAX_RES = 16, 4096


def view_pair_stats(atlases, lo=0.02, hi=0.98):
    """-> (count [V,V] i64, colour_sum [V,V,3] i64): the pair statistics the per-view gains are solved from (csrc/viewgain.hip; the
    rule is written out at ctx_view_pair_stats and in tests/exposure_rule.py).  atlases [V,4,Tc,Tc] int64: per view the weighted
    colour sums and the weight sum of a low-resolution back-projection, in units of 2^-32 as scatter_fixed leaves them.  View v is
    valid at a texel when its weight is positive and its colour lies in [lo, hi] on all three channels; count[i,j] is the number of
    texels where i and j are both valid, colour_sum[i,j] view i's colour (units of 2^-24) summed over them.  Integer sums: every
    rank computes the same bits.  1 <= V <= 16, 1 <= Tc <= 4096, 0 < lo < hi <= 1.  No host sync."""
    if not isinstance(atlases, torch.Tensor) or atlases.dim() != 4 or atlases.shape[1] != 4 or atlases.shape[2] != atlases.shape[3]:
        raise L.CtxError(f"view_pair_stats: want atlases [V,4,Tc,Tc], got {tuple(getattr(atlases, 'shape', ()))}")
    V, Tc = int(atlases.shape[0]), int(atlases.shape[2])
    if not 1 <= V <= VIEW_GAIN_MAX_VIEWS:
        raise L.CtxError(f"view_pair_stats: V={V} outside [1, {VIEW_GAIN_MAX_VIEWS}]")
    if not 1 <= Tc <= VIEW_GAIN_MAX_RES:
        raise L.CtxError(f"view_pair_stats: Tc={Tc} outside [1, {VIEW_GAIN_MAX_RES}]")
    lo, hi = float(lo), float(hi)
    if not 0 < lo < hi <= 1:
        raise L.CtxError(f"view_pair_stats: lo={lo} hi={hi}, expected 0 < lo < hi <= 1")
    p = L.ptr(atlases, torch.int64, "atlases")
    count = torch.empty(V, V, dtype=torch.int64, device=atlases.device)
    colour_sum = torch.empty(V, V, 3, dtype=torch.int64, device=atlases.device)
    L.check(L.load().ctx_view_pair_stats(p, V, Tc, lo, hi, L.ptr(count), L.ptr(colour_sum), L.stream()))
    return count, colour_sum


def solve_view_gains(count, colour_sum, ridge=0.01, max_gain=2.0):
    """-> gains float64 [V,3] (a CPU tensor): one gain per view and colour channel from view_pair_stats' sums, so that gained views
    agree in mean colour where they overlap.  Per channel, N = count, S = colour_sum[..., ch]: d_ij = log(S_ij / N_ij) - log(S_ji /
    N_ij) for i < j with N_ij > 0 (d_ji = -d_ij); the log gains l minimise sum_{i<j} N_ij (l_i + d_ij - l_j)^2 + ridge sum_i N_ii l_i^2,
    solved from the V x V normal equations by numpy.linalg.lstsq in float64 (minimum norm where they are singular: ridge = 0 is legal,
    and a view that overlaps no other keeps gain exactly 1); gains = clip(exp(l), 1 / max_gain, max_gain).  The one host sync of the
    feature: count and colour_sum (device or CPU tensors, or arrays) are brought to the host."""
    import numpy as np
    ridge, max_gain = float(ridge), float(max_gain)
    if not ridge >= 0:
        raise L.CtxError(f"solve_view_gains: ridge={ridge}, expected >= 0")
    if not max_gain >= 1:
        raise L.CtxError(f"solve_view_gains: max_gain={max_gain}, expected >= 1")
    host = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    N, S = host(count).astype(np.float64), host(colour_sum).astype(np.float64)
    if N.ndim != 2 or N.shape[0] != N.shape[1] or S.shape != N.shape + (3,):
        raise L.CtxError(f"solve_view_gains: want count [V,V] and colour_sum [V,V,3], got {N.shape} and {S.shape}")
    V = N.shape[0]
    gains = np.ones((V, 3), np.float64)
    for ch in range(3):
        M, b = np.zeros((V, V), np.float64), np.zeros(V, np.float64)
        for i in range(V):
            M[i, i] = ridge * N[i, i]
            for j in range(V):
                if j == i or not N[i, j] > 0:
                    continue
                a, c = min(i, j), max(i, j)
                d = np.log(S[a, c, ch] / N[a, c]) - np.log(S[c, a, ch] / N[a, c])
                M[i, i] += N[i, j]
                M[i, j] = -N[i, j]
                b[i] -= N[i, j] * (d if i < j else -d)
        gains[:, ch] = np.clip(np.exp(np.linalg.lstsq(M, b, rcond=None)[0]), 1.0 / max_gain, max_gain)
    return torch.from_numpy(gains)


class _TextureMapping(torch.autograd.Function):
    @staticmethod
    def forward(ctx, uv, tex, mode, mask_idx):
        lib = L.load()
        B, H, W, _ = uv.shape
        Bt, Cc, T, T2 = tex.shape
        if T != T2:
            raise L.CtxError("texture_mapping: square texture expected")
        # an expanded (stride-0) batch is the reference's texture_img.expand(B,...) — keep one copy
        if Bt > 1 and tex.stride(0) == 0:
            tex_c, Bt_eff = tex[:1].contiguous(), 1
        else:
            tex_c, Bt_eff = tex.contiguous(), Bt
        uvc = L.f32c(uv)
        out = torch.empty(B, H, W, Cc, device=uv.device)
        m = {'bilinear': 0, 'nearest': 1}[mode]
        if Bt_eff == 1 and Cc <= 4 and B * H * W >= 4 * T * T:
            # one shared texture sampled by many more pixels than it has texels: interleave the channels once (16 B per
            # texel), then every bilinear tap is one gather (bit-identical results)
            packed = torch.empty(T, T, 4, device=uv.device)
            L.check(lib.ctx_texture_pack4(L.ptr(tex_c.float() if tex_c.dtype != torch.float32 else tex_c, torch.float32, "texture_maps"),
                                          Cc, T, L.ptr(packed), L.stream()))
            L.check(lib.ctx_texture_mapping_packed_fwd(L.ptr(uvc, torch.float32, "texture_coordinates"), L.ptr(packed), B, H * W, Cc, T, m,
                                                       L.ptr(mask_idx), L.ptr(out), L.stream()))
        else:
            L.check(lib.ctx_texture_mapping_fwd(L.ptr(uvc, torch.float32, "texture_coordinates"),
                                                L.ptr(tex_c, torch.float32, "texture_maps"), B, H * W, Cc, T, Bt_eff,
                                                m, L.ptr(mask_idx), L.ptr(out), L.stream()))
        ctx.save_for_backward(uvc, mask_idx if mask_idx is not None else torch.empty(0))
        ctx.meta = (B, H * W, Cc, T, Bt, Bt_eff, mode, tex.shape, mask_idx is not None)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        uvc, mask_idx = ctx.saved_tensors
        B, HW, Cc, T, Bt, Bt_eff, mode, tshape, has_mask = ctx.meta
        if mode != 'bilinear':
            return None, torch.zeros(tshape, device=grad_out.device), None, None
        lib = L.load()
        go = L.f32c(grad_out)
        if Bt_eff == 1:
            g = torch.zeros(Cc, T, T, device=go.device)
            scatter_add_texture(go, uvc, mask_idx if has_mask else None, g, reuse=True)
            if Bt > 1:      # input was an expand(): autograd sums the batch slices, so put the whole sum in slice 0
                full = torch.zeros(tshape, device=go.device)
                full[0] = g
                g = full
            else:
                g = g[None]
        else:
            g = torch.zeros(Bt, Cc, T, T, device=go.device)
            for b in range(Bt):
                mi = mask_idx[b:b + 1].contiguous() if has_mask else None
                L.check(lib.ctx_texture_mapping_bwd(L.ptr(go[b:b + 1].contiguous()), L.ptr(uvc[b:b + 1].contiguous()), 1, HW,
                                                    Cc, T, L.ptr(mi), L.ptr(g[b]), L.stream()))
        return None, g, None, None


# ---- mip-mapped sampling (csrc/texmip.hip; the rule is tests/mipmap_rule.py) ------------------------------
def _mip_build(tex, levels, coverage=None):
    """-> (pyr uint8 buffer, cov_count uint8 | None, [level tensors]) of the atlas tex [C,T,T] f32 contiguous; level 0 is tex itself,
    the others are views of pyr.  The counts are kept whenever a coverage plane is given or a later pass needs them."""
    lib = L.load()
    if tex.dim() != 3 or tex.shape[1] != tex.shape[2]:
        raise L.CtxError(f"mip_pyramid: want a square atlas [C,T,T]; got {tuple(tex.shape)}")
    Cc, T, levels = int(tex.shape[0]), int(tex.shape[1]), int(levels)
    if Cc > 4:
        raise L.CtxError(f"mip_pyramid: C={Cc} channels; the mipmap path takes 1 to 4")
    nbytes = lib.ctx_mip_levels_bytes(Cc, T, levels)
    if nbytes < 0:
        raise L.CtxError(f"mip_pyramid: mip levels L={levels} do not fit T={T}: {lib.ctx_last_error().decode()}")
    if coverage is not None and (coverage.dtype != torch.uint8 or tuple(coverage.shape) != (T, T)):
        raise L.CtxError(f"mip_pyramid: coverage must be uint8 [{T},{T}]; got {coverage.dtype} {tuple(coverage.shape)}")
    pyr = torch.empty(nbytes, dtype=torch.uint8, device=tex.device)
    cov_count = None
    if coverage is not None or levels > 6:
        cov_count = torch.empty(lib.ctx_mip_cov_bytes(T, levels), dtype=torch.uint8, device=tex.device)
    L.check(lib.ctx_mip_build(L.ptr(tex, torch.float32, "texture_maps"), L.ptr(coverage), Cc, T, levels, L.ptr(pyr), L.ptr(cov_count), L.stream()))
    views, flt, off = [tex], pyr.view(torch.float32), 0
    for l in range(1, levels):
        n = Cc * (T >> l) ** 2
        views.append(flt[off:off + n].view(Cc, T >> l, T >> l))
        off += n
    return pyr, cov_count, views


def mip_pyramid(tex, levels, coverage=None):
    """The mip pyramid of the atlas tex [C,T,T] (C <= 4): a list of `levels` tensors, level l of side T >> l; level 0 is tex, the others
    are views of one buffer.  A coarse texel is the mean of its covered children; coverage uint8 [T,T] (None: everything) says which
    level-0 texels count, so that a chart's coarse texels do not average gutter colour."""
    return _mip_build(L.f32c(tex), levels, coverage)[2]


def face_uv_lod(face_vertices_image, uv_face_attr, H, W, T, levels, scale=None):
    """lod [B,F] f32 of every (view, face): integer part = mip level, fraction = blend towards the next.  The raster interpolates uv
    affinely on the screen, so a face's uv Jacobian is constant; the lod follows the longer of its two pixel-step lengths in texels.
    scale [B] (None: 1) widens a view's pixel footprint, for an image that is shrunk after the render."""
    lib = L.load()
    fvi, uva = L.f32c(face_vertices_image), L.f32c(uv_face_attr)
    B, F = int(fvi.shape[0]), int(fvi.shape[1])
    if tuple(fvi.shape[1:]) != (F, 3, 2) or tuple(uva.shape[1:]) != (F, 3, 2) or uva.shape[0] not in (1, B):
        raise L.CtxError(f"face_uv_lod: want face_vertices_image [B,F,3,2] and uv_face_attr [1|B,F,3,2]; got {tuple(fvi.shape)}, {tuple(uva.shape)}")
    if scale is not None:
        scale = L.f32c(torch.as_tensor(scale, dtype=torch.float32), fvi.device).reshape(-1)
        if scale.numel() != B:
            raise L.CtxError(f"face_uv_lod: scale has {scale.numel()} entries for {B} views")
    lod = torch.empty(B, F, device=fvi.device)
    L.check(lib.ctx_face_uv_lod(L.ptr(fvi), L.ptr(uva), int(uva.shape[0]), B, F, int(H), int(W), int(T), int(levels), L.ptr(scale), L.ptr(lod),
                                L.stream()))
    return lod


def mip_scatter_texture(go, uv, lod, face_idx, cov_count, C, T, levels):
    """-> grad_tex [C,T,T]: the backward of the mipmap lookup (bit-reproducible; see ctx_texture_mapping_mip_bwd)."""
    lib = L.load()
    B, HW, F = uv.shape[0], uv[0].numel() // 2, lod.shape[1]
    ws = torch.empty(lib.ctx_texture_mapping_mip_bwd_ws_bytes(C, T, levels), dtype=torch.uint8, device=uv.device)
    g = torch.empty(C, T, T, device=uv.device)
    L.check(lib.ctx_texture_mapping_mip_bwd(L.ptr(go, torch.float32, "grad_out"), L.ptr(uv, torch.float32, "uv"), L.ptr(lod, torch.float32, "lod"),
                                            L.ptr(face_idx, torch.int64, "mask_idx"), L.ptr(cov_count), B, HW, F, C, T, levels, L.ptr(ws), L.ptr(g),
                                            L.stream()))
    return g


class _TextureMappingMip(torch.autograd.Function):
    @staticmethod
    def forward(ctx, uv, tex, mask_idx, lod, levels, coverage):
        lib = L.load()
        B, H, W, _ = uv.shape
        Bt, Cc, T, T2 = tex.shape
        if T != T2:
            raise L.CtxError("texture_mapping: square texture expected")
        if Cc > 4:
            raise L.CtxError(f"texture_mapping: mode 'mipmap' takes 1 to 4 channels; got C={Cc}")
        if Bt not in (1, B):
            raise L.CtxError(f"texture_mapping: {Bt} textures for {B} views")
        if Bt > 1 and tex.stride(0) != 0 and not bool((tex == tex[:1]).all()):
            raise L.CtxError("texture_mapping: mode 'mipmap' samples one shared atlas; the textures of this batch differ")
        shared = Bt == 1 or tex.stride(0) == 0              # a materialised batch of equal textures: one pyramid, a gradient per slice
        if tuple(lod.shape) != (B, lod.shape[-1]) or tuple(mask_idx.shape) != (B, H, W):
            raise L.CtxError(f"texture_mapping: mode 'mipmap' wants lod [B,F] and mask_idx [B,H,W]; got {tuple(lod.shape)}, {tuple(mask_idx.shape)}")
        tex_c, uvc, lodc, idx = L.f32c(tex[0]), L.f32c(uv), L.f32c(lod), mask_idx.contiguous()
        pyr, cov_count, _ = _mip_build(tex_c, levels, coverage)
        out = torch.empty(B, H, W, Cc, device=uv.device)
        L.check(lib.ctx_texture_mapping_mip_fwd(L.ptr(uvc, torch.float32, "texture_coordinates"), L.ptr(tex_c), L.ptr(pyr), L.ptr(lodc),
                                                L.ptr(idx, torch.int64, "mask_idx"), B, H * W, int(lodc.shape[1]), Cc, T, int(levels), L.ptr(out),
                                                L.stream()))
        ctx.save_for_backward(uvc, lodc, idx, cov_count if cov_count is not None else torch.empty(0))
        ctx.meta = (Cc, T, int(levels), shared, tex.shape, cov_count is not None)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        uvc, lodc, idx, cov_count = ctx.saved_tensors
        Cc, T, levels, shared, tshape, has_cov = ctx.meta
        cov_count = cov_count if has_cov else None
        go = L.f32c(grad_out)
        g = torch.zeros(tshape, device=go.device)
        if shared:          # one atlas (or its expand()): autograd sums the batch slices, so the whole sum goes into slice 0
            g[0] = mip_scatter_texture(go, uvc, lodc, idx, cov_count, Cc, T, levels)
        else:
            for b in range(tshape[0]):
                g[b] = mip_scatter_texture(go[b:b + 1].contiguous(), uvc[b:b + 1].contiguous(), lodc[b:b + 1].contiguous(), idx[b:b + 1].contiguous(),
                                           cov_count, Cc, T, levels)
        return None, g, None, None, None, None


def texture_mapping(texture_coordinates, texture_maps, mode='bilinear', mask_idx=None, lod=None, levels=4, coverage=None):
    """grid_sample(tex, (u, 1-v)*2-1, align_corners=False, padding_mode='border') -> [B,H,W,C].
    Differentiable w.r.t. texture_maps (bilinear, mipmap).  mask_idx: optional face_idx to fuse `* mask`.
    mode='mipmap': trilinear lookup in the `levels`-level pyramid of one shared atlas (C <= 4); mask_idx (the raster's face_idx) and
    lod (`face_uv_lod`'s table [B,F]) are required, coverage (uint8 [T,T]) is `mip_pyramid`'s.  Where the lod is 0 the result is the
    bilinear one.  The other modes do not look at lod, levels or coverage."""
    if mode == 'mipmap':
        if mask_idx is None or lod is None:
            raise L.CtxError("texture_mapping: mode 'mipmap' needs mask_idx (the raster's face_idx) and lod (kal.face_uv_lod)")
        if texture_coordinates.dim() != 4:
            raise L.CtxError("texture_mapping: mode 'mipmap' wants texture_coordinates [B,H,W,2]")
        return _TextureMappingMip.apply(texture_coordinates, texture_maps, mask_idx, lod, int(levels), coverage)
    if mode not in ('bilinear', 'nearest'):
        raise L.CtxError(f"texture_mapping: mode {mode!r} not implemented on the HIP path (bilinear/nearest/mipmap)")
    if texture_coordinates.dim() == 3:
        return _TextureMapping.apply(texture_coordinates[:, :, None, :], texture_maps, mode, mask_idx)[:, :, 0]
    return _TextureMapping.apply(texture_coordinates, texture_maps, mode, mask_idx)


def active_texels(uv, face_idx, T, mask=None):
    """The texels of a T x T atlas that texture_mapping can read for this raster: the four bilinear taps of every pixel of
    uv [B,H,W,2] f32 with face_idx [B,H,W] i64 >= 0, whatever their weights (the rule is written out at ctx_texel_active_mark).
    -> (idx int32 [n]: their flat indices y*T + x, ascending; mask uint8 [T,T]: 1 where active).  mask: a mask an earlier call
    returned, to add this raster to (the union); it is updated in place.  A set-up call: it reads n back, which SYNCS the host."""
    lib = L.load()
    p_uv, p_idx = L.ptr(uv, torch.float32, "uv"), L.ptr(face_idx, torch.int64, "face_idx")
    T = int(T)
    if uv.dim() != 4 or uv.shape[-1] != 2 or tuple(face_idx.shape) != tuple(uv.shape[:3]):
        raise L.CtxError(f"active_texels: want uv [B,H,W,2] and face_idx [B,H,W]; got {tuple(uv.shape)}, {tuple(face_idx.shape)}")
    if mask is None:
        mask = torch.zeros(T, T, dtype=torch.uint8, device=uv.device)
    elif tuple(mask.shape) != (T, T):
        raise L.CtxError(f"active_texels: mask is {tuple(mask.shape)}, expected {(T, T)}")
    p_mask = L.ptr(mask, torch.uint8, "mask")
    B, H, W, _ = uv.shape
    L.check(lib.ctx_texel_active_mark(p_uv, p_idx, B, H, W, T, p_mask, L.stream()))
    n_ws = lib.ctx_texel_compact_ws_bytes(T * T)
    if n_ws < 0:
        raise L.CtxError(f"active_texels: T={T} gives more texels than an int32 index holds")
    ws = torch.empty(n_ws, dtype=torch.uint8, device=uv.device)
    idx = torch.empty(T * T, dtype=torch.int32, device=uv.device)
    count = torch.empty(1, dtype=torch.int64, device=uv.device)
    L.check(lib.ctx_texel_compact(p_mask, T * T, L.ptr(idx), L.ptr(count), L.ptr(ws), L.stream()))
    return idx[:int(count.item())].clone(), mask


# ---- OBJ import (host, Python like kaolin's) ------------------------------------------------------
def import_mesh(path, with_normals=False, with_materials=False, heterogeneous_mesh_handler=None):
    vs, vts, fs, fts = [], [], [], []
    with open(path) as fh:
        for line in fh:
            if line.startswith('v '):
                vs.append([float(x) for x in line.split()[1:4]])
            elif line.startswith('vt '):
                vts.append([float(x) for x in line.split()[1:3]])
            elif line.startswith('f '):
                vi, ti = [], []
                for tok in line.split()[1:]:
                    p = tok.split('/')
                    vi.append(int(p[0]))
                    ti.append(int(p[1]) if len(p) > 1 and p[1] else 0)
                nv, nt = len(vs), len(vts)
                vi = [i - 1 if i > 0 else nv + i for i in vi]
                ti = [i - 1 if i > 0 else (nt + i if i < 0 else -1) for i in ti]
                for k in range(1, len(vi) - 1):          # naive homogenize: fan triangulation
                    fs.append([vi[0], vi[k], vi[k + 1]])
                    fts.append([ti[0], ti[k], ti[k + 1]])
    return types.SimpleNamespace(
        vertices=torch.tensor(vs, dtype=torch.float32), faces=torch.tensor(fs, dtype=torch.int64),
        uvs=torch.tensor(vts, dtype=torch.float32).reshape(-1, 2),
        face_uvs_idx=torch.tensor(fts, dtype=torch.int64) if fts else torch.zeros(0, 3, dtype=torch.int64))


render = types.SimpleNamespace(
    camera=types.SimpleNamespace(generate_perspective_projection=generate_perspective_projection,
                                 generate_transformation_matrix=generate_transformation_matrix),
    mesh=types.SimpleNamespace(prepare_vertices=prepare_vertices, rasterize=rasterize, rasterize_fused=rasterize_fused,
                               texture_mapping=texture_mapping))
ops = types.SimpleNamespace(mesh=types.SimpleNamespace(index_vertices_by_faces=index_vertices_by_faces))
io = types.SimpleNamespace(obj=types.SimpleNamespace(import_mesh=import_mesh),
                           utils=types.SimpleNamespace(heterogeneous_mesh_handler_naive_homogenize=None))
