"""BASELINE configs[4]: "NeRF volume render 512^2 rays x 128 samples + SD2-depth refine".

The reference names this path in north_star but holds no body for it (its `get_rays` / `sample_pdf` are dead code and the
ray-march is absent), so this module is the thin host glue over the pieces that do exist on the HIP path:

  get_rays (src/run_nerf_helpers.py:139-148)  ->  stratified samples  ->  fused 3-D embed + NeRF2D(63 -> 4)
  ->  raw2outputs (nerf-pytorch; the compositing step run_nerf_helpers.py:130-133 points to)
  ->  depth normalised like Renderer.normalize_multiple_depth's output convention (closer = larger, background 0)
  ->  StableDiffusion.img2img_step (src/stable_diffusion_depth.py:284-578) on the rendered image + depth.

Training: `train_step` is nerf-pytorch's optimisation step on a batch of rays (stratified jitter, density noise, hierarchical
pass, photometric MSE) with the gradient through the compositing kernel's backward into the field; `fit_views` distils posed
images (e.g. renders of a painted mesh) into the 3-D field with it.

Multi-GPU: rays shard by contiguous row tiles with NO exchange until the image gather (`all_gather` of the
tiles); the refine step is one UNet denoise per image, i.e. replicas only.
"""
import numpy as np
import torch
import torch.distributed as dist
from . import _lib as L
from . import run_nerf_helpers as rnh


def pinhole(H, W, fovy=np.pi / 3):
    """K = [[f,0,W/2],[0,f,H/2],[0,0,1]] with f = (H/2)/tan(fovy/2) (SURVEY §8d cfg 5)."""
    f = (H / 2) / np.tan(fovy / 2)
    return np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], np.float32)


def view_cameras(elev, azim, radius, look_at_height, H, W, fovyangle=np.pi / 3):
    """view_camera for V poses at once: elev, azim, radius are numbers, sequences or tensors of V entries -> (K [3,3], c2ws [V,3,4])."""
    from . import kal
    e, a, r = (torch.as_tensor(x, dtype=torch.float32).detach().cpu().reshape(-1) for x in (elev, azim, radius))
    V = max(e.numel(), a.numel(), r.numel())
    e, a, r = (x.expand(V) if x.numel() == 1 else x for x in (e, a, r))
    if not (e.numel() == a.numel() == r.numel() == V and V >= 1):
        raise L.CtxError(f"view_cameras: elev, azim and radius hold {e.numel()}, {a.numel()} and {r.numel()} poses")
    pos = torch.stack([r * torch.sin(e) * torch.sin(a), r * torch.cos(e), r * torch.sin(e) * torch.cos(a)], dim=1)   # Renderer.get_camera_from_view
    look_at = torch.zeros_like(pos)
    look_at[:, 1] = float(look_at_height)
    up = torch.tensor([0.0, 1.0, 0.0]).expand(V, 3)
    M = kal.generate_transformation_matrix(pos, look_at, up)                # [V,4,3] = [rot ; -pos @ rot]: world -> camera, row vectors
    c2ws = torch.cat([M[:, :3, :], pos[:, :, None]], dim=2).to(torch.float32).contiguous()
    t = np.tan(fovyangle / 2.0)
    K = np.array([[W / (2 * t), 0, (W - 1) / 2], [0, H / (2 * t), (H - 1) / 2], [0, 0, 1]], np.float32)
    return K, c2ws


def view_camera(elev, azim, radius, look_at_height, H, W, fovyangle=np.pi / 3):
    """The camera of a Renderer pose, as get_rays takes it: -> (K float32 [3,3], c2w float32 [3,4]).  elev, azim, radius and look_at_height
    as Renderer.get_camera_from_view takes them.  kal.generate_transformation_matrix(pos, look_at, up) is [rot ; -pos @ rot], so
    c2w = [rot | pos]: the camera looks down -z, as get_rays assumes.  fx = W / (2 tan(fov/2)), fy = H / (2 tan(fov/2)) (the renderer's
    projection has ratio = 1, so x and y both span tan(fov/2)), cx = (W - 1)/2, cy = (H - 1)/2: get_rays' ((i - cx)/fx, -(j - cy)/fy, -1)
    then passes through the centre of raster pixel (j, i), x = (2i + 1 - W)/W, y = (H - 2j - 1)/H.  `pinhole` has its
    principal point half a pixel further, at the corner between the four middle pixels."""
    K, c2ws = view_cameras(elev, azim, radius, look_at_height, H, W, fovyangle)
    if c2ws.shape[0] != 1:
        raise L.CtxError(f"view_camera: one pose expected, got {c2ws.shape[0]}; use view_cameras")
    return K, c2ws[0]


def shard_rows(H, rank, world):
    """Row range [r0, r1) of this rank: contiguous tiles, remainder rows to the first ranks."""
    base, rem = divmod(H, world)
    r0 = rank * base + min(rank, rem)
    return r0, r0 + base + (1 if rank < rem else 0)


def _check_mesh(vertices, faces, dilate, who):
    """Shapes, dtypes and counts of a mesh handed to the voxeliser, looked at before any pointer is taken."""
    if not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32:
        raise L.CtxError(f"{who}: want vertices float32 [V,3], got {getattr(vertices, 'dtype', type(vertices).__name__)} "
                         f"{tuple(getattr(vertices, 'shape', ()))}")
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int64:
        raise L.CtxError(f"{who}: want faces int64 [F,3] (the dtype Mesh.faces has), got {getattr(faces, 'dtype', type(faces).__name__)} "
                         f"{tuple(getattr(faces, 'shape', ()))}")
    if vertices.shape[0] == 0:
        raise L.CtxError(f"{who}: the mesh has no vertex")
    if faces.shape[0] == 0:
        raise L.CtxError(f"{who}: the mesh has no face (F = 0): nothing to voxelise")
    if int(dilate) != dilate or dilate < 0:
        raise L.CtxError(f"{who}: dilate={dilate}: want a whole number of cells >= 0")


def _grid_box(G, lo, hi, who):
    """-> (G, lo [3], hi [3], inv [3], h [3]) of a G^3 grid over the box lo .. hi (a number or three per axis), float32."""
    G = int(G)
    if not 1 <= G <= 256:
        raise L.CtxError(f"{who}: G={G} outside [1, 256]")
    lo = np.broadcast_to(np.asarray(lo, np.float32), (3,)).copy()
    hi = np.broadcast_to(np.asarray(hi, np.float32), (3,)).copy()
    if not bool(np.all(lo < hi)) or not bool(np.all(np.isfinite(hi - lo))):
        raise L.CtxError(f"{who}: the box needs finite lo < hi on every axis, got lo={lo.tolist()}, hi={hi.tolist()}")
    ext = hi - lo                                           # binary32, once: the kernels and the restatement take these by value
    return G, lo, hi, np.float32(G) / ext, ext / np.float32(G)


class OccupancyGrid:
    """Which cells of a G^3 grid over the box lo .. hi hold density: the ray path evaluates the field only on the samples inside
    occupied cells (render_rays(occupancy=)), the ray-path counterpart of optim.field_texels = 'active'.
    cells uint8 [G,G,G] (index [cz,cy,cx], 1 = occupied) and dens float32 [G,G,G], the decayed running maximum of the density
    the field gave in each cell.  lo, hi: a number or three per axis; 1 <= G <= 256.  A new grid is all occupied with dens = 0,
    so until the first `update` it only clips the samples to the box."""

    def __init__(self, G, lo, hi, device):
        self.G, self.lo, self.hi, self.inv, self.h = _grid_box(G, lo, hi, "OccupancyGrid")
        G = self.G
        self.device = torch.device(device)
        self.cells = torch.ones(G, G, G, dtype=torch.uint8, device=self.device)
        self.dens = torch.zeros(G, G, G, dtype=torch.float32, device=self.device)

    @classmethod
    def from_mask(cls, mask, lo, hi):
        """A grid with the given occupied cells: mask bool [G,G,G] (index [cz,cy,cx]) on the device the grid lives on."""
        if not isinstance(mask, torch.Tensor) or mask.dim() != 3 or len(set(mask.shape)) != 1:
            raise L.CtxError(f"OccupancyGrid.from_mask: want a [G,G,G] tensor, got {tuple(getattr(mask, 'shape', ()))}")
        grid = cls(mask.shape[0], lo, hi, mask.device)
        grid.cells = (mask != 0).to(torch.uint8).contiguous()
        return grid

    @classmethod
    def from_mesh(cls, vertices, faces, G, lo, hi, dilate=1):
        """A grid whose occupied cells are the mesh's surface: every cell a triangle touches (`ctx_occ_voxelize`, conservative: no
        touched cell is missed), grown by `dilate` cells on every side (`ctx_occ_dilate`); dens = 0.  vertices float32 [V,3] and faces
        int64 [F,3] (the dtype Mesh.faces has) are device tensors; the grid lives on their device.
        The vertices are taken as given: they must be in the world frame of the rays.  For a TexturedMeshModel that is
        model.mesh.vertices after its normalisation, together with the c2w of the renderer's poses.
        A trained field blurs the surface over a cell or two, hence dilate=1 by default.  Such a grid is meant to stay as it is:
        fit_views(occupancy_every=0) never refreshes it from the student's density."""
        _check_mesh(vertices, faces, dilate, "OccupancyGrid.from_mesh")
        grid = cls(G, lo, hi, vertices.device)
        grid.cells.zero_()
        grid.voxelize(vertices, faces, dilate=dilate)
        return grid

    def voxelize(self, vertices, faces, dilate=0):
        """Adds a mesh to this grid: the union of what is occupied with the cells the triangles touch, those grown by `dilate` cells.
        vertices float32 [V,3], faces int64 [F,3], device tensors in the world frame of the rays (from_mesh).  A face with an index
        outside [0, V) or a non-finite vertex marks nothing.  After `update`, this gives mesh + learned density."""
        _check_mesh(vertices, faces, dilate, "OccupancyGrid.voxelize")
        p_v, p_f = L.ptr(vertices, torch.float32, "vertices"), L.ptr(faces, torch.int64, "faces")
        L.ptr(self.cells, torch.uint8, "cells")
        lib = L.load()
        target = self.cells if dilate == 0 else torch.zeros_like(self.cells)       # grown alone, then united: what is there does not grow
        L.check(lib.ctx_occ_voxelize(p_v, p_f, vertices.shape[0], faces.shape[0], self.G, *map(float, self.lo), *map(float, self.inv),
                                     L.ptr(target), L.stream()))
        if dilate > 0:
            grown, ws = torch.empty_like(target), torch.empty_like(target)
            L.check(lib.ctx_occ_dilate(L.ptr(target), self.G, min(int(dilate), self.G), L.ptr(grown), L.ptr(ws), L.stream()))
            self.cells |= grown

    def dilate(self, k):
        """Grows the occupied cells by k cells on every side (a cube: a cell is occupied when one within k on the three axes was)."""
        k = int(k)
        if k < 0:
            raise L.CtxError(f"OccupancyGrid.dilate: k={k}: want k >= 0")
        p_c = L.ptr(self.cells, torch.uint8, "cells")
        out, ws = torch.empty_like(self.cells), torch.empty_like(self.cells)
        L.check(L.load().ctx_occ_dilate(p_c, self.G, min(k, self.G), L.ptr(out), L.ptr(ws), L.stream()))
        self.cells = out

    def ray_spans(self, rays_o, rays_d, near, far):
        """-> (span float32 [R,2], hit bool [R]): per ray the parameters at which it enters its first and leaves its last occupied
        cell within [near, far] clipped to the box (`ctx_occ_ray_spans`); (near, far) and hit = False for a ray that meets none.
        rays_o, rays_d: float32 [R,3] device tensors.  No host sync."""
        near, far = float(near), float(far)
        if not (near < far and np.isfinite(near) and np.isfinite(far)):
            raise L.CtxError(f"OccupancyGrid.ray_spans: want finite near < far, got {near}, {far}")
        if not (isinstance(rays_o, torch.Tensor) and isinstance(rays_d, torch.Tensor) and rays_o.dim() == 2 and rays_o.shape[1] == 3
                and rays_o.shape[0] >= 1 and rays_d.shape == rays_o.shape):
            raise L.CtxError(f"OccupancyGrid.ray_spans: want rays_o, rays_d [R,3] with R >= 1; got {tuple(getattr(rays_o, 'shape', ()))}, "
                             f"{tuple(getattr(rays_d, 'shape', ()))}")
        p_o, p_d = L.ptr(rays_o, torch.float32, "rays_o"), L.ptr(rays_d, torch.float32, "rays_d")
        R = rays_o.shape[0]
        span = torch.empty(R, 2, dtype=torch.float32, device=rays_o.device)
        hit = torch.empty(R, dtype=torch.uint8, device=rays_o.device)
        L.check(L.load().ctx_occ_ray_spans(p_o, p_d, R, near, far, L.ptr(self.cells, torch.uint8, "cells"), self.G, *map(float, self.lo),
                                           *map(float, self.hi), *map(float, self.inv), *map(float, self.h), L.ptr(span), L.ptr(hit),
                                           L.stream()))
        return span, hit != 0

    def march_bound(self, step):
        """An upper bound on the samples `march` places on one ray: floor(D / step * (1 + 2^-15)) + (3G + 4) // 2 + 1 with D the box
        diagonal (the path inside the box over step, one per run from ceil, and the rounding)."""
        D = float(np.sqrt(np.sum((self.hi.astype(np.float64) - self.lo.astype(np.float64)) ** 2)))
        return int(np.floor(D / float(step) * (1.0 + 2.0 ** -15))) + (3 * self.G + 4) // 2 + 1

    def march(self, rays_o, rays_d, near, far, step, perturb=False, generator=None, starts=False):
        """-> (ray_off int64 [R+1], ray_id int32 [n], t [n], dt [n], pts [n,3]): every ray walks the grid once and gets samples `step`
        apart (a WORLD length, whatever |rays_d| is) inside its runs of occupied cells and nowhere else (`ctx_occ_march_count`, the
        exclusive scan, `ctx_occ_march_write`).  Ray r owns ray_off[r] .. ray_off[r+1], ascending in t; sample j of a run [a, b] cut into k
        intervals of width dt sits at a + (j + u) * dt with u = 0.5, or with perturb one uniform draw per sample (drawn after the count,
        which does not depend on it: a seeded generator repeats exactly).  n = 0 is legal: empty lists.  Reading n back SYNCS the host,
        the path's one sync.  A (G, box, step) whose per-ray bound `march_bound` exceeds 4096, the most the compositing backward holds,
        is refused.  starts=True adds a sixth tensor ts [n] = t - u * dt, the start of each sample's interval (what rnh.resample_packed
        takes): one binary32 torch expression, u = 0.5 without perturb."""
        near, far, step = float(near), float(far), float(step)
        if not (near < far and np.isfinite(near) and np.isfinite(far)):
            raise L.CtxError(f"OccupancyGrid.march: want finite near < far, got {near}, {far}")
        if not (step > 0 and np.isfinite(step)):
            raise L.CtxError(f"OccupancyGrid.march: step={step}: want a finite world length > 0")
        bound = self.march_bound(step)
        if bound > 4096:
            raise L.CtxError(f"OccupancyGrid.march: step={step:g} with G={self.G} over the box {self.lo.tolist()} .. {self.hi.tolist()} can put "
                             f"{bound} samples on one ray; the compositing backward holds 4096: use a longer step")
        if not (isinstance(rays_o, torch.Tensor) and isinstance(rays_d, torch.Tensor) and rays_o.dim() == 2 and rays_o.shape[1] == 3
                and rays_o.shape[0] >= 1 and rays_d.shape == rays_o.shape):
            raise L.CtxError(f"OccupancyGrid.march: want rays_o, rays_d [R,3] with R >= 1; got {tuple(getattr(rays_o, 'shape', ()))}, "
                             f"{tuple(getattr(rays_d, 'shape', ()))}")
        p_o, p_d = L.ptr(rays_o, torch.float32, "rays_o"), L.ptr(rays_d, torch.float32, "rays_d")
        lib = L.load()
        R, dev = rays_o.shape[0], rays_o.device
        grid = (L.ptr(self.cells, torch.uint8, "cells"), self.G, *map(float, self.lo), *map(float, self.hi), *map(float, self.inv),
                *map(float, self.h), step)
        count = torch.empty(R, dtype=torch.int32, device=dev)
        L.check(lib.ctx_occ_march_count(p_o, p_d, R, near, far, *grid, L.ptr(count), L.stream()))
        ray_off = torch.zeros(R + 1, dtype=torch.int64, device=dev)
        torch.cumsum(count, 0, dtype=torch.int64, out=ray_off[1:])
        n = int(ray_off[R].item())                                                         # the one host sync
        if n >= 2 ** 31:
            raise L.CtxError(f"OccupancyGrid.march: {n} samples on {R} rays: want n < 2^31; split the batch")
        u = torch.rand(n, device=dev, generator=generator) if perturb else None
        ray_id = torch.empty(n, dtype=torch.int32, device=dev)
        t, dt, pts = torch.empty(n, device=dev), torch.empty(n, device=dev), torch.empty(n, 3, device=dev)
        L.check(lib.ctx_occ_march_write(p_o, p_d, R, near, far, *grid, L.ptr(ray_off), L.ptr(u), n, L.ptr(ray_id), L.ptr(t), L.ptr(dt),
                                        L.ptr(pts), L.stream()))
        if starts:
            return ray_off, ray_id, t, dt, pts, t - (u if perturb else 0.5) * dt
        return ray_off, ray_id, t, dt, pts

    def select(self, rays_o, rays_d, z_vals):
        """-> idx int32 [n], ascending: the samples r*S + s of z_vals [R,S] whose point rays_o + rays_d * z lies in an occupied
        cell (`ctx_occ_mark`, then the ordered compaction `ctx_texel_compact`).  R*S < 2^31.  Reading n back SYNCS the host: one
        sync per pass of render_rays."""
        if isinstance(z_vals, torch.Tensor) and z_vals.requires_grad:
            raise L.CtxError("OccupancyGrid.select: the selection has no gradient with respect to z_vals; detach them")
        p_o, p_d = L.ptr(rays_o, torch.float32, "rays_o"), L.ptr(rays_d, torch.float32, "rays_d")
        p_z = L.ptr(z_vals, torch.float32, "z_vals")
        if z_vals.dim() != 2 or rays_o.numel() != 3 * z_vals.shape[0] or rays_d.numel() != 3 * z_vals.shape[0]:
            raise L.CtxError(f"OccupancyGrid.select: want rays_o, rays_d [R,3] and z_vals [R,S]; got {tuple(rays_o.shape)}, "
                             f"{tuple(rays_d.shape)}, {tuple(z_vals.shape)}")
        lib = L.load()
        R, S = z_vals.shape
        dev = z_vals.device
        n_ws = lib.ctx_texel_compact_ws_bytes(R * S)
        if n_ws < 0:
            raise L.CtxError(f"OccupancyGrid.select: {R} rays x {S} samples: want 1 <= R*S < 2^31 (int32 sample indices); split the batch")
        mask = torch.empty(R * S, dtype=torch.uint8, device=dev)
        L.check(lib.ctx_occ_mark(p_o, p_d, p_z, R, S, L.ptr(self.cells, torch.uint8, "cells"), self.G, *map(float, self.lo),
                                 *map(float, self.inv), L.ptr(mask), L.stream()))
        ws = torch.empty(n_ws, dtype=torch.uint8, device=dev)
        idx = torch.empty(R * S, dtype=torch.int32, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        L.check(lib.ctx_texel_compact(L.ptr(mask), R * S, L.ptr(idx), L.ptr(count), L.ptr(ws), L.stream()))
        return idx[:int(count.item())].clone()

    def cell_points(self, generator=None):
        """-> pts [G^3,3]: per cell lo + (c + u) * h with u = 0.5 (the centre) or, with a generator, one uniform draw per axis."""
        lib = L.load()
        n = self.G ** 3
        u = torch.rand(n, 3, device=self.cells.device, generator=generator) if generator is not None else None
        pts = torch.empty(n, 3, device=self.cells.device)
        L.ptr(self.cells, torch.uint8, "cells")
        L.check(lib.ctx_occ_cell_points(self.G, *map(float, self.lo), *map(float, self.h), L.ptr(u), L.ptr(pts), L.stream()))
        return pts

    @torch.no_grad()
    def update(self, field, thresh, decay=0.95, generator=None):
        """Refresh from the field: one point per cell (jittered inside it when a generator is given), field.forward_pts without
        gradients, then dens = max(dens * decay, relu(sigma)) and cells = dens > thresh (`ctx_occ_update`)."""
        lib = L.load()
        raw = L.f32c(field.forward_pts(self.cell_points(generator)))
        L.check(lib.ctx_occ_update(L.ptr(raw, torch.float32, "raw"), L.ptr(self.dens, torch.float32, "dens"),
                                   L.ptr(self.cells, torch.uint8, "cells"), self.G ** 3, float(decay), float(thresh), L.stream()))

    def fraction(self):
        """The share of occupied cells, a host float (syncs)."""
        return float(self.cells.count_nonzero().item()) / self.G ** 3


class MeshTracer:
    """Where a ray meets the mesh: per cell of a G^3 grid over the box lo .. hi the list of the triangles that touch it, and the hit kernel
    that walks a ray through the grid and tests the listed triangles (`ctx_mesh_ray_hit`; the rule is written out there, its numpy
    definition is tests/meshhit_rule.py).  vertices float32 [V,3] and faces int64 [F,3] are device tensors in the world frame of the rays,
    as OccupancyGrid.from_mesh takes them; the tracer keeps them as given (it does not follow later changes).  The lists use the
    voxeliser's predicate, so `occupancy` gives from_mesh's grid without a second pass over the mesh.
    Building the lists reads their total length back: one host sync, here; nothing after construction syncs."""

    def __init__(self, vertices, faces, G=64, lo=-1., hi=1.):
        from . import kal
        _check_mesh(vertices, faces, 0, "MeshTracer")
        self.G, self.lo, self.hi, self.inv, self.h = _grid_box(G, lo, hi, "MeshTracer")
        self.device = vertices.device
        L.ptr(vertices, torch.float32, "vertices"), L.ptr(faces, torch.int64, "faces")
        self.faces, self.n_vertices = faces, vertices.shape[0]
        self._pn = self._topology = None
        self.count, self.cell_off, self.cell_tri = kal.mesh_cell_lists(vertices, faces, self.G, self.lo, self.inv)
        self.cells = (self.count > 0).to(torch.uint8).reshape(self.G, self.G, self.G).contiguous()
        self.tri = kal.mesh_tri_records(vertices, faces)

    def _hit(self, who, rays_o, rays_d, near, far, own_face, any_hit):
        from . import kal
        near, far = float(near), float(far)
        if not (near < far and np.isfinite(near) and np.isfinite(far)):
            raise L.CtxError(f"MeshTracer.{who}: want finite near < far, got {near}, {far}")
        return kal.mesh_ray_hit(rays_o, rays_d, near, far, self.cells, self.G, self.lo, self.hi, self.inv, self.h, self.cell_off, self.cell_tri,
                                self.tri, self.faces, own_face=own_face, any_hit=any_hit)

    def trace(self, rays_o, rays_d, near, far, own_face=None):
        """-> (hit u8 [R], t f32 [R], face i64 [R], bary f32 [R,3]): the nearest triangle the ray o + d*t meets within [near, far], ties
        to the lower face id; bary weighs the face's three vertices (1 - u - v, u, v).  A miss: hit = 0, t = far, face = -1, bary = 0.
        Two-sided.  own_face int64 [R] (optional): per ray a face to leave out together with the faces that share a vertex id with it
        (a ray that starts on the surface).  rays_o, rays_d float32 [R,3] device tensors.  No host sync."""
        hit, t, face, uv = self._hit("trace", rays_o, rays_d, near, far, own_face, False)
        bary = torch.stack([1.0 - uv[:, 0] - uv[:, 1], uv[:, 0], uv[:, 1]], dim=1) * hit[:, None]
        return hit, t, face.to(torch.int64), bary

    def occluded(self, rays_o, rays_d, near, far, own_face=None):
        """-> u8 [R]: 1 where the ray meets any triangle within [near, far]: trace's hit, stopping at the first triangle found."""
        return self._hit("occluded", rays_o, rays_d, near, far, own_face, True)

    def _radius(self, who, name, value):
        """A query radius of `closest` as the float32 the kernel takes: finite, > 0 and at most 3 min(h) (a block of at most 7^3 cells)."""
        with np.errstate(all='ignore'):
            r = np.float32(value)
        limit = np.float32(3) * np.min(self.h)
        if not (np.isfinite(r) and r > 0 and r <= limit):
            raise L.CtxError(f"{who}: {name}={value!r} outside (0, 3 min(h)] = (0, {float(limit):g}]: the query looks at the cells within "
                             f"{name} of the point, at most 7^3 of them; use a coarser grid for a longer reach")
        return r

    def closest(self, pts, max_dist):
        """-> (found u8 [n], dist f32 [n], face i64 [n], bary f32 [n,3]): the nearest point of the mesh within max_dist of each of pts
        float32 [n,3] (a device tensor in the tracer's frame): how far it is, on which face it lies (ties to the lower face id) and its
        barycentrics (1 - u - v, u, v) on that face (`ctx_mesh_closest_point`; the rule is written out there, its numpy definition is
        tests/meshdist_rule.py).  A miss: found = 0, dist = max_dist, face = -1, bary = 0.  The distance is unsigned.  max_dist must lie in
        (0, 3 min(h)].  The answer is for the mesh inside the tracer's box: a nearest point outside the box lies in no cell.
        There is no gradient to the positions: a pts that requires grad is refused.  No host sync."""
        from . import kal
        if not isinstance(pts, torch.Tensor) or pts.dim() != 2 or pts.shape[1] != 3:
            raise L.CtxError(f"MeshTracer.closest: want pts [n,3], got {tuple(getattr(pts, 'shape', ()))}")
        if pts.requires_grad:
            raise L.CtxError("MeshTracer.closest: pts requires grad, and the query has no gradient with respect to the positions; detach pts")
        r = self._radius("MeshTracer.closest", "max_dist", max_dist)
        found, dist, face, uv = kal.mesh_closest_point(pts, r, self.G, self.lo, self.inv, self.cell_off, self.cell_tri, self.tri)
        bary = torch.stack([1.0 - uv[:, 0] - uv[:, 1], uv[:, 0], uv[:, 1]], dim=1) * found[:, None]
        return found, dist, face.to(torch.int64), bary

    def pseudonormals(self):
        """-> pn float32 [F,7,3], built on first use and kept: per face its unit normal, the angle-weighted pseudonormals of its three
        vertices and the pseudonormals of its three edges, in the order of signed_distance's feature code (`ctx_mesh_pseudonormals`; the
        rule is written out there, its numpy definition is tests/meshsdf_rule.py).  Building them reads the length of the vertex -> face
        lists back: one host sync, on the first call only."""
        if self._pn is None:
            from . import kal
            vf_off, vf_face = kal.mesh_vertex_faces(self.faces, self.n_vertices)
            self._pn = kal.mesh_pseudonormals(self.faces, self.n_vertices, self.tri, vf_off, vf_face)
        return self._pn

    def topology(self):
        """-> dict(boundary_edges, nonmanifold_edges, inconsistent_edges): how many undirected edges have one face, more than two faces,
        and two faces that traverse them in the same direction (host numbers: this syncs; computed once and kept).  Faces with a vertex
        id outside [0, V) are left out.  The sign of signed_distance means inside / outside only when all three are 0 AND the faces are
        wound outward; an inward-wound mesh inverts the sign, which is the caller's contract and is not detected."""
        if self._topology is None:
            V = self.n_vertices
            f = self.faces[((self.faces >= 0) & (self.faces < V)).all(1)]
            a, b = torch.cat([f[:, 0], f[:, 1], f[:, 2]]), torch.cat([f[:, 1], f[:, 2], f[:, 0]])
            und, inverse, cnt = torch.unique(torch.minimum(a, b) * V + torch.maximum(a, b), return_inverse=True, return_counts=True)
            forward = torch.zeros_like(cnt).index_add_(0, inverse, (a < b).to(cnt.dtype))
            self._topology = dict(boundary_edges=int((cnt == 1).sum()), nonmanifold_edges=int((cnt > 2).sum()),
                                  inconsistent_edges=int(((cnt == 2) & (forward != 1)).sum()))
        return dict(self._topology)

    def signed_distance(self, pts, max_dist):
        """-> (found u8 [n], sdist f32 [n], face i64 [n], bary f32 [n,3], grad f32 [n,3]): `closest` with a sign on the distance, negative
        on the inner side of the surface, and grad = d sdist / d pts, the unit direction from the nearest surface point (times the sign;
        on the surface itself the pseudonormal's direction).  found, |sdist|, face and bary are those of `closest`, bit for bit.  The
        sign is that of (p - q) . N with N the angle-weighted pseudonormal of the face, edge or vertex on which the nearest point q lies
        (`ctx_mesh_signed_distance`; numpy definition: tests/meshsdf_rule.py).  A miss: found = 0, sdist = +max_dist, face = -1,
        bary = 0, grad = 0.  Negative means INSIDE only for a mesh whose `topology()` is all zero and whose faces are wound outward; an
        inward-wound mesh inverts the sign (not detected).  grad is returned, not attached: there is no autograd gradient, and a pts
        that requires grad is refused.  No host sync once the tables exist (`pseudonormals`, built on the first call)."""
        from . import kal
        if not isinstance(pts, torch.Tensor) or pts.dim() != 2 or pts.shape[1] != 3:
            raise L.CtxError(f"MeshTracer.signed_distance: want pts [n,3], got {tuple(getattr(pts, 'shape', ()))}")
        if pts.requires_grad:
            raise L.CtxError("MeshTracer.signed_distance: pts requires grad, and the query has no autograd gradient with respect to the "
                             "positions (grad is returned beside the distance); detach pts")
        r = self._radius("MeshTracer.signed_distance", "max_dist", max_dist)
        found, sdist, face, uv, _, grad = kal.mesh_signed_distance(pts, r, self.G, self.lo, self.inv, self.cell_off, self.cell_tri, self.tri,
                                                                   self.pseudonormals())
        bary = torch.stack([1.0 - uv[:, 0] - uv[:, 1], uv[:, 0], uv[:, 1]], dim=1) * found[:, None]
        return found, sdist, face.to(torch.int64), bary, grad

    def occupancy(self, dilate=1):
        """-> an OccupancyGrid whose cells equal OccupancyGrid.from_mesh(vertices, faces, G, lo, hi, dilate) bit for bit: the cells that
        hold a list, grown by `dilate` cells."""
        if int(dilate) != dilate or dilate < 0:
            raise L.CtxError(f"MeshTracer.occupancy: dilate={dilate}: want a whole number of cells >= 0")
        grid = OccupancyGrid(self.G, self.lo, self.hi, self.device)
        grid.cells = self.cells.clone()
        if dilate > 0:
            grid.dilate(int(dilate))
        return grid

    def stats(self):
        """-> dict(entries, mean_list, max_list): the length of cell_tri, and the mean and the largest list over the cells that hold one
        (host numbers: this syncs)."""
        occupied = self.count[self.count > 0]
        return dict(entries=int(self.cell_tri.numel()), mean_list=float(occupied.float().mean()) if occupied.numel() else 0.0,
                    max_list=int(occupied.max()) if occupied.numel() else 0)


class _MeshTent:
    """The density both mesh-anchored fields share: a tent around the surface, peak * max(0, 1 - dist / width) in float32 with dist the
    tracer's unsigned distance to the mesh (MeshTracer.closest with the query radius width, so dist = width and the density is exactly 0
    on a miss).  width=None: the tracer's largest cell edge; peak=None: 16 / width, so a perpendicular crossing has the optical thickness
    peak * width = 16 and, e^-16 being below 2^-23, the wall is opaque in float32.  The march step must be at most width / 2: a longer
    step can put a single sample, or none, inside the tent, and the quadrature of a crossing then no longer sees the peak."""

    def _init_tent(self, who, tracer, width, peak):
        if not isinstance(tracer, MeshTracer):
            raise L.CtxError(f"{who}: tracer must be a MeshTracer, got {type(tracer).__name__}")
        self.tracer = tracer
        self.width = tracer._radius(who, "width", np.max(tracer.h) if width is None else width)
        with np.errstate(all='ignore'):
            self.peak = np.float32(16) / self.width if peak is None else np.float32(peak)
        if not (np.isfinite(self.peak) and self.peak > 0):
            raise L.CtxError(f"{who}: peak={peak!r}: want a finite density > 0")

    @torch.no_grad()
    def _tent(self, pts):
        """pts [n,3] float32 contiguous -> (density [n], found, face, bary): d = dist / width; peak * max(0, 1 - d), each operation rounding
        on its own (the divisor is a device scalar: a true division, not a product with a host reciprocal)."""
        found, dist, face, bary = self.tracer.closest(pts, self.width)
        d = dist / dist.new_full((), float(self.width))
        return float(self.peak) * (1.0 - d).clamp_min(0.0), found, face, bary


class MeshDensityField(torch.nn.Module, _MeshTent):
    """A field whose geometry is the mesh's: `inner`'s colour with the density channel replaced by a fixed function of the distance to the
    mesh (the tent of _MeshTent), so only colour is trained: no floaters, no mask or depth weight to tune, and a bake reads the colour at
    the surface.  inner: any field the marched path takes (forward_pts), e.g. a HashGridField; tracer: a MeshTracer of the mesh, in the
    frame of the points.  width=None: the tracer's largest cell edge; peak=None: 16 / width.  THE MARCH STEP MUST BE AT MOST width / 2.
    forward_pts(pts [..., 3]) -> inner.forward_pts(pts) with channel 3 replaced; the density carries no gradient (inner's output row for
    channel 3 gets a gradient of exactly zero), the colour channels carry theirs through inner unchanged.  view_dependent and forward_dirs
    pass through to an inner that has them, with the same replacement.  modules() / parameters() expose inner, so field_optimizer,
    FieldAdam, fit_views, OccupancyGrid.update and bake_atlas take it as they take any field.  It has no density_gradient:
    render_normals refuses it (the normals of this field are the mesh's)."""

    def __init__(self, inner, tracer, width=None, peak=None):
        super().__init__()
        if not callable(getattr(inner, 'forward_pts', None)):
            raise L.CtxError(f"MeshDensityField: inner ({type(inner).__name__}) has no forward_pts")
        self.inner = inner
        self._init_tent("MeshDensityField", tracer, width, peak)

    @property
    def view_dependent(self):
        return bool(getattr(self.inner, 'view_dependent', False))

    def _replace(self, raw, pts):
        if raw.shape[-1] != 4:
            raise L.CtxError(f"MeshDensityField: inner returned {tuple(raw.shape)}, expected [..., 4] (colour and density)")
        x = L.f32c(pts.detach()).reshape(-1, 3)
        if x.shape[0] == 0:
            return raw
        dens = self._tent(x)[0].reshape(*raw.shape[:-1], 1)
        return torch.cat([raw[..., :3], dens.to(raw.dtype)], dim=-1)

    def forward_pts(self, pts):
        """pts [..., 3] -> raw [..., 4]: inner's colour logits, the tent's density."""
        return self._replace(self.inner.forward_pts(pts), pts)

    forward = forward_pts

    def forward_dirs(self, pts, rays_d, ray_id, return_residual=False):
        """inner.forward_dirs with channel 3 replaced (an inner without forward_dirs is refused)."""
        if not callable(getattr(self.inner, 'forward_dirs', None)):
            raise L.CtxError(f"MeshDensityField.forward_dirs: inner ({type(self.inner).__name__}) has no forward_dirs")
        raw, res = self.inner.forward_dirs(pts, rays_d, ray_id, return_residual=True)
        raw = self._replace(raw, pts)
        return (raw, res) if return_residual else raw


class MeshSolidField(torch.nn.Module):
    """MeshDensityField's sibling with a side: `inner`'s colour, and a density that is zero outside the mesh and rises only inside it, the
    one-sided ramp peak * min(1, max(0, -sdist / width)) of the tracer's SIGNED distance (MeshTracer.signed_distance with the query
    radius width: d = sdist / width is a true float32 division by a device scalar, then the clamp, then the product).  The density is
    exactly 0 outside and on the surface, reaches peak at depth width, and is 0 on a miss (sdist = +width).  A ray that misses the mesh
    composites to nothing: the silhouette is the mesh's, with no halo of half a tent outside it.  Marched path only.
    width=None: the tracer's largest cell edge; peak=None: 32 / width.  THE MARCH STEP MUST BE AT MOST width / 2.
    The query radius is width, so a point deeper than width inside the mesh is a miss and has the density 0 again: the solid is a wall
    of thickness width under the surface, a ramp from 0 at the surface to peak at its inner face (the min(1, .) binds only there).
    Why 32: a perpendicular crossing of the wall has the optical thickness peak * width / 2 = 16, the tent's (two halves of
    peak' * width / 2 with peak' = 16 / width).  The quadrature, for intervals of length dt <= width / 2: the march's midpoint rule is
    exact on a linear piece, so an interval loses only where it straddles an end of the ramp.  At the foot, if a part a of the interval
    lies inside, the true integral there is (peak / width) a^2 / 2 and the midpoint gives dt (peak / width) max(0, a - dt / 2); the
    difference is at most (peak / width) dt^2 / 8 <= peak * width / 32 = 1.  At the inner face an interval whose midpoint falls beyond
    it loses the integral of the ramp over at most dt / 2 <= width / 4, where the ramp lies between 3/4 peak and peak: at most
    7/32 peak * width = 7.  So one wall keeps an optical thickness >= 16 - 1 - 7 = 8 on a perpendicular crossing, and more on an oblique
    one (the path grows with 1 / |cos|, the two losses do not); a ray that enters a closed mesh leaves it through a second wall, so it
    keeps >= 16 and acc >= 1 - e^-16 > 1 - 2^-20.  (A single wall alone, e.g. of an open mesh under allow_open, guarantees 1 - e^-8.)
    Why tracer.occupancy(1) holds the whole wall when width <= min(h): the density is positive only at points within width of the
    surface; such a point is within width <= min(h) of a cell the voxeliser marks, i.e. in that cell or in one of its neighbours, which
    occupancy(1) adds.
    forward_pts(pts [..., 3]) -> inner.forward_pts(pts) with channel 3 replaced; the density carries no gradient (inner's output row for
    channel 3 gets a gradient of exactly zero), the colour channels carry theirs through inner unchanged.  view_dependent and forward_dirs
    pass through to an inner that has them.  modules() / parameters() expose inner, so field_optimizer, FieldAdam, fit_views,
    OccupancyGrid.update and bake_atlas take it as any field.  density_gradient gives the ramp's gradient with respect to the positions,
    so render_normals takes it too: its normals are the mesh's.
    The sign means inside / outside only for a closed, consistently oriented mesh wound outward: a tracer whose topology() is not all
    zero is refused unless allow_open=True (one host sync, at construction).  An inward-wound mesh gives a solid OUTSIDE; not detected."""

    def __init__(self, inner, tracer, width=None, peak=None, allow_open=False):
        super().__init__()
        if not callable(getattr(inner, 'forward_pts', None)):
            raise L.CtxError(f"MeshSolidField: inner ({type(inner).__name__}) has no forward_pts")
        if not isinstance(tracer, MeshTracer):
            raise L.CtxError(f"MeshSolidField: tracer must be a MeshTracer, got {type(tracer).__name__}")
        self.inner, self.tracer = inner, tracer
        self.width = tracer._radius("MeshSolidField", "width", np.max(tracer.h) if width is None else width)
        with np.errstate(all='ignore'):
            self.peak = np.float32(32) / self.width if peak is None else np.float32(peak)
        if not (np.isfinite(self.peak) and self.peak > 0):
            raise L.CtxError(f"MeshSolidField: peak={peak!r}: want a finite density > 0")
        topo = tracer.topology()
        if any(topo.values()) and not allow_open:
            raise L.CtxError(f"MeshSolidField: the mesh is not closed and consistently oriented ({topo}): the signed distance has no inside; "
                             "pass allow_open=True to take its sign as it comes")
        tracer.pseudonormals()

    @property
    def view_dependent(self):
        return bool(getattr(self.inner, 'view_dependent', False))

    @torch.no_grad()
    def _ramp(self, pts):
        """pts [n,3] float32 contiguous -> (density [n], sdist [n], grad [n,3]): d = sdist / width; peak * min(1, max(0, -d))."""
        _, sdist, _, _, grad = self.tracer.signed_distance(pts, self.width)
        d = sdist / sdist.new_full((), float(self.width))
        return float(self.peak) * (-d).clamp(0.0, 1.0), sdist, grad

    def _replace(self, raw, pts):
        if raw.shape[-1] != 4:
            raise L.CtxError(f"MeshSolidField: inner returned {tuple(raw.shape)}, expected [..., 4] (colour and density)")
        x = L.f32c(pts.detach()).reshape(-1, 3)
        if x.shape[0] == 0:
            return raw
        dens = self._ramp(x)[0].reshape(*raw.shape[:-1], 1)
        return torch.cat([raw[..., :3], dens.to(raw.dtype)], dim=-1)

    def forward_pts(self, pts):
        """pts [..., 3] -> raw [..., 4]: inner's colour logits, the ramp's density."""
        return self._replace(self.inner.forward_pts(pts), pts)

    forward = forward_pts

    def forward_dirs(self, pts, rays_d, ray_id, return_residual=False):
        """inner.forward_dirs with channel 3 replaced (an inner without forward_dirs is refused)."""
        if not callable(getattr(self.inner, 'forward_dirs', None)):
            raise L.CtxError(f"MeshSolidField.forward_dirs: inner ({type(self.inner).__name__}) has no forward_dirs")
        raw, res = self.inner.forward_dirs(pts, rays_d, ray_id, return_residual=True)
        raw = self._replace(raw, pts)
        return (raw, res) if return_residual else raw

    @torch.no_grad()
    def density_gradient(self, pts, channel=3, return_raw=False):
        """pts [..., 3] -> grad [..., 3] = d raw[..., 3] / d pts, and with return_raw=True (raw [..., 4], grad), HashGridField's
        convention: (-(peak / width)) * (d sdist / d pts) where -width < sdist < 0, and 0 elsewhere (outside, on the surface, on the
        plateau, on a miss); peak / width is rounded once, in float32.  It points inward, so render_normals' -grad / |grad| is the
        outward unit direction from the nearest surface point.  Only the density has a closed form: any other channel is refused.  No
        autograd is involved; the ambient grad mode plays no part."""
        if isinstance(channel, bool) or not isinstance(channel, (int, np.integer)) or channel != 3:
            raise L.CtxError(f"MeshSolidField.density_gradient: channel={channel!r}: only channel 3, the density, has a gradient with respect "
                             "to the positions here (the colour is inner's)")
        if not isinstance(pts, torch.Tensor) or pts.dim() < 1 or pts.shape[-1] != 3:
            raise L.CtxError(f"MeshSolidField.density_gradient: want pts [..., 3], got {tuple(getattr(pts, 'shape', ()))}")
        x = L.f32c(pts.detach()).reshape(-1, 3)
        if x.shape[0] == 0:
            grad = torch.zeros(*pts.shape[:-1], 3, device=x.device)
            return (torch.zeros(*pts.shape[:-1], 4, device=x.device), grad) if return_raw else grad
        dens, sdist, g = self._ramp(x)
        on = (sdist > -float(self.width)) & (sdist < 0)
        grad = torch.where(on[:, None], float(-(self.peak / self.width)) * g, torch.zeros_like(g)).reshape(*pts.shape[:-1], 3)
        if not return_raw:
            return grad
        raw = self.inner.forward_pts(x).detach()
        return torch.cat([raw[:, :3], dens[:, None]], dim=1).reshape(*pts.shape[:-1], 4), grad


class AtlasField(torch.nn.Module, _MeshTent):
    """The atlas-to-field direction: a painted atlas read at each point's nearest surface point, a field the ray path can render
    (render_image(march=)) and fit_views can distil from.  No parameters.  tracer: a MeshTracer of the mesh; face_uv float32 [F,3,2]
    (vt[ft]); atlas float32 [3,T,T] in [0,1]; all on the tracer's device.
    forward_pts(pts [..., 3]) -> raw [..., 4]: with (found, dist, face, bary) = tracer.closest(pts, width), the colour is the atlas
    sampled bilinearly (kal.render.mesh.texture_mapping) at uv = (bary_0 face_uv[face,0] + bary_1 face_uv[face,1]) + bary_2
    face_uv[face,2], clamped to [2^-12, 1 - 2^-12] and returned as its logit, since compositing applies a sigmoid; the density is the
    tent of _MeshTent.  A miss gives colour logit 0 and density 0.  THE MARCH STEP MUST BE AT MOST width / 2.  Marched path only."""
    CLAMP = 2.0 ** -12

    def __init__(self, tracer, face_uv, atlas, width=None, peak=None):
        super().__init__()
        self._init_tent("AtlasField", tracer, width, peak)
        F = tracer.faces.shape[0]
        if not isinstance(face_uv, torch.Tensor) or tuple(face_uv.shape) != (F, 3, 2) or face_uv.dtype != torch.float32:
            raise L.CtxError(f"AtlasField: want face_uv float32 [{F},3,2], got {getattr(face_uv, 'dtype', type(face_uv).__name__)} "
                             f"{tuple(getattr(face_uv, 'shape', ()))}")
        if not isinstance(atlas, torch.Tensor) or atlas.dim() != 3 or atlas.shape[0] != 3 or atlas.shape[1] != atlas.shape[2] \
                or atlas.dtype != torch.float32:
            raise L.CtxError(f"AtlasField: want atlas float32 [3,T,T], got {getattr(atlas, 'dtype', type(atlas).__name__)} "
                             f"{tuple(getattr(atlas, 'shape', ()))}")
        L.ptr(face_uv, torch.float32, "face_uv"), L.ptr(atlas, torch.float32, "atlas")
        self.face_uv, self.atlas = face_uv, atlas

    @torch.no_grad()
    def forward_pts(self, pts):
        from . import kal
        if not isinstance(pts, torch.Tensor) or pts.dim() < 1 or pts.shape[-1] != 3:
            raise L.CtxError(f"AtlasField: want pts [..., 3], got {tuple(getattr(pts, 'shape', ()))}")
        x = L.f32c(pts.detach()).reshape(-1, 3)
        if x.shape[0] == 0:
            return torch.zeros(*pts.shape[:-1], 4, device=x.device)
        dens, found, face, bary = self._tent(x)
        fuv = self.face_uv[face.clamp_min(0)]
        uv = (bary[:, 0:1] * fuv[:, 0] + bary[:, 1:2] * fuv[:, 1]) + bary[:, 2:3] * fuv[:, 2]
        col = kal.render.mesh.texture_mapping(uv[None].contiguous(), self.atlas[None])[0]
        logit = torch.logit(col.clamp(self.CLAMP, 1.0 - self.CLAMP))
        logit = torch.where(found[:, None] != 0, logit, torch.zeros_like(logit))
        return torch.cat([logit, dens[:, None]], dim=1).reshape(*pts.shape[:-1], 4)

    forward = forward_pts


def _mesh_targets(who, mesh, mask_weight, depth_weight, rays_o, rays_d, near, far):
    """The (hit, t) pair the mask and depth terms are measured against, or None when neither term is on: from a MeshTracer (traced here,
    without gradients) or a pair traced beforehand for the same rays."""
    for name, w in (("mask_weight", mask_weight), ("depth_weight", depth_weight)):
        if not w >= 0.:
            raise L.CtxError(f"{who}: {name}={w}: want a weight >= 0")
        if w > 0. and mesh is None:
            raise L.CtxError(f"{who}: {name}={w} needs mesh=: a MeshTracer of the mesh the views show")
    if mesh is None or (mask_weight == 0. and depth_weight == 0.):
        return None
    if isinstance(mesh, (tuple, list)):
        hit, t = mesh
    else:
        with torch.no_grad():
            hit, t = mesh.trace(rays_o, rays_d, near, far)[:2]
    R = rays_o.shape[0]
    if tuple(hit.shape) != (R,) or tuple(t.shape) != (R,):
        raise L.CtxError(f"{who}: mesh= wants hit [{R}] and t [{R}] for these rays, got {tuple(hit.shape)} and {tuple(t.shape)}")
    return hit, t


@torch.no_grad()
def render_image(field, H, W, K, c2w, near, far, N_samples, white_bkgd=False, rows=None, N_importance=0, occupancy=None, clip=False,
                 march=None, resample=0):
    """-> dict(rgb [h,W,3], depth [h,W], acc [h,W], disp [h,W]) for the row range `rows` (default: all).
    N_importance > 0 adds nerf-pytorch's hierarchical pass (render_rays: sample_pdf(det=True) on the coarse weights, merged
    and sorted with the coarse samples, evaluated by the same field).  occupancy: an OccupancyGrid; clip: samples between each
    ray's first and last occupied cell; see render_rays.  march: a world-space step; the samples are then the ragged lists of
    occupancy.march (render_rays_marched) and N_samples is unused.  resample: with march, the fine samples per hit ray of the
    importance-resampled second pass (render_rays_marched); 0: none."""
    ro, rd = rnh.get_rays(H, W, K, c2w)
    r0, r1 = (0, H) if rows is None else rows
    ro, rd = ro[r0:r1].reshape(-1, 3), rd[r0:r1].reshape(-1, 3)
    rgb, disp, acc, wts, depth = rnh.render_rays(field, ro, rd, near, far, N_samples, white_bkgd=white_bkgd, N_importance=N_importance,
                                                 occupancy=occupancy, clip=clip, march=march, resample=resample)
    h = r1 - r0
    return {'rgb': rgb.reshape(h, W, 3), 'depth': depth.reshape(h, W), 'acc': acc.reshape(h, W), 'disp': disp.reshape(h, W)}


@torch.no_grad()
def render_normals(field, H, W, K, c2w, near, far, occupancy, march, rows=None):
    """-> dict(normal [h,W,3], z_normal [h,W], acc [h,W], depth [h,W]) for the row range `rows` (default: all): the normals of the field's
    density, rendered as the colour is, on the marched lists only (occupancy and march as render_rays_marched takes them, no jitter).
    field: anything with density_gradient(pts, return_raw=True) -> (raw [n,4], grad [n,3]), e.g. a HashGridField.
    Per sample n_i = -grad_i / max(|grad_i|, 1e-12); per ray N = sum_i w_i n_i with the compositing weights (rnh.weighted_sum_packed: one
    summation order, no atomics) and normal = N / max(|N|, 1e-12), in the world frame; 0 where the ray has no samples.
    z_normal = clamp((c2w[:3,:3]^T normal)_z, 0, 1): the camera looks down -z (get_rays), so a surface that faces the camera has a positive
    value, the convention the painting side's z_normals follow.  One host sync (the march's n).  No gradient flows through any of it."""
    if not callable(getattr(field, 'density_gradient', None)):
        raise L.CtxError(f"render_normals: {type(field).__name__} has no density_gradient(pts, return_raw=True): the normals are the field's "
                         "gradient with respect to the positions, which this field does not give (a HashGridField does)")
    if occupancy is None or march is None:
        raise L.CtxError("render_normals: the marched path only: want an occupancy grid (occupancy=) and a world-space step (march=)")
    ro, rd = rnh.get_rays(H, W, K, c2w)
    r0, r1 = (0, H) if rows is None else rows
    h = r1 - r0
    ro, rd = ro[r0:r1].reshape(-1, 3), rd[r0:r1].reshape(-1, 3)
    ray_off, _, t, dt, pts = occupancy.march(ro, rd, near, far, march)
    if t.numel():
        raw, g = field.density_gradient(pts, return_raw=True)
        raw, g = L.f32c(raw), L.f32c(g)
    else:
        raw, g = torch.empty(0, 4, device=ro.device), torch.empty(0, 3, device=ro.device)
    _, _, acc, weights, depth = rnh.raw2outputs_packed(raw, t, dt, rd, ray_off)
    n_i = -g / g.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    N = rnh.weighted_sum_packed(weights, n_i.contiguous(), ray_off)
    normal = N / N.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    z = (normal * L.f32c(c2w[:3, 2]).to(normal.device)).sum(-1).clamp(0, 1)              # (R^T normal)_z = R[:, 2] . normal
    return {'normal': normal.reshape(h, W, 3), 'z_normal': z.reshape(h, W), 'acc': acc.reshape(h, W), 'depth': depth.reshape(h, W)}


def gather_rows(tile, H, group=None):
    """all_gather of the ranks' row tiles [h_r, ...] -> [H, ...] (ragged tiles padded to the largest)."""
    if not (dist.is_initialized() and dist.get_world_size(group) > 1):
        return tile
    world = dist.get_world_size(group)
    hmax = -(-H // world)
    pad = torch.zeros((hmax,) + tuple(tile.shape[1:]), dtype=tile.dtype, device=tile.device)
    pad[:tile.shape[0]] = tile
    parts = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(parts, pad, group=group)
    out = []
    for r in range(world):
        r0, r1 = shard_rows(H, r, world)
        out.append(parts[r][:r1 - r0])
    return torch.cat(out, 0)


def depth_for_diffusion(depth, acc, thresh=0.5):
    """Rendered z-depth -> the depth-map convention img2img_step receives from the raster path (render.py:48-74):
    foreground in [0.5, 1] with closer = larger, background 0."""
    fg = acc > thresh
    out = torch.zeros_like(depth)
    if fg.any():
        d = depth[fg]
        lo, hi = d.min(), d.max()
        out[fg] = 1.0 - 0.5 * (d - lo) / (hi - lo).clamp_min(1e-8)
    return out


@torch.no_grad()
def render_and_refine(field, sd, text_z, H, W, c2w, near=0.5, far=2.5, N_samples=128, guidance_scale=7.5, strength=1.0,
                      num_inference_steps=50, fixed_seed=0, image_size=512, rank=0, world=1, group=None, occupancy=None, clip=False,
                      march=None, resample=0):
    """configs[4] end to end on this rank's rows; every rank returns the refined image [1,3,S,S] and the gathered render.
    occupancy, clip: an OccupancyGrid for the render and whether the samples are placed inside its spans (render_rays).
    march: a world-space step for the render's ragged sample lists (render_rays_marched); N_samples is then unused.  resample: with
    march, the fine samples per hit ray of the resampled second pass."""
    K = pinhole(H, W)
    tile = render_image(field, H, W, K, c2w, near, far, N_samples, rows=shard_rows(H, rank, world), occupancy=occupancy,
                        clip=clip, march=march, resample=resample)
    rgb = gather_rows(tile['rgb'], H, group)
    depth = gather_rows(tile['depth'], H, group)
    acc = gather_rows(tile['acc'], H, group)
    dmap = depth_for_diffusion(depth, acc)[None, None]
    img = rgb.permute(2, 0, 1)[None].clamp(0, 1).contiguous()
    mask = torch.ones_like(dmap)
    refined, _ = sd.img2img_step(text_z, img, dmap, guidance_scale=guidance_scale, strength=strength,
                                 num_inference_steps=num_inference_steps, update_mask=mask, fixed_seed=fixed_seed,
                                 image_size=image_size)
    return refined, {'rgb': rgb, 'depth': depth, 'acc': acc}


def train_step(field, optimizer, rays_o, rays_d, target_rgb, near, far, N_samples, N_importance=0, perturb=1., raw_noise_std=0.,
               white_bkgd=False, generator=None, occupancy=None, clip=False, march=None, distortion=0., resample=0, view_residual=0.,
               mesh=None, mask_weight=0., depth_weight=0.):
    """nerf-pytorch's training step on one ray batch: render (one field for the coarse and the fine pass, as render_image),
    loss = img2mse(rgb_fine, target) (+ img2mse(rgb_coarse, target) when hierarchical), backward, optimizer.step().
    rays_o, rays_d, target_rgb: [R,3].  -> dict(loss, psnr) of device scalars (psnr of the fine image); no host sync.
    occupancy: an OccupancyGrid (render_rays): the field runs, and keeps activations, on the occupied samples only, at one
    host sync per pass.  A batch in which no pass has an occupied sample has a loss without a graph: backward and the
    optimizer step are skipped and loss / psnr are still returned.  clip=True places the samples between each ray's first and
    last occupied cell (render_rays).  march: a world-space step; the batch is rendered from the ragged lists of occupancy.march
    (render_rays_marched: no [R,S] tensor, one host sync), N_samples is unused, and a batch with n = 0 skips backward and the step
    in the same way.
    distortion > 0 adds distortion * mean over the rays of rnh.distortion_loss (mip-NeRF 360's regulariser, which pulls each ray's
    weights together): on the march path of the weights and lists the render returned, otherwise of the fine pass's weights and final
    z_vals.  The dict then gains 'distortion', the unweighted mean, detached.  distortion = 0 (the default) runs nothing new.
    resample=K > 0 (needs march): the march is the coarse pass and every hit ray gets K fine samples drawn from its detached coarse
    weights (render_rays_marched); the loss is img2mse(fine) + img2mse(coarse), the distortion loss acts on the fine weights and lists,
    and the step costs a second host sync.
    A view-dependent field (hashgrid.ViewDependentField) trains on the marched lists only: without march= it is refused.
    view_residual > 0 (such a field only) adds view_residual * mean(res^2) over the samples of every pass, res being the field's colour
    residual: the term pulls colour into the base term, which is what the grid refresh, the normals and a 'diffuse' bake read.  The dict
    then gains 'view_residual', the unweighted mean, detached.  0 (the default) runs nothing new.
    mesh: a MeshTracer of the mesh the target views show, for the two geometry terms: mask_weight > 0 adds mask_weight * mean((acc - hit)^2)
    and depth_weight > 0 adds depth_weight * sum over the rays that hit of (depth - t_mesh)^2 / max(1, n_hit), with (hit, t_mesh) the
    tracer's answer for these rays within [near, far] and acc, depth those of the pass that carries the image loss (the fine pass when
    hierarchical or resampled); on the dense path and on the march path alike.  The dict then gains 'mask' and 'depth', the unweighted
    means, detached.  mesh may also be the pair (hit u8 [R], t [R]) traced beforehand for these rays (fit_views traces once).  With both
    weights 0 (the default) nothing new runs, with or without a tracer; a weight > 0 without mesh= is refused."""
    targets = _mesh_targets("train_step", mesh, mask_weight, depth_weight, rays_o, rays_d, near, far)
    if not distortion >= 0.:
        raise L.CtxError(f"train_step: distortion={distortion}: want a weight >= 0")
    if not view_residual >= 0.:
        raise L.CtxError(f"train_step: view_residual={view_residual}: want a weight >= 0")
    if view_residual > 0. and not getattr(field, 'view_dependent', False):
        raise L.CtxError(f"train_step: view_residual={view_residual} weighs the colour residual of a view-dependent field; "
                         f"{type(field).__name__} has none")
    if march is None:
        rnh._refuse_view_dependent(field, "train_step")
    optimizer.zero_grad(set_to_none=True)
    out, extras = rnh.render_rays(field, rays_o, rays_d, near, far, N_samples, white_bkgd=white_bkgd, perturb=perturb,
                                  raw_noise_std=raw_noise_std, N_importance=N_importance, generator=generator,
                                  return_extras=True, occupancy=occupancy, clip=clip, march=march, resample=resample)
    target = target_rgb.reshape(-1, 3)
    img_loss = rnh.img2mse(out[0], target)
    loss = img_loss
    if 'rgb0' in extras:
        loss = loss + rnh.img2mse(extras['rgb0'], target)
    dloss = None
    if distortion > 0.:
        if march is not None:
            dloss = rnh.distortion_loss(out[3], extras['t'], extras['dt'], rays_d, extras['ray_off']).mean()
        else:
            dloss = rnh.distortion_loss(out[3], extras['z_vals'], None, rays_d).mean()
        loss = loss + distortion * dloss
    vloss = None
    if view_residual > 0.:
        parts = [extras[k] for k in ('residual0', 'residual') if k in extras]
        count = sum(p.numel() for p in parts)
        vloss = sum((p * p).sum() for p in parts) / count if count else torch.zeros((), device=loss.device)
        loss = loss + view_residual * vloss
    mloss = zloss = None
    if targets is not None:
        hit = targets[0].to(out[2].dtype)
        mloss = ((out[2] - hit) ** 2).mean()
        zloss = (hit * (out[4] - targets[1]) ** 2).sum() / hit.sum().clamp(min=1.)
        if mask_weight > 0.:
            loss = loss + mask_weight * mloss
        if depth_weight > 0.:
            loss = loss + depth_weight * zloss
    if occupancy is None or loss.requires_grad:
        loss.backward()
        optimizer.step()
    res = {'loss': loss.detach(), 'psnr': rnh.mse2psnr(img_loss.detach()).reshape(())}
    if dloss is not None:
        res['distortion'] = dloss.detach()
    if vloss is not None:
        res['view_residual'] = vloss.detach()
    if mloss is not None:
        res['mask'], res['depth'] = mloss.detach(), zloss.detach()
    return res


def fit_views(field, images, c2ws, K, near, far, iters, rays_per_iter=4096, lr=5e-4, seed=0, N_samples=64, N_importance=0,
              perturb=1., raw_noise_std=0., white_bkgd=False, occupancy=None, occupancy_every=16, occupancy_warmup=32,
              occupancy_thresh=0.01, clip=False, march=None, distortion=0., resample=0, optimizer='torch', table_lr=None, view_residual=0.,
              mesh=None, mask_weight=0., depth_weight=0.):
    """Distil posed views into the 3-D field: images [V,H,W,3] in [0,1], c2ws [V,3,4], K the pinhole matrix of get_rays.
    Every iteration draws rays_per_iter pixels over all views with a generator seeded by `seed` (which also drives the jitter
    and the noise, so a run repeats exactly) and runs train_step with torch.optim.Adam(lr).  -> the loss history (floats).
    The views can be renders of a painted mesh: TexturedMeshModel.render on a white background (pass white_bkgd=True then)
    with the camera-to-world matrices of the same poses.
    occupancy: an OccupancyGrid handed to every train_step.  It stays as given for the first occupancy_warmup iterations; from
    then on occupancy.update(field, occupancy_thresh) runs before iterations occupancy_warmup, occupancy_warmup + occupancy_every,
    ...  The jitter of the cell points comes from the same generator, so a run still repeats exactly.  occupancy_thresh is a
    density (the default 0.01 is instant-ngp's minimum optical thickness per unit length).
    occupancy_every=0: a static grid, never refreshed.  This is how a grid made from the mesh (OccupancyGrid.from_mesh) is used: the
    surface is known before the first iteration and must not be overwritten by the student's density.  clip=True places every ray's
    samples between its first and last occupied cell (render_rays).  march: a world-space step handed to every train_step: the
    samples are the ragged lists of occupancy.march, N_samples is unused, and the refresh schedule stays as it is (the grid may
    change between iterations and the march follows it).  distortion: the weight of the distortion loss, handed to every train_step.
    resample: with march, the fine samples per hit ray of the resampled second pass, handed to every train_step.
    view_residual: the weight of a view-dependent field's residual penalty, handed to every train_step (such a field needs march=).
    optimizer: 'torch' (torch.optim.Adam) or 'fused' (optim.FieldAdam: the step is HIP, the tables of the field's hash-grid encodings are
    in a group of their own with sparse=True and take their step straight from the backward's integer sums; a field without a table
    simply gets the HIP step).  table_lr: with either optimizer, the rate of that group of tables (None: lr).  The defaults build
    torch.optim.Adam(field.parameters(), lr) as before.
    mesh, mask_weight, depth_weight: a MeshTracer of the mesh the views show and the weights of train_step's mask and depth terms.  With a
    weight > 0 all V*H*W rays are traced once before the loop and every iteration hands its rays' (hit, t) down; with both 0 (the
    default) nothing is traced and nothing new is handed down."""
    if optimizer not in ('torch', 'fused'):
        raise L.CtxError(f"fit_views: optimizer={optimizer!r}: want 'torch' or 'fused'")
    if table_lr is not None and not table_lr > 0:
        raise L.CtxError(f"fit_views: table_lr={table_lr!r}: want a rate > 0, or None for lr")
    dev = next(field.parameters()).device
    images = images.to(device=dev, dtype=torch.float32)
    V, H, W, _ = images.shape
    rays = [rnh.get_rays(H, W, K, c2ws[v].to(dev)) for v in range(V)]
    ro = torch.stack([r[0] for r in rays]).reshape(-1, 3)
    rd = torch.stack([r[1] for r in rays]).reshape(-1, 3)
    target = images.reshape(-1, 3)
    gen = torch.Generator(device=dev).manual_seed(seed)
    traced = _mesh_targets("fit_views", mesh, mask_weight, depth_weight, ro, rd, near, far)
    opt = field_optimizer(field, lr, optimizer, table_lr)
    hist = []
    try:
        for it in range(iters):
            if occupancy is not None and occupancy_every != 0 and it >= occupancy_warmup and (it - occupancy_warmup) % occupancy_every == 0:
                occupancy.update(field, occupancy_thresh, generator=gen)
            idx = torch.randint(0, ro.shape[0], (rays_per_iter,), device=dev, generator=gen)
            step = train_step(field, opt, ro[idx], rd[idx], target[idx], near, far, N_samples, N_importance=N_importance,
                              perturb=perturb, raw_noise_std=raw_noise_std, white_bkgd=white_bkgd, generator=gen,
                              occupancy=occupancy, clip=clip, march=march, distortion=distortion, resample=resample,
                              view_residual=view_residual,
                              **({} if traced is None else dict(mesh=(traced[0][idx], traced[1][idx]), mask_weight=mask_weight,
                                                               depth_weight=depth_weight)))
            hist.append(step['loss'])
    finally:
        if optimizer == 'fused':
            opt.release()
    return torch.stack(hist).tolist()


def field_optimizer(field, lr, optimizer='torch', table_lr=None, deferred=True):
    """fit_views' optimizer.  'torch' with table_lr=None: torch.optim.Adam(field.parameters(), lr), one group.  Otherwise the tables of the
    field's hash-grid encodings form a first group at table_lr (None: lr), everything else a second at lr (a group that would be empty
    is left out).  'fused': optim.FieldAdam with sparse=True on the group of tables and, with deferred=True, the encodings in deferred
    mode: call release() on it when training ends."""
    from .hashgrid import HashGridEncoding, HashGridEncoding2D
    from .optim import FieldAdam
    if optimizer == 'torch' and table_lr is None:
        return torch.optim.Adam(field.parameters(), lr=lr)
    encodings = [m for m in field.modules() if isinstance(m, (HashGridEncoding, HashGridEncoding2D))]
    tables = [e.table for e in encodings]
    rest = [p for p in field.parameters() if not any(p is t for t in tables)]
    groups = []
    if tables:
        groups.append(dict(params=tables, lr=lr if table_lr is None else table_lr, **(dict(sparse=True) if optimizer == 'fused' else {})))
    if rest:
        groups.append(dict(params=rest, lr=lr))
    if optimizer == 'torch':
        return torch.optim.Adam(groups, lr=lr)
    return FieldAdam(groups, lr=lr, encodings=encodings if deferred else ())


def _checked_bake_texels(texels, T):
    """A texel list handed to bake_atlas: int32 [n] device tensor of DISTINCT texels inside the atlas (looking costs a host sync)."""
    L.ptr(texels, torch.int32, "texels")
    if texels.dim() != 1:
        raise L.CtxError(f"bake_atlas: texels must be a 1-D int32 list, got shape {tuple(texels.shape)}")
    n = texels.numel()
    if n > T * T:
        raise L.CtxError(f"bake_atlas: texels holds {n} entries for a {T} x {T} atlas")
    if n:
        lo, hi = int(texels.min()), int(texels.max())
        if lo < 0 or hi >= T * T:
            raise L.CtxError(f"bake_atlas: texels span [{lo}, {hi}], outside the {T} x {T} atlas [0, {T * T})")
        if int(torch.unique(texels).numel()) != n:
            raise L.CtxError("bake_atlas: texels names a texel twice: the resolve adds without atomics, one writer per texel")
    return texels


@torch.no_grad()
def bake_atlas(field, vertices, faces, face_uv, texel_face, texel_bary, occupancy, step=None, shell=None, supersample=1, min_alpha=0.5,
               texels=None, rays_per_chunk=1 << 20, acc=None, colour='view', visibility=None):
    """Bakes a 3-D field into the mesh's UV atlas -> acc int64 [4,T,T] in units of 2^-32 (added to when given), what the painting side
    accumulates: kal.fixed_to_float(acc)[:3] / [3] is the colour, [3] > 0 the coverage, so dist.merge_atlas' conversion, complete_atlas,
    _painted_texture and export apply unchanged.
    Every texel of the list marches a short ray down its face normal through the field, as NeRF-to-mesh exporters do: per chunk of at most
    rays_per_chunk rays (whole texels only) kal.texel_rays places supersample^2 rays per texel `shell` outside the surface,
    rnh.render_rays_marched composites them over [0, 2 shell] with samples `step` apart inside the occupied cells (no jitter, no white
    background), and kal.bake_resolve folds the sub-samples whose mean alpha >= min_alpha into the sums.  Invalid rows (a face without
    area) are marched like any other, find no sample and are dropped by the resolve: no compaction, one host sync per chunk (the march's).
    field: anything render_rays_marched takes (forward_pts).  vertices [V,3] f32 and faces [F,3] i64 in the world frame of the field,
    face_uv [F,3,2] f32 (vt[ft]), (texel_face, texel_bary) = TexturedMeshModel.texel_map().  occupancy: an OccupancyGrid, typically
    OccupancyGrid.from_mesh(dilate=1) of the same mesh.  shell=None: 1.5 x the grid's largest cell edge, what such a grid holds on either
    side of the surface; step=None: shell / 8, sixteen samples per ray.  texels=None: the chart texels (kal.chart_texels: one more sync);
    a given list must hold distinct texels (checked: a sync).
    The rays start `shell` outside the surface, so where another wall of the mesh lies within `shell` of a texel (thin fins, tight
    concavities) that wall composites first unless visibility= is given.  visibility: a MeshTracer of the same mesh.  Per chunk every
    ray is tested against the mesh between its start and its own surface point, tracer.occluded(ro, rd, 0, shell, own_face = the
    texel's face, repeated per sub-sample): the texel's face and the faces that share a vertex id with it do not count (a face adjacent
    across a concave crease must not blind the texels next to the crease); a blocked sub-sample is dropped (valid &= ~blocked) before
    the resolve.  A texel whose every sub-sample is blocked gets nothing: complete_atlas fills it from its neighbours.  What stays: a
    wall BEHIND the surface within `shell` still lies in the march's second half; that is the field's to keep empty.
    visibility=None (the default) runs nothing new.
    colour: what a view-dependent field (hashgrid.ViewDependentField) bakes.  'view': what it shows along each texel's ray, whose
    direction is minus the face normal; 'diffuse': its base term alone (render_rays_marched(view_dirs=False)).  For any other field the
    two are the same bake."""
    from . import kal
    if colour not in ('view', 'diffuse'):
        raise L.CtxError(f"bake_atlas: colour={colour!r}: want 'view' or 'diffuse'")
    if occupancy is None:
        raise L.CtxError("bake_atlas: needs an occupancy grid (occupancy=): the samples lie in its occupied cells")
    if not isinstance(texel_face, torch.Tensor) or texel_face.dim() != 2 or texel_face.shape[0] != texel_face.shape[1]:
        raise L.CtxError(f"bake_atlas: want texel_face [T,T], got {tuple(getattr(texel_face, 'shape', ()))}")
    T = texel_face.shape[0]
    s = int(supersample)
    if s != supersample or not 1 <= s <= 4:
        raise L.CtxError(f"bake_atlas: supersample={supersample}: want a whole number in [1, 4]")
    shell = 1.5 * float(np.max(occupancy.h)) if shell is None else float(shell)
    if not (shell > 0 and np.isfinite(shell)):
        raise L.CtxError(f"bake_atlas: shell={shell}: want a finite world length > 0")
    step = shell / 8.0 if step is None else float(step)
    if acc is None:
        acc = torch.zeros(4, T, T, dtype=torch.int64, device=texel_face.device)
    elif tuple(acc.shape) != (4, T, T) or acc.dtype != torch.int64:
        raise L.CtxError(f"bake_atlas: acc is {acc.dtype} {tuple(acc.shape)}, expected int64 {(4, T, T)}")
    texels = kal.chart_texels(texel_face) if texels is None else _checked_bake_texels(texels, T)
    base_only = dict(view_dirs=False) if colour == 'diffuse' and getattr(field, 'view_dependent', False) else {}
    per = max(1, int(rays_per_chunk) // (s * s))
    for j0 in range(0, texels.numel(), per):
        part = texels[j0:j0 + per].contiguous()
        ro, rd, valid = kal.texel_rays(texel_face, texel_bary, face_uv, vertices, faces, part, s, shell)
        if visibility is not None:
            own = texel_face.reshape(-1)[part.long()].repeat_interleave(s * s)
            valid = valid & (visibility.occluded(ro, rd, 0., shell, own_face=own) == 0).to(valid.dtype)
        rgb, _, alpha, _, _ = rnh.render_rays_marched(field, ro, rd, 0., 2.0 * shell, occupancy, step, **base_only)
        kal.bake_resolve(rgb, alpha, valid, part, s, acc, min_alpha=min_alpha)
    return acc
