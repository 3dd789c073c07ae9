"""ConTEXTure (paint path only): mirror of the hot-path members of src/training/trainer.py —
`define_view_weights` :370-415 (-> create_face_view_map / compare_face_normals_between_views :155-249),
`paint_viewpoint` :971-1117, plus the per-view loop north_star describes (views sharded one per GPU,
UV back-projection as a scatter into the atlas, RCCL all-reduce of the atlas).

Also here: `project_back` under the reference's call contract (trainer.py:1076-1090; it has no body there, so the
direct UV-scatter form `project_back_scatter` stands in, parity unpinned), the eval renders (`eval_render`,
`evaluate`, `full_eval`, :913-968, 1119-1157) and the mesh export.  Not built: wandb/loguru logging; the mp4 of `full_eval` is a Motion-JPEG AVI (video.py: no H.264 encoder offline).
"""
import math
import os
import torch
import torch.nn.functional as F
from . import _lib as L
from . import dist as D
from . import utils, view_weights
from .batch import MeshBatchPainter
from .run_nerf_helpers import get_embedder, NeRF2D
from .textured_mesh import TexturedMeshModel
from .views_dataset import Zero123PlusDataset, MultiviewDataset


# TEXTure's mask constants are window sizes for 1200^2 renders; their radii scale with render.train_grid_size G in integers:
# r(G) = (2 r0 G + 1200) // 2400 (r0 G / 1200 rounded half up), k = 2 r + 1, which is k0 itself at G = 1200
TRIMAP_K0 = dict(generate=19, rim=7, open=5, project=25, blur=21)


def scaled_radius(r0, G):
    return (2 * int(r0) * int(G) + 1200) // 2400


def scaled_k(k0, G):
    return 2 * scaled_radius(int(k0) // 2, G) + 1


class ConTEXTure:
    def __init__(self, cfg, device=None, diffusion=None, mesh_arrays=None, group=None):
        self.cfg = cfg
        self.paint_step = 0
        self.group = group
        self.rank, self.world, dev = D.init()
        self.device = device if device is not None else dev
        utils.seed_everything(self.cfg.optim.seed)
        self.uv_embedder, input_ch = get_embedder(10)
        if self.cfg.guide.texture_field == 'hashgrid':
            from .hashgrid import HashGridTexture
            g = self.cfg.guide
            self.texture_mlp = HashGridTexture(g.hashgrid_levels, g.hashgrid_features, g.hashgrid_log2_table, g.hashgrid_base_res,
                                               int(g.texture_resolution), D=2, W=64, output_ch=3).to(self.device)
        elif self.cfg.guide.texture_field == 'mlp':
            self.texture_mlp = NeRF2D(D=8, W=256, input_ch=input_ch, output_ch=3, skips=[4]).to(self.device)
        else:
            raise ValueError(f"guide.texture_field={self.cfg.guide.texture_field!r}: expected 'mlp' or 'hashgrid'")
        # trainer.py:253-255: the UV unwrap of a mesh without texture coordinates is cached under cache/<mesh stem>/
        cache_path = None if mesh_arrays is not None else os.path.join('cache', os.path.splitext(os.path.basename(str(self.cfg.guide.shape_path)))[0])
        self.mesh_model = TexturedMeshModel(self.cfg.guide, render_grid_size=self.cfg.render.train_grid_size, cache_path=cache_path,
                                            texture_resolution=self.cfg.guide.texture_resolution, device=self.device,
                                            texture_mlp=self.texture_mlp, uv_embedder=self.uv_embedder, mesh_arrays=mesh_arrays)
        self.diffusion = diffusion
        self.text_z = None
        ds = Zero123PlusDataset if self.cfg.guide.use_zero123plus else MultiviewDataset
        self.train_views = list(ds(self.cfg.render, self.device))
        self.view_weights = None
        self.atlas_filled = self.atlas_fill_src = None                                  # set by complete_atlas (guide.atlas_fill = 'nearest')
        self.view_gains = self.view_gain_stats = None                                   # set by the paint loop under guide.exposure_compensation
        self.back_im = torch.full((3, 64, 64), 0.5, device=self.device)
        self.view_dirs = ['front', 'left', 'back', 'right', 'overhead', 'bottom']       # trainer.py:138
        self.text_string = None

    def _offset_phi(self, phi):
        """phi - front_offset, wrapped into [0, 2 pi) (trainer.py:378-380, 974-976): ONE helper for define_view_weights and
        paint_viewpoint, so that view-weight masks and painted views always share their cameras."""
        phi = float(phi) - math.radians(self.cfg.render.front_offset)
        return float(phi + 2 * math.pi if phi < 0 else phi)

    # ---- trainer.py:316-344 ----------------------------------------------------------------------------------
    def calc_text_embeddings(self):
        """-> (text_z, text_string) with the reference's three shapes: under use_zero123plus a pair [prompt, prompt + ", front view"]
        (and the assert that aborts the shipped YAMLs with append_direction: True, SURVEY section 5.6 defect i); without
        append_direction one embedding; with it one per view direction (`text.format(dir)`)."""
        ref_text = self.cfg.guide.text
        if self.cfg.guide.use_zero123plus:
            assert not self.cfg.guide.append_direction, "append_direction should be False when use_zero123plus is True"
            text_string = [ref_text, ref_text + ", front view"]
            return [self.diffusion.get_text_embeds([t], negative_prompt=None) for t in text_string], text_string
        if not self.cfg.guide.append_direction:
            return self.diffusion.get_text_embeds([ref_text]), ref_text
        text_string = [ref_text.format(d) for d in self.view_dirs]
        return [self.diffusion.get_text_embeds([t], negative_prompt=None) for t in text_string], text_string

    def _text_for(self, data):
        """The embedding paint_viewpoint conditions this view on (trainer.py:1018-1031).  A tensor assigned to `self.text_z` by
        the caller (benches, tests) is used as is."""
        if self.text_z is None:
            self.text_z, self.text_string = self.calc_text_embeddings()
        if isinstance(self.text_z, torch.Tensor):
            return self.text_z
        if self.cfg.guide.use_zero123plus:
            return self.text_z[1]
        d = data['dir']
        return self.text_z[int(d.reshape(-1)[0]) if isinstance(d, torch.Tensor) else int(d)]

    # ---- trainer.py:370-415 ----------------------------------------------------------------------------------
    def define_view_weights(self, view_ids=None):
        """Weight masks for the (local shard of) views; with >1 ranks the per-face maxima are all-reduced (MAX)."""
        ids = list(range(len(self.train_views))) if view_ids is None else list(view_ids)
        group = self.group if self.world > 1 else None
        if self.world > 1 and group is None:
            import torch.distributed as dist
            group = dist.group.WORLD
        self._vw_ids = ids
        if not ids:                                     # a rank without views of this mesh still joins the all-reduce(MAX)
            F_ = self.mesh_model.mesh.faces.shape[0]
            D.all_reduce_max_(torch.full((F_,), float('-inf'), device=self.device), group)
            self.view_weights = None
            return None
        thetas = torch.tensor([self.train_views[i]['theta'] for i in ids], device=self.device)
        # same front_offset shift and wrap as paint_viewpoint (trainer.py:378-380): the masks must come from the painted cameras
        phis = torch.tensor([self._offset_phi(self.train_views[i]['phi']) for i in ids], device=self.device)
        radii = torch.tensor([float(self.train_views[i]['radius']) for i in ids], device=self.device)
        B = len(ids)
        mm = self.mesh_model
        mask, depth, normals_image, face_normals, face_idx = mm.render_face_normals_face_idx(
            mm.mesh.vertices[None].repeat(B, 1, 1), mm.mesh.faces, mm.face_attributes, elev=thetas, azim=phis, radius=radii,
            look_at_height=mm.dy)
        self.view_weights = view_weights.view_weight_masks(face_idx, face_normals, group=group)
        self._vw_cache = dict(mask=mask, depth=depth, face_idx=face_idx, face_normals=face_normals)
        return self.view_weights

    # ---- trainer.py:971-1117 ---------------------------------------------------------------------------------
    @torch.no_grad()   # the paint pass is inference; the texture field keeps activations only when gradients are on
    def _paint_prepare(self, data, image_size=None, num_inference_steps=None):
        """Everything of paint_viewpoint up to the diffusion call: render, crop box; returns (img2img kwargs, context)."""
        theta, phi, radius = data['theta'], data['phi'], data['radius']
        phi = self._offset_phi(phi)
        G = self.cfg.render.train_grid_size
        background = F.interpolate(self.back_im.unsqueeze(0), (G, G), mode='bilinear', align_corners=False) \
            if not self.cfg.guide.use_background_color else torch.tensor([0.0, 0.8, 0.0], device=self.device)
        outputs = self.mesh_model.render(theta=theta, phi=phi, radius=radius, background=background)
        render_cache = outputs['render_cache']
        depth_render = outputs['depth']
        outputs = self.mesh_model.render(background=background, render_cache=render_cache, use_median=self.paint_step > 1)
        rgb_render = outputs['image']
        z_normals = outputs['normals'][:, -1:, :, :].clamp(0, 1)
        object_mask = outputs['mask']
        min_h, min_w, max_h, max_w = utils.get_nonzero_region_tuple(object_mask[0, 0])
        crop = lambda x: x[:, :, min_h:max_h, min_w:max_w]
        cropped_rgb_render, cropped_depth_render, cropped_update_mask = crop(rgb_render), crop(depth_render), crop(object_mask)
        text_z = self._text_for(data)
        kw = dict(text_embeddings=text_z, inputs=cropped_rgb_render.detach(), original_depth_mask=cropped_depth_render.detach(),
                  guidance_scale=self.cfg.guide.guidance_scale, strength=1.0, update_mask=cropped_update_mask,
                  fixed_seed=self.cfg.optim.seed, intermediate_vis=self.cfg.log.vis_diffusion_steps,
                  num_inference_steps=num_inference_steps or self.cfg.guide.num_inference_steps,
                  image_size=image_size or self.cfg.guide.sd_image_size)
        ctx = dict(render_cache=render_cache, z_normals=z_normals, rgb_render=rgb_render, object_mask=object_mask, background=background,
                   box=(min_h, min_w, max_h, max_w), crop_hw=(cropped_rgb_render.shape[2], cropped_rgb_render.shape[3]))
        return kw, ctx

    @torch.no_grad()
    def _paint_finish(self, ctx, cropped_rgb_output):
        cropped_rgb_output = F.interpolate(cropped_rgb_output, ctx['crop_hw'], mode='bilinear', align_corners=False)
        min_h, min_w, max_h, max_w = ctx['box']
        rgb_output = ctx['rgb_render'].clone()
        rgb_output[:, :, min_h:max_h, min_w:max_w] = cropped_rgb_output
        return rgb_output, ctx['object_mask']

    def paint_viewpoint(self, data, should_project_back=True, image_size=None, num_inference_steps=None):
        """trainer.py:971-1117.  With should_project_back (the reference's default) the painted view goes into the running atlas
        through `project_back` with the reference's argument list (:1076-1090; z_normals are withheld under use_zero123plus as
        there); the fitted render is kept in `self.fitted_pred_rgb`."""
        kw, ctx = self._paint_prepare(data, image_size, num_inference_steps)
        te = kw.pop('text_embeddings'); inp = kw.pop('inputs'); dm = kw.pop('original_depth_mask')
        cropped_rgb_output, _ = self.diffusion.img2img_step(te, inp, dm, **kw)
        rgb_output, object_mask = self._paint_finish(ctx, cropped_rgb_output)
        if should_project_back:
            z = None if self.cfg.guide.use_zero123plus else ctx['z_normals']
            self.fitted_pred_rgb = self.project_back(render_cache=ctx['render_cache'], background=ctx['background'], rgb_output=rgb_output,
                                                     object_mask=object_mask, update_mask=object_mask, z_normals=z, z_normals_cache=None)
        return rgb_output, object_mask

    # ---- north_star "UV back-projection" (absent in the reference) ----------------------------
    def project_back_scatter(self, render_cache, rgb_output, weight_mask, acc=None):
        """Scatter a painted view into the atlas: acc[0:3] += w*rgb, acc[3] += w at the 4 bilinear texels of each visible
        pixel (w = view weight mask).  acc [4,T,T] is INT64 in units of 2^-32 (kal.SCATTER_FRAC_BITS; uvscatter.hip's fixed mode):
        integer sums do not depend on the order of views, chunks or ranks, so the all-reduced atlas of N ranks equals the 1-rank
        atlas bit for bit (dist.merge_atlas converts once, after the collective)."""
        from . import kal
        uv = render_cache['uv_features']
        face_idx = render_cache['face_idx']
        T = self.cfg.guide.texture_resolution
        w = weight_mask.to(torch.float32).permute(0, 2, 3, 1)
        go = torch.cat([rgb_output.permute(0, 2, 3, 1) * w, w], dim=-1).contiguous()
        if acc is None:
            acc = torch.zeros(4, T, T, dtype=torch.int64, device=uv.device)
        uvc = uv if (uv.dtype == torch.float32 and uv.is_contiguous()) else L.f32c(uv)
        kal.scatter_fixed(go, uvc, face_idx.contiguous(), acc)
        return acc

    def project_back_gather(self, render_cache, rgb_output, weight_mask, acc=None):
        """The same back-projection from the texel side (guide.projection = 'gather', uvgather.hip): every chart texel of
        mesh_model.texel_map() projects its surface point into the view and, where its face (or a face sharing a vertex with it)
        owns that pixel, adds w*rgb to acc[0:3] and w to acc[3]; rgb is the bilinear colour of the painted view over the taps
        such a face owns, w the weight mask at the nearest pixel.  No pinholes where the surface is magnified and nothing
        outside the charts.  acc as in project_back_scatter (int64, 2^-32): merge_atlas, complete_atlas and export apply as
        they are."""
        from . import kal
        face_idx = render_cache['face_idx']
        T = self.cfg.guide.texture_resolution
        texel_face, texel_bary = self.mesh_model.texel_map()
        values = rgb_output.permute(0, 2, 3, 1).to(torch.float32).contiguous()
        w = weight_mask.to(torch.float32).reshape(face_idx.shape).contiguous()
        if acc is None:
            acc = torch.zeros(4, T, T, dtype=torch.int64, device=face_idx.device)
        fvi = render_cache['face_vertices_image']
        fvi = fvi if (fvi.dtype == torch.float32 and fvi.is_contiguous()) else L.f32c(fvi)
        kal.gather_fixed(values, w, face_idx.contiguous(), fvi, self.mesh_model.mesh.faces.to(torch.int64).contiguous(), texel_face, texel_bary, acc)
        return acc

    @torch.no_grad()
    def exposure_atlas(self, render_cache, rgb_output, object_mask, z_normals, Tc, acc=None):
        """A painted view's low-resolution back-projection for the exposure statistics (guide.exposure_compensation): acc [4,Tc,Tc]
        int64 += the UV scatter of (w * rgb_output, w) in units of 2^-32, w = (object_mask > 0) * (z_normals >= guide.exposure_z_min).
        The weight is binary and is NOT the view-weight mask: those masks are a partition of the surface, so views weighted by them
        share no texel, while gains are estimated from where views overlap.  Always kal.scatter_fixed at Tc, whatever guide.projection
        says: the statistics do not depend on the projection mode.  -> acc (what kal.view_pair_stats reads, one slice per view)."""
        from . import kal
        uv, face_idx = render_cache['uv_features'], render_cache['face_idx']
        w = ((object_mask > 0) & (z_normals >= self.cfg.guide.exposure_z_min)).to(torch.float32).permute(0, 2, 3, 1)
        go = torch.cat([rgb_output.permute(0, 2, 3, 1) * w, w], dim=-1).contiguous()
        if acc is None:
            acc = torch.zeros(4, int(Tc), int(Tc), dtype=torch.int64, device=uv.device)
        uvc = uv if (uv.dtype == torch.float32 and uv.is_contiguous()) else L.f32c(uv)
        kal.scatter_fixed(go, uvc, face_idx.contiguous(), acc)
        return acc

    def projector(self):
        """project_back_scatter or project_back_gather, as guide.projection says."""
        from .config import validate
        return self.project_back_gather if validate(self.cfg).guide.projection == 'gather' else self.project_back_scatter

    @torch.no_grad()
    def project_back(self, render_cache, background, rgb_output, object_mask, update_mask, z_normals=None, z_normals_cache=None):
        """The call the reference makes at trainer.py:1076-1090 (its body is missing there; upstream TEXTure fits the
        texture image to `rgb_output` under `update_mask` by Adam): here the painted pixels are scattered straight into the
        running atlas contribution `self.atlas_acc` [3+1,T,T] (int64 fixed point; `self.atlas_contrib` = its float image) with weight = update_mask * object_mask (* z_normals when given:
        the view-facing weight TEXTure's masks are built from; * the view-weight mask of this view when `define_view_weights` ran
        for it), then the view is re-rendered from the normalised atlas.  `z_normals_cache` is accepted for the call contract and
        not read (there is no meta-texture in this build).  -> fitted_pred_rgb [B,3,H,W].  PARITY UNPINNED (no reference body)."""
        from . import kal
        T = self.cfg.guide.texture_resolution
        w = (update_mask > 0).float() * (object_mask > 0).float()
        if z_normals is not None:
            w = w * z_normals.clamp(0, 1)
        if getattr(self, 'atlas_acc', None) is None:
            self.atlas_acc = torch.zeros(4, T, T, dtype=torch.int64, device=self.device)
        self.projector()(render_cache, rgb_output, w, acc=self.atlas_acc)
        self.atlas_contrib = kal.fixed_to_float(self.atlas_acc)
        wsum = self.atlas_contrib[3:]
        atlas = (self.atlas_contrib[:3] / wsum.clamp_min(1e-8))[None]
        uv, face_idx = render_cache['uv_features'], render_cache['face_idx']
        feat = kal.render.mesh.texture_mapping(uv, atlas.expand(uv.shape[0], -1, -1, -1).contiguous(), mode='bilinear', mask_idx=face_idx)
        cov = kal.render.mesh.texture_mapping(uv, (wsum > 0).float()[None].expand(uv.shape[0], -1, -1, -1).contiguous(), mode='nearest',
                                              mask_idx=face_idx)
        feat, cov = feat.permute(0, 3, 1, 2), cov.permute(0, 3, 1, 2)
        mask = (object_mask > 0).float() * (cov > 0).float()
        bg = background.reshape(1, 3, 1, 1) if background.dim() == 1 else background
        return (bg * (1 - mask) + feat * mask).clamp(0, 1)

    # ---- trainer.py:913-968, 1119-1157 ------------------------------------------------------------------------
    @torch.no_grad()
    def eval_render(self, data):
        """-> (rgb_render [1,H,W,3], texture_rgb [1,T,T,3], depth_render [1,H,W,1], pred_z_normals [1,1,H,W]).  As the reference:
        white background at cfg.render.eval_grid_size, pixels still at the default colour shaded grey by their z-normal.  The
        reference reads `pred_z_normals` from a meta-texture render; without a meta texture it is this view's own z-normal."""
        phi = self._offset_phi(data['phi'])
        dim = self.cfg.render.eval_grid_size
        mm = self.mesh_model
        outputs = mm.render(theta=data['theta'], phi=phi, radius=data['radius'], dims=(dim, dim), background='white')
        z_normals = outputs['normals'][:, -1:, :, :].clamp(0, 1)
        rgb_render = outputs['image']
        default = torch.tensor(getattr(mm, 'default_color', [0.8, 0.1, 0.8]), device=self.device).view(1, 3, 1, 1)
        uncolored = ((rgb_render - default).abs().sum(dim=1) < 0.1).float().unsqueeze(0)
        shade = torch.tensor([0.85, 0.85, 0.85], device=self.device).view(1, 3, 1, 1) * (0.3 + 0.7 * z_normals)      # utils.color_with_shade
        rgb_render = rgb_render * (1 - uncolored) + shade * uncolored
        atlas = getattr(self, 'atlas', None)
        tex = outputs['texture_map'] if atlas is None else self._painted_texture(outputs['texture_map'])
        return (rgb_render.permute(0, 2, 3, 1).contiguous().clamp(0, 1), tex.permute(0, 2, 3, 1).contiguous().clamp(0, 1),
                outputs['depth'].permute(0, 2, 3, 1).contiguous(), z_normals)

    def _painted_texture(self, base):
        if getattr(self, 'atlas_filled', None) is not None:
            cov = (self.atlas_fill_src >= 0)[None, None].to(base.dtype)
            return base * (1 - cov) + self.atlas_filled[None, :3] * cov
        cov = (self.atlas_coverage > 0)[None, None].to(base.dtype)
        return base * (1 - cov) + self.atlas[None, :3] * cov

    def complete_atlas(self, pad=None):
        """Atlas completion after the merge (guide.atlas_fill = 'nearest'): every uncovered chart texel copies the colour of its
        nearest covered texel, then the charts are padded outward by `pad` (default guide.atlas_pad) texels.  Sets
        self.atlas_filled [3,T,T] and self.atlas_fill_src [T,T] int32 (flat index of the covered texel each colour came from,
        -1 = untouched); atlas and atlas_coverage are left as they are.  The merged atlas is identical on every rank and the
        fill is integer-exact, so every rank computes the same result without a collective."""
        from . import kal
        if getattr(self, 'atlas', None) is None:
            raise RuntimeError("complete_atlas: no merged atlas yet (paint first)")
        pad = int(self.cfg.guide.atlas_pad if pad is None else pad)
        with torch.no_grad():
            self.atlas_filled, self.atlas_fill_src = kal.atlas_fill(self.atlas[:3].contiguous(), self.atlas_coverage.contiguous(),
                                                                    self.mesh_model.chart_mask(), pad)
        return self.atlas_filled, self.atlas_fill_src

    def train_view_cameras(self, H=None, W=None):
        """-> (K [3,3], c2ws [V,3,4]): the train views as volume_render.view_camera gives them, for get_rays / fit_views / render_image:
        the same _offset_phi, radius and dy mesh_model.render uses for them, so ray (j, i) of view v passes through the centre of pixel
        (j, i) of that view's raster.  H, W default to render.train_grid_size."""
        from . import volume_render as VR
        G = int(self.cfg.render.train_grid_size)
        H, W = int(G if H is None else H), int(G if W is None else W)
        return VR.view_cameras([float(v['theta']) for v in self.train_views], [self._offset_phi(v['phi']) for v in self.train_views],
                               [float(v['radius']) for v in self.train_views], self.mesh_model.dy, H, W,
                               fovyangle=self.mesh_model.renderer.fovyangle)

    def bake_field(self, field, occupancy=None, step=None, shell=None, supersample=2, min_alpha=0.5, G=128, dilate=1, colour='view',
                   visibility=False):
        """Bakes a 3-D field trained on views of this mesh (volume_render.fit_views) into the mesh's UV atlas (volume_render.bake_atlas
        with mesh_model.texel_map()) -> (atlas [3,T,T], coverage [T,T]).  Sets self.atlas_acc, self.atlas and self.atlas_coverage as the
        merge of a paint does (dist.merge_atlas' conversion, without the collective: every rank bakes the same thing), drops an earlier
        fill, and runs complete_atlas() when guide.atlas_fill == 'nearest'; eval renders and export() then show the baked colours.
        occupancy=None: OccupancyGrid.from_mesh(G, dilate) of the mesh over its bounding box padded by 0.1 of its largest extent.
        step, shell, supersample, min_alpha, colour ('view' | 'diffuse': what a view-dependent field bakes): bake_atlas.
        visibility=True builds a volume_render.MeshTracer of the mesh on the occupancy grid's box and resolution and hands it to bake_atlas:
        a sub-sample whose ray meets another wall of the mesh before its own surface point is dropped.  False (the default): the limit
        stated there holds, rays start `shell` outside the surface, and a second wall of the mesh within `shell` of a texel composites
        first."""
        from . import volume_render as VR
        from .config import validate
        mm = self.mesh_model
        verts, faces = mm.mesh.vertices.detach().to(torch.float32).contiguous(), mm.mesh.faces.to(torch.int64).contiguous()
        if occupancy is None:
            lo, hi = verts.min(0).values.cpu().numpy(), verts.max(0).values.cpu().numpy()
            pad = 0.1 * float((hi - lo).max())
            occupancy = VR.OccupancyGrid.from_mesh(verts, faces, G, lo - pad, hi + pad, dilate=dilate)
        texel_face, texel_bary = mm.texel_map()
        face_uv = mm.face_attributes[0].detach().to(torch.float32).contiguous()
        tracer = VR.MeshTracer(verts, faces, occupancy.G, occupancy.lo, occupancy.hi) if visibility else None
        self.atlas_acc = VR.bake_atlas(field, verts, faces, face_uv, texel_face, texel_bary, occupancy, step=step, shell=shell,
                                       supersample=supersample, min_alpha=min_alpha, colour=colour, visibility=tracer)
        self.atlas, self.atlas_coverage = D.atlas_from_sums(self.atlas_acc)
        self.atlas_filled = self.atlas_fill_src = None
        if validate(self.cfg).guide.atlas_fill == 'nearest':
            self.complete_atlas()
        return self.atlas, self.atlas_coverage

    @torch.no_grad()
    def view_consistency(self, images=None, view_ids=None, rows='image'):
        """How well the train views agree where they show the same surface (trainer.py:429-531, kal.view_consistency): the
        evaluation entry, it syncs and does not run unless called.  images [V,3,G,G]: painted or rendered views of `view_ids`
        (default: all train views) at train_grid_size; None renders them from the current texture.  rows: 'image' (the raster's
        row convention) | 'reference' (upstream's).  -> dict(mean, pair_mean [V][V] indexed [source][target] (0 where no pair),
        pair_count [V][V], n_outside) as Python values."""
        from . import kal
        ids = list(range(len(self.train_views))) if view_ids is None else list(view_ids)
        mm = self.mesh_model
        out = mm.render(theta=[self.train_views[i]['theta'] for i in ids], phi=[self._offset_phi(self.train_views[i]['phi']) for i in ids],
                        radius=[float(self.train_views[i]['radius']) for i in ids], background=torch.tensor([0.5, 0.5, 0.5], device=self.device))
        rc = out['render_cache']
        views = out['image'] if images is None else images.to(self.device)
        mean, st = kal.view_consistency(views.detach().float().contiguous(), mm.mesh.faces.contiguous(), rc['face_idx'].contiguous(),
                                        rc['face_vertices_image'].contiguous(), rows=rows, stats=True, n_vertices=int(mm.mesh.vertices.shape[0]))
        cnt = st['pair_count'].cpu()
        pair_mean = (st['pair_sum'].cpu().double() / 4294967296.0 / cnt.clamp_min(1).double()) * (cnt > 0)
        return dict(mean=float(mean), pair_mean=pair_mean.tolist(), pair_count=cnt.tolist(), n_outside=int(st['n_outside']), rows=rows,
                    view_ids=ids)

    @torch.no_grad()
    def evaluate(self, dataloader, save_path, save_as_video=False):
        """trainer.py:913-952: one rgb frame (+ normal map) per eval view and the texture atlas, under the reference's file names.
        `save_as_video`: the reference muxes `eval:constructed_video:all_rendered_rgb_<seed>.mp4` with imageio / ffmpeg (neither is
        importable offline); the same frames at the same 25 fps go into a Motion-JPEG `.avi` of that name (video.write_mjpeg_avi), and the
        numbered JPGs are kept beside it."""
        import os
        import numpy as np
        from PIL import Image
        save_path = str(save_path)
        os.makedirs(save_path, exist_ok=True)
        to8 = lambda t: (t.detach().cpu().numpy() * 255).astype(np.uint8)
        n, textures, all_preds = 0, None, []
        for i, data in enumerate(dataloader):
            preds, textures, depths, normals = self.eval_render(data)
            tag = 'video_frame' if save_as_video else 'rendered_image'
            if save_as_video:
                all_preds.append(to8(preds[0]))
            Image.fromarray(to8(preds[0])).save(os.path.join(save_path, f"eval:{tag}:{i:04d}_rgb.jpg"))
            if not save_as_video:
                nm = to8(normals[0, 0])
                Image.fromarray(np.stack([nm, nm, nm], -1)).save(os.path.join(save_path, f"eval:normal_map:{i:04d}_normals_cache.jpg"))
                if self.paint_step == 0:
                    torch.save(depths[0].cpu(), os.path.join(save_path, f"eval:depth_map:{i:04d}_depth.pt"))
            n += 1
        if textures is not None:
            Image.fromarray(to8(textures[0])).save(os.path.join(save_path, "eval:texture_atlas:texture.png"))
        if save_as_video and all_preds:
            from .video import write_mjpeg_avi
            write_mjpeg_avi(os.path.join(save_path, f"eval:constructed_video:all_rendered_rgb_{self.cfg.optim.seed}.avi"), all_preds, fps=25)
        return n

    def full_eval(self, output_dir=None, size=None):
        """trainer.py:954-968: the `val_large` orbit (cfg.log.full_eval_size views) + mesh export (rank 0 only)."""
        from .views_dataset import ViewsDataset
        if D.dist.is_initialized() and D.dist.get_rank(self.group) != 0:
            return None
        out = self.cfg.log.exp_dir / 'results' if output_dir is None else output_dir
        n = self.evaluate(ViewsDataset(self.cfg.render, self.device, size=size or self.cfg.log.full_eval_size), out, save_as_video=True)
        if self.cfg.log.eval_consistency:
            import json
            with open(os.path.join(str(out), 'view_consistency.json'), 'w') as fh:
                json.dump(self.view_consistency(), fh)
        if self.cfg.log.save_mesh:
            if getattr(self, 'atlas', None) is not None:
                self.export(str(self.cfg.log.exp_dir / 'mesh') if output_dir is None else str(output_dir) + '/mesh')
            else:
                self.mesh_model.export_mesh(str(self.cfg.log.exp_dir / 'mesh') if output_dir is None else str(output_dir) + '/mesh')
        return n

    # ---- trainer.py:296-315 ---------------------------------------------------------------------------------
    def init_zero123plus(self, unet=None, controlnet=None, vae=None, unet_config=None, vae_config=None, model_dir=None):
        """The Zero123++ stack the reference assembles from the hub (remote pipeline `sudo-ai/zero123plus-pipeline` + depth ControlNet
        at conditioning scale 2, scheduler swapped for DDPMScheduler): here the same wrappers over the HIP engines —
        DepthControlUNet(RefOnlyNoisedUNet(UNet in_channels 4)), AutoencoderKL, DDPMScheduler (v-prediction) as the pipeline's
        scheduler.  Offline the weights are seeded random-init (or engines / state loaded by the caller).  model_dir (or
        cfg.guide.zero123plus_model_dir): a LOCAL directory in the pipeline's layout; its `vision_encoder/`, `feature_extractor_clip/`,
        `tokenizer/`, `text_encoder/` and `model_index.json: ramping_coefficients` give the condition path of
        src/zero123plus.py:772-803 (`zero123plus.ConditionEncoder`), and `unet/`, `vae/`, `controlnet/` safetensors files are loaded
        when present.  Without one, a seeded random `prompt_embeds` stands in for encode_prompt("") + global_embeds * ramp."""
        import os
        from .unet import UNet2DConditionModel, ControlNetModel, SD2_DEPTH
        from .vae import AutoencoderKL
        from .scheduler import DDPMScheduler
        from .zero123plus import RefOnlyNoisedUNet, DepthControlUNet, Zero123PlusPipeline
        ucfg = dict(SD2_DEPTH, in_channels=4) if unet_config is None else dict(unet_config)
        seed = self.cfg.optim.seed
        model_dir = model_dir if model_dir is not None else getattr(self.cfg.guide, 'zero123plus_model_dir', None)

        def local(sub):
            f = os.path.join(str(model_dir), sub, 'diffusion_pytorch_model.safetensors') if model_dir else None
            return f if f and os.path.exists(f) else None
        if unet is None:
            unet = UNet2DConditionModel.from_file(local('unet'), ucfg, device=self.device) if local('unet') else \
                UNet2DConditionModel(ucfg, device=self.device, seed=seed + 11)
        if controlnet is None:
            controlnet = ControlNetModel(ucfg, device=self.device, seed=seed + 12, init=not local('controlnet'))
            if local('controlnet'):
                controlnet.load_file(local('controlnet'))
        if vae is None:
            vae = AutoencoderKL.from_file(local('vae'), device=self.device) if local('vae') else AutoencoderKL(vae_config, device=self.device, seed=seed + 13)
        # trainer.py:306-310: the pipeline's scheduler is replaced by a DDPMScheduler BEFORE prepare(), so RefOnlyNoisedUNet's
        # val_sched (used in eval mode to noise the condition latent) is that same DDPM object
        psched = DDPMScheduler(prediction_type="v_prediction")
        stack = DepthControlUNet(RefOnlyNoisedUNet(unet, DDPMScheduler(prediction_type="v_prediction"), psched).eval(), controlnet,
                                 conditioning_scale=2.0).eval()
        from .zero123plus import ConditionEncoder
        cenc = None
        if model_dir and os.path.isdir(os.path.join(str(model_dir), 'vision_encoder')):
            cenc = ConditionEncoder(model_dir, device=self.device)
        self.zero123plus = Zero123PlusPipeline(vae, stack, psched, condition_encoder=cenc)
        self.zero123plus.inpaint_unet_source = self.diffusion          # trainer.py:312, resolved on first use
        if cenc is None:
            g = torch.Generator().manual_seed(seed + 14)
            self.zero123plus_prompt_embeds = torch.randn(1, 77, ucfg['cross_attention_dim'], generator=g).to(self.device)
        else:
            self.zero123plus_prompt_embeds = None                      # computed from the condition image in paint_zero123plus
        return self.zero123plus

    # ---- trainer.py:545-911 ---------------------------------------------------------------------------------
    def paint_zero123plus(self, iterations=None, tile=320, on_iteration=None):
        """The reference's live `paint()`: front view painted once with SD2-depth, then `iterations` (reference: 5000) steps of
        score distillation of the UV-MLP against Zero123++ — render the 6 novel views from the cached raster, crop + resize to
        tile^2, 3x2 grid, VAE encode WITH autograd, DreamTime timestep, one Zero123++ evaluation (reference-only attention +
        depth ControlNet, CFG 10) -> v target -> `targets = z0 - grad`, 0.5 * sum-MSE on one random latent tile, backward through
        the VAE encoder / resize / texture_mapping / texture field, Adam(lr 1e-5, betas (0.9, 0.99), eps 1e-15; with
        guide.texture_field = 'hashgrid' two parameter groups, the table at optim.hashgrid_lr and its MLP at optim.hashgrid_mlp_lr).
        Host syncs of the reference's loop body that are hoisted out of it: the six crop boxes (the masks do not change) and the
        DreamTime table (rebuilt every iteration there).  -> list of per-iteration dicts (loss, t, fisher, grad_norm).
        optim.consistency_weight > 0 adds the term upstream wrote and switched off (:856-863): the loss that is back-propagated is
        `loss - weight * kal.view_consistency(six views)`; the record's `loss` stays the SDS term and gains `consistency`.
        guide.texture_interpolation_mode = 'mipmap': the six views are rendered at the footprint of the tile pixel the resize keeps
        (mip_scale = box / tile per view); nothing else in the loop changes."""
        from . import sds
        from .scheduler import DDPMScheduler
        if getattr(self, 'zero123plus', None) is None:
            self.init_zero123plus()
        pipe = self.zero123plus
        iterations = int(iterations if iterations is not None else (self.cfg.optim.sds_iterations or 5000))
        self.define_view_weights()
        self.mesh_model.train()
        gray = torch.tensor([0.5, 0.5, 0.5], device=self.device)
        with torch.no_grad():
            rgb_front, mask_front = self.paint_viewpoint(self.train_views[0], should_project_back=False)
            thetas = [v['theta'] for v in self.train_views]
            phis = [self._offset_phi(v['phi']) for v in self.train_views]
            radii = [float(v['radius']) for v in self.train_views]
            allv = self.mesh_model.render(theta=thetas, phi=phis, radius=radii, background=gray)
            object_masks, depth_maps, render_cache = allv['mask'], 1.0 - allv['depth'], allv['render_cache']
            B = object_masks.shape[0]
            min_h, min_w, max_h, max_w = utils.get_nonzero_region_tuple(mask_front[0, 0])
            rgba = torch.cat((rgb_front, mask_front), dim=1)[:, :, min_h:max_h, min_w:max_w]
            # PIL's RGBA resize to 320x320 (bicubic, the library default) stands in as a bicubic interpolate; grey the transparent part
            cond = sds.to_rgb_image(F.interpolate(rgba, (tile, tile), mode='bicubic', align_corners=False).clamp(0, 1))
            cond_image = cond * 2 - 1
            depth_grid = sds.build_depth_grid(depth_maps, object_masks, size=tile)
            boxes = [utils.get_nonzero_region_tuple(object_masks[j, 0]) for j in range(1, B)]
            if getattr(pipe, 'condition_encoder', None) is not None:
                # src/zero123plus.py:772-803, once per mesh (the pipeline recomputes the same tensors on every call in the reference):
                # encode_prompt("") + vision_encoder(feature_extractor_clip(cond)).image_embeds * ramping_coefficients
                pe, neg = pipe.condition_encoder.prompt_embeds(cond)
                self.zero123plus_prompt_embeds, pipe.negative_prompt_embeds = pe.to(self.device), neg.to(self.device)
        self._sds_setup = dict(cond_image=cond_image, depth_grid=depth_grid, boxes=boxes, render_cache=render_cache, field_texels='all')
        if self.cfg.optim.field_texels == 'active':
            # the loop renders from this one raster, so the field is evaluated and trained on the texels it can read; the list rides
            # in the cache (valid for this raster only).  Nothing foreground: nothing to restrict, the loop stays on the whole atlas
            from . import kal
            T = int(self.mesh_model.texture_resolution)
            texels, _ = kal.active_texels(render_cache['uv_features'].contiguous(), render_cache['face_idx'].contiguous(), T)
            n_active = int(texels.numel())
            self._sds_setup.update(n_active=n_active, active_fraction=n_active / float(T * T))
            if n_active > 0:
                render_cache['active_texels'] = texels
                self._sds_setup['field_texels'] = 'active'
        mip_args = {}
        if self.cfg.guide.texture_interpolation_mode == 'mipmap':
            # a tile pixel covers max(box_h, box_w) / tile render pixels: the render is pre-filtered to the footprint of the pixel the resize
            # below keeps (the front view is not resized: 1)
            mip_args = dict(mip_scale=[1.0] + [max(b[2] - b[0], b[3] - b[1]) / float(tile) for b in boxes])
        params = [p for p in self.texture_mlp.parameters()]
        if self.cfg.guide.texture_field == 'hashgrid':
            # the table and its MLP at their own rates (optim.hashgrid_lr, optim.hashgrid_mlp_lr)
            groups = [dict(params=list(self.texture_mlp.encoding.parameters()), lr=float(self.cfg.optim.hashgrid_lr)),
                      dict(params=list(self.texture_mlp.mlp.parameters()), lr=float(self.cfg.optim.hashgrid_mlp_lr))]
            if self.cfg.optim.fused_adam:
                # the HIP step; the table takes it from the backward's integer sums and leaves entries with a zero gradient alone
                from .optim import FieldAdam
                groups[0]['sparse'] = True
                optimizer = FieldAdam(groups, betas=(0.9, 0.99), eps=1e-15, encodings=[self.texture_mlp.encoding])
            else:
                optimizer = torch.optim.Adam(groups, betas=(0.9, 0.99), eps=1e-15)
        elif self.cfg.optim.fused_adam:
            from .optim import FieldAdam
            optimizer = FieldAdam(params, lr=1e-5, betas=(0.9, 0.99), eps=1e-15)
        else:
            optimizer = torch.optim.Adam(params, lr=1e-5, betas=(0.9, 0.99), eps=1e-15)
        train_sched = DDPMScheduler(prediction_type="v_prediction")
        alphas_cumprod = train_sched.alphas_cumprod.to(self.device)
        dream = utils.DreamTimeScheduler(alphas_cumprod, iterations, m=500, s=125)
        ikl, log = None, []
        cw = float(self.cfg.optim.consistency_weight)
        if cw > 0:
            from . import kal
            faces, n_vertices, vc_seen = self.mesh_model.mesh.faces.contiguous(), int(self.mesh_model.mesh.vertices.shape[0]), None
            vc_idx, vc_fvi = render_cache['face_idx'][1:].contiguous(), render_cache['face_vertices_image'][1:].contiguous()
        try:
            for i in range(iterations):
                t = dream.get_t(i)
                optimizer.zero_grad()
                out = self.mesh_model.render(render_cache=render_cache, background=gray, **mip_args)
                six = out['image'][1:]
                tiles = [F.interpolate(six[j:j + 1, :, b[0]:b[2], b[1]:b[3]], (tile, tile), mode='bilinear', align_corners=False)
                         for j, b in enumerate(boxes)]
                r = sds.sds_iteration(pipe, torch.cat(tiles, 0), cond_image, depth_grid, self.zero123plus_prompt_embeds, t,
                                      train_sched.alphas_cumprod, train_sched.add_noise, guidance_scale=10.0, grad_scale=0.2,
                                      ikl_running_avg=ikl)
                ikl = r['ikl_running_avg']
                if cw > 0:
                    # trainer.py:856-863 (`loss = sds_loss - 500 * consistency_reward`, switched off upstream): the seen-vertex map
                    # depends on the cached raster only, so it is built by the first iteration and handed back to the others
                    reward, vc = kal.view_consistency(six.contiguous(), faces, vc_idx, vc_fvi, seen=vc_seen, stats=True, n_vertices=n_vertices)
                    vc_seen = vc['seen']
                    (r['loss'] - cw * reward).backward()
                else:
                    r['loss'].backward()
                gn = torch.linalg.norm(torch.cat([p.grad.reshape(-1) for p in params if p.grad is not None]))
                optimizer.step()
                rec = dict(i=i, t=int(t), loss=float(r['loss'].detach()), fisher=r['fisher'], ikl_running_avg=ikl, grad_norm=float(gn), index=r['index'])
                if cw > 0:
                    rec['consistency'] = float(reward.detach())
                log.append(rec)
                if on_iteration is not None:
                    on_iteration(rec)
        finally:
            if self.cfg.optim.fused_adam:
                optimizer.release()
        self.mesh_model.eval()
        return log

    # ---- progressive painting (guide.paint_mode = 'progressive'): TEXTure, Richardson et al. 2023, sections 3.2-3.3 ----------------
    # The reference is forked from TEXTure and carries the remains of this loop (GuideConfig.z_update_thr / strict_projection,
    # train_config.py:79,81; the use_meta_texture render flag; project_back(update_mask=, z_normals_cache=) at trainer.py:1076-1090 with
    # undefined names; the commented-out latent blend, stable_diffusion_depth.py:382).  TEXTure's source is not available to this
    # project: the rules below are its own definition, written from the paper.  PARITY UNPINNED, as project_back is.
    def _k(self, name):
        return scaled_k(TRIMAP_K0[name], int(self.cfg.render.train_grid_size))

    @torch.no_grad()
    def calculate_trimap(self, object_mask, z_normals, painted, z_cache):
        """-> (update, generate, refine), each float {0,1} [1,1,G,G].  painted / z_cache: the nearest-mode renders of `atlas_acc[3] > 0`
        and of the meta-texture.  generate: the object where nothing is painted yet, grown by k(19); refine: painted pixels this view
        sees more than guide.z_update_thr more frontally than the view that painted them, opened by k(5) (specks go, blocks stay);
        update = generate | refine, without the object's rim of k(7) where it is not generate.  The rest of the object is kept."""
        from . import kal
        obj, ptd = object_mask > 0, painted > 0
        generate = kal.dilate((obj & ~ptd).float().contiguous(), self._k('generate'))
        better = ((z_normals > z_cache + float(self.cfg.guide.z_update_thr)) & ptd & obj).float().contiguous()
        refine = kal.dilate(kal.erode(better, self._k('open')), self._k('open'))
        update = torch.maximum(generate, refine)
        rim = kal.erode(obj.float().contiguous(), self._k('rim'))
        update[(rim == 0) & (generate == 0)] = 0
        return update, generate, refine

    @torch.no_grad()
    def checker_mask(self, update, refine, generate, S):
        """The mask of the first half of a blended denoise loop, [1,1,S,S]: `update` resized by nearest, with a checkerboard of
        S // 32 pixel cells (two latent pixels at S = 512) where the view only refines: there every other cell keeps the earlier
        paint, so the refinement stays anchored to it."""
        rs = lambda m: F.interpolate(m, (S, S), mode='nearest')
        out = rs(update)
        c = max(1, S // 32)
        i = torch.arange(S, device=out.device) // c
        board = ((i[:, None] + i[None, :]) % 2).to(out.dtype)[None, None]
        only = (rs(refine) > 0) & ~(rs(generate) > 0)
        return torch.where(only, board, out)

    @torch.no_grad()
    def projection_weight(self, object_mask, update, z_normals, painted, z_cache):
        """-> the soft weight [1,1,G,G] a painted view is projected back with: the updated part of the object eroded by k(5), grown by
        k(25) and blurred (k(21) taps, sigma 16 G / 1200), zero outside the eroded object; under guide.strict_projection also zero
        below 0.5 and where an earlier, more frontal view painted (z_cache > z_normals): that view keeps its texels."""
        from . import kal
        G = int(self.cfg.render.train_grid_size)
        oe = kal.erode((object_mask > 0).float().contiguous(), self._k('open'))
        core = ((oe > 0) & (update > 0)).float()
        soft = kal.gaussian_blur(kal.dilate(core, self._k('project')), self._k('blur'), 16.0 * G / 1200.0)
        soft[oe == 0] = 0
        if self.cfg.guide.strict_projection:
            soft[soft < 0.5] = 0
            soft[(painted > 0) & (z_cache > z_normals)] = 0
        return soft

    @torch.no_grad()
    def begin_progressive(self):
        """Empties the running atlas (atlas_acc [4,T,T] int64 sums, atlas_meta [T,T]: the z-normal every texel was painted at), the
        trimap log and paint_step."""
        from .config import validate
        validate(self.cfg)
        if self.world > 1:
            raise RuntimeError(f"guide.paint_mode='progressive' paints the views one after another on one rank; this run has {self.world} ranks")
        T = int(self.cfg.guide.texture_resolution)
        self.atlas_acc = torch.zeros(4, T, T, dtype=torch.int64, device=self.device)
        self.atlas_meta = torch.zeros(T, T, dtype=torch.float32, device=self.device)
        self.trimaps, self.paint_step = [], 0

    @torch.no_grad()
    def render_progress(self, render_cache, object_mask):
        """The running atlas seen through a raster -> (rgb [1,3,G,G] (valid where painted), painted [1,1,G,G] {0,1}, z_cache [1,1,G,G]).
        Colour is the bilinear mean over the PAINTED taps only; painted and z_cache are nearest-mode renders."""
        from . import kal
        uv, face_idx = render_cache['uv_features'], render_cache['face_idx']
        colour, wsum = D.atlas_from_sums(self.atlas_acc)
        cov = (wsum > 0).float()
        tm = lambda tex, mode: kal.render.mesh.texture_mapping(uv, tex[None].contiguous(), mode=mode, mask_idx=face_idx).permute(0, 3, 1, 2)
        pre = tm(torch.cat([colour * cov, cov[None]]), 'bilinear')
        near = tm(torch.stack([cov, self.atlas_meta]), 'nearest')
        painted = (near[:, :1] > 0).float() * (object_mask > 0).float()
        return (pre[:, :3] / pre[:, 3:].clamp_min(1e-8)).clamp(0, 1), painted, near[:, 1:] * painted

    @torch.no_grad()
    def paint_view_progressive(self, data, image_size=None, num_inference_steps=None):
        """One view of the progressive loop: raster; colour, painted and z_cache from the running atlas (unpainted pixels show the
        field's colour, as in the independent loop); trimap; crop; img2img_step on the current render (blended with it from the
        second view on); projection of the colour and of the z-normal with projection_weight into temporaries; ctx_atlas_blend.
        -> dict(rgb_output, object_mask, update, generate, refine, weight, contrib [4,T,T] i64, zsum [T,T] i64)."""
        from . import kal
        kw, ctx = self._paint_prepare(data, image_size, num_inference_steps)
        rc, obj, z = ctx['render_cache'], ctx['object_mask'], ctx['z_normals']
        rgb_atlas, painted, z_cache = self.render_progress(rc, obj)
        ctx['rgb_render'] = ctx['rgb_render'] * (1 - painted) + rgb_atlas * painted
        update, generate, refine = self.calculate_trimap(obj, z, painted, z_cache)
        min_h, min_w, max_h, max_w = ctx['box']
        crop = lambda x: x[:, :, min_h:max_h, min_w:max_w]
        S = int(kw['image_size'])
        te = kw.pop('text_embeddings'); kw.pop('inputs'); dm = kw.pop('original_depth_mask')
        kw.update(update_mask=crop(update).contiguous(), check_mask=self.checker_mask(crop(update), crop(refine), crop(generate), S),
                  blend=self.paint_step > 0)
        cropped_rgb_output, _ = self.diffusion.img2img_step(te, crop(ctx['rgb_render']).detach(), dm, **kw)
        rgb_output, _ = self._paint_finish(ctx, cropped_rgb_output)
        weight = self.projection_weight(obj, update, z, painted, z_cache)
        project = self.projector()
        contrib = project(rc, rgb_output, weight)
        zsum = project(rc, z.expand(-1, 3, -1, -1), weight)[0]
        kal.atlas_blend(contrib, zsum, self.atlas_acc, self.atlas_meta)
        self.trimaps.append(dict(object=obj, update=update, generate=generate, refine=refine))
        self.paint_step += 1
        return dict(rgb_output=rgb_output, object_mask=obj, update=update, generate=generate, refine=refine, weight=weight, contrib=contrib,
                    zsum=zsum)

    @torch.no_grad()
    def finish_progressive(self):
        """atlas, atlas_coverage and guide.atlas_fill from the running atlas, exactly as MeshBatchPainter.paint_all leaves them."""
        from .config import validate
        self.atlas, self.atlas_coverage = D.atlas_from_sums(self.atlas_acc)
        self.atlas_filled = self.atlas_fill_src = None
        if validate(self.cfg).guide.atlas_fill == 'nearest':
            self.complete_atlas()
        return self.atlas, self.atlas_coverage

    def paint_progressive(self, image_size=None, num_inference_steps=None, view_ids=None):
        """guide.paint_mode = 'progressive': the train views in dataset order, one at a time, each painted over what the earlier ones
        left (paint_view_progressive) -> (atlas [3,T,T], coverage [T,T]).  The per-view trimaps stay in self.trimaps (save_trimaps
        writes them).  One rank only; optim.views_per_eval and optim.views_in_flight are not read: a view needs the atlas its
        predecessor wrote.  Both guide.projection modes work: the blend divides by the summed weight."""
        self.begin_progressive()
        for k in (range(len(self.train_views)) if view_ids is None else view_ids):
            self.paint_view_progressive(self.train_views[k], image_size, num_inference_steps)
        return self.finish_progressive()

    def save_trimaps(self, path):
        """One PNG per painted view under `path` (the train images of log.log_images): generate red, refine green, keep blue."""
        import numpy as np
        from PIL import Image
        os.makedirs(str(path), exist_ok=True)
        for i, t in enumerate(getattr(self, 'trimaps', None) or []):
            keep = (t['object'] > 0).float() * (1 - t['update'])
            img = torch.cat([t['generate'], t['refine'] * (1 - t['generate']), keep], dim=1)[0].permute(1, 2, 0)
            Image.fromarray((img.cpu().numpy() * 255).astype(np.uint8)).save(os.path.join(str(path), f"{i:04d}_trimap.png"))
        return len(getattr(self, 'trimaps', None) or [])

    def paint(self, image_size=None, num_inference_steps=None):
        """Per-view paint loop: views sharded over the ranks (view k -> rank k mod world, as D.shard_views), one all-reduce(MAX)
        of the view-weight maxima and one atlas all-reduce(SUM); an idle rank joins both.  It is the one-mesh MeshBatchPainter.
        guide.paint_mode = 'progressive' takes paint_progressive instead."""
        if self.cfg.guide.paint_mode != 'independent':
            from .config import validate
            validate(self.cfg)
            return self.paint_progressive(image_size, num_inference_steps)
        painter = MeshBatchPainter([self], view_ids=list(range(len(self.train_views))), group=self.group)
        return painter.paint_all(image_size, num_inference_steps)[0]

    def export(self, path=None):
        """The outputs the reference writes after painting (src/training/trainer.py:954-968 -> export_mesh): mesh.obj / mesh.mtl /
        albedo.png with the painted atlas (rank 0 only; uncovered texels keep the texture field's colour, unless complete_atlas
        has filled them).  Under guide.exposure_compensation also view_gains.json: the gains of the last paint and their statistics."""
        if D.dist.is_initialized() and D.dist.get_rank(self.group) != 0:
            return None
        path = str(self.cfg.log.exp_dir / 'mesh') if path is None else str(path)
        with torch.no_grad():
            tex = self._painted_texture(self.mesh_model.get_texture_map()[0])
        self.mesh_model.export_mesh(path, texture=tex)
        if self.cfg.guide.exposure_compensation and self.view_gains is not None:
            import json
            count, colour_sum = self.view_gain_stats
            with open(os.path.join(path, 'view_gains.json'), 'w') as fh:
                json.dump(dict(gains=self.view_gains.tolist(), count=count.cpu().tolist(), colour_sum=colour_sum.cpu().tolist()), fh)
        return path
