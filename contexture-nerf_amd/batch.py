"""BASELINE configs[3]: a batch of meshes, 6 views each, painted on a view-sharded node (SURVEY section 8d cfg 4, 8e; the intended
multi-mesh usage is visible in the reference's batch driver generate_survey_textures.py:117-162, which loops
`ConTEXTure(cfg).paint()` over meshes one after another on one GPU).

Work items are (mesh, view) pairs in mesh-major order; item k goes to rank k mod world, so with 6 views and 8 ranks the views of
mesh m+1 start on the ranks mesh m leaves idle and every rank ends up with the same number of denoise loops (48 items / 8 ranks).
Exchange steps, both over RCCL, one of each per mesh:
  phase A  all-reduce(MAX) of the per-face view-weight maxima [F]    (before painting: the masks gate the scatter)
  phase B  each rank paints its items wave by wave (stable_diffusion_depth.plan_waves; items of different meshes may share a group)
  phase C  all-reduce(SUM) of the atlas contribution [3+1, T, T] as int64 fixed-point sums (bit-identical for any world size)
Every rank calls the collectives of every mesh in mesh order, whether or not it holds views of that mesh.
guide.exposure_compensation adds one exchange per mesh between B and C: phase B keeps its painted views and fills its views' slices of
the mesh's statistics tensor [V, 4, Tc, Tc] (int64), which is all-reduced (SUM) before the gains are solved and the views projected."""
import torch
from . import dist as D
from .config import validate
from .stable_diffusion_depth import plan_waves


def schedule(n_meshes, n_views, world):
    """-> plan[rank] = ordered [(mesh, view)]; item k = mesh * n_views + view -> rank k mod world."""
    plan = [[] for _ in range(world)]
    for k in range(n_meshes * n_views):
        plan[k % world].append((k // n_views, k % n_views))
    return plan


class MeshBatchPainter:
    """trainers: one ConTEXTure per mesh (same diffusion engine, same process group); view_ids: the dataset indices painted per
    mesh (Zero123PlusDataset views 1..6 by default)."""

    def __init__(self, trainers, view_ids=None, group=None):
        self.trainers = list(trainers)
        self.view_ids = list(view_ids) if view_ids is not None else list(range(1, 7))
        self.group = group
        t0 = self.trainers[0]
        self.rank, self.world, self.device = t0.rank, t0.world, t0.device
        self.plan = schedule(len(self.trainers), len(self.view_ids), self.world)

    # ---- guide.exposure_compensation: one gain per view and colour channel before the merge ------------------------------
    def _exposure_begin(self):
        """Per mesh: the statistics tensor [V,4,Tc,Tc] int64 (this rank fills its own views' slices) and the list of kept views."""
        g = validate(self.trainers[0].cfg).guide
        Tc, V = int(g.exposure_resolution), len(self.view_ids)
        return [dict(stats=torch.zeros(V, 4, Tc, Tc, dtype=torch.int64, device=self.device), views=[]) for _ in self.trainers]

    def _exposure_keep(self, kept, m, v, k, ctx, rgb_output, obj_mask):
        tr, e = self.trainers[m], kept[m]
        tr.exposure_atlas(ctx['render_cache'], rgb_output, obj_mask, ctx['z_normals'], e['stats'].shape[-1], acc=e['stats'][v])
        e['views'].append((v, k, ctx['render_cache'], rgb_output, obj_mask))

    def _exposure_finish(self, kept, project, contrib):
        """After the last wave, per mesh and in mesh order on every rank (an idle rank joins the collective): all-reduce(SUM) of the
        statistics tensor, the pair statistics, the gains (the one host sync), then the kept views are projected with their gains
        through the view-weight masks, as the plain loop projects them ungained."""
        from . import kal
        for m, tr in enumerate(self.trainers):
            g, e = tr.cfg.guide, kept[m]
            D.all_reduce_sum_(e['stats'], self.group)
            count, colour_sum = kal.view_pair_stats(e['stats'])
            gains = kal.solve_view_gains(count, colour_sum, ridge=g.exposure_ridge, max_gain=g.exposure_max_gain)
            tr.view_gains, tr.view_gain_stats = gains, (count, colour_sum)
            dev_gains = gains.to(device=self.device, dtype=torch.float32)
            for v, k, render_cache, rgb_output, obj_mask in e['views']:
                gained = (rgb_output * dev_gains[v][None, :, None, None]).clamp(0, 1)
                project[m](render_cache, gained, tr.view_weights[k:k + 1] & (obj_mask > 0), acc=contrib[m])

    def paint_all(self, image_size=None, num_inference_steps=None):
        """-> [(atlas [3,T,T], coverage [T,T])] per mesh (identical on every rank)."""
        mine = self.plan[self.rank]
        # phase A: view-weight masks of the local views of every mesh; one all-reduce(MAX) per mesh
        slot = {}
        for m, tr in enumerate(self.trainers):
            ids = [self.view_ids[v] for (mm, v) in mine if mm == m]
            tr.define_view_weights(ids)
            for j, vid in enumerate(ids):
                slot[(m, vid)] = j
        # phase B: the rank's items wave by wave as plan_waves lays them out (a group may span mesh boundaries); only the
        # current wave's renders are held
        T = self.trainers[0].cfg.guide.texture_resolution
        contrib = [torch.zeros(4, T, T, dtype=torch.int64, device=self.device) for _ in self.trainers]   # 2^-32 fixed point
        optim = self.trainers[0].cfg.optim
        vpe, infl = int(optim.views_per_eval), int(optim.views_in_flight)
        project = {m: tr.projector() for m, tr in enumerate(self.trainers)}       # guide.projection: scatter | gather
        compensate = self.trainers[0].cfg.guide.exposure_compensation
        kept = self._exposure_begin() if compensate else None
        for wave in plan_waves(len(mine), vpe, infl):
            items = [mine[k] for grp in wave for k in grp]
            preps = [self.trainers[m]._paint_prepare(self.trainers[m].train_views[self.view_ids[v]], image_size, num_inference_steps)
                     for (m, v) in items]
            outs = self.trainers[0].diffusion.img2img_steps([kw for kw, _ in preps], views_per_eval=vpe, views_in_flight=infl)
            for (m, v), (_, ctx), (rgb, _) in zip(items, preps, outs):
                tr = self.trainers[m]
                rgb_output, obj_mask = tr._paint_finish(ctx, rgb)
                k = slot[(m, self.view_ids[v])]
                if compensate:          # guide.exposure_compensation: the view waits for its gain (_exposure_finish projects it)
                    self._exposure_keep(kept, m, v, k, ctx, rgb_output, obj_mask)
                    continue
                project[m](ctx['render_cache'], rgb_output, tr.view_weights[k:k + 1] & (obj_mask > 0), acc=contrib[m])
        if compensate:
            self._exposure_finish(kept, project, contrib)
        # phase C: one all-reduce(SUM) per mesh
        res = []
        for m, tr in enumerate(self.trainers):
            atlas, cov = D.merge_atlas(contrib[m], self.group)
            tr.atlas, tr.atlas_coverage = atlas, cov
            tr.atlas_filled = tr.atlas_fill_src = None
            if validate(tr.cfg).guide.atlas_fill == 'nearest':      # every rank holds the same merged atlas: no collective
                tr.complete_atlas()
            res.append((atlas, cov))
        return res
