"""Multiresolution hash-grid field (instant-ngp): a table of trainable features, trilinearly interpolated at Lv resolutions, feeding a small
MLP.  HashGridEncoding is the table with `ctx_hashgrid_fwd` / `ctx_hashgrid_bwd` (csrc/hashgrid.hip; the rule: tests/hashgrid_rule.py,
DESIGN section 4j); HashGridField adds NeRF2D(D=2, W=64) on the `emb` seam (NeRF2D.forward_features, which carries the gradient back to the
features).  The field answers forward_pts(pts [...,3]) -> [...,4], which is all the ray path asks of a field: it goes into render_rays,
render_rays_marched, render_image, render_and_refine, train_step, fit_views and OccupancyGrid.update as NeRF2D does.
The table's gradient is summed in 64-bit integers, so a training run repeats bit for bit.  Positions get a gradient
(`ctx_hashgrid_bwd_pts`; the rule: tests/hashgrid_grad_rule.py) where it is asked for: through autograd with
grad_pts=True, and from HashGridField.density_gradient, which volume_render.render_normals turns into rendered normals.  That gradient is
first order only.
ViewDependentField adds a colour residual from a second small MLP on the same features and the spherical harmonics of the ray's direction
(csrc/viewdep.hip; the rule: tests/sh_rule.py); its forward_pts stays the position-only base term.
HashGridEncoding2D / HashGridTexture are the same idea over the unit UV square for the product's texture field (csrc/hashtex.hip; the rule:
tests/hashtex_rule.py): bilinear levels, the 2 x 64 MLP and the (tanh + 1) / 2 head behind NeRF2D.texture_map's contract,
selected by guide.texture_field = 'hashgrid'.
Both encodings can leave the table's gradient as those integer sums for optim.FieldAdam to step from (_DeferredTable);
nothing changes unless a FieldAdam lists the encoding."""
import ctypes as C
import math
import numpy as np
import torch
import torch.nn as nn
from . import _lib as L
from .run_nerf_helpers import NeRF2D

MAX_LEVELS, MAX_WIDTH, MAX_RES = 16, 64, 1 << 20


def level_resolutions(n_levels, base_res, max_res):
    """res[l] = floor(base_res * exp(l * ln(max_res / base_res) / (n_levels - 1))) in float64 (base_res for one level) -> int32 [n_levels].
    The kernels take these integers: no transcendental runs on the device."""
    if n_levels == 1:
        return np.array([int(base_res)], np.int32)
    b = math.log(max_res / base_res) / (n_levels - 1)
    return np.array([int(math.floor(base_res * math.exp(l * b))) for l in range(n_levels)], np.int32)


class _DeferredTable(nn.Module):
    """What the two encodings share: the table with the checks of its parameters, and around its backward the workspace of the integer
    accumulator and the deferred mode that optim.FieldAdam(encodings=...) switches on.  Deferred: the first backward since the last step /
    zero_grad only accumulates (stage 2, behind stage 1 unless the workspace is known to be zero), remembers its rows and returns no
    gradient: FieldAdam.step reads the sums (`ctx_table_adam`, which leaves the workspace zero).  A later backward before the step
    flushes the sums into a float gradient (stage 4), runs as without deferral (stages 7) and returns the sum of the two; from then on to
    the step every backward does.  Outside deferred mode nothing here changes what the backward computes."""
    _corners = 8

    def __init__(self, who, n_levels, n_features, log2_table, base_res, max_res):
        super().__init__()
        for name, v in (("n_levels", n_levels), ("n_features", n_features), ("log2_table", log2_table), ("base_res", base_res),
                        ("max_res", max_res)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise L.CtxError(f"{who}: {name}={v!r}: want an int")
        if not 1 <= n_levels <= MAX_LEVELS:
            raise L.CtxError(f"{who}: n_levels={n_levels} outside [1, {MAX_LEVELS}]")
        if n_features not in (1, 2, 4):
            raise L.CtxError(f"{who}: n_features={n_features}: want 1, 2 or 4 features per entry")
        if n_levels * n_features > MAX_WIDTH:
            raise L.CtxError(f"{who}: n_levels * n_features = {n_levels * n_features} is wider than the field's {MAX_WIDTH}-column embedding")
        if not 4 <= log2_table <= 22:
            raise L.CtxError(f"{who}: log2_table={log2_table} outside [4, 22]")
        if not 1 <= base_res <= max_res <= MAX_RES:
            raise L.CtxError(f"{who}: want 1 <= base_res <= max_res <= 2^20, got base_res={base_res}, max_res={max_res}")
        self.n_levels, self.n_features, self.log2_table = int(n_levels), int(n_features), int(log2_table)
        self.res = level_resolutions(self.n_levels, int(base_res), int(max_res))
        self.out_dim = self.n_levels * self.n_features
        self.table = nn.Parameter((torch.rand(self.n_levels, 1 << self.log2_table, self.n_features) * 2 - 1) * 1e-4)
        self._defer_init()

    def _defer_init(self):
        self._bwd_ws = None
        self._defer, self._pending, self._ws_clean, self._float_mode = False, None, False, False

    def _defer_begin(self):
        self._defer, self._pending, self._ws_clean, self._float_mode = True, None, False, False

    def _defer_end(self):
        self._defer, self._pending, self._ws_clean, self._float_mode = False, None, False, False

    def _defer_drop(self):
        """zero_grad: pending sums are cleared."""
        if self._pending is not None:
            self._bwd_ws.zero_()
            self._pending, self._ws_clean = None, True
        self._float_mode = False

    def _defer_consumed(self):
        """`ctx_table_adam` has read the sums and left the workspace zero."""
        self._pending, self._ws_clean, self._float_mode = None, True, False

    def _defer_stepped(self):
        self._float_mode = False

    def _defer_flush(self):
        """The pending sums as the float gradient stage 4 makes of them."""
        g = torch.empty_like(self.table)
        self._bwd_launch(self._pending, None, 4, g)
        self._pending, self._ws_clean, self._float_mode = None, False, True
        return g

    def _bwd_ws_bytes(self):
        """The accumulator and its control words: one size for both encodings, whichever query is asked."""
        return L.load().ctx_hashgrid_bwd_ws_bytes(self.n_levels, self.n_features, self.log2_table)

    def _workspace(self, device, zeroed):
        wsb = self._bwd_ws_bytes()
        if self._bwd_ws is None or self._bwd_ws.numel() < wsb or self._bwd_ws.device != device:
            self._bwd_ws = None
            # the int64 accumulator: scratch, stream-ordered
            self._bwd_ws = (torch.zeros if zeroed else torch.empty)(wsb, dtype=torch.uint8, device=device)
            self._ws_clean = zeroed
        return self._bwd_ws

    def _table_backward(self, rows, g_emb):
        """rows: what names the rows of this backward, its last entry n -> g_table, or None when the sums stay on the device."""
        device = g_emb.device
        if not self._defer:
            self._workspace(device, False)
            g_table = torch.empty(self.table.shape, device=device)
            self._bwd_launch(rows, g_emb, 7, g_table)
            return g_table
        self._workspace(device, True)
        if self._pending is None and not self._float_mode:
            self._bwd_launch(rows, g_emb, 2 if self._ws_clean else 3, None)
            self._pending, self._ws_clean = rows, False
            return None
        g1 = self._defer_flush() if self._pending is not None else None
        self._float_mode = True
        g_table = torch.empty(self.table.shape, device=device)
        self._bwd_launch(rows, g_emb, 7, g_table)
        return g_table if g1 is None else g_table + g1


class _HashGridFn(torch.autograd.Function):
    """emb [n, Lv*F] = encoding(pts [n,3]; table); the gradient goes to the table and, for an encoding with grad_pts=True and a pts that
    requires grad, to pts.  First order only (once_differentiable): the positions' gradient is itself a function of pts and of the table,
    but nothing differentiates it, so a loss on the normals cannot be trained through.  With no grad enabled this is not used and nothing is
    saved."""

    @staticmethod
    def forward(ctx, enc, pts, table):
        ctx.enc = enc
        ctx.save_for_backward(pts, table)
        return enc._launch_fwd(pts, table)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_emb):
        enc = ctx.enc
        pts, table = ctx.saved_tensors
        g_emb = L.f32c(g_emb)
        g_table = enc._table_backward((pts, pts.shape[0]), g_emb) if ctx.needs_input_grad[2] else None
        g_pts = enc._launch_bwd_pts(pts, table, g_emb) if ctx.needs_input_grad[1] else None
        return None, g_pts, g_table


class HashGridEncoding(_DeferredTable):
    """pts [..., 3] inside the box lo .. hi -> features [..., n_levels * n_features]: at every level the trilinear interpolation of the 8
    table entries at the corners of the point's cell; a level whose (res + 1)^3 nodes fit the table indexes it directly, a finer one by
    instant-ngp's spatial hash.  Points outside the box take the values on its surface; NaN coordinates read as lo.
    lo, hi: a number or three per axis, finite, lo < hi.  1 <= n_levels <= 16, n_features in {1, 2, 4}, n_levels * n_features <= 64,
    4 <= log2_table <= 22, 1 <= base_res <= max_res <= 2^20.  `table` [n_levels, 2^log2_table, n_features] starts uniform in +-1e-4.
    grad_pts=False: a pts that requires grad is refused.  grad_pts=True: it gets its gradient (`ctx_hashgrid_bwd_pts`): the derivative of the
    interpolation in the cell the point lies in, one-sided on cell faces, and 0 on an axis on or outside the box faces.  First order only:
    a loss on that gradient (on normals, an eikonal term) cannot be trained through."""

    def __init__(self, lo, hi, n_levels=16, n_features=2, log2_table=19, base_res=16, max_res=2048, grad_pts=False):
        who = "HashGridEncoding"
        super().__init__(who, n_levels, n_features, log2_table, base_res, max_res)
        lo = np.broadcast_to(np.asarray(lo, np.float32), (3,)).copy()
        hi = np.broadcast_to(np.asarray(hi, np.float32), (3,)).copy()
        if not bool(np.all(np.isfinite(lo))) or not bool(np.all(lo < hi)) or not bool(np.all(np.isfinite(hi - lo))):
            raise L.CtxError(f"{who}: the box needs finite lo < hi on every axis, got lo={lo.tolist()}, hi={hi.tolist()}")
        self.lo, self.hi = lo, hi
        self.grad_pts = bool(grad_pts)
        self._pts_ws = None

    def _grid_args(self):
        """(Lv, F, log2T, res, lo, hi) as the ABI takes them; the three arrays are host memory."""
        return (self.n_levels, self.n_features, self.log2_table, self.res.ctypes.data_as(C.c_void_p),
                self.lo.ctypes.data_as(C.c_void_p), self.hi.ctypes.data_as(C.c_void_p))

    def _launch_fwd(self, pts, table):
        emb = torch.empty(pts.shape[0], self.out_dim, device=table.device)
        L.check(L.load().ctx_hashgrid_fwd(L.ptr(pts, torch.float32, "pts"), pts.shape[0], L.ptr(table, torch.float32, "table"),
                                          *self._grid_args(), L.ptr(emb), L.stream()))
        return emb

    def _bwd_launch(self, rows, g_emb, stages, g_table):
        """`ctx_hashgrid_bwd` on rows = (pts, n); a stage that is not asked for does not touch its buffer, which only has to be live."""
        pts, n = rows
        live = self.table
        L.check(L.load().ctx_hashgrid_bwd(L.ptr(pts), n, L.ptr(live if g_emb is None else g_emb), *self._grid_args(), stages,
                                          L.ptr(self._bwd_ws), L.ptr(live if g_table is None else g_table), L.stream()))

    def _launch_bwd_pts(self, pts, table, g_emb):
        """g_pts [n,3] of pts [n,3] for g_emb [n, out_dim], all float32 contiguous on the table's device."""
        lib = L.load()
        n = pts.shape[0]
        wsb = lib.ctx_hashgrid_bwd_pts_ws_bytes(n, self.n_levels)
        if wsb < 0:
            raise L.CtxError(f"HashGridEncoding: {n} points: the positions' gradient wants 1 <= n < 2^31; split the batch")
        if self._pts_ws is None or self._pts_ws.numel() < wsb or self._pts_ws.device != table.device:
            self._pts_ws = None
            self._pts_ws = torch.empty(wsb, dtype=torch.uint8, device=table.device)      # the per-level partials: scratch, stream-ordered
        g_pts = torch.empty(n, 3, device=table.device)
        L.check(lib.ctx_hashgrid_bwd_pts(L.ptr(pts, torch.float32, "pts"), n, L.ptr(table, torch.float32, "table"),
                                         L.ptr(g_emb, torch.float32, "g_emb"), *self._grid_args(), L.ptr(self._pts_ws), L.ptr(g_pts), L.stream()))
        return g_pts

    def forward(self, pts):
        if not isinstance(pts, torch.Tensor) or pts.dim() < 1 or pts.shape[-1] != 3:
            raise L.CtxError(f"HashGridEncoding: want pts [..., 3], got {tuple(getattr(pts, 'shape', ()))}")
        grad_mode = torch.is_grad_enabled()
        want_pts = grad_mode and pts.requires_grad
        if want_pts and not self.grad_pts:
            raise L.CtxError("HashGridEncoding: the HIP path has no gradient with respect to the positions; detach pts")
        L.ptr(self.table, torch.float32, "table")
        if pts.device != self.table.device:
            raise L.CtxError(f"HashGridEncoding: pts on {pts.device}, the table on {self.table.device} (the HIP path has no CPU fallback: "
                             "want a device tensor)")
        x = L.f32c(pts).reshape(-1, 3)
        if x.shape[0] == 0:
            return torch.zeros(*pts.shape[:-1], self.out_dim, device=x.device)
        if grad_mode and (self.table.requires_grad or want_pts):
            emb = _HashGridFn.apply(self, x, self.table)
        else:
            emb = self._launch_fwd(x, self.table.detach())
        return emb.reshape(*pts.shape[:-1], self.out_dim)


class HashGridField(nn.Module):
    """instant-ngp's field: HashGridEncoding -> NeRF2D(D, W, input_ch = n_levels * n_features, output_ch, skips=[0]) on the `emb` seam.
    About 21 kFLOP and 0.7 KB of saved activations per point at the defaults, against 1 MFLOP and 8.7 KB for the 8 x 256 Fourier field."""

    def __init__(self, lo, hi, n_levels=16, n_features=2, log2_table=19, base_res=16, max_res=2048, D=2, W=64, output_ch=4,
                 grad_pts=False):
        super().__init__()
        self.encoding = HashGridEncoding(lo, hi, n_levels, n_features, log2_table, base_res, max_res, grad_pts=grad_pts)
        if D < 2:
            raise L.CtxError(f"HashGridField: D={D}: the MLP needs at least two hidden layers (the second one is the skip layer)")
        self.mlp = NeRF2D(D=D, W=W, input_ch=self.encoding.out_dim, output_ch=output_ch, skips=[0])
        self.output_ch = output_ch

    @classmethod
    def from_grid(cls, occupancy_grid, **kw):
        """The field over an OccupancyGrid's box."""
        return cls(occupancy_grid.lo, occupancy_grid.hi, **kw)

    def forward_pts(self, pts):
        """pts [..., 3] -> raw [..., output_ch]."""
        return self.mlp.forward_features(self.encoding(pts))

    forward = forward_pts

    @torch.no_grad()
    def density_gradient(self, pts, channel=3, return_raw=False):
        """pts [..., 3] -> grad [..., 3] = d raw[..., channel] / d pts (channel 3: the density before its ReLU), and with return_raw=True
        (raw [..., output_ch], grad): one forward that keeps the MLP's activations, the MLP's input gradient alone (`ctx_uvmlp_bwd_emb`
        without its weight-gradient launches) and `ctx_hashgrid_bwd_pts`.  No autograd is involved: the result carries no graph, no
        parameter gets a .grad, the ambient grad mode and grad_pts play no part, and the activation pool goes back to the MLP as after a
        backward.  The normal of the density field is -grad / |grad| (volume_render.render_normals).  First order only."""
        enc, mlp = self.encoding, self.mlp
        if isinstance(channel, bool) or not isinstance(channel, (int, np.integer)) or not 0 <= channel < self.output_ch:
            raise L.CtxError(f"HashGridField.density_gradient: channel={channel!r}: want an int in [0, {self.output_ch})")
        if not isinstance(pts, torch.Tensor) or pts.dim() < 1 or pts.shape[-1] != 3:
            raise L.CtxError(f"HashGridField.density_gradient: want pts [..., 3], got {tuple(getattr(pts, 'shape', ()))}")
        table = enc.table.detach()
        L.ptr(table, torch.float32, "table")
        if pts.device != table.device:
            raise L.CtxError(f"HashGridField.density_gradient: pts on {pts.device}, the table on {table.device} (the HIP path has no CPU "
                             "fallback: want a device tensor)")
        x = L.f32c(pts.detach()).reshape(-1, 3)
        if x.shape[0] == 0:
            grad, raw = torch.zeros(*pts.shape[:-1], 3, device=x.device), torch.zeros(*pts.shape[:-1], self.output_ch, device=x.device)
            return (raw, grad) if return_raw else grad
        g_raw = torch.zeros(x.shape[0], self.output_ch, device=x.device)
        g_raw[:, channel] = 1.0
        raw, g_emb = mlp.features_input_gradient(enc._launch_fwd(x, table), g_raw)
        grad = enc._launch_bwd_pts(x, table, g_emb).reshape(*pts.shape[:-1], 3)
        return (raw.reshape(*pts.shape[:-1], self.output_ch), grad) if return_raw else grad


# ---- view-dependent colour: a residual net on the features and the ray's spherical harmonics ----------------------
SH_MAX_DEGREE = 4


def _view_input(emb, rays_d, ray_id, deg):
    n, E = emb.shape
    inp = torch.empty(n, E + deg * deg, device=emb.device)
    L.check(L.load().ctx_viewdep_input_fwd(L.ptr(emb, torch.float32, "emb"), L.ptr(rays_d, torch.float32, "rays_d"),
                                           L.ptr(ray_id, torch.int32, "ray_id"), n, rays_d.shape[0], E, deg, L.ptr(inp), L.stream()))
    return inp


class _ViewInputFn(torch.autograd.Function):
    """inp [n, E + deg^2] = [ emb | SH(rays_d[ray_id]) ] (`ctx_viewdep_input_fwd`); the gradient goes to emb alone, the first E columns of
    g_inp (`ctx_viewdep_input_bwd`).  The directions have none.  With no grad enabled this is not used; nothing is saved either way."""

    @staticmethod
    def forward(ctx, emb, rays_d, ray_id, deg):
        ctx.deg = deg
        return _view_input(emb, rays_d, ray_id, deg)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_inp):
        g_inp = L.f32c(g_inp)
        n, E = g_inp.shape[0], g_inp.shape[1] - ctx.deg * ctx.deg
        g_emb = torch.empty(n, E, device=g_inp.device)
        L.check(L.load().ctx_viewdep_input_bwd(L.ptr(g_inp, torch.float32, "g_inp"), n, E, ctx.deg, L.ptr(g_emb), L.stream()))
        return g_emb, None, None, None


def _view_raw(base, res):
    raw = torch.empty_like(base)
    L.check(L.load().ctx_viewdep_raw_fwd(L.ptr(base, torch.float32, "base"), L.ptr(res, torch.float32, "res"), base.shape[0], L.ptr(raw),
                                         L.stream()))
    return raw


class _ViewRawFn(torch.autograd.Function):
    """raw [n,4] = base [n,4] with res [n,3] added to its colour channels (`ctx_viewdep_raw_fwd`).  The gradient to base is g_raw itself, the
    one to res its first three columns (`ctx_viewdep_raw_bwd`).  Nothing is saved."""

    @staticmethod
    def forward(ctx, base, res):
        return _view_raw(base, res)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_raw):
        g_raw = L.f32c(g_raw)
        g_res = None
        if ctx.needs_input_grad[1]:
            g_res = torch.empty(g_raw.shape[0], 3, device=g_raw.device)
            L.check(L.load().ctx_viewdep_raw_bwd(L.ptr(g_raw, torch.float32, "g_raw"), g_raw.shape[0], L.ptr(g_res), L.stream()))
        return (g_raw if ctx.needs_input_grad[0] else None), g_res


class ViewDependentField(HashGridField):
    """HashGridField with a view-dependent colour residual, as NeRF and instant-ngp condition colour on the viewing direction:
    raw[:, :3] = base[:, :3] + res, raw[:, 3] = base[:, 3].  The base term is the parent's field (`encoding` -> `mlp`), a function of position
    alone; res [n,3] = dir_mlp([ emb | SH(direction) ]) with dir_mlp = NeRF2D(dir_D, dir_W, input_ch = E + sh_degree^2, output_ch = 3,
    skips=[0]) on the same features emb and the sh_degree^2 real spherical harmonics of the ray's unit direction (csrc/viewdep.hip; the
    rule: tests/sh_rule.py).  The density never sees the direction.  dir_mlp.output_linear starts at zero, so a new field is its base term.
    forward_pts (inherited) is the base term alone: OccupancyGrid.update, density_gradient and render_normals read it and never run the
    direction net.  forward_dirs adds the residual; render_rays_marched calls it for a field with view_dependent = True.
    1 <= sh_degree <= 4 and E + sh_degree^2 <= 64 with E = n_levels * n_features, the MLP kernel's input width."""
    view_dependent = True

    def __init__(self, lo, hi, n_levels=16, n_features=2, log2_table=19, base_res=16, max_res=2048, D=2, W=64, sh_degree=4, dir_D=2,
                 dir_W=64, grad_pts=False):
        super().__init__(lo, hi, n_levels, n_features, log2_table, base_res, max_res, D=D, W=W, output_ch=4, grad_pts=grad_pts)
        if isinstance(sh_degree, bool) or not isinstance(sh_degree, (int, np.integer)) or not 1 <= sh_degree <= SH_MAX_DEGREE:
            raise L.CtxError(f"ViewDependentField: sh_degree={sh_degree!r}: want an int in [1, {SH_MAX_DEGREE}]")
        E, K = self.encoding.out_dim, int(sh_degree) ** 2
        if E + K > MAX_WIDTH:
            raise L.CtxError(f"ViewDependentField: n_levels * n_features + sh_degree^2 = {E} + {K} = {E + K} is wider than the direction "
                             f"net's {MAX_WIDTH}-column input")
        if dir_D < 2:
            raise L.CtxError(f"ViewDependentField: dir_D={dir_D}: the MLP needs at least two hidden layers (the second one is the skip layer)")
        self.sh_degree = int(sh_degree)
        self.dir_mlp = NeRF2D(D=dir_D, W=dir_W, input_ch=E + K, output_ch=3, skips=[0])
        with torch.no_grad():
            self.dir_mlp.output_linear.weight.zero_()
            self.dir_mlp.output_linear.bias.zero_()

    def forward_dirs(self, pts, rays_d, ray_id, return_residual=False):
        """pts [n,3], rays_d [R,3] float32, ray_id int32 [n] (the ray of every point, as the marched lists carry it; an entry outside [0, R)
        takes the direction (0,0,0)) -> raw [n,4], and with return_residual=True (raw, res [n,3]).  The encoding runs once; the base MLP
        and the input kernel both read its features, and the table's gradient arrives through both nets.  There is no gradient to the
        directions.  n = 0 returns empties without a launch."""
        who = "ViewDependentField.forward_dirs"
        if not isinstance(pts, torch.Tensor) or pts.dim() != 2 or pts.shape[1] != 3:
            raise L.CtxError(f"{who}: want pts [n,3], got {tuple(getattr(pts, 'shape', ()))}")
        if not isinstance(rays_d, torch.Tensor) or rays_d.dim() != 2 or rays_d.shape[1] != 3 or rays_d.shape[0] < 1:
            raise L.CtxError(f"{who}: want rays_d [R,3] with R >= 1, got {tuple(getattr(rays_d, 'shape', ()))}")
        if not isinstance(ray_id, torch.Tensor) or tuple(ray_id.shape) != (pts.shape[0],):
            raise L.CtxError(f"{who}: want ray_id [n] with n = {pts.shape[0]}, one ray per point, got {tuple(getattr(ray_id, 'shape', ()))}")
        if rays_d.requires_grad or ray_id.requires_grad:
            raise L.CtxError(f"{who}: the HIP path has no gradient with respect to rays_d / ray_id; detach them")
        device = self.encoding.table.device
        for name, t, dtype in (("rays_d", rays_d, torch.float32), ("ray_id", ray_id, torch.int32)):
            if t.dtype != dtype:
                raise L.CtxError(f"{who}: {name}: expected dtype {dtype}, got {t.dtype}")
            if t.device != device or device.type == 'cpu':
                raise L.CtxError(f"{who}: {name} on {t.device}, the table on {device} (the HIP path has no CPU fallback: want a device tensor)")
        emb = self.encoding(pts)                                             # checks pts: device, grad_pts
        n = pts.shape[0]
        if n == 0:
            raw, res = torch.zeros(0, 4, device=device), torch.zeros(0, 3, device=device)
            return (raw, res) if return_residual else raw
        rays_d, ray_id = rays_d.contiguous(), ray_id.contiguous()
        grad_mode = torch.is_grad_enabled()
        base = self.mlp.forward_features(emb)
        if grad_mode and emb.requires_grad:
            inp = _ViewInputFn.apply(emb, rays_d, ray_id, self.sh_degree)
        else:
            inp = _view_input(emb, rays_d, ray_id, self.sh_degree)
        res = self.dir_mlp.forward_features(inp)
        if grad_mode and (base.requires_grad or res.requires_grad):
            raw = _ViewRawFn.apply(base, res)
        else:
            raw = _view_raw(base, res)
        return (raw, res) if return_residual else raw


# ---- the texture field: a 2-D hash grid over the unit UV square --------------------------------------------------
class _HashTexFn(torch.autograd.Function):
    """emb [n, Lv*F] = encoding(rows; table) with the rows named by uv [n,2], by the grid (whole atlas) or by a texel list; the gradient
    goes to the table only (`ctx_hashtex_bwd`).  First order only.  With no grad enabled this is not used and nothing is saved."""

    @staticmethod
    def forward(ctx, enc, uv, idx, n, grid, table):
        ctx.enc, ctx.uv, ctx.idx, ctx.n, ctx.grid = enc, uv, idx, n, grid
        return enc._launch_fwd(uv, idx, n, grid, table)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_emb):
        enc = ctx.enc
        g_table = enc._table_backward((ctx.uv, ctx.idx, ctx.grid, ctx.n), L.f32c(g_emb))
        return None, None, None, None, None, g_table


class HashGridEncoding2D(_DeferredTable):
    """uv [..., 2] in the unit square -> features [..., n_levels * n_features]: at every level the bilinear interpolation of the 4 table
    entries at the corners of the point's cell; a level whose (res + 1)^2 nodes fit the table indexes it directly, a finer one by
    instant-ngp's spatial hash.  Points outside the square take the values on its edge; NaN coordinates read as 0.
    1 <= n_levels <= 16, n_features in {1, 2, 4}, n_levels * n_features <= 64, 4 <= log2_table <= 22, 1 <= base_res <= max_res <= 2^20.
    `table` [n_levels, 2^log2_table, n_features] starts uniform in +-1e-4.  There is no gradient to uv: a uv that requires grad is refused."""

    def __init__(self, n_levels=12, n_features=2, log2_table=18, base_res=16, max_res=1024):
        super().__init__("HashGridEncoding2D", n_levels, n_features, log2_table, base_res, max_res)

    def _grid_args(self):
        """(Lv, F, log2T, res) as the ABI takes them; res is host memory."""
        return self.n_levels, self.n_features, self.log2_table, self.res.ctypes.data_as(C.c_void_p)

    def _launch_fwd(self, uv, idx, n, grid, table):
        emb = torch.empty(n, self.out_dim, device=table.device)
        L.check(L.load().ctx_hashtex_fwd(L.ptr(uv), L.ptr(idx), n, grid, L.ptr(table, torch.float32, "table"), *self._grid_args(), L.ptr(emb),
                                         L.stream()))
        return emb

    _corners = 4

    def _bwd_launch(self, rows, g_emb, stages, g_table):
        """`ctx_hashtex_bwd` on rows = (uv, idx, grid, n); a stage that is not asked for does not touch its buffer, which only has to be live."""
        uv, idx, grid, n = rows
        live = self.table
        L.check(L.load().ctx_hashtex_bwd(L.ptr(uv), L.ptr(idx), n, grid, L.ptr(live if g_emb is None else g_emb, torch.float32, "g_emb"),
                                         *self._grid_args(), stages, L.ptr(self._bwd_ws), L.ptr(live if g_table is None else g_table),
                                         L.stream()))

    def _run(self, uv, idx, n, grid):
        L.ptr(self.table, torch.float32, "table")
        if torch.is_grad_enabled() and self.table.requires_grad:
            return _HashTexFn.apply(self, uv, idx, n, grid, self.table)
        return self._launch_fwd(uv, idx, n, grid, self.table.detach())

    def forward(self, uv):
        if not isinstance(uv, torch.Tensor) or uv.dim() < 1 or uv.shape[-1] != 2:
            raise L.CtxError(f"HashGridEncoding2D: want uv [..., 2], got {tuple(getattr(uv, 'shape', ()))}")
        if torch.is_grad_enabled() and uv.requires_grad:
            raise L.CtxError("HashGridEncoding2D: the HIP path has no gradient with respect to uv; detach uv")
        if uv.device != self.table.device or uv.device.type == 'cpu':
            raise L.CtxError(f"HashGridEncoding2D: uv on {uv.device}, the table on {self.table.device} (the HIP path has no CPU fallback: "
                             "want a device tensor)")
        x = L.f32c(uv).reshape(-1, 2)
        if x.shape[0] == 0:
            return torch.zeros(*uv.shape[:-1], self.out_dim, device=x.device)
        return self._run(x, None, x.shape[0], 0).reshape(*uv.shape[:-1], self.out_dim)

    def forward_texels(self, res, texels=None):
        """The nodes of the res x res atlas (uv = torch.linspace(0, 1, res) on both axes, node y*res + x) -> emb [res*res, out_dim], or with
        texels (int32 [n] device list of nodes) -> emb [n, out_dim] in list order; an entry outside the atlas gives a zero row."""
        if isinstance(res, bool) or not isinstance(res, (int, np.integer)) or not 2 <= res <= 46340:
            raise L.CtxError(f"HashGridEncoding2D.forward_texels: res={res!r}: want an int in [2, 46340]")
        if self.table.device.type == 'cpu':
            raise L.CtxError("HashGridEncoding2D: the table is on the cpu (the HIP path has no CPU fallback: want a device tensor)")
        if texels is None:
            return self._run(None, None, int(res) * int(res), int(res))
        L.ptr(texels, torch.int32, "texels")
        if texels.dim() != 1 or texels.device != self.table.device:
            raise L.CtxError(f"HashGridEncoding2D.forward_texels: want a 1-D int32 list on {self.table.device}, got shape {tuple(texels.shape)} "
                             f"on {texels.device}")
        if texels.numel() == 0:
            return torch.zeros(0, self.out_dim, device=self.table.device)
        return self._run(None, texels, texels.numel(), int(res))


class _TextureHeadFn(torch.autograd.Function):
    """tex [C, plane] = (tanh(raw [n,C]) + 1) / 2 on the nodes the rows name (all of them, or a texel list: zero elsewhere); the gradient
    goes to raw (`ctx_texture_head_bwd`)."""

    @staticmethod
    def forward(ctx, raw, texels, plane):
        ctx.texels, ctx.plane = texels, plane
        ctx.save_for_backward(raw)
        return _texture_head(raw, texels, plane)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_tex):
        raw, = ctx.saved_tensors
        g_raw = torch.empty_like(raw)
        L.check(L.load().ctx_texture_head_bwd(L.ptr(L.f32c(g_tex), torch.float32, "grad_tex"), None, L.ptr(raw), L.ptr(ctx.texels), raw.shape[0],
                                              ctx.plane, raw.shape[1], L.ptr(g_raw), L.stream()))
        return g_raw, None, None


def _texture_head(raw, texels, plane):
    C_ = raw.shape[1]
    tex = torch.empty(C_, plane, device=raw.device) if texels is None else torch.zeros(C_, plane, device=raw.device)
    L.check(L.load().ctx_texture_head_fwd(L.ptr(raw, torch.float32, "raw"), L.ptr(texels), raw.shape[0], plane, C_, L.ptr(tex), L.stream()))
    return tex


class HashGridTexture(nn.Module):
    """The texture field as instant-ngp's image field: HashGridEncoding2D -> NeRF2D(D, W, input_ch = n_levels * n_features, output_ch,
    skips=[0]) on the `emb` seam -> (tanh + 1) / 2.  It answers texture_map(res, texels=None) with NeRF2D.texture_map's contract, which is
    all TexturedMeshModel asks of its field, and forward_uv(uv).  The table's gradient is summed in integers: a run repeats bit for bit."""

    def __init__(self, n_levels=12, n_features=2, log2_table=18, base_res=16, max_res=1024, D=2, W=64, output_ch=3):
        super().__init__()
        self.encoding = HashGridEncoding2D(n_levels, n_features, log2_table, base_res, max_res)
        if D < 2:
            raise L.CtxError(f"HashGridTexture: D={D}: the MLP needs at least two hidden layers (the second one is the skip layer)")
        if not 1 <= output_ch <= 4:
            raise L.CtxError(f"HashGridTexture: output_ch={output_ch} outside [1, 4]")
        self.mlp = NeRF2D(D=D, W=W, input_ch=self.encoding.out_dim, output_ch=output_ch, skips=[0])
        self.output_ch = output_ch

    def _version(self):
        return tuple(p._version for p in self.parameters()) + tuple(p.data_ptr() for p in self.parameters())

    def forward_uv(self, uv):
        """uv [..., 2] -> raw [..., output_ch] (before the head)."""
        return self.mlp.forward_features(self.encoding(uv))

    def _field(self, res, texels):
        raw = self.mlp.forward_features(self.encoding.forward_texels(res, texels))
        plane = res * res
        if torch.is_grad_enabled() and raw.requires_grad:
            tex = _TextureHeadFn.apply(raw, texels, plane)
        else:
            tex = _texture_head(raw, texels, plane)
        return tex.reshape(1, self.output_ch, res, res), raw

    def texture_map(self, res, texels=None):
        """-> (texture [1,C,res,res] in [0,1], mlp_output [res*res, C]), the contract of NeRF2D.texture_map: the no-grad whole-atlas result
        is kept until a parameter's version moves; with texels (int32 [n] device list of distinct nodes y*res + x) the field is evaluated,
        and trained, on those texels only -> (texture, zero off the list; mlp_output [n, C] in list order), never cached.  Listed texels
        carry the bits of the whole-atlas call."""
        if texels is not None:
            return self._field(res, self.mlp._checked_texels(texels, res))
        if not (torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())):
            key = (self._version(), res)
            hit = getattr(self, '_tex_cache', None)
            if hit is not None and hit[0] == key:
                return hit[1], hit[2]
            out = self._field(res, None)
            self._tex_cache = (key, out[0], out[1])
            return out
        return self._field(res, None)
