"""Multiresolution hash-grid field (instant-ngp): a table of trainable features, trilinearly interpolated at Lv resolutions, feeding a small
MLP.  HashGridEncoding is the table with `ctx_hashgrid_fwd` / `ctx_hashgrid_bwd` (csrc/hashgrid.hip; the rule: tests/hashgrid_rule.py,
DESIGN section 4j); HashGridField adds NeRF2D(D=2, W=64) on the `emb` seam (NeRF2D.forward_features, which carries the gradient back to the
features).  The field answers forward_pts(pts [...,3]) -> [...,4], which is all the ray path asks of a field: it goes into render_rays,
render_rays_marched, render_image, render_and_refine, train_step, fit_views and OccupancyGrid.update as NeRF2D does.
The table's gradient is summed in 64-bit integers, so a training run repeats bit for bit.  Positions get a gradient
(`ctx_hashgrid_bwd_pts`; the rule: tests/hashgrid_grad_rule.py) where it is asked for: through autograd with
grad_pts=True, and from HashGridField.density_gradient, which volume_render.render_normals turns into rendered normals.  That gradient is
first order only."""
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
        lib = L.load()
        g_emb = L.f32c(g_emb)
        g_table = None
        if ctx.needs_input_grad[2]:
            wsb = lib.ctx_hashgrid_bwd_ws_bytes(enc.n_levels, enc.n_features, enc.log2_table)
            if enc._bwd_ws is None or enc._bwd_ws.numel() < wsb or enc._bwd_ws.device != table.device:
                enc._bwd_ws = None
                enc._bwd_ws = torch.empty(wsb, dtype=torch.uint8, device=table.device)   # the int64 accumulator: scratch, stream-ordered
            g_table = torch.empty_like(table)
            L.check(lib.ctx_hashgrid_bwd(L.ptr(pts), pts.shape[0], L.ptr(g_emb), *enc._grid_args(), 7, L.ptr(enc._bwd_ws), L.ptr(g_table),
                                         L.stream()))
        g_pts = enc._launch_bwd_pts(pts, table, g_emb) if ctx.needs_input_grad[1] else None
        return None, g_pts, g_table


class HashGridEncoding(nn.Module):
    """pts [..., 3] inside the box lo .. hi -> features [..., n_levels * n_features]: at every level the trilinear interpolation of the 8
    table entries at the corners of the point's cell; a level whose (res + 1)^3 nodes fit the table indexes it directly, a finer one by
    instant-ngp's spatial hash.  Points outside the box take the values on its surface; NaN coordinates read as lo.
    lo, hi: a number or three per axis, finite, lo < hi.  1 <= n_levels <= 16, n_features in {1, 2, 4}, n_levels * n_features <= 64,
    4 <= log2_table <= 22, 1 <= base_res <= max_res <= 2^20.  `table` [n_levels, 2^log2_table, n_features] starts uniform in +-1e-4.
    grad_pts=False: a pts that requires grad is refused.  grad_pts=True: it gets its gradient (`ctx_hashgrid_bwd_pts`): the derivative of the
    interpolation in the cell the point lies in, one-sided on cell faces, and 0 on an axis on or outside the box faces.  First order only:
    a loss on that gradient (on normals, an eikonal term) cannot be trained through."""

    def __init__(self, lo, hi, n_levels=16, n_features=2, log2_table=19, base_res=16, max_res=2048, grad_pts=False):
        super().__init__()
        who = "HashGridEncoding"
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
        lo = np.broadcast_to(np.asarray(lo, np.float32), (3,)).copy()
        hi = np.broadcast_to(np.asarray(hi, np.float32), (3,)).copy()
        if not bool(np.all(np.isfinite(lo))) or not bool(np.all(lo < hi)) or not bool(np.all(np.isfinite(hi - lo))):
            raise L.CtxError(f"{who}: the box needs finite lo < hi on every axis, got lo={lo.tolist()}, hi={hi.tolist()}")
        self.lo, self.hi = lo, hi
        self.n_levels, self.n_features, self.log2_table = int(n_levels), int(n_features), int(log2_table)
        self.res = level_resolutions(self.n_levels, int(base_res), int(max_res))
        self.out_dim = self.n_levels * self.n_features
        self.table = nn.Parameter((torch.rand(self.n_levels, 1 << self.log2_table, self.n_features) * 2 - 1) * 1e-4)
        self._bwd_ws = None
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
