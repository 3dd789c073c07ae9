"""Texture field + ray helpers: drop-in for src/run_nerf_helpers.py (get_embedder, NeRF2D, get_rays,
ndc_rays, sample_pdf) with the hot ops on libctxnerf.so.

NeRF2D keeps the reference's parameter names (`pts_linears.{i}.{weight,bias}`, `output_linear.*`) and
initialisation order so a reference state_dict loads unchanged and a seeded construction gives the same
weights.  forward(embedded) runs the fused fp32-MFMA kernel; `texture_map(res)` is the fully fused
uv -> embed -> MLP -> (tanh+1)/2 path used by TexturedMeshModel.get_texture_map.
When gradients are enabled and a parameter requires them, the forward keeps the activations
(`ctx_uvmlp_fwd_save`) and `backward` runs `ctx_uvmlp_bwd` (the texture side of the SDS loop,
src/training/trainer.py:644-907): parameter gradients only — uv / the embedding are not trainable inputs.
`NeRF2D.forward_features(emb)` is the exception: the `emb` seam for any width up to 64 (`ctx_uvmlp_fwd_emb`), whose backward
(`ctx_uvmlp_bwd_emb`) also carries the gradient to the embedding; hashgrid.HashGridField trains its table through it.
"""
import ctypes as C
import numpy as np
import torch
import torch.nn as nn
from . import _lib as L

img2mse = lambda x, y: torch.mean((x - y) ** 2)
mse2psnr = lambda x: -10. * torch.log(x) / torch.log(torch.tensor([10.], device=x.device))
to8b = lambda x: (255 * np.clip(x, 0, 1)).astype(np.uint8)


class Embedder:
    def __init__(self, input_dims=2, multires=10):
        self.input_dims, self.multires = input_dims, multires
        self.out_dim = input_dims * (1 + 2 * multires)

    def embed(self, inputs):
        lib = L.load()
        x = L.f32c(inputs).reshape(-1, self.input_dims)
        out = torch.empty(x.shape[0], self.out_dim, device=x.device)
        L.check(lib.ctx_embed_fwd(L.ptr(x, torch.float32, "inputs"), x.shape[0], self.input_dims, self.multires,
                                  L.ptr(out), L.stream()))
        return out.reshape(*inputs.shape[:-1], self.out_dim)


def get_embedder(multires, i=0):
    if i == -1:
        return nn.Identity(), 2
    eo = Embedder(2, multires)
    return (lambda x, eo=eo: eo.embed(x)), eo.out_dim


def _take_saved(net, nbytes, dev):
    """The module's activation store if it is large enough (then the module gives it up until the backward hands it back), else a new one."""
    saved = net._saved_pool if (net._saved_pool is not None and net._saved_pool.numel() >= nbytes
                                and net._saved_pool.device == dev) else None
    net._saved_pool = None
    return saved if saved is not None else torch.empty(nbytes, dtype=torch.uint8, device=dev)


def _return_saved(net, back):
    """Of the stores of two passes the module keeps the larger."""
    pool = net._saved_pool
    if pool is None or pool.device != back.device or pool.numel() <= back.numel():
        net._saved_pool = back


def _bwd_scratch(net, N, dev):
    wsb = L.load().ctx_uvmlp_bwd_ws_bytes(N, net.D, net.W)
    if net._bwd_ws is None or net._bwd_ws.numel() < wsb or net._bwd_ws.device != dev:
        net._bwd_ws = None
        net._bwd_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)     # scratch, stream-ordered: reusable
    return net._bwd_ws


class _UvMlpFn(torch.autograd.Function):
    """(raw [N,C], tex [C,N] or None) = field(uv | emb | grid(res)); gradients flow to the nn.Linear parameters.
    texels (int32 [N], nodes of the res x res grid): the field on those nodes only; tex is then [C,res*res], zero off the list."""

    @staticmethod
    def forward(ctx, net, uv, emb, N, res, want_tex, texels, *params):
        lib = L.load()
        blob = net.packed()
        dev = blob.device
        Lf = (net.input_ch // 2 - 1) // 2
        # the activation store (8.8 GB for the 1024^2 atlas) is kept by the module and handed out to one forward at a time;
        # allocating it per call makes the caching allocator split and re-malloc multi-GB blocks.  The pool only grows: N changes
        # from step to step on the occupancy path, and the kernels take the prefix of the length they need
        saved = _take_saved(net, lib.ctx_uvmlp_saved_bytes(N, net.D, net.W, net.input_ch), dev)
        raw, tex = net._launch_fwd(uv, emb, N, res, want_tex, texels, blob, saved)
        ctx.net, ctx.N, ctx.saved_acts, ctx.blob, ctx.texels, ctx.res = net, N, saved, blob, texels, res
        ctx.save_for_backward(raw)          # an output: kept through save_for_backward so the graph holds no reference cycle
        ctx.set_materialize_grads(False)
        return (raw, tex) if want_tex else raw

    @staticmethod
    def backward(ctx, g_raw, g_tex=None):
        lib = L.load()
        net, N = ctx.net, ctx.N
        raw, = ctx.saved_tensors
        dev = raw.device
        layers = list(net.pts_linears) + [net.output_linear]
        gws = [torch.empty_like(l.weight) for l in layers]
        gbs = [torch.empty_like(l.bias) for l in layers]
        ws = _bwd_scratch(net, N, dev)
        gwp = (C.c_void_p * len(gws))(*[L.ptr(g).value for g in gws])
        gbp = (C.c_void_p * len(gbs))(*[L.ptr(g).value for g in gbs])
        g_raw = None if g_raw is None else L.f32c(g_raw)
        g_tex = None if g_tex is None else L.f32c(g_tex)
        if ctx.texels is None:
            L.check(lib.ctx_uvmlp_bwd(L.ptr(g_raw), L.ptr(g_tex), L.ptr(raw), N, L.ptr(ctx.blob), net.D, net.W, net.dims,
                                      net.multires, net.output_ch, net.skips[0], L.ptr(ctx.saved_acts), L.ptr(ws), gwp, gbp, L.stream()))
        else:
            L.check(lib.ctx_uvmlp_bwd_idx(L.ptr(g_raw), L.ptr(g_tex), L.ptr(ctx.texels), ctx.res, L.ptr(raw), N, L.ptr(ctx.blob), net.D, net.W,
                                          net.multires, net.output_ch, net.skips[0], L.ptr(ctx.saved_acts), L.ptr(ws), gwp, gbp, L.stream()))
        back, ctx.saved_acts = ctx.saved_acts, None                     # back to the module for the next forward
        _return_saved(net, back)
        grads = []
        for w, b in zip(gws, gbs):
            grads += [w, b]
        return (None, None, None, None, None, None, None, *grads)


class _FeatureMlpFn(torch.autograd.Function):
    """raw [N,C] = field(emb [N,input_ch]) on the `emb` seam (`ctx_uvmlp_fwd_emb`); gradients flow to the nn.Linear parameters and, where
    it requires one, to emb (`ctx_uvmlp_bwd_emb`).  Same activation pool and backward scratch as _UvMlpFn."""

    @staticmethod
    def forward(ctx, net, emb, *params):
        lib = L.load()
        blob = net.packed()
        N = emb.shape[0]
        saved = _take_saved(net, lib.ctx_uvmlp_saved_bytes(N, net.D, net.W, net.input_ch), blob.device)
        raw = net._launch_features(emb, blob, saved)
        ctx.net, ctx.N, ctx.saved_acts, ctx.blob = net, N, saved, blob
        ctx.set_materialize_grads(False)
        return raw

    @staticmethod
    def backward(ctx, g_raw):
        lib = L.load()
        net, N = ctx.net, ctx.N
        dev = ctx.blob.device
        layers = list(net.pts_linears) + [net.output_linear]
        nparam = 2 * len(layers)
        if g_raw is None:
            return (None,) * (2 + nparam)
        gws = [torch.empty_like(l.weight) for l in layers]
        gbs = [torch.empty_like(l.bias) for l in layers]
        ws = _bwd_scratch(net, N, dev)
        gwp = (C.c_void_p * len(gws))(*[L.ptr(g).value for g in gws])
        gbp = (C.c_void_p * len(gbs))(*[L.ptr(g).value for g in gbs])
        g_emb = torch.empty(N, net.input_ch, device=dev) if ctx.needs_input_grad[1] else None
        L.check(lib.ctx_uvmlp_bwd_emb(L.ptr(L.f32c(g_raw)), N, L.ptr(ctx.blob), net.D, net.W, net.input_ch, net.output_ch, net.skips[0],
                                      L.ptr(ctx.saved_acts), L.ptr(ws), gwp, gbp, L.ptr(g_emb), L.stream()))
        back, ctx.saved_acts = ctx.saved_acts, None
        _return_saved(net, back)
        grads = []
        for w, b in zip(gws, gbs):
            grads += [w, b]
        return (None, g_emb, *grads)


class NeRF2D(nn.Module):
    def __init__(self, D=8, W=256, input_ch=3, output_ch=4, skips=[4]):
        super().__init__()
        self.D, self.W, self.input_ch, self.output_ch, self.skips = D, W, input_ch, output_ch, list(skips)
        self.pts_linears = nn.ModuleList(
            [nn.Linear(input_ch, W)] +
            [nn.Linear(W, W) if i not in self.skips else nn.Linear(W + input_ch, W) for i in range(D - 1)])
        self.output_linear = nn.Linear(W, output_ch)
        for layer in self.pts_linears:
            nn.init.kaiming_normal_(layer.weight, mode='fan_in', nonlinearity='relu')
        nn.init.kaiming_normal_(self.output_linear.weight, mode='fan_in', nonlinearity='relu')
        self.dims, self.multires = self._infer_dims(input_ch)
        self._packed = None
        self._packed_version = None
        self._saved_pool = None      # activation store of the training forward, reused across iterations
        self._bwd_ws = None          # backward scratch

    @staticmethod
    def _infer_dims(input_ch):
        """input_ch = dims * (1 + 2L) with dims 2 (uv texture field) or 3 (xyz points of the ray path)."""
        for d in (2, 3):
            if input_ch % d == 0 and (input_ch // d - 1) % 2 == 0:
                return d, (input_ch // d - 1) // 2
        return 2, 0          # only the forward(embedded) seam is meaningful then; the kernel rejects it with a message

    # -- weight packing (cached; invalidated by in-place parameter updates via _version) --------------
    def _version(self):
        return tuple(p._version for p in self.parameters()) + tuple(p.data_ptr() for p in self.parameters())

    def packed(self):
        if len(self.skips) != 1:
            raise L.CtxError("NeRF2D HIP path supports exactly one skip connection (the reference uses skips=[4])")
        v = self._version()
        if self._packed is None or self._packed_version != v:
            lib = L.load()
            dev = self.output_linear.weight.device
            n = lib.ctx_uvmlp_packed_bytes(self.D, self.W, self.input_ch, self.output_ch, self.skips[0])
            if n < 0:
                raise L.CtxError(f"NeRF2D(D={self.D},W={self.W},input_ch={self.input_ch},output_ch={self.output_ch}) "
                                 "is outside the fused kernel's envelope (W in 64/128/256, input_ch<=64, output_ch<=4)")
            blob = torch.empty(n, dtype=torch.uint8, device=dev)
            layers = list(self.pts_linears) + [self.output_linear]
            ws = [L.f32c(l.weight.detach()) for l in layers]
            bs = [L.f32c(l.bias.detach()) for l in layers]
            wp = (C.c_void_p * len(ws))(*[L.ptr(w, torch.float32, "weight").value for w in ws])
            bp = (C.c_void_p * len(bs))(*[L.ptr(b, torch.float32, "bias").value for b in bs])
            L.check(lib.ctx_uvmlp_pack(wp, bp, self.D, self.W, self.input_ch, self.output_ch, self.skips[0],
                                       L.ptr(blob), L.stream()))
            self._packed, self._packed_version = blob, v
        return self._packed

    def _params(self):
        out = []
        for l in list(self.pts_linears) + [self.output_linear]:
            out += [l.weight, l.bias]
        return out

    def _launch_fwd(self, uv, emb, N, res, want_tex, texels, blob, saved):
        """One forward launch -> (raw [N,C], tex or None).  texels given: the list entry point, tex [C,res*res] zero off the list."""
        lib = L.load()
        dev = blob.device
        raw = torch.empty(N, self.output_ch, device=dev)
        if texels is None:
            tex = torch.empty(self.output_ch, N, device=dev) if want_tex else None
            L.check(lib.ctx_uvmlp_fwd_save(L.ptr(uv), L.ptr(emb), N, res, L.ptr(blob), self.D, self.W, self.dims, self.multires,
                                           self.output_ch, self.skips[0], L.ptr(raw), L.ptr(tex), L.ptr(saved), L.stream()))
        else:
            if self.dims != 2:
                raise L.CtxError(f"a texel list addresses the 2-D atlas grid; this field has dims={self.dims}")
            tex = torch.zeros(self.output_ch, res * res, device=dev) if want_tex else None
            L.check(lib.ctx_uvmlp_fwd_save_idx(L.ptr(texels), N, res, L.ptr(blob), self.D, self.W, self.multires, self.output_ch,
                                               self.skips[0], L.ptr(raw), L.ptr(tex), L.ptr(saved), L.stream()))
        return raw, tex

    def _run(self, uv, emb, N, res, want_tex, texels=None):
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            r = _UvMlpFn.apply(self, uv, emb, N, res, want_tex, texels, *self._params())
            return r if want_tex else (r, None)
        return self._launch_fwd(uv, emb, N, res, want_tex, texels, self.packed(), None)

    def _checked_texels(self, texels, res):
        """A texel list is looked at once per tensor (dtype, device, range: the range costs a host sync), not per call."""
        seen = getattr(self, '_texels_ok', None)
        if seen is not None and seen[0] is texels and seen[1:] == (texels._version, res):
            return texels
        L.ptr(texels, torch.int32, "texels")
        if texels.dim() != 1:
            raise L.CtxError(f"texels: expected a 1-D int32 list of grid nodes, got shape {tuple(texels.shape)}")
        n = texels.numel()
        if n == 0:
            raise L.CtxError("texels: the list is empty (no texel is sampled); evaluate the whole atlas with texels=None instead")
        if n > res * res:
            raise L.CtxError(f"texels: {n} entries for a {res} x {res} atlas")
        lo, hi = int(texels.min()), int(texels.max())
        if lo < 0 or hi >= res * res:
            raise L.CtxError(f"texels: entries span [{lo}, {hi}], outside the {res} x {res} atlas [0, {res * res})")
        self._texels_ok = (texels, texels._version, res)
        return texels

    def forward(self, x):
        """x: embedded inputs [N, input_ch] (reference seam) -> raw outputs [N, output_ch]."""
        e = L.f32c(x).reshape(-1, self.input_ch)
        raw, _ = self._run(None, e, e.shape[0], 0, False)
        return raw.reshape(*x.shape[:-1], self.output_ch)

    def _launch_features(self, emb, blob, saved):
        raw = torch.empty(emb.shape[0], self.output_ch, device=blob.device)
        L.check(L.load().ctx_uvmlp_fwd_emb(L.ptr(emb, torch.float32, "emb"), emb.shape[0], L.ptr(blob), self.D, self.W, self.input_ch,
                                           self.output_ch, self.skips[0], L.ptr(raw), L.ptr(saved), L.stream()))
        return raw

    def forward_features(self, emb):
        """emb [..., input_ch]: a precomputed embedding of any width input_ch <= 64 (a hash-grid encoding's features) -> [..., output_ch].
        Differentiable in the parameters and in emb; always the exact-f32 kernels.  With input_ch = 63 it is forward(emb) bit for bit."""
        if self.input_ch > 64:
            raise L.CtxError(f"NeRF2D.forward_features: input_ch={self.input_ch} is wider than the fused kernel's 64-column embedding")
        if not isinstance(emb, torch.Tensor) or emb.shape[-1] != self.input_ch:
            raise L.CtxError(f"NeRF2D.forward_features: want emb [..., {self.input_ch}], got {tuple(getattr(emb, 'shape', ()))}")
        e = L.f32c(emb).reshape(-1, self.input_ch)
        L.ptr(e, torch.float32, "emb")
        if e.shape[0] == 0:
            return torch.zeros(*emb.shape[:-1], self.output_ch, device=e.device)
        if torch.is_grad_enabled() and (e.requires_grad or any(p.requires_grad for p in self.parameters())):
            raw = _FeatureMlpFn.apply(self, e, *self._params())
        else:
            raw = self._launch_features(e, self.packed(), None)
        return raw.reshape(*emb.shape[:-1], self.output_ch)

    @torch.no_grad()
    def features_input_gradient(self, emb, g_raw):
        """(raw [N, output_ch], g_emb [N, input_ch]) for emb [N, input_ch] and g_raw [N, output_ch], float32 contiguous device tensors:
        forward_features' launch with the activation store, then `ctx_uvmlp_bwd_emb` for the input gradient alone (no weight-gradient
        launch).  No autograd graph, no .grad; the activation pool goes back to the module as after a backward."""
        lib = L.load()
        blob = self.packed()
        N = emb.shape[0]
        saved = _take_saved(self, lib.ctx_uvmlp_saved_bytes(N, self.D, self.W, self.input_ch), blob.device)
        try:
            raw = self._launch_features(emb, blob, saved)
            g_emb = torch.empty(N, self.input_ch, device=blob.device)
            L.check(lib.ctx_uvmlp_bwd_emb(L.ptr(g_raw, torch.float32, "g_raw"), N, L.ptr(blob), self.D, self.W, self.input_ch, self.output_ch,
                                          self.skips[0], L.ptr(saved), L.ptr(_bwd_scratch(self, N, blob.device)), None, None, L.ptr(g_emb),
                                          L.stream()))
        finally:
            _return_saved(self, saved)
        return raw, g_emb

    def forward_pts(self, pts):
        """Fused embed+MLP on raw points [..., dims] (dims 2: uv, 3: xyz) -> [..., output_ch]."""
        x = L.f32c(pts).reshape(-1, self.dims)
        raw, _ = self._run(x, None, x.shape[0], 0, False)
        return raw.reshape(*pts.shape[:-1], self.output_ch)

    def forward_uv(self, uv):
        """Fused embed+MLP on raw uv [N,2]."""
        u = L.f32c(uv).reshape(-1, 2)
        raw, _ = self._run(u, None, u.shape[0], 0, False)
        return raw

    def texture_map(self, res, texels=None):
        """textured_mesh.py:266-301 fused: -> (texture [1,C,res,res] in [0,1], mlp_output [res*res, C]).
        The reference re-evaluates the field on every render() (2x per painted view, 3x per eval view); without gradients the
        atlas only changes when a parameter does, so the no-grad result is kept until the parameters' version moves.
        texels (int32 [n] device list of distinct nodes y*res + x, e.g. kal.active_texels): the field is evaluated, and trained, on
        those texels only (textured_mesh.py:303-347) -> (texture [1,C,res,res], zero off the list; mlp_output [n, C] in list
        order).  Listed texels carry the bits of the whole-atlas call.  Never cached."""
        if texels is not None:
            texels = self._checked_texels(texels, res)
            raw, tex = self._run(None, None, texels.numel(), res, True, texels)
            return tex.reshape(1, self.output_ch, res, res), raw
        if not (torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())):
            key = (self._version(), res)
            hit = getattr(self, '_tex_cache', None)
            if hit is not None and hit[0] == key:
                return hit[1], hit[2]
            raw, tex = self._run(None, None, res * res, res, True)
            out = (tex.reshape(1, self.output_ch, res, res), raw)
            self._tex_cache = (key, out[0], out[1])
            return out
        raw, tex = self._run(None, None, res * res, res, True)
        return tex.reshape(1, self.output_ch, res, res), raw


# ---- ray helpers (dead code in the reference, named by north_star) ------------------------------------
def get_rays(H, W, K, c2w):
    lib = L.load()
    c = L.f32c(c2w[:3, :4])
    ro = torch.empty(H, W, 3, device=c.device)
    rd = torch.empty(H, W, 3, device=c.device)
    L.check(lib.ctx_get_rays(H, W, float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]), L.ptr(c, torch.float32, "c2w"),
                             L.ptr(ro), L.ptr(rd), L.stream()))
    return ro, rd


def ndc_rays(H, W, focal, near, rays_o, rays_d):
    t = -(near + rays_o[..., 2]) / rays_d[..., 2]
    rays_o = rays_o + t[..., None] * rays_d
    o0 = -1. / (W / (2. * focal)) * rays_o[..., 0] / rays_o[..., 2]
    o1 = -1. / (H / (2. * focal)) * rays_o[..., 1] / rays_o[..., 2]
    o2 = 1. + 2. * near / rays_o[..., 2]
    d0 = -1. / (W / (2. * focal)) * (rays_d[..., 0] / rays_d[..., 2] - rays_o[..., 0] / rays_o[..., 2])
    d1 = -1. / (H / (2. * focal)) * (rays_d[..., 1] / rays_d[..., 2] - rays_o[..., 1] / rays_o[..., 2])
    d2 = -2. * near / rays_o[..., 2]
    return torch.stack([o0, o1, o2], -1), torch.stack([d0, d1, d2], -1)


def sample_pdf(bins, weights, N_samples, det=False, pytest=False, generator=None):
    dev = bins.device
    weights = weights + 1e-5
    pdf = weights / torch.sum(weights, -1, keepdim=True)
    cdf = torch.cumsum(pdf, -1)
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)
    if det:
        u = torch.linspace(0., 1., steps=N_samples, device=dev).expand(list(cdf.shape[:-1]) + [N_samples])
    else:
        u = torch.rand(list(cdf.shape[:-1]) + [N_samples], device=dev, generator=generator)
    if pytest:
        np.random.seed(0)
        new_shape = list(cdf.shape[:-1]) + [N_samples]
        u = np.broadcast_to(np.linspace(0., 1., N_samples), new_shape) if det else np.random.rand(*new_shape)
        u = torch.tensor(np.ascontiguousarray(u), dtype=torch.float32, device=dev)
    u = u.contiguous()
    inds = torch.searchsorted(cdf, u, right=True)
    below = torch.max(torch.zeros_like(inds - 1), inds - 1)
    above = torch.min((cdf.shape[-1] - 1) * torch.ones_like(inds), inds)
    inds_g = torch.stack([below, above], -1)
    matched_shape = [inds_g.shape[0], inds_g.shape[1], cdf.shape[-1]]
    cdf_g = torch.gather(cdf.unsqueeze(1).expand(matched_shape), 2, inds_g)
    bins_g = torch.gather(bins.unsqueeze(1).expand(matched_shape), 2, inds_g)
    denom = cdf_g[..., 1] - cdf_g[..., 0]
    denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    t = (u - cdf_g[..., 0]) / denom
    return bins_g[..., 0] + t * (bins_g[..., 1] - bins_g[..., 0])


def raw_noise(R, S, std, device, pytest=False, generator=None):
    """nerf-pytorch's density noise [R,S]: randn * std, or with pytest=True numpy's seeded uniform draw * std."""
    if pytest:
        np.random.seed(0)
        return torch.tensor(np.random.rand(R, S) * std, dtype=torch.float32, device=device)
    return torch.randn(R, S, device=device, generator=generator) * std


def perturb_z_vals(z_vals, pytest=False, generator=None):
    """nerf-pytorch's stratified jitter: one uniform draw inside each sample's interval [lower, upper] between the midpoints."""
    mids = .5 * (z_vals[..., 1:] + z_vals[..., :-1])
    upper = torch.cat([mids, z_vals[..., -1:]], -1)
    lower = torch.cat([z_vals[..., :1], mids], -1)
    if pytest:
        np.random.seed(0)
        t_rand = torch.tensor(np.random.rand(*list(z_vals.shape)), dtype=torch.float32, device=z_vals.device)
    else:
        t_rand = torch.rand(z_vals.shape, device=z_vals.device, generator=generator)
    return lower + (upper - lower) * t_rand


def _composite_fwd(r, z, d, noise, white_bkgd):
    lib = L.load()
    R, S, _ = r.shape
    dev = r.device
    rgb = torch.empty(R, 3, device=dev); disp = torch.empty(R, device=dev); acc = torch.empty(R, device=dev)
    w = torch.empty(R, S, device=dev); depth = torch.empty(R, device=dev)
    if noise is None:
        L.check(lib.ctx_raymarch_composite_fwd(L.ptr(r, torch.float32, "raw"), L.ptr(z), L.ptr(d), R, S, int(white_bkgd), L.ptr(rgb),
                                               L.ptr(disp), L.ptr(acc), L.ptr(w), L.ptr(depth), L.stream()))
    else:
        L.check(lib.ctx_raymarch_composite_fwd_noise(L.ptr(r, torch.float32, "raw"), L.ptr(z), L.ptr(d), L.ptr(noise, torch.float32, "noise"),
                                                     R, S, int(white_bkgd), L.ptr(rgb), L.ptr(disp), L.ptr(acc), L.ptr(w), L.ptr(depth),
                                                     L.stream()))
    return rgb, disp, acc, w, depth


class _CompositeFn(torch.autograd.Function):
    """raw2outputs with the gradient to raw (`ctx_raymarch_composite_bwd`); the backward recomputes alpha / transmittance /
    acc / depth from the saved inputs, so nothing of size [R,S] is kept beside them."""

    @staticmethod
    def forward(ctx, raw, z, d, noise, white_bkgd):
        out = _composite_fwd(raw, z, d, noise, white_bkgd)
        ctx.save_for_backward(raw, z, d, noise)
        ctx.white = int(white_bkgd)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, g_rgb, g_disp, g_acc, g_w, g_depth):
        lib = L.load()
        raw, z, d, noise = ctx.saved_tensors
        R, S, _ = raw.shape
        gs = [None if g is None else L.f32c(g) for g in (g_rgb, g_disp, g_acc, g_w, g_depth)]
        grad = torch.empty_like(raw)
        L.check(lib.ctx_raymarch_composite_bwd(L.ptr(raw), L.ptr(z), L.ptr(d), L.ptr(noise), R, S, ctx.white, L.ptr(gs[0]),
                                               L.ptr(gs[1]), L.ptr(gs[2]), L.ptr(gs[3]), L.ptr(gs[4]), L.ptr(grad), L.stream()))
        return grad, None, None, None, None


def raw2outputs(raw, z_vals, rays_d, raw_noise_std=0, white_bkgd=False, pytest=False, generator=None):
    """nerf-pytorch raw2outputs (the compositing step src/run_nerf_helpers.py:130-133 points to), as one
    wave-per-ray HIP kernel -> (rgb_map, disp_map, acc_map, weights, depth_map).
    raw_noise_std > 0 adds nerf-pytorch's noise to the density before the ReLU (`raw_noise`).  Under grad mode a `raw` that
    requires grad gets its gradient from `ctx_raymarch_composite_bwd`; gradients go to raw only, so a z_vals or rays_d that
    requires grad is refused instead of silently receiving None."""
    grad_mode = torch.is_grad_enabled()
    if grad_mode and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (z_vals, rays_d)):
        raise L.CtxError("raw2outputs: the HIP path has no gradient with respect to z_vals / rays_d; detach them")
    r, z, d = L.f32c(raw), L.f32c(z_vals), L.f32c(rays_d)
    noise = raw_noise(r.shape[0], r.shape[1], raw_noise_std, r.device, pytest, generator) if raw_noise_std > 0 else None
    if grad_mode and r.requires_grad:
        return _CompositeFn.apply(r, z, d, noise, white_bkgd)
    return _composite_fwd(r, z, d, noise, white_bkgd)


def _packed_fwd(r, t, dt, d, noise, ray_off, white_bkgd):
    lib = L.load()
    n, R, dev = r.shape[0], d.shape[0], d.device
    rgb = torch.empty(R, 3, device=dev); disp = torch.empty(R, device=dev); acc = torch.empty(R, device=dev)
    w = torch.empty(n, device=dev); depth = torch.empty(R, device=dev)
    L.check(lib.ctx_raymarch_packed_fwd(L.ptr(r, torch.float32, "raw"), L.ptr(t, torch.float32, "t"), L.ptr(dt, torch.float32, "dt"),
                                        L.ptr(d, torch.float32, "rays_d"), L.ptr(noise), L.ptr(ray_off, torch.int64, "ray_off"), R, n,
                                        int(white_bkgd), L.ptr(rgb), L.ptr(disp), L.ptr(acc), L.ptr(w), L.ptr(depth), L.stream()))
    return rgb, disp, acc, w, depth


class _PackedCompositeFn(torch.autograd.Function):
    """raw2outputs_packed with the gradient to raw (`ctx_raymarch_packed_bwd`): as _CompositeFn, only the inputs are saved."""

    @staticmethod
    def forward(ctx, raw, t, dt, d, noise, ray_off, white_bkgd):
        out = _packed_fwd(raw, t, dt, d, noise, ray_off, white_bkgd)
        ctx.save_for_backward(raw, t, dt, d, noise, ray_off)
        ctx.white = int(white_bkgd)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, g_rgb, g_disp, g_acc, g_w, g_depth):
        lib = L.load()
        raw, t, dt, d, noise, ray_off = ctx.saved_tensors
        gs = [None if g is None else L.f32c(g) for g in (g_rgb, g_disp, g_acc, g_w, g_depth)]
        grad = torch.empty_like(raw)
        L.check(lib.ctx_raymarch_packed_bwd(L.ptr(raw), L.ptr(t), L.ptr(dt), L.ptr(d), L.ptr(noise), L.ptr(ray_off), d.shape[0], raw.shape[0],
                                            ctx.white, L.ptr(gs[0]), L.ptr(gs[1]), L.ptr(gs[2]), L.ptr(gs[3]), L.ptr(gs[4]), L.ptr(grad),
                                            L.stream()))
        return grad, None, None, None, None, None, None


def raw2outputs_packed(raw, t, dt, rays_d, ray_off, raw_noise_std=0, white_bkgd=False, generator=None):
    """raw2outputs on ragged per-ray sample lists (OccupancyGrid.march): ray r holds the samples ray_off[r] .. ray_off[r+1] of raw [n,4],
    t [n] and dt [n]; rays_d [R,3], ray_off int64 [R+1] -> (rgb [R,3], disp [R], acc [R], weights [n], depth [R]).
    It is the dense kernel with a per-ray sample count and the given distance dt * |rays_d|: no sample gets the 1e10 distance, so the
    background shows through what the lists leave, and a ray without samples gets acc = depth = 0, rgb 0 (or white) and the 0 / 0
    disparity of a dense ray of zero density.  raw_noise_std > 0 adds randn(n) * std to the density before the ReLU.  Gradients go
    to raw only (`ctx_raymarch_packed_bwd`, at most 4096 samples per ray): a t, dt or rays_d that requires grad is refused."""
    grad_mode = torch.is_grad_enabled()
    if grad_mode and any(isinstance(x, torch.Tensor) and x.requires_grad for x in (t, dt, rays_d)):
        raise L.CtxError("raw2outputs_packed: the HIP path has no gradient with respect to t / dt / rays_d; detach them")
    r, t, dt, d = L.f32c(raw), L.f32c(t), L.f32c(dt), L.f32c(rays_d).reshape(-1, 3)
    n = r.shape[0]
    if r.dim() != 2 or r.shape[1] != 4 or t.shape != (n,) or dt.shape != (n,) or ray_off.shape != (d.shape[0] + 1,):
        raise L.CtxError(f"raw2outputs_packed: want raw [n,4], t [n], dt [n], rays_d [R,3], ray_off [R+1]; got {tuple(r.shape)}, "
                         f"{tuple(t.shape)}, {tuple(dt.shape)}, {tuple(d.shape)}, {tuple(ray_off.shape)}")
    noise = torch.randn(n, device=r.device, generator=generator) * raw_noise_std if raw_noise_std > 0 else None
    if grad_mode and r.requires_grad:
        return _PackedCompositeFn.apply(r, t, dt, d, noise, ray_off, white_bkgd)
    return _packed_fwd(r, t, dt, d, noise, ray_off, white_bkgd)


def _distortion_fwd(w, t, dt, d, ray_off):
    lib = L.load()
    R, n = d.shape[0], w.shape[0]
    loss = torch.empty(R, device=d.device)
    L.check(lib.ctx_distortion_packed_fwd(L.ptr(w, torch.float32, "weights"), L.ptr(t, torch.float32, "t"), L.ptr(dt, torch.float32, "dt"),
                                          L.ptr(d, torch.float32, "rays_d"), L.ptr(ray_off, torch.int64, "ray_off"), R, n, L.ptr(loss),
                                          L.stream()))
    return loss


class _DistortionFn(torch.autograd.Function):
    """distortion_loss with the gradient to the weights (`ctx_distortion_packed_bwd`): only the inputs are saved, no double backward."""

    @staticmethod
    def forward(ctx, w, t, dt, d, ray_off):
        ctx.save_for_backward(w, t, dt, d, ray_off)
        return _distortion_fwd(w, t, dt, d, ray_off)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss):
        lib = L.load()
        w, t, dt, d, ray_off = ctx.saved_tensors
        grad = torch.empty_like(w)
        L.check(lib.ctx_distortion_packed_bwd(L.ptr(w), L.ptr(t), L.ptr(dt), L.ptr(d), L.ptr(ray_off), d.shape[0], w.shape[0],
                                              L.ptr(L.f32c(g_loss)), L.ptr(grad), L.stream()))
        return grad, None, None, None, None


def distortion_loss(weights, t, dt, rays_d, ray_off=None):
    """mip-NeRF 360's distortion loss of each ray's weights, as nerfacc's distortion(weights, t_starts, t_ends, packed_info), by two
    wave-per-ray HIP kernels on the ragged lists of OccupancyGrid.march: weights [n], t [n], dt [n], rays_d [R,3], ray_off int64 [R+1]
    -> loss [R] with loss[r] = sum_i sum_j w_i w_j |x_i - x_j| + (1/3) sum_i w_i^2 delta_i over the ray's samples, x = (t - t_0) * |rays_d|
    and delta = dt * |rays_d|: world lengths, so the value does not depend on |rays_d|.  The position is the sample's own t, where the
    density was evaluated.  t ascending inside a ray is a precondition (the march and z_vals satisfy it).  A ray without samples and a
    zero direction give 0; a non-finite weight poisons its own ray only; any number of samples per ray.
    ray_off=None takes the rectangular layout of the dense path: weights [R,S], t = z_vals [R,S], and dt is ignored and taken as
    z[:,1:] - z[:,:-1] with 0 for the last sample, whose interval is the unbounded one and has no width to spread over.
    Gradients go to weights only (`ctx_distortion_packed_bwd`): a t, dt or rays_d that requires grad is refused."""
    grad_mode = torch.is_grad_enabled()
    if grad_mode and any(isinstance(x, torch.Tensor) and x.requires_grad for x in (t, dt, rays_d)):
        raise L.CtxError("distortion_loss: the HIP path has no gradient with respect to t / dt / rays_d; detach them")
    w, t, d = L.f32c(weights), L.f32c(t), L.f32c(rays_d).reshape(-1, 3)
    R = d.shape[0]
    if ray_off is None:
        if w.dim() != 2 or w.shape[0] != R or t.shape != w.shape:
            raise L.CtxError(f"distortion_loss: without ray_off want weights [R,S], t [R,S], rays_d [R,3]; got {tuple(w.shape)}, "
                             f"{tuple(t.shape)}, {tuple(d.shape)}")
        S = w.shape[1]
        ray_off = torch.arange(R + 1, device=w.device, dtype=torch.int64) * S
        dt = torch.cat([t[:, 1:] - t[:, :-1], torch.zeros(R, 1, device=w.device)], -1)
        w, t = w.reshape(-1), t.reshape(-1)
    dt = L.f32c(dt).reshape(-1)
    n = w.shape[0]
    if w.dim() != 1 or t.shape != (n,) or dt.shape != (n,) or ray_off.shape != (R + 1,):
        raise L.CtxError(f"distortion_loss: want weights [n], t [n], dt [n], rays_d [R,3], ray_off [R+1]; got {tuple(w.shape)}, "
                         f"{tuple(t.shape)}, {tuple(dt.shape)}, {tuple(d.shape)}, {tuple(ray_off.shape)}")
    if grad_mode and w.requires_grad:
        return _DistortionFn.apply(w, t, dt, d, ray_off)
    return _distortion_fwd(w, t, dt, d, ray_off)


def weighted_sum_packed(weights, values, ray_off):
    """Per-ray weighted sums on ragged per-ray sample lists (`ctx_weighted_sum_packed`, one wavefront per ray): weights [n], values [n,C]
    with 1 <= C <= 4, ray_off int64 [R+1] -> out [R,C] with out[r] = sum_i weights[i] * values[i] over the ray's samples, zeros for a ray
    without samples.  What torch.zeros(R, C).index_add_(0, ray_id, weights[:, None] * values) computes, without float atomics: one summation
    order, so two runs give the same bits.  No autograd: an input that requires grad is refused."""
    if not all(isinstance(x, torch.Tensor) for x in (weights, values, ray_off)):
        raise L.CtxError("weighted_sum_packed: want tensors weights [n], values [n,C], ray_off [R+1]")
    if weights.requires_grad or values.requires_grad:
        raise L.CtxError("weighted_sum_packed: the sum has no gradient with respect to weights / values; detach them")
    n = weights.shape[0] if weights.dim() == 1 else -1
    if n < 0 or values.dim() != 2 or values.shape[0] != n or ray_off.dim() != 1 or ray_off.shape[0] < 2:
        raise L.CtxError(f"weighted_sum_packed: want weights [n], values [n,C], ray_off [R+1] with R >= 1; got {tuple(weights.shape)}, "
                         f"{tuple(values.shape)}, {tuple(ray_off.shape)}")
    Cn, R = values.shape[1], ray_off.shape[0] - 1
    if not 1 <= Cn <= 4:
        raise L.CtxError(f"weighted_sum_packed: values has C={Cn} columns: want 1 <= C <= 4")
    if n >= 2 ** 31:
        raise L.CtxError(f"weighted_sum_packed: n={n}: want n < 2^31; split the batch")
    p = (L.ptr(weights, torch.float32, "weights"), L.ptr(values, torch.float32, "values"), L.ptr(ray_off, torch.int64, "ray_off"))
    out = torch.empty(R, Cn, device=ray_off.device)
    L.check(L.load().ctx_weighted_sum_packed(*p, R, n, Cn, L.ptr(out), L.stream()))
    return out


RESAMPLE_MAX_K = 4096          # the fine lists are composited too: what the compositing backward holds per ray


def _check_resample(resample, who):
    """resample= as an int: 0 (off) or the fine samples per hit ray in [1, 4096]; anything else is refused."""
    if isinstance(resample, bool) or not isinstance(resample, (int, np.integer)) or not 0 <= resample <= RESAMPLE_MAX_K:
        raise L.CtxError(f"{who}: resample={resample!r}: want 0 (off) or an int in [1, {RESAMPLE_MAX_K}], the fine samples per hit ray")
    return int(resample)


def resample_packed(weights, ts, dt, ray_off, rays_o, rays_d, K, perturb=False, generator=None):
    """Importance resampling of ragged per-ray sample lists, as nerf-pytorch's sample_pdf and nerfacc's resampling do it, by one
    wave-per-ray HIP kernel (`ctx_resample_packed`; the rule: tests/resample_rule.py).  weights [n], ts [n] (interval
    starts: OccupancyGrid.march(starts=True)), dt [n], ray_off int64 [R+1], rays_o / rays_d [R,3]
    -> (ray_off' int64 [R+1], ray_id' int32 [n'], t' [n'], dt' [n'], pts' [n',3]): every ray with samples gets exactly K fine samples
    (ray_off' = K * cumsum(count > 0), n' = K * hit rays), a ray without samples none.  Fine sample k sits where the ray's CDF of
    m = min(max(w, 0), 1) + 1e-5 reaches (k + xi_k)/K, xi = 0.5 or with perturb one uniform draw per fine sample (stratified), always
    inside a coarse interval; the widths dt' are the strata's occupied lengths, so they tile what the coarse widths tile.
    Reading n' back SYNCS the host: a second sync after the march's, kept apart because the march returns before the weights exist.
    Nothing here has a gradient: a weights, ts or dt that requires grad is refused."""
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= K <= RESAMPLE_MAX_K:
        raise L.CtxError(f"resample_packed: K={K!r}: want an int in [1, {RESAMPLE_MAX_K}]")
    if any(isinstance(x, torch.Tensor) and x.requires_grad for x in (weights, ts, dt)):
        raise L.CtxError("resample_packed: the resampling has no gradient with respect to weights / ts / dt; detach them")
    if not all(isinstance(x, torch.Tensor) for x in (weights, ts, dt, ray_off, rays_o, rays_d)):
        raise L.CtxError("resample_packed: want tensors weights [n], ts [n], dt [n], ray_off [R+1], rays_o [R,3], rays_d [R,3]")
    n = weights.shape[0] if weights.dim() == 1 else -1
    R = rays_d.shape[0] if rays_d.dim() == 2 else -1
    if (n < 0 or R < 1 or ts.shape != (n,) or dt.shape != (n,) or ray_off.shape != (R + 1,) or tuple(rays_o.shape) != (R, 3)
            or tuple(rays_d.shape) != (R, 3)):
        raise L.CtxError(f"resample_packed: want weights [n], ts [n], dt [n], ray_off [R+1], rays_o [R,3], rays_d [R,3]; got "
                         f"{tuple(weights.shape)}, {tuple(ts.shape)}, {tuple(dt.shape)}, {tuple(ray_off.shape)}, {tuple(rays_o.shape)}, "
                         f"{tuple(rays_d.shape)}")
    K = int(K)
    p = (L.ptr(weights, torch.float32, "weights"), L.ptr(ts, torch.float32, "ts"), L.ptr(dt, torch.float32, "dt"),
         L.ptr(ray_off, torch.int64, "ray_off"), L.ptr(rays_o, torch.float32, "rays_o"), L.ptr(rays_d, torch.float32, "rays_d"))
    dev = rays_d.device
    fine_off = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    torch.cumsum(ray_off[1:] > ray_off[:-1], 0, dtype=torch.int64, out=fine_off[1:])
    fine_off *= K
    n1 = int(fine_off[R].item())                                                           # the second host sync
    if n1 >= 2 ** 31:
        raise L.CtxError(f"resample_packed: {n1} fine samples on {R} rays: want n' < 2^31; split the batch")
    xi = torch.rand(n1, device=dev, generator=generator) if perturb else None
    ray_id = torch.empty(n1, dtype=torch.int32, device=dev)
    t1, dt1, pts = torch.empty(n1, device=dev), torch.empty(n1, device=dev), torch.empty(n1, 3, device=dev)
    L.check(L.load().ctx_resample_packed(*p, R, n, K, L.ptr(fine_off), L.ptr(xi), n1, L.ptr(ray_id), L.ptr(t1), L.ptr(dt1), L.ptr(pts),
                                         L.stream()))
    return fine_off, ray_id, t1, dt1, pts


def _field_on_list(field, pts, rd, ray_id, view_dirs):
    """-> (raw [n,4], res [n,3] or None): a view-dependent field (field.view_dependent) asked with view_dirs answers forward_dirs with its
    colour residual, any other field, and any field without view_dirs, forward_pts as before."""
    if view_dirs and getattr(field, 'view_dependent', False):
        raw, res = field.forward_dirs(pts, rd, ray_id, return_residual=True)
        return L.f32c(raw), res
    return L.f32c(field.forward_pts(pts)), None


def _refuse_view_dependent(field, who):
    """The dense [R,S] passes have no ray index per sample to hand a view-dependent field: it renders on the marched lists only."""
    if getattr(field, 'view_dependent', False):
        raise L.CtxError(f"{who}: a view-dependent field ({type(field).__name__}) renders on the marched lists only: it needs march= (with "
                         "occupancy=); the dense [R,S] passes do not carry the directions")


def render_rays_marched(field, rays_o, rays_d, near, far, occupancy, step, white_bkgd=False, perturb=0., raw_noise_std=0., generator=None,
                        return_extras=False, resample=0, view_dirs=True):
    """The ray path on ragged per-ray sample lists, as instant-ngp and nerfacc march: occupancy.march places samples `step` apart (a
    world length) inside each ray's runs of occupied cells and nowhere else, field.forward_pts runs on exactly those n points, and
    raw2outputs_packed composites the lists directly: no expansion, no fill, no [R,S] tensor; one host sync (n).
    -> (rgb [R,3], disp [R], acc [R], weights [n], depth [R]); return_extras=True adds dict(ray_off, ray_id, t, dt, pts).
    perturb > 0 draws one uniform offset per sample inside its interval.  n = 0: the field is not called, every ray is empty and
    the outputs carry no autograd graph.
    resample=K > 0 adds the hierarchical pass on the lists: march(starts=True), the field on the n coarse points, raw2outputs_packed,
    resample_packed on the detached coarse weights (perturb > 0: stratified draws), the field on the n' = K * (hit rays) fine points,
    raw2outputs_packed on (t', dt', ray_off').  The returned tuple is the fine one (weights [n']); the extras' ray_off / ray_id / t / dt /
    pts are the fine lists, the coarse pass is kept as rgb0 / disp0 / acc0 / weights0 / depth0 (part of the autograd graph) and
    ray_off0 / ray_id0 / t0 / dt0 / pts0.  The generator is drawn from in a fixed order: the march's u, the coarse noise, xi, the fine
    noise.  Two host syncs (n, n').  n = 0: no field call and no fine pass; the coarse keys hold the same empty-ray outputs.
    view_dirs: a field with view_dependent = True (hashgrid.ViewDependentField) is asked forward_dirs(pts, rays_d, ray_id) in both passes,
    each with its own ray_id, and the extras gain `residual` [n,3], its colour residual on the returned lists (`residual0` [n0,3]: on the
    coarse ones, with resample); view_dirs=False asks it forward_pts, its base term.  Any other field never sees the argument."""
    K = _check_resample(resample, "render_rays_marched")
    vd = bool(view_dirs) and getattr(field, 'view_dependent', False)
    if occupancy is None:
        raise L.CtxError("render_rays_marched: march needs an occupancy grid (occupancy=): the samples lie in its occupied cells")
    ro, rd = L.f32c(rays_o).reshape(-1, 3), L.f32c(rays_d).reshape(-1, 3)
    ray_off, ray_id, t, dt, pts, *ts = occupancy.march(ro, rd, near, far, step, perturb=perturb > 0., generator=generator, starts=K > 0)
    raw, res = _field_on_list(field, pts, rd, ray_id, vd) if t.numel() else (torch.empty(0, 4, device=ro.device), None)
    if vd and res is None:
        res = torch.zeros(0, 3, device=ro.device)
    out = raw2outputs_packed(raw, t, dt, rd, ray_off, raw_noise_std, white_bkgd, generator)
    extras = {}
    if K > 0:
        extras = {'rgb0': out[0], 'disp0': out[1], 'acc0': out[2], 'weights0': out[3], 'depth0': out[4], 'ray_off0': ray_off,
                  'ray_id0': ray_id, 't0': t, 'dt0': dt, 'pts0': pts}
        if vd:
            extras['residual0'] = res
        if t.numel():
            ray_off, ray_id, t, dt, pts = resample_packed(out[3].detach(), ts[0], dt, ray_off, ro, rd, K, perturb=perturb > 0.,
                                                          generator=generator)
            raw, res = _field_on_list(field, pts, rd, ray_id, vd)
            out = raw2outputs_packed(raw, t, dt, rd, ray_off, raw_noise_std, white_bkgd, generator)
    extras.update({'ray_off': ray_off, 'ray_id': ray_id, 't': t, 'dt': dt, 'pts': pts})
    if vd:
        extras['residual'] = res
    return (out, extras) if return_extras else out


def _occ_expand(raw_c, idx, total):
    lib = L.load()
    raw = torch.empty(total, 4, device=idx.device)
    n = idx.numel()
    L.check(lib.ctx_occ_expand(L.ptr(raw_c, torch.float32, "raw_c") if n else None, L.ptr(idx, torch.int32, "idx") if n else None, n,
                               total, L.ptr(raw), L.stream()))
    return raw


class _OccExpandFn(torch.autograd.Function):
    """raw [total,4] = the fill with row idx[k] = raw_c[k] (`ctx_occ_expand`); the gradient to raw_c is the gather `ctx_occ_collect`."""

    @staticmethod
    def forward(ctx, raw_c, idx, total):
        ctx.save_for_backward(idx)
        ctx.total = total
        return _occ_expand(raw_c, idx, total)

    @staticmethod
    def backward(ctx, g):
        lib = L.load()
        idx, = ctx.saved_tensors
        g = L.f32c(g)
        grad_c = torch.empty(idx.numel(), 4, device=g.device)
        L.check(lib.ctx_occ_collect(L.ptr(g), L.ptr(idx), idx.numel(), ctx.total, L.ptr(grad_c), L.stream()))
        return grad_c, None, None


def field_on_occupied(field, occupancy, ro, rd, z_vals):
    """raw [R,S,4] of one pass with the field evaluated on the occupied samples only: occupancy.select (mark + compaction, one host
    sync for n) -> ctx_occ_points -> field.forward_pts on the n points -> ctx_occ_expand.  Every other sample holds the fill
    (0, 0, 0, -1e30): zero density for the compositing.  n = 0: the field is not called and raw is all fill (no autograd node)."""
    lib = L.load()
    R, S = z_vals.shape
    idx = occupancy.select(ro, rd, z_vals)
    n = idx.numel()
    if n == 0:
        return _occ_expand(None, idx, R * S).view(R, S, 4)
    pts = torch.empty(n, 3, device=ro.device)
    L.check(lib.ctx_occ_points(L.ptr(ro), L.ptr(rd), L.ptr(z_vals), R, S, L.ptr(idx), n, L.ptr(pts), L.stream()))
    raw_c = L.f32c(field.forward_pts(pts))
    if torch.is_grad_enabled() and raw_c.requires_grad:
        return _OccExpandFn.apply(raw_c, idx, R * S).view(R, S, 4)
    return _occ_expand(raw_c, idx, R * S).view(R, S, 4)


def render_rays(field, rays_o, rays_d, near, far, N_samples, white_bkgd=False, z_vals=None, perturb=0., raw_noise_std=0.,
                N_importance=0, pytest=False, generator=None, return_extras=False, occupancy=None, clip=False, march=None, resample=0):
    """The ray path north_star names (absent in the reference): nerf-pytorch's render_rays —
    z_vals = near*(1-t)+far*t for t = linspace(0,1,N_samples) (or the given z_vals, e.g. from sample_pdf), pts = o + d*z,
    raw = field(pts) with field = NeRF2D(input_ch = 3*(1+2L), output_ch = 4) evaluated by the fused embed+MLP kernel, then
    raw2outputs.  rays_o, rays_d: [R,3] -> (rgb [R,3], disp [R], acc [R], weights [R,S], depth [R]).
    perturb > 0 jitters the samples inside their intervals (`perturb_z_vals`), raw_noise_std > 0 adds the density noise, and
    N_importance > 0 adds the hierarchical pass: sample_pdf (deterministic when perturb == 0) on the detached coarse weights,
    merged and sorted with the coarse samples and evaluated by the same field; the returned tuple is then the fine one.
    return_extras=True returns (outputs, extras) with extras = dict(z_vals) and, after a hierarchical pass, the coarse
    rgb0 / disp0 / acc0 / weights0 / depth0 (part of the autograd graph) and z_fine.
    occupancy (volume_render.OccupancyGrid): the coarse and the hierarchical pass evaluate the field only on the samples inside
    occupied cells (`field_on_occupied`); every other sample composites as empty space.  A listed sample's point, raw and gradient
    carry the bits the same rows give in a dense-ordered launch of those n points; one host sync per pass.  With a grid that is
    all occupied over a box holding every sample the results equal occupancy=None bit for bit.
    clip=True (needs occupancy, and no z_vals of the caller's): every ray spreads its N_samples over its own span, from where it enters
    its first to where it leaves its last occupied cell (occupancy.ray_spans): z_vals = t0*(1-t) + t1*t with the same linspace t.  The
    jitter, the hierarchical pass and the compositing then run on those z_vals as they do on any.  A ray that meets no occupied cell
    keeps near .. far, where the selection finds nothing for it.  No further host sync.
    march=step (needs occupancy; refuses clip=True, N_importance > 0, given z_vals and pytest=True, because it places and draws the samples itself): the
    pass is render_rays_marched with that world-space step, N_samples is unused and weights is the flat list [n].
    resample=K (an int in [1, 4096]; needs march): the march becomes the coarse pass and every hit ray gets K fine samples drawn from its
    coarse weights, the hierarchical pass of the lists (render_rays_marched); the returned tuple is the fine one.  0: off.
    A view-dependent field (hashgrid.ViewDependentField) needs march=: without it it is refused."""
    if _check_resample(resample, "render_rays") and march is None:
        raise L.CtxError("render_rays: resample= resamples the marched lists; it needs march=")
    if march is not None:
        if clip:
            raise L.CtxError("render_rays: march= places the samples itself; it cannot be combined with clip=True")
        if N_importance > 0:
            raise L.CtxError("render_rays: march= has no hierarchical pass; it cannot be combined with N_importance > 0")
        if z_vals is not None:
            raise L.CtxError("render_rays: march= places the samples itself; it cannot be combined with given z_vals")
        if pytest:
            raise L.CtxError("render_rays: march= draws its jitter and noise from torch (generator=); it cannot be combined with pytest=True")
        return render_rays_marched(field, rays_o, rays_d, near, far, occupancy, march, white_bkgd=white_bkgd, perturb=perturb,
                                   raw_noise_std=raw_noise_std, generator=generator, return_extras=return_extras, resample=resample)
    _refuse_view_dependent(field, "render_rays")
    if clip and occupancy is None:
        raise L.CtxError("render_rays: clip=True needs an occupancy grid (occupancy=): the spans are those of its occupied cells")
    if clip and z_vals is not None:
        raise L.CtxError("render_rays: clip=True places the samples itself; it cannot be combined with given z_vals")
    ro, rd = L.f32c(rays_o).reshape(-1, 3), L.f32c(rays_d).reshape(-1, 3)
    if clip:
        span, _ = occupancy.ray_spans(ro, rd, near, far)
        t = torch.linspace(0., 1., steps=N_samples, device=ro.device)
        z_vals = span[:, :1] * (1. - t) + span[:, 1:] * t
    elif z_vals is None:
        t = torch.linspace(0., 1., steps=N_samples, device=ro.device)
        z_vals = (near * (1. - t) + far * t).expand(ro.shape[0], N_samples)
    elif occupancy is not None and z_vals.requires_grad:
        raise L.CtxError("render_rays(occupancy=): the sample selection has no gradient with respect to z_vals; detach them")
    if perturb > 0.:
        z_vals = perturb_z_vals(z_vals, pytest, generator)
    z_vals = L.f32c(z_vals)
    if occupancy is None:
        pts = ro[:, None, :] + rd[:, None, :] * z_vals[:, :, None]          # [R,S,3]
        raw = field.forward_pts(pts)                                         # [R,S,4]
    else:
        raw = field_on_occupied(field, occupancy, ro, rd, z_vals)
    out = raw2outputs(raw, z_vals, rd, raw_noise_std, white_bkgd, pytest, generator)
    extras = {'z_vals': z_vals}
    if N_importance > 0:
        z_mid = .5 * (z_vals[..., 1:] + z_vals[..., :-1])
        z_fine = sample_pdf(z_mid, out[3][..., 1:-1].detach(), N_importance, det=(perturb == 0.), pytest=pytest, generator=generator)
        z_all, _ = torch.sort(torch.cat([z_vals, z_fine], -1), -1)
        z_all = z_all.contiguous()
        extras = {'z_vals': z_all, 'z_fine': z_fine, 'rgb0': out[0], 'disp0': out[1], 'acc0': out[2], 'weights0': out[3],
                  'depth0': out[4]}
        if occupancy is None:
            pts = ro[:, None, :] + rd[:, None, :] * z_all[:, :, None]
            raw = field.forward_pts(pts)
        else:
            raw = field_on_occupied(field, occupancy, ro, rd, z_all)
        out = raw2outputs(raw, z_all, rd, raw_noise_std, white_bkgd, pytest, generator)
    return (out, extras) if return_extras else out
