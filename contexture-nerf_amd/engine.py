"""HipEngine: what the Python classes over an engine handle of libctxnerf.so share (UNet2DConditionModel / ControlNetModel over
`ctx_unet_*`, AutoencoderKL over `ctx_vae_*`): the handle, the parameter table with diffusers' state_dict names, the fp16 weight
blob, the workspace that grows on demand, and loading / seeded random initialisation of the weights."""
import ctypes as C
import math
import torch
from . import _lib as L


class HipEngine:
    _prefix = None            # C prefix of the engine's entry points: 'ctx_unet' / 'ctx_vae'

    def __init__(self, config, device="cuda:0", seed=0, init=True):
        self.config = config
        self.device = torch.device(device)
        self._lib = L.load()
        self._h = self._create_handle()
        self._names, self._shapes = [], []
        shp = (C.c_int64 * 4)()
        for i in range(self._c('param_count')(self._h)):
            nd = self._c('param_shape')(self._h, i, shp)
            self._names.append(self._c('param_name')(self._h, i).decode())
            self._shapes.append(tuple(int(shp[k]) for k in range(nd)))
        self._index = {n: i for i, n in enumerate(self._names)}
        self._weights = None
        self._derived = None
        self._derived_on = True
        self._ws = None
        self._ws_key = None
        self._t = None
        self._init_state()
        if self.device.type == 'cuda':
            self._weights = torch.empty(self._c('weight_bytes')(self._h), dtype=torch.uint8, device=self.device)
            self._ws = torch.empty(256, dtype=torch.uint8, device=self.device)
            nd = self._c('derived_bytes')(self._h)
            if nd > 0:                                   # packs derived from parameters (the upsamplers' phase packs): filled by _set
                self._derived = torch.empty(nd, dtype=torch.uint8, device=self.device)
            self._bind()
            if init:
                self.init_random(seed)

    def _c(self, name):
        return getattr(self._lib, f"{self._prefix}_{name}")

    def _create_handle(self):
        """A new C handle for self.config (the subclass builds its config struct and calls its constructor)."""
        raise NotImplementedError

    def _init_state(self, src=None):
        """Subclass state beyond the table and the blobs; `src` is the engine a clone was made from."""

    def clone_shared(self):
        """A second engine over the SAME weight blob with its own workspace, so two evaluations (two views of a mesh) can be
        in flight on two HIP streams at once: the kernels of the deep UNet levels do not fill the chip, and two concurrent
        evaluations finish ~1.25x sooner than back to back (tools/bench_concurrent.py)."""
        o = type(self).__new__(type(self))
        o.config, o.device, o._lib = self.config, self.device, self._lib
        o._names, o._shapes, o._index = self._names, self._shapes, self._index
        o._h = self._create_handle()                    # same config, same C constructor
        o._weights = self._weights                      # shared, read-only during forward
        o._derived, o._derived_on = self._derived, self._derived_on     # derived from those weights: shared with them
        o._ws = torch.empty(256, dtype=torch.uint8, device=self.device)
        o._ws_key, o._t = None, None
        o._bind()
        o._init_state(self)
        return o

    def __del__(self):
        try:
            if getattr(self, '_h', None):
                self._c('destroy')(self._h)
                self._h = None
        except Exception:
            pass

    # -- parameter table ---------------------------------------------------------------------------------
    def param_shapes(self):
        return dict(zip(self._names, self._shapes))

    def num_parameters(self):
        return sum(math.prod(s) for s in self._shapes)

    def _bind(self):
        L.check(self._c('bind')(self._h, L.ptr(self._weights), L.ptr(self._ws), self._ws.numel()))
        if self._derived is not None:
            on = self._derived_on
            L.check(self._c('bind_derived')(self._h, L.ptr(self._derived) if on else None, self._derived.numel() if on else 0))

    def use_derived(self, on=True):
        """Bind (default) or unbind the derived blob.  Unbound, every layer runs from the weight blob alone (the upsamplers as
        nine-tap convolutions over the x2 grid); the blob keeps its contents, so binding it again needs no reload as long as no
        parameter was set in between."""
        self._derived_on = bool(on)
        self._ws_key = None                # the two forms split K differently: re-query the workspace
        self._bind()
        return self

    def _set(self, i, t):
        t = L.f32c(t, self.device)
        if tuple(t.shape) != self._shapes[i]:
            raise L.CtxError(f"{self._names[i]}: shape {tuple(t.shape)} != {self._shapes[i]}")
        L.check(self._c('set_param')(self._h, i, L.ptr(t, torch.float32, self._names[i]), L.stream()))

    def _load(self, sd):
        """Repack every table entry that `sd` holds (the subclass's load_state_dict decides what may be missing)."""
        for n, i in self._index.items():
            if n in sd:
                self._set(i, sd[n])
        torch.cuda.synchronize(self.device)   # sources must outlive the async repack kernels

    def load_file(self, path, strict=True):
        """Weights from a local safetensors file with diffusers' parameter names (what `from_pretrained` would have fetched by
        model name, src/stable_diffusion_depth.py:58-88); fp16 / bf16 / fp32 payloads are accepted and repacked to the engine's
        fp16 layout.  The file is memory-mapped: tensors go to the device one at a time."""
        from .safetensors_io import load_file
        return self.load_state_dict(load_file(path), strict=strict)

    @classmethod
    def from_file(cls, path, config=None, device="cuda:0", strict=True):
        net = cls(config, device=device, init=False)
        net.load_file(path, strict=strict)
        return net

    @staticmethod
    def _init_scale(u, fan):
        """u in U(-1, 1) -> U(-1/sqrt(fan), +).  Each engine keeps its own fp32 expression: the seeded weights are pinned bit for bit."""
        raise NotImplementedError

    def init_random(self, seed=0):
        """torch default initialisers (kaiming_uniform(a=sqrt 5) => U(-1/sqrt(fan_in), +)), norms = (1, 0)."""
        g = torch.Generator(device=self.device).manual_seed(seed)
        fan = {}
        for n, s in zip(self._names, self._shapes):
            if n.endswith('.weight') and len(s) >= 2:
                fan[n[:-7]] = math.prod(s[1:])
        for i, (n, s) in enumerate(zip(self._names, self._shapes)):
            base = n.rsplit('.', 1)[0]
            if len(s) == 1 and base not in fan:                 # norm affine
                t = torch.ones(s, device=self.device) if n.endswith('.weight') else torch.zeros(s, device=self.device)
            else:
                t = self._init_scale(torch.rand(s, generator=g, device=self.device) * 2 - 1, fan[base])
            self._set(i, t)
            if i % 64 == 63:
                torch.cuda.synchronize(self.device)
        torch.cuda.synchronize(self.device)

    # -- per-call plumbing -------------------------------------------------------------------------------
    def _reserve(self, need, what=None):
        """Grow the workspace to `need` bytes (a dry run's answer; negative = it refused the dimensions: raise `what`, or the
        library's own message)."""
        if need < 0:
            raise L.CtxError(what or self._lib.ctx_last_error().decode())
        if self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._bind()

    def _timestep(self, timestep):
        """The timestep as a one-element float32 device tensor: `timestep` itself if it is one, else the engine's own `_t`."""
        if isinstance(timestep, torch.Tensor) and timestep.is_cuda and timestep.dtype == torch.float32 and timestep.numel() == 1:
            return timestep.reshape(1)
        if self._t is None:
            self._t = torch.empty(1, dtype=torch.float32, device=self.device)
        self._t.fill_(float(timestep))
        return self._t
