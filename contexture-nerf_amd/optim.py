"""FieldAdam: Adam for the fields' parameters on the HIP path (csrc/adam.hip; the rule: tests/adam_rule.py).
One `ctx_adam_multi` launch steps up to 16 tensors of a group; a hash table listed in `encodings=` is stepped by `ctx_table_adam` straight
from the 64-bit integer sums its backward leaves on the device, so no float gradient of the table is allocated, written or read, and
with sparse=True (instant-ngp's rule) an entry whose gradient is exactly zero keeps its value and its moments."""
import ctypes as C
import math
import torch
from . import _lib as L

MAX_TENSORS = 16
_REFUSED = ("weight_decay", "amsgrad", "maximize")


def coefficients(lr, betas, eps, t):
    """The seven floats of the rule, from float64: (b1, b2, 1 - b1, 1 - b2, lr / (1 - b1^t), 1 / sqrt(1 - b2^t), eps); ctypes rounds each to
    binary32 (to nearest) when it is passed."""
    b1, b2 = float(betas[0]), float(betas[1])
    return b1, b2, 1.0 - b1, 1.0 - b2, float(lr) / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t), float(eps)


def adam_multi(params, exp_avgs, exp_avg_sqs, grads, lr, betas, eps, t, sparse=False):
    """One `ctx_adam_multi` launch: step t >= 1 on up to 16 contiguous float32 device tensors, in place."""
    n = len(params)
    arr = C.c_void_p * max(n, 1)
    lists = []
    for name, ts in (("param", params), ("exp_avg", exp_avgs), ("exp_avg_sq", exp_avg_sqs), ("grad", grads)):
        if len(ts) != n:
            raise L.CtxError(f"adam_multi: {len(ts)} {name} tensors for {n} parameters")
        lists.append(arr(*[L.ptr(x, torch.float32, name).value for x in ts]))
    for p, a, b, g in zip(params, exp_avgs, exp_avg_sqs, grads):
        if not (a.numel() == b.numel() == g.numel() == p.numel()):
            raise L.CtxError(f"adam_multi: a parameter of {p.numel()} elements with state or gradient of another size")
    counts = (C.c_int64 * max(n, 1))(*[p.numel() for p in params])
    L.check(L.load().ctx_adam_multi(lists[0], lists[1], lists[2], lists[3], counts, n, *coefficients(lr, betas, eps, t), int(bool(sparse)),
                                    L.stream()))


class FieldAdam(torch.optim.Optimizer):
    """Adam (no weight decay, no amsgrad, no maximize) whose step is hand-written HIP.  lr, betas, eps and sparse may be set per group.
    sparse=True: an element whose gradient is exactly zero (either sign) keeps p, exp_avg and exp_avg_sq while the step count advances.
    State per parameter: step (a float32 CPU scalar, as torch.optim.Adam keeps it), exp_avg, exp_avg_sq: state_dict() loads into
    torch.optim.Adam with the same groups, and back.  Parameters are float32, contiguous and on the device; a sparse .grad is refused.
    encodings: HashGridEncoding / HashGridEncoding2D modules whose `table` is in a group.  Until release() their backward leaves the
    table's gradient as the integer sums on the device and returns no .grad; step() reads the sums (`ctx_table_adam`).  A second backward
    of one encoding before the step (train_step's resample) turns the sums into a float .grad first, with the bits autograd accumulates
    without deferral.  Call release() when training ends (fit_views and the trainer do, in a finally)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, sparse=False, encodings=()):
        defaults = dict(lr=lr, betas=betas, eps=eps, sparse=bool(sparse), weight_decay=0, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults)
        self._deferred = []
        try:
            self._check_groups()
            for group in self.param_groups:
                for p in group['params']:
                    self._check_param(p)
            self._defer(list(encodings))
        except Exception:
            self.release()
            raise

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:                 # groups that come from torch.optim.Adam have no `sparse`
            group.setdefault('sparse', False)
        if not hasattr(self, '_deferred'):
            self._deferred = []

    def _check_groups(self):
        for i, group in enumerate(self.param_groups):
            for key in _REFUSED:
                if group.get(key):                          # weight_decay != 0, amsgrad=True, maximize=True
                    raise L.CtxError(f"FieldAdam: group {i}: {key}={group[key]!r} is not supported (the HIP step has no {key})")
            for key in ("capturable", "differentiable"):
                if group.get(key, False):
                    raise L.CtxError(f"FieldAdam: group {i}: {key}=True is not supported")
            if not group['lr'] >= 0.0 or isinstance(group['lr'], torch.Tensor):
                raise L.CtxError(f"FieldAdam: group {i}: lr={group['lr']!r}: want a number >= 0")
            if not group['eps'] >= 0.0:
                raise L.CtxError(f"FieldAdam: group {i}: eps={group['eps']!r}: want a number >= 0")
            b1, b2 = group['betas']
            if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
                raise L.CtxError(f"FieldAdam: group {i}: betas={group['betas']!r}: want both in [0, 1)")

    @staticmethod
    def _check_param(p):
        if not p.is_cuda:
            raise L.CtxError(f"FieldAdam: a parameter on {p.device} (the HIP path has no CPU fallback: want a device tensor)")
        if p.dtype != torch.float32:
            raise L.CtxError(f"FieldAdam: a parameter of dtype {p.dtype}: want float32")
        if not p.is_contiguous():
            raise L.CtxError("FieldAdam: a parameter that is not contiguous")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if hasattr(self, '_deferred'):                  # during __init__ the checks run once, after every group is in
            self._check_groups()
            for p in self.param_groups[-1]['params']:
                self._check_param(p)

    # ---- deferred table gradient ----
    def _defer(self, encodings):
        if not encodings:
            return
        if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            raise L.CtxError("FieldAdam: encodings= keeps the table's gradient off .grad, where no all-reduce sees it: one rank only")
        mine = {id(p) for group in self.param_groups for p in group['params']}
        for enc in encodings:
            if not hasattr(enc, '_defer_begin') or not hasattr(enc, 'table'):
                raise L.CtxError(f"FieldAdam: encodings= wants HashGridEncoding / HashGridEncoding2D modules, got {type(enc).__name__}")
            if id(enc.table) not in mine:
                raise L.CtxError("FieldAdam: an encoding listed in encodings= whose table is in no parameter group")
            if any(e is enc for e in self._deferred):
                raise L.CtxError("FieldAdam: an encoding listed twice in encodings=")
            enc._defer_begin()
            self._deferred.append(enc)

    def release(self):
        """Ends deferred mode: the listed encodings hand their table's gradient to autograd again.  Sums that no step consumed are turned
        into the table's .grad first, so nothing is lost."""
        for enc in getattr(self, '_deferred', []):
            if enc._pending is not None:
                self._add_grad(enc.table, enc._defer_flush())
            enc._defer_end()
        self._deferred = []

    @staticmethod
    def _add_grad(p, g):
        if p.grad is None:
            p.grad = g
        else:
            p.grad.add_(g)

    def zero_grad(self, set_to_none=True):
        super().zero_grad(set_to_none=set_to_none)
        for enc in self._deferred:
            enc._defer_drop()

    # ---- the step ----
    def _state(self, p):
        state = self.state[p]
        if len(state) == 0:
            state['step'] = torch.tensor(0.0, dtype=torch.float32)
            state['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return state

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_groups()
        tables = {id(enc.table): enc for enc in self._deferred}
        lib = L.load()
        for group in self.param_groups:
            lr, betas, eps, sparse = group['lr'], group['betas'], group['eps'], group['sparse']
            buckets = {}                                    # step count -> tensors: one launch shares c1 and c2
            for p in group['params']:
                enc = tables.get(id(p))
                if enc is not None and enc._pending is not None:
                    if p.grad is None:
                        self._check_param(p)
                        state = self._state(p)
                        state['step'] += 1
                        ws, n = enc._bwd_ws, enc._pending[-1]
                        L.check(lib.ctx_table_adam(L.ptr(p, torch.float32, "table"), L.ptr(state['exp_avg'], torch.float32, "exp_avg"),
                                                   L.ptr(state['exp_avg_sq'], torch.float32, "exp_avg_sq"), p.numel(), L.ptr(ws), n,
                                                   enc._corners, *coefficients(lr, betas, eps, int(state['step'])), int(bool(sparse)),
                                                   L.stream()))
                        enc._defer_consumed()
                        torch.autograd.graph.increment_version(p)
                        continue
                    p.grad.add_(enc._defer_flush())         # a .grad from before and sums from now: one float gradient
                if enc is not None:
                    enc._defer_stepped()
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise L.CtxError("FieldAdam: a sparse .grad is not supported (sparse=True skips exact zeros of a dense gradient)")
                self._check_param(p)
                state = self._state(p)
                state['step'] += 1
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                buckets.setdefault(int(state['step']), []).append((p, state['exp_avg'], state['exp_avg_sq'], g))
            for t, items in buckets.items():
                for i in range(0, len(items), MAX_TENSORS):
                    part = items[i:i + MAX_TENSORS]
                    adam_multi([x[0] for x in part], [x[1] for x in part], [x[2] for x in part], [x[3] for x in part], lr, betas, eps, t, sparse)
                for x in items:
                    # the kernels write through raw pointers: the caches keyed on p._version (NeRF2D's packed weights, texture_map) must see it
                    torch.autograd.graph.increment_version(x[0])
        return loss
