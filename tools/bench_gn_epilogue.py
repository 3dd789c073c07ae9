#!/usr/bin/env python3
"""The convolutions of the SD2-depth UNet (latent 96^2, CFG batch 2) whose output a GroupNorm reads next, each on the engine's plan:
  two-pass GroupNorm (96^2, 48^2): conv + k_gn_stats + k_gn_apply against conv with the partials request + k_gn_apply;
  one-kernel GroupNorm behind a split-K conv1 (24^2, 12^2): conv + reduce + k_gn_fused against conv + k_gn_fused on the slabs.
Event-timed over ITERS pairs after a warm-up.  (The proj_out GEMM 18432 x 320 x 320, two more producers per forward on the same
144 x 160 kernel, has no entry point that takes a request and is not timed here.)  Usage: bench_gn_epilogue.py [ITERS]"""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from contexture_nerf_amd import _lib as L

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 200
lib = L.load(); dev = torch.device('cuda:0')
# (latent side, Cin, Cout)
SHAPES = [(96, 320, 320), (96, 640, 320), (96, 960, 320), (48, 320, 640), (48, 640, 640), (48, 960, 640), (48, 1280, 640), (48, 1920, 640),
          (24, 640, 1280), (24, 1280, 1280), (24, 1920, 1280), (24, 2560, 1280), (12, 1280, 1280), (12, 2560, 1280)]
B, G = 2, 32


def timed(fn):
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


print(f"{'M':>6} {'Cin':>5} {'Cout':>5} {'form':>9} {'slots':>6} {'separate us':>12} {'fused us':>9} {'gain us':>8}")
for hw, cin, cout in SHAPES:
    g = torch.Generator(device=dev).manual_seed(hw + cin + cout)
    M = B * hw * hw
    x = torch.randn(B, hw, hw, cin, generator=g, device=dev).half()
    w = (torch.randn(cout, 9 * cin, generator=g, device=dev) / (9 * cin) ** 0.5).half()
    bias, rowb = torch.randn(cout, generator=g, device=dev).half(), torch.randn(B, cout, generator=g, device=dev).half()
    ga, be = torch.randn(cout, generator=g, device=dev).half(), torch.randn(cout, generator=g, device=dev).half()
    y, o = torch.empty(M, cout, dtype=torch.float16, device=dev), torch.empty(M, cout, dtype=torch.float16, device=dev)
    part = torch.empty(32 * M * cout, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.ctx_groupnorm_ws_bytes(B, G), dtype=torch.uint8, device=dev)
    s = L.stream()
    slots = C.c_int32(0)
    one_kernel = (cout // G) % 8 == 0 and hw * hw <= 12 * (512 // (cout // G // 8))

    def conv(req=False, keep=False):
        L.check(lib.ctx_conv3x3_gn_f16(L.ptr(x), L.ptr(w), L.ptr(bias), None, L.ptr(rowb), None, B, hw, hw, cin, cout, L.ptr(part), -1, 1 if keep else 0,
                                       G, L.ptr(ws) if req else None, C.byref(slots), L.ptr(y), s))

    def gn():
        L.check(lib.ctx_groupnorm_f16(L.ptr(y), L.ptr(ga), L.ptr(be), B, hw * hw, cout, G, 1e-5, 1, L.ptr(o), L.ptr(ws), s))

    def separate():
        conv(); gn()
    if one_kernel:
        # split factor of the plan: the kept-slabs call fails when the plan does not split
        try:
            conv(keep=True)
        except L.CtxError:
            print(f"{M:6d} {cin:5d} {cout:5d} {'slabs':>9} {'-':>6}   (the plan does not split K: nothing to fuse)")
            continue
        S = slots.value

        def fused_slabs():
            conv(keep=True)
            L.check(lib.ctx_groupnorm_slabs_f16(L.ptr(part), S, L.ptr(bias), None, L.ptr(rowb), cout, L.ptr(ga), L.ptr(be), B, hw * hw, cout, G, 1e-5, 1,
                                                L.ptr(o), s))
        ts, tf = timed(separate), timed(fused_slabs)
        print(f"{M:6d} {cin:5d} {cout:5d} {'slabs':>9} {S:6d} {ts:12.1f} {tf:9.1f} {ts - tf:8.1f}")
        continue
    conv(req=True)
    if not slots.value:
        print(f"{M:6d} {cin:5d} {cout:5d} {'partials':>9} {0:6d}   (declined: the plan's tile cannot serve the request)")
        continue
    ns = slots.value

    def fused():
        conv(req=True)
        L.check(lib.ctx_groupnorm_apply_f16(L.ptr(y), L.ptr(ws), ns, L.ptr(ga), L.ptr(be), B, hw * hw, cout, G, 1e-5, 1, L.ptr(o), s))
    ts, tf = timed(separate), timed(fused)
    print(f"{M:6d} {cin:5d} {cout:5d} {'partials':>9} {ns:6d} {ts:12.1f} {tf:9.1f} {ts - tf:8.1f}")
