#!/usr/bin/env python3
"""The ten conv2 shapes of the SD2-depth UNet (latent 96^2, CFG batch 2) that carry a shortcut: the shortcut folded into conv2's K
loop (ctx_conv3x3_seg_f16, the plan of the 3x3 part) against conv2 with a residual + a separate shortcut GEMM (each on its own plan).
Event-timed over ITERS launches after a warm-up.  Usage: bench_resnet_fold.py [ITERS]"""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from contexture_nerf_amd import _lib as L

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 200
lib = L.load(); dev = torch.device('cuda:0')
SHAPES = [(48, 640, (320,)), (24, 1280, (640,)), (12, 1280, (1280, 1280)), (24, 1280, (1280, 1280)), (24, 1280, (1280, 640)),
          (48, 640, (1280, 640)), (48, 640, (640, 640)), (48, 640, (640, 320)), (96, 320, (640, 320)), (96, 320, (320, 320))]


def timed(fn):
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


print(f"{'M':>6} {'cout':>5} {'segments':>12} {'folded us':>10} {'conv2+res us':>13} {'shortcut us':>12} {'separate us':>12} {'gain us':>8}")
B = 2
for hw, cout, segs in SHAPES:
    g = torch.Generator(device=dev).manual_seed(hw + cout)
    M, cin = B * hw * hw, sum(segs)
    x = torch.randn(B, hw, hw, cout, generator=g, device=dev).half()
    w = (torch.randn(cout, 9 * cout, generator=g, device=dev) / (9 * cout) ** 0.5).half()
    xs = [torch.randn(M, c, generator=g, device=dev).half() for c in segs]
    cat = torch.cat(xs, 1).contiguous()
    wsc = (torch.randn(cout, cin, generator=g, device=dev) / cin ** 0.5).half()
    b1, b2 = torch.randn(cout, generator=g, device=dev).half(), torch.randn(cout, generator=g, device=dev).half()
    y, sc = torch.empty(M, cout, dtype=torch.float16, device=dev), torch.empty(M, cout, dtype=torch.float16, device=dev)
    part = torch.empty(32 * M * cout, dtype=torch.float32, device=dev)
    two = len(segs) == 2
    wb = C.c_void_p(wsc.data_ptr() + 2 * segs[0]) if two else None
    s = L.stream()

    def folded():
        lib.ctx_conv3x3_seg_f16(L.ptr(x), L.ptr(w), L.ptr(b1), L.ptr(b2), None, None, B, hw, hw, cout, cout, L.ptr(xs[0]), L.ptr(wsc), segs[0], cin,
                                L.ptr(xs[1]) if two else None, wb, segs[1] if two else 0, cin, L.ptr(part), -1, L.ptr(y), s)
    tf = timed(folded)
    tc = lib.ctx_bench_gemm(L.ptr(x), L.ptr(w), L.ptr(b1), L.ptr(sc), M, cout, 9 * cout, L.ptr(y), B, hw, hw, cout, 0, 0, L.ptr(part), -1, iters, s) * 1e3
    tg = lib.ctx_bench_gemm(L.ptr(cat), L.ptr(wsc), L.ptr(b2), None, M, cout, cin, L.ptr(sc), 0, 0, 0, 0, 0, 0, L.ptr(part), -1, iters, s) * 1e3
    print(f"{M:6d} {cout:5d} {str(segs):>12} {tf:10.1f} {tc:13.1f} {tg:12.1f} {tc + tg:12.1f} {tc + tg - tf:8.1f}")
