"""GPU: every kernel form of the texture-field MLP (csrc/uvmlp.hip) that its host gate accepts, against the float64 oracle
(oracle/nerf.py), straight through the C ABI.  tests/test_field_envelope_cpu.py pins the gate itself; the shapes here are the ones
the callers can reach and no other test runs: the split-fp16 kernels away from input_ch = 42, the overlaid (EP = 64) forward with a 2-D
input and the side-by-side (EP = 48) one with a 3-D input, input_ch around the 48 / 49 switch and at 1 and 64, the skip layer as the last
hidden layer, D = 16 and D = 1, output_ch 1 and 2, the 8-wave weight gradient, and the refusals with live buffers.

Texel counts: 1 (one texel), 65 (a one-row tail behind a full 64-texel tile; one whole and one ragged weight-gradient range) and 193
(three tiles and a tail; four whole 48-texel ranges and a ragged one), 331 for D = 16.

Tolerances (none of them comes from what the device returns):
  gradients   max |err| <= rel * max |oracle| per tensor, rel = 3e-5 with the 48-wide embedding, 1e-4 with the 64-wide one: the figures of
              test_texture_field_backward_vs_oracle / test_field_3d_backward, which cover the same kernels.  The float32 numpy oracle
              against the float64 one with a shared ReLU pattern is 0.4 - 1.7e-6 by that measure, so both leave the reference >= 15x.
  ReLU        the pattern is the device's (saved activations > 0); it may differ from the oracle's only where |pre-activation| < 1e-5.
  raw         max |err| <= 1e-5 * max(1, max |oracle raw|), the float64 MLP being fed the device's own saved embedding.
  embedding   fused seams: the saved embedding against oracle.embed (float32, the same float32 argument x * 2^l).  numpy's float32
              sin / cos against float64 sin / cos of that argument measured 7.2e-8 at L = 15 and 7.1e-8 at L = 7 (200 000 points x 3);
              4 x the larger figure is allowed for another correctly rounded libm: EMB_TOL = 2.9e-7.
  atlas       (tanh + 1) / 2 of the device's own raw to 2e-7 absolute (one fp32 tanh)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from oracle import nerf as onerf

pytestmark = pytest.mark.gpu

GUARD = 1 << 20
EMB_TOL = 2.9e-7
NS = (1, 65, 193)


# ---- buffers with a guard nobody may write ---------------------------------------------------------------------------------------
class _Buf:
    """nbytes of payload (viewed as dtype) and, behind it, GUARD bytes of 0xA5"""

    def __init__(self, nbytes, dev, dtype=torch.float32, fill=None):
        self.nbytes = nbytes
        self.store = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.t = self.store[:nbytes].view(dtype)
        if fill is not None:
            self.t.fill_(fill)

    def intact(self):
        return bool((self.store[self.nbytes:] == 0xA5).all())


def _epad(input_ch):
    return 48 if input_ch <= 48 else 64


def _rel(input_ch):
    return 3e-5 if input_ch <= 48 else 1e-4


# ---- a network: nn.Linear's init from a seeded CPU generator, packed through the C ABI -----------------------------------------------
class _Net:
    def __init__(self, dev, D, W, input_ch, output_ch, skip, seed=0, gain=1.0):
        from contexture_nerf_amd import _lib as L
        lib = L.load()
        self.D, self.W, self.input_ch, self.output_ch, self.skip = D, W, input_ch, output_ch, skip
        self.has_skip = 0 <= skip <= D - 2
        self.skips = (skip,) if self.has_skip else ()
        torch.manual_seed(1000 * seed + 7 * D + W + input_ch)
        kin = [input_ch] + [W + (input_ch if self.has_skip and i == skip + 1 else 0) for i in range(1, D)]
        layers = [torch.nn.Linear(k, W) for k in kin] + [torch.nn.Linear(W, output_ch)]
        self.ws = [(l.weight.detach() * (gain if i < D else 1.0)).contiguous() for i, l in enumerate(layers)]
        self.bs = [l.bias.detach().clone() for l in layers]
        self.ws_np = [w.numpy() for w in self.ws]
        self.bs_np = [b.numpy() for b in self.bs]
        self.ws_d = [w.to(dev) for w in self.ws]
        self.bs_d = [b.to(dev) for b in self.bs]
        n = lib.ctx_uvmlp_packed_bytes(D, W, input_ch, output_ch, skip)
        assert n > 0
        self.blob = _Buf(n, dev, torch.uint8)
        wp = (C.c_void_p * (D + 1))(*[L.ptr(w).value for w in self.ws_d])
        bp = (C.c_void_p * (D + 1))(*[L.ptr(b).value for b in self.bs_d])
        L.check(lib.ctx_uvmlp_pack(wp, bp, D, W, input_ch, output_ch, skip, L.ptr(self.blob.t), L.stream()))
        torch.cuda.synchronize()
        assert self.blob.intact(), "ctx_uvmlp_pack wrote past ctx_uvmlp_packed_bytes"


def _device_linspace(res):
    """the grid mode's coordinates, in binary32 in the kernel's order: start + i*step for the first half, end - (res-1-i)*step after"""
    i = np.arange(res)
    step = np.float32(1.0) / np.float32(res - 1)
    lo = (i.astype(np.float32) * step).astype(np.float32)
    hi = (np.float32(1.0) - ((res - 1 - i).astype(np.float32) * step).astype(np.float32)).astype(np.float32)
    return np.where(i < res // 2, lo, hi).astype(np.float32)


def _grid_points(res):
    l = _device_linspace(res)
    u, v = np.meshgrid(l, l, indexing='xy')                 # node n = i*res + j: x0 = l[j], x1 = l[i]
    return np.stack([u, v], -1).reshape(-1, 2)


def _field_abi(net, seam, N, dev, x=None, emb=None, dims=2, L_=0, res=0, idx=None, c_raw=None, c_tex=None, backward=True,
               want_tex=True, tex_fill=7.0):
    """One training forward (+ backward) straight through the C ABI; every output buffer carries a 0xA5 guard behind it.
    seam: 'emb' (ctx_uvmlp_fwd_emb / _bwd_emb, with grad_emb), 'uv' (ctx_uvmlp_fwd_save from x [N,dims]), 'emb2d' (ctx_uvmlp_fwd_save(uv =
    NULL, emb) of the 2-D field), 'grid' (no inputs: the res x res atlas grid), 'list' (ctx_uvmlp_fwd_save_idx / _bwd_idx on idx).
    c_raw [N,C] / c_tex [C,plane] (host tensors): the upstream gradients.  Returns a dict of host arrays."""
    from contexture_nerf_amd import _lib as L
    lib = L.load()
    D, W, ic, oc, skip = net.D, net.W, net.input_ch, net.output_ch, net.skip
    EP = _epad(ic)
    raw = _Buf(N * oc * 4, dev)
    saved = _Buf(lib.ctx_uvmlp_saved_bytes(N, D, W, ic), dev)
    plane = res * res if seam == 'list' else N
    tex = _Buf(oc * plane * 4, dev, fill=tex_fill) if (want_tex and seam != 'emb') else None
    x_d = None if x is None else torch.as_tensor(x).contiguous().to(dev)
    e_d = None if emb is None else torch.as_tensor(emb).contiguous().to(dev)
    i_d = None if idx is None else torch.as_tensor(idx, dtype=torch.int32).contiguous().to(dev)
    pt = lambda b: None if b is None else L.ptr(b.t)
    if seam == 'emb':
        L.check(lib.ctx_uvmlp_fwd_emb(L.ptr(e_d), N, L.ptr(net.blob.t), D, W, ic, oc, skip, pt(raw), pt(saved), L.stream()))
    elif seam == 'list':
        L.check(lib.ctx_uvmlp_fwd_save_idx(L.ptr(i_d), N, res, L.ptr(net.blob.t), D, W, L_, oc, skip, pt(raw), pt(tex), pt(saved), L.stream()))
    else:
        assert ic == dims * (1 + 2 * L_)
        L.check(lib.ctx_uvmlp_fwd_save(L.ptr(x_d) if seam == 'uv' else None, L.ptr(e_d) if seam == 'emb2d' else None, N, res, L.ptr(net.blob.t),
                                       D, W, dims, L_, oc, skip, pt(raw), pt(tex), pt(saved), L.stream()))
    torch.cuda.synchronize()
    assert raw.intact(), "the forward wrote past raw [N, output_ch]"
    assert saved.intact(), "the forward wrote past ctx_uvmlp_saved_bytes"
    assert tex is None or tex.intact(), "the forward wrote past the atlas"
    assert net.blob.intact()
    sv = saved.t
    out = dict(raw=raw.t.reshape(N, oc).cpu().numpy(), emb=sv[:N * EP].reshape(N, EP).cpu().numpy(),
               acts=sv[N * EP:N * EP + D * N * W].reshape(D, N, W).cpu().numpy(),
               tex=None if tex is None else tex.t.reshape(oc, plane).cpu().numpy())
    if not backward:
        return out
    ws_bytes = lib.ctx_uvmlp_bwd_ws_bytes(N, D, W)
    ws = _Buf(ws_bytes, dev, torch.uint8)
    gws = [torch.full_like(w, float('nan')) for w in net.ws_d]
    gbs = [torch.full_like(b, float('nan')) for b in net.bs_d]
    gwp = (C.c_void_p * (D + 1))(*[L.ptr(t).value for t in gws])
    gbp = (C.c_void_p * (D + 1))(*[L.ptr(t).value for t in gbs])
    cr = None if c_raw is None else c_raw.contiguous().to(dev)
    ct = None if c_tex is None else c_tex.contiguous().to(dev)
    if seam == 'emb':
        ge = _Buf(N * ic * 4, dev)
        L.check(lib.ctx_uvmlp_bwd_emb(L.ptr(cr), N, L.ptr(net.blob.t), D, W, ic, oc, skip, pt(saved), pt(ws), gwp, gbp, pt(ge), L.stream()))
        torch.cuda.synchronize()
        assert ge.intact(), "the backward wrote past grad_emb [N, input_ch]"
        out['grad_emb'] = ge.t.reshape(N, ic).cpu().numpy()
        ge2 = _Buf(N * ic * 4, dev)                             # the input gradient alone: no weight-gradient launch, the same bits
        L.check(lib.ctx_uvmlp_bwd_emb(L.ptr(cr), N, L.ptr(net.blob.t), D, W, ic, oc, skip, pt(saved), pt(ws), None, None, pt(ge2), L.stream()))
        torch.cuda.synchronize()
        assert ge2.intact()
        out['grad_emb_alone'] = ge2.t.reshape(N, ic).cpu().numpy()
    elif seam == 'list':
        L.check(lib.ctx_uvmlp_bwd_idx(L.ptr(cr), L.ptr(ct), L.ptr(i_d), res, pt(raw), N, L.ptr(net.blob.t), D, W, L_, oc, skip, pt(saved), pt(ws),
                                      gwp, gbp, L.stream()))
    else:
        L.check(lib.ctx_uvmlp_bwd(L.ptr(cr), L.ptr(ct), pt(raw), N, L.ptr(net.blob.t), D, W, dims, L_, oc, skip, pt(saved), pt(ws), gwp, gbp,
                                  L.stream()))
    torch.cuda.synchronize()
    assert ws.intact(), "the backward wrote past ctx_uvmlp_bwd_ws_bytes"
    assert saved.intact() and raw.intact() and net.blob.intact()
    out['gws'] = [t.cpu().numpy() for t in gws]
    out['gbs'] = [t.cpu().numpy() for t in gbs]
    return out


def _close(a, b, rel, what):
    a = np.asarray(a, np.float64)
    err = np.abs(a - b).max()
    scale = np.abs(b).max()
    print(f"{what}: max abs err {err:.3e}, scale {scale:.3e}, ratio {err / (scale + 1e-300):.2e} (allowed {rel:.0e})")
    assert np.isfinite(a).all(), f"{what}: non-finite"
    assert err <= rel * scale, f"{what}: max abs err {err:.3e} vs scale {scale:.3e}"


def _check_embedding(net, out, e_ref, exact):
    """the saved embedding: columns [0, input_ch) against the reference rows (bit for bit where the kernel only copies them), zeros behind"""
    ic = net.input_ch
    got = out['emb']
    assert not got[:, ic:].any(), "padding columns of the saved embedding are not zero"
    if exact:
        assert np.array_equal(got[:, :ic], e_ref), "the saved embedding is not the rows it was given"
    else:
        d = np.abs(got[:, :ic].astype(np.float64) - e_ref.astype(np.float64)).max()
        print(f"embedding: max abs diff {d:.3e} (allowed {EMB_TOL:.1e})")
        assert d <= EMB_TOL, f"embedding: {d:.3e}"


def _check_forward(net, out, what):
    """raw and the saved activations against the float64 MLP on the device's own embedding; the atlas against the device's own raw"""
    e = out['emb'][:, :net.input_ch].astype(np.float64)
    D = net.D
    raw_o = onerf.nerf2d_forward(e, net.ws_np[:D], net.bs_np[:D], net.ws_np[D], net.bs_np[D], skips=net.skips, dtype=np.float64)
    err = np.abs(out['raw'] - raw_o).max()
    print(f"{what} raw: max abs err {err:.3e}, max |raw| {np.abs(raw_o).max():.3e}")
    assert np.isfinite(out['raw']).all()
    assert err <= 1e-5 * max(1.0, np.abs(raw_o).max()), f"{what} raw: {err:.3e}"
    if out['tex'] is not None and out['tex'].shape[1] == out['raw'].shape[0]:
        t_o = (np.tanh(out['raw'].astype(np.float64)) + 1) / 2
        t_err = np.abs(out['tex'].T - t_o).max()
        print(f"{what} atlas: max abs err {t_err:.3e}")
        assert t_err <= 2e-7, f"{what} atlas: {t_err:.3e}"
    return raw_o


def _check_backward(net, out, c_raw, c_tex_nc, what, rel=None):
    """gradients against the float64 oracle with the device's ReLU pattern (which may differ from the oracle's only at |pre| < 1e-5)"""
    D, ic = net.D, net.input_ch
    rel = _rel(ic) if rel is None else rel
    e = out['emb'][:, :ic].astype(np.float64)
    acts = out['acts']
    masks = [acts[i] > 0 for i in range(D)]
    gws, gbs, pre, ge = onerf.nerf2d_backward(e, net.ws_np[:D], net.bs_np[:D], net.ws_np[D], net.bs_np[D],
                                              grad_raw=None if c_raw is None else c_raw.numpy(),
                                              grad_tex=None if c_tex_nc is None else c_tex_nc.numpy(), skips=net.skips, masks=masks,
                                              return_pre=True, return_emb=True)
    n_flip = 0
    for i in range(D):
        assert np.abs(acts[i] - np.maximum(pre[i], 0)).max() <= 2e-5 * max(1.0, np.abs(pre[i]).max()), f'{what}: saved activations {i}'
        flipped = masks[i] != (pre[i] > 0)
        n_flip += int(flipped.sum())
        assert np.all(np.abs(pre[i][flipped]) < 1e-5), f'{what}: ReLU pattern of layer {i}'
    print(f"{what}: {n_flip} ReLU disagreements")
    for i in range(D + 1):
        _close(out['gws'][i], gws[i], rel, f'{what} gw{i}')
        _close(out['gbs'][i], gbs[i], rel, f'{what} gb{i}')
    if 'grad_emb' in out:
        _close(out['grad_emb'], ge, rel, f'{what} grad_emb')
        assert np.array_equal(out['grad_emb'], out['grad_emb_alone']), f'{what}: grad_emb alone has other bits'


def _grads(N, oc, plane=None, seed=0, tex=True):
    g = torch.Generator().manual_seed(100 + seed + N)
    c_raw = torch.randn(N, oc, generator=g)
    c_tex = torch.randn(oc, plane or N, generator=g) if tex else None
    return c_raw, c_tex


def _exact_f32(on):
    """context: CTX_UVMLP_EXACT_F32=1 while inside (the library reads it on every call)"""
    class _Ctx:
        def __enter__(self):
            if on:
                os.environ["CTX_UVMLP_EXACT_F32"] = "1"

        def __exit__(self, *a):
            if on:
                os.environ.pop("CTX_UVMLP_EXACT_F32", None)
    return _Ctx()


def _with_n(cases):
    return [c + (N,) for c in cases for N in (NS + ((331,) if c[0] == 16 else ()))]


# ---- the `emb` seam: any width in [1, 64], with the gradient to the embedding -----------------------------------------------------------
# At D = 16 nn.Linear's init (uniform, variance 1 / (3 fan_in)) lets the signal die out: the hidden weights are scaled by sqrt(2), and, since
# on the CPU that still leaves (16, 256, 42) with max |raw| 0.019 and a spread of 9e-4 across the points (bias-driven; an absolute tolerance
# would hide a wrong layer), once more by sqrt(6), the gain that keeps the second moment through a ReLU layer (max |raw| 1.2, spread 0.16).
EMB_CASES = [(2, 256, 1, 1, 0, 1.0), (3, 128, 47, 2, 1, 1.0), (3, 128, 48, 2, 1, 1.0), (3, 128, 49, 3, 1, 1.0), (5, 256, 64, 4, 3, 1.0),
             (16, 64, 63, 4, 14, math.sqrt(2.0)), (16, 256, 42, 3, 7, math.sqrt(2.0)), (16, 64, 63, 4, 14, math.sqrt(6.0)),
             (16, 256, 42, 3, 7, math.sqrt(6.0)), (4, 64, 33, 1, 2, 1.0)]


@pytest.mark.parametrize("D,W,ic,oc,skip,gain,N", _with_n(EMB_CASES))
def test_emb_seam_vs_oracle(dev, D, W, ic, oc, skip, gain, N):
    net = _Net(dev, D, W, ic, oc, skip, gain=gain)
    g = torch.Generator().manual_seed(N + ic)
    emb = torch.rand(N, ic, generator=g) * 2 - 1
    c_raw, _ = _grads(N, oc, tex=False)
    out = _field_abi(net, 'emb', N, dev, emb=emb, c_raw=c_raw)
    what = f"emb D={D} W={W} in={ic} out={oc} skip={skip} N={N}"
    _check_embedding(net, out, emb.numpy(), exact=True)
    raw_o = _check_forward(net, out, what)
    if gain > 2.0 and N >= 65:
        assert np.abs(raw_o).max() > 0.1, "the signal vanished: an absolute tolerance would hide a wrong layer"
    _check_backward(net, out, c_raw, None, what)


# ---- the fused seams: embedding computed in the kernel from uv (2-D) / xyz (3-D) ---------------------------------------------------------
# (D, W, L, output_ch, skip): W = 256 with L <= 11 is the split-fp16 pair (and, under CTX_UVMLP_EXACT_F32=1, the side-by-side f32 kernels);
# L >= 12 the overlaid f32 forward with a 2-D input
FUSED_2D_SPLIT = [(2, 256, 0, 1, 0), (3, 256, 4, 2, 1), (8, 256, 11, 3, 0)]
FUSED_2D_F32 = [(3, 256, 12, 4, 0), (8, 256, 15, 1, 6), (2, 64, 4, 3, 0), (8, 64, 12, 2, 6), (3, 128, 4, 4, 1), (8, 128, 12, 1, 0)]
FUSED_3D = [(2, 64, 0, 4, 0), (3, 64, 4, 2, 1), (8, 64, 7, 4, 6), (8, 256, 0, 4, 4), (2, 256, 4, 3, 0), (3, 256, 7, 4, 1), (3, 128, 8, 4, 0)]


def _fused_case(dev, dims, D, W, L_, oc, skip, N, exact):
    ic = dims * (1 + 2 * L_)
    net = _Net(dev, D, W, ic, oc, skip)
    g = torch.Generator().manual_seed(N + L_)
    x = torch.rand(N, dims, generator=g)
    if dims == 3:
        x = x * 2 - 1
    c_raw, c_tex = _grads(N, oc)
    with _exact_f32(exact):
        out = _field_abi(net, 'uv', N, dev, x=x, dims=dims, L_=L_, c_raw=c_raw, c_tex=c_tex)
    what = f"fused dims={dims} D={D} W={W} L={L_} out={oc} skip={skip} N={N}{' exact-f32' if exact else ''}"
    e_ref = onerf.embed(x.numpy(), multires=L_)
    assert e_ref.shape[1] == ic
    _check_embedding(net, out, e_ref, exact=False)
    _check_forward(net, out, what)
    _check_backward(net, out, c_raw, c_tex.T, what)
    return out


@pytest.mark.parametrize("exact", [False, True], ids=["split16", "exact_f32"])
@pytest.mark.parametrize("D,W,L_,oc,skip,N", _with_n(FUSED_2D_SPLIT))
def test_fused_2d_split_fp16_shapes_vs_oracle(dev, D, W, L_, oc, skip, N, exact):
    _fused_case(dev, 2, D, W, L_, oc, skip, N, exact)


@pytest.mark.parametrize("D,W,L_,oc,skip,N", _with_n(FUSED_2D_F32))
def test_fused_2d_f32_shapes_vs_oracle(dev, D, W, L_, oc, skip, N):
    _fused_case(dev, 2, D, W, L_, oc, skip, N, False)


@pytest.mark.parametrize("D,W,L_,oc,skip,N", _with_n(FUSED_3D))
def test_fused_3d_vs_oracle(dev, D, W, L_, oc, skip, N):
    _fused_case(dev, 3, D, W, L_, oc, skip, N, False)


@pytest.mark.parametrize("N", NS)
def test_emb_rows_given_to_the_2d_entries(dev, N):
    """ctx_uvmlp_fwd_save(uv = NULL, emb) at W = 256, L = 4: the split-fp16 kernels load the rows instead of computing them.  The saved
    embedding is the rows as two fp16 numbers (hi + lo 2^-11: 22 bits, and 2^-24 / 2^11 absolute where lo is a subnormal): 2^-21 relative
    + 2^-34 absolute is allowed there; the oracle tolerances hold."""
    D, W, L_, oc, skip = 8, 256, 4, 3, 4
    net = _Net(dev, D, W, 18, oc, skip)
    g = torch.Generator().manual_seed(N)
    uv = torch.rand(N, 2, generator=g)
    emb = torch.tensor(onerf.embed(uv.numpy(), multires=L_))
    c_raw, c_tex = _grads(N, oc)
    out = _field_abi(net, 'emb2d', N, dev, emb=emb, dims=2, L_=L_, c_raw=c_raw, c_tex=c_tex)
    got = out['emb']
    assert not got[:, 18:].any()
    assert np.all(np.abs(got[:, :18].astype(np.float64) - emb.numpy()) <= 2.0 ** -21 * np.abs(emb.numpy()) + 2.0 ** -34)
    what = f"emb rows to the 2-D entry N={N}"
    _check_forward(net, out, what)
    _check_backward(net, out, c_raw, c_tex.T, what)


# ---- the list entries against the dense grid run -------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,W,L_", [(3, 128, 4), (2, 256, 11)])
def test_list_entries_rows_of_the_dense_run(dev, D, W, L_):
    res, n, oc, skip = 9, 40, 3, D - 2
    ic = 2 * (1 + 2 * L_)
    net = _Net(dev, D, W, ic, oc, skip)
    idx = torch.randperm(res * res, generator=torch.Generator().manual_seed(5))[:n].to(torch.int32)
    li = idx.long().numpy()
    dense = _field_abi(net, 'grid', res * res, dev, res=res, dims=2, L_=L_, backward=False)
    e_ref = onerf.embed(_grid_points(res), multires=L_)
    _check_embedding(net, dense, e_ref, exact=False)
    _check_forward(net, dense, f"grid D={D} W={W} L={L_}")
    c_raw, c_tex = _grads(n, oc, plane=res * res)
    off = np.ones(res * res, bool); off[li] = False
    c_tex[:, torch.tensor(off)] = float('nan')                 # grad_tex is read at the listed texels only
    out = _field_abi(net, 'list', n, dev, res=res, idx=idx, L_=L_, c_raw=c_raw, c_tex=c_tex, tex_fill=7.0)
    assert np.array_equal(out['raw'], dense['raw'][li]), "row n of the list run is not row idx[n] of the dense run"
    assert np.array_equal(out['emb'], dense['emb'][li]) and np.array_equal(out['acts'], dense['acts'][:, li])
    assert np.array_equal(out['tex'][:, li], dense['tex'][:, li]), "listed atlas texels differ from the dense run's"
    assert np.all(out['tex'][:, off] == 7.0), "an atlas texel off the list lost its fill"
    _check_backward(net, out, c_raw, c_tex[:, idx.long()].T, f"list D={D} W={W} L={L_}")


# ---- forward only: D = 1, and a skip outside [0, D-2], which means no skip layer ---------------------------------------------------------
@pytest.mark.parametrize("D,skip", [(1, 0), (1, -1), (3, -1), (3, 2)])
@pytest.mark.parametrize("W", [64, 256])
@pytest.mark.parametrize("N", NS)
def test_forward_without_a_skip_layer(dev, D, skip, W, N):
    L_, oc = 4, 3
    g = torch.Generator().manual_seed(N)
    uv = torch.rand(N, 2, generator=g)
    net = _Net(dev, D, W, 18, oc, skip)
    assert net.skips == ()
    out = _field_abi(net, 'uv', N, dev, x=uv, dims=2, L_=L_, backward=False)
    _check_embedding(net, out, onerf.embed(uv.numpy(), multires=L_), exact=False)
    _check_forward(net, out, f"uv seam D={D} skip={skip} W={W} N={N}")
    net = _Net(dev, D, W, 33, oc, skip)
    emb = torch.rand(N, 33, generator=g) * 2 - 1
    out = _field_abi(net, 'emb', N, dev, emb=emb, backward=False)
    _check_embedding(net, out, emb.numpy(), exact=True)
    _check_forward(net, out, f"emb seam D={D} skip={skip} W={W} N={N}")


# ---- the 8-wave weight-gradient form ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [193, 64 * 5 + 7])
def test_wg8_weight_gradient_vs_oracle(dev, N):
    """CTX_UVM_WG8=1 (read on every call): the 2 x 4-wave form of the 256 x 256 weight-gradient GEMM, same oracle and tolerance as the
    default 2 x 2 form.  Both forms walk the texels of a range in the same order into one accumulator per element, but nothing in
    the code promises the same bits, so equality is reported, not asserted."""
    D, W, L_, oc, skip = 8, 256, 10, 3, 4
    net = _Net(dev, D, W, 42, oc, skip)
    g = torch.Generator().manual_seed(N)
    uv = torch.rand(N, 2, generator=g)
    c_raw, c_tex = _grads(N, oc)
    outs = []
    for wg8 in (False, True):
        if wg8:
            os.environ["CTX_UVM_WG8"] = "1"
        try:
            out = _field_abi(net, 'uv', N, dev, x=uv, dims=2, L_=L_, c_raw=c_raw, c_tex=c_tex)
        finally:
            os.environ.pop("CTX_UVM_WG8", None)
        _check_forward(net, out, f"wg8={wg8} N={N}")
        _check_backward(net, out, c_raw, c_tex.T, f"wg8={wg8} N={N}")
        outs.append(out)
    same = all(np.array_equal(a, b) for a, b in zip(outs[0]['gws'] + outs[0]['gbs'], outs[1]['gws'] + outs[1]['gbs']))
    print(f"CTX_UVM_WG8=1 gives the default form's bits at N={N}: {same}")


# ---- refusals with live buffers: nothing is launched, nothing is written -----------------------------------------------------------------
def test_refusals_leave_every_buffer_alone(dev):
    from contexture_nerf_amd import _lib as L
    lib = L.load()
    N, res = 64, 8
    big = lambda mib: torch.full((mib << 20,), 0xA5, dtype=torch.uint8, device=dev)
    # every buffer is larger than any shape named below would need, whatever the entry did with it
    blob, raw, tex, saved, ws, ge = big(64), big(1), big(1), big(16), big(128), big(1)
    gw, gb = big(4), big(1)
    src = torch.full((1 << 20,), 0.01, device=dev)                       # inputs: weights, points, embedding rows, gradients
    idx = torch.arange(N, dtype=torch.int32, device=dev)
    outputs = dict(blob=blob, raw=raw, tex=tex, saved=saved, ws=ws, grad_emb=ge, gw=gw, gb=gb)
    p = lambda t: L.ptr(t)
    arr = lambda t: (C.c_void_p * 18)(*[p(t).value] * 18)
    s = L.stream()

    def entries(D, W, dims, L_, ic, oc, skip):
        """every launch-capable entry at one shape -> {name: rc}"""
        rcs = {}
        if ic == dims * (1 + 2 * L_) or ic > 64:
            rcs['pack'] = lib.ctx_uvmlp_pack(arr(src), arr(src), D, W, ic, oc, skip, p(blob), s)
        if dims == 2:
            rcs['fwd'] = lib.ctx_uvmlp_fwd(p(src), None, N, 0, p(blob), D, W, L_, oc, skip, p(raw), p(tex), s)
            rcs['fwd_save_idx'] = lib.ctx_uvmlp_fwd_save_idx(p(idx), N, res, p(blob), D, W, L_, oc, skip, p(raw), p(tex), p(saved), s)
            rcs['bwd_idx'] = lib.ctx_uvmlp_bwd_idx(p(src), p(src), p(idx), res, p(src), N, p(blob), D, W, L_, oc, skip, p(saved), p(ws), arr(gw), arr(gb), s)
        rcs['fwd_save'] = lib.ctx_uvmlp_fwd_save(p(src), None, N, 0, p(blob), D, W, dims, L_, oc, skip, p(raw), p(tex), p(saved), s)
        rcs['bwd'] = lib.ctx_uvmlp_bwd(p(src), p(src), p(src), N, p(blob), D, W, dims, L_, oc, skip, p(saved), p(ws), arr(gw), arr(gb), s)
        rcs['fwd_emb'] = lib.ctx_uvmlp_fwd_emb(p(src), N, p(blob), D, W, ic, oc, skip, p(raw), p(saved), s)
        rcs['bwd_emb'] = lib.ctx_uvmlp_bwd_emb(p(src), N, p(blob), D, W, ic, oc, skip, p(saved), p(ws), arr(gw), arr(gb), p(ge), s)
        return rcs

    # (D, W, dims, L, input_ch of the entries that take a width, output_ch, skip)
    bad = [(8, 192, 2, 10, 42, 3, 4), (8, 320, 2, 10, 42, 3, 4), (8, 192, 3, 10, 63, 4, 4), (17, 64, 2, 10, 42, 3, 4),
           (8, 64, 2, 16, 65, 3, 4), (8, 64, 3, 11, 65, 4, 4),            # input_ch 65 on the width entries, 66 / 69 from (dims, L)
           (8, 64, 2, 10, 42, 5, 4)]
    for shape in bad:
        for name, rc in entries(*shape).items():
            assert rc != 0, f"ctx_uvmlp_{name} accepted D, W, dims, L, input_ch, output_ch, skip = {shape}"
    assert b"unsupported" in lib.ctx_last_error() or b"outside" in lib.ctx_last_error()
    # a backward without a skip layer: skip outside [0, D-2]
    for skip in (-1, 7):
        rcs = entries(8, 64, 2, 10, 42, 3, skip)
        for name in ('bwd', 'bwd_idx', 'bwd_emb'):
            assert rcs[name] != 0, f"ctx_uvmlp_{name} accepted skip={skip} at D=8"
            del rcs[name]
        assert all(rc == 0 for rc in rcs.values()), rcs                 # ... which pack and the forwards take as "no skip layer"
    torch.cuda.synchronize()
    # the accepted calls of the last loop wrote blob / raw / tex / saved; refill, then every refused shape once more
    for t in (blob, raw, tex, saved):
        t.fill_(0xA5)
    for shape in bad:
        entries(*shape)
    for skip in (-1, 7):
        lib.ctx_uvmlp_bwd(p(src), p(src), p(src), N, p(blob), 8, 64, 2, 10, 3, skip, p(saved), p(ws), arr(gw), arr(gb), s)
        lib.ctx_uvmlp_bwd_idx(p(src), p(src), p(idx), res, p(src), N, p(blob), 8, 64, 10, 3, skip, p(saved), p(ws), arr(gw), arr(gb), s)
        lib.ctx_uvmlp_bwd_emb(p(src), N, p(blob), 8, 64, 42, 3, skip, p(saved), p(ws), arr(gw), arr(gb), p(ge), s)
    torch.cuda.synchronize()
    for name, t in outputs.items():
        assert bool((t == 0xA5).all()), f"a refused call wrote to {name}"


def test_nerf2d_width_192_raises(dev):
    from contexture_nerf_amd import _lib as L, run_nerf_helpers as rnh
    net = rnh.NeRF2D(D=8, W=192, input_ch=42, output_ch=3, skips=[4]).to(dev)
    with pytest.raises(L.CtxError, match="envelope"):
        net.packed()
