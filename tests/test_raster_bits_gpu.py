"""GPU: the bits of the raster-side and atlas-side kernels (texture mapping forward, backward and packed, the active-texel mark, the
scatter plan with the binned and the fixed-point scatters, the two ordered compactions, view weights, the unfused positional encoding,
camera rays) against digests recorded from the parent commit's build, so that a refactor of these kernels is held to "no result bit
changes" by something other than the code under test.  Built like tests/test_ray_bits_gpu.py.

tests/golden/raster_atlas_bits.json holds, per case, a SHA-256 over the raw bytes of its inputs and one over the raw bytes of each group
of outputs, the `hipcc --version` line of the recording and the commit whose `csrc/` was built for it.  Every output buffer carries GUARD
bytes of 0xA5 behind it and the guard is part of the digest; of a workspace only the guard is digested.  A changed input digest means
an input maker changed, not a kernel.  A compiler change that moves the output digests re-records them from the then-parent commit's
build:

    python tests/test_raster_bits_gpu.py --write [--lib PATH] [--commit HASH]     # PATH: that build's libctxnerf.so (default: the tree's own)

Order-free by construction: the float-atomics backward gets uv for which no two pixels share a texel (asserted on the host with the numpy
tap rule before the launch), the binned and fixed-point scatters sum integers, everything else has one writer per element.  Of the
scatter plan, whose tile lists are filled in arrival order, the header and the guard are digested; the lists show in the scatters' sums.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import test_field_texels_cpu as FT

f32 = np.float32
FIXTURE = os.path.join(ROOT, "tests", "golden", "raster_atlas_bits.json")
GUARD = 1 << 16
B, HW = 2, 257
TS = (2, 64, 100)
COMPACT_N = (1, 63, 64, 65, 1023, 1024, 1025, 1024 * 1024 + 1, 3 * 1024 * 1024 + 517)
BHW = {1: (1, 1, 1), 63: (1, 7, 9), 64: (2, 4, 8), 65: (1, 5, 13), 1023: (3, 11, 31), 1024: (2, 16, 32), 1025: (1, 25, 41),
       1024 * 1024 + 1: (1, 17, 61681), 3 * 1024 * 1024 + 517: (1, 5, 629249)}
MASKS = ("none", "all", "half", "last")


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is None:
            h.update(b"none;")
            continue
        a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a))
        h.update(f"{a.dtype.str}{a.shape};".encode())
        h.update(a.tobytes())
    return h.hexdigest()


class _Buf:
    """nbytes of payload (viewed as dtype, filled with `fill`, 0xA5 bytes when None) and, behind it, GUARD bytes of 0xA5"""

    def __init__(self, nbytes, dev, dtype=torch.float32, fill=None):
        self.nbytes = nbytes
        self.store = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.t = self.store[:nbytes].view(dtype)
        if fill is not None:
            self.t.fill_(fill)

    @property
    def guard(self):
        return self.store[self.nbytes:]


def _dev(dev, xs):
    return [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs]


def _abi():
    from contexture_nerf_amd import _lib as L
    return L, L.load()


# ---- the numpy tap rule (tests/test_field_texels_cpu.py's source index; numpy rounds every product and sum on its own) -----------------
def taps_np(uv, T):
    """uv [..., 2] f32 -> x0, y0 (int64) and the weights [4, ...] (nw, ne, sw, se) in binary32"""
    uv = np.asarray(uv, f32)
    ix = FT._src_index(uv[..., 0] * f32(2) - f32(1), T)
    iy = FT._src_index((f32(1) - uv[..., 1]) * f32(2) - f32(1), T)
    fx, fy = np.floor(ix), np.floor(iy)
    x1, y1 = fx + f32(1), fy + f32(1)
    w = np.stack([(x1 - ix) * (y1 - iy), (ix - fx) * (y1 - iy), (x1 - ix) * (iy - fy), (ix - fx) * (iy - fy)]).astype(f32)
    return fx.astype(np.int64), fy.astype(np.int64), w


def _mask_idx(shape, seed):
    """face ids with -1 on about a quarter of the pixels"""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 50, shape).astype(np.int64)
    m[rng.random(shape) < 0.25] = -1
    return m


# ---- texture mapping forward -------------------------------------------------------------------------------------------------------------
def fwd_uv(T):
    """[B, HW, 2] finite: exactly 0 and 1, below 0 and above 1 (the border clamp), texel centres (one weight 1, three 0), random rest"""
    uv = np.random.default_rng(T).uniform(-0.25, 1.25, (B, HW, 2)).astype(f32)
    uv[0, :6] = [[0, 0], [1, 1], [0, 1], [1, 0], [-0.5, 1.5], [2.0, -1.0]]
    j = np.arange(min(T, 16))
    uv[1, :len(j), 0] = ((j + 0.5) / T).astype(f32)
    uv[1, :len(j), 1] = (1.0 - (j + 0.5) / T).astype(f32)
    return uv


def _texmap_fwd(T, C, packed, mode, masked, Bt):
    def run(dev):
        L, lib = _abi()
        uv = fwd_uv(T)
        tex = np.random.default_rng(100 * T + C).standard_normal((Bt, C, T, T)).astype(f32)
        mask = _mask_idx((B, HW), T + C) if masked else None
        d_uv, d_tex, d_mask = _dev(dev, [uv, tex, mask])
        out = _Buf(B * HW * C * 4, dev)
        if packed:
            pk = _Buf(T * T * 16, dev)
            L.check(lib.ctx_texture_pack4(L.ptr(d_tex), C, T, L.ptr(pk.t), L.stream()))
            L.check(lib.ctx_texture_mapping_packed_fwd(L.ptr(d_uv), L.ptr(pk.t), B, HW, C, T, mode, L.ptr(d_mask), L.ptr(out.t), L.stream()))
            return [uv, tex, mask], {"packed": [pk.store], "out": [out.store]}
        L.check(lib.ctx_texture_mapping_fwd(L.ptr(d_uv), L.ptr(d_tex), B, HW, C, T, Bt, mode, L.ptr(d_mask), L.ptr(out.t), L.stream()))
        return [uv, tex, mask], {"out": [out.store]}
    return run


def _texmap_fwd_cases(T):
    cases = {}
    for mode in (0, 1):
        for masked in (False, True):
            tail = f"{'nearest' if mode else 'bilinear'}-mask{int(masked)}"
            for C in (1, 3, 4, 6):
                for Bt in (1, B):
                    cases[f"planar-C{C}-Bt{Bt}-{tail}"] = _texmap_fwd(T, C, False, mode, masked, Bt)
            for C in (1, 3, 4):
                cases[f"packed-C{C}-{tail}"] = _texmap_fwd(T, C, True, mode, masked, 1)
    return cases


# ---- texture mapping backward by float atomics: uv for which every texel receives at most one add ----------------------------------------
BWD_T, BWD_HW = 100, 544


def bwd_uv():
    """pixel (i, j) of a 33 x 33 grid samples the 2 x 2 block at (3i, 3j) with a fractional offset in [0.25, 0.75]; 2 x 544 of the cells"""
    rng = np.random.default_rng(7)
    cells = rng.permutation(33 * 33)[:B * BWD_HW]
    i, j = cells % 33, cells // 33
    fx, fy = rng.uniform(0.25, 0.75, cells.shape), rng.uniform(0.25, 0.75, cells.shape)
    uv = np.stack([(3 * i + fx + 0.5) / BWD_T, 1.0 - (3 * j + fy + 0.5) / BWD_T], -1).astype(f32).reshape(B, BWD_HW, 2)
    return uv, i.reshape(B, BWD_HW), j.reshape(B, BWD_HW)


def assert_taps_disjoint(uv, T):
    x0, y0, _ = taps_np(uv, T)
    flat = np.concatenate([((y0 + dy) * T + (x0 + dx)).reshape(-1) for dy in (0, 1) for dx in (0, 1)])
    assert x0.min() >= 0 and y0.min() >= 0 and x0.max() + 1 < T and y0.max() + 1 < T
    assert len(np.unique(flat)) == flat.size, "two pixels share a texel: the order of the float atomics would show"


def _texmap_bwd(C, masked):
    def run(dev):
        L, lib = _abi()
        uv, _, _ = bwd_uv()
        assert_taps_disjoint(uv, BWD_T)
        go = np.random.default_rng(C).standard_normal((B, BWD_HW, C)).astype(f32)
        mask = _mask_idx((B, BWD_HW), 11 + C) if masked else None
        d_go, d_uv, d_mask = _dev(dev, [go, uv, mask])
        gt = _Buf(C * BWD_T * BWD_T * 4, dev, fill=0.0)
        L.check(lib.ctx_texture_mapping_bwd(L.ptr(d_go), L.ptr(d_uv), B, BWD_HW, C, BWD_T, L.ptr(d_mask), L.ptr(gt.t), L.stream()))
        return [go, uv, mask], {"grad_tex": [gt.store]}
    return run


# ---- the active-texel mark ---------------------------------------------------------------------------------------------------------------
def _texel_mark(T):
    def run(dev):
        L, lib = _abi()
        H, W = 17, 15
        rng = np.random.default_rng(300 + T)
        uv = rng.uniform(-0.1, 1.1, (B, H, W, 2)).astype(f32)
        fi = _mask_idx((B, H, W), 400 + T)
        bg = fi < 0
        uv[bg] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30, -7.0], f32), (int(bg.sum()), 2))   # never read
        d_uv, d_fi = _dev(dev, [uv, fi])
        mask = _Buf(T * T, dev, torch.uint8, fill=0)
        L.check(lib.ctx_texel_active_mark(L.ptr(d_uv), L.ptr(d_fi), B, H, W, T, L.ptr(mask.t), L.stream()))
        return [uv, fi], {"mask": [mask.store]}
    return run


# ---- the scatter plan, the binned backward and the fixed-point scatter with and without a plan --------------------------------------------
def scatter_uv(T, kind, hw):
    rng = np.random.default_rng(T + len(kind))
    if kind == "random":
        return rng.random((B, hw, 2)).astype(f32)
    ix, iy = rng.uniform(0.2, 30.5, (B, hw)), rng.uniform(0.2, 30.5, (B, hw))       # every tap inside tile (0, 0): texels 0..31
    return np.stack([(ix + 0.5) / T, 1.0 - (iy + 0.5) / T], -1).astype(f32)


def _scatter(T, C, kind, hw, want_multi):
    def run(dev):
        L, lib = _abi()
        uv = scatter_uv(T, kind, hw)
        if kind != "random":
            x0, y0, _ = taps_np(uv, T)
            assert x0.min() >= 0 and y0.min() >= 0 and x0.max() + 1 < 32 and y0.max() + 1 < 32
        go = np.random.default_rng(T * C).standard_normal((B, hw, C)).astype(f32)
        mask = None if want_multi else _mask_idx((B, hw), T + C + hw)       # unmasked: all 8320 pixels enter the tile's list
        d_go, d_uv, d_mask = _dev(dev, [go, uv, mask])
        plan = _Buf(lib.ctx_texmap_bwd_plan_bytes(B, hw, T), dev, torch.uint8, fill=0)
        L.check(lib.ctx_texmap_bwd_plan(L.ptr(d_uv), L.ptr(d_mask), B, hw, T, L.ptr(plan.t), L.stream()))
        torch.cuda.synchronize()
        nchunks, nmulti = plan.t[32:40].view(torch.int32).tolist()
        assert (nmulti >= 1) == want_multi, f"{nchunks} chunks, {nmulti} multi-chunk tiles"
        got = {"plan": [plan.t[:64].clone(), plan.guard]}
        ws = _Buf(lib.ctx_texture_mapping_bwd_binned_ws_bytes(C, T), dev, torch.uint8)
        gt = _Buf(C * T * T * 4, dev, fill=0.0)
        L.check(lib.ctx_texture_mapping_bwd_binned(L.ptr(d_go), L.ptr(d_uv), L.ptr(d_mask), B, hw, C, T, L.ptr(plan.t), L.ptr(ws.t), L.ptr(gt.t),
                                                   L.stream()))
        got["binned"] = [gt.store, ws.guard]
        for name, p in (("fixed_plan", plan.t), ("fixed_direct", None)):
            acc = _Buf(C * T * T * 8, dev, torch.int64, fill=0)
            L.check(lib.ctx_uv_scatter_fixed(L.ptr(d_go), L.ptr(d_uv), L.ptr(d_mask), B, hw, C, T, L.ptr(p), 32, L.ptr(acc.t), L.stream()))
            got[name] = [acc.store]
        got["plan_after"] = [plan.t[:64].clone(), plan.guard]
        return [go, uv, mask], got
    return run


# ---- the ordered compactions -------------------------------------------------------------------------------------------------------------
def keep_mask(n, kind):
    if kind == "none":
        return np.zeros(n, bool)
    if kind == "all":
        return np.ones(n, bool)
    if kind == "half":
        return np.random.default_rng(n).random(n) < 0.5
    m = np.zeros(n, bool)
    m[-1] = True
    return m


def _texel_compact(n, kind):
    def run(dev):
        L, lib = _abi()
        keep = keep_mask(n, kind)
        mask = np.where(keep, np.random.default_rng(n + 1).integers(1, 256, n), 0).astype(np.uint8)
        d_mask, = _dev(dev, [mask])
        idx, cnt = _Buf(n * 4, dev, torch.int32), _Buf(8, dev, torch.int64)
        ws = _Buf(lib.ctx_texel_compact_ws_bytes(n), dev, torch.uint8)
        L.check(lib.ctx_texel_compact(L.ptr(d_mask), n, L.ptr(idx.t), L.ptr(cnt.t), L.ptr(ws.t), L.stream()))
        return [mask], {"idx": [idx.store, cnt.store, ws.guard]}
    return run


def _face_view_map(n, kind):
    def run(dev):
        L, lib = _abi()
        b, h, w = BHW[n]
        keep = keep_mask(n, kind)
        fi = np.where(keep, np.random.default_rng(n + 2).integers(0, 1000, n), -1).astype(np.int64).reshape(b, h, w)
        d_fi, = _dev(dev, [fi])
        rows, cnt = _Buf(n * 32, dev, torch.int64), _Buf(8, dev, torch.int64)
        ws = _Buf(lib.ctx_face_view_map_ws_bytes(b, h, w), dev, torch.uint8)
        L.check(lib.ctx_face_view_map(L.ptr(d_fi), b, h, w, L.ptr(rows.t), L.ptr(cnt.t), L.ptr(ws.t), L.stream()))
        return [fi], {"rows": [rows.store, cnt.store, ws.guard]}
    return run


# ---- view weights, positional encoding, camera rays --------------------------------------------------------------------------------------
def _view_weights(dev):
    L, lib = _abi()
    Bv, hw, F = 3, 513, 37
    rng = np.random.default_rng(37)
    fi = rng.integers(-1, F, (Bv, hw)).astype(np.int64)
    fi[0, :2] = [-1, F - 1]
    fnz = rng.standard_normal((Bv, F)).astype(f32)
    d_fi, d_fnz = _dev(dev, [fi, fnz])
    max_z = _Buf(F * 4, dev, fill=-3.0e38)
    vis = _Buf(Bv * F, dev, torch.uint8)
    mask = _Buf(Bv * hw, dev, torch.uint8)
    L.check(lib.ctx_view_weights_max(L.ptr(d_fi), L.ptr(d_fnz), Bv, hw, F, L.ptr(max_z.t), L.ptr(vis.t), L.stream()))
    L.check(lib.ctx_view_weights_mask(L.ptr(d_fi), L.ptr(d_fnz), L.ptr(max_z.t), Bv, hw, F, L.ptr(mask.t), L.stream()))
    return [fi, fnz], {"max_z": [max_z.store, vis.store], "mask": [mask.store]}


def _embed(d, Lf):
    def run(dev):
        L, lib = _abi()
        N = 257
        x = np.random.default_rng(10 * d + Lf).uniform(-1, 1, (N, d)).astype(f32)
        d_x, = _dev(dev, [x])
        out = _Buf(N * d * (1 + 2 * Lf) * 4, dev)
        L.check(lib.ctx_embed_fwd(L.ptr(d_x), N, d, Lf, L.ptr(out.t), L.stream()))
        return [x], {"out": [out.store]}
    return run


def _get_rays(dev):
    L, lib = _abi()
    H, W = 5, 7
    c2w = np.random.default_rng(57).standard_normal((3, 4)).astype(f32)
    d_c2w, = _dev(dev, [c2w])
    ro, rd = _Buf(H * W * 12, dev), _Buf(H * W * 12, dev)
    L.check(lib.ctx_get_rays(H, W, 6.5, 7.25, 3.5, 2.5, L.ptr(d_c2w), L.ptr(ro.t), L.ptr(rd.t), L.stream()))
    return [c2w], {"rays": [ro.store, rd.store]}


# ---- the cases: group -> {case: function(dev) -> (inputs, {output group: arrays})} ---------------------------------------------------------
GROUPS = {}
for _T in TS:
    GROUPS[f"texmap-fwd-T{_T}"] = _texmap_fwd_cases(_T)
GROUPS["texmap-bwd-T100"] = {f"C{C}-mask{int(m)}": _texmap_bwd(C, m) for C in (1, 3) for m in (False, True)}
GROUPS["texel-mark"] = {f"T{_T}": _texel_mark(_T) for _T in TS}
# every pixel in one tile at 2 x 65 x 63 = 8190 pixels stays under the 8192 entries of one chunk; one more pixel row (2 x 65 x 64 = 8320)
# is what cuts the tile's list into two chunks, so that set is here as well
SCATTER_SETS = (("random", 65 * 63, False), ("one-tile", 65 * 63, False), ("one-tile-two-chunks", 65 * 64, True))
for _T in (33, 100):
    GROUPS[f"scatter-T{_T}"] = {f"{kind}-C{C}": _scatter(_T, C, kind, hw, multi) for kind, hw, multi in SCATTER_SETS for C in (1, 4)}
for _n in COMPACT_N:
    GROUPS[f"texel-compact-n{_n}"] = {k: _texel_compact(_n, k) for k in MASKS}
    GROUPS[f"face-view-map-n{_n}"] = {k: _face_view_map(_n, k) for k in MASKS}
GROUPS["view-weights"] = {"B3-HW513-F37": _view_weights}
GROUPS["embed"] = {f"d{d}-L{Lf}": _embed(d, Lf) for d in (2, 3) for Lf in (0, 10)}
GROUPS["get-rays"] = {"5x7": _get_rays}


def compute(group, dev):
    """-> {case: {"in": digest, "out": {output group: digest}}} of one group, from the library _lib.load() gives."""
    out = {}
    for case, run in GROUPS[group].items():
        inputs, got = run(dev)
        torch.cuda.synchronize()
        out[case] = {"in": digest(inputs), "out": {k: digest(v) for k, v in got.items()}}
    return out


def test_the_case_list_is_the_fixtures():
    """No GPU needed: the fixture holds exactly the cases of this module and says what it was recorded from; the input makers give what
    the cases are there for."""
    with open(FIXTURE) as f:
        fix = json.load(f)
    assert {g: sorted(c) for g, c in fix["cases"].items()} == {g: sorted(c) for g, c in GROUPS.items()}
    assert fix["hipcc"] and len(fix["recorded_from"]) >= 7
    assert all(np.prod(BHW[n]) == n for n in COMPACT_N) and set(BHW) == set(COMPACT_N)
    for T in TS:
        uv = fwd_uv(T)
        assert np.isfinite(uv).all() and (uv == 0).any() and (uv == 1).any() and (uv < 0).any() and (uv > 1).any()
        w = taps_np(uv, T)[2]
        assert (np.sort(w, 0) == np.array([0, 0, 0, 1], f32)[:, None, None]).all(0).any(), "no pixel sits on a texel centre"
    uv, i, j = bwd_uv()
    x0, y0, w = taps_np(uv, BWD_T)
    assert np.array_equal(x0, 3 * i) and np.array_equal(y0, 3 * j)
    assert_taps_disjoint(uv, BWD_T)


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_raster_atlas_bits_are_the_parents(dev, group):
    with open(FIXTURE) as f:
        fix = json.load(f)
    got = compute(group, dev)
    try:
        now = _hipcc_version()
    except (OSError, subprocess.SubprocessError, IndexError):
        now = "unknown"
    recorded = f"commit {fix['recorded_from']} built with {fix['hipcc']!r}"
    hint = recorded + (" (the same compiler as here: a kernel changed)" if now == fix["hipcc"] else
                       f"; the compiler here is {now!r}: re-record from the parent commit before blaming a kernel")
    for case, want in fix["cases"][group].items():
        assert got[case]["in"] == want["in"], f"{group}/{case}: the inputs changed (an input maker, not a kernel)"
        for k, h in want["out"].items():
            assert got[case]["out"][k] == h, f"{group}/{case}/{k}: bits differ from {hint}"


def _hipcc_version():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return subprocess.run([hipcc, "--version"], capture_output=True, text=True, check=True).stdout.splitlines()[0].strip()


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--write", action="store_true", required=True)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--commit", default=None, help="the commit whose csrc/ the library was built from (default: HEAD)")
    a = ap.parse_args()
    compiler = _hipcc_version()
    from contexture_nerf_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    assert torch.cuda.is_available(), "recording needs the GPU"
    _lib.check(_lib.load().ctx_device_check())
    device = torch.device("cuda:0")
    commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    fixture = {"hipcc": compiler, "recorded_from": commit, "cases": {g: compute(g, device) for g in GROUPS}}
    with open(FIXTURE, "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {sum(len(c) for c in fixture['cases'].values())} cases from {_lib.LIB_PATH} into {FIXTURE}")
