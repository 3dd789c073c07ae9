"""GPU: the bits of the ray-path kernels (dense and packed compositing forward and backward, distortion forward and backward, resample,
march count and write) against digests recorded from the parent commit's build, so that a refactor of these kernels is held to "no
result bit changes" by something other than the code under test.

tests/golden/ray_path_bits.json holds, per case, a SHA-256 over the raw bytes of its inputs and one over the raw bytes of each group of
outputs (NaN patterns included), the `hipcc --version` line of the recording and the commit whose `csrc/` was built for it.  A changed
input digest means an input maker changed, not a kernel.  A compiler change that moves the output digests re-records them from the
then-parent commit's build:

    python tests/test_ray_bits_gpu.py --write [--lib PATH] [--commit HASH]        # PATH: that build's libctxnerf.so (default: the tree's own)
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
import distortion_rule as dr
import march_rule as mr
import resample_rule as rr
import test_occupancy_mesh_cpu as OM
from test_march_cpu import ragged_counts
from test_raymarch_train_cpu import make_case, make_grads

f32 = np.float32
FIXTURE = os.path.join(ROOT, "tests", "golden", "ray_path_bits.json")
NAN = float('nan')
NEAR, FAR = 0.5, 2.5
DENSE = [(1, 1), (5, 33), (3, 64), (4, 65), (6, 257)]
SWITCHES = [(white, noise) for white in (False, True) for noise in (False, True)]
RESAMPLE_K = (1, 64, 65, 130)
MARCH = ("G4-R65-p0.5", "G32-R300-p0.02")
COUNTS = ragged_counts(23, 4)                   # {0, 1, 2, 63, 64, 65, 130}, the first and the last ray empty
POISON = [3, 4097, 70, 0]


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


def _dev(dev, xs):
    return [None if x is None else (torch.from_numpy(x) if isinstance(x, np.ndarray) else x).to(dev) for x in xs]


def _full(dev, fill, *shapes, dtype=torch.float32):
    return [torch.full(s, fill, dtype=dtype, device=dev) for s in shapes]


# ---- the cases: name -> function(dev) -> (inputs, {group: outputs}) ------------------------------------------------------------------------
def _dense(R, S, white, with_noise):
    def run(dev):
        from contexture_nerf_amd import _lib as L
        lib = L.load()
        host = make_case(R, S, seed=R * 100 + S, with_noise=with_noise)
        hgrads = {which: make_grads(R, S, which, seed=S) for which in ('all', 'rgb')}
        raw, z, d, noise = _dev(dev, host)
        outs = _full(dev, NAN, (R, 3), (R,), (R,), (R, S), (R,))
        if noise is None:
            L.check(lib.ctx_raymarch_composite_fwd(L.ptr(raw), L.ptr(z), L.ptr(d), R, S, int(white), *map(L.ptr, outs), L.stream()))
        else:
            L.check(lib.ctx_raymarch_composite_fwd_noise(L.ptr(raw), L.ptr(z), L.ptr(d), L.ptr(noise), R, S, int(white), *map(L.ptr, outs),
                                                         L.stream()))
        got = {"fwd": outs}
        for which, hg in hgrads.items():
            grad, = _full(dev, NAN, (R, S, 4))
            L.check(lib.ctx_raymarch_composite_bwd(L.ptr(raw), L.ptr(z), L.ptr(d), L.ptr(noise), R, S, int(white), *map(L.ptr, _dev(dev, hg)),
                                                   L.ptr(grad), L.stream()))
            got["bwd_" + which] = [grad]
        return list(host) + hgrads['all'], got
    return run


def _packed(counts, seed, gseed, white, with_noise, prefill):
    def run(dev):
        from contexture_nerf_amd import _lib as L
        lib = L.load()
        host = mr.make_packed_case(counts, seed=seed, with_noise=with_noise)
        R, n = len(counts), host[0].shape[0]
        hgrads = mr.make_packed_grads(R, n, seed=gseed)
        raw, t, dt, d, ray_off, noise = _dev(dev, host)
        outs = _full(dev, NAN, (R, 3), (R,), (R,), (n,), (R,))
        L.check(lib.ctx_raymarch_packed_fwd(L.ptr(raw), L.ptr(t), L.ptr(dt), L.ptr(d), L.ptr(noise), L.ptr(ray_off), R, n, int(white),
                                            *map(L.ptr, outs), L.stream()))
        got = {"fwd": outs}
        for which, hg in (("all", hgrads), ("rgb", [hgrads[0], None, None, None, None])):
            grad, = _full(dev, prefill, (n, 4))
            L.check(lib.ctx_raymarch_packed_bwd(L.ptr(raw), L.ptr(t), L.ptr(dt), L.ptr(d), L.ptr(noise), L.ptr(ray_off), R, n, int(white),
                                                *map(L.ptr, _dev(dev, hg)), L.ptr(grad), L.stream()))
            got["bwd_" + which] = [grad]
        return list(host) + hgrads, got
    return run


def _distortion(norm):
    def run(dev):
        from contexture_nerf_amd import _lib as L
        lib = L.load()
        k = dr.NORMS.index(norm)
        host = list(dr.make_case(COUNTS, seed=40 + k, norm=norm)) + [np.random.default_rng(50 + k).standard_normal(len(COUNTS)).astype(f32)]
        w, t, dt, d, ray_off, g_loss = _dev(dev, host)
        R, n = len(COUNTS), host[0].shape[0]
        loss, grad = _full(dev, NAN, (R,), (n,))
        L.check(lib.ctx_distortion_packed_fwd(L.ptr(w), L.ptr(t), L.ptr(dt), L.ptr(d), L.ptr(ray_off), R, n, L.ptr(loss), L.stream()))
        L.check(lib.ctx_distortion_packed_bwd(L.ptr(w), L.ptr(t), L.ptr(dt), L.ptr(d), L.ptr(ray_off), R, n, L.ptr(g_loss), L.ptr(grad),
                                              L.stream()))
        return host, {"fwd": [loss], "bwd": [grad]}
    return run


def _resample(K, drawn):
    def run(dev):
        from contexture_nerf_amd import _lib as L
        host = list(rr.make_lists(COUNTS, seed=31))
        fine_off = np.concatenate([[0], np.cumsum(np.asarray(COUNTS) > 0) * K]).astype(np.int64)
        n1 = int(fine_off[-1])
        host += [fine_off, np.random.default_rng(K + 1).random(n1).astype(f32) if drawn else None]
        w, ts, dt, ray_off, ro, rd, foff, xi = _dev(dev, host)
        ray_id, = _full(dev, -1, (n1,), dtype=torch.int32)
        outs = [ray_id] + _full(dev, NAN, (n1,), (n1,), (n1, 3))
        L.check(L.load().ctx_resample_packed(L.ptr(w), L.ptr(ts), L.ptr(dt), L.ptr(ray_off), L.ptr(ro), L.ptr(rd), len(COUNTS), w.shape[0], K,
                                             L.ptr(foff), L.ptr(xi), n1, *map(L.ptr, outs), L.stream()))
        return host, {"out": outs}
    return run


def _march(name, step_index, given):
    def run(dev):
        from contexture_nerf_amd import _lib as L, volume_render as vr
        lib = L.load()
        _, G, cells, R, seed = next(c for c in mr.march_cases() if c[0] == name)
        step = mr.march_steps(G)[step_index]
        ro, rd = OM.span_rays(np.random.default_rng(seed), R)
        grid = vr.OccupancyGrid.from_mask(torch.from_numpy(cells != 0).to(dev), -1.0, 1.0)
        args = (L.ptr(grid.cells, torch.uint8, "cells"), grid.G, *map(float, grid.lo), *map(float, grid.hi), *map(float, grid.inv),
                *map(float, grid.h), float(step))
        d_ro, d_rd = _dev(dev, [ro, rd])
        count, = _full(dev, -7, (R,), dtype=torch.int32)
        L.check(lib.ctx_occ_march_count(L.ptr(d_ro), L.ptr(d_rd), R, NEAR, FAR, *args, L.ptr(count), L.stream()))
        ray_off = torch.zeros(R + 1, dtype=torch.int64, device=dev)
        ray_off[1:] = torch.cumsum(count, 0, dtype=torch.int64)
        n = int(ray_off[-1].item())
        u = np.random.default_rng(seed + 5).random(n).astype(f32) if given else None
        d_u, = _dev(dev, [u])
        ray_id, = _full(dev, -1, (n,), dtype=torch.int32)
        lists = [ray_id] + _full(dev, NAN, (n,), (n,), (n, 3))
        L.check(lib.ctx_occ_march_write(L.ptr(d_ro), L.ptr(d_rd), R, NEAR, FAR, *args, L.ptr(ray_off), L.ptr(d_u), n, *map(L.ptr, lists),
                                        L.stream()))
        return [ro, rd, cells, f32(step), u], {"count": [count], "write": lists}
    return run


def _sw(white, noise):
    return f"white{int(white)}-noise{int(noise)}"


GROUPS = {}
for _R, _S in DENSE:
    GROUPS[f"dense-{_R}x{_S}"] = {_sw(w, nz): _dense(_R, _S, w, nz) for w, nz in SWITCHES}
GROUPS["packed-ragged"] = {_sw(w, nz): _packed(COUNTS, 21, 6, w, nz, NAN) for w, nz in SWITCHES}
GROUPS["packed-poison"] = {"white0-noise0": _packed(POISON, 8, 1, False, False, 0.0)}
for _norm in dr.NORMS:
    GROUPS[f"distortion-norm{_norm:g}"] = {"fwd-bwd": _distortion(_norm)}
for _K in RESAMPLE_K:
    GROUPS[f"resample-K{_K}"] = {("xi-given" if drawn else "xi-absent"): _resample(_K, drawn) for drawn in (False, True)}
for _name in MARCH:
    GROUPS[f"march-{_name}"] = {f"step{i}-{'u-given' if given else 'u-absent'}": _march(_name, i, given) for i in (0, 1) for given in (False, True)}


def compute(group, dev):
    """-> {case: {"in": digest, "out": {output group: digest}}} of one group, from the library _lib.load() gives."""
    out = {}
    for case, run in GROUPS[group].items():
        inputs, got = run(dev)
        torch.cuda.synchronize()
        out[case] = {"in": digest(inputs), "out": {k: digest(v) for k, v in got.items()}}
    return out


def test_the_case_list_is_the_fixtures():
    """No GPU needed: the fixture holds exactly the cases of this module, and says what it was recorded from."""
    with open(FIXTURE) as f:
        fix = json.load(f)
    assert {g: sorted(c) for g, c in fix["cases"].items()} == {g: sorted(c) for g, c in GROUPS.items()}
    assert set(COUNTS) == {0, 1, 2, 63, 64, 65, 130} and COUNTS[0] == 0 and COUNTS[-1] == 0
    assert fix["hipcc"] and len(fix["recorded_from"]) >= 7


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_ray_path_bits_are_the_parents(dev, group):
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
