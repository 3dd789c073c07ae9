#!/usr/bin/env python3
"""Record tests/golden/view_consistency.npz from the reference's own `ConTEXTure.compute_view_consistency`
(src/training/trainer.py:429-531), called unbound on the CPU under make_golden.py's stubs.

Runs ONLY where the reference checkout exists (see make_golden.REF); no test reads the reference.  Nothing of the reference's
source text is stored: seeded inputs, the oracle's raster of the bundled spot mesh, and the numbers the function returned.

Inputs (spot_triangulated, poses 1..6 of the seven Zero123PlusDataset poses, 160 squared, oracle.geometry raster):
  faces [F,3] i32, face_idx [6,160,160] i32, vertex_image [6,n_vertices,2] f32 (face_vertices_image = vertex_image[:, faces])
  case A: views = torch.rand from A_seed (stored as the seed); case B: views = rasterised vertex position in [0,1] per axis,
  0.5 on the background (rebuilt by the test from the oracle; B_views_crc32 pins the bytes).
Outputs per case and row convention ('image' rows are the same function fed -Y):
  *_mean (the reference's f32 mean), *_N (pairs it averaged), *_mean_err = |mean - float64 mean of its own per-pair terms|
  (the terms are caught by wrapping torch.mean as the imported module sees it);
  case A: the autograd gradient with respect to the views (sparse: A_grad_index / A_grad_values), A_grad_frac_max =
  max |grad / u - rint(grad / u)| (refused above 0.01), A_grad_dev_max_u = max |f32(rint(grad / u)) * u - grad| / u.
The script asserts that every (sy, sx) the reference forms is inside the image: it neither raised nor wrapped."""
import importlib
import os
import sys
import types
import zlib
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True
A_SEED = 20240531
H = 160


def call_reference(T, views, faces, face_idx, fvi, grad=False):
    """-> (mean f32, N, float64 mean of the reference's own per-pair terms, gradient | None)."""
    caught = []
    real_mean = T.torch.mean

    def spy(x, *a, **k):
        caught.append(x.detach().clone())
        return real_mean(x, *a, **k)
    v = torch.from_numpy(views).clone().requires_grad_(grad)
    T.torch.mean = spy
    try:
        m = T.ConTEXTure.compute_view_consistency(types.SimpleNamespace(device=torch.device('cpu')), v, torch.from_numpy(faces),
                                                  torch.from_numpy(face_idx), torch.from_numpy(fvi))
    finally:
        T.torch.mean = real_mean
    assert len(caught) == 1 and caught[0].dtype == torch.float32
    g = None
    if grad:
        m.backward()
        g = v.grad.numpy().copy()
    return np.float32(m.item()), int(caught[0].numel()), float(caught[0].double().mean()), g


def assert_inside(fvi, h, w):
    """Every pixel position the reference forms from these coordinates (its vertex_to_pixel_map, both Y signs) is inside."""
    for sign in (1.0, -1.0):
        c = fvi.copy(); c[..., 1] *= np.float32(sign)
        xy = ((torch.from_numpy(c).reshape(-1, 2) + 1) / 2 * torch.tensor([w, h], dtype=torch.float32)).long().numpy()
        assert xy.min() >= 0 and xy[:, 0].max() < w and xy[:, 1].max() < h, "a source pixel outside the image: the reference would raise or wrap"


def main():
    from make_golden import _stub_env
    import test_view_consistency_cpu as VC
    _stub_env()
    T = importlib.import_module('src.training.trainer')
    meshes = np.load(os.path.join(ROOT, "shapes", "meshes.npz"))
    faces, face_idx, fvi, views_b = VC.spot_case(meshes, H)
    V, n_vertices = face_idx.shape[0], int(faces.max()) + 1
    vimg = np.zeros((V, n_vertices, 2), np.float32)
    vimg[:, faces.reshape(-1)] = fvi.reshape(V, -1, 2)
    assert np.array_equal(vimg[:, faces], fvi), "face_vertices_image is not a per-vertex table indexed by faces"
    assert_inside(fvi, H, H)
    print(f"image coordinates span [{fvi.min():.3f}, {fvi.max():.3f}]")
    flipped = fvi.copy(); flipped[..., 1] = -flipped[..., 1]
    out = dict(faces=faces.astype(np.int32), face_idx=face_idx.astype(np.int32), vertex_image=vimg, A_seed=np.int64(A_SEED),
               B_views_crc32=np.int64(zlib.crc32(views_b.tobytes())))
    views_a = VC.random_views(A_SEED, V, 3, H, H)
    for tag, views, coords, grad in (('A_reference', views_a, fvi, True), ('B_reference', views_b, fvi, False), ('B_image', views_b, flipped, False)):
        mean, N, mean64, g = call_reference(T, views, faces, face_idx, coords, grad)
        out[tag + '_mean'], out[tag + '_N'], out[tag + '_mean_err'] = mean, np.int64(N), np.float64(abs(float(mean) - mean64))
        print(f"{tag}: mean {mean:.9f}, N {N}, |mean - mean_f64| {abs(float(mean) - mean64):.3e}")
        if grad:
            u = (np.float32(1) / np.float32(N)) / np.float32(3)
            ratio = g.astype(np.float64) / np.float64(u)
            cnt = np.rint(ratio)
            frac = float(np.abs(ratio - cnt).max())
            dev = float(np.abs((cnt.astype(np.float32) * u).astype(np.float64) - g.astype(np.float64)).max() / float(u))
            print(f"{tag} gradient: |count| up to {int(np.abs(cnt).max())}, max |grad / u - rint| {frac:.3e}, max |f32(count) * u - grad| {dev:.3e} u")
            assert frac <= 0.01, "the gradient's integers are ambiguous: fixture refused"
            nz = np.flatnonzero(g.reshape(-1))
            out['A_grad_index'], out['A_grad_values'] = nz.astype(np.int32), g.reshape(-1)[nz]
            out['A_grad_frac_max'], out['A_grad_dev_max_u'] = np.float64(frac), np.float64(dev)
    path = os.path.join(HERE, "view_consistency.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
