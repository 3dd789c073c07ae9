"""CPU: the texture field on the texels the views sample (optim.field_texels = 'active') — the definition of the active set, the
config surface and the host control flow.

`active_texels_np` below IS the rule csrc/texmap.hip (ctx_texel_active_mark) and csrc/compact.hip (ctx_texel_compact) are held to;
tests/test_field_texels_gpu.py imports it from here and compares with array_equal.  All float arithmetic is binary32 in the order of
k_texmap_fwd (numpy array operations round every product and sum on their own: no contraction).

1. the restatement on the oracle raster of spot (two poses, 96 x 80) at T = 64 and 257: it is the union of taps a plain loop lists,
   the oracle's texture_mapping of an atlas zeroed off the set equals that of the full atlas, dropping a listed texel breaks that,
   NaN uv on the background changes nothing;
2. config: optim.field_texels default, YAML / CLI, a bad value;
3. host control flow with the new entry points stubbed at the _lib seam."""
import types
import numpy as np
import pytest
import torch

import test_atlas_fill_cpu as R
import test_dist_product_cpu as P

f32 = np.float32


# ---- the numpy restatement ------------------------------------------------------------------------------------------------
def _src_index(g, T):
    c = ((g + f32(1)) * f32(T) - f32(1)) / f32(2)
    return np.fmin(f32(T - 1), np.fmax(c, f32(0)))            # fminf / fmaxf: a NaN coordinate clamps to 0


def active_texels_np(uv, face_idx, T, mask=None):
    """uv [B,H,W,2] f32, face_idx [B,H,W] i64 -> (idx int32 [n] ascending, mask uint8 [T,T]).  mask given: marked in place (a union).
    The uv of a background pixel is never looked at."""
    fg = np.asarray(face_idx) >= 0
    if mask is None:
        mask = np.zeros((T, T), np.uint8)
    q = np.asarray(uv, f32)[fg]
    with np.errstate(all='ignore'):
        ix = _src_index(q[:, 0] * f32(2) - f32(1), T)
        iy = _src_index((f32(1) - q[:, 1]) * f32(2) - f32(1), T)
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    for dy in (0, 1):
        for dx in (0, 1):
            x, y = x0 + dx, y0 + dy
            ok = (x >= 0) & (x < T) & (y >= 0) & (y < T)
            mask[y[ok], x[ok]] = 1
    return np.flatnonzero(mask.reshape(-1)).astype(np.int32), mask


def spot_raster(meshes, n_views=2, H=96, W=80):
    """The oracle raster of the first poses of spot with its own UVs -> (uv [n,H,W,2] f32, face_idx [n,H,W] i64)."""
    from oracle import geometry as og
    v, f, vt, ft, cam, proj = R.spot_arrays(meshes)
    o_cam, o_img, _ = og.prepare_vertices(np.repeat(v[None], n_views, 0), f, proj, cam[:n_views])
    return og.rasterize(H, W, o_cam[..., 2], o_img, np.repeat(vt[ft][None], n_views, 0))


@pytest.fixture(scope="module")
def raster(meshes):
    return spot_raster(meshes)


# ---- 1. the rule ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [64, 257])
def test_active_set_is_the_union_of_taps(raster, T):
    uv, idx = raster
    crop = (slice(None), slice(40, 56), slice(30, 44))
    uvc, idc = uv[crop], idx[crop]
    assert (idc >= 0).any() and (idx < 0).any()
    want = set()
    for b, y, x in zip(*np.nonzero(idc >= 0)):
        u, v = uvc[b, y, x]
        ix = float(_src_index(f32(u * f32(2) - f32(1)), T)); iy = float(_src_index(f32((f32(1) - v) * f32(2) - f32(1)), T))
        x0, y0 = int(np.floor(ix)), int(np.floor(iy))
        want |= {(yy, xx) for yy in (y0, y0 + 1) for xx in (x0, x0 + 1) if 0 <= xx < T and 0 <= yy < T}
    got, mask = active_texels_np(uvc, idc, T)
    assert got.dtype == np.int32 and np.all(np.diff(got) > 0)
    assert {(int(i) // T, int(i) % T) for i in got} == want and int(mask.sum()) == len(want)
    # two calls into one mask give the union; the whole raster holds the crop's set
    m2 = active_texels_np(uv[:1], idx[:1], T)[1]
    both, _ = active_texels_np(uv[1:], idx[1:], T, m2)
    whole, _ = active_texels_np(uv, idx, T)
    assert np.array_equal(both, whole) and set(got.tolist()) <= set(whole.tolist()) and 0 < len(whole) < T * T


@pytest.mark.parametrize("T", [64, 257])
def test_render_needs_exactly_the_active_texels(raster, T):
    from oracle import geometry as og
    uv, idx = raster
    fg = idx >= 0
    listed, mask = active_texels_np(uv, idx, T)
    rng = np.random.default_rng(T)
    tex = (rng.random((1, 3, T, T)) + 0.5).astype(f32)            # no zero texel: dropping one always changes a product with a weight > 0
    full = og.texture_mapping(uv, tex)
    part = og.texture_mapping(uv, tex * mask[None, None])
    assert np.array_equal(part[fg], full[fg])
    for t in rng.choice(listed, 24, replace=False):
        m = mask.copy(); m.reshape(-1)[t] = 0
        out = og.texture_mapping(uv, tex * m[None, None])
        assert not np.array_equal(out[fg], full[fg]), f"texel {t} is listed but no foreground pixel reads it"
    # whatever the background's uv holds, it is not read
    uv_nan = uv.copy(); uv_nan[~fg] = np.nan
    assert np.array_equal(active_texels_np(uv_nan, idx, T)[0], listed)
    assert len(active_texels_np(uv_nan, np.full_like(idx, -1), T)[0]) == 0


def test_clamped_uv_marks_inside_the_atlas_only():
    T = 8
    uv = np.array([[[[0.0, 0.0], [1.0, 1.0], [0.0, 1.0], [1.0, 0.0]]]], f32)      # ix in {0, T-1}: x1 = T is dropped
    idx, mask = active_texels_np(uv, np.zeros((1, 1, 4), np.int64), T)
    want = np.zeros((T, T), np.uint8)
    want[T - 1, 0:2] = 1; want[0, T - 1] = 1; want[0, 0:2] = 1; want[1, 0:2] = 1; want[T - 1, T - 1] = 1; want[1, T - 1] = 1
    # (u, v) = (0, 0): ix = 0, iy = T-1 -> (T-1, 0), (T-1, 1);  (1, 1): ix = T-1, iy = 0 -> (0, T-1), (1, T-1);
    # (0, 1): ix = 0, iy = 0 -> (0..1, 0..1);  (1, 0): ix = iy = T-1 -> (T-1, T-1)
    assert np.array_equal(mask, want) and np.array_equal(idx, np.flatnonzero(want))


def test_compaction_workspaces_share_one_layout():
    """ctx_texel_compact_ws_bytes(n) and ctx_face_view_map_ws_bytes(B, H, W): one int64 base and one int32 count per block of 1024
    items and 64 spare bytes, at the block edges and up to the largest n; n = 0 and n = 2^31 are refused (the indices are int32)."""
    from contexture_nerf_amd import _lib as L
    lib = L.load()
    edges = [1, 2, 63, 64, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097, 2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1, 3 * 2 ** 20 + 517, 2 ** 31 - 1]
    for n in edges:
        want = -(-n // 1024) * 12 + 64
        assert lib.ctx_texel_compact_ws_bytes(n) == want, n
        assert lib.ctx_face_view_map_ws_bytes(1, 1, n) == want, n
    assert lib.ctx_face_view_map_ws_bytes(7, 1200, 1200) == -(-7 * 1200 * 1200 // 1024) * 12 + 64
    assert lib.ctx_face_view_map_ws_bytes(3, 11, 31) == 12 + 64 and lib.ctx_face_view_map_ws_bytes(1, 25, 41) == 24 + 64
    for n in (0, -1, 2 ** 31, 2 ** 40):
        assert lib.ctx_texel_compact_ws_bytes(n) == -1, n


# ---- 2. config ------------------------------------------------------------------------------------------------------------------
def test_config_field_texels_default_cli_and_validation(tmp_path):
    from contexture_nerf_amd import config as CFG
    assert CFG.TrainConfig().optim.field_texels == 'all'
    assert CFG.parse(argv=[]).optim.field_texels == 'all'
    assert CFG.parse(argv=['--optim.field_texels=active']).optim.field_texels == 'active'
    with pytest.raises(ValueError, match="field_texels"):
        CFG.parse(argv=['--optim.field_texels=chart'])
    y = tmp_path / "c.yaml"
    y.write_text("optim:\n  field_texels: active\n  sds_iterations: 3\n")
    cfg = CFG.parse(argv=[f'--config_path={y}'])
    assert cfg.optim.field_texels == 'active' and cfg.optim.sds_iterations == 3
    y.write_text("optim:\n  field_texels: none\n")
    with pytest.raises(ValueError, match="field_texels"):
        CFG.parse(argv=[f'--config_path={y}'])
    CFG.dump(cfg, tmp_path / "d.yaml")
    assert CFG.parse(argv=[f'--config_path={tmp_path / "d.yaml"}']).optim.field_texels == 'active'


# ---- 3. host control flow with the entry points stubbed at the _lib seam --------------------------------------------------------
H, W, T, F = P.H, P.W, 32, P.F          # T: large enough that the synthetic rasters leave texels unsampled


class FieldLib(P.FakeLib):
    """The new entry points as numpy stand-ins (tensors arrive where pointers would); every call is recorded."""

    def __init__(self, calls, empty=False):
        self.calls, self.empty = calls, empty

    def ctx_texel_active_mark(self, uv, face_idx, B, H_, W_, T_, mask, stream):
        assert tuple(uv.shape) == (B, H_, W_, 2) and uv.dtype == torch.float32 and face_idx.dtype == torch.int64
        assert tuple(mask.shape) == (T_, T_) and mask.dtype == torch.uint8 and not mask.any()
        self.calls.append('mark')
        if not self.empty:
            active_texels_np(uv.numpy(), face_idx.numpy(), T_, mask.numpy())
        return 0

    def ctx_texel_compact_ws_bytes(self, n):
        return 64

    def ctx_texel_compact(self, mask, n, idx, count, ws, stream):
        assert idx.dtype == torch.int32 and idx.numel() == n and count.dtype == torch.int64
        self.calls.append('compact')
        nz = np.flatnonzero(mask.numpy().reshape(-1))
        idx.numpy()[:len(nz)] = nz
        count.numpy()[0] = len(nz)
        return 0


class FakeField(torch.nn.Module):
    """NeRF2D's texture_map seam: a constant-colour atlas of one trainable colour; records the list it was handed."""

    def __init__(self, calls):
        super().__init__()
        self.colour = torch.nn.Parameter(torch.tensor([0.2, 0.5, 0.8]))
        self.calls = calls

    def texture_map(self, res, texels=None):
        self.calls.append(('field', texels))
        n = res * res if texels is None else texels.numel()
        return self.colour.view(1, 3, 1, 1).expand(1, 3, res, res), self.colour.expand(n, 3)


class FakeRenderer:
    """Renderer.render_multiple_view_texture: the synthetic rasters of test_dist_product_cpu; like the real one it hands back a
    NEW cache dict holding its own keys only."""

    def render_multiple_view_texture(self, verts, faces, uv_face_attr, texture_map, elev, azim, radius, look_at_height=0.0, dims=None,
                                     background_type='none', render_cache=None):
        if render_cache is None:
            views = [P.fake_view(k) for k in range(len(azim))]
            uv = torch.from_numpy(np.stack([v[2] for v in views]))
            fi = torch.from_numpy(np.stack([v[0] for v in views]))
        else:
            uv, fi = render_cache['uv_features'], render_cache['face_idx']
        B = uv.shape[0]
        mask = (fi > -1).float()[:, None]
        img = texture_map.mean((2, 3))[:, :, None, None] * mask
        return img, mask, 0.5 * mask, torch.zeros(B, 3, H, W), {'uv_features': uv, 'face_idx': fi, 'face_vertices_image': torch.zeros(B, F, 3, 2)}


def _mesh_model(calls):
    from contexture_nerf_amd.textured_mesh import TexturedMeshModel
    mm = TexturedMeshModel.__new__(TexturedMeshModel)
    torch.nn.Module.__init__(mm)
    mm.device, mm.dy, mm.texture_resolution = torch.device('cpu'), 0.25, T
    mm.mesh = types.SimpleNamespace(vertices=torch.zeros(5, 3), faces=torch.zeros(F, 3, dtype=torch.int64))
    mm.face_attributes, mm.renderer, mm.texture_mlp = torch.zeros(1, F, 3, 2), FakeRenderer(), FakeField(calls)
    return mm


def _sds_trainer(monkeypatch, calls, field_texels, empty=False):
    from contexture_nerf_amd import _lib as L, config as CFG, sds
    from contexture_nerf_amd.trainer import ConTEXTure
    monkeypatch.setattr(L, 'load', lambda: FieldLib(calls, empty))
    monkeypatch.setattr(L, 'ptr', lambda t, dtype=None, name="tensor": t)
    monkeypatch.setattr(L, 'stream', lambda: None)
    monkeypatch.setattr(sds, 'to_rgb_image', lambda rgba: rgba[:, :3])
    monkeypatch.setattr(sds, 'build_depth_grid', lambda depth, masks, size: None)
    monkeypatch.setattr(sds, 'sds_iteration', lambda pipe, tiles, *a, **k: dict(loss=tiles.sum(), ikl_running_avg=0.0, fisher=0.0, index=0))
    tr = ConTEXTure.__new__(ConTEXTure)
    tr.cfg = CFG.TrainConfig(); tr.cfg.guide.texture_resolution = T; tr.cfg.optim.field_texels = field_texels
    tr.device, tr.group, tr.rank, tr.world = torch.device('cpu'), None, 0, 1
    tr.mesh_model = _mesh_model(calls)
    tr.texture_mlp = tr.mesh_model.texture_mlp
    tr.train_views = [dict(theta=1.0, phi=v / 100.0, radius=1.5) for v in range(3)]
    tr.zero123plus, tr.zero123plus_prompt_embeds = types.SimpleNamespace(condition_encoder=None), None
    tr.define_view_weights = lambda view_ids=None: None
    tr.paint_viewpoint = lambda data, should_project_back=True, **k: (torch.full((1, 3, H, W), 0.5), torch.ones(1, 1, H, W))
    return tr


def test_active_builds_the_list_once_and_attaches_it(monkeypatch):
    calls = []
    tr = _sds_trainer(monkeypatch, calls, 'active')
    log = tr.paint_zero123plus(iterations=3, tile=8)
    assert len(log) == 3
    assert [c for c in calls if isinstance(c, str)] == ['mark', 'compact']                    # built once, before the loop
    fields = [c[1] for c in calls if not isinstance(c, str)]
    assert fields[0] is None and len(fields) == 4                                             # the set-up render is a fresh one: dense
    rc = tr._sds_setup['render_cache']
    want, _ = active_texels_np(rc['uv_features'].numpy(), rc['face_idx'].numpy(), T)
    assert rc['active_texels'].dtype == torch.int32 and np.array_equal(rc['active_texels'].numpy(), want)
    assert all(t is rc['active_texels'] for t in fields[1:])                                  # every iteration, the same tensor
    s = tr._sds_setup
    assert s['field_texels'] == 'active' and s['n_active'] == len(want) and s['active_fraction'] == len(want) / (T * T)
    assert 0 < s['active_fraction'] < 1


def test_all_calls_nothing_new(monkeypatch):
    calls = []
    tr = _sds_trainer(monkeypatch, calls, 'all')
    tr.paint_zero123plus(iterations=2, tile=8)
    assert [c for c in calls if isinstance(c, str)] == []
    assert [c[1] for c in calls] == [None] * 3
    assert 'active_texels' not in tr._sds_setup['render_cache'] and tr._sds_setup['field_texels'] == 'all'
    assert 'n_active' not in tr._sds_setup


def test_empty_active_set_stays_on_all(monkeypatch):
    calls = []
    tr = _sds_trainer(monkeypatch, calls, 'active', empty=True)
    tr.paint_zero123plus(iterations=2, tile=8)
    assert [c for c in calls if isinstance(c, str)] == ['mark', 'compact']
    assert [c[1] for c in calls if not isinstance(c, str)] == [None] * 3
    s = tr._sds_setup
    assert s['field_texels'] == 'all' and s['n_active'] == 0 and s['active_fraction'] == 0.0 and 'active_texels' not in s['render_cache']


def test_render_passes_the_list_only_with_its_cache():
    calls = []
    mm = _mesh_model(calls)
    gray = torch.full((3,), 0.5)
    out = mm.render(theta=[1.0, 1.0], phi=[0.0, 0.01], radius=[1.5, 1.5], background=gray)
    assert calls == [('field', None)] and 'active_texels' not in out['render_cache']
    rc = out['render_cache']
    mm.render(render_cache=rc, background=gray)
    assert calls[-1] == ('field', None)                                                       # a cache without a list: dense
    texels = torch.arange(5, dtype=torch.int32)
    rc['active_texels'] = texels
    out2 = mm.render(render_cache=rc, background=gray)
    assert calls[-1][1] is texels and out2['render_cache']['active_texels'] is texels        # the list stays with its raster
    mm.render(theta=[1.0], phi=[0.0], radius=[1.5], background=gray)
    assert calls[-1] == ('field', None)                                                       # a fresh render never sees one


def test_host_tensors_and_bad_lists_are_refused():
    from contexture_nerf_amd import _lib as L, kal
    with pytest.raises(L.CtxError, match="device tensor"):
        kal.active_texels(torch.zeros(1, 4, 4, 2), torch.zeros(1, 4, 4, dtype=torch.int64), 8)
    from contexture_nerf_amd.run_nerf_helpers import NeRF2D
    net = NeRF2D(D=2, W=64, input_ch=42, output_ch=3, skips=[0])
    with pytest.raises(L.CtxError, match="device tensor"):
        net.texture_map(8, texels=torch.arange(4, dtype=torch.int32))
