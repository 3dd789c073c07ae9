"""CPU: host-side mirrors (crop box, grid split/merge, pose lists, view direction, DreamTime table, scale helpers,
config surface, OBJ reader, sample_pdf / ndc_rays host logic) against the reference's own outputs in tests/golden."""
import os
import numpy as np
import pytest
import torch
from contexture_nerf_amd import utils as U, views_dataset as VD, config as CFG, kal
from contexture_nerf_amd import run_nerf_helpers as rnh
from contexture_nerf_amd.mesh import Mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_crop_boxes_and_grid(golden, golden_meta):
    for spec, box in zip(golden_meta['crop_specs'], golden_meta['crop_boxes']):
        h, w, y0, y1, x0, x1 = spec
        m = torch.zeros(h, w); m[y0:y1, x0:x1] = 1
        assert list(U.get_nonzero_region_tuple(m)) == box
    grid = torch.arange(1 * 4 * 120 * 80, dtype=torch.float32).reshape(1, 4, 120, 80)
    t = U.split_3x2_grid_to_tensor_with_6_elements(grid, 40)
    assert t.shape == (6, 4, 40, 40)
    np.testing.assert_allclose(t.reshape(6, -1).sum(1).numpy(), golden['grid_tiles_sum'])
    assert np.array_equal(t[:, 0, 0, 0].numpy(), golden['grid_tiles_corner'])
    assert torch.equal(U.merge_tensor_with_6_elements_to_3x2_grid(t, 40), grid)


def test_pose_lists_and_view_direction(golden, golden_meta):
    rc = CFG.RenderConfig()
    for name, cls in (('zero123plus', VD.Zero123PlusDataset), ('multiview', VD.MultiviewDataset)):
        rows = [{'dir': int(d['dir'][0]), 'theta': float(d['theta']), 'phi': float(d['phi']), 'radius': float(d['radius']),
                 'base_theta': float(d['base_theta'])} for d in cls(rc, 'cpu')]
        assert rows == golden_meta['views_' + name]
    d = U.get_view_direction(torch.tensor(golden['viewdir_theta']), torch.tensor(golden['viewdir_phi']), np.deg2rad(40.0), np.deg2rad(70.0))
    assert np.array_equal(d.numpy(), golden['viewdir'])


def test_dreamtime_and_scales(golden):
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2
    ds = U.DreamTimeScheduler(torch.cumprod(1.0 - betas, 0), 5000, m=500, s=125)
    assert [ds.get_t(int(i)) for i in golden['dreamtime_i']] == list(golden['dreamtime_t'])
    z = torch.tensor(golden['scale_in'])
    for fn in ('scale_latents', 'unscale_latents', 'scale_image', 'unscale_image'):
        np.testing.assert_allclose(getattr(U, fn)(z).numpy(), golden[fn], rtol=1e-6, atol=1e-7)


def test_config_defaults_and_cli(golden_meta, tmp_path):
    for cls, key in ((CFG.RenderConfig, 'cfg_render'), (CFG.OptimConfig, 'cfg_optim')):
        got = {k: v for k, v in vars(cls()).items()}
        for k, v in golden_meta[key].items():
            assert got[k] == v or list(map(list, got[k])) == v, (k, got[k], v)
    g = vars(CFG.GuideConfig())
    for k, v in golden_meta['cfg_guide'].items():
        if v != '<required>':
            assert str(g[k]) == str(v), (k, g[k], v)
    l = vars(CFG.LogConfig())
    for k, v in golden_meta['cfg_log'].items():
        if v != '<required>':
            assert str(l[k]).rstrip('/') == str(v).rstrip('/'), k
    cfg = CFG.parse(CFG.TrainConfig, [f'--config_path={ROOT}/configs/text_guided/nascar.yaml', '--optim.seed=5', '--guide.guidance_scale=7.5'])
    assert cfg.guide.shape_path == 'shapes/nascar.obj' and cfg.optim.seed == 5 and cfg.guide.guidance_scale == 7.5
    try:
        CFG.parse(CFG.TrainConfig, ['--guide.guidance_scale_crossattn=1'])
        assert False, "unknown key must raise like pyrallis does"
    except KeyError:
        pass
    CFG.dump(cfg, tmp_path / 'c.yaml')
    cfg2 = CFG.parse(CFG.TrainConfig, [f'--config_path={tmp_path}/c.yaml'])
    assert cfg2.guide.text == cfg.guide.text and cfg2.render.views_after == cfg.render.views_after


def test_mesh_normalise_and_obj_reader(golden, tmp_path):
    v = torch.tensor(golden['mesh_v']); f = torch.tensor(golden['mesh_f'])
    n, a = Mesh.calculate_face_normals(v, f)
    np.testing.assert_allclose(n.numpy(), golden['mesh_fn'], rtol=1e-6, atol=1e-7)
    m = Mesh(arrays=(golden['mesh_v'], golden['mesh_f'], np.zeros((0, 2), np.float32), np.zeros((0, 3), np.int64)))
    np.testing.assert_allclose(m.normalize_mesh(inplace=True, target_scale=0.6, dy=0.25).vertices.numpy(), golden['mesh_v_norm'], rtol=1e-6, atol=1e-6)
    p = tmp_path / 'q.obj'
    p.write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nf 1/1 2/2 3/3 4/4\nf -4//1 -3//1 -2//1\n")
    mm = kal.io.obj.import_mesh(str(p))
    assert mm.faces.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2]]
    assert mm.face_uvs_idx.tolist() == [[0, 1, 2], [0, 2, 3], [-1, -1, -1]]
    big = Mesh('shapes/nascar.obj', 'cpu')
    assert big.vertices.shape == (3750, 3) and big.faces.shape == (7500, 3)


def test_export_format_round_trip(tmp_path):
    """mesh.obj / mesh.mtl / albedo.png in the layout of the reference's export_mesh (textured_mesh.py:418-474): the OBJ reads
    back through the OBJ reader, the PNG decodes to the same pixels."""
    import zlib, struct
    from contexture_nerf_amd.mesh import write_textured_obj
    rng = np.random.default_rng(0)
    v = rng.standard_normal((5, 3)).astype(np.float32); f = np.array([[0, 1, 2], [2, 3, 4]])
    vt = rng.random((6, 2)).astype(np.float32); ft = np.array([[0, 1, 2], [3, 4, 5]])
    img = rng.integers(0, 256, (7, 9, 3)).astype(np.uint8)
    write_textured_obj(str(tmp_path), v, f, vt, ft, img)
    lines = (tmp_path / 'mesh.obj').read_text().splitlines()
    assert lines[0].strip() == 'mtllib mesh.mtl' and lines[1].startswith('v ') and 'usemtl mat0' in [l.strip() for l in lines]
    assert lines[-1].strip() == 'f 3/4 4/5 5/6'
    m = kal.io.obj.import_mesh(str(tmp_path / 'mesh.obj'))
    np.testing.assert_allclose(m.vertices.numpy(), v, rtol=1e-6)
    np.testing.assert_allclose(m.uvs.numpy(), vt, rtol=1e-6)
    assert m.faces.tolist() == f.tolist() and m.face_uvs_idx.tolist() == ft.tolist()
    assert 'map_Kd albedo.png' in (tmp_path / 'mesh.mtl').read_text()
    raw = (tmp_path / 'albedo.png').read_bytes()
    assert raw[:8] == b'\x89PNG\r\n\x1a\n'
    w, h = struct.unpack('>II', raw[16:24])
    assert (w, h) == (9, 7)
    i = raw.index(b'IDAT'); n = struct.unpack('>I', raw[i - 4:i])[0]
    px = np.frombuffer(zlib.decompress(raw[i + 4:i + 4 + n]), np.uint8).reshape(7, 1 + 27)[:, 1:].reshape(7, 9, 3)
    assert np.array_equal(px, img)


def test_euler_ancestral_scheduler_vs_oracle():
    """EulerAncestralDiscreteScheduler mirror (torch) vs the oracle's numpy restatement: schedule, input scaling, add_noise, epsilon and
    v-prediction steps with the same noise, and the explicit one-step schedule of the SDS loop.  (Both restate diffusers 0.27.2:
    parity unpinned, diffusers is absent offline.)"""
    from contexture_nerf_amd.scheduler import EulerAncestralDiscreteScheduler
    from oracle.scheduler import EulerAncestralRef
    rng = np.random.default_rng(0)
    for pt in ("v_prediction", "epsilon"):
        sch = EulerAncestralDiscreteScheduler(prediction_type=pt); ref = EulerAncestralRef(prediction_type=pt)
        sch.set_timesteps(7); ts = ref.set_timesteps(7)
        np.testing.assert_allclose(sch.timesteps.numpy(), ts, rtol=1e-6)
        np.testing.assert_allclose(sch.sigmas.numpy(), ref.sigmas, rtol=1e-5)
        assert abs(float(sch.init_noise_sigma) - ref.sigmas.max()) < 1e-4
        x = rng.standard_normal((1, 4, 6, 5)).astype(np.float32); out = rng.standard_normal((1, 4, 6, 5)).astype(np.float32)
        for i in (0, 3, 6):
            t = sch.timesteps[i]
            np.testing.assert_allclose(sch.scale_model_input(torch.tensor(x), t).numpy(), ref.scale(x, i), rtol=1e-5, atol=1e-6)
            g = torch.Generator().manual_seed(5)
            nz = torch.randn(x.shape, generator=torch.Generator().manual_seed(5)).numpy()
            got = sch.step(torch.tensor(out), t, torch.tensor(x), generator=g)['prev_sample'].numpy()
            np.testing.assert_allclose(got, ref.step(out, i, x, nz), rtol=2e-5, atol=2e-5)
        np.testing.assert_allclose(sch.add_noise(torch.tensor(x), torch.tensor(out), sch.timesteps[2:3]).numpy(), x + out * ref.sigmas[2], rtol=1e-5, atol=1e-6)
        sch.set_timesteps(1, timesteps=[515.0]); ref.set_timesteps(timesteps=[515.0])          # one SDS step at a DreamTime t
        assert sch.timesteps.tolist() == [515.0] and abs(float(sch.sigmas[0]) - ref.sigmas[0]) < 1e-5 and float(sch.sigmas[1]) == 0.0
        with pytest.raises(ValueError):
            sch.scale_model_input(torch.tensor(x), 100.0)


def test_depth_grid_and_to_rgb_image_vs_pil():
    """sds.to_rgb_image / build_depth_grid against the reference's formulation run through PIL itself (trainer.py:533-543, 575-600:
    to_pil_image -> paste over grey 127 with the alpha channel): bit-exact on the 8-bit values."""
    from PIL import Image
    from contexture_nerf_amd import sds
    g = torch.Generator().manual_seed(0)
    rgba = torch.rand(1, 4, 37, 29, generator=g)
    rgba[:, 3, :10] = 0.0; rgba[:, 3, 10:20] = 1.0
    got = (sds.to_rgb_image(rgba)[0] * 255).round().to(torch.uint8).permute(1, 2, 0).numpy()
    pil = Image.fromarray((rgba[0].mul(255).byte().permute(1, 2, 0).numpy()), 'RGBA')
    bg = Image.fromarray(np.full((37, 29, 3), 127, np.uint8), 'RGB')
    bg.paste(pil, mask=pil.getchannel('A'))
    assert np.array_equal(got, np.asarray(bg))
    # grid: 7 views, tiles of views 1..6 at positions (row, col) = (k % 3, k // 3)
    depth = torch.rand(7, 1, 48, 48, generator=g)
    mask = torch.zeros(7, 1, 48, 48); mask[:, :, 8:40, 12:36] = 1.0
    grid = sds.build_depth_grid(depth, mask, size=16)
    assert grid.shape == (1, 3, 48, 32)
    from contexture_nerf_amd.utils import get_nonzero_region_tuple
    for k in range(6):
        h0, w0, h1, w1 = get_nonzero_region_tuple(mask[k + 1, 0])
        tile = torch.nn.functional.interpolate(torch.cat([depth[k + 1:k + 2]] * 3 + [mask[k + 1:k + 2]], 1)[:, :, h0:h1, w0:w1], (16, 16),
                                               mode='bilinear', align_corners=False)
        r, c = k % 3, k // 3
        assert torch.equal(grid[:, :, 16 * r:16 * r + 16, 16 * c:16 * c + 16], sds.to_rgb_image(tile))


def test_grid_layout_latent_distribution_and_depth_convention():
    """host pieces of this round: the 3x2 grid layout equals the reference's explicit cat (trainer.py:722-727: rows (0,3), (1,4),
    (2,5)); DiagonalGaussianDistribution (diffusers 0.27.2 semantics: clamp(logvar,-30,20), mean + std * noise); the ray path's depth
    convention (foreground 0.5..1 with closer = larger, background 0); contiguous row tiles."""
    from contexture_nerf_amd import sds, volume_render as vr
    from contexture_nerf_amd.vae import DiagonalGaussianDistribution
    g = torch.Generator().manual_seed(0)
    six = torch.rand(6, 3, 5, 5, generator=g)
    want = torch.cat((torch.cat((six[0:1], six[3:4]), dim=3), torch.cat((six[1:2], six[4:5]), dim=3), torch.cat((six[2:3], six[5:6]), dim=3)), dim=2)
    assert torch.equal(sds.views_to_grid(six, 5), want)
    mom = torch.randn(2, 8, 3, 3, generator=g) * 20
    d = DiagonalGaussianDistribution(mom)
    assert float(d.logvar.max()) <= 20 and float(d.logvar.min()) >= -30 and torch.equal(d.mode(), mom[:, :4])
    s1 = d.sample(generator=torch.Generator().manual_seed(3))
    n = torch.randn(d.mean.shape, generator=torch.Generator().manual_seed(3))
    assert torch.allclose(s1, d.mean + torch.exp(0.5 * d.logvar) * n)
    depth = torch.tensor([[2.0, 1.0], [3.0, 9.0]]); acc = torch.tensor([[0.9, 0.8], [0.7, 0.1]])
    dm = vr.depth_for_diffusion(depth, acc)
    assert dm[1, 1] == 0 and dm[0, 1] == 1.0 and dm[1, 0] == 0.5 and abs(float(dm[0, 0]) - 0.75) < 1e-6
    spans = [vr.shard_rows(13, r, 4) for r in range(4)]
    assert spans == [(0, 4), (4, 7), (7, 10), (10, 13)]
    assert vr.pinhole(512, 512)[0, 0] == np.float32(256 / np.tan(np.pi / 6))


def test_sampling_host_logic(golden):
    s = rnh.sample_pdf(torch.tensor(golden['pdf_bins']), torch.tensor(golden['pdf_w']), 24, det=True)
    np.testing.assert_allclose(s.numpy(), golden['pdf_det'], rtol=1e-6, atol=1e-6)
    s = rnh.sample_pdf(torch.tensor(golden['pdf_bins']), torch.tensor(golden['pdf_w']), 24, det=False, pytest=True)
    np.testing.assert_allclose(s.numpy(), golden['pdf_pytest'], rtol=1e-6, atol=1e-6)
    no, nd = rnh.ndc_rays(6, 8, 5.0, 1.0, torch.tensor(golden['rays_o']), torch.tensor(golden['rays_d']))
    np.testing.assert_allclose(no.numpy(), golden['ndc_o'], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(nd.numpy(), golden['ndc_d'], rtol=1e-6, atol=1e-6)


def test_product_camera_path_vs_oracle_and_geometry():
    """The PRODUCT's camera chain — Renderer.get_camera_from_multiple_view / get_camera_from_view ->
    kal.generate_transformation_matrix, kal.generate_perspective_projection (src/models/render.py:8-46) — fed with theta / phi / r
    of the 7 Zero123++ and 10 Multiview poses, against oracle/geometry.py's restatement AND against what a look-at camera must
    do whatever the formulas are (eye -> origin, look-at point -> -z axis at the eye distance, world up stays in the +y half
    plane, orthonormal right-handed rotation): a sign or axis slip in either restatement fails the second half."""
    from contexture_nerf_amd.render import Renderer
    from oracle import geometry as og
    rc = CFG.RenderConfig()
    dy = 0.25
    for cls in (VD.Zero123PlusDataset, VD.MultiviewDataset):
        views = list(cls(rc, 'cpu'))
        assert len(views) in (7, 10)
        th = torch.tensor([float(v['theta']) for v in views]); ph = torch.tensor([float(v['phi']) for v in views])
        r = torch.tensor([float(v['radius']) for v in views])
        M = Renderer.get_camera_from_multiple_view(th, ph, r, look_at_height=dy)                      # [B,4,3]
        want = og.get_camera_from_multiple_view(th.numpy(), ph.numpy(), r.numpy(), dy)
        assert M.shape == (len(views), 4, 3)
        np.testing.assert_allclose(M.numpy(), want, rtol=0, atol=2e-6)
        for k in range(len(views)):                                                                   # single-view twin
            M1 = Renderer.get_camera_from_view(th[k], ph[k], r=r[k], look_at_height=0.0)
            w1 = og.get_camera_from_multiple_view(th[k:k + 1].numpy(), ph[k:k + 1].numpy(), r[k:k + 1].numpy(), 0.0)
            np.testing.assert_allclose(M1.numpy(), w1, rtol=0, atol=2e-6)
        R, t = M[:, :3, :].double(), M[:, 3, :].double()
        eye = torch.stack([r * torch.sin(th) * torch.sin(ph), r * torch.cos(th), r * torch.sin(th) * torch.cos(ph)], 1).double()
        look = torch.zeros_like(eye); look[:, 1] = dy
        to_cam = lambda p: torch.einsum('bi,bij->bj', p, R) + t                                       # [v,1] @ M as kaolin applies it
        assert to_cam(eye).abs().max() < 1e-5
        lc = to_cam(look)
        dist = (eye - look).norm(dim=1)
        assert lc[:, :2].abs().max() < 1e-5 and torch.allclose(lc[:, 2], -dist, atol=1e-5)            # camera looks down -z
        upc = to_cam(eye + torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64))
        assert (upc[:, 1] > 0).all() and upc[:, 0].abs().max() < 1e-5                                 # world up -> image up, no roll
        eye3 = torch.eye(3, dtype=torch.float64).expand(len(views), 3, 3)
        assert (R.transpose(1, 2) @ R - eye3).abs().max() < 1e-5 and torch.allclose(torch.linalg.det(R), torch.ones(len(views), dtype=torch.float64), atol=1e-5)
    P = kal.render.camera.generate_perspective_projection(np.pi / 3)
    assert P.shape == (3, 1) and P.dtype == torch.float32
    np.testing.assert_array_equal(P.numpy(), og.generate_perspective_projection(np.pi / 3))
    np.testing.assert_allclose(P[:, 0].numpy(), [1 / np.tan(np.pi / 6), 1 / np.tan(np.pi / 6), -1.0], rtol=1e-6)
    assert Renderer('cpu', dim=(8, 8)).camera_projection.shape == (3, 1)


def test_text_embedding_seed_is_stable_across_interpreters():
    """The stand-in text embedding must be the same in every process (ranks under torchrun, reruns): its seed comes from a
    SHA-256 digest of the prompt, not from hash() (str hashing is randomised per interpreter)."""
    import subprocess, sys
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import hashlib, inspect\n"
            "from contexture_nerf_amd import stable_diffusion_depth as S\n"
            "src = inspect.getsource(S.StableDiffusion.get_text_embeds)\n"
            "assert 'hash((' not in src and 'sha256' in src\n"
            "import torch, types\n"
            "sd = S.StableDiffusion.__new__(S.StableDiffusion); sd.text_encoder = None; sd.device = 'cpu'\n"
            "sd.unet = types.SimpleNamespace(config={'cross_attention_dim': 32})\n"
            "z = sd.get_text_embeds(['a photo of a nascar, front view'])\n"
            "print(hashlib.sha256(z.numpy().tobytes()).hexdigest())\n") % ROOT
    outs = []
    for seed in ('1', '2'):
        env = dict(os.environ, PYTHONHASHSEED=seed)
        outs.append(subprocess.check_output([sys.executable, '-c', code], env=env).decode().strip())
    assert outs[0] == outs[1] and len(outs[0]) == 64


def test_ddpm_scheduler_step_identities():
    """DDPMScheduler mirror (the pipeline scheduler the reference swaps in, trainer.py:306): one explicit timestep as the SDS loop
    calls it; with the TRUE v (or epsilon) as model output the step's pred_original_sample is x0; init_noise_sigma is 1; the
    final step (prev_t < 0) returns x0 itself."""
    from contexture_nerf_amd.scheduler import DDPMScheduler
    g = torch.Generator().manual_seed(0)
    x0, eps = torch.randn(1, 4, 6, 4, generator=g), torch.randn(1, 4, 6, 4, generator=g)
    for pt in ("v_prediction", "epsilon"):
        sch = DDPMScheduler(prediction_type=pt, clip_sample=False)
        assert sch.init_noise_sigma == 1.0
        sch.set_timesteps(1, timesteps=[515.0])
        assert sch.timesteps.tolist() == [515] and sch.previous_timestep(515) == -1
        t = torch.tensor([515])
        ac = float(sch.alphas_cumprod[515])
        xt = sch.add_noise(x0, eps, t)
        assert torch.allclose(xt, ac ** 0.5 * x0 + (1 - ac) ** 0.5 * eps, atol=1e-6)
        out = ac ** 0.5 * eps - (1 - ac) ** 0.5 * x0 if pt == "v_prediction" else eps
        assert torch.equal(sch.scale_model_input(xt, t), xt)
        r = sch.step(out, t, xt, generator=torch.Generator().manual_seed(1))
        assert torch.allclose(r['pred_original_sample'], x0, atol=2e-5)
        sch.set_timesteps(1, timesteps=[0.0])
        r0 = sch.step(eps if pt == "epsilon" else float(sch.alphas_cumprod[0]) ** 0.5 * eps - (1 - float(sch.alphas_cumprod[0])) ** 0.5 * x0,
                      torch.tensor([0]), sch.add_noise(x0, eps, torch.tensor([0])))
        assert torch.allclose(r0['prev_sample'], x0, atol=2e-4)
    with pytest.raises(ValueError):
        DDPMScheduler().set_timesteps(2, timesteps=[10.0, 20.0])
    # the defaults `DDPMScheduler.from_config(<EulerAncestral config>)` yields (no clip_sample key there): clip to [-1, 1]
    sch = DDPMScheduler()
    assert sch.clip_sample and sch.clip_sample_range == 1.0
    sch.set_timesteps(1, timesteps=[515.0])
    ac = float(sch.alphas_cumprod[515]); t = torch.tensor([515])
    big = 3 * x0
    xt = sch.add_noise(big, eps, t)
    r = sch.step(ac ** 0.5 * eps - (1 - ac) ** 0.5 * big, t, xt, generator=torch.Generator().manual_seed(1))
    assert torch.allclose(r['pred_original_sample'], big.clamp(-1, 1), atol=5e-5) and float(r['pred_original_sample'].abs().max()) <= 1.0


def test_safetensors_reader_writer(tmp_path):
    """contexture_nerf_amd.safetensors_io: round trip on a file this test writes (fp32 / fp16 / bf16 / int64, a 0-d and an empty
    tensor), agreement with the `safetensors` package in both directions where it is importable, and loud failures on a
    truncated file, an oversized header, offsets that do not match the shape, and a non-JSON header."""
    import json, struct
    from contexture_nerf_amd import safetensors_io as sio
    g = torch.Generator().manual_seed(0)
    sd = {"conv_in.weight": torch.randn(8, 5, 3, 3, generator=g), "b.half": torch.randn(7, generator=g).half(),
          "c.bf16": torch.randn(3, 2, generator=g).bfloat16(), "d.idx": torch.arange(6).reshape(2, 3), "e.scalar": torch.tensor(2.5),
          "f.empty": torch.zeros(0, 4)}
    path = str(tmp_path / "m.safetensors")
    sio.save_file(sd, path, metadata={"format": "pt"})
    hdr, meta, off = sio.read_header(path)
    assert set(hdr) == set(sd) and meta == {"format": "pt"} and off % 8 == 0
    got = sio.load_file(path)
    for k, v in sd.items():
        assert got[k].dtype == v.dtype and got[k].shape == v.shape and torch.equal(got[k], v), k
    assert set(sio.load_file(path, names={"b.half"})) == {"b.half"}
    try:
        from safetensors.torch import load_file as st_load, save_file as st_save
    except ImportError:
        st_load = None
    if st_load is not None:
        theirs = st_load(path)
        assert all(torch.equal(theirs[k], v) for k, v in sd.items())
        p2 = str(tmp_path / "theirs.safetensors")
        st_save({k: v.contiguous() for k, v in sd.items()}, p2)
        ours = sio.load_file(p2)
        assert all(torch.equal(ours[k], v) for k, v in sd.items())
    raw = open(path, "rb").read()
    bad = tmp_path / "bad.safetensors"
    for blob, what in ((raw[:5], "shorter"), (struct.pack("<Q", 1 << 40) + raw[8:], "header length"),
                       (struct.pack("<Q", 4) + b"nope" + raw[8:], "not JSON"), (raw[:-9], "claims bytes")):
        bad.write_bytes(blob)
        with pytest.raises(sio.SafetensorsError, match=what):
            sio.load_file(str(bad))
    n = struct.unpack("<Q", raw[:8])[0]
    h = json.loads(raw[8:8 + n]); h["d.idx"]["shape"] = [2, 4]
    js = json.dumps(h).encode(); bad.write_bytes(struct.pack("<Q", len(js)) + js + raw[8 + n:])
    with pytest.raises(sio.SafetensorsError, match="claims bytes"):
        sio.load_file(str(bad))


def test_clip_text_path_from_local_directory(tmp_path):
    """get_text_embeds through the reference's own text path (CLIPTokenizer + CLIPTextModel, stable_diffusion_depth.py:222-244) when
    `model_name` is a local diffusers-layout directory: a tiny random CLIP text model and a toy BPE vocabulary written by this test.
    -> cat([uncond, cond]) of shape [2, max_length, hidden]; the unconditional half is the encoding of ''."""
    import json
    from transformers import CLIPTextConfig, CLIPTextModel, CLIPTokenizer
    from contexture_nerf_amd.stable_diffusion_depth import StableDiffusion
    tokd, encd = tmp_path / "tokenizer", tmp_path / "text_encoder"
    tokd.mkdir(); encd.mkdir()
    letters = list("abcdefghijklmnopqrstuvwxyz")
    vocab = {}
    for ch in letters:
        vocab[ch] = len(vocab)
    for ch in letters:
        vocab[ch + "</w>"] = len(vocab)
    vocab["<|startoftext|>"] = len(vocab); vocab["<|endoftext|>"] = len(vocab)
    (tokd / "vocab.json").write_text(json.dumps(vocab))
    (tokd / "merges.txt").write_text("#version: 0.2\n")
    tok = CLIPTokenizer(str(tokd / "vocab.json"), str(tokd / "merges.txt"), model_max_length=12)
    tok.save_pretrained(str(tokd))
    torch.manual_seed(0)
    cfg = CLIPTextConfig(vocab_size=len(vocab), hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2,
                         max_position_embeddings=12, bos_token_id=vocab["<|startoftext|>"], eos_token_id=vocab["<|endoftext|>"], pad_token_id=vocab["<|endoftext|>"])
    CLIPTextModel(cfg).save_pretrained(str(encd))
    import types
    sd = StableDiffusion.__new__(StableDiffusion)
    # run only the text part of __init__ (the engines need a GPU): replicate its local-directory branch
    sd.device, sd.text_encoder, sd.tokenizer = 'cpu', None, None
    sd.unet = types.SimpleNamespace(config={'cross_attention_dim': 32})
    from transformers import CLIPTextModel as M, CLIPTokenizer as T
    sd.tokenizer = T.from_pretrained(str(tokd), local_files_only=True)
    sd._clip = M.from_pretrained(str(encd), local_files_only=True).eval()
    sd.text_encoder = sd._clip_embeds
    z = sd.get_text_embeds(["a car"])
    assert z.shape == (2, 12, 32) and torch.isfinite(z).all()
    z2 = sd.get_text_embeds(["a car"], negative_prompt=[""])
    assert torch.equal(z, z2)
    zz = sd.get_text_embeds(["a bus"])
    assert torch.equal(zz[0], z[0]) and not torch.equal(zz[1], z[1])


def test_all_twelve_experiment_yamls_load_or_fail_like_the_reference():
    """configs/text_guided/*.yaml: the reference's 12 experiment files as loader fixtures.  beachball / mickey carry
    keys GuideConfig does not have -> the loader refuses them (pyrallis raises a parse error there); every other file loads with
    its values; files with append_direction: True under use_zero123plus (the default) then abort in calc_text_embeddings with the
    reference's assert (src/training/trainer.py:320); the rest produce the [prompt, prompt + ", front view"] pair."""
    import glob
    import types
    from contexture_nerf_amd import config as CFG
    from contexture_nerf_amd.trainer import ConTEXTure
    files = sorted(glob.glob(os.path.join(ROOT, "configs", "text_guided", "*.yaml")))
    assert len(files) == 12
    unknown_keys = {"beachball.yaml", "mickey.yaml"}
    aborts = {"napoleon_zero123plus_weight_mask.yaml", "nascar_zero123plus.yaml", "spiderman_zero123plus_weight_mask.yaml"}
    seen = []

    def stub_embeds(prompt, negative_prompt=None):
        seen.append((tuple(prompt), negative_prompt))
        return torch.zeros(2, 77, 8)
    for f in files:
        name = os.path.basename(f)
        if name in unknown_keys:
            with pytest.raises(KeyError, match="guidance_scale_crossattn"):
                CFG.parse(CFG.TrainConfig, [f"--config_path={f}"])
            continue
        cfg = CFG.parse(CFG.TrainConfig, [f"--config_path={f}"])
        assert cfg.log.exp_name and cfg.guide.text and cfg.guide.use_zero123plus is True
        tr = ConTEXTure.__new__(ConTEXTure)
        tr.cfg, tr.diffusion = cfg, types.SimpleNamespace(get_text_embeds=stub_embeds)
        tr.view_dirs = ['front', 'left', 'back', 'right', 'overhead', 'bottom']
        seen.clear()
        if name in aborts:
            assert cfg.guide.append_direction is True
            with pytest.raises(AssertionError, match="append_direction should be False when use_zero123plus is True"):
                tr.calc_text_embeddings()
            assert not seen
            # the same file with the Zero123++ flag off takes the per-direction branch: six prompts through text.format(dir)
            cfg.guide.use_zero123plus = False
            tz, ts = tr.calc_text_embeddings()
            assert len(tz) == 6 and ts[1] == cfg.guide.text.format('left') and "{}" not in ts[0]
        else:
            tz, ts = tr.calc_text_embeddings()
            assert ts == [cfg.guide.text, cfg.guide.text + ", front view"] and len(tz) == 2
            assert [s[0] for s in seen] == [(ts[0],), (ts[1],)] and all(s[1] is None for s in seen)
            tr.text_z, tr.text_string = tz, ts
            assert tr._text_for(dict(dir=torch.tensor([2]))) is tz[1]          # trainer.py:1019-1022: the ", front view" embedding
    cfg = CFG.parse(CFG.TrainConfig, [f"--config_path={os.path.join(ROOT, 'configs', 'text_guided', 'spiderman.yaml')}", "--optim.seed=7"])
    assert cfg.optim.alpha == -100 and cfg.optim.seed == 7 and cfg.guide.shape_path == "shapes/human.obj"


def test_zero123plus_condition_encoder_from_local_directory(tmp_path):
    """The condition path of the Zero123++ pipeline (src/zero123plus.py:772-803) read from a LOCAL directory in the pipeline's layout:
    feature_extractor_clip -> vision_encoder(...).image_embeds -> global_embeds, added with model_index.json's ramping_coefficients to
    encode_prompt("").  A tiny CLIP vision / text pair and processor written by this test; checked against the same transformers
    modules called by hand, incl. the processor's resize / centre crop / normalisation."""
    import json
    from transformers import (CLIPImageProcessor, CLIPVisionConfig, CLIPVisionModelWithProjection, CLIPTextConfig, CLIPTextModel,
                              CLIPTokenizer)
    from contexture_nerf_amd.zero123plus import ConditionEncoder
    from contexture_nerf_amd import _lib as L
    d = tmp_path / "zero123plus"
    for sub in ("feature_extractor_clip", "vision_encoder", "tokenizer", "text_encoder"):
        (d / sub).mkdir(parents=True)
    CLIPImageProcessor(size={"shortest_edge": 32}, crop_size={"height": 32, "width": 32}).save_pretrained(str(d / "feature_extractor_clip"))
    torch.manual_seed(0)
    CLIPVisionModelWithProjection(CLIPVisionConfig(hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2,
                                                   image_size=32, patch_size=8, projection_dim=16)).save_pretrained(str(d / "vision_encoder"))
    letters = list("abcdefghijklmnopqrstuvwxyz")
    vocab = {ch: i for i, ch in enumerate(letters)}
    for ch in letters:
        vocab[ch + "</w>"] = len(vocab)
    vocab["<|startoftext|>"] = len(vocab); vocab["<|endoftext|>"] = len(vocab)
    (d / "tokenizer" / "vocab.json").write_text(json.dumps(vocab))
    (d / "tokenizer" / "merges.txt").write_text("#version: 0.2\n")
    CLIPTokenizer(str(d / "tokenizer" / "vocab.json"), str(d / "tokenizer" / "merges.txt"), model_max_length=12).save_pretrained(str(d / "tokenizer"))
    CLIPTextModel(CLIPTextConfig(vocab_size=len(vocab), hidden_size=16, intermediate_size=32, num_hidden_layers=2, num_attention_heads=2,
                                 max_position_embeddings=12, bos_token_id=vocab["<|startoftext|>"], eos_token_id=vocab["<|endoftext|>"],
                                 pad_token_id=vocab["<|endoftext|>"])).save_pretrained(str(d / "text_encoder"))
    ramp = [round(0.1 * i, 3) for i in range(12)]
    (d / "model_index.json").write_text(json.dumps({"_class_name": "Zero123PlusPipeline", "ramping_coefficients": ramp}))
    ce = ConditionEncoder(str(d), device='cpu')
    assert ce.ramping_coefficients == ramp
    g = torch.Generator().manual_seed(1)
    img = torch.rand(1, 3, 80, 64, generator=g)
    ge = ce.global_embeds(img)
    assert ge.shape == (1, 1, 16) and torch.isfinite(ge).all()
    # by hand: the processor on the same 8-bit pixels, then the vision tower
    arr = (img[0] * 255).round().to(torch.uint8).permute(1, 2, 0).numpy()
    pv = CLIPImageProcessor.from_pretrained(str(d / "feature_extractor_clip"))(images=arr, return_tensors='pt').pixel_values
    assert pv.shape == (1, 3, 32, 32)
    want = CLIPVisionModelWithProjection.from_pretrained(str(d / "vision_encoder")).eval()(pv).image_embeds
    assert torch.allclose(ge[:, 0], want, atol=1e-6)
    e0 = ce.encode_prompt("")
    assert e0.shape == (1, 12, 16)
    pe, neg = ce.prompt_embeds(img, "")
    assert torch.equal(neg, e0)
    assert torch.allclose(pe, e0 + ge * torch.tensor(ramp).unsqueeze(-1), atol=1e-6)
    assert torch.equal(pe[:, 0], e0[:, 0]) and not torch.equal(pe[:, 5], e0[:, 5])      # ramp[0] == 0: the first token is untouched
    with pytest.raises(L.CtxError, match="feature_extractor_clip"):
        ConditionEncoder(str(tmp_path / "nowhere"))
    (d / "model_index.json").write_text(json.dumps({"ramping_coefficients": ramp[:5]}))
    with pytest.raises(L.CtxError, match="ramping coefficients"):
        ConditionEncoder(str(d)).prompt_embeds(img)


@pytest.mark.parametrize("name", ["nascar", "bunny", "blub_no_texture"])
def test_chart_atlas_generator(meshes, name):
    """atlas.chart_atlas, the stand-in for the reference's xatlas call (src/models/textured_mesh.py:392-404), on the bundled meshes
    without UVs: every face owns a non-degenerate, consistently oriented triangle inside [0,1]^2; no texel centre of the 1024^2
    atlas is claimed by two faces; >= 0.6 of the texels are used; neighbours on a smooth surface share their UV edge (far fewer
    seam edges than faces); bounded stretch; deterministic."""
    from contexture_nerf_amd.atlas import chart_atlas, rasterize_uv_counts
    v, f = meshes[name + '_v'], meshes[name + '_f'].astype(np.int64)
    vt, ft, info = chart_atlas(v, f, resolution=1024, gutter=2, return_info=True)
    F = f.shape[0]
    assert vt.dtype == np.float32 and ft.shape == (F, 3) and ft.min() == 0 and ft.max() == vt.shape[0] - 1
    assert vt.min() >= 0.0 and vt.max() <= 1.0
    p = vt[ft].astype(np.float64)
    area2 = (p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 2, 0] - p[:, 0, 0]) * (p[:, 1, 1] - p[:, 0, 1])
    e0, e1 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    a3 = np.linalg.norm(np.cross(e0, e1), axis=1)
    assert (np.abs(area2[a3 > 1e-12]) > 0).all()
    # 2-D area / 3-D area = texel density^2 * cos(angle to the chart plane): within [cos(50 deg), 1] of the global density
    ratio = np.abs(area2) * 1024 ** 2 / np.maximum(a3, 1e-30) / info['texels_per_unit'] ** 2
    ok = a3 > 1e-10
    assert ratio[ok].max() <= 1.0 + 1e-2 and ratio[ok].min() >= np.cos(np.deg2rad(50.0)) - 1e-2        # vt is float32
    cnt, _ = rasterize_uv_counts(vt, ft, 1024)
    assert int(cnt.max()) == 1 and info['overlap_texels'] == 0
    used = float((cnt > 0).mean())
    assert used >= 0.6 and abs(used - info['utilisation']) < 1e-4, used
    assert info['seam_edges'] < 0.2 * (info['seam_edges'] + info['interior_edges']) and info['charts'] < F // 20
    print(f"{name}: {info}")
    if name == "bunny":                                                       # deterministic (checked on the quickest mesh)
        vt2, ft2 = chart_atlas(v, f, resolution=1024, gutter=2)
        assert np.array_equal(vt, vt2) and np.array_equal(ft, ft2)


def test_mjpeg_avi_muxer_round_trip(tmp_path):
    """video.py: the orbit video of `evaluate(save_as_video=True)` (the reference's imageio mp4, trainer.py:943-950) as a Motion-JPEG AVI:
    RIFF structure (sizes, stream header, index), frame count, frame rate, and the frames back within JPEG error; bad input fails loudly."""
    import struct
    from contexture_nerf_amd.video import write_mjpeg_avi, read_mjpeg_avi
    rng = np.random.default_rng(0)
    base = (np.linspace(0, 255, 80)[None, :, None] * np.ones((60, 1, 3))).astype(np.uint8)
    frames = []
    for i in range(9):
        f = base.copy(); f[10 + 3 * i:20 + 3 * i, 8:30] = (255, 32, 0); frames.append(f)
    path = tmp_path / "orbit.avi"
    assert write_mjpeg_avi(path, frames, fps=25) == 9
    d = open(path, "rb").read()
    assert d[:4] == b"RIFF" and struct.unpack_from("<I", d, 4)[0] == len(d) - 8 and d[8:12] == b"AVI "
    avih = d.index(b"avih")
    usec, _, _, flags, nframes, _, streams, _, w, h = struct.unpack_from("<10I", d, avih + 8)
    assert (usec, nframes, streams, w, h) == (40000, 9, 1, 80, 60) and flags & 0x10
    assert d[d.index(b"strh") + 8:d.index(b"strh") + 16] == b"vidsMJPG"
    assert d.count(b"00dc") == 18                                   # nine chunks + nine index entries
    fps, back = read_mjpeg_avi(path)
    assert fps == 25 and len(back) == 9
    for a, b in zip(frames, back):
        assert b.shape == a.shape and np.abs(a.astype(int) - b.astype(int)).mean() < 4.0
    with pytest.raises(ValueError):
        write_mjpeg_avi(tmp_path / "bad.avi", [np.zeros((4, 4), np.uint8)])
    with pytest.raises(ValueError):
        write_mjpeg_avi(tmp_path / "bad.avi", [np.zeros((4, 4, 3), np.uint8), np.zeros((5, 4, 3), np.uint8)])
    with pytest.raises(ValueError):
        write_mjpeg_avi(tmp_path / "bad.avi", [])


def test_plan_waves_pins_the_multi_view_schedule():
    """stable_diffusion_depth.plan_waves: the one place that decides how a rank denoises its views (waves of concurrent groups;
    a group = one UNet batch of 2 x len(group)).  A view's bits depend on the size of its group, so these partitions are the
    ones the atlases of bench.py and tools/ were recorded with."""
    from contexture_nerf_amd.stable_diffusion_depth import plan_waves
    g = lambda a, b: list(range(a, b))
    assert plan_waves(6, 6, 3) == [[g(0, 6)]]                                       # bench.py --mode mesh --per-eval 6
    w = plan_waves(48, 6, 3, groups_in_flight=2)                                    # configs[3] on one rank
    assert w == [[g(12 * i, 12 * i + 6), g(12 * i + 6, 12 * i + 12)] for i in range(4)]
    assert plan_waves(6, 0, 3) == [[[0], [1], [2]], [[3], [4], [5]]]
    assert plan_waves(6, 1, 3) == plan_waves(6, 0, 3)
    assert plan_waves(5, 3, 3) == [[[0, 1, 2]], [[3], [4]]]                          # left-overs: single views, all in flight
    assert plan_waves(14, 6, 3) == [[g(0, 6), g(6, 12)], [[12], [13]]]
    assert plan_waves(20, 6, 3) == [[g(0, 6), g(6, 12)], [g(12, 18)], [[18], [19]]]
    assert plan_waves(2, 3, 3) == [[[0], [1]]]
    assert plan_waves(48, 6, 3, groups_in_flight=1) == [[g(6 * i, 6 * i + 6)] for i in range(8)]
    assert plan_waves(9, 9, 4) == [[[0], [1], [2], [3]], [[4], [5], [6], [7]], [[8]]]   # views_per_eval 9: not batched
    assert plan_waves(16, 8, 3) == [[g(0, 8), g(8, 16)]]                                # 8: batch 16, the largest batched
    assert plan_waves(7, 6, 2, batchable=False) == [[[0], [1]], [[2], [3]], [[4], [5]], [[6]]]
    assert plan_waves(0, 6, 3) == [] and plan_waves(3, 0, 0) == [[[0]], [[1]], [[2]]]
    # a paint loop hands the runner one wave at a time, and the runner re-plans it: every wave must plan to itself
    for n in range(0, 30):
        for vpe in (0, 1, 2, 3, 6, 8, 9):
            for infl in (1, 2, 3):
                waves = plan_waves(n, vpe, infl)
                assert sorted(k for w in waves for grp in w for k in grp) == list(range(n))
                for w in waves:
                    k0 = w[0][0]
                    assert plan_waves(sum(map(len, w)), vpe, infl) == [[[k - k0 for k in grp] for grp in w]]
