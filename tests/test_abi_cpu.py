"""CPU: the C-ABI library loads and exports every symbol include/ctx_nerf.h declares (no compute calls),
the ctypes table mirrors the header, and the host-only parts of the ABI (UNet parameter table, size queries)
agree with the oracle's module graph."""
import ctypes as C
import os
import re
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_functions():
    src = open(os.path.join(ROOT, "include", "ctx_nerf.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ctx_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from contexture_nerf_amd import _lib as L
    assert os.environ.get("CTX_ALLOW_PARTIAL") != "1"
    lib = L.load()
    names = _header_functions()
    assert len(names) >= 40
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/ctx_nerf.h but not exported"
        assert n in L.SIGNATURES, f"{n} has no ctypes signature"
    for n in L.SIGNATURES:
        assert n in names, f"{n} bound in _lib.py but not declared in the header"
    assert lib.ctx_version() >= 100


def test_product_fails_loudly_without_device_tensors():
    from contexture_nerf_amd import _lib as L, kal
    with pytest.raises(L.CtxError, match="device tensor"):
        kal.render.mesh.rasterize(8, 8, torch.zeros(1, 1, 3), torch.zeros(1, 1, 3, 2), torch.zeros(1, 1, 3, 1))


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "contexture-nerf_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            code = re.sub(r'""".*?"""', "", src, flags=re.S)       # prose may name the oracle; code may not
            code = "\n".join(l.split("#")[0] for l in code.splitlines())
            assert "oracle" not in code, f"{fn} references the oracle"


def test_unet_param_table_matches_diffusers_naming():
    from contexture_nerf_amd.unet import UNet2DConditionModel, SD2_DEPTH
    from oracle import unet_ref
    for cfg in (unet_ref.tiny_config(), unet_ref.tiny_config(ch=(64, 128, 256, 256), heads=(1, 2, 4, 4), ctx_dim=128)):
        net = UNet2DConditionModel(cfg, device="cpu", init=False)
        ref = unet_ref.UNet2DConditionModelRef(cfg)
        assert net.param_shapes() == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    net = UNet2DConditionModel(SD2_DEPTH, device="cpu", init=False)
    assert net.in_channels == 5
    assert 865e6 < net.num_parameters() < 867e6
    shapes = net.param_shapes()
    assert shapes["conv_in.weight"] == (320, 5, 3, 3)
    assert shapes["up_blocks.1.resnets.2.conv1.weight"] == (1280, 1920, 3, 3)
    assert shapes["down_blocks.0.attentions.0.transformer_blocks.0.attn2.to_k.weight"] == (320, 1024)
    assert shapes["mid_block.attentions.0.transformer_blocks.0.ff.net.0.proj.weight"] == (10240, 1280)
    # FLOP accounting of the engine == the oracle's count == SURVEY §8d
    for hw, want in ((32, 181.1e9), (64, 804.3e9), (96, 2149.2e9)):
        fl = net.flops(2, hw, hw, 77)
        total = sum(v[1] for v in fl.values()) / 2
        assert abs(total - want) / want < 2e-3, (hw, total)
        assert abs(total - unet_ref.count_flops(unet_ref.SD2_DEPTH, hw, hw)['total']) / want < 1e-6


def test_vae_param_table_matches_diffusers_naming():
    from contexture_nerf_amd.vae import AutoencoderKL
    from oracle import vae_ref
    v = AutoencoderKL(device="cpu", init=False)
    r = vae_ref.AutoencoderKLRef()
    assert v.param_shapes() == {k: tuple(t.shape) for k, t in r.state_dict().items()}
    dec = vae_ref.AutoencoderKLDecodeRef()
    assert set(list(v.param_shapes())[:v._n_dec]) == set(dec.state_dict().keys())   # decoder first: a decoder-only checkpoint loads
    assert 49e6 < sum(t.numel() for t in dec.parameters()) < 50e6
    assert 83e6 < sum(t.numel() for t in r.parameters()) < 84e6                     # AutoencoderKL of SD: 83.65 M parameters


def test_engine_layout_is_pinned():
    """What is layout and not tuning: the fp16 weight-blob sizes of the three engines (every table entry rounded up to 128
    elements) and the SD2 UNet's launches per forward by kernel class.  Workspace sizes follow the tuned plan table: not pinned."""
    from contexture_nerf_amd.unet import UNet2DConditionModel, ControlNetModel, SD2_DEPTH
    from contexture_nerf_amd.vae import AutoencoderKL
    net = UNet2DConditionModel(SD2_DEPTH, device="cpu", init=False)
    cn = ControlNetModel(SD2_DEPTH, device="cpu", init=False)
    vae = AutoencoderKL(device="cpu", init=False)
    assert net._lib.ctx_unet_weight_bytes(net._h) == 1731858176
    assert cn._lib.ctx_unet_weight_bytes(cn._h) == 728486912
    assert vae._lib.ctx_vae_weight_bytes(vae._h) == 236137728
    fl = net.flops(2, 32, 32, 77)
    assert [fl[k][0] for k in ('gemm_conv', 'attention', 'other')] == [193, 32, 189]


def test_size_queries():
    from contexture_nerf_amd import _lib as L
    lib = L.load()
    assert lib.ctx_rasterize_ws_bytes(1200, 1200, 7, 7500) > 7 * 361 * 7500 * 4
    assert lib.ctx_uvmlp_packed_bytes(8, 256, 42, 3, 4) > 483075 * 4
    assert lib.ctx_uvmlp_packed_bytes(8, 100, 42, 3, 4) == -1
    assert lib.ctx_attention_ws_bytes(2, 77, 5) == 256          # V is consumed untransposed: token size only


def test_tuned_plan_table_is_well_formed():
    """gemm_tuned.h (generated by tools/tune_gemm.py): unique keys, tile ids that exist, split-K only where it is allowed."""
    import os, re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "contexture-nerf_amd", "csrc", "gemm_tuned.h")
    rows = []
    for line in open(path):
        m = re.match(r"\s*\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (-?\d+), (-?\d+), (\d+)\}", line)
        if m:
            rows.append(tuple(int(x) for x in m.groups()))
    assert len(rows) >= 100
    keys = [r[:6] for r in rows]
    assert len(set(keys)) == len(keys), "duplicate shape in the plan table"
    for conv, M, N, K, flags, epi, tile, use8, S in rows:
        assert conv in (0, 1) and flags in (0, 1, 2) and epi in (0, 1)
        # use8: 1 gemm8.hip, 2 / 3 conv_halo.hip, 4 .. 8 gemm144.hip (8: the 288 x 160 form); tile: the 28 forms of gemm.hip
        assert (tile == -1 and use8 in (1, 2, 3, 4, 5, 6, 7, 8)) or (0 <= tile <= 27 and use8 == 0), (tile, use8)
        if use8 == 8:
            assert M >= 6912, "the 288-row tile is for the lockstep batch only"
        if use8 in (4, 5, 6, 7, 8):
            assert epi == 0 and K % 64 == 0, "gemm144.hip: plain epilogue, 64-deep stages"
        assert S >= 1 and (S == 1 or (epi == 0 and N % 4 == 0)), "split-K needs the plain epilogue"
        assert K % 32 == 0 and N % 8 == 0 and (not conv or K % 9 == 0)
        if tile >= 10:
            assert K % 64 == 0                          # 64-deep stages
        if epi == 1:
            assert tile not in (5, 6, 9, 11, 13, 15, 17, 19, 21)  # GEGLU needs 64-wide wave tiles
