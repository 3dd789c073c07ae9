"""Config surface: the dataclasses of src/configs/train_config.py (same field names and defaults) plus a
minimal pyrallis-compatible loader (pyrallis is not installable offline): YAML via --config_path and dotted
`--a.b=value` overrides, as `python -m scripts.run_texture --config_path=... --optim.seed=3`."""
import dataclasses
import sys
from dataclasses import dataclass, field
from pathlib import Path
from typing import List, Optional, Tuple, get_type_hints
import yaml


@dataclass
class RenderConfig:
    train_grid_size: int = 1200
    eval_grid_size: int = 1024
    radius: float = 1.5
    overhead_range: float = 40
    front_range: float = 70
    front_offset: float = 0.0
    n_views: int = 8
    base_theta: float = 60
    views_before: List[Tuple[float, float]] = field(default_factory=list)
    views_after: List[Tuple[float, float]] = field(default_factory=lambda: [[180, 30], [180, 150]])
    alternate_views: bool = True


@dataclass
class GuideConfig:
    text: str = ''
    shape_path: str = 'shapes/spot_triangulated.obj'
    append_direction: bool = False
    concept_name: Optional[str] = None
    concept_path: Optional[Path] = None
    diffusion_name: str = 'stabilityai/stable-diffusion-2-depth'
    second_model_type: Optional[str] = None
    individual_control_of_conditions: bool = False
    guidance_scale_i: Optional[int] = None
    guidance_scale_t: Optional[int] = None
    use_zero123plus: Optional[bool] = True
    guess_mode: Optional[bool] = False
    shape_scale: float = 0.6
    dy: float = 0.25
    texture_resolution: int = 1024
    texture_interpolation_mode: str = 'bilinear'    # 'nearest' | 'bilinear' (the reference's) | 'mipmap': trilinear lookup in the atlas's mip
                                                    # pyramid at a per-face level of detail (csrc/texmip.hip)
    mip_levels: int = 4              # read under texture_interpolation_mode = 'mipmap' only: levels of the pyramid, level 0 = the atlas;
                                     # texture_resolution must be a multiple of 2^(mip_levels-1) and the last level at least 2 x 2
    guidance_scale: float = 7.5
    use_inpainting: bool = True
    reference_texture: Optional[Path] = None
    initial_texture: Optional[Path] = None
    use_background_color: bool = False
    background_img: str = 'textures/brick_wall.png'
    z_update_thr: float = 0.2        # read under paint_mode = 'progressive' only: a painted texel is refined when a view sees it this much more
                                     # frontally than the view that painted it (ConTEXTure.calculate_trimap)
    strict_projection: bool = True   # read under paint_mode = 'progressive' only: the projection weight drops below 0.5 and where an
                                     # earlier view was more frontal (ConTEXTure.projection_weight)
    # --- additions of this build (not in the reference): BASELINE.json configs vary the SD image size ---
    sd_image_size: int = 512
    num_inference_steps: int = 50
    zero123plus_model_dir: Optional[str] = None      # LOCAL directory in the zero123plus pipeline layout (vision_encoder/, feature_extractor_clip/,
                                                     # tokenizer/, text_encoder/, model_index.json, optionally unet/ vae/ controlnet/): the condition
                                                     # path of src/zero123plus.py:772-803; nothing is fetched by name
    atlas_fill: str = 'none'         # 'none': uncovered texels keep the texture field's colour (the outputs of earlier builds, byte for byte);
                                     # 'nearest': after the atlas merge every uncovered chart texel copies its nearest covered texel and the
                                     # charts are padded outward (ConTEXTure.complete_atlas, csrc/atlasfill.hip)
    atlas_pad: int = 8               # texels of chart-edge padding of atlas_fill = 'nearest' (0: hole fill only)
    projection: str = 'scatter'      # how painted views reach the atlas.  'scatter': every visible pixel splats into the four texels round its
                                     # UV (ConTEXTure.project_back_scatter, csrc/uvscatter.hip; the outputs of earlier builds, bit for bit);
                                     # 'gather': every chart texel looks its surface point up in the views (project_back_gather,
                                     # csrc/uvgather.hip): no pinholes where the surface is magnified, nothing outside the charts
    paint_mode: str = 'independent'  # 'independent': every view is denoised from pure noise and the views are merged by the view-weight masks
                                     # (the outputs of earlier builds, bit for bit); 'progressive': TEXTure's loop (ConTEXTure.paint_progressive):
                                     # the views are painted one after another, each conditioned on what the earlier ones painted, through a
                                     # generate / refine / keep trimap, masked latent blending and a meta-texture of the z-normal every texel
                                     # was painted at (csrc/maskops.hip).  One rank; optim.views_per_eval and optim.views_in_flight are not read
    exposure_compensation: bool = False   # true: the per-view paint loop (paint_mode = 'independent', MeshBatchPainter.paint_all) keeps its painted
                                     # views, solves one gain per view and colour channel from where the views overlap on the surface
                                     # (kal.view_pair_stats, csrc/viewgain.hip; kal.solve_view_gains) and projects the gained views: no step in
                                     # tone at the borders of the view-weight partition.  false: no new kernel is called, every output, launch
                                     # and random draw as before.  Refused with paint_mode = 'progressive' (its views are consistent by
                                     # construction); not read by the SDS loop or by project_back's running atlas
    exposure_resolution: int = 256   # exposure_compensation: side Tc of the low-resolution atlases the statistics are taken on (1..4096)
    exposure_ridge: float = 0.01     # weight of the pull of every log gain towards 0, per valid texel of the view (>= 0)
    exposure_max_gain: float = 2.0   # gains are clipped to [1 / max_gain, max_gain] (>= 1)
    exposure_z_min: float = 0.25     # a pixel enters the statistics when it shows the object and its z-normal is at least this
    texture_field: str = 'mlp'       # the field behind the atlas.  'mlp': the 8 x 256 MLP on the Fourier embedding of uv (the outputs of earlier
                                     # builds, bit for bit); 'hashgrid': a multiresolution hash table over the UV square and a 2 x 64 MLP
                                     # (hashgrid.HashGridTexture, csrc/hashtex.hip; its finest level is texture_resolution)
    hashgrid_levels: int = 12        # texture_field = 'hashgrid': levels, features per entry, log2 of the entries per level, coarsest resolution
    hashgrid_features: int = 2
    hashgrid_log2_table: int = 18
    hashgrid_base_res: int = 16


@dataclass
class OptimConfig:
    seed: int = 0
    lr: float = 1e-2
    min_timestep: float = 0.02
    max_timestep: float = 0.98
    no_noise: bool = False
    learn_max_z_normals: bool = True
    alpha: float = -100
    # additions of this build (not in the reference's OptimConfig):
    views_in_flight: int = 3         # views_per_eval 0 / 1: single views a rank keeps in flight on one GPU, one lane (engine + HIP stream) each
    views_per_eval: int = 0          # 2..8: full groups of that many views are denoised in lockstep as ONE UNet evaluation of batch 2 x views_per_eval,
                                     # two groups in flight; left-over views all in flight as single views (stable_diffusion_depth.plan_waves)
    sds_iterations: int = 0          # 0: the per-view paint loop (north_star).  > 0: the reference's live paint() = paint_zero123plus
                                     # with that many SDS iterations (the reference hard-codes 5000, src/training/trainer.py:662)
    consistency_weight: float = 0.0  # > 0: the SDS loop back-propagates loss - weight * view consistency of the six rendered views
                                     # (src/training/trainer.py:856-863, where upstream fixed the weight at 500 and then switched the term
                                     # off); 0.0: the kernel is not called and the loop computes what it computed before
    field_texels: str = 'all'        # the texels the SDS loop evaluates and trains the texture field on.  'all': the whole atlas (the outputs
                                     # of earlier builds, bit for bit); 'active': only the texels the loop's cached raster can read
                                     # (kal.active_texels; the rendered images keep their bits, src/models/textured_mesh.py:303-347)
    hashgrid_lr: float = 1e-2        # guide.texture_field = 'hashgrid': Adam's rate for the hash table and for its MLP in the SDS loop
    hashgrid_mlp_lr: float = 1e-3    # (instant-ngp's rates, not tuned here)
    fused_adam: bool = False         # true: the SDS loop steps with optim.FieldAdam (HIP; same groups, betas and eps); a hashgrid texture
                                     # field's table then takes its step from the backward's integer sums and leaves entries with a zero
                                     # gradient alone, and the record's grad_norm covers the MLP only.  false: torch.optim.Adam, every bit as before


@dataclass
class LogConfig:
    exp_name: str = 'default'
    exp_root: Path = Path('experiments/')
    eval_only: bool = False
    eval_size: int = 10
    full_eval_size: int = 100
    save_mesh: bool = True
    vis_diffusion_steps: bool = False
    log_images: bool = True
    eval_consistency: bool = False   # full_eval also writes results/view_consistency.json (ConTEXTure.view_consistency of the train views)

    @property
    def exp_dir(self) -> Path:
        return self.exp_root / self.exp_name


@dataclass
class TrainConfig:
    log: LogConfig = field(default_factory=LogConfig)
    render: RenderConfig = field(default_factory=RenderConfig)
    optim: OptimConfig = field(default_factory=OptimConfig)
    guide: GuideConfig = field(default_factory=GuideConfig)


def _coerce(value, typ):
    origin = getattr(typ, '__origin__', None)
    if value is None:
        return None
    if origin is not None and type(None) in getattr(typ, '__args__', ()):      # Optional[T]
        inner = [a for a in typ.__args__ if a is not type(None)][0]
        return _coerce(value, inner)
    if typ is bool:
        return value if isinstance(value, bool) else str(value).lower() in ('1', 'true', 'yes')
    if typ in (int, float, str):
        return typ(value)
    if typ is Path:
        return Path(value)
    return value


def _apply(obj, key, value):
    hints = get_type_hints(type(obj))
    if key not in hints:
        raise KeyError(f"unknown config field {type(obj).__name__}.{key}")     # pyrallis raises on unknown keys too
    cur = getattr(obj, key)
    if dataclasses.is_dataclass(cur):
        if not isinstance(value, dict):
            raise TypeError(f"{key}: expected a mapping")
        for k, v in value.items():
            _apply(cur, k, v)
    else:
        setattr(obj, key, _coerce(value, hints[key]))


ATLAS_FILL_MODES = ('none', 'nearest')
PROJECTION_MODES = ('scatter', 'gather')
FIELD_TEXELS_MODES = ('all', 'active')
TEXTURE_FIELDS = ('mlp', 'hashgrid')
PAINT_MODES = ('independent', 'progressive')
INTERPOLATION_MODES = ('nearest', 'bilinear', 'bicubic', 'mipmap')     # 'bicubic' passes as it did: the sampler itself refuses it


def validate(cfg):
    """Value checks of the fields this build adds (the types are coerced by _apply)."""
    guide = getattr(cfg, 'guide', None)
    if guide is not None:
        if guide.atlas_fill not in ATLAS_FILL_MODES:
            raise ValueError(f"guide.atlas_fill={guide.atlas_fill!r}: expected one of {ATLAS_FILL_MODES}")
        if guide.atlas_pad < 0:
            raise ValueError(f"guide.atlas_pad={guide.atlas_pad}: expected >= 0")
        if guide.projection not in PROJECTION_MODES:
            raise ValueError(f"guide.projection={guide.projection!r}: expected one of {PROJECTION_MODES}")
        if guide.texture_field not in TEXTURE_FIELDS:
            raise ValueError(f"guide.texture_field={guide.texture_field!r}: expected one of {TEXTURE_FIELDS}")
        if guide.paint_mode not in PAINT_MODES:
            raise ValueError(f"guide.paint_mode={guide.paint_mode!r}: expected one of {PAINT_MODES}")
        if guide.texture_interpolation_mode not in INTERPOLATION_MODES:
            raise ValueError(f"guide.texture_interpolation_mode={guide.texture_interpolation_mode!r}: expected one of {INTERPOLATION_MODES}")
        if guide.texture_interpolation_mode == 'mipmap':
            T, Lm = int(guide.texture_resolution), int(guide.mip_levels)
            if not (1 <= Lm <= 16 and T % (1 << (Lm - 1)) == 0 and (T >> (Lm - 1)) >= 2):
                raise ValueError(f"guide.mip_levels={guide.mip_levels} does not fit guide.texture_resolution={T}: the resolution must be a "
                                 f"multiple of 2^(mip_levels-1) and the last level at least 2 x 2")
            optim_ = getattr(cfg, 'optim', None)
            if optim_ is not None and optim_.field_texels == 'active':
                raise ValueError("guide.texture_interpolation_mode='mipmap' with optim.field_texels='active': the active set holds the "
                                 "texels under the bilinear taps, not those under the coarse levels' taps")
        if guide.exposure_compensation:
            if guide.paint_mode == 'progressive':
                raise ValueError("guide.exposure_compensation with guide.paint_mode='progressive': the progressive views are consistent by "
                                 "construction; the switch belongs to paint_mode='independent'")
            if not 1 <= guide.exposure_resolution <= 4096:
                raise ValueError(f"guide.exposure_resolution={guide.exposure_resolution}: expected 1..4096")
            if not (guide.exposure_ridge >= 0 and guide.exposure_max_gain >= 1):
                raise ValueError(f"guide.exposure_ridge={guide.exposure_ridge}, guide.exposure_max_gain={guide.exposure_max_gain}: "
                                 f"expected >= 0 and >= 1")
    optim = getattr(cfg, 'optim', None)
    if optim is not None and not (optim.hashgrid_lr > 0 and optim.hashgrid_mlp_lr > 0):
        raise ValueError(f"optim.hashgrid_lr={optim.hashgrid_lr}, optim.hashgrid_mlp_lr={optim.hashgrid_mlp_lr}: expected > 0")
    if optim is not None and not optim.consistency_weight >= 0:
        raise ValueError(f"optim.consistency_weight={optim.consistency_weight}: expected >= 0")
    if optim is not None and optim.field_texels not in FIELD_TEXELS_MODES:
        raise ValueError(f"optim.field_texels={optim.field_texels!r}: expected one of {FIELD_TEXELS_MODES}")
    return cfg


def parse(config_class=TrainConfig, argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    cfg = config_class()
    overrides = []
    path = None
    for a in argv:
        if not a.startswith('--') or '=' not in a:
            raise SystemExit(f"unrecognised argument {a!r} (use --key=value)")
        k, v = a[2:].split('=', 1)
        if k == 'config_path':
            path = v
        else:
            overrides.append((k, yaml.safe_load(v)))
    if path:
        with open(path) as f:
            for k, v in (yaml.safe_load(f) or {}).items():
                _apply(cfg, k, v)
    for k, v in overrides:
        obj = cfg
        parts = k.split('.')
        for p in parts[:-1]:
            obj = getattr(obj, p)
        _apply(obj, parts[-1], v)
    return validate(cfg)


def dump(cfg, path):
    def enc(o):
        if dataclasses.is_dataclass(o):
            return {f.name: enc(getattr(o, f.name)) for f in dataclasses.fields(o)}
        if isinstance(o, Path):
            return str(o)
        if isinstance(o, (list, tuple)):
            return [enc(x) for x in o]
        return o
    with open(path, 'w') as f:
        yaml.safe_dump(enc(cfg), f)


def wrap():
    """pyrallis.wrap() look-alike: `@wrap() def main(cfg: TrainConfig)`."""
    def deco(fn):
        def inner(*a, **k):
            cls = list(get_type_hints(fn).values())[0]
            return fn(parse(cls), *a, **k)
        return inner
    return deco
