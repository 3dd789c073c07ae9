"""StableDiffusion: mirror of the live members of src/stable_diffusion_depth.py
(`__init__` :27-106, `get_text_embeds` :222-244, `img2img_step` :284-578 incl. inner `sample`,
`encode_imgs`/`decode_latents` :971-990, `get_timesteps` :992-999) with the denoise loop on the HIP UNet engine.

Offline facts: no SD2 weights / tokenizer / diffusers => the UNet is the SD2-depth ARCHITECTURE with
seeded random-init weights (or a local safetensors state_dict passed as `unet_state_dict`), text embeddings come
from a caller-supplied encoder or are seeded random [2,77,1024] (seed = a stable SHA-256 digest of the prompt, the
same in every process); the VAE encoder and decoder are the HIP engine of vae.py (AutoencoderKL architecture,
random-init offline or a local state_dict / safetensors file).

Additions over the reference: `image_size` is a parameter (the reference hard-wires 512, :519) because
BASELINE.json's configs run 256^2 / 512^2 / 768^2.
"""
import hashlib
import os
import torch
import torch.nn.functional as F
from . import _lib as L
from .scheduler import PNDMScheduler
from .unet import UNet2DConditionModel
from .vae import AutoencoderKL
from .utils import seed_everything


def plan_waves(n, views_per_eval, views_in_flight, groups_in_flight=2, batchable=True):
    """How a rank denoises its n views (the one place that decides it): -> waves, each a list of GROUPS that run concurrently,
    one lane each; a group is a list of view indices evaluated as ONE UNet batch of 2 x len(group) per step.
    2 <= views_per_eval <= 8 and batchable: consecutive full groups of views_per_eval views, groups_in_flight of them per wave;
    the n mod views_per_eval views left over form one last wave of single-view groups, all in flight (a padded batch would
    multiply their work).  Otherwise: single-view groups, views_in_flight per wave."""
    G = int(views_per_eval)
    if batchable and 2 <= G <= 8:
        nfull, gif = n - n % G, max(1, int(groups_in_flight))
        full = [list(range(g0, g0 + G)) for g0 in range(0, nfull, G)]
        rest = [[[k] for k in range(nfull, n)]] if nfull < n else []
        return [full[w:w + gif] for w in range(0, len(full), gif)] + rest
    infl = max(1, int(views_in_flight))
    return [[[k] for k in range(w, min(w + infl, n))] for w in range(0, n, infl)]


class StableDiffusion:
    def __init__(self, device, model_name='stabilityai/stable-diffusion-2-depth', concept_name=None, concept_path=None,
                 latent_mode=True, min_timestep=0.02, max_timestep=0.98, no_noise=False, use_inpaint=False,
                 second_model_type=None, guess_mode=False, unet=None, unet_state_dict=None, vae=None, text_encoder=None,
                 seed=0):
        if second_model_type not in (None,):
            raise L.CtxError(f"second_model_type={second_model_type!r}: dead branch in the reference (needs src/zero123), not built")
        self.device = device
        self.latent_mode = latent_mode
        self.no_noise = no_noise
        self.use_inpaint = False                      # never activates in the reference (paint_step stays 0, trainer.py:1048)
        self.second_model_type = second_model_type
        self.num_train_timesteps = 1000
        self.min_step = int(self.num_train_timesteps * min_timestep)
        self.max_step = int(self.num_train_timesteps * max_timestep)
        # `model_name` may be a LOCAL directory in the diffusers layout (unet/diffusion_pytorch_model.safetensors,
        # vae/diffusion_pytorch_model.safetensors): the files are read by safetensors_io (nothing is fetched by name offline)
        local = model_name if isinstance(model_name, str) and os.path.isdir(model_name) else None
        self._local_dir, self._seed, self._inpaint_unet = local, seed, None
        unet_file = os.path.join(local, 'unet', 'diffusion_pytorch_model.safetensors') if local else None
        vae_file = os.path.join(local, 'vae', 'diffusion_pytorch_model.safetensors') if local else None
        from_file = unet is None and unet_state_dict is None and unet_file is not None and os.path.exists(unet_file)
        self.unet = unet if unet is not None else UNet2DConditionModel(device=device, seed=seed,
                                                                       init=unet_state_dict is None and not from_file)
        if unet_state_dict is not None:
            self.unet.load_state_dict(unet_state_dict)
        elif from_file:
            self.unet.load_file(unet_file)
        if vae is not None:
            self.vae = vae
        elif vae_file is not None and os.path.exists(vae_file):
            self.vae = AutoencoderKL.from_file(vae_file, device=device)
        else:
            self.vae = AutoencoderKL(device=device, seed=seed)      # random-init offline
        self.text_encoder = text_encoder
        self.tokenizer = None
        if text_encoder is None and local and os.path.isdir(os.path.join(local, 'text_encoder')) and os.path.isdir(os.path.join(local, 'tokenizer')):
            # the reference's own text path (stable_diffusion_depth.py:61-66, 222-244): transformers' CLIPTokenizer + CLIPTextModel read from
            # the LOCAL diffusers-layout directory (local_files_only: nothing is fetched by name).  The text encoder is a once-per-prompt
            # torch module, not part of the per-step hot path.
            from transformers import CLIPTextModel, CLIPTokenizer
            self.tokenizer = CLIPTokenizer.from_pretrained(os.path.join(local, 'tokenizer'), local_files_only=True)
            self._clip = CLIPTextModel.from_pretrained(os.path.join(local, 'text_encoder'), local_files_only=True).to(self.device).eval()
            self.text_encoder = self._clip_embeds
        self.scheduler = PNDMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                       num_train_timesteps=self.num_train_timesteps, steps_offset=1, skip_prk_steps=True)
        self.alphas = self.scheduler.alphas_cumprod.to(self.device)
        self._lane_pool = []                          # (engine clone, side stream) per extra lane of _run_wave

    @property
    def inpaint_unet(self):
        """The SD2-inpainting UNet the reference loads next to the depth UNet (`stabilityai/stable-diffusion-2-inpainting`,
        in_channels 9, fp16; stable_diffusion_depth.py:73-88) and hands to the Zero123++ pipeline (trainer.py:312).  It never runs on
        the reference's live path (use_inpaint stays False), so it is built on first access: same architecture, seeded random
        init offline, or `<model_name>/inpaint_unet/diffusion_pytorch_model.safetensors` when model_name is a local directory."""
        if getattr(self, '_inpaint_unet', None) is None:
            cfg = dict(self.unet.config, in_channels=9)
            f = os.path.join(self._local_dir, 'inpaint_unet', 'diffusion_pytorch_model.safetensors') if self._local_dir else None
            if f and os.path.exists(f):
                self._inpaint_unet = UNet2DConditionModel.from_file(f, cfg, device=self.device)
            else:
                self._inpaint_unet = UNet2DConditionModel(cfg, device=self.device, seed=self._seed + 1)
        return self._inpaint_unet

    def _clip_embeds(self, prompt, negative_prompt=None):
        """stable_diffusion_depth.py:222-244: tokenise (pad to model_max_length), encode the prompt and '' (or the negative prompt),
        -> cat([uncond, cond])."""
        prompt = [prompt] if isinstance(prompt, str) else list(prompt)
        tok = self.tokenizer
        ti = tok(prompt, padding='max_length', max_length=tok.model_max_length, truncation=True, return_tensors='pt')
        negative_prompt = [''] * len(prompt) if negative_prompt is None else ([negative_prompt] if isinstance(negative_prompt, str) else list(negative_prompt))
        ui = tok(negative_prompt, padding='max_length', max_length=tok.model_max_length, return_tensors='pt')
        with torch.no_grad():
            te = self._clip(ti.input_ids.to(self.device))[0]
            ue = self._clip(ui.input_ids.to(self.device))[0]
        return torch.cat([ue, te]).float()

    def get_text_embeds(self, prompt, negative_prompt=None, seed=0):
        """-> cat([uncond, cond]) [2,77,1024].  With no encoder (offline) a seeded random embedding stands in."""
        if self.text_encoder is not None:
            return self.text_encoder(prompt, negative_prompt)
        # stable digest, not hash(): str hashing is randomised per interpreter, and every rank / run must condition its
        # views on the same embedding for the same prompt
        prompt = [prompt] if isinstance(prompt, str) else list(prompt)
        neg = [] if negative_prompt is None else ([negative_prompt] if isinstance(negative_prompt, str) else list(negative_prompt))
        key = '\0'.join(prompt) + '\1' + '\0'.join(neg) + '\1' + str(int(seed))
        g = torch.Generator().manual_seed(int.from_bytes(hashlib.sha256(key.encode('utf-8')).digest()[:4], 'little') & 0x7fffffff)
        return torch.randn(2, 77, self.unet.config['cross_attention_dim'], generator=g).to(self.device)

    def get_timesteps(self, num_inference_steps, strength):
        init_timestep = min(int(num_inference_steps * strength), num_inference_steps)
        t_start = max(num_inference_steps - init_timestep, 0)
        return self.scheduler.timesteps[t_start:], num_inference_steps - t_start

    def encode_imgs(self, imgs):
        imgs = 2 * imgs - 1
        return self.vae.encode(imgs).latent_dist.sample() * 0.18215

    def decode_latents(self, latents):
        latents = 1 / 0.18215 * latents
        with torch.no_grad():
            imgs = self.vae.decode(latents).sample
        return (imgs / 2 + 0.5).clamp(0, 1)

    def _new_scheduler(self):
        return PNDMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                             num_train_timesteps=self.num_train_timesteps, steps_offset=1, skip_prk_steps=True)

    class _Denoise:
        """The inner `sample` loop of img2img_step (stable_diffusion_depth.py:297-516) as a resumable job: construction does
        what precedes the loop, model_input() / apply() bracket one loop body's UNet evaluation (CFG pair in, fused CFG / PLMS
        update out); the evaluation itself is the lane runner's (`_run_wave`)."""

        def __init__(self, sd, scheduler, text_embeddings, latents, depth_mask, strength, num_inference_steps, update_mask,
                     fixed_seed, guidance_scale, check_mask=None, blend=False):
            self.scheduler = scheduler
            # blend (progressive painting, TEXTure section 3.3): the encoded render is kept as gt_latents and, before every evaluation,
            # put back at its noise level wherever the current mask is 0 (model_input).  The random draws are those of blend=False
            if blend and (latents is None or update_mask is None):
                raise L.CtxError("img2img_step: blend=True needs `inputs` (the render whose latents are kept) and an `update_mask`")
            self.blend, self.gt_latents = bool(blend), (latents if blend else None)
            self.update_mask, self.check_mask = (update_mask, check_mask) if blend else (None, None)
            self.text_embeddings, self.guidance_scale = text_embeddings, guidance_scale
            scheduler.set_timesteps(num_inference_steps)
            shape = (text_embeddings.shape[0] // 2, sd.unet.in_channels - 1, depth_mask.shape[2], depth_mask.shape[3])
            noise = None                                                 # `noise` of the reference's sample(): stays None when latents is None
            if latents is None:
                latents = torch.randn(shape, device=sd.device)
                timesteps = scheduler.timesteps
            else:
                init_timestep = min(int(num_inference_steps * strength), num_inference_steps)
                timesteps = scheduler.timesteps[max(num_inference_steps - init_timestep, 0):]
                latent_timestep = timesteps[:1]
                if fixed_seed is not None:
                    seed_everything(fixed_seed)
                noise = torch.randn_like(latents)
                if update_mask is not None:
                    latents = torch.randn(shape, device=sd.device)        # gt_latents are never blended (blend commented out, :382)
                else:
                    latents = scheduler.add_noise(latents, noise, latent_timestep)
            self.latents, self.timesteps, self.i = latents, timesteps, 0
            self.noise = noise
            self.on_step = None                                          # intermediate_vis hook: called with (t, latents) before the step
            self.depth2 = torch.cat([depth_mask] * 2)

        def done(self):
            return self.i >= len(self.timesteps)

        def model_input(self):
            """-> (x [2,C+1,h,w] = the CFG pair of this view's latents with its depth, t)."""
            t = self.timesteps[self.i]
            if self.blend:
                # the checkerboard holds for the first half of the evaluations, the plain update mask after it; the latents the UNet
                # sees (and the step then updates) are the blended ones
                curr = self.check_mask if self.check_mask is not None and self.i < len(self.timesteps) // 2 else self.update_mask
                self.latents = self.latents * curr + self.scheduler.add_noise(self.gt_latents, self.noise, t.reshape(1)) * (1 - curr)
            latent_model_input = torch.cat([self.latents] * 2)
            latent_model_input = self.scheduler.scale_model_input(latent_model_input, t)
            return torch.cat([latent_model_input, self.depth2], dim=1), t

        def apply(self, noise_pred, t):
            """noise_pred [2,C,h,w] = (uncond, text) of this view -> fused CFG + PLMS update."""
            if self.on_step is not None:
                self.on_step(t, self.latents, self.noise)
            self.latents = self.scheduler.step_cfg(noise_pred, self.guidance_scale, int(t), self.latents)['prev_sample']
            self.i += 1

    def _prepare(self, inputs, original_depth_mask, update_mask, latent_mode, image_size, blend=False):
        if blend and inputs is not None and not latent_mode and not hasattr(self.vae, 'encode'):
            raise L.CtxError(f"img2img_step: blend=True keeps the encoded render, and the VAE {type(self.vae).__name__} has no encode()")
        depth_mask = F.interpolate(original_depth_mask, size=(image_size // 8, image_size // 8), mode='bicubic', align_corners=False)
        if inputs is None:
            latents = None
        elif latent_mode:
            latents = inputs
        elif not hasattr(self.vae, 'encode'):
            # the encoded render only matters when update_mask is None (it is discarded otherwise, see _Denoise):
            # the reference's live call always passes update_mask, so a zero latent of the right shape is equivalent
            latents = torch.zeros(inputs.shape[0], self.unet.in_channels - 1, image_size // 8, image_size // 8, device=self.device)
        else:
            pred_rgb_small = F.interpolate(inputs, (image_size, image_size), mode='bilinear', align_corners=False)
            latents = self.encode_imgs(pred_rgb_small)
        if update_mask is not None:
            update_mask = F.interpolate(update_mask, (image_size // 8, image_size // 8), mode='nearest')
        depth_mask = 2.0 * (depth_mask - depth_mask.min()) / (depth_mask.max() - depth_mask.min()) - 1.0
        return latents, depth_mask, update_mask

    def _job(self, kw):
        """img2img_step's keyword arguments -> its _Denoise job (everything the reference does before the loop), with its own
        scheduler; `vis` collects the intermediate images when the call asks for them."""
        latent_mode, image_size = kw.get('latent_mode', False), kw.get('image_size', 512)
        blend = bool(kw.get('blend', False))
        latents, depth_mask, update_mask = self._prepare(kw['inputs'], kw['original_depth_mask'], kw.get('update_mask'), latent_mode, image_size, blend)
        check_mask = kw.get('check_mask') if blend else None
        if check_mask is not None:
            check_mask = F.interpolate(check_mask, (image_size // 8, image_size // 8), mode='nearest')
        job = StableDiffusion._Denoise(self, self._new_scheduler(), kw['text_embeddings'], latents, depth_mask, kw.get('strength', 0.5),
                                       kw.get('num_inference_steps', 50), update_mask, kw.get('fixed_seed'), kw.get('guidance_scale', 100),
                                       check_mask=check_mask, blend=blend)
        job.latent_mode, job.vis = latent_mode, []
        if kw.get('intermediate_vis'):
            job.on_step = lambda t, lat, noise: job.vis.append(self._vis_step(t, lat, noise))
        elif kw.get('on_step') is not None:
            job.on_step = kw['on_step']
        return job

    def img2img_step(self, text_embeddings, inputs, original_depth_mask, guidance_scale=100, strength=0.5,
                     num_inference_steps=50, update_mask=None, latent_mode=False, fixed_seed=None, intermediate_vis=False,
                     view_dir=None, front_image=None, phi=None, theta=None, condition_guidance_scales=None, image_size=512,
                     check_mask=None, blend=False, on_step=None):
        """One view: (rgb, latents) with latent_mode, else (rgb, intermediate images).  view_dir ... condition_guidance_scales
        are the reference's call contract and are not read.
        blend=True (single views only; progressive painting): the latents of `inputs` are kept and, before every UNet evaluation i,
        `latents = latents * curr + add_noise(gt_latents, noise, t) * (1 - curr)` with curr = check_mask while i < len(timesteps) // 2
        (when one is given), update_mask after that, both resized to the latent grid by nearest: the blend the reference carries
        commented out (stable_diffusion_depth.py:382).  blend=False is the loop as it was, bit for bit, and reads no check_mask.
        on_step(t, latents, noise): called with the latents that entered each evaluation, before its step."""
        call = dict(text_embeddings=text_embeddings, inputs=inputs, original_depth_mask=original_depth_mask,
                    guidance_scale=guidance_scale, strength=strength, num_inference_steps=num_inference_steps,
                    update_mask=update_mask, latent_mode=latent_mode, fixed_seed=fixed_seed,
                    intermediate_vis=intermediate_vis, image_size=image_size)
        if blend:
            call.update(blend=True, check_mask=check_mask)
        if on_step is not None:
            call['on_step'] = on_step
        return self.img2img_steps([call])[0]

    def _vis_step(self, t, latents, noise):
        """`intermediate_vis` of img2img_step (stable_diffusion_depth.py:500-511, LogConfig.vis_diffusion_steps): the x0 estimate
        the reference decodes at every step — `(latents - sigma_t * noise) / alpha_t` with the loop's INITIAL `noise` tensor (not the
        step's prediction; mirrored as written) — through the VAE, as an 8-bit PIL image."""
        from PIL import Image
        ac = self.scheduler.alphas_cumprod
        a_t, s_t = float(torch.sqrt(ac[int(t)])), float(torch.sqrt(1 - ac[int(t)]))
        vis_latents = (latents - s_t * noise) / a_t             # noise is None when latents was None: a TypeError, as in the reference
        image = self.decode_latents(vis_latents)
        image = image.cpu().permute(0, 2, 3, 1).numpy()
        return Image.fromarray((image[0] * 255).round().astype("uint8"))

    def img2img_steps(self, calls, views_per_eval=0, views_in_flight=3, groups_in_flight=2):
        """Several img2img_step calls (views, possibly of different meshes) evaluated wave by wave as `plan_waves` lays them out.
        `calls` = dicts of img2img_step keyword arguments; returns, per call and in order, what img2img_step(**call) returns.
        Every view keeps its own text embeddings, depth, seed, scheduler state and fused CFG / PLMS update.  A group of V views is
        ONE UNet evaluation of batch 2V per step: the executor's plan depends on the row count only and rows are arithmetically
        independent, so a view's bits depend on the size of its group, not on its mates, its position or what runs beside it.
        Calls that differ in image size, step count, strength or latent mode are not batched; a call with intermediate_vis runs
        as its own one-lane wave on the current stream."""
        if len(calls) > 1 and any(kw.get('blend') for kw in calls):
            raise L.CtxError(f"img2img_steps: blend=True is for single views (the progressive loop is sequential), got {len(calls)} calls")
        key = lambda kw: (kw.get('image_size', 512), kw.get('num_inference_steps', 50), kw.get('strength', 0.5), kw.get('latent_mode', False))
        vis = [bool(kw.get('intermediate_vis')) for kw in calls]
        batchable = not any(vis) and all(key(kw) == key(calls[0]) for kw in calls)
        outs = [None] * len(calls)
        with torch.no_grad():
            for wave in plan_waves(len(calls), views_per_eval, views_in_flight, groups_in_flight, batchable):
                for part in [[g] for g in wave if vis[g[0]]] + [[g for g in wave if not vis[g[0]]]]:
                    if not part:
                        continue
                    jobs = [[self._job(calls[k]) for k in g] for g in part]
                    for grp in jobs:
                        if any(not torch.equal(j.timesteps, grp[0].timesteps) for j in grp):
                            raise L.CtxError("img2img_steps: the views of one evaluation must share their timestep schedule")
                    self._run_wave(jobs)
                    for g, grp in zip(part, jobs):
                        for k, j in zip(g, grp):
                            rgb = self.decode_latents(j.latents)
                            outs[k] = (rgb, j.latents) if j.latent_mode else (rgb, j.vis)
        return outs

    def _lanes(self, n):
        """-> n (engine, stream) lanes.  Lane 0 is self.unet on the current stream; lane k >= 1 is pooled engine clone k
        (UNet2DConditionModel.clone_shared: the same weight blob, its own workspace) on pooled side stream k, made once."""
        pool = self._lane_pool
        while len(pool) < n - 1:
            pool.append((self.unet.clone_shared(), torch.cuda.Stream(self.device)))
        return [(self.unet, torch.cuda.current_stream(self.device))] + pool[:n - 1]

    def _run_wave(self, groups):
        """Denoise one wave: `groups` = lists of _Denoise jobs, one lane each, stepped round-robin one loop body at a time.  The
        deep UNet levels do not fill the chip, so evaluations in flight together finish sooner than back to back (two lockstep
        groups of 6: 34.0 instead of 36.9 ms per batch-12 evaluation, tools/bench_concurrent.py)."""
        lanes = self._lanes(len(groups))
        main = lanes[0][1]
        ctxs = [grp[0].text_embeddings if len(grp) == 1 else torch.cat([j.text_embeddings for j in grp]) for grp in groups]
        for (_, st), grp, ctx in zip(lanes[1:], groups[1:], ctxs[1:]):
            st.wait_stream(main)
            # made on the current stream, read on this lane: record_stream keeps the allocator from reusing their blocks on the
            # current stream before the lane is done with them (the first step frees the initial latents)
            for t in [ctx] + [x for j in grp for x in (j.latents, j.depth2, j.text_embeddings)]:
                t.record_stream(st)
        while not all(grp[0].done() for grp in groups):
            for (unet, st), grp, ctx in zip(lanes, groups, ctxs):
                if grp[0].done():
                    continue
                with torch.cuda.stream(st):
                    if len(grp) == 1:
                        x, t = grp[0].model_input()
                    else:
                        xs = [j.model_input() for j in grp]
                        x, t = torch.cat([x_ for x_, _ in xs]), xs[0][1]
                    noise = unet(x, float(t), encoder_hidden_states=ctx)['sample']
                    for v, j in enumerate(grp):
                        j.apply(noise[2 * v:2 * v + 2], t)
        for (_, st), grp in zip(lanes[1:], groups[1:]):
            main.wait_stream(st)
            for j in grp:
                j.latents.record_stream(main)             # made on the lane, decoded on the current stream
