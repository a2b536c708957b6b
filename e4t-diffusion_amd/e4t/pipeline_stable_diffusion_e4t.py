"""E4T sampling pipeline — same class name, constructor and ``__call__`` arguments as the reference's
``StableDiffusionE4TPipeline`` (e4t/pipeline_stable_diffusion_e4t.py:30-250), on the native modules.

What one denoising step does is the reference's (``:178-214``): UNet encoder pass on the current latents with the ""
context -> E4T encoder -> domain embedding written into the prompt's token embeddings -> text encoder -> UNet on
[latents, latents] with [""-context, prompt-context] -> guidance -> scheduler update.  What is organised differently for
the MI355X:

  * everything that does not depend on the latents is evaluated once per call, not once per step: the CLIP-ViT features of
    the conditioning image (``E4TEncoder.encode_vision``), the ""-prompt context, the weight-offset ``W_eff`` (cached by
    the bank while the parameters do not change);
  * guidance + the scheduler update are one kernel (``e4t_sampler_step``) reading the UNet's NHWC output in place, for every
    sampler whose update is linear (``scheduler.fused_plan``: DDIM without clipping at any eta, PLMS, LMS, Euler,
    Euler-ancestral, DPM-Solver++ 2M; epsilon or v prediction).  The coefficients of all steps are computed on the host once
    per call; earlier per-step terms (eps / derivative / x0 history, PLMS's first sample) live in device buffers, and the
    kernel also writes the next UNet input (``scale_model_input`` folded in) as the [x_in | x_in] CFG batch;
  * at 1-2 images a step is ~2000 short kernel launches; the whole step is captured once into a hipGraph
    (``torch.cuda.CUDAGraph``) and replayed per timestep: the timestep and the coefficient row are read from small device
    buffers that are refreshed between replays, and noise (Euler-ancestral, DDIM with eta > 0) is drawn outside the graph
    into a fixed buffer by the same ``torch.randn`` call ``step`` makes.  ``use_graph=None`` -> on for <= 2 images per call
    when the update is fused (measured with DDIM: 13.6 -> 11.8 ms/step at one image, nothing from four images up, where the
    step is GPU-bound); ``use_graph=False`` -> eager.  Without ``e4t_sampler_step`` (the CPU op emulation) only DDIM with
    eta == 0 is fused, through ``e4t_guided_step``; every other case takes the generic ``scale_model_input`` / ``step`` path.

Editing (not in the reference): ``init_image=`` starts from a photograph re-noised to ``strength`` of the schedule
(``scheduler.set_timesteps(n, begin=k)``), ``mask_image=`` additionally holds everything outside the mask to the photograph at
every step.  The definition is the generic loop (``step`` + the torch blend below); on the fused path the blend is part of the
step kernel (``e4t_sampler_step_edit``, rows of ``fused_plan(blend=True)``), so an edited step is still one UNet pass + one
update launch inside the replayed graph.  The CPU op emulation takes the generic loop.

Guidance rescale and identity guidance (not in the reference): ``guidance_rescale=`` scales every image's guided
output towards the conditional branch's standard deviation, ``identity_guidance_scale=`` adds a third UNet branch, the prompt
with the plain class word, and weighs subject against prompt.  The definition is ``schedulers.combine_guidance`` in the generic
loop; on the fused path the step is ``e4t_sampler_step_guided`` (the same kernel body), preceded by one ``e4t_guidance_stats``
launch when rescaling, both inside the replayed graph.  A call with neither option runs the launches it ran before.

The tokenizer is whatever object the caller passes (``transformers.CLIPTokenizer`` in inference.py): it needs
``__call__(text, padding=, truncation=, max_length=, return_tensors="pt", add_special_tokens=)``, ``add_tokens``,
``convert_tokens_to_ids``, ``model_max_length`` and ``__len__``.  The safety checker is not built (the reference runs the
pipeline with ``safety_checker=None``, inference.py:117-119).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Callable, List, Optional, Union

import numpy as np
import torch

from . import ops
from . import tome
from .schedulers import DDIMScheduler, combine_guidance


@dataclass
class StableDiffusionPipelineOutput:
    images: Any
    nsfw_content_detected: Optional[List[bool]] = None


def preprocess(image):
    """PIL image(s) / tensor -> float32 (N,3,H,W) in [-1,1]  (pipeline_stable_diffusion_e4t.py:12-27)"""
    if isinstance(image, torch.Tensor):
        return image
    if not isinstance(image, (list, tuple)):
        image = [image]
    if isinstance(image[0], torch.Tensor):
        return torch.cat(list(image), dim=0)
    arr = np.concatenate([np.array(i)[None, :] for i in image], axis=0).astype(np.float32) / 255.0
    return torch.from_numpy(2.0 * arr.transpose(0, 3, 1, 2) - 1.0)


class StableDiffusionE4TPipeline:
    def __init__(self, vae, text_encoder, tokenizer, unet, e4t_encoder, scheduler, safety_checker=None, feature_extractor=None,
                 e4t_config=None, requires_safety_checker: bool = True, already_added_placeholder_token: bool = False, vae_encoder=None):
        if safety_checker is not None:
            raise NotImplementedError("the safety checker is not part of this build: pass safety_checker=None")
        self.vae, self.text_encoder, self.tokenizer, self.unet, self.scheduler = vae, text_encoder, tokenizer, unet, scheduler
        self.vae_encoder = vae_encoder       # e4t.vae.VAEEncoder: only editing (init_image=) needs it
        self.e4t_encoder = e4t_encoder
        self.safety_checker, self.feature_extractor = None, feature_extractor
        boc = getattr(vae, "block_out_channels", None) or getattr(getattr(vae, "config", None), "block_out_channels", (0,) * 4)
        self.vae_scale_factor = 2 ** (len(boc) - 1)
        cfg = e4t_config if not isinstance(e4t_config, dict) else _Attr(e4t_config)
        if not already_added_placeholder_token:                                       # reference :45-53
            if self.tokenizer.add_tokens(cfg.placeholder_token) == 0:
                raise ValueError(f"The tokenizer already contains the token {cfg.placeholder_token}. Please pass a different "
                                 "`placeholder_token` that is not already in the tokenizer.")
            text_encoder.resize_token_embeddings(len(tokenizer))
        self.placeholder_token = cfg.placeholder_token
        self.placeholder_token_id = tokenizer.convert_tokens_to_ids(cfg.placeholder_token)
        ids = self.tokenizer(cfg.domain_class_token, add_special_tokens=False, return_tensors="pt").input_ids[0]
        assert ids.size(0) == 1, "the domain class must be a single token"
        emb = text_encoder.get_input_embeddings()
        self.class_embed = emb(ids.to(emb.weight.device)).detach()                    # (1, d)   reference :55-59
        self.domain_embed_scale = cfg.domain_embed_scale
        self._progress = {}
        self._graph = None
        self._fused_sampling = True          # False: every sampler takes the generic scale_model_input / step path

    # ---- housekeeping the reference inherits from DiffusionPipeline -------------------------------------------------
    @property
    def device(self):
        return next(self.unet.parameters()).device

    _execution_device = device

    def to(self, device):
        for m in (self.vae, self.text_encoder, self.unet, self.e4t_encoder, self.vae_encoder):
            if m is not None:
                m.to(device)
        self.class_embed = self.class_embed.to(device)
        self._graph = None
        return self

    def enable_xformers_memory_efficient_attention(self, attention_op=None):
        self.unet.enable_xformers_memory_efficient_attention()          # selects the native fused-attention processor

    def enable_freeu(self, b1=None, b2=None, s1=None, s2=None, version: int = 2):
        """FreeU at the UNet's decoder concatenations (e4t/freeu.py): backbone factors b1, b2 >= 1 and skip factors s1, s2
        in [0, 1] of the two stages; None = the authors' SD-1.4 values of the version.  Acts in every later call, fused and generic,
        eager and replayed, in every branch of a guided batch.  Returns the state (which ResBlocks were marked)."""
        from . import freeu
        if version not in freeu.DEFAULTS:
            raise ValueError(f"freeu version must be 1 or 2, got {version}")
        kw = dict(freeu.DEFAULTS[version])
        kw.update({k: v for k, v in dict(b1=b1, b2=b2, s1=s1, s2=s2).items() if v is not None})
        return freeu.apply_freeu(self.unet, version=version, **kw)

    def disable_freeu(self):
        from . import freeu
        freeu.remove_freeu(self.unet)

    def set_progress_bar_config(self, **kw):
        self._progress = kw

    # ---- reference helpers ----------------------------------------------------------------------------------------
    def prepare_for_e4t(self, prompt, device):
        """reference :68-88"""
        tok = self.tokenizer
        kw = dict(padding="max_length", truncation=True, max_length=tok.model_max_length, return_tensors="pt")
        ids_e = tok("", **kw).input_ids
        ids = tok(prompt, **kw).input_ids
        try:
            idx = ids[0].tolist().index(self.placeholder_token_id)
        except ValueError:
            raise ValueError(f"Your prompt may not have the placeholder_token={self.placeholder_token}")
        with torch.no_grad():
            ctx_e = self.text_encoder(ids_e.to(device))[0]
            emb = self.text_encoder.get_input_embeddings()(ids.to(device))
        return dict(placeholder_token_id_idx=idx, encoder_hidden_states_for_e4t=ctx_e, inputs_embeds=emb)

    def check_inputs(self, prompt, height, width, callback_steps):
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        if callback_steps is None or not isinstance(callback_steps, int) or callback_steps <= 0:
            raise ValueError(f"`callback_steps` has to be a positive integer but is {callback_steps} of type {type(callback_steps)}.")
        if prompt is None or not isinstance(prompt, (str, list)):
            raise ValueError(f"`prompt` has to be of type `str` or `list` but is {type(prompt)}")

    def prepare_latents(self, batch_size, num_channels_latents, height, width, dtype, device, generator, latents=None):
        shape = (batch_size, num_channels_latents, height // self.vae_scale_factor, width // self.vae_scale_factor)
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective batch size of {batch_size}.")
        return self._unit_noise(shape, dtype, device, generator, latents) * self.scheduler.init_noise_sigma

    @staticmethod
    def _unit_noise(shape, dtype, device, generator, latents=None):
        """the one N(0, 1) draw of the latent shape (or the caller's `latents`): the start of plain sampling, n0 of editing"""
        if latents is None:
            if isinstance(generator, list):
                latents = torch.cat([torch.randn((1,) + shape[1:], generator=g, device=g.device, dtype=dtype).to(device) for g in generator])
            else:
                gdev = generator.device if generator is not None else device
                latents = torch.randn(shape, generator=generator, device=gdev, dtype=dtype).to(device)
        else:
            latents = latents.to(device=device, dtype=dtype)
        return latents

    def prepare_edit(self, init_image, strength, mask_image, num_inference_steps, batch_size, height, width, device):
        """img2img / inpainting inputs -> (begin, x0, keep): the first kept step of the schedule, the clean latent
        of `init_image` (posterior mean * scaling factor; one for the batch, or one per image) and the [h*w] keep map
        (1 - the mask averaged onto the latent grid; None without a mask)."""
        if self.vae_encoder is None:
            raise ValueError("`init_image` needs the pipeline's `vae_encoder` (an e4t.vae.VAEEncoder)")
        if not 0.0 < strength <= 1.0:
            raise ValueError(f"`strength` has to lie in (0, 1] but is {strength}")
        init_steps = min(int(num_inference_steps * strength), num_inference_steps)
        if init_steps < 1:
            raise ValueError(f"`strength` = {strength} leaves no denoising step of {num_inference_steps}")
        pixels = preprocess(_resized(init_image, height, width)).to(device=device, dtype=torch.float32)
        if tuple(pixels.shape[1:]) != (3, height, width) or pixels.shape[0] not in (1, batch_size):
            raise ValueError(f"`init_image` has to be one or {batch_size} RGB images of {height} x {width} but is {tuple(pixels.shape)}")
        f = self.vae_scale_factor
        eps = torch.zeros((pixels.shape[0], self.unet.in_channels, height // f, width // f), dtype=torch.float32, device=device)
        x0 = self.vae_encoder.encode_sample(pixels, eps).float().contiguous()          # zero eps: the posterior mean, deterministic
        keep = None
        if mask_image is not None:
            m = _mask_tensor(mask_image, height, width).to(device=device, dtype=torch.float32)
            keep = (1.0 - torch.nn.functional.avg_pool2d(m[None, None], f)).reshape(-1).contiguous()
        return num_inference_steps - init_steps, x0, keep

    def decode_latents(self, latents):
        return self.vae.decode_latents(latents).cpu().float().numpy()                # (B, H, W, 3) in [0, 1]

    @staticmethod
    def numpy_to_pil(images):
        from PIL import Image
        if images.ndim == 3:
            images = images[None, ...]
        return [Image.fromarray(i) for i in (images * 255).round().astype("uint8")]

    # ---- one denoising step -----------------------------------------------------------------------------------------
    def _model_step(self, latents, t, s, x_in=None):
        """eps (or v) prediction for guidance: returns the UNet output tensor of the [uncond | cond] (or cond-only) batch,
        [uncond | class word | cond] with s["ctx_k"] (identity guidance).
        x_in: the scaled UNet input when the caller already has it, as the [x_in | x_in] batch under guidance (the fused
        loop: e4t_sampler_step writes it); None -> scheduler.scale_model_input(latents, t)."""
        bsz = latents.shape[0]
        x_cat = None
        if x_in is None:
            x_in = self.scheduler.scale_model_input(latents, t)
        else:
            x_cat, x_in = x_in, x_in[:bsz]
        ctx_e = s["ctx_e"].expand(bsz, -1, -1)
        enc = self.unet(x_in, t, ctx_e, return_encoder_outputs=True)                                   # :189
        if s["vision"] is not None:
            domain = self.e4t_encoder(x=s["pixels"], unet_down_block_samples=enc["down_block_samples"], vision=s["vision"])
        else:
            domain = self.e4t_encoder(x=s["pixels"], unet_down_block_samples=enc["down_block_samples"])  # :192
        domain = self.class_embed.expand(bsz, -1).to(domain.dtype) + s["scale"] * domain              # :194
        emb = s["inputs_embeds"].expand(bsz, -1, -1).clone()
        emb[:, s["idx"], :] = domain.to(emb.dtype)                                                       # :195-196
        ctx = self.text_encoder(inputs_embeds=emb)[0].to(ctx_e.dtype)                                    # :198
        if s.get("ctx_k") is not None:                   # identity guidance: [uncond | class word | cond]
            x_cat = torch.cat([x_in] * 3) if x_cat is None else x_cat
            return self.unet(x_cat, t, torch.cat([ctx_e, s["ctx_k"].expand(bsz, -1, -1).to(ctx_e.dtype), ctx])).sample
        if s["cfg"]:
            x_cat = torch.cat([x_in] * 2) if x_cat is None else x_cat
            return self.unet(x_cat, t, torch.cat([ctx_e, ctx])).sample                                     # :199-206
        return self.unet(x_in, t, ctx).sample

    def class_word_context(self, e4t):
        """the context of the prompt with the plain class word at the placeholder (what the conditional branch is at
        domain_embed_scale = 0): the middle branch of identity guidance, constant over the steps and the images"""
        emb = e4t["inputs_embeds"].clone()
        emb[:, e4t["placeholder_token_id_idx"], :] = self.class_embed.to(emb.dtype)
        return self.text_encoder(inputs_embeds=emb)[0].to(e4t["encoder_hidden_states_for_e4t"].dtype)

    def _fused_update(self, pred, latents, coef, cfg):
        """guidance + linear scheduler update in one kernel, in place on `latents`"""
        nhwc = pred.permute(0, 2, 3, 1)
        if nhwc.is_contiguous():                         # the native UNet hands out an NCHW view of NHWC storage
            ops.backend().guided_step(nhwc, latents, coef, cfg=cfg, pred_nhwc=True, out=latents)
        else:
            ops.backend().guided_step(pred.contiguous(), latents, coef, cfg=cfg, pred_nhwc=False, out=latents)

    def _sampler_update(self, pred, latents, row, bufs, cfg):
        """guidance + any linear sampler update in one kernel (e4t_sampler_step), in place on `latents`; also writes the next
        UNet input into bufs["x_in"]"""
        nhwc = pred.permute(0, 2, 3, 1)
        kw = dict(hist=bufs["hist"], saved=bufs["saved"], noise=bufs["noise"], x_in=bufs["x_in"], cfg=cfg, out=latents)
        if bufs.get("edit") is not None:                 # masked editing: the blend with the re-noised original, in the same kernel
            kw["edit"] = bufs["edit"]
        is_nhwc = nhwc.is_contiguous()                   # the native UNet hands out an NCHW view of NHWC storage
        p = nhwc if is_nhwc else pred.contiguous()
        if bufs.get("gp") is None:
            ops.backend().sampler_step(p, latents, row, pred_nhwc=is_nhwc, **kw)
            return
        # guidance rescale / identity guidance: the per-image statistics only when rescaling, then the guided step
        del kw["cfg"]
        branches = p.shape[0] // latents.shape[0]
        if bufs["gstat"] is not None:
            ops.backend().guidance_stats(p, bufs["gp"], branches, is_nhwc, out=bufs["gstat"])
        ops.backend().sampler_step_guided(p, latents, row, bufs["gp"], gstat=bufs["gstat"], branches=branches, pred_nhwc=is_nhwc, **kw)

    # ---- the call -------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, prompt: Union[str, List[str]] = None, height: Optional[int] = None, width: Optional[int] = None,
                 num_inference_steps: int = 50, guidance_scale: float = 7.5, negative_prompt=None, num_images_per_prompt: Optional[int] = 1,
                 eta: float = 0.0, generator=None, latents: Optional[torch.Tensor] = None, prompt_embeds=None, negative_prompt_embeds=None,
                 output_type: Optional[str] = "pil", return_dict: bool = True, callback: Optional[Callable] = None, callback_steps: int = 1,
                 cross_attention_kwargs=None, image=None, domain_embed_scale: Optional[float] = None, use_graph: Optional[bool] = None,
                 init_image=None, strength: float = 0.8, mask_image=None, guidance_rescale: float = 0.0,
                 identity_guidance_scale: Optional[float] = None):
        """image: the conditioning image (the subject).  init_image: the photograph to edit (img2img: re-noised to `strength` of
        the schedule and denoised from there); mask_image: white = repaint, everything else is held to init_image at every step.
        guidance_rescale: phi in [0, 1], the guided output of every image is pulled to the conditional branch's standard deviation
        (v-prediction models over-expose without it).  identity_guidance_scale: g_id of the three-branch guidance
        u + g*(k - u) + g_id*(c - k) with k the prompt with the plain class word; above guidance_scale it favours the subject,
        below it the prompt.  Both: DESIGN §2.5b, ``schedulers.combine_guidance`` is the definition."""
        if not 0.0 <= guidance_rescale <= 1.0:
            raise ValueError(f"`guidance_rescale` has to lie in [0, 1] but is {guidance_rescale}")
        if identity_guidance_scale is not None and identity_guidance_scale < 0.0:
            raise ValueError(f"`identity_guidance_scale` must not be negative but is {identity_guidance_scale}")
        guided = guidance_rescale > 0.0 or identity_guidance_scale is not None
        if guided and guidance_scale <= 1.0:
            raise ValueError("`guidance_rescale` and `identity_guidance_scale` need `guidance_scale` > 1: there is no unconditional "
                             f"branch at guidance_scale = {guidance_scale}")
        scale = self.domain_embed_scale if domain_embed_scale is None else domain_embed_scale
        height = height or self.unet.config.sample_size * self.vae_scale_factor
        width = width or self.unet.config.sample_size * self.vae_scale_factor
        self.check_inputs(prompt, height, width, callback_steps)
        assert negative_prompt is None, "negative_prompt is not supported"           # reference :151
        assert prompt_embeds is None and negative_prompt_embeds is None and not cross_attention_kwargs
        if isinstance(prompt, list):
            if len(prompt) != 1:
                raise ValueError("one prompt per call (the reference reads the placeholder position of prompt[0] only, :76-79)")
            prompt = prompt[0]
        device = self.device
        cfg = guidance_scale > 1.0
        pixels = preprocess(image).to(device=device, dtype=torch.float32)
        if pixels.shape[0] != 1:
            raise ValueError("one conditioning image per call")
        bsz = num_images_per_prompt
        if mask_image is not None and init_image is None:
            raise ValueError("`mask_image` needs `init_image`")
        edit = init_image is not None
        e4t = self.prepare_for_e4t(prompt, device)
        if edit:
            begin, x0, keep = self.prepare_edit(init_image, strength, mask_image, num_inference_steps, bsz, height, width, device)
            self.scheduler.set_timesteps(num_inference_steps, device=device, begin=begin)
        else:
            keep = None
            self.scheduler.set_timesteps(num_inference_steps, device=device)
        timesteps = self.scheduler.timesteps
        if edit:        # the start is the original at the first kept timestep's noise level; n0 is drawn where plain sampling draws
            shape = (bsz, self.unet.in_channels, height // self.vae_scale_factor, width // self.vae_scale_factor)
            n0 = self._unit_noise(shape, torch.float32, device, generator, latents).contiguous()
            a, sg = self.scheduler.noise_level(timesteps[0])
            latents = (a * x0 + sg * n0).contiguous()
        else:
            latents = self.prepare_latents(bsz, self.unet.in_channels, height, width, torch.float32, device, generator, latents).contiguous()

        vision = None
        if hasattr(self.e4t_encoder, "encode_vision"):                                # image features: once, not per step
            cls, tokens = self.e4t_encoder.encode_vision(pixels)
            vision = (cls.expand(bsz, -1), tokens.expand(bsz, -1, -1))
        s = dict(ctx_e=e4t["encoder_hidden_states_for_e4t"], inputs_embeds=e4t["inputs_embeds"], idx=e4t["placeholder_token_id_idx"],
                 pixels=pixels.expand(bsz, -1, -1, -1), vision=vision, scale=scale, cfg=cfg)
        branches = 2
        if identity_guidance_scale is not None:          # the class-word branch: one text-encoder pass per call
            s["ctx_k"], branches = self.class_word_context(e4t), 3

        sch = self.scheduler
        native = device.type == "cuda" and hasattr(ops.backend(), "sampler_step")
        plan = None
        if self._fused_sampling and hasattr(sch, "fused_plan"):
            plan = sch.fused_plan(guidance_scale, eta, blend=True) if keep is not None else sch.fused_plan(guidance_scale, eta)
        if plan is not None and not native and (edit or not (isinstance(sch, DDIMScheduler) and eta == 0.0)):
            plan = None                  # without e4t_sampler_step only plain DDIM with eta == 0 is fused (through e4t_guided_step)
        if plan is not None and guided and not (native and hasattr(ops.backend(), "sampler_step_guided")):
            plan = None                  # e4t_guided_step knows u + g*(c - u) only: the generic loop, also for DDIM with eta == 0
        if use_graph is None:       # measured (SD-1.4, 512 px, 50 steps, DDIM): 13.6 -> 11.8 ms/step at 1 image, no gain from 4 images up
            use_graph = plan is not None and device.type == "cuda" and bsz <= 2
        if use_graph and plan is None:
            raise ValueError("graph replay needs the fused linear update (a scheduler with a fused_plan: no sample clipping, "
                             "epsilon / v prediction; on the CPU op emulation DDIM with eta == 0 only)")

        if plan is not None:
            timesteps = plan.timesteps
            table = plan.table.to(device=device, dtype=torch.float32)
            t_buf = torch.empty(1, dtype=timesteps.dtype, device=device)
            if native:
                row = torch.empty(table.shape[1], dtype=torch.float32, device=device)
                bufs = dict(hist=torch.zeros((plan.K,) + tuple(latents.shape), dtype=torch.float32, device=device) if plan.K else None,
                            saved=torch.zeros_like(latents) if plan.saves_x else None,
                            noise=torch.zeros_like(latents) if any(plan.noisy) else None,
                            x_in=torch.empty(((branches if cfg else 1) * bsz,) + tuple(latents.shape[1:]), dtype=torch.float32, device=device))
                if guided:               # e4t_sampler_step_guided's scalars and the statistics' output: allocated before capture
                    g_id = guidance_scale if identity_guidance_scale is None else identity_guidance_scale
                    bufs["gp"] = torch.tensor([guidance_scale, g_id, guidance_rescale, 0.0], dtype=torch.float32, device=device)
                    bufs["gstat"] = torch.empty((bsz, 4), dtype=torch.float32, device=device) if guidance_rescale > 0.0 else None
                x_in = bufs["x_in"]
                torch.mul(latents, plan.k_in, out=x_in[:bsz])
                for r in range(1, branches if cfg else 1):
                    x_in[r * bsz:(r + 1) * bsz].copy_(x_in[:bsz])
                state = [latents] + [bufs[k] for k in ("hist", "saved", "x_in") if bufs[k] is not None]
                if keep is not None:     # fixed, read-only operands of e4t_sampler_step_edit: outside the captured state
                    bufs["edit"] = (keep, x0, n0)

                def one_step():
                    self._sampler_update(self._model_step(latents, t_buf, s, x_in=x_in), latents, row, bufs, cfg)
            else:                        # DDIM rows {g, 1, 0, c_sample, 0, c_pred, c_noise, ...} -> guided_step's {g, c_sample, c_pred, c_noise}
                table = table[:, [0, 3, 5, 6]].contiguous()
                row = torch.empty(4, dtype=torch.float32, device=device)
                state = [latents]

                def one_step():
                    self._fused_update(self._model_step(latents, t_buf, s), latents, row, cfg)

            graph = None
            for i in range(len(timesteps)):
                t_buf.copy_(timesteps[i:i + 1])
                row.copy_(table[i])
                tome.new_step(self.unet)         # token merging (opt-in): one draw per denoising step, into its fixed buffer
                if plan.noisy[i]:                # outside the graph, the same draw (generator, order) as the generic step()
                    bufs["noise"].copy_(sch._step_noise(latents.shape, torch.float32, device, generator))
                if not use_graph:
                    one_step()
                elif graph is None:
                    graph = self._capture(one_step, *state)
                    graph.replay()
                else:
                    graph.replay()
                if callback is not None and i % callback_steps == 0:
                    callback(i, timesteps[i], latents)
        else:
            import inspect
            accepted = set(inspect.signature(sch.step).parameters)          # prepare_extra_step_kwargs of the reference's base class
            extra = {}
            if "eta" in accepted:
                extra["eta"] = eta
            if "generator" in accepted and generator is not None:
                extra["generator"] = generator
            for i, t in enumerate(timesteps):
                tome.new_step(self.unet)
                pred = self._model_step(latents, t, s)
                if cfg:                                                             # :209-211, and DESIGN §2.5b
                    pred = combine_guidance(pred.chunk(branches), guidance_scale, identity_guidance_scale, guidance_rescale)
                latents = sch.step(pred.float(), t, latents, **extra).prev_sample    # :214
                if keep is not None:     # the definition of masked editing: hold the kept region at the next timestep's noise level
                    a, sg = sch.noise_level(timesteps[i + 1]) if i + 1 < len(timesteps) else (1.0, 0.0)
                    latents = keep.view(1, 1, *latents.shape[2:]) * (a * x0 + sg * n0) + (1.0 - keep.view(1, 1, *latents.shape[2:])) * latents
                if callback is not None and i % callback_steps == 0:
                    callback(i, t, latents)

        if output_type == "latent":
            images = latents
        else:
            images = self.decode_latents(latents)
            if output_type == "pil":
                images = self.numpy_to_pil(images)
        if not return_dict:
            return (images, None)
        return StableDiffusionPipelineOutput(images=images, nsfw_content_detected=None)

    def _capture(self, fn, latents, *state):
        """Warm the step up on a side stream (weight copies, workspaces and allocator pools reach their steady state), restore
        the latents and the other buffers the step updates (`state`: history, saved sample, next UNet input), then record the
        step into a graph on that stream."""
        bufs = (latents,) + state
        keep = [b.clone() for b in bufs]
        coefs_stream = torch.cuda.Stream(device=latents.device)
        coefs_stream.wait_stream(torch.cuda.current_stream(latents.device))
        with torch.cuda.stream(coefs_stream):
            fn()
            for b, k in zip(bufs, keep):
                b.copy_(k)
        torch.cuda.current_stream(latents.device).wait_stream(coefs_stream)
        graph = torch.cuda.CUDAGraph()
        with ops.capture_guard(), torch.cuda.graph(graph, stream=coefs_stream):
            fn()
        for b, k in zip(bufs, keep):      # capture does not execute: the first replay starts from the same state
            b.copy_(k)
        return graph


def _resized(image, height, width):
    """PIL image(s) -> resized to (width, height); tensors pass through (they must have that size already)"""
    if isinstance(image, (list, tuple)):
        return [_resized(i, height, width) for i in image]
    if hasattr(image, "resize") and not isinstance(image, (torch.Tensor, np.ndarray)):
        return image.convert("RGB").resize((width, height))
    return image


def _mask_tensor(mask, height, width):
    """PIL image / array / tensor -> float32 (height, width) in [0, 1], 1 (white) = repaint; soft values stay soft"""
    if hasattr(mask, "resize") and not isinstance(mask, (torch.Tensor, np.ndarray)):
        return torch.from_numpy(np.asarray(mask.convert("L").resize((width, height)), dtype=np.float32) / 255.0)
    m = torch.as_tensor(mask).float()
    m = m.reshape(m.shape[-2:]) if m.numel() == m.shape[-2] * m.shape[-1] else m
    if m.dim() != 2:
        raise ValueError(f"`mask_image` has to be one single-channel map but is {tuple(m.shape)}")
    if tuple(m.shape) != (height, width):
        m = torch.nn.functional.interpolate(m[None, None], size=(height, width), mode="bilinear", align_corners=False)[0, 0]
    return m.clamp(0.0, 1.0)


class _Attr(dict):
    __getattr__ = dict.__getitem__
