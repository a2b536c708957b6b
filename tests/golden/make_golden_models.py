"""Generates tests/golden/reference_*.pt by RUNNING THE REFERENCE'S OWN CODE (build container only: needs /root/reference).

    python tests/golden/make_golden_models.py [output_dir]
    python tests/golden/make_golden_models.py --check     # regenerate into a temporary directory, compare with the committed files

/root/reference/e4t/models/{cross_attention,attention,transformer_2d,unet_2d_blocks,unet_2d_condition}.py and
/root/reference/e4t/encoder.py are imported unmodified; `diffusers`, `kornia`, `open_clip` resolve to the stand-ins under
tests/golden/shims (see its README: only the third-party leaves come from this repository).  Each fixture holds the
configuration, the seeded state dict (the oracle uses the reference's parameter names, so it loads by key), the inputs, and
what the reference computed: outputs and parameter gradients.  tests/test_reference_golden.py replays them on the oracle.
Small on purpose (tiny widths, 8x8 latents): the whole set is ~3 MB.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(HERE, "shims"), "/root/reference", os.path.join(ROOT, "oracle"), HERE]
# NB: e4t-diffusion_amd/ must NOT be on sys.path here — its package is also called `e4t` and would shadow the reference's

import torch  # noqa: E402

torch.set_grad_enabled(True)
def torch_twin():
    """tests/torch_twins.py (the stock-torch CLIP text encoder over this repository's checkpoint tree), loaded by path: in this
    process `e4t` is the REFERENCE's package"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("torch_twins_by_path", os.path.join(ROOT, "tests", "torch_twins.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def pack(named):
    """{name: tensor} -> (one flat fp32 vector, [(name, shape)]): thousands of tiny tensors pickle to megabytes otherwise"""
    named = dict(named)
    return torch.cat([v.detach().reshape(-1).float() for v in named.values()]), [(k, tuple(v.shape)) for k, v in named.items()]


SD_MAP_CHANNELS = (320, 320, 320, 320, 640, 640, 640, 1280, 1280, 1280, 1280, 1280, 1280)      # sums to 10880 (encoder.py:102)


def unet_fixture():
    from e4t.models.unet_2d_condition import UNet2DConditionModel           # the reference's class
    assert sys.modules[UNet2DConditionModel.__module__].__file__.startswith("/root/reference/")
    cfg = dict(sample_size=8, in_channels=4, out_channels=4, block_out_channels=(8, 8, 16, 16), layers_per_block=2,
               cross_attention_dim=12, attention_head_dim=2, norm_num_groups=2, norm_eps=1e-5,
               down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"),
               up_block_types=("UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D"))
    out = {}
    for name, extra in (("sd1", {}), ("sd2", dict(use_linear_projection=True, attention_head_dim=(1, 2, 2, 4)))):
        torch.manual_seed(0)
        c = dict(cfg, **extra)
        unet = UNet2DConditionModel(**c)
        g = torch.Generator().manual_seed(1)
        sample = torch.randn(2, 4, 8, 8, generator=g)
        t = torch.tensor([3, 977])
        ctx = torch.randn(2, 5, 12, generator=g)
        G = torch.randn(2, 4, 8, 8, generator=g)
        enc = unet(sample, t, ctx, return_encoder_outputs=True)["down_block_samples"]
        full = unet(sample, t, ctx).sample
        scalar_t = unet(sample[:1], 500, ctx[:1]).sample                     # python-int timestep path (:446-455)
        (full * G).sum().backward()
        grads = {n: p.grad.clone() for n, p in unet.named_parameters() if "wo" in n}
        assert len(enc) == 13 and len(grads) == 96 * 9 and all(v.abs().sum() > 0 for v in grads.values())
        out[name] = dict(config=c, state_dict=pack(unet.state_dict()), sample=sample, timestep=t, ctx=ctx,
                         G=G, down_block_samples=[e.detach() for e in enc], out=full.detach(), out_scalar_t=scalar_t.detach(), wo_grads=pack(grads),
                         grad_conv_in=unet.conv_in.weight.grad.clone())
    return out


def unet_wide_fixture():
    """A UNet wide enough for the NATIVE modules (channel counts in multiples of 64): weights are a deterministic function of
    the parameter names (standin.deterministic_fill), so only inputs and the reference's outputs are stored"""
    from e4t.models.unet_2d_condition import UNet2DConditionModel           # the reference's class
    from standin import deterministic_fill
    assert sys.modules[UNet2DConditionModel.__module__].__file__.startswith("/root/reference/")
    cfg = dict(sample_size=8, in_channels=4, out_channels=4, block_out_channels=(64, 64, 128, 128), layers_per_block=2,
               cross_attention_dim=64, attention_head_dim=2, norm_num_groups=32, norm_eps=1e-5,
               down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"),
               up_block_types=("UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D"))
    unet = deterministic_fill(UNet2DConditionModel(**cfg), salt=11)
    g = torch.Generator().manual_seed(12)
    sample = torch.randn(2, 4, 8, 8, generator=g)
    t = torch.tensor([41, 903])
    ctx = torch.randn(2, 6, 64, generator=g)
    G = torch.randn(2, 4, 8, 8, generator=g)
    enc = unet(sample, t, ctx, return_encoder_outputs=True)["down_block_samples"]
    full = unet(sample, t, ctx).sample
    (full * G).sum().backward()
    pick = [n for n, _ in unet.named_parameters() if ".wo_" in n and (n.endswith(".v") or n.endswith("linear1.bias") or n.endswith("linear_row.bias"))]
    grads = {n: dict(unet.named_parameters())[n].grad.clone() for n in pick}
    assert len(enc) == 13 and len(pick) == 96 * 3
    return dict(config=cfg, salt=11, sample=sample, timestep=t, ctx=ctx, G=G, down_block_samples=[e.detach() for e in enc], out=full.detach(),
                wo_grads=pack(grads))


def attention_fixture():
    from e4t.models.cross_attention import AttnProcessor2_0, CrossAttention, CrossAttnProcessor
    out = {}
    for name, cad in (("self", None), ("cross", 24)):
        torch.manual_seed(2)
        attn = CrossAttention(query_dim=16, cross_attention_dim=cad, heads=2, dim_head=8)
        g = torch.Generator().manual_seed(3)
        x = torch.randn(2, 7, 16, generator=g)
        ctx = torch.randn(2, 5, 24, generator=g) if cad else None
        res = {}
        for pname, proc in (("math", CrossAttnProcessor()), ("sdpa", AttnProcessor2_0())):
            attn.set_processor(proc)
            attn.zero_grad()
            y = attn(x, encoder_hidden_states=ctx)
            y.square().sum().backward()
            res[pname] = dict(out=y.detach(), grads=pack({n: p.grad.clone() for n, p in attn.named_parameters()}))
        out[name] = dict(kwargs=dict(query_dim=16, cross_attention_dim=cad, heads=2, dim_head=8),
                         state_dict=pack(attn.state_dict()), x=x, ctx=ctx, **res)
    return out


def encoder_fixture():
    from e4t.encoder import E4TEncoder                                       # the reference's class
    assert sys.modules[E4TEncoder.__module__].__file__.startswith("/root/reference/")
    torch.manual_seed(4)
    enc = E4TEncoder(word_embedding_dim=24, arch="ViT-golden-test", version="none", n_odd_layers=9, freeze_clip_vision=False)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(2, 3, 40, 48, generator=g) * 2 - 1
    maps = [torch.randn(2, c, 1 + (i % 2), 2, generator=g) for i, c in enumerate(SD_MAP_CHANNELS)]
    y = enc(x, tuple(maps))
    y.square().sum().backward()
    grads = {n: p.grad.clone() for n, p in enc.named_parameters() if p.grad is not None}
    pre = enc.preprocess(x).detach()[:, :, ::16, ::16].clone()          # a 14x14 sample of the 224x224 CLIP input
    return dict(kwargs=dict(word_embedding_dim=24, n_odd_layers=9), state_dict=pack(enc.state_dict()),
                x=x, maps=maps, out=y.detach(), grads=pack(grads), preprocessed=pre)


def encoder_wide_fixture():
    """The reference E4TEncoder at a width the NATIVE encoder supports (ViT width 64), name-derived weights, outputs only"""
    from e4t.encoder import E4TEncoder                                       # the reference's class
    from standin import deterministic_fill
    assert sys.modules[E4TEncoder.__module__].__file__.startswith("/root/reference/")
    enc = deterministic_fill(E4TEncoder(word_embedding_dim=64, arch="ViT-golden-wide", version="none", n_odd_layers=9, freeze_clip_vision=False), salt=21)
    g = torch.Generator().manual_seed(22)
    x = torch.rand(2, 3, 40, 48, generator=g) * 2 - 1
    maps = [torch.randn(2, c, 1 + (i % 2), 2, generator=g) for i, c in enumerate(SD_MAP_CHANNELS)]
    y = enc(x, tuple(maps))
    y.square().sum().backward()
    pick = ["final_linear.weight", "feature_linear.bias", "first_linears.0.weight", "first_linears.8.bias", "unet_feature_embedder.2.weight",
            "clip_vision.ln_post.weight", "clip_vision.transformer.resblocks.0.attn.in_proj_weight", "clip_vision.class_embedding"]
    named = dict(enc.named_parameters())
    return dict(kwargs=dict(word_embedding_dim=64, n_odd_layers=9), salt=21, x=x, maps=maps, out=y.detach(), grads=pack({n: named[n].grad.clone() for n in pick}))


def pipeline_fixture(unet_blob):
    """the reference's StableDiffusionE4TPipeline.__call__ (pipeline_stable_diffusion_e4t.py:91-250) on: the reference UNet with
    the 'sd1' fixture weights, a stand-in E4T encoder, this repository's torch CLIP text twin, the offline tokenizer and the
    oracle's DDIM restatement behind the diffusers scheduler call surface"""
    import types

    import importlib.util

    import e4t_oracle as orc
    from e4t.models.unet_2d_condition import UNet2DConditionModel        # the reference's classes
    from e4t.pipeline_stable_diffusion_e4t import StableDiffusionE4TPipeline

    def native(name):            # single files of this repository's package, loaded under another name (no `e4t` clash)
        spec = importlib.util.spec_from_file_location(f"native_{name}", os.path.join(ROOT, "e4t-diffusion_amd", "e4t", f"{name}.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    CLIPTextModel, WhitespaceTokenizer = torch_twin().CLIPTextModel, native("utils").WhitespaceTokenizer
    from standin import PROMPT, TEXT_CFG, StandInEncoder
    for cls in (UNet2DConditionModel, StableDiffusionE4TPipeline):
        assert sys.modules[cls.__module__].__file__.startswith("/root/reference/"), cls

    class Sched(orc.DDIMScheduler):
        def set_timesteps(self, n, device=None):
            super().set_timesteps(n)

        def step(self, model_output, timestep, sample, eta=0.0, generator=None):
            return types.SimpleNamespace(prev_sample=super().step(model_output, timestep, sample, eta=eta))

    cfg = unet_blob["config"]
    unet = UNet2DConditionModel(**cfg)
    flat, spec = unet_blob["state_dict"]
    o, sd = 0, {}
    for name, shape in spec:
        n = int(torch.tensor(shape).prod()) if shape else 1
        sd[name] = flat[o:o + n].view(shape)
        o += n
    unet.load_state_dict(sd)
    torch.manual_seed(6)
    text = CLIPTextModel(**dict(TEXT_CFG, hidden_size=cfg["cross_attention_dim"])).requires_grad_(False)
    tok = WhitespaceTokenizer()
    enc = StandInEncoder(sum(2 * c for c in cfg["block_out_channels"]) + cfg["block_out_channels"][0] + sum(cfg["block_out_channels"][:-1]) + cfg["block_out_channels"][-1],
                         cfg["cross_attention_dim"])
    vae = types.SimpleNamespace(config=types.SimpleNamespace(block_out_channels=(1, 1, 1, 1), scaling_factor=0.18215))
    e4t_config = types.SimpleNamespace(placeholder_token="*s", domain_class_token="art", domain_embed_scale=0.1)
    pipe = StableDiffusionE4TPipeline(vae=vae, text_encoder=text, tokenizer=tok, unet=unet, e4t_encoder=enc, scheduler=Sched(),
                                      safety_checker=None, feature_extractor=None, e4t_config=e4t_config, requires_safety_checker=False)
    g = torch.Generator().manual_seed(8)
    image = torch.rand(1, 3, 16, 16, generator=g) * 2 - 1
    lat0 = torch.randn(2, 4, 8, 8, generator=g)
    res = {}
    with torch.no_grad():
        for gs in (1.0, 3.0):
            res[gs] = pipe(PROMPT, height=64, width=64, num_inference_steps=3, guidance_scale=gs, num_images_per_prompt=2, latents=lat0.clone(),
                           image=image, output_type="latent").images
    return dict(text_state=pack(text.state_dict()), image=image, latents=lat0, steps=3, final=res, placeholder_id=tok.convert_tokens_to_ids("*s"))


def pipeline_wide_fixture():
    """the reference pipeline once more, at a UNet width the NATIVE pipeline can run (name-derived weights, outputs only)"""
    import importlib.util
    import types

    import e4t_oracle as orc
    from e4t.models.unet_2d_condition import UNet2DConditionModel
    from e4t.pipeline_stable_diffusion_e4t import StableDiffusionE4TPipeline
    from standin import PROMPT, TEXT_CFG, StandInEncoder, deterministic_fill

    def native(name):
        spec = importlib.util.spec_from_file_location(f"native_{name}", os.path.join(ROOT, "e4t-diffusion_amd", "e4t", f"{name}.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    CLIPTextModel, WhitespaceTokenizer = torch_twin().CLIPTextModel, native("utils").WhitespaceTokenizer

    class Sched(orc.DDIMScheduler):
        def set_timesteps(self, n, device=None):
            super().set_timesteps(n)

        def step(self, model_output, timestep, sample, eta=0.0, generator=None):
            return types.SimpleNamespace(prev_sample=super().step(model_output, timestep, sample, eta=eta))

    cfg = dict(sample_size=8, in_channels=4, out_channels=4, block_out_channels=(64, 64, 128, 128), layers_per_block=2,
               cross_attention_dim=64, attention_head_dim=2, norm_num_groups=32, norm_eps=1e-5,
               down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"),
               up_block_types=("UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D"))
    unet = deterministic_fill(UNet2DConditionModel(**cfg), salt=31)
    tok = WhitespaceTokenizer()
    tok.add_tokens("*s")
    text = deterministic_fill(CLIPTextModel(**dict(TEXT_CFG, hidden_size=64, intermediate_size=128, vocab_size=len(tok))), salt=32).requires_grad_(False)
    boc = cfg["block_out_channels"]
    enc = StandInEncoder(sum(2 * c for c in boc) + boc[0] + sum(boc[:-1]) + boc[-1], 64)
    vae = types.SimpleNamespace(config=types.SimpleNamespace(block_out_channels=(1, 1, 1, 1), scaling_factor=0.18215))
    e4t_config = types.SimpleNamespace(placeholder_token="*s", domain_class_token="art", domain_embed_scale=0.1)
    pipe = StableDiffusionE4TPipeline(vae=vae, text_encoder=text, tokenizer=tok, unet=unet, e4t_encoder=enc, scheduler=Sched(), safety_checker=None,
                                      feature_extractor=None, e4t_config=e4t_config, requires_safety_checker=False, already_added_placeholder_token=True)
    g = torch.Generator().manual_seed(33)
    image = torch.rand(1, 3, 16, 16, generator=g) * 2 - 1
    lat0 = torch.randn(2, 4, 8, 8, generator=g)
    res = {}
    with torch.no_grad():
        for gs in (1.0, 4.0):
            res[gs] = pipe(PROMPT, height=64, width=64, num_inference_steps=3, guidance_scale=gs, num_images_per_prompt=2, latents=lat0.clone(),
                           image=image, output_type="latent").images
    return dict(config=cfg, image=image, latents=lat0, steps=3, final=res)


def step_fixture(unet_blob):
    """One pre-training step by EXECUTING THE REFERENCE'S OWN LINES: pretrain_e4t.py:561-584 (class embedding, ""-prompt context,
    prompt templates) and :597-654 (the body of `with accelerator.accumulate(unet):` — latents, noise, timesteps, prompts, both UNet
    passes, embedding injection, losses, backward, optimiser step) are read from the file, dedented and exec'd verbatim in a
    namespace holding: the reference UNet ('sd1' fixture weights), a trainable stand-in E4T encoder, the torch CLIP text twin,
    the offline tokenizer, and stand-ins for accelerate / the diffusers scheduler and VAE objects.  What the lines drew at random
    and what they computed is recorded."""
    import importlib.util
    import random
    import textwrap
    import types

    import torch.nn.functional as F

    import e4t_oracle as orc
    from e4t.models.unet_2d_condition import UNet2DConditionModel
    from standin import TEXT_CFG, StandInEncoder

    def native(name):
        spec = importlib.util.spec_from_file_location(f"native_{name}", os.path.join(ROOT, "e4t-diffusion_amd", "e4t", f"{name}.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    CLIPTextModel, WhitespaceTokenizer = torch_twin().CLIPTextModel, native("utils").WhitespaceTokenizer
    lines = open("/root/reference/pretrain_e4t.py").read().splitlines()
    prelude = textwrap.dedent("\n".join(lines[560:584]))          # file lines 561-584
    body = textwrap.dedent("\n".join(lines[596:654]))             # file lines 597-654
    assert prelude.lstrip().startswith("domain_class_token_id = tokenizer(") and body.startswith('pixel_values = batch["pixel_values"]')
    assert body.rstrip().endswith("optimizer.zero_grad()")

    cfg = unet_blob["config"]
    unet = UNet2DConditionModel(**cfg)
    flat, spec = unet_blob["state_dict"]
    o, sd = 0, {}
    for name, shape in spec:
        n = int(torch.tensor(shape).prod()) if shape else 1
        sd[name] = flat[o:o + n].view(shape)
        o += n
    unet.load_state_dict(sd)
    for n, p in unet.named_parameters():                         # pretrain_e4t.py:262-278
        p.requires_grad_("wo" in n)
    d = cfg["cross_attention_dim"]
    torch.manual_seed(9)
    tok = WhitespaceTokenizer()
    tok.add_tokens("*s")
    text = CLIPTextModel(**dict(TEXT_CFG, hidden_size=d, vocab_size=len(tok))).requires_grad_(False)
    boc = cfg["block_out_channels"]
    enc = StandInEncoder(sum(2 * c for c in boc) + boc[0] + sum(boc[:-1]) + boc[-1], d)
    enc.w.requires_grad_(True)
    acp = orc.ddpm_alphas_cumprod()
    sched = types.SimpleNamespace(config=types.SimpleNamespace(num_train_timesteps=1000, prediction_type="epsilon"),
                                  add_noise=lambda x0, nz, t: orc.add_noise(x0, nz, t, acp), get_velocity=lambda x0, nz, t: orc.get_velocity(x0, nz, t, acp))

    class VAE:                                                   # stand-in for AutoencoderKL: a fixed linear map of the pooled image
        config = types.SimpleNamespace(scaling_factor=0.18215)
        P = torch.randn(4, 3, generator=torch.Generator().manual_seed(10))

        def encode(self, x):
            z = torch.einsum("lc,bchw->blhw", self.P, F.avg_pool2d(x, 8))
            return types.SimpleNamespace(latent_dist=types.SimpleNamespace(sample=lambda: z))
    params = [enc.w] + [p for n, p in unet.named_parameters() if "wo" in n]
    optimizer = torch.optim.AdamW(params, lr=1e-3)
    g = torch.Generator().manual_seed(11)
    px = torch.rand(2, 3, 64, 64, generator=g) * 2 - 1
    ns = dict(torch=torch, F=F, random=random, tokenizer=tok, text_encoder=text, unet=unet, e4t_encoder=enc, vae=VAE(), weight_dtype=torch.float32,
              noise_scheduler=sched, optimizer=optimizer, lr_scheduler=types.SimpleNamespace(step=lambda: None),
              accelerator=types.SimpleNamespace(device=torch.device("cpu"), backward=lambda loss: loss.backward()),
              args=types.SimpleNamespace(domain_class_token="art", prompt_template="a photo of {placeholder_token}", placeholder_token="*s",
                                         domain_embed_scale=0.1, reg_lambda=0.01),
              placeholder_token_id=tok.convert_tokens_to_ids("*s"), batch=dict(pixel_values=px), print=lambda *a, **k: None)
    exec(prelude, ns)
    before = {n: p.detach().clone() for n, p in unet.named_parameters() if "wo" in n}
    torch.manual_seed(12)
    random.seed(12)
    grads = {}
    real_step = optimizer.step

    def step_and_record():
        grads.update({n: p.grad.clone() for n, p in unet.named_parameters() if "wo" in n})
        grads["__enc_w"] = enc.w.grad.clone()
        real_step()
    optimizer.step = step_and_record
    exec(body, ns)
    after = {n: p.detach().clone() for n, p in unet.named_parameters() if "wo" in n}
    moved = sum(float((after[n] - before[n]).abs().sum()) for n in after)
    assert moved > 0 and all(p.grad is None or float(p.grad.abs().sum()) == 0 for p in params)
    return dict(text_state=pack(text.state_dict()), vae_P=VAE.P, pixel_values=px, latents=ns["latents"].detach(), noise=ns["noise"], timesteps=ns["timesteps"],
                input_ids=ns["input_ids"], placeholder_idxs=ns["placeholder_token_id_idxs"], class_embed=ns["class_embed"].detach(),
                ctx_for_e4t=ns["encoder_hidden_states_for_e4t"].detach(), loss=ns["loss"].detach(), loss_diff=ns["loss_diff"].detach(),
                loss_reg=ns["loss_reg"].detach(), model_pred=ns["model_pred"].detach(), domain_embed=ns["domain_embed"].detach(),
                grads=pack(grads), params_after=pack(after), enc_w_after=enc.w.detach().clone())


def tuning_step_fixture(unet_blob):
    """One domain-tuning step by executing tuning_e4t.py's own lines: :266-269 (image expanded to the batch, latents once) and the
    body of `with accelerator.accumulate(unet):` (:272-338: per-step class embedding and ""-context, both UNet passes, losses,
    backward, global gradient-norm clipping, optimiser step) — every UNet parameter trains (:139-147)."""
    import importlib.util
    import itertools
    import random
    import textwrap
    import types

    import torch.nn.functional as F

    import e4t_oracle as orc
    from e4t.models.unet_2d_condition import UNet2DConditionModel
    from standin import TEXT_CFG, StandInEncoder

    def native(name):
        spec = importlib.util.spec_from_file_location(f"native_{name}", os.path.join(ROOT, "e4t-diffusion_amd", "e4t", f"{name}.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    CLIPTextModel, WhitespaceTokenizer = torch_twin().CLIPTextModel, native("utils").WhitespaceTokenizer
    lines = open("/root/reference/tuning_e4t.py").read().splitlines()
    i0 = next(i for i, l in enumerate(lines) if l.strip() == "pixel_values = image.expand(args.train_batch_size, -1, -1, -1)")
    iw = next(i for i, l in enumerate(lines) if l.strip() == "with accelerator.accumulate(unet):")
    iz = next(i for i, l in enumerate(lines) if i > iw and l.strip() == "optimizer.zero_grad()")
    prelude = textwrap.dedent("\n".join(lines[i0:i0 + 4]))
    body = textwrap.dedent("\n".join(lines[iw + 1:iz + 1]))
    assert (i0 + 1, iw + 2, iz + 1) == (266, 272, 338), (i0 + 1, iw + 2, iz + 1)      # the line numbers cited above

    cfg = unet_blob["config"]
    unet = UNet2DConditionModel(**cfg)
    flat, spec = unet_blob["state_dict"]
    o, sd = 0, {}
    for name, shape in spec:
        n = int(torch.tensor(shape).prod()) if shape else 1
        sd[name] = flat[o:o + n].view(shape)
        o += n
    unet.load_state_dict(sd)
    d = cfg["cross_attention_dim"]
    torch.manual_seed(9)
    tok = WhitespaceTokenizer()
    tok.add_tokens("*s")
    text = CLIPTextModel(**dict(TEXT_CFG, hidden_size=d, vocab_size=len(tok))).requires_grad_(False)
    boc = cfg["block_out_channels"]
    enc = StandInEncoder(sum(2 * c for c in boc) + boc[0] + sum(boc[:-1]) + boc[-1], d)
    enc.w.requires_grad_(True)
    acp = orc.ddpm_alphas_cumprod()
    sched = types.SimpleNamespace(config=types.SimpleNamespace(num_train_timesteps=1000, prediction_type="epsilon"),
                                  add_noise=lambda x0, nz, t: orc.add_noise(x0, nz, t, acp), get_velocity=lambda x0, nz, t: orc.get_velocity(x0, nz, t, acp))

    class VAE:
        config = types.SimpleNamespace(scaling_factor=0.18215)
        P = torch.randn(4, 3, generator=torch.Generator().manual_seed(10))

        def encode(self, x):
            z = torch.einsum("lc,bchw->blhw", self.P, F.avg_pool2d(x, 8))
            return types.SimpleNamespace(latent_dist=types.SimpleNamespace(sample=lambda: z))
    params = [enc.w] + list(unet.parameters())                  # tuning_e4t.py:139-144
    optimizer = torch.optim.AdamW(params, lr=1e-3)
    g = torch.Generator().manual_seed(13)
    image = torch.rand(1, 3, 64, 64, generator=g) * 2 - 1
    norms = []

    def clip(ps, max_norm):
        norms.append(torch.nn.utils.clip_grad_norm_(list(ps), max_norm))
        return norms[-1]
    ns = dict(torch=torch, F=F, random=random, itertools=itertools, tokenizer=tok, text_encoder=text, unet=unet, e4t_encoder=enc, vae=VAE(),
              weight_dtype=torch.float32, noise_scheduler=sched, optimizer=optimizer, lr_scheduler=types.SimpleNamespace(step=lambda: None),
              accelerator=types.SimpleNamespace(device=torch.device("cpu"), backward=lambda loss: loss.backward(), sync_gradients=True, clip_grad_norm_=clip),
              args=types.SimpleNamespace(train_batch_size=3, train_text_encoder=False, domain_embed_scale=0.1, reg_lambda=0.1, max_grad_norm=1.0),
              pretrained_args=types.SimpleNamespace(placeholder_token="*s"), prompt_templates=["a photo of {placeholder_token}"],
              placeholder_token_id=tok.convert_tokens_to_ids("*s"), domain_class_token_id=tok("art", add_special_tokens=False).input_ids[0], image=image)
    exec(prelude, ns)
    torch.manual_seed(14)
    random.seed(14)
    pick = ["conv_in.weight", "conv_out.bias", "down_blocks.0.resnets.0.conv1.weight", "down_blocks.1.attentions.0.transformer_blocks.0.attn2.to_k.weight",
            "mid_block.attentions.0.transformer_blocks.0.ff.net.0.proj.weight", "up_blocks.3.attentions.2.transformer_blocks.0.attn1.wo_q.linear_row.weight",
            "up_blocks.1.resnets.0.norm1.weight", "time_embedding.linear_1.weight", "mid_block.attentions.0.transformer_blocks.0.attn1.to_q.weight"]
    grads, real_step = {}, optimizer.step

    def step_and_record():
        named = dict(unet.named_parameters())
        grads.update({n: named[n].grad.clone() for n in pick})
        grads["__enc_w"] = enc.w.grad.clone()
        real_step()
    optimizer.step = step_and_record
    exec(body, ns)
    named = dict(unet.named_parameters())
    assert len(norms) == 1 and float(norms[0]) > 1.0               # the clip was active
    return dict(text_state=pack(text.state_dict()), vae_P=VAE.P, image=image, latents=ns["latents"].detach(), noise=ns["noise"], timesteps=ns["timesteps"],
                input_ids=ns["input_ids"], placeholder_idxs=ns["placeholder_token_id_idxs"], loss=ns["loss"].detach(), loss_diff=ns["loss_diff"].detach(),
                loss_reg=ns["loss_reg"].detach(), total_norm=norms[0].detach(), grads=pack(grads), params_after=pack({n: named[n].detach().clone() for n in pick}))


def check_against_committed(out_dir):
    """--check: the freshly generated fixtures in out_dir equal the committed ones (flattened, rtol 1e-5 / atol 1e-6)"""
    def flat(x, out):
        if torch.is_tensor(x):
            out.append(x.detach().reshape(-1).double())
        elif isinstance(x, dict):
            for k in sorted(x, key=str):
                flat(x[k], out)
        elif isinstance(x, (list, tuple)):
            for v in x:
                flat(v, out)
        return out
    for name in FIXTURES:
        a = torch.cat(flat(torch.load(os.path.join(HERE, f"reference_{name}.pt")), []))
        b = torch.cat(flat(torch.load(os.path.join(out_dir, f"reference_{name}.pt")), []))
        assert a.shape == b.shape, (name, a.shape, b.shape)
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6, msg=lambda m, name=name: f"{name}: {m}")
    print("committed fixtures are what the reference produces")


FIXTURES = ("unet", "unet_wide", "attention", "encoder", "encoder_wide", "pipeline", "pipeline_wide", "step", "tuning_step")


if __name__ == "__main__":
    import tempfile
    check = sys.argv[1:] == ["--check"]
    out_dir = tempfile.mkdtemp() if check else (sys.argv[1] if len(sys.argv) > 1 else HERE)
    import open_clip
    open_clip.TEST_ARCHS["ViT-golden-test"] = dict(image_size=224, patch_size=56, width=8, layers=2, heads=2, mlp_ratio=2.0)
    open_clip.TEST_ARCHS["ViT-golden-wide"] = dict(image_size=224, patch_size=56, width=64, layers=2, heads=2, mlp_ratio=2.0)
    blobs = {}
    for name, fn in (("unet", unet_fixture), ("unet_wide", unet_wide_fixture), ("attention", attention_fixture), ("encoder", encoder_fixture), ("encoder_wide", encoder_wide_fixture),
                     ("pipeline", lambda: pipeline_fixture(blobs["unet"]["sd1"])), ("pipeline_wide", pipeline_wide_fixture),
                     ("step", lambda: step_fixture(blobs["unet"]["sd1"])), ("tuning_step", lambda: tuning_step_fixture(blobs["unet"]["sd1"]))):
        blobs[name] = fn()
        path = os.path.join(out_dir, f"reference_{name}.pt")
        torch.save(blobs[name], path)
        print(f"{path}: {os.path.getsize(path) / 1e6:.2f} MB")
    if check:
        check_against_committed(out_dir)
