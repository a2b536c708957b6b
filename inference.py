"""E4T inference on MI355X — same command line as the reference's inference.py (:34-50).

    python inference.py --pretrained_model_name_or_path <dir> --image_path_or_url in.png --prompt "a photo of *s"

<dir> is a directory written by pretrain_e4t.py / tuning_e4t.py or the reference's scripts (config.json, weight_offsets.pt |
unet.pt, encoder.pt, optionally text_encoder.pt); the base Stable Diffusion weights are read from the checkpoint named in its
config: a local directory or a hub id whose snapshot is in the local Hugging Face cache, in the diffusers pipeline layout or as
state dicts unet.pt / vae.pt / text_encoder.pt, with a tokenizer/ folder (e4t/cli_common.py) — there is no hub access here.  With
--random_init everything is randomly initialised and an offline whitespace tokenizer is used (smoke runs, benchmarks).
All six samplers of the reference are available, each with the fused, graph-replayed update.

    python inference.py ... --init_image photo.png --strength 0.6 [--mask_image mask.png]

places the subject into an existing photograph: img2img from the re-noised photograph, and with a mask (white = repaint)
everything outside it is held to the photograph at every denoising step.

    python inference.py ... --guidance_scale 7.5 --guidance_rescale 0.7 [--identity_guidance_scale 10]

rescales the guided output against over-exposure and weighs the subject against the prompt.

    python inference.py ... --freeu [--freeu_b1 1.3 --freeu_b2 1.4 --freeu_s1 0.9 --freeu_s2 0.2 --freeu_version 2]

applies FreeU at the UNet's decoder concatenations.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "e4t-diffusion_amd"))

import torch  # noqa: E402
from PIL import Image  # noqa: E402


def image_grid(imgs, rows, cols):
    assert len(imgs) == rows * cols
    w, h = imgs[0].size
    grid = Image.new("RGB", size=(cols * w, rows * h))
    for i, img in enumerate(imgs):
        grid.paste(img, box=(i % cols * w, i // cols * h))
    return grid


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--image_path_or_url", type=str, help="path to the input image")
    p.add_argument("--pretrained_model_name_or_path", type=str, help="model dir including config.json, encoder.pt, weight_offsets.pt")
    p.add_argument("--prompt", type=str, nargs="?", default="a photo of *s", help="the prompt to render (several joined by '::')")
    p.add_argument("--num_inference_steps", type=int, default=50)
    p.add_argument("--guidance_scale", type=float, default=1.0)
    p.add_argument("--num_images_per_prompt", type=int, default=1)
    p.add_argument("--height", type=int, default=512)
    p.add_argument("--width", type=int, default=512)
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--scheduler_type", type=str, choices=["ddim", "plms", "lms", "euler", "euler_ancestral", "dpm_solver++"], default="ddim")
    p.add_argument("--enable_xformers_memory_efficient_attention", action="store_true")
    p.add_argument("--random_init", action="store_true", help="random weights + offline tokenizer (no checkpoint needed)")
    p.add_argument("--unet_variant", type=str, default="sd14", choices=["sd14", "sd21"])
    p.add_argument("--output", type=str, default="grid.png")
    p.add_argument("--init_image", type=str, default=None,
                   help="edit this photograph (img2img): it is re-noised to --strength of the schedule and denoised from there")
    p.add_argument("--strength", type=float, default=0.8,
                   help="share of the schedule an --init_image is re-noised by, in (0, 1]: 1 keeps little of it, small values stay close to it")
    p.add_argument("--mask_image", type=str, default=None,
                   help="inpainting mask for --init_image: white is repainted, black is held to the photograph at every step (soft values blend)")
    p.add_argument("--guidance_rescale", type=float, default=0.0,
                   help="in [0, 1]: pull every image's guided output to the conditional branch's standard deviation (v-prediction models "
                        "over-expose at usual guidance scales; 0.7 is the paper's value); needs --guidance_scale > 1")
    p.add_argument("--identity_guidance_scale", type=float, default=None,
                   help="guidance scale of the subject against the prompt with the plain class word (a third UNet branch): above "
                        "--guidance_scale it favours the subject, below it the prompt; needs --guidance_scale > 1")
    from e4t import cli_common as cc
    cc.add_tome_args(p)
    cc.add_freeu_args(p)
    cc.add_ema_args(p, training=False)
    args = p.parse_args(argv)
    cc.check_tome_args(p, args)
    cc.check_freeu_args(p, args)
    cc.check_ema_args(p, args)
    if not 0.0 <= args.guidance_rescale <= 1.0:
        p.error("--guidance_rescale must lie in [0, 1]")
    if args.identity_guidance_scale is not None and args.identity_guidance_scale < 0.0:
        p.error("--identity_guidance_scale must not be negative")
    if (args.guidance_rescale > 0.0 or args.identity_guidance_scale is not None) and args.guidance_scale <= 1.0:
        p.error("--guidance_rescale and --identity_guidance_scale need --guidance_scale > 1")
    if not 0.0 < args.strength <= 1.0:
        p.error("--strength must lie in (0, 1]")
    if args.mask_image is not None and args.init_image is None:
        p.error("--mask_image needs --init_image")
    if args.init_image is not None and int(args.num_inference_steps * args.strength) < 1:
        p.error(f"--strength {args.strength} leaves no denoising step of {args.num_inference_steps}")
    return args


def setup(args, dev):
    """Everything between the argument parser and the sampling loop (inference.py:52-101): models, base and E4T weights,
    tokenizer, scheduler, pipeline."""
    from e4t import builders
    from e4t import checkpoints as ck
    from e4t import cli_common as cc
    from e4t.cli_common import checked_load
    from e4t.pipeline_stable_diffusion_e4t import StableDiffusionE4TPipeline
    from e4t.schedulers import SCHEDULER_MAPPING
    from e4t.utils import AttributeDict, WhitespaceTokenizer, load_weight_offsets
    from e4t.vae import VAEDecoder
    cfg = AttributeDict(placeholder_token="*s", domain_class_token="art", domain_embed_scale=0.1)
    tok, sched = None, SCHEDULER_MAPPING[args.scheduler_type].stable_diffusion("epsilon" if args.unet_variant == "sd14" else "v_prediction")
    pipeline_cfgs = None
    edit = getattr(args, "init_image", None) is not None        # editing encodes the photograph: the VAE's encoder half is loaded too
    use_ema = getattr(args, "use_ema", False) and not args.random_init
    names = cc.ema_file_names(args.pretrained_model_name_or_path, use_ema)     # --use_ema: exits here when the directory holds no averaged weights
    if not args.random_init:
        d = args.pretrained_model_name_or_path
        with open(os.path.join(d, "config.json")) as f:
            config = AttributeDict(json.load(f))
        e4t = AttributeDict(config.pretrained_args) if config.pretrained_args is not None else config          # inference.py:56-57
        cfg = AttributeDict(placeholder_token=e4t.placeholder_token, domain_class_token=e4t.domain_class_token,
                            domain_embed_scale=float(e4t.domain_embed_scale))
        base, searched = e4t.pretrained_model_name_or_path, ""
        try:
            base = cc.resolve_base(base, e4t.revision)          # a hub id: its snapshot in the local cache
        except ck.CheckpointNotFoundError as ex:
            searched = f" ({ex})"
        if not base or not os.path.isdir(base):
            raise SystemExit(f"{d}/config.json names the base model {base!r}: a local directory with unet.pt / vae.pt / text_encoder.pt / tokenizer/ "
                             f"is needed{searched}")
        if ck.is_pipeline_layout(base):
            pipeline_cfgs = ck.pipeline_configs(base)
    if pipeline_cfgs is not None:       # the checkpoint's configs decide the architecture; the pipeline adds the placeholder row
        unet, enc, text, vae_enc = builders.build_from_configs(dev, pipeline_cfgs["unet"], pipeline_cfgs["text"], pipeline_cfgs["vae"],
                                                               builders.clip_arch(args.unet_variant), seed=args.seed or 0)
        print(f"[e4t] architecture from {base}: {ck.describe(pipeline_cfgs)}")
        vae = cc.pipeline_vae_decoder(dev, base)
        cc.load_pipeline_weights(base, unet=unet, text=text, vae=vae_enc if edit else None)
    else:
        unet, enc, text, vae_enc = builders.build_models(dev, args.unet_variant, seed=args.seed or 0)    # 49408-row token table; the pipeline adds the placeholder row
        with torch.device(dev):
            vae = VAEDecoder().requires_grad_(False)
    if not args.random_init:
        if pipeline_cfgs is None:
            # every load is strict: a misnamed key must not leave random weights behind (e4t/utils.py:119-124)
            checked_load(unet, os.path.join(base, "unet.pt"), lambda k: "wo" in k)
            checked_load(text, os.path.join(base, "text_encoder.pt"))
            vae_sd = torch.load(os.path.join(base, "vae.pt"), map_location="cpu")
            for mod, prefixes in ((vae, ("decoder.", "post_quant_conv.")), (vae_enc if edit else None, ("encoder.", "quant_conv."))):
                if mod is not None:
                    missing, unexpected = mod.load_state_dict({k: v for k, v in vae_sd.items() if k.startswith(prefixes)}, strict=False)
                    if missing or unexpected:
                        raise RuntimeError(f"{base}/vae.pt: missing {missing[:5]} unexpected {list(unexpected)[:5]}")
        if os.path.exists(os.path.join(d, "unet.pt")) and not use_ema:
            checked_load(unet, os.path.join(d, "unet.pt"))
        else:
            load_weight_offsets(unet, os.path.join(d, names["weight_offsets.pt"]))
        from transformers import CLIPTokenizer
        tok = CLIPTokenizer.from_pretrained(os.path.join(base, "tokenizer"))
        if os.path.exists(os.path.join(base, "scheduler", "scheduler_config.json")):
            sched = SCHEDULER_MAPPING[args.scheduler_type].from_pretrained(base, subfolder="scheduler")
    else:
        tok = WhitespaceTokenizer(base_size=49408, model_max_length=77)
    pipe = StableDiffusionE4TPipeline(vae=vae, text_encoder=text, tokenizer=tok, unet=unet, e4t_encoder=enc, scheduler=sched,
                                      safety_checker=None, feature_extractor=None, e4t_config=cfg, requires_safety_checker=False,
                                      vae_encoder=vae_enc.requires_grad_(False) if edit else None)
    if not args.random_init:
        d = args.pretrained_model_name_or_path
        checked_load(enc, os.path.join(d, names["encoder.pt"]))
        if os.path.exists(os.path.join(d, "text_encoder.pt")):                                                  # inference.py:92-101
            checked_load(text, os.path.join(d, "text_encoder.pt"))        # written by --train_text_encoder: already holds the placeholder row
    unet.requires_grad_(False)
    enc.requires_grad_(False)
    cc.apply_tome_args(unet, args)
    cc.apply_freeu_args(unet, args)
    if args.enable_xformers_memory_efficient_attention:
        pipe.enable_xformers_memory_efficient_attention()
    return dict(pipe=pipe, unet=unet, enc=enc, text=text, vae=vae, vae_encoder=pipe.vae_encoder, tokenizer=tok, scheduler=sched, base_dir=base if not args.random_init else None)


def main():
    args = parse_args()
    dev = torch.device("cuda:0")
    print(f"device: {dev}")
    pipe = setup(args, dev)["pipe"]
    print("loaded pipeline")
    if args.image_path_or_url:
        image = Image.open(args.image_path_or_url).convert("RGB").resize((512, 512))                           # e4t/utils.py load_image
    else:
        image = Image.fromarray((torch.rand(512, 512, 3) * 255).to(torch.uint8).numpy())
    generator = torch.Generator(device=dev).manual_seed(args.seed) if args.seed else None
    prompts = args.prompt.split("::")
    edit_kw = {}
    if args.init_image:
        edit_kw = dict(init_image=Image.open(args.init_image).convert("RGB"), strength=args.strength,
                       mask_image=Image.open(args.mask_image).convert("L") if args.mask_image else None)
    all_images = []
    for prompt in prompts:
        all_images.extend(pipe(prompt, num_inference_steps=args.num_inference_steps, guidance_scale=args.guidance_scale, generator=generator,
                               image=image, num_images_per_prompt=args.num_images_per_prompt, height=args.height, width=args.width,
                               guidance_rescale=args.guidance_rescale, identity_guidance_scale=args.identity_guidance_scale, **edit_kw).images)
    image_grid(all_images, len(prompts), args.num_images_per_prompt).save(args.output)
    print(f"DONE! See `{args.output}` for the results!")


if __name__ == "__main__":
    main()
