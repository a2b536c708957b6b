"""Generation throughput of the E4T pipeline on one MI355X (SD-1.4 shapes, 512 px, CFG 7.5): per sampler, the generic
scale_model_input / step loop vs the fused e4t_sampler_step loop run eagerly vs its hipGraph replay, at 1 and 4 images per
call, plus the VAE decode.  Random-init weights, word-level stand-in tokenizer.

    python tools/bench_inference.py --scheduler ddim dpm_solver++ euler_ancestral plms      (STEPS=50 by default)
    python tools/bench_inference.py --edit --repeats 3       masked inpainting (strength 1: every step runs) next
                                                             to plain sampling, fused legs only, each leg timed --repeats times
    python tools/bench_inference.py --images 1 --legs graph --guidance_rescale 0.7 --identity_guidance_scale 10
                                                             guidance rescale and / or the three-branch identity guidance (§2.5b)
    python tools/bench_inference.py --images 1 4 --legs graph --freeu [--freeu_version 1]
                                                             FreeU at the decoder concatenations, the default factors (§2.5c)"""
import argparse, os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "e4t-diffusion_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from bench import build_models
from e4t.pipeline_stable_diffusion_e4t import StableDiffusionE4TPipeline
from e4t.schedulers import SCHEDULER_MAPPING, DDIMScheduler
from e4t.vae import VAEDecoder, VAEEncoder
from word_tokenizer import WordTokenizer

ap = argparse.ArgumentParser()
ap.add_argument("--scheduler", nargs="+", default=["ddim"], choices=sorted(SCHEDULER_MAPPING))
ap.add_argument("--images", nargs="+", type=int, default=[1, 4])
ap.add_argument("--edit", action="store_true", help="time masked inpainting (init_image + mask, strength 1) next to plain sampling; fused legs only")
ap.add_argument("--repeats", type=int, default=1, help="timed calls per leg (their spread is the tool's run-to-run spread)")
ap.add_argument("--guidance_rescale", type=float, default=0.0, help="passed to the pipeline (DESIGN §2.5b)")
ap.add_argument("--identity_guidance_scale", type=float, default=None, help="passed to the pipeline: the three-branch step (DESIGN §2.5b)")
ap.add_argument("--freeu", action="store_true", help="enable FreeU with the default factors (DESIGN §2.5c)")
ap.add_argument("--freeu_version", type=int, choices=(1, 2), default=2)
ap.add_argument("--legs", nargs="+", default=None, choices=["generic", "fused eager", "graph"], help="time these legs only")
args = ap.parse_args()
guide_kw = {}
if args.guidance_rescale > 0.0:
    guide_kw["guidance_rescale"] = args.guidance_rescale
if args.identity_guidance_scale is not None:
    guide_kw["identity_guidance_scale"] = args.identity_guidance_scale

dev = torch.device("cuda:0")
steps = int(os.environ.get("STEPS", "50"))
unet, enc, text, _ = build_models(dev, "sd14", seed=0)
unet.requires_grad_(False); enc.requires_grad_(False)
with torch.device(dev):
    vae = VAEDecoder().requires_grad_(False)
tok = WordTokenizer(base_size=49408, model_max_length=77)
pipe = StableDiffusionE4TPipeline(vae=vae, text_encoder=text, tokenizer=tok, unet=unet, e4t_encoder=enc, scheduler=DDIMScheduler.stable_diffusion(),
                                  e4t_config=dict(placeholder_token="*s", domain_class_token="art", domain_embed_scale=0.1), already_added_placeholder_token=False)
if args.freeu:
    pipe.enable_freeu(version=args.freeu_version)
image = torch.rand(1, 3, 512, 512) * 2 - 1
modes = [("plain", {})]
if args.edit:
    with torch.device(dev):
        pipe.vae_encoder = VAEEncoder().requires_grad_(False)
    mask = torch.zeros(512, 512)
    mask[:, 252:] = 1.0                  # the edge is not on the latent grid: soft keep values occur
    modes.append(("edit", dict(init_image=torch.rand(1, 3, 512, 512) * 2 - 1, strength=1.0, mask_image=mask)))
legs = (("generic", False, False), ("fused eager", True, False), ("graph", True, True))
for name in args.scheduler:
    pipe.scheduler = SCHEDULER_MAPPING[name].stable_diffusion()
    for n in args.images:
        for mode, edit_kw in modes:
            for leg, fused, graph in (legs[1:] if args.edit else legs):
                if args.legs is not None and leg not in args.legs:
                    continue
                pipe._fused_sampling = fused
                kw = dict(num_inference_steps=steps, guidance_scale=7.5, num_images_per_prompt=n, image=image, output_type="np", use_graph=graph,
                          **edit_kw, **guide_kw)
                pipe("a painting of *s", **dict(kw, num_inference_steps=2))
                for _ in range(args.repeats):
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    out = pipe("a painting of *s", **kw).images
                    torch.cuda.synchronize(); dt = time.perf_counter() - t0
                    calls = len(pipe.scheduler.timesteps)
                    print(f"{name} {mode} images/call={n} {leg}: {dt:.2f} s for {calls} model calls ({dt/calls*1e3:.1f} ms/step incl. capture+decode"
                          f"{'+encode' if edit_kw else ''}) -> {n/dt:.2f} img/s; out {out.shape}", flush=True)
    pipe._fused_sampling = True
z = torch.randn(4, 4, 64, 64, device=dev) * 0.18215
vae.decode_latents(z); torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(5):
    vae.decode_latents(z)
torch.cuda.synchronize(); print(f"VAE decode B=4 512px: {(time.perf_counter()-t0)/5*1e3:.1f} ms")
