"""A/B of token merging (e4t/tome.py) on one MI355X, same tree, same process: the SD-1.4 B = 16 pre-training step at ratio 0 and 0.5,
alternated three times; medians and max - min per leg, and the verdict (the 0.5 median must lie below the ratio-0 median by more than
the ratio-0 spread).  Optional blocks: the tuning step (every UNet weight trains) and 50-step DDIM sampling at 1 and 4 images.

    python tools/ab_tome.py [--ratio 0.5] [--rounds 3] [--steps 5] [--tuning] [--sampling] [--out profiles/tome_ab.txt]
    rocprofv3 --kernel-trace --stats -- python tools/ab_tome.py --rounds 1 --only-tome     (per-launch times of the tome_* kernels)"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "e4t-diffusion_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from bench import build_models  # noqa: E402
from e4t import tome  # noqa: E402
from e4t.trainer import E4TTrainer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ratio", type=float, default=0.5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--only-tome", action="store_true", help="run the ToMe leg alone (for a kernel trace)")
ap.add_argument("--tuning", action="store_true")
ap.add_argument("--sampling", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
torch.cuda.set_device(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def set_ratio(unet, ratio):
    tome.remove_tome(unet)
    if ratio > 0:
        tome.apply_tome(unet, ratio, generator=torch.Generator().manual_seed(0))


def time_steps(tr, pool, steps, warmup):
    for s in range(warmup):
        tr.train_step(*pool[s % len(pool)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(steps):
        tr.train_step(*pool[(warmup + s) % len(pool)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def ab(name, tr, unet, pool):
    legs = {0.0: [], args.ratio: []}
    order = [args.ratio] if args.only_tome else [0.0, args.ratio]
    for rnd in range(args.rounds):
        for ratio in order:
            set_ratio(unet, ratio)
            ms = time_steps(tr, pool, args.steps, args.warmup)
            legs[ratio].append(ms)
            say(f"{name} round {rnd} ratio {ratio}: {ms:.2f} ms/step")
    set_ratio(unet, 0.0)
    if args.only_tome:
        return
    m0, m1 = statistics.median(legs[0.0]), statistics.median(legs[args.ratio])
    s0, s1 = max(legs[0.0]) - min(legs[0.0]), max(legs[args.ratio]) - min(legs[args.ratio])
    say(f"{name}: ratio 0 median {m0:.2f} ms (max - min {s0:.2f}); ratio {args.ratio} median {m1:.2f} ms (max - min {s1:.2f}); "
        f"gain {m0 - m1:.2f} ms = {100 * (m0 - m1) / m0:.1f} %; accepted (gain > ratio-0 spread): {m0 - m1 > s0}")


gen = torch.Generator(device=dev)
B = args.batch


def batches(n):
    out = []
    for s in range(n):
        gen.manual_seed(1234 + s)
        out.append((torch.rand((B, 3, 512, 512), generator=gen, device=dev) * 2 - 1, torch.randint(0, 49000, (B, 77), generator=gen, device=dev),
                    torch.randint(1, 20, (B,), generator=gen, device=dev)))
    return out


unet, enc, text, vae = build_models(dev, "sd14", seed=0)
empty_ids = torch.tensor([[49406] + [49407] * 76], device=dev)
tr = E4TTrainer(unet, enc, text, vae, lr=1e-6 * B, class_token_id=1125, empty_prompt_ids=empty_ids, device=dev)
say(f"# token merging A/B, SD-1.4 512 px, B = {B}, {args.rounds} alternated rounds of {args.steps} timed steps ({args.warmup} warm-up), eager steps, no prefetch")
ab("pretrain step", tr, unet, batches(4))

if args.tuning:
    del tr
    torch.cuda.empty_cache()
    unet.requires_grad_(True)
    tr = E4TTrainer(unet, enc, text, vae, lr=1e-6, class_token_id=1125, empty_prompt_ids=empty_ids, device=dev, tuning=True, max_grad_norm=1.0)
    ab("tuning step", tr, unet, batches(2))
    del tr
    torch.cuda.empty_cache()

if args.sampling:
    from e4t.pipeline_stable_diffusion_e4t import StableDiffusionE4TPipeline
    from e4t.schedulers import DDIMScheduler
    from e4t.vae import VAEDecoder
    from word_tokenizer import WordTokenizer
    unet.requires_grad_(False); enc.requires_grad_(False)
    with torch.device(dev):
        dec = VAEDecoder().requires_grad_(False)
    pipe = StableDiffusionE4TPipeline(vae=dec, text_encoder=text, tokenizer=WordTokenizer(base_size=49408, model_max_length=77), unet=unet, e4t_encoder=enc,
                                      scheduler=DDIMScheduler.stable_diffusion(),
                                      e4t_config=dict(placeholder_token="*s", domain_class_token="art", domain_embed_scale=0.1), already_added_placeholder_token=False)
    image = torch.rand(1, 3, 512, 512) * 2 - 1
    for n in (1, 4):
        for ratio in (0.0, args.ratio):
            set_ratio(unet, ratio)
            kw = dict(guidance_scale=7.5, num_images_per_prompt=n, image=image, output_type="latent")
            pipe("a painting of *s", num_inference_steps=2, **kw)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            pipe("a painting of *s", num_inference_steps=50, **kw)
            torch.cuda.synchronize()
            say(f"sampling 50 DDIM steps, {n} image(s), ratio {ratio}: {(time.perf_counter() - t0) / 50 * 1e3:.2f} ms/step")
    set_ratio(unet, 0.0)

if args.out:
    with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
