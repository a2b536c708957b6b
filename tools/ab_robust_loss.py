"""A/B of the scheduled pseudo-Huber loss (E4TTrainer(loss_type=...)) on one MI355X, same tree, same process.

  isolated: e4t_robust_loss_fwd against e4t_weighted_mse_fwd on the same operands at (16, 4, 64, 64), NCHW and NHWC pred, with mask and
            per-image weight; each forward (2 launches) is captured 200 times into one graph and the replay is timed with device events,
            so the figure is the device's time per forward, not the host's launch rate; legs alternated, median and max - min per leg.
  step:     the SD-1.4 B = 16 pre-training step, eager, with the default loss, l2 + snr_gamma (the fused weighted loss), huber + snr_gamma
            and huber alone; legs alternated, medians and max - min per leg.

    python tools/ab_robust_loss.py [--rounds 3] [--steps 5] [--no-step] [--out profiles/robust_loss_ab.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "e4t-diffusion_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--gamma", type=float, default=5.0)
ap.add_argument("--calls", type=int, default=200, help="isolated: forwards per captured graph")
ap.add_argument("--replays", type=int, default=20, help="isolated: timed replays per round")
ap.add_argument("--no-step", action="store_true", help="isolated timing only")
ap.add_argument("--out", default=None)
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


import torch  # noqa: E402

from e4t import ops  # noqa: E402
from e4t.trainer import E4TTrainer, ddpm_alphas_cumprod, huber_table, objective_coef  # noqa: E402

dev = torch.device("cuda:0")
torch.cuda.set_device(0)
hip = ops.HipBackend()
B = args.batch


# ---- isolated: the two forwards on the same operands ----
def isolated():
    shape = (B, 4, 64, 64)
    g = torch.Generator(device=dev).manual_seed(0)
    acp = ddpm_alphas_cumprod(device=dev)
    ctab = huber_table(acp, 0.1, "snr")
    t = torch.randint(0, 1000, (B,), generator=g, device=dev)
    lam = objective_coef(acp, args.gamma)[t, 2].contiguous()
    target = torch.randn(shape, generator=g, device=dev)
    mask = torch.rand((B, 64, 64), generator=g, device=dev)
    n = target.numel()
    say(f"# isolated forward, {shape}, mask + per-image weight, wd saved: {n} elements x 12 B = {12 * n / 1e6:.2f} MB per forward (2 launches); "
        f"{args.calls} forwards per graph, {args.replays} timed replays per round, {args.rounds} alternated rounds")
    for nhwc in (False, True):
        pred = torch.randn((B, 64, 64, 4) if nhwc else shape, generator=g, device=dev)
        pred = pred.permute(0, 3, 1, 2) if nhwc else pred
        calls = {"weighted_mse": lambda: hip.weighted_mse(pred, target, lam, mask),
                 "robust huber": lambda: hip.robust_loss(pred, target, ctab, t, "huber", lam, mask),
                 "robust smooth_l1": lambda: hip.robust_loss(pred, target, ctab, t, "smooth_l1", lam, mask)}
        graphs = {}
        for name, call in calls.items():
            call()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with ops.capture_guard():
                with torch.cuda.graph(graph):
                    keep = [call() for _ in range(args.calls)]
            graphs[name] = (graph, keep)
            graph.replay()
        torch.cuda.synchronize()
        us = {k: [] for k in calls}
        for rnd in range(args.rounds):
            for name, (graph, _) in graphs.items():
                graph.replay()                                       # warm
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.replays):
                    graph.replay()
                e1.record()
                torch.cuda.synchronize()
                us[name].append(e0.elapsed_time(e1) * 1e3 / (args.replays * args.calls))
        for name, v in us.items():
            med = statistics.median(v)
            say(f"{'nhwc' if nhwc else 'nchw'} {name}: median {med:.2f} us per forward (max - min {max(v) - min(v):.2f}), "
                f"{12 * n / med / 1e3:.0f} GB/s of its 12 B per element")


# ---- step: the pre-training step under the four losses ----
def step_ab():
    from bench import build_models
    gen = torch.Generator(device=dev)

    def batches(n):
        out = []
        for s in range(n):
            gen.manual_seed(1234 + s)
            out.append((torch.rand((B, 3, 512, 512), generator=gen, device=dev) * 2 - 1, torch.randint(0, 49000, (B, 77), generator=gen, device=dev),
                        torch.randint(1, 20, (B,), generator=gen, device=dev)))
        return out

    unet, enc, text, vae = build_models(dev, "sd14", seed=0)
    empty_ids = torch.tensor([[49406] + [49407] * 76], device=dev)
    tr = E4TTrainer(unet, enc, text, vae, lr=1e-6 * B, class_token_id=1125, empty_prompt_ids=empty_ids, device=dev, snr_gamma=args.gamma,
                    loss_type="huber")
    # one trainer, its options switched per leg: the attributes the constructor derives from them (coef keeps the gamma column, which only a
    # leg with snr_gamma reads; huber_tab is only read by a huber leg)
    LEGS = {"default (l2)": ("l2", None), "l2 + snr_gamma": ("l2", args.gamma), "huber + snr_gamma": ("huber", args.gamma), "huber": ("huber", None)}

    def set_leg(leg):
        tr.loss_type, tr.snr_gamma = LEGS[leg]
        tr._objective_on = tr.snr_gamma is not None or tr.noise_offset > 0

    def time_steps(pool):
        for s in range(args.warmup):
            tr.train_step(*pool[s % len(pool)])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(args.steps):
            tr.train_step(*pool[(args.warmup + s) % len(pool)])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    say(f"# step A/B, SD-1.4 512 px, B = {B}, {args.rounds} alternated rounds of {args.steps} timed steps ({args.warmup} warm-up), eager steps, "
        f"gamma = {args.gamma}, huber_c = 0.1, schedule snr")
    pool = batches(4)
    ms = {k: [] for k in LEGS}
    for rnd in range(args.rounds):
        for leg in LEGS:
            set_leg(leg)
            ms[leg].append(time_steps(pool))
            say(f"round {rnd} {leg}: {ms[leg][-1]:.2f} ms/step")
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k, v in ms.items():
        say(f"{k}: median {med[k]:.2f} ms (max - min {max(v) - min(v):.2f})")
    say(f"huber + snr_gamma over l2 + snr_gamma: {med['huber + snr_gamma'] - med['l2 + snr_gamma']:+.2f} ms/step; huber over the default step: "
        f"{med['huber'] - med['default (l2)']:+.2f} ms/step")


isolated()
if not args.no_step:
    step_ab()
if args.out:
    with open(args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out), "w") as f:
        f.write("\n".join(lines) + "\n")
