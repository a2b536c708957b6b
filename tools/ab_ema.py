"""A/B of the EMA of the trained weights (E4TTrainer(ema_decay=...)) on one MI355X, same tree, same process: the SD-1.4 B = 16
pre-training step with the EMA off, fused into the AdamW kernels, and as a separate pass (the plain AdamW launches, then e4t_ema_update over the
flat buffer); the legs alternated three times, medians and max - min per leg, and the verdict: the fused form is kept only if its median lies
below the separate pass's by more than the off leg's max - min.

    python tools/ab_ema.py [--rounds 3] [--steps 5] [--out profiles/ema_ab.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ab_ema.py --rounds 1 --steps 3 --sizes DIR/sizes.json
    python tools/ab_ema.py --rates DIR [--out profiles/ema_ab.txt]      (per-launch times and GB/s of the five kernels from that trace; appends)"""
import argparse
import csv
import glob
import json
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
ap.add_argument("--decay", type=float, default=0.9999)
ap.add_argument("--sizes", default=None, help="write the element counts of the launches here (json), for --rates")
ap.add_argument("--rates", default=None, metavar="DIR", help="no GPU work: read the rocprofv3 kernel trace (csv) and sizes.json under DIR")
ap.add_argument("--out", default=None)
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def finish(mode):
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, mode) as f:
            f.write("\n".join(lines) + "\n")


# bytes per parameter of each kernel (its launch-log figure) and which element count it runs over
KERNELS = {"adamw_kernel": (28, "rest"), "adamw_ema_kernel": (36, "rest"), "adamw_rank_kernel": (24, "stack"), "adamw_rank_ema_kernel": (32, "stack"),
           "ema_update_kernel": (12, "all")}

if args.rates:
    sizes = json.load(open(os.path.join(args.rates, "sizes.json")))
    trace = sorted(glob.glob(os.path.join(args.rates, "**", "*kernel_trace.csv"), recursive=True))
    assert trace, f"no *kernel_trace.csv under {args.rates}"
    durs = {k: [] for k in KERNELS}
    for path in trace:
        for row in csv.DictReader(open(path)):
            name = row["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].split("<")[0]
            if name in durs:
                durs[name].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    say(f"# per-launch rates from one rocprofv3 --kernel-trace --stats run (nothing else traced); stack {sizes['stack']} + rest {sizes['rest']} = {sizes['all']} parameters")
    rate = {}
    for k, (bpp, which) in KERNELS.items():
        if not durs[k]:
            say(f"{k}: not in the trace")
            continue
        us = statistics.median(durs[k])
        rate[k] = bpp * sizes[which] / us / 1e3
        say(f"{k}: {len(durs[k])} launches, median {us:.1f} us (min {min(durs[k]):.1f}, max {max(durs[k]):.1f}), {bpp} B x {sizes[which]} = "
            f"{bpp * sizes[which] / 1e6:.1f} MB -> {rate[k]:.0f} GB/s")
    for fused, plain in (("adamw_ema_kernel", "adamw_kernel"), ("adamw_rank_ema_kernel", "adamw_rank_kernel")):
        if fused in rate and plain in rate:
            say(f"{fused} / {plain}: {rate[fused] / rate[plain]:.3f} of its sibling's GB/s (allowance for the fifth stream: 0.9)")
    finish("a")
    sys.exit(0)

import torch  # noqa: E402

from bench import build_models  # noqa: E402
from e4t import ops  # noqa: E402
from e4t.optimization import ema_weight  # noqa: E402
from e4t.trainer import E4TTrainer  # noqa: E402

dev = torch.device("cuda:0")
torch.cuda.set_device(0)
B = args.batch
gen = torch.Generator(device=dev)


def batches(n):
    out = []
    for s in range(n):
        gen.manual_seed(1234 + s)
        out.append((torch.rand((B, 3, 512, 512), generator=gen, device=dev) * 2 - 1, torch.randint(0, 49000, (B, 77), generator=gen, device=dev),
                    torch.randint(1, 20, (B,), generator=gen, device=dev)))
    return out


def time_steps(tr, pool, steps, warmup, separate):
    def step(s):
        tr.train_step(*pool[s % len(pool)])
        if separate:          # the pass of its own: the rule alone over the flat buffer, behind the plain launches of the step
            ops.backend().ema_update(average, tr.flat.data, ema_weight(args.decay, tr.step_count))
    for s in range(warmup):
        step(s)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(steps):
        step(warmup + s)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


unet, enc, text, vae = build_models(dev, "sd14", seed=0)
empty_ids = torch.tensor([[49406] + [49407] * 76], device=dev)
tr = E4TTrainer(unet, enc, text, vae, lr=1e-6 * B, class_token_id=1125, empty_prompt_ids=empty_ids, device=dev, ema_decay=args.decay)
average = tr.ema
n, rows, cols = tr._stack_shape
sizes = dict(stack=n * rows * cols, rest=tr.flat.numel - n * rows * cols, all=tr.flat.numel)
if args.sizes:
    json.dump(sizes, open(args.sizes, "w"))


def set_leg(leg):
    """fused: the trainer as built; off and separate: the trainer as built without ema_decay (no average: the plain launches)"""
    tr.ema = average if leg == "fused" else None


say(f"# EMA A/B, SD-1.4 512 px, B = {B}, {sizes['all']} trained parameters, {args.rounds} alternated rounds of {args.steps} timed steps "
    f"({args.warmup} warm-up), eager steps, no prefetch")
pool = batches(4)
legs = {"off": [], "fused": [], "separate": []}
for rnd in range(args.rounds):
    for leg in legs:
        set_leg(leg)
        ms = time_steps(tr, pool, args.steps, args.warmup, leg == "separate")
        legs[leg].append(ms)
        say(f"round {rnd} EMA {leg}: {ms:.2f} ms/step")
med = {k: statistics.median(v) for k, v in legs.items()}
spread = {k: max(v) - min(v) for k, v in legs.items()}
for k in legs:
    say(f"EMA {k}: median {med[k]:.2f} ms (max - min {spread[k]:.2f})")
gain = med["separate"] - med["fused"]
say(f"fused below separate by {gain:.2f} ms (expected from bytes: {sizes['all']} x 8 B = {8 * sizes['all'] / 1e9:.2f} GB fused against "
    f"{12 * sizes['all'] / 1e9:.2f} GB as a pass of its own); off leg's max - min {spread['off']:.2f} ms; "
    f"fused kept (gain > off spread): {gain > spread['off']}; cost of the fused EMA over off: {med['fused'] - med['off']:.2f} ms/step")
finish("w")
