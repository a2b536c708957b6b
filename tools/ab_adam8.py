"""A/B of AdamW with block-wise 8-bit moments (e4t_adamw8) on one MI355X, same tree, same process.

kernels (default): e4t_adamw, e4t_adamw8 and their EMA forms over n parameters, n = the trainable-parameter count of the tuning configuration and
that of pre-training (SD-1.4; --sizes overrides): per leg a warm-up, then --groups groups of --reps launches timed between two events, the legs
alternated inside every group; microseconds per launch (median of the groups, max - min as the spread), achieved bytes/s by each kernel's own
launch-log byte count, the time ratio next to the traffic model's (16.06 / 28 = 0.57; 24.06 / 36 = 0.67 with the EMA), and the verdict: adamw8
is faster than adamw_kernel by more than the spread between the repeated groups.

--step: one full-size tuning step (SD-1.4, B = 1, max_grad_norm = 1, as tools/glue_profile.py builds it) with 32- and with 8-bit state, each in a
trainer of its own built and dropped in turn: ms per step and the allocated memory after the steps.

    python tools/ab_adam8.py [--groups 5] [--reps 20] [--out profiles/adam8_ab.txt]
    python tools/ab_adam8.py --step [--steps 5] [--out profiles/adam8_ab.txt]      (appends)"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "e4t-diffusion_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

# select_trainable over bench.build_models("sd14"): tuning=True (the whole UNet, its weight offsets and the encoder) / pre-training
SIZES = {"tuning": 1234095524, "pretrain": 374574560}

ap = argparse.ArgumentParser()
ap.add_argument("--groups", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--sizes", default=None, help="comma-separated element counts instead of the two configurations'")
ap.add_argument("--step", action="store_true", help="the full-size tuning step with 32- and 8-bit state instead of the kernels")
ap.add_argument("--steps", type=int, default=5)
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


import torch  # noqa: E402

from e4t import ops  # noqa: E402
from e4t.optimization import Adam8State, quantize_blockwise  # noqa: E402

dev = torch.device("cuda:0")
torch.cuda.set_device(0)
HP = (1e-3, 0.9, 0.999, 1e-8, 1e-2)
EMA_W = 1e-4

if args.step:
    import bench
    from e4t.trainer import E4TTrainer
    say(f"# full-size tuning step (SD-1.4, B = 1, tuning=True, max_grad_norm = 1, eager), {args.steps} timed steps after 2 warm-up steps per leg")
    res = {}
    for bits in (32, 8):
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        unet, enc, text, vae = bench.build_models(dev, "sd14", 0)
        tr = E4TTrainer(unet, enc, text, vae, lr=1e-6, class_token_id=1125, empty_prompt_ids=torch.tensor([[49406] + [49407] * 76], device=dev), device=dev,
                        tuning=True, max_grad_norm=1.0, optimizer_state_bits=bits)
        g = torch.Generator(device=dev).manual_seed(1234)
        batch = (torch.rand((1, 3, 512, 512), generator=g, device=dev) * 2 - 1, torch.randint(0, 49000, (1, 77), generator=g, device=dev),
                 torch.randint(1, 20, (1,), generator=g, device=dev))
        for _ in range(2):
            tr.train_step(*batch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            tr.train_step(*batch)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / args.steps * 1e3
        state = tr.adam8.nbytes() if bits == 8 else 8 * tr.flat.numel
        res[bits] = (ms, torch.cuda.memory_allocated(), torch.cuda.max_memory_allocated(), state, tr.flat.numel)
        say(f"{bits}-bit state: {ms:.2f} ms/step, {tr.flat.numel} trained parameters, optimiser state {state / 1e6:.1f} MB, allocated after the steps "
            f"{res[bits][1] / 1e6:.1f} MB, peak {res[bits][2] / 1e6:.1f} MB")
        del tr, unet, enc, text, vae
    say(f"8-bit against 32-bit: {res[8][0] - res[32][0]:+.2f} ms/step, allocated {(res[8][1] - res[32][1]) / 1e6:+.1f} MB, peak {(res[8][2] - res[32][2]) / 1e6:+.1f} MB "
        f"(optimiser state alone: {(res[8][3] - res[32][3]) / 1e6:+.1f} MB)")
    finish("a")
    sys.exit(0)

hip = ops.HipBackend()
sizes = [int(s) for s in args.sizes.split(",")] if args.sizes else list(SIZES.values())
names = {v: k for k, v in SIZES.items()}
say(f"# adamw / adamw8 kernels on one GPU, one process: {args.groups} groups of {args.reps} launches per leg (legs alternated inside a group, "
    f"{args.warmup} warm-up launches per leg), times between two events around the {args.reps} launches")
for n in sizes:
    gen = torch.Generator(device=dev).manual_seed(7)
    p = torch.randn(n, generator=gen, device=dev)
    g = torch.randn(n, generator=gen, device=dev)
    m = torch.randn(n, generator=gen, device=dev) * 0.1
    v = torch.randn(n, generator=gen, device=dev).abs() * 0.01
    ema = p.clone()
    st = Adam8State(n, dev)
    chunk = 1 << 24                                   # a valid, busy 8-bit state: the same moments through the definition
    for o in range(0, n, chunk):
        for (q, a), x, code in (((st.qm, st.absmax_m), m, st.code_m), ((st.qv, st.absmax_v), v, st.code_v)):
            qq, aa = quantize_blockwise(x[o:o + chunk], code)
            q[o:o + chunk] = qq
            a[o // 256:o // 256 + aa.numel()] = aa
    nb = -(-n // 256)
    legs = {
        "adamw_kernel": (28.0 * n, lambda: hip.adamw(p, g, m, v, *HP, 3)),
        "adamw8_kernel": (16.0 * n + 16.0 * nb, lambda: hip.adamw8(p, g, st.qm, st.qv, st.absmax_m, st.absmax_v, st.code_m, st.code_v, *HP, 3)),
        "adamw_ema_kernel": (36.0 * n, lambda: hip.adamw_ema(p, g, m, v, ema, *HP, 3, 1.0, EMA_W)),
        "adamw8_ema_kernel": (24.0 * n + 16.0 * nb, lambda: hip.adamw8(p, g, st.qm, st.qv, st.absmax_m, st.absmax_v, st.code_m, st.code_v, *HP, 3, ema=ema,
                                                                      ema_w=EMA_W)),
    }
    us = {k: [] for k in legs}
    for k, (_, fn) in legs.items():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.groups):
        for k, (_, fn) in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            e1.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3 / args.reps)
    say(f"n = {n}" + (f" ({names[n]})" if n in names else ""))
    med = {k: statistics.median(t) for k, t in us.items()}
    spread = {k: max(t) - min(t) for k, t in us.items()}
    for k, (nbytes, _) in legs.items():
        say(f"  {k}: {med[k]:.1f} us per launch (max - min over the groups {spread[k]:.1f}), {nbytes / 1e6:.1f} MB -> {nbytes / med[k] / 1e6:.2f} TB/s")
    for k8, k32, model in (("adamw8_kernel", "adamw_kernel", 16.0625 / 28), ("adamw8_ema_kernel", "adamw_ema_kernel", 24.0625 / 36)):
        gain, noise = med[k32] - med[k8], max(spread[k8], spread[k32])
        say(f"  {k8} / {k32}: time ratio {med[k8] / med[k32]:.3f} (traffic model {model:.3f}); faster by {gain:.1f} us, spread {noise:.1f} us; "
            f"faster by more than the spread: {gain > noise}")
    del p, g, m, v, ema, st
    torch.cuda.empty_cache()
finish("w")
