"""FreeU (e4t/freeu.py, csrc/freeu.hip) on one MI355X: the kernel pair against the stock composition on the device, same tensors, same
process, timed between events and alternated.

    python tools/ab_freeu.py [--rounds 3] [--iters 200] [--out profiles/freeu_ab.txt]

The stock composition is what the usual implementation runs on the NHWC maps this code base holds:
    skip      permute -> float -> fftn -> fftshift -> mask -> ifftshift -> ifftn -> real -> cast -> permute
    backbone  permute -> mean over channels -> min / max per image -> normalise -> scale the first half -> permute
Shapes: SD-1.4's marked ResBlocks at 512 px, B = 2 (one guided image).  Also prints each kernel's own time (events around `iters` launches
of one kernel) with the bytes it has to move, and the outputs' agreement with the composition (rel-L2; the composition rounds to bf16 too)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "e4t-diffusion_amd"), ROOT):
    sys.path.insert(0, p)
from e4t import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
torch.cuda.set_device(0)
hip = ops.HipBackend()
bf16 = torch.bfloat16
lines = []
SHAPES = [(2, 8, 8, 1280, 1280), (2, 16, 16, 1280, 640), (2, 32, 32, 640, 320), (2, 64, 64, 640, 320)]       # (B, H, W, C_h, C_k)
BS = (1.4, 0.2)


def say(s):
    print(s, flush=True)
    lines.append(s)


def stock(h, k, B, H, W, b, s, version):
    hh = h.view(B, H, W, -1).permute(0, 3, 1, 2)
    kk = k.view(B, H, W, -1).permute(0, 3, 1, 2)
    half = hh.shape[1] // 2
    if version == 2:
        m = hh.float().mean(1, keepdim=True)
        mx = m.view(B, -1).max(dim=-1).values.view(B, 1, 1, 1)
        mn = m.view(B, -1).min(dim=-1).values.view(B, 1, 1, 1)
        scale = (b - 1) * ((m - mn) / (mx - mn)) + 1
    else:
        scale = b
    h2 = torch.cat([(hh[:, :half].float() * scale).to(h.dtype), hh[:, half:]], 1)
    f = torch.fft.fftshift(torch.fft.fftn(kk.float(), dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones((B, kk.shape[1], H, W), device=k.device)
    mask[..., H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1] = s
    k2 = torch.fft.ifftn(torch.fft.ifftshift(f * mask, dim=(-2, -1)), dim=(-2, -1)).real.to(k.dtype)
    return (h2.permute(0, 2, 3, 1).reshape(B * H * W, -1).contiguous(), k2.permute(0, 2, 3, 1).reshape(B * H * W, -1).contiguous())


def timed(fn, iters):
    """us per call: `iters` calls between two events, after a warm-up"""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


say(f"# FreeU kernel pair vs the stock composition, b = {BS[0]}, s = {BS[1]}; us per call, {args.iters} calls between two events, "
    f"{args.rounds} alternated rounds, median (min .. max)")
for version in (2, 1):
    for B, H, W, Ch, Ck in SHAPES:
        g = torch.Generator(device=dev).manual_seed(H)
        h = torch.randn((B * H * W, Ch), generator=g, device=dev).to(bf16)
        k = torch.randn((B * H * W, Ck), generator=g, device=dev).to(bf16)
        ws = hip.freeu_stats(h, k, B, H, W, version)
        oh, ok = torch.empty_like(h), torch.empty_like(k)

        def pair():
            hip.freeu_stats(h, k, B, H, W, version, ws=ws)
            hip.freeu_apply(h, k, ws, B, H, W, BS[0], BS[1], version, out_h=oh, out_k=ok)

        legs = {"pair": [], "stock": [], "stats": [], "apply": []}
        for _ in range(args.rounds):
            legs["pair"].append(timed(pair, args.iters))
            legs["stock"].append(timed(lambda: stock(h, k, B, H, W, BS[0], BS[1], version), max(args.iters // 4, 10)))
            legs["stats"].append(timed(lambda: hip.freeu_stats(h, k, B, H, W, version, ws=ws), args.iters))
            legs["apply"].append(timed(lambda: hip.freeu_apply(h, k, ws, B, H, W, BS[0], BS[1], version, out_h=oh, out_k=ok), args.iters))
        pair()
        sh, sk = stock(h, k, B, H, W, BS[0], BS[1], version)
        med = {n: statistics.median(v) for n, v in legs.items()}
        fmt = lambda n: f"{med[n]:.1f} ({min(legs[n]):.1f} .. {max(legs[n]):.1f})"      # noqa: E731
        n_el = B * H * W
        stats_bytes = 2.0 * n_el * (Ck + (Ch if version == 2 else 0))
        apply_bytes = 4.0 * n_el * (Ch + Ck)
        say(f"v{version} {H}x{W}x{Ch}+{Ck} B={B}: pair {fmt('pair')}  stock {fmt('stock')}  -> x{med['stock'] / med['pair']:.1f};  "
            f"stats {fmt('stats')} = {stats_bytes / med['stats'] / 1e3:.0f} GB/s of the {stats_bytes / 1e6:.2f} MB it reads,  "
            f"apply {fmt('apply')} = {apply_bytes / med['apply'] / 1e3:.0f} GB/s of the {apply_bytes / 1e6:.2f} MB it moves;  "
            f"rel-L2 vs stock h' {rel(oh, sh):.1e} k' {rel(ok, sk):.1e}")

if args.out:
    with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
