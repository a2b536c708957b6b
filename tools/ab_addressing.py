"""A/B of the GEMM / conv kernels whose operand addressing is shared code (gemm_common.h) against another build of the library (E4T_LIB=<variant .so>):
one step-sized shape per kernel variant — every tile hint, dense and 3x3 conv in the tap-major modes, the GENERAL epilogues, batch and split-K, the fused
GEGLU epilogues — graph-replayed with operands cycled through a pool larger than the caches, plus a bitwise checksum of every output.  One line per
shape: key, what the planner chose, us, checksum.  Under E4T_GEMM_REGSTAGE the same list runs the register-staged kernel on its two tiles.
    python tools/ab_addressing.py LABEL                          (several alternating runs per library, all lines into one log)
    python tools/ab_addressing.py --verdict LOG PARENT NEW       per shape: medians, the parent's spread (max - min) / median = the margin, verdict"""
import ctypes
import os
import sys

if len(sys.argv) > 1 and sys.argv[1] == "--verdict":
    import collections
    import statistics
    log, pa, nw = sys.argv[2:5]
    t, cs, chosen = collections.defaultdict(list), collections.defaultdict(set), {}
    for line in open(log):
        f = [x.strip() for x in line.split("|")]
        if len(f) == 4 and f[0].startswith("["):
            lab, key = f[0][1:].split("] ", 1)
            t[key, lab].append(float(f[2].split()[0])); cs[key].add(f[3]); chosen[key] = f[1]
    bad = 0
    print("%-62s %-52s %3s %10s %10s %8s %8s  %-9s %s" % ("shape", "kernel / plan", "n", "parent us", "new us", "spread", "delta", "checksum", "verdict"))
    for key in chosen:
        a, b = t[key, pa], t[key, nw]
        ma, mb = statistics.median(a), statistics.median(b)
        spread, delta = (max(a) - min(a)) / ma, (mb - ma) / ma
        ok = delta <= spread and len(cs[key]) == 1
        bad += not ok
        print("%-62s %-52s %3d %10.2f %10.2f %7.2f%% %+7.2f%%  %-9s %s" % (key, chosen[key], min(len(a), len(b)), ma, mb, 100 * spread, 100 * delta,
              "equal" if len(cs[key]) == 1 else "DIFFERS", "ok" if ok else "FAIL"))
    print("%d shapes, %d fail" % (len(chosen), bad))
    sys.exit(0)

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(R, "e4t-diffusion_amd"), os.path.join(R, "tests")]
import torch  # noqa: E402
from e4t import _C, ops  # noqa: E402

label = sys.argv[1] if len(sys.argv) > 1 else os.path.basename(os.environ.get("E4T_LIB", "default"))
regstage = bool(os.environ.get("E4T_GEMM_REGSTAGE"))
dev = torch.device("cuda:0")
hip = ops.HipBackend()
bf16, f32 = torch.bfloat16, torch.float32
g = torch.Generator(device=dev).manual_seed(1)
r = lambda *s: (torch.randn(*s, device=dev, generator=g) * 0.5).to(bf16)
TILES = (64, 128) if regstage else (64, 3064, 4064, 128, 3128, 4128, 160, 3160, 4160, 5256, 512, 2320)
S1, S2, UP2, S2T, S2A = 1, 2, 3, 4, 5


def graph_time(fns, iters):
    for f in fns:
        f()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for i in range(iters):
            fns[i % len(fns)]()
    gr.replay(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); gr.replay(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def csum(t):
    return int(t.view(torch.int16).to(torch.int64).sum().item()) & 0xFFFFFFFF


def report(key, chosen, fns, outs):
    t = graph_time(fns, 3 * len(fns))
    print(f"[{label}] {key} | {chosen} | {t:9.2f} us | csum {csum(outs[0]):08x}", flush=True)


def conv(B, Hin, Win, Cin, Cout, mode, Hout, Wout, tile, general=False, splitk=0):
    import kernel_checks as kc
    nset = 3
    xs = [r(B * Hin * Win, Cin) for _ in range(nset)]
    w = r(Cout, 9 * Cin) * (9 * Cin) ** -0.5
    bias = torch.randn(Cout, device=dev, generator=g)
    rb = torch.randn(B, Cout, device=dev, generator=g) if general else None      # a row bias over Hout * Wout % 32 != 0 rows: the GENERAL epilogue
    outs = [torch.empty((B * Hout * Wout, Cout), dtype=bf16, device=dev) for _ in range(nset)]
    fns = [(lambda x=x, o=o: hip.conv3x3(x, w, B, Hin, Win, Hout, Wout, mode, bias=bias, rowbias=rb, out=o, tile=tile, splitk=splitk)) for x, o in zip(xs, outs)]
    d = kc.conv_desc((B, Hin, Win, Cin, Cout, mode, Hout, Wout, tile, splitk), "bare")
    d.bias, d.rowbias, d.ldrb = 1 << 24, ((1 << 24) if general else None), (Cout if general else 0)
    sym, sk = ctypes.c_char_p(), ctypes.c_int(0)
    _C.check(hip.lib.e4t_conv3x3_kernel(ctypes.byref(d), ctypes.byref(sym), ctypes.byref(sk)), "e4t_conv3x3_kernel")
    report(f"conv mode{mode} B{B} {Hin}x{Win} {Cin}->{Cout} t{tile}{' rowbias' if general else ''}{f' sk{splitk}' if splitk else ''}", f"{sym.value.decode()} splitk{sk.value}", fns, outs)


def gemm(M, N, K, tile, gelu=False, batch=1, splitk=0, K2=0):
    nset = 3
    sh = (batch, M, K) if batch > 1 else (M, K)
    As = [r(*sh) for _ in range(nset)]
    a2 = r(M, K2) if K2 else None
    b = (r(batch, N, K + K2) if batch > 1 else r(N, K + K2)) * (K + K2) ** -0.5
    outs = [torch.empty(((batch, M, N) if batch > 1 else (M, N)), dtype=bf16, device=dev) for _ in range(nset)]
    fns = [(lambda a=a, o=o: hip.gemm(a, b, a2=a2, out=o, gelu=gelu, tile=tile, splitk=splitk)) for a, o in zip(As, outs)]
    d = _C.GemmDesc(M=M, N=N, K=K + K2, K1=K, lda=K, lda2=K2, ldb=K + K2, ldc=N, batch=batch, alpha=1.0, flags=_C.ACT_GELU if gelu else 0, tile=tile, splitk=splitk,
                    strideA=M * K if batch > 1 else 0, strideB=N * K if batch > 1 else 0, strideC=M * N if batch > 1 else 0, A=1 << 24, B=1 << 24, C=1 << 24,
                    A2=(1 << 24) if K2 else None, workspace=1 << 24, workspace_bytes=1 << 40)
    pl = _C.GemmPlan()
    hip.lib.e4t_gemm_plan(ctypes.byref(d), ctypes.byref(pl))
    report(f"gemm M{M} N{N} K{K}{f'+{K2}' if K2 else ''} t{tile}{' gelu' if gelu else ''}{f' batch{batch}' if batch > 1 else ''}{f' sk{splitk}' if splitk else ''}",
           f"tile{pl.tile} stages{pl.stages} splitk{pl.splitk}", fns, outs)


for t in TILES:
    gemm(16384, 640, 640, t)                                  # the 32 x 32 level's projections
    conv(16, 64, 64, 320, 320, S2, 32, 32, t)                  # the first Downsample2D
    conv(16, 16, 16, 1280, 1280, UP2, 32, 32, t)               # an Upsample2D conv
for t in ((64, 128) if regstage else (64, 3064, 128, 160, 512, 2320)):      # the GENERAL instantiations
    gemm(4112, 1280, 1280, t, gelu=True)
    conv(16, 60, 60, 320, 320, S2, 30, 30, t, general=True)
for t in ((64, 128) if regstage else (64, 128, 512, 2320)):
    conv(16, 32, 32, 640, 640, S2T, 64, 64, t)                 # data gradient of a Downsample2D
    conv(4, 128, 128, 128, 128, S2A, 64, 64, t)                # the VAE encoder's Downsample2D
    conv(16, 32, 32, 640, 640, S1, 32, 32, t)                  # stride 1: the channel-major walk of the same kernels
    gemm(4096, 1280, 640, t, K2=640)                           # a shortcut conv over cat([h, skip])
    gemm(1024, 1280, 5120, t, splitk=2)
    gemm(2048, 320, 320, t, batch=8)
conv(16, 8, 8, 1280, 1280, S1, 8, 8, 0)                        # the 8 x 8 level: split-K by the planner
if not regstage:
    for M, K, H in [(65536, 320, 1280), (16384, 640, 2560), (4096, 1280, 5120), (1024, 1280, 5120)]:      # the feed-forward GEMMs with the GEGLU in the epilogue
        xs = [r(M, K) for _ in range(3)]
        w, bias = r(2 * H, K) * K ** -0.5, torch.randn(2 * H, device=dev, generator=g)
        res = [hip.gemm_geglu(x, w, bias) for x in xs]
        if res[0] is not None:
            print(f"[{label}] geglu fwd M{M} K{K} H{H} | fused | {graph_time([(lambda x=x: hip.gemm_geglu(x, w, bias)) for x in xs], 9):9.2f} us | csum {csum(res[0][1]):08x}", flush=True)
            dys, w2T, u = [r(M, K) for _ in range(3)], r(H, K) * K ** -0.5, res[0][0]
            du = hip.gemm_geglu_bwd(dys[0], w2T, u)
            if du is not None:
                print(f"[{label}] geglu bwd M{M} K{K} H{H} | fused | {graph_time([(lambda dy=dy: hip.gemm_geglu_bwd(dy, w2T, u)) for dy in dys], 9):9.2f} us | csum {csum(du):08x}", flush=True)
        del xs, res
