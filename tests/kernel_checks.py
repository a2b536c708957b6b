"""Per-kernel parity checks: HIP op (through the C ABI) vs the torch restatement in emu_backend.py,
on the same seeded inputs.  Each check returns a list of (label, rel_l2_error, tolerance).
Used by tests/test_kernels_gpu.py (pytest, -m gpu) and tests/gpu_report.py (prints everything).

Tolerances (stated per check): outputs are bf16 (8 mantissa bits, eps = 2^-8 = 3.9e-3) computed from
bf16 inputs with fp32 accumulation, so the relative L2 error against an fp32 evaluation of the same
bf16 inputs is bounded by ~eps/sqrt(3) per output rounding (~2.3e-3) plus accumulation-order noise;
we allow 6e-3 for single-rounding kernels, 1.5e-2 where an intermediate (P, dS) is also rounded to
bf16 inside the kernel, 1e-5 for fp32-only kernels.

Importable without a GPU: the attention, conv, norm, GEMM, weight-offset and streaming case lists (stream_value_cases, stream_layout_cases),
the stream_ref64_* definitions, stream_slices() (tests/test_streaming_slices_cpu.py), slices(), conv_slices(), norm_slices(), gemm_slices() and
wo_slices(), norm_plan() and the fp64 norm, GEMM and weight-offset references are shared with CPU tests (test_gemm_dispatch.py,
test_attention_slices_cpu.py, test_conv_slices_cpu.py, test_norm_slices_cpu.py, test_norm_plan_cpu.py, test_gemm_slices_cpu.py, test_wo_slices_cpu.py).
"""
from __future__ import annotations

import math
from collections import namedtuple

import torch

from emu_backend import EmuBackend, CONV_S1, CONV_S2, CONV_UP2, CONV_S2T

bf16, f32 = torch.bfloat16, torch.float32
TOL1, TOL2, TOLF = 6e-3, 1.5e-2, 2e-5


def rel(a, b):
    a, b = a.float(), b.float()
    d = (a - b).norm()
    n = b.norm()
    if not torch.isfinite(d):
        return float("inf")
    return float(d / (n + 1e-20))


def rnd(g, *shape, scale=1.0, dtype=bf16, dev="cuda"):
    return (torch.randn(*shape, generator=g, device=dev, dtype=f32) * scale).to(dtype)


def gen(seed, dev="cuda"):
    return torch.Generator(device=dev).manual_seed(seed)


def check_probe(hip, emu, dev):
    rows, cols = hip.probe_mfma(dev)
    l = torch.arange(64, device=dev)[:, None]
    r = torch.arange(16, device=dev)[None, :]
    exp_rows = ((r & 3) + 8 * (r >> 2) + 4 * (l >> 5) + 1).float()
    exp_cols = ((l & 31) + 1).float().expand(64, 16)
    return [("mfma32 row map", rel(rows, exp_rows), 0.0), ("mfma32 col map", rel(cols, exp_cols), 0.0)]


# the shapes of check_gemm as plain data (tests/test_gemm_dispatch.py pins their kernels through check_gemm_pinned())
CHECK_GEMM_NT = [  # M, N, K, tile, splitk
    (256, 256, 128, 0, 0), (200, 72, 64, 0, 0), (1000, 320, 320, 128, 1), (130, 200, 1032, 64, 3),
    (16, 1280, 1280, 0, 0), (4096, 640, 2560, 0, 0), (64, 64, 4096, 0, 0), (1000, 200, 328, 256, 1), (2048, 256, 64, 256, 1),
    (700, 320, 1280, 256, 2), (900, 320, 384, 160, 1), (300, 480, 128, 160, 2), (513, 200, 72, 160, 1),
    (512, 512, 512, 512, 1), (700, 520, 256, 512, 1), (300, 256, 64, 512, 1), (1000, 300, 128, 512, 1), (513, 1000, 1152, 512, 2),
    (2048, 1280, 1920, 512, 0), (257, 64, 192, 512, 1),
    (4096, 1280, 10240, 0, 0), (4096, 2560, 8192, 0, 0),       # auto: K-deep, 64-255 tiles of 256 x 256 -> ping-pong + split-K (3 | 1)
    (900, 384, 512, 5256, 1), (5000, 640, 320, 5256, 1),         # 256 x 128 with 32-wide K-tiles: ragged M, N one and a half / five column tiles
    # k-step-phased ping-pong tile (gemm_pq_kernel): 256 x 320 (wave tile 64 x 160); ragged M / N, one K-tile, split-K
    (1000, 320, 320, 2320, 1), (700, 640, 256, 2320, 1), (300, 200, 64, 2320, 1), (4096, 1280, 2560, 2320, 0), (513, 1000, 1152, 2320, 2),
    (65536, 320, 320, 2320, 1), (16384, 640, 640, 2320, 0),
]
CHECK_GEMM_TN = [(64, 128, 128, 1), (1000, 320, 320, 0), (4096, 960, 320, 0), (777, 200, 72, 3), (65536, 320, 320, 0),
                 (1232, 2560, 768, 0), (130, 8, 1280, 1)]      # K, M, N, splitk
CHECK_GEMM_COLSTATS = [(256, 128, 128, 0), (4096, 320, 320, 160), (1024, 640, 1280, 128), (2048, 512, 2304, 512), (192, 72, 64, 64),
                       (4096, 320, 320, 160), (8192, 256, 128, 128), (66560, 640, 192, 160), (34816, 128, 64, 128),      # more than 65536 rows, K = 192, one K-tile
                       (4096, 320, 320, 2320), (8192, 640, 640, 2320)]      # M, N, K, tile
CHECK_GEMM_TAIL = [(4112, 1280, 1280, dict(f32=True)), (4112, 5120, 1280, dict(gelu=True)), (4112, 1280, 5120, dict(f32=True)), (4112, 3840, 1280, {}),
                   (8224, 1280, 1280, dict(res=True)), (8224, 5120, 1280, dict(gelu=True)), (4096 + 1, 1280, 1280, dict(res=True)), (4096 + 31, 3840, 1280, {}),
                   (4112, 1280, 1296, dict(f32=True)), (2056, 1280, 5120, {})]
CHECK_GEMM_F32RES = [(4112, 1280, 1280, 0), (4112, 1280, 5120, 0), (1000, 1280, 320, 160), (700, 512, 256, 512), (513, 200, 64, 64), (900, 384, 96, 5256),
                     (1000, 640, 320, 2320)]      # M, N, K, tile
CHECK_GEMM_PQ_GENERAL = [(1000, 640, 320), (4096, 320, 1280), (513, 960, 64)]
CHECK_GEMM_PANELS = [(3, 257, 640, 128, 256, bf16), (16, 257, 5120, 1280, 256, bf16), (2, 520, 320, 64, 512, f32), (5, 257, 960, 192, 256, bf16)]      # B, T, N, K, panel rows, C type


def check_gemm(hip, emu, dev):
    out = []
    cases = CHECK_GEMM_NT
    for i, (M, N, K, tile, sk) in enumerate(cases):
        g = gen(10 + i, dev)
        a, b = rnd(g, M, K, dev=dev), rnd(g, N, K, scale=K ** -0.5, dev=dev)
        bias = rnd(g, N, dtype=f32, dev=dev)
        res = rnd(g, M, N, dev=dev)
        y = hip.gemm(a, b, bias=bias, residual=res, tile=tile, splitk=sk)
        yr = emu.gemm(a, b, bias=bias, residual=res)
        out.append((f"gemm {M}x{N}x{K} t{tile} s{sk} bias+res", rel(y, yr), TOL1))
    # TN: contraction over the rows (weight gradients)
    for i, (K, M, N, sk) in enumerate(CHECK_GEMM_TN):
        g = gen(40 + i, dev)
        a, b = rnd(g, K, M + 8, dev=dev)[:, :M], rnd(g, K, N, scale=K ** -0.5, dev=dev)
        out.append((f"gemm_tn K{K} M{M} N{N} s{sk}", rel(hip.gemm_tn(a, b, splitk=sk), emu.gemm_tn(a, b)), TOLF * 50))
    g = gen(48, dev)
    a, b = rnd(g, 500, 320, dev=dev), rnd(g, 500, 328, scale=0.05, dev=dev)
    c1 = rnd(g, 320, 328, dtype=f32, dev=dev); c2 = c1.clone()
    hip.gemm_tn(a, b, out=c1, accum=True); emu.gemm_tn(a, b, out=c2, accum=True)
    out.append(("gemm_tn fp32 accumulate", rel(c1, c2), TOLF * 50))
    wide = torch.zeros(320, 700, dtype=f32, device=dev); wide2 = wide.clone()
    hip.gemm_tn(a, b, out=wide[:, 100:428]); emu.gemm_tn(a, b, out=wide2[:, 100:428])
    out.append(("gemm_tn into a column slice", rel(wide, wide2), TOLF * 50))
    # column statistics left by the epilogue for the consuming GroupNorm (all tile variants; with / without residual)
    for i, (M, N, K, tile) in enumerate(CHECK_GEMM_COLSTATS):
        g = gen(60 + i, dev)
        a, b = rnd(g, M, K, dev=dev), rnd(g, N, K, scale=K ** -0.5, dev=dev)
        res = rnd(g, M, N, dev=dev) if i % 2 == 0 else None
        y = hip.gemm(a, b, bias=rnd(g, N, dtype=f32, dev=dev), residual=res, tile=tile, splitk=1, colstats=True)
        cs = getattr(y, "_e4t_colstats", None)
        blk = y.float().reshape(M // 32, 32, N)
        ref = torch.stack([blk.sum(1), (blk * blk).sum(1)], dim=-1)
        out.append((f"gemm {M}x{N}x{K} t{tile} colstats", rel(cs, ref) if cs is not None else 1.0, 1e-5))
    g = gen(30, dev)
    # two-source A, gelu, fp32 out, accumulate, rowbias
    M, N, K1, K2 = 384, 192, 128, 64
    a1, a2, b = rnd(g, M, K1, dev=dev), rnd(g, M, K2, dev=dev), rnd(g, N, K1 + K2, scale=0.07, dev=dev)
    out.append(("gemm two-source A", rel(hip.gemm(a1, b, a2=a2), emu.gemm(a1, b, a2=a2)), TOL1))
    out.append(("gemm two-source A t512", rel(hip.gemm(a1, b, a2=a2, tile=512), emu.gemm(a1, b, a2=a2)), TOL1))
    out.append(("gemm gelu fp32-out t512", rel(hip.gemm(a1, b[:, :K1].contiguous(), gelu=True, out_dtype=f32, tile=512),
                                                emu.gemm(a1, b[:, :K1].contiguous(), gelu=True, out_dtype=f32)), TOLF * 50))
    out.append(("gemm gelu", rel(hip.gemm(a1, b[:, :K1].contiguous(), gelu=True), emu.gemm(a1, b[:, :K1].contiguous(), gelu=True)), TOL1))
    for t in (3064, 512, 2320):      # the GENERAL epilogue instantiations of the 3-stage 64 tile and the ping-pong kernels
        out.append((f"gemm gelu t{t}", rel(hip.gemm(a1, b[:, :K1].contiguous(), gelu=True, tile=t), emu.gemm(a1, b[:, :K1].contiguous(), gelu=True)), TOL1))
        out.append((f"gemm two-source A t{t}", rel(hip.gemm(a1, b, a2=a2, tile=t), emu.gemm(a1, b, a2=a2)), TOL1))
    c0 = rnd(g, M, N, dtype=f32, dev=dev)
    c1, c2 = c0.clone(), c0.clone()
    hip.gemm(a1, b[:, :K1].contiguous(), out=c1, accum=True, alpha=0.5)
    emu.gemm(a1, b[:, :K1].contiguous(), out=c2, accum=True, alpha=0.5)
    out.append(("gemm fp32 out + accumulate + alpha", rel(c1, c2), TOLF * 50))
    # tail rows (round 5): M = 128 k + r, r <= 32 — the tile grid covers M - r rows, gemm_tail() computes the rest at the end of the launch
    # (the CLIP-ViT's 16 x 257 = 4112 token rows).  The tail rows are ALSO compared on their own: 16 of 4112 rows move the whole-matrix
    # rel-L2 by 6 % when they are garbage but a subtler error would drown in it.
    gt = gen(35, dev)
    import ctypes as _ct
    from e4t import _C as _Cm
    for (Mt, Nt, Kt, kw) in CHECK_GEMM_TAIL:
        at, bt = rnd(gt, Mt, Kt, dev=dev), rnd(gt, Nt, Kt, scale=Kt ** -0.5, dev=dev)
        bi = rnd(gt, Nt, dtype=f32, dev=dev)
        res = rnd(gt, Mt, Nt, dtype=f32 if kw.get("f32") else bf16, dev=dev) if (kw.get("f32") or kw.get("res")) else None
        args = dict(bias=bi, residual=res, gelu=bool(kw.get("gelu")), out_dtype=f32 if kw.get("f32") else bf16)
        d = _Cm.GemmDesc(M=Mt, N=Nt, K=Kt, K1=Kt, lda=Kt, ldb=Kt, ldc=Nt, batch=1, alpha=1.0,
                         flags=(_Cm.OUT_F32 | _Cm.RES_F32 if kw.get("f32") else 0) | (_Cm.ACT_GELU if kw.get("gelu") else 0), residual=(1 << 20) if res is not None else None)
        pl = _Cm.GemmPlan()
        hip.lib.e4t_gemm_plan(_ct.byref(d), _ct.byref(pl))
        y, yr = hip.gemm(at, bt, **args), emu.gemm(at, bt, **args)
        tol = TOLF * 50 if kw.get("f32") else TOL1
        r = pl.tail_rows
        out.append((f"gemm {Mt}x{Nt}x{Kt} tail{r} t{pl.tile} {'gelu ' if kw.get('gelu') else ''}{'f32' if kw.get('f32') else 'bf16'}", rel(y, yr), tol))
        if r > 0:      # (r == 0: the planner ran the shape without a tail stage — e.g. M = 2056, whose 2048 main rows want split-K)
            out.append((f"gemm {Mt}x{Nt}x{Kt} tail{r}: the tail rows alone", rel(y[Mt - r:], yr[Mt - r:]), tol))
            out.append((f"gemm {Mt}x{Nt}x{Kt} tail{r}: the last tile rows in front of the tail", rel(y[Mt - r - 64:Mt - r], yr[Mt - r - 64:Mt - r]), tol))
    # fp32 C + fp32 residual (the CLIP-ViT's fp32 residual stream): the line-wide direct-store epilogue, every kernel family
    gv = gen(33, dev)
    for (Mv, Nv, Kv, t) in CHECK_GEMM_F32RES:
        av, bw = rnd(gv, Mv, Kv, dev=dev), rnd(gv, Nv, Kv, scale=Kv ** -0.5, dev=dev)
        r32, bi = rnd(gv, Mv, Nv, dtype=f32, dev=dev), rnd(gv, Nv, dtype=f32, dev=dev)
        out.append((f"gemm {Mv}x{Nv}x{Kv} t{t} fp32 out + fp32 residual", rel(hip.gemm(av, bw, bias=bi, residual=r32, out_dtype=f32, tile=t),
                                                                            emu.gemm(av, bw, bias=bi, residual=r32, out_dtype=f32)), TOLF * 50))
    # the GENERAL (GELU / row-lookup) epilogue of the 256 x 320 ping-pong tile (GEMM only) and its row panels (e4t_gemm_desc.panel_*):
    # ragged M, several K depths, bf16 and fp32 output; panels leave the rows between them (the class-token rows) untouched
    gp = gen(34, dev)
    for (Mg, Ng, Kg) in CHECK_GEMM_PQ_GENERAL:
        ag, bg, big = rnd(gp, Mg, Kg, dev=dev), rnd(gp, Ng, Kg, scale=Kg ** -0.5, dev=dev), rnd(gp, Ng, dtype=f32, dev=dev)
        out.append((f"gemm {Mg}x{Ng}x{Kg} t2320 gelu", rel(hip.gemm(ag, bg, bias=big, gelu=True, tile=2320), emu.gemm(ag, bg, bias=big, gelu=True)), TOL1))
        Mr = (Mg // 97) * 97                      # rows_per_batch = 97 (not a multiple of 32): the per-row row-bias lookup of the GENERAL epilogue
        rbg = rnd(gp, Mr // 97, Ng, dtype=f32, dev=dev)
        out.append((f"gemm {Mr}x{Ng}x{Kg} t2320 row bias, rows_per_batch 97", rel(hip.gemm(ag[:Mr], bg, rowbias=rbg, rows_per_batch=97, tile=2320),
                                                                                 emu.gemm(ag[:Mr], bg, rowbias=rbg, rows_per_batch=97)), TOL1))
    for (Bp, Tp, Np, Kp, pr, dt) in CHECK_GEMM_PANELS:
        ap, bp, bip = rnd(gp, Bp * Tp, Kp, dev=dev), rnd(gp, Np, Kp, scale=Kp ** -0.5, dev=dev), rnd(gp, Np, dtype=f32, dev=dev)
        resid = rnd(gp, Bp * Tp, Np, dtype=dt, dev=dev) if dt == f32 else None
        yh = torch.full((Bp * Tp, Np), 7.0, dtype=dt, device=dev)
        ye = yh.clone()
        pan = (pr, Tp, Tp - pr, Bp)
        hip.gemm(ap, bp, bias=bip, gelu=(dt == bf16), residual=resid, out=yh, panels=pan)
        emu.gemm(ap, bp, bias=bip, gelu=(dt == bf16), residual=resid, out=ye, panels=pan)
        out.append((f"gemm row panels B{Bp} T{Tp} N{Np} K{Kp} ({pr} rows, offset {Tp - pr}) {'bf16 gelu' if dt == bf16 else 'fp32 out + residual'}", rel(yh, ye), TOL1 if dt == bf16 else TOLF * 50))
        skipped = torch.arange(Bp * Tp, device=dev).remainder(Tp) < Tp - pr
        out.append((f"gemm row panels B{Bp} T{Tp}: rows outside the panels untouched", float((yh[skipped] != 7.0).sum()), 0.0))
    rb = rnd(g, M // 96, N, dtype=f32, dev=dev)
    out.append(("gemm rowbias", rel(hip.gemm(a1, b[:, :K1].contiguous(), rowbias=rb, rows_per_batch=96),
                                    emu.gemm(a1, b[:, :K1].contiguous(), rowbias=rb, rows_per_batch=96)), TOL1))
    # strided views (column slices of a wider buffer)
    wide = rnd(g, M, 3 * K1, dev=dev)
    out.append(("gemm strided A view", rel(hip.gemm(wide[:, K1:2 * K1], b[:, :K1].contiguous()), emu.gemm(wide[:, K1:2 * K1], b[:, :K1].contiguous())), TOL1))
    # batched + reduce-batch (E4T head shape, small)
    nb, M, N, K = 9, 16, 128, 128
    A, Bw = rnd(g, nb, M, K, dev=dev), rnd(g, nb, N, K, scale=0.09, dev=dev)
    bias = rnd(g, nb, N, dtype=f32, dev=dev)
    out.append(("gemm batched", rel(hip.gemm(A, Bw, bias=bias), emu.gemm(A, Bw, bias=bias)), TOL1))
    out.append(("gemm batched reduce (mean over slots)", rel(hip.gemm(A, Bw, reduce_batch=True, alpha=1.0 / nb, out_dtype=f32),
                                                            emu.gemm(A, Bw, reduce_batch=True, alpha=1.0 / nb, out_dtype=f32)), TOLF * 50))
    Ab = A[0].unsqueeze(0).expand(nb, M, K)   # broadcast operand (stride 0)
    out.append(("gemm batched broadcast A", rel(hip.gemm(Ab, Bw), emu.gemm(Ab, Bw)), TOL1))
    # a batch entry other than 0 on the ping-pong kernels (the hints hold for N = 320: 256 x 256 and 256 x 320 tiles), ragged M
    A2, B2, bias2 = rnd(g, 2, 300, K, dev=dev), rnd(g, 2, 320, K, scale=0.09, dev=dev), rnd(g, 2, 320, dtype=f32, dev=dev)
    yr = emu.gemm(A2, B2, bias=bias2)
    for t in (512, 2320):
        d = _Cm.GemmDesc(M=300, N=320, K=K, K1=K, lda=K, ldb=K, ldc=320, batch=2, alpha=1.0, tile=t, strideA=300 * K, strideB=320 * K, strideC=300 * 320, strideBias=320)
        pl = _Cm.GemmPlan()
        hip.lib.e4t_gemm_plan(_ct.byref(d), _ct.byref(pl))
        out.append((f"gemm batched t{t}: the plan keeps the hint (got tile {pl.tile})", float(pl.tile != t), 0.0))
        y = hip.gemm(A2, B2, bias=bias2, tile=t)
        out.append((f"gemm batched t{t}", rel(y, yr), TOL1))
        out.append((f"gemm batched t{t}: batch entry 1", rel(y[1], yr[1]), TOL1))
    return out


# ------------------------------------------------------------------------------------------------ 3x3 conv
# Plain data, importable without a GPU: tests/test_gemm_dispatch.py pins the kernel symbol (and split-K) every case gets in every call form, and
# holds the symbols x conv modes the cases reach against everything e4t_conv3x3_kernel can return; tests/test_conv_slices_cpu.py holds a
# rounding-only model to half the tolerance on every row conv_slices() emits for them.
CONV_S2A = 5
# B, Hin, Win, Cin, Cout, mode, Hout, Wout, tile, splitk
CONV_CASES = [
    (2, 16, 16, 64, 64, CONV_S1, 16, 16, 0, 0), (2, 8, 8, 128, 192, CONV_S1, 8, 8, 64, 3),
    (3, 16, 16, 64, 128, CONV_S2, 8, 8, 0, 0), (2, 9, 9, 64, 64, CONV_S2, 5, 5, 0, 0),
    (2, 8, 8, 64, 64, CONV_UP2, 16, 16, 0, 0), (2, 8, 8, 128, 64, CONV_S2T, 16, 16, 0, 0),
    (2, 5, 5, 64, 64, CONV_S2T, 9, 9, 0, 0), (4, 32, 32, 320, 320, CONV_S1, 32, 32, 128, 1),
    (2, 16, 16, 64, 4, CONV_S1, 16, 16, 0, 0), (3, 24, 24, 64, 192, CONV_S1, 24, 24, 256, 1), (3, 24, 24, 64, 320, CONV_S1, 24, 24, 160, 1), (2, 16, 16, 128, 128, 5, 8, 8, 0, 0), (1, 64, 64, 128, 128, 5, 32, 32, 0, 0),
    (3, 24, 24, 64, 320, CONV_S1, 24, 24, 512, 1), (2, 32, 32, 128, 256, CONV_S1, 32, 32, 512, 1), (2, 16, 16, 256, 512, CONV_S1, 16, 16, 512, 2),
    (3, 16, 16, 64, 128, CONV_S2, 8, 8, 512, 1), (2, 8, 8, 64, 64, CONV_UP2, 16, 16, 512, 1), (2, 8, 8, 128, 64, CONV_S2T, 16, 16, 512, 1),
    (1, 64, 64, 128, 128, 5, 32, 32, 512, 1),
    (2, 48, 40, 64, 320, CONV_S1, 48, 40, 5256, 1),
    (2, 20, 12, 192, 128, CONV_S1, 20, 12, 5256, 1),   # channel-chunk-major K order with 32-wide chunks
    (4, 32, 32, 320, 320, CONV_S1, 32, 32, 2320, 1), (2, 16, 16, 256, 640, CONV_S1, 16, 16, 2320, 2), (2, 8, 8, 128, 320, CONV_S2T, 16, 16, 2320, 1),
    (3, 16, 16, 64, 320, CONV_S2, 8, 8, 2320, 1), (2, 8, 8, 64, 320, CONV_UP2, 16, 16, 2320, 1),
    (16, 64, 64, 64, 320, CONV_S1, 64, 64, 2320, 1),
    # round 6: conv_strip_kernel (stride 1, W % 256 == 0, the 256 x 128 x 32 tile): image borders in both directions, several 256-pixel
    # segments per row, one-row images, Cout beyond one column tile, batch crossing
    (2, 6, 256, 64, 128, CONV_S1, 6, 256, 5256, 1), (1, 3, 768, 192, 256, CONV_S1, 3, 768, 5256, 1), (3, 1, 256, 64, 128, CONV_S1, 1, 256, 5256, 1),
    (2, 5, 512, 128, 128, CONV_S1, 5, 512, 0, 0),
    # ... and gemm_pps_kernel (the ping-pong kernel on half-strips): whole-row tiles W = 16 / 64, row segments W = 256 / 512, split-K on kernel-row boundaries
    (2, 64, 64, 64, 256, CONV_S1, 64, 64, 512, 1), (1, 4, 256, 128, 320, CONV_S1, 4, 256, 512, 1), (1, 2, 512, 64, 256, CONV_S1, 2, 512, 512, 1),
    (2, 16, 16, 192, 256, CONV_S1, 16, 16, 512, 3), (3, 128, 128, 64, 128, CONV_S1, 128, 128, 512, 1),
]


def _reach_geometry(mode):
    """input 9 x 9 where the mode allows odd sizes (5 x 5 for S2T, whose output is then 9 x 9): Hout * Wout % 32 != 0 in every mode, so that the
    row bias of the full form takes the GENERAL epilogue where the tile has one; S2A drops the last input row and column"""
    return {CONV_S1: (9, 9, 9, 9), CONV_S2: (9, 9, 5, 5), CONV_UP2: (9, 9, 18, 18), CONV_S2T: (5, 5, 9, 9), CONV_S2A: (9, 9, 4, 4)}[mode]


# every tile code x conv mode (the mode is a run-time branch of the gather): B = 2, Cin = 64, Cout = the tile width + 8 where the tile takes a ragged N
CONV_REACH_TILES = [(64, 72), (3064, 72), (4064, 72), (128, 136), (3128, 136), (4128, 136), (160, 168), (3160, 168), (4160, 168), (5256, 136), (512, 264), (2320, 320)]
CONV_REACH_CASES = [(2, g[0], g[1], 64, cout, mode, g[2], g[3], tile, 1)
                    for tile, cout in CONV_REACH_TILES for mode in (CONV_S1, CONV_S2, CONV_UP2, CONV_S2T, CONV_S2A) for g in [_reach_geometry(mode)]]
# one-pixel-wide and one-pixel images (every pixel is several borders at once), odd sizes for S2A; B = 3: image boundaries in M sit inside a tile
CONV_DEGENERATE_CASES = [
    (3, 1, 1, 64, 64, CONV_S1, 1, 1, 0, 0), (3, 1, 7, 64, 64, CONV_S1, 1, 7, 0, 0), (3, 7, 1, 64, 64, CONV_S1, 7, 1, 0, 0), (3, 2, 2, 64, 64, CONV_S1, 2, 2, 0, 0),
    (3, 1, 1, 64, 64, CONV_S2, 1, 1, 0, 0), (3, 2, 3, 64, 64, CONV_S2, 1, 2, 0, 0),
    (3, 1, 1, 64, 64, CONV_UP2, 2, 2, 0, 0),
    (3, 1, 1, 64, 64, CONV_S2T, 1, 1, 0, 0), (3, 2, 2, 64, 64, CONV_S2T, 3, 3, 0, 0),
    (3, 9, 7, 64, 64, CONV_S2A, 4, 3, 0, 0), (3, 2, 2, 64, 64, CONV_S2A, 1, 1, 0, 0),
]
CONV_ALL_CASES = CONV_CASES + CONV_REACH_CASES + CONV_DEGENERATE_CASES      # check_conv runs these, each in the full and the bare form
# The call forms: which optional operands are given (NULL or not is part of the plan) and the flags
CONV_FORMS = {
    "full": dict(bias=True, rowbias=True, residual=True),      # the ResBlock's first conv
    "bare": dict(),                                            # the data-gradient convs: nothing in the epilogue
    "colstats": dict(bias=True, colstats=True), "colstats+res": dict(bias=True, residual=True, colstats=True),
    "f32 bias": dict(bias=True, f32=True), "f32 res32": dict(bias=True, residual=True, f32=True, res32=True), "f32 res16": dict(bias=True, residual=True, f32=True),
    "accum16": dict(accum=True), "accum32": dict(accum=True, f32=True),
    "rowbias slice": dict(rowbias=True),
    "gelu": dict(bias=True, gelu=True),      # E4T_ACT_GELU: no conv of the model sets it, the ABI takes it (raw descriptor; the GENERAL epilogue)
}
# check_conv_forms: the smallest shape of every conv kernel family (M % 32 == 0 for the column statistics; 8 x 8 is no strip geometry, 16 x 16 is)
CONV_FORM_CASES = {
    "64": (2, 8, 8, 64, 64, CONV_S1, 8, 8, 64, 1), "128": (2, 8, 8, 64, 128, CONV_S1, 8, 8, 128, 1), "160": (2, 8, 8, 64, 160, CONV_S1, 8, 8, 160, 1),
    "5256": (2, 8, 8, 64, 128, CONV_S1, 8, 8, 5256, 1), "5256 strip": (2, 16, 16, 64, 128, CONV_S1, 16, 16, 5256, 1),
    "512": (2, 8, 8, 64, 256, CONV_S1, 8, 8, 512, 1), "512 pps": (2, 16, 16, 64, 256, CONV_S1, 16, 16, 512, 1),
    "2320": (2, 8, 8, 64, 320, CONV_S1, 8, 8, 2320, 1),
}
CONV_GELU_FAMILIES = ("512", "512 pps")                                   # the GENERAL instantiations of the ping-pong kernels; nothing else reaches gemm_pps_kernel<true>
CONV_FORM_SPLITK = 3                                                      # explicit split-K: the call reports the statistics NOT written
CONV_OUT_CASES = [(2, 16, 16, 64, 4, CONV_S1, 16, 16, t, 0) for t in (0, 64, 128)]      # conv_out: bias only, fp32 output, Cout = 4
# check_conv_guards: every conv kernel symbol, ragged M and (where the tile takes it) ragged Cout: the stride-1 cases (the channel-major gather, whose
# buffer window starts in front of X) and the S2A ones (the kernels' other K order; the last input row and column are never read) of the reach list
CONV_GUARD_CASES = [c for c in CONV_REACH_CASES if c[5] in (CONV_S1, CONV_S2A)] + [
    (3, 16, 16, 64, 136, CONV_S1, 16, 16, 5256, 1),      # conv_strip_kernel (its geometries make M a multiple of 256): a ragged column tile
    (2, 16, 16, 64, 264, CONV_S1, 16, 16, 512, 1),       # gemm_pps_kernel (wants M % 256 == 0): ragged Cout
]


def conv_tag(case):
    B, Hin, Win, Cin, Cout, mode, Hout, Wout, tile, sk = case
    return f"conv mode{mode} B{B} {Hin}x{Win} {Cin}->{Cout} t{tile} s{sk}"


def conv_desc(case, form, splitk=None):
    """the descriptor hip.conv3x3 hands the library for a case in a call form, with a pointer that is never dereferenced wherever one is given and
    the workspace the plan asks for: for e4t_conv3x3_plan / e4t_conv3x3_kernel (pure host code)"""
    from e4t import _C
    B, Hin, Win, Cin, Cout, mode, Hout, Wout, tile, sk = case
    f, fake = CONV_FORMS[form], 1 << 24
    M = B * Hout * Wout
    flags = (_C.OUT_F32 if f.get("f32") else 0) | (_C.RES_F32 if f.get("res32") else 0) | (_C.ACCUM if f.get("accum") else 0) | (_C.ACT_GELU if f.get("gelu") else 0)
    ptr = lambda k: fake if f.get(k) else None
    return _C.ConvDesc(X=fake, W=fake, Y=fake, bias=ptr("bias"), residual=ptr("residual"), rowbias=ptr("rowbias"), workspace=fake, workspace_bytes=1 << 40,
                       B=B, Hin=Hin, Win=Win, Cin=Cin, Hout=Hout, Wout=Wout, Cout=Cout, mode=mode, flags=flags, tile=tile, splitk=sk if splitk is None else splitk,
                       ldrb=1280 if form == "rowbias slice" else Cout if f.get("rowbias") else 0,
                       colstats=fake if f.get("colstats") and not f.get("f32") and M % 32 == 0 else None)


def conv_plan(case, form, splitk=None):
    import ctypes
    from e4t import _C
    pl = _C.GemmPlan()
    _C.check(_C.load().e4t_conv3x3_plan(ctypes.byref(conv_desc(case, form, splitk)), ctypes.byref(pl)), "e4t_conv3x3_plan")
    return pl


def conv_kernel(case, form, splitk=None):
    """'<kernel symbol> splitk<n>' of the launch, from the library's own decision (e4t_conv3x3_kernel)"""
    import ctypes
    from e4t import _C
    sym, sk = ctypes.c_char_p(), ctypes.c_int(0)
    _C.check(_C.load().e4t_conv3x3_kernel(ctypes.byref(conv_desc(case, form, splitk)), ctypes.byref(sym), ctypes.byref(sk)), "e4t_conv3x3_kernel")
    return "%s splitk%d" % (sym.value.decode(), sk.value)


def conv_inputs(case, seed, dev):
    """x, w, bias, row bias, residual of a case: unit-variance conv product, bias, row bias and residual"""
    B, Hin, Win, Cin, Cout, mode, Hout, Wout, tile, sk = case
    g = gen(seed, dev)
    x = rnd(g, B * Hin * Win, Cin, dev=dev)
    w = rnd(g, Cout, 9 * Cin, scale=(9 * Cin) ** -0.5, dev=dev)
    bias = rnd(g, Cout, dtype=f32, dev=dev)
    rb = rnd(g, B, Cout, dtype=f32, dev=dev)
    res = rnd(g, B * Hout * Wout, Cout, dev=dev)
    return x, w, bias, rb, res


def conv_slices(tag, got, ref, B, Hout, Wout, plan, tol=TOL1):
    """Result rows that a whole-tensor relative L2 dilutes: got, ref = [B * Hout * Wout, Cout].  The relative L2 of the top / bottom row, the left /
    right column, the four corners together, the interior, the first / last image, the rows of the last, partial M-tile (M % plan.tile_m) and the
    columns of the last, partial N-tile (Cout % plan.tile_n).  Empty regions, and a bottom row / right column / last image that is the top row / left
    column / first image, are skipped.  The tolerance is the whole tensor's: the stated bound is per element, so it holds for any region
    (tests/test_conv_slices_cpu.py holds a rounding-only model to half of it on every row emitted here, down to 32 values)."""
    Cout = ref.shape[-1]
    M = B * Hout * Wout
    g, r = got.float().reshape(B, Hout, Wout, Cout), ref.float().reshape(B, Hout, Wout, Cout)
    d2, r2 = (g - r) ** 2, r * r
    out = []

    def row(label, sel):
        d, n = d2[sel], r2[sel]
        if d.numel():
            e = (d.sum() / (n.sum() + 1e-38)).sqrt()
            out.append((f"{tag}: {label}", float(torch.nan_to_num(e, nan=float("inf"))), tol))
    A = slice(None)
    row("top row", (A, 0))
    if Hout > 1:
        row("bottom row", (A, Hout - 1))
    row("left column", (A, A, 0))
    if Wout > 1:
        row("right column", (A, A, Wout - 1))
    ys, xs = sorted({0, Hout - 1}), sorted({0, Wout - 1})
    row("corners", (A, torch.tensor(ys)[:, None], torch.tensor(xs)[None, :]))
    row("interior", (A, slice(1, Hout - 1), slice(1, Wout - 1)))
    row("first image", (0,))
    if B > 1:
        row("last image", (B - 1,))
    d2, r2 = d2.reshape(M, Cout), r2.reshape(M, Cout)
    if M % plan.tile_m:
        row(f"rows {M - M % plan.tile_m}-{M - 1} (the partial {plan.tile_m}-row tile)", (slice(M - M % plan.tile_m, M),))
    if Cout % plan.tile_n:
        row(f"columns {Cout - Cout % plan.tile_n}-{Cout - 1} (the partial {plan.tile_n}-column tile)", (A, slice(Cout - Cout % plan.tile_n, Cout)))
    return out


def check_conv(hip, emu, dev):
    out = []
    for i, case in enumerate(CONV_ALL_CASES):
        B, Hin, Win, Cin, Cout, mode, Hout, Wout, tile, sk = case
        x, w, bias, rb, res = conv_inputs(case, 50 + i, dev)
        tag = conv_tag(case)
        y = hip.conv3x3(x, w, B, Hin, Win, Hout, Wout, mode, bias=bias, rowbias=rb, residual=res, tile=tile, splitk=sk)
        yr = emu.conv3x3(x, w, B, Hin, Win, Hout, Wout, mode, bias=bias, rowbias=rb, residual=res)
        out.append((tag, rel(y, yr), TOL1))
        out += conv_slices(tag, y, yr, B, Hout, Wout, conv_plan(case, "full"))
        # bare: no bias, no row bias, no residual — the call form of the data-gradient convs, and the one in which nothing dilutes the conv product
        y = hip.conv3x3(x, w, B, Hin, Win, Hout, Wout, mode, tile=tile, splitk=sk)
        yr = emu.conv3x3(x, w, B, Hin, Win, Hout, Wout, mode)
        out.append((tag + " bare", rel(y, yr), TOL1))
        out += conv_slices(tag + " bare", y, yr, B, Hout, Wout, conv_plan(case, "bare"))
    # weight relayout + dgrad identity: conv dgrad == autograd of conv
    g = gen(70, dev)
    O, I = 96, 64
    w4 = rnd(g, O, I, 3, 3, scale=0.05, dtype=f32, dev=dev)
    wf, wd = hip.conv_weight_prepare(w4)
    wf2, wd2 = emu.conv_weight_prepare(w4)
    out.append(("conv_weight_prepare fwd layout", rel(wf, wf2), 0.0))
    out.append(("conv_weight_prepare dgrad layout", rel(wd, wd2), 0.0))
    return out


def check_conv_forms(hip, emu, dev):
    """the call forms the model uses and check_conv does not: column statistics out of a conv (into the consuming GroupNorm), fp32 output, accumulate,
    a row bias that is a column slice of a wider matrix — each on every conv kernel family (CONV_FORM_CASES)"""
    import torch.nn.functional as F
    out = []
    for i, (fam, case) in enumerate(CONV_FORM_CASES.items()):
        B, Hin, Win, Cin, Cout, mode, Hout, Wout, tile, sk = case
        M, HW = B * Hout * Wout, Hout * Wout
        x, w, bias, rb, res = conv_inputs(case, 300 + i, dev)
        g = gen(320 + i, dev)
        geo, kw = (x, w, B, Hin, Win, Hout, Wout, mode), dict(tile=tile, splitk=sk)
        tag = f"conv family {fam} ({Hin}x{Win} {Cin}->{Cout})"
        for form, r in (("colstats", None), ("colstats+res", res)):
            y = hip.conv3x3(*geo, bias=bias, residual=r, colstats=True, **kw)
            cs = getattr(y, "_e4t_colstats", None)
            blk = y.float().reshape(M // 32, 32, Cout)
            ref = torch.stack([blk.sum(1), (blk * blk).sum(1)], dim=-1)
            out.append((f"{tag} {form}: reported written (1 = not)", float(cs is None), 0.0))
            out.append((f"{tag} {form}: == the statistics of the kernel's own output", rel(cs, ref) if cs is not None else 1.0, 1e-5))
            out.append((f"{tag} {form}: y", rel(y, emu.conv3x3(*geo, bias=bias, residual=r)), TOL1))
        if cs is not None:      # the conv's statistics through the consuming GroupNorm == the same GroupNorm with its own statistics pass
            gamma, beta = rnd(g, Cout, dtype=f32, dev=dev) * 0.3 + 1.0, rnd(g, Cout, dtype=f32, dev=dev) * 0.2
            n1, st1 = hip.groupnorm_fwd(y, None, gamma, beta, B, HW, 32, 1e-5, True)
            n2, st2 = hip.groupnorm_fwd(y.clone(), None, gamma, beta, B, HW, 32, 1e-5, True)      # (a clone carries no statistics)
            out.append((f"{tag} colstats+res -> GroupNorm: y", rel(n1, n2), 2e-3))
            out.append((f"{tag} colstats+res -> GroupNorm: stats", rel(st1, st2), 1e-4))
        y = hip.conv3x3(*geo, bias=bias, colstats=True, tile=tile, splitk=CONV_FORM_SPLITK)
        out.append((f"{tag} colstats, split-K {CONV_FORM_SPLITK}: reported written (0 = not)", float(hasattr(y, "_e4t_colstats")), 0.0))
        out.append((f"{tag} colstats, split-K {CONV_FORM_SPLITK}: y", rel(y, emu.conv3x3(*geo, bias=bias)), TOL1))
        res32 = rnd(g, M, Cout, dtype=f32, dev=dev)
        for form, r in (("f32 bias", None), ("f32 res32", res32), ("f32 res16", res)):
            y, yr = hip.conv3x3(*geo, bias=bias, residual=r, out_dtype=f32, **kw), emu.conv3x3(*geo, bias=bias, residual=r, out_dtype=f32)
            out.append((f"{tag} {form}", rel(y, yr), TOLF * 50))
            out += conv_slices(f"{tag} {form}", y, yr, B, Hout, Wout, conv_plan(case, form), tol=TOLF * 50)
        for form, dt, tol in (("accum16", bf16, TOL1), ("accum32", f32, TOLF * 50)):
            o1 = rnd(g, M, Cout, dtype=dt, dev=dev)
            o2 = o1.clone()
            hip.conv3x3(*geo, out=o1, accum=True, **kw); emu.conv3x3(*geo, out=o2, accum=True)
            out.append((f"{tag} {form}", rel(o1, o2), tol))
            out += conv_slices(f"{tag} {form}", o1, o2, B, Hout, Wout, conv_plan(case, form), tol=tol)
        wide = rnd(g, B, 1280, dtype=f32, dev=dev)      # all ResBlocks' time-embedding projections in one matrix: this conv's is a column slice of it
        rbs = wide[:, 320:320 + Cout]
        y, yr = hip.conv3x3(*geo, rowbias=rbs, **kw), emu.conv3x3(*geo, rowbias=rbs)
        out.append((f"{tag} row bias = columns 320-{320 + Cout - 1} of a [B][1280] matrix", rel(y, yr), TOL1))
        out += conv_slices(f"{tag} row bias slice", y, yr, B, Hout, Wout, conv_plan(case, "rowbias slice"))
    for i, fam in enumerate(CONV_GELU_FAMILIES):      # through the raw ABI: the descriptor of conv_desc() with the operands' addresses
        import ctypes
        from e4t import _C, ops
        case = CONV_FORM_CASES[fam]
        B, Hin, Win, Cin, Cout, mode, Hout, Wout, tile, sk = case
        x, w, bias, _, _ = conv_inputs(case, 330 + i, dev)
        y = torch.empty(B * Hout * Wout, Cout, dtype=bf16, device=dev)
        d = conv_desc(case, "gelu")
        d.X, d.W, d.Y, d.bias, d.workspace, d.workspace_bytes = x.data_ptr(), w.data_ptr(), y.data_ptr(), bias.data_ptr(), None, 0      # (one pass: sk = 1)
        _C.check(hip.lib.e4t_conv3x3(ctypes.byref(d), ops._stream()), "e4t_conv3x3")
        yr = emu._act(F.gelu(emu.conv3x3(x, w, B, Hin, Win, Hout, Wout, mode, bias=bias, out_dtype=f32)))
        out.append((f"conv family {fam} ({Hin}x{Win} {Cin}->{Cout}) gelu (raw ABI)", rel(y, yr), TOL1))
        out += conv_slices(f"conv family {fam} gelu", y, yr, B, Hout, Wout, conv_plan(case, "gelu"))
    for i, case in enumerate(CONV_OUT_CASES):      # conv_out: 4 output channels, bias only, fp32
        B, Hin, Win, Cin, Cout, mode, Hout, Wout, tile, sk = case
        x, w, bias, _, _ = conv_inputs(case, 340 + i, dev)
        geo = (x, w, B, Hin, Win, Hout, Wout, mode)
        y, yr = hip.conv3x3(*geo, bias=bias, out_dtype=f32, tile=tile, splitk=sk), emu.conv3x3(*geo, bias=bias, out_dtype=f32)
        out.append((conv_tag(case) + " f32 bias (conv_out)", rel(y, yr), TOLF * 50))
        out += conv_slices(conv_tag(case) + " f32 bias (conv_out)", y, yr, B, Hout, Wout, conv_plan(case, "f32 bias"), tol=TOLF * 50)
    return out


GUARD_ROWS_W, GUARD_ROWS_Y = 320, 256      # the widest column tile of weight rows behind Cout; the tallest row tile of sentinel rows around Y


def guarded_conv_operands(x, w, M, Win):
    """x, w and a bf16 y [M][Cout], each a view into ONE larger allocation, so that an out-of-range access of a wrong kernel lands in memory the test
    owns: NaN for 2 * (Win + 1) * Cin elements in front of and behind x (the channel-major gather's buffer window starts (Win + 1) * Cin elements in
    front of x: what lies there is read and must be masked), NaN weight rows behind Cout (a ragged column tile reads them), sentinel rows around y,
    and y itself filled with the sentinel.  -> xg, wg, yg, the two y guards as int16 views"""
    Cin, Cout = x.shape[-1], w.shape[0]
    gx = 2 * (Win + 1) * Cin
    xb = torch.full((gx + x.numel() + gx,), float("nan"), dtype=bf16, device=x.device)
    xg = xb[gx:gx + x.numel()].view(x.shape)
    xg.copy_(x)
    wb = torch.full((Cout + GUARD_ROWS_W, w.shape[1]), float("nan"), dtype=bf16, device=x.device)
    wb[:Cout].copy_(w)
    yb = torch.full((GUARD_ROWS_Y + M + GUARD_ROWS_Y, Cout), SENT16, dtype=torch.int16, device=x.device)
    return xg, wb[:Cout], yb[GUARD_ROWS_Y:GUARD_ROWS_Y + M].view(bf16), (yb[:GUARD_ROWS_Y], yb[GUARD_ROWS_Y + M:])


def check_conv_guards(hip, emu, dev):
    """every conv kernel symbol on operands with poison around them (CONV_GUARD_CASES: ragged M, ragged Cout where the tile takes it), bare and with
    the full epilogue: bitwise the unguarded run, finite, no sentinel touched"""
    out = []
    for i, case in enumerate(CONV_GUARD_CASES):
        B, Hin, Win, Cin, Cout, mode, Hout, Wout, tile, sk = case
        x, w, bias, rb, res = conv_inputs(case, 400 + i, dev)
        for form, epi in (("full", dict(bias=bias, rowbias=rb, residual=res)), ("bare", {})):
            tag = f"{conv_tag(case)} {form}, guarded"
            y0 = hip.conv3x3(x, w, B, Hin, Win, Hout, Wout, mode, tile=tile, splitk=sk, **epi)
            xg, wg, yg, guards = guarded_conv_operands(x, w, B * Hout * Wout, Win)
            hip.conv3x3(xg, wg, B, Hin, Win, Hout, Wout, mode, out=yg, tile=tile, splitk=sk, **epi)
            out.append((f"{tag}: elements differing from the unguarded run", float((yg.view(torch.int16) != y0.view(torch.int16)).sum()), 0.0))
            out.append((f"{tag}: non-finite elements", float((~torch.isfinite(yg.float())).sum()), 0.0))
            out.append((f"{tag}: sentinel elements changed", float(sum((gd != SENT16).sum() for gd in guards)), 0.0))
    return out


# ------------------------------------------------------------------------------------------------ attention
# (B, H, T, S, DH[, causal]) of check_attention.  tests/test_gemm_dispatch.py pins which kernels every one of them gets (and holds the set
# of kernel symbols they reach against everything e4t_attention_plan can return), so this list is plain data: importable without a GPU.
ATTENTION_CASES = [
    (2, 2, 64, 64, 32), (2, 3, 200, 200, 40), (1, 2, 128, 77, 40), (2, 2, 96, 77, 80), (1, 2, 64, 64, 160),
    (1, 2, 257, 257, 80), (2, 2, 130, 33, 64), (1, 8, 1024, 1024, 40),
    (3, 5, 300, 300, 40), (2, 8, 4096, 4096, 40),        # 45 workgroups (XCD re-deal with a remainder); the step's own 64 x 64 self-attention
    # S >= 2048, ragged tiles: dh 40 on the LDS-DMA kernels, dh 64 on attn_bwd_dkv_kernel<64, 2> with the query range cut in 7
    (1, 2, 300, 2100, 40), (1, 1, 2050, 2050, 64),
    (3, 12, 77, 77, 64, True), (2, 3, 200, 200, 40, True), (1, 2, 128, 128, 80, True),      # causal: CLIP text encoder
    # few key blocks, long query range: the dK/dV kernel cuts T into chunks + fp32 partial reduce (round 4) — the step's own
    # cross-attention shape at a smaller batch, a ragged T (3 chunks of 384 / 384 / 232), dh 80 / 64, a short self-attention
    (2, 8, 4096, 77, 40), (1, 2, 1000, 77, 40), (2, 2, 1024, 77, 80), (1, 2, 600, 33, 64), (1, 4, 1024, 1024, 40),
    # round 6: the 64-queries-per-wave forward (dh 40, S >= 512): last tile of 8 keys (its second sub-tile fully masked), of 33
    # keys, ragged T inside a 256-query block, exactly one tile pair
    (1, 2, 520, 520, 40), (2, 3, 700, 545, 40), (1, 1, 40, 512, 40), (2, 2, 256, 640, 40),
    # ... and the 64-keys-per-wave dK/dV kernel + 64-queries-per-wave dQ kernel (dh 40, enough key blocks that the query range is
    # not split): ragged T (last tile of 24 / 12 queries) and ragged S (last workgroup with 208 / 42 keys)
    (4, 8, 600, 2000, 40), (2, 16, 1100, 2090, 40),
]
# The three-workgroups-per-CU instantiations attn_bwd_dkv_kernel<32 | 40, 3> (no register prefetch: another order of loads, barriers and
# stores in the query loop), attn_bwd_dq_dma_kernel<32>, and the same no-prefetch loop at dh 160 over more than one query tile:
ATTENTION_NEW_CASES = [
    (1, 2, 130, 2100, 40),             # dkv<40, 3> (T < 192): query tiles of 64 / 64 / 2, last key block of 52
    (1, 1, 2080, 2080, 40, True),      # dkv<40, 3> causal, query range cut in 7 chunks of 320 (the last: 160) + reduce
    (1, 2, 200, 2100, 32),             # dq_dma<32> / dkv<32, 3>: last query tile of 8
    (2, 2, 256, 256, 32),              # dq_dma<32> / dkv<32, 2>: the tiny-test UNet's own self-attention, fused qkv
    (2, 2, 256, 256, 160),             # SD-1.x 16 x 16 level: 4 query tiles in the no-prefetch loop, 2 workgroups per head
    (1, 2, 200, 77, 160),              # ... its cross-attention: ragged T and S
    (1, 1, 300, 130, 160),             # last query tile of 44, last key block of 2
    (1, 2, 600, 77, 160),              # query range cut in 2: fp32 partial store + attn_dkv_reduce_kernel<160>
    (2, 2, 200, 233, 64),              # dq_dma<64> with a ragged last key tile and B, H > 1
]
ATTENTION_CASES += ATTENTION_NEW_CASES
ATTENTION_DETERMINISM_CASES = [(16, 8, 4096, 4096, 40), (4, 8, 4096, 4096, 40)]      # the bitwise run-to-run check and its four batch chunks
# The backward through the raw ABI with less workspace than the library asks for: (case, labels, entry point).  Labels as in
# tools/gemm_dispatch_dump.py: delta = B * H * T floats, short = the stated size minus 1; "plain" = e4t_attention_bwd, which takes no size.
ATTENTION_WS_CASES = [
    ((1, 2, 300, 2100, 40), ("delta",), "ws"),            # no {L, Delta} pairs: dq_dma<40> with LD == nullptr in front of dkv<40, 3> (full: dkv_dma)
    ((2, 3, 200, 200, 40), ("delta", "short"), "ws"),     # dkv<40, 2> instead of dkv_dma
    ((2, 8, 1024, 77, 40), ("delta",), "plain"),          # one query chunk instead of four
    ((1, 1, 2080, 2080, 40, True), ("delta",), "ws"),     # un-split causal dkv<40, 3>
    ((1, 2, 600, 77, 160), ("delta",), "ws"),             # one query chunk instead of two
]
# cases that run once more with batch strides beyond dense, NaN in the input gaps and sentinels around every output (besides every new one)
ATTENTION_GAP_CASES = [(3, 5, 300, 300, 40), (2, 2, 96, 77, 80), (2, 16, 1100, 2090, 40)]
ATTENTION_NULL_LSE_CASES = [(2, 3, 200, 200, 40), (1, 2, 520, 520, 40)]
# Peaked scores at scale 1.0: name -> (seed, (B, H, T, S, DH), ((key, query row, factor), ...)): k[key] = factor * q[row], i.e. a score of
# factor * |q[row]|^2 ~ factor * DH for that pair — |LSE| up to ~1050 natural-log units.  The forward's online softmax sees large jumps of
# the running max (first / middle / last tile, a best key that comes first, a huge negative score); the backward recomputes P from the
# stored LSE, which the dh-40 dK/dV kernels fold into three bf16 pieces of the Q image.
_FIVE = lambda last, mid, neg: ((3, 7, 8.0), (mid, 40, 12.0), (last, 5, 20.0), (0, 70, 30.0), (neg, 9, -30.0))
ATTENTION_PEAKED = {
    "dh64": (120, (1, 1, 64, 160, 64), ((130, 5, 6.0),)),
    "dh40 long-key": (121, (1, 1, 96, 840, 40), _FIVE(834, 333, 500)),
    "dh40 long-key T256": (122, (1, 1, 256, 840, 40), _FIVE(834, 333, 500)),      # dq_dma<40> / dkv_dma<40>; dkv<40, 2> with a Delta-only workspace
    "dh80": (123, (1, 2, 96, 77, 80), ((70, 5, 4.0), (0, 50, 10.0))),            # attn_fwd_kernel<80>: row sum in the MFMA's spare row, lazy rescale
    "dh40 short-key": (124, (1, 1, 96, 200, 40), _FIVE(197, 100, 150)),           # attn_fwd_kernel<40> (S < 512)
}
BLOCK_Q, BLOCK_K = 64, 128      # rows per query tile (O, dQ, LSE) and per dK/dV workgroup


def peaked_attention_inputs(name, dev):
    """(q, k, v, dO) of ATTENTION_PEAKED[name]: [T | S, H * DH] bf16, the spiked key rows set across all heads"""
    seed, (B, H, T, S, DH), spikes = ATTENTION_PEAKED[name]
    g = gen(seed, dev)
    q, k, v = rnd(g, T, H * DH, dev=dev), rnd(g, S, H * DH, dev=dev), rnd(g, S, H * DH, dev=dev)
    for key, row, mul in spikes:
        k[key] = (q[row].float() * mul).to(bf16)
    return q, k, v, rnd(g, T, H * DH, dev=dev)


def lse_rows(lse):
    """fp32 [B][H][T] -> [B * T, H]: the row layout slices() takes (one column per head)"""
    B, H, T = lse.shape
    return lse.permute(0, 2, 1).reshape(B * T, H)


def slices(tag, got, ref, B, L, H, DH, block, tol=TOL2, blocks=True, every_block=False):
    """Result rows that a whole-tensor relative L2 cannot give: got, ref = [B * L, >= H * DH] row-major, head h in columns [h * DH, (h + 1) * DH).
      - the worst relative L2 of one (batch, head);
      - the worst (batch, head) of the last `block`-row block alone, ragged or not, and of the block in front of it (blocks=True, L > block);
      - the worst (batch, head, block) of all (every_block=True).
    Never finer than a row block: a single row whose softmax is saturated has dS = 0 exactly, and its relative error means nothing.
    The tolerance is the whole tensor's: the stated bound is per element, so it holds for any slice (tests/test_attention_slices_cpu.py
    holds a rounding-only model of the kernels to half of it on every slice emitted here)."""
    g = got[:, : H * DH].float().reshape(B, L, H, DH)
    r = ref[:, : H * DH].float().reshape(B, L, H, DH)
    d2, r2 = ((g - r) ** 2).sum(-1), (r * r).sum(-1)      # [B, L, H]

    def worst(lo, hi):
        e = (d2[:, lo:hi].sum(1) / (r2[:, lo:hi].sum(1) + 1e-38)).sqrt()
        return float(torch.nan_to_num(e, nan=float("inf")).max())
    out = [(f"{tag}: worst (batch, head)", worst(0, L), tol)]
    last = (L - 1) // block * block
    if blocks and last > 0:
        out.append((f"{tag}: rows {last}-{L - 1} (last {block}-row block), worst (batch, head)", worst(last, L), tol))
        out.append((f"{tag}: rows {last - block}-{last - 1} (the block in front), worst (batch, head)", worst(last - block, last), tol))
    if every_block:
        out.append((f"{tag}: worst {block}-row block of any (batch, head)", max(worst(lo, min(lo + block, L)) for lo in range(0, L, block)), tol))
    return out


def attention_slices(tag, B, H, T, S, DH, o, o_r, lse, lse_r, grads, grads_r, blocks=True, every_block=False):
    """slices() of everything one attention case produces; o / lse may be None (backward-only comparisons)"""
    out, kw = [], dict(blocks=blocks, every_block=every_block)
    if o is not None:
        out += slices(tag + " fwd O", o, o_r, B, T, H, DH, BLOCK_Q, **kw)
        out += slices(tag + " fwd LSE", lse_rows(lse), lse_rows(lse_r), B, T, H, 1, BLOCK_Q, tol=1e-3, **kw)
    for nm, a, b_, L, blk in zip(("dQ", "dK", "dV"), grads, grads_r, (T, S, S), (BLOCK_Q, BLOCK_K, BLOCK_K)):
        out += slices(f"{tag} bwd {nm}", a, b_, B, L, H, DH, blk, **kw)
    return out


# ---- the raw ABI: explicit batch strides, a workspace of the caller's size, poison around everything -------------------------------
SENT16, SENT32 = 0x5A5B, 0x5A5B5C5D      # what outputs, gaps and guards hold before a call: finite as bf16 and as fp32 (~1.5e16)
GAP_Q, GAP_K, GUARD_ROWS, GUARD_LSE, PAD_COLS, WS_EXCESS = 3, 5, 128, 64, 8, 1024


class _Operand:
    """B batches of L rows x d columns at column c0 of a row-major bf16 buffer [rows][width], batch b starting at row b * (L + gap)"""

    def __init__(self, buf, B, L, gap, c0, d):
        self.buf, self.c0, self.d, self.ld, self.bstride = buf, c0, d, buf.stride(0), (L + gap) * buf.stride(0)
        ar = lambda n: torch.arange(n, device=buf.device)
        self.idx = (ar(B)[:, None] * (L + gap) + ar(L)[None, :]).reshape(-1)
        self.ptr = buf.data_ptr() + 2 * c0

    def put(self, t):
        self.buf[self.idx, self.c0:self.c0 + self.d] = t[:, : self.d]
        return self

    def get(self):
        return self.buf[self.idx, self.c0:self.c0 + self.d]


def _sentinel_buf(rows, width, dev):
    return torch.full((rows, width), SENT16, dtype=torch.int16, device=dev).view(bf16)


def _changed_outside(buf, operands):
    """elements of an output buffer outside its operands' valid rows x columns that no longer hold the sentinel"""
    chk = buf.view(torch.int16).clone()
    for op in operands:
        chk[op.idx, op.c0:op.c0 + op.d] = SENT16
    return int((chk != SENT16).sum())


class RawAttention:
    """e4t_attention_fwd / e4t_attention_bwd / e4t_attention_bwd_ws through ctypes, on buffers laid out here.  gaps=False: dense batch strides
    (T * ld, S * ld), as e4t.ops passes them.  gaps=True: Q / O / dO / dQ have GAP_Q rows between batches and K / V / dK / dV GAP_K, GUARD_ROWS
    rows follow the last batch, PAD_COLS columns lie beside the operands' own, GUARD_LSE floats behind the LSE; every input element outside the
    operands is bf16 NaN and every output element a sentinel.  q | k | v share one buffer when T == S (the self-attention layout), else k | v do.
    The workspace is WS_EXCESS floats longer than the size offered to the library, sentinel throughout."""

    def __init__(self, hip, q, k, v, B, H, T, S, DH, scale, causal=False, gaps=False):
        self.lib, self.shape, self.scale, self.causal, self.dev = hip.lib, (B, H, T, S, DH), float(scale), int(bool(causal)), q.device
        d = H * DH
        self.d, self.fused = d, T == S
        self.gq, self.gk, self.guard, self.guard_lse, pad = (GAP_Q, GAP_K, GUARD_ROWS, GUARD_LSE, PAD_COLS) if gaps else (0, 0, 0, 0, 0)
        rq, rk = B * (T + self.gq) + self.guard, B * (S + self.gk) + self.guard
        self.shapes = [(max(rq, rk), 3 * d + pad)] if self.fused else [(rq, d + pad), (rk, 2 * d + pad)]
        self.o_shape = (rq, d + pad)
        self.inputs = self._operands([torch.full(s, float("nan"), dtype=bf16, device=self.dev) for s in self.shapes])
        for op, t in zip(self.inputs, (q, k, v)):
            op.put(t)

    def _operands(self, bufs):
        (B, H, T, S, DH), d = self.shape, self.d
        if self.fused:
            return [_Operand(bufs[0], B, T, self.gq, 0, d), _Operand(bufs[0], B, S, self.gk, d, d), _Operand(bufs[0], B, S, self.gk, 2 * d, d)]
        return [_Operand(bufs[0], B, T, self.gq, 0, d), _Operand(bufs[1], B, S, self.gk, 0, d), _Operand(bufs[1], B, S, self.gk, d, d)]

    def _tail(self, o_op):
        from e4t.ops import _stream
        B, H, T, S, DH = self.shape
        q, k, v = self.inputs
        return [B, H, T, S, DH, q.ld, k.ld, v.ld, o_op.ld, q.bstride, k.bstride, v.bstride, o_op.bstride, self.scale, self.causal, _stream()]

    def forward(self, need_lse=True):
        """-> dict(o [B*T, d], lse [B, H, T] | None, changed = sentinel elements overwritten, nan = NaN elements in O / LSE)"""
        from e4t import _C
        B, H, T, S, DH = self.shape
        o_op = _Operand(_sentinel_buf(*self.o_shape, self.dev), B, T, self.gq, 0, self.d)
        lse = torch.full((B * H * T + self.guard_lse,), SENT32, dtype=torch.int32, device=self.dev).view(f32)
        q, k, v = self.inputs
        _C.check(self.lib.e4t_attention_fwd(q.ptr, k.ptr, v.ptr, o_op.ptr, lse.data_ptr() if need_lse else None, *self._tail(o_op)), "e4t_attention_fwd")
        o, L = o_op.get(), lse[: B * H * T].reshape(B, H, T)
        changed = _changed_outside(o_op.buf, [o_op]) + int((lse.view(torch.int32)[B * H * T if need_lse else 0:] != SENT32).sum())
        nan = int(torch.isnan(o).sum()) + (int(torch.isnan(L).sum()) if need_lse else 0)
        return dict(o=o, lse=L.clone() if need_lse else None, changed=changed, nan=nan)

    def backward(self, o, do, lse, ws="full", entry="ws"):
        """-> dict(dq, dk, dv [B*T | B*S, d], changed = sentinel elements overwritten (gradient buffers and the workspace behind the offer), nan)"""
        from e4t import _C
        B, H, T, S, DH = self.shape
        nan16 = lambda: torch.full(self.o_shape, float("nan"), dtype=bf16, device=self.dev)
        o_op, do_op = _Operand(nan16(), B, T, self.gq, 0, self.d).put(o), _Operand(nan16(), B, T, self.gq, 0, self.d).put(do)
        L = torch.full((B * H * T + self.guard_lse,), float("nan"), dtype=f32, device=self.dev)
        L[: B * H * T] = lse.reshape(-1)
        gbufs = [_sentinel_buf(*s, self.dev) for s in self.shapes]
        grads = self._operands(gbufs)
        full = self.lib.e4t_attention_bwd_workspace_floats(B, H, T, S, DH)
        offer = {"full": full, "delta": B * H * T, "short": full - 1}[ws]
        wsb = torch.full((offer + WS_EXCESS,), SENT32, dtype=torch.int32, device=self.dev)
        q, k, v = self.inputs
        head = [q.ptr, k.ptr, v.ptr, o_op.ptr, do_op.ptr, L.data_ptr(), wsb.data_ptr()]
        out = [g.ptr for g in grads]
        if entry == "plain":
            assert ws == "delta", "e4t_attention_bwd takes no workspace size: it is B * H * T floats"
            _C.check(self.lib.e4t_attention_bwd(*head, *out, *self._tail(o_op)), "e4t_attention_bwd")
        else:
            _C.check(self.lib.e4t_attention_bwd_ws(*head, offer, *out, *self._tail(o_op)), "e4t_attention_bwd_ws")
        res = [g.get() for g in grads]
        changed = sum(_changed_outside(b_, [g for g in grads if g.buf is b_]) for b_ in gbufs) + int((wsb[offer:] != SENT32).sum())
        return dict(dq=res[0], dk=res[1], dv=res[2], changed=changed, nan=sum(int(torch.isnan(t).sum()) for t in res))


def _neq(a, b):
    """elements that differ bitwise (bf16 / fp32 tensors of one dtype)"""
    it = torch.int16 if a.dtype == bf16 else torch.int32
    return int((a.contiguous().view(it) != b.contiguous().view(it)).sum())


def attention_gap_rows(hip, tag, q, k, v, o, lse, do, grads, B, H, T, S, DH, scale, causal, ws="full", entry="ws"):
    """Forward and backward once more with batch strides beyond dense, NaN in every input gap and guard and sentinels in every output gap
    and guard (RawAttention, gaps=True), against o / lse / grads = what the dense-stride call made of the same inputs.  The kernels mask
    nothing: they rely on bounds-checked loads returning zeros behind a batch's last row, on L = +inf for query rows beyond T and on key
    lanes beyond S polluting only their own, never stored, column — a NaN that leaks in anywhere shows here.  The arithmetic of the two
    calls is the same (same kernels, same grid, same order), so the results must agree bitwise."""
    raw = RawAttention(hip, q, k, v, B, H, T, S, DH, scale, causal, gaps=True)
    f = raw.forward()
    b = raw.backward(o, do, lse, ws=ws, entry=entry)
    diff = _neq(f["o"], o) + _neq(f["lse"], lse) + sum(_neq(b[n], g) for n, g in zip(("dq", "dk", "dv"), grads))
    tag = f"{tag} gaps {GAP_Q} | {GAP_K} rows" + ("" if ws == "full" else f" ws={ws}")
    return [(tag + ": sentinel elements overwritten (O, LSE guard; dQ | dK | dV buffers, workspace excess)", float(f["changed"] + b["changed"]), 0.0),
            (tag + ": NaN in O, LSE, dQ, dK, dV", float(f["nan"] + b["nan"]), 0.0),
            (tag + ": elements differing bitwise from the dense-stride call", float(diff), 0.0)]


def _attention_inputs(g, B, H, T, S, DH, dev):
    """q, k, v as column slices of fused buffers (self-attn layout) when T == S, separate otherwise; gradient views of the same layout, twice"""
    d = H * DH
    if T == S:
        qkv = rnd(g, B * T, 3 * d, dev=dev)
        q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
        dqkv_h = torch.zeros_like(qkv); dqkv_e = torch.zeros_like(qkv)
        gh = (dqkv_h[:, :d], dqkv_h[:, d:2 * d], dqkv_h[:, 2 * d:])
        ge = (dqkv_e[:, :d], dqkv_e[:, d:2 * d], dqkv_e[:, 2 * d:])
    else:
        q = rnd(g, B * T, d, dev=dev)
        kv = rnd(g, B * S, 2 * d, dev=dev)
        k, v = kv[:, :d], kv[:, d:]
        dq_h, dq_e = torch.zeros_like(q), torch.zeros_like(q)
        dkv_h, dkv_e = torch.zeros_like(kv), torch.zeros_like(kv)
        gh = (dq_h, dkv_h[:, :d], dkv_h[:, d:]); ge = (dq_e, dkv_e[:, :d], dkv_e[:, d:])
    return q, k, v, gh, ge


def _attention_tag(case):
    B, H, T, S, DH = case[:5]
    return f"attn B{B} H{H} T{T} S{S} dh{DH}" + (" causal" if len(case) > 5 and case[5] else "")


def check_attention(hip, emu, dev):
    out = []
    for i, case in enumerate(ATTENTION_CASES):
        (B, H, T, S, DH), causal = case[:5], (len(case) > 5 and case[5])
        g = gen(90 + i, dev)
        q, k, v, gh, ge = _attention_inputs(g, B, H, T, S, DH, dev)
        scale = DH ** -0.5
        o, lse = hip.attention_fwd(q, k, v, B, H, T, S, DH, scale, causal=causal)
        o_r, lse_r = emu.attention_fwd(q, k, v, B, H, T, S, DH, scale, causal=causal)
        tag = _attention_tag(case)
        out.append((tag + " fwd O", rel(o, o_r), TOL2))
        out.append((tag + " fwd LSE", rel(lse, lse_r), 1e-3))
        do = rnd(g, B * T, H * DH, dev=dev)
        hip.attention_bwd(q, k, v, o, do, lse, gh[0], gh[1], gh[2], B, H, T, S, DH, scale, causal=causal)
        emu.attention_bwd(q, k, v, o_r, do, lse_r, ge[0], ge[1], ge[2], B, H, T, S, DH, scale, causal=causal)
        for nm, a, b in zip(("dQ", "dK", "dV"), gh, ge):
            out.append((tag + " bwd " + nm, rel(a, b), TOL2))
        # per (batch, head), and the ragged last tiles the shapes were chosen for, on their own (B * T >= 8192: per head only)
        out += attention_slices(tag, B, H, T, S, DH, o, o_r, lse, lse_r, gh, ge, blocks=B * T < 8192)
        if case in ATTENTION_NEW_CASES or case in ATTENTION_GAP_CASES:
            out += attention_gap_rows(hip, tag, q, k, v, o, lse, do, gh, B, H, T, S, DH, scale, causal)
        if case in ATTENTION_NULL_LSE_CASES:      # the sampling path: no LSE wanted
            o_n, _ = hip.attention_fwd(q, k, v, B, H, T, S, DH, scale, need_lse=False, causal=causal)
            out.append((tag + " fwd O without LSE: elements differing bitwise from O with it", float(_neq(o_n, o)), 0.0))
        del q, k, v, gh, ge, o, o_r, lse, lse_r, do
    out += _check_attention_determinism(hip, emu, dev)
    out += _check_attention_small_workspace(hip, emu, dev)
    out += _check_attention_peaked(hip, emu, dev)
    return out


def _check_attention_small_workspace(hip, emu, dev):
    """ATTENTION_WS_CASES: the backward through e4t_attention_bwd / e4t_attention_bwd_ws with a workspace that holds Delta only (or is one float
    short of the stated size).  The library then runs one query chunk instead of the split and leaves no {L, Delta} pairs, hence the
    register-staged dK/dV kernel behind a dQ kernel with LD == nullptr (which plan: tests/test_gemm_dispatch.py).  Against the emu backward,
    as every other case; against the full-workspace result of the same inputs to rounding (other kernels run: both sides carry their own bf16
    output rounding, rms 2^-9 / sqrt(3) = 1.1e-3 each, and P / dS rounded at other values — TOL1, as for single-rounding kernels); no float
    behind the offered size may change; and once more with gaps and poison."""
    out = []
    for j, (case, labels, entry) in enumerate(ATTENTION_WS_CASES):
        (B, H, T, S, DH), causal = case[:5], (len(case) > 5 and case[5])
        g = gen(600 + j, dev)
        q, k, v, gh, ge = _attention_inputs(g, B, H, T, S, DH, dev)
        scale = DH ** -0.5
        o, lse = hip.attention_fwd(q, k, v, B, H, T, S, DH, scale, causal=causal)
        o_r, lse_r = emu.attention_fwd(q, k, v, B, H, T, S, DH, scale, causal=causal)
        do = rnd(g, B * T, H * DH, dev=dev)
        hip.attention_bwd(q, k, v, o, do, lse, gh[0], gh[1], gh[2], B, H, T, S, DH, scale, causal=causal)
        emu.attention_bwd(q, k, v, o_r, do, lse_r, ge[0], ge[1], ge[2], B, H, T, S, DH, scale, causal=causal)
        raw = RawAttention(hip, q, k, v, B, H, T, S, DH, scale, causal)
        for ws in labels:
            tag = f"{_attention_tag(case)} ws={ws}" + (" (e4t_attention_bwd)" if entry == "plain" else "")
            r = raw.backward(o, do, lse, ws=ws, entry=entry)
            got = (r["dq"], r["dk"], r["dv"])
            for nm, a, b, f in zip(("dQ", "dK", "dV"), got, ge, gh):
                out.append((f"{tag} bwd {nm}", rel(a, b), TOL2))
                out.append((f"{tag} bwd {nm} ~ the full-workspace result", rel(a, f), TOL1))
            out += attention_slices(tag, B, H, T, S, DH, None, None, None, None, got, ge)
            out.append((tag + ": workspace floats behind the offered size overwritten", float(r["changed"]), 0.0))
            out.append((tag + ": NaN in dQ, dK, dV", float(r["nan"]), 0.0))
            out += attention_gap_rows(hip, _attention_tag(case), q, k, v, o, lse, do, got, B, H, T, S, DH, scale, causal, ws=ws, entry=entry)
    return out


def _check_attention_peaked(hip, emu, dev):
    """ATTENTION_PEAKED, forward and backward.  The backward of both sides gets the SAME O and LSE, the emu's: where the softmax is saturated
    dP - Delta cancels, and two differently rounded O would dominate the comparison instead of the backward kernels.  Whole tensor and
    64 / 128-row blocks only (slices())."""
    out = []
    for name, (_, (B, H, T, S, DH), _) in ATTENTION_PEAKED.items():
        q, k, v, do = peaked_attention_inputs(name, dev)
        tag = f"attn peaked-score {name} (T{T} S{S} dh{DH})"
        o, lse = hip.attention_fwd(q, k, v, B, H, T, S, DH, 1.0)
        o_r, lse_r = emu.attention_fwd(q, k, v, B, H, T, S, DH, 1.0)
        out.append((tag + " fwd O", rel(o, o_r), TOL2))
        out.append((tag + " fwd LSE", rel(lse, lse_r), 1e-3))
        gh, ge = [torch.zeros_like(t) for t in (q, k, v)], [torch.zeros_like(t) for t in (q, k, v)]
        hip.attention_bwd(q, k, v, o_r, do, lse_r, gh[0], gh[1], gh[2], B, H, T, S, DH, 1.0)
        emu.attention_bwd(q, k, v, o_r, do, lse_r, ge[0], ge[1], ge[2], B, H, T, S, DH, 1.0)
        for nm, a, b in zip(("dQ", "dK", "dV"), gh, ge):
            out.append((tag + " bwd " + nm, rel(a, b), TOL2))
        out += attention_slices(tag, B, H, T, S, DH, o, o_r, lse, lse_r, gh, ge, every_block=True)
        if name == "dh40 long-key T256":      # ... and through attn_bwd_dkv_kernel<40, 2>, which a Delta-only workspace gives this shape
            r = RawAttention(hip, q, k, v, B, H, T, S, DH, 1.0).backward(o_r, do, lse_r, ws="delta")
            got = (r["dq"], r["dk"], r["dv"])
            for nm, a, b in zip(("dQ", "dK", "dV"), got, ge):
                out.append((f"{tag} ws=delta bwd {nm}", rel(a, b), TOL2))
            out += attention_slices(tag + " ws=delta", B, H, T, S, DH, None, None, None, None, got, ge, every_block=True)
            out.append((tag + " ws=delta: workspace floats behind the offered size overwritten", float(r["changed"]), 0.0))
    return out


def _check_attention_determinism(hip, emu, dev):
    out = []
    # The step's own dh-40 self-attention at the bench batch (B16 H8 T = S = 4096: 2048-4096 workgroups = several rounds of two / three
    # resident workgroups per CU — the regime in which round 6's LDS-DMA kernels first showed a race: pad columns written into rows
    # whose DMA piece another wave still had in flight; every smaller case above ran one round and passed): outputs must be BITWISE equal
    # run to run, and equal to a second evaluation in four batch chunks of B = 4 (other grid, other residency) to rounding.
    g = gen(119, dev)
    B, H, T, S, DH = 16, 8, 4096, 4096, 40
    d = H * DH
    qkv = rnd(g, B * T, 3 * d, scale=0.7, dev=dev)
    q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    do = rnd(g, B * T, d, dev=dev)
    runs = []
    for rep in range(3):
        o, lse = hip.attention_fwd(q, k, v, B, H, T, S, DH, DH ** -0.5)
        gq = torch.zeros_like(qkv)
        hip.attention_bwd(q, k, v, o, do, lse, gq[:, :d], gq[:, d:2 * d], gq[:, 2 * d:], B, H, T, S, DH, DH ** -0.5)
        runs.append((o.clone(), lse.clone(), gq))
    for rep in (1, 2):
        out.append((f"attn B16 H8 T4096 dh40 run {rep} == run 0 bitwise (O, LSE, dQ|dK|dV)",
                    float(sum((a != b).sum() for a, b in zip(runs[rep], runs[0]))), 0.0))
    o4, g4 = torch.empty_like(runs[0][0]), torch.zeros_like(qkv)
    for c in range(4):
        sl = slice(c * 4 * T, (c + 1) * 4 * T)
        oc, lc = hip.attention_fwd(q[sl], k[sl], v[sl], 4, H, T, S, DH, DH ** -0.5)
        o4[sl] = oc
        hip.attention_bwd(q[sl], k[sl], v[sl], oc, do[sl], lc, g4[sl, :d], g4[sl, d:2 * d], g4[sl, 2 * d:], 4, H, T, S, DH, DH ** -0.5)
    out.append(("attn B16 == 4 x B4 fwd O", rel(runs[0][0], o4), 1e-5))
    for nm, sl_ in (("dQ", slice(0, d)), ("dK", slice(d, 2 * d)), ("dV", slice(2 * d, 3 * d))):
        out.append((f"attn B16 == 4 x B4 bwd {nm}", rel(runs[0][2][:, sl_], g4[:, sl_]), 1e-5))
    del runs, o4, g4, qkv, do
    return out


# ------------------------------------------------------------------------------------------------ norms
# Plain data and host arithmetic, importable without a GPU: tests/test_norm_plan_cpu.py holds norm_plan() against a hand-written table of every
# logged instantiation of norm.hip, tests/test_norm_slices_cpu.py holds a rounding-only model to half the tolerance on every row norm_slices()
# emits for these cases and measures the statistics tolerance (STAT_TOL).
f64 = torch.float64
GNCase = namedtuple("GNCase", "B HW C1 C2 G silu eps shift adds seed new")
GN_SLAB_MAX = 10240      # norm.hip: elements of one (batch, group) slab the one-launch kernels take
GN_MIN_REGION = 256      # gn_slices: values in the smallest region of pixel rows it reports


def _gn(B, HW, C1, C2, silu, G=32, eps=1e-5, shift=0.0, adds=((True, True),)):
    adds = tuple((a1, a2 and C2 > 0) for a1, a2 in adds)
    return GNCase(B, HW, C1, C2, G, silu, eps, shift, adds, 0, True)


# (B, HW, C1, C2, G, silu) of the first list: the cases check_norms has always run, with their seeds (140 + i) and their shortcut gradients (add1
# on the even ones, add2 wherever there is a second source except on case 3).  The last six take the one-launch slab kernels (HW x C/G <= 10240,
# C/G % 4 == 0, no group straddling the concat): 3 / 5 / 10 quads per thread, two sources, with and without SiLU / shortcut gradients.
_GN_FIRST = [(2, 64, 64, 0, 32, True), (3, 256, 320, 0, 32, True), (2, 100, 320, 640, 32, True), (2, 64, 1280, 1280, 32, False), (16, 4096, 320, 0, 32, True),
             (2, 64, 1280, 0, 32, True), (3, 256, 1280, 0, 32, True), (2, 64, 1280, 1280, 32, True), (2, 60, 640, 0, 32, True), (1, 256, 640, 640, 32, False),
             (2, 64, 640, 640, 32, True)]
GN_CASES = [GNCase(B, HW, C1, C2, G, silu, 1e-5, 0.0, ((i % 2 == 0, bool(C2) and i != 3),), 140 + i, False) for i, (B, HW, C1, C2, G, silu) in enumerate(_GN_FIRST)]
GN_NEW_CASES = [
    _gn(2, 256, 1280, 1280, True),       # chunked, two slots, two sources: the UNet's 16 x 16 up-block concat (gn_apply<true, 2>, gn_stats<2>, colstats with cs2)
    _gn(2, 256, 1280, 640, True, adds=((True, False), (False, True))),      # C = 1920: 240 chunk lanes, 16 idle threads; cpg = 60 straddles the concat and the 8-channel chunks
    _gn(2, 260, 320, 0, True),           # ch = 32, ppc = 9: three empty trailing chunks, a ragged last one (8 of 9 pixels)
    _gn(1, 257, 1280, 0, False),         # one pixel over the slab limit (HW * cpg = 10280): chunked; three empty trailing chunks, 5 of 9 pixels in the last
    _gn(2, 16, 320, 320, False),         # slab NI = 3 without SiLU: 80 items, trips 1 and 2 fully masked (the `items - 1` clamp)
    _gn(2, 100, 640, 640, True),         # slab NI = 5: 1000 items, ragged
    _gn(2, 100, 1280, 1280, True),       # slab NI = 10: 2000 items, two trips fully masked, one ragged
    _gn(2, 64, 64, 0, False, eps=1e-6),  # Transformer2DModel.norm's eps
    _gn(48, 1024, 64, 0, True),          # ch = 21, 32 blocks of 32 pixels: 32 % 21 != 0, groupnorm_fwd falls back to the statistics pass
    _gn(2, 1024, 320, 0, True, shift=64.0),      # mean^2 / var ~ 1.5e4: pins the fp64 finalisation of E[x^2] - mean^2 (chunked, and via column statistics)
    _gn(2, 64, 1280, 0, True, shift=64.0),       # ... and in the slab kernel
]
GN_NEW_CASES = [c._replace(seed=1400 + i) for i, c in enumerate(GN_NEW_CASES)]
GN_CASES += GN_NEW_CASES
# (M, D).  The last three of the first eight take the several-rows-per-wave forward (4 / 2 / 2 rows for 1 / 2 / 3 chunks per lane) with a ragged last wave
LN_CASES = [(37, 64), (1000, 320), (4112, 1280), (300, 768), (128, 1024), (8195, 320), (4101, 640), (4111, 1280),
            (300, 1280),       # ln_fwd_kernel<3, 1, false>: D = 1280 with fewer than 2731 rows (the 16 x 16 transformer at small batch)
            (5, 1536),         # the largest D, fewer rows than one block
            (4101, 200)]       # D % 64 != 0 for the parameter-gradient column blocks; 25 of 64 lanes active
LN_NEED_STATS_CASE = (300, 768)      # once more with need_stats=False (mean_rstd == NULL)
# Worst |d mean| * rstd and |d rstd| / rstd of a (batch, group) against fp64.  tests/test_norm_slices_cpu.py measures the model of the kernels'
# statistics (one fp32 chain per chunk or slab thread, fp64 across, fp32 store) at 6.0e-6 — the fp32 store of a mean of 64 at rstd 1.9, on the
# shifted-mean cases; 1.05e-6 on every other case — and asserts STAT_TOL == min(4 x that, 1e-5): the cap binds.
STAT_TOL = 1e-5


def gn_tag(c):
    return f"groupnorm B{c.B} HW{c.HW} C{c.C1}+{c.C2} silu{int(c.silu)}" + (f" eps{c.eps:g}" if c.eps != 1e-5 else "") + (f" shift{c.shift:g}" if c.shift else "")


def gn_slab_ni(C1, C2, HW, G):
    """norm.hip gn_slab_ni: quads per thread of the slab kernels, 0 = not eligible"""
    cpg = (C1 + C2) // G
    if cpg % 4 != 0 or (C2 > 0 and C1 % cpg != 0) or HW * cpg > GN_SLAB_MAX:
        return 0
    ni = -(-HW * (cpg // 4) // 256)
    return 3 if ni <= 3 else 5 if ni <= 5 else 10


def gn_chunks(B, HW):
    """norm.hip gn_chunks: workgroups per batch entry of the chunked kernels"""
    return min(max(1024 // max(B, 1), 1), max(HW // 8, 1), 256)


def ln_rows_per_wave(M, D, xf32=False):
    """norm.hip launch_ln_fwd: (16-byte chunks per lane, rows per wave)"""
    ncl = -(-(D // 8) // 64)
    return ncl, (1 if (M * ncl < 256 * 4 * 8 or xf32) else 4 if ncl == 1 else 2)


def norm_plan(case):
    """What the library does with a case, restated from norm.hip's dispatch (gn_slab_ni, gn_chunks, GN_TWO_SLOTS, the rpw rule of launch_ln_fwd) and
    the colstats precondition of ops.groupnorm_fwd: calls = {call form: [launch-log symbols in launch order]}, symbols = their union, and the
    geometry the slices need.  GroupNorm call forms: fwd, fwd_cs (column statistics attached; HW % 32 == 0 only), unfused (e4t_groupnorm_stats +
    _apply), bwd_pg (with parameter gradients: always chunked), bwd.  LayerNorm: fwd, fwd_f32, bwd."""
    if not isinstance(case, GNCase):
        M, D = case
        ncl, rpw = ln_rows_per_wave(M, D)
        nc = min(ncl, 3)
        calls = {"fwd": [f"ln_fwd_kernel<{nc}, {rpw}, false>"], "fwd_f32": [f"ln_fwd_kernel<{nc}, 1, true>"], "bwd": [f"ln_bwd_kernel<{nc}>"]}
        return dict(calls=calls, symbols={s for v in calls.values() for s in v}, ncl=ncl, rpw=rpw)
    c = case
    C = c.C1 + c.C2
    ns = 2 if C // 8 > 256 else 1
    ni = gn_slab_ni(c.C1, c.C2, c.HW, c.G)
    ch = gn_chunks(c.B, c.HW)
    ppc = -(-c.HW // ch)
    nblk = c.HW // 32
    cs_ok = c.HW % 32 == 0 and nblk % min(ch, nblk) == 0
    t = "true" if c.silu else "false"
    two_pass = [f"gn_stats_kernel<{ns}>", f"gn_apply_kernel<true, {ns}>"]
    bwd = [f"gn_bwd_stats_kernel<{ns}>", f"gn_bwd_apply_kernel<{ns}>"]
    calls = {"fwd": [f"gn_slab_fwd_kernel<{ni}, {t}>"] if ni else two_pass,
             "unfused": [f"gn_stats_kernel<{ns}>", f"gn_apply_kernel<false, {ns}>"],
             "bwd_pg": bwd, "bwd": [f"gn_slab_bwd_kernel<{ni}, {t}>"] if ni else bwd}
    if c.HW % 32 == 0:
        calls["fwd_cs"] = calls["fwd"] if (ni or not cs_ok) else ["gn_stats_cols_kernel", f"gn_apply_kernel<true, {ns}>"]
    return dict(calls=calls, symbols={s for v in calls.values() for s in v}, ns=ns, ni=ni, ch=ch, ppc=ppc, empty=ch - -(-c.HW // ppc), colstats=cs_ok)


def gn_inputs(case, dev):
    """x1, x2, gamma, beta, dy, add1, add2 of a case (add1 / add2: None where no backward variant of the case uses them)"""
    c, g = case, gen(case.seed, dev)
    n, C = c.B * c.HW, c.C1 + c.C2
    if c.shift:      # x = shift + 0.5 randn, rounded to bf16 once
        x1 = (torch.randn(n, c.C1, generator=g, device=dev, dtype=f32) * 0.5 + c.shift).to(bf16)
    else:
        x1 = rnd(g, n, c.C1, dev=dev) + 0.3
    x2 = rnd(g, n, c.C2, scale=2.0, dev=dev) if c.C2 else None
    gamma, beta = rnd(g, C, dtype=f32, dev=dev) * 0.3 + 1.0, rnd(g, C, dtype=f32, dev=dev) * 0.2
    dy = rnd(g, n, C, dev=dev)
    add1 = rnd(g, n, c.C1, dev=dev) if any(a for a, _ in c.adds) else None
    add2 = rnd(g, n, c.C2, dev=dev) if any(a for _, a in c.adds) else None
    return x1, x2, gamma, beta, dy, add1, add2


def ln_inputs(case, i, dev):
    """x, gamma, beta, dy, x32 (fp32 rows), skip (a residual gradient) of LN_CASES[i]"""
    M, D = case
    g = gen(160 + i, dev)
    x = rnd(g, M, D, dev=dev) + 0.5
    gamma, beta = rnd(g, D, dtype=f32, dev=dev) * 0.3 + 1.0, rnd(g, D, dtype=f32, dev=dev) * 0.2
    dy = rnd(g, M, D, dev=dev)
    x32 = (rnd(g, M, D, dtype=f32, dev=dev) + 0.5) * 3.0
    return x, gamma, beta, dy, x32, rnd(g, M, D, dev=dev)


def _cat64(x1, x2):
    return x1.to(f64) if x2 is None else torch.cat([x1.to(f64), x2.to(f64)], dim=-1)


def _silu64(z):
    return z * torch.sigmoid(z)


def _dsilu64(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def gn_ref64_fwd(x1, x2, gamma, beta, B, HW, G, eps, silu):
    """fp64 GroupNorm (+ SiLU) of the bf16 inputs, two-pass variance -> y [B * HW, C], stats [B, G, 2] = (mean, rstd), both fp64"""
    x = _cat64(x1, x2)
    C = x.shape[-1]
    xg = x.reshape(B, HW, G, C // G)
    mean = xg.mean(dim=(1, 3), keepdim=True)
    xc = xg - mean
    rstd = (xc.square().mean(dim=(1, 3), keepdim=True) + eps).rsqrt()
    y = (xc * rstd).reshape(B * HW, C) * gamma.to(f64) + beta.to(f64)
    return (_silu64(y) if silu else y), torch.stack([mean.reshape(B, G), rstd.reshape(B, G)], dim=-1)


def gn_ref64_bwd(x1, x2, dy, stats, gamma, beta, add1, add2, B, HW, G, silu):
    """fp64 GroupNorm backward from `stats` as the kernel receives them (the forward's fp64 statistics rounded to fp32)
    -> dx [B * HW, C] (dx1 | dx2 side by side), dgamma, dbeta"""
    x = _cat64(x1, x2)
    C, C1 = x.shape[-1], x1.shape[-1]
    cpg = C // G
    st = stats.to(f64)
    mean, rstd = st[..., 0].reshape(B, 1, G, 1), st[..., 1].reshape(B, 1, G, 1)
    xh = (x.reshape(B, HW, G, cpg) - mean) * rstd
    dz = dy.to(f64)
    if silu:
        dz = dz * _dsilu64(xh.reshape(B * HW, C) * gamma.to(f64) + beta.to(f64))
    dzg = (dz * gamma.to(f64)).reshape(B, HW, G, cpg)
    s1, s2 = dzg.mean(dim=(1, 3), keepdim=True), (dzg * xh).mean(dim=(1, 3), keepdim=True)
    dx = (rstd * (dzg - s1 - xh * s2)).reshape(B * HW, C)
    if add1 is not None:
        dx[:, :C1] += add1.to(f64)
    if add2 is not None:
        dx[:, C1:] += add2.to(f64)
    return dx, (dz * xh.reshape(B * HW, C)).sum(0), dz.sum(0)


def ln_ref64_fwd(x, gamma, beta, eps):
    """fp64 LayerNorm of bf16 / fp32 rows, two-pass variance -> y [M, D], stats [M, 2] = (mean, rstd)"""
    xd = x.to(f64)
    mean = xd.mean(-1, keepdim=True)
    xc = xd - mean
    rstd = (xc.square().mean(-1, keepdim=True) + eps).rsqrt()
    return xc * rstd * gamma.to(f64) + beta.to(f64), torch.cat([mean, rstd], dim=-1)


def ln_ref64_bwd(x, dy, gamma, stats, add=None):
    """fp64 LayerNorm backward from the fp32 `stats` the kernel receives -> dx, dgamma, dbeta"""
    st = stats.to(f64)
    xh = (x.to(f64) - st[:, :1]) * st[:, 1:]
    dg = dy.to(f64) * gamma.to(f64)
    dx = st[:, 1:] * (dg - dg.mean(-1, keepdim=True) - xh * (dg * xh).mean(-1, keepdim=True))
    if add is not None:
        dx = dx + add.to(f64)
    return dx, (dy.to(f64) * xh).sum(0), dy.to(f64).sum(0)


def _region(d, n):
    """relative L2 from sums of squared differences d and squared reference values n (tensors of one shape): the worst entry, NaN -> inf"""
    e = (d / (n + 1e-300)).sqrt()
    return float(torch.nan_to_num(e, nan=float("inf"), posinf=float("inf")).max())


def gn_slices(tag, got, ref, case, chunked, tol=TOL1):
    """Rows a whole-tensor relative L2 dilutes, each the worst of its kind: got, ref = [B * HW, C] (y, or dx1 | dx2 side by side; ref fp64).
      - the worst (batch, group);
      - chunked=True (the chunked kernels: pixels split into norm_plan's ch chunks of ppc): the worst first and the worst last pixel row of a chunk
        (all C channels of one pixel — the masked tail of the `unconditional load, masked store` loop is the last).  Coarsened for C < 256 to as
        many pixel rows as make GN_MIN_REGION = 256 values: the rounding-only model of one pixel row of 64 channels, worst of 1008, is 3.2e-3;
      - two sources: the 8-channel chunks on either side of the concat boundary;
      - the 8 channels of the last active thread, and the second slot's channels (2048 and up) for C > 2048;
      - chunked=False (the slab kernels): the worst last pixel row (the last item row of every group) and the worst (batch, group) of the items
        of the last, ragged trip of 256 quads.
    Never finer than a whole pixel row or 170 values: the rounding-only model of a single (pixel, group) cell of 10 channels reaches 3.7e-3,
    over half the tolerance, the worst row emitted here 2.0e-3 (tests/test_norm_slices_cpu.py)."""
    c, pl = case, norm_plan(case)
    B, HW, G, C = c.B, c.HW, c.G, c.C1 + c.C2
    cpg = C // G
    d2 = (got.to(f64) - ref.to(f64)).square().reshape(B, HW, C)
    r2 = ref.to(f64).square().reshape(B, HW, C)
    out = []

    def row(label, d, n):
        out.append((f"{tag}: {label}", _region(d, n), tol))
    row("worst (batch, group)", d2.reshape(B, HW, G, cpg).sum(dim=(1, 3)), r2.reshape(B, HW, G, cpg).sum(dim=(1, 3)))
    dp, rp = d2.sum(-1), r2.sum(-1)      # [B, HW]: whole pixel rows
    if chunked:
        first = torch.arange(0, HW, pl["ppc"], device=got.device)
        last = torch.clamp(first + pl["ppc"], max=HW) - 1
        k = min(-(-GN_MIN_REGION // C), pl["ppc"])      # pixel rows per region: 1 from C = 256 up
        what = "pixel row" if k == 1 else f"{k} pixel rows"
        ends = lambda sgn, t: sum(torch.where((first + j <= last), t[:, (first + j) if sgn > 0 else torch.clamp(last - j, min=0)], 0.0) for j in range(k))
        row(f"worst first {what} of a chunk ({len(first)} chunks of {pl['ppc']})", ends(1, dp), ends(1, rp))
        row(f"worst last {what} of a chunk (the last: pixel {int(last[-1])})", ends(-1, dp), ends(-1, rp))
    else:
        row(f"worst last pixel row (pixel {HW - 1}: the last item row)", dp[:, HW - 1], rp[:, HW - 1])
        q4 = cpg // 4
        t0 = (-(-HW * q4 // 256) - 1) * 256
        if t0 > 0:
            item = torch.arange(HW, device=got.device)[:, None] * q4 + torch.arange(cpg, device=got.device)[None, :] // 4
            m = (item >= t0).to(f64)[None, :, None, :]
            row(f"worst (batch, group) of items {t0}-{HW * q4 - 1} (the last trip)", (d2.reshape(B, HW, G, cpg) * m).sum(dim=(1, 3)), (r2.reshape(B, HW, G, cpg) * m).sum(dim=(1, 3)))
    if c.C2:
        row(f"channels {c.C1 - 8}-{c.C1 - 1} (the last chunk of the first source)", d2[..., c.C1 - 8:c.C1].sum(), r2[..., c.C1 - 8:c.C1].sum())
        row(f"channels {c.C1}-{c.C1 + 7} (the first chunk of the second source)", d2[..., c.C1:c.C1 + 8].sum(), r2[..., c.C1:c.C1 + 8].sum())
    row(f"channels {C - 8}-{C - 1} (the last active thread)", d2[..., C - 8:].sum(), r2[..., C - 8:].sum())
    if C > 2048:
        row(f"channels 2048-{C - 1} (the second slot)", d2[..., 2048:].sum(), r2[..., 2048:].sum())
    return out


def gn_stat_rows(tag, st, st64, tol=STAT_TOL):
    """statistics [B, G, 2] = (mean, rstd) against fp64: the worst |d mean| * rstd and |d rstd| / rstd of one (batch, group)"""
    d = (st.to(f64) - st64).abs()
    nn = lambda t: float(torch.nan_to_num(t, nan=float("inf")).max())
    return [(f"{tag}: worst |d mean| * rstd of a (batch, group) against fp64", nn(d[..., 0] * st64[..., 1]), tol),
            (f"{tag}: worst |d rstd| / rstd of a (batch, group) against fp64", nn(d[..., 1] / st64[..., 1]), tol)]


def ln_slices(tag, got, ref, rpw, tol=TOL1):
    """LayerNorm y / dx [M, D] against fp64, each row the worst of its kind:
      - the worst row (the rounding-only model of a single row stays under half the tolerance even at D = 64: 2.3e-3 at worst over all cases);
      - the rows of the last wave (rpw rows per wave: the forward's 1 / 2 / 4, the backward's 1) and the rows of the last block of 4 waves: ragged
        where M is no multiple, reported separately;
      - the last active 16-byte chunk of a row (columns D - 8 .. D - 1) and the first chunk of each lane trip (columns 512 i .. 512 i + 7)."""
    M, D = ref.shape
    d2, r2 = (got.to(f64) - ref.to(f64)).square(), ref.to(f64).square()
    dr, rr = d2.sum(1), r2.sum(1)
    out = []

    def row(label, d, n):
        out.append((f"{tag}: {label}", _region(d, n), tol))
    row("worst row", dr, rr)
    w0, b0 = (M - 1) // rpw * rpw, (M - 1) // (4 * rpw) * (4 * rpw)
    row(f"rows {w0}-{M - 1} (the last wave, {rpw} per wave)", dr[w0:].sum(), rr[w0:].sum())
    row(f"rows {b0}-{M - 1} (the last block, {4 * rpw} per block)", dr[b0:].sum(), rr[b0:].sum())
    row(f"columns {D - 8}-{D - 1} (the last active chunk)", d2[:, D - 8:].sum(), r2[:, D - 8:].sum())
    for i in range(-(-D // 512)):
        row(f"columns {512 * i}-{512 * i + 7} (the first chunk of lane trip {i})", d2[:, 512 * i:512 * i + 8].sum(), r2[:, 512 * i:512 * i + 8].sum())
    return out


def colblock_rows(tag, got, ref, tol=1e-3):
    """parameter gradients [C] against fp64: the worst block of 64 columns (the column block of one colreduce workgroup; the last may be ragged)"""
    d2, r2 = (got.to(f64) - ref.to(f64)).square(), ref.to(f64).square()
    C = ref.numel()
    worst = max(_region(d2[lo:lo + 64].sum(), r2[lo:lo + 64].sum()) for lo in range(0, C, 64))
    return [(f"{tag}: worst 64-column block", worst, tol)]


def norm_slices(tag, got, ref, case, chunked=True, rpw=1, tol=TOL1):
    """the localised rows of one norm output, in the style of slices() and conv_slices(): gn_slices() for a GNCase, ln_slices() for (M, D)"""
    if isinstance(case, GNCase):
        return gn_slices(tag, got, ref, case, chunked, tol)
    return ln_slices(tag, got, ref, rpw, tol)


def _logged(hip, fn):
    """run fn() with the library's launch log on -> (fn's result, [kernel symbol per logged launch])"""
    import os
    import tempfile
    fd, path = tempfile.mkstemp(suffix=".launchlog")
    os.close(fd)
    try:
        assert hip.lib.e4t_set_launch_log(path.encode()) == 0
        try:
            res = fn()
            torch.cuda.synchronize()
        finally:
            hip.lib.e4t_set_launch_log(None)
        with open(path) as f:
            return res, [l.split("|")[0] for l in f.read().splitlines() if l]
    finally:
        os.unlink(path)


def _plan_row(tag, form, logged, planned):
    return (f"{tag}: launch log of {form} == the plan {planned}" + ("" if logged == planned else f" (logged {logged})"), float(logged != planned), 0.0)


def _with_colstats(t):
    """the column statistics a producing GEMM / conv epilogue would have left on t: [rows / 32][C][2] = (sum, sum of squares) per 32-row block"""
    blk = t.float().reshape(t.shape[0] // 32, 32, t.shape[1])
    t._e4t_colstats = torch.stack([blk.sum(1), (blk * blk).sum(1)], dim=-1).contiguous()
    return t


def _cat(a, b):
    return a if b is None else torch.cat([a, b], dim=-1)


def _check_groupnorm_case(hip, emu, dev, c):
    out = []
    B, HW, C1, C2, G, silu, eps = c.B, c.HW, c.C1, c.C2, c.G, c.silu, c.eps
    pl, tag = norm_plan(c), gn_tag(c)
    slab = pl["ni"] > 0
    x1, x2, gamma, beta, dy, a1, a2 = gn_inputs(c, dev)
    geo = (gamma, beta, B, HW, G, eps, silu)
    (y, st), log = _logged(hip, lambda: hip.groupnorm_fwd(x1, x2, *geo))
    out.append(_plan_row(tag, "fwd", log, pl["calls"]["fwd"]))
    yr, str_ = emu.groupnorm_fwd(x1, x2, *geo)
    y64, st64 = gn_ref64_fwd(x1, x2, *geo)
    out.append((tag + " fwd", rel(y, yr), TOL1))
    out.append((tag + " stats", rel(st, str_), 1e-4))
    out += gn_slices(tag + " fwd vs fp64", y, y64, c, not slab)
    out += gn_stat_rows(tag + " stats", st, st64)
    if HW % 32 == 0:       # the same GroupNorm fed with the column statistics a producing GEMM would have left behind
        x1c, x2c = _with_colstats(x1.clone()), (_with_colstats(x2.clone()) if x2 is not None else None)
        (y3, st3), log = _logged(hip, lambda: hip.groupnorm_fwd(x1c, x2c, *geo))
        out.append(_plan_row(tag, "fwd with column statistics", log, pl["calls"]["fwd_cs"]))
        out.append((tag + " via column statistics: y", rel(y3, y), 2e-3))
        out.append((tag + " via column statistics: stats", rel(st3, st), 1e-4))
        if c.new:
            out += gn_slices(tag + " via column statistics vs fp64", y3, y64, c, not slab)
            out += gn_stat_rows(tag + " via column statistics: stats", st3, st64)
    (y2, st2), log = _logged(hip, lambda: hip.groupnorm_fwd_unfused(x1, x2, *geo))
    out.append(_plan_row(tag, "stats/finalize/apply", log, pl["calls"]["unfused"]))
    if slab:     # one-launch kernel: same arithmetic, different summation tree
        out.append((tag + " slab kernel ~ stats/finalize/apply entry points: y", rel(y, y2), 2e-3))
        out.append((tag + " slab kernel ~ stats/finalize/apply entry points: stats", rel(st, st2), 1e-5))
        out += gn_slices(tag + " stats/finalize/apply vs fp64", y2, y64, c, True)      # (their statistics: the rows of the chunked cases, bitwise the fused path's)
    else:
        out.append((tag + f" fused == stats/finalize/apply entry points (NS = {pl['ns']})", float((y2 != y).sum() + (st2 != st).sum()), 0.0))
    st32 = st64.to(f32)      # what the fp64 backward and the kernel both start from
    for add1, add2 in ((a1 if u1 else None, a2 if u2 else None) for u1, u2 in c.adds):
        vt = tag + ("" if len(c.adds) == 1 else f" add{'1' if add1 is not None else '2'} only")
        bw = (x1, x2, dy)
        tail = (B, HW, G, silu)
        dx1, dx2, dga, dbe = hip.groupnorm_bwd(*bw, str_, gamma, beta, add1, *tail, want_param_grads=True, add2=add2)
        ex1, ex2, ega, ebe = emu.groupnorm_bwd(*bw, str_, gamma, beta, add1, *tail, want_param_grads=True, add2=add2)
        out.append((vt + " bwd dx1", rel(dx1, ex1), TOL1))
        if C2:
            out.append((vt + " bwd dx2", rel(dx2, ex2), TOL1))
        out.append((vt + " bwd dgamma", rel(dga, ega), 1e-3))
        out.append((vt + " bwd dbeta", rel(dbe, ebe), 1e-3))
        # frozen gamma / beta (pre-training): no parameter-gradient partials -> slab kernel where eligible
        fx1, fx2, _, _ = hip.groupnorm_bwd(*bw, str_, gamma, beta, add1, *tail, want_param_grads=False, add2=add2)
        out.append((vt + " bwd dx1 (no param grads)", rel(fx1, ex1), TOL1))
        if C2:
            out.append((vt + " bwd dx2 (no param grads)", rel(fx2, ex2), TOL1))
        # ... and against fp64, from the fp64 statistics rounded to fp32, localised
        d64, ga64, be64 = gn_ref64_bwd(*bw, st32, gamma, beta, add1, add2, *tail)
        (dx1, dx2, dga, dbe), log = _logged(hip, lambda: hip.groupnorm_bwd(*bw, st32, gamma, beta, add1, *tail, want_param_grads=True, add2=add2))
        out.append(_plan_row(vt, "bwd with parameter gradients", log, pl["calls"]["bwd_pg"]))
        out += gn_slices(vt + " bwd dx1 | dx2 vs fp64", _cat(dx1, dx2), d64, c, True)
        out += colblock_rows(vt + " bwd dgamma vs fp64", dga, ga64) + colblock_rows(vt + " bwd dbeta vs fp64", dbe, be64)
        (fx1, fx2, _, _), log = _logged(hip, lambda: hip.groupnorm_bwd(*bw, st32, gamma, beta, add1, *tail, want_param_grads=False, add2=add2))
        out.append(_plan_row(vt, "bwd", log, pl["calls"]["bwd"]))
        out += gn_slices(vt + " bwd dx1 | dx2 (no param grads) vs fp64", _cat(fx1, fx2), d64, c, not slab)
        if c.new:      # the file's header claims a fixed summation order: repeated launches are bitwise equal
            differing = 0
            for _ in range(2):
                yb, sb = hip.groupnorm_fwd(x1, x2, *geo)
                g1, g2, gg, gb = hip.groupnorm_bwd(*bw, st32, gamma, beta, add1, *tail, want_param_grads=True, add2=add2)
                h1, h2, _, _ = hip.groupnorm_bwd(*bw, st32, gamma, beta, add1, *tail, want_param_grads=False, add2=add2)
                differing += _neq(yb, y) + _neq(sb, st) + _neq(g1, dx1) + _neq(gg, dga) + _neq(gb, dbe) + _neq(h1, fx1)
                if C2:
                    differing += _neq(g2, dx2) + _neq(h2, fx2)
            out.append((vt + ": elements differing bitwise between three launches (y, stats, dx, dgamma, dbeta)", float(differing), 0.0))
    return out


def _check_layernorm_case(hip, emu, dev, i, case):
    out = []
    M, D = case
    pl, tag = norm_plan(case), f"layernorm {M}x{D}"
    x, gamma, beta, dy, x32, skip = ln_inputs(case, i, dev)
    (y, st), log = _logged(hip, lambda: hip.layernorm_fwd(x, gamma, beta, 1e-5))
    out.append(_plan_row(tag, "fwd", log, pl["calls"]["fwd"]))
    yr, str_ = emu.layernorm_fwd(x, gamma, beta, 1e-5)
    y64, st64 = ln_ref64_fwd(x, gamma, beta, 1e-5)
    out.append((f"{tag} fwd", rel(y, yr), TOL1))
    out.append((f"{tag} stats", rel(st, str_), 1e-4))
    out += ln_slices(f"{tag} fwd vs fp64", y, y64, pl["rpw"])
    (dx, dga, dbe), log = _logged(hip, lambda: hip.layernorm_bwd(x, dy, gamma, str_, want_param_grads=True))
    out.append(_plan_row(tag, "bwd", log, pl["calls"]["bwd"]))
    ex, ega, ebe = emu.layernorm_bwd(x, dy, gamma, str_, want_param_grads=True)
    out.append((f"{tag} bwd dx", rel(dx, ex), TOL1))
    out.append((f"{tag} bwd dgamma", rel(dga, ega), 1e-3))
    out.append((f"{tag} bwd dbeta", rel(dbe, ebe), 1e-3))
    st32 = st64.to(f32)
    d64, ga64, be64 = ln_ref64_bwd(x, dy, gamma, st32)
    dx, dga, dbe = hip.layernorm_bwd(x, dy, gamma, st32, want_param_grads=True)
    out += ln_slices(f"{tag} bwd dx vs fp64", dx, d64, 1)
    out += colblock_rows(f"{tag} bwd dgamma vs fp64", dga, ga64) + colblock_rows(f"{tag} bwd dbeta vs fp64", dbe, be64)
    (y32, s32), log = _logged(hip, lambda: hip.layernorm_fwd(x32, gamma, beta, 1e-5))      # fp32 rows (ViT residual stream) -> bf16 y
    out.append(_plan_row(tag, "fwd, fp32 input", log, pl["calls"]["fwd_f32"]))
    yr32, str32 = emu.layernorm_fwd(x32, gamma, beta, 1e-5)
    out.append((f"{tag} fwd, fp32 input", rel(y32, yr32), TOL1))
    out.append((f"{tag} stats, fp32 input", rel(s32, str32), 1e-4))
    out += ln_slices(f"{tag} fwd, fp32 input vs fp64", y32, ln_ref64_fwd(x32, gamma, beta, 1e-5)[0], 1)
    out.append((f"{tag} bwd dx + residual grad", rel(hip.layernorm_bwd(x, dy, gamma, str_, add=skip)[0], emu.layernorm_bwd(x, dy, gamma, str_, add=skip)[0]), TOL1))
    out += ln_slices(f"{tag} bwd dx + residual grad vs fp64", hip.layernorm_bwd(x, dy, gamma, st32, add=skip)[0], ln_ref64_bwd(x, dy, gamma, st32, add=skip)[0], 1)
    if case == LN_NEED_STATS_CASE:      # the sampling path: mean_rstd == NULL
        yn, sn = hip.layernorm_fwd(x, gamma, beta, 1e-5, need_stats=False)
        out.append((f"{tag} fwd without statistics: elements differing bitwise from y with them", float(_neq(yn, y) + (sn is not None)), 0.0))
    return out


def check_norms(hip, emu, dev):
    out = []
    for c in GN_CASES:
        out += _check_groupnorm_case(hip, emu, dev, c)
    for i, case in enumerate(LN_CASES):
        out += _check_layernorm_case(hip, emu, dev, i, case)
    return out


# ---- norm_guards: the norm entry points through the raw ABI, poison around every operand ---------------------------------------------
NORM_GUARD_ROWS = 64       # sentinel / NaN rows in front of and behind every operand
# one chunked one-slot case (empty trailing chunks, a ragged last one), one chunked two-slot two-source case, one slab case per NI with a ragged tail
GN_GUARD_CASES = [_gn(2, 260, 320, 0, True), _gn(2, 256, 1280, 1280, True), _gn(2, 60, 640, 0, True), _gn(2, 100, 640, 640, True), _gn(2, 100, 1280, 1280, True)]
GN_GUARD_CASES = [c._replace(seed=1600 + i) for i, c in enumerate(GN_GUARD_CASES)]
LN_GUARD_CASES = [(4101, 640), (300, 1280)]


class _Rows:
    """rows r0 .. r0 + n - 1 of a sentinel buffer, all columns: what _changed_outside() needs to know of an operand"""

    def __init__(self, buf, r0, n):
        self.idx, self.c0, self.d = torch.arange(r0, r0 + n, device=buf.device), 0, buf.shape[1]


class _Guarded:
    """an output [rows][width] (bf16 or fp32) carved out of a sentinel buffer with NORM_GUARD_ROWS sentinel rows on either side, itself sentinel"""

    def __init__(self, rows, width, dtype, dev):
        w16 = width * (2 if dtype == f32 else 1)
        self.buf = _sentinel_buf(rows + 2 * NORM_GUARD_ROWS, w16, dev)
        self.rows, self.dtype = rows, dtype
        self.op = _Rows(self.buf, NORM_GUARD_ROWS, rows)
        self.view = self.buf[NORM_GUARD_ROWS:NORM_GUARD_ROWS + rows].view(dtype)
        self.ptr = self.view.data_ptr()

    def outside(self):
        """sentinel elements changed outside the output"""
        return _changed_outside(self.buf, [self.op])

    def touched(self):
        """16-bit words of the whole buffer, output included, that no longer hold the sentinel (a rejected call must leave 0)"""
        return int((self.buf.view(torch.int16) != SENT16).sum())


def _nan_wrapped(t):
    """a copy of t [rows][width] with NORM_GUARD_ROWS whole rows of NaN in front of and behind it, in one allocation"""
    if t is None:
        return None
    t2 = t.reshape(t.shape[0], -1)
    buf = torch.full((t2.shape[0] + 2 * NORM_GUARD_ROWS, t2.shape[1]), float("nan"), dtype=t.dtype, device=t.device)
    buf[NORM_GUARD_ROWS:NORM_GUARD_ROWS + t2.shape[0]] = t2
    return buf[NORM_GUARD_ROWS:NORM_GUARD_ROWS + t2.shape[0]].view(t.shape)


class _Workspace:
    """exactly nbytes of workspace with 1024 sentinel floats behind it"""

    def __init__(self, nbytes, dev):
        assert nbytes % 4 == 0
        self.n = nbytes // 4
        self.buf = torch.full((self.n + 1024,), SENT32, dtype=torch.int32, device=dev)
        self.ptr, self.bytes = self.buf.data_ptr(), nbytes

    def outside(self):
        return int((self.buf[self.n:] != SENT32).sum())


def _finite_rel(got, ref):
    """relative L2, infinite if any element of got is not finite"""
    return rel(got, ref) if bool(torch.isfinite(got.float()).all()) else float("inf")


def _last_error(lib):
    msg = lib.e4t_last_error()
    return msg.decode() if msg else ""


def _guard_groupnorm(hip, dev, c):
    from e4t.ops import _stream, _ptr
    lib, out = hip.lib, []
    B, HW, C1, C2, G, silu = c.B, c.HW, c.C1, c.C2, c.G, c.silu
    C, n, pl, tag = C1 + C2, c.B * c.HW, norm_plan(c), gn_tag(c) + " guarded"
    x1, x2, gamma, beta, dy, a1, a2 = gn_inputs(c, dev)
    y64, st64 = gn_ref64_fwd(x1, x2, gamma, beta, B, HW, G, c.eps, silu)
    st32 = st64.to(f32)
    d64, ga64, be64 = gn_ref64_bwd(x1, x2, dy, st32, gamma, beta, a1, a2, B, HW, G, silu)
    x1g, x2g, dyg, a1g, a2g = (_nan_wrapped(t) for t in (x1, x2, dy, a1, a2))
    stg = _nan_wrapped(st32.reshape(B * G, 2))
    need = lib.e4t_groupnorm_workspace_bytes(B, HW, C, G, 0)
    chunked = pl["ni"] == 0

    def fwd_rows(form, call, ws_bytes, rejects_short):
        y, st, ws = _Guarded(n, C, bf16, dev), _Guarded(B * G, 2, f32, dev), _Workspace(ws_bytes, dev)
        code = call(y, st, ws, ws.bytes)
        torch.cuda.synchronize()
        rows = [(f"{tag} {form}: return code", float(code), 0.0),
                (f"{tag} {form}: sentinel elements changed around y, mean_rstd, behind the workspace", float(y.outside() + st.outside() + ws.outside()), 0.0),
                (f"{tag} {form}: y (finite, vs fp64)", _finite_rel(y.view, y64), TOL1)]
        rows += gn_stat_rows(f"{tag} {form}: stats", st.view.reshape(B, G, 2), st64)
        if rejects_short:      # one byte class smaller: -22, nothing written
            y, st, ws = _Guarded(n, C, bf16, dev), _Guarded(B * G, 2, f32, dev), _Workspace(ws_bytes, dev)
            code = call(y, st, ws, ws.bytes - 4)
            torch.cuda.synchronize()
            rows.append((f"{tag} {form}, workspace 4 bytes short: return code + 22", float(code + 22), 0.0))
            rows.append((f"{tag} {form}, workspace 4 bytes short: error text missing", float("workspace" not in _last_error(lib)), 0.0))
            rows.append((f"{tag} {form}, workspace 4 bytes short: output / workspace words changed", float(y.touched() + st.touched() + int((ws.buf != SENT32).sum())), 0.0))
        return rows
    out += fwd_rows("e4t_groupnorm_fwd", lambda y, st, ws, nb: lib.e4t_groupnorm_fwd(_ptr(x1g), C1, _ptr(x2g), C2, _ptr(gamma), _ptr(beta), y.ptr, st.ptr, B, HW, G,
                                                                                     float(c.eps), int(silu), ws.ptr, nb, _stream()), need, chunked)
    if HW % 32 == 0 and pl["colstats"]:
        cs1 = _nan_wrapped(_with_colstats(x1.clone())._e4t_colstats.reshape(n // 32, C1 * 2))
        cs2 = _nan_wrapped(_with_colstats(x2.clone())._e4t_colstats.reshape(n // 32, C2 * 2)) if x2 is not None else None
        out += fwd_rows("e4t_groupnorm_fwd_cs", lambda y, st, ws, nb: lib.e4t_groupnorm_fwd_cs(_ptr(x1g), C1, _ptr(cs1), _ptr(x2g), C2, _ptr(cs2), _ptr(gamma), _ptr(beta), y.ptr,
                                                                                               st.ptr, B, HW, G, float(c.eps), int(silu), ws.ptr, nb, _stream()), need, False)
    # the unfused entry points: statistics into a guarded mean_rstd, then apply from it
    st, ws, y = _Guarded(B * G, 2, f32, dev), _Workspace(need, dev), _Guarded(n, C, bf16, dev)
    code = lib.e4t_groupnorm_stats(_ptr(x1g), C1, _ptr(x2g), C2, B, HW, G, float(c.eps), st.ptr, ws.ptr, ws.bytes, _stream())
    code2 = lib.e4t_groupnorm_apply(_ptr(x1g), C1, _ptr(x2g), C2, st.ptr, _ptr(gamma), _ptr(beta), y.ptr, B, HW, G, int(silu), _stream())
    torch.cuda.synchronize()
    out.append((f"{tag} e4t_groupnorm_stats + _apply: return codes", float(abs(code) + abs(code2)), 0.0))
    out.append((f"{tag} e4t_groupnorm_stats + _apply: sentinel elements changed", float(y.outside() + st.outside() + ws.outside()), 0.0))
    out.append((f"{tag} e4t_groupnorm_stats + _apply: y (finite, vs fp64)", _finite_rel(y.view, y64), TOL1))
    out += gn_stat_rows(f"{tag} e4t_groupnorm_stats: stats", st.view.reshape(B, G, 2), st64)
    st, ws = _Guarded(B * G, 2, f32, dev), _Workspace(need, dev)
    code = lib.e4t_groupnorm_stats(_ptr(x1g), C1, _ptr(x2g), C2, B, HW, G, float(c.eps), st.ptr, ws.ptr, ws.bytes - 4, _stream())
    torch.cuda.synchronize()
    out.append((f"{tag} e4t_groupnorm_stats, workspace 4 bytes short: return code + 22", float(code + 22), 0.0))
    out.append((f"{tag} e4t_groupnorm_stats, workspace 4 bytes short: output / workspace words changed", float(st.touched() + int((ws.buf != SENT32).sum())), 0.0))
    # backward: the workspace query + B * G * 8 bytes; with parameter-gradient partials (chunked kernels) and without
    need_b = need + B * G * 8
    for pg in (True, False):
        form = "e4t_groupnorm_bwd" + (" with parameter-gradient partials" if pg else "")

        def call(nb, bufs):
            dx1, dx2, cp, ws = bufs
            return lib.e4t_groupnorm_bwd(_ptr(x1g), C1, _ptr(x2g), C2, _ptr(dyg), stg.data_ptr(), _ptr(gamma), _ptr(beta), _ptr(a1g), _ptr(a2g), dx1.ptr,
                                         dx2.ptr if dx2 else None, cp.ptr if cp else None, B, HW, G, int(silu), ws.ptr, nb, _stream())
        make = lambda: (_Guarded(n, C1, bf16, dev), _Guarded(n, C2, bf16, dev) if C2 else None, _Guarded(B * pl["ch"], C * 2, f32, dev) if pg else None, _Workspace(need_b, dev))
        bufs = make()
        code = call(need_b, bufs)
        torch.cuda.synchronize()
        dx1, dx2, cp, ws = bufs
        out.append((f"{tag} {form}: return code", float(code), 0.0))
        out.append((f"{tag} {form}: sentinel elements changed around dx1, dx2, the partials, behind the workspace", float(sum(b.outside() for b in bufs if b is not None)), 0.0))
        out.append((f"{tag} {form}: dx1 (finite, vs fp64)", _finite_rel(dx1.view, d64[:, :C1]), TOL1))
        if C2:
            out.append((f"{tag} {form}: dx2 (finite, vs fp64)", _finite_rel(dx2.view, d64[:, C1:]), TOL1))
        if pg:
            s = cp.view.reshape(B * pl["ch"], C, 2).sum(0)
            out.append((f"{tag} {form}: dbeta (finite, vs fp64)", _finite_rel(s[:, 0], be64), 1e-3))
            out.append((f"{tag} {form}: dgamma (finite, vs fp64)", _finite_rel(s[:, 1], ga64), 1e-3))
        if pg or chunked:
            bufs = make()
            code = call(need_b - 4, bufs)
            torch.cuda.synchronize()
            out.append((f"{tag} {form}, workspace 4 bytes short: return code + 22", float(code + 22), 0.0))
            out.append((f"{tag} {form}, workspace 4 bytes short: output / workspace words changed",
                        float(sum(b.touched() for b in bufs[:3] if b is not None) + int((bufs[3].buf != SENT32).sum())), 0.0))
    return out


def _guard_layernorm(hip, dev, case):
    from e4t.ops import _stream, _ptr
    lib, out = hip.lib, []
    M, D = case
    tag = f"layernorm {M}x{D} guarded"
    x, gamma, beta, dy, x32, skip = ln_inputs(case, LN_CASES.index(case), dev)
    xg, dyg, x32g, skipg = (_nan_wrapped(t) for t in (x, dy, x32, skip))
    for form, fn, xin, ref in (("e4t_layernorm_fwd", lib.e4t_layernorm_fwd, xg, x), ("e4t_layernorm_fwd_f32", lib.e4t_layernorm_fwd_f32, x32g, x32)):
        y64, st64 = ln_ref64_fwd(ref, gamma, beta, 1e-5)
        y, st = _Guarded(M, D, bf16, dev), _Guarded(M, 2, f32, dev)
        code = fn(_ptr(xin), _ptr(gamma), _ptr(beta), y.ptr, st.ptr, M, D, 1e-5, _stream())
        torch.cuda.synchronize()
        out.append((f"{tag} {form}: return code", float(code), 0.0))
        out.append((f"{tag} {form}: sentinel elements changed around y, mean_rstd", float(y.outside() + st.outside()), 0.0))
        out.append((f"{tag} {form}: y (finite, vs fp64)", _finite_rel(y.view, y64), TOL1))
        out.append((f"{tag} {form}: stats (finite, vs fp64)", _finite_rel(st.view, st64), 1e-4))
    y64, st64 = ln_ref64_fwd(x, gamma, beta, 1e-5)
    stg = _nan_wrapped(st64.to(f32))
    d64, ga64, be64 = ln_ref64_bwd(x, dy, gamma, stg, add=skip)
    dx = _Guarded(M, D, bf16, dev)
    code = lib.e4t_layernorm_bwd(_ptr(xg), _ptr(dyg), _ptr(gamma), _ptr(stg), _ptr(skipg), dx.ptr, M, D, _stream())
    torch.cuda.synchronize()
    out.append((f"{tag} e4t_layernorm_bwd: return code", float(code), 0.0))
    out.append((f"{tag} e4t_layernorm_bwd: sentinel elements changed around dx", float(dx.outside()), 0.0))
    out.append((f"{tag} e4t_layernorm_bwd: dx (finite, vs fp64)", _finite_rel(dx.view, d64), TOL1))
    ns = lib.e4t_colreduce_splits(M)
    dg, db, ws = _Guarded(1, D, f32, dev), _Guarded(1, D, f32, dev), _Workspace(2 * ns * D * 4, dev)
    code = lib.e4t_layernorm_param_grad(_ptr(xg), _ptr(dyg), _ptr(stg), M, D, dg.ptr, db.ptr, 0, ws.ptr, ws.bytes, _stream())
    torch.cuda.synchronize()
    out.append((f"{tag} e4t_layernorm_param_grad: return code", float(code), 0.0))
    out.append((f"{tag} e4t_layernorm_param_grad: sentinel elements changed around dgamma, dbeta, behind the workspace", float(dg.outside() + db.outside() + ws.outside()), 0.0))
    out.append((f"{tag} e4t_layernorm_param_grad: dgamma (finite, vs fp64)", _finite_rel(dg.view.reshape(-1), ga64), 1e-3))
    out.append((f"{tag} e4t_layernorm_param_grad: dbeta (finite, vs fp64)", _finite_rel(db.view.reshape(-1), be64), 1e-3))
    dg, db, ws = _Guarded(1, D, f32, dev), _Guarded(1, D, f32, dev), _Workspace(2 * ns * D * 4, dev)
    code = lib.e4t_layernorm_param_grad(_ptr(xg), _ptr(dyg), _ptr(stg), M, D, dg.ptr, db.ptr, 0, ws.ptr, ws.bytes - 4, _stream())
    torch.cuda.synchronize()
    out.append((f"{tag} e4t_layernorm_param_grad, workspace 4 bytes short: return code + 22", float(code + 22), 0.0))
    out.append((f"{tag} e4t_layernorm_param_grad, workspace 4 bytes short: output / workspace words changed", float(dg.touched() + db.touched() + int((ws.buf != SENT32).sum())), 0.0))
    # e4t_colsum over the same rows as a column slice of a wider matrix (ldx = D + 8), NaN in the columns beside it and the rows around it
    wide = torch.full((M + 2 * NORM_GUARD_ROWS, D + 8), float("nan"), dtype=bf16, device=dev)
    wide[NORM_GUARD_ROWS:NORM_GUARD_ROWS + M, :D] = x
    o, ws = _Guarded(1, D, f32, dev), _Workspace(ns * D * 4, dev)
    code = lib.e4t_colsum(wide[NORM_GUARD_ROWS:].data_ptr(), D + 8, M, D, o.ptr, 0, ws.ptr, ws.bytes, _stream())
    torch.cuda.synchronize()
    out.append((f"{tag} e4t_colsum: return code", float(code), 0.0))
    out.append((f"{tag} e4t_colsum: sentinel elements changed around out, behind the workspace", float(o.outside() + ws.outside()), 0.0))
    out.append((f"{tag} e4t_colsum: out (finite, vs fp64)", _finite_rel(o.view.reshape(-1), x.to(f64).sum(0)), 1e-3))
    return out


def _norm_rejections(hip, dev):
    """calls the library must refuse with -22 (E4T_REQUIRE), an error text, and every output word untouched; none launches a kernel"""
    from e4t.ops import _stream
    lib, out = hip.lib, []
    st = _stream()
    src = torch.zeros(1 << 16, dtype=bf16, device=dev)            # any input: never read
    par = torch.ones(8192, dtype=f32, device=dev)                # gamma / beta / statistics
    X, P = src.data_ptr(), par.data_ptr()

    def outs():
        return _Guarded(64, 512, bf16, dev), _Guarded(64, 512, bf16, dev), _Guarded(64, 2, f32, dev), _Workspace(1 << 16, dev)

    def row(name, fn, word):
        y, y2, s, ws = outs()
        code = fn(y, y2, s, ws)
        torch.cuda.synchronize()
        err = _last_error(lib)
        out.append((f"rejected: {name}: return code + 22", float(code + 22), 0.0))
        out.append((f"rejected: {name}: error text names {word!r} (got {err!r})", float(word not in err), 0.0))
        out.append((f"rejected: {name}: output / workspace words changed", float(y.touched() + y2.touched() + s.touched() + int((ws.buf != SENT32).sum())), 0.0))

    def fwd(C1, C2, G, x2=None, B=1, HW=8):
        return lambda y, y2, s, ws: lib.e4t_groupnorm_fwd(X, C1, x2, C2, P, P, y.ptr, s.ptr, B, HW, G, 1e-5, 1, ws.ptr, ws.bytes, st)

    def bwd(C1, C2, G, x2=None, add2=None, dx2=False):
        return lambda y, y2, s, ws: lib.e4t_groupnorm_bwd(X, C1, x2, C2, X, P, P, P, None, add2, y.ptr, y2.ptr if dx2 else None, None, 1, 8, G, 1, ws.ptr, ws.bytes, st)
    row("groupnorm C1 % 8 != 0", fwd(36, 0, 4), "groupnorm")
    row("groupnorm C % G != 0", fwd(320, 0, 33), "groupnorm")
    row("groupnorm C > 4096", fwd(4104, 0, 8), "too large")
    row("groupnorm G > 256", fwd(1024, 0, 512), "too large")
    row("groupnorm x2 given with C2 == 0", fwd(64, 0, 32, x2=X), "x2/C2")
    row("groupnorm C2 > 0 without x2", fwd(64, 64, 32), "x2/C2")
    row("groupnorm_bwd dx2 missing with C2 > 0", bwd(64, 64, 32, x2=X), "groupnorm_bwd")
    row("groupnorm_bwd add2 given with C2 == 0", bwd(64, 0, 32, add2=X, dx2=False), "groupnorm_bwd")
    cs = lambda C1, B, HW: lambda y, y2, s, ws: lib.e4t_groupnorm_fwd_cs(X, C1, P, None, 0, None, P, P, y.ptr, s.ptr, B, HW, 32, 1e-5, 1, ws.ptr, ws.bytes, st)
    row("groupnorm_fwd_cs HW % 32 != 0", cs(64, 1, 40), "groupnorm_fwd_cs")
    row("groupnorm_fwd_cs B48 HW1024 (32 blocks, 21 chunks)", cs(64, 48, 1024), "do not split")
    ln = lambda D, fn=lib.e4t_layernorm_fwd, x=X: lambda y, y2, s, ws: fn(x, P, P, y.ptr, s.ptr, 4, D, 1e-5, st)
    row("layernorm D % 8 != 0", ln(36), "layernorm")
    row("layernorm D = 1544", ln(1544), "layernorm")
    row("layernorm_fwd_f32 x offset by 8 bytes", ln(64, lib.e4t_layernorm_fwd_f32, P + 8), "16-byte aligned")
    row("layernorm_bwd D = 1544", lambda y, y2, s, ws: lib.e4t_layernorm_bwd(X, X, P, P, None, y.ptr, 4, 1544, st), "layernorm")
    row("colsum ldx % 8 != 0", lambda y, y2, s, ws: lib.e4t_colsum(X, 68, 16, 64, s.ptr, 0, ws.ptr, ws.bytes, st), "colsum")
    return out


def check_norm_guards(hip, emu, dev):
    """Every norm entry point through the C ABI with each output between sentinel rows, the workspace exactly the required size with sentinels behind
    it (4 bytes less: -22, nothing written), every input between whole rows of NaN (an out-of-range read that reaches a sum, or a masked lane that
    multiplies by 0, turns the result non-finite: the rows are `finite and within tolerance of fp64`); then the argument checks (-22, error text,
    outputs untouched)."""
    out = []
    for c in GN_GUARD_CASES:
        out += _guard_groupnorm(hip, dev, c)
    for case in LN_GUARD_CASES:
        out += _guard_layernorm(hip, dev, case)
    return out + _norm_rejections(hip, dev)


def check_streaming(hip, emu, dev):
    out = []
    g = gen(179, dev)
    for M, Cn in [(37, 64), (5000, 320), (65536, 320), (1232, 2560), (300, 8)]:
        xs = rnd(g, M, Cn + 8, dev=dev)[:, :Cn]                      # strided view
        out.append((f"colsum {M}x{Cn}", rel(hip.colsum(xs), emu.colsum(xs)), 1e-3))
    for B, Cn, HW, cfg, nhwc, noise in [(2, 4, 4096, True, True, False), (3, 4, 100, True, False, True), (1, 4, 9216, False, True, True), (2, 4, 37, False, False, False)]:
        pred = torch.randn(((2 if cfg else 1) * B * Cn * HW,), generator=g, device=dev)
        x = torch.randn((B, Cn, HW), generator=g, device=dev)
        nz = torch.randn((B, Cn, HW), generator=g, device=dev) if noise else None
        coef = torch.tensor([7.5, 1.0123, -0.0456, 0.3], dtype=f32, device=dev)
        got = hip.guided_step(pred, x, coef, noise=nz, cfg=cfg, pred_nhwc=nhwc)
        out.append((f"guided_step B{B} HW{HW} cfg={cfg} nhwc={nhwc}", rel(got, emu.guided_step(pred, x, coef, noise=nz, cfg=cfg, pred_nhwc=nhwc)), 1e-6))
    x2 = x.clone()
    hip.guided_step(pred, x2, coef, cfg=False, pred_nhwc=False, out=x2)          # in place on the sample, as the pipeline uses it
    out.append(("guided_step in place", rel(x2, emu.guided_step(pred, x, coef, cfg=False)), 1e-6))
    acc = torch.ones(320, dtype=f32, device=dev)
    xs = rnd(g, 700, 320, dev=dev)
    hip.colsum(xs, out=acc, accumulate=True)
    out.append(("colsum accumulate", rel(acc, 1.0 + emu.colsum(xs)), 1e-3))
    g = gen(180, dev)
    u = rnd(g, 300, 2 * 640, dev=dev)
    dh = rnd(g, 300, 640, dev=dev)
    out.append(("geglu fwd", rel(hip.geglu_fwd(u), emu.geglu_fwd(u)), TOL1))
    out.append(("geglu bwd", rel(hip.geglu_bwd(u, dh), emu.geglu_bwd(u, dh)), TOL1))
    x, dy = rnd(g, 64, 1280, dev=dev), rnd(g, 64, 1280, dev=dev)
    for op in range(8):
        out.append((f"unary op{op}", rel(hip.unary(x, op, dy if op & 1 else None), emu.unary(x, op, dy if op & 1 else None)), TOL1))
    out.append(("add", rel(hip.add(x, dy), emu.add(x, dy)), TOL1))
    t = rnd(g, 130, 72, dev=dev)
    out.append(("transpose", rel(hip.transpose(t), emu.transpose(t)), 0.0))
    out.append(("transpose padded + strided in", rel(hip.transpose(u[:, 8:80], pad_to=320), emu.transpose(u[:, 8:80], pad_to=320)), 0.0))
    xx = rnd(g, 2 * 16 * 16, 64, dev=dev)
    out.append(("sumpool2", rel(hip.sumpool2(xx, 2, 8, 8), emu.sumpool2(xx, 2, 8, 8)), TOL1))
    o1 = torch.zeros(2, 200, dtype=f32, device=dev); o2 = torch.zeros_like(o1)
    hip.spatial_mean(xx, 2, 256, o1, 100); emu.spatial_mean(xx, 2, 256, o2, 100)
    out.append(("spatial_mean", rel(o1, o2), TOLF))
    gg = rnd(g, 2, 200, dtype=f32, dev=dev)
    out.append(("spatial_mean_bwd", rel(hip.spatial_mean_bwd(gg, xx, 2, 256, 64, 100), emu.spatial_mean_bwd(gg, xx, 2, 256, 64, 100)), TOL1))
    ts = torch.tensor([0, 1, 17, 500, 999], device=dev)
    out.append(("timestep_embedding", rel(hip.timestep_embedding(ts, 320), emu.timestep_embedding(ts, 320)), TOL1))
    px = torch.rand(2, 3, 512, 512, generator=g, device=dev) * 2 - 1
    out.append(("clip_preprocess 512->224 p14", rel(hip.clip_preprocess(px, 224, 14, 640), emu.clip_preprocess(px, 224, 14, 640)), TOL1))
    px = torch.rand(2, 3, 64, 64, generator=g, device=dev) * 2 - 1
    out.append(("clip_preprocess 64->28 p14", rel(hip.clip_preprocess(px, 28, 14, 640), emu.clip_preprocess(px, 28, 14, 640)), TOL1))
    n = 100003
    p = rnd(g, n, dtype=f32, dev=dev); gr = rnd(g, n, dtype=f32, dev=dev); m = rnd(g, n, dtype=f32, dev=dev) * 0.1; v = rnd(g, n, dtype=f32, dev=dev).abs() * 0.01
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    hip.adamw(p, gr, m, v, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 3, 0.5)
    emu.adamw(p2, gr, m2, v2, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 3, 0.5)
    out += [("adamw p", rel(p, p2), TOLF), ("adamw m", rel(m, m2), TOLF), ("adamw v", rel(v, v2), TOLF)]
    out.append(("sumsq", rel(hip.sumsq(gr), emu.sumsq(gr)), 1e-4))
    # AdamW of a weight stack under the never-materialised rank-K gradient G^T Z_i (round 6): K = 16 (one k chunk), 40 (three, ragged),
    # rows not a multiple of the row block, columns that are / are not a multiple of the 64-lane quad count, device-resident scalars
    for i, (n, rows, cols, K) in enumerate(((5, 64, 128, 16), (3, 100, 320, 40), (2, 1280, 1280, 16), (4, 24, 72, 3))):
        gg = gen(470 + i, dev)
        P = rnd(gg, n, rows, cols, dtype=f32, dev=dev)
        M = rnd(gg, n, rows, cols, dtype=f32, dev=dev) * 0.1
        Vv = rnd(gg, n, rows, cols, dtype=f32, dev=dev).abs() * 0.01
        Gf, Zf = rnd(gg, K, rows, dev=dev), rnd(gg, K, n * cols, dev=dev)
        P2, M2, V2 = P.clone(), M.clone(), Vv.clone()
        hyper = torch.tensor([2e-3, 1 - 0.9 ** 4, (1 - 0.999 ** 4) ** 0.5, 0.25], dtype=f32, device=dev) if i == 1 else None
        hip.adamw_rank(P, M, Vv, Gf, Zf, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 3, 0.5, hyper=hyper)
        emu.adamw_rank(P2, M2, V2, Gf, Zf, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 3, 0.5, hyper=hyper)
        tag = f"adamw_rank n{n} {rows}x{cols} K{K}" + (" hyper" if hyper is not None else "")
        out += [(tag + " p", rel(P, P2), TOLF), (tag + " m", rel(M, M2), TOLF), (tag + " v", rel(Vv, V2), TOLF)]
    for mode, (Bn, Hin, Hout) in ((1, (2, 12, 12)), (2, (3, 9, 5)), (3, (2, 6, 12))):
        xi = rnd(g, Bn * Hin * Hin, 72, dev=dev)
        out.append((f"im2col_T mode{mode}", rel(hip.im2col_T(xi, Bn, Hin, Hin, Hout, Hout, mode), emu.im2col_T(xi, Bn, Hin, Hin, Hout, Hout, mode)), 0.0))
        out.append((f"im2col mode{mode}", rel(hip.im2col(xi, Bn, Hin, Hin, Hout, Hout, mode), emu.im2col(xi, Bn, Hin, Hin, Hout, Hout, mode)), 0.0))
    sc = rnd(g, 3, 100, 4096, scale=2.0, dev=dev)
    out.append(("softmax_rows 4096", rel(hip.softmax_rows_(sc.clone()), emu.softmax_rows_(sc.clone())), TOL1))
    sc = rnd(g, 77, 64, scale=3.0, dev=dev)
    out.append(("softmax_rows 64", rel(hip.softmax_rows_(sc.clone()), emu.softmax_rows_(sc.clone())), TOL1))
    px = torch.rand(2, 3, 40, 24, generator=g, device=dev) * 2 - 1
    out.append(("im2col3_rgb", rel(hip.im2col3_rgb(px), emu.im2col3_rgb(px)), 0.0))
    big = rnd(g, 2 * 4096, 320, dev=dev)
    o1 = torch.zeros(2, 320, dtype=f32, device=dev); o2 = torch.zeros_like(o1)
    hip.spatial_mean(big, 2, 4096, o1, 0); emu.spatial_mean(big, 2, 4096, o2, 0)
    out.append(("spatial_mean 4096x320", rel(o1, o2), TOLF * 5))
    return out + _check_grid_stride(hip, emu, dev)


STRIDE_ITEMS, STRIDE_TAIL = 2048 * 256 + 333, 333      # = 107 * 4903 work items: a full grid of 2048 blocks, then a ragged second trip of 333 items


def _check_grid_stride(hip, emu, dev):
    """Every kernel of elementwise.hip, optim.hip and objective.hip launched through grid_for() caps its grid (2048 blocks of 256; 4096 for the weight relayout and AdamW) and
    walks the rest with a grid-stride loop: one case per kernel whose work is one full grid plus a ragged second trip, with the existing tolerance,
    and the items of the second trip once more on their own (333 of 524621 items move a whole-tensor relative L2 by 2.5 % when they are garbage;
    a subtler error in them would drown)."""
    out = []
    g = gen(181, dev)
    N, T = STRIDE_ITEMS, STRIDE_TAIL

    def rows(name, got, ref, tol, tail):
        """tail: the output elements (flat, trailing) the second trip wrote"""
        out.append((f"{name}, {N} items", rel(got, ref), tol))
        out.append((f"{name}, {N} items: the {T} items of the second trip", rel(got.reshape(-1)[-tail:], ref.reshape(-1)[-tail:]), tol))
    x, dy = rnd(g, N, 8, dev=dev), rnd(g, N, 8, dev=dev)
    for op in (0, 1):      # silu forward / backward (one forward, one backward op: the loop is the op's own)
        rows(f"unary op{op}", hip.unary(x, op, dy if op & 1 else None), emu.unary(x, op, dy if op & 1 else None), TOL1, T * 8)
    rows("add", hip.add(x, dy), emu.add(x, dy), TOL1, T * 8)
    u = rnd(g, N, 16, dev=dev)      # H = 8: one item per row
    rows("geglu fwd", hip.geglu_fwd(u), emu.geglu_fwd(u), TOL1, T * 8)
    rows("geglu bwd", hip.geglu_bwd(u, dy), emu.geglu_bwd(u, dy), TOL1, T * 16)
    xx = rnd(g, 2 * 107 * 2 * 4903, 8, dev=dev)      # one image of 214 x 9806 pixels, 8 channels -> 107 x 4903
    rows("sumpool2", hip.sumpool2(xx, 1, 107, 4903), emu.sumpool2(xx, 1, 107, 4903), TOL1, T * 8)
    del xx
    gg = rnd(g, 107, 16, dtype=f32, dev=dev)
    rows("spatial_mean_bwd", hip.spatial_mean_bwd(gg, x, 107, 4903, 8, 8), emu.spatial_mean_bwd(gg, x, 107, 4903, 8, 8), TOL1, T * 8)
    px = torch.rand(4, 3, 512, 512, generator=g, device=dev) * 2 - 1      # 4 * 3 * 224 * 224 = 602112 items: the second trip holds the last 77824
    got, ref = hip.clip_preprocess(px, 224, 14, 640), emu.clip_preprocess(px, 224, 14, 640)
    out.append(("clip_preprocess B4 512->224 p14 (602112 items)", rel(got, ref), TOL1))
    out.append(("clip_preprocess B4 512->224 p14: the last image (items 451584 up; the second trip starts at 524288)", rel(got[3 * 256:], ref[3 * 256:]), TOL1))
    w4 = rnd(g, 320, 320, 3, 3, scale=0.05, dtype=f32, dev=dev)      # 2 * 320 * 9 * 320 = 1843200 items against a grid of 4096 blocks
    (wf, wd), (wf2, wd2) = hip.conv_weight_prepare(w4), emu.conv_weight_prepare(w4)
    out.append(("conv_weight_prepare 320->320 fwd layout (1843200 items, grid cap 4096)", rel(wf, wf2), 0.0))
    out.append(("conv_weight_prepare 320->320 dgrad layout", rel(wd, wd2), 0.0))
    out.append(("conv_weight_prepare 320->320 dgrad layout: the last 794624 items (the second trip)", rel(wd.reshape(-1)[-794624:], wd2.reshape(-1)[-794624:]), 0.0))
    n = 4096 * 1024 + 4 * T + 1      # AdamW: four elements per thread, grid cap 4096; the last thread holds one element
    p = rnd(g, n, dtype=f32, dev=dev); gr = rnd(g, n, dtype=f32, dev=dev); m = rnd(g, n, dtype=f32, dev=dev) * 0.1; v = rnd(g, n, dtype=f32, dev=dev).abs() * 0.01
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    hip.adamw(p, gr, m, v, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 3, 0.5)
    emu.adamw(p2, gr, m2, v2, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 3, 0.5)
    for nm, a, b in (("p", p, p2), ("m", m, m2), ("v", v, v2)):
        out.append((f"adamw {nm}, {n} elements", rel(a, b), TOLF))
        out.append((f"adamw {nm}, {n} elements: the {4 * T + 1} elements of the second trip", rel(a[-(4 * T + 1):], b[-(4 * T + 1):]), TOLF))
    del p, gr, m, v, p2, m2, v2
    wdm = rnd(g, N, dtype=f32, dev=dev)      # masked_mse_bwd: dpred = g * 2 / den * wd, den = stats[1]
    stats, up = torch.tensor([0.25, 37.0, 0.0, 0.0], dtype=f32, device=dev), torch.tensor([0.7], dtype=f32, device=dev)
    rows("masked_mse_bwd", hip.masked_mse_bwd(wdm, stats, up), (wdm.double() * (0.7 * 2.0 / 37.0)).float(), TOLF, T)
    return out


def make_wo_entry(g, row, col, dev, ops_mod, with_gW=False, ld_pad=0):
    WOEntry = ops_mod.WOEntry
    s = lambda *sh, sc=1.0: rnd(g, *sh, scale=sc, dtype=f32, dev=dev)
    params = dict(v=torch.full((1,), 0.8, device=dev), w1=s(row, 1, sc=0.5), b1=s(row, sc=0.5), w2=s(col, 1, sc=0.5), b2=s(col, sc=0.5),
                  wc=s(row, row, sc=row ** -0.5), bc=s(row, sc=0.1), wr=s(col, col, sc=col ** -0.5), br=s(col, sc=0.1))
    grads = {"g_" + k: torch.zeros_like(v) for k, v in params.items()}
    W = s(col, row, sc=row ** -0.5)
    weff = torch.zeros(col, row + ld_pad, dtype=bf16, device=dev)
    weffT = torch.zeros(row, col + ld_pad, dtype=bf16, device=dev)
    dweff = s(col, row + ld_pad)
    return WOEntry(row=row, col=col, W=W, params=params, weff=weff, weffT=weffT, dweff=dweff, grads=grads,
                   g_W=torch.zeros_like(W) if with_gW else None)


def check_wo(hip, emu, dev, ops_mod):
    import copy
    out = []
    g = gen(200, dev)
    dims = [(64, 64), (96, 160), (320, 320), (768, 320), (1280, 1280)]
    ents = [make_wo_entry(g, r, c, dev, ops_mod, with_gW=(i == 1), ld_pad=(8 if i == 2 else 0)) for i, (r, c) in enumerate(dims)]
    ents2 = copy.deepcopy(ents)
    th, te = ops_mod.WOTable(ents), ops_mod.WOTable(ents2)
    hip.wo_forward(th); emu.wo_forward(te)
    for (r, c), a, b in zip(dims, ents, ents2):
        out.append((f"wo fwd W_eff {r}->{c}", rel(a.weff, b.weff), TOL1))
        out.append((f"wo fwd W_eff^T {r}->{c}", rel(a.weffT, b.weffT), TOL1))
    hip.wo_backward(th, False); emu.wo_backward(te, False)
    for (r, c), a, b in zip(dims, ents, ents2):
        for k in a.grads:
            out.append((f"wo bwd {k} {r}->{c}", rel(a.grads[k], b.grads[k]), 2e-4))
        if a.g_W is not None:
            out.append((f"wo bwd g_W {r}->{c}", rel(a.g_W, b.g_W), 2e-4))
    hip.wo_backward(th, True); emu.wo_backward(te, True)
    out.append(("wo bwd accumulate g_wc", rel(ents[2].grads["g_wc"], ents2[2].grads["g_wc"]), 2e-4))
    # plain weights (cast + transpose only)
    W = rnd(g, 200, 136, dtype=f32, dev=dev)
    e1 = ops_mod.WOEntry(row=136, col=200, W=W, weff=torch.zeros(200, 136, dtype=bf16, device=dev), weffT=torch.zeros(136, 200, dtype=bf16, device=dev))
    e2 = copy.deepcopy(e1)
    hip.weight_prepare(ops_mod.WOTable([e1])); emu.weight_prepare(ops_mod.WOTable([e2]))
    out.append(("weight_prepare cast", rel(e1.weff, e2.weff), 0.0))
    out.append(("weight_prepare transpose", rel(e1.weffT, e2.weffT), 0.0))
    return out


# ---- wo_forms, wo_guards: the weight-offset kernels against the fp64 DEFINITION (the two-Linear module of oracle/e4t_oracle.py) ------------
WO_F32, WO_OFF = 1, 2      # E4T_WO_STORE_F32, E4T_WO_OFFSETS_ONLY (include/e4t_hip.h)
WO_PNAMES = ("v", "w1", "b1", "w2", "b2", "wc", "bc", "wr", "br")
WO_VNAMES = ("a", "b", "s", "vx", "vy", "da", "db", "ds")      # the vecs scratch, in its order (wo.hip: V_a .. V_ds)
# Tolerance per class of row = 2 x the worst row of the CPU model of the kernels' fp32 arithmetic (tests/test_wo_slices_cpu.py: lane-strided chains
# of stride 256, wave tree, 32-chunk partials in chunk order, multiply-adds fused where the compiled kernels fuse them, bf16 / fp32 stores) against
# wo_ref64, over every row of every case of WO_CASES and WO_GUARD_CASES and the inputs of tests/test_wo_gpu.py; measured there (it prints them):
# bf16 matrix 2.17e-3 (the 16 elements of the 4->4 weff), fp32 matrix 4.3e-7 (a 32x256 block of a g_wc), fp32 vector 1.35e-6 (a last quad of g_w2
# whose four values cancel to a fifth of the vector's), scalar g_v 7.7e-8 of the sum of its absolute terms.  The former bound on every gradient was
# 2e-4 on the whole tensor; no fp32 class gets more than 2.7e-6 now, and the bf16 rows stay under TOL1.
WO_TOL = {"bf16": 4.4e-3, "f32": 8.7e-7, "vec": 2.7e-6, "scalar": 1.6e-7}
WO_TOL["outer"] = WO_TOL["f32"]
WoCase = namedtuple("WoCase", "name groups mode weff weffT seed")      # groups: ((row, (col, ...)), ...) as WOBank._build lays a fused projection out;
#                                                                        weff / weffT False: that output pointer is NULL


def _wo1(row, col, mode=0, weff=True, weffT=True, name=None):
    return WoCase(name or f"{row}->{col}", ((row, (col,)),), mode, weff, weffT, 0)


WO_TAIL_DIMS = [(4, 4), (36, 100), (100, 36), (260, 68), (68, 260), (516, 1028)]      # the minimum; across 32 and 64; 4 past 256; 4 past 512 and 1024
WO_REAL_DIMS = [(640, 640), (768, 640), (768, 1280)]
WO_MIXED = WoCase("mixed table", ((4, (4,)), (768, (320,)), (320, (1280,)), (260, (68,))), 0, True, True, 0)      # max_row, max_col from different entries
WO_RAGGED = WoCase("ragged group 36->(100|36|4)", ((36, (100, 36, 4)),), 0, True, True, 0)
WO_PRODUCT = [WoCase("q|k|v 320->3x320", ((320, (320, 320, 320)),), 0, True, True, 0),
              WoCase("k|v 768->2x640 + ragged 36->(100|36|4)", ((768, (640, 640)), (36, (100, 36, 4))), 0, True, True, 0)]
WO_MODES = [("offsets only, fp32, weffT NULL (WeightOffsets.forward())", WO_OFF | WO_F32, True, False), ("fp32 weff, bf16 weffT", WO_F32, True, True),
            ("offsets only, bf16", WO_OFF, True, True), ("weff NULL", 0, False, True)]
WO_MODE_DIMS = [(36, 100), (320, 320)]
WO_CASES = ([_wo1(r, c) for r, c in WO_TAIL_DIMS + WO_REAL_DIMS] + [WO_MIXED] + WO_PRODUCT
            + [_wo1(r, c, m, we, wt, f"{r}->{c} {nm}") for r, c in WO_MODE_DIMS for nm, m, we, wt in WO_MODES])
WO_CASES = [c._replace(seed=2100 + i) for i, c in enumerate(WO_CASES)]
WO_GUARD_CASES = [c._replace(seed=2200 + i) for i, c in enumerate([_wo1(36, 100), _wo1(260, 68), WO_RAGGED])]


class WoValues:
    """the inputs of one entry as dense tensors: what wo_ref64 and the CPU model read (row, col, W, params, dweff, mode as a WOEntry has them)"""

    def __init__(self, row, col, W, params, dweff, mode):
        self.row, self.col, self.W, self.params, self.dweff, self.mode = row, col, W, params, dweff, mode

    def to(self, dev):
        return WoValues(self.row, self.col, self.W.to(dev), {k: t.to(dev) for k, t in self.params.items()}, self.dweff.to(dev), self.mode)


def wo_values(case, dev):
    """one WoValues per entry of the case, in table order: make_wo_entry's distributions (offsets of mean magnitude ~0.3).  With OFFSETS_ONLY W is all
    ones, as WeightOffsets.forward() passes it: the backward forms G = dweff o W whatever the mode.  Drawn on the CPU and copied: the GPU rows and
    the CPU model that sets their tolerances (tests/test_wo_slices_cpu.py) see the same numbers."""
    g = gen(case.seed, "cpu")
    s = lambda *sh, sc=1.0: rnd(g, *sh, scale=sc, dtype=f32, dev="cpu").to(dev)
    out = []
    for row, cols in case.groups:
        for col in cols:
            params = dict(v=torch.full((1,), 0.8, device=dev), w1=s(row, 1, sc=0.5), b1=s(row, sc=0.5), w2=s(col, 1, sc=0.5), b2=s(col, sc=0.5),
                          wc=s(row, row, sc=row ** -0.5), bc=s(row, sc=0.1), wr=s(col, col, sc=col ** -0.5), br=s(col, sc=0.1))
            W = torch.ones(col, row, dtype=f32, device=dev) if case.mode & WO_OFF else s(col, row, sc=row ** -0.5)
            out.append(WoValues(row, col, W, params, s(col, row), case.mode))
    return out



# the Python paths (tests/test_wo_gpu.py): modules with torch's default initialisation, as the trainer meets them; the CPU model holds these too
WO_MODULE_DIMS = [(48, 80), (36, 100)]
WO_BANK_GROUPS = ((36, (36, 36, 36)), (100, (36, 36)))      # a self-attention q|k|v and a cross-attention k|v at tiny dims


def _wo_module_params(m):
    return {k: t.detach() for k, t in dict(v=m.v, w1=m.linear1.weight, b1=m.linear1.bias, w2=m.linear2.weight, b2=m.linear2.bias, wc=m.linear_column.weight,
                                           bc=m.linear_column.bias, wr=m.linear_row.weight, br=m.linear_row.bias).items()}


def wo_module_values(row, col, seed=5):
    """-> (state dict of a default-initialised oracle WeightOffsets(row, col), its WoValues with W = ones and a random upstream gradient in the
    mode of WeightOffsets.forward()); on the CPU, the global generator left alone"""
    import e4t_oracle as orc
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        m = orc.WeightOffsets(row, col)
        g = torch.randn(col, row)
    return m.state_dict(), WoValues(row, col, torch.ones(col, row), _wo_module_params(m), g, WO_OFF | WO_F32)


def wo_bank_values(seed=11):
    """per entry of WO_BANK_GROUPS, in table order: (state dict of its default-initialised WeightOffsets, [WoValues of step 1, of step 2]): the
    projection weight is a default nn.Linear's, each step has a dW_eff of its own"""
    import e4t_oracle as orc
    out = []
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        for row, cols in WO_BANK_GROUPS:
            for col in cols:
                m, W = orc.WeightOffsets(row, col), torch.nn.Linear(row, col, bias=False).weight.detach()
                out.append((m.state_dict(), [WoValues(row, col, W, _wo_module_params(m), torch.randn(col, row), 0) for _ in range(2)]))
    return out


def wo_ref64(e):
    """The definition in fp64: the entry's nine parameters loaded into the literal two-Linear WeightOffsets of oracle/e4t_oracle.py, W_eff = W o (1 + m())
    (m() itself with OFFSETS_ONLY), dweff[:, :row] backpropagated with autograd.  -> dict: weff [col][row]; g_<parameter> (the parameter's shape);
    g_W (None with OFFSETS_ONLY); g_v_terms = sum |dvx w1| + sum |dvy w2| (what g_v is measured against: it cancels); vecs = {a, b, s, vx, vy, da,
    db, ds} from their formulas in the header of wo.hip — the only use of the closed form on this side, for the rows that localise a failure."""
    import e4t_oracle as orc
    dev = e.W.device
    m = orc.WeightOffsets(e.row, e.col).double().to(dev)
    plist = [m.v, m.linear1.weight, m.linear1.bias, m.linear2.weight, m.linear2.bias, m.linear_column.weight, m.linear_column.bias, m.linear_row.weight, m.linear_row.bias]
    with torch.no_grad():
        for p, k in zip(plist, WO_PNAMES):
            p.copy_(e.params[k].to(f64).reshape(p.shape))
    W = e.W.to(f64).clone().requires_grad_(True)
    off = m()
    only = bool(e.mode & WO_OFF)
    weff = off if only else W * (1.0 + off)
    grads = torch.autograd.grad(weff, plist + ([] if only else [W]), e.dweff[:, :e.row].to(f64))
    ref = {"weff": weff.detach(), "g_W": None if only else grads[-1]}
    for k, g in zip(WO_PNAMES, grads):
        ref["g_" + k] = g.reshape(e.params[k].shape)
    p = {k: t.to(f64) for k, t in e.params.items()}
    vx, vy = p["w1"][:, 0] * p["v"] + p["b1"], p["w2"][:, 0] * p["v"] + p["b2"]
    a, b, s = p["wc"] @ vx, p["wr"] @ vy, p["wr"].sum(1)
    G = e.dweff[:, :e.row].to(f64) * e.W.to(f64)
    da, db, ds = G.t() @ b, G @ a, G @ p["bc"]
    ref["vecs"] = dict(a=a, b=b, s=s, vx=vx, vy=vy, da=da, db=db, ds=ds)
    ref["g_v_terms"] = float(((p["wc"].t() @ da) * p["w1"][:, 0]).abs().sum() + ((p["wr"].t() @ db) * p["w2"][:, 0]).abs().sum())
    return ref


def wo_slices(tag, got, ref, kind, norm=None, tol=None):
    """Rows along the kernels' own decomposition (ref float64); each is the relative L2 of its slice.
    kind 'bf16' / 'f32': a matrix in 64x64 tiles (wo_apply_kernel; g_W shares the grid of its rows): whole, the first tile, the last tile row and the
    last tile column (the remainders col % 64 and row % 64 where there are any), their corner, the worst tile.
    kind 'outer': blocks of 32 rows x 256 columns (wo_bwd_outer_kernel): whole, the last 32-chunk, the last 256-block, the worst block.
    kind 'vec': blocks of 256: whole, the last block, the last quad, the worst block.
    kind 'scalar': |got - ref| / norm (g_v cancels: norm is the fp64 sum of the absolute terms, ref['g_v_terms'])."""
    tol = WO_TOL[kind] if tol is None else tol
    g, r = got.to(f64), ref.to(f64)
    fin = lambda e: float(torch.nan_to_num(torch.as_tensor(e, dtype=f64), nan=float("inf")))
    if kind == "scalar":
        return [(f"{tag}: |error| / sum of |terms|", fin((g - r).abs().sum() / norm), tol)]
    out, seen = [], set()
    if kind == "vec":
        g, r = g.reshape(1, -1), r.reshape(1, -1)
        bh, bw = 1, 256
    else:
        bh, bw = (32, 256) if kind == "outer" else (64, 64)
    R, C = r.shape
    d2, r2 = (g - r) ** 2, r * r

    def row(label, rs, cs):
        key = (rs.indices(R), cs.indices(C))
        if key not in seen and d2[rs, cs].numel():
            seen.add(key)
            out.append((f"{tag}: {label}", fin((d2[rs, cs].sum() / (r2[rs, cs].sum() + 1e-300)).sqrt()), tol))
    A = slice(None)
    r_last, c_last = (R - 1) // bh * bh, (C - 1) // bw * bw
    row("whole", A, A)
    if kind == "vec":
        row(f"elements {c_last}-{C - 1} (the last block of 256)", A, slice(c_last, C))
        row(f"elements {C - 4}-{C - 1} (the last quad)", A, slice(C - 4, C))
    elif kind == "outer":
        row(f"rows {r_last}-{R - 1} (the last 32-chunk)", slice(r_last, R), A)
        row(f"columns {c_last}-{C - 1} (the last 256-block)", A, slice(c_last, C))
    else:
        row("the first tile", slice(0, bh), slice(0, bw))
        row(f"rows {r_last}-{R - 1} (the last tile row)", slice(r_last, R), A)
        row(f"columns {c_last}-{C - 1} (the last tile column)", A, slice(c_last, C))
        row("the corner tile (last tile row x last tile column)", slice(r_last, R), slice(c_last, C))
    pad = lambda t: torch.nn.functional.pad(t, (0, -C % bw, 0, -R % bh)).reshape(-(-R // bh), bh, -(-C // bw), bw).sum(dim=(1, 3))
    e = (pad(d2) / (pad(r2) + 1e-300)).sqrt()
    e = torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)
    out.append((f"{tag}: worst {'block of 256' if kind == 'vec' else f'{bh}x{bw} block'} of {e.numel()}", float(e.max()), tol))
    return out


def wo_value_rows(tag, got, ref, mode=0):
    """every value row of one entry: got holds any of weff, weffT, the nine g_<parameter>, g_W and vecs (a dict); all against wo_ref64"""
    out = []
    if got.get("weff") is not None:
        out += wo_slices(f"{tag} weff", got["weff"], ref["weff"], "f32" if mode & WO_F32 else "bf16")
    if got.get("weffT") is not None:
        out += wo_slices(f"{tag} weffT", got["weffT"], ref["weff"].t(), "bf16")
    for k in WO_PNAMES:
        if got.get("g_" + k) is None:
            continue
        if k == "v":
            out += wo_slices(f"{tag} g_v", got["g_v"], ref["g_v"], "scalar", norm=ref["g_v_terms"])
        else:
            out += wo_slices(f"{tag} g_{k}", got["g_" + k], ref["g_" + k], "outer" if k in ("wc", "wr") else "vec")
    if got.get("g_W") is not None:
        out += wo_slices(f"{tag} g_W", got["g_W"], ref["g_W"], "f32")
    for k, t in (got.get("vecs") or {}).items():
        out += wo_slices(f"{tag} vecs.{k}", t, ref["vecs"][k], "vec")
    return out


def wo_transpose_row(tag, weff, weffT):
    """weffT is weff (rounded to bf16 where it is stored in fp32) transposed, bit for bit: both come from one f2bf / pack4 of the same fp32 value"""
    return [(f"{tag}: elements of weffT that are not weff{'.to(bf16)' if weff.dtype == f32 else ''} transposed", float(_neq(weffT.contiguous(), weff.to(bf16).t().contiguous())), 0.0)]


def wo_accumulate_rows(tag, acc, g0, g):
    """accumulate = 1 onto g0 gives g0 + g in fp32, bit for bit (g: the accumulate = 0 result of the same inputs): the nine gradients, and g_W"""
    keys = [k for k in acc if acc[k] is not None]
    out = [(f"{tag} accumulate = 1: elements of the nine gradients that are not G0 + g", float(sum(_neq(acc[k], g0[k] + g[k]) for k in keys if k != "g_W")), 0.0)]
    if "g_W" in keys:
        out.append((f"{tag} accumulate = 1: elements of g_W that are not G0 + g", float(_neq(acc["g_W"], g0["g_W"] + g["g_W"])), 0.0))
    return out


class _WoBuffers:
    """Every buffer of a case's table, laid out exactly as WOBank._build lays a projection group out: one weff [tot][row], one weffT [row][tot] and
    one dweff [tot][row] per group, the entries row slices of weff / dweff and COLUMN slices of weffT.  Every output (weff, weffT, the nine gradients,
    g_W) lies between sentinel rows; vecs and partial are exactly e4t_wo_vecs_floats / e4t_wo_partial_floats long with sentinels behind them."""

    def __init__(self, lib, ops_mod, case, vals, dev):
        self.case, self.guards, self.scratch, self.entries, self.grads = case, [], [], [], []
        mode, i = case.mode, 0
        for row, cols in case.groups:
            tot = sum(cols)
            weff = _Guarded(tot, row, f32 if mode & WO_F32 else bf16, dev) if case.weff else None
            weffT = _Guarded(row, tot, bf16, dev) if case.weffT else None
            self.guards += [b for b in (weff, weffT) if b is not None]
            dweff = torch.cat([vals[i + j].dweff for j in range(len(cols))])
            off = 0
            for col in cols:
                v = vals[i]
                G = {"g_" + k: _Guarded(p.shape[0], p.shape[1], f32, dev) if k in ("wc", "wr") else _Guarded(1, p.numel(), f32, dev) for k, p in v.params.items()}
                if not mode & WO_OFF:
                    G["g_W"] = _Guarded(col, row, f32, dev)
                vecs, part = _Workspace(4 * lib.e4t_wo_vecs_floats(row, col), dev), _Workspace(4 * lib.e4t_wo_partial_floats(row, col), dev)
                self.guards += list(G.values())
                self.scratch += [vecs, part]
                self.grads.append({k: b.view.reshape(v.params[k[2:]].shape) if k != "g_W" else b.view for k, b in G.items()})
                self.entries.append(ops_mod.WOEntry(
                    row=row, col=col, W=v.W, params=v.params, weff=weff.view[off:off + col] if weff else None, weffT=weffT.view[:, off:off + col] if weffT else None,
                    dweff=dweff[off:off + col], grads={k: t for k, t in self.grads[-1].items() if k != "g_W"}, g_W=self.grads[-1].get("g_W"),
                    vecs=vecs.buf.view(f32)[:vecs.n], partial=part.buf.view(f32)[:part.n], mode=mode))
                off += col
                i += 1
        self.table = ops_mod.WOTable(self.entries)

    def forward_outputs(self):
        return [dict(weff=None if e.weff is None else e.weff.clone(), weffT=None if e.weffT is None else e.weffT.clone()) for e in self.entries]

    def backward_outputs(self):
        return [{k: t.clone() for k, t in g.items()} for g in self.grads]

    def vecs(self):
        out = []
        for e in self.entries:
            sizes = dict(a=e.row, b=e.col, s=e.col, vx=e.row, vy=e.col, da=e.row, db=e.col, ds=e.col)
            out.append(dict(zip(WO_VNAMES, e.vecs.clone().split([sizes[k] for k in WO_VNAMES]))))
        return out

    def poison(self):
        """NaN into every output and every word of the scratch"""
        for e, g in zip(self.entries, self.grads):
            for t in [e.weff, e.weffT, e.vecs, e.partial] + list(g.values()):
                if t is not None:
                    t.fill_(float("nan"))

    def prefill(self, g):
        """random G0 into the nine gradients and g_W of every entry -> copies of it"""
        for gr in self.grads:
            for t in gr.values():
                t.copy_(torch.randn(t.shape, generator=g, device=t.device, dtype=f32))
        return self.backward_outputs()

    def scratch_nans(self):
        return sum(int(torch.isnan(t).sum()) for e in self.entries for t in (e.vecs, e.partial))

    def sentinels_changed(self):
        return sum(b.outside() for b in self.guards) + sum(w.outside() for w in self.scratch)

    def touched(self):
        return sum(b.touched() for b in self.guards) + sum(int((w.buf != SENT32).sum()) for w in self.scratch)


def _sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def _wo_case_rows(hip, ops_mod, case, dev, poison=False):
    """One case: forward twice, backward (accumulate = 0) twice, backward with accumulate = 1 onto random G0; every entry of a table of several once
    more alone.  Value rows against wo_ref64 (wo_value_rows), the exact rows (tolerance 0.0), sentinels.  poison: NaN in every output and all of
    the scratch before the first launch; no NaN may be left in the scratch after the first backward."""
    lib = hip.lib
    vals = wo_values(case, dev)
    B = _WoBuffers(lib, ops_mod, case, vals, dev)
    if poison:
        B.poison()
    tag = "wo " + case.name + (" poisoned" if poison else "")
    hip.wo_forward(B.table)
    f1 = B.forward_outputs()
    hip.wo_forward(B.table)
    f2 = B.forward_outputs()
    hip.wo_backward(B.table, False)
    g1, vecs, nans = B.backward_outputs(), B.vecs(), B.scratch_nans()
    hip.wo_backward(B.table, False)
    g2 = B.backward_outputs()
    g0 = B.prefill(gen(case.seed + 50000, dev))
    hip.wo_backward(B.table, True)
    g3 = B.backward_outputs()
    _sync(dev)
    out = [(f"{tag}: sentinel words changed around weff, weffT, the gradients, g_W, behind vecs and partial", float(B.sentinels_changed()), 0.0)]
    if poison:
        out.append((f"{tag}: NaN words left in vecs / partial after forward + backward (every word is written)", float(nans), 0.0))
    both = lambda a, b: sum(_neq(a[k], b[k]) for k in a if a[k] is not None)
    for i, v in enumerate(vals):
        et = tag if len(vals) == 1 else f"{tag} [{i}] {v.row}->{v.col}"
        out += wo_value_rows(et, {**f1[i], **g1[i], "vecs": vecs[i]}, wo_ref64(v), case.mode)
        if f1[i]["weff"] is not None and f1[i]["weffT"] is not None:
            out += wo_transpose_row(et, f1[i]["weff"], f1[i]["weffT"])
        out.append((f"{et}: elements a second forward launch changes", float(both(f1[i], f2[i])), 0.0))
        out.append((f"{et}: elements a second backward launch changes", float(both(g1[i], g2[i])), 0.0))
        out += wo_accumulate_rows(et, g3[i], g0[i], g1[i])
        if len(vals) > 1:      # the same entry alone in a table of one, dense buffers of its own: bit for bit what it gave inside the table
            one = _WoBuffers(lib, ops_mod, _wo1(v.row, v.col, case.mode, case.weff, case.weffT), [v], dev)
            hip.wo_forward(one.table)
            hip.wo_backward(one.table, False)
            _sync(dev)
            diff = both(f1[i], one.forward_outputs()[0]) + both(g1[i], one.backward_outputs()[0])
            out.append((f"{et}: elements that differ from the same entry run alone", float(diff + one.sentinels_changed()), 0.0))
    return out


def check_wo_forms(hip, emu, dev, ops_mod):
    """WO_CASES: tail dims, the projection shapes check_wo leaves out, a mixed table, fused groups in WOBank's layout, every mode bit and NULL output;
    every kernel of wo.hip against the fp64 definition along its own blocks, g_W and accumulate = 0 / 1 on every case"""
    out = []
    for c in WO_CASES:
        out += _wo_case_rows(hip, ops_mod, c, dev)
    return out


def _wo_rejections(hip, dev, ops_mod):
    """calls the three entry points must refuse (-22, an error text) before launching anything: every guarded buffer keeps its sentinels"""
    from e4t.ops import _stream
    lib, out = hip.lib, []
    case = WO_GUARD_CASES[0]
    B = _WoBuffers(lib, ops_mod, case, wo_values(case, dev), dev)
    hip._pack_table(B.table, dev)
    T, st = B.table.dev.data_ptr(), _stream()
    calls = {"e4t_wo_forward": lambda *a: lib.e4t_wo_forward(*a, st), "e4t_weight_prepare": lambda *a: lib.e4t_weight_prepare(*a, st),
             "e4t_wo_backward": lambda *a: lib.e4t_wo_backward(*a, 0, st)}
    for name, fn in calls.items():
        for what, args, word in (("n = 0", (T, 0, 36, 100), "bad arguments"), ("a null table", (None, 1, 36, 100), "bad arguments"),
                                 ("max_row = 6", (T, 1, 6, 100), "multiples of 4"), ("max_col = 34", (T, 1, 36, 34), "multiples of 4")):
            code = fn(*args)
            _sync(dev)
            err = _last_error(lib)
            out.append((f"rejected: {name} with {what}: return code + 22", float(code + 22), 0.0))
            out.append((f"rejected: {name} with {what}: error text names {word!r} (got {err!r})", float(word not in err or name[4:] not in err), 0.0))
            out.append((f"rejected: {name} with {what}: output / scratch words changed", float(B.touched()), 0.0))
    return out


def check_wo_guards(hip, emu, dev, ops_mod):
    """WO_GUARD_CASES with NaN in every output and in all of the exactly sized scratch before the first launch: outputs finite and within tolerance
    of fp64 (a NaN anywhere makes its row infinite), no NaN left in the scratch, no sentinel changed; then the argument checks of the entry points"""
    out = []
    for c in WO_GUARD_CASES:
        out += _wo_case_rows(hip, ops_mod, c, dev, poison=True)
    return out + _wo_rejections(hip, dev, ops_mod)


def check_image_prep(hip, emu, dev):
    """data path (N2): byte-exact against the numpy restatement of SmallestMaxSize(INTER_AREA)+crop+flip+normalise,
    every resize branch (untouched / integer box / 2x2 / general area / enlarging fixed point), ragged sizes in one batch"""
    import numpy as np
    import image_prep_oracle as ipo
    sys_rng = np.random.default_rng(7)
    res = []
    for S, dims in ((64, [(128, 192), (192, 192), (97, 131), (40, 55), (64, 80), (65, 64), (64, 64), (201, 77)]),
                    (512, [(1024, 1536), (1536, 1536), (700, 933), (300, 400), (512, 640), (513, 700), (2048, 2731), (1200, 512)])):
        samples = []
        for i, (H, W) in enumerate(dims):
            img = sys_rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            nh, nw = ipo.smallest_max_size_dims(H, W, S)
            y0, x0 = ipo.random_crop_origin(nh, nw, S, sys_rng.random(), sys_rng.random())
            samples.append(dict(image=img, plan=(nh, nw, y0, x0, i & 1)))
        offs, total = [], 0
        for smp in samples:
            offs.append(total)
            total += (smp["image"].size + 15) // 16 * 16
        pool = np.zeros(total, np.uint8)
        table = []
        for smp, off in zip(samples, offs):
            im = smp["image"]
            pool[off:off + im.size] = im.reshape(-1)
            table.append([off, im.shape[0], im.shape[1], *smp["plan"]])
        d_pool = torch.from_numpy(pool).to(dev)
        d_table = torch.tensor(table, dtype=torch.int64, device=dev)
        got = hip.image_prep(d_pool, d_table, len(samples), S).cpu()
        for i, smp in enumerate(samples):
            nh, nw, y0, x0, flip = smp["plan"]
            want = torch.from_numpy(ipo.image_prep(smp["image"], S, y0, x0, bool(flip)))
            H, W = smp["image"].shape[:2]
            res.append((f"image_prep S={S} {H}x{W}->{nh}x{nw} flip={flip}", float((got[i] - want).abs().max()), 0.0))
    return res


def check_gemm_races(hip, emu, dev):
    """The DMA GEMM kernels hand an LDS stage back to the loader right after the K-loop barrier.  Until round 2 that barrier
    did not wait for the fragment reads of the stage to complete (gemm.hip, loop_barrier): with several workgroups per CU a
    tile in a thousand came out wrong, not reproducibly.  The kernels are deterministic, so ANY difference between
    repeated launches — and between the 2 / 3 / 4-stage variants, which accumulate in the same order — is a race.
    Grids of several waves, 2-5 workgroups per CU, operands larger than one XCD's L2."""
    out = []
    g = gen(400, dev)
    for M, N, K in [(4096, 1280, 320), (8192, 1280, 512), (16384, 640, 640), (131072, 320, 320)]:
        a, w = rnd(g, M, K, dev=dev), rnd(g, N, K, dev=dev)
        want = emu.gemm(a, w)
        ref = hip.gemm(a, w, tile=128)
        out.append((f"race-check reference {M}x{N}x{K}", rel(ref, want), TOL1))
        for code in (64, 3064, 4064, 128, 3128, 4128, 160, 3160, 4160, 5256, 512, 2320):
            if code % 1000 == 160 and N % 160:
                continue
            if code == 512 and N % 256:
                continue
            if code == 2320 and N % 320:
                continue
            differing = 0
            for _ in range(12):
                differing += int((hip.gemm(a, w, tile=code) != ref).sum() > 0)
            out.append((f"gemm {M}x{N}x{K} tile code {code}: launches (of 12) differing from the reference", float(differing), 0.0))
    x, w = rnd(g, 16 * 32 * 32, 640, dev=dev), rnd(g, 640, 9 * 640, dev=dev)
    ref = hip.conv3x3(x, w, 16, 32, 32, 32, 32, CONV_S1, tile=128)
    for code in (128, 3128, 160, 4160, 64, 3064, 2320, 512, 5256):
        sk = 1 if code in (2320, 512) else 0          # (its automatic split-K would change the summation order, not a race)
        run = lambda: hip.conv3x3(x, w, 16, 32, 32, 32, 32, CONV_S1, tile=code, splitk=sk)
        # 5256 walks 32-wide channel chunks: another fp32 summation order than the 64-wide tiles, so its bitwise reference is its own first
        # launch (checked against `ref` to tolerance)
        own = code == 5256
        r = run() if own else ref
        if own:
            out.append((f"conv 32x32 640->640 tile code {code} vs the channel-major kernels", rel(r, ref), TOL2))
        differing = sum(int((run() != r).sum() > 0) for _ in range(6))
        out.append((f"conv 32x32 640->640 tile code {code}: launches (of 6) differing", float(differing), 0.0))
    # tail rows (gemm_tail: cross-wave reduction through LDS in wave order, behind the tile epilogue's staging): repeated launches of the
    # ViT's shapes on the 128 x 160 / 256 x 320 / 256 x 256 tiles must be bitwise reproducible
    for (Mt, Nt, Kt, gelu) in [(4112, 1280, 5120, False), (4112, 5120, 1280, True), (4112, 3840, 1280, False)]:
        at, bt = rnd(g, Mt, Kt, dev=dev), rnd(g, Nt, Kt, scale=Kt ** -0.5, dev=dev)
        ref = hip.gemm(at, bt, gelu=gelu)
        differing = sum(int((hip.gemm(at, bt, gelu=gelu) != ref).sum() > 0) for _ in range(12))
        out.append((f"gemm {Mt}x{Nt}x{Kt} with tail rows: launches (of 12) differing", float(differing), 0.0))
    dy, xx = rnd(g, 16384, 640, dev=dev), rnd(g, 16384, 1280, dev=dev)
    ref = hip.gemm_tn(dy, xx)
    differing = sum(int((hip.gemm_tn(dy, xx) != ref).sum() > 0) for _ in range(12))
    out.append(("gemm_tn 640x1280 K=16384: launches (of 12) differing", float(differing), 0.0))
    return out


# ------------------------------------------------------------------------------------------------ dense GEMM: K-loop, edges, forms, guards
# Plain data, importable without a GPU.  tests/test_gemm_dispatch.py pins what e4t_gemm_kernel / e4t_gemm_tn_kernel say every case runs (kernel symbol,
# split-K, store path, reduce kernel, tail rows) and holds the set the cases reach against everything the query returns over the dispatch corpus;
# tests/test_gemm_slices_cpu.py holds a rounding-only model to half the tolerance on every row gemm_slices() emits for them.
# hint -> tile_m, tile_n, K-tile width, LDS stages, needs whole K-tiles, needs whole column tiles, has a GENERAL instantiation, carries the tail stage
GEMM_TILES = {
    64: (64, 64, 64, 2, False, False, True, False), 3064: (64, 64, 64, 3, False, False, True, False), 4064: (64, 64, 64, 4, False, False, False, False),
    128: (128, 128, 64, 2, False, False, True, False), 3128: (128, 128, 64, 3, False, False, False, False), 4128: (128, 128, 64, 4, False, False, False, False),
    160: (128, 160, 64, 2, False, False, True, True), 3160: (128, 160, 64, 3, False, False, False, True), 4160: (128, 160, 64, 4, False, False, False, True),
    5256: (256, 128, 32, 3, False, False, False, False), 512: (256, 256, 64, 2, True, False, True, True), 2320: (256, 320, 64, 2, True, True, True, True),
}
GemmCase = namedtuple("GemmCase", "M N K tile sk form batch K1", defaults=(1, 0))      # K1 > 0: two-source A, columns [K1, K) from A2
TnCase = namedtuple("TnCase", "K M N sk form")
# The call forms: which optional operands are given (NULL or not, and their alignment, are part of the launcher's decision), flags and strides.
# rowbias = rows_per_batch (32: a 32-row fragment lies in one entry; 24: the per-row lookup of the GENERAL instantiation)
GEMM_FORM_DEFS = {
    "bare": dict(), "bias": dict(bias=True), "bias+res": dict(bias=True, residual=True), "full": dict(bias=True, rowbias=32, residual=True),
    "gelu": dict(gelu=True), "gelu+bias+res": dict(bias=True, gelu=True, residual=True), "general full": dict(bias=True, rowbias=24, gelu=True, residual=True),
    "rowbias24": dict(rowbias=24),
    "f32": dict(bias=True, f32=True), "f32 res32": dict(bias=True, residual=True, f32=True, res32=True), "f32 res16": dict(bias=True, residual=True, f32=True),
    "accum16": dict(accum=True), "accum32": dict(accum=True, f32=True), "alpha": dict(bias=True, alpha=0.5),
    "rowbias slice": dict(rowbias=32, ldrb=1280),      # a column slice of a wider [rows][1280] matrix
    "C slice8": dict(bias=True, ldc_pad=8), "C slice4": dict(bias=True, ldc_pad=4), "res slice": dict(residual=True, ldr_pad=16),
    "colstats": dict(bias=True, colstats=True), "colstats+res": dict(bias=True, residual=True, colstats=True),
    "gelu C slice4": dict(bias=True, gelu=True, ldc_pad=4),      # the GENERAL instantiation through the scalar store
    "bias misaligned": dict(bias=True, bias_off=1),      # the bias starts 4 bytes behind a 16-byte boundary: the scalar reduce kernel under split-K
    "f32 bare": dict(f32=True),                          # fp32 C with nothing in the epilogue: the float4 reduce kernel under split-K
}
TN_FORM_DEFS = {"f32": dict(f32=True), "lda": dict(f32=True, lda_pad=8), "C slice": dict(f32=True, ldc_pad=372), "accum": dict(f32=True, accum=True),
                "alpha": dict(f32=True, alpha=0.5), "bf16": dict()}


def _gemm_mnk(hint):
    """one partial tile beside one full tile (tm + 40 rows, tn + 24 columns; two whole column tiles where the row needs them) and a K of two K-tiles
    plus the 16-byte granule (whole K-tiles where the row needs them)"""
    tm, tn, kt, st, whole_k, whole_n, general, tail = GEMM_TILES[hint]
    return tm + 40, (2 * tn if whole_n else tn + 24), (128 if whole_k else 136)


def _kloop_cases():
    out = []
    for hint, (tm, tn, kt, st, whole_k, whole_n, general, tail) in GEMM_TILES.items():
        M, N, _ = _gemm_mnk(hint)
        Ks = [kt * n for n in sorted({1, 2, 3, st, st + 1, st + 2, st + 3})]      # nkt % stages, nkt < stages: prologue, unrolled body, 1..3-step remainder
        if not whole_k:
            Ks += [64 + 8, 64 * st + 40]                                            # a ragged last K-tile: the 16-byte granule, and 40 of 64
        if kt == 32:
            Ks += [32 * 2 + 24, 32 * 3 + 16]                                        # ... which both leave 8 of a 32-wide K-tile: 24 and 16 of 32 too
        for forms in (("bare", "bias+res"),) + ((("gelu", "gelu+bias+res"),) if general else ()):
            for form in forms:
                out += [GemmCase(M, N, K, hint, 1, form) for K in Ks]
                # (splits are counted in 64-wide K-tiles on every row, the 32-wide one included: resolve_launch, ktiles_per_split)
                out.append(GemmCase(M, N, 320, hint, 2, form))      # 5 K-tiles of 64 in 2 splits: 3 + 2, the last one shorter
                out.append(GemmCase(M, N, 192, hint, 3, form))      # splitk == nkt: one 64-wide K-tile per split
    return out


def _edge_cases():
    out = []
    for hint, (tm, tn, kt, st, whole_k, whole_n, general, tail) in GEMM_TILES.items():
        M, N, K = _gemm_mnk(hint)
        cases = [GemmCase(1, N if whole_n else tn + 40, K, hint, 1, "?"), GemmCase(tm - 1, N, K, hint, 1, "?")]      # (M = 1: 40 columns, so that every slice holds >= 32 values)
        if not whole_n:
            cases += [GemmCase(M, 8, K, hint, 1, "?"), GemmCase(M, tn + 20, K, hint, 1, "?")]      # N = 8; N % 8 == 4: the scalar store
        # 10 row tiles x 3 column tiles = 30 tiles: crosses a raster group of group_m = 8 row panels, and the XCD re-deal has a remainder
        cases.append(GemmCase(9 * tm + 40, 3 * tn if whole_n else 2 * tn + 24, K, hint, 1, "?"))
        # two-source A: e4t_gemm_nt takes K1 % 64 == 0 only (no row takes another K1: the rejection is reached in gemm_guards); K - K1 = 40 < 64
        # where the row takes a ragged K
        cases.append(GemmCase(M, N, 128 if whole_k else 104, hint, 1, "?", 1, 64))
        if tail:
            cases += [GemmCase(1152 + r, 320, K if whole_k else 144, hint, 1, "?") for r in (1, 17, 32)]      # the tail stage (it wants K % 16 == 0)
        out += [c._replace(form=f) for c in cases for f in ("bare", "bias+res")]
        out += [GemmCase(M, N, K, hint, 1, f, 2) for f in ("bare", "bias")]      # batch 2, ragged M (a residual is not batched: every entry would read the same one)
    return out


GEMM_FORM_FAMILIES = (64, 128, 160, 5256, 512, 2320)      # gemm_dma_kernel at each tile shape, gemm_pp_kernel, gemm_pq_kernel
_GENERAL_FORMS = ("gelu", "gelu+bias+res", "general full", "rowbias24", "gelu C slice4")
GEMM_FORM_SPLITK = {"bias+res": "splitk_reduce8_kernel", "bias misaligned": "splitk_reduce_kernel", "f32 bare": "splitk_reduce4f_kernel"}


def _form_cases():
    out = []
    for hint in GEMM_FORM_FAMILIES:
        tm, tn, kt, st, whole_k, whole_n, general, tail = GEMM_TILES[hint]
        M, N, K = _gemm_mnk(hint)
        for form, f in GEMM_FORM_DEFS.items():
            if form in _GENERAL_FORMS and not general:      # (the planner's own answer: it sends these to a narrower tile, which has its own row here)
                continue
            out.append(GemmCase(tm + 32 if f.get("colstats") else M, N, K, hint, 1, form))      # column statistics: M % 32 == 0
        out += [GemmCase(M, N, 320, hint, 2, form) for form in GEMM_FORM_SPLITK]
    out.append(GemmCase(*_gemm_mnk(3064), 3064, 1, "gelu C slice4"))      # (the one GENERAL instantiation that is no family of its own)
    # the 3- and 4-stage rows share write_tile with their family; the direct fp32 store is the one path the K-loop and edge lists do not take them through
    return out + [GemmCase(*_gemm_mnk(h), h, 1, "f32 res32") for h in GEMM_TILES if h not in GEMM_FORM_FAMILIES]


GEMM_KLOOP_CASES = _kloop_cases()
GEMM_EDGE_CASES = _edge_cases()
GEMM_FORMS = _form_cases()
GEMM_TN_CASES = [
    TnCase(200, 168, 152, 1, "f32"),       # partial tiles in M and N; 200 rows = 3 K-tiles of 64 + 8
    TnCase(136, 8, 152, 1, "f32"),         # M = 8
    TnCase(300, 168, 152, 2, "f32"),       # 5 K-tiles in 2 splits: 3 + 2
    TnCase(2048, 136, 136, 0, "f32"),      # automatic split-K wants >= 16 K-tiles per split: K = 2048 is the smallest that splits (4 tiles, 2 splits)
    TnCase(200, 168, 152, 1, "lda"), TnCase(200, 168, 152, 1, "C slice"), TnCase(200, 168, 152, 1, "accum"), TnCase(200, 168, 152, 1, "alpha"),
    TnCase(200, 168, 152, 1, "bf16"), TnCase(300, 168, 152, 2, "bf16"), TnCase(300, 168, 152, 2, "accum"),
]
# gemm_guards: one ragged case per kernel symbol, bare and with the full epilogue, the GENERAL instantiations, the three reduce kernels, two-source A
GEMM_GUARD_CASES = (
    [GemmCase(*_gemm_mnk(h), h, 1, f) for h in GEMM_TILES for f in ("bare", "full")] +
    [GemmCase(*_gemm_mnk(h), h, 1, f) for h, t in GEMM_TILES.items() if t[6] for f in ("gelu", "general full")] +
    [GemmCase(104, 88, 320, 64, 2, f) for f in ("full", "bias misaligned", "f32 bare")] +
    [GemmCase(104, 88, 104, 64, 1, "full", 1, 64), GemmCase(296, 280, 128, 512, 1, "full", 1, 64)] +
    [GemmCase(1152 + 17, 320, 144, 160, 1, "bias+res")])
GEMM_AUTO_SPLIT_CASES = [GemmCase(104, 88, 2048, 64, 0, "bias+res"), TnCase(2048, 136, 136, 0, "f32")]      # the smallest K at which the automatic rule splits
GEMM_TN_GUARD_CASES = [TnCase(200, 168, 152, 1, "f32"), TnCase(300, 168, 152, 2, "f32"), TnCase(300, 168, 152, 2, "bf16")]
# fp32 output and TN against float64: 8 x the worst row a float32 restatement (float32 matmul, epilogue in float32) reaches against float64 over all
# fp32 and TN cases on the CPU (tests/test_gemm_slices_cpu.py measures it: GEMM_F32_WORST); the margin covers the MFMA's summation order and the
# split-K partial sums.  Never above the TOLF * 50 the existing fp32 rows use.
GEMM_F32_WORST = 1.3e-7      # measured 1.273e-7: gemm 104x88x320 t64 s2 f32 bare, rows 64-103
TOL_GEMM_F32 = min(8 * GEMM_F32_WORST, TOLF * 50)
GEMM_GUARD = 320      # NaN / sentinel rows in front of and behind every operand: the widest column tile (rows of B behind N), more than the tallest row tile


def gemm_tag(c):
    if isinstance(c, TnCase):
        return f"gemm_tn K{c.K} M{c.M} N{c.N} s{c.sk} {c.form}"
    return f"gemm {c.M}x{c.N}x{c.K} t{c.tile} s{c.sk} {c.form}" + (f" batch{c.batch}" if c.batch > 1 else "") + (f" K1={c.K1}" if c.K1 else "")


def gemm_form(c):
    return TN_FORM_DEFS[c.form] if isinstance(c, TnCase) else GEMM_FORM_DEFS[c.form] if c.form in GEMM_FORM_DEFS else CHECK_GEMM_FORM_DEFS[c.form]


def gemm_layout(c, guarded=False):
    """leading dimensions and row counts of every operand of a case; guarded: 8 more elements per row of A, A2 and B (the `lda > K` gap), of C (the
    `ldc - N` gap columns, which hold sentinels) and of the residual — a pad of 8 keeps every 16-byte alignment, so kernel and store path stay"""
    f, pad = gemm_form(c), 8 if guarded else 0
    if isinstance(c, TnCase):
        return dict(lda=c.M + f.get("lda_pad", 0) + pad, ldb=c.N + pad, ldc=c.N + f.get("ldc_pad", 0) + pad, K1=c.K, lda2=0, ldr=0, ldrb=0, rb_rows=0)
    K1 = c.K1 or c.K
    rpb = f.get("rowbias", 0)
    return dict(lda=K1 + pad, lda2=(c.K - K1 + pad) if c.K1 else 0, ldb=c.K + pad, ldc=c.N + f.get("ldc_pad", 0) + pad, K1=K1,
                ldr=(c.N + f.get("ldr_pad", 0) + pad) if f.get("residual") else 0, ldrb=f.get("ldrb", c.N) if rpb else 0, rb_rows=-(-c.M // rpb) if rpb else 0)


def gemm_flags(c):
    from e4t import _C
    f = gemm_form(c)
    return ((_C.OUT_F32 if f.get("f32") else 0) | (_C.RES_F32 if f.get("res32") else 0) | (_C.ACT_GELU if f.get("gelu") else 0) | (_C.ACCUM if f.get("accum") else 0))


def gemm_desc(c, ptrs=None, guarded=False, ws=None, ws_bytes=None, splitk=None):
    """the descriptor of a case.  ptrs = None: pointers that are never dereferenced, with the alignment the real operands have, and a workspace that
    is large enough — for e4t_gemm_plan / e4t_gemm_kernel / e4t_gemm_tn_kernel (pure host code)"""
    from e4t import _C
    f, L, fake = gemm_form(c), gemm_layout(c, guarded), 1 << 24
    tn = isinstance(c, TnCase)
    if ptrs is None:
        used = dict(A=True, B=True, C=True, A2=not tn and c.K1, bias=f.get("bias"), residual=f.get("residual"), rowbias=f.get("rowbias"),
                    colstats=f.get("colstats"))
        ptrs = {k: fake for k, v in used.items() if v}
        if f.get("bias_off"):
            ptrs["bias"] = fake + 4 * f["bias_off"]
        ws, ws_bytes = (fake, 1 << 40) if ws_bytes is None else (ws, ws_bytes)
    batch = 1 if tn else c.batch
    d = _C.GemmDesc(M=c.M, N=c.N, K=c.K, K1=L["K1"], lda=L["lda"], lda2=L["lda2"], ldb=L["ldb"], ldc=L["ldc"], ldr=L["ldr"], ldrb=L["ldrb"],
                    rows_per_batch=f.get("rowbias", 0), flags=gemm_flags(c), tile=0 if tn else c.tile, splitk=c.sk if splitk is None else splitk, batch=batch,
                    alpha=f.get("alpha", 1.0), workspace=ws, workspace_bytes=ws_bytes or 0)
    if batch > 1:
        d.strideA, d.strideB, d.strideC = c.M * L["lda"], c.N * L["ldb"], c.M * L["ldc"]
    for k, v in ptrs.items():
        setattr(d, k, v)
    return d


# call forms of check_gemm that GEMM_FORMS does not run as such
CHECK_GEMM_FORM_DEFS = {"gelu+bias": dict(bias=True, gelu=True), "gelu f32": dict(gelu=True, f32=True), "accum32 alpha": dict(accum=True, f32=True, alpha=0.5),
                        "rowbias96": dict(rowbias=96), "rowbias97": dict(rowbias=97)}


def check_gemm_pinned():
    """every launch of check_gemm as (label, case, descriptor fields set last): what hip.gemm / hip.gemm_tn hand the library for it, from the same
    shape lists, for tests/test_gemm_dispatch.py to pin (the row labels of check_gemm where one launch makes one row)"""
    from e4t import _C
    out = [(f"gemm {M}x{N}x{K} t{t} s{sk} bias+res", GemmCase(M, N, K, t, sk, "bias+res"), {}) for M, N, K, t, sk in CHECK_GEMM_NT]
    out += [(f"gemm_tn K{K} M{M} N{N} s{sk}", TnCase(K, M, N, sk, "lda"), {}) for K, M, N, sk in CHECK_GEMM_TN]
    out += [("gemm_tn fp32 accumulate", TnCase(500, 320, 328, 0, "accum"), {}), ("gemm_tn into a column slice", TnCase(500, 320, 328, 0, "C slice"), {})]
    out += [(f"gemm {M}x{N}x{K} t{t} colstats" + (" + residual" if i % 2 == 0 else ""), GemmCase(M, N, K, t, 1, "colstats+res" if i % 2 == 0 else "colstats"), {})
            for i, (M, N, K, t) in enumerate(CHECK_GEMM_COLSTATS)]
    out += [("gemm two-source A" + (f" t{t}" if t else ""), GemmCase(384, 192, 192, t, 0, "bare", 1, 128), {}) for t in (0, 512, 3064, 2320)]
    out += [("gemm gelu" + (f" t{t}" if t else ""), GemmCase(384, 192, 128, t, 0, "gelu"), {}) for t in (0, 3064, 512, 2320)]
    out += [("gemm gelu fp32-out t512", GemmCase(384, 192, 128, 512, 0, "gelu f32"), {}), ("gemm fp32 out + accumulate + alpha", GemmCase(384, 192, 128, 0, 0, "accum32 alpha"), {}),
            ("gemm rowbias", GemmCase(384, 192, 128, 0, 0, "rowbias96"), {}), ("gemm strided A view", GemmCase(384, 192, 128, 0, 0, "bare"), dict(lda=384))]
    for M, N, K, kw in CHECK_GEMM_TAIL:
        form = "f32 res32" if kw.get("f32") else "gelu+bias" if kw.get("gelu") else "bias+res" if kw.get("res") else "bias"
        out.append((f"gemm {M}x{N}x{K} tail {form}", GemmCase(M, N, K, 0, 0, form), {}))
    out += [(f"gemm {M}x{N}x{K} t{t} fp32 out + fp32 residual", GemmCase(M, N, K, t, 0, "f32 res32"), {}) for M, N, K, t in CHECK_GEMM_F32RES]
    for M, N, K in CHECK_GEMM_PQ_GENERAL:
        out.append((f"gemm {M}x{N}x{K} t2320 gelu", GemmCase(M, N, K, 2320, 0, "gelu+bias"), {}))
        out.append((f"gemm {M // 97 * 97}x{N}x{K} t2320 row bias, rows_per_batch 97", GemmCase(M // 97 * 97, N, K, 2320, 0, "rowbias97"), {}))
    for B, T, N, K, pr, dt in CHECK_GEMM_PANELS:
        out.append((f"gemm row panels B{B} T{T} N{N} K{K}", GemmCase(B * pr, N, K, 0, 0, "gelu+bias" if dt == bf16 else "f32 res32"), dict(panel_rows=pr, panel_stride=T, panel_off=T - pr)))
    out += [("gemm batched", GemmCase(16, 128, 128, 0, 0, "bias", 9), dict(strideBias=128)),
            ("gemm batched reduce (mean over slots)", GemmCase(16, 128, 128, 0, 0, "f32 bare", 9), dict(flags=_C.OUT_F32 | _C.REDUCE_BATCH, alpha=1.0 / 9, strideC=0)),
            ("gemm batched broadcast A", GemmCase(16, 128, 128, 0, 0, "bare", 9), dict(strideA=0))]
    out += [(f"gemm batched t{t}", GemmCase(300, 320, 128, t, 0, "bias", 2), dict(strideBias=320)) for t in (512, 2320)]
    return out


def check_gemm_logged(hip, emu, dev):
    """check_gemm with the launch log on, plus one row that ties check_gemm_pinned() to it: the "<symbol>|<shape string>" of every GEMM / TN launch
    the log shows == those the pinned descriptors give (symbol and split-K from e4t_gemm_kernel / e4t_gemm_tn_kernel, shape, batch and flags from the
    descriptor), as sets (CHECK_GEMM_COLSTATS runs one shape twice).  A check_gemm call or an ops.gemm change that the restatement misses fails here."""
    import os
    import tempfile
    fd, path = tempfile.mkstemp(suffix=".launchlog")
    os.close(fd)
    try:
        assert hip.lib.e4t_set_launch_log(path.encode()) == 0
        try:
            out = check_gemm(hip, emu, dev)
            torch.cuda.synchronize()
        finally:
            hip.lib.e4t_set_launch_log(None)
        with open(path) as f:
            logged = {"|".join(l.split("|")[:2]) for l in f.read().splitlines() if "|gemm M" in l or "|gemm_tn M" in l}
    finally:
        os.unlink(path)
    want = set()
    for label, c, override in check_gemm_pinned():
        d = gemm_desc(c)
        for k, v in override.items():
            setattr(d, k, v)
        rc, k = gemm_kernel(c, d)
        if isinstance(c, TnCase):
            want.add(f"{k.symbol.decode()}|gemm_tn M{c.M} N{c.N} K{c.K} splitk{k.splitk} flags{d.flags}")
        else:
            want.add(f"{k.symbol.decode()}|gemm M{c.M} N{c.N} K{c.K} batch{c.batch} splitk{k.splitk} flags{d.flags}")
    diff = sorted(logged ^ want)
    return out + [(f"check_gemm's launch log == the pinned descriptors of check_gemm_pinned() ({len(logged)} distinct launches; differing: {diff[:6]})", float(len(diff)), 0.0)]


def gemm_plan(c, **kw):
    import ctypes
    from e4t import _C
    pl = _C.GemmPlan()
    fn = _C.load().e4t_gemm_tn_plan if isinstance(c, TnCase) else _C.load().e4t_gemm_plan
    _C.check(fn(ctypes.byref(gemm_desc(c, **kw)), ctypes.byref(pl)), "e4t_gemm_plan")
    return pl


def gemm_kernel(c, d=None):
    """the launcher's own decision for a case (e4t_gemm_kernel / e4t_gemm_tn_kernel) -> (rc, e4t_gemm_kernel_t)"""
    import ctypes
    from e4t import _C
    k = _C.GemmKernel()
    fn = _C.load().e4t_gemm_tn_kernel if isinstance(c, TnCase) else _C.load().e4t_gemm_kernel
    return fn(ctypes.byref(d if d is not None else gemm_desc(c)), ctypes.byref(k)), k


def gemm_kernel_text(k):
    """'<symbol> splitk<n> <store path> [<reduce symbol>] [tail<r>]' in clear text"""
    from e4t import _C
    return " ".join([f"{k.symbol.decode()} splitk{k.splitk} {_C.STORE_NAMES[k.store]}"] + ([k.reduce.decode()] if k.reduce else []) +
                    ([f"tail{k.tail_rows}"] if k.tail_rows else []))


def gemm_values(c, seed, dev):
    """dense values of every operand of a case: unit-variance product, bias, row bias, residual and (accumulate) initial C"""
    g, f = gen(seed, dev), gemm_form(c)
    out_dt = f32 if f.get("f32") else bf16
    if isinstance(c, TnCase):
        v = dict(a=rnd(g, c.K, c.M, dev=dev), b=rnd(g, c.K, c.N, scale=c.K ** -0.5, dev=dev))
        rows = c.M
    else:
        K1, rows = c.K1 or c.K, c.batch * c.M
        v = dict(a=rnd(g, rows, K1, dev=dev), b=rnd(g, c.batch * c.N, c.K, scale=c.K ** -0.5, dev=dev))
        if c.K1:
            v["a2"] = rnd(g, rows, c.K - K1, dev=dev)
    if f.get("bias"):
        v["bias"] = rnd(g, c.N, dtype=f32, dev=dev)
    if f.get("rowbias"):
        v["rowbias"] = rnd(g, -(-c.M // f["rowbias"]), c.N, dtype=f32, dev=dev)
    if f.get("residual"):
        v["residual"] = rnd(g, rows, c.N, dtype=f32 if f.get("res32") else bf16, dev=dev)
    if f.get("accum"):
        v["c0"] = rnd(g, rows, c.N, dtype=out_dt, dev=dev)
    return v


def _gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * (0.5 ** 0.5)))


def gemm_ref64(c, v, store, tail=0):
    """float64 restatement of the descriptor's semantics from the bf16 inputs -> [batch * M, N], BEFORE the rounding to the output type.  Rounding
    points as write_tile states them: alpha, bias, row bias and GELU are applied before any rounding; the LDS-staged bf16 path (store ==
    'bf16-staged') rounds that value to bf16, adds the residual to the ROUNDED value and rounds again; every other path (scalar store, fp32 direct,
    the reduce kernels, the tail rows) adds residual and (accumulate) the old C first and rounds once."""
    f64 = torch.float64
    f = gemm_form(c)
    if isinstance(c, TnCase):
        y = v["a"].to(f64).t() @ v["b"].to(f64)
    else:
        a = torch.cat([v["a"], v["a2"]], dim=1) if c.K1 else v["a"]
        y = torch.cat([a[i * c.M:(i + 1) * c.M].to(f64) @ v["b"][i * c.N:(i + 1) * c.N].to(f64).t() for i in range(c.batch)])
    y = y * f.get("alpha", 1.0)
    if "bias" in v:
        y = y + v["bias"].to(f64)
    if "rowbias" in v:
        y = y + v["rowbias"].to(f64).repeat_interleave(f["rowbias"], dim=0)[:c.M]
    if f.get("gelu"):
        y = _gelu64(y)
    if "residual" in v:
        if store == "bf16-staged":
            main = y.shape[0] - tail
            y = torch.cat([y[:main].to(f32).to(bf16).to(f64), y[main:]])
        y = y + v["residual"].to(f64)
    if "c0" in v:
        y = y + v["c0"].to(f64)
    return y


def gemm_slices(tag, got, ref, plan, batch=1, tol=TOL1):
    """Result rows that one whole-matrix relative L2 dilutes: got, ref = [batch * M, N] (ref float64).  The relative L2 of the whole matrix, the first
    row tile and the last, partial one, the first and the last column tile, the corner block of the last row tile x the last column tile, the interior
    (everything else), the tail rows and the 64 rows in front of them, and the first and last batch entry.  Empty and duplicate regions are skipped.
    The tolerance is the whole matrix's: the stated bound is per element (tests/test_gemm_slices_cpu.py holds a rounding-only model to half of it on
    every row emitted here, down to 32 values)."""
    f64 = torch.float64
    N = ref.shape[-1]
    M = ref.shape[0] // batch
    g, r = got.to(f64).reshape(batch, M, N), ref.to(f64).reshape(batch, M, N)
    d2, r2 = (g - r) ** 2, r * r
    tm, tn, tail = plan.tile_m, plan.tile_n, plan.tail_rows
    Mg = M - tail                                     # rows of the tile grid
    r_last = (Mg - 1) // tm * tm                      # first row of the last row tile, first column of the last column tile
    c_last = (N - 1) // tn * tn
    out, seen = [], set()

    def row(label, rs, cs, bs=slice(None)):
        key = (rs.indices(M), cs.indices(N), bs.indices(batch))
        d, n = d2[bs, rs, cs], r2[bs, rs, cs]
        if d.numel() and key not in seen:
            seen.add(key)
            e = (d.sum() / (n.sum() + 1e-300)).sqrt()
            out.append((f"{tag}: {label}", float(torch.nan_to_num(e, nan=float("inf"))), tol))
    A = slice(None)
    row("whole", A, A)
    row(f"rows 0-{min(tm, Mg) - 1} (the first row tile)", slice(0, min(tm, Mg)), A)
    row(f"rows {r_last}-{Mg - 1} (the last row tile)", slice(r_last, Mg), A)
    row(f"columns 0-{min(tn, N) - 1} (the first column tile)", A, slice(0, min(tn, N)))
    row(f"columns {c_last}-{N - 1} (the last column tile)", A, slice(c_last, N))
    row("corner (last row tile x last column tile)", slice(r_last, Mg), slice(c_last, N))
    row("interior", slice(tm, r_last), slice(tn, c_last))
    if tail:
        row(f"the {tail} tail rows", slice(Mg, M), A)
        row("the 64 rows in front of the tail", slice(Mg - 64, Mg), A)
    if batch > 1:
        row("batch entry 0", A, A, slice(0, 1))
        row(f"batch entry {batch - 1}", A, A, slice(batch - 1, batch))
    return out


class _GemmOperands:
    """every operand of a case as a view into a larger allocation the test owns.  guard = 0: dense, nothing around them.  guard > 0: NaN rows in
    front of and behind A, A2, B, bias, row bias and residual, NaN in the 8-element gap behind every row of A, A2, B and the residual, sentinel rows
    around C and the column statistics, sentinels in the 8 gap columns behind every row of C (gemm_layout)."""

    def __init__(self, c, v, dev, guard=0):
        self.c, self.guard, self.dev = c, guard, dev
        f, L = gemm_form(c), gemm_layout(c, guard > 0)
        self.f, self.L, self.tn = f, L, isinstance(c, TnCase)
        self.ptrs, self.keep = {}, []
        nan = float("nan")
        self.ptrs["A"] = self._inp(v["a"], L["lda"], nan)
        self.ptrs["B"] = self._inp(v["b"], L["ldb"], nan)
        if "a2" in v:
            self.ptrs["A2"] = self._inp(v["a2"], L["lda2"], nan)
        if "bias" in v:
            off = f.get("bias_off", 0)
            buf = torch.full((guard + off + c.N + guard,), nan, dtype=f32, device=dev)
            buf[guard + off:guard + off + c.N] = v["bias"]
            self.keep.append(buf)
            self.ptrs["bias"] = buf[guard + off:].data_ptr()
        if "rowbias" in v:
            self.ptrs["rowbias"] = self._inp(v["rowbias"], L["ldrb"], nan)
        if "residual" in v:
            self.ptrs["residual"] = self._inp(v["residual"], L["ldr"], nan)
        rows = c.M if self.tn else c.batch * c.M
        self.out_dt = f32 if f.get("f32") else bf16
        w16 = L["ldc"] * (2 if self.out_dt == f32 else 1)
        self.cbuf = torch.full((guard + rows + guard, w16), SENT16, dtype=torch.int16, device=dev)
        self.C = self.cbuf[guard:guard + rows].view(self.out_dt)[:, :c.N]
        if "c0" in v:
            self.C.copy_(v["c0"])
        self.ptrs["C"] = self.C.data_ptr()
        self.cs = None
        if f.get("colstats"):
            n = (c.M // 32) * c.N * 2
            self.csbuf = torch.full((guard * 8 + n + guard * 8,), SENT32, dtype=torch.int32, device=dev)
            self.cs = self.csbuf[guard * 8:guard * 8 + n].view(f32).view(c.M // 32, c.N, 2)
            self.ptrs["colstats"] = self.cs.data_ptr()
        self.c_before = self.cbuf.clone()

    def _inp(self, t, ld, fill):
        rows, cols = t.shape
        buf = torch.full((self.guard + rows + self.guard, ld), fill, dtype=t.dtype, device=self.dev)
        buf[self.guard:self.guard + rows, :cols] = t
        self.keep.append(buf)
        return buf[self.guard:].data_ptr()

    def sentinels_changed(self):
        """elements outside C[:, :N] (guard rows, gap columns) and around the column statistics that changed"""
        ch = self.cbuf != self.c_before
        rows = self.C.shape[0]
        ch[self.guard:self.guard + rows, :self.c.N * (2 if self.out_dt == f32 else 1)] = False      # (cbuf is int16: an fp32 element is two of its columns)
        n = int(ch.sum())
        if self.cs is not None and self.guard:
            g8 = self.guard * 8
            n += int((self.csbuf[:g8] != SENT32).sum()) + int((self.csbuf[g8 + self.cs.numel():] != SENT32).sum())
        return n

    def c_touched(self):
        """elements of the whole C allocation, C included, that changed (a rejected call must leave 0)"""
        return int((self.cbuf != self.c_before).sum())


def gemm_launch(hip, c, ops, ws="plan", splitk=None, override=None, only_if_refused=False):
    """one launch of a case through the raw ABI on placed operands `ops` -> (rc, e4t_gemm_kernel_t of the same descriptor, workspace).  ws: 'plan' = exactly
    the plan's workspace_bytes (sentinels behind it), 'short' = one float less, 'none'.  override: descriptor fields set last."""
    import ctypes
    from e4t.ops import _stream
    tn = isinstance(c, TnCase)
    d = gemm_desc(c, ptrs=ops.ptrs, guarded=ops.guard > 0, ws=None, ws_bytes=0, splitk=splitk)
    for k, val in (override or {}).items():
        setattr(d, k, val)
    pl = _Cmod().GemmPlan()
    rc = (hip.lib.e4t_gemm_tn_plan if tn else hip.lib.e4t_gemm_plan)(ctypes.byref(d), ctypes.byref(pl))
    w = None
    if rc == 0 and ws != "none" and pl.workspace_bytes:
        w = _Workspace(pl.workspace_bytes - (4 if ws == "short" else 0), ops.dev)
        d.workspace, d.workspace_bytes = w.ptr, w.bytes
    rcq, k = gemm_kernel(c, d)
    if only_if_refused and rcq >= 0:      # a descriptor that is meant to be refused is never launched: the query makes the launch's own checks
        return 0, rcq, k, w, pl
    rc = (hip.lib.e4t_gemm_tn if tn else hip.lib.e4t_gemm_nt)(ctypes.byref(d), _stream())
    return rc, rcq, k, w, pl


def _Cmod():
    from e4t import _C
    return _C


def _gemm_case_rows(hip, c, seed, dev, tol_f32=None):
    """one case: launch, float64 reference with the store path's rounding points, slices"""
    f = gemm_form(c)
    v = gemm_values(c, seed, dev)
    ops = _GemmOperands(c, v, dev)
    rc, rcq, k, w, pl = gemm_launch(hip, c, ops)
    tag = gemm_tag(c)
    if rc < 0 or rcq != 0:
        return [(f"{tag}: launch rc {rc}, query rc {rcq} ({_last_error(hip.lib)})", 1.0, 0.0)]
    store = _Cmod().STORE_NAMES[k.store]
    ref = gemm_ref64(c, v, store, k.tail_rows)
    tol = TOL_GEMM_F32 if f.get("f32") else TOL1
    batch = 1 if isinstance(c, TnCase) else c.batch
    out = gemm_slices(f"{tag} [{gemm_kernel_text(k)}]", ops.C, ref, pl, batch, tol)
    if ops.L["ldc"] > c.N:
        out.append((f"{tag}: sentinels in the {ops.L['ldc'] - c.N} gap columns of C changed", float(ops.sentinels_changed()), 0.0))
    if f.get("colstats"):
        y = ops.C.float().reshape(c.M // 32, 32, c.N)
        want = torch.stack([y.sum(1), (y * y).sum(1)], dim=-1)
        out.append((f"{tag} colstats: reported written (1 = not)", float(rc != 1 or not k.colstats), 0.0))
        out.append((f"{tag} colstats: == the statistics of the kernel's own output", rel(ops.cs, want) if rc == 1 else 1.0, 1e-5))
    return out


def check_gemm_kloop(hip, emu, dev):
    """every DMA row of the variant table crossed with the K-loop's code paths (GEMM_KLOOP_CASES), bare and bias + residual, in slices"""
    return [r for i, c in enumerate(GEMM_KLOOP_CASES) for r in _gemm_case_rows(hip, c, 5000 + i, dev)]


def check_gemm_edges(hip, emu, dev):
    """M = 1, M = tile - 1, N = 8, N % 8 == 4, more than one raster group, two-source A, batch, the tail stage, on every kernel row; the TN kernel"""
    return [r for i, c in enumerate(GEMM_EDGE_CASES + GEMM_TN_CASES) for r in _gemm_case_rows(hip, c, 6000 + i, dev)]


def check_gemm_forms(hip, emu, dev):
    """every call form on one case per kernel family (GEMM_FORMS); column statistics as check_conv_forms checks them"""
    return [r for i, c in enumerate(GEMM_FORMS) for r in _gemm_case_rows(hip, c, 7000 + i, dev)]


def _gemm_guard_rows(hip, c, seed, dev):
    tag = gemm_tag(c) + ", guarded"
    v = gemm_values(c, seed, dev)
    plain, guarded = _GemmOperands(c, v, dev), _GemmOperands(c, v, dev, GEMM_GUARD)
    rc0, _, k0, _, _ = gemm_launch(hip, c, plain)
    rc1, rcq, k1, w, pl = gemm_launch(hip, c, guarded)
    if rc0 < 0 or rc1 < 0 or rcq != 0:
        return [(f"{tag}: launch rc {rc0} / {rc1}, query rc {rcq} ({_last_error(hip.lib)})", 1.0, 0.0)]
    bits = lambda t: t.contiguous().view(torch.int16)
    out = [(f"{tag}: the guarded run takes another kernel ({gemm_kernel_text(k0)} / {gemm_kernel_text(k1)})", float(gemm_kernel_text(k0) != gemm_kernel_text(k1)), 0.0),
           (f"{tag} [{gemm_kernel_text(k1)}]: elements differing from the unguarded run", float((bits(guarded.C) != bits(plain.C)).sum()), 0.0),
           (f"{tag}: non-finite elements", float((~torch.isfinite(guarded.C.float())).sum()), 0.0),
           (f"{tag}: sentinel elements changed (rows around C, the {guarded.L['ldc'] - c.N} gap columns of every row)", float(guarded.sentinels_changed()), 0.0)]
    if w is not None:
        out.append((f"{tag}: sentinels behind the {w.bytes}-byte workspace changed", float(w.outside()), 0.0))
    if guarded.cs is not None:
        out.append((f"{tag}: column statistics differing from the unguarded run", float((guarded.cs != plain.cs).sum()), 0.0))
    return out


def _gemm_short_workspace_rows(hip, c, seed, dev):
    """one float less than the plan's workspace: -12 with an explicit split (C untouched); in auto mode one pass that is bitwise the splitk = 1 run"""
    tag, v = gemm_tag(c), gemm_values(c, seed, dev)
    ops = _GemmOperands(c, v, dev, GEMM_GUARD)
    rc, rcq, k, w, pl = gemm_launch(hip, c, ops, ws="short", only_if_refused=True)
    out = [(f"{tag}: one float less of workspace, explicit split-K: launch rc {rc}, query rc {rcq}, want -12", float(rc != -12 or rcq != -12), 0.0),
           (f"{tag}: ... leaves C untouched", float(ops.c_touched()), 0.0)]
    return out


def _gemm_rejection_rows(hip, dev):
    """each argument rejection of e4t_gemm_nt / e4t_gemm_tn once: its code, the query agrees, C untouched"""
    out = []
    c = GemmCase(104, 88, 136, 64, 1, "full")
    t = TnCase(200, 168, 152, 1, "f32")
    v, vt = gemm_values(c, 8900, dev), gemm_values(t, 8901, dev)
    two = GemmCase(104, 88, 104, 64, 1, "full", 1, 64)
    v2 = gemm_values(two, 8902, dev)
    pan = GemmCase(512, 320, 128, 2320, 1, "bare")
    vp = gemm_values(pan, 8903, dev)
    nt = [("null A", c, v, dict(A=None), "null operand"), ("M = 0", c, v, dict(M=0), "bad shape"), ("K % 8 != 0", c, v, dict(K=132), "multiples of 8"),
          ("lda % 8 != 0", c, v, dict(lda=140), "multiples of 8"), ("ldb % 8 != 0", c, v, dict(ldb=140), "multiples of 8"),
          ("misaligned A", c, v, "A+2", "16-B aligned"), ("misaligned B", c, v, "B+2", "16-B aligned"),
          ("K1 % 64 != 0", two, v2, dict(K1=40), "two-source A"), ("K1 = 0", two, v2, dict(K1=0), "two-source A"), ("K1 >= K", two, v2, dict(K1=128), "two-source A"),
          ("misaligned A2", two, v2, "A2+2", "two-source A"), ("lda2 % 8 != 0", two, v2, dict(lda2=44), "two-source A"),
          ("row bias without rows_per_batch", c, v, dict(rows_per_batch=0), "rowbias needs rows_per_batch"),
          ("batch stride % 8 != 0", c, v, dict(batch=2, strideA=104 * 136 + 4, strideB=0, strideC=0), "batch strides"),
          ("reduce-batch with two-source A", two, v2, dict(flags=16 | 1, batch=2), "reduce-batch with two-source A"),
          ("panel_rows % 256 != 0", pan, vp, dict(panel_rows=128, panel_stride=128), "panel_rows %% 256"),
          ("row panels with split-K", pan, vp, dict(panel_rows=256, panel_stride=256, splitk=2), "do not combine"),
          ("row panels on a tile without them", pan, vp, dict(panel_rows=256, panel_stride=256, N=88), "the plan chose tile"),
          ("fused GEGLU without aux", c, v, dict(flags=32), "need aux")]
    tnr = [("null B", t, vt, dict(B=None), "null operand"), ("batch 2", t, vt, dict(batch=2), "bad / unsupported"), ("GELU", t, vt, dict(flags=1 | 4), "not built for the TN kernel"),
           ("M % 8 != 0", t, vt, dict(M=164), "multiples of 8"), ("N % 8 != 0", t, vt, dict(N=148), "multiples of 8"), ("lda % 8 != 0", t, vt, dict(lda=172), "multiples of 8"),
           ("misaligned A", t, vt, "A+2", "multiples of 8"),
           ("operands beyond 4 GB", t, vt, dict(lda=12000000), "beyond 4 GB")]      # (199 rows of 12e6 elements; refused before anything is launched or read)
    for what, case, vals, ov, says in nt + tnr:
        ops = _GemmOperands(case, vals, dev, GEMM_GUARD)
        if isinstance(ov, str):
            ov = {ov[:-2]: ops.ptrs[ov[:-2]] + 2}
        rc, rcq, k, w, pl = gemm_launch(hip, case, ops, override=ov, only_if_refused=True)
        msg = _last_error(hip.lib)
        fn = "e4t_gemm_tn" if isinstance(case, TnCase) else "e4t_gemm_nt"
        out.append((f"{fn} rejects {what}: launch rc {rc}, query rc {rcq}, want -22 and '{says.replace('%%', '%')}' in the message ({msg})",
                    float(rc != -22 or rcq != -22 or says.replace("%%", "%") not in msg), 0.0))
        out.append((f"{fn} rejects {what}: C untouched", float(ops.c_touched()), 0.0))
    return out


def check_gemm_guards(hip, emu, dev):
    """every GEMM kernel symbol, the reduce kernels and the TN kernel on operands with poison around and between them (GEMM_GUARD_CASES): bitwise the
    unguarded run, finite, no sentinel changed; the workspace is exactly the plan's; one float less; row panels; every argument rejection"""
    out = []
    cases = GEMM_GUARD_CASES + GEMM_TN_GUARD_CASES
    for i, c in enumerate(cases):
        out += _gemm_guard_rows(hip, c, 8000 + i, dev)
    for i, c in enumerate([x for x in cases if x.sk > 1]):
        out += _gemm_short_workspace_rows(hip, c, 8500 + i, dev)
    # automatic split-K (the smallest shapes whose plan splits) with one float less: one pass, bitwise the splitk = 1 run
    for i, c in enumerate(GEMM_AUTO_SPLIT_CASES):
        v = gemm_values(c, 8600 + i, dev)
        one, short = _GemmOperands(c, v, dev), _GemmOperands(c, v, dev, GEMM_GUARD)
        rc0, _, k0, _, _ = gemm_launch(hip, c, one, splitk=1)
        rc1, rcq, k1, w, pl = gemm_launch(hip, c, short, ws="short")
        tag = gemm_tag(c)
        out.append((f"{tag}: the plan splits (split-K {pl.splitk}); one float less of workspace runs one pass (query: split-K {k1.splitk}, rc {rc1} / {rcq})",
                    float(pl.splitk <= 1 or rc1 < 0 or rcq != 0 or k1.splitk != 1 or k1.reduce is not None), 0.0))
        out.append((f"{tag}: ... bitwise the splitk = 1 run", float((short.C.contiguous().view(torch.int16) != one.C.contiguous().view(torch.int16)).sum()), 0.0))
        out.append((f"{tag}: ... sentinels changed", float(short.sentinels_changed() + (w.outside() if w else 0)), 0.0))
    # row panels: the rows between the panels (and around them) stay untouched
    pr, T, nb, N, K = 256, 257, 3, 320, 64
    c = GemmCase(nb * pr, N, K, 2320, 1, "bias")
    v = gemm_values(c, 8700, dev)
    g = gen(8701, dev)
    a_all = rnd(g, nb * T, K, dev=dev)
    y = torch.full((GEMM_GUARD + nb * T + GEMM_GUARD, N), SENT16, dtype=torch.int16, device=dev)
    yv = y[GEMM_GUARD:GEMM_GUARD + nb * T].view(bf16)
    hip.gemm(a_all, v["b"], bias=v["bias"], out=yv, panels=(pr, T, T - pr, nb))
    inside = torch.arange(nb * T, device=dev).remainder(T) >= T - pr
    ref = a_all[inside].to(torch.float64) @ v["b"].to(torch.float64).t() + v["bias"].to(torch.float64)
    out.append((f"gemm row panels B{nb} T{T} N{N} K{K}: the panel rows", float(((yv[inside].to(torch.float64) - ref).norm() / ref.norm())), TOL1))
    y16 = y.clone()
    y16[GEMM_GUARD:GEMM_GUARD + nb * T][inside] = SENT16
    out.append((f"gemm row panels B{nb} T{T}: rows outside the panels and sentinel rows changed", float((y16 != SENT16).sum()), 0.0))
    return out + _gemm_rejection_rows(hip, dev)


# ---- streaming_values / streaming_layout / streaming_guards: elementwise.hip against fp64 definitions, per slice --------------------
# A value row is  max |got - ref| / (rel * |ref| + floor * scale + STREAM_TINY)  over a region, and passes at <= 1.  rel is one bf16 rounding
# (2^-8, the format's) for a bf16 output and 0 for an fp32 one; `scale` is what the op's fp32 arithmetic error is proportional to (|x| / 2 for a
# GELU value, |dy| for a derivative, sum |terms| for a sum, ...) and `floor` the class's bound on that error in units of the scale: twice the
# worst the fp32 model of tests/test_streaming_slices_cpu.py shows before its output rounding, rounded up (measured there, printed there).
# STREAM_TINY = 2^-126: fp32 arithmetic on the fast paths (v_exp_f32, v_rcp_f32) takes subnormals as zero.  Permutation rows count unequal elements.
STREAM_REL, STREAM_TINY = 2.0 ** -8, 2.0 ** -126
BF16_MAX = (2.0 - 2.0 ** -7) * 2.0 ** 127
STREAM_TOL = {      # class -> (rel, floor)
    "gelu": (STREAM_REL, 1.0e-6),        # of |x| / 2 (times |a| or |dh|): erf by Abramowitz & Stegun 7.1.26, 1.5e-7 absolute, and five roundings
    "dgelu": (STREAM_REL, 5.0e-7),       # of |dy| (|dh a|)
    "sigmoid": (STREAM_REL, 2.2e-7),     # x * sigmoid(x), x * sigmoid(1.702 x) and their derivatives
    "round": (STREAM_REL, 1.5e-7),       # one fp32 operation, one rounding: leaky ReLU, add
    "sum": (STREAM_REL, 2.0e-7),         # sumpool2, spatial_mean_bwd: against the sum of the absolute terms
    "softmax": (STREAM_REL, 6.6e-6),     # against p itself: exp(v - max) at v - max down to -87, the sum
    "embed": (STREAM_REL, 1.3e-4),       # absolute, on [-1, 1]: the angle is fp32 at up to 1000 rad
    "clip": (STREAM_REL, 4.8e-5),        # absolute, in units of 1 / std: fy = oy * sy in fp32 at up to 511
    "mean32": (0.0, 7.6e-8),             # fp32 output, against the mean of |x|
    "sumsq32": (0.0, 2.0e-7),            # fp32 output, against the sum itself
}
StreamCase = namedtuple("StreamCase", "op tag a")      # a: dict of CPU tensors and ints
_STREAM_CACHE = {}
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)


def _cg(seed):
    return torch.Generator().manual_seed(seed)


def _cr(g, *shape, scale=1.0, dtype=bf16):
    return (torch.randn(*shape, generator=g, dtype=f32) * scale).to(dtype)


def bf16_patterns():
    """all 65536 bf16 bit patterns (one tensor, a multiple of 8)"""
    return (torch.arange(65536, dtype=torch.int32) - 32768).to(torch.int16).view(bf16)


def _Phi64(x):
    return 0.5 * torch.special.erfc(-x / math.sqrt(2.0))


def _phi64(x):
    return torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def stream_ref64_unary(op, x, dy=None):
    x = x.to(f64)
    d = dy.to(f64) if dy is not None else None
    k = 1.702 if op >= 6 else 1.0
    if op in (0, 6):
        return x * torch.sigmoid(k * x)
    if op in (1, 7):
        s, ns = torch.sigmoid(k * x), torch.sigmoid(-k * x)      # 1 - s without the cancellation
        return d * s * (1.0 + k * x * ns)
    if op == 2:
        return x * _Phi64(x)
    if op == 3:
        return d * (_Phi64(x) + x * _phi64(x))
    if op == 4:
        return torch.where(x > 0, x, 0.01 * x)
    return torch.where(x > 0, d, 0.01 * d)


def stream_ref64_geglu(u, dh=None):
    H = u.shape[1] // 2
    a, g = u[:, :H].to(f64), u[:, H:].to(f64)
    out = {"h": a * g * _Phi64(g)}
    if dh is not None:
        d = dh.to(f64)
        out.update(da=d * g * _Phi64(g), dg=d * a * (_Phi64(g) + g * _phi64(g)))
    return out


def stream_ref64_softmax(x):
    x = x.to(f64)
    e = torch.exp(x - x.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def stream_ref64_timestep(t, dim):
    half = dim // 2
    ang = t.to(f64)[:, None] * torch.pow(torch.tensor(10000.0, dtype=f64), -torch.arange(half, dtype=f64) / half)[None, :]
    return torch.cat([torch.cos(ang), torch.sin(ang)], 1)


def _cubic64(d):
    """the cubic convolution kernel, A = -0.75, at distance d >= 0"""
    A = -0.75
    return torch.where(d <= 1, ((A + 2) * d - (A + 3)) * d * d + 1, ((A * d - 5 * A) * d + 8 * A) * d - 4 * A)


def stream_ref64_clip(px, S, P, Kpad):
    """bicubic (A = -0.75, align corners, clamped indices) to S x S, (x + 1) / 2, CLIP mean / std, patches [B * g * g][Kpad], k = (c * P + py) * P + px"""
    B, _, Hin, Win = px.shape
    x = px.to(f64)

    def taps(n_in):
        f = torch.arange(S, dtype=f64) * ((n_in - 1) / (S - 1) if S > 1 else 0.0)
        i0 = torch.floor(f)
        t = f - i0
        w = torch.stack([_cubic64(t + 1), _cubic64(t), _cubic64(1 - t), _cubic64(2 - t)], 1)
        idx = (i0.long()[:, None] + torch.arange(-1, 3)[None, :]).clamp(0, n_in - 1)
        return w, idx
    wy, iy = taps(Hin)
    wx, ix = taps(Win)
    rows = (x[:, :, iy, :] * wy[None, None, :, :, None]).sum(3)                 # [B][3][S][Win]
    img = (rows[:, :, :, ix] * wx[None, None, None, :, :]).sum(4)               # [B][3][S][S]
    mean, std = torch.tensor(CLIP_MEAN, dtype=f64), torch.tensor(CLIP_STD, dtype=f64)
    img = ((img + 1.0) * 0.5 - mean[None, :, None, None]) / std[None, :, None, None]
    return clip_patchify(img, P, Kpad)


def clip_patchify(img, P, Kpad):
    """[B][3][S][S] -> [B * g * g][Kpad], k = (c * P + py) * P + px, zero pad columns"""
    B, S = img.shape[0], img.shape[2]
    g = S // P
    pat = img.reshape(B, 3, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, 3 * P * P)
    return torch.nn.functional.pad(pat, (0, Kpad - 3 * P * P))


def stream_ref_conv_weight(w, Ipad, Opad):
    """fwd[o][tap][i], dgrad[i][8 - tap][o], zero in the pads; one RNE rounding"""
    O, I = w.shape[:2]
    w9 = w.reshape(O, I, 9).to(bf16)
    fwd = torch.zeros(O, 9, Ipad, dtype=bf16)
    fwd[:, :, :I] = w9.permute(0, 2, 1)
    dg = torch.zeros(I, 9, Opad, dtype=bf16)
    dg[:, :, :O] = w9.flip(2).permute(1, 2, 0)
    return fwd.reshape(O, 9 * Ipad), dg.reshape(I, 9 * Opad)


def _conv_src(Hin, Win, Hout, Wout, mode):
    """per output pixel and tap: source row, column and validity, written out plainly"""
    oy, ox = torch.arange(Hout)[:, None, None, None], torch.arange(Wout)[None, :, None, None]
    ky, kx = torch.arange(3)[None, None, :, None], torch.arange(3)[None, None, None, :]
    if mode == CONV_S1:
        iy, ix = oy + ky - 1 + 0 * ox + 0 * kx, ox + kx - 1 + 0 * oy + 0 * ky
        ok = (iy >= 0) & (iy < Hin) & (ix >= 0) & (ix < Win)
    elif mode == CONV_S2:
        iy, ix = 2 * oy + ky - 1 + 0 * ox + 0 * kx, 2 * ox + kx - 1 + 0 * oy + 0 * ky
        ok = (iy >= 0) & (iy < Hin) & (ix >= 0) & (ix < Win)
    else:      # UP2: the 3x3 window on the nearest-neighbour upsampled image
        uy, ux = oy + ky - 1 + 0 * ox + 0 * kx, ox + kx - 1 + 0 * oy + 0 * ky
        ok = (uy >= 0) & (uy < 2 * Hin) & (ux >= 0) & (ux < 2 * Win)
        iy, ix = torch.div(uy, 2, rounding_mode="floor"), torch.div(ux, 2, rounding_mode="floor")
    return iy.clamp(0, Hin - 1), ix.clamp(0, Win - 1), ok      # [Hout][Wout][3][3]


def stream_ref_im2col(x, B, Hin, Win, Hout, Wout, mode):
    """out[(b, oy, ox)][tap * C + c] = x[b][iy][ix][c], zero outside"""
    C = x.shape[1]
    iy, ix, ok = _conv_src(Hin, Win, Hout, Wout, mode)
    v = x.reshape(B, Hin, Win, C)[:, iy, ix, :]                                         # [B][Hout][Wout][3][3][C]
    v = torch.where(ok[None, ..., None], v, torch.zeros_like(v))
    return v.reshape(B * Hout * Wout, 9 * C)


def stream_ref_im2col_T(x, B, Hin, Win, Hout, Wout, mode, ld):
    m = stream_ref_im2col(x, B, Hin, Win, Hout, Wout, mode)
    return torch.nn.functional.pad(m.t(), (0, ld - m.shape[0])).contiguous()


def stream_ref_im2col3(px):
    """out[(b, y, x)][(ky * 3 + kx) * 3 + c] = px[b][c][y + ky - 1][x + kx - 1], zero outside, columns 27..31 zero; one RNE rounding"""
    B, _, H, W = px.shape
    iy, ix, ok = _conv_src(H, W, H, W, CONV_S1)
    v = px.to(bf16).permute(0, 2, 3, 1)[:, iy, ix, :]
    v = torch.where(ok[None, ..., None], v, torch.zeros_like(v))
    return torch.nn.functional.pad(v.reshape(B * H * W, 27), (0, 5))


def _padb(m, pads):
    return torch.nn.functional.pad(m.to(torch.uint8), pads).bool()


def _ring(H, W):
    m = torch.zeros(H, W, dtype=torch.bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return m


def _default_regions(shape):
    if len(shape) != 2:
        return []
    R, C = shape
    reg = []
    if R > 1:
        reg += [("first row", (slice(0, 1), slice(None))), ("last row", (slice(R - 1, R), slice(None)))]
    if C > 8:
        reg += [("first 8 columns", (slice(None), slice(0, 8))), ("last 8 columns", (slice(None), slice(C - 8, C)))]
    return reg


def stream_slices(tag, got, ref, cls, scale=None, regions=None):
    """(label, error, tolerance) for the whole output and per region.  cls "exact": the number of unequal elements against 0; else the elementwise
    measure of STREAM_TOL[cls] against 1.  regions: [(label, index)] with index a boolean mask or a tuple of slices; default first / last row and
    8-wide column chunk.  A non-finite output where the reference is finite is an infinite error."""
    if got is None or tuple(got.shape) != tuple(ref.shape):
        return [(f"{tag}: output missing or shaped {None if got is None else tuple(got.shape)}, not {tuple(ref.shape)}", float("inf"), 0.0)]
    if cls == "exact":
        r = (got != ref.to(got.dtype)).to(f64)
        tol = 0.0
    else:
        rel_, floor = STREAM_TOL[cls]
        g, rf = got.to(f64), ref.to(f64)
        den = rel_ * rf.abs() + STREAM_TINY + (floor * scale.to(f64) if scale is not None else 0.0)
        r = (g - rf).abs() / den
        # equal, both NaN, or an infinity where the reference lies beyond the largest bf16: no error; any other non-finite value: an infinite one
        same = (g == rf) | (torch.isnan(g) & torch.isnan(rf)) | (torch.isinf(g) & (rf.abs() >= BF16_MAX) & (torch.sign(g) == torch.sign(rf)) & (got.dtype == bf16))
        r = torch.where(same, torch.zeros_like(r), torch.where(torch.isfinite(g) & torch.isfinite(rf), r, torch.full_like(r, float("inf"))))
        tol = 1.0
    red = (lambda t: float(t.sum())) if cls == "exact" else (lambda t: float(t.max()) if t.numel() else 0.0)
    rows = [(f"{tag}: whole {tuple(ref.shape)}", red(r), tol)]
    for label, idx in (_default_regions(ref.shape) if regions is None else regions):
        rows.append((f"{tag}: {label}", red(r[idx]), tol))
    return rows


def stream_excess(pre, ref, scale):
    """the fp32 arithmetic error of an unrounded output in units of its scale: what a class's floor bounds"""
    p, rf, s = pre.to(f64), ref.to(f64), scale.to(f64)
    ok = torch.isfinite(p) & torch.isfinite(rf) & (s > 0)
    d = torch.where(ok, ((p - rf).abs() - STREAM_TINY).clamp(min=0.0) / torch.where(ok, s, torch.ones_like(s)), torch.zeros_like(rf))      # (a subnormal fp32 result has no relative precision: STREAM_TINY is its bound)
    return float(d.max()) if d.numel() else 0.0


# ---- the cases: inputs drawn on the CPU, once -------------------------------------------------------------------------------------------
SOFTMAX_ROWS = {8: ("seeded", "peaked", "some -inf"), 64: ("seeded", "constant", "offset 3e4"), 2056: ("seeded", "peaked", "some -inf"),
                16384: ("seeded", "constant", "offset 3e4")}
TIMESTEPS, TIMESTEP_DIMS = (0, 1, 17, 500, 999, 1000), (2, 6, 320, 322, 1280)
SUMSQ_N, SUMSQ_BLOCKS = (1, 255, 257, 100003), (1, 1024)
GEGLU_SHAPES = [(1, 8), (3, 72), (300, 640)]
TRANSPOSE_CASES = [(1, 1, 0), (3, 65, 1), (63, 64, 0), (64, 63, 1), (65, 130, 0), (130, 72, 0)]      # R, C, ldi - C
CONV_WEIGHT_CASES = [(4, 320, None, None), (320, 4, None, None), (72, 200, 256, 128), (8, 8, 8, 8)]      # O, I, Ipad, Opad
SUMPOOL_CASES = [(3, 1, 1, 8), (2, 5, 3, 72), (1, 8, 8, 64)]
IM2COL_GEOM = [(CONV_S1, 2, 6, 10, 6, 10), (CONV_S2, 2, 7, 9, 4, 5), (CONV_UP2, 1, 3, 5, 6, 10),
               (CONV_S1, 2, 12, 12, 12, 12), (CONV_S2, 3, 9, 9, 5, 5), (CONV_UP2, 2, 6, 6, 12, 12)]      # mode, B, Hin, Win, Hout, Wout; the last three: check_streaming's
IM2COL3_CASES = [(1, 1, 1), (2, 5, 3)]
SPATIAL_MEAN_CASES = [(1, 1, 4, 4, 0, 0.0), (2, 63, 68, 68, 0, 0.0), (3, 65, 132, 200, 60, 0.0), (2, 4096, 320, 320, 0, 0.0), (2, 63, 68, 68, 0, 100.0)]      # B, HW, C, ldo, coff, mean
SPATIAL_BWD_CASES = [(2, 5, 8, 8, 0, False), (2, 5, 8, 8, 0, True), (2, 5, 8, 24, 8, True), (3, 7, 16, 40, 16, False)]      # B, HW, C, ldg, coff, base
CLIP_CASES = [("identity 28->28", 1, 28, 28, 28, 14, 588, "rand"), ("enlarging 20x20->28", 2, 20, 20, 28, 14, 640, "rand"), ("48x80->28", 1, 48, 80, 28, 14, 640, "rand"),
              ("64->28 S == P", 1, 64, 64, 28, 28, 3 * 28 * 28, "rand"), ("512->224", 1, 512, 512, 224, 14, 640, "rand"),
              ("constant 48x80->28", 1, 48, 80, 28, 14, 588, "constant"), ("ramp 48x80->28", 1, 48, 80, 28, 14, 640, "ramp")]


def softmax_rows_input(L, kinds, g):
    x = _cr(g, len(kinds), L, scale=2.0).float()
    for r, kind in enumerate(kinds):
        if kind == "peaked":
            x[r, (7 * L) // 11] += 40.0
        elif kind == "constant":
            x[r] = 1.25
        elif kind == "offset 3e4":
            x[r] += 3.0e4
        elif kind == "some -inf":
            x[r, ::3] = float("-inf")
    return x.to(bf16)


def stream_value_cases():
    if "values" in _STREAM_CACHE:
        return _STREAM_CACHE["values"]
    cases, g = [], _cg(3100)
    pat = bf16_patterns()
    fin = pat[torch.isfinite(pat.float())]      # 65280 = 8160 * 8
    for op in range(8):
        cases.append(StreamCase("unary", f"unary op{op}, every bf16 pattern" + (", dy = 1" if op & 1 else ""), dict(op=op, x=pat, dy=torch.ones_like(pat) if op & 1 else None)))
        if op & 1:
            cases.append(StreamCase("unary", f"unary op{op}, every bf16 pattern, seeded dy", dict(op=op, x=pat, dy=_cr(g, pat.numel()))))
    u = torch.cat([_cr(g, fin.numel() // 8, 8), fin.reshape(-1, 8)], 1)
    cases.append(StreamCase("geglu", "geglu gate = every finite bf16 pattern, H8", dict(u=u, dh=_cr(g, fin.numel() // 8, 8))))
    for M, H in GEGLU_SHAPES:
        cases.append(StreamCase("geglu", f"geglu {M}x{H}", dict(u=_cr(g, M, 2 * H, scale=2.0), dh=_cr(g, M, H))))
    a = _cr(g, 37, 72)
    cases.append(StreamCase("add", "add seeded", dict(a=a, b=_cr(g, 37, 72))))
    cases.append(StreamCase("add", "add a = -b", dict(a=a, b=-a)))
    cases.append(StreamCase("add", "add magnitudes 2^16 apart", dict(a=a, b=(_cr(g, 37, 72).float() * 2.0 ** -16).to(bf16))))
    for L, kinds in SOFTMAX_ROWS.items():
        cases.append(StreamCase("softmax", f"softmax_rows L{L}", dict(x=softmax_rows_input(L, kinds, g), kinds=kinds)))
    for dim in TIMESTEP_DIMS:
        cases.append(StreamCase("timestep", f"timestep_embedding dim{dim}", dict(t=torch.tensor(TIMESTEPS), dim=dim)))
    for n in SUMSQ_N:
        cases.append(StreamCase("sumsq", f"sumsq n{n}", dict(g=_cr(g, n, dtype=f32))))
    _STREAM_CACHE["values"] = cases
    return cases


def clip_input(kind, B, Hin, Win, g):
    if kind == "constant":
        return torch.full((B, 3, Hin, Win), 0.3125)
    if kind == "ramp":      # linear in y and x, another slope per channel: cubic convolution reproduces degree 1 away from the clamped border
        y, x = torch.arange(Hin, dtype=f32)[:, None] / Hin, torch.arange(Win, dtype=f32)[None, :] / Win
        return torch.stack([0.9 * y - 0.7 * x, x - 0.5 * y - 0.2, 0.3 * y + 0.4 * x - 0.6], 0)[None].repeat(B, 1, 1, 1).contiguous()
    return torch.rand(B, 3, Hin, Win, generator=g) * 2 - 1


def stream_layout_cases():
    if "layout" in _STREAM_CACHE:
        return _STREAM_CACHE["layout"]
    cases, g = [], _cg(3200)
    for R, C, pad in TRANSPOSE_CASES:
        cases.append(StreamCase("transpose", f"transpose {R}x{C}" + (f" ldi {C + pad}" if pad else ""), dict(x=_cr(g, R, C + pad)[:, :C])))
    for O, I, Ipad, Opad in CONV_WEIGHT_CASES:
        w = _cr(g, O, I, 3, 3, scale=0.05, dtype=f32)
        for form, (wf, wd) in (("fwd only", (True, False)), ("dgrad only", (False, True)), ("both", (True, True))):
            cases.append(StreamCase("conv_weight", f"conv_weight_prepare {I}->{O} pads {Ipad}/{Opad} {form}", dict(w=w, Ipad=Ipad, Opad=Opad, fwd=wf, dgrad=wd)))
    for B, H, W, C in SUMPOOL_CASES:
        cases.append(StreamCase("sumpool2", f"sumpool2 B{B} {H}x{W} C{C}", dict(x=_cr(g, B * 2 * H * 2 * W, C), B=B, H=H, W=W)))
    for i, (mode, B, Hin, Win, Hout, Wout) in enumerate(IM2COL_GEOM):
        for C in ((8, 72, 4) if i < 3 else (72,)):
            geo = dict(x=_cr(g, B * Hin * Win, C), B=B, Hin=Hin, Win=Win, Hout=Hout, Wout=Wout, mode=mode)
            tag = f"mode{mode} B{B} {Hin}x{Win}->{Hout}x{Wout} C{C}"
            if C % 8 == 0:
                cases.append(StreamCase("im2col", "im2col " + tag, geo))
            cases.append(StreamCase("im2col_T", "im2col_T " + tag, geo))
    for B, H, W in IM2COL3_CASES:
        cases.append(StreamCase("im2col3", f"im2col3_rgb B{B} {H}x{W}", dict(px=torch.rand(B, 3, H, W, generator=g) * 2 - 1)))
    for B, HW, C, ldo, coff, mean in SPATIAL_MEAN_CASES:
        cases.append(StreamCase("spatial_mean", f"spatial_mean B{B} HW{HW} C{C} ldo{ldo} coff{coff}" + (f" mean {mean:g}" if mean else ""),
                                dict(x=(torch.randn(B * HW, C, generator=g) + mean).to(bf16), B=B, HW=HW, ldo=ldo, coff=coff)))
    for B, HW, C, ldg, coff, base in SPATIAL_BWD_CASES:
        cases.append(StreamCase("spatial_mean_bwd", f"spatial_mean_bwd B{B} HW{HW} C{C} ldg{ldg} coff{coff}" + (" + base" if base else ""),
                                dict(g=_cr(g, B, ldg, dtype=f32), base=_cr(g, B * HW, C) if base else None, B=B, HW=HW, C=C, coff=coff)))
    for name, B, Hin, Win, S, P, Kpad, kind in CLIP_CASES:
        cases.append(StreamCase("clip", f"clip_preprocess {name} P{P} Kpad{Kpad}", dict(px=clip_input(kind, B, Hin, Win, g), S=S, P=P, Kpad=Kpad, kind=kind)))
    _STREAM_CACHE["layout"] = cases
    return cases


def _pixel_regions(mask_hw, expand):
    """border ring / interior of the output pixels; expand: [H][W] mask -> mask of the output's shape"""
    reg = [("border ring", expand(mask_hw))]
    if bool((~mask_hw).any()):
        reg.append(("interior", expand(~mask_hw)))
    return reg


def stream_ref64(case):
    """{output name: (class, fp64 reference or the exact expected tensor, scale or None, regions or None)} of a case, from the definition"""
    if case.tag in _STREAM_CACHE:
        return _STREAM_CACHE[case.tag]
    a, op = case.a, case.op
    if op == "unary":
        x, dy, o = a["x"], a["dy"], a["op"]
        fin = torch.isfinite(x.float())
        ref = stream_ref64_unary(o, x, dy)
        xa, da = x.to(f64).abs(), (dy.to(f64).abs() if dy is not None else None)
        if dy is not None:
            dx = da * (1.0 + xa)      # s * (1 + x * (1 - s)): the rounding of 1 - s is multiplied by x
        cls, scale = {0: ("sigmoid", xa), 1: ("sigmoid", dx if o == 1 else None), 2: ("gelu", xa / 2), 3: ("dgelu", da), 4: ("round", ref.abs()), 5: ("round", ref.abs()),
                      6: ("sigmoid", xa), 7: ("sigmoid", dx if o == 7 else None)}[o]
        xf = x.float()[fin]      # the rows are over the finite patterns; stream_rows() looks at the others
        out = {"y": (cls, ref[fin], scale[fin], [("x < -4", xf < -4), ("x > 4", xf > 4), ("|x| <= 4", xf.abs() <= 4), ("|x| < 2^-100", xf.abs() < 2.0 ** -100)])}
    elif op == "geglu":
        H = a["u"].shape[1] // 2
        r = stream_ref64_geglu(a["u"], a["dh"])
        A, G, D = a["u"][:, :H].to(f64).abs(), a["u"][:, H:].to(f64).abs(), a["dh"].to(f64).abs()
        out = {"h": ("gelu", r["h"], A * G / 2, None), "da": ("gelu", r["da"], D * G / 2, None), "dg": ("dgelu", r["dg"], D * A, None)}
    elif op == "add":
        s = a["a"].to(f64) + a["b"].to(f64)
        out = {"y": ("round", s, s.abs(), None)}
    elif op == "softmax":
        p = stream_ref64_softmax(a["x"])
        out = {"p": ("softmax", p, p, [(f"row {r} ({k})", (slice(r, r + 1), slice(None))) for r, k in enumerate(a["kinds"])])}
    elif op == "timestep":
        e, half = stream_ref64_timestep(a["t"], a["dim"]), a["dim"] // 2
        reg = [("cos half", (slice(None), slice(0, half))), ("sin half", (slice(None), slice(half, None)))]
        reg += [(f"t = {int(t)}", (slice(b, b + 1), slice(None))) for b, t in enumerate(a["t"])]
        out = {"emb": ("embed", e, torch.ones_like(e), reg)}
    elif op == "sumsq":
        s = (a["g"].to(f64) ** 2).sum().reshape(1)
        out = {"sum": ("sumsq32", s, s, [])}
    elif op == "transpose":
        out = {"y": ("exact", a["x"].t().contiguous(), None, None)}
    elif op == "conv_weight":
        O, I = a["w"].shape[:2]
        f, d = stream_ref_conv_weight(a["w"], a["Ipad"] or (I + 63) // 64 * 64, a["Opad"] or (O + 63) // 64 * 64)
        out = {}
        if a["fwd"]:
            out["fwd"] = ("exact", f, None, None)
        if a["dgrad"]:
            out["dgrad"] = ("exact", d, None, None)
    elif op == "sumpool2":
        B, H, W, C = a["B"], a["H"], a["W"], a["x"].shape[1]
        x = a["x"].to(f64).reshape(B, H, 2, W, 2, C)
        ex = lambda m: m[None, :, :, None].expand(B, H, W, C).reshape(B * H * W, C)
        out = {"y": ("sum", x.sum((2, 4)).reshape(B * H * W, C), x.abs().sum((2, 4)).reshape(B * H * W, C), _pixel_regions(_ring(H, W), ex))}
    elif op in ("im2col", "im2col_T"):
        B, Ho, Wo, C = a["B"], a["Hout"], a["Wout"], a["x"].shape[1]
        ring = _ring(Ho, Wo)
        if op == "im2col":
            ref = stream_ref_im2col(a["x"], B, a["Hin"], a["Win"], Ho, Wo, a["mode"])
            ex = lambda m: m[None, :, :, None].expand(B, Ho, Wo, 9 * C).reshape(B * Ho * Wo, 9 * C)
        else:
            ld = (B * Ho * Wo + 7) // 8 * 8
            ref = stream_ref_im2col_T(a["x"], B, a["Hin"], a["Win"], Ho, Wo, a["mode"], ld)
            ex = lambda m: _padb(m[None].expand(B, Ho, Wo).reshape(1, -1).expand(9 * C, -1), (0, ld - B * Ho * Wo))
        out = {"y": ("exact", ref, None, _pixel_regions(ring, ex))}
    elif op == "im2col3":
        B, _, H, W = a["px"].shape
        ex = lambda m: m[None, :, :, None].expand(B, H, W, 32).reshape(B * H * W, 32)
        out = {"y": ("exact", stream_ref_im2col3(a["px"]), None, _pixel_regions(_ring(H, W), ex))}
    elif op == "spatial_mean":
        B, HW, C = a["B"], a["HW"], a["x"].shape[1]
        x = a["x"].to(f64).reshape(B, HW, C)
        reg = [(f"image {b}", (slice(b, b + 1), slice(None))) for b in range(B)] + [(f"channels {c}-{min(c + 64, C) - 1}", (slice(None), slice(c, c + 64))) for c in range(0, C, 64)]
        out = {"mean": ("mean32", x.mean(1), x.abs().mean(1), reg)}
    elif op == "spatial_mean_bwd":
        B, HW, C, coff = a["B"], a["HW"], a["C"], a["coff"]
        gs = (a["g"].to(f64)[:, coff:coff + C] / HW)[:, None, :].expand(B, HW, C).reshape(B * HW, C)
        bs = a["base"].to(f64) if a["base"] is not None else torch.zeros_like(gs)
        out = {"dx": ("sum", bs + gs, bs.abs() + gs.abs(), None)}
    elif op == "clip":
        B, _, Hin, Win = a["px"].shape
        S, P, Kpad = a["S"], a["P"], a["Kpad"]
        gp, k3 = S // P, 3 * P * P
        ref = stream_ref64_clip(a["px"], S, P, Kpad)

        def ex(m):      # [S][S] pixel mask -> [B * g * g][Kpad]
            mm = m[None, None].expand(B, 3, S, S).reshape(B, 3, gp, P, gp, P).permute(0, 2, 4, 1, 3, 5).reshape(B * gp * gp, k3)
            return _padb(mm, (0, Kpad - k3))
        ring = ~_padb(torch.ones(S - 4, S - 4, dtype=torch.bool), (2, 2, 2, 2))      # two pixels wide: the rows and columns whose window can reach past the image
        reg = _pixel_regions(ring, ex)
        if Kpad > k3:
            reg.append(("pad columns (zero)", (slice(None), slice(k3, Kpad))))
        out = {"patches": ("clip", ref, torch.full_like(ref, 1.0 / min(CLIP_STD)), reg)}
    _STREAM_CACHE[case.tag] = out
    return out


def stream_rows(case, got, ref=None):
    """the rows of one case: got = {output name: tensor on the CPU}"""
    rows = []
    for name, (cls, rf, scale, reg) in (ref or stream_ref64(case)).items():
        g = got.get(name)
        if case.op == "unary" and g is not None:
            g = g[torch.isfinite(case.a["x"].float())]
        rows += stream_slices(f"{case.tag} {name}", g, rf, cls, scale, reg)
    if case.op == "unary":      # the non-finite patterns: NaN gives NaN (leaky ReLU backward: what `x > 0` false gives), no finite x a non-finite y
        x, y, o = case.a["x"].float(), got["y"].float(), case.a["op"]
        want_nan = torch.isnan(stream_ref64_unary(o, case.a["x"], case.a["dy"]))
        rows.append((f"{case.tag}: NaN patterns that do not give NaN", float((torch.isnan(x) & want_nan & ~torch.isnan(y)).sum()), 0.0))
        rows.append((f"{case.tag}: finite patterns that give a non-finite value", float((torch.isfinite(x) & ~torch.isfinite(y)).sum()), 0.0))
    if case.op == "clip" and case.a["kind"] == "rand" and case.tag.startswith("clip_preprocess identity"):
        px = case.a["px"]      # the identity resize: the normalised input, rounded once (the fp32 expression of the kernel: every step is one IEEE operation)
        img = ((px + 1.0) * 0.5 - torch.tensor(CLIP_MEAN)[None, :, None, None]) / torch.tensor(CLIP_STD)[None, :, None, None]
        B, S, P = px.shape[0], case.a["S"], case.a["P"]
        want = img.reshape(B, 3, S // P, P, S // P, P).permute(0, 2, 4, 1, 3, 5).reshape(-1, 3 * P * P).to(bf16)
        rows.append((f"{case.tag}: elements that are not the normalised input rounded once", float((got["patches"][:, :3 * P * P] != want).sum()), 0.0))
    return rows


def stream_run(hip, case, dev):
    """the case through e4t.ops on the GPU -> {output name: CPU tensor}"""
    a, op = case.a, case.op
    d = lambda t: None if t is None else t.to(dev)
    if op == "unary":
        return {"y": hip.unary(d(a["x"]), a["op"], d(a["dy"])).cpu()}
    if op == "geglu":
        u, H = d(a["u"]), a["u"].shape[1] // 2
        du = hip.geglu_bwd(u, d(a["dh"])).cpu()
        return {"h": hip.geglu_fwd(u).cpu(), "da": du[:, :H], "dg": du[:, H:]}
    if op == "add":
        return {"y": hip.add(d(a["a"]), d(a["b"])).cpu()}
    if op == "softmax":
        return {"p": hip.softmax_rows_(d(a["x"]).clone()).cpu()}
    if op == "timestep":
        return {"emb": hip.timestep_embedding(d(a["t"]), a["dim"]).cpu()}
    if op == "sumsq":
        return {"sum": hip.sumsq(d(a["g"])).reshape(1).cpu()}
    if op == "transpose":
        R, C = a["x"].shape
        xb = torch.zeros(R, a["x"].stride(0), dtype=bf16, device=dev)      # the case's row stride (ldi = C + 1 for two of them)
        xb[:, :C] = d(a["x"])
        return {"y": hip.transpose(xb[:, :C]).cpu()}
    if op == "conv_weight":
        f, g = hip.conv_weight_prepare(d(a["w"]), a["Ipad"], a["Opad"], want_fwd=a["fwd"], want_dgrad=a["dgrad"])
        return {k: v.cpu() for k, v in (("fwd", f), ("dgrad", g)) if v is not None}
    if op == "sumpool2":
        return {"y": hip.sumpool2(d(a["x"]), a["B"], a["H"], a["W"]).cpu()}
    if op in ("im2col", "im2col_T"):
        fn = hip.im2col if op == "im2col" else hip.im2col_T
        return {"y": fn(d(a["x"]), a["B"], a["Hin"], a["Win"], a["Hout"], a["Wout"], a["mode"]).cpu()}
    if op == "im2col3":
        return {"y": hip.im2col3_rgb(d(a["px"])).cpu()}
    if op == "spatial_mean":
        C = a["x"].shape[1]
        out = torch.full((a["B"], a["ldo"]), float("nan"), dtype=f32, device=dev)
        hip.spatial_mean(d(a["x"]), a["B"], a["HW"], out, a["coff"])
        return {"mean": out[:, a["coff"]:a["coff"] + C].cpu()}
    if op == "spatial_mean_bwd":
        return {"dx": hip.spatial_mean_bwd(d(a["g"]), d(a["base"]), a["B"], a["HW"], a["C"], a["coff"]).cpu()}
    if op == "clip":
        return {"patches": hip.clip_preprocess(d(a["px"]), a["S"], a["P"], a["Kpad"]).cpu()}
    raise KeyError(op)


def _sumsq_raw_rows(hip, case, dev):
    """e4t_sumsq_partial through the ABI: partial NaN-filled first, nblocks = 1 and 1024 (n = 1: 1023 blocks without an element must still write 0)"""
    from e4t.ops import _stream, _ptr
    rows = []
    g = case.a["g"].to(dev)
    cls, ref, scale, _ = stream_ref64(case)["sum"]
    for nb in SUMSQ_BLOCKS:
        part = torch.full((nb,), float("nan"), dtype=f32, device=dev)
        code = hip.lib.e4t_sumsq_partial(_ptr(g), g.numel(), _ptr(part), nb, _stream())
        torch.cuda.synchronize()
        rows.append((f"{case.tag} nblocks {nb}: return code", float(code), 0.0))
        rows.append((f"{case.tag} nblocks {nb}: NaN left in partial", float(torch.isnan(part).sum()), 0.0))
        rows += stream_slices(f"{case.tag} nblocks {nb}: sum of the partials", part.to(f64).sum().reshape(1).cpu(), ref, cls, scale, [])
    return rows


def check_streaming_values(hip, emu, dev):
    """the activation, softmax, embedding and sum-of-squares kernels against their fp64 definitions on CPU-drawn inputs: every bf16 bit pattern
    through the eight unary ops and the GEGLU gate, saturating and cancelling rows, per-region elementwise errors (stream_slices)"""
    out = []
    for case in stream_value_cases():
        out += stream_rows(case, stream_run(hip, case, dev))
        if case.op == "sumsq":
            out += _sumsq_raw_rows(hip, case, dev)
    return out


def check_streaming_layout(hip, emu, dev):
    """the layout, pooling and preprocessing kernels on non-square and ragged shapes: permutations exact against plainly written index
    arithmetic, sums and the bicubic resize against fp64, border ring and interior apart"""
    out = []
    for case in stream_layout_cases():
        out += stream_rows(case, stream_run(hip, case, dev))
    return out


# ---- streaming_guards: the raw ABI, exactly sized buffers between sentinel bands; no out-of-range argument anywhere ---------------------
def _left(view):
    """16-bit words of an output region that still hold the sentinel (poison the kernel should have overwritten)"""
    if view.dtype == bf16:
        return int((view.contiguous().view(torch.int16) == SENT16).sum())
    return int((view.contiguous().view(torch.int32) == SENT16 * 0x10001).sum())      # an fp32 word of a _Guarded buffer: the 16-bit sentinel twice


def _guard_rows(tag, code, outs, values):
    """outs: [(a _Guarded, the view of what the kernel owns or None = all of it)]; values: rows"""
    torch.cuda.synchronize()
    rows = [(f"{tag}: return code", float(code), 0.0),
            (f"{tag}: sentinel words changed around the outputs", float(sum(o.outside() for o, _ in outs)), 0.0),
            (f"{tag}: poison left in what the kernel owns", float(sum(_left(o.view if own is None else own) for o, own in outs)), 0.0)]
    return rows + values


def check_streaming_guards(hip, emu, dev):
    """every entry point of the family through the C ABI: outputs exactly sized inside sentinel bands and poisoned, inputs between rows of NaN;
    per kernel the return code, sentinel words changed (0), poison left in what the kernel owns (0), and the values against fp64.  Strides,
    offsets and pads no e4t.ops call passes: transpose batches with gaps and ldo > R, softmax ld > L, spatial_mean coff / ldo, clip_preprocess
    Kpad > 3 P^2 (the kernel leaves the pad alone; ops.clip_preprocess zeroes it), im2col_T ldo rounded up (zero fill)."""
    from e4t.ops import _stream, _ptr
    lib, out, st = hip.lib, [], _stream()
    g = _cg(3300)
    keep = []      # every device input stays referenced until the rows are read: a temporary's memory would be handed to the next allocation

    def d(t):
        keep.append(t.to(dev))
        return keep[-1]

    def wrapped(t):
        keep.append(_nan_wrapped(d(t)))
        return keep[-1]
    val = lambda tag, got, ref, cls, scale=None: stream_slices(tag, got.cpu(), ref, cls, scale, [])
    # geglu, unary, add: exactly sized outputs
    M, H = 37, 72
    u, dh = _cr(g, M, 2 * H), _cr(g, M, H)
    r = stream_ref64_geglu(u, dh)
    A, G, D = u[:, :H].to(f64).abs(), u[:, H:].to(f64).abs(), dh.to(f64).abs()
    ug, dhg = wrapped(u), wrapped(dh)
    h = _Guarded(M, H, bf16, dev)
    code = lib.e4t_geglu_fwd(_ptr(ug), h.ptr, M, H, st)
    out += _guard_rows("geglu_fwd 37x72 guarded", code, [(h, None)], val("geglu_fwd guarded h", h.view, r["h"], "gelu", A * G / 2))
    du = _Guarded(M, 2 * H, bf16, dev)
    code = lib.e4t_geglu_bwd(_ptr(ug), _ptr(dhg), du.ptr, M, H, st)
    out += _guard_rows("geglu_bwd 37x72 guarded", code, [(du, None)],
                       val("geglu_bwd guarded da", du.view[:, :H], r["da"], "gelu", D * G / 2) + val("geglu_bwd guarded dg", du.view[:, H:], r["dg"], "dgelu", D * A))
    x, dy = _cr(g, M, H), _cr(g, M, H)
    xg, dyg = wrapped(x), wrapped(dy)
    for op, cls, scale in ((0, "sigmoid", x.to(f64).abs()), (3, "dgelu", dy.to(f64).abs())):
        y = _Guarded(M, H, bf16, dev)
        code = lib.e4t_unary(_ptr(xg), _ptr(dyg) if op & 1 else None, y.ptr, M * H, op, st)
        out += _guard_rows(f"unary op{op} 37x72 guarded", code, [(y, None)], val(f"unary op{op} guarded y", y.view, stream_ref64_unary(op, x, dy), cls, scale))
    y = _Guarded(M, H, bf16, dev)
    code = lib.e4t_add(_ptr(xg), _ptr(dyg), y.ptr, M * H, st)
    s = x.to(f64) + dy.to(f64)
    out += _guard_rows("add 37x72 guarded", code, [(y, None)], val("add guarded y", y.view, s, "round", s.abs()))
    # transpose: three images with sentinel gaps between them, ldo = R + 8
    nb, R, C, gap = 3, 37, 70, 5
    xs = _cr(g, nb, R, C)
    xin = torch.full((nb * (R + gap), C + 2), float("nan"), dtype=bf16, device=dev)
    for b in range(nb):
        xin[b * (R + gap):b * (R + gap) + R, :C] = d(xs[b])
    y = _Guarded(nb * (C + gap), R + 8, bf16, dev)
    code = lib.e4t_transpose(_ptr(xin), y.ptr, nb, R, C, C + 2, R + 8, (R + gap) * (C + 2), (C + gap) * (R + 8), st)
    torch.cuda.synchronize()
    yb = y.view.reshape(nb, C + gap, R + 8)
    own = yb[:, :C, :R]
    rest = yb.contiguous().view(torch.int16).clone()
    rest[:, :C, :R] = SENT16
    out += _guard_rows(f"transpose batch {nb} {R}x{C} ldo {R + 8}, gaps of {gap} rows, guarded", code, [(y, own)],
                       [("transpose guarded: pad columns and gap rows changed", float((rest != SENT16).sum()), 0.0)] + val("transpose guarded y", own, xs.transpose(1, 2), "exact"))
    # softmax_rows in place with ld = L + 8: the gap columns bitwise unchanged
    rows_, L = 3, 2056
    xs = softmax_rows_input(L, SOFTMAX_ROWS[L], g)
    y = _Guarded(rows_, L + 8, bf16, dev)
    y.view[:, :L] = d(xs)
    code = lib.e4t_softmax_rows(y.ptr, rows_, L, L + 8, st)
    p = stream_ref64_softmax(xs)
    out += _guard_rows(f"softmax_rows {rows_}x{L} ld {L + 8} guarded", code, [(y, y.view[:, :L])],
                       [("softmax_rows guarded: gap columns changed", float((y.view[:, L:].contiguous().view(torch.int16) != SENT16).sum()), 0.0)] + val("softmax_rows guarded p", y.view[:, :L], p, "softmax", p))
    # spatial_mean into a column slice; spatial_mean_bwd out of one
    B, HW, C, ldo, coff = 3, 65, 132, 200, 60
    xs = _cr(g, B * HW, C)
    o = _Guarded(B, ldo, f32, dev)
    code = lib.e4t_spatial_mean(_ptr(wrapped(xs)), o.ptr, B, HW, C, ldo, coff, st)
    torch.cuda.synchronize()
    side = torch.cat([o.view[:, :coff], o.view[:, coff + C:]], 1).contiguous().view(torch.int16)
    x64 = xs.to(f64).reshape(B, HW, C)
    out += _guard_rows(f"spatial_mean B{B} HW{HW} C{C} ldo{ldo} coff{coff} guarded", code, [(o, o.view[:, coff:coff + C])],
                       [("spatial_mean guarded: columns left and right changed", float((side != SENT16).sum()), 0.0)] + val("spatial_mean guarded mean", o.view[:, coff:coff + C], x64.mean(1), "mean32", x64.abs().mean(1)))
    B, HW, C, ldg, coff = 2, 5, 8, 24, 8
    gs = torch.full((B, ldg), float("nan"), dtype=f32)
    gs[:, coff:coff + C] = _cr(g, B, C, dtype=f32)
    base = _cr(g, B * HW, C)
    dx = _Guarded(B * HW, C, bf16, dev)
    code = lib.e4t_spatial_mean_bwd(_ptr(d(gs)), _ptr(wrapped(base)), dx.ptr, B, HW, C, ldg, coff, st)
    gq = (gs.to(f64)[:, coff:coff + C] / HW)[:, None, :].expand(B, HW, C).reshape(B * HW, C)
    out += _guard_rows(f"spatial_mean_bwd B{B} HW{HW} C{C} ldg{ldg} coff{coff} guarded (NaN beside the slice of g)", code, [(dx, None)],
                       val("spatial_mean_bwd guarded dx", dx.view, base.to(f64) + gq, "sum", base.to(f64).abs() + gq.abs()))
    # sumpool2, im2col, im2col_T (ldo rounded up: zero fill), im2col3_rgb, conv_weight_prepare
    B, H, W, C = 2, 5, 3, 72
    xs = _cr(g, B * 2 * H * 2 * W, C)
    y = _Guarded(B * H * W, C, bf16, dev)
    code = lib.e4t_sumpool2(_ptr(wrapped(xs)), y.ptr, B, H, W, C, st)
    x6 = xs.to(f64).reshape(B, H, 2, W, 2, C)
    out += _guard_rows(f"sumpool2 B{B} {H}x{W} C{C} guarded", code, [(y, None)], val("sumpool2 guarded y", y.view, x6.sum((2, 4)).reshape(-1, C), "sum", x6.abs().sum((2, 4)).reshape(-1, C)))
    mode, B, Hin, Win, Hout, Wout, C = CONV_S2, 1, 7, 9, 4, 5, 72      # 20 output pixels: ldo = 24 leaves four pad columns
    xs = _cr(g, B * Hin * Win, C)
    xg = wrapped(xs)
    Mpix, ld = B * Hout * Wout, (B * Hout * Wout + 7) // 8 * 8
    y = _Guarded(Mpix, 9 * C, bf16, dev)
    code = lib.e4t_im2col(_ptr(xg), y.ptr, B, Hin, Win, C, Hout, Wout, mode, st)
    out += _guard_rows(f"im2col mode{mode} {Hin}x{Win}->{Hout}x{Wout} C{C} guarded", code, [(y, None)], val("im2col guarded y", y.view, stream_ref_im2col(xs, B, Hin, Win, Hout, Wout, mode), "exact"))
    y = _Guarded(9 * C, ld, bf16, dev)
    code = lib.e4t_im2col_T(_ptr(xg), y.ptr, B, Hin, Win, C, Hout, Wout, ld, mode, st)
    out += _guard_rows(f"im2col_T mode{mode} {Hin}x{Win}->{Hout}x{Wout} C{C} ldo {ld} (Mpix {Mpix}) guarded", code, [(y, None)],
                       val("im2col_T guarded y, columns [Mpix, ldo) zero", y.view, stream_ref_im2col_T(xs, B, Hin, Win, Hout, Wout, mode, ld), "exact"))
    B, H, W = 2, 5, 3
    px = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    y = _Guarded(B * H * W, 32, bf16, dev)
    code = lib.e4t_im2col3_rgb(_ptr(wrapped(px)), y.ptr, B, H, W, st)
    out += _guard_rows(f"im2col3_rgb B{B} {H}x{W} guarded", code, [(y, None)], val("im2col3_rgb guarded y", y.view, stream_ref_im2col3(px), "exact"))
    O, I, Ipad, Opad = 72, 200, 256, 128
    w = _cr(g, O, I, 3, 3, scale=0.05, dtype=f32)
    f_ref, d_ref = stream_ref_conv_weight(w, Ipad, Opad)
    wg = wrapped(w)
    for form in ("fwd only", "dgrad only", "both"):
        wf = _Guarded(O, 9 * Ipad, bf16, dev) if form != "dgrad only" else None
        wd = _Guarded(I, 9 * Opad, bf16, dev) if form != "fwd only" else None
        code = lib.e4t_conv_weight_prepare(_ptr(wg), wf.ptr if wf else None, wd.ptr if wd else None, O, I, Ipad, Opad, st)
        vals = (val("conv_weight_prepare guarded fwd", wf.view, f_ref, "exact") if wf else []) + (val("conv_weight_prepare guarded dgrad", wd.view, d_ref, "exact") if wd else [])
        out += _guard_rows(f"conv_weight_prepare {I}->{O} pads {Ipad}/{Opad} {form} guarded", code, [(b, None) for b in (wf, wd) if b], vals)
    # clip_preprocess, Kpad > 3 P^2: through the ABI the pad columns keep the sentinel; through e4t.ops they are zero
    B, Hin, Win, S, P, Kpad = 1, 48, 80, 28, 14, 640
    px = torch.rand(B, 3, Hin, Win, generator=g) * 2 - 1
    ref = stream_ref64_clip(px, S, P, Kpad)
    k3, gp = 3 * P * P, S // P
    y = _Guarded(B * gp * gp, Kpad, bf16, dev)
    code = lib.e4t_clip_preprocess(_ptr(wrapped(px)), y.ptr, B, Hin, Win, S, P, Kpad, st)
    out += _guard_rows(f"clip_preprocess {Hin}x{Win}->{S} P{P} Kpad{Kpad} guarded", code, [(y, y.view[:, :k3])],
                       [("clip_preprocess guarded: pad columns changed by the kernel", float((y.view[:, k3:].contiguous().view(torch.int16) != SENT16).sum()), 0.0)]
                       + val("clip_preprocess guarded patches", y.view[:, :k3], ref[:, :k3], "clip", torch.full_like(ref[:, :k3], 1.0 / min(CLIP_STD))))
    got = hip.clip_preprocess(d(px), S, P, Kpad)
    out.append(("clip_preprocess through e4t.ops: nonzero words in the pad columns", float((got[:, k3:].contiguous().view(torch.int16) != 0).sum()), 0.0))
    # timestep_embedding and sumsq_partial: exactly sized
    t = torch.tensor(TIMESTEPS)
    e = _Guarded(len(TIMESTEPS), 322, bf16, dev)
    code = lib.e4t_timestep_embedding(_ptr(d(t)), e.ptr, len(TIMESTEPS), 322, st)
    e64 = stream_ref64_timestep(t, 322)
    out += _guard_rows("timestep_embedding B6 dim322 guarded", code, [(e, None)], val("timestep_embedding guarded emb", e.view, e64, "embed", torch.ones_like(e64)))
    gv = _cr(g, 257, dtype=f32)
    part = _Guarded(1, 1024, f32, dev)
    code = lib.e4t_sumsq_partial(_ptr(wrapped(gv.reshape(1, -1))), 257, part.ptr, 1024, st)
    s = (gv.to(f64) ** 2).sum().reshape(1)
    out += _guard_rows("sumsq_partial n257 nblocks 1024 guarded", code, [(part, None)], val("sumsq_partial guarded sum", part.view.to(f64).sum().reshape(1), s, "sumsq32", s))
    return out


def all_checks(hip, emu, dev, ops_mod):
    yield "gemm_races", lambda: check_gemm_races(hip, emu, dev)
    yield "probe", lambda: check_probe(hip, emu, dev)
    yield "gemm", lambda: check_gemm_logged(hip, emu, dev)
    yield "gemm_kloop", lambda: check_gemm_kloop(hip, emu, dev)
    yield "gemm_edges", lambda: check_gemm_edges(hip, emu, dev)
    yield "gemm_forms", lambda: check_gemm_forms(hip, emu, dev)
    yield "gemm_guards", lambda: check_gemm_guards(hip, emu, dev)
    yield "conv", lambda: check_conv(hip, emu, dev)
    yield "conv_forms", lambda: check_conv_forms(hip, emu, dev)
    yield "conv_guards", lambda: check_conv_guards(hip, emu, dev)
    yield "attention", lambda: check_attention(hip, emu, dev)
    yield "norms", lambda: check_norms(hip, emu, dev)
    yield "norm_guards", lambda: check_norm_guards(hip, emu, dev)
    yield "streaming", lambda: check_streaming(hip, emu, dev)
    yield "streaming_values", lambda: check_streaming_values(hip, emu, dev)
    yield "streaming_layout", lambda: check_streaming_layout(hip, emu, dev)
    yield "streaming_guards", lambda: check_streaming_guards(hip, emu, dev)
    yield "wo", lambda: check_wo(hip, emu, dev, ops_mod)
    yield "wo_forms", lambda: check_wo_forms(hip, emu, dev, ops_mod)
    yield "wo_guards", lambda: check_wo_guards(hip, emu, dev, ops_mod)
    yield "image_prep", lambda: check_image_prep(hip, emu, dev)
