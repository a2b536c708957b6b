"""-m gpu: gemm_kernel, the register-staged fallback (operands beyond 4 GB, or E4T_GEMM_REGSTAGE), against the emulated reference.

The library reads E4T_GEMM_REGSTAGE once per process, so the cases run in a fresh child process with the switch set (this file, run as a
script); the child prints one JSON line per check and the test asserts on them.  The shapes are the smallest at which the kernel's operand
addressing can go wrong: partial M and N tiles and a ragged last K-tile, the second A source, a batch entry and a split index other than 0,
and every conv mode on odd maps with two images in one row tile — on both tiles the kernel is built for (64 and 128)."""
import json
import os
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILES = (64, 128)
# B, Hin, Win, Cin, Cout, mode, Hout, Wout, splitk (modes: emu_backend CONV_*; 5 = S2A)
CONV_CASES = [(2, 5, 7, 64, 72, "S1", 5, 7, 1), (2, 5, 7, 64, 72, "S2", 3, 4, 1), (2, 3, 4, 64, 72, "UP2", 6, 8, 1), (2, 3, 4, 64, 72, "S2T", 5, 7, 1),
              (2, 6, 8, 64, 72, "S2A", 3, 4, 1), (2, 5, 7, 64, 72, "S1", 5, 7, 2)]


def child():
    for p in (os.path.join(ROOT, "e4t-diffusion_amd"), ROOT, os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch
    import emu_backend as eb
    import kernel_checks as kc
    from e4t import _C, ops
    assert os.environ.get("E4T_GEMM_REGSTAGE"), "the child runs with the switch set"
    hip, emu, dev = ops.HipBackend(), eb.EmuBackend(), torch.device("cuda:0")
    f32 = torch.float32
    out = []
    M, N = 200, 72
    log = os.path.join(tempfile.mkdtemp(), "launches.txt")
    for tile in TILES:
        _C.check(hip.lib.e4t_set_launch_log(log.encode()), "e4t_set_launch_log")      # the dense launches of this tile, by kernel symbol
        g = kc.gen(700 + tile, dev)
        # dense: partial M and N tiles, K = 136 = two K-tiles and a ragged third
        a, b = kc.rnd(g, M, 136, dev=dev), kc.rnd(g, N, 136, scale=136 ** -0.5, dev=dev)
        bias, res = kc.rnd(g, N, dtype=f32, dev=dev), kc.rnd(g, M, N, dev=dev)
        out.append((f"regstage gemm {M}x{N}x136 t{tile}", kc.rel(hip.gemm(a, b, bias=bias, residual=res, tile=tile, splitk=1), emu.gemm(a, b, bias=bias, residual=res)), kc.TOL1))
        # two-source A: K1 = 64, K = 192
        a1, a2, b2 = kc.rnd(g, M, 64, dev=dev), kc.rnd(g, M, 128, dev=dev), kc.rnd(g, N, 192, scale=192 ** -0.5, dev=dev)
        ref2 = emu.gemm(a1, b2, a2=a2, bias=bias)
        out.append((f"regstage gemm two-source A t{tile}", kc.rel(hip.gemm(a1, b2, a2=a2, bias=bias, tile=tile, splitk=1), ref2), kc.TOL1))
        # split-K = 2 through the workspace (three K-tiles: the second split holds one)
        out.append((f"regstage gemm two-source A t{tile} split-K 2", kc.rel(hip.gemm(a1, b2, a2=a2, bias=bias, tile=tile, splitk=2), ref2), kc.TOL1))
        # batch = 2, non-zero batch strides of A, B, bias and C (the ABI has one batch stride for both A sources: two column slices of one buffer)
        wide, B2 = kc.rnd(g, 2, M, 192, dev=dev), kc.rnd(g, 2, N, 192, scale=192 ** -0.5, dev=dev)
        A1, A2 = wide[:, :, :64], wide[:, :, 64:]
        bb = kc.rnd(g, 2, N, dtype=f32, dev=dev)
        y, yr = hip.gemm(A1, B2, a2=A2, bias=bb, tile=tile, splitk=1), emu.gemm(A1, B2, a2=A2, bias=bb)
        out.append((f"regstage gemm batched two-source A t{tile}", kc.rel(y, yr), kc.TOL1))
        out.append((f"regstage gemm batched two-source A t{tile}: batch entry 1", kc.rel(y[1], yr[1]), kc.TOL1))
        _C.check(hip.lib.e4t_set_launch_log(None), "e4t_set_launch_log")
        gemms = [l.split("|")[:2] for l in open(log) if "|gemm " in l]      # "<symbol>|gemm M.. N.. K.. batch.. splitk.. flags..|bytes|flops"
        out.append((f"regstage gemm t{tile}: 4 launches, all gemm_kernel (got {sorted(set(sym for sym, _ in gemms))})", float(len(gemms) != 4 or any(sym != "gemm_kernel" for sym, _ in gemms)), 0.0))
        out.append((f"regstage gemm t{tile}: one launch with split-K 2, one with batch 2", float(sum(" splitk2 " in d for _, d in gemms) != 1 or sum(" batch2 " in d for _, d in gemms) != 1), 0.0))
        for i, (B, Hin, Win, Cin, Cout, mname, Hout, Wout, sk) in enumerate(CONV_CASES):
            mode = kc.CONV_S2A if mname == "S2A" else getattr(eb, "CONV_" + mname)
            case = (B, Hin, Win, Cin, Cout, mode, Hout, Wout, tile, sk)
            sym = kc.conv_kernel(case, "full")
            out.append((f"{kc.conv_tag(case)}: runs {sym}, wanted gemm_kernel splitk{sk}", 0.0 if sym == f"gemm_kernel splitk{sk}" else 1.0, 0.0))
            x, w, cb, rb, r = kc.conv_inputs(case, 720 + 10 * (tile // 64) + i, dev)
            y = hip.conv3x3(x, w, B, Hin, Win, Hout, Wout, mode, bias=cb, rowbias=rb, residual=r, tile=tile, splitk=sk)
            yr = emu.conv3x3(x, w, B, Hin, Win, Hout, Wout, mode, bias=cb, rowbias=rb, residual=r)
            out.append((kc.conv_tag(case), kc.rel(y, yr), kc.TOL1))
            out += kc.conv_slices(kc.conv_tag(case), y, yr, B, Hout, Wout, kc.conv_plan(case, "full"))
            y, yr = hip.conv3x3(x, w, B, Hin, Win, Hout, Wout, mode, tile=tile, splitk=sk), emu.conv3x3(x, w, B, Hin, Win, Hout, Wout, mode)
            out.append((kc.conv_tag(case) + " bare", kc.rel(y, yr), kc.TOL1))
            out += kc.conv_slices(kc.conv_tag(case) + " bare", y, yr, B, Hout, Wout, kc.conv_plan(case, "bare"))
    torch.cuda.synchronize()
    for row in out:
        print("CHECK " + json.dumps(row))


@pytest.mark.gpu
def test_register_staged_kernel_in_a_child_process():
    env = dict(os.environ, E4T_GEMM_REGSTAGE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"child failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    rows = [json.loads(l[6:]) for l in r.stdout.splitlines() if l.startswith("CHECK ")]
    per_tile = 7 + len(CONV_CASES) * 3      # dense checks and their launch-log rows + per conv: symbol, full, bare (slices on top)
    assert len(rows) >= len(TILES) * per_tile, f"{len(rows)} checks came back"
    for n, e, t in rows:
        print(f"{n}: {e:.3e} (tol {t:.1e})")
    bad = [(n, e, t) for n, e, t in rows if not (e <= t)]
    assert not bad, "parity failures:\n" + "\n".join(f"  {n}: rel_l2={e:.3e} > tol={t:.1e}" for n, e, t in bad)


if __name__ == "__main__":
    child()
