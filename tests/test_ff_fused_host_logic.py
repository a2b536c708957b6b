"""CPU: the one-node GEGLU feed-forward (functional.FeedForwardFn) against the composition it replaces (LinearFn -> GegluFn -> LinearFn), driven
through a stand-in backend defined HERE: the emulation backend's gemm + geglu_* composed into gemm_geglu / gemm_geglu_bwd, exactly what the fused
GEMM epilogues of the library compute.  Plus the host half of the library's side: a fused descriptor gets the plain descriptor's plan, and a plan
the fused kernels cannot run is refused with its own code before anything is launched."""
import ctypes as C

import pytest
import torch

from e4t import _C
from emu_backend import EmuBackend


class FusedEmu(EmuBackend):
    """emu + the two fused ops, counting their calls; refuse=True answers None as HipBackend does for a shape it has no fused kernel for"""

    def __init__(self, refuse=False, **kw):
        super().__init__(**kw)
        self.refuse, self.calls = refuse, {"gemm_geglu": 0, "gemm_geglu_bwd": 0, "geglu_fwd": 0, "geglu_bwd": 0}

    def gemm_geglu(self, x, w, bias):
        self.calls["gemm_geglu"] += 1
        if self.refuse:
            return None
        u = self.gemm(x, w, bias=bias)
        return u, EmuBackend.geglu_fwd(self, u)

    def gemm_geglu_bwd(self, dy, w2T, u):
        self.calls["gemm_geglu_bwd"] += 1
        if self.refuse:
            return None
        return EmuBackend.geglu_bwd(self, u, self.gemm(dy, w2T))

    def geglu_fwd(self, u):
        self.calls["geglu_fwd"] += 1
        return super().geglu_fwd(u)

    def geglu_bwd(self, u, dh):
        self.calls["geglu_bwd"] += 1
        return super().geglu_bwd(u, dh)


@pytest.fixture()
def use_backend():
    from e4t import ops
    old = ops.backend() if ops._backend is not None else None

    def install(b):
        ops.set_backend(b)
        return b
    yield install
    ops.set_backend(old)


def run_ff(trainable, seed=0, M=24, dim=16):
    """forward + backward of one FeedForward with residual; returns (y, grads by name) — x and the residual always need gradients"""
    from e4t import ops
    from e4t.models.attention import FeedForward
    torch.manual_seed(seed)
    ff = FeedForward(dim)
    for p in ff.parameters():
        p.requires_grad_(trainable)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(M, dim, generator=g).to(ops.ACT).requires_grad_(True)
    res = torch.randn(M, dim, generator=g).to(ops.ACT).requires_grad_(True)
    y = ff(x, residual=res)
    dy = torch.randn(M, dim, generator=g).to(y.dtype)
    y.backward(dy)
    grads = {"x": x.grad, "residual": res.grad}
    if trainable:
        grads.update({n: p.grad for n, p in ff.named_parameters()})
    return y.detach(), grads, y.grad_fn


def assert_same(a, b):
    ya, ga, _ = a
    yb, gb, _ = b
    assert torch.equal(ya, yb)
    assert set(ga) == set(gb)
    for n in ga:
        assert ga[n] is not None and gb[n] is not None, n
        assert torch.equal(ga[n], gb[n]), n


@pytest.mark.parametrize("trainable", [False, True])
def test_fused_feed_forward_equals_the_composition(use_backend, trainable):
    use_backend(EmuBackend())
    ref = run_ff(trainable)
    assert "FeedForwardFn" not in type(ref[2]).__name__          # a backend without the ops: the old path
    be = use_backend(FusedEmu())
    got = run_ff(trainable)
    assert "FeedForwardFn" in type(got[2]).__name__
    assert be.calls == {"gemm_geglu": 1, "gemm_geglu_bwd": 1, "geglu_fwd": 0, "geglu_bwd": 0}
    assert_same(ref, got)
    if trainable:
        assert set(got[1]) == {"x", "residual", "net.0.proj.weight", "net.0.proj.bias", "net.2.weight", "net.2.bias"}


@pytest.mark.parametrize("trainable", [False, True])
def test_a_refusing_backend_runs_the_unfused_pair(use_backend, trainable):
    use_backend(EmuBackend())
    ref = run_ff(trainable)
    be = use_backend(FusedEmu(refuse=True))
    got = run_ff(trainable)
    assert be.calls == {"gemm_geglu": 1, "gemm_geglu_bwd": 1, "geglu_fwd": 1, "geglu_bwd": 1}
    assert_same(ref, got)


@pytest.mark.parametrize("trainable", [False, True])
def test_h_is_saved_only_for_a_trainable_w2(use_backend, trainable):
    use_backend(FusedEmu())
    from e4t import ops
    from e4t.models.attention import FeedForward
    torch.manual_seed(0)
    M, dim = 8, 16
    ff = FeedForward(dim)
    for p in ff.parameters():
        p.requires_grad_(trainable)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
        y = ff(torch.randn(M, dim).to(ops.ACT).requires_grad_(True))
    shapes = sorted(tuple(t.shape) for t in saved)
    H = 4 * dim
    assert (M, 2 * H) in shapes                                   # u: the backward needs both halves
    assert ((M, H) in shapes) == trainable                        # h: only for dW2
    assert ((M, dim) in shapes) == trainable                      # x: only for dW1
    y.sum().backward()


# ---- the library's host side (no launch) -----------------------------------------------------------------------------------------------
lib = _C.load()
FWD_SHAPES = [(65536, 2560, 320), (16384, 5120, 640), (4096, 10240, 1280), (1024, 10240, 1280)]
BWD_SHAPES = [(65536, 1280, 320), (16384, 2560, 640), (4096, 5120, 1280), (1024, 5120, 1280)]


def plan(M, N, K, flags=0, splitk=0, **kw):
    wide = 2 * N if flags == _C.EPI_GEGLU_BWD else N
    d = _C.GemmDesc(M=M, N=N, K=K, K1=K, lda=K, ldb=K, ldc=wide, batch=1, alpha=1.0, flags=flags, splitk=splitk,
                    ldaux=(N // 2 if flags == _C.EPI_GEGLU else wide), **kw)
    pl = _C.GemmPlan()
    rc = lib.e4t_gemm_plan(C.byref(d), C.byref(pl))
    return rc, (pl.tile, pl.tile_m, pl.tile_n, pl.splitk, pl.workspace_bytes, pl.tail_rows, pl.stages)


@pytest.mark.parametrize("flag, shapes", [(_C.EPI_GEGLU, FWD_SHAPES), (_C.EPI_GEGLU_BWD, BWD_SHAPES)])
def test_a_fused_descriptor_gets_the_plain_plan(flag, shapes):
    for M, N, K in shapes:
        rc0, plain = plan(M, N, K)
        rc1, fused = plan(M, N, K, flags=flag)
        assert rc0 == 0 and rc1 == 0, (M, N, K, lib.e4t_last_error())
        assert fused == plain and plain[3] == 1 and plain[5] == 0, (M, N, K, plain, fused)


@pytest.mark.parametrize("flag, shape", [(_C.EPI_GEGLU, FWD_SHAPES[2]), (_C.EPI_GEGLU_BWD, BWD_SHAPES[2])])
def test_a_plan_without_a_fused_kernel_is_refused_with_its_own_code(flag, shape):
    M, N, K = shape
    rc, pl = plan(M, N, K, flags=flag, splitk=3)
    assert rc == _C.ERR_NO_FUSED and pl[3] == 3 and b"split-K" in lib.e4t_last_error()
    assert _C.ERR_NO_FUSED not in (-22, -12, -5)                  # distinct from bad arguments / workspace / launch failure
    # a tile without the capability (256 x 256 ping-pong), a residual, a second flag
    rc, pl = plan(M, N, K, flags=flag, tile=512)
    assert rc == _C.ERR_NO_FUSED and pl[0] == 512 and b"carries no fused" in lib.e4t_last_error()
    assert plan(M, N, K, flags=flag, residual=1 << 20, ldr=N)[0] == _C.ERR_NO_FUSED
    assert plan(M, N, K, flags=flag | _C.ACT_GELU)[0] == _C.ERR_NO_FUSED
    # e4t_gemm_nt refuses the same descriptor before launching anything (no device is touched: this runs without a GPU)
    wide = 2 * N if flag == _C.EPI_GEGLU_BWD else N
    d = _C.GemmDesc(A=1 << 20, B=1 << 21, C=1 << 22, aux=1 << 23, M=M, N=N, K=K, K1=K, lda=K, ldb=K, ldc=wide, ldaux=wide, batch=1, alpha=1.0,
                    flags=flag, splitk=3)
    assert lib.e4t_gemm_nt(C.byref(d), None) == _C.ERR_NO_FUSED and b"split-K" in lib.e4t_last_error()
    d.aux, d.splitk = None, 0
    assert lib.e4t_gemm_nt(C.byref(d), None) == -22 and b"aux" in lib.e4t_last_error()
