"""GPU: the GEGLU fused into the epilogues of the feed-forward GEMMs (E4T_EPI_GEGLU / E4T_EPI_GEGLU_BWD) against the unfused pair it replaces
— e4t_gemm_nt followed by e4t_geglu_fwd / e4t_geglu_bwd — BITWISE (same K-ordered fp32 dot product, rounded to bf16 at the same point, then the
same per-element helper), and against the emulation backend's restatement under the tolerance tests/kernel_checks.py uses for gemm and geglu."""
import pytest
import torch

import kernel_checks as kc

pytestmark = pytest.mark.gpu

# (M, dim): the feed-forward of the B = 16 training step at its four levels, and of SD-2.x @768 (96 x 96 latents) at B = 1 and 4; H = 4 dim
STEP = [(65536, 320), (16384, 640), (4096, 1280), (1024, 1280)]
SD2 = [(9216 * b // s, d) for b in (1, 4) for s, d in ((1, 320), (4, 640), (16, 1280), (64, 1280))]
# ragged: (M, dim, mult) with H = dim * mult = 1288 (dim a multiple of 8: every GEMM needs 16-byte rows); may run fused or be refused
RAGGED = [(77, 184, 7), (4129, 184, 7)]


def operands(dev, M, dim, seed, bias=True):
    g = kc.gen(seed, dev)
    H = 4 * dim
    x, dy = kc.rnd(g, M, dim, dev=dev), kc.rnd(g, M, dim, dev=dev)
    w1 = kc.rnd(g, 2 * H, dim, scale=dim ** -0.5, dev=dev)
    w2T = kc.rnd(g, H, dim, scale=H ** -0.5, dev=dev)            # W2^T: [H, dim]
    b1 = (torch.randn(2 * H, generator=g, device=dev) * 0.5) if bias else None
    return x, dy, w1, w2T, b1


def launch_log(hip, path, fn):
    """run fn() with the library's launch log on; returns its lines"""
    assert hip.lib.e4t_set_launch_log(str(path).encode()) == 0
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        hip.lib.e4t_set_launch_log(None)
    return open(path).read().splitlines()


@pytest.mark.parametrize("M, dim", STEP + SD2, ids=lambda v: str(v))
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
def test_fused_equals_unfused_bitwise(hip_env, tmp_path, M, dim, bias):
    hip, emu, dev, _ = hip_env
    x, dy, w1, w2T, b1 = operands(dev, M, dim, 7 + M % 97, bias)
    got = {}

    def fused():
        got["fwd"] = hip.gemm_geglu(x, w1, b1)
        got["u"] = hip.gemm(x, w1, bias=b1)
        got["du"] = hip.gemm_geglu_bwd(dy, w2T, got["u"])
    lines = launch_log(hip, tmp_path / "launch.log", fused)
    # none of these shapes may fall back: the ops answered, and the log shows one fused launch of each kind
    assert got["fwd"] is not None and got["du"] is not None, hip.lib.e4t_last_error()
    assert sum("|gemm_geglu M" in l and "_geglu_kernel<" in l for l in lines) == 1, lines
    assert sum("|gemm_geglu_bwd M" in l and "_geglu_kernel<" in l for l in lines) == 1, lines
    u, h = got["fwd"]
    u0 = got["u"]
    h0 = hip.geglu_fwd(u0)
    dh0 = hip.gemm(dy, w2T)
    du0 = hip.geglu_bwd(u0, dh0)
    assert torch.equal(u, u0), f"u: {(u != u0).sum().item()} elements differ"
    assert torch.equal(h, h0), f"h: {(h != h0).sum().item()} elements differ"
    assert torch.equal(got["du"], du0), f"du: {(got['du'] != du0).sum().item()} elements differ"
    # the emulation's restatement of each op on the op's own inputs, 8192 rows at a time (each output row depends on its own input row only:
    # the slices keep the fp32 intermediates of the restatement small at M = 65536)
    du = got["du"]
    for r0 in range(0, M, 8192):
        r = slice(r0, min(r0 + 8192, M))
        for label, a, b in (("u", u[r], emu.gemm(x[r], w1, bias=b1)), ("h", h[r], emu.geglu_fwd(u[r])), ("dh", dh0[r], emu.gemm(dy[r], w2T)),
                            ("du", du[r], emu.geglu_bwd(u[r], dh0[r]))):
            err = kc.rel(a, b)
            if r0 == 0:
                print(f"M{M} dim{dim} {label}: rel {err:.2e}")
            assert err <= kc.TOL1, (label, r0, err)


@pytest.mark.parametrize("M, dim", STEP + SD2, ids=lambda v: str(v))
def test_fused_launches_are_reproducible(hip_env, M, dim):
    """each fused shape again and again into fresh buffers: an ordering bug between the LDS staging writes and the store phase that reads value and
    gate chunks back would show as a difference between launches (the kernels are deterministic) — the pattern of kernel_checks.check_gemm_races"""
    hip, _, dev, _ = hip_env
    x, dy, w1, w2T, b1 = operands(dev, M, dim, 11)
    u, h = hip.gemm_geglu(x, w1, b1)
    du = hip.gemm_geglu_bwd(dy, w2T, u)
    differing = 0
    for _ in range(6):
        u2, h2 = hip.gemm_geglu(x, w1, b1)
        du2 = hip.gemm_geglu_bwd(dy, w2T, u)
        differing += int(not (torch.equal(u2, u) and torch.equal(h2, h) and torch.equal(du2, du)))
    assert differing == 0, f"{differing} of 6 repeated launches differ"


def ff_run(dev, M, dim, mult, seed, trainable):
    from e4t.models.attention import FeedForward
    torch.manual_seed(seed)
    ff = FeedForward(dim, mult=mult).to(dev)
    for p in ff.parameters():
        p.requires_grad_(trainable)
    g = kc.gen(seed + 1, dev)
    x = kc.rnd(g, M, dim, dev=dev).requires_grad_(True)
    res = kc.rnd(g, M, dim, dev=dev).requires_grad_(True)
    y = ff(x, residual=res)
    y.backward(kc.rnd(g, M, dim, dev=dev))
    out = {"y": y.detach(), "dx": x.grad, "dres": res.grad}
    out.update({n: p.grad for n, p in ff.named_parameters() if trainable})
    return out


@pytest.mark.parametrize("M, dim, mult", RAGGED + [(2048, 320, 4)], ids=lambda v: str(v))
@pytest.mark.parametrize("trainable", [False, True], ids=["frozen", "trainable"])
def test_feed_forward_module_fused_vs_unfused(hip_env, monkeypatch, M, dim, mult, trainable):
    """through FeedForward, ragged shapes included (which the library may refuse): whichever way it goes the result is the unfused composition's"""
    _, _, dev, ops = hip_env
    from e4t import functional as Fn
    # which way each half goes: what the module's own calls (its weights, its bias) to the product backend were answered
    went, be = {}, ops.backend()
    for name in ("gemm_geglu", "gemm_geglu_bwd"):
        def spy(*a, _f=getattr(be, name), _n=name):
            r = _f(*a)
            went[_n] = "fused" if r is not None else "refused -> unfused pair"
            return r
        monkeypatch.setattr(be, name, spy)
    got = ff_run(dev, M, dim, mult, 5, trainable)
    print(f"M{M} dim{dim} H{mult * dim}: forward {went.get('gemm_geglu')}, backward {went.get('gemm_geglu_bwd')}")
    assert set(went) == {"gemm_geglu", "gemm_geglu_bwd"}
    monkeypatch.setattr(Fn, "has_fused_feed_forward", lambda: False)
    want = ff_run(dev, M, dim, mult, 5, trainable)
    assert set(got) == set(want)
    for n in want:
        assert torch.equal(got[n], want[n]), n


def test_unet_transformer_blocks_fused_vs_forced_off(hip_env, monkeypatch):
    """a small UNet (every transformer block of it) forward + backward with the fused feed-forward on and forced off: output, input gradient and
    all parameter gradients bitwise equal — weight offsets trainable as in pre-training, plus the feed-forward weights as in tuning"""
    import e4t_oracle as orc
    from e4t import functional as Fn
    from e4t.models.unet_2d_condition import UNet2DConditionModel
    _, _, dev, _ = hip_env

    def run():
        torch.manual_seed(0)
        unet = UNet2DConditionModel(**orc.tiny_unet_config(ctx_dim=64)).to(dev)
        for n, p in unet.named_parameters():
            p.requires_grad_("wo" in n or ".ff." in n)
        g = kc.gen(3, dev)
        x = torch.randn(2, 4, 16, 16, generator=g, device=dev)
        ctx = torch.randn(2, 7, 64, generator=g, device=dev).requires_grad_(True)
        y = unet(x, torch.tensor([3, 977], device=dev), ctx).sample
        (y * torch.randn(y.shape, generator=g, device=dev).to(y.dtype)).sum().backward()
        grads = {n: p.grad for n, p in unet.named_parameters() if p.requires_grad}
        assert all(v is not None for v in grads.values()) and any(".ff." in n for n in grads)
        return y.detach(), ctx.grad, grads

    y1, c1, g1 = run()
    monkeypatch.setattr(Fn, "has_fused_feed_forward", lambda: False)
    y0, c0, g0 = run()
    assert torch.equal(y1, y0) and torch.equal(c1, c0)
    for n in g0:
        assert torch.equal(g1[n], g0[n]), n
