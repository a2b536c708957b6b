"""-m gpu: the FreeU kernels (csrc/freeu.hip) against the float64 definition (tests/freeu_reference.py) on the same bf16 inputs, and
FreeU in the sampling pipeline: graph replay, fused eager and the generic loop.

Bounds.  The outputs are ONE bf16 rounding of an fp32 result, so elementwise |got - ref| <= 2^-7 |ref| + 1e-6 max|input| (one bf16 ulp:
half an ulp of rounding plus room for the fp32 error to flip it; max|input| per image and tensor) and rel-L2 <= 2^-8 overall; unit factors
give the inputs back bit for bit.  The fp32 workspace is held to float64 within 1e-5 of the largest magnitude in the image."""
import pytest
import torch

import freeu_reference as ref
from test_sampler_fused_gpu import tiny_pipe  # noqa: F401  (module-scoped fixture: the tiny pipeline on the GPU)

pytestmark = pytest.mark.gpu

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
SHAPES = [(1, 2, 2, 16, 8),            # smallest legal
          (3, 3, 5, 16, 8),            # odd, non-square
          (2, 6, 10, 80, 40),          # widths that are no power of two; several vectors per row
          (2, 8, 8, 1280, 1280),       # real stage-1 widths
          (2, 16, 16, 1280, 640),      # real stage-1 widths
          (1, 64, 64, 32, 16),         # rows far beyond one workgroup: the multi-chunk reduction
          (2, 24, 24, 640, 320)]       # real stage-2 widths
FACTORS = [(1.3, 0.9), (1.4, 0.2), (1.0, 1.0)]
KINDS = [(0.0, 1.0), (3.0, 0.05), (-2.0, 4.0), "flat"]       # per-image (mean, sd); "flat": the channel mean is constant over the map
GUARD = 64                                                    # rows (outputs) / floats (workspace) of guard band on either side
_cache = {}


def inputs(si, dev):
    """bf16 (h, k) of SHAPES[si], made once; image i of shape si is of kind (si + i) % 4, so every kind occurs and a batch mixes them"""
    if si not in _cache:
        B, H, W, Ch, Ck = SHAPES[si]
        g = torch.Generator().manual_seed(100 + si)
        hs, ks = [], []
        for i in range(B):
            kind = KINDS[(si + i) % 4]
            if kind == "flat":             # every pixel carries the same channel vector: max == min exactly
                hs.append((torch.randn(1, Ch, generator=g) * 2 + 1).expand(H * W, Ch))
                ks.append(torch.randn(H * W, Ck, generator=g))
            else:
                hs.append(torch.randn(H * W, Ch, generator=g) * kind[1] + kind[0])
                ks.append(torch.randn(H * W, Ck, generator=g) * kind[1] + kind[0])
        _cache[si] = (torch.cat(hs).to(bf16).contiguous().to(dev), torch.cat(ks).to(bf16).contiguous().to(dev))
    return _cache[si]


def reference(si, b, s, version, dev):
    key = (si, b, s, version)
    if key not in _cache:
        B, H, W, _, _ = SHAPES[si]
        h, k = inputs(si, dev)
        h2, k2 = ref.freeu_pair(ref.to_nchw(h, B, H, W), ref.to_nchw(k, B, H, W), b, s, version)
        _cache[key] = (ref.to_rows(h2).contiguous(), ref.to_rows(k2).contiguous())
    return _cache[key]


def guarded(shape, dtype, dev, fill):
    """a buffer with GUARD rows (or elements) of `fill` on either side of the part handed to the kernel -> (whole, part)"""
    whole = torch.full((shape[0] + 2 * GUARD,) + tuple(shape[1:]), fill, dtype=dtype, device=dev)
    return whole, whole[GUARD:GUARD + shape[0]]


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == bf16 else torch.int32)


def run(hip, ops, si, b, s, version, dev):
    B, H, W, Ch, Ck = SHAPES[si]
    h, k = inputs(si, dev)
    n = ops.freeu_ws_floats(B, H * W, Ck)
    ws_all, ws = guarded((n,), f32, dev, float("nan"))          # NaN: a value the statistics did not write cannot be read unnoticed
    oh_all, oh = guarded((B * H * W, Ch), bf16, dev, 7.0)
    ok_all, ok = guarded((B * H * W, Ck), bf16, dev, 7.0)
    h0, k0 = h.clone(), k.clone()
    assert hip.freeu_stats(h, k, B, H, W, version, ws=ws) is ws
    h2, k2 = hip.freeu_apply(h, k, ws, B, H, W, b, s, version, out_h=oh, out_k=ok)
    torch.cuda.synchronize()
    assert torch.equal(bits(h), bits(h0)) and torch.equal(bits(k), bits(k0))             # neither input is written
    for whole in (oh_all, ok_all):
        assert bool((whole[:GUARD] == 7.0).all()) and bool((whole[-GUARD:] == 7.0).all())
    assert bool(torch.isnan(ws_all[:GUARD]).all()) and bool(torch.isnan(ws_all[-GUARD:]).all())
    return h2, k2, ws


def check_close(got, want, src, B, what):
    got, want, src = got.to(f64).view(B, -1), want.view(B, -1), src.to(f64).view(B, -1)
    assert bool(torch.isfinite(got).all()), what
    bound = 2.0 ** -7 * want.abs() + 1e-6 * src.abs().amax(dim=1, keepdim=True)
    err = (got - want).abs()
    worst = float((err - bound).max())
    r = float((got - want).norm() / want.norm())
    print(f"{what}: max (err - bound) {worst:.3e}, rel-L2 {r:.3e}")
    assert worst <= 0.0, (what, worst)
    assert r <= 2.0 ** -8, (what, r)


@pytest.mark.parametrize("version", [2, 1])
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_kernels_match_the_float64_definition(hip_env, si, version):
    hip, _, dev, ops = hip_env
    B, H, W, Ch, Ck = SHAPES[si]
    h, k = inputs(si, dev)
    for b, s in FACTORS:
        h2, k2, ws = run(hip, ops, si, b, s, version, dev)
        if (b, s) == (1.0, 1.0):
            assert torch.equal(bits(h2), bits(h)) and torch.equal(bits(k2), bits(k)), (SHAPES[si], version)
            continue
        want_h, want_k = reference(si, b, s, version, dev)
        check_close(h2, want_h, h, B, f"h' {SHAPES[si]} v{version} b={b}")
        check_close(k2, want_k, k, B, f"k' {SHAPES[si]} v{version} s={s}")
        assert torch.equal(bits(h2[:, Ch // 2:]), bits(h[:, Ch // 2:]))                   # the second half of the backbone passes through
    # two calls agree to the bit, workspace included (fixed-order reductions, no atomics)
    a = run(hip, ops, si, 1.4, 0.2, version, dev)
    c = run(hip, ops, si, 1.4, 0.2, version, dev)
    for x, y in zip(a, c):
        assert torch.equal(bits(x), bits(y))


@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_workspace_matches_float64(hip_env, si):
    hip, _, dev, ops = hip_env
    B, H, W, Ch, Ck = SHAPES[si]
    h, k = inputs(si, dev)
    ws = hip.freeu_stats(h, k, B, H, W, 2)
    v = ops.freeu_ws_views(ws, B, H * W, Ck)
    want = ref.coefficients(ref.to_nchw(k, B, H, W))                                      # [B, 7, C_k]
    err = (v["coef"].to(f64) - want).abs().amax(dim=(1, 2))
    scale = want.abs().amax(dim=(1, 2))
    print(f"{SHAPES[si]}: coefficients, max error / largest magnitude per image {(err / scale).tolist()}")
    assert bool((err <= 1e-5 * scale).all()), (err / scale).tolist()
    mn, mx = v["mm"][:, :, 0].amin(dim=1, keepdim=True).to(f64), v["mm"][:, :, 1].amax(dim=1, keepdim=True).to(f64)
    msum = v["msum"].to(f64)
    assert bool(torch.isfinite(msum).all()) and bool((mn == msum.amin(dim=1, keepdim=True)).all()) and bool((mx == msum.amax(dim=1, keepdim=True)).all())
    rng = mx - mn
    got = torch.where(rng > 0, (msum - mn) / torch.where(rng > 0, rng, torch.ones_like(rng)), torch.zeros_like(msum))
    want_m = ref.mhat(ref.to_nchw(h, B, H, W)).reshape(B, H * W)
    err = (got - want_m).abs().amax(dim=1)
    print(f"{SHAPES[si]}: m^ map, max error per image {err.tolist()}")
    assert bool((err <= 1e-5 * want_m.abs().amax(dim=1)).all()), err.tolist()
    flat = [i for i in range(B) if KINDS[(si + i) % 4] == "flat"]
    assert all(float(rng[i]) == 0.0 for i in flat)                                       # the max == min path is taken


def test_unsupported_widths_raise(hip_env):
    from e4t import _C
    hip, _, dev, ops = hip_env
    for Ch, Ck in ((24, 8), (16, 12), (8, 8)):
        h, k = torch.zeros(16, Ch, dtype=bf16, device=dev), torch.zeros(16, Ck, dtype=bf16, device=dev)
        ws = torch.zeros(ops.freeu_ws_floats(1, 16, Ck), dtype=f32, device=dev)
        with pytest.raises(_C.E4TError, match="multiple of"):
            hip.freeu_stats(h, k, 1, 4, 4)
        with pytest.raises(_C.E4TError, match="multiple of"):
            hip.freeu_apply(h, k, ws, 1, 4, 4, 1.3, 0.9)
    h, k = torch.zeros(4, 16, dtype=bf16, device=dev), torch.zeros(4, 8, dtype=bf16, device=dev)
    with pytest.raises(_C.E4TError, match=">= 2"):
        hip.freeu_stats(h, k, 1, 1, 4)


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------------
def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_pipeline_with_freeu_graph_eager_generic(tiny_pipe):
    from e4t import freeu
    from e4t.schedulers import DDIMScheduler
    pipe, image, lat0 = tiny_pipe
    pipe.scheduler = DDIMScheduler.stable_diffusion()

    def call(use_graph, fused=True):
        pipe._fused_sampling = fused
        try:
            return pipe("a painting of *s", height=32, width=32, num_inference_steps=3, guidance_scale=5.0, num_images_per_prompt=2, image=image,
                        latents=lat0.clone(), output_type="latent", use_graph=use_graph).images
        finally:
            pipe._fused_sampling = True

    off = call(True)
    try:
        st = pipe.enable_freeu()
        assert len(st.stages) == 12 and freeu.get_state(pipe.unet) is st
        eager, graph, generic = call(False), call(True), call(False, fused=False)
    finally:
        pipe.disable_freeu()
    assert freeu.get_state(pipe.unet) is None
    assert bool(torch.isfinite(eager).all())
    assert torch.equal(eager, graph), rel(graph, eager)
    r = rel(eager, generic)
    print(f"FreeU, DDIM, 3 steps: fused vs generic rel-L2 {r:.2e}; FreeU on vs off rel-L2 {rel(eager, off):.2e}")
    assert r < 1e-3, r
    assert rel(eager, off) > 1e-3                                # the option is not silently ignored
    assert torch.equal(call(True), off)                          # enabled and undone: the unmarked pipeline, bit for bit
