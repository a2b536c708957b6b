"""-m gpu: e4t_sampler_step_edit (the sampler step with the masked blend of editing) against a float64 restatement
of its contract and against e4t_sampler_step, and the pipeline's img2img / inpainting call for every sampler on the tiny models:
fused eager == graph replay bit for bit, fused close to the generic step + torch-blend loop (the definition), held pixels end at
the original's latent exactly, and plain sampling is untouched by an edit call."""
import pytest
import torch

from test_sampler_fused_gpu import SAMPLERS, reference, rel, tiny_pipe  # noqa: F401  (tiny_pipe: this module's own instance)

pytestmark = pytest.mark.gpu

f32 = torch.float32
K = 3


def edit_reference(o, row, keep, x0, n0):
    """the header's blend in float64 on the fp32 inputs; o = the unblended float64 out"""
    a, s = float(row[14]), float(row[15])
    B, C, H, W = o.shape
    k = keep.double().reshape(-1, 1, H, W)
    y = s * n0.double() + a * x0.double().reshape(-1, C, H, W)
    return k * y + (1 - k) * o, y


@pytest.mark.parametrize("B", [1, 2, 3])
def test_sampler_step_edit_matches_restatement(hip_env, B):
    hip, _, dev, _ = hip_env
    g = torch.Generator(device=dev).manual_seed(20 + B)
    H, W = 7, 9 + B                                       # HW = 70, 77, 84: not multiples of 256, more than one block with C = 4
    shape = (B, 4, H, W)
    worst, cases = 0.0, 0
    for cfg in (False, True):
        for nhwc in (False, True):
            for keep_pi in (False, True):
                for x0_pi in (False, True):
                    for w in (-1, 0, 1, 2):
                        for with_noise in (False, True):
                            save_x = (w + cases) % 2 == 0
                            P = (2 if cfg else 1) * B
                            x = torch.randn(shape, generator=g, device=dev)
                            pshape = (P, H, W, 4) if nhwc else (P, 4, H, W)
                            pred = torch.randn(pshape, generator=g, device=dev)
                            pred2 = torch.randn(pshape, generator=g, device=dev)
                            hist = torch.randn((K,) + shape, generator=g, device=dev)
                            saved = torch.randn(shape, generator=g, device=dev)
                            noise = torch.randn(shape, generator=g, device=dev) if with_noise else None
                            keep = torch.rand((B if keep_pi else 1, H, W), generator=g, device=dev)
                            sel = torch.rand(keep.shape, generator=g, device=dev)
                            keep[sel < 0.3], keep[sel > 0.7] = 0.0, 1.0
                            x0 = torch.randn((B if x0_pi else 1, 4, H, W), generator=g, device=dev)
                            n0 = torch.randn(shape, generator=g, device=dev)
                            coefs = (torch.rand(16, generator=g, device=dev) * 2 - 1).tolist()
                            row = torch.tensor([7.5] + coefs[:6] + [0.8, float(w), float(save_x)] + coefs[6:9] + [0.0] + coefs[9:11],
                                               dtype=f32, device=dev)
                            o64, m, _ = reference(pred, x, row, hist, saved, noise, cfg, nhwc)
                            want, y = edit_reference(o64, row, keep, x0, n0)
                            # the unblended kernel on the same inputs
                            hp, sp = hist.clone(), saved.clone()
                            plain = hip.sampler_step(pred, x, row, hist=hp, saved=sp, noise=noise, cfg=cfg, pred_nhwc=nhwc)
                            he, se = hist.clone(), saved.clone()
                            x_in = torch.full((P,) + shape[1:], float("nan"), device=dev)
                            ro = (keep.clone(), x0.clone(), n0.clone())
                            out = hip.sampler_step_edit(pred, x, row, keep, x0, n0, hist=he, saved=se, noise=noise, x_in=x_in, cfg=cfg, pred_nhwc=nhwc)
                            out2 = hip.sampler_step_edit(pred2, x, row, keep, x0, n0, hist=hist.clone(), saved=saved.clone(), noise=noise,
                                                         cfg=cfg, pred_nhwc=nhwc)
                            torch.cuda.synchronize()
                            tag = (B, cfg, nhwc, keep_pi, x0_pi, w, save_x, with_noise)
                            err = rel(out, want)
                            worst, cases = max(worst, err), cases + 1
                            assert err <= 1e-6, (tag, err)
                            kb = keep.reshape(-1, 1, H, W).expand(B, 4, H, W)
                            assert (kb == 0).any() and (kb == 1).any()
                            assert torch.equal(out[kb == 0], plain[kb == 0]), tag             # keep == 0: e4t_sampler_step's bits
                            assert torch.equal(out[kb == 1], out2[kb == 1]), tag              # keep == 1: independent of pred
                            assert rel(out[kb == 1], y[kb == 1]) <= 1e-6, tag
                            assert not torch.equal(out[(kb > 0) & (kb < 1)], out2[(kb > 0) & (kb < 1)])
                            assert torch.equal(x_in[:B], row[7] * out), tag                  # x_in = k_in * the blended value
                            if cfg:
                                assert torch.equal(x_in[B:], x_in[:B]), tag
                            assert torch.equal(he, hp) and torch.equal(se, sp), tag           # hist / saved: as the unblended kernel
                            assert rel(he[w], m) <= 1e-6 if w >= 0 else torch.equal(he, hist), tag
                            assert torch.equal(se, x if save_x else saved), tag
                            for t, t0 in zip((keep, x0, n0), ro):
                                assert torch.equal(t, t0), tag                                # read-only operands
    print(f"sampler_step_edit B={B}: {cases} cases, worst rel err {worst:.2e}")


def test_sampler_step_edit_in_place_and_last_row(hip_env):
    """out aliases x, no hist / saved / x_in (an eager DDIM row); a last row (a_keep, s_keep) = (1, 0) ends at x0 exactly"""
    hip, _, dev, _ = hip_env
    g = torch.Generator(device=dev).manual_seed(31)
    shape = (2, 4, 5, 13)
    x = torch.randn(shape, generator=g, device=dev)
    pred = torch.randn((4,) + shape[1:], generator=g, device=dev)
    keep = torch.rand(5, 13, generator=g, device=dev)
    keep[0, :4], keep[1, :4] = 0.0, 1.0
    x0 = torch.randn((1,) + shape[1:], generator=g, device=dev)
    n0 = torch.randn(shape, generator=g, device=dev)
    for a_keep, s_keep in ((0.7, 0.6), (1.0, 0.0)):
        row = torch.tensor([3.0, 0.9, 0.2, 1.1, 0.0, -0.4, 0.0, 1.0, -1.0, 0.0] + [0.0] * 4 + [a_keep, s_keep], dtype=f32, device=dev)
        want, _ = edit_reference(reference(pred, x, row, None, None, None, True, False)[0], row, keep, x0, n0)
        plain = hip.sampler_step(pred, x, row, cfg=True)
        xi = x.clone()
        got = hip.sampler_step_edit(pred, xi, row, keep, x0, n0, cfg=True, out=xi)
        assert got is xi and rel(xi, want) <= 1e-6
        kb = keep.expand(shape)
        assert torch.equal(xi[kb == 0], plain[kb == 0])
        if s_keep == 0.0:
            assert torch.equal(xi[kb == 1], x0.expand(shape)[kb == 1])


@pytest.fixture(scope="module")
def edit_pipe(tiny_pipe):
    """tiny_pipe plus a tiny VAE encoder, a photograph and a half-plane mask whose edge is not on the latent grid"""
    from e4t.vae import VAEEncoder
    pipe, image, lat0 = tiny_pipe
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(3)
        enc = VAEEncoder(block_out_channels=(64, 64)).requires_grad_(False)
    pipe.vae_encoder = enc.to(pipe.device)
    g = torch.Generator().manual_seed(8)
    photo = torch.rand(1, 3, 32, 32, generator=g) * 2 - 1
    mask = torch.zeros(32, 32)
    mask[:, 13:] = 1.0                                     # white = repaint; latent column 6 (pixels 12, 13) is half covered
    assert pipe.vae_scale_factor == 2
    keep = 1.0 - torch.nn.functional.avg_pool2d(mask[None, None], 2)[0, 0]
    assert (keep == 1).any() and (keep == 0).any() and (keep == 0.5).any()
    x0 = enc.encode_sample(photo.to(pipe.device), torch.zeros(1, 4, 16, 16, device=pipe.device)).float()
    return pipe, image, lat0, photo, mask, keep.to(pipe.device), x0


def call(pipe, image, lat0, name, eta, guidance, steps, use_graph, fused=True, seed=1, **edit):
    from e4t.schedulers import SCHEDULER_MAPPING
    pipe.scheduler = SCHEDULER_MAPPING[name].stable_diffusion()
    calls = []
    pipe._fused_sampling = fused
    try:
        out = pipe("a painting of *s", height=32, width=32, num_inference_steps=steps, guidance_scale=guidance, num_images_per_prompt=2,
                   image=image, latents=lat0.clone(), output_type="latent", eta=eta, use_graph=use_graph,
                   generator=torch.Generator(device="cuda").manual_seed(seed), callback=lambda i, t, l: calls.append(i), **edit).images
    finally:
        pipe._fused_sampling = True
    return out, len(calls)


@pytest.mark.parametrize("guidance", [1.0, 5.0])
@pytest.mark.parametrize("name,eta", SAMPLERS)
def test_pipeline_inpainting(edit_pipe, name, eta, guidance):
    pipe, image, lat0, photo, mask, keep, x0 = edit_pipe
    kw = dict(init_image=photo, strength=0.5, mask_image=mask)
    kept = 3                                               # 6 steps at strength 0.5
    want_calls = kept + 1 if name == "plms" else kept
    eager, n_e = call(pipe, image, lat0, name, eta, guidance, 6, False, **kw)
    graph, n_g = call(pipe, image, lat0, name, eta, guidance, 6, True, **kw)
    generic, n_s = call(pipe, image, lat0, name, eta, guidance, 6, False, fused=False, **kw)
    assert (n_e, n_g, n_s) == (want_calls,) * 3
    assert torch.isfinite(eager).all()
    assert torch.equal(eager, graph), rel(graph, eager)
    r = rel(eager, generic)
    print(f"{name} eta={eta} guidance={guidance}: inpainting fused vs generic rel-L2 {r:.2e}")
    assert r < 1e-3, r
    held = (keep == 1).expand(2, 4, 16, 16)
    for out in (eager, graph, generic):
        assert torch.equal(out[held], x0.expand(2, 4, 16, 16)[held])            # outside the mask: the photograph's latent, bitwise
    free = (keep == 0).expand(2, 4, 16, 16)
    assert not torch.equal(eager[free], x0.expand(2, 4, 16, 16)[free])


@pytest.mark.parametrize("name,eta", SAMPLERS)
def test_pipeline_img2img_full_strength_and_plain_call_untouched(edit_pipe, name, eta):
    pipe, image, lat0, photo, mask, keep, x0 = edit_pipe
    steps = 6
    want_calls = steps + 1 if name == "plms" else steps
    before, n_b = call(pipe, image, lat0, name, eta, 5.0, steps, True)
    # strength 1.0 without a mask (keep == 0 everywhere): every step runs, from the photograph at the first timestep's level
    eager, n_e = call(pipe, image, lat0, name, eta, 5.0, steps, False, init_image=photo, strength=1.0)
    graph, n_g = call(pipe, image, lat0, name, eta, 5.0, steps, True, init_image=photo, strength=1.0)
    generic, n_s = call(pipe, image, lat0, name, eta, 5.0, steps, False, fused=False, init_image=photo, strength=1.0)
    assert (n_b, n_e, n_g, n_s) == (want_calls,) * 4
    assert torch.equal(eager, graph)
    assert rel(eager, generic) < 1e-3
    assert not torch.equal(eager, before)
    inpaint, _ = call(pipe, image, lat0, name, eta, 5.0, steps, True, init_image=photo, strength=0.5, mask_image=mask)
    after, n_a = call(pipe, image, lat0, name, eta, 5.0, steps, True)
    assert n_a == want_calls and torch.equal(after, before)                     # a plain call: the same bits before and after editing


def test_pipeline_refuses_bad_edit_calls(edit_pipe):
    pipe, image, lat0, photo, mask, keep, x0 = edit_pipe
    with pytest.raises(ValueError, match="init_image"):
        call(pipe, image, lat0, "ddim", 0.0, 5.0, 6, False, mask_image=mask)
    with pytest.raises(ValueError, match="no denoising step"):
        call(pipe, image, lat0, "ddim", 0.0, 5.0, 6, False, init_image=photo, strength=0.1)
    with pytest.raises(ValueError, match="strength"):
        call(pipe, image, lat0, "ddim", 0.0, 5.0, 6, False, init_image=photo, strength=0.0)
    enc, pipe.vae_encoder = pipe.vae_encoder, None
    try:
        with pytest.raises(ValueError, match="vae_encoder"):
            call(pipe, image, lat0, "ddim", 0.0, 5.0, 6, False, init_image=photo)
    finally:
        pipe.vae_encoder = enc
