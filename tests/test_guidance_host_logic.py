"""CPU: guidance rescale and identity guidance above the kernels.  ``schedulers.combine_guidance`` (the definition)
against its own properties; the pipeline's two options on the tiny models (op emulation in fp32, so the generic loop) against a
loop written here from the oracle's modules and the definition evaluated in float64; the wiring of the three-branch batch; that
a call with neither option stays away from the new ops; argument errors of the pipeline, of the C entry points (validated on
the host before any launch) and of inference.py's two flags."""
import os
import sys

import pytest
import torch

import e4t_oracle as orc
from emu_backend import EmuBackend
from test_pipeline_host_logic import _pipeline
from test_train_step_host_logic import build
from test_unet_host_logic import emu_fp32  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f64 = torch.float64


def test_combine_guidance_properties():
    from e4t.schedulers import combine_guidance
    g = torch.Generator().manual_seed(0)
    mean = torch.tensor([0.0, 3.0, -2.0, 10.0], dtype=f64).view(4, 1, 1, 1)
    sd = torch.tensor([1.0, 0.05, 4.0, 0.01], dtype=f64).view(4, 1, 1, 1)
    u, k, c = (mean + sd * torch.randn(4, 4, 7, 9, generator=g, dtype=f64) for _ in range(3))
    two = combine_guidance((u, c), 7.5)
    assert torch.equal(two, u + 7.5 * (c - u)) and two.dtype == f64
    # g_id = g (given or defaulted) is two-branch guidance on c, whatever k holds
    for g_id in (7.5, None):
        assert float((combine_guidance((u, k, c), 7.5, g_id) - two).abs().max() / two.abs().max()) <= 1e-12
    three = combine_guidance((u, k, c), 7.5, 10.0)
    torch.testing.assert_close(three, u + 7.5 * (k - u) + 10.0 * (c - k), rtol=1e-12, atol=0)
    assert not torch.allclose(three, two)
    # rescale = 0: the guided value itself; rescale = 1: every image's deviation is the conditional branch's
    assert torch.equal(combine_guidance((u, k, c), 7.5, 10.0, rescale=0.0), three)
    for br, e0 in (((u, c), two), ((u, k, c), three)):
        full = combine_guidance(br, 7.5, 10.0, rescale=1.0)
        torch.testing.assert_close(full.reshape(4, -1).std(dim=1), c.reshape(4, -1).std(dim=1), rtol=1e-12, atol=0)
        f = (c.reshape(4, -1).std(dim=1) / e0.reshape(4, -1).std(dim=1)).view(4, 1, 1, 1)
        torch.testing.assert_close(combine_guidance(br, 7.5, 10.0, rescale=0.7), (0.3 + 0.7 * f) * e0, rtol=1e-12, atol=0)
        assert len(set(f.flatten().tolist())) == 4                                  # one factor per image
    # a constant e0 (u == c, or one value per branch): factor 1, not 0/0
    const = torch.full((2, 4, 3, 3), 0.5, dtype=f64)
    assert torch.equal(combine_guidance((const, const), 7.5, rescale=1.0), const)
    assert torch.equal(combine_guidance((const, 3 * const, const), 7.5, 10.0, rescale=0.7), const + 7.5 * (2 * const) + 10.0 * (-2 * const))
    # any dtype
    assert combine_guidance((u.float(), k.float(), c.float()), 7.5, 10.0, rescale=0.7).dtype == torch.float32


def _setup():
    from e4t.vae import VAEDecoder
    r_unet, r_enc, n_unet, n_enc, text = build()
    torch.manual_seed(3)
    vae = VAEDecoder(block_out_channels=(64, 64)).requires_grad_(False)
    pipe, tok = _pipeline(n_unet, n_enc, text, vae)
    g = torch.Generator().manual_seed(5)
    image = torch.rand(1, 3, 64, 64, generator=g) * 2 - 1
    lat0 = torch.randn(2, 4, 16, 16, generator=g)
    return pipe, tok, text, r_unet, r_enc, image, lat0


def oracle_loop(r_unet, r_enc, text, tok, scheduler, image, latents, steps, g, g_id, rescale, domain_embed_scale=0.1):
    """e4t_oracle.e4t_sample's loop (the reference's :160-218) with the class-word branch and the definition in float64"""
    from e4t.schedulers import combine_guidance
    ids = tok("a painting of *s", padding="max_length", max_length=9).input_ids
    idx = ids[0].tolist().index(tok.convert_tokens_to_ids("*s"))
    with torch.no_grad():
        emb0 = text.get_input_embeddings()(ids)
        ctx0 = text(tok("", padding="max_length", max_length=9).input_ids)[0]
        class_embed = text.get_input_embeddings()(torch.tensor([11]))
        emb_k = emb0.clone()
        emb_k[:, idx, :] = class_embed
        ctx_k = text(inputs_embeds=emb_k)[0]
        scheduler.set_timesteps(steps)
        latents = latents * scheduler.init_noise_sigma
        bsz = latents.shape[0]
        n = 2 if g_id is None else 3
        for t in scheduler.timesteps:
            x_in = scheduler.scale_model_input(latents, t)
            ctx_e = ctx0.expand(bsz, -1, -1)
            enc = r_unet(x_in, t.expand(bsz), ctx_e, return_encoder_outputs=True)
            domain = class_embed.clone().expand(bsz, -1) + domain_embed_scale * r_enc(image.expand(bsz, -1, -1, -1), enc["down_block_samples"])
            emb = emb0.expand(bsz, -1, -1).clone()
            emb[:, idx, :] = domain
            ctx = text(inputs_embeds=emb)[0]
            prompt = [ctx_e, ctx] if g_id is None else [ctx_e, ctx_k.expand(bsz, -1, -1), ctx]
            pred = r_unet(torch.cat([x_in] * n), t.expand(n * bsz), torch.cat(prompt))
            pred = combine_guidance([b.double() for b in pred.chunk(n)], g, g_id, rescale).float()
            out = scheduler.step(pred, t, latents)
            latents = getattr(out, "prev_sample", out)
    return latents


OPTIONS = {"rescale": dict(guidance_rescale=0.7), "identity": dict(identity_guidance_scale=6.5),
           "both": dict(guidance_rescale=0.7, identity_guidance_scale=6.5)}


@pytest.mark.parametrize("sampler", ["ddim", "euler"])
@pytest.mark.parametrize("option", list(OPTIONS))
def test_pipeline_options_match_oracle_loop(emu_fp32, sampler, option):
    from e4t.schedulers import SCHEDULER_MAPPING
    pipe, tok, text, r_unet, r_enc, image, lat0 = _setup()
    kw = OPTIONS[option]
    if sampler == "ddim":
        ref_sch = orc.DDIMScheduler()
    else:
        pipe.scheduler = SCHEDULER_MAPPING[sampler].stable_diffusion()
        ref_sch = SCHEDULER_MAPPING[sampler].stable_diffusion()          # the oracle has DDIM only: the sigma sampler's own step()
    batches = []
    forward = pipe.unet.forward
    pipe.unet.forward = lambda x, *a, **k: (batches.append(x.shape[0]), forward(x, *a, **k))[1]
    steps = 3
    out = pipe("a painting of *s", height=32, width=32, num_inference_steps=steps, guidance_scale=4.0, num_images_per_prompt=2,
               latents=lat0.clone(), image=image, output_type="latent", **kw).images
    three = "identity_guidance_scale" in kw
    assert batches == [2, 6 if three else 4] * steps                     # the encoder pass, then the guided batch: 3 * bsz with the class word
    want = oracle_loop(r_unet, r_enc, text, tok, ref_sch, image, lat0.clone(), steps, 4.0, kw.get("identity_guidance_scale"),
                       kw.get("guidance_rescale", 0.0))
    torch.testing.assert_close(out, want, rtol=2e-3, atol=2e-4)
    plain = pipe("a painting of *s", height=32, width=32, num_inference_steps=steps, guidance_scale=4.0, num_images_per_prompt=2,
                 latents=lat0.clone(), image=image, output_type="latent").images
    assert not torch.allclose(out, plain, rtol=2e-3, atol=2e-4)          # the option is not a no-op at this tolerance


def test_class_word_context_is_the_conditional_context_at_scale_zero(emu_fp32):
    pipe, tok, text, r_unet, r_enc, image, lat0 = _setup()
    seen = []
    forward = pipe.unet.forward
    pipe.unet.forward = lambda x, t, ctx, *a, **k: (seen.append(ctx), forward(x, t, ctx, *a, **k))[1]
    pipe("a painting of *s", height=32, width=32, num_inference_steps=1, guidance_scale=4.0, num_images_per_prompt=2, latents=lat0.clone(),
         image=image, output_type="latent", identity_guidance_scale=6.0, domain_embed_scale=0.0)
    ctx_e, ctx_k, ctx = seen[1].chunk(3)
    torch.testing.assert_close(ctx_k, ctx, rtol=1e-6, atol=1e-7)
    assert not torch.allclose(ctx_k, ctx_e)
    torch.testing.assert_close(ctx_k[:1], pipe.class_word_context(pipe.prepare_for_e4t("a painting of *s", pipe.device)), rtol=0, atol=0)
    assert torch.equal(ctx_k[0], ctx_k[1])                               # one context for every image


class SpyBackend(EmuBackend):
    """the op emulation plus the names of the new ops, recording every use"""

    def __init__(self):
        super().__init__(round_bf16=False)
        self.used = []

    def guidance_stats(self, *a, **k):
        self.used.append("guidance_stats")
        raise AssertionError("guidance_stats reached")

    def sampler_step_guided(self, *a, **k):
        self.used.append("sampler_step_guided")
        raise AssertionError("sampler_step_guided reached")

    def guided_step(self, *a, cfg=True, **k):
        if cfg:                                                          # (DDIMScheduler.step itself runs it with cfg=False)
            self.used.append("guided_step")
        return super().guided_step(*a, cfg=cfg, **k)


def test_plain_call_stays_away_from_the_new_ops_and_options_take_the_generic_loop(emu_fp32):
    pipe, tok, text, r_unet, r_enc, image, lat0 = _setup()
    spy = SpyBackend()
    old = emu_fp32.set_backend(spy)
    try:
        kw = dict(height=32, width=32, num_inference_steps=2, guidance_scale=4.0, num_images_per_prompt=2, image=image, output_type="latent")
        pipe("a painting of *s", latents=lat0.clone(), **kw)
        assert spy.used == ["guided_step"] * 2                           # DDIM with eta == 0 on the emulation: the fused update it had
        spy.used.clear()
        for opt in OPTIONS.values():                                     # no e4t_sampler_step on this backend: the generic loop
            pipe("a painting of *s", latents=lat0.clone(), **kw, **opt)
            assert spy.used == []
            with pytest.raises(ValueError, match="graph replay"):
                pipe("a painting of *s", latents=lat0.clone(), use_graph=True, **kw, **opt)
    finally:
        emu_fp32.set_backend(old)


def test_pipeline_refuses_bad_guidance_arguments(emu_fp32):
    pipe, tok, text, r_unet, r_enc, image, lat0 = _setup()
    kw = dict(height=32, width=32, num_inference_steps=1, image=image, output_type="latent", latents=lat0[:1].clone())
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="guidance_rescale"):
            pipe("a painting of *s", guidance_scale=4.0, guidance_rescale=bad, **kw)
    with pytest.raises(ValueError, match="identity_guidance_scale"):
        pipe("a painting of *s", guidance_scale=4.0, identity_guidance_scale=-1.0, **kw)
    for opt in OPTIONS.values():
        with pytest.raises(ValueError, match="guidance_scale` > 1"):
            pipe("a painting of *s", guidance_scale=1.0, **opt, **kw)
    pipe("a painting of *s", guidance_scale=1.0, guidance_rescale=0.0, **kw)                 # 0 is "not given"
    pipe("a painting of *s", guidance_scale=4.0, guidance_rescale=1.0, identity_guidance_scale=0.0, **kw)    # the closed ends are allowed


def test_entry_points_reject_bad_arguments():
    """e4t_guidance_stats / e4t_sampler_step_guided validate on the host before any launch (safe without a GPU)"""
    from e4t import _C
    lib = _C.load()
    p = 4096                                                              # never dereferenced: every call below fails validation

    def stats(pred=p, gp=p, gstat=p, B=1, C=4, HW=64, branches=2):
        return lib.e4t_guidance_stats(pred, gp, gstat, B, C, HW, branches, 0, None)

    for br in (1, 4, 0):
        assert stats(branches=br) == -22 and b"branches" in lib.e4t_last_error()
    assert stats(C=1, HW=1) == -22 and b"N = " in lib.e4t_last_error()
    for name in ("pred", "gp", "gstat"):
        assert stats(**{name: None}) == -22 and name.encode() in lib.e4t_last_error()
    assert stats(B=0) == -22

    def step(keep=None, x0=None, n0=None, K=0, hist=None, copies=0, x_in=None, branches=2, gp=p, kpi=0, xpi=0):
        return lib.e4t_sampler_step_guided(p, p, p, hist, None, None, x_in, p, gp, None, keep, x0, n0, 1, 4, 64, K, branches, 1, copies, kpi, xpi, None)

    for mixed in ((p, None, None), (None, p, None), (None, None, p), (p, p, None), (p, None, p), (None, p, p)):
        assert step(*mixed) == -22 and b"keep, x0 and n0" in lib.e4t_last_error()
    assert step(copies=4, x_in=p) == -22 and b"x_in_copies = 4 (0..3" in lib.e4t_last_error()
    assert step(copies=1) == -22
    assert step(branches=1) == -22 and b"branches" in lib.e4t_last_error()
    assert step(gp=None) == -22
    assert step(K=5, hist=p) == -22 and b"history slots" in lib.e4t_last_error()
    assert step(p, p, p, kpi=2) == -22 and b"keep_per_image" in lib.e4t_last_error()


def parse(monkeypatch, *argv):
    monkeypatch.syspath_prepend(ROOT)
    import inference
    monkeypatch.setattr(sys, "argv", ["inference.py", *argv])
    return inference.parse_args()


def test_inference_cli_parses_the_guidance_flags(monkeypatch, capsys):
    args = parse(monkeypatch)
    assert args.guidance_rescale == 0.0 and args.identity_guidance_scale is None
    args = parse(monkeypatch, "--guidance_scale", "7.5", "--guidance_rescale", "0.7", "--identity_guidance_scale", "10")
    assert args.guidance_rescale == 0.7 and args.identity_guidance_scale == 10.0
    for bad in (("--guidance_scale", "7.5", "--guidance_rescale", "1.5"), ("--guidance_scale", "7.5", "--identity_guidance_scale", "-1"),
                ("--guidance_rescale", "0.7"), ("--identity_guidance_scale", "5")):
        with pytest.raises(SystemExit):
            parse(monkeypatch, *bad)
    assert "guidance_scale > 1" in capsys.readouterr().err
