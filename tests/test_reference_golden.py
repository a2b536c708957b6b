"""CPU: the oracle against what THE REFERENCE'S OWN CODE computed (tests/golden/reference_*.pt, generated in the build
container by tests/golden/make_golden_models.py, which runs /root/reference/e4t/models/*.py and e4t/encoder.py unmodified
on stand-ins for their third-party imports; `make_golden_models.py --check` regenerates them and compares).  This pins the oracle for everything the reference itself wrote — the
weight-offset modulated attention processors (math and SDPA paths), transformer blocks, UNet block wiring, the 13-map
early return, the sample output, the gradients of all 96 x 9 weight-offset tensors, the E4T encoder head — leaving only
the restated third-party leaves (ResnetBlock2D, Down/Upsample2D, time embedding, the ViT, the bicubic resize) unpinned."""
import os

import pytest
import torch

import e4t_oracle as orc
from test_unet_host_logic import emu_fp32  # noqa: F401

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def unpack(packed):
    flat, spec = packed
    out, o = {}, 0
    for name, shape in spec:
        n = 1
        for d in shape:
            n *= d
        out[name] = flat[o:o + n].view(shape).clone()
        o += n
    assert o == flat.numel()
    return out


def close(a, b, what, rtol=2e-5, atol=2e-6):
    torch.testing.assert_close(a, b, rtol=rtol, atol=atol, msg=lambda m: f"{what}: {m}")


@pytest.mark.parametrize("variant", ["sd1", "sd2"])
def test_unet_matches_reference_code(variant):
    blob = torch.load(os.path.join(GOLD, "reference_unet.pt"))[variant]
    unet = orc.UNet2DConditionModel(**blob["config"])
    sd = unpack(blob["state_dict"])
    missing, unexpected = unet.load_state_dict(sd, strict=True)
    assert not missing and not unexpected                                   # same parameter names as the reference's state dict
    enc = unet(blob["sample"], blob["timestep"], blob["ctx"], return_encoder_outputs=True)["down_block_samples"]
    assert len(enc) == 13 and sum(e.shape[1] for e in enc) == sum(e.shape[1] for e in blob["down_block_samples"])
    for i, (a, b) in enumerate(zip(enc, blob["down_block_samples"])):
        close(a, b, f"encoder map {i}")
    out = unet(blob["sample"], blob["timestep"], blob["ctx"])
    out = out.sample if hasattr(out, "sample") else out
    close(out, blob["out"], "sample")
    one = unet(blob["sample"][:1], 500, blob["ctx"][:1])
    close(one.sample if hasattr(one, "sample") else one, blob["out_scalar_t"], "python-int timestep")
    (out * blob["G"]).sum().backward()
    want = unpack(blob["wo_grads"])
    got = {n: p.grad for n, p in unet.named_parameters() if "wo" in n}
    assert got.keys() == want.keys() and len(want) == 96 * 9
    for n in want:
        close(got[n], want[n], f"grad {n}", rtol=2e-4, atol=2e-6)
    close(unet.conv_in.weight.grad, blob["grad_conv_in"], "grad conv_in", rtol=2e-4, atol=2e-5)      # the deepest gradient: fp32 summation order


@pytest.mark.parametrize("kind", ["self", "cross"])
def test_attention_processors_match_reference_code(kind):
    blob = torch.load(os.path.join(GOLD, "reference_attention.pt"))[kind]
    attn = orc.CrossAttention(**blob["kwargs"])
    attn.load_state_dict(unpack(blob["state_dict"]), strict=True)
    close(blob["math"]["out"], blob["sdpa"]["out"], "the reference's two processors agree with each other", rtol=1e-5, atol=1e-6)
    y = attn(blob["x"], blob["ctx"])
    close(y, blob["math"]["out"], "CrossAttnProcessor output")
    close(y, blob["sdpa"]["out"], "AttnProcessor2_0 output")
    y.square().sum().backward()
    want = unpack(blob["sdpa"]["grads"])
    for n, p in attn.named_parameters():
        close(p.grad, want[n], f"grad {n}", rtol=2e-4, atol=2e-6)


def test_e4t_encoder_matches_reference_code():
    blob = torch.load(os.path.join(GOLD, "reference_encoder.pt"))
    vit = dict(image_size=224, patch_size=56, width=8, layers=2, heads=2, mlp_ratio=2.0)
    enc = orc.E4TEncoder(vit_cfg=vit, freeze_clip_vision=False, **blob["kwargs"])
    sd = unpack(blob["state_dict"])
    missing, unexpected = enc.load_state_dict(sd, strict=False)
    assert not unexpected and all(k in ("mean", "std") for k in missing)   # the reference registers mean/std as non-persistent buffers
    y = enc(blob["x"], tuple(blob["maps"]))
    close(y, blob["out"], "domain embedding")
    y.square().sum().backward()
    want = unpack(blob["grads"])
    got = {n: p.grad for n, p in enc.named_parameters() if p.grad is not None}
    assert got.keys() == want.keys()
    for n in want:
        close(got[n], want[n], f"grad {n}", rtol=2e-4, atol=2e-6)
    pre = orc.clip_preprocess(blob["x"]) if hasattr(orc, "clip_preprocess") else enc.preprocess(blob["x"])
    close(pre[:, :, ::16, ::16], blob["preprocessed"], "CLIP input (224 x 224 bicubic, normalised)")


@pytest.mark.parametrize("guidance", [1.0, 3.0])
def test_sampling_loop_matches_reference_pipeline(guidance):
    """oracle e4t_sample + DDIMScheduler against the reference's StableDiffusionE4TPipeline.__call__ (run on the reference UNet
    with the 'sd1' fixture weights, a stand-in E4T encoder, the torch CLIP text twin and the offline tokenizer)"""
    import sys
    sys.path.insert(0, GOLD)
    from standin import PROMPT, TEXT_CFG, StandInEncoder
    from torch_twins import CLIPTextModel
    from e4t.utils import WhitespaceTokenizer
    ub = torch.load(os.path.join(GOLD, "reference_unet.pt"))["sd1"]
    pb = torch.load(os.path.join(GOLD, "reference_pipeline.pt"))
    cfg = ub["config"]
    unet = orc.UNet2DConditionModel(**cfg)
    unet.load_state_dict(unpack(ub["state_dict"]))
    text = CLIPTextModel(**dict(TEXT_CFG, hidden_size=cfg["cross_attention_dim"])).requires_grad_(False)
    tok = WhitespaceTokenizer()
    assert tok.add_tokens("*s") == 1 and tok.convert_tokens_to_ids("*s") == pb["placeholder_id"]
    text.resize_token_embeddings(len(tok))
    text.load_state_dict(unpack(pb["text_state"]))
    boc = cfg["block_out_channels"]
    enc = StandInEncoder(sum(2 * c for c in boc) + boc[0] + sum(boc[:-1]) + boc[-1], cfg["cross_attention_dim"])
    kw = dict(padding="max_length", truncation=True, max_length=tok.model_max_length, return_tensors="pt")
    ids = tok(PROMPT, **kw).input_ids
    idx = ids[0].tolist().index(pb["placeholder_id"])
    with torch.no_grad():
        emb = text.get_input_embeddings()(ids)
        ctx0 = text(tok("", **kw).input_ids)[0]
        class_embed = text.get_input_embeddings()(tok("art", add_special_tokens=False).input_ids[0])
    got = orc.e4t_sample(unet, enc, lambda inputs_embeds: text(inputs_embeds=inputs_embeds)[0], orc.DDIMScheduler(), pb["image"], emb, idx,
                         ctx0, class_embed, pb["latents"].clone(), num_inference_steps=pb["steps"], guidance_scale=guidance)
    close(got, pb["final"][guidance], f"final latents, guidance {guidance}", rtol=1e-4, atol=1e-5)


def test_native_unet_matches_reference_code_directly(emu_fp32):
    """The NATIVE UNet (host graph + hand-written backward orchestration, through the fp32 op emulation) against what the
    reference's own UNet computed at a width the native modules support — no oracle in between.  Weights are a deterministic
    function of the parameter names (tests/golden/standin.py), so the fixture holds only inputs and reference outputs."""
    import sys
    sys.path.insert(0, GOLD)
    from standin import deterministic_fill
    from e4t.models.unet_2d_condition import UNet2DConditionModel
    blob = torch.load(os.path.join(GOLD, "reference_unet_wide.pt"))
    want_g = unpack(blob["wo_grads"])
    for kind in ("oracle", "native"):
        unet = deterministic_fill((orc.UNet2DConditionModel if kind == "oracle" else UNet2DConditionModel)(**blob["config"]), salt=blob["salt"])
        enc = unet(blob["sample"], blob["timestep"], blob["ctx"], return_encoder_outputs=True)["down_block_samples"]
        tol = dict(rtol=5e-5, atol=1e-5) if kind == "oracle" else dict(rtol=2e-3, atol=2e-4)      # native: bf16-free emulation, different op order
        for i, (a, b) in enumerate(zip(enc, blob["down_block_samples"])):
            close(a.float(), b, f"{kind} encoder map {i}", **tol)
        out = unet(blob["sample"], blob["timestep"], blob["ctx"])
        out = out.sample if hasattr(out, "sample") else out
        close(out.float(), blob["out"], f"{kind} sample", **tol)
        (out.float() * blob["G"]).sum().backward()
        got = dict(unet.named_parameters())
        for n, g in want_g.items():
            close(got[n].grad, g, f"{kind} grad {n}", rtol=5e-3 if kind == "native" else 5e-4, atol=5e-4 if kind == "native" else 5e-6)


def test_native_e4t_encoder_matches_reference_code_directly(emu_fp32):
    """the NATIVE E4TEncoder (ViT on the op backend, grouped 129-slot-style head with its hand-written backward) through the
    fp32 emulation against the reference's own E4TEncoder at ViT width 64 — name-derived weights, no oracle in between"""
    import sys
    sys.path.insert(0, GOLD)
    from standin import deterministic_fill
    from e4t.encoder import E4TEncoder
    blob = torch.load(os.path.join(GOLD, "reference_encoder_wide.pt"))
    vit = dict(image_size=224, patch_size=56, width=64, layers=2, heads=2, mlp_ratio=2.0)
    want_g = unpack(blob["grads"])
    for kind in ("oracle", "native"):
        if kind == "oracle":
            enc = orc.E4TEncoder(vit_cfg=vit, freeze_clip_vision=False, **blob["kwargs"])
        else:
            enc = E4TEncoder(arch="ViT-golden-wide", vit_cfg=vit, freeze_clip_vision=False, **blob["kwargs"])
        deterministic_fill(enc, salt=blob["salt"])
        y = enc(blob["x"], tuple(blob["maps"]))
        tol = dict(rtol=5e-5, atol=1e-5) if kind == "oracle" else dict(rtol=2e-3, atol=2e-4)
        close(y.float(), blob["out"], f"{kind} domain embedding", **tol)
        y.float().square().sum().backward()
        got = dict(enc.named_parameters())
        for n, g in want_g.items():
            close(got[n].grad, g, f"{kind} grad {n}", rtol=5e-3 if kind == "native" else 5e-4, atol=1e-3 if kind == "native" else 1e-5)


@pytest.mark.parametrize("guidance", [1.0, 4.0])
def test_native_pipeline_matches_reference_pipeline_directly(emu_fp32, guidance):
    """this repository's StableDiffusionE4TPipeline (native UNet + text encoder through the emulation, fused guidance/DDIM
    update, per-call hoisting) against the final latents of the reference's pipeline __call__ on the same name-derived weights"""
    import sys
    sys.path.insert(0, GOLD)
    from standin import PROMPT, TEXT_CFG, StandInEncoder, deterministic_fill
    from e4t.models.unet_2d_condition import UNet2DConditionModel
    from e4t.pipeline_stable_diffusion_e4t import StableDiffusionE4TPipeline
    from e4t.schedulers import DDIMScheduler
    from e4t.text import CLIPTextModel
    from e4t.utils import WhitespaceTokenizer
    blob = torch.load(os.path.join(GOLD, "reference_pipeline_wide.pt"))
    cfg = blob["config"]
    unet = deterministic_fill(UNet2DConditionModel(**cfg), salt=31).requires_grad_(False)
    tok = WhitespaceTokenizer()
    tok.add_tokens("*s")
    text = deterministic_fill(CLIPTextModel(**dict(TEXT_CFG, hidden_size=64, intermediate_size=128, vocab_size=len(tok))), salt=32).requires_grad_(False)
    boc = cfg["block_out_channels"]
    enc = StandInEncoder(sum(2 * c for c in boc) + boc[0] + sum(boc[:-1]) + boc[-1], 64)
    vae = type("V", (), {"block_out_channels": (1, 1, 1, 1)})()
    pipe = StableDiffusionE4TPipeline(vae=vae, text_encoder=text, tokenizer=tok, unet=unet, e4t_encoder=enc, scheduler=DDIMScheduler.stable_diffusion(),
                                      e4t_config=dict(placeholder_token="*s", domain_class_token="art", domain_embed_scale=0.1),
                                      already_added_placeholder_token=True)
    out = pipe(PROMPT, height=64, width=64, num_inference_steps=blob["steps"], guidance_scale=guidance, num_images_per_prompt=2,
               latents=blob["latents"].clone(), image=blob["image"], output_type="latent", use_graph=False).images
    close(out, blob["final"][guidance], f"final latents, guidance {guidance}", rtol=3e-3, atol=3e-4)


def test_training_step_matches_reference_lines():
    """oracle e4t_losses + torch AdamW against what pretrain_e4t.py:561-584,597-654 computed when those lines were executed
    verbatim (tests/golden/make_golden_models.py::step_fixture): class embedding, ""-context, latents, both UNet passes, the
    embedding injection, loss_diff / loss_reg / loss, every weight-offset gradient and the parameters after the optimiser step"""
    import sys
    import torch.nn.functional as F
    sys.path.insert(0, GOLD)
    from standin import TEXT_CFG, StandInEncoder
    from torch_twins import CLIPTextModel
    from e4t.utils import WhitespaceTokenizer
    ub = torch.load(os.path.join(GOLD, "reference_unet.pt"))["sd1"]
    sb = torch.load(os.path.join(GOLD, "reference_step.pt"))
    cfg = ub["config"]
    unet = orc.UNet2DConditionModel(**cfg)
    unet.load_state_dict(unpack(ub["state_dict"]))
    for n, p in unet.named_parameters():
        p.requires_grad_("wo" in n)
    d = cfg["cross_attention_dim"]
    tok = WhitespaceTokenizer()
    tok.add_tokens("*s")
    text = CLIPTextModel(**dict(TEXT_CFG, hidden_size=d, vocab_size=len(tok))).requires_grad_(False)
    text.load_state_dict(unpack(sb["text_state"]))
    boc = cfg["block_out_channels"]
    enc = StandInEncoder(sum(2 * c for c in boc) + boc[0] + sum(boc[:-1]) + boc[-1], d)
    enc.w.requires_grad_(True)
    # prelude (:561-584)
    kw = dict(padding="max_length", truncation=True, max_length=tok.model_max_length, return_tensors="pt")
    with torch.no_grad():
        class_embed = text.get_input_embeddings()(tok("art", add_special_tokens=False).input_ids[0])
        ctx0 = text(tok("", **kw).input_ids)[0]
    close(class_embed, sb["class_embed"], "class embedding")
    close(ctx0, sb["ctx_for_e4t"], '""-prompt context')
    # the VAE stand-in's latents (:597-599) and the prompt the reference built (:609-616)
    lat = torch.einsum("lc,bchw->blhw", sb["vae_P"], F.avg_pool2d(sb["pixel_values"], 8)) * 0.18215
    close(lat, sb["latents"], "latents")
    ids = tok(["a photo of *s"] * 2, **kw).input_ids
    assert torch.equal(ids, sb["input_ids"]) and [r.index(tok.convert_tokens_to_ids("*s")) for r in ids.tolist()] == sb["placeholder_idxs"]
    with torch.no_grad():
        emb = text.get_input_embeddings()(ids)
    params = [enc.w] + [p for n, p in unet.named_parameters() if "wo" in n]
    opt = torch.optim.AdamW(params, lr=1e-3)
    loss, ld, lr_, aux = orc.e4t_losses(unet, enc, lambda inputs_embeds: text(inputs_embeds=inputs_embeds)[0], sb["pixel_values"], lat, sb["noise"],
                                        sb["timesteps"], emb, sb["placeholder_idxs"], ctx0, class_embed, orc.ddpm_alphas_cumprod(), reg_lambda=0.01)
    close(aux["domain_embed"], sb["domain_embed"], "domain embedding")
    pred = aux["pred"].sample if hasattr(aux["pred"], "sample") else aux["pred"]
    close(pred, sb["model_pred"], "model_pred")
    close(ld, sb["loss_diff"], "loss_diff")
    close(lr_, sb["loss_reg"], "loss_reg")
    close(loss, sb["loss"], "loss")
    loss.backward()
    want = unpack(sb["grads"])
    close(enc.w.grad, want.pop("__enc_w"), "grad encoder", rtol=2e-4, atol=2e-6)
    named = dict(unet.named_parameters())
    for n, g in want.items():
        close(named[n].grad, g, f"grad {n}", rtol=2e-4, atol=2e-6)
    opt.step()
    after = unpack(sb["params_after"])
    bad = 0
    for n, v in after.items():
        bad += int(((named[n].detach() - v).abs() > 1e-5).sum())        # Adam's first step is sign-like: tolerate flips where |g| is rounding noise
    assert bad <= 5, bad
    assert int(((enc.w.detach() - sb["enc_w_after"]).abs() > 1e-5).sum()) <= 2


def test_tuning_step_matches_reference_lines():
    """oracle step with every UNet parameter trainable + clip_grad_norm_(1.0) + AdamW against tuning_e4t.py:266-269,272-338 exec'd
    verbatim: latents of the expanded image, losses, the global gradient norm, clipped gradients and post-step parameters"""
    import sys
    import torch.nn.functional as F
    sys.path.insert(0, GOLD)
    from standin import TEXT_CFG, StandInEncoder
    from torch_twins import CLIPTextModel
    from e4t.utils import WhitespaceTokenizer
    ub = torch.load(os.path.join(GOLD, "reference_unet.pt"))["sd1"]
    sb = torch.load(os.path.join(GOLD, "reference_tuning_step.pt"))
    cfg = ub["config"]
    unet = orc.UNet2DConditionModel(**cfg)
    unet.load_state_dict(unpack(ub["state_dict"]))
    d = cfg["cross_attention_dim"]
    tok = WhitespaceTokenizer()
    tok.add_tokens("*s")
    text = CLIPTextModel(**dict(TEXT_CFG, hidden_size=d, vocab_size=len(tok))).requires_grad_(False)
    text.load_state_dict(unpack(sb["text_state"]))
    boc = cfg["block_out_channels"]
    enc = StandInEncoder(sum(2 * c for c in boc) + boc[0] + sum(boc[:-1]) + boc[-1], d)
    enc.w.requires_grad_(True)
    B = 3
    px = sb["image"].expand(B, -1, -1, -1)
    lat = torch.einsum("lc,bchw->blhw", sb["vae_P"], F.avg_pool2d(px, 8)) * 0.18215
    close(lat, sb["latents"], "latents (computed once, :266-269)")
    kw = dict(padding="max_length", truncation=True, max_length=tok.model_max_length, return_tensors="pt")
    ids = tok(["a photo of *s"] * B, **kw).input_ids
    assert torch.equal(ids, sb["input_ids"])
    with torch.no_grad():
        class_embed = text.get_input_embeddings()(tok("art", add_special_tokens=False).input_ids[0])
        ctx0 = text(tok("", **kw).input_ids)[0]
        emb = text.get_input_embeddings()(ids)
    params = [enc.w] + list(unet.parameters())
    opt = torch.optim.AdamW(params, lr=1e-3)
    loss, ld, lr_, _ = orc.e4t_losses(unet, enc, lambda inputs_embeds: text(inputs_embeds=inputs_embeds)[0], px, lat, sb["noise"], sb["timesteps"], emb,
                                      sb["placeholder_idxs"], ctx0, class_embed, orc.ddpm_alphas_cumprod(), reg_lambda=0.1)
    close(ld, sb["loss_diff"], "loss_diff")
    close(lr_, sb["loss_reg"], "loss_reg")
    close(loss, sb["loss"], "loss")
    loss.backward()
    total = torch.nn.utils.clip_grad_norm_(params, 1.0)
    close(total, sb["total_norm"], "global gradient norm", rtol=1e-4, atol=1e-6)
    want = unpack(sb["grads"])
    close(enc.w.grad, want.pop("__enc_w"), "clipped grad encoder", rtol=3e-4, atol=3e-6)
    named = dict(unet.named_parameters())
    for n, g in want.items():
        close(named[n].grad, g, f"clipped grad {n}", rtol=3e-4, atol=3e-6)
    opt.step()
    bad = sum(int(((named[n].detach() - v).abs() > 1e-5).sum()) for n, v in unpack(sb["params_after"]).items())
    assert bad <= 5, bad
