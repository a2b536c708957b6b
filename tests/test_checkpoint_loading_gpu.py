"""-m gpu: weights loaded from a published-layout checkpoint reach the kernels.  Each tiny module runs once (its prepared copies:
the VAE's _prepare cache, the text encoder's fused q|k|v and graphs, the ViT's PreparedLinears, the UNet's weight-offset banks and
time-embedding concatenation), then loads the fake snapshot and runs again: bit-identical to a fresh module loaded from the same
files.  And one pre-training step from a hub id + an open_clip file equals the step from a flat .pt directory holding the same
tensors with a resumed encoder.pt, bit for bit."""
import pytest
import torch

import checkpoint_fixtures as fx
from test_cli_setup import pretrain_args

pytestmark = pytest.mark.gpu


@pytest.fixture()
def hub(tmp_path, monkeypatch):
    cache = tmp_path / "hub"
    cache.mkdir()
    monkeypatch.setenv("HF_HUB_CACHE", str(cache))
    return cache


def test_load_after_forward_leaves_no_stale_prepared_copy(hip_env, hub, tmp_path):
    from e4t import builders
    from e4t import cli_common as cc
    _, _, dev, _ = hip_env
    src = fx.source_models()
    snap = fx.write_snapshot(hub, src)
    clip = "ViT-tiny-test::" + fx.write_openclip(tmp_path / "vit.bin", src["enc"])
    g = torch.Generator().manual_seed(0)
    px = (torch.rand(2, 3, 64, 64, generator=g) * 2 - 1).to(dev)
    ids = torch.randint(3, 99, (2, 9), generator=g).to(dev)
    lat = torch.randn(2, 4, 16, 16, generator=g).to(dev)
    t = torch.tensor([10, 700], device=dev)
    ctx = torch.randn(2, 9, 64, generator=g).to(dev)

    def run(m):
        unet, enc, text, vae = m
        with torch.no_grad():
            outs = [*vae.moments(px), text(input_ids=ids)[0], *enc.clip_vision(px), unet(lat, t, ctx, return_dict=False)[0]]
        e = text.get_input_embeddings()(ids).detach().requires_grad_(True)
        outs.append(text(inputs_embeds=e)[0].detach())                 # the graph-replayed stack the training step uses
        torch.cuda.synchronize()
        return [o.detach().float().cpu() for o in outs]

    def load(m):
        unet, enc, text, vae = m
        cc.load_pipeline_weights(snap, unet=unet, text=text, vae=vae)
        cc.load_clip_tower(enc, clip)

    used = builders.build_models(dev, "tiny-test", seed=5)
    before = run(used)
    load(used)
    after = run(used)
    fresh = builders.build_models(dev, "tiny-test", seed=5)     # same seed: the same weight offsets, which no base checkpoint holds
    load(fresh)
    want = run(fresh)
    names = ["vae mean", "vae logvar", "text", "vit pooled", "vit tokens", "unet", "text (graph)"]
    for n, b, a, w in zip(names, before, after, want):
        assert torch.isfinite(w).all(), n
        assert not torch.equal(a, b), f"{n}: the load changed nothing"
        assert torch.equal(a, w), f"{n}: a prepared copy from before the load survived ({float((a - w).abs().max()):.3e})"


def test_pretrain_step_from_snapshot_equals_flat_layout(hip_env, hub, tmp_path):
    from e4t.utils import save_e4t_encoder, save_e4t_unet
    import pretrain_e4t
    _, _, dev, _ = hip_env
    src = fx.source_models()
    fx.write_snapshot(hub, src, fmt="sharded", vae_new_names=True)
    clip = "ViT-tiny-test::" + fx.write_openclip(tmp_path / "open_clip_model.safetensors", src["enc"], fmt="safetensors")
    flat = tmp_path / "flat"
    flat.mkdir()
    torch.save(fx.unet_sd(src), flat / "unet.pt")
    torch.save(fx.text_sd(src), flat / "text_encoder.pt")
    torch.save(fx.vae_sd(src), flat / "vae.pt")
    kw = dict(train_batch_size=2, resolution=64, gradient_accumulation_steps=1, scale_lr=False, learning_rate=1e-3, seed=7)

    def step(args, before_step=None):
        st = pretrain_e4t.setup(args, dev)
        if before_step is not None:
            before_step(st)
        px, ids, pidx = next(pretrain_e4t.synthetic_batches(args, dev, 0, 1, st["prompts"]))
        with torch.no_grad():
            vis = [v.float().cpu() for v in st["enc"].clip_vision(px)]
        g = torch.Generator().manual_seed(1234)       # the tiny VAE downsamples by 2: latents are 32 x 32 at 64 px
        noise, eps = (torch.randn(2, 4, 32, 32, generator=g).to(dev) for _ in range(2))
        t = torch.randint(0, 1000, (2,), generator=g).to(dev)
        losses = torch.stack([o.detach().float() for o in st["trainer"].train_step(px, ids, pidx, noise=noise, timesteps=t, vae_eps=eps)]).cpu()
        torch.cuda.synchronize()
        return dict(losses=losses, vis=vis, params=st["trainer"].flat.data.detach().cpu().clone(),
                    emb=st["text"].get_input_embeddings().weight.detach().cpu().clone())

    def resumable(st):
        """the flat directory as an E4T run: weight_offsets.pt marks it, and a run's unet.pt is the whole UNet (stock keys + offsets)"""
        save_e4t_unet(st["unet"], str(flat))
        save_e4t_encoder(st["enc"], str(flat))
        torch.save({k: v.detach().cpu() for k, v in st["unet"].state_dict().items()}, flat / "unet.pt")

    a = step(pretrain_args(pretrained_model_name_or_path="org/tiny", clip_model_name_or_path=clip, **kw), before_step=resumable)
    b = step(pretrain_args(pretrained_model_name_or_path=str(flat), **kw))
    assert torch.equal(a["emb"], b["emb"])
    assert all(torch.equal(x, y) for x, y in zip(a["vis"], b["vis"]))
    assert torch.isfinite(a["losses"]).all() and torch.equal(a["losses"], b["losses"]), (a["losses"], b["losses"])
    assert torch.equal(a["params"], b["params"]), float((a["params"] - b["params"]).abs().max())
