"""CPU: Stable Diffusion and OpenCLIP weights from published-layout checkpoints (e4t/checkpoints.py, e4t/cli_common.py): hub ids
resolved in a local Hugging Face cache, the diffusers pipeline layout in safetensors / bin / sharded / fp16 form, config.json ->
native architecture, new VAE attention names, the open_clip vision tower, the CLIP-source policy of pretrain_e4t.py, and run
directories that name their base model by hub id.  Every fixture is written under tmp_path (tests/checkpoint_fixtures.py); the
network is switched off for the whole file."""
import argparse
import json
import os
import socket

import pytest
import torch

import checkpoint_fixtures as fx
from test_cli_setup import _write_base, pretrain_args, tuning_args
from test_unet_host_logic import emu_fp32  # noqa: F401

CPU = torch.device("cpu")


@pytest.fixture(autouse=True)
def no_network(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("checkpoint loading tried to reach the network")
    monkeypatch.setattr(socket.socket, "connect", refuse)
    monkeypatch.setattr(socket.socket, "connect_ex", refuse)


@pytest.fixture()
def hub(tmp_path, monkeypatch):
    cache = tmp_path / "hf" / "hub"
    cache.mkdir(parents=True)
    monkeypatch.setenv("HF_HUB_CACHE", str(cache))
    monkeypatch.delenv("HF_HOME", raising=False)
    return cache


def assert_same(got, want, what):
    assert set(got) == set(want), (what, set(got) ^ set(want))
    for k, v in want.items():
        assert got[k].dtype == torch.float32 and torch.equal(got[k], v.float()), (what, k)


def check_base(st, src):
    """the UNet's stock keys, the VAE encoder half, the text encoder (rows before the placeholder) equal the files' tensors"""
    usd = st["unet"].state_dict()
    for k, v in fx.unet_sd(src).items():
        assert torch.equal(usd[k], v), k
    for k, v in src["vae"].state_dict().items():
        assert torch.equal(st["vae"].state_dict()[k], v), k
    tsd = st["text"].state_dict()
    for k, v in src["text"].state_dict().items():
        assert torch.equal(tsd[k][: v.shape[0]] if "token_embedding" in k else tsd[k], v), k


def tower(enc):
    return {k: v for k, v in enc.state_dict().items() if k.startswith("clip_vision.")}


@pytest.mark.parametrize("version", ["file", "tag"])
def test_pretrain_setup_from_hub_id_and_openclip(emu_fp32, hub, tmp_path, monkeypatch, version):
    from e4t import checkpoints as ck
    import pretrain_e4t
    src = fx.source_models()
    snap = fx.write_snapshot(hub, src, tokenizer=True)
    seen = fx.patch_tokenizer(monkeypatch)
    if version == "file":
        clip = "ViT-tiny-test::" + fx.write_openclip(tmp_path / "open_clip_pytorch_model.bin", src["enc"])
    else:
        monkeypatch.setitem(ck.OPENCLIP_PRETRAINED, ("ViT-tiny-test", "tiny_tag"), "org/clip-tiny")
        fx.CacheRepo(hub, "org/clip-tiny").put("open_clip_model.safetensors", fx._bytes(fx.openclip_sd(src["enc"]), "safetensors"))
        clip = "ViT-tiny-test::tiny_tag"
    st = pretrain_e4t.setup(pretrain_args(pretrained_model_name_or_path="org/tiny", clip_model_name_or_path=clip, seed=5), CPU)
    check_base(st, src)
    assert st["text"].get_input_embeddings().weight.shape[0] == 101 and st["base_dir"] == snap
    for k, v in tower(src["enc"]).items():
        assert torch.equal(st["enc"].state_dict()[k], v), k
    assert not any(p.requires_grad for p in st["enc"].clip_vision.parameters())          # still frozen after the load
    assert seen == [os.path.join(snap, "tokenizer")]                                      # the snapshot's tokenizer, not a hub call


@pytest.mark.parametrize("fmt", ["safetensors", "bin", "sharded", "fp16"])
def test_weight_formats_read_to_the_same_fp32_tensors(hub, fmt):
    from e4t import checkpoints as ck
    src = fx.source_models()
    snap = fx.write_snapshot(hub, src, fmt=fmt)
    rnd = (lambda t: t.half().float()) if fmt == "fp16" else (lambda t: t)
    for sub, sd in (("unet", fx.unet_sd(src)), ("vae", fx.vae_sd(src)), ("text_encoder", fx.text_sd(src))):
        got = ck.read_state_dict(os.path.join(snap, sub))
        want = {k: (rnd(v) if v.is_floating_point() else v) for k, v in sd.items()}
        assert set(got) == set(want), sub
        for k, v in want.items():
            assert got[k].dtype == (torch.float32 if v.is_floating_point() else v.dtype) and torch.equal(got[k], v), (sub, k)
    if fmt in ("safetensors", "fp16"):             # the format parsed without the safetensors package gives the same tensors
        from safetensors.torch import load_file
        for f in ck.weight_files(os.path.join(snap, "unet")):
            a, b = ck.parse_safetensors(f), load_file(f)
            assert set(a) == set(b) and all(a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]) for k in a)
    # safetensors wins over bin, the full-precision file over the fp16 variant
    repo = fx.CacheRepo(hub, "org/tiny")
    fx.put_weights(repo, "unet", "diffusion_pytorch_model", {"x": torch.zeros(1)}, "bin" if fmt != "bin" else "fp16")
    assert ck.weight_files(os.path.join(snap, "unet"))[0].endswith("-00001-of-00002.safetensors" if fmt == "sharded" else
                                                                  {"safetensors": ".safetensors", "bin": ".fp16.safetensors", "fp16": ".fp16.safetensors"}[fmt])


def test_new_vae_attention_names_load_like_the_old(emu_fp32, hub, tmp_path):
    from e4t import checkpoints as ck
    from e4t import cli_common as cc
    src = fx.source_models()
    snap = fx.write_snapshot(hub, src, vae_new_names=True)
    raw = ck.read_state_dict(os.path.join(snap, "vae"))
    assert "encoder.mid_block.attentions.0.to_out.0.weight" in raw and "decoder.mid_block.attentions.0.to_q.bias" in raw
    assert_same(ck.normalize_vae_keys(raw), fx.vae_sd(src), "vae")
    _, _, _, vae = cc.build_models(CPU, "org/tiny", "tiny-test", seed=3)
    for k, v in src["vae"].state_dict().items():
        assert torch.equal(vae.state_dict()[k], v), k
    dec = cc.pipeline_vae_decoder(CPU, snap)
    for k, v in src["dec"].state_dict().items():
        assert torch.equal(dec.state_dict()[k], v), k
    with pytest.raises(ValueError, match="both the old and the new name"):
        ck.normalize_vae_keys({"encoder.mid_block.attentions.0.query.weight": 1, "encoder.mid_block.attentions.0.to_q.weight": 2})


def test_sd2_style_unet_config_builds_that_architecture(emu_fp32, hub):
    from e4t import checkpoints as ck
    from e4t import cli_common as cc
    cfg = dict(fx.TINY_UNET, attention_head_dim=[2, 4, 4, 4], use_linear_projection=True, upcast_attention=True, dual_cross_attention=False,
               only_cross_attention=False, num_class_embeds=None, class_embed_type=None, resnet_time_scale_shift="default",
               mid_block_type="UNetMidBlock2DCrossAttn", transformer_layers_per_block=1, addition_embed_type=None)
    src = fx.source_models(unet_cfg=cfg)
    fx.write_snapshot(hub, src)
    unet, _, _, _ = cc.build_models(CPU, "org/tiny", "tiny-test", seed=3)
    t = unet.down_blocks[1].attentions[0]
    assert isinstance(t.proj_in, torch.nn.Linear) and t.transformer_blocks[0].attn1.heads == 4
    assert unet.config.use_linear_projection and unet.config.upcast_attention and tuple(unet.config.attention_head_dim) == (2, 4, 4, 4)
    for k, v in fx.unet_sd(src).items():
        assert torch.equal(unet.state_dict()[k], v), k
    for bad, name in ((dict(addition_embed_type="text"), "addition_embed_type"), (dict(some_new_field=1), "some_new_field"),
                      (dict(down_block_types=["SimpleCrossAttnDownBlock2D"] + fx.TINY_UNET["down_block_types"][1:]), "SimpleCrossAttnDownBlock2D"),
                      (dict(up_block_types=fx.TINY_UNET["up_block_types"][:3] + ["AttnUpBlock2D"]), "AttnUpBlock2D"),
                      (dict(attention_head_dim=[2, 4]), "attention_head_dim"), (dict(transformer_layers_per_block=2), "transformer_layers_per_block")):
        with pytest.raises(ValueError, match=name):
            ck.unet_kwargs(dict(fx.TINY_UNET, **bad))
    with pytest.raises(ValueError, match="hidden_act"):
        ck.text_kwargs(dict(fx.TINY_TEXT, hidden_act="relu"))
    with pytest.raises(ValueError, match="layer_norm_eps"):
        ck.text_kwargs(dict(fx.TINY_TEXT, layer_norm_eps=1e-6))
    with pytest.raises(ValueError, match="layers_per_block"):
        ck.vae_kwargs(dict(fx.TINY_VAE, layers_per_block=3))
    assert ck.text_kwargs(fx.TINY_TEXT) == dict(vocab_size=100, hidden_size=64, num_layers=2, num_heads=2, intermediate_size=128, max_len=9,
                                                act="quick_gelu")


def test_openclip_checkpoint_checks(tmp_path):
    from e4t import builders
    from e4t import checkpoints as ck
    enc = builders.build_models(CPU, "tiny-test", seed=4)[1]
    for fmt in ("bin", "safetensors"):
        f = fx.write_openclip(tmp_path / f"ok.{fmt}", enc, fmt=fmt)
        arch, path = ck.resolve_clip_file(f"ViT-tiny-test::{f}")
        assert (arch, path) == ("ViT-tiny-test", f)
        assert_same(ck.read_openclip_visual(arch, path), tower(enc), fmt)         # text tower and visual.proj ignored
    with pytest.raises(ValueError, match="visual.ln_post.bias"):
        ck.read_openclip_visual("ViT-tiny-test", fx.write_openclip(tmp_path / "miss.bin", enc, drop=("visual.ln_post.bias",)))
    with pytest.raises(ValueError, match="shape"):
        ck.read_openclip_visual("ViT-tiny-test", fx.write_openclip(tmp_path / "wide.bin", enc, width=64))
    with pytest.raises(ValueError, match="ViT-H-14 tower"):
        ck.read_openclip_visual("ViT-H-14", str(tmp_path / "ok.bin"))
    with pytest.raises(ValueError, match="unknown pretrained tag 'laion9b'"):
        ck.resolve_clip_file("ViT-H-14::laion9b")
    with pytest.raises(ValueError, match="unknown tower"):
        ck.resolve_clip_file("ViT-Q-99::laion2b_s32b_b79k")
    with pytest.raises(ck.CheckpointNotFoundError, match="nowhere.bin"):
        ck.resolve_clip_file(f"ViT-tiny-test::{tmp_path / 'nowhere.bin'}")


def test_resolver_reads_the_cache_layout(hub, tmp_path, monkeypatch):
    from e4t import checkpoints as ck
    src = fx.source_models()
    snap = fx.write_snapshot(hub, src)
    assert ck.resolve_model_dir("org/tiny") == snap
    assert ck.resolve_model_dir("org/tiny", fx.COMMIT) == snap                    # a commit hash names the snapshot directly
    other = fx.CacheRepo(hub, "org/tiny", commit="f" * 40, ref="v2")
    other.put("model_index.json", "{}")
    assert ck.resolve_model_dir("org/tiny", "v2") == other.snap
    assert ck.resolve_model_dir(str(tmp_path)) == str(tmp_path)                   # an existing path is used as it is
    assert os.path.islink(os.path.join(snap, "unet", "config.json"))
    with pytest.raises(ck.CheckpointNotFoundError) as e:
        ck.resolve_model_dir("org/absent", "dev")
    assert os.path.join(str(hub), "models--org--absent", "refs", "dev") in str(e.value) and "'org/absent'" in str(e.value)
    monkeypatch.delenv("HF_HUB_CACHE")
    monkeypatch.setenv("HF_HOME", str(hub.parent))
    assert ck.resolve_model_dir("org/tiny") == snap
    monkeypatch.delenv("HF_HOME")
    monkeypatch.setenv("HOME", str(tmp_path / "home"))
    assert ck.hub_cache_dir() == os.path.join(str(tmp_path / "home"), ".cache", "huggingface", "hub")


def test_clip_source_policy(emu_fp32, hub, tmp_path, monkeypatch, capsys):
    from e4t import builders
    from e4t import checkpoints as ck
    from e4t.utils import save_e4t_encoder, save_e4t_unet
    import pretrain_e4t
    src = fx.source_models()
    snap = fx.write_snapshot(hub, src)
    monkeypatch.setitem(ck.OPENCLIP_PRETRAINED, ("ViT-tiny-test", "absent_tag"), "org/clip-absent")
    # a pipeline-layout base whose CLIP source is not on this machine: exit, listing the paths searched
    with pytest.raises(SystemExit) as e:
        pretrain_e4t.setup(pretrain_args(pretrained_model_name_or_path="org/tiny", clip_model_name_or_path="ViT-tiny-test::absent_tag"), CPU)
    assert os.path.join(str(hub), "models--org--clip-absent", "refs", "main") in str(e.value.code)
    # 'none': a randomly initialised tower (the seed's), the base still loads
    st = pretrain_e4t.setup(pretrain_args(pretrained_model_name_or_path="org/tiny", clip_model_name_or_path="none", seed=5), CPU)
    check_base(st, src)
    assert_same(tower(st["enc"]), tower(builders.build_models(CPU, "tiny-test", seed=5)[1]), "random tower")
    # the flat layout warns and runs as it does without a CLIP source
    base, _, _, _ = _write_base(tmp_path)
    capsys.readouterr()
    st = pretrain_e4t.setup(pretrain_args(pretrained_model_name_or_path=base, clip_model_name_or_path=f"ViT-tiny-test::{tmp_path / 'no.bin'}"), CPU)
    err = capsys.readouterr().err
    assert "WARNING" in err and "no.bin" in err
    ref = pretrain_e4t.setup(pretrain_args(pretrained_model_name_or_path=base), CPU)
    assert_same(st["enc"].state_dict(), ref["enc"].state_dict(), "flat layout, unresolvable CLIP")
    # ... and loads the tower when the source resolves
    clip = "ViT-tiny-test::" + fx.write_openclip(tmp_path / "vit.bin", src["enc"])
    st = pretrain_e4t.setup(pretrain_args(pretrained_model_name_or_path=base, clip_model_name_or_path=clip), CPU)
    assert_same(tower(st["enc"]), tower(src["enc"]), "flat layout + CLIP file")
    # a resumed encoder.pt wins over the CLIP source, which is then not even looked up
    other = builders.build_models(CPU, "tiny-test", seed=8)
    save_e4t_unet(other[0], snap)
    save_e4t_encoder(other[1], snap)
    st = pretrain_e4t.setup(pretrain_args(pretrained_model_name_or_path="org/tiny", clip_model_name_or_path="ViT-tiny-test::absent_tag"), CPU)
    assert_same(st["enc"].state_dict(), other[1].state_dict(), "resumed encoder")
    check_base(st, src)


def test_run_directory_naming_a_hub_id(emu_fp32, hub, tmp_path, monkeypatch):
    from e4t.utils import save_config, save_e4t_encoder, save_e4t_unet
    import inference
    import pretrain_e4t
    import tuning_e4t
    src = fx.source_models()
    snap = fx.write_snapshot(hub, src, tokenizer=True, fmt="bin")
    seen = fx.patch_tokenizer(monkeypatch)
    args = pretrain_args(pretrained_model_name_or_path="org/tiny", clip_model_name_or_path="none", revision=None)
    pre = pretrain_e4t.setup(args, CPU)
    run = str(tmp_path / "run" / "100")
    save_config(vars(args), run)                       # what the reference writes too: the base model by hub id
    save_e4t_unet(pre["unet"], run)
    save_e4t_encoder(pre["enc"], run)
    st = tuning_e4t.setup(tuning_args(pretrained_model_name_or_path=run), CPU)
    check_base(st, src)
    assert_same(st["enc"].state_dict(), pre["enc"].state_dict(), "tuning encoder")
    iargs = argparse.Namespace(random_init=False, pretrained_model_name_or_path=run, unet_variant="tiny-test", seed=0, scheduler_type="ddim",
                               enable_xformers_memory_efficient_attention=False)
    ist = inference.setup(iargs, CPU)
    check_base(dict(ist, vae=pre["vae"]), src)
    for k, v in src["dec"].state_dict().items():
        assert torch.equal(ist["vae"].state_dict()[k], v), k
    assert_same(ist["enc"].state_dict(), pre["enc"].state_dict(), "inference encoder")
    assert ist["base_dir"] == snap and ist["scheduler"].config["steps_offset"] == 1                # the snapshot's scheduler config
    assert seen == [os.path.join(snap, "tokenizer")] * 3
    # a name that resolves to nothing still ends inference, now with the paths searched
    json.dump(dict(json.load(open(os.path.join(run, "config.json"))), pretrained_model_name_or_path="org/absent"), open(os.path.join(run, "config.json"), "w"))
    with pytest.raises(SystemExit, match="models--org--absent"):
        inference.setup(iargs, CPU)
