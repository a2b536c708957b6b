"""CPU: inference.py --init_image builds and loads the VAE's encoder half next to the decoder, strictly, for the three checkpoint
layouts (diffusers pipeline directory, flat state dicts, --random_init); without the flag the pipeline gets no encoder."""
import argparse
import os

import pytest
import torch

import checkpoint_fixtures as fx
from test_checkpoint_loading import hub  # noqa: F401
from test_cli_setup import _write_base, pretrain_args
from test_unet_host_logic import emu_fp32  # noqa: F401

CPU = torch.device("cpu")


def iargs(run, **kw):
    d = dict(random_init=False, pretrained_model_name_or_path=run, unet_variant="tiny-test", seed=0, scheduler_type="ddim",
             enable_xformers_memory_efficient_attention=False, init_image=None, strength=0.8, mask_image=None)
    d.update(kw)
    return argparse.Namespace(**d)


def write_run(tmp_path, base):
    """a run directory naming `base`: config.json + weight_offsets.pt + encoder.pt"""
    import pretrain_e4t
    from e4t.utils import save_config, save_e4t_encoder, save_e4t_unet
    args = pretrain_args(pretrained_model_name_or_path=base, clip_model_name_or_path="none", revision=None)
    pre = pretrain_e4t.setup(args, CPU)
    run = str(tmp_path / "run" / "100")
    save_config(vars(args), run)
    save_e4t_unet(pre["unet"], run)
    save_e4t_encoder(pre["enc"], run)
    return run


def same(mod, want):
    got = mod.state_dict()
    assert set(got) == set(want.state_dict())
    for k, v in want.state_dict().items():
        assert torch.equal(got[k], v), k


def test_pipeline_layout_loads_the_encoder_half(emu_fp32, hub, tmp_path, monkeypatch):  # noqa: F811
    import inference
    src = fx.source_models()
    fx.write_snapshot(hub, src, tokenizer=True)
    fx.patch_tokenizer(monkeypatch)
    run = write_run(tmp_path, "org/tiny")
    st = inference.setup(iargs(run, init_image="photo.png"), CPU)
    same(st["vae_encoder"], src["vae"])
    same(st["vae"], src["dec"])
    assert st["pipe"].vae_encoder is st["vae_encoder"] and not any(p.requires_grad for p in st["vae_encoder"].parameters())
    plain = inference.setup(iargs(run), CPU)
    assert plain["vae_encoder"] is None and plain["pipe"].vae_encoder is None


def test_flat_layout_loads_the_encoder_half_strictly(emu_fp32, tmp_path, monkeypatch):  # noqa: F811
    import inference
    from e4t import vae as vae_mod
    base, _, _, vae0 = _write_base(tmp_path)
    fx.patch_tokenizer(monkeypatch)
    tiny = vae_mod.VAEDecoder                 # this layout has no config: inference.py builds the full-size decoder; the fixture's is tiny
    monkeypatch.setattr(vae_mod, "VAEDecoder", lambda: tiny(block_out_channels=(64, 64)))
    run = write_run(tmp_path, base)
    st = inference.setup(iargs(run, init_image="photo.png"), CPU)
    same(st["vae_encoder"], vae0)
    assert st["pipe"].vae_encoder is st["vae_encoder"]
    assert inference.setup(iargs(run), CPU)["pipe"].vae_encoder is None
    # a vae.pt whose encoder half misses a key ends the edit setup, and only the edit setup
    sd = torch.load(os.path.join(base, "vae.pt"), map_location="cpu")
    sd["quant_convv.weight"] = sd.pop("quant_conv.weight")
    torch.save(sd, os.path.join(base, "vae.pt"))
    with pytest.raises(RuntimeError, match="quant_conv"):
        inference.setup(iargs(run, init_image="photo.png"), CPU)
    assert inference.setup(iargs(run), CPU)["pipe"].vae_encoder is None


def test_random_init_builds_an_encoder_only_for_editing(emu_fp32):  # noqa: F811
    import inference
    st = inference.setup(iargs(None, random_init=True, init_image="photo.png"), CPU)
    from e4t.vae import VAEEncoder
    assert isinstance(st["pipe"].vae_encoder, VAEEncoder) and not any(p.requires_grad for p in st["pipe"].vae_encoder.parameters())
    assert inference.setup(iargs(None, random_init=True), CPU)["pipe"].vae_encoder is None
