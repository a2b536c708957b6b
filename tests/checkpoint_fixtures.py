"""Published-checkpoint fixtures written at test time (tests/test_checkpoint_loading*.py): a Hugging Face cache (refs/<rev>,
snapshots/<hash>/ with symlinks into blobs/) holding a diffusers pipeline of the tiny-test models, saved the way the libraries
save real ones, and open_clip files of the tiny ViT (vision tower + text tower + visual.proj)."""
import hashlib
import io
import json
import os

import torch

COMMIT = "0123456789abcdef0123456789abcdef01234567"
TINY_UNET = dict(_class_name="UNet2DConditionModel", _diffusers_version="0.27.2", act_fn="silu", attention_head_dim=2,
                 block_out_channels=[64, 128, 128, 128], center_input_sample=False, cross_attention_dim=64,
                 down_block_types=["CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"], downsample_padding=1,
                 flip_sin_to_cos=True, freq_shift=0, in_channels=4, layers_per_block=2, mid_block_scale_factor=1, norm_eps=1e-05,
                 norm_num_groups=32, out_channels=4, sample_size=16,
                 up_block_types=["UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D"])
TINY_TEXT = dict(_name_or_path="openai/clip-vit-large-patch14", architectures=["CLIPTextModel"], attention_dropout=0.0, bos_token_id=0,
                 dropout=0.0, eos_token_id=2, hidden_act="quick_gelu", hidden_size=64, initializer_factor=1.0, initializer_range=0.02,
                 intermediate_size=128, layer_norm_eps=1e-05, max_position_embeddings=9, model_type="clip_text_model", num_attention_heads=2,
                 num_hidden_layers=2, pad_token_id=1, projection_dim=64, torch_dtype="float32", transformers_version="4.22.0.dev0", vocab_size=100)
TINY_VAE = dict(_class_name="AutoencoderKL", _diffusers_version="0.2.2", act_fn="silu", block_out_channels=[64, 64],
                down_block_types=["DownEncoderBlock2D", "DownEncoderBlock2D"], in_channels=3, latent_channels=4, layers_per_block=2,
                out_channels=3, sample_size=64, up_block_types=["UpDecoderBlock2D", "UpDecoderBlock2D"])
SCHEDULER = dict(_class_name="PNDMScheduler", _diffusers_version="0.7.0.dev0", beta_end=0.012, beta_schedule="scaled_linear",
                 beta_start=0.00085, num_train_timesteps=1000, set_alpha_to_one=False, skip_prk_steps=True, steps_offset=1,
                 trained_betas=None, clip_sample=False)
NEW_VAE_NAMES = {"query": "to_q", "key": "to_k", "value": "to_v", "proj_attn": "to_out.0"}


def source_models(seed=11, unet_cfg=None):
    """the tensors the checkpoints hold: tiny-test UNet (stock keys), text encoder, VAE encoder + decoder, E4T encoder (its tower)"""
    from e4t import builders, checkpoints
    from e4t.vae import VAEDecoder
    cfg = checkpoints.unet_kwargs(unet_cfg or TINY_UNET)
    unet, enc, text, vae = builders.build_from_configs("cpu", cfg, dict(builders.TEXT_CONFIGS["tiny-test"]), dict(block_out_channels=(64, 64)),
                                                       "ViT-tiny-test", seed)
    torch.manual_seed(seed + 1)
    dec = VAEDecoder(block_out_channels=(64, 64))
    return dict(unet=unet, enc=enc, text=text, vae=vae, dec=dec, unet_cfg=unet_cfg or TINY_UNET)


def unet_sd(src):
    return {k: v.detach().clone().contiguous() for k, v in src["unet"].state_dict().items() if "wo" not in k}


def text_sd(src):
    sd = {k: v.detach().clone().contiguous() for k, v in src["text"].state_dict().items()}
    sd["text_model.embeddings.position_ids"] = torch.arange(9)[None]          # what transformers < 4.31 saved
    return sd


def vae_sd(src, new_names=False):
    sd = {k: v.detach().clone().contiguous() for k, v in {**src["vae"].state_dict(), **src["dec"].state_dict()}.items()}
    if new_names:
        out = {}
        for k, v in sd.items():
            parts = k.split(".")
            if ".mid_block.attentions." in k and parts[-2] in NEW_VAE_NAMES:
                k = ".".join(parts[:-2] + [NEW_VAE_NAMES[parts[-2]], parts[-1]])
            out[k] = v
        sd = out
    return sd


def _bytes(sd, fmt):
    if fmt == "safetensors":
        from safetensors.torch import save
        return save(sd)
    buf = io.BytesIO()
    torch.save(sd, buf)
    return buf.getvalue()


class CacheRepo:
    """models--org--name in a fake cache: files are content-addressed blobs, the snapshot holds relative symlinks to them"""

    def __init__(self, cache, repo_id, commit=COMMIT, ref="main"):
        self.root = os.path.join(str(cache), "models--" + repo_id.replace("/", "--"))
        self.snap = os.path.join(self.root, "snapshots", commit)
        os.makedirs(os.path.join(self.root, "refs"), exist_ok=True)
        os.makedirs(os.path.join(self.root, "blobs"), exist_ok=True)
        with open(os.path.join(self.root, "refs", ref), "w") as fh:
            fh.write(commit)

    def put(self, rel, data):
        if isinstance(data, str):
            data = data.encode()
        blob = os.path.join(self.root, "blobs", hashlib.sha256(data).hexdigest())
        with open(blob, "wb") as fh:
            fh.write(data)
        dst = os.path.join(self.snap, rel)
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        os.symlink(os.path.relpath(blob, os.path.dirname(dst)), dst)
        return dst


def put_weights(repo, sub, stem, sd, fmt):
    """one component's weights the way diffusers / transformers save them: fmt safetensors | bin | sharded | fp16"""
    if fmt in ("safetensors", "bin"):
        repo.put(f"{sub}/{stem}.{fmt}", _bytes(sd, fmt))
    elif fmt == "fp16":
        repo.put(f"{sub}/{stem}.fp16.safetensors", _bytes({k: (v.half() if v.is_floating_point() else v) for k, v in sd.items()}, "safetensors"))
    elif fmt == "sharded":
        keys = sorted(sd)
        halves = (keys[: len(keys) // 2], keys[len(keys) // 2:])
        wmap = {}
        for i, ks in enumerate(halves):
            name = f"{stem}-{i + 1:05d}-of-00002.safetensors"
            repo.put(f"{sub}/{name}", _bytes({k: sd[k] for k in ks}, "safetensors"))
            wmap.update({k: name for k in ks})
        repo.put(f"{sub}/{stem}.safetensors.index.json", json.dumps(dict(metadata=dict(total_size=0), weight_map=wmap)))
    else:
        raise ValueError(fmt)


def write_snapshot(cache, src, repo_id="org/tiny", fmt="safetensors", vae_new_names=False, tokenizer=False, model_index=True):
    """a diffusers pipeline snapshot of `src` in the fake cache; returns the snapshot directory"""
    repo = CacheRepo(cache, repo_id)
    if model_index:
        repo.put("model_index.json", json.dumps(dict(_class_name="StableDiffusionPipeline", _diffusers_version="0.27.2",
                                                     unet=["diffusers", "UNet2DConditionModel"], vae=["diffusers", "AutoencoderKL"],
                                                     text_encoder=["transformers", "CLIPTextModel"], tokenizer=["transformers", "CLIPTokenizer"],
                                                     scheduler=["diffusers", "PNDMScheduler"])))
    repo.put("unet/config.json", json.dumps(src["unet_cfg"]))
    repo.put("text_encoder/config.json", json.dumps(TINY_TEXT))
    repo.put("vae/config.json", json.dumps(TINY_VAE))
    repo.put("scheduler/scheduler_config.json", json.dumps(SCHEDULER))
    bin_ = fmt == "bin"
    put_weights(repo, "unet", "diffusion_pytorch_model", unet_sd(src), fmt)
    put_weights(repo, "vae", "diffusion_pytorch_model", vae_sd(src, vae_new_names), fmt)
    put_weights(repo, "text_encoder", "pytorch_model" if bin_ else "model", text_sd(src), fmt)
    if tokenizer:
        repo.put("tokenizer/tokenizer_config.json", json.dumps(dict(model_max_length=9)))
    return repo.snap


def openclip_sd(enc, drop=(), width=None):
    """a full open_clip state dict around enc.clip_vision: visual.* (+ visual.proj) and a text tower"""
    from e4t.encoder import VIT_ARCHS, VisionTransformer
    tower = enc.clip_vision
    if width is not None:
        torch.manual_seed(3)
        tower = VisionTransformer(**dict(VIT_ARCHS["ViT-tiny-test"], width=width))
    g = torch.Generator().manual_seed(2)
    sd = {"visual." + k: v.detach().clone().contiguous() for k, v in tower.state_dict().items()}
    w = tower.width
    sd.update({"visual.proj": torch.randn(w, 32, generator=g), "positional_embedding": torch.randn(9, 32, generator=g),
               "text_projection": torch.randn(32, 32, generator=g), "logit_scale": torch.tensor(4.6052),
               "token_embedding.weight": torch.randn(100, 32, generator=g), "ln_final.weight": torch.ones(32), "ln_final.bias": torch.zeros(32),
               "transformer.resblocks.0.attn.in_proj_weight": torch.randn(96, 32, generator=g)})
    for k in drop:
        del sd[k]
    return sd


def write_openclip(path, enc, fmt="bin", **kw):
    with open(path, "wb") as fh:
        fh.write(_bytes(openclip_sd(enc, **kw), "safetensors" if fmt == "safetensors" else "bin"))
    return str(path)


def patch_tokenizer(monkeypatch):
    """CLIPTokenizer.from_pretrained -> the offline whitespace tokenizer at the tiny sizes; records the directories asked for"""
    import transformers
    from e4t.utils import WhitespaceTokenizer
    seen = []

    def fake(path, *a, **k):
        seen.append(str(path))
        return WhitespaceTokenizer(base_size=100, model_max_length=9)
    monkeypatch.setattr(transformers.CLIPTokenizer, "from_pretrained", staticmethod(fake))
    return seen
