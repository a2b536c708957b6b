"""Checkpoint resolution and reading for the scripts' set-up code: published Stable Diffusion and OpenCLIP weights, read from
local files only.

  * `resolve_model_dir(name, revision)`: an existing path as it is, else a hub-style id `org/name` looked up in the local
    Hugging Face cache by reading its files (`models--org--name/refs/<revision>` -> `snapshots/<hash>/`).  No hub client is
    imported and nothing is downloaded: a name that is not on disk raises `CheckpointNotFoundError` listing every path tried.
  * `read_state_dict(component_dir)`: one component's weights (`*.safetensors` preferred over `*.bin`, sharded
    `*.index.json`, the `fp16` variant file names), every floating tensor cast to fp32 (the native master-weight dtype).
  * The diffusers pipeline layout (`model_index.json`; `unet/`, `vae/`, `text_encoder/`, `tokenizer/`, `scheduler/`):
    `pipeline_configs` maps the components' `config.json` to the native constructor kwargs (the SD-1.x / 2.x subset; any
    other non-default field is an error that names it), `normalize_vae_keys` maps the VAE attention names of newer diffusers
    releases to the 0.14 names the native VAE uses.
  * OpenCLIP (`--clip_model_name_or_path arch::version`): `read_openclip_visual` returns the vision tower as a
    `clip_vision.*` state dict checked against the shape of `arch` (the native ViT follows open_clip's names).
"""
from __future__ import annotations

import json
import os
import re
import struct
from typing import Dict, List, Optional, Tuple

import torch


class CheckpointNotFoundError(FileNotFoundError):
    """A checkpoint name that resolves to nothing on this machine; `tried` lists every path that was looked at."""

    def __init__(self, name: str, tried: List[str], what: str = "checkpoint"):
        self.name, self.tried = name, list(tried)
        super().__init__(f"{what} {name!r} not found locally (no hub access in this build); tried: " + ", ".join(self.tried))


# ------------------------------------------------------------------------------------------------
# name -> local directory
# ------------------------------------------------------------------------------------------------
def hub_cache_dir() -> str:
    """$HF_HUB_CACHE, else $HF_HOME/hub, else ~/.cache/huggingface/hub (the hub client's own order)"""
    if os.environ.get("HF_HUB_CACHE"):
        return os.environ["HF_HUB_CACHE"]
    if os.environ.get("HF_HOME"):
        return os.path.join(os.environ["HF_HOME"], "hub")
    return os.path.join(os.path.expanduser("~"), ".cache", "huggingface", "hub")


_REPO_ID = re.compile(r"[A-Za-z0-9][\w.-]*/[\w.-]+")
_COMMIT = re.compile(r"[0-9a-f]{40}")


def cached_snapshot(repo_id: str, revision: Optional[str], tried: List[str]) -> Optional[str]:
    """snapshots/<hash>/ of `repo_id` in the local cache, or None; appends the paths it looked at to `tried`"""
    repo = os.path.join(hub_cache_dir(), "models--" + repo_id.replace("/", "--"))
    rev = revision or "main"
    if _COMMIT.fullmatch(rev):
        commit = rev
    else:
        ref = os.path.join(repo, "refs", rev)
        tried.append(ref)
        if not os.path.isfile(ref):
            return None
        with open(ref) as fh:
            commit = fh.read().strip()
    snap = os.path.join(repo, "snapshots", commit)
    tried.append(snap)
    return snap if os.path.isdir(snap) else None


def resolve_model_dir(name: str, revision: Optional[str] = None) -> str:
    """An existing path is returned as it is; `org/name` is looked up in the local Hugging Face cache."""
    if os.path.exists(name):
        return name
    tried = [name]
    if _REPO_ID.fullmatch(name):
        snap = cached_snapshot(name, revision, tried)
        if snap is not None:
            return snap
    raise CheckpointNotFoundError(name, tried, "base model")


def is_pipeline_layout(d: Optional[str]) -> bool:
    """a diffusers pipeline directory (model_index.json or unet/config.json), as opposed to the flat unet.pt / vae.pt layout"""
    return bool(d) and (os.path.isfile(os.path.join(d, "model_index.json")) or os.path.isfile(os.path.join(d, "unet", "config.json")))


# ------------------------------------------------------------------------------------------------
# weight files -> fp32 state dict
# ------------------------------------------------------------------------------------------------
_ST_DTYPES = {"F64": torch.float64, "F32": torch.float32, "F16": torch.float16, "BF16": torch.bfloat16, "I64": torch.int64,
              "I32": torch.int32, "I16": torch.int16, "I8": torch.int8, "U8": torch.uint8, "BOOL": torch.bool}


def parse_safetensors(path: str) -> Dict[str, torch.Tensor]:
    """The safetensors format read directly: u64 little-endian header size, a JSON header {name: {dtype, shape,
    data_offsets}}, then the raw little-endian data."""
    with open(path, "rb") as fh:
        (n,) = struct.unpack("<Q", fh.read(8))
        header = json.loads(fh.read(n))
        data = bytearray(fh.read())
    out = {}
    for k, m in header.items():
        if k == "__metadata__":
            continue
        if m["dtype"] not in _ST_DTYPES:
            raise ValueError(f"{path}: tensor {k!r} has the unsupported dtype {m['dtype']}")
        b, e = m["data_offsets"]
        dt = _ST_DTYPES[m["dtype"]]
        t = torch.frombuffer(data, dtype=dt, offset=b, count=(e - b) // dt.itemsize) if e > b else torch.empty(0, dtype=dt)
        out[k] = t.reshape(m["shape"]).clone()
    return out


def read_weight_file(path: str) -> Dict[str, torch.Tensor]:
    if path.endswith(".safetensors"):
        try:
            from safetensors.torch import load_file
        except ImportError:
            return parse_safetensors(path)
        return load_file(path, device="cpu")
    return torch.load(path, map_location="cpu", weights_only=True)


_STEMS = ("diffusion_pytorch_model", "model", "pytorch_model")


def weight_files(d: str) -> List[str]:
    """The files holding one component's weights, in the order the libraries that wrote them prefer: safetensors before
    bin, the full-precision files before the `fp16` variant, a sharded index (`weight_map`) before a single file."""
    for ext in (".safetensors", ".bin"):
        for variant in ("", ".fp16"):
            for stem in _STEMS:
                index = os.path.join(d, f"{stem}{ext}.index{variant}.json")
                if os.path.isfile(index):
                    with open(index) as fh:
                        shards = sorted(set(json.load(fh)["weight_map"].values()))
                    return [os.path.join(d, s) for s in shards]
                single = os.path.join(d, f"{stem}{variant}{ext}")
                if os.path.isfile(single):
                    return [single]
    raise CheckpointNotFoundError(d, [os.path.join(d, f"{s}{v}{e}") for e in (".safetensors", ".bin") for v in ("", ".fp16") for s in _STEMS],
                                  "component weights in")


def read_state_dict(d: str) -> Dict[str, torch.Tensor]:
    """One component directory's state dict, floating tensors cast to fp32 (integer buffers keep their dtype)"""
    sd = {}
    for f in weight_files(d):
        part = read_weight_file(f)
        dup = set(part) & set(sd)
        if dup:
            raise ValueError(f"{f}: keys also present in another shard: {sorted(dup)[:5]}")
        sd.update(part)
    return {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}


_VAE_ATTN = {"to_q": "query", "to_k": "key", "to_v": "value", "to_out.0": "proj_attn"}
_VAE_ATTN_RE = re.compile(r"^((?:encoder|decoder)\.mid_block\.attentions\.\d+\.)(to_q|to_k|to_v|to_out\.0)\.(weight|bias)$")


def normalize_vae_keys(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """diffusers >= 0.15 saves the VAE mid-block attention as to_q / to_k / to_v / to_out.0; the native VAE (and the 0.14
    checkpoints) name them query / key / value / proj_attn.  Every other key passes unchanged."""
    out = {}
    for k, v in sd.items():
        m = _VAE_ATTN_RE.match(k)
        k2 = f"{m.group(1)}{_VAE_ATTN[m.group(2)]}.{m.group(3)}" if m else k
        if k2 in out:
            raise ValueError(f"VAE state dict holds both the old and the new name of {k2!r}")
        out[k2] = v
    return out


# ------------------------------------------------------------------------------------------------
# diffusers / transformers config.json -> native constructor kwargs
# ------------------------------------------------------------------------------------------------
# UNet2DConditionModel fields the native UNet implements only at their default value (diffusers' defaults)
_UNET_FIXED = dict(center_input_sample=False, flip_sin_to_cos=True, freq_shift=0, mid_block_type="UNetMidBlock2DCrossAttn",
                   only_cross_attention=False, downsample_padding=1, mid_block_scale_factor=1, act_fn="silu", dual_cross_attention=False,
                   class_embed_type=None, num_class_embeds=None, resnet_time_scale_shift="default", time_embedding_type="positional",
                   conv_in_kernel=3, conv_out_kernel=3, num_attention_heads=None, transformer_layers_per_block=1,
                   reverse_transformer_layers_per_block=None, encoder_hid_dim=None, encoder_hid_dim_type=None, addition_embed_type=None,
                   addition_time_embed_dim=None, addition_embed_type_num_heads=64, time_embedding_dim=None, time_embedding_act_fn=None,
                   timestep_post_act=None, time_cond_proj_dim=None, projection_class_embeddings_input_dim=None, class_embeddings_concat=False,
                   mid_block_only_cross_attention=None, cross_attention_norm=None, resnet_skip_time_act=False, resnet_out_scale_factor=1.0,
                   dropout=0.0, attention_type="default")
_UNET_MAPPED = ("sample_size", "in_channels", "out_channels", "block_out_channels", "layers_per_block", "norm_num_groups", "norm_eps",
                "cross_attention_dim", "attention_head_dim", "use_linear_projection", "upcast_attention", "down_block_types", "up_block_types")
_DOWN_TYPES = ("CrossAttnDownBlock2D", "DownBlock2D")
_UP_TYPES = ("CrossAttnUpBlock2D", "UpBlock2D")

_VAE_FIXED = dict(in_channels=3, out_channels=3, layers_per_block=2, act_fn="silu", norm_num_groups=32, force_upcast=True, shift_factor=None,
                  latents_mean=None, latents_std=None, use_quant_conv=True, use_post_quant_conv=True, mid_block_add_attention=True)
_VAE_MAPPED = ("block_out_channels", "latent_channels", "scaling_factor", "down_block_types", "up_block_types")
_VAE_IGNORED = ("sample_size",)            # the resolution the VAE was trained at, not a shape of its weights

_TEXT_FIXED = dict(layer_norm_eps=1e-5, dropout=0.0, attention_dropout=0.0, model_type="clip_text_model", architectures=["CLIPTextModel"])
_TEXT_MAPPED = ("vocab_size", "hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size", "max_position_embeddings",
                "hidden_act")
# transformers metadata that does not enter CLIPTextModel's forward (token ids, init ranges, the projection head it has not got)
_TEXT_IGNORED = ("bos_token_id", "eos_token_id", "pad_token_id", "initializer_range", "initializer_factor", "projection_dim", "torch_dtype",
                 "dtype", "transformers_version")


def _same(a, b) -> bool:
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def _check_fields(cfg: dict, fixed: dict, mapped, ignored, what: str):
    """every field is mapped, metadata, or at the one value the native model implements; anything else names itself"""
    for k, v in cfg.items():
        if k.startswith("_") or k in mapped or k in ignored:
            continue
        if k not in fixed:
            raise ValueError(f"{what}: unsupported field {k!r} = {v!r} (the native model does not implement it)")
        if not _same(v, fixed[k]):
            raise ValueError(f"{what}: unsupported value {k} = {v!r} (only {fixed[k]!r} is implemented)")


def _read_json(path: str) -> dict:
    with open(path) as fh:
        return json.load(fh)


def unet_kwargs(cfg: dict, what: str = "unet/config.json") -> dict:
    """diffusers UNet2DConditionModel config -> native UNet2DConditionModel kwargs (the fields of builders.UNET_CONFIGS)"""
    if cfg.get("_class_name", "UNet2DConditionModel") != "UNet2DConditionModel":
        raise ValueError(f"{what}: unsupported _class_name {cfg['_class_name']!r}")
    _check_fields(cfg, _UNET_FIXED, _UNET_MAPPED, (), what)
    boc = tuple(int(c) for c in cfg.get("block_out_channels", (320, 640, 1280, 1280)))
    down = tuple(cfg.get("down_block_types", ("CrossAttnDownBlock2D",) * 3 + ("DownBlock2D",)))
    up = tuple(cfg.get("up_block_types", ("UpBlock2D",) + ("CrossAttnUpBlock2D",) * 3))
    for kind, types, ok in (("down", down, _DOWN_TYPES), ("up", up, _UP_TYPES)):
        for t in types:
            if t not in ok:
                raise ValueError(f"{what}: unsupported {kind} block type {t!r} (supported: {', '.join(ok)})")
        if len(types) != len(boc):
            raise ValueError(f"{what}: {len(types)} {kind} block types for {len(boc)} block_out_channels")
    heads = cfg.get("attention_head_dim", 8)
    heads = int(heads) if isinstance(heads, int) else tuple(int(h) for h in heads)
    if isinstance(heads, tuple) and len(heads) != len(boc):
        raise ValueError(f"{what}: attention_head_dim {list(heads)} does not have one entry per block ({len(boc)})")
    return dict(sample_size=cfg.get("sample_size"), in_channels=int(cfg.get("in_channels", 4)), out_channels=int(cfg.get("out_channels", 4)),
                block_out_channels=boc, layers_per_block=int(cfg.get("layers_per_block", 2)), norm_num_groups=int(cfg.get("norm_num_groups", 32)),
                norm_eps=float(cfg.get("norm_eps", 1e-5)), cross_attention_dim=int(cfg.get("cross_attention_dim", 1280)), attention_head_dim=heads,
                use_linear_projection=bool(cfg.get("use_linear_projection", False)), upcast_attention=bool(cfg.get("upcast_attention", False)),
                down_block_types=down, up_block_types=up)


def vae_kwargs(cfg: dict, what: str = "vae/config.json") -> dict:
    """diffusers AutoencoderKL config -> kwargs of the native VAEEncoder / VAEDecoder"""
    if cfg.get("_class_name", "AutoencoderKL") != "AutoencoderKL":
        raise ValueError(f"{what}: unsupported _class_name {cfg['_class_name']!r}")
    _check_fields(cfg, _VAE_FIXED, _VAE_MAPPED, _VAE_IGNORED, what)
    boc = tuple(int(c) for c in cfg.get("block_out_channels", (64,)))
    for key, typ in (("down_block_types", "DownEncoderBlock2D"), ("up_block_types", "UpDecoderBlock2D")):
        types = tuple(cfg.get(key, (typ,) * len(boc)))
        if any(t != typ for t in types) or len(types) != len(boc):
            raise ValueError(f"{what}: unsupported {key} {list(types)} (supported: {len(boc)} x {typ})")
    return dict(block_out_channels=boc, latent_channels=int(cfg.get("latent_channels", 4)), scaling_factor=float(cfg.get("scaling_factor", 0.18215)))


def text_kwargs(cfg: dict, what: str = "text_encoder/config.json") -> dict:
    """transformers CLIPTextConfig -> native CLIPTextModel kwargs (the fields of builders.TEXT_CONFIGS)"""
    _check_fields(cfg, _TEXT_FIXED, _TEXT_MAPPED, _TEXT_IGNORED, what)
    act = cfg.get("hidden_act", "quick_gelu")
    if act not in ("quick_gelu", "gelu"):
        raise ValueError(f"{what}: unsupported hidden_act {act!r} (supported: quick_gelu, gelu)")
    return dict(vocab_size=int(cfg.get("vocab_size", 49408)), hidden_size=int(cfg.get("hidden_size", 512)),
                num_layers=int(cfg.get("num_hidden_layers", 12)), num_heads=int(cfg.get("num_attention_heads", 8)),
                intermediate_size=int(cfg.get("intermediate_size", 2048)), max_len=int(cfg.get("max_position_embeddings", 77)), act=act)


def pipeline_configs(d: str) -> dict:
    """{unet, text, vae}: native constructor kwargs read from a diffusers pipeline directory's component configs"""
    out = {}
    for name, sub, fn in (("unet", "unet", unet_kwargs), ("text", "text_encoder", text_kwargs), ("vae", "vae", vae_kwargs)):
        f = os.path.join(d, sub, "config.json")
        if not os.path.isfile(f):
            raise CheckpointNotFoundError(f, [f], "component config")
        out[name] = fn(_read_json(f), what=f)
    return out


def describe(cfgs: dict) -> str:
    u, t, v = cfgs["unet"], cfgs["text"], cfgs["vae"]
    return (f"UNet block_out_channels={list(u['block_out_channels'])} cross_attention_dim={u['cross_attention_dim']} "
            f"attention_head_dim={u['attention_head_dim']} use_linear_projection={u['use_linear_projection']} "
            f"upcast_attention={u['upcast_attention']}; text encoder hidden={t['hidden_size']} layers={t['num_layers']} heads={t['num_heads']} "
            f"act={t['act']}; VAE block_out_channels={list(v['block_out_channels'])} scaling_factor={v['scaling_factor']}")


# ------------------------------------------------------------------------------------------------
# OpenCLIP vision tower
# ------------------------------------------------------------------------------------------------
CLIP_ARCHS = ("ViT-H-14", "ViT-tiny-test")         # tower shapes: encoder.VIT_ARCHS
# (arch, pretrained tag) -> Hugging Face cache repository that holds open_clip's weights (open_clip's pretrained table)
OPENCLIP_PRETRAINED = {("ViT-H-14", "laion2b_s32b_b79k"): "laion/CLIP-ViT-H-14-laion2B-s32B-b79K"}
OPENCLIP_FILES = ("open_clip_model.safetensors", "open_clip_pytorch_model.bin")


def parse_clip_source(src: str) -> Tuple[str, str]:
    """'arch::version' -> (arch, version); arch must be in the tower table"""
    arch, sep, version = src.partition("::")
    if not sep or not version:
        raise ValueError(f"--clip_model_name_or_path {src!r}: expected 'arch::version' (e.g. ViT-H-14::laion2b_s32b_b79k) or 'none'")
    if arch not in CLIP_ARCHS:
        raise ValueError(f"--clip_model_name_or_path {src!r}: unknown tower {arch!r} (known: {', '.join(CLIP_ARCHS)})")
    return arch, version


def resolve_clip_file(src: str) -> Tuple[str, str]:
    """'arch::version' -> (arch, local weight file).  version: a .bin / .pt / .safetensors path, or a pretrained tag looked up
    in OPENCLIP_PRETRAINED and then in the local cache.  CheckpointNotFoundError lists every path tried."""
    arch, version = parse_clip_source(src)
    if version.endswith((".bin", ".pt", ".pth", ".safetensors")) or os.sep in version:
        if os.path.isfile(version):
            return arch, version
        raise CheckpointNotFoundError(src, [version], "CLIP checkpoint")
    repo = OPENCLIP_PRETRAINED.get((arch, version))
    if repo is None:
        tags = sorted(t for a, t in OPENCLIP_PRETRAINED if a == arch)
        raise ValueError(f"--clip_model_name_or_path {src!r}: unknown pretrained tag {version!r} for {arch} "
                         f"(known: {', '.join(tags) or 'none'}; or give a weight file)")
    tried: List[str] = []
    snap = cached_snapshot(repo, None, tried)
    if snap is not None:
        for fn in OPENCLIP_FILES:
            f = os.path.join(snap, fn)
            tried.append(f)
            if os.path.isfile(f):
                return arch, f
    raise CheckpointNotFoundError(src, tried, "CLIP checkpoint")


def read_openclip_visual(arch: str, path: str) -> Dict[str, torch.Tensor]:
    """open_clip state dict -> the E4T encoder's `clip_vision.*` keys (fp32).  The text tower and `visual.proj` are dropped (the
    E4T encoder runs the tower with proj = None, reference encoder.py:91-97); every kept key and shape is checked against `arch`."""
    from .encoder import VIT_ARCHS, VisionTransformer
    sd = read_weight_file(path)
    if isinstance(sd.get("state_dict"), dict):
        sd = sd["state_dict"]
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
    vis = {k: v for k, v in sd.items() if k.startswith("visual.") and k != "visual.proj"}
    if not vis:
        raise ValueError(f"{path}: no 'visual.*' keys: not an open_clip checkpoint")
    with torch.device("meta"):
        want = {"visual." + k: v.shape for k, v in VisionTransformer(**VIT_ARCHS[arch]).state_dict().items()}
    missing, unexpected = sorted(set(want) - set(vis)), sorted(set(vis) - set(want))
    if missing or unexpected:
        raise ValueError(f"{path}: does not match the {arch} tower: missing keys {missing[:5]} unexpected keys {unexpected[:5]}")
    for k, v in vis.items():
        if tuple(v.shape) != tuple(want[k]):
            raise ValueError(f"{path}: {k} has shape {list(v.shape)}, the {arch} tower needs {list(want[k])}")
    return {"clip_vision." + k[len("visual."):]: v.float() for k, v in vis.items()}
