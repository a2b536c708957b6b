"""Host-side set-up shared by pretrain_e4t.py / tuning_e4t.py / inference.py: the glue lines of the reference scripts that sit
between "parse the arguments" and "run the step" — tokenizer + placeholder token, class-token / empty-prompt ids, prompt
templates, base-model loading — restated once so the three scripts condition the models identically (the E4T encoder pass is
conditioned on tokenizer("") and the class token in training AND in sampling; getting one of them different in one script
silently trains a model the pipeline cannot use).  No tensor arithmetic lives here.

There is no network in this build: "pretrained_model_name_or_path" is a local directory, or a hub id (`org/name`,
`--revision`) whose snapshot is in the local Hugging Face cache (e4t/checkpoints.py reads the cache's files; nothing is
downloaded).  Two layouts:
  the diffusers pipeline layout of published checkpoints (model_index.json; the components' config.json decide the architecture)
    <dir>/unet/  vae/  text_encoder/              config.json + *.safetensors | *.bin (sharded or not, fp16 variant too)
    <dir>/tokenizer/                              CLIPTokenizer files
    <dir>/scheduler/scheduler_config.json         optional
  the flat layout (the --unet_variant architecture)
    <dir>/unet.pt  vae.pt  text_encoder.pt        plain state dicts with the diffusers / transformers key names
    <dir>/tokenizer/                              CLIPTokenizer files
    <dir>/scheduler/scheduler_config.json         optional
The E4T encoder's CLIP tower comes from --clip_model_name_or_path 'arch::version' (an open_clip weight file, or a pretrained
tag found in the local cache) unless an E4T run's encoder.pt is resumed; 'none' keeps it randomly initialised.
"""
from __future__ import annotations

import os
import random
import sys
from typing import List, Optional, Sequence

import torch

# the reference's prompt templates (pretrain_e4t.py:36-62 == tuning_e4t.py:28-54): data, kept verbatim so that a model trained
# here sees the prompt distribution a model trained with the reference sees
templates = [
    "a photo of {placeholder_token}",
    "the photo of {placeholder_token}",
    "a photo of a {placeholder_token}",
    "a photo of the {placeholder_token}",
    "a photo of one {placeholder_token}",
    "a close-up photo of the {placeholder_token}",
    "a bright photo of the {placeholder_token}",
    "a photo of a nice {placeholder_token}",
    "a good photo of {placeholder_token}",
    "a photo of a cool {placeholder_token}",
]
face_templates = templates + [
    "a portrait of {placeholder_token}",
    "the portrait of {placeholder_token}",
    "a portrait photo of {placeholder_token}",
    "portrait of {placeholder_token}",
    "portrait of the {placeholder_token}",
    "photo realistic portrait of {placeholder_token}",
]
art_templates = templates + [
    "art of {placeholder_token}",
    "art by {placeholder_token}",
]
NAMED_TEMPLATES = {"normal": templates, "face": face_templates, "art": art_templates}


def resolve_prompt_templates(prompt_template: str) -> List[str]:
    """pretrain_e4t.py:570-581 / tuning_e4t.py:254-265: a named list, or ONE custom template containing '{placeholder_token}'"""
    if prompt_template in NAMED_TEMPLATES:
        out = NAMED_TEMPLATES[prompt_template]
        print(f"Using the default {len(out)} templates!")
        return list(out)
    assert "{placeholder_token}" in prompt_template, "You must specify the location of placeholder token by '{placeholder_token}'"
    return [prompt_template]


def load_tokenizer(base_dir: Optional[str], allow_offline_standin: bool, vocab_size: int = 49408, max_len: int = 77):
    """CLIPTokenizer from <base_dir>/tokenizer (pretrain_e4t.py:233).  Without one — synthetic / random-init runs only — the
    offline whitespace tokenizer with CLIP's sizes stands in (its ids mean nothing to pretrained weights: loud message)."""
    tdir = os.path.join(base_dir or "", "tokenizer")
    if base_dir and os.path.isdir(tdir):
        from transformers import CLIPTokenizer
        return CLIPTokenizer.from_pretrained(tdir)
    if not allow_offline_standin:
        raise FileNotFoundError(f"no tokenizer under {tdir!r}: real-data training needs the checkpoint's CLIPTokenizer files "
                                f"(pass --synthetic_data / --random_init for a run on random weights)")
    from .utils import WhitespaceTokenizer
    print("[e4t] no tokenizer directory: using the offline whitespace stand-in (only meaningful with randomly initialised weights)")
    return WhitespaceTokenizer(base_size=vocab_size, model_max_length=max_len)


def add_placeholder_token(tokenizer, text_encoder, placeholder_token: str) -> int:
    """pretrain_e4t.py:253-259 / tuning_e4t.py:121-127: add the token, grow the embedding table by it, return its id"""
    num_added = tokenizer.add_tokens(placeholder_token)
    if num_added == 0:
        raise ValueError(f"The tokenizer already contains the token {placeholder_token}. Please pass a different `placeholder_token` "
                         f"that is not already in the tokenizer.")
    pid = tokenizer.convert_tokens_to_ids(placeholder_token)
    text_encoder.resize_token_embeddings(len(tokenizer))
    assert text_encoder.get_input_embeddings().weight.shape[0] == len(tokenizer) and pid < len(tokenizer)
    return pid


def conditioning_ids(tokenizer, domain_class_token: str):
    """-> (class_token_id, empty_prompt_ids [1, max_len]).  pretrain_e4t.py:561-569: the class token must be ONE token; the E4T
    encoder pass is conditioned on tokenizer("") padded to the model length (BOS + EOS padding for CLIP)."""
    ids = tokenizer(domain_class_token, add_special_tokens=False, return_tensors="pt").input_ids[0]
    assert ids.shape[0] == 1, f"--domain_class_token {domain_class_token!r} must be a single token, got ids {ids.tolist()}"
    empty = tokenizer("", padding="max_length", truncation=True, max_length=tokenizer.model_max_length, return_tensors="pt").input_ids
    return int(ids[0]), empty


def tokenize_prompts(tokenizer, prompt_templates: Sequence[str], placeholder_token: str, placeholder_token_id: int, bsz: int, rng=random):
    """pretrain_e4t.py:607-615: one random template per sample -> (input_ids [bsz, max_len], index of the placeholder in each row)"""
    batch = rng.choices(list(prompt_templates), k=bsz)
    prompt = [t.format(placeholder_token=placeholder_token) for t in batch]
    ids = tokenizer(prompt, padding="max_length", truncation=True, max_length=tokenizer.model_max_length, return_tensors="pt").input_ids
    idx = torch.tensor([row.index(placeholder_token_id) for row in ids.tolist()])
    return ids, idx


def checked_load(module: torch.nn.Module, path: str, may_miss=lambda k: False, what: str = ""):
    """load_state_dict that fails loudly: unexpected keys always raise, missing keys raise unless `may_miss(key)` (the reference's
    load_e4t_unet / load_e4t_encoder contract, e4t/utils.py:119-124,150-154).  A shape mismatch raises inside torch."""
    return checked_load_state_dict(module, torch.load(path, map_location="cpu"), may_miss, what or path)


def checked_load_state_dict(module: torch.nn.Module, sd: dict, may_miss=lambda k: False, what: str = ""):
    """checked_load of a state dict already read (e4t/checkpoints.py).  The parameters are written in place; every prepared
    compute copy of the modules (bf16 GEMM operands, fused q|k|v, the VAE's and the weight-offset banks' caches) is keyed on
    the parameters' versions and is re-made at the next forward."""
    # transformers < 4.31 saved the (persistent, integer) buffer `*.embeddings.position_ids` with every CLIP state dict; it is an
    # arange, not a weight, and the module trees here do not carry it: drop it, keep the strict check for every other key
    sd = {k: v for k, v in sd.items() if not k.endswith(".position_ids")}
    missing, unexpected = module.load_state_dict(sd, strict=False)
    missing = [k for k in missing if not may_miss(k)]
    if missing or unexpected:
        raise RuntimeError(f"{what}: missing keys {missing[:5]}{'...' if len(missing) > 5 else ''} "
                           f"unexpected keys {list(unexpected)[:5]}{'...' if len(unexpected) > 5 else ''}")
    return module


def resolve_base(base: Optional[str], revision: Optional[str] = None) -> Optional[str]:
    """--pretrained_model_name_or_path -> a local directory: an existing path as it is, a hub id from the local Hugging Face
    cache; None stays None.  Raises checkpoints.CheckpointNotFoundError (listing the paths tried) otherwise."""
    from .checkpoints import resolve_model_dir
    return resolve_model_dir(base, revision) if base else base


def load_pipeline_weights(base_dir: str, unet=None, text=None, vae=None, vae_decoder=None):
    """The components of a diffusers pipeline directory into built native modules, strictly (a stock UNet has no "wo" keys).
    The VAE file holds both halves of the AutoencoderKL: `vae` takes the encoder half, `vae_decoder` the decoder half."""
    from . import checkpoints as ck
    for sub, mod, may_miss in (("unet", unet, lambda k: "wo" in k), ("text_encoder", text, lambda k: False)):
        if mod is not None:
            d = os.path.join(base_dir, sub)
            checked_load_state_dict(mod, ck.read_state_dict(d), may_miss, what=d)
    if vae is not None or vae_decoder is not None:
        d = os.path.join(base_dir, "vae")
        sd = ck.normalize_vae_keys(ck.read_state_dict(d))
        for mod, prefixes in ((vae, ("encoder.", "quant_conv.")), (vae_decoder, ("decoder.", "post_quant_conv."))):
            if mod is not None:
                checked_load_state_dict(mod, {k: v for k, v in sd.items() if k.startswith(prefixes)}, what=d)


def pipeline_vae_decoder(dev, base_dir: str):
    """The AutoencoderKL decoder of a diffusers pipeline directory (its vae/config.json decides the shape), for sampling."""
    from . import checkpoints as ck
    from .vae import VAEDecoder
    with torch.device(dev):
        dec = VAEDecoder(**ck.pipeline_configs(base_dir)["vae"]).requires_grad_(False)
    load_pipeline_weights(base_dir, vae_decoder=dec)
    return dec


def load_clip_tower(enc, clip_source: str) -> str:
    """--clip_model_name_or_path 'arch::version' -> enc.clip_vision, strictly.  Returns the file read; raises
    checkpoints.CheckpointNotFoundError when the source names nothing on this machine."""
    from . import checkpoints as ck
    arch, path = ck.resolve_clip_file(clip_source)
    if arch != enc.config.arch:
        raise ValueError(f"--clip_model_name_or_path {clip_source!r} is a {arch} tower; the E4T encoder was built with {enc.config.arch}")
    sd = ck.read_openclip_visual(arch, path)
    enc.clip_vision.load_state_dict({k[len("clip_vision."):]: v for k, v in sd.items()}, strict=True)
    print(f"[e4t] CLIP tower {arch} loaded from {path}")
    return path


def build_models(dev, base_dir: Optional[str], variant: str, seed: int, freeze_clip_vision: bool = True, e4t_dir: Optional[str] = None,
                 need_vae_encoder: bool = True, clip_source: Optional[str] = None, revision: Optional[str] = None, use_ema: bool = False):
    """(unet, e4t_encoder, text_encoder, vae_encoder) on `dev` (pretrain_e4t.py:233-251, tuning_e4t.py:97-118).
    base_dir: Stable Diffusion checkpoint in either layout of the module docstring (a hub id is looked up in the local cache at
    `revision`) or None = random init from `seed`.  The pipeline layout's configs decide the architecture; otherwise `variant` does.
    clip_source: --clip_model_name_or_path for the E4T encoder's CLIP tower; None = not requested, 'none' = random init.  It is
    not read when e4t_dir holds an encoder.pt (that wins).  If it names nothing on this machine, a pipeline-layout base exits
    listing the paths searched, a flat-layout base warns and keeps the random tower, and a random base keeps it.
    e4t_dir: directory with weight_offsets.pt | unet.pt and encoder.pt of an earlier E4T run, loaded on top (both strict);
    use_ema: its weight_offsets_ema.pt and encoder_ema.pt instead (ema_file_names: SystemExit when they are not there)."""
    from . import builders
    from . import checkpoints as ck
    names = ema_file_names(e4t_dir, use_ema)
    if base_dir and not os.path.exists(base_dir):
        base_dir = ck.resolve_model_dir(base_dir, revision)
    pipeline = ck.is_pipeline_layout(base_dir)
    want_clip = bool(clip_source) and clip_source.lower() != "none"
    if pipeline:
        cfgs = ck.pipeline_configs(base_dir)
        arch = ck.parse_clip_source(clip_source)[0] if want_clip else builders.clip_arch(variant)
        unet, enc, text, vae = builders.build_from_configs(dev, cfgs["unet"], cfgs["text"], cfgs["vae"], arch, seed,
                                                           freeze_clip_vision=freeze_clip_vision)
        print(f"[e4t] architecture from {base_dir}: {ck.describe(cfgs)}; CLIP tower {arch}")
        load_pipeline_weights(base_dir, unet=unet, text=text, vae=vae)
    else:
        unet, enc, text, vae = builders.build_models(dev, variant, seed, freeze_clip_vision=freeze_clip_vision)
    if base_dir and not pipeline:
        if not os.path.isdir(base_dir):
            raise FileNotFoundError(f"{base_dir}: only local checkpoint directories are supported (no hub access in this build)")
        found = 0
        for name, mod, may_miss in (("unet", unet, lambda k: "wo" in k), ("vae", vae, lambda k: False), ("text_encoder", text, lambda k: False)):
            f = os.path.join(base_dir, f"{name}.pt")
            if os.path.exists(f):
                if name == "vae":       # an AutoencoderKL state dict also holds the decoder: keep the encoder half
                    sd = {k: v for k, v in torch.load(f, map_location="cpu").items() if k.startswith(("encoder.", "quant_conv."))}
                    missing, unexpected = mod.load_state_dict(sd, strict=False)
                    if missing or unexpected:
                        raise RuntimeError(f"{f}: missing {missing[:5]} unexpected {list(unexpected)[:5]}")
                else:
                    checked_load(mod, f, may_miss, what=f)
                found += 1
        if found == 0:
            raise FileNotFoundError(f"{base_dir} holds none of unet.pt / vae.pt / text_encoder.pt")
    if want_clip and not (e4t_dir and os.path.exists(os.path.join(e4t_dir, "encoder.pt"))):
        try:
            load_clip_tower(enc, clip_source)
        except ck.CheckpointNotFoundError as ex:
            if pipeline:
                raise SystemExit(f"{ex}\nThe E4T encoder's CLIP tower needs these weights next to a pretrained base model; "
                                 f"--clip_model_name_or_path none starts it from random init instead.")
            if base_dir:
                print(f"[e4t] WARNING: {ex}: the E4T encoder's CLIP tower stays randomly initialised", file=sys.stderr)
            else:
                print(f"[e4t] {ex}: randomly initialised CLIP tower (random base model)")
    if e4t_dir:
        for fn in ((names["weight_offsets.pt"],) if use_ema else ("weight_offsets.pt", "unet.pt")):
            f = os.path.join(e4t_dir, fn)
            if os.path.exists(f):
                checked_load(unet, f, (lambda k: "wo" not in k) if fn != "unet.pt" else (lambda k: False), what=f)
                print(f"Resuming from {f}")
        f = os.path.join(e4t_dir, names["encoder.pt"])
        if os.path.exists(f):
            checked_load(enc, f, what=f)
            print(f"Resuming from {f}")
    return unet, enc, text, vae


# ---- token merging (e4t/tome.py): a runtime choice of the three command lines, not a property of the run ------------------------
TOME_ARGS = ("tome_ratio", "tome_no_rand")       # utils.save_config leaves them out of config.json


def add_tome_args(p):
    p.add_argument("--tome_ratio", type=float, default=0.0,
                   help="token merging (ToMe) around the UNet's self-attention at the input resolution: the share of tokens merged, "
                        "0 = off (default), at most 0.75")
    p.add_argument("--tome_no_rand", action="store_true", help="ToMe: the top-left token of every 2x2 cell is the dst token (no per-step draw)")


def check_tome_args(p, args):
    from .tome import MAX_RATIO
    if not (0.0 <= args.tome_ratio <= MAX_RATIO):
        p.error(f"--tome_ratio must lie in [0, {MAX_RATIO}]")


def apply_tome_args(unet, args):
    """--tome_ratio > 0: mark the UNet (e4t.tome.apply_tome) with a generator of ToMe's own seeded from --seed; returns the state or None"""
    if not getattr(args, "tome_ratio", 0.0):
        return None
    from . import tome
    g = torch.Generator().manual_seed(int(getattr(args, "seed", None) or 0))
    return tome.apply_tome(unet, args.tome_ratio, use_rand=not args.tome_no_rand, generator=g)


# ---- FreeU (e4t/freeu.py): like ToMe a runtime choice of the command line (inference.py), config.json does not record it ---------------------------
FREEU_ARGS = ("freeu", "freeu_b1", "freeu_b2", "freeu_s1", "freeu_s2", "freeu_version")


def add_freeu_args(p):
    p.add_argument("--freeu", action="store_true",
                   help="FreeU at the UNet's decoder concatenations: amplify half of the backbone channels and damp the skip connections' "
                        "lowest frequencies (no training, no weights; DESIGN §2.5c)")
    p.add_argument("--freeu_b1", type=float, default=None, help="backbone factor of stage 1 (the widest maps), >= 1; default 1.3 (version 1: 1.2)")
    p.add_argument("--freeu_b2", type=float, default=None, help="backbone factor of stage 2, >= 1; default 1.4")
    p.add_argument("--freeu_s1", type=float, default=None, help="skip factor of stage 1, in [0, 1]; default 0.9")
    p.add_argument("--freeu_s2", type=float, default=None, help="skip factor of stage 2, in [0, 1]; default 0.2")
    p.add_argument("--freeu_version", type=int, choices=(1, 2), default=2,
                   help="2 (default): the backbone factor follows the normalised channel mean of every pixel; 1: a constant factor")


def check_freeu_args(p, args):
    from .freeu import DEFAULTS
    given = [n for n in ("freeu_b1", "freeu_b2", "freeu_s1", "freeu_s2") if getattr(args, n) is not None]
    if given and not args.freeu:
        p.error(f"--{given[0]} needs --freeu")
    for n, dflt in DEFAULTS[args.freeu_version].items():
        if getattr(args, "freeu_" + n) is None:
            setattr(args, "freeu_" + n, dflt)
    for n in ("freeu_b1", "freeu_b2"):
        v = getattr(args, n)
        if not (v >= 1.0 and v != float("inf")):
            p.error(f"--{n} must be finite and >= 1")
    for n in ("freeu_s1", "freeu_s2"):
        if not 0.0 <= getattr(args, n) <= 1.0:
            p.error(f"--{n} must lie in [0, 1]")


def apply_freeu_args(unet, args):
    """--freeu: mark the UNet (e4t.freeu.apply_freeu); returns the state or None"""
    if not getattr(args, "freeu", False):
        return None
    from . import freeu
    return freeu.apply_freeu(unet, args.freeu_b1, args.freeu_b2, args.freeu_s1, args.freeu_s2, version=args.freeu_version)


# ---- the diffusion objective's options (E4TTrainer(snr_gamma=..., noise_offset=..., loss_type=...)): properties of the run, so config.json
# records them like reg_lambda; tuning_e4t.py takes its own flags and inherits neither from the pre-trained run's config.json ----
def add_objective_args(p):
    p.add_argument("--snr_gamma", type=float, default=None,
                   help="min-SNR-gamma loss weighting: each image's loss is weighted by min(SNR(t), gamma) / SNR(t) (the usual choice is 5); "
                        "must be > 0, default off")
    p.add_argument("--noise_offset", type=float, default=0.0,
                   help="noise offset: a per-(image, channel) N(0, 1) constant times this scale is added to the noise (0.05 - 0.1 is usual); "
                        "must be >= 0, default 0 = off")
    p.add_argument("--loss_type", choices=("l2", "huber", "smooth_l1"), default="l2",
                   help="the diffusion loss: l2 (default, squared error), or the scheduled pseudo-Huber loss / its smooth-L1 form, quadratic "
                        "for small residuals and linear for large ones (DESIGN §2.4b)")
    p.add_argument("--huber_c", type=float, default=0.1,
                   help="the Huber parameter: the transition point under --huber_schedule constant, its floor at the noisiest timestep "
                        "otherwise; finite and > 0, and <= 1 unless the schedule is constant (default 0.1)")
    p.add_argument("--huber_schedule", choices=("constant", "exponential", "snr"), default="snr",
                   help="how the Huber parameter depends on the timestep: constant, exponential (1 at t = 0 decaying to huber_c) or snr "
                        "((1 - huber_c) / (1 + sigma_t)^2 + huber_c, default)")
    p.add_argument("--optimizer_state_bits", type=int, choices=(32, 8), default=32,
                   help="AdamW's moments: 32 (default, two fp32 buffers) or 8 (block-wise 8-bit: one byte per moment plus one fp32 scale per 256 "
                        "elements, about 2 instead of 8 bytes of optimiser state per parameter; DESIGN §2.3d)")


def check_objective_args(p, args):
    if args.snr_gamma is not None and not args.snr_gamma > 0.0:
        p.error("--snr_gamma must be > 0")
    if not args.noise_offset >= 0.0:
        p.error("--noise_offset must be >= 0")
    if not (args.huber_c > 0.0 and args.huber_c != float("inf")):
        p.error("--huber_c must be finite and > 0")
    if args.huber_schedule != "constant" and args.huber_c > 1.0:
        p.error(f"--huber_c must be <= 1 with --huber_schedule {args.huber_schedule}")


def objective_kwargs(args):
    """the E4TTrainer keyword arguments of add_objective_args' flags (a namespace without them: all off, 32-bit optimiser state)"""
    return dict(snr_gamma=getattr(args, "snr_gamma", None), noise_offset=getattr(args, "noise_offset", 0.0),
                loss_type=getattr(args, "loss_type", "l2"), huber_c=getattr(args, "huber_c", 0.1),
                huber_schedule=getattr(args, "huber_schedule", "snr"), optimizer_state_bits=getattr(args, "optimizer_state_bits", 32))


# ---- EMA of the trained weights (E4TTrainer(ema_decay=...)): like ToMe a choice of the command line, config.json does not record it --------------
EMA_ARGS = ("use_ema", "ema_decay")              # utils.save_config leaves them out of config.json
EMA_DEFAULT_DECAY = 0.9999
EMA_FILES = {"weight_offsets.pt": "weight_offsets_ema.pt", "encoder.pt": "encoder_ema.pt"}


def add_ema_args(p, training=True):
    """training=True (pretrain_e4t.py): --use_ema keeps the average and writes the *_ema files, --ema_decay sets its decay.
    training=False (tuning_e4t.py, inference.py): --use_ema loads the *_ema files of the directory given."""
    if training:
        p.add_argument("--use_ema", action="store_true",
                       help="keep an exponential moving average of the trained weights (fused into AdamW): every checkpoint directory gains "
                            "weight_offsets_ema.pt / encoder_ema.pt and the training-time samples are drawn from the average")
        p.add_argument("--ema_decay", type=float, default=None,
                       help=f"EMA decay in (0, 1), default {EMA_DEFAULT_DECAY}; warmed up as min(decay, (1 + t) / (10 + t)).  Needs --use_ema")
    else:
        p.add_argument("--use_ema", action="store_true",
                       help="load the averaged weights (weight_offsets_ema.pt / encoder_ema.pt, written by pretrain_e4t.py --use_ema)")


def check_ema_args(p, args):
    decay = getattr(args, "ema_decay", None)
    if decay is not None and not args.use_ema:
        p.error("--ema_decay needs --use_ema")
    if decay is not None and not 0.0 < decay < 1.0:
        p.error("--ema_decay must lie in (0, 1)")
    if args.use_ema and hasattr(args, "ema_decay") and decay is None:
        args.ema_decay = EMA_DEFAULT_DECAY


def ema_file_names(e4t_dir, use_ema):
    """file name -> the name to read in `e4t_dir`: with --use_ema the *_ema twins, which must both be there (SystemExit names what is missing)"""
    if not use_ema:
        return {k: k for k in EMA_FILES}
    missing = [v for v in EMA_FILES.values() if not (e4t_dir and os.path.exists(os.path.join(e4t_dir, v)))]
    if missing:
        raise SystemExit(f"--use_ema: {e4t_dir!r} holds no {' / '.join(missing)} (averaged weights are written by pretrain_e4t.py --use_ema)")
    return dict(EMA_FILES)
