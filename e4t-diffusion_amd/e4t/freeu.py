"""FreeU (Si et al., "FreeU: Free Lunch in Diffusion U-Net", 2023) for the UNet's decoder — sampling only, opt-in.

``apply_freeu(unet, b1, b2, s1, s2, version)`` marks the up-block ResBlocks whose hidden input is ``block_out_channels[-1]`` wide (stage 1:
``b1, s1``) or half that (stage 2: ``b2, s2``), as the authors' code chooses them.  The up blocks never materialise ``torch.cat([hidden,
skip])``: they hand the pair to the ResBlock, and a marked ResBlock's pair passes through ``transform`` first — two launches of csrc/freeu.hip
(e4t_freeu_stats / e4t_freeu_apply):

    backbone  h' = h * ((b - 1) m^ + 1) on the first C_h / 2 channels; version 2 (the default): m = the mean over the C_h channels,
              m^ = (m - min) / (max - min) per image; version 1: m^ = 1, i.e. h' = b h
    skip      k' = k + (s - 1) LP(k): LP keeps the frequencies {0, -1} x {0, -1} of the map's 2-D DFT, which is all the usual fftn ->
              fftshift -> scale the centre box of threshold 1 -> ifftshift -> ifftn -> real touches

Where an image's channel mean is constant over the map (max == min) m^ is 0 here; the authors' code divides by zero there.  Every image of the
batch — every branch of a guided batch — is treated on its own.  ``remove_freeu(unet)`` removes the marks; a model that was never marked runs
exactly the launches it ran before this module existed.  There is no backward: a marked model asked for a gradient raises."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import ops

DEFAULTS = {2: dict(b1=1.3, b2=1.4, s1=0.9, s2=0.2), 1: dict(b1=1.2, b2=1.4, s1=0.9, s2=0.2)}     # the authors' SD-1.4 values


def check_params(b1, b2, s1, s2, version):
    if version not in (1, 2):
        raise ValueError(f"freeu version must be 1 or 2, got {version}")
    for name, b in (("b1", b1), ("b2", b2)):
        if not (float(b) >= 1.0 and float(b) != float("inf")):
            raise ValueError(f"freeu {name} must be finite and >= 1, got {b}")
    for name, s in (("s1", s1), ("s2", s2)):
        if not 0.0 <= float(s) <= 1.0:
            raise ValueError(f"freeu {name} must lie in [0, 1], got {s}")


class FreeuState:
    def __init__(self, b1: float, b2: float, s1: float, s2: float, version: int = 2):
        check_params(b1, b2, s1, s2, version)
        self.b1, self.b2, self.s1, self.s2, self.version = float(b1), float(b2), float(s1), float(s2), int(version)
        self.stages: Dict[str, int] = {}          # "up_blocks.<i>.resnets.<j>" -> 1 | 2, in forward order

    def params(self, stage: int):
        return (self.b1, self.s1) if stage == 1 else (self.b2, self.s2)

    def transform(self, stage: int, m, skip):
        """(m, skip) -> (m', skip'): FMaps in, new FMaps out"""
        from .models.resnet import FMap
        if torch.is_grad_enabled() and (m.x.requires_grad or skip.x.requires_grad):
            raise RuntimeError("FreeU is sampling-only: no backward is built (run the marked model under torch.no_grad(), or remove_freeu first)")
        if (skip.B, skip.H, skip.W) != (m.B, m.H, m.W):
            raise ValueError(f"freeu: hidden map {(m.B, m.H, m.W)} and skip map {(skip.B, skip.H, skip.W)} differ")
        b, s = self.params(stage)
        be = ops.backend()
        ws = be.freeu_stats(m.x, skip.x, m.B, m.H, m.W, self.version)
        h2, k2 = be.freeu_apply(m.x, skip.x, ws, m.B, m.H, m.W, b, s, self.version)
        return FMap(h2, m.B, m.H, m.W), FMap(k2, m.B, m.H, m.W)


def _up_resnets(unet):
    """(name, ResBlock, width of its hidden input) of every up-block ResBlock in forward order: the first ResBlock of a block receives the
    previous block's output (the mid block's for the first), the others their own block's"""
    prev = int(unet.config.block_out_channels[-1])
    for i, blk in enumerate(unet.up_blocks):
        out_ch = blk.resnets[0].out_channels
        for j, r in enumerate(blk.resnets):
            yield f"up_blocks.{i}.resnets.{j}", r, prev if j == 0 else out_ch
        prev = out_ch


def get_state(unet) -> Optional[FreeuState]:
    return getattr(unet, "_freeu", None)


def apply_freeu(unet, b1: float, b2: float, s1: float, s2: float, version: int = 2) -> FreeuState:
    """Mark the up-block ResBlocks by the stage rule; returns the state, whose ``stages`` lists which ResBlock got which stage."""
    remove_freeu(unet)
    st = FreeuState(b1, b2, s1, s2, version)
    c_top = int(unet.config.block_out_channels[-1])
    for name, r, c_h in _up_resnets(unet):
        stage = 1 if c_h == c_top else 2 if c_h == c_top // 2 else 0
        if stage:
            r._freeu = (st, stage)
            st.stages[name] = stage
    unet._freeu = st
    return st


def remove_freeu(unet):
    if get_state(unet) is None:
        return
    for _, r, _ in _up_resnets(unet):
        if "_freeu" in r.__dict__:
            del r._freeu
    del unet._freeu
