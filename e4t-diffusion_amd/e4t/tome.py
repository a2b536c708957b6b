"""Token merging (ToMe, Bolya & Hoffman, "Token Merging for Stable Diffusion") for the UNet's self-attention — opt-in.

The reference's last open TODO ("Support ToMe for more efficient training", README.md:116).  ``apply_tome(unet, ratio)`` marks every
``BasicTransformerBlock`` of the UNet; a marked block whose level qualifies (``ceil(sqrt(T_latent / T)) <= max_downsample``) runs

    LN -> match on the block input -> merge(LN(x)) -> attn1 on (B, T', d) -> unmerge + residual

on the kernels of csrc/tome.hip (e4t_tome_match / e4t_tome_merge / e4t_tome_unmerge).  Only ``attn1`` is merged: no cross-attention or MLP
merging, no proportional attention, 2x2 cells only, nothing in the ViT.  ``remove_tome(unet)`` restores the unmarked model; a model that
was never marked runs exactly the launches it ran before this module existed.

Randomness: which token of every 2x2 cell is the dst token is ONE draw per step (``new_step``), shared by all blocks of a level and by
every UNet pass of the step, from a generator of ToMe's own — the noise / timestep streams of training and sampling are not touched.  The
draw lives in a fixed device buffer that ``new_step`` refreshes in place, so a captured step (the trainer's step graph, the sampler's
hipGraph loop) replays with the new choice; shapes are static (r follows from the ratio alone).

Plans are data (``ops.TomePlan``): ``state.record = True`` keeps the plans a run computed, ``state.plans = [...]`` makes a run use the
given plans in call order instead of matching — how two back ends are compared without depending on how each breaks a near-tie.
"""
from __future__ import annotations

import math
from typing import List, Optional

import torch

from . import ops

MAX_RATIO = 0.75


class TomeState:
    def __init__(self, ratio: float, max_downsample: int = 1, use_rand: bool = True, generator: Optional[torch.Generator] = None):
        if not (0.0 < ratio <= MAX_RATIO):
            raise ValueError(f"tome ratio must lie in (0, {MAX_RATIO}], got {ratio}")
        self.ratio, self.max_downsample, self.use_rand = float(ratio), int(max_downsample), bool(use_rand)
        self.generator = generator if generator is not None else torch.Generator().manual_seed(0)     # ToMe's own stream (host side)
        self.latent_tokens: Optional[int] = None       # tokens of the UNet's input map, recorded by the forward pre-hook
        self.plans: Optional[List[ops.TomePlan]] = None
        self.record = False
        self.recorded: List[ops.TomePlan] = []
        self._cursor = 0
        self._choice = {}                               # (h, w, device) -> int32 [(h/2)*(w/2)] device buffer, refreshed in place
        self._hook = None

    # ---- what is merged -------------------------------------------------------------------------------------------------------
    def r_for(self, T: int) -> int:
        return min(T - T // 4, int(T * self.ratio))

    def applies(self, T: int, h: int, w: int) -> bool:
        if self.latent_tokens is None or h % 2 or w % 2 or h * w != T or self.r_for(T) < 1:
            return False
        return math.ceil(math.sqrt(self.latent_tokens / T)) <= self.max_downsample

    # ---- the per-step draw ----------------------------------------------------------------------------------------------------
    def _draw(self, n: int) -> torch.Tensor:
        return torch.randint(0, 4, (n,), generator=self.generator, dtype=torch.int32)

    def choice(self, h: int, w: int, device) -> Optional[torch.Tensor]:
        if not self.use_rand:
            return None
        key = (h, w, str(device))
        buf = self._choice.get(key)
        if buf is None:                                 # first sight of this level (an eager warm-up step: never inside a capture)
            buf = self._choice[key] = self._draw((h // 2) * (w // 2)).to(device)
        return buf

    def new_step(self):
        """Start a training / denoising step: a fresh draw into every level's buffer (in place: captured graphs read the same memory)
        and the injected plans are read from the top again."""
        self._cursor = 0
        for (h, w, _), buf in self._choice.items():
            buf.copy_(self._draw((h // 2) * (w // 2)))

    # ---- the plan of one block call ---------------------------------------------------------------------------------------------
    def plan_for(self, x2d: torch.Tensor, B: int, h: int, w: int) -> ops.TomePlan:
        if self.plans is not None:
            if self._cursor >= len(self.plans):
                raise RuntimeError(f"tome: {len(self.plans)} plans were injected, a further block asked for one")
            plan = self.plans[self._cursor]
            self._cursor += 1
            if (plan.B, plan.T, plan.r) != (B, h * w, self.r_for(h * w)):
                raise RuntimeError(f"tome: injected plan {self._cursor - 1} is for (B, T, r) = {(plan.B, plan.T, plan.r)}, the block has "
                                   f"{(B, h * w, self.r_for(h * w))}")
            return plan
        with torch.no_grad():
            plan = ops.backend().tome_match(x2d.detach(), B, h, w, self.r_for(h * w), self.choice(h, w, x2d.device))
        if self.record:
            self.recorded.append(plan)
        return plan


def _blocks(unet):
    from .models.attention import BasicTransformerBlock
    return [m for m in unet.modules() if isinstance(m, BasicTransformerBlock)]


def get_state(unet) -> Optional[TomeState]:
    return getattr(unet, "_tome", None)


def new_step(unet):
    """what a trainer / sampler calls once per step; a no-op for a model without ToMe"""
    st = get_state(unet)
    if st is not None:
        st.new_step()


def apply_tome(unet, ratio: float, max_downsample: int = 1, use_rand: bool = True, generator: Optional[torch.Generator] = None,
               plans=None, record: bool = False) -> TomeState:
    """Merge ``ratio`` of the tokens around ``attn1`` of every transformer block at most ``max_downsample`` x below the UNet's input
    resolution (1: the 64x64 level at 512 px).  Returns the state object (ratio, the current choice buffers, injected / recorded plans)."""
    remove_tome(unet)
    st = TomeState(ratio, max_downsample, use_rand, generator)
    st.plans, st.record = plans, record

    def pre(module, args, kwargs):
        sample = args[0] if args else kwargs["sample"]
        st.latent_tokens = int(sample.shape[-2]) * int(sample.shape[-1])

    st._hook = unet.register_forward_pre_hook(pre, with_kwargs=True)
    unet._tome = st
    for blk in _blocks(unet):
        blk._tome = st
    return st


def remove_tome(unet):
    st = get_state(unet)
    if st is None:
        return
    if st._hook is not None:
        st._hook.remove()
    for blk in _blocks(unet):
        if "_tome" in blk.__dict__:
            del blk._tome
    del unet._tome
