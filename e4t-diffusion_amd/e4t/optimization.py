"""Learning-rate schedules of the reference's ``--lr_scheduler`` flag (pretrain_e4t.py:110-111,402-408 →
``diffusers.optimization.get_scheduler``; [3P] diffusers 0.14, restated): a multiplier lambda(step) on the base rate, stepped
once per optimiser step.  The native trainer has no ``torch.optim`` object: ``LRSchedule.apply(trainer)`` sets the scalar the
fused AdamW kernel receives."""
from __future__ import annotations

import math

SCHEDULES = ("linear", "cosine", "cosine_with_restarts", "polynomial", "constant", "constant_with_warmup")


def get_lr_lambda(name: str, num_warmup_steps: int = 0, num_training_steps: int = 0, num_cycles=None, power: float = 1.0,
                  lr_init: float = 1.0, lr_end: float = 1e-7):
    if name not in SCHEDULES:
        raise ValueError(f"{name} is not a valid scheduler: choose from {list(SCHEDULES)}")
    w, T = num_warmup_steps, num_training_steps
    if name == "constant":
        return lambda step: 1.0
    if name == "constant_with_warmup":
        return lambda step: float(step) / float(max(1.0, w)) if step < w else 1.0
    if name == "linear":
        return lambda step: float(step) / float(max(1, w)) if step < w else max(0.0, float(T - step) / float(max(1, T - w)))
    if name == "cosine":
        nc = 0.5 if num_cycles is None else num_cycles

        def f(step):
            if step < w:
                return float(step) / float(max(1, w))
            progress = float(step - w) / float(max(1, T - w))
            return max(0.0, 0.5 * (1.0 + math.cos(math.pi * float(nc) * 2.0 * progress)))
        return f
    if name == "cosine_with_restarts":
        nc = 1 if num_cycles is None else num_cycles

        def f(step):
            if step < w:
                return float(step) / float(max(1, w))
            progress = float(step - w) / float(max(1, T - w))
            if progress >= 1.0:
                return 0.0
            return max(0.0, 0.5 * (1.0 + math.cos(math.pi * ((float(nc) * progress) % 1.0))))
        return f
    # polynomial
    if not lr_init > lr_end:
        raise ValueError(f"lr_end ({lr_end}) must be be smaller than initial lr ({lr_init})")

    def f(step):
        if step < w:
            return float(step) / float(max(1, w))
        if step > T:
            return lr_end / lr_init
        decay = (lr_init - lr_end) * (1 - (step - w) / (T - w)) ** power + lr_end
        return decay / lr_init
    return f


class LRSchedule:
    """``get_scheduler(name, optimizer, num_warmup_steps, num_training_steps)`` for the native trainer."""

    def __init__(self, name, base_lr, num_warmup_steps=0, num_training_steps=0, last_step=0):
        self.base_lr, self.step_count = base_lr, last_step
        self.fn = get_lr_lambda(name, num_warmup_steps, num_training_steps, lr_init=base_lr)

    def get_last_lr(self):
        return [self.base_lr * self.fn(self.step_count)]

    def apply(self, trainer):
        trainer.lr = self.get_last_lr()[0]

    def step(self):
        self.step_count += 1


def ema_weight(decay: float, t: int) -> float:
    """Weight w = 1 - d_t of the parameters in the EMA update e' = e - w * (e - p) at the 1-based optimiser step t, with LDM's (LitEma) /
    diffusers' (EMAModel) warm-up d_t = min(decay, (1 + t) / (10 + t)) so that the first steps are not dominated by the initial weights.
    Computed in double and rounded ONCE to fp32 (returned as the Python float of that fp32 value): the eager launch argument, the step graph's
    device scalar and the tests all take it from here, the only statement of the formula."""
    import ctypes
    if not 0.0 < decay < 1.0:
        raise ValueError(f"EMA decay {decay!r} must lie in (0, 1)")
    if t < 1:
        raise ValueError(f"optimiser steps count from 1, got {t}")
    return ctypes.c_float(1.0 - min(float(decay), (1.0 + t) / (10.0 + t))).value


# ---- block-wise 8-bit AdamW moments (E4TTrainer(optimizer_state_bits=8)) ---------------------------------------------------
# The fp32 torch composition below is the DEFINITION of the format: the codebooks and the rounding rule are stated here and nowhere else;
# adamw8_kernel (csrc/optim.hip) receives the codebooks as device arrays and restates the rule, the tests take both from here.
ADAM8_BLOCK = 256


def dynamic_codebook(signed: bool):
    """The dynamic-tree map in bitsandbytes' style as fp32 [256], sorted ascending.  For i in 0..6: k = 2^i + 1 (signed) or 2^(i+1) + 1
    (unsigned) points linspace(0.1, 1, k) in float64, the midpoints of neighbouring points times 10^(i-6); the signed map also takes the
    negatives; 0.0 and 1.0 are appended; rounded once to fp32.  Both maps hold 256 distinct values; the signed one runs from -0.99296874
    to 1.0 (it has no -1), index 0 of the unsigned one is 0.0."""
    import torch
    vals = []
    for i in range(7):
        k = 2 ** i + 1 if signed else 2 ** (i + 1) + 1
        pts = torch.linspace(0.1, 1, k, dtype=torch.float64)
        mid = (pts[:-1] + pts[1:]) / 2.0 * 10.0 ** (i - 6)
        vals.append(mid)
        if signed:
            vals.append(-mid)
    vals.append(torch.tensor([0.0, 1.0], dtype=torch.float64))
    code = torch.cat(vals).to(torch.float32).sort().values
    assert code.numel() == 256 and bool((code[1:] > code[:-1]).all())
    return code


def quantize_blockwise(x, code):
    """fp32 [n] -> (q uint8 [n], absmax fp32 [ceil(n / 256)]).  Per block of 256 consecutive elements (the last may be short): a = max|x|,
    y = x / a by fp32 division (0 where a == 0), q = the index of the code value nearest to y with the distances y - code[lo] and code[hi] - y
    taken in fp32 between the two neighbours lo = hi - 1 and hi = #{j < 255: code[j] < y}; the LOWER index on an exact tie."""
    import torch
    x = x.detach().reshape(-1).to(torch.float32)
    code = code.to(x.device)
    n = x.numel()
    nb = -(-n // ADAM8_BLOCK)
    xp = torch.zeros(nb * ADAM8_BLOCK, dtype=torch.float32, device=x.device)
    xp[:n] = x
    xp = xp.view(nb, ADAM8_BLOCK)
    a = xp.abs().amax(dim=1)
    y = torch.where(a[:, None] > 0, xp / a[:, None], torch.zeros_like(xp))
    hi = torch.searchsorted(code[:255].contiguous(), y.contiguous())
    lo = (hi - 1).clamp_min(0)
    q = torch.where(y - code[lo] <= code[hi] - y, lo, hi).to(torch.uint8)
    return q.view(-1)[:n].clone(), a


def dequantize_blockwise(q, absmax, code):
    """code[q] * absmax[block], fp32 [n]"""
    import torch
    code = code.to(q.device)
    return code[q.long()] * absmax.repeat_interleave(ADAM8_BLOCK)[:q.numel()]


class Adam8State:
    """AdamW's two moments of a flat buffer of n parameters as one byte each plus one fp32 scale per 256 elements: exp_avg through the signed
    codebook, exp_avg_sq through the unsigned one.  A fresh state has every scale 0 and every code the index of 0.0 in its codebook (byte 0 of
    the signed map is -0.993: a zero-filled byte buffer is NOT a fresh state)."""
    BUFFERS = ("qm", "qv", "absmax_m", "absmax_v")
    CHUNK = ADAM8_BLOCK << 16          # quantize_from works through whole blocks, 16 M elements at a time: quantize_blockwise's temporaries are ~50 B per element

    def __init__(self, n, device):
        import torch
        self.n, self.block = int(n), ADAM8_BLOCK
        nb = -(-self.n // ADAM8_BLOCK)
        code_m, code_v = dynamic_codebook(True), dynamic_codebook(False)
        self.zero_m, self.zero_v = (int((c == 0).nonzero()[0]) for c in (code_m, code_v))
        self.code_m, self.code_v = code_m.to(device), code_v.to(device)
        self.qm = torch.full((self.n,), self.zero_m, dtype=torch.uint8, device=device)
        self.qv = torch.full((self.n,), self.zero_v, dtype=torch.uint8, device=device)
        self.absmax_m = torch.zeros(nb, dtype=torch.float32, device=device)
        self.absmax_v = torch.zeros(nb, dtype=torch.float32, device=device)

    def buffers(self):
        return tuple(getattr(self, k) for k in self.BUFFERS)

    def dequantize(self):
        """-> (exp_avg, exp_avg_sq) as fp32 [n], for inspection and for handing the state to a 32-bit trainer"""
        return dequantize_blockwise(self.qm, self.absmax_m, self.code_m), dequantize_blockwise(self.qv, self.absmax_v, self.code_v)

    def quantize_from(self, exp_avg, exp_avg_sq):
        """take fp32 moments (a 32-bit trainer's state) through quantize_blockwise"""
        chunk = self.CHUNK
        for (qk, ak), x, code in ((("qm", "absmax_m"), exp_avg, self.code_m), (("qv", "absmax_v"), exp_avg_sq, self.code_v)):
            x = x.reshape(-1)
            for o in range(0, self.n, chunk):
                q, a = quantize_blockwise(x[o:o + chunk].to(self.qm.device), code)
                getattr(self, qk)[o:o + chunk].copy_(q)
                getattr(self, ak)[o // ADAM8_BLOCK:o // ADAM8_BLOCK + a.numel()].copy_(a)

    def nbytes(self):
        return sum(b.numel() * b.element_size() for b in self.buffers())
