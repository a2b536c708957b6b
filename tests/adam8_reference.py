"""TEST-ONLY references for AdamW with block-wise 8-bit moments (e4t_adamw8):
  * adamw8_f64: the float64 restatement of one step (the GPU kernel is compared against it), with the distance of every normalised moment to
    the nearest code midpoint, so that a test can tell a code that may legitimately flip from one that may not;
  * Adam8EmuBackend: tests/ema_reference.py's double with adamw8 added (fp32, the kernel's operation order), swapped in through
    e4t.ops.set_backend() by the CPU host-logic tests.
The codebooks and the rounding rule are e4t.optimization's: that module is their only statement.  The product never imports this file."""
from __future__ import annotations

import math

import torch

from ema_reference import EmaEmuBackend, bias_corrections, ema_update_f64, f32r, _adamw_f64

f64 = torch.float64
BLOCK = 256


def _blocks(x, fill=0.0):
    n = x.numel()
    nb = -(-n // BLOCK)
    out = torch.full((nb * BLOCK,), fill, dtype=x.dtype, device=x.device)
    out[:n] = x
    return out.view(nb, BLOCK)


def quantize_f64(x, code):
    """float64 restatement of optimization.quantize_blockwise -> (q int64 [n], absmax f64 [nb], band f64 [n]): band is the distance of the
    normalised value y to the nearest midpoint of two neighbouring code values, relative to max(|y|, the midpoint's magnitude)"""
    n = x.numel()
    c = code.to(f64).to(x.device)
    xb = _blocks(x.to(f64))
    a = xb.abs().amax(dim=1)
    y = torch.where(a[:, None] > 0, xb / a[:, None].clamp_min(1e-300), torch.zeros_like(xb))
    hi = torch.searchsorted(c[:255].contiguous(), y.contiguous())
    lo = (hi - 1).clamp_min(0)
    q = torch.where(y - c[lo] <= c[hi] - y, lo, hi)
    mid = (c[:-1] + c[1:]) / 2
    j = torch.searchsorted(mid, y.contiguous()).clamp(1, 254)
    near = torch.minimum((y - mid[j - 1]).abs() / torch.maximum(y.abs(), mid[j - 1].abs()).clamp_min(1e-300),
                         (y - mid[j]).abs() / torch.maximum(y.abs(), mid[j].abs()).clamp_min(1e-300))
    return q.view(-1)[:n], a, near.view(-1)[:n]


def dequantize_f64(q, absmax, code):
    """the moments a state denotes, as float64: they ARE the fp32 numbers optimization.dequantize_blockwise returns (one fp32 product per element; that
    function is the definition of what a state means), so the restatement starts from those, as adamw_ema_f64 starts from fp32 m and v"""
    from e4t.optimization import dequantize_blockwise
    return dequantize_blockwise(q.to(torch.uint8), absmax.to(torch.float32), code).to(f64)


def adamw8_f64(p, g, qm, qv, absmax_m, absmax_v, code_m, code_v, lr, beta1, beta2, eps, wd, step, grad_scale, ema=None, ema_w=0.0):
    """one e4t_adamw8 step in float64 from fp32 / uint8 inputs (bias corrections as the entry point forms them)
    -> dict(p, qm, qv, absmax_m, absmax_v, band_m, band_v, m, v[, ema])"""
    bc1, bc2s = bias_corrections(beta1, beta2, step)
    m, v = dequantize_f64(qm, absmax_m, code_m), dequantize_f64(qv, absmax_v, code_v)
    p2, m2, v2 = _adamw_f64(p, g.to(f64) * f32r(grad_scale), m, v, lr, beta1, beta2, eps, wd, bc1, bc2s)
    q_m, a_m, band_m = quantize_f64(m2, code_m)
    q_v, a_v, band_v = quantize_f64(v2, code_v)
    out = dict(p=p2, qm=q_m, qv=q_v, absmax_m=a_m, absmax_v=a_v, band_m=band_m, band_v=band_v, m=m2, v=v2)
    if ema is not None:
        out["ema"] = ema_update_f64(ema, p2, ema_w)
    return out


def adamw32_f64_trajectory(p0, grads, lr, beta1, beta2, eps, wd, grad_scale=1.0):
    """float64 AdamW with unquantised moments over a gradient sequence -> the parameters after the last step"""
    p, m, v = p0.to(f64), torch.zeros_like(p0, dtype=f64), torch.zeros_like(p0, dtype=f64)
    for t, g in enumerate(grads, start=1):
        bc1, bc2s = bias_corrections(beta1, beta2, t)
        p, m, v = _adamw_f64(p, g.to(f64) * f32r(grad_scale), m, v, lr, beta1, beta2, eps, wd, bc1, bc2s)
    return p


# ---- the emulation with adamw8 ---------------------------------------------------------------------------------------------------------
class Adam8EmuBackend(EmaEmuBackend):
    def adamw8(self, p, g, qm, qv, absmax_m, absmax_v, code_m, code_v, lr, beta1, beta2, eps, wd, step, grad_scale=1.0, ema=None, ema_w=0.0, hyper=None):
        from e4t.optimization import dequantize_blockwise, quantize_blockwise
        n = p.numel()
        assert qm.numel() == n and qv.numel() == n and absmax_m.numel() == -(-n // BLOCK) == absmax_v.numel()
        m, v = dequantize_blockwise(qm, absmax_m, code_m), dequantize_blockwise(qv, absmax_v, code_v)
        if hyper is not None:
            h = hyper.tolist()
            lr, bc1, bc2s, grad_scale = h[:4]
            if ema is not None:
                ema_w = h[4]
        else:          # (EmuBackend.adamw's host arithmetic: from a fresh state the two emulations agree bit for bit)
            bc1, bc2s = 1 - beta1 ** step, math.sqrt(1 - beta2 ** step)
        gg = g * grad_scale
        p.mul_(1 - lr * wd)
        m.mul_(beta1).add_(gg, alpha=1 - beta1)
        v.mul_(beta2).addcmul_(gg, gg, value=1 - beta2)
        p.addcdiv_(m, v.sqrt() / bc2s + eps, value=-lr / bc1)
        for (q_out, a_out), x, code in (((qm, absmax_m), m, code_m), ((qv, absmax_v), v, code_v)):
            q, a = quantize_blockwise(x, code)
            q_out.copy_(q)
            a_out.copy_(a)
        if ema is not None:
            self._ema(ema, p, ema_w)
