"""TEST-ONLY references for the EMA of the trained weights (e4t_adamw_ema / e4t_adamw_rank_ema / e4t_ema_update):
  * a float64 restatement of the three ops (the GPU kernels are compared against it);
  * EmaEmuBackend: tests/emu_backend.py's double with the three ops added (fp32, the operation order of the device helper), swapped in
    through e4t.ops.set_backend() by the CPU host-logic tests;
  * ema_trajectory: the recurrence over per-step parameter snapshots, in float64.
The product never imports this file."""
from __future__ import annotations

import numpy as np
import torch

from emu_backend import EmuBackend

f64 = torch.float64


def f32r(x):
    """x rounded to fp32, as a Python float (what a kernel sees of a float launch argument)"""
    return float(np.float32(x))


def bias_corrections(beta1, beta2, step):
    """e4t_adamw's host arithmetic, bit for bit: 1 - powf(beta1, t) and sqrtf(1 - powf(beta2, t)) in fp32 through the C library (the figures a
    hyper_dev buffer carries)"""
    import ctypes
    libm = ctypes.CDLL("libm.so.6")
    libm.powf.restype, libm.powf.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
    libm.sqrtf.restype, libm.sqrtf.argtypes = ctypes.c_float, [ctypes.c_float]
    return f32r(1.0 - libm.powf(beta1, float(step))), libm.sqrtf(f32r(1.0 - libm.powf(beta2, float(step))))


# ---- float64 restatement ------------------------------------------------------------------------------------------------------
def ema_update_f64(ema, p, w):
    """e' = e - w * (e - p)"""
    e = ema.to(f64)
    return e - f32r(w) * (e - p.to(f64))


def _adamw_f64(p, g, m, v, lr, beta1, beta2, eps, wd, bc1, bc2s):
    lr, beta1, beta2, eps, wd = (f32r(x) for x in (lr, beta1, beta2, eps, wd))
    p, g, m, v = p.to(f64) * (1.0 - lr * wd), g.to(f64), m.to(f64), v.to(f64)
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    p = p - (lr / bc1) * m / (v.sqrt() / bc2s + eps)
    return p, m, v


def adamw_ema_f64(p, g, m, v, ema, lr, beta1, beta2, eps, wd, step, grad_scale, ema_w):
    """-> (p', m', v', ema') in float64 from fp32 inputs (bias corrections as the entry point forms them)"""
    bc1, bc2s = bias_corrections(beta1, beta2, step)
    p2, m2, v2 = _adamw_f64(p, g.to(f64) * f32r(grad_scale), m, v, lr, beta1, beta2, eps, wd, bc1, bc2s)
    return p2, m2, v2, ema_update_f64(ema, p2, ema_w)


def adamw_rank_ema_f64(p, m, v, ema, G, Z, lr, beta1, beta2, eps, wd, step, grad_scale, ema_w):
    """the stack form: dW_i = grad_scale * G^T Z[:, i*cols:(i+1)*cols] from the bf16 factors, then the same update"""
    n, rows, cols = p.shape
    g = torch.einsum("kr,knc->nrc", G.to(f64), Z.to(f64).view(G.shape[0], n, cols)) * f32r(grad_scale)
    bc1, bc2s = bias_corrections(beta1, beta2, step)
    p2, m2, v2 = _adamw_f64(p, g, m, v, lr, beta1, beta2, eps, wd, bc1, bc2s)
    return p2, m2, v2, ema_update_f64(ema, p2, ema_w)


def ema_trajectory(params_per_step, decay):
    """float64 EMA over parameter snapshots: params_per_step[0] the initial weights (where the average starts), params_per_step[t] the
    parameters after optimiser step t = 1, 2, ..."""
    from e4t.optimization import ema_weight
    e = params_per_step[0].to(f64).clone()
    for t, p in enumerate(params_per_step[1:], start=1):
        e = e - ema_weight(decay, t) * (e - p.to(f64))
    return e


def rel_l2(got, want):
    want = want.to(f64)
    return float((got.to(f64) - want).norm() / want.norm().clamp_min(1e-300))


# ---- the emulation with the three ops ---------------------------------------------------------------------------------------------
class EmaEmuBackend(EmuBackend):
    @staticmethod
    def _ema(ema, p, w):
        ema.sub_((ema - p) * w)            # e - w * (e - p), fp32

    def ema_update(self, ema, p, ema_w, w_dev=None):
        self._ema(ema, p, float(w_dev) if w_dev is not None else ema_w)

    def adamw_ema(self, p, g, m, v, ema, lr, beta1, beta2, eps, wd, step, grad_scale=1.0, ema_w=0.0, hyper=None):
        if hyper is not None:
            lr, bc1, bc2s, grad_scale, ema_w = (float(x) for x in hyper.tolist()[:5])
            gg = g * grad_scale
            p.mul_(1 - lr * wd)
            m.mul_(beta1).add_(gg, alpha=1 - beta1)
            v.mul_(beta2).addcmul_(gg, gg, value=1 - beta2)
            p.addcdiv_(m, v.sqrt() / bc2s + eps, value=-lr / bc1)
        else:
            self.adamw(p, g, m, v, lr, beta1, beta2, eps, wd, step, grad_scale)
        self._ema(ema, p, ema_w)

    def adamw_rank_ema(self, p, m, v, ema, G, Z, lr, beta1, beta2, eps, wd, step, grad_scale=1.0, ema_w=0.0, hyper=None):
        if hyper is not None:
            ema_w = float(hyper[4])
            hyper = hyper[:4]
        self.adamw_rank(p, m, v, G, Z, lr, beta1, beta2, eps, wd, step, grad_scale, hyper=hyper)
        self._ema(ema, p, ema_w)

