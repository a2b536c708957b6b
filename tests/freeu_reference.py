"""TEST-ONLY: FreeU's definition in float64, in plain torch, and the two freeu ops added to the op emulation.  The definition is the
specification the HIP kernels of csrc/freeu.hip are held to (include/e4t_hip.h, e4t/freeu.py):

  backbone  h' = h * ((b - 1) m^ + 1) on the first C_h / 2 channels, the rest unchanged
            version 1: m^ = 1.  version 2: m = the mean over all C_h channels, m^ = (m - min) / (max - min) per image over its H W values,
            m^ = 0 where max == min
  skip      k' = k + (s - 1) LP(k) per image and channel,
            X[ky,kx]   = sum_{y,x} k[y,x] exp(-2 pi i (ky y / H + kx x / W)),      ky, kx in {0, -1}
            LP(k)[y,x] = (1 / HW) Re sum_{ky,kx in {0,-1}} X[ky,kx] exp(+2 pi i (ky y / H + kx x / W))

`skip_closed` is that closed form; `skip_fft` is the usual recipe (fftn -> fftshift -> scale the centre box of threshold 1 -> ifftshift ->
ifftn -> real), written independently with torch.fft.  Maps are NCHW here; `to_nchw` / `to_rows` convert from / to the kernels' NHWC matrices.

The product never imports this file."""
from __future__ import annotations

import math

import torch

from emu_backend import EmuBackend

f64 = torch.float64
COEFS, MM_CHUNKS = 7, 64


def to_nchw(x2d, B, H, W):
    return x2d.reshape(B, H, W, x2d.shape[1]).permute(0, 3, 1, 2)


def to_rows(x4d):
    B, C, H, W = x4d.shape
    return x4d.permute(0, 2, 3, 1).reshape(B * H * W, C)


def _phases(H, W, device=None):
    ty = 2.0 * math.pi * torch.arange(H, dtype=f64, device=device) / H
    px = 2.0 * math.pi * torch.arange(W, dtype=f64, device=device) / W
    return ty[:, None], px[None, :]


def coefficients(k):
    """k [B, C, H, W] -> float64 [B, 7, C]: X[0,0], Re / Im X[-1,0], Re / Im X[0,-1], Re / Im X[-1,-1]"""
    k = k.to(f64)
    ty, px = _phases(k.shape[2], k.shape[3], k.device)
    basis = [torch.ones_like(ty + px), torch.cos(ty) + 0 * px, torch.sin(ty) + 0 * px, torch.cos(px) + 0 * ty, torch.sin(px) + 0 * ty,
             torch.cos(ty + px), torch.sin(ty + px)]            # exp(-2 pi i (-1) y / H) = cos + i sin of +theta_y
    return torch.stack([(k * b).sum(dim=(2, 3)) for b in basis], dim=1)


def lowpass_closed(k):
    """LP(k) of the definition, float64"""
    k = k.to(f64)
    H, W = k.shape[2], k.shape[3]
    ty, px = _phases(H, W, k.device)
    X = coefficients(k)[..., None, None]                       # [B, 7, C, 1, 1]
    lp = X[:, 0] + X[:, 1] * torch.cos(ty) + X[:, 2] * torch.sin(ty) + X[:, 3] * torch.cos(px) + X[:, 4] * torch.sin(px) \
        + X[:, 5] * torch.cos(ty + px) + X[:, 6] * torch.sin(ty + px)          # Re((A + iB)(cos - i sin)) = A cos + B sin
    return lp / (H * W)


def skip_closed(k, s):
    k = k.to(f64)
    return k + (s - 1.0) * lowpass_closed(k)


def skip_fft(k, s, threshold=1):
    """the usual recipe, float64"""
    k = k.to(f64)
    H, W = k.shape[2], k.shape[3]
    f = torch.fft.fftshift(torch.fft.fftn(k, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones(k.shape, dtype=f64, device=k.device)
    cr, cc = H // 2, W // 2
    mask[..., cr - threshold:cr + threshold, cc - threshold:cc + threshold] = s
    return torch.fft.ifftn(torch.fft.ifftshift(f * mask, dim=(-2, -1)), dim=(-2, -1)).real


def mhat(h):
    """h [B, C, H, W] -> float64 [B, 1, H, W], 0 where the image's channel mean is constant"""
    m = h.to(f64).mean(dim=1, keepdim=True)
    mn = m.amin(dim=(2, 3), keepdim=True)
    mx = m.amax(dim=(2, 3), keepdim=True)
    rng = mx - mn
    return torch.where(rng > 0, (m - mn) / torch.where(rng > 0, rng, torch.ones_like(rng)), torch.zeros_like(m))


def backbone(h, b, version=2):
    h = h.to(f64)
    half = h.shape[1] // 2
    scale = torch.full_like(h[:, :1], float(b)) if version == 1 else (b - 1.0) * mhat(h) + 1.0
    out = h.clone()
    out[:, :half] = h[:, :half] * scale
    return out


def freeu_pair(h, k, b, s, version=2):
    """(h', k') of the definition for NCHW h, k: float64"""
    return backbone(h, b, version), skip_closed(k, s)


class FreeuEmuBackend(EmuBackend):
    """the op emulation with the two FreeU ops (signatures of e4t.ops.HipBackend; the workspace has e4t_freeu_stats' layout)"""

    def freeu_stats(self, h, k, B, H, W, version=2, ws=None):
        HW, Ch, Ck = H * W, h.shape[1], k.shape[1]
        if Ch % 16 or Ck % 8 or H < 2 or W < 2:
            raise ValueError(f"freeu_stats: unsupported shape C_h={Ch} C_k={Ck} {H}x{W}")
        coef = coefficients(to_nchw(k, B, H, W))
        msum = to_nchw(h, B, H, W).to(f64).sum(dim=1).reshape(B, HW)
        mm = torch.full((B, MM_CHUNKS, 2), float("inf"), dtype=f64, device=h.device)
        mm[:, :, 1] = -float("inf")
        mm[:, 0, 0], mm[:, 0, 1] = msum.amin(dim=1), msum.amax(dim=1)
        return torch.cat([coef.reshape(-1), msum.reshape(-1), mm.reshape(-1)]).float()

    def freeu_apply(self, h, k, ws, B, H, W, b, s, version=2, out_h=None, out_k=None):
        HW, Ch, Ck = H * W, h.shape[1], k.shape[1]
        n0 = B * COEFS * Ck
        X = ws[:n0].view(B, COEFS, Ck).to(f64)[..., None, None]
        msum = ws[n0:n0 + B * HW].view(B, 1, H, W).to(f64)
        mm = ws[n0 + B * HW:n0 + B * HW + B * MM_CHUNKS * 2].view(B, MM_CHUNKS, 2).to(f64)
        mn, mx = mm[:, :, 0].amin(dim=1).view(B, 1, 1, 1), mm[:, :, 1].amax(dim=1).view(B, 1, 1, 1)
        rng = mx - mn
        mh = torch.where(rng > 0, (msum - mn) / torch.where(rng > 0, rng, torch.ones_like(rng)), torch.zeros_like(msum))
        hh = to_nchw(h, B, H, W).to(f64)
        scale = torch.full_like(mh, float(b)) if version == 1 else (b - 1.0) * mh + 1.0
        h2 = hh.clone()
        h2[:, :Ch // 2] = hh[:, :Ch // 2] * scale
        ty, px = _phases(H, W, k.device)
        lp = (X[:, 0] + X[:, 1] * torch.cos(ty) + X[:, 2] * torch.sin(ty) + X[:, 3] * torch.cos(px) + X[:, 4] * torch.sin(px)
              + X[:, 5] * torch.cos(ty + px) + X[:, 6] * torch.sin(ty + px)) / HW
        k2 = to_nchw(k, B, H, W).to(f64) + (s - 1.0) * lp
        return self._act(to_rows(h2).float()), self._act(to_rows(k2).float())
