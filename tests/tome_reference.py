"""TEST-ONLY: the token-merging algorithm (ToMe around attn1, 2x2 cells) restated in plain torch, and the three tome ops added to
the op emulation.  The restatement is the specification the HIP kernels of csrc/tome.hip are held to:

  split   one dst token per 2x2 cell (choice[cell] = cy*2+cx, none = top-left), nd = T/4; the other ns = 3T/4 are src tokens,
          numbered in ascending token order
  match   x^ = bf16(x / ||x||_2), the norm from the exact sum of squares, the division in fp32; score = x^_src . x^_dst; node_max /
          node_idx = max / argmax over the dst (ties: lowest index); the r src with the largest node_max (ties: lower src position) merge
  plan    map [B][T], row_tok [B][T'], seg_off [B][nd+1], seg_src [B][r] (include/e4t_hip.h)
  merge   row j < nd = (x[dst j] + x[seg_src of j, in order]) (/ count); the other rows copy x[row_tok]
  unmerge out[i] = (residual[i] +) y[map[i]] (/ count[map[i]])

The product never imports this file."""
from __future__ import annotations

import torch

from emu_backend import EmuBackend

bf16, f32 = torch.bfloat16, torch.float32


def split_tokens(h, w, choice=None):
    """-> (dst_tok [nd], src_tok [ns]) int64, src ascending"""
    hs, ws = h // 2, w // 2
    ch = torch.zeros(hs * ws, dtype=torch.int64) if choice is None else choice.to("cpu", torch.int64) & 3
    cell = torch.arange(hs * ws)
    dst = (2 * (cell // ws) + (ch >> 1)) * w + 2 * (cell % ws) + (ch & 1)
    is_dst = torch.zeros(h * w, dtype=torch.bool)
    is_dst[dst] = True
    src = torch.nonzero(~is_dst).reshape(-1)
    return dst, src


def xhat(x):
    """x: [B, T, d].  bf16 input: exactly the kernel's bf16(x / ||x||); other dtypes (the fp32 emulation): plain normalisation."""
    if x.dtype != bf16:
        xf = x.float()
        return xf / xf.norm(dim=-1, keepdim=True)
    xf = x.float()
    nrm = (xf.double() ** 2).sum(-1, keepdim=True).float().sqrt()     # squares of bf16 are exact, their fp64 sum is order-free
    return (xf / nrm).to(bf16)


def scores(x, h, w, choice=None, dtype=f32):
    """[B, ns, nd] scores of the restatement, accumulated in `dtype`"""
    dst, src = split_tokens(h, w, choice)
    xh = xhat(x).to(dtype)
    return xh[:, src.to(x.device)] @ xh[:, dst.to(x.device)].transpose(1, 2)


def plan_from_nodes(node_max, node_idx, h, w, r, choice=None):
    """top-r selection and the plan's four arrays from [B, ns] node_max / node_idx -> dict of int32 CPU tensors"""
    node_max, node_idx = node_max.cpu(), node_idx.cpu().to(torch.int64)
    B, ns = node_max.shape
    T, nd = h * w, (h * w) // 4
    dst, src = split_tokens(h, w, choice)
    Tm = T - r
    out = dict(map=torch.empty(B, T, dtype=torch.int64), row_tok=torch.empty(B, Tm, dtype=torch.int64),
               seg_off=torch.empty(B, nd + 1, dtype=torch.int64), seg_src=torch.empty(B, r, dtype=torch.int64))
    for b in range(B):
        order = torch.sort(node_max[b], descending=True, stable=True).indices       # ties: ascending src position
        merged = torch.zeros(ns, dtype=torch.bool)
        merged[order[:r]] = True
        mi = torch.nonzero(merged).reshape(-1)
        mj = node_idx[b, mi]
        o2 = torch.sort(mj * ns + mi).indices                                        # by (dst, src position)
        out["seg_src"][b] = src[mi[o2]]
        out["seg_off"][b] = torch.cat([torch.zeros(1, dtype=torch.int64), torch.bincount(mj, minlength=nd).cumsum(0)])
        un = torch.nonzero(~merged).reshape(-1)
        out["map"][b, dst] = torch.arange(nd)
        out["map"][b, src[mi]] = mj
        out["map"][b, src[un]] = nd + torch.arange(un.numel())
        out["row_tok"][b, :nd] = dst
        out["row_tok"][b, nd:] = src[un]
    return {k: v.to(torch.int32) for k, v in out.items()}


def match_plan(x, h, w, r, choice=None, dtype=f32):
    """the restatement's plan for x [B, T, d]"""
    s = scores(x, h, w, choice, dtype)
    node_max = s.max(-1).values
    node_idx = (s == node_max[..., None]).to(torch.int32).argmax(-1)                 # the first maximal index
    return plan_from_nodes(node_max.float(), node_idx, h, w, r, choice)


def counts(plan):
    """[B, T'] token count of every merged row"""
    c = torch.ones(plan.B, plan.Tm, dtype=torch.int64, device=plan.buf.device)
    so = plan.seg_off.to(torch.int64)
    c[:, :plan.nd] += so[:, 1:] - so[:, :-1]
    return c


def merge(x, plan, mean=True):
    """x [B, T, d] -> fp32 [B, T', d], accumulated in the kernel's order: the dst token, then its segment of seg_src"""
    B, nd, dev = plan.B, plan.nd, x.device
    xf = x.float()
    row_tok, so, ss = plan.row_tok.to(dev, torch.int64), plan.seg_off.to(dev, torch.int64), plan.seg_src.to(dev, torch.int64)
    bi = torch.arange(B, device=dev)[:, None]
    y = xf[bi, row_tok]
    ln = so[:, 1:] - so[:, :-1]
    acc = y[:, :nd].clone()
    for k in range(int(ln.max()) if ln.numel() else 0):
        sel = ln > k
        tok = ss[bi.expand_as(sel)[sel], (so[:, :-1] + k)[sel]]
        acc[sel] = acc[sel] + xf[bi.expand_as(sel)[sel], tok]
    if mean:
        acc = torch.where((ln > 0)[..., None], acc / (1 + ln)[..., None].float(), acc)
    y[:, :nd] = acc
    return y


def unmerge(y, plan, residual=None, scale=False):
    """y [B, T', d] -> fp32 [B, T, d] in the kernel's operation order (division, then the residual add)"""
    dev = y.device
    mp = plan.map.to(dev, torch.int64)
    bi = torch.arange(plan.B, device=dev)[:, None]
    o = y.float()[bi, mp]
    if scale:
        o = o / counts(plan).to(dev)[bi, mp][..., None].float()
    if residual is not None:
        o = residual.float() + o
    return o


class TomeEmuBackend(EmuBackend):
    """the op emulation with the three token-merging ops (signatures of e4t.ops.HipBackend)"""

    def tome_match(self, x, B, h, w, r, choice=None, out=None):
        from e4t.ops import TomePlan
        p = match_plan(x.reshape(B, h * w, -1), h, w, r, choice)
        return TomePlan.from_fields(**p).to(x.device)

    def tome_merge(self, x, plan, mean=True):
        d = x.shape[1]
        return self._act(merge(x.reshape(plan.B, plan.T, d), plan, mean).reshape(plan.B * plan.Tm, d))

    def tome_unmerge(self, y, plan, residual=None, scale=False):
        d = y.shape[1]
        res = None if residual is None else residual.reshape(plan.B, plan.T, d)
        return self._act(unmerge(y.reshape(plan.B, plan.Tm, d), plan, res, scale).reshape(plan.B * plan.T, d))
