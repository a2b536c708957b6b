"""float64 restatement of the guidance contract in include/e4t_hip.h (e4t_guidance_stats, e4t_sampler_step_guided)
on the kernels' fp32 inputs: what tests/test_guidance_gpu.py holds the kernels against.  Not a test module."""
import torch

PAIRS = [(0.0, 1.0), (3.0, 0.05), (-2.0, 4.0), (10.0, 0.01)]      # (mean, sd) of an image's model outputs; image b of case s takes PAIRS[(s + b) % 4]


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def draw(shape, branches, nhwc, gen, device, first_pair=0):
    """pred = [u | (k |) c]: every branch an independent draw, image b with PAIRS[(first_pair + b) % 4]; in the given layout"""
    B, C, H, W = shape
    z = torch.randn((branches, B, C, H, W), generator=gen, device=device)
    mean = torch.tensor([PAIRS[(first_pair + b) % 4][0] for b in range(B)], device=device).view(1, B, 1, 1, 1)
    sd = torch.tensor([PAIRS[(first_pair + b) % 4][1] for b in range(B)], device=device).view(1, B, 1, 1, 1)
    pred = (mean + sd * z).reshape(branches * B, C, H, W)
    return pred.permute(0, 2, 3, 1).contiguous() if nhwc else pred.contiguous()


def split(pred, shape, branches, nhwc):
    """pred in its layout -> the branches as float64 [B, C, H, W]"""
    B, C, H, W = shape
    p = pred.double()
    if nhwc:
        p = p.reshape(-1, H * W, C).permute(0, 2, 1)
    return p.reshape(branches, B, C, H, W).unbind(0)


def guided(pred, gp, shape, branches, nhwc):
    """e0 and c"""
    g, g_id = (float(v) for v in gp[:2].double())
    br = split(pred, shape, branches, nhwc)
    if branches == 2:
        u, c = br
        return u + g * (c - u), c
    u, k, c = br
    return u + g * (k - u) + g_id * (c - k), c


def stats(pred, gp, shape, branches, nhwc):
    """gstat: float64 [B, 4] = {f, s_c, s_e, mean_e}"""
    phi = float(gp[2].double())
    e0, c = guided(pred, gp, shape, branches, nhwc)
    B = shape[0]
    s_e, s_c, mean_e = e0.reshape(B, -1).std(dim=1), c.reshape(B, -1).std(dim=1), e0.reshape(B, -1).mean(dim=1)
    ratio = s_c / s_e
    f = torch.where((s_e == 0) | ~torch.isfinite(ratio), torch.ones_like(ratio), (1.0 - phi) + phi * ratio)
    return torch.stack([f, s_c, s_e, mean_e], dim=1)


def step(pred, x, row, gp, gstat, hist, saved, noise, branches, nhwc, edit=None):
    """e4t_sampler_step_guided: gstat = None or anything whose [:, 0] is the per-image factor -> (out, m, x_in), float64"""
    r = row.double().tolist()
    _, a_e, a_x, c_x, c_s, c_m, c_n, k_in = r[:8]
    shape = tuple(x.shape)
    B, C, H, W = shape
    e, _ = guided(pred, gp, shape, branches, nhwc)
    if gstat is not None:
        e = gstat[:, 0].double().view(B, 1, 1, 1) * e
    xd = x.double()
    m = a_e * e + a_x * xd
    out = c_x * xd + c_m * m
    if saved is not None:
        out = out + c_s * saved.double()
    if hist is not None:
        for k in range(hist.shape[0]):
            out = out + r[10 + k] * hist[k].double()
    if noise is not None:
        out = out + c_n * noise.double()
    if edit is not None:
        keep, x0, n0 = edit
        kp = keep.double().reshape(-1, 1, H, W)
        y = r[15] * n0.double() + r[14] * x0.double().reshape(-1, C, H, W)
        out = kp * y + (1 - kp) * out
    return out, m, k_in * out
