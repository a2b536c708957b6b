"""CPU: the localised conv comparison of tests/kernel_checks.py (conv_slices()) is neither too tight nor too loose.

Not too tight: a rounding-only model of the kernels — the fp64 conv of the bf16 inputs, rounded to fp32 (the accumulator) and then to bf16 (the
output) — held against the fp64 evaluation stays at or under HALF the GPU check's tolerance (TOL1) on EVERY row conv_slices() emits, for every case
check_conv runs, bare and with the full epilogue.  What the kernels add to that model is the fp32 summation order; the other half is theirs.

Not too loose: two gather errors that the whole-tensor relative L2 of the full-epilogue form cannot see, or sees only diluted, fail their slice."""
import math

import pytest
import torch
import torch.nn.functional as F

import kernel_checks as kc
from kernel_checks import CONV_S1, CONV_S2, CONV_UP2, CONV_S2A

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
DEV = torch.device("cpu")


def conv64(x, w, case, xpad=None):
    """fp64 conv product [B * Hout * Wout, Cout] of a case; xpad (stride 1 only): the zero-padded input [B, Cin, H + 2, W + 2] to use instead"""
    B, Hin, Win, Cin, Cout, mode, Hout, Wout, _, _ = case
    xi = x.to(f64).reshape(B, Hin, Win, Cin).permute(0, 3, 1, 2)
    wk = w.to(f64).reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
    if xpad is not None:
        assert mode == CONV_S1
        y = F.conv2d(xpad, wk)
    elif mode == CONV_S1:
        y = F.conv2d(xi, wk, padding=1)
    elif mode == CONV_S2:
        y = F.conv2d(xi, wk, stride=2, padding=1)
    elif mode == CONV_UP2:
        y = F.conv2d(F.interpolate(xi, scale_factor=2.0, mode="nearest"), wk, padding=1)
    elif mode == CONV_S2A:
        y = F.conv2d(F.pad(xi, (0, 1, 0, 1)), wk, stride=2)
    else:      # CONV_S2T: the zero-stuffed input, then stride 1
        z = torch.zeros(B, Cin, Hout, Wout, dtype=f64)
        z[:, :, ::2, ::2] = xi
        y = F.conv2d(z, wk, padding=1)
    assert y.shape[2:] == (Hout, Wout)
    return y.permute(0, 2, 3, 1).reshape(B * Hout * Wout, Cout)


def full_epilogue(y, case, bias, rb, res):
    return y + bias.to(f64) + rb.to(f64).repeat_interleave(case[6] * case[7], dim=0) + res.to(f64)


def rounded(y):
    return y.to(f32).to(bf16)


def rows_of(case, form, got, ref):
    B, Hout, Wout = case[0], case[6], case[7]
    tag = kc.conv_tag(case) + " " + form
    return [(tag, kc.rel(got, ref), kc.TOL1)] + kc.conv_slices(tag, got, ref, B, Hout, Wout, kc.conv_plan(case, form))


def test_rounding_only_model_stays_under_half_the_tolerance():
    """one test over all cases (the fp64 conv of each is computed once, for both forms); prints the worst row"""
    assert len(set(kc.CONV_ALL_CASES)) == len(kc.CONV_ALL_CASES)
    worst, bad, n = ("", 0.0), [], 0
    for i, case in enumerate(kc.CONV_ALL_CASES):
        x, w, bias, rb, res = kc.conv_inputs(case, 50 + i, DEV)
        y = conv64(x, w, case)
        yf = full_epilogue(y, case, bias, rb, res)
        for form, ref in (("bare", y), ("full", yf)):
            for name, e, tol in rows_of(case, form, rounded(ref), ref):
                n += 1
                assert math.isfinite(e), name
                if e > worst[1]:
                    worst = (name, e)
                if not e <= tol / 2:
                    bad.append((name, e, tol))
    print("rounding-only model: %d rows, worst %.3e (%s)" % (n, worst[1], worst[0]))
    assert n > 2000
    assert not bad, "the rounding-only model is not within half the tolerance:\n" + "\n".join(f"  {nm}: {e:.3e} > {t / 2:.1e}" for nm, e, t in bad)


def _row(rows, label):
    hit = [(n, e, t) for n, e, t in rows if n.endswith(": " + label)]
    assert len(hit) == 1, (label, [n for n, _, _ in rows])
    return hit[0][1]


def _padded(x, case):
    B, Hin, Win, Cin = case[:4]
    return F.pad(x.to(f64).reshape(B, Hin, Win, Cin).permute(0, 3, 1, 2), (1, 1, 1, 1))


# (case, image): one wrong tap at the top-left pixel of that image.  With 4 output channels the planted error is four numbers and its size is the
# draw's: the image is one where the whole-tensor row passes (at 128 channels either image does).
WRONG_TAP_CASES = [((2, 16, 16, 64, 4, CONV_S1, 16, 16, 0, 0), 1), ((2, 6, 256, 64, 128, CONV_S1, 6, 256, 5256, 1), 1)]


@pytest.mark.parametrize("case,image", WRONG_TAP_CASES, ids=[kc.conv_tag(c) for c, _ in WRONG_TAP_CASES])
def test_one_wrong_tap_at_one_corner_passes_the_whole_tensor_and_fails_the_corner_slice(case, image):
    """tap (ky 0, kx 0) of output pixel (0, 0) of one image reads the pixel Win + 1 in front of it in memory (the last row of the image before)
    instead of the zero pad: what a gather that forgets the border mask at that one place does"""
    assert case in kc.CONV_CASES
    B, Hin, Win, Cin = case[:4]
    x, w, bias, rb, res = kc.conv_inputs(case, 50 + kc.CONV_CASES.index(case), DEV)
    ref = conv64(x, w, case)
    xp = _padded(x, case)
    xp[image, :, 0, 0] = x[image * Hin * Win - (Win + 1)].to(f64)
    got = conv64(x, w, case, xpad=xp)
    assert int(((got - ref).abs().sum(1) > 0).sum()) == 1      # one output pixel
    full = rows_of(case, "full", rounded(full_epilogue(got, case, bias, rb, res)), full_epilogue(ref, case, bias, rb, res))
    assert full[0][1] < kc.TOL1                                 # what check_conv had: passes
    assert _row(full, "corners") > kc.TOL1
    bare = rows_of(case, "bare", rounded(got), ref)
    assert _row(bare, "corners") > 2 * kc.TOL1                  # undiluted: twice as visible
    for label in ("bottom row", "right column", "interior", "first image"):
        assert _row(bare, label) <= kc.TOL1 / 2 and _row(full, label) <= kc.TOL1 / 2      # ... and the slices say where it is not


@pytest.mark.parametrize("case", [c for c, _ in WRONG_TAP_CASES], ids=kc.conv_tag)
def test_right_border_reading_the_next_pixel_fails_the_right_column_slice(case):
    """the kx = 2 taps of the right border column read the pixel that follows in memory (the first of the next row) instead of the zero pad"""
    B, Hin, Win, Cin = case[:4]
    x, w, bias, rb, res = kc.conv_inputs(case, 50 + kc.CONV_CASES.index(case), DEV)
    ref = conv64(x, w, case)
    nxt = torch.cat([x[1:], torch.zeros(1, Cin, dtype=x.dtype)]).to(f64).reshape(B, Hin, Win, Cin)
    xp = _padded(x, case)
    xp[:, :, 1:Hin + 1, Win + 1] = nxt[:, :, Win - 1, :].permute(0, 2, 1)
    got = conv64(x, w, case, xpad=xp)
    for form, g, r in (("bare", got, ref), ("full", full_epilogue(got, case, bias, rb, res), full_epilogue(ref, case, bias, rb, res))):
        rows = rows_of(case, form, rounded(g), r)
        assert _row(rows, "right column") > 10 * kc.TOL1, form
        assert _row(rows, "left column") <= kc.TOL1 / 2 and _row(rows, "interior") <= kc.TOL1 / 2, form


def test_conv_slices_regions():
    """the regions on a tensor whose value is its own (image, row, column, channel): labels, empty regions skipped, NaN reported as infinite"""
    class Plan:
        tile_m, tile_n = 64, 64
    B, H, W, C = 3, 5, 4, 72
    ref = torch.randn(B * H * W, C, generator=torch.Generator().manual_seed(1))
    got = ref.clone()
    assert [n.split(": ")[1].split(" (")[0] for n, _, _ in kc.conv_slices("t", got, ref, B, H, W, Plan)] == [
        "top row", "bottom row", "left column", "right column", "corners", "interior", "first image", "last image", "rows 0-59", "columns 64-71"]
    got4 = got.reshape(B, H, W, C)
    got4[1, H - 1, 0, 3] += 1.0      # a bottom-left corner of the middle image
    hit = {n.split(": ")[1].split(" (")[0] for n, e, _ in kc.conv_slices("t", got, ref, B, H, W, Plan) if e > 0}
    assert hit == {"bottom row", "left column", "corners", "rows 0-59"}
    got4[1, H - 1, 0, 3] = float("nan")
    assert {e for n, e, _ in kc.conv_slices("t", got, ref, B, H, W, Plan) if "corners" in n} == {float("inf")}
    # a one-pixel image: one region each, no interior, no duplicate of top row / left column
    names = [n.split(": ")[1] for n, _, _ in kc.conv_slices("t", ref[:3], ref[:3], 3, 1, 1, Plan)]
    assert names[:5] == ["top row", "left column", "corners", "first image", "last image"] and "interior" not in names
