"""CPU: the streaming comparison of tests/kernel_checks.py (stream_ref64_*, stream_slices, the three families streaming_values, streaming_layout,
streaming_guards) is neither too tight nor too loose.

Not too tight: stream_model() below restates every value kernel of csrc/elementwise.hip in fp32 in the kernel's own arithmetic — the Abramowitz &
Stegun erf polynomial in its fmaf order with exp(-x^2 / 2) as exp2 of the rounded product with log2(e) (what __expf is), x / (1 + exp(-x)),
spatial_mean's 64 pixel groups that stride the pixels by 64 and sum in order, then the 64 group sums in order, then the division by HW, softmax's
max, exp(v - max), per-thread chunk order, xor wave tree, four wave sums in order and the reciprocal multiply, the bicubic weights with
w[3] = 1 - w0 - w1 - w2 and fy = oy * sy in fp32, sumsq's grid-stride fma chain and block tree — and returns each output BEFORE its rounding to
bf16.  A row's measure is max |got - ref| / (rel |ref| + floor * scale): rel = 2^-8 is the one bf16 rounding of the output, a property of the format
(so the elementwise bound on a bf16 output is 3.9e-3 |ref| + floor, under check_streaming's whole-tensor TOL1 = 6e-3), and the floor is what is
measured: per class, the model's worst unrounded error against the fp64 definition in units of the scale, doubled and rounded up
(test_floors_are_twice_the_models_worst prints it).  The factor of two is for what the CPU cannot know: its exp2 / sin / cos are not the GPU's
v_exp_f32 / sinf / cosf, and the compiler's choice of fused multiply-adds is not read off the code object here.  With those floors the model, rounded,
passes every row of every case of streaming_values and streaming_layout (test_the_rounded_model_passes_every_row); streaming_guards draws further
inputs of the same kernels inside the GPU check and holds them to the same classes.

MEASURED ON THE CPU (this file: the unrounded model against fp64, worst element per class in units of the scale; 2 x worst, rounded up -> floor):
  gelu    4.99e-7 of |x| / 2 (geglu 300x640 da)  -> 1.0e-6     (the erf's documented 1.5e-7 plus the roundings of 1 + erf, the two products
                                                                and the exp; the issue's 1.5e-7 |x| / 2 alone is less than the arithmetic has)
  dgelu   2.47e-7 of |dy| (op 3, every pattern)   -> 5.0e-7     sigmoid 1.06e-7 of |x|, backward of |dy| (1 + |x|) (op 7)  -> 2.2e-7
  round   7.47e-8 of |y| (op 4: 0.01f is not 0.01) -> 1.5e-7    sum     9.55e-8 of the sum of |terms| (spatial_mean_bwd)   -> 2.0e-7
  softmax 3.23e-6 of p (L 2056)                   -> 6.6e-6     embed   6.28e-5 absolute (dim 322: fp32 angle at 1000 rad)  -> 1.3e-4
  clip    2.34e-5 of 1 / min(std) (512 -> 224)    -> 4.8e-5     mean32  3.76e-8 of mean |x| (mean 100, HW 63)              -> 7.6e-8
  sumsq32 9.68e-8 of the sum (n 255)              -> 2.0e-7
  Every bf16 class: rel + floor <= 3.91e-3 + 1.3e-4 < TOL1 = 6e-3; the fp32 classes 7.6e-8 and 2.0e-7 < TOLF = 2e-5.
MEASURED ON THE MI355X (tests/gpu_report.py: 230 + 248 + 83 rows, none failing; the worst row per class, of 1):
  sigmoid 0.996 (op 1, dy = 1)   gelu 0.996 (geglu 300x640 h)   dgelu 0.995   round 0.996 (add)   sum 0.996 (sumpool2)   softmax 0.986 (L 2056)
  clip 0.968 (512 -> 224)   embed 0.922 (dim 322)   mean32 0.494   sumsq32 0.484.
  The bf16 classes sit just under 1 because rel is the format's exact worst case: among 65536 patterns or 192000 outputs some value lands next
  to a rounding tie and uses the whole half ulp; what the floors are for (small |ref| against the scale: the GELU tails, zero crossings of sin,
  cancelling sums) stayed inside them.  The two fp32 classes show the model's own figure: the GPU's sums are the model's.  No class was widened.
  Guard rows: 0 sentinel words changed and 0 poison words left for every kernel; the three families take 0.3 s, 0.04 s and 0.03 s.

Not too loose: planted errors that the whole-tensor relative L2 of check_streaming passes (TOL1 = 6e-3 for bf16 outputs, TOLF = 2e-5 for fp32 ones)
fail a row, and the right one.

Fixes that went in with these rows (csrc/elementwise.hip):
  * e4t_clip_preprocess formed S % P before it looked at P: P = 0 divided by zero on the host.  It tests P, S, Hin, Win > 0 first now
    (test_streaming_args_cpu.py runs the case), which also closes Hin = 0 (the clamp gave row -1).
  * e4t_spatial_mean / e4t_spatial_mean_bwd refuse coff < 0 and ld < coff + C; _bwd, e4t_sumpool2 and e4t_im2col_T refuse C <= 0; spatial_mean,
    its backward and e4t_transpose refuse batch counts above 65535 by name.
  * unary op 7 (quick-GELU backward) formed 1.702 x, which overflows to infinity for |x| > 2e38, and multiplied it by a sigmoid term that is
    exactly 0 there: inf * 0 = NaN from a finite input, at the 210 bf16 patterns with |x| >= 2.007e38 (counted with the fp32 model of the old
    expression; the row "finite patterns that give a non-finite value" of the every-bit-pattern case holds them to 0).  The product is clamped to
    +-3e38 before the multiply; for every input that gave a finite value before, the bits are unchanged.
The value, layout and guard rows exposed nothing else in the kernels.
Left alone: leaky ReLU backward (op 5) gives 0.01 dy for a NaN x, because `x > 0` is false; that is the definition's answer (and torch's), so the
NaN row of that op asks for what the definition gives.
"""
import math

import pytest
import torch

import kernel_checks as kc

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
LOG2E = torch.tensor(1.4426950408889634, dtype=f32)
LANE = torch.arange(64)


def _fma(a, b, c):
    a, b, c = torch.broadcast_tensors(torch.as_tensor(a, dtype=f32), torch.as_tensor(b, dtype=f32), torch.as_tensor(c, dtype=f32))
    return (a.to(f64) * b.to(f64) + c.to(f64)).to(f32)


def _expf(x):
    """__expf: v_exp_f32 of the rounded product with log2(e)"""
    return torch.exp2(x.float() * LOG2E)


def _wave_tree(v):
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., LANE ^ o]
    return v[..., 0]


def _block_sum(v):
    """block_sum of 256 threads [..., 256]: the wave tree, then the four wave sums in order from 0"""
    w = _wave_tree(v.reshape(*v.shape[:-1], 4, 64))
    t = torch.zeros_like(w[..., 0])
    for i in range(4):
        t = t + w[..., i]
    return t


def _erf_pos(z, e):
    t = 1.0 / _fma(torch.tensor(0.3275911), z, torch.tensor(1.0))
    q = torch.full_like(z, 1.061405429)
    for c in (-1.453152027, 1.421413741, -0.284496736, 0.254829592):
        q = _fma(q, t, torch.tensor(c))
    return _fma(-(q * t), e, torch.tensor(1.0))


def _gelu(x):
    e = _expf((-0.5 * x) * x)
    er = _erf_pos(x.abs() * 0.70710678118654752, e)
    return (0.5 * x) * (1.0 + torch.copysign(er, x))


def _dgelu(x):
    e = _expf((-0.5 * x) * x)
    er = _erf_pos(x.abs() * 0.70710678118654752, e)
    cdf = 0.5 * (1.0 + torch.copysign(er, x))
    return _fma(x * 0.39894228040143268, e, cdf)


def model_unary(op, x, dy):
    x = x.float()
    d = dy.float() if dy is not None else None
    if op == 0:
        return x / (1.0 + _expf(-x))
    if op == 1:
        s = 1.0 / (1.0 + _expf(-x))
        return d * (s * _fma(x, 1.0 - s, torch.tensor(1.0)))
    if op == 2:
        return _gelu(x)
    if op == 3:
        return d * _dgelu(x)
    if op == 4:
        return torch.where(x > 0, x, torch.tensor(0.01, dtype=f32) * x)
    if op == 5:
        return torch.where(x > 0, d, torch.tensor(0.01, dtype=f32) * d)
    k = torch.tensor(1.702, dtype=f32)
    if op == 6:
        return x / (1.0 + _expf(-k * x))
    sg = 1.0 / (1.0 + _expf(-k * x))
    return d * sg * _fma((k * x).clamp(-3.0e38, 3.0e38), 1.0 - sg, torch.tensor(1.0))


def model_spatial_mean(x, B, HW):
    """64 pixel groups, group pg sums pixels pg, pg + 64, ... in order; then the 64 group sums in order; then / HW"""
    C = x.shape[1]
    steps = -(-HW // 64)
    xp = torch.nn.functional.pad(x.float().reshape(B, HW, C), (0, 0, 0, steps * 64 - HW)).reshape(B, steps, 64, C)
    s = torch.zeros(B, 64, C)
    for i in range(steps):
        s = s + xp[:, i]
    t = torch.zeros(B, C)
    for g in range(64):
        t = t + s[:, g]
    return t / torch.tensor(float(HW), dtype=f32)


def model_softmax(x):
    R, L = x.shape
    v = x.float()
    mx = v.max(-1, keepdim=True).values
    e = _expf(v - mx)
    nch = L // 8
    ep = torch.nn.functional.pad(e.reshape(R, nch, 8), (0, 0, 0, 8 * 256 - nch)).reshape(R, 8, 256, 8)      # [row][i][thread][j]
    s = torch.zeros(R, 256)
    for i in range(8):
        for j in range(8):
            s = s + ep[:, i, :, j]
    inv = 1.0 / _block_sum(s)
    return e * inv[:, None]


def model_timestep(t, dim):
    half = dim // 2
    k = torch.arange(half, dtype=f32)
    freq = _expf((torch.tensor(-9.210340371976184, dtype=f32) * k) / torch.tensor(float(half), dtype=f32))
    ang = t.float()[:, None] * freq[None, :]
    return torch.cat([torch.cos(ang.to(f64)), torch.sin(ang.to(f64))], 1).float()      # cosf / sinf: correctly rounded here


def _cubic_w(t):
    A = torch.tensor(-0.75, dtype=f32)
    t1, u = t + 1.0, 1.0 - t
    w0 = ((A * t1 - 5.0 * A) * t1 + 8.0 * A) * t1 - 4.0 * A
    w1 = ((A + 2.0) * t - (A + 3.0)) * t * t + 1.0
    w2 = ((A + 2.0) * u - (A + 3.0)) * u * u + 1.0
    return torch.stack([w0, w1, w2, 1.0 - w0 - w1 - w2], 1)


def model_clip(px, S, P, Kpad, clamp=True, image=False):
    B, _, Hin, Win = px.shape
    x = px.float()

    def taps(n_in):
        sc = torch.tensor(float(n_in - 1), dtype=f32) / torch.tensor(float(S - 1), dtype=f32)
        f = torch.arange(S, dtype=f32) * sc
        i0 = torch.floor(f)
        idx = i0.long()[:, None] + torch.arange(-1, 3)[None, :]
        return _cubic_w(f - i0), (idx.clamp(0, n_in - 1) if clamp else idx % n_in)
    wy, iy = taps(Hin)
    wx, ix = taps(Win)
    g = x[:, :, iy, :][:, :, :, :, ix]                                  # [B][3][S][4 a][S][4 b]
    r = torch.zeros(B, 3, S, 4, S)
    for b in range(4):
        r = _fma(wx[None, None, None, None, :, b], g[..., b], r)
    acc = torch.zeros(B, 3, S, S)
    for a in range(4):
        acc = _fma(wy[None, None, :, a, None], r[:, :, :, a], acc)
    mean, std = torch.tensor(kc.CLIP_MEAN, dtype=f32), torch.tensor(kc.CLIP_STD, dtype=f32)
    img = ((acc + 1.0) * 0.5 - mean[None, :, None, None]) / std[None, :, None, None]
    return img if image else kc.clip_patchify(img, P, Kpad)


def model_sumsq(g, nb):
    """thread (blk, th): s = fma(g_i, g_i, s) over i = blk * 256 + th + k * nb * 256; block_sum; the partials summed in fp64 as the rows do"""
    n = g.numel()
    steps = -(-n // (nb * 256))
    gp = torch.nn.functional.pad(g.float(), (0, steps * nb * 256 - n)).reshape(steps, nb, 256)
    s = torch.zeros(nb, 256)
    for k in range(steps):
        s = _fma(gp[k], gp[k], s)
    return _block_sum(s)


def stream_model(case):
    """{output name: the fp32 value before the output's rounding} of a value case; None for the permutation kernels"""
    a, op = case.a, case.op
    if op == "unary":
        return {"y": model_unary(a["op"], a["x"], a["dy"])}
    if op == "geglu":
        H = a["u"].shape[1] // 2
        A, G, D = a["u"][:, :H].float(), a["u"][:, H:].float(), a["dh"].float()
        return {"h": A * _gelu(G), "da": D * _gelu(G), "dg": D * A * _dgelu(G)}
    if op == "add":
        return {"y": a["a"].float() + a["b"].float()}
    if op == "softmax":
        return {"p": model_softmax(a["x"])}
    if op == "timestep":
        return {"emb": model_timestep(a["t"], a["dim"])}
    if op == "sumsq":
        return {"sum": model_sumsq(a["g"], 1024).sum().reshape(1)}
    if op == "sumpool2":
        B, H, W, C = a["B"], a["H"], a["W"], a["x"].shape[1]
        x = a["x"].float().reshape(B, H, 2, W, 2, C)
        return {"y": (((x[:, :, 0, :, 0] + x[:, :, 0, :, 1]) + x[:, :, 1, :, 0]) + x[:, :, 1, :, 1]).reshape(B * H * W, C)}
    if op == "spatial_mean":
        return {"mean": model_spatial_mean(a["x"], a["B"], a["HW"])}
    if op == "spatial_mean_bwd":
        B, HW, C, coff = a["B"], a["HW"], a["C"], a["coff"]
        inv = 1.0 / torch.tensor(float(HW), dtype=f32)
        gs = a["g"][:, coff:coff + C][:, None, :].expand(B, HW, C).reshape(B * HW, C)
        base = a["base"].float() if a["base"] is not None else torch.zeros(B * HW, C)
        return {"dx": _fma(gs, inv, base)}
    if op == "clip":
        return {"patches": model_clip(a["px"], a["S"], a["P"], a["Kpad"])}
    return None


def _rounded(case, pre):
    ref = kc.stream_ref64(case)
    return {k: (v if kc.STREAM_TOL[ref[k][0]][0] == 0.0 else v.to(bf16)) for k, v in pre.items()}


@pytest.fixture(scope="module")
def model_results():
    """per value case: (case, the model's unrounded outputs), computed once"""
    out = []
    for case in kc.stream_value_cases() + kc.stream_layout_cases():
        pre = stream_model(case)
        if pre is not None:
            out.append((case, pre))
    return out


def test_the_rounded_model_passes_every_row(model_results):
    """the model rounded once to the output type against the fp64 definition: every row of every value case <= 1 (the NaN and overflow rows included)"""
    n, bad = 0, []
    for case, pre in model_results:
        rows = kc.stream_rows(case, _rounded(case, pre))
        n += len(rows)
        bad += [(nm, e, t) for nm, e, t in rows if not (math.isfinite(e) and e <= t)]
    print("model of elementwise.hip against the fp64 definitions: %d rows of %d cases" % (n, len(model_results)))
    assert n > 250
    assert not bad, "the rounded model fails:\n" + "\n".join(f"  {nm}: {e:.3e} > {t:.1e}" for nm, e, t in bad)


def _worst_excess(model_results):
    worst = {}
    for case, pre in model_results:
        for name, (cls, ref, scale, _) in kc.stream_ref64(case).items():
            p = pre[name]
            if case.op == "unary":
                p = p[torch.isfinite(case.a["x"].float())]
            e = kc.stream_excess(p, ref, scale)
            if e > worst.get(cls, (0.0, ""))[0]:
                worst[cls] = (e, f"{case.tag} {name}")
        if case.op == "sumsq":      # the raw-ABI rows: one block that walks the whole buffer
            cls, ref, scale, _ = kc.stream_ref64(case)["sum"]
            e = kc.stream_excess(model_sumsq(case.a["g"], 1).to(f64).sum().reshape(1), ref, scale)
            if e > worst[cls][0]:
                worst[cls] = (e, f"{case.tag} nblocks 1")
    return worst


def test_floors_are_twice_the_models_worst(model_results):
    """prints the model's worst unrounded error per class; each floor is twice it, rounded up by at most a tenth: the model stays at or under half of
    every tolerance.  No bf16 class's elementwise bound exceeds TOL1, no fp32 class's TOLF"""
    worst = _worst_excess(model_results)
    for cls, (rel_, floor) in kc.STREAM_TOL.items():
        e, where = worst[cls]
        print("class %-8s worst %.3e (%s) -> 2 x worst = %.3e, floor %.2e" % (cls, e, where, 2 * e, floor))
    for cls, (rel_, floor) in kc.STREAM_TOL.items():
        e = worst[cls][0]
        assert 2 * e <= floor <= 2.2 * e, (cls, e, floor)
        assert rel_ in (0.0, 2.0 ** -8) and rel_ + floor <= (kc.TOL1 if rel_ else kc.TOLF), cls


def test_every_shape_and_edge_the_kernels_branch_on_has_a_case():
    v, l = kc.stream_value_cases(), kc.stream_layout_cases()
    assert sum(c.op == "unary" for c in v) == 12 and all(c.a["x"].numel() == 65536 for c in v if c.op == "unary")
    assert len({int(b) for b in kc.bf16_patterns().view(torch.int16)}) == 65536
    gate = [c for c in v if c.op == "geglu"][0].a["u"]
    assert gate.shape == (8160, 16) and bool(torch.isfinite(gate.float()).all())
    assert sorted(kc.SOFTMAX_ROWS) == [8, 64, 2056, 16384] and {k for ks in kc.SOFTMAX_ROWS.values() for k in ks} == {"seeded", "peaked", "constant", "offset 3e4", "some -inf"}
    assert (6 * 322 // 2) // 256 != 0 and kc.TIMESTEPS == (0, 1, 17, 500, 999, 1000)
    assert sum(pad for _, _, pad in kc.TRANSPOSE_CASES) == 2
    assert all(H != W for _, _, H, W, _, _ in kc.IM2COL_GEOM[:3]) and {m for m, *_ in kc.IM2COL_GEOM[:3]} == {1, 2, 3}
    assert sum(c.op == "im2col_T" and c.a["x"].shape[1] == 4 for c in l) == 3
    assert sum(c.op == "conv_weight" for c in l) == 12
    assert (3, 65, 132, 200, 60, 0.0) in kc.SPATIAL_MEAN_CASES and (1, 1, 4, 4, 0, 0.0) in kc.SPATIAL_MEAN_CASES
    assert {c[6] for c in kc.CLIP_CASES} >= {588, 640}


# ---- not too loose --------------------------------------------------------------------------------------------------------------------
def _failing(rows):
    return [nm for nm, e, t in rows if not e <= t]


def _case(cases, start):
    return [c for c in cases if c.tag.startswith(start)][0]


def test_a_gelu_tail_zeroed_or_mirrored_fails_the_tail_row_only():
    x = torch.randn(64, 1280, generator=torch.Generator().manual_seed(5)).to(bf16)      # check_streaming's draw: randn
    ref = kc.stream_ref64_unary(2, x)
    for plant in ("zeroed", "mirrored"):
        got = ref.clone()
        got[x.float() < -3] = 0.0 if plant == "zeroed" else -ref[x.float() < -3]
        assert kc.rel(got.to(bf16), ref) < kc.TOL1                     # the whole-tensor bound passes it on a randn draw
    case = _case(kc.stream_value_cases(), "unary op2")
    cls, ref, scale, reg = kc.stream_ref64(case)["y"]
    xf = case.a["x"].float()[torch.isfinite(case.a["x"].float())]
    for plant in ("zeroed", "mirrored"):
        got = ref.clone()
        got[xf < -3] = 0.0 if plant == "zeroed" else -ref[xf < -3]
        bad = _failing(kc.stream_slices("t", got.to(bf16), ref, cls, scale, reg))
        assert any("x < -4" in nm for nm in bad) and any("|x| <= 4" in nm for nm in bad) and not any("x > 4" in nm for nm in bad), bad


def test_one_wrong_row_or_column_chunk_fails_its_row():
    case = _case(kc.stream_value_cases(), "geglu 300x640")
    cls, ref, scale, reg = kc.stream_ref64(case)["h"]
    got = ref.clone()
    got[-1] *= 1.05
    assert kc.rel(got.to(bf16), ref) < kc.TOL1
    bad = _failing(kc.stream_slices("t", got.to(bf16), ref, cls, scale, reg))
    assert any("last row" in nm for nm in bad) and not any("first row" in nm for nm in bad)
    got = ref.clone()
    got[:, :8] *= 1.03
    assert kc.rel(got.to(bf16), ref) < kc.TOL1
    bad = _failing(kc.stream_slices("t", got.to(bf16), ref, cls, scale, reg))
    assert any("first 8 columns" in nm for nm in bad) and not any("last 8 columns" in nm for nm in bad)


def test_h_and_w_swapped_in_im2col_fails_on_the_non_square_case():
    sq = _case(kc.stream_layout_cases(), "im2col mode1 B2 12x12")
    a = sq.a
    assert bool((kc.stream_ref_im2col(a["x"], a["B"], a["Win"], a["Hin"], a["Wout"], a["Hout"], a["mode"]) == kc.stream_ref64(sq)["y"][1]).all())      # square: unseen
    ns = _case(kc.stream_layout_cases(), "im2col mode1 B2 6x10")
    a = ns.a
    got = kc.stream_ref_im2col(a["x"], a["B"], a["Win"], a["Hin"], a["Wout"], a["Hout"], a["mode"])
    assert _failing(kc.stream_rows(ns, {"y": got}))


def test_a_dgrad_tap_not_mirrored_fails():
    case = _case(kc.stream_layout_cases(), "conv_weight_prepare 200->72 pads 256/128 both")
    f, d = kc.stream_ref_conv_weight(case.a["w"], 256, 128)
    wrong = d.reshape(200, 9, 128).flip(1).reshape(200, 9 * 128)
    bad = _failing(kc.stream_rows(case, {"fwd": f, "dgrad": wrong}))      # (the last 8 columns are pad: zero either way)
    assert len(bad) == 4 and all(" dgrad: " in nm for nm in bad) and any("whole" in nm for nm in bad) and any("first 8 columns" in nm for nm in bad)
    assert kc.rel(wrong[:, 4 * 128:5 * 128], d[:, 4 * 128:5 * 128]) == 0.0      # the centre tap is its own mirror


def test_a_spatial_mean_slab_tail_dropped_fails_the_last_slab():
    """B2 HW63 C68, mean 100: the partial slab (channels 64-67) without its last pixel, that pixel a thousandth of the others there (3.9e-6 on the
    whole tensor, under TOLF); and one channel of one image off by 1e-4"""
    case = _case(kc.stream_layout_cases(), "spatial_mean B2 HW63 C68 ldo68 coff0 mean 100")
    cls, _, _, reg = kc.stream_ref64(case)["mean"]
    x = case.a["x"].to(f64).reshape(2, 63, 68).clone()
    x[:, 62, 64:] *= 1e-3
    ref, scale = x.mean(1), x.abs().mean(1)
    got = ref.clone()
    got[:, 64:] = x[:, :62, 64:].sum(1) / 63
    print("spatial_mean without the last pixel of its partial slab: whole %.3e" % kc.rel(got.float(), ref))
    assert kc.rel(got.float(), ref) < kc.TOLF
    bad = _failing(kc.stream_slices("t", got.float(), ref, cls, scale, reg))
    assert any("channels 64-67" in nm for nm in bad) and not any("channels 0-63" in nm for nm in bad)
    got = ref.clone()
    got[1, 66] *= 1 + 1e-4
    assert kc.rel(got.float(), ref) < kc.TOLF
    bad = _failing(kc.stream_slices("t", got.float(), ref, cls, scale, reg))
    assert any("channels 64-67" in nm for nm in bad) and any("image 1" in nm for nm in bad) and not any("image 0" in nm for nm in bad)


def test_a_softmax_row_normalised_by_the_wrong_sum_fails_that_row():
    case = _case(kc.stream_value_cases(), "softmax_rows L2056")
    cls, ref, scale, reg = kc.stream_ref64(case)["p"]
    got = ref.clone()
    got[2] *= 1.02      # of three rows; the peaked row carries most of the norm
    assert kc.rel(got.to(bf16), ref) < kc.TOL1
    bad = _failing(kc.stream_slices("t", got.to(bf16), ref, cls, scale, reg))
    assert any("row 2" in nm for nm in bad) and not any("row 0" in nm or "row 1" in nm for nm in bad)


def test_the_sin_half_shifted_by_one_frequency_fails_the_sin_half():
    case = _case(kc.stream_value_cases(), "timestep_embedding dim1280")
    cls, ref, scale, reg = kc.stream_ref64(case)["emb"]
    got = ref.clone()
    got[:, 640:] = torch.sin(case.a["t"].to(f64)[:, None] * torch.pow(torch.tensor(10000.0, dtype=f64), -(torch.arange(640, dtype=f64) + 1) / 640)[None, :])
    bad = _failing(kc.stream_slices("t", got.to(bf16), ref, cls, scale, reg))
    assert any("sin half" in nm for nm in bad) and not any("cos half" in nm or "t = 0" in nm for nm in bad)
    got = ref.clone()
    got[:, 1278:] = got[:, 1277:1279]                # the last two sine columns shifted: 2 of 1280 columns
    assert kc.rel(got.to(bf16)[1:], ref[1:]) < kc.TOL1
    assert any("sin half" in nm for nm in _failing(kc.stream_slices("t", got.to(bf16), ref, cls, scale, reg)))


def test_a_clip_border_row_without_the_clamp_fails_the_border_ring():
    """align-corners keeps the window inside the image except where the source is at most about as large as the output: at 20x20 -> 28 output row 1
    reads source row -1 and row 26 source row 20 (at 512 -> 224 only weights that are 0 fall outside).  One such row of one channel of one image
    with the index wrapped instead of clamped"""
    case = _case(kc.stream_layout_cases(), "clip_preprocess enlarging 20x20->28")
    a = case.a
    cls, ref, scale, reg = kc.stream_ref64(case)["patches"]
    img = model_clip(a["px"], a["S"], a["P"], a["Kpad"], image=True)
    assert not _failing(kc.stream_slices("t", kc.clip_patchify(img, a["P"], a["Kpad"]).to(bf16), ref, cls, scale, reg))
    wrong = model_clip(a["px"], a["S"], a["P"], a["Kpad"], clamp=False, image=True)
    assert bool((wrong[:, :, 2:26, 2:26] == img[:, :, 2:26, 2:26]).all()) and not bool((wrong[1, 2, 1] == img[1, 2, 1]).all())
    img[1, 2, 1, 14:] = wrong[1, 2, 1, 14:]
    got = kc.clip_patchify(img, a["P"], a["Kpad"]).to(bf16)
    print("half a border row of clip_preprocess without the clamp: whole %.3e" % kc.rel(got, ref))
    assert kc.rel(got, ref) < kc.TOL1
    bad = _failing(kc.stream_slices("t", got, ref, cls, scale, reg))
    assert any("border ring" in nm for nm in bad) and not any("interior" in nm or "pad columns" in nm for nm in bad)


def test_stream_slices_counts_inf_nan_and_overflow():
    ref = torch.tensor([1.0, 2.0, 4e38, float("nan")], dtype=f64)
    ok = torch.tensor([1.0, 2.0, float("inf"), float("nan")]).to(bf16)
    assert kc.stream_slices("t", ok, ref, "round", ref.abs(), [])[0][1] == 0.0
    for bad in ([1.0, float("inf"), float("inf"), float("nan")], [float("nan"), 2.0, float("inf"), float("nan")], [1.0, 2.0, float("-inf"), float("nan")], [1.0, 2.0, float("inf"), 0.0]):
        assert kc.stream_slices("t", torch.tensor(bad).to(bf16), ref, "round", ref.abs(), [])[0][1] == float("inf")
    assert kc.stream_slices("t", torch.tensor([1.0, 2.5]).to(bf16), torch.tensor([1.0, 2.0]).to(bf16), "exact")[0][1:] == (1.0, 0.0)
