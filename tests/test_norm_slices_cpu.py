"""CPU: the localised norm comparison of tests/kernel_checks.py (norm_slices(), gn_stat_rows(), colblock_rows()) is neither too tight nor too loose.

Not too tight: a rounding-only model of the kernels — the fp64 result rounded to fp32 and then to the stored dtype — held against the fp64 reference
stays at or under HALF the GPU check's tolerance on every row emitted for every case of GN_CASES and LN_CASES.  What the kernels add to that model
is their fp32 arithmetic and summation order; the other half is theirs.

The statistics tolerance (kc.STAT_TOL) is derived here: the model of the kernels' statistics is one fp32 accumulation chain per chunk (chunked
kernels) or per slab thread (slab kernels), fp64 across chunks / threads, E[x^2] - mean^2 and 1 / sqrt in fp64, then the fp32 store.  Measured
(test_statistics_tolerance prints it): worst |d rstd| / rstd 1.05e-6 (B2 HW256 C1280+1280: chains of 640 values, the second source at twice
the scale), worst |d mean| * rstd 1.5e-8 on the cases without a shift — and 6.0e-6 for |d mean| * rstd on the two shifted-mean cases, which is
nothing but the fp32 store of a mean of 64 (up to half an ulp, 3.8e-6) at rstd 1.9.  4 x 6.0e-6 = 2.4e-5 exceeds the cap, so STAT_TOL is the
cap, 1e-5 (without the shifted cases it would be 4.2e-6), and the shifted-mean mean rows have no factor of two to spare: a kernel that finalises
in fp64 stores the correctly rounded mean, i.e. exactly the model's value, and that row is held to half an fp32 ulp of the mean times rstd
(7.3e-6) instead of to half the tolerance.  Every other statistics row of the model is under a ninth of the tolerance.

Not too loose: planted errors that the whole-tensor relative L2 passes fail their slice; the statistics model finalised in fp32, or with the
element count's reciprocal rounded to fp32 (what norm.hip did before this test existed), fails the statistics row on the shifted-mean inputs."""
import math

import numpy as np
import pytest
import torch

import kernel_checks as kc

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
DEV = torch.device("cpu")


def rounded(t, dtype=bf16):
    return t.to(f32).to(dtype)


def _chain_sums(v):
    """v: float32 [chains, steps] -> (sum, sum of squares) per chain, accumulated in fp32 in step order"""
    s, q = np.zeros(v.shape[0], np.float32), np.zeros(v.shape[0], np.float32)
    for t in range(v.shape[1]):
        x = v[:, t]
        s = s + x
        q = q + x * x
    return s, q


def stats_model(x1, x2, case, final=f64, inv_n_f32=False, cols=False, centred=True):
    """(mean, rstd) [B, G, 2] as fp32, from the model of the kernels' statistics on the path norm_plan gives the case's forward:
    one fp32 chain per (batch, chunk, group) or per slab thread, summed across in fp64.  final=f32: the finalisation E[x^2] - mean^2, 1 / sqrt in
    fp32 instead; inv_n_f32: 1 / n rounded to fp32 before it meets the fp64 sums; cols: the column-statistics path of a chunked case instead
    (gn_stats_cols_kernel: min(ch, HW / 32) chunks of whole 32-pixel blocks; centred=False: with the raw sum of squares in its fp32 partial)."""
    c, pl = case, kc.norm_plan(case)
    B, HW, G, C = c.B, c.HW, c.G, c.C1 + c.C2
    cpg = C // G
    x = (x1.float() if x2 is None else torch.cat([x1.float(), x2.float()], dim=-1)).reshape(B, HW, G, cpg)
    if cols:      # column statistics: one fp32 chain per (32-pixel block, channel), as the producing epilogue leaves them; the kernel sums
        assert not pl["ni"] and pl["colstats"]      # them per (chunk, group) in fp64 and stores (s, M2 = q - s^2 / n_c) in fp32
        npart = min(pl["ch"], HW // 32)
        s, q = _chain_sums(x.reshape(B, HW // 32, 32, C).permute(0, 1, 3, 2).reshape(-1, 32).numpy())
        tot = lambda t: torch.from_numpy(t).to(f64).reshape(B, npart, HW // 32 // npart, G, cpg).sum(dim=(2, 4))      # [B, npart, G]
        nc = float(HW // npart * cpg)
        sf = tot(s).to(f32).to(f64)
        m2 = (tot(q) - sf * sf / nc).to(f32 if centred else f64)
        S = sf.sum(1).reshape(B * G)
        Q = ((m2.to(f64) + sf * sf / nc) if centred else tot(q).to(f32).to(f64)).sum(1).reshape(B * G)
        chains = None
    elif pl["ni"]:      # thread t of 256 owns the quads t, t + 256, ... of the slab's [HW][cpg / 4] items
        items, ni = HW * (cpg // 4), pl["ni"]
        it = x.permute(0, 2, 1, 3).reshape(B * G, items, 4)
        it = torch.cat([it, torch.zeros(B * G, ni * 256 - items, 4)], dim=1).reshape(B * G, ni, 256, 4)
        chains = it.permute(0, 2, 1, 3).reshape(B * G * 256, ni * 4)
        per = 256
    else:             # one chain per chunk of ppc pixels
        ch, ppc = pl["ch"], pl["ppc"]
        xp = torch.cat([x, torch.zeros(B, ch * ppc - HW, G, cpg)], dim=1).reshape(B, ch, ppc, G, cpg)
        chains = xp.permute(0, 3, 1, 2, 4).reshape(B * G * ch, ppc * cpg)
        per = ch
    if chains is not None:
        s, q = _chain_sums(chains.numpy())
        S = torch.from_numpy(s).to(f64).reshape(B * G, per).sum(1)
        Q = torch.from_numpy(q).to(f64).reshape(B * G, per).sum(1)
    n = float(cpg * HW)
    inv = torch.tensor(1.0 / n, dtype=f32 if inv_n_f32 else f64).to(f64)
    if final == f32:
        S, Q, inv = S.to(f32), Q.to(f32), inv.to(f32)
    mean = S * inv
    var = torch.clamp(Q * inv - mean * mean, min=0.0)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(c.eps, dtype=f32).to(final))
    return torch.stack([mean, rstd], dim=-1).to(f32).reshape(B, G, 2)


@pytest.fixture(scope="module")
def gn_refs():
    """per GroupNorm case: inputs, the fp64 forward, the model statistics — computed once, shared, left unchanged"""
    refs = {}
    for c in kc.GN_CASES:
        x1, x2, gamma, beta, dy, a1, a2 = kc.gn_inputs(c, DEV)
        y64, st64 = kc.gn_ref64_fwd(x1, x2, gamma, beta, c.B, c.HW, c.G, c.eps, c.silu)
        refs[c] = dict(inputs=(x1, x2, gamma, beta, dy, a1, a2), y64=y64, st64=st64, model=stats_model(x1, x2, c))
    return refs


def _check(rows, bad, worst, half=True):
    for name, e, tol in rows:
        assert math.isfinite(e), name
        if e > worst[1]:
            worst[:] = [name, e]
        if not e <= (tol / 2 if half else tol):
            bad.append((name, e, tol))
    return len(rows)


def test_rounding_only_model_stays_under_half_the_tolerance(gn_refs):
    """every row check_norms emits from norm_slices / colblock_rows / gn_stat_rows, for every case, on the rounding-only model; prints the worst"""
    assert len(set(kc.GN_CASES)) == len(kc.GN_CASES) and len(set(kc.LN_CASES)) == len(kc.LN_CASES)
    worst, worst_stat, bad, n = ["", 0.0], ["", 0.0], [], 0
    for c in kc.GN_CASES:
        r = gn_refs[c]
        x1, x2, gamma, beta, dy, a1, a2 = r["inputs"]
        tag, slab = kc.gn_tag(c), kc.norm_plan(c)["ni"] > 0
        ym = rounded(r["y64"])
        for chunked in sorted({not slab, True}):
            n += _check(kc.norm_slices(f"{tag} fwd chunked={chunked}", ym, r["y64"], c, chunked=chunked), bad, worst)
        stat_rows = kc.gn_stat_rows(tag, r["model"], r["st64"])
        if c.shift:      # the fp32 store of the mean: half an ulp of the mean, in units of the standard deviation (see the module docstring)
            bound = float((r["st64"][..., 0].abs().max().log2().floor() - 24).exp2() * r["st64"][..., 1].max())
            assert stat_rows[0][1] <= bound < kc.STAT_TOL, (stat_rows[0], bound)
            _check(stat_rows[:1], [], worst_stat)
            stat_rows = stat_rows[1:]
        n += _check(stat_rows, bad, worst_stat)
        st32 = r["st64"].to(f32)
        for u1, u2 in c.adds:
            d64, ga64, be64 = kc.gn_ref64_bwd(x1, x2, dy, st32, gamma, beta, a1 if u1 else None, a2 if u2 else None, c.B, c.HW, c.G, c.silu)
            dm = rounded(d64)
            for chunked in sorted({not slab, True}):
                n += _check(kc.norm_slices(f"{tag} bwd add{int(u1)}{int(u2)} chunked={chunked}", dm, d64, c, chunked=chunked), bad, worst)
            n += _check(kc.colblock_rows(tag + " dgamma", rounded(ga64, f32), ga64) + kc.colblock_rows(tag + " dbeta", rounded(be64, f32), be64), bad, worst_stat)
    for i, case in enumerate(kc.LN_CASES):
        x, gamma, beta, dy, x32, skip = kc.ln_inputs(case, i, DEV)
        tag, rpw = "layernorm %dx%d" % case, kc.norm_plan(case)["rpw"]
        y64, st64 = kc.ln_ref64_fwd(x, gamma, beta, 1e-5)
        n += _check(kc.norm_slices(tag + " fwd", rounded(y64), y64, case, rpw=rpw), bad, worst)
        y64f = kc.ln_ref64_fwd(x32, gamma, beta, 1e-5)[0]
        n += _check(kc.norm_slices(tag + " fwd fp32 input", rounded(y64f), y64f, case, rpw=1), bad, worst)
        for add in (None, skip):
            d64, ga64, be64 = kc.ln_ref64_bwd(x, dy, gamma, st64.to(f32), add=add)
            n += _check(kc.norm_slices(tag + " bwd" + (" + residual grad" if add is not None else ""), rounded(d64), d64, case, rpw=1), bad, worst)
        n += _check(kc.colblock_rows(tag + " dgamma", rounded(ga64, f32), ga64) + kc.colblock_rows(tag + " dbeta", rounded(be64, f32), be64), bad, worst_stat)
    print("rounding-only model: %d rows; worst bf16 row %.3e (%s); worst statistics / fp32 row %.3e (%s)" % (n, worst[1], worst[0], worst_stat[1], worst_stat[0]))
    assert n > 600
    assert not bad, "the rounding-only model is not within half the tolerance:\n" + "\n".join(f"  {nm}: {e:.3e} > {t / 2:.1e}" for nm, e, t in bad)


def test_finer_slices_would_be_too_tight(gn_refs):
    """why gn_slices stops at whole pixel rows: the rounding-only model of a single (pixel, group) cell of 10 channels is over half the
    tolerance; whole pixel rows and (batch, group) slabs are under it (single LayerNorm rows are too, down to D = 64: they stay)"""
    c = next(c for c in kc.GN_CASES if (c.B, c.HW, c.C1, c.C2) == (3, 256, 320, 0))
    y64 = gn_refs[c]["y64"]
    d2 = (rounded(y64).to(f64) - y64).square().reshape(c.B * c.HW, c.G, 10).sum(-1)
    cell = float((d2 / y64.square().reshape(c.B * c.HW, c.G, 10).sum(-1)).sqrt().max())
    rows = kc.norm_slices("t", rounded(y64), y64, c)
    coarse = max(e for _, e, _ in rows)
    print("single (pixel, group) cell of 10 channels: %.3e; worst row of norm_slices: %.3e" % (cell, coarse))
    assert cell > kc.TOL1 / 2 >= coarse


def test_statistics_tolerance(gn_refs):
    """STAT_TOL = min(4 x the model's worst statistics error over all cases, 1e-5); prints the measurement per kind"""
    worst = {}
    for c in kc.GN_CASES:
        r = gn_refs[c]
        (_, em, _), (_, er, _) = kc.gn_stat_rows("", r["model"], r["st64"])
        for kind, e in (("mean, shifted" if c.shift else "mean", em), ("rstd", er)):
            if e > worst.get(kind, ("", -1.0))[1]:
                worst[kind] = (kc.gn_tag(c), e)
    for kind, (tag, e) in sorted(worst.items()):
        print("statistics model, worst %s error: %.3e (%s)" % (kind, e, tag))
    w = max(e for _, e in worst.values())
    print("4 x worst = %.3e, cap 1e-5 -> STAT_TOL %.1e" % (4 * w, min(4 * w, 1e-5)))
    assert kc.STAT_TOL == pytest.approx(min(4 * w, 1e-5), rel=0.02)
    assert 4 * max(worst["rstd"][1], worst["mean"][1]) <= kc.STAT_TOL / 2      # every row but the shifted means: 4 x 1.05e-6 = 4.2e-6
    assert worst["mean, shifted"][1] < kc.STAT_TOL      # the cap binds on these: reported in the module docstring and DESIGN 2.2b


@pytest.mark.parametrize("kw", [dict(final=f32), dict(inv_n_f32=True)], ids=["fp32 finalisation", "fp32 reciprocal of n"])
def test_a_statistics_shortcut_fails_the_statistics_row_on_the_shifted_mean_inputs(gn_refs, kw):
    for c in kc.GN_CASES:
        if not c.shift:
            continue
        r = gn_refs[c]
        rows = kc.gn_stat_rows(kc.gn_tag(c), stats_model(r["inputs"][0], r["inputs"][1], c, **kw), r["st64"])
        print(["%.2e" % e for _, e, _ in rows])
        assert rows[1][1] > 5 * kc.STAT_TOL, rows      # |d rstd| / rstd
        # ... which the whole-tensor figure check_norms had (relative L2 of all (mean, rstd) at 1e-4) lets through: the means dominate its norm
        assert kc.rel(stats_model(r["inputs"][0], r["inputs"][1], c, **kw), r["st64"]) <= 1e-4


def test_the_column_statistics_path_needs_centred_partials_on_the_shifted_mean_inputs(gn_refs):
    """gn_stats_cols_kernel's fp32 partial of one (batch, chunk, group): with the raw sum of squares (32 pixels x 10 channels of x^2 ~ 4100 =
    1.3e6, an fp32 ulp 0.125) the model of that path is over the tolerance on the shifted-mean inputs — var = Q / n - mean^2 magnifies the
    partials' rounding by mean^2 / var = 1.5e4; norm.hip did that and measured 1.9e-4 on the MI355X.  With the centred second moment
    M2 = q - s^2 / n_c in the partial, which it stores now, the model is exact before the store."""
    for c in kc.GN_CASES:
        if kc.norm_plan(c)["calls"].get("fwd_cs", [""])[0] != "gn_stats_cols_kernel":
            continue
        r = gn_refs[c]
        raw, cen = (kc.gn_stat_rows("cols", stats_model(r["inputs"][0], r["inputs"][1], c, cols=True, centred=k), r["st64"])[1][1] for k in (False, True))
        print("column-statistics path model on %s: |d rstd| / rstd %.3e with raw, %.3e with centred partials" % (kc.gn_tag(c), raw, cen))
        assert cen <= kc.STAT_TOL / 2
        if c.shift:
            assert raw > kc.STAT_TOL and cen < 1e-7


def _case(B, HW, C1, C2):
    return next(c for c in kc.GN_CASES if (c.B, c.HW, c.C1, c.C2) == (B, HW, C1, C2))


def _failing(rows):
    return [nm for nm, e, t in rows if not e <= t]


def test_one_group_with_a_wrong_rstd_fails_the_group_slice():
    """one (batch, group) of 64 of (2, 256, 320) normalised with rstd x 1.02"""
    c = kc._gn(2, 256, 320, 0, True)._replace(seed=1500)
    x1, x2, gamma, beta, _, _, _ = kc.gn_inputs(c, DEV)
    y64, st64 = kc.gn_ref64_fwd(x1, None, gamma, beta, c.B, c.HW, c.G, c.eps, False)      # pre-activation
    xh = (y64 - beta.to(f64)) / gamma.to(f64)
    xh4 = xh.reshape(c.B, c.HW, c.G, 10).clone()
    xh4[1, :, 17] *= 1.02
    ref, got = kc._silu64(y64), rounded(kc._silu64(xh4.reshape(-1, 320) * gamma.to(f64) + beta.to(f64)))
    assert kc.rel(got, ref) <= kc.TOL1
    bad = _failing(kc.norm_slices("t", got, ref, c))
    assert any("worst (batch, group)" in nm for nm in bad), bad


def test_a_chunks_last_pixel_carrying_its_neighbours_output_fails_the_last_pixel_slice(gn_refs):
    """the last pixel of one chunk of (2, 260, 320) carries the previous pixel's output.  With independent pixels that is one wholly wrong pixel
    row of 520, which the whole tensor sees too (6e-2); the slice sees it 20 times as large.  The same error at 5 % of its size — a last pixel
    leaning towards its neighbour — passes the whole tensor and fails the slice."""
    c = _case(2, 260, 320, 0)
    pl = kc.norm_plan(c)
    y64 = gn_refs[c]["y64"]
    p = 7 * pl["ppc"] + pl["ppc"] - 1      # the last pixel of chunk 7
    for frac, whole_passes in ((1.0, False), (0.05, True)):
        g64 = y64.reshape(c.B, c.HW, 320).clone()
        g64[1, p] += frac * (g64[1, p - 1] - g64[1, p])
        got = rounded(g64.reshape(-1, 320))
        rows = kc.norm_slices("t", got, y64, c)
        hit = [e for nm, e, _ in rows if "last pixel row of a chunk" in nm][0]
        print("last pixel of a chunk, %g of its neighbour: whole tensor %.3e, slice %.3e" % (frac, kc.rel(got, y64), hit))
        assert (kc.rel(got, y64) <= kc.TOL1) == whole_passes
        assert hit > 10 * kc.rel(got, y64) and hit > kc.TOL1
        assert not any("first pixel row" in nm for nm in _failing(rows))


def test_dx2s_first_chunk_taken_from_dx1s_last_fails_the_concat_slice(gn_refs):
    """the first 8-channel chunk of dx2 taken from dx1's last chunk in (2, 256, 1280, 640): dx1 is right, dx2 as one tensor sees 8 wrong channels
    of 640 (0.38: dx1 carries its shortcut gradient), the slice sees them undiluted (3.3) and names the place.  At 1 % of its size the error passes
    dx2's whole-tensor figure and fails the slice."""
    c = _case(2, 256, 1280, 640)
    x1, x2, gamma, beta, dy, a1, a2 = gn_refs[c]["inputs"]
    d64, _, _ = kc.gn_ref64_bwd(x1, x2, dy, gn_refs[c]["st64"].to(f32), gamma, beta, a1, None, c.B, c.HW, c.G, c.silu)
    for frac, whole_passes in ((1.0, False), (0.01, True)):
        g64 = d64.clone()
        g64[:, 1280:1288] += frac * (d64[:, 1272:1280] - d64[:, 1280:1288])
        got = rounded(g64)
        e1, e2 = kc.rel(got[:, :1280], d64[:, :1280]), kc.rel(got[:, 1280:], d64[:, 1280:])
        rows = kc.norm_slices("t", got, d64, c)
        hit = [e for nm, e, _ in rows if "first chunk of the second source" in nm]
        print("dx2's first chunk, %g of dx1's last: dx1 %.3e, dx2 %.3e, slice %.3e" % (frac, e1, e2, hit[0]))
        assert e1 <= kc.TOL1 and (e2 <= kc.TOL1) == whole_passes
        assert len(hit) == 1 and hit[0] > kc.TOL1 and hit[0] > 5 * e2
        assert not any("last chunk of the first source" in nm for nm in _failing(rows))


def test_the_last_row_normalised_with_its_neighbours_statistics_fails_the_last_wave_slice():
    case = (4101, 640)
    x, gamma, beta, _, _, _ = kc.ln_inputs(case, kc.LN_CASES.index(case), DEV)
    y64, st64 = kc.ln_ref64_fwd(x, gamma, beta, 1e-5)
    got = rounded(y64).clone()
    got[-1] = rounded((x[-1].to(f64) - st64[-2, 0]) * st64[-2, 1] * gamma.to(f64) + beta.to(f64))
    assert kc.rel(got, y64) <= kc.TOL1
    bad = _failing(kc.norm_slices("t", got, y64, case, rpw=kc.norm_plan(case)["rpw"]))
    assert any("the last wave" in nm for nm in bad) and any("the last block" in nm for nm in bad), bad


def test_a_column_block_missing_its_last_row_split_fails_the_block_row():
    """columns 64-127 of dgamma at D = 200 without the rows of the last of the five row splits of M = 4101.  The whole-vector figure sees this
    one too (a fifth of the rows of a third of the columns is no subtle error): the block row sees it sqrt(200 / 64) = 1.8 times as large, which
    is the window in which an error passes the whole vector at its tolerance and fails the block."""
    case = (4101, 200)
    x, gamma, beta, dy, _, _ = kc.ln_inputs(case, kc.LN_CASES.index(case), DEV)
    _, st64 = kc.ln_ref64_fwd(x, gamma, beta, 1e-5)
    _, ga64, _ = kc.ln_ref64_bwd(x, dy, gamma, st64.to(f32))
    r0 = 4 * -(-4101 // 5)
    part = kc.ln_ref64_bwd(x[:r0], dy[:r0], gamma, st64[:r0].to(f32))[1]
    got = ga64.clone()
    got[64:128] = part[64:128]
    whole, block = kc.rel(got.to(f32), ga64), kc.colblock_rows("t", got.to(f32), ga64)[0][1]
    print("dgamma without the last row split in columns 64-127: whole vector %.3e, worst 64-column block %.3e" % (whole, block))
    assert block > 1e-3 and block > 1.5 * whole
    got = ga64.clone()
    got[64:128] += (part[64:128] - ga64[64:128]) * (1.4e-3 / block)      # the same error scaled into the window
    assert kc.rel(got, ga64) <= 1e-3 < kc.colblock_rows("t", got, ga64)[0][1]


def test_norm_slices_labels_and_nan():
    c = _case(2, 260, 320, 0)
    ref = torch.randn(c.B * c.HW, 320, generator=torch.Generator().manual_seed(1), dtype=f64)
    names = [nm.split(": ")[1].split(" (")[0] for nm, _, _ in kc.norm_slices("t", ref, ref, c)]
    assert names == ["worst", "worst first pixel row of a chunk", "worst last pixel row of a chunk", "channels 312-319"]
    got = ref.clone()
    got[300, 5] = float("nan")
    assert {e for _, e, _ in kc.norm_slices("t", got, ref, c)[:1]} == {float("inf")}
    c2 = _case(2, 100, 1280, 1280)
    names = [nm.split(": ")[1] for nm, _, _ in kc.norm_slices("t", torch.ones(200, 2560), torch.ones(200, 2560), c2, chunked=False)]
    assert any("items 1792-1999" in nm for nm in names) and any("the second slot" in nm for nm in names) and any("channels 1280-1287" in nm for nm in names)
    assert [nm.split(": ")[1].split(" (")[0] for nm, _, _ in kc.norm_slices("t", torch.ones(5, 1536), torch.ones(5, 1536), (5, 1536))] == [
        "worst row", "rows 4-4", "rows 4-4", "columns 1528-1535", "columns 0-7", "columns 512-519", "columns 1024-1031"]
