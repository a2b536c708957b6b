"""CPU: the localised attention comparison of tests/kernel_checks.py (slices()) is neither too tight nor too loose.

Not too tight: a rounding-only model of the kernels — an fp32 restatement of forward and backward that rounds what the kernels round to bf16
(P in front of P.V and P^T.dO, dS in front of dS.K and dS^T.Q, every output), and is otherwise exact — held against an fp64 evaluation of the
same bf16 inputs stays under HALF the GPU check's tolerance (TOL2, 1e-3 for the LSE) on EVERY row slices() emits, for the shapes the check
adds and for its peaked-score inputs.  What the kernels add to that model is summation order and exp2's last bits; the other half is theirs.

Not too loose: an error the whole-tensor relative L2 cannot see (5 % on the last 12 query rows of one head of 32) fails the slice rows."""
import math

import pytest
import torch

import kernel_checks as kc

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
LOG2E = 1.0 / math.log(2.0)


def _heads(t, B, L, H, DH, dt):
    return t[:, : H * DH].to(dt).reshape(B, L, H, DH).permute(0, 2, 1, 3)


def _rows(t, B, L, H, DH):
    return t.permute(0, 2, 1, 3).reshape(B * L, H * DH)


def attention_model(q, k, v, do, B, H, T, S, DH, scale, causal, dt, o=None, lse=None):
    """dt = fp64: the reference (nothing rounded but the outputs' storage types, as EmuBackend); dt = fp32: the rounding-only model of the
    kernels.  o / lse given: the backward uses them instead of its own forward's.  -> o (bf16), lse (fp32, log2 units), dq, dk, dv (bf16)"""
    rb = (lambda t: t.to(bf16).to(dt)) if dt == f32 else (lambda t: t)
    Q, K, V, dO = _heads(q, B, T, H, DH, dt), _heads(k, B, S, H, DH, dt), _heads(v, B, S, H, DH, dt), _heads(do, B, T, H, DH, dt)
    s2 = (Q @ K.transpose(-1, -2)) * (scale * LOG2E)
    if causal:
        s2 = s2.masked_fill(torch.arange(S)[None, :] > torch.arange(T)[:, None], float("-inf"))
    m = s2.amax(-1, keepdim=True)
    p = torch.exp2(s2 - m)
    l = p.sum(-1, keepdim=True)
    if o is None:
        o = _rows((rb(p) @ V) / l, B, T, H, DH).to(bf16)
        lse = (m + torch.log2(l)).squeeze(-1).to(f32)
    P = torch.exp2(s2 - lse.to(dt)[..., None])
    dV = rb(P).transpose(-1, -2) @ dO
    delta = (dO * _heads(o, B, T, H, DH, dt)).sum(-1, keepdim=True)
    dS = rb(P * (dO @ V.transpose(-1, -2) - delta))
    dQ, dK = dS @ K * scale, dS.transpose(-1, -2) @ Q * scale
    return o, lse, _rows(dQ, B, T, H, DH).to(bf16), _rows(dK, B, S, H, DH).to(bf16), _rows(dV, B, S, H, DH).to(bf16)


def _slice_rows(tag, B, H, T, S, DH, got, ref, **kw):
    return kc.attention_slices(tag, B, H, T, S, DH, got[0], ref[0], got[1], ref[1], got[2:], ref[2:], **kw)


def _assert_half(rows):
    assert rows and all(math.isfinite(e) for _, e, _ in rows)
    bad = [(n, e, t) for n, e, t in rows if not e <= t / 2]
    assert not bad, "the rounding-only model is not within half the tolerance:\n" + "\n".join(f"  {n}: {e:.3e} > {t / 2:.1e}" for n, e, t in bad)


@pytest.mark.parametrize("case", kc.ATTENTION_NEW_CASES, ids=kc._attention_tag)
def test_rounding_only_model_stays_under_half_the_tolerance(case):
    (B, H, T, S, DH), causal = case[:5], len(case) > 5 and case[5]
    dev = torch.device("cpu")
    g = kc.gen(90 + kc.ATTENTION_CASES.index(case), dev)
    q, k, v, _, _ = kc._attention_inputs(g, B, H, T, S, DH, dev)
    do = kc.rnd(g, B * T, H * DH, dev=dev)
    args = (q, k, v, do, B, H, T, S, DH, DH ** -0.5, causal)
    ref, got = attention_model(*args, f64), attention_model(*args, f32)
    rows = [(nm, kc.rel(a, b), 1e-3 if nm == "LSE" else kc.TOL2) for nm, a, b in zip(("O", "LSE", "dQ", "dK", "dV"), got, ref)]
    _assert_half(rows + _slice_rows(kc._attention_tag(case), B, H, T, S, DH, got, ref))


@pytest.mark.parametrize("name", list(kc.ATTENTION_PEAKED))
def test_rounding_only_model_on_the_peaked_inputs(name):
    _, (B, H, T, S, DH), _ = kc.ATTENTION_PEAKED[name]
    q, k, v, do = kc.peaked_attention_inputs(name, torch.device("cpu"))
    args = (q, k, v, do, B, H, T, S, DH, 1.0, False)
    ref = attention_model(*args, f64)
    assert float(ref[1].abs().max()) * math.log(2.0) > 200.0      # |LSE| in natural-log units: the inputs are peaked indeed
    fwd = attention_model(*args, f32)
    got = fwd[:2] + attention_model(*args, f32, o=ref[0], lse=ref[1])[2:]      # the backward of both sides on the reference's O and LSE
    rows = [(nm, kc.rel(a, b), 1e-3 if nm == "LSE" else kc.TOL2) for nm, a, b in zip(("O", "LSE", "dQ", "dK", "dV"), got, ref)]
    _assert_half(rows + _slice_rows(name, B, H, T, S, DH, got, ref, every_block=True))


def test_slices_fail_where_the_whole_tensor_passes():
    """(2, 16, 1100, 2090, 40): the last query tile holds 12 rows.  5 % on those rows of one head moves the whole dQ by 0.05 * sqrt(12 / (32 * 1100))
    = 0.09 % and that head's by 0.5 %: both pass at TOL2 = 1.5 %.  The last block alone shows the 5 %."""
    B, H, T, S, DH = 2, 16, 1100, 2090, 40
    assert (B, H, T, S, DH) in kc.ATTENTION_CASES
    g = kc.gen(7, torch.device("cpu"))
    ref = kc.rnd(g, B * T, H * DH, dev="cpu")
    got = ref.clone()
    assert not any(e > 0 for _, e, _ in kc.slices("dQ", got, ref, B, T, H, DH, kc.BLOCK_Q))
    b, h = 1, 9
    got[b * T + T - 12:(b + 1) * T, h * DH:(h + 1) * DH] = (ref[b * T + T - 12:(b + 1) * T, h * DH:(h + 1) * DH].float() * 1.05).to(bf16)
    assert kc.rel(got, ref) < kc.TOL2
    rows = kc.slices("dQ", got, ref, B, T, H, DH, kc.BLOCK_Q)
    assert len(rows) == 3
    (_, head, _), (n_last, last, tol), (_, front, _) = rows
    assert "rows 1088-1099" in n_last and tol == kc.TOL2
    assert head < kc.TOL2 and front == 0.0      # per head it still drowns; the block in front is clean
    assert 0.04 < last < 0.06 and last > tol
    # per head alone (what the B * T >= 8192 cases get) sees an error over a whole head
    got = ref.clone()
    got[:T, :DH] = (ref[:T, :DH].float() * 1.05).to(bf16)
    assert kc.rel(got, ref) < kc.TOL2 < kc.slices("dQ", got, ref, B, T, H, DH, kc.BLOCK_Q, blocks=False)[0][1]


def test_slices_report_nan_as_infinite():
    ref = torch.ones(128, 8)
    got = ref.clone()
    got[100, 3] = float("nan")
    assert all(e == float("inf") for _, e, _ in kc.slices("x", got, ref, 1, 128, 1, 8, 64)[:2])
