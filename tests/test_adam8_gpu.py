"""GPU: AdamW with block-wise 8-bit moments (e4t_adamw8).  The kernel against the float64 restatement of
tests/adam8_reference.py (parameters, average and scales by rel-L2; codes equal outside a 1e-5 band around the code midpoints), bitwise between
its EMA / plain and scalar / device-scalar forms, against e4t_adamw from a fresh state, on slices, inside guard bands, its argument checks,
special blocks, twenty steps against float64 AdamW; the trainer on the tiny models: eager equals replayed, and what is launched."""
import pytest
import torch

import adam8_reference as ref8
import ema_reference as ref
from kernel_checks import TOLF, gen, rnd
from test_ema_gpu import PIDX, _models, _run, batches  # noqa: F401  (batches: the module-scoped fixture of the EMA tests, instantiated for this module)

pytestmark = pytest.mark.gpu
f32, f64, u8 = torch.float32, torch.float64, torch.uint8
HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-2, step=3, grad_scale=0.5)
EMA_W = 0.125 + 1e-3
DECAY = 0.9999
BAND = 1e-5              # relative distance of a normalised moment to a code midpoint inside which fp32 and float64 may choose different neighbours
BAND_CAP = 0.005         # at most this fraction of the elements may lie in the band (Gaussian inputs of this style: about 0.06 %)


@pytest.fixture(scope="module")
def codes():
    from e4t.optimization import dynamic_codebook
    dev = torch.device("cuda:0")
    return dynamic_codebook(True).to(dev), dynamic_codebook(False).to(dev)


def _hyper(dev, lr, beta1, beta2, step, grad_scale, ema_w=None):
    bc1, bc2s = ref.bias_corrections(beta1, beta2, step)
    return torch.tensor([lr, bc1, bc2s, grad_scale] + ([ema_w, 0.0, 0.0, 0.0] if ema_w is not None else []), dtype=f32, device=dev)


def _state_inputs(n, seed, dev, codes):
    """test_ema_gpu._flat_inputs' style, with the moments quantised: a valid 8-bit state -> p, g, qm, qv, am, av, ema"""
    from e4t.optimization import quantize_blockwise
    g = gen(seed, dev)
    p, grad, m, v, e = (rnd(g, n, dtype=f32, dev=dev), rnd(g, n, dtype=f32, dev=dev), rnd(g, n, dtype=f32, dev=dev) * 0.1,
                        rnd(g, n, dtype=f32, dev=dev).abs() * 0.01, rnd(g, n, dtype=f32, dev=dev))
    qm, am = quantize_blockwise(m, codes[0])
    qv, av = quantize_blockwise(v, codes[1])
    return p, grad, qm, qv, am, av, e


def _launch(hip, codes, p, g, qm, qv, am, av, ema=None, hyper=None, **over):
    """one adamw8 call on clones -> (p', qm', qv', am', av', ema')"""
    hp = dict(HP, **over)
    out = [t.clone() for t in (p, qm, qv, am, av)] + [None if ema is None else ema.clone()]
    hip.adamw8(out[0], g, out[1], out[2], out[3], out[4], codes[0], codes[1], hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["wd"], hp["step"],
               hp["grad_scale"], ema=out[5], ema_w=hp.get("ema_w", 0.0), hyper=hyper)
    return out


def _grid_cap(hip, dev, codes, tmp_path):
    """the capped grid of the kernel, read from its own launch-log line at a size far past one trip"""
    n = 16 << 20
    p = torch.zeros(n, dtype=f32, device=dev)
    qm = torch.zeros(n, dtype=u8, device=dev)
    am = torch.zeros(n // 256, dtype=f32, device=dev)
    log = tmp_path / "cap.txt"
    assert hip.lib.e4t_set_launch_log(str(log).encode()) == 0
    try:
        hip.adamw8(p, p.clone(), qm, qm.clone(), am, am.clone(), codes[0], codes[1], 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    finally:
        hip.lib.e4t_set_launch_log(None)
    torch.cuda.synchronize()
    shape = log.read_text().splitlines()[0].split("|")[1]
    grid = int(shape.split("grid")[1])
    assert grid * 1024 < n          # the cap was in force
    return grid


def _same(got, want, tag):
    """bit-identical (p', qm', qv', absmax_m', absmax_v'[, ema']) tuples, naming the first that is not"""
    for name, a, b in zip(("p", "qm", "qv", "absmax_m", "absmax_v", "ema"), got, want):
        assert torch.equal(a, b), (tag, name, int((a != b).sum()), "elements differ, first at", int((a != b).nonzero()[0]))


def _compare(tag, got, want, n):
    p1, qm1, qv1, am1, av1, e1 = got
    for name, a, b in (("p", p1, want["p"]), ("absmax_m", am1, want["absmax_m"]), ("absmax_v", av1, want["absmax_v"])) + \
            ((("ema", e1, want["ema"]),) if e1 is not None else ()):
        err = ref.rel_l2(a, b)
        print(f"{tag} {name}: rel-L2 {err:.3e}")
        assert err <= TOLF, (tag, name, err)
    for name, q, wq, band in (("qm", qm1, want["qm"], want["band_m"]), ("qv", qv1, want["qv"], want["band_v"])):
        inside = band <= BAND
        frac = float(inside.double().mean())
        diff = (q.long() - wq).abs()
        print(f"{tag} {name}: {100 * frac:.4f} % of {n} in the band, {int((diff != 0).sum())} codes differ, largest difference {int(diff.max())}")
        assert frac <= BAND_CAP, (tag, name, frac)
        assert not bool(diff[~inside].any()), (tag, name, "a code outside the band differs")
        assert int(diff.max()) <= 1, (tag, name)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1027, 100003, "second_trip"])
def test_kernel_against_float64_and_bitwise(hip_env, codes, tmp_path, n):
    hip, _, dev, _ = hip_env
    if n == "second_trip":
        n = _grid_cap(hip, dev, codes, tmp_path) * 1024 + 257          # one full grid-stride trip of the capped grid, a block and one element
    p, g, qm, qv, am, av, e = _state_inputs(n, 580, dev, codes)
    want = ref8.adamw8_f64(p, g, qm, qv, am, av, codes[0], codes[1], HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], HP["wd"], HP["step"], HP["grad_scale"],
                           ema=e, ema_w=EMA_W)
    with_ema = _launch(hip, codes, p, g, qm, qv, am, av, ema=e, ema_w=EMA_W)
    _compare(f"adamw8_ema n={n}", with_ema, want, n)
    assert not torch.equal(with_ema[5], e) and not torch.equal(with_ema[0], p)
    if n > 4:
        assert not torch.equal(with_ema[1], qm) and not torch.equal(with_ema[2], qv)
    # the plain instantiation: the same p', codes and scales, bit for bit
    plain = _launch(hip, codes, p, g, qm, qv, am, av)
    _same(plain[:5], with_ema[:5], "plain against EMA")
    # device-resident scalars (fp32 [4] / [8]): the same bits, the scalar arguments they replace are ignored
    junk = dict(lr=7.0, step=0, grad_scale=9.0)
    h4 = _launch(hip, codes, p, g, qm, qv, am, av, hyper=_hyper(dev, HP["lr"], HP["beta1"], HP["beta2"], HP["step"], HP["grad_scale"]), **junk)
    _same(h4[:5], plain[:5], "device scalars [4] against scalar arguments")
    h8 = _launch(hip, codes, p, g, qm, qv, am, av, ema=e, ema_w=0.9,
                 hyper=_hyper(dev, HP["lr"], HP["beta1"], HP["beta2"], HP["step"], HP["grad_scale"], EMA_W), **junk)
    _same(h8, with_ema, "device scalars [8] against scalar arguments")


@pytest.mark.parametrize("step", [1, 3])
def test_fresh_state_equals_adamw_from_zero_moments(hip_env, codes, step):
    """m = v = 0 exactly and p moves by the unquantised new moments (the same body, the same contraction): e4t_adamw's p', bit for bit.
    This equality depends on the compiler: adamw_kernel is built with -ffp-contract=fast and adamw8_kernel writes out the fused multiply-adds that the
    current hipcc picks for it (fused in the float4 path, a product and a difference in the scalar loop of the last partial quad).  A
    ROCm update that contracts adamw_kernel differently breaks this test with no source change; the remedy is then to read adamw_kernel's new
    assembly and restate it in adamw8_kernel, not to touch the test."""
    from e4t.optimization import Adam8State
    hip, _, dev, _ = hip_env
    n = 100003
    p, g = _state_inputs(n, 581, dev, codes)[:2]
    st = Adam8State(n, dev)
    assert st.zero_m != 0 and bool((st.qm == st.zero_m).all())
    got = _launch(hip, codes, p, g, st.qm, st.qv, st.absmax_m, st.absmax_v, step=step)
    p2, m2, v2 = p.clone(), torch.zeros_like(p), torch.zeros_like(p)
    hip.adamw(p2, g, m2, v2, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], HP["wd"], step, HP["grad_scale"])
    assert torch.equal(got[0], p2)
    # ... and the scales are the block maxima of that kernel's moments
    from adam8_reference import _blocks
    assert torch.equal(got[3], _blocks(m2).abs().amax(1)) and torch.equal(got[4], _blocks(v2).amax(1))


def test_a_slice_at_a_block_boundary_gives_the_whole_buffers_bits(hip_env, codes):
    hip, _, dev, _ = hip_env
    n, k = 256 * 9 + 77, 3
    p, g, qm, qv, am, av, e = _state_inputs(n, 582, dev, codes)
    whole = _launch(hip, codes, p, g, qm, qv, am, av, ema=e, ema_w=EMA_W)
    lo = 256 * k
    part = _launch(hip, codes, p[lo:], g[lo:], qm[lo:], qv[lo:], am[k:], av[k:], ema=e[lo:], ema_w=EMA_W)
    for w, s, o in zip(whole, part, (lo, lo, lo, k, k, lo)):
        assert torch.equal(w[o:], s)
    # a middle slice of whole blocks
    hi = 256 * 7
    mid = _launch(hip, codes, p[lo:hi], g[lo:hi], qm[lo:hi], qv[lo:hi], am[k:7], av[k:7])
    for w, s, (a, b) in zip(whole[:5], mid[:5], ((lo, hi), (lo, hi), (lo, hi), (k, 7), (k, 7))):
        assert torch.equal(w[a:b], s)


SENT = 0x7FC00ABC          # a quiet NaN with a payload (test_ema_gpu's sentinel); its bytes are the poison of the byte buffers


def _guarded(t, guard=64):
    """t inside a buffer of sentinels (guard 4-byte words on either side; t starts 16-byte aligned) -> (the view in t's place, the whole buffer as bytes, the
    byte range of t in it)"""
    nbytes = t.numel() * t.element_size()
    words = guard + (nbytes + 3) // 4 + guard
    buf = torch.full((words,), SENT, dtype=torch.int32, device=t.device).view(u8)
    lo = 4 * guard
    inner = buf[lo:lo + nbytes].view(t.dtype)
    inner.copy_(t)
    return inner, buf, (lo, lo + nbytes)


def test_guard_bands(hip_env, codes):
    hip, _, dev, _ = hip_env
    n = 1027          # neither a multiple of 4 nor of 256: a short last block whose last lane holds three elements
    p, g, qm, qv, am, av, e = _state_inputs(n, 583, dev, codes)
    plain = _launch(hip, codes, p, g, qm, qv, am, av, ema=e, ema_w=EMA_W)
    held = [_guarded(t) for t in (p, qm, qv, am, av, e)]
    pristine = [buf.clone() for _, buf, _ in held]
    g0, c0 = g.clone(), (codes[0].clone(), codes[1].clone())
    pg, qmg, qvg, amg, avg, eg = (h[0] for h in held)
    hip.adamw8(pg, g, qmg, qvg, amg, avg, codes[0], codes[1], HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], HP["wd"], HP["step"], HP["grad_scale"],
               ema=eg, ema_w=EMA_W)
    torch.cuda.synchronize()
    for (inner, buf, (lo, hi)), was, want in zip(held, pristine, plain):
        assert torch.equal(inner, want)
        assert torch.equal(buf[:lo], was[:lo]) and torch.equal(buf[hi:], was[hi:])          # not one byte outside the n elements
    assert torch.equal(g, g0) and torch.equal(codes[0], c0[0]) and torch.equal(codes[1], c0[1])


def test_bad_arguments_are_refused_before_any_launch(hip_env, codes, tmp_path):
    hip, _, dev, ops = hip_env
    n = 1024
    p, g, qm, qv, am, av, e = _state_inputs(n + 16, 584, dev, codes)
    am, av = torch.cat([am, am]), torch.cat([av, av])          # (room for the misaligned views below)
    hyper = _hyper(dev, 1e-3, 0.9, 0.999, 3, 0.5, EMA_W)
    tensors = (p, qm, qv, am, av, e)
    before = [t.clone() for t in tensors]
    ptr, s = (lambda t: t.data_ptr()), ops._stream()
    good = dict(p=ptr(p), g=ptr(g), qm=ptr(qm), qv=ptr(qv), am=ptr(am), av=ptr(av), ema=ptr(e), cm=ptr(codes[0]), cv=ptr(codes[1]), step=3, hyper=None)

    def call(**kw):
        a = dict(good, **kw)
        return hip.lib.e4t_adamw8(a["p"], a["g"], a["qm"], a["qv"], a["am"], a["av"], a["ema"], n, a["cm"], a["cv"], 1e-3, 0.9, 0.999, 1e-8, 1e-2, a["step"],
                                  0.5, EMA_W, a["hyper"], s)
    log = tmp_path / "launches.txt"
    assert hip.lib.e4t_set_launch_log(str(log).encode()) == 0
    try:
        for k in ("p", "g", "qm", "qv", "am", "av", "cm", "cv"):                       # no null pointer other than ema and hyper_dev
            assert call(**{k: None}) == -22, k
        for k in ("p", "g", "ema"):                                                     # 16-byte alignment
            assert call(**{k: good[k] + 4}) == -22 and call(**{k: good[k] + 8}) == -22, k
        for k in ("qm", "qv"):                                                          # 4-byte alignment
            assert call(**{k: good[k] + 1}) == -22 and call(**{k: good[k] + 2}) == -22, k
        for k in ("am", "av", "cm", "cv"):
            assert call(**{k: good[k] + 2}) == -22, k
        assert call(step=0) == -22 and call(step=-1) == -22                             # a step below 1 without device scalars
        assert call(hyper=ptr(hyper) + 4) == -22                                        # a misaligned hyper buffer
        assert hip.lib.e4t_adamw8(good["p"], good["g"], good["qm"], good["qv"], good["am"], good["av"], None, 0, good["cm"], good["cv"], 1e-3, 0.9, 0.999,
                                  1e-8, 1e-2, 3, 0.5, 0.0, None, s) == -22              # n = 0
    finally:
        hip.lib.e4t_set_launch_log(None)
    torch.cuda.synchronize()
    assert log.read_text() == ""                                                        # nothing was launched
    assert all(torch.equal(a, b) for a, b in zip(before, tensors))
    # what IS accepted, and its launch-log lines: step 0 with device scalars; 16 n + 16 ceil(n / 256) bytes, 8 n more with the average
    assert hip.lib.e4t_set_launch_log(str(log).encode()) == 0
    try:
        assert call(step=0, hyper=ptr(hyper)) == 0
        assert call(ema=None) == 0
        m = 1027
        hip.adamw8(p[:m], g[:m], qm[:m], qv[:m], am[:5], av[:5], codes[0], codes[1], 1e-3, 0.9, 0.999, 1e-8, 1e-2, 3)
    finally:
        hip.lib.e4t_set_launch_log(None)
    torch.cuda.synchronize()
    lines = [ln.split("|") for ln in log.read_text().splitlines()]
    assert [ln[0] for ln in lines] == ["adamw8_ema_kernel", "adamw8_kernel", "adamw8_kernel"]
    assert [float(ln[2]) for ln in lines] == [24.0 * n + 16.0 * 4, 16.0 * n + 16.0 * 4, 16.0 * 1027 + 16.0 * 5]
    assert [float(ln[3]) for ln in lines] == [0.0, 0.0, 0.0]


def test_special_blocks(hip_env, codes):
    from e4t.optimization import Adam8State, quantize_blockwise
    hip, _, dev, _ = hip_env
    n = 3 * 256 + 100
    st = Adam8State(n, dev)
    p = rnd(gen(585, dev), n, dtype=f32, dev=dev)
    g = torch.zeros(n, dtype=f32, device=dev)
    g[256:512] = 1e-3
    g[256 + 17] = 1e5                                            # block 1: one element 1e8 times the others
    g[512:768] = torch.linspace(-1, 0.5, 256, device=dev) * 0.25          # block 2: the minimum is -absmax
    # blocks 0 and 3 (short): an all-zero gradient on a fresh state
    got = _launch(hip, codes, p, g, st.qm, st.qv, st.absmax_m, st.absmax_v, step=1, grad_scale=1.0)
    p1, qm1, qv1, am1, av1, _ = got
    assert all(bool(torch.isfinite(t).all()) for t in (p1, am1, av1))
    for blk in (slice(0, 256), slice(768, n)):
        assert bool((qm1[blk] == st.zero_m).all()) and bool((qv1[blk] == st.zero_v).all())
        assert bool((p1[blk].abs() < p[blk].abs()).all()) and ref.rel_l2(p1[blk], p[blk].to(f64) * (1.0 - ref.f32r(HP["lr"]) * ref.f32r(HP["wd"]))) <= TOLF      # the decay alone
    assert am1[0] == 0 and av1[0] == 0 and am1[3] == 0 and av1[3] == 0
    # the moments the kernel formed, in fp32 (from zero moments the contraction cannot matter), through the definition
    one = torch.tensor(1.0, dtype=f32)
    m = (one - torch.tensor(HP["beta1"], dtype=f32)).to(dev) * g
    v = (one - torch.tensor(HP["beta2"], dtype=f32)).to(dev) * g * g
    wqm, wam = quantize_blockwise(m, codes[0])
    wqv, wav = quantize_blockwise(v, codes[1])
    assert torch.equal(qm1, wqm) and torch.equal(qv1, wqv) and torch.equal(am1, wam) and torch.equal(av1, wav)
    assert qm1[256 + 17] == 255 and qv1[256 + 17] == 255
    rest = torch.cat([qm1[256:256 + 17], qm1[256 + 18:512]]).long()
    assert bool(((rest == st.zero_m) | (rest == st.zero_m + 1)).all())
    assert qm1[512] == 0 and float(am1[2]) == float(m[512:768].abs().max())          # -absmax: index 0 of the signed map (-0.993)


def test_twenty_steps_against_float64_adamw(hip_env, codes):
    """rel-L2 between the displacement p_20 - p_0 of the kernel and that of float64 AdamW with unquantised moments, bounded by twice the figure the
    float64 restatement of the 8-bit algorithm gives on the same inputs (the factor 2 covers fp32-versus-float64 code flips)"""
    from e4t.optimization import Adam8State
    hip, _, dev, _ = hip_env
    n, steps = 4096, 20
    gg = gen(586, dev)
    p0 = rnd(gg, n, dtype=f32, dev=dev)
    drift = rnd(gg, n, dtype=f32, dev=dev)
    grads = [0.5 * drift + rnd(gg, n, dtype=f32, dev=dev) for _ in range(steps)]
    hp = dict(lr=HP["lr"], beta1=HP["beta1"], beta2=HP["beta2"], eps=HP["eps"], wd=HP["wd"])
    want = ref8.adamw32_f64_trajectory(p0, grads, grad_scale=1.0, **hp) - p0.to(f64)
    # the kernel
    st = Adam8State(n, dev)
    p = p0.clone()
    for t, g in enumerate(grads, start=1):
        hip.adamw8(p, g, st.qm, st.qv, st.absmax_m, st.absmax_v, codes[0], codes[1], hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["wd"], t)
    # the float64 restatement of the same algorithm (scales stored as fp32, as the format has them)
    r = Adam8State(n, dev)
    pr = p0.to(f64)
    for t, g in enumerate(grads, start=1):
        o = ref8.adamw8_f64(pr, g, r.qm, r.qv, r.absmax_m, r.absmax_v, codes[0], codes[1], hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["wd"], t, 1.0)
        pr = o["p"]
        r.qm, r.qv, r.absmax_m, r.absmax_v = o["qm"].to(u8), o["qv"].to(u8), o["absmax_m"].to(f32), o["absmax_v"].to(f32)
    fig_ref = ref.rel_l2(pr - p0.to(f64), want)
    fig = ref.rel_l2(p.to(f64) - p0.to(f64), want)
    print(f"20 steps, n = {n}: displacement vs float64 32-bit AdamW: kernel rel-L2 {fig:.3e}, float64 8-bit restatement {fig_ref:.3e}")
    assert fig_ref > 0 and fig <= 2 * fig_ref


# ---- the trainer on the tiny models -------------------------------------------------------------------------------------------------------------
def _tiny_trainer(dev, bits, ema_decay=None, hyper=False, graph=False):
    from e4t.trainer import E4TTrainer
    n_unet, n_enc, text = _models(dev)
    tr = E4TTrainer(n_unet, n_enc, text, vae=None, lr=1e-3, class_token_id=11, empty_prompt_ids=torch.zeros(1, 9, dtype=torch.long, device=dev), device=dev,
                    ema_decay=ema_decay, optimizer_state_bits=bits)
    if hyper or graph:
        assert tr.enable_step_graph(True)
        tr._step_graph_on = graph              # the eager leg keeps the device-side scalars
    return tr


def _logged_run(tr, batches):
    import tempfile
    from e4t import ops
    hip = ops.HipBackend()
    with tempfile.TemporaryDirectory() as d:
        assert hip.lib.e4t_set_launch_log((d + "/log.txt").encode()) == 0
        try:
            losses, snaps = _run(tr, batches)
        finally:
            hip.lib.e4t_set_launch_log(None)
        names = [ln.split("|")[0] for ln in open(d + "/log.txt").read().splitlines()]
    return losses, snaps, names


def test_trainer_eager_equals_replayed_and_launches_adamw8(hip_env, batches):
    _, _, dev, _ = hip_env
    tr = _tiny_trainer(dev, 8, DECAY)
    assert tr.exp_avg is None and tr.exp_avg_sq is None
    losses, snaps, names = _logged_run(tr, batches)
    assert sum(n == "adamw8_ema_kernel" for n in names) == 5          # once per step: the stack's gradient is materialised and rides the same launch
    assert not any(n in ("adamw_kernel", "adamw_ema_kernel", "adamw8_kernel", "ema_update_kernel") or n.startswith("adamw_rank") for n in names)
    assert not torch.equal(snaps[-1], snaps[0]) and not torch.equal(tr.ema, snaps[-1])
    m, v = tr.adam8.dequantize()
    assert torch.isfinite(m).all() and torch.isfinite(v).all() and bool(m.any()) and bool(v.any())
    for graph in (False, True):          # eager with device scalars; replayed (1 eager warm-up, 1 capture + replay, 3 replays)
        t2 = _tiny_trainer(dev, 8, DECAY, hyper=True, graph=graph)
        l2, s2 = _run(t2, batches)
        assert len(t2._step_graphs) == (1 if graph else 0)
        assert torch.equal(l2, losses)
        assert torch.equal(s2[-1], snaps[-1]), float((s2[-1] - snaps[-1]).abs().max())
        assert all(torch.equal(a, b) for a, b in zip(t2.adam8.buffers(), tr.adam8.buffers()))
        assert torch.equal(t2.ema, tr.ema)


def test_the_default_trainers_launches_are_unchanged(hip_env, batches):
    _, _, dev, _ = hip_env
    tr = _tiny_trainer(dev, 32)
    assert tr.adam8 is None
    _, _, names = _logged_run(tr, batches)
    assert sum(n.startswith("adamw_rank_kernel") for n in names) == 5 and sum(n == "adamw_kernel" for n in names) == 5
    assert not any(n.startswith("adamw8") or n in ("adamw_ema_kernel", "ema_update_kernel") or n.startswith("adamw_rank_ema") for n in names)
