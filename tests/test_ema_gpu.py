"""GPU: the EMA of the trained weights.  The three kernels (adamw_ema_kernel, adamw_rank_ema_kernel, ema_update_kernel) against
the float64 restatement of tests/ema_reference.py, bitwise against their plain siblings and each other, guards; the trainer on the tiny
models: the average only observes, follows the float64 recurrence, survives graph replay, and ema_weights() swaps it in and out."""
import pytest
import torch

import ema_reference as ref
from kernel_checks import STRIDE_TAIL, TOLF, gen, rnd

pytestmark = pytest.mark.gpu
f32, bf16 = torch.float32, torch.bfloat16
HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-2, step=3, grad_scale=0.5)
EMA_W = 0.125 + 1e-3          # not a power of two: the product in the rule rounds
DECAY = 0.9999
RANK_STACKS = ((5, 64, 128, 16), (3, 100, 320, 40), (2, 1280, 1280, 16), (4, 24, 72, 3))      # check_streaming's: (n, rows, cols, K)


def _hyper8(dev, lr, beta1, beta2, step, grad_scale, ema_w):
    bc1, bc2s = ref.bias_corrections(beta1, beta2, step)
    return torch.tensor([lr, bc1, bc2s, grad_scale, ema_w, 0.0, 0.0, 0.0], dtype=f32, device=dev)


def _flat_inputs(n, seed, dev):
    g = gen(seed, dev)
    return (rnd(g, n, dtype=f32, dev=dev), rnd(g, n, dtype=f32, dev=dev), rnd(g, n, dtype=f32, dev=dev) * 0.1, rnd(g, n, dtype=f32, dev=dev).abs() * 0.01,
            rnd(g, n, dtype=f32, dev=dev))


def _check(tag, got, want, tail=None):
    for name, a, b in zip("p m v ema".split(), got, want):
        e = ref.rel_l2(a, b)
        print(f"{tag} {name}: rel-L2 {e:.3e}")
        assert e <= TOLF, (tag, name, e)
        if tail:
            e = ref.rel_l2(a.reshape(-1)[-tail:], b.reshape(-1)[-tail:])
            print(f"{tag} {name}, the last {tail} elements: rel-L2 {e:.3e}")
            assert e <= TOLF, (tag, name, "tail", e)


@pytest.mark.parametrize("n", [1, 5, 100003, 4096 * 1024 + 4 * STRIDE_TAIL + 1], ids=["tail_only", "vector_plus_tail", "n100003", "second_trip"])
def test_adamw_ema_against_float64_and_bitwise(hip_env, n):
    hip, _, dev, _ = hip_env
    p, g, m, v, e = _flat_inputs(n, 480, dev)
    want = ref.adamw_ema_f64(p, g, m, v, e, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], HP["wd"], HP["step"], HP["grad_scale"], EMA_W)
    args = (HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], HP["wd"], HP["step"], HP["grad_scale"])
    p1, m1, v1, e1 = p.clone(), m.clone(), v.clone(), e.clone()
    hip.adamw_ema(p1, g, m1, v1, e1, *args, EMA_W)
    _check(f"adamw_ema n={n}", (p1, m1, v1, e1), want, tail=4 * STRIDE_TAIL + 1 if n > 4096 * 1024 else None)
    # p, m, v: the plain kernel's, bit for bit
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    hip.adamw(p2, g, m2, v2, *args)
    assert torch.equal(p1, p2) and torch.equal(m1, m2) and torch.equal(v1, v2)
    # the average: the rule alone applied to that p (scalar and device-resident weight)
    for w_dev in (None, torch.tensor([EMA_W], dtype=f32, device=dev)):
        e2 = e.clone()
        hip.ema_update(e2, p2, EMA_W if w_dev is None else 0.0, w_dev)
        assert torch.equal(e1, e2)
    err = ref.rel_l2(e2, ref.ema_update_f64(e, p2, EMA_W))
    print(f"ema_update n={n}: rel-L2 {err:.3e}")
    assert err <= TOLF
    # device-resident scalars: the same bits (the scalar arguments they replace are ignored)
    p3, m3, v3, e3 = p.clone(), m.clone(), v.clone(), e.clone()
    hip.adamw_ema(p3, g, m3, v3, e3, 7.0, HP["beta1"], HP["beta2"], HP["eps"], HP["wd"], 0, 9.0, 0.9,
                  hyper=_hyper8(dev, HP["lr"], HP["beta1"], HP["beta2"], HP["step"], HP["grad_scale"], EMA_W))
    assert torch.equal(p1, p3) and torch.equal(m1, m3) and torch.equal(v1, v3) and torch.equal(e1, e3)
    assert not torch.equal(e1, e)


@pytest.mark.parametrize("i", range(4), ids=[f"n{n}_{r}x{c}_K{K}" for n, r, c, K in RANK_STACKS])
def test_adamw_rank_ema_against_float64_and_bitwise(hip_env, i):
    hip, _, dev, _ = hip_env
    n, rows, cols, K = RANK_STACKS[i]
    gg = gen(470 + i, dev)
    P = rnd(gg, n, rows, cols, dtype=f32, dev=dev)
    M = rnd(gg, n, rows, cols, dtype=f32, dev=dev) * 0.1
    V = rnd(gg, n, rows, cols, dtype=f32, dev=dev).abs() * 0.01
    G, Z = rnd(gg, K, rows, dev=dev), rnd(gg, K, n * cols, dev=dev)
    E = rnd(gg, n, rows, cols, dtype=f32, dev=dev)
    args = (HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], HP["wd"], HP["step"], HP["grad_scale"])
    # the second stack runs with device-resident scalars (and other values than the arguments, which must be ignored)
    dev_scalars = dict(lr=2e-3, step=4, grad_scale=0.25, ema_w=0.3) if i == 1 else None
    hyper8 = hyper4 = None
    eff = dict(HP, ema_w=EMA_W)
    if dev_scalars:
        eff.update(dev_scalars)
        hyper8 = _hyper8(dev, eff["lr"], eff["beta1"], eff["beta2"], eff["step"], eff["grad_scale"], eff["ema_w"])
        hyper4 = hyper8[:4].clone()
    want = ref.adamw_rank_ema_f64(P, M, V, E, G, Z, eff["lr"], eff["beta1"], eff["beta2"], eff["eps"], eff["wd"], eff["step"], eff["grad_scale"], eff["ema_w"])
    P1, M1, V1, E1 = P.clone(), M.clone(), V.clone(), E.clone()
    hip.adamw_rank_ema(P1, M1, V1, E1, G, Z, *args, EMA_W, hyper=hyper8)
    _check(f"adamw_rank_ema n{n} {rows}x{cols} K{K}" + (" hyper" if hyper8 is not None else ""), (P1, M1, V1, E1), want)
    P2, M2, V2 = P.clone(), M.clone(), V.clone()
    hip.adamw_rank(P2, M2, V2, G, Z, *args, hyper=hyper4)
    assert torch.equal(P1, P2) and torch.equal(M1, M2) and torch.equal(V1, V2)
    E2 = E.clone()
    hip.ema_update(E2.view(-1), P2.view(-1), eff["ema_w"])
    assert torch.equal(E1, E2)
    # scalar form == device-resident form
    P3, M3, V3, E3 = P.clone(), M.clone(), V.clone(), E.clone()
    if hyper8 is None:
        hip.adamw_rank_ema(P3, M3, V3, E3, G, Z, 7.0, HP["beta1"], HP["beta2"], HP["eps"], HP["wd"], 0, 9.0, 0.9,
                           hyper=_hyper8(dev, HP["lr"], HP["beta1"], HP["beta2"], HP["step"], HP["grad_scale"], EMA_W))
    else:
        hip.adamw_rank_ema(P3, M3, V3, E3, G, Z, eff["lr"], HP["beta1"], HP["beta2"], HP["eps"], HP["wd"], eff["step"], eff["grad_scale"], eff["ema_w"])
    assert torch.equal(P1, P3) and torch.equal(M1, M3) and torch.equal(V1, V3) and torch.equal(E1, E3)


SENT = 0x7FC00ABC          # a quiet NaN with a payload: poison for whoever reads it, a sentinel for whoever writes it


def _guarded(t, guard=64):
    """t inside a buffer of NaN sentinels (guard floats on either side: the 16-byte alignment is kept) -> (view of t's place, the two guards as int32)"""
    buf = torch.full((guard + t.numel() + guard,), SENT, dtype=torch.int32, device=t.device)
    inner = buf[guard:guard + t.numel()].view(f32)
    inner.copy_(t.reshape(-1))
    return inner.view(t.shape), (buf[:guard], buf[guard + t.numel():])


def test_guards_around_the_average(hip_env):
    hip, _, dev, _ = hip_env
    args = (HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], HP["wd"], HP["step"], HP["grad_scale"])
    untouched = lambda guards: all(bool((gd == SENT).all()) for gd in guards)
    for n in (1029, 4096 * 1024 + 4 * STRIDE_TAIL + 1):
        p, g, m, v, e = _flat_inputs(n, 481, dev)
        e_plain, p_plain, m_plain, v_plain = e.clone(), p.clone(), m.clone(), v.clone()
        hip.adamw_ema(p_plain, g, m_plain, v_plain, e_plain, *args, EMA_W)
        eg, guards = _guarded(e)
        pg, pguards = _guarded(p)
        hip.adamw_ema(pg, g, m.clone(), v.clone(), eg, *args, EMA_W)
        assert torch.isfinite(eg).all() and torch.equal(eg, e_plain) and torch.equal(pg, p_plain) and untouched(guards) and untouched(pguards)
        eg, guards = _guarded(e)
        hip.ema_update(eg, p_plain, EMA_W)
        assert torch.isfinite(eg).all() and torch.equal(eg, e_plain) and untouched(guards)
    n, rows, cols, K = RANK_STACKS[3]
    gg = gen(490, dev)
    P, E = rnd(gg, n, rows, cols, dtype=f32, dev=dev), rnd(gg, n, rows, cols, dtype=f32, dev=dev)
    M, V = torch.zeros_like(P), torch.zeros_like(P)
    G, Z = rnd(gg, K, rows, dev=dev), rnd(gg, K, n * cols, dev=dev)
    E_plain = E.clone()
    hip.adamw_rank_ema(P.clone(), M.clone(), V.clone(), E_plain, G, Z, *args, EMA_W)
    Eg, guards = _guarded(E)
    hip.adamw_rank_ema(P.clone(), M.clone(), V.clone(), Eg, G, Z, *args, EMA_W)
    assert torch.isfinite(Eg).all() and torch.equal(Eg, E_plain) and untouched(guards)


def test_bad_average_pointers_are_refused_before_any_launch(hip_env, tmp_path):
    hip, _, dev, ops = hip_env
    n = 4 * 24 * 72          # (every buffer is large enough for every call below, refused or not)
    p, g, m, v, e = _flat_inputs(n + 4, 482, dev)
    before = [t.clone() for t in (p, m, v, e)]
    G, Z = rnd(gen(1, dev), 3, 24, dev=dev), rnd(gen(2, dev), 3, 4 * 72, dev=dev)
    ptr, s = (lambda t: t.data_ptr()), ops._stream()
    log = tmp_path / "launches.txt"
    assert hip.lib.e4t_set_launch_log(str(log).encode()) == 0
    try:
        for bad in (None, ptr(e) + 4):
            assert hip.lib.e4t_adamw_ema(ptr(p), ptr(g), ptr(m), ptr(v), bad, n, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 3, 0.5, EMA_W, None, s) == -22
            assert hip.lib.e4t_adamw_rank_ema(ptr(p), ptr(m), ptr(v), bad, ptr(G), ptr(Z), 4, 24, 72, 3, 24, 4 * 72, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 3, 0.5,
                                              EMA_W, None, s) == -22
            assert hip.lib.e4t_ema_update(bad, ptr(p), n, EMA_W, None, s) == -22
        # the plain entry points' own checks still hold: no parameters, a step of 0 without device scalars, a misaligned hyper buffer
        assert hip.lib.e4t_adamw_ema(None, ptr(g), ptr(m), ptr(v), ptr(e), n, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 3, 0.5, EMA_W, None, s) == -22
        assert hip.lib.e4t_adamw_ema(ptr(p), ptr(g), ptr(m), ptr(v), ptr(e), n, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 0, 0.5, EMA_W, None, s) == -22
        assert hip.lib.e4t_adamw_ema(ptr(p), ptr(g), ptr(m), ptr(v), ptr(e), n, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 3, 0.5, EMA_W, ptr(g) + 4, s) == -22
        assert hip.lib.e4t_ema_update(ptr(e), None, n, EMA_W, None, s) == -22
    finally:
        hip.lib.e4t_set_launch_log(None)
    torch.cuda.synchronize()
    assert log.read_text() == ""                                      # nothing was launched
    assert all(torch.equal(a, b) for a, b in zip(before, (p, m, v, e)))
    # launch-log lines: the new symbols with 36 / 32 / 12 B per parameter
    assert hip.lib.e4t_set_launch_log(str(log).encode()) == 0
    try:
        hip.adamw_ema(p[:n], g[:n], m[:n], v[:n], e[:n], 1e-3, 0.9, 0.999, 1e-8, 1e-2, 3, 0.5, EMA_W)
        hip.ema_update(e[:n], p[:n], EMA_W)
        P = torch.zeros(4, 24, 72, dtype=f32, device=dev)
        hip.adamw_rank_ema(P, P.clone(), P.clone(), P.clone(), G, Z, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 3, 0.5, EMA_W)
    finally:
        hip.lib.e4t_set_launch_log(None)
    lines = [ln.split("|") for ln in log.read_text().splitlines()]
    assert [ln[0] for ln in lines] == ["adamw_ema_kernel", "ema_update_kernel", "adamw_rank_ema_kernel<8>"]
    assert [float(ln[2]) for ln in lines] == [36.0 * n, 12.0 * n, 32.0 * 4 * 24 * 72]


# ---- the trainer on the tiny models -------------------------------------------------------------------------------------------------
def _models(dev):
    from test_train_step_host_logic import TEXT_CFG, build
    from e4t.text import CLIPTextModel
    _, _, n_unet, n_enc, text_t = build(seed=0)
    text = CLIPTextModel(**TEXT_CFG).requires_grad_(False)
    text.load_state_dict(text_t.state_dict())
    n_unet.to(dev), n_enc.to(dev), text.to(dev)
    return n_unet, n_enc, text


def _tiny_trainer(dev, ema_decay, hyper=False, graph=False):
    from e4t.trainer import E4TTrainer
    n_unet, n_enc, text = _models(dev)
    tr = E4TTrainer(n_unet, n_enc, text, vae=None, lr=1e-3, class_token_id=11, empty_prompt_ids=torch.zeros(1, 9, dtype=torch.long, device=dev), device=dev,
                    ema_decay=ema_decay)
    if hyper or graph:
        assert tr.enable_step_graph(True)
        assert tr._hyper.numel() == (8 if ema_decay else 4)
        tr._step_graph_on = graph              # the eager leg keeps the device-side scalars (as test_step_graph_replay_equals_eager does)
    return tr


@pytest.fixture(scope="module")
def batches():
    g = torch.Generator().manual_seed(3)
    B = 2
    return [tuple(t.cuda() for t in (torch.rand(B, 3, 64, 64, generator=g) * 2 - 1, torch.randn(B, 4, 16, 16, generator=g) * 0.18215,
                                     torch.randn(B, 4, 16, 16, generator=g), torch.randint(0, 1000, (B,), generator=g), torch.randint(1, 99, (B, 9), generator=g)))
            for _ in range(6)]


PIDX = [2, 4]


def _run(tr, batches, steps=5):
    pidx = torch.tensor(PIDX, device=tr.device)
    losses, snaps = [], [tr.flat.data.clone()]
    for px, lat, noise, t, ids in batches[:steps]:
        out = tr.train_step(px, ids, pidx, noise=noise, timesteps=t, latents=lat)
        losses.append(torch.stack([o.detach().float() for o in out]))
        snaps.append(tr.flat.data.clone())
    torch.cuda.synchronize()
    return torch.stack(losses), snaps


@pytest.fixture(scope="module")
def eager_run(batches):
    """five eager steps with ema_decay = 0.9999, launches logged: shared by the tests below, left unchanged"""
    import tempfile
    from e4t import ops
    dev = torch.device("cuda:0")
    hip = ops.HipBackend()
    tr = _tiny_trainer(dev, DECAY)
    with tempfile.TemporaryDirectory() as d:
        assert hip.lib.e4t_set_launch_log((d + "/log.txt").encode()) == 0
        try:
            losses, snaps = _run(tr, batches)
        finally:
            hip.lib.e4t_set_launch_log(None)
        log = open(d + "/log.txt").read().splitlines()
    return dict(tr=tr, losses=losses, snaps=snaps, log=log, ema=tr.ema.clone(), m=tr.exp_avg.clone(), v=tr.exp_avg_sq.clone())


def test_the_average_only_observes(hip_env, batches, eager_run):
    _, _, dev, _ = hip_env
    off = _tiny_trainer(dev, None)
    assert off.ema is None and set(off.state_dict()) == {"params", "exp_avg", "exp_avg_sq", "step_count", "lr"}
    losses, snaps = _run(off, batches)
    assert torch.equal(losses, eager_run["losses"])
    assert all(torch.equal(a, b) for a, b in zip(snaps, eager_run["snaps"]))
    assert torch.equal(off.exp_avg, eager_run["m"]) and torch.equal(off.exp_avg_sq, eager_run["v"])


def test_the_average_follows_the_float64_recurrence(hip_env, eager_run):
    from e4t.optimization import ema_weight
    assert len({ema_weight(DECAY, t) for t in range(1, 6)}) == 5          # five steps, five weights: a stale scalar shows
    err = ref.rel_l2(eager_run["ema"], ref.ema_trajectory(eager_run["snaps"], DECAY))
    print(f"ema after 5 steps vs the float64 trajectory: rel-L2 {err:.3e}")
    assert err <= TOLF
    assert not torch.equal(eager_run["ema"], eager_run["snaps"][-1]) and not torch.equal(eager_run["ema"], eager_run["snaps"][0])


def test_the_factored_head_update_is_kept(hip_env, eager_run):
    names = [ln.split("|")[0] for ln in eager_run["log"]]
    assert sum(n.startswith("adamw_rank_ema_kernel") for n in names) == 5            # once per step
    assert sum(n == "adamw_ema_kernel" for n in names) == 5
    assert not any(n.startswith("adamw_rank_kernel") or n in ("adamw_kernel", "ema_update_kernel") for n in names)


def test_step_graph_replay_equals_eager(hip_env, batches, eager_run):
    """eager with host scalars (the shared run), eager with device scalars, and replayed (1 eager warm-up, 1 capture + replay, 3 replays):
    parameters and average after five steps are the same bits"""
    _, _, dev, _ = hip_env
    for graph in (False, True):
        tr = _tiny_trainer(dev, DECAY, hyper=True, graph=graph)
        losses, snaps = _run(tr, batches)
        assert len(tr._step_graphs) == (1 if graph else 0)
        assert torch.equal(losses, eager_run["losses"])
        assert torch.equal(snaps[-1], eager_run["snaps"][-1]), float((snaps[-1] - eager_run["snaps"][-1]).abs().max())
        assert torch.equal(tr.ema, eager_run["ema"]), float((tr.ema - eager_run["ema"]).abs().max())
        assert tr._hyper.tolist()[5:] == [0.0, 0.0, 0.0]


def test_ema_weights_swaps_in_and_out(hip_env, batches):
    from e4t.trainer import E4TTrainer
    _, _, dev, _ = hip_env
    tr, twin = _tiny_trainer(dev, DECAY), _tiny_trainer(dev, DECAY)
    for t in (tr, twin):
        _run(t, batches, steps=2)
    raw, avg = tr.flat.data.clone(), tr.ema.clone()
    px, lat, noise, t, ids = batches[2]
    pidx = torch.tensor(PIDX, device=dev)
    with torch.no_grad():
        l_raw = torch.stack(tr.losses(px, lat, noise, t, ids, pidx))
        with tr.ema_weights():
            assert torch.equal(tr.flat.data, avg)
            l_avg = torch.stack(tr.losses(px, lat, noise, t, ids, pidx))
        l_back = torch.stack(tr.losses(px, lat, noise, t, ids, pidx))
    assert torch.equal(tr.flat.data, raw) and torch.equal(tr.ema, avg)
    assert torch.equal(l_raw, l_back) and not torch.equal(l_raw, l_avg)          # no stale compute copy either way
    # a trainer built from the averaged values
    other = _tiny_trainer(dev, None)
    other.flat.data.copy_(avg)
    from e4t import ops
    ops.bump_weights_epoch()
    with torch.no_grad():
        l_other = torch.stack(other.losses(px, lat, noise, t, ids, pidx))
    assert torch.equal(l_avg, l_other), (l_avg, l_other)
    # the next step equals the untouched twin's
    out, out_twin = _run(tr, batches[2:], steps=1), _run(twin, batches[2:], steps=1)
    assert torch.equal(out[0], out_twin[0]) and torch.equal(tr.flat.data, twin.flat.data) and torch.equal(tr.ema, twin.ema)
    # refusals: pending micro-batch gradients, an announced prefetch
    tr.train_step(px, ids, pidx, noise=noise, timesteps=t, latents=lat, sync=False, loss_scale=0.5)
    with pytest.raises(RuntimeError, match="micro-batch"):
        with tr.ema_weights():
            pass
    tr.train_step(px, ids, pidx, noise=noise, timesteps=t, latents=lat, sync=True, loss_scale=0.5)
    twin.prefetch(batches[3][0])
    if twin._next_px is not None or twin._pref:           # (a trainer without frozen front ends to prefetch announces nothing)
        with pytest.raises(RuntimeError, match="prefetch"):
            with twin.ema_weights():
                pass


def test_pipeline_samples_from_the_average_inside_the_context(hip_env, batches):
    """2 DDIM steps inside and outside ema_weights(): different latents, each the latents of a pipeline BUILT on the respective weights"""
    from word_tokenizer import WordTokenizer
    from e4t import ops
    from e4t.pipeline_stable_diffusion_e4t import StableDiffusionE4TPipeline
    from e4t.schedulers import DDIMScheduler
    from e4t.vae import VAEDecoder
    _, _, dev, _ = hip_env
    tr = _tiny_trainer(dev, DECAY)
    _run(tr, batches, steps=2)
    torch.manual_seed(0)
    vae = VAEDecoder(block_out_channels=(64, 64)).requires_grad_(False)
    cfg = dict(placeholder_token="*s", domain_class_token="art", domain_embed_scale=0.1)

    tok, text = WordTokenizer(), tr.text_encoder          # (frozen, shared: the first pipeline adds the placeholder token to both)

    def pipeline(unet, enc, first=False):
        return StableDiffusionE4TPipeline(vae=vae, text_encoder=text, tokenizer=tok, unet=unet, e4t_encoder=enc, scheduler=DDIMScheduler.stable_diffusion(),
                                          safety_checker=None, e4t_config=dict(cfg), already_added_placeholder_token=not first).to(dev)
    g = torch.Generator().manual_seed(5)
    image = torch.rand(1, 3, 64, 64, generator=g) * 2 - 1
    lat0 = torch.randn(1, 4, 16, 16, generator=g)
    kw = dict(height=32, width=32, num_inference_steps=2, guidance_scale=5.0, num_images_per_prompt=1, image=image, output_type="latent", use_graph=False)
    sample = lambda pipe: pipe("a painting of *s", latents=lat0.clone(), **kw).images
    states = {"raw": (tr.unet.state_dict(), tr.encoder.state_dict())}
    states["raw"] = tuple({k: v.detach().clone() for k, v in sd.items()} for sd in states["raw"])
    pipe = pipeline(tr.unet, tr.encoder, first=True)
    was = tr.unet.training
    out = {"raw": sample(pipe)}
    with tr.ema_weights():
        states["ema"] = tuple({k: v.detach().clone() for k, v in sd.items()} for sd in (tr.unet.state_dict(), tr.encoder.state_dict()))
        out["ema"] = sample(pipe)
    assert torch.equal(sample(pipe), out["raw"])                     # back outside: the raw weights' latents again
    tr.unet.train(was)
    assert torch.isfinite(out["raw"]).all() and torch.isfinite(out["ema"]).all() and not torch.equal(out["raw"], out["ema"])
    for which in ("raw", "ema"):
        unet, enc, _ = _models(dev)
        unet.load_state_dict(states[which][0])
        enc.load_state_dict(states[which][1])
        ops.bump_weights_epoch()
        built = sample(pipeline(unet, enc))
        assert torch.equal(built, out[which]), (which, float((built - out[which]).abs().max()))
