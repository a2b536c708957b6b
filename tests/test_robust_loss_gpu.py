"""-m gpu: the scheduled pseudo-Huber / smooth-L1 loss on the real kernels — e4t_robust_loss_fwd (+ e4t_masked_mse_bwd)
against the float64 restatement of the definition (rel-L2 <= 2e-5, the project's fp32-kernel bound), the saved buffer, run-to-run and
layout facts, the clamp, the c -> inf limit against the weighted loss, the neighbours' results unchanged, the forward replayed from a
graph with new timesteps, one Huber training step against the same step on the torch composition, and the whole Huber step replayed
from the step graph."""
import pytest
import torch

from test_masked_loss_host_logic import BOUND, make_mask, rel, restate64
from test_objective_host_logic import GAMMA, lam_for, operands, timestep_sets, timesteps_for, weighted64
from test_objective_gpu import _pred, _tiny_trainer, tables
from test_robust_loss_host_logic import C_TABLES, KINDS, RL_SHAPES, T, ctab_for, robust64, wd64

pytestmark = pytest.mark.gpu

GPU_SHAPES = RL_SHAPES + [(2, 4, 64, 64), (16, 4, 64, 64)]        # the last one fills more than one block per stage (1024 pixels per 4 blocks)
ids_shape = lambda s: "x".join(map(str, s))


# ---------------------------------------------------------------------------------------------- 6. the kernels
@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", GPU_SHAPES, ids=ids_shape)
def test_robust_loss_kernels(hip_env, shape, kind, nhwc):
    from e4t import functional as Fn
    hip, emu, dev, ops = hip_env
    assert ops.backend().name == "hip" and hasattr(ops.backend(), "robust_loss")
    B, C, h, w = shape
    acp, coef = tables(dev, False)
    x = operands(shape)
    target = x["noise"].to(dev)
    worst = [0.0, 0.0]
    for cname in C_TABLES:
        ctab = ctab_for(cname, acp.cpu()).to(dev)
        for mask in ("none", "soft", "ones", "zero"):
            m = None if mask == "none" else make_mask(mask, B, h, w, x["g"]).to(dev)
            for lam_kind in ("none", "mixed"):
                for t in timestep_sets(B):
                    t = t.to(dev)
                    lam = lam_for(lam_kind, t, coef)
                    base, pred = _pred(shape, nhwc, dev)
                    loss = Fn.robust_loss(pred, target, ctab, t, kind, lam, m)
                    assert loss.dtype == torch.float32 and loss.dim() == 0
                    (loss * 3.0).backward()                           # an upstream gradient other than 1
                    dpred = base.grad.permute(0, 3, 1, 2) if nhwc else base.grad
                    if mask == "zero":
                        assert float(loss.detach()) == 0.0 and float(dpred.abs().max()) == 0.0
                        continue
                    want, dwant = robust64(pred, target, ctab, t, kind, lam, m)
                    r_loss, r_grad = rel(loss.detach().cpu(), want), rel(dpred.cpu(), 3.0 * dwant)
                    worst = [max(worst[0], r_loss), max(worst[1], r_grad)]
                    assert r_loss <= BOUND and r_grad <= BOUND, (cname, mask, lam_kind, t.tolist()[:4], r_loss, r_grad)
    print(f"robust_loss {shape} {kind} nhwc={nhwc}: worst rel loss {worst[0]:.3e} dpred {worst[1]:.3e}")
    # run to run: bitwise; the gradient comes back in pred's own layout; the saved buffer is lam_b * w * (k / 2) * d / r
    base, pred = _pred(shape, nhwc, dev, seed=1)
    m = make_mask("soft", B, h, w, x["g"]).to(dev)
    t = timesteps_for(B).to(dev)
    lam = lam_for("mixed", t, coef)
    ctab = ctab_for("snr", acp.cpu()).to(dev)
    g = torch.full((), 0.5, device=dev)
    runs = []
    for _ in range(2):
        loss, wd, stats = hip.robust_loss(pred.detach(), target, ctab, t, kind, lam, m)
        dp = hip.robust_loss_bwd(wd, stats, g)
        assert dp.shape == pred.shape and (pred.is_contiguous() or (dp.stride() == pred.stride() and wd.stride() == pred.stride()))
        runs.append((loss.clone(), dp.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert rel(wd.cpu(), wd64(pred, target, ctab, t, kind, lam, m)) <= BOUND
    assert hip.robust_loss(pred.detach(), target, ctab, t, kind, lam, m, save=False)[1] is None


@pytest.mark.parametrize("kind", KINDS)
def test_robust_loss_clamp_none_zero_residual_and_bad_kind(hip_env, kind):
    from e4t import _C
    hip, emu, dev, ops = hip_env
    shape = (2, 4, 5, 7)
    acp, _ = tables(dev, False)
    ctab = ctab_for("snr", acp.cpu()).to(dev)
    x = operands(shape)
    _, pred = _pred(shape, True, dev)
    pred, target = pred.detach(), x["noise"].to(dev)
    g = torch.ones((), device=dev)

    def both(t):
        loss, wd, stats = hip.robust_loss(pred, target, ctab, t, kind)
        return loss.clone(), hip.robust_loss_bwd(wd, stats, g)

    got, want = both(torch.tensor([-5, 2000], device=dev)), both(torch.tensor([0, 999], device=dev))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    none, first = both(None), both(torch.tensor([0, 0], device=dev))
    assert torch.equal(none[0], first[0]) and torch.equal(none[1], first[1]) and not torch.equal(none[0], got[0])
    r64 = robust64(pred, target, ctab, None, kind, None, None)
    assert rel(none[0].cpu(), r64[0]) <= BOUND and rel(none[1].cpu(), r64[1]) <= BOUND
    loss, wd, stats = hip.robust_loss(target.clone(), target, ctab, None, kind)          # d == 0
    assert float(loss) == 0.0 and float(wd.abs().max()) == 0.0
    for bad in (0, 3, -1):
        with pytest.raises(_C.E4TError, match="kind"):
            hip.robust_loss(pred, target, ctab, None, bad)


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
def test_huber_with_a_huge_c_is_the_weighted_mse(hip_env, nhwc):
    from e4t import functional as Fn
    hip, emu, dev, ops = hip_env
    shape = (3, 4, 5, 7)
    B, C, h, w = shape
    _, coef = tables(dev, False)
    x = operands(shape)
    target = x["noise"].to(dev)
    ctab = torch.full((T,), 1e4, device=dev)
    t = timesteps_for(B).to(dev)
    for m in (None, make_mask("soft", B, h, w, x["g"]).to(dev)):
        for lam in (None, lam_for("mixed", t, coef)):
            (ba, pa), (bb, pb) = _pred(shape, nhwc, dev), _pred(shape, nhwc, dev)
            a, b = Fn.robust_loss(pa, target, ctab, t, "huber", lam, m), Fn.weighted_mse(pb, target, lam, m)
            a.backward(), b.backward()
            assert rel(a.detach().cpu(), b.detach().cpu()) <= BOUND and rel(ba.grad.cpu(), bb.grad.cpu()) <= BOUND


def test_the_neighbours_results_are_unchanged(hip_env):
    """e4t_weighted_mse_fwd / e4t_masked_mse_fwd keep their kernels: their float64 bound and run-to-run equality on a fixed input"""
    hip, emu, dev, ops = hip_env
    shape = (16, 4, 64, 64)
    B, C, h, w = shape
    _, coef = tables(dev, False)
    x = operands(shape)
    target = x["noise"].to(dev)
    m = make_mask("soft", B, h, w, x["g"]).to(dev)
    lam = lam_for("mixed", timesteps_for(B).to(dev), coef)
    g = torch.full((), 3.0, device=dev)
    for nhwc in (False, True):
        _, pred = _pred(shape, nhwc, dev)
        pred = pred.detach()
        for name, call, want in (("weighted", lambda: hip.weighted_mse(pred, target, lam, m), weighted64(pred, target, lam, m)),
                                 ("masked", lambda: hip.masked_mse(pred, target, m), restate64(pred.cpu(), target.cpu(), m.cpu()))):
            runs = []
            for _ in range(2):
                loss, wd, stats = call()
                runs.append((loss.clone(), hip.masked_mse_bwd(wd, stats, g)))
            assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
            assert rel(runs[0][0].cpu(), want[0]) <= BOUND and rel(runs[0][1].cpu(), 3.0 * want[1]) <= BOUND, name


# ---------------------------------------------------------------------------------------------- 7. graph replay of the forward
def test_robust_forward_replays_from_a_graph_with_new_timesteps(hip_env):
    hip, emu, dev, ops = hip_env
    shape = (3, 4, 5, 7)
    acp, coef = tables(dev, False)
    ctab = ctab_for("snr", acp.cpu()).to(dev)
    _, pred = _pred(shape, True, dev, seed=2)
    pred = pred.detach()
    target = torch.randn(shape, generator=torch.Generator().manual_seed(5)).to(dev)
    m = make_mask("soft", 3, 5, 7, torch.Generator().manual_seed(6)).to(dev)
    t = torch.tensor([0, 10, 500], device=dev)
    lam = coef[t, 2].clone()

    def forward():
        loss, wd, stats = hip.robust_loss(pred, target, ctab, t, "huber", lam, m)
        return loss, wd

    eager = [o.clone() for o in forward()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with ops.capture_guard():
        with torch.cuda.graph(graph):
            outs = forward()
    for o in outs:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, eager))
    seen = {float(eager[0])}
    for new in ([999, 147, 3], [-4, 5000, 250], [600, 600, 1]):        # nothing was read on the host or baked in: the replay gathers the new c
        t.copy_(torch.tensor(new, device=dev))
        graph.replay()
        fresh = forward()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(outs, fresh))
        seen.add(float(outs[0]))
    assert len(seen) == 4


# ---------------------------------------------------------------------------------------------- 8. one Huber training step
def test_huber_training_step_against_the_composition(hip_env, monkeypatch):
    """loss_type="huber" with snr_gamma and a mask: the step on the kernels against the same step with the backend's robust_loss hidden
    (functional.robust_loss then runs its torch composition).  The forward is the same launches, so pred is the same bits; loss_diff of
    either leg lies within BOUND of the float64 restatement on that pred; each leg repeats bit for bit.  The two legs' dpred differ by
    fp32 rounding, which the bf16 backward can only turn into isolated one-ulp flips of bf16 values, so the flat gradients agree to well
    within one bf16 ulp (2^-8) in rel-L2."""
    from e4t import functional as Fn
    hip, emu, dev, ops = hip_env
    g = torch.Generator().manual_seed(3)
    B = 2
    b = dict(px=torch.rand(B, 3, 64, 64, generator=g) * 2 - 1, lat=torch.randn(B, 4, 16, 16, generator=g) * 0.18215,
             noise=torch.randn(B, 4, 16, 16, generator=g), ids=torch.randint(1, 99, (B, 9), generator=g), mask=torch.rand(B, 16, 16, generator=g),
             t=torch.tensor([10, 500]))
    b = {k: v.to(dev) for k, v in b.items()}
    pidx = torch.tensor([2, 4], device=dev)
    seen, paths = [], []
    orig = Fn.robust_loss

    def recording(pred, target, ctab, t, kind, lam=None, w=None):
        seen.append((pred.detach().clone(), target.detach().clone(), ctab, t, kind, lam.clone(), w))
        loss = orig(pred, target, ctab, t, kind, lam, w)
        paths.append(type(loss.grad_fn).__name__)
        return loss

    monkeypatch.setattr(Fn, "robust_loss", recording)

    def leg():
        runs = []
        for _ in range(2):
            tr0, tr = (_tiny_trainer(dev, loss_type="huber", snr_gamma=GAMMA) for _ in range(2))
            out = tr0.losses(b["px"], b["lat"], b["noise"], b["t"], b["ids"], pidx, loss_mask=b["mask"])
            out[0].backward()
            grad = tr0.flat.grad.detach().clone()
            step = tr.train_step(b["px"], b["ids"], pidx, noise=b["noise"], timesteps=b["t"], latents=b["lat"], loss_mask=b["mask"])
            torch.cuda.synchronize()
            runs.append((torch.stack([o.detach().float() for o in out]).cpu(), grad.cpu(), torch.stack([o.detach().float() for o in step]).cpu(),
                         tr.flat.data.detach().cpu().clone()))
        for a, c in zip(runs[0], runs[1]):
            assert torch.equal(a, c)
        return runs[0], tr

    kern, tr = leg()
    assert len(seen) == 4
    with monkeypatch.context() as mp:
        mp.delattr(type(ops.backend()), "robust_loss")
        assert not hasattr(ops.backend(), "robust_loss")
        comp, _ = leg()
    assert hasattr(ops.backend(), "robust_loss") and len(seen) == 8
    assert all(p == "RobustLossFnBackward" for p in paths[:4]) and not any(p == "RobustLossFnBackward" for p in paths[4:])
    pred, target, ctab, t, kind, lam, w = seen[0]
    assert torch.equal(pred, seen[4][0]) and torch.equal(target, seen[4][1])           # the same forward in both legs
    assert ctab is not None and kind == "huber" and w is b["mask"] and torch.equal(t, b["t"])
    assert float(lam[0]) < 1.0 and float(lam[1]) == 1.0                  # t = 10 is clamped by gamma = 5, t = 500 is not
    want = robust64(pred, target, tr.huber_tab, b["t"], "huber", lam, b["mask"])[0]
    r_k, r_c, r_kc = rel(kern[0][1], want), rel(comp[0][1], want), rel(kern[0][1], comp[0][1])
    r_g, r_p = rel(kern[1], comp[1]), rel(kern[3], comp[3])
    print(f"huber step loss_diff kernels {float(kern[0][1]):.6f} composition {float(comp[0][1]):.6f} float64 {float(want):.6f}: rel {r_k:.3e} "
          f"{r_c:.3e}, legs {r_kc:.3e}; flat gradient rel {r_g:.3e}, parameters after the step rel {r_p:.3e}")
    assert r_k <= BOUND and r_c <= BOUND and r_kc <= BOUND
    assert float(kern[1].abs().max()) > 0 and r_g <= 2.0 ** -8 and r_p <= BOUND
    # the loss matters: the squared error of the same prediction is another number
    assert abs(float(weighted64(pred, target, lam, b["mask"])[0]) - float(kern[0][1])) > 1e-3 * float(kern[0][1])


# ---------------------------------------------------------------------------------------------- 9. the step graph
@pytest.mark.parametrize("mode", ["inputs_given", "masked"])
def test_huber_step_graph_replay_equals_eager(hip_env, mode):
    """the whole Huber step (with snr_gamma and noise_offset) captured and replayed: four steps with different timesteps, losses and every
    trained parameter equal to the eager run bit for bit, one graph; with a loss mask the step runs eagerly and no graph exists"""
    from e4t.vae import VAEEncoder
    hip, emu, dev, ops = hip_env
    g = torch.Generator().manual_seed(9)
    B = 2
    batches = [dict(px=torch.rand(B, 3, 128, 128, generator=g) * 2 - 1, noise=torch.randn(B, 4, 16, 16, generator=g), ids=torch.randint(1, 99, (B, 9), generator=g),
                    z=torch.randn(B, 4, generator=g), mask=torch.rand(B, 16, 16, generator=g)) for _ in range(4)]
    for b, t in zip(batches, ([0, 500], [10, 999], [146, 147], [700, 3])):
        b["t"] = torch.tensor(t)
    batches = [{k: v.to(dev) for k, v in b.items()} for b in batches]
    pidx = torch.tensor([2, 4], device=dev)

    def run(graph, **kw_tr):
        torch.manual_seed(11)
        vae = VAEEncoder(block_out_channels=(64, 128, 128, 128)).requires_grad_(False).to(dev)
        tr = _tiny_trainer(dev, vae=vae, snr_gamma=GAMMA, noise_offset=0.1, **kw_tr)
        assert tr.enable_step_graph(True)
        tr._step_graph_on = graph                  # the eager leg keeps the device-side AdamW scalars, launches from the host
        torch.manual_seed(5)
        losses = []
        for b in batches:
            kw = dict(noise=b["noise"], timesteps=b["t"], offset_eps=b["z"])
            if mode == "masked":
                kw["loss_mask"] = b["mask"]
            out = tr.train_step(b["px"], b["ids"], pidx, **kw)
            losses.append(torch.stack([o.detach().float() for o in out]).cpu())
        torch.cuda.synchronize()
        return torch.stack(losses), tr.flat.data.detach().cpu().clone(), len(tr._step_graphs)

    l0, p0, n0 = run(False, loss_type="huber")
    l1, p1, n1 = run(True, loss_type="huber")
    assert n0 == 0 and n1 == (0 if mode == "masked" else 1)
    assert torch.equal(l0, l1), (l0, l1)
    assert torch.equal(p0, p1), float((p0 - p1).abs().max())
    assert len({float(x) for x in l0[:, 1]}) == 4
    if mode == "inputs_given":                     # and it is another loss than the squared error's
        assert not torch.equal(l0[:, 1], run(False)[0][:, 1])
