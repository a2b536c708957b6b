"""-m gpu: min-SNR-gamma loss weighting and the noise offset on the real kernels — e4t_diffuse against the torch
composition it replaces, bit for bit; e4t_weighted_mse_fwd (+ e4t_masked_mse_bwd) against a float64 restatement (rel-L2 <= 2e-5, the
project's fp32-kernel bound); the forward replayed from a graph with new timesteps; one weighted training step at the tiny model sizes;
and the whole step with both options replayed from the step graph."""
import pytest
import torch

from test_masked_loss_host_logic import BOUND, make_mask, rel
from test_objective_host_logic import GAMMA, OBJ_SHAPES, lam_for, objective64, operands, timestep_sets, timesteps_for, weighted64

pytestmark = pytest.mark.gpu

ids_shape = lambda s: "x".join(map(str, s))


def ulps(a, b):
    """largest distance between two fp32 tensors in units in the last place (ordered-integer view)"""
    def key(x):
        i = x.contiguous().view(torch.int32).long()
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int((key(a) - key(b)).abs().max())


def torch_objective(x0, noise, t, acp, z, s, v_prediction):
    """the stock-torch ops of the definitions on x0's device: for s = 0 the trainer's add_noise and target lines"""
    B = x0.shape[0]
    a = acp[t].sqrt().view(-1, 1, 1, 1)
    sg = (1 - acp[t]).sqrt().view(-1, 1, 1, 1)
    n1 = noise + (s * z).view(B, -1, 1, 1) if s else noise
    return a * x0 + sg * n1, (a * n1 - sg * x0) if v_prediction else n1


def tables(dev, v_prediction, gamma=GAMMA):
    from e4t.trainer import ddpm_alphas_cumprod, objective_coef
    acp = ddpm_alphas_cumprod(device=dev)
    return acp, objective_coef(acp, gamma, v_prediction)


# ---------------------------------------------------------------------------------------------- 6. e4t_diffuse
@pytest.mark.parametrize("s", [0.0, 0.1])
@pytest.mark.parametrize("v_prediction", [False, True], ids=["epsilon", "v_prediction"])
@pytest.mark.parametrize("shape", OBJ_SHAPES, ids=ids_shape)
def test_diffuse_is_the_torch_composition_bitwise(hip_env, shape, v_prediction, s):
    hip, emu, dev, ops = hip_env
    acp, coef = tables(dev, v_prediction)
    x = {k: v.to(dev) for k, v in operands(shape).items() if k != "g"}
    for t in timestep_sets(shape[0]):
        t = t.to(dev)
        noisy, target, lam = hip.diffuse(x["x0"], x["noise"], t, coef, z=x["z"] if s else None, offset=s, v_prediction=v_prediction)
        w_noisy, w_target = torch_objective(x["x0"], x["noise"], t, acp, x["z"], s, v_prediction)
        assert noisy.shape == target.shape == shape and lam.shape == (shape[0],)
        for name, got, want in (("noisy", noisy, w_noisy), ("target", target, w_target), ("lam", lam, coef[t, 2])):
            if not torch.equal(got, want):
                print(f"e4t_diffuse {shape} v={v_prediction} s={s} t={t.tolist()[:4]}: {name} differs by up to {ulps(got, want)} ulp")
        assert torch.equal(noisy, w_noisy) and torch.equal(target, w_target) and torch.equal(lam, coef[t, 2])
        # and against the float64 restatement
        r_noisy, r_target, r_lam = objective64(x["x0"], x["noise"], t, acp, x["z"], s, v_prediction, GAMMA)
        assert rel(noisy.cpu(), r_noisy) <= BOUND and rel(target.cpu(), r_target) <= BOUND and rel(lam.cpu(), r_lam) <= BOUND
        # offset 0 with a z handed in: no offset term at all
        if not s:
            again = hip.diffuse(x["x0"], x["noise"], t, coef, z=x["z"], offset=0.0, v_prediction=v_prediction)
            assert all(torch.equal(a, b) for a, b in zip(again, (noisy, target, lam)))
    if shape[0] >= 4 and not v_prediction:                      # images on both sides of the clamp
        lam = coef[timesteps_for(shape[0]).to(dev), 2]
        assert bool((lam < 1).any()) and bool((lam == 1).any())


def test_diffuse_clamps_a_timestep_outside_the_table(hip_env):
    hip, emu, dev, ops = hip_env
    acp, coef = tables(dev, True)
    x = {k: v.to(dev) for k, v in operands((2, 4, 5, 7)).items() if k != "g"}
    got = hip.diffuse(x["x0"], x["noise"], torch.tensor([-5, 2000], device=dev), coef, z=x["z"], offset=0.1, v_prediction=True)
    want = hip.diffuse(x["x0"], x["noise"], torch.tensor([0, 999], device=dev), coef, z=x["z"], offset=0.1, v_prediction=True)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    from e4t import _C
    with pytest.raises(_C.E4TError, match="needs z"):
        hip.diffuse(x["x0"], x["noise"], torch.tensor([0, 999], device=dev), coef, z=None, offset=0.1)


# ---------------------------------------------------------------------------------------------- 7. the weighted loss
def _pred(shape, nhwc, dev, seed=0):
    B, C, h, w = shape
    g = torch.Generator().manual_seed(seed + 17 * B + w)
    base = torch.randn((B, h, w, C) if nhwc else shape, generator=g).to(dev).requires_grad_(True)
    return base, (base.permute(0, 3, 1, 2) if nhwc else base)


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("shape", OBJ_SHAPES, ids=ids_shape)
def test_weighted_mse_kernels(hip_env, shape, nhwc):
    from e4t import functional as Fn
    hip, emu, dev, ops = hip_env
    assert ops.backend().name == "hip"
    B, C, h, w = shape
    _, coef = tables(dev, False)
    x = operands(shape)
    target = x["noise"].to(dev)
    for kind in ("none", "soft", "ones", "zero"):
        m = None if kind == "none" else make_mask(kind, B, h, w, x["g"]).to(dev)
        for lam_kind in ("mixed", "ones"):
            for t in timestep_sets(B):
                lam = lam_for(lam_kind, t.to(dev), coef).to(dev)
                base, pred = _pred(shape, nhwc, dev)
                loss = Fn.weighted_mse(pred, target, lam, m)
                assert loss.dtype == torch.float32 and loss.dim() == 0
                (loss * 3.0).backward()                               # an upstream gradient other than 1
                dpred = base.grad.permute(0, 3, 1, 2) if nhwc else base.grad
                want, dwant = weighted64(pred, target, lam, m)
                if kind == "zero":
                    assert float(loss.detach()) == 0.0 and float(dpred.abs().max()) == 0.0
                    continue
                r_loss, r_grad = rel(loss.detach().cpu(), want), rel(dpred.cpu(), 3.0 * dwant)
                print(f"weighted_mse {shape} nhwc={nhwc} mask={kind} lam={lam_kind}: rel loss {r_loss:.3e} dpred {r_grad:.3e}")
                assert r_loss <= BOUND and r_grad <= BOUND
                if lam_kind == "ones":                                # the masked loss / the plain mean
                    plain = torch.nn.functional.mse_loss(pred.detach(), target) if m is None else Fn.masked_mse(pred.detach(), target, m)
                    assert rel(loss.detach().cpu(), plain.cpu()) <= BOUND
                    assert rel(Fn.weighted_mse(pred.detach(), target, None, m).cpu(), plain.cpu()) <= BOUND
    if B >= 4:
        lam = lam_for("mixed", timesteps_for(B).to(dev), coef)
        assert bool((lam < 1).any()) and bool((lam == 1).any())
    # run to run: bitwise; the gradient comes back in pred's own layout
    base, pred = _pred(shape, nhwc, dev, seed=1)
    m = make_mask("soft", B, h, w, x["g"]).to(dev)
    lam = lam_for("mixed", timesteps_for(B).to(dev), coef)
    g = torch.full((), 0.5, device=dev)
    runs = []
    for _ in range(2):
        loss, wd, stats = hip.weighted_mse(pred.detach(), target, lam, m)
        dp = hip.weighted_mse_bwd(wd, stats, g)
        assert dp.shape == pred.shape and (pred.is_contiguous() or (dp.stride() == pred.stride() and wd.stride() == pred.stride()))
        runs.append((loss.clone(), dp.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    # the saved buffer is lam_b * w * d
    want_wd = lam.double().cpu().view(B, 1, 1, 1) * m.double().cpu().unsqueeze(1) * (pred.detach().double().cpu() - target.double().cpu())
    assert rel(wd.cpu(), want_wd) <= BOUND


# ---------------------------------------------------------------------------------------------- 8. graph replay of the forward
def test_objective_forward_replays_from_a_graph(hip_env):
    hip, emu, dev, ops = hip_env
    shape = (3, 4, 5, 7)
    _, coef = tables(dev, True)
    x = {k: v.to(dev) for k, v in operands(shape, seed=2).items() if k != "g"}
    base, pred = _pred(shape, True, dev, seed=2)
    pred = pred.detach()
    target_in = torch.randn(shape, generator=torch.Generator().manual_seed(5)).to(dev)
    m = make_mask("soft", 3, 5, 7, torch.Generator().manual_seed(6)).to(dev)
    t = torch.tensor([0, 10, 500], device=dev)
    z = x["z"].clone()

    def forward():
        noisy, target, lam = hip.diffuse(x["x0"], x["noise"], t, coef, z=z, offset=0.1, v_prediction=True)
        loss, wd, stats = hip.weighted_mse(pred, target_in, lam, m)
        return noisy, target, lam, loss, wd

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
    # new values in the captured buffers, same graph: nothing was read on the host or baked in
    t.copy_(torch.tensor([999, 147, 3], device=dev))
    target_in.mul_(0.5)
    z.copy_(torch.randn(3, 4, generator=torch.Generator().manual_seed(8)).to(dev))
    graph.replay()
    fresh = forward()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, fresh))
    assert not torch.equal(outs[2], eager[2]) and not torch.equal(outs[3], eager[3])


# ---------------------------------------------------------------------------------------------- 9. one weighted training step
def _tiny_trainer(dev, vae=None, **kw):
    from test_train_step_host_logic import TEXT_CFG, build
    from e4t.text import CLIPTextModel
    from e4t.trainer import E4TTrainer
    _, _, n_unet, n_enc, text_t = build(seed=0)
    text = CLIPTextModel(**TEXT_CFG).requires_grad_(False)
    text.load_state_dict(text_t.state_dict())
    n_unet.to(dev), n_enc.to(dev), text.to(dev)
    return E4TTrainer(n_unet, n_enc, text, vae=vae, lr=1e-3, class_token_id=11, empty_prompt_ids=torch.zeros(1, 9, dtype=torch.long, device=dev),
                      device=dev, **kw)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "soft_mask"])
def test_weighted_training_step(hip_env, monkeypatch, masked):
    from e4t import functional as Fn
    hip, emu, dev, ops = hip_env
    g = torch.Generator().manual_seed(3)
    B = 2
    b = dict(px=torch.rand(B, 3, 64, 64, generator=g) * 2 - 1, lat=torch.randn(B, 4, 16, 16, generator=g) * 0.18215,
             noise=torch.randn(B, 4, 16, 16, generator=g), ids=torch.randint(1, 99, (B, 9), generator=g), mask=torch.rand(B, 16, 16, generator=g),
             z=torch.randn(B, 4, generator=g), t=torch.tensor([10, 500]))
    b = {k: v.to(dev) for k, v in b.items()}
    pidx = torch.tensor([2, 4], device=dev)
    mask = b["mask"] if masked else None
    seen = []
    orig = Fn.weighted_mse

    def recording(pred, target, lam=None, w=None):
        seen.append((pred.detach().clone(), target.detach().clone(), lam.clone(), w))
        return orig(pred, target, lam, w)

    monkeypatch.setattr(Fn, "weighted_mse", recording)
    runs = []
    for _ in range(2):
        tr0, tr = (_tiny_trainer(dev, snr_gamma=GAMMA, noise_offset=0.1) for _ in range(2))
        out = tr0.losses(b["px"], b["lat"], b["noise"], b["t"], b["ids"], pidx, loss_mask=mask, offset_eps=b["z"])
        out[0].backward()
        grad = tr0.flat.grad.detach().clone()
        step = tr.train_step(b["px"], b["ids"], pidx, noise=b["noise"], timesteps=b["t"], latents=b["lat"], loss_mask=mask, offset_eps=b["z"])
        torch.cuda.synchronize()
        runs.append((torch.stack([o.detach().float() for o in out]).cpu(), grad.cpu(), torch.stack([o.detach().float() for o in step]).cpu(),
                     tr.flat.data.detach().cpu().clone()))
    assert len(seen) == 4
    pred, target, lam, w = seen[0]
    assert w is mask and float(runs[0][1].abs().max()) > 0
    assert float(lam[0]) < 1.0 and float(lam[1]) == 1.0                  # t = 10 is clamped by gamma = 5, t = 500 is not
    _, w_target, w_lam = objective64(b["lat"], b["noise"], b["t"], tr.acp, b["z"], 0.1, False, GAMMA)
    assert rel(target.cpu(), w_target) <= BOUND and rel(lam.cpu(), w_lam) <= BOUND
    want = weighted64(pred, target, lam, mask)[0]
    r = rel(runs[0][0][1], want)
    print(f"weighted step loss_diff {float(runs[0][0][1]):.6f} vs float64 restatement {float(want):.6f}: rel {r:.3e}")
    assert r <= BOUND
    for a, c in zip(runs[0], runs[1]):
        assert torch.equal(a, c)


# ---------------------------------------------------------------------------------------------- 10. the step graph
@pytest.mark.parametrize("mode", ["inputs_given", "draws_inside", "masked"])
def test_weighted_step_graph_replay_equals_eager(hip_env, mode):
    """the whole step with snr_gamma and noise_offset captured and replayed: four steps with different timesteps, losses and every
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

    def run(graph):
        torch.manual_seed(11)
        vae = VAEEncoder(block_out_channels=(64, 128, 128, 128)).requires_grad_(False).to(dev)
        tr = _tiny_trainer(dev, vae=vae, snr_gamma=GAMMA, noise_offset=0.1)
        assert tr.enable_step_graph(True)
        tr._step_graph_on = graph                  # the eager leg keeps the device-side AdamW scalars, launches from the host
        torch.manual_seed(5)
        losses = []
        for b in batches:
            kw = {} if mode == "draws_inside" else dict(noise=b["noise"], timesteps=b["t"], offset_eps=b["z"])
            if mode == "masked":
                kw["loss_mask"] = b["mask"]
            out = tr.train_step(b["px"], b["ids"], pidx, **kw)
            losses.append(torch.stack([o.detach().float() for o in out]).cpu())
        torch.cuda.synchronize()
        return torch.stack(losses), tr.flat.data.detach().cpu().clone(), len(tr._step_graphs)

    l0, p0, n0 = run(False)
    l1, p1, n1 = run(True)
    assert n0 == 0 and n1 == (0 if mode == "masked" else 1)
    assert torch.equal(l0, l1), (l0, l1)
    assert torch.equal(p0, p1), float((p0 - p1).abs().max())
    assert len({float(x) for x in l0[:, 1]}) == 4
