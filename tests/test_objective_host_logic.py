"""CPU: min-SNR-gamma loss weighting and the noise offset above the kernels — the per-timestep coefficient table, the fp32
compositions of functional.diffusion_objective / weighted_mse (the executable specification, and what the op emulation runs) against
a float64 restatement, the trainer with both options through the op emulation, the two command-line flags, and the new entry points'
argument checks.

Bound: rel-L2 <= 2e-5 (BOUND), the project's bound for an fp32 kernel against a float64 restatement."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from test_unet_host_logic import emu_fp32  # noqa: F401
from test_masked_loss_host_logic import BOUND, SHAPES, make_mask, parse, rel
from test_train_step_host_logic import build

OBJ_SHAPES = SHAPES + [(2, 3, 3, 5), (16, 4, 64, 64)]
BASE_T = (0, 10, 500, 999)          # on the project's schedule snr <= 5 first at t = 147: with gamma = 5 the first two clamp, the last two do not
GAMMA = 5.0
CPU = torch.device("cpu")


# ---------------------------------------------------------------------------------------------- float64 restatements
def timesteps_for(B, seed=0):
    """always 0, 10, 500, 999 (the first B of them for B < 4), then seeded random ones"""
    t = list(BASE_T[:B])
    if B > 4:
        t += torch.randint(0, 1000, (B - 4,), generator=torch.Generator().manual_seed(seed)).tolist()
    return torch.tensor(t, dtype=torch.int64)


def timestep_sets(B):
    """the timestep vectors a shape is tested with: for B = 1 each of the four on its own"""
    return [torch.tensor([t], dtype=torch.int64) for t in BASE_T] if B == 1 else [timesteps_for(B)]


def lam64(acp, gamma, v_prediction):
    """the loss weight per timestep in float64 from the fp32 table"""
    a = acp.double().cpu()
    snr = a / (1.0 - a)
    if gamma is None:
        return torch.ones_like(snr)
    return torch.clamp(snr, max=gamma) / ((snr + 1.0) if v_prediction else snr)


def objective64(x0, noise, t, acp, z, s, v_prediction, gamma):
    """'Definitions' in float64: (noisy, target, lam)"""
    a64 = acp.double().cpu()
    B = x0.shape[0]
    t = t.cpu()
    a, sg = a64.sqrt()[t].view(B, 1, 1, 1), (1.0 - a64).sqrt()[t].view(B, 1, 1, 1)
    n1 = noise.double().cpu()
    if s:
        n1 = n1 + s * z.double().cpu().view(B, -1, 1, 1)
    x = x0.double().cpu()
    return a * x + sg * n1, (a * n1 - sg * x) if v_prediction else n1, lam64(acp, gamma, v_prediction)[t]


def weighted64(pred, target, lam, w):
    """loss = sum lam_b w (pred - target)^2 / (C max(sum w, 1)) in float64, gradient by autograd: (loss, dloss/dpred)"""
    p = pred.detach().double().cpu().requires_grad_(True)
    d = p - target.detach().double().cpu()
    B, C = pred.shape[0], pred.shape[1]
    wl = torch.ones(B, 1, 1, 1, dtype=torch.float64) if lam is None else lam.detach().double().cpu().view(B, 1, 1, 1)
    if w is None:
        den = float(pred.numel())
    else:
        w64 = w.detach().double().cpu()
        den = C * torch.clamp(w64.sum(), min=1.0)
        wl = wl * w64.unsqueeze(1)
    loss = (wl * d * d).sum() / den
    loss.backward()
    return loss.detach(), p.grad


def operands(shape, seed=0):
    B, C, h, w = shape
    g = torch.Generator().manual_seed(seed + B * 1000 + h)
    return dict(x0=torch.randn(shape, generator=g), noise=torch.randn(shape, generator=g), z=torch.randn(B, C, generator=g),
                pred=torch.randn(shape, generator=g), g=g)


def lam_for(kind, t, coef):
    return None if kind == "none" else (torch.ones(len(t)) if kind == "ones" else coef[t, 2].clone())


# ---------------------------------------------------------------------------------------------- 1. the coefficient table
def test_schedule_facts():
    from e4t.trainer import ddpm_alphas_cumprod
    acp = ddpm_alphas_cumprod()
    assert acp.dtype == torch.float32 and bool(((acp > 0) & (acp < 1)).all())
    snr = acp.double() / (1 - acp.double())
    assert abs(float(snr[0]) - 1175.4) < 0.1 and abs(float(snr[999]) - 0.00468) < 1e-5
    assert int((snr <= 5).nonzero()[0]) == 147


@pytest.mark.parametrize("v_prediction", [False, True], ids=["epsilon", "v_prediction"])
@pytest.mark.parametrize("gamma", [1.0, 5.0, 20.0])
def test_coef_table(gamma, v_prediction):
    from e4t.trainer import ddpm_alphas_cumprod, objective_coef
    acp = ddpm_alphas_cumprod()
    coef = objective_coef(acp, gamma, v_prediction)
    assert coef.shape == (1000, 3) and coef.dtype == torch.float32 and coef.is_contiguous()
    assert torch.equal(coef[:, 0], acp.sqrt()) and torch.equal(coef[:, 1], (1 - acp).sqrt())
    t = torch.tensor(BASE_T)
    assert torch.equal(coef[t, 0], acp[t].sqrt()) and torch.equal(coef[t, 1], (1 - acp[t]).sqrt())          # what add_noise gathers
    assert torch.equal(coef[:, 2], lam64(acp, gamma, v_prediction).float())
    snr = acp.double() / (1 - acp.double())
    below = snr <= gamma
    assert bool(below.any()) and bool((~below).any())
    if v_prediction:
        assert torch.equal(coef[below, 2], (snr / (snr + 1))[below].float())
    else:
        assert bool((coef[below, 2] == 1.0).all()) and bool((coef[~below, 2] < 1.0).all())
    # without snr_gamma: all ones
    assert torch.equal(objective_coef(acp, None, v_prediction)[:, 2], torch.ones(1000))
    assert torch.equal(objective_coef(acp, None, v_prediction)[:, :2], coef[:, :2])


def test_coef_table_refuses_a_zero_terminal_snr_schedule():
    from e4t.trainer import ddpm_alphas_cumprod, objective_coef
    acp = ddpm_alphas_cumprod()
    for bad in (0.0, 1.0):
        a = acp.clone()
        a[-1] = bad
        with pytest.raises(AssertionError):
            objective_coef(a, 5.0, False)


# ---------------------------------------------------------------------------------------------- 2. the fallback compositions
@pytest.mark.parametrize("shape", OBJ_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("v_prediction", [False, True], ids=["epsilon", "v_prediction"])
@pytest.mark.parametrize("s", [0.0, 0.1])
def test_diffusion_objective_fallback_matches_float64(emu_fp32, shape, v_prediction, s):
    from e4t import functional as Fn
    from e4t.trainer import ddpm_alphas_cumprod, objective_coef
    acp = ddpm_alphas_cumprod()
    coef = objective_coef(acp, GAMMA, v_prediction)
    x = operands(shape)
    for t in timestep_sets(shape[0]):
        noisy, target, lam = Fn.diffusion_objective(x["x0"], x["noise"], t, coef, z=x["z"] if s else None, offset=s, v_prediction=v_prediction)
        assert noisy.dtype == target.dtype == lam.dtype == torch.float32 and noisy.shape == target.shape == shape and lam.shape == (shape[0],)
        w_noisy, w_target, w_lam = objective64(x["x0"], x["noise"], t, acp, x["z"], s, v_prediction, GAMMA)
        assert rel(noisy, w_noisy) <= BOUND and rel(target, w_target) <= BOUND and rel(lam, w_lam) <= BOUND
        assert torch.equal(lam, coef[t, 2])
        if not s and not v_prediction:
            assert torch.equal(target, x["noise"])              # no offset term at all
        if not s:                                               # today's add_noise, bit for bit
            a, sg = acp[t].sqrt().view(-1, 1, 1, 1), (1 - acp[t]).sqrt().view(-1, 1, 1, 1)
            assert torch.equal(noisy, a * x["x0"] + sg * x["noise"])
    if shape[0] >= 4 and not v_prediction:                      # both sides of the clamp
        lam = coef[timesteps_for(shape[0]), 2]
        assert bool((lam < 1).any()) and bool((lam == 1).any())
    with pytest.raises(ValueError):
        Fn.diffusion_objective(x["x0"], x["noise"], timesteps_for(shape[0]), coef, z=None, offset=0.1)


@pytest.mark.parametrize("shape", OBJ_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ["none", "soft", "ones", "zero"])
@pytest.mark.parametrize("lam_kind", ["mixed", "ones"])
def test_weighted_mse_fallback_matches_float64(emu_fp32, shape, kind, lam_kind):
    from e4t import functional as Fn
    from e4t.trainer import ddpm_alphas_cumprod, objective_coef
    B, C, h, w = shape
    coef = objective_coef(ddpm_alphas_cumprod(), GAMMA, False)
    x = operands(shape)
    m = None if kind == "none" else make_mask(kind, B, h, w, x["g"])
    for t in timestep_sets(B):
        lam = lam_for(lam_kind, t, coef)
        pred = x["pred"].clone().requires_grad_(True)
        loss = Fn.weighted_mse(pred, x["noise"], lam, m)
        assert loss.dtype == torch.float32 and loss.dim() == 0
        (loss * 3.0).backward()
        want, dwant = weighted64(pred, x["noise"], lam, m)
        if kind == "zero":
            assert float(loss.detach()) == 0.0 and float(pred.grad.abs().max()) == 0.0
            continue
        assert rel(loss.detach(), want) <= BOUND and rel(pred.grad, 3.0 * dwant) <= BOUND
        if lam_kind == "ones":
            plain = F.mse_loss(pred.detach(), x["noise"]) if m is None else Fn.masked_mse(pred.detach(), x["noise"], m)
            assert rel(loss.detach(), plain) <= BOUND
            assert rel(Fn.weighted_mse(pred.detach(), x["noise"], None, m), plain) <= BOUND


# ---------------------------------------------------------------------------------------------- 3. the trainer
def _inputs(seed=7, B=2):
    g = torch.Generator().manual_seed(seed)
    return dict(pixels=torch.rand(B, 3, 64, 64, generator=g) * 2 - 1, latents=torch.randn(B, 4, 16, 16, generator=g) * 0.18215,
                noise=torch.randn(B, 4, 16, 16, generator=g), t=torch.tensor([10, 500]), ids=torch.randint(1, 99, (B, 9), generator=g),
                pidx=torch.tensor([2, 4]), soft=torch.rand(B, 16, 16, generator=g), z=torch.randn(B, 4, generator=g))


def _trainer(**kw):
    from e4t.trainer import E4TTrainer
    _, _, n_unet, n_enc, text = build()
    return E4TTrainer(n_unet, n_enc, text, vae=None, lr=1e-3, class_token_id=11, empty_prompt_ids=torch.zeros(1, 9, dtype=torch.long),
                      device=CPU, **kw)


def _record(monkeypatch):
    from e4t import functional as Fn
    seen = []
    orig = Fn.weighted_mse

    def recording(pred, target, lam=None, w=None):
        seen.append((pred.detach().clone(), target.detach().clone(), lam, w))
        return orig(pred, target, lam, w)

    monkeypatch.setattr(Fn, "weighted_mse", recording)
    return seen


def test_constructor_validates_and_builds_the_table(emu_fp32):
    from e4t.trainer import objective_coef
    for bad in (dict(snr_gamma=0.0), dict(snr_gamma=-1.0), dict(noise_offset=-0.1), dict(snr_gamma=float("nan"))):
        with pytest.raises(ValueError):
            _trainer(**bad)
    tr = _trainer(snr_gamma=GAMMA, noise_offset=0.1)
    assert tr.snr_gamma == GAMMA and tr.noise_offset == 0.1
    assert torch.equal(tr.coef, objective_coef(tr.acp, GAMMA, False))
    plain = _trainer()
    assert plain.snr_gamma is None and plain.noise_offset == 0.0 and torch.equal(plain.coef[:, 2], torch.ones(1000))
    assert set(tr.state_dict()) == set(plain.state_dict())          # constructor state: nothing new to save


@pytest.mark.parametrize("pred_type", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_losses_with_both_options_agree_with_the_manual_composition(emu_fp32, monkeypatch, pred_type, masked):
    x = _inputs()
    seen = _record(monkeypatch)
    tr = _trainer(snr_gamma=GAMMA, noise_offset=0.1, prediction_type=pred_type)
    mask = x["soft"] if masked else None
    out = tr.losses(x["pixels"], x["latents"], x["noise"], x["t"], x["ids"], x["pidx"], loss_mask=mask, offset_eps=x["z"])
    assert len(seen) == 1
    pred, target, lam, w = seen[0]
    v = pred_type != "epsilon"
    _, w_target, w_lam = objective64(x["latents"], x["noise"], x["t"], tr.acp, x["z"], 0.1, v, GAMMA)
    assert rel(target, w_target) <= BOUND and rel(lam, w_lam) <= BOUND and w is mask
    if not v:
        assert float(lam[0]) < 1.0 and float(lam[1]) == 1.0         # t = 10 clamps (snr > gamma), t = 500 does not
    assert rel(out[1].detach(), weighted64(pred, target, lam, mask)[0]) <= BOUND
    assert rel(out[0].detach(), out[1].detach().double() + out[2].detach().double()) <= BOUND
    out[0].backward()
    assert float(tr.flat.grad.abs().max()) > 0
    # the weighting matters: the unweighted loss of the same prediction is another number
    assert abs(float(weighted64(pred, target, None, mask)[0]) - float(out[1].detach())) > 1e-4 * float(out[1].detach())


def test_offset_draw_order_and_reproduction(emu_fp32):
    """the [B, C] draw comes right after the noise and before the timesteps; handing the same draws in reproduces the step"""
    x = _inputs()
    tr = _trainer(snr_gamma=GAMMA, noise_offset=0.1)
    torch.manual_seed(21)
    inside = tr.train_step(x["pixels"], x["ids"], x["pidx"], latents=x["latents"])
    state_after = torch.get_rng_state()
    torch.manual_seed(21)
    noise = torch.randn_like(x["latents"])
    z = torch.randn((2, 4))
    t = torch.randint(0, 1000, (2,)).long()
    assert torch.equal(torch.get_rng_state(), state_after)
    tr2 = _trainer(snr_gamma=GAMMA, noise_offset=0.1)
    given = tr2.train_step(x["pixels"], x["ids"], x["pidx"], noise=noise, timesteps=t, latents=x["latents"], offset_eps=z)
    for a, b in zip(inside, given):
        assert torch.equal(a, b)
    assert torch.equal(tr.flat.data, tr2.flat.data)
    # losses() on its own draws z too when it is not given
    torch.manual_seed(4)
    a = _trainer(noise_offset=0.1).losses(x["pixels"], x["latents"], x["noise"], x["t"], x["ids"], x["pidx"])
    torch.manual_seed(4)
    b = _trainer(noise_offset=0.1).losses(x["pixels"], x["latents"], x["noise"], x["t"], x["ids"], x["pidx"], offset_eps=torch.randn((2, 4)))
    assert torch.equal(a[1], b[1])
    c = _trainer(noise_offset=0.1).losses(x["pixels"], x["latents"], x["noise"], x["t"], x["ids"], x["pidx"], offset_eps=x["z"])
    assert not torch.equal(a[1], c[1])                              # and the draw matters


def test_without_the_options_the_step_and_its_rng_stream_are_todays(emu_fp32, monkeypatch):
    from e4t import functional as Fn
    x = _inputs()
    calls = []
    for name in ("diffusion_objective", "weighted_mse"):
        monkeypatch.setattr(Fn, name, lambda *a, _n=name, **k: calls.append(_n))
    tr = _trainer()
    torch.manual_seed(33)
    tr.train_step(x["pixels"], x["ids"], x["pidx"], latents=x["latents"])
    after = torch.get_rng_state()
    torch.manual_seed(33)
    torch.randn_like(x["latents"])
    torch.randint(0, 1000, (2,))
    assert torch.equal(torch.get_rng_state(), after) and not calls


def test_noise_offset_alone_keeps_todays_loss_call(emu_fp32, monkeypatch):
    x = _inputs()
    seen = _record(monkeypatch)
    tr = _trainer(noise_offset=0.1)
    out = tr.losses(x["pixels"], x["latents"], x["noise"], x["t"], x["ids"], x["pidx"], offset_eps=x["z"])
    plain = _trainer().losses(x["pixels"], x["latents"], x["noise"], x["t"], x["ids"], x["pidx"])
    assert not seen and torch.isfinite(out[1]) and not torch.equal(out[1], plain[1])


def test_a_huge_gamma_is_the_plain_step(emu_fp32):
    x = _inputs()
    a = _trainer(snr_gamma=1e9).losses(x["pixels"], x["latents"], x["noise"], x["t"], x["ids"], x["pidx"])
    b = _trainer().losses(x["pixels"], x["latents"], x["noise"], x["t"], x["ids"], x["pidx"])
    assert rel(a[1].detach(), b[1].detach()) <= BOUND
    m = x["soft"]
    a = _trainer(snr_gamma=1e9).losses(x["pixels"], x["latents"], x["noise"], x["t"], x["ids"], x["pidx"], loss_mask=m)
    b = _trainer().losses(x["pixels"], x["latents"], x["noise"], x["t"], x["ids"], x["pidx"], loss_mask=m)
    assert rel(a[1].detach(), b[1].detach()) <= BOUND


def test_weighted_step_takes_the_graphed_path_and_a_masked_one_never(emu_fp32, monkeypatch):
    x = _inputs()
    tr = _trainer(snr_gamma=GAMMA, noise_offset=0.1)
    tr._step_graph_on = True
    taken = []

    def graphed(*a, **k):
        taken.append(a[7] if len(a) > 7 else k.get("offset_eps"))
        return tr._train_step(*a[:3], noise=a[3], timesteps=a[4], latents=a[6], offset_eps=taken[-1])

    monkeypatch.setattr(tr, "_graphed_step", graphed)
    kw = dict(noise=x["noise"], timesteps=x["t"], latents=x["latents"])
    tr.train_step(x["pixels"], x["ids"], x["pidx"], offset_eps=x["z"], **kw)
    assert len(taken) == 1 and taken[0] is x["z"]
    tr.train_step(x["pixels"], x["ids"], x["pidx"], loss_mask=x["soft"], **kw)
    assert len(taken) == 1


# ---------------------------------------------------------------------------------------------- 4. command lines
def test_objective_flags(monkeypatch, capsys):
    for module, base in (("pretrain_e4t", ["--synthetic_data"]), ("tuning_e4t", ["--synthetic_data"])):
        a = parse(module, base, monkeypatch)
        assert a.snr_gamma is None and a.noise_offset == 0.0
        a = parse(module, base + ["--snr_gamma", "5", "--noise_offset", "0.1"], monkeypatch)
        assert a.snr_gamma == 5.0 and a.noise_offset == 0.1
        assert parse(module, base + ["--noise_offset", "0"], monkeypatch).noise_offset == 0.0
        for bad, msg in ((["--snr_gamma", "0"], "--snr_gamma must be > 0"), (["--snr_gamma", "-1"], "--snr_gamma must be > 0"),
                         (["--noise_offset", "-0.1"], "--noise_offset must be >= 0")):
            with pytest.raises(SystemExit) as ex:
                parse(module, base + bad, monkeypatch)
            assert ex.value.code == 2 and msg in capsys.readouterr().err


def test_setup_hands_the_flags_to_the_trainer_and_config_records_them(emu_fp32, tmp_path):
    import pretrain_e4t
    import tuning_e4t
    from e4t.utils import save_config
    from test_cli_setup import pretrain_args, tuning_args
    for module, mk in ((pretrain_e4t, pretrain_args), (tuning_e4t, tuning_args)):
        tr = module.setup(mk(), CPU)["trainer"]                     # a namespace without the attributes: both off
        assert tr.snr_gamma is None and tr.noise_offset == 0.0
        args = mk(snr_gamma=5.0, noise_offset=0.1)
        tr = module.setup(args, CPU)["trainer"]
        assert tr.snr_gamma == 5.0 and tr.noise_offset == 0.1 and bool((tr.coef[:, 2] < 1).any())
        d = str(tmp_path / module.__name__)
        save_config(vars(args), d)
        cfg = json.load(open(os.path.join(d, "config.json")))
        assert cfg["snr_gamma"] == 5.0 and cfg["noise_offset"] == 0.1


# ---------------------------------------------------------------------------------------------- 5. entry points
def test_new_entry_points_check_their_arguments():
    """argument validation happens on the host before any launch: safe to call without a GPU"""
    import ctypes
    from e4t import _C
    lib = _C.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    # e4t_diffuse(x0, noise, z, timesteps, coef, noisy, target, lam, B, C, HW, T, s, v_prediction, stream)
    for k in (0, 1, 3, 4, 5, 6, 7):                                  # every pointer but z
        ptrs = [p] * 8
        ptrs[k] = None
        assert lib.e4t_diffuse(*ptrs, 1, 4, 1, 1000, 0.0, 0, None) == -22 and b"diffuse" in lib.e4t_last_error()
    for sizes in ((0, 4, 1, 1000), (1, 0, 1, 1000), (1, 4, 0, 1000), (1, 4, 1, 0), (-1, 4, 1, 1000)):
        assert lib.e4t_diffuse(*([p] * 8), *sizes, 0.0, 0, None) == -22 and b"diffuse" in lib.e4t_last_error()
    assert lib.e4t_diffuse(p, p, None, p, p, p, p, p, 1, 4, 1, 1000, 0.1, 0, None) == -22
    assert b"diffuse" in lib.e4t_last_error() and b"needs z" in lib.e4t_last_error()
    assert lib.e4t_diffuse(*([p] * 8), 1, 4, 1, 1000, -0.1, 0, None) == -22
    # e4t_weighted_mse_fwd(pred, target, w, lam, wd, stats, B, C, HW, pred_nhwc, stream): w, lam and wd may be null
    for k in (0, 1, 5):
        ptrs = [p] * 6
        ptrs[k] = None
        assert lib.e4t_weighted_mse_fwd(*ptrs, 1, 4, 1, 0, None) == -22 and b"weighted_mse_fwd" in lib.e4t_last_error()
    for sizes in ((0, 4, 1), (1, 0, 1), (1, 4, 0)):
        assert lib.e4t_weighted_mse_fwd(*([p] * 6), *sizes, 0, None) == -22 and b"weighted_mse_fwd" in lib.e4t_last_error()
    # the backward is e4t_masked_mse_bwd: no e4t_weighted_mse_bwd is exported
    assert "e4t_weighted_mse_bwd" not in _C.SIGNATURES and not hasattr(lib, "e4t_weighted_mse_bwd")
