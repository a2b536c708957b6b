"""CPU: editing (img2img, masked inpainting) on the scheduler side.  ``set_timesteps(n, begin=k)`` keeps the last
n - k steps, ``fused_plan(blend=True)`` fills the rows' slots 14 / 15, and a float64 interpretation of the rows (the contract of
e4t_sampler_step_edit in include/e4t_hip.h) reproduces the definition: the generic ``step`` loop with
``latents = keep*(a*x0 + s*n0) + (1 - keep)*latents`` after every step."""
import os
import sys

import pytest
import torch

from e4t.schedulers import SCHEDULER_MAPPING, ROW
from test_sampler_fused_gpu import SAMPLERS
from test_sampler_plan import SHAPE, ToyModel, apply_row, f64, make, run_plan, run_steps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 10
BEGINS = (0, 3, 9)


def sample_noise(sch, plan_noisy, gen):
    return sch._step_noise(SHAPE, f64, torch.device("cpu"), gen) if plan_noisy else torch.zeros(SHAPE, dtype=f64)


def run_plan_edit(plan, start, model, cfg, sch, seed, keep, x0, n0):
    """the rows in float64, slots 14 / 15 included: out' = keep*(a_keep*x0 + s_keep*n0) + (1 - keep)*out; hist / saved as unblended"""
    gen = torch.Generator().manual_seed(seed)
    x = start.clone()
    hist = torch.zeros(plan.K, *SHAPE, dtype=f64)
    saved = torch.zeros(SHAPE, dtype=f64)
    x_in = plan.k_in * x
    for i in range(len(plan.timesteps)):
        row = plan.table[i]
        o, _ = apply_row(row, model(x_in, i, cfg), x, hist, saved, sample_noise(sch, plan.noisy[i], gen), cfg)
        x = keep * (float(row[14]) * x0 + float(row[15]) * n0) + (1 - keep) * o
        x_in = float(row[7]) * x
    return x


def run_steps_edit(sch, start, model, g, cfg, eta, seed, keep, x0, n0):
    """the definition: scale_model_input / step, then the blend at the next timestep's level ((1, 0) after the last step)"""
    gen = torch.Generator().manual_seed(seed)
    x = start.clone()
    ts = sch.timesteps
    for i, t in enumerate(ts):
        pred = model(sch.scale_model_input(x, t), i, cfg)
        if cfg:
            u, c = pred.chunk(2)
            pred = u + g * (c - u)
        if "eta" in sch.step.__code__.co_varnames:
            kw = dict(eta=eta, variance_noise=sch._step_noise(SHAPE, f64, torch.device("cpu"), gen) if eta > 0 else None)
        elif "generator" in sch.step.__code__.co_varnames:
            kw = dict(generator=gen)
        else:
            kw = {}
        x = sch.step(pred, t, x, **kw).prev_sample
        a, s = sch.noise_level(ts[i + 1]) if i + 1 < len(ts) else (1.0, 0.0)
        x = keep * (a * x0 + s * n0) + (1 - keep) * x
    return x


def inputs(seed):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(SHAPE, generator=g, dtype=f64)
    n0 = torch.randn(SHAPE, generator=g, dtype=f64)
    keep = torch.rand(SHAPE[-2:], generator=g, dtype=f64)
    keep[0, 0], keep[0, 1], keep[1, 2], keep[2, 4] = 0.0, 1.0, 0.0, 1.0          # exact 0 and exact 1 entries among the soft ones
    return x0, n0, keep


@pytest.mark.parametrize("begin", BEGINS)
@pytest.mark.parametrize("name,eta", SAMPLERS)
@pytest.mark.parametrize("pt", ["epsilon", "v_prediction"])
def test_blend_plan_reproduces_step_and_blend_loop(name, eta, pt, begin):
    x0, n0, keep = inputs(3)
    assert (keep == 0).any() and (keep == 1).any() and ((keep > 0) & (keep < 1)).any()
    for g in (1.0, 7.5):
        cfg = g > 1.0
        sch = make(name, pt)
        sch.set_timesteps(N)
        full = sch.timesteps.clone()
        sch.set_timesteps(N, begin=begin)
        kept = N - begin
        calls = kept + 1 if name == "plms" and kept > 1 else kept
        assert len(sch.timesteps) == calls
        if name != "plms":
            assert torch.equal(sch.timesteps, full[begin:])
        else:                                           # the doubled call moves to the first kept step
            assert sorted(set(sch.timesteps.tolist()), reverse=True) == sorted(set(full.tolist()), reverse=True)[begin:]
        plan = sch.fused_plan(guidance_scale=g, eta=eta, blend=True)
        assert plan.table.shape == (calls, ROW)
        plain = sch.fused_plan(guidance_scale=g, eta=eta)
        assert torch.equal(plan.table[:, :14], plain.table[:, :14]) and (plain.table[:, 14:] == 0).all()
        levels = [sch.noise_level(t) for t in sch.timesteps.tolist()[1:]] + [(1.0, 0.0)]
        assert plan.table[:, 14:].tolist() == [list(l) for l in levels]
        a, s = sch.noise_level(sch.timesteps[0])
        start = a * x0 + s * n0
        model = ToyModel(seed=begin, calls=calls)
        got = run_plan_edit(plan, start, model, cfg, sch, 7, keep, x0, n0)
        sch.set_timesteps(N, begin=begin)
        want = run_steps_edit(sch, start, model, g, cfg, eta, 7, keep, x0, n0)
        rel = float((got - want).norm() / want.norm())
        assert torch.isfinite(want).all() and rel < 1e-10, (g, rel)
        assert torch.equal(got[..., keep == 1], x0[..., keep == 1])                  # held pixels end clean, exactly


@pytest.mark.parametrize("name,eta", SAMPLERS)
@pytest.mark.parametrize("pt", ["epsilon", "v_prediction"])
def test_begin_zero_without_blend_is_the_plain_schedule(name, eta, pt):
    """begin = 0, blend = False: timesteps, sigmas, init_noise_sigma and the table are what set_timesteps(n) / fused_plan give,
    exactly; keep == 0 then reproduces the plain loop and keep == 1 ends at x0"""
    a, b = make(name, pt), make(name, pt)
    a.set_timesteps(N)
    b.set_timesteps(N, begin=0)
    assert torch.equal(a.timesteps, b.timesteps) and a.timesteps.dtype == b.timesteps.dtype
    assert a.init_noise_sigma == b.init_noise_sigma
    if hasattr(a, "sigmas"):
        assert torch.equal(a.sigmas, b.sigmas)
    pa, pb = a.fused_plan(7.5, eta), b.fused_plan(7.5, eta, blend=False)
    assert torch.equal(pa.table, pb.table) and (pa.table[:, 14:] == 0).all()
    assert (pa.K, pa.k_in, pa.noisy, pa.saves_x) == (pb.K, pb.k_in, pb.noisy, pb.saves_x)

    x0, n0, _ = inputs(4)
    model = ToyModel(seed=1, calls=len(a.timesteps))
    start = torch.randn(SHAPE, generator=torch.Generator().manual_seed(9), dtype=f64) * a.init_noise_sigma
    zero, one = torch.zeros(SHAPE[-2:], dtype=f64), torch.ones(SHAPE[-2:], dtype=f64)
    blend = b.fused_plan(7.5, eta, blend=True)
    assert torch.equal(run_plan_edit(blend, start, model, True, b, 7, zero, x0, n0), run_plan(pa, start, model, 7.5, True, a, seed=7))
    assert torch.equal(run_plan_edit(blend, start, model, True, b, 7, one, x0, n0), x0)
    b.set_timesteps(N, begin=0)
    got = run_steps_edit(b, start, model, 7.5, True, eta, 7, zero, x0, n0)
    a.set_timesteps(N)
    assert torch.equal(got, run_steps(a, start, model, 7.5, True, eta, seed=7))
    b.set_timesteps(N, begin=0)
    assert torch.equal(run_steps_edit(b, start, model, 7.5, True, eta, 7, one, x0, n0), x0)


@pytest.mark.parametrize("name", sorted(SCHEDULER_MAPPING))
def test_begin_out_of_range_is_refused(name):
    sch = make(name, "epsilon")
    for begin in (-1, N):
        with pytest.raises(ValueError):
            sch.set_timesteps(N, begin=begin)


@pytest.mark.parametrize("name", sorted(SCHEDULER_MAPPING))
def test_noise_level_agrees_with_add_noise(name):
    sch = make(name, "epsilon")
    sch.set_timesteps(N, begin=2)
    x0, n0, _ = inputs(5)
    for t in sch.timesteps.tolist():
        a, s = sch.noise_level(t)
        if name in ("lms", "euler", "euler_ancestral"):
            assert a == 1.0 and s == float(sch.sigmas[sch._index(t)])
        else:
            acp = float(sch.alphas_cumprod[int(t)])
            assert abs(a - acp ** 0.5) < 1e-15 and abs(s - (1 - acp) ** 0.5) < 1e-15
        tt = torch.tensor([t] * SHAPE[0], dtype=sch.timesteps.dtype)
        got = sch.add_noise(x0, n0, tt)
        assert float((got - (a * x0 + s * n0)).abs().max()) < 1e-14, (name, t)


def test_ddim_add_noise_is_unchanged():
    """DDIM had add_noise before: fp32, per-sample integer timesteps, straight from alphas_cumprod"""
    sch = make("ddim", "epsilon")
    g = torch.Generator().manual_seed(2)
    x, n = torch.randn(3, 4, 5, 5, generator=g), torch.randn(3, 4, 5, 5, generator=g)
    t = torch.tensor([1, 500, 999])
    acp = sch.alphas_cumprod
    want = acp[t].sqrt().view(-1, 1, 1, 1) * x + (1 - acp[t]).sqrt().view(-1, 1, 1, 1) * n
    assert torch.equal(sch.add_noise(x, n, t), want)


def test_sampler_step_edit_rejects_bad_arguments():
    """e4t_sampler_step_edit validates on the host before any launch (safe without a GPU)"""
    from e4t import _C
    lib = _C.load()
    p = 4096                                                          # never dereferenced: every call below fails validation

    def call(keep=p, x0=p, n0=p, K=0, hist=None, copies=0, x_in=None, kpi=0, xpi=0, pred=p, B=1):
        return lib.e4t_sampler_step_edit(pred, p, p, hist, None, None, x_in, p, keep, x0, n0, B, 4, 64, K, 1, 1, copies, kpi, xpi, None)

    assert call(keep=None) == -22 and b"keep, x0 and n0" in lib.e4t_last_error()
    assert call(x0=None) == -22
    assert call(n0=None) == -22
    assert call(kpi=2) == -22 and b"keep_per_image" in lib.e4t_last_error()
    assert call(kpi=-1) == -22
    assert call(xpi=2) == -22
    assert call(xpi=-1) == -22
    assert call(K=5, hist=p) == -22 and b"history slots" in lib.e4t_last_error()
    assert call(K=2) == -22
    assert call(copies=3, x_in=p) == -22 and b"x_in_copies" in lib.e4t_last_error()
    assert call(copies=1) == -22
    assert call(pred=None) == -22
    assert call(B=0) == -22


def parse(monkeypatch, *argv):
    monkeypatch.syspath_prepend(ROOT)
    import inference
    monkeypatch.setattr(sys, "argv", ["inference.py", *argv])
    return inference.parse_args()


def test_inference_cli_parses_the_edit_flags(monkeypatch, capsys):
    args = parse(monkeypatch, "--init_image", "photo.png", "--strength", "0.5", "--mask_image", "mask.png")
    assert (args.init_image, args.strength, args.mask_image) == ("photo.png", 0.5, "mask.png")
    args = parse(monkeypatch)
    assert (args.init_image, args.strength, args.mask_image) == (None, 0.8, None)
    assert parse(monkeypatch, "--init_image", "photo.png", "--strength", "1.0").strength == 1.0
    for bad in (["--init_image", "p.png", "--strength", "0"], ["--init_image", "p.png", "--strength", "1.5"], ["--mask_image", "m.png"],
                ["--init_image", "p.png", "--strength", "0.01"]):
        with pytest.raises(SystemExit) as ex:
            parse(monkeypatch, *bad)
        assert ex.value.code == 2, bad
    capsys.readouterr()


def test_pipeline_refuses_bad_edit_arguments():
    """the checks come before any model runs: a pipeline object without models is enough"""
    from e4t.pipeline_stable_diffusion_e4t import StableDiffusionE4TPipeline as P
    pipe = P.__new__(P)
    pipe.vae_encoder = None
    with pytest.raises(ValueError, match="vae_encoder"):
        pipe.prepare_edit(torch.zeros(1, 3, 32, 32), 0.5, None, 6, 1, 32, 32, torch.device("cpu"))
    pipe.vae_encoder = object()
    for strength in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="strength"):
            pipe.prepare_edit(torch.zeros(1, 3, 32, 32), strength, None, 6, 1, 32, 32, torch.device("cpu"))
    with pytest.raises(ValueError, match="no denoising step"):
        pipe.prepare_edit(torch.zeros(1, 3, 32, 32), 0.1, None, 6, 1, 32, 32, torch.device("cpu"))
