"""CPU: every sampler's fused plan (``fused_plan``: the rows of e4t_sampler_step for one call) reproduces the scheduler's own
``step`` loop.  The rows are applied by a float64 torch restatement of the kernel's formula (include/e4t_hip.h) and compared
with driving ``scale_model_input`` / ``step`` in float64 on the same inputs, noise included, with a model output that
depends on the latent it is given."""
import pytest
import torch

from e4t.schedulers import SCHEDULER_MAPPING, DDIMScheduler, DPMSolverMultistepScheduler, FusedPlan, MAX_HIST, ROW

f64 = torch.float64
SHAPE = (2, 4, 3, 5)
STEPS = (1, 2, 3, 4, 5, 14, 15, 20, 50)
CASES = [("ddim", 0.0), ("ddim", 0.6), ("plms", 0.0), ("lms", 0.0), ("euler", 0.0), ("euler_ancestral", 0.0), ("dpm_solver++", 0.0)]


def apply_row(row, pred, x, hist, saved, noise, cfg):
    """one e4t_sampler_step in float64: returns (x', x_in); updates hist / saved in place"""
    g, a_e, a_x, c_x, c_s, c_m, c_n, k_in, w, save_x = row[:10].tolist()
    if cfg:
        u, c = pred.chunk(2)
        e = u + g * (c - u)
    else:
        e = pred
    m = a_e * e + a_x * x
    out = c_x * x + c_m * m + c_s * saved + c_n * noise
    for k in range(hist.shape[0]):
        out = out + float(row[10 + k]) * hist[k]
    if w >= 0:
        hist[int(w)] = m
    if save_x:
        saved.copy_(x)
    return out, k_in * out


class ToyModel:
    """[u | c] = tanh(x_in W_u,c) + per-call noise: depends on x, so an error anywhere in the update shows up downstream"""

    def __init__(self, seed, calls):
        g = torch.Generator().manual_seed(seed)
        self.w = torch.randn(2, SHAPE[-1], SHAPE[-1], generator=g, dtype=f64) * 0.7
        self.nz = torch.randn(calls, 2, *SHAPE, generator=g, dtype=f64) * 0.3

    def __call__(self, x_in, i, cfg):
        u, c = (torch.tanh(x_in @ self.w[k]) + self.nz[i, k] for k in range(2))
        return torch.cat([u, c]) if cfg else c


def make(name, pt):
    return SCHEDULER_MAPPING[name].stable_diffusion(prediction_type=pt)


def state(sch):
    return {k: (v.clone() if torch.is_tensor(v) else list(v) if isinstance(v, list) else v) for k, v in vars(sch).items()}


def same_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] is b[k] or a[k] == b[k], k


def run_plan(plan, x0, model, g, cfg, sch, seed):
    gen = torch.Generator().manual_seed(seed)
    x = x0.clone()
    hist = torch.zeros(plan.K, *SHAPE, dtype=f64)
    saved = torch.zeros(SHAPE, dtype=f64)
    x_in = plan.k_in * x
    for i in range(len(plan.timesteps)):
        noise = sch._step_noise(SHAPE, f64, torch.device("cpu"), gen) if plan.noisy[i] else torch.zeros(SHAPE, dtype=f64)
        x, x_in = apply_row(plan.table[i], model(x_in, i, cfg), x, hist, saved, noise, cfg)
    return x


def run_steps(sch, x0, model, g, cfg, eta, seed):
    gen = torch.Generator().manual_seed(seed)
    x = x0.clone()
    for i, t in enumerate(sch.timesteps):
        pred = model(sch.scale_model_input(x, t), i, cfg)
        if cfg:
            u, c = pred.chunk(2)
            pred = u + g * (c - u)
        if isinstance(sch, DDIMScheduler):
            kw = dict(eta=eta, variance_noise=sch._step_noise(SHAPE, f64, torch.device("cpu"), gen) if eta > 0 else None)
        elif "generator" in sch.step.__code__.co_varnames:
            kw = dict(generator=gen)
        else:
            kw = {}
        x = sch.step(pred, t, x, **kw).prev_sample
    return x


@pytest.mark.parametrize("name,eta", CASES)
@pytest.mark.parametrize("pt", ["epsilon", "v_prediction"])
def test_plan_reproduces_step_loop(name, eta, pt):
    worst = 0.0
    for n in STEPS:
        for g in (1.0, 7.5):
            cfg = g > 1.0
            sch = make(name, pt)
            sch.set_timesteps(n)
            before = state(sch)
            plan = sch.fused_plan(guidance_scale=g, eta=eta)
            same_state(before, state(sch))                       # the plan leaves the scheduler's Python state alone
            assert isinstance(plan, FusedPlan)
            calls = len(sch.timesteps)
            assert calls == (n + 1 if name == "plms" and n > 1 else n)
            assert plan.table.dtype == f64 and plan.table.shape == (calls, ROW) and 0 <= plan.K <= MAX_HIST
            assert torch.equal(plan.timesteps, sch.timesteps) and plan.timesteps.dtype == sch.timesteps.dtype
            assert (plan.table[:, 0] == g).all() and len(plan.noisy) == calls
            assert ((plan.table[:, 8] >= -1) & (plan.table[:, 8] < max(plan.K, 1))).all()
            model = ToyModel(seed=n, calls=calls)
            x0 = torch.randn(SHAPE, generator=torch.Generator().manual_seed(100 + n), dtype=f64) * sch.init_noise_sigma
            got = run_plan(plan, x0, model, g, cfg, sch, seed=7)
            sch.set_timesteps(n)
            want = run_steps(sch, x0, model, g, cfg, eta, seed=7)
            rel = float((got - want).norm() / want.norm())
            assert torch.isfinite(want).all() and rel < 1e-10, (n, g, rel)
            worst = max(worst, rel)
    print(f"{name} eta={eta} {pt}: worst rel diff {worst:.2e}")


def test_ddim_eta0_rows_are_guided_step_rows():
    """a DDIM eta = 0 row is {g, 1, 0, c_sample, 0, c_pred, 0, 1, -1, 0, ...}: what e4t_guided_step computes"""
    sch = DDIMScheduler.stable_diffusion()
    sch.set_timesteps(10)
    plan = sch.fused_plan(guidance_scale=5.0)
    assert plan.K == 0 and not any(plan.noisy) and not plan.saves_x and plan.k_in == 1.0
    for t, r in zip(sch.timesteps.tolist(), plan.table.tolist()):
        cs, cp, _ = sch.coefficients(t)
        assert r == [5.0, 1.0, 0.0, cs, 0.0, cp, 0.0, 1.0, -1.0, 0.0] + [0.0] * 6


def test_nonlinear_configurations_have_no_plan():
    clip = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=True, set_alpha_to_one=False,
                         steps_offset=1)
    clip.set_timesteps(10)
    assert clip.fused_plan(7.5) is None
    for name in SCHEDULER_MAPPING:
        sch = make(name, "sample")
        sch.set_timesteps(10)
        assert sch.fused_plan(7.5) is None, name
        assert make(name, "epsilon").fused_plan(7.5) is None, name          # set_timesteps not called: step() would refuse too
    dpm = DPMSolverMultistepScheduler.stable_diffusion()
    dpm.set_timesteps(1000)                                                  # rounded timesteps collide: step() cannot index them
    assert len(set(dpm.timesteps.tolist())) < 1000 and dpm.fused_plan(7.5) is None


def test_sampler_step_rejects_bad_arguments():
    """e4t_sampler_step validates its arguments on the host, before any launch (safe without a GPU)"""
    from e4t import _C
    lib = _C.load()
    p = 4096                                                          # never dereferenced: every call below fails validation
    assert lib.e4t_sampler_step(None, p, p, p, None, None, None, p, 1, 4, 64, 0, 1, 1, 0, None) == -22
    assert lib.e4t_sampler_step(p, p, p, p, None, None, None, p, 1, 4, 64, 5, 1, 1, 0, None) == -22
    assert b"history slots" in lib.e4t_last_error()
    assert lib.e4t_sampler_step(p, p, p, None, None, None, None, p, 1, 4, 64, 2, 1, 1, 0, None) == -22
    assert lib.e4t_sampler_step(p, p, p, None, None, None, None, p, 1, 4, 64, 0, 1, 1, 3, None) == -22
    assert b"x_in_copies" in lib.e4t_last_error()
    assert lib.e4t_sampler_step(p, p, p, None, None, None, None, p, 1, 4, 64, 0, 1, 1, 1, None) == -22
    assert lib.e4t_sampler_step(p, p, p, None, None, None, None, p, 0, 4, 64, 0, 1, 1, 0, None) == -22
