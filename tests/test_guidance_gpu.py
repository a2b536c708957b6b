"""-m gpu: guidance rescale and identity guidance.  e4t_guidance_stats and e4t_sampler_step_guided against the
float64 restatement of their header contract (tests/guidance_reference.py) and, where the contract says so, bit for bit against
e4t_sampler_step / e4t_sampler_step_edit; then the pipeline's two options for every sampler on the tiny models: fused eager ==
graph replay bit for bit, fused close to the generic loop (schedulers.combine_guidance, the definition), held pixels of an edit
end at the original's latent exactly, and a plain call is untouched by a guided one.

Bounds: 1e-6 relative on the statistics and on the step with a given factor is what this kernel family carries in
test_sampler_edit_gpu.py; an fp32 two-pass deviation with a fixed-order tree sum stays within 2e-7 on f for N >= 1020 and the
four (mean, sd) pairs below, a one-pass sum / sum of squares is off by 3e-5 .. 4.5e-1 in every offset case.  End to end
through the statistics kernel the step may add the factor's error to its own: 2e-6.

Which image takes which (mean, sd): image b takes PAIRS[b]; the shapes with N >= 1020 rotate the start so that every pair,
(10, 0.01) included, meets every code path.  The three shapes with N <= 231 do not rotate: the contract forms e0 in fp32, and
rounding a value of size 10 to fp32 (ulp 9.5e-7) moves a deviation of 0.1 taken over N values by about ulp / (0.1 sqrt(N)),
4e-6 at N = 5 and 6e-7 at N = 231, whatever the kernel does afterwards (an fp32 two-pass on the CPU: up to 8e-6 at N = 4 and 5,
1.8e-7 at N = 1024); the bound has no meaning there."""
import pytest
import torch

import guidance_reference as gr
from guidance_reference import rel
from test_sampler_edit_gpu import call, edit_pipe  # noqa: F401
from test_sampler_fused_gpu import SAMPLERS, tiny_pipe  # noqa: F401  (tiny_pipe: this module's own instance)

pytestmark = pytest.mark.gpu

f32 = torch.float32
SHAPES = [(1, 4, 16, 16),      # N = 1024: one full pass of the workgroup
          (2, 4, 15, 17),      # N = 1020: ragged, not a multiple of 4
          (3, 4, 31, 33),      # N = 4092: several trips and a tail
          (2, 3, 7, 11),       # odd C: NHWC indexing, no 16-byte loads
          (2, 5, 1, 1),        # tiny N
          (1, 4, 1, 1),
          (1, 4, 96, 96)]      # the 768 px latent
G, G_ID = 7.5, 10.0


def first_pair(shape, r):
    """the rotation of PAIRS for a case (module docstring): none for the shapes too small to carry the offset pairs' bound"""
    return r if shape[1] * shape[2] * shape[3] >= 1020 else 0


def guide_params(dev, phi, g=G, g_id=G_ID):
    return torch.tensor([g, g_id, phi, 0.0], dtype=f32, device=dev)


def relerr(got, want):
    return float(((got.double() - want).abs() / want.abs()).max())


@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_guidance_stats_matches_restatement(hip_env, si):
    hip, _, dev, _ = hip_env
    shape = SHAPES[si]
    B, C, H, W = shape
    gen = torch.Generator(device=dev).manual_seed(40 + si)
    worst, worst_torch = 0.0, 0.0
    for branches in (2, 3):
        for nhwc in (False, True):
            for phi in (1.0, 0.7):
                pred = gr.draw(shape, branches, nhwc, gen, dev, first_pair=first_pair(shape, si + branches))
                gp = guide_params(dev, phi)
                pred0, gp0 = pred.clone(), gp.clone()
                want = gr.stats(pred, gp, shape, branches, nhwc)
                band = torch.full((B + 2, 4), float("nan"), device=dev)             # NaN guard rows around gstat
                got = hip.guidance_stats(pred, gp, branches, nhwc, out=band[1:B + 1])
                again = hip.guidance_stats(pred, gp, branches, nhwc)
                torch.cuda.synchronize()
                tag = (shape, branches, nhwc, phi)
                assert torch.isnan(band[0]).all() and torch.isnan(band[B + 1]).all(), tag
                assert torch.equal(got, again), tag                                    # fixed order, no atomics
                assert torch.equal(pred, pred0) and torch.equal(gp, gp0), tag
                errs = [relerr(got[:, k], want[:, k]) for k in range(3)]               # f, s_c, s_e
                err_mean = float(((got[:, 3].double() - want[:, 3]).abs() / want[:, 2]).max())   # the mean, in units of the deviation
                # the stock composition on the device, for the record: fp32 torch.std over the same values
                br = [b.float() for b in gr.split(pred, shape, branches, nhwc)]
                e0 = br[0] + G * (br[1] - br[0]) if branches == 2 else br[0] + G * (br[1] - br[0]) + G_ID * (br[2] - br[1])
                f_t = (1.0 - phi) + phi * br[-1].reshape(B, -1).std(dim=1) / e0.reshape(B, -1).std(dim=1)
                err_t = relerr(f_t, want[:, 0])
                print(f"guidance_stats {tag}: rel err f {errs[0]:.2e} s_c {errs[1]:.2e} s_e {errs[2]:.2e}, mean/s_e {err_mean:.2e}; torch.std f {err_t:.2e}")
                worst, worst_torch = max(worst, *errs), max(worst_torch, err_t)
                assert max(errs) <= 1e-6, (tag, errs)
                assert err_mean <= 1e-3, (tag, err_mean)     # fp32 rounding of a mean of size 10 against a deviation of 0.01 is 1e-4
    print(f"guidance_stats {shape}: worst rel err {worst:.2e} (torch.std composition {worst_torch:.2e})")


def test_guidance_stats_constant_image_gives_factor_one(hip_env):
    hip, _, dev, _ = hip_env
    for branches in (2, 3):
        for shape in ((2, 4, 15, 17), (1, 4, 16, 16)):
            B = shape[0]
            pred = torch.full((branches * B,) + shape[1:], 3.0, device=dev)
            if branches == 3:
                pred[B:2 * B] = 0.5                                                    # e0 is still one value per image
            if B > 1:                                                                  # c of the last image: an ordinary one
                pred[-1] = torch.randn(shape[1:], device=dev, generator=torch.Generator(device=dev).manual_seed(3))
            got = hip.guidance_stats(pred, guide_params(dev, 0.7), branches, False)
            assert float(got[0, 0]) == 1.0 and float(got[0, 2]) == 0.0, got        # s_e == 0 -> f = 1
            if B > 1:
                want = gr.stats(pred, guide_params(dev, 0.7), shape, branches, False)
                assert relerr(got[1, :3], want[1, :3]) <= 1e-6


@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_sampler_step_guided_matches_restatement(hip_env, si):
    hip, _, dev, _ = hip_env
    shape = SHAPES[si]
    B, C, H, W = shape
    K = 3
    gen = torch.Generator(device=dev).manual_seed(60 + si)
    worst, cases = {"none": 0.0, "given": 0.0, "kernel": 0.0}, 0
    for branches in (2, 3):
        for nhwc in (False, True):
            for blend in (False, True):
                for w in (-1, 0, 2):
                    for with_noise in (False, True):
                        cases += 1
                        save_x = cases % 2 == 0
                        pred = gr.draw(shape, branches, nhwc, gen, dev, first_pair=first_pair(shape, si + cases))
                        x = torch.randn(shape, generator=gen, device=dev)
                        hist = torch.randn((K,) + shape, generator=gen, device=dev)
                        saved = torch.randn(shape, generator=gen, device=dev)
                        noise = torch.randn(shape, generator=gen, device=dev) if with_noise else None
                        coefs = (torch.rand(16, generator=gen, device=dev) * 2 - 1).tolist()
                        row = torch.tensor([-99.0] + coefs[:6] + [0.8, float(w), float(save_x)] + coefs[6:9] + [0.0] + coefs[9:11],
                                           dtype=f32, device=dev)                      # row[0] is ignored: g comes from gp
                        gp = guide_params(dev, 0.7)
                        edit = None
                        if blend:
                            per_image = cases % 4 < 2
                            keep = torch.rand((B if per_image else 1, H, W), generator=gen, device=dev)
                            x0 = torch.randn((B if not per_image else 1, C, H, W), generator=gen, device=dev)
                            edit = (keep, x0, torch.randn(shape, generator=gen, device=dev))
                        want_stat = gr.stats(pred, gp, shape, branches, nhwc)
                        kern_stat = hip.guidance_stats(pred, gp, branches, nhwc)
                        for mode, gstat, want_f, bound in (("none", None, None, 1e-6), ("given", want_stat.float(), want_stat.float(), 1e-6),
                                                           ("kernel", kern_stat, want_stat, 2e-6)):
                            want, m, want_in = gr.step(pred, x, row, gp, want_f, hist, saved, noise, branches, nhwc, edit)
                            h, s = hist.clone(), saved.clone()
                            x_in = torch.full((branches * B,) + shape[1:], float("nan"), device=dev)
                            out = hip.sampler_step_guided(pred, x, row, gp, gstat=gstat, branches=branches, hist=h, saved=s, noise=noise, x_in=x_in,
                                                          pred_nhwc=nhwc, edit=edit)
                            torch.cuda.synchronize()
                            tag = (shape, branches, nhwc, blend, w, with_noise, mode)
                            errs = [rel(out, want), rel(x_in[:B], want_in)]
                            assert all(torch.equal(x_in[r * B:(r + 1) * B], x_in[:B]) for r in range(1, branches)), tag
                            for k in range(K):
                                errs.append(rel(h[k], m) if k == w else float(not torch.equal(h[k], hist[k])))
                            errs.append(float(not torch.equal(s, x if save_x else saved)))
                            worst[mode] = max(worst[mode], *errs)
                            assert max(errs) <= bound, (tag, errs)
    print(f"sampler_step_guided {shape}: {cases} cases x 3, worst rel err {worst}")


@pytest.mark.parametrize("nhwc", [False, True])
def test_guided_two_branches_are_the_plain_kernels_bits(hip_env, nhwc):
    """branches = 2, no gstat, gp[0] == row[0]: out, hist, saved and x_in of e4t_sampler_step (cfg = 1), with the blend those of
    e4t_sampler_step_edit, bit for bit: the three entry points are instances of one kernel body"""
    hip, _, dev, _ = hip_env
    gen = torch.Generator(device=dev).manual_seed(71)
    shape = (2, 4, 15, 17)
    B, C, H, W = shape
    for w, save_x, with_noise in ((-1, False, False), (0, True, True), (2, True, False)):
        pred = gr.draw(shape, 2, nhwc, gen, dev, first_pair=w + 1)
        x = torch.randn(shape, generator=gen, device=dev)
        hist = torch.randn((3,) + shape, generator=gen, device=dev)
        saved = torch.randn(shape, generator=gen, device=dev)
        noise = torch.randn(shape, generator=gen, device=dev) if with_noise else None
        coefs = (torch.rand(16, generator=gen, device=dev) * 2 - 1).tolist()
        row = torch.tensor([G] + coefs[:6] + [0.8, float(w), float(save_x)] + coefs[6:9] + [0.0] + coefs[9:11], dtype=f32, device=dev)
        gp = guide_params(dev, 0.0, g=G, g_id=123.0)                                  # g_id and phi play no part here
        edit = (torch.rand((B, H, W), generator=gen, device=dev), torch.randn((1, C, H, W), generator=gen, device=dev),
                torch.randn(shape, generator=gen, device=dev))
        for e in (None, edit):
            res = []
            for guided in (False, True):
                h, s = hist.clone(), saved.clone()
                x_in = torch.full((2 * B,) + shape[1:], float("nan"), device=dev)
                kw = dict(hist=h, saved=s, noise=noise, x_in=x_in, pred_nhwc=nhwc, edit=e)
                out = hip.sampler_step_guided(pred, x, row, gp, **kw) if guided else hip.sampler_step(pred, x, row, cfg=True, **kw)
                res.append((out, h, s, x_in))
            for a, b in zip(*res):
                assert torch.equal(a, b), (w, e is not None)


def test_guided_x_in_copies_aliasing_and_refusals(hip_env):
    hip, _, dev, ops = hip_env
    from e4t import _C
    gen = torch.Generator(device=dev).manual_seed(72)
    shape = (2, 4, 5, 13)
    pred = gr.draw(shape, 3, False, gen, dev, first_pair=1)
    x = torch.randn(shape, generator=gen, device=dev)
    row = torch.tensor([0.0, 0.9, 0.2, 1.1, 0.0, -0.4, 0.0, 0.7, -1.0, 0.0] + [0.0] * 6, dtype=f32, device=dev)
    gp = guide_params(dev, 1.0)
    gstat = hip.guidance_stats(pred, gp, 3, False)
    want, _, want_in = gr.step(pred, x, row, gp, gr.stats(pred, gp, shape, 3, False), None, None, None, 3, False)
    x_in = torch.full((6,) + shape[1:], float("nan"), device=dev)
    xi = x.clone()
    got = hip.sampler_step_guided(pred, xi, row, gp, gstat=gstat, branches=3, x_in=x_in, out=xi)         # out aliases x
    assert got is xi and rel(xi, want) <= 2e-6
    assert rel(x_in[:2], want_in) <= 2e-6 and torch.equal(x_in[2:4], x_in[:2]) and torch.equal(x_in[4:], x_in[:2])
    # refusals: validated on the host, nothing is launched
    with pytest.raises(_C.E4TError, match="x_in_copies = 4"):
        hip.sampler_step_guided(pred, x, row, gp, branches=3, x_in=torch.empty((8,) + shape[1:], device=dev))
    lib, p = hip.lib, x.data_ptr()
    keep, x0, n0 = (torch.zeros(shape, device=dev).data_ptr() for _ in range(3))

    def raw(keep=None, x0=None, n0=None, branches=3, copies=0, gp_=gp.data_ptr()):
        return lib.e4t_sampler_step_guided(pred.data_ptr(), p, p, None, None, None, x_in.data_ptr() if copies else None, row.data_ptr(), gp_, None,
                                           keep, x0, n0, 2, 4, 65, 0, branches, 0, copies, 0, 0, None)

    for mixed in ((keep, None, None), (None, x0, None), (None, None, n0), (keep, x0, None), (keep, None, n0), (None, x0, n0)):
        assert raw(*mixed) == -22 and b"keep, x0 and n0" in lib.e4t_last_error(), mixed
    assert raw(copies=4) == -22 and b"x_in_copies" in lib.e4t_last_error()
    assert raw(branches=1) == -22 and b"branches" in lib.e4t_last_error()
    assert raw(branches=4) == -22
    assert raw(gp_=None) == -22


# ---- the pipeline -------------------------------------------------------------------------------------------------------------
MODES = {"rescale": dict(guidance_rescale=0.7), "identity": dict(identity_guidance_scale=7.0),
         "both": dict(guidance_rescale=0.7, identity_guidance_scale=7.0), "both+edit": dict(guidance_rescale=0.7, identity_guidance_scale=7.0)}


NOISE_SEED = 2      # of the two samplers that draw noise (DDIM with eta > 0, Euler-ancestral); see test_pipeline_guided_sampling


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name,eta", SAMPLERS)
def test_pipeline_guided_sampling(edit_pipe, name, eta, mode):
    """Fused against generic is a comparison through a bf16 model: the two loops' latents differ in last fp32 bits (2e-8 .. 9e-8
    rel-L2 per step, measured), the UNet's bf16 cast of its input absorbs that, and the result stays at 1e-7, unless one of the
    2048 latent values lies so close to a bf16 rounding boundary that the two loops round it apart (about 6e-8 / 2^-8 = 1.5e-5
    per differing value and step).  Then one input pixel moves by a bf16 ulp and the difference jumps in that step, by a size
    that depends on the pixel, and the guidance scales multiply it.  Measured over 64 runs (DDIM eta 0.5 and Euler-ancestral x
    plain / rescale / identity / both x noise seeds 1..8, 4 steps, per-step figures): 5 jumps, 8.6e-6 (plain sampling, code that
    this feature leaves alone), 1.1e-5, 1.2e-5, 4.2e-4 and, DDIM eta 0.5 / both / seed 1 at step 3, 1.6e-3 after 2.5e-8 and
    3.4e-8; the other 59 end at 1e-8 .. 9e-8.  The update itself is held to 2e-6 against float64 above.  The jump says nothing
    about the fused step, so the noise seed is one without it; the tolerance is test_sampler_fused_gpu.py's."""
    pipe, image, lat0, photo, mask, keep, x0 = edit_pipe
    kw, steps = dict(MODES[mode]), 4
    want_calls = steps
    if mode == "both+edit":
        kw.update(init_image=photo, strength=0.5, mask_image=mask)
        steps, want_calls = 6, 3
    want_calls += name == "plms"
    eager, n_e = call(pipe, image, lat0, name, eta, 5.0, steps, False, seed=NOISE_SEED, **kw)
    graph, n_g = call(pipe, image, lat0, name, eta, 5.0, steps, True, seed=NOISE_SEED, **kw)
    generic, n_s = call(pipe, image, lat0, name, eta, 5.0, steps, False, fused=False, seed=NOISE_SEED, **kw)
    assert (n_e, n_g, n_s) == (want_calls,) * 3
    assert torch.isfinite(eager).all()
    assert torch.equal(eager, graph), rel(graph, eager)
    r = rel(eager, generic)
    print(f"{name} eta={eta} {mode}: fused vs generic rel-L2 {r:.2e}")
    assert r < 1e-3, r
    if mode == "both+edit":
        held = (keep == 1).expand(2, 4, 16, 16)
        for out in (eager, graph, generic):
            assert torch.equal(out[held], x0.expand(2, 4, 16, 16)[held])            # outside the mask: the photograph's latent, bitwise
        free = (keep == 0).expand(2, 4, 16, 16)
        assert not torch.equal(eager[free], x0.expand(2, 4, 16, 16)[free])


@pytest.mark.parametrize("name,eta", SAMPLERS)
def test_pipeline_options_act_and_plain_call_untouched(tiny_pipe, name, eta):
    pipe, image, lat0 = tiny_pipe
    before, _ = call(pipe, image, lat0, name, eta, 5.0, 4, True)
    same, _ = call(pipe, image, lat0, name, eta, 5.0, 4, True, identity_guidance_scale=5.0)      # g_id == g: plain guidance on c, another route
    assert rel(same, before) < 1e-3
    for kw in (dict(guidance_rescale=0.7), dict(identity_guidance_scale=9.0)):
        assert not torch.equal(call(pipe, image, lat0, name, eta, 5.0, 4, True, **kw)[0], before), kw   # the options do enter the result
    after, _ = call(pipe, image, lat0, name, eta, 5.0, 4, True)
    assert torch.equal(after, before)                                               # a plain call: the same bits before and after
