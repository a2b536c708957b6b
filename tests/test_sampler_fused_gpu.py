"""-m gpu: e4t_sampler_step (guidance + any linear sampler update in one kernel) against a torch restatement of its row
contract, bit-identity of a DDIM row with e4t_guided_step, and the pipeline's fused loop for every sampler on the tiny
models: graph replay == fused eager bit for bit, fused close to the generic scale_model_input / step path."""
import pytest
import torch

pytestmark = pytest.mark.gpu

f32 = torch.float32
SAMPLERS = [("ddim", 0.0), ("ddim", 0.5), ("plms", 0.0), ("lms", 0.0), ("euler", 0.0), ("euler_ancestral", 0.0), ("dpm_solver++", 0.0)]


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def reference(pred, x, row, hist, saved, noise, cfg, nhwc):
    """the header's contract in float64 on the fp32 inputs; pred in its given layout"""
    r = row.double().tolist()
    g, a_e, a_x, c_x, c_s, c_m, c_n, k_in, w, save_x = r[:10]
    B, C, H, W = x.shape
    p = pred.double()
    if nhwc:
        p = p.reshape(-1, H * W, C).permute(0, 2, 1).reshape(-1, C, H, W)
    p = p.reshape(-1, C, H, W)
    e = p[:B] + g * (p[B:] - p[:B]) if cfg else p
    xd = x.double()
    m = a_e * e + a_x * xd
    out = c_x * xd + c_m * m
    if saved is not None:
        out = out + c_s * saved.double()
    if hist is not None:
        for k in range(hist.shape[0]):
            out = out + r[10 + k] * hist[k].double()
    if noise is not None:
        out = out + c_n * noise.double()
    return out, m, k_in * out


def test_sampler_step_matches_restatement(hip_env):
    hip, _, dev, _ = hip_env
    g = torch.Generator(device=dev).manual_seed(11)
    K, worst, cases = 3, 0.0, 0
    for B in (1, 2, 3):
        H, W = 7, 9 + B                                   # HW = 70, 77, 84: not multiples of 256
        for cfg in (False, True):
            for nhwc in (False, True):
                for w in (-1, 0, 1, 2):
                    for save_x in (False, True):
                        for with_noise in (False, True):
                            shape = (B, 4, H, W)
                            x = torch.randn(shape, generator=g, device=dev)
                            pshape = ((2 if cfg else 1) * B, H, W, 4) if nhwc else ((2 if cfg else 1) * B, 4, H, W)
                            pred = torch.randn(pshape, generator=g, device=dev)
                            hist = torch.randn((K,) + shape, generator=g, device=dev)
                            saved = torch.randn(shape, generator=g, device=dev)
                            noise = torch.randn(shape, generator=g, device=dev) if with_noise else None
                            coefs = (torch.rand(14, generator=g, device=dev) * 2 - 1).tolist()
                            row = torch.tensor([7.5] + coefs[:6] + [0.8, float(w), float(save_x)] + coefs[6:9] + [0.0, 0.0, 0.0],
                                               dtype=f32, device=dev)
                            want, m, want_in = reference(pred, x, row, hist, saved, noise, cfg, nhwc)
                            h0, s0 = hist.clone(), saved.clone()
                            x_in = torch.full(((2 if cfg else 1) * B,) + shape[1:], float("nan"), device=dev)
                            out = hip.sampler_step(pred, x, row, hist=hist, saved=saved, noise=noise, x_in=x_in, cfg=cfg, pred_nhwc=nhwc)
                            torch.cuda.synchronize()
                            errs = [rel(out, want), rel(x_in[:B], want_in), rel(x_in[B:], want_in) if cfg else 0.0]
                            for k in range(K):
                                errs.append(rel(hist[k], m) if k == w else float(not torch.equal(hist[k], h0[k])))
                            errs.append(float(not torch.equal(saved, x if save_x else s0)))
                            worst = max(worst, *errs)
                            cases += 1
                            assert max(errs) <= 1e-6, (B, cfg, nhwc, w, save_x, with_noise, errs)
    # in place on x, no saved / hist / x_in, as the pipeline's eager DDIM rows use it
    x = torch.randn((2, 4, 5, 13), generator=g, device=dev)
    pred = torch.randn((4, 4, 5, 13), generator=g, device=dev)
    row = torch.tensor([3.0, 0.9, 0.2, 1.1, 0.0, -0.4, 0.0, 1.0, -1.0, 0.0] + [0.0] * 6, dtype=f32, device=dev)
    want = reference(pred, x, row, None, None, None, True, False)[0]
    hip.sampler_step(pred, x, row, cfg=True, out=x)
    assert rel(x, want) <= 1e-6
    print(f"sampler_step: {cases} cases, worst rel err {worst:.2e}")


def test_ddim_row_is_bit_identical_to_guided_step(hip_env):
    hip, _, dev, _ = hip_env
    from e4t.schedulers import DDIMScheduler
    g = torch.Generator(device=dev).manual_seed(12)
    sch = DDIMScheduler.stable_diffusion()
    sch.set_timesteps(20)
    for eta in (0.0, 0.7):
        plan = sch.fused_plan(guidance_scale=7.5, eta=eta)
        for i in (0, 7, 19):
            r = plan.table[i].tolist()
            row = torch.tensor(r, dtype=f32, device=dev)
            coef = torch.tensor([r[0], r[3], r[5], r[6]], dtype=f32, device=dev)
            for cfg in (False, True):
                for nhwc in (False, True):
                    x = torch.randn((2, 4, 64, 64), generator=g, device=dev)
                    pred = torch.randn(((2 if cfg else 1) * 2, 64, 64, 4) if nhwc else ((2 if cfg else 1) * 2, 4, 64, 64), generator=g, device=dev)
                    noise = torch.randn_like(x) if eta > 0 else None
                    want = hip.guided_step(pred, x, coef, noise=noise, cfg=cfg, pred_nhwc=nhwc)
                    got = hip.sampler_step(pred, x, row, noise=noise, cfg=cfg, pred_nhwc=nhwc)
                    assert torch.equal(got, want), (eta, i, cfg, nhwc)


@pytest.fixture(scope="module")
def tiny_pipe(hip_env):
    """the tiny models of tests/test_model_gpu.py::test_pipeline_graph_replay_equals_eager"""
    from word_tokenizer import WordTokenizer
    from test_train_step_host_logic import build
    from e4t.pipeline_stable_diffusion_e4t import StableDiffusionE4TPipeline
    from e4t.schedulers import DDIMScheduler
    from e4t.text import CLIPTextModel
    from e4t.vae import VAEDecoder
    dev = torch.device("cuda:0")
    _, _, n_unet, n_enc, text_t = build()
    text = CLIPTextModel(**text_t.config).requires_grad_(False)
    text.load_state_dict(text_t.state_dict())
    vae = VAEDecoder(block_out_channels=(64, 64)).requires_grad_(False)
    pipe = StableDiffusionE4TPipeline(vae=vae, text_encoder=text, tokenizer=WordTokenizer(), unet=n_unet, e4t_encoder=n_enc,
                                      scheduler=DDIMScheduler.stable_diffusion(), safety_checker=None,
                                      e4t_config=dict(placeholder_token="*s", domain_class_token="art", domain_embed_scale=0.1)).to(dev)
    g = torch.Generator().manual_seed(5)
    image = torch.rand(1, 3, 64, 64, generator=g) * 2 - 1
    lat0 = torch.randn(2, 4, 16, 16, generator=g)
    return pipe, image, lat0


@pytest.mark.parametrize("guidance", [1.0, 5.0])
@pytest.mark.parametrize("name,eta", SAMPLERS)
def test_pipeline_fused_sampler(tiny_pipe, name, eta, guidance):
    from e4t.schedulers import SCHEDULER_MAPPING
    pipe, image, lat0 = tiny_pipe
    pipe.scheduler = SCHEDULER_MAPPING[name].stable_diffusion()
    steps = 4

    def run(use_graph, fused=True, seed=1):
        calls = []
        pipe._fused_sampling = fused
        try:
            out = pipe("a painting of *s", height=32, width=32, num_inference_steps=steps, guidance_scale=guidance, num_images_per_prompt=2,
                       image=image, latents=lat0.clone(), output_type="latent", eta=eta, use_graph=use_graph,
                       generator=torch.Generator(device="cuda").manual_seed(seed), callback=lambda i, t, l: calls.append(i)).images
        finally:
            pipe._fused_sampling = True
        assert len(calls) == (steps + 1 if name == "plms" else steps), calls
        return out

    eager = run(False)
    graph = run(True)
    generic = run(False, fused=False)
    assert torch.isfinite(eager).all()
    assert torch.equal(eager, graph), rel(graph, eager)
    r = rel(eager, generic)
    print(f"{name} eta={eta} guidance={guidance}: fused vs generic rel-L2 {r:.2e}")
    assert r < 1e-3, r
    if name == "euler_ancestral":
        assert torch.equal(run(True), graph)                        # seeded: the same noise again
        assert not torch.equal(run(True, seed=2), graph)            # and the noise does enter the update
