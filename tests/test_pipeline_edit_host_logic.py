"""CPU, through the op emulation: img2img / masked inpainting take the pipeline's generic step + blend loop (there is
no sampler kernel here), for every sampler on the tiny models: the schedule is truncated by `strength`, the start is the photograph
at the first kept timestep's level, held latent pixels end at the photograph's latent exactly, `latents=` is taken as n0, and a
plain call is unchanged by an edit call."""
import pytest
import torch

from test_pipeline_host_logic import _pipeline
from test_train_step_host_logic import build
from test_unet_host_logic import emu_fp32  # noqa: F401


@pytest.fixture()
def edit_pipe(emu_fp32):  # noqa: F811
    from e4t.vae import VAEDecoder, VAEEncoder
    _, _, n_unet, n_enc, text = build()
    torch.manual_seed(3)
    vae = VAEDecoder(block_out_channels=(64, 64)).requires_grad_(False)
    enc = VAEEncoder(block_out_channels=(64, 64)).requires_grad_(False)
    pipe, _ = _pipeline(n_unet, n_enc, text, vae)
    g = torch.Generator().manual_seed(5)
    image = torch.rand(1, 3, 64, 64, generator=g) * 2 - 1
    photo = torch.rand(1, 3, 32, 32, generator=g) * 2 - 1
    lat0 = torch.randn(2, 4, 16, 16, generator=g)
    mask = torch.zeros(32, 32)
    mask[:, 13:] = 1.0                                    # latent column 6 is half covered: keep = 0.5 there
    return pipe, enc, image, photo, lat0, mask


def run(pipe, image, lat0, steps=4, **kw):
    calls = []
    out = pipe("a painting of *s", height=32, width=32, num_inference_steps=steps, guidance_scale=3.0, num_images_per_prompt=2, image=image,
               latents=lat0.clone(), output_type="latent", generator=torch.Generator().manual_seed(1),
               callback=lambda i, t, l: calls.append(float(t)), **kw).images
    return out, calls


@pytest.mark.parametrize("name", ["ddim", "plms", "euler_ancestral", "dpm_solver++"])       # one per family, the doubled call, noise, multistep
def test_edit_takes_the_generic_loop(edit_pipe, name):
    from e4t.schedulers import SCHEDULER_MAPPING
    pipe, enc, image, photo, lat0, mask = edit_pipe
    pipe.scheduler = SCHEDULER_MAPPING[name].stable_diffusion()
    before, plain_calls = run(pipe, image, lat0, steps=2)
    pipe.scheduler.set_timesteps(4)
    full = pipe.scheduler.timesteps.tolist()
    with pytest.raises(ValueError, match="vae_encoder"):
        run(pipe, image, lat0, init_image=photo)
    pipe.vae_encoder = enc
    x0 = enc.encode_sample(photo, torch.zeros(1, 4, 16, 16)).float()
    keep = 1.0 - torch.nn.functional.avg_pool2d(mask[None, None], 2)[0, 0]
    out, calls = run(pipe, image, lat0, init_image=photo, strength=0.5, mask_image=mask)
    kept = 2                                               # 4 steps at strength 0.5
    assert len(calls) == (kept + 1 if name == "plms" else kept)
    assert calls[0] < full[0] and calls[-1] == full[-1]                        # the tail of the 4-step schedule
    held = (keep == 1).expand(2, 4, 16, 16)
    assert torch.isfinite(out).all() and torch.equal(out[held], x0.expand(2, 4, 16, 16)[held])
    assert not torch.equal(out[~held], x0.expand(2, 4, 16, 16)[~held])
    # img2img without a mask: the first model call sees a*x0 + s*n0 with n0 = the caller's latents
    seen = []
    pipe.scheduler.set_timesteps(4, begin=2)
    a, s = pipe.scheduler.noise_level(pipe.scheduler.timesteps[0])
    orig = pipe._model_step
    pipe._model_step = lambda latents, t, st, x_in=None: (seen.append(latents.clone()), orig(latents, t, st, x_in=x_in))[1]
    try:
        img2img, calls = run(pipe, image, lat0, init_image=photo, strength=0.5)
    finally:
        del pipe._model_step
    assert torch.equal(seen[0], a * x0 + s * lat0) and len(calls) == (kept + 1 if name == "plms" else kept)
    assert not torch.equal(img2img, out)
    with pytest.raises(ValueError, match="graph replay"):
        run(pipe, image, lat0, init_image=photo, use_graph=True)              # no sampler kernel here: edit mode is not fused
    with pytest.raises(ValueError, match="init_image"):
        run(pipe, image, lat0, mask_image=mask)
    with pytest.raises(ValueError, match="no denoising step"):
        run(pipe, image, lat0, init_image=photo, strength=0.1)
    after, calls = run(pipe, image, lat0, steps=2)
    assert torch.equal(after, before) and calls == plain_calls                        # a plain call: as before the edit calls


def test_mask_and_image_inputs(edit_pipe):
    """PIL inputs are resized to (height, width); a soft mask stays soft; the keep map is 1 - the 2 x 2 (8 x 8 at SD's VAE) block mean"""
    from PIL import Image
    pipe, enc, image, photo, lat0, mask = edit_pipe
    pipe.vae_encoder = enc
    dev = torch.device("cpu")
    soft = torch.linspace(0, 1, 32).expand(32, 32).contiguous()
    _, x0, keep = pipe.prepare_edit(photo, 0.5, soft, 6, 2, 32, 32, dev)
    assert x0.shape == (1, 4, 16, 16) and keep.shape == (256,)
    torch.testing.assert_close(keep.view(16, 16), 1.0 - torch.nn.functional.avg_pool2d(soft[None, None], 2)[0, 0])
    pil_mask = Image.fromarray((mask.numpy() * 255).astype("uint8")).resize((64, 64), Image.NEAREST)
    pil_photo = Image.fromarray(((photo[0].permute(1, 2, 0).numpy() + 1) * 127.5).round().astype("uint8")).resize((64, 64))
    begin, x0p, keep_p = pipe.prepare_edit(pil_photo, 1.0, pil_mask, 6, 2, 32, 32, dev)
    assert begin == 0 and x0p.shape == (1, 4, 16, 16) and keep_p.shape == (256,)
    assert float(keep_p.min()) == 0.0 and float(keep_p.max()) == 1.0
    assert pipe.prepare_edit(photo, 0.5, None, 6, 2, 32, 32, dev)[2] is None
    with pytest.raises(ValueError, match="RGB images of 32 x 32"):
        pipe.prepare_edit(torch.zeros(1, 3, 16, 16), 0.5, None, 6, 2, 32, 32, dev)
    both = pipe.prepare_edit(torch.cat([photo, -photo]), 0.5, None, 6, 2, 32, 32, dev)[1]
    assert both.shape == (2, 4, 16, 16)
    torch.testing.assert_close(both[:1], x0)
