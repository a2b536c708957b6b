"""CPU: FreeU's host logic (e4t/freeu.py, the up blocks, the pipeline, the command line) on the op emulation, and the definition itself:
the four-frequency closed form against the torch.fft recipe."""
import importlib
import json
import os
import sys

import pytest
import torch

import e4t_oracle as orc
import freeu_reference as ref
from test_unet_host_logic import build_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SD14_LIKE = dict(block_out_channels=(64, 128, 256, 256))       # SD-1.4's layout (320, 640, 1280, 1280), scaled down (the op emulation's convolutions need >= 64 channels)
TEN = {"up_blocks.0.resnets.0": 1, "up_blocks.0.resnets.1": 1, "up_blocks.0.resnets.2": 1,
       "up_blocks.1.resnets.0": 1, "up_blocks.1.resnets.1": 1, "up_blocks.1.resnets.2": 1,
       "up_blocks.2.resnets.0": 1, "up_blocks.2.resnets.1": 2, "up_blocks.2.resnets.2": 2, "up_blocks.3.resnets.0": 2}


class SpyBackend(ref.FreeuEmuBackend):
    def __init__(self, **kw):
        super().__init__(**kw)
        self.calls = []

    def freeu_stats(self, h, k, B, H, W, version=2, ws=None):
        self.calls.append(("stats", B, H, W, h.shape[1], k.shape[1], version))
        return super().freeu_stats(h, k, B, H, W, version, ws)

    def freeu_apply(self, h, k, ws, B, H, W, b, s, version=2, out_h=None, out_k=None):
        self.calls.append(("apply", B, H, W, h.shape[1], k.shape[1], version, b, s))
        return super().freeu_apply(h, k, ws, B, H, W, b, s, version, out_h, out_k)


@pytest.fixture()
def emu_fp32():
    from e4t import ops
    old_b, old_act = ops.set_backend(SpyBackend(round_bf16=False)), ops.ACT
    ops.ACT = torch.float32
    yield ops
    ops.set_backend(old_b)
    ops.ACT = old_act


def _cfg():
    return dict(orc.tiny_unet_config(ctx_dim=64), **SD14_LIKE)


def _inputs(B=2, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 4, 16, 16, generator=g), torch.tensor([3, 977][:B]), torch.randn(B, 7, 64, generator=g)


# ---- the definition ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(2, 2), (2, 3), (3, 5), (7, 7), (6, 10), (16, 16)])
def test_closed_form_equals_the_fft_recipe(H, W):
    g = torch.Generator().manual_seed(H * 100 + W)
    k = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64) * 2 + 0.5
    for s in (0.9, 0.2, 0.0):
        a, b = ref.skip_closed(k, s), ref.skip_fft(k, s)
        assert float((a - b).abs().max()) <= 1e-12, (H, W, s, float((a - b).abs().max()))


def test_unit_factors_are_the_identity():
    g = torch.Generator().manual_seed(0)
    h, k = torch.randn(2, 16, 5, 6, generator=g, dtype=torch.float64), torch.randn(2, 8, 5, 6, generator=g, dtype=torch.float64)
    for version in (1, 2):
        h2, k2 = ref.freeu_pair(h, k, 1.0, 1.0, version)
        assert torch.equal(h2, h) and torch.equal(k2, k)
    h2, k2 = ref.freeu_pair(h, k, 1.4, 0.2, 2)
    assert torch.equal(h2[:, 8:], h[:, 8:]) and not torch.equal(h2[:, :8], h[:, :8]) and not torch.equal(k2, k)
    flat = torch.ones(1, 16, 4, 4, dtype=torch.float64) * 3.0                 # max == min: m^ = 0, the backbone is untouched
    assert torch.equal(ref.backbone(flat, 1.4, 2), flat)
    be = ref.FreeuEmuBackend(round_bf16=False)
    hr, kr = ref.to_rows(h).float().contiguous(), ref.to_rows(k).float().contiguous()
    for version in (1, 2):
        h3, k3 = be.freeu_apply(hr, kr, be.freeu_stats(hr, kr, 2, 5, 6, version), 2, 5, 6, 1.0, 1.0, version)
        assert torch.equal(h3, hr) and torch.equal(k3, kr)
    h3, k3 = be.freeu_apply(hr, kr, be.freeu_stats(hr, kr, 2, 5, 6), 2, 5, 6, 1.4, 0.2)
    w_h, w_k = ref.freeu_pair(ref.to_nchw(hr, 2, 5, 6), ref.to_nchw(kr, 2, 5, 6), 1.4, 0.2)
    torch.testing.assert_close(h3.double(), ref.to_rows(w_h), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(k3.double(), ref.to_rows(w_k), rtol=1e-6, atol=1e-6)


# ---- marking ---------------------------------------------------------------------------------------------------------------------------
def test_apply_freeu_marks_the_ten_resblocks_of_the_sd14_layout():
    from e4t import freeu
    from e4t.models.resnet import ResnetBlock2D
    _, nat = build_pair(_cfg())
    assert freeu.get_state(nat) is None
    st = freeu.apply_freeu(nat, 1.3, 1.4, 0.9, 0.2)
    assert freeu.get_state(nat) is st and st.version == 2 and st.stages == TEN and list(st.stages) == list(TEN)
    marked = {n: m._freeu[1] for n, m in nat.named_modules() if isinstance(m, ResnetBlock2D) and m._freeu is not None}
    assert marked == TEN
    assert all(m._freeu[0] is st for m in nat.modules() if isinstance(m, ResnetBlock2D) and m._freeu is not None)
    assert st.params(1) == (1.3, 0.9) and st.params(2) == (1.4, 0.2)
    freeu.remove_freeu(nat)
    assert freeu.get_state(nat) is None and not any("_freeu" in m.__dict__ for m in nat.modules())
    for bad in (dict(b1=0.9), dict(b2=float("inf")), dict(s1=1.1), dict(s2=-0.1), dict(version=3)):
        with pytest.raises(ValueError):
            freeu.apply_freeu(nat, **dict(dict(b1=1.3, b2=1.4, s1=0.9, s2=0.2), **bad))
    assert freeu.get_state(nat) is None


def test_remove_freeu_restores_the_model_bitwise_and_the_spy_counts_two_calls_per_mark(emu_fp32):
    from e4t import freeu
    _, nat = build_pair(_cfg(), seed=2)
    spy = emu_fp32.backend()
    x, t, ctx = _inputs()
    with torch.no_grad():
        y0 = nat(x, t, ctx).sample.clone()
        assert spy.calls == []                                   # an unmarked model never reaches the ops
        freeu.apply_freeu(nat, 1.3, 1.4, 0.9, 0.2)
        enc = nat(x, t, ctx, return_encoder_outputs=True)
        assert spy.calls == [] and len(enc["down_block_samples"]) == 13      # the encoder pass stops before the up blocks
        y1 = nat(x, t, ctx).sample.clone()
        assert len(spy.calls) == 2 * len(TEN)
        assert [c[0] for c in spy.calls] == ["stats", "apply"] * len(TEN)
        # stage by the hidden map's width, every image on its own (B = 2), maps from 2x2 to 16x16
        assert [(c[4], c[7], c[8]) for c in spy.calls if c[0] == "apply"] == [(256, 1.3, 0.9)] * 7 + [(128, 1.4, 0.2)] * 3
        assert [c[2:4] for c in spy.calls if c[0] == "apply"] == [(2, 2)] * 3 + [(4, 4)] * 3 + [(8, 8)] * 3 + [(16, 16)]
        freeu.apply_freeu(nat, 1.0, 1.0, 1.0, 1.0)               # unit factors: the transform runs and changes nothing
        y_id = nat(x, t, ctx).sample.clone()
        freeu.remove_freeu(nat)
        del spy.calls[:]
        y2 = nat(x, t, ctx).sample.clone()
    assert spy.calls == []
    assert float((y1 - y0).abs().max()) > 1e-4
    assert torch.equal(y_id, y0)
    assert torch.equal(y2, y0)


def test_a_marked_model_asked_for_a_gradient_raises(emu_fp32):
    from e4t import freeu
    _, nat = build_pair(_cfg())
    for n, p in nat.named_parameters():
        p.requires_grad_("wo" in n)
    freeu.apply_freeu(nat, 1.3, 1.4, 0.9, 0.2)
    x, t, ctx = _inputs()
    with pytest.raises(RuntimeError, match="sampling-only"):
        nat(x, t, ctx)
    with torch.no_grad():
        nat(x, t, ctx)
    freeu.remove_freeu(nat)
    nat(x, t, ctx).sample.sum().backward()                       # and the unmarked model trains as before


# ---- against the oracle --------------------------------------------------------------------------------------------------------------
def _hook_oracle(unet, stages, params, version):
    """FreeU on the oracle UNet: a forward-pre-hook on every marked up-block ResBlock splits the concatenated input at C_h, transforms the
    two parts by the float64 definition and concatenates them again"""
    widths = {}
    prev = SD14_LIKE["block_out_channels"][-1]
    for i, blk in enumerate(unet.up_blocks):
        out_ch = blk.resnets[0].conv1.out_channels
        for j in range(len(blk.resnets)):
            widths[f"up_blocks.{i}.resnets.{j}"] = prev if j == 0 else out_ch
        prev = out_ch
    mods = dict(unet.named_modules())
    for name, stage in stages.items():
        c_h, (b, s) = widths[name], params[stage]

        def pre(mod, args, c_h=c_h, b=b, s=s):
            x = args[0]
            h2, k2 = ref.freeu_pair(x[:, :c_h], x[:, c_h:], b, s, version)
            return (torch.cat([h2, k2], 1).to(x.dtype),) + tuple(args[1:])
        mods[name].register_forward_pre_hook(pre)


@pytest.mark.parametrize("version", [2, 1])
def test_unet_with_freeu_matches_the_hooked_oracle(emu_fp32, version):
    from e4t import freeu
    r_unet, n_unet = build_pair(_cfg())
    st = freeu.apply_freeu(n_unet, 1.3, 1.4, 0.9, 0.2, version=version)
    x, t, ctx = _inputs()
    with torch.no_grad():
        plain = r_unet(x, t, ctx)
        out_n = n_unet(x, t, ctx).sample
        _hook_oracle(r_unet, st.stages, {1: (1.3, 0.9), 2: (1.4, 0.2)}, version)
        out_r = r_unet(x, t, ctx)
    torch.testing.assert_close(out_n, out_r, rtol=2e-3, atol=2e-4)
    assert float((out_r - plain).abs().max()) > 1e-3             # and FreeU does change the result: the plain oracle is NOT matched


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------------
def test_pipeline_generic_loop_with_and_without_freeu(emu_fp32):
    from e4t import freeu
    from e4t.vae import VAEDecoder
    from test_pipeline_host_logic import _pipeline
    from test_train_step_host_logic import build
    _, _, n_unet, n_enc, text = build()
    torch.manual_seed(3)
    pipe, _ = _pipeline(n_unet, n_enc, text, VAEDecoder(block_out_channels=(64, 64)).requires_grad_(False))
    pipe._fused_sampling = False                                  # the generic scale_model_input / step loop
    g = torch.Generator().manual_seed(5)
    image, lat0 = torch.rand(1, 3, 64, 64, generator=g) * 2 - 1, torch.randn(2, 4, 16, 16, generator=g)
    kw = dict(height=32, width=32, num_inference_steps=3, guidance_scale=4.0, num_images_per_prompt=2, image=image, output_type="latent", use_graph=False)
    spy = emu_fp32.backend()
    off = pipe("a painting of *s", latents=lat0.clone(), **kw).images
    assert spy.calls == []
    st = pipe.enable_freeu()
    assert st is freeu.get_state(n_unet) and (st.b1, st.b2, st.s1, st.s2, st.version) == (1.3, 1.4, 0.9, 0.2, 2)
    on = pipe("a painting of *s", latents=lat0.clone(), **kw).images
    n_marked = len(st.stages)
    # (this model is 64 / 128 / 128 / 128 wide: all of up_blocks.0-2 and up_blocks.3.resnets.0 are stage 1, its last two ResBlocks stage 2)
    assert n_marked == 12 and len(spy.calls) == 3 * 2 * n_marked          # one guided batch (B = 4: both branches) per step
    assert all(c[1] == 4 for c in spy.calls)
    assert float((on - off).abs().max()) > 1e-3                   # a silently ignored option would give the same latents
    assert pipe.enable_freeu(version=1).b1 == 1.2 and pipe.enable_freeu(b1=1.1, s2=0.5).params(1) == (1.1, 0.9)
    pipe.disable_freeu()
    assert freeu.get_state(n_unet) is None
    again = pipe("a painting of *s", latents=lat0.clone(), **kw).images
    assert torch.equal(again, off)


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def _parse(argv, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["inference.py"] + argv)
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module("inference").parse_args()


def test_cli_flags_and_range_errors(monkeypatch, tmp_path):
    from e4t import cli_common as cc, freeu
    from e4t.utils import save_config
    a = _parse([], monkeypatch)
    assert a.freeu is False and a.freeu_version == 2
    _, nat = build_pair(_cfg())
    assert cc.apply_freeu_args(nat, a) is None and freeu.get_state(nat) is None
    a = _parse(["--freeu"], monkeypatch)
    assert (a.freeu, a.freeu_b1, a.freeu_b2, a.freeu_s1, a.freeu_s2, a.freeu_version) == (True, 1.3, 1.4, 0.9, 0.2, 2)
    assert _parse(["--freeu", "--freeu_version", "1"], monkeypatch).freeu_b1 == 1.2
    a = _parse(["--freeu", "--freeu_b1", "1.1", "--freeu_b2", "1.2", "--freeu_s1", "0.8", "--freeu_s2", "0", "--freeu_version", "1"], monkeypatch)
    st = cc.apply_freeu_args(nat, a)
    assert st is freeu.get_state(nat) and (st.b1, st.b2, st.s1, st.s2, st.version) == (1.1, 1.2, 0.8, 0.0, 1) and st.stages == TEN
    save_config(vars(a), str(tmp_path))
    saved = json.load(open(tmp_path / "config.json"))
    assert not any(k.startswith("freeu") for k in saved) and "prompt" in saved
    for bad in (["--freeu", "--freeu_b1", "0.9"], ["--freeu", "--freeu_b2", "inf"], ["--freeu", "--freeu_s1", "1.5"], ["--freeu", "--freeu_s2", "-0.1"],
                ["--freeu", "--freeu_version", "3"], ["--freeu_b1", "1.2"]):
        with pytest.raises(SystemExit):
            _parse(bad, monkeypatch)


def test_abi_rejects_unsupported_shapes_without_a_launch():
    """e4t_freeu_*: -22 and a message before anything is launched (safe without a GPU)"""
    from e4t import _C
    lib = _C.load()
    x = (_C.C.c_char * 64)()
    p = _C.C.addressof(x)
    for H, W, Ch, Ck, version, word in ((1, 4, 16, 8, 2, b">= 2"), (4, 1, 16, 8, 2, b">= 2"), (4, 4, 24, 8, 2, b"multiple of 16"),
                                        (4, 4, 16, 12, 2, b"multiple of 8"), (4, 4, 16, 8, 3, b"version"), (4000, 100, 16, 8, 2, b"exceeds")):
        assert lib.e4t_freeu_stats(p, Ch, p, Ck, p, 1, H, W, Ch, Ck, version, None) == -22
        assert word in lib.e4t_last_error(), (word, lib.e4t_last_error())
        assert lib.e4t_freeu_apply(p, Ch, p, Ck, p, p + 16, Ch, p + 32, Ck, 1, H, W, Ch, Ck, 1.3, 0.9, version, None) == -22
        assert word in lib.e4t_last_error(), (word, lib.e4t_last_error())
    assert lib.e4t_freeu_stats(None, 16, p, 8, p, 1, 4, 4, 16, 8, 2, None) == -22
    assert lib.e4t_freeu_apply(p, 16, p, 8, p, p, 16, p + 32, 8, 1, 4, 4, 16, 8, 1.3, 0.9, 2, None) == -22 and b"new buffers" in lib.e4t_last_error()
