"""CPU: the host side of token merging (e4t/tome.py, the ToMe'd BasicTransformerBlock, trainer / sampler / CLI plumbing) through the fp32
op emulation: the native UNet with ToMe against the oracle's UNet whose attn1 calls are wrapped with the torch restatement, the random
streams, the apply / remove round trip, the command-line flags and the C ABI's argument checks."""
import importlib
import json
import os
import sys

import pytest
import torch

import e4t_oracle as orc
import tome_reference as ref
from test_unet_host_logic import build_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def emu_fp32():
    from e4t import ops
    old_b, old_act = ops.set_backend(ref.TomeEmuBackend(round_bf16=False)), ops.ACT
    ops.ACT = torch.float32
    yield ops
    ops.set_backend(old_b)
    ops.ACT = old_act


def _dense(plan):
    """the plan as matrices: M [B, T', T] (group means) and U [B, T, T'] (copy back)"""
    mp = plan.map.to(torch.int64)
    U = torch.nn.functional.one_hot(mp, plan.Tm).float()
    M = U.transpose(1, 2) / ref.counts(plan)[..., None].float()
    return M, U


def _wrap_oracle_attn1(unet, state, latent_hw):
    """run time only: every oracle block at the merged level matches on its input, merges LN(x), runs attn1 on T' rows, unmerges"""
    h, w = latent_hw
    seen = []
    for blk in [m for m in unet.modules() if isinstance(m, orc.BasicTransformerBlock)]:
        stash = {}
        blk.register_forward_pre_hook(lambda mod, args, stash=stash: stash.__setitem__("x", args[0]))
        orig = blk.attn1.forward

        def wrapped(n, *a, _orig=orig, _stash=stash, **k):
            x = _stash["x"]
            B, T, d = x.shape
            if T != h * w:
                return _orig(n, *a, **k)
            from e4t.ops import TomePlan
            plan = TomePlan.from_fields(**ref.match_plan(x.detach(), h, w, state.r_for(T), state.choice(h, w, "cpu")))
            seen.append(plan)
            M, U = _dense(plan)
            return U @ _orig(M @ n, *a, **k)
        blk.attn1.forward = wrapped
    return seen


def test_unet_with_tome_matches_wrapped_oracle(emu_fp32):
    from e4t import tome
    cfg = orc.tiny_unet_config(ctx_dim=64)
    r_unet, n_unet = build_pair(cfg)
    for m in (r_unet, n_unet):
        for n, p in m.named_parameters():
            p.requires_grad_("wo" in n)
    st = tome.apply_tome(n_unet, 0.5, use_rand=True, generator=torch.Generator().manual_seed(4), record=True)
    g = torch.Generator().manual_seed(1)
    B = 2
    x = torch.randn(B, 4, 16, 16, generator=g)
    t = torch.tensor([3, 977])
    ctx = torch.randn(B, 7, 64, generator=g)
    w = torch.randn(B, 4, 16, 16, generator=g)
    enc_n = n_unet(x, t, ctx, return_encoder_outputs=True)["down_block_samples"]
    n_enc_plans = len(st.recorded)
    out_n = n_unet(x, t, ctx).sample
    assert n_enc_plans == 2 and len(st.recorded) == 2 + 5        # the 16x16 level only: 2 down blocks, + 3 up blocks in the full pass
    assert all(p.T == 256 and p.Tm == 128 for p in st.recorded)
    seen = _wrap_oracle_attn1(r_unet, st, (16, 16))
    enc_r = r_unet(x, t, ctx, return_encoder_outputs=True)["down_block_samples"]
    out_r = r_unet(x, t, ctx)
    assert len(seen) == len(st.recorded)
    for a, b in zip(st.recorded, seen):                          # the emulation's match is the restatement's: the same plans
        assert torch.equal(a.buf, b.buf)
    assert len(enc_n) == 13
    for a, b in zip(enc_n, enc_r):
        torch.testing.assert_close(a, b, rtol=2e-4, atol=2e-4)
    torch.testing.assert_close(out_n, out_r, rtol=2e-4, atol=2e-4)
    (out_n * w).sum().backward()
    (out_r * w).sum().backward()
    gr = dict(r_unet.named_parameters())
    checked = 0
    for n, p in n_unet.named_parameters():
        if "wo" in n:
            assert p.grad is not None, n
            torch.testing.assert_close(p.grad, gr[n].grad, rtol=5e-3, atol=2e-4, msg=lambda m, n=n: f"{n}: {m}")
            checked += 1
    assert checked == 16 * 2 * 3 * 9
    # and merging does change the result: the unmerged oracle is NOT matched
    r2, _ = build_pair(cfg)
    assert float((r2(x, t, ctx) - out_r).detach().abs().max()) > 1e-3


def test_remove_tome_restores_the_model_bitwise(emu_fp32):
    from e4t import tome
    _, nat = build_pair(orc.tiny_unet_config(ctx_dim=64), seed=2)
    g = torch.Generator().manual_seed(3)
    x, t, ctx = torch.randn(1, 4, 16, 16, generator=g), torch.tensor([40]), torch.randn(1, 5, 64, generator=g)
    with torch.no_grad():
        y0 = nat(x, t, ctx).sample.clone()
        st = tome.apply_tome(nat, 0.5)
        assert tome.get_state(nat) is st
        y1 = nat(x, t, ctx).sample.clone()
        tome.remove_tome(nat)
        y2 = nat(x, t, ctx).sample.clone()
    assert tome.get_state(nat) is None and not any("_tome" in m.__dict__ for m in nat.modules())
    assert float((y1 - y0).abs().max()) > 1e-4
    assert torch.equal(y2, y0)


def test_choice_is_one_draw_per_step_from_tomes_own_generator(emu_fp32):
    """the trainer's noise / timestep draws are those of a run without ToMe; all blocks and both UNet passes of a step share one draw,
    the next step gets a new one, in the same buffer"""
    from e4t import tome
    from e4t.trainer import E4TTrainer
    from test_train_step_host_logic import build
    g = torch.Generator().manual_seed(7)
    B = 2
    pixels = torch.rand(B, 3, 64, 64, generator=g) * 2 - 1
    latents = torch.randn(B, 4, 16, 16, generator=g) * 0.18215
    ids = torch.randint(1, 99, (B, 9), generator=g)
    pidx = torch.tensor([2, 4])
    states = []
    for ratio in (0.0, 0.5):
        _, _, n_unet, n_enc, text = build()
        tr = E4TTrainer(n_unet, n_enc, text, vae=None, lr=1e-3, class_token_id=11, empty_prompt_ids=torch.zeros(1, 9, dtype=torch.long),
                        device=torch.device("cpu"))
        st = tome.apply_tome(n_unet, ratio, record=True) if ratio else None
        torch.manual_seed(123)
        draws = []
        real = tr.add_noise
        tr.add_noise = lambda x0, noise, t, _r=real: (draws.append((noise.clone(), t.clone())), _r(x0, noise, t))[1]
        loss = tr.train_step(pixels, ids, pidx, latents=latents)[0]
        assert torch.isfinite(loss)
        if st is not None:
            buf = st.choice(16, 16, torch.device("cpu"))
            first = buf.clone()
            assert len(st.recorded) == 6 and len(st._choice) == 1          # 2 + 2 + 3 block calls at the 16x16 level, the very first shared by the two passes
            tr.train_step(pixels, ids, pidx, latents=latents)
            assert st.choice(16, 16, torch.device("cpu")) is buf and not torch.equal(buf, first)
        else:
            tr.train_step(pixels, ids, pidx, latents=latents)
        states.append((draws, torch.get_rng_state()))
    (d0, s0), (d1, s1) = states
    assert len(d0) == len(d1) == 2
    for (n0, t0), (n1, t1) in zip(d0, d1):
        assert torch.equal(n0, n1) and torch.equal(t0, t1)
    assert torch.equal(s0, s1)


def test_injected_plans_are_used_in_call_order(emu_fp32):
    from e4t import tome
    _, nat = build_pair(orc.tiny_unet_config(ctx_dim=64), seed=5)
    g = torch.Generator().manual_seed(6)
    x, t, ctx = torch.randn(2, 4, 16, 16, generator=g), torch.tensor([40, 7]), torch.randn(2, 5, 64, generator=g)
    with torch.no_grad():
        st = tome.apply_tome(nat, 0.25, record=True)
        y0 = nat(x, t, ctx).sample.clone()
        plans = list(st.recorded)
        st2 = tome.apply_tome(nat, 0.25, plans=plans)
        calls = []
        from e4t import ops
        real = ops.backend().tome_match
        ops.backend().tome_match = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
        try:
            y1 = nat(x, t, ctx).sample.clone()
        finally:
            del ops.backend().tome_match
        assert not calls and st2._cursor == len(plans) == 5 and torch.equal(y0, y1)
        with pytest.raises(RuntimeError, match="plans were injected"):
            nat(x, t, ctx)                                  # no new_step(): the list is exhausted
        tome.new_step(nat)
        assert torch.equal(nat(x, t, ctx).sample, y0)


def test_level_selection_follows_max_downsample():
    from e4t.tome import TomeState
    st = TomeState(0.5)
    assert not st.applies(4096, 64, 64)                     # latent size unknown yet
    st.latent_tokens = 4096
    assert st.applies(4096, 64, 64) and not st.applies(1024, 32, 32)
    assert st.r_for(4096) == 2048 and TomeState(0.75).r_for(4096) == 3072 and TomeState(0.7).r_for(64) == 44
    st2 = TomeState(0.5, max_downsample=2)
    st2.latent_tokens = 4096
    assert st2.applies(1024, 32, 32) and not st2.applies(256, 16, 16)
    st.latent_tokens = 15 * 16
    assert not st.applies(240, 15, 16)                      # odd side: the 2x2 cells do not tile it
    for bad in (0.0, 0.8, -1.0):
        with pytest.raises(ValueError):
            TomeState(bad)


def _parse(module, argv, monkeypatch):
    monkeypatch.setattr(sys, "argv", [f"{module}.py"] + argv)
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module(module).parse_args()


@pytest.mark.parametrize("module,extra", [("pretrain_e4t", ["--synthetic_data"]), ("tuning_e4t", []), ("inference", [])])
def test_cli_flags(monkeypatch, module, extra):
    a = _parse(module, extra, monkeypatch)
    assert a.tome_ratio == 0.0 and a.tome_no_rand is False           # off by default
    a = _parse(module, extra + ["--tome_ratio", "0.5", "--tome_no_rand"], monkeypatch)
    assert a.tome_ratio == 0.5 and a.tome_no_rand is True
    assert _parse(module, extra + ["--tome_ratio", "0.75"], monkeypatch).tome_ratio == 0.75
    for bad in ("0.76", "-0.1"):
        with pytest.raises(SystemExit):
            _parse(module, extra + ["--tome_ratio", bad], monkeypatch)


def test_cli_applies_tome_and_config_json_does_not_record_it(tmp_path, monkeypatch):
    from e4t import cli_common as cc, tome
    from e4t.utils import save_config
    a = _parse("pretrain_e4t", ["--synthetic_data", "--tome_ratio", "0.5", "--seed", "3"], monkeypatch)
    save_config(vars(a), str(tmp_path))
    saved = json.load(open(tmp_path / "config.json"))
    assert "tome_ratio" not in saved and "tome_no_rand" not in saved and saved["seed"] == 3
    _, nat = build_pair(orc.tiny_unet_config(ctx_dim=64))
    st = cc.apply_tome_args(nat, a)
    assert st is tome.get_state(nat) and st.ratio == 0.5 and st.use_rand
    _, nat2 = build_pair(orc.tiny_unet_config(ctx_dim=64))
    assert cc.apply_tome_args(nat2, _parse("pretrain_e4t", ["--synthetic_data"], monkeypatch)) is None and tome.get_state(nat2) is None


def test_abi_rejects_bad_arguments_without_a_launch():
    """e4t_tome_*: -22 and a message before anything is launched (safe without a GPU)"""
    from e4t import _C
    lib = _C.load()
    assert lib.e4t_tome_plan_ints(4096, 2048) == (2 * 4096 + 1024 + 1) + 2 * 4096 + 2 * 3072
    assert lib.e4t_tome_plan_ints(4096, 0) == 0 and lib.e4t_tome_plan_ints(4096, 3073) == 0 and lib.e4t_tome_plan_ints(16388, 4) == 0
    x = (_C.C.c_char * 64)()
    p = _C.C.addressof(x)
    for ld, h, w, d, r, word in ((64, 8, 8, 24, 16, b"multiple of 16"), (64, 7, 8, 64, 16, b"even"), (64, 8, 9, 64, 16, b"even"),
                                 (64, 8, 8, 64, 0, b"r=0"), (64, 8, 8, 64, 49, b"r=49"), (64, 130, 128, 64, 16, b"exceeds 16384"),
                                 (60, 8, 8, 64, 16, b"aligned")):
        assert lib.e4t_tome_match(p, ld, 1, h, w, d, r, None, p, None) == -22
        assert word in lib.e4t_last_error(), (word, lib.e4t_last_error())
    assert lib.e4t_tome_merge(p, 64, p, p, 64, 1, 64, 49, 64, 1, None) == -22
    assert lib.e4t_tome_merge(p, 64, p, p, 64, 1, 64, 16, 60, 1, None) == -22
    assert lib.e4t_tome_unmerge(p, 64, p, None, p, 64, 1, 62, 16, 64, 0, None) == -22
    assert lib.e4t_tome_unmerge(None, 64, p, None, p, 64, 1, 64, 16, 64, 0, None) == -22
