"""CPU: block-wise 8-bit AdamW moments (E4TTrainer(optimizer_state_bits=8)).  The definition in e4t/optimization.py (codebooks,
quantize_blockwise / dequantize_blockwise) on constructed cases, and the trainer's host logic on the op emulation of tests/adam8_reference.py:
the first step from a fresh state, the block-rounded split around a deferred region, the head factors, the state dict and its two conversions,
the command lines' flag, and a two-rank (gloo) run under the replica check."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from adam8_reference import Adam8EmuBackend
from test_train_step_host_logic import _data, _step, build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
CPU = torch.device("cpu")
f32 = torch.float32


@pytest.fixture()
def adam8_emu():
    from e4t import ops
    old_b, old_act = ops.set_backend(Adam8EmuBackend(round_bf16=False)), ops.ACT
    ops.ACT = torch.float32
    yield ops
    ops.set_backend(old_b)
    ops.ACT = old_act


def _trainer(bits=8, lr=1e-3, seed=0, **kw):
    from e4t.trainer import E4TTrainer
    _, _, n_unet, n_enc, text = build(seed)
    return E4TTrainer(n_unet, n_enc, text, vae=None, lr=lr, class_token_id=11, empty_prompt_ids=torch.zeros(1, 9, dtype=torch.long), device=CPU,
                      optimizer_state_bits=bits, **kw)


# ---- the codebooks ------------------------------------------------------------------------------------------------------------------------
def test_codebooks():
    from e4t.optimization import ADAM8_BLOCK, dynamic_codebook
    assert ADAM8_BLOCK == 256
    for signed in (True, False):
        c = dynamic_codebook(signed)
        assert c.dtype == f32 and c.shape == (256,)
        assert bool((c[1:] > c[:-1]).all())                                  # sorted, 256 distinct values
        assert int((c == 0).sum()) == 1 and int((c == 1).sum()) == 1 and float(c[-1]) == 1.0
        assert torch.equal(c, dynamic_codebook(signed))                      # a second construction gives the same bits
    s, u = dynamic_codebook(True), dynamic_codebook(False)
    assert float(s[0]) == float(np.float32(-0.99296875)) and float(s[0]) > -1.0          # the signed map has no -1
    assert float(u[0]) == 0.0 and bool((u >= 0).all())
    assert int((s == 0).nonzero()[0]) != 0                                   # byte 0 of the signed map is not zero
    assert int((s < 0).sum()) == 127 and int((s > 0).sum()) == 128


# ---- quantize / dequantize ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signed", [True, False])
def test_every_code_value_round_trips(signed):
    from e4t.optimization import dequantize_blockwise, dynamic_codebook, quantize_blockwise
    c = dynamic_codebook(signed)
    for scale in (1.0, 0.37, 3e-7, 1e5):            # (1.0 is in the block, so the block's scale is `scale` itself)
        x = c * np.float32(scale)
        q, a = quantize_blockwise(x, c)
        assert a.tolist() == [float(np.float32(scale))]
        assert torch.equal(q.long(), torch.arange(256)), scale
        assert torch.equal(dequantize_blockwise(q, a, c), x)


def test_an_exact_midpoint_takes_the_lower_index():
    from e4t.optimization import dynamic_codebook, quantize_blockwise
    for signed in (True, False):
        c = dynamic_codebook(signed)
        # pairs of neighbours whose midpoint is an fp32 number at equal fp32 distances from both
        mid = ((c[:-1].double() + c[1:].double()) / 2).to(f32)
        exact = (mid - c[:-1] == c[1:] - mid) & (mid.double() == (c[:-1].double() + c[1:].double()) / 2)
        js = exact.nonzero().flatten().tolist()
        assert len(js) >= 8, len(js)
        for j in js[:: max(1, len(js) // 16)]:
            x = torch.zeros(256)
            x[0] = 1.0                      # the block's scale is 1: y = x
            x[1] = mid[j]
            x[2] = torch.nextafter(mid[j], torch.tensor(2.0))
            x[3] = torch.nextafter(mid[j], torch.tensor(-2.0))
            q, _ = quantize_blockwise(x, c)
            assert q[1] == j and q[2] == j + 1 and q[3] == j, (signed, j, q[:4].tolist())


def test_special_blocks():
    from e4t.optimization import dequantize_blockwise, dynamic_codebook, quantize_blockwise
    s, u = dynamic_codebook(True), dynamic_codebook(False)
    zs, zu = int((s == 0).nonzero()[0]), int((u == 0).nonzero()[0])
    # all zero: scale 0, the zero index, no NaN on the way back
    for c, z in ((s, zs), (u, zu)):
        q, a = quantize_blockwise(torch.zeros(300), c)
        assert a.tolist() == [0.0, 0.0] and bool((q == z).all())
        back = dequantize_blockwise(q, a, c)
        assert torch.isfinite(back).all() and not back.any()
    # one element 1e8 times the others: it maps to 1.0 exactly, the others to zero or the smallest code values (finite, no NaN)
    x = torch.full((256,), 1e-3)
    x[17] = 1e5
    q, a = quantize_blockwise(x, s)
    assert a.tolist() == [1e5] and q[17] == 255
    rest = torch.cat([q[:17], q[18:]]).long()
    assert bool(((rest == zs) | (rest == zs + 1)).all())
    back = dequantize_blockwise(q, a, s)
    assert torch.isfinite(back).all() and back[17] == 1e5
    # -absmax: index 0 of the signed map (-0.993: the map has no -1)
    x = torch.linspace(-1, 0.5, 256) * 0.25
    q, a = quantize_blockwise(x, s)
    assert a.tolist() == [0.25] and q[0] == 0
    assert float(dequantize_blockwise(q, a, s)[0]) == float(s[0] * np.float32(0.25))


@pytest.mark.parametrize("n", [257, 511])
def test_a_short_last_block(n):
    from e4t.optimization import dequantize_blockwise, dynamic_codebook, quantize_blockwise
    c = dynamic_codebook(True)
    x = torch.randn(n, generator=torch.Generator().manual_seed(n))
    x[256:] *= 1e-3                         # the last block has its own, much smaller scale
    q, a = quantize_blockwise(x, c)
    assert q.shape == (n,) and q.dtype == torch.uint8 and a.shape == (2,)
    assert float(a[0]) == float(x[:256].abs().max()) and float(a[1]) == float(x[256:].abs().max())
    # each block alone gives the same codes
    q0, _ = quantize_blockwise(x[:256], c)
    q1, a1 = quantize_blockwise(x[256:], c)
    assert torch.equal(q, torch.cat([q0, q1])) and float(a1) == float(a[1])
    back = dequantize_blockwise(q, a, c)
    assert back.shape == (n,)
    # the map's relative resolution: neighbouring values are at most ~ 9 % of the block's scale apart (the top decade has 64 steps of 0.9 / 64)
    assert float((back - x)[256:].abs().max()) <= 0.9 / 64 / 2 * float(a[1]) * 1.0001
    assert float((back - x)[:256].abs().max()) <= 0.9 / 64 / 2 * float(a[0]) * 1.0001


def test_quantize_from_in_chunks_equals_one_pass():
    from e4t.optimization import Adam8State, quantize_blockwise
    n = 256 * 5 + 77
    g = torch.Generator().manual_seed(9)
    m, v = torch.randn(n, generator=g), torch.randn(n, generator=g).abs()
    st = Adam8State(n, CPU)
    st.CHUNK = 512          # three chunks, the last one short
    st.quantize_from(m, v)
    qm, am = quantize_blockwise(m, st.code_m)
    qv, av = quantize_blockwise(v, st.code_v)
    assert torch.equal(st.qm, qm) and torch.equal(st.absmax_m, am) and torch.equal(st.qv, qv) and torch.equal(st.absmax_v, av)


# ---- the trainer ---------------------------------------------------------------------------------------------------------------------------
def test_constructor_and_fresh_state(adam8_emu):
    tr = _trainer(8)
    assert tr.exp_avg is None and tr.exp_avg_sq is None          # no fp32 moments are allocated
    st = tr.adam8
    n = tr.flat.numel
    assert st.qm.dtype == torch.uint8 and st.qm.shape == (n,) and st.qv.shape == (n,) and st.absmax_m.shape == (-(-n // 256),) == st.absmax_v.shape
    assert bool((st.qm == st.zero_m).all()) and bool((st.qv == st.zero_v).all()) and st.zero_m != 0
    assert not st.absmax_m.any() and not st.absmax_v.any()
    m, v = st.dequantize()
    assert m.shape == (n,) and not m.any() and not v.any()
    assert _trainer(32).adam8 is None and _trainer(32).exp_avg is not None
    with pytest.raises(ValueError, match="optimizer_state_bits"):
        _trainer(16)


def test_first_step_from_a_fresh_state_equals_the_32_bit_trainers(adam8_emu):
    """the moments are exactly zero and p moves by the UNQUANTISED new moments: the first step's parameters are the 32-bit trainer's, bit for
    bit (a state of zero BYTES would start exp_avg at -0.993 * 0 = -0 ... and, after any load, at wrong values)"""
    d = _data(2, 41)
    t32, t8 = _trainer(32), _trainer(8)
    assert torch.equal(t32.flat.data, t8.flat.data)
    out32, out8 = _step(t32, d), _step(t8, d)
    assert all(torch.equal(a, b) for a, b in zip(out32, out8))
    assert torch.equal(t32.flat.data, t8.flat.data)
    assert t8.step_count == 1
    # ... and the state now holds the quantised moments of that step
    from e4t.optimization import quantize_blockwise
    qm, am = quantize_blockwise(t32.exp_avg, t8.adam8.code_m)
    qv, av = quantize_blockwise(t32.exp_avg_sq, t8.adam8.code_v)
    assert torch.equal(qm, t8.adam8.qm) and torch.equal(am, t8.adam8.absmax_m) and torch.equal(qv, t8.adam8.qv) and torch.equal(av, t8.adam8.absmax_v)
    # the second step differs: it starts from rounded moments
    d2 = _data(2, 42)
    _step(t32, d2), _step(t8, d2)
    assert torch.isfinite(t8.flat.data).all() and not torch.equal(t32.flat.data, t8.flat.data)


@pytest.mark.parametrize("ema", [None, 0.999])
def test_adamw_in_three_launches_around_a_deferred_region_equals_one(adam8_emu, ema):
    class Handle:
        def wait(self):
            pass
    res, launches = [], []
    be = adam8_emu.backend()
    orig = be.adamw8
    for split in (False, True):
        tr = _trainer(8, ema_decay=ema)
        _step(tr, _data(2, 30))             # a state away from the fresh one
        loss, _, _ = tr.losses(*[_data(2, 31)[k] for k in ("px", "lat", "noise", "t", "ids", "pidx")])
        loss.backward()
        n = tr.flat.numel
        lo, hi = n // 3 + 7, 2 * n // 3 + 131
        assert lo % 256 and hi % 256 and hi // 256 > lo // 256 + 1
        calls = []
        be.adamw8 = lambda p, *a, **k: (calls.append(p.numel()), orig(p, *a, **k))[1]
        try:
            tr.optimizer_step(((lo, hi), [Handle()]) if split else None)
        finally:
            del be.adamw8
        launches.append(calls)
        res.append([tr.flat.data.clone()] + [b.clone() for b in tr.adam8.buffers()] + ([tr.ema.clone()] if ema else []))
    n = res[0][0].numel()
    lo8, hi8 = lo // 256 * 256, -(-hi // 256) * 256
    assert launches[0] == [n] and launches[1] == [lo8, n - hi8, hi8 - lo8]          # every block in exactly one launch
    assert all(torch.equal(a, b) for a, b in zip(*res))


def test_the_head_factors_are_not_taken(adam8_emu):
    taken = {}
    for bits in (32, 8):
        tr = _trainer(bits)
        orig = tr._take_head_factors
        seen = []
        tr.encoder.take_head_factors = lambda gb, Z, orig=orig, seen=seen: (seen.append(orig(gb, Z)), seen[-1])[1]
        _step(tr, _data(2, 33))
        taken[bits] = seen
    assert taken[32] == [True] and taken[8] == [False]


def test_state_dict_round_trip_and_both_conversions(adam8_emu, tmp_path):
    from e4t.optimization import quantize_blockwise
    batches = [_data(2, 31 + i) for i in range(3)]
    full = _trainer(8)
    for d in batches:
        _step(full, d)
    tr = _trainer(8)
    for d in batches[:2]:
        _step(tr, d)
    sd = tr.state_dict()
    assert set(sd) == {"params", "step_count", "lr", "state_bits", "block", "qm", "qv", "absmax_m", "absmax_v"}
    assert sd["state_bits"] == 8 and sd["block"] == 256 and sd["qm"].dtype == torch.uint8
    torch.save(sd, tmp_path / "state.pt")
    tr2 = _trainer(8)
    tr2.load_state_dict(torch.load(tmp_path / "state.pt"))
    assert all(torch.equal(a, b) for a, b in zip(tr2.adam8.buffers(), tr.adam8.buffers())) and tr2.step_count == 2
    _step(tr2, batches[2])
    assert torch.equal(tr2.flat.data, full.flat.data) and all(torch.equal(a, b) for a, b in zip(tr2.adam8.buffers(), full.adam8.buffers()))
    # 8 -> 32: the 32-bit trainer's moments are dequantize() of the state
    t32 = _trainer(32)
    t32.load_state_dict(sd)
    m, v = tr.adam8.dequantize()
    assert torch.equal(t32.exp_avg, m) and torch.equal(t32.exp_avg_sq, v) and torch.equal(t32.flat.data, sd["params"]) and t32.step_count == 2
    assert set(t32.state_dict()) == {"params", "exp_avg", "exp_avg_sq", "step_count", "lr"}          # the 32-bit format is unchanged
    # 32 -> 8: quantize_blockwise of the moments
    s32 = _trainer(32)
    for d in batches[:2]:
        _step(s32, d)
    t8 = _trainer(8)
    t8.load_state_dict(s32.state_dict())
    qm, am = quantize_blockwise(s32.exp_avg, t8.adam8.code_m)
    qv, av = quantize_blockwise(s32.exp_avg_sq, t8.adam8.code_v)
    assert torch.equal(t8.adam8.qm, qm) and torch.equal(t8.adam8.absmax_m, am) and torch.equal(t8.adam8.qv, qv) and torch.equal(t8.adam8.absmax_v, av)
    assert torch.equal(t8.flat.data, s32.flat.data) and t8.step_count == 2
    # another block size fails loudly, in either kind of trainer
    for t in (_trainer(8), _trainer(32)):
        with pytest.raises(RuntimeError, match="blocks of 128"):
            t.load_state_dict(dict(sd, block=128))


# ---- command lines ------------------------------------------------------------------------------------------------------------------------
def test_flags(adam8_emu, monkeypatch, capsys):
    import importlib
    import json
    import pretrain_e4t
    import tuning_e4t
    from test_cli_setup import pretrain_args, tuning_args

    def parse(module, argv):
        monkeypatch.setattr(sys, "argv", [f"{module}.py"] + argv)
        return importlib.import_module(module).parse_args()
    for module in ("pretrain_e4t", "tuning_e4t"):
        assert parse(module, ["--synthetic_data"] if module == "pretrain_e4t" else []).optimizer_state_bits == 32
        assert parse(module, ["--optimizer_state_bits", "8"]).optimizer_state_bits == 8
        with pytest.raises(SystemExit):
            parse(module, ["--optimizer_state_bits", "16"])
        capsys.readouterr()
        with pytest.raises(SystemExit) as ex:
            parse(module, ["--use_8bit_adam"])
        assert ex.value.code == 2 and "--optimizer_state_bits 8" in capsys.readouterr().err
    assert pretrain_e4t.setup(pretrain_args(), CPU)["trainer"].adam8 is None
    tr = pretrain_e4t.setup(pretrain_args(optimizer_state_bits=8), CPU)["trainer"]
    assert tr.adam8 is not None and tr.exp_avg is None
    assert tuning_e4t.setup(tuning_args(), CPU)["trainer"].adam8 is None
    tr = tuning_e4t.setup(tuning_args(optimizer_state_bits=8), CPU)["trainer"]
    assert tr.adam8 is not None and tr.exp_avg is None and tr.tuning
    from e4t.utils import save_config
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        save_config(vars(pretrain_args(optimizer_state_bits=8)), d)
        assert json.load(open(os.path.join(d, "config.json")))["optimizer_state_bits"] == 8


# ---- two ranks over gloo ----------------------------------------------------------------------------------------------------------------------
def _gloo_worker(rank, world, port, out_dir, mode):
    for p in (os.path.join(ROOT, "e4t-diffusion_amd"), ROOT, HERE, os.path.join(ROOT, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), E4T_REPLICA_CHECK_EVERY="1")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    from e4t import ops
    from test_ddp_gloo import _batch
    ops.set_backend(Adam8EmuBackend(round_bf16=False))
    ops.ACT = torch.float32
    tr = _trainer(8, seed=rank if mode == "seeds" else 0)
    step = lambda r: (lambda b: tr.train_step(b["pixels"], b["ids"], b["pidx"], noise=b["noise"], timesteps=b["t"], latents=b["latents"]))(_batch(r))
    msg = "no error"
    if mode == "seeds":
        for i in range(3):
            step(rank + 2 * i)              # the per-step replica check covers the four 8-bit buffers
    else:                                   # "diverge": one code byte alone differs
        step(rank)
        if rank == 1:
            tr.adam8.qv[5] += 1
        try:
            step(rank + 2)
        except RuntimeError as e:
            msg = str(e)
    torch.save(dict(params=tr.flat.data.clone(), bufs=[b.clone() for b in tr.adam8.buffers()], msg=msg), os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["seeds", "diverge"])
def test_two_ranks_keep_one_8_bit_state(tmp_path, mode):
    from test_ema_host_logic import _free_port
    world = 2
    mp.spawn(_gloo_worker, args=(world, _free_port(), str(tmp_path), mode), nprocs=world, join=True)
    r0, r1 = (torch.load(tmp_path / f"rank{r}.pt") for r in range(world))
    if mode == "diverge":
        assert all("replicas diverged" in r["msg"] for r in (r0, r1))
        return
    assert r0["msg"] == r1["msg"] == "no error"
    assert torch.equal(r0["params"], r1["params"]) and all(torch.equal(a, b) for a, b in zip(r0["bufs"], r1["bufs"]))
    assert r0["bufs"][2].any() and r0["bufs"][3].any()
