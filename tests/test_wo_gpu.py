"""-m gpu: the Python paths onto the weight-offset kernels (e4t/weightoffsets.py) on the device with the HIP backend, against the fp64 definition
(kernel_checks.wo_ref64: the oracle's two-Linear WeightOffsets with autograd) at the tolerances of kernel_checks.WO_TOL, along the kernels' own
blocks (wo_value_rows).  tests/test_wo_slices_cpu.py holds the CPU model of the kernels to half of those tolerances on these very inputs."""
import pytest
import torch

import kernel_checks as kc

pytestmark = pytest.mark.gpu
f32, f64 = torch.float32, torch.float64


def _assert_rows(rows):
    bad = [(n, e, t) for n, e, t in rows if not (e <= t)]
    assert not bad, "against the fp64 definition:\n" + "\n".join(f"  {n}: {e:.3e} > tol={t:.1e}" for n, e, t in bad)


@pytest.mark.parametrize("row,col", kc.WO_MODULE_DIMS)
def test_standalone_weightoffsets_module(hip_env, row, col):
    """WeightOffsets.forward() (OFFSETS_ONLY | STORE_F32, W = ones, weffT NULL through _OffsetsFn) and its backward: the GPU twin of
    test_unet_host_logic.py::test_standalone_weightoffsets_module"""
    hip, _, dev, ops = hip_env
    from e4t.weightoffsets import WeightOffsets, _wo_params
    sd, v = kc.wo_module_values(row, col)
    nat = WeightOffsets(row, col)
    nat.load_state_dict(sd)
    nat.to(dev)
    old = ops.set_backend(hip)
    try:
        o = nat()
        o.backward(v.dweff.to(dev))
        torch.cuda.synchronize()
    finally:
        ops.set_backend(old)
    assert o.dtype == f32 and o.shape == (col, row)
    got = {"weff": o.detach(), **{"g_" + k: p.grad for k, p in _wo_params(nat).items()}}
    assert all(g is not None for g in got.values())
    _assert_rows(kc.wo_value_rows(f"WeightOffsets({row}, {col})", got, kc.wo_ref64(v.to(dev)), v.mode))


def test_wobank_forward_and_two_accumulating_backward_passes(hip_env):
    """WOBank over a fused q|k|v group and a fused k|v group (WO_BANK_GROUPS): forward, then two backward passes with a dW_eff of their own each.
    On the first pass .grad is None and the bank hands out zeroed buffers; on the second it adopts the .grad that is there and the kernels
    accumulate into it (accumulate = 1 is the only mode the trainer uses).  W_eff and W_eff^T against the fp64 oracle, every .grad — the nine
    parameters of every head and the projection weights — against the fp64 oracle of the two steps' sum."""
    hip, _, dev, ops = hip_env
    from e4t.weightoffsets import WeightOffsets, WOBank, _wo_params
    vals = kc.wo_bank_values()
    bank, mods, i = WOBank("t"), [], 0
    for row, cols in kc.WO_BANK_GROUPS:
        linears, wos = [], []
        for col in cols:
            sd, (v1, _) = vals[i]
            lin, wo = torch.nn.Linear(row, col, bias=False), WeightOffsets(row, col)
            wo.load_state_dict(sd)
            with torch.no_grad():
                lin.weight.copy_(v1.W)
            linears.append(lin.to(dev))
            wos.append(wo.to(dev))
            i += 1
        bank.add(linears, wos)
        mods += list(zip(linears, wos))
    old = ops.set_backend(hip)
    try:
        for step in range(2):
            token = bank.begin(dev)
            i = 0
            for slot, (row, cols) in zip(bank.slots, kc.WO_BANK_GROUPS):      # what the consumers' backward leaves: dW_eff of the whole group, valid
                slot.dweff.copy_(torch.cat([vals[i + j][1][step].dweff for j in range(len(cols))]).to(dev))
                slot.dweff_valid = True
                i += len(cols)
            token.sum().backward()
        torch.cuda.synchronize()
    finally:
        ops.set_backend(old)
    rows, i = [], 0
    for slot, (row, cols) in zip(bank.slots, kc.WO_BANK_GROUPS):
        assert slot.weff.shape == (sum(cols), row) and slot.weffT.shape == (row, sum(cols))
        off = 0
        for col in cols:
            v1, v2 = vals[i][1]
            lin, wo = mods[i]
            both = kc.WoValues(row, col, v1.W, v1.params, v1.dweff.to(f64) + v2.dweff.to(f64), 0)
            got = {"weff": slot.weff[off:off + col], "weffT": slot.weffT[:, off:off + col], "g_W": lin.weight.grad, **{"g_" + k: p.grad for k, p in _wo_params(wo).items()}}
            assert all(g is not None for g in got.values()), [k for k, g in got.items() if g is None]
            rows += kc.wo_value_rows(f"WOBank [{i}] {row}->{col}, two steps", got, kc.wo_ref64(both.to(dev)), 0)
            rows += kc.wo_transpose_row(f"WOBank [{i}] {row}->{col}", got["weff"], got["weffT"])
            off += col
            i += 1
    _assert_rows(rows)
