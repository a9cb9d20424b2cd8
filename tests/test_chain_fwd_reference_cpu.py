"""The float64 model behind tests/test_chain_fwd_steps_gpu.py (gnnqc/ops/lstm_chain_ref.py): without
rounding it is torch's float64 LSTM and max-pool; with rounding it stays within bf16 reach of it; and
every scheduling defect the GPU test is there to catch (a wrong x buffer, a late or missing store, a
pool reading the other h buffer) lies at least five times the GPU test's bound away from it, on the
GPU test's own cases."""
import importlib.util
import os

import pytest
import torch

from gnnqc.ops.lstm_chain_ref import MUTANTS, chain_fwd_ref

_spec = importlib.util.spec_from_file_location(
    "chain_fwd_steps_gpu", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_chain_fwd_steps_gpu.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

TWO = ([16, 16], [0, 0])
CML = ([16, 16, 32, 32, 64, 64], [0, 3, 0, 3, 0, 3])
CASES = [(TWO, T, M, 18) for T in (1, 2, 3, 4, 5, 9) for M in (16, 40)] + \
        [(CML, T, M, 18) for T in (27, 28, 29, 36) for M in (16, 40)] + [(CML, 28, 16, 40)]


def _case(stack, T, M, din):
    units, pools = stack
    cpu = torch.device("cpu")
    Ws, Us, bs = G._weights(units, din, 0, cpu)
    x = G._input(T, M, din, 1000 * T + M, cpu).transpose(0, 1).double()
    return x, [w.double() for w in Ws], [u.double() for u in Us], [b.double() for b in bs], pools


def _rel(a, b):
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@pytest.mark.parametrize("stack,T,M,din", CASES)
def test_model_without_rounding_is_torch_float64(stack, T, M, din):
    x, Ws, Us, bs, pools = _case(stack, T, M, din)
    ref = chain_fwd_ref(x, Ws, Us, bs, pools, rounding=False)
    rounded = chain_fwd_ref(x, Ws, Us, bs, pools)
    cur = x
    for s, (W, U, b, P) in enumerate(zip(Ws, Us, bs, pools)):
        H = U.shape[0]
        lstm = torch.nn.LSTM(W.shape[0], H, batch_first=True).double()
        with torch.no_grad():
            lstm.weight_ih_l0.copy_(W.t())
            lstm.weight_hh_l0.copy_(U.t())
            lstm.bias_ih_l0.copy_(b)
            lstm.bias_hh_l0.zero_()
            h, _ = lstm(cur[..., :W.shape[0]])
        assert _rel(ref[s]["h"], h) < 1e-12, s
        cur = h
        if P:
            cur = torch.nn.functional.max_pool1d(h.transpose(1, 2), 3).transpose(1, 2)
            own = torch.nn.functional.max_pool1d(ref[s]["h"].transpose(1, 2), 3).transpose(1, 2)
            assert torch.equal(ref[s]["pooled"], own), s
            hr = ref[s]["h"]
            pick = torch.gather(hr[:, :hr.shape[1] // 3 * 3].reshape(hr.shape[0], -1, 3, H), 2,
                                ref[s]["idx"].long().unsqueeze(2)).squeeze(2)
            assert torch.equal(pick, own), s
        # the rounding moves the model by bf16's reach (2^-9 per rounded operand), not more
        assert _rel(rounded[s]["h"], h) < 2e-2, s


MUTANT_CASES = [(TWO, 5, 16), (TWO, 9, 40), (CML, 27, 16), (CML, 28, 16), (CML, 29, 40), (CML, 36, 16)]


MUTANT_PARAMS = [(stack, T, M, mutant, stage) for stack, T, M in MUTANT_CASES for mutant in MUTANTS for stage in (0, 1)
                 if mutant != "pool_wrong_buf" or stack[1][stage]]      # (a pool behind the stage)


@pytest.mark.parametrize("stack,T,M,mutant,stage", MUTANT_PARAMS)
def test_scheduling_mutants_lie_outside_the_bounds(stack, T, M, mutant, stage):
    x, Ws, Us, bs, pools = _case(stack, T, M, 18)
    ref = chain_fwd_ref(x, Ws, Us, bs, pools)[stage]
    mut = chain_fwd_ref(x, Ws, Us, bs, pools, mutant=mutant, mutant_stage=stage)[stage]
    keys = {"x_next": ["h"], "xbuf_mod2": ["h"], "publish_late": ["h", "g", "c"], "drop_last_two": ["h", "g", "c"],
            "pool_wrong_buf": ["pooled"]}[mutant]
    for k in keys:
        d = _rel(mut[k], ref[k])
        assert d >= 5 * G.BOUND[k], (mutant, stage, k, d)
