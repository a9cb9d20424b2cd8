"""The kernel-rounding LSTM reference (gnnqc/ops/lstm_ref.py): without rounding its hand-written
backward is the exact float64 gradient (== autograd through the eager recurrence); with rounding
it differs from float64 by bf16-sized amounts only."""
import pytest
import torch


@pytest.mark.parametrize("H,ret", [(16, True), (64, True), (128, False)])
def test_kernel_lstm_backward_is_exact_without_rounding(H, ret):
    from gnnqc.ops.lstm import lstm_eager
    from gnnqc.ops.lstm_ref import KernelLSTM
    g = torch.Generator().manual_seed(H)
    M, T, D = 5, 9, 7
    x = torch.randn(M, T, D, generator=g, dtype=torch.float64, requires_grad=True)
    W = (torch.randn(D, 4 * H, generator=g, dtype=torch.float64) * 0.3).requires_grad_()
    U = (torch.randn(H, 4 * H, generator=g, dtype=torch.float64) * 0.3).requires_grad_()
    b = (torch.randn(4 * H, generator=g, dtype=torch.float64) * 0.1).requires_grad_()
    gout = torch.randn((M, T, H) if ret else (M, H), generator=g, dtype=torch.float64)
    ref = torch.autograd.grad((lstm_eager(x, W, U, b, ret) * gout).sum(), (x, W, U, b))
    out = KernelLSTM.apply(x, W, U, b, ret, False)
    torch.testing.assert_close(out, lstm_eager(x, W, U, b, ret), rtol=1e-12, atol=1e-12)
    got = torch.autograd.grad((out * gout).sum(), (x, W, U, b))
    for a, r in zip(got, ref):
        torch.testing.assert_close(a, r, rtol=1e-10, atol=1e-10)


def test_kernel_rounding_context_switches_the_eager_lstm():
    from gnnqc.ops.lstm import lstm_eager
    from gnnqc.ops.lstm_ref import kernel_rounding
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 6, 4, generator=g, dtype=torch.float64)
    W = torch.randn(4, 64, generator=g, dtype=torch.float64) * 0.3
    U = torch.randn(16, 64, generator=g, dtype=torch.float64) * 0.3
    b = torch.zeros(64, dtype=torch.float64)
    full = lstm_eager(x, W, U, b)
    with kernel_rounding():
        rounded = lstm_eager(x, W, U, b)
    assert not torch.equal(full, rounded)
    assert (full - rounded).abs().max().item() < 3e-2       # bf16-sized differences only


def _rg_inputs(H, seed=0):
    g = torch.Generator().manual_seed(seed)
    M, T, D = 5, 9, 7
    x = torch.randn(M, T, D, generator=g, dtype=torch.float64, requires_grad=True)
    W = (torch.randn(D, 4 * H, generator=g, dtype=torch.float64) * 0.3).requires_grad_()
    U = (torch.randn(H, 4 * H, generator=g, dtype=torch.float64) * 0.3).requires_grad_()
    b = (torch.randn(4 * H, generator=g, dtype=torch.float64) * 0.1).requires_grad_()
    return x, W, U, b, torch.randn(M, T, H, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("H,ret", [(16, True), (32, False)])
def test_kernel_lstm_rg_mode_is_exact_without_rounding(H, ret):
    """saved="rg" with rounding=False is the exact float64 gradient (== autograd), like the default."""
    from gnnqc.ops.lstm import lstm_eager
    from gnnqc.ops.lstm_ref import KernelLSTM
    x, W, U, b, gout = _rg_inputs(H)
    gout = gout if ret else gout[:, -1]
    ref = torch.autograd.grad((lstm_eager(x, W, U, b, ret) * gout).sum(), (x, W, U, b))
    out = KernelLSTM.apply(x, W, U, b, ret, False, "rg")
    torch.testing.assert_close(out, lstm_eager(x, W, U, b, ret), rtol=1e-12, atol=1e-12)
    for a, r in zip(torch.autograd.grad((out * gout).sum(), (x, W, U, b)), ref):
        torch.testing.assert_close(a, r, rtol=1e-10, atol=1e-10)
    with pytest.raises(ValueError):
        KernelLSTM.apply(x, W, U, b, ret, True, "gates")


def test_kernel_lstm_modes_differ_only_in_the_saved_state_rounding(monkeypatch):
    """The two saved-state modes run the same forward (bitwise) and round the same tensors except one:
    the default rounds the saved gates [M, T, 4H], "rg" rounds the saved c [M, T, H] (read back as
    tanh(c_t) and c_{t-1}) and leaves the gates alone. Their gradients differ by bf16-sized amounts."""
    from gnnqc.ops import lstm_ref
    H = 16
    x, W, U, b, gout = _rg_inputs(H, seed=1)
    M, T, _ = x.shape
    real_bf = lstm_ref._bf
    runs = {}
    for mode in ("gates_bf16", "rg"):
        seen = []
        monkeypatch.setattr(lstm_ref, "_bf", lambda t, seen=seen: (seen.append(tuple(t.shape)), real_bf(t))[1])
        out = lstm_ref.KernelLSTM.apply(x, W, U, b, True, True, mode)
        grads = torch.autograd.grad((out * gout).sum(), (x, W, U, b))
        runs[mode] = (out.detach(), grads, sorted(seen))
    monkeypatch.setattr(lstm_ref, "_bf", real_bf)
    assert torch.equal(runs["rg"][0], runs["gates_bf16"][0])
    a, r = list(runs["gates_bf16"][2]), list(runs["rg"][2])
    a.remove((M, T, 4 * H))
    r.remove((M, T, H))
    assert a == r and (M, T, 4 * H) not in r
    for u, v in zip(runs["rg"][1], runs["gates_bf16"][1]):
        rel = (u - v).norm().item() / v.norm().item()
        assert 0 < rel < 2e-2, rel
    # the default argument is the saved-gates mode, bit for bit
    out = lstm_ref.KernelLSTM.apply(x, W, U, b, True, True)
    for u, v in zip(torch.autograd.grad((out * gout).sum(), (x, W, U, b)), runs["gates_bf16"][1]):
        assert torch.equal(u, v)
