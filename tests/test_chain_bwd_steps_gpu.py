"""Chain backward (lstm_chain_bwd.hip) at the sequence lengths where the H = 16 stages' one-step-ahead
dh staging can go wrong: stages shorter than the ring, un-pooling tails, lengths that are / are not
multiples of the ring depth, one and three row tiles.

The CML stack is TimeLayer(18, 16, 2, "lstm", pool_size=3): six chain stages, T -> T/3 -> T/9 steps,
and a last pool to T/27. The whole layer needs T >= 27, so the shortest top stages that exist run
3 steps (T = 27 .. 35): still shorter than the H = 16 / H = 32 ring (4) and, at T = 27, the only
length without an un-pooling tail anywhere, i.e. with a live gradient in every stage's first reverse
step. Lengths:

    T   H=16 stages   T % 3   T % 4   note
    27  27 steps      0       3       no zero-gradient tail in any stage
    28  28            1       0       tail of 1 step below the first pool
    29  29            2       1       tail of 2 steps
    36  36            0       0       multiple of ring and pool; 36 -> 12 -> 4 (tail at the top)
"""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _layer(cuda_device, pool_size=3, seed=0, din=18):
    from gnnqc.models.timelayer import TimeLayer
    torch.manual_seed(seed)
    return TimeLayer(din, 16, 2, "lstm", pool_size=pool_size).to(cuda_device)


def _padded(x):
    """[M, T, C] -> the time-major kernel input [T, Mp, C rounded up to 4] (zero rows / channels;
    18 -> 20, 40 -> 40)."""
    M, C = x.shape[0], x.shape[2]
    Mp = (M + 15) // 16 * 16
    return F.pad(x.transpose(0, 1), (0, -C % 4, 0, Mp - M)).contiguous()


def _run(tl, h, M, monkeypatch, chain):
    monkeypatch.setenv("GNNQC_CHAIN", "1" if chain else "0")
    hi = h.clone().requires_grad_(True)
    for p in tl.parameters():
        p.grad = None
    out = tl.forward_time_major(hi, M)
    out.pow(2).sum().backward()
    return out.detach(), [hi.grad.clone()] + [p.grad.clone() for p in tl.parameters()]


def _check_chain_vs_per_layer(cuda_device, monkeypatch, tl, T, M, nstages, din=18):
    from gnnqc.utils.native import hip_ops
    monkeypatch.setenv("GNNQC_NO_PAIR", "1")
    monkeypatch.setenv("GNNQC_CHAIN_BWD", "1")
    gen = torch.Generator().manual_seed(1000 * T + M)
    x = torch.randn(M, T, din, generator=gen).to(cuda_device)
    h = _padded(x)
    plan = tl._chain_plan(tl._sequence(), h)
    assert plan is not None and len(plan[0]) == nstages, plan
    # stage 0 takes the whole padded input: more than 32 channels make it a KX = 2 stage
    assert plan[0][0].units == 16 and plan[0][0].kernel.shape[0] == din and (h.shape[2] > 32) == (din > 32)
    o0, g0 = _run(tl, h, M, monkeypatch, False)
    st0 = hip_ops().lstm_chain_status(h).cpu()
    runs = [_run(tl, h, M, monkeypatch, True) for _ in range(3)]
    torch.cuda.synchronize()
    st1 = hip_ops().lstm_chain_status(h).cpu()
    assert int(st1[2]) == 0, "a consumer spin timed out"
    # one forward and one backward launch per run, every workgroup of the last one finished
    assert int(st1[0]) - int(st0[0]) == 6 and int(st1[1]) == 0, (st0, st1)
    o1, g1 = runs[0]
    torch.testing.assert_close(o1, o0, atol=1e-5, rtol=1e-5)
    for k, (a, b_) in enumerate(zip(g1, g0)):
        err, ref = (a - b_).norm().item(), b_.norm().item()
        print(f"T={T} M={M} grad[{k}] rel err {err / (ref + 1e-6):.3e}")
        assert err <= 5e-3 * (ref + 1e-6), (k, err, ref)
    # fresh epochs over reused granule addresses: bitwise the same gradients
    for _, g in runs[1:]:
        for a, b_ in zip(g, g1):
            assert torch.equal(a, b_)
    # rows past M (the padding of the last 16-row tile) get no gradient
    if h.shape[1] > M:
        assert float(g1[0][:, M:].abs().max()) == 0.0


@pytest.mark.parametrize("M", [16, 40])
@pytest.mark.parametrize("T", [27, 28, 29, 36])
def test_chain_bwd_short_and_tailed_sequences_match_per_layer(cuda_device, monkeypatch, T, M):
    """Chain forward + backward == the per-layer kernels (output 1e-5, every gradient 5e-3 in
    relative norm), three launches bitwise equal, no spin timeout, epoch counter advanced by 6."""
    _check_chain_vs_per_layer(cuda_device, monkeypatch, _layer(cuda_device), T, M, 6)


def test_chain_bwd_identity_unpool_matches_per_layer(cuda_device, monkeypatch):
    """pool_size = 1: a two-stage chain whose un-pooling stage takes the identity (every step has a
    source step, phase 0), at a length that is no multiple of the ring depth."""
    _check_chain_vs_per_layer(cuda_device, monkeypatch, _layer(cuda_device, pool_size=1), 10, 40, 2)


def test_chain_bwd_wide_input_first_stage_matches_per_layer(cuda_device, monkeypatch):
    """A 40-channel input: stage 0 is an H = 16 stage with KX = 2 (33-64 input channels), the
    instantiations that the 18-channel CML stack never reaches (forward stage 0 streaming fp32 x,
    backward bottom stage with a two-block dx). Same bounds as the cases above."""
    _check_chain_vs_per_layer(cuda_device, monkeypatch, _layer(cuda_device, din=40), 28, 16, 6, din=40)


def test_chain_bwd_matches_fp64_oracle(cuda_device, monkeypatch):
    """T = 28, M = 16, three seeds: the chain's gradients against the float64 model that rounds to
    bf16 where the kernels do (gnnqc/ops/lstm_ref.py). Bounds as for the other whole-model
    comparisons with that oracle (test_kernels_gpu.py): output 3e-3, every gradient 8e-3 in
    relative norm. Prints the largest relative gradient error of each seed (measured: 1.93e-3,
    1.61e-3, 1.47e-3; before the first reverse step kept its own saved state: 4.39e-3, 4.37e-3,
    4.81e-3)."""
    from gnnqc.ops.lstm_ref import kernel_rounding
    monkeypatch.setenv("GNNQC_NO_PAIR", "1")
    monkeypatch.setenv("GNNQC_CHAIN_BWD", "1")
    T, M = 28, 16
    worst = []
    for seed in (0, 1, 2):
        tl = _layer(cuda_device, seed=seed)
        gen = torch.Generator().manual_seed(77 + seed)
        x = torch.randn(M, T, 18, generator=gen)
        h = _padded(x.to(cuda_device))
        assert tl._chain_plan(tl._sequence(), h) is not None
        o1, g1 = _run(tl, h, M, monkeypatch, True)
        ref = copy.deepcopy(tl).cpu().double()
        xr = x.double().requires_grad_(True)
        with kernel_rounding():
            o0 = ref(xr)
            o0.pow(2).sum().backward()
        g0 = [xr.grad] + [p.grad for p in ref.parameters()]
        got = [g1[0][:, :M, :18].transpose(0, 1)] + g1[1:]
        o1 = o1.double().cpu()
        assert (o1 - o0.detach()).norm().item() < 3e-3 * o0.norm().item()
        errs = [(a.double().cpu() - b_).norm().item() / (b_.norm().item() + 1e-6) for a, b_ in zip(got, g0)]
        print(f"seed {seed}: largest relative gradient error {max(errs):.4e}")
        worst.append(max(errs))
        assert max(errs) < 8e-3, (seed, errs)
    print(f"mean over seeds {sum(worst) / len(worst):.4e}, largest seed {max(worst):.4e}")
