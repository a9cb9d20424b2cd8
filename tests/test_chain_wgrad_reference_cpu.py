"""CPU part of the chain weight-gradient tests (``tests/test_chain_wgrad_gpu.py``): the float64 reference
agrees with autograd on a plain LSTM, and the GPU bound tells the three ways the epilogue's row tiling can
go wrong apart: each named mutant of the reference lies at least 5 bounds away on every upper layer's
geometry (odd T, 12 padding sequences)."""
import pytest
import torch

import test_chain_wgrad_gpu as S

# (H, Dw, T) of the upper layers at T = 27 (-> 9 -> 3 -> 1) with M = 20 real of Mp = 32 sequences
GEOMS = [(32, 16, 9), (32, 32, 9), (64, 32, 3), (64, 64, 3), (128, 64, 1)]
M, MP = 20, 32


def _synthetic(H, Dw, T):
    gen = torch.Generator().manual_seed(5200 + 31 * H + Dw + T)
    return (S._bf(torch.randn(T + 1, MP, 4 * H, generator=gen)), S._bf(torch.randn(T, MP, Dw, generator=gen)),
            S._bf(torch.randn(T, MP, H, generator=gen) * 0.5))


def test_cases_cover_the_shapes_that_can_go_wrong():
    Ts, Ms = {c[2] for c in S.CASES}, {c[1] for c in S.CASES}
    assert {27, 54} <= Ts and {16, 20, 128} <= Ms and any(c[3] != 0 for c in S.CASES)
    assert float(torch.tensor(S.PREFILL).to(torch.bfloat16)) == S.PREFILL
    # din tiles of the upper layers: the 64-channel H = 64 layer and time4 have 5
    assert [(S.UNITS[i - 1] + 16) // 16 for i in S.UPPER] == [2, 3, 3, 5, 5]
    assert set(S.BOUND) == set(S.QUANT) and all(S.BOUND[q] == 3.0 * S.PARENT_WORST[q] for q in S.QUANT)


@pytest.mark.parametrize("T", [1, 4, 5])
def test_reference_is_autograd_of_a_plain_lstm(T):
    """dW, dU, db of a float64 LSTM whose recurrent input is its bf16-rounded state (what the kernels
    multiply) == the reference fed with autograd's own dz."""
    H, Dw = 16, 6
    gen = torch.Generator().manual_seed(77 + T)
    x = S._bf(torch.randn(T, M, Dw, generator=gen)).double()
    W = (torch.randn(Dw, 4 * H, generator=gen) * 0.3).double().requires_grad_(True)
    U = (torch.randn(H, 4 * H, generator=gen) * 0.3).double().requires_grad_(True)
    b = (torch.randn(4 * H, generator=gen) * 0.1).double().requires_grad_(True)
    r = torch.randn(T, M, H, generator=gen).double()
    h = torch.zeros(M, H, dtype=torch.float64)
    c = torch.zeros(M, H, dtype=torch.float64)
    zs, hs = [], []
    for t in range(T):
        hin = h + (S._bf(h.detach().float()).double() - h.detach())        # bf16 value, straight-through gradient
        z = x[t] @ W + hin @ U + b
        z.retain_grad()
        i, f, g, o = z.split(H, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        zs.append(z)
        hs.append(h)
    (torch.stack(hs) * r).sum().backward()
    dz = torch.stack([z.grad for z in zs])
    ref = S.wgrad_reference(dz, x, torch.stack(hs).detach(), M)
    for q, a in (("dW", W.grad), ("dU", U.grad), ("db", b.grad)):
        assert (ref[q] - a).abs().max().item() <= 1e-12 * max(1.0, a.abs().max().item()), q


@pytest.mark.parametrize("geom", GEOMS, ids=[f"h{g[0]}_d{g[1]}_t{g[2]}" for g in GEOMS])
def test_every_mutant_is_five_bounds_away(geom):
    H, Dw, T = geom
    dz, x, h = _synthetic(H, Dw, T)
    ref = S.wgrad_reference(dz, x, h, M)
    bound = max(S.BOUND.values())
    # (a single step has no h_{t-1}: dU is zero with or without the padding sequences)
    pad_moves = S.QUANT if T > 1 else ("dW", "db")
    for mut, quants in (("h0", ("dU",)), ("odd_last", S.QUANT), ("pad", pad_moves)):
        m = S.wgrad_reference(dz, x, h, M, mut)
        for q in quants:
            dist = S.rel_err(m[q], ref[q])
            print(f"WGRADMUT h{H}_d{Dw}_t{T} {mut} {q} {dist / bound:.3g}")
            assert dist / bound >= S.MUTANT_FACTOR, f"mutant {mut} moves {q} by {dist:.3e} only"
        for q in set(S.QUANT) - set(quants):
            assert torch.equal(m[q], ref[q]), (mut, q)
