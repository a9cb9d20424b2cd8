"""Chain forward (lstm_chain_fwd.hip chain_stage) at the sequence lengths where the H = 16 stages' step
pipeline can go wrong: the publisher wave runs two steps behind the cells and drains the last two
steps behind the loop, the H = 16 stream consumer has a ring depth of its own (D = CHAIN_D16S = 4)
and loads a 16-channel tile class.

* two H = 16 stages without a pool: T in {1, 2, 3, D - 1, D, D + 1, 2 D + 1}, M in {16, 40} (one tile;
  three tiles with 8 padding rows);
* the six-stage CML stack (16, 16, 32, 32, 64, 64 units, a pool of 3 behind every second stage, the
  last stage pooling its own output): T in {27, 28, 29, 36}, M in {16, 40}, through lstm_chain_fwd
  and through lstm_chain_head_fwd (time4 then consumes the last stage and writes its pooled input);
  and a 40-channel input (stage 0 with KX = 2).

Per stage h, the packed gates, c, the pooled output and the consumer-written pooled input are
compared with the float64 model that rounds where the kernel does (gnnqc/ops/lstm_chain_ref.py), in
relative Frobenius norm, train and inference instances. Bounds: one per quantity, three times the
largest error of the parent library (the commit before the H = 16 step was reordered) on these same
cases, all below the project's 3e-3. The new library's outputs are bit-equal to the parent's, so its
errors are the same; per-case figures of both are in profiles/chain_fwd_steps_tests.txt. Largest:

    h 4.465e-04   gates 4.382e-04   c 4.298e-04   pooled 4.373e-04

Exact: the argmax bytes and the pooled values against the kernel's own h; three launches over
reused granule addresses bitwise equal; no spin timeout, every workgroup finished, the epoch
advanced by one per launch; the padding rows (x = 0) all hold one and the same sequence, and values
in the input's pad channels (beyond the Dw rows of W) change nothing.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

D16S = 4                       # CHAIN_D16S (lstm_chain_fwd.hip)
# 3 x the parent library's largest error on these cases (profiles/chain_fwd_steps_tests.txt), <= 3e-3
BOUND = {"h": 1.34e-3, "g": 1.31e-3, "c": 1.29e-3, "pooled": 1.31e-3}


def _weights(units, din, seed, dev):
    g = torch.Generator().manual_seed(seed)
    Ws, Us, bs = [], [], []
    for i, H in enumerate(units):
        dw = din if i == 0 else units[i - 1]
        Ws.append((torch.randn(dw, 4 * H, generator=g) * 0.3).to(dev))
        Us.append((torch.randn(H, 4 * H, generator=g) * 0.3).to(dev))
        bs.append((torch.randn(4 * H, generator=g) * 0.1).to(dev))
    return Ws, Us, bs


def _input(T, M, din, seed, dev):
    """[T, Mp, din rounded up to 4]: rows past M and the pad channels zero."""
    Mp, dp = (M + 15) // 16 * 16, (din + 3) // 4 * 4
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(T, Mp, dp)
    x[:, :M, :din] = torch.randn(T, M, din, generator=g)
    return x.to(dev)


def _unpack(t, T, Mp, H, last):
    """Saved gates / c: [T + 1][tile][wave H / 4][lane = (quad, col)](4) with cell (unit 4 wave + quad,
    sequence 16 tile + col) -> [Mp, T, H(, 4)]."""
    v = t[:T].reshape(T, Mp // 16, H // 4, 4, 16, *last)
    perm = (1, 4, 0, 2, 3) + tuple(range(5, 5 + len(last)))
    return v.permute(*perm).reshape(Mp, T, H, *last)


def _launch(ops, x, Ws, Us, bs, pools, train, headed, M):
    if not headed:
        return ops.lstm_chain_fwd(x, Ws, Us, bs, pools, train)
    dev = x.device
    g = torch.Generator().manual_seed(5)
    W4 = (torch.randn(64, 512, generator=g) * 0.1).to(dev)
    U4 = (torch.randn(128, 512, generator=g) * 0.1).to(dev)
    b4 = torch.zeros(512, device=dev)
    head = [(torch.randn(128, 64, generator=g) * 0.1).to(dev), torch.zeros(64, device=dev),
            (torch.randn(64, 64, generator=g) * 0.1).to(dev), torch.zeros(64, device=dev),
            (torch.randn(64, 1, generator=g) * 0.1).to(dev), torch.zeros(1, device=dev)]
    y = torch.zeros(M, device=dev)
    mask = torch.ones(M, device=dev)
    e = torch.zeros(0, device=dev)
    return ops.lstm_chain_head_fwd(x, Ws, Us, bs, pools, train, W4, U4, b4, head, y, mask, M, 0.3, 0.3, 1.0, 5.0,
                                   e.double(), e)


def case_errors(dev, units, pools, din, T, M, train, headed=False, seed=0):
    """Runs one case three times; exact checks asserted here, relative errors against the float64
    model returned as {quantity: largest over the stages}."""
    from gnnqc.ops.lstm_chain_ref import chain_fwd_ref
    from gnnqc.utils.native import hip_ops
    ops = hip_ops()
    ns = len(units)
    Ws, Us, bs = _weights(units, din, seed, dev)
    x = _input(T, M, din, 1000 * T + M, dev)
    Mp = x.shape[1]
    st0 = ops.lstm_chain_status(x).cpu()
    runs = [[o.clone() for o in _launch(ops, x, Ws, Us, bs, pools, train, headed, M)[:5 * ns]] for _ in range(3)]
    torch.cuda.synchronize()
    st1 = ops.lstm_chain_status(x).cpu()
    assert int(st1[2]) == 0, "a consumer spin timed out"
    assert int(st1[0]) - int(st0[0]) == 3 and int(st1[1]) == 0, (st0, st1)
    # a pooled output exists where the stage's consumer (or, for the last stage, the stage) wrote it
    has_pool = [bool(pools[s]) for s in range(ns)]
    Ts = [T]
    for s in range(ns - 1):
        Ts.append(Ts[-1] // 3 if pools[s] else Ts[-1])
    outs = runs[0]
    for other in runs[1:]:
        for s in range(ns):
            for k in range(5):
                a, b = outs[5 * s + k], other[5 * s + k]
                if k in (1, 2) and a.numel():
                    a, b = a[:Ts[s]], b[:Ts[s]]             # (row T of g / c is scratch)
                assert torch.equal(a, b), (s, k)
    # values in the pad channels of x change nothing (W has Dw = din rows)
    if x.shape[2] > din:
        xg = x.clone()
        xg[..., din:] = 7.0
        og = _launch(ops, xg, Ws, Us, bs, pools, train, headed, M)[:5 * ns]
        torch.cuda.synchronize()
        assert all(torch.equal(og[5 * s], outs[5 * s]) for s in range(ns))
    ref = chain_fwd_ref(x.transpose(0, 1).double().cpu(), [w.double().cpu() for w in Ws], [u.double().cpu() for u in Us],
                        [b.double().cpu() for b in bs], pools)
    errs = {"h": 0.0, "g": 0.0, "c": 0.0, "pooled": 0.0}

    def rel(a, b):
        return ((a - b).norm() / (b.norm() + 1e-12)).item()

    for s in range(ns):
        H, Tt = units[s], Ts[s]
        h = outs[5 * s].transpose(0, 1).double().cpu()
        assert h.shape == (Mp, Tt, H) and torch.isfinite(h).all()
        errs["h"] = max(errs["h"], rel(h, ref[s]["h"]))
        if Mp > M:                                   # padding rows: x = 0, one and the same sequence
            assert torch.equal(h[M:], h[M:M + 1].expand(Mp - M, Tt, H))
        if train:
            g = _unpack(outs[5 * s + 1].float(), Tt, Mp, H, (4,)).double().cpu()
            c = _unpack(outs[5 * s + 2], Tt, Mp, H, ()).double().cpu()
            errs["g"] = max(errs["g"], rel(g, ref[s]["g"]))
            errs["c"] = max(errs["c"], rel(c, ref[s]["c"]))
        else:
            assert outs[5 * s + 1].numel() == 0 and outs[5 * s + 2].numel() == 0
        if has_pool[s]:        # (written by the consumer stage, by time4, or by a last stage that pools itself)
            pooled = outs[5 * s + 3].transpose(0, 1).cpu()
            idx = outs[5 * s + 4].transpose(0, 1).cpu()
            assert pooled.shape == (Mp, Tt // 3, H) and idx.shape == pooled.shape
            errs["pooled"] = max(errs["pooled"], rel(pooled.double(), ref[s]["pooled"]))
            # exact: the pool of the kernel's own h, first maximum wins
            w = outs[5 * s].transpose(0, 1).cpu()[:, :Tt // 3 * 3].reshape(Mp, Tt // 3, 3, H)
            m = w.max(2).values
            first = torch.where(w[:, :, 0] == m, 0, torch.where(w[:, :, 1] == m, 1, 2)).to(torch.uint8)
            assert torch.equal(pooled, m), s
            assert torch.equal(idx, first), s
    return errs


def _check(errs, train):
    for k, v in errs.items():
        print(f"  {k}: {v:.3e} (bound {BOUND[k]:.1e})")
    for k, v in errs.items():
        if train or k not in ("g", "c"):
            assert v <= BOUND[k], (k, v)


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("M", [16, 40])
@pytest.mark.parametrize("T", sorted({1, 2, 3, D16S - 1, D16S, D16S + 1, 2 * D16S + 1}))
def test_two_h16_stages_match_fp64_model(cuda_device, T, M, train):
    _check(case_errors(cuda_device, [16, 16], [0, 0], 18, T, M, train), train)


@pytest.mark.parametrize("headed", [False, True])
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("M", [16, 40])
@pytest.mark.parametrize("T", [27, 28, 29, 36])
def test_cml_stack_matches_fp64_model(cuda_device, T, M, train, headed):
    _check(case_errors(cuda_device, [16, 16, 32, 32, 64, 64], [0, 3, 0, 3, 0, 3], 18, T, M, train, headed), train)


@pytest.mark.parametrize("train", [True, False])
def test_wide_input_first_stage_matches_fp64_model(cuda_device, train):
    """40 input channels: stage 0 is the H = 16 stage with KX = 2."""
    _check(case_errors(cuda_device, [16, 16, 32, 32, 64, 64], [0, 3, 0, 3, 0, 3], 40, 28, 16, train), train)
