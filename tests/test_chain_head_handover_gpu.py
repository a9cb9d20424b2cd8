"""The hand-over between the two recurrences of the CML step: the classifier head + weighted BCE at the
end of the chain forward launch (lstm_chain_head_fwd) and its backward, of which the forward launch
computes dh_{T-1} and the backward launch the weight-gradient records (lstm_chain_head_bwd), against a
float64 reference of the head with time4's output taken as given.

Reference: Dense 64, LeakyReLU .3, Dense 64, LeakyReLU .3, Dense 1, class-weighted binary cross-entropy
with SUM_OVER_BATCH_SIZE over the mask. Its closed-form gradients are checked against torch autograd on
the CPU (unmarked test); the GPU tests compare the kernels with it on the smallest shapes that can still
go wrong: one tile (M = 16) and three tiles with eight padding rows (M = 40), one time4 step (T = 27, 28)
and two (T = 54), a mask with zeros and an all-zero mask, dL/dloss = 1 and 0.37, both values of
GNNQC_HEAD_BWD_IN_FWD, and every case twice on the same buffers (the counters are re-armed; the second
call equals the first bit for bit).

Quantities: dW1, db1, dW2, db2, dW3, db3, the loss, and the gradient of the head's LSTM input h_{T-1},
seen twice: as the forward launch's dh tile (default mode only; dL/dloss = 1 there, scaled here) and as
time4's first reverse dz (both modes; bf16, from the float64 dh and the saved gates / cells).

Bounds: four times the worst relative Frobenius error of the commit before the hand-over change, per
quantity, over these same cases (profiles/chain_head_handover_tests.txt holds both commits' figures)."""
import pytest
import torch

UNITS = [16, 16, 32, 32, 64, 64, 128]
POOLS = [0, 3, 0, 3, 0, 3]
DIN, DW0 = 20, 18
CONSTS = (0.3, 0.3, 1.0, 5.0)          # alpha1, alpha2, w0, w1

# (name, M, T, mask kind)
CASES = [
    ("m16_t27_zeros", 16, 27, "zeros"),
    ("m40_t28_zeros", 40, 28, "zeros"),
    ("m40_t54_zeros", 40, 54, "zeros"),
    ("m16_t54_ones", 16, 54, "ones"),
    ("m40_t27_allzero", 40, 27, "allzero"),
]
DLOSS = [1.0, 0.37]
MODES = ["1", "0"]                      # GNNQC_HEAD_BWD_IN_FWD

# worst relative Frobenius error of the parent commit over CASES x DLOSS x MODES (all-zero masks
# excluded: every gradient is exactly zero there)
PARENT_WORST = {
    "dW1": 3.582e-07, "db1": 3.722e-07, "dW2": 3.411e-07, "db2": 2.097e-07, "dW3": 3.024e-07, "db3": 2.771e-07,
    "loss": 1.090e-07, "dh": 2.121e-07, "dz_last": 1.777e-03,
}
BOUND = {k: 4.0 * v for k, v in PARENT_WORST.items()}


# ---------------------------------------------------------------- float64 reference of the head

def head_reference(h, head, y, mask, dloss, consts=CONSTS):
    """h [M, F] (time4's last state), head = [W1 [F, 64], b1, W2 [64, 64], b2, W3 [64, 1], b3], all
    float64. Returns loss and the closed-form gradients times dloss."""
    a1c, a2c, w0, w1 = consts
    W1, b1, W2, b2, W3, b3 = head
    z1 = h @ W1 + b1
    a1 = torch.where(z1 > 0, z1, a1c * z1)
    z2 = a1 @ W2 + b2
    a2 = torch.where(z2 > 0, z2, a2c * z2)
    z = (a2 @ W3.reshape(-1, 1)).reshape(-1) + b3.reshape(())
    wc = torch.where(y > 0.5, torch.full_like(y, w1), torch.full_like(y, w0))
    per = torch.clamp(z, min=0) - z * y + torch.log1p(torch.exp(-z.abs()))
    n = torch.clamp(mask.sum(), min=1.0)
    loss = (mask * wc * per).sum() / n
    d = dloss / n * mask * wc * (torch.sigmoid(z) - y)                 # dL/dz [M]
    dW3 = (a2 * d[:, None]).sum(0).reshape(W3.shape)
    db3 = d.sum().reshape(b3.shape)
    dz2 = d[:, None] * W3.reshape(1, -1) * torch.where(z2 > 0, torch.ones_like(z2), torch.full_like(z2, a2c))
    dW2 = a1.t() @ dz2
    db2 = dz2.sum(0)
    dz1 = (dz2 @ W2.t()) * torch.where(z1 > 0, torch.ones_like(z1), torch.full_like(z1, a1c))
    dW1 = h.t() @ dz1
    db1 = dz1.sum(0)
    dh = dz1 @ W1.t()
    return {"loss": loss, "dW1": dW1, "db1": db1, "dW2": dW2, "db2": db2, "dW3": dW3, "db3": db3, "dh": dh}


def _autograd_head(h, head, y, mask, dloss, consts=CONSTS):
    a1c, a2c, w0, w1 = consts
    h = h.clone().requires_grad_(True)
    ps = [p.clone().requires_grad_(True) for p in head]
    W1, b1, W2, b2, W3, b3 = ps
    x = torch.nn.functional.leaky_relu(h @ W1 + b1, a1c)
    x = torch.nn.functional.leaky_relu(x @ W2 + b2, a2c)
    z = (x @ W3.reshape(-1, 1)).reshape(-1) + b3.reshape(())
    wc = torch.where(y > 0.5, torch.full_like(y, w1), torch.full_like(y, w0))
    per = torch.nn.functional.binary_cross_entropy_with_logits(z, y, reduction="none")
    loss = (mask * wc * per).sum() / torch.clamp(mask.sum(), min=1.0)
    loss.backward(torch.tensor(dloss, dtype=loss.dtype))
    out = {"loss": loss.detach(), "dh": h.grad}
    out.update({k: p.grad for k, p in zip(["dW1", "db1", "dW2", "db2", "dW3", "db3"], ps)})
    return out


def _labels(M, kind, gen, device="cpu"):
    y = (torch.rand(M, generator=gen) < 0.3).float()
    if kind == "zeros":
        mask = (torch.rand(M, generator=gen) < 0.7).float()
        mask[0], mask[M - 1] = 1.0, 0.0
    elif kind == "ones":
        mask = torch.ones(M)
    else:
        mask = torch.zeros(M)
    return y.to(device), mask.to(device)


def _head_params(gen, dtype=torch.float32):
    return [(torch.randn(128, 64, generator=gen) * 0.1).to(dtype), (torch.randn(64, generator=gen) * 0.1).to(dtype),
            (torch.randn(64, 64, generator=gen) * 0.1).to(dtype), (torch.randn(64, generator=gen) * 0.1).to(dtype),
            (torch.randn(64, 1, generator=gen) * 0.1).to(dtype), (torch.randn(1, generator=gen) * 0.1).to(dtype)]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("dloss", DLOSS)
def test_reference_matches_autograd_cpu(case, dloss):
    """The closed-form float64 head gradients == torch autograd on the same cases."""
    _, M, _, kind = case
    gen = torch.Generator().manual_seed(M + len(kind))
    head = _head_params(gen, torch.float64)
    y, mask = _labels(M, kind, gen)
    h = torch.tanh(torch.randn(M, 128, generator=gen)).double()
    r = head_reference(h, head, y.double(), mask.double(), dloss)
    a = _autograd_head(h, head, y.double(), mask.double(), dloss)
    for k in r:
        err = (r[k] - a[k]).norm().item()
        assert err <= 1e-12 * a[k].norm().item() + 1e-300, (k, err, a[k].norm().item())
        if kind == "allzero" and k != "loss":
            assert float(r[k].abs().max()) == 0.0, k


# ---------------------------------------------------------------- the kernels

def _t4_state(g4, c4, T4, Mp):
    """time4's saved gates / cells of the last step in [Mp, 128, *] order (t4_sidx layout:
    [t][tile][gi & 7][gi >> 3][quad][col], unit = 4 gi + quad, row = 16 tile + col)."""
    nt = Mp // 16

    def un(v, k):
        v = v.view(T4, nt, 8, 4, 4, 16, k)[T4 - 1]          # [tile, a, b, quad, col, k]
        return v.permute(0, 4, 2, 1, 3, 5).reshape(Mp, 128, k)
    return un(g4, 4), un(c4, 2)


def _run(ops, dev, case, dloss, mode, monkeypatch):
    """Two forward + backward passes of the headed chain on the same inputs and gradient sinks.
    Returns the observed quantities of both passes."""
    _, M, T, kind = case
    Mp = (M + 15) // 16 * 16
    gen = torch.Generator().manual_seed(1000 * M + T)
    Ws, Us, bs = [], [], []
    for i, H in enumerate(UNITS):
        dw = DW0 if i == 0 else UNITS[i - 1]
        Ws.append((torch.randn(dw, 4 * H, generator=gen) * 0.3).to(dev))
        Us.append((torch.randn(H, 4 * H, generator=gen) * 0.3).to(dev))
        bs.append((torch.randn(4 * H, generator=gen) * 0.1).to(dev))
    head = [p.to(dev) for p in _head_params(gen)]
    y, mask = _labels(M, kind, gen, dev)
    x = torch.randn(T, Mp, DIN, generator=gen).to(dev)
    e = torch.zeros(0, device=dev)
    e8 = torch.zeros(0, dtype=torch.uint8, device=dev)
    gl = torch.full((1,), dloss, device=dev)
    hg = [torch.zeros_like(p) for p in head]
    monkeypatch.setenv("GNNQC_HEAD_BWD_IN_FWD", mode)
    ns = len(POOLS)
    order = list(reversed(range(ns)))
    xw = [DIN] + UNITS[:ns - 1]
    passes = []
    for _ in range(2):
        for g in hg:
            g.zero_()
        outs = ops.lstm_chain_head_fwd(x, Ws[:ns], Us[:ns], bs[:ns], POOLS, True, Ws[ns], Us[ns], bs[ns], head, y, mask,
                                       M, *CONSTS, e.double(), e)
        h4, g4, c4, logits, loss = outs[-5:]
        hb, pk = outs[-6], outs[-7]
        outs = outs[:-7]
        xt = outs[5 * (ns - 1) + 3]
        chain_args = ([outs[5 * i + 1] for i in order], [outs[5 * i + 2] for i in order], [Ws[i] for i in order],
                      [Us[i] for i in order], [outs[5 * i + 4] if POOLS[i] else e8 for i in order],
                      [POOLS[i] for i in order], [xw[i] for i in order], [outs[5 * i].shape[0] for i in order])
        res = ops.lstm_chain_head_bwd(gl, xt, h4, g4, c4, Ws[ns], Us[ns], pk, hb, head, y, mask, M, *CONSTS, hg,
                                      *chain_args)
        torch.cuda.synchronize()
        T4 = h4.shape[0]
        o = {"loss": loss.clone(), "logits": logits.clone(), "h_last": h4[T4 - 1, :M].clone(),
             "dz_last": res[0][T4 - 1, :M].clone(), "dz4": res[0][:T4].clone(), "dx": res[-1].clone(),
             "dh_fwd": hb[:Mp * 128].view(Mp, 128)[:M].clone() if hb.numel() > 0 else None,
             "g4": g4, "c4": c4, "T4": T4, "Mp": Mp}
        for k, g in zip(["dW1", "db1", "dW2", "db2", "dW3", "db3"], hg):
            o[k] = g.clone()
        passes.append(o)
    st = ops.lstm_chain_status(x).cpu()
    assert int(st[2]) == 0, "a consumer spin timed out"
    return passes, (head, y, mask)


def _rel(a, ref):
    return (a.double().cpu() - ref).norm().item() / max(ref.norm().item(), 1e-300)


def _errors(o, head, y, mask, dloss, M):
    """Relative Frobenius errors of one pass against the float64 reference."""
    ref = head_reference(o["h_last"].double().cpu(), [p.double().cpu() for p in head], y.double().cpu(),
                         mask.double().cpu(), dloss)
    g, c = _t4_state(o["g4"].double().cpu(), o["c4"].double().cpu(), o["T4"], o["Mp"])
    g, c = g[:M], c[:M]
    gi, gf, gg, go = g.unbind(-1)
    ct, cprev = c.unbind(-1)
    tc = torch.tanh(ct)
    dh = ref["dh"]
    dct = dh * go * (1 - tc * tc)
    ref["dz_last"] = torch.cat([dct * gg * gi * (1 - gi), dct * cprev * gf * (1 - gf), dct * gi * (1 - gg * gg),
                                dh * tc * go * (1 - go)], dim=1)
    err = {}
    for k in ["dW1", "db1", "dW2", "db2", "dW3", "db3", "loss", "dz_last"]:
        err[k] = _rel(o[k].reshape(ref[k].shape), ref[k])
    if o["dh_fwd"] is not None:                 # the forward launch's tile holds dh for dL/dloss = 1
        err["dh"] = _rel(o["dh_fwd"].double() * dloss, ref["dh"])
    return err, ref


BITWISE = ["loss", "logits", "dW1", "db1", "dW2", "db2", "dW3", "db3", "dz4", "dx"]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=["in_fwd", "in_bwd"])
@pytest.mark.parametrize("dloss", DLOSS)
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_head_handover_against_float64(cuda_device, monkeypatch, case, dloss, mode):
    from gnnqc.utils.native import hip_ops
    name, M, T, kind = case
    passes, (head, y, mask) = _run(hip_ops(), cuda_device, case, dloss, mode, monkeypatch)
    first, second = passes
    for k in BITWISE:                           # the second call on the same buffers == the first
        assert torch.equal(first[k], second[k]), (k, "second call differs")
    err, ref = _errors(first, head, y, mask, dloss, M)
    print("handover", name, "dloss", dloss, "mode", mode, " ".join(f"{k}={v:.3e}" for k, v in sorted(err.items())))
    for k in BITWISE:
        assert torch.isfinite(first[k].float()).all(), k
    if kind == "allzero":                       # max(n, 1): no division by zero, every gradient exactly 0
        assert float(first["loss"]) == 0.0
        for k in ["dW1", "db1", "dW2", "db2", "dW3", "db3", "dz4", "dx"]:
            assert float(first[k].float().abs().max()) == 0.0, k
        if first["dh_fwd"] is not None:
            assert float(first["dh_fwd"].abs().max()) == 0.0
        return
    for k, v in err.items():
        assert v <= BOUND[k], (k, v, BOUND[k])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_head_handover_modes_agree_bitwise(cuda_device, monkeypatch, case):
    """dL/dloss = 1: the default mode and GNNQC_HEAD_BWD_IN_FWD=0 run the same arithmetic, so the head
    gradients, dh (through time4's dz) and everything downstream are bit-equal."""
    from gnnqc.utils.native import hip_ops
    a, _ = _run(hip_ops(), cuda_device, case, 1.0, "1", monkeypatch)
    b, _ = _run(hip_ops(), cuda_device, case, 1.0, "0", monkeypatch)
    for k in BITWISE:
        assert torch.equal(a[0][k], b[0][k]), k
