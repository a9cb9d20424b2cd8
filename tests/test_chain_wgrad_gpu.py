"""Weight-gradient records built inside the chain backward launch (``csrc/kernels/chain_wgrad.h``): the
H = 32 / 64 chain stages and time4 compute the dW | db and dU partial of their own 16-sequence tile after
their reverse steps; ``lstm_grads_multi`` then only reduces them (and still runs the H = 16 layers' jobs).

``lstm_chain_head_fwd`` / ``lstm_chain_head_bwd`` and ``lstm_grads_multi`` are called directly on the CML
stack (widths 16/16/32/32/64/64 + time4 128, pools 3/3/3; din tiles 2, 3, 3, 5 and 5 on the upper layers:
the 64-channel H = 64 layer and time4 have DT = 5), in both modes: the records built by the chain launch
(``wgrad`` lists) and by the jobs of the tail launch (the path before this change).

Reference: each upper layer's dW, dU, db as float64 products of the returned bf16 dz with x and h_{t-1}
rounded to bf16 - the operands the kernels multiply - over the real sequences only, so padding sequences
must contribute exactly 0 (``wgrad_reference``; ``tests/test_chain_wgrad_reference_cpu.py`` checks it
against autograd and asserts the discriminating power of the bound).

Shapes: T = 27 (-> 9 -> 3 -> 1: odd pair counts everywhere, time4 with a single step and no h_{t-1}) and
T = 54 (-> 18 -> 6 -> 2: even); M = 16 (one tile), M = 20 (Mp = 32, 12 padding sequences) and M = 128 (8
tiles); one case also with the gradient buffers pre-filled (accumulation is +=: the pre-filled result is
the constant plus the result on zeroed buffers, bit for bit).

Metric: relative Frobenius error per quantity (dW, dU, db), worst over the upper layers. Bound: 3 x the
tail-launch path's worst error over these same cases, measured on an MI355X (:data:`PARENT_WORST`;
fp32 accumulation in another, fixed order may differ in the last bits, not more). The per-case figures
of both modes are in ``profiles/chain_wgrad_epilogue_tests.txt``."""
import copy

import pytest
import torch

UNITS = [16, 16, 32, 32, 64, 64, 128]
POOLS = [0, 3, 0, 3, 0, 3]
UPPER = [2, 3, 4, 5, 6]                 # layers whose records the chain launch builds
DIN, DW0 = 20, 18
CONSTS = (0.3, 0.3, 1.0, 5.0)           # alpha1, alpha2, w0, w1
PREFILL = 0.5                           # bf16-exact

# (name, M, T, prefill)
CASES = [
    ("m16_t27", 16, 27, 0.0),
    ("m20_t54", 20, 54, 0.0),
    ("m20_t27_prefill", 20, 27, PREFILL),
    ("m128_t27", 128, 27, 0.0),
    ("m128_t54", 128, 54, 0.0),
]
QUANT = ("dW", "dU", "db")
# worst relative Frobenius error of the tail-launch path (no wgrad lists: the path of the commit before)
# over CASES and UPPER, per quantity, on an MI355X
PARENT_WORST = {"dW": 7.584e-08, "dU": 7.547e-08, "db": 5.130e-08}
BOUND = {k: 3.0 * v for k, v in PARENT_WORST.items()}
MUTANT_FACTOR = 5.0


def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


# ---------------------------------------------------------------- float64 reference (CPU)
def wgrad_reference(dz, x, h, M, mut=None):
    """dz [>= T, Mp, 4H] (bf16 values), x [T, Mp, >= Dw], h [T, Mp, H] of one layer, time-major; the first M
    sequences are real. float64 (dW [x width, 4H], dU, db) of the bf16-rounded operands. ``mut``: 'h0'
    (h_{t-1} of t = 0 not zeroed: the clamped row h_0 in its place), 'odd_last' (the masked second step
    of an odd T's last pair not masked: the rows clamped to step T - 1 counted once more), 'pad' (padding
    sequences included)."""
    T = h.shape[0]
    m = dz.shape[1] if mut == "pad" else M
    z = dz[:T, :m].double()
    xb = _bf(x[:T, :m].float()).double()
    hb = _bf(h[:T, :m].float()).double()
    hprev = torch.cat([hb[:1] if mut == "h0" else torch.zeros_like(hb[:1]), hb[:T - 1]], 0)
    if mut == "odd_last" and T % 2 == 1:         # step T: dz and x rows clamped to T - 1, its h_{t-1} is h_{T-1}
        z, xb, hprev = torch.cat([z, z[T - 1:]], 0), torch.cat([xb, xb[T - 1:]], 0), torch.cat([hprev, hb[T - 1:]], 0)
    return dict(dW=torch.einsum("tmd,tmg->dg", xb, z), dU=torch.einsum("tmk,tmg->kg", hprev, z), db=z.sum((0, 1)))


def rel_err(a, r):
    return (a - r).norm().item() / max(r.norm().item(), 1e-300)


# ---------------------------------------------------------------- device side
def _labels(M, gen, dev):
    y = (torch.rand(M, generator=gen) < 0.3).float()
    mask = (torch.rand(M, generator=gen) < 0.7).float()
    mask[0], mask[M - 1] = 1.0, 0.0
    return y.to(dev), mask.to(dev)


def _params(gen, dev):
    Ws, Us, bs = [], [], []
    for i, H in enumerate(UNITS):
        dw = DW0 if i == 0 else UNITS[i - 1]
        Ws.append((torch.randn(dw, 4 * H, generator=gen) * 0.3).to(dev))
        Us.append((torch.randn(H, 4 * H, generator=gen) * 0.3).to(dev))
        bs.append((torch.randn(4 * H, generator=gen) * 0.1).to(dev))
    head = [(torch.randn(*s, generator=gen) * 0.1).to(dev) for s in ((128, 64), (64,), (64, 64), (64,), (64, 1), (1,))]
    return Ws, Us, bs, head


_FORWARD = {}


def forward_state(case, dev):
    """Inputs and the forward launch's results of a case, computed once per process and left unchanged."""
    name, M, T, _ = case
    if name not in _FORWARD:
        from gnnqc.utils.native import hip_ops
        ops = hip_ops()
        Mp = (M + 15) // 16 * 16
        gen = torch.Generator().manual_seed(4100 * M + T)
        Ws, Us, bs, head = _params(gen, dev)
        y, mask = _labels(M, gen, dev)
        x = torch.randn(T, Mp, DIN, generator=gen).to(dev)
        e = torch.zeros(0, device=dev)
        ns = len(POOLS)
        outs = ops.lstm_chain_head_fwd(x, Ws[:ns], Us[:ns], bs[:ns], POOLS, True, Ws[ns], Us[ns], bs[ns], head, y, mask,
                                       M, *CONSTS, e.double(), e)
        h4, g4, c4 = outs[-5:-2]
        hb, pk = outs[-6], outs[-7]
        outs = outs[:-7]
        xs = [x] + [outs[5 * i + 3] if POOLS[i] else outs[5 * i] for i in range(ns)]     # layer inputs
        hs = [outs[5 * i] for i in range(ns)] + [h4]
        _FORWARD[name] = dict(M=M, Mp=Mp, T=T, Ws=Ws, Us=Us, head=head, y=y, mask=mask, x=x, outs=outs, h4=h4, g4=g4,
                              c4=c4, hb=hb, pk=pk, xs=xs, hs=hs)
    return _FORWARD[name]


def backward(case, dev, chain, frozen=()):
    """One backward launch + ``lstm_grads_multi`` on fresh gradient buffers. chain: the upper layers' records
    are built by the chain launch; ``frozen`` layers get neither a record nor a job nor a reduction. Returns
    ([dz per layer], {layer: [dW, dU, db]}, {layer: workspace})."""
    from gnnqc.utils.native import hip_ops
    ops = hip_ops()
    s = forward_state(case, dev)
    prefill = case[3]
    ns = len(POOLS)
    order = list(reversed(range(ns)))
    Ws, Us, outs, Mp = s["Ws"], s["Us"], s["outs"], s["Mp"]
    e = torch.zeros(0, device=dev)
    e8 = torch.zeros(0, dtype=torch.uint8, device=dev)
    xw = [DIN] + UNITS[:ns - 1]
    chain_args = ([outs[5 * i + 1] for i in order], [outs[5 * i + 2] for i in order], [Ws[i] for i in order],
                  [Us[i] for i in order], [outs[5 * i + 4] if POOLS[i] else e8 for i in order],
                  [POOLS[i] for i in order], [xw[i] for i in order], [outs[5 * i].shape[0] for i in order])
    hg = [torch.zeros_like(p) for p in s["head"]]
    wws = {i: ops.lstm_grads_record_ws(Ws[i], Mp // 16) for i in UPPER if chain and i not in frozen}
    wgrad = None
    if chain:
        wgrad = [t for i in order for t in (s["xs"][i], s["hs"][i], wws.get(i, e))] + [wws.get(ns, e)]
    res = ops.lstm_chain_head_bwd(torch.ones(1, device=dev), s["xs"][ns], s["h4"], s["g4"], s["c4"], Ws[ns], Us[ns],
                                  s["pk"], s["hb"], s["head"], s["y"], s["mask"], s["M"], *CONSTS, hg, *chain_args, wgrad)
    dzs = {ns: res[0]}
    for k, i in enumerate(order):
        dzs[i] = res[1 + k]
    g = {i: [torch.full_like(Ws[i], prefill), torch.full_like(Us[i], prefill),
             torch.full((4 * UNITS[i],), prefill, device=dev)] for i in range(ns + 1)}
    jobs = [i for i in range(ns + 1) if i not in wws and i not in frozen]
    jws = {i: ops.lstm_grads_job_ws(dzs[i], s["xs"][i], Ws[i], UNITS[i]) for i in jobs}
    reds = [i for i in range(ns + 1) if i not in frozen]
    rws = {**jws, **wws}
    rows = lambda i: s["hs"][i].shape[0] * Mp
    ops.lstm_grads_multi([dzs[i] for i in jobs], [s["xs"][i] for i in jobs], [s["hs"][i] for i in jobs],
                         [Ws[i] for i in jobs], [rows(i) for i in jobs], [Mp for _ in jobs], [jws[i] for i in jobs],
                         [rws[i] for i in reds], [Ws[i] for i in reds], [g[i][0] for i in reds], [g[i][1] for i in reds],
                         [g[i][2] for i in reds], [], [])
    torch.cuda.synchronize()
    st = ops.lstm_chain_status(s["x"]).cpu()
    assert int(st[2]) == 0, "a consumer spin timed out"
    return dzs, g, wws


def errors(case, dev, dzs, g):
    """{(layer, quantity): relative Frobenius error} of the upper layers against the float64 reference."""
    s = forward_state(case, dev)
    out = {}
    for i in UPPER:
        Dw = s["Ws"][i].shape[0]
        ref = wgrad_reference(dzs[i].float().cpu(), s["xs"][i][..., :Dw].cpu(), s["hs"][i].cpu(), s["M"])
        for q, a in zip(QUANT, g[i]):
            out[(i, q)] = rel_err(a.double().cpu() - case[3], ref[q])
    return out


# ---------------------------------------------------------------- tests
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_chain_records_against_float64(cuda_device, case):
    """Both modes against the reference; the new path twice: bitwise-equal gradients; dz is the same."""
    plain = (*case[:3], 0.0)                     # the errors are measured on zeroed buffers
    dz0, g0, _ = backward(plain, cuda_device, chain=False)
    dz1, g1, _ = backward(plain, cuda_device, chain=True)
    dz2, g2, _ = backward(plain, cuda_device, chain=True)
    if case[3] != 0.0:
        # += : on buffers holding a constant the result is that constant plus the sum found on zeroed
        # buffers, rounded once to fp32 - bit for bit, since the summation order is fixed
        _, gp, _ = backward(case, cuda_device, chain=True)
        for i in range(len(UNITS)):
            for a, b, q in zip(gp[i], g1[i], QUANT):
                assert torch.equal(a, case[3] + b), ("accumulation", i, q)
    case = plain
    for i in dz0:
        T = forward_state(case, cuda_device)["hs"][i].shape[0]
        assert torch.equal(dz0[i][:T].view(torch.int16), dz1[i][:T].view(torch.int16)), ("dz", i)
    s = forward_state(case, cuda_device)
    for i in UPPER:                              # padding sequences carry no gradient at all
        assert float(dz1[i][:s["hs"][i].shape[0], s["M"]:].float().abs().max() if s["Mp"] > s["M"] else 0.0) == 0.0
    e0, e1 = errors(case, cuda_device, dz0, g0), errors(case, cuda_device, dz1, g1)
    for (i, q), v in sorted(e1.items()):
        print(f"WGRAD {case[0]} layer{i}_H{UNITS[i]} {q} tail={e0[(i, q)]:.3e} chain={v:.3e}")
    for i in range(len(UNITS)):
        for a, b, q in zip(g1[i], g2[i], QUANT):
            assert torch.equal(a, b), ("second run differs", i, q)
    for i in (0, 1):                             # the H = 16 layers keep their jobs: the same arithmetic
        for a, b, q in zip(g0[i], g1[i], QUANT):
            assert torch.equal(a, b), ("H = 16 layer changed", i, q)
    failures = [f"layer {i} {q}: {v:.3e} > {BOUND[q]:.1e}" for (i, q), v in sorted(e1.items()) if not v <= BOUND[q]]
    assert not failures, "; ".join(failures)


@pytest.mark.gpu
def test_frozen_layers_write_no_record_and_touch_no_buffer(cuda_device):
    """Layers without a workspace in the wgrad lists (frozen weights) run the stage as before: their
    gradient buffers keep the pre-filled value, the other layers' gradients are bit-equal to a run with
    every layer on."""
    case = CASES[2]
    _, g_all, _ = backward(case, cuda_device, chain=True)
    _, g_fr, wws = backward(case, cuda_device, chain=True, frozen=(3, 6))
    assert set(wws) == {2, 4, 5}
    for i in (3, 6):
        for a in g_fr[i]:
            assert torch.equal(a, torch.full_like(a, PREFILL)), i
    for i in (0, 1, 2, 4, 5):
        for a, b in zip(g_all[i], g_fr[i]):
            assert torch.equal(a, b), i


@pytest.mark.gpu
def test_epilogue_refuses_a_wrong_workspace(cuda_device):
    from gnnqc.utils.native import hip_ops
    ops = hip_ops()
    s = forward_state(CASES[0], cuda_device)
    with pytest.raises(RuntimeError, match="records"):
        ops.lstm_grads_record_ws(s["Ws"][2], 0)
    ws = ops.lstm_grads_record_ws(s["Ws"][2], s["Mp"] // 16)
    assert ws.numel() == (s["Mp"] // 16) * ((16 + 16) // 16 + 2) * 1024 * 2


@pytest.mark.gpu
def test_trainer_step_with_and_without_chain_records(cuda_device, monkeypatch):
    """One Trainer step at B = 32, T = 27 with the switch on and off: the LSTM stack's and the head's
    parameters (everything the switch can reach; the GCN's come from float atomics) agree within the
    bound scaled by the learning rate - the first Adam step moves every element by about lr, so the
    measure is the bound times the update's norm - plus the fp32 rounding of the stored parameter."""
    from gnnqc import config as C
    from gnnqc.data.preprocessing import create_windows_dataset
    from gnnqc.data.store import DeviceStore
    from gnnqc.data.synthetic import make_cml_raw
    from gnnqc.models import GCNClassifier
    from gnnqc.ops import lstm_chain as L
    from gnnqc.ops.optim import make_optimizer
    from gnnqc.train.engine import Trainer
    lr = 1e-3
    pc = C.normalize_preproc(C.default("preprocessing_cml"))
    pc.timestep_before, pc.timestep_after = 17, 9
    ws = create_windows_dataset(pc, raw=make_cml_raw(n_sensors=8, n_minutes=2 * 1440, seed=5))
    st = DeviceStore(ws, "rolling_median", pc.graph, device=cuda_device)
    torch.manual_seed(0)
    model = GCNClassifier(C.default("model_cml"), pc).to(cuda_device)
    ids = torch.randperm(st.n_windows, generator=torch.Generator().manual_seed(3))[:32].to(cuda_device)
    assert st.gather(ids).model_inputs("cml")[0].shape[1] == 27
    res = {}
    for on in (True, False):
        monkeypatch.setattr(L._ChainWgrad, "on", on)
        m = copy.deepcopy(model)
        tr = Trainer(m, st, make_optimizer("adam", m.parameters(), lr), {0: 1.0, 1: 5.0}, use_graph=False, batch_size=32)
        loss = float(tr.train_step(ids).item())
        torch.cuda.synchronize()
        res[on] = (loss, {n: p.detach().clone() for n, p in m.named_parameters()})
    assert res[True][0] == res[False][0]
    bound = max(BOUND.values())
    init = dict(model.named_parameters())
    moved = 0
    for n, p0 in res[False][1].items():
        if n.startswith("gcn_layer"):
            continue
        d0 = p0 - init[n].detach()
        moved += int(d0.abs().max().item() > 0)
        err = (res[True][1][n] - p0).norm().item()
        # the update (every element about lr) within the gradients' bound, plus what storing the new value
        # in fp32 can add: half a unit in the last place of each parameter at most, taken as |p| 2^-24
        allowed = bound * d0.norm().item() + (p0.abs() * 2.0 ** -24).norm().item()
        print(f"WGRAD trainer {n} |update| {d0.norm().item():.3e} |difference| {err:.3e} allowed {allowed:.3e}")
        assert err <= allowed, (n, err, allowed)
    assert moved >= 26          # (time4's recurrent kernel has no gradient at a single step)
