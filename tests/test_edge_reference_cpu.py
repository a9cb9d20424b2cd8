"""CPU part of the EdgeConv kernel tests (``tests/test_edge_kernels_gpu.py``): the float64 oracle is
checked against the layer, the ``p_i + q_j`` form the kernels compute - forward AND the hand-written
backward - is checked against the oracle and its autograd, named mutants of that form are shown to
lie far outside the GPU test's bound, every case of the GPU table is checked to still reach the
branch it names, and the kink margin the GPU verdicts rest on is asserted."""
import copy

import pytest
import torch

import test_edge_kernels_gpu as S
from gnnqc.ops import gcn as G

HIP_CASES = [c.name for c in S.CASES if "hip" in c.tags]
F32_ULP = 2.0 ** -23


def pq_form(c, d, self_loop=False, mean_by_n=False, act_after_sum=False, wa_for_p=False, transposed_is_mask=False,
            alpha_below_zero_only=False):
    """The kernels' math (``csrc/kernels/edge.hip``) in float64, written out: ``z_ij = p_i + q_j``
    with ``p = x (Wa - Wb) + b`` and ``q = x Wb``, the per-edge activation, the neighbour sum or
    mean, the node pool weights and the concat; then the backward by hand (``e_ij``, ``dp``, ``dq``
    over the transposed neighbour sets, the parameter gradients and ``dx``). Returns
    ``(out [B, T, Fo], grads)``. The keyword arguments switch on the named mutants."""
    dt = torch.float64
    L = d["layer"]
    x, adj, mask = d["x"].to(dt), d["adj"].to(dt), d["mask"].to(dt)
    W, b = L.out.kernel.detach().to(dt), L.out.bias.detach().to(dt)
    al = L.prelu_alpha.detach().to(dt) if L.prelu_alpha is not None else None
    B, T, N, Cin = x.shape
    Wa, Wb = W[:Cin], W[Cin:]
    Wd = Wa if wa_for_p else Wa - Wb
    p, q = x @ Wd + b, x @ Wb                                               # [B, T, N, C]
    nb = adj > 0                                                            # [B, i, j]
    if self_loop:
        nb = nb | ((torch.eye(N, dtype=dt) * mask[:, :, None]) > 0)
    nbf = nb.to(dt)[:, None, :, :, None]
    z = p[:, :, :, None, :] + q[:, :, None, :, :]                           # [B, T, i, j, C]

    def act(v):
        if L.activation == "prelu":
            return torch.where(v > 0, v, al * v)
        return torch.relu(v) if L.activation == "relu" else v

    def act_grad(v):
        if L.activation == "prelu":
            return torch.where((v >= 0) if alpha_below_zero_only else (v > 0), torch.ones_like(v), al.expand_as(v))
        return (v > 0).to(dt) if L.activation == "relu" else torch.ones_like(v)

    o = act((z * nbf).sum(3)) if act_after_sum else (act(z) * nbf).sum(3)   # [B, T, N, C]
    deg = torch.full((B, N), float(N), dtype=dt) if mean_by_n else nb.sum(-1).to(dt).clamp(min=1)
    k = G.gat_pool_weights(mask, d["anom_pos"], c.pooling) * (1 / deg if L.aggregate == "mean" else 1.0)
    pooled = torch.einsum("bi,btic->btc", k, o)
    out = pooled if d["anom"] is None else torch.cat([d["anom"].to(dt), pooled], -1)
    # ---- backward
    Ca = 0 if d["anom"] is None else Cin
    g = d["g"].to(dt)
    g = g[:, :B, :Ca + W.shape[1]].transpose(0, 1) if c.tm else g
    gi = k[:, None, :, None] * g[..., Ca:][:, :, None, :]                   # [B, T, N, C]
    dz = act_grad(z) * gi[:, :, :, None, :]
    e = dz * nbf
    dp = e.sum(3)
    dq = (dz * nbf.transpose(2, 3)).sum(2) if transposed_is_mask else e.sum(2)
    dWd = torch.einsum("btif,btic->fc", x, dp)
    grads = {"x": dp @ Wd.T + dq @ Wb.T, "W": torch.cat([dWd, torch.einsum("btif,btic->fc", x, dq) - dWd]),
             "bias": dp.sum((0, 1, 2))}
    if Ca:
        grads["anom"] = g[..., :Ca].clone()
    if al is not None:
        below = (z < 0) if alpha_below_zero_only else (z <= 0)
        grads["alpha"] = (torch.where(below, z, torch.zeros_like(z)) * gi[:, :, :, None, :] * nbf).sum((0, 1, 2, 3))
    return out, grads


def preactivations(d):
    """float64 pre-activations of every Dense of the layer on the neighbour edges of valid nodes:
    [edges, width] per Dense, the output layer's ``z_ij`` last."""
    L = copy.deepcopy(d["layer"]).double()
    x, adj, mask = d["x"].double(), d["adj"].double(), d["mask"].double()
    B, T, N, Fd = x.shape
    sel = ((adj > 0) & (mask[:, :, None] > 0))[:, None].expand(B, T, N, N)
    m = torch.cat([x[:, :, :, None, :].expand(B, T, N, N, Fd),
                   x[:, :, None, :, :] - x[:, :, :, None, :]], -1)[sel]
    pre = []
    with torch.no_grad():
        for dense in list(L.hidden) + [L.out]:
            pre.append(m @ dense.kernel + dense.bias)
            m = torch.relu(pre[-1])
    return pre


@pytest.mark.parametrize("name", [c.name for c in S.CASES])
def test_oracle_is_the_layer_plus_pool_plus_cat(name):
    """edge_pool_eager in float64 == EdgeConv + pool_nodes + cat, written out here; its time-major
    layout is the padded transpose."""
    c, d, (out64, _), _ = S.reference(name)
    layer = copy.deepcopy(d["layer"]).double()
    x, adj, mask = d["x"].double(), d["adj"].double(), d["mask"].double()
    with torch.no_grad():
        pooled = G.pool_nodes(layer(x, adj, mask), mask, d["anom_pos"], c.pooling)
        want = pooled if d["anom"] is None else torch.cat([d["anom"].double(), pooled], -1)
        assert torch.equal(out64, want)
        tm, Bret = G.edge_pool_eager(x, adj, mask, None if d["anom"] is None else d["anom"].double(),
                                     d["anom_pos"], layer, c.pooling, time_major=True)
    Mp, Cp = S.time_major_pad(c)
    Fo = want.shape[-1]
    assert Bret == c.B and tuple(tm.shape) == (c.T, Mp, Cp)
    assert torch.equal(tm[:, :c.B, :Fo].transpose(0, 1), want)
    assert torch.count_nonzero(tm[:, c.B:]) == 0 and torch.count_nonzero(tm[:, :, Fo:]) == 0


@pytest.mark.parametrize("name", HIP_CASES)
def test_pq_form_is_the_oracle(name):
    """The kernels' forward and hand-written backward equal the layer and its autograd in float64 on
    every HIP case of the GPU table."""
    c, d, (out64, g64), _ = S.reference(name)
    out, grads = pq_form(c, d)
    tol = 1e-12 * max(1.0, c.xscale) ** 2
    assert (out - out64).abs().max().item() < tol * (1.0 + out64.abs().max().item())
    assert set(grads) == set(g64)
    for k, ref in g64.items():
        assert grads[k].shape == ref.shape, k
        assert (grads[k] - ref).abs().max().item() < tol * (1.0 + ref.abs().max().item()), k


def _dispatch(**want):
    return [c.name for c in S.CASES if c.name.startswith("dispatch_") and all(getattr(c, k) == v for k, v in want.items())]


FORWARD_MUTANTS = {
    # mutant -> (keyword arguments of pq_form, the cases meant to catch it)
    "self loop added": (dict(self_loop=True), _dispatch() + ["nodes_1", "degenerate_selection"]),
    "mean divides by N": (dict(mean_by_n=True), _dispatch(agg="mean") + ["nodes_7", "degenerate_mean"]),
    "activation after the sum": (dict(act_after_sum=True), _dispatch() + ["act_relu", "nodes_64"]),
    "Wa used for p_i": (dict(wa_for_p=True), _dispatch() + ["act_linear", "x30"]),
}
BACKWARD_MUTANTS = {
    # mutant -> (keyword arguments, the cases meant to catch it, the gradients it must move)
    "transposed mask = mask": (dict(transposed_is_mask=True), _dispatch() + ["degenerate_sum", "nodes_33"],
                               ("x", "W")),
    "alpha branch at z < 0 only": (dict(alpha_below_zero_only=True), ["kink_zeros"], ("x", "bias")),
}


@pytest.mark.parametrize("mutant,name", [(m, n) for m, (_, names) in FORWARD_MUTANTS.items() for n in names])
def test_forward_mutant_is_far_outside_the_bound(mutant, name):
    """Each named mutant of the kernel's forward is at least 5 of the GPU test's output bounds away
    from the oracle on the cases meant to catch it."""
    c, d, (out64, _), e32 = S.reference(name)
    got, _ = pq_form(c, d, **FORWARD_MUTANTS[mutant][0])
    assert S.out_excess(got, out64, e32["out"]) >= 5.0, S.out_excess(got, out64, e32["out"])


@pytest.mark.parametrize("mutant,name", [(m, n) for m, (_, names, _) in BACKWARD_MUTANTS.items() for n in names])
def test_backward_mutant_is_far_outside_the_bound(mutant, name):
    """Each named mutant of the kernel's backward moves the gradients it is named for by at least 5
    of the GPU test's gradient bounds, and leaves the forward alone."""
    c, d, (out64, g64), e32 = S.reference(name)
    kw, _, moved = BACKWARD_MUTANTS[mutant]
    out, grads = pq_form(c, d, **kw)
    assert S.out_excess(out, out64, e32["out"]) <= 1.0
    for k in moved:
        far = (grads[k] - g64[k]).abs().max().item() / S.grad_bound(g64[k], e32[k])
        assert far >= 5.0, (k, far)


def test_alpha_branch_mutant_is_invisible_without_exact_zeros():
    """...and that mutant needs the constructed case: on a case that honours the kink condition no
    z_ij is zero and the two branch rules agree."""
    c, d, (_, g64), e32 = S.reference("dispatch_c2f16_sum_mean")
    _, grads = pq_form(c, d, alpha_below_zero_only=True)
    for k, ref in g64.items():
        assert (grads[k] - ref).abs().max().item() <= S.grad_bound(ref, e32[k]), k


@pytest.mark.parametrize("name", [c.name for c in S.CASES])
def test_kink_condition(name):
    """No pre-activation of a neighbour edge lies within 64 float32 ulps of the case's max |z| of
    zero (ReLU / PReLU per edge make the gradients discontinuous there: a float32 sign flip, not a
    kernel bug, would decide the GPU verdict). ``kink_zeros`` holds exact zeros by construction; its
    other pre-activations honour the margin."""
    c, d, _, _ = S.reference(name)
    for z in preactivations(d):
        if z.numel() == 0:
            continue
        az = z.abs()
        thr = 64 * F32_ULP * az.max().item()
        if c.kind == "zeros":
            assert (az == 0).any(), "the case built for exact zeros has none"
            az = az[az > 0]
        assert az.min().item() >= thr > 0, (az.min().item(), thr)
        # (the lattice: z is the same float32 number in every evaluation order)
        assert torch.equal(z.float().double(), z)


def test_degenerate_builder():
    c, d, (out64, g64), _ = S.reference("degenerate_mean")
    m, adj = d["mask"], d["adj"]
    assert m[0].sum() == 0 and d["anom_pos"][0] == -1 and m[1].sum() == 1
    assert m[2, 3] == 1 and adj[2, 3].sum() == 0 and adj[2, :, 3].sum() == 0 and d["anom_pos"][2] == 3
    assert (d["x"][(m == 0)[:, None, :].expand(c.B, c.T, c.N)] == 123.0).all()
    assert torch.count_nonzero(out64[0, :, c.Cin:]) == 0                  # nothing valid: the pooled row is zero
    assert torch.count_nonzero(g64["x"][0]) == 0
    assert m[3, 0] == 1 and m[3, 2] == 0 and adj[3, 0, 2] == 1            # an edge towards a masked node ...
    assert g64["x"][3, :, 2].abs().max() > 0                              # ... which the layer follows
    assert not torch.equal(adj, adj.transpose(1, 2))                      # asymmetric
    # the diagonal is in the data for every other sample only (no self loop is added)
    d2 = S.reference("dispatch_c2f16_sum_mean")[1]
    diag = torch.diagonal(d2["adj"], dim1=1, dim2=2)
    assert torch.equal(diag[0], d2["mask"][0]) and diag[1].sum() == 0
    z = S.reference("kink_zeros")[1]
    assert torch.count_nonzero(z["x"][0]) == 0 and torch.count_nonzero(z["layer"].out.bias) == 0
    assert z["mask"][0].sum() >= 2 and (z["adj"][0].sum(-1) * z["mask"][0]).max() > 0


@pytest.mark.parametrize("case", S.CASES, ids=[c.name for c in S.CASES])
def test_case_reaches_its_branches(case, monkeypatch):
    """Tags are recomputed from the shapes; edge_pool_hip_ok (with the device test forced on) agrees
    with the table on which cases take the HIP path."""
    assert case.tags, case.name
    for tag in case.tags:
        assert S.PREDICATES[tag](case), f"{case.name} no longer reaches '{tag}'"
    assert ("hip" in case.tags) != ("eager" in case.tags)
    import gnnqc.ops as ops
    monkeypatch.setattr(ops, "use_hip", lambda t: True)
    monkeypatch.delenv("GNNQC_EDGE_HIP", raising=False)
    d = S.reference(case.name)[1]
    assert G.edge_pool_hip_ok(d["x"], d["layer"], case.pooling) == ("hip" in case.tags)
    monkeypatch.setenv("GNNQC_EDGE_HIP", "0")
    assert not G.edge_pool_hip_ok(d["x"], d["layer"], case.pooling)
    assert case.B * case.T * case.N * case.N * max(case.C, *case.hidden, 1) * 8 < 64 << 20   # the oracle's edge tensor


def test_hip_gate_conditions(monkeypatch):
    """Each condition of edge_pool_hip_ok on its own: a CPU tensor, a float64 tensor, N = 65,
    Cin = 5, an uninstantiated width, hidden MLP layers, aggregate = max, pooling = max, an
    activation the kernels lack, the environment switch; time_major off the HIP path raises."""
    import gnnqc.ops as ops
    from gnnqc.models.graphconv import EdgeConv
    x = torch.zeros(2, 3, 64, 2)
    ok = EdgeConv(2, 16, None, "relu", "sum", "prelu")
    assert not G.edge_pool_hip_ok(x, ok, "mean")                           # not on a GPU
    monkeypatch.setattr(ops, "use_hip", lambda t: True)
    monkeypatch.delenv("GNNQC_EDGE_HIP", raising=False)
    for pooling in ("mean", "sum", "selection"):
        assert G.edge_pool_hip_ok(x, ok, pooling)
    assert G.edge_pool_hip_ok(x, EdgeConv(2, 16, None, "relu", "mean", "relu"), "mean")
    assert G.edge_pool_hip_ok(x, EdgeConv(2, 16, [], "relu", "mean", None), "mean")
    assert not G.edge_pool_hip_ok(x.double(), ok, "mean")
    assert not G.edge_pool_hip_ok(x[0], ok, "mean")
    assert not G.edge_pool_hip_ok(torch.zeros(2, 3, 65, 2), ok, "mean")
    assert not G.edge_pool_hip_ok(torch.zeros(2, 3, 9, 5), EdgeConv(5, 16, None, "relu", "sum", "prelu"), "mean")
    assert not G.edge_pool_hip_ok(torch.zeros(2, 3, 9, 3), ok, "mean")     # W is not [2 Cin, C]
    assert not G.edge_pool_hip_ok(x, EdgeConv(2, 12, None, "relu", "sum", "prelu"), "mean")
    assert not G.edge_pool_hip_ok(x, EdgeConv(2, 16, [16], "relu", "sum", "prelu"), "mean")
    assert not G.edge_pool_hip_ok(x, EdgeConv(2, 16, None, "relu", "max", "prelu"), "mean")
    assert not G.edge_pool_hip_ok(x, ok, "max")
    assert not G.edge_pool_hip_ok(x, EdgeConv(2, 16, None, "relu", "sum", "tanh"), "mean")
    with pytest.raises(ValueError):
        G.edge_pool(x, torch.zeros(2, 64, 64), torch.ones(2, 64), None, None,
                    EdgeConv(2, 16, None, "relu", "max", "prelu"), "mean", time_major=True)
    monkeypatch.setenv("GNNQC_EDGE_HIP", "0")
    assert not G.edge_pool_hip_ok(x, ok, "mean")


def test_fallback_layers_keep_the_eager_route():
    """Out of the fused EdgeConv route's scope, and so still on the eager layer: the network-wide
    SoilNet layout, ``mlp_hidden`` not null, ``aggregation_type: max``, AGNNConv and GatedGraphConv."""
    from gnnqc import config as C
    from gnnqc.models import GCNClassifier
    from gnnqc.models.graphconv import AGNNConv, EdgeConv, GatedGraphConv
    pc = C.normalize_preproc(C.default("preprocessing_cml"))
    x = torch.zeros(2, 181, 5, 2)
    inputs = (x, torch.zeros(2, 181, 2), torch.zeros(2, 5, 5), torch.ones(2, 5), torch.zeros(2, dtype=torch.long))

    def model(**gc):
        mc = C.default("model_cml")
        mc["graph_convolution"].update(gc)
        return GCNClassifier(mc, pc)

    for gc, cls in ((dict(layer="EdgeConv", mlp_hidden=[16]), EdgeConv),
                    (dict(layer="EdgeConv", aggregation_type="max"), EdgeConv),
                    (dict(layer="AGNNConv"), AGNNConv), (dict(layer="GatedGraphConv"), GatedGraphConv)):
        m = model(**gc)
        assert isinstance(m.gcn_layer, cls)
        assert not m._cml_edge_time_major(inputs) and not m._cml_gat_time_major(inputs) and not m._fused_ok()
    m = model(layer="EdgeConv")
    assert isinstance(m.gcn_layer, EdgeConv) and not m.gcn_layer.hidden       # the config default: mlp_hidden null
    assert not m._cml_edge_time_major(inputs)                                # (CPU tensors)
    m.per_sensor = False
    assert not m._cml_edge_time_major(inputs)                                # network-wide layout


def test_case_table_covers_the_issue():
    names = {c.name for c in S.CASES}
    assert len(names) == len(S.CASES)
    assert {t for c in S.CASES for t in c.tags} == set(S.PREDICATES)
    hip = [c for c in S.CASES if "hip" in c.tags]
    disp = [c for c in hip if c.name.startswith("dispatch_")]
    assert {(c.Cin, c.C) for c in disp} == {(a, b) for a in (1, 2, 3, 4) for b in (8, 16, 32)}
    assert {c.agg for c in disp} == {"sum", "mean"} and {c.pooling for c in disp} == {"mean", "selection"}
    assert {(c.agg, c.pooling) for c in disp} == {(a, p) for a in ("sum", "mean") for p in ("mean", "selection")}
    assert {c.N for c in hip} >= {1, 7, 33, 64} and {c.pooling for c in hip} == {"mean", "sum", "selection"}
    assert any((c.B, c.T, c.N) == (3, 7, 5) for c in hip)
    assert {c.tm for c in hip if (c.B, c.T, c.N) == (48, 181, 7)} == {True, False}
    assert {c.B for c in hip if c.tm} >= {5, 16, 17} and any(not c.anom for c in hip)
    assert {c.act for c in hip} == {"prelu", "relu", None} and any(not c.training for c in hip)
    assert any(c.xscale == 30 for c in hip) and any(c.kind == "zeros" for c in hip)
    assert {c.kind for c in hip if c.kind == "degenerate"} and {c.pooling for c in hip if c.kind == "degenerate"} == \
        {"mean", "sum", "selection"}
    eager = [c for c in S.CASES if "eager" in c.tags]
    assert {c.N for c in eager} >= {65} and any(c.agg == "max" for c in eager) and any(c.hidden == (16,) for c in eager)
