"""CPU part of the AGNNConv kernel tests (``tests/test_agnn_kernels_gpu.py``): the float64 oracle is
checked against the layer, the per-node walk over neighbour words the kernels compute - forward AND
the hand-written backward - is checked against the oracle and its autograd, named mutants of that
walk are shown to lie far outside the GPU test's bound, every case of the GPU table is checked to
still reach the branch it names, and the kink margin the GPU verdicts rest on is asserted."""
import copy

import pytest
import torch

import test_agnn_kernels_gpu as S
from gnnqc.ops import gcn as G

HIP_CASES = [c.name for c in S.CASES if "hip" in c.tags]
F32_ULP = 2.0 ** -23


def _bits(w):
    out = []
    while w:
        low = w & -w
        out.append(low.bit_length() - 1)
        w ^= low
    return out


def adj_words(nb):
    """The neighbour words as ``edge_adj_bits`` builds them, from the boolean ``adj > 0`` [B, N, N]:
    ``word[b][i]`` bit j: j is a neighbour of i; ``wordT[b][i]`` bit j: i is a neighbour of j."""
    rows, cols = nb.tolist(), nb.transpose(1, 2).tolist()
    pack = lambda r: sum(1 << j for j, v in enumerate(r) if v)   # noqa: E731
    return [[pack(r) for r in s] for s in rows], [[pack(r) for r in s] for s in cols]


def walk_form(c, d, self_loop=False, raw_scores=False, beta_after_softmax=False, aggregates_xn=False,
              mean_by_valid=False, transposed_is_word=False, alpha_below_zero_only=False, mask_in_word=False):
    """The kernels' math (``csrc/kernels/agnn.hip``) in float64, written out: every node walks the
    set bits of its neighbour word twice (row maximum, then normaliser and aggregate), the activation,
    the node pool weights and the concat; then the backward by hand: phase 1 keeps every node's
    (max, normaliser, u, <u, r>), phase 2 gathers ``dx`` and ``dxn`` over the node's own word and its
    transposed word and goes through the normalisation; ``dbeta`` and ``dalpha`` are summed on the
    way. Returns ``(out [B, T, Fo], grads, aux)``. The keyword arguments switch on the named mutants."""
    dt = torch.float64
    L = d["layer"]
    x, mask = d["x"].to(dt), d["mask"].to(dt)
    beta = float(L.beta.detach())
    al = L.prelu_alpha.detach().to(dt) if L.prelu_alpha is not None else None
    B, T, N, Cin = x.shape
    nb = d["adj"] > 0
    if self_loop:
        nb = nb | (torch.eye(N, dtype=torch.bool) & (mask[:, :, None] > 0))
    if mask_in_word:
        nb = nb & (mask[:, None, :] > 0)
    word, wordT = adj_words(nb)
    if transposed_is_word:
        wordT = word
    nrm = x.norm(dim=-1)
    xn = x / nrm.clamp(min=S.K_EPS)[..., None]
    sv = x if raw_scores else xn                                           # the vectors the scores are made of
    av = xn if aggregates_xn else x                                        # the vectors that are aggregated
    pw = G.gat_pool_weights(mask, d["anom_pos"], c.pooling)
    sd = torch.ones(B, N, dtype=dt)
    if L.aggregate == "mean":
        for b in range(B):
            for i in range(N):
                sd[b, i] = 1.0 / max(int(mask[b].sum()) if mean_by_valid else bin(word[b][i]).count("1"), 1)

    def act(v):
        if L.activation == "prelu":
            return torch.where(v > 0, v, al * v)
        return torch.relu(v) if L.activation == "relu" else v

    def act_grad(v):
        if L.activation == "prelu":
            return torch.where((v >= 0) if alpha_below_zero_only else (v > 0), torch.ones_like(v), al.expand_as(v))
        return (v > 0).to(dt) if L.activation == "relu" else torch.ones_like(v)

    def scores(b, i, js):                                                  # [T, len(js)]: <., .> and the score
        cos = (sv[b, :, i, None, :] * sv[b][:, js, :]).sum(-1)
        return cos, (cos if beta_after_softmax else beta * cos)

    # ---- forward: two walks per node
    m = torch.zeros(B, T, N, dtype=dt)
    l = torch.zeros(B, T, N, dtype=dt)
    r = torch.zeros(B, T, N, Cin, dtype=dt)
    for b in range(B):
        for i in range(N):
            js = _bits(word[b][i])
            if not js:
                continue
            _, s = scores(b, i, js)
            m[b, :, i] = s.amax(-1)
            e = torch.exp(s - m[b, :, i, None])
            l[b, :, i] = e.sum(-1)
            r[b, :, i] = (e[..., None] * av[b][:, js, :]).sum(1) / l[b, :, i, None]
    if beta_after_softmax:
        r = beta * r
    o = r * sd[:, None, :, None]
    pooled = torch.einsum("bi,btic->btc", pw, act(o))
    out = pooled if d["anom"] is None else torch.cat([d["anom"].to(dt), pooled], -1)
    # ---- backward, phase 1: u_i and <u_i, r_i>; dalpha; dbeta over the node's own word
    Ca = 0 if d["anom"] is None else Cin
    g = d["g"].to(dt)
    g = g[:, :B, :Ca + Cin].transpose(0, 1) if c.tm else g
    gl = g[..., Ca:][:, :, None, :]                                        # [B, T, 1, Cin]
    u = act_grad(o) * (pw * sd)[:, None, :, None] * gl
    cu = (u * r).sum(-1)
    grads = {}
    if Ca:
        grads["anom"] = g[..., :Ca].clone()
    if al is not None:
        below = (o < 0) if alpha_below_zero_only else (o <= 0)
        grads["alpha"] = (torch.where(below, o, torch.zeros_like(o)) * pw[:, None, :, None] * gl).sum((0, 1, 2))
    dbeta = torch.zeros((), dtype=dt)
    mass = 0.0
    dx = torch.zeros_like(x)
    dxn = torch.zeros_like(x)
    for b in range(B):
        for i in range(N):
            js = _bits(word[b][i])
            if not js or pw[b, i] == 0:
                continue
            cos, s = scores(b, i, js)
            att = torch.exp(s - m[b, :, i, None]) / l[b, :, i, None]
            ds = att * ((u[b, :, i, None, :] * x[b][:, js, :]).sum(-1) - cu[b, :, i, None])
            dbeta = dbeta + (ds * cos).sum()
            mass += (ds * cos).abs().sum().item()
            dxn[b, :, i] += (ds[..., None] * xn[b][:, js, :]).sum(1)
    # ---- phase 2: the gather over the transposed word
    for b in range(B):
        for k in range(N):
            src = [i for i in _bits(wordT[b][k]) if pw[b, i] != 0 and word[b][i]]
            if not src:
                continue
            cos = (sv[b][:, src, :] * sv[b, :, k, None, :]).sum(-1)        # [T, len(src)]
            s = cos if beta_after_softmax else beta * cos
            att = torch.exp(s - m[b][:, src]) / l[b][:, src]
            us = u[b][:, src, :]
            dx[b, :, k] += (att[..., None] * us).sum(1)
            ds = att * ((us * x[b, :, k, None, :]).sum(-1) - cu[b][:, src])
            dxn[b, :, k] += (ds[..., None] * xn[b][:, src, :]).sum(1)
    dxn = beta * dxn
    big = (nrm >= S.K_EPS)[..., None]
    through = (dxn - xn * (xn * dxn).sum(-1, keepdim=True)) / nrm.clamp(min=S.K_EPS)[..., None]
    grads["x"] = dx + torch.where(big, through, dxn / S.K_EPS)
    grads["beta"] = dbeta.reshape(1) if L.beta.requires_grad else torch.zeros(0, dtype=dt)
    deg = torch.tensor([[bin(w).count("1") for w in ws] for ws in word])
    return out, S.split_dx(d, grads), dict(o=o, deg=deg, mass=mass)


def farthest(c, grads_out, ref):
    """max over the compared quantities of |got - ref| / bound for a (mutant) result."""
    (out, grads), (out64, g64), e32, mass = grads_out, ref[2], ref[3], ref[4]
    far = {"out": S.out_excess(out, out64, e32["out"])}
    for k, r in g64.items():
        if r.numel():
            err, bound = (grads[k] - r).abs().max().item(), S.grad_bound(k, r, e32[k], mass)
            far[k] = err / bound if bound > 0 else (float("inf") if err > 0 else 0.0)
    return far


@pytest.mark.parametrize("name", [c.name for c in S.CASES])
def test_oracle_is_the_layer_plus_pool_plus_cat(name):
    """agnn_pool_eager in float64 == AGNNConv + pool_nodes + cat, written out here; its time-major
    layout is the padded transpose."""
    c, d, (out64, _), _, _ = S.reference(name)
    layer = copy.deepcopy(d["layer"]).double()
    x, adj, mask = d["x"].double(), d["adj"].double(), d["mask"].double()
    with torch.no_grad():
        pooled = G.pool_nodes(layer(x, adj, mask), mask, d["anom_pos"], c.pooling)
        want = pooled if d["anom"] is None else torch.cat([d["anom"].double(), pooled], -1)
        assert torch.equal(out64, want)
        tm, Bret = G.agnn_pool_eager(x, adj, mask, None if d["anom"] is None else d["anom"].double(),
                                     d["anom_pos"], layer, c.pooling, time_major=True)
    Mp, Cp = S.time_major_pad(c)
    Fo = want.shape[-1]
    assert Bret == c.B and tuple(tm.shape) == (c.T, Mp, Cp)
    assert torch.equal(tm[:, :c.B, :Fo].transpose(0, 1), want)
    assert torch.count_nonzero(tm[:, c.B:]) == 0 and torch.count_nonzero(tm[:, :, Fo:]) == 0


@pytest.mark.parametrize("name", HIP_CASES)
def test_walk_form_is_the_oracle(name):
    """The kernels' forward and hand-written backward equal the layer and its autograd in float64
    within 1e-10 relative on every HIP case of the GPU table, and the mass of dbeta's summands is the
    one the GPU test's bound uses."""
    c, d, (out64, g64), _, mass = S.reference(name)
    out, grads, aux = walk_form(c, d)
    tol = 1e-10
    assert (out - out64).abs().max().item() <= tol * (1.0 + out64.abs().max().item())
    assert set(grads) == set(g64)
    for k, ref in g64.items():
        assert grads[k].shape == ref.shape, k
        if k == "beta" and ref.numel():
            assert (grads[k] - ref).abs().max().item() <= tol * (1.0 + ref.abs().max().item() + mass), k
        elif ref.numel():
            assert (grads[k] - ref).abs().max().item() <= tol * (1.0 + ref.abs().max().item()), k
    assert abs(aux["mass"] - mass) <= 1e-9 * (1.0 + mass)


def _inst(**want):
    return [c.name for c in S.CASES if c.name.startswith("inst_") and all(getattr(c, k) == v for k, v in want.items())]


MUTANTS = {
    # mutant -> (keyword arguments of walk_form, the cases meant to catch it, the quantities that
    # may show it - None: any compared quantity)
    "self loop added": (dict(self_loop=True), _inst() + ["nodes_1", "nodes_7", "degenerate_selection"], None),
    "scores from un-normalised x": (dict(raw_scores=True), _inst(Cin=2) + _inst(Cin=4) + ["act_linear", "beta_30"],
                                    None),
    "beta applied after the softmax": (dict(beta_after_softmax=True), _inst() + ["beta_neg3", "beta_30", "nodes_64"],
                                       None),
    "aggregates xn instead of x": (dict(aggregates_xn=True), _inst() + ["act_linear", "nodes_64", "zero_norm"], None),
    "mean divides by the valid-node count": (dict(mean_by_valid=True), _inst(agg="mean") + ["nodes_7",
                                                                                            "degenerate_mean"], None),
    "transposed word = word": (dict(transposed_is_word=True), _inst() + ["degenerate_sum", "nodes_33"], ("x",)),
    "alpha branch at o < 0 only": (dict(alpha_below_zero_only=True), ["zeros"], ("x", "x0")),
    "mask folded into the neighbour word": (dict(mask_in_word=True), ["degenerate_mean", "degenerate_sum",
                                                                      "degenerate_selection"], None),
}


@pytest.mark.parametrize("mutant,name", [(m, n) for m, (_, names, _) in MUTANTS.items() for n in names])
def test_mutant_is_far_outside_the_bound(mutant, name):
    """Each named mutant of the kernel's math is at least 5 of the GPU test's bounds away from the
    oracle in at least one compared quantity of every case meant to catch it."""
    ref = S.reference(name)
    kw, _, where = MUTANTS[mutant]
    out, grads, _ = walk_form(ref[0], ref[1], **kw)
    far = farthest(ref[0], (out, grads), ref)
    if where is not None:
        far = {k: v for k, v in far.items() if k in where}
    assert far and max(far.values()) >= 5.0, far


def test_mutant_table_leaves_the_dense_sum_case_alone():
    """The dense N = 64 sum case is not tagged for the two mutants a probe found only marginally
    visible there."""
    for m in ("self loop added", "transposed word = word"):
        assert "nodes_64" not in MUTANTS[m][1]
    assert set(MUTANTS) == {"self loop added", "scores from un-normalised x", "beta applied after the softmax",
                            "aggregates xn instead of x", "mean divides by the valid-node count",
                            "transposed word = word", "alpha branch at o < 0 only",
                            "mask folded into the neighbour word"}
    assert all(S.reference(n)[0].agg == "mean" for n in MUTANTS["mean divides by the valid-node count"][1])


def test_alpha_branch_mutant_is_invisible_without_exact_zeros():
    """...and that mutant needs the constructed case: on a case that honours the kink condition no
    o_ic is zero and the two branch rules agree."""
    ref = S.reference("inst_c2_sum_mean")
    out, grads, _ = walk_form(ref[0], ref[1], alpha_below_zero_only=True)
    assert max(farthest(ref[0], (out, grads), ref).values()) <= 1.0


@pytest.mark.parametrize("name", [c.name for c in S.CASES if "hip" in c.tags and c.act in ("prelu", "relu")])
def test_kink_condition(name):
    """For every PReLU / ReLU case the activation's argument of a valid node with a neighbour is at
    least 64 float32 ulps of the case's max |o| away from zero (the gradients are discontinuous there:
    a float32 sign flip, not a kernel bug, would decide the GPU verdict). ``zeros`` holds exact zeros
    by construction; its other values honour the margin."""
    c, d, _, _, _ = S.reference(name)
    assert c.xkind == "sign"
    aux = walk_form(c, d)[2]
    sel = ((d["mask"] > 0) & (aux["deg"] > 0))[:, None, :, None].expand_as(aux["o"])
    ao = aux["o"][sel].abs()
    if ao.numel() == 0:
        assert c.N == 1
        return
    thr = 64 * F32_ULP * ao.max().item()
    if c.kind == "zeros":
        assert (ao == 0).any(), "the case built for exact zeros has none"
        ao = ao[ao > 0]
    assert ao.min().item() >= thr > 0, (ao.min().item(), thr)
    if c.kind != "degenerate":                  # (one sign per row: the structural floor of the module docstring)
        assert ao.min().item() >= 0.25 / 64
    signs = torch.sign(aux["o"][sel])
    assert (signs > 0).any() and (signs < 0).any(), "both branches of the activation"


def test_free_sign_cases_are_linear():
    for c in S.CASES:
        if "hip" in c.tags and c.xkind == "free":
            assert c.act in (None, "linear"), c.name
    cos_neg = False
    for name in ("beta_neg3", "act_linear"):
        d = S.reference(name)[1]
        xn = torch.nn.functional.normalize(d["x"].double(), dim=-1)
        cos = torch.einsum("btif,btjf->btij", xn, xn)[(d["adj"] > 0)[:, None].expand(-1, d["x"].shape[1], -1, -1)]
        cos_neg = cos_neg or bool((cos < -0.5).any())
    assert cos_neg


def test_builders():
    c, d, (out64, g64), _, _ = S.reference("degenerate_mean")
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
    d2 = S.reference("inst_c2_sum_mean")[1]
    diag = torch.diagonal(d2["adj"], dim1=1, dim2=2)
    assert torch.equal(diag[0], d2["mask"][0]) and diag[1].sum() == 0
    z = S.reference("zeros")[1]
    assert torch.count_nonzero(z["x"][0]) == 0
    assert z["mask"][0].sum() >= 2 and (z["adj"][0].sum(-1) * z["mask"][0]).max() > 0
    _, zg, (_, g64z), _, _ = S.reference("zeros")
    assert torch.isfinite(g64z["x"]).all() and torch.isfinite(g64z["x0"]).all() and g64z["x0"].abs().max() > 0
    # zero_norm: one valid all-zero node with non-zero neighbours; its dx carries the 1 / 1e-12 factor
    cz, dz, (_, gz), _, _ = S.reference("zero_norm")
    zn = S.zero_norm_nodes(dz)
    assert dz["mask"][1, 0] == 1 and zn[1, :, 0].all() and not zn[1, :, 1:3].any()
    assert dz["adj"][1, 0, 1] == 1 and dz["adj"][1, 1, 0] == 1
    assert gz["x0"][1, :, 0].abs().max() > 1e6 * gz["x"].abs().max() > 0
    assert torch.count_nonzero(gz["x"][1, :, 0]) == 0 and torch.count_nonzero(gz["x0"][1, :, 1:3]) == 0
    # a frozen beta: no gradient in the oracle either
    assert S.reference("beta_frozen")[2][1]["beta"].numel() == 0
    assert not S.reference("beta_frozen")[1]["layer"].beta.requires_grad


@pytest.mark.parametrize("case", S.CASES, ids=[c.name for c in S.CASES])
def test_case_reaches_its_branches(case, monkeypatch):
    """Tags are recomputed from the shapes; agnn_pool_hip_ok (with the device test forced on) agrees
    with the table on which cases take the HIP path."""
    assert case.tags, case.name
    for tag in case.tags:
        assert S.PREDICATES[tag](case), f"{case.name} no longer reaches '{tag}'"
    assert ("hip" in case.tags) != ("eager" in case.tags)
    import gnnqc.ops as ops
    monkeypatch.setattr(ops, "use_hip", lambda t: True)
    monkeypatch.delenv("GNNQC_AGNN_HIP", raising=False)
    d = S.reference(case.name)[1]
    assert G.agnn_pool_hip_ok(d["x"], d["layer"], case.pooling) == ("hip" in case.tags)
    monkeypatch.setenv("GNNQC_AGNN_HIP", "0")
    assert not G.agnn_pool_hip_ok(d["x"], d["layer"], case.pooling)
    assert case.B * case.T * case.N * case.N * 8 * 8 < 64 << 20             # the oracle's edge tensors


def test_hip_gate_conditions(monkeypatch):
    """Each condition of agnn_pool_hip_ok on its own: a CPU tensor, a float64 tensor, a 3-d tensor,
    N = 65, Cin = 5, a layer built for another width, aggregate = max, pooling = max, an activation
    the kernels lack, the environment switch; time_major off the HIP path raises."""
    import gnnqc.ops as ops
    from gnnqc.models.graphconv import AGNNConv
    x = torch.zeros(2, 3, 64, 2)
    ok = AGNNConv(2, "sum", "prelu")
    assert G.AGNN_MAX_NODES == 64
    assert not G.agnn_pool_hip_ok(x, ok, "mean")                           # not on a GPU
    monkeypatch.setattr(ops, "use_hip", lambda t: True)
    monkeypatch.delenv("GNNQC_AGNN_HIP", raising=False)
    for pooling in ("mean", "sum", "selection"):
        assert G.agnn_pool_hip_ok(x, ok, pooling)
    assert G.agnn_pool_hip_ok(x, AGNNConv(2, "mean", "relu"), "mean")
    assert G.agnn_pool_hip_ok(x, AGNNConv(2, "mean", None, trainable=False), "mean")
    assert G.agnn_pool_hip_ok(torch.zeros(2, 3, 1, 1), AGNNConv(1, "mean", "linear"), "mean")
    assert G.agnn_pool_hip_ok(torch.zeros(2, 3, 9, 4), AGNNConv(4, "sum", "prelu"), "mean")
    assert not G.agnn_pool_hip_ok(x.double(), ok, "mean")
    assert not G.agnn_pool_hip_ok(x[0], ok, "mean")
    assert not G.agnn_pool_hip_ok(torch.zeros(2, 3, 65, 2), ok, "mean")
    assert not G.agnn_pool_hip_ok(torch.zeros(2, 3, 0, 2), ok, "mean")
    assert not G.agnn_pool_hip_ok(torch.zeros(2, 3, 9, 5), AGNNConv(5, "sum", "prelu"), "mean")
    assert not G.agnn_pool_hip_ok(torch.zeros(2, 3, 9, 3), ok, "mean")     # the layer was built for Cin = 2
    assert not G.agnn_pool_hip_ok(x, AGNNConv(2, "max", "prelu"), "mean")
    assert not G.agnn_pool_hip_ok(x, ok, "max")
    assert not G.agnn_pool_hip_ok(x, AGNNConv(2, "sum", "tanh"), "mean")
    with pytest.raises(ValueError):
        G.agnn_pool(x, torch.zeros(2, 64, 64), torch.ones(2, 64), None, None, AGNNConv(2, "max", "prelu"), "mean",
                    time_major=True)
    monkeypatch.setenv("GNNQC_AGNN_HIP", "0")
    assert not G.agnn_pool_hip_ok(x, ok, "mean")


def test_make_graph_layer_honours_trainable():
    """``graph_convolution.trainable`` (default true, spektral's default) reaches AGNNConv."""
    from gnnqc import config as C
    from gnnqc.models.graphconv import AGNNConv, make_graph_layer
    gc = C.default("model_cml")["graph_convolution"]
    gc["layer"] = "AGNNConv"
    layer = make_graph_layer(gc, 2)
    assert isinstance(layer, AGNNConv) and layer.beta.requires_grad and layer.in_features == 2
    gc["trainable"] = False
    frozen = make_graph_layer(gc, 2)
    assert not frozen.beta.requires_grad and frozen.prelu_alpha.requires_grad
    gc["trainable"] = True
    assert make_graph_layer(gc, 2).beta.requires_grad


def test_routes_out_of_scope_stay_eager():
    """GatedGraphConv and the network-wide layout keep the eager route, and an AGNNConv model on CPU
    tensors does too (and computes what the layer + pool_nodes + cat compute)."""
    from gnnqc import config as C
    from gnnqc.models import GCNClassifier
    from gnnqc.models.graphconv import AGNNConv, GatedGraphConv
    pc = C.normalize_preproc(C.default("preprocessing_cml"))
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(2, 181, 5, 2, generator=gen)
    adj = (torch.rand(2, 5, 5, generator=gen) > 0.5).float()
    inputs = (x, torch.randn(2, 181, 2, generator=gen), adj, torch.ones(2, 5), torch.zeros(2, dtype=torch.long))

    def model(**gc):
        mc = C.default("model_cml")
        mc["graph_convolution"].update(gc)
        return GCNClassifier(mc, pc)

    m = model(layer="GatedGraphConv")
    assert isinstance(m.gcn_layer, GatedGraphConv)
    assert not m._cml_agnn_time_major(inputs) and not m._cml_edge_time_major(inputs)
    assert not m._cml_gat_time_major(inputs) and not m._fused_ok()
    m = model(layer="AGNNConv")
    assert isinstance(m.gcn_layer, AGNNConv)
    assert not m._cml_agnn_time_major(inputs)                                # (CPU tensors)
    assert not m._cml_edge_time_major(inputs) and not m._cml_gat_time_major(inputs) and not m._fused_ok()
    with torch.no_grad():
        want = torch.cat([inputs[1], G.pool_nodes(m.gcn_layer(x, adj, inputs[3]), inputs[3], inputs[4], "mean")], -1)
        assert torch.equal(m.temporal_input(inputs), want)
    m.per_sensor = False
    assert not m._cml_agnn_time_major(inputs)                                # network-wide layout


def test_case_table_covers_the_issue():
    names = {c.name for c in S.CASES}
    assert len(names) == len(S.CASES)
    assert {t for c in S.CASES for t in c.tags} == set(S.PREDICATES)
    hip = [c for c in S.CASES if "hip" in c.tags]
    inst = [c for c in hip if c.name.startswith("inst_")]
    assert {(c.Cin, c.agg, c.pooling) for c in inst} == {(a, g, p) for a in (1, 2, 3, 4) for g in ("sum", "mean")
                                                        for p in ("mean", "selection")}
    assert {c.N for c in hip} >= {1, 7, 33, 64} and {c.pooling for c in hip} == {"mean", "sum", "selection"}
    assert any(c.N == 64 and c.pooling == "selection" for c in hip)
    assert any((c.B, c.T, c.N) == (3, 7, 5) for c in hip)
    assert {c.tm for c in hip if (c.B, c.T, c.N) == (48, 181, 7)} == {True, False}
    tm = [c for c in hip if c.tm]
    assert {c.B for c in tm} >= {5, 16, 17} and {c.anom for c in tm} == {True, False}
    assert any(c.anom and c.Cin == 3 for c in tm) and any(c.anom and c.Cin == 2 for c in tm)
    assert {c.act for c in hip} == {"prelu", "relu", None} and any(not c.training for c in hip)
    assert {c.beta for c in hip} >= {30.0, -3.0, 0.0, 4.0} and any(not c.trainable for c in hip)
    assert {c.kind for c in hip} >= {"degenerate", "zeros", "zero_norm"}
    assert {c.pooling for c in hip if c.kind == "degenerate"} == {"mean", "sum", "selection"}
    eager = [c for c in S.CASES if "eager" in c.tags]
    assert any(c.N == 65 for c in eager) and any(c.agg == "max" for c in eager)
    assert any(c.pooling == "max" for c in eager) and any(c.act == "tanh" for c in eager)
