"""CPU part of the GatedGraphConv kernel tests (``tests/test_gated_kernels_gpu.py``): the float64
oracle is checked against the layer, the per-node walk over neighbour words the kernels compute -
forward, with the layer-0 shortcut, AND the closed-form backward with its transposed-word gather - is
checked against the oracle and its autograd, named mutants of that walk are shown to lie far outside
the GPU test's bound, every case of the GPU table is checked to still reach the branch it names, and
the cap on the zeroed kink entries is asserted."""
import copy

import pytest
import torch

import test_gated_kernels_gpu as S
from gnnqc.ops import gcn as G

HIP_CASES = [c.name for c in S.CASES if "hip" in c.tags]


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


def _gather(words, v):
    """out[b, :, i] = sum of v[b, :, j] over the set bits j of words[b][i]."""
    out = torch.zeros_like(v)
    for b, ws in enumerate(words):
        for i, w in enumerate(ws):
            js = _bits(w)
            if js:
                out[b, :, i] = v[b][:, js].sum(1)
    return out


def walk_form(c, d, gates_rzh=False, reset_before=False, no_recurrent_bias=False, self_loop=False,
              adj_transposed=False, dp_over_row_word=False, pad_left=False):
    """The kernels' math (``csrc/kernels/gated.hip``) in float64, written out: layer 0 multiplies
    only the Cin rows of ``W_0`` and ``R`` that ``h^0 = [x | 0]`` reaches, every node sums ``p_j`` over
    the set bits of its neighbour word, the GRU cell (reset_after, gates z, r, h), the activation, the
    node pool weights and the concat; then the closed-form backward, layer by layer, with ``dp``
    gathered over the transposed word. Returns ``(out [B, T, Fo], grads)``. The keyword arguments
    switch on the named mutants (a mutant of the forward keeps the unmutated backward formulas)."""
    dt = torch.float64
    L = d["layer"]
    x, mask = d["x"].to(dt), d["mask"].to(dt)
    W, K, R, bias = (p.detach().to(dt) for p in (L.kernel, L.rnn.kernel, L.rnn.recurrent_kernel, L.rnn.bias))
    al = L.prelu_alpha.detach().to(dt) if L.prelu_alpha is not None else None
    B, T, N, Cin = x.shape
    C, nl = L.channels, L.n_layers
    nb = d["adj"] > 0
    if self_loop:
        nb = nb | torch.eye(N, dtype=torch.bool)
    if adj_transposed:
        nb = nb.transpose(1, 2)
    word, wordT = adj_words(nb)
    if dp_over_row_word:
        wordT = word
    lo = C - Cin if pad_left else 0                                        # where x sits in h^0
    zg, rg = (1, 0) if gates_rzh else (0, 1)                               # the gates' column blocks
    sl = lambda g: slice(g * C, (g + 1) * C)                               # noqa: E731
    pw = G.gat_pool_weights(mask, d["anom_pos"], c.pooling)

    def act(v):
        if L.activation == "prelu":
            return torch.where(v > 0, v, al * v)
        return torch.relu(v) if L.activation == "relu" else v

    def act_grad(v):
        if L.activation == "prelu":
            return torch.where(v > 0, torch.ones_like(v), al.expand_as(v))
        return (v > 0).to(dt) if L.activation == "relu" else torch.ones_like(v)

    # ---- forward
    h = torch.zeros(B, T, N, C, dtype=dt)
    h[..., lo:lo + Cin] = x
    saved = []
    b1 = torch.zeros_like(bias[1]) if no_recurrent_bias else bias[1]
    for l in range(nl):
        if l == 0:                                                         # the shortcut: Cin rows only
            p, g = x @ W[0][lo:lo + Cin], x @ R[lo:lo + Cin] + b1
        else:
            p, g = h @ W[l], h @ R + b1
        m = _gather(word, p)
        a = m @ K + bias[0]
        z = torch.sigmoid(a[..., sl(zg)] + g[..., sl(zg)])
        r = torch.sigmoid(a[..., sl(rg)] + g[..., sl(rg)])
        gh = g[..., sl(2)]
        if reset_before:
            cc = torch.tanh(a[..., sl(2)] + (r * h) @ R[:, sl(2)] + b1[sl(2)])
        else:
            cc = torch.tanh(a[..., sl(2)] + r * gh)
        saved.append((h, m, z, r, cc, gh))
        h = z * h + (1 - z) * cc
    pooled = torch.einsum("bi,btic->btc", pw, act(h))
    out = pooled if d["anom"] is None else torch.cat([d["anom"].to(dt), pooled], -1)
    # ---- backward
    Ca = c.Ca
    gq = d["g"].to(dt)
    gq = gq[:, :B, :Ca + C].transpose(0, 1) if c.tm else gq
    gl = gq[..., Ca:][:, :, None, :]                                       # [B, T, 1, C]
    grads = {}
    if Ca:
        grads["anom"] = gq[..., :Ca].clone()
    if al is not None:
        grads["alpha"] = (torch.where(h > 0, torch.zeros_like(h), h) * pw[:, None, :, None] * gl).sum((0, 1, 2))
    dh = pw[:, None, :, None] * act_grad(h) * gl
    dW = torch.zeros_like(W)
    dK, dR, db = torch.zeros_like(K), torch.zeros_like(R), torch.zeros_like(bias)
    for l in reversed(range(nl)):
        hl, m, z, r, cc, gh = saved[l]
        dz = dh * (hl - cc) * z * (1 - z)
        dc = dh * (1 - z) * (1 - cc * cc)
        dr = dc * gh * r * (1 - r)
        da = torch.cat([dz, dr, dc], -1)
        dg = torch.cat([dz, dr, dc * r], -1)
        db[0] += da.sum((0, 1, 2))
        db[1] += dg.sum((0, 1, 2))
        dK += torch.einsum("btik,btic->kc", m, da)
        dR += torch.einsum("btik,btic->kc", hl, dg)
        dp = _gather(wordT, da @ K.T)                                      # every dp element: one gather
        dW[l] += torch.einsum("btik,btic->kc", hl, dp)
        dh = dh * z + dg @ R.T + dp @ W[l].T
    grads["x"] = dh[..., lo:lo + Cin].clone()
    grads.update(kernel=dW, K=dK, R=dR, bias=db)
    for k in S.FROZEN[c.grads]:
        if k in grads:
            grads[k] = torch.zeros(0, dtype=dt)
    return out, S.split_kernel(grads, nl)


# mutant -> (keyword, the cases that must see it)
_PLAIN = ["inst_c2_w16", "layers_1", "layers_4", "nodes_33", "passes", "act_linear", "inst_c3_w8", "inst_c4_w32"]
MUTANTS = {
    "gates in the order r, z, h": ("gates_rzh", _PLAIN),
    "reset applied before the recurrent product": ("reset_before", ["inst_c2_w16", "layers_4", "nodes_33", "passes",
                                                                   "act_linear", "inst_c4_w32"]),
    "bias[1] dropped": ("no_recurrent_bias", _PLAIN),
    "self loop added": ("self_loop", ["inst_c2_w16", "no_diagonal", "nodes_33", "passes", "act_linear"]),
    "adj transposed in the message": ("adj_transposed", ["inst_c2_w16", "no_diagonal", "nodes_33", "passes",
                                                         "act_linear"]),
    "dp gathered over the row word": ("dp_over_row_word", ["inst_c2_w16", "no_diagonal", "nodes_33", "passes",
                                                           "act_linear", "layers_4"]),
    "h^0 padded on the wrong side": ("pad_left", _PLAIN),
}


@pytest.mark.parametrize("name", HIP_CASES)
def test_oracle_is_the_layer_plus_pool_plus_cat(name):
    """gated_pool_eager in float64 == GatedGraphConv + pool_nodes + cat, written out here; its
    time-major layout is the padded transpose."""
    c, d, (out64, _), _, _ = S.reference(name)
    layer = copy.deepcopy(d["layer"]).double()
    x, adj, mask = d["x"].double(), d["adj"].double(), d["mask"].double()
    with torch.no_grad():
        pooled = G.pool_nodes(layer(x, adj, mask), mask, d["anom_pos"], c.pooling)
        want = pooled if d["anom"] is None else torch.cat([d["anom"].double(), pooled], -1)
        assert torch.equal(out64, want)
        tm, Bret = G.gated_pool_eager(x, adj, mask, None if d["anom"] is None else d["anom"].double(),
                                      d["anom_pos"], layer, c.pooling, time_major=True)
    Mp, Cp = S.time_major_pad(c)
    assert Bret == c.B and tuple(tm.shape) == (c.T, Mp, Cp)
    assert torch.equal(tm[:, :c.B, :c.Ca + c.C].transpose(0, 1), want)
    assert torch.count_nonzero(tm[:, c.B:]) == 0 and torch.count_nonzero(tm[:, :, c.Ca + c.C:]) == 0


@pytest.mark.parametrize("name", HIP_CASES)
def test_walk_form_is_the_oracle(name):
    """The kernels' forward and closed-form backward equal the layer and its autograd in float64
    within 1e-10 of each quantity's scale on every HIP case of the GPU table."""
    c, d, (out64, g64), _, _ = S.reference(name)
    out, grads = walk_form(c, d)
    assert (out - out64).abs().max().item() <= 1e-10 * (1 + out64.abs().max().item())
    assert set(grads) == set(g64)
    for k, ref in g64.items():
        assert grads[k].shape == ref.shape, k
        if ref.numel():
            assert (grads[k] - ref).abs().max().item() <= 1e-10 * (1 + ref.abs().max().item()), k


@pytest.mark.parametrize("mutant,name", [(m, n) for m, (_, names) in MUTANTS.items() for n in names])
def test_mutant_is_far_outside_the_bound(mutant, name):
    """Each named mutant of the kernel's math is at least 5 of the GPU test's bounds away from the
    oracle in at least one compared quantity of every case meant to catch it."""
    c, d, (out64, g64), e32, _ = S.reference(name)
    out, grads = walk_form(c, d, **{MUTANTS[mutant][0]: True})
    worst = S.out_excess(out, out64, e32["out"])
    for k, ref in g64.items():
        if ref.numel():
            worst = max(worst, S._ratio((grads[k] - ref).abs().max().item(), S.grad_bound(ref, e32[k])))
    assert worst >= 5.0, (mutant, name, worst)


@pytest.mark.parametrize("name", [c.name for c in S.CASES if "hip" in c.tags and c.act in ("prelu", "relu")])
def test_kink_cap(name):
    """At most 5 % of a PReLU / ReLU case's (window, step, channel) entries have their upstream
    gradient zeroed, from the float64 oracle alone; the zeroed entries are zero in ``g`` and the
    anomaly channels are untouched."""
    c, d, _, _, (share, eps) = S.reference(name)
    assert eps >= S.KINK_EPS
    assert share <= S.KINK_SHARE, (name, share, eps)
    kink, _ = S.kink_mask(c, d)
    g = d["g"][:, :c.B, :c.Ca + c.C].transpose(0, 1) if c.tm else d["g"]
    assert torch.count_nonzero(g[..., c.Ca:][kink]) == 0
    if c.Ca:
        assert torch.count_nonzero(g[..., :c.Ca]) > 0


def test_linear_cases_zero_nothing():
    for name in ("act_linear",):
        c, d, _, _, (share, _) = S.reference(name)
        assert share == 0.0 and torch.count_nonzero(d["g"]) == d["g"].numel()


def test_builders():
    c, d, _, _, _ = S.reference("degenerate_mean")
    m, adj = d["mask"], d["adj"]
    assert m[0].sum() == 0 and d["anom_pos"][0] == -1 and m[1].sum() == 1
    assert m[2, 3] == 1 and adj[2, 3].sum() == 0 and adj[2, :, 3].sum() == 0 and d["anom_pos"][2] == 3
    assert m[3, 2] == 0 and adj[3, 0, 2] == 1
    assert (d["x"][0] == 2.5).all()
    c, d, _, _, _ = S.reference("inst_c2_w16")
    adj = d["adj"]
    assert not torch.equal(adj, adj.transpose(1, 2))                       # asymmetric
    diag = torch.diagonal(adj, dim1=1, dim2=2)
    assert diag[0].sum() > 0 and diag[1].sum() == 0                        # a diagonal in every other sample
    c, d, _, _, _ = S.reference("no_diagonal")
    assert torch.diagonal(d["adj"], dim1=1, dim2=2).sum() == 0
    c, d, (out64, _), _, _ = S.reference("zeros")
    assert torch.count_nonzero(d["x"]) == 0 and out64[..., c.Ca:].abs().max() > 0
    c, d, _, _, _ = S.reference("nodes_64_dense")
    v = d["mask"][0] > 0
    assert (d["adj"][0][v][:, v] == 1).all()
    assert d["layer"].rnn.bias.abs().min() > 0
    c, d, _, _, _ = S.reference("grads_some")
    ps = S.layer_params(d["layer"])
    assert ps["kernel"].requires_grad and ps["bias"].requires_grad and not ps["K"].requires_grad
    assert not any(p.requires_grad for p in S.layer_params(S.reference("grads_none")[1]["layer"]).values())


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_case_reaches_its_branches(case, monkeypatch):
    """Tags are recomputed from the shapes; gated_pool_hip_ok (with the device test forced on) agrees
    with the table on which cases take the HIP path."""
    assert case.tags, case.name
    for t in case.tags:
        assert S.PREDICATES[t](case), (case.name, t)
    import gnnqc.ops as ops
    monkeypatch.setattr(ops, "use_hip", lambda t: True)
    monkeypatch.delenv("GNNQC_GATED_HIP", raising=False)
    d = S.reference(case.name)[1]
    assert G.gated_pool_hip_ok(d["x"], d["layer"], case.pooling) == ("hip" in case.tags)


def test_hip_gate_conditions(monkeypatch):
    """Each condition of gated_pool_hip_ok on its own: a CPU tensor, a float64 tensor, a 3-d tensor,
    N = 65, Cin = 5, a layer built for another width, C = 12, n_layers = 5, pooling = max, an
    activation the kernels lack, the environment switch; time_major off the HIP path raises."""
    import gnnqc.ops as ops
    from gnnqc.models.graphconv import GatedGraphConv
    assert (G.GATED_MAX_NODES, G.GATED_WIDTHS, G.GATED_MAX_LAYERS) == (64, (8, 16, 32), 4)
    x = torch.randn(2, 3, 9, 2)
    ok = GatedGraphConv(2, 16, 2, "prelu")
    assert not G.gated_pool_hip_ok(x, ok, "mean")                          # CPU tensor, no device
    monkeypatch.setattr(ops, "use_hip", lambda t: True)
    monkeypatch.delenv("GNNQC_GATED_HIP", raising=False)
    for pooling in ("mean", "sum", "selection"):
        assert G.gated_pool_hip_ok(x, ok, pooling)
    for C in (8, 16, 32):
        for L in (1, 2, 3, 4):
            for act in (None, "linear", "relu", "prelu"):
                assert G.gated_pool_hip_ok(x, GatedGraphConv(2, C, L, act), "mean")
    assert G.gated_pool_hip_ok(torch.randn(2, 3, 64, 4), GatedGraphConv(4, 8, 1), "mean")
    assert G.gated_pool_hip_ok(torch.randn(2, 3, 1, 1), GatedGraphConv(1, 8, 1), "mean")
    assert not G.gated_pool_hip_ok(x.double(), ok, "mean")
    assert not G.gated_pool_hip_ok(x[0], ok, "mean")
    assert not G.gated_pool_hip_ok(torch.randn(2, 3, 65, 2), ok, "mean")
    assert not G.gated_pool_hip_ok(torch.randn(2, 3, 9, 5), GatedGraphConv(5, 16, 2), "mean")
    assert not G.gated_pool_hip_ok(torch.randn(2, 3, 9, 3), ok, "mean")    # built for Cin = 2
    assert not G.gated_pool_hip_ok(x, GatedGraphConv(2, 12, 2), "mean")
    assert not G.gated_pool_hip_ok(x, GatedGraphConv(2, 64, 2), "mean")
    assert not G.gated_pool_hip_ok(x, GatedGraphConv(2, 16, 5), "mean")
    assert not G.gated_pool_hip_ok(x, ok, "max")
    assert not G.gated_pool_hip_ok(x, GatedGraphConv(2, 16, 2, "tanh"), "mean")
    monkeypatch.setenv("GNNQC_GATED_HIP", "0")
    assert not G.gated_pool_hip_ok(x, ok, "mean")
    adj, mask = torch.ones(2, 9, 9), torch.ones(2, 9)
    with pytest.raises(ValueError):
        G.gated_pool(x, adj, mask, None, torch.zeros(2, dtype=torch.long), ok, "mean", time_major=True)
    with torch.no_grad():                                                  # ... and batch-major is the eager layer
        got = G.gated_pool(x, adj, mask, None, torch.zeros(2, dtype=torch.long), ok, "mean")
        assert torch.equal(got, G.pool_nodes(ok(x, adj, mask), mask, None, "mean"))


def test_routes():
    """The GatedGraphConv route predicate: false on CPU tensors, for the network-wide layout, with a
    SensorsTimeLayer, a SpatialTransformer or coordinates in front, for pooling max, N > 64 and
    widths or activations the kernels lack; true (device test forced on) for the CML configuration,
    where the other layers' predicates stay false. On the CPU the model computes the layer +
    pool_nodes + cat."""
    import gnnqc.ops as ops
    from gnnqc import config as C
    from gnnqc.models import GCNClassifier
    from gnnqc.models.graphconv import GatedGraphConv
    pc = C.normalize_preproc(C.default("preprocessing_cml"))
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(2, 181, 5, 2, generator=gen)
    adj = (torch.rand(2, 5, 5, generator=gen) > 0.5).float()
    inputs = (x, torch.randn(2, 181, 2, generator=gen), adj, torch.ones(2, 5), torch.zeros(2, dtype=torch.long))

    def model(top=None, pool=None, **gc):
        mc = C.default("model_cml")
        mc["graph_convolution"].update(dict(layer="GatedGraphConv", n_layers=2), **gc)
        for k, v in (top or {}).items():
            mc[k] = v
        if pool:
            mc["pooling"] = dict(mc.get("pooling") or {}, **pool)
        return GCNClassifier(mc, pc)

    m = model()
    assert isinstance(m.gcn_layer, GatedGraphConv) and m.gcn_layer.n_layers == 2 and m.gcn_layer.channels == 16
    assert not m._cml_gated_time_major(inputs)                               # (CPU tensors)
    assert not m._cml_agnn_time_major(inputs) and not m._cml_edge_time_major(inputs)
    assert not m._cml_gat_time_major(inputs) and not m._cml_time_major(inputs) and not m._fused_ok()
    assert m.fused_loss(inputs, torch.zeros(2), torch.ones(2), 1.0, 5.0) is None
    with torch.no_grad():
        want = torch.cat([inputs[1], G.pool_nodes(m.gcn_layer(x, adj, inputs[3]), inputs[3], inputs[4], "mean")], -1)
        assert torch.equal(m.temporal_input(inputs), want)
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(ops, "use_hip", lambda t: True)
        mp.delenv("GNNQC_GATED_HIP", raising=False)
        mp.setattr(type(m.time_layer), "time_major_ok", lambda self, x, c: True)
        assert m._cml_gated_time_major(inputs)
        assert not m._cml_agnn_time_major(inputs) and not m._cml_edge_time_major(inputs)
        assert not m._cml_gat_time_major(inputs) and not m._fused_ok()
        assert not m._cml_gated_time_major(inputs + (torch.zeros(2, 5, 4),))   # coordinates in front
        assert not model(pool=dict(aggregation_type="max"))._cml_gated_time_major(inputs)
        assert model(pool=dict(type="selection"))._cml_gated_time_major(inputs)
        assert not model(units=12)._cml_gated_time_major(inputs)
        assert not model(n_layers=5)._cml_gated_time_major(inputs)
        assert not model(activation="tanh")._cml_gated_time_major(inputs)
        assert model(units=32, n_layers=4, activation="relu")._cml_gated_time_major(inputs)
        big = (torch.randn(2, 181, 65, 2),) + inputs[1:]
        assert not m._cml_gated_time_major(big)                              # N > 64
        assert not model(layer="AGNNConv")._cml_gated_time_major(inputs)
        mp.setenv("GNNQC_GATED_HIP", "0")
        assert not m._cml_gated_time_major(inputs)
        mp.delenv("GNNQC_GATED_HIP")
        m.sensors_time_layer = object()
        assert not m._cml_gated_time_major(inputs)
        m.sensors_time_layer = None
        m.spatial_transformer = object()
        assert not m._cml_gated_time_major(inputs)
        m.spatial_transformer = None
        m.per_sensor = False
        assert not m._cml_gated_time_major(inputs)                           # network-wide layout
    finally:
        mp.undo()


def test_case_table_covers_the_issue():
    names = {c.name for c in S.CASES}
    assert len(names) == len(S.CASES)
    assert {t for c in S.CASES for t in c.tags} == set(S.PREDICATES)
    hip = [c for c in S.CASES if "hip" in c.tags]
    inst = [c for c in hip if c.name.startswith("inst_")]
    assert {(c.Cin, c.C) for c in inst} == {(a, w) for a in (1, 2, 3, 4) for w in (8, 16, 32)}
    assert {c.L for c in hip if c.C == 16} >= {1, 2, 3, 4} and any(c.L == 4 and c.C == 32 for c in hip)
    assert {c.N for c in hip} >= {1, 7, 33, 64} and {c.pooling for c in hip} == {"mean", "sum", "selection"}
    assert any(c.N == 64 and c.pooling == "selection" for c in hip) and any(c.N == 64 and c.kind == "dense" for c in hip)
    assert any((c.B, c.T, c.N) == (3, 7, 5) for c in hip)
    assert {c.tm for c in hip if (c.B, c.T, c.N) == (48, 181, 7)} == {True, False}
    tm = [c for c in hip if c.tm]
    assert {c.B for c in tm} >= {5, 16, 17} and {c.Ca > 0 for c in tm} == {True, False}
    assert {"tm_pad_ch", "tm_full_ch"} <= {t for c in tm for t in c.tags}
    assert {c.act for c in hip} == {"prelu", "relu", None} and any(not c.training for c in hip)
    assert {c.kind for c in hip} >= {"degenerate", "zeros", "dense", "plain"}
    assert {c.pooling for c in hip if c.kind == "degenerate"} == {"mean", "sum", "selection"}
    assert {c.grads for c in hip} == {"all", "some", "none"}
    eager = [c for c in S.CASES if "eager" in c.tags]
    assert any(c.N == 65 for c in eager) and any(c.C == 12 for c in eager) and any(c.L == 5 for c in eager)
    assert any(c.pooling == "max" for c in eager) and any(c.act == "tanh" for c in eager)
