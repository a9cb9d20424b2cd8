"""CPU part of the per-node GATConv kernel tests (``tests/test_gat_node_kernels_gpu.py``): the
input-space form the kernels compute, written in float64 in the node layout, is checked against the
oracle (:func:`gnnqc.ops.gcn.gat_node_tm_eager`), named mutants of that form are shown to lie far
outside the GPU test's bound, every case of the GPU table is checked to still reach the branch it
names, and each condition of :func:`gnnqc.ops.gcn.gat_node_tm_ok` is tested on its own."""
import copy

import pytest
import torch
import torch.nn.functional as F

import test_gat_node_kernels_gpu as S
from gnnqc.ops import gcn as G


def node_form(c, d, dtype=torch.float64, self_loops=True, padded_neighbours=False, skip_word=None,
              raw_first=False, row_order="bn"):
    """The kernels' math (``csrc/kernels/gat_node.hip``), written out: scores as input-space dot
    products with ``u = W a``, masked edge softmax over the neighbours j, aggregation of x, then
    ``W``, bias, activation and mask; row ``m = b*N + i`` of step t holds ``[H*C GAT | Cin raw x |
    0 pad]`` and the rows past ``B*N`` are zero. The keyword arguments switch on the named mutants."""
    L = d["layer"]
    x, adj, mask = d["x"].to(dtype), d["adj"].to(dtype), d["mask"].to(dtype)
    W = L.kernel.detach().to(dtype)                                          # [Cin, H, C]
    a_s, a_n = L.attn_kernel_self.detach().to(dtype)[..., 0], L.attn_kernel_neighs.detach().to(dtype)[..., 0]
    B, T, N, Cin = x.shape
    H, C = W.shape[1], W.shape[2]
    u_s = torch.einsum("fhc,ch->fh", W, a_s)
    u_n = torch.einsum("fhc,ch->fh", W, a_n)
    s_self, s_nb = x @ u_s, x @ u_n                                          # [B, T, N, H]
    e = F.leaky_relu(s_self[:, :, :, None, :] + s_nb[:, :, None, :, :], 0.2)     # [B, T, i, j, H]
    nb = adj + torch.eye(N, dtype=dtype) * mask[:, :, None] if self_loops else adj
    nb = nb > 0
    if padded_neighbours:
        nb = nb | (mask[:, None, :] == 0)
    if skip_word is not None:
        nb = nb.clone()
        nb[:, :, 64 * skip_word:64 * skip_word + 64] = False
    nb = nb[:, None, :, :, None]
    m = torch.where(nb, e, torch.full_like(e, -float("inf"))).amax(3, keepdim=True)
    e = e - torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    p = torch.exp(e) * nb
    den = p.sum(3, keepdim=True)
    att = torch.where(den > 0, p / den, torch.zeros_like(p))
    z = torch.einsum("btijh,btjf->btihf", att, x)
    o = torch.einsum("btihf,fhc->btihc", z, W).reshape(B, T, N, H * C) + L.bias.detach().to(dtype)
    if L.activation == "prelu":
        o = torch.where(o > 0, o, L.prelu_alpha.detach().to(dtype) * o)
    elif L.activation == "relu":
        o = torch.relu(o)
    o = o * mask[:, None, :, None]
    rows = torch.cat([x, o] if raw_first else [o, x], -1)                    # [B, T, N, Fo]
    M, Mp, Cp = S.time_major_pad(c)
    seq = rows.permute(1, 0, 2, 3) if row_order == "bn" else rows.permute(1, 2, 0, 3)
    return F.pad(seq.reshape(T, M, -1), (0, Cp - rows.shape[-1], 0, Mp - M))


@pytest.mark.parametrize("name", S.HIP_CASES)
def test_oracle_is_the_models_temporal_input(name):
    """gat_node_tm_eager in float64 == the layer, cat([h, x]) and graph_reshape (the model's eager
    ``temporal_input``), time-major, with zero padding rows and channels."""
    from gnnqc.models.gcn import graph_reshape
    c, d, (out64, _), _ = S.reference(name)
    layer = copy.deepcopy(d["layer"]).double()
    x, adj, mask = d["x"].double(), d["adj"].double(), d["mask"].double()
    with torch.no_grad():
        want = graph_reshape(torch.cat([layer(x, adj, mask), x], -1))        # [B*N, T, Fo]
    M, Mp, Cp = S.time_major_pad(c)
    Fo = want.shape[-1]
    assert tuple(out64.shape) == (c.T, Mp, Cp) and Fo == c.H * c.C + c.Cin
    assert torch.equal(out64[:, :M, :Fo].transpose(0, 1), want)
    assert torch.count_nonzero(out64[:, M:]) == 0 and torch.count_nonzero(out64[:, :, Fo:]) == 0


@pytest.mark.parametrize("name", S.HIP_CASES)
def test_node_form_is_the_oracle(name):
    """The kernels' math in the node layout equals the oracle in float64 on every HIP case."""
    c, d, (out64, _), _ = S.reference(name)
    got = node_form(c, d)
    assert got.shape == out64.shape
    scale = 1.0 + out64.abs().max().item()
    assert (got - out64).abs().max().item() < 1e-12 * scale * max(1.0, c.xscale)


DISPATCH = [n for n in S.HIP_CASES if n.startswith("dispatch_")]
MUTANTS = {
    # mutant -> (keyword arguments of node_form, the cases meant to catch it)
    "no_self_loops": (dict(self_loops=False), DISPATCH + ["nodes_1", "nodes_210", "degenerate"]),
    "padded_neighbours": (dict(padded_neighbours=True), ["degenerate", "degenerate_h2_relu"]),
    "word_1_ignored": (dict(skip_word=1), DISPATCH + ["nodes_128", "nodes_129", "nodes_210", "nodes_256_dense",
                                                      "rows_300_n130"]),
    "raw_and_gat_swapped": (dict(raw_first=True), DISPATCH + ["nodes_7", "nodes_256_dense"]),
    "row_order_i_b": (dict(row_order="nb"), DISPATCH + ["nodes_7", "nodes_65", "passes"]),
}


@pytest.mark.parametrize("mutant,name", [(m, n) for m, (_, names) in MUTANTS.items() for n in names])
def test_mutant_is_far_outside_the_bound(mutant, name):
    """Each named mutant of the kernel's math is at least 5 of the GPU test's output bounds away
    from the oracle on the cases meant to catch it."""
    c, d, (out64, _), e32 = S.reference(name)
    got = node_form(c, d, **MUTANTS[mutant][0])
    assert S.out_excess(got, out64, e32["out"]) >= 5.0, S.out_excess(got, out64, e32["out"])


def test_degenerate_builder():
    c, d, (out64, g64), _ = S.reference("degenerate")
    m, adj = d["mask"], d["adj"]
    assert m[0].sum() == 0 and m[1].sum() == 1
    assert m[2, 3] == 1 and adj[2, 3].sum() == 0 and adj[2, :, 3].sum() == 0
    assert (d["x"][(m == 0)[:, None, :].expand(c.B, c.T, c.N)] == 123.0).all()
    HC = c.H * c.C
    # nothing valid in sample 0: its GAT channels are zero, its raw channels are the input
    assert torch.count_nonzero(out64[:, :c.N, :HC]) == 0
    assert (out64[:, :c.N, HC:HC + c.Cin] == 123.0).all()
    # the diagonal is in the data for every other sample only
    d2 = S.reference("dispatch_c3f16h1")[1]
    diag = torch.diagonal(d2["adj"], dim1=1, dim2=2)
    assert torch.equal(diag[0], d2["mask"][0]) and diag[1].sum() == 0
    eq = S.reference("scores_equal")[1]
    xv = eq["x"][0, 0][eq["mask"][0] > 0]
    assert (xv == xv[0]).all()
    dense = S.reference("nodes_256_dense")[1]
    mm = dense["mask"][1]
    assert torch.equal(dense["adj"][1], (mm[:, None] * mm[None, :]) * (1 - torch.eye(256)))
    sparse = S.reference("nodes_210")[1]
    deg = sparse["adj"].sum(-1)[sparse["mask"] > 0].mean().item()
    assert 3.0 < deg < 12.0, deg


@pytest.mark.parametrize("case", S.CASES, ids=[c.name for c in S.CASES])
def test_case_reaches_its_branches(case, monkeypatch):
    """Tags are recomputed from the shapes; gat_node_tm_ok (with the device test forced on) agrees
    with the table on which cases take the HIP path; valid inputs: every sample keeps a node except
    in the degenerate cases."""
    assert case.tags, case.name
    for tag in case.tags:
        assert S.PREDICATES[tag](case), f"{case.name} no longer reaches '{tag}'"
    assert ("hip" in case.tags) != ("off_hip" in case.tags)
    import gnnqc.ops as ops
    monkeypatch.setattr(ops, "use_hip", lambda t: True)
    monkeypatch.delenv("GNNQC_GAT_HIP", raising=False)
    d = S.node_inputs(case)
    assert G.gat_node_tm_ok(d["x"], d["layer"]) == ("hip" in case.tags)
    monkeypatch.setenv("GNNQC_GAT_HIP", "0")
    assert not G.gat_node_tm_ok(d["x"], d["layer"])
    if case.kind != "degenerate":
        assert (d["mask"].sum(-1) > 0).all()
    assert case.B * case.T * case.N * case.N * case.H * 8 < 64 << 20       # the oracle's edge tensor stays small


def test_tm_ok_conditions(monkeypatch):
    """Each condition of gat_node_tm_ok on its own: a CPU tensor, a float64 tensor, N = 257, Cin = 5,
    an uninstantiated width or head count, averaged heads, an activation the kernels lack, attention
    dropout while training (fine in eval mode), and the GNNQC_GAT_HIP switch."""
    import gnnqc.ops as ops
    from gnnqc.models.graphconv import GATConv
    monkeypatch.delenv("GNNQC_GAT_HIP", raising=False)
    x = torch.zeros(2, 3, 256, 3)
    ok = GATConv(3, 16, 1, dropout_rate=0.0, activation="prelu")
    assert not G.gat_node_tm_ok(x, ok)                                     # not on a GPU
    monkeypatch.setattr(ops, "use_hip", lambda t: True)
    assert G.gat_node_tm_ok(x, ok)
    assert not G.gat_node_tm_ok(x.double(), ok)
    assert not G.gat_node_tm_ok(x[0], ok)
    assert not G.gat_node_tm_ok(torch.zeros(2, 3, 257, 3), ok)
    assert not G.gat_node_tm_ok(torch.zeros(2, 3, 9, 5), GATConv(5, 16, 1, dropout_rate=0.0))
    assert not G.gat_node_tm_ok(torch.zeros(2, 3, 9, 2), ok)               # the layer's Cin is 3
    drop = GATConv(3, 16, 1, dropout_rate=0.5, activation="prelu")
    assert not G.gat_node_tm_ok(x, drop)
    assert G.gat_node_tm_ok(x, drop.eval())
    assert not G.gat_node_tm_ok(x, GATConv(3, 12, 1, dropout_rate=0.0))
    assert not G.gat_node_tm_ok(x, GATConv(3, 16, 3, dropout_rate=0.0))
    assert not G.gat_node_tm_ok(x, GATConv(3, 16, 1, dropout_rate=0.0, activation="tanh"))
    assert not G.gat_node_tm_ok(x, GATConv(3, 16, 2, concat_heads=False, dropout_rate=0.0))
    for act in (None, "linear", "relu", "prelu"):
        assert G.gat_node_tm_ok(x, GATConv(3, 8, 2, dropout_rate=0.0, activation=act))
    monkeypatch.setenv("GNNQC_GAT_HIP", "0")
    assert not G.gat_node_tm_ok(x, ok)
    monkeypatch.setenv("GNNQC_GAT_HIP", "1")
    assert G.gat_node_tm_ok(x, ok)
    with pytest.raises(ValueError):
        G.gat_node_tm(x, torch.zeros(2, 256, 256), torch.ones(2, 256), drop.train())


def test_case_table_covers_the_issue():
    names = {c.name for c in S.CASES}
    assert len(names) == len(S.CASES)
    assert {t for c in S.CASES for t in c.tags} == set(S.PREDICATES)
    hip = [c for c in S.CASES if "hip" in c.tags]
    assert {c.N for c in hip} >= {1, 7, 33, 64, 65, 128, 129, 210, 256}
    assert {(c.C, c.H) for c in hip} == {(C, H) for C in S.K_WIDTHS[0] for H in S.K_WIDTHS[1]}
    assert {c.Cin for c in hip} >= {1, 3, 4} and {c.act for c in hip} == {"prelu", "relu", None}
    assert any(c.adj == "dense" and c.N == 256 for c in hip)
    assert any((c.B, c.T, c.N) == (3, 100, 130) for c in hip)
    multi = [c for c in hip if "multi_pass_bwd" in c.tags]
    assert any(c.N > 64 for c in multi) and any("multi_pass_all" in c.tags for c in multi)
    assert all(c.B <= 3 for c in hip) and all(c.T <= 11 for c in hip if c not in multi and c.N != 130)
    assert {c.N for c in S.CASES if "off_hip" in c.tags} >= {257}
    assert any(c.dropout > 0 and c.training for c in S.CASES if "off_hip" in c.tags)


def test_model_route_predicate_on_the_cpu(monkeypatch):
    """_soil_gat_fused is false without a GPU, and for a GeneralConv model, whatever the switch; the
    model then computes what it computes today (the eager temporal_input)."""
    from gnnqc import config as C
    from gnnqc.models import GCNClassifier
    pc = C.normalize_preproc(C.default("preprocessing_soilnet"))
    mc = C.default("model_soilnet")
    mc["graph_convolution"]["layer"] = "GATConv"
    torch.manual_seed(0)
    model = GCNClassifier(mc, pc).eval()
    x = torch.rand(1, 337, 5, 3)
    inputs = (x, torch.ones(1, 5, 5), torch.ones(1, 5))
    assert not model._soil_gat_fused(inputs) and not model._soil_fused(inputs)
    with torch.no_grad():
        want = model.time_layer(model.temporal_input(inputs))
        assert torch.equal(model.features(inputs), want)
