"""CPU part of the GATConv kernel tests (``tests/test_gat_kernels_gpu.py``): the float64 oracle is
checked against the layer, the input-space form the kernels compute is checked against the oracle,
named mutants of that form are shown to lie far outside the GPU test's bound, and every case of the
GPU table is checked to still reach the branch it names."""
import copy

import pytest
import torch
import torch.nn.functional as F

import test_gat_kernels_gpu as S
from gnnqc.ops import gcn as G

HIP_CASES = [c.name for c in S.CASES if "hip" in c.tags]


def input_space_form(c, d, dtype=torch.float64, self_loops=True, slope=0.2, softmax_dim="j", concat=True,
                     subtract_max=True, padded_neighbours=False):
    """The kernels' math (``csrc/kernels/gat.hip``), written out: scores as input-space dot products
    with ``u = W a``, masked edge softmax over the neighbours j, aggregation of x, then ``W``, bias,
    activation, mask, node pool weights and the concat with the flagged series. The keyword
    arguments switch on the named mutants."""
    L = d["layer"]
    x, adj, mask = d["x"].to(dtype), d["adj"].to(dtype), d["mask"].to(dtype)
    W = L.kernel.detach().to(dtype)                                          # [Cin, H, C]
    a_s, a_n = L.attn_kernel_self.detach().to(dtype)[..., 0], L.attn_kernel_neighs.detach().to(dtype)[..., 0]
    B, T, N, _ = x.shape
    H, C = W.shape[1], W.shape[2]
    u_s = torch.einsum("fhc,ch->fh", W, a_s)
    u_n = torch.einsum("fhc,ch->fh", W, a_n)
    s_self, s_nb = x @ u_s, x @ u_n                                          # [B, T, N, H]
    e = F.leaky_relu(s_self[:, :, :, None, :] + s_nb[:, :, None, :, :], slope)   # [B, T, i, j, H]
    nb = adj + torch.eye(N, dtype=dtype) * mask[:, :, None] if self_loops else adj
    nb = nb > 0
    if padded_neighbours:
        nb = nb | (mask[:, None, :] == 0)
    nb = nb[:, None, :, :, None]
    dim = 3 if softmax_dim == "j" else 2
    if subtract_max:
        m = torch.where(nb, e, torch.full_like(e, -float("inf"))).amax(dim, keepdim=True)
        e = e - torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    p = torch.exp(e) * nb
    den = p.sum(dim, keepdim=True)
    att = torch.where(den > 0, p / den, torch.zeros_like(p))
    z = torch.einsum("btijh,btjf->btihf", att, x)
    o = torch.einsum("btihf,fhc->btihc", z, W)
    if not concat:
        o = o.mean(3, keepdim=True).expand(B, T, N, H, C)
    o = o.reshape(B, T, N, H * C) + L.bias.detach().to(dtype)
    if L.activation == "prelu":
        o = torch.where(o > 0, o, L.prelu_alpha.detach().to(dtype) * o)
    elif L.activation == "relu":
        o = torch.relu(o)
    pw = G.gat_pool_weights(mask, d["anom_pos"], c.pooling)
    pooled = torch.einsum("bi,btik->btk", pw, o)
    return pooled if d["anom"] is None else torch.cat([d["anom"].to(dtype), pooled], -1)


@pytest.mark.parametrize("name", [c.name for c in S.CASES])
def test_oracle_is_the_layer_plus_pool_plus_cat(name):
    """gat_pool_eager in float64 == GATConv + pool_nodes + cat, written out here; its time-major
    layout is the padded transpose."""
    c, d, (out64, _), _ = S.reference(name)
    layer = copy.deepcopy(d["layer"]).double()
    x, adj, mask = d["x"].double(), d["adj"].double(), d["mask"].double()
    with torch.no_grad():
        pooled = G.pool_nodes(layer(x, adj, mask), mask, d["anom_pos"], c.pooling)
        want = pooled if d["anom"] is None else torch.cat([d["anom"].double(), pooled], -1)
        assert torch.equal(out64, want)
        tm, Bret = G.gat_pool_eager(x, adj, mask, None if d["anom"] is None else d["anom"].double(), d["anom_pos"],
                                    layer, c.pooling, time_major=True)
    Mp, Cp = S.time_major_pad(c)
    Fo = want.shape[-1]
    assert Bret == c.B and tuple(tm.shape) == (c.T, Mp, Cp)
    assert torch.equal(tm[:, :c.B, :Fo].transpose(0, 1), want)
    assert torch.count_nonzero(tm[:, c.B:]) == 0 and torch.count_nonzero(tm[:, :, Fo:]) == 0


@pytest.mark.parametrize("name", HIP_CASES)
def test_input_space_form_is_the_oracle(name):
    """The kernels' math equals the layer in float64 on every HIP case of the GPU table."""
    c, d, (out64, _), _ = S.reference(name)
    got = input_space_form(c, d)
    scale = 1.0 + out64.abs().max().item()
    assert (got - out64).abs().max().item() < 1e-12 * scale * max(1.0, c.xscale)


def _dispatch(*triples):
    return [f"dispatch_c{a}f{b}h{h}_{p}" for a, b, h in triples for p in ("mean", "selection")]


ALL_DISPATCH = _dispatch((2, 16, 1), (2, 8, 2), (2, 16, 2), (1, 8, 1), (3, 32, 1), (4, 16, 1))
MUTANTS = {
    # mutant -> (keyword arguments of input_space_form, the cases meant to catch it)
    "no_self_loops": (dict(self_loops=False), ALL_DISPATCH + ["degenerate_selection", "nodes_1"]),
    "leaky_slope_0.3": (dict(slope=0.3), ALL_DISPATCH + ["nodes_64"]),
    "softmax_over_i": (dict(softmax_dim="i"), ALL_DISPATCH + ["nodes_33"]),
    "head_mean": (dict(concat=False), _dispatch((2, 8, 2), (2, 16, 2)) + ["nodes_33", "train_no_dropout_h2"]),
    "padded_neighbours": (dict(padded_neighbours=True),
                          ALL_DISPATCH + ["degenerate_mean", "degenerate_sum", "degenerate_selection"]),
}


@pytest.mark.parametrize("mutant,name", [(m, n) for m, (_, names) in MUTANTS.items() for n in names])
def test_mutant_is_far_outside_the_bound(mutant, name):
    """Each named mutant of the kernel's math is at least 5 of the GPU test's output bounds away
    from the oracle on the cases meant to catch it."""
    c, d, (out64, _), e32 = S.reference(name)
    got = input_space_form(c, d, **MUTANTS[mutant][0])
    assert S.out_excess(got, out64, e32["out"]) >= 5.0, S.out_excess(got, out64, e32["out"])


@pytest.mark.parametrize("name", ["scores_x30", "scores_x30_selection_h2"])
def test_max_not_subtracted_overflows_only_on_large_scores(name):
    """Without the max the float32 softmax overflows on the large-score cases (non-finite output,
    which the GPU test rejects) - and only there: on a unit-scale case that mutant is invisible."""
    c, d, (out64, _), e32 = S.reference(name)
    got = input_space_form(c, d, dtype=torch.float32, subtract_max=False)
    assert not torch.isfinite(got).all()
    assert S.out_excess(got.double(), out64, e32["out"]) == float("inf")
    ok = input_space_form(c, d, dtype=torch.float32)
    assert torch.isfinite(ok).all()
    c1, d1, (o1, _), e1 = S.reference("dispatch_c2f16h1_mean")
    assert S.out_excess(input_space_form(c1, d1, dtype=torch.float32, subtract_max=False).double(), o1,
                        e1["out"]) <= 1.0


def test_degenerate_builder():
    c, d, (out64, g64), _ = S.reference("degenerate_selection")
    m, adj = d["mask"], d["adj"]
    assert m[0].sum() == 0 and d["anom_pos"][0] == -1 and m[1].sum() == 1
    assert m[2, 3] == 1 and adj[2, 3].sum() == 0 and adj[2, :, 3].sum() == 0 and d["anom_pos"][2] == 3
    assert (d["x"][(m == 0)[:, None, :].expand(c.B, c.T, c.N)] == 123.0).all()
    assert torch.count_nonzero(out64[0, :, c.Cin:]) == 0                  # nothing valid: the pooled row is zero
    assert torch.count_nonzero(g64["x"][0]) == 0
    # the diagonal is in the data for every other sample only
    d2 = S.reference("dispatch_c2f16h1_mean")[1]
    diag = torch.diagonal(d2["adj"], dim1=1, dim2=2)
    assert torch.equal(diag[0], d2["mask"][0]) and diag[1].sum() == 0
    eq = S.reference("scores_equal")[1]
    xv = eq["x"][0, 0][eq["mask"][0] > 0]
    assert (xv == xv[0]).all()


@pytest.mark.parametrize("case", S.CASES, ids=[c.name for c in S.CASES])
def test_case_reaches_its_branches(case, monkeypatch):
    """Tags are recomputed from the shapes; gat_pool_hip_ok (with the device test forced on) agrees
    with the table on which cases take the HIP path."""
    assert case.tags, case.name
    for tag in case.tags:
        assert S.PREDICATES[tag](case), f"{case.name} no longer reaches '{tag}'"
    assert ("hip" in case.tags) != ("eager" in case.tags)
    import gnnqc.ops as ops
    monkeypatch.setattr(ops, "use_hip", lambda t: True)
    monkeypatch.delenv("GNNQC_GAT_HIP", raising=False)
    d = S.reference(case.name)[1]
    assert G.gat_pool_hip_ok(d["x"], d["layer"], case.pooling) == ("hip" in case.tags)
    monkeypatch.setenv("GNNQC_GAT_HIP", "0")
    assert not G.gat_pool_hip_ok(d["x"], d["layer"], case.pooling)
    assert case.B * case.T * case.N * case.N * case.H * 8 < 64 << 20       # the oracle's edge tensor stays small


def test_hip_gate_conditions(monkeypatch):
    """Each condition of gat_pool_hip_ok on its own: N = 65, pooling = max, Cin = 5, attention
    dropout while training, an uninstantiated width, an activation the kernels lack, a CPU tensor."""
    import gnnqc.ops as ops
    from gnnqc.models.graphconv import GATConv
    x = torch.zeros(2, 3, 64, 2)
    ok = GATConv(2, 16, 1, dropout_rate=0.0, activation="prelu")
    assert not G.gat_pool_hip_ok(x, ok, "mean")                            # not on a GPU
    monkeypatch.setattr(ops, "use_hip", lambda t: True)
    assert G.gat_pool_hip_ok(x, ok, "mean") and G.gat_pool_hip_ok(x, ok, "selection")
    assert not G.gat_pool_hip_ok(torch.zeros(2, 3, 65, 2), ok, "mean")
    assert not G.gat_pool_hip_ok(x, ok, "max")
    assert not G.gat_pool_hip_ok(torch.zeros(2, 3, 9, 5), GATConv(5, 16, 1, dropout_rate=0.0), "mean")
    drop = GATConv(2, 16, 1, dropout_rate=0.5, activation="prelu")
    assert not G.gat_pool_hip_ok(x, drop, "mean")
    assert G.gat_pool_hip_ok(x, drop.eval(), "mean")
    assert not G.gat_pool_hip_ok(x, GATConv(2, 12, 1, dropout_rate=0.0), "mean")
    assert not G.gat_pool_hip_ok(x, GATConv(2, 16, 3, dropout_rate=0.0), "mean")
    assert not G.gat_pool_hip_ok(x, GATConv(2, 16, 1, dropout_rate=0.0, activation="tanh"), "mean")
    assert not G.gat_pool_hip_ok(x, GATConv(2, 16, 2, concat_heads=False, dropout_rate=0.0), "mean")
    with pytest.raises(ValueError):
        G.gat_pool(x, torch.zeros(2, 64, 64), torch.ones(2, 64), None, None, drop.train(), "mean", time_major=True)


def test_case_table_covers_the_issue():
    names = {c.name for c in S.CASES}
    assert len(names) == len(S.CASES)
    assert {t for c in S.CASES for t in c.tags} == set(S.PREDICATES)
    hip = [c for c in S.CASES if "hip" in c.tags]
    assert {(c.Cin, c.C, c.H) for c in hip} >= {(2, 16, 1), (2, 8, 2), (2, 16, 2), (1, 8, 1), (3, 32, 1), (4, 16, 1)}
    assert {c.N for c in hip} >= {1, 7, 33, 64} and {c.pooling for c in hip} == {"mean", "sum", "selection"}
    assert {c.B for c in hip if c.tm} >= {5, 17} and any(not c.anom for c in hip)
    assert any((c.B, c.T, c.N) == (48, 181, 7) for c in hip)
    assert {c.N for c in S.CASES if "eager" in c.tags} >= {65} and any(c.pooling == "max" for c in S.CASES)


def test_pool_weights_are_pool_nodes():
    """sum_i gat_pool_weights[b, i] h[b, t, i] == pool_nodes(h * mask) for the three linear poolings."""
    d = S.reference("degenerate_mean")[1]
    h = torch.randn(5, 11, 9, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    m = d["mask"].double()
    for pooling in ("mean", "sum", "selection"):
        pw = G.gat_pool_weights(m, d["anom_pos"], pooling)
        want = G.pool_nodes(h * m[:, None, :, None], m, d["anom_pos"], pooling)
        assert (torch.einsum("bi,btik->btk", pw, h) - want).abs().max().item() < 1e-14
