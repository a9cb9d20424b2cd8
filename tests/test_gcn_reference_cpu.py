"""CPU part of the GeneralConv shape tests (``tests/test_gcn_shapes_gpu.py``): the float64 reference
itself is checked at the edges the GPU tests rely on, and every case of the GPU tables is checked
to still reach the kernel branch it names."""
import pytest
import torch

import test_gcn_shapes_gpu as S
from gnnqc.ops import gcn as G


def _act(d, training):
    """float64 activations a[b,t,j,f] = PReLU(BN(x W + b)) * mask (GeneralConv with an identity graph)."""
    B, N = d["mask"].shape
    eye = torch.eye(N, dtype=torch.float64).expand(B, N, N)
    return G.general_conv_eager(d["x"].double(), eye, d["mask"].double(), d["W"].double(), d["b"].double(),
                                d["gamma"].double(), d["beta"].double(), d["rm"].double().clone(),
                                d["rv"].double().clone(), d["alpha"].double(), training, "sum")


@pytest.mark.parametrize("degenerate", [False, True])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("aggregate", ["mean", "sum"])
@pytest.mark.parametrize("pooling", ["mean", "sum", "selection"])
def test_pooled_reference_two_ways_agree(pooling, aggregate, training, degenerate):
    """pool_nodes(general_conv_eager(...)) == sum_j node_pool_weights[b,j] act[b,t,j] in float64 to
    1e-12 on the GPU tests' input builder: random masks and flagged positions, a fully masked
    sample with anom_pos = -1, a sample with a single valid node."""
    gen = torch.Generator().manual_seed(17 + degenerate)
    d = S.gcn_inputs(gen, 6, 5, 9, 3, 8, degenerate=degenerate)
    if degenerate:
        assert d["mask"][0].sum() == 0 and d["anom_pos"][0] == -1 and d["mask"][1].sum() == 1
    assert all(d["mask"][b, d["anom_pos"][b]] == 1 for b in range(6) if d["anom_pos"][b] >= 0)
    one, _, _, _ = S.pooled_reference(dict(d, anom=None), pooling, aggregate, training)
    w = G.node_pool_weights(d["adj"].double(), d["mask"].double(), d["anom_pos"], aggregate, pooling)
    two = torch.einsum("bj,btjf->btf", w, _act(d, training))
    assert one.shape == two.shape == (6, 5, 8)
    assert (one.detach() - two).abs().max().item() < 1e-12
    if degenerate:
        assert torch.count_nonzero(one[0]) == 0          # nothing valid: the pooled row is zero


def test_builder_masks_are_not_forced():
    """The builder leaves node 0 masked in some samples and flags nodes other than node 0."""
    d = S.gcn_inputs(torch.Generator().manual_seed(1), 32, 2, 9, 2, 8)
    assert (d["mask"][:, 0] == 0).any() and (d["anom_pos"] > 0).any()
    assert (d["mask"].sum(1) >= 1).all()
    assert torch.equal(d["adj"], d["adj"].transpose(1, 2))
    assert S.gcn_inputs(torch.Generator().manual_seed(1), 3, 2, 4, 2, 8, anom=False)["anom"] is None


def test_node_builder_has_isolated_node_and_dense_row():
    d = S.node_inputs(torch.Generator().manual_seed(1), 2, 3, 33, 3, 16)
    assert d["mask"][0].sum() == 33 and d["mask"][1].sum() == 30
    assert d["adj"][0, 1].sum() == 0 and d["adj"][0, :, 1].sum() == 0
    assert d["adj"][0, 0].sum() == 32


@pytest.mark.parametrize("case", S.POOL_CASES, ids=[c.name for c in S.POOL_CASES])
def test_pool_case_reaches_its_branches(case):
    assert case.tags, case.name
    assert case.Cin <= 4 and case.F in (8, 16, 32)
    for tag in case.tags:
        assert S.POOL_PREDICATES[tag](case), f"{case.name} no longer reaches '{tag}'"
    # all tensors of a case stay small
    assert case.B * case.T * case.N * max(case.Cin, case.F) * 8 < 64 << 20


@pytest.mark.parametrize("case", S.NODE_CASES, ids=[c.name for c in S.NODE_CASES])
def test_node_case_reaches_its_branches(case):
    assert case.tags, case.name
    assert case.Cin <= 4 and 64 % case.F == 0
    for tag in case.tags:
        assert S.NODE_PREDICATES[tag](case), f"{case.name} no longer reaches '{tag}'"


def test_case_tables_cover_every_branch_family():
    """Every predicate is claimed by at least one case, and the issue's shapes are present."""
    pool_tags = {t for c in S.POOL_CASES for t in c.tags}
    node_tags = {t for c in S.NODE_CASES for t in c.tags}
    assert pool_tags == set(S.POOL_PREDICATES), set(S.POOL_PREDICATES) ^ pool_tags
    assert node_tags == set(S.NODE_PREDICATES), set(S.NODE_PREDICATES) ^ node_tags
    assert {(c.Cin, c.F) for c in S.POOL_CASES} >= {(1, 8), (3, 8), (4, 16), (1, 32), (4, 32), (2, 16)}
    assert {c.N * c.Cin for c in S.POOL_CASES} >= {12, 14, 48, 49, 52}
    assert {c.T * c.N for c in S.POOL_CASES} >= {1024, 1025, 2500}
    assert {c.B for c in S.POOL_CASES} >= {1, 257}
    assert {c.N for c in S.NODE_CASES} >= {31, 32, 33, 64, 65}
    assert {c.F for c in S.NODE_CASES} >= {1, 2, 4, 8, 32, 64} and {c.Cin for c in S.NODE_CASES} >= {1, 2, 4}
    assert len({c.name for c in S.POOL_CASES}) == len(S.POOL_CASES)
    assert len({c.name for c in S.NODE_CASES}) == len(S.NODE_CASES)
