"""GeneralConv kernels over their shape and dispatch space, against float64 eager on the CPU.

Three families, each compared with the project's own eager functions run in float64 (output,
every gradient by autograd on the float64 graph, and the BatchNorm running statistics):

* the pooled path (``gcn_prep`` -> ``gcn_pool_fwd`` ; ``gcn_pool_bwd`` -> ``gcn_bwd_finalize``
  -> ``gcn_pool_bwd_input``) through :func:`gnnqc.ops.gcn.gcn_pool`;
* the per-node path (``gcn_adj_bits``, ``gcn_stats``, ``gcn_bn_prep``, ``gcn_node_fwd / bwd /
  bwd_input``) through :func:`gnnqc.ops.gcn.gcn_node_tm`;
* the store-fused path (``gcn_fused_fwd / bwd``, ``gcn_coef_bwd``) through
  :func:`gnnqc.ops.gcn.gcn_pool_from_store`, against a CPU twin of the window store.

Every case of the tables below names the kernel branches it is there to reach (``tags``); the
predicates of those branches are recomputed from the shapes by ``tests/test_gcn_reference_cpu.py``
(no GPU needed), so a case that stops reaching its branch fails there. The constants the
predicates use mirror the ``.hip`` sources and are kept in one place (``K_*`` below).

The store-fused cases keep ``Cin = 2``: the store's feature count comes from the data set (the
session's synthetic CML windows have two features), so other ``Cin`` are not reachable there.
"""
import math
import os
from collections import namedtuple

import pytest
import torch

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------ constants of the kernels
K_STAGE_MAX = 48            # gcn.hip: GCN_STAGE_MAX (x floats per row staged in LDS)
K_FWD_RPB = 64              # gcn.hip gcn_pool_fwd_kernel: RPB (rows per workgroup and pass)
K_FWD_GRID_CAP = 8192       # gcn.hip gcn_pool_fwd host: grid_for(rows, 64, 8192)
K_BWD_THREADS = 256         # gcn.hip gcn_pool_bwd host: rows_per_blk = 256 / F
K_BWD_GRID_CAP = 512        # gcn.hip gcn_pool_bwd host: grid_for(B * T, rows_per_blk, 512)
K_BWD_XSLOTS = 6 * 256      # gcn.hip gcn_pool_bwd_kernel: XG * 256 prefetched x floats per pass
K_TWO_STAGE_R = 256         # gcn_glue.hip gcn_bwd_finalize host: R > 256 -> gcn_acc_colsum_kernel
K_WIDE_NCOL = 128           # gcn_glue.hip gcn_acc_colsum_kernel: ncol <= 128, else the wide branch
K_ADJ_LDS = 8192            # gcn_glue.hip: GLUE_ADJ_LDS (adjacency floats staged in LDS)
K_MOMENT_ROUND = 4 * 256    # gcn_glue.hip gcn_prep_kernel: moment loop, 4 rows x 256 threads a round
K_RECORD_ROUND = 256        # gcn_glue.hip gcn_prep_kernel: last arrival, one record per thread a round
K_NODE_STEPS = 1024         # gcn_node.hip node_geom: tchunk = min(tmax, B * T / 1024)
K_NODE_TMAX_FWD = 2         # gcn_node.hip node_geom: tdef = 2 (forward, input gradient)
K_NODE_TMAX_BWD = 4         # gcn_node.hip gcn_node_bwd host: node_geom(x, bitsT, W, 4)
# (gcn_pool_fwd only loops over passes past K_FWD_GRID_CAP * K_FWD_RPB = 524,288 rows: too large
# for a unit test, left out on purpose)


def _cdiv(a, b):
    return -(-a // b)


PoolCase = namedtuple("PoolCase", "name B T N Cin F pooling aggregate training tm anom degenerate tags")
NodeCase = namedtuple("NodeCase", "name B T N Cin F aggregate training tags")


def _pc(name, B, T, N, Cin, F, pooling="mean", aggregate="mean", training=True, tm=False, anom=True,
        degenerate=False, tags=()):
    return PoolCase(name, B, T, N, Cin, F, pooling, aggregate, training, tm, anom, degenerate, tuple(tags))


def _pool_cases():
    cs = []
    # dispatch: every (Cin, F) pair the models can reach, training and eval, two poolings
    for Cin, F in [(1, 8), (3, 8), (4, 16), (1, 32), (4, 32), (2, 16)]:
        for training in (True, False):
            for pooling in ("mean", "selection"):
                cs.append(_pc(f"dispatch_c{Cin}f{F}_{'train' if training else 'eval'}_{pooling}", 5, 11, 9, Cin, F,
                              pooling, training=training, tags=("staged",)))
    # staging of x rows in LDS
    cs += [
        _pc("stage_L12_vec4", 5, 11, 6, 2, 16, tags=("staged", "vec4", "zero_fill")),
        _pc("stage_L48_limit", 5, 13, 12, 4, 16, tags=("staged", "vec4", "zero_fill", "stage_limit",
                                                        "fwd_multi_block")),
        _pc("stage_L14_scalar", 5, 11, 7, 2, 16, tags=("staged", "scalar", "zero_fill")),
        _pc("stage_L49_unstaged", 5, 11, 49, 1, 16, tags=("unstaged",)),
        _pc("stage_L52_unstaged", 5, 11, 13, 4, 8, pooling="selection", tags=("unstaged",)),
    ]
    # the backward's prefetch registers exactly full, the node-weight slab at its largest
    cs += [
        _pc("prefetch_corner_T1", 70, 1, 48, 1, 8, tags=("staged", "prefetch_full", "slab_max")),
        _pc("prefetch_corner_T2", 70, 2, 48, 1, 8, pooling="selection", tags=("staged", "prefetch_full")),
    ]
    # several passes per workgroup (register prefetch one pass ahead) and the two-stage finalize
    cs += [
        _pc("multi_pass_f16", 48, 181, 7, 2, 16, tags=("staged", "multi_pass", "two_stage", "narrow_ncol")),
        _pc("multi_pass_f32_wide", 24, 181, 5, 4, 32, pooling="selection",
            tags=("staged", "multi_pass", "two_stage", "wide_ncol")),
    ]
    # gcn_prep
    cs += [
        _pc("prep_adj_global", 2, 3, 91, 1, 8, tags=("adj_global", "unstaged")),
        _pc("prep_adj_global_selection", 2, 3, 91, 1, 8, pooling="selection", aggregate="sum",
            tags=("adj_global", "unstaged")),
        _pc("prep_moments_1024", 2, 64, 16, 2, 16, tags=("moment_one_round",)),
        _pc("prep_moments_1025", 2, 25, 41, 1, 16, tags=("moment_rounds",)),
        _pc("prep_moments_2500", 2, 50, 50, 1, 8, tags=("moment_rounds", "unstaged")),
        _pc("prep_B1", 1, 11, 9, 2, 16, tags=("single_sample",)),
        _pc("prep_B257", 257, 3, 5, 2, 16, tags=("many_records",)),
    ]
    # masks: a sample with every node masked (anom_pos -1 there), a sample with one valid node
    for pooling in ("mean", "sum", "selection"):
        for aggregate in ("mean", "sum"):
            for training in (True, False):
                cs.append(_pc(f"masks_{pooling}_{aggregate}_{'train' if training else 'eval'}", 5, 11, 9, 2, 16,
                              pooling, aggregate, training, degenerate=True, tags=("staged", "degenerate")))
    # time-major output with padding rows and channels; the backward reads the time-major dout
    for training in (True, False):
        tr = "train" if training else "eval"
        cs += [
            _pc(f"tm_staged_{tr}", 21, 11, 9, 3, 16, training=training, tm=True,
                tags=("staged", "tm_pad_rows", "tm_pad_ch")),
            _pc(f"tm_unstaged_{tr}", 21, 11, 17, 3, 16, pooling="selection", training=training, tm=True,
                tags=("unstaged", "tm_pad_rows", "tm_pad_ch")),
        ]
    # no flagged series (Ca = 0)
    cs += [
        _pc("no_anom", 5, 11, 9, 2, 16, anom=False, tags=("staged", "no_anom")),
        _pc("no_anom_eval_sum", 5, 11, 9, 2, 16, pooling="sum", aggregate="sum", training=False, anom=False,
            tags=("staged", "no_anom")),
        _pc("no_anom_tm", 21, 11, 9, 2, 16, tm=True, anom=False, tags=("staged", "no_anom", "tm_pad_rows")),
    ]
    return cs


def _node_cases():
    cs = []

    def add(name, B, T, N, Cin, F, tags, aggs=("mean", "sum"), trains=(True, False)):
        for a in aggs:
            for tr in trains:
                cs.append(NodeCase(f"{name}_{a}_{'train' if tr else 'eval'}", B, T, N, Cin, F, a, tr, tuple(tags)))

    add("tchunk2_oddT", 8, 257, 6, 3, 16, ("tchunk2", "odd_T", "vec"))
    add("tchunk2_evenT", 8, 256, 6, 3, 16, ("tchunk2", "even_T", "vec"), aggs=("mean",))
    for N, tags in [(31, ("words1",)), (32, ("words1", "full_word")), (33, ("words2",)),
                    (64, ("words2", "full_word")), (65, ("words3",))]:
        add(f"words_N{N}", 2, 3, N, 3, 16, tags + ("vec",), trains=(True,))
    add("dispatch_c1f4", 2, 3, 33, 1, 4, ("vec",), aggs=("mean",))
    add("dispatch_c2f8", 2, 3, 33, 2, 8, ("vec",), aggs=("sum",))
    add("dispatch_c4f32", 2, 3, 33, 4, 32, ("vec",), aggs=("mean",))
    add("dispatch_c1f64_N65", 2, 3, 65, 1, 64, ("vec", "words3"), aggs=("mean",))
    add("dispatch_c4f64_N65", 2, 3, 65, 4, 64, ("vec", "words3"), aggs=("sum",), trains=(True,))
    add("dispatch_c2f1", 2, 3, 33, 2, 1, ("scalar",), aggs=("mean",))
    add("dispatch_c4f2", 2, 3, 33, 4, 2, ("scalar",), aggs=("sum",))
    add("finalize_two_stage_wide", 3, 100, 5, 3, 32, ("two_stage", "wide_ncol", "vec"), aggs=("mean",))
    return cs


POOL_CASES = _pool_cases()
NODE_CASES = _node_cases()
FUSED_F = (8, 16, 32)
FUSED_B = ((1, 0), (100, 4), (130, 0))      # (batch size, padded ids at its end)


def _time_major_pad(c):
    """(Mp, Cp) of gcn_pool(time_major=True) for a pooled case."""
    Ca = c.Cin if c.anom else 0
    Cp = Ca + c.F
    return _cdiv(c.B, 16) * 16, Cp + (-Cp) % 4


def node_tchunk(c, tmax):
    return max(1, min(tmax, (c.B * c.T) // K_NODE_STEPS))


# the branch each tag stands for, as a predicate of the case's shape
POOL_PREDICATES = {
    "staged": lambda c: c.N * c.Cin <= K_STAGE_MAX,
    "unstaged": lambda c: c.N * c.Cin > K_STAGE_MAX,
    "vec4": lambda c: c.N * c.Cin <= K_STAGE_MAX and (c.N * c.Cin) % 4 == 0,
    "scalar": lambda c: c.N * c.Cin <= K_STAGE_MAX and (c.N * c.Cin) % 4 != 0,
    "zero_fill": lambda c: c.N * c.Cin <= K_STAGE_MAX and (c.B * c.T) % K_FWD_RPB != 0,
    "stage_limit": lambda c: c.N * c.Cin == K_STAGE_MAX,
    "fwd_multi_block": lambda c: c.B * c.T > K_FWD_RPB,
    "prefetch_full": lambda c: c.N * c.Cin <= K_STAGE_MAX and (K_BWD_THREADS // c.F) * c.N * c.Cin == K_BWD_XSLOTS,
    "slab_max": lambda c: c.T == 1 and c.F == 8 and c.N == K_STAGE_MAX,
    "multi_pass": lambda c: c.N * c.Cin <= K_STAGE_MAX and c.B * c.T > K_BWD_GRID_CAP * (K_BWD_THREADS // c.F),
    "two_stage": lambda c: min(K_BWD_GRID_CAP, _cdiv(c.B * c.T, K_BWD_THREADS // c.F)) > K_TWO_STAGE_R,
    "wide_ncol": lambda c: (3 + c.Cin) * c.F > K_WIDE_NCOL,
    "narrow_ncol": lambda c: (3 + c.Cin) * c.F <= K_WIDE_NCOL,
    "adj_global": lambda c: c.N * c.N > K_ADJ_LDS,
    "moment_one_round": lambda c: c.T * c.N == K_MOMENT_ROUND,
    "moment_rounds": lambda c: c.T * c.N > K_MOMENT_ROUND and (c.T * c.N) % K_MOMENT_ROUND != 0,
    "single_sample": lambda c: c.B == 1,
    "many_records": lambda c: c.B > K_RECORD_ROUND,
    "degenerate": lambda c: c.degenerate and c.B >= 3,
    "tm_pad_rows": lambda c: c.tm and _time_major_pad(c)[0] > c.B,
    "tm_pad_ch": lambda c: c.tm and _time_major_pad(c)[1] > (c.Cin if c.anom else 0) + c.F,
    "no_anom": lambda c: not c.anom,
}
NODE_PREDICATES = {
    "tchunk2": lambda c: (c.B * c.T) // K_NODE_STEPS >= 2 and node_tchunk(c, K_NODE_TMAX_FWD) == 2,
    "odd_T": lambda c: c.T % 2 == 1,
    "even_T": lambda c: c.T % 2 == 0,
    "words1": lambda c: _cdiv(c.N, 32) == 1,
    "words2": lambda c: _cdiv(c.N, 32) == 2,
    "words3": lambda c: _cdiv(c.N, 32) == 3,
    "full_word": lambda c: c.N % 32 == 0,
    "vec": lambda c: c.F % 4 == 0,
    "scalar": lambda c: c.F % 4 != 0,
    "two_stage": lambda c: c.B * _cdiv(c.T, node_tchunk(c, K_NODE_TMAX_BWD)) > K_TWO_STAGE_R,
    "wide_ncol": lambda c: (3 + c.Cin) * c.F > K_WIDE_NCOL,
}


# ------------------------------------------------------------------ input builders (CPU, float32)
def _params(gen, Cin, F):
    return dict(W=torch.randn(Cin, F, generator=gen) * 0.5, b=torch.randn(F, generator=gen) * 0.1,
                gamma=1 + 0.1 * torch.randn(F, generator=gen), beta=0.1 * torch.randn(F, generator=gen),
                alpha=0.2 * torch.rand(F, generator=gen), rm=0.1 * torch.randn(F, generator=gen),
                rv=0.5 + 1.5 * torch.rand(F, generator=gen))


def gcn_inputs(gen, B, T, N, Cin, F, anom=True, degenerate=False):
    """Inputs of the pooled path on the CPU: random masks (no node forced valid, but every sample
    keeps at least one), ``anom_pos`` drawn among each sample's valid nodes, symmetric adjacency with
    self loops restricted to valid nodes, ``anom=None`` on request. ``degenerate`` (B >= 3): sample 0
    has every node masked and ``anom_pos = -1`` (a padded sample), sample 1 a single valid node."""
    x = torch.randn(B, T, N, Cin, generator=gen)
    mask = (torch.rand(B, N, generator=gen) > 0.25).float()
    for b in range(B):
        if mask[b].sum() == 0:
            mask[b, int(torch.randint(N, (1,), generator=gen))] = 1
    if degenerate:
        assert B >= 3
        mask[0] = 0
        mask[1] = 0
        mask[1, int(torch.randint(N, (1,), generator=gen))] = 1
    adj = (torch.rand(B, N, N, generator=gen) > 0.5).float()
    adj = ((adj + adj.transpose(1, 2)) > 0).float() + torch.eye(N)
    adj = (adj > 0).float() * mask[:, :, None] * mask[:, None, :]
    x = x * mask[:, None, :, None]
    anom_pos = torch.full((B,), -1, dtype=torch.long)
    for b in range(B):
        valid = mask[b].nonzero().flatten()
        if valid.numel():
            anom_pos[b] = valid[int(torch.randint(valid.numel(), (1,), generator=gen))]
    d = dict(x=x, adj=adj, mask=mask, anom=torch.randn(B, T, Cin, generator=gen) if anom else None,
             anom_pos=anom_pos)
    d.update(_params(gen, Cin, F))
    return d


def node_inputs(gen, B, T, N, Cin, F):
    """Inputs of the per-node path: sample b keeps its first ``N - 3 b`` nodes (sample 0 is full, so
    ``N % 32 == 0`` gives an exactly full last bit word), sparse symmetric graphs with self loops;
    in sample 0, node 0 is connected to every valid node (a dense row) and node 1 to none, not even
    itself (an isolated valid node: row scale 0 under mean aggregation)."""
    adj = torch.zeros(B, N, N)
    mask = torch.zeros(B, N)
    for b in range(B):
        nv = max(2, N - 3 * b)
        mask[b, :nv] = 1
        a = (torch.rand(nv, nv, generator=gen) < 0.2).float()
        a = ((a + a.t()) > 0).float()
        a.fill_diagonal_(1.0)
        adj[b, :nv, :nv] = a
    adj[0, 0, :] = mask[0]
    adj[0, :, 0] = mask[0]
    adj[0, 1, :] = 0
    adj[0, :, 1] = 0
    x = torch.randn(B, T, N, Cin, generator=gen) * mask[:, None, :, None]
    d = dict(x=x, adj=adj, mask=mask)
    d.update(_params(gen, Cin, F))
    return d


# ------------------------------------------------------------------ float64 references (CPU)
_GRAD_NAMES = ("W", "b", "gamma", "beta", "alpha")


def pooled_reference(d, pooling, aggregate, training):
    """float64 eager: ``(out [B,T,Ca+F], leaves, running mean, running variance)``."""
    from gnnqc.ops import gcn as G
    leaves = {k: d[k].double().clone().requires_grad_(True) for k in ("x",) + _GRAD_NAMES}
    if d["anom"] is not None:
        leaves["anom"] = d["anom"].double().clone().requires_grad_(True)
    rm, rv = d["rm"].double().clone(), d["rv"].double().clone()
    h = G.general_conv_eager(leaves["x"], d["adj"].double(), d["mask"].double(), leaves["W"], leaves["b"],
                             leaves["gamma"], leaves["beta"], rm, rv, leaves["alpha"], training, aggregate)
    pooled = G.pool_nodes(h, d["mask"].double(), d["anom_pos"], pooling)
    out = pooled if d["anom"] is None else torch.cat([leaves["anom"], pooled], -1)
    return out, leaves, rm, rv


def _assert_grads(got, leaves, what):
    """The pooled path's gradient bound: |err| < 2e-3 (1 + max |ref|)."""
    for name, r in leaves.items():
        ref = r.grad if r.grad is not None else torch.zeros_like(r)
        g = got[name]
        g = torch.zeros_like(ref) if g is None else g.detach().double().cpu()
        assert g.shape == ref.shape, (what, name, g.shape, ref.shape)
        err = (g - ref).abs().max().item()
        bound = 2e-3 * (1 + ref.abs().max().item())
        assert err < bound, f"{what}: d{name} err {err:.3e} >= {bound:.3e}"


# ------------------------------------------------------------------ 1. pooled path
def _run_pooled(dev, c, d):
    """gcn_pool on the device: (out, B or None, leaves, running mean, running variance)."""
    from gnnqc.ops import gcn as G
    leaves = {k: d[k].to(dev).clone().requires_grad_(True) for k in ("x",) + _GRAD_NAMES}
    anom = None
    if d["anom"] is not None:
        anom = leaves["anom"] = d["anom"].to(dev).clone().requires_grad_(True)
    rm, rv = d["rm"].to(dev).clone(), d["rv"].to(dev).clone()
    assert G.gcn_pool_hip_ok(leaves["x"], leaves["W"], c.aggregate, c.pooling, 0.0, c.training)
    out = G.gcn_pool(leaves["x"], d["adj"].to(dev), d["mask"].to(dev), anom, d["anom_pos"].to(dev), leaves["W"],
                     leaves["b"], leaves["gamma"], leaves["beta"], leaves["alpha"], rm, rv, c.training, c.aggregate,
                     c.pooling, time_major=c.tm)
    return out, leaves, rm, rv


@pytest.mark.parametrize("case", POOL_CASES, ids=[c.name for c in POOL_CASES])
def test_gcn_pool_case_matches_float64(cuda_device, case):
    """Output, dx, danom, dW, db, dgamma, dbeta, dalpha and the running statistics of one pooled
    case against float64 eager; time-major cases: padding rows and channels exactly zero."""
    c = case
    gen = torch.Generator().manual_seed(1000 + POOL_CASES.index(c))
    d = gcn_inputs(gen, c.B, c.T, c.N, c.Cin, c.F, c.anom, c.degenerate)
    if c.degenerate:
        assert d["mask"][0].sum() == 0 and d["anom_pos"][0] == -1 and d["mask"][1].sum() == 1
    ref, rleaves, rrm, rrv = pooled_reference(d, c.pooling, c.aggregate, c.training)
    out, leaves, rm, rv = _run_pooled(cuda_device, c, d)
    Fo = ref.shape[-1]
    if c.tm:
        out, Bret = out
        Mp, Cp = _time_major_pad(c)
        assert Bret == c.B and tuple(out.shape) == (c.T, Mp, Cp)
        o = out.detach().double().cpu()
        assert torch.count_nonzero(o[:, c.B:]) == 0, "time-major padding rows"
        assert torch.count_nonzero(o[:, :, Fo:]) == 0, "time-major padding channels"
        got = o[:, :c.B, :Fo].transpose(0, 1)
    else:
        assert tuple(out.shape) == (c.B, c.T, Fo)
        got = out.detach().double().cpu()
    err = (got - ref.detach()).abs().max().item()
    assert torch.allclose(got, ref.detach(), atol=1e-4, rtol=1e-4), f"{c.name}: output err {err:.3e}"
    if c.training:
        torch.testing.assert_close(rm.double().cpu(), rrm, atol=1e-5, rtol=1e-4)
        torch.testing.assert_close(rv.double().cpu(), rrv, atol=1e-5, rtol=1e-4)
    else:
        assert torch.equal(rm.cpu(), d["rm"]) and torch.equal(rv.cpu(), d["rv"])
    g = torch.randn(out.shape, generator=gen)            # (padding rows / channels included)
    out.backward(g.to(cuda_device))
    gref = g[:, :c.B, :Fo].transpose(0, 1) if c.tm else g
    ref.backward(gref.double())
    _assert_grads({k: v.grad for k, v in leaves.items()}, rleaves, c.name)


def test_gcn_prep_many_records_twice_bitwise(cuda_device):
    """B = 257: the last-arriving workgroup's record loop takes two rounds, and the arrival counter
    is persistent: a second launch right after the first gives bitwise-equal w, S, st."""
    from gnnqc.utils.native import hip_ops
    c = next(c for c in POOL_CASES if c.name == "prep_B257")
    d = gcn_inputs(torch.Generator().manual_seed(7), c.B, c.T, c.N, c.Cin, c.F)
    dev = cuda_device
    t = {k: v.to(dev) for k, v in d.items() if v is not None}
    outs = []
    for _ in range(2):
        rm, rv = t["rm"].clone(), t["rv"].clone()
        w, S, st = hip_ops().gcn_prep(t["x"], t["adj"], t["mask"], t["anom_pos"], True, 2, t["W"], t["b"], t["gamma"],
                                      t["beta"], rm, rv, True, 0.99, 1e-3)
        outs.append([v.clone() for v in (w, S, st, rm, rv)])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    from gnnqc.ops.gcn import node_pool_weights
    wref = node_pool_weights(d["adj"].double(), d["mask"].double(), d["anom_pos"], "mean", "selection")
    torch.testing.assert_close(outs[0][0].double().cpu(), wref, atol=1e-6, rtol=1e-6)


def test_gcn_pool_five_channels_takes_eager_path(cuda_device):
    """gcn_prep handles 1..4 input channels; with Cin = 5 gcn_pool() must use the eager path on the
    device (it used to pass the gate and raise inside gcn_prep)."""
    from gnnqc.ops import gcn as G
    c = _pc("cin5", 5, 11, 9, 5, 16)
    gen = torch.Generator().manual_seed(55)
    d = gcn_inputs(gen, c.B, c.T, c.N, c.Cin, c.F)
    dev = cuda_device
    assert not G.gcn_pool_hip_ok(d["x"].to(dev), d["W"].to(dev), "mean", "mean", 0.0, True)
    assert G.gcn_pool_hip_ok(d["x"][..., :4].to(dev), d["W"][:4].to(dev), "mean", "mean", 0.0, True)
    ref, rleaves, rrm, rrv = pooled_reference(d, c.pooling, c.aggregate, True)
    leaves = {k: d[k].to(dev).clone().requires_grad_(True) for k in ("x", "anom") + _GRAD_NAMES}
    rm, rv = d["rm"].to(dev).clone(), d["rv"].to(dev).clone()
    out = G.gcn_pool(leaves["x"], d["adj"].to(dev), d["mask"].to(dev), leaves["anom"], d["anom_pos"].to(dev),
                     leaves["W"], leaves["b"], leaves["gamma"], leaves["beta"], leaves["alpha"], rm, rv, True)
    assert out.is_cuda and tuple(out.shape) == tuple(ref.shape)
    assert torch.allclose(out.detach().double().cpu(), ref.detach(), atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(rm.double().cpu(), rrm, atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(rv.double().cpu(), rrv, atol=1e-5, rtol=1e-4)
    g = torch.randn(out.shape, generator=gen)
    out.backward(g.to(dev))
    ref.backward(g.double())
    _assert_grads({k: v.grad for k, v in leaves.items()}, rleaves, c.name)


# ------------------------------------------------------------------ 2. per-node path
@pytest.mark.parametrize("case", NODE_CASES, ids=[c.name for c in NODE_CASES])
def test_gcn_node_case_matches_float64(cuda_device, case):
    """Time-major output (2e-4), running statistics and every gradient (relative max error 1e-3)
    of one per-node case against float64 ``gcn_node_tm_eager``."""
    from gnnqc.ops.gcn import gcn_node_tm, gcn_node_tm_eager, gcn_node_tm_ok
    c = case
    if "tchunk2" in c.tags and os.environ.get("GNNQC_NODE_TCHUNK"):
        pytest.skip("GNNQC_NODE_TCHUNK is set: node_geom reads it once per process, the chunk is not the default")
    dev = cuda_device
    gen = torch.Generator().manual_seed(2000 + NODE_CASES.index(c))
    d = node_inputs(gen, c.B, c.T, c.N, c.Cin, c.F)
    assert d["adj"][0, 1].sum() == 0 and d["mask"][0, 1] == 1            # isolated valid node
    assert d["adj"][0, 0].sum() == d["mask"][0].sum() - 1                 # dense row (all but the isolated node)
    names = ("x",) + _GRAD_NAMES
    ps = {k: d[k].to(dev).clone().requires_grad_(True) for k in names}
    rps = {k: d[k].double().clone().requires_grad_(True) for k in names}
    rm, rv = d["rm"].to(dev).clone(), d["rv"].to(dev).clone()
    rrm, rrv = d["rm"].double().clone(), d["rv"].double().clone()
    assert gcn_node_tm_ok(ps["x"], ps["W"], c.aggregate, 0.0, c.training)
    h, M = gcn_node_tm(ps["x"], d["adj"].to(dev), d["mask"].to(dev), ps["W"], ps["b"], ps["gamma"], ps["beta"],
                       ps["alpha"], rm, rv, c.training, c.aggregate)
    ref, Mr = gcn_node_tm_eager(rps["x"], d["adj"].double(), d["mask"].double(), rps["W"], rps["b"], rps["gamma"],
                                rps["beta"], rps["alpha"], rrm, rrv, c.training, c.aggregate)
    assert M == Mr == c.B * c.N and h.shape == ref.shape, (h.shape, ref.shape)
    torch.testing.assert_close(h.detach().double().cpu(), ref.detach(), atol=2e-4, rtol=2e-4)
    assert torch.count_nonzero(h[:, M:]) == 0 and torch.count_nonzero(h[:, :, c.F + c.Cin:]) == 0
    torch.testing.assert_close(rm.double().cpu(), rrm, atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(rv.double().cpu(), rrv, atol=1e-5, rtol=1e-5)
    g = torch.randn(ref.shape, generator=gen)
    g[:, M:] = 0
    h.backward(g.to(dev))
    ref.backward(g.double())
    for name in names:
        r = rps[name].grad
        if r is None:
            continue
        got = ps[name].grad
        got = torch.zeros_like(r) if got is None else got.double().cpu()
        err = (got - r).abs().max().item()
        scale = r.abs().max().item() + 1e-6
        assert err / scale < 1e-3, f"{c.name}: d{name} rel err {err / scale:.3e}"


# ------------------------------------------------------------------ 3. store-fused path
@pytest.fixture(scope="module")
def cml_stores(cuda_device, cml_windows):
    """The session's CML windows resident on the device, and a CPU twin of the same store."""
    from gnnqc.data.store import DeviceStore
    pc, ws = cml_windows
    dev_store = DeviceStore(ws, "rolling_median", pc.graph, device=cuda_device)
    cpu_store = DeviceStore(ws, "rolling_median", pc.graph, device="cpu")
    assert dev_store.n_feat == 2 and dev_store.n_windows >= max(b for b, _ in FUSED_B)
    return dev_store, cpu_store


def _fused_ids(store, B, pad):
    ids = torch.randperm(store.n_windows, generator=torch.Generator().manual_seed(3))[:B]
    if pad:
        ids[-pad:] = -1
    return ids


def _fused_layer(F, aggregate, seed):
    """GeneralConv(2, F) with every parameter and both running statistics randomised (CPU)."""
    from gnnqc.models.graphconv import GeneralConv
    torch.manual_seed(seed)
    g = GeneralConv(2, F, aggregate=aggregate)
    with torch.no_grad():
        g.bn_gamma.uniform_(0.5, 1.5)
        g.bn_beta.normal_(0, 0.2)
        g.prelu_alpha.uniform_(0.0, 0.4)
        g.bias.normal_(0, 0.1)
        g.bn_moving_mean.normal_(0, 0.1)
        g.bn_moving_variance.uniform_(0.5, 2.0)
    return g


def _fused_reference(layer, batch, training):
    """float64 eager per-node output h [B,T,N,F] of ``layer`` on a CPU batch, its float64 leaves
    and the float64 running statistics after the call."""
    from gnnqc.ops import gcn as G
    x, anom, adj, mask, ap = batch.model_inputs("cml")
    names = ("kernel", "bias", "bn_gamma", "bn_beta", "prelu_alpha")
    leaves = {n: getattr(layer, n).detach().double().clone().requires_grad_(True) for n in names}
    rm, rv = layer.bn_moving_mean.double().clone(), layer.bn_moving_variance.double().clone()
    h = G.general_conv_eager(x.double(), adj.double(), mask.double(), leaves["kernel"], leaves["bias"],
                             leaves["bn_gamma"], leaves["bn_beta"], rm, rv, leaves["prelu_alpha"], training,
                             layer.aggregate, 0.0, layer.momentum, layer.eps)
    return h, leaves, rm, rv


def _fused_check_forward(dev_store, layer, ids, batch, h64, rm64, rv64, training, pooling, dev):
    import copy

    from gnnqc.ops import gcn as G
    x, anom, adj, mask, ap = batch.model_inputs("cml")
    B, T = x.shape[0], x.shape[1]
    F = layer.channels
    g = copy.deepcopy(layer).to(dev)
    assert G.store_gcn_ok(dev_store, g, training, pooling)
    with torch.no_grad():
        h, M, y, ym, wid = G.gcn_pool_from_store(dev_store, ids.to(dev), g, training, pooling)
    torch.cuda.synchronize()
    Mp, Cp = _cdiv(B, 16) * 16, 2 + F + (-(2 + F)) % 4
    assert M == B and tuple(h.shape) == (T, Mp, Cp)
    ref = torch.cat([anom.double(), G.pool_nodes(h64, mask.double(), ap, pooling)], -1)       # [B, T, 2 + F]
    o = h.double().cpu()
    assert torch.count_nonzero(o[:, B:]) == 0 and torch.count_nonzero(o[:, :, 2 + F:]) == 0, "padding not zero"
    got = o[:, :B, :2 + F].transpose(0, 1)
    err = (got - ref).abs().max().item()
    assert torch.allclose(got, ref, atol=1e-4, rtol=1e-4), f"{pooling}: output err {err:.3e}"
    torch.testing.assert_close(y.cpu(), batch.y)
    torch.testing.assert_close(ym.cpu(), batch.y_mask)
    assert torch.equal(wid.cpu(), ids)
    if training:
        torch.testing.assert_close(g.bn_moving_mean.double().cpu(), rm64, atol=1e-5, rtol=1e-4)
        torch.testing.assert_close(g.bn_moving_variance.double().cpu(), rv64, atol=1e-5, rtol=1e-4)
    else:
        assert torch.equal(g.bn_moving_mean.cpu(), layer.bn_moving_mean)
        assert torch.equal(g.bn_moving_variance.cpu(), layer.bn_moving_variance)


@pytest.mark.parametrize("B,pad", FUSED_B)
@pytest.mark.parametrize("aggregate", ["mean", "sum"])
@pytest.mark.parametrize("F", FUSED_F)
def test_fused_forward_matches_float64(cuda_device, cml_stores, F, aggregate, B, pad):
    """gcn_pool_from_store (training mode) against float64 eager on the CPU twin's batch, for the
    three poolings (they share one float64 per-node reference): h on valid rows and channels,
    padding exactly zero, y, y_mask, wid and the running statistics."""
    dev_store, cpu_store = cml_stores
    ids = _fused_ids(cpu_store, B, pad)
    batch = cpu_store.gather(ids)
    layer = _fused_layer(F, aggregate, seed=F + B)
    with torch.no_grad():
        h64, _, rm64, rv64 = _fused_reference(layer, batch, True)
    for pooling in ("mean", "sum", "selection"):
        _fused_check_forward(dev_store, layer, ids, batch, h64, rm64, rv64, True, pooling, cuda_device)


@pytest.mark.parametrize("F", FUSED_F)
def test_fused_forward_eval_matches_float64(cuda_device, cml_stores, F):
    """The same in eval mode (BatchNorm from the running statistics, which stay untouched)."""
    dev_store, cpu_store = cml_stores
    ids = _fused_ids(cpu_store, 100, 4)
    batch = cpu_store.gather(ids)
    layer = _fused_layer(F, "mean", seed=F)
    with torch.no_grad():
        h64, _, rm64, rv64 = _fused_reference(layer, batch, False)
    for pooling in ("mean", "sum", "selection"):
        _fused_check_forward(dev_store, layer, ids, batch, h64, rm64, rv64, False, pooling, cuda_device)


@pytest.mark.parametrize("pooling", ["mean", "selection"])
@pytest.mark.parametrize("F,coef", [(8, "1"), (32, "1"), (16, "1"), (16, "0")])
def test_fused_gradients_match_float64(cuda_device, cml_stores, monkeypatch, F, coef, pooling):
    """Training gradients of W, b, gamma, beta, alpha of the store-fused backward against autograd
    on the float64 graph. F = 8 / 32: gcn_fused_bwd (no coefficient form exists there); F = 16: the
    coefficient form (GNNQC_GCN_COEF=1) and the recomputing form (=0)."""
    import copy

    from gnnqc.ops import gcn as G
    monkeypatch.setenv("GNNQC_GCN_COEF", coef)
    dev = cuda_device
    dev_store, cpu_store = cml_stores
    B, pad = 100, 4
    ids = _fused_ids(cpu_store, B, pad)
    batch = cpu_store.gather(ids)
    layer = _fused_layer(F, "mean", seed=100 + F)
    h64, leaves, _, _ = _fused_reference(layer, batch, True)
    x, anom, adj, mask, ap = batch.model_inputs("cml")
    ref = G.pool_nodes(h64, mask.double(), ap, pooling)                   # [B, T, F]
    g = copy.deepcopy(layer).to(dev)
    h, M, _, _, _ = G.gcn_pool_from_store(dev_store, ids.to(dev), g, True, pooling)
    dh = torch.randn(h.shape, generator=torch.Generator().manual_seed(5))   # (padding included)
    h.backward(dh.to(dev))
    torch.cuda.synchronize()
    ref.backward(dh[:, :B, 2:2 + F].transpose(0, 1).double())
    names = {"kernel": "W", "bias": "b", "bn_gamma": "gamma", "bn_beta": "beta", "prelu_alpha": "alpha"}
    got = {names[n]: getattr(g, n).grad for n in names}
    _assert_grads(got, {names[n]: leaves[n] for n in names}, f"fused F={F} coef={coef} {pooling}")
    assert got["W"] is not None and got["gamma"] is not None and got["alpha"] is not None
