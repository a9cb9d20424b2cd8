"""The per-node GATConv kernels (``csrc/kernels/gat_node.hip``) over their shape and dispatch space,
against the float64 eager layer on the CPU.

Every case runs :func:`gnnqc.ops.gcn.gat_node_tm` on the device and compares the time-major output
``[T, Mp, Cp]``, ``dx`` and every parameter gradient (``dW``, ``da_s``, ``da_n``, ``dbias``,
``dalpha``) with the eager layer, ``cat([h, x])``, permute and pad in float64
(:func:`gnnqc.ops.gcn.gat_node_tm_eager`, autograd on the float64 graph). Padding rows and padding
channels of the output must be exactly zero.

The bound convention is that of ``tests/test_gat_kernels_gpu.py`` (its module docstring gives the
reasoning): per case and quantity ``bound = max(4 x e32, floor)``, where ``e32`` is the error of
the SAME eager layer run in float32 on the CPU against the float64 oracle, and the floor is
``1e-4 + 1e-4 |ref|`` per output element and ``1e-3 max|ref|`` on a gradient.

Each case names the branches it is there to reach (``tags``); ``tests/test_gat_node_reference_cpu.py``
recomputes their predicates from the shapes, checks the kernel's math in float64 against the oracle
and checks that named mutants of that math lie at least 5 bounds away.

With ``GNNQC_GAT_NODE_REPORT=<path>`` the measured error, e32 and bound of every case and quantity
are written there (``profiles/gat_node_kernel_tests.txt`` is such a run).
"""
import copy
import functools
import os
from collections import namedtuple

import pytest
import torch

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------ constants of the kernels
K_MAX_N = 256               # gat_node.hip GATN_MAX_N (four 64-bit neighbour mask words per node)
K_THREADS = 256             # gat_node.hip: lanes per workgroup; rows per workgroup = 256 / pow2(N)
# gat_node.hip GATN_*_WGS: workgroups per launch (more row blocks: several passes per workgroup)
K_GRID_CAP = {"fwd": 2048, "bwd_input": 1024, "bwd": 512}
K_WIDTHS = ((8, 16, 32), (1, 2))      # gat_common.h GQ_GAT_DISPATCH: C, H
K_FLOOR_MULT = 4.0          # allowed kernel error / float32 eager error
OUT_ATOL = OUT_RTOL = 1e-4  # the floor on outputs
GRAD_REL = 1e-3             # the floor on gradients, relative to max |ref|

NodeCase = namedtuple("NodeCase", "name B T N Cin C H training dropout act kind xscale adj tags")


def _nc(name, B=3, T=5, N=9, Cin=3, C=16, H=1, training=True, dropout=0.0, act="prelu", kind="", xscale=1.0,
        adj="sparse", tags=()):
    return NodeCase(name, B, T, N, Cin, C, H, training, dropout, act, kind, xscale, adj, tuple(tags))


def _cases():
    cs = [
        # node counts: word boundaries, NP > N, the limit; B*N a multiple of 16 and not
        _nc("nodes_1", N=1, T=11, tags=("hip", "words_1", "single_node", "pad_rows", "wide_wg")),
        _nc("nodes_7", N=7, T=11, tags=("hip", "words_1", "np_gt_n", "pad_rows", "wide_wg", "ragged_rows")),
        _nc("nodes_33", N=33, T=11, H=2, C=8, tags=("hip", "words_1", "np_gt_n", "pad_rows")),
        _nc("nodes_64", N=64, B=2, tags=("hip", "words_1", "no_pad_rows", "ragged_rows")),
        _nc("nodes_65", N=65, tags=("hip", "words_2", "np_gt_n", "pad_rows", "ragged_rows")),
        _nc("nodes_128", N=128, B=2, tags=("hip", "words_2", "no_pad_rows")),
        _nc("nodes_129", N=129, tags=("hip", "words_3", "np_gt_n", "pad_rows", "one_row_wg")),
        _nc("nodes_210", N=210, B=2, tags=("hip", "words_4", "np_gt_n", "pad_rows", "one_row_wg")),
        _nc("nodes_256_dense", N=256, B=2, T=3, adj="dense",
            tags=("hip", "words_4", "limit", "dense", "no_pad_rows", "one_row_wg")),
        _nc("nodes_210_dense_h2", N=210, B=2, T=3, H=2, C=8, adj="dense", tags=("hip", "words_4", "dense")),
    ]
    # input widths (Cp with and without padding channels) and every (C, H) instance once
    for Cin, C, H in [(3, 16, 1), (1, 8, 1), (4, 32, 1), (3, 8, 2), (4, 16, 2), (1, 32, 2)]:
        pad = (H * C + Cin) % 4 != 0
        cs.append(_nc(f"dispatch_c{Cin}f{C}h{H}", N=70, B=2, T=7, Cin=Cin, C=C, H=H,
                      tags=("hip", "words_2", "np_gt_n", "pad_ch" if pad else "no_pad_ch")))
    cs += [
        # more row blocks than the grid caps. The caps are 2048 / 1024 / 512 workgroups (forward, input
        # backward, parameter backward), and the float64 oracle's [B, T, N, N, H] edge tensor has to stay
        # below 64 MB, so B = 3, T = 100, N = 130 (300 row blocks) takes one pass: the record-writing
        # backward is multi-pass at two mask words (N = 65: 513 blocks of two rows), all three kernels
        # at N = 5 (2054 blocks of 32 rows, the last one ragged)
        _nc("rows_300_n130", B=3, T=100, N=130, tags=("hip", "one_pass", "words_3", "one_row_wg")),
        _nc("passes", B=3, T=342, N=65, tags=("hip", "multi_pass_bwd", "words_2", "np_gt_n")),
        _nc("passes_small_n", B=3, T=21900, N=5, Cin=2,
            tags=("hip", "multi_pass_bwd", "multi_pass_all", "wide_wg", "ragged_rows")),
        _nc("degenerate", N=70, T=7, kind="degenerate", tags=("hip", "degenerate", "words_2")),
        _nc("degenerate_h2_relu", N=130, T=5, H=2, C=8, act="relu", kind="degenerate",
            tags=("hip", "degenerate", "words_3", "act_relu")),
        _nc("scores_x30", N=70, T=7, kind="scores", xscale=30.0, tags=("hip", "large_scores")),
        _nc("scores_equal", N=70, T=7, kind="equal", tags=("hip", "equal_scores")),
        _nc("act_linear", N=70, T=7, act=None, tags=("hip", "act_linear")),
        _nc("act_relu", N=70, T=7, act="relu", tags=("hip", "act_relu")),
        _nc("eval_dropout", N=70, T=7, training=False, dropout=0.5, tags=("hip", "eval_dropout")),
        # not on the HIP path: gat_node_tm_ok is false and gat_node_tm raises
        _nc("off_nodes_257", B=2, T=3, N=257, tags=("off_hip",)),
        _nc("off_train_dropout", N=9, dropout=0.5, tags=("off_hip",)),
    ]
    return cs


CASES = _cases()
HIP_CASES = [c.name for c in CASES if "hip" in c.tags]
OFF_CASES = [c.name for c in CASES if "off_hip" in c.tags]


def _cdiv(a, b):
    return -(-a // b)


def _pow2(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def rows_per_workgroup(c):
    return K_THREADS // _pow2(c.N)


def row_blocks(c):
    return _cdiv(c.B * c.T, rows_per_workgroup(c))


def time_major_pad(c):
    """(M, Mp, Cp) of gat_node_tm."""
    Cp = c.H * c.C + c.Cin
    return c.B * c.N, _cdiv(c.B * c.N, 16) * 16, Cp + (-Cp) % 4


def on_hip_path(c):
    """The conditions of gat_node_tm_ok, from the case's shape alone."""
    return (c.N <= K_MAX_N and c.Cin <= 4 and not (c.dropout > 0 and c.training) and c.C in K_WIDTHS[0]
            and c.H in K_WIDTHS[1] and c.act in (None, "linear", "prelu", "relu"))


def _words(n):
    return lambda c: _cdiv(c.N, 64) == n


PREDICATES = {
    "hip": on_hip_path,
    "off_hip": lambda c: not on_hip_path(c),
    "words_1": _words(1), "words_2": _words(2), "words_3": _words(3), "words_4": _words(4),
    "np_gt_n": lambda c: _pow2(c.N) > c.N,
    "single_node": lambda c: c.N == 1,
    "limit": lambda c: c.N == K_MAX_N,
    "one_row_wg": lambda c: rows_per_workgroup(c) == 1,
    "wide_wg": lambda c: rows_per_workgroup(c) >= 32,
    "one_pass": lambda c: row_blocks(c) <= min(K_GRID_CAP.values()),
    "multi_pass_bwd": lambda c: row_blocks(c) > K_GRID_CAP["bwd"],
    "multi_pass_all": lambda c: row_blocks(c) > max(K_GRID_CAP.values()),
    "ragged_rows": lambda c: (c.B * c.T) % rows_per_workgroup(c) != 0,
    "pad_rows": lambda c: time_major_pad(c)[1] > c.B * c.N,
    "no_pad_rows": lambda c: time_major_pad(c)[1] == c.B * c.N,
    "pad_ch": lambda c: time_major_pad(c)[2] > c.H * c.C + c.Cin,
    "no_pad_ch": lambda c: time_major_pad(c)[2] == c.H * c.C + c.Cin,
    "dense": lambda c: c.adj == "dense",
    "degenerate": lambda c: c.kind == "degenerate" and c.B >= 3,
    "large_scores": lambda c: c.kind == "scores" and c.xscale >= 30,
    "equal_scores": lambda c: c.kind == "equal",
    "eval_dropout": lambda c: not c.training and c.dropout > 0,
    "act_linear": lambda c: c.act in (None, "linear"),
    "act_relu": lambda c: c.act == "relu",
}


# ------------------------------------------------------------------ input builder (CPU, float32)
def node_inputs(c):
    """Inputs and the layer of a case on the CPU. Random masks (every sample keeps a node), a
    symmetric adjacency between valid nodes - ``sparse``: about 8 neighbours per node, ``dense``: all
    ones - whose diagonal is set only in every other sample (the layer adds the self loops).
    ``kind``:

    * ``degenerate``: sample 0 has every node masked, sample 1 a single valid node, sample 2 a valid
      node (3) without any edge, and every padded node holds 123.0 (with the neighbour attention
      kernel oriented so that such a row would dominate a softmax it was let into);
    * ``scores``: ``x`` times ``xscale`` (scores beyond float32's exp range without the max);
    * ``equal``: all nodes of a (sample, step) share one feature vector (all scores equal).
    """
    from gnnqc.models.graphconv import GATConv
    gen = torch.Generator().manual_seed(7000 + [k.name for k in CASES].index(c.name))
    B, T, N, Cin = c.B, c.T, c.N, c.Cin
    x = torch.randn(B, T, N, Cin, generator=gen) * c.xscale
    mask = (torch.rand(B, N, generator=gen) > 0.25).float()
    for b in range(B):
        if mask[b].sum() == 0:
            mask[b, int(torch.randint(N, (1,), generator=gen))] = 1
    if c.kind == "degenerate":
        mask[0] = 0
        mask[1] = 0
        mask[1, int(torch.randint(N, (1,), generator=gen))] = 1
        mask[2, 3] = 1
    eye = torch.eye(N)
    if c.adj == "dense":
        adj = torch.ones(B, N, N)
    else:
        adj = (torch.rand(B, N, N, generator=gen) < min(0.5, 4.0 / N)).float()
        adj = ((adj + adj.transpose(1, 2)) > 0).float()
    adj = adj * (1 - eye)
    adj[::2] += eye
    adj = adj * mask[:, :, None] * mask[:, None, :]
    if c.kind == "degenerate":
        adj[2, 3, :] = 0
        adj[2, :, 3] = 0
    if c.kind == "equal":
        x = x[:, :, :1].expand(B, T, N, Cin).contiguous()
    x = x * mask[:, None, :, None]
    if c.kind == "degenerate":
        x = x + 123.0 * (1 - mask)[:, None, :, None]
    layer = GATConv(Cin, c.C, c.H, dropout_rate=c.dropout, activation=c.act)
    with torch.no_grad():
        layer.kernel.copy_(torch.randn(layer.kernel.shape, generator=gen) * 0.5)
        layer.attn_kernel_self.copy_(torch.randn(layer.attn_kernel_self.shape, generator=gen) * 0.5)
        layer.attn_kernel_neighs.copy_(torch.randn(layer.attn_kernel_neighs.shape, generator=gen) * 0.5)
        layer.bias.copy_(torch.randn(layer.bias.shape, generator=gen) * 0.1)
        if layer.prelu_alpha is not None:
            layer.prelu_alpha.copy_(torch.rand(layer.prelu_alpha.shape, generator=gen) * 0.3)
        if c.kind == "degenerate":
            # orient the neighbour scores so that a 123.0 row would win every softmax it was let into
            u_n = torch.einsum("fhc,ch->fh", layer.kernel, layer.attn_kernel_neighs[..., 0]).sum(0)
            layer.attn_kernel_neighs.mul_(torch.where(u_n < 0, -1.0, 1.0)[None, :, None])
    layer.train(c.training)
    M, Mp, Cp = time_major_pad(c)
    return dict(x=x, adj=adj, mask=mask, layer=layer, g=torch.randn((T, Mp, Cp), generator=gen))


PARAMS = (("W", "kernel"), ("a_s", "attn_kernel_self"), ("a_n", "attn_kernel_neighs"), ("bias", "bias"),
          ("alpha", "prelu_alpha"))


def run_case(c, d, dtype, device="cpu"):
    """``gat_node_tm_eager`` on the CPU (or ``gat_node_tm`` on a device) in ``dtype``: the output
    ``[T, Mp, Cp]`` and the gradients of x and every parameter for the upstream gradient ``d['g']``,
    as float64 CPU tensors."""
    from gnnqc.ops import gcn as G
    layer = copy.deepcopy(d["layer"]).to(device=device, dtype=dtype)
    x = d["x"].to(device=device, dtype=dtype).clone().requires_grad_(True)          # (clone: a fresh leaf)
    adj, mask = d["adj"].to(device=device, dtype=dtype), d["mask"].to(device=device, dtype=dtype)
    out, M = (G.gat_node_tm_eager if device == "cpu" else G.gat_node_tm)(x, adj, mask, layer)
    assert M == c.B * c.N
    out.backward(d["g"].to(device=device, dtype=dtype))
    grads = {"x": x.grad}
    for name, attr in PARAMS:
        p = getattr(layer, attr)
        if p is not None:
            grads[name] = p.grad
    grads = {k: (torch.zeros(0) if v is None else v.detach().double().cpu()) for k, v in grads.items()}
    return out.detach().double().cpu(), grads


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, inputs, float64 oracle (out, grads), float32 eager errors {quantity: max |err|})."""
    c = next(k for k in CASES if k.name == name)
    d = node_inputs(c)
    out64, g64 = run_case(c, d, torch.float64)
    out32, g32 = run_case(c, d, torch.float32)
    e32 = {"out": (out32 - out64).abs().max().item()}
    for k in g64:
        e32[k] = (g32[k] - g64[k]).abs().max().item() if g64[k].numel() else 0.0
    return c, d, (out64, g64), e32


def out_excess(got, ref, e32):
    """max over elements of |got - ref| / bound, bound = max(K e32, 1e-4 + 1e-4 |ref|); inf if
    ``got`` is not finite. <= 1 passes."""
    if not torch.isfinite(got).all():
        return float("inf")
    bound = torch.clamp(OUT_ATOL + OUT_RTOL * ref.abs(), min=K_FLOOR_MULT * e32)
    return ((got - ref).abs() / bound).max().item() if ref.numel() else 0.0


def grad_bound(ref, e32):
    return max(K_FLOOR_MULT * e32, GRAD_REL * (ref.abs().max().item() + 1e-6))


_REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _report_file():
    yield
    path = os.environ.get("GNNQC_GAT_NODE_REPORT")
    if path and _REPORT:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("# tests/test_gat_node_kernels_gpu.py: measured |err| of the HIP path against the float64 oracle,\n"
                    f"# the float32 eager layer's own error (e32) and the bound (max of {K_FLOOR_MULT:g} x e32 and the\n"
                    "# floor: 1e-4 + 1e-4 |ref| on outputs, 1e-3 max|ref| on gradients; 'out' lists err / bound).\n"
                    f"# {'case':<28} {'quantity':<8} {'err':>11} {'e32':>11} {'bound':>11}\n")
            f.write("\n".join(_REPORT) + "\n")


@pytest.mark.parametrize("name", HIP_CASES)
def test_gat_node_case_matches_float64(cuda_device, name):
    """Output, dx, dW, da_s, da_n, dbias, dalpha of one case against float64 eager, within the
    measured bound; padding rows and padding channels exactly zero."""
    from gnnqc.ops import gcn as G
    c, d, (out64, g64), e32 = reference(name)
    dev = cuda_device
    assert G.gat_node_tm_ok(d["x"].to(dev), copy.deepcopy(d["layer"]).to(dev))
    out, grads = run_case(c, d, torch.float32, dev)
    M, Mp, Cp = time_major_pad(c)
    Fo = c.H * c.C + c.Cin
    assert tuple(out.shape) == (c.T, Mp, Cp) == tuple(out64.shape)
    assert torch.count_nonzero(out[:, M:]) == 0, "padding rows"
    assert torch.count_nonzero(out[:, :, Fo:]) == 0, "padding channels"
    ex = out_excess(out, out64, e32["out"])
    _REPORT.append(f"{c.name:<30} {'out':<8} {(out - out64).abs().max().item():11.3e} {e32['out']:11.3e} "
                   f"{ex:11.3e}")
    print(_REPORT[-1])
    fails = [] if ex <= 1.0 else [f"out: err / bound = {ex:.3f}"]
    assert set(grads) == set(g64)
    for k, ref in g64.items():
        got = grads[k] if grads[k].numel() else torch.zeros_like(ref)
        assert got.shape == ref.shape, (k, got.shape, ref.shape)
        err = (got - ref).abs().max().item() if ref.numel() else 0.0
        bound = grad_bound(ref, e32[k])
        _REPORT.append(f"{c.name:<30} {'d' + k:<8} {err:11.3e} {e32[k]:11.3e} {bound:11.3e}")
        print(_REPORT[-1])
        if not (err <= bound) or not torch.isfinite(got).all():
            fails.append(f"d{k}: err {err:.3e} > bound {bound:.3e}")
    assert not fails, f"{c.name}: " + "; ".join(fails)


@pytest.mark.parametrize("name", OFF_CASES)
def test_gat_node_off_the_hip_path_raises(cuda_device, name):
    """N = 257 and training-mode attention dropout: gat_node_tm_ok is false and gat_node_tm raises,
    as gat_pool(time_major=True) does."""
    from gnnqc.ops import gcn as G
    c = next(k for k in CASES if k.name == name)
    d = node_inputs(c)
    dev = cuda_device
    layer = copy.deepcopy(d["layer"]).to(dev)
    x, adj, mask = d["x"].to(dev), d["adj"].to(dev), d["mask"].to(dev)
    assert not G.gat_node_tm_ok(x, layer)
    with pytest.raises(ValueError):
        G.gat_node_tm(x, adj, mask, layer)


def test_gat_node_backward_is_bitwise_reproducible(cuda_device):
    """Two runs of a multi-pass case give bitwise-equal outputs and gradients (fixed-order record
    sum, no float atomics)."""
    c, d, _, _ = reference("passes")
    a = run_case(c, d, torch.float32, cuda_device)
    b = run_case(c, d, torch.float32, cuda_device)
    assert torch.equal(a[0], b[0])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
