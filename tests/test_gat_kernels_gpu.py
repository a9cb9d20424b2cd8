"""The fused GATConv kernels (``csrc/kernels/gat.hip``) over their shape and dispatch space, against
the float64 eager layer on the CPU.

Every case runs :func:`gnnqc.ops.gcn.gat_pool` on the device and compares the output, ``dx``,
``danom`` and every parameter gradient (``dW``, ``da_s``, ``da_n``, ``dbias``, ``dalpha``) with
``GATConv`` + ``pool_nodes`` + ``cat`` in float64 (:func:`gnnqc.ops.gcn.gat_pool_eager`, autograd on
the float64 graph).

The bound is measured per case and quantity. The yardstick is the error of the SAME eager layer run
in float32 on the CPU against that float64 oracle (``e32``); the kernel may be ``K_FLOOR_MULT = 4``
times as far off. (Both are float32 evaluations of the same expression with about the same number of
roundings per score and per output - the kernel forms ``u = W a`` first and then ``x . u``, the layer
``(x W) . a`` - so their errors are samples of one distribution; the maximum over a case's elements
of two such samples differs by a small factor, and ``__expf`` adds an argument error of the size of
the score's own rounding error. 4 covers that with margin; it is not fitted to the kernel.) The bound
never drops below the floor the GeneralConv tests use: ``1e-4 + 1e-4 |ref|`` per output element,
``1e-3 max|ref|`` on a gradient.

Each case names the branches it is there to reach (``tags``); ``tests/test_gat_reference_cpu.py``
recomputes their predicates from the shapes, checks the oracle and the kernel's math in float64,
and checks that named mutants of that math lie at least 5 bounds away.

With ``GNNQC_GAT_REPORT=<path>`` the measured error and bound of every case and quantity are
written there (``profiles/gat_kernel_tests.txt`` is such a run).
"""
import copy
import functools
import os
from collections import namedtuple

import pytest
import torch

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------ constants of the kernels
K_MAX_N = 64                # gat.hip GAT_MAX_N (one 64-bit neighbour mask per node)
K_THREADS = 256             # gat.hip: lanes per workgroup; rows per workgroup = 256 / pow2(N)
K_GRID_CAP = 256            # gat.hip GAT_GRID_CAP (more row blocks: several passes per workgroup)
K_WIDTHS = ((8, 16, 32), (1, 2))      # gat.hip GQ_GAT_DISPATCH: C, H
K_FLOOR_MULT = 4.0          # allowed kernel error / float32 eager error (see the module docstring)
OUT_ATOL = OUT_RTOL = 1e-4  # the floor on outputs
GRAD_REL = 1e-3             # the floor on gradients, relative to max |ref|

GatCase = namedtuple("GatCase", "name B T N Cin C H pooling tm anom training dropout act kind xscale tags")


def _gc(name, B=5, T=11, N=9, Cin=2, C=16, H=1, pooling="mean", tm=False, anom=True, training=True, dropout=0.0,
        act="prelu", kind="", xscale=1.0, tags=()):
    return GatCase(name, B, T, N, Cin, C, H, pooling, tm, anom, training, dropout, act, kind, xscale, tuple(tags))


def _cases():
    cs = []
    for Cin, C, H in [(2, 16, 1), (2, 8, 2), (2, 16, 2), (1, 8, 1), (3, 32, 1), (4, 16, 1)]:
        for pooling in ("mean", "selection"):
            cs.append(_gc(f"dispatch_c{Cin}f{C}h{H}_{pooling}", Cin=Cin, C=C, H=H, pooling=pooling,
                          tags=("hip", "np_gt_n", "ragged_rows")))
    cs += [
        _gc("nodes_1", N=1, tags=("hip", "single_node", "one_pass")),
        _gc("nodes_7", N=7, tags=("hip", "np_gt_n")),
        _gc("nodes_33", N=33, H=2, C=8, tags=("hip", "two_words", "np_gt_n")),
        _gc("nodes_64", N=64, tags=("hip", "two_words", "limit")),
        _gc("nodes_64_selection", N=64, pooling="selection", tags=("hip", "two_words", "limit")),
        _gc("tm_b5", B=5, tm=True, tags=("hip", "tm_pad_rows", "tm_pad_ch")),
        _gc("tm_b17_selection", B=17, tm=True, pooling="selection", H=2, tags=("hip", "tm_pad_rows", "tm_pad_ch")),
        _gc("tm_b16_c3", B=16, tm=True, Cin=3, tags=("hip", "tm_pad_ch")),
        _gc("no_anom", anom=False, tags=("hip", "no_anom")),
        _gc("no_anom_tm", B=17, anom=False, tm=True, tags=("hip", "no_anom", "tm_pad_rows")),
        _gc("passes", B=48, T=181, N=7, tags=("hip", "multi_pass", "many_records", "np_gt_n")),
        _gc("passes_tm_h2", B=48, T=181, N=7, H=2, C=8, tm=True, pooling="selection",
            tags=("hip", "multi_pass", "many_records")),
        _gc("rows_ragged", B=3, T=7, N=5, tags=("hip", "ragged_rows", "one_pass")),
    ]
    for pooling in ("mean", "sum", "selection"):
        cs.append(_gc(f"degenerate_{pooling}", pooling=pooling, kind="degenerate", tags=("hip", "degenerate")))
    cs += [
        _gc("scores_x30", kind="scores", xscale=30.0, tags=("hip", "large_scores")),
        _gc("scores_x30_selection_h2", kind="scores", xscale=30.0, H=2, pooling="selection",
            tags=("hip", "large_scores")),
        _gc("scores_equal", kind="equal", tags=("hip", "equal_scores")),
        _gc("pool_sum", pooling="sum", tags=("hip",)),
        _gc("pool_sum_tm", pooling="sum", tm=True, B=17, tags=("hip", "tm_pad_rows")),
        _gc("eval_dropout", training=False, dropout=0.5, tags=("hip", "eval_dropout")),
        _gc("train_no_dropout_h2", training=True, dropout=0.0, H=2, tags=("hip",)),
        _gc("act_linear", act=None, tags=("hip", "act_linear")),
        _gc("act_relu", act="relu", pooling="selection", tags=("hip", "act_relu")),
        # not on the HIP path: gat_pool() must take the eager layer on the device
        _gc("eager_nodes_65", B=2, T=3, N=65, tags=("eager",)),
        _gc("eager_pool_max", pooling="max", tags=("eager",)),
    ]
    return cs


CASES = _cases()


def _cdiv(a, b):
    return -(-a // b)


def _pow2(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def rows_per_workgroup(c):
    return K_THREADS // _pow2(c.N)


def time_major_pad(c):
    """(Mp, Cp) of gat_pool(time_major=True)."""
    Cp = (c.Cin if c.anom else 0) + c.H * c.C
    return _cdiv(c.B, 16) * 16, Cp + (-Cp) % 4


def on_hip_path(c):
    """The conditions of gat_pool_hip_ok, from the case's shape alone."""
    return (c.N <= K_MAX_N and c.Cin <= 4 and c.pooling in ("mean", "sum", "selection")
            and not (c.dropout > 0 and c.training) and c.C in K_WIDTHS[0] and c.H in K_WIDTHS[1]
            and c.act in (None, "linear", "prelu", "relu"))


PREDICATES = {
    "hip": on_hip_path,
    "eager": lambda c: not on_hip_path(c),
    "np_gt_n": lambda c: _pow2(c.N) > c.N,
    "single_node": lambda c: c.N == 1,
    "two_words": lambda c: c.N > 32,
    "limit": lambda c: c.N == K_MAX_N,
    "one_pass": lambda c: _cdiv(c.B * c.T, rows_per_workgroup(c)) <= K_GRID_CAP,
    "multi_pass": lambda c: _cdiv(c.B * c.T, rows_per_workgroup(c)) > K_GRID_CAP,
    "many_records": lambda c: min(K_GRID_CAP, _cdiv(c.B * c.T, rows_per_workgroup(c))) * c.H >= 128,
    "ragged_rows": lambda c: (c.B * c.T) % rows_per_workgroup(c) != 0,
    "tm_pad_rows": lambda c: c.tm and time_major_pad(c)[0] > c.B,
    "tm_pad_ch": lambda c: c.tm and time_major_pad(c)[1] > (c.Cin if c.anom else 0) + c.H * c.C,
    "no_anom": lambda c: not c.anom,
    "degenerate": lambda c: c.kind == "degenerate" and c.B >= 4,
    "large_scores": lambda c: c.kind == "scores" and c.xscale >= 30,
    "equal_scores": lambda c: c.kind == "equal",
    "eval_dropout": lambda c: not c.training and c.dropout > 0,
    "act_linear": lambda c: c.act in (None, "linear"),
    "act_relu": lambda c: c.act == "relu",
}


# ------------------------------------------------------------------ input builder (CPU, float32)
def gat_inputs(c):
    """Inputs and the layer of a case on the CPU. Random masks (every sample keeps a node),
    ``anom_pos`` among the valid nodes, a symmetric adjacency between valid nodes whose diagonal is
    set only in every other sample (the layer adds the self loops). ``kind``:

    * ``degenerate``: sample 0 has every node masked and ``anom_pos = -1``, sample 1 a single valid
      node, sample 2 a valid node without any edge (flagged), and every padded node holds 123.0
      (with the neighbour attention kernel oriented so that such a row would dominate a softmax);
    * ``scores``: ``x`` times ``xscale`` (scores beyond float32's exp range without the max);
    * ``equal``: all nodes of a (sample, step) share one feature vector (all scores equal).
    """
    from gnnqc.models.graphconv import GATConv
    gen = torch.Generator().manual_seed(4000 + [k.name for k in CASES].index(c.name))
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
    adj = (torch.rand(B, N, N, generator=gen) > 0.5).float()
    adj = ((adj + adj.transpose(1, 2)) > 0).float() * (1 - torch.eye(N))
    adj[::2] += torch.eye(N)
    adj = adj * mask[:, :, None] * mask[:, None, :]
    if c.kind == "degenerate":
        adj[2, 3, :] = 0
        adj[2, :, 3] = 0
    if c.kind == "equal":
        x = x[:, :, :1].expand(B, T, N, Cin).contiguous()
    x = x * mask[:, None, :, None]
    if c.kind == "degenerate":
        x = x + 123.0 * (1 - mask)[:, None, :, None]
    anom_pos = torch.full((B,), -1, dtype=torch.long)
    for b in range(B):
        valid = mask[b].nonzero().flatten()
        if valid.numel():
            anom_pos[b] = valid[int(torch.randint(valid.numel(), (1,), generator=gen))]
    if c.kind == "degenerate":
        anom_pos[2] = 3
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
    anom =torch.randn(B, T, Cin, generator=gen) if c.anom else None
    Mp, Cp = time_major_pad(c)
    gshape = (T, Mp, Cp) if c.tm else (B, T, (Cin if c.anom else 0) + c.H * c.C)
    return dict(x=x, adj=adj, mask=mask, anom=anom, anom_pos=anom_pos, layer=layer,
                g=torch.randn(gshape, generator=gen))


PARAMS = (("W", "kernel"), ("a_s", "attn_kernel_self"), ("a_n", "attn_kernel_neighs"), ("bias", "bias"),
          ("alpha", "prelu_alpha"))


def run_eager(c, d, dtype, device="cpu"):
    """``gat_pool_eager`` (or ``gat_pool`` on a device) in ``dtype``: the output as [B, T, Fo] and
    the gradients of x, anom and every parameter for the case's upstream gradient ``d['g']``, as
    float64 CPU tensors. Returns ``(out, grads, raw output)``."""
    from gnnqc.ops import gcn as G
    layer = copy.deepcopy(d["layer"]).to(device=device, dtype=dtype)
    x = d["x"].to(device=device, dtype=dtype).clone().requires_grad_(True)          # (clone: a fresh leaf)
    anom = d["anom"].to(device=device, dtype=dtype).clone().requires_grad_(True) if d["anom"] is not None else None
    args = (x, d["adj"].to(device=device, dtype=dtype), d["mask"].to(device=device, dtype=dtype), anom,
            d["anom_pos"].to(device), layer, c.pooling)
    Fo = (c.Cin if c.anom else 0) + c.H * c.C
    if device == "cpu":
        raw = out = G.gat_pool_eager(*args)
        g = d["g"][:, :c.B, :Fo].transpose(0, 1) if c.tm else d["g"]
    else:
        raw = G.gat_pool(*args, time_major=c.tm)
        if c.tm:
            raw, Bret = raw
            assert Bret == c.B
        out = raw[:, :c.B, :Fo].transpose(0, 1) if c.tm else raw
        g = d["g"]
    raw.backward(g.to(device=device, dtype=dtype))
    grads = {"x": x.grad}
    if anom is not None:
        grads["anom"] = anom.grad
    for name, attr in PARAMS:
        p = getattr(layer, attr)
        if p is not None:
            grads[name] = p.grad
    grads = {k: (torch.zeros(0) if v is None else v.detach().double().cpu()) for k, v in grads.items()}
    return out.detach().double().cpu(), grads, raw.detach()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, inputs, float64 oracle (out, grads), float32 eager errors {quantity: max |err|})."""
    c = next(k for k in CASES if k.name == name)
    d = gat_inputs(c)
    out64, g64, _ = run_eager(c, d, torch.float64)
    out32, g32, _ = run_eager(c, d, torch.float32)
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
    path = os.environ.get("GNNQC_GAT_REPORT")
    if path and _REPORT:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("# tests/test_gat_kernels_gpu.py: measured |err| of the HIP path against the float64 oracle,\n"
                    f"# the float32 eager layer's own error (e32) and the bound (max of {K_FLOOR_MULT:g} x e32 and the\n"
                    "# floor: 1e-4 + 1e-4 |ref| on outputs, 1e-3 max|ref| on gradients; 'out' lists err / bound).\n"
                    f"# {'case':<28} {'quantity':<8} {'err':>11} {'e32':>11} {'bound':>11}\n")
            f.write("\n".join(_REPORT) + "\n")


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_gat_case_matches_float64(cuda_device, name):
    """Output, dx, danom, dW, da_s, da_n, dbias, dalpha of one case against float64 eager, within the
    measured bound; time-major cases: padding rows and channels exactly zero; the cases off the HIP
    path run the eager layer on the device."""
    from gnnqc.ops import gcn as G
    c, d, (out64, g64), e32 = reference(name)
    dev = cuda_device
    layer_dev = copy.deepcopy(d["layer"]).to(dev)
    assert G.gat_pool_hip_ok(d["x"].to(dev), layer_dev, c.pooling) == ("eager" not in c.tags)
    out, grads, raw = run_eager(c, d, torch.float32, dev)
    Fo = out64.shape[-1]
    if c.tm:
        Mp, Cp = time_major_pad(c)
        assert tuple(raw.shape) == (c.T, Mp, Cp)
        assert torch.count_nonzero(raw[:, c.B:]) == 0, "time-major padding rows"
        assert torch.count_nonzero(raw[:, :, Fo:]) == 0, "time-major padding channels"
    else:
        assert tuple(raw.shape) == (c.B, c.T, Fo)
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


def test_gat_backward_is_bitwise_reproducible(cuda_device):
    """Two runs of the multi-pass case give bitwise-equal outputs and gradients (fixed-order record
    sum, no float atomics)."""
    c, d, _, _ = reference("passes")
    a = run_eager(c, d, torch.float32, cuda_device)
    b = run_eager(c, d, torch.float32, cuda_device)
    assert torch.equal(a[0], b[0])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
