"""The fused EdgeConv kernels (``csrc/kernels/edge.hip``) over their shape and dispatch space,
against the float64 eager layer on the CPU.

Every case runs :func:`gnnqc.ops.gcn.edge_pool` on the device and compares the output, ``dx``,
``danom`` and every parameter gradient (``dW``, ``dbias``, ``dalpha``) with ``EdgeConv`` +
``pool_nodes`` + ``cat`` in float64 (:func:`gnnqc.ops.gcn.edge_pool_eager`, autograd on the float64
graph).

The bound is measured per case and quantity, by the rule of ``tests/test_gat_kernels_gpu.py``. The
yardstick is the error of the SAME eager layer run in float32 on the CPU against that float64 oracle
(``e32``); the kernel may be ``K_FLOOR_MULT = 4`` times as far off. The bound never drops below the
floor the GeneralConv tests use: ``1e-4 + 1e-4 |ref|`` per output element, ``1e-3 max|ref|`` on a
gradient.

Kinks. ReLU and PReLU are applied per edge, so every gradient is discontinuous where an edge's
pre-activation ``z_ij`` crosses zero: a float32 sign flip there would decide the verdict instead of
the kernel. The inputs are therefore drawn on a dyadic lattice (``x`` in steps of ``xscale / 8``,
weights in steps of 1/16, biases odd multiples of half the products' quantum): every ``z_ij`` is an
exact float32 number at least half a quantum away from zero, the same number in the layer, in the
kernel's ``p_i + q_j`` split and in float64. ``tests/test_edge_reference_cpu.py`` asserts the
resulting margin (no neighbour edge within 64 float32 ulps of the case's ``max |z|``) for every case
except ``kink_zeros``, which is built to hold exact zeros (zero bias, one all-zero sample) and pins
the branch taken AT zero.

Each case names the branches it is there to reach (``tags``); the CPU file recomputes their
predicates from the shapes, checks the oracle and the kernel's math in float64, and checks that
named mutants of that math lie at least 5 bounds away.

With ``GNNQC_EDGE_REPORT=<path>`` the measured error and bound of every case and quantity are
written there (``profiles/edge_kernel_tests.txt`` is such a run).
"""
import copy
import functools
import os
from collections import namedtuple

import pytest
import torch

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------ constants of the kernels
K_MAX_N = 64                # edge.hip EDGE_MAX_N (one 64-bit neighbour word per node)
K_THREADS = 256             # edge.hip: lanes per workgroup; rows per workgroup = 256 / pow2(N)
K_GRID_CAP = 256            # edge.hip EDGE_GRID_CAP (more row blocks: several passes per workgroup)
K_WIDTHS = (8, 16, 32)      # edge.hip GQ_EDGE_DISPATCH: C
K_CHUNK = 8                 # edge.hip EDGE_CH: channels per LDS stage / per backward workgroup
K_FLOOR_MULT = 4.0          # allowed kernel error / float32 eager error (see the module docstring)
OUT_ATOL = OUT_RTOL = 1e-4  # the floor on outputs
GRAD_REL = 1e-3             # the floor on gradients, relative to max |ref|

EdgeCase = namedtuple("EdgeCase", "name B T N Cin C agg pooling tm anom training act hidden kind xscale tags")


def _ec(name, B=5, T=11, N=9, Cin=2, C=16, agg="sum", pooling="mean", tm=False, anom=True, training=True,
        act="prelu", hidden=(), kind="", xscale=1.0, tags=()):
    return EdgeCase(name, B, T, N, Cin, C, agg, pooling, tm, anom, training, act, tuple(hidden), kind, xscale,
                    tuple(tags))


def _cases():
    cs = []
    k = 0
    for Cin in (1, 2, 3, 4):
        for C in (8, 16, 32):
            agg, pooling = ("sum", "mean")[k % 2], ("mean", "selection")[(k // 2) % 2]
            k += 1
            cs.append(_ec(f"dispatch_c{Cin}f{C}_{agg}_{pooling}", Cin=Cin, C=C, agg=agg, pooling=pooling,
                          tags=("hip", "np_gt_n", "ragged_rows") + (("chunks",) if C > K_CHUNK else ())))
    cs += [
        _ec("nodes_1", N=1, agg="mean", tags=("hip", "single_node", "one_pass")),
        _ec("nodes_7", N=7, agg="mean", tags=("hip", "np_gt_n")),
        _ec("nodes_33", N=33, C=8, tags=("hip", "two_words", "np_gt_n")),
        _ec("nodes_64", N=64, agg="mean", tags=("hip", "two_words", "limit")),
        _ec("nodes_64_selection", N=64, pooling="selection", tags=("hip", "two_words", "limit")),
        _ec("rows_ragged", B=3, T=7, N=5, agg="mean", tags=("hip", "ragged_rows", "one_pass")),
        _ec("passes", B=48, T=181, N=7, agg="mean", tags=("hip", "multi_pass", "many_records", "np_gt_n")),
        _ec("passes_tm", B=48, T=181, N=7, C=8, tm=True, pooling="selection",
            tags=("hip", "multi_pass", "many_records")),
        _ec("tm_b5", B=5, tm=True, agg="mean", tags=("hip", "tm_pad_rows", "tm_pad_ch")),
        _ec("tm_b16_c4", B=16, tm=True, Cin=4, tags=("hip", "tm_full_rows", "tm_full_ch")),
        _ec("tm_b17_selection", B=17, tm=True, pooling="selection", C=32,
            tags=("hip", "tm_pad_rows", "tm_pad_ch", "chunks")),
        _ec("no_anom", anom=False, tags=("hip", "no_anom")),
        _ec("no_anom_tm", B=17, anom=False, tm=True, agg="mean", tags=("hip", "no_anom", "tm_pad_rows", "tm_full_ch")),
        _ec("pool_sum", pooling="sum", agg="mean", tags=("hip", "pool_sum")),
        _ec("pool_sum_tm", pooling="sum", tm=True, B=17, tags=("hip", "pool_sum", "tm_pad_rows")),
        _ec("act_linear", act=None, agg="mean", tags=("hip", "act_linear")),
        _ec("act_relu", act="relu", pooling="selection", tags=("hip", "act_relu")),
        _ec("eval_mode", training=False, agg="mean", tags=("hip", "eval")),
    ]
    for pooling, agg in (("mean", "mean"), ("sum", "sum"), ("selection", "mean")):
        cs.append(_ec(f"degenerate_{pooling}", pooling=pooling, agg=agg, kind="degenerate",
                      tags=("hip", "degenerate")))
    cs += [
        _ec("x30", xscale=30.0, agg="mean", tags=("hip", "large_x")),
        _ec("x30_selection_relu", xscale=30.0, pooling="selection", act="relu", C=32,
            tags=("hip", "large_x", "chunks")),
        _ec("kink_zeros", kind="zeros", tags=("hip", "exact_zeros")),
        # not on the HIP path: edge_pool() must take the eager layer on the device
        _ec("eager_nodes_65", B=2, T=3, N=65, tags=("eager",)),
        _ec("eager_agg_max", agg="max", tags=("eager",)),
        _ec("eager_mlp_hidden", B=3, T=5, hidden=(16,), tags=("eager",)),
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
    """(Mp, Cp) of edge_pool(time_major=True)."""
    Cp = (c.Cin if c.anom else 0) + c.C
    return _cdiv(c.B, 16) * 16, Cp + (-Cp) % 4


def on_hip_path(c):
    """The conditions of edge_pool_hip_ok, from the case's shape alone."""
    return (c.N <= K_MAX_N and 1 <= c.Cin <= 4 and c.pooling in ("mean", "sum", "selection")
            and c.agg in ("sum", "mean") and not c.hidden and c.C in K_WIDTHS
            and c.act in (None, "linear", "prelu", "relu"))


PREDICATES = {
    "hip": on_hip_path,
    "eager": lambda c: not on_hip_path(c),
    "np_gt_n": lambda c: _pow2(c.N) > c.N,
    "single_node": lambda c: c.N == 1,
    "two_words": lambda c: c.N > 32,
    "limit": lambda c: c.N == K_MAX_N,
    "chunks": lambda c: c.C > K_CHUNK,
    "one_pass": lambda c: _cdiv(c.B * c.T, rows_per_workgroup(c)) <= K_GRID_CAP,
    "multi_pass": lambda c: _cdiv(c.B * c.T, rows_per_workgroup(c)) > K_GRID_CAP,
    "many_records": lambda c: min(K_GRID_CAP, _cdiv(c.B * c.T, rows_per_workgroup(c))) >= 128,
    "ragged_rows": lambda c: (c.B * c.T) % rows_per_workgroup(c) != 0,
    "tm_pad_rows": lambda c: c.tm and time_major_pad(c)[0] > c.B,
    "tm_full_rows": lambda c: c.tm and time_major_pad(c)[0] == c.B,
    "tm_pad_ch": lambda c: c.tm and time_major_pad(c)[1] > (c.Cin if c.anom else 0) + c.C,
    "tm_full_ch": lambda c: c.tm and time_major_pad(c)[1] == (c.Cin if c.anom else 0) + c.C,
    "no_anom": lambda c: not c.anom,
    "pool_sum": lambda c: c.pooling == "sum",
    "degenerate": lambda c: c.kind == "degenerate" and c.B >= 5 and c.N >= 6,
    "large_x": lambda c: c.xscale >= 30,
    "exact_zeros": lambda c: c.kind == "zeros" and c.act == "prelu",
    "act_linear": lambda c: c.act in (None, "linear"),
    "act_relu": lambda c: c.act == "relu",
    "eval": lambda c: not c.training,
}


# ------------------------------------------------------------------ input builder (CPU, float32)
def _lattice_layer(layer, q, gen, zero_bias=False):
    """Dense kernels in steps of 1/16 and biases that are odd multiples of half the quantum of the
    layer's products, so that no pre-activation is closer to zero than that. ``q``: the quantum of
    the layer's input. Returns the quantum of the output layer's pre-activations."""
    with torch.no_grad():
        for dense in list(layer.hidden) + [layer.out]:
            dense.kernel.copy_(torch.round(torch.randn(dense.kernel.shape, generator=gen) * 0.5 * 16) / 16)
            q = q / 32                                       # products: q / 16; the bias sits at odd q / 32
            odd = 2 * torch.randint(-3, 3, dense.bias.shape, generator=gen) + 1
            dense.bias.copy_(torch.zeros_like(dense.bias) if zero_bias else odd.float() * q)
        if layer.prelu_alpha is not None:
            layer.prelu_alpha.copy_(torch.rand(layer.prelu_alpha.shape, generator=gen) * 0.3)
    return q


def edge_inputs(c):
    """Inputs and the layer of a case on the CPU, on the dyadic lattice of the module docstring.
    Random masks (every sample keeps a node), ``anom_pos`` among the valid nodes, a random
    ASYMMETRIC 0/1 adjacency between valid nodes whose diagonal is set only in every other sample
    (the layer adds no self loop). ``kind``:

    * ``degenerate``: sample 0 has every node masked and ``anom_pos = -1``; sample 1 a single valid
      node; sample 2 a valid, flagged node (3) without any edge (degree 0) and node 3 in nobody's
      neighbourhood; sample 3 keeps adjacency entries from valid nodes TOWARDS its masked nodes;
      every padded node holds 123.0;
    * ``zeros``: zero bias and sample 0 all zero, so every ``z_ij`` of sample 0 is exactly 0.
    """
    from gnnqc.models.graphconv import EdgeConv
    gen = torch.Generator().manual_seed(7000 + [k.name for k in CASES].index(c.name))
    B, T, N, Cin = c.B, c.T, c.N, c.Cin
    gx = c.xscale / 8
    x = torch.round(torch.randn(B, T, N, Cin, generator=gen) * 8) * gx
    mask = (torch.rand(B, N, generator=gen) > 0.25).float()
    for b in range(B):
        if mask[b].sum() == 0:
            mask[b, int(torch.randint(N, (1,), generator=gen))] = 1
    if c.kind == "degenerate":
        mask[0] = 0
        mask[1] = 0
        mask[1, int(torch.randint(N, (1,), generator=gen))] = 1
        mask[2, 3] = 1
        mask[3, :2] = 1
        mask[3, 2] = 0
    adj = (torch.rand(B, N, N, generator=gen) > 0.5).float() * (1 - torch.eye(N))
    adj[::2] += torch.eye(N)
    keep = adj.clone()
    adj = adj * mask[:, :, None] * mask[:, None, :]
    if c.kind == "degenerate":
        adj[2, 3, :] = 0
        adj[2, :, 3] = 0
        adj[3] = keep[3] * mask[3, :, None]                  # rows of valid nodes keep their masked neighbours
        adj[3, 0, 2] = 1
    if c.kind == "zeros":
        x[0] = 0
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
    layer = EdgeConv(Cin, c.C, list(c.hidden) or None, "relu", c.agg, c.act)
    _lattice_layer(layer, gx, gen, zero_bias=c.kind == "zeros")
    layer.train(c.training)
    anom = torch.randn(B, T, Cin, generator=gen) if c.anom else None
    Mp, Cp = time_major_pad(c)
    gshape = (T, Mp, Cp) if c.tm else (B, T, (Cin if c.anom else 0) + c.C)
    return dict(x=x, adj=adj, mask=mask, anom=anom, anom_pos=anom_pos, layer=layer,
                g=torch.randn(gshape, generator=gen))


def layer_params(layer):
    """{quantity name: parameter} of an EdgeConv: W / bias / alpha of the output layer, hidden
    layers as W<k> / bias<k>."""
    ps = {"W": layer.out.kernel, "bias": layer.out.bias}
    if layer.prelu_alpha is not None:
        ps["alpha"] = layer.prelu_alpha
    for k, dense in enumerate(layer.hidden):
        ps[f"W{k}"], ps[f"bias{k}"] = dense.kernel, dense.bias
    return ps


def run_eager(c, d, dtype, device="cpu"):
    """``edge_pool_eager`` (or ``edge_pool`` on a device) in ``dtype``: the output as [B, T, Fo] and
    the gradients of x, anom and every parameter for the case's upstream gradient ``d['g']``, as
    float64 CPU tensors. Returns ``(out, grads, raw output)``."""
    from gnnqc.ops import gcn as G
    layer = copy.deepcopy(d["layer"]).to(device=device, dtype=dtype)
    x = d["x"].to(device=device, dtype=dtype).clone().requires_grad_(True)          # (clone: a fresh leaf)
    anom = d["anom"].to(device=device, dtype=dtype).clone().requires_grad_(True) if d["anom"] is not None else None
    args = (x, d["adj"].to(device=device, dtype=dtype), d["mask"].to(device=device, dtype=dtype), anom,
            d["anom_pos"].to(device), layer, c.pooling)
    Fo = (c.Cin if c.anom else 0) + c.C
    if device == "cpu":
        raw = out = G.edge_pool_eager(*args)
        g = d["g"][:, :c.B, :Fo].transpose(0, 1) if c.tm else d["g"]
    else:
        raw = G.edge_pool(*args, time_major=c.tm)
        if c.tm:
            raw, Bret = raw
            assert Bret == c.B
        out = raw[:, :c.B, :Fo].transpose(0, 1) if c.tm else raw
        g = d["g"]
    raw.backward(g.to(device=device, dtype=dtype))
    grads = {"x": x.grad}
    if anom is not None:
        grads["anom"] = anom.grad
    for name, p in layer_params(layer).items():
        grads[name] = p.grad
    grads = {k: (torch.zeros(0) if v is None else v.detach().double().cpu()) for k, v in grads.items()}
    return out.detach().double().cpu(), grads, raw.detach()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, inputs, float64 oracle (out, grads), float32 eager errors {quantity: max |err|})."""
    c = next(k for k in CASES if k.name == name)
    d = edge_inputs(c)
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
    path = os.environ.get("GNNQC_EDGE_REPORT")
    if path and _REPORT:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("# tests/test_edge_kernels_gpu.py: measured |err| of edge_pool on the device against the float64\n"
                    f"# oracle, the float32 eager layer's own error (e32) and the bound (max of {K_FLOOR_MULT:g} x e32 and\n"
                    "# the floor: 1e-4 + 1e-4 |ref| on outputs, 1e-3 max|ref| on gradients; 'out' lists err / bound).\n"
                    f"# {'case':<28} {'quantity':<8} {'err':>11} {'e32':>11} {'bound':>11}\n")
            f.write("\n".join(_REPORT) + "\n")


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_edge_case_matches_float64(cuda_device, name):
    """Output, dx, danom, dW, dbias, dalpha of one case against float64 eager, within the measured
    bound; time-major cases: padding rows and channels exactly zero; the cases off the HIP path run
    the eager layer on the device."""
    from gnnqc.ops import gcn as G
    c, d, (out64, g64), e32 = reference(name)
    dev = cuda_device
    layer_dev = copy.deepcopy(d["layer"]).to(dev)
    assert G.edge_pool_hip_ok(d["x"].to(dev), layer_dev, c.pooling) == ("eager" not in c.tags)
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


def test_edge_time_major_needs_the_hip_path(cuda_device):
    """edge_pool(time_major=True) returns the kernel's own [T, Mp, Cp] tensor on the HIP path and
    raises off it (the eager layer has no time-major form)."""
    from gnnqc.ops import gcn as G
    c, d, _, _ = reference("tm_b5")
    dev = cuda_device
    layer = copy.deepcopy(d["layer"]).to(dev)
    args = [d[k].to(dev) for k in ("x", "adj", "mask", "anom", "anom_pos")]
    h, Bret = G.edge_pool(*args, layer, c.pooling, time_major=True)
    assert Bret == c.B and tuple(h.shape) == (c.T, *time_major_pad(c))
    layer.aggregate = "max"
    with pytest.raises(ValueError):
        G.edge_pool(*args, layer, c.pooling, time_major=True)


def test_edge_forward_and_backward_are_bitwise_reproducible(cuda_device):
    """Two runs of the multi-pass cases give bitwise-equal outputs and gradients (fixed-order record
    sum, no float atomics)."""
    for name in ("passes", "passes_tm"):
        c, d, _, _ = reference(name)
        a = run_eager(c, d, torch.float32, cuda_device)
        b = run_eager(c, d, torch.float32, cuda_device)
        assert torch.equal(a[0], b[0])
        for k in a[1]:
            assert torch.equal(a[1][k], b[1][k]), (name, k)
