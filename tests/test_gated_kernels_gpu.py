"""The fused GatedGraphConv kernels (``csrc/kernels/gated.hip``) over their shape and dispatch
space, against the float64 eager layer on the CPU.

Every case runs :func:`gnnqc.ops.gcn.gated_pool` on the device and compares the output, ``dx``,
``danom``, each ``dW_l``, ``dK``, ``dR``, ``dbias`` and ``dalpha`` with ``GatedGraphConv`` +
``pool_nodes`` + ``cat`` in float64 (:func:`gnnqc.ops.gcn.gated_pool_eager`, autograd on the float64
graph).

The bound is measured per case and quantity, by the rule of ``tests/test_agnn_kernels_gpu.py``. The
yardstick is the error of the SAME eager layer run in float32 on the CPU against that float64 oracle
(``e32``); the kernel may be ``K_FLOOR_MULT = 4`` times as far off. The bound never drops below the
floor: ``1e-4 + 1e-4 |ref|`` per output element, ``1e-3 max|ref|`` on a gradient.

Kinks. The activation acts on a GRU state, so no lattice keeps it off zero. For PReLU / ReLU cases
:func:`reference` finds, in the float64 oracle, every (window, step, channel) where some node has
``|h_ic^L| < eps`` with ``eps = max(1e-4, 8 x the case's float32 error of h^L)`` and sets the upstream
gradient of that pooled channel to zero, for the kernel and the oracle alike: ``dh^L_ic = pw_i
act'(h_ic) dout[b, t, c]``, so a branch flipped by float32 rounding reaches no gradient. The forward
output is compared everywhere. ``tests/test_gated_reference_cpu.py`` asserts that at most 5 % of a
case's entries are zeroed.

Each case names the branches it is there to reach (``tags``); the CPU file recomputes their
predicates from the shapes, checks the oracle and the kernel's math in float64, and checks that
named mutants of that math lie at least 5 bounds away.

With ``GNNQC_GATED_REPORT=<path>`` the measured error and bound of every case and quantity are
written there (``profiles/gated_kernel_tests.txt`` is such a run).
"""
import copy
import functools
import os
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------ constants of the kernels
K_MAX_N = 64                # gated.hip GATED_MAX_N (one 64-bit neighbour word per node)
K_WIDTHS = (8, 16, 32)      # gated.hip GQ_GATED_DISPATCH
K_MAX_L = 4                 # gated.hip GATED_MAX_L
K_THREADS = 256             # gated.hip: lanes per workgroup; rows per workgroup = 256 / pow2(N)
K_GRID_CAP = 256            # gated.hip GATED_GRID_CAP (more row blocks: several passes per workgroup)
K_FLOOR_MULT = 4.0          # allowed kernel error / float32 eager error (see the module docstring)
OUT_ATOL = OUT_RTOL = 1e-4  # the floor on outputs
GRAD_REL = 1e-3             # the floor on gradients, relative to max |ref|
KINK_EPS = 1e-4             # |h^L| below max(this, 8 e32(h^L)): the pooled channel's dout is zeroed
KINK_SHARE = 0.05           # at most this share of a case's (window, step, channel) entries

GatedCase = namedtuple("GatedCase", "name B T N Cin C L pooling tm Ca training act kind grads tags")


def _gc(name, B=5, T=11, N=9, Cin=2, C=16, L=2, pooling="mean", tm=False, Ca=2, training=True, act="prelu", kind="",
        grads="all", tags=()):
    return GatedCase(name, B, T, N, Cin, C, L, pooling, tm, Ca, training, act, kind, grads, tuple(tags))


def _cases():
    cs = []
    for Cin in (1, 2, 3, 4):
        for C in K_WIDTHS:
            cs.append(_gc(f"inst_c{Cin}_w{C}", Cin=Cin, C=C, pooling="selection" if Cin % 2 else "mean",
                          tags=("hip", "np_gt_n", "ragged_rows", "asymmetric", "diagonal")
                          + (("pad_tile",) if C < 16 else ()) + (("four_tiles",) if C == 32 else ())))
    for L in (1, 2, 3, 4):
        cs.append(_gc(f"layers_{L}", L=L, tags=("hip", "rewalk") if L > 1 else ("hip", "one_layer")))
    cs += [
        _gc("layers_4_w32", L=4, C=32, tags=("hip", "rewalk", "four_tiles", "limit_layers")),
        _gc("nodes_1", N=1, tags=("hip", "single_node", "one_pass")),
        _gc("nodes_7", N=7, tags=("hip", "np_gt_n")),
        _gc("nodes_33", N=33, tags=("hip", "two_words", "np_gt_n")),
        _gc("nodes_64_selection", N=64, pooling="selection", tags=("hip", "two_words", "limit")),
        _gc("nodes_64_dense", N=64, kind="dense", C=32, tags=("hip", "two_words", "limit", "dense", "four_tiles")),
        _gc("rows_ragged", B=3, T=7, N=5, tags=("hip", "ragged_rows", "one_pass")),
        _gc("passes", B=48, T=181, N=7, tags=("hip", "multi_pass", "many_records", "np_gt_n")),
        _gc("passes_tm", B=48, T=181, N=7, tm=True, pooling="selection", tags=("hip", "multi_pass", "many_records")),
        _gc("tm_b5", B=5, tm=True, Cin=3, tags=("hip", "tm_pad_rows", "tm_pad_ch")),
        _gc("tm_b16", B=16, tm=True, Ca=4, tags=("hip", "tm_full_rows", "tm_full_ch")),
        _gc("tm_b17_selection", B=17, tm=True, pooling="selection", Cin=1, tags=("hip", "tm_pad_rows", "tm_pad_ch")),
        _gc("no_anom", Ca=0, tags=("hip", "no_anom")),
        _gc("no_anom_tm", B=17, Ca=0, tm=True, Cin=4, tags=("hip", "no_anom", "tm_pad_rows", "tm_full_ch")),
        _gc("no_anom_tm_w8", B=5, Ca=0, tm=True, C=8, tags=("hip", "no_anom", "tm_pad_rows", "tm_full_ch", "pad_tile")),
        _gc("tm_w8_anom", B=16, Ca=2, tm=True, C=8, L=1, tags=("hip", "tm_full_rows", "tm_pad_ch", "pad_tile",
                                                             "one_layer")),
        _gc("pool_sum", pooling="sum", tags=("hip", "pool_sum")),
        _gc("pool_sum_tm", pooling="sum", tm=True, B=17, tags=("hip", "pool_sum", "tm_pad_rows")),
        _gc("act_linear", act=None, tags=("hip", "act_linear")),
        _gc("act_relu", act="relu", pooling="selection", tags=("hip", "act_relu")),
        _gc("eval_mode", training=False, tags=("hip", "eval")),
        _gc("no_diagonal", kind="plain", tags=("hip", "asymmetric")),
        _gc("grads_some", grads="some", tags=("hip", "some_param_grads")),
        _gc("grads_none", grads="none", tags=("hip", "no_param_grad")),
    ]
    for pooling in ("mean", "sum", "selection"):
        cs.append(_gc(f"degenerate_{pooling}", pooling=pooling, kind="degenerate", tags=("hip", "degenerate")))
    cs += [
        _gc("zeros", kind="zeros", tags=("hip", "exact_zeros")),
        # not on the HIP path: gated_pool() must take the eager layer on the device
        _gc("eager_nodes_65", B=2, T=3, N=65, tags=("eager",)),
        _gc("eager_width_12", C=12, tags=("eager",)),
        _gc("eager_layers_5", L=5, tags=("eager",)),
        _gc("eager_pool_max", pooling="max", tags=("eager",)),
        _gc("eager_act_tanh", act="tanh", tags=("eager",)),
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
    """(Mp, Cp) of gated_pool(time_major=True)."""
    Cp = c.Ca + c.C
    return _cdiv(c.B, 16) * 16, Cp + (-Cp) % 4


def on_hip_path(c):
    """The conditions of gated_pool_hip_ok, from the case's shape alone."""
    return (1 <= c.N <= K_MAX_N and 1 <= c.Cin <= 4 and c.Cin <= c.C and c.C in K_WIDTHS and 1 <= c.L <= K_MAX_L
            and c.pooling in ("mean", "sum", "selection") and c.act in (None, "linear", "prelu", "relu"))


PREDICATES = {
    "hip": on_hip_path,
    "eager": lambda c: not on_hip_path(c),
    "np_gt_n": lambda c: _pow2(c.N) > c.N,
    "single_node": lambda c: c.N == 1,
    "two_words": lambda c: c.N > 32,
    "limit": lambda c: c.N == K_MAX_N,
    "dense": lambda c: c.kind == "dense" and c.N == K_MAX_N,
    "pad_tile": lambda c: c.C < 16,
    "four_tiles": lambda c: c.C == 32,
    "one_layer": lambda c: c.L == 1,
    "rewalk": lambda c: c.L > 1,
    "limit_layers": lambda c: c.L == K_MAX_L and c.C == 32,
    "one_pass": lambda c: _cdiv(c.B * c.T, rows_per_workgroup(c)) <= K_GRID_CAP,
    "multi_pass": lambda c: _cdiv(c.B * c.T, rows_per_workgroup(c)) > K_GRID_CAP,
    "many_records": lambda c: min(K_GRID_CAP, _cdiv(c.B * c.T, rows_per_workgroup(c))) >= 128,
    "ragged_rows": lambda c: (c.B * c.T) % rows_per_workgroup(c) != 0,
    "tm_pad_rows": lambda c: c.tm and time_major_pad(c)[0] > c.B,
    "tm_full_rows": lambda c: c.tm and time_major_pad(c)[0] == c.B,
    "tm_pad_ch": lambda c: c.tm and time_major_pad(c)[1] > c.Ca + c.C,
    "tm_full_ch": lambda c: c.tm and time_major_pad(c)[1] == c.Ca + c.C,
    "no_anom": lambda c: c.Ca == 0,
    "pool_sum": lambda c: c.pooling == "sum",
    "asymmetric": lambda c: c.kind in ("", "plain") and c.N >= 5,
    "diagonal": lambda c: c.kind == "" and c.B >= 2,
    "degenerate": lambda c: c.kind == "degenerate" and c.B >= 5 and c.N >= 6,
    "exact_zeros": lambda c: c.kind == "zeros",
    "act_linear": lambda c: c.act in (None, "linear"),
    "act_relu": lambda c: c.act == "relu",
    "eval": lambda c: not c.training,
    "some_param_grads": lambda c: c.grads == "some",
    "no_param_grad": lambda c: c.grads == "none",
}

FROZEN = {"all": (), "some": ("K", "R", "alpha"), "none": ("kernel", "K", "R", "bias", "alpha")}


# ------------------------------------------------------------------ input builder (CPU, float32)
def gated_inputs(c):
    """Inputs and the layer of a case on the CPU. Random masks (every sample keeps a node),
    ``anom_pos`` among the valid nodes, a random ASYMMETRIC 0/1 adjacency between valid nodes whose
    diagonal is set only in every other sample (the layer adds no self loop: a diagonal entry is an
    edge like any other), ``x`` = randn on valid nodes. ``kind``:

    * ``plain``: no diagonal entries at all;
    * ``dense``: every pair of valid nodes is an edge, the diagonal included;
    * ``degenerate``: sample 0 has every node masked and ``anom_pos = -1``; sample 1 a single valid
      node; sample 2 a valid, flagged node (3) without any edge (m = 0) and in nobody's
      neighbourhood; sample 3 keeps adjacency entries from valid nodes TOWARDS its masked nodes;
      every masked node holds 2.5 (a value that reaches its neighbours but does not saturate the gates);
    * ``zeros``: ``x`` is zero everywhere (the states then come from the biases alone).
    """
    from gnnqc.models.graphconv import GatedGraphConv
    gen = torch.Generator().manual_seed(7000 + [k.name for k in CASES].index(c.name))
    B, T, N, Cin = c.B, c.T, c.N, c.Cin
    x = torch.randn(B, T, N, Cin, generator=gen)
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
    if c.kind != "plain":
        adj[::2] += torch.eye(N)
    if c.kind == "dense":
        adj = torch.ones(B, N, N)
    keep = adj.clone()
    adj = adj * mask[:, :, None] * mask[:, None, :]
    if c.kind == "degenerate":
        adj[2, 3, :] = 0
        adj[2, :, 3] = 0
        adj[3] = keep[3] * mask[3, :, None]                  # rows of valid nodes keep their masked neighbours
        adj[3, 0, 2] = 1
    x = x * mask[:, None, :, None]
    if c.kind == "zeros":
        x = torch.zeros_like(x)
    if c.kind == "degenerate":
        x = x + 2.5 * (1 - mask)[:, None, :, None]
    anom_pos = torch.full((B,), -1, dtype=torch.long)
    for b in range(B):
        valid = mask[b].nonzero().flatten()
        if valid.numel():
            anom_pos[b] = valid[int(torch.randint(valid.numel(), (1,), generator=gen))]
    if c.kind == "degenerate":
        anom_pos[2] = 3
    torch.manual_seed(7000 + len(c.name))
    layer = GatedGraphConv(Cin, c.C, c.L, c.act)
    with torch.no_grad():                                    # (Keras starts the biases at zero: make them count)
        layer.rnn.bias.copy_(torch.randn(layer.rnn.bias.shape, generator=gen) * 0.3)
        if layer.prelu_alpha is not None:
            layer.prelu_alpha.copy_(0.05 + torch.rand(layer.prelu_alpha.shape, generator=gen) * 0.3)
    ps = layer_params(layer)
    for k in FROZEN[c.grads]:
        if k in ps:
            ps[k].requires_grad_(False)
    layer.train(c.training)
    anom = torch.randn(B, T, c.Ca, generator=gen) if c.Ca else None
    Mp, Cp = time_major_pad(c)
    gshape = (T, Mp, Cp) if c.tm else (B, T, c.Ca + c.C)
    return dict(x=x, adj=adj, mask=mask, anom=anom, anom_pos=anom_pos, layer=layer,
                g=torch.randn(gshape, generator=gen))


def layer_params(layer):
    """{quantity name: parameter} of a GatedGraphConv."""
    ps = {"kernel": layer.kernel, "K": layer.rnn.kernel, "R": layer.rnn.recurrent_kernel, "bias": layer.rnn.bias}
    if layer.prelu_alpha is not None:
        ps["alpha"] = layer.prelu_alpha
    return ps


def final_state(layer, x, adj):
    """h^L [B, T, N, C] of the eager layer: its forward without the activation and the mask."""
    h = F.pad(x, (0, layer.channels - x.shape[-1]))
    for i in range(layer.n_layers):
        h = layer.rnn(torch.einsum("bij,btjf->btif", adj, h @ layer.kernel[i]), h)
    return h


def kink_mask(c, d):
    """[B, T, C] bool: pooled channels whose upstream gradient is zeroed (module docstring, Kinks),
    and the eps used. All False for the linear activation."""
    with torch.no_grad():
        h64 = final_state(copy.deepcopy(d["layer"]).double(), d["x"].double(), d["adj"].double())
        h32 = final_state(d["layer"], d["x"], d["adj"]).double()
    eps = max(KINK_EPS, 8.0 * (h32 - h64).abs().max().item())
    if c.act not in ("prelu", "relu"):
        return torch.zeros(c.B, c.T, c.C, dtype=torch.bool), eps
    return (h64.abs() < eps).any(dim=2), eps


def split_kernel(grads, L):
    """``kernel`` [L, C, C] -> ``W0`` .. ``W{L-1}``: each layer's gradient has its own scale."""
    out = {k: v for k, v in grads.items() if k != "kernel"}
    for l in range(L):
        out[f"W{l}"] = grads["kernel"][l] if grads["kernel"].numel() else grads["kernel"]
    return out


def run_eager(c, d, dtype, device="cpu", eager_on_device=False):
    """``gated_pool_eager`` (or ``gated_pool`` on a device) in ``dtype``: the output as [B, T, Fo]
    and the gradients of x, anom and every parameter for the case's upstream gradient ``d['g']``, as
    float64 CPU tensors. Returns ``(out, grads, raw output)``."""
    from gnnqc.ops import gcn as G
    layer = copy.deepcopy(d["layer"]).to(device=device, dtype=dtype)
    x = d["x"].to(device=device, dtype=dtype).clone().requires_grad_(True)          # (clone: a fresh leaf)
    anom = d["anom"].to(device=device, dtype=dtype).clone().requires_grad_(True) if d["anom"] is not None else None
    args = (x, d["adj"].to(device=device, dtype=dtype), d["mask"].to(device=device, dtype=dtype), anom,
            d["anom_pos"].to(device), layer, c.pooling)
    Fo = c.Ca + c.C
    if device == "cpu" or eager_on_device:
        raw = out = G.gated_pool_eager(*args)
        g = d["g"][:, :c.B, :Fo].transpose(0, 1) if c.tm else d["g"]
    else:
        raw = G.gated_pool(*args, time_major=c.tm)
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
    return out.detach().double().cpu(), split_kernel(grads, c.L), raw.detach()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, inputs with the kinked channels of ``g`` zeroed, float64 oracle (out, grads), float32
    eager errors {quantity: max |err|}, (share of zeroed entries, eps))."""
    c = next(k for k in CASES if k.name == name)
    d = gated_inputs(c)
    kink, eps = kink_mask(c, d)
    if c.tm:
        d["g"][:, :c.B, c.Ca:c.Ca + c.C][kink.transpose(0, 1)] = 0
    else:
        d["g"][..., c.Ca:][kink] = 0
    out64, g64, _ = run_eager(c, d, torch.float64)
    out32, g32, _ = run_eager(c, d, torch.float32)
    e32 = {"out": (out32 - out64).abs().max().item()}
    for k in g64:
        e32[k] = (g32[k] - g64[k]).abs().max().item() if g64[k].numel() else 0.0
    return c, d, (out64, g64), e32, (kink.float().mean().item(), eps)


def out_bound(ref, e32):
    return torch.clamp(OUT_ATOL + OUT_RTOL * ref.abs(), min=K_FLOOR_MULT * e32)


def out_excess(got, ref, e32):
    """max over elements of |got - ref| / bound, bound = max(K e32, 1e-4 + 1e-4 |ref|); inf if
    ``got`` is not finite. <= 1 passes."""
    if not torch.isfinite(got).all():
        return float("inf")
    return ((got - ref).abs() / out_bound(ref, e32)).max().item() if ref.numel() else 0.0


def out_worst(got, ref, e32):
    """(|got - ref|, bound) at the output element of the largest |got - ref| / bound (the report's row)."""
    if not ref.numel() or not torch.isfinite(got).all():
        return float("nan"), float("nan")
    bound = out_bound(ref, e32)
    err = (got - ref).abs()
    i = int((err / bound).argmax())
    return err.reshape(-1)[i].item(), bound.reshape(-1)[i].item()


def _ratio(err, bound):
    return err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))


def grad_bound(ref, e32):
    """The bound on a gradient: max(4 e32, 1e-3 max|ref|)."""
    if not ref.numel():                                     # (a frozen parameter: nothing to compare)
        return 0.0
    return max(K_FLOOR_MULT * e32, GRAD_REL * (ref.abs().max().item() + 1e-6))


_REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _report_file():
    yield
    path = os.environ.get("GNNQC_GATED_REPORT")
    if path and _REPORT:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("# tests/test_gated_kernels_gpu.py: measured |err| of gated_pool on the device against the float64\n"
                    f"# oracle, the float32 eager layer's own error (e32) and the bound (max of {K_FLOOR_MULT:g} x e32 and\n"
                    "# the floor: 1e-4 + 1e-4 |ref| on outputs, 1e-3 max|ref| on gradients; the 'out' row gives err and\n"
                    "# bound at the element of the largest err / bound). err / bound <= 1 passes.\n"
                    f"# {'case':<28} {'quantity':<8} {'err':>11} {'e32':>11} {'bound':>11} {'err/bound':>11}\n")
            f.write("\n".join(_REPORT) + "\n")


@pytest.mark.parametrize("name", [c.name for c in CASES if "hip" in c.tags])
def test_gated_case_matches_float64(cuda_device, name):
    """Output, dx, danom, every dW_l, dK, dR, dbias, dalpha of one case against float64 eager, within
    the measured bound; time-major cases: padding rows and channels exactly zero; a frozen parameter
    gets no gradient."""
    from gnnqc.ops import gcn as G
    c, d, (out64, g64), e32, _ = reference(name)
    dev = cuda_device
    layer_dev = copy.deepcopy(d["layer"]).to(dev)
    assert G.gated_pool_hip_ok(d["x"].to(dev), layer_dev, c.pooling)
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
    werr, wbound = out_worst(out, out64, e32["out"])
    _REPORT.append(f"{c.name:<30} {'out':<8} {werr:11.3e} {e32['out']:11.3e} {wbound:11.3e} {ex:11.3e}")
    print(_REPORT[-1])
    fails = [] if ex <= 1.0 else [f"out: err / bound = {ex:.3f}"]
    assert set(grads) == set(g64)
    for k, ref in g64.items():
        assert grads[k].shape == ref.shape, (k, grads[k].shape, ref.shape)
        got = grads[k]
        err = (got - ref).abs().max().item() if ref.numel() else 0.0
        bound = grad_bound(ref, e32[k])
        _REPORT.append(f"{c.name:<30} {'d' + k:<8} {err:11.3e} {e32[k]:11.3e} {bound:11.3e} "
                       f"{_ratio(err, bound):11.3e}")
        print(_REPORT[-1])
        if not (err <= bound) or not torch.isfinite(got).all():
            fails.append(f"d{k}: err {err:.3e} > bound {bound:.3e}")
    assert not fails, f"{c.name}: " + "; ".join(fails)


@pytest.mark.parametrize("name", [c.name for c in CASES if "eager" in c.tags])
def test_gated_off_the_hip_path_is_the_eager_layer(cuda_device, name):
    """N = 65, C = 12, n_layers = 5, pooling max, activation tanh: gated_pool takes the eager layer on
    the device and agrees with it exactly, output and gradients."""
    from gnnqc.ops import gcn as G
    c, d, _, _, _ = reference(name)
    dev = cuda_device
    assert not G.gated_pool_hip_ok(d["x"].to(dev), copy.deepcopy(d["layer"]).to(dev), c.pooling)
    a = run_eager(c, d, torch.float32, dev)
    b = run_eager(c, d, torch.float32, dev, eager_on_device=True)
    assert torch.isfinite(a[0]).all() and torch.equal(a[0], b[0])
    assert set(a[1]) == set(b[1])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k


def test_gated_time_major_needs_the_hip_path(cuda_device):
    """gated_pool(time_major=True) returns the kernel's own [T, Mp, Cp] tensor on the HIP path and
    raises off it (the eager layer has no time-major form)."""
    from gnnqc.ops import gcn as G
    c, d, _, _, _ = reference("tm_b5")
    dev = cuda_device
    layer = copy.deepcopy(d["layer"]).to(dev)
    args = [d[k].to(dev) for k in ("x", "adj", "mask", "anom", "anom_pos")]
    h, Bret = G.gated_pool(*args, layer, c.pooling, time_major=True)
    assert Bret == c.B and tuple(h.shape) == (c.T, *time_major_pad(c))
    with pytest.raises(ValueError):
        G.gated_pool(*args, layer, "max", time_major=True)


def test_gated_frozen_parameter_launches(cuda_device, monkeypatch):
    """With no parameter needing a gradient gated_pool_bwd is not launched; with only some needing
    one it is, and the frozen ones still get no gradient (test_gated_case_matches_float64)."""
    from gnnqc.utils import native
    real = native.hip_ops()
    calls = []

    class Rec:
        def __getattr__(self, n):
            f = getattr(real, n)
            return (lambda *a, **k: calls.append(n) or f(*a, **k)) if n.startswith(("gated_", "edge_")) else f

    monkeypatch.setattr(native, "hip_ops", lambda: Rec())
    for name, want in (("grads_none", False), ("grads_some", True), ("layers_2", True)):
        c, d, _, _, _ = reference(name)
        calls.clear()
        _, grads, _ = run_eager(c, d, torch.float32, cuda_device)
        assert calls[:2] == ["edge_adj_bits", "gated_pool_fwd"] and "gated_pool_bwd_input" in calls, calls
        assert ("gated_pool_bwd" in calls) == want and ("gated_bwd_finalize" in calls) == want, (name, calls)
        for k in FROZEN[c.grads]:
            assert grads["W0" if k == "kernel" else k].numel() == 0, (name, k)


def test_gated_forward_and_backward_are_bitwise_reproducible(cuda_device):
    """Two runs of the multi-pass cases give bitwise-equal outputs and gradients (fixed-order record
    sum, no float atomics)."""
    for name in ("passes", "passes_tm"):
        c, d, _, _, _ = reference(name)
        a = run_eager(c, d, torch.float32, cuda_device)
        b = run_eager(c, d, torch.float32, cuda_device)
        assert torch.equal(a[0], b[0])
        for k in a[1]:
            assert torch.equal(a[1][k], b[1][k]), (name, k)
