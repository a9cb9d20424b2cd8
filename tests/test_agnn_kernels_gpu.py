"""The fused AGNNConv kernels (``csrc/kernels/agnn.hip``) over their shape and dispatch space,
against the float64 eager layer on the CPU.

Every case runs :func:`gnnqc.ops.gcn.agnn_pool` on the device and compares the output, ``dx``,
``danom``, ``dbeta`` and ``dalpha`` with ``AGNNConv`` + ``pool_nodes`` + ``cat`` in float64
(:func:`gnnqc.ops.gcn.agnn_pool_eager`, autograd on the float64 graph).

The bound is measured per case and quantity, by the rule of ``tests/test_gat_kernels_gpu.py`` and
``tests/test_edge_kernels_gpu.py``. The yardstick is the error of the SAME eager layer run in
float32 on the CPU against that float64 oracle (``e32``); the kernel may be ``K_FLOOR_MULT = 4``
times as far off. The bound never drops below the floor: ``1e-4 + 1e-4 |ref|`` per output element,
``1e-3 max|ref|`` on a gradient. ``dbeta`` is ONE scalar sum over every row, node and edge, with
cancellation (for Cin = 1 and one sign per row every cosine is 1, the softmax is flat and ``dbeta``
vanishes identically), so its floor is ``1e-3 |ref| + 2^-20 A`` with ``A`` the float64 sum of
``|ds_ij <xn_i, xn_j>|``: 16 float32 ulps of the summands' mass (:func:`dbeta_mass`). ``dx`` is
compared in two groups, nodes of zero norm and the rest, each against its own ``max|ref|``: the
normalisation's clamp puts a factor ``1 / 1e-12`` on a zero-norm node's gradient, which must not
hide the other nodes' errors (``zero_norm``).

Kinks. The activation acts on ``o_i``, a softmax-weighted mean of neighbour values, so no lattice
makes it exact. Cases with PReLU or ReLU instead draw ``x[b, t, j, c] = sign[b, t, c] (0.25 +
|randn|)``: one random sign per (window, step, channel), shared by the row's nodes. ``o_ic`` is then
a convex combination (divided by the degree under ``mean``) of values of one sign, so
``|o_ic| >= 0.25 / 64`` for every node with a neighbour, and both branches occur because the signs
vary over rows and channels. ``tests/test_agnn_reference_cpu.py`` asserts the resulting margin for
every such case except ``zeros``, which holds exact zeros by construction and pins the branch taken
AT zero. Cases with free-sign ``x`` (negative cosines) use the linear activation.

Each case names the branches it is there to reach (``tags``); the CPU file recomputes their
predicates from the shapes, checks the oracle and the kernel's math in float64, and checks that
named mutants of that math lie at least 5 bounds away.

With ``GNNQC_AGNN_REPORT=<path>`` the measured error and bound of every case and quantity are
written there (``profiles/agnn_kernel_tests.txt`` is such a run).
"""
import copy
import functools
import os
from collections import namedtuple

import pytest
import torch

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------ constants of the kernels
K_MAX_N = 64                # agnn.hip AGNN_MAX_N (one 64-bit neighbour word per node)
K_THREADS = 256             # agnn.hip: lanes per workgroup; rows per workgroup = 256 / pow2(N)
K_GRID_CAP = 256            # agnn.hip AGNN_GRID_CAP (more row blocks: several passes per workgroup)
K_EPS = 1e-12               # F.normalize's clamp (agnn.hip AGNN_EPS)
K_FLOOR_MULT = 4.0          # allowed kernel error / float32 eager error (see the module docstring)
OUT_ATOL = OUT_RTOL = 1e-4  # the floor on outputs
GRAD_REL = 1e-3             # the floor on gradients, relative to max |ref|
DBETA_MASS = 2.0 ** -20     # the floor on dbeta: 16 float32 ulps of sum |ds_ij cos_ij|

AgnnCase = namedtuple("AgnnCase", "name B T N Cin agg pooling tm anom training act beta trainable kind xkind tags")


def _ac(name, B=5, T=11, N=9, Cin=2, agg="sum", pooling="mean", tm=False, anom=True, training=True, act="prelu",
        beta=4.0, trainable=True, kind="", xkind=None, tags=()):
    if xkind is None:
        xkind = "sign" if act in ("prelu", "relu") else "free"
    return AgnnCase(name, B, T, N, Cin, agg, pooling, tm, anom, training, act, beta, trainable, kind, xkind,
                    tuple(tags))


def _cases():
    cs = []
    for Cin in (1, 2, 3, 4):
        for agg in ("sum", "mean"):
            for pooling in ("mean", "selection"):
                cs.append(_ac(f"inst_c{Cin}_{agg}_{pooling}", Cin=Cin, agg=agg, pooling=pooling,
                              tags=("hip", "np_gt_n", "ragged_rows") + (("packed",) if Cin <= 2 else ("two_slabs",))))
    cs += [
        _ac("nodes_1", N=1, agg="mean", tags=("hip", "single_node", "one_pass")),
        _ac("nodes_7", N=7, agg="mean", tags=("hip", "np_gt_n")),
        _ac("nodes_33", N=33, tags=("hip", "two_words", "np_gt_n")),
        _ac("nodes_64", N=64, agg="sum", tags=("hip", "two_words", "limit")),
        _ac("nodes_64_mean", N=64, agg="mean", Cin=3, tags=("hip", "two_words", "limit", "two_slabs")),
        _ac("nodes_64_selection", N=64, pooling="selection", agg="mean", tags=("hip", "two_words", "limit")),
        _ac("rows_ragged", B=3, T=7, N=5, agg="mean", tags=("hip", "ragged_rows", "one_pass")),
        _ac("passes", B=48, T=181, N=7, agg="mean", tags=("hip", "multi_pass", "many_records", "np_gt_n")),
        _ac("passes_tm", B=48, T=181, N=7, tm=True, pooling="selection", tags=("hip", "multi_pass", "many_records")),
        _ac("tm_b5", B=5, tm=True, agg="mean", Cin=3, tags=("hip", "tm_pad_rows", "tm_pad_ch", "two_slabs")),
        _ac("tm_b16", B=16, tm=True, tags=("hip", "tm_full_rows", "tm_full_ch")),
        _ac("tm_b17_selection", B=17, tm=True, pooling="selection", Cin=1, tags=("hip", "tm_pad_rows", "tm_pad_ch")),
        _ac("no_anom", anom=False, tags=("hip", "no_anom")),
        _ac("no_anom_tm", B=17, anom=False, tm=True, agg="mean", Cin=4,
            tags=("hip", "no_anom", "tm_pad_rows", "tm_full_ch", "two_slabs")),
        _ac("no_anom_tm_pad", B=5, anom=False, tm=True, tags=("hip", "no_anom", "tm_pad_rows", "tm_pad_ch")),
        _ac("pool_sum", pooling="sum", agg="mean", tags=("hip", "pool_sum")),
        _ac("pool_sum_tm", pooling="sum", tm=True, B=17, tags=("hip", "pool_sum", "tm_pad_rows")),
        _ac("act_linear", act=None, agg="mean", tags=("hip", "act_linear", "free_sign")),
        _ac("act_relu", act="relu", pooling="selection", tags=("hip", "act_relu")),
        _ac("eval_mode", training=False, agg="mean", tags=("hip", "eval")),
        _ac("beta_30", beta=30.0, agg="mean", tags=("hip", "large_beta")),
        _ac("beta_30_free", beta=30.0, act=None, Cin=3, tags=("hip", "large_beta", "free_sign", "act_linear",
                                                             "two_slabs")),
        _ac("beta_neg3", beta=-3.0, act=None, tags=("hip", "negative_beta", "free_sign", "act_linear")),
        _ac("beta_0", beta=0.0, agg="mean", tags=("hip", "flat_softmax")),
        _ac("beta_frozen", trainable=False, tags=("hip", "frozen_beta")),
        _ac("beta_frozen_linear", trainable=False, act=None, tags=("hip", "frozen_beta", "no_param_grad",
                                                                  "act_linear", "free_sign")),
    ]
    for pooling, agg in (("mean", "mean"), ("sum", "sum"), ("selection", "mean")):
        cs.append(_ac(f"degenerate_{pooling}", pooling=pooling, agg=agg, kind="degenerate",
                      tags=("hip", "degenerate")))
    cs += [
        _ac("zeros", kind="zeros", tags=("hip", "exact_zeros")),
        _ac("zero_norm", kind="zero_norm", act=None, tags=("hip", "zero_norm", "act_linear", "free_sign")),
        # not on the HIP path: agnn_pool() must take the eager layer on the device
        _ac("eager_nodes_65", B=2, T=3, N=65, tags=("eager",)),
        _ac("eager_agg_max", agg="max", tags=("eager",)),
        _ac("eager_pool_max", pooling="max", tags=("eager",)),
        _ac("eager_act_tanh", act="tanh", xkind="free", tags=("eager",)),
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
    """(Mp, Cp) of agnn_pool(time_major=True)."""
    Cp = (c.Cin if c.anom else 0) + c.Cin
    return _cdiv(c.B, 16) * 16, Cp + (-Cp) % 4


def on_hip_path(c):
    """The conditions of agnn_pool_hip_ok, from the case's shape alone."""
    return (1 <= c.N <= K_MAX_N and 1 <= c.Cin <= 4 and c.pooling in ("mean", "sum", "selection")
            and c.agg in ("sum", "mean") and c.act in (None, "linear", "prelu", "relu"))


PREDICATES = {
    "hip": on_hip_path,
    "eager": lambda c: not on_hip_path(c),
    "np_gt_n": lambda c: _pow2(c.N) > c.N,
    "single_node": lambda c: c.N == 1,
    "two_words": lambda c: c.N > 32,
    "limit": lambda c: c.N == K_MAX_N,
    "packed": lambda c: c.Cin <= 2,
    "two_slabs": lambda c: c.Cin > 2,
    "one_pass": lambda c: _cdiv(c.B * c.T, rows_per_workgroup(c)) <= K_GRID_CAP,
    "multi_pass": lambda c: _cdiv(c.B * c.T, rows_per_workgroup(c)) > K_GRID_CAP,
    "many_records": lambda c: min(K_GRID_CAP, _cdiv(c.B * c.T, rows_per_workgroup(c))) >= 128,
    "ragged_rows": lambda c: (c.B * c.T) % rows_per_workgroup(c) != 0,
    "tm_pad_rows": lambda c: c.tm and time_major_pad(c)[0] > c.B,
    "tm_full_rows": lambda c: c.tm and time_major_pad(c)[0] == c.B,
    "tm_pad_ch": lambda c: c.tm and time_major_pad(c)[1] > (c.Cin if c.anom else 0) + c.Cin,
    "tm_full_ch": lambda c: c.tm and time_major_pad(c)[1] == (c.Cin if c.anom else 0) + c.Cin,
    "no_anom": lambda c: not c.anom,
    "pool_sum": lambda c: c.pooling == "sum",
    "degenerate": lambda c: c.kind == "degenerate" and c.B >= 5 and c.N >= 6,
    "exact_zeros": lambda c: c.kind == "zeros" and c.act == "prelu",
    "zero_norm": lambda c: c.kind == "zero_norm" and c.act in (None, "linear") and c.B >= 2 and c.N >= 3,
    "act_linear": lambda c: c.act in (None, "linear"),
    "act_relu": lambda c: c.act == "relu",
    "free_sign": lambda c: c.xkind == "free" and c.act in (None, "linear"),
    "eval": lambda c: not c.training,
    "large_beta": lambda c: c.beta >= 30,
    "negative_beta": lambda c: c.beta < 0 and c.xkind == "free",
    "flat_softmax": lambda c: c.beta == 0,
    "frozen_beta": lambda c: not c.trainable,
    "no_param_grad": lambda c: not c.trainable and c.act != "prelu",
}


# ------------------------------------------------------------------ input builder (CPU, float32)
def agnn_inputs(c):
    """Inputs and the layer of a case on the CPU. Random masks (every sample keeps a node),
    ``anom_pos`` among the valid nodes, a random ASYMMETRIC 0/1 adjacency between valid nodes whose
    diagonal is set only in every other sample (the layer adds no self loop). ``xkind``: ``sign`` -
    one sign per (window, step, channel) and magnitudes 0.25 + |randn| (module docstring, Kinks);
    ``free`` - randn. ``kind``:

    * ``degenerate``: sample 0 has every node masked and ``anom_pos = -1``; sample 1 a single valid
      node; sample 2 a valid, flagged node (3) without any edge (degree 0) and node 3 in nobody's
      neighbourhood; sample 3 keeps adjacency entries from valid nodes TOWARDS its masked nodes;
      every masked node holds 123.0;
    * ``zeros``: sample 0 all zero (the clamp of the normalisation, the flat softmax, ``act`` and
      ``act'`` AT zero);
    * ``zero_norm``: in sample 1 the valid node 0 is all zero and has the non-zero valid nodes 1 and
      2 as neighbours, both ways.
    """
    from gnnqc.models.graphconv import AGNNConv
    gen = torch.Generator().manual_seed(9000 + [k.name for k in CASES].index(c.name))
    B, T, N, Cin = c.B, c.T, c.N, c.Cin
    x = torch.randn(B, T, N, Cin, generator=gen)
    if c.xkind == "sign":
        sign = torch.randint(0, 2, (B, T, 1, Cin), generator=gen).float() * 2 - 1
        x = sign * (0.25 + x.abs())
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
    if c.kind == "zero_norm":
        mask[1, :3] = 1
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
    if c.kind == "zero_norm":
        x[1, :, 0] = 0
        adj[1, 0, 1] = adj[1, 0, 2] = adj[1, 1, 0] = adj[1, 2, 0] = 1
    if c.kind == "degenerate":
        x = x + 123.0 * (1 - mask)[:, None, :, None]
    anom_pos = torch.full((B,), -1, dtype=torch.long)
    for b in range(B):
        valid = mask[b].nonzero().flatten()
        if valid.numel():
            anom_pos[b] = valid[int(torch.randint(valid.numel(), (1,), generator=gen))]
    if c.kind == "degenerate":
        anom_pos[2] = 3
    if c.kind == "zero_norm":
        anom_pos[1] = 1                                      # (a neighbour of the zero node is pooled)
    layer = AGNNConv(Cin, c.agg, c.act, trainable=c.trainable)
    with torch.no_grad():
        layer.beta.fill_(c.beta)
        if layer.prelu_alpha is not None:
            layer.prelu_alpha.copy_(0.05 + torch.rand(layer.prelu_alpha.shape, generator=gen) * 0.3)
    layer.train(c.training)
    anom = torch.randn(B, T, Cin, generator=gen) if c.anom else None
    Mp, Cp = time_major_pad(c)
    gshape = (T, Mp, Cp) if c.tm else (B, T, (Cin if c.anom else 0) + Cin)
    return dict(x=x, adj=adj, mask=mask, anom=anom, anom_pos=anom_pos, layer=layer,
                g=torch.randn(gshape, generator=gen))


def layer_params(layer):
    """{quantity name: parameter} of an AGNNConv."""
    ps = {"beta": layer.beta}
    if layer.prelu_alpha is not None:
        ps["alpha"] = layer.prelu_alpha
    return ps


def zero_norm_nodes(d):
    """[B, T, N] bool: nodes whose float32 norm is below the normalisation's clamp."""
    return d["x"].double().norm(dim=-1) < K_EPS


def split_dx(d, grads):
    """``x`` -> ``x`` (nodes of non-zero norm) and ``x0`` (zero-norm nodes), the other group zeroed
    in each: the two are compared against their own scales."""
    z = zero_norm_nodes(d)[..., None].to(grads["x"].dtype)
    out = dict(grads)
    out["x"], out["x0"] = grads["x"] * (1 - z), grads["x"] * z
    return out


def run_eager(c, d, dtype, device="cpu", eager_on_device=False):
    """``agnn_pool_eager`` (or ``agnn_pool`` on a device) in ``dtype``: the output as [B, T, Fo] and
    the gradients of x, anom and every parameter for the case's upstream gradient ``d['g']``, as
    float64 CPU tensors. Returns ``(out, grads, raw output)``."""
    from gnnqc.ops import gcn as G
    layer = copy.deepcopy(d["layer"]).to(device=device, dtype=dtype)
    x = d["x"].to(device=device, dtype=dtype).clone().requires_grad_(True)          # (clone: a fresh leaf)
    anom = d["anom"].to(device=device, dtype=dtype).clone().requires_grad_(True) if d["anom"] is not None else None
    args = (x, d["adj"].to(device=device, dtype=dtype), d["mask"].to(device=device, dtype=dtype), anom,
            d["anom_pos"].to(device), layer, c.pooling)
    Fo = (c.Cin if c.anom else 0) + c.Cin
    if device == "cpu" or eager_on_device:
        raw = out = G.agnn_pool_eager(*args)
        g = d["g"][:, :c.B, :Fo].transpose(0, 1) if c.tm else d["g"]
    else:
        raw = G.agnn_pool(*args, time_major=c.tm)
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
    return out.detach().double().cpu(), split_dx(d, grads), raw.detach()


def dbeta_mass(c, d):
    """A = sum over rows, nodes and edges of |ds_ij <xn_i, xn_j>| in float64 (module docstring):
    the mass of the summands of dbeta."""
    dt = torch.float64
    L = d["layer"]
    x, adj, mask = d["x"].to(dt), d["adj"].to(dt), d["mask"].to(dt)
    beta = L.beta.detach().to(dt)
    al = L.prelu_alpha.detach().to(dt) if L.prelu_alpha is not None else None
    B, T, N, Cin = x.shape
    nb = (adj > 0)[:, None]                                                  # [B, 1, i, j]
    xn = x / x.norm(dim=-1, keepdim=True).clamp(min=K_EPS)
    cos = torch.einsum("btif,btjf->btij", xn, xn)
    s = torch.where(nb, beta * cos, torch.full_like(cos, -float("inf")))
    m = s.amax(-1, keepdim=True)
    e = torch.where(nb, torch.exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m))), torch.zeros_like(s))
    att = e / e.sum(-1, keepdim=True).clamp(min=1e-300)
    r = torch.einsum("btij,btjf->btif", att, x)
    sd = 1 / (adj > 0).sum(-1).to(dt).clamp(min=1) if L.aggregate == "mean" else torch.ones(B, N, dtype=dt)
    o = r * sd[:, None, :, None]
    if L.activation == "prelu":
        da = torch.where(o > 0, torch.ones_like(o), al.expand_as(o))
    elif L.activation == "relu":
        da = (o > 0).to(dt)
    else:
        da = torch.ones_like(o)
    Ca = 0 if d["anom"] is None else Cin
    g = d["g"].to(dt)
    g = g[:, :B, :Ca + Cin].transpose(0, 1) if c.tm else g
    pw = G_pool_weights(mask, d["anom_pos"], c.pooling)
    u = da * (pw * sd)[:, None, :, None] * g[..., Ca:][:, :, None, :]
    ds = att * (torch.einsum("btif,btjf->btij", u, x) - (u * r).sum(-1, keepdim=True))
    return (ds * cos).abs().sum().item()


def G_pool_weights(mask, anom_pos, pooling):
    from gnnqc.ops import gcn as G
    return G.gat_pool_weights(mask, anom_pos, pooling)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, inputs, float64 oracle (out, grads), float32 eager errors {quantity: max |err|}, the
    mass A of dbeta's summands)."""
    c = next(k for k in CASES if k.name == name)
    d = agnn_inputs(c)
    out64, g64, _ = run_eager(c, d, torch.float64)
    out32, g32, _ = run_eager(c, d, torch.float32)
    e32 = {"out": (out32 - out64).abs().max().item()}
    for k in g64:
        e32[k] = (g32[k] - g64[k]).abs().max().item() if g64[k].numel() else 0.0
    mass = dbeta_mass(c, d) if on_hip_path(c) else 0.0
    return c, d, (out64, g64), e32, mass


def out_excess(got, ref, e32):
    """max over elements of |got - ref| / bound, bound = max(K e32, 1e-4 + 1e-4 |ref|); inf if
    ``got`` is not finite. <= 1 passes."""
    if not torch.isfinite(got).all():
        return float("inf")
    bound = torch.clamp(OUT_ATOL + OUT_RTOL * ref.abs(), min=K_FLOOR_MULT * e32)
    return ((got - ref).abs() / bound).max().item() if ref.numel() else 0.0


def out_worst(got, ref, e32):
    """(|got - ref|, bound) at the output element of the largest |got - ref| / bound (the report's row)."""
    if not ref.numel() or not torch.isfinite(got).all():
        return float("nan"), float("nan")
    bound = torch.clamp(OUT_ATOL + OUT_RTOL * ref.abs(), min=K_FLOOR_MULT * e32)
    err = (got - ref).abs()
    i = int((err / bound).argmax())
    return err.reshape(-1)[i].item(), bound.reshape(-1)[i].item()


def _ratio(err, bound):
    return err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))


def grad_bound(k, ref, e32, mass):
    """The bound on gradient ``k``: max(4 e32, floor); the floor is 1e-3 max|ref|, for ``beta``
    1e-3 |ref| + 2^-20 A."""
    if not ref.numel():                                     # (a frozen beta: nothing to compare)
        return 0.0
    if k == "beta":
        return max(K_FLOOR_MULT * e32, GRAD_REL * ref.abs().max().item() + DBETA_MASS * mass)
    return max(K_FLOOR_MULT * e32, GRAD_REL * (ref.abs().max().item() + 1e-6))


_REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _report_file():
    yield
    path = os.environ.get("GNNQC_AGNN_REPORT")
    if path and _REPORT:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("# tests/test_agnn_kernels_gpu.py: measured |err| of agnn_pool on the device against the float64\n"
                    f"# oracle, the float32 eager layer's own error (e32) and the bound (max of {K_FLOOR_MULT:g} x e32 and\n"
                    "# the floor: 1e-4 + 1e-4 |ref| on outputs, 1e-3 max|ref| on gradients, 1e-3 |ref| + 2^-20 A on dbeta;\n"
                    "# the 'out' row gives err and bound at the element of the largest err / bound; dx0: the zero-norm\n"
                    "# nodes' dx). err / bound <= 1 passes.\n"
                    f"# {'case':<28} {'quantity':<8} {'err':>11} {'e32':>11} {'bound':>11} {'err/bound':>11}\n")
            f.write("\n".join(_REPORT) + "\n")


@pytest.mark.parametrize("name", [c.name for c in CASES if "hip" in c.tags])
def test_agnn_case_matches_float64(cuda_device, name):
    """Output, dx (two groups), danom, dbeta, dalpha of one case against float64 eager, within the
    measured bound; time-major cases: padding rows and channels exactly zero; a frozen beta gets no
    gradient."""
    from gnnqc.ops import gcn as G
    c, d, (out64, g64), e32, mass = reference(name)
    dev = cuda_device
    layer_dev = copy.deepcopy(d["layer"]).to(dev)
    assert G.agnn_pool_hip_ok(d["x"].to(dev), layer_dev, c.pooling)
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
    if not c.trainable:
        assert grads["beta"].numel() == 0 and g64["beta"].numel() == 0, "a frozen beta got a gradient"
    for k, ref in g64.items():
        assert grads[k].shape == ref.shape, (k, grads[k].shape, ref.shape)
        got = grads[k]
        err = (got - ref).abs().max().item() if ref.numel() else 0.0
        bound = grad_bound(k, ref, e32[k], mass)
        _REPORT.append(f"{c.name:<30} {'d' + k:<8} {err:11.3e} {e32[k]:11.3e} {bound:11.3e} "
                       f"{_ratio(err, bound):11.3e}")
        print(_REPORT[-1])
        if not (err <= bound) or not torch.isfinite(got).all():
            fails.append(f"d{k}: err {err:.3e} > bound {bound:.3e}")
    assert not fails, f"{c.name}: " + "; ".join(fails)


@pytest.mark.parametrize("name", [c.name for c in CASES if "eager" in c.tags])
def test_agnn_off_the_hip_path_is_the_eager_layer(cuda_device, name):
    """N = 65, aggregate max, pooling max, activation tanh: agnn_pool takes the eager layer on the
    device and agrees with it exactly, output and gradients."""
    from gnnqc.ops import gcn as G
    c, d, _, _, _ = reference(name)
    dev = cuda_device
    assert not G.agnn_pool_hip_ok(d["x"].to(dev), copy.deepcopy(d["layer"]).to(dev), c.pooling)
    a = run_eager(c, d, torch.float32, dev)
    b = run_eager(c, d, torch.float32, dev, eager_on_device=True)
    assert torch.isfinite(a[0]).all() and torch.equal(a[0], b[0])
    assert set(a[1]) == set(b[1])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k


def test_agnn_time_major_needs_the_hip_path(cuda_device):
    """agnn_pool(time_major=True) returns the kernel's own [T, Mp, Cp] tensor on the HIP path and
    raises off it (the eager layer has no time-major form)."""
    from gnnqc.ops import gcn as G
    c, d, _, _, _ = reference("tm_b5")
    dev = cuda_device
    layer = copy.deepcopy(d["layer"]).to(dev)
    args = [d[k].to(dev) for k in ("x", "adj", "mask", "anom", "anom_pos")]
    h, Bret = G.agnn_pool(*args, layer, c.pooling, time_major=True)
    assert Bret == c.B and tuple(h.shape) == (c.T, *time_major_pad(c))
    layer.aggregate = "max"
    with pytest.raises(ValueError):
        G.agnn_pool(*args, layer, c.pooling, time_major=True)


def test_agnn_frozen_beta_launches(cuda_device, monkeypatch):
    """With no parameter needing a gradient agnn_pool_bwd is not launched; with only alpha needing
    one it is, and beta still gets no gradient."""
    from gnnqc.utils import native
    real = native.hip_ops()
    calls = []

    class Rec:
        def __getattr__(self, n):
            f = getattr(real, n)
            return (lambda *a, **k: calls.append(n) or f(*a, **k)) if n.startswith(("agnn_", "edge_")) else f

    monkeypatch.setattr(native, "hip_ops", lambda: Rec())
    for name, want in (("beta_frozen_linear", False), ("beta_frozen", True), ("inst_c2_sum_mean", True)):
        c, d, _, _, _ = reference(name)
        calls.clear()
        run_eager(c, d, torch.float32, cuda_device)
        assert calls[:2] == ["edge_adj_bits", "agnn_pool_fwd"] and "agnn_pool_bwd_input" in calls, calls
        assert ("agnn_pool_bwd" in calls) == want and ("agnn_bwd_finalize" in calls) == want, (name, calls)


def test_agnn_forward_and_backward_are_bitwise_reproducible(cuda_device):
    """Two runs of the multi-pass cases give bitwise-equal outputs and gradients (fixed-order record
    sum, no float atomics)."""
    for name in ("passes", "passes_tm"):
        c, d, _, _, _ = reference(name)
        a = run_eager(c, d, torch.float32, cuda_device)
        b = run_eager(c, d, torch.float32, cuda_device)
        assert torch.equal(a[0], b[0])
        for k in a[1]:
            assert torch.equal(a[1][k], b[1][k]), (name, k)
