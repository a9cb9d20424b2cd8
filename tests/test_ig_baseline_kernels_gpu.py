"""Path-folded integrated-gradients kernels from a baseline (``csrc/kernels/ig.hip``:
``ig_gcn_pool_fwd_base``, ``ig_gcn_pool_bwd_base``, ``ig_interp_base``) called directly over the case
table of ``tests/test_ig_kernels_gpu.py`` (same shapes, tags and inputs), each case with a baseline
``xb = 0.6 randn mask``, ``ab = 0.6 randn`` from a seed of its own, against a plain float64 reference
on the CPU.

The reference (:func:`base_reference`) evaluates every path point ``xb + alpha_s (x - xb)`` plainly,
``y = (x_s W + bias) scale + shift``, ``prelu(y) = y if y > 0 else a y``, the weighted node sum laid
out step-major (``row = s B + b``), and takes the input gradients of every path point by autograd on
the float64 graph, trapezoid-weighted and summed over the steps.

Nothing is compared with a kernel's own output and no tolerance is tuned: the bounds are
forward-error bounds from the operation counts, evaluated in float64 from the reference's
intermediates (``EPS = 2^-24``). With the magnitude sum of a (step, window, time, node, channel)

    mag = alpha_s sum_k |dx_k W_kf| |sc_f| + sum_k |xb_k W_kf sc_f| + |bias_f sc_f| + |shift_f|

(``dx = x - xb``; two dot products of Cin terms, one subtraction per term, two more operations for
the per-node offset than the zero-baseline kernels):

* forward, per ``(s, b, t, f)``: ``4 (N + 2 Cin + 6) EPS sum_n |w_n| max(1, |a_f|) mag + 1e-30``,
  relative to the magnitude sum, not to the result (the running sums cancel); PReLU is continuous,
  so a sign decided differently in fp32 at ``|y| ~ 0`` stays inside it.
* backward, per ``(b, t, n, k)``: ``(ks_max + F + 2 Cin + 10) EPS |w_bn| sum_f |W_kf sc_f| max(1,
  |a_f|) sum_s |wt_s g_f(s)| + 1e-30`` with ``ks_max`` the longest slice. A flip index off by one
  step changes a flipping element by one whole term of that sum: far outside the bound
  (``tests/test_ig_baseline_reference_cpu.py`` shows it).
* an element ``(b, t, n)`` is *ambiguous* when for any ``f`` and ``s`` the float64 ``|y|`` is
  non-zero and below ``1e-5 mag``. Ambiguous elements are not skipped: on top of the bound above
  they get one path step per ambiguous channel, ``|w_bn| sum_{f ambiguous} |W_kf sc_f| |1 - a_f|
  max_s |wt_s g_f(s)|``, exactly as the zero-baseline tests.
* ``acc_a = sum_s wt_s g_c(s)``: ``(ks_max + slices + 4) EPS sum_s |wt_s g_c(s)| + 1e-30``.
* anomaly channels: ``|out - ref| <= 4 EPS (|ab| + alpha_s |a - ab|)``, and the row of
  ``alpha = 1`` is ``anom`` bit for bit.

The worst measured ratio of error to bound of every case is recorded in
``profiles/ig_baseline_kernel_tests.txt``.
"""
import pytest
import torch

import test_ig_kernels_gpu as S

pytestmark = pytest.mark.gpu

EPS = S.EPS
# extra seed of a case's baseline (as slices_257 carries one for its inputs): n_edges_N1 has 8 live
# elements, so a single ambiguous one is 12.5 % of them
BASE_SEEDS = {"n_edges_N1": 1}
# the shapes the two special baselines run on: a tail of windows and nodes, three input channels,
# the largest instance, several store passes
SPECIAL_CASES = ("dispatch_c2f16", "dispatch_c3f16", "dispatch_c2f32", "kk17")


def base_inputs(c, kk=None, kind="random"):
    """The inputs of ``S.ig_inputs`` plus a baseline: ``random`` (``xb = 0.6 randn mask``, ``ab = 0.6
    randn``, seeded by the case), ``zero`` (``xb = ab = 0``) or ``equals_x`` (``xb = x``, ``ab = anom``)."""
    d = dict(S.ig_inputs(c, kk))
    gen = torch.Generator().manual_seed(9000 + S.IG_CASES.index(c) + BASE_SEEDS.get(c.name, 0))
    if kind == "random":
        d["xb"] = 0.6 * torch.randn(c.B, c.T, c.N, c.Cin, generator=gen) * d["mask"][:, None, :, None]
        d["ab"] = 0.6 * torch.randn(c.B, c.T, c.Ca, generator=gen) if c.Ca else torch.zeros(0)
    elif kind == "zero":
        d["xb"], d["ab"] = torch.zeros_like(d["x"]), torch.zeros_like(d["anom"])
    else:
        assert kind == "equals_x"
        d["xb"], d["ab"] = d["x"].clone(), d["anom"].clone()
    return d


def base_reference(c, d):
    """Plain float64 evaluation of every path point ``xb + alpha_s (x - xb)`` of one case and autograd
    on that graph; the entries of ``S.ig_reference`` with the bounds of this module's docstring, plus
    ``an_bound [T, kk B, Ca]`` of the anomaly channels."""
    B, T, N, Cin, F, Ca, kk = c.B, c.T, c.N, c.Cin, c.F, c.Ca, d["kk"]
    f64 = {k: v.double() for k, v in d.items() if isinstance(v, torch.Tensor)}
    a, wts = f64["alphas"], f64["wts"]
    W, bias, sc, sh, al, w = f64["W"], f64["bias"], f64["scale"], f64["shift"], f64["prelu_alpha"], f64["w"]
    x, xb = f64["x"], f64["xb"]
    xs = (xb + a.view(kk, 1, 1, 1, 1) * (x - xb)).detach().requires_grad_(True)        # [kk,B,T,N,Cin]
    y = (torch.matmul(xs, W) + bias) * sc + sh                                         # [kk,B,T,N,F]
    act = torch.where(y > 0, y, al * y)
    pooled = torch.einsum("bn,sbtnf->sbtf", w, act)
    parts = [pooled]
    an = None
    an_bound = torch.zeros(T, kk * B, 0, dtype=torch.float64)
    if Ca:
        an = (f64["ab"] + a.view(kk, 1, 1, 1) * (f64["anom"] - f64["ab"])).detach().requires_grad_(True)
        parts = [an, pooled]
        an_bound = 4 * EPS * (f64["ab"].abs() + a.view(kk, 1, 1, 1) * (f64["anom"] - f64["ab"]).abs())
        an_bound = an_bound.permute(2, 0, 1, 3).reshape(T, kk * B, Ca)
    out = torch.cat(parts, -1).permute(2, 0, 1, 3).reshape(T, kk * B, Ca + F)          # row = s B + b
    gsel = f64["g"][:, :kk * B, :Ca + F]
    (out * gsel).sum().backward()
    live = d["mask"] != 0
    acc_x = (wts.view(kk, 1, 1, 1, 1) * xs.grad).sum(0) * live[:, None, :, None]
    acc_a = (wts.view(kk, 1, 1, 1) * an.grad).sum(0) if Ca else torch.zeros(B, T, 0, dtype=torch.float64)

    slope = al.abs().clamp(min=1.0)
    mag = (a.view(kk, 1, 1, 1, 1) * torch.matmul((x - xb).abs(), W.abs()) * sc.abs()
           + torch.matmul(xb.abs(), (W * sc).abs()) + (bias * sc).abs() + sh.abs())    # [kk,B,T,N,F]
    fwd_bound = 4 * (N + 2 * Cin + 6) * EPS * torch.einsum("bn,sbtnf->sbtf", w.abs(), slope * mag) + 1e-30
    fwd_bound = fwd_bound.permute(2, 0, 1, 3).reshape(T, kk * B, F)
    yd = y.detach()
    amb_f = ((yd != 0) & (yd.abs() < S.AMBIGUOUS_REL * mag)).any(0)                    # [B,T,N,F]
    wg = (wts.view(kk, 1, 1, 1) * gsel.reshape(T, kk, B, Ca + F).permute(1, 2, 0, 3)).abs()   # [kk,B,T,Ca+F]
    gsum, gmax = wg.sum(0), wg.max(0).values                                           # [B,T,Ca+F]
    Wsc = (W * sc).abs()                                                               # [Cin,F]
    ks_max, slices = min(kk, S.IGG_KMAX), S._cdiv(kk, S.IGG_KMAX)
    bwd_bound = ((ks_max + F + 2 * Cin + 10) * EPS * w.abs()[:, None, :, None]
                 * torch.einsum("kf,btf->btk", Wsc * slope, gsum[..., Ca:])[:, :, None, :]) + 1e-30
    loose = w.abs()[:, None, :, None] * torch.einsum("btnf,kf,btf->btnk", amb_f.double(), Wsc * (1 - al).abs(),
                                                     gmax[..., Ca:])
    a_bound = (ks_max + slices + 4) * EPS * gsum[..., :Ca] + 1e-30
    p0, p1 = yd[0] > 0, yd[-1] > 0
    flip = p0 != p1
    other = (yd > 0) != p0
    j = torch.where(flip, other.int().argmax(0), torch.full_like(p0, kk, dtype=torch.long))
    return dict(out=out.detach(), acc_x=acc_x, acc_a=acc_a, fwd_bound=fwd_bound, bwd_bound=bwd_bound, loose=loose,
                a_bound=a_bound, an_bound=an_bound, y=yd, live=live, ambiguous=amb_f.any(-1), flip=flip, j=j)


_REFERENCES = {}


def case_reference(c, kk=None, kind="random"):
    """(inputs, reference) of a case and baseline kind, computed once per process and shared (never
    modified)."""
    key = (c.name, c.kk if kk is None else kk, kind)
    if key not in _REFERENCES:
        d = base_inputs(c, kk, kind)
        _REFERENCES[key] = (d, base_reference(c, d))
    return _REFERENCES[key]


def by_name(name):
    return next(c for c in S.IG_CASES if c.name == name)


# ------------------------------------------------------------------ device runs
def run_fwd(t, alphas=None):
    from gnnqc.utils.native import hip_ops
    return hip_ops().ig_gcn_pool_fwd_base(t["x"], t["xb"], t["w"], t["anom"], t["ab"], *[t[k] for k in S._PARAMS],
                                          t["alphas"] if alphas is None else alphas, t["Cp"])


def run_bwd(t, acc_x, acc_a, overwrite, g=None, alphas=None, wts=None):
    from gnnqc.utils.native import hip_ops
    hip_ops().ig_gcn_pool_bwd_base(t["x"], t["xb"], t["w"], t["mask"], t["g"] if g is None else g,
                                   *[t[k] for k in S._PARAMS], t["alphas"] if alphas is None else alphas,
                                   t["wts"] if wts is None else wts, acc_x, acc_a, overwrite)


def check_forward(c, d, r, out, kk, what=""):
    """Shape, exact padding rows and channels, anomaly channels within their bound and bitwise
    ``anom`` at alpha = 1, GCN channels within the forward bound. Returns the worst error / bound."""
    Ca, F, B = c.Ca, c.F, c.B
    Mp = S._cdiv(kk * B, 16) * 16
    assert tuple(out.shape) == (c.T, Mp, d["Cp"]), (c.name, tuple(out.shape))
    o = out.cpu()
    assert torch.count_nonzero(o[:, kk * B:]) == 0, f"{c.name}: padding rows"
    assert torch.count_nonzero(o[:, :, Ca + F:]) == 0, f"{c.name}: padding channels"
    ra = 0.0
    if Ca:
        got = o[:, :kk * B, :Ca]
        ra = S._ratio((got.double() - r["out"][..., :Ca]).abs(), r["an_bound"] + 1e-30)
        for s in range(kk):
            if d["alphas"][s] == 1:
                assert torch.equal(got[:, s * B:(s + 1) * B], d["anom"].transpose(0, 1)), f"{c.name}: anom at alpha 1"
    err = (o[:, :kk * B, Ca:Ca + F].double() - r["out"][..., Ca:]).abs()
    ratio = S._ratio(err, r["fwd_bound"])
    print(f"IGBRATIO {c.name}{what} kk={kk} fwd {ratio:.4f} anom {ra:.4f}")
    assert ratio <= 1.0, f"{c.name}{what}: forward error / bound {ratio:.3f}"
    assert ra <= 1.0, f"{c.name}{what}: anomaly channels error / bound {ra:.3f}"
    return ratio


def check_backward(c, r, acc_x, acc_a, pre_x=None, pre_a=None, what=""):
    """As ``S.check_backward`` against this module's reference and bounds."""
    ax, aa = acc_x.double().cpu(), acc_a.double().cpu()
    ref_x, ref_a = r["acc_x"], r["acc_a"]
    bx, ba = r["bwd_bound"] + r["loose"], r["a_bound"]
    if pre_x is not None:
        ref_x, ref_a = ref_x + pre_x.double(), ref_a + pre_a.double()
        bx = bx + EPS * (pre_x.double().abs() + r["acc_x"].abs() + bx)
        ba = ba + EPS * (pre_a.double().abs() + r["acc_a"].abs() + ba)
    assert ax.shape == ref_x.shape and aa.shape == ref_a.shape
    dead = ~r["live"][:, None, :, None].expand_as(ax)
    assert torch.equal(ax[dead], ref_x[dead] if pre_x is not None else torch.zeros_like(ax[dead])), \
        f"{c.name}{what}: masked nodes"
    rx, ra = S._ratio((ax - ref_x).abs(), bx), S._ratio((aa - ref_a).abs(), ba)
    print(f"IGBRATIO {c.name}{what} bwd_x {rx:.4f} bwd_a {ra:.4f}")
    assert rx <= 1.0, f"{c.name}{what}: acc_x error / bound {rx:.3f}"
    assert ra <= 1.0, f"{c.name}{what}: acc_a error / bound {ra:.3f}"
    return rx, ra


def _fwd_bwd(c, d, r, dev, what=""):
    t = S._to(dev, d)
    out = run_fwd(t)
    check_forward(c, d, r, out, d["kk"], what)
    acc_x, acc_a = S._nan_accumulators(c, dev)
    run_bwd(t, acc_x, acc_a, True)
    torch.cuda.synchronize()
    check_backward(c, r, acc_x, acc_a, what=what)
    return out


@pytest.mark.parametrize("case", S.IG_CASES, ids=[c.name for c in S.IG_CASES])
def test_ig_gcn_pool_base_case_matches_float64(cuda_device, case):
    """ig_gcn_pool_fwd_base and ig_gcn_pool_bwd_base of one case against the float64 reference. The
    backward writes NaN-filled accumulators (overwrite: the first launch reads nothing)."""
    d, r = case_reference(case)
    _fwd_bwd(case, d, r, cuda_device)


@pytest.mark.parametrize("name", SPECIAL_CASES)
def test_zero_base_through_the_base_ops(cuda_device, name):
    """xb = ab = 0 through the _base ops: inside the zero-baseline reference's bounds taken with the
    baseline kernels' factors (the reference is ``S.ig_reference``'s, see the CPU file)."""
    c = by_name(name)
    d, r = case_reference(c, kind="zero")
    _fwd_bwd(c, d, r, cuda_device, " zero_base")


@pytest.mark.parametrize("name", SPECIAL_CASES)
def test_base_equals_x(cuda_device, name):
    """xb = x, ab = anom: every slope is 0 and no flip is possible, so every path point's output
    equals the alpha = 1 output within the bound, and acc_x stays within the bound of the reference."""
    c = by_name(name)
    d, r = case_reference(c, kind="equals_x")
    assert not r["flip"].any()
    out = _fwd_bwd(c, d, r, cuda_device, " base_equals_x").cpu()
    B, kk, Ca, F = c.B, c.kk, c.Ca, c.F
    last = out[:, (kk - 1) * B:kk * B]
    for s in range(kk):
        rows = out[:, s * B:(s + 1) * B]
        assert Ca and torch.equal(rows[..., :Ca], d["anom"].transpose(0, 1))
        err = (rows[..., Ca:Ca + F].double() - last[..., Ca:Ca + F].double()).abs()
        bound = r["fwd_bound"][:, s * B:(s + 1) * B] + r["fwd_bound"][:, (kk - 1) * B:kk * B]
        assert (err <= bound).all(), (name, s)


def test_ig_gcn_pool_base_accumulates(cuda_device):
    """overwrite = False adds to pre-filled accumulators; one path of 17 points in the explainer's
    chunks ([0:6], [6:12], [12:17], overwrite on the first only) gives the whole path's result."""
    dev = cuda_device
    c = by_name("accumulate")
    d, r = case_reference(c)
    t = S._to(dev, d)
    gen = torch.Generator().manual_seed(11)
    pre_x, pre_a = torch.randn(c.B, c.T, c.N, c.Cin, generator=gen), torch.randn(c.B, c.T, c.Ca, generator=gen)
    acc_x, acc_a = pre_x.to(dev), pre_a.to(dev)
    run_bwd(t, acc_x, acc_a, False)
    check_backward(c, r, acc_x, acc_a, pre_x, pre_a, what=" prefilled")
    # the same through the op's default (overwrite is False when left out)
    from gnnqc.utils.native import hip_ops
    acc_x2, acc_a2 = pre_x.to(dev), pre_a.to(dev)
    hip_ops().ig_gcn_pool_bwd_base(t["x"], t["xb"], t["w"], t["mask"], t["g"], *[t[k] for k in S._PARAMS],
                                   t["alphas"], t["wts"], acc_x2, acc_a2)
    assert torch.equal(acc_x2, acc_x) and torch.equal(acc_a2, acc_a)

    kk = S.ACCUMULATE_CHUNKS[-1][1]
    d17, r17 = case_reference(c, kk)
    t17 = S._to(dev, d17)
    one_x, one_a = S._nan_accumulators(c, dev)
    check_forward(c, d17, r17, run_fwd(t17), kk, " one launch of 17")
    run_bwd(t17, one_x, one_a, True)
    check_backward(c, r17, one_x, one_a, what=" one launch of 17")
    acc_x, acc_a = S._nan_accumulators(c, dev)
    B, Ca, F = c.B, c.Ca, c.F
    for s0, s1 in S.ACCUMULATE_CHUNKS:
        a, wt = t17["alphas"][s0:s1].contiguous(), t17["wts"][s0:s1].contiguous()
        out = run_fwd(t17, alphas=a)                                # the chunk's own forward
        err = (out[:, :(s1 - s0) * B, Ca:Ca + F].double().cpu() - r17["out"][:, s0 * B:s1 * B, Ca:]).abs()
        assert S._ratio(err, r17["fwd_bound"][:, s0 * B:s1 * B]) <= 1.0, (s0, s1)
        g = torch.zeros(c.T, S._cdiv((s1 - s0) * B, 16) * 16, d17["Cp"], device=dev)
        g[:, :(s1 - s0) * B] = t17["g"][:, s0 * B:s1 * B]
        run_bwd(t17, acc_x, acc_a, s0 == 0, g=g, alphas=a, wts=wt)
    torch.cuda.synchronize()
    check_backward(c, r17, acc_x, acc_a, what=" three chunks")


@pytest.mark.parametrize("Cin,F,N", S.REFUSED_SHAPES)
def test_ig_gcn_pool_base_refuses_unsupported_shapes(cuda_device, Cin, F, N):
    """Shapes outside GQ_IGG_DISPATCH / IGG_NMAX raise from both ops (a host check, before any launch)."""
    from gnnqc.utils.native import hip_ops
    dev = cuda_device
    B, T, kk, Ca = 2, 2, 3, 1
    Cp = Ca + F + (-(Ca + F)) % 4
    z = lambda *s: torch.zeros(*s, device=dev)      # noqa: E731
    alphas, wts = (v.to(dev) for v in S.path_points(kk))
    with pytest.raises(RuntimeError, match="unsupported"):
        hip_ops().ig_gcn_pool_fwd_base(z(B, T, N, Cin), z(B, T, N, Cin), z(B, N), z(B, T, Ca), z(B, T, Ca), z(Cin, F),
                                       z(F), z(F), z(F), z(F), alphas, Cp)
    acc_x, acc_a = z(B, T, N, Cin), z(B, T, Ca)
    with pytest.raises(RuntimeError, match="unsupported"):
        hip_ops().ig_gcn_pool_bwd_base(z(B, T, N, Cin), z(B, T, N, Cin), z(B, N), z(B, N), z(T, 16, Cp), z(Cin, F),
                                       z(F), z(F), z(F), z(F), alphas, wts, acc_x, acc_a, True)
    torch.cuda.synchronize()
    assert torch.count_nonzero(acc_x) == 0 and torch.count_nonzero(acc_a) == 0


def test_ig_gcn_pool_base_refuses_a_baseline_of_another_shape(cuda_device):
    """xb must have the shape of x and ab that of anom: a host check, before any launch."""
    c = by_name("dispatch_c2f16")
    d, _ = case_reference(c)
    t = S._to(cuda_device, d)
    with pytest.raises(RuntimeError, match="shape of x"):
        run_fwd(dict(t, xb=t["xb"][:, :, :-1].contiguous()))
    with pytest.raises(RuntimeError, match="shape of anom"):
        run_fwd(dict(t, ab=t["ab"][:, :-1].contiguous()))
    acc_x, acc_a = torch.zeros_like(t["x"]), torch.zeros_like(t["anom"])
    with pytest.raises(RuntimeError, match="shape of x"):
        run_bwd(dict(t, xb=t["xb"][:-1].contiguous()), acc_x, acc_a, True)
    torch.cuda.synchronize()
    assert torch.count_nonzero(acc_x) == 0


@pytest.mark.parametrize("kk", [1, 7])
@pytest.mark.parametrize("shape", [(5, 37, 3), (5, 36, 4), (3, 1000, 7), (3, 1001, 7)])
def test_ig_interp_base_matches_float64(cuda_device, shape, kk):
    """ig_interp_base against float64 within 2 EPS (|b| + alpha |v - b|) (one subtraction, one fused
    multiply-add), the alpha = 1 row bitwise v, on the float4 path (numel % 4 == 0) and the scalar
    path with its tail (numel % 4 != 0), in one workgroup and in several."""
    from gnnqc.utils.native import hip_ops
    dev = cuda_device
    gen = torch.Generator().manual_seed(23 * kk + shape[1])
    v, b = torch.randn(*shape, generator=gen), 0.6 * torch.randn(*shape, generator=gen)
    assert (v.numel() % 4 == 0) == (shape[1] % 4 == 0)
    a = torch.linspace(0, 1, kk) if kk > 1 else torch.tensor([1.0])
    out = hip_ops().ig_interp_base(v.to(dev), b.to(dev), a.to(dev))
    torch.cuda.synchronize()
    assert tuple(out.shape) == (kk * shape[0],) + shape[1:]
    o = out.cpu().view(kk, *shape)
    a64 = a.double().view(kk, 1, 1, 1)
    ref = b.double() + a64 * (v.double() - b.double())
    bound = 2 * EPS * (b.double().abs() + a64 * (v.double() - b.double()).abs())
    assert ((o.double() - ref).abs() <= bound).all()
    assert a[-1] == 1 and torch.equal(o[-1], v)
    if kk > 1:
        assert a[0] == 0 and torch.equal(o[0], b)


@pytest.mark.parametrize("shape", [(3, 181, 2), (5, 37, 3), (5, 36, 4)])
def test_ig_interp_base_takes_draws_cut_from_a_stack(cuda_device, shape):
    """Every draw of a stack [n_draws, *shape] as the baseline: with numel % 4 != 0 the odd draws
    start 4 or 8 bytes off a 16-byte boundary, which the scalar path reads as well as any; with
    numel % 4 == 0 every draw is aligned and the float4 path runs. Same bound as above."""
    from gnnqc.utils.native import hip_ops
    dev = cuda_device
    gen = torch.Generator().manual_seed(5 + shape[1])
    kk, draws = 5, 3
    v, stack = torch.randn(*shape, generator=gen), 0.6 * torch.randn(draws, *shape, generator=gen)
    a = torch.linspace(0, 1, kk)
    vd, sd, ad = v.to(dev), stack.to(dev), a.to(dev)
    offsets = [sd[i].data_ptr() % 16 for i in range(draws)]
    assert (v.numel() % 4 == 0) == all(o == 0 for o in offsets), offsets
    a64 = a.double().view(kk, 1, 1, 1)
    for i in range(draws):
        b = sd[i]
        assert b.is_contiguous()
        o = hip_ops().ig_interp_base(vd, b, ad).cpu().view(kk, *shape)
        b64 = stack[i].double()
        ref = b64 + a64 * (v.double() - b64)
        bound = 2 * EPS * (b64.abs() + a64 * (v.double() - b64).abs())
        assert ((o.double() - ref).abs() <= bound).all(), i
        assert torch.equal(o[-1], v) and torch.equal(o[0], stack[i])
    torch.cuda.synchronize()
