"""Path-folded integrated-gradients kernels (``csrc/kernels/ig.hip``: ``ig_gcn_pool_fwd`` and
``ig_gcn_pool_bwd``) called directly, over their template instances, path slicing, tails and
padding, against a plain float64 reference of the same operation on the CPU.

The reference (:func:`ig_reference`) evaluates every path point, ``y = ((alpha_s x) W + bias) scale
+ shift``, ``prelu(y) = y if y > 0 else a y`` (the ``a`` side at exactly 0, as the kernels), the
weighted node sum laid out step-major (``row = s B + b``), and takes the input gradients of every
path point by autograd on the float64 graph, trapezoid-weighted and summed over the steps.

Nothing is compared with a kernel's own output and no tolerance is tuned: the bounds are
forward-error bounds from the operation counts, evaluated in float64 from the reference's
intermediates (``EPS = 2^-24``):

* forward, per ``(s, b, t, f)``: ``4 (N + Cin + 4) EPS sum_n |w_n| max(1, |a_f|) (alpha_s sum_k
  |x_k W_kf| |sc_f| + |bias_f sc_f| + |shift_f|) + 1e-30``. It is relative to the magnitude sum,
  not to the result (the running sums cancel); PReLU is continuous, so a sign decided differently
  in fp32 at ``|y| ~ 0`` stays inside it.
* backward, per ``(b, t, n, k)``: ``(ks_max + F + Cin + 8) EPS |w_bn| sum_f |W_kf sc_f| max(1,
  |a_f|) sum_s |wt_s g_f(s)| + 1e-30`` with ``ks_max`` the longest slice. A flip index off by one
  step changes a flipping element by one whole term of that sum (about ``1 / kk`` of it): far
  outside a bound of a few hundred ``EPS``.
* ``prelu'`` jumps at 0. An element ``(b, t, n)`` is *ambiguous* when for any ``f`` and ``s`` the
  float64 ``|y|`` is non-zero and below ``1e-5 (alpha_s sum_k |x_k W_kf sc_f| + |bias_f sc_f| +
  |shift_f|)``. Ambiguous elements are not skipped: on top of the bound above they get one path
  step per ambiguous channel, ``|w_bn| sum_{f ambiguous} |W_kf sc_f| |1 - a_f| max_s |wt_s
  g_f(s)|``. At most 10 % of a case's live elements may be ambiguous
  (``tests/test_ig_reference_cpu.py`` asserts it from the reference alone).
* ``acc_a = sum_s wt_s g_c(s)`` is a sequential fp32 sum per slice, slices added in turn:
  ``(ks_max + slices + 4) EPS sum_s |wt_s g_c(s)| + 1e-30``.

Every case names the kernel branches it is there to reach (``tags``); their predicates are
recomputed from the shapes in ``tests/test_ig_reference_cpu.py`` (no GPU needed), which also checks
the reference a second way, the share of sign flips per case and the ambiguity cap. The worst
measured ratio of error to bound of every case is recorded in ``profiles/ig_kernel_tests.txt``.
"""
from collections import namedtuple

import pytest
import torch

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------ constants of the kernels
IGG_NMAX = 32               # ig.hip: nodes per window (lanes of the backward's node axis)
IGG_FSG = 8                 # ig.hip: path points per coalesced store pass of the forward
IGG_KMAX = 128              # ig.hip: path points per backward launch (the host slices longer paths)
IGG_BWB = 4                 # ig.hip: windows per backward workgroup
IGG_THREADS = 256           # ig.hip forward: BB = 256 / F windows per workgroup
IGG_PAIRS = ((2, 16), (1, 16), (3, 16), (2, 32), (2, 8))     # GQ_IGG_DISPATCH
IGG_NM = (8, 16, 24, 32)    # forward node-slot instances
LDS_DEFAULT = 64 * 1024     # dynamic LDS a launch may ask for without raising the function's limit
EPS = 2.0 ** -24
AMBIGUOUS_REL = 1e-5
AMBIGUOUS_CAP = 0.10
MIN_FLIP_SHARE = 0.15


def _cdiv(a, b):
    return -(-a // b)


def fwd_bb(c):
    return IGG_THREADS // c.F


def fwd_nm(c):
    return next(nm for nm in IGG_NM if c.N <= nm)


def fwd_passes(c):
    return _cdiv(c.kk, IGG_FSG)


def bwd_slices(c):
    return _cdiv(c.kk, IGG_KMAX)


def bwd_ks_max(c):
    return min(c.kk, IGG_KMAX)


def bwd_lds_bytes(c):
    return IGG_BWB * (bwd_ks_max(c) + 1) * (c.F + 4) * 4


def min_cp(c):
    return c.Ca + c.F + (-(c.Ca + c.F)) % 4


def case_cp(c):
    return min_cp(c) + c.cp_extra


def case_mp(c):
    """Rows of the forward's output: kk B rounded up to 16."""
    return _cdiv(c.kk * c.B, 16) * 16


IGCase = namedtuple("IGCase", "name B T N Cin F Ca kk cp_extra mp_extra zero_a0 seed tags")


def _ic(name, B, T, N, Cin, F, Ca, kk, tags, cp_extra=0, mp_extra=0, zero_a0=False, seed=0):
    return IGCase(name, B, T, N, Cin, F, Ca, kk, cp_extra, mp_extra, zero_a0, seed, tuple(tags))


def _ig_cases():
    cs = [
        # every (Cin, F) pair of GQ_IGG_DISPATCH, every NM instance of the forward
        _ic("dispatch_c2f16", 5, 3, 7, 2, 16, 1, 9, ("c2f16", "nm8", "fwd_tail", "bwd_tail", "store_tail")),
        _ic("dispatch_c1f16", 6, 2, 9, 1, 16, 1, 25, ("c1f16", "nm16", "fwd_tail", "bwd_tail")),
        _ic("dispatch_c3f16", 3, 2, 24, 3, 16, 2, 25, ("c3f16", "nm24", "n_at_nm")),
        _ic("dispatch_c2f8", 33, 2, 17, 2, 8, 0, 9, ("c2f8", "nm24", "fwd_two_wg", "fwd_tail", "bwd_tail", "ca0")),
        _ic("dispatch_c2f32", 9, 2, 32, 2, 32, 4, 17, ("c2f32", "nm32", "fwd_two_wg", "fwd_tail", "ca4", "n_max",
                                                       "n_at_nm")),
    ]
    # N at and just past each NM boundary (B a multiple of the backward's 4 windows)
    for N, nm, edge in ((8, "nm8", "n_at_nm"), (16, "nm16", "n_at_nm"), (25, "nm32", "n_past_nm")):
        cs.append(_ic(f"n_edges_N{N}", 4, 2, N, 2, 16, 1, 9, (nm, edge, "bwd_full")))
    cs += [
        _ic("n_edges_N1", 4, 2, 1, 2, 16, 1, 9, ("nm8", "single_node")),
        # the binary search's smallest cases
        _ic("kk1", 6, 2, 9, 2, 16, 1, 1, ("kk1", "store_tail", "n_past_nm")),
        _ic("kk2", 6, 2, 9, 2, 16, 1, 2, ("kk2", "store_tail")),
    ]
    # forward store passes of IGG_FSG path points, full and tailed
    for kk, tags in ((8, ("store_full", "store_one_pass")), (9, ("store_tail", "store_multi")),
                     (16, ("store_full", "store_multi")), (17, ("store_tail", "store_multi"))):
        cs.append(_ic(f"kk{kk}", 5, 2, 9, 2, 16, 1, kk, tags))
    cs += [
        # the backward's slicing of the path into launches of IGG_KMAX points (slices_257's seed: one
        # whose float64 reference has flip indices in the one-point last slice and nothing ambiguous)
        _ic("slices_129", 3, 2, 9, 2, 16, 1, 129, ("slices2", "last_slice_one_point")),
        _ic("slices_257", 3, 2, 9, 2, 16, 2, 257, ("slices3", "last_slice_one_point"), seed=34),
        _ic("slices_200_b1", 1, 2, 9, 2, 16, 1, 200, ("slices2", "single_window")),
        # IGG_BWB (ks + 1) (F + 4) 4 bytes of dynamic LDS: 74,304 for F = 32, ks = 128
        _ic("lds_f32_k128", 5, 2, 32, 2, 32, 4, 128, ("lds_over_64k", "slices1", "kmax_exact", "c2f32", "nm32")),
        # bias = shift = 0: y = 0 exactly at alpha = 0, the flip at index 1 for every positive x W
        _ic("a0_zero", 3, 2, 12, 2, 16, 2, 25, ("a0_zero",), zero_a0=True),
        # Cp above the minimum; g with more padding rows than the forward makes
        _ic("pad_wide", 5, 2, 9, 2, 16, 2, 9, ("cp_wide", "mp_wide"), cp_extra=4, mp_extra=32),
        # overwrite = False, NaN-filled accumulators with overwrite = True, a path in three chunks
        _ic("accumulate", 5, 2, 9, 2, 16, 1, 9, ("accumulate",)),
    ]
    return cs


IG_CASES = _ig_cases()
ACCUMULATE_CHUNKS = ((0, 6), (6, 12), (12, 17))       # one path of 17 points as the explainer chunks it
REFUSED_SHAPES = ((2, 64, 9), (4, 16, 9), (2, 16, IGG_NMAX + 1))       # (Cin, F, N)

# the branch each tag stands for, as a predicate of the case's shape
IG_PREDICATES = {
    "nm8": lambda c: fwd_nm(c) == 8,
    "nm16": lambda c: fwd_nm(c) == 16,
    "nm24": lambda c: fwd_nm(c) == 24,
    "nm32": lambda c: fwd_nm(c) == 32,
    "n_at_nm": lambda c: c.N == fwd_nm(c),
    "n_past_nm": lambda c: c.N - 1 in IGG_NM,
    "n_max": lambda c: c.N == IGG_NMAX,
    "single_node": lambda c: c.N == 1,
    "fwd_tail": lambda c: c.B % fwd_bb(c) != 0,
    "fwd_two_wg": lambda c: c.B > fwd_bb(c),
    "bwd_tail": lambda c: c.B % IGG_BWB != 0,
    "bwd_full": lambda c: c.B % IGG_BWB == 0,
    "single_window": lambda c: c.B == 1,
    "ca0": lambda c: c.Ca == 0,
    "ca4": lambda c: c.Ca == 4,
    "kk1": lambda c: c.kk == 1,
    "kk2": lambda c: c.kk == 2,
    "store_full": lambda c: c.kk % IGG_FSG == 0,
    "store_tail": lambda c: c.kk % IGG_FSG != 0,
    "store_one_pass": lambda c: fwd_passes(c) == 1,
    "store_multi": lambda c: fwd_passes(c) > 1,
    "slices1": lambda c: bwd_slices(c) == 1,
    "slices2": lambda c: bwd_slices(c) == 2,
    "slices3": lambda c: bwd_slices(c) == 3,
    "last_slice_one_point": lambda c: bwd_slices(c) > 1 and c.kk % IGG_KMAX == 1,
    "kmax_exact": lambda c: c.kk == IGG_KMAX,
    "lds_over_64k": lambda c: bwd_lds_bytes(c) > LDS_DEFAULT,
    "a0_zero": lambda c: c.zero_a0,
    "cp_wide": lambda c: case_cp(c) > min_cp(c),
    "mp_wide": lambda c: c.mp_extra > 0,
    "accumulate": lambda c: c.kk < ACCUMULATE_CHUNKS[-1][1] and bwd_slices(c) == 1,
}
IG_PREDICATES.update({f"c{ci}f{f}": (lambda c, ci=ci, f=f: (c.Cin, c.F) == (ci, f)) for ci, f in IGG_PAIRS})


# ------------------------------------------------------------------ input builder (CPU, float32)
PINNED_PRELU = (0.0, 1.0, -0.3, 1.7)


def path_points(kk):
    """(alphas, trapezoid weights) of a zero-baseline path of kk points, float32."""
    from gnnqc.xai.ig import trapezoid_weights
    alphas = torch.linspace(0.0, 1.0, kk, dtype=torch.float32)
    wts = trapezoid_weights(kk - 1) if kk > 1 else torch.ones(1, dtype=torch.float32)
    return alphas, wts


def ig_inputs(c, kk=None):
    """Inputs of one case on the CPU (seeded by the case): masked nodes' rows of ``x`` zeroed, about
    a quarter of the nodes masked but node 0 always valid, window 1 with node 0 as its only valid
    node, pool weights zero on masked nodes, about a quarter of the BN scales negative, the PReLU
    slopes 0, 1, -0.3 and 1.7 pinned on the first four channels."""
    kk = c.kk if kk is None else kk
    gen = torch.Generator().manual_seed(7000 + 97 * IG_CASES.index(c) + c.seed)
    B, T, N, Cin, F, Ca = c.B, c.T, c.N, c.Cin, c.F, c.Ca
    mask = (torch.rand(B, N, generator=gen) > 0.25).float()
    mask[:, 0] = 1
    if B > 1:
        mask[1] = 0
        mask[1, 0] = 1
    x = torch.randn(B, T, N, Cin, generator=gen) * mask[:, None, :, None]
    w = (0.05 + 0.95 * torch.rand(B, N, generator=gen)) * mask
    anom = torch.randn(B, T, Ca, generator=gen) if Ca else torch.zeros(0)
    W = 0.7 * torch.randn(Cin, F, generator=gen)
    bias = 0.3 * torch.randn(F, generator=gen)
    scale = (0.5 + torch.rand(F, generator=gen)) * torch.where(torch.rand(F, generator=gen) < 0.25, -1.0, 1.0)
    shift = 0.3 * torch.randn(F, generator=gen)
    if c.zero_a0:
        bias, shift = torch.zeros(F), torch.zeros(F)
    prelu_alpha = 0.4 * torch.randn(F, generator=gen)
    prelu_alpha[:len(PINNED_PRELU)] = torch.tensor(PINNED_PRELU)
    alphas, wts = path_points(kk)
    Cp = case_cp(c)
    g = torch.randn(T, _cdiv(kk * B, 16) * 16 + c.mp_extra, Cp, generator=gen)
    return dict(x=x, mask=mask, w=w, anom=anom, W=W, bias=bias, scale=scale, shift=shift, prelu_alpha=prelu_alpha,
                alphas=alphas, wts=wts, g=g, Cp=Cp, kk=kk)


# ------------------------------------------------------------------ float64 reference (CPU)
def ig_reference(c, d):
    """Plain float64 evaluation of every path point of one case and autograd on that graph.

    Returns ``out [T, kk B, Ca + F]`` (step-major rows), ``acc_x [B,T,N,Cin]``, ``acc_a [B,T,Ca]``,
    the bounds of the module docstring (``fwd_bound`` for the GCN channels ``[T, kk B, F]``,
    ``bwd_bound`` and ``loose`` ``[B,T,N,Cin]``, ``a_bound [B,T,Ca]``) and what the CPU tests look at:
    ``y [kk,B,T,N,F]``, ``live [B,N]``, ``ambiguous [B,T,N]``, ``flip [B,T,N,F]`` and the flip index
    ``j [B,T,N,F]`` (first path point on the other side; kk where the sign never changes)."""
    B, T, N, Cin, F, Ca, kk = c.B, c.T, c.N, c.Cin, c.F, c.Ca, d["kk"]
    f64 = {k: v.double() for k, v in d.items() if isinstance(v, torch.Tensor)}
    a, wts = f64["alphas"], f64["wts"]
    W, bias, sc, sh, al, w = f64["W"], f64["bias"], f64["scale"], f64["shift"], f64["prelu_alpha"], f64["w"]
    xs = (a.view(kk, 1, 1, 1, 1) * f64["x"]).detach().requires_grad_(True)             # [kk,B,T,N,Cin]
    y = (torch.matmul(xs, W) + bias) * sc + sh                                         # [kk,B,T,N,F]
    act = torch.where(y > 0, y, al * y)
    pooled = torch.einsum("bn,sbtnf->sbtf", w, act)
    parts = [pooled]
    an = None
    if Ca:
        an = (a.view(kk, 1, 1, 1) * f64["anom"]).detach().requires_grad_(True)         # [kk,B,T,Ca]
        parts = [an, pooled]
    out = torch.cat(parts, -1).permute(2, 0, 1, 3).reshape(T, kk * B, Ca + F)          # row = s B + b
    gsel = f64["g"][:, :kk * B, :Ca + F]
    (out * gsel).sum().backward()
    live = d["mask"] != 0
    acc_x = (wts.view(kk, 1, 1, 1, 1) * xs.grad).sum(0) * live[:, None, :, None]
    acc_a = (wts.view(kk, 1, 1, 1) * an.grad).sum(0) if Ca else torch.zeros(B, T, 0, dtype=torch.float64)

    slope = al.abs().clamp(min=1.0)
    mag = (a.view(kk, 1, 1, 1, 1) * torch.matmul(f64["x"].abs(), W.abs()) * sc.abs()
           + (bias * sc).abs() + sh.abs())                                             # [kk,B,T,N,F]
    fwd_bound = 4 * (N + Cin + 4) * EPS * torch.einsum("bn,sbtnf->sbtf", w.abs(), slope * mag) + 1e-30
    fwd_bound = fwd_bound.permute(2, 0, 1, 3).reshape(T, kk * B, F)
    yd = y.detach()
    amb_f = ((yd != 0) & (yd.abs() < AMBIGUOUS_REL * mag)).any(0)                      # [B,T,N,F]
    wg = (wts.view(kk, 1, 1, 1) * gsel.reshape(T, kk, B, Ca + F).permute(1, 2, 0, 3)).abs()   # [kk,B,T,Ca+F]
    gsum, gmax = wg.sum(0), wg.max(0).values                                           # [B,T,Ca+F]
    Wsc = (W * sc).abs()                                                               # [Cin,F]
    ks_max, slices = min(kk, IGG_KMAX), _cdiv(kk, IGG_KMAX)
    bwd_bound = ((ks_max + F + Cin + 8) * EPS * w.abs()[:, None, :, None]
                 * torch.einsum("kf,btf->btk", Wsc * slope, gsum[..., Ca:])[:, :, None, :]) + 1e-30
    loose = w.abs()[:, None, :, None] * torch.einsum("btnf,kf,btf->btnk", amb_f.double(), Wsc * (1 - al).abs(),
                                                     gmax[..., Ca:])
    a_bound = (ks_max + slices + 4) * EPS * gsum[..., :Ca] + 1e-30
    p0, p1 = yd[0] > 0, yd[-1] > 0
    flip = p0 != p1
    other = (yd > 0) != p0
    j = torch.where(flip, other.int().argmax(0), torch.full_like(p0, kk, dtype=torch.long))
    return dict(out=out.detach(), acc_x=acc_x, acc_a=acc_a, fwd_bound=fwd_bound, bwd_bound=bwd_bound, loose=loose,
                a_bound=a_bound, y=yd, live=live, ambiguous=amb_f.any(-1), flip=flip, j=j)


_REFERENCES = {}


def case_reference(c, kk=None):
    """(inputs, reference) of a case, computed once per process and shared (never modified)."""
    key = (c.name, c.kk if kk is None else kk)
    if key not in _REFERENCES:
        d = ig_inputs(c, kk)
        _REFERENCES[key] = (d, ig_reference(c, d))
    return _REFERENCES[key]


def flip_share(c, r):
    """Share of live (window, step, node, channel) pairs whose sign differs between the path's ends."""
    lv = r["live"][:, None, :, None].expand_as(r["flip"])
    return (r["flip"] & lv).sum().item() / max(1, lv.sum().item())


def ambiguous_share(c, r):
    lv = r["live"][:, None, :].expand_as(r["ambiguous"])
    return (r["ambiguous"] & lv).sum().item() / max(1, lv.sum().item())


# ------------------------------------------------------------------ device runs
_PARAMS = ("W", "bias", "scale", "shift", "prelu_alpha")


def _to(dev, d):
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


def run_fwd(t, alphas=None):
    from gnnqc.utils.native import hip_ops
    return hip_ops().ig_gcn_pool_fwd(t["x"], t["w"], t["anom"], *[t[k] for k in _PARAMS],
                                     t["alphas"] if alphas is None else alphas, t["Cp"])


def run_bwd(t, acc_x, acc_a, overwrite, g=None, alphas=None, wts=None):
    from gnnqc.utils.native import hip_ops
    hip_ops().ig_gcn_pool_bwd(t["x"], t["w"], t["mask"], t["g"] if g is None else g, *[t[k] for k in _PARAMS],
                              t["alphas"] if alphas is None else alphas, t["wts"] if wts is None else wts,
                              acc_x, acc_a, overwrite)


def _ratio(err, bound):
    return (err / bound).max().item() if err.numel() else 0.0


def check_forward(c, d, r, out, kk):
    """Shape, exact padding rows and channels, exact anomaly channels, GCN channels within the
    forward bound. Returns the worst error / bound."""
    Ca, F, B = c.Ca, c.F, c.B
    Mp = _cdiv(kk * B, 16) * 16
    assert tuple(out.shape) == (c.T, Mp, d["Cp"]), (c.name, tuple(out.shape))
    o = out.cpu()
    assert torch.count_nonzero(o[:, kk * B:]) == 0, f"{c.name}: padding rows"
    assert torch.count_nonzero(o[:, :, Ca + F:]) == 0, f"{c.name}: padding channels"
    if Ca:
        an = (d["alphas"].view(kk, 1, 1, 1) * d["anom"]).permute(2, 0, 1, 3).reshape(c.T, kk * B, Ca)   # fp32
        assert torch.equal(o[:, :kk * B, :Ca], an), f"{c.name}: anomaly channels"
    err = (o[:, :kk * B, Ca:Ca + F].double() - r["out"][..., Ca:]).abs()
    ratio = _ratio(err, r["fwd_bound"])
    print(f"IGRATIO {c.name} kk={kk} fwd {ratio:.4f}")
    assert ratio <= 1.0, f"{c.name}: forward error / bound {ratio:.3f}"
    return ratio


def check_backward(c, r, acc_x, acc_a, pre_x=None, pre_a=None, what=""):
    """acc_x, acc_a within the backward bounds of the reference (plus the pre-filled values where
    the launch accumulates: one more fp32 addition, EPS (|pre| + |ref| + bound)); masked nodes'
    acc_x exactly as before the launch (zero when it writes)."""
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
    rx, ra = _ratio((ax - ref_x).abs(), bx), _ratio((aa - ref_a).abs(), ba)
    print(f"IGRATIO {c.name}{what} bwd_x {rx:.4f} bwd_a {ra:.4f}")
    assert rx <= 1.0, f"{c.name}{what}: acc_x error / bound {rx:.3f}"
    assert ra <= 1.0, f"{c.name}{what}: acc_a error / bound {ra:.3f}"
    return rx, ra


def _nan_accumulators(c, dev):
    return (torch.full((c.B, c.T, c.N, c.Cin), float("nan"), device=dev),
            torch.full((c.B, c.T, c.Ca), float("nan"), device=dev))       # (Ca = 0: an empty acc_a)


@pytest.mark.parametrize("case", IG_CASES, ids=[c.name for c in IG_CASES])
def test_ig_gcn_pool_case_matches_float64(cuda_device, case):
    """ig_gcn_pool_fwd and ig_gcn_pool_bwd of one case against the float64 reference. The backward
    writes NaN-filled accumulators (overwrite: the first launch reads nothing)."""
    c = case
    d, r = case_reference(c)
    t = _to(cuda_device, d)
    out = run_fwd(t)
    check_forward(c, d, r, out, c.kk)
    acc_x, acc_a = _nan_accumulators(c, cuda_device)
    run_bwd(t, acc_x, acc_a, True)
    torch.cuda.synchronize()
    check_backward(c, r, acc_x, acc_a)


def test_ig_gcn_pool_accumulates(cuda_device):
    """overwrite = False adds to pre-filled accumulators; one path of 17 points in the explainer's
    chunks ([0:6], [6:12], [12:17], overwrite on the first only) gives the whole path's result."""
    dev = cuda_device
    c = next(c for c in IG_CASES if c.name == "accumulate")
    d, r = case_reference(c)
    t = _to(dev, d)
    gen = torch.Generator().manual_seed(11)
    pre_x, pre_a = torch.randn(c.B, c.T, c.N, c.Cin, generator=gen), torch.randn(c.B, c.T, c.Ca, generator=gen)
    acc_x, acc_a = pre_x.to(dev), pre_a.to(dev)
    run_bwd(t, acc_x, acc_a, False)
    check_backward(c, r, acc_x, acc_a, pre_x, pre_a, what=" prefilled")
    # the same through the op's default (overwrite is False when left out)
    from gnnqc.utils.native import hip_ops
    acc_x2, acc_a2 = pre_x.to(dev), pre_a.to(dev)
    hip_ops().ig_gcn_pool_bwd(t["x"], t["w"], t["mask"], t["g"], *[t[k] for k in _PARAMS], t["alphas"], t["wts"],
                              acc_x2, acc_a2)
    assert torch.equal(acc_x2, acc_x) and torch.equal(acc_a2, acc_a)

    kk = ACCUMULATE_CHUNKS[-1][1]
    d17, r17 = case_reference(c, kk)
    t17 = _to(dev, d17)
    one_x, one_a = _nan_accumulators(c, dev)
    check_forward(c, d17, r17, run_fwd(t17), kk)
    run_bwd(t17, one_x, one_a, True)
    check_backward(c, r17, one_x, one_a, what=" one launch of 17")
    acc_x, acc_a = _nan_accumulators(c, dev)
    B, Ca, F = c.B, c.Ca, c.F
    for s0, s1 in ACCUMULATE_CHUNKS:
        a, wt = t17["alphas"][s0:s1].contiguous(), t17["wts"][s0:s1].contiguous()
        out = run_fwd(t17, alphas=a)                                # the chunk's own forward
        err = (out[:, :(s1 - s0) * B, Ca:Ca + F].double().cpu() - r17["out"][:, s0 * B:s1 * B, Ca:]).abs()
        assert _ratio(err, r17["fwd_bound"][:, s0 * B:s1 * B]) <= 1.0, (s0, s1)
        g = torch.zeros(c.T, _cdiv((s1 - s0) * B, 16) * 16, d17["Cp"], device=dev)
        g[:, :(s1 - s0) * B] = t17["g"][:, s0 * B:s1 * B]
        run_bwd(t17, acc_x, acc_a, s0 == 0, g=g, alphas=a, wts=wt)
    torch.cuda.synchronize()
    check_backward(c, r17, acc_x, acc_a, what=" three chunks")


@pytest.mark.parametrize("Cin,F,N", REFUSED_SHAPES)
def test_ig_gcn_pool_refuses_unsupported_shapes(cuda_device, Cin, F, N):
    """Shapes outside GQ_IGG_DISPATCH / IGG_NMAX raise from both ops (a host check, before any launch)."""
    from gnnqc.utils.native import hip_ops
    dev = cuda_device
    B, T, kk, Ca = 2, 2, 3, 1
    Cp = Ca + F + (-(Ca + F)) % 4
    z = lambda *s: torch.zeros(*s, device=dev)      # noqa: E731
    alphas, wts = (v.to(dev) for v in path_points(kk))
    with pytest.raises(RuntimeError, match="unsupported"):
        hip_ops().ig_gcn_pool_fwd(z(B, T, N, Cin), z(B, N), z(B, T, Ca), z(Cin, F), z(F), z(F), z(F), z(F), alphas, Cp)
    acc_x, acc_a = z(B, T, N, Cin), z(B, T, Ca)
    with pytest.raises(RuntimeError, match="unsupported"):
        hip_ops().ig_gcn_pool_bwd(z(B, T, N, Cin), z(B, N), z(B, N), z(T, 16, Cp), z(Cin, F), z(F), z(F), z(F), z(F),
                                  alphas, wts, acc_x, acc_a, True)
    torch.cuda.synchronize()
    assert torch.count_nonzero(acc_x) == 0 and torch.count_nonzero(acc_a) == 0
