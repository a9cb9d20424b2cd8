"""CPU part of the baseline integrated-gradients kernel tests
(``tests/test_ig_baseline_kernels_gpu.py``): the float64 reference is checked against a second route,
every case of the table is checked to still reach the kernel branches it names, and the properties
the GPU comparison relies on (sign flips inside the path, few elements with an ambiguous sign, a
backward bound that a flip index off by one step cannot meet) are asserted from the reference
alone."""
import pytest
import torch

import test_ig_baseline_kernels_gpu as Bk
import test_ig_kernels_gpu as S
from gnnqc.ops import gcn as G

_IDS = [c.name for c in S.IG_CASES]


def _second_route(c, d):
    """The project's eager pooled GeneralConv in eval mode, in float64, on the kk x B replicated
    inputs interpolated from the baseline (what the explainer's generic path runs): ``(out [T, kk B,
    Ca + F], acc_x, acc_a)``; pool weights as a diagonal aggregation matrix, as the zero-baseline
    tests' second route."""
    B, T, N, Cin, F, Ca, kk = c.B, c.T, c.N, c.Cin, c.F, c.Ca, d["kk"]
    a, wts = d["alphas"].double(), d["wts"].double()
    x, xb = d["x"].double(), d["xb"].double()
    xr = (xb + a.view(kk, 1, 1, 1, 1) * (x - xb)).reshape(kk * B, T, N, Cin).requires_grad_(True)
    adj = torch.diag_embed(d["w"].double()).repeat(kk, 1, 1)
    mask = (d["mask"] != 0).double().repeat(kk, 1)
    h = G.general_conv_eager(xr, adj, mask, d["W"].double(), d["bias"].double(), d["scale"].double(),
                             d["shift"].double(), torch.zeros(F, dtype=torch.float64),
                             torch.ones(F, dtype=torch.float64), d["prelu_alpha"].double(), False, "sum", eps=0.0)
    parts = [G.pool_nodes(h, mask, None, "sum")]                                     # [kk B, T, F]
    anr = None
    if Ca:
        an, ab = d["anom"].double(), d["ab"].double()
        anr = (ab + a.view(kk, 1, 1, 1) * (an - ab)).reshape(kk * B, T, Ca).requires_grad_(True)
        parts = [anr, parts[0]]
    out = torch.cat(parts, -1).transpose(0, 1)                                       # [T, kk B, Ca + F]
    (out * d["g"].double()[:, :kk * B, :Ca + F]).sum().backward()
    acc_x = (wts.view(kk, 1, 1, 1, 1) * xr.grad.view(kk, B, T, N, Cin)).sum(0)
    acc_a = (wts.view(kk, 1, 1, 1) * anr.grad.view(kk, B, T, Ca)).sum(0) if Ca else torch.zeros(B, T, 0).double()
    return out.detach(), acc_x, acc_a


def _close(a, b, what):
    scale = b.abs().max().item() if b.numel() else 0.0
    err = (a - b).abs().max().item() if b.numel() else 0.0
    assert err <= 1e-12 * scale + 1e-300, f"{what}: {err:.3e} against max |ref| {scale:.3e}"


@pytest.mark.parametrize("case", S.IG_CASES, ids=_IDS)
def test_base_reference_two_ways_agree(case):
    """The plain float64 reference == eager pooled GeneralConv (eval, float64) on the replicated
    path batch, to 1e-12 relative: output, acc_x and acc_a; masked nodes' acc_x exactly zero."""
    d, r = Bk.case_reference(case)
    out, acc_x, acc_a = _second_route(case, d)
    assert out.shape == r["out"].shape and acc_x.shape == r["acc_x"].shape and acc_a.shape == r["acc_a"].shape
    _close(out, r["out"], "out")
    _close(acc_x, r["acc_x"], "acc_x")
    _close(acc_a, r["acc_a"], "acc_a")
    dead = ~r["live"][:, None, :, None].expand_as(acc_x)
    assert torch.count_nonzero(r["acc_x"][dead]) == 0 and torch.count_nonzero(acc_x[dead]) == 0
    assert r["acc_x"].abs().max() > 0 and torch.isfinite(r["acc_x"]).all() and torch.isfinite(r["out"]).all()


def test_baseline_builder_properties():
    for c in S.IG_CASES:
        d, d0 = Bk.base_inputs(c), S.ig_inputs(c)
        assert all(torch.equal(d[k], d0[k]) for k in d0 if isinstance(d0[k], torch.Tensor)), c.name
        assert d["xb"].shape == d["x"].shape and d["ab"].shape == d["anom"].shape
        assert torch.count_nonzero(d["xb"] * (1 - d["mask"])[:, None, :, None]) == 0
        assert d["xb"].abs().max() > 0 and (c.Ca == 0 or d["ab"].abs().max() > 0)
        assert not torch.equal(d["xb"], d["x"])
        d2 = Bk.base_inputs(c)
        assert torch.equal(d["xb"], d2["xb"]) and torch.equal(d["ab"], d2["ab"])
    assert set(Bk.BASE_SEEDS) == {"n_edges_N1"}
    assert {Bk.by_name(n).name for n in Bk.SPECIAL_CASES} == set(Bk.SPECIAL_CASES)


@pytest.mark.parametrize("case", S.IG_CASES, ids=_IDS)
def test_base_case_reaches_its_branches(case):
    """Every tag's predicate re-asserted: the baseline ops share the dispatch table, the NM
    instances, the store passes, the path slicing and the padding rules of the zero-baseline ops."""
    c = case
    assert c.tags, c.name
    for tag in c.tags:
        assert S.IG_PREDICATES[tag](c), f"{c.name} no longer reaches '{tag}'"
    assert {t for k in S.IG_CASES for t in k.tags} == set(S.IG_PREDICATES)


@pytest.mark.parametrize("name", Bk.SPECIAL_CASES)
def test_zero_base_reference_is_the_zero_baseline_reference(name):
    """xb = ab = 0: the reference is the zero-baseline tests' reference (same output and gradients to
    1e-12 relative), and its bounds are theirs with the baseline kernels' factors."""
    c = Bk.by_name(name)
    d, r = Bk.case_reference(c, kind="zero")
    _, r0 = S.case_reference(c)
    for k in ("out", "acc_x", "acc_a"):
        _close(r[k], r0[k], k)
    assert torch.equal(r["flip"], r0["flip"]) and torch.equal(r["j"], r0["j"])
    assert torch.equal(r["ambiguous"], r0["ambiguous"])
    ks_max = S.bwd_ks_max(c)
    _close(r["fwd_bound"] - 1e-30, (r0["fwd_bound"] - 1e-30) * (c.N + 2 * c.Cin + 6) / (c.N + c.Cin + 4), "fwd_bound")
    _close(r["bwd_bound"] - 1e-30,
           (r0["bwd_bound"] - 1e-30) * (ks_max + c.F + 2 * c.Cin + 10) / (ks_max + c.F + c.Cin + 8), "bwd_bound")
    _close(r["loose"], r0["loose"], "loose")


@pytest.mark.parametrize("name", Bk.SPECIAL_CASES)
def test_base_equals_x_reference_has_no_slope(name):
    c = Bk.by_name(name)
    d, r = Bk.case_reference(c, kind="equals_x")
    assert not r["flip"].any() and (r["j"] == d["kk"]).all()
    B = c.B
    for s in range(d["kk"]):
        assert torch.equal(r["out"][:, s * B:(s + 1) * B], r["out"][:, :B])


@pytest.mark.parametrize("case", S.IG_CASES, ids=_IDS)
def test_base_flips_inside_the_path_and_ambiguity_cap(case):
    """At least 15 % of a case's live (window, step, node, channel) pairs change sign inside the
    path (kk1 has a single point), and at most 10 % of its live elements have an ambiguous sign."""
    c = case
    d, r = Bk.case_reference(c)
    share, amb = S.flip_share(c, r), S.ambiguous_share(c, r)
    print(f"{c.name}: flips {share:.3f} ambiguous {amb:.4f}")
    if c.kk == 1:
        assert share == 0
    else:
        assert share >= S.MIN_FLIP_SHARE, f"{c.name}: {share:.3f} of the live pairs flip"
    assert amb <= S.AMBIGUOUS_CAP, f"{c.name}: {amb:.3f} of the live elements are ambiguous"
    # the looser bound is zero exactly where nothing is ambiguous
    assert torch.count_nonzero(r["loose"][~r["ambiguous"]]) == 0


def test_base_accumulate_path_of_17_has_flips_in_every_chunk():
    c = Bk.by_name("accumulate")
    d, r = Bk.case_reference(c, S.ACCUMULATE_CHUNKS[-1][1])
    assert S.flip_share(c, r) >= S.MIN_FLIP_SHARE and S.ambiguous_share(c, r) <= S.AMBIGUOUS_CAP
    j = r["j"][r["flip"] & r["live"][:, None, :, None]]
    for s0, s1 in S.ACCUMULATE_CHUNKS:
        assert ((j >= s0) & (j < s1)).any(), (s0, s1)


def _closed_form_acc_x(c, d, r, j):
    """acc_x from the kernels' closed form in float64, with the per-node offset: per (window, step,
    node, channel) the PReLU derivative is c0 before the flip index j and c1 from it on, so with the
    prefix sums P(j) = sum_{s<j} wt_s g_f(s) and Q = P(kk): H = c0 P(j) + c1 (Q - P(j)),
    acc_x = w sum_f W_kf sc_f H. (c0, c1 are the signs of y = alpha xs_n + A0_n at the path's ends.)"""
    B, T, F, Ca, kk = c.B, c.T, c.F, c.Ca, d["kk"]
    al, wts = d["prelu_alpha"].double(), d["wts"].double()
    gs = d["g"].double()[:, :kk * B, Ca:Ca + F].reshape(T, kk, B, F).permute(1, 2, 0, 3)      # [kk,B,T,F]
    P = torch.cat([torch.zeros(1, B, T, F).double(), (wts.view(kk, 1, 1, 1) * gs).cumsum(0)])   # [kk+1,B,T,F]
    Pj = torch.gather(P[:, :, :, None, :].expand(-1, -1, -1, c.N, -1), 0, j[None])[0]           # [B,T,N,F]
    Q = P[kk][:, :, None, :]
    c0 = torch.where(r["y"][0] > 0, torch.ones(()).double(), al)
    c1 = torch.where(r["y"][-1] > 0, torch.ones(()).double(), al)
    H = c0 * Pj + c1 * (Q - Pj)
    Wsc = d["W"].double() * d["scale"].double()
    return torch.einsum("btnf,kf->btnk", H, Wsc) * (d["w"].double() * r["live"])[:, None, :, None]


@pytest.mark.parametrize("name", ["kk2", "kk9", "slices_257", "lds_f32_k128"])
def test_base_bound_rejects_a_flip_index_off_by_one(name):
    """The closed form the kernels use equals the reference with the reference's flip indices, and
    leaves the backward bound (the looser one of ambiguous elements included) for nearly every
    affected element when every flip index is one step late."""
    c = Bk.by_name(name)
    d, r = Bk.case_reference(c)
    good = _closed_form_acc_x(c, d, r, r["j"])
    _close(good, r["acc_x"], "closed form")
    late = torch.where(r["flip"], (r["j"] + 1).clamp(max=d["kk"]), r["j"])
    bad = _closed_form_acc_x(c, d, r, late)
    ratio = (bad - r["acc_x"]).abs() / (r["bwd_bound"] + r["loose"])
    hit = (r["flip"] & (d["prelu_alpha"] != 1) & r["live"][:, None, :, None]).any(-1)          # [B,T,N]
    assert hit.sum() >= 10
    caught = (ratio.max(-1).values > 1)[hit].double().mean().item()
    print(f"{name}: {caught:.3f} of {int(hit.sum())} affected elements leave the bound, median ratio "
          f"{ratio.max(-1).values[hit].median().item():.0f}")
    assert caught >= 0.95
