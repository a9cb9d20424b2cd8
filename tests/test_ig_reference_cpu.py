"""CPU part of the integrated-gradients kernel tests (``tests/test_ig_kernels_gpu.py``): the float64
reference is checked against a second route, every case of the GPU table is checked to still reach
the kernel branches it names, and the properties the GPU comparison relies on (sign flips inside
the path, few elements with an ambiguous sign, a backward bound that a flip index off by one step
cannot meet) are asserted from the reference alone."""
import pytest
import torch

import test_ig_kernels_gpu as S
from gnnqc.ops import gcn as G

_IDS = [c.name for c in S.IG_CASES]


def _second_route(c, d):
    """The project's eager pooled GeneralConv in eval mode, in float64, on the kk x B replicated and
    interpolated inputs (what the explainer's generic path runs): ``(out [T, kk B, Ca + F], acc_x,
    acc_a)``. The pool weights enter as a diagonal aggregation matrix with sum aggregation and sum
    pooling; BatchNorm with mean 0, variance 1 and eps 0 applies exactly ``scale`` and ``shift``."""
    B, T, N, Cin, F, Ca, kk = c.B, c.T, c.N, c.Cin, c.F, c.Ca, d["kk"]
    a, wts = d["alphas"].double(), d["wts"].double()
    xr = (a.view(kk, 1, 1, 1, 1) * d["x"].double()).reshape(kk * B, T, N, Cin).requires_grad_(True)
    adj = torch.diag_embed(d["w"].double()).repeat(kk, 1, 1)
    mask = (d["mask"] != 0).double().repeat(kk, 1)
    h = G.general_conv_eager(xr, adj, mask, d["W"].double(), d["bias"].double(), d["scale"].double(),
                             d["shift"].double(), torch.zeros(F, dtype=torch.float64),
                             torch.ones(F, dtype=torch.float64), d["prelu_alpha"].double(), False, "sum", eps=0.0)
    parts = [G.pool_nodes(h, mask, None, "sum")]                                     # [kk B, T, F]
    anr = None
    if Ca:
        anr = (a.view(kk, 1, 1, 1) * d["anom"].double()).reshape(kk * B, T, Ca).requires_grad_(True)
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
def test_ig_reference_two_ways_agree(case):
    """The plain float64 reference == eager pooled GeneralConv (eval, float64) on the replicated
    path batch, to 1e-12 relative: output, acc_x and acc_a; masked nodes' acc_x exactly zero."""
    d, r = S.case_reference(case)
    out, acc_x, acc_a = _second_route(case, d)
    assert out.shape == r["out"].shape and acc_x.shape == r["acc_x"].shape and acc_a.shape == r["acc_a"].shape
    _close(out, r["out"], "out")
    _close(acc_x, r["acc_x"], "acc_x")
    _close(acc_a, r["acc_a"], "acc_a")
    dead = ~r["live"][:, None, :, None].expand_as(acc_x)
    assert torch.count_nonzero(r["acc_x"][dead]) == 0 and torch.count_nonzero(acc_x[dead]) == 0
    assert r["acc_x"].abs().max() > 0 and torch.isfinite(r["acc_x"]).all() and torch.isfinite(r["out"]).all()


def test_reference_takes_the_slope_side_at_zero():
    """At y == 0 exactly the reference's PReLU derivative is the slope ``a`` (the kernels' ``y > 0``
    predicate): a0_zero's first path point has y = 0 for every node and channel."""
    c = next(c for c in S.IG_CASES if c.name == "a0_zero")
    d, r = S.case_reference(c)
    assert torch.count_nonzero(r["y"][0]) == 0
    assert torch.count_nonzero(d["bias"]) == 0 and torch.count_nonzero(d["shift"]) == 0
    # every live pair with positive scaled x W flips, and flips at index 1; the others never flip
    xw = torch.matmul(d["x"].double(), d["W"].double()) * d["scale"].double()
    assert torch.equal(r["flip"], xw > 0)
    assert (r["j"][r["flip"]] == 1).all() and (r["j"][~r["flip"]] == d["kk"]).all()
    assert not r["ambiguous"].any()                      # exact zeros are not ambiguous
    # the step at alpha = 0 carries weight wt_0 with derivative a, not 1: check one element by hand
    b, t, n = 0, 0, 0
    kk, Ca = d["kk"], c.Ca
    al, wts = d["prelu_alpha"].double(), d["wts"].double()
    gs = d["g"].double()[t, b:kk * c.B:c.B, Ca:Ca + c.F]                              # [kk, F]
    dact = torch.where(xw[b, t, n] > 0, torch.ones(c.F).double(), al).expand(kk, c.F).clone()
    dact[0] = al
    hand = torch.einsum("s,sf,kf->k", wts, dact * gs, d["W"].double() * d["scale"].double()) * d["w"][b, n].double()
    assert (hand - r["acc_x"][b, t, n]).abs().max() <= 1e-12 * hand.abs().max()


def test_builder_properties():
    for c in S.IG_CASES:
        d = S.ig_inputs(c)
        m = d["mask"]
        assert (m[:, 0] == 1).all(), c.name
        if c.B > 1:
            assert m[1].sum() == 1
        if c.B * c.N >= 40:
            assert (m == 0).any()
        assert torch.count_nonzero(d["x"] * (1 - m)[:, None, :, None]) == 0
        assert torch.count_nonzero(d["w"] * (1 - m)) == 0 and (d["w"][m != 0] > 0).all()
        assert torch.equal(d["prelu_alpha"][:4], torch.tensor(S.PINNED_PRELU))
        assert (d["scale"] < 0).any() and (d["scale"] > 0).any()
        assert d["anom"].numel() == c.B * c.T * c.Ca
        assert d["alphas"][0] == 0 and (c.kk == 1 or d["alphas"][-1] == 1)
        assert abs(d["wts"].sum().item() - 1) < 1e-6
        assert tuple(d["g"].shape) == (c.T, S.case_mp(c) + c.mp_extra, S.case_cp(c))
        d2 = S.ig_inputs(c)
        assert all(torch.equal(d[k], d2[k]) for k in d if isinstance(d[k], torch.Tensor))


@pytest.mark.parametrize("case", S.IG_CASES, ids=_IDS)
def test_ig_case_reaches_its_branches(case):
    c = case
    assert c.tags, c.name
    assert (c.Cin, c.F) in S.IGG_PAIRS and 1 <= c.N <= S.IGG_NMAX and c.Ca <= min(4, c.F) and c.T in (2, 3)
    for tag in c.tags:
        assert S.IG_PREDICATES[tag](c), f"{c.name} no longer reaches '{tag}'"
    # the 64 KiB request belongs to one case only
    assert (S.bwd_lds_bytes(c) > S.LDS_DEFAULT) == (c.name == "lds_f32_k128")
    # the forward's LDS request stays small, every tensor of a case stays small
    assert (S.IGG_FSG * S.fwd_bb(c) * S.case_cp(c) + 2 * S.IGG_FSG * S.IGG_THREADS) * 4 <= S.LDS_DEFAULT
    assert c.kk * c.B * c.T * c.N * c.F * 8 < 64 << 20


def test_case_table_covers_the_kernels_surface():
    """Every predicate is claimed by a case, and the shapes the kernels branch on are all present."""
    cs = S.IG_CASES
    assert {t for c in cs for t in c.tags} == set(S.IG_PREDICATES), \
        set(S.IG_PREDICATES) ^ {t for c in cs for t in c.tags}
    assert len({c.name for c in cs}) == len(cs)
    by = {c.name: c for c in cs}
    # template instances
    assert {(c.Cin, c.F) for c in cs} == set(S.IGG_PAIRS)
    assert {S.fwd_nm(c) for c in cs} == set(S.IGG_NM)
    assert {S.fwd_bb(c) for c in cs} == {8, 16, 32}
    assert {c.N for c in cs} >= {1, 7, 8, 9, 16, 17, 24, 25, 32}
    # path slicing of the backward, store passes of the forward, the search's smallest cases
    assert {S.bwd_slices(c) for c in cs} == {1, 2, 3}
    assert {c.kk for c in cs} >= {1, 2, 8, 9, 16, 17, 25, 128, 129, 257}
    assert S.bwd_lds_bytes(by["lds_f32_k128"]) == 74304
    assert [c.name for c in cs if S.bwd_lds_bytes(c) > S.LDS_DEFAULT] == ["lds_f32_k128"]
    # tails and padding
    assert {c.Ca for c in cs} == {0, 1, 2, 4}
    assert any(c.B % S.fwd_bb(c) and c.B > S.fwd_bb(c) for c in cs) and any(c.B % S.IGG_BWB == 0 for c in cs)
    assert S.case_cp(by["pad_wide"]) == 24 and S.min_cp(by["pad_wide"]) == 20 and by["pad_wide"].mp_extra == 32
    assert any(S.case_mp(c) > c.kk * c.B for c in cs)
    assert by["a0_zero"].zero_a0 and sum(c.zero_a0 for c in cs) == 1
    assert S.ACCUMULATE_CHUNKS == ((0, 6), (6, 12), (12, 17))
    assert set(S.REFUSED_SHAPES) >= {(2, 64, 9), (4, 16, 9), (2, 16, 33)}
    assert (S.IGG_NMAX, S.IGG_FSG, S.IGG_KMAX, S.IGG_BWB) == (32, 8, 128, 4)


@pytest.mark.parametrize("case", S.IG_CASES, ids=_IDS)
def test_flips_inside_the_path_and_ambiguity_cap(case):
    """At least 15 % of a case's live (node, channel) pairs change sign inside the path (kk1 has a
    single point), and at most 10 % of its live elements have an ambiguous sign."""
    c = case
    d, r = S.case_reference(c)
    share, amb = S.flip_share(c, r), S.ambiguous_share(c, r)
    print(f"{c.name}: flips {share:.3f} ambiguous {amb:.4f}")
    if c.kk == 1:
        assert share == 0
    else:
        assert share >= S.MIN_FLIP_SHARE, f"{c.name}: {share:.3f} of the live pairs flip"
        # flips occur on pinned and on random slopes other than 1 (where the two sides differ)
        lv = r["live"][:, None, :, None]
        assert (r["flip"] & lv)[..., (0, 2, 3)].any() and (r["flip"] & lv)[..., 4:].any()
    assert amb <= S.AMBIGUOUS_CAP, f"{c.name}: {amb:.3f} of the live elements are ambiguous"
    # the looser bound is zero exactly where nothing is ambiguous
    assert torch.count_nonzero(r["loose"][~r["ambiguous"]]) == 0


def test_accumulate_path_of_17_has_flips_in_every_chunk():
    c = next(c for c in S.IG_CASES if c.name == "accumulate")
    d, r = S.case_reference(c, S.ACCUMULATE_CHUNKS[-1][1])
    assert S.flip_share(c, r) >= S.MIN_FLIP_SHARE and S.ambiguous_share(c, r) <= S.AMBIGUOUS_CAP
    j = r["j"][r["flip"] & r["live"][:, None, :, None]]
    for s0, s1 in S.ACCUMULATE_CHUNKS:
        assert ((j >= s0) & (j < s1)).any(), (s0, s1)


def test_slices_257_flips_in_each_slice():
    """Flip indices fall in each of the three backward slices [0, 128), [128, 256), [256, 257), and on
    both sides of the first slice boundary."""
    c = next(c for c in S.IG_CASES if c.name == "slices_257")
    d, r = S.case_reference(c)
    j = r["j"][r["flip"] & r["live"][:, None, :, None]]
    for s0 in range(0, c.kk, S.IGG_KMAX):
        n = ((j >= s0) & (j < min(c.kk, s0 + S.IGG_KMAX))).sum().item()
        assert n >= 1, f"no flip index in slice [{s0}, {s0 + S.IGG_KMAX})"
    assert ((j > 96) & (j < 128)).any() and ((j >= 128) & (j < 160)).any()


def _closed_form_acc_x(c, d, r, j):
    """acc_x from the kernels' closed form in float64: per (window, step, node, channel) the PReLU
    derivative is c0 before the flip index j and c1 from it on, so with the prefix sums P(j) =
    sum_{s<j} wt_s g_f(s) and Q = P(kk): H = c0 P(j) + c1 (Q - P(j)), acc_x = w sum_f W_kf sc_f H."""
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


@pytest.mark.parametrize("name", ["kk2", "kk9", "a0_zero", "slices_257", "lds_f32_k128"])
def test_bound_rejects_a_flip_index_off_by_one(name):
    """The closed form the kernels use equals the reference with the reference's flip indices, and
    leaves the backward bound (the looser one of ambiguous elements included) for nearly every
    affected element when every flip index is one step late."""
    c = next(c for c in S.IG_CASES if c.name == name)
    d, r = S.case_reference(c)
    good = _closed_form_acc_x(c, d, r, r["j"])
    _close(good, r["acc_x"], "closed form")
    late = torch.where(r["flip"], (r["j"] + 1).clamp(max=d["kk"]), r["j"])
    bad = _closed_form_acc_x(c, d, r, late)
    ratio = (bad - r["acc_x"]).abs() / (r["bwd_bound"] + r["loose"])
    # elements with a flip on a channel whose two slopes differ
    hit = (r["flip"] & (d["prelu_alpha"] != 1) & r["live"][:, None, :, None]).any(-1)          # [B,T,N]
    assert hit.sum() >= 10
    caught = (ratio.max(-1).values > 1)[hit].double().mean().item()
    print(f"{name}: {caught:.3f} of {int(hit.sum())} affected elements leave the bound, median ratio "
          f"{ratio.max(-1).values[hit].median().item():.0f}")
    assert caught >= 0.95
