"""CPU part of the time-major LSTM kernel tests (``tests/test_lstm_tm_kernels_gpu.py``): every case
of the GPU table is checked to still reach the kernel branches it names (the host's predicates are
recomputed here from the shapes and the per-case environment), the oracle is checked a second way
(float64 autograd of the eager LSTM, ``max_unpool1d``), and the discriminating power of the GPU
bounds is asserted from the reference alone: every named mutant of the reference that applies to a
case lies at least 5x the bound away in the GPU test's metric."""
import pytest
import torch

import test_lstm_tm_kernels_gpu as S

_IDS = [c.name for c in S.TM_CASES]

# ------------------------------------------------------------------ constants of lstm_tm_fwd.hip / lstm_tm_bwd.hip, mirrored
K_H = (16, 32, 64)              # tm_supported
K_H_PAIR = (16, 32)             # lstm_tm2_fwd, tm_rg_ok, tm_fused_wgrad
K_DIN_MAX = 127                 # tm_supported
K_FUSED_DIN_MAX = 64            # tm_fused_wgrad, the recompute-gates backward
K_MIN_TILES_DEFAULT = 64        # GNNQC_TM_FUSED_WGRAD_MIN_TILES
K_GR_CB = 64                    # lstm_grads: gate columns per column block
K_GROUP_SPLITS = 512            # split records per reduction group
K_FWD_D = 6                     # TM_FWD_D: lstm_tm_fwd / lstm_tm2_fwd ring depth
K_BWD_D, K_BWD_D_H64 = 4, 2     # tm_bwd_depth
K_RG_D = 4                      # TM_RG_D: frozen recompute-gates backward
K_TMW_D16, K_TMW_D32 = 4, 6     # lstm_tm_bwd_wg_kernel
K_ELEMS_SECOND_REFERENCE = 200000       # Mp T (Din + 4 H): cases above it skip the autograd route


def tm_granule(Din, off):
    a = 4 * off                                     # the base pointer mod 16 (buffers are 512-byte aligned)
    if Din % 4 == 0 and a % 16 == 0:
        return 4
    if Din % 2 == 0 and a % 8 == 0:
        return 2
    return 1


def tm_supported(H, Din, gr):
    return H in K_H and 1 <= Din <= K_DIN_MAX and (16 * Din) // gr <= 16 * H


def tm_rg_ok(H, gr):
    return H in K_H_PAIR and gr == 4


def kx(Din):
    n = (Din + 31) // 32
    return n if n <= 2 else 4


def col_blocks(H):
    return 4 * H // K_GR_CB


def layer_dims(c):
    """(Din, granule) of each lstm_tm_bwd call of the case: the pair's layer B reads hA (H channels)."""
    gr = tm_granule(c.Din, c.off)
    return [(c.Din, gr)] if c.kind == "single" else [(c.H, 4), (c.Din, gr)]


def fused_wgrad(c, Din, gr):
    if not (c.bwd and c.wg):
        return False
    if c.mode == "rg":
        return True
    return c.fused and c.H in K_H_PAIR and gr == 4 and Din <= K_FUSED_DIN_MAX and c.tiles >= c.min_tiles


def any_fused(c):
    return any(fused_wgrad(c, D, g) for D, g in layer_dims(c))


def rows_pass(c):
    return c.bwd and c.wg and not all(fused_wgrad(c, D, g) for D, g in layer_dims(c))


def rec_dx(c):
    return rows_pass(c) and c.need_dx and col_blocks(c.H) > 1 and c.recdx


def dx_slabs(c):
    return rows_pass(c) and c.need_dx and col_blocks(c.H) > 1 and not c.recdx


def bwd_ring(c):
    if any_fused(c):
        return K_TMW_D16 if c.H == 16 else K_TMW_D32
    if c.mode == "rg":
        return K_RG_D
    return K_BWD_D_H64 if c.H >= 64 else K_BWD_D


def rings(c):
    return {K_FWD_D} | ({bwd_ring(c)} if c.bwd else set())


def up_on_load(c):
    """The recurrence un-pools on load: the fused kernel, a frozen path, or the rec-dx recurrence."""
    return bool(c.P) and c.bwd and (any_fused(c) or not c.wg or rec_dx(c))


PREDICATES = {
    "fwd_eval": lambda c: c.kind == "single" and c.mode == "eval",
    "fwd_sg": lambda c: c.kind == "single" and c.mode == "sg",
    "fwd_rg": lambda c: c.kind == "single" and c.mode == "rg" and tm_rg_ok(c.H, tm_granule(c.Din, c.off)),
    "dw_lt_din": lambda c: c.Dw < c.Din,
    "kx1": lambda c: kx(c.Din) == 1,
    "kx2": lambda c: kx(c.Din) == 2,
    "kx4_from3": lambda c: kx(c.Din) == 4 and (c.Din + 31) // 32 == 3 and c.H == 64,
    "kx4": lambda c: (c.Din + 31) // 32 == 4 and c.H == 64,
    "gr4": lambda c: tm_granule(c.Din, c.off) == 4,
    "gr2": lambda c: tm_granule(c.Din, c.off) == 2,
    "gr1": lambda c: tm_granule(c.Din, c.off) == 1,
    "misaligned_base": lambda c: c.off % 4 != 0 and c.Din % 4 == 0,
    "t1": lambda c: c.T == 1,
    "t_even": lambda c: c.T % 2 == 0,
    "t_odd": lambda c: c.T % 2 == 1 and c.T > 1,
    "t_lt_ring": lambda c: any(c.T < D for D in rings(c)),
    "t_eq_ring": lambda c: c.T in rings(c),
    "wg_fused": lambda c: any_fused(c),
    "wg_last": lambda c: any_fused(c) and c.last,
    "wg_nodx": lambda c: any_fused(c) and not c.need_dx,
    "wg_rg": lambda c: any_fused(c) and c.mode == "rg",
    "wg_kx2": lambda c: any_fused(c) and kx(c.Din) == 2,
    "wg_rows": lambda c: rows_pass(c),
    "wg_off": lambda c: rows_pass(c) and not c.fused and c.tiles >= c.min_tiles,
    "rec_dx": lambda c: rec_dx(c),
    "dx_slabs": lambda c: dx_slabs(c),
    "rec_dx_last": lambda c: rec_dx(c) and c.last and c.H == 64,
    "ng1": lambda c: any_fused(c) and S.n_groups(c) == 1,
    "splits_gt_512": lambda c: any_fused(c) and c.tiles > K_GROUP_SPLITS and S.n_groups(c) == 1,
    "ng2": lambda c: any_fused(c) and S.n_groups(c) == 2,
    "ng2_ragged": lambda c: any_fused(c) and S.n_groups(c) == 2 and c.tiles % (16 * 2) != 0,
    "up": lambda c: up_on_load(c),
    "up_tail1": lambda c: bool(c.P) and c.T % c.P == 1,
    "up_tail2": lambda c: bool(c.P) and c.T % c.P == 2,
    "up_p1": lambda c: c.P == 1,
    "up_single": lambda c: bool(c.P) and c.T // c.P == 1,
    "up_lt_ring": lambda c: up_on_load(c) and c.T < bwd_ring(c),
    "up_fallback": lambda c: bool(c.P) and rows_pass(c) and not rec_dx(c),
    "pair_eval": lambda c: c.kind == "pair" and c.mode == "eval",
    "pair_sg": lambda c: c.kind == "pair" and c.mode == "sg",
    "pair_rg": lambda c: c.kind == "pair" and c.mode == "rg",
    "xb": lambda c: c.kind == "pair" and c.mode == "rg" and c.bwd,
    "hb": lambda c: c.kind == "pair" and c.mode == "rg" and c.bwd,
    "pair_pool": lambda c: c.kind == "pair" and c.pool > 0,
    "one_tile": lambda c: c.tiles == 1,
    "pad_rows": lambda c: c.M < 16 * c.tiles,
}
# the tags of the issue's case table
REQUIRED_TAGS = {
    "fwd_eval", "fwd_sg", "fwd_rg", "dw_lt_din", "kx1", "kx2", "kx4_from3", "kx4", "gr4", "gr2", "gr1",
    "misaligned_base", "t1", "t_lt_ring", "t_eq_ring", "t_even", "t_odd", "wg_fused", "wg_last", "wg_nodx", "wg_rg",
    "wg_kx2", "wg_rows", "rec_dx", "dx_slabs", "rec_dx_last", "splits_gt_512", "ng2", "ng2_ragged", "up", "up_tail1",
    "up_tail2", "up_p1", "up_single", "up_lt_ring", "up_fallback", "pair_eval", "pair_sg", "pair_rg", "xb", "hb",
    "pair_pool", "one_tile", "pad_rows"}


@pytest.mark.parametrize("case", S.TM_CASES, ids=_IDS)
def test_tm_case_reaches_its_branches(case):
    c = case
    assert c.tags and c.family in S.FAMILIES, c.name
    gr = tm_granule(c.Din, c.off)
    assert tm_supported(c.H, c.Din, gr), c.name
    assert 1 <= c.Dw <= c.Din and 1 <= c.M <= 16 * c.tiles and c.T >= 1 and c.off in (0, 1, 2)
    assert c.mode in ("eval", "sg", "rg") and (c.mode != "eval" or not c.bwd)
    assert c.min_tiles in (1, K_MIN_TILES_DEFAULT, 100000)
    if c.mode == "rg":
        assert tm_rg_ok(c.H, gr) and c.Din <= K_FUSED_DIN_MAX
    if c.kind == "pair":
        assert c.H in K_H_PAIR and not c.P and not c.last and (not c.pool or c.T // c.pool >= 1)
    if c.P:
        assert not c.last and 1 <= c.P <= 255 and c.T // c.P >= 1
        # the host refuses un-pooling on a frozen or rec-dx recurrence with granules below 16 bytes
        assert gr == 4 or (rows_pass(c) and not rec_dx(c))
    for tag in c.tags:
        assert PREDICATES[tag](c), f"{c.name} no longer reaches '{tag}'"
    # every tensor of a case stays small
    assert 16 * c.tiles * c.T * (c.Din + 4 * c.H) * 8 < 64 << 20


def test_case_table_covers_the_dispatch_space():
    cs = S.TM_CASES
    used = {t for c in cs for t in c.tags}
    assert REQUIRED_TAGS <= used, REQUIRED_TAGS - used
    assert used == set(PREDICATES), used ^ set(PREDICATES)
    assert len({c.name for c in cs}) == len(cs)
    assert {c.family for c in cs} == set(S.FAMILIES)
    # ring edges: every T of the issue's list on every recurrence of the ring family
    ring = [c for c in cs if c.family == "ring"]
    for key in ((32, "sg", False), (64, "sg", False), (16, "sg", True), (32, "sg", True), (16, "rg", False)):
        assert {c.T for c in ring if (c.H, c.mode, c.wg) == key} == {1, 2, 3, 4, 5, 6, 7, 12, 13}, key
    assert {bwd_ring(c) for c in ring} == {2, 4, 6}
    # un-pooling: every (T, P) on every un-pooling recurrence
    tp = {(12, 3), (13, 3), (14, 3), (7, 1), (5, 5), (9, 4), (3, 2)}
    for key in ((16, "sg", False), (32, "sg", False), (64, "sg", False), (16, "rg", False), (16, "sg", True),
                (32, "rg", True)):
        assert {(c.T, c.P) for c in cs if c.family == "up" and up_on_load(c) and (c.H, c.mode, c.wg) == key
                and not rec_dx(c)} == tp, key
    assert {c.tiles for c in cs if c.family == "records"} == {3, 513, 1024, 1029}
    assert {(c.Din, c.off, tm_granule(c.Din, c.off)) for c in cs if c.family == "granule"} >= \
        {(20, 0, 4), (18, 0, 2), (19, 0, 1), (7, 0, 1), (20, 2, 2), (20, 1, 1)}
    assert {kx(c.Din) for c in cs if c.H == 64} == {1, 2, 4}
    assert {col_blocks(h) for h in K_H} == {1, 2, 4}
    assert (S.OUT_BOUND, S.GRAD_BOUND) == (3e-3, 8e-3)
    assert set(S.BOUNDS) == set(S.FAMILIES) and all(0 < v <= S.OUT_BOUND for v in S.BOUNDS.values())


# ------------------------------------------------------------------ the reference, a second way
def _small(c):
    return 16 * c.tiles * c.T * (c.Din + 4 * c.H) <= K_ELEMS_SECOND_REFERENCE


@pytest.mark.parametrize("case", S.TM_CASES, ids=_IDS)
def test_hand_written_reference_is_the_oracle(case):
    """layer_ref without a mutant == KernelLSTM (rounding on, the case's saved-state mode) and its own
    backward, bit for bit up to summation order (1e-12)."""
    c = case
    d, r = S.case_reference(c)
    mine = S.tm_reference(c, d)
    for q in S.compared_quantities(c):
        a, b = mine[q], r[q].view(mine[q].shape)
        if q == "hA" and c.mode == "rg":
            a = S._bf(a)
        assert (a - b).abs().max().item() <= 1e-12 * max(1.0, b.abs().max().item()), (c.name, q)


@pytest.mark.parametrize("case", [c for c in S.TM_CASES if _small(c)], ids=[c.name for c in S.TM_CASES if _small(c)])
def test_oracle_without_rounding_is_autograd(case):
    """KernelLSTM (rounding=False, the case's saved-state mode) == float64 autograd of lstm_eager on the
    case's inputs, about 1e-10; the test's un-pooling == max_unpool1d."""
    from gnnqc.ops.lstm import lstm_eager
    from gnnqc.ops.lstm_ref import KernelLSTM
    c = case
    d = S.tm_inputs(c)
    dh = S.dh_full(c, d)
    names = ("W", "U", "b") + (("WB", "UB", "bB") if c.kind == "pair" else ())

    def run(fn):
        x = d["x"][:, :, :c.Dw].double().transpose(0, 1).contiguous().requires_grad_(True)
        ps = [d[n].double().requires_grad_(True) for n in names]
        out = fn(x, *ps[:3])
        if c.kind == "pair":
            out = fn(out, *ps[3:])
        return [out.detach()] + list(torch.autograd.grad((out * dh).sum(), [x] + ps))

    a = run(lambda x, W, U, b: KernelLSTM.apply(x, W, U, b, True, False, S.saved_mode(c)))
    e = run(lambda x, W, U, b: lstm_eager(x, W, U, b, True))
    for u, v in zip(a, e):
        assert (u - v).abs().max().item() <= 1e-10 * max(1.0, v.abs().max().item()), c.name
    if c.P:
        To, Mp, H = d["dh"].shape
        idx = (torch.arange(To).view(To, 1, 1) * c.P + d["pidx"].long()).permute(1, 2, 0).reshape(1, Mp * H, To)
        ref = torch.nn.functional.max_unpool1d(d["dh"].double().permute(1, 2, 0).reshape(1, Mp * H, To), idx, c.P,
                                               output_size=(c.T,))
        mine = S.unpool64(d["dh"], d["pidx"], c.T, c.P)
        assert torch.equal(mine.permute(1, 2, 0).reshape(1, Mp * H, c.T), ref)
        assert torch.count_nonzero(mine[To * c.P:]) == 0


def test_pool64_is_max_pool1d():
    g = torch.Generator().manual_seed(2)
    h = torch.randn(13, 5, 4, generator=g, dtype=torch.float64)
    pooled, arg, gap = S._pool64(h, 3)
    ref, idx = torch.nn.functional.max_pool1d(h.permute(1, 2, 0), 3, return_indices=True)
    assert torch.equal(pooled.permute(1, 2, 0), ref)
    assert torch.equal(arg.permute(1, 2, 0) + 3 * torch.arange(4), idx)
    assert (gap > 0).all()


# ------------------------------------------------------------------ discriminating power
_GRADS = ("dx", "dW", "dU", "db")


def mutants_of(c):
    """Mutant name -> the compared quantities (by kind) it must move by at least 5x their bound. Decided
    from the case's structure alone, never from the distance."""
    if not c.bwd:
        return {}
    T = c.T
    m = {}
    if T >= 2:
        m["dh_shift"] = set(_GRADS)
    if c.P > 1:
        m["up_phase"] = set(_GRADS)
    if c.P and T % c.P:
        m["up_tail"] = set(_GRADS)
    m["forget_c"] = set(_GRADS) - ({"dU"} if T == 1 else set())
    if c.wg:
        m["wg_final"] = {"dW", "db"} | ({"dU"} if T % 2 == 0 else set())
        if T >= 2:
            m["du_h"] = {"dU"}
        m["tile"] = {"dW", "dU", "db"} - ({"dU"} if T == 1 else set())
        if S.n_groups(c) > 1 and any_fused(c):
            m["group"] = {"dW", "dU", "db"}
    return m


@pytest.mark.parametrize("case", [c for c in S.TM_CASES if c.bwd], ids=[c.name for c in S.TM_CASES if c.bwd])
def test_every_mutant_is_five_bounds_away(case):
    """Each named mutant of the reference, in the GPU test's metric (relative Frobenius norm against the
    unmutated reference), lies at least 5x the quantity's bound away for every compared quantity it
    applies to."""
    c = case
    d, _ = S.case_reference(c)
    ref = S.tm_reference(c, d)
    qs = [q for q in S.compared_quantities(c) if S.quantity_kind(q) != "h"]
    worst = float("inf")
    for name, kinds in mutants_of(c).items():
        mut = S.tm_reference(c, d, name)
        for q in qs:
            if S.quantity_kind(q) not in kinds or ref[q].norm().item() == 0:
                continue
            dist = S.rel_err(mut[q], ref[q])[0]
            ratio = dist / S.bound_of(c, q)
            worst = min(worst, ratio)
            assert ratio >= S.MUTANT_FACTOR, f"{c.name}: mutant {name} moves {q} by {dist:.3e}, {ratio:.1f} bounds"
    assert worst < float("inf"), c.name
    print(f"TMMUT {c.name} {worst:.1f}")
