"""Time-major LSTM kernels (``csrc/kernels/lstm_tm_fwd.hip``: ``lstm_tm_fwd``, ``lstm_tm2_fwd``;
``csrc/kernels/lstm_tm_bwd.hip``: ``lstm_tm_bwd``) called directly through ``hip_ops()``, over their template instances, ring
prologues, granules, weight-gradient paths, record reduction, un-pooling and the layer pair, against
the rounding-aware float64 oracle :class:`gnnqc.ops.lstm_ref.KernelLSTM` on the CPU
(``rounding=True``; ``saved="rg"`` where the backward recomputes its gates; two stacked layers for
the pair). The outputs and every gradient are taken by the oracle's own backward.

A case selects its branch by its arguments (``train``, ``store_gates``, empty or non-empty
``dW/dU/db``, ``need_dx``, 2-D or 3-D ``dh``, ``pidx/pool``, the dtype of x / h) and by the three
switches the host reads per call (``GNNQC_TM_FUSED_WGRAD_MIN_TILES``, ``GNNQC_TM_FUSED_WGRAD``,
``GNNQC_TM_RECDX``). Every case names the branches it is there to reach (``tags``); their predicates
are recomputed from the shapes in ``tests/test_lstm_tm_reference_cpu.py`` (no GPU needed), which also
checks the oracle a second way and that every named mutant of the reference (:func:`layer_ref`
``mut``) lies at least 5x the bound away in the metric used here.

Metric: relative Frobenius norm per tensor (the project's metric for this oracle), over all Mp rows
(pad rows are ordinary sequences with x = 0 and dh = 0). The bounds (:data:`BOUNDS`) are per family:
the smaller of the project's bound for this oracle (3e-3 on outputs, 8e-3 on gradients) and 3x the
worst error measured in the family on an MI355X, rounded up to one significant digit; the measured
errors of every case are in ``profiles/lstm_tm_kernel_tests.txt``. (An output's error is about 1e-7
until one bf16 operand rounds the other way in fp32 than in float64, which moves it to 1e-5..1e-4:
one bound per family, not per quantity, keeps such a flip inside the 3x margin.) A recompute-gates
pair returns layer A's h in bf16 (TM_RG_BF16H); it is compared with the oracle's hA rounded to bf16.
Nothing is compared with a kernel's own output, except that the recompute-gates forward's h must be
within 1e-5 of the saved-gates forward's. Exact checks (no tolerance): dx of pad rows and of channels
>= Dw is 0, a quantity whose reference is identically 0 (dU at T = 1) is 0, non-empty ``dW/dU/db``
are accumulated into (they are pre-filled, the pre-fill is subtracted). A pair's in-launch
MaxPooling1D is compared with the float64 max-pool of the oracle's hB: the pooled values in the
same metric, the argmax bytes wherever the two largest candidates differ by more than the bound
times the largest |hB|.
"""
from collections import namedtuple

import pytest
import torch

pytestmark = pytest.mark.gpu

OUT_BOUND, GRAD_BOUND = 3e-3, 8e-3          # the project's bounds for this oracle
FAMILIES = ("fwd", "kx", "granule", "ring", "wg_fused", "wg_rows", "records", "up", "pair", "tiles")
# one bound per family (a row of the case table): 3 x the worst error measured in the family on an MI355X over
# all its cases and quantities, rounded up to one significant digit (profiles/lstm_tm_kernel_tests.txt); a
# quantity is held to the smaller of it and the project's bound for its kind (bound_of)
BOUNDS = {"fwd": 2e-3, "kx": 6e-4, "granule": 2e-3, "ring": 2e-3, "wg_fused": 1e-3, "wg_rows": 2e-3, "records": 3e-4,
          "up": 2e-3, "pair": 2e-3, "tiles": 4e-4}
MUTANT_FACTOR = 5.0

TMCase = namedtuple("TMCase", "name family kind H Din Dw T tiles M mode bwd wg need_dx last P off min_tiles fused "
                              "recdx pool tags")


def _c(name, family, H, Din, T, tiles, tags, kind="single", Dw=None, M=None, mode="sg", bwd=None, wg=False,
       need_dx=True, last=False, P=0, off=0, min_tiles=64, fused=True, recdx=True, pool=0):
    return TMCase(name, family, kind, H, Din, Din if Dw is None else Dw, T, tiles, 16 * tiles if M is None else M,
                  mode, (mode != "eval") if bwd is None else bwd, wg, need_dx, last, P, off, min_tiles, fused, recdx,
                  pool, tuple(tags))


def _parity(T):
    return ("t1",) if T == 1 else (("t_even",) if T % 2 == 0 else ("t_odd",))


def _tm_cases():
    cs = []
    # ---- forward instances: H x {eval, train + gates, train + recomputed gates}, Dw = Din and Dw < Din
    for H in (16, 32, 64):
        for Din, Dw in ((20, 20), (20, 18)):
            for mode in ("eval", "sg", "rg"):
                if mode == "rg" and H == 64:
                    continue
                tags = ["fwd_" + mode, "gr4", "kx1"] + (["dw_lt_din"] if Dw < Din else [])
                cs.append(_c(f"fwd_h{H}_d{Dw}of{Din}_{mode}", "fwd", H, Din, 7, 2, tags, Dw=Dw, mode=mode))
    cs.append(_c("fwd_h32_d19of20_sg_wg", "fwd", 32, 20, 7, 2, ("fwd_sg", "dw_lt_din", "rec_dx"), Dw=19, wg=True))
    # ---- KX: x channel blocks of 32 (H = 64 reaches 4; 3 is sent to 4)
    for Din, tag in ((32, "kx1"), (64, "kx2"), (96, "kx4_from3"), (124, "kx4")):
        cs.append(_c(f"kx_h64_d{Din}_frozen", "kx", 64, Din, 5, 2, (tag, "fwd_sg")))
        cs.append(_c(f"kx_h64_d{Din}_wg", "kx", 64, Din, 5, 2, (tag, "rec_dx"), wg=True))
    cs.append(_c("kx_h64_d124_eval", "kx", 64, 124, 5, 2, ("kx4", "fwd_eval"), mode="eval"))
    cs.append(_c("kx_h16_d64_frozen", "kx", 16, 64, 5, 2, ("kx2",)))
    cs.append(_c("kx_h16_d64_rg", "kx", 16, 64, 5, 2, ("kx2", "fwd_rg"), mode="rg"))
    cs.append(_c("kx_h16_d64_fused", "kx", 16, 64, 5, 2, ("kx2", "wg_fused", "wg_kx2"), wg=True, min_tiles=1))
    # ---- granules: Din % 4, Din % 2 and a misaligned base pointer; forward, frozen dx, weight gradients
    for Din, off, tag in ((20, 0, "gr4"), (18, 0, "gr2"), (19, 0, "gr1"), (7, 0, "gr1"), (20, 2, "gr2"),
                          (20, 1, "gr1")):
        mis = ["misaligned_base"] if off else []
        nm = f"gran_h32_d{Din}" + (f"_off{off}" if off else "")
        cs.append(_c(nm + "_frozen", "granule", 32, Din, 7, 2, [tag] + mis, off=off))
        cs.append(_c(nm + "_wg", "granule", 32, Din, 7, 2, [tag, "wg_rows"] + mis, off=off, wg=True))
        cs.append(_c(nm + "_eval", "granule", 32, Din, 7, 2, [tag, "fwd_eval"] + mis, off=off, mode="eval"))
    cs.append(_c("gran_h16_d18_wg", "granule", 16, 18, 7, 2, ("gr2", "wg_rows"), wg=True))
    cs.append(_c("gran_h16_d7_wg", "granule", 16, 7, 7, 2, ("gr1", "wg_rows"), wg=True))
    cs.append(_c("gran_h64_d19_wg", "granule", 64, 19, 7, 2, ("gr1", "rec_dx"), wg=True))
    cs.append(_c("gran_h64_d20_off2_frozen", "granule", 64, 20, 7, 2, ("gr2", "misaligned_base"), off=2))
    # ---- short and ring-edge T (forward ring 6; backward 4, H = 64: 2; fused weight gradients 4 / 6)
    for T in (1, 2, 3, 4, 5, 6, 7, 12, 13):
        for nm, H, ring, kw in (("sg_h32", 32, 4, {}), ("sg_h64", 64, 2, {}),
                                ("fused_h16", 16, 4, dict(wg=True, min_tiles=1)),
                                ("fused_h32", 32, 6, dict(wg=True, min_tiles=1)),
                                ("rg_h16", 16, 4, dict(mode="rg"))):
            tags = list(_parity(T))
            if T < 6 or T < ring:
                tags.append("t_lt_ring")
            if T in (6, ring):
                tags.append("t_eq_ring")
            cs.append(_c(f"ring_{nm}_t{T}", "ring", H, 20, T, 2, tags, **kw))
    # ---- weight gradients inside the recurrence
    k = 0
    for H in (16, 32):
        for Din in (20, 64):
            for need_dx in (True, False):
                for last in (True, False):
                    for rg in (True, False):
                        tags = ["wg_fused"] + (["wg_last"] if last else []) + ([] if need_dx else ["wg_nodx"]) + \
                               (["wg_rg"] if rg else []) + (["wg_kx2"] if Din > 32 else []) + ["pad_rows"]
                        T = (3, 4)[k % 2] if last else (5, 6)[k % 2]
                        k += 1
                        cs.append(_c(f"wgf_h{H}_d{Din}_{'dx' if need_dx else 'nodx'}_{'last' if last else 'seq'}_"
                                     f"{'rg' if rg else 'sg'}", "wg_fused", H, Din, T, 3, tags, M=40, wg=True,
                                     need_dx=need_dx, last=last, mode="rg" if rg else "sg", min_tiles=1))
    # ---- separate weight-gradient pass
    for need_dx in (True, False):
        for last in (True, False):
            cs.append(_c(f"wgr_h16_{'dx' if need_dx else 'nodx'}_{'last' if last else 'seq'}", "wg_rows", 16, 20,
                         3 if last else 5, 3, ("wg_rows", "pad_rows"), M=40, wg=True, need_dx=need_dx, last=last,
                         min_tiles=100000))
    for H in (32, 64):
        cs.append(_c(f"wgr_h{H}_recdx", "wg_rows", H, 20, 5, 3, ("wg_rows", "rec_dx"), M=40, wg=True, min_tiles=100000))
        cs.append(_c(f"wgr_h{H}_recdx_last", "wg_rows", H, 20, 3, 3,
                     ("wg_rows", "rec_dx") + (("rec_dx_last",) if H == 64 else ()), M=40, wg=True, last=True,
                     min_tiles=100000))
        cs.append(_c(f"wgr_h{H}_slabs", "wg_rows", H, 20, 5, 3, ("wg_rows", "dx_slabs"), M=40, wg=True,
                     min_tiles=100000, recdx=False))
        cs.append(_c(f"wgr_h{H}_nodx", "wg_rows", H, 20, 6, 3, ("wg_rows",), M=40, wg=True, need_dx=False,
                     min_tiles=100000))
    cs.append(_c("wgr_h64_slabs_last", "wg_rows", 64, 20, 3, 3, ("wg_rows", "dx_slabs"), M=40, wg=True, last=True,
                 min_tiles=100000, recdx=False))
    cs.append(_c("wgr_h32_fused_off", "wg_rows", 32, 20, 5, 3, ("wg_rows", "wg_off", "rec_dx"), M=40, wg=True,
                 min_tiles=1, fused=False))
    # ---- record reduction of the fused weight gradients: one split record per tile
    for tiles, tags in ((3, ("ng1",)), (513, ("splits_gt_512", "ng1")), (1024, ("ng2",)),
                        (1029, ("ng2", "ng2_ragged"))):
        cs.append(_c(f"rec_t{tiles}", "records", 16, 4, 2, tiles, ("wg_fused",) + tags, wg=True, min_tiles=1))
    cs.append(_c("rec_t1029_rg_h32", "records", 32, 4, 2, 1029, ("wg_fused", "wg_rg", "ng2", "ng2_ragged"), wg=True,
                 mode="rg", min_tiles=1, need_dx=False))
    # ---- un-pooling on load
    up_tp = ((12, 3, ()), (13, 3, ("up_tail1",)), (14, 3, ("up_tail2",)), (7, 1, ("up_p1",)),
             (5, 5, ("up_single",)), (9, 4, ("up_tail1",)), (3, 2, ("up_tail1", "up_single")))
    for nm, H, ring, kw in (("sg_h16", 16, 4, {}), ("sg_h32", 32, 4, {}), ("sg_h64", 64, 2, {}),
                            ("rg_h16", 16, 4, dict(mode="rg")), ("fused_h16", 16, 4, dict(wg=True, min_tiles=1)),
                            ("fused_rg_h32", 32, 6, dict(wg=True, min_tiles=1, mode="rg"))):
        for T, P, tg in up_tp:
            tags = ("up",) + tg + (("up_lt_ring",) if T < ring else ())
            cs.append(_c(f"up_{nm}_t{T}p{P}", "up", H, 20, T, 2, tags, P=P, **kw))
    for T, P, tg in ((13, 3, ("up_tail1",)), (3, 2, ("up_tail1", "up_single")), (7, 1, ("up_p1",))):
        cs.append(_c(f"up_fallback_h16_t{T}p{P}", "up", 16, 20, T, 2, ("up_fallback", "wg_rows") + tg, P=P, wg=True,
                     min_tiles=100000))
    cs.append(_c("up_fallback_h32_nodx_t14p3", "up", 32, 20, 14, 2, ("up_fallback", "wg_rows", "up_tail2"), P=3,
                 wg=True, need_dx=False, min_tiles=100000))
    cs.append(_c("up_recdx_h32_t13p3", "up", 32, 20, 13, 2, ("up", "rec_dx", "up_tail1"), P=3, wg=True,
                 min_tiles=100000))
    cs.append(_c("up_recdx_h64_t3p2", "up", 64, 20, 3, 2, ("up", "rec_dx", "up_tail1", "up_single"), P=2, wg=True,
                 min_tiles=100000))
    # ---- the layer pair (lstm_tm2_fwd) and the backward of its two layers
    k = 0
    for H in (16, 32):
        for Din, T in ((20, 1), (20, 2), (32, 7), (64, 13), (20, 13)):
            for mode in ("eval", "sg", "rg"):
                wg = bool(k % 2) and mode != "eval"
                k += 1
                pool = 3 if T >= 7 else 0
                tags = ["pair_" + mode] + (["xb", "hb"] if mode == "rg" else []) + (["pair_pool"] if pool else []) + \
                       list(_parity(T))
                cs.append(_c(f"pair_h{H}_d{Din}_t{T}_{mode}" + ("_wg" if wg else ""), "pair", H, Din, T, 2, tags,
                             kind="pair", mode=mode, wg=wg, min_tiles=1, pool=pool))
    cs.append(_c("pair_h16_d20_t7_rg_wg", "pair", 16, 20, 7, 3, ("pair_rg", "xb", "hb", "pad_rows", "wg_rg"),
                 kind="pair", M=40, mode="rg", wg=True, min_tiles=1))
    cs.append(_c("pair_h32_d20_t7_rg_frozen", "pair", 32, 20, 7, 3, ("pair_rg", "xb", "hb", "pad_rows"), kind="pair",
                 M=40, mode="rg"))
    # ---- tiles
    for tiles, M, tg in ((1, 16, ("one_tile",)), (1, 9, ("one_tile", "pad_rows")), (3, 40, ("pad_rows",)),
                         (5, 72, ("pad_rows",))):
        cs.append(_c(f"tiles_{tiles}_m{M}_frozen", "tiles", 16, 20, 7, tiles, tg, M=M))
        cs.append(_c(f"tiles_{tiles}_m{M}_fused", "tiles", 32, 20, 7, tiles, tg + ("wg_fused",), M=M, wg=True,
                     min_tiles=1))
    return cs


TM_CASES = _tm_cases()
_INDEX = {c.name: i for i, c in enumerate(TM_CASES)}


def saved_mode(c):
    return "rg" if c.mode == "rg" else "gates_bf16"


# ------------------------------------------------------------------ input builder (CPU, float32)
def _params(Din, H, gen):
    """Weights scaled like test_kernels_gpu._lstm_params."""
    return (torch.randn(Din, 4 * H, generator=gen) * 0.3, torch.randn(H, 4 * H, generator=gen) * 0.3,
            torch.randn(4 * H, generator=gen) * 0.1)


def tm_inputs(c):
    """randn inputs of one case (seeded by the case): x [T, Mp, Din] with rows >= M and channels >= Dw
    zero, non-zero dout on every live row and zero on pad rows, random argmax bytes in [0, P)."""
    gen = torch.Generator().manual_seed(9100 + 31 * _INDEX[c.name])
    T, Mp, M, H = c.T, 16 * c.tiles, c.M, c.H
    x = torch.zeros(T, Mp, c.Din)
    x[:, :M, :c.Dw] = torch.randn(T, M, c.Dw, generator=gen)
    d = dict(x=x)
    d["W"], d["U"], d["b"] = _params(c.Dw, H, gen)
    if c.kind == "pair":
        d["WB"], d["UB"], d["bB"] = _params(H, H, gen)
    if c.last:
        dh = torch.randn(Mp, H, generator=gen)
        dh[M:] = 0
    else:
        dh = torch.randn(T // c.P if c.P else T, Mp, H, generator=gen)
        dh[:, M:] = 0
    d["dh"] = dh
    if c.P:
        d["pidx"] = torch.randint(0, c.P, dh.shape, generator=gen, dtype=torch.uint8)
    for n in (("W", "U", "b") + (("WB", "UB", "bB") if c.kind == "pair" else ())) if c.wg else ():
        d["pre_" + n] = torch.randn(d[n].shape, generator=gen)
    return d


def unpool64(dh, pidx, T, P):
    """Float64 un-pooling of a pooled gradient [T // P, Mp, H] with argmax bytes: [T, Mp, H], zero in the
    T % P tail."""
    To = T // P
    full = torch.zeros(T, *dh.shape[1:], dtype=torch.float64)
    t_idx = torch.arange(To).view(To, 1, 1) * P + pidx.long()
    return full.scatter_(0, t_idx, dh.double())


def dh_full(c, d, mut=None):
    """The per-step output gradient [Mp, T, H] in float64 the case stands for (``mut``: the input-level
    mutants ``dh_shift``, ``up_phase``, ``up_tail``)."""
    T, P = c.T, c.P
    if c.last:
        full = torch.zeros(T, *d["dh"].shape, dtype=torch.float64)
        full[-1] = d["dh"].double()
    elif P:
        pidx = d["pidx"]
        if mut == "up_phase":
            pidx = (pidx + 1) % P
        full = unpool64(d["dh"], pidx, T, P)
        if mut == "up_tail":
            full[(T // P) * P:] = d["dh"][-1].double()
    else:
        full = d["dh"].double().clone()
    if mut == "dh_shift":                               # every step's gradient lands one step early
        full = torch.cat([full[1:], torch.zeros_like(full[:1])])
    return full.transpose(0, 1).contiguous()


# ------------------------------------------------------------------ float64 references (CPU)
def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def n_groups(c):
    return max(1, c.tiles // 512)


def layer_ref(x, W, U, b, dh, saved, mut=None, NG=1):
    """One layer with the kernels' rounding points written out by hand, float64: x [M, T, D], dh
    [M, T, H] -> (h, dx, dW, dU, db). ``mut=None`` is KernelLSTM (rounding on) operation for operation
    (tests/test_lstm_tm_reference_cpu.py asserts equality); the named mutants are the bugs the GPU
    bounds must tell from it:

    forget_c   c_t instead of c_{t-1} in the forget gate's term
    du_h       h_t instead of h_{t-1} in dU
    wg_final   the weight-gradient kernel's final step pair (t = 0, 1; t = 0 alone at odd T) left out of
               dW / dU / db
    tile       the last 16-row tile left out of dW / dU / db
    group      the last split-record group (tiles with (tile // 16) % NG == NG - 1) left out of them
    """
    M, T, _ = x.shape
    H = U.shape[0]
    Wr, Ur, xr = _bf(W), _bf(U), _bf(x)
    xp = xr @ Wr + b
    h, c = x.new_zeros(M, H), x.new_zeros(M, H)
    hs, cs, gs = [], [], []
    for t in range(T):
        z = xp[:, t] + _bf(h) @ Ur
        i, f, g, o = z.split(H, dim=-1)
        i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
        c = f * c + i * g
        h = o * torch.tanh(c)
        hs.append(h)
        cs.append(c)
        gs.append(torch.cat([i, f, g, o], -1))
    hseq, cseq, gates = torch.stack(hs, 1), torch.stack(cs, 1), torch.stack(gs, 1)
    if saved == "rg":
        cseq = _bf(cseq)
    else:
        gates = _bf(gates)
    dz = hseq.new_zeros(M, T, 4 * H)
    dh_rec, dc = hseq.new_zeros(M, H), hseq.new_zeros(M, H)
    for t in reversed(range(T)):
        dht = dh[:, t] + dh_rec
        i, f, g, o = gates[:, t].split(H, dim=-1)
        tc = torch.tanh(cseq[:, t])
        cprev = cseq[:, t - 1] if t > 0 else torch.zeros_like(dc)
        if mut == "forget_c":
            cprev = cseq[:, t]
        dct = dc + dht * o * (1 - tc * tc)
        dc = dct * f
        z = _bf(torch.cat([dct * g * i * (1 - i), dct * cprev * f * (1 - f), dct * i * (1 - g * g),
                           dht * tc * o * (1 - o)], -1))
        dz[:, t] = z
        dh_rec = z @ Ur.t()
    dx = dz @ Wr.t()
    hprev = torch.cat([hseq.new_zeros(M, 1, H), hseq[:, :-1]], 1)
    if mut == "du_h":
        hprev = hseq
    dzw = dz
    if mut == "wg_final":
        dzw = dz.clone()
        dzw[:, :(1 if T % 2 else 2)] = 0
    elif mut == "tile":
        dzw = dz.clone()
        dzw[M - 16:] = 0
    elif mut == "group":
        dzw = dz.clone()
        tile = torch.arange(M) // 16
        dzw[(tile // 16) % NG == NG - 1] = 0
    dW = torch.einsum("mtd,mtg->dg", xr, dzw)
    dU = torch.einsum("mth,mtg->hg", _bf(hprev), dzw)
    db = dzw.sum((0, 1))
    return hseq, dx, dW, dU, db


def _tm(t):
    return t.transpose(0, 1).contiguous()


def _pool64(hB, P):
    """Float64 MaxPooling1D(P) of a time-major [T, Mp, H] tensor: (pooled, argmax, gap between the two
    largest candidates; inf at P = 1)."""
    T = hB.shape[0]
    win = hB[:(T // P) * P].reshape(T // P, P, *hB.shape[1:])
    top = win.topk(min(2, P), dim=1).values
    gap = top[:, 0] - top[:, 1] if P > 1 else torch.full_like(top[:, 0], float("inf"))
    return win.max(1).values, win.argmax(1), gap


def tm_reference(c, d, mut=None):
    """The case's quantities (time-major, float64) from :func:`layer_ref`; ``mut`` switches one named
    mutant in (both layers of a pair)."""
    x = _tm(d["x"][:, :, :c.Dw].double())
    f64 = {k: v.double() for k, v in d.items() if v.dtype == torch.float32}
    dh = dh_full(c, d, mut)
    lm = mut if mut in ("forget_c", "du_h", "wg_final", "tile", "group") else None
    sv, NG = saved_mode(c), n_groups(c)
    if c.kind == "single":
        h, dx, dW, dU, db = layer_ref(x, f64["W"], f64["U"], f64["b"], dh, sv, lm, NG)
        return dict(h=_tm(h), dx=_tm(dx), dW=dW, dU=dU, db=db)
    hA = layer_ref(x, f64["W"], f64["U"], f64["b"], torch.zeros(x.shape[0], c.T, c.H, dtype=torch.float64), sv)[0]
    hB, dhA, dWB, dUB, dbB = layer_ref(hA, f64["WB"], f64["UB"], f64["bB"], dh, sv, lm, NG)
    _, dx, dWA, dUA, dbA = layer_ref(x, f64["W"], f64["U"], f64["b"], dhA, sv, lm, NG)
    return dict(hA=_tm(hA), hB=_tm(hB), dx=_tm(dx), dWA=dWA, dUA=dUA, dbA=dbA, dWB=dWB, dUB=dUB, dbB=dbB)


def oracle_reference(c, d):
    """The same quantities from KernelLSTM (rounding on) and its own backward: what the GPU is held to."""
    from gnnqc.ops.lstm_ref import KernelLSTM
    names = ("W", "U", "b") + (("WB", "UB", "bB") if c.kind == "pair" else ())
    x = _tm(d["x"][:, :, :c.Dw].double()).requires_grad_(True)
    ps = [d[n].double().requires_grad_(True) for n in names]
    sv = saved_mode(c)
    hA = KernelLSTM.apply(x, ps[0], ps[1], ps[2], True, True, sv)
    out = hA if c.kind == "single" else KernelLSTM.apply(hA, ps[3], ps[4], ps[5], True, True, sv)
    r = {}
    if c.bwd:
        gr = torch.autograd.grad((out * dh_full(c, d)).sum(), [x] + ps)
        r["dx"] = _tm(gr[0])
        if c.kind == "single":
            r["dW"], r["dU"], r["db"] = gr[1:]
        else:
            r["dWA"], r["dUA"], r["dbA"], r["dWB"], r["dUB"], r["dbB"] = gr[1:]
    if c.kind == "single":
        r["h"] = _tm(hA.detach())
    else:
        r["hA"], r["hB"] = _tm(hA.detach()), _tm(out.detach())
        if c.mode == "rg":                              # the pair saves (and returns) hA in bf16
            r["hA"] = _bf(r["hA"])
    return r


_REFERENCES = {}


def case_reference(c):
    """(inputs, oracle reference) of a case, computed once per process and shared (never modified)."""
    if c.name not in _REFERENCES:
        d = tm_inputs(c)
        _REFERENCES[c.name] = (d, oracle_reference(c, d))
    return _REFERENCES[c.name]


def quantity_kind(q):
    """'hA' -> 'h', 'dWB' -> 'dW', 'pooled' -> 'h'."""
    return "h" if q in ("pooled",) else (q[:-1] if q[-1] in "AB" else q)


def bound_of(c, q):
    return min(OUT_BOUND if quantity_kind(q) == "h" else GRAD_BOUND, BOUNDS[c.family])


def rel_err(a, r):
    """Relative Frobenius distance and the largest element error over the largest reference element."""
    n = r.norm().item()
    return ((a - r).norm().item() / n if n > 0 else float("nan"),
            (a - r).abs().max().item() / r.abs().max().item() if n > 0 else float("nan"))


def compared_quantities(c):
    """What the GPU test compares for this case (frozen weights: no dW / dU / db; need_dx false: no dx)."""
    qs = ["h"] if c.kind == "single" else ["hA", "hB"]
    if c.bwd:
        if c.need_dx:
            qs.append("dx")
        if c.wg:
            qs += ["dW", "dU", "db"] if c.kind == "single" else ["dWA", "dUA", "dbA", "dWB", "dUB", "dbB"]
    return qs


# ------------------------------------------------------------------ device runs
def place_x(x, off, dev):
    """x on the device as a contiguous view of a larger flat buffer, ``off`` floats past its base."""
    if off == 0:
        return x.to(dev)
    buf = torch.zeros(x.numel() + 8, device=dev)
    v = buf[off:off + x.numel()].view(x.shape)
    v.copy_(x)
    return v


def _set_env(monkeypatch, c):
    monkeypatch.setenv("GNNQC_TM_FUSED_WGRAD_MIN_TILES", str(c.min_tiles))
    monkeypatch.setenv("GNNQC_TM_FUSED_WGRAD", "1" if c.fused else "0")
    monkeypatch.setenv("GNNQC_TM_RECDX", "1" if c.recdx else "0")


def _sinks(c, d, names, dev):
    if not c.wg:
        return [torch.zeros(0, device=dev)] * 3
    return [d["pre_" + n].to(dev) for n in names]


def run_case(c, d, dev):
    """The case's ops on the device: quantity name -> float64 CPU tensor (pre-fills subtracted), plus
    'pidx' for a pooled pair."""
    from gnnqc.utils.native import hip_ops
    ops = hip_ops()
    x = place_x(d["x"], c.off, dev)
    assert x.is_contiguous() and x.data_ptr() % 16 == (4 * c.off) % 16
    t = {k: v.to(dev) for k, v in d.items() if k != "x"}
    train, sg = c.mode != "eval", c.mode != "rg"
    got = {}
    pidx = t["pidx"] if c.P else None
    if c.kind == "single":
        h, g, cs = ops.lstm_tm_fwd(x, t["W"], t["U"], t["b"], train, sg)
        assert tuple(h.shape) == (c.T, 16 * c.tiles, c.H) and (g.numel() > 0) == (train and sg)
        got["h"] = h
        if c.mode == "rg":      # the recompute-gates forward instance computes the same h
            h_sg = ops.lstm_tm_fwd(x, t["W"], t["U"], t["b"], True, True)[0]
            assert (h - h_sg).abs().max().item() <= 1e-5
        if c.bwd:
            sk = _sinks(c, d, ("W", "U", "b"), dev)
            dx = ops.lstm_tm_bwd(t["dh"], g, cs, x, h, t["W"], t["U"], t["b"], *sk, c.need_dx, pidx, c.P)
            got.update(dx=dx, dW=sk[0], dU=sk[1], db=sk[2])
    else:
        hA, gA, cA, hB, gB, cB, pooled, pi = ops.lstm_tm2_fwd(x, t["W"], t["U"], t["b"], t["WB"], t["UB"], t["bB"],
                                                              train, sg, c.pool)
        assert hA.dtype == (torch.bfloat16 if c.mode == "rg" else torch.float32)
        got.update(hA=hA.float(), hB=hB)
        if c.pool:
            got.update(pooled=pooled, pidx=pi)
        if c.bwd:
            sB, sA = _sinks(c, d, ("WB", "UB", "bB"), dev), _sinks(c, d, ("W", "U", "b"), dev)
            dhA = ops.lstm_tm_bwd(t["dh"], gB, cB, hA, hB, t["WB"], t["UB"], t["bB"], *sB, True, None, 0)      # XB
            dx = ops.lstm_tm_bwd(dhA, gA, cA, x, hA, t["W"], t["U"], t["b"], *sA, c.need_dx, None, 0)          # HB
            got.update(dx=dx, dWA=sA[0], dUA=sA[1], dbA=sA[2], dWB=sB[0], dUB=sB[1], dbB=sB[2])
    torch.cuda.synchronize()
    out = {}
    for q, v in got.items():
        if v.numel() == 0:
            continue
        out[q] = v.cpu() if q == "pidx" else v.double().cpu()
        pre = {"dW": "W", "dU": "U", "db": "b", "dWA": "W", "dUA": "U", "dbA": "b", "dWB": "WB", "dUB": "UB",
               "dbB": "bB"}.get(q)
        if pre is not None:
            out[q] = out[q] - d["pre_" + pre].double().view(out[q].shape)
    return out


@pytest.mark.parametrize("case", TM_CASES, ids=[c.name for c in TM_CASES])
def test_lstm_tm_case_matches_oracle(cuda_device, monkeypatch, case):
    """One case of the table: every compared quantity within its family's bound of the KernelLSTM
    oracle in relative Frobenius norm; the exact checks of the module docstring."""
    c = case
    _set_env(monkeypatch, c)
    d, r = case_reference(c)
    got = run_case(c, d, cuda_device)
    qs = compared_quantities(c)
    assert set(qs) <= set(got), (c.name, sorted(got))
    M, Dw = c.M, c.Dw
    if "dx" in qs:
        assert tuple(got["dx"].shape) == (c.T, 16 * c.tiles, c.Din)
        assert torch.count_nonzero(got["dx"][:, M:]) == 0, f"{c.name}: dx of pad rows"
        assert torch.count_nonzero(got["dx"][:, :, Dw:]) == 0, f"{c.name}: dx of channels >= Dw"
        got["dx"] = got["dx"][:, :, :Dw]
    failures = []
    for q in qs:
        ref = r[q]
        a = got[q].view(ref.shape)
        if ref.norm().item() == 0:                     # (dU at T = 1: h_{-1} = 0)
            assert torch.count_nonzero(a) == 0, f"{c.name}: {q} must be exactly zero"
            print(f"TMERR {c.name} {q} zero zero")
            continue
        e, m = rel_err(a, ref)
        print(f"TMERR {c.name} {q} {e:.3e} {m:.3e}")
        if not e <= bound_of(c, q):
            failures.append(f"{q}: {e:.3e} > {bound_of(c, q):.0e}")
    if c.pool:
        pooled, arg, gap = _pool64(r["hB"], c.pool)
        e, m = rel_err(got["pooled"], pooled)
        print(f"TMERR {c.name} pooled {e:.3e} {m:.3e}")
        if not e <= bound_of(c, "pooled"):
            failures.append(f"pooled: {e:.3e}")
        clear = gap > bound_of(c, "pooled") * r["hB"].abs().max()
        assert clear.double().mean() > 0.5
        if not torch.equal(got["pidx"].long()[clear], arg[clear]):
            failures.append("pidx differs from the float64 argmax where the top two candidates are clearly apart")
    assert not failures, f"{c.name}: " + "; ".join(failures)


def test_lstm_tm_refuses_unsupported_arguments(cuda_device):
    """Argument combinations the host refuses (a check before any launch)."""
    from gnnqc.utils.native import hip_ops
    ops, dev = hip_ops(), cuda_device
    gen = torch.Generator().manual_seed(5)
    T, Mp, H = 6, 16, 16
    e = torch.zeros(0, device=dev)

    def setup(Din, Hh=H, sg=True):
        x = torch.randn(T, Mp, Din, generator=gen).to(dev)
        W, U, b = (p.to(dev) for p in _params(Din, Hh, gen))
        return (x, W, U, b) + tuple(ops.lstm_tm_fwd(x, W, U, b, True, sg))

    x, W, U, b, h, g, cs = setup(20)
    pidx = torch.zeros(T // 3, Mp, H, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="pool size|dh shape|pidx"):      # un-pooling a 2-D (last-state) dh
        ops.lstm_tm_bwd(torch.zeros(Mp, H, device=dev), g, cs, x, h, W, U, b, e, e, e, True,
                        torch.zeros(Mp, H, dtype=torch.uint8, device=dev), 3)
    x18, W18, U18, b18, h18, g18, c18 = setup(18)
    with pytest.raises(RuntimeError, match="un-pooling takes"):             # frozen path, 8-byte granules
        ops.lstm_tm_bwd(torch.zeros(T // 3, Mp, H, device=dev), g18, c18, x18, h18, W18, U18, b18, e, e, e, True,
                        pidx, 3)
    with pytest.raises(RuntimeError, match="bf16 x or h"):                  # bf16 x with saved gates
        ops.lstm_tm_bwd(torch.zeros(T, Mp, H, device=dev), g, cs, x.to(torch.bfloat16), h, W, U, b, e, e, e, True,
                        None, 0)
    x64 = torch.randn(T, Mp, 20, generator=gen).to(dev)
    W64, U64, b64 = (p.to(dev) for p in _params(20, 64, gen))
    with pytest.raises(RuntimeError, match="recomputed gates"):             # store_gates = false at H = 64
        ops.lstm_tm_fwd(x64, W64, U64, b64, True, False)
    torch.cuda.synchronize()
