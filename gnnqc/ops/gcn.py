"""GeneralConv (+ BatchNorm + PReLU) with fused node pooling.

Semantics of spektral 1.3 ``GeneralConv(channels, batch_norm=True, dropout,
aggregate, activation='prelu')`` as built at ``libs/create_model.py:184-189``:
``x@W+b -> BatchNorm(momentum .99, eps 1e-3) -> Dropout -> PReLU -> aggregate
messages x_j over edges (i <- j)``, followed for CML by ``timeseries_pooling``
(mean/sum/max over the nodes of a sample, or ``selection`` of the flagged node,
``:8-41``).

Graphs here are dense per-sample adjacencies ``[B, N, N]`` shared by all time
steps, with a node mask for padding. BatchNorm statistics run over the valid
node rows only (exactly the rows the reference's ragged batch contains).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F


def normalized_adjacency(adj: torch.Tensor, aggregate: str = "mean") -> torch.Tensor:
    """Row-normalised (mean) or raw (sum) aggregation matrix. Row i aggregates j."""
    if aggregate == "mean":
        deg = adj.sum(-1, keepdim=True)
        return adj / deg.clamp(min=1.0)
    if aggregate == "sum":
        return adj
    raise ValueError(f"linear aggregation expected, got {aggregate}")


def node_pool_weights(adj: torch.Tensor, mask: torch.Tensor, anom_pos: torch.Tensor | None,
                      aggregate: str = "mean", pooling: str = "mean") -> torch.Tensor:
    """w[b, j] such that pool(aggregate(a))[b, t] = sum_j w[b, j] a[b, t, j]."""
    A = normalized_adjacency(adj, aggregate)
    if pooling == "mean":
        p = mask / mask.sum(-1, keepdim=True).clamp(min=1.0)
    elif pooling == "sum":
        p = mask
    elif pooling == "selection":
        p = F.one_hot(anom_pos.clamp(min=0), adj.shape[-1]).to(adj.dtype)
    else:
        raise ValueError(f"linear pooling expected, got {pooling}")
    return torch.bmm(p.unsqueeze(1), A).squeeze(1).contiguous()


def masked_batchnorm(z: torch.Tensor, mask: torch.Tensor, gamma, beta, running_mean, running_var,
                     training: bool, momentum: float = 0.99, eps: float = 1e-3) -> torch.Tensor:
    """BatchNorm over the last axis using only rows where ``mask`` (broadcast) is 1.

    ``z``: [B, T, N, F]; ``mask``: [B, N]. Keras semantics: biased batch variance,
    ``moving = moving * momentum + batch * (1 - momentum)``.
    """
    m = mask[:, None, :, None].to(z.dtype)
    if training:
        cnt = (mask.sum() * z.shape[1]).clamp(min=1.0)
        mu = (z * m).sum(dim=(0, 1, 2)) / cnt
        var = (((z - mu) ** 2) * m).sum(dim=(0, 1, 2)) / cnt
        with torch.no_grad():
            running_mean.mul_(momentum).add_(mu.detach() * (1 - momentum))
            running_var.mul_(momentum).add_(var.detach() * (1 - momentum))
    else:
        mu, var = running_mean, running_var
    return (z - mu) * torch.rsqrt(var + eps) * gamma + beta


def prelu(x, alpha):
    return torch.where(x > 0, x, alpha * x)


def general_conv_eager(x, adj, mask, W, b, gamma, beta, running_mean, running_var, alpha, training,
                       aggregate="mean", dropout=0.0, momentum=0.99, eps=1e-3, use_batch_norm=True,
                       activation="prelu"):
    """Per-node GeneralConv output [B, T, N, F] (reference oracle, any aggregation)."""
    z = torch.matmul(x, W) + b
    if use_batch_norm:
        z = masked_batchnorm(z, mask, gamma, beta, running_mean, running_var, training, momentum, eps)
    if dropout and training:
        z = F.dropout(z, dropout, training=True)
    if activation == "prelu":
        a = prelu(z, alpha)
    elif activation in (None, "linear"):
        a = z
    else:
        a = getattr(torch, activation)(z) if hasattr(torch, activation) else getattr(F, activation)(z)
    a = a * mask[:, None, :, None]
    if aggregate == "max":
        # max over neighbours j of a[j] (messages only along edges)
        big = torch.finfo(a.dtype).max
        msg = a.unsqueeze(2).expand(-1, -1, a.shape[2], -1, -1)          # [B,T,N(i),N(j),F]
        edge = adj[:, None, :, :, None] > 0
        out = torch.where(edge, msg, torch.full_like(msg, -big)).amax(3)
        out = torch.where(edge.any(3), out, torch.zeros_like(out))
        return out * mask[:, None, :, None]
    A = normalized_adjacency(adj, aggregate)
    return torch.einsum("bij,btjf->btif", A, a)


class _HipGCNPool(torch.autograd.Function):
    """Fused stats -> affine/BN/PReLU -> weighted node sum -> concat (HIP).

    Launches per training step: gcn_prep (pool weights + batch moments + BN prep) and
    gcn_pool_fwd forward; gcn_pool_bwd and gcn_bwd_finalize (+ gcn_pool_bwd_input when dx is
    needed) backward. Weight gradients go straight into the optimiser's flat buffer when
    direct accumulation is on (see ``gnnqc.ops.wgrad.direct_grad_accumulation``)."""

    @staticmethod
    def forward(ctx, x, adj, mask, anom, anom_pos, agg_mean: bool, pool: int, W, b, gamma, beta, alpha,
                running_mean, running_var, training: bool, momentum: float, eps: float, Mp: int = 0, Cp: int = 0):
        from ..utils.native import hip_ops
        ops = hip_ops()
        w, S, st = ops.gcn_prep(x, adj, mask, anom_pos, bool(agg_mean), int(pool), W.contiguous(), b.contiguous(),
                                gamma.contiguous(), beta.contiguous(), running_mean, running_var, bool(training),
                                float(momentum), float(eps))
        anom_t = anom.contiguous() if anom is not None else x.new_zeros(0)
        out = ops.gcn_pool_fwd(x, w, anom_t, W.contiguous(), b.contiguous(), st[2], st[3], alpha.contiguous(),
                               int(Mp), int(Cp))
        ctx.tm = Mp > 0
        ctx.training = training
        ctx.ca = 0 if anom is None else anom.shape[-1]
        ctx.has_anom = anom is not None
        ctx.params = (W, b, gamma, beta, alpha)
        ctx.save_for_backward(x, w, mask, W, b, alpha, st, S)
        return out

    @staticmethod
    def backward(ctx, dout):
        from ..utils.native import hip_ops
        from .wgrad import _grad_sink
        ops = hip_ops()
        x, w, mask, W, b, alpha, st, S = ctx.saved_tensors
        dout = dout.contiguous()
        need = ctx.needs_input_grad
        need_w = any(need[7:12])
        empty = x.new_zeros(0)
        acc = empty
        if ctx.training or need_w:
            acc = ops.gcn_pool_bwd(x, w, dout, W.contiguous(), b.contiguous(), st[2], st[3], alpha.contiguous(),
                                   ctx.ca, ctx.tm)
        sinks = [(_grad_sink(p) if n else (empty, True)) for p, n in zip(ctx.params, need[7:12])]
        coef = ops.gcn_bwd_finalize(acc, S, W.contiguous(), b.contiguous(), st, bool(ctx.training),
                                    *[s[0] for s in sinks])
        dx = None
        if need[0]:
            dx = ops.gcn_pool_bwd_input(x, w, mask, dout, W.contiguous(), b.contiguous(), st[2], st[3],
                                        alpha.contiguous(), coef, ctx.ca, ctx.tm)
        danom = None
        if ctx.has_anom and need[3]:
            danom = dout[:, : x.shape[0], : ctx.ca].transpose(0, 1) if ctx.tm else dout[..., : ctx.ca]
        grads = [None if direct or not n else buf for (buf, direct), n in zip(sinks, need[7:12])]
        return (dx, None, None, danom, None, None, None, *grads, None, None, None, None, None, None, None)


def gcn_pool_hip_ok(x, W, aggregate: str, pooling: str, dropout: float, training: bool) -> bool:
    from . import use_hip
    linear = aggregate in ("mean", "sum") and pooling in ("mean", "sum", "selection")
    # (1..4 input channels: what gcn_prep instantiates, gcn_glue.hip GQ_GLUE_CIN_DISPATCH)
    return bool(use_hip(x) and linear and not (dropout and training) and x.shape[-1] <= 4
                and W.shape[1] in (8, 16, 32))


def gcn_pool(x, adj, mask, anom, anom_pos, W, b, gamma, beta, alpha, running_mean, running_var,
             training: bool, aggregate: str = "mean", pooling: str = "mean", momentum: float = 0.99,
             eps: float = 1e-3, dropout: float = 0.0, time_major: bool = False):
    """GeneralConv + node pooling + concat -> LSTM input ``[B, T, Ca + F]``.

    Uses the fused HIP kernels for linear aggregation/pooling on GPU; otherwise the
    eager per-node path. ``time_major=True`` (HIP path only) returns ``(h [T, Mp, Cp], B)``:
    the time-major, row- and channel-padded input of
    :meth:`gnnqc.models.timelayer.TimeLayer.forward_time_major`, written by the kernel itself.
    """
    if gcn_pool_hip_ok(x, W, aggregate, pooling, dropout, training):
        ap = anom_pos.long().contiguous() if (pooling == "selection" and anom_pos is not None) else x.new_zeros(0)
        Mp = Cp = 0
        if time_major:
            B = x.shape[0]
            Mp = (B + 15) // 16 * 16
            Cp = W.shape[1] + (anom.shape[-1] if anom is not None else 0)
            Cp += (-Cp) % 4
        out = _HipGCNPool.apply(x.contiguous(), adj.float().contiguous(), mask.contiguous().float(), anom, ap,
                                aggregate == "mean", {"mean": 0, "sum": 1, "selection": 2}[pooling], W, b, gamma,
                                beta, alpha, running_mean, running_var, bool(training), float(momentum), float(eps),
                                Mp, Cp)
        return (out, x.shape[0]) if time_major else out
    if time_major:
        raise ValueError("gcn_pool(time_major=True) needs the HIP path")
    h = general_conv_eager(x, adj, mask, W, b, gamma, beta, running_mean, running_var, alpha, training,
                           aggregate, dropout, momentum, eps)
    pooled = pool_nodes(h, mask, anom_pos, pooling)
    return pooled if anom is None else torch.cat([anom, pooled], dim=-1)


class _HipGCNNodeTM(torch.autograd.Function):
    """Per-node GeneralConv -> time-major LSTM input ``[T, Mp, Cp]`` (``gcn_node.hip``).

    Forward: gcn_stats, gcn_bn_prep, gcn_node_fwd; backward: gcn_node_bwd,
    gcn_bwd_finalize (+ gcn_node_bwd_input when dx is needed, e.g. integrated gradients)."""

    @staticmethod
    def forward(ctx, x, bits, bitsT, rs, mask, W, b, gamma, beta, alpha, running_mean, running_var,
                training: bool, momentum: float, eps: float, Mp: int, Cp: int):
        from ..utils.native import hip_ops
        ops = hip_ops()
        S = ops.gcn_stats(x, mask) if training else x.new_zeros(0, dtype=torch.float64)
        st = ops.gcn_bn_prep(S, W.contiguous(), b.contiguous(), gamma.contiguous(), beta.contiguous(),
                             running_mean, running_var, bool(training), float(momentum), float(eps))
        out = ops.gcn_node_fwd(x, bits, rs, mask, W.contiguous(), b.contiguous(), st[2], st[3], alpha.contiguous(),
                               int(Mp), int(Cp))
        ctx.training = training
        ctx.params = (W, b, gamma, beta, alpha)
        ctx.save_for_backward(x, bitsT, rs, mask, W, b, alpha, st, S)
        return out

    @staticmethod
    def backward(ctx, dout):
        from ..utils.native import hip_ops
        from .wgrad import _grad_sink
        ops = hip_ops()
        x, bitsT, rs, mask, W, b, alpha, st, S = ctx.saved_tensors
        dout = dout.contiguous()
        need = ctx.needs_input_grad
        empty = x.new_zeros(0)
        acc = empty
        if ctx.training or any(need[5:10]):
            acc = ops.gcn_node_bwd(x, bitsT, rs, mask, dout, W.contiguous(), b.contiguous(), st[2], st[3],
                                   alpha.contiguous())
        sinks = [(_grad_sink(p) if n else (empty, True)) for p, n in zip(ctx.params, need[5:10])]
        coef = ops.gcn_bwd_finalize(acc, S, W.contiguous(), b.contiguous(), st, bool(ctx.training),
                                    *[s[0] for s in sinks])
        dx = None
        if need[0]:
            dx = ops.gcn_node_bwd_input(x, bitsT, rs, mask, dout, W.contiguous(), b.contiguous(), st[2], st[3],
                                        alpha.contiguous(), coef)
        grads = [None if direct or not n else buf for (buf, direct), n in zip(sinks, need[5:10])]
        return (dx, None, None, None, None, *grads, None, None, None, None, None, None, None)


def gcn_node_tm_ok(x: torch.Tensor, W: torch.Tensor, aggregate: str, dropout: float, training: bool) -> bool:
    """Whether :func:`gcn_node_tm` runs the HIP kernels for this input."""
    from . import use_hip
    F_ = W.shape[1]
    N = x.shape[2]
    lds = (N * ((N + 31) // 32) + 3) // 4 * 16 + N * F_ * 4 + N * 8     # gcn_node.hip node_smem_bytes
    return (use_hip(x) and aggregate in ("mean", "sum") and not (dropout and training) and x.shape[-1] <= 4
            and F_ <= 64 and 64 % F_ == 0 and lds <= 150 * 1024)


def gcn_node_tm(x, adj, mask, W, b, gamma, beta, alpha, running_mean, running_var, training: bool,
                aggregate: str = "mean", momentum: float = 0.99, eps: float = 1e-3, cpad_to: int = 4):
    """SoilNet GeneralConv + ``Concatenate([gcn, x])`` + ``graph_reshape`` as ONE time-major tensor.

    Returns ``(h [T, Mp, Cp], M)`` with row ``m = b*N + i`` (the reference's
    per-node sequence order), channels ``[F gcn | Cin raw | 0 pad]`` (Cp a multiple
    of ``cpad_to``) and zero rows past ``M = B*N`` - the input layout of
    :meth:`gnnqc.models.timelayer.TimeLayer.forward_time_major`.
    """
    from ..utils.native import hip_ops
    B, T, N, Cin = x.shape
    M = B * N
    Mp = (M + 15) // 16 * 16
    Cp = W.shape[1] + Cin
    Cp += (-Cp) % cpad_to
    bits, bitsT, rs = hip_ops().gcn_adj_bits(adj.float().contiguous(), aggregate == "mean")
    h = _HipGCNNodeTM.apply(x.float().contiguous(), bits, bitsT, rs, mask.float().contiguous(), W, b, gamma, beta,
                            alpha, running_mean, running_var, bool(training), float(momentum), float(eps), Mp, Cp)
    return h, M


def gcn_node_tm_eager(x, adj, mask, W, b, gamma, beta, alpha, running_mean, running_var, training: bool,
                      aggregate: str = "mean", momentum: float = 0.99, eps: float = 1e-3, cpad_to: int = 4):
    """Eager oracle of :func:`gcn_node_tm` (same output layout)."""
    B, T, N, Cin = x.shape
    M = B * N
    Mp = (M + 15) // 16 * 16
    h = general_conv_eager(x, adj, mask, W, b, gamma, beta, running_mean, running_var, alpha, training, aggregate,
                           0.0, momentum, eps)
    seq = torch.cat([h, x], -1).permute(1, 0, 2, 3).reshape(T, M, -1)
    C = seq.shape[-1]
    return F.pad(seq, (0, (-C) % cpad_to, 0, Mp - M)), M


class _HipStoreGCN(torch.autograd.Function):
    """Window gather + GeneralConv + BatchNorm + PReLU + node pooling + concat in ONE launch,
    straight from the resident window store (``gcn_fused.hip``): ``(h [T, Mp, Cp], y, y_mask,
    wid)``. Backward: ONE launch adding the parameter gradients with float atomics (training mode
    only; not bitwise reproducible, so the deterministic mode keeps :class:`_HipGCNPool`). In the
    CML configuration the forward also emits the backward's coefficients and the backward is the
    dot product of dh with them (``gcn_coef_bwd``), usually run inside the batched weight-gradient
    launch."""

    @staticmethod
    def forward(ctx, data, ids, W, b, gamma, beta, alpha, running_mean, running_var, training: bool,
                momentum: float, eps: float, Mp: int, Cp: int, coef: bool = False, defer: bool = False):
        from ..utils.native import hip_ops
        wids, table, cursor = ids
        h, S, st, y, ym, wid, cf = hip_ops().gcn_fused_fwd(
            *data["fwd"], wids, table, cursor, *data["dims"], W.contiguous(), b.contiguous(), gamma.contiguous(),
            beta.contiguous(), alpha.contiguous(), running_mean, running_var, bool(training), float(momentum),
            float(eps), int(Mp), int(Cp), coef, defer)
        ctx.data, ctx.ids, ctx.training = data, ids, bool(training)
        ctx.params = (W, b, gamma, beta, alpha)
        ctx.save_for_backward(W, b, alpha, S, st, cf)
        ctx.mark_non_differentiable(y, ym, wid)
        ctx.set_materialize_grads(False)
        return h, y, ym, wid

    @staticmethod
    def backward(ctx, dh, _dy, _dym, _dwid):
        from ..utils.native import hip_ops
        from .wgrad import _grad_sink
        W, b, alpha, S, st, cf = ctx.saved_tensors
        need = ctx.needs_input_grad[2:7]
        if dh is None or not any(need):
            return (None,) * 15
        if not ctx.training:
            raise RuntimeError("gcn_fused backward: parameter gradients in eval mode take the generic path")
        sinks = [(_grad_sink(p) if n else (torch.zeros_like(p), False)) for p, n in zip(ctx.params, need)]
        from .wgrad import defer_to_grads_launch
        direct = all(direct for (_, direct), n in zip(sinks, need) if n)
        if cf.numel() > 0:
            # coefficient form: dh x coef, deferred onto the batched LSTM weight-gradient launch when
            # every gradient goes straight into .grad
            ca = int(ctx.data["ca"])
            # (the coefficients are normally written by spare workgroups of the chain forward launch;
            # if no chain launch took the job, run it now)
            hip_ops().gcn_coef_flush(cf)
            jt = [dh.contiguous(), cf, S, st, W.contiguous(), b.contiguous(), sinks[0][0], sinks[2][0], sinks[3][0],
                  sinks[4][0]]
            if not (direct and defer_to_grads_launch((jt, [ca]))):
                hip_ops().gcn_coef_bwd(jt[0], ca, *jt[1:])
            grads = [None if direct or not n else buf for (buf, direct), n in zip(sinks, need)]
            return (None, None, *grads, None, None, None, None, None, None, None, None, None)
        wids, table, cursor = ctx.ids
        args = (dh.contiguous(), int(ctx.data["ca"]), *ctx.data["bwd"], wids, table, cursor, *ctx.data["dims"], S, st,
                W.contiguous(), b.contiguous(), alpha.contiguous(), sinks[0][0], sinks[2][0], sinks[3][0], sinks[4][0])
        # (deferred onto the batched LSTM weight-gradient launch when every gradient goes straight
        # into .grad and the configuration is the one that launch instantiates)
        if not (direct and tuple(W.shape) == (2, 16) and defer_to_grads_launch(_gcn_job_lists(args))):
            hip_ops().gcn_fused_bwd(*args)
        grads = [None if direct or not n else buf for (buf, direct), n in zip(sinks, need)]
        return (None, None, *grads, None, None, None, None, None, None, None, None, None)


def _gcn_job_lists(args):
    """gcn_fused_bwd's arguments as lstm_grads_multi's (gcn_t, gcn_i) job lists."""
    (dh, c_off, series, shift, scale, wg, wc, wv, gap, pw, wids, table, cursor, tb, seq_len, time_norm, S, st, W, b,
     alpha, dW, dgamma, dbeta, dalpha) = args
    cur = cursor if cursor is not None else series.new_zeros(0, dtype=torch.long)
    return ([dh, series, shift, scale, wg, wc, wv, gap, pw, wids, table, cur, S, st, W, b, alpha, dW, dgamma, dbeta,
             dalpha], [int(c_off), int(tb), int(seq_len), int(bool(time_norm))])


def store_gcn_ok(store, layer, training: bool, pooling: str) -> bool:
    """Whether :func:`gcn_pool_from_store` runs for this store / GeneralConv configuration."""
    from . import deterministic, use_hip
    if not (use_hip(store.series) and getattr(store, "per_sensor", False) and store.series.dtype == torch.float32
            and store.win_label.dim() == 1):
        return False
    if training and deterministic():
        return False
    W = layer.kernel
    C, N = store.n_feat, store.n_nodes
    return (layer.aggregate in ("mean", "sum") and pooling in ("mean", "sum", "selection")
            and not (layer.dropout and training) and W.shape[0] == C and 1 <= C <= 4 and N * C <= 128
            and W.shape[1] in (8, 16, 32) and store.seq_len >= 1)


def gcn_pool_from_store(store, ids, layer, training: bool, pooling: str = "mean", defer: bool = False):
    """The CML GCN front end of a training / evaluation step straight from ``store``:
    ``(h [T, Mp, Cp], B, y [B], y_mask [B], wid [B])`` with ``h`` the time-major LSTM input
    (``[flagged series | pooled GCN | 0 pad]``) of :meth:`gnnqc.models.timelayer.TimeLayer.forward_time_major`.
    ``ids``: window ids [B] (-1 = padding) or a :class:`gnnqc.data.store.CursorIds`.

    ``defer`` (training with the coefficient-form backward only): no launch here; the next headed
    LSTM chain forward launch whose input is ``h`` runs this forward as producer workgroups and its
    first stage streams their output (``gcn_fused.h`` ``gcn_prod_body``). Every other consumer of the
    outputs must call ``hip_ops().gcn_prod_flush(h)`` first (the backward does)."""
    from ..data.store import CursorIds
    agg_mean = layer.aggregate == "mean"
    pool = {"mean": 0, "sum": 1, "selection": 2}[pooling]
    data = store.gcn_fused_data(agg_mean, pool)
    e = store.series.new_zeros(0, dtype=torch.long)
    if isinstance(ids, CursorIds):
        idt = (e, ids.table, ids.cursor)
        B = int(ids.table.shape[1])
    else:
        idt = (ids.to(store.device).long().contiguous(), e, None)
        B = int(idt[0].shape[0])
    F_ = layer.kernel.shape[1]
    C = store.n_feat
    Mp = (B + 15) // 16 * 16
    Cp = C + F_
    Cp += (-Cp) % 4
    # training with gradients: the forward also writes the backward's per-(t, sample, feature)
    # coefficients, so the backward is a streaming dot product against dh (gcn_coef_bwd). (Decided
    # here: inside an autograd Function's forward grad mode is always off.)
    import os
    coef = (bool(training) and torch.is_grad_enabled() and tuple(layer.kernel.shape) == (2, 16)
            and any(p.requires_grad for p in (layer.kernel, layer.bn_gamma, layer.bn_beta, layer.prelu_alpha))
            and os.environ.get("GNNQC_GCN_COEF", "1") == "1")
    # (off by default: measured slower - the producers' id -> window -> series load chain and
    # per-row compute take ~13 us inside the chain launch vs 11.4 us for the forward's own launch;
    # profiles/r5_gcn_producer_ab.txt)
    defer = bool(defer and coef and os.environ.get("GNNQC_GCN_PROD", "0") == "1")
    h, y, ym, wid = _HipStoreGCN.apply(data, idt, layer.kernel, layer.bias, layer.bn_gamma, layer.bn_beta,
                                       layer.prelu_alpha, layer.bn_moving_mean, layer.bn_moving_variance,
                                       bool(training), float(layer.momentum), float(layer.eps), Mp, Cp, coef, defer)
    return h, B, y, ym, wid


def pool_nodes(h: torch.Tensor, mask: torch.Tensor, anom_pos, pooling: str = "mean") -> torch.Tensor:
    """``timeseries_pooling`` over valid nodes: [B,T,N,F] -> [B,T,F]."""
    m = mask[:, None, :, None].to(h.dtype)
    if pooling == "mean":
        return (h * m).sum(2) / m.sum(2).clamp(min=1.0)
    if pooling == "sum":
        return (h * m).sum(2)
    if pooling == "max":
        big = torch.finfo(h.dtype).max
        return torch.where(m > 0, h, torch.full_like(h, -big)).amax(2) * (m.sum(2) > 0)
    if pooling == "selection":
        idx = anom_pos.clamp(min=0)[:, None, None, None].expand(-1, h.shape[1], 1, h.shape[3])
        return h.gather(2, idx).squeeze(2)
    raise ValueError(pooling)


# ---------------------------------------------------------------------------------------------
# GATConv + node pooling + concat (gat.hip). ``layer`` is a :class:`gnnqc.models.graphconv.GATConv`
# (or anything with its attributes); the eager path is the layer itself plus :func:`pool_nodes`.
GAT_MAX_NODES = 64                      # gat.hip: one 64-bit neighbour mask per node
GAT_WIDTHS = ((8, 16, 32), (1, 2))      # gat.hip GQ_GAT_DISPATCH: channels per head, heads
_GAT_ACT = {None: 0, "linear": 0, "prelu": 1, "relu": 2}


def gat_pool_weights(mask: torch.Tensor, anom_pos: torch.Tensor | None, pooling: str = "mean") -> torch.Tensor:
    """p[b, i] such that pool_nodes(h * mask)[b, t] = sum_i p[b, i] h[b, t, i] (mask included)."""
    m = (mask > 0).to(mask.dtype)
    if pooling == "mean":
        return (m / m.sum(-1, keepdim=True).clamp(min=1.0)).contiguous()
    if pooling == "sum":
        return m.contiguous()
    if pooling == "selection":
        return (F.one_hot(anom_pos.clamp(min=0), mask.shape[-1]).to(mask.dtype) * m).contiguous()
    raise ValueError(f"linear pooling expected, got {pooling}")


class _HipGATPool(torch.autograd.Function):
    """Fused edge softmax -> input-space aggregation -> W, bias, activation -> node pool -> concat
    (HIP). Launches: gat_adj_bits and gat_pool_fwd forward; gat_pool_bwd, its fixed-order record
    sum and gat_bwd_finalize (+ gat_pool_bwd_input when dx is needed) backward. Parameter gradients
    go straight into the optimiser's flat buffer under direct accumulation, like
    :class:`_HipGCNPool`'s."""

    @staticmethod
    def forward(ctx, x, adj, mask, anom, pw, W, a_s, a_n, bias, alpha, act: int, Mp: int = 0, Cp: int = 0):
        from ..utils.native import hip_ops
        ops = hip_ops()
        bits = ops.gat_adj_bits(adj, mask)
        empty = x.new_zeros(0)
        anom_t = anom.contiguous() if anom is not None else empty
        al = alpha.contiguous() if alpha is not None else empty
        out = ops.gat_pool_fwd(x, bits, pw, anom_t, W.contiguous(), a_s.contiguous(), a_n.contiguous(),
                               bias.contiguous(), al, int(act), int(Mp), int(Cp))
        ctx.tm = Mp > 0
        ctx.act = int(act)
        ctx.ca = 0 if anom is None else anom.shape[-1]
        ctx.has_anom = anom is not None
        ctx.params = (W, a_s, a_n, bias, alpha)
        ctx.save_for_backward(x, bits, pw, W, a_s, a_n, bias, al)
        return out

    @staticmethod
    def backward(ctx, dout):
        from ..utils.native import hip_ops
        from .wgrad import _grad_sink
        ops = hip_ops()
        x, bits, pw, W, a_s, a_n, bias, al = ctx.saved_tensors
        dout = dout.contiguous()
        need = ctx.needs_input_grad
        need_p = list(need[5:10])
        args = (W.contiguous(), a_s.contiguous(), a_n.contiguous(), bias.contiguous(), al, ctx.act, ctx.ca, ctx.tm)
        empty = x.new_zeros(0)
        grads = [None] * 5
        if any(need_p):
            tot = ops.gat_pool_bwd(x, bits, pw, dout, *args)
            sinks = [(_grad_sink(p) if n else (empty, True)) for p, n in zip(ctx.params, need_p)]
            ops.gat_bwd_finalize(tot, *args[:3], *[s[0] for s in sinks])
            grads = [None if direct or not n else buf for (buf, direct), n in zip(sinks, need_p)]
        dx = ops.gat_pool_bwd_input(x, bits, pw, dout, *args) if need[0] else None
        danom = None
        if ctx.has_anom and need[3]:
            danom = dout[:, : x.shape[0], : ctx.ca].transpose(0, 1) if ctx.tm else dout[..., : ctx.ca]
        return (dx, None, None, danom, None, *grads, None, None, None)


def gat_pool_hip_ok(x: torch.Tensor, layer, pooling: str) -> bool:
    """Whether :func:`gat_pool` runs the HIP kernels: on the GPU, N <= 64, Cin <= 4, linear node
    pooling, no attention dropout while training, concatenated heads of an instantiated width and an
    activation the kernels implement. ``GNNQC_GAT_HIP=0`` keeps the eager layer (A/B runs)."""
    import os

    from . import use_hip
    if os.environ.get("GNNQC_GAT_HIP", "1") != "1" or x.dim() != 4 or x.dtype != torch.float32:
        return False
    W = layer.kernel
    return bool(use_hip(x) and x.shape[2] <= GAT_MAX_NODES and 1 <= x.shape[-1] <= 4 and W.shape[0] == x.shape[-1]
                and pooling in ("mean", "sum", "selection") and not (layer.dropout_rate > 0 and layer.training)
                and layer.concat and W.shape[2] in GAT_WIDTHS[0] and W.shape[1] in GAT_WIDTHS[1]
                and layer.activation in _GAT_ACT)


def _time_major_pad(seq: torch.Tensor):
    """[B, T, C] -> the time-major LSTM input [T, Mp, Cp] (Mp = B rounded up to 16, Cp to 4)."""
    B, T, C = seq.shape
    return F.pad(seq.transpose(0, 1), (0, (-C) % 4, 0, (-B) % 16)).contiguous()


def gat_pool_eager(x, adj, mask, anom, anom_pos, layer, pooling: str = "mean", time_major: bool = False):
    """Eager oracle of :func:`gat_pool` in its output layouts: the layer, :func:`pool_nodes` and
    ``Concatenate([anom, pooled])``."""
    pooled = pool_nodes(layer(x, adj, mask), mask, anom_pos, pooling)
    out = pooled if anom is None else torch.cat([anom, pooled], dim=-1)
    return (_time_major_pad(out), x.shape[0]) if time_major else out


def gat_pool(x, adj, mask, anom, anom_pos, layer, pooling: str = "mean", time_major: bool = False):
    """GATConv + node pooling + concat -> LSTM input ``[B, T, Ca + H*C]``; mirrors :func:`gcn_pool`.

    Uses the fused HIP kernels when :func:`gat_pool_hip_ok`, otherwise the eager layer plus
    :func:`pool_nodes`. ``time_major=True`` (HIP path only) returns ``(h [T, Mp, Cp], B)``, the
    time-major, row- and channel-padded input of
    :meth:`gnnqc.models.timelayer.TimeLayer.forward_time_major`, written by the kernel itself."""
    if gat_pool_hip_ok(x, layer, pooling):
        B = x.shape[0]
        Mp = Cp = 0
        if time_major:
            Mp = (B + 15) // 16 * 16
            Cp = layer.out_features + (anom.shape[-1] if anom is not None else 0)
            Cp += (-Cp) % 4
        mask_f = mask.float().contiguous()
        pw = gat_pool_weights(mask_f, anom_pos.long() if anom_pos is not None else None, pooling)
        out = _HipGATPool.apply(x.contiguous(), adj.float().contiguous(), mask_f, anom, pw, layer.kernel,
                                layer.attn_kernel_self, layer.attn_kernel_neighs, layer.bias, layer.prelu_alpha,
                                _GAT_ACT[layer.activation], Mp, Cp)
        return (out, B) if time_major else out
    if time_major:
        raise ValueError("gat_pool(time_major=True) needs the HIP path")
    return gat_pool_eager(x, adj, mask, anom, anom_pos, layer, pooling)


# ---------------------------------------------------------------------------------------------
# EdgeConv + node pooling + concat (edge.hip). ``layer`` is a :class:`gnnqc.models.graphconv.EdgeConv`
# (or anything with its attributes); the eager path is the layer itself plus :func:`pool_nodes`.
EDGE_MAX_NODES = 64                     # edge.hip: one 64-bit neighbour word per node
EDGE_WIDTHS = (8, 16, 32)               # edge.hip GQ_EDGE_DISPATCH: output channels


class _HipEdgePool(torch.autograd.Function):
    """Fused per-edge ``act(p_i + q_j)`` -> neighbour sum / mean -> node pool -> concat (HIP).
    Launches: edge_adj_bits and edge_pool_fwd forward; edge_pool_bwd, its fixed-order record sum and
    edge_bwd_finalize (+ edge_pool_bwd_input when dx is needed) backward. Parameter gradients go
    straight into the optimiser's flat buffer under direct accumulation, like :class:`_HipGATPool`'s."""

    @staticmethod
    def forward(ctx, x, adj, mask, anom, pw, W, bias, alpha, act: int, mean: bool, Mp: int = 0, Cp: int = 0):
        from ..utils.native import hip_ops
        ops = hip_ops()
        bits = ops.edge_adj_bits(adj, mask)
        empty = x.new_zeros(0)
        anom_t = anom.contiguous() if anom is not None else empty
        al = alpha.contiguous() if alpha is not None else empty
        out = ops.edge_pool_fwd(x, bits, pw, anom_t, W.contiguous(), bias.contiguous(), al, int(act), bool(mean),
                                int(Mp), int(Cp))
        ctx.tm = Mp > 0
        ctx.act, ctx.mean = int(act), bool(mean)
        ctx.ca = 0 if anom is None else anom.shape[-1]
        ctx.has_anom = anom is not None
        ctx.params = (W, bias, alpha)
        ctx.save_for_backward(x, bits, pw, W, bias, al)
        return out

    @staticmethod
    def backward(ctx, dout):
        from ..utils.native import hip_ops
        from .wgrad import _grad_sink
        ops = hip_ops()
        x, bits, pw, W, bias, al = ctx.saved_tensors
        dout = dout.contiguous()
        need = ctx.needs_input_grad
        need_p = list(need[5:8])
        args = (W.contiguous(), bias.contiguous(), al, ctx.act, ctx.mean, ctx.ca, ctx.tm)
        empty = x.new_zeros(0)
        grads = [None] * 3
        if any(need_p):
            tot = ops.edge_pool_bwd(x, bits, pw, dout, *args)
            sinks = [(_grad_sink(p) if n else (empty, True)) for p, n in zip(ctx.params, need_p)]
            ops.edge_bwd_finalize(tot, args[0], *[s[0] for s in sinks])
            grads = [None if direct or not n else buf for (buf, direct), n in zip(sinks, need_p)]
        dx = ops.edge_pool_bwd_input(x, bits, pw, dout, *args) if need[0] else None
        danom = None
        if ctx.has_anom and need[3]:
            danom = dout[:, : x.shape[0], : ctx.ca].transpose(0, 1) if ctx.tm else dout[..., : ctx.ca]
        return (dx, None, None, danom, None, *grads, None, None, None, None)


def edge_pool_hip_ok(x: torch.Tensor, layer, pooling: str) -> bool:
    """Whether :func:`edge_pool` runs the HIP kernels: a float32 GPU tensor ``[B, T, N, Cin]`` with
    N <= 64 and Cin <= 4, no hidden MLP layers (``mlp_hidden: null``), a biased output layer of an
    instantiated width, sum or mean aggregation, linear node pooling and an activation the kernels
    implement. ``GNNQC_EDGE_HIP=0`` keeps the eager layer (A/B runs)."""
    import os

    from . import use_hip
    if os.environ.get("GNNQC_EDGE_HIP", "1") != "1" or x.dim() != 4 or x.dtype != torch.float32:
        return False
    if len(layer.hidden) > 0 or layer.out.bias is None or layer.out.activation not in (None, "linear"):
        return False
    W = layer.out.kernel
    return bool(use_hip(x) and 1 <= x.shape[2] <= EDGE_MAX_NODES and 1 <= x.shape[-1] <= 4
                and W.shape[0] == 2 * x.shape[-1] and W.shape[1] in EDGE_WIDTHS
                and layer.aggregate in ("sum", "mean") and pooling in ("mean", "sum", "selection")
                and layer.activation in _GAT_ACT)


def edge_pool_eager(x, adj, mask, anom, anom_pos, layer, pooling: str = "mean", time_major: bool = False):
    """Eager oracle of :func:`edge_pool` in its output layouts: the layer, :func:`pool_nodes` and
    ``Concatenate([anom, pooled])``."""
    pooled = pool_nodes(layer(x, adj, mask), mask, anom_pos, pooling)
    out = pooled if anom is None else torch.cat([anom, pooled], dim=-1)
    return (_time_major_pad(out), x.shape[0]) if time_major else out


def edge_pool(x, adj, mask, anom, anom_pos, layer, pooling: str = "mean", time_major: bool = False):
    """EdgeConv + node pooling + concat -> LSTM input ``[B, T, Ca + C]``; mirrors :func:`gat_pool`.

    Uses the fused HIP kernels when :func:`edge_pool_hip_ok`, otherwise the eager layer plus
    :func:`pool_nodes`. The kernels take ``adj`` as the 0/1 matrix of the data pipeline (an entry > 0
    is an edge of weight one). ``time_major=True`` (HIP path only) returns ``(h [T, Mp, Cp], B)``,
    the time-major, row- and channel-padded input of
    :meth:`gnnqc.models.timelayer.TimeLayer.forward_time_major`, written by the kernel itself."""
    if edge_pool_hip_ok(x, layer, pooling):
        B = x.shape[0]
        Mp = Cp = 0
        if time_major:
            Mp = (B + 15) // 16 * 16
            Cp = layer.out_features + (anom.shape[-1] if anom is not None else 0)
            Cp += (-Cp) % 4
        mask_f = mask.float().contiguous()
        pw = gat_pool_weights(mask_f, anom_pos.long() if anom_pos is not None else None, pooling)
        out = _HipEdgePool.apply(x.contiguous(), adj.float().contiguous(), mask_f, anom, pw, layer.out.kernel,
                                 layer.out.bias, layer.prelu_alpha, _GAT_ACT[layer.activation],
                                 layer.aggregate == "mean", Mp, Cp)
        return (out, B) if time_major else out
    if time_major:
        raise ValueError("edge_pool(time_major=True) needs the HIP path")
    return edge_pool_eager(x, adj, mask, anom, anom_pos, layer, pooling)


# ---------------------------------------------------------------------------------------------
# AGNNConv + node pooling + concat (agnn.hip). ``layer`` is a :class:`gnnqc.models.graphconv.AGNNConv`
# (or anything with its attributes); the eager path is the layer itself plus :func:`pool_nodes`.
AGNN_MAX_NODES = 64                     # agnn.hip: one 64-bit neighbour word per node


class _HipAGNNPool(torch.autograd.Function):
    """Fused cosine-attention softmax -> neighbour aggregate -> activation -> node pool -> concat
    (HIP). Launches: edge_adj_bits and agnn_pool_fwd forward; agnn_pool_bwd, its fixed-order record
    sum and agnn_bwd_finalize (+ agnn_pool_bwd_input when dx is needed) backward. Parameter gradients
    go straight into the optimiser's flat buffer under direct accumulation, like :class:`_HipEdgePool`'s.
    With no parameter needing a gradient (a frozen ``beta`` and no PReLU) agnn_pool_bwd is not launched."""

    @staticmethod
    def forward(ctx, x, adj, mask, anom, pw, beta, alpha, act: int, mean: bool, Mp: int = 0, Cp: int = 0):
        from ..utils.native import hip_ops
        ops = hip_ops()
        bits = ops.edge_adj_bits(adj, mask)
        empty = x.new_zeros(0)
        anom_t = anom.contiguous() if anom is not None else empty
        al = alpha.contiguous() if alpha is not None else empty
        out = ops.agnn_pool_fwd(x, bits, pw, anom_t, beta.contiguous(), al, int(act), bool(mean), int(Mp), int(Cp))
        ctx.tm = Mp > 0
        ctx.act, ctx.mean = int(act), bool(mean)
        ctx.ca = 0 if anom is None else anom.shape[-1]
        ctx.has_anom = anom is not None
        ctx.params = (beta, alpha)
        ctx.save_for_backward(x, bits, pw, beta, al)
        return out

    @staticmethod
    def backward(ctx, dout):
        from ..utils.native import hip_ops
        from .wgrad import _grad_sink
        ops = hip_ops()
        x, bits, pw, beta, al = ctx.saved_tensors
        dout = dout.contiguous()
        need = ctx.needs_input_grad
        need_p = list(need[5:7])
        args = (beta.contiguous(), al, ctx.act, ctx.mean, ctx.ca, ctx.tm)
        empty = x.new_zeros(0)
        grads = [None] * 2
        if any(need_p):
            tot = ops.agnn_pool_bwd(x, bits, pw, dout, *args)
            # (a parameter that needs no gradient gets an empty sink: the finalizer discards its sum)
            sinks = [(_grad_sink(p) if n else (empty, True)) for p, n in zip(ctx.params, need_p)]
            ops.agnn_bwd_finalize(tot, *[s[0] for s in sinks])
            grads = [None if direct or not n else buf for (buf, direct), n in zip(sinks, need_p)]
        dx = ops.agnn_pool_bwd_input(x, bits, pw, dout, *args) if need[0] else None
        danom = None
        if ctx.has_anom and need[3]:
            danom = dout[:, : x.shape[0], : ctx.ca].transpose(0, 1) if ctx.tm else dout[..., : ctx.ca]
        return (dx, None, None, danom, None, *grads, None, None, None, None)


def agnn_pool_hip_ok(x: torch.Tensor, layer, pooling: str) -> bool:
    """Whether :func:`agnn_pool` runs the HIP kernels: a float32 GPU tensor ``[B, T, N, Cin]`` with
    1 <= N <= 64 and 1 <= Cin <= 4, a layer built for that width, sum or mean aggregation, linear node
    pooling and an activation the kernels implement. ``GNNQC_AGNN_HIP=0`` keeps the eager layer
    (A/B runs)."""
    import os

    from . import use_hip
    if os.environ.get("GNNQC_AGNN_HIP", "1") != "1" or x.dim() != 4 or x.dtype != torch.float32:
        return False
    return bool(use_hip(x) and 1 <= x.shape[2] <= AGNN_MAX_NODES and 1 <= x.shape[-1] <= 4
                and layer.in_features == x.shape[-1]
                and layer.aggregate in ("sum", "mean") and pooling in ("mean", "sum", "selection")
                and layer.activation in _GAT_ACT)


def agnn_pool_eager(x, adj, mask, anom, anom_pos, layer, pooling: str = "mean", time_major: bool = False):
    """Eager oracle of :func:`agnn_pool` in its output layouts: the layer, :func:`pool_nodes` and
    ``Concatenate([anom, pooled])``."""
    pooled = pool_nodes(layer(x, adj, mask), mask, anom_pos, pooling)
    out = pooled if anom is None else torch.cat([anom, pooled], dim=-1)
    return (_time_major_pad(out), x.shape[0]) if time_major else out


def agnn_pool(x, adj, mask, anom, anom_pos, layer, pooling: str = "mean", time_major: bool = False):
    """AGNNConv + node pooling + concat -> LSTM input ``[B, T, Ca + Cin]``; mirrors :func:`edge_pool`.

    Uses the fused HIP kernels when :func:`agnn_pool_hip_ok`, otherwise the eager layer plus
    :func:`pool_nodes`. The kernels take ``adj`` as the 0/1 matrix of the data pipeline (an entry > 0
    is an edge; under ``aggregate: mean`` the degree is the number of such entries).
    ``time_major=True`` (HIP path only) returns ``(h [T, Mp, Cp], B)``, the time-major, row- and
    channel-padded input of :meth:`gnnqc.models.timelayer.TimeLayer.forward_time_major`, written by
    the kernel itself."""
    if agnn_pool_hip_ok(x, layer, pooling):
        B = x.shape[0]
        Mp = Cp = 0
        if time_major:
            Mp = (B + 15) // 16 * 16
            Cp = layer.out_features + (anom.shape[-1] if anom is not None else 0)
            Cp += (-Cp) % 4
        mask_f = mask.float().contiguous()
        pw = gat_pool_weights(mask_f, anom_pos.long() if anom_pos is not None else None, pooling)
        out = _HipAGNNPool.apply(x.contiguous(), adj.float().contiguous(), mask_f, anom, pw, layer.beta,
                                 layer.prelu_alpha, _GAT_ACT[layer.activation], layer.aggregate == "mean", Mp, Cp)
        return (out, B) if time_major else out
    if time_major:
        raise ValueError("agnn_pool(time_major=True) needs the HIP path")
    return agnn_pool_eager(x, adj, mask, anom, anom_pos, layer, pooling)


# ---------------------------------------------------------------------------------------------
# GatedGraphConv + node pooling + concat (gated.hip). ``layer`` is a
# :class:`gnnqc.models.graphconv.GatedGraphConv` (or anything with its attributes); the eager path is
# the layer itself plus :func:`pool_nodes`.
GATED_MAX_NODES = 64                    # gated.hip: one 64-bit neighbour word per node
GATED_WIDTHS = (8, 16, 32)              # gated.hip GQ_GATED_DISPATCH: channels
GATED_MAX_LAYERS = 4                    # gated.hip: dW_l accumulators of the backward


class _HipGatedPool(torch.autograd.Function):
    """Fused message rounds (``h W_l`` -> neighbour sum -> GRU cell) -> activation -> node pool ->
    concat (HIP). Launches: edge_adj_bits and gated_pool_fwd forward; gated_pool_bwd, its fixed-order
    record sum and gated_bwd_finalize (+ gated_pool_bwd_input when dx is needed) backward. Parameter
    gradients go straight into the optimiser's flat buffer under direct accumulation, like
    :class:`_HipAGNNPool`'s. With no parameter needing a gradient gated_pool_bwd is not launched."""

    @staticmethod
    def forward(ctx, x, adj, mask, anom, pw, Wl, K, R, bias, alpha, act: int, Mp: int = 0, Cp: int = 0):
        from ..utils.native import hip_ops
        ops = hip_ops()
        bits = ops.edge_adj_bits(adj, mask)
        empty = x.new_zeros(0)
        anom_t = anom.contiguous() if anom is not None else empty
        al = alpha.contiguous() if alpha is not None else empty
        out = ops.gated_pool_fwd(x, bits, pw, anom_t, Wl.contiguous(), K.contiguous(), R.contiguous(),
                                 bias.contiguous(), al, int(act), int(Mp), int(Cp))
        ctx.tm = Mp > 0
        ctx.act = int(act)
        ctx.ca = 0 if anom is None else anom.shape[-1]
        ctx.has_anom = anom is not None
        ctx.params = (Wl, K, R, bias, alpha)
        ctx.save_for_backward(x, bits, pw, Wl, K, R, bias, al)
        return out

    @staticmethod
    def backward(ctx, dout):
        from ..utils.native import hip_ops
        from .wgrad import _grad_sink
        ops = hip_ops()
        x, bits, pw, Wl, K, R, bias, al = ctx.saved_tensors
        dout = dout.contiguous()
        need = ctx.needs_input_grad
        need_p = list(need[5:10])
        args = (Wl.contiguous(), K.contiguous(), R.contiguous(), bias.contiguous(), al, ctx.act, ctx.ca, ctx.tm)
        empty = x.new_zeros(0)
        grads = [None] * 5
        if any(need_p):
            tot = ops.gated_pool_bwd(x, bits, pw, dout, *args)
            # (a parameter that needs no gradient gets an empty sink: the finalizer discards its sum)
            sinks = [(_grad_sink(p) if n else (empty, True)) for p, n in zip(ctx.params, need_p)]
            ops.gated_bwd_finalize(tot, int(Wl.shape[0]), int(Wl.shape[1]), *[s[0] for s in sinks])
            grads = [None if direct or not n else buf for (buf, direct), n in zip(sinks, need_p)]
        dx = ops.gated_pool_bwd_input(x, bits, pw, dout, *args) if need[0] else None
        danom = None
        if ctx.has_anom and need[3]:
            danom = dout[:, : x.shape[0], : ctx.ca].transpose(0, 1) if ctx.tm else dout[..., : ctx.ca]
        return (dx, None, None, danom, None, *grads, None, None, None)


def gated_pool_hip_ok(x: torch.Tensor, layer, pooling: str) -> bool:
    """Whether :func:`gated_pool` runs the HIP kernels: a float32 GPU tensor ``[B, T, N, Cin]`` with
    1 <= N <= 64 and 1 <= Cin <= 4, a layer built for that input width with an instantiated channel
    count and 1..4 message rounds, linear node pooling and an activation the kernels implement.
    ``GNNQC_GATED_HIP=0`` keeps the eager layer (A/B runs)."""
    import os

    from . import use_hip
    if os.environ.get("GNNQC_GATED_HIP", "1") != "1" or x.dim() != 4 or x.dtype != torch.float32:
        return False
    C = layer.channels
    return bool(use_hip(x) and 1 <= x.shape[2] <= GATED_MAX_NODES and 1 <= x.shape[-1] <= 4
                and layer.in_features == x.shape[-1] and x.shape[-1] <= C and C in GATED_WIDTHS
                and 1 <= layer.n_layers <= GATED_MAX_LAYERS and tuple(layer.kernel.shape) == (layer.n_layers, C, C)
                and pooling in ("mean", "sum", "selection") and layer.activation in _GAT_ACT)


def gated_pool_eager(x, adj, mask, anom, anom_pos, layer, pooling: str = "mean", time_major: bool = False):
    """Eager oracle of :func:`gated_pool` in its output layouts: the layer, :func:`pool_nodes` and
    ``Concatenate([anom, pooled])``."""
    pooled = pool_nodes(layer(x, adj, mask), mask, anom_pos, pooling)
    out = pooled if anom is None else torch.cat([anom, pooled], dim=-1)
    return (_time_major_pad(out), x.shape[0]) if time_major else out


def gated_pool(x, adj, mask, anom, anom_pos, layer, pooling: str = "mean", time_major: bool = False):
    """GatedGraphConv + node pooling + concat -> LSTM input ``[B, T, Ca + C]``; mirrors :func:`agnn_pool`.

    Uses the fused HIP kernels when :func:`gated_pool_hip_ok`, otherwise the eager layer plus
    :func:`pool_nodes`. The kernels take ``adj`` as the 0/1 matrix of the data pipeline (an entry > 0
    is an edge of weight one; a weighted adjacency is not supported and not checked).
    ``time_major=True`` (HIP path only) returns ``(h [T, Mp, Cp], B)``, the time-major, row- and
    channel-padded input of :meth:`gnnqc.models.timelayer.TimeLayer.forward_time_major`, written by
    the kernel itself."""
    if gated_pool_hip_ok(x, layer, pooling):
        B = x.shape[0]
        Mp = Cp = 0
        if time_major:
            Mp = (B + 15) // 16 * 16
            Cp = layer.out_features + (anom.shape[-1] if anom is not None else 0)
            Cp += (-Cp) % 4
        mask_f = mask.float().contiguous()
        pw = gat_pool_weights(mask_f, anom_pos.long() if anom_pos is not None else None, pooling)
        out = _HipGatedPool.apply(x.contiguous(), adj.float().contiguous(), mask_f, anom, pw, layer.kernel,
                                  layer.rnn.kernel, layer.rnn.recurrent_kernel, layer.rnn.bias, layer.prelu_alpha,
                                  _GAT_ACT[layer.activation], Mp, Cp)
        return (out, B) if time_major else out
    if time_major:
        raise ValueError("gated_pool(time_major=True) needs the HIP path")
    return gated_pool_eager(x, adj, mask, anom, anom_pos, layer, pooling)


# ---------------------------------------------------------------------------------------------
# GATConv per node -> time-major LSTM input (gat_node.hip): the network-wide SoilNet front end.
GAT_NODE_MAX_NODES = 256                # gat_node.hip: up to four 64-bit neighbour mask words per node


class _HipGATNodeTM(torch.autograd.Function):
    """Fused edge softmax -> input-space aggregation -> W, bias, activation -> mask, written per node
    as the time-major LSTM input ``[T, Mp, Cp]`` (``gat_node.hip``). Launches: gat_node_adj_bits and
    gat_node_fwd forward; gat_node_bwd, its fixed-order record sum and gat_bwd_finalize (+
    gat_node_bwd_input when dx is needed, e.g. integrated gradients) backward. Parameter gradients
    go straight into the optimiser's flat buffer under direct accumulation, like
    :class:`_HipGATPool`'s."""

    @staticmethod
    def forward(ctx, x, adj, mask, W, a_s, a_n, bias, alpha, act: int, Mp: int, Cp: int):
        from ..utils.native import hip_ops
        ops = hip_ops()
        bits = ops.gat_node_adj_bits(adj, mask)
        al = alpha.contiguous() if alpha is not None else x.new_zeros(0)
        out = ops.gat_node_fwd(x, bits, mask, W.contiguous(), a_s.contiguous(), a_n.contiguous(), bias.contiguous(),
                               al, int(act), int(Mp), int(Cp))
        ctx.act = int(act)
        ctx.params = (W, a_s, a_n, bias, alpha)
        ctx.save_for_backward(x, bits, mask, W, a_s, a_n, bias, al)
        return out

    @staticmethod
    def backward(ctx, dout):
        from ..utils.native import hip_ops
        from .wgrad import _grad_sink
        ops = hip_ops()
        x, bits, mask, W, a_s, a_n, bias, al = ctx.saved_tensors
        dout = dout.contiguous()
        need = ctx.needs_input_grad
        need_p = list(need[3:8])
        args = (W.contiguous(), a_s.contiguous(), a_n.contiguous(), bias.contiguous(), al, ctx.act)
        empty = x.new_zeros(0)
        grads = [None] * 5
        if any(need_p):
            tot = ops.gat_node_bwd(x, bits, mask, dout, *args)
            sinks = [(_grad_sink(p) if n else (empty, True)) for p, n in zip(ctx.params, need_p)]
            ops.gat_bwd_finalize(tot, *args[:3], *[s[0] for s in sinks])
            grads = [None if direct or not n else buf for (buf, direct), n in zip(sinks, need_p)]
        dx = ops.gat_node_bwd_input(x, bits, mask, dout, *args) if need[0] else None
        return (dx, None, None, *grads, None, None, None)


def gat_node_tm_ok(x: torch.Tensor, layer) -> bool:
    """Whether :func:`gat_node_tm` runs for this input: a float32 GPU tensor ``[B, T, N, Cin]`` with
    N <= 256 and Cin <= 4, concatenated heads of an instantiated width, an activation the kernels
    implement and no attention dropout while training. ``GNNQC_GAT_HIP=0`` keeps the eager layer
    (A/B runs)."""
    import os

    from . import use_hip
    if os.environ.get("GNNQC_GAT_HIP", "1") != "1" or x.dim() != 4 or x.dtype != torch.float32:
        return False
    W = layer.kernel
    return bool(use_hip(x) and 1 <= x.shape[2] <= GAT_NODE_MAX_NODES and 1 <= x.shape[-1] <= 4
                and W.shape[0] == x.shape[-1] and not (layer.dropout_rate > 0 and layer.training)
                and layer.concat and W.shape[2] in GAT_WIDTHS[0] and W.shape[1] in GAT_WIDTHS[1]
                and layer.activation in _GAT_ACT)


def gat_node_tm(x, adj, mask, layer, cpad_to: int = 4):
    """SoilNet GATConv + ``Concatenate([gat, x])`` + ``graph_reshape`` as ONE time-major tensor;
    mirrors :func:`gcn_node_tm`.

    Returns ``(h [T, Mp, Cp], M)`` with row ``m = b*N + i``, channels ``[H*C gat | Cin raw | 0 pad]``
    (Cp a multiple of ``cpad_to``, itself a multiple of 4) and zero rows past ``M = B*N`` - the input
    layout of :meth:`gnnqc.models.timelayer.TimeLayer.forward_time_major`. HIP path only: raises
    when :func:`gat_node_tm_ok` does not hold."""
    if not gat_node_tm_ok(x, layer):
        raise ValueError("gat_node_tm needs the HIP path (see gat_node_tm_ok)")
    if cpad_to % 4:
        raise ValueError("gat_node_tm: cpad_to must be a multiple of 4")
    B, T, N, Cin = x.shape
    M = B * N
    Mp = (M + 15) // 16 * 16
    Cp = layer.out_features + Cin
    Cp += (-Cp) % cpad_to
    h = _HipGATNodeTM.apply(x.contiguous(), adj.float().contiguous(), mask.float().contiguous(), layer.kernel,
                            layer.attn_kernel_self, layer.attn_kernel_neighs, layer.bias, layer.prelu_alpha,
                            _GAT_ACT[layer.activation], Mp, Cp)
    return h, M


def gat_node_tm_eager(x, adj, mask, layer, cpad_to: int = 4):
    """Eager oracle of :func:`gat_node_tm` (same output layout): the layer, ``cat([h, x])``, permute
    and pad."""
    B, T, N, Cin = x.shape
    M = B * N
    Mp = (M + 15) // 16 * 16
    seq = torch.cat([layer(x, adj, mask), x], -1).permute(1, 0, 2, 3).reshape(T, M, -1)
    C = seq.shape[-1]
    return F.pad(seq, (0, (-C) % cpad_to, 0, Mp - M)), M


__all__ = ["gat_pool", "gat_pool_eager", "gat_pool_hip_ok", "gat_pool_weights",
           "gat_node_tm", "gat_node_tm_eager", "gat_node_tm_ok",
           "edge_pool", "edge_pool_eager", "edge_pool_hip_ok",
           "agnn_pool", "agnn_pool_eager", "agnn_pool_hip_ok",
           "gated_pool", "gated_pool_eager", "gated_pool_hip_ok",
           "gcn_pool", "gcn_pool_hip_ok", "gcn_node_tm", "gcn_node_tm_eager", "gcn_node_tm_ok", "node_pool_weights", "masked_batchnorm", "general_conv_eager", "pool_nodes",
           "normalized_adjacency", "prelu"]
