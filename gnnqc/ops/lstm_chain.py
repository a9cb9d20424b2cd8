"""The cross-CU pipelined LSTM chain: a stack of time-major layers as one forward and one backward
launch (``lstm_chain_fwd.hip`` / ``lstm_chain_bwd.hip``), alone (:func:`lstm_chain_tm`) or with time4,
the classifier head and the loss as further stages (:func:`lstm_chain_head_tm`), the launches'
residency rule and the device's chain control words."""
from __future__ import annotations

from typing import Optional

import torch

from . import switch_on
from .wgrad import _grad_sink, _ops, _pipe_chain_layer, _pipe_on, _pipe_x_ok, returned_grads


def _chain_on() -> bool:
    """Cross-CU pipelined forward of the time-major LSTM stack (``GNNQC_CHAIN``, default on)."""
    return switch_on("GNNQC_CHAIN")


def _chain_bwd_on() -> bool:
    """Cross-CU pipelined backward of the chain (``GNNQC_CHAIN_BWD``, default on)."""
    return switch_on("GNNQC_CHAIN_BWD")


def _t4_chain_on() -> bool:
    """time4 + head as a stage of the chain launches (``lstm_chain_head_fwd`` / ``_bwd``;
    ``GNNQC_T4_CHAIN``, default on) instead of their own launches after / before the chain."""
    return switch_on("GNNQC_T4_CHAIN")


class _ChainWgrad:
    on = None       # GNNQC_CHAIN_WGRAD, read once per process (tests set it)


def _chain_wgrad_on() -> bool:
    """The upper layers' (H = 32 / 64 chain stages, time4) weight-gradient records are built by their
    own workgroups of the chain backward launch (``chain_wgrad.h``; ``GNNQC_CHAIN_WGRAD``, default
    on) instead of by jobs of the ``lstm_grads_multi`` launch behind it."""
    if _ChainWgrad.on is None:
        _ChainWgrad.on = switch_on("GNNQC_CHAIN_WGRAD")
    return _ChainWgrad.on


def _chain_wgrad_ws(x, h, W, sinks, need_w):
    """The workspace (one record per 16-sequence tile) of a chain layer whose weight gradients its own
    backward workgroups can build, or None: the layer keeps its job of the tail launch (an H = 16
    layer: the critical path; frozen weights; gradient buffers or an input layout the jobs do not take)."""
    H = W.shape[1] // 4
    if not (_chain_wgrad_on() and H in (32, 64, 128) and any(need_w) and _pipe_on(sinks, h.shape[1])
            and _pipe_x_ok(x, W.shape[0]) and W.shape[0] <= 64 and x.dim() == 3
            and x.stride(0) == x.shape[1] * x.stride(1)):
        return None
    return _ops().lstm_grads_record_ws(W, h.shape[1] // 16)


def _device_index(device) -> Optional[int]:
    device = torch.device(device)
    if device.type != "cuda":
        return None
    return device.index if device.index is not None else torch.cuda.current_device()


_CHAIN_CAP = {}


def chain_capacity(device) -> int:
    """Chain workgroups that can be resident at once on ``device``: its CU count (queried: a
    partitioned MI355X exposes 32 or 64) times the occupancy of the 1024-thread chain kernels."""
    idx = _device_index(device)
    if idx is None:
        return 0
    if idx not in _CHAIN_CAP:
        _CHAIN_CAP[idx] = int(_ops().lstm_chain_capacity(torch.empty(0, device=torch.device("cuda", idx))))
    return _CHAIN_CAP[idx]


def chain_fits(Mp: int, n_stages: int, device=None, spare: int = 0) -> bool:
    """All workgroups of a chain launch must be co-resident (one 1024-thread workgroup per CU);
    ``spare``: workgroups needed besides the stages' (the weight-gradient role of the backward)."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return (2 <= n_stages <= 8 and n_stages * ((Mp // 16 + 7) // 8 * 8) + spare <= chain_capacity(device))


_CHAIN_CTL = {}


def chain_ctl(device) -> Optional[torch.Tensor]:
    """The device's chain control words ``[epoch, finished, timeout flag, rejected steps, fwd / bwd
    head tickets, debug spin limit, non-finite gradient flag, head backward arrivals, 0 ...]`` as an
    int32[16] view (``lstm_chain_ctl.hip``); None off the GPU. The optimiser's update reads and clears
    the timeout / non-finite flags inside the captured step."""
    idx = _device_index(device)
    if idx is None:
        return None
    if idx not in _CHAIN_CTL:
        _CHAIN_CTL[idx] = _ops().lstm_chain_ctl(torch.empty(0, device=torch.device("cuda", idx)))
    return _CHAIN_CTL[idx]


class ChainTimeoutError(RuntimeError):
    """A chain consumer gave up waiting for its producer (not all workgroups were resident, or
    another kernel held the CUs): the affected results were computed from stale data."""


def check_chain(device, rejected_before: Optional[int] = None) -> int:
    """Raise :class:`ChainTimeoutError` if a chain spin timed out since the last check (forward-only
    use: evaluation, prediction) or if training steps were rejected for it since
    ``rejected_before``. Synchronises. Returns the current rejected-step count."""
    ctl = chain_ctl(device)
    if ctl is None:
        return 0
    v = ctl.cpu().tolist()
    if v[2]:
        ctl[2:3].zero_()
        raise ChainTimeoutError("LSTM chain kernel: a consumer spin timed out; results of this pass are invalid "
                                "(is another kernel sharing the GPU, or is the device partitioned?)")
    if rejected_before is not None and v[3] > rejected_before:
        raise ChainTimeoutError(f"LSTM chain kernel: {v[3] - rejected_before} training step(s) rejected after a "
                                "consumer spin timeout (skipped on the device, parameters untouched)")
    return int(v[3])


class _ChainSaved:
    """A chain's saved state by name. ``outs``: five tensors per stage, as the chain forward returns
    them; ``x``: the chain's input; ``pools[i]`` > 0: a MaxPooling1D after stage i."""

    def __init__(self, x, outs, pools):
        self.x, self.outs, self.pools = x, outs, pools

    def h(self, i):
        return self.outs[5 * i]

    def gates(self, i):
        return self.outs[5 * i + 1]

    def c(self, i):
        return self.outs[5 * i + 2]

    def pooled(self, i):
        return self.outs[5 * i + 3]

    def argmax(self, i):
        return self.outs[5 * i + 4]

    def out(self, i):
        """What stage i hands on: its pooled output where it has a pool, else h."""
        return self.pooled(i) if self.pools[i] else self.h(i)

    def x_in(self, i):
        """The input of stage i (i = the number of stages: of the layer after the chain)."""
        return self.x if i == 0 else self.out(i - 1)


def _stack_params(mods):
    return [p for m in mods for p in (m.kernel, m.recurrent_kernel, m.bias)]


def _per_layer(seq, first: int, n: int):
    """``seq[first:]`` cut into ``n`` (W, U, b) triples."""
    return [seq[first + 3 * i:first + 3 * i + 3] for i in range(n)]


def _needed_sinks(params, need_w):
    """The gradient sinks of the layers whose weights need a gradient, by layer (a frozen layer has
    none: a sink handed to autograd counts as an unflagged gradient write)."""
    return {i: [_grad_sink(p) for p in ps] for i, (ps, nw) in enumerate(zip(params, need_w)) if any(nw)}


def _chain_bwd_args(st, Ws, Us, hs, sinks, need_w, t4_stage: bool = False):
    """The per-stage lists of ``lstm_chain_bwd`` (the arguments after dh; the last ones of
    ``lstm_chain_head_bwd``), top stage first, and ``wws``: by layer, the record workspace that the
    layer's own backward workgroups fill inside the launch (:func:`_chain_wgrad_ws`), or None.
    ``hs``: every layer's h; ``t4_stage``: time4 (layer ``ns``) is a stage of the launch too. The
    ``wgrad`` list (per stage x, h, workspace or empty; then time4's workspace) is left out when no
    layer builds records."""
    ns = len(st.pools)
    order = list(reversed(range(ns)))
    e, e8 = st.x.new_zeros(0), st.x.new_zeros(0, dtype=torch.uint8)
    wws = {i: _chain_wgrad_ws(st.x_in(i), hs[i], Ws[i], sinks[i], need_w[i]) if i in sinks else None
           for i in (order + [ns] if t4_stage else order)}
    args = [[st.gates(i) for i in order], [st.c(i) for i in order], [Ws[i] for i in order], [Us[i] for i in order],
            [st.argmax(i) if st.pools[i] else e8 for i in order], [st.pools[i] for i in order],
            [st.x_in(i).shape[-1] for i in order], [st.h(i).shape[0] for i in order]]
    if any(w is not None for w in wws.values()):
        wgrad = [t for i in order for t in (st.x_in(i), st.h(i), wws[i] if wws[i] is not None else e)]
        if t4_stage:
            wgrad.append(wws[ns] if wws[ns] is not None else e)
        args.append(wgrad)
    return args, wws


def _chain_wgrads(st, Ws, hs, dzs, sinks, need_w, wws):
    """Route every layer's weight gradient after the launch, top layer first (the order of the tail
    launch's jobs); the flat list of gradients to hand to autograd."""
    grads = [None] * (3 * len(hs))
    for i in reversed(range(len(hs))):
        grads[3 * i:3 * i + 3] = _pipe_chain_layer(dzs[i], st.x_in(i), hs[i], Ws[i], sinks.get(i), need_w[i],
                                                   wws.get(i))
    return grads


class _HipLSTMChain(torch.autograd.Function):
    """A stack of time-major layers (with MaxPooling1D between some of them) whose forward
    runs as ONE cross-CU pipelined kernel (``lstm_chain_fwd.hip``: every layer of a 16-sequence
    tile on its own CU, consuming the previous layer's output as it is produced). The backward is
    ONE such launch too (``lstm_chain_bwd.hip``) where it fits, else the per-layer backward kernels
    in reverse, un-pooling between them."""

    @staticmethod
    def forward(ctx, x, pools, *params):
        ns = len(pools)
        Ws, Us, bs = ([params[3 * i + k].contiguous() for i in range(ns)] for k in range(3))
        need = any(ctx.needs_input_grad)
        outs = _ops().lstm_chain_fwd(x, Ws, Us, bs, [int(p) for p in pools], need)
        ctx.pools = tuple(int(p) for p in pools)
        ctx.params = params
        if need:
            ctx.save_for_backward(x, *Ws, *Us, *outs)
        return _ChainSaved(x, outs, pools).out(ns - 1)

    @staticmethod
    def backward(ctx, dout):
        ops = _ops()
        pools = ctx.pools
        ns = len(pools)
        saved = ctx.saved_tensors
        Ws, Us = saved[1:1 + ns], saved[1 + ns:1 + 2 * ns]
        st = _ChainSaved(saved[0], saved[1 + 2 * ns:], pools)
        need = ctx.needs_input_grad
        params, need_w = _per_layer(ctx.params, 0, ns), _per_layer(need, 2, ns)
        dh = dout.contiguous()
        if (_chain_bwd_on() and chain_fits(dh.shape[1], ns, dh.device)
                and all(st.x_in(i).shape[-1] % 4 == 0 for i in range(ns))):
            # all reverse recurrences in ONE cross-CU pipelined launch (dz of every layer + dx
            # of the bottom one), then the weight-gradient passes
            hs = [st.h(i) for i in range(ns)]
            sinks = _needed_sinks(params, need_w)
            args, wws = _chain_bwd_args(st, Ws, Us, hs, sinks, need_w)
            res = ops.lstm_chain_bwd(dh, *args)
            grads = _chain_wgrads(st, Ws, hs, res[ns - 1::-1], sinks, need_w, wws)
            return (res[ns] if need[0] else None, None, *grads)
        from .lstm import _tm_layer_backward
        grads = [None] * (3 * ns)
        dx = None
        for i in reversed(range(ns)):
            h = st.h(i)
            T, Mp, H = h.shape
            if pools[i]:
                dh = ops.maxpool1d_bwd(dh.view(1, -1, Mp * H), st.argmax(i).view(1, -1, Mp * H), T,
                                       pools[i]).view(T, Mp, H)
            dx, grads[3 * i:3 * i + 3] = _tm_layer_backward(dh, st.x_in(i), Ws[i], Us[i], params[i][2], h, st.gates(i),
                                                            st.c(i), params[i], need_w[i], i > 0 or bool(need[0]))
            dh = dx
        return (dx if need[0] else None, None, *grads)


class _HipLSTMChainHead(torch.autograd.Function):
    """CML TimeLayer + classifier head + weighted BCE in two forward and two backward launches:
    the six pipelined time-major layers as ONE chain kernel (``lstm_chain_fwd.hip``), then time4
    (H = 128, last state) with the Dense head, the loss and the metric accumulation as ONE
    kernel (``time4_head.hip``); backward: the head backward + time4's reverse recurrence as ONE
    kernel, whose dx (gradient of the chain's pooled output) feeds ONE chain backward.

    Weight gradients: the H = 32 / 64 layers' and time4's backward workgroups are done 30 - 60 us into
    a launch that the two H = 16 stages hold open for ~100 us, so each builds the dW | db and dU
    record of its own 16-sequence tile after its reverse steps (``chain_wgrad.h``,
    ``GNNQC_CHAIN_WGRAD``, default on) and the ``lstm_grads_multi`` launch behind the chain only
    reduces those; the two H = 16 layers' passes (and the GCN backward) still run in that launch, now
    alone, and all seven reductions in one more. (In-launch chain weight gradients were rejected in
    rounds 3 and 5 for the critical-path stages: the H = 16 stages' post-pass lengthened the launch.
    They still have none. With the switch off all seven passes run in the ``lstm_grads_multi`` launch.)

    Inputs: x [T, Mp, C] time-major, y / mask [M]; ``consts`` = (alpha1, alpha2, w0, w1);
    params = 7 x (W, U, b) then the head's (W1, b1, W2, b2, W3, b3). Returns (loss, logits [M])."""

    @staticmethod
    def forward(ctx, x, y, mask, sums, hist, consts, pools, M, *params):
        ops = _ops()
        ns = len(pools)                    # chain stages (time4 follows)
        Ws, Us, bs = ([params[3 * i + k].contiguous() for i in range(ns + 1)] for k in range(3))
        head = [p.contiguous() for p in params[3 * (ns + 1):]]
        need = any(ctx.needs_input_grad)
        e = x.new_zeros(0)
        sums_ = sums if sums is not None else e.double()
        hist_ = hist if hist is not None else e
        if _t4_chain_on() and pools[-1] == 3:
            # time4 + head + loss as one more stage of the chain launch (it consumes the last
            # stage's output as it is produced); spare workgroups build time4's backward fragments
            outs = ops.lstm_chain_head_fwd(x, Ws[:ns], Us[:ns], bs[:ns], [int(p) for p in pools], need, Ws[ns],
                                           Us[ns], bs[ns], head, y, mask, int(M), *[float(c) for c in consts],
                                           sums_, hist_)
            h4, g4, c4, logits, loss = outs[-5:]
            del outs[-5:]
            hb = outs.pop()       # the head's dh_{T-1} computed by the launch (dL/dloss = 1), or empty
            pk = outs.pop()
        else:
            # (the chain's spare workgroups build time4's weight-fragment image on the way)
            outs = ops.lstm_chain_fwd_pack(x, Ws[:ns], Us[:ns], bs[:ns], [int(p) for p in pools], need, Ws[ns],
                                           Us[ns])
            pk = outs.pop()
            hb = e
            xt = _ChainSaved(x, outs, pools).x_in(ns)      # time4's input [T4, Mp, C]
            h4, g4, c4, logits, loss = ops.time4_head_fwd(xt, Ws[ns], Us[ns], bs[ns], pk, need, head, y, mask, int(M),
                                                          *[float(c) for c in consts], sums_, hist_)
        ctx.pools, ctx.consts, ctx.M = tuple(int(p) for p in pools), tuple(float(c) for c in consts), int(M)
        ctx.params = params
        ctx.set_materialize_grads(False)     # (no zeros tensor for the non-differentiable logits)
        if need:
            ctx.save_for_backward(x, y, mask, *Ws, *Us, *head, *outs, h4, g4, c4, pk, hb)
        ctx.mark_non_differentiable(logits)
        return loss.reshape(()), logits

    @staticmethod
    def backward(ctx, dloss, _dlogits):
        ops = _ops()
        pools = ctx.pools
        ns = len(pools)
        saved = ctx.saved_tensors
        y, mask = saved[1:3]
        Ws, Us = saved[3:4 + ns], saved[4 + ns:5 + 2 * ns]
        head = saved[5 + 2 * ns:11 + 2 * ns]
        st = _ChainSaved(saved[0], saved[11 + 2 * ns:11 + 7 * ns], pools)
        h4, g4, c4, pk, hb = saved[11 + 7 * ns:]
        need = ctx.needs_input_grad
        npar = 3 * (ns + 1)
        params, need_w = _per_layer(ctx.params, 0, ns + 1), _per_layer(need, 8, ns + 1)
        g = dloss.reshape(1).float()
        if not g.is_contiguous():
            g = g.contiguous()
        hsinks = [_grad_sink(p) for p in ctx.params[npar:]]
        xt = st.x_in(ns)
        hs = [st.h(i) for i in range(ns)] + [h4]
        sinks = _needed_sinks(params, need_w)
        t4_chain = _t4_chain_on() and pools[-1] == 3 and xt.is_contiguous()
        args, wws = _chain_bwd_args(st, Ws, Us, hs, sinks, need_w, t4_chain)
        if t4_chain:
            # time4 + head backward as the first stage of the chain backward launch: the top
            # chain stage consumes time4's dx as it is produced
            res = ops.lstm_chain_head_bwd(g, xt, h4, g4, c4, Ws[ns], Us[ns], pk, hb, list(head), y, mask, ctx.M, *ctx.consts,
                                          [s for s, _ in hsinks], *args)
            dz4 = res.pop(0)
        else:
            dz4, dxt = ops.time4_head_bwd(g, xt, h4, g4, c4, Ws[ns], Us[ns], pk, list(head), y, mask, ctx.M,
                                          *ctx.consts, [s for s, _ in hsinks])
            res = ops.lstm_chain_bwd(dxt, *args)
        grads = _chain_wgrads(st, Ws, hs, [*res[ns - 1::-1], dz4], sinks, need_w, wws)
        return (res[ns] if need[0] else None, None, None, None, None, None, None, None, *grads,
                *returned_grads(hsinks, need[8 + npar:]))


def lstm_chain_tm(x_tm: torch.Tensor, mods, pools) -> torch.Tensor:
    """Forward of stacked LSTM modules (``gnnqc.models.layers.LSTM``, all returning sequences)
    with ``pools[i]`` > 0 a MaxPooling1D after module i; returns the last stage's output."""
    return _HipLSTMChain.apply(x_tm, tuple(int(p) for p in pools), *_stack_params(mods))


def lstm_chain_head_tm(x_tm: torch.Tensor, mods, pools, head, y: torch.Tensor, mask: torch.Tensor, M: int,
                       alpha1: float, alpha2: float, w0: float, w1: float, sums=None, hist=None):
    """(loss, logits) of ``mods`` (LSTM modules: the chain layers, then time4 - H = 128 returning its
    last state) followed by the Dense head ``head`` = (dense, dense2, dense_out) and the weighted
    BCE. ``pools``: the chain layers' pools (time4 has none)."""
    params = _stack_params(mods) + [p for d in head for p in (d.kernel, d.bias)]
    return _HipLSTMChainHead.apply(x_tm, y, mask, sums, hist, (alpha1, alpha2, w0, w1), tuple(int(p) for p in pools),
                                   int(M), *params)
