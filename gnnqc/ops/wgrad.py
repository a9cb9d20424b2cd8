"""Where the operators' weight gradients go, and when the LSTM weight-gradient launches run.

Under :func:`direct_grad_accumulation` (the training engine) the HIP backward kernels add weight
gradients straight into ``param.grad`` (:func:`_grad_sink`); elsewhere they are handed back to
autograd (:func:`returned_grads`). In direct mode the LSTM layers' weight-gradient passes are not
launched where they arise but queued (:class:`_Pipe`) and run behind later recurrences or in one
batched launch at the end of the backward, and split reductions can wait for the context's exit
(:func:`_deferred_reduce`).
"""
from __future__ import annotations

import contextlib

import torch

from . import switch_on


def _ops():
    # (fetched on every call: tools and tests put a recording namespace in its place)
    from ..utils import native
    return native.hip_ops()


class _DirectGrad:
    """When enabled (by the training engine), LSTM weight gradients are accumulated by the
    ``lstm_grads`` kernels straight into ``param.grad`` (the optimiser's flat gradient
    buffer views) instead of being returned to autograd - no separate AccumulateGrad add
    per parameter. Off by default so that ``torch.autograd.grad`` (e.g. integrated
    gradients) never touches ``.grad``. In this mode the weight-gradient passes are deferred
    and batched (:class:`_Pipe`).

    (Measured on MI355X and removed: dW/dU/db on a side stream behind a dx-only kernel -
    0.885 vs 0.757 ms/step, cross-stream event waits cost more than the overlap won - and the
    chain's weight-gradient batch on a side stream concurrent with the GCN backward, 0.3812 vs
    0.3788 ms/step.)"""

    enabled = False


class _Unflagged:
    count = 0     # gradients handed back to autograd (summed into .grad by PyTorch: no non-finite flag)


def unflagged_grad_writes() -> int:
    """How many weight gradients so far went through autograd's own accumulation instead of a HIP
    kernel that raises the non-finite flag (chain control word 7). The trainer takes the flag-driven
    Adam only for steps whose backward added none (``gnnqc.train.engine.Trainer._body``)."""
    return _Unflagged.count


def _grad_sink(p: torch.Tensor):
    """(buffer, direct): ``p.grad`` itself in direct mode, else a zero buffer to hand to autograd."""
    g = p.grad if _DirectGrad.enabled and isinstance(p, torch.nn.Parameter) else None
    if g is not None and g.is_contiguous() and g.dtype == torch.float32 and g.device == p.device:
        return g, True
    _Unflagged.count += 1
    return torch.zeros_like(p), False


def _layer_sinks(params, need_w, like: torch.Tensor):
    """The sinks of one LSTM layer's (W, U, b); empty stand-ins when none of them needs a gradient
    (the fused backward kernels skip the weight pass for empty buffers)."""
    if any(need_w):
        return [_grad_sink(p) for p in params]
    return [(like.new_zeros(0), True)] * 3


def returned_grads(sinks, need):
    """What a backward hands to autograd for ``sinks``: nothing for a gradient that went into
    ``.grad`` directly or that is not needed, else the buffer."""
    return [None if (direct or not n) else buf for (buf, direct), n in zip(sinks, need)]


class _Pipe:
    """Pipelined backward (direct-accumulation mode only; measured 0.667 vs 0.709 ms/step for
    one weight-gradient kernel per layer behind its recurrence, the fallback for layers the pipe
    does not take).

    A layer's weight-gradient pass does not feed any later recurrence, so it is deferred:
    each time-major backward recurrence launches ONE kernel (``lstm_tm_bwd_pipe``) whose
    first workgroups run the recurrence (a handful of tiles - most CUs idle) while the
    remaining workgroups run the weight-gradient pass of the previously finished layer and
    the split reduction of the one before. dx of the layer is a separate small kernel
    (the next recurrence's input). Leftover work is flushed when the direct-accumulation
    context exits. Single stream: ordering is plain stream order, no events."""

    enabled = True  # (tests switch it off to compare with the per-layer fused backward)
    job = None      # layer whose weight-gradient pass has not run yet
    red = None      # layer whose gradient pass ran; its split reduction has not
    batch = []      # jobs of a chain backward: all gradient passes in one launch at the flush
    reds = []       # layers whose records the chain backward built itself: reduce-only entries of that flush
    gcn = None      # (gcn_t, gcn_i): the fused GCN backward, run as extra workgroups of that launch


# Largest sequence count (rows of 16-sequence tiles) a recurrence may have for its layer to
# join the pipe: the gradient workgroups only help when the recurrence leaves most CUs idle
# (CML: 8 tiles). With hundreds of tiles (SoilNet: 418) they compete with the recurrence
# for the CUs and the step got slower (6.11 vs 5.15 ms), so such layers keep the fused path.
PIPE_MAX_SEQ = 2048

_MULTI_MAX = 12        # jobs per lstm_grads_multi launch (lstm_grads_jobs.hip MULTI_MAX)


def _pipe_on(sinks, n_seq: int) -> bool:
    return _Pipe.enabled and _DirectGrad.enabled and all(d for _, d in sinks) and n_seq <= PIPE_MAX_SEQ


def _pipe_x_ok(x: torch.Tensor, Dw: int) -> bool:
    return (x.stride(-1) == 1 and x.stride(-2) % 4 == 0 and x.data_ptr() % 16 == 0 and (Dw + 16) // 16 <= 5
            and x.shape[-1] % 4 == 0)


def _pipe_takes(x, W, g, sinks, need_w) -> bool:
    """Whether a time-major layer's backward goes through the pipe: weight gradients wanted, saved
    gates (the pipe kernel does not recompute them), sinks and an input layout the jobs take."""
    return any(need_w) and g.numel() > 0 and _pipe_on(sinks, x.shape[1]) and _pipe_x_ok(x, W.shape[0])


def _pipe_job(dz, x, h, W, sinks, period: int, hshift: int):
    H = W.shape[1] // 4
    return dict(dz=dz, x=x, h=h, W=W, period=int(period), hshift=int(hshift),
                ws=_ops().lstm_grads_job_ws(dz, x, W, H), g=[s for s, _ in sinks])


def _pipe_launch(dh=None, g=None, c=None, W=None, U=None, T: int = 0, job=None, red=None):
    """One pipe kernel: [recurrence] + [grads of ``job``] + [reduce of ``red``]. Returns dz."""
    ref = dh if dh is not None else (job or red)["dz"]
    e = ref.new_zeros(0)
    rec = (dh, g, c, W, U) if dh is not None else (e, e, e, e, e)
    jb = (job["dz"], job["x"], job["h"], job["W"], job["period"], job["hshift"], job["ws"]) if job else \
        (e, e, e, e, 1, 1, e)
    rd = (red["ws"], red["W"], *red["g"]) if red else (e, e, e, e, e)
    return _ops().lstm_tm_bwd_pipe(*rec, int(T), *jb, *rd)


def _pipe_drain_one():
    """Advance the pending jobs by one stage without a recurrence."""
    job, red = _Pipe.job, _Pipe.red
    if job is None and red is None:
        return
    _pipe_launch(job=job, red=red)
    _Pipe.job, _Pipe.red = None, job


def defer_to_grads_launch(gcn_lists) -> bool:
    """Queue the fused GCN backward (``lstm_grads_multi``'s gcn_t / gcn_i lists) onto the pending
    batched weight-gradient launch of this backward: the two are independent, and one launch
    overlaps them on the CUs the recurrences left idle. False (the caller launches it itself) when
    no batch is pending or ``GNNQC_GCN_DEFER=0``."""
    if not (_DirectGrad.enabled and _Pipe.batch and _Pipe.gcn is None and switch_on("GNNQC_GCN_DEFER")):
        return False
    _Pipe.gcn = gcn_lists
    return True


def pipe_flush():
    """Run all pending weight-gradient / reduction work (end of the backward). With a chain
    backward's batch: every pending gradient pass in ONE launch, every reduction in one more."""
    if _Pipe.batch or _Pipe.reds:
        grads = ([_Pipe.job] if _Pipe.job is not None else []) + _Pipe.batch
        reds = ([_Pipe.red] if _Pipe.red is not None else []) + _Pipe.reds + grads
        gt, gi = _Pipe.gcn if _Pipe.gcn is not None else ([], [])
        _ops().lstm_grads_multi([j["dz"] for j in grads], [j["x"] for j in grads], [j["h"] for j in grads],
                                [j["W"] for j in grads], [j["period"] for j in grads],
                                [j["hshift"] for j in grads], [j["ws"] for j in grads],
                                [r["ws"] for r in reds], [r["W"] for r in reds], [r["g"][0] for r in reds],
                                [r["g"][1] for r in reds], [r["g"][2] for r in reds], gt, gi)
        _Pipe.job, _Pipe.red, _Pipe.batch, _Pipe.reds, _Pipe.gcn = None, None, [], [], None
    while _Pipe.job is not None or _Pipe.red is not None:
        _pipe_drain_one()


def _pipe_push(job):
    """Queue ``job``: if a job is still pending (no recurrence consumed it), advance first."""
    if _Pipe.job is not None:
        _pipe_drain_one()
    _Pipe.job = job


def _pipe_tm_backward(dh, g, c, x, h, W, U, sinks, need_dx):
    """Time-major layer backward in pipe mode: one pipe launch (recurrence + pending grads +
    pending reduce), dx = dz W^T, then this layer's own weight-gradient job is queued."""
    T, Mp = x.shape[0], x.shape[1]
    HR = U.shape[0]
    if dh.dim() == 2:        # gradient only at the last step
        dh = torch.nn.functional.pad(dh.unsqueeze(0), (0, 0, 0, 0, T - 1, 0))
    job, red = _Pipe.job, _Pipe.red
    if job is not None and job["W"].shape[1] // 4 not in (HR, 2 * HR):
        _pipe_drain_one()              # shape the fused kernel does not take: run it alone
        job, red = _Pipe.job, _Pipe.red
    dz = _pipe_launch(dh, g, c, W, U, T, job, red)
    _Pipe.job, _Pipe.red = None, job
    dx = _ops().lstm_dx(dz, W, x) if need_dx else None
    _pipe_push(_pipe_job(dz, x, h, W, sinks, T * Mp, Mp))
    return dx


def _pipe_chain_layer(dz, x, h, W, sinks, need_w, ws=None):
    """Route the weight gradient of one layer of a finished chain backward (``dz`` [T, Mp, 4H] from
    the launch): with ``ws``, the records the launch built itself, a reduce-only entry of the flush;
    else a job of the flush's batched launch while it has room (that launch also takes a pipe job and
    a pipe reduce still pending: two of its ``_MULTI_MAX`` slots) and the queue takes the layer; else
    its own launch now. Returns the gradients to hand to autograd (``sinks`` None: a frozen layer, nothing to do)."""
    if sinks is None or not any(need_w):
        return [None, None, None]
    if ws is not None:
        _Pipe.reds.append(dict(ws=ws, W=W, g=[s for s, _ in sinks]))
    elif _pipe_on(sinks, h.shape[1]) and _pipe_x_ok(x, W.shape[0]) and len(_Pipe.batch) < _MULTI_MAX - 2:
        _Pipe.batch.append(_pipe_job(dz, x, h, W, sinks, h.shape[0] * h.shape[1], h.shape[1]))
    else:
        _ops().lstm_tm_grads(dz, x, h, W, sinks[0][0], sinks[1][0], sinks[2][0], False)
    return returned_grads(sinks, need_w)


class _Deferred:
    pending = False     # split reductions queued in the native library (lstm_reduce_flush)


@contextlib.contextmanager
def _deferred_reduce(on: bool):
    """Queue the split reductions of the weight-gradient launches issued inside (direct
    accumulation into the optimiser's gradient buffers only: nothing reads those before the
    step's optimizer update) for :func:`direct_grad_accumulation`'s exit, which runs all of them
    in one launch (``lstm_reduce_flush``) instead of one reduce launch per layer."""
    if not (on and _DirectGrad.enabled and switch_on("GNNQC_DEFER_REDUCE")):
        yield
        return
    ops = _ops()
    prev = ops.lstm_defer_reduce(True)
    _Deferred.pending = True
    try:
        yield
    finally:
        ops.lstm_defer_reduce(prev)


@contextlib.contextmanager
def direct_grad_accumulation(flag: bool = True):
    prev = _DirectGrad.enabled
    _DirectGrad.enabled = flag
    try:
        yield
    finally:
        _DirectGrad.enabled = prev
        if _Pipe.job is not None or _Pipe.red is not None or _Pipe.batch or _Pipe.reds:
            pipe_flush()
        _Pipe.gcn = None
        if _Deferred.pending:
            _Deferred.pending = False
            _ops().lstm_reduce_flush()
