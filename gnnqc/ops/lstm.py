"""Keras-semantics LSTM layer.

Gate order i, f, c(g), o; ``z_t = x_t W + h_{t-1} U + b``; recurrent activation
sigmoid; ``activation`` (tanh by default) for g and the cell output; zero initial
state (Keras ``LSTM`` as built by ``libs/create_model.py:61-79``).

GPU path: one library GEMM for the input projection of all T steps, then the
persistent HIP recurrence (``lstm_fwd``); backward = persistent BPTT kernel
(``lstm_bwd``) producing dz for all steps, then the weight/input gradients as
plain GEMMs over all (sequence, step) rows.

Here: that sequence-major layer, the time-major layer and layer pair (``lstm_tm_*.hip``), the
H = 128 last-state layer (``time4_head.hip``) and the predicates that choose between them. The
cross-CU chain of time-major layers is :mod:`gnnqc.ops.lstm_chain`; where weight gradients go and
when their launches run is :mod:`gnnqc.ops.wgrad`. Both modules' public names are also exported here.
"""
from __future__ import annotations

import torch

from . import switch_on, use_hip
from .lstm_chain import (ChainTimeoutError, chain_capacity, chain_ctl, chain_fits, check_chain,  # noqa: F401
                         lstm_chain_head_tm, lstm_chain_tm)
from .wgrad import (PIPE_MAX_SEQ, _deferred_reduce, _grad_sink, _layer_sinks, _ops, _Pipe, _pipe_job, _pipe_on,
                    _pipe_push, _pipe_takes, _pipe_tm_backward, _pipe_x_ok, defer_to_grads_launch,  # noqa: F401
                    direct_grad_accumulation, pipe_flush, returned_grads, unflagged_grad_writes)  # noqa: F401

_ACT = {
    "tanh": torch.tanh,
    "relu": torch.relu,
    "sigmoid": torch.sigmoid,
    "linear": lambda x: x,
    None: lambda x: x,
}


def lstm_eager(x: torch.Tensor, W: torch.Tensor, U: torch.Tensor, b: torch.Tensor,
               return_sequences: bool = True, activation: str = "tanh") -> torch.Tensor:
    """Reference implementation: x [M,T,Din], W [Din,4H], U [H,4H], b [4H]. Inside
    :func:`gnnqc.ops.lstm_ref.kernel_rounding` it rounds where the HIP kernels do (numerics tests)."""
    from .lstm_ref import KernelLSTM, kernel_rounding_on
    if kernel_rounding_on() and activation == "tanh":
        return KernelLSTM.apply(x, W, U, b, bool(return_sequences), True)
    act = _ACT[activation]
    M, T, _ = x.shape
    H = U.shape[0]
    xp = torch.matmul(x, W) + b
    h = x.new_zeros(M, H)
    c = x.new_zeros(M, H)
    outs = []
    for t in range(T):
        z = xp[:, t] + h @ U
        i, f, g, o = z.split(H, dim=-1)
        i, f, o = torch.sigmoid(i), torch.sigmoid(f), torch.sigmoid(o)
        c = f * c + i * act(g)
        h = o * act(c)
        if return_sequences:
            outs.append(h)
    return torch.stack(outs, 1) if return_sequences else h


class _HipLSTM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, U, b, bf16: bool, return_sequences: bool):
        ops = _ops()
        # rows may be padded (e.g. a channel-padded producer): only unit inner stride needed
        if not (x.stride(2) == 1 and x.stride(0) == x.shape[1] * x.stride(1)):
            # (.contiguous() keeps odd strides on size-1 dims, e.g. T = 1 cut from a time-major view)
            x = x.clone(memory_format=torch.contiguous_format)
        need = any(ctx.needs_input_grad[:4])
        h, c, g = ops.lstm_fwd(x, W.contiguous(), U.contiguous(), b.contiguous(), need, bf16)
        ctx.bf16 = bf16
        ctx.return_sequences = return_sequences
        ctx.params = (W, U, b)       # leaf Parameters (for direct gradient accumulation)
        if need:
            ctx.save_for_backward(x, W, U, h, c, g)
        return h if return_sequences else h[:, -1]

    @staticmethod
    def backward(ctx, dout):
        ops = _ops()
        x, W, U, h, c, g = ctx.saved_tensors
        M, T, Din = x.shape
        H = U.shape[0]
        if ctx.return_sequences:
            dh = dout.contiguous()
        else:
            # gradient only at the last step: one constant-pad launch (not zeros + slice copy)
            dh = torch.nn.functional.pad(dout.unsqueeze(1), (0, 0, T - 1, 0))
        dz = ops.lstm_bwd(dh, g, c, U.contiguous(), ctx.bf16)
        if not ctx.bf16:
            # fp32 numerics-reference mode: exact fp32 GEMMs for the weight gradients
            dz2 = dz.reshape(M * T, 4 * H)
            dx = (dz2 @ W.t()).view(M, T, Din) if ctx.needs_input_grad[0] else None
            dW = torch.einsum("mtd,mtg->dg", x, dz) if ctx.needs_input_grad[1] else None
            dU = None
            if ctx.needs_input_grad[2]:
                dU = torch.einsum("mth,mtg->hg", h[:, :-1], dz[:, 1:]) if T > 1 else torch.zeros_like(U)
            db = dz2.sum(0) if ctx.needs_input_grad[3] else None
            return dx, dW, dU, db, None, None
        if not any(ctx.needs_input_grad[1:4]):
            # frozen weights (integrated gradients): only dx = dz W^T (bf16 dz: one HIP pass)
            dx = None
            if ctx.needs_input_grad[0]:
                if Din % 4 == 0 and Din <= 128:
                    dx = ops.lstm_dx(dz, W.contiguous(), x)
                else:
                    dx = (dz.reshape(M * T, 4 * H).float() @ W.t()).view(M, T, Din)
            return dx, None, None, None, None, None
        sinks = [_grad_sink(p) for p in ctx.params]
        need_dx = bool(ctx.needs_input_grad[0])
        Wc = W.contiguous()
        if _pipe_on(sinks, M) and _pipe_x_ok(x, W.shape[0]):
            # sequence-major recurrence (H = 128); the weight-gradient job joins the pipe
            dx = ops.lstm_dx(dz, Wc, x) if need_dx else None
            _pipe_push(_pipe_job(dz, x, h, Wc, sinks, T, 1))
            return dx, None, None, None, None, None
        with _deferred_reduce(all(d for _, d in sinks)):
            dx = ops.lstm_grads(dz, x, h, Wc, sinks[0][0], sinks[1][0], sinks[2][0], need_dx)
        return (dx if need_dx else None, *returned_grads(sinks, ctx.needs_input_grad[1:4]), None, None)


def _tm_launch(dout, x, W, U, b, h, g, c, sinks, need_dx: bool, pipe: bool, idx=None, pool: int = 0):
    """The launches of one time-major layer's backward, the route decided: through the pipe (a pool
    fused behind the layer is un-pooled first), or ONE fused kernel (recurrence, dx, weight gradients
    into ``sinks``) whose dh loads un-pool. Returns dx (the fused kernel: also when not needed)."""
    dout, Wc, Uc = dout.contiguous(), W.contiguous(), U.contiguous()
    if pipe:
        return _pipe_tm_backward(_unpool(dout, idx, pool, h.shape[0]), g, c, x, h, Wc, Uc, sinks, need_dx)
    return _ops().lstm_tm_bwd(dout, g, c, x, h, Wc, Uc, b.contiguous(), sinks[0][0], sinks[1][0], sinks[2][0],
                              need_dx, idx if pool else None, pool)


def _tm_layer_backward(dout, x, W, U, b, h, g, c, params, need_w, need_dx, idx=None, pool: int = 0):
    """Backward of one time-major layer (the pipe when it takes the layer, else one fused kernel);
    ``idx`` / ``pool``: the argmax of a pool fused behind the layer, whose pooled gradient ``dout`` then is.
    Returns dx (or None) and the three weight gradients to hand to autograd (None where they
    were accumulated directly into ``.grad``)."""
    if not any(need_w) and not need_dx:
        return None, [None, None, None]
    sinks = _layer_sinks(params, need_w, x)
    pipe = _pipe_takes(x, W, g, sinks, need_w)
    with _deferred_reduce(not pipe and any(need_w) and all(d for _, d in sinks)):
        dx = _tm_launch(dout, x, W, U, b, h, g, c, sinks, need_dx, pipe, idx, pool)
    return (dx if need_dx else None), returned_grads(sinks, need_w)


class _HipLSTMTM(torch.autograd.Function):
    """Time-major LSTM layer (``lstm_tm_fwd.hip`` / ``lstm_tm_bwd.hip``): x [T, Mp, Din] -> h [T, Mp, H] (or the last
    step [Mp, H]), optionally with a MaxPooling1D behind it in the same node. The backward is
    :func:`_tm_layer_backward`."""

    @staticmethod
    def forward(ctx, x, W, U, b, return_sequences: bool, pool: int = 0):
        x = x.contiguous()
        need = any(ctx.needs_input_grad[:4])
        sg = not recompute_gates(x, U.shape[0], any(ctx.needs_input_grad[1:4]))
        h, g, c = _ops().lstm_tm_fwd(x, W.contiguous(), U.contiguous(), b.contiguous(), need, sg)
        ctx.params = (W, U, b)
        ctx.return_sequences = return_sequences
        out, idx = _pool_out(h, pool) if (pool and return_sequences) else (h, x.new_zeros(0, dtype=torch.uint8))
        ctx.pool = int(pool) if return_sequences else 0
        if need:
            ctx.save_for_backward(x, W, U, b, h, g, c, idx)
        return out if return_sequences else h[-1]

    @staticmethod
    def backward(ctx, dout):
        x, W, U, b, h, g, c, idx = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx, grads = _tm_layer_backward(dout, x, W, U, b, h, g, c, ctx.params, need[1:4], bool(need[0]), idx, ctx.pool)
        return (dx, *grads, None, None)


class _HipLSTMTMPair(torch.autograd.Function):
    """Two stacked time-major layers A (Din -> H) and B (H -> H), both returning sequences:
    ONE wavefront-pipelined forward kernel (``lstm_tm2_fwd``); the backward runs the
    per-layer kernels (B first, its dx is A's dh). (A pipelined pair backward was measured
    slower - 148 vs 118 us for the CML H=16 pair: B's in-loop dx MFMAs and A's waves share each
    SIMD's MFMA pipe - and removed.)"""

    @staticmethod
    def forward(ctx, x, WA, UA, bA, WB, UB, bB, pool: int = 0):
        x = x.contiguous()
        need = any(ctx.needs_input_grad[:7])
        sg = not recompute_gates(x, UA.shape[0], any(ctx.needs_input_grad[1:7]))
        # (pooling by layer B's storer lanes in the same launch measured slower than the separate
        # maxpool pass - SoilNet 3.21 vs 3.11 ms, IG 4.84 vs 4.74 ms per call, profiles/r6_pool_in_fwd_ab.txt,
        # as in round 3 - so it is opt-in)
        kp = int(pool) if (pool and switch_on("GNNQC_TM_POOL_IN_FWD", False)) else 0
        hA, gA, cA, hB, gB, cB, pooled, pidx = _ops().lstm_tm2_fwd(
            x, WA.contiguous(), UA.contiguous(), bA.contiguous(), WB.contiguous(), UB.contiguous(), bB.contiguous(),
            need, sg, kp)
        ctx.params = (WA, UA, bA, WB, UB, bB)
        if kp:                            # pooled by layer B's storer lanes in the same launch
            out, idx = pooled, pidx
        else:
            out, idx = _pool_out(hB, pool) if pool else (hB, x.new_zeros(0, dtype=torch.uint8))
        ctx.pool = int(pool)
        if need:
            ctx.save_for_backward(x, WA, UA, bA, hA, gA, cA, WB, UB, bB, hB, gB, cB, idx)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, WA, UA, bA, hA, gA, cA, WB, UB, bB, hB, gB, cB, idx = ctx.saved_tensors
        need = ctx.needs_input_grad
        nA, nB, need_dx = need[1:4], need[4:7], bool(need[0])
        sB = _layer_sinks(ctx.params[3:], nB, x)
        sA = _layer_sinks(ctx.params[:3], nA, x)
        # one decision for both layers: the queue only if it takes both, else one reduce scope around both
        pipe = _pipe_takes(hA, WB, gB, sB, nB) and _pipe_takes(x, WA, gA, sA, nA)
        dx = None
        with _deferred_reduce(not pipe and all(d for _, d in sB) and all(d for _, d in sA)):
            dhA = _tm_launch(dout, hA, WB, UB, bB, hB, gB, cB, sB, True, pipe, idx, ctx.pool)
            if need_dx or any(nA):
                dx = _tm_launch(dhA, x, WA, UA, bA, hA, gA, cA, sA, need_dx, pipe)
        return (dx if need_dx else None, *returned_grads(sA, nA), *returned_grads(sB, nB), None)


def _pool_out(h: torch.Tensor, pool: int):
    """MaxPooling1D(pool) of a time-major [T, Mp, H] output inside a layer's autograd node: (pooled
    [T // pool, Mp, H], byte argmax). The node's backward then takes the pooled gradient and the
    recurrence un-pools it on load (``lstm_tm_bwd`` pidx)."""
    T, Mp, H = h.shape
    y, idx = _ops().maxpool1d_fwd(h.contiguous().view(1, T, Mp * H), int(pool))
    return y.view(T // pool, Mp, H), idx.view(T // pool, Mp, H)


def _unpool(dout: torch.Tensor, idx: torch.Tensor, pool: int, T: int) -> torch.Tensor:
    """Full-resolution gradient of a fused pool (paths whose recurrence does not un-pool on load)."""
    if not pool:
        return dout
    Ts, Mp, H = dout.shape
    return _ops().maxpool1d_bwd(dout.contiguous().view(1, Ts, Mp * H), idx.view(1, Ts, Mp * H), T,
                                int(pool)).view(T, Mp, H)


def pool_fusion() -> bool:
    """Whether a MaxPooling1D after a time-major layer (pair) runs inside that layer's autograd node
    with the un-pooling done by the recurrence's dh loads (``GNNQC_TM_POOL_FUSE=0``: separate pool)."""
    return switch_on("GNNQC_TM_POOL_FUSE")


def lstm_pair_tm(x_tm, A, B, pool: int = 0) -> torch.Tensor:
    """Fused forward of two stacked LSTM modules (``gnnqc.models.layers.LSTM``), optionally followed
    by MaxPooling1D(``pool``) in the same autograd node."""
    return _HipLSTMTMPair.apply(x_tm, A.kernel, A.recurrent_kernel, A.bias, B.kernel, B.recurrent_kernel, B.bias,
                                int(pool))


def recompute_gates(x: torch.Tensor, H: int, weight_grads: bool) -> bool:
    """Whether a time-major layer's forward saves no gates and its backward recomputes them from
    x_t and h_{t-1} (``lstm_tm_bwd_body.h`` RG: bitwise the forward's pre-activations; halves the forward's
    state stream). H in {16, 32}, 16-byte x granules, and the backward must take the fused kernel:
    frozen weights (integrated gradients), or too many sequences for the pipelined backward
    (``PIPE_MAX_SEQ``). ``GNNQC_TM_RG=0`` keeps the saved gates."""
    if not switch_on("GNNQC_TM_RG") or H not in (16, 32):
        return False
    Din = x.shape[-1]
    if Din % 4 or Din > 64 or x.data_ptr() % 16 or not x.is_contiguous():
        return False
    return (not weight_grads) or x.shape[1] > PIPE_MAX_SEQ or not _Pipe.enabled


def tm_eligible(x: torch.Tensor, H: int, Din: int, activation: str = "tanh", bf16: bool = True) -> bool:
    """Whether the time-major kernels handle this layer (GPU, bf16, tanh, H in {16, 32, 64})."""
    return (use_hip(x) and bf16 and activation == "tanh" and H in (16, 32, 64) and 1 <= Din <= 127
            and (16 * Din) // (4 if Din % 4 == 0 else (2 if Din % 2 == 0 else 1)) <= 16 * H)


def lstm_layer_tm(x_tm: torch.Tensor, W: torch.Tensor, U: torch.Tensor, b: torch.Tensor,
                  return_sequences: bool = True, pool: int = 0) -> torch.Tensor:
    """Time-major layer ``[T, Mp, Din] -> [T, Mp, H]`` (or the last step), optionally followed by
    MaxPooling1D(``pool``) in the same autograd node."""
    return _HipLSTMTM.apply(x_tm, W, U, b, bool(return_sequences), int(pool))


class _HipLSTMLast128(torch.autograd.Function):
    """An H = 128 layer returning its last state on a time-major input [T, Mp, Din] (T <= 16):
    ``time4_head.hip`` in its standalone mode (``time4_fwd`` / ``time4_bwd``: no head, compact
    saved state, workgroups looping over 16-sequence tiles). Replaces, for the time layer's last
    LSTM (time4, ``libs/create_model.py:61-79``), the sequence-major lstm_fwd<128> / lstm_bwd /
    lstm_dx kernels and the [T, Mp, C] <-> [M, T, C] copies around them. Weight gradients: the
    backward's dz through ``lstm_tm_grads`` (the training chain-head path's weight pass)."""

    @staticmethod
    def forward(ctx, x, W, U, b):
        x = x.contiguous()
        need = any(ctx.needs_input_grad[:4])
        wgrad = any(ctx.needs_input_grad[1:4])
        h, g, c = _ops().time4_fwd(x, W.contiguous(), U.contiguous(), b.contiguous(), need, wgrad)
        ctx.params = (W, U, b)
        if need:
            ctx.save_for_backward(x, W, U, g, c, h if wgrad else x.new_zeros(0))
        return h[-1] if wgrad else h

    @staticmethod
    def backward(ctx, dout):
        ops = _ops()
        x, W, U, g, c, h = ctx.saved_tensors
        need = ctx.needs_input_grad
        wgrad = any(need[1:4])
        Wc = W.contiguous()
        dz, dx = ops.time4_bwd(dout.contiguous(), x, g, c, Wc, U.contiguous(), wgrad)
        if not wgrad:
            return dx if need[0] else None, None, None, None
        sinks = [_grad_sink(p) for p in ctx.params]
        with _deferred_reduce(all(d for _, d in sinks)):
            ops.lstm_tm_grads(dz, x, h, Wc, sinks[0][0], sinks[1][0], sinks[2][0], False)
        return (dx if need[0] else None, *returned_grads(sinks, need[1:4]))


class _HipLSTMLast128Prob(torch.autograd.Function):
    """time4 (as :class:`_HipLSTMLast128`) + the FROZEN Dense head for integrated gradients:
    ``time4_prob_fwd`` returns the head's sigmoid outputs and, from the same launch,
    d prob / d h_{T-1}; the backward scales those rows by d loss / d prob and runs the time4
    recurrence (``time4_bwd`` row_scale): input gradient only (weights and head frozen)."""

    @staticmethod
    def forward(ctx, x, W, U, b, head, alphas, M):
        x = x.contiguous()
        need = bool(ctx.needs_input_grad[0])
        prob, dh, g, c = _ops().time4_prob_fwd(x, W.contiguous(), U.contiguous(), b.contiguous(),
                                               [t.contiguous() for t in head], float(alphas[0]),
                                               float(alphas[1]), int(M), need)
        if need:
            ctx.save_for_backward(x, W, U, g, c, dh)
        ctx.M = int(M)
        return prob[:M]

    @staticmethod
    def backward(ctx, dprob):
        x, W, U, g, c, dh = ctx.saved_tensors
        scale = dprob.float().contiguous()          # [M]: the rows past M get no gradient
        _, dx = _ops().time4_bwd(dh, x, g, c, W.contiguous(), U.contiguous(), False, 0, scale)
        return dx, None, None, None, None, None, None


def lstm_last128_prob_tm(x_tm: torch.Tensor, mod, head, alphas, M: int) -> torch.Tensor:
    """Sigmoid outputs [M] of LSTM module ``mod`` (H = 128, last state; see ``last128_eligible``) and
    the frozen head ``head`` = [W1, b1, W2, b2, W3, b3] with LeakyReLU slopes ``alphas``."""
    if any(t.requires_grad for t in [mod.kernel, mod.recurrent_kernel, mod.bias, *head]):
        raise ValueError("lstm_last128_prob_tm: weights must be frozen (integrated gradients)")
    return _HipLSTMLast128Prob.apply(x_tm, mod.kernel, mod.recurrent_kernel, mod.bias, tuple(head), tuple(alphas), int(M))


def last128_eligible(x: torch.Tensor, mod) -> bool:
    """Whether :class:`_HipLSTMLast128` takes LSTM module ``mod`` on time-major ``x`` [T, Mp, Din]
    (``GNNQC_T4_TM=0``: the sequence-major kernels)."""
    if not switch_on("GNNQC_T4_TM") or not use_hip(x) or x.dim() != 3:
        return False
    T, Mp, Din = x.shape
    return (mod.units == 128 and not mod.return_sequences and mod.activation == "tanh" and mod.compute_bf16
            and 1 <= T <= 16 and Mp % 16 == 0 and Din % 4 == 0 and 4 <= Din <= 64
            and mod.kernel.shape[0] <= Din and x.dtype == torch.float32)


def lstm_last128_tm(x_tm: torch.Tensor, mod) -> torch.Tensor:
    """Last state [Mp, 128] of LSTM module ``mod`` on time-major ``x_tm`` (see ``last128_eligible``)."""
    return _HipLSTMLast128.apply(x_tm, mod.kernel, mod.recurrent_kernel, mod.bias)


def lstm_layer(x: torch.Tensor, W: torch.Tensor, U: torch.Tensor, b: torch.Tensor,
               return_sequences: bool = True, activation: str = "tanh", bf16: bool = True) -> torch.Tensor:
    """Dispatch: HIP persistent kernel on GPU (tanh, H multiple of 16), eager otherwise."""
    H = U.shape[0]
    if use_hip(x) and activation == "tanh" and H % 16 == 0 and H in (16, 32, 64, 128) and x.shape[-1] <= 128:
        return _HipLSTM.apply(x, W, U, b, bool(bf16), bool(return_sequences))
    return lstm_eager(x, W, U, b, return_sequences, activation)


__all__ = ["unflagged_grad_writes", "lstm_layer", "lstm_eager", "lstm_layer_tm", "lstm_pair_tm", "lstm_chain_tm", "chain_fits", "tm_eligible",
           "chain_capacity", "chain_ctl", "check_chain", "ChainTimeoutError", "lstm_chain_head_tm",
           "lstm_last128_tm", "lstm_last128_prob_tm", "last128_eligible",
           "direct_grad_accumulation"]
