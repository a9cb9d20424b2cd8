"""Float64 model of the chain forward (``lstm_chain_fwd.hip``) that rounds where the kernel rounds, stage by
stage, with everything the kernel stores: per stage h, the gates (bf16-rounded, as packed), c, the
MaxPooling1D(3) output that feeds the next stage (or leaves the chain) and its first-maximum argmax.

``mutant`` names one scheduling defect of a pipelined step (what the kernel would compute if a buffer
index or a publishing lag were off by one); the tests use them to show that their bounds tell such
a defect from rounding:

    x_next          x_{t+1} fed in place of x_t
    xbuf_mod2       x staged two steps ahead into three buffers, the written buffer indexed modulo 2
    publish_late    the stored h / gates / c one step late (row t holds step t - 1)
    drop_last_two   the last two steps never stored
    pool_wrong_buf  the pooled output taken from the other h buffer (h_{t-1} for h_t)
"""
from __future__ import annotations

import torch

from .lstm_ref import _bf, _same

MUTANTS = ("x_next", "xbuf_mod2", "publish_late", "drop_last_two", "pool_wrong_buf")


def _x_sequence(x: torch.Tensor, mutant: str | None) -> torch.Tensor:
    """The x_t each step reads, [M, T, D]."""
    T = x.shape[1]
    if mutant == "x_next":
        return torch.cat([x[:, 1:], x[:, -1:]], 1)
    if mutant == "xbuf_mod2":
        # x_0, x_1 staged up front, x_{t+2} during step t: written to slot (index mod 2), read from
        # slot (index mod 3) - slot 2 is never written
        slots = [torch.zeros_like(x[:, 0]) for _ in range(3)]
        for k in range(min(2, T)):
            slots[k % 2] = x[:, k]
        out = []
        for t in range(T):
            out.append(slots[t % 3])
            if t + 2 < T:
                slots[(t + 2) % 2] = x[:, t + 2]
        return torch.stack(out, 1)
    return x


def lstm_stage_ref(x, W, U, b, rounding=True, mutant=None):
    """One layer: x [M, T, D], W [Dw, 4H] (Dw <= D: further channels are padding), U [H, 4H], b [4H]
    -> h [M, T, H], gates [M, T, H, 4] (i, f, g, o), c [M, T, H], all float64."""
    r = _bf if rounding else _same
    M, T, _ = x.shape
    H, Dw = U.shape[0], W.shape[0]
    xp = r(_x_sequence(x, mutant)[..., :Dw]) @ r(W) + b
    Ur = r(U)
    h = x.new_zeros(M, H)
    c = x.new_zeros(M, H)
    hs, gs, cs = [], [], []
    for t in range(T):
        z = xp[:, t] + r(h) @ Ur
        i, f, g, o = z.split(H, dim=-1)
        i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
        c = f * c + i * g
        h = o * torch.tanh(c)
        hs.append(h)
        cs.append(c)
        gs.append(torch.stack([i, f, g, o], -1))
    h, g, c = torch.stack(hs, 1), torch.stack(gs, 1), torch.stack(cs, 1)
    if rounding:
        g = _bf(g)                              # the kernel packs the gates as bf16
    if mutant == "publish_late":
        h, g, c = (torch.cat([torch.zeros_like(v[:, :1]), v[:, :-1]], 1) for v in (h, g, c))
    elif mutant == "drop_last_two":
        h, g, c = (torch.cat([v[:, :-2], torch.zeros_like(v[:, -2:])], 1) for v in (h, g, c))
    return h, g, c


def maxpool3_ref(h, mutant=None):
    """MaxPooling1D(3), valid: h [M, T, H] -> pooled [M, T // 3, H], argmax (first maximum) uint8."""
    if mutant == "pool_wrong_buf":
        h = torch.cat([torch.zeros_like(h[:, :1]), h[:, :-1]], 1)
    M, T, H = h.shape
    w = h[:, : T // 3 * 3].reshape(M, T // 3, 3, H)
    m = w.max(2).values
    one, two = torch.ones_like(m, dtype=torch.uint8), torch.full_like(m, 2, dtype=torch.uint8)
    first = torch.where(w[:, :, 0] == m, torch.zeros_like(one), torch.where(w[:, :, 1] == m, one, two))
    return m, first


def chain_fwd_ref(x, Ws, Us, bs, pools, rounding=True, mutant=None, mutant_stage=0):
    """The whole stack: x [M, T, D]; per stage a dict h, g, c, pooled, idx (pooled / idx None without a
    pool behind the stage). The next stage reads the pooled output (or h). ``mutant`` applies to
    stage ``mutant_stage`` only."""
    out = []
    for s, (W, U, b, P) in enumerate(zip(Ws, Us, bs, pools)):
        mu = mutant if s == mutant_stage else None
        h, g, c = lstm_stage_ref(x, W, U, b, rounding, mu if mu != "pool_wrong_buf" else None)
        pooled = idx = None
        if P:
            pooled, idx = maxpool3_ref(h, mu)
        out.append({"h": h, "g": g, "c": c, "pooled": pooled, "idx": idx})
        x = pooled if P else h
    return out


__all__ = ["MUTANTS", "chain_fwd_ref", "lstm_stage_ref", "maxpool3_ref"]
