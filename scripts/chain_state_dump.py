#!/usr/bin/env python3
"""Dump the forward chain's outputs (h, gates, c, pooled, argmax per stage) for a fixed random input
to OUT (torch.save), to diff two builds' saved state on the host. Default: the CML shape (8 tiles,
T = 181); `chain_state_dump.py T M` runs M sequences (padded to whole 16-row tiles) of T steps.

    OUT=a.pt GNNQC_HIP_LIB=<library A> python scripts/chain_state_dump.py 28 40
    OUT=b.pt GNNQC_HIP_LIB=<library B> python scripts/chain_state_dump.py 28 40
    python scripts/chain_state_dump.py --diff a.pt b.pt      # host only: every tensor bitwise equal?
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def diff(a, b):
    A, B = torch.load(a), torch.load(b)
    assert len(A) == len(B), (len(A), len(B))
    bad = 0
    for i, (u, v) in enumerate(zip(A, B)):
        same = u.shape == v.shape and torch.equal(u, v)
        bad += not same
        if not same:
            d = (u.double() - v.double()).abs().max().item() if u.shape == v.shape else float("nan")
            print(f"tensor {i} (stage {i // 5}, output {i % 5}) differs: shape {tuple(u.shape)}, max |diff| {d:.3e}")
    print(f"{len(A)} tensors, {bad} differ")
    return 1 if bad else 0


def main(argv):
    if argv and argv[0] == "--diff":
        return diff(argv[1], argv[2])
    T = int(argv[0]) if len(argv) > 0 else 181
    M = int(argv[1]) if len(argv) > 1 else 128
    Mp = (M + 15) // 16 * 16
    from gnnqc.utils.native import hip_ops
    ops = hip_ops()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    units = [16, 16, 32, 32, 64, 64]
    pools = [0, 3, 0, 3, 0, 3]
    Ws, Us, bs = [], [], []
    for i, H in enumerate(units):
        dw = 18 if i == 0 else units[i - 1]
        Ws.append(torch.randn(dw, 4 * H, device=dev) * 0.3)
        Us.append(torch.randn(H, 4 * H, device=dev) * 0.3)
        bs.append(torch.randn(4 * H, device=dev) * 0.1)
    x = torch.randn(T, Mp, 20, device=dev)
    x[..., 18:] = 0
    x[:, M:] = 0
    outs = ops.lstm_chain_fwd(x, Ws, Us, bs, pools, True)
    torch.cuda.synchronize()
    # (the buffers' scratch row T of g / c is never written: keep the T written rows only)
    keep = []
    for i, o in enumerate(outs):
        if i % 5 in (1, 2) and o.shape[0] > 1:
            o = o[:-1]
        keep.append(o.float().cpu() if o.dtype != torch.uint8 else o.cpu())
    torch.save(keep, os.environ["OUT"])
    st = ops.lstm_chain_status(x).cpu().tolist()
    print("status", st[:4])
    return 5 if st[2] != 0 else 0       # (a consumer's bounded spin timed out)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
