#!/usr/bin/env python
"""Network-wide SoilNet training step with ``graph_convolution.layer: GATConv``: the fused per-node
HIP front end (``csrc/kernels/gat_node.hip``) against the eager layer (``GNNQC_GAT_HIP=0``), A/B in
ONE process, with the GeneralConv step (``gcn_node.hip``) on the same data for context.

    python scripts/bench_gat_soilnet.py                # B=32, T=337, 40 boxes; prints a JSON line
    python scripts/bench_gat_soilnet.py --only hip     # the HIP route alone (for a kernel trace)

All trainers are built from the same seed on the same store and capture their step graphs up front
(the switch is read while a step is traced, so each graph keeps its route). The timed windows of
full training steps (gather, forward, backward, guarded Adam) alternate between the routes,
``--reps`` times; the medians and the ratio are reported. The eager layer builds ``[B, t, N, N, H]``
edge tensors and keeps the attention for autograd, so its windows are ``--eager-steps`` steps long
(default 8) instead of ``--steps``; the output says so. The HIP side is never shrunk. Needs a GPU.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

ROUTES = ("hip", "eager", "generalconv")


def build(args, dev, route: str, store, pc, mc_gat, mc_gcn):
    from gnnqc.data.store import DeviceLoader
    from gnnqc.models import GCNClassifier
    from gnnqc.ops.optim import make_optimizer
    from gnnqc.train.engine import Trainer
    from gnnqc.train.loss import calculate_weights
    os.environ["GNNQC_GAT_HIP"] = "0" if route == "eager" else "1"
    mc = mc_gcn if route == "generalconv" else mc_gat
    torch.manual_seed(1234)
    model = GCNClassifier(mc, pc).to(dev)
    opt = make_optimizer("adam", model.parameters(), mc.learning_rate)
    trainer = Trainer(model, store, opt, calculate_weights(mc), use_graph=not args.no_graph, batch_size=args.batch)
    rows = DeviceLoader(store, list(range(store.n_windows)), args.batch, shuffle=True, seed=44,
                        drop_last=True).batch_ids()
    trainer.prepare_graphs(rows)
    model.train()
    inputs = store.gather(rows[0]).model_inputs("soilnet")
    assert model._soil_gat_fused(inputs) == (route == "hip"), "route"
    assert model._soil_fused(inputs) == (route == "generalconv"), "route"
    trainer.train_steps(rows, 0, min(args.warmup, steps_of(args, route)))
    torch.cuda.synchronize()
    return trainer, rows


def steps_of(args, route: str) -> int:
    return args.eager_steps if route == "eager" else args.steps


def window(args, trainer, rows, route: str, start: int) -> float:
    os.environ["GNNQC_GAT_HIP"] = "0" if route == "eager" else "1"
    n = steps_of(args, route)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    trainer.train_steps(rows, start, n)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=64, help="training steps per timed window (HIP routes)")
    ap.add_argument("--eager-steps", type=int, default=8, help="training steps per timed window of the eager layer")
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7, help="timed windows per route (alternated)")
    ap.add_argument("--boxes", type=int, default=40)
    ap.add_argument("--days", type=int, default=30)
    ap.add_argument("--heads", type=int, default=1)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--only", choices=ROUTES, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_gat_soilnet.py needs a GPU")
    from gnnqc import config as C
    from gnnqc.data.preprocessing import create_windows_dataset
    from gnnqc.data.store import DeviceStore
    from gnnqc.data.synthetic import make_soilnet_raw
    dev = torch.device("cuda:0")
    pc = C.normalize_preproc(C.default("preprocessing_soilnet"))
    mc_gcn = C.default("model_soilnet")
    mc_gat = C.default("model_soilnet")
    mc_gat["graph_convolution"]["layer"] = "GATConv"
    mc_gat["graph_convolution"]["attention_heads"] = args.heads
    raw = make_soilnet_raw(n_boxes=args.boxes, n_time=args.days * 96, seed=7)
    pc["min_date"], pc["max_date"] = str(raw.time[0]), str(raw.time[-1])
    store = DeviceStore(create_windows_dataset(pc, raw=raw), "scale_range", pc.graph, device=dev)
    routes = [r for r in ROUTES if args.only in (None, r)]
    tr = {r: build(args, dev, r, store, pc, mc_gat, mc_gcn) for r in routes}
    ms = {r: [] for r in routes}
    start = args.warmup
    for _ in range(args.reps):
        for r in routes:
            ms[r].append(window(args, *tr[r], r, start))
        start += args.steps
    out = {"bench": "gat_soilnet_ab", "device": torch.cuda.get_device_name(0), "batch": args.batch,
           "T": int(store.seq_len), "N": int(store.n_nodes), "boxes": args.boxes, "heads": args.heads,
           "graphs": not args.no_graph, "windows": args.reps,
           "steps_per_window": {r: steps_of(args, r) for r in routes}}
    if "eager" in routes and args.eager_steps != args.steps:
        out["note"] = (f"the eager layer is timed on {args.eager_steps}-step windows (edge tensors [B,t,N,N,H] and the "
                       f"stored attention make its step slow); the HIP routes on {args.steps}-step windows")
    for r in routes:
        out[f"{r}_ms_per_step_median"] = round(statistics.median(ms[r]), 4)
        out[f"{r}_ms_per_step_all"] = [round(v, 4) for v in ms[r]]
        out[f"{r}_last_loss"] = float(tr[r][0].last_loss.item())
    if "hip" in routes and "eager" in routes:
        out["eager_over_hip"] = round(out["eager_ms_per_step_median"] / out["hip_ms_per_step_median"], 3)
    if "hip" in routes and "generalconv" in routes:
        out["gat_hip_over_generalconv"] = round(out["hip_ms_per_step_median"] / out["generalconv_ms_per_step_median"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
