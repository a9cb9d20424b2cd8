#!/usr/bin/env python
"""CML training step with ``graph_convolution.layer: AGNNConv``: the fused HIP front end
(``csrc/kernels/agnn.hip``) against the eager layer (``GNNQC_AGNN_HIP=0``), A/B in ONE process, with
the EdgeConv HIP step (``csrc/kernels/edge.hip``) timed in the same call as a same-box yardstick.

    python scripts/bench_agnn.py                 # B=128, T=181, synthetic store; prints a JSON line
    python scripts/bench_agnn.py --only hip      # the HIP route alone (for a kernel trace)

The trainers are built from the same seed on the same store and capture their step graphs up front
(the switch is read while a step is traced, so each graph keeps its route). The timed windows of
``--steps`` full training steps (gather, forward, backward, guarded Adam) alternate between the
routes, ``--reps`` times; the medians and the ratios are reported. Needs a GPU.
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

ROUTES = {"hip": ("AGNNConv", True), "eager": ("AGNNConv", False), "edge_hip": ("EdgeConv", True)}


def _set_route(route):
    os.environ["GNNQC_AGNN_HIP"] = "1" if ROUTES[route][1] else "0"
    os.environ["GNNQC_EDGE_HIP"] = "1"


def build(args, dev, route, store, pc, mc):
    from gnnqc.data.store import DeviceLoader
    from gnnqc.models import GCNClassifier
    from gnnqc.ops.optim import make_optimizer
    from gnnqc.train.engine import Trainer
    from gnnqc.train.loss import calculate_weights
    layer, hip = ROUTES[route]
    mc = copy.deepcopy(mc)
    mc["graph_convolution"]["layer"] = layer
    _set_route(route)
    torch.manual_seed(1234)
    model = GCNClassifier(mc, pc).to(dev)
    opt = make_optimizer("adam", model.parameters(), mc.learning_rate)
    trainer = Trainer(model, store, opt, calculate_weights(mc), use_graph=not args.no_graph, batch_size=args.batch)
    rows = DeviceLoader(store, list(range(store.n_windows)), args.batch, shuffle=True, seed=44,
                        drop_last=True).batch_ids()
    trainer.prepare_graphs(rows)
    model.train()
    inputs = store.gather(rows[0]).model_inputs("cml")
    if layer == "AGNNConv":
        assert model._cml_agnn_time_major(inputs) == hip and not model._cml_edge_time_major(inputs), "route"
    else:
        assert model._cml_edge_time_major(inputs) and not model._cml_agnn_time_major(inputs), "route"
    trainer.train_steps(rows, 0, args.warmup)
    torch.cuda.synchronize()
    return trainer, rows


def window(args, trainer, rows, route, start: int) -> float:
    _set_route(route)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    trainer.train_steps(rows, start, args.steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / args.steps * 1e3


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=64, help="training steps per timed window")
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7, help="timed windows per route (alternated)")
    ap.add_argument("--sensors", type=int, default=23)
    ap.add_argument("--days", type=int, default=7)
    ap.add_argument("--aggregate", default="sum", choices=["sum", "mean"], help="neighbour aggregation")
    ap.add_argument("--pooling", default="mean", choices=["mean", "sum", "selection"])
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--only", choices=list(ROUTES), default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_agnn.py needs a GPU")
    from gnnqc import config as C
    from gnnqc.data.preprocessing import create_windows_dataset
    from gnnqc.data.store import DeviceStore
    from gnnqc.data.synthetic import make_cml_raw
    dev = torch.device("cuda:0")
    pc = C.normalize_preproc(C.default("preprocessing_cml"))
    mc = C.default("model_cml")
    mc["graph_convolution"]["aggregation_type"] = args.aggregate
    if args.pooling == "selection":
        mc["pooling"]["type"] = "selection"
    else:
        mc["pooling"]["aggregation_type"] = args.pooling
    ws = create_windows_dataset(pc, raw=make_cml_raw(n_sensors=args.sensors, n_minutes=args.days * 1440, seed=7))
    store = DeviceStore(ws, "rolling_median", pc.graph, device=dev)
    routes = [r for r in ROUTES if args.only in (None, r)]
    tr = {r: build(args, dev, r, store, pc, mc) for r in routes}
    ms = {r: [] for r in routes}
    start = args.warmup
    for _ in range(args.reps):
        for r in routes:
            ms[r].append(window(args, *tr[r], r, start))
        start += args.steps
    out = {"bench": "agnn_ab", "device": torch.cuda.get_device_name(0), "batch": args.batch, "T": int(store.seq_len),
           "N": int(store.n_nodes), "aggregate": args.aggregate, "pooling": args.pooling, "graphs": not args.no_graph,
           "steps_per_window": args.steps, "windows": args.reps}
    for r in routes:
        out[f"{r}_ms_per_step_median"] = round(statistics.median(ms[r]), 4)
        out[f"{r}_ms_per_step_all"] = [round(v, 4) for v in ms[r]]
        out[f"{r}_last_loss"] = float(tr[r][0].last_loss.item())
    if "hip" in routes and "eager" in routes:
        out["eager_over_hip"] = round(out["eager_ms_per_step_median"] / out["hip_ms_per_step_median"], 3)
    if "hip" in routes and "edge_hip" in routes:
        out["hip_over_edge_hip"] = round(out["hip_ms_per_step_median"] / out["edge_hip_ms_per_step_median"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
