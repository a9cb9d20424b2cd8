#!/usr/bin/env python
"""CML training step with ``graph_convolution.layer: GatedGraphConv``: the fused HIP front end
(``csrc/kernels/gated.hip``) against the eager layer (``GNNQC_GATED_HIP=0``), A/B in ONE process, for
``n_layers`` 1 and 2.

    python scripts/bench_gated.py                       # B=128, T=181, synthetic store; prints a JSON line
    python scripts/bench_gated.py --only hip --layers 2 # the HIP route alone (for a kernel trace)

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


def _set_route(hip: bool):
    os.environ["GNNQC_GATED_HIP"] = "1" if hip else "0"


def build(args, dev, hip: bool, n_layers: int, store, pc, mc):
    from gnnqc.data.store import DeviceLoader
    from gnnqc.models import GCNClassifier
    from gnnqc.ops.optim import make_optimizer
    from gnnqc.train.engine import Trainer
    from gnnqc.train.loss import calculate_weights
    mc = copy.deepcopy(mc)
    mc["graph_convolution"]["layer"] = "GatedGraphConv"
    mc["graph_convolution"]["n_layers"] = n_layers
    _set_route(hip)
    torch.manual_seed(1234)
    model = GCNClassifier(mc, pc).to(dev)
    opt = make_optimizer("adam", model.parameters(), mc.learning_rate)
    trainer = Trainer(model, store, opt, calculate_weights(mc), use_graph=not args.no_graph, batch_size=args.batch)
    rows = DeviceLoader(store, list(range(store.n_windows)), args.batch, shuffle=True, seed=44,
                        drop_last=True).batch_ids()
    trainer.prepare_graphs(rows)
    model.train()
    inputs = store.gather(rows[0]).model_inputs("cml")
    assert model._cml_gated_time_major(inputs) == hip, "route"
    trainer.train_steps(rows, 0, args.warmup)
    torch.cuda.synchronize()
    return trainer, rows


def window(args, trainer, rows, hip: bool, start: int) -> float:
    _set_route(hip)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    trainer.train_steps(rows, start, args.steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / args.steps * 1e3


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=32, help="training steps per timed window")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5, help="timed windows per route (alternated)")
    ap.add_argument("--sensors", type=int, default=23)
    ap.add_argument("--days", type=int, default=7)
    ap.add_argument("--units", type=int, default=16)
    ap.add_argument("--layers", type=int, nargs="+", default=[1, 2], help="n_layers values to time")
    ap.add_argument("--pooling", default="mean", choices=["mean", "sum", "selection"])
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--only", choices=["hip", "eager"], default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_gated.py needs a GPU")
    from gnnqc import config as C
    from gnnqc.data.preprocessing import create_windows_dataset
    from gnnqc.data.store import DeviceStore
    from gnnqc.data.synthetic import make_cml_raw
    dev = torch.device("cuda:0")
    pc = C.normalize_preproc(C.default("preprocessing_cml"))
    mc = C.default("model_cml")
    mc["graph_convolution"]["units"] = args.units
    if args.pooling == "selection":
        mc["pooling"]["type"] = "selection"
    else:
        mc["pooling"]["aggregation_type"] = args.pooling
    ws = create_windows_dataset(pc, raw=make_cml_raw(n_sensors=args.sensors, n_minutes=args.days * 1440, seed=7))
    store = DeviceStore(ws, "rolling_median", pc.graph, device=dev)
    routes = [(("hip" if hip else "eager") + f"_l{L}", hip, L) for L in args.layers for hip in (True, False)
              if args.only in (None, "hip" if hip else "eager")]
    tr = {name: build(args, dev, hip, L, store, pc, mc) for name, hip, L in routes}
    ms = {name: [] for name, _, _ in routes}
    start = args.warmup
    for _ in range(args.reps):
        for name, hip, _ in routes:
            ms[name].append(window(args, *tr[name], hip, start))
        start += args.steps
    out = {"bench": "gated_ab", "device": torch.cuda.get_device_name(0), "batch": args.batch, "T": int(store.seq_len),
           "N": int(store.n_nodes), "units": args.units, "pooling": args.pooling, "graphs": not args.no_graph,
           "steps_per_window": args.steps, "windows": args.reps}
    for name, _, _ in routes:
        out[f"{name}_ms_per_step_median"] = round(statistics.median(ms[name]), 4)
        out[f"{name}_ms_per_step_all"] = [round(v, 4) for v in ms[name]]
        out[f"{name}_last_loss"] = float(tr[name][0].last_loss.item())
    for L in args.layers:
        if f"hip_l{L}" in ms and f"eager_l{L}" in ms:
            out[f"eager_over_hip_l{L}"] = round(out[f"eager_l{L}_ms_per_step_median"]
                                                / out[f"hip_l{L}_ms_per_step_median"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
