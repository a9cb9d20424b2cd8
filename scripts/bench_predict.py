#!/usr/bin/env python3
"""Inference throughput: ``engine.predict`` (eager loop) vs ``gnnqc.infer.Predictor`` (graph replay).

    python scripts/bench_predict.py [--repeats 5] [--out profiles/predict_throughput.json]
    python scripts/bench_predict.py --trace --passes 3            (Predictor CML GCN passes only: kernel trace runs)

Data of ``bench.py``'s training measurement (synthetic CML 23 links x 28 days, seed 7, B = 128,
bf16; SoilNet 40 boxes x 89 days at the config batch size as context), random-init weights. One
run = every window of the set, ids -> probabilities on the host, ending in a synchronise. In one
process the two paths alternate; after a warm-up of both, each of ``--repeats`` timed windows of a
path repeats the run until it lasted ``--min-seconds``. Prints one JSON line (and writes it to
``--out``): per model and path windows/s and ms/batch at the median, min / median / max over the
repeats, the Predictor's speed-up over the eager loop (ratio of medians) and the ratio to the
reference's Keras ``predict()`` rates (GCN 350, baseline 3657 windows/s).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REFERENCE_WPS = {"cml_gcn": 350.0, "cml_baseline": 3657.0}


def setup(name, dev, sensors=None, days=None):
    from gnnqc import config as C
    from gnnqc.data.preprocessing import create_windows_dataset
    from gnnqc.data.store import DeviceLoader, DeviceStore
    from gnnqc.data.synthetic import make_cml_raw, make_soilnet_raw
    from gnnqc.models import BaselineClassifier, GCNClassifier
    ds = "soilnet" if name.startswith("soilnet") else "cml"
    baseline = name.endswith("baseline")
    pc = C.normalize_preproc(C.default(f"preprocessing_{ds}"))
    mc = C.default(f"model_{ds}")
    mc.runtime.compute_dtype = "bf16"
    if ds == "soilnet":
        raw = make_soilnet_raw(n_boxes=sensors or 40, n_time=int((days or 89) * 96), seed=7)
        pc["min_date"], pc["max_date"] = str(raw.time[0]), str(raw.time[-1])
        batch = int(pc["batch_size"])
    else:
        raw = make_cml_raw(n_sensors=sensors or 23, n_minutes=int((days or 28) * 1440), seed=7)
        batch = 128
    ws = create_windows_dataset(pc, raw=raw)
    store = DeviceStore(ws, "scale_range" if ds == "soilnet" else "rolling_median", pc.graph, device=dev)
    loader = DeviceLoader(store, list(range(ws.n_windows)), batch, shuffle=False)
    torch.manual_seed(1234)
    model = (BaselineClassifier if baseline else GCNClassifier)(mc, pc).to(dev).eval()
    return model, store, loader, baseline


def sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def timed(fn, dev, min_seconds):
    """Seconds per run: the run repeated until the window lasted ``min_seconds``."""
    sync(dev)
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        sync(dev)
        n += 1
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            return dt / n


def measure(name, dev, args):
    from gnnqc.infer import Predictor
    from gnnqc.train.engine import predict
    model, store, loader, baseline = setup(name, dev, args.sensors, args.days)
    pr = Predictor(model, store, baseline=baseline, steps_per_graph=args.steps_per_graph)
    paths = {"eager": lambda: predict(model, store, loader, baseline),
             "predictor": lambda: pr.predict(loader)}
    for _ in range(args.warmup):
        for fn in paths.values():
            fn()
    a, b = paths["eager"](), paths["predictor"]()
    live = a["mask"] > 0
    max_dp = float(abs(a["p"] - b["p"])[live].max())
    same_rows = bool((a["wid"] == b["wid"]).all() and (a["y"] == b["y"]).all())
    secs = {k: [] for k in paths}
    for _ in range(args.repeats):
        for k, fn in paths.items():                   # alternating, in one process
            secs[k].append(timed(fn, dev, args.min_seconds))
    n, nb = store.n_windows, len(loader)
    out = {"n_windows": n, "batch": loader.batch_size, "n_batches": nb, "predictor_path": pr.path,
           "graphed": bool(pr.graphed), "steps_per_graph": pr.steps_per_graph, "max_abs_dp_vs_eager": max_dp,
           "rows_equal": same_rows}
    for k, s in secs.items():
        med = statistics.median(s)
        out[k] = {"windows_per_s": round(n / med, 1), "ms_per_batch": round(1e3 * med / nb, 4), "n_windows": n,
                  "windows_per_s_min": round(n / max(s), 1), "windows_per_s_median": round(n / med, 1),
                  "windows_per_s_max": round(n / min(s), 1), "seconds_per_pass": [round(v, 5) for v in s]}
    out["speedup_vs_eager"] = round(statistics.median(secs["eager"]) / statistics.median(secs["predictor"]), 3)
    if name in REFERENCE_WPS:
        out["vs_reference"] = {k: round(out[k]["windows_per_s"] / REFERENCE_WPS[name], 2) for k in paths}
        out["reference_windows_per_s"] = REFERENCE_WPS[name]
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="cml_gcn,cml_baseline,soilnet_gcn")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--steps-per-graph", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_throughput.json"))
    ap.add_argument("--trace", action="store_true", help="only Predictor passes of the CML GCN (kernel trace runs)")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--sensors", type=int, default=None)
    ap.add_argument("--days", type=float, default=None)
    ap.add_argument("--allow-cpu", action="store_true", help="rehearsal of the script's logic: nothing is written")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available() and not args.allow_cpu:
        raise SystemExit("bench_predict: no GPU; a CPU timing says nothing about the MI355X (--allow-cpu rehearses)")
    dev = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
    if args.trace:
        from gnnqc.infer import Predictor
        name = "cml_gcn"
        model, store, loader, baseline = setup(name, dev, args.sensors, args.days)
        pr = Predictor(model, store, baseline=baseline, steps_per_graph=args.steps_per_graph)
        for _ in range(args.passes):
            pr.predict(loader)
        sync(dev)
        print(json.dumps({"trace": name, "passes": args.passes, "n_batches": len(loader), "path": pr.path,
                          "graphed": bool(pr.graphed)}), flush=True)
        return
    res = {"metric": "inference windows/s, ids -> host probabilities (one pass over every window)",
           "device": torch.cuda.get_device_name(0) if dev.type == "cuda" else "cpu (rehearsal, not a measurement)",
           "dtype": "bf16", "repeats": args.repeats, "min_seconds_per_timed_window": args.min_seconds,
           "data": ("synthetic CML 23 links x 28 days / SoilNet 40 boxes x 89 days, seed 7, random init"
                    if args.sensors is None and args.days is None else
                    f"synthetic, --sensors {args.sensors} --days {args.days}, seed 7, random init")}
    for name in args.models.split(","):
        res[name] = measure(name, dev, args)
    line = json.dumps(res)
    print(line, flush=True)
    if dev.type == "cuda" and args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
