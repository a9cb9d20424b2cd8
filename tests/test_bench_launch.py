"""bench.py as the driver runs it: ``python bench.py --gpus N`` without a launcher spawns the N rank
processes itself (gloo on the CPU here), rank 0 prints ONE JSON line for the whole job, and a
launcher whose WORLD_SIZE disagrees with --gpus, or a failing rank, makes the command fail."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, timeout=600, **env):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, env=e,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)


def test_bench_spawns_ranks_and_reports_dp_line():
    r = _bench(["--gpus", "2", "--steps", "2", "--warmup", "1", "--full", "--sensors", "8", "--days", "3",
                "--cv-folds", "2", "--cv-epochs", "1"], timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout            # rank 0 only
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["warmup"] == 1
    assert out["config"]["global_batch"] == 256 and out["config"]["parallelism"] == "dp2"
    assert out["value"] > 0 and out["ms_per_step"] > 0
    ig = out["ig"]
    assert ig["n_ranks"] == 2 and ig["value"] > 0 and ig["sharding"].startswith("round-robin")
    cv = out["cv"]                              # the headline's ROC-AUC half: every fold run exactly once
    assert cv["folds"] == 2 and cv["epochs"] == 1 and cv["fold_per_rank"] is True
    for m in ("gcn", "baseline"):
        assert cv[f"{m}_folds_run"] == [0, 1]
        assert len(cv[f"{m}_fold_auc"]) == 2 and 0.0 <= cv[f"{m}_mean_auc"] <= 1.0
    assert cv["seconds"] > 0 and cv["dtype"] == "bf16"
    assert len(cv["gcn_minus_baseline_fold_auc"]) == 2 and cv["paper_parity"].startswith("unpinned")
    assert "vs_reference_gcn_auc" not in cv
    soil = out["soilnet"]                       # the headline's second dataset: throughput + its own CV
    assert soil["global_batch"] == 64 and soil["seq_len"] == 337 and soil["value"] > 0 and soil["ms_per_step"] > 0
    scv = soil["cv"]
    assert scv["folds"] == 2 and scv["fold_per_rank"] is True and "spatial_fault_frac=0.5" in scv["data"]
    for m in ("gcn", "baseline"):
        assert scv[f"{m}_folds_run"] == [0, 1] and 0.0 <= scv[f"{m}_mean_auc"] <= 1.0
    assert scv["paper_mean_auc"] == {"gcn": 0.858, "baseline": 0.816}


def test_bench_eight_ranks_cv_and_ig_cover_every_fold_once():
    """The driver's 8-GPU form rehearsed on gloo: 8 rank processes, 5 CV folds dealt over 8 ranks (3
    ranks idle), IG batches round-robin over 8 ranks, ONE JSON line, every fold run exactly once."""
    r = _bench(["--gpus", "8", "--steps", "1", "--warmup", "0", "--full", "--sensors", "8", "--days", "3",
                "--cv-folds", "5", "--cv-epochs", "1", "--cv-days", "4", "--no-soil-line"], timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 8 and out["config"]["parallelism"] == "dp8" and out["config"]["global_batch"] == 1024
    assert out["ig"]["n_ranks"] == 8 and out["ig"]["value"] > 0
    cv = out["cv"]
    assert cv["folds"] == 5 and cv["fold_per_rank"] is True
    for m in ("gcn", "baseline"):
        assert cv[f"{m}_folds_run"] == [0, 1, 2, 3, 4]
        assert len(cv[f"{m}_fold_auc"]) == 5


def test_bench_plain_run_is_lean_and_dumps_reproducible_outputs(tmp_path):
    """Without --full the line carries the headline only (no side record); --steps sets the timed
    steps (the dump's exact step counts say how many ran and that the guard rejected none); and
    --dump-outputs writes float .npy files that a second run with the same arguments reproduces
    (bit-exact on the CPU)."""
    import numpy as np
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "4", "--sensors", "8", "--days", "3"]
    outs = []
    for d in ("a", "b"):
        r = _bench([*args, "--dump-outputs", str(tmp_path / d)], timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout
        outs.append(json.loads(lines[0]))
    out = outs[0]
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["metric"].startswith("ROC-AUC (5-fold CV) + train windows/sec") and out["higher_is_better"] is True
    assert out["unit"] == "train windows/s (whole job)" and out["dtype"] == "bf16"
    assert not {"knn5", "ig", "cv", "soilnet"} & set(out)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and len(names) > 10
    assert {"loss.npy", "timed_steps.npy", "optimizer.m.npy", "optimizer.v.npy"} <= set(names)
    gpu = out["config"]["hip_graph"]
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
        total += a.nbytes
        if not gpu or n == "timed_steps.npy":
            np.testing.assert_array_equal(a, b, err_msg=n)
            continue
        # On a GPU the GCN backward adds its parameter gradients with float atomics, in an order that changes
        # from run to run. Each gradient is an fp32 sum of at most 4 windows x 181 steps x 8 nodes = 5,792
        # terms, so reordering moves it by at most n u = 5,792 x 2^-24 = 3.5e-4 of the sum of the terms'
        # magnitudes. The moments are linear (m) and quadratic (v) in the gradient, the loss and the
        # BatchNorm statistics come from the forward, which has no such sums.
        scale = float(np.abs(a).max())
        if n.startswith("optimizer."):
            np.testing.assert_allclose(a, b, rtol=0, atol=(7e-4 if n.endswith("v.npy") else 3.5e-4) * scale, err_msg=n)
        elif n == "loss.npy" or "moving" in n:
            np.testing.assert_allclose(a, b, rtol=1e-6, atol=0, err_msg=n)
        else:
            # a weight after the first Adam step is w0 - lr g / (|g| + eps'): where g is of the size of
            # the noise the step can differ by up to its whole size, lr = 5e-4 either way
            np.testing.assert_allclose(a, b, rtol=0, atol=1.05e-3, err_msg=n)
    assert total <= 64 << 20
    # 1 warm-up + 3 timed steps were attempted and applied, none rejected
    assert np.load(tmp_path / "a" / "timed_steps.npy")[:3].tolist() == [4.0, 4.0, 0.0]


def test_bench_dump_runs_from_the_seeded_state_and_restores_the_trainer(tmp_path):
    """dump_outputs in process, on the CPU (bit-exact): the dumped step starts from the seeded weights
    and ZERO Adam moments whatever the timed steps did (after one step v = (1 - b2) g^2 and
    m = (1 - b1) g, so v = 0.1 m^2 exactly where neither moment carried anything over), its batch is the
    last timed one, and afterwards the trainer holds what the timed steps left - weights, moments, step
    counts - as in a run without a dump, which is what the --full records then measure on."""
    import argparse

    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from gnnqc.parallel import dist as D
    args = argparse.Namespace(dtype="bf16", time_layer="lstm", no_graph=False, warmup=1, steps=3)
    dev = torch.device("cpu")
    pc, mc, ws = bench.train_data(args, "cml", 8, 3)

    def run(dump_dir):
        dt, trainer, loss, _ = bench.measure_train(args, "cml", pc, mc, ws, pc.graph, 4, dev, 1, 0, D, dump_dir=dump_dir)
        return trainer, loss

    t0, loss0 = run(None)
    t1, loss1 = run(str(tmp_path))
    assert loss0 == loss1 and t0.global_step == t1.global_step == 4
    assert t0.opt.iterations == t1.opt.iterations == 4 and float(t1.opt.step_t) == 4.0
    for (k, a), (_, b) in zip(t0.model.state_dict().items(), t1.model.state_dict().items()):
        assert torch.equal(a, b), k
    assert torch.equal(t0.opt.m, t1.opt.m) and torch.equal(t0.opt.v, t1.opt.v)
    m, v = np.load(tmp_path / "optimizer.m.npy"), np.load(tmp_path / "optimizer.v.npy")
    assert np.abs(m).max() > 0
    np.testing.assert_allclose(v, 0.1 * m.astype(np.float64) ** 2, rtol=1e-5, atol=1e-12)
    # the dumped step is one step on the last timed batch from the seeded model: the same thing done by hand
    from gnnqc.data.store import DeviceLoader
    loader = DeviceLoader(t0.store, list(range(ws.n_windows)), 4, shuffle=True, seed=44, rank=0, world_size=1,
                          drop_last=True)
    args0 = argparse.Namespace(**{**vars(args), "warmup": 0, "steps": 0})
    _, t2, _, _ = bench.measure_train(args0, "cml", pc, mc, ws, pc.graph, 4, dev, 1, 0, D)
    rows = loader.batch_ids()
    loss2 = float(t2.train_steps(rows, 3, 1))
    assert float(np.load(tmp_path / "loss.npy")[0]) == loss2
    for k, a in t2.model.state_dict().items():
        if a.is_floating_point():
            np.testing.assert_array_equal(np.load(tmp_path / (k + ".npy")), a.detach().float().numpy(), err_msg=k)


def test_bench_parent_never_initialises_hip():
    """The spawning parent must not call torch.cuda at all (on ROCm device_count() falls back to
    hipGetDeviceCount without amdsmi, initialising HIP in a process that then forks its ranks): run
    the parent with every such entry point poisoned; the children are fresh interpreters."""
    boot = ("import sys, runpy, torch\n"
            "def boom(*a, **k):\n"
            "    raise RuntimeError('parent touched torch.cuda')\n"
            "for name in ('device_count', '_lazy_init', 'is_available', 'init', 'set_device'):\n"
            "    setattr(torch.cuda, name, boom)\n"
            "torch._C._cuda_getDeviceCount = boom\n"
            "sys.argv = [sys.argv[1]] + sys.argv[2:]\n"
            "runpy.run_path(sys.argv[0], run_name='__main__')\n")
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, "-c", boot, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1",
                        "--warmup", "0", "--sensors", "8", "--days", "3", "--no-ig-line", "--no-cv-line",
                        "--no-knn-line", "--no-soil-line"], cwd=ROOT, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0])["n_gpus"] == 2


def test_bench_world_size_mismatch_fails():
    r = _bench(["--gpus", "2", "--steps", "1"], WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    assert r.returncode != 0
    assert "WORLD_SIZE" in r.stderr


def test_bench_failing_rank_fails_the_job():
    """Rank 1 fails right after joining the process group; rank 0 would wait in its first collective
    forever - the parent must stop it and exit with the failing rank's code."""
    r = _bench(["--gpus", "2", "--steps", "1", "--warmup", "0", "--sensors", "8", "--days", "3", "--no-soil-line"],
               timeout=300,
               GNNQC_BENCH_FAIL_RANK="1")
    assert r.returncode == 3, r.stderr[-2000:]
    assert "rank 1 exited with 3" in r.stderr
