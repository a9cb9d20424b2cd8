"""Inference engine off the GPU: the Predictor runs the same scoring steps uncaptured with the
plain-torch forms of its two kernels, and the ``predict`` CLI command writes per-window scores."""
import argparse

import numpy as np
import pytest
import torch


@pytest.mark.parametrize("baseline", [False, True])
def test_predictor_equals_engine_predict_on_cpu(cml_windows, baseline):
    from gnnqc import config as C
    from gnnqc.data.store import DeviceLoader, DeviceStore
    from gnnqc.infer import Predictor
    from gnnqc.models import create_model
    from gnnqc.train.engine import flatten_predictions, predict
    pc, ws = cml_windows
    st = DeviceStore(ws, "rolling_median", pc.graph, device="cpu")
    torch.manual_seed(1)
    model = create_model(C.default("model_cml"), pc, baseline=baseline)
    B = 8
    loader = DeviceLoader(st, list(range(2 * B + 3)), B, shuffle=False)          # last batch: 3 live, 5 padding
    ref = predict(model, st, loader, baseline)
    pr = Predictor(model, st, baseline=baseline, steps_per_graph=2)
    got = pr.predict(loader)
    assert pr.graphed is False
    assert pr.path == ("baseline_store" if baseline else "generic")
    assert set(got) == set(ref)
    for k in ref:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, k
        assert np.array_equal(got[k], ref[k]), k
    assert (got["wid"][-5:] == -1).all() and (got["mask"][-5:] == 0).all()
    again = pr.predict(loader)                      # the first result is not a view of reused tables
    assert np.array_equal(again["p"], got["p"]) and again["p"] is not got["p"]
    f0, f1 = flatten_predictions(ref), flatten_predictions(got)
    assert np.array_equal(f0["p"], f1["p"]) and np.array_equal(f0["wid"], f1["wid"])
    assert model.training                           # the caller's mode is restored


def test_series_tm_gather_and_emit_torch_forms(cml_windows):
    """The CPU forms of the two kernels: layout, padding and cursor rules."""
    from gnnqc.data.store import CursorIds, DeviceStore
    from gnnqc.infer import predict_emit, series_tm_gather
    pc, ws = cml_windows
    st = DeviceStore(ws, "rolling_median", pc.graph, device="cpu")
    ids = torch.tensor([3, 0, 17, -1, 5])
    b = st.gather(ids)
    table = torch.stack([torch.zeros(5, dtype=torch.long), ids])
    for arg in (ids, CursorIds(table, torch.tensor([3]))):          # 3 % 2 rows -> row 1
        h, y, ym, wid = series_tm_gather(st, arg)
        assert h.shape == (st.seq_len, 16, 4)
        assert torch.equal(h[:, :5, :2], b.anom.transpose(0, 1))
        assert not h[:, 5:].any() and not h[..., 2:].any()
        assert torch.equal(y, b.y) and torch.equal(ym, b.y_mask) and torch.equal(wid, b.wid)
    z = torch.tensor([-50.0, 0.0, 50.0])
    tabs = [torch.zeros(2, 3) for _ in range(3)] + [torch.zeros(2, 3, dtype=torch.long)]
    cur = torch.zeros(1, dtype=torch.long)
    for step in range(3):
        predict_emit(z + step, True, torch.ones(3), torch.ones(3) * step, torch.arange(3) + step, *tabs, cur)
    assert int(cur) == 3                            # the step past the tables wrote nothing, and advanced
    assert torch.equal(tabs[0][1], torch.sigmoid(z + 1)) and torch.equal(tabs[3][1], torch.arange(3) + 1)
    assert torch.equal(tabs[2], torch.tensor([[0.0] * 3, [1.0] * 3]))


def test_cli_predict_writes_scores(tmp_path):
    from gnnqc.ckpt import save_model
    from gnnqc.cli.__main__ import _windows, main
    from gnnqc.cli.common import load_configs
    from gnnqc.data.store import DeviceLoader, DeviceStore
    from gnnqc.models import create_model
    from gnnqc.train.engine import flatten_predictions, predict
    common = ["--ds", "cml", "--synthetic", "--sensors", "5", "--days", "0.5", "--device", "cpu",
              "--set", "pre.batch_size=32"]
    args = argparse.Namespace(ds="cml", preproc=None, model_config=None, overrides=["pre.batch_size=32"],
                              synthetic=True, sensors=5, days=0.5, flagged=None, seed=0)
    pc, mc = load_configs(args)
    ws = _windows(args, pc)
    torch.manual_seed(4)
    model = create_model(mc, pc)
    mdir, out = str(tmp_path / "model"), str(tmp_path / "scores.npz")
    save_model(model, mdir, preproc_config=pc, keras_layout=False)
    main(["predict", *common, "--model-dir", mdir, "--split", "all", "--out", out])
    z = np.load(out)
    assert {"p", "y", "wid", "time", "group", "sensor"} <= set(z.files)
    n = len(z["p"])
    assert n == ws.n_windows and all(len(z[k]) == n for k in ("y", "wid", "time", "group", "sensor"))
    assert np.array_equal(z["wid"], np.arange(n))
    assert np.array_equal(z["time"], ws.window_dates())
    st = DeviceStore(ws, "rolling_median", pc.graph, device="cpu")
    loader = DeviceLoader(st, np.arange(ws.n_windows), 32, shuffle=False)
    ref = flatten_predictions(predict(model.eval(), st, loader))
    assert np.array_equal(z["p"], ref["p"]) and np.array_equal(z["y"], ref["y"])
