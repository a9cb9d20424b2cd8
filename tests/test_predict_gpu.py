"""Graph-replayed inference on the GPU: the two predict.hip kernels against the existing gather and
torch, and Predictor.predict against engine.predict for the CML GCN (store-fused front end + headed
chain), the per-sensor baseline (series_tm_gather + headed chain) and the SoilNet GCN (generic)."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 40
TOL = dict(atol=2e-3, rtol=2e-3)        # headed chain vs separate kernels on logits (test_cml_fused_gpu.py:63)


def _soil_small_windows():
    from gnnqc import config as C
    from gnnqc.data.preprocessing import create_windows_dataset
    from gnnqc.data.synthetic import make_soilnet_raw
    pc = C.normalize_preproc(C.default("preprocessing_soilnet"))
    raw = make_soilnet_raw(n_boxes=6, n_time=10 * 96, seed=2)
    pc["min_date"], pc["max_date"] = str(raw.time[0]), str(raw.time[-1])
    return pc, create_windows_dataset(pc, raw=raw)


@pytest.fixture(scope="module")
def cml(cuda_device, cml_windows):
    """Store, models with non-trivial statistics / biases, the 4-batch loader (last batch: 7 live
    windows + 33 padding slots) and engine.predict's result on it, computed once."""
    from gnnqc import config as C
    from gnnqc.data.store import DeviceLoader, DeviceStore
    from gnnqc.models import BaselineClassifier, GCNClassifier
    from gnnqc.train.engine import predict
    pc, ws = cml_windows
    st = DeviceStore(ws, "rolling_median", pc.graph, device=cuda_device)
    assert st.n_windows >= 127
    torch.manual_seed(0)
    mc = C.default("model_cml")
    gcn = GCNClassifier(mc, pc).to(cuda_device)
    base = BaselineClassifier(mc, pc).to(cuda_device)
    with torch.no_grad():
        g = gcn.gcn_layer
        g.bn_gamma.uniform_(0.5, 1.5)
        g.bn_beta.normal_(0, 0.2)
        g.prelu_alpha.uniform_(0.0, 0.4)
        g.bias.normal_(0, 0.1)
        g.bn_moving_mean.normal_(0, 0.2)
        g.bn_moving_variance.uniform_(0.5, 1.5)
        for p in (gcn.dense.bias, gcn.dense2.bias, gcn.dense_out.bias, base.dense1.bias, base.dense2.bias,
                  base.dense_out.bias):
            p.normal_(0, 0.1)
    loader = DeviceLoader(st, list(range(3 * B + 7)), B, shuffle=False)
    ref = {False: predict(gcn, st, loader, False), True: predict(base, st, loader, True)}
    return {"pc": pc, "st": st, "models": {False: gcn, True: base}, "loader": loader, "ref": ref}


def _check(got, ref):
    assert set(got) == set(ref)
    for k in ref:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, (k, got[k].shape, ref[k].shape)
    for k in set(ref) - {"p"}:
        assert np.array_equal(got[k], ref[k]), k
    err = np.abs(got["p"] - ref["p"]).max()
    print("max |p - p_ref|", err)
    np.testing.assert_allclose(got["p"], ref["p"], **TOL)


def _no_spin_timeout(device):
    from gnnqc.utils.native import hip_ops
    st = hip_ops().lstm_chain_status(torch.empty(1, device=device)).cpu()
    assert int(st[2]) == 0, "a consumer spin timed out"


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("via_cursor", [False, True])
@pytest.mark.parametrize("nb", [40, 16])
def test_series_tm_gather_matches_gather(cuda_device, cml, nb, via_cursor):
    from gnnqc.data.store import CursorIds
    from gnnqc.infer import series_tm_gather
    st = cml["st"]
    ids = torch.randperm(st.n_windows, generator=torch.Generator().manual_seed(5))[:nb].to(cuda_device)
    if nb == 40:
        ids[-4:] = -1
    b = st.gather(ids)
    if via_cursor:
        rows = 3
        table = torch.stack([ids.flip(0), ids, torch.full_like(ids, -1)])
        arg = CursorIds(table.contiguous(), torch.tensor([rows + 1], device=cuda_device))      # wraps to row 1
    else:
        arg = ids
    h, y, ym, wid = series_tm_gather(st, arg)
    T, C, Mp = st.seq_len, st.n_feat, (nb + 15) // 16 * 16
    assert h.shape == (T, Mp, 4) and h.dtype == torch.float32 and h.is_contiguous()
    assert torch.equal(h[:, :nb, :C], b.anom.transpose(0, 1))
    assert not h[:, nb:].any().item() and not h[..., C:].any().item()
    assert torch.equal(y, b.y) and torch.equal(ym, b.y_mask) and torch.equal(wid, b.wid)
    assert y.shape == (nb,) and wid.dtype == torch.long
    assert h.data_ptr() % 16 == 0
    tl = cml["models"][True].time_layer
    assert tl._chain_plan(tl._sequence(), h) is not None


@pytest.mark.parametrize("shape,logits", [((40,), True), ((4, 7), False)])
def test_predict_emit_matches_torch(cuda_device, shape, logits):
    from gnnqc.infer import predict_emit
    dev = cuda_device
    gen = torch.Generator().manual_seed(9)
    R, nb = int(np.prod(shape)), shape[0]
    rows_out = 3
    tabs = [torch.full((rows_out, R), -7.0, device=dev) for _ in range(3)]
    tabs.append(torch.full((rows_out, nb), -7, dtype=torch.long, device=dev))
    cur = torch.zeros(1, dtype=torch.long, device=dev)
    steps = []
    for s in range(4):
        v = torch.randn(shape, generator=gen) * 4 if logits else torch.rand(shape, generator=gen)
        if logits:
            v[0], v[1] = 50.0, -50.0
        y = (torch.rand(shape, generator=gen) > 0.5).float()
        m = (torch.rand(shape, generator=gen) > 0.3).float()
        w = torch.randint(-1, 1000, (nb,), generator=gen)
        steps.append((v, y, m, w))
        predict_emit(v.to(dev), logits, y.to(dev), m.to(dev), w.to(dev), *tabs, cur)
    assert int(cur.item()) == 4
    p, yo, mo, wo = (t.cpu() for t in tabs)
    for s in range(3):                     # (the fourth step found the tables full: nothing written)
        v, y, m, w = steps[s]
        want = torch.sigmoid(v) if logits else v
        if logits:
            torch.testing.assert_close(p[s], want.reshape(-1), atol=1e-6, rtol=0)
            assert torch.isfinite(p[s]).all()
        else:
            assert torch.equal(p[s], want.reshape(-1))
        assert torch.equal(yo[s], y.reshape(-1)) and torch.equal(mo[s], m.reshape(-1)) and torch.equal(wo[s], w)


# ------------------------------------------------------------------ CML end to end
@pytest.mark.parametrize("baseline", [False, True])
def test_cml_predictor_matches_engine_predict(cuda_device, cml, baseline):
    from gnnqc.infer import Predictor
    st, model, loader = cml["st"], cml["models"][baseline], cml["loader"]
    pr = Predictor(model, st, baseline=baseline, steps_per_graph=3)
    got = pr.predict(loader)
    assert pr.path == ("baseline_store" if baseline else "gcn_store") and pr.graphed is True
    assert got["p"].shape == (4 * B,)
    assert (got["wid"][3 * B + 7:] == -1).all() and (got["mask"][3 * B + 7:] == 0).all()
    _check(got, cml["ref"][baseline])
    eager = Predictor(model, st, baseline=baseline, steps_per_graph=3, use_graph=False)
    un = eager.predict(loader)
    assert eager.graphed is False and eager.path == pr.path
    for k in got:
        assert np.array_equal(un[k], got[k]), k       # the same kernels on the same values
    _no_spin_timeout(cuda_device)


def test_weights_are_read_by_address(cuda_device, cml):
    from gnnqc.infer import Predictor
    from gnnqc.train.engine import predict
    st, loader = cml["st"], cml["loader"]
    model = copy.deepcopy(cml["models"][False])
    pr = Predictor(model, st, steps_per_graph=3)
    first = pr.predict(loader)
    graph = pr.graph
    with torch.no_grad():
        model.dense_out.bias.add_(1.0)
        model.gcn_layer.bn_moving_mean.add_(0.1)
    second = pr.predict(loader)
    assert pr.graph is graph and pr.graphed            # no recapture
    _check(second, predict(model, st, loader))
    live = first["mask"] > 0
    assert np.abs(second["p"] - first["p"])[live].max() > 2e-3 + 2e-3 * np.abs(first["p"][live]).max()


def test_replays_do_not_leak_state(cuda_device, cml):
    from gnnqc.data.store import DeviceLoader
    from gnnqc.infer import Predictor
    from gnnqc.train.engine import predict
    st, model, loader = cml["st"], cml["models"][False], cml["loader"]
    pr = Predictor(model, st, steps_per_graph=3)
    a = pr.predict(loader)
    b = pr.predict(loader)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    short = DeviceLoader(st, list(range(50, 50 + 2 * B - 5)), B, shuffle=False)        # 2 batches
    c = pr.predict(short)
    assert c["p"].shape == (2 * B,) and c["wid"].shape == (2 * B,)
    _check(c, predict(model, st, short))
    d = pr.predict(loader)                              # and back: recaptured for the first table shape
    for k in a:
        assert np.array_equal(a[k], d[k]), k


# ------------------------------------------------------------------ SoilNet
def test_soilnet_gcn_generic_path(cuda_device):
    from gnnqc import config as C
    from gnnqc.data.store import DeviceLoader, DeviceStore
    from gnnqc.infer import Predictor
    from gnnqc.models import GCNClassifier
    from gnnqc.train.engine import flatten_predictions, predict
    pc, ws = _soil_small_windows()
    st = DeviceStore(ws, "scale_range", pc.graph, device=cuda_device)
    torch.manual_seed(2)
    model = GCNClassifier(C.default("model_soilnet"), pc).to(cuda_device)
    nb = 4
    assert st.n_windows >= 2 * nb + 3
    loader = DeviceLoader(st, list(range(2 * nb + 3)), nb, shuffle=False)        # last batch: 3 live + 1 padding
    ref = predict(model, st, loader)
    pr = Predictor(model, st, steps_per_graph=2)
    got = pr.predict(loader)
    assert pr.path == "generic"
    assert "node" in got and got["p"].shape == (3 * nb, st.n_nodes)
    _check(got, ref)
    f0, f1 = flatten_predictions(ref), flatten_predictions(got)
    assert np.array_equal(f0["wid"], f1["wid"]) and np.array_equal(f0["node"], f1["node"])
