"""The network-wide SoilNet classifier with ``graph_convolution.layer: GATConv`` on the GPU: the
fused per-node GAT kernels (``csrc/kernels/gat_node.hip``) write the time-major LSTM input
(``features``), the training step is capturable and bitwise reproducible, ``engine.predict`` and the
``Predictor`` pick the route up, and integrated gradients run through the input gradient kernel."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 2
# The GAT front end itself agrees with the eager layer to ~1e-6 (tests/test_gat_node_kernels_gpu.py);
# behind it both routes run the bf16 LSTM recurrences, so logits and loss carry the tolerance of the
# chain tests, as in tests/test_gat_model_gpu.py (tests/test_cml_fused_gpu.py: 2e-3 on logits,
# 1e-4 / 1e-3 on the loss)
TOL = dict(atol=2e-3, rtol=2e-3)


@pytest.fixture(scope="module")
def soil_setup(cuda_device):
    """A 13-box SoilNet store (N = 72: two neighbour mask words, T = 33) on the device and the model
    configuration."""
    from gnnqc import config as C
    from gnnqc.data.preprocessing import create_windows_dataset
    from gnnqc.data.store import DeviceStore
    from gnnqc.data.synthetic import make_soilnet_raw
    pc = C.normalize_preproc(C.default("preprocessing_soilnet"))
    pc["timestep_before"], pc["timestep_after"] = 360, 120
    raw = make_soilnet_raw(n_boxes=13, n_time=2 * 96, seed=2)
    pc["min_date"], pc["max_date"] = str(raw.time[0]), str(raw.time[-1])
    st = DeviceStore(create_windows_dataset(pc, raw=raw), "scale_range", pc.graph, device=cuda_device)
    mc = C.default("model_soilnet")
    mc["graph_convolution"]["layer"] = "GATConv"
    assert 64 < st.n_nodes <= 128 and st.seq_len == 33 and st.n_windows >= 8 * B
    return pc, mc, st


def _model(pc, mc, dev, seed=0):
    from gnnqc.models import GATConv, GCNClassifier
    torch.manual_seed(seed)
    model = GCNClassifier(mc, pc).to(dev)
    assert isinstance(model.gcn_layer, GATConv) and not model.per_sensor
    with torch.no_grad():                  # non-trivial biases and PReLU slopes
        for p in (model.dense.bias, model.dense2.bias, model.dense_out.bias, model.gcn_layer.bias):
            p.normal_(0, 0.1)
        model.gcn_layer.prelu_alpha.uniform_(0.0, 0.3)
    return model


def test_soilnet_gat_model_takes_the_fused_route(cuda_device, soil_setup, monkeypatch):
    """features() goes through gat_node_tm into the time-major LSTM kernels: the route predicate
    holds, the eager switch turns it off, and logits and loss match the GNNQC_GAT_HIP=0 model."""
    from gnnqc.ops import gcn as G
    from gnnqc.train.loss import weighted_bce_with_logits
    pc, mc, st = soil_setup
    model = _model(pc, mc, cuda_device).eval()
    b = st.gather(torch.arange(B, device=cuda_device))
    inputs = b.model_inputs("soilnet")
    N = st.n_nodes
    assert tuple(inputs[0].shape) == (B, 33, N, 3) and (b.node_mask.sum(1) > 0).all()
    monkeypatch.delenv("GNNQC_GAT_HIP", raising=False)
    assert model._soil_gat_fused(inputs) and not model._soil_fused(inputs) and not model._fused_ok()
    h, M = G.gat_node_tm(inputs[0], inputs[1], inputs[2], model.gcn_layer)
    assert M == B * N and tuple(h.shape) == (33, (B * N + 15) // 16 * 16, 20)
    calls = []
    real = G._HipGATNodeTM.apply
    monkeypatch.setattr(G._HipGATNodeTM, "apply", staticmethod(lambda *a: calls.append(a[-2:]) or real(*a)))
    with torch.no_grad():
        z1 = model.logits(inputs)
    assert calls == [(h.shape[1], 20)], calls
    assert tuple(z1.shape) == (B, N)
    l1 = weighted_bce_with_logits(z1, b.y, b.y_mask, 1.0, 5.0)
    monkeypatch.setenv("GNNQC_GAT_HIP", "0")
    assert not model._soil_gat_fused(inputs)
    with torch.no_grad():
        z0 = model.logits(inputs)
    l0 = weighted_bce_with_logits(z0, b.y, b.y_mask, 1.0, 5.0)
    assert len(calls) == 1
    print(f"max |logit diff| {(z1 - z0).abs().max().item():.3e}  loss {l1.item():.6f} vs {l0.item():.6f}")
    torch.testing.assert_close(z1, z0, **TOL)
    torch.testing.assert_close(l1, l0, atol=1e-4, rtol=1e-3)


def _train3(pc, mc, st, rows, dev, use_graph):
    from gnnqc.ops.optim import make_optimizer
    from gnnqc.train.engine import Trainer
    model = _model(pc, mc, dev, seed=0)
    opt = make_optimizer("adam", model.parameters(), 1e-3)
    tr = Trainer(model, st, opt, {0: 1.0, 1: 5.0}, use_graph=use_graph, batch_size=B)
    assert model.train()._soil_gat_fused(st.gather(rows[0]).model_inputs("soilnet"))
    for i in range(3):
        tr.train_step(rows[i])
    torch.cuda.synchronize()
    assert (tr.graph is not None) == use_graph
    assert opt.iterations == 3 and tr.global_step == 3
    assert opt.skipped_steps == 0, "the guarded Adam rejected a step (non-finite gradient or chain timeout)"
    params = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    gat = torch.cat([p.detach().reshape(-1) for p in model.gcn_layer.parameters()])
    return params, opt.flat_p.clone(), opt.m.clone(), tr.train_metrics.sums.clone(), gat


def test_soilnet_gat_training_graph_equals_eager_bitwise(cuda_device, soil_setup, monkeypatch):
    """Three Trainer steps from one seed with the captured step graph and without it, on the HIP
    route: bitwise-equal parameters, Adam moments and metric sums in deterministic mode (the GAT
    backward sums its records in a fixed order and uses no float atomics); the guarded Adam accepts
    every step and the GAT layer's parameters move.

    (torch's NaN fill of uninitialised memory is kept off as in tests/test_gat_model_gpu.py; the
    kernels' deterministic mode itself stays on.)"""
    from gnnqc.data.store import DeviceLoader
    from gnnqc.ops import set_deterministic
    pc, mc, st = soil_setup
    monkeypatch.delenv("GNNQC_GAT_HIP", raising=False)
    rows = DeviceLoader(st, list(range(st.n_windows)), B, shuffle=True, seed=1).batch_ids()
    prev = set_deterministic(True)
    monkeypatch.setattr(torch.utils.deterministic, "fill_uninitialized_memory", False)
    try:
        a = _train3(pc, mc, st, rows, cuda_device, True)
        b = _train3(pc, mc, st, rows, cuda_device, False)
    finally:
        set_deterministic(prev)
    for x, y in zip(a, b):
        assert torch.isfinite(x).all() and torch.equal(x, y), (x - y).abs().max().item()
    model = _model(pc, mc, cuda_device, seed=0)
    fresh = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    assert a[0].numel() == fresh.numel() and not torch.equal(a[0], fresh)
    # (attn_kernel_self is left out: s_self shifts all scores of a node alike, so it reaches the softmax
    # only through leaky_relu's kink, and on these [0, 1]-scaled windows a fresh layer's scores of one
    # node all have one sign: its gradient is rounding noise below Adam's epsilon. The kernel tests
    # check da_s on scores of both signs.)
    off = 0
    for n, p in model.gcn_layer.named_parameters():
        moved = a[4][off:off + p.numel()]
        off += p.numel()
        if n != "attn_kernel_self":
            assert not torch.equal(moved, p.detach().reshape(-1)), f"gcn_layer.{n} did not train"


def test_soilnet_gat_inference_on_and_off_the_route(cuda_device, soil_setup, monkeypatch):
    """engine.predict and the Predictor (generic route, captured graphs) give the same probabilities
    with the fused GAT front end as with the eager layer."""
    from gnnqc.data.store import DeviceLoader
    from gnnqc.infer import Predictor
    from gnnqc.train.engine import predict
    pc, mc, st = soil_setup
    model = _model(pc, mc, cuda_device, seed=2).eval()
    loader = DeviceLoader(st, list(range(2 * B + 1)), B, shuffle=False)        # last batch: 1 live + 1 padding
    out = {}
    for hip in (True, False):
        monkeypatch.setenv("GNNQC_GAT_HIP", "1" if hip else "0")
        assert model._soil_gat_fused(st.gather(torch.arange(B, device=cuda_device)).model_inputs("soilnet")) == hip
        pr = Predictor(model, st, steps_per_graph=2)
        out[hip] = (predict(model, st, loader), pr.predict(loader))
        assert pr.path == "generic"
    (e1, p1), (e0, p0) = out[True], out[False]
    for got in (e1, p1, p0):
        assert got["p"].shape == e0["p"].shape == (3 * B, st.n_nodes)
        for k in set(e0) - {"p"}:
            assert np.array_equal(got[k], e0[k]), k
        print("max |p - p_eager|", np.abs(got["p"] - e0["p"]).max())
        np.testing.assert_allclose(got["p"], e0["p"], **TOL)


def test_soilnet_gat_integrated_gradients(cuda_device, soil_setup, monkeypatch):
    """Two batches through IntegratedGradients on the same target nodes: the path batches go through
    features() and gat_node_bwd_input. Attributions are finite and the completeness gap is no worse
    than the eager-layer model's on the same windows (up to 1e-5: both sum ~7e3 float32 attributions
    per sample, and the path discretisation that dominates the gap is the same)."""
    from gnnqc.ops import gcn as G
    from gnnqc.xai.ig import IntegratedGradients, completeness_gap
    pc, mc, st = soil_setup
    model = _model(pc, mc, cuda_device, seed=5).eval()
    batches = [st.gather(torch.arange(i * B, i * B + B, device=cuda_device)) for i in range(2)]
    calls = []
    real = G._HipGATNodeTM.apply
    monkeypatch.setattr(G._HipGATNodeTM, "apply", staticmethod(lambda *a: calls.append(1) or real(*a)))

    def run(hip):
        monkeypatch.setenv("GNNQC_GAT_HIP", "1" if hip else "0")
        ig = IntegratedGradients(model, "soilnet", m_steps=16)
        assert model._soil_gat_fused(batches[0].model_inputs("soilnet")) == hip
        out = []
        for b in batches:
            r = ig.attribute(b, target=b.node_mask.argmax(1))
            out.append({k: r[k].detach().clone() for k in ("grad_x", "path_pred")})
        torch.cuda.synchronize()
        return out

    got = run(True)
    n_hip = len(calls)
    ref = run(False)
    assert n_hip > 0 and len(calls) == n_hip
    for r, e in zip(got, ref):
        assert tuple(r["grad_x"].shape) == (B, 33, st.n_nodes, 3)
        assert torch.isfinite(r["grad_x"]).all() and r["grad_x"].abs().max() > 0
        gap, gap_ref = completeness_gap(r).abs().max().item(), completeness_gap(e).abs().max().item()
        print(f"completeness gap: hip {gap:.3e} eager {gap_ref:.3e}")
        assert gap <= gap_ref + 1e-5, (gap, gap_ref)
