"""The CML classifier with ``graph_convolution.layer: EdgeConv`` on the GPU: the fused EdgeConv
kernels feed the time-major LSTM chain (``features``) and the headed chain (``fused_loss``), the
training step is capturable and bitwise reproducible, and integrated gradients run through the
input gradient kernel."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 16


@pytest.fixture(scope="module")
def edge_setup(cuda_device):
    """A five-sensor CML store (N = 5, T = 181) on the device and the model configuration."""
    from gnnqc import config as C
    from gnnqc.data.preprocessing import create_windows_dataset
    from gnnqc.data.store import DeviceStore
    from gnnqc.data.synthetic import make_cml_raw
    pc = C.normalize_preproc(C.default("preprocessing_cml"))
    ws = create_windows_dataset(pc, raw=make_cml_raw(n_sensors=5, n_minutes=2 * 1440, seed=7))
    st = DeviceStore(ws, "rolling_median", pc.graph, device=cuda_device)
    mc = C.default("model_cml")
    mc["graph_convolution"]["layer"] = "EdgeConv"
    assert st.n_nodes == 5 and st.seq_len == 181 and st.n_windows >= 4 * B
    return pc, mc, st


def _model(pc, mc, dev, seed=0):
    from gnnqc.models import EdgeConv, GCNClassifier
    torch.manual_seed(seed)
    model = GCNClassifier(mc, pc).to(dev)
    assert isinstance(model.gcn_layer, EdgeConv) and len(model.gcn_layer.hidden) == 0
    with torch.no_grad():                  # non-trivial biases and PReLU slopes
        for p in (model.dense.bias, model.dense2.bias, model.dense_out.bias, model.gcn_layer.out.bias):
            p.normal_(0, 0.1)
        model.gcn_layer.prelu_alpha.uniform_(0.0, 0.3)
    return model


def test_edge_model_takes_the_time_major_route(cuda_device, edge_setup, monkeypatch):
    """features() and fused_loss() go through edge_pool(time_major=True) into the LSTM chain / the
    headed chain: the route predicates hold, the eager switch turns them off, and logits and loss
    match the GNNQC_EDGE_HIP=0 model within the bf16 tolerance of the chain tests
    (tests/test_cml_fused_gpu.py: 2e-3 on logits, 1e-4 / 1e-3 on the loss)."""
    from gnnqc.ops import gcn as G
    pc, mc, st = edge_setup
    model = _model(pc, mc, cuda_device).eval()
    b = st.gather(torch.arange(B, device=cuda_device))
    inputs = b.model_inputs("cml")
    assert tuple(inputs[0].shape) == (B, 181, 5, 2)
    monkeypatch.delenv("GNNQC_EDGE_HIP", raising=False)
    assert model._cml_edge_time_major(inputs) and not model._cml_gat_time_major(inputs)
    assert not model._cml_time_major(inputs) and not model._fused_ok()
    x, anom, adj, mask, anom_pos = inputs[:5]
    h, M = G.edge_pool(x, adj, mask, anom, anom_pos, model.gcn_layer, "mean", time_major=True)
    assert M == B and tuple(h.shape) == (181, 16, 20) and model.time_layer.head_chain_ok(h)
    calls = []
    real = G._HipEdgePool.apply
    monkeypatch.setattr(G._HipEdgePool, "apply", staticmethod(lambda *a: calls.append(a[-2:]) or real(*a)))
    with torch.no_grad():
        z1 = model.logits(inputs)
        l1, zf1 = model.fused_loss(inputs, b.y, b.y_mask, 1.0, 5.0)
    assert calls == [(16, 20), (16, 20)], calls           # both took the time-major kernel output
    monkeypatch.setenv("GNNQC_EDGE_HIP", "0")
    assert not model._cml_edge_time_major(inputs)
    with torch.no_grad():
        z0 = model.logits(inputs)
        assert model.fused_loss(inputs, b.y, b.y_mask, 1.0, 5.0) is None
        from gnnqc.train.loss import weighted_bce_with_logits
        l0 = weighted_bce_with_logits(z0, b.y, b.y_mask, 1.0, 5.0)
    assert len(calls) == 2
    torch.testing.assert_close(z1, z0, atol=2e-3, rtol=2e-3)
    torch.testing.assert_close(zf1, z0, atol=2e-3, rtol=2e-3)
    torch.testing.assert_close(l1, l0, atol=1e-4, rtol=1e-3)


def _train3(pc, mc, st, rows, dev, use_graph):
    from gnnqc.ops.optim import make_optimizer
    from gnnqc.train.engine import Trainer
    model = _model(pc, mc, dev, seed=0)
    opt = make_optimizer("adam", model.parameters(), 1e-3)
    tr = Trainer(model, st, opt, {0: 1.0, 1: 5.0}, use_graph=use_graph, batch_size=B)
    for i in range(3):
        tr.train_step(rows[i])
    torch.cuda.synchronize()
    assert (tr.graph is not None) == use_graph
    assert opt.iterations == 3 and tr.global_step == 3
    assert opt.skipped_steps == 0, "the guarded Adam rejected a step (non-finite gradient or chain timeout)"
    params = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    return params, opt.flat_p.clone(), opt.m.clone(), tr.train_metrics.sums.clone()


def test_edge_training_graph_equals_eager_bitwise(cuda_device, edge_setup, monkeypatch):
    """Three Trainer steps from one seed with the captured step graph and without it: bitwise-equal
    parameters, Adam moments and metric sums in deterministic mode (the EdgeConv backward sums its
    records in a fixed order and uses no float atomics); every step is applied and the parameters
    moved. (torch's NaN fill of uninitialised memory is kept off, as in
    tests/test_gat_model_gpu.py, which gives the reason.)"""
    from gnnqc.data.store import DeviceLoader
    from gnnqc.ops import set_deterministic
    pc, mc, st = edge_setup
    monkeypatch.delenv("GNNQC_EDGE_HIP", raising=False)
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


def test_edge_layer_parameters_train(cuda_device, edge_setup, monkeypatch):
    """One training step changes W, bias and alpha of the EdgeConv layer (the kernels' gradients
    reach the optimiser's flat buffer through direct accumulation)."""
    from gnnqc.ops.optim import make_optimizer
    from gnnqc.train.engine import Trainer
    pc, mc, st = edge_setup
    monkeypatch.delenv("GNNQC_EDGE_HIP", raising=False)
    model = _model(pc, mc, cuda_device, seed=3)
    before = {n: p.detach().clone() for n, p in model.gcn_layer.named_parameters()}
    opt = make_optimizer("adam", model.parameters(), 1e-3)
    tr = Trainer(model, st, opt, {0: 1.0, 1: 5.0}, use_graph=False, batch_size=B)
    tr.train_step(torch.arange(B, device=cuda_device))
    torch.cuda.synchronize()
    assert set(before) == {"out.kernel", "out.bias", "prelu_alpha"}
    for n, p in model.gcn_layer.named_parameters():
        assert torch.isfinite(p).all() and not torch.equal(p.detach(), before[n]), n


def test_edge_integrated_gradients_on_the_generic_route(cuda_device, edge_setup, monkeypatch):
    """Two batches through IntegratedGradients: the EdgeConv model is not on the path-folded GCN
    route, so the path batches go through features() and the input-gradient kernel. Attributions are
    finite, agree with the eager-layer model's, and the completeness gap is no worse than the
    eager-layer model's on the same windows (up to 1e-5, the tolerance of the GAT model test: both
    sum ~1e4 float32 attributions per sample, the path discretisation that dominates the gap is the
    same)."""
    from gnnqc.xai.ig import IntegratedGradients, completeness_gap
    pc, mc, st = edge_setup
    model = _model(pc, mc, cuda_device, seed=5).eval()
    batches = [st.gather(torch.arange(i * 8, i * 8 + 8, device=cuda_device)) for i in range(2)]

    def run(hip):
        monkeypatch.setenv("GNNQC_EDGE_HIP", "1" if hip else "0")
        ig = IntegratedGradients(model, "cml", m_steps=16)
        assert not ig._cml_path_folded_ok(batches[0])
        assert model._cml_edge_time_major(batches[0].model_inputs("cml")) == hip
        out = []
        for b in batches:
            r = ig.attribute(b)
            out.append({k: r[k].detach().clone() for k in ("grad_x", "grad_anom", "path_pred")})
        torch.cuda.synchronize()
        return out

    got, ref = run(True), run(False)
    for r, e in zip(got, ref):
        assert tuple(r["grad_x"].shape) == (8, 181, 5, 2) and tuple(r["grad_anom"].shape) == (8, 181, 2)
        assert torch.isfinite(r["grad_x"]).all() and torch.isfinite(r["grad_anom"]).all()
        assert r["grad_x"].abs().max() > 0
        gap, gap_ref = completeness_gap(r).abs().max().item(), completeness_gap(e).abs().max().item()
        print(f"completeness gap: hip {gap:.3e} eager {gap_ref:.3e}")
        assert gap <= gap_ref + 1e-5, (gap, gap_ref)
        # the two routes differ by where the LSTM stack rounds to bf16 (time-major chain against the
        # sequence-major time layer), not in the front end (float32 both ways): a gradient crosses the
        # four LSTM layers and the head input, five bf16-rounded stages of relative error 2^-8 each,
        # so 5 * 2^-8 = 2e-2 of the attributions' own scale
        for k in ("grad_x", "grad_anom"):
            scale = e[k].abs().max().item()
            err = (r[k] - e[k]).abs().max().item()
            print(f"{k}: max |hip - eager| {err:.3e} of scale {scale:.3e}")
            assert err <= 2e-2 * scale + 1e-6, (k, err, scale)
