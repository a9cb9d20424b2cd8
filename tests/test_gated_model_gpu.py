"""The CML classifier with ``graph_convolution.layer: GatedGraphConv`` on the GPU: the fused
GatedGraphConv kernels feed the time-major LSTM chain (``features``) and the headed chain
(``fused_loss``), the training step is capturable and bitwise reproducible, integrated gradients run
through the input gradient kernel, inference gives the model's own probabilities, and a NaN that
reaches the layer's weight gradients rejects the whole step."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 16
# The front end itself agrees with the eager layer to ~1e-6 (tests/test_gated_kernels_gpu.py); behind
# it both routes run the bf16 LSTM recurrences, so logits and loss carry the tolerance of the chain
# tests (tests/test_agnn_model_gpu.py: 2e-3 on logits, 1e-4 / 1e-3 on the loss)
TOL = dict(atol=2e-3, rtol=2e-3)


@pytest.fixture(scope="module")
def gated_setup(cuda_device):
    """A five-sensor CML store (N = 5, T = 181) on the device and the model configuration."""
    from gnnqc import config as C
    from gnnqc.data.preprocessing import create_windows_dataset
    from gnnqc.data.store import DeviceStore
    from gnnqc.data.synthetic import make_cml_raw
    pc = C.normalize_preproc(C.default("preprocessing_cml"))
    ws = create_windows_dataset(pc, raw=make_cml_raw(n_sensors=5, n_minutes=2 * 1440, seed=7))
    st = DeviceStore(ws, "rolling_median", pc.graph, device=cuda_device)
    mc = C.default("model_cml")
    mc["graph_convolution"]["layer"] = "GatedGraphConv"
    mc["graph_convolution"]["n_layers"] = 2
    assert st.n_nodes == 5 and st.seq_len == 181 and st.n_windows >= 4 * B
    return pc, mc, st


def _model(pc, mc, dev, seed=0):
    from gnnqc.models import GCNClassifier
    from gnnqc.models.graphconv import GatedGraphConv
    torch.manual_seed(seed)
    model = GCNClassifier(mc, pc).to(dev)
    g = model.gcn_layer
    assert isinstance(g, GatedGraphConv) and (g.in_features, g.channels, g.n_layers) == (2, 16, 2)
    with torch.no_grad():                  # non-trivial biases and PReLU slopes
        for p in (model.dense.bias, model.dense2.bias, model.dense_out.bias):
            p.normal_(0, 0.1)
        g.rnn.bias.normal_(0, 0.2)
        g.prelu_alpha.uniform_(0.05, 0.3)
    return model


def test_gated_model_takes_the_time_major_route(cuda_device, gated_setup, monkeypatch):
    """features() and fused_loss() go through gated_pool(time_major=True) into the LSTM chain / the
    headed chain: the route predicate holds and the others do not, the eager switch turns it off, and
    logits and loss match the GNNQC_GATED_HIP=0 model within the bf16 tolerance of the chain tests."""
    from gnnqc.ops import gcn as G
    pc, mc, st = gated_setup
    model = _model(pc, mc, cuda_device).eval()
    b = st.gather(torch.arange(B, device=cuda_device))
    inputs = b.model_inputs("cml")
    assert tuple(inputs[0].shape) == (B, 181, 5, 2)
    monkeypatch.delenv("GNNQC_GATED_HIP", raising=False)
    assert model._cml_gated_time_major(inputs)
    assert not model._cml_agnn_time_major(inputs) and not model._cml_edge_time_major(inputs)
    assert not model._cml_gat_time_major(inputs) and not model._cml_time_major(inputs) and not model._fused_ok()
    x, anom, adj, mask, anom_pos = inputs[:5]
    h, M = G.gated_pool(x, adj, mask, anom, anom_pos, model.gcn_layer, "mean", time_major=True)
    assert M == B and tuple(h.shape) == (181, 16, 20) and model.time_layer.head_chain_ok(h)
    calls = []
    real = G._HipGatedPool.apply
    monkeypatch.setattr(G._HipGatedPool, "apply", staticmethod(lambda *a: calls.append(a[-2:]) or real(*a)))
    with torch.no_grad():
        z1 = model.logits(inputs)
        l1, zf1 = model.fused_loss(inputs, b.y, b.y_mask, 1.0, 5.0)
    assert calls == [(16, 20), (16, 20)], calls           # both took the time-major kernel output
    monkeypatch.setenv("GNNQC_GATED_HIP", "0")
    assert not model._cml_gated_time_major(inputs)
    with torch.no_grad():
        z0 = model.logits(inputs)
        assert model.fused_loss(inputs, b.y, b.y_mask, 1.0, 5.0) is None
        from gnnqc.train.loss import weighted_bce_with_logits
        l0 = weighted_bce_with_logits(z0, b.y, b.y_mask, 1.0, 5.0)
    assert len(calls) == 2
    torch.testing.assert_close(z1, z0, **TOL)
    torch.testing.assert_close(zf1, z0, **TOL)
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
    layer = {n: p.detach().clone() for n, p in model.gcn_layer.named_parameters()}
    return (params, opt.flat_p.clone(), opt.m.clone(), tr.train_metrics.sums.clone()), layer


def test_gated_training_graph_equals_eager_bitwise(cuda_device, gated_setup, monkeypatch):
    """Three Trainer steps from one seed with the captured step graph and without it: bitwise-equal
    parameters, Adam moments and metric sums in deterministic mode (the GatedGraphConv backward sums
    its records in a fixed order and uses no float atomics); no step is skipped, and every parameter
    of the layer moved. (torch's NaN fill of uninitialised memory is kept off, as in
    tests/test_gat_model_gpu.py, which gives the reason.)"""
    from gnnqc.data.store import DeviceLoader
    from gnnqc.ops import set_deterministic
    pc, mc, st = gated_setup
    monkeypatch.delenv("GNNQC_GATED_HIP", raising=False)
    rows = DeviceLoader(st, list(range(st.n_windows)), B, shuffle=True, seed=1).batch_ids()
    prev = set_deterministic(True)
    monkeypatch.setattr(torch.utils.deterministic, "fill_uninitialized_memory", False)
    try:
        a, layer = _train3(pc, mc, st, rows, cuda_device, True)
        b, _ = _train3(pc, mc, st, rows, cuda_device, False)
    finally:
        set_deterministic(prev)
    for x, y in zip(a, b):
        assert torch.isfinite(x).all() and torch.equal(x, y), (x - y).abs().max().item()
    fresh = _model(pc, mc, cuda_device, seed=0)
    before = dict(fresh.gcn_layer.named_parameters())
    assert set(layer) == set(before) == {"kernel", "rnn.kernel", "rnn.recurrent_kernel", "rnn.bias", "prelu_alpha"}
    for n, p in layer.items():
        assert torch.isfinite(p).all() and not torch.equal(p, before[n].detach()), n


def test_gated_integrated_gradients_on_the_generic_route(cuda_device, gated_setup, monkeypatch):
    """Two batches through IntegratedGradients: the GatedGraphConv model is not on the path-folded
    GCN route, so the path batches go through features() and gated_pool_bwd_input (the zero baseline's
    first path point is the all-zero input, which the kernel tests' ``zeros`` case pins).
    Attributions are finite, agree with the eager-layer model's within the tolerance of
    tests/test_edge_model_gpu.py, and the completeness gap is finite."""
    from gnnqc.xai.ig import IntegratedGradients, completeness_gap
    pc, mc, st = gated_setup
    model = _model(pc, mc, cuda_device, seed=5).eval()
    batches = [st.gather(torch.arange(i * 8, i * 8 + 8, device=cuda_device)) for i in range(2)]

    def run(hip):
        monkeypatch.setenv("GNNQC_GATED_HIP", "1" if hip else "0")
        ig = IntegratedGradients(model, "cml", m_steps=16)
        assert not ig._cml_path_folded_ok(batches[0])
        assert model._cml_gated_time_major(batches[0].model_inputs("cml")) == hip
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
        assert np.isfinite(gap) and np.isfinite(gap_ref)
        # the two routes differ by where the LSTM stack rounds to bf16 (time-major chain against the
        # sequence-major time layer), not in the front end (float32 both ways): a gradient crosses the
        # four LSTM layers and the head input, five bf16-rounded stages of relative error 2^-8 each,
        # so 5 * 2^-8 = 2e-2 of the attributions' own scale (tests/test_edge_model_gpu.py)
        for k in ("grad_x", "grad_anom"):
            scale = e[k].abs().max().item()
            err = (r[k] - e[k]).abs().max().item()
            print(f"{k}: max |hip - eager| {err:.3e} of scale {scale:.3e}")
            assert err <= 2e-2 * scale + 1e-6, (k, err, scale)


def test_gated_inference_matches_the_model(cuda_device, gated_setup, monkeypatch):
    """engine.predict and Predictor (captured and not) give the probabilities of model.forward on the
    same windows, on the fused route."""
    from gnnqc.data.store import DeviceLoader
    from gnnqc.infer import Predictor
    from gnnqc.train.engine import predict
    pc, mc, st = gated_setup
    monkeypatch.delenv("GNNQC_GATED_HIP", raising=False)
    model = _model(pc, mc, cuda_device, seed=2).eval()
    loader = DeviceLoader(st, list(range(2 * B + 3)), B, shuffle=False)        # last batch: 3 live + 13 padding
    with torch.no_grad():
        want = np.concatenate([model(st.gather(row).model_inputs("cml")).reshape(-1).float().cpu().numpy()
                               for row in loader.batch_ids()])
    ref = predict(model, st, loader)
    pr = Predictor(model, st, steps_per_graph=2)
    got = pr.predict(loader)
    assert pr.path == "generic"
    assert ref["p"].shape == got["p"].shape == want.shape == (3 * B,)
    live = ref["mask"].reshape(-1) > 0
    assert live.sum() > 0
    for k in set(ref) - {"p"}:
        assert np.array_equal(got[k], ref[k]), k
    np.testing.assert_allclose(ref["p"][live], want[live], **TOL)
    np.testing.assert_allclose(got["p"][live], ref["p"][live], **TOL)
    assert np.isfinite(got["p"]).all() and np.isfinite(ref["p"]).all()


def test_gated_nan_in_x_rejects_whole_step(cuda_device, gated_setup, monkeypatch):
    """A NaN injected into the x the layer saved for its backward (as tests/test_flag_reject_gpu.py
    injects one into a saved activation) reaches the layer's weight gradients through
    gated_pool_bwd: the whole step is rejected - one skipped step, no parameter changes - and the
    next clean step updates again."""
    from gnnqc.ops.optim import make_optimizer
    from gnnqc.train.engine import Trainer
    pc, mc, st = gated_setup
    monkeypatch.delenv("GNNQC_GATED_HIP", raising=False)
    model = _model(pc, mc, cuda_device, seed=0)
    opt = make_optimizer("adam", model.parameters(), 1e-3)
    tr = Trainer(model, st, opt, {0: 1.0, 1: 5.0}, use_graph=False, batch_size=B)
    ids = torch.arange(B, device=cuda_device)
    tr.train_step(ids)                                      # a clean step updates
    torch.cuda.synchronize()
    assert opt.skipped_steps == 0
    hit = []

    def pack(t):
        if not hit and t.dtype == torch.float32 and t.is_cuda and tuple(t.shape) == (B, 181, 5, 2):
            t = t.clone()
            t[B // 2, 0] = float("nan")                     # (every node of one row: a valid one among them)
            hit.append(tuple(t.shape))
        return t

    before = opt.flat_p.clone()
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        tr.train_step(ids)
    torch.cuda.synchronize()
    assert hit, "the layer's saved x was not seen"
    assert opt.skipped_steps == 1, "the poisoned step must be rejected as a whole"
    assert torch.equal(opt.flat_p, before), "a rejected step changes no parameter"
    tr.train_step(ids)                                      # and training goes on
    torch.cuda.synchronize()
    assert opt.skipped_steps == 1 and not torch.equal(opt.flat_p, before)
