"""Integrated gradients from a baseline other than zero on the GPU (``ig_gcn_pool_fwd_base`` /
``ig_gcn_pool_bwd_base`` on the path-folded route, ``ig_interp_base`` on the generic one, one HIP
graph per input shape and baseline kind) against the same explainer in float64 on the CPU with the
LSTM rounded where the kernels round, in the forms of ``tests/test_ig_gpu.py``.

The windows are the four of the shared CML set whose features deviate most from their own mean
over time (at least 30 windows apart): on quiet windows ``x - mean`` is too small to carry a
pre-activation across zero, and a test of the flip search needs flips."""
import copy
import os

import pytest
import torch

import test_ig_gpu as Z

pytestmark = pytest.mark.gpu

MIN_FLIP_SHARE = 0.15
M = 24
KINDS = ("mean", "random")
N_DRAWS = 2


@pytest.fixture(scope="module")
def moving_ids(cml_windows):
    """Ids of the four windows with the largest mean absolute deviation from their window mean."""
    from gnnqc.data.store import DeviceStore
    pc, ws = cml_windows
    allb = DeviceStore(ws, "rolling_median", pc.graph, device="cpu").gather(torch.arange(ws.n_windows))
    m = (allb.node_mask > 0).float()
    dev = ((allb.x - allb.x.mean(1, keepdim=True)).abs().mean((1, 3)) * m).sum(1) / m.sum(1)
    ids = []
    for i in dev.argsort(descending=True).tolist():
        if all(abs(i - j) >= 30 for j in ids):
            ids.append(i)
        if len(ids) == 4:
            break
    return torch.tensor(ids)


def _engine(model, kind, **kw):
    from gnnqc.xai.ig import IntegratedGradients
    return IntegratedGradients(model, "cml", m_steps=kw.pop("m_steps", M), baseline=kind, n_baselines=N_DRAWS, seed=9,
                               **kw)


def _batches(cuda_device, cml_windows, ids):
    from gnnqc.data.store import DeviceStore
    pc, ws = cml_windows
    b = DeviceStore(ws, "rolling_median", pc.graph, device=cuda_device).gather(ids.to(cuda_device))
    bc = DeviceStore(ws, "rolling_median", pc.graph, device="cpu").gather(ids)
    for f in ("x", "anom", "adj", "node_mask"):
        setattr(bc, f, getattr(bc, f).double())
    return b, bc


def _flip_share_fp64(ref_model, bc, base_x):
    """Share of valid (window, step, node, channel) pairs whose GCN pre-activation (eval BatchNorm,
    float64) has another sign at the path's end (x) than at its start (the baseline)."""
    g = ref_model.gcn_layer
    with torch.no_grad():
        sc = g.bn_gamma * torch.rsqrt(g.bn_moving_variance + g.eps)
        y0 = (torch.matmul(base_x, g.kernel) + g.bias - g.bn_moving_mean) * sc + g.bn_beta
        y1 = (torch.matmul(bc.x, g.kernel) + g.bias - g.bn_moving_mean) * sc + g.bn_beta
        valid = (bc.node_mask > 0)[:, None, :, None].expand_as(y1)
        flip = ((y0 > 0) != (y1 > 0)) & valid
    return flip.sum().item() / valid.sum().item()


@pytest.mark.parametrize("kind", KINDS)
def test_ig_baseline_gpu_matches_fp64_cpu(cuda_device, cml_windows, moving_ids, kind):
    """GPU (path-folded, graph replay) against the float64 CPU engine with kernel_rounding(), in the
    flipping model state; at least 15 % of the valid pairs change sign between the baseline and x."""
    from gnnqc.ops.lstm_ref import kernel_rounding
    from gnnqc.xai.ig import completeness_gap
    pc, ws = cml_windows
    model = Z._ig_model(cuda_device, pc, "flipping", seed=3)
    b, bc = _batches(cuda_device, cml_windows, moving_ids)
    ig = _engine(model, kind)
    got = ig.attribute(b)
    torch.cuda.synchronize()
    assert ig._graph is not None
    ref_model = copy.deepcopy(model).cpu().double()
    ref_ig = _engine(ref_model, kind)
    with kernel_rounding():
        ref = ref_ig.attribute(bc)
    if kind == "mean":
        shares = [_flip_share_fp64(ref_model, bc, ref["baseline_x"])]
    else:
        shares = [_flip_share_fp64(ref_model, bc, d) for d in ref_ig._draws(bc, "random")[0]]
    print(f"{kind}: flip shares {shares}")
    assert min(shares) >= MIN_FLIP_SHARE, shares
    Z._assert_ig_close(got, ref)
    for k in ("baseline_x", "baseline_anom", "baseline_pred"):
        a, r = got[k].double().cpu(), ref[k]
        assert (a - r).norm().item() <= 6e-3 * r.norm().item() + 1e-6, k
    assert torch.equal(got["baseline_pred"], got["path_pred"][0])
    gap_g = completeness_gap(got).abs().cpu().double()
    gap_r = completeness_gap(ref).abs()
    span = (ref["path_pred"][-1] - ref["path_pred"][0]).abs()
    assert bool((gap_g <= gap_r + 0.05 * span + 2e-3).all()), (gap_g, gap_r, span)


@pytest.mark.parametrize("kind", KINDS + ("explicit",))
def test_ig_baseline_path_folded_matches_generic_route(cuda_device, cml_windows, moving_ids, kind, monkeypatch):
    """The _base kernels (baseline folded into the GCN kernels) == the generic route over kk x B
    copies interpolated by ig_interp_base, with several path chunks (max_rows < (m + 1) B), in the
    form of test_ig_path_folded_gcn_matches_replicated_path."""
    from gnnqc.xai.ig import IntegratedGradients
    pc, ws = cml_windows
    model = Z._ig_model(cuda_device, pc, "flipping", seed=5)
    b, _ = _batches(cuda_device, cml_windows, moving_ids)
    base = None
    if kind == "explicit":
        gen = torch.Generator().manual_seed(3)
        live = (b.node_mask > 0).float()[:, None, :, None]
        base = ((0.5 * torch.randn(b.x.shape, generator=gen)).to(cuda_device) * live,
                (0.5 * torch.randn(b.anom.shape, generator=gen)).to(cuda_device))
    kw = dict(m_steps=30, max_rows=4 * 8, use_graph=False)
    names = []

    def run():
        import gnnqc.xai.ig as I
        ops = I._ops()

        class Spy:
            def __getattr__(self, name):
                names.append(name)
                return getattr(ops, name)

        monkeypatch.setattr(I, "_ops", lambda: Spy())
        try:
            return _engine(model, "zero" if kind == "explicit" else kind, **kw).attribute(b, baselines=base)
        finally:
            monkeypatch.setattr(I, "_ops", lambda: ops)

    got = run()
    assert "ig_gcn_pool_fwd_base" in names and "ig_gcn_pool_bwd_base" in names
    assert "ig_gcn_pool_fwd" not in names and "ig_interp_base" not in names
    del names[:]
    monkeypatch.setattr(IntegratedGradients, "_cml_path_folded_ok", lambda self, batch: False)
    ref = run()
    torch.cuda.synchronize()
    assert "ig_interp_base" in names and "ig_interp" not in names and not any("gcn_pool_fwd" in n for n in names)
    for k in ("grad_x", "grad_anom", "pred", "path_pred", "baseline_pred"):
        err = (got[k] - ref[k]).abs().max().item()
        scale = ref[k].abs().max().item()
        assert err <= 1e-4 * scale + 1e-7, (k, err, scale)


def test_zero_baseline_calls_the_zero_baseline_ops(cuda_device, cml_windows, moving_ids, monkeypatch):
    """baseline="zero" launches the ops it launched before the baseline ops existed, none of them."""
    import gnnqc.xai.ig as I
    pc, ws = cml_windows
    model = Z._ig_model(cuda_device, pc, "flipping", seed=5)
    b, _ = _batches(cuda_device, cml_windows, moving_ids)
    ops, names = I._ops(), []

    class Spy:
        def __getattr__(self, name):
            names.append(name)
            return getattr(ops, name)

    monkeypatch.setattr(I, "_ops", lambda: Spy())
    res = _engine(model, "zero", use_graph=False).attribute(b)
    torch.cuda.synchronize()
    assert names == ["gcn_prep", "ig_gcn_pool_fwd", "ig_gcn_pool_bwd", "ig_finalize", "ig_finalize"], names
    assert "baseline_x" not in res and torch.equal(res["baseline_pred"], res["path_pred"][0])


@pytest.mark.parametrize("kind", KINDS + ("explicit",))
def test_ig_baseline_graph_replay(cuda_device, cml_windows, moving_ids, kind):
    """Graph replay equals eager; a second batch replayed through the same graph gives that batch's
    own result; graphed B1, a non-graphed call of another shape (it replaces the engine's cached
    backward seed), graphed B1 again reproduces the first result bit for bit."""
    pc, ws = cml_windows
    model = Z._ig_model(cuda_device, pc, "flipping", seed=7)
    b1, _ = _batches(cuda_device, cml_windows, moving_ids[:3])
    b2, _ = _batches(cuda_device, cml_windows, moving_ids[1:] + 7)
    b3, _ = _batches(cuda_device, cml_windows, moving_ids[:2] + 3)

    def base(b, seed):
        if kind != "explicit":
            return None
        gen = torch.Generator().manual_seed(seed)
        live = (b.node_mask > 0).float()[:, None, :, None]
        return ((0.5 * torch.randn(b.x.shape, generator=gen)).to(cuda_device) * live,
                (0.5 * torch.randn(b.anom.shape, generator=gen)).to(cuda_device))

    k0 = "zero" if kind == "explicit" else kind
    ig = _engine(model, k0, m_steps=20)
    eager = _engine(model, k0, m_steps=20, use_graph=False)
    first = ig.attribute(b1, baselines=base(b1, 1))
    rec = ig._graph
    assert rec is not None and kind in rec[0]
    for b, seed, got in ((b1, 1, first), (b2, 2, ig.attribute(b2, baselines=base(b2, 2)))):
        assert ig._graph is rec                               # one capture, replayed
        ref = eager.attribute(b, baselines=base(b, seed))
        torch.cuda.synchronize()
        for k in ("grad_x", "grad_anom", "pred", "path_pred", "baseline_pred", "baseline_x", "baseline_anom"):
            err = (got[k] - ref[k]).abs().max().item()
            assert err <= 1e-5 * ref[k].abs().max().item() + 1e-7, (k, err)
    # a non-graphed call of another shape on the same engine (a given target goes the eager way)
    other = ig.attribute(b3, target=torch.zeros(2, dtype=torch.long, device=cuda_device), baselines=base(b3, 3))
    assert ig._graph is rec and other["grad_x"].shape[0] == 2
    again = ig.attribute(b1, baselines=base(b1, 1))
    torch.cuda.synchronize()
    for k in ("grad_x", "grad_anom", "pred", "path_pred"):
        assert torch.equal(again[k], first[k]), k
    # the zero baseline has a graph of its own (the capture key names the kind)
    z = _engine(model, "zero", m_steps=20)
    z.attribute(b1)
    assert z._graph[0] != rec[0] and not any(isinstance(e, str) and e in KINDS + ("explicit",) for e in z._graph[0])


def test_explainer_run_with_mean_baseline(cuda_device, cml_windows, tmp_path):
    """One explainer run with ``baseline: mean`` writes baseline_features_unwrapped_* and
    baseline_anom_ts_unwrapped_* per sample, and otherwise the files of a zero-baseline run."""
    import numpy as np
    from gnnqc import config as C
    from gnnqc.ckpt import save_model
    from gnnqc.xai.ig import IntegratedGradientsExplainer
    pc, ws = cml_windows
    mc = C.default("model_cml")
    model = Z._ig_model(cuda_device, pc, "flipping", seed=1)
    mdir = str(tmp_path / "model")
    save_model(model, mdir, preproc_config=pc)
    mc["model_path"] = mdir
    pc2 = C.Config(dict(pc))
    pc2["batch_size"] = 8
    kinds = {}
    for baseline in ("zero", "mean"):
        xc = C.default("xai_ig")
        xc["output_dir"] = str(tmp_path / baseline)
        ig = xc.integrated_gradients
        ig["m_steps"], ig["dataset"], ig["threshold"], ig["baseline"] = 4, "all", 0.5, baseline
        ex = IntegratedGradientsExplainer(pc2, mc, xc, windows=ws, device=cuda_device)
        ex.prepare_data()
        ex.sample_ids = ex.sample_ids[:8]
        res = ex.get_gradients()
        assert len(res) == 8
        per_sample = []
        for r in res:
            stem = r["file_stem"]
            per_sample.append({f[:-len(f"_{stem}.npy")] for f in os.listdir(r["dir"]) if f.endswith(".npy")})
        assert all(s == per_sample[0] for s in per_sample)
        kinds[baseline] = (per_sample[0], res)
    new = {"baseline_features_unwrapped", "baseline_anom_ts_unwrapped"}
    assert kinds["mean"][0] == kinds["zero"][0] | new and not (kinds["zero"][0] & new)
    r = kinds["mean"][1][0]
    load = lambda k: np.load(os.path.join(r["dir"], f"{k}_{r['file_stem']}.npy"))      # noqa: E731
    bf, f, ba, a = (load(k) for k in ("baseline_features_unwrapped", "features_unwrapped",
                                       "baseline_anom_ts_unwrapped", "anom_ts_unwrapped"))
    assert bf.shape == f.shape and ba.shape == a.shape
    np.testing.assert_allclose(bf, np.broadcast_to(f.mean(1, keepdims=True), f.shape), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(ba, np.broadcast_to(a.mean(0, keepdims=True), a.shape), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("which", ["cml_baseline_model", "gcn_units_64"])
def test_random_baseline_generic_route_odd_batch(cuda_device, cml_windows, moving_ids, which):
    """The random baseline on the generic route (ig_interp_base over draws cut from the stacked
    draws) with three windows: 3 x 181 x 2 elements of the flagged series are no multiple of 4, so
    every odd draw starts off a 16-byte boundary. The CML baseline model, and the CML GCN at a
    shape the path-folded kernels refuse, against the float64 CPU engine in the 6e-3 form."""
    from gnnqc import config as C
    from gnnqc.models import create_model
    from gnnqc.ops.lstm_ref import kernel_rounding
    pc, ws = cml_windows
    if which == "cml_baseline_model":
        torch.manual_seed(4)
        model = create_model(C.default("model_cml"), pc, baseline=True).to(cuda_device)
        with torch.no_grad():
            model.dense_out.bias.fill_(0.3)
    else:
        mc = C.default("model_cml")
        mc["graph_convolution"]["units"] = 64
        model = Z._ig_model(cuda_device, pc, "flipping", mc=mc, seed=4)
    b, bc = _batches(cuda_device, cml_windows, moving_ids[:3])
    assert b.anom.numel() % 4 != 0
    ig = _engine(model, "random", m_steps=16)
    model.eval()
    assert not ig._cml_path_folded_ok(b)
    draws = ig._draws(b, "random")
    assert any(d[i].data_ptr() % 16 for d in draws for i in range(N_DRAWS))
    got = ig.attribute(b)
    torch.cuda.synchronize()
    ref_model = copy.deepcopy(model).cpu().double()
    with kernel_rounding():
        ref = _engine(ref_model, "random", m_steps=16).attribute(bc)
    keys = [k for k in ("grad_x", "grad_anom", "pred", "path_pred", "baseline_x", "baseline_anom", "baseline_pred")
            if k in ref]
    assert "grad_anom" in keys and ("grad_x" in keys) == (which == "gcn_units_64")
    for k in keys:
        a, r = got[k].double().cpu(), ref[k].double()
        err, scale = (a - r).norm().item(), r.norm().item()
        assert err <= 6e-3 * scale + 1e-6, (k, err, scale)
