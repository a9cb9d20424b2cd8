"""Integrated gradients from a baseline other than zero (``gnnqc.xai.ig``), in float64 on the CPU:
the CML GCN, the CML baseline model and the SoilNet GCN, each from the ``mean`` baseline, the
``random`` baseline and an explicit pair, against a plain loop over the path points (one forward
and one backward per alpha, the trapezoid mean of the gradients, then ``(x - b) * mean``).

``m_steps`` is a power of two throughout: the engine builds its trapezoid weights in float32
(``1 / m_steps`` is then exact), so the comparison to 1e-10 relative is one of the path, not of that
constant."""
import pytest
import torch

from gnnqc import config as C
from gnnqc.data.preprocessing import create_windows_dataset
from gnnqc.data.store import DeviceStore
from gnnqc.data.synthetic import make_cml_raw, make_soilnet_raw
from gnnqc.models import create_model
from gnnqc.xai.ig import IntegratedGradients, completeness_gap

KINDS = ("mean", "random", "explicit")
MODELS = ("cml_gcn", "cml_baseline", "soilnet_gcn")
N_DRAWS = 2


def _double(batch):
    for f in ("x", "anom", "adj", "node_mask"):
        if getattr(batch, f) is not None:
            setattr(batch, f, getattr(batch, f).double())
    return batch


@pytest.fixture(scope="module")
def setups():
    """(model, ds_type, batch) per model kind, float64, output layer scaled so the scores move."""
    out = {}
    pc = C.normalize_preproc(C.default("preprocessing_cml"))
    ws = create_windows_dataset(pc, raw=make_cml_raw(n_sensors=8, n_minutes=2 * 1440, seed=5))
    store = DeviceStore(ws, "rolling_median", pc.graph)
    for name, base in (("cml_gcn", False), ("cml_baseline", True)):
        torch.manual_seed(1)
        model = create_model(C.default("model_cml"), pc, baseline=base)
        with torch.no_grad():
            model.dense_out.kernel.mul_(40.0)
            if not base:                      # GCN pre-activations that change sign inside a path
                g = model.gcn_layer
                g.bias.normal_(0, 0.3)
                g.bn_moving_mean.normal_(0, 0.3)
                g.prelu_alpha.copy_(torch.tensor([0.0, -0.3, 1.0, 1.7, 0.25])[torch.arange(g.kernel.shape[1]) % 5])
        out[name] = (model.double().eval(), "cml", _double(store.gather(torch.tensor([0, 21]))))
    ps = C.normalize_preproc(C.default("preprocessing_soilnet"))
    ps["timestep_before"], ps["timestep_after"] = 360, 60         # T = 29 survives three pool-3 stages
    ps = C.normalize_preproc(ps)
    wss = create_windows_dataset(ps, raw=make_soilnet_raw(n_boxes=4, n_time=6 * 96, seed=2))
    torch.manual_seed(0)
    model = create_model(C.default("model_soilnet"), ps)
    with torch.no_grad():
        model.dense_out.kernel.mul_(40.0)
    out["soilnet_gcn"] = (model.double().eval(), "soilnet",
                          _double(DeviceStore(wss, "scale_range", ps.graph).gather(torch.arange(3))))
    return out


def _vals(ig, batch):
    return ig._split(batch)[0]


def _explicit_pair(batch):
    gen = torch.Generator().manual_seed(77)
    xb = 0.5 * torch.randn(batch.x.shape, generator=gen, dtype=torch.float64) * (batch.node_mask > 0)[:, None, :, None]
    ab = None if batch.anom is None else 0.5 * torch.randn(batch.anom.shape, generator=gen, dtype=torch.float64)
    return xb, ab


def _engine(model, ds, kind, m, **kw):
    return IntegratedGradients(model, ds, m_steps=m, baseline="zero" if kind == "explicit" else kind,
                               n_baselines=N_DRAWS, seed=5, **kw)


def _attribute(ig, batch, kind):
    return ig.attribute(batch, baselines=_explicit_pair(batch) if kind == "explicit" else None)


def _loop(ig, batch, base, target):
    """One forward and one backward per path point from ``base`` (a tensor per interpolated
    input): (attributions per input, path predictions [m + 1, B])."""
    vals, static, build = ig._split(batch)
    B, m = vals[0].shape[0], ig.m_steps
    grads, path = [], []
    for i in range(m + 1):
        a = i / m
        xs = [(b + a * (v - b)).detach().requires_grad_(True) for v, b in zip(vals, base)]
        out = ig.model(build(xs, static)).reshape(B, -1)
        y = out[:, 0] if out.shape[1] == 1 else out.gather(1, target[:, None])[:, 0]
        grads.append(torch.autograd.grad(y.sum(), xs))
        path.append(y.detach())
    attr = []
    for j, (v, b) in enumerate(zip(vals, base)):
        g = torch.stack([gs[j] for gs in grads])
        attr.append(((g[:-1] + g[1:]) / 2).mean(0) * (v - b))
    return attr, torch.stack(path)


def _bases(ig, batch, kind):
    """The baselines of a kind, worked out here: a list (draws) of lists (one tensor per input)."""
    vals = _vals(ig, batch)
    live = (batch.node_mask > 0)[:, None, :, None]
    if kind == "mean":
        return [[(v.mean(1, keepdim=True).expand_as(v) * (live if v is batch.x else 1)) for v in vals]]
    if kind == "explicit":
        xb, ab = _explicit_pair(batch)
        return [[xb if v is batch.x else ab for v in vals]]
    gen = torch.Generator().manual_seed(ig.seed)
    us = [torch.rand((N_DRAWS,) + tuple(v.shape), generator=gen, dtype=torch.float32).double() for v in vals]
    out = []
    for i in range(N_DRAWS):
        row = []
        for v, u in zip(vals, us):
            lo, hi = v.amin(1, keepdim=True), v.amax(1, keepdim=True)
            row.append((lo + (hi - lo) * u[i]) * (live if v is batch.x else 1))
        out.append(row)
    return out


def _close(a, b, what):
    err, scale = (a - b).abs().max().item(), b.abs().max().item()
    assert err <= 1e-10 * scale + 1e-300, f"{what}: {err:.3e} against max |ref| {scale:.3e}"


def test_mean_baseline_constructs_and_attributes(setups):
    """The engine accepted only ``baseline="zero"`` before; any other string keeps raising."""
    model, ds, batch = setups["cml_gcn"]
    res = IntegratedGradients(model, "cml", baseline="mean", m_steps=4).attribute(batch)
    assert res["grad_x"].shape == batch.x.shape and res["grad_anom"].shape == batch.anom.shape
    assert torch.equal(res["baseline_pred"], res["path_pred"][0])
    assert res["grad_x"].abs().max() > 0 and res["grad_anom"].abs().max() > 0
    with pytest.raises(NotImplementedError):
        IntegratedGradients(model, "cml", baseline="blurred")
    with pytest.raises(ValueError):
        IntegratedGradients(model, "cml", baseline="random", n_baselines=0)
    with pytest.raises(ValueError):
        IntegratedGradients(model, "cml").attribute(batch, baselines=(batch.x[:, :-1], batch.anom))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", MODELS)
def test_engine_matches_plain_alpha_loop(setups, name, kind):
    """Engine == the loop over path points to 1e-10 relative (attributions and path predictions
    averaged over the draws), with the path in several chunks; ``pred`` is the model at x and the
    SoilNet ``target`` is chosen there; the saved baseline is the one the path started from."""
    model, ds, batch = setups[name]
    m = 8
    ig = _engine(model, ds, kind, m, max_rows=len(batch.wid) * 4)
    res = _attribute(ig, batch, kind)
    vals = _vals(ig, batch)
    with torch.no_grad():
        full = model(ig._split(batch)[2](vals, ig._split(batch)[1])).reshape(len(batch.wid), -1)
    target = None
    if full.shape[1] > 1:
        target = full.masked_fill(batch.node_mask <= 0, -1.0).argmax(1)
        assert torch.equal(res["target"], target)
        full = full.gather(1, target[:, None])
    assert torch.equal(res["pred"], full[:, 0].float())          # (the engine returns it in float32)
    bases = _bases(ig, batch, kind)
    assert len(bases) == (N_DRAWS if kind == "random" else 1)
    loops = [_loop(ig, batch, b, target) for b in bases]
    keys = ["grad_x" if v is batch.x else "grad_anom" for v in vals]
    for j, k in enumerate(keys):
        ref = torch.stack([at[j] for at, _ in loops]).mean(0)
        assert ref.abs().max() > 0
        _close(res[k], ref, k)
        bref = torch.stack([b[j] for b in bases]).mean(0)
        _close(res["baseline_x" if k == "grad_x" else "baseline_anom"], bref, "baseline " + k)
    path = torch.stack([p for _, p in loops]).mean(0)
    _close(res["path_pred"], path, "path_pred")
    assert torch.equal(res["baseline_pred"], res["path_pred"][0])
    _close(res["path_pred"][-1], full[:, 0], "path end")
    if "grad_x" in res:                        # masked nodes get no attribution
        dead = (batch.node_mask <= 0)[:, None, :, None].expand_as(res["grad_x"])
        assert torch.count_nonzero(res["grad_x"][dead]) == 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", MODELS)
def test_completeness_from_a_baseline(setups, name, kind):
    """sum of attributions ~ f(x) - f(b), in the form of tests/test_ig_gpu.py:
    |gap| <= 0.05 |f(x) - f(b)| + 2e-3."""
    model, ds, batch = setups[name]
    res = _attribute(_engine(model, ds, kind, 32), batch, kind)
    gap = completeness_gap(res).abs()
    span = (res["path_pred"][-1] - res["path_pred"][0]).abs()
    print(f"{name} {kind}: gap {gap.tolist()} span {span.tolist()}")
    assert bool((gap <= 0.05 * span + 2e-3).all()), (gap, span)


@pytest.mark.parametrize("name", MODELS)
def test_random_baseline_is_reproducible(setups, name):
    """The same seed gives the same draws and results (in any call order); another seed does not."""
    model, ds, batch = setups[name]
    a = IntegratedGradients(model, ds, m_steps=4, baseline="random", n_baselines=2, seed=3)
    b = IntegratedGradients(model, ds, m_steps=4, baseline="random", n_baselines=2, seed=3)
    c = IntegratedGradients(model, ds, m_steps=4, baseline="random", n_baselines=2, seed=4)
    ra, _, ra2 = a.attribute(batch), a.attribute(batch), a.attribute(batch)
    rb, rc = b.attribute(batch), c.attribute(batch)
    k = "grad_x" if "grad_x" in ra else "grad_anom"
    kb = "baseline_x" if "grad_x" in ra else "baseline_anom"
    for r in (ra2, rb):
        assert torch.equal(ra[k], r[k]) and torch.equal(ra[kb], r[kb]) and torch.equal(ra["path_pred"], r["path_pred"])
    assert not torch.equal(ra[kb], rc[kb]) and not torch.equal(ra[k], rc[k])
    # draws lie between the window's min and max over time, per (node, channel)
    v = batch.x if k == "grad_x" else batch.anom
    d = a._draws(batch, "random")[0]
    assert d.shape == (2,) + tuple(v.shape)
    assert bool((d >= v.amin(1, keepdim=True)).all() and (d <= v.amax(1, keepdim=True)).all())


@pytest.mark.parametrize("name", MODELS)
def test_zero_baseline_takes_the_unchanged_code_path(setups, name, monkeypatch):
    """baseline="zero" is one call of the zero-baseline path function with no baseline and no policy
    override, never builds a baseline, and returns that call's tensors bit for bit; the only
    addition is ``baseline_pred``, a view of ``path_pred[0]``."""
    model, ds, batch = setups[name]
    ig = IntegratedGradients(model, ds, m_steps=4)
    calls = []
    orig = IntegratedGradients._attribute_one

    def spy(self, *a, **kw):
        calls.append((a[1:], kw))
        return orig(self, *a, **kw)

    def no_baseline(*a, **kw):
        raise AssertionError("the zero baseline builds no baseline tensor")

    monkeypatch.setattr(IntegratedGradients, "_attribute_one", spy)
    monkeypatch.setattr(IntegratedGradients, "_window_mean", staticmethod(no_baseline))
    assert ig._draws(batch, "zero") is None
    res = ig.attribute(batch)
    assert calls == [((None,), {})]
    ref = orig(ig, batch, None)
    assert set(res) == set(ref) | {"baseline_pred"}
    for k, v in ref.items():
        assert torch.equal(res[k], v) if isinstance(v, torch.Tensor) else res[k] == v, k
    assert res["baseline_pred"].data_ptr() == res["path_pred"][0].data_ptr()
    assert "baseline_x" not in res and "baseline_anom" not in res


def test_negative_value_policy_applies_to_the_average(setups):
    model, ds, batch = setups["cml_baseline"]
    keep = IntegratedGradients(model, ds, m_steps=4, baseline="random", n_baselines=2, seed=1).attribute(batch)
    assert (keep["grad_anom"] < 0).any()
    for policy, fn in (("abs", torch.abs), ("clip", lambda t: t.clamp(min=0))):
        got = IntegratedGradients(model, ds, m_steps=4, baseline="random", n_baselines=2, seed=1,
                                  negative_values=policy).attribute(batch)
        assert torch.equal(got["grad_anom"], fn(keep["grad_anom"]))


def test_cli_explain_takes_xai_overrides(tmp_path):
    """``explain --set integrated_gradients.<key>=v`` and ``--set xai.<key>=v`` reach the XAI
    config: a SoilNet run with the mean baseline writes the baseline of every sample into a tree
    named by the overridden project, and the analyser reads that tree."""
    import os

    import numpy as np

    from gnnqc.ckpt import save_model
    from gnnqc.cli.__main__ import main
    from gnnqc.xai.analyse import IntegrateGradientsAnalyser
    ps = C.default("preprocessing_soilnet")
    ps["timestep_before"], ps["timestep_after"] = 360, 60
    ps = C.normalize_preproc(ps)
    torch.manual_seed(0)
    model = create_model(C.default("model_soilnet"), ps)
    with torch.no_grad():
        model.dense_out.kernel.mul_(40.0)
    mdir, out = str(tmp_path / "model"), str(tmp_path / "xplain")
    save_model(model, mdir, preproc_config=ps)
    pre = ["--set", "pre.timestep_before=360", "--set", "pre.timestep_after=60", "--set", "pre.batch_size=4"]
    main(["explain", "--ds", "soilnet", "--synthetic", "--sensors", "4", "--days", "6", "--device", "cpu",
          "--model-dir", mdir, "--max-batches", "1", "--out-dir", out, *pre,
          "--set", "integrated_gradients.baseline=mean", "--set", "integrated_gradients.m_steps=4",
          "--set", "integrated_gradients.dataset=all", "--set", "integrated_gradients.threshold=0.5",
          "--set", "xai.project=meanbase"])
    root = os.path.join(out, "integrated_gradients", "meanbase", "soilnet", "all")
    samples = [os.path.join(d, f) for d, _, fs in os.walk(root) for f in fs if f.startswith("features_unwrapped_")]
    assert len(samples) == 4
    for p in samples:
        f = np.load(p)
        b = np.load(p.replace("features_unwrapped_", "baseline_features_unwrapped_"))
        np.testing.assert_allclose(b, np.broadcast_to(f.mean(1, keepdims=True), f.shape), rtol=1e-5, atol=1e-6)
        assert not os.path.exists(p.replace("features_unwrapped_", "baseline_anom_ts_unwrapped_"))
    xc = C.default("xai_ig")
    xc["output_dir"], xc["project"] = out, "meanbase"
    xc.integrated_gradients["dataset"], xc.integrated_gradients["threshold"] = "all", 0.5
    xc.integrated_gradients.analyser["which_samples"] = ["TP", "FP", "TN", "FN"]
    pc2 = C.Config(dict(ps))
    pc2["batch_size"] = 4
    assert len(IntegrateGradientsAnalyser(pc2, C.default("model_soilnet"), xc).get_overview(plots=False)) == 4


def test_first_baseline_is_the_start_of_the_first_path(setups):
    """What the explainer's path plot draws from: nothing for zero, the window mean, the first of
    the random draws (not their mean), the explicit pair."""
    model, ds, batch = setups["cml_gcn"]
    assert IntegratedGradients(model, ds).first_baseline(batch) == {}
    ig = IntegratedGradients(model, ds, baseline="random", n_baselines=3, seed=2)
    fb, draws = ig.first_baseline(batch), ig._draws(batch, "random")
    assert set(fb) == {"baseline_x", "baseline_anom"}
    assert torch.equal(fb["baseline_x"], draws[0][0]) and torch.equal(fb["baseline_anom"], draws[1][0])
    assert not torch.equal(fb["baseline_x"], draws[0].mean(0))
    mean = IntegratedGradients(model, ds, baseline="mean").first_baseline(batch)
    assert torch.equal(mean["baseline_anom"], batch.anom.mean(1, keepdim=True).expand_as(batch.anom))
    xb, ab = _explicit_pair(batch)
    ex = IntegratedGradients(model, ds).first_baseline(batch, baselines=(xb, ab))
    assert torch.equal(ex["baseline_x"], xb) and torch.equal(ex["baseline_anom"], ab)
