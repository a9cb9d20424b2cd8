"""Integrated gradients on the GPU (alpha folded into the batch, HIP chain / GCN input-gradient
kernels, ig_interp / ig_accum / ig_finalize) against the same explainer evaluated in float64 on the
CPU with the LSTM rounded where the kernels round (gnnqc/ops/lstm_ref.py)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

# "flipping" model state: at least this share of the valid (window, step, node, channel) pairs changes
# sign strictly inside the path on the float64 side (the windows' features are mostly near zero, so
# x W moves y = alpha x W + A0 across 0 for a few per cent of them: thousands of pairs per batch)
MIN_FLIP_SHARE = 0.01


def _flipping_state(model, seed):
    """GCN layer state under which y(s) = alpha_s x W + A0 changes sign inside the path (a fresh model
    has bias 0 and moving mean 0, so A0 = 0 and the sign never changes): bias and moving mean
    N(0, 0.3), moving variance U(0.5, 2), some negative bn_gamma, PReLU slopes 0, negative, 1 and
    above 1 (cycled over the channels)."""
    g = model.gcn_layer
    gen = torch.Generator().manual_seed(seed)
    F = g.kernel.shape[1]
    with torch.no_grad():
        g.bias.copy_(0.3 * torch.randn(F, generator=gen))
        g.bn_moving_mean.copy_(0.3 * torch.randn(F, generator=gen))
        g.bn_moving_variance.copy_(0.5 + 1.5 * torch.rand(F, generator=gen))
        gamma = 0.5 + torch.rand(F, generator=gen)
        gamma[1::4] *= -1
        g.bn_gamma.copy_(gamma)
        slopes = torch.tensor([0.0, -0.3, 1.0, 1.7, 0.25])
        g.prelu_alpha.copy_(slopes[torch.arange(F) % 5])


def _flip_share_fp64(ref_model, bc, m):
    """Share of valid (window, step, node, channel) pairs whose GCN pre-activation (eval BatchNorm,
    float64) has another sign at the path's end (alpha = 1) than at its first step (alpha = 1 / m):
    sign changes strictly inside the path."""
    g = ref_model.gcn_layer
    with torch.no_grad():
        sc = g.bn_gamma * torch.rsqrt(g.bn_moving_variance + g.eps)
        xw = torch.matmul(bc.x, g.kernel)
        y0 = (xw / m + g.bias - g.bn_moving_mean) * sc + g.bn_beta
        y1 = (xw + g.bias - g.bn_moving_mean) * sc + g.bn_beta
        valid = (bc.node_mask > 0)[:, None, :, None].expand_as(y1)
        flip = ((y0 > 0) != (y1 > 0)) & valid
    return flip.sum().item() / valid.sum().item()


def _ig_model(cuda_device, pc, state, mc=None, seed=0):
    from gnnqc import config as C
    from gnnqc.models import GCNClassifier
    torch.manual_seed(seed)
    model = GCNClassifier(mc if mc is not None else C.default("model_cml"), pc).to(cuda_device)
    with torch.no_grad():                      # a non-trivial output range along the path
        model.dense_out.bias.fill_(0.3)
        for p in (model.dense.bias, model.dense2.bias):
            p.normal_(0, 0.2)
    if state == "flipping":
        _flipping_state(model, 100 + seed)
    return model


def _ig_gpu_and_fp64(cuda_device, cml_windows, model, ids, m, negative_values="keep"):
    """(GPU attribution, float64 CPU attribution with the LSTM rounded where the kernels round,
    float64 model, float64 CPU batch) of ``model`` on the windows ``ids``."""
    from gnnqc.data.store import DeviceStore
    from gnnqc.xai.ig import IntegratedGradients
    pc, ws = cml_windows
    st = DeviceStore(ws, "rolling_median", pc.graph, device=cuda_device)
    st_cpu = DeviceStore(ws, "rolling_median", pc.graph, device="cpu")
    b = st.gather(ids.to(cuda_device))
    got = IntegratedGradients(model, "cml", m_steps=m, negative_values=negative_values).attribute(b)
    torch.cuda.synchronize()

    ref_model = copy.deepcopy(model).cpu().double()
    bc = st_cpu.gather(ids)
    for f in ("x", "anom", "adj", "node_mask"):
        setattr(bc, f, getattr(bc, f).double())
    from gnnqc.ops.lstm_ref import kernel_rounding
    with kernel_rounding():
        ref = IntegratedGradients(ref_model, "cml", m_steps=m, negative_values=negative_values).attribute(bc)
    return got, ref, ref_model, bc


def _assert_ig_close(got, ref):
    for k in ("grad_x", "grad_anom", "pred", "path_pred"):
        a, r = got[k].double().cpu(), ref[k]
        err = (a - r).norm().item()
        scale = r.norm().item()
        assert err <= 6e-3 * scale + 1e-6, (k, err, scale)


@pytest.mark.parametrize("state", ["fresh", "flipping"])
@pytest.mark.parametrize("negative_values", ["keep", "abs"])
def test_ig_gpu_matches_fp64_cpu(cuda_device, cml_windows, negative_values, state):
    """fresh: a new model (GCN bias 0, BN moving mean 0: no sign change inside the path);
    flipping: :func:`_flipping_state`, where the float64 side shows sign changes inside the path."""
    from gnnqc.xai.ig import completeness_gap
    pc, ws = cml_windows
    model = _ig_model(cuda_device, pc, state)
    got, ref, ref_model, bc = _ig_gpu_and_fp64(cuda_device, cml_windows, model, torch.tensor([0, 7, 19, 33]), 24,
                                               negative_values)
    share = _flip_share_fp64(ref_model, bc, 24)
    if state == "flipping":
        assert share >= MIN_FLIP_SHARE, share
    else:
        assert share == 0
    _assert_ig_close(got, ref)
    if negative_values == "keep":
        # completeness (sum of attributions ~ f(x) - f(0)) holds on the GPU as well as in fp64
        gap_g = completeness_gap(got).abs().cpu().double()
        gap_r = completeness_gap(ref).abs()
        span = (ref["path_pred"][-1] - ref["path_pred"][0]).abs()
        assert bool((gap_g <= gap_r + 0.05 * span + 2e-3).all()), (gap_g, gap_r, span)


def test_ig_gpu_sliced_path_matches_fp64_cpu(cuda_device, cml_windows):
    """m_steps = 130 on three windows: one path-folded chunk of kk = 131 points, which
    ig_gcn_pool_bwd slices into launches of 128 + 3 (flipping model state), against float64."""
    from gnnqc.xai.ig import IntegratedGradients
    pc, ws = cml_windows
    model = _ig_model(cuda_device, pc, "flipping", seed=2)
    m = 130
    ig = IntegratedGradients(model, "cml", m_steps=m)
    assert m + 1 > 128 and ig.max_rows // 3 >= m + 1          # one chunk, longer than a backward slice
    got, ref, ref_model, bc = _ig_gpu_and_fp64(cuda_device, cml_windows, model, torch.tensor([2, 9, 17]), m)
    assert _flip_share_fp64(ref_model, bc, m) >= MIN_FLIP_SHARE
    assert tuple(got["path_pred"].shape) == (m + 1, 3)
    _assert_ig_close(got, ref)


def test_ig_gpu_refused_model_takes_generic_path(cuda_device, cml_windows):
    """GCN units 64 is outside the path-folded kernels' dispatch: _cml_path_folded_ok is False and
    the generic path (kk x B interpolated copies) matches the float64 explainer."""
    from gnnqc import config as C
    from gnnqc.data.store import DeviceStore
    from gnnqc.xai.ig import IntegratedGradients
    pc, ws = cml_windows
    mc = C.default("model_cml")
    mc["graph_convolution"]["units"] = 64
    model = _ig_model(cuda_device, pc, "flipping", mc=mc, seed=4)
    assert model.gcn_layer.kernel.shape[1] == 64
    ids = torch.tensor([3, 8, 21])
    b = DeviceStore(ws, "rolling_median", pc.graph, device=cuda_device).gather(ids.to(cuda_device))
    model.eval()
    assert not IntegratedGradients(model, "cml", m_steps=16)._cml_path_folded_ok(b)
    model.train()
    got, ref, ref_model, bc = _ig_gpu_and_fp64(cuda_device, cml_windows, model, ids, 16)
    assert _flip_share_fp64(ref_model, bc, 16) >= MIN_FLIP_SHARE
    _assert_ig_close(got, ref)


def test_ig_hip_kernels_match_torch(cuda_device):
    from gnnqc.utils.native import hip_ops
    ops = hip_ops()
    torch.manual_seed(1)
    v = torch.randn(5, 37, 3, device=cuda_device)            # numel % 4 != 0: scalar tail
    a = torch.linspace(0, 1, 7, device=cuda_device)
    out = ops.ig_interp(v, a)
    torch.testing.assert_close(out.view(7, 5, 37, 3), a.view(7, 1, 1, 1) * v.unsqueeze(0))
    g = torch.randn(7 * 5, 37, 3, device=cuda_device)
    w = torch.rand(7, device=cuda_device)
    acc = torch.randn(5, 37, 3, device=cuda_device)
    expect = acc + torch.tensordot(w, g.view(7, 5, 37, 3), dims=1)
    ops.ig_accum(acc, g, w)
    torch.testing.assert_close(acc, expect, rtol=1e-5, atol=1e-5)
    for mode, fn in ((0, lambda t: t), (1, lambda t: t.clamp(min=0)), (2, torch.abs)):
        torch.testing.assert_close(ops.ig_finalize(acc, v, mode), fn(acc * v))
    torch.testing.assert_close(ops.ig_finalize(acc, v.new_zeros(0), 0), acc)


@pytest.mark.parametrize("kk", [1, 7])
@pytest.mark.parametrize("shape", [(5, 37, 3), (5, 36, 4), (3, 1000, 7), (3, 1001, 7), (4, 1024, 8)])
def test_ig_elementwise_kernels_match_float64(cuda_device, shape, kk):
    """ig_interp, ig_accum, ig_finalize against float64 on the float4 path (numel % 4 == 0) and the
    scalar path, in one workgroup and in several ((3, 1000, 7) and (4, 1024, 8): 21 and 32 workgroups,
    float4; (3, 1001, 7): 21 workgroups, scalar). Bounds (EPS = 2^-24): one product: EPS |ref|; kk multiply-adds onto acc:
    (kk + 2) EPS (|acc| + sum_s |w_s g_s|) (kk products, kk additions of partial sums below that
    magnitude sum, second-order terms)."""
    from gnnqc.utils.native import hip_ops
    ops = hip_ops()
    dev = cuda_device
    EPS = 2.0 ** -24
    gen = torch.Generator().manual_seed(17 * kk + shape[1])
    v = torch.randn(*shape, generator=gen)
    n = v.numel()
    assert (n % 4 == 0) == (shape[1] % 4 == 0) and (n > 4 * 256) == (shape[1] >= 1000)
    a = torch.linspace(0, 1, kk) if kk > 1 else torch.tensor([0.625])
    out = ops.ig_interp(v.to(dev), a.to(dev))
    assert tuple(out.shape) == (kk * shape[0],) + shape[1:]
    ref = a.double().view(kk, 1, 1, 1) * v.double().unsqueeze(0)
    assert ((out.double().cpu().view(ref.shape) - ref).abs() <= EPS * ref.abs()).all()
    g = torch.randn(kk * shape[0], *shape[1:], generator=gen)
    w = torch.rand(kk, generator=gen)
    acc0 = torch.randn(*shape, generator=gen)
    accs = []
    for _ in range(2):
        acc = acc0.to(dev)
        ops.ig_accum(acc, g.to(dev), w.to(dev))
        accs.append(acc)
    assert torch.equal(accs[0], accs[1])                       # fixed step order: deterministic
    terms = w.double().view(kk, 1, 1, 1) * g.double().view(kk, *shape)
    ref = acc0.double() + terms.sum(0)
    bound = (kk + 2) * EPS * (acc0.double().abs() + terms.abs().sum(0))
    assert ((accs[0].double().cpu() - ref).abs() <= bound).all()
    acc = accs[0]
    a64 = acc.double().cpu()
    for scaled in (True, False):
        prod = a64 * v.double() if scaled else a64
        for mode, fn in ((0, lambda t: t), (1, lambda t: t.clamp(min=0)), (2, torch.abs)):
            got = ops.ig_finalize(acc, v.to(dev) if scaled else v.new_zeros(0).to(dev), mode)
            assert got.shape == acc.shape
            assert ((got.double().cpu() - fn(prod)).abs() <= EPS * prod.abs()).all(), (scaled, mode)
    torch.cuda.synchronize()


def test_ig_path_folded_gcn_matches_replicated_path(cuda_device, cml_windows, monkeypatch):
    """The CML GCN's path-folded IG (alpha applied inside ig_gcn_pool_fwd, input gradients
    trapezoid-summed inside ig_gcn_pool_bwd) == the generic path over kk x B interpolated copies
    (ig_interp -> GCN kernels -> ig_accum), with several path chunks (max_rows < (m+1) B)."""
    from gnnqc import config as C
    from gnnqc.data.store import DeviceStore
    from gnnqc.models import GCNClassifier
    from gnnqc.xai.ig import IntegratedGradients
    pc, ws = cml_windows
    torch.manual_seed(3)
    model = GCNClassifier(C.default("model_cml"), pc).to(cuda_device)
    with torch.no_grad():
        model.dense_out.bias.fill_(0.2)
        model.gcn_layer.bn_moving_mean.normal_(0, 0.3)
        model.gcn_layer.bn_moving_variance.uniform_(0.5, 2.0)
    st = DeviceStore(ws, "rolling_median", pc.graph, device=cuda_device)
    b = st.gather(torch.tensor([1, 5, 11, 23, 40], device=cuda_device))
    ig = IntegratedGradients(model, "cml", m_steps=30, max_rows=5 * 8)
    model.eval()                               # (attribute() switches to eval itself)
    assert ig._cml_path_folded_ok(b)
    model.train()
    got = ig.attribute(b)
    monkeypatch.setattr(IntegratedGradients, "_cml_path_folded_ok", lambda self, batch: False)
    ref = IntegratedGradients(model, "cml", m_steps=30, max_rows=5 * 8).attribute(b)
    torch.cuda.synchronize()
    for k in ("grad_x", "grad_anom", "pred", "path_pred"):
        err = (got[k] - ref[k]).abs().max().item()
        scale = ref[k].abs().max().item()
        assert err <= 1e-4 * scale + 1e-7, (k, err, scale)


def test_ig_graph_replay_matches_eager(cuda_device, cml_windows):
    """The path-folded IG replays one HIP graph per input shape: a second batch of the same shape
    (inputs copied into the captured buffers) gives what the eager attribution gives."""
    from gnnqc import config as C
    from gnnqc.data.store import DeviceStore
    from gnnqc.models import GCNClassifier
    from gnnqc.xai.ig import IntegratedGradients
    pc, ws = cml_windows
    torch.manual_seed(5)
    model = GCNClassifier(C.default("model_cml"), pc).to(cuda_device)
    st = DeviceStore(ws, "rolling_median", pc.graph, device=cuda_device)
    b1 = st.gather(torch.tensor([2, 9, 17], device=cuda_device))
    b2 = st.gather(torch.tensor([4, 12, 30], device=cuda_device))
    ig = IntegratedGradients(model, "cml", m_steps=20)
    ig.attribute(b1)
    assert ig._graph is not None
    got = ig.attribute(b2)
    ref = IntegratedGradients(model, "cml", m_steps=20, use_graph=False).attribute(b2)
    torch.cuda.synchronize()
    for k in ("grad_x", "grad_anom", "pred", "path_pred"):
        err = (got[k] - ref[k]).abs().max().item()
        assert err <= 1e-5 * ref[k].abs().max().item() + 1e-7, (k, err)


def test_head_prob_kernels_match_torch(cuda_device):
    """head_prob_fwd / head_prob_bwd (head.hip PROB mode): sigmoid of the Dense-LeakyReLU head and
    the input gradient of sum(sigmoid) against autograd on a plain fp32 PyTorch head."""
    from gnnqc.ops.head import head_eager
    from gnnqc.utils.native import hip_ops
    torch.manual_seed(0)
    for R, F in ((37, 128), (300, 64)):
        feat = torch.randn(R, F, device=cuda_device)
        W1, b1 = torch.randn(F, 64, device=cuda_device) * 0.2, torch.randn(64, device=cuda_device) * 0.1
        W2, b2 = torch.randn(64, 64, device=cuda_device) * 0.2, torch.randn(64, device=cuda_device) * 0.1
        W3, b3 = torch.randn(64, 1, device=cuda_device) * 0.3, torch.randn(1, device=cuda_device) * 0.1
        z1, z2, prob = hip_ops().head_prob_fwd(feat, W1, b1, W2, b2, W3, b3, 0.3, 0.2)
        dfeat = hip_ops().head_prob_bwd(feat, W1, W2, W3, z1, z2, prob, 0.3, 0.2)
        f = feat.clone().requires_grad_(True)
        ref = torch.sigmoid(head_eager(f, W1, b1, W2, b2, W3, b3, 0.3, 0.2))
        (g,) = torch.autograd.grad(ref.sum(), f)
        torch.testing.assert_close(prob, ref.detach(), atol=2e-6, rtol=1e-5)
        torch.testing.assert_close(dfeat, g, atol=1e-6, rtol=1e-4)


def test_ig_hip_head_matches_torch_head(cuda_device, cml_windows, monkeypatch):
    """The path-folded IG with the frozen head on HIP (GNNQC_IG_HEAD_HIP=1, default) == with the
    PyTorch head (rocBLAS GEMMs + aten LeakyReLU / sigmoid)."""
    from gnnqc import config as C
    from gnnqc.data.store import DeviceStore
    from gnnqc.models import GCNClassifier
    from gnnqc.xai.ig import IntegratedGradients
    pc, ws = cml_windows
    torch.manual_seed(7)
    model = GCNClassifier(C.default("model_cml"), pc).to(cuda_device)
    st = DeviceStore(ws, "rolling_median", pc.graph, device=cuda_device)
    b = st.gather(torch.tensor([3, 8, 21, 33], device=cuda_device))
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("GNNQC_IG_HEAD_HIP", flag)
        res[flag] = IntegratedGradients(model, "cml", m_steps=24, use_graph=False).attribute(b)
    torch.cuda.synchronize()
    for k in ("grad_x", "grad_anom", "pred", "path_pred"):
        err = (res["1"][k] - res["0"][k]).abs().max().item()
        assert err <= 1e-5 * res["0"][k].abs().max().item() + 1e-7, (k, err)


def test_ig_time4_fused_head_matches_separate_head(cuda_device, cml_windows, monkeypatch):
    """The path-folded IG with time4 + the frozen head in one launch (GNNQC_IG_T4_HEAD=1, default:
    time4_prob_fwd -> sigmoid outputs and d p / d h_{T-1}; time4_bwd seeded with them) == time4 alone
    followed by the head_prob kernels (GNNQC_IG_T4_HEAD=0); and the fused launch really ran."""
    from gnnqc import config as C
    from gnnqc.data.store import DeviceStore
    from gnnqc.models import GCNClassifier
    from gnnqc.ops import lstm as L
    from gnnqc.xai.ig import IntegratedGradients
    pc, ws = cml_windows
    torch.manual_seed(11)
    model = GCNClassifier(C.default("model_cml"), pc).to(cuda_device)
    with torch.no_grad():
        model.dense_out.bias.fill_(0.3)
    st = DeviceStore(ws, "rolling_median", pc.graph, device=cuda_device)
    b = st.gather(torch.tensor([3, 8, 21, 33, 34], device=cuda_device))
    calls = []
    orig = L._HipLSTMLast128Prob.forward

    def spy(ctx, *a):
        calls.append(1)
        return orig(ctx, *a)

    monkeypatch.setattr(L._HipLSTMLast128Prob, "forward", staticmethod(spy))
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("GNNQC_IG_T4_HEAD", flag)
        res[flag] = IntegratedGradients(model, "cml", m_steps=24, use_graph=False).attribute(b)
    torch.cuda.synchronize()
    assert calls, "the fused time4 + head path did not run"
    for k in ("grad_x", "grad_anom", "pred", "path_pred"):
        err = (res["1"][k] - res["0"][k]).abs().max().item()
        assert err <= 1e-4 * res["0"][k].abs().max().item() + 1e-7, (k, err)
