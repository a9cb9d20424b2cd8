"""The shared HIP-graph helpers on the GPU (gnnqc.utils.graphs): the cursor machine with captured
graphs, the Trainer's lazily captured step graphs against the prepared ones, and the integrated
gradients graph's ownership of the backward seed it reads by address."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_cursor_graphs_captured_walk_the_table(cuda_device):
    """What tests/test_graphs_cpu.py asserts, replayed from graphs: the step is device work only."""
    from gnnqc.utils.graphs import CursorGraphs
    dev = cuda_device
    L = 64
    log = torch.full((L, 4), -1, dtype=torch.long, device=dev)
    count = torch.zeros(1, dtype=torch.long, device=dev)

    def step(ids):
        row = ids.table.index_select(0, ids.cursor % ids.table.shape[0])       # [1, B]
        log.index_copy_(0, count % L, row)
        count.add_(1)
        ids.cursor.add_(1)
        return row

    def visited():
        n = int(count)
        out = (log[:n, 0] // 4).tolist()
        count.zero_()
        return out

    rows = torch.arange(20, dtype=torch.long, device=dev).reshape(5, 4)
    cg = CursorGraphs(step, 2, dev)
    assert cg.captured is True
    assert cg.load(rows) == (True, True)
    cg.capture()
    g, g1 = cg.graph, cg.graph1
    assert g is not None and g1 is not None and g is not g1
    visited()                                           # (the warm-up steps logged too)

    n, n1, out = cg.run(3, 5)
    assert (n, n1) == (2, 1) and visited() == [3, 4, 0, 1, 2]
    assert out is cg.out1 and torch.equal(out[0], rows[2]) and torch.equal(cg.out[0], rows[1])
    n, n1, out = cg.run(0, 1)
    assert (n, n1) == (0, 1) and visited() == [0] and out is cg.out1 and torch.equal(out[0], rows[0])
    assert cg.run(0, 0)[:2] == (0, 0) and visited() == []
    n, n1, out = cg.run(7, 2)
    assert (n, n1) == (1, 0) and visited() == [2, 3] and out is cg.out and torch.equal(out[0], rows[3])

    assert cg.load(rows) == (False, False)              # the same tensor, unmodified: no copy
    rows[0] += 100
    assert cg.load(rows) == (True, False)
    assert cg.graph is g and cg.graph1 is g1            # same shape: the graphs stay
    assert torch.equal(cg.run(0, 1)[2][0], torch.arange(100, 104, device=dev))
    count.zero_()
    table = cg.table
    assert cg.load(torch.arange(12, dtype=torch.long, device=dev).reshape(3, 4)) == (True, True)
    assert cg.table is not table and cg.graph is None and cg.graph1 is None
    cg.capture()
    assert cg.graph is not None and cg.graph is not g and cg.graph1 is not None and cg.graph1 is not g1
    visited()
    assert cg.run(4, 3)[:2] == (1, 1) and visited() == [1, 2, 0]


def _run_train_steps(prepare, st, pc, mc, rows, dev):
    from gnnqc.models import GCNClassifier
    from gnnqc.ops.optim import make_optimizer
    from gnnqc.train.engine import Trainer
    torch.manual_seed(0)
    model = GCNClassifier(mc, pc).to(dev)
    opt = make_optimizer("adam", model.parameters(), 1e-3)
    tr = Trainer(model, st, opt, {0: 1.0, 1: 5.0}, use_graph=True, batch_size=32)
    if prepare:
        tr.prepare_graphs(rows)
    tr.train_steps(rows, 3, 11)
    torch.cuda.synchronize()
    assert tr.multi_graph is not None and tr.multi_graph1 is not None
    bufs = torch.cat([b.reshape(-1).double() for b in model.buffers() if b.is_floating_point()])
    return (opt.flat_p.clone(), opt.m.clone(), bufs, tr.train_metrics.sums.clone()), (opt.iterations, tr.global_step)


def test_lazy_capture_equals_prepared_capture(cuda_device, cml_windows, monkeypatch):
    """train_steps captures what prepare_graphs captures (the one-step graph included): 11 steps =
    one 8-step replay + three one-step replays either way. Bitwise-reproducible kernels, as in
    tests/test_step_fusion_gpu.py and for the reason given there."""
    from gnnqc import config as C
    from gnnqc.data.store import DeviceLoader, DeviceStore
    from gnnqc.ops import set_deterministic
    pc, ws = cml_windows
    mc = C.default("model_cml")
    st = DeviceStore(ws, "rolling_median", pc.graph, device=cuda_device)
    rows = DeviceLoader(st, list(range(st.n_windows)), 32, shuffle=True, seed=1).batch_ids()
    monkeypatch.setenv("GNNQC_GRAPH_STEPS", "8")
    prev = set_deterministic(True)
    try:
        (a, na), (b, nb) = [_run_train_steps(prepare, st, pc, mc, rows, cuda_device) for prepare in (False, True)]
    finally:
        set_deterministic(prev)
    for x, y in zip(a, b):
        torch.testing.assert_close(x, y, rtol=1e-5, atol=1e-6)
    assert na == nb == (11, 11)


def test_ig_graph_owns_its_backward_seed(cuda_device, cml_windows):
    """The captured attribution reads its ones seed by address. A non-graphed call of another shape
    replaces ``_ones``; the graph's record keeps the captured one alive, so a later replay reads
    ones, not whatever took the freed memory."""
    from gnnqc import config as C
    from gnnqc.data.store import DeviceStore
    from gnnqc.models import GCNClassifier
    from gnnqc.xai.ig import IntegratedGradients
    pc, ws = cml_windows
    torch.manual_seed(5)
    model = GCNClassifier(C.default("model_cml"), pc).to(cuda_device)
    st = DeviceStore(ws, "rolling_median", pc.graph, device=cuda_device)
    b1 = st.gather(torch.tensor([2, 9, 17], device=cuda_device))
    b2 = st.gather(torch.tensor([4, 12, 30, 41], device=cuda_device))
    ig = IntegratedGradients(model, "cml", m_steps=20)
    first = ig.attribute(b1)
    seed = ig._graph[4]
    assert seed is ig._ones
    ptr = seed.data_ptr()
    ig.attribute(b2, target=torch.zeros(4, dtype=torch.long, device=cuda_device))
    assert ig._ones is not seed and ig._ones.shape != seed.shape          # the eager call replaced it
    third = ig.attribute(b1)
    torch.cuda.synchronize()
    assert ig._graph[4] is seed and seed.data_ptr() == ptr and bool((seed == 1).all())
    for k in ("grad_x", "grad_anom", "pred", "path_pred"):
        err = (third[k] - first[k]).abs().max().item()
        assert err <= 1e-5 * first[k].abs().max().item() + 1e-7, (k, err)


def test_capture_graph_keeps_the_garbage_collector_off_while_capturing(cuda_device):
    """capture_graph collects dead cycles before capture_begin and keeps the cyclic collector off
    until capture_end (an automatic collection on any thread in between could destroy an earlier
    graph, which a capturing stream does not allow), then restores the collector's state."""
    import gc

    from gnnqc.utils.graphs import capture_graph
    buf = torch.zeros(8, device=cuda_device)
    seen = []

    class Node:
        pass

    a, b = Node(), Node()
    a.other, b.other = b, a                              # a dead cycle once the names are dropped
    import weakref
    alive = weakref.ref(a)
    del a, b

    def body():
        seen.append((gc.isenabled(), alive() is None, torch.cuda.is_current_stream_capturing()))
        buf.add_(1)
        return buf

    assert gc.isenabled()
    graph, out = capture_graph(body, warm=lambda: None, warmups=1)
    assert seen == [(False, True, True)]                 # collector off, cycle already collected
    assert gc.isenabled() and out is buf
    graph.replay()
    torch.cuda.synchronize()
    assert buf.tolist() == [1.0] * 8                     # (captured work runs at replay only)
    gc.disable()
    try:                                                 # a caller that had it off keeps it off
        capture_graph(body, warm=lambda: None, warmups=1)
        assert not gc.isenabled()
    finally:
        gc.enable()
