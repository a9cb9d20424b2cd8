"""The weight-gradient queue of ``gnnqc/ops/wgrad.py`` and the chain's saved-state view, without a GPU: the
operators fetch their namespace through ``hip_ops()`` on every call, so a stand-in that records each call
(and returns a tensor where the queue keeps one) lets the queue run on CPU tensors. What is asserted is
which launch is issued when, carrying which job, and what stays queued. No kernel runs."""
import pytest
import torch

from gnnqc.ops import wgrad as Q
from gnnqc.ops.lstm_chain import _ChainSaved

# positions in lstm_tm_bwd_pipe's arguments: the recurrence (dh, g, c, W, U), T, the gradient job
# (gz, gx, gh, gW, period, hshift, gws), the reduce (rws, rW, rdW, rdU, rdb)
REC, T_ARG, JOB, JOB_WS, RED = slice(0, 5), 5, 6, 12, 13


class RecordingOps:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def op(*args):
            self.calls.append((name, args))
            if name in ("lstm_grads_job_ws", "lstm_tm_bwd_pipe", "lstm_dx"):
                return torch.zeros(1)
        return op

    def named(self, name):
        return [a for n, a in self.calls if n == name]

    def names(self):
        return [n for n, _ in self.calls]


@pytest.fixture
def ops(monkeypatch):
    rec = RecordingOps()
    monkeypatch.setattr("gnnqc.utils.native.hip_ops", lambda: rec)
    for k, v in dict(enabled=True, job=None, red=None, batch=[], reds=[], gcn=None).items():
        monkeypatch.setattr(Q._Pipe, k, v)
    monkeypatch.setattr(Q._DirectGrad, "enabled", True)
    monkeypatch.setattr(Q._Deferred, "pending", False)
    monkeypatch.delenv("GNNQC_GCN_DEFER", raising=False)
    return rec


def _layer(H=16, D=4, T=2, Mp=16):
    """x [T, Mp, D], h [T, Mp, H], W [D, 4H], dz, and direct sinks of (W, U, b)."""
    sinks = [(torch.zeros(D, 4 * H), True), (torch.zeros(H, 4 * H), True), (torch.zeros(4 * H), True)]
    return dict(x=torch.zeros(T, Mp, D), h=torch.zeros(T, Mp, H), W=torch.zeros(D, 4 * H), U=torch.zeros(H, 4 * H),
                dz=torch.zeros(T, Mp, 4 * H), sinks=sinks)


def _job(**kw):
    L = _layer(**kw)
    return Q._pipe_job(L["dz"], L["x"], L["h"], L["W"], L["sinks"], L["x"].shape[0] * 16, 16)


def _empty(args):
    return all(a.numel() == 0 for a in args)


def _push_two(ops):
    j1, j2 = _job(), _job()
    Q._pipe_push(j1)
    Q._pipe_push(j2)
    return j1, j2


def test_second_push_advances_the_first_job(ops):
    j1, j2 = _push_two(ops)
    (a,) = ops.named("lstm_tm_bwd_pipe")
    assert _empty(a[REC]) and a[T_ARG] == 0                      # no recurrence
    assert a[JOB] is j1["dz"] and a[JOB_WS] is j1["ws"]
    assert _empty(a[RED:])                                       # nothing to reduce yet
    assert Q._Pipe.job is j2 and Q._Pipe.red is j1


def test_recurrence_carries_pending_job_and_reduce(ops):
    j1, j2 = _push_two(ops)
    L = _layer()
    dh, g, c = torch.zeros(2, 16, 16), torch.zeros(3, 16, 16, 4), torch.zeros(3, 16, 16)
    del ops.calls[:]
    dx = Q._pipe_tm_backward(dh, g, c, L["x"], L["h"], L["W"], L["U"], L["sinks"], True)
    assert ops.names() == ["lstm_tm_bwd_pipe", "lstm_dx", "lstm_grads_job_ws"]
    a = ops.named("lstm_tm_bwd_pipe")[0]
    assert a[0] is dh and a[1] is g and a[2] is c and a[T_ARG] == 2
    assert a[JOB] is j2["dz"] and a[JOB_WS] is j2["ws"]
    assert a[RED] is j1["ws"] and [a[RED + 2], a[RED + 3], a[RED + 4]] == j1["g"]
    dz_arg, W_arg, x_arg = ops.named("lstm_dx")[0]
    assert W_arg is L["W"] and x_arg is L["x"] and dx is not None
    own = Q._Pipe.job
    assert own["dz"] is dz_arg and own["x"] is L["x"] and (own["period"], own["hshift"]) == (2 * 16, 16)
    assert Q._Pipe.red is j2


@pytest.mark.parametrize("H_job, alone", [(16, False), (32, False), (64, True), (128, True)])
def test_job_of_another_width_is_drained_alone(ops, H_job, alone):
    j = _job(H=H_job)
    Q._pipe_push(j)
    L = _layer(H=16)
    dh, g, c = torch.zeros(2, 16, 16), torch.zeros(3, 16, 16, 4), torch.zeros(3, 16, 16)
    Q._pipe_tm_backward(dh, g, c, L["x"], L["h"], L["W"], L["U"], L["sinks"], False)
    launches = ops.named("lstm_tm_bwd_pipe")
    assert "lstm_dx" not in ops.names()
    if alone:
        first, rec = launches
        assert _empty(first[REC]) and first[JOB] is j["dz"] and _empty(first[RED:])
        assert rec[0] is dh and rec[JOB].numel() == 0 and rec[RED] is j["ws"]
        assert Q._Pipe.red is None
    else:
        (rec,) = launches
        assert rec[0] is dh and rec[JOB] is j["dz"] and _empty(rec[RED:])
        assert Q._Pipe.red is j


def test_flush_with_a_chain_batch_is_one_launch(ops):
    red, job, b1, b2 = _job(), _job(), _job(H=32), _job(H=64)
    rec_only = dict(ws=torch.zeros(1), W=torch.zeros(4, 128), g=[torch.zeros(1), torch.zeros(1), torch.zeros(1)])
    Q._Pipe.job, Q._Pipe.red = job, red
    Q._Pipe.batch.extend([b1, b2])
    Q._Pipe.reds.append(rec_only)
    gcn_t, gcn_i = [torch.zeros(1)], [1, 2, 3, 4]
    assert Q.defer_to_grads_launch((gcn_t, gcn_i))
    del ops.calls[:]
    Q.pipe_flush()
    assert ops.names() == ["lstm_grads_multi"]
    a = ops.named("lstm_grads_multi")[0]
    grads = [job, b1, b2]
    reds = [red, rec_only, job, b1, b2]
    for pos, key in enumerate(["dz", "x", "h", "W", "period", "hshift", "ws"]):
        same = (lambda u, v: u == v) if key in ("period", "hshift") else (lambda u, v: u is v)
        assert len(a[pos]) == 3 and all(same(got, j[key]) for got, j in zip(a[pos], grads)), key
    assert len(a[7]) == 5 and all(got is r["ws"] for got, r in zip(a[7], reds))
    assert all(got is r["W"] for got, r in zip(a[8], reds))
    for k in range(3):
        assert all(got is r["g"][k] for got, r in zip(a[9 + k], reds))
    assert a[12] is gcn_t and a[13] is gcn_i
    P = Q._Pipe
    assert P.job is None and P.red is None and P.batch == [] and P.reds == [] and P.gcn is None


def test_defer_to_grads_launch_refusals(ops, monkeypatch):
    lists = ([torch.zeros(1)], [0])
    assert not Q.defer_to_grads_launch(lists)                    # no batch pending
    Q._Pipe.batch.append(_job())
    assert Q.defer_to_grads_launch(lists) and Q._Pipe.gcn is lists
    assert not Q.defer_to_grads_launch(lists)                    # a GCN job is queued already
    Q._Pipe.gcn = None
    monkeypatch.setenv("GNNQC_GCN_DEFER", "0")
    assert not Q.defer_to_grads_launch(lists) and Q._Pipe.gcn is None


def test_leaving_direct_accumulation_drains_the_queue(ops, monkeypatch):
    monkeypatch.setattr(Q._DirectGrad, "enabled", False)
    with Q.direct_grad_accumulation(True):
        j1, j2 = _push_two(ops)
        del ops.calls[:]
    first, second = ops.named("lstm_tm_bwd_pipe")
    assert ops.names() == ["lstm_tm_bwd_pipe"] * 2
    assert first[JOB] is j2["dz"] and first[RED] is j1["ws"] and _empty(first[REC])
    assert second[JOB].numel() == 0 and second[RED] is j2["ws"]
    assert Q._Pipe.job is None and Q._Pipe.red is None and not Q._DirectGrad.enabled
    with Q.direct_grad_accumulation(True):
        Q._Pipe.gcn = ([], [])
        del ops.calls[:]
    assert Q._Pipe.gcn is None and ops.calls == []


def test_chain_router(ops):
    before = Q.unflagged_grad_writes()
    L = _layer(H=32)
    ws = torch.zeros(1)
    out = Q._pipe_chain_layer(L["dz"], L["x"], L["h"], L["W"], L["sinks"], (True, True, True), ws)
    assert out == [None, None, None] and ops.calls == []         # records built in the launch: reduce only
    assert len(Q._Pipe.reds) == 1 and Q._Pipe.reds[0]["ws"] is ws and Q._Pipe.reds[0]["W"] is L["W"]
    assert Q._Pipe.reds[0]["g"] == [s for s, _ in L["sinks"]] and Q._Pipe.batch == []
    for n in range(Q._MULTI_MAX - 2):                            # jobs of the tail launch while it has room
        assert len(Q._Pipe.batch) == n
        Q._pipe_chain_layer(L["dz"], L["x"], L["h"], L["W"], L["sinks"], (True, False, True))
    assert len(Q._Pipe.batch) == Q._MULTI_MAX - 2 and ops.names() == ["lstm_grads_job_ws"] * (Q._MULTI_MAX - 2)
    assert (Q._Pipe.batch[0]["period"], Q._Pipe.batch[0]["hshift"]) == (2 * 16, 16)
    del ops.calls[:]
    out = Q._pipe_chain_layer(L["dz"], L["x"], L["h"], L["W"], L["sinks"], (True, True, True))
    (a,) = ops.named("lstm_tm_grads")                            # the next one: its own launch
    assert a[0] is L["dz"] and a[3] is L["W"] and [a[4], a[5], a[6]] == [s for s, _ in L["sinks"]] and a[7] is False
    assert out == [None, None, None] and len(Q._Pipe.batch) == Q._MULTI_MAX - 2
    # gradients that do not go into .grad directly are handed back where they are needed, launched at once
    loose = [(s, False) for s, _ in L["sinks"]]
    del ops.calls[:]
    Q._Pipe.batch.clear()
    out = Q._pipe_chain_layer(L["dz"], L["x"], L["h"], L["W"], loose, (True, False, True))
    assert ops.names() == ["lstm_tm_grads"] and Q._Pipe.batch == []
    assert out[0] is loose[0][0] and out[1] is None and out[2] is loose[2][0]
    # a frozen layer: nothing queued, nothing launched, nothing counted
    n_reds = len(Q._Pipe.reds)
    del ops.calls[:]
    out = Q._pipe_chain_layer(L["dz"], L["x"], L["h"], L["W"], None, (False, False, False))
    assert out == [None, None, None] and ops.calls == []
    assert Q._Pipe.batch == [] and len(Q._Pipe.reds) == n_reds and Q.unflagged_grad_writes() == before


def test_returned_grads():
    a, b, c = torch.zeros(1), torch.zeros(1), torch.zeros(1)
    out = Q.returned_grads([(a, False), (b, True), (c, False)], (True, True, False))
    assert out[0] is a and out[1] is None and out[2] is None


def test_saved_state_view():
    names = ["h", "gates", "c", "pooled", "argmax"]
    tag = {}
    outs = []
    for i in range(3):
        for k, n in enumerate(names):
            t = torch.full((1,), float(5 * i + k))
            tag[(i, n)] = t
            outs.append(t)
    x = torch.full((1,), -1.0)
    st = _ChainSaved(x, outs, (0, 3, 0))
    for i in range(3):
        assert st.h(i) is tag[(i, "h")] and st.gates(i) is tag[(i, "gates")] and st.c(i) is tag[(i, "c")]
        assert st.pooled(i) is tag[(i, "pooled")] and st.argmax(i) is tag[(i, "argmax")]
    assert st.x_in(0) is x
    assert st.x_in(1) is tag[(0, "h")]               # no pool after layer 0
    assert st.x_in(2) is tag[(1, "pooled")]          # layer 1 is pooled
    assert st.x_in(3) is tag[(2, "h")]               # what the layer after the chain reads
