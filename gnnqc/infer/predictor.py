"""Graph-replayed inference: score every window of a loader with no host work between batches.

:func:`gnnqc.train.engine.predict` is a Python loop: per batch it cuts the full ``[B,T,N,C]``
window (adjacency and masks included, even for the baseline, which reads one node), runs the
model's generic ``forward`` and appends to a list. :class:`Predictor` runs the same scoring as a
HIP graph of ``steps_per_graph`` steps that walks a device table of batch ids:

* ``gcn_store`` (CML GCN): ``gcn_fused_fwd`` straight from the resident store (moving BatchNorm
  statistics) -> the headed LSTM chain (``lstm_chain_head_fwd``, ``train=false``) -> ``predict_emit``;
* ``baseline_store`` (per-sensor baseline): ``series_tm_gather`` writes the flagged sensor's
  normalised window as the time-major LSTM input -> headed chain -> ``predict_emit``;
* ``generic`` (everything else): ``store.gather`` -> ``model(inputs)`` -> ``predict_emit``.

``predict_emit`` writes the step's row of the output tables and advances the device cursor that
every step's front end reads its batch ids by. The batches left over after the full multi-step
replays replay a one-step graph of the same form. One device-to-host copy per output table ends
the pass. The graph reads parameters and moving statistics by address: in-place weight updates
(training between two passes) need no recapture.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..data.store import CursorIds
from ..ops import use_hip
from ..parallel import dist as D
from ..utils.graphs import CursorGraphs


def series_tm_gather(store, ids):
    """The per-sensor baseline's batch straight from the resident store: ``(h [T, Mp, Cp], y [B],
    y_mask [B], wid [B])`` with ``h`` the flagged sensor's normalised window as the time-major,
    zero-padded LSTM input (Mp = B rounded up to 16, Cp = C rounded up to 4). ``ids``: window ids
    [B] (-1 = padding) or a :class:`gnnqc.data.store.CursorIds`. Only node ``max(anom_pos, 0)`` of
    each window is read (``predict.hip``; plain torch off the GPU)."""
    cur = ids if isinstance(ids, CursorIds) else None
    if use_hip(store.series) and store.series.dtype == torch.float32:
        from ..utils.native import hip_ops
        e = store.series.new_zeros(0, dtype=torch.long)
        idt = (e, cur.table, cur.cursor) if cur is not None else (ids.to(store.device).long().contiguous(), e, None)
        return tuple(hip_ops().series_tm_gather(store.series, store.shift, store.scale, store.win_group,
                                                store.win_center, store.win_valid_u8, store.win_label,
                                                store.group_anom_pos, *idt, store.tb, store.seq_len,
                                                store.time_varying_norm))
    wids = cur.table[cur.cursor[0] % cur.table.shape[0]] if cur is not None else ids
    wids = wids.to(store.device).long()
    live = (wids >= 0).to(torch.float32)
    w = wids.clamp(min=0)
    g = store.win_group[w]
    c = store.win_center[w]
    n0 = store.group_anom_pos[g].clamp(min=0)
    v = live * store.win_valid[w, n0].to(torch.float32)
    t = c[:, None] + store.t_offsets[None, :]                          # [B, T]
    x = store.series[g[:, None], t, n0[:, None]].float()               # [B, T, C]
    tc = c if store.time_varying_norm else torch.zeros_like(c)
    x = (x - store.shift[g, tc, n0][:, None]) * store.scale[g, tc, n0][:, None] * v[:, None, None]
    B, T, C = x.shape
    h = x.new_zeros(T, (B + 15) // 16 * 16, (C + 3) // 4 * 4)
    h[:, :B, :C] = x.transpose(0, 1)
    return h, store.win_label[w] * live, live, wids


def predict_emit(vals, logits: bool, y, mask, wid, p_out, y_out, mask_out, wid_out, cursor):
    """Output stage of one scoring step: row ``cursor[0]`` of the tables ``p_out, y_out, mask_out
    [rows_out, R]`` and ``wid_out [rows_out, B]`` takes ``sigmoid(vals)`` (``logits``) or ``vals``,
    ``y``, ``mask`` and ``wid``; a cursor at or past ``rows_out`` writes nothing. Then the cursor
    advances by one (``predict.hip``: on the device, as the last act of the launch)."""
    vals, y, mask = (t.reshape(-1).float().contiguous() for t in (vals, y, mask))
    if use_hip(vals):
        from ..utils.native import hip_ops
        hip_ops().predict_emit(vals, bool(logits), y, mask, wid.contiguous(), p_out, y_out, mask_out, wid_out, cursor)
        return
    r = int(cursor[0].item())
    if 0 <= r < p_out.shape[0]:
        p_out[r] = torch.sigmoid(vals) if logits else vals
        y_out[r] = y
        mask_out[r] = mask
        wid_out[r] = wid
    cursor += 1


class Predictor:
    """Scores loaders of ``store`` windows with ``model``; :meth:`predict` returns what
    :func:`gnnqc.train.engine.predict` returns. ``path`` names the scoring step that ran
    (``"gcn_store" | "baseline_store" | "generic"``), ``graphed`` whether the last pass replayed
    a captured HIP graph (``use_graph=False`` and CPU devices run the same steps uncaptured)."""

    def __init__(self, model, store, baseline: bool = False, steps_per_graph: int = 8, use_graph: bool = True):
        self.model = model
        self.store = store
        self.baseline = bool(baseline)
        self.device = store.device
        self.steps_per_graph = max(1, int(steps_per_graph))
        # (a store whose gather is not one HIP launch reads the cursor on the host: never captured)
        self.use_graph = (bool(use_graph) and self.device.type == "cuda" and use_hip(store.series)
                          and store.series.dtype == torch.float32)
        self.graphed = False
        self._steps = CursorGraphs(self._step, self.steps_per_graph, self.device, self.use_graph)
        self._out = None
        self._path: Optional[str] = None

    graph = property(lambda self: self._steps.graph)
    graph1 = property(lambda self: self._steps.graph1)

    # ---------------------------------------------------------------- the scoring step
    @property
    def path(self) -> str:
        if self._path is None:
            self._path = self._choose_path()
        return self._path

    def _choose_path(self) -> str:
        model, store = self.model, self.store
        was = model.training
        model.eval()
        try:
            if not self.baseline and hasattr(model, "store_fused_ok") and model.store_fused_ok(store):
                return "gcn_store"
            if (self.baseline and getattr(model, "per_sensor", False) and store.per_sensor
                    and store.win_label.dim() == 1 and hasattr(model, "time_layer")
                    and (not store.series.is_cuda or (use_hip(store.series) and store.series.dtype == torch.float32))):
                return "baseline_store"
            return "generic"
        finally:
            model.train(was)

    def _baseline_headed(self, h) -> bool:
        """The 64-64-1 head behind an LSTM branch the headed chain launch takes whole."""
        m = self.model
        spec = m.head_spec() if hasattr(m, "head_spec") else None
        if spec is None or not h.is_cuda:
            return False
        d1, d2, do = spec[:3]
        return (tuple(d1.kernel.shape) == (128, 64) and tuple(d2.kernel.shape) == (64, 64)
                and tuple(do.kernel.shape) == (64, 1) and m.time_layer.head_chain_ok(h))

    def _step(self, ids: CursorIds):
        """One batch: front end by the device cursor -> model -> row ``cursor`` of the output tables."""
        m, st = self.model, self.store
        if self.path == "gcn_store":
            _, z, y, ym, wid = m.fused_store_loss(st, ids, 1.0, 1.0, return_batch=True)
            logits = True
        elif self.path == "baseline_store":
            h, y, ym, wid = series_tm_gather(st, ids)
            B = int(wid.shape[0])
            if self._baseline_headed(h):
                spec = m.head_spec()
                _, z = m.time_layer.forward_time_major_head(h, B, spec[:3], spec[3:], y, ym, 1.0, 1.0)
            else:
                z = m.head(m.time_layer.forward_time_major(h, B))
            logits = True
        else:
            b = st.gather(ids)
            z = m(b.model_inputs(st.ds_type, self.baseline))
            y, ym, wid = b.y, b.y_mask, b.wid
            logits = False
        predict_emit(z, logits, y, ym, wid, *self._out, ids.cursor)

    # ---------------------------------------------------------------- tables and graph
    def _prepare(self, rows: torch.Tensor):
        """Device id table and output tables for these batches; (re)captures the graphs when the
        table shape changed. The table is not padded: the steps left over after the full
        ``steps_per_graph``-step replays replay a one-step graph of the same form (same table,
        same cursor), so no all-padding batch is ever scored."""
        cg = self._steps
        if cg.load(rows)[1]:
            nb, B = int(rows.shape[0]), int(rows.shape[1])
            R = B if self.store.per_sensor else B * self.store.n_nodes
            dev = self.device
            self._out = (torch.zeros(nb, R, device=dev), torch.zeros(nb, R, device=dev),
                         torch.zeros(nb, R, device=dev), torch.full((nb, B), -1, dtype=torch.long, device=dev))
        if cg.graph is None:                  # (always so when nothing is captured)
            self._touch_store_tables()
            if cg.captured:
                # (every warm-up step starts at row 0; thread-local capture mode: a process group's
                # watchdog thread keeps polling its events)
                cg.capture(warm=lambda ids: (ids.cursor.zero_(), self._step(ids)), upload=True,
                           thread_local=D.is_initialized())

    def _touch_store_tables(self):
        # per-window tables of the fused GCN front end: computed on first use, never inside a capture
        if self.path == "gcn_store":
            g = self.model.gcn_layer
            pooling = "selection" if self.model.pooling_type == "selection" else self.model.aggregation_type
            self.store.gcn_fused_data(g.aggregate == "mean", {"mean": 0, "sum": 1, "selection": 2}[pooling])

    # ---------------------------------------------------------------- the pass
    @torch.no_grad()
    def predict(self, loader, gather_all: bool = True):
        """Probabilities, labels, label mask and window id of every window in ``loader`` (host
        numpy; SoilNet: per (window, node), with ``node``), rows in the loader's batch order,
        padding slots included (``wid == -1``, ``mask == 0``)."""
        model, store = self.model, self.store
        was_training = model.training
        model.eval()
        try:
            rows = loader.batch_ids()
            nb = int(rows.shape[0]) if torch.is_tensor(rows) and rows.dim() == 2 else 0
            self.graphed = False
            if nb:
                rows = rows.to(self.device)
                self._prepare(rows)
                self._steps.run(0, nb)              # (from a cursor of zero: step i writes output row i)
                self.graphed = self.use_graph
        finally:
            if was_training:
                model.train()
        if self.device.type == "cuda":
            from ..ops.lstm import check_chain
            check_chain(self.device)
        N = () if store.per_sensor else (store.n_nodes,)
        if nb:
            B = int(rows.shape[1])
            p, y, m = (t[:nb].reshape(nb * B, *N) for t in self._out[:3])
            w = self._out[3][:nb].reshape(nb * B)
        else:                               # no batch on this rank (e.g. a tiny held-out fold)
            p = y = m = torch.zeros((0, *N), device=self.device)
            w = torch.zeros(0, dtype=torch.long, device=self.device)
        if gather_all:
            p, y, m, w = (D.all_gather_var(t) for t in (p, y, m, w))
        # one device-to-host copy per table (a host store's tables are copied: the next pass reuses them)
        p, y, m, w = ((t.cpu() if t.is_cuda else t.clone()).numpy() for t in (p, y, m, w))
        out = {"p": p, "y": y, "mask": m, "wid": w}
        if not store.per_sensor:
            out["node"] = np.broadcast_to(np.arange(out["p"].shape[1]), out["p"].shape).copy()
        return out


__all__ = ["Predictor", "predict_emit", "series_tm_gather"]
