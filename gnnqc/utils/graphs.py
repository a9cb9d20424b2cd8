"""HIP-graph plumbing shared by training, inference and attribution.

* :func:`graph_upload` - ``hipGraphUpload`` of a captured graph;
* :func:`capture_graph` - warm up on a side stream, join, capture into a new graph;
* :class:`CursorGraphs` - a device table of batch ids ``[rows, B]`` walked by a device cursor: a
  graph of ``steps`` steps and a one-step graph of the same form for the leftover steps, both
  reading their ids through one :class:`gnnqc.data.store.CursorIds`.
"""
from __future__ import annotations

import contextlib
import gc

import torch

from ..data.store import CursorIds


def graph_upload(graph) -> bool:
    """hipGraphUpload of a captured graph's executable on the current stream: the first replay of a
    graph otherwise pays the upload of its command buffers (done here, outside any timed region).
    False when the runtime or the executable handle is not available (no effect then)."""
    if graph is None or not torch.cuda.is_available():
        return False
    try:
        import ctypes
        exe = graph.raw_cuda_graph_exec()
        lib = ctypes.CDLL("libamdhip64.so")
        rc = lib.hipGraphUpload(ctypes.c_void_p(int(exe)), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        return rc == 0
    except Exception:         # (older torch / no HIP runtime: the first replay uploads instead)
        return False


def capture_graph(body, warm=None, warmups: int = 2, before_capture=None, thread_local: bool = False):
    """``(graph, body())``: ``warm`` (default ``body``) runs ``warmups`` times on a fresh side stream
    (allocator + lazy initialisation), the side stream is joined, ``before_capture`` runs if given,
    then ``body`` is captured on the current stream into a new graph with a memory pool of its own.
    What ``body`` returned are the tensors every replay refreshes. ``thread_local``: thread-local
    capture mode (a process group's watchdog thread keeps polling its own events meanwhile)."""
    if warmups:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmups):
                (warm or body)()
        torch.cuda.current_stream().wait_stream(side)
    if before_capture is not None:
        before_capture()
    graph = torch.cuda.CUDAGraph()
    # No cyclic garbage collection may run between capture_begin and capture_end: a dead cycle that
    # holds an earlier CUDAGraph (a dropped Trainer / Predictor) is destroyed by whichever thread the
    # collector happens to run on - the autograd worker too - and releasing a graph's memory pool is
    # a runtime call a capturing stream does not allow; the error is raised in a destructor and ends
    # the process. torch.cuda.graph() collected before capture_begin up to torch 2.8 and no longer
    # does, so: collect now, and keep the collector off until the capture has ended.
    gc.collect()
    gc_on = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph, **({"capture_error_mode": "thread_local"} if thread_local else {})):
            out = body()
    finally:
        if gc_on:
            gc.enable()
    return graph, out


class CursorGraphs:
    """``step(ids)`` is one step that reads its batch ids through ``ids`` (row ``cursor % rows`` of
    ``table``) and advances the cursor itself, on the device. :meth:`run` replays ``k`` of them:
    ``graph`` (``steps`` steps a replay) ``k // steps`` times, then ``graph1`` (one step)
    ``k % steps`` times. ``out`` / ``out1`` are what ``step`` last returned inside each capture.
    Without ``use_graph`` (and off the GPU) nothing is captured and :meth:`run` calls ``step``."""

    def __init__(self, step, steps: int, device, use_graph: bool = True):
        self.step = step
        self.steps = max(1, int(steps))
        self.captured = bool(use_graph) and torch.device(device).type == "cuda"
        self.cursor = torch.zeros(1, dtype=torch.long, device=device)
        self.table = self.ids = self._src = None
        self.graph = self.graph1 = self.out = self.out1 = None

    def load(self, rows: torch.Tensor):
        """Make ``rows`` [rows, B] the table: ``(copied, dropped)``. A new shape allocates the table
        and drops both graphs; the copy is skipped when the table already holds exactly these rows
        (same tensor, unmodified since): a copy launch and its gap less per call."""
        dropped = self.table is None or self.table.shape != rows.shape
        if dropped:
            self.table = torch.empty(rows.shape, dtype=torch.long, device=self.cursor.device)
            self.ids, self._src = CursorIds(self.table, self.cursor), None
            self.graph = self.graph1 = self.out = self.out1 = None
        # (the source is kept referenced, so no other tensor can take its memory and pass as it)
        copied = self._src is None or self._src[0] is not rows or self._src[1] != rows._version
        if copied:
            self.table.copy_(rows, non_blocking=True)
            self._src = (rows, rows._version)
        return copied, dropped

    def holds(self, rows: torch.Tensor) -> bool:
        """Graphs exist and were captured over a table of ``rows``' shape."""
        return self.graph is not None and self.table.shape == rows.shape

    def capture(self, warm=None, scope=contextlib.nullcontext, upload: bool = False, **kw):
        """Capture the ``steps``-step graph, then the one-step graph, each by :func:`capture_graph`
        (``warm`` takes the ids as ``step`` does; ``kw``: its ``warmups``, ``before_capture``,
        ``thread_local``) inside a ``scope()`` context of its own, and upload each if asked to."""
        def one(n):
            with scope():
                graph, out = capture_graph(lambda: [self.step(self.ids) for _ in range(n)][-1],
                                           warm=warm and (lambda: warm(self.ids)), **kw)
            if upload:
                graph_upload(graph)
            return graph, out

        self.graph, self.out = one(self.steps)
        self.graph1, self.out1 = one(1)

    def run(self, start: int, k: int):
        """``k`` steps from row ``start % rows``: ``(full replays, one-step replays, result)`` with
        the result of the graph that ran last (uncaptured: of the last step, None when ``k`` is 0)."""
        self.cursor.fill_(start % self.table.shape[0])
        n, n1 = divmod(k, self.steps)
        if not self.captured:
            out = None
            for _ in range(k):
                out = self.step(self.ids)
            return n, n1, out
        for _ in range(n):
            self.graph.replay()
        for _ in range(n1):
            self.graph1.replay()
        return n, n1, (self.out1 if n1 or not n else self.out)
