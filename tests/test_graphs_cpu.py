"""The cursor-graph helper (gnnqc.utils.graphs.CursorGraphs) with nothing captured: the step runs
on the host, reads its row by the cursor and advances it, as the captured steps do on the device."""
import torch


def test_cursor_graphs_uncaptured_walks_the_table():
    from gnnqc.utils.graphs import CursorGraphs
    log = []

    def step(ids):
        row = ids.table[int(ids.cursor[0]) % ids.table.shape[0]].clone()
        log.append(row)
        ids.cursor.add_(1)
        return row

    rows = torch.arange(20, dtype=torch.long).reshape(5, 4)
    cg = CursorGraphs(step, 2, "cpu")
    assert cg.captured is False
    assert cg.load(rows) == (True, True)
    assert cg.table is not rows and torch.equal(cg.table, rows)

    def visited():
        out = [int(r[0]) // 4 for r in log]
        log.clear()
        return out

    n, n1, out = cg.run(3, 5)
    assert (n, n1) == (2, 1) and visited() == [3, 4, 0, 1, 2] and torch.equal(out, rows[2])
    assert cg.run(0, 1)[:2] == (0, 1) and visited() == [0]
    assert cg.run(0, 0) == (0, 0, None) and visited() == []
    assert cg.run(7, 2)[:2] == (1, 0) and visited() == [2, 3]
    assert cg.graph is None and cg.graph1 is None

    assert cg.load(rows) == (False, False)              # the same tensor, unmodified: no copy
    rows[0] += 100                                      # (bumps rows._version)
    assert cg.load(rows) == (True, False)
    assert torch.equal(cg.run(0, 1)[2], torch.arange(100, 104))
    table = cg.table
    assert cg.load(rows.clone()) == (True, False) and cg.table is table     # another tensor, same shape
    assert cg.load(torch.zeros(3, 4, dtype=torch.long)) == (True, True)     # a new shape: new table, graphs dropped
    assert cg.table is not table and cg.table.shape == (3, 4)
    log.clear()
    assert cg.run(4, 1)[:2] == (0, 1) and int(cg.cursor) == 2               # row 4 % 3, then advanced
