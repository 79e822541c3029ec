"""The queries the covariance tests share (tests/test_pose_graph_cov.py on the CPU, tests/test_gpu_pose_graph_cov.py on the device)
over the graphs of tests/pose_graph_cases.py.  Sources are chosen by row, so that the columns solved are the ones where the lane
sums and the cyclic reduction take another path: the first rows, the rows around the middle, the last rows and, from 1024 rows on,
the rows either side of the lane stride."""
import numpy as np

import pose_graph_oracle as po

MAX_SOURCES = 64


def vertex_of_rows(fixed):
    row, n = po.rows_of(fixed)
    out = np.zeros(n, dtype=np.int64)
    for vtx, r in enumerate(row):
        if r >= 0:
            out[r] = vtx
    return out


def pairs_over(vertices, fixed_vertex):
    """Queries that use every vertex of the list: neighbours in the list, then a == b, a query with a fixed vertex on either side,
    a repeated query, and (b, a) beside (a, b)."""
    v = [int(a) for a in vertices]
    q = [(v[k], v[k + 1]) for k in range(len(v) - 1)] or [(v[0], v[0])]
    a, b = v[0], v[-1]
    q += [(a, a), (b, b), (a, fixed_vertex), (fixed_vertex, b), (fixed_vertex, fixed_vertex), (a, b), (b, a), (a, b)]
    return q


def source_rows(n, count=None):
    """the rows the tests solve for a graph of n rows (count: how many sources, where the test sets it)"""
    if count is not None:                                                   # rows_63 / 64 / 65 with 1, 2 or 64 sources
        first = [r for r in (0, 1, 31, 32, n - 2, n - 1) if 0 <= r < n]
        rows = list(dict.fromkeys(first))[:count]
        run = [r for r in range(2, n) if r not in rows]                      # a run of rows fills the count
        return rows + run[:max(0, min(count, n, MAX_SOURCES) - len(rows))]
    if n >= 1000:
        return list(dict.fromkeys(r for r in (0, min(1023, n - 1), n - 1)))
    return list(dict.fromkeys(r for r in (0, 1, n // 2, n - 2, n - 1) if 0 <= r < n))


def queries_for(case, count=None):
    """(queries, the vertices of the sources expected, in order)"""
    fixed = case["fixed"]
    N = len(fixed)
    by_row = vertex_of_rows(fixed)
    n = len(by_row)
    fixed_vertex = int(np.flatnonzero(np.asarray(fixed) != 0)[0])
    if n <= 11 and count is None:
        q = [(a, b) for a in range(N) for b in range(N)]
    elif 63 <= n <= 65 and count is None:
        q = pairs_over(by_row[source_rows(n, MAX_SOURCES)], fixed_vertex)
    else:
        q = pairs_over(by_row[source_rows(n, count)], fixed_vertex)
    seen = []
    for a, b in q:
        for vtx in (a, b):
            if not fixed[vtx] and vtx not in seen:
                seen.append(vtx)
    return q, seen
