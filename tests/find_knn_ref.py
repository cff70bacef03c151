"""findKNN restated on the oracle's queryKNN: the reference the find_knn tests share (tests/test_cpu_find_knn.py holds the
restatement itself against a brute-force search that skips the row)."""
import numpy as np


def subset_rows(n, subset):
    """0-based query rows of `subset` (None, 1-based integers in the caller's order, or a logical mask over the n rows)."""
    if subset is None:
        return np.arange(n)
    s = np.asarray(subset)
    if s.dtype == bool:
        assert s.size == n
        return np.flatnonzero(s)
    return s.astype(np.int64) - 1


def drop_self(idx, dist, own):
    """The rule: idx / dist [nq x (k + 1)] (1-based, ascending, ties to the lower row) of a search of X against itself, own [nq]
    the 1-based row of each query.  The query's own entry goes and the later ones move up; where it is not among the k + 1
    (k + 1 lower-numbered rows coincide with the query) the last entry goes.  Distances are moved, never recomputed."""
    nq, k1 = idx.shape
    hit = idx == own[:, None]
    assert (hit.sum(axis=1) <= 1).all()
    pos = np.where(hit.any(axis=1), hit.argmax(axis=1), k1 - 1)
    keep = np.arange(k1)[None, :] != pos[:, None]
    return idx[keep].reshape(nq, k1 - 1), dist[keep].reshape(nq, k1 - 1), ~hit.any(axis=1)


def find_knn_ref(oracle, X, k, subset=None):
    """(index [nq x k] int32 1-based, distance [nq x k]) = oracle.query_knn(X, X[rows], k + 1) without each row itself."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    rows = subset_rows(X.shape[0], subset)
    assert 0 <= k <= X.shape[0] - 1
    if k == 0 or rows.size == 0:
        return np.zeros((rows.size, k), dtype=np.int32), np.zeros((rows.size, k))
    idx, dist = oracle.query_knn(X, X[rows], k + 1)
    i, dd, _ = drop_self(idx, dist, rows + 1)
    return i.astype(np.int32), dd
