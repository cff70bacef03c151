"""BiocNeighbors-shaped entry points used on the fastMNN path (queryKNN, findMutualNN) and after it (findKNN on the
corrected coordinates), served by the HIP kernels."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .inputs import subset_index


def query_knn(X, query, k, get_index=True, get_distance=True):
    """queryKNN(X, query, k) (call sites R/MNN_tree.R:129 via findMutualNN, R/fastMNN.R:605).

    Returns (index [nq x k] 1-based into rows of X, distance [nq x k] Euclidean), ascending distance, exact.
    """
    _lib.require_gpu()
    X = _lib.as_f(X)
    query = _lib.as_f(query)
    if X.ndim != 2 or query.ndim != 2 or X.shape[1] != query.shape[1]:
        raise ValueError("number of dimensions do not match between 'X' and 'query'")
    nx, d = X.shape
    nq = query.shape[0]
    k = int(k)
    index = np.zeros((nq, k), dtype=np.int32, order="F")
    distance = np.zeros((nq, k), dtype=np.float64, order="F")
    _lib.check(_lib.lib().bmx_query_knn(_lib.f64p(X), nx, _lib.f64p(query), nq, d, k,
                                        _lib.i32p(index) if get_index else None,
                                        _lib.f64p(distance) if get_distance else None))
    return index, distance


def find_knn(X, k, subset=None, get_index=True, get_distance=True):
    """findKNN(X, k, subset=): each row's k nearest OTHER rows of X (or those of the rows `subset` names: 1-based integers in
    any order, repeats kept, or a logical mask over the rows).

    Returns (index [nq x k] 1-based into rows of X, distance [nq x k] Euclidean), ascending distance, exact, ties to the
    lower row.  A row is never in its own list; rows that coincide with it are.  X goes to the device once; the search is
    query_knn's at k + 1 (so k = 36 on at most 61 columns and k = 20 beyond take its partitioned path: exact, slower).
    """
    X = _lib.as_f(X)
    if X.ndim != 2:
        raise ValueError("'X' must be a matrix")
    n, d = X.shape
    k = int(k)
    if k < 0 or k > n - 1:
        raise ValueError("'k' must be between 0 and the number of other points in 'X'")
    rows = subset_index(subset, n)
    if rows is not None and rows.ndim != 1:
        raise ValueError("'subset' must be a vector")
    if d == 0:
        raise ValueError("'X' has no columns")
    _lib.require_gpu()
    nq = n if rows is None else rows.size
    index = np.zeros((nq, k), dtype=np.int32, order="F")
    distance = np.zeros((nq, k), dtype=np.float64, order="F")
    _lib.check(_lib.lib().bmx_find_knn(_lib.f64p(X), n, d, k, None if rows is None else _lib.i32p(rows), nq,
                                       _lib.i32p(index) if get_index else None,
                                       _lib.f64p(distance) if get_distance else None))
    return index, distance


def last_knn_exact_fallbacks():
    return int(_lib.lib().bmx_last_knn_exact_fallbacks())


def set_force_exact_knn(on):
    _lib.lib().bmx_set_force_exact_knn(ctypes.c_int32(1 if on else 0))
