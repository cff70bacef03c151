"""BiocNeighbors-shaped entry points used on the fastMNN path (queryKNN, findMutualNN) and after it (findKNN on the
corrected coordinates, and bluster's makeSNNGraph / neighborsToSNNGraph on its lists), served by the HIP kernels."""
from __future__ import annotations

import ctypes
import dataclasses

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


SNN_TYPES = ("rank", "number", "jaccard")
SNN_MAX_K = 128


@dataclasses.dataclass
class SnnGraph:
    """The shared-nearest-neighbour graph of n cells: edge e joins cells first[e] > second[e] (1-based, int32; ascending
    first, then second) with weight[e] (float64)."""
    n: int
    k: int
    type: str
    first: np.ndarray
    second: np.ndarray
    weight: np.ndarray

    def to_csr(self):
        """The symmetric n x n scipy.sparse.csr_matrix of the weights: both triangles, no diagonal."""
        import scipy.sparse as sp
        i = self.first.astype(np.int64) - 1
        j = self.second.astype(np.int64) - 1
        return sp.coo_matrix((np.concatenate([self.weight, self.weight]), (np.concatenate([i, j]), np.concatenate([j, i]))),
                             shape=(self.n, self.n)).tocsr()


def _snn_type(type):
    if not isinstance(type, str) or type not in SNN_TYPES:
        raise ValueError("'type' must be one of 'rank', 'number', 'jaccard'")
    return SNN_TYPES.index(type)


def _snn_k(n, k):
    k = int(k)
    if n > 1 and not 1 <= k <= min(n - 1, SNN_MAX_K):
        raise ValueError("'k' must be between 1 and min(number of other points, 128)")
    if n > 1 and n * k >= 2 ** 31 - 1:
        raise ValueError("the index has 2^31 entries or more")
    return k


class _LibraryArray:
    """m values the library malloc'ed, as numpy sees them through __array_interface__; freed when the last array over them goes."""

    def __init__(self, ptr, m, dtype):
        self._address = ctypes.cast(ptr, ctypes.c_void_p).value
        self._free = _lib.lib().bmx_free
        self.__array_interface__ = {"version": 3, "shape": (m,), "typestr": np.dtype(dtype).str, "data": (self._address, False)}

    def __del__(self):
        self._free(self._address)


def _adopt(ptr, m, dtype):
    """The library's array as a numpy array WITHOUT a copy: a graph of 100 000 cells at k = 20 is 1.2 GB of edges, and copying
    them once more took longer than building them."""
    if m == 0:
        _lib.lib().bmx_free(ptr)
        return np.zeros(0, dtype=dtype)
    return np.asarray(_LibraryArray(ptr, m, dtype))


def _snn_take(n, k, type, pf, ps, pw, m):
    m = int(m.value)
    return SnnGraph(n=n, k=k, type=type, first=_adopt(pf, m, np.int32), second=_adopt(ps, m, np.int32),
                    weight=_adopt(pw, m, np.float64))


def neighbors_to_snn_graph(index, type="rank"):
    """bluster::neighborsToSNNGraph(index, type=): the graph of a nearest-neighbour index [n x k] -- 1-based, each row's k
    nearest OTHER rows (distinct, never the row itself), what find_knn returns.

    With L(c) = (c, index[c, 0], ..., index[c, k - 1]) at ranks 0..k, cells a > b share an edge exactly when L(a) and L(b) have
    a cell in common; S = their common cells.  "rank": max(k - r / 2, 1e-6) with r the smallest sum of a shared cell's two
    ranks; "number": |S|; "jaccard": |S| / (2 (k + 1) - |S|).  Built on the device; the same input gives the same bytes.
    """
    code = _snn_type(type)
    index = np.asarray(index)
    if index.ndim != 2:
        raise ValueError("'index' must be a matrix")
    if not np.issubdtype(index.dtype, np.integer):
        raise ValueError("'index' must hold integers")
    n, k = index.shape
    k = _snn_k(n, k)
    if index.dtype != np.int32:  # (what does not fit int32 is outside 1..n: 0 says so to the device's check)
        index = np.where((index < 1) | (index > 2 ** 31 - 1), 0, index)
    index = np.asfortranarray(index, dtype=np.int32)
    _lib.require_gpu()
    pf, ps, pw, m = _lib.c_i32p(), _lib.c_i32p(), _lib.c_f64p(), ctypes.c_int64(0)
    _lib.check(_lib.lib().bmx_snn_graph(_lib.i32p(index), n, k, code, ctypes.byref(pf), ctypes.byref(ps), ctypes.byref(pw),
                                        ctypes.byref(m)))
    return _snn_take(n, k, type, pf, ps, pw, m)


def make_snn_graph(X, k=10, type="rank"):
    """bluster::makeSNNGraph(X, k=, type=): neighbors_to_snn_graph of find_knn(X, k)'s index.  X goes to the device once and
    the lists never leave it: the search (find_knn's, at k + 1) and the graph run back to back."""
    code = _snn_type(type)
    X = _lib.as_f(X)
    if X.ndim != 2:
        raise ValueError("'X' must be a matrix")
    n, d = X.shape
    k = _snn_k(n, k)
    if d == 0:
        raise ValueError("'X' has no columns")
    _lib.require_gpu()
    pf, ps, pw, m = _lib.c_i32p(), _lib.c_i32p(), _lib.c_f64p(), ctypes.c_int64(0)
    _lib.check(_lib.lib().bmx_make_snn_graph(_lib.f64p(X), n, d, k, code, ctypes.byref(pf), ctypes.byref(ps), ctypes.byref(pw),
                                             ctypes.byref(m)))
    return _snn_take(n, k, type, pf, ps, pw, m)


def last_snn_spilled_cells():
    """Cells of the last graph whose candidates did not fit one LDS window (the knob "snn_lds_candidates" sets its size)."""
    return _lib.dev_get("snn_spilled_cells")


def last_knn_exact_fallbacks():
    return int(_lib.lib().bmx_last_knn_exact_fallbacks())


def set_force_exact_knn(on):
    _lib.lib().bmx_set_force_exact_knn(ctypes.c_int32(1 if on else 0))
