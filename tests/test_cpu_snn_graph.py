"""makeSNNGraph without a GPU: the host-list reference (tests/snn_graph_ref.py) equals a brute-force set intersection over all
pairs, gives the known answer, the entry points are declared and exported, and bad arguments are refused before any device is
asked for."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.snn_graph_ref import (SNN_TYPES, chain_index, complete_index, hub_index, snn_brute_force, snn_graph_ref,
                                 snn_weights)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOWN_INDEX = np.array([[2], [1], [2], [3]], dtype=np.int32)
KNOWN_FIRST = [2, 3, 3, 4]
KNOWN_SECOND = [1, 1, 2, 3]
KNOWN_WEIGHTS = {"rank": [0.5, 1e-6, 0.5, 0.5], "number": [2.0, 1.0, 1.0, 1.0], "jaccard": [1.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0]}


def nearest_others(X, k):
    """1-based brute-force index: each row's k nearest other rows, ties to the lower row."""
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d2, np.inf)
    return (np.argsort(d2, axis=1, kind="stable")[:, :k] + 1).astype(np.int32)


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("k", [1, 3, 10])
def test_reference_equals_brute_force_on_geometry(k):
    rng = np.random.default_rng(20250314 + k)
    X = rng.standard_normal((300, 5)) / np.sqrt(1.0 + np.arange(5) / 5.0)
    index = nearest_others(X, k)
    ref = snn_graph_ref(index)
    assert same(ref, snn_brute_force(index))
    first, second, rank_sum, count = ref
    assert first.dtype == np.int32 and second.dtype == np.int32
    assert (first > second).all()
    order = np.lexsort((second, first))
    assert np.array_equal(order, np.arange(first.size))
    assert (count >= 1).all() and (count <= k + 1).all() and (rank_sum >= 0).all() and (rank_sum <= 2 * k).all()
    # every cell is joined to the cells it lists (the listed cell is in both lists)
    edges = set(zip(first.tolist(), second.tolist()))
    for c in range(300):
        for v in index[c]:
            assert (max(c + 1, int(v)), min(c + 1, int(v))) in edges


@pytest.mark.parametrize("index", [hub_index(120, 3), hub_index(40, 1), chain_index(50, 3), chain_index(11, 10),
                                   complete_index(11), complete_index(2), complete_index(4)],
                         ids=["hub3", "hub1", "chain3", "chain10", "complete11", "two", "complete4"])
def test_reference_equals_brute_force_on_crafted_indices(index):
    n, k = index.shape
    assert not (index == np.arange(1, n + 1)[:, None]).any()
    assert all(len(set(row)) == k for row in index.tolist())
    assert same(snn_graph_ref(index), snn_brute_force(index))


def test_hub_has_in_degree_about_n():
    index = hub_index(120, 3)
    assert (index == 1).sum() == 119 and (index == 3).sum() == 119
    first, second, rank_sum, count = snn_graph_ref(index)
    assert first.size == 120 * 119 // 2          # every pair shares a hub


@pytest.mark.parametrize("type", SNN_TYPES)
def test_known_answer(type):
    for graph in (snn_graph_ref, snn_brute_force):
        first, second, rank_sum, count = graph(KNOWN_INDEX)
        assert first.tolist() == KNOWN_FIRST and second.tolist() == KNOWN_SECOND
        w = snn_weights(1, rank_sum, count, type)
        assert w.dtype == np.float64
        assert np.array_equal(w, np.array(KNOWN_WEIGHTS[type]))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from batchelor_amd import _lib
    L = _lib.lib()
    L.bmx_snn_graph.restype = ctypes.c_int32
    L.bmx_make_snn_graph.restype = ctypes.c_int32
    return L


def test_header_declares_and_library_exports_the_entry_points(lib):
    header = open(os.path.join(ROOT, "include", "batchelor_mi355x.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert "bmx_snn_graph(" in header and "bmx_make_snn_graph(" in header
    assert hasattr(lib, "bmx_snn_graph") and hasattr(lib, "bmx_make_snn_graph")


@pytest.mark.parametrize("n,k,type", [(10, 0, 0), (10, 10, 0), (10, -1, 0), (200, 129, 0), (10, 3, 3), (10, 3, -1), (-1, 3, 0)])
def test_c_entries_refuse_before_any_device(lib, n, k, type):
    index = np.ones((max(n, 1), max(k, 1)), dtype=np.int32, order="F")
    X = np.zeros((max(n, 1), 3), order="F")
    pf, ps, pw, m = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64(-7)
    out = (ctypes.byref(pf), ctypes.byref(ps), ctypes.byref(pw), ctypes.byref(m))
    for rc in (lib.bmx_snn_graph(index.ctypes.data_as(ctypes.c_void_p), n, k, type, *out),
               lib.bmx_make_snn_graph(X.ctypes.data_as(ctypes.c_void_p), n, 3, k, type, *out)):
        assert rc == -6      # BMX_ERR_ARG
        assert lib.bmx_last_error().decode().startswith("makeSNNGraph:")
        assert m.value == -7 and pf.value is None
    assert lib.bmx_make_snn_graph(X.ctypes.data_as(ctypes.c_void_p), 10, 0, 3, 0, *out) == -6


def test_c_entries_give_an_empty_graph_below_two_cells(lib):
    for n in (0, 1):
        pf, ps, pw, m = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64(-7)
        assert lib.bmx_snn_graph(None, n, 5, 0, ctypes.byref(pf), ctypes.byref(ps), ctypes.byref(pw), ctypes.byref(m)) == 0
        assert m.value == 0
        for p in (pf, ps, pw):
            assert p.value is not None
            lib.bmx_free(p)


def test_python_refuses_before_any_device():
    import batchelor_amd
    from batchelor_amd import neighbors
    assert batchelor_amd.make_snn_graph is neighbors.make_snn_graph
    assert batchelor_amd.neighbors_to_snn_graph is neighbors.neighbors_to_snn_graph
    assert batchelor_amd.SnnGraph is neighbors.SnnGraph
    X = np.arange(30.0).reshape(10, 3)
    index = chain_index(10, 3)
    for bad in (np.zeros(10), np.zeros((2, 5, 3))):
        with pytest.raises(ValueError):
            neighbors.make_snn_graph(bad, 1)                    # X not a matrix
    with pytest.raises(ValueError):
        neighbors.make_snn_graph(np.zeros((10, 0)), 2)          # no columns
    for k in (0, -1, 10, 129):
        with pytest.raises(ValueError):
            neighbors.make_snn_graph(X, k)                      # k outside [1, min(n - 1, 128)]
    with pytest.raises(ValueError):
        neighbors.make_snn_graph(np.zeros((200, 3)), 129)
    for type in ("Rank", "weighted", None, 0):
        with pytest.raises(ValueError):
            neighbors.make_snn_graph(X, 3, type=type)
        with pytest.raises(ValueError):
            neighbors.neighbors_to_snn_graph(index, type=type)
    with pytest.raises(ValueError):
        neighbors.neighbors_to_snn_graph(index[:, 0])           # not a matrix
    with pytest.raises(ValueError):
        neighbors.neighbors_to_snn_graph(index.astype(np.float64))   # not integers
    with pytest.raises(ValueError):
        neighbors.neighbors_to_snn_graph(np.ones((10, 10), dtype=np.int32))   # k > n - 1
    with pytest.raises(ValueError):
        neighbors.neighbors_to_snn_graph(np.ones((10, 0), dtype=np.int32))    # k = 0
    with pytest.raises(ValueError):
        neighbors.neighbors_to_snn_graph(np.ones((200, 129), dtype=np.int32))


def test_to_csr_of_the_known_answer():
    from batchelor_amd import SnnGraph
    first, second, rank_sum, count = snn_graph_ref(KNOWN_INDEX)
    g = SnnGraph(n=4, k=1, type="number", first=first, second=second, weight=snn_weights(1, rank_sum, count, "number"))
    A = g.to_csr()
    assert A.shape == (4, 4) and A.nnz == 8
    assert np.array_equal(A.toarray(), np.array([[0, 2, 1, 0], [2, 0, 1, 0], [1, 1, 0, 1], [0, 0, 1, 0]], dtype=np.float64))
