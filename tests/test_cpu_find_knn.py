"""findKNN without a GPU: the entry point is declared and exported, refuses bad arguments before it asks for a device, and
the rule it applies on the device (search at k + 1, drop the row itself -- or the last entry where the row is not in its own
list) equals a brute-force search that skips the row."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.find_knn_ref import drop_self, find_knn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from batchelor_amd import _lib
    L = _lib.lib()
    L.bmx_find_knn.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                               ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    L.bmx_find_knn.restype = ctypes.c_int32
    return L


def test_header_declares_and_library_exports_find_knn(lib):
    header = open(os.path.join(ROOT, "include", "batchelor_mi355x.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert "bmx_find_knn(" in header
    assert hasattr(lib, "bmx_find_knn")


@pytest.mark.parametrize("n,d,k,subset,n_subset", [
    (-1, 3, 0, None, 0),            # negative sizes
    (10, 3, -1, None, 0),
    (10, 0, 2, None, 0),            # d <= 0
    (10, -2, 2, None, 0),
    (10, 3, 10, None, 0),           # k > n - 1
    (1, 3, 1, None, 0),
    (0, 3, 0, None, 0),             # (no k with 0 <= k <= n - 1)
    (10, 3, 2, [1, 11, 2], 3),      # a subset index outside [1, n]
    (10, 3, 2, [0], 1),
    (10, 3, 2, [-4, 3], 2),
    (10, 3, 2, [1, 2], -1),         # a subset of negative length
])
def test_c_entry_refuses_before_any_device(lib, n, d, k, subset, n_subset):
    X = np.zeros((max(n, 1), max(d, 1)), order="F")
    index = np.full((12, 12), -7, dtype=np.int32)
    distance = np.full((12, 12), -7.0)
    sub = None if subset is None else np.asarray(subset, dtype=np.int32)
    rc = lib.bmx_find_knn(X.ctypes.data, n, d, k, None if sub is None else sub.ctypes.data, n_subset, index.ctypes.data,
                          distance.ctypes.data)
    assert rc != 0
    assert lib.bmx_last_error().decode().startswith("findKNN:")
    assert (index == -7).all() and (distance == -7.0).all()


def test_python_refuses_before_any_device():
    from batchelor_amd import find_knn
    from batchelor_amd import neighbors
    assert find_knn is neighbors.find_knn
    X = np.arange(30.0).reshape(10, 3)
    with pytest.raises(ValueError):
        find_knn(np.zeros(10), 2)                       # X not 2-D
    with pytest.raises(ValueError):
        find_knn(np.zeros((2, 5, 3)), 1)
    with pytest.raises(ValueError):
        find_knn(X, -1)                                 # k not in [0, n - 1]
    with pytest.raises(ValueError):
        find_knn(X, 10)
    with pytest.raises(ValueError):
        find_knn(X[:1], 1)
    with pytest.raises(ValueError):
        find_knn(X, 2, subset=[1, 11])                  # subset out of range
    with pytest.raises(ValueError):
        find_knn(X, 2, subset=[0, 3])
    with pytest.raises(ValueError):
        find_knn(X, 2, subset=np.ones(9, dtype=bool))   # a mask of the wrong length
    with pytest.raises(ValueError):
        find_knn(X, 2, subset=np.ones(11, dtype=bool))


def tripled_grid_and_random_rows():
    core = np.column_stack([np.repeat(np.arange(1, 11), 10), np.tile(np.arange(1, 11), 10)]).astype(np.float64)
    rng = np.random.default_rng(20250314)
    return np.vstack([core, core, core, rng.uniform(0.0, 11.0, (200, 2))])


def brute_force_skipping_the_row(X, k):
    n = X.shape[0]
    idx = np.zeros((n, k), dtype=np.int64)
    dist = np.zeros((n, k))
    for i in range(n):
        dx = X[:, 0] - X[i, 0]
        dy = X[:, 1] - X[i, 1]
        dd = np.sqrt(dx * dx + dy * dy)
        others = np.delete(np.arange(n), i)
        order = others[np.argsort(dd[others], kind="stable")][:k]  # ascending, ties to the lower row
        idx[i] = order + 1
        dist[i] = dd[order]
    return idx, dist


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_rule_equals_brute_force_search_that_skips_the_row(oracle, k):
    X = tripled_grid_and_random_rows()
    n = X.shape[0]
    idx, dist = find_knn_ref(oracle, X, k)
    assert idx.shape == (n, k) and dist.shape == (n, k) and idx.dtype == np.int32
    bi, bd = brute_force_skipping_the_row(X, k)
    assert np.array_equal(idx, bi)
    assert np.allclose(dist, bd, rtol=1e-13, atol=0.0)
    assert not (idx == np.arange(1, n + 1)[:, None]).any()
    # the second branch of the rule is in the case: rows whose own id is not among their k + 1 nearest
    oi, od = oracle.query_knn(X, X, k + 1)
    absent = drop_self(oi, od, np.arange(1, n + 1))[2]
    print("k", k, "rows absent from their own k + 1 list:", int(absent.sum()))
    if k == 1:
        assert absent.sum() > 0
        assert absent.sum() == 100      # the third copy of every grid point: two lower-numbered copies at distance 0
    # a subset in the caller's order, with repeats, is those rows of the full answer
    sub = np.array([n, 1, 201, 201, 250, 7, 301])
    si, sd = find_knn_ref(oracle, X, k, sub)
    assert np.array_equal(si, idx[sub - 1]) and np.array_equal(sd, dist[sub - 1])
