"""GPU parity of make_snn_graph / neighbors_to_snn_graph with the host-list reference (tests/snn_graph_ref.py): ends equal, weights
bitwise equal for all three types ("rank" and "number" are exact in double, "jaccard" is one correctly rounded division)."""
import numpy as np
import pytest

from tests.conftest import synth_batches
from tests.find_knn_ref import find_knn_ref
from tests.snn_graph_ref import SNN_TYPES, chain_index, complete_index, hub_index, snn_graph_ref, snn_weights

pytestmark = pytest.mark.gpu

GEOMETRY = [(2000, 20, 1), (2000, 20, 5), (2000, 20, 10), (2000, 20, 20), (2000, 50, 20)]


@pytest.fixture(scope="module")
def nb():
    from batchelor_amd import neighbors
    return neighbors


_cache = {}


def geometry(oracle, n, d, k):
    """(X, the oracle's find_knn index, the reference graph of it): computed once, shared, never written to."""
    key = (n, d, k)
    if key not in _cache:
        X, = synth_batches(1, [n], d)
        index, _ = find_knn_ref(oracle, X, k)
        ref = snn_graph_ref(index)
        for a in (X, index) + ref:
            a.setflags(write=False)
        _cache[key] = (X, index, ref)
    return _cache[key]


def check(g, n, k, type, ref):
    first, second, rank_sum, count = ref
    assert (g.n, g.k, g.type) == (n, k, type)
    assert g.first.dtype == np.int32 and g.second.dtype == np.int32 and g.weight.dtype == np.float64
    assert g.first.shape == g.second.shape == g.weight.shape == first.shape
    assert np.array_equal(g.first, first)
    assert np.array_equal(g.second, second)
    assert np.array_equal(g.weight, snn_weights(k, rank_sum, count, type))


def same_bytes(a, b):
    return (a.first.tobytes() == b.first.tobytes() and a.second.tobytes() == b.second.tobytes() and
            a.weight.tobytes() == b.weight.tobytes())


@pytest.mark.parametrize("n,d,k", GEOMETRY)
def test_make_snn_graph_matches_reference(oracle, nb, n, d, k):
    X, index, ref = geometry(oracle, n, d, k)
    for type in SNN_TYPES:
        g = nb.make_snn_graph(X, k, type=type)
        check(g, n, k, type, ref)
        print("spilled cells", nb.last_snn_spilled_cells())
        if d == 20:
            assert nb.last_snn_spilled_cells() == 0    # the default budget holds every cell (at most 1498 candidates, k = 20)
    print("edges per cell", ref[0].size / n, "most of one cell", np.bincount(ref[0]).max())


@pytest.mark.parametrize("n,d,k", [(2000, 20, 10), (2000, 50, 20)])
def test_make_snn_graph_is_the_graph_of_find_knn(nb, n, d, k):
    X, = synth_batches(1, [n], d)
    index, _ = nb.find_knn(X, k)
    for type in SNN_TYPES:
        assert same_bytes(nb.make_snn_graph(X, k, type=type), nb.neighbors_to_snn_graph(index, type=type))
    # an index of another integer type, row-major
    assert same_bytes(nb.neighbors_to_snn_graph(np.ascontiguousarray(index, dtype=np.int64)), nb.neighbors_to_snn_graph(index))


def tripled_grid_index(nb, k):
    core = np.column_stack([np.repeat(np.arange(1, 11), 10), np.tile(np.arange(1, 11), 10)]).astype(np.float64)
    return nb.find_knn(np.vstack([core, core, core]), k)[0]


CRAFTED = {
    "hub": lambda nb: hub_index(1500, 3),
    "complete": lambda nb: complete_index(12),
    "complete_k128": lambda nb: complete_index(129),
    "two": lambda nb: complete_index(2),
    "chain": lambda nb: chain_index(700, 7),
    "chain_k128": lambda nb: chain_index(160, 128),
    "tripled_grid": lambda nb: tripled_grid_index(nb, 3),
}


def crafted(nb, name):
    """(index, its reference graph): computed once, shared, never written to."""
    if name not in _cache:
        index = CRAFTED[name](nb)
        ref = snn_graph_ref(index)
        for a in (index,) + ref:
            a.setflags(write=False)
        _cache[name] = (index, ref)
    return _cache[name]


@pytest.mark.parametrize("name", list(CRAFTED))
def test_crafted_indices(nb, name):
    index, ref = crafted(nb, name)
    n, k = index.shape
    for type in SNN_TYPES:
        check(nb.neighbors_to_snn_graph(index, type=type), n, k, type, ref)
    if name == "hub":
        # the last cells meet k hubs of in-degree about n: some 4500 candidates, beyond the default budget of 2048
        assert nb.last_snn_spilled_cells() > 0
        assert ref[0].size == n * (n - 1) // 2
    if name == "complete":
        assert ref[0].size == n * (n - 1) // 2 and (ref[3] == n).all()


def test_known_answer(nb):
    index = np.array([[2], [1], [2], [3]], dtype=np.int32)
    want = {"rank": [0.5, 1e-6, 0.5, 0.5], "number": [2.0, 1.0, 1.0, 1.0], "jaccard": [1.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0]}
    for type in SNN_TYPES:
        g = nb.neighbors_to_snn_graph(index, type=type)
        assert g.first.tolist() == [2, 3, 3, 4] and g.second.tolist() == [1, 1, 2, 3]
        assert np.array_equal(g.weight, np.array(want[type]))


def test_empty_graphs(nb):
    for n in (0, 1):
        g = nb.neighbors_to_snn_graph(np.zeros((n, 3), dtype=np.int32))
        assert g.first.size == 0 and g.second.size == 0 and g.weight.size == 0 and g.n == n
        g = nb.make_snn_graph(np.zeros((n, 4)), 3)
        assert g.first.size == 0 and g.weight.dtype == np.float64


@pytest.mark.parametrize("budget", [16, 32, 100])
def test_slow_path_gives_the_same_graph(oracle, nb, dev, budget):
    n, d, k = 2000, 20, 10
    X, index, ref = geometry(oracle, n, d, k)
    default = {type: nb.make_snn_graph(X, k, type=type) for type in SNN_TYPES}
    assert nb.last_snn_spilled_cells() == 0
    dev("snn_lds_candidates", budget)
    for type in SNN_TYPES:
        g = nb.make_snn_graph(X, k, type=type)
        spilled = nb.last_snn_spilled_cells()
        print("budget", budget, "spilled cells", spilled)
        assert spilled > 0
        if budget <= 32:
            assert spilled > n // 2            # most cells: about 100 candidates below the cell on average
        assert same_bytes(g, default[type])
        check(g, n, k, type, ref)
    h = nb.neighbors_to_snn_graph(index)
    assert nb.last_snn_spilled_cells() > 0 and same_bytes(h, default["rank"])
    dev("snn_lds_candidates", 0)
    nb.make_snn_graph(X, k)
    assert nb.last_snn_spilled_cells() == 0


def test_slow_path_on_the_hub_and_long_rows(nb, dev):
    for name, budget in (("hub", 4), ("chain_k128", 130), ("complete_k128", 129)):
        index, ref = crafted(nb, name)
        n, k = index.shape
        dev("snn_lds_candidates", budget)      # (below k + 1 the library takes k + 1)
        check(nb.neighbors_to_snn_graph(index, type="jaccard"), n, k, "jaccard", ref)
        assert nb.last_snn_spilled_cells() > 0


def test_two_runs_give_the_same_bytes(oracle, nb):
    X, index, ref = geometry(oracle, 2000, 50, 20)
    for type in SNN_TYPES:
        assert same_bytes(nb.make_snn_graph(X, 20, type=type), nb.make_snn_graph(X, 20, type=type))
    hub, _ = crafted(nb, "hub")
    assert same_bytes(nb.neighbors_to_snn_graph(hub), nb.neighbors_to_snn_graph(hub))


def test_input_errors(nb):
    from batchelor_amd import BatchelorMI355XError
    good = chain_index(200, 5)
    for v in (0, 201, -3, 2 ** 40):
        bad = good.astype(np.int64)
        bad[17, 2] = v
        with pytest.raises(BatchelorMI355XError, match="entry outside 1..n") as err:
            nb.neighbors_to_snn_graph(bad)
        assert err.value.code == -6
    bad = good.copy()
    bad[150, 4] = 151
    with pytest.raises(BatchelorMI355XError, match="lists itself") as err:
        nb.neighbors_to_snn_graph(bad)
    assert err.value.code == -6
    bad = good.copy()
    bad[199, 0] = bad[199, 3]
    with pytest.raises(BatchelorMI355XError, match="lists a row twice") as err:
        nb.neighbors_to_snn_graph(bad)
    assert err.value.code == -6
    wide = chain_index(300, 129)
    with pytest.raises(ValueError):
        nb.neighbors_to_snn_graph(wide)
    with pytest.raises(ValueError):
        nb.make_snn_graph(np.zeros((300, 3)), 129)
    # the library is in order after the refusals
    check(nb.neighbors_to_snn_graph(good), 200, 5, "rank", snn_graph_ref(good))


def test_k_beyond_128_is_refused_by_the_library(nb):
    import ctypes
    from batchelor_amd import _lib
    wide = np.asfortranarray(chain_index(300, 129))
    pf, ps, pw, m = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64(0)
    rc = _lib.lib().bmx_snn_graph(_lib.i32p(wide), 300, 129, 0, ctypes.byref(pf), ctypes.byref(ps), ctypes.byref(pw), ctypes.byref(m))
    assert rc == -6 and "'k' must be between 1 and min(n - 1, 128)" in _lib.lib().bmx_last_error().decode()


def test_to_csr(oracle, nb):
    X, index, ref = geometry(oracle, 2000, 20, 10)
    g = nb.make_snn_graph(X, 10, type="number")
    A = g.to_csr()
    m = g.first.size
    assert A.shape == (2000, 2000) and A.nnz == 2 * m
    assert (A != A.T).nnz == 0
    assert (A.diagonal() == 0).all()
    assert np.array_equal(np.asarray(A[g.first - 1, g.second - 1]).ravel(), g.weight)
    # "number" is what the membership matrix's product with its transpose holds off the diagonal
    import scipy.sparse as sp
    members = np.concatenate([np.arange(2000)[:, None], index.astype(np.int64) - 1], axis=1)
    M = sp.csr_matrix((np.ones(members.size), (np.repeat(np.arange(2000), 11), members.ravel())), shape=(2000, 2000))
    P = M @ M.T
    P = (P - sp.diags(P.diagonal())).tocsr()
    P.eliminate_zeros()
    assert (P != A).nnz == 0
