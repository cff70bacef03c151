"""GPU parity of find_knn (findKNN: each row's k nearest OTHER rows of the same matrix) against the oracle's queryKNN at k + 1
with the row itself dropped (tests/find_knn_ref.py) -- indices equal, distances bitwise, as test_gpu_knn.py holds query_knn."""
import numpy as np
import pytest

from tests.conftest import synth_batches
from tests.find_knn_ref import find_knn_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nb():
    from batchelor_amd import neighbors
    return neighbors


def check(nb, oracle, X, k, subset=None):
    idx, dist = nb.find_knn(X, k, subset=subset)
    ri, rd = find_knn_ref(oracle, X, k, subset)
    assert idx.shape == ri.shape and dist.shape == rd.shape
    assert idx.dtype == np.int32 and dist.dtype == np.float64
    assert idx.flags.f_contiguous and dist.flags.f_contiguous
    assert np.array_equal(idx, ri)
    assert np.array_equal(dist, rd)
    return idx, dist


@pytest.mark.parametrize("n,d,k", [(2000, 50, 20), (700, 10, 5),      # first tier
                                   (300, 2, 1),
                                   (2500, 100, 19),                   # k + 1 = 20: the longest list of rows beyond 61 columns
                                   (2500, 100, 20),                   # one beyond it: the partitioned path
                                   (3000, 20, 35), (3000, 20, 36),    # the same pair for short rows
                                   (1200, 130, 10)])                  # beyond 125 columns: the FP64 scan
def test_find_knn_matches_oracle(oracle, nb, n, d, k):
    X, = synth_batches(1, [n], d)
    idx, _ = check(nb, oracle, X, k)
    assert not (idx == np.arange(1, n + 1)[:, None]).any()


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_find_knn_tripled_grid(oracle, nb, k):
    # every point three times: the third copy of a point is not among its own k + 1 = 2 nearest (ties go to the lower row)
    core = np.column_stack([np.repeat(np.arange(1, 11), 10), np.tile(np.arange(1, 11), 10)]).astype(np.float64)
    X = np.vstack([core, core, core])
    idx, dist = check(nb, oracle, X, k)
    own = np.arange(1, 301)[:, None]
    assert not (idx == own).any()
    # the nearest other rows are the point's copies, lowest row first
    copies = np.sort(np.stack([(own[:, 0] - 1 + 100 * j) % 300 + 1 for j in (1, 2)], axis=1), axis=1)
    assert np.array_equal(idx[:, :min(k, 2)], copies[:, :min(k, 2)])
    assert (dist[:, :min(k, 2)] == 0.0).all()


def test_find_knn_rows_missing_from_their_own_list(oracle, nb):
    # the first 40 rows five times: with k + 1 = 4 the fifth copy (and no other) has four lower-numbered rows at distance 0
    X0, = synth_batches(5, [900 - 160], 50)
    X = np.concatenate([X0[:40]] * 5 + [X0[40:]])
    assert X.shape == (900, 50)
    k = 3
    oi, _ = oracle.query_knn(X, X, k + 1)
    absent = ~(oi == np.arange(1, 901)[:, None]).any(axis=1)
    assert np.array_equal(np.flatnonzero(absent), np.arange(160, 200))
    idx, dist = check(nb, oracle, X, k)
    assert not (idx == np.arange(1, 901)[:, None]).any()
    assert np.array_equal(idx[160:200], np.arange(1, 41)[:, None] + 40 * np.arange(3)[None, :])
    assert (dist[:200] == 0.0).all()


def test_find_knn_subset(oracle, nb):
    n, d, k = 1500, 50, 20
    X, = synth_batches(2, [n], d)
    full_i, full_d = check(nb, oracle, X, k)
    rng = np.random.default_rng(5)
    sub = rng.integers(1, n + 1, 257)
    sub[100:110] = sub[:10]          # repeats
    sub[0], sub[256] = n, 1          # unsorted, both ends
    si, sd = check(nb, oracle, X, k, sub)
    assert np.array_equal(si, full_i[sub - 1]) and np.array_equal(sd, full_d[sub - 1])
    mask = np.zeros(n, dtype=bool)
    mask[np.unique(sub) - 1] = True
    mi, md = check(nb, oracle, X, k, mask)
    ii, idd = nb.find_knn(X, k, subset=np.flatnonzero(mask) + 1)
    assert np.array_equal(mi, ii) and np.array_equal(md, idd)
    assert np.array_equal(mi, full_i[mask]) and np.array_equal(md, full_d[mask])
    ei, ed = nb.find_knn(X, k, subset=np.zeros(0, dtype=np.int64))
    assert ei.shape == (0, k) and ed.shape == (0, k)


def test_find_knn_edges(oracle, nb):
    X, = synth_batches(3, [37], 7)
    for k in (0, 1, 36):
        idx, dist = check(nb, oracle, X, k)
        assert idx.shape == (37, k)
    assert np.array_equal(np.sort(idx, axis=1), np.array([np.delete(np.arange(1, 38), i) for i in range(37)]))  # k = 36
    with pytest.raises(ValueError):
        nb.find_knn(X, 37)
    idx, dist = nb.find_knn(X[:1], 0)
    assert idx.shape == (1, 0) and dist.shape == (1, 0)
    idx, dist = nb.find_knn(X, 5)
    i2, d2 = nb.find_knn(X, 5, get_index=False)
    assert np.array_equal(d2, dist) and not i2.any()
    i3, d3 = nb.find_knn(X, 5, get_distance=False)
    assert np.array_equal(i3, idx) and not d3.any()


def test_find_knn_runs_the_search_of_query_knn(oracle, nb):
    from batchelor_amd import _lib
    X, = synth_batches(1, [2000], 50)
    counters = ("knn_exact_fallbacks", "knn_tier2_queries")
    c0 = [_lib.dev_get(c) for c in counters]
    a = nb.find_knn(X, 20)
    fb_find = nb.last_knn_exact_fallbacks()
    c1 = [_lib.dev_get(c) for c in counters]
    nb.query_knn(X, X, 21)
    c2 = [_lib.dev_get(c) for c in counters]
    assert fb_find == nb.last_knn_exact_fallbacks()
    assert fb_find <= 2000 // 100
    # the counters of this thread's searches count find_knn's as they count query_knn's
    assert [y - x for x, y in zip(c0, c1)] == [y - x for x, y in zip(c1, c2)]
    assert c1[0] - c0[0] == fb_find
    nb.set_force_exact_knn(True)
    try:
        b = nb.find_knn(X, 20)
        assert nb.last_knn_exact_fallbacks() == 2000
    finally:
        nb.set_force_exact_knn(False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_find_knn_reports_its_exact_fallbacks(nb):
    X, = synth_batches(1, [1200], 130)      # beyond 125 columns: every query through the FP64 scan
    nb.find_knn(X, 10, subset=np.arange(1, 301))
    assert nb.last_knn_exact_fallbacks() == 300


def test_query_knn_unchanged_by_the_shared_way_out(oracle, nb):
    X, Q = synth_batches(1, [700, 1300], 10)
    idx, dist = nb.query_knn(X, Q, 5)
    oi, od = oracle.query_knn(X, Q, 5)
    assert np.array_equal(idx, oi) and np.array_equal(dist, od)
    # 4200 x 1000 results >= 2^22: transposed on the device, out through the staging ring
    X, Q = synth_batches(3, [4200, 4200], 10)
    assert 4200 * 1000 >= 1 << 22
    idx, dist = nb.query_knn(X, Q, 1000)
    oi, od = oracle.query_knn(X, Q, 1000)
    assert np.array_equal(idx, oi) and np.array_equal(dist, od)
    for get_index, get_distance in ((False, True), (True, False)):
        i2, d2 = nb.query_knn(X, Q, 1000, get_index=get_index, get_distance=get_distance)
        assert np.array_equal(i2, oi if get_index else np.zeros_like(oi))
        assert np.array_equal(d2, od if get_distance else np.zeros_like(od))


def test_find_knn_large_result_takes_the_device_transposition(oracle, nb):
    # 4200 x 1000 results >= 2^22 for find_knn too (the search at k = 1001)
    X, = synth_batches(3, [4200], 10)
    check(nb, oracle, X, 1000)
