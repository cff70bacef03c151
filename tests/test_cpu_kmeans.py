"""kmeans() without a GPU: the numpy restatement (tests/kmeans_ref.py) against scipy's Lloyd, its errors and tie rule,
KmeansParam, the argument errors of kmeans() and of clusterMNN(clusters=KmeansParam) that are raised before any device
work, and the new symbols."""
import warnings

import numpy as np
import pytest

from tests.kmeans_ref import direct_distances, kmeans_ref


def blobs(seed, n, d, K, spread=1.5, noise=1.0):
    """n observations around K blob centres drawn from N(0, spread^2), noise of the given standard deviation."""
    rng = np.random.default_rng(seed)
    mu = rng.normal(scale=spread, size=(K, d))
    return mu[rng.integers(0, K, n)] + rng.normal(scale=noise, size=(n, d))


@pytest.mark.parametrize("n,d,K", [(300, 2, 3), (500, 10, 7), (450, 40, 6)])
def test_restatement_equals_scipy_lloyd(n, d, K):
    from scipy.cluster.vq import kmeans2
    x = blobs(n + d, n, d, K, spread=10.0, noise=0.5)  # separated blobs
    init = x[np.random.default_rng(K).choice(n, K, replace=False)]
    out = kmeans_ref(x, init, iter_max=100)
    assert out.converged and out.iter >= 2
    # (the converged assignment of the restatement updates nothing: scipy's `iter` counts assignment + update)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        cen, lab = kmeans2(x, init, iter=out.iter, minit="matrix")
    assert np.array_equal(lab + 1, out.cluster)
    np.testing.assert_allclose(cen, out.centers, rtol=1e-12, atol=0)
    assert np.array_equal(out.size, np.bincount(lab, minlength=K))
    assert out.tot_withinss == pytest.approx(((x - cen[lab]) ** 2).sum(), rel=1e-12)


def test_restatement_errors():
    x = blobs(1, 50, 3, 2)
    far = np.vstack([x[:2], np.full((1, 3), 1e6)])
    with pytest.raises(ValueError, match="empty cluster: try a better set of initial centers"):
        kmeans_ref(x, far)
    with pytest.raises(ValueError, match="initial centers are not distinct"):
        kmeans_ref(x, x[[0, 3, 0]])
    with pytest.raises(ValueError, match="more cluster centers than observations"):
        kmeans_ref(x[:2], x[:3])


def test_restatement_tie_goes_to_the_lower_index_and_counts_iterations():
    x = np.array([[0.0], [1.0], [2.0], [10.0]])
    out = kmeans_ref(x, np.array([[2.0], [0.0], [11.0]]), iter_max=1)
    assert out.cluster.tolist() == [2, 1, 1, 3]        # 1.0 is as far from 2.0 (index 0) as from 0.0 (index 1)
    assert out.margin == 0.0 and out.iter == 1 and not out.converged
    np.testing.assert_array_equal(out.centers, [[1.5], [0.0], [10.0]])
    two = kmeans_ref(x, np.array([[0.0], [9.0]]), iter_max=10)
    assert two.converged and two.iter == 2 and two.cluster.tolist() == [1, 1, 1, 2]
    assert two.withinss.tolist() == [2.0, 0.0] and two.size.tolist() == [3, 1]
    assert direct_distances(x, np.array([[1.0]])).ravel().tolist() == [1.0, 0.0, 1.0, 81.0]


def test_kmeans_param():
    from batchelor_amd import KmeansParam
    p = KmeansParam(centers=lambda n: int(np.sqrt(n)), nstart=3)
    assert p.n_centers(400) == 20 and (p.iter_max, p.nstart, p.seed) == (10, 3, 0)
    assert KmeansParam(7).n_centers(10) == 7
    with pytest.raises(ValueError, match="must be an integer or a function that returns one"):
        KmeansParam(lambda n: n / 2).n_centers(10)


def test_start_indices_are_one_choice_per_start():
    from batchelor_amd.kmeans import start_indices
    rng = np.random.default_rng(5)
    want = [rng.choice(100, 7, replace=False) for _ in range(3)]
    got = start_indices(100, 7, nstart=3, seed=5)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_kmeans_argument_errors_need_no_device():
    import batchelor_amd as bx
    x = blobs(2, 40, 3, 2)
    for args, kw, msg in (((x[0], 2), {}, "'x' must be a matrix"),
                          ((x, 0), {}, "number of cluster centres must be positive"),
                          ((x, 41), {}, "more cluster centers than observations"),
                          ((np.zeros((2000, 1)), 1025), {}, "at most 1024 centers"),
                          ((x, x[:3, :2]), {}, "same number of columns"),
                          ((x, x[:3]), {"nstart": 2}, "'nstart' must be 1 when 'centers' is a matrix"),
                          ((x, 3), {"nstart": 0}, "'nstart' must be a positive integer"),
                          ((x, 3), {"iter_max": 0}, "'iter_max' must be positive")):
        with pytest.raises(ValueError, match=msg):
            bx.kmeans(*args, **kw)


def test_cluster_mnn_argument_errors_need_no_device():
    import batchelor_amd as bx
    rng = np.random.default_rng(3)
    b1, b2 = rng.normal(size=(30, 20)), rng.normal(size=(30, 25))
    with pytest.raises(ValueError, match="'cluster_d' must be a positive integer or None"):
        bx.clusterMNN(b1, b2, clusters=bx.KmeansParam(3), cluster_d=0)
    with pytest.raises(ValueError, match="batch 1 of 20 cells cannot be split into 21 clusters"):
        bx.clusterMNN(b1, b2, clusters=bx.KmeansParam(21))
    with pytest.raises(ValueError, match="'nstart' of a KmeansParam must be a positive integer"):
        bx.clusterMNN(b1, b2, clusters=bx.KmeansParam(3, nstart=0))
    with pytest.raises(ValueError, match="batch 2 of 25 cells cannot be split into 0 clusters"):
        bx.clusterMNN(np.hstack([b1, b2]), batch=np.repeat([1, 2], [20, 25]),
                      clusters=bx.KmeansParam(lambda n: n - 25 if n > 20 else 2))
    wide = rng.normal(size=(5, 200))
    with pytest.raises(ValueError, match=r"sum\(number of clusters\) - 1 = 259 dimensions"):
        bx.clusterMNN(wide, wide, clusters=bx.KmeansParam(130))
    with pytest.raises(ValueError, match="at least two batches must be specified"):
        bx.clusterMNN([b1], batch=np.zeros(20), clusters=bx.KmeansParam(3))
    for bad in (1, np.zeros(20, dtype=int)):
        with pytest.raises(ValueError, match="'clusters' must be either a list or a BlusterParam object"):
            bx.clusterMNN(b1, b2, clusters=bad)


def test_device_pca_predicate():
    from batchelor_amd.multi_batch_pca import device_pca_takes
    assert device_pca_takes(64, 65, 50) and device_pca_takes(200, 300, 10)
    assert not device_pca_takes(63, 300, 10) and not device_pca_takes(200, 64, 10)
    assert device_pca_takes(128, 129, 57) and not device_pca_takes(127, 300, 57)
    assert device_pca_takes(300, 300, 120) and not device_pca_takes(300, 300, 121)


def test_new_symbols_are_exported():
    import ctypes
    import batchelor_amd as bx
    from batchelor_amd import _lib
    for name in ("kmeans", "KmeansParam", "KmeansResult"):
        assert hasattr(bx, name)
    lib = _lib.lib()
    for name in ("create", "destroy", "begin", "add_block", "run", "stage_ms"):
        assert hasattr(lib, "bmx_kmeans_" + name)
    # no device is touched: a null handle is refused as by the other resident handles
    out = (ctypes.c_double * 5)()
    assert lib.bmx_kmeans_begin(None, ctypes.c_int64(1)) == -6 and lib.bmx_last_error().decode() == "null handle"
    assert lib.bmx_kmeans_add_block(None, None, ctypes.c_int64(1)) == -6
    assert lib.bmx_last_error().decode() == "null handle"
    assert lib.bmx_kmeans_run(None, None, 1, 1, None, None, None, None, None, None, None) == -6
    assert lib.bmx_last_error().decode() == "null handle"
    assert lib.bmx_kmeans_stage_ms(None, out) == -6 and lib.bmx_last_error().decode() == "null argument"
    assert lib.bmx_kmeans_create(0, 0, None) == -6 and lib.bmx_last_error().decode() == "null output pointer"
    lib.bmx_kmeans_destroy(None)
