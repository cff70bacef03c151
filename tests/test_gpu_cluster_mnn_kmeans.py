"""clusterMNN(clusters=KmeansParam(...), cluster_d=...) on the device (R/clusterMNN.R:199-221): every batch clustered by
kmeans() on its own PCs, the labels then going the way labels given by the caller go.

The labels are compared with the CPU pipeline: numpy's SVD of the centred subset rows, then tests/kmeans_ref.py from the
same seeded rows.  The device's PCs differ from numpy's by the sign of a column and by about the PCA's tolerance (a Ritz
residual of 1e-9); k-means does not see the former, and the restatement's smallest tie margin is first asserted to lie
three orders above the latter (> 1e-6), so both must give the same labels.

Lloyd from randomly drawn rows often leaves a cluster empty on well-separated populations, which is an error by definition
(tests/kmeans_ref.py): the seeds below are ones at which the CPU pipeline meets none in any batch and start."""
import warnings

import numpy as np
import pytest

from tests.kmeans_ref import kmeans_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bx():
    import batchelor_amd
    return batchelor_amd


def blob_batches(seed, n=(400, 520), genes=200, npop=6):
    """Batches in the style of test-cluster-mnn.R:5-16 with npop well-separated populations and a per-gene batch effect."""
    rng = np.random.default_rng(seed)
    means = rng.normal(scale=2.0, size=(genes, npop))
    out = []
    for b, nb in enumerate(n):
        lab = rng.integers(0, npop, nb)
        x = means[:, lab] + rng.normal(size=(genes, nb))
        if b:
            x = x + rng.normal(size=(genes, 1))
        out.append(x)
    return out


def quiet(fn, *args, **kw):
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message="did not converge")
        return fn(*args, **kw)


def cpu_labels(m, param, cluster_d, subset_row=None):
    """.format_clusters for one batch on the CPU: labels, the restatement's tie margin."""
    from batchelor_amd.kmeans import start_indices
    cur = m if subset_row is None else m[np.asarray(subset_row) - 1]
    obs = np.ascontiguousarray(cur.T)
    if cluster_d is not None:
        u, s, _ = np.linalg.svd(obs - obs.mean(axis=0), full_matrices=False)
        obs = u[:, :cluster_d] * s[:cluster_d]
    K = param.n_centers(obs.shape[0])
    idx = start_indices(obs.shape[0], K, 1, param.seed)[0]
    ref = kmeans_ref(obs, obs[idx], iter_max=param.iter_max)
    return ref.cluster, ref.margin


def split(v, sizes):
    return np.split(v, np.cumsum(sizes)[:-1])


def test_kmeans_param_equals_its_own_labels_given_as_a_list(bx):
    b1, b2 = blob_batches(4, n=(400, 520), genes=200, npop=8)
    auto = quiet(bx.clusterMNN, b1, b2, clusters=bx.KmeansParam(centers=8, nstart=3, seed=4))
    l1, l2 = split(auto.cluster, [400, 520])
    assert all(np.unique(v).size == 8 for v in (l1, l2))
    given = bx.clusterMNN(b1, b2, clusters=[l1, l2])
    assert np.array_equal(auto.corrected, given.corrected)
    assert np.array_equal(auto.rotation, given.rotation) and np.array_equal(auto.centers, given.centers)
    for (al, ar), (gl, gr) in zip(auto.merge_info.pairs, given.merge_info.pairs):
        assert np.array_equal(al, gl) and np.array_equal(ar, gr)
    assert set(auto.cluster_info) == set(given.cluster_info)
    for key in auto.cluster_info:
        assert np.array_equal(auto.cluster_info[key], given.cluster_info[key])
    assert np.array_equal(auto.sigma, given.sigma) and np.array_equal(auto.batch, given.batch)
    info = auto.stats["clustering"]
    assert given.stats["clustering"] is None and len(info) == 2
    assert [i["pca"] for i in info] == ["device-pca", "device-pca"] and all(i["d"] == 50 and i["centers"] == 8 for i in info)
    assert set(auto.stats["stage_ms"]) == {"upload", "centroids", "projection", "nearest_median", "smoothing"}


@pytest.mark.parametrize("case", ["d10", "none", "subset", "host_svd", "clamped"])
def test_labels_equal_the_cpu_pipeline(bx, case):
    sizes, genes, kw, paths = (400, 520), 200, {"cluster_d": 10}, ["device-pca", "device-pca"]
    if case == "none":
        kw, paths = {"cluster_d": None}, ["none", "none"]
    elif case == "subset":
        kw["subset_row"] = np.random.default_rng(4).choice(genes, 120, replace=False) + 1
    elif case == "host_svd":
        sizes, paths = (60, 520), ["host-svd", "device-pca"]       # 60 cells: not more than the PCA's block of 64
    elif case == "clamped":
        sizes, genes, kw, paths = (300, 320), 40, {"cluster_d": 50}, ["host-svd", "host-svd"]
    batches = blob_batches(7, n=sizes, genes=genes, npop=6)
    param = bx.KmeansParam(centers=lambda n: 6 if n > 100 else 4, iter_max=30, seed=6)
    d_used = None if kw["cluster_d"] is None else min(kw["cluster_d"], genes)
    want = []
    for m in batches:
        lab, margin = cpu_labels(m, param, d_used, kw.get("subset_row"))
        print(f"{case}: batch of {m.shape[1]} cells, restatement margin {margin:.3g}")
        assert margin > 1e-6
        want.append(lab)
    if case == "clamped":
        with pytest.warns(UserWarning, match="'cluster_d' = 50 exceeds"):
            out = bx.clusterMNN(*batches, clusters=param, **kw)
    else:
        out = quiet(bx.clusterMNN, *batches, clusters=param, **kw)
    for got, lab in zip(split(out.cluster, sizes), want):
        assert np.array_equal(got, lab)
    assert [i["pca"] for i in out.stats["clustering"]] == paths
    assert np.isfinite(out.corrected).all() and out.corrected.shape[0] == sum(sizes)


def test_single_object_form_equals_the_list_form(bx):
    b1, b2 = blob_batches(3, n=(330, 410), genes=200, npop=5)
    x = np.hstack([b1, b2])
    batch = np.repeat(["A", "X"], [330, 410])
    perm = np.random.default_rng(5).permutation(x.shape[1])
    x, batch = x[:, perm], batch[perm]
    param = bx.KmeansParam(centers=7, nstart=2, seed=14)
    single = quiet(bx.clusterMNN, x, batch=batch, clusters=param, cluster_d=20)
    order = np.r_[np.flatnonzero(batch == "A"), np.flatnonzero(batch == "X")]
    listed = quiet(bx.clusterMNN, x[:, batch == "A"], x[:, batch == "X"], clusters=param, cluster_d=20)
    assert np.array_equal(single.corrected[order], listed.corrected)
    assert np.array_equal(single.cluster[order], listed.cluster)
    assert single.batch.tolist() == batch.tolist()
    assert np.array_equal(single.rotation, listed.rotation)
    assert np.array_equal(single.cluster_info["cluster"], listed.cluster_info["cluster"])
    assert np.array_equal(single.cluster_info["meta"], listed.cluster_info["meta"])


def test_other_clusters_are_still_refused(bx):
    b1, b2 = blob_batches(4, n=(100, 120), genes=80, npop=3)
    for bad in (1, np.zeros(100, dtype=int)):
        with pytest.raises(ValueError, match="'clusters' must be either a list or a BlusterParam object"):
            bx.clusterMNN(b1, b2, clusters=bad)
        with pytest.raises(ValueError, match="'clusters' must be either a list or a BlusterParam object"):
            bx.clusterMNN(np.hstack([b1, b2]), batch=np.repeat([1, 2], [100, 120]), clusters=bad)
