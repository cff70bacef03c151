"""clusterMNN() without a GPU: the numpy restatement (tests/cluster_mnn_ref.py) against the reference's own properties
(tests/testthat/test-cluster-mnn.R), the new ABI symbols, and the argument errors, which are raised before any device work."""
import ctypes
import os

import numpy as np
import pytest

from tests import cluster_mnn_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mock_batches(seed=10000001, n=(500, 500), genes=1000, nclust=10):
    """test-cluster-mnn.R:5-16: three populations, a per-gene batch effect, crude clusters (population x random split)."""
    rng = np.random.default_rng(seed)
    means = rng.normal(size=(genes, 3))
    nsub = np.array([nclust // 3 + (i < nclust % 3) for i in range(3)])
    first = np.r_[0, np.cumsum(nsub)[:-1]]
    batches, clusters = [], []
    for b, nb in enumerate(n):
        lab = rng.integers(0, 3, nb)
        x = means[:, lab] + rng.normal(size=(genes, nb))
        if b:
            x = x + rng.normal(size=(genes, 1))
        batches.append(x)
        clusters.append(first[lab] + np.floor(rng.random(nb) * nsub[lab]).astype(np.int64))
    return batches, clusters


def test_full_rank_pca_preserves_distances():
    # test-cluster-mnn.R:35-45
    rng = np.random.default_rng(1)
    stuff = [rng.normal(size=(20, 50)), rng.normal(size=(20, 25)), rng.normal(size=(20, 100))]
    _, _, pcs, _, _ = ref.full_rank_pca(stuff)
    a = np.concatenate(pcs)
    b = np.concatenate(stuff, axis=1).T
    da = np.sqrt(((a[:, None] - a[None]) ** 2).sum(2))
    db = np.sqrt(((b[:, None] - b[None]) ** 2).sum(2))
    np.testing.assert_allclose(da, db, rtol=1e-10, atol=1e-10)


def test_smoothing_equals_naive_form():
    # test-cluster-mnn.R:47-65
    rng = np.random.default_rng(2)
    pcs = rng.normal(size=(50, 20))
    centers = rng.normal(size=(10, 20))
    delta = rng.normal(size=(10, 20)) - centers
    out = ref.smooth_gaussian_from_centroids(pcs, centers, 0.5, delta)
    d2 = ((pcs[:, None] - centers[None]) ** 2).sum(2)
    w = np.exp(-d2 / 0.5 ** 2)
    w = w / w.sum(1, keepdims=True)
    np.testing.assert_allclose(out, pcs + w @ delta, rtol=1e-10, atol=1e-12)


def test_propagation_aligns_cluster_means():
    # test-cluster-mnn.R:67-94
    rng = np.random.default_rng(10000002)
    cluster = np.repeat([1, 2, 3], 100)
    y = np.tile(cluster.astype(float), (50, 1))
    y1 = np.vstack([y + rng.uniform(-0.01, 0.01, y.shape), np.zeros((1, 300))])
    y2 = np.vstack([y + rng.uniform(-0.01, 0.01, y.shape), np.full((1, 300), 1000.0)])
    out = ref.cluster_mnn(y1, y2, cos_norm=False, clusters=[cluster, cluster])
    for i in (1, 2, 3):
        left = out.corrected[(out.batch == 1) & (out.cluster == i)].mean(0)
        right = out.corrected[(out.batch == 2) & (out.cluster == i)].mean(0)
        np.testing.assert_allclose(left, right, rtol=1e-7, atol=1e-7 * np.abs(out.corrected).max())


def test_restriction_equals_leaving_cells_out():
    # test-cluster-mnn.R:135-158
    (b1, b2), (c1, c2) = mock_batches(n=(300, 320), genes=200)
    full = ref.cluster_mnn(b1, b2, clusters=[c1, c2])
    e1 = np.r_[np.arange(10), np.arange(b1.shape[1])]
    e2 = np.r_[np.arange(10), np.arange(b2.shape[1])]
    out = ref.cluster_mnn(b1[:, e1], b2[:, e2], clusters=[c1[e1], c2[e2]],
                          restrict=[np.arange(11, e1.size + 1), np.arange(11, e2.size + 1)])
    keep = np.r_[10 + np.arange(b1.shape[1]), 10 + b1.shape[1] + 10 + np.arange(b2.shape[1])]
    a, b = out.corrected[keep] @ out.rotation.T, full.corrected @ full.rotation.T
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-10 * np.abs(b).max())
    dup = np.r_[np.arange(10), 10 + b1.shape[1] + np.arange(10)]
    np.testing.assert_allclose(out.corrected[dup], out.corrected[dup + 10], rtol=0, atol=1e-12)


def test_single_object_form_equals_list_form():
    # test-cluster-mnn.R:160-197
    (b1, b2), (c1, c2) = mock_batches(n=(300, 320), genes=200)
    full = ref.cluster_mnn(b1, b2, clusters=[c1, c2])
    x = np.hstack([b1, b2])
    batch = np.repeat(["A", "X"], [b1.shape[1], b2.shape[1]])
    call = np.r_[c1, c2]
    single = ref.cluster_mnn(x, batch=batch, clusters=[call])
    # (identical in R; numpy's BLAS may block a sliced copy differently, so equal to rounding)
    a, b = single.corrected @ single.rotation.T, full.corrected @ full.rotation.T
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-10 * np.abs(b).max())
    assert single.batch.tolist() == batch.tolist()
    perm = np.random.default_rng(3).permutation(x.shape[1])
    single2 = ref.cluster_mnn(x[:, perm], batch=batch[perm], clusters=[call[perm]])
    a, b = single2.corrected @ single2.rotation.T, single.corrected[perm] @ single.rotation.T
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-10 * np.abs(b).max())
    assert np.array_equal(single2.cluster, call[perm])
    with pytest.raises(ValueError, match="must be a list of length 1"):
        ref.cluster_mnn(x, batch=batch, clusters=[c1, c2])


def test_meta_clusters_numbering():
    # rows 1-2-5 and 3-4 are joined, 6 is alone: numbered by lowest row
    pairs = [(np.array([5, 3]), np.array([2, 4])), (np.array([1]), np.array([5]))]
    assert ref.meta_clusters(pairs, 6).tolist() == [1, 1, 2, 2, 1, 3]
    from batchelor_amd.cluster_mnn import meta_clusters
    assert meta_clusters(pairs, 6).tolist() == [1, 1, 2, 2, 1, 3]


def test_package_full_rank_pca_matches_restatement():
    from batchelor_amd.cluster_mnn import full_rank_pca
    rng = np.random.default_rng(4)
    cents = [rng.normal(size=(40, 6)), rng.normal(size=(40, 9)), rng.normal(size=(40, 4))]
    sub = np.arange(5, 36)
    for kw in ({}, {"subset_row": sub}, {"subset_row": sub, "correct_all": True}):
        got = full_rank_pca(cents, **kw)
        rotation, centers, pcs, u, grand = ref.full_rank_pca(cents, **kw)
        # the basis is defined up to sign: compare what does not depend on it
        np.testing.assert_allclose(got["rotation"] @ got["rotation"].T, rotation @ rotation.T, atol=1e-10)
        np.testing.assert_allclose(got["centers"], centers, atol=1e-13)
        for p, q in zip(got["pcs"], pcs):
            np.testing.assert_allclose(p @ got["rotation_used"].T, q @ u.T, atol=1e-10)


def test_abi_exports():
    import __graft_entry__ as g
    g.build()
    lib = ctypes.CDLL(os.path.join(ROOT, "batchelor_amd", "libbatchelor_mi355x.so"))
    header = open(os.path.join(ROOT, "include", "batchelor_mi355x.h")).read()
    for sym in ("bmx_cluster_create", "bmx_cluster_destroy", "bmx_cluster_add_batch", "bmx_cluster_begin_batch",
                "bmx_cluster_add_block", "bmx_cluster_centroids", "bmx_cluster_propagate", "bmx_cluster_stage_ms"):
        assert hasattr(lib, sym), sym
        assert sym + "(" in header, sym


def test_argument_errors_need_no_device():
    import batchelor_amd as bx
    (b1, b2), (c1, c2) = mock_batches(n=(60, 70), genes=30)
    with pytest.raises(ValueError, match="must be either a list or a BlusterParam object"):
        bx.clusterMNN(b1, b2, clusters=1)
    with pytest.raises(ValueError, match="should be of the same length"):
        bx.clusterMNN(b1, b2, clusters=[c1])
    with pytest.raises(ValueError, match="should have the same number of cells"):
        bx.clusterMNN(b1, b2, clusters=[c1, c2[:-1]])
    with pytest.raises(ValueError, match="must be a list of length 1"):
        bx.clusterMNN(np.hstack([b1, b2]), batch=np.repeat([1, 2], [60, 70]), clusters=[c1, c2])
    with pytest.raises(ValueError, match="'batch' must be specified"):
        bx.clusterMNN(b1, clusters=[c1])
    with pytest.raises(ValueError, match="number of rows is not the same"):
        bx.clusterMNN(b1, b2[:-1], clusters=[c1, c2])
    with pytest.raises(ValueError, match="'restrictions' must of length"):
        bx.clusterMNN(b1, b2, clusters=[c1, c2], restrict=[None])
    # a cluster whose cells are all outside the restriction
    r1 = np.flatnonzero(c1 != c1[0]) + 1
    with pytest.raises(ValueError, match="no cells remaining after restriction"):
        bx.clusterMNN(b1, b2, clusters=[c1, c2], restrict=[r1, None])
    # sum(C_b) - 1 > 256 columns
    rng = np.random.default_rng(5)
    big = [rng.normal(size=(30, 200)) for _ in range(2)]
    with pytest.raises(ValueError, match="at most 256"):
        bx.clusterMNN(*big, clusters=[np.arange(200) % 130, np.arange(200) % 130])
