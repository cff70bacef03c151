"""clusterMNN() on the device against its numpy restatement (tests/cluster_mnn_ref.py).

The PCA basis is defined up to the sign of each column (up to a rotation where singular values coincide), so the end-to-end
comparison is of `corrected @ rotation.T`, which does not depend on the basis (the restatement under random sign flips and a
random orthogonal change of basis moved it by 2e-15 relative), at the project's relative 1e-5.  Pair arrays are compared
exactly for two batches; for three and more the claims of tests/test_gpu_degenerate_k.py's docstring apply (k = 1 puts cells
an ulp apart): the same merges, the same number of pairs per merge, the pairs equal as multisets once ulp twins are
identified.  Default merge order only, as that docstring explains.
Every test prints the figure it asserts on; the measured maxima are in MEASUREMENTS.md."""
import ctypes

import numpy as np
import pytest

from tests import cluster_mnn_ref as ref
from tests.test_cpu_cluster_mnn import mock_batches
from tests.test_gpu_degenerate_k import twin_representatives

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bx():
    import batchelor_amd
    return batchelor_amd


@pytest.fixture(scope="module")
def handle():
    from batchelor_amd.cluster_mnn import _ClusterHandle
    return _ClusterHandle


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def unequal_clusters(rng, n, sizes):
    """Labels with the given relative sizes, shuffled over n cells, every label present."""
    p = np.asarray(sizes, dtype=float)
    lab = rng.choice(len(sizes), size=n, p=p / p.sum())
    lab[:len(sizes)] = np.arange(len(sizes))
    return rng.permutation(lab)


# ---------------------------------------------------------------------------------------------------------------------
# centroid kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [10, 500, 2000])
@pytest.mark.parametrize("cos_norm", [False, True])
@pytest.mark.parametrize("restricted", [False, True])
def test_centroids_against_numpy(handle, G, cos_norm, restricted):
    rng = np.random.default_rng(G + 2 * cos_norm + restricted)
    n = 3000
    x = rng.normal(size=(G, n)) + 2.0
    lab = unequal_clusters(rng, n, [1, 1, 40, 3, 8, 0.2, 5])  # the third cluster spans several chunks of 256 cells
    restrict = None
    if restricted:
        restrict = rng.choice(n, size=2 * n // 3, replace=False) + 1
        restrict = np.unique(np.r_[restrict, [np.flatnonzero(lab == c)[0] + 1 for c in range(7)]]).astype(np.int32)
    kept = lab if restrict is None else lab[restrict - 1]
    assert np.bincount(kept).max() > 512
    outs = []
    for _ in range(2):
        h = handle(G, None, 0)
        h.add_batch(x, lab.astype(np.int32), 7, restrict, cos_norm)
        outs.append(h.centroids(0))
        h.close()
    assert np.array_equal(outs[0], outs[1])  # bitwise the same from run to run
    y = x / np.maximum(ref.cosine_l2(x), 1e-8) if cos_norm else x
    want, levels = ref.compute_centroids(y, lab, restrict)
    err = rel(outs[0], want)
    print(f"centroids G={G} cos_norm={cos_norm} restricted={restricted}: max rel err {err:.3e}")
    assert err < 1e-5


@pytest.mark.parametrize("G,subset", [(1, None), (2, None), (255, 1), (256, 63), (257, 64), (258, 65)])
@pytest.mark.parametrize("restricted", [False, True])
def test_centroids_at_the_edges_of_the_chunk_walk(handle, G, subset, restricted):
    """Clusters of 1, 3, 4, 5, 255, 256, 257 and 513 cells (chunks of 256), restricted lists of 4k + 1, 4k + 2 and 4k + 3
    cells, gene counts on either side of the 256-gene tile; the cosine norms over all genes or over a list of 1, 63, 64
    and 65 (a wave takes 64 at a time)."""
    sizes = np.array([1, 3, 4, 5, 255, 256, 257, 513])
    rng = np.random.default_rng(G + restricted)
    lab = rng.permutation(np.repeat(np.arange(sizes.size), sizes))
    x = rng.normal(size=(G, lab.size)) + 2.0
    sub = None if subset is None else (np.sort(rng.choice(G, size=subset, replace=False)) + 1).astype(np.int32)
    restrict = None
    if restricted:
        keep = [1, 2, 3, 5, 6, 7, 255, 257]
        restrict = np.sort(np.concatenate([rng.choice(np.flatnonzero(lab == c), size=m, replace=False)
                                           for c, m in enumerate(keep)]) + 1).astype(np.int32)
    h = handle(G, sub, 0)
    h.add_batch(x, lab.astype(np.int32), sizes.size, restrict, True)
    got = h.centroids(0)
    h.close()
    want, levels = ref.compute_centroids(x / np.maximum(ref.cosine_l2(x, sub), 1e-8), lab, restrict)
    err = rel(got, want)
    print(f"centroids at the edges G={G} norm genes={subset} restricted={restricted}: max rel err {err:.3e}")
    assert err < 1e-5


def test_centroids_blocked_upload_equals_whole(handle):
    rng = np.random.default_rng(11)
    G, n = 300, 5000
    x = rng.normal(size=(G, n))
    lab = unequal_clusters(rng, n, [1, 2, 3, 4]).astype(np.int32)
    outs = []
    for block_bytes in (1 << 28, 8 * G * 777):
        h = handle(G, None, 0)
        h.add_batch(x, lab, 4, None, True, block_bytes=block_bytes)
        outs.append(h.centroids(0))
        h.close()
    assert np.array_equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------------------------------
# propagation kernels on their own
# ---------------------------------------------------------------------------------------------------------------------
def run_propagation(handle, x, lab, C, rotation, centers, cp, corr, restrict=None, cos_norm=False, subset=None):
    h = handle(x.shape[0], subset, 0)
    h.add_batch(x, lab.astype(np.int32), C, restrict, cos_norm)
    cur, _ = h.propagate(0, rotation, centers, cp, cp)  # zero deltas: the device's own projection, bit for bit
    out, sigma = h.propagate(0, rotation, centers, cp, corr)
    h.close()
    return out, sigma, cur


@pytest.mark.parametrize("n,G,C,d,cos_norm,restricted,subset", [
    (50, 20, 10, 20, False, False, False),     # test-cluster-mnn.R:47-65's sizes
    (1001, 300, 13, 12, True, False, False),   # odd count: the median is one value
    (1000, 300, 13, 12, True, True, False),    # restricted, even count
    (4000, 500, 37, 36, True, False, True),    # subset.row
    (3000, 400, 257, 256, False, False, False),  # the widest the engine takes
])
def test_propagation_against_restatement(handle, n, G, C, d, cos_norm, restricted, subset):
    rng = np.random.default_rng(n + C)
    sub = (np.sort(rng.choice(G, size=max(d, 2 * G // 3), replace=False)) + 1).astype(np.int32) if subset else None
    rows = G if sub is None else sub.size
    x = rng.normal(size=(G, n)) + 1.0
    rotation = np.linalg.qr(rng.normal(size=(rows, d)))[0]
    centers = rng.normal(size=rows) * 0.1
    lab = np.arange(n) % C
    restrict = None
    if restricted:
        restrict = np.union1d(rng.choice(n, size=n // 2, replace=False) + 1, np.arange(1, C + 1))
        if restrict.size % 2:  # an even count: the median is the mean of the two middle values
            restrict = np.union1d(restrict, np.setdiff1d(np.arange(1, n + 1), restrict)[:1])
        restrict = restrict.astype(np.int32)
    l2 = ref.cosine_l2(x, sub) if cos_norm else None
    y = (x if sub is None else x[sub - 1])
    y = y / np.maximum(l2, 1e-8) if cos_norm else y
    proj = y.T @ rotation - centers @ rotation
    cp = np.stack([proj[lab == c].mean(0) for c in range(C)])  # centroids among the cells, as in a real run
    corr = cp + rng.normal(size=cp.shape) * 0.3
    out, sigma, cur = run_propagation(handle, x, lab, C, rotation, centers, cp, corr, restrict, cos_norm, sub)
    want, want_sigma, want_cur = ref.propagate_to_cells(x, rotation, centers, cp, corr, restrict, sub, l2)
    # sigma, from the device's own projection: bit for bit numpy.median of the restatement's distances
    dist = ref.nearest_distance(cur, cp)
    own = float(np.median(dist if restrict is None else dist[restrict - 1]))
    print(f"propagation n={n} C={C} d={d}: sigma {sigma!r} own {own!r} restatement {want_sigma!r} "
          f"rel {abs(sigma - want_sigma) / want_sigma:.3e}; cur rel {rel(cur, want_cur):.3e}; rows rel {rel(out, want):.3e}")
    assert sigma == own
    assert abs(sigma - want_sigma) <= 1e-12 * want_sigma
    assert rel(out, want) < 1e-5


def test_smoothing_fixed_sigma_shape(handle):
    # test-cluster-mnn.R:47-65: 50 cells, 10 centroids, 20 columns, sigma 0.5.  The bandwidth is the median distance to the
    # nearest centroid, so the cells are laid out to make it 0.5 exactly: the centroids far apart on a grid of 1/1024, every
    # cell at 0.5 from its own centroid along one axis
    rng = np.random.default_rng(47)
    n, C, d = 50, 10, 20
    cp = np.round(rng.normal(size=(C, d)) * 4.0 * 1024) / 1024
    lab = np.arange(n) % C
    pcs = cp[lab].copy()
    pcs[np.arange(n), np.arange(n) % d] += 0.5
    delta = rng.normal(size=(C, d)) - cp
    rotation, centers = np.eye(d), np.zeros(d)
    out, sigma, cur = run_propagation(handle, np.asfortranarray(pcs.T), lab, C, rotation, centers, cp, cp + delta)
    assert np.array_equal(cur, pcs)
    assert sigma == 0.5
    d2 = ((pcs[:, None] - cp[None]) ** 2).sum(2)
    w = np.exp(-d2 / 0.5 ** 2)
    naive = pcs + (w / w.sum(1, keepdims=True)) @ delta
    err = rel(out, naive)
    print(f"smoothing, sigma 0.5, against the naive form: max rel err {err:.3e}")
    assert err < 1e-5
    assert rel(out, ref.smooth_gaussian_from_centroids(pcs, cp, 0.5, delta)) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
def compare(out, want, exact_pairs):
    a, b = out.corrected @ out.rotation.T, want.corrected @ want.rotation.T
    err = rel(a, b)
    assert err < 1e-5, err
    serr = float(np.abs(out.sigma / want.sigma - 1).max())
    assert serr < 1e-9, serr
    assert out.batch.tolist() == want.batch.tolist()
    assert out.cluster.tolist() == want.cluster.tolist()
    assert out.merge_info.left == want.merge_info.left and out.merge_info.right == want.merge_info.right
    rep = twin_representatives(want.merged.corrected)
    for (ol, orr), (wl, wr) in zip(out.merge_info.pairs, want.merge_info.pairs):
        assert ol.size == wl.size
        if exact_pairs:
            assert np.array_equal(ol, wl) and np.array_equal(orr, wr)
        mine = np.stack([rep[ol - 1], rep[orr - 1]], axis=1)
        theirs = np.stack([rep[wl - 1], rep[wr - 1]], axis=1)
        assert np.array_equal(mine[np.lexsort(mine.T[::-1])], theirs[np.lexsort(theirs.T[::-1])])
    for col in ("cluster", "batch", "meta"):
        assert out.cluster_info[col].tolist() == want.cluster_info[col].tolist(), col
    np.testing.assert_allclose(out.centers, want.centers, rtol=1e-9, atol=1e-12)
    return err


def test_reference_shape_two_batches(bx):
    # test-cluster-mnn.R:5-16: 2 x 500 cells x 1 000 genes, 10 clusters each
    (b1, b2), (c1, c2) = mock_batches()
    out = bx.clusterMNN(b1, b2, clusters=[c1, c2])
    want = ref.cluster_mnn(b1, b2, clusters=[c1, c2])
    err = compare(out, want, exact_pairs=True)
    print(f"2 x 500 x 1000: corrected @ rotation.T max rel err {err:.3e}; pairs {[p[0].size for p in out.merge_info.pairs]}")
    assert set(out.stats["stage_ms"]) == {"upload", "centroids", "projection", "nearest_median", "smoothing"}
    assert out.corrected.shape == (1000, 19) and out.rotation.shape == (1000, 19)


@pytest.mark.parametrize("sizes", [(400, 650, 300), (500, 250, 700, 350)])
def test_three_and_four_batches(bx, sizes):
    batches, clusters = mock_batches(seed=len(sizes), n=sizes, genes=600, nclust=9)
    out = bx.clusterMNN(*batches, clusters=clusters)
    want = ref.cluster_mnn(*batches, clusters=clusters)
    err = compare(out, want, exact_pairs=False)
    print(f"{len(sizes)} batches {sizes}: corrected @ rotation.T max rel err {err:.3e}")


@pytest.mark.parametrize("correct_all", [False, True])
def test_subset_row(bx, correct_all):
    (b1, b2), (c1, c2) = mock_batches(seed=7, n=(450, 520), genes=400)
    sub = np.arange(11, 401)
    out = bx.clusterMNN(b1, b2, clusters=[c1, c2], subset_row=sub, correct_all=correct_all)
    want = ref.cluster_mnn(b1, b2, clusters=[c1, c2], subset_row=sub, correct_all=correct_all)
    err = compare(out, want, exact_pairs=True)
    print(f"subset_row correct_all={correct_all}: max rel err {err:.3e}")
    assert out.rotation.shape[0] == (400 if correct_all else 390)
    # test-cluster-mnn.R:96-110: the subset's genes are corrected as if the others were not there
    plain = bx.clusterMNN(b1[10:], b2[10:], clusters=[c1, c2])
    a = out.corrected @ (out.rotation[10:] if correct_all else out.rotation).T
    assert rel(a, plain.corrected @ plain.rotation.T) < 1e-5


def test_restrict(bx):
    (b1, b2), (c1, c2) = mock_batches(seed=8, n=(450, 520), genes=300)
    e1 = np.r_[np.arange(10), np.arange(b1.shape[1])]
    e2 = np.r_[np.arange(10), np.arange(b2.shape[1])]
    args = (b1[:, e1], b2[:, e2])
    kw = dict(clusters=[c1[e1], c2[e2]], restrict=[np.arange(11, e1.size + 1), np.arange(11, e2.size + 1)])
    out = bx.clusterMNN(*args, **kw)
    err = compare(out, ref.cluster_mnn(*args, **kw), exact_pairs=True)
    print(f"restrict: max rel err {err:.3e}")
    # test-cluster-mnn.R:135-158
    plain = bx.clusterMNN(b1, b2, clusters=[c1, c2])
    keep = np.r_[10 + np.arange(b1.shape[1]), 10 + b1.shape[1] + 10 + np.arange(b2.shape[1])]
    assert rel(out.corrected[keep] @ out.rotation.T, plain.corrected @ plain.rotation.T) < 1e-5
    dup = np.r_[np.arange(10), 10 + b1.shape[1] + np.arange(10)]
    assert np.array_equal(out.corrected[dup], out.corrected[dup + 10])


def test_single_object_shuffled_batch(bx):
    (b1, b2, b3), (c1, c2, c3) = mock_batches(seed=9, n=(300, 420, 260), genes=300, nclust=6)
    perm = np.random.default_rng(9).permutation(980)
    x = np.hstack([b1, b2, b3])[:, perm]
    batch = np.repeat(["A", "M", "X"], [300, 420, 260])[perm]
    call = np.r_[c1, c2, c3][perm]
    out = bx.clusterMNN(x, batch=batch, clusters=[call])
    want = ref.cluster_mnn(x, batch=batch, clusters=[call])
    err = compare(out, want, exact_pairs=False)
    print(f"single object, shuffled: max rel err {err:.3e}")
    assert out.batch.tolist() == batch.tolist()
    listed = bx.clusterMNN(b1, b2, b3, clusters=[c1, c2, c3])
    assert rel(out.corrected @ out.rotation.T, (listed.corrected @ listed.rotation.T)[perm]) < 1e-5


def test_cos_norm_off_and_string_labels(bx):
    (b1, b2), (c1, c2) = mock_batches(seed=10, n=(350, 300), genes=250)
    s1 = np.array([f"c{v}" for v in c1])
    s2 = np.array([f"k{v}" for v in c2])
    out = bx.clusterMNN(b1, b2, clusters=[s1, s2], cos_norm=False)
    want = ref.cluster_mnn(b1, b2, clusters=[s1, s2], cos_norm=False)
    err = compare(out, want, exact_pairs=True)
    print(f"cos_norm=False, string labels: max rel err {err:.3e}")


def test_larger_case_blocked_upload(bx):
    # 4 x 50 000 cells x 2 000 genes, 30 clusters each: every batch (800 MB) goes over in column blocks
    rng = np.random.default_rng(50000)
    G, n, K = 2000, 50000, 30
    means = rng.normal(size=(G, K))
    batches, clusters = [], []
    for b in range(4):
        lab = unequal_clusters(rng, n, 1.0 + np.arange(K))
        x = np.asfortranarray(means[:, lab])
        x += rng.normal(size=(n, G)).T
        x += (b > 0) * rng.normal(size=(G, 1))
        batches.append(x)
        clusters.append(lab)
    out = bx.clusterMNN(*batches, clusters=clusters)
    want = ref.cluster_mnn(*batches, clusters=clusters)
    err = compare(out, want, exact_pairs=False)
    print(f"4 x 50000 x 2000, 30 clusters: max rel err {err:.3e}; stage ms {out.stats['stage_ms']}")


def test_refusals(bx):
    (b1, b2), (c1, c2) = mock_batches(seed=12, n=(300, 300), genes=50)
    with pytest.raises(ValueError, match="at most 256"):
        bx.clusterMNN(b1, b2, clusters=[np.arange(300) % 130, np.arange(300) % 130])
    with pytest.raises(ValueError, match="must be either a list or a BlusterParam object"):
        bx.clusterMNN(b1, b2, clusters=c1)
    with pytest.raises(ValueError, match="should be of the same length"):
        bx.clusterMNN(b1, b2, clusters=[c1, c2, c2])
    with pytest.raises(ValueError, match="should have the same number of cells"):
        bx.clusterMNN(b1, b2, clusters=[c1[:-1], c2])
    with pytest.raises(ValueError, match="no cells remaining after restriction"):
        bx.clusterMNN(b1, b2, clusters=[c1, c2], restrict=[np.flatnonzero(c1 != c1[0]) + 1, None])


def test_abi_argument_checks():
    from batchelor_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.bmx_cluster_create(0, 0, None, 0, ctypes.byref(h)) == -6
    sub = np.array([1, 99], dtype=np.int32)
    assert L.bmx_cluster_create(0, 10, _lib.i32p(sub), 2, ctypes.byref(h)) == -4
    _lib.check(L.bmx_cluster_create(0, 10, None, 0, ctypes.byref(h)))
    L.bmx_cluster_destroy.argtypes = [ctypes.c_void_p]
    L.bmx_cluster_destroy.restype = None
    try:
        x = np.zeros((10, 6), order="F")
        ids = np.array([0, 1, 2, 0, 1, 5], dtype=np.int32)
        rc = L.bmx_cluster_add_batch(h, _lib.f64p(x), ctypes.c_int64(6), _lib.i32p(ids), 3, None, ctypes.c_int64(-1), 0)
        assert rc == -6 and b"out of range" in L.bmx_last_error()
        ids[5] = 2
        r = np.array([1, 2, 4], dtype=np.int32)  # cluster 2 has no restricted cell
        rc = L.bmx_cluster_add_batch(h, _lib.f64p(x), ctypes.c_int64(6), _lib.i32p(ids), 3, _lib.i32p(r), ctypes.c_int64(3), 0)
        assert rc == -6 and b"no cells remaining" in L.bmx_last_error()
        out = np.zeros((10, 3), order="F")
        assert L.bmx_cluster_centroids(h, 0, _lib.f64p(out)) == -6  # no batch yet
        _lib.check(L.bmx_cluster_add_batch(h, _lib.f64p(x), ctypes.c_int64(6), _lib.i32p(ids), 3, None, ctypes.c_int64(-1), 0))
        rot = np.zeros((10, 300), order="F")
        rc = L.bmx_cluster_propagate(h, 0, _lib.f64p(rot), 300, _lib.f64p(out), _lib.f64p(out), _lib.f64p(out), _lib.f64p(rot),
                                     None)
        assert rc == -6 and b"256" in L.bmx_last_error()
    finally:
        L.bmx_cluster_destroy(h)
