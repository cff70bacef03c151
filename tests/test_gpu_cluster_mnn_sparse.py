"""clusterMNN() on scipy.sparse batches kept CSC on the device (bmx_cluster_sparse_*), against the dense handle on the
densified matrices and against the numpy restatement (tests/cluster_mnn_ref.py).

Tolerance: the project's relative 1e-5, rel(a, b) = max|a - b| / max|b|.  Bit equalities are asked for where the arithmetic
gives them: without cos_norm the sparse centroid pass adds the dense pass's terms with the +0.0 ones left out, which changes
no sum; no kernel uses floating-point atomics, so two runs and any cut into upload blocks agree bit for bit.
Every test prints the figure it asserts on."""
import ctypes
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

from tests import cluster_mnn_ref as ref
from tests.kmeans_ref import kmeans_ref
from tests.test_cpu_cluster_mnn import mock_batches
from tests.test_gpu_degenerate_k import twin_representatives

pytestmark = pytest.mark.gpu

SIZES = np.array([1, 3, 4, 5, 255, 256, 257, 513])  # cells per cluster: the edges of the chunk walk (chunks of 256)


@pytest.fixture(scope="module")
def bx():
    import batchelor_amd
    return batchelor_amd


@pytest.fixture(scope="module")
def handles():
    from batchelor_amd.cluster_mnn import _ClusterHandle, _ClusterSparseHandle
    return _ClusterHandle, _ClusterSparseHandle


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def sparse_values(rng, G, n, density=0.3):
    return (rng.normal(size=(G, n)) + 2.0) * (rng.random((G, n)) < density)


def with_stored_zero(x, col):
    """x as canonical CSC with one stored entry of column `col` turned into an explicit zero (none stored: x as it is)."""
    c = sp.csc_matrix(x)
    if c.indptr[col + 1] > c.indptr[col]:
        c.data[c.indptr[col]] = 0.0
    return c


# ---------------------------------------------------------------------------------------------------------------------
# centroid kernel: the sparse handle against the dense handle on the densified matrix
# ---------------------------------------------------------------------------------------------------------------------
def edge_case(G, subset, restricted):
    """The shapes of test_centroids_at_the_edges_of_the_chunk_walk at density 0.3, with a cell without an entry, a cell
    with one, a full column, a stored explicit zero, a cluster whose every cell is empty and -- in the unrestricted
    cases of three genes and more, where the full column is then full but for that gene -- a gene without an entry."""
    rng = np.random.default_rng(G + restricted)
    lab = rng.permutation(np.repeat(np.arange(SIZES.size), SIZES))
    x = sparse_values(rng, G, lab.size)
    big = np.flatnonzero(lab == 7)
    x[:, big[0]] = 0.0                                   # a cell with no entry
    x[:, big[1]] = 0.0
    x[rng.integers(G), big[1]] = 1.5                     # a cell with one entry
    x[:, big[2]] = rng.normal(size=G) + 3.0              # a full column
    x[:, lab == 1] = 0.0                                 # a cluster (3 cells) whose every cell is empty
    if G >= 3 and not restricted:
        x[G // 2] = 0.0                                  # a gene with no entry
    c = with_stored_zero(x, int(big[2]))                 # a stored explicit zero (the full column's first entry)
    sub = None if subset is None else (np.sort(rng.choice(G, size=subset, replace=False)) + 1).astype(np.int32)
    restrict = None
    if restricted:
        keep = [1, 2, 3, 5, 6, 7, 255, 257]
        restrict = np.sort(np.concatenate([rng.choice(np.flatnonzero(lab == cl), size=m, replace=False)
                                           for cl, m in enumerate(keep)]) + 1).astype(np.int32)
    return c, np.asfortranarray(c.toarray()), lab.astype(np.int32), sub, restrict


@pytest.mark.parametrize("G,subset", [(1, None), (2, None), (255, 1), (256, 63), (257, 64), (258, 65),
                                      (("tile", -1), None), (("tile", 0), 64), (("tile", 1), 65)])
@pytest.mark.parametrize("restricted", [False, True])
def test_centroids_at_the_edges_equal_the_dense_handle(handles, G, subset, restricted):
    from batchelor_amd import _lib
    if isinstance(G, tuple):  # one below, at and one above the LDS gene tile of the sparse centroid kernel
        G = _lib.dev_get("cluster_sparse_gene_tile") + G[1]
    dense_handle, sparse_handle = handles
    c, x, lab, sub, restrict = edge_case(G, subset, restricted)
    assert c.nnz > np.count_nonzero(x)  # the explicit zero is stored
    got = {}
    for cos_norm in (False, True):
        for name, cls, m in (("dense", dense_handle, x), ("sparse", sparse_handle, c)):
            h = cls(G, sub, 0)
            h.add_batch(m, lab, SIZES.size, restrict, cos_norm)
            got[name, cos_norm] = h.centroids(0)
            h.close()
    same = np.array_equal(got["sparse", False], got["dense", False])
    y = x / np.maximum(ref.cosine_l2(x, sub), 1e-8)
    want, levels = ref.compute_centroids(y, lab, restrict)
    err = rel(got["sparse", True], want)
    print(f"sparse centroids G={G} norm genes={subset} restricted={restricted}: bit-equal to dense without cos_norm {same}; "
          f"cos_norm max rel err {err:.3e} (dense handle {rel(got['dense', True], want):.3e})")
    assert same
    assert err < 1e-5
    assert not got["sparse", True][:, 1].any()  # the cluster of empty cells


def test_centroids_of_a_cluster_spanning_chunks_against_numpy(handles):
    _, sparse_handle = handles
    rng = np.random.default_rng(31)
    G, n = 500, 3000
    x = sparse_values(rng, G, n)
    lab = rng.choice(7, size=n, p=np.array([1, 1, 40, 3, 8, 0.2, 5]) / 58.2)
    lab[:7] = np.arange(7)
    restrict = np.unique(np.r_[rng.choice(n, size=2000, replace=False), np.arange(7)] + 1).astype(np.int32)
    for cos_norm, r in ((False, None), (True, restrict)):
        h = sparse_handle(G, None, 0)
        h.add_batch(sp.csc_matrix(x), lab.astype(np.int32), 7, r, cos_norm)
        got = h.centroids(0)
        h.close()
        y = x / np.maximum(ref.cosine_l2(x), 1e-8) if cos_norm else x
        want, _ = ref.compute_centroids(y, lab, r)
        err = rel(got, want)
        print(f"sparse centroids 500 x 3000 cos_norm={cos_norm}: max rel err {err:.3e}")
        assert err < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# determinism
# ---------------------------------------------------------------------------------------------------------------------
def test_two_runs_and_a_blocked_upload_are_bitwise_equal(handles):
    """Blocks of 777 cells (no multiple of the 256-cell chunk); the second block's cells are all empty: it brings no entry."""
    _, sparse_handle = handles
    rng = np.random.default_rng(11)
    G, n, C, d = 300, 3000, 4, 20
    x = sparse_values(rng, G, n)
    x[:, 777:1554] = 0.0
    c = sp.csc_matrix(x)
    assert c.indptr[777] == c.indptr[1554]
    lab = (np.arange(n) % C).astype(np.int32)
    rotation = np.linalg.qr(rng.normal(size=(G, d)))[0]
    centers = rng.normal(size=G) * 0.1
    cp = rng.normal(size=(C, d))
    corr = cp + rng.normal(size=cp.shape) * 0.3
    outs = []
    for block_cells in (None, None, 777):
        h = sparse_handle(G, None, 0)
        h.add_batch(c, lab, C, None, True, block_cells=block_cells)
        cen = h.centroids(0)
        out, sigma = h.propagate(0, rotation, centers, cp, corr)
        h.close()
        outs.append((cen, out, sigma))
    runs = all(np.array_equal(a, b) for a, b in zip(outs[0], outs[1]))
    blocks = all(np.array_equal(a, b) for a, b in zip(outs[0], outs[2]))
    print(f"sparse handle: two runs bitwise equal {runs}; blocks of 777 cells bitwise equal to one block {blocks}")
    assert runs and blocks


# ---------------------------------------------------------------------------------------------------------------------
# projection and propagation on their own
# ---------------------------------------------------------------------------------------------------------------------
def run_propagation(handle, c, lab, C, rotation, centers, cp, corr, restrict=None, cos_norm=False, subset=None):
    h = handle(c.shape[0], subset, 0)
    h.add_batch(c, lab.astype(np.int32), C, restrict, cos_norm)
    cur, _ = h.propagate(0, rotation, centers, cp, cp)  # zero deltas: the device's own projection
    out, sigma = h.propagate(0, rotation, centers, cp, corr)
    h.close()
    return out, sigma, cur


@pytest.mark.parametrize("d,cos_norm,restricted,subset", [(1, False, False, False), (63, True, False, True),
                                                          (64, True, True, False), (65, False, True, True),
                                                          (256, True, False, True), (256, False, False, False)])
def test_projection_and_propagation_against_restatement(handles, d, cos_norm, restricted, subset):
    """Cells with 0, 1, 3, 4, 5, 63, 64, 65 and 129 stored entries (the gather takes 64 entries at a time, four in flight),
    the others at density 0.3; subset_row a list in no order that is no prefix."""
    _, sparse_handle = handles
    rng = np.random.default_rng(1000 + d)
    G, n, C = 400, 700, d + 1
    x = sparse_values(rng, G, n)
    counts = [0, 1, 3, 4, 5, 63, 64, 65, 129]
    for cell, m in enumerate(counts):
        x[:, cell] = 0.0
        x[rng.choice(G, size=m, replace=False), cell] = rng.normal(size=m) + 2.0
    c = sp.csc_matrix(x)
    assert np.diff(c.indptr)[:len(counts)].tolist() == counts
    sub = (rng.permutation(np.arange(20, G))[:max(d, 2 * G // 3)] + 1).astype(np.int32) if subset else None
    rows = G if sub is None else sub.size
    rotation = np.linalg.qr(rng.normal(size=(rows, d)))[0]
    centers = rng.normal(size=rows) * 0.1
    lab = np.arange(n) % C
    restrict = None
    if restricted:
        restrict = np.union1d(rng.choice(n, size=n // 2, replace=False) + 1, np.arange(1, C + 1)).astype(np.int32)
    l2 = ref.cosine_l2(x, sub) if cos_norm else None
    y = x if sub is None else x[sub - 1]
    y = y / np.maximum(l2, 1e-8) if cos_norm else y
    proj = y.T @ rotation - centers @ rotation
    cp = np.stack([proj[lab == cl].mean(0) for cl in range(C)])
    corr = cp + rng.normal(size=cp.shape) * 0.3
    out, sigma, cur = run_propagation(sparse_handle, c, lab, C, rotation, centers, cp, corr, restrict, cos_norm, sub)
    want, want_sigma, want_cur = ref.propagate_to_cells(x, rotation, centers, cp, corr, restrict, sub, l2)
    e_cur, e_sigma, e_out = rel(cur, want_cur), abs(sigma - want_sigma) / want_sigma, rel(out, want)
    print(f"sparse propagation d={d} cos_norm={cos_norm} restricted={restricted} subset={subset}: projection rel "
          f"{e_cur:.3e}; sigma rel {e_sigma:.3e}; smoothed rel {e_out:.3e}")
    assert e_cur < 1e-5
    assert e_sigma < 1e-5
    assert e_out < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
def sparse_mock(form=sp.csc_matrix, density=0.35, **kw):
    """mock_batches with the values outside a random pattern set to zero: (sparse batches, the same dense, clusters)."""
    batches, clusters = mock_batches(**kw)
    rng = np.random.default_rng(77)
    dense = [b * (rng.random(b.shape) < density) for b in batches]
    return [form(b) for b in dense], dense, clusters


def same_call(out, want, rep, exact_pairs, what):
    """`out` (the sparse call) against the dense call or the restatement; rep: twin_representatives of the restatement."""
    err = rel(out.corrected @ out.rotation.T, want.corrected @ want.rotation.T)
    serr = float(np.abs(out.sigma / want.sigma - 1).max())
    print(f"{what}: corrected @ rotation.T max rel err {err:.3e}; sigma max rel err {serr:.3e}; "
          f"pairs {[p[0].size for p in out.merge_info.pairs]}")
    assert err < 1e-5
    assert serr < 1e-5
    assert out.corrected.shape == want.corrected.shape and isinstance(out.corrected, np.ndarray)
    assert out.batch.tolist() == want.batch.tolist()
    assert out.cluster.tolist() == want.cluster.tolist()
    for col in ("cluster", "batch", "meta"):
        assert out.cluster_info[col].tolist() == want.cluster_info[col].tolist(), col
    assert out.merge_info.left == want.merge_info.left and out.merge_info.right == want.merge_info.right
    for (ol, orr), (wl, wr) in zip(out.merge_info.pairs, want.merge_info.pairs):
        assert ol.size == wl.size
        if exact_pairs:
            assert np.array_equal(ol, wl) and np.array_equal(orr, wr)
        mine = np.stack([rep[ol - 1], rep[orr - 1]], axis=1)
        theirs = np.stack([rep[wl - 1], rep[wr - 1]], axis=1)
        assert np.array_equal(mine[np.lexsort(mine.T[::-1])], theirs[np.lexsort(theirs.T[::-1])])


def both_ways(bx, sparse, dense, exact_pairs, what, **kw):
    out = bx.clusterMNN(*sparse, **kw)
    want = ref.cluster_mnn(*dense, **kw)
    rep = twin_representatives(want.merged.corrected)
    same_call(out, want, rep, exact_pairs, what + " against the restatement")
    same_call(out, bx.clusterMNN(*dense, **kw), rep, exact_pairs, what + " against the dense call")
    assert set(out.stats["stage_ms"]) == {"upload", "centroids", "projection", "nearest_median", "smoothing"}
    return out


def test_two_batches(bx):
    sparse, dense, clusters = sparse_mock()
    out = both_ways(bx, sparse, dense, True, "2 x 500 x 1000 sparse", clusters=clusters)
    assert out.corrected.shape == (1000, 19) and out.rotation.shape == (1000, 19)


def test_three_batches(bx):
    sparse, dense, clusters = sparse_mock(form=sp.csr_matrix, seed=3, n=(400, 650, 300), genes=600, nclust=9)
    both_ways(bx, sparse, dense, False, "3 batches sparse", clusters=clusters)


def test_restrict(bx):
    sparse, dense, (c1, c2) = sparse_mock(seed=8, n=(450, 520), genes=300)
    e1 = np.r_[np.arange(10), np.arange(450)]
    e2 = np.r_[np.arange(10), np.arange(520)]
    kw = dict(clusters=[c1[e1], c2[e2]], restrict=[np.arange(11, e1.size + 1), np.arange(11, e2.size + 1)])
    out = both_ways(bx, [sparse[0][:, e1], sparse[1][:, e2]], [dense[0][:, e1], dense[1][:, e2]], True, "restrict sparse", **kw)
    dup = np.r_[np.arange(10), 10 + 450 + np.arange(10)]
    assert np.array_equal(out.corrected[dup], out.corrected[dup + 10])


def test_subset_row_and_correct_all(bx):
    sparse, dense, clusters = sparse_mock(seed=7, n=(450, 520), genes=400)
    out = both_ways(bx, sparse, dense, True, "subset_row, correct_all sparse", clusters=clusters, subset_row=np.arange(11, 401),
                    correct_all=True)
    assert out.rotation.shape[0] == 400


@pytest.mark.parametrize("form", [sp.csc_matrix, sp.csr_array], ids=["csc_matrix", "csr_array"])
def test_single_object_shuffled_batch(bx, form):
    _, (b1, b2, b3), (c1, c2, c3) = sparse_mock(seed=9, n=(300, 420, 260), genes=300, nclust=6)
    perm = np.random.default_rng(9).permutation(980)
    x = np.hstack([b1, b2, b3])[:, perm]
    batch = np.repeat(["A", "M", "X"], [300, 420, 260])[perm]
    call = np.r_[c1, c2, c3][perm]
    out = both_ways(bx, [form(x)], [x], False, f"single object, shuffled, {form.__name__}", batch=batch, clusters=[call])
    assert out.batch.tolist() == batch.tolist()


# ---------------------------------------------------------------------------------------------------------------------
# clusters=KmeansParam(...)
# ---------------------------------------------------------------------------------------------------------------------
def blob_batches(seed, n, genes=200, npop=6, density=0.4):
    """Well-separated populations (means of scale 4 against noise of 1) on a random pattern of stored entries."""
    rng = np.random.default_rng(seed)
    means = rng.normal(scale=4.0, size=(genes, npop))
    out = []
    for b, nb in enumerate(n):
        lab = rng.integers(0, npop, nb)
        x = means[:, lab] + rng.normal(size=(genes, nb))
        if b:
            x = x + rng.normal(size=(genes, 1))
        out.append(x * (rng.random(x.shape) < density))
    return out


def partition(labels):
    """Labels renumbered by first occurrence: equal for equal partitions."""
    _, first, inverse = np.unique(labels, return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inverse]


@pytest.mark.parametrize("case", ["sparse_pca", "subset", "few_cells", "no_pca"])
def test_kmeans_param_gives_the_dense_call_s_partition(bx, case):
    from batchelor_amd.cluster_mnn import _batch_pcs
    from batchelor_amd.kmeans import start_indices
    sizes, kw, paths = (400, 520), {"cluster_d": 10}, ["device-sparse-pca", "device-sparse-pca"]
    if case == "subset":
        kw["subset_row"] = np.random.default_rng(4).choice(200, 120, replace=False) + 1
    elif case == "few_cells":   # 60 cells: not more than the PCA's block of 64, the subset rows are made dense
        sizes, paths = (60, 520), ["densified: host-svd", "device-sparse-pca"]
    elif case == "no_pca":      # kmeans takes dense observations
        kw, paths = {"cluster_d": None}, ["densified: none", "densified: none"]
    dense = blob_batches(7, sizes)
    param = bx.KmeansParam(centers=lambda n: 6 if n > 100 else 4, iter_max=30, seed=6)
    # the partition does not hang on the last bits of the PCs: a relative 1e-9 perturbation of the dense route's leaves it
    rng = np.random.default_rng(1)
    for m in dense:
        cur = m if "subset_row" not in kw else m[kw["subset_row"] - 1]
        obs = np.ascontiguousarray(cur.T) if kw["cluster_d"] is None else _batch_pcs(cur, kw["cluster_d"], 0)[0]
        idx = start_indices(obs.shape[0], param.n_centers(obs.shape[0]), 1, param.seed)[0]
        moved = obs * (1.0 + 1e-9 * rng.normal(size=obs.shape))
        a, b = kmeans_ref(obs, obs[idx], iter_max=param.iter_max), kmeans_ref(moved, moved[idx], iter_max=param.iter_max)
        print(f"{case}: batch of {m.shape[1]} cells, restatement margin {a.margin:.3g}")
        assert np.array_equal(a.cluster, b.cluster)
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message="did not converge")
        out = bx.clusterMNN(*[sp.csr_matrix(m) for m in dense], clusters=param, **kw)
        want = bx.clusterMNN(*dense, clusters=param, **kw)
    got_paths = [i["pca"] for i in out.stats["clustering"]]
    same = [bool(np.array_equal(partition(a), partition(b)))
            for a, b in zip(np.split(out.cluster, [sizes[0]]), np.split(want.cluster, [sizes[0]]))]
    print(f"{case}: paths {got_paths}; partitions equal to the dense call's {same}")
    assert got_paths == paths
    assert all(same)
    assert np.isfinite(out.corrected).all() and out.corrected.shape == want.corrected.shape


# ---------------------------------------------------------------------------------------------------------------------
# patterns only the device sees
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("indices,message", [([3, 1, 1, 2], "strictly ascending"),
                                             ([2, 2, 1, 2], "strictly ascending"),
                                             ([0, 5, 1, 2], "row index is outside"),
                                             ([0, -1, 1, 2], "row index is outside")])
def test_patterns_only_the_device_sees(bx, indices, message):
    """Through the C ABI, past canonical_csc: rows that do not ascend, a repeated row, a row equal to G and a row of -1 are
    reported by both passes -- the kernels leave such entries out, they never address memory with them --, the handle can be
    destroyed and the next ordinary call works."""
    from batchelor_amd import _lib
    L = _lib.lib()
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    L.bmx_cluster_sparse_destroy.argtypes = [ctypes.c_void_p]
    L.bmx_cluster_sparse_destroy.restype = None
    h = ctypes.c_void_p()
    _lib.check(L.bmx_cluster_sparse_create(i32(0), i32(5), None, i32(0), ctypes.byref(h)))
    try:
        indptr = np.array([0, 2, 3, 4], dtype=np.int64)
        idx = np.array(indices, dtype=np.int32)
        data = np.ones(4)
        ids = np.zeros(3, dtype=np.int32)
        _lib.check(L.bmx_cluster_sparse_begin_batch(h, i64(3), i64(4), _lib.i32p(ids), i32(1), None, i64(-1), i32(1)))
        _lib.check(L.bmx_cluster_sparse_add_block(h, i64(3), indptr.ctypes.data_as(_lib.c_i64p), _lib.i32p(idx),
                                                  _lib.f64p(data), i64(4)))
        out = np.full((5, 1), 7.0, order="F")
        rc = L.bmx_cluster_sparse_centroids(h, i32(0), _lib.f64p(out))
        text = L.bmx_last_error().decode()
        print(f"indices {indices}: centroids status {rc}, '{text}'")
        assert rc == -6 and message in text
        assert (out == 7.0).all()  # nothing was written
        rot, cen, cp = np.eye(5, 2, order="F"), np.zeros(5), np.zeros((1, 2), order="F")
        cells = np.full((3, 2), 7.0, order="F")
        rc = L.bmx_cluster_sparse_propagate(h, i32(0), _lib.f64p(rot), i32(2), _lib.f64p(cen), _lib.f64p(cp), _lib.f64p(cp),
                                            _lib.f64p(cells), None)
        assert rc == -6 and message in L.bmx_last_error().decode()
        assert (cells == 7.0).all()
    finally:
        L.bmx_cluster_sparse_destroy(h)
    (b1, b2), dense, clusters = sparse_mock(n=(60, 70), genes=30)
    out = bx.clusterMNN(b1, b2, clusters=clusters)
    assert rel(out.corrected @ out.rotation.T, (lambda w: w.corrected @ w.rotation.T)(ref.cluster_mnn(*dense, clusters=clusters))) < 1e-5
